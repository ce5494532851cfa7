"""Inputs built for every form and instantiation of K1, the log-likelihood kernels (csrc/khg_k1.hip), and their yardstick.

A case names its options, its model (D and the Gaussians of every pdf), its set (utterance lengths with ONE shared pdf list, or
hand-built chain graphs whose pdf lists, first and last needed frames follow from the graphs), the call (all cells, from the first
needed tile on, the band) and the exact record UtteranceSet.k1_last() must report after it: which form ran, which one was asked
for, why earlier forms handed over, and the plan -- pdfs per tile, persistent or not, workgroups, work units and their cap, chunk
order, shifted tiles, the fp32 forms' tile counts, the pdf-major slices per block count, what was packed.

`restate` derives that record from the shapes alone -- D -> KS / KQ, the largest pdf -> packing and the 128-Gaussian limit of the
pdf-major form, `small` (csrc/khg_utts.hip), plan_x32_chunks with the empty chunks of order 4, the chunk split of the utterance-major
form, the slice planner of the pdf-major form -- and, in numpy on the case's own arrays, the three domain decisions of the split forms:
k1_split_domain, the scales of f16x2s (common scale and the absolute part of its error bound) and k1h_balance / k1h_fits of f16x2.
The weight columns are those of k0_model_stats (csrc/khg_ctx_model.hip): max |mean x inverse variance| and half the largest inverse
variance per dimension, and the largest |gconst|.  tests/test_k1_form_cases_cpu.py holds every case's stated record to the
restatement, so a case that claims "f16x2s declines, f16x2 accepts" is checked before a device sees it.

The yardstick is helpers.exact_loglikes: the float64 evaluation and the magnitude bound B that fp32 rounding scales with; the
tolerance is the project's, |got - exact| <= 1e-5 + 1e-6 B (x D / 80 above D = 80, as tests/test_gpu_wide.py).  The CPU test holds
the oracle's fp32 chain to it on every case.

Chain graphs: a main chain of states with a self-loop and a forward arc each (the pdf of state s is first needed at frame s, last
needed at s + slack), an arc into a dead end (a pdf no accepting path reads: last = -1), and a spur of L arcs without self-loops
from the start state whose last arc carries a pdf into the final state (first = L, at or past the utterance's end)."""
import functools
from dataclasses import dataclass

import numpy as np

from graph_frames import first_frames, last_frames
from helpers import exact_loglikes
from kaldi_hmm_gmm_amd import synth
from oracle import oracle as orc

LL_ATOL, LL_RTOL = 1e-5, 1e-6          # tests/test_gpu_parity.py
NMAX = {5: 15, 10: 7}                  # k1s_nmax: 32-frame tiles per f16x2s chunk
K1P_MAXENT = 256                       # entries per pdf-major slice
NEVER = 10**9


def ks_of(D):
    return 5 if D <= 40 else 10


def kq_of(D):
    return 10 if D <= 40 else 20 if D <= 80 else 0


def tolerance(bound, D):
    return (LL_ATOL + LL_RTOL * bound) * max(1.0, D / 80.0)


# ---- the records ------------------------------------------------------------------------------------------------------------------
ZERO = dict(form="none", asked="f16x2s", declined=0, K=0, mode=0, pack=0, persistent=0, grid=0, chunks=0, per=0, order=0, tail_shift=0,
            shift_mode=0, nf=0, aligned=0, interleave=0, nb_slices=(0,) * 8, repacked=0, repaired=0)


def _rec(base, kw):
    d = dict(ZERO)
    d.update(base)
    d.update(kw)
    assert set(d) == set(ZERO), sorted(set(d) - set(ZERO))
    d["nb_slices"] = list(d["nb_slices"])
    return d


def S(K, chunks, per, **kw):
    """f16x2s: one pdf per tile, one workgroup per chunk, the planes and the image packed by this call, unless said otherwise"""
    return _rec(dict(form="f16x2s", K=K, pack=1, grid=chunks, chunks=chunks, per=per, shift_mode=2, repacked=3), kw)


def H(K, chunks, **kw):
    return _rec(dict(form="f16x2", asked="f16x2", K=K, grid=chunks, chunks=chunks, per=16, repacked=3), kw)


def Pm(K, nb_slices, per=1024, **kw):
    n = sum(nb_slices)
    return _rec(dict(form="pdf", asked="pdf", K=K, grid=n, chunks=n, per=per, nb_slices=tuple(nb_slices), repacked=1), kw)


def U(K, chunks, nf, aligned, **kw):
    return _rec(dict(form="utt", asked="utt", K=K, grid=chunks, chunks=chunks, per=4 * nf, nf=nf, aligned=aligned), kw)


def W(chunks, **kw):
    return _rec(dict(form="wide", grid=chunks, chunks=chunks, per=64), kw)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Chain:
    pdf_at: tuple           # the pdf of main-chain state s (self-loop and forward arc); the state behind the last one is final
    slack: int              # T = len(pdf_at) + slack: the pdf of state s is needed in frames s .. s + slack
    dead: tuple = ()        # ((state, pdf), ...): an arc from a main-chain state into a dead end
    late: tuple = ()        # ((L, fill pdf, pdf), ...): L arcs of the fill pdf from the start state, then `pdf` into the final state

    @property
    def T(self):
        return len(self.pdf_at) + self.slack


def _tids(p):
    return 2 * p + 1, 2 * p + 2      # self-loop, forward (ID2PDF below)


def id2pdf_of(P):
    tid = np.arange(2 * P + 1)
    return np.where(tid > 0, (tid - 1) // 2, 0).astype(np.int32)


def build_graphs(chains):
    """CSR dict of the set (state_off, arc_off, start, ilabel, olabel, weight, nextstate, final) from the chains"""
    state_off, arc_off, il, ns, fin = [0], [0], [], [], []
    for c in chains:
        n = len(c.pdf_at)
        arcs = [[] for _ in range(n + 1)]          # main chain: states 0 .. n, n final
        for s, p in enumerate(c.pdf_at):
            arcs[s] += [(_tids(p)[0], s), (_tids(p)[1], s + 1)]
        for s, p in c.dead:
            arcs.append([])
            arcs[s].append((_tids(p)[1], len(arcs) - 1))
        for L, pf, p in c.late:
            cur = 0
            for _ in range(L):
                arcs.append([])
                arcs[cur].append((_tids(pf)[1], len(arcs) - 1))
                cur = len(arcs) - 1
            arcs[cur].append((_tids(p)[1], n))
        f = np.full(len(arcs), np.inf, np.float32)
        f[n] = 0.0
        fin.append(f)
        for a in arcs:
            il += [t for t, _ in a]
            ns += [d for _, d in a]
            arc_off.append(len(il))
        state_off.append(state_off[-1] + len(arcs))
    return {"state_off": np.array(state_off, np.int64), "arc_off": np.array(arc_off, np.int64), "start": np.zeros(len(chains), np.int32),
            "ilabel": np.array(il, np.int32), "olabel": np.zeros(len(il), np.int32), "weight": np.zeros(len(il), np.float32),
            "nextstate": np.array(ns, np.int32), "final": np.concatenate(fin)}


def _chain_a():
    at = [8] * 39
    for s, p in ((0, 0), (1, 1), (15, 2), (16, 3), (17, 4), (31, 5), (32, 6), (33, 7)):
        at[s] = p
    return at


# A: T = 70 (three 32-frame tiles).  First needed frames 0, 1, 15, 16, 17, 31, 32, 33; with slack 31 the bands are [0, 31] and
# [32, 63] (inside one tile: no shift) and [1, 32], [15, 46], [16, 47], [17, 48], [31, 62], [33, 64]: each ends earlier inside its
# tile than it starts -- shifts 1, 15, 16, 17, 31 and 1 again.  pdf 9 is read by no accepting path, pdf 10 first at frame 100 > T.
CH_A = Chain(tuple(_chain_a()), 31, dead=((3, 9),), late=((100, 8, 10),))
# B: the same heads with pdf 10 at state 5 and thirty more states: T = 100, four tiles
CH_B = Chain(tuple(_chain_a()[:5] + [10] + _chain_a()[6:] + [8] * 30), 31, dead=((3, 9),))
CH_EMPTY = Chain((), 40)               # one state, start and final, no arc: 40 frames and an empty pdf list
CH_ZERO = Chain((0,), -1)              # a graph, but no frame


def _chain_long():
    at = [8] * 8196
    for s, p in ((0, 0), (2050, 1), (8161, 2), (8195, 3)):
        at[s] = p
    return at


# one utterance of 8 200 frames: pdfs first needed at 2 050 (past the 127 x 16-frame clamp of f16x2 and the utterance-major form),
# at 8 161 (tile 255, the f16x2s clamp's own value) and at 8 195 (tile 256: clamped)
CH_LONG = Chain(tuple(_chain_long()), 4)


def _chain_p(n):
    at = [8] * n
    for s, p in ((0, 0), (1, 1), (15, 2), (16, 3), (33, 4), (40, 5), (64, 6), (65, 7)):
        at[s] = p
    return tuple(at)


# for the packed kernels, whose groups of 4 / 2 consecutive list entries start at the earliest first needed tile among them: the
# entries 4 .. 7 are first needed at 33, 40, 64, 65 (four per tile: tile 1; two per tile: tiles 1 and 2), pdf 10 -- alone in the last
# group of two -- past the utterance's end.  T = 100 and 130.
CH_PA = Chain(_chain_p(69), 31, dead=((3, 9),), late=((130, 8, 10),))
CH_PB = Chain(_chain_p(99), 31, dead=((3, 9),))


def _chain_long_p():
    at = [3] * 8196
    for s, p in ((0, 0), (1, 1), (2, 2), (2050, 4), (4000, 5), (8161, 6), (8190, 7), (8195, 8)):
        at[s] = p
    return tuple(at)


# ... and 8 200 frames: list entries 4 .. 7 first needed at 2 050 or later (tile 64), entry 8 at 8 195 (tile 256: clamped to 255)
CH_LONG_P = Chain(_chain_long_p(), 4)
G4 = (CH_B, CH_A, CH_B, CH_A)          # pdf 10's entries of the pdf-major plan: tiles, none, tiles, none
G17 = (CH_A, CH_B) * 8 + (CH_A,)
GE = (CH_A, CH_EMPTY, CH_ZERO, CH_B)
GL = (CH_LONG,)
GP4S = (CH_PB, CH_PA, CH_PB, CH_PA)
GP17 = (CH_PA, CH_PB) * 8 + (CH_PA,)
GPE = (CH_PA, CH_EMPTY, CH_ZERO, CH_PB)
GPL = (CH_LONG_P,)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Case:
    name: str
    D: int
    gauss: tuple            # Gaussians of every pdf of the model
    expect: dict            # the k1_last() record
    lens: tuple = ()        # features-only set: utterance lengths ...
    plist: tuple = ()       # ... and the shared pdf list
    graphs: tuple = ()      # or: one Chain per utterance
    call: str = "full"      # "full" | "reach" | "band"
    k1: str = "auto"        # the k1_form option
    opts: tuple = ()        # ((option, value), ...)
    rescale: float = 0.0    # the model's dimension 5 in units this much smaller (tests/test_gpu_parity.py: _rescaled on the model only)
    bitwise: bool = False   # one Gaussian per pdf and an fp32 form: equal to the oracle's k-ordered fmaf chain bit for bit


CASES = []


def C(name, D, gauss, expect, **kw):
    opts = tuple(sorted((k, kw.pop(k)) for k in list(kw) if k.startswith("k1_") or k == "k1p_ts"))
    CASES.append(Case(name, D, tuple(gauss), expect, opts=opts, **kw))


# Gaussian counts: one to five 32-Gaussian W tiles per pdf -- one to three passes of two tiles (KS 5), one to five of one (KS 10)
GA = (17, 32, 33, 64, 65, 96, 97, 128, 129, 40, 50, 20)
GC = (129, 65, 17, 97, 33, 128, 64, 96, 32, 40, 50, 20)          # the graphs' pdfs: 0 .. 7 heads, 8 fill, 9 dead, 10 late
GCP = (128, 65, 17, 97, 33, 113, 64, 96, 32, 40, 50, 20)         # ... for the pdf-major form (<= 128)
GP4 = (1, 8, 3, 8, 1, 5, 8, 2, 8, 1, 7, 8)                       # four pdfs per tile
GP2A = (9, 16, 12, 16, 9, 10, 16, 11, 16, 9, 13, 16)             # two
GP2B = (1, 16, 3, 8, 1, 16, 8, 2, 9, 1, 7, 16)
GP1 = (1, 8, 3, 8, 17, 5, 8, 2, 8, 1, 7, 8)                      # one pdf of 17: no packing
GH = (32, 33, 64, 65, 32, 33, 64, 65, 1, 17, 128, 129)
GPD = (1, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)      # both ends of 1 .. 8 blocks of sixteen
G1 = (1,) * 16
# 17 utterances (no small set): 1, 1, 1, 2, 2, 3, 3, 5, 7, 8, 8, 15, 15, 16, 16, 2, 3 tiles
LENS17 = (1, 31, 32, 33, 64, 65, 96, 160, 224, 225, 256, 449, 480, 481, 500, 40, 70)
LENS17Z = LENS17[:15] + (0, 70)
LENSH = (32, 221, 256, 283, 480, 511, 537)                       # 1, 7, 8, 9, 15, 16, 17 tiles: f16x2 cuts at 16
LENSP = (1, 16, 17, 100)
LENSU6 = tuple(16 * n - (0 if i % 2 == 0 else 5) for i, n in enumerate((1, 2, 3, 4, 5, 6, 7, 23, 24, 25)))      # 4 NF - 1, 4 NF, 4 NF + 1 at NF = 6
LENSU5 = tuple(16 * n - (0 if i % 2 == 0 else 5) for i, n in enumerate((1, 2, 3, 4, 5, 6, 7, 19, 20, 21)))      # ... at NF = 5
LENS300 = tuple(1 + i % 16 for i in range(300))

# ---- f16x2s, one pdf per tile: list lengths 1, 2, 3, 8, 9; 1, 2, 3, 5, NMAX, NMAX + 1 tiles; small sets, persistent sets, order 4
for D in (40, 39, 41, 80):
    K, N = ks_of(D), NMAX[ks_of(D)]
    C(f"s{D}_one", D, GA, S(K, 1, 3), lens=(1,), plist=(8,))
    C(f"s{D}_two", D, GA, S(K, 3, 3), lens=(31, 160), plist=(8, 0))
    C(f"s{D}_three", D, GA, S(K, 4, N), lens=(65, 32 * N, 32 * N + 1), plist=(7, 1, 4))
C("s40_17", 40, GA, S(5, 19, 15, persistent=1), lens=LENS17, plist=tuple(range(8)))
C("s39_17z", 39, GA, S(5, 18, 15, persistent=1), lens=LENS17Z, plist=tuple(range(9)))
# KS 10 chooses order 4 by itself: 4 utterances of 3 chunks, 2 of 2, 11 (10) of 1 -> bands of eight: 3 x 8 + 8 + 1 (3 x 8 + 8) work items
C("s41_17", 41, GA, S(10, 33, 7, persistent=1, order=4), lens=LENS17, plist=tuple(range(8)))
C("s80_17z", 80, GA, S(10, 32, 7, persistent=1, order=4), lens=LENS17Z, plist=tuple(range(9)))
for o in (1, 2, 3):
    C(f"s40_17_order{o}", 40, GA, S(5, 19, 15, persistent=1, order=o), lens=LENS17, plist=tuple(range(8)), k1_order=o)
C("s40_17_order4", 40, GA, S(5, 25, 15, persistent=1, order=4), lens=LENS17, plist=tuple(range(8)), k1_order=4)      # 2 x 8 + 8 + 1
C("s41_17_order1", 41, GA, S(10, 27, 7, persistent=1, order=1), lens=LENS17, plist=tuple(range(8)), k1_order=1)
C("s40_17_launch1", 40, GA, S(5, 19, 15), lens=LENS17, plist=tuple(range(8)), k1_launch=1)
C("s40_two_launch2", 40, GA, S(5, 3, 3, persistent=1), lens=(31, 160), plist=(8, 0), k1_launch=2)
# ---- cell modes on chain graphs
for D in (40, 41):
    K, N = ks_of(D), NMAX[ks_of(D)]
    C(f"s{D}_g4_full", D, GC, S(K, 4, N), graphs=G4)
    C(f"s{D}_g4_reach", D, GC, S(K, 4, N, mode=1, tail_shift=1), graphs=G4, call="reach")
    C(f"s{D}_g4_band", D, GC, S(K, 4, N, mode=2), graphs=G4, call="band")
C("s40_g4_band_dbg32", 40, GC, S(5, 4, 15, mode=2, shift_mode=0), graphs=G4, call="band", k1_dbg=32)
C("s40_g4_band_dbg64", 40, GC, S(5, 4, 15, mode=2, shift_mode=1), graphs=G4, call="band", k1_dbg=64)
C("s40_g4_reach_dbg32", 40, GC, S(5, 4, 15, mode=1, shift_mode=0), graphs=G4, call="reach", k1_dbg=32)
C("s40_g4_reach_dbg64", 40, GC, S(5, 4, 15, mode=1, tail_shift=1, shift_mode=1), graphs=G4, call="reach", k1_dbg=64)
C("s40_g17_band", 40, GC, S(5, 17, 15, mode=2, persistent=1), graphs=G17, call="band")
C("s41_g17_reach", 41, GC, S(10, 17, 7, mode=1, tail_shift=1, persistent=1, order=4), graphs=G17, call="reach")
C("s40_ge_band", 40, GC, S(5, 2, 15, mode=2), graphs=GE, call="band")            # an empty pdf list and an utterance without frames
C("s41_ge_reach", 41, GC, S(10, 2, 7, mode=1, tail_shift=1), graphs=GE, call="reach")
C("s40_long_reach", 40, GC, S(5, 86, 3, mode=1, tail_shift=1), graphs=GL, call="reach")      # 257 tiles in chunks of 3
C("s40_long_band", 40, GC, S(5, 86, 3, mode=2), graphs=GL, call="band")
# ---- packed: 4 / 2 pdfs per tile (KS 5 only), groups partly filled (lists of 1 .. 5), 1, NMAX, NMAX + 1 tiles
C("pk4_d40", 40, GP4, S(5, 6, 15, pack=4), lens=(32, 480, 481, 7, 100), plist=(0, 1, 2, 3, 4))
C("pk4_d13_one", 13, GP4, S(5, 6, 3, pack=4), lens=(481,), plist=(1,))
C("pk4_d39", 39, GP4, S(5, 4, 15, pack=4), lens=(1, 480, 512), plist=(0, 1, 2))
C("pk4_d40_17", 40, GP4, S(5, 19, 15, pack=4), lens=LENS17, plist=(0, 1, 2, 3, 4, 5))
C("pk2_d40", 40, GP2A, S(5, 4, 15, pack=2), lens=(32, 480, 481), plist=(0, 1))
C("pk2_d39", 39, GP2B, S(5, 4, 15, pack=2), lens=(1, 480, 512), plist=(0, 1, 2, 3))
C("pk2_d13", 13, GP2A, S(5, 6, 15, pack=2), lens=(32, 480, 481, 7, 100), plist=(0, 1, 2, 3, 4))
C("pk1_d40_one17", 40, GP1, S(5, 4, 15), lens=(32, 480, 481), plist=(3, 4, 5))
C("pk1_d40_dbg16", 40, GP4, S(5, 6, 15), lens=(32, 480, 481, 7, 100), plist=(0, 1, 2, 3, 4), k1_dbg=16)
C("pk1_d41", 41, GP4, S(10, 4, 7), lens=(32, 224, 225), plist=(0, 1, 2, 3, 4))
# mono training's calls: the packed kernels from the first needed tile on; they keep the front-only form under band = True
C("pk4_d40_g4_reach", 40, GP4, S(5, 4, 15, pack=4, mode=1), graphs=GP4S, call="reach")
C("pk4_d40_g4_band", 40, GP4, S(5, 4, 15, pack=4, mode=1), graphs=GP4S, call="band")
C("pk4_d13_g17_band", 13, GP4, S(5, 17, 15, pack=4, mode=1), graphs=GP17, call="band")
C("pk2_d39_g4_reach", 39, GP2A, S(5, 4, 15, pack=2, mode=1), graphs=GP4S, call="reach")
C("pk2_d39_ge_band", 39, GP2A, S(5, 2, 15, pack=2, mode=1), graphs=GPE, call="band")
C("pk4_d40_long_reach", 40, GP4, S(5, 86, 3, pack=4, mode=1), graphs=GPL, call="reach")
# ---- f16x2, forced: 1, 7, 8, 9, 15, 16, 17 tiles (one chunk up to 16); 32 / 33 / 64 / 65 Gaussians
for D in (40, 39, 41, 80):
    C(f"h{D}", D, GH, H(ks_of(D), 8), lens=LENSH, plist=tuple(range(12)), k1="f16x2")
C("h40_dbg8", 40, GH, H(5, 8), lens=LENSH, plist=tuple(range(12)), k1="f16x2", k1_dbg=8)
C("h40_g4_reach", 40, GC, H(5, 4, mode=1), graphs=G4, call="reach", k1="f16x2")
C("h41_g4_band", 41, GC, H(10, 4, mode=1), graphs=G4, call="band", k1="f16x2")
C("h40_long_reach", 40, GC, H(5, 17, mode=1), graphs=GL, call="reach", k1="f16x2")       # 257 tiles in chunks of <= 16
C("h40_auto", 40, GH, H(5, 8, asked="f16x2s", declined=2), lens=LENSH, plist=tuple(range(12)), rescale=1e-3)
# ---- pdf-major: every block count 1 .. 8 at both ends, slices of 1 / 3 / 1024 tiles, 256 entries, a 263-tile slice
for D in (40, 39, 80, 77):
    C(f"p{D}", D, GPD, Pm(kq_of(D), [2] * 8), lens=LENSP, plist=tuple(range(16)), k1="pdf")
C("p40_ts1", 40, GPD, Pm(10, [22] * 8, per=1), lens=LENSP, plist=tuple(range(16)), k1="pdf", k1p_ts=1)       # 1 + 1 + 2 + 7 tiles per pdf
C("p40_ts3", 40, GPD, Pm(10, [8] * 8, per=3), lens=LENSP, plist=tuple(range(16)), k1="pdf", k1p_ts=3)        # ... in four slices: entries split
C("p77_ts3", 77, GPD, Pm(20, [8] * 8, per=3), lens=LENSP, plist=tuple(range(16)), k1="pdf", k1p_ts=3)
C("p40_300", 40, GPD, Pm(10, [4] * 8), lens=LENS300, plist=tuple(range(16)), k1="pdf")                      # 300 one-tile entries: 256 + 44
C("p39_4200", 39, GPD, Pm(10, [2] * 8), lens=(4200,), plist=tuple(range(16)), k1="pdf")                     # 263 tiles in one slice
C("p40_auto", 40, GPD, Pm(10, [2] * 8, asked="f16x2s", declined=1), lens=LENSP, plist=tuple(range(16)), rescale=1e-6)
C("p40_g4_reach", 40, GCP, Pm(10, [0, 2, 2, 2, 1, 1, 1, 2], mode=1), graphs=G4, call="reach", k1="pdf")
C("p40_ge_reach", 40, GCP, Pm(10, [0, 2, 2, 2, 1, 1, 1, 2], mode=1), graphs=GE, call="reach", k1="pdf")
C("p40_long_reach", 40, GCP, Pm(10, [0, 2, 0, 0, 1, 0, 1, 1], mode=1), graphs=GL, call="reach", k1="pdf")
C("p40_g1", 40, G1, Pm(10, [16, 0, 0, 0, 0, 0, 0, 0]), lens=LENSP, plist=tuple(range(16)), k1="pdf", bitwise=True)
C("p77_g1", 77, G1, Pm(20, [16, 0, 0, 0, 0, 0, 0, 0]), lens=LENSP, plist=tuple(range(16)), k1="pdf", bitwise=True)
# ---- utterance-major: NF 6 / 5 at KQ 10, KQ 20, aligned loads or not, 1 .. 7 and 4 NF - 1, 4 NF, 4 NF + 1 tiles, the deal of tiles
C("u40", 40, GA, U(10, 11, 6, 1), lens=LENSU6, plist=tuple(range(12)), k1="utt")
C("u39", 39, GA, U(10, 11, 6, 0), lens=LENSU6, plist=tuple(range(12)), k1="utt")
C("u40_nf5", 40, GA, U(10, 11, 5, 1), lens=LENSU5, plist=tuple(range(12)), k1="utt", k1_nf=5)
C("u13_nf5", 13, GA, U(10, 11, 5, 0), lens=LENSU5, plist=tuple(range(12)), k1="utt", k1_nf=5)
C("u80", 80, GA, U(20, 11, 5, 1), lens=LENSU5, plist=tuple(range(12)), k1="utt")
C("u77", 77, GA, U(20, 11, 5, 0), lens=LENSU5, plist=tuple(range(12)), k1="utt")
C("u40_il1", 40, GA, U(10, 11, 6, 1, interleave=1), lens=LENSU6, plist=tuple(range(12)), k1="utt", k1_interleave=1)
C("u40_g4_reach", 40, GC, U(10, 4, 6, 1, mode=1, interleave=1), graphs=G4, call="reach", k1="utt")
C("u40_g4_reach_il0", 40, GC, U(10, 4, 6, 1, mode=1), graphs=G4, call="reach", k1="utt", k1_interleave=0)
C("u77_ge_reach", 77, GC, U(20, 2, 5, 0, mode=1, interleave=1), graphs=GE, call="reach", k1="utt")
C("u40_long_reach", 40, GC, U(10, 22, 6, 1, mode=1, interleave=1), graphs=GL, call="reach", k1="utt")      # 513 tiles in 22 chunks of 24
C("u77_walk70", 77, tuple(33 + (7 * i) % 32 for i in range(70)), U(20, 2, 5, 0), lens=(40, 17), plist=tuple(range(70)), k1="utt")     # 140 W tiles: three blocks of 64
C("u40_auto", 40, GA, U(10, 11, 6, 1, asked="f16x2s", declined=1 | 8), lens=LENSU6, plist=tuple(range(12)), rescale=1e-6)
C("u40_from_pdf", 40, GA, U(10, 11, 6, 1, asked="pdf", declined=8), lens=LENSU6, plist=tuple(range(12)), k1="pdf")
C("u40_g1", 40, G1, U(10, 4, 6, 1), lens=LENSP, plist=tuple(range(16)), k1="utt", bitwise=True)
C("u40_g1_nf5_il1", 40, G1, U(10, 4, 5, 1, interleave=1), lens=LENSP, plist=tuple(range(16)), k1="utt", bitwise=True, k1_nf=5, k1_interleave=1)
C("u39_g1_il0", 39, G1, U(10, 4, 6, 0), lens=LENSP, plist=tuple(range(16)), k1="utt", bitwise=True, k1_interleave=0)
C("u77_g1", 77, G1, U(20, 4, 5, 0), lens=LENSP, plist=tuple(range(16)), k1="utt", bitwise=True)
# ---- D > 80: one form, whatever was asked for; and nothing to do
C("w81", 81, GA, W(7), lens=(1, 64, 65, 130), plist=tuple(range(12)))
C("w81_asked_utt", 81, GA, W(7, asked="utt"), lens=(1, 64, 65, 130), plist=(8,), k1="utt")
C("none_d40", 40, GA, _rec({}, {}), lens=(0, 0), plist=(0, 1))
C("none_ge", 40, GC, _rec({}, dict(asked="pdf", mode=1)), graphs=(CH_EMPTY,), call="reach", k1="pdf")      # frames, but no pdf

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- building a case --------------------------------------------------------------------------------------------------------------
@dataclass(eq=False)
class Built:
    case: Case
    m: object               # synth.SynthModel
    gc: np.ndarray
    frame_off: np.ndarray
    feats: np.ndarray
    graphs: object          # CSR dict or None
    id2pdf: np.ndarray
    lists: list             # per utterance: the listed pdfs, ascending for graphs
    first: list             # per utterance: {pdf: first needed frame} (all 0 without graphs)
    last: list              # per utterance: {pdf: last needed frame}  (T - 1 without graphs)
    exact: list             # per utterance: float64 scores [listed pdf, frame] ...
    bound: list             # ... and the magnitude bound B


def rescaled_model(m, dim, factor):
    """tests/test_gpu_parity.py's _rescaled, for the model alone: dimension `dim` in units `factor` times smaller"""
    import dataclasses
    s = np.ones(m.means.shape[1], np.float32)
    s[dim] = factor
    means = (m.means * s).astype(np.float32)
    inv_vars = (m.inv_vars / (s * s)).astype(np.float32)
    return dataclasses.replace(m, means=means, inv_vars=inv_vars, means_invvars=(means * inv_vars).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _model(D, gauss, rescale):
    m = synth.make_model(len(gauss), 0, D, seed=7000 + 13 * D + len(gauss) + sum(gauss), mean_scale=1.0, gauss_counts=gauss)
    if rescale:
        m = rescaled_model(m, 5, rescale)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    return m, gc


@functools.lru_cache(maxsize=8)
def build(name):
    c = BY_NAME[name]
    m0, _ = _model(c.D, c.gauss, 0.0)
    m, gc = _model(c.D, c.gauss, c.rescale)
    P = len(c.gauss)
    id2pdf = id2pdf_of(P)
    if c.graphs:
        lens = [ch.T for ch in c.graphs]
        graphs = build_graphs(c.graphs)
        lists = []
        for u in range(len(lens)):
            a0, a1 = int(graphs["arc_off"][graphs["state_off"][u]]), int(graphs["arc_off"][graphs["state_off"][u + 1]])
            lists.append(np.unique(id2pdf[graphs["ilabel"][a0:a1]]).astype(np.int32))
        first = [first_frames(graphs, u, id2pdf, lists[u]) for u in range(len(lens))]
        last = [last_frames(graphs, u, id2pdf, lists[u], lens[u]) for u in range(len(lens))]
    else:
        lens, graphs = list(c.lens), None
        lists = [np.array(c.plist, np.int32)] * len(lens)
        first = [{int(p): 0 for p in c.plist}] * len(lens)
        last = [{int(p): T - 1 for p in c.plist} for T in lens]
    frame_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(len(name) + 31 * c.D + int(frame_off[-1]))
    # every frame drawn from a component of one of its utterance's listed pdfs (of the model in its own units)
    frame_pdf = np.concatenate([rng.choice(lists[u] if len(lists[u]) else np.array([0]), size=lens[u]) for u in range(len(lens))] + [np.zeros(0, np.int64)])
    feats = synth.sample_feats(m0, frame_pdf.astype(np.int64), rng) if len(frame_pdf) else np.zeros((0, c.D), np.float32)
    exact, bound = [], []
    for u in range(len(lens)):
        e, b = exact_loglikes(m, gc, feats[frame_off[u]: frame_off[u + 1]], lists[u])
        exact.append(e); bound.append(b)
    for a in (feats, frame_off, gc):
        a.setflags(write=False)
    return Built(c, m, gc, frame_off, feats, graphs, id2pdf, lists, first, last, exact, bound)


# ---- the restatement of the selection and planning rules --------------------------------------------------------------------------
FORM_OPT = {"auto": "f16x2s", "f16x2s": "f16x2s", "f16x2": "f16x2", "pdf": "pdf", "utt": "utt"}


def _ilogb(x):
    return int(np.frexp(np.float32(x))[1]) - 1


def column_maxima(m, gc, feats, K):
    """xk, wk [K] and gcmax: k1_maxima / model_stats (k = 2 d: the linear term, 2 d + 1: the quadratic one), fp32 as there"""
    D = feats.shape[1]
    xmax = np.abs(feats).max(0).astype(np.float32) if len(feats) else np.zeros(D, np.float32)
    xk, wk = np.zeros(K, np.float32), np.zeros(K, np.float32)
    xk[0:2 * D:2], xk[1:2 * D:2] = xmax, xmax * xmax
    wk[0:2 * D:2] = np.abs(m.means_invvars).max(0)
    wk[1:2 * D:2] = np.float32(0.5) * m.inv_vars.max(0)
    return xk, wk, np.float32(np.abs(gc).max())


def split_domain(xk, wk, gcmax):
    return float(gcmax) + float((wk.astype(np.float64) * xk.astype(np.float64)).sum()) <= 268435456.0


def f16x2s_scales(xk, wk):
    """the scales() lambda of k1_plan_f16x2s for a model that has scored no other set"""
    ex = [14 - _ilogb(v) if v > 0 else 0 for v in xk]
    cand = [14 - _ilogb(w) + e for w, e in zip(wk, ex) if w > 0]
    Sc = min(cand) if cand else 0
    if Sc < -100 or Sc > 100:
        return False
    floor_sum = sum(np.ldexp(float(w), Sc - e) + np.ldexp(float(x), e) for w, x, e in zip(wk, xk, ex))
    return bool(np.ldexp(floor_sum, -25 - Sc) <= 2.0e-6)


def k1h_fits(xk, wk):
    """k1h_balance, then k1h_fits with those exponents"""
    for x, w in zip(xk.astype(np.float64), wk.astype(np.float64)):
        hx, hw = x > 0 and np.isfinite(x), w > 0 and np.isfinite(w)
        e = 0.5 * (np.log2(w) - np.log2(x)) if hx and hw else -np.log2(x) if hx else np.log2(w) if hw else 0.0
        e = int(np.rint(min(120.0, max(-120.0, e))))
        if not (np.ldexp(np.float32(x), e) <= 32768.0) or not (np.ldexp(np.float32(w), -e) <= 32768.0):
            return False
    return True


def is_small(n_utt, N, D, graphs):
    small_graphs = graphs is None or (int(graphs["state_off"][-1]) <= 32768 and len(graphs["ilabel"]) <= 65536)
    return n_utt <= 16 and N <= 16384 and N * D <= (512 << 10) and small_graphs


def x32_chunks(lens, nlist, per, order):
    """plan_x32_chunks: (utterance, first tile, tiles) in launch order; order 4 adds empty items (tiles = 0)"""
    ch = []
    for u, T in enumerate(lens):
        n32 = (T + 31) // 32
        if nlist[u] == 0:
            continue
        nch = (n32 + per - 1) // per
        for c in range(nch):
            t0, t1 = n32 * c // nch, n32 * (c + 1) // nch
            if t1 > t0:
                ch.append((u, t0, t1 - t0))
    if order == 4:
        groups = []
        for c in ch:
            if groups and groups[-1][0][0] == c[0]:
                groups[-1].append(c)
            else:
                groups.append([c])
        cost = lambda g: sum(c[2] for c in g) * nlist[g[0][0]]
        groups.sort(key=lambda g: (-len(g), -cost(g)))          # (stable, as std::stable_sort)
        out = []
        for b in range(0, len(groups), 8):
            band = groups[b: b + 8]
            for r in range(max(len(g) for g in band)):
                out += [g[r] if r < len(g) else (g[0][0], 0, 0) for g in band]
        return out
    cost = lambda c: c[2] * (1 if order == 3 else nlist[c[0]])
    if order == 2:
        ch.sort(key=cost)
    elif order != 1:
        ch.sort(key=lambda c: -cost(c))
    return ch


def utt_chunks(lens, nlist, maxtiles):
    n = 0
    for u, T in enumerate(lens):
        if T <= 0 or nlist[u] == 0:
            continue
        n16 = (T + 15) // 16
        nch = (n16 + maxtiles - 1) // maxtiles
        per = (n16 + nch - 1) // nch
        for c in range(nch):
            if min(per * 16, T - c * per * 16) <= 0:
                break
            n += 1
    return n


def pdf_slices(b, reach, TS):
    """the slice planner of run_pdf_major: [(pdf, first entry, entries, first tile offset, tiles)] in pdf order"""
    P = len(b.case.gauss)
    ents = [[] for _ in range(P)]
    lens = np.diff(b.frame_off)
    for u, T in enumerate(lens):
        n16 = (int(T) + 15) // 16
        for p in b.lists[u]:
            ef = min(n16, b.first[u][int(p)] // 16) if reach else 0
            ents[int(p)].append(n16 - ef)
    out = []
    for p in range(P):
        e, off, n = 0, 0, len(ents[p])
        while e < n:
            while e < n and ents[p][e] - off <= 0:
                e += 1; off = 0
            if e >= n:
                break
            ee, o, nt, nent = e, off, 0, 0
            while ee < n and nt < TS and nent < K1P_MAXENT:
                avail = ents[p][ee] - o
                if avail <= 0:
                    nent += 1; ee += 1; o = 0
                    continue
                take = min(avail, TS - nt)
                nt += take; nent += 1
                if take == avail:
                    ee += 1; o = 0
                else:
                    o += take
                    break
            if nt > 0:
                out.append((p, e, nent, off, nt))
            e, off = ee, o
    return out


def restate(b):
    """the k1_last() record of the case's call on a fresh set and a fresh model, from its shapes and arrays"""
    c = b.case
    opts = dict(c.opts)
    D, P = c.D, len(c.gauss)
    lens = [int(t) for t in np.diff(b.frame_off)]
    nlist = [len(x) for x in b.lists]
    N = int(b.frame_off[-1])
    has_first = b.graphs is not None
    reach = 0 if not has_first else {"full": 0, "reach": 1, "band": 2}[c.call]
    r = dict(ZERO, nb_slices=[0] * 8, asked=FORM_OPT[c.k1], mode=1 if reach else 0)
    if N == 0 or sum(nlist) == 0:
        return r
    if D > 80:
        n = sum((T + 63) // 64 for T, k in zip(lens, nlist) if T > 0 and k)
        return dict(r, form="wide", chunks=n, grid=n, per=64)
    KS, KQ = ks_of(D), kq_of(D)
    maxG = max(c.gauss)
    small = is_small(len(lens), N, D, b.graphs)
    xk, wk, gcmax = column_maxima(b.m, b.gc, b.feats, 16 * KS)
    dbg, order_opt = opts.get("k1_dbg", 0), opts.get("k1_order", 0)
    form = r["asked"]
    if form == "f16x2s":
        if not split_domain(xk, wk, gcmax):
            r["declined"] |= 1
        elif not f16x2s_scales(xk, wk):
            r["declined"] |= 2
        else:
            pack = 1 if KS != 5 or dbg & 16 else 4 if maxG <= 8 else 2 if maxG <= 16 else 1
            band = reach == 2 and pack == 1
            shift_mode = 0 if dbg & 32 else 1 if dbg & 64 else 2
            order = 4 if order_opt == 0 and KS == 10 and not small else order_opt
            per = min(NMAX[KS], 3) if small and len(lens) <= 2 else NMAX[KS]
            n = len(x32_chunks(lens, nlist, per, order))
            launch = opts.get("k1_launch", 0)
            persistent = int(pack == 1 and (launch == 2 or (launch == 0 and not small)))
            return dict(r, form="f16x2s", K=KS, mode=2 if band else int(reach != 0), pack=pack, persistent=persistent, grid=n, chunks=n, per=per,
                        order=order, tail_shift=int(not band and reach != 0 and pack == 1 and shift_mode != 0), shift_mode=shift_mode, repacked=3)
        form = "f16x2"
    if form == "f16x2":
        if not split_domain(xk, wk, gcmax):
            r["declined"] |= 1
        elif not k1h_fits(xk, wk):
            r["declined"] |= 4
        else:
            n = len(x32_chunks(lens, nlist, 16, order_opt))
            return dict(r, form="f16x2", K=KS, grid=n, chunks=n, per=16, order=order_opt, repacked=3)
        form = "pdf"
    if form == "pdf":
        if maxG <= 128:
            TS = max(1, opts.get("k1p_ts", 1024))
            nb = [0] * 8
            for s in pdf_slices(b, reach != 0, TS):
                nb[(c.gauss[s[0]] + 15) // 16 - 1] += 1
            return dict(r, form="pdf", K=KQ, grid=sum(nb), chunks=sum(nb), per=TS, nb_slices=nb, repacked=1)
        r["declined"] |= 8
    nf = 5 if KQ != 10 or opts.get("k1_nf", 0) == 5 else 6
    n = utt_chunks(lens, nlist, 4 * nf)
    il = opts.get("k1_interleave", -1)
    # (aligned: D % 4 == 0 and a 16-byte aligned feature block, which every device allocation is)
    return dict(r, form="utt", K=KQ, grid=n, chunks=n, per=4 * nf, nf=nf, aligned=int(D % 4 == 0), interleave=il if il >= 0 else int(reach != 0))


def shift_of(first, last_needed, T, call, shift_mode):
    """the shifted-tile rule of K1sUnit (f16x2s, one pdf per tile): tiles start at the band's first frame when it ends earlier inside
    its tile than it starts.  -> the shift in frames (0: aligned tiles)"""
    pl = last_needed if call == "band" else T - 1
    need = min(255, first // 32)
    lastt = 0 if pl < 0 else min(255, pl // 32)
    shift = first % 32 if pl >= 0 and need < 255 and lastt < 255 and lastt > need and pl % 32 < first % 32 else 0
    if shift_mode == 0:
        return 0
    if shift_mode == 1:
        return 16 if shift >= 16 and pl % 32 < 16 else 0
    return shift


def instantiations(rec):
    """the kernels of csrc/khg_k1.hip a call with this record launched"""
    K, f = rec["K"], rec["form"]
    out = set()
    if f == "f16x2s":
        out.add("k1s_loglikes_packed<5, %d>" % rec["pack"] if rec["pack"] > 1 else "k1s_persistent<%d>" % K if rec["persistent"] else "k1s_loglikes<%d>" % K)
        if rec["repacked"] & 1:
            out.add("k1s_pack_x<%d>" % K)
        if rec["repacked"] & 2:
            out.add("k0s_pack_tiles<%d>" % K)
    elif f == "f16x2":
        out.add("k1h_loglikes<%d, 2>" % K)
        if rec["repacked"] & 1:
            out.add("k1h_pack_x<%d>" % K)
        if rec["repacked"] & 2:
            out.add("k0h_pack_tiles<%d>" % K)
    elif f == "pdf":
        out |= {"k1p_loglikes<%d, %d, %d>" % (K, nb + 1, 2 if K == 10 else 1) for nb in range(8) if rec["nb_slices"][nb]}
        if rec["repacked"] & 1:
            out.add("k1p_pack_x<%d>" % K)
    elif f == "utt":
        out.add("k1_loglikes<%d, %d, %s, %d>" % (K, rec["nf"], "true" if rec["aligned"] else "false", 2 if K == 10 else 1))
    elif f == "wide":
        out.add("k1w_loglikes")
    return out


# every instantiation loglikes_impl can launch (k1s_repair<5 / 10> belongs to khg_align: tests/test_gpu_k1_forms.py runs it by itself)
ALL_INSTANTIATIONS = (
    {"k1_loglikes<%d, %d, %s, %d>" % (kq, nf, al, 2 if kq == 10 else 1) for kq, nf in ((10, 6), (10, 5), (20, 5)) for al in ("true", "false")}
    | {"k1p_loglikes<%d, %d, %d>" % (kq, nb, 2 if kq == 10 else 1) for kq in (10, 20) for nb in range(1, 9)}
    | {"k1p_pack_x<10>", "k1p_pack_x<20>", "k1w_loglikes", "k1s_loglikes_packed<5, 4>", "k1s_loglikes_packed<5, 2>"}
    | {t % k for k in (5, 10) for t in ("k1s_loglikes<%d>", "k1s_persistent<%d>", "k1s_pack_x<%d>", "k0s_pack_tiles<%d>", "k1h_loglikes<%d, 2>",
                                        "k1h_pack_x<%d>", "k0h_pack_tiles<%d>")})
