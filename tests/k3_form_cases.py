"""Inputs built for every row of K3's instantiation table (k3_insts in csrc/khg_k3.hip, khg_k3_forms), and their yardstick.

A case is a features-only set of N_UTT utterances, a model of P = 12 pdfs and an uploaded alignment (or posteriors) whose per-pdf
buckets hold exactly COUNTS frames: nothing, one lane, the ends of a 16-frame tile, of a 32-frame pair, of a 64-frame chunk, and two
chunks + 1.  The frames of a pdf are scattered over the set, N_SKIP frames carry transition-id 0 and must stay out.  The Gaussian
counts pin the case's class at both ends (a pdf of lo and one of hi Gaussians; where the dispatch keeps one run, also pdfs of 1 and
17 inside the wider instantiation: the masking of padding Gaussians).  Gaussians of a pdf overlap (means ~0.7 / sqrt(D) sigma apart,
variances within 10 %), so posteriors are diffuse: the largest component's share of a pdf's mass is under 0.5 on average
(tests/test_k3_form_cases_cpu.py asserts it), and a wrong softmax, Gaussian mapping or a dropped frame moves occ.  Features are
random per frame and dimension.

Every case names the options it sets and the exact record UtteranceSet.k3_last() must report per run of the plan: FIELDS.  The rows
of the table the cases expect (expected_rows: the accumulate kernel of every run, and k3_wave_finalize behind a wave form) must be
khg_k3_forms() exactly -- a row without a case, or a case naming a row that is not there, fails without a device.

The yardstick (`restate`) is AccumulateForGmm in float64 numpy on the stored fp32 parameters: log-likelihoods, log-sum-exp,
posteriors, then occ / mean_acc / var_acc / total_log_like / total_frames / trans_acc.  The CPU test holds the oracle's fp32 chain
(orc.acc_stats_ali) to it at the tolerances the GPU test uses, so a case whose inputs fp32 cannot resolve is found there.

`fp16_domain` restates k3_phase_a_scales (csrc/khg_k3.hip) so that a case's claim -- the fp16 forms' domain holds, the model's side
fails, a feature of the set overflows -- is checked before a device sees it; what the device decided is what k3_last() reports."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

from kaldi_hmm_gmm_amd import synth
from oracle import oracle as orc

INF = 2 ** 31 - 1
COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
P = len(COUNTS)
N_UTT = 20          # (more than the 16 utterances of a small set, which never builds the split feature records by itself)
N_SKIP = 12         # frames with transition-id 0
N_REAL = sum(COUNTS)
FIELDS = ("variant", "KQ", "NB", "waves", "POST", "f16a", "f16b", "planes", "cls_lo", "cls_hi")
WAVE_VARIANTS = ("wave", "wave16", "wave16_records")
TINY = 1e-31        # a weight k3_weight_ordinary rejects (|w| <= 1e-30): no fp16 phase B


def _rec(variant, KQ, NB, waves=4, post=False, f16a=False, f16b=False, planes=False, lo=0, hi=INF):
    return (variant, KQ, NB, waves, post, f16a, f16b, planes, lo, hi)


def wave(nb, f16a=False, hi=INF):
    return _rec("wave", 10, nb, f16a=f16a, hi=hi)


def wave16(nb, hi=INF):
    return _rec("wave16", 10, nb, f16a=True, f16b=True, hi=hi)


def wave16r(nb, hi=INF):
    return _rec("wave16_records", 10, nb, f16a=True, f16b=True, planes=True, hi=hi)


def mfma(kq, nb, post=False, lo=0):
    return _rec("mfma", kq, nb, post=post, lo=lo)


def block16(kq, nb, waves, lo=0):
    return _rec("block16", kq, nb, waves=waves, f16a=True, f16b=True, lo=lo)


def valu(kq, post=False, lo=0):
    return _rec("valu", kq, 0, post=post, lo=lo)


@dataclass(frozen=True)
class Case:
    name: str
    D: int
    gauss: tuple            # (lo, hi): the class of Gaussian counts, pinned at both ends; or the 12 counts themselves
    expect: tuple           # the k3_last() records, FIELDS each, per run
    opts: tuple = ()        # ((option, value), ...) set before the pass; everything else stays at its default
    weight: float = 0.75
    post: str = ""          # "": khg_acc_stats; "arrays" / "alignment": khg_acc_stats_post on DevicePosteriors.from_arrays / .from_alignment
    tweak: str = ""         # "narrow": the model's side of the fp16 domain fails; "spike": one feature of this set overflows fp16
    rot: int = 0            # pdf p holds COUNTS[(p + rot) % 12] frames

    @property
    def kq(self):
        return 10 if self.D <= 40 else 20 if self.D <= 80 else 0


def C(name, D, gauss, expect, post="", weight=0.75, tweak="", rot=0, **opts):
    return Case(name, D, tuple(gauss), tuple(expect), tuple(sorted(opts.items())), weight, post, tweak, rot)


def _mixed(big):
    """pdfs of the four-block wave class (49 .. 64, with one of 1 and one of 17) and ONE of `big` Gaussians, which holds 65 frames"""
    g = list(gauss_counts(C("", 40, (49, 64), ())))
    g[COUNTS.index(65)] = big
    return g


def gauss_counts(case):
    """the Gaussians of the 12 pdfs: lo and hi (twice), pdfs of 1 and 17 below lo where the plan stays ONE run with them (every pdf
    of <= 64 Gaussians goes to the wave form under the default dispatch at D <= 40), the rest drawn from lo .. hi"""
    if len(case.gauss) == P:
        return tuple(case.gauss)
    lo, hi = case.gauss
    rng = np.random.default_rng(1000 * lo + hi)
    g = rng.integers(max(lo, 2), hi + 1, size=P)
    g[0], g[1], g[5] = lo, hi, hi
    small = hi <= 64 or bool(case.post) or case.D > 40 or any(k == "k3_form" for k, _ in case.opts)
    if small:
        if lo > 1:
            g[2] = 1
        if lo > 17:
            g[3] = 17
    return tuple(int(x) for x in g)


CASES = [
    # ---- the wave form, fp32 phase A / fp64 phase B: one and two Gaussian blocks have nothing else (two waves per SIMD)
    C("wave1_d40", 40, (1, 16), [wave(1)]),
    C("wave2_d40", 40, (17, 32), [wave(2)], rot=3),
    C("wave3_f32_d40", 40, (33, 48), [wave(3)], k3_phase_a=1, rot=6),
    C("wave4_f32_d40", 40, (49, 64), [wave(4)], k3_phase_a=1, rot=9),
    C("wave1_d1", 1, (1, 16), [wave(1)], rot=4),
    C("wave2_d39_ny3", 39, (17, 32), [wave(2)], k3_ny=3, rot=7),
    # ---- fp16 phase A with the fp64 phase B: k3_phase_b = 0, or a weight that is no ordinary number
    C("wave3_f16a_d40", 40, (33, 48), [wave(3, True)], k3_phase_b=0, rot=1),
    C("wave4_f16a_d40_tiny", 40, (49, 64), [wave(4, True)], weight=TINY, rot=2),
    C("wave3_f16a_d39_neg", 39, (33, 48), [wave(3, True)], k3_phase_b=0, weight=-0.5, rot=5),
    C("wave4_f16a_d1", 1, (49, 64), [wave(4, True)], k3_phase_b=0, rot=8),
    # ---- both phases on the fp16 matrix cores, the in-loop split (k3_planes = off)
    C("wave16_3_d40", 40, (33, 48), [wave16(3)], k3_planes=1, rot=10),
    C("wave16_4_d40_neg", 40, (49, 64), [wave16(4)], k3_planes=1, weight=-0.5, rot=11),
    C("wave16_3_d39", 39, (33, 48), [wave16(3)], k3_planes=1, rot=2),
    C("wave16_4_d1", 1, (49, 64), [wave16(4)], k3_planes=1, rot=6),
    # ---- ... from the set's split feature records (the default)
    C("wave16r_3_d40", 40, (33, 48), [wave16r(3)], rot=4),
    C("wave16r_4_d40_neg", 40, (49, 64), [wave16r(4)], weight=-0.5, rot=1),
    C("wave16r_4_d39", 39, (49, 64), [wave16r(4)], rot=8),
    C("wave16r_3_d1", 1, (33, 48), [wave16r(3)], rot=3),
    C("wave16r_4_d40_ny3", 40, (49, 64), [wave16r(4)], k3_ny=3, rot=5),
    # ---- the fp16 forms' fallbacks: reported as such, and still right
    C("wave4_d40_narrow", 40, (49, 64), [wave(4)], tweak="narrow", rot=7),
    C("wave4_d40_spike", 40, (49, 64), [wave(4)], tweak="spike", rot=9),
    C("mfma10_2_d40_narrow", 40, (65, 128), [mfma(10, 2)], tweak="narrow", rot=2),
    # ---- the chunk-per-block fp32 + fp64 MFMA form
    C("mfma10_1_d40", 40, (1, 64), [mfma(10, 1)], k3_form=1, k3_phase_b=0, rot=1),
    C("mfma10_2_d40", 40, (65, 128), [mfma(10, 2)], k3_phase_a=1, rot=4),
    C("mfma10_3_d40_tiny", 40, (129, 192), [mfma(10, 3)], weight=TINY, rot=7),
    C("mfma10_4_d40", 40, (193, 256), [mfma(10, 4)], rot=10),
    C("mfma10_2_d39", 39, (65, 128), [mfma(10, 2)], k3_form=1, k3_phase_b=0, rot=3),
    C("mfma10_1_d1", 1, (1, 64), [mfma(10, 1)], k3_form=1, k3_phase_b=0, rot=6),
    C("mfma20_1_d80", 80, (1, 64), [mfma(20, 1)], k3_phase_b=0, rot=9),
    C("mfma20_2_d80", 80, (65, 128), [mfma(20, 2)], k3_phase_a=1, rot=0),
    C("mfma20_1_d41_tiny", 41, (1, 64), [mfma(20, 1)], weight=TINY, rot=5),
    C("mfma20_2_d79", 79, (65, 128), [mfma(20, 2)], k3_phase_b=0, rot=8),
    # ---- ... from posteriors (POST: every entry carries its own weight)
    C("post_mfma10_1_d40", 40, (1, 64), [mfma(10, 1, post=True)], post="arrays", rot=2),
    C("post_mfma10_2_d40", 40, (65, 128), [mfma(10, 2, post=True)], post="alignment", rot=5),
    C("post_mfma10_3_d40", 40, (129, 192), [mfma(10, 3, post=True)], post="arrays", rot=8),
    C("post_mfma10_4_d40", 40, (193, 256), [mfma(10, 4, post=True)], post="arrays", rot=11),
    C("post_mfma10_2_d1", 1, (65, 128), [mfma(10, 2, post=True)], post="arrays", rot=1),
    C("post_mfma20_1_d80", 80, (1, 64), [mfma(20, 1, post=True)], post="arrays", rot=4),
    C("post_mfma20_2_d80", 80, (65, 128), [mfma(20, 2, post=True)], post="arrays", rot=7),
    C("post_mfma20_1_d41", 41, (1, 64), [mfma(20, 1, post=True)], post="alignment", rot=10),
    C("post_mfma20_2_d79", 79, (65, 128), [mfma(20, 2, post=True)], post="arrays", rot=3),
    # ---- the chunk-per-block form with both phases on the fp16 matrix cores
    C("block16_10_1_4_d40", 40, (1, 64), [block16(10, 1, 4)], k3_form=1, rot=6),
    C("block16_10_1_8_d40", 40, (65, 128), [block16(10, 1, 8)], rot=9),
    C("block16_10_3_4_d40_neg", 40, (129, 192), [block16(10, 3, 4)], weight=-0.5, rot=0),
    C("block16_10_1_8_d39", 39, (65, 128), [block16(10, 1, 8)], k3_form=1, rot=2),
    C("block16_10_1_4_d1", 1, (1, 64), [block16(10, 1, 4)], k3_form=1, rot=5),
    C("block16_20_1_4_d80", 80, (1, 64), [block16(20, 1, 4)], rot=8),
    C("block16_20_1_8_d80", 80, (65, 128), [block16(20, 1, 8)], rot=11),
    C("block16_20_1_4_d41", 41, (1, 64), [block16(20, 1, 4)], rot=1),
    C("block16_20_1_8_d79", 79, (65, 128), [block16(20, 1, 8)], weight=-0.5, rot=4),
    # ---- the VALU form: any size
    C("valu10_d40", 40, (257, 264), [valu(10)], rot=7),
    C("valu10_d39_form2", 39, (1, 64), [valu(10)], k3_form=2, rot=10),
    C("valu10_d1_form2", 1, (17, 32), [valu(10)], k3_form=2, rot=3),
    C("valu20_d80", 80, (129, 136), [valu(20)], rot=6),
    C("valu20_d41_form2", 41, (1, 64), [valu(20)], k3_form=2, rot=9),
    C("valu20_d79", 79, (129, 136), [valu(20)], rot=0),
    C("valu0_d81", 81, (1, 64), [valu(0)], rot=2),
    C("valu0_d83", 83, (17, 32), [valu(0)], rot=5),
    C("post_valu10_d40", 40, (257, 264), [valu(10, post=True)], post="arrays", rot=8),
    C("post_valu10_d39_form2", 39, (1, 64), [valu(10, post=True)], post="arrays", k3_form=2, rot=11),
    C("post_valu20_d80", 80, (129, 136), [valu(20, post=True)], post="arrays", rot=1),
    C("post_valu20_d41_form2", 41, (1, 64), [valu(20, post=True)], post="alignment", k3_form=2, rot=4),
    C("post_valu0_d81", 81, (1, 64), [valu(0, post=True)], post="arrays", rot=7),
    C("post_valu0_d83", 83, (33, 48), [valu(0, post=True)], post="alignment", rot=10),
    # ---- two runs: the wave form keeps the pdfs of <= 64 Gaussians, ONE wider pdf goes to a chunk-per-block form
    C("mixed_65", 40, _mixed(65), [wave16r(4, hi=64), block16(10, 1, 8, lo=64)]),
    C("mixed_129", 40, _mixed(129), [wave16r(4, hi=64), block16(10, 3, 4, lo=64)]),
    C("mixed_257", 40, _mixed(257), [wave16r(4, hi=64), valu(10, lo=64)]),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def expected_rows(cases=None):
    """the rows of khg_k3_forms() the cases' records name: (variant, KQ, NB, waves, POST, f16a)"""
    rows = set()
    for c in CASES if cases is None else cases:
        for r in c.expect:
            rows.add(r[:6])
            if r[0] in WAVE_VARIANTS:
                rows.add(("finalize", r[1], r[2], 4, False, False))
    return rows


# ---- the fp16 phases' domain, as csrc/khg_k3.hip decides it (k3_phase_a_scales; k0_model_stats and absmax_cols for the maxima)
def fp16_domain(m, gc, feats):
    """-> (the model's side holds, no feature of the set overflows fp16, the absolute part of phase A's error bound that the rule holds
    against 4e-6 -- None where it is not reached)"""
    D = m.dim
    if D > 80:
        return False, False, None
    f32 = np.float32
    miv, iv = m.means_invvars.astype(f32), m.inv_vars.astype(f32)
    wmax = np.zeros(2 * D)
    wmax[0::2], wmax[1::2] = np.abs(miv).max(0), 0.5 * np.abs(iv).max(0)
    xb = (np.abs(miv / iv) + f32(8) / np.sqrt(iv)).max(0).astype(np.float64)
    if not ((xb > 0).all() and (xb < 1e18).all()):
        return False, False, None
    ilogb = lambda v: int(np.floor(np.log2(v)))     # noqa: E731
    ex = np.zeros(2 * D, np.int64)
    for d in range(D):
        ex[2 * d], ex[2 * d + 1] = 12 - ilogb(xb[d]), 9 - ilogb(f32(xb[d]) * f32(xb[d]))
    S = min([14 - ilogb(wmax[k]) + ex[k] for k in range(2 * D) if wmax[k] > 0] or [0])
    if S < -40 or S > 40:
        return False, False, None
    xbk = np.empty(2 * D)
    xbk[0::2], xbk[1::2] = xb, xb * xb
    floor_sum = float((np.ldexp(wmax, S - ex) + np.ldexp(xbk, ex)).sum())
    bound = float(np.abs(gc[np.isfinite(gc)]).max() + (wmax * xbk * np.where(np.arange(2 * D) & 1, 128.0, 16.0)).sum())
    floor = float(np.ldexp(floor_sum, -25 - S))
    if not (floor <= 4.0e-6 and bound <= 268435456.0):
        return False, False, floor
    xmax = np.abs(feats).max(0).astype(np.float64)
    xk = np.empty(2 * D)
    xk[0::2], xk[1::2] = xmax, (xmax.astype(f32) * xmax.astype(f32))
    return True, bool((np.ldexp(xk, ex) < 65504.0).all()), floor


# ---- the yardstick
def restate(m, gc, feats, frames, tids, w, unit_trans):
    """AccumulateForGmm per (frame, transition-id, weight) entry in float64 on the stored fp32 parameters.  unit_trans: an alignment's
    transition statistics count 1 per frame (transition-model.h:183-189 with prob = 1.0); the posteriors' add the weight."""
    sumG, D = int(m.gauss_off[-1]), m.dim
    occ, mean, var = np.zeros(sumG), np.zeros((sumG, D)), np.zeros((sumG, D))
    trans = np.zeros(m.num_tids + 1)
    tot_ll = 0.0
    pdf = m.id2pdf[tids]
    w = np.asarray(w, np.float64)
    x64 = feats.astype(np.float64)
    for p in np.unique(pdf):
        sel = pdf == p
        a, b = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
        x, wp = x64[frames[sel]], w[sel]
        ll = gc[a:b].astype(np.float64)[None, :] + x @ m.means_invvars[a:b].astype(np.float64).T - 0.5 * (x * x) @ m.inv_vars[a:b].astype(np.float64).T
        mx = ll.max(1, keepdims=True)
        e = np.exp(ll - mx)
        s = e.sum(1, keepdims=True)
        g = wp[:, None] * e / s
        occ[a:b] = g.sum(0)
        mean[a:b] = g.T @ x
        var[a:b] = g.T @ (x * x)
        tot_ll += float(((mx + np.log(s))[:, 0] * wp).sum())
    np.add.at(trans, tids, 1.0 if unit_trans else w)
    return {"occ": occ, "mean_acc": mean, "var_acc": var, "trans_acc": trans, "total_frames": float(w.sum()), "total_log_like": tot_ll}


@dataclass
class Built:
    case: Case
    m: object
    gc: np.ndarray
    feats: np.ndarray
    ali: np.ndarray
    frame_off: np.ndarray
    counts: np.ndarray          # frames (entries) per pdf
    frames: np.ndarray          # the entries: frame, transition-id, weight as the pass rounds it (float32)
    tids: np.ndarray
    w: np.ndarray
    post_arrays: tuple          # (frame_off, entry_begin, tid, weight float64) for DevicePosteriors.from_arrays, or None
    scale: float                # khg_acc_stats_post's scale
    ref: dict
    bucket_w: np.ndarray        # per pdf: the sum of its entries' weights


@functools.lru_cache(maxsize=None)
def build(name):
    c = BY_NAME[name]
    D = c.D
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    g = np.array(gauss_counts(c))
    m = synth.make_model(P, 1, D, seed=zlib.crc32(name.encode()) % 10000, gauss_counts=g)
    sumG = int(m.gauss_off[-1])
    of = np.repeat(np.arange(P), g)
    base = rng.uniform(0.5, 2.0, size=D)
    centre = 0.5 * rng.standard_normal((P, D))
    means = centre[of] + (0.7 / np.sqrt(D)) * np.sqrt(base)[None, :] * rng.standard_normal((sumG, D))
    var = base[None, :] * rng.uniform(0.9, 1.1, size=(sumG, D))
    counts = np.array([COUNTS[(p + c.rot) % P] for p in range(P)])
    if c.tweak == "narrow":
        # one Gaussian of the fullest pdf is 1/1000 as wide in one dimension (its mean at the pdf's centre): wmax there grows by 2^10, S
        # drops with it and the absolute part of the error bound passes 4e-6
        gn = int(m.gauss_off[int(np.argmax(counts))])
        var[gn, 3 % D] = 1e-3 * base[3 % D]
        means[gn, 3 % D] = centre[of[gn], 3 % D]
    means, var = means.astype(np.float32), var.astype(np.float32)
    inv_vars = (1.0 / var).astype(np.float32)
    miv = (means * inv_vars).astype(np.float32)
    import dataclasses
    m = dataclasses.replace(m, means=means, vars=var, inv_vars=inv_vars, means_invvars=miv)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    # the frames: COUNTS per pdf under a random Gaussian of the pdf, N_SKIP without a transition-id; scattered through the set.  The
    # posteriors made from the alignment take an utterance whose first id is 0 for a failed one, so there the frames without an id are
    # one whole utterance; everywhere else they lie among the others.
    frame_pdf = np.repeat(np.arange(P), counts)
    whole = c.post == "alignment"
    if whole:
        order = rng.permutation(N_REAL)
        sizes = np.diff(np.linspace(0, N_REAL, N_UTT).astype(np.int64))          # N_UTT - 1 utterances
        cut = int(sizes[:7].sum())
        frame_pdf = np.concatenate([frame_pdf[order][:cut], np.full(N_SKIP, -1), frame_pdf[order][cut:]])
        frame_off = np.concatenate([[0], np.cumsum(np.concatenate([sizes[:7], [N_SKIP], sizes[7:]]))]).astype(np.int64)
    else:
        frame_pdf = np.concatenate([frame_pdf, np.full(N_SKIP, -1)])[rng.permutation(N_REAL + N_SKIP)]
        frame_off = np.linspace(0, N_REAL + N_SKIP, N_UTT + 1).astype(np.int64)
    N = len(frame_pdf)
    real = frame_pdf >= 0
    pick = m.gauss_off[np.maximum(frame_pdf, 0)] + (rng.random(N) * g[np.maximum(frame_pdf, 0)]).astype(np.int64)
    feats = (means[pick] + np.sqrt(var[pick]) * rng.standard_normal((N, D))).astype(np.float32)
    feats[~real] = rng.standard_normal((int((~real).sum()), D)).astype(np.float32)
    if c.tweak == "spike":
        # on a frame WITHOUT a transition-id: the set's column maxima see it (fp32 phase A for this set), the statistics do not, so the
        # tolerances -- which scale with the largest cell -- stay those of every other case
        xb = (np.abs(miv / inv_vars) + 8.0 / np.sqrt(inv_vars)).max(0)
        feats[np.nonzero(~real)[0][0], D // 2] = np.float32(20.0 * xb[D // 2])
    ali = np.where(real, 2 * np.maximum(frame_pdf, 0) + 1 + (rng.random(N) < 0.5), 0).astype(np.int32)     # either transition-id of the pdf
    frames = np.nonzero(real)[0]
    tids = ali[frames]
    post_arrays, scale = None, 1.0
    if c.post == "arrays":
        # one entry per frame with an id, weights k / 64 that differ from entry to entry: every sum of them is exact in any order
        w64 = rng.integers(8, 97, size=len(frames)) / 64.0
        eb = np.concatenate([[0], np.cumsum(real)]).astype(np.int64)
        post_arrays = (frame_off, eb, tids.astype(np.int32), w64.astype(np.float64))
        w = w64.astype(np.float32)
    elif c.post == "alignment":
        scale = c.weight
        w = np.full(len(frames), np.float32(c.weight), np.float32)
    else:
        w = np.full(len(frames), np.float32(c.weight), np.float32)
    ref = restate(m, gc, feats, frames, tids, w, unit_trans=not c.post)
    bucket_w = np.bincount(m.id2pdf[tids], weights=w.astype(np.float64), minlength=P)
    for a in (feats, ali, frame_off, counts, gc, *[v for v in ref.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return Built(c, m, gc, feats, ali, frame_off, counts, frames, tids, w, post_arrays, scale, ref, bucket_w)


def oracle_stats(b):
    """the oracle's fp32 chain on the case: one orc.acc_stats_ali call over the frames with an id (an alignment), or one per entry with
    the entry's weight (posteriors: tests/acc_post_ref.py) -- in the layout of DeviceAccs.download()"""
    m = b.m
    om = orc.OModel(m.gauss_off, b.gc, m.means_invvars, m.inv_vars)
    oa = orc.OAccs(int(m.gauss_off[-1]), m.dim, m.num_tids)
    if not b.case.post:
        orc.acc_stats_ali(om, m.id2pdf, b.feats[b.frames], b.tids, oa, weight=float(b.w[0]))
        trans = oa.trans_acc.copy()
    else:
        for f, t, w in zip(b.frames, b.tids, b.w):
            orc.acc_stats_ali(om, m.id2pdf, b.feats[f:f + 1], [int(t)], oa, weight=float(w))
        trans = np.bincount(b.tids, weights=b.w.astype(np.float64), minlength=m.num_tids + 1)
    return {"occ": oa.occ, "mean_acc": oa.mean_acc, "var_acc": oa.var_acc, "trans_acc": trans, "total_frames": oa.total_frames,
            "total_log_like": oa.total_log_like}


def assert_stats(got, b, what=""):
    """`got` (DeviceAccs.download(), or the oracle's statistics) against the float64 restatement, at the tolerances the project states for
    diffuse posteriors (tests/test_gpu_parity.py: a posterior is exp() of the difference of two fp32 log-likelihoods): rtol 2e-4, atol
    1e-6 for occ, 2e-5 x the largest cell for mean_acc / var_acc, rel 2e-6 for the log-likelihood.  trans_acc and total_frames are
    exact sums (weights of 24 bits, at most 2^9 of them: every partial sum is a double).  Under the weight 1e-31 the occupancies are
    compared after division by it as well: the absolute 1e-6 would pass anything there."""
    ref, c = b.ref, b.case
    assert np.array_equal(got["trans_acc"], ref["trans_acc"]), what
    assert abs(got["total_frames"] - ref["total_frames"]) <= 1e-12 * abs(ref["total_frames"]), (what, got["total_frames"], ref["total_frames"])
    assert abs(got["total_log_like"] - ref["total_log_like"]) <= 2e-6 * abs(ref["total_log_like"]), (what, got["total_log_like"], ref["total_log_like"])
    np.testing.assert_allclose(got["occ"], ref["occ"], rtol=2e-4, atol=1e-6, err_msg=str(what))
    if not c.post and abs(c.weight) < 1e-3:
        np.testing.assert_allclose(got["occ"] / np.float64(np.float32(c.weight)), ref["occ"] / np.float64(np.float32(c.weight)), rtol=2e-4, atol=1e-6,
                                   err_msg=str(what))
    for k in ("mean_acc", "var_acc"):
        np.testing.assert_allclose(got[k], ref[k], rtol=2e-4, atol=2e-5 * np.abs(ref[k]).max(), err_msg="%s %s" % (what, k))
    # the empty pdf: exact zeros
    for p in np.nonzero(b.counts == 0)[0]:
        a, e = int(b.m.gauss_off[p]), int(b.m.gauss_off[p + 1])
        assert not got["occ"][a:e].any() and not got["mean_acc"][a:e].any() and not got["var_acc"][a:e].any(), (what, "empty pdf", p)
    # a pdf's posteriors sum to one per frame: sum of occ = the bucket's weight, up to the softmax's fp32 roundings (exp, the sum's
    # reciprocal and one product per Gaussian: (G + 8) 2^-24, doubled for the weight's product) and, where gamma enters an fp16 phase
    # B as two fp16 pieces, 2^-21 per gamma (doubled)
    G = np.diff(b.m.gauss_off)
    per_pdf = np.add.reduceat(got["occ"], b.m.gauss_off[:-1].astype(np.int64))
    tol = ((G + 8) * 2.0 ** -23 + 2.0 ** -20) * np.abs(b.bucket_w)
    assert (np.abs(per_pdf - b.bucket_w) <= tol).all(), (what, "per-pdf occupancy", per_pdf - b.bucket_w, tol)


def diffuseness(b):
    """the largest component's share of a pdf's mass, averaged over the pdfs with mass"""
    occ = np.abs(b.ref["occ"])
    off = b.m.gauss_off[:-1].astype(np.int64)
    mx, sm = np.maximum.reduceat(occ, off), np.add.reduceat(occ, off)
    return float((mx[sm > 0] / sm[sm > 0]).mean())
