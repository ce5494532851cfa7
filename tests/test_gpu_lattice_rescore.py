"""khg_lattices_rescore and khg_lattices_boost on the device against tests/lattice_rescore_ref.py.

Lattices are mostly hand-made "sausages" through DeviceLattices.from_lattices, so every case controls its cells: frame t has one state
(plus what a case adds) and one arc per listed transition-id into frame t + 1.  The transition table of those cases maps id k to pdf
k - 1.  The bound of a CELLS value is the project's own K1 tolerance (include/khg_hip.h): |error| <= 1e-5 + 1e-6 B against float64,
times the acoustic scale for a cost."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import helpers  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_ref as pr  # noqa: E402
import lattice_rescore_ref as rr  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_faster_raw import _decoder_launches, _feats, _fst, _is_empty, _slice_bytes, setup, trained  # noqa: E402,F401
from test_gpu_lattice_ops import _dict, _entry  # noqa: E402
from test_lattice_ops_cpu import _hand  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
INF = np.inf
WORST = {"share": 0.0}          # the largest share of the K1 bound a CELLS value used, over the whole module


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ops.FIELDS], int(lat["start"]))


def sausage(frames, seed=0, final=0.5):
    """frames: per frame the transition-ids of its arcs -> the lattice (state t on frame t)"""
    rng = np.random.default_rng(seed)
    T = len(frames)
    st = [(t, INF) for t in range(T)] + [(T, final)]
    ar = [(t, int(il), 0, float(rng.uniform(0, 2)), float(rng.uniform(0, 9)), t + 1) for t, ids in enumerate(frames) for il in ids]
    return _hand(st, ar)


def _same(got, want, tag):
    for k in ops.FIELDS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), (tag, k)
    assert got.start == want["start"], tag


class Model:
    """a synthetic model on a context: every pdf p behind transition-id p + 1"""

    def __init__(self, khg, ctx, P, G, D, seed=1, ragged=False, gauss_counts=None):
        from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, synth
        from oracle import oracle as orc
        self.m = synth.make_model(P, G, D, seed=20230414 + seed, ragged=ragged, gauss_counts=gauss_counts)
        self.gc = orc.model_gconsts(self.m.gauss_off, self.m.weights, self.m.inv_vars, self.m.means_invvars)
        self.id2pdf = np.concatenate([[-1], np.arange(P)]).astype(np.int32)
        self.dm = DeviceModel(ctx, self.m.gauss_off, self.gc, self.m.means_invvars, self.m.inv_vars)
        self.dt = DeviceTransitions(ctx, self.id2pdf)
        self.P, self.D = P, D

    def feats(self, T, seed):
        """rows near the model's means (so that no cell underflows), a few far away"""
        rng = np.random.default_rng(seed)
        g = rng.integers(0, len(self.gc), T)
        mean = self.m.means_invvars[g] / self.m.inv_vars[g]
        x = mean + rng.normal(size=(T, self.D)) / np.sqrt(self.m.inv_vars[g])
        return np.ascontiguousarray(x, F)

    def close(self):
        self.dm.close(); self.dt.close()


def _check_cells(mod, lats_in, got, feats_list, scale, tag, id2pdf=None, model=None):
    """every rescored arc within scale * (1e-5 + 1e-6 B) of float64; everything else as the input; -> arcs checked"""
    id2pdf = mod.id2pdf if id2pdf is None else id2pdf
    m, gc = model if model is not None else (mod.m, mod.gc)
    n = 0
    for u, (lat, g, x) in enumerate(zip(lats_in, got, feats_list)):
        for k in ops.FIELDS:
            if k != "acoustic_cost":
                assert np.asarray(getattr(g, k)).tobytes() == lat[k].tobytes(), (tag, u, k)
        if len(lat["ilabel"]) == 0:
            continue
        pdfs = sorted({int(id2pdf[il]) for il in lat["ilabel"] if il != 0})
        ex, bd = helpers.exact_loglikes(m, gc, x, pdfs)
        full_e = np.zeros((int(max(id2pdf)) + 1, len(x))); full_b = np.zeros_like(full_e)
        full_e[pdfs], full_b[pdfs] = ex, bd
        want, B = rr.rescore_exact(lat, full_e, full_b, id2pdf, scale)
        ac = np.asarray(g.acoustic_cost, np.float64)
        em = lat["ilabel"] != 0
        assert ops.bits(np.asarray(g.acoustic_cost)[~em]) == ops.bits(lat["acoustic_cost"][~em]), (tag, u)
        tol = abs(float(F(scale))) * (1e-5 + 1e-6 * B[em])
        err = np.abs(ac[em] - want[em])
        share = float((err / tol).max())
        WORST["share"] = max(WORST["share"], share)
        assert share <= 1.0, (tag, u, share)
        n += int(em.sum())
    return n


@pytest.fixture(scope="module")
def ctx():
    from kaldi_hmm_gmm_amd import Context
    return Context(0)


# ---- 1. FROM_LL, bit for bit ----------------------------------------------------------------------------------------------------
def test_from_ll_bit_for_bit_on_uploaded_scores(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    n_idx, used = 12, 10
    lens = [1, 33, 70]                                             # tpad = 32, 64, 96
    # one state, a self-loop per index 1 .. used: every length decodes; pdfs 10 and 11 are on no graph
    g = {"start": 0, "arc_off": np.array([0, used], np.int64), "ilabel": np.arange(1, used + 1, dtype=np.int32),
         "olabel": np.zeros(used, np.int32), "weight": np.linspace(0.1, 0.5, used).astype(F), "nextstate": np.zeros(used, np.int32),
         "final": np.array([0.25], F)}
    tabs = [np.random.default_rng(3 + i).normal(size=(T, n_idx + 1)).astype(F) for i, T in enumerate(lens)]
    dt = DeviceTransitions(ctx, np.concatenate([[-1], np.arange(n_idx)]).astype(np.int32))
    dm = DeviceModel(ctx, np.arange(n_idx + 1, dtype=np.int32), np.zeros(n_idx, F), np.zeros((n_idx, 1), F), np.ones((n_idx, 1), F))
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    us = UtteranceSet(ctx, dt, fo, np.zeros((int(fo[-1]), 1), F), graphs=tg.concat([g] * len(lens)))
    po, pl = us.pdf_lists()
    assert pl[po[0]: po[1]].tolist() == list(range(used))
    us.upload_loglikes([np.ascontiguousarray(t[:, 1 + np.asarray(pl[po[u]: po[u + 1]])].T) for u, t in enumerate(tabs)])
    dd = us.raw_lattices_faster_device(dt, beam=3.0, lattice_beam=2.0, acoustic_scale=1.0)
    dl = dd["lattices"]
    assert all(int(s) & 1 for s in dd["status"])
    L = dl.download()
    lats = [_dict(x) for x in L]
    assert sum(int((x["ilabel"] != 0).sum()) for x in lats) > sum(lens)           # the lattices branch
    for scale in (1.0, 0.1):
        R = dl.rescore(us, dm, dt, scale, "from_ll")
        assert R.status.tolist() == [rr.SUCCEEDED] * 3 and R.rescore_stats["arcs"] == int(dl.arc_off[-1])
        for u, (got, lat) in enumerate(zip(R.download(), lats)):
            _same(got, rr.rescore_from_ll(lat, lambda t, il, u=u: tabs[u][t, il], scale), (scale, u))
        R.close()
    for u, (got, lat) in enumerate(zip(dl.download(), lats)):
        _same(got, lat, ("the input is untouched", u))
    # an arc naming pdf 11, which is on no list: that utterance alone is left empty
    bad = sausage([[12]])
    H = khg.DeviceLattices.from_lattices([_lattice(khg, bad), L[1], L[2]], ctx)
    R = H.rescore(us, dm, dt, 1.0, "from_ll")
    assert R.status.tolist() == [rr.NO_REF, rr.SUCCEEDED, rr.SUCCEEDED]
    out = R.download()
    assert _is_empty(out[0]) and R.state_off.tolist() == [0, 0, L[1].num_states, L[1].num_states + L[2].num_states]
    for u in (1, 2):
        _same(out[u], rr.rescore_from_ll(lats[u], lambda t, il, u=u: tabs[u][t, il], 1.0), ("beside the empty one", u))
    assert R.best_path([1.0], [1.0])["status"].tolist() == [ops.NO_PATH, ops.SUCCEEDED, ops.SUCCEEDED]
    R.close(); H.close(); dl.close(); us.close(); dm.close(); dt.close()


def test_from_ll_refusals(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    from kaldi_hmm_gmm_amd import synth
    from oracle import oracle as orc
    m = synth.make_model(30, 64, 40, seed=7)              # (a shape the band form of K1 takes)
    ut = synth.make_utts(m, 2, seed=2, min_phones=3, max_phones=6)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, ut.frame_off, ut.feats, graphs=ut.graphs)
    lens = np.diff(ut.frame_off)
    H = khg.DeviceLattices.from_lattices([_lattice(khg, sausage([[1]] * int(T))) for T in lens], ctx)
    with pytest.raises(RuntimeError, match="resident scores"):
        H.rescore(us, dm, dt, 1.0, "from_ll")
    us.loglikes(dm, reachable_only=True, band=True)
    with pytest.raises(RuntimeError, match="khg_loglikes_band"):
        H.rescore(us, dm, dt, 1.0, "from_ll")
    H.rescore(us, dm, dt, 1.0, "cells").close()          # CELLS needs no resident scores
    H.close(); us.close(); dm.close(); dt.close()


# ---- 2. CELLS against float64, and against FROM_LL on the strict-fp32 K1 ------------------------------------------------------
SHAPES = [(6, 1, 13, False), (6, 7, 40, False), (4, 64, 40, False), (4, 65, 40, False), (3, 100, 77, True), (3, 130, 23, False), (2, 70, 120, False)]


@pytest.mark.parametrize("P,G,D,ragged", SHAPES, ids=["%dx%dx%d" % s[:3] for s in SHAPES])
def test_cells_against_float64_and_the_fp32_k1(ctx, P, G, D, ragged):
    """(2, 70, 120): 67 200 bytes of rows, past the LDS staging limit -- the same chain read from HBM"""
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import UtteranceSet
    mod = Model(khg, ctx, P, G, D, seed=P + G, ragged=ragged)
    lens = [9, 34]
    rng = np.random.default_rng(G)
    feats = [mod.feats(T, 10 + i) for i, T in enumerate(lens)]
    # every pdf on every frame, in a random order; some ids twice (two arcs, one cell)
    lats = [sausage([list(rng.permutation(P) + 1) + [int(rng.integers(1, P + 1))] for _ in range(T)], seed=T) for T in lens]
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    us = UtteranceSet(ctx, None, fo, np.concatenate(feats))
    H = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats], ctx)
    arcs = 0
    for scale in (1.0, 0.1):
        R = H.rescore(us, mod.dm, mod.dt, scale)
        assert R.rescore_stats == {"arcs": sum(lens) * (P + 1), "emitting_arcs": sum(lens) * (P + 1), "cells": sum(lens) * P}
        arcs += _check_cells(mod, lats, R.download(), feats, scale, (P, G, D, scale))
        if scale == 1.0:
            # the same arcs gathered from khg_loglikes under KHG_K1_FP32_PDF: two values, each within the bound of float64
            us.set_pdf_list(np.arange(P, dtype=np.int32))
            old = ctx.set_option("k1_form", 2)
            try:
                us.loglikes(mod.dm)
                Q = H.rescore(us, mod.dm, mod.dt, scale, "from_ll")
            finally:
                ctx.set_option("k1_form", old)
            for u, (a, b, lat, x) in enumerate(zip(R.download(), Q.download(), lats, feats)):
                _, bd = helpers.exact_loglikes(mod.m, mod.gc, x, list(range(P)))
                fr = rr.arc_frames(lat)
                B = bd[mod.id2pdf[lat["ilabel"]], fr]
                diff = np.abs(np.asarray(a.acoustic_cost, np.float64) - np.asarray(b.acoustic_cost, np.float64))
                assert (diff <= 2 * (1e-5 + 1e-6 * B)).all(), (u, float((diff / (1e-5 + 1e-6 * B)).max()))
            Q.close()
        R.close()
    assert arcs == 2 * sum(lens) * (P + 1)
    print("largest share of the K1 bound so far: %.3f" % WORST["share"])
    H.close(); us.close(); mod.close()


# ---- 3. bucket and slice edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [7, 40])
def test_bucket_and_slice_edges(ctx, G):
    """pdf 0 with n = 1, 63, 64, 65, 129 distinct cells; pdf 1 with none; pdf 2 with 300, i.e. three work items of 128 cells; pdf 3
    with one.  G = 7 packs two cells into a wave (an odd count leaves half a wave idle), G = 40 takes a wave per cell."""
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import UtteranceSet
    mod = Model(khg, ctx, 4, G, 13, seed=G)
    T = 300
    x = mod.feats(T, 77)
    us = UtteranceSet(ctx, None, np.array([0, T], np.int64), x)
    for n in (1, 63, 64, 65, 129):
        lat = sausage([[3] + ([1] if t < n else []) + ([4] if t == 7 else []) for t in range(T)], seed=n)
        H = khg.DeviceLattices.from_lattices([_lattice(khg, lat)], ctx)
        R = H.rescore(us, mod.dm, mod.dt, 1.0)
        assert R.rescore_stats == {"arcs": T + n + 1, "emitting_arcs": T + n + 1, "cells": T + n + 1}
        assert _check_cells(mod, [lat], R.download(), [x], 1.0, ("edges", G, n)) == T + n + 1
        R.close(); H.close()
    us.close(); mod.close()


# ---- 4. sharing -----------------------------------------------------------------------------------------------------------------
def test_five_arcs_of_different_states_share_one_cell(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import UtteranceSet
    mod = Model(khg, ctx, 5, 9, 17, seed=8)
    # frame 0: the start and four states behind epsilon arcs; each of the five has an arc with id 3 into frame 1, and one of its own
    st = [(0, INF)] * 5 + [(1, INF), (1, INF), (2, 0.0)]
    ar = [(0, 0, k, 0.1 * k, 0.0, k) for k in range(1, 5)]
    ar += [(s, 3, 0, 0.2 * s, 1.0 + s, 5 + s % 2) for s in range(5)] + [(s, (1, 2, 4, 5, 4)[s], 0, 0.3, 2.0, 6) for s in range(5)]
    ar += [(5, 2, 0, 0.5, 1.0, 7), (6, 2, 0, 0.25, 3.0, 7), (6, 4, 0, 0.25, 3.0, 7)]
    lat = _hand(st, ar)
    lats = [lat, sausage([[1, 2], [2]])]
    feats = [mod.feats(2, 1), mod.feats(2, 2)]
    fo = np.array([0, 2, 4], np.int64)
    us = UtteranceSet(ctx, None, fo, np.concatenate(feats))
    H = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats], ctx)
    R = H.rescore(us, mod.dm, mod.dt, 0.5)
    got = R.download()
    _check_cells(mod, lats, got, feats, 0.5, "sharing")
    ac = np.asarray(got[0].acoustic_cost)
    five = [a for a in range(len(lat["ilabel"])) if lat["ilabel"][a] == 3]
    assert len(five) == 5 and len({int(lat["frame"][s]) for s in range(5)}) == 1
    assert len(set(ops.bits(ac[five]))) == 1
    keys = rr.cell_keys(lats, mod.id2pdf, fo)
    n_arcs = sum(len(x["ilabel"]) for x in lats)
    n_em = sum(int((x["ilabel"] != 0).sum()) for x in lats)
    assert R.rescore_stats == {"arcs": n_arcs, "emitting_arcs": n_em, "cells": len(np.unique(keys))}
    assert len(keys) == n_em and len(np.unique(keys)) < n_em
    R.close(); H.close(); us.close(); mod.close()


# ---- 5. independence ------------------------------------------------------------------------------------------------------------
def test_a_cell_depends_on_row_pdf_and_model_only(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    m, gc, om, ut, cost = helpers.build(6, 7, 13, 5, seed=9)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    rng = np.random.default_rng(12)
    lens = np.diff(ut.frame_off)
    lats = [sausage([list(rng.choice(m.num_tids, 3, replace=False) + 1) for _ in range(int(T))], seed=int(T)) for T in lens]
    L = [_lattice(khg, x) for x in lats]
    feats = [helpers.utt_feats(ut, u) for u in range(5)]
    full = UtteranceSet(ctx, dt, ut.frame_off, ut.feats, graphs=ut.graphs)
    bare = UtteranceSet(ctx, None, ut.frame_off, ut.feats)
    H = khg.DeviceLattices.from_lattices(L, ctx)
    a = [np.asarray(x.acoustic_cost) for x in H.rescore(full, dm, dt, 1.0).download()]
    b = [np.asarray(x.acoustic_cost) for x in H.rescore(full, dm, dt, 1.0).download()]
    c = [np.asarray(x.acoustic_cost) for x in H.rescore(bare, dm, dt, 1.0).download()]
    for u in range(5):
        assert a[u].tobytes() == b[u].tobytes(), ("two runs", u)
        assert a[u].tobytes() == c[u].tobytes(), ("features-only set", u)
        one = UtteranceSet(ctx, None, np.array([0, lens[u]], np.int64), np.ascontiguousarray(feats[u]))
        H1 = khg.DeviceLattices.from_lattices([L[u]], ctx)
        d = np.asarray(H1.rescore(one, dm, dt, 1.0).download()[0].acoustic_cost)
        assert a[u].tobytes() == d.tobytes(), ("one-utterance batch", u)
        H1.close(); one.close()
    H.close(); full.close(); bare.close(); dm.close(); dt.close()


# ---- 6. handles -----------------------------------------------------------------------------------------------------------------
def test_two_chunk_handle_and_the_copied_index(setup):
    """the two-chunk construction of test_gpu_lattice_faster_raw.py::test_more_than_one_launch; the rescored handle is an ordinary one"""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    dctx = _gpu.default_context()
    g = sg.word_loop_graph(np.random.default_rng(sg.BIG_W), m.num_tids, sg.BIG_W, sg.BIG_CHAIN)
    S, A = len(g["final"]), len(g["ilabel"])
    lens3 = [12, 11, 13]
    hb = max(1000, int(F(S) * F(2.0))) + 1
    U = int((4 << 30) // min(_slice_bytes(T, S, A, hb) for T in lens3)) + 9
    feats = _feats(ut, U, [lens3[u % 3] for u in range(U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=8.0, max_active=100, min_active=0, lattice_beam=4.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    co = dl.chunk_off
    assert dl.num_chunks >= 2
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    dm = DeviceModel(dctx, go, gc, miv, iv)
    dt = DeviceTransitions(dctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats), F))
    lats = [_dict(x) for x in dl.download()]
    mm = type("M", (), {"gauss_off": np.asarray(go, np.int32), "means_invvars": np.asarray(miv, F), "inv_vars": np.asarray(iv, F)})
    pick = sorted({0, 1, co[1] - 1, co[1], U - 1})

    def check(R, tag):
        assert R.num_chunks == dl.num_chunks and R.chunk_off == co and R.arc_off.tolist() == dl.arc_off.tolist()
        got = R.download()
        n = _check_cells(None, [lats[u] for u in pick], [got[u] for u in pick], [feats[u] for u in pick], 0.1, tag, id2pdf=id2pdf,
                         model=(mm, np.asarray(gc, F)))
        assert n > 0
        return got

    R0 = dl.rescore(us, dm, dt, 0.1)                      # the input has no in-arc index yet
    check(R0, "no index")
    (P0, names) = _decoder_launches(dctx, lambda: R0.posteriors(1.0, 1.0))
    assert names.count("k2_lattice_post_index") == dl.num_chunks
    P1 = dl.posteriors(1.0, 1.0)                           # builds the input's index
    (R1, names) = _decoder_launches(dctx, lambda: dl.rescore(us, dm, dt, 0.1))
    print(names)
    assert {"k2x_flatten", "k1c_sort", "k1c_heads", "k1c_score", "k1c_scatter"} <= set(names)
    got = check(R1, "index copied")
    (P2, names) = _decoder_launches(dctx, lambda: R1.posteriors(1.0, 1.0))
    assert "k2_lattice_post_index" not in names and "k2_lattice_post_fb" in names
    assert np.asarray(P2.tot_like).tobytes() == np.asarray(P0.tot_like).tobytes()       # the copied index is the rebuilt one
    # best_path, prune, download on the result; the decoder's scores were the fp16 K1's, so the path may differ: compare with the host
    bp = R1.best_path([1.0], [1.0])
    for u in pick:
        want = got[u].best_path(1.0, 1.0)
        assert _entry(bp, 0, u, U)[:3] == (want["status"], want["ali"], want["words"]), u
    Pr = R1.prune(0.5)
    assert Pr.num_chunks == dl.num_chunks and int(Pr.arc_off[-1]) <= int(R1.arc_off[-1])
    for x in (P0, P1, P2, Pr, R0, R1, us, dm, dt, dl, dg):
        x.close()


def test_failing_statuses_stay_empty(setup):
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    dctx = _gpu.default_context()
    rng = np.random.default_rng(5)
    good = tg.random_graph(rng, m.num_tids, n_main=6)
    dead = {"start": 0, "arc_off": np.array([0, 1, 1], np.int64), "ilabel": np.array([1], np.int32), "olabel": np.array([0], np.int32),
            "weight": np.array([0.0], F), "nextstate": np.array([1], np.int32), "final": np.array([np.inf, 0.0], F)}
    feats = _feats(ut, 3)
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    rd, dl = khg.get_raw_lattice_faster_device_batch(am, tm, [_fst(khg, x) for x in (good, dead, good)], feats, cfg, 0.1)
    assert [r["status"] for r in rd] == [1, 8, 1]
    go, gc, w, miv, iv = am.flat()
    dm = DeviceModel(dctx, go, gc, miv, iv)
    dt = DeviceTransitions(dctx, np.asarray(tm.transition_id_to_pdf_array(), np.int32))
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats), F))
    for mode in ("cells", "from_ll"):
        if mode == "from_ll":
            us.set_pdf_list(np.arange(len(go) - 1, dtype=np.int32))
            us.loglikes(dm)
        R = dl.rescore(us, dm, dt, 1.0, mode)
        assert R.status.tolist() == [rr.SUCCEEDED, rr.NO_PATH, rr.SUCCEEDED], mode
        out = R.download()
        assert [_is_empty(x) for x in out] == [False, True, False] and R.state_off.tolist() == dl.state_off.tolist()
        R.close()
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    B = dl.boost(tid2phone, np.array([1], np.int32), alignment=[np.asarray(r["alignment"], np.int32) for r in rd], b=0.5)
    assert B.status.tolist() == [rr.SUCCEEDED, rr.NO_PATH, rr.SUCCEEDED] and _is_empty(B.download()[1])
    B.close(); us.close(); dm.close(); dt.close(); dl.close()


def test_rescore_refusals(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import Context, UtteranceSet
    mod = Model(khg, ctx, 4, 3, 5, seed=2)
    lats = [_lattice(khg, sausage([[1], [2]])), _lattice(khg, sausage([[3]]))]
    H = khg.DeviceLattices.from_lattices(lats, ctx)
    x = mod.feats(3, 0)
    us = UtteranceSet(ctx, None, np.array([0, 2, 3], np.int64), x)
    H.rescore(us, mod.dm, mod.dt, 1.0).close()
    with pytest.raises(RuntimeError, match="mode"):
        H.rescore(us, mod.dm, mod.dt, 1.0, "dense")
    with pytest.raises(RuntimeError, match="finite"):
        H.rescore(us, mod.dm, mod.dt, float("nan"))
    two = UtteranceSet(ctx, None, np.array([0, 3], np.int64), x)
    with pytest.raises(RuntimeError, match="2 utterances, the set 1"):
        H.rescore(two, mod.dm, mod.dt, 1.0)
    other = UtteranceSet(ctx, None, np.array([0, 1, 3], np.int64), x)
    with pytest.raises(RuntimeError, match="utterance 0: the lattice spans 2 frames, the set has 1"):
        H.rescore(other, mod.dm, mod.dt, 1.0)
    wide = UtteranceSet(ctx, None, np.array([0, 2, 3], np.int64), np.zeros((3, 6), F))
    with pytest.raises(RuntimeError, match="dimensions"):
        H.rescore(wide, mod.dm, mod.dt, 1.0)
    ctx2 = Context(0)
    mod2 = Model(khg, ctx2, 4, 3, 5, seed=2)
    with pytest.raises(RuntimeError, match="another context"):
        H.rescore(us, mod2.dm, mod2.dt, 1.0)
    # an ilabel the transition table does not have: the device guard raises the context's error word
    bad = khg.DeviceLattices.from_lattices([_lattice(khg, sausage([[1], [9]])), lats[1]], ctx)
    with pytest.raises(RuntimeError, match="out of range"):
        bad.rescore(us, mod.dm, mod.dt, 1.0)
    H.rescore(us, mod.dm, mod.dt, 1.0).close()             # the context is usable afterwards
    for o in (bad, H, us, two, other, wide):
        o.close()
    mod2.close(); ctx2.close(); mod.close()


# ---- 7. boost -------------------------------------------------------------------------------------------------------------------
def test_boost_on_the_bits_host_alignment_and_ali_set(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import UtteranceSet
    rng = np.random.default_rng(21)
    nt = 12
    t2p = np.concatenate([[0], 1 + np.arange(nt) // 3]).astype(np.int32)          # phones 1 .. 4; 1 is silence
    lens = [5, 70, 1, 9, 4, 6]
    lats = [sausage([list(rng.choice(nt, 4, replace=False) + 1) for _ in range(T)], seed=T) for T in lens]
    lats[3] = rr.empty()
    alis = [rng.integers(1, nt + 1, T).astype(np.int32) for T in lens]
    alis[1][::3] = 2                                      # silence as the reference on every third frame
    alis[4] = alis[4][:3]                                 # a short alignment
    alis[5][2] = 0                                        # id 0
    want_st = [rr.boost_status(l, nt, a) for l, a in zip(lats, alis)]
    assert want_st == [rr.SUCCEEDED, rr.SUCCEEDED, rr.SUCCEEDED, rr.NO_PATH, rr.NO_REF, rr.NO_REF]
    H = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats], ctx)
    # the resident alignment of a set: an utterance that failed to align holds zeros (utterance 4; its length cannot differ there)
    set_lens = [len(l["frame"]) and int(l["frame"][-1]) for l in lats]
    set_lens[3] = lens[3]
    fo = np.concatenate([[0], np.cumsum(set_lens)]).astype(np.int64)
    flat = np.zeros(int(fo[-1]), np.int32)
    for u, a in enumerate(alis):
        if u != 4:
            flat[fo[u]: fo[u] + len(a)] = a
    us = UtteranceSet(ctx, None, fo, np.zeros((int(fo[-1]), 1), F))
    with pytest.raises(RuntimeError, match="no resident alignment"):
        H.boost(t2p, np.array([1], np.int32), ali_set=us)
    us.upload_ali(flat)
    n = 0
    for b, mse in ((0.1, 0.0), (1.75, 0.5), (0.0, 0.5)):
        A = H.boost(t2p, np.array([1], np.int32), alignment=alis, b=b, max_silence_error=mse)
        S = H.boost(t2p, np.array([1], np.int32), ali_set=us, b=b, max_silence_error=mse)
        assert A.status.tolist() == want_st and S.status.tolist() == want_st
        for u, (ga, gs, lat) in enumerate(zip(A.download(), S.download(), lats)):
            want = rr.boost(lat, t2p, [1], alis[u], b, mse) if want_st[u] == rr.SUCCEEDED else rr.empty()
            _same(ga, want, ("host alignment", b, mse, u))
            _same(gs, want, ("ali_set", b, mse, u))
            if b == 0.0:
                _same(ga, lat if want_st[u] == rr.SUCCEEDED else rr.empty(), ("b = 0", u))
            n += int((want["ilabel"] != 0).sum())
        assert A.best_path([1.0], [1.0])["status"].tolist() == [ops.SUCCEEDED] * 3 + [ops.NO_PATH] * 3
        A.close(); S.close()
    assert n > 800
    for u, got in enumerate(H.download()):
        _same(got, lats[u], ("the input is untouched", u))
    H.close(); us.close()


def test_boost_refusals(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import UtteranceSet
    t2p = np.array([0, 1, 1, 2, 2], np.int32)
    sil = np.array([1], np.int32)
    H = khg.DeviceLattices.from_lattices([_lattice(khg, sausage([[1, 3], [2, 4]]))], ctx)
    ali = [np.array([1, 3], np.int32)]
    us = UtteranceSet(ctx, None, np.array([0, 2], np.int64), np.zeros((2, 1), F))
    us.upload_ali(ali[0])
    H.boost(t2p, sil, alignment=ali).close()
    with pytest.raises(RuntimeError, match="either"):
        H.boost(t2p, sil)
    with pytest.raises(RuntimeError, match="either"):
        H.boost(t2p, sil, alignment=ali, ali_set=us)
    with pytest.raises(RuntimeError, match="finite"):
        H.boost(t2p, sil, alignment=ali, b=float("inf"))
    with pytest.raises(RuntimeError, match="finite"):
        H.boost(t2p, sil, alignment=ali, max_silence_error=float("nan"))
    with pytest.raises(RuntimeError, match="silence phone 7"):
        H.boost(t2p, np.array([1, 7], np.int32), alignment=ali)
    with pytest.raises(RuntimeError, match="ilabel outside"):
        H.boost(t2p[:4], sil, alignment=ali)               # the lattice carries id 4
    with pytest.raises(RuntimeError, match="1 lattices"):
        H.boost(t2p, sil, alignment=ali + ali)
    two = UtteranceSet(ctx, None, np.array([0, 1, 2], np.int64), np.zeros((2, 1), F))
    two.upload_ali(ali[0])
    with pytest.raises(RuntimeError, match="ali_set 2"):
        H.boost(t2p, sil, ali_set=two)
    H.boost(t2p, sil, ali_set=us).close()
    H.close(); us.close(); two.close()


# ---- 8. end to end on the trained YES/NO word loop -------------------------------------------------------------------------------
def test_trained_word_loop_rescored_with_another_model(trained):
    khg, dx, tm, am, graph, test_utts = trained
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    from oracle import oracle as orc
    from test_gpu_acc_stats_post import _lattice_posts_to_stats
    dctx = _gpu.default_context()
    kappa = 0.1
    feats = [np.ascontiguousarray(u[2], F) for u in test_utts]
    U = len(feats)
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    rd, dl = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, cfg, kappa)
    assert all(r["status"] == 1 for r in rd)
    go, gc, w, miv, iv = [np.asarray(x) for x in am.flat()]
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    # model B: the means moved by a twentieth of a standard deviation
    mean_b = miv / iv + 0.05 * np.random.default_rng(1).normal(size=miv.shape) / np.sqrt(iv)
    miv_b = (mean_b * iv).astype(F)
    gc_b = orc.model_gconsts(go.astype(np.int32), w.astype(F), iv.astype(F), miv_b)
    dt = DeviceTransitions(dctx, id2pdf)
    dma = DeviceModel(dctx, go, gc, miv, iv)
    dmb = DeviceModel(dctx, go, gc_b, miv_b, iv)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.concatenate(feats))
    lats = [_dict(x) for x in dl.download()]
    L = dl.download()
    mb = type("M", (), {"gauss_off": go.astype(np.int32), "means_invvars": miv_b, "inv_vars": iv.astype(F)})
    ma = type("M", (), {"gauss_off": go.astype(np.int32), "means_invvars": miv.astype(F), "inv_vars": iv.astype(F)})

    R = dl.rescore(us, dmb, dt, 1.0)
    got = R.download()
    assert _check_cells(None, lats, got, feats, 1.0, "model B", id2pdf=id2pdf, model=(mb, gc_b)) > sum(len(f) for f in feats)
    P = R.posteriors(1.0, kappa)
    assert all(int(s) == 1 for s in P.status)
    for u in range(U):
        # the download rescored on the host with the values the device gave its cells: one value per (frame, id), or the costs differ
        cell = {}
        for t, il, c in zip(rr.arc_frames(lats[u]), lats[u]["ilabel"], np.asarray(got[u].acoustic_cost)):
            if il != 0:
                cell.setdefault((int(t), int(id2pdf[il])), F(-c))
        host = L[u].rescore(lambda t, il: float(cell[(t, int(id2pdf[il]))]), 1.0)
        assert np.asarray(host.acoustic_cost).tobytes() == np.asarray(got[u].acoustic_cost).tobytes(), u
        hd = _dict(host)
        want = pr.forward_backward(hd, 1.0, kappa)
        fb = host.forward_backward(1.0, kappa)
        tol_log, _ = pr.tolerances(want, hd)
        assert abs(float(P.tot_like[u]) - want["tot"]) <= tol_log and abs(fb["tot_like"] - want["tot"]) <= tol_log, u
    P.close()
    amb = type("A", (), {"flat": lambda self: (go, gc_b, w, miv_b, iv)})()
    _lattice_posts_to_stats(khg, amb, tm, R, feats, "word loop rescored with model B")
    R.close()

    # rescored with A itself at scale kappa: the best path's cost at (1, 1) against the decoder's `like`.  Both score sets lie within
    # kappa (1e-5 + 1e-6 B) of float64 per arc (the decoder's are the default K1's), so any path's cost moves by at most twice that
    # per frame, and so does the minimum; the decoder stores fl(cost - offset) and both sides add in float32: four roundings per
    # frame of values no larger than |like| + 1.
    RA = dl.rescore(us, dma, dt, kappa)
    bp = RA.best_path([1.0], [1.0])
    for u in range(U):
        T = len(feats[u])
        _, bd = helpers.exact_loglikes(ma, gc.astype(F), feats[u], list(range(len(go) - 1)))
        bound = 2 * kappa * float((1e-5 + 1e-6 * bd.max(0)).sum()) + 2.0 ** -22 * T * (abs(rd[u]["like"]) + 1)
        v = bp["weight"][u]
        assert int(bp["status"][u]) == 1 and abs(-(float(v[0]) + float(v[1])) - rd[u]["like"]) <= bound, (u, v, rd[u]["like"], bound)
    RA.close()

    # boosted: every arc's cost falls by b e, 0 <= e <= 1, so every path's log-likelihood rises by between 0 and b T, and so does the
    # log of their sum; it does not move where no arc with a posterior is touched, and rises where one with a posterior of 1e-3 or
    # more is.  With the decoder's own best path as the reference these lattices stay as they are (every competing arc carries the
    # reference's phone on its frame), so the same is asked with that path moved five frames on: it disagrees with the lattice's
    # heaviest arcs around every phone boundary.  Silence errors count in full.
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    b, mse = 0.5, 1.0
    sil = np.array([dx.tr.SIL], np.int32)
    own = [np.asarray(r["alignment"], np.int32) for r in rd]
    P0 = dl.posteriors(1.0, kappa)
    arc_post = P0.arc_post()
    for name, refs in (("own best path", own), ("best path moved five frames", [np.roll(a, 5) for a in own])):
        Bd = dl.boost(tid2phone, sil, alignment=refs, b=b, max_silence_error=mse)
        assert Bd.status.tolist() == [1] * U
        P1 = Bd.posteriors(1.0, kappa)
        boosted = Bd.download()
        touched = moved = 0
        for u in range(U):
            want = rr.boost(lats[u], tid2phone, sil, refs[u], b, mse)
            assert np.asarray(boosted[u].graph_cost).tobytes() == want["graph_cost"].tobytes(), (name, u)
            changed = want["graph_cost"] != lats[u]["graph_cost"]
            touched += int(changed.sum())
            d = float(P1.tot_like[u]) - float(P0.tot_like[u])
            assert -1e-9 <= d <= b * len(feats[u]) + 1e-9, (name, u, d)
            heaviest = float(np.asarray(arc_post[u])[changed].max()) if changed.any() else 0.0
            if heaviest == 0.0:
                assert abs(d) <= 1e-9, (name, u, d)
            if heaviest >= 1e-3:
                assert d > 0.0, (name, u, d, heaviest)
                moved += 1
        print("boost, %s: %d arcs touched, tot_like rose for %d of %d utterances" % (name, touched, moved, U))
        if refs is not own:
            assert touched > 0 and moved > 0
        P1.close(); Bd.close()
    for x in (P0, us, dma, dmb, dt, dl):
        x.close()


# ---- the scripts named after the Kaldi programs ---------------------------------------------------------------------------------
def test_scripts_gmm_rescore_lattice_and_lattice_boost_ali(setup):
    khg, synth, m, am, tm, ut = setup
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    t2p = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    nt = tm.num_transition_ids
    rng = np.random.default_rng(31)
    feats = _feats(ut, 2, [7, 40])
    lats = [sausage([list(rng.choice(nt, 3, replace=False) + 1) for _ in range(len(f))], seed=len(f)) for f in feats]
    L = [_lattice(khg, x) for x in lats]
    go, gc, w, miv, iv = am.flat()
    mm = type("M", (), {"gauss_off": np.asarray(go, np.int32), "means_invvars": np.asarray(miv, F), "inv_vars": np.asarray(iv, F)})
    out = khg.gmm_rescore_lattice_batch(am, tm, L, feats, 0.1)
    assert _check_cells(None, lats, out, feats, 0.1, "script", id2pdf=id2pdf, model=(mm, np.asarray(gc, F))) == 3 * 47
    one = khg.gmm_rescore_lattice(am, tm, L[1], feats[1], 0.1)
    assert np.asarray(one.acoustic_cost).tobytes() == np.asarray(out[1].acoustic_cost).tobytes()
    alis = [rng.integers(1, nt + 1, len(f)).astype(np.int32) for f in feats]
    bo = khg.lattice_boost_ali_batch(tm, L, alis, [1], b=0.25, max_silence_error=0.5)
    for u in range(2):
        _same(bo[u], rr.boost(lats[u], t2p, [1], alis[u], 0.25, 0.5), ("boost script", u))
    _same(khg.lattice_boost_ali(tm, L[0], alis[0], [1], 0.25, 0.5), rr.boost(lats[0], t2p, [1], alis[0], 0.25, 0.5), "one")
    dev = khg.DeviceLattices.from_lattices(L)
    R = khg.gmm_rescore_lattice_batch(am, tm, dev, feats, 0.1)
    assert R.rescore_stats["arcs"] == 3 * 47 and np.asarray(R.download()[0].acoustic_cost).tobytes() == np.asarray(out[0].acoustic_cost).tobytes()
    R.close(); dev.close()
