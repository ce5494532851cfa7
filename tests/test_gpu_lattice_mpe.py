"""MPE / sMBR posteriors of device-resident lattices (khg_lattices_mpe_posteriors through DeviceLattices.mpe_posteriors, DESIGN.md
section 7k) against the plain-Python restatement (tests/lattice_mpe_ref.py): status, offsets, ids and exact zeros equal, values within
the derived tolerance; statuses, structure and tot_like bit-equal to DeviceLattices.posteriors on the same handle; every test prints
its largest error / bound ratio.  The inputs of tests/test_lattice_mpe_cpu.py, lattices the lattice-faster decoder emits on the
device (the reference from host arrays and from an utterance set: equal bits), the LDS staging thresholds with staging on and off,
batches of 64, 65 and 130 utterances with empty and NO_REF ones at the edges, a two-chunk handle, pruned and rescored handles."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_mpe_cases as mc  # noqa: E402
import lattice_mpe_ref as mr  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_cases as pc  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_faster_raw import _decoder_launches, _feats, _fst, _slice_bytes, setup  # noqa: E402,F401
from test_lattice_ops_cpu import _dict  # noqa: E402

pytestmark = pytest.mark.gpu
SIL = np.asarray(mc.SILENCE, np.int32)


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ops.FIELDS], int(lat["start"]))


def _gots(P):
    """DevicePosteriors of mpe_posteriors -> one dict per utterance, as lattice_mpe_ref.compare takes it"""
    st, tl, av, ap, post = P.status, P.tot_like, P.avg_acc, P.arc_post(), P.download()
    fo, eo = P.frame_off, P.entry_off
    assert len(st) == len(tl) == len(av) == len(ap) == len(post) == P.num_utts and len(fo) == len(eo) == P.num_utts + 1 and fo[0] == eo[0] == 0
    for u in range(P.num_utts):
        assert len(post[u]) == fo[u + 1] - fo[u] and sum(len(r) for r in post[u]) == eo[u + 1] - eo[u], u
    return [{"status": int(st[u]), "tot": float(tl[u]), "avg": float(av[u]), "arc_post": ap[u], "post": post[u]} for u in range(P.num_utts)]


def _bits(g):
    return (g["status"], np.float64(g["tot"]).tobytes(), np.float64(g["avg"]).tobytes(), g["arc_post"].tobytes(),
            [[(int(t), np.float64(w).tobytes()) for t, w in row] for row in g["post"]])


def _frame_sums(g, lat, w):
    tol_d = mr.tolerances(w, lat)[2]
    worst = 0.0
    for t, (row, mcnt) in enumerate(zip(g["post"], w["merged"])):
        assert row, t
        worst = max(worst, abs(sum(x for _, x in row)) / (sum(mcnt) * tol_d))
    assert worst <= 1.0, worst
    return worst


def _same_likelihood_part(dl, got, gs, as_, tag):
    """statuses, the list structure, the live flags and tot_like are DeviceLattices.posteriors' on the same handle, on the bits -- for
    every utterance the reference does not rule out"""
    P = dl.posteriors(gs, as_)
    st, tl, post, ap = P.status, P.tot_like, P.download(), P.arc_post()
    for u, g in enumerate(got):
        if g["status"] == mr.NO_REF:
            continue
        assert g["status"] == int(st[u]) and np.float64(g["tot"]).tobytes() == np.float64(tl[u]).tobytes(), (tag, u)
        assert [[int(t) for t, _ in row] for row in g["post"]] == [[int(t) for t, _ in row] for row in post[u]], (tag, u)
        assert len(g["arc_post"]) == len(ap[u]) and ((g["arc_post"] == 0.0) | (ap[u] != 0.0)).all(), (tag, u)
    P.close()


def _check(khg, lats, alis, criterion="smbr", one_sil=True, gs=1.0, as_=1.0, dl=None, tag="", nt=None):
    """upload (or take the handle), mpe_posteriors with one table for the batch, compare every utterance with the restatement
    -> (the per-utterance results, the worst ratio)"""
    own = dl is None
    if own:
        dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    nt = nt or max(mc.num_tids_of(x) for x in lats)
    tid2phone, tid2pdf = mc.tables(nt)
    P = dl.mpe_posteriors(tid2phone, SIL, alignment=[np.asarray(a, np.int32) for a in alis], criterion=criterion, tid2pdf=tid2pdf,
                          one_silence_class=one_sil, graph_scale=gs, acoustic_scale=as_)
    assert isinstance(P, khg.DevicePosteriors) and P.device_bytes >= 8 * sum(len(x["ilabel"]) for x in lats)
    got = _gots(P)
    worst = 0.0
    for u, lat in enumerate(lats):
        w = mc.want(lat, (tid2phone, tid2pdf, np.asarray(alis[u], np.int32)), criterion, one_sil, gs, as_)
        worst = max(worst, mr.compare(got[u], w, lat, (tag, u, criterion, one_sil, gs, as_)))
        if w["status"] == mr.SUCCEEDED:
            worst = max(worst, _frame_sums(got[u], lat, w))
    _same_likelihood_part(dl, got, gs, as_, tag)
    P.close()
    if own:
        dl.close()
    return got, worst


def _cases(names=None):
    cs = [c for c in mc.constructed() if names is None or c[0] in names]
    return [c[1] for c in cs], [c[2][2] for c in cs], [c[0] for c in cs]


@pytest.mark.parametrize("criterion,one_sil", mc.VARIANTS)
def test_constructed_lattices(setup, criterion, one_sil):
    """the hand-built lattices, in-degrees 64 / 65 / 66 / 200 (the hub path), the 70-state epsilon chain, states per utterance 63 / 64 /
    65 / 127 / 128 / 129 / 193, merges across 64-arc tiles, dead states"""
    khg = setup[0]
    lats, alis, names = _cases()
    keep = [i for i, n in enumerate(names) if n != "tile_N5003"]           # (its bound says nothing: test_lattice_mpe_cpu.py)
    lats, alis, names = [lats[i] for i in keep], [alis[i] for i in keep], [names[i] for i in keep]
    assert {len(x["frame"]) for x in lats} >= {63, 64, 65, 129}
    assert {pc.HUB, pc.HUB + 1} <= {int(np.bincount(x["nextstate"]).max()) for x in lats} and "epsilon_chain_70" in names
    worst = 0.0
    for pair in ((1.0, 1.0), (0.5, 1.7)):
        got, w = _check(khg, lats, alis, criterion, one_sil, *pair, tag="constructed")
        assert all(g["status"] == mr.SUCCEEDED for g in got)
        worst = max(worst, w)
    print("device / restatement: worst error / bound %.3g over %d lattices" % (worst, len(lats)))


def test_one_path_is_exact(setup):
    khg = setup[0]
    lat, (tid2phone, tid2pdf, ali) = mc.one_path_reference()
    for criterion, one_sil in mc.VARIANTS:
        got, _ = _check(khg, [lat], [ali], criterion, one_sil, 1.0, 0.1, nt=len(tid2phone) - 1, tag="one path")
        want = sum(mr.arc_acc(lat, mr.pr._arcs(lat), tid2phone, tid2pdf, mc.SILENCE, ali, criterion, one_sil))
        assert got[0]["avg"] == float(want) and (got[0]["arc_post"] == 0.0).all() and all(w == 0.0 for row in got[0]["post"] for _, w in row)


def test_lds_thresholds_staged_and_hbm_forms(setup):
    """the staging threshold of k2_lattice_post_mpe exactly and the next size up, a lattice that k2_lattice_post_fb stages and this
    kernel does not, together and alone; everything again with staging off: the same bits"""
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    e = mc.mpe_lds_edge()
    by_name = {c[0]: c for c in mc.constructed()}
    pick = [by_name["mpe_lds_at"], by_name["lds_small"], by_name["mpe_lds_over"], by_name["post_lds_at"], by_name["post_lds_over"], by_name["lds_at"]]
    assert pick[3][1] is e["post_only"]
    groups = [pick, pick[0:1], pick[2:3], pick[3:4]]
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    outs, worst = [], 0.0
    try:
        for opt in (0, 1):
            ctx.set_option("lat_ops_lds", opt)
            row = []
            for grp in groups:
                got, w = _check(khg, [c[1] for c in grp], [c[2][2] for c in grp], "smbr", True, 1.0, 1.0, tag=("lds", opt))
                worst = max(worst, w)
                row.append([_bits(g) for g in got])
            outs.append(row)
    finally:
        ctx.set_option("lat_ops_lds", default)
    assert outs[0] == outs[1]
    assert outs[0][0][0] == outs[0][1][0] and outs[0][0][2] == outs[0][2][0] and outs[0][0][3] == outs[0][3][0]          # together = alone
    print("worst error / bound %.3g" % worst)


@pytest.mark.parametrize("U", [64, 65, 130])
def test_batches(setup, U):
    """empty and NO_REF utterances (no alignment, a short one, an id out of range) and a refused structure at 0, 63, 64 and last; a
    batch equals its one-utterance handles on the bits; two calls on one handle are bit-identical"""
    khg = setup[0]
    pool = sorted(mc.faster_rule(), key=lambda c: len(c[1]["frame"]))[:40] + [c for c in mc.constructed() if c[0] in pc.hand_built()]
    nt = max(mc.num_tids_of(c[1]) for c in pool)
    lats = [pool[(7 * i) % len(pool)][1] for i in range(U)]
    alis = [pool[(7 * i) % len(pool)][2][2] for i in range(U)]
    edge = sorted({0, 63, 64, U - 1} & set(range(U)))
    want_st = [mr.SUCCEEDED] * U
    for k, at in enumerate(edge + [5, 6, 7, 8]):
        kind = k % 5
        if kind == 0:
            lats[at], alis[at], want_st[at] = ops.empty_lattice(), np.zeros(0, np.int32), mr.NO_PATH
        elif kind == 1:
            alis[at], want_st[at] = np.zeros(0, np.int32), mr.NO_REF
        elif kind == 2:
            alis[at], want_st[at] = alis[at][:-1], mr.NO_REF
        elif kind == 3:
            alis[at] = alis[at].copy()
            alis[at][len(alis[at]) // 2] = nt + 1
            want_st[at] = mr.NO_REF
        else:
            lats[at], alis[at], want_st[at] = pc.eps_self_loop(), np.ones(1, np.int32), mr.EPS_LOOP
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    got, worst = _check(khg, lats, alis, "smbr", True, 1.0, 0.1, dl=dl, nt=nt, tag=("batch", U))
    assert [g["status"] for g in got] == want_st and want_st[0] == mr.NO_PATH and want_st[U - 1] != mr.SUCCEEDED
    assert {mr.NO_PATH, mr.NO_REF, mr.EPS_LOOP, mr.SUCCEEDED} == set(want_st)
    for g in got:
        if g["status"] != mr.SUCCEEDED:
            assert g["tot"] == -np.inf and g["avg"] == 0.0 and len(g["post"]) == 0
    again, _ = _check(khg, lats, alis, "smbr", True, 1.0, 0.1, dl=dl, nt=nt, tag=("batch again", U))
    assert [_bits(g) for g in got] == [_bits(g) for g in again]
    for u in sorted((set(range(0, U, 9)) | {0, 1, 5, 6, 7, 8, 62, 63, 64, U - 2, U - 1}) & set(range(U))):
        one, _ = _check(khg, lats[u: u + 1], alis[u: u + 1], "smbr", True, 1.0, 0.1, nt=nt, tag=("one", u))
        assert _bits(one[0]) == _bits(got[u]), u
    print("worst error / bound %.3g" % worst)
    dl.close()


def _flat_set(ctx, alis, lens):
    """an utterance set whose resident alignment holds `alis` (zeros where one is missing)"""
    from kaldi_hmm_gmm_amd import UtteranceSet
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.zeros(int(fo[-1]), np.int32)
    for u, a in enumerate(alis):
        flat[fo[u]: fo[u] + len(a)] = a
    us = UtteranceSet(ctx, None, fo, np.zeros((int(fo[-1]), 1), np.float32))
    us.upload_ali(flat)
    return us


@pytest.mark.parametrize("max_active", [3, 7000])
def test_lattice_faster_decoder_lattices(setup, max_active):
    """decoder lattices at T = 24; the reference is the decoder's best path (even utterances) or the next utterance's (odd ones: a
    path of another lattice), given as host arrays and resident in an utterance set: equal bits"""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    T, n = 24, 6
    rng = np.random.default_rng(900 + max_active + T)
    gs = [tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) for _ in range(n)]
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, max_active=max_active, min_active=min(200, max_active), lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, [_fst(khg, g) for g in gs], _feats(ut, n, [T] * n), cfg, 0.1)
    lats = [_dict(x) for x in dl.download()]
    ok = [bool(r["succeeded"]) for r in res]
    assert any(ok)
    alis = [np.asarray(res[(u + 1) % n]["alignment"] if u % 2 else res[u]["alignment"], np.int32) for u in range(n)]
    alis = [a if len(a) == T else np.zeros(0, np.int32) for a in alis]
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    tid2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    assert len(tid2pdf) == len(tid2phone) == m.num_tids + 1
    sil = np.asarray([int(tid2phone[1])], np.int32)
    us = _flat_set(ctx, alis, [T] * n)
    worst = 0.0
    for criterion, one_sil in mc.VARIANTS:
        A = dl.mpe_posteriors(tid2phone, sil, alignment=alis, criterion=criterion, tid2pdf=tid2pdf, one_silence_class=one_sil, acoustic_scale=0.1)
        S = dl.mpe_posteriors(tid2phone, sil, ali_set=us, criterion=criterion, tid2pdf=tid2pdf, one_silence_class=one_sil, acoustic_scale=0.1)
        ga, gset = _gots(A), _gots(S)
        assert [_bits(g) for g in ga] == [_bits(g) for g in gset]
        for u, lat in enumerate(lats):
            w = mr.forward_backward_mpe(lat, tid2phone, tid2pdf, (int(sil[0]),), alis[u], criterion, one_sil, 1.0, 0.1)
            worst = max(worst, mr.compare(ga[u], w, lat, (max_active, criterion, one_sil, u)))
            if w["status"] == mr.SUCCEEDED:
                assert len(ga[u]["post"]) == T and 0.0 <= ga[u]["avg"] <= T
                worst = max(worst, _frame_sums(ga[u], lat, w))
        _same_likelihood_part(dl, ga, 1.0, 0.1, ("decoder", max_active))
        A.close(); S.close()
    print("worst error / bound %.3g; arcs %s" % (worst, [len(x["ilabel"]) for x in lats]))
    us.close(); dl.close()


def test_pruned_handles_and_the_index_is_built_once(setup):
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    cs = mc.faster_rule()[:30]
    lats, alis = [c[1] for c in cs], [c[2][2] for c in cs]
    nt = max(mc.num_tids_of(x) for x in lats)
    tid2phone, tid2pdf = mc.tables(nt)
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    call = lambda h: h.mpe_posteriors(tid2phone, SIL, alignment=alis, criterion="mpfe", tid2pdf=None)  # noqa: E731
    (P0, names) = _decoder_launches(ctx, lambda: call(dl))
    assert names.count("k2_lattice_post_index") == dl.num_chunks and "k2_lattice_post_mpe" in names and "k2_lattice_post_fb" not in names
    (P1, names) = _decoder_launches(ctx, lambda: call(dl))
    assert "k2_lattice_post_index" not in names and "k2_lattice_post_mpe" in names and "k2_lattice_post_fill" in names
    assert [_bits(g) for g in _gots(P0)] == [_bits(g) for g in _gots(P1)]
    P0.close(); P1.close()
    Pr = dl.prune(0.5)
    pruned = [_dict(x) for x in Pr.download()]
    assert sum(len(x["ilabel"]) for x in pruned) < sum(len(x["ilabel"]) for x in lats)
    # a pruned lattice keeps its frames, so the references still fit
    got, worst = _check(khg, pruned, alis, "mpfe", False, 1.0, 1.0, dl=Pr, nt=nt, tag="pruned")
    assert all(g["status"] == mr.SUCCEEDED for g in got)
    print("worst error / bound %.3g" % worst)
    Pr.close(); dl.close()


def test_rescored_handles(setup):
    """rescore (cells) then mpe_posteriors with the reference resident in the rescoring set: the downloaded rescored lattices through
    the restatement"""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    ctx = _gpu.default_context()
    T, n = 24, 4
    rng = np.random.default_rng(77)
    gs = [tg.random_graph(rng, m.num_tids, n_main=10, p_eps=0.3) for _ in range(n)]
    feats = _feats(ut, n, [T] * n)
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, [_fst(khg, g) for g in gs], feats, cfg, 0.1)
    assert all(r["succeeded"] for r in res)
    go, gc, w, miv, iv = am.flat()
    tid2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    dm, dt = DeviceModel(ctx, go, gc, miv, iv), DeviceTransitions(ctx, tid2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    alis = [np.asarray(r["alignment"], np.int32) for r in res]
    us.upload_ali(np.concatenate(alis))
    R = dl.rescore(us, dm, dt, 1.0)
    P = R.mpe_posteriors(tid2phone, np.asarray([int(tid2phone[1])], np.int32), ali_set=us, criterion="smbr", tid2pdf=tid2pdf, acoustic_scale=0.1)
    got = _gots(P)
    worst = 0.0
    for u, x in enumerate(R.download()):
        lat = _dict(x)
        wnt = mr.forward_backward_mpe(lat, tid2phone, tid2pdf, (int(tid2phone[1]),), alis[u], "smbr", True, 1.0, 0.1)
        worst = max(worst, mr.compare(got[u], wnt, lat, ("rescored", u)))
    _same_likelihood_part(R, got, 1.0, 0.1, "rescored")
    print("worst error / bound %.3g" % worst)
    for o in (P, R, us, dm, dt, dl):
        o.close()


def test_bad_arguments_and_closed_handles(setup):
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    lat, (tid2phone, tid2pdf, ali) = mc.one_path_reference()
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, lat)])
    kw = dict(alignment=[ali], tid2pdf=tid2pdf)
    for gs, as_ in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("inf"))):
        with pytest.raises(RuntimeError, match="finite and >= 0"):
            dl.mpe_posteriors(tid2phone, SIL, graph_scale=gs, acoustic_scale=as_, **kw)
    with pytest.raises(RuntimeError, match="criterion"):
        dl.mpe_posteriors(tid2phone, SIL, criterion="mmi", **kw)
    with pytest.raises(RuntimeError, match="tid2pdf"):
        dl.mpe_posteriors(tid2phone, SIL, alignment=[ali], criterion="smbr")
    with pytest.raises(RuntimeError, match="either"):
        dl.mpe_posteriors(tid2phone, SIL, tid2pdf=tid2pdf)
    with pytest.raises(RuntimeError, match="silence phone 99"):
        dl.mpe_posteriors(tid2phone, np.asarray([99], np.int32), **kw)
    with pytest.raises(RuntimeError, match="ilabel outside"):
        dl.mpe_posteriors(tid2phone[:4], SIL, alignment=[ali], criterion="mpfe")
    with pytest.raises(RuntimeError, match="1 lattices"):
        dl.mpe_posteriors(tid2phone, SIL, alignment=[ali, ali], tid2pdf=tid2pdf)
    us = _flat_set(ctx, [ali], [len(ali)])
    P = dl.mpe_posteriors(tid2phone, SIL, ali_set=us, tid2pdf=tid2pdf)
    assert P.status.tolist() == [mr.SUCCEEDED] and P.frame_off.tolist() == [0, 7] and P.entry_off.tolist() == [0, 7] and P.avg_acc.tolist() == [5.0]
    plain = dl.posteriors()
    assert plain.avg_acc is None
    plain.close()
    P.close()
    with pytest.raises(RuntimeError, match="closed"):
        P.download()
    empty = khg.DeviceLattices.from_lattices([])
    E = empty.mpe_posteriors(tid2phone, SIL, alignment=[], tid2pdf=tid2pdf)
    assert E.num_utts == 0 and E.download() == [] and E.arc_post() == [] and len(E.avg_acc) == 0
    E.close(); empty.close(); us.close(); dl.close()
    with pytest.raises(RuntimeError, match="closed"):
        dl.mpe_posteriors(tid2phone, SIL, **kw)


def test_two_chunks(setup):
    """the two-chunk construction of tests/test_gpu_lattice_post.py::test_two_chunks: the two-chunk handle equals the one-chunk
    sub-batches on the bits; a sample of utterances (the chunk edges among them) against the restatement"""
    khg, synth, m, am, tm, ut = setup
    g = sg.word_loop_graph(np.random.default_rng(sg.BIG_W), m.num_tids, sg.BIG_W, sg.BIG_CHAIN)
    S, A = len(g["final"]), len(g["ilabel"])
    lens3 = [12, 11, 13]
    hb = max(1000, int(np.float32(S) * np.float32(2.0))) + 1
    U = int((4 << 30) // min(_slice_bytes(T, S, A, hb) for T in lens3)) + 9
    lens = [lens3[u % 3] for u in range(U)]
    feats = _feats(ut, U, lens)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=8.0, max_active=100, min_active=0, lattice_beam=4.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    co = dl.chunk_off
    assert dl.num_chunks >= 2 and co[0] == 0 and co[-1] == U
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    tid2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    sil = np.asarray([int(tid2phone[1])], np.int32)
    alis = [np.asarray(res[u + 3 if u + 3 < U else u - 3]["alignment"], np.int32) for u in range(U)]          # (u +- 3 has u's frame count)
    call = lambda h, a: h.mpe_posteriors(tid2phone, sil, alignment=a, criterion="smbr", tid2pdf=tid2pdf, acoustic_scale=0.1)  # noqa: E731
    P = call(dl, alis)
    got = _gots(P)
    assert all(x["status"] == mr.SUCCEEDED for x in got)
    lats = dl.download()
    worst = 0.0
    for u in sorted({0, 1, co[1] - 1, co[1], co[1] + 1, U - 1} | set(range(0, U, max(1, U // 12)))):
        lat = _dict(lats[u])
        w = mr.forward_backward_mpe(lat, tid2phone, tid2pdf, (int(sil[0]),), alis[u], "smbr", True, 1.0, 0.1)
        worst = max(worst, mr.compare(got[u], w, lat, ("two chunks", u)))
    _same_likelihood_part(dl, got, 1.0, 0.1, "two chunks")
    for a, b in zip(co, co[1:]):
        r1, d1 = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats[a:b], cfg, 0.1)
        assert d1.num_chunks == 1
        P1 = call(d1, alis[a:b])
        assert [_bits(x) for x in _gots(P1)] == [_bits(x) for x in got[a:b]], (a, b)
        P1.close(); d1.close()
    print("worst error / bound %.3g over a sample of %d utterances in %d chunks" % (worst, U, dl.num_chunks))
    P.close(); dl.close(); dg.close()
