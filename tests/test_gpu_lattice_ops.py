"""Best path under scales and beam pruning of device-resident raw lattices (khg_lattices_best_path / khg_lattices_prune through
DeviceLattices, get_raw_lattice_simple_device_batch and UtteranceSet.raw_lattices_simple_device) against the float32 restatement of
the rule (tests/lattice_ops_ref.py), bit for bit.  The lattices come from K1's own scores on the graphs and
beams of tests/test_gpu_lattice_raw.py (which checks the lattices themselves against their rule); here every operation on them is
compared with the restatement applied to the downloaded lattice."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_raw import OLD_KEYS, _feats, _fst, setup  # noqa: E402,F401
from lattice_geometry_cases import _wide_lattice  # noqa: E402
from test_lattice_ops_cpu import hand_cases  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
WEIGHTS = list(range(7, 18))                                   # the language-model-weight sweep: graph_scale 1, acoustic_scale 1 / w
SWEEP_GS = np.ones(len(WEIGHTS), np.float32)
SWEEP_AS = (1.0 / np.arange(7, 18)).astype(np.float32)
PRUNE_PAIRS = [(1.0, 1.0), (0.5, 1.7)]
BEAMS = [0.0, 0.5, 2.0, float("inf")]


def _dict(L):
    d = {k: np.asarray(getattr(L, k)) for k in ops.FIELDS}
    d["start"] = L.start
    return d


def _entry(bp, k, u, U):
    """pair k, utterance u of DeviceLattices.best_path's dict -> (status, ali, words, weight bits)"""
    o = k * U + u
    ao, wo = bp["ali_off"], bp["words_off"]
    return (int(bp["status"][o]), bp["ali"][k, ao[u]: ao[u + 1]].tolist(), bp["words"][wo[o]: wo[o + 1]].tolist(), ops.bits(bp["weight"][o]))


def _want_entry(lat, gs, as_):
    w = ops.best_path(lat, gs, as_)
    T = int(lat["frame"][-1]) if len(lat["frame"]) else 0
    ali = w["ali"] if w["status"] == ops.SUCCEEDED else [0] * T
    return (w["status"], ali, w["words"], ops.bits(w["weight"]))


def _same_lattice(got, want, tag):
    for k in ops.FIELDS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (tag, k)
    assert got.start == want["start"], tag


class Evidence:
    def __init__(self):
        self.lattices = self.paths = self.sweep_changes = self.pruned_smaller = self.dead = 0

    def __repr__(self):
        return "lattices %d paths %d sweeps that change the path %d prunes that removed something %d lattices with dead states %d" % (
            self.lattices, self.paths, self.sweep_changes, self.pruned_smaller, self.dead)


def _check_ops(khg, dl, lats, ev, decoded=None, sweep=True, beams=BEAMS, pairs=PRUNE_PAIRS):
    """Every operation on the handle `dl` against the restatement on its downloaded lattices `lats` (dicts); decoded: the decoder's
    per-utterance dicts (the best path at (1, 1) is the decoder's)."""
    U = len(lats)
    assert dl.num_utts == U
    assert dl.state_off.tolist() == np.concatenate([[0], np.cumsum([len(x["frame"]) for x in lats])]).tolist()
    assert dl.arc_off.tolist() == np.concatenate([[0], np.cumsum([len(x["ilabel"]) for x in lats])]).tolist()
    one = dl.best_path([1.0], [1.0])
    assert one["ali"].shape == (1, int(one["ali_off"][-1])) and one["weight"].shape == (U, 2) and one["status"].shape == (U,)
    for u, lat in enumerate(lats):
        got = _entry(one, 0, u, U)
        assert got == _want_entry(lat, 1.0, 1.0), u
        ev.lattices += 1
        if decoded is not None:
            r = decoded[u]
            if not r["succeeded"]:
                assert len(lat["frame"]) == 0 and got[0] == ops.NO_PATH and got[2] == [] and one["ali_off"][u + 1] == one["ali_off"][u], u
                continue
            v = one["weight"][u]
            assert got[0] == ops.SUCCEEDED and got[1] == r["alignment"] and got[2] == r["words"], u
            assert float(F(-F(v[0] + v[1]))) == r["like"], (u, v, r["like"])
    if sweep:
        # the 11-weight sweep in one call is 11 single calls, and the restatement's
        many = dl.best_path(SWEEP_GS, SWEEP_AS)
        assert many["ali"].shape[0] == len(WEIGHTS)
        for k in range(len(WEIGHTS)):
            single = dl.best_path(SWEEP_GS[k: k + 1], SWEEP_AS[k: k + 1])
            for u, lat in enumerate(lats):
                e = _entry(many, k, u, U)
                assert e == _entry(single, 0, u, U), (k, u)
                assert e == _want_entry(lat, SWEEP_GS[k], SWEEP_AS[k]), (k, u)
                ev.paths += 1
        for u in range(U):
            ev.sweep_changes += len({tuple(_entry(many, k, u, U)[1]) for k in range(len(WEIGHTS))}) > 1
    for gs, as_ in pairs:
        before = dl.best_path([gs], [as_])
        for beam in beams:
            P = dl.prune(beam, gs, as_)
            assert P.num_utts == U and P.status.shape == (U,)
            got = P.download()
            after = P.best_path([gs], [as_])
            for u, lat in enumerate(lats):
                want, st = ops.prune(lat, beam, gs, as_)
                assert int(P.status[u]) == st, (u, beam, gs, as_)
                _same_lattice(got[u], want, (u, beam, gs, as_))
                # the pruned lattice's best path is the input's (no path: the pruned lattice is empty)
                if _entry(before, 0, u, U)[0] == ops.SUCCEEDED:
                    assert _entry(after, 0, u, U) == _entry(before, 0, u, U), (u, beam, gs, as_)
                else:
                    assert _entry(after, 0, u, U)[:3] == (ops.NO_PATH, [], []) and len(want["frame"]) == 0, (u, beam, gs, as_)
                ev.pruned_smaller += len(want["ilabel"]) < len(lat["ilabel"])
                if beam == float("inf"):
                    ev.dead += len(want["frame"]) < len(lat["frame"])
            P.close()


def _decode(khg, am, tm, fsts, feats, beam, lbeam, scale=0.1, scratch=0):
    cfg = khg.LatticeSimpleDecoderConfig(beam=beam, lattice_beam=lbeam)
    old = khg.decode_lattice_simple_batch(am, tm, fsts, feats, cfg, scale, scratch_per_frame=scratch)
    res, dl = khg.get_raw_lattice_simple_device_batch(am, tm, fsts, feats, cfg, scale, scratch_per_frame=scratch)
    assert isinstance(dl, khg.DeviceLattices) and len(res) == len(old) == len(feats) and dl.device_bytes > 0
    for r, o in zip(res, old):
        assert set(r) == set(OLD_KEYS)
        for k in OLD_KEYS:
            assert r[k] == o[k] and type(r[k]) is type(o[k]), k
    return res, dl


@pytest.mark.parametrize("kind", ["random", "hub"])
@pytest.mark.parametrize("loop_w", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("beams", [(13.0, 6.0), (6.0, 2.0), (16.0, 4.0), (8.0, 1.0)])
def test_graphs_with_self_loops(setup, kind, loop_w, beams):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(int(beams[0] * 10 + beams[1] + 100 * loop_w) + (3 if kind == "hub" else 0))
    n = 6
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if kind == "random"
                                 else tg.hub_graph(rng, m.num_tids, fan=8, tail=5), loop_w) for _ in range(n)]
    res, dl = _decode(khg, am, tm, [_fst(khg, g) for g in gs], _feats(ut, n), *beams)
    lats = [_dict(x) for x in dl.download()]
    ev = Evidence()
    _check_ops(khg, dl, lats, ev, decoded=res)
    print(ev)
    assert ev.lattices == n and ev.paths > 0
    dl.close()


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(setup, T):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(T)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.3), 0.25) for _ in range(4)]
    res, dl = _decode(khg, am, tm, [_fst(khg, g) for g in gs], _feats(ut, 4, [T] * 4), 10.0, 4.0)
    ev = Evidence()
    _check_ops(khg, dl, [_dict(x) for x in dl.download()], ev, decoded=res)
    assert ev.paths > 0, ev


def test_mismatched_model(setup):
    khg, synth, m, am, tm, ut = setup
    mm = synth.mismatched_model(m, 0.5, seed=3)
    am2, tm2 = synth.host_objects(mm)
    rng = np.random.default_rng(9)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=10, p_branch=0.6, p_eps=0.3), 0.25) for _ in range(8)]
    res, dl = _decode(khg, am2, tm2, [_fst(khg, g) for g in gs], _feats(ut, 8), 6.0, 2.0)
    ev = Evidence()
    _check_ops(khg, dl, [_dict(x) for x in dl.download()], ev, decoded=res)
    assert ev.paths > 0, ev


def test_large_graph_batch_equals_one_utterance_batches_and_round_trip(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(1234)
    g = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=1100, p_eps=0.2), 0.25)
    small = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=9, p_eps=0.3), 0.25) for _ in range(3)]
    gs = [g, small[0], g, small[1], small[2]]
    feats = _feats(ut, 5, [60, 30, 40, 20, 25])
    res, dl = _decode(khg, am, tm, [_fst(khg, x) for x in gs], feats, 13.0, 6.0)
    L = dl.download()
    lats = [_dict(x) for x in L]
    ev = Evidence()
    _check_ops(khg, dl, lats, ev, decoded=res, beams=[0.5, float("inf")], pairs=PRUNE_PAIRS[1:])
    print(ev)
    assert ev.pruned_smaller > 0, ev
    # from_lattices(...).download() round-trips, and a batch is its one-utterance batches
    up = khg.DeviceLattices.from_lattices(L)
    for a, b in zip(up.download(), lats):
        _same_lattice(a, b, "round trip")
    many = up.best_path(SWEEP_GS, SWEEP_AS)
    whole = dl.best_path(SWEEP_GS, SWEEP_AS)
    pruned = dl.prune(2.0, 1.0, float(SWEEP_AS[5])).download()
    for u in range(len(L)):
        one = khg.DeviceLattices.from_lattices(L[u: u + 1])
        bp = one.best_path(SWEEP_GS, SWEEP_AS)
        for k in range(len(WEIGHTS)):
            assert _entry(bp, k, 0, 1) == _entry(many, k, u, len(L)) == _entry(whole, k, u, len(L)), (u, k)
        _same_lattice(one.prune(2.0, 1.0, float(SWEEP_AS[5])).download()[0], _dict(pruned[u]), u)
        one.close()
    up.close(); dl.close()


def test_decoding_graph_300_word_loop_at_every_hub_threshold(setup):
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    g = ref.add_eps_self_loops(sg.word_loop_graph(np.random.default_rng(300), m.num_tids, 300, 1), 0.25)
    lens = [40, 24, 25, 26]
    feats = _feats(ut, len(lens), lens)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    default = ctx.get_option("k2s_hub")
    outs = []
    try:
        for thr in (0, 1, 32):
            ctx.set_option("k2s_hub", thr)
            res, dl = _decode(khg, am, tm, dg, feats, 13.0, 6.0)
            lats = [_dict(x) for x in dl.download()]
            if thr == 0:
                ev = Evidence()
                _check_ops(khg, dl, lats, ev, decoded=res, beams=[0.5, float("inf")])
                print(ev)
                assert ev.pruned_smaller > 0, ev
            outs.append((dl.best_path(SWEEP_GS, SWEEP_AS), [_dict(x) for x in dl.prune(2.0, 1.0, 0.1).download()]))
            dl.close()
    finally:
        ctx.set_option("k2s_hub", default)
    for bp, pr in outs[1:]:
        for k in ("ali", "words", "words_off", "weight", "status"):
            assert bp[k].tobytes() == outs[0][0][k].tobytes(), k
        for a, b in zip(pr, outs[0][1]):
            for k in ops.FIELDS:
                assert a[k].tobytes() == b[k].tobytes(), k
    dg.close()


def test_failing_decoder_statuses_stay_empty(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(5)
    base = tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.0)                  # no epsilon arc anywhere: no token at frame -1
    nofinal = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, with_final=False))
    good = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6))
    gs = [base, nofinal, good]
    res, dl = _decode(khg, am, tm, [_fst(khg, g) for g in gs], _feats(ut, 3), 13.0, 6.0)
    assert [r["succeeded"] for r in res] == [False, False, True]
    lats = [_dict(x) for x in dl.download()]
    ev = Evidence()
    _check_ops(khg, dl, lats, ev, decoded=res)
    P = dl.prune(1.0)
    assert P.status.tolist() == [ops.NO_PATH, ops.NO_PATH, ops.SUCCEEDED]
    assert np.diff(P.state_off).tolist()[:2] == [0, 0] and np.diff(P.arc_off).tolist()[:2] == [0, 0]
    got = P.download()
    assert got[0].num_states == 0 and got[0].start == -1 and got[2].num_states > 0
    bp = P.best_path(SWEEP_GS, SWEEP_AS)
    U = 3
    assert all(int(bp["status"][k * U + u]) == ops.NO_PATH for k in range(len(WEIGHTS)) for u in (0, 1))
    assert all(np.isinf(bp["weight"][k * U + u]).all() for k in range(len(WEIGHTS)) for u in (0, 1))
    # a frame over scratch_per_frame: KHG_LAT_SCRATCH and an empty lattice through both operations
    res, dl2 = _decode(khg, am, tm, [_fst(khg, good)], _feats(ut, 3)[2:3], 13.0, 6.0, scratch=1)
    assert not res[0]["succeeded"] and dl2.state_off.tolist() == [0, 0]
    assert int(dl2.best_path([1.0], [1.0])["status"][0]) == ops.NO_PATH and dl2.prune(0.5).state_off.tolist() == [0, 0]


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ops.FIELDS], int(lat["start"]))


def test_hand_built_lattices_through_from_lattices(setup):
    khg = setup[0]
    cases = hand_cases()
    names = sorted(cases)
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, cases[n][0]) for n in names])
    U = len(names)
    for gs, as_ in {(cases[n][1], cases[n][2]) for n in names}:
        bp = dl.best_path([gs], [as_])
        pruned = {beam: dl.prune(beam, gs, as_) for beam in BEAMS}
        for u, n in enumerate(names):
            lat, cgs, cas, status, ali, words = cases[n]
            e = _entry(bp, 0, u, U)
            assert e == _want_entry(lat, gs, as_), (n, gs, as_)
            if (cgs, cas) == (gs, as_):
                assert e[0] == status and e[2] == words and (status != ops.SUCCEEDED or e[1] == ali), n
            for beam, P in pruned.items():
                want, st = ops.prune(lat, beam, gs, as_)
                assert int(P.status[u]) == st, (n, beam)
                _same_lattice(P.download()[u], want, (n, beam))
    # a short words_cap is reported per entry through the C-ABI; what khg_lattices_upload refuses is refused here too
    bad = {k: np.array(v) for k, v in cases["epsilon_chain"][0].items() if k != "start"}
    bad["ilabel"][4] = 0
    with pytest.raises(RuntimeError, match="utterance 0.*epsilon arc"):
        khg.DeviceLattices.from_lattices([_lattice(khg, dict(bad, start=0))])
    with pytest.raises(RuntimeError):
        dl.best_path([-1.0], [1.0])
    with pytest.raises(RuntimeError):
        dl.best_path([1.0], [float("nan")])
    with pytest.raises(RuntimeError):
        dl.prune(-0.5)
    with pytest.raises(RuntimeError):
        dl.prune(float("nan"))
    dl.close()
    with pytest.raises(RuntimeError, match="closed"):
        dl.best_path([1.0], [1.0])


def test_lds_staged_and_hbm_forms_agree(setup):
    """A lattice too large for the LDS-staged form (over 48 KiB of staged arrays) next to small ones, and every lattice again with
    staging switched off (KHG_OPT_LAT_OPS_LDS = 1): the same answers, and the restatement's."""
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    rng = np.random.default_rng(77)
    big = _wide_lattice(rng, 30, 24, 6)
    small = _wide_lattice(rng, 12, 5, 2)
    cases = hand_cases()
    lats = [small, big, cases["epsilon_chain"][0], cases["negative_epsilon_cycle"][0], small]
    need = [4 * (3 * len(x["frame"]) + 4 * len(x["ilabel"])) for x in lats]
    assert need[1] > 48 * 1024 > need[0], need
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    outs = []
    try:
        for opt in (0, 1):
            ctx.set_option("lat_ops_lds", opt)
            if opt == 0:
                ev = Evidence()
                _check_ops(khg, dl, lats, ev, beams=[0.5, float("inf")], pairs=PRUNE_PAIRS[1:])
                print(ev)
                assert ev.pruned_smaller > 0
            outs.append((dl.best_path(SWEEP_GS, SWEEP_AS), [_dict(x) for x in dl.prune(2.0, 0.5, 1.7).download()]))
        with pytest.raises(RuntimeError):
            ctx.set_option("lat_ops_lds", 2)
    finally:
        ctx.set_option("lat_ops_lds", default)
    for k in ("ali", "words", "words_off", "weight", "status"):
        assert outs[0][0][k].tobytes() == outs[1][0][k].tobytes(), k
    for a, b in zip(outs[0][1], outs[1][1]):
        for k in ops.FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), k
    dl.close()


def test_utterance_set_keeps_the_handle(setup):
    """UtteranceSet.raw_lattices_simple_device: raw_lattice_simple's decoder outputs and the same lattices, kept on the device."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    rng = np.random.default_rng(31)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=8, p_eps=0.3), 0.25) for _ in range(3)]
    feats = _feats(ut, 3)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ctx = Context(0)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, fo, np.concatenate(feats), graphs=tg.concat(gs))
    us.loglikes(dm)
    raw_ = us.raw_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    d = us.raw_lattices_simple_device(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    for k in ("ali", "like", "status", "error_frame", "words", "words_off"):
        assert np.asarray(d[k]).tobytes() == np.asarray(raw_[k]).tobytes(), k
    dl = d["lattices"]
    assert dl.state_off.tolist() == raw_["state_off"].tolist() and dl.arc_off.tolist() == raw_["arc_off"].tolist()
    L = dl.download()
    for u in range(3):
        so, ao = raw_["state_off"], raw_["arc_off"]
        assert np.asarray(L[u].graph_cost).tobytes() == raw_["graph_cost"][ao[u]: ao[u + 1]].tobytes()
        assert np.asarray(L[u].tot_cost).tobytes() == raw_["tot_cost"][so[u]: so[u + 1]].tobytes()
    bp = dl.best_path([1.0], [1.0])
    if (np.asarray(d["status"]) == ops.SUCCEEDED).all():
        assert bp["ali"][0].tolist() == np.asarray(d["ali"]).tolist() and bp["words"].tolist() == np.asarray(d["words"]).tolist()
        assert bp["ali_off"].tolist() == fo.tolist()
    ev = Evidence()
    _check_ops(khg, dl, [_dict(x) for x in L], ev, beams=[0.5])
    dl.close(); us.close()
