"""The launch geometry of the lattice operations on the GPU (K2O; khg_lattices_best_path / khg_lattices_prune
through DeviceLattices), on the inputs of tests/lattice_geometry_cases.py: more scale pairs than a wave, lanes of one wave that
disagree and fail differently, more utterances than a tile of the scans and than the fill's stripe budget, kept and dropped states
either side of every 64-state tile edge, the LDS staging threshold, and handles of several chunks out of the decoder.  Every
comparison is on the bits, against the float32 restatement (tests/lattice_ops_ref.py) or against answers the restatement has checked;
every count used as a condition comes from the restatement.  Each test prints what shows its case was reached, and its wall time.

State: written and checked against a host stand-in for DeviceLattices only; no run on an MI355X yet (Numbers)."""
import os
import sys
import time
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_geometry_cases as gc  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_ops import (SWEEP_AS, SWEEP_GS, WEIGHTS, Evidence, _check_ops, _dict, _entry, _lattice, _same_lattice,  # noqa: E402,F401
                                  setup)
from test_gpu_lattice_raw import OLD_KEYS, _fst  # noqa: E402
from test_gpu_shared_graph import _path_feats  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
OUT_KEYS = ("ali", "words", "words_off", "weight", "status")


@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.time()
    yield
    print("wall time of %s: %.1f s" % (request.node.name, time.time() - t0))


def _want(lat, gs, as_):
    """the restatement's entry (cached per lattice and pair) in _entry's form"""
    w = gc.want_best_path(lat, gs, as_)
    T = int(lat["frame"][-1]) if len(lat["frame"]) else 0
    return (w["status"], w["ali"] if w["status"] == ops.SUCCEEDED else [0] * T, w["words"], ops.bits(w["weight"]))


def _host_entry(L, gs, as_):
    """the host Lattice's entry (bit-checked against the restatement by the CPU tests)"""
    b = L.best_path(float(gs), float(as_))
    T = int(L.frame[-1]) if L.num_states else 0
    return (b["status"], b["ali"] if b["status"] == ops.SUCCEEDED else [0] * T, b["words"], ops.bits(b["weight"]))


def _same_outputs(a, b, tag):
    for k in OUT_KEYS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (tag, k)


def _same_handles(a, b, tag):
    """two lists of downloaded lattices, every array on the bits"""
    assert len(a) == len(b), tag
    for u, (x, y) in enumerate(zip(a, b)):
        _same_lattice(x, _dict(y), (tag, u))


def _words_are_packed(bp, K, U):
    wo = bp["words_off"]
    assert wo.shape == (K * U + 1,) and wo[0] == 0 and (np.diff(wo) >= 0).all() and int(wo[-1]) == len(bp["words"])


@pytest.fixture(scope="module")
def rule_handle(setup):
    khg = setup[0]
    lats = [x for x in gc.many_utterances() if len(x["frame"])]
    assert len(lats) == 157
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    yield lats, dl
    dl.close()


# ---- pairs beyond one wave, lanes that disagree ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 65, 130])
def test_more_pairs_than_a_wave_on_157_utterances(setup, rule_handle, K):
    """k2_lattice_best_path at gridDim.y = 1 full (K = 64), 2 with one lane (65) and 3 (130): every (pair, utterance) entry equals
    the restatement; the lanes of one wave hold different paths (counted from the restatement)."""
    lats, dl = rule_handle
    U = len(lats)
    gs, as_ = gc.wide_sweeps()[K]
    bp = dl.best_path(gs, as_)
    assert bp["ali"].shape[0] == K and bp["status"].shape == (K * U,) and bp["weight"].shape == (K * U, 2)
    _words_are_packed(bp, K, U)
    for k in range(K):
        for u, lat in enumerate(lats):
            assert _entry(bp, k, u, U) == _want(lat, gs[k], as_[k]), (K, k, u)
    waves = [(lo, min(lo + 64, K)) for lo in range(0, K, 64)]
    per_wave = [sum(gc.distinct_paths(lat, gs, as_, lo, hi) > 1 for lat in lats) for lo, hi in waves]
    most = max(gc.distinct_paths(lat, gs, as_, lo, hi) for lat in lats for lo, hi in waves)
    print("K %d: gridDim.y %d; lattices (of %d) with more than one path inside wave %s: %s; most paths in one wave %d; entries %d, words %d" % (
        K, len(waves), U, waves, per_wave, most, K * U, len(bp["words"])))
    assert all(2 * n >= U for n, (lo, hi) in zip(per_wave, waves) if hi - lo == 64), per_wave
    assert K * U == len(bp["status"]) and (K < 130 or K * U > 20000)


def test_130_pairs_in_one_call_equal_130_one_pair_calls(setup, rule_handle):
    lats, dl = rule_handle
    U = len(lats)
    gs, as_ = gc.wide_sweeps()[130]
    many = dl.best_path(gs, as_)
    sample = list(range(0, U, 13)) + [63, 64, 65, U - 1]
    assert len(set(sample)) >= 10
    changed = 0
    for k in range(130):
        single = dl.best_path(gs[k: k + 1], as_[k: k + 1])
        for u in sample:
            assert _entry(many, k, u, U) == _entry(single, 0, u, U), (k, u)
    for u in sample:
        changed += len({tuple(_entry(many, k, u, U)[1]) for k in range(130)}) > 1
    print("sample %s: utterances whose alignment changes over the 130 pairs: %d of %d" % (sample, changed, len(sample)))
    assert changed > 0


def test_eleven_weight_sweep_changes_the_path(setup, rule_handle):
    """Evidence.sweep_changes of the plain 11-weight sweep, asserted: the lanes of that sweep do not all agree"""
    lats, dl = rule_handle
    U = len(lats)
    many = dl.best_path(SWEEP_GS, SWEEP_AS)
    want_changes = sum(len({tuple(gc.want_best_path(lat, SWEEP_GS[k], SWEEP_AS[k])["arcs"]) for k in range(len(WEIGHTS))}) > 1 for lat in lats)
    got_changes = 0
    for u, lat in enumerate(lats):
        for k in range(len(WEIGHTS)):
            assert _entry(many, k, u, U) == _want(lat, SWEEP_GS[k], SWEEP_AS[k]), (k, u)
        got_changes += len({tuple(_entry(many, k, u, U)[1]) for k in range(len(WEIGHTS))}) > 1
    print("11-weight sweep: the restatement's path changes in %d of %d lattices, the device's alignment in %d" % (want_changes, U, got_changes))
    assert want_changes > 0 and got_changes > 0


def test_mixed_statuses_within_one_wave(setup):
    """SUCCEEDED and KHG_LAT_EPS_LOOP on alternate lanes of one wave for one utterance, KHG_LAT_NO_PATH on every lane of another, a
    path on every lane of the rest: statuses come out per entry, failed entries keep zero alignment rows, no words, infinite sums."""
    khg = setup[0]
    names, lats, gs, as_, want = gc.mixed_status_sweep()
    K, U = len(gs), len(lats)
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    bp = dl.best_path(gs, as_)
    _words_are_packed(bp, K, U)
    ao, wo = bp["ali_off"], bp["words_off"]
    seen = {}
    for k in range(K):
        for u, lat in enumerate(lats):
            o = k * U + u
            st = int(bp["status"][o])
            assert st == want[k][u], (k, names[u])
            assert _entry(bp, k, u, U) == _want(lat, gs[k], as_[k]), (k, names[u])
            seen[(u, k // 64, st)] = seen.get((u, k // 64, st), 0) + 1
            if st != ops.SUCCEEDED:
                assert (bp["ali"][k, ao[u]: ao[u + 1]] == 0).all() and wo[o + 1] == wo[o] and np.isinf(bp["weight"][o]).all(), (k, names[u])
    print("entries by (utterance, wave, status):", sorted(seen.items()))
    for wave in (0, 1, 2):
        assert seen[(0, wave, ops.SUCCEEDED)] > 0 and seen[(0, wave, ops.EPS_LOOP)] > 0 and seen[(2, wave, ops.NO_PATH)] > 0
    # the same pairs one at a time
    for k in (0, 1, 2, 3, 64, 65, 129):
        single = dl.best_path(gs[k: k + 1], as_[k: k + 1])
        for u in range(U):
            assert _entry(single, 0, u, U) == _entry(bp, k, u, U), (k, u)
    # pruning under a pair that loops: an empty lattice and the status, beside utterances that prune
    P = dl.prune(0.5, 1.0, 1.0)
    wst = [gc.want_prune(lat, 0.5, 1.0, 1.0)[1] for lat in lats]
    assert wst == [ops.EPS_LOOP, ops.SUCCEEDED, ops.NO_PATH, ops.SUCCEEDED] and P.status.tolist() == wst
    got = P.download()
    for u, lat in enumerate(lats):
        pr, st = gc.want_prune(lat, 0.5, 1.0, 1.0)
        _same_lattice(got[u], pr, names[u])
    P.close(); dl.close()


# ---- more than 64 utterances: the carries of the scans ----------------------------------------------------------------------------
BEAMS3 = [0.0, 0.5, INF]


@pytest.mark.parametrize("U", gc.UTT_CUTS)
def test_more_utterances_than_a_tile_of_the_scans(setup, U):
    """U = 64, 65, 129, 162 of the rule lattices with empty ones at 0, 63, 64, 65 (and last): k2_lattice_scan_pairs,
    k2_lattice_ops_scan and k2_lattice_ops_last_frame carry a total from one 64-wide tile to the next."""
    khg = setup[0]
    lats = gc.many_utterances()[:U]
    host = [_lattice(khg, x) for x in lats]
    dl = khg.DeviceLattices.from_lattices(host)
    assert dl.num_chunks == 1 and dl.chunk_off == [0, U]
    ev = Evidence()
    # status, state_off, arc_off, every downloaded array at beams 0, 0.5, +inf; prune(...).best_path equals the input's; the sweep
    _check_ops(khg, dl, lats, ev, beams=BEAMS3, pairs=[(1.0, 1.0)])
    kept = [len(gc.want_prune(x, 0.5, 1.0, 1.0)[0]["frame"]) for x in lats]
    tiles = [(sum(kept[t: t + 64]), sum(len(x["frame"]) for x in lats[t: t + 64])) for t in range(0, U, 64)]
    print("U %d: tiles of the utterance scans %d, (kept, input) states per tile at beam 0.5 %s; %s" % (U, len(tiles), tiles, ev))
    assert all(0 < k < n for k, n in tiles if n) and ev.pruned_smaller > 0 and ev.sweep_changes > 0
    # a batch equals its one-utterance handles
    many = dl.best_path(SWEEP_GS, SWEEP_AS)
    P = dl.prune(0.5, 1.0, 1.0)
    pruned = P.download()
    for u in sorted(x for x in {0, 1, 62, 63, 64, 65, 66, U - 2, U - 1} if x < U):
        one = khg.DeviceLattices.from_lattices(host[u: u + 1])
        bp = one.best_path(SWEEP_GS, SWEEP_AS)
        for k in range(len(WEIGHTS)):
            assert _entry(bp, k, 0, 1) == _entry(many, k, u, U), (u, k)
        Q = one.prune(0.5, 1.0, 1.0)
        assert Q.status.tolist() == [int(P.status[u])]
        _same_lattice(Q.download()[0], _dict(pruned[u]), u)
        Q.close(); one.close()
    P.close(); dl.close()


def test_more_utterances_than_the_stripe_budget_of_the_fill(setup):
    """At least 4100 utterances: 4096 / n is 0, so k2_lattice_prune_fill runs with one stripe per utterance; 65 tiles of the scans."""
    khg = setup[0]
    distinct, idx = gc.thousands_of_utterances()
    U = len(idx)
    hostd = [_lattice(khg, x) for x in distinct]
    dl = khg.DeviceLattices.from_lattices([hostd[i] for i in idx])
    assert dl.num_utts == U >= 4100 and dl.num_chunks == 1
    ns, na = [len(x["frame"]) for x in distinct], [len(x["ilabel"]) for x in distinct]
    assert dl.state_off.tolist() == np.concatenate([[0], np.cumsum([ns[i] for i in idx])]).tolist()
    assert dl.arc_off.tolist() == np.concatenate([[0], np.cumsum([na[i] for i in idx])]).tolist()
    gsK = np.concatenate([[1.0], SWEEP_GS]).astype(F)
    asK = np.concatenate([[1.0], SWEEP_AS]).astype(F)
    K = len(gsK)
    bp = dl.best_path(gsK, asK)
    _words_are_packed(bp, K, U)
    want = [[_want(x, gsK[k], asK[k]) for x in distinct] for k in range(K)]
    statuses = set()
    for k in range(K):
        for u, i in enumerate(idx):
            e = _entry(bp, k, u, U)
            assert e == want[k][i], (k, u, i)
            statuses.add(e[0])
    assert statuses == {ops.SUCCEEDED, ops.NO_PATH, ops.EPS_LOOP}
    before = dl.best_path([1.0], [1.0])
    removed = 0
    for beam in BEAMS3:
        P = dl.prune(beam, 1.0, 1.0)
        wp = [gc.want_prune(x, beam, 1.0, 1.0) for x in distinct]
        assert P.status.tolist() == [wp[i][1] for i in idx], beam
        assert P.state_off.tolist() == np.concatenate([[0], np.cumsum([len(wp[i][0]["frame"]) for i in idx])]).tolist(), beam
        assert P.arc_off.tolist() == np.concatenate([[0], np.cumsum([len(wp[i][0]["ilabel"]) for i in idx])]).tolist(), beam
        got = P.download()
        after = P.best_path([1.0], [1.0])
        for u, i in enumerate(idx):
            _same_lattice(got[u], wp[i][0], (beam, u, i))
            if wp[i][1] == ops.SUCCEEDED:
                assert _entry(after, 0, u, U) == _entry(before, 0, u, U), (beam, u)
            else:
                assert _entry(after, 0, u, U)[:3] == (ops.NO_PATH, [], []), (beam, u)
        removed += int(P.state_off[-1]) < int(dl.state_off[-1])
        P.close()
    gy = max(1, min((max(ns) + 63) // 64, max(1, 4096 // U)))
    print("U %d: 4096 / U = %d, stripes of the fill %d, tiles of the utterance scans %d, K U = %d entries, prunes that removed states %d of 3" % (
        U, 4096 // U, gy, (U + 63) // 64, K * U, removed))
    assert gy == 1 and removed > 0
    # a batch equals its one-utterance handles, on a sample across the tiles
    for u in (0, 63, 64, 4095, 4096, 4097, U - 1):
        one = khg.DeviceLattices.from_lattices([hostd[idx[u]]])
        b1 = one.best_path(gsK, asK)
        for k in range(K):
            assert _entry(b1, k, 0, 1) == _entry(bp, k, u, U), (u, k)
        one.close()
    dl.close()


# ---- tile edges inside an utterance, stripes of the fill ----------------------------------------------------------------------------
def _prune_both_forms(ctx, dl, beam, gs, as_):
    """prune with staging on and staging off -> [(status, state_off, arc_off, downloaded lattices)] for lat_ops_lds 0 and 1"""
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    outs = []
    try:
        for opt in (0, 1):
            ctx.set_option("lat_ops_lds", opt)
            P = dl.prune(beam, gs, as_)
            outs.append((P.status.tolist(), P.state_off.tolist(), P.arc_off.tolist(), P.download(), P.best_path(SWEEP_GS, SWEEP_AS)))
            P.close()
    finally:
        ctx.set_option("lat_ops_lds", default)
    return outs


def _tile_checks(khg, ctx, items, tag):
    """items: [(lattice, beam, gs, as_)] sharing one (beam, pair), in one handle"""
    lats = [x[0] for x in items]
    _, beam, gs, as_ = items[0]
    assert all(x[1:] == items[0][1:] for x in items)
    U = len(lats)
    dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
    outs = _prune_both_forms(ctx, dl, beam, gs, as_)
    wp = [gc.want_prune(x, beam, gs, as_) for x in lats]
    for opt, (st, so, ao, got, bp) in enumerate(outs):
        assert st == [w[1] for w in wp] == [ops.SUCCEEDED] * U, (tag, opt)
        assert so == np.concatenate([[0], np.cumsum([len(w[0]["frame"]) for w in wp])]).tolist(), (tag, opt)
        assert ao == np.concatenate([[0], np.cumsum([len(w[0]["ilabel"]) for w in wp])]).tolist(), (tag, opt)
        for u in range(U):
            _same_lattice(got[u], wp[u][0], (tag, opt, u))
    _same_outputs(outs[0][4], outs[1][4], tag)
    # the pruned lattice's best path is the input's, and the input's is the restatement's, staged and not
    default = ctx.get_option("lat_ops_lds")
    try:
        for opt in (0, 1):
            ctx.set_option("lat_ops_lds", opt)
            bp = dl.best_path(SWEEP_GS, SWEEP_AS)
            for k in range(len(WEIGHTS)):
                for u, lat in enumerate(lats):
                    assert _entry(bp, k, u, U) == _want(lat, SWEEP_GS[k], SWEEP_AS[k]), (tag, opt, k, u)
            one = dl.best_path([gs], [as_])
            P = dl.prune(beam, gs, as_)
            after = P.best_path([gs], [as_])
            for u in range(U):
                assert _entry(after, 0, u, U) == _entry(one, 0, u, U), (tag, opt, u)
            P.close()
    finally:
        ctx.set_option("lat_ops_lds", default)
    max_n = max(len(x["frame"]) for x in lats)
    gy = max(1, min((max_n + 63) // 64, max(1, 4096 // U)))
    for u, lat in enumerate(lats):
        tc = gc.tile_counts(lat, wp[u][0]["kept_states"])
        keep = set(wp[u][0]["kept_states"])
        N = len(lat["frame"])
        assert all((k > 0 and d > 0) or k + d == 1 for k, d in tc), (tag, N, tc)
        assert all(((e - 1) in keep) != (e in keep) for e in range(64, N, 64)), (tag, N)
        print("%s: N %d, staged bytes %d (%s), tiles %d, kept / dropped per tile %s%s" % (
            tag, N, gc.staged_bytes(lat), "staged" if gc.staged_bytes(lat) <= gc.LDS_LIMIT else "read from HBM", len(tc), tc[:4],
            " ... %s" % (tc[-1],) if len(tc) > 4 else ""))
    print("%s: utterances %d, stripes of the fill (gridDim.y) %d" % (tag, U, gy))
    dl.close()
    return gy


def test_tile_edges_inside_an_utterance(setup):
    """N = 63, 64, 65, 127, 128, 129, 193 and 5003 states, kept and dropped states in every 64-state tile and a change of fate across
    every tile edge: the ranks k2_lattice_prune_mark carries from tile to tile (sbase, abase), with staging on and off; together in
    one handle and each alone (gridDim.y of the fill = the lattice's own tiles, 79 for the largest)."""
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    items = gc.tile_edge_lattices()
    assert _tile_checks(khg, ctx, items, "together") == 79
    gys = [_tile_checks(khg, ctx, [it], "alone") for it in items]
    assert gys == [1, 1, 2, 2, 2, 3, 4, 79], gys


def test_stripes_of_the_fill_bounded_by_the_utterance_count(setup):
    """The 5003-state lattice after the 162 utterances of many_utterances(): gridDim.y = min(79, 4096 / 163) = 25, so a stripe of
    k2_lattice_prune_fill walks more than one tile; and in the middle of a handle of 70, where 4096 / 70 = 58."""
    khg = setup[0]
    big, beam, gs, as_ = gc.tile_edge_lattices()[-1]
    for lats in (gc.many_utterances() + [big], gc.many_utterances()[:35] + [big] + gc.many_utterances()[35:69]):
        U = len(lats)
        dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
        P = dl.prune(beam, gs, as_)
        got = P.download()
        for u, lat in enumerate(lats):
            pr, st = gc.want_prune(lat, beam, gs, as_)
            assert int(P.status[u]) == st, u
            _same_lattice(got[u], pr, u)
        max_n = max(len(x["frame"]) for x in lats)
        gy = max(1, min((max_n + 63) // 64, max(1, 4096 // U)))
        print("U %d, largest lattice %d states (%d tiles): stripes of the fill %d" % (U, max_n, (max_n + 63) // 64, gy))
        assert 1 < gy < (max_n + 63) // 64
        P.close(); dl.close()


# ---- the staging threshold ---------------------------------------------------------------------------------------------------------
def test_lds_staging_threshold(setup):
    """Staged arrays of exactly 49152 bytes (staged), 49156 (the next size: read from HBM) and 3.5 kB in one handle; the over-size
    lattice alone (the launch asks for 0 bytes of LDS); an empty lattice beside a staged one.  The restatement's answers, and the
    same with staging switched off."""
    khg = setup[0]
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    L = gc.lds_edge_lattices()
    handles = {"three sizes": [L["small"], L["at"], L["over"]], "over alone": [L["over"]], "empty beside staged": [ops.empty_lattice(), L["at"]],
               "at alone": [L["at"]]}
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    for name, lats in handles.items():
        need = [gc.staged_bytes(x) for x in lats]
        lds = max([n for n in need if n <= gc.LDS_LIMIT] + [0])
        dl = khg.DeviceLattices.from_lattices([_lattice(khg, x) for x in lats])
        outs = []
        try:
            for opt in (0, 1):
                ctx.set_option("lat_ops_lds", opt)
                ev = Evidence()
                _check_ops(khg, dl, lats, ev, beams=[0.5, INF], pairs=[(0.5, 1.7)])
                P = dl.prune(2.0, 0.5, 1.7)
                outs.append((dl.best_path(SWEEP_GS, SWEEP_AS), P.download()))
                P.close()
        finally:
            ctx.set_option("lat_ops_lds", default)
        _same_outputs(outs[0][0], outs[1][0], name)
        _same_handles(outs[0][1], outs[1][1], name)
        print("%s: staged bytes per utterance %s, dynamic LDS of the launch %d; %s" % (name, need, lds, ev))
        assert ev.pruned_smaller > 0
        dl.close()
    assert gc.staged_bytes(L["at"]) == 48 * 1024 and gc.staged_bytes(L["over"]) == 48 * 1024 + 4


# ---- more than one chunk out of the decoder ----------------------------------------------------------------------------------------
def test_more_than_one_chunk(setup):
    """165 utterances on the 66 001-state word loop (one shared DecodingGraph): the decoder's scratch passes 4 GiB twice, so the
    batch is decoded in three launches and every kernel of K2S, K2R and K2O runs with u0 > 0, s_base > 0, a_base > 0 on a handle of
    three chunks.  The decoder's restatement takes minutes per utterance on this graph; the yardstick for the decode is the same
    utterances in sub-batches of one chunk each (cut at the chunk boundaries and at shifted ones), and for the operations the host
    Lattice methods (bit-checked against the restatement without a GPU) and the restatement itself on every lattice."""
    khg, synth, m, am, tm, ut = setup
    e = types.SimpleNamespace(m=m, synth=synth)
    g = sg.word_loop_graph(np.random.default_rng(sg.BIG_W), m.num_tids, sg.BIG_W, sg.BIG_CHAIN)
    gl = ref.add_eps_self_loops(g, 0.25)
    U = 165
    lens = [40, 38, 42]
    feats = [_path_feats(e, g, [17 + 5 * (u % 97), 4000 + u], lens[u % 3], 100 + u) for u in range(U)]
    dg = khg.DecodingGraph(_fst(khg, gl), tm)
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    t0 = time.time()
    old = khg.decode_lattice_simple_batch(am, tm, dg, feats, cfg, 0.1)
    t_old = time.time() - t0
    rawl = khg.get_raw_lattice_simple_batch(am, tm, dg, feats, cfg, 0.1)
    res, dl = khg.get_raw_lattice_simple_device_batch(am, tm, dg, feats, cfg, 0.1)
    co = dl.chunk_off
    print("utterances %d, chunks %d at %s; states %d arcs %d; the plain decode call took %.1f s" % (
        U, dl.num_chunks, co, int(dl.state_off[-1]), int(dl.arc_off[-1]), t_old))
    assert dl.num_chunks >= 3 and len(co) == dl.num_chunks + 1 and co[0] == 0 and co[-1] == U
    assert all(b % 64 != 0 for b in co[1:-1]) and all(b > a for a, b in zip(co, co[1:])), co
    assert all(r["succeeded"] for r in res)

    def same_results(a, b, tag):
        assert len(a) == len(b), tag
        for u, (x, y) in enumerate(zip(a, b)):
            for k in OLD_KEYS:
                assert x[k] == y[k] and type(x[k]) is type(y[k]), (tag, u, k)

    same_results(res, old, "device handle / plain call")
    same_results(rawl, old, "raw call / plain call")
    L = dl.download()
    lats = [_dict(x) for x in L]
    for u in range(U):
        _same_lattice(rawl[u]["lattice"], lats[u], ("raw call", u))
    assert dl.state_off.tolist() == np.concatenate([[0], np.cumsum([x.num_states for x in L])]).tolist()
    assert dl.arc_off.tolist() == np.concatenate([[0], np.cumsum([x.num_arcs_total for x in L])]).tolist()
    # the same utterances in sub-batches of one chunk each: cut at the chunk boundaries, and at shifted ones
    shifted = [0] + [b - 20 - 5 * i for i, b in enumerate(co[1:-1])] + [U]       # (every piece shorter than the chunk it straddles: it fits)
    for cuts in (co, shifted):
        for a, b in zip(cuts, cuts[1:]):
            r1, d1 = khg.get_raw_lattice_simple_device_batch(am, tm, dg, feats[a:b], cfg, 0.1)
            assert d1.num_chunks == 1, (a, b)
            same_results(r1, res[a:b], (a, b))
            for i, x in enumerate(d1.download()):
                _same_lattice(x, lats[a + i], ("sub-batch", a, b, i))
            d1.close()
    # the operations on the handle of three chunks: the restatement on every lattice (state_off, arc_off, best path at (1, 1) = the
    # decoder's, the 11-weight sweep, prune at 0.5 and +inf with every downloaded array, prune(...).best_path = the input's)
    ev = Evidence()
    _check_ops(khg, dl, lats, ev, decoded=res, beams=[0.5, INF], pairs=[(1.0, 1.0)])
    print(ev)
    assert ev.lattices == U and ev.pruned_smaller > 0
    # ... and the host Lattice methods for every utterance
    many = dl.best_path(SWEEP_GS, SWEEP_AS)
    for k in range(len(WEIGHTS)):
        for u in range(U):
            assert _entry(many, k, u, U) == _host_entry(L[u], SWEEP_GS[k], SWEEP_AS[k]), (k, u)
    pruned = {}
    for beam in (0.5, INF):
        P = dl.prune(beam, 1.0, float(SWEEP_AS[5]))
        assert P.num_chunks == dl.num_chunks and P.chunk_off == co
        got = P.download()
        bp = P.best_path(SWEEP_GS[5: 6], SWEEP_AS[5: 6])
        for u in range(U):
            want, st = L[u].prune_with_status(beam, 1.0, float(SWEEP_AS[5]))
            assert int(P.status[u]) == st == ops.SUCCEEDED, (beam, u)
            _same_lattice(got[u], _dict(want), (beam, u))
            assert _entry(bp, 0, u, U) == _entry(many, 5, u, U), (beam, u)
        pruned[beam] = got
        P.close()
    # the restatement under the scaled pair either side of every chunk boundary, first and last
    near = sorted({0, U - 1} | {b + d for b in co[1:-1] for d in (-2, -1, 0, 1)})
    for u in near:
        for beam in (0.5, INF):
            want, st = ops.prune(lats[u], beam, 1.0, SWEEP_AS[5])
            assert st == ops.SUCCEEDED
            _same_lattice(pruned[beam][u], want, ("restatement", beam, u))
    print("restated under (1, 1/12) at utterances %s" % near)
    # from_lattices(dl.download()): one chunk, the same answers
    up = khg.DeviceLattices.from_lattices(L)
    assert up.num_chunks == 1 and up.chunk_off == [0, U]
    _same_outputs(up.best_path(SWEEP_GS, SWEEP_AS), many, "one chunk")
    for beam in (0.5, INF):
        Q = up.prune(beam, 1.0, float(SWEEP_AS[5]))
        _same_handles(Q.download(), pruned[beam], ("one chunk", beam))
        Q.close()
    up.close(); dl.close(); dg.close()
