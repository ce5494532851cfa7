"""lattice-determinize-pruned on the device (khg_lattices_determinize through DeviceLattices.determinize) against
the host form (Lattice.determinize, which tests/test_lattice_det_cpu.py holds to the plain restatement and to the path property), bit
for bit: states, arcs, start, statuses and stats, on the hand-made cases and the 200 seeded random lattices of
tests/lattice_det_cases.py, as batches and one by one, twice; the operations that take the result; lattices the lattice-faster decoder
leaves on the device; get_lattice_faster_device_batch.  A handle of more than one chunk is not covered: the only way the lattice tests
have to make one is a decode with more than 4 GiB of scratch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_det_cases as cases  # noqa: E402
import lattice_det_ref as ref  # noqa: E402
import lattice_lm_cases as lmc  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_ref as pr  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_faster_raw import _feats, _fst, setup  # noqa: E402,F401
from test_gpu_lattice_ops import _entry  # noqa: E402
from test_gpu_lattice_post import _gots  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STAT_SUMS = ("in_states", "in_arcs", "pruned_states", "det_states", "out_states", "out_arcs")


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


def _dict(L):
    d = {k: np.asarray(getattr(L, k)) for k in ref.FIELDS}
    d["start"] = L.start
    return d


def _same(got, want, tag):
    for k in ref.FIELDS:
        g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (tag, k)
    assert got.start == want.start, tag


@pytest.fixture(scope="module")
def work():
    """every case with the host form's answer, computed once"""
    import kaldi_hmm_gmm_amd as khg
    out = []
    for name, lat, gs, as_, beam, delta, sf, expect in cases.all_cases():
        L = _lattice(khg, lat)
        host, st, stats = L.determinize(gs, as_, beam, delta, sf)
        assert expect is None or st == expect, name
        out.append({"name": name, "lat": L, "key": (gs, as_, beam, delta, sf), "host": host, "status": st, "stats": stats})
    return khg, out


def _groups(items):
    by = {}
    for x in items:
        by.setdefault(x["key"], []).append(x)
    return [by[k] for k in sorted(by)]


def _run(khg, group):
    """one call over the utterances of `group` -> (the result handle, its lattices, statuses, stats)"""
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in group])
    res, st, stats = dl.determinize(*group[0]["key"])
    assert res.status.tolist() == st.tolist()
    lats = res.download()
    dl.close()
    return res, lats, st.tolist(), stats


def _want_stats(group):
    ok = [x for x in group if x["status"] == ref.SUCCEEDED]
    want = {k: sum(x["stats"][k] for x in group) for k in STAT_SUMS}
    want.update({k: max([x["stats"][k] for x in ok] + [0]) for k in ("max_subset", "max_closure")})
    return want


def test_device_equals_the_host_form_batched_and_twice(work):
    khg, items = work
    seen = {}
    n_utt = 0
    for group in _groups(items):
        res, lats, st, stats = _run(khg, group)
        assert st == [x["status"] for x in group], [x["name"] for x in group]
        for x, got in zip(group, lats):
            _same(got, x["host"], x["name"])
            seen[x["status"]] = seen.get(x["status"], 0) + 1
        assert stats == _want_stats(group), group[0]["name"]
        assert res.state_off.tolist() == np.concatenate([[0], np.cumsum([x["host"].num_states for x in group])]).tolist()
        res.close()
        res2, lats2, st2, stats2 = _run(khg, group)       # the same bits over two runs
        assert st2 == st and stats2 == stats
        for a, b in zip(lats, lats2):
            _same(a, b, "second run")
        res2.close()
        n_utt += len(group)
    assert n_utt == len(items)
    assert seen[ref.SUCCEEDED] > 100 and seen[ref.SCRATCH] >= 1 and seen[ref.EPS_LOOP] == 2 and seen[ref.NO_PATH] >= 2, seen


def test_device_one_utterance_at_a_time_twice(work):
    """independent of the batch: every hand case and every fourth random one alone"""
    khg, items = work
    alone = [x for x in items if not x["name"].startswith("random")] + [x for x in items if x["name"].startswith("random")][::4]
    for x in alone:
        for rep in range(2):
            res, lats, st, stats = _run(khg, [x])
            assert st == [x["status"]] and stats == x["stats"], (x["name"], rep, stats, x["stats"])
            _same(lats[0], x["host"], (x["name"], "alone", rep))
            res.close()
    assert len(alone) > 70


def test_refusals(work):
    khg, items = work
    dl = khg.DeviceLattices.from_lattices([items[0]["lat"]])
    for kw, msg in (({"beam": -1.0}, "beam must be finite"), ({"beam": float("inf")}, "beam must be finite"), ({"delta": float("nan")}, "delta must be finite"),
                    ({"delta": -1.0}, "delta must be finite"), ({"state_factor": 0}, "state_factor must be >= 1"), ({"graph_scale": -1.0}, "finite and >= 0")):
        with pytest.raises(khg.KhgError, match=msg):
            dl.determinize(**kw)
    empty = khg.DeviceLattices.from_lattices([])
    r, st, stats = empty.determinize()
    assert r.num_utts == 0 and len(st) == 0 and stats["out_states"] == 0
    r.close(); empty.close(); dl.close()


def test_the_operations_take_the_result(work):
    """best_path, posteriors, lm_rescore, oracle and mbr on the result handle against the host forms on the downloaded result"""
    khg, items = work
    group = max(_groups(items), key=len)
    res, lats, st, _ = _run(khg, group)
    U = len(group)
    pairs = cases.SCALES
    bp = res.best_path(np.array([p[0] for p in pairs], F), np.array([p[1] for p in pairs], F))
    P = res.posteriors(1.0, 0.1)
    gots = _gots(P)
    lm = khg.NgramLm(**lmc.unigram(80))
    dlm = khg.DeviceLm(lm)
    lmres, lmst, _ = res.lm_rescore(dlm, 1.0)
    lml = lmres.download()
    rng = np.random.default_rng(9)
    refs = [rng.integers(1, 6, size=int(rng.integers(0, 5))).astype(np.int32) for _ in range(U)]
    orc = res.oracle(refs, 0)
    mbr = khg.mbr_utterances(res.mbr(1.0, 1.0, True, 32, None, 0, 0))
    worst, n_ok = 0.0, 0
    for u, (x, L) in enumerate(zip(group, lats)):
        t = x["name"]
        for k, (g, a) in enumerate(pairs):
            hb = L.best_path(g, a)
            got = _entry(bp, k, u, U)
            assert got[0] == hb["status"], (t, g, a)
            if hb["status"] == ref.SUCCEEDED:
                assert (got[1], got[2], got[3]) == (list(hb["ali"]), list(hb["words"]), ops.bits(hb["weight"])), (t, g, a)
        worst = max(worst, pr.compare(gots[u], pr.forward_backward(_dict(L), 1.0, 0.1), _dict(L), t))
        assert L.forward_backward(1.0, 0.1)["status"] == gots[u]["status"], t
        H, hst, _ = L.lm_rescore(lm, 1.0)
        assert int(lmst[u]) == hst, t
        _same(lml[u], H, (t, "lm_rescore"))
        ho = L.oracle(refs[u])
        wo, ao = orc["words_off"], orc["ali_off"]
        assert int(orc["status"][u]) == ho["status"] and orc["counts"][u].tolist() == ho["counts"].tolist(), t
        assert orc["words"][wo[u]: wo[u + 1]].tolist() == ho["words"].tolist() and orc["ali"][ao[u]: ao[u + 1]].tolist() == ho["ali"].tolist(), t
        hm = L.mbr(1.0, 1.0, True, 32, None, 0, arc_cond=mbr[u]["arc_cond"], final_cond=mbr[u]["final_cond"])
        assert mbr[u]["status"] == hm["status"] and mbr[u]["iters"] == hm["iters"] and mbr[u]["bayes_risk"] == hm["bayes_risk"], t
        assert mbr[u]["words"].tolist() == hm["words"].tolist() and mbr[u]["conf"].tobytes() == hm["conf"].tobytes(), t
        n_ok += st[u] == ref.SUCCEEDED
    assert n_ok >= 15 and worst <= 1.0
    for h in (P, lmres, dlm, res):
        h.close()


def _decoded(setup, W=5, U=20, lattice_beam=6.0, determinize=False):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    g = sg.word_loop_graph(rng, m.num_tids, W, 2)
    feats = _feats(ut, U, [int(t) for t in rng.integers(8, 20, size=U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=10.0, max_active=200, min_active=0, lattice_beam=lattice_beam, determinize_lattice=determinize)
    return khg, am, tm, dg, feats, cfg


def test_decoded_lattices_and_get_lattice(setup):  # noqa: F811
    """lattices the lattice-faster decoder leaves on the device: the device equals the host form; every word sequence of the result has
    one path (the best path's words are those of the pruned input); get_lattice_faster_device_batch equals raw plus determinize"""
    khg, am, tm, dg, feats, cfg = _decoded(setup)
    dres, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    out, st, stats = dl.determinize(1.0, 1.0, cfg.lattice_beam, cfg.det_opts.delta)
    host, got = dl.download(), out.download()
    n = shrank = 0
    for u, (L, G) in enumerate(zip(host, got)):
        H, hst, _ = L.determinize(1.0, 1.0, cfg.lattice_beam, cfg.det_opts.delta)
        assert int(st[u]) == hst, u
        _same(G, H, u)
        if hst != ref.SUCCEEDED:
            continue
        n += 1
        shrank += G.num_states < L.num_states
        a, b = G.best_path(1.0, 1.0), L.best_path(1.0, 1.0)
        assert a["words"] == b["words"] and a["weight"] == b["weight"], u
    assert n >= 15 and shrank >= 1 and stats["det_states"] >= n and stats["out_states"] == sum(G.num_states for G in got)
    # GetLattice: the configuration's determinize_lattice, lattice_beam and det_opts.delta
    cfg.determinize_lattice = True
    res2, dl2 = khg.get_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    assert [r["status"] for r in res2] == [r["status"] for r in dres]
    for u, (a, b) in enumerate(zip(dl2.download(), got)):
        _same(a, b, (u, "get_lattice"))
    cfg.determinize_lattice = False
    res3, dl3 = khg.get_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    for u, (a, b) in enumerate(zip(dl3.download(), host)):
        _same(a, b, (u, "get_lattice without determinization"))
    lats = khg.lattice_determinize_pruned_batch(host[:3], 1.0, 1.0, cfg.lattice_beam)
    for u in range(3):
        _same(lats[u], got[u], (u, "lattice_determinize_pruned_batch"))
    for h in (dl, out, dl2, dl3, dg):
        h.close()
