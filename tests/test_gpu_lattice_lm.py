"""lattice-lmrescore on the device (khg_lattices_lm_rescore through DeviceLattices.lm_rescore) against the host
form (Lattice.lm_rescore, which tests/test_lattice_lm_cpu.py holds to the plain restatement and to the path property), bit for bit:
states, arcs, start, statuses and stats, on the hand-made cases and the 200 seeded random lattices of tests/lattice_lm_cases.py, as
one batch and one by one, twice; the operations that take the result; a unigram taken out and put back; lattices the lattice-faster
decoder leaves on the device.  A handle of more than one chunk is not covered: the only way the lattice tests have to make one is a
decode with more than 4 GiB of scratch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_lm_cases as cases  # noqa: E402
import lattice_lm_ref as ref  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_ref as pr  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_faster_raw import _feats, _fst, setup  # noqa: E402,F401
from test_gpu_lattice_ops import _entry, _want_entry  # noqa: E402
from test_gpu_lattice_post import _gots  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
PAIRS = [(1.0, 1.0), (1.0, 0.1), (0.5, 1.7)]


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
    """the cases grouped by (LM, scale, hist_factor) -- one call takes one LM -- with the host form's answer for each, computed once"""
    import kaldi_hmm_gmm_amd as khg
    items = [(name,) + c[:4] for name, c in sorted(cases.hand_cases().items())]
    items += [("random%d" % i,) + c for i, c in enumerate(cases.random_cases())]
    out = []
    for name, lat, lm, scale, hf in items:
        L, nlm = _lattice(khg, lat), khg.NgramLm(**lm)
        host, st, stats = L.lm_rescore(nlm, scale, hf)
        out.append({"name": name, "lat": L, "lm": nlm, "scale": scale, "hf": hf, "host": host, "status": st, "stats": stats})
    return khg, out


def _run(khg, group, lm, scale, hf):
    """one call over the utterances of `group` -> (the result handle, its lattices, statuses, stats)"""
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in group])
    dlm = khg.DeviceLm(lm)
    res, st, stats = dl.lm_rescore(dlm, scale, hf)
    assert res.status.tolist() == st.tolist()
    lats = res.download()
    dl.close(); dlm.close()
    return res, lats, st.tolist(), stats


def _groups(items):
    """one call takes one LM, one scale and one hist_factor: the hand cases that share all three make a batch, every random case (an LM
    of its own) is a batch of one"""
    by = {}
    for x in items:
        lm = x["lm"]
        key = (x["scale"], x["hf"], lm.start) + tuple(getattr(lm, k).tobytes() for k in ("backoff", "backoff_cost", "arc_begin", "word", "cost", "next", "final_cost"))
        by.setdefault(key, []).append(x)
    return list(by.values())


def test_device_equals_the_host_form_batched_one_by_one_and_twice(work):
    khg, items = work
    n_utt = n_batched = 0
    seen = {}
    for group in _groups(items):
        lm, scale, hf = group[0]["lm"], group[0]["scale"], group[0]["hf"]
        res, lats, st, stats = _run(khg, group, lm, scale, hf)
        assert st == [x["status"] for x in group], [x["name"] for x in group]
        for x, got in zip(group, lats):
            _same(got, x["host"], x["name"])
            seen[x["status"]] = seen.get(x["status"], 0) + 1
        ok = [x for x in group if x["status"] == ref.SUCCEEDED]
        assert stats == {"in_states": sum(x["stats"]["in_states"] for x in group), "in_arcs": sum(x["stats"]["in_arcs"] for x in group),
                         "out_states": sum(x["stats"]["out_states"] for x in group), "out_arcs": sum(x["stats"]["out_arcs"] for x in group),
                         "max_hist": max([x["stats"]["max_hist"] for x in ok] + [0])}, group[0]["name"]
        res.close()
        # the same bits over two runs
        res2, lats2, st2, stats2 = _run(khg, group, lm, scale, hf)
        assert st2 == st and stats2 == stats
        for a, b in zip(lats, lats2):
            _same(a, b, "second run")
        res2.close()
        if len(group) > 1:      # ... and independent of the batch
            n_batched += len(group)
            for x, got in zip(group, lats):
                r1, l1, s1, t1 = _run(khg, [x], lm, scale, hf)
                assert s1 == [x["status"]] and t1 == x["stats"], x["name"]
                _same(l1[0], got, (x["name"], "alone"))
                r1.close()
        n_utt += len(group)
    assert n_utt == len(items) and n_batched >= 10
    assert seen[ref.SUCCEEDED] > 150 and seen[ref.SCRATCH] > 5 and seen[ref.LM_OOV] == 1 and seen[ref.EPS_LOOP] == 2 and seen[ref.NO_PATH] == 1


def test_one_batch_with_an_empty_utterance_between_two_good_ones_and_every_failure(work):
    khg, items = work
    by = {x["name"]: x for x in items}
    names = ["diamond_bigram", "empty", "chain3", "oov_reachable", "arc_to_lower_state", "unreachable", "oov_unreachable", "self_loop", "one_state"]
    group = [by[n] for n in names]
    lm = group[0]["lm"]
    assert all(x["lm"].cost.tobytes() == lm.cost.tobytes() for x in group)
    res, lats, st, stats = _run(khg, group, lm, 1.0, 8)
    assert st == [ref.SUCCEEDED, ref.NO_PATH, ref.SUCCEEDED, ref.LM_OOV, ref.EPS_LOOP, ref.SUCCEEDED, ref.SUCCEEDED, ref.EPS_LOOP, ref.SUCCEEDED]
    for x, got in zip(group, lats):
        _same(got, x["host"], x["name"])
    assert res.state_off.tolist() == np.concatenate([[0], np.cumsum([x["host"].num_states for x in group])]).tolist()
    # hist_factor 1: the diamond runs out, the chain does not
    res1, lats1, st1, _ = _run(khg, [by["diamond_bigram"], by["chain3"]], lm, 1.0, 1)
    assert st1 == [ref.SCRATCH, ref.SUCCEEDED] and lats1[0].num_states == 0
    _same(lats1[1], by["chain3"]["host"], "chain3 at hist_factor 1")
    res.close(); res1.close()


def test_refusals(work):
    khg, items = work
    x = items[0]
    dl = khg.DeviceLattices.from_lattices([x["lat"]])
    dlm = khg.DeviceLm(x["lm"])
    assert dlm.num_states == x["lm"].num_states and dlm.device_bytes >= 4 * (4 * x["lm"].num_states + 1 + 3 * x["lm"].num_arcs)
    for scale, hf, msg in ((float("nan"), 8, "scale must be finite"), (float("inf"), 8, "scale must be finite"), (1.0, 0, "hist_factor must be >= 1")):
        with pytest.raises(khg.KhgError, match=msg):
            dl.lm_rescore(dlm, scale, hf)
    other = khg.Context(0)
    olm = khg.DeviceLm(x["lm"], other)
    with pytest.raises(khg.KhgError, match="a handle of another context"):
        dl.lm_rescore(olm, 1.0, 8)
    olm.close()
    empty = khg.DeviceLattices.from_lattices([])
    r, st, stats = empty.lm_rescore(dlm)
    assert r.num_utts == 0 and len(st) == 0 and stats["out_states"] == 0
    r.close(); empty.close(); dl.close(); dlm.close()


def test_best_path_and_posteriors_take_the_result(work):
    khg, items = work
    ok = [x for x in items if x["status"] == ref.SUCCEEDED][:60]
    worst = 0.0
    n = 0
    gs = np.array([p[0] for p in PAIRS], np.float32)
    as_ = np.array([p[1] for p in PAIRS], np.float32)
    for x in ok:
        res, lats, st, _ = _run(khg, [x], x["lm"], x["scale"], x["hf"])
        want = _dict(x["host"])
        bp = res.best_path(gs, as_)
        for k, (g, a) in enumerate(PAIRS):
            assert _entry(bp, k, 0, 1) == _want_entry(want, g, a), (x["name"], g, a)
            hb = x["host"].best_path(g, a)
            assert (hb["status"], ops.bits(hb["weight"])) == (_entry(bp, k, 0, 1)[0], _entry(bp, k, 0, 1)[3]), (x["name"], g, a)
        P = res.posteriors(1.0, 0.1)
        w = pr.forward_backward(want, 1.0, 0.1)
        worst = max(worst, pr.compare(_gots(P)[0], w, want, x["name"]))
        hf = x["host"].forward_backward(1.0, 0.1)
        assert hf["status"] == int(P.status[0])
        n += w["status"] == pr.SUCCEEDED
        P.close(); res.close()
    assert n > 30 and worst <= 1.0
    print("posteriors of %d rescored lattices: worst error / bound %.3g" % (n, worst))


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def _decoded(setup, W=5, U=20):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    g = sg.word_loop_graph(rng, m.num_tids, W, 2)
    feats = _feats(ut, U, [int(t) for t in rng.integers(8, 20, size=U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=10.0, max_active=200, min_active=0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    dg.close()
    return khg, res, dl


def test_a_unigram_taken_out_and_put_back(setup):
    """scale -1 then +1 with a one-state LM: the structure is the input's, a graph cost has been rounded twice -- fl(fl(g - c) + c) is
    within one ulp of each rounding's result, 2 ulps of g's neighbourhood in all, measured at the larger of the two magnitudes"""
    khg, res, dl = _decoded(setup)
    lm = khg.NgramLm.unigram({w: p for w, p in zip(range(1, 6), [0.4, 0.3, 0.15, 0.1, 0.05])})
    dlm = khg.DeviceLm(lm)
    out, st1, stats1 = dl.lm_rescore(dlm, -1.0)
    back, st2, stats2 = out.lm_rescore(dlm, 1.0)
    assert stats1["max_hist"] == 1 and stats2["max_hist"] == 1 and stats1["in_states"] >= stats1["out_states"] == stats2["out_states"]
    a, mid, b = dl.download(), out.download(), back.download()
    n = 0
    for u, (x, y, z) in enumerate(zip(a, mid, b)):
        assert (int(st1[u]) == ref.SUCCEEDED) == (x.num_states > 0) and st1[u] == st2[u]
        if x.num_states == 0:
            continue
        # unreachable states go (the decoder leaves none); everything else keeps its place
        for k in ref.FIELDS:
            if k not in ("graph_cost", "final_cost"):
                assert np.asarray(getattr(y, k)).tobytes() == np.asarray(getattr(x, k)).tobytes(), (u, k)
                assert np.asarray(getattr(z, k)).tobytes() == np.asarray(getattr(x, k)).tobytes(), (u, k)
        gx, gy, gz = (np.asarray(v.graph_cost) for v in (x, y, z))
        worded = np.asarray(x.olabel) != 0
        assert gz[~worded].tobytes() == gx[~worded].tobytes() and (gy[worded] != gx[worded]).any()
        # 2 ulps at the larger magnitude the value passed through
        big = np.maximum(np.abs(gx), np.abs(gy)).astype(np.float32)
        assert (np.abs(gz.astype(np.float64) - gx.astype(np.float64)) <= 2.0 * np.spacing(big).astype(np.float64)).all(), u
        assert np.asarray(z.final_cost).tobytes() == np.asarray(x.final_cost).tobytes()
        n += int(worded.sum())
    assert n > 50
    for h in (out, back, dl, dlm):
        h.close()


def test_decoded_lattices_rescored_with_an_estimated_bigram(setup):
    khg, res, dl = _decoded(setup)
    rng = np.random.default_rng(5)
    lm = khg.estimate_ngram_lm([rng.integers(1, 6, size=int(rng.integers(1, 6))).tolist() for _ in range(40)], 2, range(1, 6))
    dlm = khg.DeviceLm(lm)
    out, st, stats = dl.lm_rescore(dlm, 1.0)
    host = dl.download()
    got = out.download()
    n = grew = 0
    for u, (L, G) in enumerate(zip(host, got)):
        H, hst, hstats = L.lm_rescore(lm, 1.0)
        assert int(st[u]) == hst, u
        _same(G, H, u)
        n += hst == ref.SUCCEEDED
        grew += H.num_states > L.num_states
    assert n >= 15 and grew >= 1 and stats["max_hist"] >= 2 and stats["out_states"] > stats["in_states"]
    assert khg.lattice_lmrescore(lm, host[0]).num_states == got[0].num_states
    for h in (out, dl, dlm):
        h.close()
