"""Minimum Bayes risk decoding on the device (khg_lattices_mbr through DeviceLattices.mbr).  The rule takes an
arg-min at every (arc, position) and an arg-max at every position, and one ulp in a weight can move a tie, so nothing downstream of the
weights is compared under a tolerance: the device hands back the weights it used (arc_cond, final_cond), these are held to the
restatement's within the bound of section 7g, and every other output must EQUAL the host form's (Lattice.mbr, which
tests/test_lattice_mbr_cpu.py holds to the restatement) given the device's weights -- as one batch, one utterance at a time, three times
over, and with a scratch size that forces many launches.  A handle of more than one chunk is not covered: the only way the lattice tests
have to make one is a decode with more than 4 GiB of scratch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_mbr_cases as cases  # noqa: E402
import lattice_mbr_ref as ref  # noqa: E402
import lattice_post_ref as post  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from lattice_score_ref import FIELDS  # noqa: E402
from test_gpu_lattice_faster_raw import _feats, _fst, setup  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("status", "iters", "bayes_risk", "words", "words_off", "conf", "vocab", "vocab_off", "gamma", "gamma_off", "arc_cond", "final_cond")


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in FIELDS], int(lat["start"]))


def _groups(items):
    """the cases that share (decode_mbr, max_iter, max_words): one device call each"""
    g = {}
    for x in items:
        g.setdefault((x["decode_mbr"], x["max_iter"], x["max_words"]), []).append(x)
    return g


@pytest.fixture(scope="module")
def work():
    """every hand case, and every third seeded lattice from the best path and from its unrelated reference, as host Lattices"""
    import kaldi_hmm_gmm_amd as khg
    items = cases.hand_cases() + cases.seeded_cases()[::3]
    for x in items:
        x["L"] = _lattice(khg, x["lat"])
    return khg, items


def _check(khg, r, items, gs, as_, tag, scratch=None):
    """DeviceLattices.mbr's dict for `items` (one call: the same decode_mbr, max_iter, max_words) against the host form given the
    device's weights; -> the number of utterances refused for scratch"""
    per = khg.mbr_utterances(r)
    assert len(per) == len(items)
    n_scratch = 0
    for x, got in zip(items, per):
        t = (tag, x["name"], gs, as_)
        want = x["L"].mbr(gs, as_, x["decode_mbr"], x["max_iter"], x["init"], x["max_words"], arc_cond=got["arc_cond"], final_cond=got["final_cond"])
        if scratch is not None and want["status"] & ref.SUCCEEDED and ref.table_bytes(x["lat"], want["cap"]) > scratch:
            assert got["status"] == ref.SCRATCH and got["bayes_risk"] == np.inf and len(got["words"]) == 0 and got["gamma"].size == 0, t
            n_scratch += 1
            continue
        assert got["status"] == want["status"] and got["iters"] == want["iters"], (t, got["status"], want["status"], got["iters"], want["iters"])
        assert got["bayes_risk"] == want["bayes_risk"], (t, got["bayes_risk"], want["bayes_risk"])
        assert got["words"].dtype == np.int32 and got["words"].tolist() == want["words"].tolist(), t
        assert got["conf"].tobytes() == want["conf"].tobytes(), t
        assert got["vocab"].tolist() == want["vocab"].tolist(), t
        assert got["gamma"].shape == want["gamma"].shape and got["gamma"].tobytes() == want["gamma"].tobytes(), t
        if x["expect"] is not None and scratch is None:
            assert got["status"] == x["expect"], t
    return n_scratch


def _run(khg, items, gs, as_, tag, scratch=0):
    outs = []
    n = 0
    for (decode, max_iter, max_words), xs in sorted(_groups(items).items()):
        dl = khg.DeviceLattices.from_lattices([x["L"] for x in xs])
        inits = None if all(x["init"] is None for x in xs) else [x["init"] for x in xs]
        r = dl.mbr(gs, as_, decode, max_iter, inits, max_words, scratch)
        dl.close()
        n += _check(khg, r, xs, gs, as_, tag, scratch or None)
        outs.append(r)
    return outs, n


def test_device_weights_agree_with_the_restatements(work):
    """arc_cond / final_cond within the bound section 7g derived for an arc posterior; zeros and statuses equal"""
    khg, items = work
    dl = khg.DeviceLattices.from_lattices([x["L"] for x in items])
    worst = 0.0
    for gs, as_ in cases.PAIRS:
        per = khg.mbr_utterances(dl.mbr(gs, as_, False, 0, None, 0, 0))
        for x, got in zip(items, per):
            st, ac, fc, fb = ref.weights(x["lat"], gs, as_)
            assert got["status"] == st, (x["name"], got["status"], st)
            for g, w in ((got["arc_cond"], np.asarray(ac)), (got["final_cond"], np.asarray(fc))):
                assert g.shape == w.shape and ((g == 0.0) == (w == 0.0)).all() and not np.signbit(g).any(), x["name"]
                if st == ref.SUCCEEDED and len(w):
                    tol = post.tolerances(fb, x["lat"])[1]
                    assert np.abs(g - w).max() <= tol, (x["name"], gs, as_, np.abs(g - w).max(), tol)
                    worst = max(worst, float(np.abs(g - w).max()) / tol)
    dl.close()
    print("worst device weight error / bound: %.3g" % worst)


def test_device_equals_the_host_form_given_its_weights_as_batches_three_times(work):
    khg, items = work
    for gs, as_ in cases.PAIRS:
        first, _ = _run(khg, items, gs, as_, "batch")
        if (gs, as_) != cases.PAIRS[0]:
            continue
        for rep in (1, 2):
            again, _ = _run(khg, items, gs, as_, "batch again %d" % rep)
            for a, b in zip(first, again):
                for k in KEYS:
                    assert a[k].tobytes() == b[k].tobytes(), (rep, k)


def test_device_one_utterance_at_a_time(work):
    khg, items = work
    gs, as_ = cases.PAIRS[0]
    for x in items:
        dl = khg.DeviceLattices.from_lattices([x["L"]])
        r = dl.mbr(gs, as_, x["decode_mbr"], x["max_iter"], None if x["init"] is None else [x["init"]], x["max_words"], 0)
        dl.close()
        _check(khg, r, [x], gs, as_, "alone")


def test_device_with_a_scratch_size_that_forces_many_launches(work):
    """64 KiB of tables a launch: the same answers from many launches; an utterance whose own table is larger comes back as
    KHG_LAT_SCRATCH; exactly its size runs, one byte less does not"""
    khg, items = work
    gs, as_ = cases.PAIRS[0]
    scratch = 64 << 10
    total = sum(ref.table_bytes(x["lat"], max(1, len(x["init"] or []))) for x in items)
    assert total > 8 * scratch
    _, n = _run(khg, items, gs, as_, "64 KiB", scratch)
    assert 2 <= n < len(items) // 4, n
    x = [y for y in items if y["name"] == "segment_edge_w63"][0]
    host = x["L"].mbr(gs, as_, True, 32, x["init"])
    need = ref.table_bytes(x["lat"], host["cap"])
    assert need > scratch
    dl = khg.DeviceLattices.from_lattices([x["L"]])
    assert _check(khg, dl.mbr(gs, as_, True, 32, [x["init"]], 0, need), [x], gs, as_, "exact", need) == 0
    assert _check(khg, dl.mbr(gs, as_, True, 32, [x["init"]], 0, need - 1), [x], gs, as_, "one less", need - 1) == 1
    # the refusals that need a handle
    with pytest.raises(RuntimeError, match="utterances"):
        dl.mbr(gs, as_, True, 32, [x["init"], [1]], 0, 0)
    with pytest.raises(RuntimeError, match="utterance 0"):
        dl.mbr(gs, as_, True, 32, [[1, 0]], 0, 0)
    with pytest.raises(RuntimeError, match="scratch_bytes"):
        dl.mbr(gs, as_, True, 32, None, 0, -1)
    with pytest.raises(RuntimeError, match="max_iter"):
        dl.mbr(gs, as_, True, -1, None, 0, 0)
    with pytest.raises(RuntimeError, match="finite"):
        dl.mbr(float("nan"), as_, True, 32, None, 0, 0)
    # a per-utterance None takes the best path's words for that utterance alone
    two = khg.DeviceLattices.from_lattices([x["L"], x["L"]])
    per = khg.mbr_utterances(two.mbr(gs, as_, False, 0, [None, x["init"]], 0, 0))
    assert per[0]["words"].tolist() == x["L"].best_path(gs, as_)["words"] and per[1]["words"].tolist() == x["init"]
    two.close()
    dl.close()
    out = khg.lattice_mbr_decode(x["L"], gs, as_, init=x["init"])
    assert out["status"] & ref.SUCCEEDED and len(out["sausage"]) == 2 * len(out["words"]) + 1
    for q, bins in enumerate(out["sausage"]):
        assert bins and all(p > 0 for _, p in bins) and bins == sorted(bins, key=lambda b: (-b[1], b[0])), q


def test_single_path_lattices_equal_the_restatement_with_its_own_weights(work):
    """every weight of a single-path lattice is exactly 1.0 on every side, so here the device equals the restatement outright"""
    khg, items = work
    sel = [x for x in items if x["name"].startswith(("single_path", "chain3"))]
    assert len(sel) >= 9
    for gs, as_ in cases.PAIRS:
        for x in sel:
            dl = khg.DeviceLattices.from_lattices([x["L"]])
            got = khg.mbr_utterances(dl.mbr(gs, as_, x["decode_mbr"], x["max_iter"], [x["init"]], x["max_words"], 0))[0]
            dl.close()
            want = ref.mbr(x["lat"], gs, as_, x["decode_mbr"], x["max_iter"], x["init"], x["max_words"])
            assert got["status"] == want["status"] and got["iters"] == want["iters"] and got["bayes_risk"] == want["bayes_risk"], x["name"]
            assert got["words"].tolist() == want["words"] and got["conf"].tolist() == want["conf"] and got["vocab"].tolist() == want["vocab"], x["name"]
            assert got["gamma"].tolist() == [list(g) for g in want["gamma"]], x["name"]
            if want["status"] & ref.SUCCEEDED:
                assert (got["arc_cond"] == 1.0).all() and got["final_cond"][-1] == 1.0, x["name"]


def test_lattices_the_lattice_faster_decoder_leaves_on_the_device(setup):  # noqa: F811
    """20 decoded utterances at (1, 1) with decode_mbr=False: the words are best_path's, every confidence lies in [0, 1 + tol] (tol:
    mass conservation's (states + arcs) * (Q + 1) * 2^-52), and the device equals the host form given its weights"""
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    U = 20
    g = sg.word_loop_graph(rng, m.num_tids, 5, 2)
    feats = _feats(ut, U, [int(t) for t in rng.integers(8, 20, size=U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=10.0, max_active=200, min_active=0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    dg.close()
    bp = dl.best_path(np.ones(1, F), np.ones(1, F))
    per = khg.mbr_utterances(dl.mbr(1.0, 1.0, False, 32, None, 0, 0))
    dec = khg.mbr_utterances(dl.mbr(1.0, 1.0, True, 32, None, 0, 0))
    host = dl.download()
    n_ok = 0
    for u in range(U):
        ok = int(bp["status"][u]) == ref.SUCCEEDED
        words = bp["words"][bp["words_off"][u]: bp["words_off"][u + 1]].tolist() if ok else []
        for got, decode in ((per[u], False), (dec[u], True)):
            want = host[u].mbr(1.0, 1.0, decode, 32, None, 0, arc_cond=got["arc_cond"], final_cond=got["final_cond"])
            assert got["status"] == want["status"] and got["iters"] == want["iters"] and got["bayes_risk"] == want["bayes_risk"], (u, decode)
            assert got["words"].tolist() == want["words"].tolist() and got["conf"].tobytes() == want["conf"].tobytes(), (u, decode)
            assert got["gamma"].tobytes() == want["gamma"].tobytes(), (u, decode)
        if not per[u]["status"] & ref.SUCCEEDED:
            continue
        n_ok += 1
        assert per[u]["iters"] == 0 and per[u]["words"].tolist() == words, u
        tol = (host[u].num_states + host[u].num_arcs_total) * (2 * len(words) + 2) * 2.0 ** -52
        assert ((per[u]["conf"] >= 0.0) & (per[u]["conf"] <= 1.0 + tol)).all(), (u, per[u]["conf"])
        assert np.abs(per[u]["gamma"].sum(axis=1) - 1.0).max() <= tol, u
    assert n_ok >= 15
    dl.close()
