"""Scoring lattices on the device (khg_lattices_add_penalty, khg_lattices_oracle, khg_lattices_wer through DeviceLattices; DESIGN.md
section 7s) against the host forms (Lattice.add_penalty, Lattice.oracle, khg_edit_distance -- which tests/test_lattice_score_cpu.py holds
to the plain restatement, to a textbook Levenshtein and to the brute-force path property) on every output, with no tolerance: the
hand-made cases and the 200 seeded random lattices of tests/lattice_score_cases.py as one batch and one by one, twice, with the rows
in LDS and read back from HBM, with a scratch size that forces several launches; the sweep against best_path + khg_edit_distance at
its two consistency points and against the restatement at general triples; lattices the lattice-faster decoder leaves on the device.
A handle of more than one chunk is not covered: the only way the lattice tests have to make one is a decode with more than 4 GiB of
scratch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_score_cases as cases  # noqa: E402
import lattice_score_ref as ref  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_faster_raw import _feats, _fst, setup  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("counts", "words", "words_off", "ali", "ali_off", "status")


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


@pytest.fixture(scope="module")
def work():
    """every case with the host form's answer, computed once"""
    import kaldi_hmm_gmm_amd as khg
    items = [(name, c[0], c[1]) for name, c in sorted(cases.hand_cases().items())]
    items += [("random%d" % i, lat, r) for i, (lat, r) in enumerate(cases.random_cases())]
    out = []
    for name, lat, r in items:
        L = _lattice(khg, lat)
        out.append({"name": name, "dict": lat, "lat": L, "ref": r, "host": L.oracle(r)})
    return khg, out


def _check_oracle(r, items, tag, scratch=None):
    """DeviceLattices.oracle's dict against the host form's answers; an utterance whose table exceeds `scratch` bytes: KHG_LAT_SCRATCH"""
    wo, ao = r["words_off"], r["ali_off"]
    assert len(r["status"]) == len(items) and r["counts"].shape == (len(items), 4) and r["counts"].dtype == np.int32
    n_scratch = 0
    for u, x in enumerate(items):
        h, R = x["host"], len(x["ref"])
        words, ali = r["words"][wo[u]: wo[u + 1]].tolist(), r["ali"][ao[u]: ao[u + 1]].tolist()
        if scratch is not None and 8 * x["lat"].num_states * (R + 1) > scratch:
            assert int(r["status"][u]) == ref.SCRATCH and r["counts"][u].tolist() == [R, 0, R, 0] and words == [], (tag, x["name"])
            assert ali == [0] * len(ali)
            n_scratch += 1
            continue
        assert int(r["status"][u]) == h["status"], (tag, x["name"])
        assert r["counts"][u].tolist() == h["counts"].tolist(), (tag, x["name"])
        assert words == h["words"].tolist(), (tag, x["name"])
        assert ali == h["ali"].tolist(), (tag, x["name"])
    return n_scratch


def test_oracle_equals_the_host_form_as_one_batch_twice_in_lds_and_from_hbm(work):
    khg, items = work
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in items])
    refs = [x["ref"] for x in items]
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    outs = []
    try:
        for opt in (0, 1, 0):
            ctx.set_option("lat_ops_lds", opt)
            r = dl.oracle(refs)
            _check_oracle(r, items, "lds option %d" % opt)
            outs.append(r)
    finally:
        ctx.set_option("lat_ops_lds", default)
    for r in outs[1:]:
        for k in KEYS:
            assert r[k].tobytes() == outs[0][k].tobytes(), k
    st = outs[0]["status"].tolist()
    assert st.count(ref.SUCCEEDED) > 200 and st.count(ref.NO_PATH) >= 3 and st.count(ref.EPS_LOOP) == 2
    # the lattices are as they were, and the call works on what the other operations return
    for x, got in zip(items[:40], dl.download()[:40]):
        for k in ref.FIELDS:
            assert np.asarray(getattr(got, k)).tobytes() == np.asarray(getattr(x["lat"], k)).tobytes(), (x["name"], k)
    dl.close()
    with pytest.raises(RuntimeError, match="closed"):
        dl.oracle(refs)


def test_oracle_one_by_one(work):
    khg, items = work
    for x in items:
        dl = khg.DeviceLattices.from_lattices([x["lat"]])
        _check_oracle(dl.oracle([x["ref"]]), [x], "alone")
        dl.close()


def test_oracle_with_a_scratch_size_that_forces_several_launches(work):
    """64 KiB of tables a launch: the batch takes many launches, with the same answers; the utterances whose own table is larger --
    the frame of 200 states among them -- come back as KHG_LAT_SCRATCH"""
    khg, items = work
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in items])
    refs = [x["ref"] for x in items]
    scratch = 64 << 10
    total = sum(8 * x["lat"].num_states * (len(x["ref"]) + 1) for x in items)
    assert total > 8 * scratch
    n = _check_oracle(dl.oracle(refs, scratch), items, "64 KiB", scratch)
    names = [x["name"] for x in items if 8 * x["lat"].num_states * (len(x["ref"]) + 1) > scratch]
    assert n == len(names) >= 2 and "frame_of_200_states_w131" in names and len(names) < len(items) // 4, names
    # exactly the largest table still runs; one byte less and it does not
    big = [x for x in items if x["name"] == "frame_of_200_states_w131"]
    need = 8 * big[0]["lat"].num_states * 131
    one = khg.DeviceLattices.from_lattices([big[0]["lat"]])
    assert _check_oracle(one.oracle([big[0]["ref"]], need), big, "exact", need) == 0
    assert _check_oracle(one.oracle([big[0]["ref"]], need - 1), big, "one less", need - 1) == 1
    one.close()
    with pytest.raises(RuntimeError, match="scratch_bytes"):
        dl.oracle(refs, -1)
    with pytest.raises(RuntimeError, match="utterances"):
        dl.oracle(refs[:-1])
    with pytest.raises(RuntimeError, match="utterance 3"):
        dl.oracle(refs[:3] + [[1, 0]] + refs[4:])
    small = khg.DeviceLattices.from_lattices([items[5]["lat"]] * 3)
    r = small.oracle([items[5]["ref"]] * 3)
    wo = r["words_off"]
    assert wo[-1] == 3 * len(items[5]["host"]["words"])
    small.close()
    dl.close()


def test_add_penalty_equals_the_host_form_on_the_bits(work):
    khg, items = work
    sel = items[::2]
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in sel])
    before = dl.oracle([x["ref"] for x in sel])          # (builds the in-arc index, which goes along)
    changed = 0
    for p in (0.5, -1.25, 0.0):
        res = dl.add_penalty(p)
        assert res.num_utts == len(sel) and res.state_off.tolist() == dl.state_off.tolist() and res.arc_off.tolist() == dl.arc_off.tolist()
        for x, got in zip(sel, res.download()):
            want = x["lat"].add_penalty(p)
            for k in ref.FIELDS:
                g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
                assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (x["name"], p, k)
            assert got.start == want.start
            changed += int((np.asarray(want.graph_cost) != np.asarray(x["lat"].graph_cost)).sum())
        after = res.oracle([x["ref"] for x in sel])      # the oracle ignores the costs
        for k in KEYS:
            assert after[k].tobytes() == before[k].tobytes(), k
        res.close()
    assert changed > 1000
    for x, got in zip(sel, dl.download()):               # the input is untouched
        assert np.asarray(got.graph_cost).tobytes() == np.asarray(x["lat"].graph_cost).tobytes()
    for bad in (float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="finite"):
            dl.add_penalty(bad)
    got = khg.lattice_add_penalty(sel[3]["lat"], 0.75)
    assert np.asarray(got.graph_cost).tobytes() == np.asarray(sel[3]["lat"].add_penalty(0.75).graph_cost).tobytes()
    dl.close()


def _bp_words(bp, k, u, U):
    o = k * U + u
    ok = int(bp["status"][o]) == ref.SUCCEEDED
    return bp["words"][bp["words_off"][o]: bp["words_off"][o + 1]].tolist() if ok else []


def test_wer_at_its_consistency_points_and_against_the_restatement(work):
    khg, items = work
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    U = len(items)
    dl = khg.DeviceLattices.from_lattices([x["lat"] for x in items])
    refs = [x["ref"] for x in items]
    # penalty 0: the words scored are best_path's at the same pair
    gs, as_ = np.array([1.0, 1.0, 0.5, 2.0], F), np.array([1.0, 0.1, 1.7, 0.0], F)
    bp = dl.best_path(gs, as_)
    w0 = dl.wer(refs, gs, as_, np.zeros(4, F))
    assert w0["counts"].shape == (4 * U, 4) and w0["status"].tolist() == bp["status"].tolist()
    for k in range(4):
        for u, x in enumerate(items):
            words = _bp_words(bp, k, u, U)
            assert int(w0["nwords"][k * U + u]) == len(words), (k, x["name"])
            assert w0["counts"][k * U + u].tolist() == khg.edit_distance_counts(x["ref"], words).tolist(), (k, x["name"])
    # graph scale 1: the words scored are those of add_penalty(p) | best_path(1, as)
    pens, as1 = np.array([0.5, 1.0, -0.75, 3.0], F), np.array([1.0, 0.1, 0.0625, 1.0], F)
    w1 = dl.wer(refs, np.ones(4, F), as1, pens)
    differ = 0
    for k in range(4):
        res = dl.add_penalty(float(pens[k]))
        bpk = res.best_path(np.ones(1, F), as1[k: k + 1])
        res.close()
        assert w1["status"][k * U: (k + 1) * U].tolist() == bpk["status"].tolist(), k
        for u, x in enumerate(items):
            words = _bp_words(bpk, 0, u, U)
            assert int(w1["nwords"][k * U + u]) == len(words), (k, x["name"])
            assert w1["counts"][k * U + u].tolist() == khg.edit_distance_counts(x["ref"], words).tolist(), (k, x["name"])
            differ += words != _bp_words(bp, 0, u, U)
    print("paths the penalty changed:", differ)
    assert differ > 0           # the penalty changes paths
    # general triples, against the restatement; with the tables in LDS and in HBM
    tri = [(0.5, 1.7, 0.25), (2.0, 0.3, -0.5), (1.0, 1.0 / 12, 1.0)]
    sel = list(range(0, U, 3))
    ds = khg.DeviceLattices.from_lattices([items[u]["lat"] for u in sel])
    args = ([items[u]["ref"] for u in sel], np.array([t[0] for t in tri], F), np.array([t[1] for t in tri], F), np.array([t[2] for t in tri], F))
    default = ctx.get_option("lat_ops_lds")
    try:
        got = ds.wer(*args)
        ctx.set_option("lat_ops_lds", 1)
        hbm = ds.wer(*args)
    finally:
        ctx.set_option("lat_ops_lds", default)
    for k in ("counts", "nwords", "status"):
        assert got[k].tobytes() == hbm[k].tobytes(), k
    seen = set()
    for k, (g, a, p) in enumerate(tri):
        for j, u in enumerate(sel):
            st, nw, counts = ref.wer(items[u]["dict"], items[u]["ref"], g, a, p)
            o = k * len(sel) + j
            assert (int(got["status"][o]), int(got["nwords"][o]), got["counts"][o].tolist()) == (st, nw, counts), (k, items[u]["name"])
            seen.add(st)
    assert {ref.SUCCEEDED, ref.NO_PATH} <= seen
    ds.close()
    with pytest.raises(RuntimeError, match="point 1"):
        dl.wer(refs, np.ones(2, F), np.ones(2, F), np.array([0.0, np.inf], F))
    with pytest.raises(RuntimeError, match="same length"):
        dl.wer(refs, np.ones(2, F), np.ones(2, F), np.zeros(3, F))
    dl.close()


def _decoded(setup, W=5, U=20, lattice_beam=6.0):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    g = sg.word_loop_graph(rng, m.num_tids, W, 2)
    feats = _feats(ut, U, [int(t) for t in rng.integers(8, 20, size=U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=10.0, max_active=200, min_active=0, lattice_beam=lattice_beam)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    dg.close()
    return khg, res, dl


def test_lattices_the_lattice_faster_decoder_leaves_on_the_device(setup):  # noqa: F811
    khg, res, dl = _decoded(setup)
    U = len(res)
    rng = np.random.default_rng(3)
    refs = [cases.perturbed(rng, list(r["words"]), 5, p=0.5) if u % 2 else rng.integers(1, 6, size=int(rng.integers(0, 6))).tolist() for u, r in enumerate(res)]
    pts = [(1.0, 1.0, 0.0)] + [(1.0, 1.0 / w, p) for w in (7, 12, 17) for p in (0.0, 0.5, 1.0)]
    sweep = dl.wer(refs, np.array([t[0] for t in pts], F), np.array([t[1] for t in pts], F), np.array([t[2] for t in pts], F))
    orc = dl.oracle(refs)
    host = dl.download()
    n_ok = strictly = 0
    for u, r in enumerate(res):
        h = host[u].oracle(refs[u])
        assert int(orc["status"][u]) == h["status"] and orc["counts"][u].tolist() == h["counts"].tolist(), u
        assert orc["words"][orc["words_off"][u]: orc["words_off"][u + 1]].tolist() == h["words"].tolist(), u
        assert orc["ali"][orc["ali_off"][u]: orc["ali_off"][u + 1]].tolist() == h["ali"].tolist(), u
        if not r["succeeded"]:
            continue
        n_ok += 1
        # at (1, 1, 0) the words scored are the decoder's own
        assert int(sweep["nwords"][u]) == len(r["words"]), u
        assert sweep["counts"][u].tolist() == khg.edit_distance_counts(refs[u], list(r["words"])).tolist(), u
        # the oracle is a lower bound of every point of the sweep
        for k in range(len(pts)):
            assert orc["counts"][u][0] <= sweep["counts"][k * U + u][0], (u, k)
        strictly += orc["counts"][u][0] < sweep["counts"][u][0]
    assert n_ok >= 15 and strictly >= 1
    # pruning with an infinite beam keeps every path: the same oracle
    pruned = dl.prune(float("inf"))
    again = pruned.oracle(refs)
    for k in KEYS:
        assert again[k].tobytes() == orc[k].tobytes(), k
    out = khg.lattice_oracle_batch(dl, refs)
    assert [o["counts"].tolist() for o in out] == orc["counts"].tolist()
    table, best = khg.score_lattices(dl, refs, lmwts=(7, 12, 17), penalties=(0.0, 0.5, 1.0))
    for k, (g, a, p) in enumerate(pts[1:], 1):
        w = int(round(1.0 / a))
        assert table[(w, p)]["errors"] == int(sweep["counts"][k * U: (k + 1) * U, 0].sum()), (w, p)
    assert table[best]["errors"] == min(v["errors"] for v in table.values()) >= int(orc["counts"][:, 0].sum())
    pruned.close(); dl.close()
