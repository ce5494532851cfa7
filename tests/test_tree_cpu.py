"""Tree building on the host: khg_build_tree against the restatement of tests/tree_ref.py (equal text, objf_impr to
1e-9 relative) on seeded statistics whose decisions are no near ties, the stub round trip, gmm_init_model, convert_ali, and the argument
refusals of the C entries.  None of these needs a device."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_cases as cases  # noqa: E402
import tree_ref as ref  # noqa: E402

import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import _lib  # noqa: E402
from kaldi_hmm_gmm_amd.context_dep import ContextDependency, get_stub_map  # noqa: E402

CASES = cases.build_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_build_tree_equals_restatement(case):
    want = cases.reference_tree(case)
    N, P = case["N"], case["P"]
    tree, info = khg.build_tree(cases.numpy_stats(case["stats"], N, P), case["questions"], case["phone_sets"], case["p2n"], case["share_roots"],
                                case["do_split"], thresh=case["thresh"], max_leaves=case["max_leaves"], cluster_thresh=case["cluster_thresh"], N=N, P=P,
                                return_info=True)
    print(case["name"], "leaves", info["num_leaves"], "removed", info["num_removed"], "objf_impr", info["objf_impr"], want["objf_impr"], "min gap", want["min_gap"])
    assert tree.to_bytes(False) == want["tree"].to_bytes(False)
    assert (tree.context_width, tree.central_position) == (N, P)
    assert info["num_leaves"] == want["num_leaves"] == tree.num_pdfs and info["num_removed"] == want["num_removed"]
    assert abs(info["objf_impr"] - want["objf_impr"]) <= 1e-9 * abs(want["objf_impr"])
    assert abs(info["cluster_loss"] - want["cluster_loss"]) <= 1e-9 * max(abs(want["cluster_loss"]), 1e-300)


def test_cases_cover_what_they_claim():
    """the named cases exercise their paths: max_leaves binds, thresh binds, each clustering mode removes or keeps leaves"""
    by = {c["name"]: cases.reference_tree(c) for c in CASES}
    c = {c["name"]: c for c in CASES}
    assert by["tri_max_leaves"]["num_leaves"] == c["tri_max_leaves"]["max_leaves"]
    free = dict(c["tri_thresh_binds"], thresh=0.0, name="free")
    assert 5 < by["tri_thresh_binds"]["num_leaves"] < ref.build_tree(free["stats"], free["questions"], free["phone_sets"], free["p2n"], free["share_roots"],
                                                                      free["do_split"], 0.0, 0, 0.0, 3, 1)["num_leaves"]
    assert by["tri_cluster_positive"]["num_removed"] > 0 and by["tri_unshared"]["num_removed"] == 0
    assert by["mono_unshared"]["num_leaves"] == 15          # N = 1: the pdf-class questions cannot split a leaf of one pdf-class
    assert by["tri_nonsplit_root"]["tree"].compute([2, 1, 3], 0) == by["tri_nonsplit_root"]["tree"].compute([5, 1, 0], 2)   # phone 1's shared root stays whole


@pytest.mark.parametrize("N,P", [(1, 0), (2, 1), (3, 1)])
def test_stub_round_trip(N, P):
    """no questions and thresh = +inf: monophone_context_dependency's tree, widened to (N, P)"""
    phones, p2n = [1, 2, 3], [0, 5, 3, 3]
    st = cases.numpy_stats(cases.seeded_stats(N, P, phones, 3, 2, 5), N, P)
    tree = khg.build_tree(st, {}, [[p] for p in phones], p2n, [False] * 3, [True] * 3, thresh=float("inf"), N=N, P=P)
    mono = khg.monophone_context_dependency(phones, p2n)
    assert tree.to_bytes(False) == ContextDependency(N, P, get_stub_map(P, [[p] for p in phones], p2n, [False] * 3, [0])).to_bytes(False)
    assert tree.num_pdfs == mono.num_pdfs == 11
    if N == 1:
        assert tree.to_bytes(True) == mono.to_bytes(True)
    for ph in phones:
        for pc in range(p2n[ph]):
            w = [0] * N
            w[P] = ph
            assert tree.compute(w, pc) == mono.compute([ph], pc)


def test_statistics_outside_the_phone_sets_are_an_error():
    st = cases.numpy_stats(cases.seeded_stats(3, 1, [1, 2, 3], 3, 2, 5), 3, 1)
    with pytest.raises(khg.KhgError, match="no phone set"):
        khg.build_tree(st, {}, [[1], [2]], [0, 3, 3, 3], [True, True], [True, True], thresh=10.0)


def _arr(v):
    return np.asarray(v() if callable(v) else v, np.float64).reshape(-1)


def _tri_setup(seed=3):
    """a model over phones 1 (silence), 2 .. 5 with a split N = 3 tree built from seeded statistics"""
    tm, topo, mono = cases.make_model([2, 3, 4, 5], 1)
    p2n = topo.get_phone_to_num_pdf_classes()
    phones = [1, 2, 3, 4, 5]
    raw = cases.seeded_stats(3, 1, [2, 3, 4, 5], 3, 4, seed, keys_per_phone=30)
    # silence: context-independent keys (window 0 1 0), all five pdf-classes
    rng = np.random.default_rng(seed)
    for pc in range(5):
        raw["keys"].append([0, 1, 0, pc]); raw["count"].append(40.0)
        m = rng.normal(size=4)
        raw["x"].append([float(v) for v in m * 40]); raw["x2"].append([float(v) for v in (m * m + 1) * 40])
    order = sorted(range(len(raw["keys"])), key=lambda i: raw["keys"][i])
    raw = {k: [raw[k][i] for i in order] for k in raw}
    st = cases.numpy_stats(raw, 3, 1)
    tree, info = khg.build_tree(st, [[2, 4], [3, 5], [2], [0]], [[p] for p in phones], p2n, [True] * 5, [False] + [True] * 4, thresh=20.0, cluster_thresh=0.0,
                                return_info=True)
    return tm, topo, mono, tree, st, raw, info


def test_gmm_init_model_leaf_parameters_and_empty_leaf_rule():
    tm, topo, mono, tree, st, raw, info = _tri_setup()
    assert tree.num_pdfs > mono.num_pdfs - 4              # silence shares one root; the others split
    am, new_tm = khg.gmm_init_model(tree, st, topo)
    assert am.num_pdfs == tree.num_pdfs == new_tm.num_pdfs
    # per-leaf sums, restated with fsum
    import math
    rows = {}
    for i, k in enumerate(raw["keys"]):
        ok, pdf = tree.compute(k[:3], k[3])
        assert ok
        rows.setdefault(pdf, []).append(i)
    for pdf in range(tree.num_pdfs):
        r = rows.get(pdf, [])
        assert r, "every leaf of this tree has statistics"
        c = math.fsum(raw["count"][i] for i in r)
        mean, var = ref.gmm_init_leaf(c, [math.fsum(raw["x"][i][d] for i in r) for d in range(4)], [math.fsum(raw["x2"][i][d] for i in r) for d in range(4)])
        g = am.get_pdf(pdf)
        np.testing.assert_allclose(_arr(g.get_component_mean(0)), mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(_arr(g.get_component_variance(0)), var, rtol=1e-5)
        assert _arr(g.weights).tolist() == [1.0]
    # the empty-leaf rule: drop every row of one leaf of a split root; that leaf then takes the sum over its stub root
    victim = next(p for p in range(tree.num_pdfs) if raw["keys"][rows[p][0]][1] != 1)
    phone = raw["keys"][rows[victim][0]][1]
    keep = [i for i in range(len(raw["keys"])) if i not in set(rows[victim])]
    st2 = cases.numpy_stats({k: [raw[k][i] for i in keep] for k in raw}, 3, 1)
    am2, _ = khg.gmm_init_model(tree, st2, topo)
    root = [i for i in keep if raw["keys"][i][1] == phone]          # shared root: every pdf-class of the phone
    c = math.fsum(raw["count"][i] for i in root)
    mean, var = ref.gmm_init_leaf(c, [math.fsum(raw["x"][i][d] for i in root) for d in range(4)], [math.fsum(raw["x2"][i][d] for i in root) for d in range(4)])
    np.testing.assert_allclose(_arr(am2.get_pdf(victim).get_component_variance(0)), var, rtol=1e-5)
    np.testing.assert_allclose(_arr(am2.get_pdf(victim).get_component_mean(0)), mean, rtol=1e-5, atol=1e-6)


def test_convert_ali_identity_and_mono_to_tri():
    tm, topo, mono, tree, st, raw, info = _tri_setup()
    _, new_tm = khg.gmm_init_model(tree, st, topo)
    rng = np.random.default_rng(7)
    for phones in ([1, 2, 3, 1], [4], [1], [2, 2, 5, 3, 1, 4], [5, 1, 1, 2]):
        ali = cases.utterance(tm, mono, phones, rng)
        assert khg.convert_ali(tm, tm, mono, ali).tolist() == ali.tolist()
        tri = khg.convert_ali(tm, new_tm, tree, ali)
        assert len(tri) == len(ali)
        segs = khg.split_to_phones(tm, ali)
        assert [tm.transition_id_to_phone(s[0]) for s in segs] == phones
        t = 0
        for i, seg in enumerate(segs):
            window = [phones[i - 1] if i > 0 else 0, phones[i], phones[i + 1] if i + 1 < len(phones) else 0]
            entry = topo.topology_for_phone(phones[i])
            for old in seg:
                new = int(tri[t]); t += 1
                assert new_tm.transition_id_to_phone(new) == phones[i]
                hs = tm.transition_id_to_hmm_state(old)
                assert new_tm.transition_id_to_hmm_state(new) == hs
                assert new_tm.is_self_loop(new) == tm.is_self_loop(old) and new_tm.is_final(new) == tm.is_final(old)
                pc = entry[hs].self_loop_pdf_class if tm.is_self_loop(old) else entry[hs].forward_pdf_class
                assert (True, new_tm.transition_id_to_pdf(new)) == tree.compute(window, pc)
        assert khg.convert_ali(new_tm, new_tm, tree, tri).tolist() == tri.tolist()


def test_tid_tables_against_the_transition_model():
    tm, topo, mono = cases.make_model([2, 3], 1)
    phone, pdf_class, flags = khg.tid_tables(tm)
    for t in range(1, tm.num_transition_ids + 1):
        assert phone[t] == tm.transition_id_to_phone(t)
        assert bool(flags[t] & ref.SELF_LOOP) == tm.is_self_loop(t) and bool(flags[t] & ref.FINAL) == tm.is_final(t)
        ok, pdf = mono.compute([int(phone[t])], int(pdf_class[t]))
        assert ok and pdf == tm.transition_id_to_pdf(t)


def test_argument_refusals():
    """N = 4, phone 70 000, pdf-class 300: invalid-argument before anything else; the header, the ctypes table and the library agree"""
    lib = _lib.lib
    out = ctypes.c_void_p()
    assert lib.khg_tree_stats_create(None, 13, 3, 1, ctypes.byref(out)) == -1
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "khg_hip.h")) as fh:
        header = fh.read()
    for name in ("khg_tree_stats_create", "khg_tree_stats_destroy", "khg_tree_stats_zero", "khg_tree_stats_num_keys", "khg_tree_stats_download",
                 "khg_tree_stats_upload", "khg_tree_stats_add", "khg_acc_tree_stats", "khg_build_tree"):
        assert ("int %s(" % name) in header and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    base = cases.seeded_stats(3, 1, [1, 2, 3], 3, 2, 5)

    def build(st, N=3, P=1):
        return khg.build_tree(cases.numpy_stats(st, N, P), {}, [[1], [2], [3]], [0, 3, 3, 3], [True] * 3, [True] * 3, thresh=10.0, N=N, P=P)

    build(base)
    with pytest.raises(khg.KhgError, match="N = 4"):
        st4 = dict(base, keys=[[0] + k for k in base["keys"]])
        build(st4, N=4, P=1)
    with pytest.raises(khg.KhgError, match="70000"):
        build(dict(base, keys=base["keys"][:-1] + [[70000, 3, 0, 0]]))
    with pytest.raises(khg.KhgError, match="300"):
        build(dict(base, keys=base["keys"][:-1] + [[1, 3, 0, 300]]))
    for name in ("DeviceTreeStats", "acc_tree_stats", "acc_tree_stats_batch", "build_tree", "pdf_class_questions", "gmm_init_model", "convert_ali"):
        assert hasattr(khg, name), name
    assert hasattr(khg.UtteranceSet, "acc_tree_stats")
    assert khg.pdf_class_questions(3) == [[0], [0, 1]]
    assert (khg.TREE_MAX_CONTEXT, khg.TREE_MAX_PHONE, khg.TREE_MAX_PDF_CLASS) == (3, 65535, 255)


def test_gmm_init_model_empty_leaf_on_an_unshared_root():
    """unshared roots: the stub leaf is per (phone, pdf-class), so an empty leaf takes the sums of its own pdf-class only; the sets come
    from the tree build_tree returned, or from the caller; a tree that has lost them falls back to one shared root per phone"""
    import math
    tm, topo, mono, _, st, raw, _ = _tri_setup()
    p2n = topo.get_phone_to_num_pdf_classes()
    sets, share = [[p] for p in [1, 2, 3, 4, 5]], [False] * 5
    tree = khg.build_tree(st, [[2, 4], [3, 5], [2], [0]], sets, p2n, share, [False] + [True] * 4, thresh=20.0, cluster_thresh=0.0)
    rows = {}
    for i, k in enumerate(raw["keys"]):
        rows.setdefault(tree.compute(k[:3], k[3])[1], []).append(i)
    victim = next(p for p in range(tree.num_pdfs) if raw["keys"][rows[p][0]][1] != 1 and
                  any(q != p and raw["keys"][rows[q][0]][1::2] == raw["keys"][rows[p][0]][1::2] for q in rows))      # a leaf of a root that did split
    phone, pc = raw["keys"][rows[victim][0]][1], raw["keys"][rows[victim][0]][3]
    keep = [i for i in range(len(raw["keys"])) if i not in set(rows[victim])]
    st2 = cases.numpy_stats({k: [raw[k][i] for i in keep] for k in raw}, 3, 1)

    def want(root):
        c = math.fsum(raw["count"][i] for i in root)
        return ref.gmm_init_leaf(c, [math.fsum(raw["x"][i][d] for i in root) for d in range(4)], [math.fsum(raw["x2"][i][d] for i in root) for d in range(4)])

    own_class = [i for i in keep if raw["keys"][i][1] == phone and raw["keys"][i][3] == pc]
    whole_phone = [i for i in keep if raw["keys"][i][1] == phone]
    assert own_class and len(own_class) < len(whole_phone)
    bare = ContextDependency.from_bytes(tree.to_bytes(True), True)           # as read from a file: no stub remembered
    for t, kw, root in ((tree, {}, own_class), (bare, {"phone_sets": sets, "share_roots": share}, own_class), (bare, {}, whole_phone)):
        am, _ = khg.gmm_init_model(t, st2, topo, **kw)
        mean, var = want(root)
        np.testing.assert_allclose(_arr(am.get_pdf(victim).get_component_mean(0)), mean, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(_arr(am.get_pdf(victim).get_component_variance(0)), var, rtol=1e-5)
