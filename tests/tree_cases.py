"""Seeded cases for the tree tests: statistics for build-tree (with the condition that no decision of the restatement is a near tie),
and topologies / alignments / features for acc-tree-stats."""
import numpy as np

import tree_ref as ref

MIN_GAP = 1e-9


# ---------------------------------------------------------------- build-tree statistics ---------------------------------------------
def seeded_stats(N, P, phones, num_pdf_classes, dim, seed, keys_per_phone=14):
    """Statistics whose means depend on the class (odd / even) of the neighbouring phones and on the pdf-class: splits on context
    and on the pdf-class both pay.  -> plain lists (the restatement's input); numpy() turns them into build_tree's."""
    rng = np.random.default_rng(seed)
    keys = set()
    for c in phones:
        for _ in range(keys_per_phone):
            w = [int(rng.choice([0] + list(phones))) for _ in range(N)]
            w[P] = c
            keys.add(tuple(w) + (int(rng.integers(num_pdf_classes)),))
    keys = sorted(keys)
    count, x, x2 = [], [], []
    for k in keys:
        n = float(rng.integers(3, 60))
        ctx = sum((k[j] % 2) * (j + 1) for j in range(N) if j != P)
        mean = rng.normal(size=dim) * 0.3 + 0.9 * ctx + 0.5 * k[N] + 0.1 * k[P]
        var = rng.uniform(0.5, 1.5, size=dim)
        s = mean * n
        count.append(n)
        x.append([float(v) for v in s])
        x2.append([float(v) for v in (var + mean * mean) * n])
    return {"keys": [list(k) for k in keys], "count": count, "x": x, "x2": x2}


def numpy_stats(stats, N, P):
    return {"keys": np.asarray(stats["keys"], np.int32).reshape(-1, N + 1), "count": np.asarray(stats["count"], np.float64),
            "x": np.asarray(stats["x"], np.float64), "x2": np.asarray(stats["x2"], np.float64), "N": N, "P": P}


def questions_for(N, phones, num_pdf_classes):
    qs = [[p for p in phones if p % 2 == 1], [p for p in phones if p <= phones[len(phones) // 2]], [phones[0]], [0], [0, phones[-1]]]
    q = {k: [sorted(s) for s in qs] for k in range(N)}
    q[-1] = [list(range(i + 1)) for i in range(num_pdf_classes - 1)]
    return q


def reference_tree(case):
    """the restatement's tree of a case; asserts the condition on the inputs (no near tie at any decision)"""
    r = ref.build_tree(case["stats"], case["questions"], case["phone_sets"], case["p2n"], case["share_roots"], case["do_split"], case["thresh"],
                       case["max_leaves"], case["cluster_thresh"], case["N"], case["P"])
    assert r["min_gap"] > MIN_GAP, "case %s: a decision of the restatement is a near tie (gap %.3g): pick another seed" % (case["name"], r["min_gap"])
    return r


def build_cases():
    phones = [1, 2, 3, 4, 5]
    p2n = [0, 3, 3, 3, 3, 3]
    single = [[p] for p in phones]
    out = []

    def case(name, N, P, seed, phone_sets, share, split, thresh, max_leaves, cluster_thresh):
        out.append({"name": name, "N": N, "P": P, "stats": seeded_stats(N, P, phones, 3, 3, seed), "questions": questions_for(N, phones, 3),
                    "phone_sets": phone_sets, "p2n": p2n, "share_roots": share, "do_split": split, "thresh": thresh, "max_leaves": max_leaves,
                    "cluster_thresh": cluster_thresh})

    case("mono_unshared", 1, 0, 11, single, [False] * 5, [True] * 5, 5.0, 0, 0.0)
    case("bi_left_shared", 2, 1, 12, single, [True] * 5, [True] * 5, 20.0, 0, -1.0)
    case("tri_unshared", 3, 1, 13, single, [False] * 5, [True] * 5, 30.0, 0, 0.0)
    case("tri_shared_sets", 3, 1, 14, [[1], [2, 3], [4, 5]], [True, True, False], [True, True, True], 30.0, 0, -1.0)
    case("tri_nonsplit_root", 3, 1, 15, [[1], [2, 3], [4, 5]], [True, True, True], [False, True, True], 30.0, 0, -1.0)
    case("tri_max_leaves", 3, 1, 16, single, [True] * 5, [True] * 5, 0.0, 12, 0.0)
    case("tri_thresh_binds", 3, 1, 17, single, [True] * 5, [True] * 5, 150.0, 0, 0.0)
    case("tri_cluster_positive", 3, 1, 18, single, [True] * 5, [True] * 5, 20.0, 0, 60.0)
    return out


# ---------------------------------------------------------------- acc-tree-stats inputs ---------------------------------------------
def make_model(non_sil, sil, non_sil_states=3, sil_states=5):
    """(TransitionModel, topology, monophone tree) over phones `non_sil` + [sil]"""
    import kaldi_hmm_gmm_amd as khg
    topo = khg.generate_hmm_topo(list(non_sil), sil, num_non_sil_states=non_sil_states, num_sil_states=sil_states)
    tree = khg.monophone_context_dependency(topo.phones, topo.get_phone_to_num_pdf_classes())
    return khg.TransitionModel(ctx_dep=tree, hmm_topo=topo), topo, tree


def phone_alignment(tm, tree, phone, rng, max_loops=3, loops=None):
    """One pass through the phone's topology in the "reorder" convention: a forward transition-id, then self-loops of the state it
    left.  Forward arcs are drawn at random (the silence topology has several per state)."""
    from kaldi_hmm_gmm_amd.hmm_topology import kNoPdf
    entry = tm.topo.topology_for_phone(phone)
    ali, h = [], 0
    while entry[h].forward_pdf_class != kNoPdf:
        st = entry[h]
        _, fpdf = tree.compute([phone], st.forward_pdf_class)
        _, spdf = tree.compute([phone], st.self_loop_pdf_class)
        ts = tm.tuple_to_transition_state(phone, h, fpdf, spdf)
        fwd = [i for i, (dst, _) in enumerate(st.transitions) if dst != h]
        # towards the end often enough that the walk through the silence states stays short
        ends = [i for i in fwd if st.transitions[i][0] > h]
        idx = int(rng.choice(ends if (ends and rng.random() < 0.7) else fwd))
        ali.append(tm.pair_to_transition_id(ts, idx))
        sl = tm.self_loop_of(ts)
        if sl:
            ali.extend([sl] * (int(rng.integers(0, max_loops + 1)) if loops is None else loops))
        h = st.transitions[idx][0]
    return ali


def utterance(tm, tree, phones, rng, **kw):
    ali = []
    for p in phones:
        ali.extend(phone_alignment(tm, tree, p, rng, **kw))
    return np.asarray(ali, np.int32)


def features(lens, dim, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.standard_normal((T, dim)) * 1.5 + 0.7, np.float32) for T in lens]
