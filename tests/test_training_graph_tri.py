"""Context-dependent training and decoding graphs: TrainingGraphCompiler on trees of context width 3.

All accepting paths of at most a bounded number of arcs are enumerated (self-loops included).  For a tree that ignores context the
set of (transition-id sequence, cost) equals the monophone compiler's; for a split tree the paths are the monophone graph's paths
(same phones, HMM states, arc choices, words and costs) and every transition-id carries the pdf tree.compute gives for the window
its path implies, 0 at both ends -- on both lexicon forms, with and without optional silence, and across the word loop."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_cases as cases  # noqa: E402

import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd.context_dep import ContextDependency, get_stub_map  # noqa: E402

SIL = 1
PHONES = [2, 3, 4]
LEXICON = {1: [(1.0, [2, 3])], 2: [(0.6, [3]), (0.4, [4, 2])], 3: [(1.0, [4, 4, 3])]}
TRANSCRIPTS = [[], [2], [1, 2], [3, 1, 2]]


@pytest.fixture(scope="module")
def setup():
    topo = khg.generate_hmm_topo(PHONES, SIL, num_non_sil_states=2, num_sil_states=3)
    p2n = topo.get_phone_to_num_pdf_classes()
    mono = khg.monophone_context_dependency(topo.phones, p2n)
    sets = [[p] for p in topo.phones]
    flat = ContextDependency(3, 1, get_stub_map(1, sets, p2n, [False] * len(sets), [0]))         # the stub, widened: ignores context
    raw = cases.seeded_stats(3, 1, PHONES, 2, 3, 8, keys_per_phone=40)
    rng = np.random.default_rng(8)
    for pc in range(3):
        m = rng.normal(size=3)
        raw["keys"].append([0, SIL, 0, pc]); raw["count"].append(30.0)
        raw["x"].append([float(v) for v in m * 30]); raw["x2"].append([float(v) for v in (m * m + 1) * 30])
    order = sorted(range(len(raw["keys"])), key=lambda i: raw["keys"][i])
    st = cases.numpy_stats({k: [raw[k][i] for i in order] for k in raw}, 3, 1)
    split = khg.build_tree(st, [[2], [3], [2, 4], [0, SIL]], sets, p2n, [True] * 4, [False, True, True, True], thresh=10.0, cluster_thresh=0.0)
    assert split.num_pdfs > mono.num_pdfs
    tms = {name: khg.TransitionModel(ctx_dep=t, hmm_topo=topo) for name, t in (("mono", mono), ("flat", flat), ("split", split))}
    return topo, {"mono": mono, "flat": flat, "split": split}, tms


def _compiler(setup, which, form, sil):
    topo, trees, tms = setup
    if form == "dict":
        return khg.TrainingGraphCompiler(tms[which], trees[which], LEXICON, sil_phone=SIL if sil else None, sil_prob=0.5)
    return khg.TrainingGraphCompiler(tms[which], trees[which], khg.make_lexicon_fst_with_silence(LEXICON, SIL, 0.5))


def _shortest(fst):
    dist, frontier, n = {fst.start: 0}, [fst.start], 0
    while frontier:
        if any(fst.is_final(s) for s in frontier):
            return n
        n += 1
        nxt = []
        for s in frontier:
            for a in fst.arcs(s):
                if a.nextstate not in dist:
                    dist[a.nextstate] = n
                    nxt.append(a.nextstate)
        frontier = nxt
    raise AssertionError("no final state")


def _paths(fst, bound):
    """every accepting path of <= bound arcs: {(ilabels, olabels without epsilons, cost rounded)}"""
    out = set()
    arcs = {}

    def walk(s, il, ol, cost):
        if fst.is_final(s):
            out.add((tuple(il), tuple(ol), round(cost + float(fst.final(s)), 4)))
        if len(il) == bound:
            return
        if s not in arcs:
            arcs[s] = [(a.ilabel, a.olabel, float(a.weight), a.nextstate) for a in fst.arcs(s)]
        for (i, o, w, d) in arcs[s]:
            walk(d, il + [i], ol + ([o] if o else []), cost + w)

    walk(fst.start, [], [], 0.0)
    return out


def _signature(tm, tids):
    """what a path is apart from its pdfs: per transition-id (phone, HMM state, index of the arc in its state)"""
    return tuple((tm.transition_id_to_phone(t), tm.transition_id_to_hmm_state(t), t - tm.pair_to_transition_id(tm.transition_id_to_transition_state(t), 0))
                 for t in tids)


def _check_pdfs(tm, tree, topo, tids):
    segs = khg.split_to_phones(tm, list(tids))
    phones = [tm.transition_id_to_phone(s[0]) for s in segs]
    for i, seg in enumerate(segs):
        window = [phones[i - 1] if i > 0 else 0, phones[i], phones[i + 1] if i + 1 < len(phones) else 0]
        entry = topo.topology_for_phone(phones[i])
        for t in seg:
            assert tm.transition_id_to_phone(t) == phones[i]
            st = entry[tm.transition_id_to_hmm_state(t)]
            pc = st.self_loop_pdf_class if tm.is_self_loop(t) else st.forward_pdf_class
            assert (True, tm.transition_id_to_pdf(t)) == tree.compute(window, pc), (phones, i, t)


FORMS = [("dict", False), ("dict", True), ("lfst", True)]


@pytest.mark.parametrize("form,sil", FORMS)
@pytest.mark.parametrize("transcript", TRANSCRIPTS, ids=[str(len(t)) + "w" for t in TRANSCRIPTS])
def test_context_free_tree_gives_the_monophone_graph(setup, form, sil, transcript):
    gm = _compiler(setup, "mono", form, sil).compile_graph_from_text(transcript)
    gf = _compiler(setup, "flat", form, sil).compile_graph_from_text(transcript)
    bound = _shortest(gm) + (4 if sil else 2)
    pm, pf = _paths(gm, bound), _paths(gf, bound)
    print(form, sil, transcript, "bound", bound, "paths", len(pm), "states", gm.num_states, gf.num_states)
    assert pm and pm == pf


@pytest.mark.parametrize("form,sil", FORMS)
@pytest.mark.parametrize("transcript", TRANSCRIPTS, ids=[str(len(t)) + "w" for t in TRANSCRIPTS])
def test_split_tree_paths_and_pdfs(setup, form, sil, transcript):
    topo, trees, tms = setup
    gm = _compiler(setup, "mono", form, sil).compile_graph_from_text(transcript)
    gs = _compiler(setup, "split", form, sil).compile_graph_from_text(transcript)
    bound = _shortest(gm) + (4 if sil else 2)
    pm, ps = _paths(gm, bound), _paths(gs, bound)
    assert {(_signature(tms["mono"], p[0]), p[1], p[2]) for p in pm} == {(_signature(tms["split"], p[0]), p[1], p[2]) for p in ps}
    assert len(pm) == len(ps)            # one tri path per monophone path
    for tids in {p[0] for p in ps}:
        _check_pdfs(tms["split"], trees["split"], topo, tids)


@pytest.mark.parametrize("sil", [False, True])
def test_word_loop_graph_across_the_loop(setup, sil):
    topo, trees, tms = setup
    gm = _compiler(setup, "mono", "dict", sil).compile_word_loop_graph()
    gs = _compiler(setup, "split", "dict", sil).compile_word_loop_graph()
    bound = 9                         # two words of one and two phones with two states each, and a self-loop or a silence start
    pm, ps = _paths(gm, bound), _paths(gs, bound)
    print("word loop", sil, "paths", len(pm), len(ps), "states", gm.num_states, gs.num_states)
    assert any(len(p[1]) >= 2 for p in ps), "the bound must reach across the loop"
    assert {(_signature(tms["mono"], p[0]), p[1], p[2]) for p in pm} == {(_signature(tms["split"], p[0]), p[1], p[2]) for p in ps}
    for tids in {p[0] for p in ps}:
        _check_pdfs(tms["split"], trees["split"], topo, tids)
    gf = _compiler(setup, "flat", "dict", sil).compile_word_loop_graph()
    assert _paths(gf, bound) == pm


def test_unsupported_context_is_refused(setup):
    topo, trees, tms = setup
    bad = ContextDependency(4, 1, trees["flat"].to_pdf)
    with pytest.raises(khg.KhgError, match="N=4"):
        khg.TrainingGraphCompiler(tms["flat"], bad, LEXICON)
