"""LatticeFasterDecoder without a GPU: the bound names against the reference's signatures, and the plain-Python restatement
(tests/lattice_faster_ref.py, the yardstick of tests/test_gpu_lattice_faster.py) on hand-built graphs with hand-computed answers."""
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_faster_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _sig():
    with open(os.path.join(ROOT, "tests", "golden", "lattice_decoder_signatures.json")) as fh:
        return json.load(fh)


def _doc_args(fn):
    """pybind11's signature line -> [(name, default text or None)]"""
    line = fn.__doc__.strip().splitlines()[0]
    inner = line[line.index("(") + 1: line.rindex(")")]
    out = []
    for part in re.split(r",\s*(?![^\[]*\])", inner):
        name = part.split(":")[0].strip()
        if name == "self":
            continue
        out.append((name, part.split(" = ", 1)[1] if " = " in part else None))
    return out


@pytest.mark.parametrize("cname", sorted(_sig()["classes"]))
def test_class_signature_matches_reference(cname):
    import kaldi_hmm_gmm_amd as khg
    want = _sig()["classes"][cname]
    cls = getattr(khg, cname)
    got = _doc_args(cls.__init__)
    assert [n for n, _ in got] == [n for n, _ in want["args"]]
    for (n, d), (_, wd) in zip(got, want["args"]):
        assert (d is None) == (wd == "required"), n
    if want["args"][0][1] != "required":
        obj = cls()
        for n, wd in want["args"]:
            if wd is None:
                continue
            v = getattr(obj, n)
            assert v == pytest.approx(wd, rel=1e-7) if isinstance(wd, float) else v == wd, n
    for f in want["fields"]:
        assert isinstance(getattr(cls, f), property), f
    if want["str"]:
        assert str(cls()).startswith(cname + "(")


def test_function_signature_matches_reference():
    import kaldi_hmm_gmm_amd as khg
    for fname, want in _sig()["functions"].items():
        got = _doc_args(getattr(khg, fname))
        assert [n for n, _ in got] == [n for n, _ in want["args"]]
        assert all(d is None for _, d in got)
        assert getattr(khg, fname).__doc__.strip().splitlines()[0].endswith("-> " + want["returns"])


def test_config_str_and_alias():
    import kaldi_hmm_gmm_amd as khg
    c = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    assert str(c) == ("LatticeFasterDecoderConfig(beam=13, max_active=7000, min_active=200, lattice_beam=6, prune_interval=25, "
                      "determinize_lattice=True, beam_delta=0.5, hash_ratio=2, prune_scale=0.1, memory_pool_tokens_block_size=256, "
                      "memory_pool_links_block_size=256)")
    assert khg.LatticeFasterDecoderStdVectorFst is khg.LatticeFasterDecoder
    with pytest.raises(Exception):
        khg.LatticeFasterDecoder(khg.StdVectorFst(), khg.LatticeFasterDecoderConfig(prune_scale=1.5))


def test_restatement_hashlist_pinned_to_the_reference():
    """tests/golden/hashlist_ref_fresh.json: the reference's own HashList answers to the script of tests/test_oracle_pins.py."""
    rng = np.random.default_rng(77)
    script = ["S 64"]
    for f in range(60):
        script += ["D", f"S {64 + 8 * f}"] + [f"I {int(k)} {f}" for k in rng.integers(0, 3000, size=int(rng.integers(5, 400)))] + ["L"]
        script += [f"F {int(k)}" for k in rng.integers(0, 3000, size=5)]
    with open(os.path.join(ROOT, "tests", "golden", "hashlist_ref_fresh.json")) as fh:
        gold = json.load(fh)
    assert gold["script_sha1"] == hashlib.sha1("\n".join(script).encode()).hexdigest()
    h = ref.HashList()
    ans, bits = [], []

    def flush():
        if bits:
            ans.append("I= " + "".join(bits))
            bits.clear()
    for line in script:
        a = line.split()
        if a[0] == "I":
            e, _ = h.insert_elem(int(a[1]), int(a[2]))       # the harness answers "value now equals the one inserted"
            bits.append("1" if e.val == int(a[2]) else "0")
        elif a[0] == "S":
            h.set_size(int(a[1]))
        elif a[0] == "D":
            h.drop()
        elif a[0] == "F":
            flush()
            v = h.find(int(a[1]))
            ans.append("F none" if v is None else f"F {v}")
        elif a[0] == "L":
            flush()
            txt = "L" + "".join(f" {k}:{v}" for k, v in h.items())
            ans.append("L# %d %s" % (txt.count(":"), hashlib.sha1(txt.encode()).hexdigest()[:16]) if txt.count(":") > 12 else txt)
    flush()
    assert ans == gold["answers"]


# ---- hand-built graphs -------------------------------------------------------------------------------------------------------
def _graph(nstates, arcs, final, start=0):
    arcs = sorted(arcs, key=lambda a: a[0])          # stable: arcs of a state keep their order
    off = [0] * (nstates + 1)
    for a in arcs:
        off[a[0] + 1] += 1
    off = list(np.cumsum(off))
    fin = [np.inf] * nstates
    for s, w in final.items():
        fin[s] = w
    return ref.Graph(start, off, [a[1] for a in arcs], [a[2] for a in arcs], [a[3] for a in arcs], [a[4] for a in arcs], fin)


def _scores(table):
    return lambda f, i: F(table.get((f, i), 0.0))


def _decode(g, T, table=None, allow_partial=True, **cfg):
    return ref.decode_utterance_lattice_faster(g, ref.Config(**cfg), _scores(table or {}), T, allow_partial)


def _star():
    """0 -> i (i = 1..5) on tid i, weight i - 1, olabel i; state i: self-loop tid 5 + i, weight 0, final 0."""
    arcs = [(0, i, i, float(i - 1), i) for i in range(1, 6)] + [(i, 5 + i, 0, 0.0, i) for i in range(1, 6)]
    return _graph(6, arcs, {i: 0.0 for i in range(1, 6)})


def test_max_active_cut_and_adaptive_beam():
    """Frame 1 holds states 1..5 at costs 0..4.  State 4's self-loop scores +10 on frame 1 (path cost 3 - 10 = -7, the best).
    max_active 2: GetCutoff's cutoff is the 2nd order statistic, 2.0 (< beam cutoff 100): states 1-3 expand, 4 does not, the best
    path left is 0 -> 1 -> 1 (words [1], like -0).  max_active 7000: state 4 survives (words [4], like = -(3 + -10) = 7)."""
    table = {(1, 9): 10.0}
    cut = _decode(_star(), 2, table, beam=100.0, max_active=2, min_active=0)
    assert cut["succeeded"] and cut["words"] == [1] and cut["alignment"] == [1, 6] and cut["like"] == 0.0
    full = _decode(_star(), 2, table, beam=100.0, max_active=7000, min_active=0)
    assert full["words"] == [4] and full["alignment"] == [4, 9] and full["like"] == 7.0


def test_min_active_branch():
    """beam 0.5.  min_active 0 (the fast GetCutoff branch): the online next_cutoff of frame 0 (0 + 0.5) keeps only state 1.
    min_active 4: frame 0 has one token (< min_active: cutoff and adaptive beam infinite), frame 1 has five, the 4th order
    statistic 4.0 is looser than the beam (adaptive beam 4 + 0.5): state 4 is expanded and wins (like 7)."""
    table = {(1, 9): 10.0}
    narrow = _decode(_star(), 2, table, beam=0.5, min_active=0)
    assert narrow["words"] == [1] and narrow["like"] == 0.0
    wide = _decode(_star(), 2, table, beam=0.5, min_active=4)
    assert wide["words"] == [4] and wide["alignment"] == [4, 9] and wide["like"] == 7.0


def test_epsilon_chain_revisited_deletes_links():
    """0 -eps/7 (5)-> 2, 0 -eps/8 (1)-> 1, 1 -eps/9 (1)-> 2, 2 -eps/11 (0)-> 3, 3 self-loop tid 1, final 0.  LIFO queue: state 1 is
    popped first and improves state 2 (5 -> 2), which is queued twice; its second visit deletes and regenerates its one link.
    Frame 0 then holds 4 links (not 5); the best path reads words 8, 9, 11 at like -(2 + 0)."""
    g = _graph(4, [(0, 0, 7, 5.0, 2), (0, 0, 8, 1.0, 1), (1, 0, 9, 1.0, 2), (2, 0, 11, 0.0, 3), (3, 1, 0, 0.0, 3)], {3: 0.0})
    dec = ref.LatticeFasterDecoder(g, ref.Config())
    dec.init_decoding()
    assert sum(len(t.links) for t in dec.active_toks[0].toks) == 4
    r = _decode(g, 1)
    assert r["succeeded"] and r["words"] == [8, 9, 11] and r["alignment"] == [1] and r["like"] == -2.0


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(T):
    """0 self-loop tid 1 (0.1), 0 -> 1 tid 2 (0.2), 1 self-loop tid 3 (0), 1 final 0; all scores 0: the best path leaves state 0 on
    the first frame, alignment [2, 3, ...], like -0.2f -- with PruneActiveTokens running at frame 25 when T > 25."""
    g = _graph(2, [(0, 1, 0, 0.1, 0), (0, 2, 5, 0.2, 1), (1, 3, 0, 0.0, 1)], {1: 0.0})
    r = _decode(g, T, prune_interval=25, lattice_beam=1.0)
    assert r["succeeded"] and not r["partial"]
    assert r["alignment"] == [2] + [3] * (T - 1) and r["words"] == [5]
    assert r["like"] == float(F(-F(0.2)))


@pytest.mark.parametrize("allow_partial", [True, False])
def test_allow_partial(allow_partial):
    """No final state anywhere: ReachedFinal() is false; with allow_partial every last-frame token is final with One() and the
    cheaper branch (tid 1, weight 0.5, word 3) is returned, else nothing."""
    g = _graph(3, [(0, 1, 3, 0.5, 1), (0, 2, 4, 1.5, 2)], {})
    r = _decode(g, 1, allow_partial=allow_partial)
    assert r["partial"]
    if allow_partial:
        assert r["succeeded"] and r["alignment"] == [1] and r["words"] == [3] and r["like"] == -0.5
    else:
        assert not r["succeeded"] and r["alignment"] == [] and r["words"] == []


@pytest.mark.parametrize("first", ["graph_heavy", "graph_light"])
def test_tie_equal_sums_different_graph_cost(first):
    """Two arcs 0 -> 1: A (tid 1, weight 1, word 10) scores ll 1 -> (1, -1); B (tid 2, weight 0, word 20) scores 0 -> (0, 0).  Equal
    sums: LatticeWeight's order then compares Value1, so B wins whatever the arc order."""
    A, B = (0, 1, 10, 1.0, 1), (0, 2, 20, 0.0, 1)
    g = _graph(2, [A, B] if first == "graph_heavy" else [B, A], {1: 0.0})
    r = _decode(g, 1, {(0, 1): 1.0})
    assert r["words"] == [20] and r["alignment"] == [2] and r["like"] == 0.0


@pytest.mark.parametrize("order", [0, 1])
def test_tie_identical_pairs(order):
    """Two arcs 0 -> 1 with identical weights (0.5, 0): the forward links of state 0 are head-first (the arc added last is
    relaxed first) and only a strictly better pair replaces a predecessor: the graph's LAST arc is on the path."""
    A, B = (0, 1, 10, 0.5, 1), (0, 2, 20, 0.5, 1)
    arcs = [A, B] if order == 0 else [B, A]
    r = _decode(_graph(2, arcs, {1: 0.0}), 1)
    assert r["words"] == [arcs[-1][2]] and r["like"] == -0.5
