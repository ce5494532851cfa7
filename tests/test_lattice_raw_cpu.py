"""The raw lattice of the lattice-simple decoder without a GPU: the order-independent rule the kernels
follow (tests/lattice_raw_ref.py) against the reference's GetRawLattice as restated in tests/lattice_simple_ref.py, for three walk
orders of its hash maps; hand-built graphs; the host Lattice class; the C-ABI symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_raw_ref as raw  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
from test_lattice_simple_cpu import WALKS, _graph, _random_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)


def _walk(g, cfg, ll, T, walk, seed):
    """-> (decoder, decoded) or (None, False) where the reference throws"""
    dec = ref.LatticeSimpleDecoder(ref.Graph.from_dict(g), cfg, walk, seed)
    try:
        ok = dec.decode(ll, T)
    except ref.DecodeError:
        return None, False
    return dec, ok


def test_rule_is_a_subset_and_equal_without_late_links():
    """For every decoding (case, walk) pair the rule's lattice is a subset of the walk's, and equal to it -- costs included, bit for
    bit -- whenever the walk's holds no emitting link of cost >= its frame's fl(best + beam)."""
    pairs = clean = clean_nonzero = cases = 0
    for seed in range(220):
        g, m, cfg = _random_case(seed)
        ll, T = ref.matrix_ll(m), len(m)
        decs = [_walk(g, cfg, ll, T, w, seed) for w in WALKS]
        if not all(ok for _, ok in decs):
            continue
        cases += 1
        lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ll, T)
        assert lat is not None, seed
        rtoks, rlinks = raw.lattice_sets(lat)
        pcut = lat["rows"]["pcut"]
        for (dec, _), walk in zip(decs, WALKS):
            pairs += 1
            wtoks, wlinks, wfin = raw.walk_lattice(dec)
            for k, v in rtoks.items():
                assert k in wtoks and raw.bits(v[0]) == raw.bits(wtoks[k][0]), (seed, walk, k)
            for k, v in rlinks.items():
                assert k in wlinks and raw.same_link(v, wlinks[k]), (seed, walk, k)
            late = False
            for (f, s, a), (il, _, gc, ac, _) in wlinks.items():
                if il != 0 and not (F(F(wtoks[(f, s)][0] + ac) + gc) < pcut[f + 1]):
                    late = True
            if late:
                continue
            clean += 1
            assert set(rtoks) == set(wtoks) and set(rlinks) == set(wlinks), (seed, walk)
            assert all(raw.same_token(rtoks[k], wtoks[k]) for k in rtoks), (seed, walk)
            fin = {(int(lat["frame"][i]), int(lat["graph_state"][i])): lat["final_cost"][i] for i in range(len(lat["frame"]))
                   if lat["final_cost"][i] != INF}
            assert set(fin) == set(wfin) and all(raw.bits(fin[k]) == raw.bits(wfin[k]) for k in fin), (seed, walk)
            clean_nonzero += any(v[1] != 0.0 for v in rtoks.values())
    print("cases %d pairs %d clean %d clean with a nonzero extra cost %d" % (cases, pairs, clean, clean_nonzero))
    # the second assertion is not vacuous
    assert clean >= 250 and clean_nonzero >= 50, (cases, pairs, clean, clean_nonzero)


def _lattice(lat):
    import kaldi_hmm_gmm_amd as khg
    return khg.Lattice.from_arrays(*[lat[k] for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel",
                                                      "graph_cost", "acoustic_cost", "nextstate")], int(lat["start"]))


def test_shortest_path_of_the_rule_lattice_is_the_decoders_best_path():
    n = 0
    for seed in range(0, 220, 3):
        g, m, cfg = _random_case(seed)
        ll, T = ref.matrix_ll(m), len(m)
        try:
            want = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), cfg, ll, T)
        except ref.DecodeError:
            continue
        if not want["succeeded"]:
            continue
        lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ll, T)
        lin = _lattice(lat).shortest_path()
        ok, ali, words, _ = lin.get_linear_symbol_sequence()
        assert ok and ali == want["alignment"] and words == want["words"], seed
        assert raw.path_like(lin) == want["like"], seed
        n += 1
    assert n >= 30


def test_final_weights_and_epsilon_chain():
    # an epsilon chain 0 -> 1 -> 2 (words 7, 8) next to the direct arc 0 -> 2 (word 9, dearer); 2 emits into the final states 3 and 4
    arcs = [(0, 0, 0, 0.0, 0), (0, 0, 9, 5.0, 2), (0, 0, 7, 1.0, 1), (1, 0, 0, 0.0, 1), (1, 0, 8, 1.0, 2), (2, 0, 0, 0.0, 2),
            (2, 1, 0, 0.25, 3), (2, 1, 0, 0.5, 4), (3, 0, 0, 0.5, 3), (4, 0, 0, 0.5, 4)]      # (a zero-weight loop would pin 4's extra cost at 0)
    g = _graph(5, 0, arcs, {3: 0.125, 4: 0.0})
    m = np.array([[-0.5]], np.float32)
    cfg = ref.Config(beam=16.0, lattice_beam=10.0)
    lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ref.matrix_ll(m), 1)
    toks, links = raw.lattice_sets(lat)
    assert set(toks) == {(0, 0), (0, 1), (0, 2), (1, 3), (1, 4)}
    assert lat["start"] == 0
    # the chain's two arcs and the direct arc (extra cost 3 <= lattice_beam) all survive; both emitting arcs; the five self-loops
    assert len(links) == 3 + 2 + 5
    fin = {int(lat["graph_state"][i]): float(lat["final_cost"][i]) for i in range(len(lat["frame"])) if lat["final_cost"][i] != INF}
    assert fin == {3: 0.125, 4: 0.0}
    assert all(lat["final_cost"][i] == INF for i in range(len(lat["frame"])) if lat["frame"][i] == 0)
    assert float(toks[(0, 2)][0]) == 2.0 and float(toks[(1, 3)][0]) == 2.75 and float(toks[(1, 3)][1]) == 0.0
    assert float(toks[(1, 4)][1]) == 0.125          # (3.0 + 0) - (2.75 + 0.125)
    for walk in WALKS:
        dec, ok = _walk(g, cfg, ref.matrix_ll(m), 1, walk, 0)
        wtoks, wlinks, wfin = raw.walk_lattice(dec)
        assert ok and set(wtoks) == set(toks) and set(wlinks) == set(links)
        assert {k[1]: float(v) for k, v in wfin.items()} == fin
    # lattice_beam 2: the direct arc (extra cost 3) is excised
    lat2 = raw.rule_lattice(ref.Graph.from_dict(g), ref.Config(beam=16.0, lattice_beam=2.0), ref.matrix_ll(m), 1)
    assert len(lat2["ilabel"]) == len(lat["ilabel"]) - 1 and lat2["excised"] >= 1
    assert 9 not in lat2["olabel"].tolist()


def test_state_pruned_by_prune_current_tokens_and_recreated_by_the_closure():
    # frame 0: arc to 1 (tot 20) and to 2 (tot 1); PruneCurrentTokens (beam 16) drops state 1; the closure re-creates it from 2 through
    # an epsilon arc of weight 3.  The pruned twin (cost 20) and the emitting link into it must not appear.
    arcs = [(0, 0, 0, 0.0, 0), (0, 1, 0, 0.0, 1), (0, 2, 0, 0.0, 2), (1, 0, 0, 0.0, 1), (2, 0, 0, 0.0, 2), (2, 0, 5, 3.0, 1)]
    g = _graph(3, 0, arcs, {1: 0.0, 2: 1.0})
    m = np.array([[-20.0, -1.0]], np.float32)
    cfg = ref.Config(beam=16.0, lattice_beam=10.0)
    lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ref.matrix_ll(m), 1)
    toks, links = raw.lattice_sets(lat)
    assert set(toks) == {(0, 0), (1, 1), (1, 2)}
    assert float(toks[(1, 1)][0]) == 4.0             # the re-created token, not the twin of cost 20
    assert (0, 0, 1) not in links and (0, 0, 2) in links and (1, 2, 5) in links
    for walk in WALKS:
        dec, ok = _walk(g, cfg, ref.matrix_ll(m), 1, walk, 0)
        wtoks, wlinks, _ = raw.walk_lattice(dec)
        assert ok and set(wtoks) == set(toks) and set(wlinks) == set(links)
        assert all(raw.same_token(toks[k], wtoks[k]) for k in toks)


def test_lattice_round_trips():
    import kaldi_hmm_gmm_amd as khg
    g, m, cfg = _random_case(8)
    for seed in range(8, 220):
        g, m, cfg = _random_case(seed)
        lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ref.matrix_ll(m), len(m))
        if lat is not None and lat["paths_gt_1"] and len(lat["ilabel"]) > 20:
            break
    L = _lattice(lat)
    N = len(lat["frame"])
    assert L.num_states == N and L.start == lat["start"] and L.num_arcs_total == len(lat["ilabel"])
    for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost",
              "nextstate"):
        v = getattr(L, k)
        assert v.dtype == lat[k].dtype and v.tobytes() == lat[k].tobytes(), k
        assert not v.flags.writeable
        with pytest.raises(ValueError):
            v[...] = 0
    text = []
    for s in range(N):
        arcs = L.arcs(s)
        assert L.num_arcs(s) == len(arcs) == lat["arc_begin"][s + 1] - lat["arc_begin"][s]
        for j, a in zip(range(lat["arc_begin"][s], lat["arc_begin"][s + 1]), arcs):
            assert isinstance(a, khg.LatticeArc)
            assert (a.ilabel, a.olabel, a.nextstate) == (lat["ilabel"][j], lat["olabel"][j], lat["nextstate"][j])
            assert (a.weight.value1, a.weight.value2) == (float(lat["graph_cost"][j]), float(lat["acoustic_cost"][j]))
            text.append("%d %d %d %d %.9g,%.9g" % (s, a.nextstate, a.ilabel, a.olabel, a.weight.value1, a.weight.value2))
        w = L.final(s)
        if lat["final_cost"][s] == INF:
            assert w.value1 == np.inf and w.value2 == np.inf
        else:
            assert (w.value1, w.value2) == (float(lat["final_cost"][s]), 0.0)
    text += ["%d %.9g,0" % (s, float(lat["final_cost"][s])) for s in range(N) if lat["final_cost"][s] != INF]
    assert L.to_text() == "\n".join(text) + "\n" == str(L)
    # text -> arrays: every arc line parses back to the arc it came from
    rows = [ln.split() for ln in L.to_text().splitlines() if len(ln.split()) == 5]
    assert [int(r[1]) for r in rows] == lat["nextstate"].tolist()
    assert [F(r[4].split(",")[0]) for r in rows] == lat["graph_cost"].tolist()
    # bad arrays are refused
    bad = dict(lat)
    bad["nextstate"] = lat["nextstate"].copy()
    bad["nextstate"][0] = N
    with pytest.raises(RuntimeError, match="nextstate"):
        _lattice(bad)
    empty = khg.Lattice.from_arrays([], [], [], [], [], [0], [], [], [], [], [], -1)
    assert empty.num_states == 0 and empty.start == -1 and empty.shortest_path().num_states == 0 and empty.to_text() == ""


def test_shortest_path_tie_rule():
    import kaldi_hmm_gmm_amd as khg
    # two paths of exactly the same weight into the last state: through lattice state 1 and through 2; the lower source wins
    L = khg.Lattice.from_arrays([0, 1, 1, 2], [0, 1, 2, 3], [0, 1, 1, 2], [0, 0, 0, 0], [np.inf, np.inf, np.inf, 0.5], [0, 2, 3, 4, 4],
                                [2, 1, 3, 4], [0, 0, 11, 12], [1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [2, 1, 3, 3], 0)
    lin = L.shortest_path()
    ok, ali, words, w = lin.get_linear_symbol_sequence()
    assert ok and ali == [1, 3] and words == [11] and (w.value1, w.value2) == (1.5, 2.0)
    assert raw.path_like(lin) == -3.5 and lin.num_states == 3 and lin.final.value1 == 0.5


def test_cabi_symbols():
    names = ["khg_decode_lattice_simple_raw", "khg_lattices_sizes", "khg_lattices_download", "khg_lattices_device_bytes", "khg_lattices_destroy"]
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header), n
    assert "typedef struct khg_lattices khg_lattices;" in header
    from kaldi_hmm_gmm_amd import _lib
    for n in names:
        assert n in _lib.SIGNATURES and getattr(_lib.lib, n) is not None, n
    so = os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r" T %s$" % n, out, re.M), n
    import kaldi_hmm_gmm_amd as khg
    assert khg.Lattice is khg.align.Lattice and khg.get_raw_lattice_simple_batch is khg.align.get_raw_lattice_simple_batch
