"""The raw lattice of the lattice-faster decoder without a GPU: the C-ABI call and the Python names exist; the
restatement of the rule (tests/lattice_faster_raw_ref.py) on 120 seeded cases -- every lattice passes khg_lattices_validate, and its
best path at (1, 1), by the restatement of the lattice operations (tests/lattice_ops_ref.py) and by the host Lattice, is the decoder
restatement's own (alignment, words, Value1, Value2) on the bits, exact ties included; pruning keeps that path and leaves a trim
lattice; the hand-built graphs of tests/test_lattice_faster_cpu.py."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_faster_raw_ref as rawf  # noqa: E402
import lattice_faster_ref as ref  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
from test_lattice_faster_cpu import _graph, _scores, _star  # noqa: E402
from test_lattice_ops_cpu import _dict, _lattice, _reach  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
N_CASES = 120
BEAMS = [(13.0, 6.0), (6.0, 2.0), (10.0, 4.0)]
MAX_ACTIVE = [7000, 10, 3]
MIN_ACTIVE = [200, 2, 0]


def test_the_call_and_the_names_exist():
    name = "khg_decode_lattice_faster_raw"
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        assert re.search(r"\bint %s\(" % name, fh.read())
    from kaldi_hmm_gmm_amd import _lib
    assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None
    so = os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % name, out, re.M)
    import kaldi_hmm_gmm_amd as khg
    assert khg.get_raw_lattice_faster_batch is khg.align.get_raw_lattice_faster_batch
    assert khg.get_raw_lattice_faster_device_batch is khg.align.get_raw_lattice_faster_device_batch
    assert hasattr(khg.UtteranceSet, "raw_lattice_faster") and hasattr(khg.UtteranceSet, "raw_lattices_faster_device")


def _case(seed):
    """-> (graph dict, scores [T][ntid + 1], Config): random and hub graphs mixed with the beams, the active limits and three kinds
    of scores -- random, rounded to quarters and all zero; the last two make exact ties"""
    rng = np.random.default_rng(1000 + seed)
    ntid = int(rng.integers(3, 12))
    if seed % 2 == 0:
        g = tg.random_graph(rng, ntid, n_main=int(rng.integers(4, 14)), p_branch=0.5, p_eps=0.4)
    else:
        g = tg.hub_graph(rng, ntid, fan=8, tail=5)
    T = int(rng.integers(8, 40))
    m = (rng.standard_normal((T, ntid + 1)) * 3 - 2).astype(np.float32)
    kind = (seed // 2) % 3
    if kind == 1:
        m = (np.round(m * 4) / 4).astype(np.float32)
    elif kind == 2:
        m[:] = 0.0
    beam, lbeam = BEAMS[(seed // 6) % 3]
    max_active = MAX_ACTIVE[(seed // 18) % 3]
    min_active = min(MIN_ACTIVE[int(rng.integers(0, 3))], max_active)
    return g, m, ref.Config(beam=beam, lattice_beam=lbeam, max_active=max_active, min_active=min_active, prune_interval=int(rng.integers(1, 30)))


@functools.lru_cache(maxsize=None)
def _cases():
    out = []
    for seed in range(N_CASES):
        g, m, cfg = _case(seed)
        lat, res = rawf.rule_lattice(ref.Graph.from_dict(g), cfg, lambda f, i, m=m: m[f, i], len(m))
        out.append((seed, lat, res))
    return out


def _num_paths(lat):
    """start -> final paths of an acyclic, top-sorted lattice"""
    N = len(lat["frame"])
    ab, nx = lat["arc_begin"], lat["nextstate"]
    T = lat["frame"][-1]
    cnt = [0] * N
    for s in range(N - 1, -1, -1):
        c = 1 if lat["frame"][s] == T and lat["final_cost"][s] != INF else 0
        for a in range(ab[s], ab[s + 1]):
            assert nx[a] > s                        # top-sorted: GetRawLattice's state order
            c += cnt[nx[a]]
        cnt[s] = c
    return cnt[0]


def test_every_case_decodes():
    cases = _cases()
    assert len(cases) == N_CASES and all(res["succeeded"] for _, _, res in cases)
    kinds = {(s % 2, (s // 2) % 3, (s // 6) % 3, (s // 18) % 3) for s, _, _ in cases}
    assert len(kinds) == 2 * 3 * 3 * 3
    print("states %.0f arcs %.0f per lattice" % (np.mean([len(l["frame"]) for _, l, _ in cases]), np.mean([len(l["ilabel"]) for _, l, _ in cases])))


def test_lattices_are_valid():
    import kaldi_hmm_gmm_amd as khg
    for seed, lat, _ in _cases():
        khg.DeviceLattices.validate([_lattice(lat)])
        fr = lat["frame"]
        assert lat["start"] == 0 and fr[0] == 0 and (np.diff(fr) >= 0).all(), seed
        assert (lat["final_cost"][fr < fr[-1]] == INF).all(), seed
        assert (lat["acoustic_cost"][lat["ilabel"] == 0] == 0).all(), seed


def test_best_path_is_the_decoders():
    """lattice_ops_ref.best_path (Jacobi rounds inside a frame) and the decoder restatement (state-order relaxation on the top-sorted
    lattice) are two tie rules; on every case, tied ones included, they give the same labels and the same two sums."""
    for seed, lat, res in _cases():
        want = (res["alignment"], res["words"], ops.bits(res["weight"]))
        got = ops.best_path(lat, 1.0, 1.0)
        assert got["status"] == ops.SUCCEEDED, seed
        assert (got["ali"], got["words"], ops.bits(got["weight"])) == want, (seed, got["weight"], res["weight"])
        L = _lattice(lat)
        host = L.best_path()
        assert (host["ali"], host["words"], ops.bits(host["weight"])) == want, seed
        lin = L.shortest_path()
        ok, ali, words, _ = lin.get_linear_symbol_sequence()
        assert ok and (ali, words) == want[:2], seed
        v1, v2 = F(0.0), F(0.0)
        for a in lin.arcs:
            v1, v2 = F(v1 + F(a.weight.value1)), F(v2 + F(a.weight.value2))
        v1, v2 = F(v1 + F(lin.final.value1)), F(v2 + F(0.0))
        assert ops.bits((v1, v2)) == want[2], seed
        assert float(F(-F(v1 + v2))) == res["like"], seed


def test_most_lattices_hold_more_than_one_path():
    many = sum(_num_paths(lat) > 1 for _, lat, _ in _cases())
    ties = sum(seed // 2 % 3 != 0 for seed, _, _ in _cases())
    print("lattices with more than one path: %d of %d (%d on tied scores)" % (many, N_CASES, ties))
    assert many > N_CASES // 2


def test_pruning_keeps_the_best_path_and_trims():
    smaller = 0
    for seed, lat, res in _cases():
        L = _lattice(lat)
        for beam in (0.5, float("inf")):
            want, st = ops.prune(lat, beam)
            assert st == ops.SUCCEEDED, (seed, beam)
            P = L.prune(beam)
            assert rawf.same_lattice(P, want) is None, (seed, beam)
            bp = ops.best_path(want)
            assert (bp["ali"], bp["words"], ops.bits(bp["weight"])) == (res["alignment"], res["words"], ops.bits(res["weight"])), (seed, beam)
            acc, co = _reach(_dict(P))
            assert len(acc) == len(co) == P.num_states > 0, (seed, beam)
            smaller += P.num_states < len(lat["frame"]) or P.num_arcs_total < len(lat["ilabel"])
    assert smaller > 0


# ---- the hand-built graphs of tests/test_lattice_faster_cpu.py ----------------------------------------------------------------
def _rule(g, T, table=None, allow_partial=True, **cfg):
    return rawf.rule_lattice(g, ref.Config(**cfg), _scores(table or {}), T, allow_partial)


def test_revisited_epsilon_chain_has_four_links_on_frame_0():
    g = _graph(4, [(0, 0, 7, 5.0, 2), (0, 0, 8, 1.0, 1), (1, 0, 9, 1.0, 2), (2, 0, 11, 0.0, 3), (3, 1, 0, 0.0, 3)], {3: 0.0})
    lat, res = _rule(g, 1)
    assert res["succeeded"] and res["words"] == [8, 9, 11]
    src = ops._src_of(lat)
    eps0 = [a for a in range(len(src)) if lat["frame"][src[a]] == 0 and lat["ilabel"][a] == 0]
    assert len(eps0) == 4 and sorted(int(lat["olabel"][a]) for a in eps0) == [7, 8, 9, 11]
    # the second visit of state 2 regenerated its one link: state 2 has exactly one arc
    s2 = [s for s in range(len(lat["frame"])) if lat["frame"][s] == 0 and lat["graph_state"][s] == 2]
    assert len(s2) == 1 and lat["arc_begin"][s2[0] + 1] - lat["arc_begin"][s2[0]] == 1
    # frame 0 in TopSortTokens order: every epsilon arc goes up
    assert all(lat["nextstate"][a] > src[a] for a in range(len(src)))
    assert lat["graph_state"][: 4].tolist() == [0, 1, 2, 3] and lat["frame"].tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("allow_partial", [True, False])
def test_no_final_state_makes_every_last_token_final(allow_partial):
    g = _graph(3, [(0, 1, 3, 0.5, 1), (0, 2, 4, 1.5, 2)], {})
    lat, res = _rule(g, 1, allow_partial=allow_partial)
    assert res["partial"]
    if not allow_partial:
        assert len(lat["frame"]) == 0 and lat["start"] == -1
        return
    last = lat["frame"] == 1
    assert last.sum() == 2 and ops.bits(lat["final_cost"][last]) == ops.bits([0.0, 0.0])
    assert sorted(lat["graph_state"][last].tolist()) == [1, 2]


def test_star_graph_under_max_active_loses_branch_4():
    table = {(1, 9): 10.0}
    cut, _ = _rule(_star(), 2, table, beam=100.0, max_active=2, min_active=0)
    full, _ = _rule(_star(), 2, table, beam=100.0, max_active=7000, min_active=0)

    def states(lat, f):
        return sorted(lat["graph_state"][lat["frame"] == f].tolist())
    assert 4 in states(full, 1) and 4 in states(full, 2)
    assert 4 not in states(cut, 2)
    assert 1 in states(cut, 2)
