"""Inputs for the forward-backward posteriors, shared by tests/test_lattice_post_cpu.py (the host Lattice) and
tests/test_gpu_lattice_post.py (the device): hand-built lattices small enough for the brute-force sum over paths, and lattices that
reach the kernels' geometry -- frames wider than a wave, states at and past the hub threshold, an epsilon chain longer than a wave,
merges across 64-arc tiles, and the LDS staging threshold of k2_lattice_post_fb.  Plain Python and numpy."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_post_ref as pr  # noqa: E402
from lattice_geometry_cases import _padded, _wide_lattice  # noqa: E402
from test_lattice_ops_cpu import _hand  # noqa: E402

INF = np.inf
SCALES = [(1.0, 1.0), (1.0, 0.1), (0.5, 1.7), (1.0, 0.0), (0.0, 1.0)]
HUB = 64                        # PO_HUB: a state with more arcs than this is taken by a whole wave
POST_LDS_LIMIT = 48 * 1024      # kLatOpsLds: 24 N + 4 (3 N + 4 A) bytes are staged up to this


def post_staged_bytes(lat):
    N, A = len(lat["frame"]), len(lat["ilabel"])
    return 24 * N + 4 * (3 * N + 4 * A)


_WANT = {}


def want(lat, gs, as_):
    """pr.forward_backward(lat, gs, as_), kept per (lattice object, pair)"""
    k = (id(lat["frame"]), float(np.float32(gs)), float(np.float32(as_)))
    if k not in _WANT:
        _WANT[k] = (lat, pr.forward_backward(lat, gs, as_))
    return _WANT[k][1]


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> lattice; each has at most a few hundred paths (enumerate_paths)"""
    c = {}
    c["diamond"] = _hand([(0, INF), (1, INF), (1, INF), (2, 0.5)],
                         [(0, 1, 0, 1.0, 2.0, 1), (0, 2, 0, 0.5, 3.0, 2), (1, 3, 11, 0.25, 1.0, 3), (2, 4, 12, 0.0, 0.5, 3)])
    # an epsilon chain of depth 5 inside frame 0 (and a shortcut), every state of it emitting into frame 1
    st = [(0, INF)] * 6 + [(1, 0.0), (1, 1.5)]
    ar = [(s, 0, 0, 0.3 + 0.1 * s, 0.0, s + 1) for s in range(5)] + [(0, 0, 0, 2.0, 0.0, 3)]
    ar += [(s, 1 + s % 3, 0, 0.2 * s, 1.0 + 0.5 * s, 6 + s % 2) for s in range(6)]
    c["epsilon_chain_5"] = _hand(st, ar)
    # epsilon arcs s -> s + 1 and s -> s + 2 in two frames
    st = [(0, INF)] * 5 + [(1, INF)] * 4 + [(2, 0.0), (2, 0.25)]
    ar = []
    for lo, hi in ((0, 5), (5, 9)):
        for s in range(lo, hi):
            if s + 1 < hi:
                ar.append((s, 0, 0, 0.4, 0.0, s + 1))
            if s + 2 < hi:
                ar.append((s, 0, 0, 0.9, 0.0, s + 2))
    ar += [(s, 1 + s, 0, 0.1 * s, 2.0 - 0.3 * s, 5 + s % 4) for s in range(5)]
    ar += [(s, 10 + s, 0, 0.2, 0.7 * (s - 4), 9 + s % 2) for s in range(5, 9)]
    c["epsilon_skips"] = _hand(st, ar)
    # two arcs with the same id between the same two states, a third with that id into another state: one entry
    c["same_id_merged"] = _hand([(0, INF), (1, INF), (1, INF), (2, 0.0)],
                                [(0, 5, 0, 1.0, 1.0, 1), (0, 5, 0, 0.5, 2.0, 1), (0, 5, 0, 0.25, 1.5, 2), (0, 3, 0, 0.0, 2.5, 2),
                                 (1, 7, 0, 0.0, 1.0, 3), (2, 7, 0, 1.0, 0.0, 3), (2, 6, 0, 0.5, 0.25, 3)])
    # ids in arc order 9, 2, 7, 2, 1: the entries come out ascending
    c["ids_out_of_order"] = _hand([(0, INF), (1, INF), (1, INF), (1, INF), (2, 0.0)],
                                  [(0, 9, 0, 1.0, 1.0, 1), (0, 2, 0, 0.5, 2.0, 2), (0, 7, 0, 0.25, 1.5, 3), (0, 2, 0, 0.0, 2.5, 1), (0, 1, 0, 0.0, 2.0, 3),
                                   (1, 8, 0, 0.0, 1.0, 4), (2, 4, 0, 1.0, 0.0, 4), (3, 6, 0, 0.5, 0.25, 4)])
    return c


def dead_states():
    """(lattice, dead arcs): state 2 is not reached from the start, state 3 reaches no final state (its successor's final cost is
    +inf, as after a prune that dropped it); ids 40 .. 43 sit on dead arcs only, id 1 on a dead and a live arc"""
    lat = _hand([(0, INF), (1, INF), (1, INF), (1, INF), (2, 0.0), (2, INF)],
                [(0, 1, 0, 1.0, 1.0, 1), (0, 40, 0, 0.5, 1.0, 3), (1, 2, 0, 0.0, 1.0, 4), (1, 41, 0, 0.0, 1.0, 5), (2, 42, 0, 0.0, 1.0, 4),
                 (2, 1, 0, 0.0, 1.0, 5), (3, 43, 0, 0.0, 1.0, 5), (0, 1, 0, 2.0, 0.0, 3)])
    return lat, [1, 2, 4, 5, 6, 7]


def one_path(T=7):
    """a linear lattice with an epsilon arc in it"""
    st = [(0, INF), (0, INF)] + [(t, INF) for t in range(1, T)] + [(T, 0.75)]
    ar = [(0, 0, 3, 0.5, 0.0, 1)] + [(1 + t, 1 + t, 0, 0.125 * t, 1.0 + 0.25 * t, 2 + t) for t in range(T)]
    return _hand(st, ar)


def in_degree(D):
    """frame 0: the start and D - 1 states behind epsilon arcs from it; all D of them emit into state D of frame 1 (in-degree D) and
    into state D + 1; the start's out-degree is D + 1"""
    rng = np.random.default_rng(D)
    st = [(0, INF)] * D + [(1, INF), (1, INF), (2, 0.0)]
    ar = [(0, 0, 0, float(rng.uniform(0.1, 2)), 0.0, k) for k in range(1, D)]
    for s in range(D):
        ar.append((s, 1 + s % 5, 0, float(rng.uniform(0, 2)), float(rng.uniform(0, 5)), D))
        ar.append((s, 1 + s % 7, 0, float(rng.uniform(0, 2)), float(rng.uniform(0, 5)), D + 1))
    ar += [(D, 3, 0, 0.5, 1.0, D + 2), (D + 1, 4, 0, 0.25, 2.0, D + 2)]
    return _hand(st, ar)


def epsilon_chain(n=70):
    """n states of frame 0 in one epsilon chain: the Jacobi rounds exceed the wave width"""
    st = [(0, INF)] * n + [(1, 0.0), (1, 0.5)]
    ar = [(s, 0, 0, 0.05 + 0.01 * (s % 7), 0.0, s + 1) for s in range(n - 1)]
    ar += [(s, 1 + s % 4, 0, 0.1, 0.5 + 0.1 * (s % 9), n + s % 2) for s in range(n)]
    return _hand(st, ar)


def three_ids_130_arcs():
    """frame 0: 13 states (the start and 12 behind epsilon arcs), each with 10 emitting arcs into frame 1: 130 arcs over ids 1, 2, 3,
    every id in both full 64-arc tiles"""
    rng = np.random.default_rng(130)
    st = [(0, INF)] * 13 + [(1, float(rng.uniform(0, 1))) for _ in range(10)]
    ar = [(0, 0, 0, 0.5, 0.0, k) for k in range(1, 13)]
    for s in range(13):
        for j in range(10):
            ar.append((s, 1 + (s * 10 + j) % 3, 0, float(rng.uniform(0, 1)), float(rng.uniform(0, 4)), 13 + j))
    lat = _hand(st, ar)
    em = lat["ilabel"][lat["ilabel"] != 0]
    assert len(em) == 130 and all(set(em[t: t + 64]) == {1, 2, 3} for t in (0, 64))
    return lat


def descending_ids(n=65):
    """the start with n emitting arcs whose ids run n, n - 1, .. 1"""
    st = [(0, INF)] + [(1, 0.1 * (k % 5)) for k in range(n)]
    ar = [(0, n - k, 0, 0.01 * k, 0.5 + 0.03 * (k % 11), 1 + k) for k in range(n)]
    return _hand(st, ar)


@functools.lru_cache(maxsize=None)
def geometry():
    """name -> lattice"""
    rng = np.random.default_rng(77)
    c = {"wide_%d" % W: _wide_lattice(rng, 2, W, 3) for W in (63, 64, 65, 130)}
    for D in (HUB, HUB + 1, HUB + 2, 200):
        c["in_degree_%d" % D] = in_degree(D)
    c["epsilon_chain_70"] = epsilon_chain(70)
    c["three_ids_130_arcs"] = three_ids_130_arcs()
    c["descending_ids_65"] = descending_ids(65)
    for lat in c.values():
        assert pr.admissible(lat)
    return c


@functools.lru_cache(maxsize=None)
def post_lds_edge():
    """{"at": 24 N + 4 (3 N + 4 A) = 49152 exactly (staged), "over": 49156, the next size that exists (9 N + 4 A takes every integer
    from some point on; not staged)}"""
    rng = np.random.default_rng(4813)
    at = _padded(rng, 23, 16, 5, 2208)                # N = 384: 9 N + 4 A = 3456 + 8832 = 12288
    over = _padded(rng, 24, 13, 6, 2341)              # N = 325: 9 N + 4 A = 2925 + 9364 = 12289
    assert len(at["frame"]) == 384 and len(over["frame"]) == 325
    assert post_staged_bytes(at) == POST_LDS_LIMIT and post_staged_bytes(over) == POST_LDS_LIMIT + 4
    assert pr.admissible(at) and pr.admissible(over)
    return {"at": at, "over": over}


def eps_self_loop():
    return _hand([(0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 0), (0, 1, 0, 1.0, 1.0, 1)])


def eps_to_lower_state():
    return _hand([(0, INF), (0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 1), (1, 0, 0, 0.5, 0.0, 0), (1, 1, 0, 1.0, 1.0, 2)])


def no_reachable_final():
    return _hand([(0, INF), (1, INF), (1, 0.0)], [(0, 1, 0, 1.0, 1.0, 1)])
