"""Inputs that reach the launch geometry of the lattice operations (K2O): scale-pair sweeps wider than one
wave whose lanes disagree, pairs that mix statuses inside one wave, handles of more than 64 and more than 4096 utterances, lattices
whose kept and dropped states straddle every 64-state tile edge, and lattices at the LDS staging threshold.  Plain Python and numpy:
every property a builder promises is asserted here from the restatement (tests/lattice_ops_ref.py) alone, never from the device.
tests/test_lattice_geometry_cpu.py checks the promises on any machine; tests/test_gpu_lattice_geometry.py sends the inputs to the
device."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_ops_ref as ops  # noqa: E402
from test_lattice_ops_cpu import _cases, _hand, hand_cases  # noqa: E402

F = np.float32
TILE = 64                      # LO_NT: states per tile of k2_lattice_prune_mark, utterances per tile of the scans, pairs per wave
LDS_LIMIT = 48 * 1024          # kLatOpsLds: an utterance's staged arrays, 4 * (3 N + 4 A) bytes, fit up to this


def staged_bytes(lat):
    return 4 * (3 * len(lat["frame"]) + 4 * len(lat["ilabel"]))


# ---- restatement, once per (lattice, pair) -------------------------------------------------------------------------------------
_BP = {}


def _key(lat):
    return id(lat["frame"])


def want_best_path(lat, gs, as_):
    """ops.best_path(lat, gs, as_), kept per (lattice object, pair bits): the sweeps share pairs and the lists repeat lattices"""
    k = (_key(lat), ops.bits(F(gs)), ops.bits(F(as_)))
    if k not in _BP:
        _BP[k] = (lat, ops.best_path(lat, F(gs), F(as_)))          # (the lattice is held: its id stays its own)
    return _BP[k][1]


_PR = {}


def want_prune(lat, beam, gs, as_):
    k = (_key(lat), float(beam), float(F(gs)), float(F(as_)))
    if k not in _PR:
        _PR[k] = (lat, ops.prune(lat, beam, F(gs), F(as_)))
    return _PR[k][1]


# ---- sweeps wider than a wave --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _grid130():
    """130 pairs: the acoustic scale runs over three decades (10^-1.5 .. 10^1.5) in an order that puts the whole range inside every
    64 consecutive pairs, the graph scale cycles through 1, 0.5, 2, 0.25; graph_scale = 0 and acoustic_scale = 0 appear in the first
    wave, in the second and in the tail"""
    k = np.arange(130)
    as_ = (10.0 ** (-1.5 + 3.0 * ((k * 37) % 64) / 63.0)).astype(F)
    gs = np.asarray([1.0, 0.5, 2.0, 0.25], F)[k % 4].copy()
    for j in (5, 70, 128):
        gs[j] = 0.0
    for j in (9, 100, 129):
        as_[j] = 0.0
    return gs, as_


def wide_sweeps():
    """{K: (graph_scales, acoustic_scales)} for K = 64, 65, 130.  K = 64 is the first wave of the 130-pair grid and K = 65 its pairs
    65 .. 129, so one restatement of the grid serves all three."""
    gs, as_ = _grid130()
    out = {64: (gs[:64].copy(), as_[:64].copy()), 65: (gs[65:].copy(), as_[65:].copy()), 130: (gs, as_)}
    for K, (g, a) in out.items():
        assert len(g) == len(a) == K and (g == 0).any() and (a == 0).any() and (g >= 0).all() and (a >= 0).all()
        pos = a[a > 0]
        assert pos.max() / pos.min() > 500.0, K                    # about three decades
    return out


def distinct_paths(lat, gs, as_, lo, hi):
    """distinct best paths (arc lists) of the restatement among pairs lo .. hi - 1"""
    return len({tuple(want_best_path(lat, gs[k], as_[k])["arcs"]) for k in range(lo, min(hi, len(gs)))})


def mixed_status_sweep(K=130):
    """(names, lattices, graph_scales, acoustic_scales, want[k][u] status): `negative_epsilon_cycle` succeeds where graph_scale = 0
    and is KHG_LAT_EPS_LOOP where graph_scale > 0, alternating lane by lane; `no_reachable_final` has no path under any pair; a lattice
    with a path sits between and after them."""
    c = hand_cases()
    names = ["negative_epsilon_cycle", "scales_change_the_winner_a", "no_reachable_final", "epsilon_chain"]
    lats = [c[n][0] for n in names]
    positive = [(1.0, 1.0), (0.5, 1.7), (1.0, 0.0), (1e-3, 1.0)]
    gs, as_ = np.zeros(K, F), np.ones(K, F)
    for k in range(K):
        if k % 2 == 1:
            gs[k], as_[k] = positive[(k // 2) % 4]
    want = [[want_best_path(lat, gs[k], as_[k])["status"] for lat in lats] for k in range(K)]
    for k in range(K):
        assert want[k][0] == (ops.EPS_LOOP if k % 2 else ops.SUCCEEDED), (k, want[k])
        assert want[k][2] == ops.NO_PATH and want[k][1] == want[k][3] == ops.SUCCEEDED, (k, want[k])
    for g, a in positive:
        assert ops.best_path(lats[0], g, a)["status"] == ops.EPS_LOOP
    assert ops.best_path(lats[0], 0.0, 1.0)["status"] == ops.SUCCEEDED
    return names, lats, gs, as_, want


# ---- more utterances than a tile of the scans ----------------------------------------------------------------------------------
EMPTY_AT = (0, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def many_utterances():
    """The 157 rule lattices in one list of 162, with empty lattices (start = -1) at positions 0, 63, 64, 65 and last."""
    rule = [lat for _, lat in _cases()]
    assert len(rule) == 157
    out, it = [], iter(rule)
    for i in range(len(rule) + len(EMPTY_AT) + 1):
        out.append(ops.empty_lattice() if i in EMPTY_AT or i == len(rule) + len(EMPTY_AT) else next(it))
    assert len(out) == 162 and all(len(out[i]["frame"]) == 0 and out[i]["start"] == -1 for i in EMPTY_AT + (161,))
    assert sum(len(x["frame"]) == 0 for x in out) == 5
    return out


UTT_CUTS = (64, 65, 129, 162)


@functools.lru_cache(maxsize=None)
def thousands_of_utterances(U=4160):
    """(distinct lattices, index list of length U >= 4100): the hand-built lattices, an empty one and the 12 smallest rule lattices,
    repeated in an order that is not periodic in 64; 4096 / U is 0, so k2_lattice_prune_fill's stripe count falls back to 1"""
    c = hand_cases()
    rule = sorted((lat for _, lat in _cases()), key=lambda x: len(x["frame"]))[:12]
    distinct = [c[n][0] for n in sorted(c)] + [ops.empty_lattice()] + rule
    idx = [(7 * i + (i // 61)) % len(distinct) for i in range(U)]
    assert U >= 4100 and 4096 // U == 0 and set(idx) == set(range(len(distinct)))
    return distinct, idx


# ---- tile edges inside an utterance --------------------------------------------------------------------------------------------
def _tile_lattice(N, W=5):
    """N states: the start alone on frame 0, then frames of W states (the last may be narrower), every state with an emitting arc to
    every state of the next frame and an epsilon arc to its right-hand neighbour.  An arc's graph cost is the penalty of the state
    it enters: 0 for one state per frame (the best path), 0.25 or 1 for the others by a pattern over the state index that changes at
    every multiple of 64; the epsilon arcs cost 2 and never help.  Every number is a small multiple of 1/8, so the sums are exact
    and at beam 0.5 under (1, 1) a state's fate is its penalty's -- which the builder does not rely on: tile_edge_lattices asserts
    what it needs from the restatement."""
    frame_of = [0] + [1 + (s - 1) // W for s in range(1, N)]
    T = frame_of[-1]
    pen = [0.25 if (s % 2 == 0) != (s % 7 == 3 and s % TILE not in (0, TILE - 1)) else 1.0 for s in range(N)]
    by_frame = {}
    for s, f in enumerate(frame_of):
        by_frame.setdefault(f, []).append(s)
    for f, ss in by_frame.items():
        best = [s for s in ss if pen[s] == 0.25]
        pen[best[0] if best else ss[0]] = 0.0
    states = [(f, 0.0 if f == T else np.inf) for f in frame_of]
    arcs = []
    for s, f in enumerate(frame_of):
        for d in by_frame.get(f + 1, []):
            arcs.append((s, 1 + (s + 3 * d) % 40, (d % 11 == 0) * (1 + d % 5), pen[d], ((f * 5) % 8) / 4.0, d))
        if s + 1 < N and frame_of[s + 1] == f:
            arcs.append((s, 0, (s % 13 == 0) * 7, 2.0, 0.0, s + 1))
    return _hand(states, arcs)


TILE_NS = (63, 64, 65, 127, 128, 129, 193, 5003)


def tile_counts(lat, kept_states):
    """[(kept, dropped)] per 64-state tile"""
    N = len(lat["frame"])
    keep = np.zeros(N, bool)
    keep[kept_states] = True
    return [(int(keep[t: t + TILE].sum()), int((~keep[t: t + TILE]).sum())) for t in range(0, N, TILE)]


@functools.lru_cache(maxsize=None)
def tile_edge_lattices():
    """[(lattice, beam, graph_scale, acoustic_scale)] for N = 63, 64, 65, 127, 128, 129, 193 and 5003 states: the restatement keeps
    some and drops some states in every 64-state tile (a last tile of one state can only do one: the edge condition covers it), and
    the two states either side of every tile edge have different fates"""
    out = []
    for N in TILE_NS:
        lat = _tile_lattice(N)
        assert len(lat["frame"]) == N
        beam, gs, as_ = 0.5, 1.0, 1.0
        pr, st = want_prune(lat, beam, gs, as_)
        assert st == ops.SUCCEEDED
        keep = set(pr["kept_states"])
        for kept, dropped in tile_counts(lat, pr["kept_states"]):
            assert (kept > 0 and dropped > 0) or kept + dropped == 1, (N, kept, dropped)       # (N = 65, 129, 193: a last tile of one state)
        for e in range(TILE, N, TILE):
            assert ((e - 1) in keep) != (e in keep), (N, e)
        assert 0 < len(pr["kept_arcs"]) < len(lat["ilabel"])
        out.append((lat, beam, gs, as_))
    assert max(len(x[0]["frame"]) for x in out) >= 5000
    return out


# ---- the LDS staging threshold -------------------------------------------------------------------------------------------------
def _wide_parts(rng, T, W, fan):
    states = [(f, np.inf if f < T else float(rng.uniform(0, 1))) for f in range(T + 1) for _ in range(W)]
    arcs = []
    for f in range(T + 1):
        for i in range(W):
            s = f * W + i
            if f < T:
                for j in rng.choice(W, fan, replace=False):
                    arcs.append((s, int(rng.integers(1, 50)), int(rng.integers(0, 3)), float(rng.uniform(0, 3)), float(rng.uniform(0, 9)), (f + 1) * W + int(j)))
            if i + 1 < W:
                arcs.append((s, 0, int(rng.integers(0, 2)) * 7, float(rng.uniform(0.1, 1)), 0.0, s + 1))
    return states, arcs


def _wide_lattice(rng, T, W, fan):
    """T + 1 frames of W states; every state has `fan` emitting arcs into the next frame and an epsilon arc to its right-hand
    neighbour (weights positive): far more arcs than the LDS-staged form takes"""
    return _hand(*_wide_parts(rng, T, W, fan))


def _padded(rng, T, W, fan, A):
    """a wide lattice padded to exactly A arcs with epsilon arcs s -> s + 2 inside a frame (weights positive)"""
    states, arcs = _wide_parts(rng, T, W, fan)
    s = 0
    while len(arcs) < A:
        if s + 2 < len(states) and states[s + 2][0] == states[s][0]:
            arcs.append((s, 0, 0, float(rng.uniform(0.1, 1)), 0.0, s + 2))
        s += 1
    lat = _hand(states, arcs)
    assert len(lat["ilabel"]) == A
    return lat


@functools.lru_cache(maxsize=None)
def lds_edge_lattices():
    """{"at": 4 * (3 N + 4 A) = 49152 exactly (staged), "over": 49156, the next size that exists (3 N + 4 A takes every integer, so
    one word more; not staged), "small": well below}"""
    rng = np.random.default_rng(4812)
    at = _padded(rng, 23, 16, 6, 3072 - 3 * 96)              # N = 384 = 4 * 96: 3 N + 4 A = 12288
    over = _padded(rng, 26, 13, 7, 3070 - 3 * 87)            # N = 351 = 4 * 87 + 3: 3 N + 4 A = 12289
    small = _wide_lattice(rng, 12, 5, 2)
    assert len(at["frame"]) == 384 and len(over["frame"]) == 351
    assert staged_bytes(at) == LDS_LIMIT == 49152 and staged_bytes(over) == LDS_LIMIT + 4 and staged_bytes(small) < LDS_LIMIT // 8
    for lat in (at, over, small):
        assert ops.best_path(lat)["status"] == ops.SUCCEEDED
    return {"at": at, "over": over, "small": small}


def all_constructed():
    """every lattice a builder here makes, named: for the host-side checks"""
    out = [("tile_N%d" % len(x[0]["frame"]), x[0]) for x in tile_edge_lattices()]
    out += [("lds_" + k, v) for k, v in lds_edge_lattices().items()]
    out += [("mixed_" + n, lat) for n, lat in zip(*mixed_status_sweep()[:2])]
    out += [("many_%d" % i, lat) for i, lat in enumerate(many_utterances())]
    return out
