"""Inputs for the MPE / sMBR posteriors, shared by tests/test_lattice_mpe_cpu.py (the host Lattice) and
tests/test_gpu_lattice_mpe.py (the device): the lattices of tests/lattice_post_cases.py and of the lattice-faster rule cases, each
with tables (transition-id -> phone, -> pdf), a silence set and a reference alignment -- for the even-numbered lattices the labels of
a seeded random complete path of the lattice (not the best path), for the odd ones random ids.  Plain Python and numpy."""
import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_mpe_ref as mr  # noqa: E402
import lattice_post_cases as pc  # noqa: E402
import lattice_post_ref as pr  # noqa: E402
from lattice_geometry_cases import _padded, lds_edge_lattices, tile_edge_lattices  # noqa: E402

SCALES = pc.SCALES
VARIANTS = [("smbr", True), ("smbr", False), ("mpfe", True), ("mpfe", False)]
SILENCE = (1,)
MPE_LDS_LIMIT = 48 * 1024       # kLatOpsLds: 40 N + 4 (3 N + 4 A) bytes are staged up to this


def mpe_staged_bytes(lat):
    N, A = len(lat["frame"]), len(lat["ilabel"])
    return 40 * N + 4 * (3 * N + 4 * A)


def tables(num_tids):
    """three ids per phone, two per pdf (so the two criteria differ); phone 1 is the silence phone.  Entry 0 is unused."""
    t = np.arange(num_tids + 1)
    tid2phone = np.where(t > 0, 1 + (t - 1) // 3, 0).astype(np.int32)
    tid2pdf = np.where(t > 0, (t - 1) // 2, 0).astype(np.int32)
    return tid2phone, tid2pdf


def num_tids_of(lat):
    return max(4, int(lat["ilabel"].max()) if len(lat["ilabel"]) else 4)


def random_path_labels(lat, seed):
    """the non-zero ilabels of a random complete path: from the start, a uniformly drawn arc among those whose target still reaches a
    final state of the last frame, until a final state is drawn as the end"""
    w = pc.want(lat, 1.0, 1.0)
    assert w["status"] == pr.SUCCEEDED
    rng = np.random.default_rng(seed)
    ab, T = lat["arc_begin"], int(lat["frame"][-1])
    s, out = int(lat["start"]), []
    while True:
        arcs = [a for a in range(int(ab[s]), int(ab[s + 1])) if w["beta"][int(lat["nextstate"][a])] != pr.NINF]
        final = int(lat["frame"][s]) == T and lat["final_cost"][s] != np.inf
        if final and (not arcs or rng.integers(2) == 0):
            break
        a = arcs[int(rng.integers(len(arcs)))]
        if lat["ilabel"][a] != 0:
            out.append(int(lat["ilabel"][a]))
        s = int(lat["nextstate"][a])
    assert len(out) == T
    return np.asarray(out, np.int32)


def reference(name, index, lat):
    """(tid2phone, tid2pdf, alignment) of the lattice `name`, number `index` of its group: even -> a random path, odd -> random ids"""
    nt = num_tids_of(lat)
    tid2phone, tid2pdf = tables(nt)
    seed = zlib.crc32(str(name).encode()) & 0xFFFF
    T = int(lat["frame"][-1])
    if index % 2 == 0:
        ali = random_path_labels(lat, seed)
    else:
        ali = np.random.default_rng(seed).integers(1, nt + 1, T).astype(np.int32)
    return tid2phone, tid2pdf, ali


_WANT = {}


def want(lat, ref, criterion, one_sil, gs, as_):
    """mr.forward_backward_mpe, kept per (lattice object, alignment, variant, pair)"""
    tid2phone, tid2pdf, ali = ref
    k = (id(lat["frame"]), len(tid2phone), np.asarray(ali, np.int32).tobytes(), criterion, one_sil, float(np.float32(gs)), float(np.float32(as_)))
    if k not in _WANT:
        _WANT[k] = (lat, mr.forward_backward_mpe(lat, tid2phone, tid2pdf, SILENCE, ali, criterion, one_sil, gs, as_))
    return _WANT[k][1]


@functools.lru_cache(maxsize=None)
def constructed():
    """[(name, lattice, reference)]: the tile-edge and LDS-edge lattices, the geometry of lattice_post_cases and its hand-built ones"""
    out = [("tile_N%d" % len(x[0]["frame"]), x[0]) for x in tile_edge_lattices()]
    out += [("lds_" + k, v) for k, v in lds_edge_lattices().items()]
    out += [("post_lds_" + k, v) for k, v in pc.post_lds_edge().items()]
    out += [("mpe_lds_" + k, v) for k, v in mpe_lds_edge().items() if k != "post_only"]
    out += sorted(pc.geometry().items()) + sorted(pc.hand_built().items())
    out += [("dead_states", pc.dead_states()[0])]
    return [(n, lat, reference(n, i, lat)) for i, (n, lat) in enumerate(out)]


@functools.lru_cache(maxsize=None)
def faster_rule():
    """[(name, lattice, reference)] of the 120 lattice-faster rule lattices"""
    from test_lattice_faster_raw_cpu import _cases
    return [("faster_%s" % (seed,), lat, reference("faster_%s" % (seed,), i, lat)) for i, (seed, lat, _) in enumerate(_cases())]


@functools.lru_cache(maxsize=None)
def mpe_lds_edge():
    """{"at": 40 N + 4 (3 N + 4 A) = 49152 exactly (k2_lattice_post_mpe stages it), "over": 49156, the next size that exists (not
    staged), "post_only": a lattice that k2_lattice_post_fb stages (24 N + ... = 49152) and k2_lattice_post_mpe does not (55296)}"""
    rng = np.random.default_rng(4814)
    at = _padded(rng, 19, 16, 5, 2032)                # N = 320: 13 N + 4 A = 4160 + 8128 = 12288
    over = _padded(rng, 24, 13, 5, 2016)              # N = 325: 13 N + 4 A = 4225 + 8064 = 12289
    post_only = pc.post_lds_edge()["at"]
    assert mpe_staged_bytes(at) == MPE_LDS_LIMIT and mpe_staged_bytes(over) == MPE_LDS_LIMIT + 4
    assert pc.post_staged_bytes(post_only) <= pc.POST_LDS_LIMIT < mpe_staged_bytes(post_only)
    assert pr.admissible(at) and pr.admissible(over)
    return {"at": at, "over": over, "post_only": post_only}


def one_path_reference(T=7):
    """pc.one_path(T) with a reference that matches its labels on every frame but frames 2 and 5 (a non-silence phone apart)"""
    lat = pc.one_path(T)
    labels = [int(x) for x in lat["ilabel"] if x != 0]
    tid2phone, tid2pdf = tables(max(labels) + 6)
    ali = np.asarray(labels, np.int32)
    ali[[2, 5]] += 6
    return lat, (tid2phone, tid2pdf, ali)
