"""The inputs of tests/test_gpu_lattice_geometry.py reach the code they are meant for, shown without a GPU: every property the
builders of tests/lattice_geometry_cases.py promise is checked from the restatement (tests/lattice_ops_ref.py), the host
Lattice.best_path / prune_with_status agree with the restatement on the bits for every constructed lattice, and
DeviceLattices.validate (the host-only half of the upload) accepts them all."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_geometry_cases as gc  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
from test_lattice_ops_cpu import _cases, _lattice, _same_lattice, _same_path  # noqa: E402

F = np.float32
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _paths_per_wave():
    """per rule lattice: distinct restated best paths among pairs 0..63, 64..127 and 128..129 of the 130-pair grid (once per module:
    157 lattices x 130 pairs of plain Python)"""
    gs, as_ = gc.wide_sweeps()[130]
    return [(gc.distinct_paths(lat, gs, as_, 0, 64), gc.distinct_paths(lat, gs, as_, 64, 128), gc.distinct_paths(lat, gs, as_, 128, 130))
            for _, lat in _cases()]


def test_wide_sweeps_make_lanes_of_one_wave_disagree():
    sw = gc.wide_sweeps()
    assert sorted(sw) == [64, 65, 130]
    gs, as_ = sw[130]
    assert sw[64][0].tobytes() == gs[:64].tobytes() and sw[65][1].tobytes() == as_[65:].tobytes()
    for lo, hi in ((0, 64), (64, 128), (128, 130)):                   # both zeros inside each wave of the K = 130 launch
        assert (gs[lo:hi] == 0).any() and (as_[lo:hi] == 0).any(), (lo, hi)
    pw = _paths_per_wave()
    first = sum(a > 1 for a, _, _ in pw)
    second = sum(b > 1 for _, b, _ in pw)
    print("lattices %d; more than one path within pairs 0..63: %d, within 64..127: %d; most paths in one wave: %d" % (
        len(pw), first, second, max(max(a, b) for a, b, _ in pw)))
    assert len(pw) == 157 and 2 * first >= 157 and 2 * second >= 157


def test_wide_sweeps_host_equals_the_restatement():
    """the host best path under every pair of the grid, on a sample of the rule lattices (all of them at the zero scales)"""
    gs, as_ = gc.wide_sweeps()[130]
    zero = [k for k in range(130) if gs[k] == 0 or as_[k] == 0]
    n = 0
    for i, (seed, lat) in enumerate(_cases()):
        L = _lattice(lat)
        for k in (range(130) if i % 16 == 0 else zero):
            _same_path(L.best_path(float(gs[k]), float(as_[k])), gc.want_best_path(lat, gs[k], as_[k]), (seed, k))
            n += 1
    assert n >= 10 * 130


def test_mixed_status_sweep():
    names, lats, gs, as_, want = gc.mixed_status_sweep()
    assert len(gs) == 130 and (gs[0::2] == 0).all() and (gs[1::2] > 0).all()
    per_wave = [{want[k][0] for k in range(lo, hi)} for lo, hi in ((0, 64), (64, 128), (128, 130))]
    assert all(s == {ops.SUCCEEDED, ops.EPS_LOOP} for s in per_wave), per_wave
    for lat in lats:
        L = _lattice(lat)
        for k in range(130):
            _same_path(L.best_path(float(gs[k]), float(as_[k])), gc.want_best_path(lat, gs[k], as_[k]), k)


def test_many_utterances():
    lats = gc.many_utterances()
    assert [i for i, x in enumerate(lats) if len(x["frame"]) == 0] == [0, 63, 64, 65, 161]
    assert gc.UTT_CUTS == (64, 65, 129, 162)
    # at beam 0.5 and (1, 1) every rule lattice prunes to strictly between 0 and N states: the scans add up non-trivial counts
    for i, lat in enumerate(lats):
        pr, st = gc.want_prune(lat, 0.5, 1.0, 1.0)
        if len(lat["frame"]) == 0:
            assert st == ops.NO_PATH and len(pr["frame"]) == 0
        else:
            assert st == ops.SUCCEEDED and 0 < len(pr["frame"]) < len(lat["frame"]), i
    distinct, idx = gc.thousands_of_utterances()
    assert len(idx) >= 4100 and 4096 // len(idx) == 0
    assert len({tuple(idx[i: i + 64]) for i in range(0, len(idx) - 64, 64)}) > 60       # the tiles of the scans differ
    st = {ops.best_path(x)["status"] for x in distinct}
    assert st == {ops.SUCCEEDED, ops.NO_PATH, ops.EPS_LOOP}


def test_tile_edge_lattices():
    got = gc.tile_edge_lattices()
    assert tuple(len(x[0]["frame"]) for x in got) == gc.TILE_NS == (63, 64, 65, 127, 128, 129, 193, 5003)
    for lat, beam, gs, as_ in got:
        N = len(lat["frame"])
        pr, st = gc.want_prune(lat, beam, gs, as_)
        tc = gc.tile_counts(lat, pr["kept_states"])
        keep = set(pr["kept_states"])
        assert len(tc) == (N + 63) // 64
        assert all((k > 0 and d > 0) or k + d == 1 for k, d in tc), (N, tc)
        assert all(((e - 1) in keep) != (e in keep) for e in range(64, N, 64)), N
        print("N %d: tiles %d, stripes of the fill alone in a handle %d, kept / dropped in the first tiles %s, arcs %d -> %d" % (
            N, len(tc), min((N + 63) // 64, 4096), tc[:3], len(lat["ilabel"]), len(pr["kept_arcs"])))
    assert (5003 + 63) // 64 == 79


def test_lds_edge_lattices():
    L = gc.lds_edge_lattices()
    assert gc.staged_bytes(L["at"]) == 49152 and gc.staged_bytes(L["over"]) == 49156 and gc.staged_bytes(L["small"]) < 6144
    # no size lies between: 3 N + 4 A moves in steps of one word
    assert gc.staged_bytes(L["over"]) - gc.staged_bytes(L["at"]) == 4
    for lat in L.values():
        assert (np.asarray(lat["ilabel"]) == 0).any()


@pytest.mark.parametrize("which", ["tile", "lds", "mixed", "many"])
def test_host_equals_the_restatement_on_every_constructed_lattice(which):
    import kaldi_hmm_gmm_amd as khg
    todo = [(n, lat) for n, lat in gc.all_constructed() if n.startswith(which)]
    assert todo
    pairs = [(1.0, 1.0), (0.5, 1.7)]
    for name, lat in todo:
        L = _lattice(lat)
        big = len(lat["frame"]) > 1000
        for gs, as_ in pairs[:1] if big else pairs:
            _same_path(L.best_path(gs, as_), gc.want_best_path(lat, gs, as_), (name, gs, as_))
            for beam in (0.5,) if big else (0.0, 0.5, INF):
                want, wst = gc.want_prune(lat, beam, gs, as_)
                got, st = L.prune_with_status(beam, gs, as_)
                assert st == wst, (name, beam, gs, as_)
                _same_lattice(got, want, (name, beam, gs, as_))
    khg.DeviceLattices.validate([_lattice(lat) for _, lat in todo])


def test_validate_accepts_the_lists():
    import kaldi_hmm_gmm_amd as khg
    lats = [_lattice(x) for x in gc.many_utterances()]
    for n in gc.UTT_CUTS:
        khg.DeviceLattices.validate(lats[:n])
    distinct, idx = gc.thousands_of_utterances()
    host = [_lattice(x) for x in distinct]
    khg.DeviceLattices.validate([host[i] for i in idx])
    L = gc.lds_edge_lattices()
    khg.DeviceLattices.validate([_lattice(L["over"])])
    khg.DeviceLattices.validate([_lattice(L["at"]), _lattice(ops.empty_lattice()), _lattice(L["over"]), _lattice(L["small"])])


def test_num_chunks_entry_points():
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ["khg_lattices_num_chunks", "khg_lattices_chunk_utts"]
    with open(os.path.join(root, "include", "khg_hip.h")) as fh:
        header = fh.read()
    from kaldi_hmm_gmm_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(root, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    for n in names:
        assert re.search(r"\bint %s\(" % n, header) and n in _lib.SIGNATURES and re.search(r" T %s$" % n, out, re.M), n
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.DeviceLattices, "num_chunks") and hasattr(khg.DeviceLattices, "chunk_off")
