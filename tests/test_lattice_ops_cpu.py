"""Best path under scales and beam pruning of raw lattices without a GPU: the host Lattice.shortest_path(gs, as)
/ best_path / prune against the plain-Python restatement of the rule (tests/lattice_ops_ref.py), bit for bit, on the rule lattices of
the 220 seeded cases of tests/test_lattice_simple_cpu.py; the properties of a pruned lattice; hand-built lattices; what
khg_lattices_upload refuses (through its host-only half, khg_lattices_validate); the C-ABI symbols."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_ops_ref as ops  # noqa: E402
import lattice_raw_ref as raw  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
from test_lattice_simple_cpu import _random_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = F(np.inf)
SCALES = [(1.0, 1.0), (0.5, 1.7), (1.0, 0.0), (0.0, 1.0)]
BEAMS = [0.0, 0.5, 2.0, float("inf")]


@functools.lru_cache(maxsize=None)
def _cases():
    """the rule lattices of the seeded cases that decode"""
    out = []
    for seed in range(220):
        g, m, cfg = _random_case(seed)
        lat = raw.rule_lattice(ref.Graph.from_dict(g), cfg, ref.matrix_ll(m), len(m))
        if lat is not None:
            out.append((seed, lat))
    return out


def _lattice(lat):
    import kaldi_hmm_gmm_amd as khg
    return khg.Lattice.from_arrays(*[lat[k] for k in ops.FIELDS], int(lat["start"]))


def _same_lattice(got, want, tag):
    for k in ops.FIELDS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (tag, k)
    assert got.start == want["start"], tag


def _same_path(got, want, tag):
    """Lattice.best_path's dict against the restatement's"""
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    assert got["ali"] == want["ali"] and got["words"] == want["words"], tag
    assert ops.bits(got["weight"]) == ops.bits(want["weight"]), (tag, got["weight"], want["weight"])


def test_cases_exist():
    assert len(_cases()) == 157


def test_shortest_path_under_scales_equals_the_restatement():
    n = 0
    for seed, lat in _cases():
        L = _lattice(lat)
        for gs, as_ in SCALES:
            want = ops.best_path(lat, gs, as_)
            got = L.best_path(gs, as_)
            _same_path(got, want, (seed, gs, as_))
            assert got["arcs"] == want["arcs"], (seed, gs, as_)
            lin = L.shortest_path(gs, as_)
            ok, ali, words, _ = lin.get_linear_symbol_sequence()
            assert ok and ali == want["ali"] and words == want["words"], (seed, gs, as_)
            assert len(want["ali"]) == int(lat["frame"][-1])          # a decoder lattice's path has T transition-ids
            n += 1
        # at (1, 1): today's shortest_path()
        a, b = L.shortest_path(), L.shortest_path(1.0, 1.0)
        assert [(x.ilabel, x.olabel, x.weight.value1, x.weight.value2, x.nextstate) for x in a.arcs] == \
               [(x.ilabel, x.olabel, x.weight.value1, x.weight.value2, x.nextstate) for x in b.arcs], seed
        assert (a.final.value1, a.final.value2) == (b.final.value1, b.final.value2)
        v = ops.best_path(lat, 1.0, 1.0)["weight"]
        assert raw.path_like(a) == float(F(-F(v[0] + v[1]))), seed
    assert n == 157 * 4


def test_some_scale_pair_changes_the_path():
    changed = 0
    for seed, lat in _cases():
        a, b = ops.best_path(lat, 1.0, 1.0), ops.best_path(lat, 0.5, 1.7)
        changed += a["arcs"] != b["arcs"]
    assert changed > 0, changed


def test_prune_equals_the_restatement():
    n = 0
    for seed, lat in _cases():
        L = _lattice(lat)
        for gs, as_ in SCALES[:2]:
            for beam in BEAMS:
                want, wst = ops.prune(lat, beam, gs, as_)
                got, st = L.prune_with_status(beam, gs, as_)
                assert st == wst == ops.SUCCEEDED, (seed, gs, as_, beam)
                _same_lattice(got, want, (seed, gs, as_, beam))
                _same_lattice(L.prune(beam, gs, as_), want, (seed, gs, as_, beam))
                n += 1
    assert n == 157 * 2 * 4


def _reach(lat):
    """(accessible, coaccessible) state sets by plain reachability"""
    N = len(lat["frame"])
    ab, nx = lat["arc_begin"], lat["nextstate"]
    acc, stack = set(), [int(lat["start"])] if N else []
    while stack:
        s = stack.pop()
        if s in acc:
            continue
        acc.add(s)
        stack.extend(int(nx[a]) for a in range(ab[s], ab[s + 1]))
    rev = [[] for _ in range(N)]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            rev[int(nx[a])].append(s)
    T = lat["frame"][-1] if N else 0
    co, stack = set(), [s for s in range(N) if lat["frame"][s] == T and lat["final_cost"][s] != INF]
    while stack:
        s = stack.pop()
        if s in co:
            continue
        co.add(s)
        stack.extend(rev[s])
    return acc, co


def _dict(L):
    d = {k: np.asarray(getattr(L, k)) for k in ops.FIELDS}
    d["start"] = L.start
    return d


def test_properties_of_the_pruned_lattice():
    lattices = not_trim_inputs = removed = 0
    kept_frac = {0.5: [], 2.0: []}
    for seed, lat in _cases():
        L = _lattice(lat)
        acc, co = _reach(lat)
        not_trim_inputs += len(acc & co) < len(lat["frame"])
        for gs, as_ in SCALES[:2]:
            want_path = ops.best_path(lat, gs, as_)
            prev_states = prev_arcs = None
            for beam in BEAMS:
                P = L.prune(beam, gs, as_)
                pd = _dict(P)
                lattices += 1
                # the pruned lattice's best path is the input's: labels and both sums, bit for bit
                _same_path(P.best_path(gs, as_), want_path, (seed, gs, as_, beam))
                # trim: every state is reachable from the start and reaches a final state
                pacc, pco = _reach(pd)
                assert len(pacc) == len(pco) == P.num_states > 0, (seed, gs, as_, beam)
                rp, _ = ops.prune(lat, beam, gs, as_)
                ks, ka = set(rp["kept_states"]), set(rp["kept_arcs"])
                if beam == float("inf"):
                    # the accessible and coaccessible sub-lattice
                    both = acc & co
                    assert ks == both, (seed, gs, as_)
                    src = ops._src_of(lat)
                    assert ka == {a for a in range(len(src)) if int(src[a]) in both and int(lat["nextstate"][a]) in both}, (seed, gs, as_)
                else:
                    kept_frac.setdefault(beam, []).append(len(ka) / max(1, len(lat["ilabel"])))
                # nested as the beam grows
                if prev_states is not None:
                    assert prev_states <= ks and prev_arcs <= ka, (seed, gs, as_, beam)
                prev_states, prev_arcs = ks, ka
                removed += P.num_states < len(lat["frame"]) or P.num_arcs_total < len(lat["ilabel"])
    print("lattices %d inputs with dead states %d pruned smaller %d; arcs kept at 0.5: %.2f at 2.0: %.2f" % (
        lattices, not_trim_inputs, removed, np.mean(kept_frac[0.5]), np.mean(kept_frac[2.0])))
    assert lattices == 157 * 2 * 4
    assert removed > 0 and not_trim_inputs > 0
    assert np.mean(kept_frac[0.5]) < np.mean(kept_frac[2.0]) < 1.0


def _hand(states, arcs, start=0):
    """states: [(frame, final_cost)], arcs: [(src, ilabel, olabel, graph, acoustic, dst)] -> the dict of arrays"""
    arcs = sorted(arcs, key=lambda a: a[0])          # stable: the order inside a state stays
    N = len(states)
    ab = np.zeros(N + 1, np.int32)
    for a in arcs:
        ab[a[0] + 1] += 1
    lat = {"frame": np.array([s[0] for s in states], np.int32), "graph_state": np.arange(N, dtype=np.int32),
           "tot_cost": np.zeros(N, np.float32), "extra_cost": np.zeros(N, np.float32),
           "final_cost": np.array([s[1] for s in states], np.float32), "arc_begin": np.cumsum(ab).astype(np.int32),
           "ilabel": np.array([a[1] for a in arcs], np.int32), "olabel": np.array([a[2] for a in arcs], np.int32),
           "graph_cost": np.array([a[3] for a in arcs], np.float32), "acoustic_cost": np.array([a[4] for a in arcs], np.float32),
           "nextstate": np.array([a[5] for a in arcs], np.int32), "start": start if N else -1}
    return lat


def hand_cases():
    """name -> (lattice, graph_scale, acoustic_scale, expected status, expected ali, expected words)"""
    inf = np.inf
    c = {}
    # two paths of exactly the same weight into the last state: the lower source state wins
    c["tie_by_source_order"] = (_hand([(0, inf), (1, inf), (1, inf), (2, 0.5)],
                                      [(0, 2, 0, 1.0, 1.0, 2), (0, 1, 0, 1.0, 1.0, 1), (1, 3, 11, 0.0, 1.0, 3), (2, 4, 12, 0.0, 1.0, 3)]),
                                1.0, 1.0, ops.SUCCEEDED, [1, 3], [11])
    # the same sum 3.0 two ways: (1, 2) against (2, 1): the smaller first component wins although its source is the higher state
    c["tie_on_the_sum_by_v1"] = (_hand([(0, inf), (1, inf), (1, inf), (2, 0.0)],
                                       [(0, 1, 0, 2.0, 1.0, 1), (0, 2, 0, 1.0, 2.0, 2), (1, 3, 11, 0.0, 0.0, 3), (2, 4, 12, 0.0, 0.0, 3)]),
                                 1.0, 1.0, ops.SUCCEEDED, [2, 4], [12])
    # an epsilon chain 0 -> 1 -> 2 -> 3 listed against its direction (one Jacobi round per hop), cheaper than the direct arc
    c["epsilon_chain"] = (_hand([(0, inf), (0, inf), (0, inf), (0, inf), (1, 0.25)],
                                [(2, 0, 9, 0.5, 0.0, 3), (1, 0, 8, 0.5, 0.0, 2), (0, 0, 7, 0.5, 0.0, 1), (0, 0, 6, 3.0, 0.0, 3), (3, 5, 0, 1.0, 2.0, 4)]),
                          1.0, 1.0, ops.SUCCEEDED, [5], [7, 8, 9])
    # a negative epsilon cycle 1 <-> 2
    c["negative_epsilon_cycle"] = (_hand([(0, inf), (0, inf), (0, inf), (1, 0.0)],
                                         [(0, 0, 0, 1.0, 0.0, 1), (1, 0, 0, -1.0, 0.0, 2), (2, 0, 0, 0.5, 0.0, 1), (2, 1, 0, 0.0, 1.0, 3)]),
                                   1.0, 1.0, ops.EPS_LOOP, [], [])
    # the only final state is not reachable
    c["no_reachable_final"] = (_hand([(0, inf), (1, inf), (1, 0.0)], [(0, 1, 0, 1.0, 1.0, 1)]), 1.0, 1.0, ops.NO_PATH, [], [])
    # graph-heavy against acoustic-heavy: the scale pair picks the winner
    lat = _hand([(0, inf), (1, inf), (1, inf), (2, 0.0)],
                [(0, 1, 21, 4.0, 1.0, 1), (0, 2, 22, 1.0, 3.0, 2), (1, 3, 0, 0.0, 0.5, 3), (2, 4, 0, 0.0, 0.5, 3)])
    c["scales_change_the_winner_a"] = (lat, 1.0, 1.0, ops.SUCCEEDED, [2, 4], [22])
    c["scales_change_the_winner_b"] = (lat, 0.1, 1.0, ops.SUCCEEDED, [1, 3], [21])
    return c


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_built_lattices(name):
    lat, gs, as_, status, ali, words = hand_cases()[name]
    want = ops.best_path(lat, gs, as_)
    assert (want["status"], want["ali"], want["words"]) == (status, ali, words)
    L = _lattice(lat)
    _same_path(L.best_path(gs, as_), want, name)
    for beam in BEAMS:
        wp, wst = ops.prune(lat, beam, gs, as_)
        got, st = L.prune_with_status(beam, gs, as_)
        assert st == wst == status, (name, beam)
        _same_lattice(got, wp, (name, beam))
        if status != ops.SUCCEEDED:
            assert got.num_states == 0 and got.num_arcs_total == 0 and got.start == -1 and list(got.arc_begin) == [0]
    if status == ops.EPS_LOOP:
        with pytest.raises(RuntimeError, match="epsilon cycle"):
            L.shortest_path(gs, as_)
    if name == "epsilon_chain":
        assert ops.bits(want["weight"]) == ops.bits((F(2.75), F(2.0)))
        assert L.prune(0.0).num_arcs_total == 4 and L.prune(2.0).num_arcs_total == 5       # the direct arc costs 1.5 more


def test_bad_arguments():
    lat, *_ = hand_cases()["epsilon_chain"]
    L = _lattice(lat)
    for bad in (-1.0, float("nan")):
        with pytest.raises(RuntimeError):
            L.best_path(bad, 1.0)
        with pytest.raises(RuntimeError):
            L.prune(1.0, 1.0, bad)
        with pytest.raises(RuntimeError):
            L.prune(bad)
    import kaldi_hmm_gmm_amd as khg
    empty = khg.Lattice.from_arrays([], [], [], [], [], [0], [], [], [], [], [], -1)
    assert empty.best_path()["status"] == ops.NO_PATH and empty.prune(1.0).num_states == 0


def test_upload_refusals():
    """What khg_lattices_upload checks before anything reaches the device (DeviceLattices.validate runs khg_lattices_validate)."""
    import kaldi_hmm_gmm_amd as khg
    good, *_ = hand_cases()["epsilon_chain"]
    khg.DeviceLattices.validate([_lattice(good), khg.Lattice.from_arrays([], [], [], [], [], [0], [], [], [], [], [], -1)])

    def broken(**kw):
        d = {k: np.array(v) for k, v in good.items() if k != "start"}
        d["start"] = kw.pop("start", good["start"])
        for k, (i, v) in kw.items():
            d[k][i] = v
        return [_lattice(good), _lattice(d)]

    # an emitting arc inside a frame, an epsilon arc across frames, an emitting arc over two frames, the start off frame 0
    for kw, what in ((dict(ilabel=(0, 5)), "utterance 1.*emitting arc"), (dict(ilabel=(4, 0)), "utterance 1.*epsilon arc"),
                     (dict(frame=(4, 2)), "utterance 1.*emitting arc"), (dict(start=4), "utterance 1.*start must be on frame 0")):
        with pytest.raises(RuntimeError, match=what):
            khg.DeviceLattices.validate(broken(**kw))
    # through the C-ABI: offsets that decrease, a nextstate out of range, an arc_begin that is not monotone
    from kaldi_hmm_gmm_amd import _lib
    import ctypes as C

    def call(lat, so=None, ao=None):
        N, A = len(lat["frame"]), len(lat["ilabel"])
        so = np.array([0, N] if so is None else so, np.int64)
        ao = np.array([0, A] if ao is None else ao, np.int64)
        arrs = [np.ascontiguousarray(lat[k][:N] if k == "arc_begin" else lat[k]) for k in ops.FIELDS]
        start = np.array([lat["start"]] * (len(so) - 1), np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        fn = _lib.lib.khg_lattices_validate
        fn.argtypes = [C.c_int32] + [C.c_void_p] * 14
        return fn(len(so) - 1, ptr(so), ptr(ao), *[ptr(a) for a in arrs], ptr(start))

    assert call(good) == 0
    assert call(good, so=[0, 5, 3], ao=[0, 5, 5]) != 0
    bad = dict(good, nextstate=good["nextstate"].copy())
    bad["nextstate"][0] = 9
    assert call(bad) != 0
    bad = dict(good, arc_begin=good["arc_begin"].copy())
    bad["arc_begin"][1] = 4
    assert call(bad) != 0


def test_cabi_symbols():
    names = ["khg_lattices_validate", "khg_lattices_upload", "khg_lattices_num_utts", "khg_lattices_ali_layout", "khg_lattices_best_path",
             "khg_lattices_prune"]
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    for n in names:
        assert re.search(r"\bint %s\(" % n, header), n
    assert "KHG_OPT_LAT_OPS_LDS" in header
    from kaldi_hmm_gmm_amd import _lib
    for n in names:
        assert n in _lib.SIGNATURES and getattr(_lib.lib, n) is not None, n
    so = os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r" T %s$" % n, out, re.M), n
    import kaldi_hmm_gmm_amd as khg
    assert khg.DeviceLattices is khg.align.DeviceLattices
    assert khg.get_raw_lattice_simple_device_batch is khg.align.get_raw_lattice_simple_device_batch
    for n in ("from_lattices", "validate", "best_path", "prune", "download", "close", "num_utts", "state_off", "arc_off", "device_bytes"):
        assert hasattr(khg.DeviceLattices, n), n
    assert hasattr(khg.UtteranceSet, "raw_lattices_simple_device")
