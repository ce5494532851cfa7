"""lattice-to-nbest on the host (Lattice.nbest; the rule is written out at khg_lattices_nbest in include/khg_hip.h):
the host form against the plain restatement of tests/lattice_nbest_ref.py on every array and status; against brute force over every
path (the sorted totals are exactly the n least totals over all paths, with ==); entry 0 against Lattice.best_path where rounding cannot
decide between the two cheapest paths; and on determinized inputs the n best distinct word sequences.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_nbest_cases as cases  # noqa: E402
import lattice_nbest_ref as ref  # noqa: E402

F = np.float32


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


@pytest.fixture(scope="module")
def work():
    import kaldi_hmm_gmm_amd as khg
    return khg, [(name, lat, _lattice(khg, lat), expect) for name, lat, expect in cases.all_cases()]


@pytest.fixture(scope="module")
def brute(work):
    """per (case, pair): every path with its values, or None when the lattice has more than 10 000 paths or is refused"""
    _, items = work
    out = {}
    for name, lat, _, _ in items:
        paths = ref.all_paths(lat)
        for pair in cases.PAIRS:
            out[(name, pair)] = None if paths is None else {p: ref.path_values(lat, p, *pair) for p in paths}
    return out


def _same(got, want):
    return (list(got[0]) == want[0] and list(got[1]) == want[1] and ref.bits(got[2]) == ref.bits(want[2]) and ref.bits(got[3]) == ref.bits(want[3]))


def test_host_form_equals_the_restatement(work):
    _, items = work
    seen = {}
    for name, lat, L, expect in items:
        for gs, as_ in cases.PAIRS:
            for n in cases.NS:
                got, st, _ = L.nbest_with_status(n, gs, as_)
                wst, want = ref.nbest(lat, n, gs, as_)
                assert st == wst and len(got) == len(want), (name, gs, as_, n)
                assert all(_same(g, w) for g, w in zip(got, want)), (name, gs, as_, n)
                assert [tuple(x) for x in L.nbest(n, gs, as_)] == [tuple(x) for x in got], name
                if expect is not None and (gs, as_) == (1.0, 1.0):
                    assert st == expect, name
                seen[st] = seen.get(st, 0) + 1
    assert seen[ref.SUCCEEDED] > 100 * 32 and seen[ref.EPS_LOOP] == 2 * 32 and seen[ref.NO_PATH] >= 3 * 32, seen


def test_hand_cases_say_what_they_are_for(work):
    _, items = work
    by = {name: L for name, _, L, _ in items}
    e = by["tie_in_arcs"].nbest(2)
    assert e[0][3] == e[1][3] and e[0][0] == [1, 3] and e[1][0] == [2, 4]          # the lower arc first
    e = by["tie_ranks"].nbest(2)
    assert e[0][3] == e[1][3] and e[0][0] == [1, 3] and e[1][0] == [2, 3]          # the lower rank first
    assert len(by["inf_arc_into_final"].nbest(5)) == 1 and len(by["nan_cost"].nbest(5)) == 1
    assert len(by["two_finals_and_an_early_one"].nbest(10)) == 4
    assert by["word_on_ilabel_0"].nbest(1, 1.0, 1.0)[0][0] == [3]
    assert len(by["sausage7x3"].nbest(1024)) == 1024 and len(by["sausage7x3_all_equal"].nbest(1024, 0.0, 0.0)) == 1024
    assert len(by["fan70_into_one_state"].nbest(130)) == 70
    assert len(by["dead_end_unreachable"].nbest(5)) == 1 and len(by["one_state"].nbest(3)) == 1
    with pytest.raises(Exception, match="n must lie in 1 .. 1024"):
        by["diamond"].nbest(0)
    with pytest.raises(Exception, match="n must lie in 1 .. 1024"):
        by["diamond"].nbest(1025)
    with pytest.raises(Exception, match="finite and >= 0"):
        by["diamond"].nbest(1, -1.0, 1.0)


def test_brute_force_over_every_path(work, brute):
    _, items = work
    checked = 0
    for name, lat, L, _ in items:
        for pair in cases.PAIRS:
            vals = brute[(name, pair)]
            if vals is None:
                continue
            live = {p: v for p, v in vals.items() if v[0] < ref.INF}
            totals = sorted(v[0] for v in live.values())
            for n in cases.NS:
                got, st, paths = L.nbest_with_status(n, *pair)
                assert len(got) == min(n, len(live)), (name, pair, n)
                assert (st == ref.SUCCEEDED) == (len(live) > 0), (name, pair, n)
                mine = [F(g[3]) for g in got]
                assert mine == sorted(mine) and all(a == b for a, b in zip(mine, totals[:n])), (name, pair, n)
                assert len(set(paths)) == len(paths), (name, pair, n)
                for g, p in zip(got, paths):
                    assert p in live, (name, pair, n, p)
                    v = live[p]
                    assert _same(g, (v[2], v[3], v[1], v[0])), (name, pair, n, p)
                checked += 1
    assert checked > 200 * 4 * 8, checked


def test_entry_0_is_best_path_where_rounding_cannot_decide(work, brute):
    """equal in alignment, words and weight bits on every case whose float64 gap between the two cheapest paths exceeds
    (L + 1) * 2^-22 * M: L the arcs of the longest path, M the largest absolute partial sum -- the accumulated rounding of both orders"""
    _, items = work
    total = qualify = 0
    for name, lat, L, _ in items:
        for pair in cases.PAIRS:
            vals = brute[(name, pair)]
            if vals is None:
                continue
            ok = ref.gap_exceeds_rounding(vals)
            if ok is None:
                continue
            total += 1
            if not ok:
                continue
            qualify += 1
            bp = L.best_path(*pair)
            e = L.nbest(1, *pair)[0]
            assert bp["status"] == ref.SUCCEEDED, (name, pair)
            assert [x for x in e[1] if x != 0] == list(bp["ali"]) and list(e[0]) == list(bp["words"]), (name, pair)
            assert ref.bits(e[2]) == ref.bits(bp["weight"]), (name, pair)
    print("entry 0 against best_path: %d of %d (case, pair) qualify" % (qualify, total))
    assert 2 * qualify >= total, (qualify, total)


def test_determinized_inputs_give_distinct_word_sequences(work):
    """after determinize every word sequence has one path: nbest gives pairwise distinct word sequences, the n cheapest of the brute-force
    per-sequence minima"""
    _, items = work
    done = 0
    for name, lat, L, _ in items:
        for pair in ((1.0, 1.0), (0.5, 1.7)):
            D, st, _ = L.determinize(pair[0], pair[1], 1.0e6, 1.0 / 1024, 8)
            if st != ref.SUCCEEDED:
                continue
            dlat = {k: np.asarray(getattr(D, k)) for k in ref.FIELDS}
            dlat["start"] = D.start
            paths = ref.all_paths(dlat)
            if paths is None:
                continue
            best = {}
            for p in paths:
                v = ref.path_values(dlat, p, *pair)
                if v[0] < ref.INF:
                    w = tuple(v[2])
                    best[w] = min(best.get(w, ref.INF), v[0])
            minima = sorted(best.values())
            for n in (1, 5, 64):
                got = D.nbest(n, *pair)
                seqs = [tuple(g[0]) for g in got]
                assert len(set(seqs)) == len(seqs) == min(n, len(best)), (name, pair, n)
                assert all(F(g[3]) == t for g, t in zip(got, minima[:n])), (name, pair, n)
                assert all(F(g[3]) == best[s] for g, s in zip(got, seqs)), (name, pair, n)
            done += 1
    assert done > 200, done


def test_the_arena_option_is_exported_bound_and_in_the_environment_table():
    """KHG_OPT_NBEST_ARENA (the lists of one launch, in KiB; 0: 1 GiB) and the clause of KHG_OPT_LAT_OPS_LDS that names khg_lattices_nbest"""
    import ctypes as C
    import re

    from kaldi_hmm_gmm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "khg_hip.h")).read()
    opt = int(re.search(r"#define KHG_OPT_NBEST_ARENA (\d+)", h).group(1))
    assert opt < int(re.search(r"#define KHG_OPT_COUNT (\d+)", h).group(1)) and "[KHG_NBEST_ARENA]" in h
    assert "khg_lattices_nbest" in h[h.index("#define KHG_OPT_LAT_OPS_LDS"):h.index("#define KHG_OPT_K1_LAUNCH")]
    with open(os.path.join(root, "kaldi_hmm_gmm_amd", "csrc", "khg_pybind.cpp")) as fh:
        names = re.findall(r'"(\w+)"', re.search(r"names\[KHG_OPT_COUNT\] = \{(.*?)\};", fh.read(), re.S).group(1))
    assert names[opt] == "nbest_arena"
    o, v = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.khg_option_from_env(b"KHG_NBEST_ARENA", b"64", C.byref(o), C.byref(v)) == 0 and (o.value, v.value) == (opt, 64)
    assert _lib.lib.khg_option_check(opt, 0) == 0 and _lib.lib.khg_option_check(opt, 1 << 20) == 0
    assert _lib.lib.khg_option_check(opt, -1) != 0 and _lib.lib.khg_option_check(opt, (1 << 20) + 1) != 0
