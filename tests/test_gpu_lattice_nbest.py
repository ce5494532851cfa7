"""lattice-to-nbest on the device (khg_lattices_nbest through DeviceLattices.nbest) against the host form
(Lattice.nbest, which tests/test_lattice_nbest_cpu.py holds to the plain restatement and to brute force), bit for bit: statuses, counts,
alignments, words, weight pairs and totals, on the hand-made cases and the 200 seeded random lattices of tests/lattice_nbest_cases.py,
as one batch per (scale pair, n), one utterance at a time, twice; refused lattices at the edges of a wave's worth of utterances; a
handle of 130 utterances; lattices the lattice-faster decoder leaves on the device, determinized; nbest(1) against best_path; the
running lists in HBM rows instead of LDS (KHG_OPT_LAT_OPS_LDS = 1); one chunk in many launches (KHG_OPT_NBEST_ARENA = 1).  Alone, every
case runs at two of the 32 (n, pair) combinations.  A handle of more than one chunk is not covered: no test here can make one.
KHG_LAT_SCRATCH needs list bounds above 2^31 - 1 and is not covered either."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_nbest_cases as cases  # noqa: E402
import lattice_nbest_ref as ref  # noqa: E402
from test_gpu_lattice_det import _decoded  # noqa: E402
from test_gpu_lattice_faster_raw import setup  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


@pytest.fixture(scope="module")
def work():
    """every case as a Lattice, and the host form's answers, computed once per (case, pair, n) on demand"""
    import kaldi_hmm_gmm_amd as khg
    items = [{"name": name, "lat": lat, "L": _lattice(khg, lat)} for name, lat, _ in cases.all_cases()]
    memo = {}

    def host(i, n, pair):
        key = (i, n, pair)
        if key not in memo:
            got, st, _ = items[i]["L"].nbest_with_status(n, *pair)
            memo[key] = (st, got)
        return memo[key]
    return khg, items, host


def _check(nl, u, want, tag):
    """utterance u of the NbestList against the host's (status, entries)"""
    st, entries = want
    assert int(nl.status[u]) == st, (tag, int(nl.status[u]), st)
    assert nl.count(u) == len(entries), (tag, nl.count(u), len(entries))
    for k, (words, ali, weight, total) in enumerate(entries):
        assert nl.words(u, k).tolist() == list(words) and nl.alignment(u, k).tolist() == list(ali), (tag, k)
        assert nl.weights(u)[k].tobytes() == ref.bits(weight) and nl.totals(u)[k].tobytes() == ref.bits(total), (tag, k)


def _run(khg, dl, n, pair):
    nb = dl.nbest(n, *pair)
    assert nb.num_utts == dl.num_utts and nb.device_bytes >= 0
    arrays = nb.download()
    assert nb.counts.tolist() == np.diff(arrays["entry_off"]).tolist() and nb.status.tolist() == arrays["status"].tolist()
    nb.close()
    return arrays


def test_device_equals_the_host_form_batched_and_twice(work):
    khg, items, host = work
    dl = khg.DeviceLattices.from_lattices([x["L"] for x in items])
    seen = {}
    for pair in cases.PAIRS:
        for n in cases.NS:
            a = _run(khg, dl, n, pair)
            nl = khg.NbestList(a)
            for u, x in enumerate(items):
                _check(nl, u, host(u, n, pair), (x["name"], pair, n))
                seen[int(nl.status[u])] = seen.get(int(nl.status[u]), 0) + 1
            b = _run(khg, dl, n, pair)       # the same bits over two runs
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (k, pair, n)
    dl.close()
    assert seen[ref.SUCCEEDED] > 100 * 32 and seen[ref.EPS_LOOP] == 2 * 32 and seen[ref.NO_PATH] >= 3 * 32, seen


def test_device_one_utterance_at_a_time_twice(work):
    """independent of the batch: EVERY case as a handle of one, at two (n, pair) combinations, each twice (the other combinations run
    in the batches; the utterances of a launch share nothing, so what a batch can change is the indexing, which does not depend on n)"""
    khg, items, host = work
    alone = list(range(len(items)))
    for i in alone:
        dl = khg.DeviceLattices.from_lattices([items[i]["L"]])
        for n, pair in ((5, (1.0, 1.0)), (1024, (0.5, 1.7))):
            for rep in range(2):
                _check(khg.NbestList(_run(khg, dl, n, pair)), 0, host(i, n, pair), (items[i]["name"], "alone", n, rep))
        dl.close()
    assert len(alone) == len(items) >= 220


def test_refused_lattices_at_the_edges_of_a_handle_of_130(work):
    """the empty and the refused lattices at positions 0, 63, 64 and last of 130 utterances"""
    khg, items, host = work
    by = {x["name"]: i for i, x in enumerate(items)}
    order = [i for i, x in enumerate(items) if x["name"] not in ("empty", "self_loop", "arc_to_lower_state", "no_final")][:130]
    order[0], order[63], order[64], order[129] = by["empty"], by["self_loop"], by["arc_to_lower_state"], by["no_final"]
    dl = khg.DeviceLattices.from_lattices([items[i]["L"] for i in order])
    assert dl.num_utts == 130
    for n, pair in ((1, (1.0, 1.0)), (65, (1.0, 0.1)), (1024, (0.0, 0.0))):
        nl = khg.NbestList(_run(khg, dl, n, pair))
        for u, i in enumerate(order):
            _check(nl, u, host(i, n, pair), (items[i]["name"], u, n))
        assert [int(nl.status[u]) for u in (0, 63, 64, 129)] == [ref.NO_PATH, ref.EPS_LOOP, ref.EPS_LOOP, ref.NO_PATH]
        assert [nl.count(u) for u in (0, 63, 64, 129)] == [0, 0, 0, 0] and nl.counts.sum() > (130 if n > 1 else 60)
    dl.close()


def test_running_lists_in_hbm_rows(work):
    """KHG_OPT_LAT_OPS_LDS = 1 keeps the running lists in HBM rows instead of LDS: the same bits, and the host's"""
    khg, items, host = work
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    dl = khg.DeviceLattices.from_lattices([x["L"] for x in items])
    default = ctx.get_option("lat_ops_lds")
    assert default == 0
    try:
        for n, pair in ((5, (1.0, 1.0)), (1024, (0.5, 1.7))):
            ctx.set_option("lat_ops_lds", 0)
            a = _run(khg, dl, n, pair)
            ctx.set_option("lat_ops_lds", 1)
            b = _run(khg, dl, n, pair)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (k, n, pair)
            nl = khg.NbestList(b)
            for u, x in enumerate(items):
                _check(nl, u, host(u, n, pair), (x["name"], "hbm rows", n))
    finally:
        ctx.set_option("lat_ops_lds", default)
    dl.close()


def test_a_chunk_in_many_launches(work):
    """option nbest_arena = 1 (KiB: 42 list elements) splits the one chunk into many launches -- an utterance above the budget is a
    launch of its own --, each with its own arena and output block: the same bits as one launch, and the host's"""
    khg, items, host = work
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    dl = khg.DeviceLattices.from_lattices([x["L"] for x in items])
    default = ctx.get_option("nbest_arena")
    assert default == 0
    try:
        for n, pair in ((5, (1.0, 1.0)), (65, (0.5, 1.7))):
            ctx.set_option("nbest_arena", 0)
            a = _run(khg, dl, n, pair)
            ctx.set_option("nbest_arena", 1)
            b = _run(khg, dl, n, pair)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (k, n, pair)
            nl = khg.NbestList(b)
            for u, x in enumerate(items):
                _check(nl, u, host(u, n, pair), (x["name"], "many launches", n))
        with pytest.raises(RuntimeError):
            ctx.set_option("nbest_arena", -1)
    finally:
        ctx.set_option("nbest_arena", default)
    dl.close()


def test_nbest_1_against_best_path(work):
    """entry 0 is best_path's path, with its weight pair bit for bit, wherever rounding cannot decide between the two cheapest paths
    (the condition of the CPU test)"""
    khg, items, host = work
    dl = khg.DeviceLattices.from_lattices([x["L"] for x in items])
    U = len(items)
    paths = [ref.all_paths(x["lat"]) for x in items]
    bp = dl.best_path(np.array([p[0] for p in cases.PAIRS], F), np.array([p[1] for p in cases.PAIRS], F))
    held = 0
    for k, pair in enumerate(cases.PAIRS):
        nl = khg.NbestList(_run(khg, dl, 1, pair))
        for u, x in enumerate(items):
            if paths[u] is None:
                continue
            if not ref.gap_exceeds_rounding({p: ref.path_values(x["lat"], p, *pair) for p in paths[u]}):
                continue
            e = k * U + u
            assert int(bp["status"][e]) == ref.SUCCEEDED and int(nl.status[u]) == ref.SUCCEEDED, (x["name"], pair)
            assert nl.alignment(u, 0).tolist() == bp["ali"][k, bp["ali_off"][u]: bp["ali_off"][u + 1]].tolist(), (x["name"], pair)
            assert nl.words(u, 0).tolist() == bp["words"][bp["words_off"][e]: bp["words_off"][e + 1]].tolist(), (x["name"], pair)
            assert nl.weights(u)[0].tobytes() == bp["weight"][e].tobytes(), (x["name"], pair)
            held += 1
    dl.close()
    assert held > 300, held


def test_refusals_and_the_python_surface(work):
    khg, items, host = work
    dl = khg.DeviceLattices.from_lattices([items[0]["L"]])
    for args, msg in (((0,), "n must lie in 1 .. 1024"), ((1025,), "n must lie in 1 .. 1024"), ((1, -1.0, 1.0), "finite and >= 0"),
                      ((1, 1.0, float("inf")), "finite and >= 0")):
        with pytest.raises(khg.KhgError, match=msg):
            dl.nbest(*args)
    dl.close()
    empty = khg.DeviceLattices.from_lattices([])
    nb = empty.nbest(3)
    assert nb.num_utts == 0 and len(nb.download()["total"]) == 0
    nb.close(); empty.close()
    by = {x["name"]: i for i, x in enumerate(items)}
    i = by["sausage7x3"]
    raw = khg.lattice_to_nbest(items[i]["L"], 7, 1.0, 1.0, determinize=False)
    assert [tuple(x) for x in raw] == [tuple(x) for x in items[i]["L"].nbest(7, 1.0, 1.0)]
    det = khg.lattice_to_nbest_batch([items[i]["L"], items[by["empty"]]["L"], items[by["diamond"]]["L"]], 7, 0.5, 1.7, beam=1.0e6)
    assert det.status.tolist() == [ref.SUCCEEDED, ref.NO_PATH, ref.SUCCEEDED] and det.counts.tolist()[:2] == [7, 0]
    for u in (0, 2):
        seqs = [tuple(e[0]) for e in det.entries(u)]
        assert len(set(seqs)) == len(seqs) == det.count(u)
        D, _, _ = items[(i, None, by["diamond"])[u]]["L"].determinize(0.5, 1.7, 1.0e6, 1.0 / 1024, 8)
        assert [tuple(x) for x in det.entries(u)] == [tuple(x) for x in D.nbest(7, 0.5, 1.7)]


def test_decoded_lattices_determinized(setup):  # noqa: F811
    """a lattice-faster decode left on the device -> determinize -> nbest(5) against the host form on the downloaded result"""
    khg, am, tm, dg, feats, cfg = _decoded(setup)
    dres, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    det, st, _ = dl.determinize(1.0, 1.0, cfg.lattice_beam, cfg.det_opts.delta)
    nb = det.nbest(5, 1.0, 1.0)
    nl = khg.NbestList(nb.download())
    n_ok = several = 0
    for u, D in enumerate(det.download()):
        got, hst, _ = D.nbest_with_status(5, 1.0, 1.0)
        _check(nl, u, (hst, got), ("decoded", u))
        if hst == ref.SUCCEEDED:
            n_ok += 1
            seqs = [tuple(e[0]) for e in nl.entries(u)]
            assert len(set(seqs)) == len(seqs), u
            several += len(seqs) > 1
            b = D.best_path(1.0, 1.0)
            assert b["status"] == ref.SUCCEEDED
    assert n_ok >= 15 and several >= 1
    for h in (nb, det, dl, dg):
        h.close()
