"""One decoding graph shared by many utterances (khg_graph_create / khg_utts_create_on_graph / DecodingGraph), without a GPU:
the entry points exist, and the inputs of tests/test_gpu_shared_graph.py are fit for purpose -- word loops whose loop state has
more incoming arcs than the aligner's 254 and a graph of more than 65 535 states, on which both restatements of the reference's
lattice decoders (tests/lattice_faster_ref.py, tests/lattice_simple_ref.py) succeed, and on which the simple decoder's backward
pass really works (nonzero extra costs, links excised), so that a GPU test over them cannot pass vacuously.

The generators and the restatement runner below are imported by the GPU test."""
import ctypes
import multiprocessing
import os
import re
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import lattice_faster_ref as fref  # noqa: E402
import lattice_simple_ref as sref  # noqa: E402

NEW_SYMBOLS = ("khg_graph_create", "khg_graph_destroy", "khg_graph_info", "khg_utts_create_on_graph", "khg_utts_graph_bytes")
NUM_TIDS = 90          # the transition-ids of the CPU-only inputs (the GPU tests take their model's)


# ---- input generators ------------------------------------------------------------------------------------------------------
def _csr(arcs, S, final_states):
    arcs.sort(key=lambda a: a[0])            # stable: the order inside a state is the order of creation
    arc_off = np.zeros(S + 1, np.int64)
    for a in arcs:
        arc_off[a[0] + 1] += 1
    final = np.full(S, np.inf, np.float32)
    for s, w in final_states:
        final[s] = w
    return {"start": 0, "arc_off": np.cumsum(arc_off),
            "ilabel": np.array([a[1] for a in arcs], np.int32), "olabel": np.array([a[2] for a in arcs], np.int32),
            "weight": np.array([a[3] for a in arcs], np.float32), "nextstate": np.array([a[4] for a in arcs], np.int32), "final": final}


def word_loop_graph(rng, num_tids, W, chain=1):
    """A W-word unigram loop: state 0 is the loop state, start and final; word w is 0 -> s_w1 (carrying the word label w + 1), a
    chain s_w1 -> ... -> s_w`chain` with a self-loop on every state, and s_w`chain` -> 0.  The loop state has W incoming and W
    outgoing arcs; 1 + W * chain states."""
    arcs = []
    tid = lambda: int(rng.integers(1, num_tids + 1))  # noqa: E731
    for w in range(W):
        first = 1 + w * chain
        arcs.append((0, tid(), w + 1, float(rng.random()), first))
        for k in range(chain):
            s = first + k
            arcs.append((s, tid(), 0, float(rng.random()) * 0.5, s))
            arcs.append((s, tid(), 0, float(rng.random()), s + 1 if k + 1 < chain else 0))
    return _csr(arcs, 1 + W * chain, [(0, 0.0)])


def max_in_degree(g):
    return int(np.bincount(np.asarray(g["nextstate"]), minlength=len(g["final"])).max())


def tid_scores(seed, T, num_tids, scale=1.0):
    """[T][num_tids] scores for matrix_ll: ll(frame, tid) = m[frame, tid - 1]."""
    return (np.random.default_rng(seed).standard_normal((T, num_tids)) * scale).astype(np.float32)


# ---- the restatements, several at once (plain Python: a W = 3000 utterance is ~35 s, the 66 001-state one ~170 s) --------------
def restate(job):
    """job: dict(kind 'faster' | 'simple', graph, cfg (keywords of the restatement's Config), T, and the scores: `matrix`
    ([T][num_tids], matrix_ll) or `k1` = (loglikes, pdfs, id2pdf, acoustic_scale) (score_fn)) -> the restatement's dict (+ stats)."""
    ll = sref.matrix_ll(job["matrix"]) if "matrix" in job else fref.score_fn(*job["k1"])
    g = fref.Graph.from_dict(job["graph"])
    if job["kind"] == "faster":
        return fref.decode_utterance_lattice_faster(g, fref.Config(**job["cfg"]), ll, job["T"], True)
    stats = {}
    try:
        out = sref.decode_utterance_lattice_simple(g, sref.Config(**job["cfg"]), ll, job["T"], stats=stats)
    except sref.DecodeError as e:
        out = {"error": str(e)}
    out["stats"] = stats
    return out


def restate_many(jobs, workers=None):
    """The jobs' restatements, in worker processes that import nothing but numpy and the two restatements (started fresh: they
    share nothing with a caller that holds a GPU)."""
    workers = min(len(jobs), 8, os.cpu_count() or 1) if workers is None else workers
    if workers <= 1:
        return [restate(j) for j in jobs]
    with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
        return list(ex.map(restate, jobs))


FASTER_CFG = dict(beam=13.0, lattice_beam=6.0)
SIMPLE_CFG = dict(beam=13.0, lattice_beam=6.0)
BIG_W, BIG_CHAIN = 6600, 10          # 66 001 states, 138 600 arcs, hub in-degree 6 600


# ---- the entry points exist --------------------------------------------------------------------------------------------------
def test_entry_points_declared_and_exported():
    from kaldi_hmm_gmm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "khg_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in include/khg_hip.h"
        assert hasattr(lib, name), name + " is not exported by libkhg_hip.so"
        assert name in _lib.SIGNATURES
    assert re.search(r"typedef\s+struct\s+khg_graph\s+khg_graph\s*;", hdr)
    assert "KHG_OPT_K2S_HUB" in hdr


def test_python_names():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import device
    assert khg.DecodingGraph is device.DecodingGraph
    for attr in ("num_states", "num_arcs", "num_pdfs", "max_in_degree", "device_bytes", "close"):
        assert hasattr(khg.DecodingGraph, attr), attr
    doc = khg.UtteranceSet.__init__.__doc__
    assert "graphs:" in doc and "graph:" in doc, doc
    assert "fst" in khg.DecodingGraph.__init__.__doc__ and "tm" in khg.DecodingGraph.__init__.__doc__


# ---- the inputs are fit for purpose -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    """Every restatement this file asserts on, run once, side by side."""
    jobs, keys = [], []
    for W, T in ((300, 40), (300, 60), (3000, 40), (3000, 60)):
        g = word_loop_graph(np.random.default_rng(W), NUM_TIDS, W)
        m = tid_scores(W + T, T, NUM_TIDS)
        jobs.append(dict(kind="faster", graph=g, cfg=FASTER_CFG, T=T, matrix=m)); keys.append((W, T, "faster"))
        for lw in (0.0, 0.25):
            jobs.append(dict(kind="simple", graph=sref.add_eps_self_loops(g, lw), cfg=SIMPLE_CFG, T=T, matrix=m)); keys.append((W, T, "simple", lw))
    g = word_loop_graph(np.random.default_rng(66001), NUM_TIDS, BIG_W, BIG_CHAIN)
    m = tid_scores(66001, 40, NUM_TIDS)
    jobs.append(dict(kind="faster", graph=g, cfg=dict(FASTER_CFG, max_active=7000), T=40, matrix=m)); keys.append(("big", "faster"))
    jobs.append(dict(kind="simple", graph=sref.add_eps_self_loops(g, 0.25), cfg=SIMPLE_CFG, T=40, matrix=m)); keys.append(("big", "simple"))
    return dict(zip(keys, restate_many(jobs)))


@pytest.mark.parametrize("W", [300, 3000])
def test_word_loop_inputs(restated, W):
    g = word_loop_graph(np.random.default_rng(W), NUM_TIDS, W)
    assert max_in_degree(g) == W > 254 and len(g["final"]) == W + 1
    assert max_in_degree(sref.add_eps_self_loops(g)) == W + 1
    for T in (40, 60):
        fa = restated[(W, T, "faster")]
        assert fa["succeeded"] and not fa["partial"] and len(fa["words"]) >= 2 and len(fa["alignment"]) == T
        s0 = restated[(W, T, "simple", 0.0)]
        # zero-weight epsilon self-loops change no path's weight: the simple decoder returns the faster decoder's path
        assert s0["succeeded"] and (s0["alignment"], s0["words"], s0["like"]) == (fa["alignment"], fa["words"], fa["like"])
        s1 = restated[(W, T, "simple", 0.25)]
        assert s1["succeeded"] and s1["stats"]["nonzero_extra"] > 0 and s1["stats"]["excised"] > 0, s1["stats"]


def test_graph_of_more_than_65535_states(restated):
    g = word_loop_graph(np.random.default_rng(66001), NUM_TIDS, BIG_W, BIG_CHAIN)
    assert len(g["final"]) == 66001 > 65535 and int(g["arc_off"][-1]) == 138600 and max_in_degree(g) == BIG_W
    fa, si = restated[("big", "faster")], restated[("big", "simple")]
    assert fa["succeeded"] and not fa["partial"] and len(fa["words"]) >= 1
    assert si["succeeded"] and len(si["words"]) >= 1
    assert si["stats"]["nonzero_extra"] > 0 and si["stats"]["excised"] > 0, si["stats"]
