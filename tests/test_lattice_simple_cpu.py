"""LatticeSimpleDecoder without a GPU: the bound names against the reference's signatures, the configuration's defaults, __str__ and
Check, and the plain-Python restatement (tests/lattice_simple_ref.py, the yardstick of tests/test_gpu_lattice_simple.py) on
hand-built graphs with hand-computed answers.  The property test shows what the data-parallel kernel rests on: the reference's
answer does not depend on the order it walks its hash maps in."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
from test_lattice_faster_cpu import _doc_args  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
WALKS = ("insertion", "reversed", "shuffle")


def _sig():
    with open(os.path.join(ROOT, "tests", "golden", "lattice_simple_signatures.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("cname", sorted(_sig()["classes"]))
def test_class_signature_matches_reference(cname):
    import kaldi_hmm_gmm_amd as khg
    want = _sig()["classes"][cname]
    cls = getattr(khg, cname)
    got = _doc_args(cls.__init__)
    assert [n for n, _ in got] == [n for n, _ in want["args"]]
    for (n, d), (_, wd) in zip(got, want["args"]):
        assert (d is None) == (wd == "required"), n
    if want["args"][0][1] != "required":
        obj = cls()
        for n, wd in want["args"]:
            if wd is None:
                continue
            v = getattr(obj, n)
            assert v == pytest.approx(wd, rel=1e-7) if isinstance(wd, float) else v == wd, n
    for f in want["fields"]:
        assert isinstance(getattr(cls, f), property), f


def test_function_signature_matches_reference():
    import kaldi_hmm_gmm_amd as khg
    for fname, want in _sig()["functions"].items():
        got = _doc_args(getattr(khg, fname))
        assert [n for n, _ in got] == [n for n, _ in want["args"]]
        assert all(d is None for _, d in got)
        assert getattr(khg, fname).__doc__.strip().splitlines()[0].endswith("-> " + want["returns"])


def test_config_str_and_check():
    import kaldi_hmm_gmm_amd as khg
    det = str(khg.DeterminizeLatticePhonePrunedOptions())
    assert str(khg.LatticeSimpleDecoderConfig()) == (
        "LatticeSimpleDecoderConfig(beam=16, lattice_beam=10, prune_interval=25, determinize_lattice=True, prune_lattice=False, "
        "beam_ratio=0.9, prune_scale=0.1, det_opts=" + det + ")")
    c = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0, prune_interval=7)
    c.beam_ratio = 0.5
    assert str(c).startswith("LatticeSimpleDecoderConfig(beam=13, lattice_beam=6, prune_interval=7, ")
    assert "beam_ratio=0.5" in str(c)
    for bad in (dict(beam=0.0), dict(lattice_beam=-1.0), dict(prune_interval=0)):
        with pytest.raises(RuntimeError, match="Check failed"):
            khg.LatticeSimpleDecoder(khg.StdVectorFst(), khg.LatticeSimpleDecoderConfig(**bad))


def test_decodable_ctc():
    import kaldi_hmm_gmm_amd as khg
    m = np.arange(12, dtype=np.float32).reshape(3, 4) - 5
    d = khg.DecodableCtc(m)
    assert isinstance(d, khg.DecodableInterface)
    assert d.num_frames_ready() == 3 and d.num_indices() == 4
    assert [d.is_last_frame(t) for t in range(3)] == [False, False, True]
    assert d.log_likelihood(2, 1) == m[2, 0] and d.log_likelihood(0, 4) == m[0, 3]
    with pytest.raises(RuntimeError):
        d.log_likelihood(0, 0)


# ---- the restatement on hand-built graphs --------------------------------------------------------------------------------------
def _graph(S, start, arcs, finals):
    """arcs: (src, ilabel, olabel, weight, dst) in the order they are added; finals: {state: weight}"""
    arcs = sorted(arcs, key=lambda a: a[0])      # stable: per-state order kept
    off = np.zeros(S + 1, np.int64)
    for a in arcs:
        off[a[0] + 1] += 1
    final = np.full(S, np.inf, np.float32)
    for s, w in finals.items():
        final[s] = w
    return {"start": start, "arc_off": np.cumsum(off), "ilabel": np.array([a[1] for a in arcs], np.int32),
            "olabel": np.array([a[2] for a in arcs], np.int32), "weight": np.array([a[3] for a in arcs], np.float32),
            "nextstate": np.array([a[4] for a in arcs], np.int32), "final": final}


def _run(g, m, cfg=None, walk="insertion", seed=0, T=None):
    m = np.asarray(m, np.float32).reshape(-1, np.asarray(m).shape[-1]) if np.asarray(m).size else np.zeros((0, 1), np.float32)
    return ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), cfg or ref.Config(), ref.matrix_ll(m), len(m) if T is None else T,
                                               True, walk, seed)


def test_quirk1_at_init():
    g = _graph(2, 0, [(0, 1, 0, 0.0, 1), (1, 1, 0, 0.0, 1)], {1: 0.0})
    with pytest.raises(ref.DecodeError, match=r"^Error in ProcessNonEmitting: no surviving tokens: frame is -1$"):
        _run(g, [[-1.0]])


def test_quirk1_at_a_later_frame():
    # state 0 has an epsilon arc, state 1 (reached by frame 0's emitting arc) has none
    g = _graph(2, 0, [(0, 0, 0, 0.0, 0), (0, 1, 0, 0.0, 1), (1, 1, 0, 0.0, 1)], {1: 0.0})
    with pytest.raises(ref.DecodeError, match=r"frame is 0$"):
        _run(g, [[-1.0], [-1.0]])


@pytest.mark.parametrize("allow_partial", [True, False])
def test_quirk2_no_partial_output(allow_partial):
    g = _graph(2, 0, [(0, 0, 0, 0.0, 0), (0, 1, 3, 0.5, 1), (1, 0, 0, 0.0, 1)], {0: 0.0})    # the only final state is not live at the end
    out = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(), ref.matrix_ll([[-1.0]]), 1, allow_partial)
    assert out == dict(succeeded=False, alignment=[], words=[], like=0.0)


def test_epsilon_chain_revisited():
    # LIFO: 0 -> 2 (5) first, then 0 -> 1 (1); popping 1 improves 2 to 2, so 2 is queued again and its links are rebuilt
    arcs = [(0, 0, 0, 0.0, 0), (0, 0, 9, 5.0, 2), (0, 0, 7, 1.0, 1), (1, 0, 0, 0.0, 1), (1, 0, 8, 1.0, 2), (2, 0, 0, 0.0, 2),
            (2, 1, 0, 0.25, 3), (3, 0, 0, 0.0, 3)]
    g = _graph(4, 0, arcs, {3: 0.125})
    for walk in WALKS:
        out = _run(g, [[-0.5]], walk=walk)
        assert out["succeeded"] and out["alignment"] == [1] and out["words"] == [7, 8]
        assert out["like"] == float(F(-(F(2.375) + F(0.5))))


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(T):
    g = _graph(1, 0, [(0, 1, 0, 0.5, 0), (0, 0, 0, 0.0, 0)], {0: 0.0})
    out = _run(g, np.full((T, 1), -1.0, np.float32))
    v1 = F(0.0)
    for _ in range(T):
        v1 = F(v1 + F(0.5))
    assert out["succeeded"] and out["alignment"] == [1] * T and out["words"] == []
    assert out["like"] == float(F(-F(v1 + F(T))))


def test_running_cutoff_keeps_what_prune_current_tokens_drops():
    # arc to 1 (tot 20) comes first and is kept by the running cutoff (inf -> 36); the arc to 2 (tot 1) tightens it to 17, and
    # PruneCurrentTokens drops state 1: its epsilon arc to the better-weighted final state 3 is never taken
    arcs = [(0, 0, 0, 0.0, 0), (0, 1, 0, 0.0, 1), (0, 2, 0, 0.0, 2), (1, 0, 5, 0.0, 3), (2, 0, 6, 0.0, 2), (2, 0, 0, 0.0, 4),
            (3, 0, 0, 0.0, 3), (4, 0, 0, 0.0, 4)]
    g = _graph(5, 0, arcs, {3: 0.0, 4: 3.0})
    dec = ref.LatticeSimpleDecoder(ref.Graph.from_dict(g), ref.Config())
    dec.init_decoding()
    dec.process_emitting(ref.matrix_ll([[-20.0, -1.0]]))
    assert {s: float(t.tot_cost) for s, t in dec.cur_toks.items()} == {1: 20.0, 2: 1.0}
    dec.prune_current_tokens()
    assert set(dec.cur_toks) == {2}
    for walk in WALKS:
        out = _run(g, [[-20.0, -1.0]], walk=walk)
        assert out["succeeded"] and out["alignment"] == [2] and out["words"] == [] and out["like"] == -(1.0 + 3.0)


def test_tie_rule_lowest_source_state():
    # two paths of exactly the same weight into state 3: through 1 (tid 1) and through 2 (tid 2); the lower source state wins
    arcs = [(0, 0, 0, 0.0, 0), (0, 2, 0, 1.0, 2), (0, 1, 0, 1.0, 1), (1, 0, 0, 0.0, 1), (2, 0, 0, 0.0, 2), (1, 3, 11, 0.0, 3),
            (2, 3, 12, 0.0, 3), (3, 0, 0, 0.0, 3)]
    g = _graph(4, 0, arcs, {3: 0.0})
    m = [[-1.0, -1.0, -9.0], [-9.0, -9.0, -1.0]]
    for walk in WALKS:
        out = _run(g, m, walk=walk)
        assert out["alignment"] == [1, 3] and out["words"] == [11] and out["like"] == -3.0


def test_zero_frames():
    g = _graph(1, 0, [(0, 0, 0, 0.0, 0)], {0: 0.0})
    with pytest.raises(ref.DecodeError, match=r"^Check failed!\nx: num_frames > 0$"):
        _run(g, np.zeros((0, 1), np.float32))
    g["final"][:] = np.inf
    assert not _run(g, np.zeros((0, 1), np.float32))["succeeded"]


def test_negative_epsilon_cycle_raises():
    g = _graph(2, 0, [(0, 0, 0, -1.0, 1), (1, 0, 0, 0.5, 0), (0, 1, 0, 0.0, 0)], {0: 0.0})
    with pytest.raises(ref.EpsilonLoop):
        _run(g, [[-1.0]])


def test_nan_link_raises_check_failed():
    # a NaN score on an arc whose target also gets a finite arc first in no walk: the NaN link survives to PruneForwardLinks
    arcs = [(0, 0, 0, 0.0, 0), (0, 1, 0, 0.0, 1), (0, 2, 0, 0.0, 2), (1, 0, 0, 0.0, 1), (2, 0, 0, 0.0, 2), (1, 1, 0, 0.0, 1),
            (2, 2, 0, 0.0, 2)]
    g = _graph(3, 0, arcs, {1: 0.0, 2: 0.0})
    m = np.array([[-1.0, np.nan], [-1.0, -1.0]], np.float32)
    for walk in WALKS:
        with pytest.raises(ref.DecodeError, match=r"^Check failed!"):
            _run(g, m, walk=walk)


# ---- the property the kernel rests on ------------------------------------------------------------------------------------------
def _random_case(seed):
    rng = np.random.default_rng(seed)
    ntid = int(rng.integers(3, 12))
    g = tg.random_graph(rng, ntid, n_main=int(rng.integers(2, 14)), p_branch=0.5, p_eps=0.5)
    # extra epsilon arcs, backward ones included (cycles of positive weight)
    S = len(g["final"])
    arcs = [(s, int(g["ilabel"][a]), int(g["olabel"][a]), float(g["weight"][a]), int(g["nextstate"][a]))
            for s in range(S) for a in range(int(g["arc_off"][s]), int(g["arc_off"][s + 1]))]
    for _ in range(int(rng.integers(0, 4))):
        arcs.append((int(rng.integers(0, S)), 0, int(rng.integers(0, 20)), float(rng.random() * 2), int(rng.integers(0, S))))
    if rng.random() < 0.3:
        g2 = _graph(S, 0, arcs, {})
        g2["final"] = g["final"]
    else:
        g2 = ref.add_eps_self_loops(_graph(S, 0, arcs, {}) | {"final": g["final"]})
    T = int(rng.integers(1, 40))
    m = (rng.standard_normal((T, ntid)) * 3 - 2).astype(np.float32)
    beam, lbeam = [(13.0, 6.0), (6.0, 2.0), (16.0, 10.0), (3.0, 8.0)][seed % 4]
    return g2, m, ref.Config(beam=beam, lattice_beam=lbeam, prune_interval=int(rng.integers(1, 30)))


def _outcome(g, m, cfg, walk, seed):
    try:
        o = _run(g, m, cfg, walk, seed)
        return (o["succeeded"], o["alignment"], o["words"], o["like"])
    except ref.DecodeError as e:
        return ("raises", str(e))


def test_walk_order_does_not_change_the_answer():
    kinds = {"succeeded": 0, "failed": 0, "raises": 0}
    for seed in range(220):
        g, m, cfg = _random_case(seed)
        outs = [_outcome(g, m, cfg, w, seed) for w in WALKS] + [_outcome(g, m, cfg, "shuffle", seed + 1000)]
        assert all(o == outs[0] for o in outs[1:]), (seed, outs)
        kinds["raises" if outs[0][0] == "raises" else "succeeded" if outs[0][0] else "failed"] += 1
    assert kinds["succeeded"] >= 100 and kinds["raises"] > 0, kinds
