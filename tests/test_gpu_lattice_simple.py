"""The data-parallel lattice-simple decoder on the GPU (khg_decode_lattice_simple through decode_lattice_simple_batch /
decode_utterance_lattice_simple) against the plain-Python restatement of the reference (tests/lattice_simple_ref.py), bit for bit:
succeeded, alignment, words and `like`.  Scores come from K1 (return_scores=True), so only the decoder is compared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAT_SUCCEEDED, LAT_SCRATCH, LAT_NO_PATH, LAT_EPS_LOOP, LAT_NO_EPS_TOKEN, LAT_NAN = 1, 4, 8, 16, 128, 256


@pytest.fixture(scope="module")
def setup():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import synth
    m = synth.make_model(30, 4, 12, seed=11)
    am, tm = synth.host_objects(m)
    ut = synth.make_utts(m, 24, seed=5, min_phones=8, max_phones=20)
    return khg, synth, m, am, tm, ut


def _fst(khg, g):
    return khg.StdVectorFst.from_csr(int(g["start"]), np.asarray(g["arc_off"], np.int64), np.asarray(g["ilabel"], np.int32),
                                     np.asarray(g["olabel"], np.int32), np.asarray(g["weight"], np.float32),
                                     np.asarray(g["nextstate"], np.int32), np.asarray(g["final"], np.float32))


def _feats(ut, n, lens=None):
    out = []
    for u in range(n):
        f = ut.feats[ut.frame_off[u % (len(ut.frame_off) - 1)]: ut.frame_off[u % (len(ut.frame_off) - 1) + 1]]
        if lens is not None:
            f = np.concatenate([f] * (lens[u] // len(f) + 1))[: lens[u]]
        out.append(np.ascontiguousarray(f, np.float32))
    return out


def _want(g, rcfg, ll, T, stats=None):
    try:
        return ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), rcfg, ll, T, stats=stats), None
    except ref.DecodeError as e:
        return None, e


def _check(khg, m, am, tm, gs, feats, beam, lbeam, scale=0.1, scratch=0, expect_errors=False, stats=None):
    fsts = [_fst(khg, g) for g in gs]
    cfg = khg.LatticeSimpleDecoderConfig(beam=beam, lattice_beam=lbeam)
    rcfg = ref.Config(beam=beam, lattice_beam=lbeam)
    res = khg.decode_lattice_simple_batch(am, tm, fsts, feats, cfg, scale, return_scores=True, scratch_per_frame=scratch)
    n_ok = 0
    for u, (g, r) in enumerate(zip(gs, res)):
        ll = ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, scale)
        want, err = _want(g, rcfg, ll, len(feats[u]), stats)
        if err is not None:
            assert expect_errors, (u, str(err))
            if "ProcessNonEmitting" in str(err):
                assert r["status"] == LAT_NO_EPS_TOKEN and str(err).endswith("frame is %d" % r["error_frame"]), (u, r["status"])
            continue
        assert r["succeeded"] == want["succeeded"], (u, r["status"], want)
        assert r["alignment"] == want["alignment"], u
        assert r["words"] == want["words"], u
        assert r["like"] == want["like"], (u, r["like"], want["like"])
        n_ok += want["succeeded"]
    return res, n_ok


@pytest.mark.parametrize("kind", ["random", "hub"])
@pytest.mark.parametrize("beams", [(13.0, 6.0), (6.0, 2.0), (16.0, 10.0)])
def test_graphs_with_self_loops(setup, kind, beams):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(int(beams[0]) * 7 + (3 if kind == "hub" else 0))
    n = 8
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if kind == "random"
                                 else tg.hub_graph(rng, m.num_tids, fan=8, tail=5)) for _ in range(n)]
    _, n_ok = _check(khg, m, am, tm, gs, _feats(ut, n), *beams)
    assert n_ok > 0


@pytest.mark.parametrize("loop_w", [0.25, 1.0])
@pytest.mark.parametrize("beams", [(13.0, 6.0), (6.0, 2.0), (16.0, 4.0), (8.0, 1.0)])
def test_nonzero_extra_costs_and_lattice_beam_pruning(setup, loop_w, beams):
    """Positive-weight epsilon self-loops leave the extra costs free (a zero-weight loop pins them at 0): the backward pass --
    ComputeFinalCosts, the final-frame rule, the extra-cost recurrences -- and the links it excises decide which paths survive.
    The restatement's own counts show the pass really worked: nonzero extra costs and links excised by lattice_beam."""
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(int(beams[0] * 10 + beams[1] + 100 * loop_w))
    n = 8
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if u % 2 == 0
                                 else tg.hub_graph(rng, m.num_tids, fan=8, tail=5), loop_w) for u in range(n)]
    stats = {}
    _, n_ok = _check(khg, m, am, tm, gs, _feats(ut, n), *beams, stats=stats)
    assert n_ok > 0
    assert stats["nonzero_extra"] > 0 and stats["excised"] > 0, stats


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(setup, T):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(T)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.3)) for _ in range(4)]
    _check(khg, m, am, tm, gs, _feats(ut, 4, [T] * 4), 10.0, 4.0)


def test_mismatched_model(setup):
    khg, synth, m, am, tm, ut = setup
    mm = synth.mismatched_model(m, 0.5, seed=3)
    am2, tm2 = synth.host_objects(mm)
    rng = np.random.default_rng(9)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=10, p_branch=0.6, p_eps=0.3)) for _ in range(8)]
    _check(khg, mm, am2, tm2, gs, _feats(ut, 8), 6.0, 2.0)


def test_large_graph_and_batch_equals_single(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(1234)
    g = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=1100, p_eps=0.2))
    small = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=9, p_eps=0.3)) for _ in range(3)]
    gs = [g, small[0], g, small[1], small[2]]
    feats = _feats(ut, 5, [60, 30, 40, 20, 25])
    res, n_ok = _check(khg, m, am, tm, gs, feats, 13.0, 6.0)
    assert n_ok >= 3
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    for u in range(len(gs)):
        dec = khg.LatticeSimpleDecoder(_fst(khg, gs[u]), cfg)
        d = khg.DecodableAmDiagGmmScaled(am, tm, feats[u], 0.1)
        one = khg.decode_utterance_lattice_simple(dec, d, tm, "utt%d" % u, True)
        assert one == (res[u]["succeeded"], res[u]["alignment"], res[u]["words"], res[u]["like"]), u


def test_status_bits_and_messages(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(5)
    base = tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.0)                  # no epsilon arc anywhere: Quirk 1 at frame -1
    nofinal = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, with_final=False))
    good = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6))
    later = {k: np.array(v) for k, v in base.items()}                             # an epsilon self-loop on the start only
    S = len(later["final"])
    n0 = int(later["arc_off"][1])
    for k, v in (("ilabel", 0), ("olabel", 0), ("weight", 0.0), ("nextstate", 0)):
        later[k] = np.insert(later[k], n0, v)
    later["arc_off"] = np.concatenate([[0], np.asarray(later["arc_off"][1:]) + 1]).astype(np.int64)
    assert S > 1
    gs = [base, nofinal, good, later]
    feats = _feats(ut, 4)
    res, _ = _check(khg, m, am, tm, gs, feats, 13.0, 6.0, expect_errors=True)
    assert res[0]["status"] == LAT_NO_EPS_TOKEN and res[0]["error_frame"] == -1
    assert res[1]["status"] == LAT_NO_PATH and not res[1]["succeeded"]
    assert res[2]["status"] == LAT_SUCCEEDED
    assert res[3]["status"] == LAT_NO_EPS_TOKEN and res[3]["error_frame"] == 0
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    with pytest.raises(RuntimeError, match=r"^Error in ProcessNonEmitting: no surviving tokens: frame is -1$"):
        khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, base), cfg), khg.DecodableAmDiagGmmScaled(am, tm, feats[0], 0.1),
                                            tm, "u0", True)
    for ap in (True, False):     # Quirk 2: no partial output whatever allow_partial says
        assert khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, nofinal), cfg),
                                                   khg.DecodableAmDiagGmmScaled(am, tm, feats[1], 0.1), tm, "u1", ap) == (False, [], [], 0.0)
    # scratch_per_frame: a frame over the limit gets KHG_LAT_SCRATCH, no output
    res = khg.decode_lattice_simple_batch(am, tm, [_fst(khg, good)], feats[2:3], cfg, 0.1, scratch_per_frame=1)
    assert res[0]["status"] == LAT_SCRATCH and not res[0]["succeeded"]


def _hand(S, start, arcs, finals):
    arcs = sorted(arcs, key=lambda a: a[0])
    off = np.zeros(S + 1, np.int64)
    for a in arcs:
        off[a[0] + 1] += 1
    final = np.full(S, np.inf, np.float32)
    for st, w in finals.items():
        final[st] = w
    return {"start": start, "arc_off": np.cumsum(off), "ilabel": np.array([a[1] for a in arcs], np.int32),
            "olabel": np.array([a[2] for a in arcs], np.int32), "weight": np.array([a[3] for a in arcs], np.float32),
            "nextstate": np.array([a[4] for a in arcs], np.int32), "final": final}


def test_words_overflow_and_scratch_at_the_start_closure(setup):
    khg, synth, m, am, tm, ut = setup
    # every frame walks an epsilon chain 0 -> ... -> 9 with a word on each arc: 9 (T + 1) words > T + S + 64 (KHG_LAT_WORDS)
    arcs = [(i, 0, i + 1, 0.01, i + 1) for i in range(9)] + [(9, 1, 0, 0.0, 0)]
    g = _hand(10, 0, arcs, {9: 0.0})
    feats = _feats(ut, 1, [20])
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    r = khg.decode_lattice_simple_batch(am, tm, [_fst(khg, g)], feats, cfg, 0.1, return_scores=True)[0]
    want = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(13.0, 6.0),
                                               ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, 0.1), 20)
    assert want["succeeded"] and len(want["words"]) == 9 * 21 > 20 + 10 + 64
    assert r["status"] == 32 and not r["succeeded"] and r["words"] == []
    with pytest.raises(RuntimeError, match="more words on the best path"):
        khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, g), cfg), khg.DecodableAmDiagGmmScaled(am, tm, feats[0], 0.1),
                                            tm, "w", True)
    # the start closure holds 3 live tokens (0, 1, 2), every later frame 2: a limit of 2 stops at InitDecoding, 3 decodes
    arcs = [(0, 0, 0, 0.5, 1), (0, 0, 0, 0.5, 2), (1, 0, 0, 0.1, 1), (2, 0, 0, 0.1, 2), (1, 1, 0, 0.0, 1), (2, 2, 0, 0.0, 2)]
    g = _hand(3, 0, arcs, {1: 0.0, 2: 0.5})
    feats = _feats(ut, 1, [12])
    assert khg.decode_lattice_simple_batch(am, tm, [_fst(khg, g)], feats, cfg, 0.1, scratch_per_frame=2)[0]["status"] == LAT_SCRATCH
    r3 = khg.decode_lattice_simple_batch(am, tm, [_fst(khg, g)], feats, cfg, 0.1, scratch_per_frame=3)[0]
    r0 = khg.decode_lattice_simple_batch(am, tm, [_fst(khg, g)], feats, cfg, 0.1)[0]
    assert r3["status"] == LAT_SUCCEEDED and r3 == r0


def test_nan_status_on_resident_scores(setup):
    """A NaN score on the one arc into state 2 at frame 0: the NaN link reaches PruneForwardLinks' assertion (KHG_LAT_NAN)."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    pdf = np.asarray(m.id2pdf)
    ta = 1
    tb = next(t for t in range(2, m.num_tids + 1) if pdf[t] != pdf[ta])
    arcs = [(0, 0, 0, 0.0, 0), (0, ta, 0, 0.0, 1), (0, tb, 0, 0.0, 2), (1, 0, 0, 0.0, 1), (2, 0, 0, 0.0, 2), (1, ta, 0, 0.0, 1),
            (2, tb, 0, 0.0, 2)]
    g = _hand(3, 0, arcs, {1: 0.0, 2: 0.0})
    T = 6
    feats = _feats(ut, 1, [T])[0]
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ctx = Context(0)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, np.array([0, T], np.int64), feats, graphs=tg.concat([g]))
    us.loglikes(dm)
    clean = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    assert int(clean["status"][0]) == LAT_SUCCEEDED
    mats = [np.array(x, np.float32) for x in us.download_loglikes()]
    row = sorted(set(int(pdf[t]) for t in (ta, tb))).index(int(pdf[tb]))
    mats[0][row, 0] = np.nan
    us.upload_loglikes(mats)
    d = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    assert int(d["status"][0]) == LAT_NAN and int(d["error_frame"][0]) == -1


def _ctc_topo(n_tokens):
    """scripts/ctc_topo.py's shape: state 0 is the blank state (start, final); state i is token i.  Indices are token + 1 (the
    DecodableCtc convention); olabel = token id on entry.  Disambiguation-style input-epsilon self-loops on every state."""
    arcs = []
    S = n_tokens
    for i in range(S):
        for j in range(S):
            if i == j:
                arcs.append((i, i + 1, 0, 0.0, i))
            else:
                arcs.append((i, j + 1, j, 0.0, j))
        arcs.append((i, 0, 0, 0.0, i))
    arcs.sort(key=lambda a: a[0])
    off = np.zeros(S + 1, np.int64)
    for a in arcs:
        off[a[0] + 1] += 1
    final = np.full(S, np.inf, np.float32)
    final[0] = 0.0
    return {"start": 0, "arc_off": np.cumsum(off), "ilabel": np.array([a[1] for a in arcs], np.int32),
            "olabel": np.array([a[2] for a in arcs], np.int32), "weight": np.array([a[3] for a in arcs], np.float32),
            "nextstate": np.array([a[4] for a in arcs], np.int32), "final": final}


def test_ctc_topology_decodable_ctc_and_python_decodable(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(21)
    g = _ctc_topo(12)
    fst = _fst(khg, g)

    class PyMat(khg.DecodableInterface):
        def __init__(self, mat):
            super().__init__()
            self.m = mat

        def log_likelihood(self, frame, index):
            return float(self.m[frame, index - 1])

        def num_frames_ready(self):
            return self.m.shape[0]

        def num_indices(self):
            return self.m.shape[1]

        def is_last_frame(self, frame):
            return frame == self.m.shape[0] - 1

    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    for u in range(6):
        T = int(rng.integers(5, 40))
        x = rng.standard_normal((T, 12)).astype(np.float32) * 3
        mat = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)      # log-softmax rows
        want = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(13.0, 6.0), ref.matrix_ll(mat), T)
        assert want["succeeded"]
        got = khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(fst, cfg), khg.DecodableCtc(mat), tm, "c%d" % u, True)
        assert got == (want["succeeded"], want["alignment"], want["words"], want["like"]), u
        assert khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(fst, cfg), PyMat(mat), tm, "p%d" % u, True) == got
        # the other decoders read DecodableCtc's matrix directly: same answers as through a Python decodable
        fc = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
        assert (khg.decode_utterance_lattice_faster(khg.LatticeFasterDecoder(fst, fc), khg.DecodableCtc(mat), tm, "c", True)
                == khg.decode_utterance_lattice_faster(khg.LatticeFasterDecoder(fst, fc), PyMat(mat), tm, "p", True))
        fd1 = khg.FasterDecoder(fst, khg.FasterDecoderOptions(beam=13.0))
        fd1.decode(khg.DecodableCtc(mat))
        fd2 = khg.FasterDecoder(fst, khg.FasterDecoderOptions(beam=13.0))
        fd2.decode(PyMat(mat))
        (ok1, l1), (ok2, l2) = fd1.get_best_path(), fd2.get_best_path()
        s1, s2 = l1.get_linear_symbol_sequence(), l2.get_linear_symbol_sequence()
        assert ok1 == ok2 and s1[:3] == s2[:3] and str(s1[3]) == str(s2[3])


def test_nan_and_zero_frames_through_decodable_ctc(setup):
    khg, synth, m, am, tm, ut = setup
    # state 0 loops; 0 -> 1 on index 1 and 0 -> 2 on index 2; a NaN score on index 2 at frame 0 (state 2 gets only that arc)
    g = {"start": 0, "arc_off": np.array([0, 4, 6, 8], np.int64), "ilabel": np.array([0, 1, 2, 3, 0, 1, 0, 2], np.int32),
         "olabel": np.zeros(8, np.int32), "weight": np.zeros(8, np.float32), "nextstate": np.array([0, 1, 2, 0, 1, 1, 2, 2], np.int32),
         "final": np.array([np.inf, 0.0, 0.0], np.float32)}
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    mat = np.full((3, 3), -1.0, np.float32)
    mat[0, 1] = np.nan
    with pytest.raises(ref.DecodeError, match="Check failed"):
        ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(13.0, 6.0), ref.matrix_ll(mat), 3)
    with pytest.raises(RuntimeError, match=r"^Check failed!"):
        khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, g), cfg), khg.DecodableCtc(mat), tm, "nan", True)
    # zero frames: a final start closure stops at GetRawLattice's assertion, a non-final one gives no output
    z = np.zeros((0, 3), np.float32)
    g["final"][0] = 0.0
    with pytest.raises(RuntimeError, match=r"^Check failed!\nx: num_frames > 0$"):
        khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, g), cfg), khg.DecodableCtc(z), tm, "z", True)
    g["final"][0] = np.inf
    assert khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, g), cfg), khg.DecodableCtc(z), tm, "z", True) == (False, [], [], 0.0)


def test_negative_epsilon_cycle_and_band_refused(setup):
    khg, synth, m, am, tm, ut = setup
    g = {"start": 0, "arc_off": np.array([0, 2, 3], np.int64), "ilabel": np.array([0, 1, 0], np.int32), "olabel": np.zeros(3, np.int32),
         "weight": np.array([-1.0, 0.0, 0.5], np.float32), "nextstate": np.array([1, 0, 0], np.int32), "final": np.array([0.0, np.inf], np.float32)}
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    res = khg.decode_lattice_simple_batch(am, tm, [_fst(khg, g)], _feats(ut, 1), cfg, 0.1)
    assert res[0]["status"] == LAT_EPS_LOOP
    # band-mode scores hold bounds past the band: refused
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    m = synth.make_model(30, 64, 40, seed=7)              # the band form of K1 runs on the packed kernel: pdfs of 64 Gaussians, dim 40
    ut = synth.make_utts(m, 8, seed=2, min_phones=3, max_phones=6)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ctx = Context(0)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm, reachable_only=True, band=True)
    with pytest.raises(Exception, match="khg_loglikes_band"):
        us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    us.loglikes(dm, reachable_only=False, band=False)
    d = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    # training graphs are epsilon-free: Quirk 1 at InitDecoding for every utterance, as in the reference
    assert (np.asarray(d["status"]) == LAT_NO_EPS_TOKEN).all() and (np.asarray(d["error_frame"]) == -1).all()
