"""The lattice decoder on the GPU (khg_decode_lattice_faster through decode_lattice_faster_batch / decode_utterance_lattice_faster)
against the plain-Python restatement of the reference (tests/lattice_faster_ref.py), bit for bit: succeeded, partial, alignment,
words and `like`.  Scores come from K1 (return_scores=True), so only the decoder is compared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_faster_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

LAT_SUCCEEDED, LAT_PARTIAL, LAT_SCRATCH = 1, 2, 4


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


def _check(khg, m, am, tm, gs, feats, cfg, scale=0.1, allow_partial=True, rcfg=None, scratch=0):
    fsts = [_fst(khg, g) for g in gs]
    res = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, scale, allow_partial=allow_partial, return_scores=True,
                                          scratch_per_frame=scratch)
    stats = {"succeeded": 0, "partial": 0}
    for u, (g, r) in enumerate(zip(gs, res)):
        ll = ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, scale)
        want = ref.decode_utterance_lattice_faster(ref.Graph.from_dict(g), rcfg, ll, len(feats[u]), allow_partial)
        assert r["succeeded"] == want["succeeded"], (u, r["status"], want)
        assert r["partial"] == want["partial"], (u, r["status"], want)
        assert r["alignment"] == want["alignment"], u
        assert r["words"] == want["words"], u
        assert r["like"] == want["like"], (u, r["like"], want["like"])
        stats["succeeded"] += want["succeeded"]
        stats["partial"] += want["partial"]
    return res, stats


def _cfgs(khg, **kw):
    return khg.LatticeFasterDecoderConfig(**kw), ref.Config(**{k: v for k, v in kw.items() if k != "determinize_lattice"})


@pytest.mark.parametrize("kind", ["random", "hub"])
@pytest.mark.parametrize("max_active", [3, 10, 7000])
@pytest.mark.parametrize("min_active", [0, 200])
def test_graphs_active_limits(setup, kind, max_active, min_active):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(100 + max_active + min_active + (7 if kind == "hub" else 0))
    n = 6
    gs = [tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if kind == "random" else tg.hub_graph(rng, m.num_tids, fan=8, tail=5)
          for _ in range(n)]
    if min_active > max_active:
        min_active = max_active
    cfg, rcfg = _cfgs(khg, beam=13.0, max_active=max_active, min_active=min_active, lattice_beam=6.0)
    _, st = _check(khg, m, am, tm, gs, _feats(ut, n), cfg, rcfg=rcfg)
    assert st["succeeded"] > 0


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(setup, T):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(T)
    gs = [tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.3) for _ in range(4)]
    cfg, rcfg = _cfgs(khg, beam=10.0, lattice_beam=4.0)
    _check(khg, m, am, tm, gs, _feats(ut, 4, [T] * 4), cfg, rcfg=rcfg)


def test_mismatched_model_pruning_bites(setup):
    khg, synth, m, am, tm, ut = setup
    mm = synth.mismatched_model(m, 0.5, seed=3)
    am2, tm2 = synth.host_objects(mm)
    rng = np.random.default_rng(9)
    gs = [tg.random_graph(rng, m.num_tids, n_main=10, p_branch=0.6, p_eps=0.3) for _ in range(8)]
    cfg, rcfg = _cfgs(khg, beam=6.0, max_active=10, min_active=2, lattice_beam=2.0)
    _check(khg, mm, am2, tm2, gs, _feats(ut, 8), cfg, rcfg=rcfg)


def test_large_graph_above_1000_states(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(1234)
    g = tg.random_graph(rng, m.num_tids, n_main=1100, p_eps=0.2)
    cfg, rcfg = _cfgs(khg, beam=13.0, max_active=7000, lattice_beam=6.0)
    _check(khg, m, am, tm, [g, g], _feats(ut, 2, [120, 60]), cfg, rcfg=rcfg)


@pytest.mark.parametrize("allow_partial", [True, False])
def test_no_final_state(setup, allow_partial):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    gs = [tg.random_graph(rng, m.num_tids, n_main=8, with_final=(u % 2 == 0)) for u in range(6)]
    cfg, rcfg = _cfgs(khg, beam=13.0, lattice_beam=6.0)
    res, st = _check(khg, m, am, tm, gs, _feats(ut, 6), cfg, allow_partial=allow_partial, rcfg=rcfg)
    assert st["partial"] == 3
    for u in (1, 3, 5):
        assert res[u]["partial"] and res[u]["succeeded"] == allow_partial


def test_batch_equals_per_utterance_calls(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(5)
    gs = [tg.random_graph(rng, m.num_tids, n_main=10, p_eps=0.3) for _ in range(5)]
    feats = _feats(ut, 5)
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    batch = khg.decode_lattice_faster_batch(am, tm, [_fst(khg, g) for g in gs], feats, cfg, 0.1)
    for u, g in enumerate(gs):
        dec = khg.LatticeFasterDecoder(_fst(khg, g), cfg)
        d = khg.DecodableAmDiagGmmScaled(am, tm, feats[u], 0.1)
        ok, ali, words, like = khg.decode_utterance_lattice_faster(decoder=dec, decodable=d, trans_model=tm, utt=str(u), allow_partial=True)
        assert (ok, ali, words, like) == (batch[u]["succeeded"], batch[u]["alignment"], batch[u]["words"], batch[u]["like"])


def test_python_decodable_matches_restatement(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(8)
    g = tg.hub_graph(rng, 12, fan=5, tail=4)
    T = 30
    tab = np.random.default_rng(3).normal(size=(T, 13)).astype(np.float32)

    class Dec(khg.DecodableInterface):
        def log_likelihood(self, frame, index):
            return float(tab[frame, index])

        def is_last_frame(self, frame):
            return frame == T - 1

        def num_frames_ready(self):
            return T

        def num_indices(self):
            return 12
    cfg, rcfg = _cfgs(khg, beam=9.0, lattice_beam=5.0, max_active=6, min_active=2)
    got = khg.decode_utterance_lattice_faster(khg.LatticeFasterDecoder(_fst(khg, g), cfg), Dec(), tm, "u", True)
    want = ref.decode_utterance_lattice_faster(ref.Graph.from_dict(g), rcfg, lambda f, i: np.float32(tab[f, i]), T, True)
    assert got == (want["succeeded"], want["alignment"], want["words"], want["like"])


def test_small_scratch_reports_status_bit(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(21)
    gs = [tg.hub_graph(rng, m.num_tids, fan=10, tail=5) for _ in range(4)]
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    res = khg.decode_lattice_faster_batch(am, tm, [_fst(khg, g) for g in gs], _feats(ut, 4), cfg, 0.1, scratch_per_frame=1)
    assert all(r["status"] & LAT_SCRATCH and not r["succeeded"] for r in res)
    assert all(r["alignment"] == [] for r in res)
    ok = khg.decode_lattice_faster_batch(am, tm, [_fst(khg, g) for g in gs], _feats(ut, 4), cfg, 0.1)
    assert all(not (r["status"] & LAT_SCRATCH) for r in ok)


def test_seeded_fuzz_slice(setup):
    """A fixed number of seeded cases (about 5 s with the restatement): random graphs, beams, active limits, prune intervals,
    lengths from 1 to 60 frames, missing final states, allow_partial on and off."""
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(2024)
    for _ in range(12):
        gs = [tg.random_graph(rng, m.num_tids, n_main=int(rng.integers(3, 15)), p_branch=float(rng.random()), p_eps=float(rng.random() * 0.6),
                              with_final=bool(rng.random() < 0.8)) for _ in range(4)]
        ma = int(rng.choice([2, 4, 16, 7000]))
        cfg, rcfg = _cfgs(khg, beam=float(rng.uniform(3, 15)), max_active=ma, min_active=int(rng.integers(0, ma)),
                          lattice_beam=float(rng.uniform(0.5, 8)), prune_interval=int(rng.integers(1, 30)))
        lens = [int(x) for x in rng.integers(1, 60, size=4)]
        _check(khg, m, am, tm, gs, _feats(ut, 4, lens), cfg, allow_partial=bool(rng.random() < 0.7), rcfg=rcfg)


def test_epsilon_loop_is_reported(setup):
    """0 -eps(0.1)-> 1 -eps(0.1)-> 0: both links survive, TopSortTokens cannot order the frame -- the reference asserts
    "Epsilon loops exist in your decoding graph"; so does the binding, and the batch reports KHG_LAT_EPS_LOOP (16)."""
    khg, synth, m, am, tm, ut = setup
    g = {"start": 0, "arc_off": np.array([0, 2, 3], np.int64), "ilabel": np.array([1, 0, 0], np.int32),
         "olabel": np.array([0, 5, 6], np.int32), "weight": np.array([0.0, 0.1, 0.1], np.float32),
         "nextstate": np.array([0, 1, 0], np.int32), "final": np.array([0.0, np.inf], np.float32)}
    f = _feats(ut, 1)[0]
    res = khg.decode_lattice_faster_batch(am, tm, [_fst(khg, g)], [f], khg.LatticeFasterDecoderConfig(), 0.1)
    assert res[0]["status"] & 16 and not res[0]["succeeded"]
    with pytest.raises(Exception, match="Epsilon loops"):
        khg.decode_utterance_lattice_faster(khg.LatticeFasterDecoder(_fst(khg, g), khg.LatticeFasterDecoderConfig()),
                                            khg.DecodableAmDiagGmmScaled(am, tm, f, 0.1), tm, "u", True)
    with pytest.raises(Exception, match="num_frames > 0"):
        khg.decode_lattice_faster_batch(am, tm, [_fst(khg, g)], [f[:0]], khg.LatticeFasterDecoderConfig(), 0.1)


def test_band_scores_are_refused(setup):
    """khg_loglikes_band leaves upper bounds past each pdf's band: the lattice decoder refuses such scores (KHG_E_ARG) instead of
    decoding on them, and decodes the same set once its scores are complete."""
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    khg, synth = setup[0], setup[1]
    m = synth.make_model(30, 64, 40, seed=7)              # the band form of K1 runs on the packed kernel: pdfs of 64 Gaussians, dim 40
    ut = synth.make_utts(m, 8, seed=2, min_phones=3, max_phones=6)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ctx = Context(0)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm, reachable_only=True, band=True)
    with pytest.raises(Exception, match="khg_loglikes_band"):
        us.decode_lattice_faster(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    us.loglikes(dm, reachable_only=False, band=False)
    d = us.decode_lattice_faster(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    assert (np.asarray(d["status"]) & LAT_SUCCEEDED).all()


def test_trained_word_loop_model_at_decode_py_config(setup):
    """egs/yesno/decode.py's configuration (max_active 7000, beam 13, lattice_beam 6) on the trained monophone model and the
    unigram word-loop graph of examples/decode_synthetic.py (cycles, in-degree 7): every held-out utterance matches the
    restatement bit for bit, and the words recover the transcripts."""
    import types
    khg = setup[0]
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import decode_synthetic as dx
    from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions
    args = types.SimpleNamespace(utts=200, test_utts=30, iters=80, dim=23, seed=3)
    tm, tree, am, lexicon, test_utts = dx.train(args, log=lambda *a: None)
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                  opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gcomp.compile_word_loop_graph()
    feats = [u[2] for u in test_utts]
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    res = khg.decode_lattice_faster_batch(am, tm, graph, feats, cfg, 0.1, allow_partial=True, return_scores=True)
    c = graph.to_csr()
    g = ref.Graph(c["start"], c["arc_off"], c["ilabel"], c["olabel"], c["weight"], c["nextstate"], c["final"])
    rcfg = ref.Config(max_active=7000, beam=13.0, lattice_beam=6.0)
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    errs = nref = 0
    for u, r in zip(test_utts, res):
        want = ref.decode_utterance_lattice_faster(g, rcfg, ref.score_fn(r["loglikes"], r["pdfs"], id2pdf, 0.1), len(u[2]), True)
        assert r["status"] == 1 and want["succeeded"] and not want["partial"]
        assert (r["alignment"], r["words"], r["like"]) == (want["alignment"], want["words"], want["like"])
        errs += dx.edit_distance(u[1], r["words"])
        nref += len(u[1])
    assert errs <= 0.05 * nref, (errs, nref)
    # the reference's three calls (decode.py:143-179) give the batch's answer
    dec = khg.LatticeFasterDecoder(graph, cfg)
    ok, ali, words, like = khg.decode_utterance_lattice_faster(decoder=dec, decodable=khg.DecodableAmDiagGmmScaled(am, tm, feats[0], 0.1),
                                                                trans_model=tm, utt=str(test_utts[0][0]), allow_partial=True)
    assert (ok, ali, words, like) == (True, res[0]["alignment"], res[0]["words"], res[0]["like"])
