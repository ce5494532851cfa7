"""One decoding graph resident in HBM, shared by many utterances (khg_graph_create / khg_utts_create_on_graph / DecodingGraph):
  1. the shared path gives the answers of the replicated path (U copies of the graph through khg_utts_create), which the other
     test files pin to the restatements and the oracle -- every comparison exact, `==` on the bits of every score;
  2. graphs beyond the aligner's limits (more than 254 arcs into a state, more than 65 535 states) are still refused by the
     list-of-graphs path, decode on the shared path as the restatements of the reference say, and make khg_align return
     KHG_E_UNSUPPORTED while the set stays usable;
  3. the cooperative (hub) form of k2_lattice_simple gives the serial loop's outputs, error cases included;
  4. sharing: graph bytes, two live sets on one graph, a set outliving its graph handle, a graph of another context."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_simple_ref as sref  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402

pytestmark = pytest.mark.gpu

LAT_SUCCEEDED, LAT_SCRATCH, LAT_NO_EPS_TOKEN, LAT_NAN = 1, 4, 128, 256
BEAMS = [(13.0, 6.0), (6.0, 2.0), (16.0, 10.0)]
LENS37 = [24, 25, 26, 50] + [20 + (7 * i) % 41 for i in range(33)]


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _gpu, synth
    from kaldi_hmm_gmm_amd import _kaldi_hmm_gmm_amd as ext
    e = Env()
    e.khg, e.synth = khg, synth
    e.m = synth.make_model(30, 4, 12, seed=11)
    e.am, e.tm = synth.host_objects(e.m)
    e.ut = synth.make_utts(e.m, 24, seed=5, min_phones=8, max_phones=20)
    e.ctx = _gpu.default_context()

    def device_model(m):
        gc, bad = ext.compute_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
        assert bad == 0
        return khg.DeviceModel(e.ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    e.dm = device_model(e.m)
    e.mm = synth.mismatched_model(e.m, 0.5, seed=3)
    e.dm_mis = device_model(e.mm)
    e.dtm = khg.DeviceTransitions(e.ctx, e.m.id2pdf)
    assert (np.asarray(e.mm.id2pdf) == np.asarray(e.m.id2pdf)).all()
    return e


def _fst(khg, g):
    return khg.StdVectorFst.from_csr(int(g["start"]), np.asarray(g["arc_off"], np.int64), np.asarray(g["ilabel"], np.int32),
                                     np.asarray(g["olabel"], np.int32), np.asarray(g["weight"], np.float32),
                                     np.asarray(g["nextstate"], np.int32), np.asarray(g["final"], np.float32))


def _feats(ut, lens):
    out = []
    n0 = len(ut.frame_off) - 1
    for u, T in enumerate(lens):
        f = ut.feats[ut.frame_off[u % n0]: ut.frame_off[u % n0 + 1]]
        out.append(np.ascontiguousarray(np.concatenate([f] * (T // len(f) + 1))[:T], np.float32))
    return out


def _flat(feats):
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    return fo, np.ascontiguousarray(np.concatenate(feats), np.float32)


def _pair(e, g, feats):
    """(replicated set, shared set, graph handle) of the same utterances on the same graph."""
    fo, allf = _flat(feats)
    rep = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graphs=tg.concat([g] * len(feats)))
    dg = e.khg.DecodingGraph(_fst(e.khg, g), e.dtm)
    sh = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    return rep, sh, dg


def _same(a, b, what):
    """Exact equality of two result dicts / arrays / lists of arrays: the bits of every float."""
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], what + "." + k)
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert a.tobytes() == b.tobytes(), what


def _kind_graph(e, kind):
    rng = np.random.default_rng({"random": 1, "hub": 2, "loop200": 3}[kind])
    if kind == "random":
        return tg.random_graph(rng, e.m.num_tids, n_main=12, p_eps=0.4)
    if kind == "hub":
        return tg.hub_graph(rng, e.m.num_tids, fan=8, tail=5)
    return sg.word_loop_graph(rng, e.m.num_tids, 200)


def _align_graph(e, kind):
    """More states than min_active (20): with a narrow beam the exact DP's beam certificate fails and the order-faithful decoders decide."""
    rng = np.random.default_rng({"random": 11, "hub": 12, "loop200": 13}[kind])
    if kind == "random":
        return tg.random_graph(rng, e.m.num_tids, n_main=48, p_eps=0.3)
    if kind == "hub":
        return tg.hub_graph(rng, e.m.num_tids, fan=20, tail=6)
    return sg.word_loop_graph(rng, e.m.num_tids, 200)


def _random_scores(us, seed):
    """Scores with no structure (every path about as good as the next): a narrow beam really prunes."""
    off, _ = us.pdf_lists()
    rng = np.random.default_rng(seed)
    fo = np.asarray(us.frame_off)
    return [(-8 * rng.random((int(off[u + 1] - off[u]), int(fo[u + 1] - fo[u])))).astype(np.float32) for u in range(us.n_utt)]


def _scores_from(e, us, first_only):
    """The resident scores; with first_only the cells before a pdf's first readable frame (which the reachable / band forms of K1
    leave unwritten) are masked."""
    mats = us.download_loglikes()
    if first_only:
        off, _ = us.pdf_lists()
        first = us.pdf_first_frames()
        for u, m in enumerate(mats):
            for j in range(m.shape[0]):
                m[j, : min(int(first[off[u] + j]), m.shape[1])] = 0.0
    return mats


# ---- 1. the shared path gives the replicated path's answers -----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "hub", "loop200"])
def test_loglikes_forms_and_pdf_tables(env, kind):
    e = env
    rep, sh, dg = _pair(e, _kind_graph(e, kind), _feats(e.ut, LENS37))
    assert sh.graph_bytes == 0 and rep.graph_bytes > 0
    _same(rep.pdf_lists(), sh.pdf_lists(), "pdf_lists")
    _same(rep.pdf_first_frames(), sh.pdf_first_frames(), "pdf_first")
    _same(rep.pdf_last_frames(), sh.pdf_last_frames(), "pdf_last")
    _same(rep.loglikes_layout(), sh.loglikes_layout(), "layout")
    for mode in ({}, {"reachable_only": True}, {"band": True}):
        rep.loglikes(e.dm, **mode); sh.loglikes(e.dm, **mode)
        _same(_scores_from(e, rep, bool(mode)), _scores_from(e, sh, bool(mode)), "loglikes %r" % mode)
    for s in (rep, sh, dg):
        s.close()


@pytest.mark.parametrize("kind", ["random", "hub", "loop200"])
def test_align_and_acc_stats(env, kind):
    e = env
    rep, sh, dg = _pair(e, _align_graph(e, kind), _feats(e.ut, LENS37))
    n_fallback = 0
    for dm, cfg in ((e.dm, dict(beam=200.0, acoustic_scale=0.1)), (e.dm_mis, dict(beam=6.0, retry_beam=40.0, acoustic_scale=0.1)),
                    (e.dm_mis, dict(beam=6.0, retry_beam=40.0, acoustic_scale=1.0)),
                    (None, dict(beam=0.8, retry_beam=4.0)), (None, dict(beam=2.5))):
        out = []
        for s in (rep, sh):
            if dm is None:                     # uploaded scores (K3 below reads the features under the true model)
                s.upload_loglikes(_random_scores(s, 5))
            else:
                s.loglikes(dm, reachable_only=True)
            r = s.align(e.dtm, **cfg)
            accs = e.khg.DeviceAccs(e.ctx, dm or e.dm, e.dtm)
            s.acc_stats(dm or e.dm, e.dtm, accs)
            out.append((r, accs.download()))
            accs.close()
        _same(out[0], out[1], "align %r" % cfg)
        n_fallback += int(((out[0][0]["status"] & e.khg.ALIGN_FALLBACK) != 0).sum())
    if kind != "loop200":
        assert n_fallback > 0          # the order-faithful decoders ran (narrow beams)
    for s in (rep, sh, dg):
        s.close()


def test_align_split_mode_on_more_than_64_utterances(env):
    e = env
    lens = [24, 25, 26, 50] + [20 + (5 * i) % 37 for i in range(80)]
    rep, sh, dg = _pair(e, _align_graph(e, "random"), _feats(e.ut, lens))
    for uploaded, cfg in ((False, dict(beam=6.0, retry_beam=40.0, acoustic_scale=0.1)), (True, dict(beam=0.8, retry_beam=4.0))):
        out = []
        for s in (rep, sh):
            if uploaded:
                s.upload_loglikes(_random_scores(s, 6))
            else:
                s.loglikes(e.dm_mis, reachable_only=True)
            assert s.align(e.dtm, download=False, **cfg) is None       # asynchronous, more than 64 utterances: split mode
            accs = e.khg.DeviceAccs(e.ctx, e.dm_mis, e.dtm)
            s.acc_stats(e.dm_mis, e.dtm, accs)
            out.append((s.download_ali(), accs.download(), s.align(e.dtm, download="summary", **cfg)))
            accs.close()
        _same(out[0], out[1], "split mode %r" % cfg)
        assert (out[0][0] != 0).any()
        if uploaded:
            assert ((out[0][2]["status"] & e.khg.ALIGN_FALLBACK) != 0).any()       # the order-faithful decoders ran
    for s in (rep, sh, dg):
        s.close()


@pytest.mark.parametrize("kind", ["random", "hub", "loop200"])
@pytest.mark.parametrize("decoder", ["faster", "simple0", "simple25"])
def test_lattice_decoders(env, kind, decoder):
    e = env
    g = _kind_graph(e, kind)
    if decoder != "faster":
        g = sref.add_eps_self_loops(g, 0.0 if decoder == "simple0" else 0.25)
    rep, sh, dg = _pair(e, g, _feats(e.ut, LENS37))
    n_ok = 0
    for s in (rep, sh):
        s.loglikes(e.dm)
    for beam, lbeam in BEAMS:
        if decoder == "faster":
            a, b = (s.decode_lattice_faster(e.dtm, beam=beam, lattice_beam=lbeam, acoustic_scale=0.1) for s in (rep, sh))
        else:
            a, b = (s.decode_lattice_simple(e.dtm, beam=beam, lattice_beam=lbeam, acoustic_scale=0.1) for s in (rep, sh))
        _same(a, b, "%s %r" % (decoder, (beam, lbeam)))
        n_ok += int(((a["status"] & LAT_SUCCEEDED) != 0).sum())
    assert n_ok > 0
    for s in (rep, sh, dg):
        s.close()


def test_one_utterance_and_the_batch_calls(env):
    """U = 1 (scratch from the context's arena), and the batch entry points: one StdVectorFst, a list of one and a DecodingGraph run
    on the shared path and return what a list of U graphs returns."""
    e, khg = env, env.khg
    g = sref.add_eps_self_loops(_kind_graph(e, "hub"), 0.25)
    rep, sh, dg = _pair(e, g, _feats(e.ut, [33]))
    for s in (rep, sh):
        s.loglikes(e.dm)
    _same(rep.decode_lattice_simple(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1),
          sh.decode_lattice_simple(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1), "U = 1 simple")
    _same(rep.decode_lattice_faster(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1),
          sh.decode_lattice_faster(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1), "U = 1 faster")
    for s in (rep, sh, dg):
        s.close()
    g_plain = _kind_graph(e, "hub")
    rep, sh, dg = _pair(e, g_plain, _feats(e.ut, [33]))
    for s in (rep, sh):
        s.loglikes(e.dm, reachable_only=True)
    _same(rep.align(e.dtm, acoustic_scale=0.1), sh.align(e.dtm, acoustic_scale=0.1), "U = 1 align")
    for s in (rep, sh, dg):
        s.close()
    feats = _feats(e.ut, LENS37[:9])
    fst = _fst(khg, g)
    hdg = khg.DecodingGraph(fst, e.tm)                 # a host TransitionModel: its device table on the default context
    assert (hdg.num_states, hdg.num_arcs) == (len(g["final"]), len(g["ilabel"]))
    scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    fcfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    want_s = khg.decode_lattice_simple_batch(e.am, e.tm, [fst] * len(feats), feats, scfg, 0.1, return_scores=True)
    want_f = khg.decode_lattice_faster_batch(e.am, e.tm, [fst] * len(feats), feats, fcfg, 0.1, return_scores=True)
    fst_a = _fst(khg, g_plain)
    adg = khg.DecodingGraph(fst_a, e.tm)
    want_a = khg.align_batch(e.am, e.tm, [fst_a] * len(feats), feats, khg.AlignConfig(), 0.1, return_scores=True)
    assert any(r["succeeded"] for r in want_s) and any(r["succeeded"] for r in want_f) and any(r["ok"] for r in want_a)
    for one, one_a in ((fst, fst_a), ([fst], [fst_a]), (hdg, adg)):
        _same(want_s, khg.decode_lattice_simple_batch(e.am, e.tm, one, feats, scfg, 0.1, return_scores=True), "simple batch")
        _same(want_f, khg.decode_lattice_faster_batch(e.am, e.tm, one, feats, fcfg, 0.1, return_scores=True), "faster batch")
        _same(want_a, khg.align_batch(e.am, e.tm, one_a, feats, khg.AlignConfig(), 0.1, return_scores=True), "align batch")
    hdg.close(); adg.close()


def test_compiled_word_loop_graph(env):
    """TrainingGraphCompiler.compile_word_loop_graph on the trained monophone model of examples/decode_synthetic.py: 40 held-out
    utterances on one shared graph against 40 copies of it."""
    khg = env.khg
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import decode_synthetic as dx
    from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions
    args = types.SimpleNamespace(utts=200, test_utts=40, iters=80, dim=23, seed=3)
    tm, tree, am, lexicon, test_utts = dx.train(args, log=lambda *a: None)
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                  opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gcomp.compile_word_loop_graph()
    feats = [u[2] for u in test_utts]
    assert len(feats) >= 37
    fcfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    a = khg.decode_lattice_faster_batch(am, tm, [graph] * len(feats), feats, fcfg, 0.1, return_scores=True)
    b = khg.decode_lattice_faster_batch(am, tm, graph, feats, fcfg, 0.1, return_scores=True)
    _same(a, b, "faster")
    assert all(r["succeeded"] for r in a)
    c = graph.to_csr()
    gl = _fst(khg, sref.add_eps_self_loops(c, 0.25))
    scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    a = khg.decode_lattice_simple_batch(am, tm, [gl] * len(feats), feats, scfg, 0.1, return_scores=True)
    b = khg.decode_lattice_simple_batch(am, tm, gl, feats, scfg, 0.1, return_scores=True)
    _same(a, b, "simple")
    assert all(r["succeeded"] for r in a)
    a = khg.align_batch(am, tm, [graph] * len(feats), feats, khg.AlignConfig(), 0.1)
    b = khg.align_batch(am, tm, graph, feats, khg.AlignConfig(), 0.1)
    _same(a, b, "align")
    assert all(r["ok"] for r in a)


# ---- 2. beyond the aligner's limits -----------------------------------------------------------------------------------------
BIG = {"W300": (300, 1, [40, 60, 24, 25, 26, 50, 33, 47], "more than 254 incoming arcs"),
       "W3000": (3000, 1, [40, 30], "more than 254 incoming arcs"),
       "S66001": (sg.BIG_W, sg.BIG_CHAIN, [40, 26], "more than 65535 states")}


def _path_feats(e, g, words, T, seed):
    """Features sampled from the model along a path of the word loop `g` through `words` that takes exactly T frames (every arc of
    each word once, self-loops dealt round-robin for the rest): the graph accepts them inside any beam.  Words of ten states on
    unrelated features do not reach the final state within beam 13, which leaves nothing to compare."""
    ao, il, ns = np.asarray(g["arc_off"]), np.asarray(g["ilabel"]), np.asarray(g["nextstate"])
    steps = []                                   # (tid of the arc taken, tid of the self-loop of the state it enters or 0)
    for w in words:
        a = int(ao[0]) + w
        s = int(ns[a])
        steps.append([int(il[a]), 0])
        while s != 0:
            loop, fwd = int(ao[s]), int(ao[s]) + 1          # word_loop_graph: [self-loop, forward] on every chain state
            assert int(ns[loop]) == s
            steps[-1][1] = int(il[loop])
            steps.append([int(il[fwd]), 0])
            s = int(ns[fwd])
    extra = T - len(steps)
    assert extra >= 0
    loops = [i for i, st in enumerate(steps) if st[1]]
    reps = [0] * len(steps)
    for k in range(extra):
        reps[loops[k % len(loops)]] += 1
    tids = []
    for (tid, loop), n in zip(steps, reps):
        tids += [tid] + [loop] * n
    assert len(tids) == T
    frame_pdf = np.asarray(e.m.id2pdf)[np.asarray(tids)].astype(np.int32)
    return np.ascontiguousarray(e.synth.sample_feats(e.m, frame_pdf, np.random.default_rng(seed)), np.float32)


@pytest.fixture(scope="module")
def big(env):
    """The three graphs over the old limits, decoded by both lattice decoders on the shared path (K1's scores returned), and the
    restatements of the same utterances on those scores -- computed once, in worker processes, for the tests below."""
    e, khg = env, env.khg
    out, jobs, keys = {}, [], []
    for name, (W, chain, lens, _) in BIG.items():
        g = sg.word_loop_graph(np.random.default_rng(W), e.m.num_tids, W, chain)
        gl = sref.add_eps_self_loops(g, 0.25)
        if chain > 1:
            feats = [_path_feats(e, g, [17 + 5 * u, 4000 + u], T, 100 + u) for u, T in enumerate(lens)]
        else:
            feats = _feats(e.ut, lens)
        fcfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
        scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
        rf = khg.decode_lattice_faster_batch(e.am, e.tm, _fst(khg, g), feats, fcfg, 0.1, return_scores=True)
        rs = khg.decode_lattice_simple_batch(e.am, e.tm, _fst(khg, gl), feats, scfg, 0.1, return_scores=True)
        out[name] = dict(g=g, gl=gl, feats=feats, faster=rf, simple=rs)
        for u, T in enumerate(lens):
            jobs.append(dict(kind="faster", graph=g, cfg=dict(sg.FASTER_CFG, max_active=7000), T=T,
                             k1=(rf[u]["loglikes"], rf[u]["pdfs"], np.asarray(e.m.id2pdf), 0.1))); keys.append((name, "want_faster", u))
            jobs.append(dict(kind="simple", graph=gl, cfg=sg.SIMPLE_CFG, T=T,
                             k1=(rs[u]["loglikes"], rs[u]["pdfs"], np.asarray(e.m.id2pdf), 0.1))); keys.append((name, "want_simple", u))
    # the slow ones first
    order = sorted(range(len(jobs)), key=lambda i: -len(jobs[i]["graph"]["ilabel"]) * jobs[i]["T"] * (3 if jobs[i]["kind"] == "simple" else 1))
    res = sg.restate_many([jobs[i] for i in order])
    for i, r in zip(order, res):
        name, what, u = keys[i]
        out[name].setdefault(what, {})[u] = r
    return out


@pytest.mark.parametrize("name", list(BIG))
def test_beyond_the_limits_decodes_as_the_restatements(env, big, name):
    b = big[name]
    assert sg.max_in_degree(b["g"]) > 254
    stats = {"nonzero_extra": 0, "excised": 0}
    for u in range(len(b["feats"])):
        r, want = b["faster"][u], b["want_faster"][u]
        assert want["succeeded"] and not want["partial"], (name, u)
        assert (r["succeeded"], r["partial"], r["alignment"], r["words"], r["like"]) == \
               (want["succeeded"], want["partial"], want["alignment"], want["words"], want["like"]), (name, u)
        r, want = b["simple"][u], b["want_simple"][u]
        assert "error" not in want and want["succeeded"], (name, u, want)
        assert (r["succeeded"], r["alignment"], r["words"], r["like"], r["status"], r["error_frame"]) == \
               (True, want["alignment"], want["words"], want["like"], LAT_SUCCEEDED, -1), (name, u)
        for k in stats:
            stats[k] += want["stats"][k]
    assert stats["nonzero_extra"] > 0 and stats["excised"] > 0, stats


@pytest.mark.parametrize("name", list(BIG))
def test_beyond_the_limits_list_path_and_align(env, big, name):
    e, khg, b = env, env.khg, big[name]
    msg = BIG[name][3]
    feats = b["feats"][:2]
    fst = _fst(khg, b["g"])
    fcfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    # one graph per utterance: khg_utts_create keeps both checks and both messages
    with pytest.raises(khg.KhgError, match="khg_utts_create: .*" + msg):
        khg.decode_lattice_faster_batch(e.am, e.tm, [fst, fst], feats, fcfg, 0.1)
    fo, allf = _flat(feats)
    with pytest.raises(khg.KhgError, match="khg_utts_create: .*" + msg):
        khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graphs=tg.concat([b["g"]] * 2))
    # the shared set: the aligner names its limit and leaves the set usable
    dg = khg.DecodingGraph(fst, e.dtm)
    assert dg.max_in_degree == sg.max_in_degree(b["g"]) and dg.num_states == len(b["g"]["final"])
    us = khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    us.loglikes(e.dm)
    with pytest.raises(khg.KhgError, match="khg_align: .*" + msg):
        us.align(e.dtm, acoustic_scale=0.1)
    with pytest.raises(khg.KhgError, match="khg_align: .*" + msg):
        khg.align_batch(e.am, e.tm, fst, feats, khg.AlignConfig(), 0.1)
    r = us.decode_lattice_faster(e.dtm, beam=13.0, max_active=7000, lattice_beam=6.0, acoustic_scale=0.1)
    for u in range(2):
        want = b["faster"][u]
        assert int(r["status"][u]) & LAT_SUCCEEDED
        assert r["ali"][fo[u]: fo[u + 1]].tolist() == want["alignment"] and float(r["like"][u]) == want["like"]
        assert r["words"][r["words_off"][u]: r["words_off"][u + 1]].tolist() == want["words"]
    us.close(); dg.close()


# ---- 3. the hub form of k2_lattice_simple --------------------------------------------------------------------------------------
def _hub_modes(e, us, **kw):
    """decode_lattice_simple with the cooperative form off, at its default threshold and for every state: identical outputs."""
    default = e.ctx.get_option("k2s_hub")
    assert default > 0
    outs = []
    try:
        for thr in (0, default, 1):
            e.ctx.set_option("k2s_hub", thr)
            outs.append(us.decode_lattice_simple(e.dtm, acoustic_scale=0.1, **kw))
    finally:
        e.ctx.set_option("k2s_hub", default)
    _same(outs[0], outs[1], "hub off / default")
    _same(outs[0], outs[2], "hub off / every state")
    return outs[0]


@pytest.mark.parametrize("kind", ["random", "hub", "loop200"])
@pytest.mark.parametrize("loop_w", [0.0, 0.25])
def test_hub_form_small_graphs(env, kind, loop_w):
    e = env
    g = sref.add_eps_self_loops(_kind_graph(e, kind), loop_w)
    fo, allf = _flat(_feats(e.ut, LENS37))
    dg = e.khg.DecodingGraph(_fst(e.khg, g), e.dtm)
    us = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    us.loglikes(e.dm)
    n_ok = 0
    for beam, lbeam in BEAMS:
        r = _hub_modes(e, us, beam=beam, lattice_beam=lbeam)
        n_ok += int(((r["status"] & LAT_SUCCEEDED) != 0).sum())
    assert n_ok > 0
    us.close(); dg.close()


@pytest.mark.parametrize("name", list(BIG))
def test_hub_form_beyond_the_limits(env, big, name):
    e, b = env, big[name]
    fo, allf = _flat(b["feats"])
    dg = e.khg.DecodingGraph(_fst(e.khg, b["gl"]), e.dtm)
    us = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    us.loglikes(e.dm)
    r = _hub_modes(e, us, beam=13.0, lattice_beam=6.0)
    for u, want in enumerate(b["simple"]):           # ... and they are the batch call's, which test 2 pins to the restatement
        assert int(r["status"][u]) == LAT_SUCCEEDED
        assert r["ali"][fo[u]: fo[u + 1]].tolist() == want["alignment"] and float(r["like"][u]) == want["like"]
        assert r["words"][r["words_off"][u]: r["words_off"][u + 1]].tolist() == want["words"]
    us.close(); dg.close()


def test_hub_form_error_cases(env, big):
    e, b = env, big["W300"]
    g, gl = b["g"], b["gl"]
    fo, allf = _flat(b["feats"])
    # KHG_LAT_NAN: a NaN in the resident scores of an arc into the hub (s_w -> 0), at a frame where its source holds a token
    dg = e.khg.DecodingGraph(_fst(e.khg, gl), e.dtm)
    us = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    us.loglikes(e.dm)
    mats = us.download_loglikes()
    off, pdfs = us.pdf_lists()
    into_hub = set(np.asarray(gl["ilabel"])[(np.asarray(gl["nextstate"]) == 0) & (np.asarray(gl["ilabel"]) > 0)].tolist())
    for u in (0, 3):
        ali = b["simple"][u]["alignment"]
        t = len(ali) - 1                    # the loop state is the only final state: the best path's last arc goes into the hub
        assert ali[t] in into_hub
        j = pdfs[off[u]: off[u + 1]].tolist().index(int(e.m.id2pdf[ali[t]]))
        mats[u][j, t] = np.nan
    us.upload_loglikes(mats)
    r = _hub_modes(e, us, beam=13.0, lattice_beam=6.0)
    assert int(r["status"][0]) == LAT_NAN and int(r["status"][3]) == LAT_NAN and int(r["status"][1]) == LAT_SUCCEEDED
    # KHG_LAT_SCRATCH: fewer tokens allowed on a frame than the word loop holds
    us.loglikes(e.dm)
    r = _hub_modes(e, us, beam=13.0, lattice_beam=6.0, scratch_per_frame=5)
    assert (r["status"] == LAT_SCRATCH).all()
    us.close(); dg.close()
    # KHG_LAT_NO_EPS_TOKEN: no input-epsilon arc anywhere (Quirk 1 at frame -1)
    dg = e.khg.DecodingGraph(_fst(e.khg, g), e.dtm)
    us = e.khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg)
    us.loglikes(e.dm)
    r = _hub_modes(e, us, beam=13.0, lattice_beam=6.0)
    assert (r["status"] == LAT_NO_EPS_TOKEN).all() and (r["error_frame"] == -1).all()
    us.close(); dg.close()


# ---- 4. sharing ---------------------------------------------------------------------------------------------------------------
def test_sharing_and_lifetime(env):
    e, khg = env, env.khg
    g = sref.add_eps_self_loops(_kind_graph(e, "loop200"), 0.25)
    S, A = len(g["final"]), len(g["ilabel"])
    feats = _feats(e.ut, LENS37)
    fo, allf = _flat(feats)
    rep, sh, dg = _pair(e, g, feats)
    # the graph's tables do not depend on how many utterances decode on it; a replicated set pays them per utterance
    assert dg.device_bytes == 8 * 2 + 4 + 16 * (S + 1) + 24 * A + 4 * S
    assert (dg.num_states, dg.num_arcs, dg.max_in_degree) == (S, A, 201)
    assert sh.graph_bytes == 0
    assert rep.graph_bytes >= len(feats) * (16 * S + 24 * A + 4 * S)
    fo2, allf2 = _flat(feats[:5])
    sh2 = khg.UtteranceSet(e.ctx, e.dtm, fo2, allf2, graph=dg)           # two live sets on one graph
    assert sh2.graph_bytes == 0
    dg.close()                                                            # ... which both outlive its handle
    dg.close()
    for s in (rep, sh, sh2):
        s.loglikes(e.dm)
    want = rep.decode_lattice_simple(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    got = sh.decode_lattice_simple(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    _same(want, got, "after the handle was closed")
    sh.close()
    got2 = sh2.decode_lattice_simple(e.dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)      # the last holder
    assert got2["ali"].tolist() == want["ali"][: fo2[-1]].tolist() and got2["like"].tobytes() == want["like"][:5].tobytes()
    assert (got2["status"] == want["status"][:5]).all() and int((got2["status"] & LAT_SUCCEEDED).sum()) > 0
    sh2.close(); rep.close()
    with pytest.raises(khg.KhgError, match="closed"):
        khg.decode_lattice_simple_batch(e.am, e.tm, dg, feats[:2], khg.LatticeSimpleDecoderConfig(), 0.1)
    with pytest.raises(ValueError):
        khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graphs=tg.concat([g] * len(feats)), graph=dg)
    # a graph belongs to the context that created it
    ctx2 = khg.Context(e.ctx.device)
    dtm2 = khg.DeviceTransitions(ctx2, e.m.id2pdf)
    dg2 = khg.DecodingGraph(_fst(khg, g), dtm2)
    with pytest.raises(khg.KhgError, match="context that created it"):
        khg.UtteranceSet(e.ctx, e.dtm, fo, allf, graph=dg2)
    ok = khg.UtteranceSet(ctx2, dtm2, fo2, allf2, graph=dg2)
    ok.close(); dg2.close(); dtm2.close(); ctx2.close()
