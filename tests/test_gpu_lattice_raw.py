"""The raw lattice of the data-parallel lattice-simple decoder on the GPU (khg_decode_lattice_simple_raw through
get_raw_lattice_simple_batch / UtteranceSet.raw_lattice_simple) against the float32 restatement of its rule
(tests/lattice_raw_ref.py), bit for bit: every state field, every arc field and their orders.  Scores come from
K1 (return_scores=True), so only the emission is compared.  Inputs as in tests/test_gpu_lattice_simple.py and
tests/test_gpu_shared_graph.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_raw_ref as raw  # noqa: E402
import lattice_simple_ref as ref  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402

pytestmark = pytest.mark.gpu

LAT_SUCCEEDED, LAT_SCRATCH, LAT_NO_PATH, LAT_EPS_LOOP, LAT_NO_EPS_TOKEN, LAT_NAN = 1, 4, 8, 16, 128, 256
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")
OLD_KEYS = ("succeeded", "partial", "status", "alignment", "words", "like", "num_frames", "error_frame")


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


def _same_lattice(lat, want, tag):
    """A khg.Lattice (or a dict of arrays with arc_begin one longer) against rule_lattice's arrays: dtype, length, every bit."""
    for k in FIELDS:
        got = np.asarray(lat[k] if isinstance(lat, dict) else getattr(lat, k))
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, (tag, k, got.shape, want[k].shape)
        assert got.tobytes() == want[k].tobytes(), (tag, k)
    assert (lat["start"] if isinstance(lat, dict) else lat.start) == want["start"], tag


class Evidence:
    def __init__(self):
        self.excised = self.nonzero_extra = self.multi_path = self.compared = self.states = self.arcs = 0

    def add(self, want):
        self.compared += 1
        self.excised += want["excised"]
        self.nonzero_extra += int((want["extra_cost"] != 0.0).sum())
        self.multi_path += bool(want["paths_gt_1"])
        self.states += len(want["frame"])
        self.arcs += len(want["ilabel"])

    def __repr__(self):
        return "compared %d states %d arcs %d excised %d nonzero_extra %d multi_path %d" % (
            self.compared, self.states, self.arcs, self.excised, self.nonzero_extra, self.multi_path)


def _check(khg, m, am, tm, graphs, fsts, feats, beam, lbeam, ev, scale=0.1, scratch=0):
    """graphs: the graph dict of every utterance; fsts: what the batch calls take (a list, one StdVectorFst or a DecodingGraph)."""
    cfg = khg.LatticeSimpleDecoderConfig(beam=beam, lattice_beam=lbeam)
    rcfg = ref.Config(beam=beam, lattice_beam=lbeam)
    old = khg.decode_lattice_simple_batch(am, tm, fsts, feats, cfg, scale, scratch_per_frame=scratch)     # the unchanged call
    res = khg.get_raw_lattice_simple_batch(am, tm, fsts, feats, cfg, scale, scratch_per_frame=scratch, return_scores=True)
    assert len(res) == len(old) == len(feats)
    for u, (g, r, o) in enumerate(zip(graphs, res, old)):
        assert set(o) == set(OLD_KEYS) and set(r) == set(OLD_KEYS) | {"lattice", "loglikes", "pdfs"}
        for k in OLD_KEYS:
            assert r[k] == o[k] and type(r[k]) is type(o[k]), (u, k)
        lat = r["lattice"]
        assert isinstance(lat, khg.Lattice)
        want = raw.rule_lattice(ref.Graph.from_dict(g), rcfg, ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, scale), len(feats[u]))
        if not r["succeeded"]:
            assert want is None or scratch > 0, (u, r["status"])
            assert lat.num_states == 0 and lat.num_arcs_total == 0 and lat.start == -1 and list(lat.arc_begin) == [0], u
            continue
        assert want is not None, u
        _same_lattice(lat, want, u)
        ev.add(want)
        # the decoder's best path is the lattice's: ShortestPath by the same tie rule gives it back, bit for bit
        lin = lat.shortest_path()
        ok, ali, words, _ = lin.get_linear_symbol_sequence()
        assert ok and ali == r["alignment"] and words == r["words"], u
        assert raw.path_like(lin) == r["like"], (u, raw.path_like(lin), r["like"])
        at = {lat.start}
        for a in lin.arcs:           # ... and every one of its arcs is an arc of the lattice, from the start to a final state
            key = (a.ilabel, a.olabel, a.weight.value1, a.weight.value2)
            at = {b.nextstate for s in at for b in lat.arcs(s) if (b.ilabel, b.olabel, b.weight.value1, b.weight.value2) == key}
            assert at, u
        assert any(lat.final(s).value1 == lin.final.value1 for s in at) and len(lin.arcs) >= len(feats[u]), u
    return res


@pytest.mark.parametrize("kind", ["random", "hub"])
@pytest.mark.parametrize("loop_w", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("beams", [(13.0, 6.0), (6.0, 2.0), (16.0, 4.0), (8.0, 1.0)])
def test_graphs_with_self_loops(setup, kind, loop_w, beams):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(int(beams[0] * 10 + beams[1] + 100 * loop_w) + (3 if kind == "hub" else 0))
    n = 6
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if kind == "random"
                                 else tg.hub_graph(rng, m.num_tids, fan=8, tail=5), loop_w) for _ in range(n)]
    ev = Evidence()
    _check(khg, m, am, tm, gs, [_fst(khg, g) for g in gs], _feats(ut, n), *beams, ev)
    print(ev)
    assert ev.compared > 0
    if loop_w > 0.0:
        assert ev.excised > 0 and ev.nonzero_extra > 0, ev
    if loop_w > 0.0 and beams[1] >= 4.0:
        assert ev.multi_path > 0, ev


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(setup, T):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(T)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.3), 0.25) for _ in range(4)]
    ev = Evidence()
    _check(khg, m, am, tm, gs, [_fst(khg, g) for g in gs], _feats(ut, 4, [T] * 4), 10.0, 4.0, ev)
    assert ev.compared > 0, ev


def test_mismatched_model(setup):
    khg, synth, m, am, tm, ut = setup
    mm = synth.mismatched_model(m, 0.5, seed=3)
    am2, tm2 = synth.host_objects(mm)
    rng = np.random.default_rng(9)
    gs = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=10, p_branch=0.6, p_eps=0.3), 0.25) for _ in range(8)]
    ev = Evidence()
    _check(khg, mm, am2, tm2, gs, [_fst(khg, g) for g in gs], _feats(ut, 8), 6.0, 2.0, ev)
    assert ev.compared > 0, ev


def test_large_graph_batch_equals_single_and_one_utterance(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(1234)
    g = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=1100, p_eps=0.2), 0.25)
    small = [ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=9, p_eps=0.3), 0.25) for _ in range(3)]
    gs = [g, small[0], g, small[1], small[2]]
    feats = _feats(ut, 5, [60, 30, 40, 20, 25])
    ev = Evidence()
    res = _check(khg, m, am, tm, gs, [_fst(khg, x) for x in gs], feats, 13.0, 6.0, ev)
    print(ev)
    assert ev.compared >= 3 and ev.excised > 0 and ev.nonzero_extra > 0 and ev.multi_path > 0, ev
    # a batch is its one-utterance batches (U = 1)
    cfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
    for u in range(len(gs)):
        one = khg.get_raw_lattice_simple_batch(am, tm, [_fst(khg, gs[u])], feats[u: u + 1], cfg, 0.1)
        assert len(one) == 1 and set(one[0]) == set(OLD_KEYS) | {"lattice"}
        for k in OLD_KEYS:
            assert one[0][k] == res[u][k], (u, k)
        for k in FIELDS:
            assert getattr(one[0]["lattice"], k).tobytes() == getattr(res[u]["lattice"], k).tobytes(), (u, k)
        assert one[0]["lattice"].start == res[u]["lattice"].start
        assert one[0]["lattice"].to_text() == res[u]["lattice"].to_text()


def test_decoding_graph_300_word_loop_at_every_hub_threshold(setup):
    """One DecodingGraph (a loop state with 300 out-arcs: over every threshold but 0) shared by the batch; the hub form off, for
    every state and at the default threshold: the same arrays, and the rule's."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    g = ref.add_eps_self_loops(sg.word_loop_graph(np.random.default_rng(300), m.num_tids, 300, 1), 0.25)
    lens = [40, 24, 25, 26]
    feats = _feats(ut, len(lens), lens)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    default = ctx.get_option("k2s_hub")
    assert default == 32
    ev = Evidence()
    outs = []
    try:
        for thr in (0, 1, 32):
            ctx.set_option("k2s_hub", thr)
            if thr == 0:
                outs.append(_check(khg, m, am, tm, [g] * len(lens), dg, feats, 13.0, 6.0, ev))
            else:
                outs.append(khg.get_raw_lattice_simple_batch(am, tm, dg, feats, khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0), 0.1))
    finally:
        ctx.set_option("k2s_hub", default)
    print(ev)
    assert ev.compared == len(lens) and ev.excised > 0 and ev.nonzero_extra > 0 and ev.multi_path > 0, ev
    for other in outs[1:]:
        for u in range(len(lens)):
            for k in OLD_KEYS:
                assert other[u][k] == outs[0][u][k], (u, k)
            for k in FIELDS:
                assert getattr(other[u]["lattice"], k).tobytes() == getattr(outs[0][u]["lattice"], k).tobytes(), (u, k)
            assert other[u]["lattice"].start == outs[0][u]["lattice"].start
    # a single StdVectorFst is shared the same way
    one = khg.get_raw_lattice_simple_batch(am, tm, _fst(khg, g), feats, khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0), 0.1)
    for u in range(len(lens)):
        for k in FIELDS:
            assert getattr(one[u]["lattice"], k).tobytes() == getattr(outs[0][u]["lattice"], k).tobytes(), (u, k)
    dg.close()


def test_failing_statuses_give_empty_lattices(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(5)
    base = tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.0)                  # no epsilon arc anywhere: Quirk 1 at frame -1
    nofinal = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6, with_final=False))
    good = ref.add_eps_self_loops(tg.random_graph(rng, m.num_tids, n_main=6))
    later = {k: np.array(v) for k, v in base.items()}                             # an epsilon self-loop on the start only
    n0 = int(later["arc_off"][1])
    for k, v in (("ilabel", 0), ("olabel", 0), ("weight", 0.0), ("nextstate", 0)):
        later[k] = np.insert(later[k], n0, v)
    later["arc_off"] = np.concatenate([[0], np.asarray(later["arc_off"][1:]) + 1]).astype(np.int64)
    loop = {"start": 0, "arc_off": np.array([0, 2, 3], np.int64), "ilabel": np.array([0, 1, 0], np.int32), "olabel": np.zeros(3, np.int32),
            "weight": np.array([-1.0, 0.0, 0.5], np.float32), "nextstate": np.array([1, 0, 0], np.int32), "final": np.array([0.0, np.inf], np.float32)}
    gs = [base, nofinal, good, later, loop]
    feats = _feats(ut, 5)
    ev = Evidence()
    res = _check(khg, m, am, tm, gs, [_fst(khg, g) for g in gs], feats, 13.0, 6.0, ev)
    assert [(r["status"], r["error_frame"]) for r in res] == [(LAT_NO_EPS_TOKEN, -1), (LAT_NO_PATH, -1), (LAT_SUCCEEDED, -1), (LAT_NO_EPS_TOKEN, 0),
                                                             (LAT_EPS_LOOP, -1)]
    assert [r["lattice"].num_states > 0 for r in res] == [False, False, True, False, False]
    # scratch_per_frame: a frame over the limit gets KHG_LAT_SCRATCH and an empty lattice
    res = _check(khg, m, am, tm, [good], [_fst(khg, good)], feats[2:3], 13.0, 6.0, ev, scratch=1)
    assert res[0]["status"] == LAT_SCRATCH and res[0]["lattice"].num_states == 0


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


def _set_lattices(d):
    """UtteranceSet.raw_lattice_simple's flat arrays -> one dict of arrays per utterance (arc_begin one longer, as khg.Lattice)."""
    out = []
    so, ao = d["state_off"], d["arc_off"]
    for u in range(len(so) - 1):
        lat = {k: np.asarray(d[k][so[u]: so[u + 1]]) for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost")}
        lat.update({k: np.asarray(d[k][ao[u]: ao[u + 1]]) for k in ("ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")})
        lat["arc_begin"] = np.concatenate([d["arc_begin"][so[u]: so[u + 1]], [ao[u + 1] - ao[u]]]).astype(np.int32)
        lat["start"] = int(d["start"][u])
        out.append(lat)
    return out


def test_nan_status_on_resident_scores_and_unchanged_decode(setup):
    """The C-ABI call on a set's resident scores: the clean decode's lattice is the rule's; a NaN score (KHG_LAT_NAN) gives an empty
    one, with the status and error frame of khg_decode_lattice_simple."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    pdf = np.asarray(m.id2pdf)
    ta = 1
    tb = next(t for t in range(2, m.num_tids + 1) if pdf[t] != pdf[ta])
    arcs = [(0, 0, 0, 0.0, 0), (0, ta, 0, 0.0, 1), (0, tb, 0, 0.0, 2), (1, 0, 0, 0.25, 1), (2, 0, 0, 0.25, 2), (1, ta, 0, 0.0, 1),
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
    old = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    d = us.raw_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    for k in old:
        assert np.asarray(d[k]).tobytes() == np.asarray(old[k]).tobytes(), k
    assert int(d["status"][0]) == LAT_SUCCEEDED and d["device_bytes"] > 0
    mats = [np.array(x, np.float32) for x in us.download_loglikes()]
    rows = sorted(set(int(pdf[t]) for t in (ta, tb)))
    want = raw.rule_lattice(ref.Graph.from_dict(g), ref.Config(13.0, 6.0), ref.score_fn(mats[0], rows, m.id2pdf, 0.1), T)
    _same_lattice(_set_lattices(d)[0], want, "clean")
    mats[0][rows.index(int(pdf[tb])), 0] = np.nan
    us.upload_loglikes(mats)
    old = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    d = us.raw_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
    assert int(d["status"][0]) == LAT_NAN == int(old["status"][0]) and int(d["error_frame"][0]) == -1 == int(old["error_frame"][0])
    assert d["state_off"].tolist() == [0, 0] and d["arc_off"].tolist() == [0, 0] and int(d["start"][0]) == -1 and len(d["frame"]) == 0
    # scores from the band form of K1 are refused, as by khg_decode_lattice_simple
    us.close()


def test_band_scores_refused(setup):
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceModel, DeviceTransitions, UtteranceSet
    from oracle import oracle as orc
    m = synth.make_model(30, 64, 40, seed=7)
    ut = synth.make_utts(m, 8, seed=2, min_phones=3, max_phones=6)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ctx = Context(0)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    dt = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, dt, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm, reachable_only=True, band=True)
    with pytest.raises(Exception, match="khg_loglikes_band"):
        us.raw_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)


def _ctc_topo(n_tokens):
    """scripts/ctc_topo.py's shape (tests/test_gpu_lattice_simple.py): state i is token i, indices are token + 1, an input-epsilon
    self-loop on every state."""
    arcs = []
    S = n_tokens
    for i in range(S):
        for j in range(S):
            arcs.append((i, j + 1, 0 if i == j else j, 0.0, j))
        arcs.append((i, 0, 0, 0.25, i))
    final = {0: 0.0}
    return _hand(S, 0, arcs, final)


def test_decodable_ctc_scores_through_loglikes_upload(setup):
    """DecodableCtc's matrix as the set's resident scores (khg_loglikes_upload, index - 1 as the pdf): the path
    decode_utterance_lattice_simple takes for any decodable that is not a GMM."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceTransitions, UtteranceSet
    rng = np.random.default_rng(21)
    n_tok = 12
    g = _ctc_topo(n_tok)
    ctx = Context(0)
    dt = DeviceTransitions(ctx, np.concatenate([[-1], np.arange(n_tok)]).astype(np.int32))
    lens = [int(rng.integers(5, 40)) for _ in range(4)]
    mats = []
    for T in lens:
        x = rng.standard_normal((T, n_tok)).astype(np.float32) * 3
        mats.append((x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32))      # log-softmax rows
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    us = UtteranceSet(ctx, dt, fo, np.zeros((int(fo[-1]), 1), np.float32), graphs=tg.concat([g] * len(lens)))
    us.upload_loglikes([np.ascontiguousarray(x.T) for x in mats])
    old = us.decode_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=1.0)
    d = us.raw_lattice_simple(dt, beam=13.0, lattice_beam=6.0, acoustic_scale=1.0)
    for k in old:
        assert np.asarray(d[k]).tobytes() == np.asarray(old[k]).tobytes(), k
    lats = _set_lattices(d)
    ev = Evidence()
    for u, T in enumerate(lens):
        dec = khg.DecodableCtc(mats[u])
        want = raw.rule_lattice(ref.Graph.from_dict(g), ref.Config(13.0, 6.0), lambda f, i, dec=dec: np.float32(dec.log_likelihood(f, i)), T)
        assert int(d["status"][u]) == LAT_SUCCEEDED and want is not None
        _same_lattice(lats[u], want, u)
        ev.add(want)
        one = khg.decode_utterance_lattice_simple(khg.LatticeSimpleDecoder(_fst(khg, g), khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)),
                                                  dec, tm, "c%d" % u, True)
        L = khg.Lattice.from_arrays(*[lats[u][k] for k in FIELDS], lats[u]["start"])
        lin = L.shortest_path()
        ok, ali, words, _ = lin.get_linear_symbol_sequence()
        assert (ok, ali, words, raw.path_like(lin)) == one, u
    print(ev)
    assert ev.excised > 0 and ev.nonzero_extra > 0 and ev.multi_path > 0, ev
    us.close()
