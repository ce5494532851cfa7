"""The raw lattice of the lattice-faster decoder on the GPU (khg_decode_lattice_faster_raw through get_raw_lattice_faster_batch,
get_raw_lattice_faster_device_batch and the UtteranceSet methods) against the plain-Python restatement of its rule
(tests/lattice_faster_raw_ref.py), bit for bit: every state field, every arc field and their orders.  Scores
come from K1 (return_scores=True), so only the decoder and the emission are compared.  Configurations as in
tests/test_gpu_lattice_faster.py."""
import os
import sys
import time
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graphs as tg  # noqa: E402
import lattice_faster_raw_ref as rawf  # noqa: E402
import lattice_faster_ref as ref  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import test_shared_graph_cpu as sg  # noqa: E402
from test_gpu_lattice_ops import SWEEP_AS, SWEEP_GS, WEIGHTS, Evidence, _check_ops, _dict, _entry  # noqa: E402

pytestmark = pytest.mark.gpu

LAT_SUCCEEDED, LAT_PARTIAL, LAT_SCRATCH, LAT_NO_PATH, LAT_EPS_LOOP = 1, 2, 4, 8, 16
FIELDS = ops.FIELDS
OLD_KEYS = ("succeeded", "partial", "status", "alignment", "words", "like", "num_frames")
F = np.float32
INF = F(np.inf)


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
    k = rawf.same_lattice(lat, want)
    assert k is None, (tag, k)


def _is_empty(lat):
    return lat.num_states == 0 and lat.num_arcs_total == 0 and lat.start == -1 and list(lat.arc_begin) == [0]


def _same_results(a, b, tag):
    assert len(a) == len(b), tag
    for u, (x, y) in enumerate(zip(a, b)):
        for k in OLD_KEYS:
            assert x[k] == y[k] and type(x[k]) is type(y[k]), (tag, u, k)


class Seen:
    def __init__(self):
        self.compared = self.states = self.arcs = self.multi_arc_states = self.nonzero_extra = self.eps_arcs = self.partial = 0

    def add(self, want, partial):
        self.compared += 1
        self.states += len(want["frame"])
        self.arcs += len(want["ilabel"])
        self.multi_arc_states += int((np.diff(want["arc_begin"]) > 1).sum())
        self.nonzero_extra += int((want["extra_cost"] != 0.0).sum())
        self.eps_arcs += int((want["ilabel"] == 0).sum())
        self.partial += bool(partial)

    def __repr__(self):
        return "compared %d states %d arcs %d states with several arcs %d nonzero extra costs %d epsilon arcs %d partial %d" % (
            self.compared, self.states, self.arcs, self.multi_arc_states, self.nonzero_extra, self.eps_arcs, self.partial)


def _check(khg, id2pdf, am, tm, graphs, fsts, feats, cfg, rcfg, seen, scale=0.1, allow_partial=True, scratch=0):
    """graphs: the restatement's Graph (or the graph dict) of every utterance; fsts: what the batch calls take."""
    old = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, scale, allow_partial=allow_partial, scratch_per_frame=scratch)
    res = khg.get_raw_lattice_faster_batch(am, tm, fsts, feats, cfg, scale, allow_partial=allow_partial, scratch_per_frame=scratch,
                                           return_scores=True)
    assert len(res) == len(old) == len(feats)
    for u, (g, r, o) in enumerate(zip(graphs, res, old)):
        assert set(o) == set(OLD_KEYS) and set(r) == set(OLD_KEYS) | {"lattice", "loglikes", "pdfs"}
        for k in OLD_KEYS:
            assert r[k] == o[k] and type(r[k]) is type(o[k]), (u, k)          # khg_decode_lattice_faster returns what it returned
        lat = r["lattice"]
        assert isinstance(lat, khg.Lattice)
        G = g if isinstance(g, ref.Graph) else ref.Graph.from_dict(g)
        want, wres = rawf.rule_lattice(G, rcfg, ref.score_fn(r["loglikes"], r["pdfs"], id2pdf, scale), len(feats[u]), allow_partial)
        assert (r["succeeded"], r["partial"], r["alignment"], r["words"], r["like"]) == \
               (wres["succeeded"], wres["partial"], wres["alignment"], wres["words"], wres["like"]), (u, r["status"])
        if not r["succeeded"]:
            assert _is_empty(lat), u
            continue
        _same_lattice(lat, want, u)
        seen.add(want, r["partial"])
        # the decoder's best path is the lattice's, by the host Lattice's tie rule too
        bp = lat.best_path()
        assert (bp["ali"], bp["words"]) == (r["alignment"], r["words"]), u
        v = bp["weight"]
        assert float(F(-F(F(v[0]) + F(v[1])))) == r["like"], (u, v, r["like"])
    return res


def _cfgs(khg, **kw):
    return khg.LatticeFasterDecoderConfig(**kw), ref.Config(**kw)


@pytest.mark.parametrize("kind", ["random", "hub"])
@pytest.mark.parametrize("max_active", [3, 10, 7000])
@pytest.mark.parametrize("min_active", [0, 200])
def test_graphs_active_limits(setup, kind, max_active, min_active):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(100 + max_active + min_active + (7 if kind == "hub" else 0))
    n = 6
    gs = [tg.random_graph(rng, m.num_tids, n_main=12, p_eps=0.4) if kind == "random" else tg.hub_graph(rng, m.num_tids, fan=8, tail=5)
          for _ in range(n)]
    min_active = min(min_active, max_active)
    cfg, rcfg = _cfgs(khg, beam=13.0, max_active=max_active, min_active=min_active, lattice_beam=6.0)
    seen = Seen()
    _check(khg, m.id2pdf, am, tm, gs, [_fst(khg, g) for g in gs], _feats(ut, n), cfg, rcfg, seen)
    print(seen)
    assert seen.compared > 0
    if max_active == 7000:
        assert seen.multi_arc_states > 0 and seen.eps_arcs > 0, seen


@pytest.mark.parametrize("T", [24, 25, 26, 50])
def test_frames_around_prune_interval(setup, T):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(T)
    gs = [tg.random_graph(rng, m.num_tids, n_main=6, p_eps=0.3) for _ in range(4)]
    cfg, rcfg = _cfgs(khg, beam=10.0, lattice_beam=4.0)
    seen = Seen()
    _check(khg, m.id2pdf, am, tm, gs, [_fst(khg, g) for g in gs], _feats(ut, 4, [T] * 4), cfg, rcfg, seen)
    assert seen.compared > 0, seen


def test_mismatched_model(setup):
    khg, synth, m, am, tm, ut = setup
    mm = synth.mismatched_model(m, 0.5, seed=3)
    am2, tm2 = synth.host_objects(mm)
    rng = np.random.default_rng(9)
    gs = [tg.random_graph(rng, m.num_tids, n_main=10, p_branch=0.6, p_eps=0.3) for _ in range(8)]
    cfg, rcfg = _cfgs(khg, beam=6.0, max_active=10, min_active=2, lattice_beam=2.0)
    seen = Seen()
    _check(khg, mm.id2pdf, am2, tm2, gs, [_fst(khg, g) for g in gs], _feats(ut, 8), cfg, rcfg, seen)
    assert seen.compared > 0, seen


def test_large_graph_above_1000_states_and_batch_equals_one_utterance_batches(setup):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(1234)
    g = tg.random_graph(rng, m.num_tids, n_main=1100, p_eps=0.2)
    small = [tg.random_graph(rng, m.num_tids, n_main=9, p_eps=0.3) for _ in range(3)]
    gs = [g, small[0], g, small[1], small[2]]
    feats = _feats(ut, 5, [120, 30, 60, 20, 25])
    cfg, rcfg = _cfgs(khg, beam=13.0, max_active=7000, lattice_beam=6.0)
    seen = Seen()
    res = _check(khg, m.id2pdf, am, tm, gs, [_fst(khg, x) for x in gs], feats, cfg, rcfg, seen)
    print(seen)
    assert seen.compared == 5 and seen.multi_arc_states > 0, seen
    # a batch is its one-utterance batches
    for u in range(len(gs)):
        one = khg.get_raw_lattice_faster_batch(am, tm, [_fst(khg, gs[u])], feats[u: u + 1], cfg, 0.1)
        assert len(one) == 1 and set(one[0]) == set(OLD_KEYS) | {"lattice"}
        _same_results(one, res[u: u + 1], u)
        _same_lattice(one[0]["lattice"], _dict(res[u]["lattice"]), u)
        assert one[0]["lattice"].to_text() == res[u]["lattice"].to_text()


@pytest.mark.parametrize("allow_partial", [True, False])
def test_no_final_state(setup, allow_partial):
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(77)
    gs = [tg.random_graph(rng, m.num_tids, n_main=8, with_final=(u % 2 == 0)) for u in range(6)]
    cfg, rcfg = _cfgs(khg, beam=13.0, lattice_beam=6.0)
    seen = Seen()
    res = _check(khg, m.id2pdf, am, tm, gs, [_fst(khg, g) for g in gs], _feats(ut, 6), cfg, rcfg, seen, allow_partial=allow_partial)
    for u in (1, 3, 5):
        lat = res[u]["lattice"]
        assert res[u]["partial"] and res[u]["succeeded"] == allow_partial
        if allow_partial:
            # no final state was reached: One() on every token of the last frame
            last = np.asarray(lat.frame) == lat.frame[-1]
            assert ops.bits(np.asarray(lat.final_cost)[last]) == ops.bits(np.zeros(int(last.sum()))), u
        else:
            assert res[u]["status"] == LAT_PARTIAL and _is_empty(lat), u
    assert seen.partial == (3 if allow_partial else 0)


def test_failing_statuses_give_empty_lattices(setup):
    """NO_PATH (a beam nothing survives), EPS_LOOP (an epsilon cycle among a frame's tokens), SCRATCH (scratch_per_frame = 1): an empty
    lattice each, with the status khg_decode_lattice_faster gives; their neighbours in the batch are not disturbed."""
    khg, synth, m, am, tm, ut = setup
    rng = np.random.default_rng(5)
    good = tg.random_graph(rng, m.num_tids, n_main=6)
    loop = {"start": 0, "arc_off": np.array([0, 2, 3], np.int64), "ilabel": np.array([1, 0, 0], np.int32),
            "olabel": np.array([0, 5, 6], np.int32), "weight": np.array([0.0, 0.1, 0.1], np.float32),
            "nextstate": np.array([0, 1, 0], np.int32), "final": np.array([0.0, np.inf], np.float32)}
    # one emitting arc into a dead end: no token is left on frame 2
    dead = {"start": 0, "arc_off": np.array([0, 1, 1], np.int64), "ilabel": np.array([1], np.int32), "olabel": np.array([0], np.int32),
            "weight": np.array([0.0], np.float32), "nextstate": np.array([1], np.int32), "final": np.array([np.inf, 0.0], np.float32)}
    gs = [good, loop, dead, good]
    feats = _feats(ut, 4)
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    fsts = [_fst(khg, g) for g in gs]
    old = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
    res = khg.get_raw_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
    _same_results(res, old, "statuses")
    assert [r["status"] for r in res] == [LAT_SUCCEEDED, LAT_EPS_LOOP, LAT_NO_PATH, LAT_SUCCEEDED]
    assert [_is_empty(r["lattice"]) for r in res] == [False, True, True, False]
    rd, dl = khg.get_raw_lattice_faster_device_batch(am, tm, fsts, feats, cfg, 0.1)
    _same_results(rd, old, "device statuses")
    assert np.diff(dl.state_off).tolist() == [r["lattice"].num_states for r in res]
    bp = dl.best_path([1.0], [1.0])
    assert bp["status"].tolist() == [ops.SUCCEEDED, ops.NO_PATH, ops.NO_PATH, ops.SUCCEEDED]
    dl.close()
    hubs = [tg.hub_graph(rng, m.num_tids, fan=10, tail=5) for _ in range(3)]
    res = khg.get_raw_lattice_faster_batch(am, tm, [_fst(khg, g) for g in hubs], feats[:3], cfg, 0.1, scratch_per_frame=1)
    assert all(r["status"] & LAT_SCRATCH and not r["succeeded"] and _is_empty(r["lattice"]) for r in res)


def test_words_status_gives_an_empty_lattice(setup):
    """KHG_LAT_WORDS (32): more words on the best path than frames + states + 64.  An epsilon chain of 99 word arcs through 100 states
    and one emitting arc back to its head: 99 words a frame, 5 frames, 495 words against 169.  (A small words_cap of the caller's is
    KHG_E_ARG for the whole call, not this status.)"""
    khg, synth, m, am, tm, ut = setup
    S = 100
    il = [0] * (S - 1) + [1]
    g = {"start": 0, "arc_off": np.arange(S + 1, dtype=np.int64), "ilabel": np.array(il, np.int32),
         "olabel": np.array(list(range(1, S)) + [0], np.int32), "weight": np.full(S, 0.01, np.float32),
         "nextstate": np.array(list(range(1, S)) + [0], np.int32), "final": np.array([0.0] + [np.inf] * (S - 1), np.float32)}
    rng = np.random.default_rng(6)
    good = tg.random_graph(rng, m.num_tids, n_main=6)
    fsts = [_fst(khg, good), _fst(khg, g)]
    feats = _feats(ut, 2, [20, 5])
    cfg = khg.LatticeFasterDecoderConfig(beam=13.0, lattice_beam=6.0)
    old = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
    res = khg.get_raw_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
    _same_results(res, old, "words")
    assert res[0]["succeeded"] and not _is_empty(res[0]["lattice"])
    assert res[1]["status"] & 32 and not res[1]["succeeded"] and _is_empty(res[1]["lattice"]), res[1]["status"]


def test_resident_scores_uploaded_and_python_decodable(setup):
    """A table of scores that is no GMM's: uploaded as the set's resident scores (UtteranceSet.upload_loglikes, index - 1 as the pdf)
    and decoded by UtteranceSet.raw_lattice_faster; the restatement reads the same table, and so does a Python DecodableInterface
    through decode_utterance_lattice_faster."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import Context, DeviceTransitions, UtteranceSet
    rng = np.random.default_rng(8)
    n_idx = 12
    g = tg.hub_graph(rng, n_idx, fan=5, tail=4)
    lens = [30, 17, 44]
    tabs = [np.random.default_rng(3 + i).normal(size=(T, n_idx + 1)).astype(np.float32) for i, T in enumerate(lens)]
    ctx = Context(0)
    dt = DeviceTransitions(ctx, np.concatenate([[-1], np.arange(n_idx)]).astype(np.int32))
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    us = UtteranceSet(ctx, dt, fo, np.zeros((int(fo[-1]), 1), np.float32), graphs=tg.concat([g] * len(lens)))
    po, pl = us.pdf_lists()                                          # the rows of an utterance's matrix: the pdfs of its graph
    us.upload_loglikes([np.ascontiguousarray(t[:, 1 + np.asarray(pl[po[u]: po[u + 1]])].T) for u, t in enumerate(tabs)])
    kw = dict(beam=9.0, lattice_beam=5.0, max_active=6, min_active=2, acoustic_scale=1.0)
    old = us.decode_lattice_faster(dt, **kw)
    d = us.raw_lattice_faster(dt, **kw)
    for k in old:
        assert np.asarray(d[k]).tobytes() == np.asarray(old[k]).tobytes(), k
    assert d["device_bytes"] > 0
    dd = us.raw_lattices_faster_device(dt, **kw)
    for k in old:
        assert np.asarray(dd[k]).tobytes() == np.asarray(old[k]).tobytes(), k
    dev = dd["lattices"].download()
    so, ao = d["state_off"], d["arc_off"]
    rcfg = ref.Config(beam=9.0, lattice_beam=5.0, max_active=6, min_active=2)
    cfg = khg.LatticeFasterDecoderConfig(beam=9.0, lattice_beam=5.0, max_active=6, min_active=2)
    for u, T in enumerate(lens):
        tab = tabs[u]
        want, wres = rawf.rule_lattice(ref.Graph.from_dict(g), rcfg, lambda f, i, tab=tab: np.float32(tab[f, i]), T)
        assert wres["succeeded"] and int(d["status"][u]) & LAT_SUCCEEDED
        lat = {k: np.asarray(d[k][so[u]: so[u + 1]]) for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost")}
        lat.update({k: np.asarray(d[k][ao[u]: ao[u + 1]]) for k in ("ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")})
        lat["arc_begin"] = np.concatenate([d["arc_begin"][so[u]: so[u + 1]], [ao[u + 1] - ao[u]]]).astype(np.int32)
        lat["start"] = int(d["start"][u])
        _same_lattice(lat, want, u)
        _same_lattice(dev[u], want, ("device", u))
        assert d["ali"][fo[u]: fo[u + 1]].tolist() == wres["alignment"] and float(d["like"][u]) == wres["like"]

        class Dec(khg.DecodableInterface):
            def log_likelihood(self, frame, index):
                return float(tab[frame, index])

            def is_last_frame(self, frame):
                return frame == T - 1

            def num_frames_ready(self):
                return T

            def num_indices(self):
                return n_idx
        got = khg.decode_utterance_lattice_faster(khg.LatticeFasterDecoder(_fst(khg, g), cfg), Dec(), tm, "u", True)
        assert got == (True, wres["alignment"], wres["words"], wres["like"]), u
    dd["lattices"].close()
    us.close()


def test_decoding_graph_and_single_fst_are_shared(setup):
    khg, synth, m, am, tm, ut = setup
    g = sg.word_loop_graph(np.random.default_rng(300), m.num_tids, 300, 1)
    lens = [40, 24, 25, 26]
    feats = _feats(ut, len(lens), lens)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg, rcfg = _cfgs(khg, beam=13.0, max_active=7000, lattice_beam=6.0)
    seen = Seen()
    res = _check(khg, m.id2pdf, am, tm, [g] * len(lens), dg, feats, cfg, rcfg, seen)
    print(seen)
    assert seen.compared == len(lens) and seen.multi_arc_states > 0, seen
    one = khg.get_raw_lattice_faster_batch(am, tm, _fst(khg, g), feats, cfg, 0.1)
    _same_results(one, res, "one StdVectorFst")
    for u in range(len(lens)):
        _same_lattice(one[u]["lattice"], _dict(res[u]["lattice"]), u)
    rd, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    _same_results(rd, res, "device")
    for u, x in enumerate(dl.download()):
        _same_lattice(x, _dict(res[u]["lattice"]), ("device", u))
    dl.close()
    dg.close()


@pytest.fixture(scope="module")
def trained():
    import kaldi_hmm_gmm_amd as khg
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import decode_synthetic as dx
    from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions
    args = types.SimpleNamespace(utts=200, test_utts=30, iters=80, dim=23, seed=3)
    tm, tree, am, lexicon, test_utts = dx.train(args, log=lambda *a: None)
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                  opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gcomp.compile_word_loop_graph()
    return khg, dx, tm, am, graph, test_utts


def test_trained_word_loop_at_decode_py_config_and_device_lattices(trained):
    """egs/yesno/decode.py's configuration on the trained word loop as compiled (no epsilon self-loops added): every lattice is the
    restatement's; on the device handle the best path at (1, 1) is the decoder's, the 11-weight sweep equals 11 single calls and the
    restatement, pruning keeps the best path, and from_lattices(download()) round-trips."""
    khg, dx, tm, am, graph, test_utts = trained
    feats = [u[2] for u in test_utts]
    cfg, rcfg = _cfgs(khg, max_active=7000, beam=13.0, lattice_beam=6.0)
    c = graph.to_csr()
    G = ref.Graph(c["start"], c["arc_off"], c["ilabel"], c["olabel"], c["weight"], c["nextstate"], c["final"])
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    seen = Seen()
    res = _check(khg, id2pdf, am, tm, [G] * len(feats), graph, feats, cfg, rcfg, seen)
    print(seen)
    assert seen.compared == len(feats) and all(r["status"] == 1 for r in res)
    assert seen.multi_arc_states > 0, seen
    errs = sum(dx.edit_distance(u[1], r["words"]) for u, r in zip(test_utts, res))
    assert errs <= 0.05 * sum(len(u[1]) for u in test_utts)
    rd, dl = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, cfg, 0.1)
    _same_results(rd, res, "device")
    assert dl.num_chunks == 1 and dl.chunk_off == [0, len(feats)]
    L = dl.download()
    lats = [_dict(x) for x in L]
    for u in range(len(feats)):
        _same_lattice(res[u]["lattice"], lats[u], u)
    ev = Evidence()
    _check_ops(khg, dl, lats, ev, decoded=res, beams=[0.5, float("inf")], pairs=[(1.0, float(SWEEP_AS[5]))])
    print(ev)
    assert ev.lattices == len(feats) and ev.paths == len(WEIGHTS) * len(feats) and ev.pruned_smaller > 0
    up = khg.DeviceLattices.from_lattices(L)
    for a, b in zip(up.download(), lats):
        _same_lattice(a, b, "round trip")
    many, again = dl.best_path(SWEEP_GS, SWEEP_AS), up.best_path(SWEEP_GS, SWEEP_AS)
    for k in range(len(WEIGHTS)):
        for u in range(len(feats)):
            assert _entry(many, k, u, len(feats)) == _entry(again, k, u, len(feats)), (k, u)
    assert "\n" in L[0].to_text()
    up.close(); dl.close()


def _decoder_launches(ctx, call):
    """-> (call's result, the kernel names of its launches under the context's kernel timing)"""
    ctx.sync(); ctx.timings(); ctx.set_timing(True)
    try:
        out = call()
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.set_timing(False)
    return out, names


def test_second_pass_for_some_utterances(setup):
    """One batch, one chunk, on the 3000-word loop (one shared DecodingGraph: its loop state is past the list-of-graphs path's
    in-degree limit) under a beam that prunes nothing.  The automatic scratch is (T + 1) * 256 + 3002 tokens and (T + 1) * 1024 + 9001
    links: a one-frame utterance (3001 tokens, 3000 links) fits, an utterance of 24 or 33 frames (up to 3001 tokens and 9000 links
    a frame) runs out and is decoded again.  The decoder kernel runs twice, the lattices come back in utterance order, and each
    equals its one-utterance batch's -- which itself takes one launch for the short utterances and two for the long ones."""
    khg, synth, m, am, tm, ut = setup
    from kaldi_hmm_gmm_amd import _gpu
    ctx = _gpu.default_context()
    g = sg.word_loop_graph(np.random.default_rng(3000), m.num_tids, 3000, 1)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    lens = [1, 24, 1, 33, 1]
    U = len(lens)
    feats = _feats(ut, U, lens)
    cfg = khg.LatticeFasterDecoderConfig(beam=100.0, max_active=7000, lattice_beam=6.0)
    old = khg.decode_lattice_faster_batch(am, tm, dg, feats, cfg, 0.1)
    (res, dl), names = _decoder_launches(ctx, lambda: khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1))
    print(names)
    assert dl.num_chunks == 1 and names.count("k2_lattice_faster") == 2 and names.count("k2_lattice_faster_raw_fill") == 2
    assert names.count("k2_lattice_faster_raw_gather") == 1
    _same_results(res, old, "second pass")
    assert all(r["succeeded"] for r in res) and not any(r["status"] & LAT_SCRATCH for r in res)
    L = dl.download()
    assert dl.state_off.tolist() == np.concatenate([[0], np.cumsum([x.num_states for x in L])]).tolist()
    assert dl.arc_off.tolist() == np.concatenate([[0], np.cumsum([x.num_arcs_total for x in L])]).tolist()
    host = khg.get_raw_lattice_faster_batch(am, tm, dg, feats, cfg, 0.1)
    for u in range(U):
        one, n1 = _decoder_launches(ctx, lambda: khg.get_raw_lattice_faster_batch(am, tm, dg, feats[u: u + 1], cfg, 0.1))
        assert n1.count("k2_lattice_faster") == (1 if lens[u] == 1 else 2), (u, n1)      # which utterances ran out
        _same_results(one, res[u: u + 1], u)
        assert one[0]["lattice"].num_states > 0 and int(one[0]["lattice"].frame[-1]) == lens[u]
        _same_lattice(L[u], _dict(one[0]["lattice"]), u)
        _same_lattice(host[u]["lattice"], _dict(one[0]["lattice"]), ("host", u))
        khg.DeviceLattices.validate([L[u]])
    print("states %s arcs %s" % (np.diff(dl.state_off).tolist(), np.diff(dl.arc_off).tolist()))
    # the gathered handle is an ordinary one
    bp = dl.best_path([1.0], [1.0])
    for u, r in enumerate(res):
        assert _entry(bp, 0, u, U)[:3] == (ops.SUCCEEDED, r["alignment"], r["words"]), u
    dl.close(); dg.close()


def _slice_bytes(T, S, A, hb, lat=True):
    """lat_layout (khg_k2_lattice.hip.inc) at the automatic scratch size: the bytes of one utterance's slice"""
    tc, lc = (T + 1) * min(S, 256) + S + 1, (T + 1) * min(A, 1024) + A + 1
    qcap, rpcap = 2 * (S + A) + 16, 2 * S + 64
    slotcap = S + 2 * rpcap
    rows = [48 * tc, 24 * lc, 12 * S, 12 * S, 4 * hb, 4 * hb, 4 * qcap, 4 * S, 4 * A, 4 * S, 4 * (T + 1), 4 * (T + 1), 4 * (T + 1), 4 * (S + 1),
            4 * rpcap, 4 * rpcap, 4 * slotcap]
    if lat:
        rows += [4 * tc, 4 * tc, 4 * tc, 4 * (tc + 1), 4 * (T + 2)]
    return (sum((r + 15) & ~15 for r in rows) + 255) & ~255


def test_more_than_one_launch(setup):
    """Short utterances on the 66 001-state word loop (one shared DecodingGraph), as many as take the scratch slices past 4 GiB: the
    batch is decoded and emitted in two launches, the handle has two chunks, and everything equals the one-chunk sub-batches cut at
    the chunk boundary.  (The restatement takes minutes per utterance on this graph.)"""
    khg, synth, m, am, tm, ut = setup
    g = sg.word_loop_graph(np.random.default_rng(sg.BIG_W), m.num_tids, sg.BIG_W, sg.BIG_CHAIN)
    S, A = len(g["final"]), len(g["ilabel"])
    lens3 = [12, 11, 13]
    hb = max(1000, int(np.float32(S) * np.float32(2.0))) + 1
    per = [_slice_bytes(T, S, A, hb) for T in lens3]
    U = int((4 << 30) // min(per)) + 9
    lens = [lens3[u % 3] for u in range(U)]
    assert sum(_slice_bytes(T, S, A, hb) for T in lens) > (4 << 30) and sum(_slice_bytes(T, S, A, hb) for T in lens[: U // 2]) < (4 << 30)
    feats = _feats(ut, U, lens)
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=8.0, max_active=100, min_active=0, lattice_beam=4.0)
    t0 = time.time()
    old = khg.decode_lattice_faster_batch(am, tm, dg, feats, cfg, 0.1)
    t_old = time.time() - t0
    t0 = time.time()
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    t_new = time.time() - t0
    co = dl.chunk_off
    print("utterances %d, chunks %d at %s; states %d arcs %d; decode_lattice_faster_batch %.1f s, with the lattices %.1f s" % (
        U, dl.num_chunks, co, int(dl.state_off[-1]), int(dl.arc_off[-1]), t_old, t_new))
    assert dl.num_chunks >= 2 and co[0] == 0 and co[-1] == U and all(b > a for a, b in zip(co, co[1:]))
    _same_results(res, old, "device handle / plain call")
    assert all(r["succeeded"] for r in res) and not any(r["status"] & LAT_SCRATCH for r in res)
    L = dl.download()
    lats = [_dict(x) for x in L]
    assert all(x.num_states > 0 for x in L)
    for a, b in zip(co, co[1:]):
        r1, d1 = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats[a:b], cfg, 0.1)
        assert d1.num_chunks == 1, (a, b)
        _same_results(r1, res[a:b], (a, b))
        for i, x in enumerate(d1.download()):
            _same_lattice(x, lats[a + i], ("sub-batch", a, b, i))
        d1.close()
    # the operations run once per chunk: the best path at (1, 1) is the decoder's for every utterance of both chunks
    bp = dl.best_path([1.0], [1.0])
    for u, r in enumerate(res):
        e = _entry(bp, 0, u, U)
        assert e[:3] == (ops.SUCCEEDED, r["alignment"], r["words"]), u
        v = bp["weight"][u]
        assert float(F(-F(v[0] + v[1]))) == r["like"], u
    P = dl.prune(0.5)
    assert P.num_chunks == dl.num_chunks and P.chunk_off == co
    after = P.best_path([1.0], [1.0])
    for u in (0, co[1] - 1, co[1], U - 1):
        assert _entry(after, 0, u, U) == _entry(bp, 0, u, U), u
    P.close(); dl.close(); dg.close()
