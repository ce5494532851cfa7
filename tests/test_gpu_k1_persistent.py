"""The persistent launch of the default K1 (option k1_launch = 2: one workgroup per CU takes chunks of frame tiles from a counter and
copies the next chunk's tiles into LDS under the tail of the current one) against the one-workgroup-per-chunk launch (k1_launch = 1).

Every (pdf, frame tile) cell goes through the same instruction sequence in both; only which wave computes it when differs.  So the
scores are compared BIT FOR BIT between the two option values, and once per case against the fp64 restatement at the tolerance of
tests/test_gpu_parity.py (1e-5 + 1e-6 B).

The launches here have more chunks than workgroups: option k1_pgrid caps the persistent grid (1 or 2 workgroups), and k1_order = 1
("none") keeps the chunks in utterance order, so with one workgroup the sequence of chunk sizes -- which decides how much of the
next chunk fits beside the current one -- is the list of lengths the test wrote down.  A workgroup puts its chunks at the two ends
of its tile slots in turn: the chunks at odd positions of that sequence stand end-aligned, their last tile in the last slot."""
import numpy as np
import pytest

from helpers import build, exact_loglikes, utt_feats
from kaldi_hmm_gmm_amd import KhgError

pytestmark = pytest.mark.gpu

LL_ATOL, LL_RTOL = 1e-5, 1e-6        # tests/test_gpu_parity.py
POISON = np.float32(12345.0)


def _nmax(D):
    return 15 if D <= 40 else 7      # k1s_nmax: frame tiles per chunk (LDS)


def _lens(tiles, rng):
    """Utterance lengths in frames with the given numbers of 32-frame tiles (a partial last tile, except for every third)."""
    return np.array([32 * n - (0 if i % 3 == 0 else int(rng.integers(1, 32))) for i, n in enumerate(tiles)])


def _feature_set(ctx, P, G, D, tiles, seed, pdf_list):
    from kaldi_hmm_gmm_amd import DeviceModel, UtteranceSet

    m, gc, om, ut, cost = build(P, G, D, n_utt=2, seed=seed)
    rng = np.random.default_rng(seed)
    lens = _lens(tiles, rng)
    frame_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feats = (rng.standard_normal((int(frame_off[-1]), D)) * 1.5 + 0.3).astype(np.float32)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    return m, gc, dm, frame_off, feats, np.asarray(pdf_list, np.int32)


def _scores(ctx, opt, dm, frame_off, feats, pl, launch, pgrid):
    """Scores of a features-only set (one shared pdf list) under one launch shape; a fresh set, so that its chunk plan follows k1_order."""
    from kaldi_hmm_gmm_amd import UtteranceSet

    opt("k1_launch", launch)
    opt("k1_pgrid", pgrid)
    us = UtteranceSet(ctx, None, frame_off, feats)
    us.set_pdf_list(pl)
    us.loglikes(dm)
    got = us.download_loglikes()
    us.close()
    return got


def _assert_exact(m, gc, feats, frame_off, pl, got):
    for u in range(len(frame_off) - 1):
        exact, bound = exact_loglikes(m, gc, feats[frame_off[u]: frame_off[u + 1]], pl)
        tol = LL_ATOL + LL_RTOL * bound
        assert got[u].shape == exact.shape and np.isfinite(got[u]).all()
        err = np.abs(got[u] - exact)
        assert (err <= tol).all(), f"utt {u}: max err/tol {(err / tol).max()}"


# chunk sizes in tiles, as fractions of NMAX = N: 1 tile | exactly N | N + 1 (two chunks of one utterance) | a small chunk followed by
# a full one (the prefetch fits partly, the rest is copied behind the barrier) | a full one followed by a small one (nothing fits) |
# sizes that fit completely (no second barrier) | ... up to 30 utterances
def _tiles(N):
    t = [1, N, N + 1, 3, N, N, 2, 1, 1, N - 1, 1, N // 2, N // 2, N // 2 + 1, N, 1, 2 * N + 1, 2, N - 2, 3, 1, N, N, 4, 2, N + 2, 1, 5, N - 3, 1]
    assert len(t) == 30
    return t


@pytest.mark.parametrize("pgrid", [1, 2, 0])
@pytest.mark.parametrize("P,G,D", [(12, 64, 40), (6, 128, 80)])
def test_persistent_equals_one_chunk_launch_bit_for_bit(ctx, opt, P, G, D, pgrid):
    """Full matrices of 30 utterances whose chunk sizes walk every boundary path, with 1 and 2 workgroups (more chunks than
    workgroups) and the uncapped grid (fewer chunks than workgroups).  D = 80: KS = 10, a 7-slot ring, one W tile per pass."""
    opt.k1("f16x2s")
    opt("k1_order", 1)
    N = _nmax(D)
    m, gc, dm, frame_off, feats, pl = _feature_set(ctx, P, G, D, _tiles(N), seed=P + D, pdf_list=np.arange(P))
    old = _scores(ctx, opt, dm, frame_off, feats, pl, 1, 0)
    new = _scores(ctx, opt, dm, frame_off, feats, pl, 2, pgrid)
    for u in range(len(old)):
        assert np.array_equal(old[u], new[u]), f"utt {u} ({_tiles(N)[u]} tiles) differs"
    if pgrid == 1:
        _assert_exact(m, gc, feats, frame_off, pl, new)


def test_persistent_default_order_and_one_utterance(ctx, opt):
    """The default chunk order (largest first) under the persistent launch; and a set of ONE utterance (a small set: chunks of at
    most 3 tiles, the automatic setting keeps the one-chunk launch -- option 2 still runs the persistent kernel on it)."""
    opt.k1("f16x2s")
    m, gc, dm, frame_off, feats, pl = _feature_set(ctx, 12, 64, 40, _tiles(15), seed=5, pdf_list=np.arange(12))
    old = _scores(ctx, opt, dm, frame_off, feats, pl, 1, 0)
    for pgrid in (2, 3):
        new = _scores(ctx, opt, dm, frame_off, feats, pl, 2, pgrid)
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
    auto = _scores(ctx, opt, dm, frame_off, feats, pl, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(old, auto))
    one_off, one_feats = frame_off[4:6] - frame_off[4], feats[frame_off[4]: frame_off[5]]       # 15 tiles -> five chunks of 3
    old1 = _scores(ctx, opt, dm, one_off, one_feats, pl, 1, 0)
    for pgrid in (0, 1, 2):
        new1 = _scores(ctx, opt, dm, one_off, one_feats, pl, 2, pgrid)
        assert np.array_equal(old1[0], new1[0])
    _assert_exact(m, gc, one_feats, one_off, pl, new1)


def test_persistent_many_pass_pdf_last_in_the_list(ctx, opt):
    """A pdf of more than TPS = 2 W tiles (150 Gaussians: five tiles, three passes that combine with the stored value) as the LAST
    item of every chunk's list -- cut into four frame ranges, whose owed last value is drained before the chunk's barrier."""
    opt.k1("f16x2s")
    opt("k1_order", 1)
    counts = np.full(12, 64)
    counts[11] = 150
    from kaldi_hmm_gmm_amd import DeviceModel

    m, gc, om, ut, cost = build(12, 64, 40, n_utt=2, seed=9, gauss_counts=counts)
    rng = np.random.default_rng(9)
    tiles = [4, 15, 2, 15, 1, 9, 16, 3]
    lens = _lens(tiles, rng)
    frame_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    feats = (rng.standard_normal((int(frame_off[-1]), 40)) * 1.5 + 0.3).astype(np.float32)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    pl = np.arange(12, dtype=np.int32)
    old = _scores(ctx, opt, dm, frame_off, feats, pl, 1, 0)
    for pgrid in (1, 2):
        new = _scores(ctx, opt, dm, frame_off, feats, pl, 2, pgrid)
        assert all(np.array_equal(a, b) for a, b in zip(old, new))
    _assert_exact(m, gc, feats, frame_off, pl, new)


def _chunks_in_utterance_order(T, N):
    """(utterance, first tile, tiles) of every chunk in launch order under k1_order = 1: plan_x32_chunks' rule."""
    out = []
    for u, t in enumerate(T):
        n32 = (int(t) + 31) // 32
        nch = (n32 + N - 1) // N
        for c in range(nch):
            t0, t1 = n32 * c // nch, n32 * (c + 1) // nch
            if t1 > t0:
                out.append((u, t0, t1 - t0))
    return out


@pytest.fixture(scope="module")
def graph_set():
    """30 utterances of 1 .. 45 phones with their training graphs: chunks of 1 .. 15 tiles, a few utterances of two chunks."""
    return build(12, 64, 40, n_utt=30, seed=41, min_phones=1, max_phones=45)


@pytest.mark.parametrize("mode", ["full", "reachable_only", "band"])
def test_persistent_cell_modes_and_shifted_band_in_the_last_slot(ctx, opt, graph_set, mode):
    """The three cell modes on graphs, old launch against new with 1 and 2 workgroups, untouched cells included (both start from
    the same poisoned block).  With one workgroup and utterance order the chunks at odd positions stand END-ALIGNED in the tile
    slots: a shifted band (tiles that start at the band's first frame: every read also takes columns of the NEXT tile) that ends in
    such a chunk's last tile reads up to the last slot's last byte -- the edge of the placement."""
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet

    opt.k1("f16x2s")
    opt("k1_order", 1)
    m, gc, om, ut, cost = graph_set
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    kw = {"full": {}, "reachable_only": {"reachable_only": True}, "band": {"band": True}}[mode]

    def run(launch, pgrid):
        opt("k1_launch", launch)
        opt("k1_pgrid", pgrid)
        us = UtteranceSet(ctx, tm, ut.frame_off, ut.feats, graphs=ut.graphs)
        us.loglikes(dm)                                      # shapes of the score blocks
        shapes = us.download_loglikes()
        us.upload_loglikes([np.full_like(f, POISON) for f in shapes])
        us.loglikes(dm, **kw)
        return us, us.download_loglikes()

    us_old, old = run(1, 0)
    T = np.diff(ut.frame_off)
    if mode == "band":
        # shifted bands (the host's rule, khg_k1.hip) inside ONE chunk, ending in the last tile of a chunk at an odd position
        poff, pdfs = us_old.pdf_lists()
        first, last = us_old.pdf_first_frames(), us_old.pdf_last_frames()
        edge = 0
        for pos, (u, t0, n) in enumerate(_chunks_in_utterance_order(T, 15)):
            for k in range(poff[u], poff[u + 1]):
                fp, lp = int(first[k]), int(last[k])
                shifted = lp >= 0 and lp // 32 > fp // 32 and lp % 32 < fp % 32
                if shifted and pos % 2 == 1 and fp // 32 >= t0 and lp // 32 == t0 + n - 1 and n >= 2:
                    edge += 1
        print("shifted bands ending in the last slot of an end-aligned chunk:", edge)
        assert edge > 0
    assert (T > 480).any() and (T <= 32).any(), "the set was meant to hold one-tile and two-chunk utterances"
    for pgrid in (1, 2):
        us_new, new = run(2, pgrid)
        for u in range(len(old)):
            assert np.array_equal(old[u], new[u]), (mode, pgrid, u)
        us_new.close()
    if mode == "full":
        poff, pdfs = us_old.pdf_lists()
        for u in range(us_old.n_utt):
            exact, bound = exact_loglikes(m, gc, utt_feats(ut, u), pdfs[poff[u]: poff[u + 1]])
            assert (np.abs(new[u] - exact) <= LL_ATOL + LL_RTOL * bound).all()
    us_old.close()


def test_persistent_band_then_repair_gives_unbanded_scores(ctx, opt, graph_set):
    """Band scores from the persistent launch, then a forced certificate failure (max_active set: the exact DP certifies nothing):
    the repair launch recomputes every utterance without the band's upper limit -- the scores from each pdf's first needed tile on
    are those of the full matrix, and the alignment is the full matrix's."""
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet

    opt.k1("f16x2s")
    m, gc, om, ut, cost = graph_set
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    opt("k1_launch", 1)
    us = UtteranceSet(ctx, tm, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm)
    full = us.download_loglikes()
    res_full = us.align(tm, beam=200.0, retry_beam=0.0, acoustic_scale=0.1, max_active=100000)
    opt("k1_launch", 2)
    opt("k1_pgrid", 2)
    us.loglikes(dm, band=True)
    res = us.align(tm, beam=200.0, retry_beam=0.0, acoustic_scale=0.1, max_active=100000)
    assert ((res["status"] & 8) != 0).all(), "max_active was meant to send every utterance through the repair launch"
    assert np.array_equal(res["ali"], res_full["ali"]) and np.array_equal(res["status"] & 3, res_full["status"] & 3)
    np.testing.assert_array_equal(res["like"], res_full["like"])
    got = us.download_loglikes()
    poff, pdfs = us.pdf_lists()
    first = us.pdf_first_frames()
    for u in range(us.n_utt):
        for j in range(poff[u + 1] - poff[u]):
            t0 = 32 * (min(int(first[poff[u] + j]), 10**6) // 32)
            assert np.array_equal(got[u][j, t0:], full[u][j, t0:]), (u, j)
    us.close()


def test_persistent_error_flag_from_the_last_chunk(ctx, opt):
    """A NaN feature in the last utterance -- the last chunk a workgroup takes -- still raises (KHG_E_RUNTIME -> KhgError); and so
    does a value the persistent kernel itself finds invalid there: a pdf whose components all have weight zero (gconst = -inf, which
    the domain check of the fp16 form skips) gives -inf in every chunk, the last one included."""
    from kaldi_hmm_gmm_amd import DeviceModel, UtteranceSet

    opt.k1("f16x2s")
    opt("k1_order", 1)
    opt("k1_launch", 2)
    opt("k1_pgrid", 2)
    m, gc, dm, frame_off, feats, pl = _feature_set(ctx, 12, 64, 40, [3, 15, 2, 7, 1, 4, 2], seed=17, pdf_list=np.arange(12))
    bad = feats.copy()
    bad[-5, 7] = np.nan
    us = UtteranceSet(ctx, None, frame_off, bad)
    us.set_pdf_list(pl)
    with pytest.raises(KhgError):
        us.loglikes(dm)
        ctx.sync()
    us.close()
    gc2 = gc.copy()
    gc2[m.gauss_off[11]: m.gauss_off[12]] = -np.inf
    dm2 = DeviceModel(ctx, m.gauss_off, gc2, m.means_invvars, m.inv_vars)
    ctx.set_timing(True)
    ctx.timings()
    us = UtteranceSet(ctx, None, frame_off[-2:] - frame_off[-2], feats[frame_off[-2]:])      # the last utterance alone: one chunk, one workgroup
    us.set_pdf_list(pl)
    with pytest.raises(KhgError):
        us.loglikes(dm2)
        ctx.sync()
    names = [n for n, _ in ctx.timings()]
    ctx.set_timing(False)
    assert "k1_loglikes" in names and "k0s_pack_tiles" in names, names      # the fp16 form ran (not a fallback form)
    us.close()
    # the context is usable afterwards and the flag is clear
    got = _scores(ctx, opt, dm, frame_off, feats, pl, 2, 2)
    _assert_exact(m, gc, feats, frame_off, pl, got)


def test_k1_prof_stamps_leave_scores_alone(ctx, opt, capfd):
    """Option k1_prof = 1 (boundary stamps of every chunk, one line on stderr): same scores, both launch shapes."""
    opt.k1("f16x2s")
    m, gc, dm, frame_off, feats, pl = _feature_set(ctx, 12, 64, 40, _tiles(15), seed=3, pdf_list=np.arange(12))
    old = _scores(ctx, opt, dm, frame_off, feats, pl, 1, 0)
    nch = len(_chunks_in_utterance_order(np.diff(frame_off), 15))
    opt("k1_prof", 1)
    for launch, pgrid in ((1, 0), (2, 2)):
        capfd.readouterr()
        got = _scores(ctx, opt, dm, frame_off, feats, pl, launch, pgrid)
        assert all(np.array_equal(a, b) for a, b in zip(old, got))
        err = capfd.readouterr().err
        assert "[KHG_K1_PROF]" in err and "%d chunks" % nch in err, err
