"""Every form and instantiation of K1 on inputs built for it (tests/k1_form_cases.py): the call reports the record the case names
-- UtteranceSet.k1_last(): the form that ran, the hand-overs from the fp16 forms, packing, launch shape, chunks, order, shifted
tiles, slices, what was packed -- so a model, a set or a rule that takes a test to another kernel fails here instead of passing
there; and the scores are those of the float64 yardstick at the project's tolerance, 1e-5 + 1e-6 B.

Every call runs on a score block filled with a poison value.  For the calls that skip cells (from a pdf's first needed tile on; the
band) the same form's full run on a second set is the reference: needed cells are equal bit for bit, the whole tiles in front of
the first needed frame stay untouched, per pdf (32 frames for f16x2s, 16 for the others, clamped at 255 / 127 tiles; every cell
in front where f16x2s shifts its tiles), every other cell in front is untouched or the full run's, and cells behind a band are the
full run's or one fill value per row that bounds the row from above."""
import dataclasses

import numpy as np
import pytest

import k1_form_cases as kc
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

POISON = np.float32(12345.0)


def _model(ctx, b):
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions
    dm = DeviceModel(ctx, b.m.gauss_off, b.gc, b.m.means_invvars, b.m.inv_vars)
    tm = DeviceTransitions(ctx, b.id2pdf) if b.graphs is not None else None
    return dm, tm


def _set(ctx, b, tm):
    from kaldi_hmm_gmm_amd import UtteranceSet
    us = UtteranceSet(ctx, tm, np.array(b.frame_off, np.int64), np.array(b.feats, np.float32), graphs=b.graphs)      # (copies: the case's arrays are shared)
    if b.graphs is None:
        us.set_pdf_list(np.array(b.case.plist, np.int32))
    return us


def _poison(us, b):
    lens = np.diff(b.frame_off)
    if sum(len(l) * int(T) for l, T in zip(b.lists, lens)):
        us.upload_loglikes([np.full((len(l), int(T)), POISON, np.float32) for l, T in zip(b.lists, lens)])


def _call(us, dm, call):
    us.loglikes(dm, reachable_only=call == "reach", band=call == "band")


def _options(opt, c, **more):
    opt.k1(c.k1)
    for k, v in list(c.opts) + sorted(more.items()):
        opt(k, v)


def _run(ctx, b, dm, tm, call):
    """the call on a fresh, poisoned set -> (set, scores, record)"""
    us = _set(ctx, b, tm)
    assert us.k1_last() is None, "no call yet"
    _poison(us, b)
    _call(us, dm, call)
    return us, us.download_loglikes(), us.k1_last()


def _assert_yardstick(b, got, name):
    worst = 0.0
    for u in range(len(b.lists)):
        assert got[u].shape == b.exact[u].shape, (name, u)
        if not got[u].size:
            continue
        tol = kc.tolerance(b.bound[u], b.case.D)
        err = np.abs(got[u] - b.exact[u])
        assert np.isfinite(got[u]).all() and (err <= tol).all(), f"{name} utt {u}: max err/tol {(err / tol).max()} at {np.unravel_index((err / tol).argmax(), err.shape)}"
        worst = max(worst, float((err / tol).max()))
    return worst


def _assert_cells(b, rec, part, full, name):
    """the skipping rules of the module's docstring, for a call that reported `rec`"""
    c = b.case
    form, band = rec["form"], rec["mode"] == 2
    granule = 32 if form == "f16x2s" else 16
    clamp = {"f16x2s": 255, "f16x2": 127, "utt": 127, "pdf": 10**9}[form]
    shifting = form == "f16x2s" and rec["pack"] == 1 and (band or rec["tail_shift"])
    untouched = filled = shifted = 0
    for u in range(len(b.lists)):
        T = int(b.frame_off[u + 1] - b.frame_off[u])
        one_chunk = (T + 31) // 32 <= rec["per"]
        for j, p in enumerate(b.lists[u]):
            row, ref = part[u][j], full[u][j]
            first, last = b.first[u][int(p)], b.last[u][int(p)]
            f = min(first, T)
            # whole granules in front of the first needed frame stay untouched, per pdf (a packed group, f16x2's 32-frame tiles and
            # the utterance-major form compute some of them all the same, but do not write them)
            skip = min(T, granule * min(clamp, first // granule))
            lo, hi = f, T
            if band:
                hi = min(T, 32 * (last // 32 + 1)) if last >= 0 else f
            shift = kc.shift_of(first, last, T, "band" if band else "reach", rec["shift_mode"]) if shifting else 0
            if shift:
                s0 = 32 * (first // 32) + shift
                took = bool((row[32 * (first // 32): s0] == POISON).all())
                assert took or not one_chunk, (name, u, int(p), "a band inside one chunk keeps aligned tiles")
                if took:
                    shifted += 1
                    skip = s0
                    if band:
                        hi = min(T, s0 + 32 * (last // 32 - first // 32))
            hi = max(hi, lo)
            assert not band or last < 0 or last < hi or f == T, (name, u, int(p))
            assert np.array_equal(row[lo:hi], ref[lo:hi]), (name, u, int(p), "needed cells differ from the full run")
            front = row[:lo]
            assert ((front == POISON) | (front == ref[:lo])).all(), (name, u, int(p), "a cell in front is neither untouched nor the full run's")
            assert int((front == POISON).sum()) >= skip, (name, u, int(p), int((front == POISON).sum()), skip)
            untouched += int((front == POISON).sum())
            tail, tref = row[hi:], ref[hi:]
            other = tail[tail != tref]
            if other.size:
                assert band and (other == other[0]).all(), (name, u, int(p), "cells behind the band hold more than one fill value")
                assert other[0] >= b.exact[u][j].max(), (name, u, int(p), "the fill is no upper bound of the row")
                assert last < 0 or other[0] != POISON, (name, u, int(p), "cells behind the band were left untouched")
                filled += other.size
    return untouched, filled, shifted


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_form_case(ctx, opt, name):
    b = kc.build(name)
    c = b.case
    _options(opt, c)
    dm, tm = _model(ctx, b)
    us, got, rec = _run(ctx, b, dm, tm, c.call)
    print(name, rec)
    assert rec == c.expect, {k: (rec[k], c.expect[k]) for k in rec if rec[k] != c.expect[k]}
    assert kc.instantiations(rec) == kc.instantiations(c.expect)
    if b.graphs is not None:
        poff, pdfs = us.pdf_lists()
        fd, ld = us.pdf_first_frames(), us.pdf_last_frames()
        for u in range(len(b.lists)):
            assert pdfs[poff[u]: poff[u + 1]].tolist() == b.lists[u].tolist()
            assert fd[poff[u]: poff[u + 1]].tolist() == [b.first[u][int(p)] for p in b.lists[u]], (name, u)
            assert ld[poff[u]: poff[u + 1]].tolist() == [b.last[u][int(p)] for p in b.lists[u]], (name, u)
    # the same call again: nothing is packed twice, the plan is the same, the bits are the same
    _call(us, dm, c.call)
    assert us.k1_last() == dict(c.expect, repacked=0)
    again = us.download_loglikes()
    assert all(np.array_equal(a, g) for a, g in zip(again, got)), name
    us.close()
    if rec["form"] == "none":
        assert all(g.size == 0 for g in got)
    elif rec["mode"] == 0:
        print(name, "worst err/tol", _assert_yardstick(b, got, name))
        assert not any((g == POISON).any() for g in got)
    else:
        # the same form's full run (a second set, the same model: its image is packed already)
        us2, full, rec2 = _run(ctx, b, dm, tm, "full")
        want2 = dict(c.expect, mode=0, tail_shift=0, repacked=c.expect["repacked"] & 1)
        if rec["form"] == "utt" and dict(c.opts).get("k1_interleave", -1) < 0:
            want2["interleave"] = 0
        if rec["form"] == "pdf":
            want2 = dict(want2, **{k: rec2[k] for k in ("nb_slices", "chunks", "grid")})       # (more tiles: maybe more slices)
        assert rec2 == want2, {k: (rec2[k], want2[k]) for k in rec2 if rec2[k] != want2[k]}
        print(name, "full run: worst err/tol", _assert_yardstick(b, full, name))
        untouched, filled, shifted = _assert_cells(b, rec, got, full, name)
        print(name, "untouched cells in front", untouched, "filled behind", filled, "shifted bands", shifted)
        assert untouched > 0
        if rec["mode"] == 2:
            assert filled > 0
        if rec["form"] == "f16x2s" and rec["pack"] == 1 and rec["shift_mode"] and c.graphs in (kc.G4, kc.G17, kc.GE):
            assert shifted > 0
        us2.close()
    if c.bitwise:
        # one Gaussian per pdf: the log-sum-exp of one term is that term, the MFMA contraction is the oracle's k-ordered fmaf chain
        m = b.m
        for u in range(len(b.lists)):
            x = b.feats[b.frame_off[u]: b.frame_off[u + 1]]
            for j, p in enumerate(b.lists[u]):
                g0 = int(m.gauss_off[p])
                want = np.array([orc.loglikes(b.gc[g0:g0 + 1], m.means_invvars[g0:g0 + 1], m.inv_vars[g0:g0 + 1], x[t], fma_order=True)[0] for t in range(len(x))], np.float32)
                assert np.array_equal(got[u][j], want), (name, u, j)
    if tm is not None:
        tm.close()
    dm.close()


def stated_bound(form, first, T):
    """untouched cells in front of a pdf's first needed frame, stated per pdf for every form: granule x min(clamp, first // granule), the
    granule 32 frames for f16x2s (packed or not) and 16 for f16x2, the utterance-major and the pdf-major form, the clamp 255 tiles for
    f16x2s, 127 for f16x2 and the utterance-major form, none for the pdf-major form"""
    granule = 32 if form == "f16x2s" else 16
    clamp = {"f16x2s": 255, "f16x2": 127, "utt": 127, "pdf": 10**9}[form]
    return min(T, granule * min(clamp, first // granule))


@pytest.mark.parametrize("name", [c.name for c in kc.CASES if c.graphs and c.call != "full" and c.expect["form"] != "none"])
def test_untouched_cells_reach_the_stated_bound(ctx, opt, name):
    """Per (utterance, pdf) the cells left untouched in front of the first needed frame reach stated_bound, in every form.

    Three kernels compute more than that in front of a pdf's first needed frame -- four or two pdfs per tile
    (k1s_loglikes_packed) start a group at the earliest first needed tile among its pdfs, f16x2 (k1h_loglikes) walks 32-frame tiles,
    the utterance-major form (k1_loglikes) skips at most two tiles per wave -- and used to write it: the pdfs first needed at
    frames 64 and 65 grouped with 33 and 40 had 32 untouched cells against 64, f16x2 0 against 16 and 2 016 against 2 032, the
    utterance-major form 0 against 16 / 32 / 70 and 752 against 2 032.  They now keep those values out of the score block (the
    store is predicated on the pdf's own first needed tile), as the one-pdf f16x2s kernel and the pdf-major form always did."""
    b = kc.build(name)
    c = b.case
    _options(opt, c)
    dm, tm = _model(ctx, b)
    us, got, rec = _run(ctx, b, dm, tm, c.call)
    us.close(); tm.close(); dm.close()
    short = []
    for u in range(len(b.lists)):
        T = int(b.frame_off[u + 1] - b.frame_off[u])
        for j, p in enumerate(b.lists[u]):
            first = b.first[u][int(p)]
            n, want = int((got[u][j, :min(first, T)] == POISON).sum()), stated_bound(rec["form"], first, T)
            if n < want:
                short.append((u, int(p), first, n, want))
    print(name, rec["form"], "pack", rec["pack"], "(utterance, pdf, first, untouched, bound) short of the bound:", short)
    assert not short, short


def _scores(ctx, opt, name, call=None, **more):
    """scores and record of a case's set under further options (a fresh model and set each time)"""
    b = kc.build(name)
    _options(opt, b.case, **more)
    dm, tm = _model(ctx, b)
    us, got, rec = _run(ctx, b, dm, tm, call or b.case.call)
    us.close()
    if tm is not None:
        tm.close()
    dm.close()
    return b, got, rec


@pytest.mark.parametrize("name", ["s40_17", "s41_17", "s40_g17_band", "s41_g17_reach"])
def test_chunk_order_changes_no_bit(ctx, opt, name):
    """k1_order 0 .. 4 on 17 utterances (the persistent launch): which workgroup takes which chunk when, empty work items included
    (order 4), changes no score and no untouched cell"""
    ks = kc.ks_of(kc.BY_NAME[name].D)
    _, base, rec0 = _scores(ctx, opt, name)
    assert rec0["order"] == (4 if ks == 10 else 0)
    seen = {rec0["chunks"]}
    for o in (1, 2, 3, 4):
        _, got, rec = _scores(ctx, opt, name, k1_order=o)
        assert rec["order"] == o and rec["persistent"] == 1
        seen.add(rec["chunks"])
        assert all(np.array_equal(a, g) for a, g in zip(base, got)), (name, o)
    assert len(seen) == 2 or name.endswith(("g17_band", "g17_reach")), "order 4 adds its empty work items"


def test_shift_experiments_change_no_needed_cell(ctx, opt):
    """k1_dbg 32 (no shifted tiles) and 64 (only the sixteen-frame shift) against the default on every cell of every band"""
    b, base, rec0 = _scores(ctx, opt, "s40_g4_band")
    for dbg, mode in ((32, 0), (64, 1)):
        _, got, rec = _scores(ctx, opt, "s40_g4_band", k1_dbg=dbg)
        assert rec == dict(rec0, shift_mode=mode)
        for u in range(len(b.lists)):
            for j, p in enumerate(b.lists[u]):
                f, l = b.first[u][int(p)], b.last[u][int(p)]
                assert np.array_equal(got[u][j, f: l + 1], base[u][j, f: l + 1]), (dbg, u, int(p))


@pytest.mark.parametrize("name", ["p40", "p77", "p40_300", "p40_g4_reach", "p40_long_reach"])
def test_pdf_major_slices_change_no_bit(ctx, opt, name):
    """k1p_ts 1, 3 and 1024: a tile's value does not depend on the slice it falls into, nor on where in its entry the slice starts"""
    b, base, rec0 = _scores(ctx, opt, name, k1p_ts=1024)
    assert rec0["form"] == "pdf"
    for ts in (1, 3):
        _, got, rec = _scores(ctx, opt, name, k1p_ts=ts)
        assert rec["per"] == ts and rec["chunks"] > rec0["chunks"] and sum(rec["nb_slices"]) == rec["chunks"]
        case = dataclasses.replace(b.case, opts=tuple(sorted(dict(b.case.opts, k1p_ts=ts).items())))
        assert rec == dict(kc.restate(dataclasses.replace(b, case=case)), repacked=rec0["repacked"])
        assert all(np.array_equal(a, g) for a, g in zip(base, got)), (name, ts)


@pytest.mark.parametrize("first", ["larger", "smaller"])
@pytest.mark.parametrize("D", [40, 41])
def test_two_sets_share_the_models_exponents(ctx, opt, D, first):
    """Two sets whose features differ by 2^6 in one dimension, scored in turn against ONE model, which keeps the element-wise minimum
    of the feature exponents of the sets it has scored.  The set with the larger features first: the other set packs its planes
    with the model's exponents from its first call on, so after the first round no call packs anything.  The other way round the
    second set lowers the model's exponents and takes the image with it (one re-pack), and the first set, whose planes were made
    with its own, packs them once more in the second round -- planes only, never the image again; nothing after that."""
    from kaldi_hmm_gmm_amd import UtteranceSet
    opt.k1("auto")
    b = kc.build("s%d_17" % D)
    dm, _ = _model(ctx, b)
    big = np.array(b.feats, np.float32)
    small = big.copy()
    small[:, 3] *= np.float32(1.0 / 64.0)
    for feats in (big, small):          # both sets are inside f16x2s' domain by themselves (the restated check)
        xk, wk, gcmax = kc.column_maxima(b.m, b.gc, feats, 16 * kc.ks_of(D))
        assert kc.split_domain(xk, wk, gcmax) and kc.f16x2s_scales(xk, wk)
    pl = np.array(b.case.plist, np.int32)
    sets, exact = [], []
    for feats in ((big, small) if first == "larger" else (small, big)):
        us = UtteranceSet(ctx, None, np.array(b.frame_off, np.int64), feats)
        us.set_pdf_list(pl)
        sets.append(us)
        exact.append([kc.exact_loglikes(b.m, b.gc, feats[b.frame_off[u]: b.frame_off[u + 1]], pl) for u in range(len(b.lists))])
    packed = []
    for rnd in range(3):
        for k, us in enumerate(sets):
            _poison(us, b)
            us.loglikes(dm)
            rec = us.k1_last()
            assert rec["form"] == "f16x2s" and rec["declined"] == 0, rec
            packed.append(rec["repacked"])
            got = us.download_loglikes()
            for u, (e, bound) in enumerate(exact[k]):
                if got[u].size:
                    assert (np.abs(got[u] - e) <= kc.tolerance(bound, D)).all(), (rnd, k, u)
    print("repacked per call:", packed)
    assert packed == ([3, 1, 0, 0, 0, 0] if first == "larger" else [3, 3, 1, 0, 0, 0]), packed
    for us in sets:
        us.close()
    dm.close()


@pytest.mark.parametrize("D", [40, 72])
def test_band_then_repair_is_reported(ctx, opt, D):
    """band scores, then an alignment whose exact DP certifies nothing (max_active set): khg_align's repair launch (k1s_repair<5>,
    <10>) recomputes the utterances and the record says so until the next K1 call"""
    from helpers import build
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    opt.k1("f16x2s")
    m, gc, om, ut, cost = build(12, 64, D, n_utt=6, seed=41 + D, min_phones=2, max_phones=12)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    us = UtteranceSet(ctx, tm, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm)
    full = us.download_loglikes()
    res_full = us.align(tm, beam=200.0, retry_beam=0.0, acoustic_scale=0.1, max_active=100000)
    assert us.k1_last()["repaired"] == 0 and us.k1_last()["mode"] == 0
    us.loglikes(dm, band=True)
    rec = us.k1_last()
    assert (rec["form"], rec["K"], rec["mode"], rec["pack"], rec["repaired"]) == ("f16x2s", kc.ks_of(D), 2, 1, 0), rec
    res = us.align(tm, beam=200.0, retry_beam=0.0, acoustic_scale=0.1, max_active=100000)
    assert ((res["status"] & 8) != 0).all(), "max_active was meant to send every utterance through the repair launch"
    assert us.k1_last() == dict(rec, repaired=1)
    assert np.array_equal(res["ali"], res_full["ali"])
    got = us.download_loglikes()
    poff, pdfs = us.pdf_lists()
    first = us.pdf_first_frames()
    for u in range(us.n_utt):
        for j in range(poff[u + 1] - poff[u]):
            t0 = 32 * (min(int(first[poff[u] + j]), 10**6) // 32)
            assert np.array_equal(got[u][j, t0:], full[u][j, t0:]), (u, j)
    us.loglikes(dm, band=True)
    assert us.k1_last()["repaired"] == 0
    us.close(); tm.close(); dm.close()
