"""The waveform front end on the device under every option branch and FFT size: cases.OPTION_CASES names one
option set for every line of k_fe_wave that the defaults of tests/test_gpu_wave.py never reach -- the other windows, preemph_coeff 0
and 1, no DC removal, N = 256 and 1024, L == N, S > L and S = 1, 3 to 128 mel bins with empty filters, up to 128 cepstra, a lifter of
ones, the largest frame shift the LDS limit accepts.  The batch is cases.option_batch_lengths: eleven utterances of 0 .. 5, F - 1, F,
F + 1, 2 F + 1 and 37 frames, the smallest in which every tile shape and every pattern of idle waves occurs.

As in the sibling file the mel energies must equal the numpy host form ON THE BITS, what follows the log is compared within the
rounding of the log carried through the DCT, and six cases also meet the float64 restatement within the derived bound.  Then the
empty filters, the LDS ceiling, two handles with different dynamic-LDS sizes alive together, one non-finite sample inside an
utterance, and full-scale signals.  The host forms are computed once per option set and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_cases as cases  # noqa: E402
import wave_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = list(cases.OPTION_CASES)
U24 = 2.0 ** -24
LOG_EPS = np.float32(np.log(np.float64(np.finfo(np.float32).eps)))
_cache = {}


def _o(name, snip, **kw):
    return cases.case_opts(name, snip_edges=snip, **kw)


def _waves(name, o):
    """the case's batch under o's edge mode and shift: whole-number samples, so that int16 and float32 hold the same values"""
    key = ("waves", name, o["snip_edges"]) + ref.dims(o)
    if key not in _cache:
        _cache[key] = cases.option_waves(o, dc=cases.case_dc(name))
    return _cache[key]


def _host(name, o):
    """host form of every utterance of the case's batch under o, computed once"""
    import kaldi_hmm_gmm_amd as khg
    key = ("host", name, tuple(sorted(o.items())))
    if key not in _cache:
        lo = cases.lib_opts(o)
        fn = khg.compute_mfcc_feats if o["kind"] == "mfcc" else khg.compute_fbank_feats
        _cache[key] = [fn(w, lo) for w in _waves(name, o)]
    return _cache[key]


def _device(ctx, o, waves, stype="f32"):
    import kaldi_hmm_gmm_amd as khg
    if stype == "i16":
        waves = [w.astype(np.int16) for w in waves]
    fn = khg.compute_mfcc_feats_batch if o["kind"] == "mfcc" else khg.compute_fbank_feats_batch
    fo, t = fn(ctx, waves, cases.lib_opts(o))
    return fo, t.cpu().numpy()


def _rows(fo, x):
    return [x[fo[i]:fo[i + 1]] for i in range(len(fo) - 1)]


def _assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    first = [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in np.argwhere(bad)[:5]]
    assert not bad.any(), (what, int(bad.sum()), first)


def _cepstra_bound(lm, tab):
    """sum_b |dct_cb| lifter_c 2 ulp(lm_b) plus the DCT chain's own (B + 1) 2^-24 sum_b |terms| (the sibling file's formula)"""
    dct, lif = np.abs(tab["dct"].astype(np.float64)), np.abs(tab["lifter"].astype(np.float64))
    B = dct.shape[1]
    return ((2.0 * np.spacing(np.abs(lm)).astype(np.float64)) @ dct.T + (B + 1) * U24 * (np.abs(lm.astype(np.float64)) @ dct.T)) * lif[None, :]


# ---- a. mel energies on the bits ----
@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_mel_energies_on_the_bits(ctx, name, snip):
    import kaldi_hmm_gmm_amd as khg
    assert (cases.TILE_FRAMES, cases.TILE_LDS_BYTES) == (khg.FE_TILE_FRAMES, khg.FEAT_TILE_LDS_BYTES)
    for power in (True, False):
        o = _o(name, snip, kind="fbank", use_log_fbank=False, use_power=power)
        waves = _waves(name, o)
        lo = cases.lib_opts(o)
        T = [khg.num_frames(lo, len(w)) for w in waves]
        assert T[:11] == [0, 1, 2, 3, 4, 5, 15, 16, 17, 33, 37] and 11 <= len(waves) <= 13 and sum(T) <= 135
        want = np.concatenate(_host(name, o))
        for stype in ("f32", "i16"):
            fo, got = _device(ctx, o, waves, stype)
            assert fo.dtype == np.int64 and fo.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
            assert got.shape == (sum(T), o["num_mel_bins"])
            _assert_bits(got, want, (name, snip, power, stype))
    assert np.isfinite(want).all() and (want >= 0).all() and (want > 0).any()


# ---- b. what follows the log ----
@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_log_mel_cepstra_and_energies(ctx, name, snip):
    """log-mel and both log-energies within 2 float ulps of the host form (their arguments are the same bits; the two logs round on
    their own); the cepstra, with C0 and with the energy in column 0, from float32 and from int16 samples, within sum_b |dct_cb|
    lifter_c 2 ulp(lm_b) plus the DCT chain's (B + 1) 2^-24 sum_b |terms|; for c1 a floor that binds on some frames only.
    Measured on an MI355X: 2 ulps at most; cepstra largest error / bound 0.46 (b3, a bound of three terms), 0.14 at 23 bins."""
    import kaldi_hmm_gmm_amd as khg
    worst_u = 0.0
    for raw in (False, True):
        o = _o(name, snip, kind="fbank", use_energy=True, raw_energy=raw)
        _, got = _device(ctx, o, _waves(name, o))
        lm = np.concatenate(_host(name, o))
        u = cases.ulps(got, lm)
        worst_u = max(worst_u, float(u.max()))
        assert got.shape == lm.shape and np.isfinite(got).all() and (u <= 2).all(), (raw, float(u.max()))
    worst = 0.0
    for kw in (dict(), dict(use_energy=True, raw_energy=True), dict(use_energy=True, raw_energy=False)):
        if kw and name == "c1" and kw["raw_energy"]:
            kw["energy_floor"] = 9.0e6 * 400                     # the raw energy of a noise-only frame (sigma 3000): the floor binds on some
        om = _o(name, snip, kind="mfcc", **kw)
        waves = _waves(name, om)
        lm = np.concatenate(_host(name, dict(om, kind="fbank", use_energy=False)))      # the log-mel of the same frames (the host form has no LDS limit)
        want = np.concatenate(_host(name, om))
        bound = _cepstra_bound(lm, khg.frontend_tables(cases.lib_opts(om)))
        e0 = 1 if kw else 0
        assert (bound[:, e0:] > 0).all()
        for stype in ("f32", "i16"):
            _, got = _device(ctx, om, waves, stype)
            assert got.shape == want.shape == (len(lm), om["num_ceps"]) and np.isfinite(got).all()
            err = np.abs(got.astype(np.float64) - want.astype(np.float64))
            if om["num_ceps"] > e0:
                worst = max(worst, float((err[:, e0:] / bound[:, e0:]).max()))
            assert (err[:, e0:] <= bound[:, e0:]).all(), (kw, stype)
            if e0:
                assert (cases.ulps(got[:, 0], want[:, 0]) <= 2).all()
            if "energy_floor" in kw:
                floor = np.float32(np.log(np.float64(np.float32(kw["energy_floor"]))))
                assert (got[:, 0] >= floor).all() and (got[:, 0] == floor).any() and (got[:, 0] > floor).any()
            if name == "c128" and not kw:                        # the DCT loop's second trip: lanes 0 .. 63 again, cepstra 64 .. 127
                assert (err[:, 64:] <= bound[:, 64:]).all() and (got[:, 64:] != 0).any() and (want[:, 64:] != 0).any()
                assert (np.abs(got[:, 64:]).max(0) > 0).all()
    print("%s snip=%s: log-mel and log-energies: largest difference %.3g ulp; cepstra: largest error / bound %.3g" % (name, snip, worst_u, worst))


# ---- c. against the restatement ----
@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", ["n1024", "preemph0", "nodc_rect_c0", "l_eq_n_256", "b128_8k", "c128"])
def test_against_the_restatement_within_the_derived_bound(ctx, name, snip):
    """device against tests/wave_ref.py (float64, an explicit DFT) on every non-empty utterance: log-mel and cepstra within the bound
    of DESIGN.md 7q with K = ref.bound_roundings(o).  Measured on an MI355X: largest error / bound 0.25 (log-mel, nodc_rect_c0 and
    preemph0; 0.24 at 128 bins) and 0.062 (cepstra)."""
    worst = {}
    for kind in ("fbank", "mfcc"):
        o = _o(name, snip, kind=kind)
        waves = _waves(name, o)
        fo, got = _device(ctx, o, waves)
        rows = _rows(fo, got)
        worst[kind], seen = 0.0, 0
        for i, w in enumerate(waves):
            if len(rows[i]) == 0:
                continue
            want, det = ref.features(w, o, detail=True)
            lmb = ref.log_mel_bound(o, det)
            bound = ref.cepstra_bound(o, lmb) if kind == "mfcc" else lmb
            ratio = np.abs(rows[i] - want) / bound
            worst[kind] = max(worst[kind], float(ratio.max()))
            seen += len(want)
            assert rows[i].shape == want.shape and (ratio <= 1.0).all(), (kind, i, float(ratio.max()))
        assert seen == len(got) >= 133
    print("%s snip=%s: largest error / bound: log-mel %.3g, cepstra %.3g (K = %d)" % (name, snip, worst["fbank"], worst["mfcc"], ref.bound_roundings(o)))


# ---- d. empty filters ----
@pytest.mark.parametrize("name", ["b128_16k", "b128_8k"])
def test_empty_filters_give_zero_and_the_floor(ctx, name):
    import kaldi_hmm_gmm_amd as khg
    o = _o(name, True, kind="fbank", use_log_fbank=False)
    tab = khg.frontend_tables(cases.lib_opts(o))
    empty = np.flatnonzero(tab["mel_len"] == 0)
    assert len(empty) >= 1
    _, got = _device(ctx, o, _waves(name, o))
    assert len(got) >= 133 and (got[:, empty].view(np.uint32) == 0).all()      # +0.0, not -0.0, on every frame
    full = np.setdiff1d(np.arange(o["num_mel_bins"]), empty)
    assert (got[:, full] > 0).all()
    o = dict(o, use_log_fbank=True)
    _, got = _device(ctx, o, _waves(name, o))
    assert (cases.ulps(got[:, empty], LOG_EPS) <= 2).all() and (got[:, full] > 0).all()


# ---- e. the LDS ceiling ----
@pytest.mark.parametrize("kw", [dict(kind="mfcc"), dict(kind="fbank", use_log_fbank=False), dict(kind="fbank", use_energy=True)], ids=["mfcc13", "mel23", "fbank24"])
def test_the_lds_ceiling(ctx, kw):
    """the largest S that 7q's formula admits, from the library's own dims and tables: the batch runs there and equals the host form;
    at S + 1 the handle and the batch call are refused with "LDS" before any launch"""
    import torch

    import kaldi_hmm_gmm_amd as khg
    base = cases.lib_opts(ref.opts(**kw))
    d, tab = khg.frontend_dims(base), khg.frontend_tables(base)
    assert d["num_weights"] == len(tab["mel_w"]) == int(tab["mel_len"].sum())

    def nbytes(S):
        return 4 * (15 * S + 2 * d["L"] + d["N"] + d["num_weights"] + 3 * d["num_mel_bins"] + 4 * (3 * d["N"] // 2 + 128) + 16 * d["dim"])

    S = max(s for s in range(1, 2000) if nbytes(s) <= khg.FEAT_TILE_LDS_BYTES)
    assert nbytes(S) <= khg.FEAT_TILE_LDS_BYTES < nbytes(S + 1) and S > d["L"]
    o = _o("lds_ceiling", True, **kw)
    assert khg.frontend_dims(cases.lib_opts(o))["S"] == S == cases.lds_ceiling_shift(o) and o["frame_shift_ms"] == S / 16.0
    print("%s: S = %d at %d bytes" % (kw, S, nbytes(S)))
    waves = _waves("lds_ceiling", o)
    fe = khg.DeviceFrontend(ctx, cases.lib_opts(o))
    fn = khg.compute_mfcc_feats_batch if kw["kind"] == "mfcc" else khg.compute_fbank_feats_batch
    fo, t = fn(ctx, waves, fe)
    fe.close()
    got, want = t.cpu().numpy(), np.concatenate(_host("lds_ceiling", o))
    assert fo[-1] == len(want) >= 133
    if not o["use_log_fbank"]:
        _assert_bits(got, want, kw)
    elif kw["kind"] == "fbank":
        assert (cases.ulps(got, want) <= 2).all()
    else:
        lm = np.concatenate(_host("lds_ceiling", dict(o, kind="fbank")))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= _cepstra_bound(lm, khg.frontend_tables(cases.lib_opts(o)))).all()
    over = cases.lib_opts(dict(o, frame_shift_ms=(S + 1) / 16.0))
    assert khg.frontend_dims(over)["S"] == S + 1
    with pytest.raises(Exception, match="LDS"):
        khg.DeviceFrontend(ctx, over)
    x = cases.noise(d["L"] + 2 * (S + 1), 3)
    out = torch.full((3, d["dim"]), 7.0, dtype=torch.float32, device="cuda:%d" % ctx.device)
    assert khg.num_frames(over, len(x)) == 3
    with pytest.raises(Exception, match="LDS"):
        fn(ctx, [x], over, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- f. handles side by side ----
def test_two_handles_with_different_lds_side_by_side(ctx):
    """the dynamic-LDS attribute belongs to the function, not the handle: a handle above 48 KiB (N = 1024) and one below, alive
    together, used in turn, each give the bits of their first result and of the host form"""
    import kaldi_hmm_gmm_amd as khg
    kw = dict(kind="fbank", use_log_fbank=False)
    o_big, o_small = _o("n1024", True, **kw), _o("c1", True, **kw)      # c1's filterbank is the defaults'
    assert o_small == ref.opts(num_ceps=1, **kw)
    d = khg.frontend_dims(cases.lib_opts(o_big))
    w = khg.frontend_tables(cases.lib_opts(o_big))
    assert cases.lds_bytes(d["L"], d["S"], d["N"], len(w["mel_w"]), d["num_mel_bins"], d["dim"]) > 48 * 1024
    d = khg.frontend_dims(cases.lib_opts(o_small))
    assert cases.lds_bytes(d["L"], d["S"], d["N"], d["num_weights"], d["num_mel_bins"], d["dim"]) < 48 * 1024
    big, small = khg.DeviceFrontend(ctx, cases.lib_opts(o_big)), khg.DeviceFrontend(ctx, cases.lib_opts(o_small))
    first = {}
    for which in ("small", "big", "small", "big"):
        fe, o, name = (small, o_small, "c1") if which == "small" else (big, o_big, "n1024")
        fo, t = khg.compute_fbank_feats_batch(ctx, _waves(name, o), fe)
        got = t.cpu().numpy()
        _assert_bits(got, np.concatenate(_host(name, o)), which)
        assert first.setdefault(which, got.tobytes()) == got.tobytes()
    big.close()
    small.close()


# ---- g. a frame depends on its own samples only, inside one utterance ----
@pytest.mark.parametrize("snip", [True, False])
def test_one_bad_sample_reaches_its_own_frames_only(ctx, snip):
    """one sample NaN, then +Inf, at index 0, mid-utterance and at n - 1 of a 37-frame utterance: exactly the frames whose L indices
    cover it after reflection are non-finite in every cell, every other frame has the bits of the clean run -- the frames of a tile
    share the workgroup's zr / zi / pw / lm buffers and its barriers, and nothing may cross between them"""
    import kaldi_hmm_gmm_amd as khg
    o = ref.opts(snip_edges=snip, use_energy=True)
    lo = cases.lib_opts(o)
    L, S, _ = ref.dims(o)
    n = L + 36 * S if snip else 37 * S - S // 2 + 5      # with snip_edges the last frame ends at n - 1
    x = cases.noise(n, 31, tone=True)
    starts = khg.frame_starts(lo, n)
    assert len(starts) == 37
    idx = (starts[:, None] + np.arange(L)[None, :]) % (2 * n)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    assert idx.min() >= 0 and idx.max() < n and (snip or (idx[0, :40] == np.arange(119, 79, -1)).all())
    for fn in (khg.compute_mfcc_feats_batch, khg.compute_fbank_feats_batch):
        _, t = fn(ctx, [x], lo)
        clean = t.cpu().numpy()
        assert np.isfinite(clean).all() and len(clean) == 37
        for pos in (0, 17 * S + 123, n - 1):
            hit = (idx == pos).any(1)
            assert 1 <= hit.sum() <= 4 and not hit.all()
            for bad in (np.nan, np.inf):
                y = x.copy()
                y[pos] = bad
                _, t = fn(ctx, [y], lo)
                got = t.cpu().numpy()
                assert (~np.isfinite(got[hit])).all(), (pos, bad, np.flatnonzero(np.isfinite(got[hit]).any(1)).tolist())
                assert got[~hit].tobytes() == clean[~hit].tobytes(), (pos, bad, np.flatnonzero((got[~hit] != clean[~hit]).any(1)).tolist())


# ---- h. full-scale and degenerate signals ----
def test_full_scale_and_degenerate_signals(ctx):
    """a constant 32767, the alternating 32767, -32768 (all energy at Nyquist, the bin that is never formed) and one full-scale
    impulse in silence, float32 and int16: the bits of the host form without the log, 2 ulps with it, finite throughout; the
    constant with DC removal leaves nothing, log(FLT_EPSILON) in every cell"""
    n = 3000
    const = np.full(n, 32767.0, np.float32)
    alt = np.where(np.arange(n) % 2 == 0, 32767.0, -32768.0).astype(np.float32)
    imp = np.zeros(n, np.float32)
    imp[1234] = -32768.0
    waves = [const, alt, imp]
    import kaldi_hmm_gmm_amd as khg
    for dc in (True, False):
        for log in (False, True):
            o = ref.opts(kind="fbank", remove_dc_offset=dc, use_log_fbank=log)
            want = [khg.compute_fbank_feats(w, cases.lib_opts(o)) for w in waves]
            for stype in ("f32", "i16"):
                fo, got = _device(ctx, o, waves, stype)
                assert fo.tolist() == [0, 17, 34, 51] and np.isfinite(got).all()
                if log:
                    assert (cases.ulps(got, np.concatenate(want)) <= 2).all(), (dc, stype)
                else:
                    _assert_bits(got, np.concatenate(want), (dc, stype))
                if dc and log:
                    assert (cases.ulps(got[:17], LOG_EPS) <= 2).all() and abs(float(want[0][0, 0]) + 15.942385) < 1e-6
                if not dc:
                    assert (got[:17] > (0 if not log else LOG_EPS)).all()      # the constant is still there
