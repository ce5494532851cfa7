"""MFCC and filterbank features from waveforms on the device: khg_frontend_compute through
compute_mfcc_feats_batch / compute_fbank_feats_batch on a ragged batch of about 40 utterances -- empty ones, ones shorter than a
frame, the lengths around a frame and around the kernel's tile, a few of 300 to 700 frames -- at three shapes, with and without
snip_edges, from float32 and from int16 samples.

The mel energies (FBANK without the log, power and magnitude spectrum) must equal the numpy host form ON THE BITS: that covers the
staging, the reflection, the butterfly schedule, the post-pass and the mel chains end to end.  What follows the log is compared
within the rounding of the log (2 float ulps) carried through the DCT, and against the float64 restatement (tests/wave_ref.py)
within the derived bound of the CPU tests.  The host forms and the restatement are computed once per shape and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_cases as cases  # noqa: E402
import wave_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = sorted(cases.SHAPES)
U24 = 2.0 ** -24
_cache = {}


def _waves(shape, snip):
    """the batch: whole-number samples (so that int16 and float32 hold the same values), every third utterance with the tone"""
    key = ("waves", shape, snip)
    if key not in _cache:
        o = ref.opts(snip_edges=snip, **cases.SHAPES[shape])
        lens = cases.batch_lengths(o)
        _cache[key] = [cases.noise(n, 100 + i, tone=(i % 3 == 0), samp_freq=o["samp_freq"]) for i, n in enumerate(lens)]
    return _cache[key]


def _o(shape, snip, **kw):
    return ref.opts(snip_edges=snip, **dict(cases.SHAPES[shape], **kw))


def _host(shape, snip, name, **kw):
    """host form of every utterance, computed once: name is the cache key of the option set kw"""
    import kaldi_hmm_gmm_amd as khg
    key = ("host", shape, snip, name)
    if key not in _cache:
        lo = cases.lib_opts(_o(shape, snip, **kw))
        fn = khg.compute_mfcc_feats if kw.get("kind", "mfcc") == "mfcc" else khg.compute_fbank_feats
        _cache[key] = [fn(w, lo) for w in _waves(shape, snip)]
    return _cache[key]


def _device(ctx, shape, snip, stype, waves=None, **kw):
    import kaldi_hmm_gmm_amd as khg
    lo = cases.lib_opts(_o(shape, snip, **kw))
    waves = _waves(shape, snip) if waves is None else waves
    if stype == "i16":
        waves = [w.astype(np.int16) for w in waves]
    fn = khg.compute_mfcc_feats_batch if kw.get("kind", "mfcc") == "mfcc" else khg.compute_fbank_feats_batch
    fo, t = fn(ctx, waves, lo)
    return fo, t.cpu().numpy()


def _rows(fo, x):
    return [x[fo[i]:fo[i + 1]] for i in range(len(fo) - 1)]


@pytest.mark.parametrize("stype", ["f32", "i16"])
@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_frame_off_and_mel_energies_on_the_bits(ctx, shape, snip, stype):
    import kaldi_hmm_gmm_amd as khg
    waves = _waves(shape, snip)
    assert 35 <= len(waves) <= 50
    lo = cases.lib_opts(_o(shape, snip))
    T = [khg.num_frames(lo, len(w)) for w in waves]
    F = khg.FE_TILE_FRAMES
    if snip:
        assert {0, 1, 2, F - 1, F, F + 1, 2 * F, 2 * F + 1, 300, 457, 700} <= set(T)
    assert T[0] == T[1] == T[2] == 0 and max(T) >= 700
    for power in (True, False):
        kw = dict(kind="fbank", use_log_fbank=False, use_power=power)
        fo, got = _device(ctx, shape, snip, stype, **kw)
        assert fo.dtype == np.int64 and fo.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
        want = np.concatenate(_host(shape, snip, "mel_p%d" % power, **kw))
        assert got.shape == want.shape == (sum(T), cases.SHAPES[shape]["num_mel_bins"]) and got.dtype == np.float32
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (power, int(bad.sum()), np.argwhere(bad)[:5].tolist())
        assert (got > 0).all()


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_log_mel_cepstra_and_energies(ctx, shape, snip):
    """log-mel within 2 float ulps of the host form (the mel energies are the same bits; the two logs round on their own); the
    cepstra within sum_b |dct_cb| lifter_c times 2 ulp(log-mel_b) plus the DCT chain's own (num_mel_bins + 1) 2^-24 sum_b |terms|;
    the log-energies within 2 ulps (their sums are the same bits)"""
    import kaldi_hmm_gmm_amd as khg
    B = cases.SHAPES[shape]["num_mel_bins"]
    kw = dict(kind="fbank", use_energy=True, raw_energy=False)
    _, got = _device(ctx, shape, snip, "f32", **kw)
    lm = np.concatenate(_host(shape, snip, "logmel_e", **kw))
    u = cases.ulps(got, lm)
    print("%s snip=%s: log-mel and windowed log-energy: largest difference %.3g ulp" % (shape, snip, float(u.max())))
    assert np.isfinite(got).all() and (u <= 2).all()
    floor_e = 9.0e6 * ref.dims(_o(shape, snip))[0]              # the raw energy of a noise-only frame (sigma 3000) is about this: the floor binds on some
    kw = dict(kind="mfcc", use_energy=True, raw_energy=True, energy_floor=floor_e)
    _, got = _device(ctx, shape, snip, "i16", **kw)
    want = np.concatenate(_host(shape, snip, "mfcc_e", **kw))
    tab = khg.frontend_tables(cases.lib_opts(_o(shape, snip, **kw)))
    dct, lif = np.abs(tab["dct"].astype(np.float64)), np.abs(tab["lifter"].astype(np.float64))
    lmv = lm[:, 1:].astype(np.float64)
    bound = ((2.0 * np.spacing(np.abs(lm[:, 1:])).astype(np.float64)) @ dct.T + (B + 1) * U24 * (np.abs(lmv) @ dct.T)) * lif[None, :]
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("%s snip=%s: cepstra: largest error / bound %.3g" % (shape, snip, float((err[:, 1:] / bound[:, 1:]).max())))
    assert (err[:, 1:] <= bound[:, 1:]).all()
    assert (cases.ulps(got[:, 0], want[:, 0]) <= 2).all()
    floor = np.float32(np.log(np.float64(np.float32(floor_e))))
    assert (got[:, 0] >= floor).all() and (got[:, 0] == floor).any() and (got[:, 0] > floor).any()      # the floor binds on some frames only


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_cepstra_with_c0_against_the_host_form(ctx, shape, snip):
    """MFCC without use_energy, so that column 0 is C0, the DCT's row 0: every cepstrum, from float32 and from int16 samples, within
    sum_b |dct_cb| lifter_c 2 ulp(log-mel_b) plus the DCT chain's (num_mel_bins + 1) 2^-24 sum_b |terms| of the host form"""
    import kaldi_hmm_gmm_amd as khg
    B = cases.SHAPES[shape]["num_mel_bins"]
    lm = np.concatenate(_host(shape, snip, "logmel", kind="fbank"))
    want = np.concatenate(_host(shape, snip, "mfcc", kind="mfcc"))
    tab = khg.frontend_tables(cases.lib_opts(_o(shape, snip)))
    dct, lif = np.abs(tab["dct"].astype(np.float64)), np.abs(tab["lifter"].astype(np.float64))
    bound = ((2.0 * np.spacing(np.abs(lm)).astype(np.float64)) @ dct.T + (B + 1) * U24 * (np.abs(lm.astype(np.float64)) @ dct.T)) * lif[None, :]
    assert (bound[:, 0] > 0).all()
    for stype in ("f32", "i16"):
        _, got = _device(ctx, shape, snip, stype, kind="mfcc")
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("%s snip=%s %s: cepstra with C0: largest error / bound %.3g (C0 alone %.3g)" %
              (shape, snip, stype, float((err / bound).max()), float((err[:, 0] / bound[:, 0]).max())))
        assert got.shape == want.shape and (err <= bound).all()


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_restatement_within_the_derived_bound(ctx, shape, snip):
    """device against tests/wave_ref.py (float64, an explicit DFT): log-mel and cepstra within the bound of DESIGN.md 7q"""
    waves = _waves(shape, snip)
    pick = [i for i, w in enumerate(waves) if len(w)][:12] + [len(waves) - 6]      # the short ones, the tile edges and the 300-frame one
    worst = {}
    for kind in ("fbank", "mfcc"):
        fo, got = _device(ctx, shape, snip, "f32", kind=kind)
        rows = _rows(fo, got)
        o = _o(shape, snip, kind=kind)
        worst[kind] = 0.0
        for i in pick:
            if len(rows[i]) == 0:
                continue
            want, det = ref.features(waves[i], o, detail=True)
            lmb = ref.log_mel_bound(o, det)
            bound = ref.cepstra_bound(o, lmb) if kind == "mfcc" else lmb
            ratio = np.abs(rows[i] - want) / bound
            worst[kind] = max(worst[kind], float(ratio.max()))
            assert rows[i].shape == want.shape and (ratio <= 1.0).all(), (kind, i)
    print("%s snip=%s: largest error / bound: log-mel %.3g, cepstra %.3g" % (shape, snip, worst["fbank"], worst["mfcc"]))


@pytest.mark.parametrize("snip", [True, False])
def test_bits_do_not_depend_on_the_batch(ctx, snip):
    """an utterance alone, inside the batch, with every neighbour's samples replaced by NaN, from run to run, from a device tensor
    and from a host array: the same bits"""
    import torch

    import kaldi_hmm_gmm_amd as khg
    shape = "16k23"
    waves = _waves(shape, snip)
    lo = cases.lib_opts(_o(shape, snip))
    fo, t = khg.compute_mfcc_feats_batch(ctx, waves, lo)
    base = t.cpu().numpy()
    fo2, t2 = khg.compute_mfcc_feats_batch(ctx, waves, lo)
    assert fo2.tolist() == fo.tolist() and t2.cpu().numpy().tobytes() == base.tobytes()
    rows = _rows(fo, base)
    picks = [i for i, r in enumerate(rows) if len(r)][:8] + [len(waves) - 6]      # around a frame, around the tile, and a 300-frame one
    for i in picks:
        fo1, t1 = khg.compute_mfcc_feats_batch(ctx, [waves[i]], lo)
        assert fo1.tolist() == [0, len(rows[i])] and t1.cpu().numpy().tobytes() == rows[i].tobytes(), i
        poisoned = [w if j == i else np.full(len(w), np.nan, np.float32) for j, w in enumerate(waves)]
        fo3, t3 = khg.compute_mfcc_feats_batch(ctx, poisoned, lo)
        got = t3.cpu().numpy()
        assert got[fo[i]:fo[i + 1]].tobytes() == rows[i].tobytes(), i
        others = np.concatenate([got[:fo[i]], got[fo[i + 1]:]])
        assert np.isnan(others).all()
    # the (sample_off, samples) forms: a host array, a device tensor, float32 and int16, and a caller's output tensor
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    flat = np.concatenate(waves)
    dev = "cuda:%d" % ctx.device
    for data in (flat, torch.from_numpy(flat).to(dev), flat.astype(np.int16), torch.from_numpy(flat.astype(np.int16)).to(dev)):
        out = torch.full(base.shape, float("nan"), dtype=torch.float32, device=dev)
        fo4, t4 = khg.compute_mfcc_feats_batch(ctx, (off, data), lo, out=out)
        assert t4 is out and fo4.tolist() == fo.tolist() and out.cpu().numpy().tobytes() == base.tobytes()


def test_all_zero_and_empty(ctx):
    import kaldi_hmm_gmm_amd as khg
    lo = khg.FrontendOptions(use_energy=1)
    fo, t = khg.compute_fbank_feats_batch(ctx, [np.zeros(5000, np.float32), np.zeros(0, np.float32), np.zeros(3000, np.int16)], lo)
    got = t.cpu().numpy()
    floor = np.float32(np.log(np.float64(np.finfo(np.float32).eps)))
    assert fo.tolist() == [0, 29, 29, 46] and got.shape == (46, 24) and np.isfinite(got).all() and (cases.ulps(got, floor) <= 2).all()
    fo, t = khg.compute_mfcc_feats_batch(ctx, [np.zeros(5000, np.float32)], None)
    assert np.isfinite(t.cpu().numpy()).all() and tuple(t.shape) == (29, 13)
    fo, t = khg.compute_mfcc_feats_batch(ctx, [np.zeros(10, np.float32), np.zeros(0, np.float32)], None)
    assert fo.tolist() == [0, 0, 0] and tuple(t.shape) == (0, 13)
    fo, t = khg.compute_mfcc_feats_batch(ctx, [], None)
    assert fo.tolist() == [0] and tuple(t.shape) == (0, 13)


def test_refusals_come_before_any_launch(ctx):
    import torch

    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    dev = "cuda:%d" % ctx.device
    x = cases.noise(4000, 1)
    out = torch.full((23, 13), 7.0, dtype=torch.float32, device=dev)
    for kw, word in ((dict(dither=1.0), "dither"), (dict(round_to_power_of_two=0), "round_to_power_of_two"), (dict(vtln_warp=0.9), "vtln_warp"),
                     (dict(htk_compat=1), "htk_compat"), (dict(frame_length_ms=5.0), "padded window"), (dict(frame_length_ms=70.0), "padded window"),
                     (dict(num_mel_bins=2), "num_mel_bins"), (dict(num_mel_bins=200), "num_mel_bins"), (dict(num_ceps=24), "num_ceps"),
                     (dict(frame_shift_ms=120.0), "LDS")):
        with pytest.raises(Exception, match=word):
            khg.compute_mfcc_feats_batch(ctx, [x], khg.FrontendOptions(**kw), out=out)
        with pytest.raises(Exception, match=word):
            khg.DeviceFrontend(ctx, khg.FrontendOptions(**kw))
    fe = khg.DeviceFrontend(ctx, khg.FrontendOptions())
    off = np.array([0, 4000], np.int64)
    fo = np.full(2, -5, np.int64)
    up = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()
    p = lambda a, t: _lib.ptr(a, t)      # noqa: E731
    calls = {
        "no samples": (1, off, None, None, khg.WAVE_F32),
        "both samples": (1, off, x.ctypes.data, up.data_ptr(), khg.WAVE_F32),
        "sample type": (1, off, x.ctypes.data, None, 5),
        "descending": (2, np.array([0, 4000, 100], np.int64), x.ctypes.data, None, khg.WAVE_F32),
        "negative": (1, np.array([-1, 4000], np.int64), x.ctypes.data, None, khg.WAVE_F32),
    }
    for name, (n_utt, so, sh, sd, st) in calls.items():
        rc = _lib.lib.khg_frontend_compute(ctx.h, fe.h, n_utt, p(so, _lib.C.c_int64), sh, sd, st, p(np.full(3, -5, np.int64), _lib.C.c_int64), out.data_ptr())
        assert rc == -1, name                                   # KHG_E_ARG
    assert _lib.lib.khg_frontend_compute(ctx.h, fe.h, 1, p(off, _lib.C.c_int64), x.ctypes.data, None, khg.WAVE_F32, None, out.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # and the same arguments put right fill it
    assert _lib.lib.khg_frontend_compute(ctx.h, fe.h, 1, p(off, _lib.C.c_int64), x.ctypes.data, None, khg.WAVE_F32, p(fo, _lib.C.c_int64), out.data_ptr()) == 0
    assert fo.tolist() == [0, 23] and np.abs(out.cpu().numpy() - khg.compute_mfcc_feats(x, None)).max() < 1e-3
    fe.close()
    with pytest.raises(Exception):
        khg.compute_mfcc_feats_batch(ctx, [x], None, out=torch.zeros((5, 13), dtype=torch.float32, device=dev))


def test_the_output_feeds_a_set_and_cmvn(ctx):
    """wave -> mfcc -> UtteranceSet(dim=13) -> acc_cmvn_stats: equal to compute_cmvn_stats of the downloaded rows within 7p's bound
    (each an n-term fp64 sum of exact terms in its own order: n 2^-52 sum |terms| apiece)"""
    import kaldi_hmm_gmm_amd as khg
    waves = _waves("16k23", True)
    fo, t = khg.compute_mfcc_feats_batch(ctx, waves, None)
    us = khg.UtteranceSet(ctx, None, fo, (t.data_ptr(), t), dim=13)
    assert us.n_utt == len(waves) and us.dim == 13
    stats = khg.compute_cmvn_stats_batch(us)
    got = stats.download()
    rows = _rows(fo, t.cpu().numpy())
    for i, r in enumerate(rows):
        want = khg.compute_cmvn_stats(r)
        x = np.abs(r.astype(np.float64))
        bound = np.zeros((2, 14))
        bound[0, :13], bound[1, :13] = 2 * len(r) * 2.0 ** -52 * x.sum(0), 2 * len(r) * 2.0 ** -52 * (x * x).sum(0)
        assert (np.abs(got[i] - want) <= bound).all(), i
    norm = khg.cmvn_compute(stats)
    d = khg.add_deltas_batch(us, 2, 2, norm=norm["norm"], status=norm["status"])
    i = len(waves) - 6                                          # the 300-frame utterance
    assert len(rows[i]) == 300
    assert d.cpu().numpy()[fo[i]:fo[i + 1]].tobytes() == khg.add_deltas(rows[i], 2, 2, norm=norm["norm"][i]).tobytes()
    stats.close()
    us.close()


def test_a_resident_handle_serves_the_batch_calls(ctx):
    """a DeviceFrontend in place of the options: the same bits, nothing rebuilt; one made for the other kind, or on another context, is
    refused before a launch, as is a sample_off that runs past the samples"""
    import torch

    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    dev = "cuda:%d" % ctx.device
    waves = _waves("16k23", True)[:14]
    lo = khg.FrontendOptions()
    fo, t = khg.compute_mfcc_feats_batch(ctx, waves, lo)
    assert fo.tolist() == khg.frame_offsets(lo, np.concatenate([[0], np.cumsum([len(w) for w in waves])])).tolist()
    fe = khg.DeviceFrontend(ctx, lo)
    for _ in range(2):
        fo2, t2 = khg.compute_mfcc_feats_batch(ctx, waves, fe)
        assert fo2.tolist() == fo.tolist() and bool((t2 == t).all())
    out = torch.full(tuple(t.shape), 7.0, dtype=torch.float32, device=dev)
    with pytest.raises(Exception, match="other kind"):
        khg.compute_fbank_feats_batch(ctx, waves, fe, out=out)
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    flat = np.concatenate(waves)
    for data in (flat[:-1], torch.from_numpy(flat[:-1].copy()).to(dev)):
        with pytest.raises(ValueError, match="sample_off ends"):
            khg.compute_mfcc_feats_batch(ctx, (off, data), fe, out=out)
    other = khg.Context(ctx.device)                             # another context's handle
    fe_other = khg.DeviceFrontend(other, lo)
    with pytest.raises(ValueError, match="another context"):
        khg.compute_mfcc_feats_batch(ctx, waves, fe_other, out=out)
    fo_h = np.full(len(off), -5, np.int64)
    rc = _lib.lib.khg_frontend_compute(ctx.h, fe_other.h, len(waves), _lib.ptr(off, _lib.C.c_int64), flat.ctypes.data, None, khg.WAVE_F32,
                                       _lib.ptr(fo_h, _lib.C.c_int64), out.data_ptr())
    assert rc == -1 and (fo_h == -5).all()                      # KHG_E_ARG, nothing written
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    fe_other.close()
    other.close()
    fe.close()
