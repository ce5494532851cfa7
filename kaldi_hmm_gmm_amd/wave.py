"""MFCC and filterbank features from waveforms on the batched device path: Kaldi's compute-mfcc-feats and
compute-fbank-feats for a ragged batch.

    frames -> minus the mean -> (raw log-energy) -> pre-emphasis -> window -> real FFT of N -> power -> mel filters -> log -> (DCT, lifter)

Samples are on Kaldi's scale (+-32768), float32 or int16.  The host forms (compute_mfcc_feats, compute_fbank_feats) repeat the
device kernel's operations one by one in numpy float32 -- the same chains, the same butterfly schedule, every operation rounded on
its own --, so the mel energies agree with the device on the bits and the logs to the rounding of the log.  The tables (window, mel
filters, DCT rows, lifter, twiddles) come from the library's host code (frontend_tables); neither form computes a transcendental
function except the final log (and the root of the magnitude spectrum)."""
from typing import Optional

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext

FrontendOptions = _ext.FrontendOptions
DeviceFrontend = _ext.DeviceFrontend
num_frames = _ext.num_frames
frontend_tables = _ext.frontend_tables
frontend_dims = _ext.frontend_dims
FE_MFCC, FE_FBANK, FE_TILE_FRAMES = _ext.FE_MFCC, _ext.FE_FBANK, _ext.FE_TILE_FRAMES
WIN_POVEY, WIN_HAMMING, WIN_HANNING = _ext.WIN_POVEY, _ext.WIN_HAMMING, _ext.WIN_HANNING
WIN_RECTANGULAR, WIN_BLACKMAN = _ext.WIN_RECTANGULAR, _ext.WIN_BLACKMAN
WAVE_F32, WAVE_I16 = _ext.WAVE_F32, _ext.WAVE_I16

_EPS = np.float32(np.finfo(np.float32).eps)


def _of_kind(opts, kind):
    o = FrontendOptions() if opts is None else opts.copy()
    o.kind = kind
    return o


def frame_starts(opts, n_samples: int) -> np.ndarray:
    """the first sample of every frame of an utterance of n_samples (negative, or past the end, without snip_edges)"""
    d = frontend_dims(opts)
    T = num_frames(opts, n_samples)
    return np.arange(T, dtype=np.int64) * d["S"] + (0 if opts.snip_edges else d["S"] // 2 - d["L"] // 2)


def _lane_sum(v: np.ndarray) -> np.ndarray:
    """the kernel's sum over a frame: lane l adds v[l], v[l + 64], .. in turn; then lane l takes lane l ^ 32, ^ 16, .. ^ 1"""
    T, L = v.shape
    J = -(-L // 64)
    pad = np.zeros((T, J * 64), np.float32)
    pad[:, :L] = v
    acc = np.zeros((T, 64), np.float32)
    for j in range(J):
        acc = acc + pad[:, j * 64:(j + 1) * 64]
    h = 32
    while h >= 1:
        acc = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return acc[:, 0]


def _log_floor(e: np.ndarray) -> np.ndarray:
    return np.log(np.maximum(e, _EPS).astype(np.float64)).astype(np.float32)


def _features(wave, opts) -> np.ndarray:
    tab = frontend_tables(opts)
    d = frontend_dims(opts)
    L, N, B, C = d["L"], d["N"], d["num_mel_bins"], d["num_ceps"]
    M = N // 2
    logM = M.bit_length() - 1
    x = np.asarray(wave)
    if x.ndim != 1:
        raise ValueError("a waveform is a 1-d array of samples")
    x = np.ascontiguousarray(x, np.float32)
    n = len(x)
    starts = frame_starts(opts, n)
    T = len(starts)
    out = np.zeros((T, d["dim"]), np.float32)
    if T == 0:
        return out
    mfcc = opts.kind == FE_MFCC
    use_log = mfcc or bool(opts.use_log_fbank)
    use_power = mfcc or bool(opts.use_power)
    with np.errstate(all="ignore"):
        idx = (starts[:, None] + np.arange(L)[None, :]) % (2 * n)     # the reflection has period 2 n
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
        w = x[idx]                                                    # [T, L]
        if opts.remove_dc_offset:
            mean = _lane_sum(w) * np.float32(1.0 / L)
            w = w - mean[:, None]
        energy = None
        if opts.use_energy and opts.raw_energy:
            energy = _lane_sum(w * w)
        c = np.float32(opts.preemph_coeff)
        if c != 0:
            prev = np.concatenate([w[:, :1], w[:, :-1]], axis=1)
            w = w - c * prev
        w = w * tab["window"][None, :]
        if opts.use_energy and not opts.raw_energy:
            energy = _lane_sum(w * w)
        v = np.zeros((T, N), np.float32)
        v[:, :L] = w
        rev = np.array([int(format(j, "0%db" % logM)[::-1], 2) for j in range(M)])
        zr, zi = np.zeros((T, M), np.float32), np.zeros((T, M), np.float32)
        zr[:, rev], zi[:, rev] = v[:, 0::2], v[:, 1::2]
        twr, twi = tab["twiddles"][:, 0], tab["twiddles"][:, 1]
        q = np.arange(M // 2)
        for s in range(logM):
            half = 1 << s
            k = q & (half - 1)
            a = ((q >> s) << (s + 1)) + k
            b = a + half
            j = k << (logM - 1 - s)
            wr, wi = twr[2 * j][None, :], twi[2 * j][None, :]
            br, bi, ar, ai = zr[:, b], zi[:, b], zr[:, a], zi[:, a]
            tr = wr * br - wi * bi
            ti = wr * bi + wi * br
            zr[:, a], zi[:, a], zr[:, b], zi[:, b] = ar + tr, ai + ti, ar - tr, ai - ti
        P = np.zeros((T, M), np.float32)
        a0 = zr[:, 0] + zi[:, 0]
        P[:, 0] = a0 * a0
        k = np.arange(1, M)
        xr, xi, yr, yi = zr[:, k], zi[:, k], zr[:, M - k], zi[:, M - k]
        half_ = np.float32(0.5)
        er, ei, pr, pi = half_ * (xr + yr), half_ * (xi - yi), half_ * (xi + yi), half_ * (yr - xr)
        wr, wi = twr[k][None, :], twi[k][None, :]
        re = er + (wr * pr - wi * pi)
        im = ei + (wr * pi + wi * pr)
        P[:, 1:] = re * re + im * im
        if not use_power:
            P = np.sqrt(P.astype(np.float64)).astype(np.float32)
        mel = np.zeros((T, B), np.float32)
        at = 0
        for b in range(B):
            off, ln = int(tab["mel_off"][b]), int(tab["mel_len"][b])
            acc = np.zeros(T, np.float32)
            for kk in range(ln):
                acc = acc + tab["mel_w"][at + kk] * P[:, off + kk]
            at += ln
            mel[:, b] = acc
        if use_log:
            mel = _log_floor(mel)
        if energy is not None:
            energy = _log_floor(energy)
            if opts.energy_floor > 0:
                energy = np.maximum(energy, np.float32(np.log(float(np.float32(opts.energy_floor)))))
        if mfcc:
            acc = np.zeros((T, C), np.float32)
            for b in range(B):
                acc = acc + tab["dct"][:, b][None, :] * mel[:, b][:, None]
            out[:] = acc * tab["lifter"][None, :]
            if energy is not None:
                out[:, 0] = energy
        else:
            e0 = 1 if energy is not None else 0
            if e0:
                out[:, 0] = energy
            out[:, e0:] = mel
    assert out.dtype == np.float32
    return out


def compute_mfcc_feats(wave, opts: Optional[FrontendOptions] = None) -> np.ndarray:
    """compute-mfcc-feats of one utterance on the host, float32 in the device kernel's order -> [T, num_ceps]"""
    return _features(wave, _of_kind(opts, FE_MFCC))


def compute_fbank_feats(wave, opts: Optional[FrontendOptions] = None) -> np.ndarray:
    """compute-fbank-feats of one utterance on the host, float32 in the device kernel's order -> [T, num_mel_bins (+ 1 with use_energy)]"""
    return _features(wave, _of_kind(opts, FE_FBANK))


def frame_offsets(opts, sample_off) -> np.ndarray:
    """the rows' prefix sums for utterances at [sample_off[u], sample_off[u + 1]): num_frames of every one, without a device"""
    d = frontend_dims(opts)
    n = np.diff(np.asarray(sample_off, np.int64))
    if (n < 0).any():
        raise ValueError("sample_off must not descend")
    L, S = d["L"], d["S"]
    T = np.where(n < L, 0, 1 + (n - L) // S) if opts.snip_edges else (n + S // 2) // S
    return np.concatenate([[0], np.cumsum(T)]).astype(np.int64)


def _batch(who, ctx, waves, opts, kind, out):
    import torch
    own = not isinstance(opts, DeviceFrontend)
    if own:
        o = _of_kind(opts, kind)
    else:                                                             # the caller's resident tables: nothing is built or uploaded here
        o = opts.opts
        if o.kind != kind:
            raise ValueError("%s: the DeviceFrontend was made for the other kind of features" % who)
        if opts.ctx is not ctx:
            raise ValueError("%s: the DeviceFrontend belongs to another context" % who)
    samples_h, samples_d, keep = None, 0, None
    if isinstance(waves, tuple):
        sample_off, data = waves
        sample_off = np.ascontiguousarray(sample_off, np.int64)
        if sample_off.ndim != 1 or len(sample_off) < 1 or sample_off[0] < 0:
            raise ValueError("%s: sample_off must be [n_utt + 1], starting at or above 0" % who)
        if isinstance(data, torch.Tensor):
            if not data.is_cuda or not data.is_contiguous() or data.dim() != 1 or data.dtype not in (torch.float32, torch.int16):
                raise ValueError("%s: device samples must be a contiguous 1-d float32 or int16 tensor" % who)
            if data.device.index != ctx.device:
                raise ValueError("%s: the samples are on another device than the context" % who)
            stype = WAVE_I16 if data.dtype == torch.int16 else WAVE_F32
            torch.cuda.current_stream(data.device).synchronize()      # the samples may still be being written on torch's stream
            samples_d, keep, have = data.data_ptr(), data, data.numel()
        else:
            data = np.asarray(data)
            if data.ndim != 1:
                raise ValueError("%s: the samples must be one 1-d array" % who)
            stype = WAVE_I16 if data.dtype == np.int16 else WAVE_F32
            samples_h = np.ascontiguousarray(data, np.int16 if stype == WAVE_I16 else np.float32)
            have = len(samples_h)
        if int(sample_off[-1]) > have:
            raise ValueError("%s: sample_off ends at %d, the samples at %d" % (who, int(sample_off[-1]), have))
    else:
        arrs = [np.asarray(w) for w in waves]
        if any(a.ndim != 1 for a in arrs):
            raise ValueError("%s: a waveform is a 1-d array of samples" % who)
        stype = WAVE_I16 if arrs and all(a.dtype == np.int16 for a in arrs) else WAVE_F32
        dt = np.int16 if stype == WAVE_I16 else np.float32
        sample_off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
        samples_h = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros(0), dt)
    frame_off = frame_offsets(o, sample_off)                          # refuses what the options refuse, before anything is allocated
    fe = DeviceFrontend(ctx, o) if own else opts
    try:
        rows, dim = int(frame_off[-1]), fe.dim
        if out is None:
            out = torch.empty((rows, dim), dtype=torch.float32, device="cuda:%d" % ctx.device)
        elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (rows, dim) or not out.is_cuda:
            raise ValueError("%s: out must be a contiguous float32 device tensor [%d, %d]" % (who, rows, dim))
        torch.cuda.current_stream(out.device).synchronize()           # the tensor's memory may still be in use by work queued on torch's stream
        if rows:
            got = fe.compute(sample_off, samples_h, samples_d, stype, out.data_ptr())
            assert (got == frame_off).all()
    finally:
        if own:
            fe.close()
    del keep
    return frame_off, out


def compute_mfcc_feats_batch(ctx, waves, opts: Optional[FrontendOptions] = None, out=None):
    """compute-mfcc-feats for a ragged batch on the device.  opts: FrontendOptions (the tables are built and uploaded for this call)
    or a DeviceFrontend made for MFCC on `ctx` (its resident tables are used: the way to call this again and again).  waves: a list of 1-d arrays (int16 if all are, else float32), or
    (sample_off, samples) with samples one 1-d numpy array or torch device tensor (float32 or int16) holding utterance u at
    [sample_off[u], sample_off[u + 1]).  -> (frame_off int64 [n_utt + 1], torch float32 device tensor [rows, num_ceps]), ready for
    UtteranceSet(ctx, tm, frame_off, (t.data_ptr(), t), dim=num_ceps, graphs=...).  Synchronous."""
    return _batch("compute_mfcc_feats_batch", ctx, waves, opts, FE_MFCC, out)


def compute_fbank_feats_batch(ctx, waves, opts: Optional[FrontendOptions] = None, out=None):
    """compute-fbank-feats for a ragged batch on the device; arguments and result as compute_mfcc_feats_batch, the tensor
    [rows, num_mel_bins (+ 1 with use_energy)]."""
    return _batch("compute_fbank_feats_batch", ctx, waves, opts, FE_FBANK, out)
