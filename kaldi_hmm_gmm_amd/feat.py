"""The feature stage in front of the acoustic model on the batched device path: Kaldi's compute-cmvn-stats, apply-cmvn
and add-deltas.

    stats = per speaker sum x, sum x x and the frame count, fp64, from the set's resident rows   (UtteranceSet.acc_cmvn_stats)
    norm  = ApplyCmvn's offset and scale per speaker and dimension, fp64 on the host             (cmvn_compute)
    feats = fl(fl(x scale) + offset), in place or out of place                                   (UtteranceSet.apply_cmvn)
    feats = [v | delta v | delta-delta v ..] with v = x or its CMVN value, out of place          (UtteranceSet.add_deltas)

Statistics are float64 [n_spk, 2, dim + 1] in Kaldi's layout (row 0: sums and, last, the count; row 1: sums of squares and 0);
normalisers are float32 [n_spk, 2, dim] (row 0 the offset, row 1 the scale) with an int32 status per speaker.  Both are numpy arrays
(numpy.save keeps them), as in fmllr.py.  utt2spk: one speaker number per utterance, < 0 for none; per-utterance CMVN is
numpy.arange(n_utt)."""
from typing import List, Optional

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext
from .device import DeviceCmvnStats
from .fmllr import _fmaf

CMVN_OK = _ext.CMVN_OK
CMVN_NO_DATA = _ext.CMVN_NO_DATA
CMVN_NONFINITE = _ext.CMVN_NONFINITE
FEAT_TILE_LDS_BYTES = _ext.FEAT_TILE_LDS_BYTES
delta_scales = _ext.delta_scales


def compute_cmvn_stats(feats: np.ndarray) -> np.ndarray:
    """compute-cmvn-stats of one utterance on the host: float64 [2, dim + 1], the sums in numpy's order (the device's order is its
    own; the two agree to the rounding of an fp64 sum)."""
    x = np.ascontiguousarray(feats, np.float32).astype(np.float64)
    st = np.zeros((2, x.shape[1] + 1))
    st[0, :-1], st[0, -1], st[1, :-1] = x.sum(0), x.shape[0], (x * x).sum(0)
    return st


def compute_cmvn_stats_batch(utts, utt2spk=None, n_spk: Optional[int] = None, stats: Optional[DeviceCmvnStats] = None) -> DeviceCmvnStats:
    """compute-cmvn-stats for a set: the statistics of its resident rows per speaker.  utt2spk None: per utterance.  `stats`: a
    DeviceCmvnStats to add into (statistics of several sets); otherwise a fresh one of n_spk (default max(utt2spk) + 1) speakers.
    -> the statistics (download() brings them to the host)."""
    ids = np.arange(utts.n_utt, dtype=np.int32) if utt2spk is None else np.ascontiguousarray(utt2spk, np.int32)
    if stats is None:
        if n_spk is None:
            n_spk = int(ids.max()) + 1 if len(ids) else 0
        if n_spk < 1:
            raise ValueError("compute_cmvn_stats: no speaker")
        stats = DeviceCmvnStats(utts.ctx, n_spk, utts.dim)
    utts.acc_cmvn_stats(ids, stats)
    return stats


def cmvn_compute(stats, norm_means: bool = True, norm_vars: bool = False, reverse: bool = False) -> dict:
    """ApplyCmvn's normaliser from statistics (a DeviceCmvnStats, or float64 [n_spk, 2, dim + 1] / [2, dim + 1] for one speaker).
    -> {"norm" float32 [n_spk, 2, dim]: offset, scale; "status" int32 [n_spk]: CMVN_*}.  A speaker that is not CMVN_OK gets offset 0
    and scale 1, and apply_cmvn / add_deltas given the statuses leave its utterances as they are."""
    s = stats.download() if isinstance(stats, DeviceCmvnStats) else np.asarray(stats, np.float64)
    one = s.ndim == 2
    r = _ext.cmvn_compute(np.ascontiguousarray(s[None] if one else s), norm_means=norm_means, norm_vars=norm_vars, reverse=reverse)
    return {"norm": r["norm"][0], "status": int(r["status"][0])} if one else r


def apply_cmvn(feats: np.ndarray, norm: Optional[np.ndarray]) -> np.ndarray:
    """apply-cmvn of one utterance on the host in the device kernel's arithmetic: y = fl(fl(x scale) + offset) in float32, two
    roundings.  norm: float32 [2, dim] (offset, scale), or None for a copy."""
    x = np.ascontiguousarray(feats, np.float32)
    if norm is None:
        return x.copy()
    n = np.asarray(norm, np.float32)
    if n.shape != (2, x.shape[1]):
        raise ValueError("apply_cmvn: norm must be [2, %d], got %s" % (x.shape[1], n.shape,))
    with np.errstate(all="ignore"):
        return ((x * n[1][None, :]).astype(np.float32) + n[0][None, :]).astype(np.float32)


def _norm_args(utts, norm, utt2spk, status):
    norm = np.ascontiguousarray(norm, np.float32)
    if norm.ndim == 2:
        norm = norm[None]
    ids = np.arange(utts.n_utt, dtype=np.int32) if utt2spk is None else np.ascontiguousarray(utt2spk, np.int32)
    st = None if status is None else np.ascontiguousarray(np.atleast_1d(status), np.int32)
    return norm, ids, st


def _out_tensor(who, utts, out_dim, out):
    import torch
    rows = int(np.asarray(utts.frame_off)[-1])
    if out is None:
        out = torch.empty((rows, out_dim), dtype=torch.float32, device="cuda:%d" % utts.ctx.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (rows, out_dim) or not out.is_cuda:
        raise ValueError("%s: out must be a contiguous float32 device tensor [%d, %d]" % (who, rows, out_dim))
    torch.cuda.current_stream(out.device).synchronize()       # the tensor's memory may still be in use by work queued on torch's stream
    return out


def apply_cmvn_batch(utts, norm, utt2spk=None, status=None, out=None, in_place: bool = True):
    """apply-cmvn on the set's resident rows: utterance u through norm[utt2spk[u]] (kept as it is where utt2spk[u] < 0 or, with
    `status`, where the speaker is not CMVN_OK).  utt2spk None: per utterance.  By default the set's own rows are rewritten in place
    (the set then forgets what it derived from the old ones) and None is returned; with in_place=False (or a tensor `out`) the rows go
    to a torch float32 device tensor [rows, dim], which is returned, and the set is untouched."""
    norm, ids, st = _norm_args(utts, norm, utt2spk, status)
    if out is None and in_place:
        utts.apply_cmvn(ids, norm, st, None)
        return None
    out = _out_tensor("apply_cmvn_batch", utts, utts.dim, out)
    utts.apply_cmvn(ids, norm, st, out.data_ptr())
    return out


def add_deltas(feats: np.ndarray, order: int = 2, window: int = 2, norm: Optional[np.ndarray] = None) -> np.ndarray:
    """add-deltas of one utterance on the host, float32 in the device kernel's order: block i of frame t is y = 0, then
    y = fl(scales[i][j] v[clamp(t + j, 0, T - 1)] + y) with one rounding per step (a fused multiply-add) for j ascending, the zero
    coefficients skipped.  v = feats, or with `norm` ([2, dim]) its apply_cmvn.  -> [T, dim (order + 1)]."""
    v = apply_cmvn(feats, norm)
    T, D = v.shape
    out = np.zeros((T, D * (order + 1)), np.float32)
    if T == 0:
        return out
    v64 = v.astype(np.float64)
    scales: List[np.ndarray] = delta_scales(order, window)
    with np.errstate(all="ignore"):
        for i, s in enumerate(scales):
            H = i * window
            y = np.zeros((T, D), np.float64)
            for j in range(-H, H + 1):
                a = float(s[j + H])
                if a == 0.0:
                    continue
                rows = np.clip(np.arange(T) + j, 0, T - 1)
                y = _fmaf(np.full((T, D), a), v64[rows], y).astype(np.float64)
            out[:, i * D:(i + 1) * D] = y.astype(np.float32)
    return out


def add_deltas_batch(utts, order: int = 2, window: int = 2, norm=None, utt2spk=None, status=None, out=None):
    """add-deltas on the set's resident rows, out of place (the set is untouched), with apply-cmvn fused in when `norm` is given
    (float32 [n_spk, 2, dim]; utt2spk None: per utterance; `status`: the speakers' CMVN_* -- utterances of one that is not OK, like
    those with utt2spk < 0, go in as they are).  out: a torch float32 device tensor [rows, dim (order + 1)] to fill; otherwise one is
    allocated.  -> the tensor, ready for UtteranceSet(ctx, tm, frame_off, (t.data_ptr(), t), dim=dim (order + 1), graphs=...)."""
    if order < 0 or window < 1:
        raise ValueError("add_deltas_batch: order must be >= 0 and window >= 1")
    out = _out_tensor("add_deltas_batch", utts, utts.dim * (order + 1), out)
    if norm is None:
        utts.add_deltas(order, window, out.data_ptr())
    else:
        norm, ids, st = _norm_args(utts, norm, utt2spk, status)
        utts.add_deltas(order, window, out.data_ptr(), norm, ids, st)
    return out
