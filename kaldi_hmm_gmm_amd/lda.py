"""LDA on spliced features on the batched device path: Kaldi's splice-feats, acc-lda, est-lda and transform-feats.

    stats = accumulate from posteriors resident on the device; the class is the pdf of the transition-id   (UtteranceSet.acc_lda_stats_post)
    M     = LdaEstimate::Estimate, fp64, on the host                                                       (lda_compute)
    feats = M z with z the frame spliced with its neighbours, out of place                                 (UtteranceSet.splice_transform_feats)

The spliced frame is z_t[k dim + j] = x[clamp(t + k - left, 0, T - 1)][j], k = 0 .. left + right; it is never written to device memory.
The transform is a float32 [target_dim, dim_z] matrix, [target_dim, dim_z + 1] with an offset column; transforms are numpy arrays
(numpy.save keeps them), as in fmllr.py."""
from typing import Iterable, Optional

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext
from .align import DevicePosteriors
from .device import DeviceLdaStats, LDA_MAX_SPLICED_DIM, LDA_OK, LDA_SINGULAR  # noqa: F401
from .fmllr import _fmaf, weight_silence_post

lda_compute = _ext.lda_compute


def acc_lda_batch(tm, utts, post, left: int = 4, right: int = 4, stats: Optional[DeviceLdaStats] = None, scale: float = 1.0,
                  silence_tids: Optional[Iterable[int]] = None, silence_weight: float = 0.0) -> DeviceLdaStats:
    """acc-lda for a set: the statistics of `post` (a DevicePosteriors, or the Kaldi Posteriors / the four arrays of
    posterior.posts_to_arrays, which are uploaded) on the set's resident features spliced with `left` / `right` frames of context.
    `tm`: the DeviceTransitions whose pdfs are the classes.  With `silence_tids` the posteriors are silence-weighted first
    (weight-silence-post; a DevicePosteriors is brought down, weighted and uploaded again).  `stats`: a DeviceLdaStats to add into;
    otherwise a fresh one of max(id2pdf) + 1 classes.  -> the statistics."""
    own_post = None
    if isinstance(post, DevicePosteriors):
        if silence_tids is not None:
            arrays = weight_silence_post(np.asarray(post.frame_off, np.int64), *post.download_arrays(), silence_tids, silence_weight)
            post = own_post = DevicePosteriors.from_arrays(utts.ctx, *arrays)
    else:
        from .posterior import posts_to_arrays
        arrays = post if isinstance(post, tuple) and len(post) == 4 else posts_to_arrays(post)
        if silence_tids is not None:
            arrays = weight_silence_post(*arrays, silence_tids, silence_weight)
        post = own_post = DevicePosteriors.from_arrays(utts.ctx, *arrays)
    try:
        if stats is None:
            stats = DeviceLdaStats(utts.ctx, int(np.max(np.asarray(tm.id2pdf)[1:])) + 1, utts.dim, left, right)
        utts.acc_lda_stats_post(tm, post, stats, scale)
    finally:
        if own_post is not None:
            own_post.close()
    return stats


def acc_lda(tm, utts, post, **kw) -> dict:
    """acc-lda with the statistics brought to the host: -> {"zero_acc", "first_acc", "total_second_acc" (float64, Kaldi's layout), "stats"}."""
    stats = acc_lda_batch(tm, utts, post, **kw)
    out = stats.download()
    out["stats"] = stats
    return out


def est_lda(stats, target_dim: int = 40, remove_offset: bool = False, within_class_factor: float = 1.0) -> dict:
    """est-lda: the transform from a DeviceLdaStats (or the dict of its download()).  -> {"M" float32 [target_dim, dim_z (+ 1 with
    remove_offset)], "M64", "M_full" float64 [dim_z, dim_z], "eig" (descending), "count", "status" (LDA_*)}."""
    s = stats if isinstance(stats, dict) else stats.download()
    return lda_compute(np.ascontiguousarray(s["zero_acc"], np.float64), np.ascontiguousarray(s["first_acc"], np.float64),
                       np.ascontiguousarray(s["total_second_acc"], np.float64), target_dim=target_dim, remove_offset=remove_offset,
                       within_class_factor=within_class_factor)


def splice_feats(feats: np.ndarray, left: int = 4, right: int = 4) -> np.ndarray:
    """splice-feats of one utterance on the host: [T, dim] -> [T, dim (left + right + 1)], edge frames replicated."""
    x = np.ascontiguousarray(feats, np.float32)
    T = x.shape[0]
    if T == 0:
        return np.zeros((0, x.shape[1] * (left + right + 1)), np.float32)
    idx = np.clip(np.arange(T)[:, None] + np.arange(-left, right + 1)[None, :], 0, T - 1)
    return np.ascontiguousarray(x[idx].reshape(T, -1))


def splice_transform_feats(feats: np.ndarray, M: Optional[np.ndarray], left: int = 4, right: int = 4) -> np.ndarray:
    """splice-feats | transform-feats of one utterance on the host, float32 in the device kernel's order: y = the offset column (0
    without one), then y = fl(M[:, c] z[c] + y) with one rounding per step (a fused multiply-add), c ascending.  M None: the spliced rows."""
    z = splice_feats(feats, left, right)
    if M is None:
        return z
    M = np.asarray(M, np.float32)
    Dz = z.shape[1]
    if M.ndim != 2 or M.shape[1] not in (Dz, Dz + 1):
        raise ValueError("splice_transform_feats: M must be [out_dim, %d] or one column more, got %s" % (Dz, M.shape,))
    y = (np.broadcast_to(M[:, Dz], (z.shape[0], M.shape[0])) if M.shape[1] == Dz + 1 else np.zeros((z.shape[0], M.shape[0]))).astype(np.float64)
    for c in range(Dz):
        y = _fmaf(M[:, c].astype(np.float64)[None, :], z[:, c].astype(np.float64)[:, None], y).astype(np.float64)
    return y.astype(np.float32)


def splice_transform_feats_batch(utts, M: Optional[np.ndarray], left: int = 4, right: int = 4, out=None):
    """splice-feats | transform-feats on the set's resident rows, out of place (the set is untouched).  M: float32 [out_dim, dim_z] or
    [out_dim, dim_z + 1], or None for the spliced rows (out_dim = dim_z).  out: a torch float32 device tensor [rows, out_dim] to
    fill; otherwise one is allocated.  -> the tensor, ready for UtteranceSet(ctx, tm, frame_off, (t.data_ptr(), t), dim=out_dim, graphs=...)."""
    import torch
    Dz = utts.dim * (left + right + 1)
    if M is not None:
        M = np.ascontiguousarray(M, np.float32)
        if M.ndim != 2 or M.shape[1] not in (Dz, Dz + 1):
            raise ValueError("splice_transform_feats_batch: M must be [out_dim, %d] or one column more, got %s" % (Dz, M.shape,))
    out_dim = Dz if M is None else M.shape[0]
    rows = int(np.asarray(utts.frame_off)[-1])
    if out is None:
        out = torch.empty((rows, out_dim), dtype=torch.float32, device="cuda:%d" % utts.ctx.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (rows, out_dim) or not out.is_cuda:
        raise ValueError("splice_transform_feats_batch: out must be a contiguous float32 device tensor [%d, %d]" % (rows, out_dim))
    torch.cuda.current_stream(out.device).synchronize()       # the tensor's memory may still be in use by work queued on torch's stream
    utts.splice_transform_feats(left, right, M, out.data_ptr())
    return out


def compose_with_lda(M_after: np.ndarray, lda_M: np.ndarray, lda_has_offset: bool = False) -> np.ndarray:
    """compose-transforms for a square [d, d] or affine [d, d + 1] transform applied AFTER the rectangular LDA matrix [d, dim_z] (or
    [d, dim_z + 1] with lda_has_offset): est_mllt on the projected features then yields one final.mat.  float64 arithmetic, float32
    result: [d, dim_z], or [d, dim_z + 1] when either transform has an offset."""
    a, b = np.asarray(M_after, np.float64), np.asarray(lda_M, np.float64)
    d = b.shape[0]
    if a.ndim != 2 or a.shape[0] != d or a.shape[1] not in (d, d + 1):
        raise ValueError("compose_with_lda: M_after must be [%d, %d] or one column more, got %s" % (d, d, a.shape,))
    Dz = b.shape[1] - (1 if lda_has_offset else 0)
    A = a[:, :d] @ b[:, :Dz]
    if a.shape[1] == d and not lda_has_offset:
        return A.astype(np.float32)
    off = (a[:, :d] @ b[:, Dz] if lda_has_offset else np.zeros(d)) + (a[:, d] if a.shape[1] == d + 1 else 0.0)
    return np.concatenate([A, off[:, None]], 1).astype(np.float32)
