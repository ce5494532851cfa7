"""MLLT / semi-tied covariance on the batched device path: Kaldi's gmm-acc-mllt, est-mllt and gmm-transform-means.

    stats = accumulate from posteriors resident on the device, over all the data   (UtteranceSet.acc_mllt_stats_post)
    M     = the row-by-row update of MlltAccs::Update, fp64, on the host           (mllt_compute)
    feats = M x  (transform_feats_batch with one speaker and W = [M | 0]);  means = M mu  (DeviceModel.transform_means)

The transform is a float32 [dim, dim] matrix.  Where a feature transform is asked for it is returned as fmllr.py's [dim, dim + 1] with
a zero offset column, so that it composes with earlier transforms (compose_transforms) and applies with transform_feats_batch."""
from typing import Optional

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext
from .align import DevicePosteriors
from .device import DeviceMlltStats
from .fmllr import compose_transforms

MLLT_OK = _ext.MLLT_OK
MLLT_SINGULAR = _ext.MLLT_SINGULAR
MLLT_MAX_DIM = _ext.MLLT_MAX_DIM
mllt_compute = _ext.mllt_compute


def gmm_acc_mllt_batch(model, tm, utts, post, stats: Optional[DeviceMlltStats] = None, scale: float = 1.0) -> DeviceMlltStats:
    """gmm-acc-mllt for a set: the statistics of `post` (a DevicePosteriors, or the Kaldi Posteriors / the four arrays of
    posterior.posts_to_arrays, which are uploaded) on the set's resident features under `model`, every frame counted (no random
    pruning).  `stats`: a DeviceMlltStats to add into (several sets under ONE model); otherwise a fresh one.  -> the statistics."""
    own_post = None
    if not isinstance(post, DevicePosteriors):
        from .posterior import posts_to_arrays
        arrays = post if isinstance(post, tuple) and len(post) == 4 else posts_to_arrays(post)
        post = own_post = DevicePosteriors.from_arrays(utts.ctx, *arrays)
    if stats is None:
        stats = DeviceMlltStats(utts.ctx, utts.dim)
    try:
        utts.acc_mllt_stats_post(model, tm, post, stats, scale)
    finally:
        if own_post is not None:
            own_post.close()
    return stats


def gmm_acc_mllt(model, tm, utts, post, **kw) -> dict:
    """gmm-acc-mllt with the statistics brought to the host: -> {"beta", "G" float64 [dim, dim (dim + 1) / 2], "stats"}."""
    stats = gmm_acc_mllt_batch(model, tm, utts, post, **kw)
    out = stats.download()
    out["stats"] = stats
    return out


def est_mllt(stats, num_iters: int = 200, prev: Optional[np.ndarray] = None) -> dict:
    """est-mllt: the transform from a DeviceMlltStats (or the dict of its download()).  -> {"M" float32 [dim, dim], "M64", "W" float32
    [dim, dim + 1] = [M | 0] for transform_feats_batch, "objf_impr", "count", "status" (MLLT_*)}.  With `prev` (an earlier feature
    transform, [dim, dim] or [dim, dim + 1]) "W" is the composition that applies `prev` first and M second."""
    s = stats if isinstance(stats, dict) else stats.download()
    out = mllt_compute(float(s["beta"]), np.ascontiguousarray(s["G"], np.float64), num_iters=num_iters)
    D = out["M"].shape[0]
    W = np.concatenate([out["M"], np.zeros((D, 1), np.float32)], 1)
    if prev is not None:
        prev = np.asarray(prev, np.float32)
        if prev.shape == (D, D):
            prev = np.concatenate([prev, np.zeros((D, 1), np.float32)], 1)
        W = compose_transforms(W, prev)
    out["W"] = W
    return out


def gmm_transform_means(M: np.ndarray, model=None, am_gmm=None) -> None:
    """gmm-transform-means: every mean of `model` (a DeviceModel, rewritten in place and ready for the next pass) and / or `am_gmm` (a
    host AmDiagGmm or DiagGmm) through M [dim, dim]; gconsts are recomputed, weights and variances stay.  The two forms give the same
    bits for weights, inv_vars and means_invvars.  M must be square: an affine [dim, dim + 1] transform (est_mllt's W) is refused
    rather than its offset column dropped -- pass est_mllt's M."""
    M = np.ascontiguousarray(M, np.float32)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("gmm_transform_means: M must be [dim, dim], got %s" % (M.shape,))
    if model is not None:
        model.transform_means(M)
    if am_gmm is not None:
        am_gmm.transform_means(M)
