"""fMLLR speaker adaptation on the batched device path: Kaldi's gmm-est-fmllr and transform-feats.

    stats = accumulate per speaker from posteriors resident on the device   (UtteranceSet.acc_fmllr_stats_post)
    W     = the row-by-row update of ComputeFmllrMatrixDiagGmmFull, fp64    (DeviceFmllrStats.estimate; fmllr_compute on the host)
    feats = A x + b per utterance with its speaker's W                      (UtteranceSet.transform_feats)

A transform is a float32 [dim, dim + 1] matrix W = [A | b]; a batch of them [n_spk, dim, dim + 1].  Speakers are numbered 0 .. n_spk - 1
and `utt2spk` is one number per utterance of the set, -1 for an utterance that belongs to nobody (it adds no statistics and its rows
are copied).  kaldi_io.py has no matrix form, so transforms are not read or written as Kaldi files here: they are numpy arrays
(numpy.save keeps them)."""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext
from .align import DevicePosteriors
from .device import DeviceFmllrStats

FMLLR_OK = _ext.FMLLR_OK
FMLLR_LOW_COUNT = _ext.FMLLR_LOW_COUNT
FMLLR_SINGULAR = _ext.FMLLR_SINGULAR
FMLLR_MAX_DIM = _ext.FMLLR_MAX_DIM
fmllr_compute = _ext.fmllr_compute


def utt2spk_ids(utts: Sequence[str], utt2spk: Dict[str, str]) -> Tuple[np.ndarray, List[str]]:
    """Kaldi's utt2spk map for the utterances of a set, in set order -> (int32 speaker number per utterance, speaker names by number).
    Speakers are numbered in order of first appearance; an utterance the map lacks gets -1."""
    names: List[str] = []
    index: Dict[str, int] = {}
    ids = np.full(len(utts), -1, np.int32)
    for i, u in enumerate(utts):
        s = utt2spk.get(u)
        if s is None:
            continue
        if s not in index:
            index[s] = len(names)
            names.append(s)
        ids[i] = index[s]
    return ids, names


def spk2utt(utt2spk: Iterable[int], n_spk: Optional[int] = None) -> List[List[int]]:
    """The inverse of a numbered utt2spk: per speaker the utterances of the set that belong to it, in set order."""
    ids = np.asarray(list(utt2spk), np.int64)
    n = int(ids.max()) + 1 if n_spk is None and len(ids) else int(n_spk or 0)
    out: List[List[int]] = [[] for _ in range(n)]
    for u, s in enumerate(ids):
        if s >= 0:
            out[int(s)].append(u)
    return out


def weight_silence_post(frame_off, entry_begin, tid, weight, silence_tids: Iterable[int], silence_weight: float):
    """weight-silence-post on the flat arrays of posterior.posts_to_arrays: the weight of every entry whose transition-id is in
    `silence_tids` is multiplied by `silence_weight`.  -> the four arrays (weight is a new array)."""
    sil = np.zeros(int(np.max(tid)) + 2 if len(tid) else 1, bool)
    for t in silence_tids:
        if 0 <= int(t) < len(sil):
            sil[int(t)] = True
    w = np.array(weight, np.float64, copy=True)
    w[sil[np.asarray(tid, np.int64)]] *= float(silence_weight)
    return frame_off, entry_begin, tid, w


def gmm_est_fmllr_batch(model, tm, utts, post, utt2spk, n_spk: Optional[int] = None, scale: float = 1.0, min_count: float = 500.0,
                        num_iters: int = 40, stats: Optional[DeviceFmllrStats] = None,
                        silence_tids: Optional[Iterable[int]] = None, silence_weight: float = 0.0, device: bool = True,
                        W_d: Optional[int] = None) -> dict:
    """gmm-est-fmllr for every speaker of a set: the statistics of `post` (a DevicePosteriors, or the Kaldi Posteriors / the four
    arrays of posterior.posts_to_arrays, which are uploaded) on the set's resident features under `model`, then the estimate.
    With `silence_tids`, host posteriors are silence-weighted first (weight-silence-post).  `stats`: a DeviceFmllrStats to add into
    (statistics of several sets); otherwise a fresh one.  The estimate runs on the device where the statistics are (`device`, the
    default; W_d: a device pointer that also receives the transforms and keeps them resident) or, with device=False, on the host on
    the downloaded statistics (then "W64" holds W before narrowing).  -> {"W" float32 [n_spk, dim, dim + 1], "objf_impr", "count",
    "status" (FMLLR_*), "stats"}."""
    ids = np.ascontiguousarray(utt2spk, np.int32)
    if n_spk is None:
        n_spk = int(ids.max()) + 1 if len(ids) else 0
    if n_spk < 1:
        raise ValueError("gmm_est_fmllr: no speaker")
    ctx = utts.ctx
    own_post = None
    if not isinstance(post, DevicePosteriors):
        from .posterior import posts_to_arrays
        arrays = post if isinstance(post, tuple) and len(post) == 4 else posts_to_arrays(post)
        if silence_tids is not None:
            arrays = weight_silence_post(*arrays, silence_tids, silence_weight)
        post = own_post = DevicePosteriors.from_arrays(ctx, *arrays)
    elif silence_tids is not None:
        raise ValueError("gmm_est_fmllr: silence weighting applies to host posteriors; weight a DevicePosteriors before the upload")
    if stats is None:
        stats = DeviceFmllrStats(ctx, n_spk, utts.dim)
    try:
        utts.acc_fmllr_stats_post(model, tm, post, ids, stats, scale)
        if device:
            out = stats.estimate(min_count=min_count, num_iters=num_iters, W_d=W_d)
        else:
            s = stats.download()
            out = fmllr_compute(s["beta"], s["K"], s["G"], min_count=min_count, num_iters=num_iters)
    finally:
        if own_post is not None:
            own_post.close()
    out["stats"] = stats
    return out


def gmm_est_fmllr(model, tm, utts, post, **kw) -> dict:
    """gmm-est-fmllr with every utterance of the set belonging to ONE speaker: -> gmm_est_fmllr_batch's dict with W [dim, dim + 1]."""
    r = gmm_est_fmllr_batch(model, tm, utts, post, np.zeros(utts.n_utt, np.int32), n_spk=1, **kw)
    for k in ("W", "W64", "objf_impr", "count", "status"):
        if k in r:
            r[k] = r[k][0]
    return r


def transform_feats_batch(utts, utt2spk, W, out: Optional[int] = None, n_spk: int = 0) -> None:
    """transform-feats on the set's resident rows: utterance u through W[utt2spk[u]] (copied where utt2spk[u] < 0).  W: float32
    [n_spk, dim, dim + 1] on the host, or a device pointer (int) with n_spk; out: a device pointer for the transformed rows, or None
    to rewrite the set's own rows in place (the set then forgets what it derived from the old ones)."""
    ids = np.ascontiguousarray(utt2spk, np.int32)
    if not isinstance(W, int):
        W = np.ascontiguousarray(W, np.float32)
    utts.transform_feats(ids, W, out, n_spk)


def transform_feats(feats: np.ndarray, W: np.ndarray) -> np.ndarray:
    """transform-feats of one utterance on the host, float32 in the device kernel's order: y = b, then y = fl(A[:, j] x[j] + y) with
    one rounding per step (a fused multiply-add), j ascending."""
    x = np.ascontiguousarray(feats, np.float32)
    W = np.asarray(W, np.float32)
    D = x.shape[1]
    y = np.broadcast_to(W[:, D], (x.shape[0], D)).astype(np.float64)
    for j in range(D):
        y = _fmaf(W[:, j].astype(np.float64)[None, :], x[:, j].astype(np.float64)[:, None], y).astype(np.float64)
    return y.astype(np.float32)


def _fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 fma of float32 values held in float64 arrays: the product is exact in a double; the sum is rounded to ODD in double (its
    error from the two-sum), so the final rounding to float32 is the single rounding of the exact a b + c."""
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    si = s.view(np.int64).copy()
    fix = (e != 0) & ((si & 1) == 0) & np.isfinite(s)
    grow = (e > 0) == (s > 0)
    si[fix & grow] += 1
    si[fix & ~grow] -= 1
    return si.view(np.float64).astype(np.float32)


def compose_transforms(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """compose-transforms: the transform that applies `b` first and `a` second, y = A_a (A_b x + b_b) + b_a (float64 arithmetic,
    float32 result).  Works on one transform or on matching batches."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = a64.shape[-2]
    A = a64[..., :, :D] @ b64[..., :, :D]
    off = np.einsum("...ij,...j->...i", a64[..., :, :D], b64[..., :, D]) + a64[..., :, D]
    return np.concatenate([A, off[..., None]], axis=-1).astype(np.float32)
