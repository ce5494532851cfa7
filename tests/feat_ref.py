"""Plain-Python restatement of DESIGN.md section 7p: the CMVN statistics (sums by math.fsum, with sum |terms| and n for the bound of the
device's fp64 sums), ApplyCmvn's normaliser in Python floats, and DeltaFeatures' coefficient recurrence in float32.  The oracle of
tests/test_feat_cpu.py and tests/test_gpu_feat.py; it shares no code with the library."""
import math

import numpy as np

CMVN_OK, CMVN_NO_DATA, CMVN_NONFINITE = 0, 1, 2


def delta_scales(order, window):
    """scales[0] = [1]; cur[j + k] += (float)j * prev[k] over j = -window .. window, k = -po .. po, every step rounded to float32;
    then every element times (float)(1.0 / normalizer)."""
    f32 = np.float32
    scales = [np.array([1.0], f32)]
    for _ in range(order):
        prev = scales[-1]
        po = (len(prev) - 1) // 2
        co = po + window
        cur = [f32(0.0)] * (2 * co + 1)
        normalizer = f32(0.0)
        for j in range(-window, window + 1):
            normalizer = f32(normalizer + f32(j * j))
            for k in range(-po, po + 1):
                cur[j + k + co] = f32(cur[j + k + co] + f32(f32(j) * prev[k + po]))
        inv = f32(1.0 / float(normalizer))
        scales.append(np.array([f32(c * inv) for c in cur], f32))
    return scales


def cmvn_stats(feats, utt2spk, n_spk):
    """-> {"stats" [n_spk, 2, D + 1] by math.fsum (one rounding per element), "abs" the sums of |terms|, "n" the frames per speaker}"""
    D = feats[0].shape[1]
    rows = [[] for _ in range(n_spk)]
    for f, s in zip(feats, utt2spk):
        if s >= 0 and len(f):
            rows[int(s)].append(np.asarray(f, np.float32).astype(np.float64))
    stats, ab, n = np.zeros((n_spk, 2, D + 1)), np.zeros((n_spk, 2, D + 1)), np.zeros(n_spk)
    for s in range(n_spk):
        if not rows[s]:
            continue
        x = np.concatenate(rows[s])
        n[s] = stats[s, 0, D] = ab[s, 0, D] = len(x)
        for d in range(D):
            col = x[:, d].tolist()
            stats[s, 0, d], ab[s, 0, d] = math.fsum(col), math.fsum(abs(v) for v in col)
            stats[s, 1, d] = ab[s, 1, d] = math.fsum(v * v for v in col)         # a float32 squared is exact in a double
    return {"stats": stats, "abs": ab, "n": n}


def cmvn_compute(stats, norm_means, norm_vars, reverse):
    """-> (norm float32 [n_spk, 2, D]: offset, scale; status [n_spk]) by the steps of 7p, one Python-float operation at a time"""
    S, _, D1 = stats.shape
    D = D1 - 1
    norm, status = np.zeros((S, 2, D), np.float32), np.zeros(S, np.int32)
    for s in range(S):
        count = float(stats[s, 0, D])
        st = CMVN_OK if count >= 1.0 else CMVN_NO_DATA
        if st == CMVN_OK:
            for d in range(D):
                mean = float(stats[s, 0, d]) / count
                scale, offset = 1.0, -mean
                if norm_vars:
                    var = float(stats[s, 1, d]) / count - mean * mean
                    if var < 1e-20:
                        var = 1e-20
                    scale = 1.0 / math.sqrt(var) if var == var else float("nan")
                    offset = -(mean * scale)
                    if reverse:
                        scale = math.sqrt(var) if var == var else float("nan")
                if reverse:
                    offset = mean
                with np.errstate(all="ignore"):
                    norm[s, 0, d], norm[s, 1, d] = np.float32(offset), np.float32(scale)
                if not (np.isfinite(norm[s, 0, d]) and np.isfinite(norm[s, 1, d])):
                    st = CMVN_NONFINITE                         # judged before norm_means takes the offset away
                if not norm_means:
                    norm[s, 0, d] = 0.0
        if st != CMVN_OK:
            norm[s, 0], norm[s, 1] = 0.0, 1.0
        status[s] = st
    return norm, status
