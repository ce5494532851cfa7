"""Cases of the LDA tests (tests/test_lda_cpu.py, tests/test_gpu_lda.py): seeded statistics for the host estimate, and sets with
posteriors for the device accumulation -- computed once per case and shared read-only."""
import functools

import numpy as np

import lda_ref as ref

ESTIMATE_CASES = [(2, 1, 1), (3, 5, 2), (7, 17, 6), (12, 117, 11)]        # C, Dz, target_dim


@functools.lru_cache(maxsize=None)
def estimate_case(C, Dz, seed=11):
    """statistics of 60 Dz + 200 float32 frames in C classes: class means of decreasing spread along random directions (so that the
    eigenvalues of P are apart), within-class noise through a fixed mild mixing matrix (so that Wc is well conditioned)"""
    rng = np.random.default_rng(seed + 100 * C + Dz)
    T = 60 * Dz + 200
    mu = rng.standard_normal((C, Dz)) * (3.0 / (1.0 + np.arange(C)))[:, None] + 0.5
    A = np.eye(Dz) + 0.3 * rng.standard_normal((Dz, Dz)) / np.sqrt(Dz)
    cls = np.concatenate([np.arange(C), rng.integers(0, C, T - C)])
    x = (mu[cls] + rng.standard_normal((T, Dz)) @ A.T).astype(np.float32).astype(np.float64)
    w = rng.uniform(0.25, 1.0, T)
    zero = np.bincount(cls, weights=w, minlength=C)
    first = np.zeros((C, Dz))
    np.add.at(first, cls, w[:, None] * x)
    second = (w[:, None] * x).T @ x
    second = 0.5 * (second + second.T)
    out = dict(zero=zero, first=first, second=second, packed=ref.packed(second))
    for v in out.values():
        v.setflags(write=False)
    return out
