"""Inputs for the CMVN / add-deltas tests, shared by tests/test_feat_cpu.py and tests/test_gpu_feat.py, with the
reference results (tests/feat_ref.py) computed once per case."""
import functools

import numpy as np

import feat_ref as ref

SLICE = 1024
STATS_DIMS = (1, 13, 40, 41)
TILE_DIMS = (1, 13, 40)
TILE_LENS = (1, 2, 3, 63, 64, 65, 129)


def stats_layout():
    """(lens, utt2spk, n_spk): speaker 0 one frame; 1, 2, 3 of 1023, 1024 and 1025 frames in one utterance each; 4 with a first slice
    that spans three utterances (500 + 400 + 300: the slice edge falls inside the third) interleaved with the others; 5 without
    utterances; 6 whose only utterance has no frames; one utterance of 7 frames with utt2spk = -1; an utterance of 0 frames of speaker 4"""
    lens = [1, 500, 1023, 400, 7, 1024, 0, 300, 1025, 0]
    u2s = [0, 4, 1, 4, -1, 2, 4, 4, 3, 6]
    return lens, np.array(u2s, np.int32), 7


def int_feats(lens, D, seed):
    """small integers, |x| <= 1024: every sum of x and of x x over fewer than 2^32 frames is exact in fp64"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-1024, 1025, size=(T, D)).astype(np.float32) for T in lens]


def float_feats(lens, D, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.standard_normal((T, D)) * 1.5 + 0.7, np.float32) for T in lens]


@functools.lru_cache(maxsize=None)
def stats_case(D, kind):
    lens, u2s, S = stats_layout()
    feats = int_feats(lens, D, 10 + D) if kind == "int" else float_feats(lens, D, 20 + D)
    return lens, u2s, S, feats, ref.cmvn_stats(feats, u2s, S)


def int_sums(feats, u2s, S):
    """numpy's integer sums: the exact statistics of integer features"""
    D = feats[0].shape[1]
    st = np.zeros((S, 2, D + 1), np.int64)
    for f, s in zip(feats, u2s):
        if s >= 0:
            x = f.astype(np.int64)
            st[s, 0, :D] += x.sum(0)
            st[s, 0, D] += len(x)
            st[s, 1, :D] += (x * x).sum(0)
    return st.astype(np.float64)


def compute_inputs():
    """statistics [4, 2, D + 1] for cmvn_compute: random, a constant column (the variance floor), count 0, a NaN"""
    D = 5
    rng = np.random.default_rng(5)
    st = np.zeros((4, 2, D + 1))
    x = rng.standard_normal((200, D)) * 3.0 + 1.0
    x[:, 2] = 0.1                                         # 0.1 is not representable: s2 / n - mean^2 is a rounding residue, below the floor
    for s in (0, 2, 3):
        st[s, 0, :D], st[s, 0, D], st[s, 1, :D] = x.sum(0), len(x), (x * x).sum(0)
    st[1] = st[0]
    st[1, 0, :D], st[1, 1, :D] = 200 * 0.1, 200 * 0.1 * 0.1      # every column constant
    st[2, 0, D] = 0.0
    st[3, 0, 1] = np.nan
    return st


def tile_set(D, seed=0, lens=TILE_LENS):
    """every test utterance between two neighbours whose rows are 1e30 (a read across an utterance boundary cannot stay hidden); the
    last utterance of the set is a test utterance too.  -> (lens of all, feats of all, indices of the test utterances)"""
    rng = np.random.default_rng(100 + D + seed)
    all_lens, feats, mine = [], [], []
    for T in lens:
        all_lens.append(3)
        feats.append(np.full((3, D), 1e30, np.float32))
        mine.append(len(all_lens))
        all_lens.append(T)
        feats.append(np.ascontiguousarray(rng.standard_normal((T, D)) * 2.0 + 0.5, np.float32))
    all_lens.append(3)
    feats.append(np.full((3, D), 1e30, np.float32))
    mine.append(len(all_lens))
    all_lens.append(5)
    feats.append(np.ascontiguousarray(rng.standard_normal((5, D)), np.float32))      # the last utterance of the set
    return all_lens, feats, mine
