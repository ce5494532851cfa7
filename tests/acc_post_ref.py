"""The yardstick of khg_acc_stats_post (gmm-acc-stats) and its test inputs.

`oracle_post` is the oracle, never the library: one call of orc.acc_stats_ali on the entry's one frame per (utterance, frame,
transition-id, weight) entry, with weight = (float)((double)scale * w64) -- literally AccumulateForGmm(am, x[u][t], id2pdf[tid], w)
per entry.  The oracle's own transition count is 1 per frame (an alignment's), so the transition statistics are summed here:
trans_acc[tid] += (double)w, in entry order.  `exact_post` is the same rule as plain float64 numpy, `random_posts` the seeded
posterior generator, `bucket_edge_posts` the construction of the bucket-edge test.

Where the yardstick is defined.  The tolerances are the project's own for K3 (occ rtol 2e-5 ...), and they hold where the
reference's fp32 chain determines a frame's posteriors that well: on a frame under a pdf that fits it.  Under a pdf that does not
(synth's pdfs lie ~27 sigma apart: |ll| ~ 400, one ulp 3e-5) two Gaussians of that pdf can compete, and their posteriors move by
1e-4 .. 1e-3 with the ORDER of the fp32 sum (tests/helpers.py says the same of the alignment tests).  Measured with ids drawn
uniformly and weights in (0.05, 1): the oracle itself against float64 at 0.97 x (30 x 8 x 39) and 1.42 x (30 x 64 x 40, 3 elements
out) the occ tolerance; the device against the oracle up to 6.6e-4 relative on 1 .. 8 % of the occupancies at every shape, on the
same elements in the MFMA and the VALU form, which share K1's fmaf chain and nothing else.  So `random_posts` keeps what a
posterior is: the ids of the frame's own pdf carry the ordinary weights, ids of other pdfs a weight in (1e-5, 2e-4) -- at 1e-3
relative their indeterminacy stays a decade under the absolute tolerance, while a misplaced row or weight of such an entry (1e-4
of occupancy on Gaussians that hold none) is a hundred times over it.

Ordinary weights on ids of ANY pdf -- the case of a lattice posterior -- are held to float64 instead (`uniform_posts`,
`exact_post(..., bounds=True)`, `assert_within_bounds`), with a bound derived from the project's own statement of what an fp32
log-likelihood is worth (tests/test_gpu_parity.py): |ll - exact| <= 1e-5 + 1e-6 B, B = |gconst| + sum|M x| + 0.5 sum V x^2.  If every
Gaussian's ll of an entry is off by at most d = 1e-5 + 1e-6 max_g B_g, its softmax moves by a factor within exp(+-2 d); exp and the
division add a few ulps at the arguments that matter (|v - max| < 16: 16 x 2^-24 = 1e-6 each).  So an entry's contribution w gamma_g
(times x_d, x_d^2) is known to w gamma_g (expm1(2 d) + 4e-6), and the bound of a cell is the sum of that over its entries; the
fp64 accumulation and the fp32 products (2^-24 per term) are inside the 4e-6.  The oracle must meet the same bound."""
import functools

import numpy as np

from oracle import oracle as orc

F32 = np.float32


def entry_weight(scale, w64):
    """the rule's one rounding"""
    return F32(np.float64(F32(scale)) * np.float64(w64))


def random_posts(frame_pdfs, id2pdf, seed, normalise=False, max_entries=5):
    """frame_pdfs[u][t]: the pdf that fits frame t of utterance u.  Per frame 0 .. max_entries entries with distinct ids, in random
    order, and positive weights (summing to one per frame when normalise): ids of the frame's own pdf weigh (0.05, 1), ids of other
    pdfs (1e-5, 2e-4) -- see the module's text."""
    rng = np.random.default_rng(seed)
    id2pdf = np.asarray(id2pdf)
    num_tids = len(id2pdf) - 1
    posts = []
    for pdfs in frame_pdfs:
        post = []
        for p in pdfs:
            k = int(rng.integers(0, max_entries + 1))
            own = [int(t) for t in np.nonzero(id2pdf[1:] == int(p))[0] + 1]
            rng.shuffle(own)
            ids = own[:k]
            others = [int(t) for t in rng.permutation(np.arange(1, num_tids + 1)) if id2pdf[t] != int(p)]
            ids += others[:k - len(ids)]
            w = np.array([rng.uniform(0.05, 1.0) if id2pdf[t] == int(p) else rng.uniform(1e-5, 2e-4) for t in ids])
            if normalise and len(ids):
                w = w / w.sum()
            order = rng.permutation(len(ids))
            post.append([(ids[i], float(w[i])) for i in order])
        posts.append(post)
    return posts


def uniform_posts(frame_counts, num_tids, seed, max_entries=5):
    """Per frame 0 .. max_entries entries, ids drawn uniformly from ALL transition-ids (distinct), weights in (0.05, 1)."""
    rng = np.random.default_rng(seed)
    posts = []
    for T in frame_counts:
        post = []
        for _ in range(int(T)):
            k = int(rng.integers(0, max_entries + 1))
            ids = rng.choice(np.arange(1, num_tids + 1), size=min(k, num_tids), replace=False)
            post.append([(int(t), float(w)) for t, w in zip(ids, rng.uniform(0.05, 1.0, size=len(ids)))])
        posts.append(post)
    return posts


def utt_pdfs(ut):
    """the generating pdf of every frame of a synthetic set, per utterance"""
    return [ut.frame_pdf[ut.frame_off[u]: ut.frame_off[u + 1]] for u in range(len(ut.frame_off) - 1)]


def oracle_post(om, id2pdf, sumG, D, num_tids, feats_list, posts, scale=1.0):
    """-> dict of the statistics the entries add, in the layout of DeviceAccs.download()"""
    oa = orc.OAccs(sumG, D, num_tids)
    trans = np.zeros(num_tids + 1, np.float64)
    frames, sum_abs = 0.0, 0.0
    for x, post in zip(feats_list, posts):
        assert len(post) in (0, len(x))
        for t, frame in enumerate(post):
            for tid, w64 in frame:
                w = entry_weight(scale, w64)
                orc.acc_stats_ali(om, id2pdf, x[t:t + 1], [tid], oa, weight=float(w))
                trans[tid] += np.float64(w)
                frames += np.float64(w)
                sum_abs += abs(np.float64(w))
    return {"occ": oa.occ.copy(), "mean_acc": oa.mean_acc.copy(), "var_acc": oa.var_acc.copy(), "trans_acc": trans,
            "total_frames": oa.total_frames, "total_log_like": oa.total_log_like, "sum_abs_w": sum_abs, "frames_seq": frames}


def exact_post(m, gc, feats_list, posts, scale=1.0, bounds=False):
    """the same statistics in plain float64 numpy (no fp32 chain, no fp32 products); bounds: also "bound", the per-cell bounds of an
    fp32 evaluation's distance to them (the module's text)"""
    sumG, D = int(m.gauss_off[-1]), m.dim
    occ, mean, var = np.zeros(sumG), np.zeros((sumG, D)), np.zeros((sumG, D))
    b_occ, b_mean, b_var = np.zeros(sumG), np.zeros((sumG, D)), np.zeros((sumG, D))
    trans = np.zeros(m.num_tids + 1)
    tot_ll, frames = 0.0, 0.0
    for x, post in zip(feats_list, posts):
        x64 = np.asarray(x, np.float64)
        for t, frame in enumerate(post):
            for tid, w64 in frame:
                w = np.float64(entry_weight(scale, w64))
                p = int(m.id2pdf[tid])
                a, b = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
                ll = gc[a:b].astype(np.float64) + m.means_invvars[a:b].astype(np.float64) @ x64[t] \
                    - 0.5 * (m.inv_vars[a:b].astype(np.float64) @ (x64[t] * x64[t]))
                mx = ll.max()
                e = np.exp(ll - mx)
                g = w * e / e.sum()
                occ[a:b] += g
                mean[a:b] += g[:, None] * x64[t][None, :]
                var[a:b] += g[:, None] * (x64[t] * x64[t])[None, :]
                tot_ll += (mx + np.log(e.sum())) * w
                frames += w
                trans[tid] += w
                if bounds:
                    B = np.abs(gc[a:b].astype(np.float64)) + np.abs(m.means_invvars[a:b].astype(np.float64)) @ np.abs(x64[t]) \
                        + 0.5 * (m.inv_vars[a:b].astype(np.float64) @ (x64[t] * x64[t]))
                    r = np.abs(g) * (np.expm1(2.0 * (1e-5 + 1e-6 * B.max())) + 4e-6)
                    b_occ[a:b] += r
                    b_mean[a:b] += r[:, None] * np.abs(x64[t])[None, :]
                    b_var[a:b] += r[:, None] * (x64[t] * x64[t])[None, :]
    out = {"occ": occ, "mean_acc": mean, "var_acc": var, "trans_acc": trans, "total_frames": frames, "total_log_like": tot_ll}
    if bounds:
        out["bound"] = {"occ": b_occ, "mean_acc": b_mean, "var_acc": b_var}
    return out


def assert_within_bounds(got, exact, what=""):
    """got's occ / mean_acc / var_acc within exact_post(..., bounds=True)'s per-cell bounds (+ 1e-12); -> the largest error / bound"""
    worst = 0.0
    for k in ("occ", "mean_acc", "var_acc"):
        err, bound = np.abs(np.asarray(got[k]) - exact[k]), exact["bound"][k] + 1e-12
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (what, k, float((err / bound).max()))
    return worst


def assert_stats(got, want, what=""):
    """the project's tolerances for K3 (tests/test_gpu_parity.py) and, for the transition statistics and total_frames, the
    re-association of at most 10^4 widened floats: |got - want| <= 1e-12 * sum|w|"""
    np.testing.assert_allclose(got["occ"], want["occ"], rtol=2e-5, atol=1e-6, err_msg=str(what))
    np.testing.assert_allclose(got["mean_acc"], want["mean_acc"], rtol=2e-5, atol=2e-6 * np.abs(want["mean_acc"]).max(), err_msg=str(what))
    np.testing.assert_allclose(got["var_acc"], want["var_acc"], rtol=2e-5, atol=2e-6 * np.abs(want["var_acc"]).max(), err_msg=str(what))
    assert abs(got["total_log_like"] - want["total_log_like"]) <= 2e-6 * abs(want["total_log_like"]), (what, got["total_log_like"], want["total_log_like"])
    if "sum_abs_w" in want:
        bound = 1e-12 * want["sum_abs_w"]
        err_t = np.abs(np.asarray(got["trans_acc"]) - want["trans_acc"]).max()
        err_f = abs(got["total_frames"] - want["total_frames"])
        print("%s: trans_acc err %.3g, total_frames err %.3g, bound %.3g" % (what, err_t, err_f, bound))
        assert err_t <= bound and err_f <= bound, (what, err_t, err_f, bound)


# ---- the bucket-edge construction: P = 4 (ids 2 p + 1, 2 p + 2 of synth.make_model), one utterance ------------------------
EDGE_PDF = np.repeat(np.array([0, 2, 3], np.int32), [129, 1000, 61])       # the pdf every frame is drawn from (and fits)
EDGE_T = len(EDGE_PDF)                                                      # 1190 frames


def bucket_edge_posts(n, seed=5):
    """pdf 0 receives exactly n entries (id 1 or 2 on n of its 129 frames; the others stay without an entry), pdf 1 none, pdf 2 three
    on each of its 1000 frames (ids 5, 6 and 5 again: ids may repeat within a frame) = 3000, pdf 3 one per frame of its own (id 7
    or 8).  Every entry sits on a frame of its own pdf (the module's text); weights in (0.05, 1).  The frames are shuffled."""
    rng = np.random.default_rng(seed + n)
    order = edge_order()
    on0 = np.zeros(129, bool)
    on0[rng.choice(129, size=n, replace=False)] = True
    post = []
    for t in order:
        p = int(EDGE_PDF[t])
        w = [float(x) for x in rng.uniform(0.05, 1.0, size=3)]
        if p == 0:
            post.append([(int(rng.integers(1, 3)), w[0])] if on0[t] else [])
        elif p == 2:
            post.append([(5, w[0]), (6, w[1]), (5, w[2])])
        else:
            post.append([(int(rng.integers(7, 9)), w[0])])
    return [post]


def edge_order():
    return np.random.default_rng(123).permutation(EDGE_T)


def entries_per_pdf(posts, id2pdf, P):
    cnt = np.zeros(P, np.int64)
    for post in posts:
        for frame in post:
            for tid, _ in frame:
                cnt[int(id2pdf[tid])] += 1
    return cnt


@functools.lru_cache(maxsize=None)
def edge_model():
    """(model, gconsts, oracle model, features [EDGE_T, 40]) of the bucket-edge test"""
    from kaldi_hmm_gmm_amd import synth
    m = synth.make_model(4, 64, 40, seed=20230414 + 41)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    om = orc.OModel(m.gauss_off, gc, m.means_invvars, m.inv_vars)
    x = synth.sample_feats(m, EDGE_PDF[edge_order()], np.random.default_rng(77))
    return m, gc, om, np.ascontiguousarray(x, np.float32)
