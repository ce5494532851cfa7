"""The yardstick of khg_acc_stats_post2 (gmm-acc-stats2): the sign split of a batch of posteriors, and the
yardstick of khg_acc_stats_post (tests/acc_post_ref.py) called once per sign.  With w = (float)((double)scale * w64) an entry with
w > 0 belongs to the numerator with weight w, one with w < 0 to the denominator with weight -w, one with w == 0 (a zero, or a product
that underflows a float) to neither.  Rounding to float is symmetric, so -w is the rule's weight under -scale: the denominator's
yardstick is oracle_post(the negative entries, -scale)."""
import numpy as np

import acc_post_ref as ref


def split_posts(posts, scale):
    """-> (the entries with w > 0, those with w < 0), frames kept (empty where nothing is left)"""
    pos = [[[(t, w64) for t, w64 in f if ref.entry_weight(scale, w64) > 0] for f in p] for p in posts]
    neg = [[[(t, w64) for t, w64 in f if ref.entry_weight(scale, w64) < 0] for f in p] for p in posts]
    return pos, neg


def oracle_post2(om, id2pdf, sumG, D, num_tids, feats_list, posts, scale=1.0):
    """-> (num, den): dicts in the layout of DeviceAccs.download()"""
    pos, neg = split_posts(posts, scale)
    return (ref.oracle_post(om, id2pdf, sumG, D, num_tids, feats_list, pos, scale),
            ref.oracle_post(om, id2pdf, sumG, D, num_tids, feats_list, neg, -float(np.float32(scale))))


def exact_post2(m, gc, feats_list, posts, scale=1.0):
    pos, neg = split_posts(posts, scale)
    return ref.exact_post(m, gc, feats_list, pos, scale), ref.exact_post(m, gc, feats_list, neg, -float(np.float32(scale)))
