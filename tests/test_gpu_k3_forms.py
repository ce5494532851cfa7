"""Every instantiation of K3's accumulate kernels (k3_insts in csrc/khg_k3.hip) on inputs built for it (tests/k3_form_cases.py): the
pass launches the kernel the case names -- UtteranceSet.k3_last() reports what k3_run settled, fallbacks from the fp16 forms
included, so a model or a rule that takes the tests off the fp16 forms fails here instead of passing on another kernel -- and its
statistics are those of the float64 restatement of AccumulateForGmm at the project's tolerances for diffuse posteriors.  Buckets of
0 / 1 / 15 / 16 / 17 / 31 / 32 / 33 / 63 / 64 / 65 / 129 frames in every case: the ends of a tile, a pair and a chunk."""
import numpy as np
import pytest

import k3_form_cases as kc

pytestmark = pytest.mark.gpu

KEYS = ("occ", "mean_acc", "var_acc", "trans_acc")
LDS_MAX = 160 * 1024


def _objects(ctx, b):
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    m = b.m
    dm = DeviceModel(ctx, m.gauss_off, b.gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, tm, np.array(b.frame_off, np.int64), np.array(b.feats, np.float32))      # (copies: the case's arrays are shared and read-only)
    return dm, tm, us, DeviceAccs(ctx, dm, tm)


def _pass(ctx, b, dm, tm, us, accs):
    """one statistics pass of the case into the zeroed block -> the downloaded block"""
    from kaldi_hmm_gmm_amd import DevicePosteriors
    accs.zero()
    c = b.case
    if not c.post:
        us.acc_stats(dm, tm, accs, weight=c.weight)
    else:
        post = DevicePosteriors.from_alignment(us) if c.post == "alignment" else DevicePosteriors.from_arrays(ctx, *[np.array(a) for a in b.post_arrays])
        us.acc_stats_post(dm, tm, post, accs, scale=b.scale)
        post.close()
    return accs.download()


def _records(us):
    last = us.k3_last()
    return [tuple(r[f] for f in kc.FIELDS) for r in last], last


@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_form_case(ctx, opt, name):
    b = kc.build(name)
    c = b.case
    for k, v in c.opts:
        opt(k, v)
    dm, tm, us, accs = _objects(ctx, b)
    assert us.k3_last() == [], "no pass yet"
    if c.post != "arrays":
        us.upload_ali(np.array(b.ali, np.int32))
    got = _pass(ctx, b, dm, tm, us, accs)
    recs, last = _records(us)
    print(name, last)
    assert recs == list(c.expect)
    assert all(0 <= r["lds_bytes"] <= LDS_MAX for r in last)
    ny = dict(c.opts).get("k3_ny")
    if ny:
        assert all(r["ny"] == ny for r in last if r["variant"] != "valu")
    kc.assert_stats(got, b, name)
    if all(r[0] in kc.WAVE_VARIANTS for r in c.expect):
        # the wave forms fold a pdf's slices in one fixed order: the same bits from run to run, parked slice images (k3_ny = 3) included
        again = _pass(ctx, b, dm, tm, us, accs)
        assert _records(us)[0] == recs
        for k in KEYS:
            assert np.array_equal(again[k], got[k]), (name, k)
        assert again["total_frames"] == got["total_frames"] and again["total_log_like"] == got["total_log_like"], name
    accs.close(); us.close(); tm.close(); dm.close()


def test_no_frames_no_runs(ctx):
    """a pass over an alignment without a single transition-id accumulates nothing; the record of the pass before it is gone"""
    b = kc.build("wave16r_4_d40_neg")
    dm, tm, us, accs = _objects(ctx, b)
    us.upload_ali(np.array(b.ali, np.int32))
    _pass(ctx, b, dm, tm, us, accs)
    assert len(us.k3_last()) == 1
    from kaldi_hmm_gmm_amd import DevicePosteriors
    fo = np.asarray(b.frame_off, np.int64)
    empty = DevicePosteriors.from_arrays(ctx, fo, np.zeros(int(fo[-1]) + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64))
    accs.zero()
    us.acc_stats_post(dm, tm, empty, accs)
    assert us.k3_last() == []
    got = accs.download()
    assert not got["occ"].any() and got["total_frames"] == 0.0
    empty.close(); accs.close(); us.close(); tm.close(); dm.close()


def test_default_options_on_a_benchmark_like_set_run_wave16_from_the_records(ctx):
    """The guard of the flagship path: a model and a set like bench.py's -- synth.make_model with 64 Gaussians at D = 40, features
    sampled from it, more than 16 utterances (no arena set), every option at its default -- must run k3_accumulate_wave16<4> on the
    set's split feature records, the kernel the benchmark times, and give the restatement's statistics."""
    from helpers import build
    m, gc, om, ut, _ = build(24, 64, 40, n_utt=24, seed=11, max_phones=4)
    frames = np.arange(len(ut.ref_ali))
    w = np.ones(len(frames), np.float32)
    case = kc.Case("benchmark_like", 40, (64, 64), (kc.wave16r(4),), weight=1.0)
    counts = np.bincount(m.id2pdf[ut.ref_ali], minlength=m.num_pdfs)
    b = kc.Built(case, m, gc, np.ascontiguousarray(ut.feats, np.float32), np.ascontiguousarray(ut.ref_ali, np.int32), ut.frame_off.astype(np.int64),
                 counts, frames, ut.ref_ali, w, None, 1.0, kc.restate(m, gc, ut.feats, frames, ut.ref_ali, w, True), counts.astype(np.float64))
    assert (ut.ref_ali > 0).all() and kc.fp16_domain(m, gc, ut.feats)[:2] == (True, True)
    dm, tm, us, accs = _objects(ctx, b)
    us.upload_ali(np.array(b.ali, np.int32))
    got = _pass(ctx, b, dm, tm, us, accs)
    recs, last = _records(us)
    print(last)
    assert recs == [kc.wave16r(4)] and last[0]["lds_bytes"] <= LDS_MAX
    assert us.k3_planes()["used"]
    kc.assert_stats(got, b, "benchmark-like")
    accs.close(); us.close(); tm.close(); dm.close()
