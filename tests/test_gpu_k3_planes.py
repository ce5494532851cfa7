"""K3's wave form with both phases on the fp16 matrix cores (k3_accumulate_wave16): one frame-major LDS image read by rows (phase A)
and through transposed reads (phase B), filled either by the in-loop split of the raw features (KHG_OPT_K3_PLANES = off) or from the
set's split feature records (k3_pack_x; the default where they fit).  Both fills put the same bits into LDS, so every accumulator
array is np.array_equal between them; against the oracle the suite's 2e-5 holds (tests/test_gpu_parity.py).  Alignments are uploaded
(khg_ali_upload), so that the per-pdf frame counts are the chosen ones: the tile edges of the 16-frame tiles and 32-frame pairs."""
import numpy as np
import pytest

from helpers import build
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 65]       # frames per pdf: nothing, one lane, a tile -1 / exact / +1, a pair -1 / exact / +1, two pairs + 1
N_UTT = 20                                        # (more than the 16 utterances of a small set: those never build records by themselves)
KEYS = ("occ", "mean_acc", "var_acc", "trans_acc")


def _case(P, G, D, rot, seed=3):
    """Model, features and an alignment with COUNTS (rotated by `rot`) frames per pdf, the frames of a pdf scattered over the utterances."""
    m, gc, om, ut, cost = build(P, G, D, n_utt=24, seed=seed, max_phones=6)
    counts = np.array([COUNTS[(rot + p) % len(COUNTS)] for p in range(P)])
    N = int(counts.sum())
    # frames of the synthetic set that belong to the pdf (a frame under a foreign pdf has posteriors fp32 does not define to 2e-5:
    # tests/helpers.py, assert_matches_oracle_replay), in a random order
    pdf_of = m.id2pdf[ut.ref_ali]
    pick = np.concatenate([np.nonzero(pdf_of == p)[0][: counts[p]] for p in range(P)])
    assert len(pick) == N, "the synthetic set holds too few frames of a pdf"
    np.random.default_rng(seed + rot).shuffle(pick)
    feats = np.ascontiguousarray(ut.feats[pick], np.float32)
    ali = np.ascontiguousarray(ut.ref_ali[pick], np.int32)
    frame_off = np.linspace(0, N, N_UTT + 1).astype(np.int64)
    assert (np.bincount(m.id2pdf[ali], minlength=P) == counts).all() and (np.diff(frame_off) > 0).all()
    return m, gc, om, feats, ali, frame_off, counts


def _oracle(m, om, D, feats, ali, frame_off):
    oa = orc.OAccs(int(m.gauss_off[-1]), D, m.num_tids)
    for u in range(len(frame_off) - 1):
        a, b = int(frame_off[u]), int(frame_off[u + 1])
        orc.acc_stats_ali(om, m.id2pdf, feats[a:b], ali[a:b], oa)
    return oa


def _assert_oracle(got, oa):
    assert (got["trans_acc"] == oa.trans_acc).all() and got["total_frames"] == oa.total_frames
    assert got["total_log_like"] == pytest.approx(oa.total_log_like, rel=2e-6)
    np.testing.assert_allclose(got["occ"], oa.occ, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(got["mean_acc"], oa.mean_acc, rtol=2e-5, atol=2e-6 * np.abs(oa.mean_acc).max())
    np.testing.assert_allclose(got["var_acc"], oa.var_acc, rtol=2e-5, atol=2e-6 * np.abs(oa.var_acc).max())


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert a["total_frames"] == b["total_frames"] and a["total_log_like"] == pytest.approx(b["total_log_like"], rel=1e-12), what


def _run(ctx, dm, tm, us):
    from kaldi_hmm_gmm_amd import DeviceAccs

    accs = DeviceAccs(ctx, dm, tm)
    us.acc_stats(dm, tm, accs, weight=1.0)
    got = accs.download()
    accs.close()
    return got


def _objects(ctx, m, gc, feats, frame_off, ali):
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet

    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, tm, frame_off, feats)
    us.upload_ali(ali)
    return dm, tm, us


@pytest.mark.parametrize("ny", [0, 3])
@pytest.mark.parametrize("D", [40, 39, 13])
@pytest.mark.parametrize("P,G,rot", [(6, 33, 0), (6, 48, 3), (6, 64, 6)])
def test_records_equal_the_in_loop_split(ctx, opt, P, G, D, rot, ny):
    """Edge shapes (NB = 3 and 4; D even, odd, short; every tile edge among the per-pdf frame counts), one block per pdf and three
    slices per pdf (k3_ny = 3: the slices park images, k3_wave_finalize adds them): the default path reads the records, `off` -- the
    one-image kernel with the in-loop split, part 1 alone -- builds none, both give the same bits and the oracle's statistics."""
    m, gc, om, feats, ali, frame_off, counts = _case(P, G, D, rot)
    if ny:
        opt("k3_ny", ny)
    dm, tm, us = _objects(ctx, m, gc, feats, frame_off, ali)
    nothing = us.k3_planes()
    assert nothing == {"bytes": 0, "packs": 0, "used": False}
    opt("k3_planes", 1)
    off = _run(ctx, dm, tm, us)
    assert us.k3_planes() == nothing, "off: no buffer, no pack"
    opt("k3_planes", 0)
    got = _run(ctx, dm, tm, us)
    assert us.k3_planes() == {"bytes": 320 * (len(ali) + 1), "packs": 1, "used": True}
    again = _run(ctx, dm, tm, us)
    assert us.k3_planes()["packs"] == 1, "the records are reused"
    _same(got, off, "records against the in-loop split")
    _same(again, got, "second pass on the same records")
    _assert_oracle(got, _oracle(m, om, D, feats, ali, frame_off))
    per_pdf = np.add.reduceat(got["occ"], m.gauss_off[:-1].astype(np.int64))
    np.testing.assert_allclose(per_pdf, counts, rtol=1e-5, atol=1e-4)
    us.close(); tm.close(); dm.close()


def test_changed_exponents_repack(ctx, opt):
    """A model whose dimension 5 is twice as wide (means x 2, variances x 4) has twice the envelope there, so k3_ex one / two lower
    (and the same S: the fp16 domain holds as before): the records are made again, once, and the statistics are those of the in-loop
    split.  (The features no longer match the model in that dimension: only the two paths are compared.)"""
    import dataclasses
    from kaldi_hmm_gmm_amd import DeviceModel

    m, gc, om, feats, ali, frame_off, _ = _case(6, 48, 40, 1)
    dm, tm, us = _objects(ctx, m, gc, feats, frame_off, ali)
    _run(ctx, dm, tm, us)
    assert us.k3_planes()["packs"] == 1 and us.k3_planes()["used"]
    means, inv_vars = m.means.copy(), m.inv_vars.copy()
    means[:, 5] *= 2.0
    inv_vars[:, 5] *= 0.25
    m2 = dataclasses.replace(m, means=means, inv_vars=inv_vars, means_invvars=(means * inv_vars).astype(np.float32))
    gc2 = orc.model_gconsts(m2.gauss_off, m2.weights, m2.inv_vars, m2.means_invvars)
    dm2 = DeviceModel(ctx, m2.gauss_off, gc2, m2.means_invvars, m2.inv_vars)
    got = _run(ctx, dm2, tm, us)
    assert us.k3_planes()["packs"] == 2 and us.k3_planes()["used"]
    _run(ctx, dm2, tm, us)
    assert us.k3_planes()["packs"] == 2
    opt("k3_planes", 1)
    off = _run(ctx, dm2, tm, us)
    assert not us.k3_planes()["used"]
    _same(got, off, "after the re-pack")
    us.close(); tm.close(); dm.close(); dm2.close()


def test_rewritten_features_repack(ctx, opt):
    """Borrowed device features rewritten in place + khg_utts_features_changed: the next pass packs again and equals the in-loop split
    of the new features.  (Without the call the records are stale by contract: nothing is asserted.)"""
    import torch
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet

    m, gc, om, feats, ali, frame_off, _ = _case(6, 64, 39, 2)
    t = torch.from_numpy(feats).cuda()
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, tm, frame_off, (t.data_ptr(), t), dim=39)
    us.upload_ali(ali)
    first = _run(ctx, dm, tm, us)
    assert us.k3_planes()["packs"] == 1
    feats2 = np.ascontiguousarray(feats * np.float32(0.97) + np.float32(0.01))
    t.copy_(torch.from_numpy(feats2))
    torch.cuda.synchronize()
    us.features_changed()
    got = _run(ctx, dm, tm, us)
    assert us.k3_planes()["packs"] == 2 and us.k3_planes()["used"]
    opt("k3_planes", 1)
    off = _run(ctx, dm, tm, us)
    _same(got, off, "after features_changed")
    assert not np.array_equal(got["mean_acc"], first["mean_acc"])
    _assert_oracle(got, _oracle(m, om, 39, feats2, ali, frame_off))
    us.close(); tm.close(); dm.close()


def test_split_mode_second_pass_reads_the_records(ctx, opt):
    """An asynchronous align of more than 64 utterances in which every eighth utterance has scores without structure, so that the narrow
    beam leaves it to the order-faithful decoders (status bit 8; tests/test_gpu_shared_graph.py): khg_acc_stats accumulates the
    certified utterances, then the flagged ones' frames in a second pass -- from the same records, packed once, with the bits of the
    in-loop split.  (K3 reads the features under the model whatever the scores were: only the two paths are compared.)"""
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet

    P, G, D, U = 12, 48, 40, 96
    m, gc, om, ut, cost = build(P, G, D, n_utt=U, seed=5, min_phones=2, max_phones=4)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    us = UtteranceSet(ctx, tm, ut.frame_off, ut.feats, graphs=ut.graphs)
    off, pdfs = us.pdf_lists()
    rng = np.random.default_rng(6)
    scores = []
    for u in range(U):
        pl = np.asarray(pdfs[off[u]: off[u + 1]])
        ref = m.id2pdf[ut.ref_ali[ut.frame_off[u]: ut.frame_off[u + 1]]]
        if u % 8 == 3:
            scores.append((-8 * rng.random((len(pl), len(ref)))).astype(np.float32))
        else:                                         # the reference path far ahead of every other: certified at any beam
            scores.append(np.where(pl[:, None] == ref[None, :], 0.0, -50.0).astype(np.float32))
    us.upload_loglikes(scores)
    cfg = dict(beam=0.5, retry_beam=40.0, min_active=0)       # (with the default min_active a chain graph never loses its last tokens)
    st = us.align(tm, **cfg)["status"]
    flagged = int((st & 8 != 0).sum())
    print("utterances through the order-faithful decoder:", flagged, "of", U)
    assert 0 < flagged < U
    out = []
    for planes in (0, 1):
        opt("k3_planes", planes)
        assert us.align(tm, download=False, **cfg) is None
        out.append(_run(ctx, dm, tm, us))
        info = us.k3_planes()
        assert info["used"] == (planes == 0) and info["packs"] == 1
    _same(out[0], out[1], "split mode")
    assert out[0]["total_frames"] > 0
    us.close(); tm.close(); dm.close()
