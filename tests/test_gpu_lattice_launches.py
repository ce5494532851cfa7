"""The launch sequence of every operation on a resident lattice handle that no other test pins: with kernel timing on, one call of
best_path, prune, posteriors (twice), boost, mpe_posteriors, lm_rescore, add_penalty, oracle, wer and mbr on a fresh handle each, and
the exact list of timing names the call leaves: which kernels an operation launches, in which order, and which launches share one
timing entry.  Every operation is then called a second time on the same handle and must give the same bits: scratch freed before its
last reader would show here.

The handle is the smallest with an empty utterance beside non-empty ones: the first five non-empty lattices of
lattice_geometry_cases.many_utterances() and one empty lattice, one chunk of six utterances."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_geometry_cases as gc  # noqa: E402
import lattice_mpe_cases as mc  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402

pytestmark = pytest.mark.gpu
SIL = np.asarray(mc.SILENCE, np.int32)
BEST_PATH = ["k2_lattice_best_path", "k2_lattice_ops_words", "k2_lattice_ops_words"]       # the kernel, the scan of the counts, the packing
POST_TAIL = ["k2_lattice_post_scan", "k2_lattice_post_fill"]
INDEX = "k2_lattice_post_index"


@pytest.fixture(scope="module")
def work():
    """(khg, ctx, make: -> a fresh handle of the six lattices, what the calls need beside it)"""
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _gpu
    lats = [x for x in gc.many_utterances() if len(x["frame"])][:5]
    lats.insert(2, ops.empty_lattice())
    Ls = [khg.Lattice.from_arrays(*[x[k] for k in ops.FIELDS], int(x["start"])) for x in lats]
    best = [L.best_path(1.0, 1.0) for L in Ls]
    assert [b["status"] for b in best] == [ops.SUCCEEDED, ops.SUCCEEDED, ops.NO_PATH, ops.SUCCEEDED, ops.SUCCEEDED, ops.SUCCEEDED]
    nt = max(mc.num_tids_of(x) for x in lats)
    tid2phone, tid2pdf = mc.tables(nt)
    words = sorted({int(w) for x in lats for w in x["olabel"] if w > 0}) or [1]
    aux = {
        "alis": [np.asarray(b["ali"], np.int32) for b in best],            # a reference alignment of the lattice's own length
        "refs": [[int(w) for w in b["words"]] + [words[0]] for b in best],    # the best path's words and one more
        "tid2phone": tid2phone, "tid2pdf": tid2pdf,
        "lm": khg.NgramLm.unigram({w: 1.0 / len(words) for w in words}),
    }

    def make():
        dl = khg.DeviceLattices.from_lattices(Ls)
        assert dl.num_chunks == 1 and dl.num_utts == 6
        return dl
    return khg, _gpu.default_context(), make, aux


def _launches(ctx, call):
    """-> (call's result, the names of the context's kernel timings that the call left)"""
    ctx.sync(); ctx.timings(); ctx.set_timing(True)
    try:
        out = call()
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.set_timing(False)
    return out, names


def _arrays(d):
    return [(k, np.asarray(d[k]).dtype.str, np.asarray(d[k]).tobytes()) for k in sorted(d)]


def _lattices(dl):
    st = dl.status
    return [None if st is None else st.tolist(), dl.state_off.tolist(), dl.arc_off.tolist(),
            [[np.asarray(getattr(L, k)).tobytes() for k in ops.FIELDS] + [L.start] for L in dl.download()]]


def _posteriors(P):
    av = P.avg_acc
    return [P.status.tolist(), P.tot_like.tobytes(), None if av is None else av.tobytes(), P.frame_off.tolist(), P.entry_off.tolist(),
            [a.tobytes() for a in P.arc_post()], [[[(int(t), np.float64(w).tobytes()) for t, w in row] for row in u] for u in P.download()]]


def _lm(r):
    return [_lattices(r[0]), r[1].tolist(), sorted(r[2].items())]


def _check(work, call, bits, want):
    """one timed call on a fresh handle leaves exactly the names `want`; a second call on the same handle gives the same bits"""
    khg, ctx, make, aux = work
    dl = make()
    first, names = _launches(ctx, lambda: call(dl, aux))
    assert names == want
    assert bits(first) == bits(call(dl, aux))
    dl.close()


def test_best_path(work):
    _check(work, lambda dl, aux: dl.best_path([1.0, 0.5], [1.0, 0.1]), _arrays, BEST_PATH)


def test_prune(work):
    _check(work, lambda dl, aux: dl.prune(0.5), _lattices, ["k2_lattice_prune_mark", "k2_lattice_prune_scan", "k2_lattice_prune_fill"])


def test_posteriors_twice(work):
    """the in-arc index is made by the first call on a handle and found there by the second"""
    khg, ctx, make, aux = work
    dl = make()
    P0, names = _launches(ctx, lambda: dl.posteriors(1.0, 0.1))
    assert names == [INDEX, "k2_lattice_post_fb"] + POST_TAIL
    P1, names = _launches(ctx, lambda: dl.posteriors(1.0, 0.1))
    assert names == ["k2_lattice_post_fb"] + POST_TAIL
    assert _posteriors(P0) == _posteriors(P1)
    dl.close()


def test_boost(work):
    _check(work, lambda dl, aux: dl.boost(aux["tid2phone"], SIL, alignment=aux["alis"], b=0.5), _lattices, ["k2x_label_check", "k2x_boost"])


def test_mpe_posteriors(work):
    _check(work, lambda dl, aux: dl.mpe_posteriors(aux["tid2phone"], SIL, alignment=aux["alis"], criterion="smbr", tid2pdf=aux["tid2pdf"]),
           _posteriors, ["k2x_label_check", INDEX, "k2_lattice_post_mpe"] + POST_TAIL)


def test_lm_rescore(work):
    khg = work[0]
    dlm = khg.DeviceLm(work[3]["lm"])
    _check(work, lambda dl, aux: dl.lm_rescore(dlm, 1.0, 8), _lm, [INDEX, "k2_lattice_lm_mark", "k2_lattice_lm_scan", "k2_lattice_lm_fill"])
    dlm.close()


def test_add_penalty(work):
    _check(work, lambda dl, aux: dl.add_penalty(0.5), _lattices, ["k2_lattice_score_add_penalty"])


def test_oracle(work):
    _check(work, lambda dl, aux: dl.oracle(aux["refs"]), _arrays, [INDEX, "k2_lattice_score_oracle"])


def test_wer(work):
    _check(work, lambda dl, aux: dl.wer(aux["refs"], [1.0, 0.5], [1.0, 0.1], [0.0, 0.5]), _arrays,
           ["k2_lattice_score_best_path", "k2_lattice_score_wer"])


def test_mbr_without_initial_hypotheses(work):
    """the initial hypotheses are the best path's words: its launches come first.  The rule lattices carry epsilon loops, which the
    forward-backward pass refuses (KHG_LAT_EPS_LOOP), so no utterance of this handle reaches k2_lattice_mbr: the list ends with the
    preparation (the next test has utterances that run)"""
    _check(work, lambda dl, aux: dl.mbr(1.0, 0.1, True, 32, None, 0, 0), _arrays, BEST_PATH + [INDEX, "k2_lattice_mbr_weights", "k2_lattice_mbr_prepare"])


def test_mbr_of_utterances_that_run(work):
    """four hand-built lattices of lattice_mbr_cases, each a single path with words: every utterance goes through k2_lattice_mbr, in one
    launch"""
    import lattice_mbr_cases as bc
    khg, ctx = work[0], work[1]
    Ls = [khg.Lattice.from_arrays(*[x["lat"][k] for k in ops.FIELDS], int(x["lat"]["start"])) for x in bc.hand_cases()[:4]]
    dl = khg.DeviceLattices.from_lattices(Ls)
    first, names = _launches(ctx, lambda: dl.mbr(1.0, 0.1, True, 32, None, 0, 0))
    assert first["status"].tolist() == [ops.SUCCEEDED] * 4
    assert names == BEST_PATH + [INDEX, "k2_lattice_mbr_weights", "k2_lattice_mbr_prepare", "k2_lattice_mbr"]
    assert _arrays(first) == _arrays(dl.mbr(1.0, 0.1, True, 32, None, 0, 0))
    dl.close()
