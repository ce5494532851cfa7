"""Scoring lattices on the device (the rules are written out at khg_lattices_oracle in include/khg_hip.h):
lattice-add-penalty, lattice-oracle, compute-wer and the sweep of Kaldi's score.sh -- lattice-scale | lattice-add-penalty |
lattice-best-path | compute-wer over LMWT x word insertion penalty -- in one call on the lattices a decode left in HBM."""
from typing import Sequence

import numpy as np

from . import _gpu
from ._kaldi_hmm_gmm_amd import edit_distance_counts  # noqa: F401


def _refs(refs):
    return [np.asarray(r, np.int32).reshape(-1) for r in refs]


def _on_device(lattices):
    from .align import DeviceLattices
    on = isinstance(lattices, DeviceLattices)
    return on, lattices if on else DeviceLattices.from_lattices(list(lattices), _gpu.default_context())


def lattice_add_penalty_batch(lattices, word_ins_penalty: float):
    """Kaldi's lattice-add-penalty for several utterances on the device (khg_lattices_add_penalty): graph_cost += word_ins_penalty on
    every arc that carries a word.  lattices: a list of Lattice (-> a list of Lattice) or a DeviceLattices (-> a DeviceLattices)."""
    on, dl = _on_device(lattices)
    try:
        res = dl.add_penalty(float(word_ins_penalty))
    finally:
        if not on:
            dl.close()
    if on:
        return res
    out = res.download()
    res.close()
    return out


def lattice_add_penalty(lattice, word_ins_penalty: float):
    """Kaldi's lattice-add-penalty for one utterance -> the Lattice (lattice_add_penalty_batch of one)."""
    return lattice_add_penalty_batch([lattice], word_ins_penalty)[0]


def lattice_oracle_batch(lattices, refs, scratch_bytes: int = 0):
    """Kaldi's lattice-oracle for several utterances on the device (khg_lattices_oracle): per utterance the lattice path with the fewest
    word errors against refs[u] (word ids > 0).  -> one dict per utterance: status (KHG_LAT_* bits), counts (errors, insertions,
    deletions, substitutions), words, ali (the path's transition-ids by frame).  lattices: a list of Lattice or a DeviceLattices."""
    on, dl = _on_device(lattices)
    try:
        r = dl.oracle(_refs(refs), int(scratch_bytes))
    finally:
        if not on:
            dl.close()
    wo, ao = r["words_off"], r["ali_off"]
    return [{"status": int(r["status"][u]), "counts": r["counts"][u].copy(), "words": r["words"][wo[u]:wo[u + 1]].copy(),
             "ali": r["ali"][ao[u]:ao[u + 1]].copy()} for u in range(len(r["status"]))]


def lattice_oracle(lattice, ref: Sequence[int], scratch_bytes: int = 0):
    """Kaldi's lattice-oracle for one utterance (lattice_oracle_batch of one)."""
    return lattice_oracle_batch([lattice], [ref], scratch_bytes)[0]


def mbr_utterances(r):
    """DeviceLattices.mbr's dict of arrays -> one dict per utterance: status, iters, bayes_risk, words, conf, vocab, gamma [Q][len(vocab)],
    arc_cond, final_cond, and sausage: per position q = 1 .. Q the (word, prob) pairs with prob > 0, by descending prob, then ascending id"""
    wo, vo, go, ao, so = r["words_off"], r["vocab_off"], r["gamma_off"], r["arc_off"], r["state_off"]
    out = []
    for u in range(len(r["status"])):
        vocab = r["vocab"][vo[u]:vo[u + 1]].copy()
        gamma = r["gamma"][go[u]:go[u + 1]].reshape(-1, max(len(vocab), 1))[:, :len(vocab)].copy()
        sausage = [sorted(((int(vocab[k]), float(row[k])) for k in np.flatnonzero(row > 0)), key=lambda x: (-x[1], x[0])) for row in gamma]
        out.append({"status": int(r["status"][u]), "iters": int(r["iters"][u]), "bayes_risk": float(r["bayes_risk"][u]),
                    "words": r["words"][wo[u]:wo[u + 1]].copy(), "conf": r["conf"][wo[u]:wo[u + 1]].copy(), "vocab": vocab, "gamma": gamma,
                    "arc_cond": r["arc_cond"][ao[u]:ao[u + 1]].copy(), "final_cond": r["final_cond"][so[u]:so[u + 1]].copy(), "sausage": sausage})
    return out


def lattice_mbr_decode_batch(lattices, graph_scale: float = 1.0, acoustic_scale: float = 1.0, decode_mbr: bool = True, max_iter: int = 32,
                             init=None, max_words: int = 0, scratch_bytes: int = 0):
    """Kaldi's lattice-mbr-decode and the confidences of lattice-to-ctm-conf for several utterances on the device (khg_lattices_mbr;
    DESIGN.md section 7t): per utterance the hypothesis of least expected word error under the scale pair, a confidence per word and the
    confusion bins.  init: None, or per utterance a word sequence or None (the best path's words).  decode_mbr=False: confidences of the
    initial hypothesis only.  -> one dict per utterance (mbr_utterances).  lattices: a list of Lattice or a DeviceLattices."""
    on, dl = _on_device(lattices)
    if init is not None:
        init = [None if h is None else np.asarray(h, np.int32).reshape(-1) for h in init]
    try:
        r = dl.mbr(float(graph_scale), float(acoustic_scale), bool(decode_mbr), int(max_iter), init, int(max_words), int(scratch_bytes))
    finally:
        if not on:
            dl.close()
    return mbr_utterances(r)


def lattice_mbr_decode(lattice, graph_scale: float = 1.0, acoustic_scale: float = 1.0, decode_mbr: bool = True, max_iter: int = 32, init=None,
                       max_words: int = 0, scratch_bytes: int = 0):
    """lattice-mbr-decode for one utterance (lattice_mbr_decode_batch of one); init: a word sequence or None"""
    return lattice_mbr_decode_batch([lattice], graph_scale, acoustic_scale, decode_mbr, max_iter, None if init is None else [init], max_words,
                                    scratch_bytes)[0]


def compute_wer(refs, hyps):
    """Kaldi's compute-wer --mode=all on word ids, on the host (khg_edit_distance) -> (the WER in percent, the summed counts: errors,
    insertions, deletions, substitutions, and the reference's words)."""
    refs, hyps = _refs(refs), _refs(hyps)
    if len(refs) != len(hyps):
        raise ValueError("compute_wer: %d references for %d hypotheses" % (len(refs), len(hyps)))
    tot = np.zeros(4, np.int64)
    for r, h in zip(refs, hyps):
        tot += edit_distance_counts(r, h)
    n = int(sum(len(r) for r in refs))
    return (100.0 * float(tot[0]) / n if n else 0.0), {"errors": int(tot[0]), "insertions": int(tot[1]), "deletions": int(tot[2]),
                                                      "substitutions": int(tot[3]), "ref_words": n}


def score_lattices(dl, refs, lmwts=range(7, 18), penalties=(0.0, 0.5, 1.0), lattice_acoustic_scale: float = 1.0):
    """The sweep of Kaldi's score.sh on resident lattices, in one call (khg_lattices_wer): for every LMWT and word insertion penalty the
    best path under graph scale 1, acoustic scale 1 / LMWT and the penalty, scored against refs.  dl: a DeviceLattices (or a list of
    Lattice).  lattice_acoustic_scale: the scale the decoder left in the lattices' acoustic costs (Kaldi's lattices hold them unscaled: 1);
    the sweep multiplies them by (1 / LMWT) / lattice_acoustic_scale.  -> (table, best): table[(lmwt, penalty)] = {"wer", "errors", "insertions", "deletions", "substitutions", "ref_words"},
    best = (lmwt, penalty) of the lowest WER (the first among ties, LMWT-major)."""
    refs = _refs(refs)
    points = [(int(w), float(p)) for w in lmwts for p in penalties]
    if not points:
        raise ValueError("score_lattices: no (LMWT, penalty) point")
    on, d = _on_device(dl)
    try:
        r = d.wer(refs, np.ones(len(points), np.float32), np.asarray([1.0 / (w * float(lattice_acoustic_scale)) for w, _ in points], np.float32),
                  np.asarray([p for _, p in points], np.float32))
    finally:
        if not on:
            d.close()
    U = len(refs)
    n = int(sum(len(x) for x in refs))
    counts = r["counts"].reshape(len(points), U, 4).astype(np.int64).sum(axis=1)
    table = {}
    for pt, c in zip(points, counts):
        table[pt] = {"wer": 100.0 * float(c[0]) / n if n else 0.0, "errors": int(c[0]), "insertions": int(c[1]), "deletions": int(c[2]),
                     "substitutions": int(c[3]), "ref_words": n}
    best = min(points, key=lambda pt: table[pt]["errors"])
    return table, best
