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
