"""The four "binary-level" entry points of the reference (scripts/gmm_init_mono.py,
gmm_align_compiled.py, gmm_acc_stats_ali.py, gmm_est.py) with the same names, keyword arguments
and return conventions, plus batched variants that keep a whole shard on the GPU."""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _gpu
from ._lib import KhgError
from .align import AlignConfig, DecodableAmDiagGmmScaled, add_transition_probs, align_batch, align_utterance_wrapper
from .context_dep import monophone_context_dependency, monophone_context_dependency_shared
from .device import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
from .diag_gmm import AmDiagGmm, DiagGmm
from .fst import StdVectorFst
from .hmm_topology import HmmTopology
from .posterior import posts_to_arrays
from .mle import (AccumAmDiagGmm, EbwOptions, EbwWeightOptions, GmmUpdateFlags, MleDiagGmmOptions, mle_am_diag_gmm_update, str_to_gmm_flags,
                  update_ebw_am_diag_gmm, update_ebw_weights_am_diag_gmm)
from .transition_model import MleTransitionUpdateConfig, TransitionModel


def gmm_init_mono(topo: HmmTopology, cuts, shared_phones: Optional[List[List[int]]] = None,
                  perturb_factor: float = 0.0):
    """scripts/gmm_init_mono.py:10-73.  `cuts` is anything with compute_global_feature_stats()
    (lhotse CutSet), a dict with norm_means / norm_stds, or a [N, D] feature matrix."""
    if hasattr(cuts, "compute_global_feature_stats"):
        stats = cuts.compute_global_feature_stats()
        means, stds = np.asarray(stats["norm_means"]), np.asarray(stats["norm_stds"])
    elif isinstance(cuts, dict):
        means, stds = np.asarray(cuts["norm_means"]), np.asarray(cuts["norm_stds"])
    else:
        x = np.asarray(cuts, np.float64)
        means, stds = x.mean(0), x.std(0)
    means = means.astype(np.float32)[None, :]
    variances = np.square(stds.astype(np.float32))[None, :]
    feat_dim = means.shape[1]
    p2n = topo.get_phone_to_num_pdf_classes()
    tree = (monophone_context_dependency(topo.phones, p2n) if shared_phones is None
            else monophone_context_dependency_shared(shared_phones, p2n))
    g = DiagGmm(nmix=1, dim=feat_dim)
    g.set_weights(np.ones(1, np.float32))
    g.set_means(means)
    g.set_invvars(1 / variances)
    g.compute_gconsts()
    am = AmDiagGmm()
    for _ in range(tree.num_pdfs):
        am.add_pdf(g)
    if perturb_factor != 0:
        for i in range(tree.num_pdfs):
            am.get_pdf(i).perturb(perturb_factor)
    return TransitionModel(ctx_dep=tree, hmm_topo=topo), tree, am


def gmm_info(am_gmm: AmDiagGmm, transition_model: TransitionModel) -> Dict[str, int]:
    """scripts/gmm_info.py:9-29 (the key "feature_dimensition" is spelled as the reference spells it)."""
    return {"number_of_phones": len(transition_model.phones), "number_of_pdfs": transition_model.num_pdfs,
            "number_of_transition_ids": transition_model.num_transition_ids,
            "number_of_transition_states": transition_model.num_transition_states, "feature_dimensition": am_gmm.dim,
            "number_of_gaussians": am_gmm.num_gauss}


def gmm_align_compiled(am_gmm: AmDiagGmm, transition_model: TransitionModel, utt: str, fst: StdVectorFst, feats,
                       align_config: AlignConfig, acoustic_scale: float = 1.0, transition_scale: float = 1.0,
                       self_loop_scale: float = 1.0, num_done: int = 0, num_error: int = 0, num_retried: int = 0,
                       tot_like: float = 0, frame_count: int = 0) -> Dict[str, Any]:
    """scripts/gmm_align_compiled.py:10-79 (mutates `fst` like the reference: callers pass a copy)."""
    add_transition_probs(trans_model=transition_model, transition_scale=transition_scale,
                         self_loop_scale=self_loop_scale, fst=fst)
    dec = DecodableAmDiagGmmScaled(am=am_gmm, tm=transition_model, feats=feats, scale=acoustic_scale)
    (num_done, num_error, num_retried, tot_like, frame_count, alignment, words) = align_utterance_wrapper(
        config=align_config, utt=utt, acoustic_scale=acoustic_scale, fst=fst, decodable=dec, num_done=num_done,
        num_error=num_error, num_retried=num_retried, tot_like=tot_like, frame_count=frame_count)
    return {"num_done": num_done, "num_error": num_error, "num_retried": num_retried, "tot_like": tot_like,
            "frame_count": frame_count, "alignment": alignment, "words": words}


def gmm_align_compiled_batch(am_gmm: AmDiagGmm, transition_model: TransitionModel, utts: Sequence[str],
                             fsts: Sequence[StdVectorFst], feats: Sequence[np.ndarray], align_config: AlignConfig,
                             acoustic_scale: float = 1.0, transition_scale: float = 1.0, self_loop_scale: float = 1.0):
    """All utterances of a shard in one GPU pass.  Graphs are NOT mutated: the per-transition-id cost
    AddTransitionProbs would add is applied on the device.  Returns the same counters as the loop of
    single calls would, plus per-utterance alignments / words."""
    cost = transition_model.scaled_trans_cost(transition_scale, self_loop_scale)
    res = align_batch(am_gmm, transition_model, list(fsts), list(feats), align_config, acoustic_scale, trans_cost=cost)
    out = {"num_done": 0, "num_error": 0, "num_retried": 0, "tot_like": 0.0, "frame_count": 0, "alignment": [],
           "words": [], "utts": list(utts)}
    for r in res:
        out["num_retried"] += int(r["retried"])
        if r["ok"]:
            out["num_done"] += 1
            out["tot_like"] += r["like"]
            out["frame_count"] += r["num_frames"]
        else:
            out["num_error"] += 1
        out["alignment"].append(r["alignment"])
        out["words"].append(r["words"])
    return out


def gmm_acc_stats_ali(am_gmm: AmDiagGmm, gmm_accs: AccumAmDiagGmm, transition_model: TransitionModel, feats,
                      ali: List[int], transition_accs: Optional[np.ndarray] = None):
    """scripts/gmm_acc_stats_ali.py:9-58 -> (log_like, transition_accs); gmm_accs is updated in place.
    One K3 pass over the utterance; the model is on the device already (cached on am_gmm, uploaded again only after it changed) and
    the statistics STAY on the device between calls (gmm_accs adds them into its host accumulators when something reads those:
    get_acc, tot_count, mle_am_diag_gmm_update, pickling) -- the reference's caller makes this call once per utterance."""
    feats = np.ascontiguousarray(feats, np.float32)
    return gmm_accs._acc_stats_ali(am_gmm, transition_model, feats, ali, transition_accs)


def gmm_acc_stats_ali_batch(am_gmm: AmDiagGmm, gmm_accs: AccumAmDiagGmm, transition_model: TransitionModel,
                            feats: Sequence[np.ndarray], alis: Sequence[Sequence[int]],
                            transition_accs: Optional[np.ndarray] = None):
    """Several utterances, same contract: -> (total log_like, transition_accs)."""
    tot = 0.0
    if transition_accs is None:
        transition_accs = transition_model.init_stats()
    for f, a in zip(feats, alis):
        ll, transition_accs = gmm_acc_stats_ali(am_gmm, gmm_accs, transition_model, f, a, transition_accs)
        tot += ll
    return tot, transition_accs


def gmm_acc_stats(am_gmm: AmDiagGmm, gmm_accs: AccumAmDiagGmm, transition_model: TransitionModel, feats, post,
                  transition_accs: Optional[np.ndarray] = None):
    """Kaldi's gmm-acc-stats for one utterance -> (log_like, transition_accs); gmm_accs is updated in place.
    `post` is a Posterior: per frame a list of (transition-id, weight).  Every entry adds what gmm_acc_stats_ali adds for a frame with
    that weight; the statistics stay on the device between calls, as gmm_acc_stats_ali's do."""
    feats = np.ascontiguousarray(feats, np.float32)
    _, entry_begin, tid, weight = posts_to_arrays([post])
    return gmm_accs._acc_stats_post(am_gmm, transition_model, feats, entry_begin, tid, weight, transition_accs)


def gmm_acc_stats_batch(am_gmm: AmDiagGmm, gmm_accs: AccumAmDiagGmm, transition_model: TransitionModel,
                        feats: Sequence[np.ndarray], posts: Sequence, transition_accs: Optional[np.ndarray] = None):
    """Several utterances, same contract: -> (total log_like, transition_accs)."""
    tot = 0.0
    if transition_accs is None:
        transition_accs = transition_model.init_stats()
    for f, p in zip(feats, posts):
        ll, transition_accs = gmm_acc_stats(am_gmm, gmm_accs, transition_model, f, p, transition_accs)
        tot += ll
    return tot, transition_accs


def gmm_est(am_gmm: AmDiagGmm, gmm_accs: AccumAmDiagGmm, transition_model: TransitionModel, transition_accs,
            tcfg: MleTransitionUpdateConfig, gmm_opts: MleDiagGmmOptions, mixup: int = 0, mixdown: int = 0,
            perturb_factor: float = 0.01, power: float = 0.2, min_count: float = 20.0, update_flags: str = "mvwt",
            verbose: bool = True, randn=None) -> Dict[str, float]:
    """scripts/gmm_est.py:8-96.  Returns the printed statistics as a dict as well."""
    flags = str_to_gmm_flags(update_flags)
    info = {}
    if int(flags) & int(GmmUpdateFlags.kGmmTransitions):
        objf_impr, count = transition_model.mle_update(transition_accs, tcfg)
        info["transition_objf_impr"], info["transition_count"] = objf_impr, count
        if verbose:
            print("Transition model update: Overall", objf_impr / count, "log-like improvement per frame over", count, "frames.")
    tot_like, tot_t = gmm_accs.tot_log_like, gmm_accs.tot_count
    objf_impr, count = mle_am_diag_gmm_update(config=gmm_opts, amdiag_gmm_acc=gmm_accs, flags=flags, am_gmm=am_gmm)
    info.update(gmm_objf_impr=objf_impr, gmm_count=count, avg_like=tot_like / tot_t if tot_t else float("nan"), frames=tot_t)
    if verbose:
        print("GMM update: Overall", objf_impr / count, "objective function improvement per frame over", count, "frames")
        print("GMM update: Overall avg like per frame =", tot_like / tot_t, "over", tot_t, "frames.")
    if mixup != 0 or mixdown != 0:
        pdf_occs = np.asarray([gmm_accs.get_acc(i).occupancy.sum() for i in range(gmm_accs.num_accs)], np.float32)
        if mixdown != 0:
            am_gmm.merge_by_count(state_occs=pdf_occs, target_components=mixdown, power=power, min_count=min_count)
        if mixup != 0:
            am_gmm.split_by_count(state_occs=pdf_occs, target_components=mixup, perturb_factor=perturb_factor,
                                  power=power, min_count=min_count, randn=randn)
    return info


def gmm_boost_silence(am_gmm: AmDiagGmm, transition_model: TransitionModel, silence_phones: List[int], boost: float = 1.5,
                      verbose: bool = False) -> AmDiagGmm:
    """scripts/gmm_boost_silence.py:10-45: a COPY of am_gmm with the weights of the silence phones' pdfs scaled by `boost`
    (gconsts recomputed); the argument is left untouched, as in the reference, whose recipe does
    `am = gmm_boost_silence(am_gmm=am, ...)` (egs/yesno/train.py:158).  silence_phones is sorted in place like there."""
    from .transition_model import get_pdfs_for_phones
    if len(silence_phones) == 0:
        raise KhgError("gmm_boost_silence: no silence phones")
    silence_phones.sort()
    is_unique, pdfs = get_pdfs_for_phones(transition_model, silence_phones)
    if not is_unique and verbose:
        print("The pdfs for the silence phones may be shared by other phones (note: this probably does not matter.)")
    dgm = AmDiagGmm()
    dgm.copy_from_am_diag_gmm(am_gmm)
    for pdf in pdfs:
        g = dgm.get_pdf(pdf)
        g.set_weights(g.weights * np.float32(boost))
        g.compute_gconsts()
    if verbose:
        print("Boosted weights for", len(pdfs), "pdfs, by factor of", boost)
    return dgm


def gmm_sum_accs(gmm_accs: Sequence[AccumAmDiagGmm], transition_accs: Optional[Sequence[np.ndarray]] = None):
    """Kaldi's gmm-sum-accs: the sum of several accumulators (AccumAmDiagGmm::Add with scale 1, csrc/mle-am-diag-gmm.cc:119-128) and
    of their transition statistics -> (gmm_accs[0], summed transition_accs or None); gmm_accs[0] is updated in place.  Blocks that
    live on the device are summed there with DeviceAccs.add."""
    if len(gmm_accs) == 0:
        raise KhgError("gmm_sum_accs: no accumulators")
    total = gmm_accs[0]
    for a in gmm_accs[1:]:
        total.add(1.0, a)
    tacc = None
    if transition_accs is not None and len(transition_accs) > 0:
        tacc = np.array(transition_accs[0], np.float64)
        for t in transition_accs[1:]:
            tacc = tacc + np.asarray(t, np.float64)
    return total, tacc


def gmm_ismooth_stats(gmm_accs: AccumAmDiagGmm, tau: float, src_accs: Optional[AccumAmDiagGmm] = None) -> AccumAmDiagGmm:
    """Kaldi's gmm-ismooth-stats: I-smoothing of `gmm_accs` (in place) with tau counts per Gaussian of the statistics in src_accs
    (AccumDiagGmm::SmoothWithAccum, csrc/mle-diag-gmm.cc:209-226); src_accs = None smooths the block with itself (--smooth-from-model
    is not offered).  On the device: DeviceAccs.smooth_with_accum."""
    src = gmm_accs if src_accs is None else src_accs
    if src.num_accs != gmm_accs.num_accs:
        raise KhgError("gmm_ismooth_stats: the two accumulators have different numbers of pdfs")
    for i in range(gmm_accs.num_accs):
        gmm_accs._accs[i].smooth_with_accum(tau, src.get_acc(i))
    return gmm_accs


def gmm_est_gmm_ebw(am_gmm: AmDiagGmm, num_accs: AccumAmDiagGmm, den_accs: AccumAmDiagGmm, ebw_opts: Optional[EbwOptions] = None,
                    update_flags: str = "mv", verbose: bool = True) -> Dict[str, float]:
    """Kaldi's gmm-est-gmm-ebw: the Extended Baum-Welch update of the means / variances from a numerator and a
    denominator accumulator; am_gmm is updated in place.  Returns the printed statistics as a dict as well."""
    flags = int(str_to_gmm_flags(update_flags)) & 0x3
    r = update_ebw_am_diag_gmm(num_accs, den_accs, flags, ebw_opts if ebw_opts is not None else EbwOptions(), am_gmm)
    if verbose:
        print("GMM update: Overall", r["auxf_impr_gauss"] / r["count"] if r["count"] else float("nan"),
              "auxiliary-function improvement per frame over", r["count"], "frames;", r["floored"], "Gaussians floored,", r["failed"], "failed,",
              r["skipped"], "skipped")
    return r


def gmm_est_weights_ebw(am_gmm: AmDiagGmm, num_accs: AccumAmDiagGmm, den_accs: AccumAmDiagGmm,
                        weight_opts: Optional[EbwWeightOptions] = None, verbose: bool = True) -> Dict[str, float]:
    """Kaldi's gmm-est-weights-ebw: the Extended Baum-Welch update of the mixture weights; am_gmm is updated in place."""
    r = update_ebw_weights_am_diag_gmm(num_accs, den_accs, weight_opts if weight_opts is not None else EbwWeightOptions(), am_gmm)
    if verbose:
        print("Weight update: Overall", r["auxf_impr_weights"] / r["count"] if r["count"] else float("nan"),
              "auxiliary-function improvement per frame over", r["count"], "frames;", r["weights_skipped"], "pdfs skipped")
    return r


def gmm_rescore_lattice_batch(am_gmm: AmDiagGmm, transition_model: TransitionModel, lattices, feats: Sequence[np.ndarray],
                              acoustic_scale: float = 1.0):
    """Kaldi's gmm-rescore-lattice for several utterances on the device (khg_lattices_rescore): every arc with a
    transition-id gets acoustic_cost = -(acoustic_scale * loglike(frame, pdf of the id)) under `am_gmm`; only the (frame, pdf) cells
    the lattices name are evaluated.  lattices: a list of Lattice (-> a list of Lattice; an utterance's status is not reported, an
    empty lattice stays empty) or a DeviceLattices on the default context (-> a DeviceLattices with .status and .rescore_stats)."""
    from .align import DeviceLattices
    ctx = _gpu.default_context()
    feats = [np.ascontiguousarray(f, np.float32) for f in feats]
    go, gc, _, miv, iv = am_gmm.flat()
    dm = DeviceModel(ctx, go, gc, miv, iv)
    dt = DeviceTransitions(ctx, np.asarray(transition_model.transition_id_to_pdf_array(), np.int32))
    fo = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
    allf = np.concatenate(feats) if feats else np.zeros((0, am_gmm.dim), np.float32)
    us = UtteranceSet(ctx, None, fo, np.ascontiguousarray(allf, np.float32))
    on_device = isinstance(lattices, DeviceLattices)
    dl = lattices if on_device else DeviceLattices.from_lattices(list(lattices), ctx)
    try:
        res = dl.rescore(us, dm, dt, float(acoustic_scale), "cells")
    finally:
        us.close(); dm.close(); dt.close()
        if not on_device:
            dl.close()
    if on_device:
        return res
    out = res.download()
    res.close()
    return out


def gmm_rescore_lattice(am_gmm: AmDiagGmm, transition_model: TransitionModel, lattice, feats, acoustic_scale: float = 1.0):
    """Kaldi's gmm-rescore-lattice for one utterance -> the rescored Lattice (gmm_rescore_lattice_batch of one)."""
    return gmm_rescore_lattice_batch(am_gmm, transition_model, [lattice], [feats], acoustic_scale)[0]


def lattice_boost_ali_batch(transition_model: TransitionModel, lattices, alignments: Sequence[Sequence[int]], silence_phones: Sequence[int],
                            b: float = 0.1, max_silence_error: float = 0.0):
    """Kaldi's lattice-boost-ali for several utterances on the device (khg_lattices_boost): every arc with a
    transition-id at frame t gets graph_cost += -b * e, e = 0 where its phone is the phone of alignments[u][t], max_silence_error
    where it differs and is a silence phone, 1 otherwise.  An utterance whose alignment is missing, of another length than its lattice
    or holds a bad id gets an empty lattice, as lattice-boost-ali skips it.  lattices: a list of Lattice (-> a list of Lattice) or a
    DeviceLattices on the default context (-> a DeviceLattices with .status)."""
    from .align import DeviceLattices
    on_device = isinstance(lattices, DeviceLattices)
    dl = lattices if on_device else DeviceLattices.from_lattices(list(lattices), _gpu.default_context())
    try:
        res = dl.boost(np.asarray(transition_model.transition_id_to_phone_array(), np.int32), np.asarray(list(silence_phones), np.int32),
                       alignment=[np.asarray(a, np.int32) for a in alignments], b=float(b), max_silence_error=float(max_silence_error))
    finally:
        if not on_device:
            dl.close()
    if on_device:
        return res
    out = res.download()
    res.close()
    return out


def lattice_boost_ali(transition_model: TransitionModel, lattice, alignment: Sequence[int], silence_phones: Sequence[int], b: float = 0.1,
                      max_silence_error: float = 0.0):
    """Kaldi's lattice-boost-ali for one utterance -> the boosted Lattice (lattice_boost_ali_batch of one)."""
    return lattice_boost_ali_batch(transition_model, [lattice], [alignment], silence_phones, b, max_silence_error)[0]


def lattice_lmrescore_batch(lm, lattices, scale: float = 1.0, hist_factor: int = 8):
    """Kaldi's lattice-lmrescore for several utterances on the device (khg_lattices_lm_rescore): every state is split by
    the histories of the backoff n-gram `lm` (an NgramLm) that reach it, every arc with a word gets graph_cost += scale * the LM's cost
    of the word; scale -1 takes an LM out again.  An utterance with a word the LM lacks (or whose history sets outgrow hist_factor
    entries per state) gets an empty lattice.  lattices: a list of Lattice (-> a list of Lattice) or a DeviceLattices on the default
    context (-> a DeviceLattices with .status)."""
    from .align import DeviceLattices, DeviceLm
    ctx = _gpu.default_context()
    on_device = isinstance(lattices, DeviceLattices)
    dl = lattices if on_device else DeviceLattices.from_lattices(list(lattices), ctx)
    dlm = DeviceLm(lm, ctx)
    try:
        res, _, _ = dl.lm_rescore(dlm, float(scale), int(hist_factor))
    finally:
        dlm.close()
        if not on_device:
            dl.close()
    if on_device:
        return res
    out = res.download()
    res.close()
    return out


def lattice_lmrescore(lm, lattice, scale: float = 1.0, hist_factor: int = 8):
    """Kaldi's lattice-lmrescore for one utterance -> the rescored Lattice (lattice_lmrescore_batch of one)."""
    return lattice_lmrescore_batch(lm, [lattice], scale, hist_factor)[0]


def _lattice_to_mpe_post_batch(criterion, transition_model, lattices, alignments, silence_phones, one_silence_class, acoustic_scale, lm_scale):
    from .align import DeviceLattices
    on_device = isinstance(lattices, DeviceLattices)
    dl = lattices if on_device else DeviceLattices.from_lattices(list(lattices), _gpu.default_context())
    try:
        res = dl.mpe_posteriors(np.asarray(transition_model.transition_id_to_phone_array(), np.int32), np.asarray(list(silence_phones), np.int32),
                                alignment=[np.asarray(a, np.int32) for a in alignments], criterion=criterion,
                                tid2pdf=np.asarray(transition_model.transition_id_to_pdf_array(), np.int32), one_silence_class=bool(one_silence_class),
                                graph_scale=float(lm_scale), acoustic_scale=float(acoustic_scale))
    finally:
        if not on_device:
            dl.close()
    if on_device:
        return res
    out = (res.download(), np.asarray(res.avg_acc, np.float64))
    res.close()
    return out


def lattice_to_mpe_post_batch(transition_model: TransitionModel, lattices, alignments: Sequence[Sequence[int]], silence_phones: Sequence[int],
                              one_silence_class: bool = True, acoustic_scale: float = 1.0, lm_scale: float = 1.0):
    """Kaldi's lattice-to-mpe-post for several utterances on the device (khg_lattices_mpe_posteriors with KHG_MPE_MPFE):
    the signed posteriors of the expected phone frame accuracy against alignments[u].  lattices: a list of Lattice (-> (a list of
    Posterior, the expected accuracy per utterance)) or a DeviceLattices on the default context (-> a DevicePosteriors with .avg_acc).
    An utterance whose alignment is missing, of another length than its lattice or holds a bad id has no frames (KHG_LAT_NO_REF)."""
    return _lattice_to_mpe_post_batch("mpfe", transition_model, lattices, alignments, silence_phones, one_silence_class, acoustic_scale, lm_scale)


def lattice_to_smbr_post_batch(transition_model: TransitionModel, lattices, alignments: Sequence[Sequence[int]], silence_phones: Sequence[int],
                               one_silence_class: bool = True, acoustic_scale: float = 1.0, lm_scale: float = 1.0):
    """Kaldi's lattice-to-smbr-post: lattice_to_mpe_post_batch with an arc counted correct when its pdf is the reference's (KHG_MPE_SMBR)."""
    return _lattice_to_mpe_post_batch("smbr", transition_model, lattices, alignments, silence_phones, one_silence_class, acoustic_scale, lm_scale)


def lattice_to_mpe_post(transition_model: TransitionModel, lattice, alignment: Sequence[int], silence_phones: Sequence[int],
                        one_silence_class: bool = True, acoustic_scale: float = 1.0, lm_scale: float = 1.0):
    """Kaldi's lattice-to-mpe-post for one utterance -> (Posterior, expected accuracy)."""
    posts, avg = lattice_to_mpe_post_batch(transition_model, [lattice], [alignment], silence_phones, one_silence_class, acoustic_scale, lm_scale)
    return posts[0], float(avg[0])


def lattice_to_smbr_post(transition_model: TransitionModel, lattice, alignment: Sequence[int], silence_phones: Sequence[int],
                         one_silence_class: bool = True, acoustic_scale: float = 1.0, lm_scale: float = 1.0):
    """Kaldi's lattice-to-smbr-post for one utterance -> (Posterior, expected accuracy)."""
    posts, avg = lattice_to_smbr_post_batch(transition_model, [lattice], [alignment], silence_phones, one_silence_class, acoustic_scale, lm_scale)
    return posts[0], float(avg[0])


def gmm_acc_stats2(am_gmm: AmDiagGmm, num_accs: AccumAmDiagGmm, den_accs: AccumAmDiagGmm, transition_model: TransitionModel, feats, post,
                   num_transition_accs: Optional[np.ndarray] = None, den_transition_accs: Optional[np.ndarray] = None):
    """Kaldi's gmm-acc-stats2 for one utterance -> (num_transition_accs, den_transition_accs); the two accumulators are updated in place.
    `post` is a signed Posterior (lattice_to_mpe_post / lattice_to_smbr_post): an entry with a positive weight adds to num_accs what
    gmm_acc_stats adds, one with a negative weight adds to den_accs with the weight negated (the rule of khg_acc_stats_post2, DESIGN.md
    7k, which UtteranceSet.acc_stats_post2 runs for posteriors resident on the device; this per-utterance form splits the Posterior on
    the host and makes gmm_acc_stats's call once per block)."""
    if num_accs is den_accs:
        raise KhgError("gmm_acc_stats2: num_accs and den_accs are the same accumulator")
    pos = [[(t, w) for t, w in f if w > 0] for f in post]
    neg = [[(t, -w) for t, w in f if w < 0] for f in post]
    _, num_transition_accs = gmm_acc_stats(am_gmm, num_accs, transition_model, feats, pos, num_transition_accs)
    _, den_transition_accs = gmm_acc_stats(am_gmm, den_accs, transition_model, feats, neg, den_transition_accs)
    return num_transition_accs, den_transition_accs


def gmm_acc_stats2_batch(am_gmm: AmDiagGmm, num_accs: AccumAmDiagGmm, den_accs: AccumAmDiagGmm, transition_model: TransitionModel,
                         feats: Sequence[np.ndarray], posts: Sequence, num_transition_accs: Optional[np.ndarray] = None,
                         den_transition_accs: Optional[np.ndarray] = None):
    """Several utterances, same contract."""
    for f, p in zip(feats, posts):
        num_transition_accs, den_transition_accs = gmm_acc_stats2(am_gmm, num_accs, den_accs, transition_model, f, p, num_transition_accs,
                                                                  den_transition_accs)
    return num_transition_accs, den_transition_accs
