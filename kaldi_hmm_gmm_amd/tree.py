"""Decision-tree building on the batched device path: Kaldi's acc-tree-stats, build-tree, gmm-init-model and convert-ali.

    stats = accumulate (count, x, x2) per (phone-context window, pdf-class) event from the resident alignment   (acc_tree_stats_batch)
    tree  = GetStubMap, best-first splitting, restricted clustering, renumbering -- on the host, in C++          (build_tree)
    model = one Gaussian per leaf from the statistics                                                           (gmm_init_model)
    ali   = the old alignment's phones, HMM states and arc choices on the new model                             (convert_ali)

The accumulation is the device part (csrc/khg_tree.hip); the tree building is csrc/khg_host_tree.cpp behind khg_build_tree."""
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from . import _kaldi_hmm_gmm_amd as _ext
from ._lib import KhgError
from .context_dep import ContextDependency, get_stub_map, kPdfClass
from .device import DeviceTreeStats, UtteranceSet
from .diag_gmm import AmDiagGmm, DiagGmm
from .hmm_topology import HmmTopology
from .transition_model import TransitionModel

TREE_MAX_CONTEXT = _ext.TREE_MAX_CONTEXT
TREE_MAX_PHONE = _ext.TREE_MAX_PHONE
TREE_MAX_PDF_CLASS = _ext.TREE_MAX_PDF_CLASS
TREE_STATUS_NO_ALI = _ext.TREE_STATUS_NO_ALI
TREE_STATUS_MIXED_PHONES = _ext.TREE_STATUS_MIXED_PHONES
TREE_STATUS_OPEN_END = _ext.TREE_STATUS_OPEN_END


def tid_tables(tm: TransitionModel):
    """-> (tid2phone, tid2pdf_class, tid_flags), each int32 [num_transition_ids + 1] with index 0 unused: what khg_acc_tree_stats reads.
    The pdf-class of a transition-id is its source state's forward_pdf_class, or self_loop_pdf_class for a self-loop."""
    n = tm.num_transition_ids
    phone, pdf_class, flags = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    entries: Dict[int, list] = {}
    for t in range(1, n + 1):
        ph = tm.transition_id_to_phone(t)
        if ph not in entries:
            entries[ph] = tm.topo.topology_for_phone(ph)
        st = entries[ph][tm.transition_id_to_hmm_state(t)]
        sl = tm.is_self_loop(t)
        phone[t] = ph
        pdf_class[t] = st.self_loop_pdf_class if sl else st.forward_pdf_class
        flags[t] = (_ext.TREE_TID_SELF_LOOP if sl else 0) | (_ext.TREE_TID_FINAL if tm.is_final(t) else 0)
    return phone, pdf_class, flags


def _utts_acc_tree_stats(self, ctx, tm: TransitionModel, stats: DeviceTreeStats, ci_phones: Iterable[int] = ()) -> np.ndarray:
    """UtteranceSet.acc_tree_stats: adds the set's events (resident alignment, resident feature rows) into `stats`.
    -> int32 status [n_utt]: 0, or the TREE_STATUS_* bits of an utterance that was skipped."""
    if stats.ctx is not ctx:
        raise KhgError("acc_tree_stats: the statistics belong to another context")
    phone, pdf_class, flags = tid_tables(tm)
    return self._acc_tree_stats(phone, pdf_class, flags, np.asarray(sorted(set(int(p) for p in ci_phones)), np.int32), stats)


UtteranceSet.acc_tree_stats = _utts_acc_tree_stats


def acc_tree_stats_batch(tm: TransitionModel, utts, N: int = 3, P: int = 1, ci_phones: Iterable[int] = (),
                         stats: Optional[DeviceTreeStats] = None) -> DeviceTreeStats:
    """acc-tree-stats for a set whose alignment is resident (UtteranceSet.align or upload_ali).  `stats`: a DeviceTreeStats to add into;
    None makes one.  The per-utterance status is left in stats.last_status."""
    if stats is None:
        stats = DeviceTreeStats(utts.ctx, utts.dim, N, P)
    stats.last_status = utts.acc_tree_stats(utts.ctx, tm, stats, ci_phones)
    return stats


def acc_tree_stats(tm: TransitionModel, utts, **kw) -> dict:
    """acc-tree-stats with the statistics brought to the host: -> {"keys" int32 [num_keys, N + 1] (window, pdf-class; ascending),
    "count", "x", "x2" (float64), "N", "P", "status", "stats"}."""
    stats = acc_tree_stats_batch(tm, utts, **kw)
    d = dict(stats.download())
    d.update(N=stats.N, P=stats.P, status=stats.last_status, stats=stats)
    return d


def _host_stats(stats) -> dict:
    if isinstance(stats, DeviceTreeStats):
        d = dict(stats.download())
        d.update(N=stats.N, P=stats.P)
        return d
    return stats


def pdf_class_questions(max_pdf_classes: int) -> List[List[int]]:
    """The default questions of key -1 (Kaldi's QuestionsForKey for kPdfClass): [[0], [0, 1], .., [0 .. n - 2]]."""
    return [list(range(i + 1)) for i in range(max(0, int(max_pdf_classes) - 1))]


def build_tree(stats, questions, phone_sets: Sequence[Sequence[int]], phone2num_pdf_classes: Sequence[int], share_roots: Sequence[bool],
               do_split: Sequence[bool], thresh: float = 300.0, max_leaves: int = 0, cluster_thresh: float = -1.0, N: int = 3, P: int = 1,
               var_floor: float = 0.01, return_info: bool = False):
    """build-tree: -> ContextDependency; its figures {"objf_impr", "cluster_loss", "num_leaves", "num_removed"} are left in
    tree.build_info (with return_info, (tree, that dict) is returned).
    `stats`: a DeviceTreeStats or the dict of acc_tree_stats (then N, P are the statistics').  `questions`: phone sets asked of every
    window position (a list), or {key: [sets]} with key -1 for the pdf-class; a list gets pdf_class_questions for key -1, as
    compile-questions does.  The rule is DESIGN.md 7o's; improvements stay double where Kaldi narrows Objf to float."""
    s = _host_stats(stats)
    N, P = int(s.get("N", N)), int(s.get("P", P))
    if not isinstance(questions, dict):
        qs = [sorted(set(int(v) for v in q)) for q in questions]
        questions = {k: qs for k in range(N)} if qs else {}
        pq = pdf_class_questions(max(phone2num_pdf_classes) if len(phone2num_pdf_classes) else 0)
        if pq:
            questions[kPdfClass] = pq
    qkeys, qkey_off, q_off, q_vals = [], [0], [0], []
    for k in sorted(questions):
        qkeys.append(int(k))
        for q in questions[k]:
            q_vals.extend(sorted(set(int(v) for v in q)))
            q_off.append(len(q_vals))
        qkey_off.append(len(q_off) - 1)
    set_off, set_phones = [0], []
    for ps in phone_sets:
        set_phones.extend(int(p) for p in ps)
        set_off.append(len(set_phones))
    keys = np.ascontiguousarray(s["keys"], np.int32).reshape(-1, N + 1)
    x = np.ascontiguousarray(s["x"], np.float64)
    x = x.reshape(keys.shape[0], -1) if x.size else x.reshape(0, max(1, x.shape[-1] if x.ndim == 2 else 1))
    r = _ext.build_tree(N, P, keys, np.ascontiguousarray(s["count"], np.float64).reshape(-1), x, np.ascontiguousarray(s["x2"], np.float64).reshape(x.shape),
                        np.asarray(qkeys, np.int32), np.asarray(qkey_off, np.int64), np.asarray(q_off, np.int64), np.asarray(q_vals, np.int32),
                        np.asarray(set_off, np.int64), np.asarray(set_phones, np.int32), np.asarray([1 if b else 0 for b in share_roots], np.int32),
                        np.asarray([1 if b else 0 for b in do_split], np.int32), np.asarray(list(phone2num_pdf_classes), np.int32), float(thresh),
                        int(max_leaves), float(cluster_thresh), float(var_floor))
    tree = ContextDependency.from_bytes(r["tree"], True)
    tree.build_info = {k: r[k] for k in ("objf_impr", "cluster_loss", "num_leaves", "num_removed")}
    tree.stub = {"phone_sets": [sorted(int(p) for p in ps) for ps in phone_sets], "share_roots": [bool(b) for b in share_roots]}   # gmm_init_model's empty-leaf rule
    if return_info:
        return tree, tree.build_info
    return tree


def leaf_stats(tree: ContextDependency, stats) -> dict:
    """The statistics summed per leaf through tree.to_pdf.map, keys in ascending order: -> {"count" [num_pdfs], "x", "x2" [num_pdfs, dim]}."""
    s = _host_stats(stats)
    keys = np.asarray(s["keys"]).reshape(-1, tree.context_width + 1)
    dim = np.asarray(s["x"]).shape[-1]
    out = {"count": np.zeros(tree.num_pdfs), "x": np.zeros((tree.num_pdfs, dim)), "x2": np.zeros((tree.num_pdfs, dim))}
    for i, row in enumerate(keys):
        ok, pdf = tree.compute([int(v) for v in row[:-1]], int(row[-1]))
        if not ok:
            raise KhgError("leaf_stats: the tree has no leaf for event %s" % (row.tolist(),))
        out["count"][pdf] += s["count"][i]
        out["x"][pdf] += s["x"][i]
        out["x2"][pdf] += s["x2"][i]
    return out


def _stub_roots(tree: ContextDependency, topo: HmmTopology, phone_sets, share_roots) -> Dict[int, List[int]]:
    """leaf -> the leaves of the stub root it was split from: the stub map of (phone_sets, share_roots) names the stub leaf of every
    (central phone, pdf-class), and a stub root is every leaf the tree gives the pairs of one stub leaf, in any context"""
    P = tree.central_position
    p2n = topo.get_phone_to_num_pdf_classes()
    stub = get_stub_map(P, [sorted(int(p) for p in ps) for ps in phone_sets], list(p2n), [bool(b) for b in share_roots], [0])
    by_stub: Dict[int, set] = {}
    for ph in topo.phones:
        for pc in range(p2n[ph]):
            sl = stub.map({P: ph, kPdfClass: pc})
            if sl is None:
                continue
            found: List[int] = []
            tree.to_pdf.multi_map({P: ph, kPdfClass: pc}, found)
            by_stub.setdefault(sl, set()).update(found)
    roots: Dict[int, List[int]] = {}
    for leaves in by_stub.values():
        for leaf in leaves:
            roots[leaf] = sorted(set(roots.get(leaf, [])) | leaves)
    return roots


def gmm_init_model(tree: ContextDependency, stats, topo: HmmTopology, var_floor: float = 0.01, phone_sets=None, share_roots=None):
    """gmm-init-model: one Gaussian per leaf -- weight 1, mean x / count, variance max(x2 / count - mean^2, var_floor) -- and the
    TransitionModel of (tree, topo).  A leaf whose count is below 1 (no statistics reached it) takes the sums over its stub root: the
    leaves that were split from the same leaf of the stub map.  The stub map is that of `phone_sets` / `share_roots`; a tree that
    build_tree returned remembers its own (tree.stub).  A tree without them (read from a file) is taken to have one shared root per
    phone: the leaf then takes the sums of every leaf the tree can give its central phones.  -> (AmDiagGmm, TransitionModel)."""
    ls = leaf_stats(tree, stats)
    P, n = tree.central_position, tree.num_pdfs
    if phone_sets is None and getattr(tree, "stub", None):
        phone_sets, share_roots = tree.stub["phone_sets"], tree.stub["share_roots"]
    if phone_sets is None:
        phone_sets, share_roots = [[p] for p in topo.phones], [True] * len(topo.phones)
    if len(share_roots) != len(phone_sets):
        raise KhgError("gmm_init_model: one share_roots entry per phone set")
    am = AmDiagGmm()
    roots = None
    for pdf in range(n):
        c, x, x2 = ls["count"][pdf], ls["x"][pdf], ls["x2"][pdf]
        if c < 1.0:
            if roots is None:
                roots = _stub_roots(tree, topo, phone_sets, share_roots)
            root = roots.get(pdf, [pdf])
            c, x, x2 = ls["count"][root].sum(), ls["x"][root].sum(0), ls["x2"][root].sum(0)
            if c < 1.0:
                raise KhgError("gmm_init_model: pdf %d and its whole stub root have no statistics" % pdf)
        mean = x / c
        var = np.maximum(x2 / c - mean * mean, var_floor)
        g = DiagGmm(nmix=1, dim=len(mean))
        g.set_weights(np.ones(1, np.float32))
        g.set_means(mean.astype(np.float32)[None, :])
        g.set_invvars((1.0 / var).astype(np.float32)[None, :])
        g.compute_gconsts()
        am.add_pdf(g)
    return am, TransitionModel(ctx_dep=tree, hmm_topo=topo)


def split_to_phones(tm: TransitionModel, ali: Sequence[int]) -> List[List[int]]:
    """SplitToPhones for reordered graphs: a segment ends after a final transition-id and the self-loops that follow it."""
    out, cur, closing = [], [], False
    for t in ali:
        t = int(t)
        if closing and not tm.is_self_loop(t):
            out.append(cur)
            cur, closing = [], False
        cur.append(t)
        if tm.is_final(t):
            closing = True
    if cur:
        out.append(cur)
    return out


def convert_ali(old_tm: TransitionModel, new_tm: TransitionModel, new_tree: ContextDependency, ali: Sequence[int]) -> np.ndarray:
    """convert-ali on the host: per phone segment the same phone, HMM states and self-loop / forward-arc choices; the pdfs from
    new_tree.compute(window, pdf-class) with the window of the segment's neighbours (0 outside the utterance)."""
    segs = split_to_phones(old_tm, ali)
    phones = [old_tm.transition_id_to_phone(s[0]) for s in segs]
    N, P = new_tree.context_width, new_tree.central_position
    out = np.zeros(len(ali), np.int32)
    k = 0
    for i, seg in enumerate(segs):
        window = [phones[i - P + j] if 0 <= i - P + j < len(segs) else 0 for j in range(N)]
        entry = new_tm.topo.topology_for_phone(phones[i])
        for t in seg:
            if old_tm.transition_id_to_phone(t) != phones[i]:
                raise KhgError("convert_ali: two phones inside one segment")
            hs = old_tm.transition_id_to_hmm_state(t)
            ts_old = old_tm.transition_id_to_transition_state(t)
            idx = t - old_tm.pair_to_transition_id(ts_old, 0)
            pdfs = []
            for pc in (entry[hs].forward_pdf_class, entry[hs].self_loop_pdf_class):
                ok, pdf = new_tree.compute(window, pc)
                if not ok:
                    raise KhgError("convert_ali: the tree has no leaf for window %s, pdf-class %d" % (window, pc))
                pdfs.append(pdf)
            ts_new = new_tm.tuple_to_transition_state(phones[i], hs, pdfs[0], pdfs[1])
            out[k] = new_tm.pair_to_transition_id(ts_new, idx)
            k += 1
    return out
