#!/usr/bin/env python3
"""Wall-clock time of a batched lattice decode (decode_lattice_faster_batch: K1 over every cell of the graphs' pdfs + the lattice
decoder kernel + transfers) beside the FasterDecoder batch (align_batch at FasterDecoderOptions(beam=13, max_active=7000)) on the
bench workload's model (tri5000x64: 5000 pdfs x 64 Gaussians, dim 40) and its linear training graphs, at decode.py's configuration
(max_active 7000, beam 13, lattice_beam 6, acoustic scale 0.1).  Prints one JSON line.

--decoder simple times decode_lattice_simple_batch (LatticeSimpleDecoderConfig(beam=13, lattice_beam=6)) instead, beside the faster
lattice decoder and the FasterDecoder batch on the same graphs.  All three then decode the graphs with a zero-weight input-epsilon
self-loop added on every state: no path's weight changes, and the simple decoder's ProcessNonemitting always has a token to queue
(the training graphs alone are epsilon-free, on which the reference stops at InitDecoding).

--check N (with --decoder simple) also decodes the first N utterances with their K1 scores returned and compares them, outside the
timing, with the plain-Python restatement of the reference (tests/lattice_simple_ref.py): succeeded, alignment, words, like.

--shared-graph --words W is the decoding case: ONE W-word unigram loop over the model's phones (each word a seeded random string
of 3-6 phones, expanded to transition-id arcs with self-loops the way synth.make_utts expands its transcripts, word ids on the
output side, an epsilon arc from a word's last state back to the loop state) and --utts utterances sampled from random word
sequences of that lexicon.  Both lattice decoders run on the resident scores of a set created on a shared DecodingGraph and, while
U copies of the tables stay under 8 GiB, of a set created from a list of U copies; the simple decoder (every state also carries
an epsilon self-loop) with its hub form off and at each threshold of --hub.  Paths and options alternate inside every
repetition.  The JSON line reports the graph, per path the set creation time, the graph bytes and the decode times (median, min,
max), and the share of utterances that succeeded.  --check N compares the first N with both restatements.  --yesno times the simple
decoder at the same thresholds on the 46-state word loop of examples/decode_synthetic.py instead.

--lattices (with --decoder simple, or with --shared-graph) also times the raw-lattice call beside the old one, alternated inside
every repetition: get_raw_lattice_simple_batch (UtteranceSet.raw_lattice_simple on the shared-graph sets).  It reports the states,
arcs and bytes per utterance, the download apart from the decode call (seconds, bytes, effective GB/s), and -- from one more pass of
each call under the context's kernel timing -- the device time of k2_lattice_simple and of the emission kernels (count, scans, fill).

With the default --decoder faster, --lattices times get_raw_lattice_faster_batch (the order-faithful decoder's own raw lattice, on the
graphs as they are) beside decode_lattice_faster_batch the same way: sizes, download, the decoder kernel's time in both calls (their
difference is what the emission adds inside the decoder's lane), the emission kernels, and a hash of the plain call's outputs.

--sweep LO:HI and --prune-beam B (next to --lattices) keep the batch's lattices on the device (get_raw_lattice_simple_device_batch,
UtteranceSet.raw_lattices_simple_device) and time, over max(--reps, 5) repetitions after a warm-up: the best path at every integer
language-model weight w in LO..HI (graph_scale 1, acoustic_scale 1 / w) in ONE DeviceLattices.best_path call, one pair alone, and
DeviceLattices.prune(B) at the middle weight -- beside what gives the same answers without them: the download of every lattice, the
Lattice objects and a host ShortestPath per weight and utterance.  Kernel milliseconds come from one more pass under the context's
kernel timing; the report says how many of the host's paths the device's equal.

--acc (next to --lattices --post) times khg_acc_stats_post on those posteriors -- flatten, bucket, accumulate, entries per frame --
beside khg_acc_stats under k3_form = 1, k3_phase_a = 1 (the same fp32 form) on the best-path alignment of the same set, and reports
the ratio per entry.

--post (next to --lattices) times DeviceLattices.posteriors(1, 0.1) on the resident lattices the same way, beside the download of every
lattice plus a host Lattice.forward_backward per utterance and beside the one-pair best path on the same handle; it reports the kernels
of the first call on the handle (which builds the in-arc index) and of a later one, the posterior handle's bytes, and how many of the
host's (transition-id, weight) entries the device's agree with to 1e-9.  (The lattice-simple decoder's lattices carry epsilon
self-loops and are refused with KHG_LAT_EPS_LOOP: use --decoder faster.)

--mpe [--criterion mpe|smbr] (next to --lattices) times DeviceLattices.mpe_posteriors(1, 0.1) alternated with posteriors(1, 0.1) on
the same handle, and khg_acc_stats_post2 alternated with khg_acc_stats_post on the signed posteriors.

--lmrescore [ORDER] (next to --lattices) times DeviceLattices.lm_rescore on the resident lattices with a backoff n-gram of that order
(default 2) estimated from the decoded word sequences: mark / scan / fill device times, the call beside a fresh decode, the growth in
states and arcs and the largest history set.  The linear training graphs carry no words (every state keeps one history);
with --shared-graph the lattices come from the --words word loop, whose words the n-gram covers.

--nbest N (next to --shared-graph --lattices) times DeviceLattices.nbest(N) on the resident lattices, determinized first:
the call with everything downloaded beside the download of the lattices and a loop of the host form Lattice.nbest, and counts the
utterances whose entries equal the host's bit for bit.
--oracle and --score LO:HI (next to --lattices) time scoring on the resident lattices: DeviceLattices.oracle beside the
download plus a loop of the host form Lattice.oracle; DeviceLattices.wer at the LM weights LO..HI x penalties {0, 0.5, 1} beside
add_penalty + best_path with the words downloaded + khg_edit_distance on the host; add_penalty beside a device-to-device copy of the
same bytes.  The references are the words that were said (--shared-graph: the word loop's; the linear training graphs carry none), the
report gives the table bytes per utterance, the lane occupancy (R + 1 over 64) and the states per frame, and with --shared-graph the
same again on a denser set decoded at --dense-lattice-beam.

Usage: python tools/decode_lattice_bench.py [--utts 100000] [--reps 2] [--decoder faster|simple] [--check N] [--lattices] [--sweep 7:17] [--prune-beam 4] [--post] [--acc] [--mpe] [--lmrescore [ORDER]] [--oracle] [--score 7:17]
       python tools/decode_lattice_bench.py --shared-graph --words 1000 --utts 2000 [--reps 3] [--hub 0,32] [--check N] [--yesno]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import synth  # noqa: E402


def with_eps_self_loops(graphs, u):
    """Utterance u of a CSR graph set with a 0:0/0 self-loop after the arcs of every state."""
    so = graphs["state_off"]
    s0, s1 = int(so[u]), int(so[u + 1])
    ao = graphs["arc_off"]
    il, ol, w, ns, off = [], [], [], [], [0]
    for s in range(s0, s1):
        a0, a1 = int(ao[s]), int(ao[s + 1])
        il += list(graphs["ilabel"][a0:a1]) + [0]
        ol += list(graphs["olabel"][a0:a1]) + [0]
        w += list(graphs["weight"][a0:a1]) + [0.0]
        ns += list(graphs["nextstate"][a0:a1]) + [s - s0]
        off.append(len(il))
    return khg.StdVectorFst.from_csr(int(graphs["start"][u]), np.asarray(off, np.int64), np.asarray(il, np.int32), np.asarray(ol, np.int32),
                                     np.asarray(w, np.float32), np.asarray(ns, np.int32), np.asarray(graphs["final"][s0:s1], np.float32))


def word_loop(m, W, seed, eps_self_loops, loops=1):
    """-> (graph dict, lexicon): state 0 is the loop state (start, final); word w enters its chain on the forward transition-id of
    its first HMM state, carrying the word id w + 1, every chain state has its self-loop, the last one an epsilon arc back to 0.
    loops = K > 1: K copies of the loop state (states 0 .. K - 1, all final, each with an arc into every word), word w returning to
    copy w mod K -- the in-degree W divided among the copies, as with compile_word_loop_graph's loop state per final transition-state."""
    rng = np.random.default_rng(seed)
    nphones = m.num_pdfs // 3
    lex = [rng.integers(0, nphones, size=int(rng.integers(3, 7))) for _ in range(W)]
    pdfs = [(3 * np.repeat(ph, 3) + np.tile(np.arange(3), len(ph))).astype(np.int64) for ph in lex]
    il, ol, w, ns, off = [], [], [], [], [0]
    first, nxt = [], loops
    for p in pdfs:
        first.append(nxt)
        nxt += len(p)
    cost = float(np.log(W))
    for c in range(loops):
        for k, p in enumerate(pdfs):                       # a loop state: one arc per word
            il.append(2 * int(p[0]) + 2); ol.append(k + 1); w.append(cost); ns.append(first[k])
        if eps_self_loops:
            il.append(0); ol.append(0); w.append(0.0); ns.append(c)
        off.append(len(il))
    for k, p in enumerate(pdfs):
        for i in range(len(p)):                            # chain state i + 1 of the word: [forward (or the way back), self-loop]
            s = first[k] + i
            if i + 1 < len(p):
                il.append(2 * int(p[i + 1]) + 2); ol.append(0); w.append(0.0); ns.append(s + 1)
            else:
                il.append(0); ol.append(0); w.append(0.0); ns.append(k % loops)
            il.append(2 * int(p[i]) + 1); ol.append(0); w.append(0.0); ns.append(s)
            if eps_self_loops:
                il.append(0); ol.append(0); w.append(0.0); ns.append(s)
            off.append(len(il))
    final = np.full(nxt, np.inf, np.float32)
    final[:loops] = 0.0
    g = {"start": 0, "arc_off": np.asarray(off, np.int64), "ilabel": np.asarray(il, np.int32), "olabel": np.asarray(ol, np.int32),
         "weight": np.asarray(w, np.float32), "nextstate": np.asarray(ns, np.int32), "final": final}
    return g, pdfs


def tiled(g, U):
    """U copies of one graph dict in the CSR layout UtteranceSet(graphs=) takes."""
    S, A = len(g["final"]), len(g["ilabel"])
    out = {k: np.tile(g[k], U) for k in ("ilabel", "olabel", "weight", "nextstate", "final")}
    out["arc_off"] = np.concatenate([[0], (g["arc_off"][1:][None, :] + A * np.arange(U, dtype=np.int64)[:, None]).ravel()]).astype(np.int64)
    out["state_off"] = (S * np.arange(U + 1)).astype(np.int64)
    out["start"] = np.full(U, g["start"], np.int32)
    return out


def fst_of(g):
    return khg.StdVectorFst.from_csr(int(g["start"]), g["arc_off"], g["ilabel"], g["olabel"], g["weight"], g["nextstate"], g["final"])


def med(xs):
    return {"median_s": float(np.median(xs)), "min_s": float(min(xs)), "max_s": float(max(xs))}


def kernel_ms(ctx, call):
    """One run of `call` under the context's kernel timing -> {kernel name: milliseconds, summed over its launches}."""
    ctx.sync()
    ctx.timings()
    ctx.set_timing(True)
    try:
        call()
        out = {}
        for name, ms in ctx.timings():
            out[name] = out.get(name, 0.0) + float(ms)
    finally:
        ctx.set_timing(False)
    return out


def lattice_sizes(state_counts, arc_counts, download_s):
    """Per-utterance sizes of a batch's raw lattices (24 bytes a state, 20 an arc) and the download's rate."""
    st, ar = np.asarray(state_counts, np.int64), np.asarray(arc_counts, np.int64)
    nbytes = int(24 * st.sum() + 20 * ar.sum())
    return {"states_per_utt": {"mean": float(st.mean()), "max": int(st.max())}, "arcs_per_utt": {"mean": float(ar.mean()), "max": int(ar.max())},
            "bytes_per_utt": nbytes / max(len(st), 1), "download_bytes": nbytes, "download": med(download_s),
            "download_GB_per_s": nbytes / float(np.median(download_s)) / 1e9, "empty_lattices": int((st == 0).sum())}


def emission_summary(k_old, k_new):
    """Kernel milliseconds of the old call and of the raw-lattice call -> the decoder's and the emission's device time."""
    emit = sum(v for k, v in k_new.items() if k.startswith("k2_lattice_raw"))
    return {"old_call_kernels_ms": k_old, "raw_call_kernels_ms": k_new, "k2_lattice_simple_ms": k_old.get("k2_lattice_simple"),
            "emission_ms": emit, "emission_over_decoder": emit / k_old["k2_lattice_simple"] if k_old.get("k2_lattice_simple") else None}


def lattice_ops(ctx, dl, sweep, prune_beam, reps, post=False):
    """The operations on a DeviceLattices handle beside the host loop that gives the same answers -> the report dict."""
    reps = max(reps, 5)
    out = {"repetitions": reps, "device_bytes": int(dl.device_bytes), "utterances": int(dl.num_utts)}
    U = dl.num_utts
    if sweep:
        lo, hi = (int(x) for x in sweep.split(":"))
        ws = np.arange(lo, hi + 1)
        gs, as_ = np.ones(len(ws), np.float32), (1.0 / ws).astype(np.float32)
        dl.best_path(gs, as_); dl.best_path(gs[:1], as_[:1])                       # warm-up
        t_sweep, t_one, t_host, t_dl = [], [], [], []
        for _ in range(reps):
            ctx.sync(); t0 = time.time()
            many = dl.best_path(gs, as_)
            t_sweep.append(time.time() - t0)
            t0 = time.time()
            dl.best_path(gs[len(ws) // 2: len(ws) // 2 + 1], as_[len(ws) // 2: len(ws) // 2 + 1])
            t_one.append(time.time() - t0)
            t0 = time.time()
            lats = dl.download()                                                    # the download and the Lattice objects
            t_dl.append(time.time() - t0)
            host = [[L.best_path(1.0, float(a)) for L in lats] for a in as_]
            t_host.append(time.time() - t0)
        same = 0
        ao, wo = many["ali_off"], many["words_off"]
        for k in range(len(ws)):
            for u in range(U):
                o = k * U + u
                h = host[k][u]
                ok = h["status"] == int(many["status"][o]) and h["words"] == many["words"][wo[o]: wo[o + 1]].tolist() \
                    and np.asarray(h["weight"], np.float32).tobytes() == many["weight"][o].tobytes()
                same += bool(ok and (h["status"] != 1 or h["ali"] == many["ali"][k, ao[u]: ao[u + 1]].tolist()))
        k_sweep = kernel_ms(ctx, lambda: dl.best_path(gs, as_))
        k_one = kernel_ms(ctx, lambda: dl.best_path(gs[:1], as_[:1]))
        paths = [tuple(many["ali"][k].tolist()) for k in range(len(ws))]
        out["sweep"] = {"weights": [int(w) for w in ws], "best_path_call": med(t_sweep), "one_pair_call": med(t_one),
                        "host_download_and_lattices": med(t_dl), "host_download_lattices_and_shortest_paths": med(t_host),
                        "host_over_device": float(np.median(t_host) / np.median(t_sweep)), "kernels_ms": k_sweep, "one_pair_kernels_ms": k_one,
                        "entries": len(ws) * U, "entries_equal_to_host": same, "distinct_alignment_rows": len(set(paths)),
                        "succeeded": int((many["status"] == 1).sum())}
    if prune_beam is not None:
        a = float(np.float32(1.0 / ((lo + hi) // 2))) if sweep else 0.1
        dl.prune(prune_beam, 1.0, a).close()
        t_p = []
        for _ in range(reps):
            ctx.sync(); t0 = time.time()
            P = dl.prune(prune_beam, 1.0, a)
            t_p.append(time.time() - t0)
            kept = (int(P.state_off[-1]), int(P.arc_off[-1]))
            P.close()
        k_p = kernel_ms(ctx, lambda: dl.prune(prune_beam, 1.0, a).close())
        out["prune"] = {"beam": prune_beam, "acoustic_scale": a, "prune_call": med(t_p), "kernels_ms": k_p, "kernels_total_ms": sum(k_p.values()),
                        "states_before": int(dl.state_off[-1]), "arcs_before": int(dl.arc_off[-1]), "states_after": kept[0], "arcs_after": kept[1]}
    if post:
        a = 0.1
        k_first = kernel_ms(ctx, lambda: dl.posteriors(1.0, a).close())             # the first call on the handle builds its in-arc index
        t_post, t_host, t_dl, t_bp = [], [], [], []
        P = None
        for _ in range(reps):
            if P is not None:
                P.close()
            ctx.sync(); t0 = time.time()
            P = dl.posteriors(1.0, a)
            t_post.append(time.time() - t0)
            t0 = time.time()
            dl.best_path([1.0], [a])
            t_bp.append(time.time() - t0)
            t0 = time.time()
            lats = dl.download()
            t_dl.append(time.time() - t0)
            host = [L.forward_backward(1.0, a) for L in lats]
            t_host.append(time.time() - t0)
        got, st, tl = P.download(), P.status, P.tot_like
        entries = same = same_status = 0
        worst_tot = 0.0
        for u, h in enumerate(host):
            same_status += h["status"] == int(st[u])
            if h["status"] == 1:
                worst_tot = max(worst_tot, abs(h["tot_like"] - float(tl[u])))
            for hr, gr in zip(h["post"], got[u]):
                entries += len(hr)
                same += sum(1 for (t1, w1), (t2, w2) in zip(hr, gr) if t1 == t2 and abs(w1 - w2) <= 1e-9) if len(hr) == len(gr) else 0
        k_post = kernel_ms(ctx, lambda: dl.posteriors(1.0, a).close())
        k_bp = kernel_ms(ctx, lambda: dl.best_path([1.0], [a]))
        out["posteriors"] = {"acoustic_scale": a, "posteriors_call": med(t_post), "one_pair_best_path_call": med(t_bp),
                             "host_download_and_lattices": med(t_dl), "host_download_lattices_and_forward_backward": med(t_host),
                             "host_over_device": float(np.median(t_host) / np.median(t_post)), "kernels_ms": k_post,
                             "first_call_kernels_ms": k_first, "in_arc_index_ms": k_first.get("k2_lattice_post_index"),
                             "one_pair_best_path_kernels_ms": k_bp, "handle_bytes": int(P.device_bytes),
                             "handle_bytes_per_utt": int(P.device_bytes) / max(U, 1), "frames": int(P.frame_off[-1]), "entries": entries,
                             "entries_equal_to_host_within_1e-9": same, "statuses_equal_to_host": same_status, "succeeded": int((st == 1).sum()),
                             "largest_tot_like_difference": worst_tot}
        P.close()
    return out


def mpe_bench(ctx, dl, am, tm, feats, alignments, criterion, reps):
    """--mpe: DeviceLattices.mpe_posteriors(1, 0.1) (the best-path alignments as the reference) alternated in this process with
    posteriors(1, 0.1) on the same handle, and acc_stats_post2 of the signed posteriors alternated with acc_stats_post of the same
    handle -> medians of the kernel times and the two ratios."""
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    reps = max(reps, 5)
    tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
    tid2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    sil = np.asarray([int(tid2phone[1])], np.int32)
    alis = [np.asarray(a, np.int32) for a in alignments]
    crit = "mpfe" if criterion == "mpe" else "smbr"
    call = lambda: dl.mpe_posteriors(tid2phone, sil, alignment=alis, criterion=crit, tid2pdf=tid2pdf, acoustic_scale=0.1)  # noqa: E731
    dl.posteriors(1.0, 0.1).close()                                       # builds the in-arc index
    call().close()
    k_fb, k_mpe = [], []
    for _ in range(reps):
        k_fb.append(kernel_ms(ctx, lambda: dl.posteriors(1.0, 0.1).close()))
        k_mpe.append(kernel_ms(ctx, lambda: call().close()))
    medians = lambda rows: {k: float(np.median([r.get(k, 0.0) for r in rows])) for k in sorted({k for r in rows for k in r})}  # noqa: E731
    fb_ms, mpe_ms = medians(k_fb), medians(k_mpe)
    go, gc, w, miv, iv = am.flat()
    dm, dt = DeviceModel(ctx, go, gc, miv, iv), DeviceTransitions(ctx, tid2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    one, num, den = DeviceAccs(ctx, dm, dt), DeviceAccs(ctx, dm, dt), DeviceAccs(ctx, dm, dt)
    P = call()
    ok = (np.asarray(P.status) & 1) != 0
    us.acc_stats_post(dm, dt, P, one); us.acc_stats_post2(dm, dt, P, num, den); ctx.sync()          # warm-up (allocates the scratch)
    k_one, k_two = [], []
    for _ in range(reps):
        k_one.append(kernel_ms(ctx, lambda: us.acc_stats_post(dm, dt, P, one)))
        k_two.append(kernel_ms(ctx, lambda: us.acc_stats_post2(dm, dt, P, num, den)))
    one_ms, two_ms = medians(k_one), medians(k_two)
    out = {"criterion": crit, "repetitions": reps, "succeeded": int(ok.sum()), "frames": int(P.frame_off[-1]), "entries": int(P.entry_off[-1]),
           "mean_avg_acc_per_frame": float(np.mean(np.asarray(P.avg_acc)[ok] / np.diff(np.asarray(P.frame_off))[ok])) if ok.any() else None,
           "posteriors_kernels_ms": fb_ms, "mpe_posteriors_kernels_ms": mpe_ms,
           "k2_lattice_post_fb_ms": fb_ms.get("k2_lattice_post_fb"), "k2_lattice_post_mpe_ms": mpe_ms.get("k2_lattice_post_mpe"),
           "mpe_over_fb": mpe_ms.get("k2_lattice_post_mpe", 0.0) / fb_ms["k2_lattice_post_fb"] if fb_ms.get("k2_lattice_post_fb") else None,
           "acc_stats_post_kernels_ms": one_ms, "acc_stats_post2_kernels_ms": two_ms,
           "acc_stats_post_total_ms": sum(one_ms.values()), "acc_stats_post2_total_ms": sum(two_ms.values()),
           "post2_over_post": sum(two_ms.values()) / sum(one_ms.values()) if sum(one_ms.values()) else None}
    for h in (P, us, one, num, den, dm, dt):
        h.close()
    return out


def acc_from_post(ctx, dl, am, tm, feats, alignments, reps):
    """--acc: khg_acc_stats_post on the posteriors (1, 0.1) of the resident lattices -- device time of flatten, bucket and accumulate --
    beside khg_acc_stats under k3_form = 1, k3_phase_a = 1 (the same fp32 / fp64 MFMA form, one entry per frame) on the best-path
    alignment of the same set, in the same process -> the report dict with the ratio per entry."""
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    reps = max(reps, 5)
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    dm, dt = DeviceModel(ctx, go, gc, miv, iv), DeviceTransitions(ctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    accs = DeviceAccs(ctx, dm, dt)
    P = dl.posteriors(1.0, 0.1)
    ok = (np.asarray(P.status) & 1) != 0
    pfo = np.asarray(P.frame_off)
    frames, entries = int(pfo[-1]), int(P.entry_off[-1])
    eb, tid, _ = P.download_arrays()
    fr = np.repeat(np.arange(frames, dtype=np.int64), np.diff(np.asarray(eb)))
    merged = entries - len(np.unique(fr * (int(id2pdf.max()) + 1) + id2pdf[np.asarray(tid)]))
    us.acc_stats_post(dm, dt, P, accs); ctx.sync()                       # warm-up (allocates the scratch)
    k_post = [kernel_ms(ctx, lambda: us.acc_stats_post(dm, dt, P, accs)) for _ in range(reps)]
    t_post = []
    for _ in range(reps):
        ctx.sync(); t0 = time.time()
        us.acc_stats_post(dm, dt, P, accs); ctx.sync()
        t_post.append(time.time() - t0)
    # the best-path alignment of the utterances with posteriors (0 = no statistics for a frame of the others)
    ali = np.zeros(int(fo[-1]), np.int32)
    for u, a in enumerate(alignments):
        if ok[u] and len(a) == fo[u + 1] - fo[u]:
            ali[fo[u]: fo[u + 1]] = a
    us.upload_ali(ali)
    # (k3_form = 1 alone lets an alignment pass take the fp16 form k3_accumulate_block16; k3_phase_a = 1 keeps the fp32 / fp64 MFMA form)
    old, old_a = ctx.set_option("k3_form", 1), ctx.set_option("k3_phase_a", 1)
    try:
        us.acc_stats(dm, dt, accs); ctx.sync()
        k_ali = [kernel_ms(ctx, lambda: us.acc_stats(dm, dt, accs)) for _ in range(reps)]
    finally:
        ctx.set_option("k3_form", old); ctx.set_option("k3_phase_a", old_a)
    names = sorted({k for r in k_post for k in r})
    post_ms = {k: float(np.median([r.get(k, 0.0) for r in k_post])) for k in names}
    ali_ms = {k: float(np.median([r.get(k, 0.0) for r in k_ali])) for k in sorted({k for r in k_ali for k in r})}
    n_ali = int((ali > 0).sum())
    tot_post, tot_ali = sum(post_ms.values()), sum(ali_ms.values())
    out = {"repetitions": reps, "frames": frames, "entries": entries, "entries_per_frame": entries / max(frames, 1),
           "entries_post_to_pdf_post_would_merge": int(merged), "share_merged": merged / max(entries, 1),
           "acc_stats_post_kernels_ms": post_ms, "acc_stats_post_total_ms": tot_post, "acc_stats_post_call": med(t_post),
           "acc_stats_fp32_form_kernels_ms": ali_ms, "acc_stats_fp32_form_total_ms": tot_ali, "aligned_frames": n_ali,
           "ns_per_entry_post": 1e6 * tot_post / max(entries, 1), "ns_per_frame_ali": 1e6 * tot_ali / max(n_ali, 1),
           "ratio_per_entry": (tot_post / max(entries, 1)) / (tot_ali / max(n_ali, 1)) if tot_ali and n_ali else None}
    P.close(); us.close(); accs.close(); dm.close(); dt.close()
    return out


def rescore_bench(ctx, dl, am, tm, fsts, feats, alignments, cfg, reps, boost):
    """--rescore: khg_lattices_rescore (CELLS) on the resident lattices -- device time of flatten / sort / heads / score / scatter, the
    call from the host, arcs / emitting arcs / distinct cells per frame -- and one MMI iteration's denominator side both ways, alternated
    in this process: rescore + posteriors(1, 0.1) + acc_stats_post against loglikes + raw_lattices_faster_device + posteriors(1, 1) +
    acc_stats_post.  Memory: the device bytes of a decoding set's dense score buffer (khg_loglikes_layout), which the rescoring path
    never allocates.  --boost B: the call of khg_lattices_boost with the best paths as the reference."""
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    reps = max(reps, 3)
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    dm, dt = DeviceModel(ctx, go, gc, miv, iv), DeviceTransitions(ctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    allf = np.ascontiguousarray(np.concatenate(feats), np.float32)
    us = UtteranceSet(ctx, None, fo, allf)                               # features only: no graph, no score buffer
    accs = DeviceAccs(ctx, dm, dt)
    frames = int(fo[-1])
    dl.rescore(us, dm, dt, 1.0).close(); ctx.sync()                      # warm-up (allocates the scratch)
    k_res, t_res, stats = [], [], None
    for _ in range(reps):
        k_res.append(kernel_ms(ctx, lambda: dl.rescore(us, dm, dt, 1.0).close()))
        ctx.sync(); t0 = time.time()
        R = dl.rescore(us, dm, dt, 1.0)
        t_res.append(time.time() - t0)
        stats = R.rescore_stats
        R.close()
    res_ms = {k: float(np.median([r.get(k, 0.0) for r in k_res])) for k in sorted({k for r in k_res for k in r})}
    out = {"repetitions": reps, "frames": frames, "arcs": stats["arcs"], "emitting_arcs": stats["emitting_arcs"], "cells": stats["cells"],
           "arcs_per_frame": stats["arcs"] / max(frames, 1), "emitting_arcs_per_frame": stats["emitting_arcs"] / max(frames, 1),
           "cells_per_frame": stats["cells"] / max(frames, 1), "rescore_kernels_ms": res_ms, "rescore_kernels_total_ms": sum(res_ms.values()),
           "rescore_call": med(t_res)}
    if boost:
        tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
        ali = [np.asarray(a, np.int32) for a in alignments]
        t_b = []
        for _ in range(reps):
            ctx.sync(); t0 = time.time()
            B = dl.boost(tid2phone, np.asarray([1], np.int32), alignment=ali, b=boost)
            t_b.append(time.time() - t0)
            nref = int((np.asarray(B.status) & 512 != 0).sum())
            B.close()
        out.update(boost_call=med(t_b), boost_b=boost, boost_no_ref=nref,
                   boost_kernels_ms=kernel_ms(ctx, lambda: dl.boost(tid2phone, np.asarray([1], np.int32), alignment=ali, b=boost).close()))
    # one iteration's denominator side, both ways, alternated
    from kaldi_hmm_gmm_amd.fst import concat_graphs
    usg = UtteranceSet(ctx, dt, fo, allf, graphs=concat_graphs(fsts))
    dec = dict(beam=cfg.beam, max_active=cfg.max_active, lattice_beam=cfg.lattice_beam, acoustic_scale=0.1)

    def iter_rescore():
        R = dl.rescore(us, dm, dt, 1.0)
        P = R.posteriors(1.0, 0.1)
        us.acc_stats_post(dm, dt, P, accs); ctx.sync()
        P.close(); R.close()

    def iter_decode():
        usg.loglikes(dm)
        L = usg.raw_lattices_faster_device(dt, **dec)["lattices"]
        P = L.posteriors(1.0, 1.0)
        usg.acc_stats_post(dm, dt, P, accs); ctx.sync()
        P.close(); L.close()

    iter_rescore(); iter_decode()
    t_r, t_d = [], []
    for _ in range(reps):
        ctx.sync(); t0 = time.time(); iter_rescore(); t_r.append(time.time() - t0)
        ctx.sync(); t0 = time.time(); iter_decode(); t_d.append(time.time() - t0)
    ll_off, ll_total = usg.loglikes_layout()
    out.update(iteration_rescore_post_acc=med(t_r), iteration_decode_post_acc=med(t_d), iteration_ratio=float(np.median(t_d) / np.median(t_r)),
               iteration_rescore_kernels_ms=kernel_ms(ctx, iter_rescore), iteration_decode_kernels_ms=kernel_ms(ctx, iter_decode),
               dense_score_buffer_bytes=int(4 * ll_total), features_bytes=int(allf.nbytes))
    usg.close(); us.close(); accs.close(); dm.close(); dt.close()
    return out


def lmrescore_bench(ctx, dl, transcripts, vocab, order, reps, decode_call_s):
    """--lmrescore [ORDER]: khg_lattices_lm_rescore on the resident lattices with a backoff n-gram estimated from the decoded word
    sequences over the graphs' vocabulary -- device time of mark / scan / fill, the call from the host beside a fresh decode of the same
    set, the growth in states and arcs and the largest history set."""
    reps = max(reps, 3)
    lm = khg.estimate_ngram_lm(transcripts, order, vocab, 0.5)
    dlm = khg.DeviceLm(lm, ctx)
    dl.lm_rescore(dlm, 1.0)[0].close(); ctx.sync()                       # warm-up (builds the in-arc index once)
    k_ms, t_call, stats, st = [], [], None, None
    for _ in range(reps):
        k_ms.append(kernel_ms(ctx, lambda: dl.lm_rescore(dlm, 1.0)[0].close()))
        ctx.sync(); t0 = time.time()
        R, st, stats = dl.lm_rescore(dlm, 1.0)
        t_call.append(time.time() - t0)
        R.close()
    ms = {k: float(np.median([r.get(k, 0.0) for r in k_ms])) for k in sorted({k for r in k_ms for k in r})}
    out = {"order": order, "lm_states": lm.num_states, "lm_arcs": lm.num_arcs, "lm_device_bytes": dlm.device_bytes, "repetitions": reps,
           "kernels_ms": ms, "kernels_total_ms": sum(ms.values()), "call": med(t_call), "decode_call": decode_call_s,
           "call_over_decode": float(np.median(t_call)) / decode_call_s["median_s"] if decode_call_s else None,
           "succeeded": int((np.asarray(st) & 1 != 0).sum()), "oov": int((np.asarray(st) & 1024 != 0).sum()),
           "scratch": int((np.asarray(st) & 4 != 0).sum()),
           "state_growth": stats["out_states"] / max(stats["in_states"], 1), "arc_growth": stats["out_arcs"] / max(stats["in_arcs"], 1)}
    out.update(stats)
    dlm.close()
    return out


def score_bench(ctx, dl, refs, score, oracle, reps):
    """--oracle / --score LO:HI on resident lattices, both sides in this process and alternated.  --oracle:
    DeviceLattices.oracle beside the download of every lattice and a loop of the host form Lattice.oracle.  --score: DeviceLattices.wer at
    the LM weights LO..HI x penalties {0, 0.5, 1} beside the same points formed the old way -- add_penalty, best_path, the words
    downloaded, khg_edit_distance on the host -- and add_penalty beside a device-to-device copy of the handle's bytes."""
    import ctypes as C
    from kaldi_hmm_gmm_amd import _lib
    reps = max(reps, 3)
    U = dl.num_utts
    refs = [np.asarray(r, np.int32) for r in refs]
    so, ao = np.asarray(dl.state_off), np.asarray(dl.arc_off)
    N, R = np.diff(so), np.asarray([len(r) for r in refs])
    out = {"utterances": U, "states_mean": float(N.mean()), "arcs_mean": float(np.diff(ao).mean()), "ref_words_mean": float(R.mean()), "repetitions": reps,
           "table_bytes_per_utt_mean": float((8 * N * (R + 1)).mean()), "table_bytes_per_utt_max": int((8 * N * (R + 1)).max()),
           "lane_occupancy_mean": float(((R + 1) / (64.0 * np.ceil((R + 1) / 64.0))).mean())}
    if oracle:
        r = dl.oracle(refs); ctx.sync()                                  # warm-up (builds the in-arc index once)
        frames = np.maximum(np.diff(r["ali_off"]), 0) + 1
        out["states_per_frame_mean"] = float((N / frames).mean())
        t_dev, t_dl, t_host, k_ms, same = [], [], [], [], 0
        for _ in range(reps):
            k_ms.append(kernel_ms(ctx, lambda: dl.oracle(refs)))
            ctx.sync(); t0 = time.time()
            r = dl.oracle(refs)
            t_dev.append(time.time() - t0)
            t0 = time.time()
            lats = dl.download()
            t_dl.append(time.time() - t0)
            t0 = time.time()
            host = [L.oracle(x) for L, x in zip(lats, refs)]
            t_host.append(time.time() - t0)
            same = sum(1 for u, h in enumerate(host) if h["counts"].tolist() == r["counts"][u].tolist() and int(r["status"][u]) == h["status"])
        ms = {k: float(np.median([x.get(k, 0.0) for x in k_ms])) for k in sorted({k for x in k_ms for k in x})}
        c = r["counts"].astype(np.int64).sum(axis=0)
        out["oracle"] = {"kernels_ms": ms, "call": med(t_dev), "download": med(t_dl), "host_loop": med(t_host), "same_as_host": same,
                         "host_over_device": float(np.median(t_host)) / float(np.median(t_dev)), "succeeded": int((r["status"] & 1 != 0).sum()),
                         "errors": int(c[0]), "ref_words": int(R.sum())}
    if score:
        lo, hi = (int(x) for x in score.split(":"))
        pens = (0.0, 0.5, 1.0)
        pts = [(w, p) for w in range(lo, hi + 1) for p in pens]
        gs = np.ones(len(pts), np.float32)
        as_ = np.asarray([1.0 / w for w, _ in pts], np.float32)
        pn = np.asarray([p for _, p in pts], np.float32)
        ro = np.concatenate([[0], np.cumsum(R)]).astype(np.int64)
        rf = np.concatenate(refs + [np.zeros(1, np.int32)]).astype(np.int32)
        p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

        def old_way():
            """-> counts [points * U][4] in wer's order"""
            res = np.zeros((len(pts) * U, 4), np.int32)
            for j, p in enumerate(pens):
                d = dl.add_penalty(p)
                ws = list(range(lo, hi + 1))
                bp = d.best_path(np.ones(len(ws), np.float32), np.asarray([1.0 / w for w in ws], np.float32))
                d.close()
                ho = np.asarray(bp["words_off"], np.int64)
                hf = np.concatenate([bp["words"], np.zeros(1, np.int32)]).astype(np.int32)
                cnt = np.zeros((len(ws) * U, 4), np.int32)
                rr = np.concatenate([[0], np.cumsum(np.tile(R, len(ws)))]).astype(np.int64)
                rt = np.concatenate([np.concatenate(refs)] * len(ws) + [np.zeros(1, np.int32)]).astype(np.int32)
                rc = _lib.lib.khg_edit_distance(len(ws) * U, rt.ctypes.data_as(p32), rr.ctypes.data_as(p64), hf.ctypes.data_as(p32), ho.ctypes.data_as(p64),
                                                cnt.ctypes.data_as(p32))
                assert rc == 0
                for i in range(len(ws)):
                    k = i * len(pens) + j
                    res[k * U: (k + 1) * U] = cnt[i * U: (i + 1) * U]
            return res

        dl.wer(refs, gs, as_, pn); old_way(); ctx.sync()                  # warm-up
        t_new, t_old, k_ms, same = [], [], [], False
        for _ in range(reps):
            k_ms.append(kernel_ms(ctx, lambda: dl.wer(refs, gs, as_, pn)))
            ctx.sync(); t0 = time.time()
            w = dl.wer(refs, gs, as_, pn)
            t_new.append(time.time() - t0)
            t0 = time.time()
            o = old_way()
            t_old.append(time.time() - t0)
            same = bool((o == w["counts"]).all())
        ms = {k: float(np.median([x.get(k, 0.0) for x in k_ms])) for k in sorted({k for x in k_ms for k in x})}
        err = w["counts"][:, 0].reshape(len(pts), U).astype(np.int64).sum(axis=1)
        out["wer"] = {"points": len(pts), "kernels_ms": ms, "call": med(t_new), "old_way": med(t_old), "same_counts_as_old_way": same,
                      "old_over_new": float(np.median(t_old)) / float(np.median(t_new)), "best_point": list(pts[int(err.argmin())]),
                      "best_errors": int(err.min()), "ref_words": int(R.sum()), "bytes_back": int(w["counts"].nbytes + w["nwords"].nbytes + w["status"].nbytes)}
        # add_penalty beside a device-to-device copy of the same bytes
        nbytes = 4 * (6 * int(so[-1]) + 5 * int(ao[-1]))
        t_pen, t_copy, k_pen = [], [], []
        try:
            import torch
            a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            b = torch.empty_like(a)
        except Exception:
            torch = None
        for _ in range(reps):
            k_pen.append(kernel_ms(ctx, lambda: dl.add_penalty(0.5).close()))
            ctx.sync(); t0 = time.time()
            d = dl.add_penalty(0.5)
            t_pen.append(time.time() - t0)
            d.close()
            if torch is not None:
                torch.cuda.synchronize(); t0 = time.time()
                b.copy_(a); torch.cuda.synchronize()
                t_copy.append(time.time() - t0)
        out["add_penalty"] = {"bytes": nbytes, "call": med(t_pen), "device_copy": med(t_copy) if t_copy else None,
                              "kernel_ms": float(np.median([x.get("k2_lattice_score_add_penalty", 0.0) for x in k_pen]))}
    return out


def mbr_bench(ctx, dl, reps, gs=1.0, as_=0.1):
    """--mbr on resident lattices, both sides in this process and alternated: DeviceLattices.mbr at (gs, as_) from the
    best path beside the download of every lattice and a loop of the host form Lattice.mbr; then the host form once more with the
    device's weights, which must give the device's outputs bit for bit."""
    reps = max(reps, 3)
    U = dl.num_utts
    so, ao = np.asarray(dl.state_off), np.asarray(dl.arc_off)
    r = dl.mbr(gs, as_); ctx.sync()                                      # warm-up (builds the in-arc index once)
    t_dev, t_dl, t_host, k_ms = [], [], [], []
    for _ in range(reps):
        k_ms.append(kernel_ms(ctx, lambda: dl.mbr(gs, as_)))
        ctx.sync(); t0 = time.time()
        r = dl.mbr(gs, as_)
        t_dev.append(time.time() - t0)
        t0 = time.time()
        lats = dl.download()
        t_dl.append(time.time() - t0)
        t0 = time.time()
        host = [L.mbr(gs, as_) for L in lats]
        t_host.append(time.time() - t0)
    per = khg.mbr_utterances(r)
    same = same_words = 0
    for L, d, h in zip(lats, per, host):
        g = L.mbr(gs, as_, arc_cond=d["arc_cond"], final_cond=d["final_cond"])
        same += g["status"] == d["status"] and g["iters"] == d["iters"] and g["bayes_risk"] == d["bayes_risk"] and g["words"].tolist() == d["words"].tolist() \
            and g["conf"].tobytes() == d["conf"].tobytes() and g["gamma"].tobytes() == d["gamma"].tobytes()
        same_words += h["words"].tolist() == d["words"].tolist()
    ok = [d for d in per if d["status"] & 1]
    W = np.asarray([len(d["words"]) for d in ok] or [0])
    V = np.asarray([len(d["vocab"]) for d in ok] or [1])
    it = np.asarray([d["iters"] for d in ok] or [0])
    ms = {k: float(np.median([x.get(k, 0.0) for x in k_ms])) for k in sorted({k for x in k_ms for k in x})}
    return {"utterances": U, "graph_scale": gs, "acoustic_scale": as_, "states_mean": float(np.diff(so).mean()), "arcs_mean": float(np.diff(ao).mean()),
            "repetitions": reps, "succeeded": len(ok), "not_converged": sum(1 for d in ok if d["status"] & 2048), "words_mean": float(W.mean()),
            "vocab_mean": float(V.mean()), "vocab_max": int(V.max()), "iters_mean": float(it.mean()), "iters_max": int(it.max()),
            "iters_histogram": np.bincount(it).tolist(), "lane_occupancy_mean": float(((2 * W + 2) / (64.0 * np.ceil((2 * W + 2) / 64.0))).mean()),
            "positions_mean": float((2 * W + 2).mean()), "bayes_risk_mean": float(np.mean([d["bayes_risk"] for d in ok] or [0.0])),
            "kernels_ms": ms, "call": med(t_dev), "download": med(t_dl), "host_loop": med(t_host),
            "host_over_device": float(np.median(t_host)) / float(np.median(t_dev)), "same_as_host_given_device_weights": same,
            "same_words_as_host_with_its_own_weights": same_words}


def det_bench(ctx, dl, reps, beam, delta=1.0 / 1024, state_factor=8):
    """--det on resident lattices, both sides in this process and alternated: DeviceLattices.determinize at (1, 1, beam)
    beside the download of every lattice and a loop of the host form Lattice.determinize, which must give the device's lattices bit
    for bit; states before and after."""
    reps = max(reps, 3)
    U = dl.num_utts
    so, ao = np.asarray(dl.state_off), np.asarray(dl.arc_off)
    res, st, stats = dl.determinize(1.0, 1.0, beam, delta, state_factor); ctx.sync()       # warm-up
    res.close()
    t_dev, t_dl, t_host, k_ms = [], [], [], []
    for _ in range(reps):
        def call():
            dl.determinize(1.0, 1.0, beam, delta, state_factor)[0].close()
        k_ms.append(kernel_ms(ctx, call))
        ctx.sync(); t0 = time.time()
        res, st, stats = dl.determinize(1.0, 1.0, beam, delta, state_factor)
        t_dev.append(time.time() - t0)
        t0 = time.time()
        lats = dl.download()
        t_dl.append(time.time() - t0)
        t0 = time.time()
        host = [L.determinize(1.0, 1.0, beam, delta, state_factor) for L in lats]
        t_host.append(time.time() - t0)
        got = res.download()
        res.close()
    fields = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")
    same = sum(1 for G, (H, hst, _), s in zip(got, host, st)
               if hst == int(s) and G.start == H.start and all(np.asarray(getattr(G, f)).tobytes() == np.asarray(getattr(H, f)).tobytes() for f in fields))
    ms = {k: float(np.median([x.get(k, 0.0) for x in k_ms])) for k in sorted({k for x in k_ms for k in x})}
    return {"utterances": U, "beam": beam, "delta": delta, "state_factor": state_factor, "repetitions": reps, "succeeded": int((np.asarray(st) == 1).sum()),
            "scratch": int((np.asarray(st) == 4).sum()), "states_before_mean": float(np.diff(so).mean()), "arcs_before_mean": float(np.diff(ao).mean()),
            "states_after_mean": stats["out_states"] / max(U, 1), "arcs_after_mean": stats["out_arcs"] / max(U, 1), "stats": {k: int(v) for k, v in stats.items()},
            "kernels_ms": ms, "call": med(t_dev), "download": med(t_dl), "host_loop": med(t_host),
            "host_over_device": float(np.median(t_host)) / float(np.median(t_dev)), "same_as_host": same}


def nbest_bench(ctx, dl, reps, n, beam, delta=1.0 / 1024, state_factor=8):
    """--nbest N on resident lattices, both sides in this process and alternated: the lattices are determinized once at
    (1, 1, beam); then DeviceLattices.nbest(N) with everything downloaded beside the download of every determinized lattice and a loop
    of the host form Lattice.nbest, which must give the device's entries bit for bit."""
    from kaldi_hmm_gmm_amd import NbestList
    reps = max(reps, 3)
    det, dst, _ = dl.determinize(1.0, 1.0, beam, delta, state_factor)
    U = det.num_utts
    so, ao = np.asarray(det.state_off), np.asarray(det.arc_off)
    det.nbest(n).close(); ctx.sync()       # warm-up (builds the handle's in-arc index)
    t_dev, t_dl, t_host, k_ms = [], [], [], []
    for _ in range(reps):
        def call():
            nb = det.nbest(n); nb.download(); nb.close()
        k_ms.append(kernel_ms(ctx, call))
        ctx.sync(); t0 = time.time()
        nb = det.nbest(n)
        arrays = nb.download()
        t_dev.append(time.time() - t0)
        nbytes = nb.device_bytes
        nb.close()
        t0 = time.time()
        lats = det.download()
        t_dl.append(time.time() - t0)
        t0 = time.time()
        host = [L.nbest_with_status(n) for L in lats]
        t_host.append(time.time() - t0)
    nl = NbestList(arrays)
    same = sum(1 for u, (got, hst, _) in enumerate(host) if hst == int(nl.status[u]) and [tuple(x) for x in got] == [tuple(x) for x in nl.entries(u)])
    ms = {k: float(np.median([x.get(k, 0.0) for x in k_ms])) for k in sorted({k for x in k_ms for k in x})}
    counts = np.asarray(nl.counts)
    det.close()
    return {"utterances": U, "n": n, "beam": beam, "repetitions": reps, "succeeded": int((np.asarray(nl.status) == 1).sum()),
            "determinize_succeeded": int((np.asarray(dst) == 1).sum()), "states_mean": float(np.diff(so).mean()), "arcs_mean": float(np.diff(ao).mean()),
            "entries": int(counts.sum()), "entries_mean": float(counts.mean()), "lists_full": int((counts == n).sum()), "device_bytes": int(nbytes),
            "kernels_ms": ms, "call_with_download": med(t_dev), "download_lattices": med(t_dl), "host_loop": med(t_host),
            "host_over_device": (float(np.median(t_host)) + float(np.median(t_dl))) / float(np.median(t_dev)), "same_as_host": same}


def time_paths(ctx, dtm, sets, hubs, reps, with_faster=True, lattices=False):
    """sets: {path: UtteranceSet with resident scores}.  -> {path: {what: [seconds]}}, paths and options alternated inside every repetition
    after one warm-up round; and the last results."""
    times = {p: {} for p in sets}
    last = {}
    default = ctx.get_option("k2s_hub")
    try:
        for rep in range(reps + 1):
            for p, us in sets.items():
                if with_faster:
                    ctx.sync(); t0 = time.time()
                    last[(p, "faster")] = us.decode_lattice_faster(dtm, beam=13.0, max_active=7000, lattice_beam=6.0, acoustic_scale=0.1)
                    if rep:
                        times[p].setdefault("lattice_faster", []).append(time.time() - t0)
                for h in hubs:
                    ctx.set_option("k2s_hub", h)
                    ctx.sync(); t0 = time.time()
                    last[(p, "simple", h)] = us.decode_lattice_simple(dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
                    if rep:
                        times[p].setdefault("lattice_simple_hub_%d" % h, []).append(time.time() - t0)
                    if lattices:
                        ctx.sync(); t0 = time.time()
                        r = us.raw_lattice_simple(dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
                        last[(p, "raw", h)] = r
                        if rep:
                            times[p].setdefault("raw_lattice_simple_hub_%d" % h, []).append(time.time() - t0)
                            times[p].setdefault("raw_decode_call_hub_%d" % h, []).append(r["decode_s"])
                            times[p].setdefault("raw_download_hub_%d" % h, []).append(r["download_s"])
    finally:
        ctx.set_option("k2s_hub", default)
    return times, last


def shared_graph_main(args):
    from kaldi_hmm_gmm_amd import _gpu
    from kaldi_hmm_gmm_amd import _kaldi_hmm_gmm_amd as ext
    hubs = [int(x) for x in args.hub.split(",")]
    ctx = _gpu.default_context()
    out = {"mode": "yesno" if args.yesno else "shared-graph", "utterances": args.utts, "hub_thresholds": hubs, "hub_default": ctx.get_option("k2s_hub")}
    if args.yesno:                      # the trained monophone model and the 46-state YES/NO word loop of examples/decode_synthetic.py
        import types
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
        import decode_synthetic as dx
        from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions
        tm, tree, am, lexicon, test_utts = dx.train(types.SimpleNamespace(utts=200, test_utts=30, iters=80, dim=23, seed=3), log=lambda *a: None)
        gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                   opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import lattice_simple_ref as ref
        gl = ref.add_eps_self_loops(gc.compile_word_loop_graph().to_csr(), 0.0)
        feats = [np.ascontiguousarray(test_utts[u % len(test_utts)][2], np.float32) for u in range(args.utts)]
        dg = khg.DecodingGraph(fst_of(gl), tm)
        out.update(states=dg.num_states, arcs=dg.num_arcs, max_in_degree=dg.max_in_degree)
        scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
        times = {}
        khg.decode_lattice_simple_batch(am, tm, dg, feats, scfg, 0.1)
        for rep in range(args.reps):
            for h in hubs:
                ctx.set_option("k2s_hub", h)
                t0 = time.time()
                res = khg.decode_lattice_simple_batch(am, tm, dg, feats, scfg, 0.1)
                times.setdefault("lattice_simple_batch_hub_%d" % h, []).append(time.time() - t0)
        ctx.set_option("k2s_hub", out["hub_default"])
        out["shared"] = {k: med(v) for k, v in times.items()}
        out["succeeded_share"] = sum(1 for r in res if r["succeeded"]) / len(res)
        print(json.dumps(out))
        return
    m = synth.make_model(5000, 64, 40, seed=args.seed)
    g, pdfs = word_loop(m, args.words, args.seed + 7, False, args.loop_states)
    gl, _ = word_loop(m, args.words, args.seed + 7, True, args.loop_states)
    rng = np.random.default_rng(args.seed + 1000)
    picks = [rng.integers(0, args.words, size=int(rng.integers(2, 5))) for _ in range(args.utts)]          # the words said: word k carries the id k + 1
    seqs = [np.concatenate([pdfs[int(k)] for k in p]) for p in picks]
    durs = [rng.geometric(0.25, size=len(sq)) for sq in seqs]
    frame_pdf = np.concatenate([np.repeat(sq, d) for sq, d in zip(seqs, durs)])
    fo = np.concatenate([[0], np.cumsum([int(d.sum()) for d in durs])]).astype(np.int64)
    feats = synth.sample_feats(m, frame_pdf, rng)
    gcs, bad = ext.compute_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    dm = khg.DeviceModel(ctx, m.gauss_off, gcs, m.means_invvars, m.inv_vars)
    dtm = khg.DeviceTransitions(ctx, m.id2pdf)
    U = args.utts
    out.update(words=args.words, loop_states=args.loop_states, frames=int(fo[-1]))
    res = {}
    for name, gg in (("faster", g), ("simple", gl)):       # the simple decoder's graph carries the epsilon self-loops
        S, A = len(gg["final"]), len(gg["ilabel"])
        rep_bytes = 8 * (U + 1) + 4 * U + 16 * (U * S + 1) + 24 * U * A + 4 * U * S          # from the shapes, before anything is allocated
        ctx.sync(); t0 = time.time()
        dg = khg.DecodingGraph(fst_of(gg), dtm)
        sh = khg.UtteranceSet(ctx, dtm, fo, feats, graph=dg)
        ctx.sync(); t_sh = time.time() - t0
        entry = {"states": S, "arcs": A, "max_in_degree": dg.max_in_degree, "num_pdfs": dg.num_pdfs,
                 "shared": {"create_s": t_sh, "graph_bytes_graph": dg.device_bytes, "graph_bytes_set": sh.graph_bytes}}
        sets = {"shared": sh}
        if dg.max_in_degree > 254 or S > 65535:
            entry["replicated"] = "not run: the list-of-graphs path refuses this graph (the aligner's limits)"
        elif rep_bytes < (8 << 30) and not args.no_replicated:
            tg = tiled(gg, U)
            ctx.sync(); t0 = time.time()
            rp = khg.UtteranceSet(ctx, dtm, fo, feats, graphs=tg)
            ctx.sync()
            entry["replicated"] = {"create_s": time.time() - t0, "graph_bytes_set": rp.graph_bytes}
            entry["create_ratio"] = entry["replicated"]["create_s"] / t_sh
            entry["bytes_ratio"] = rp.graph_bytes / dg.device_bytes
            sets["replicated"] = rp
            del tg
        else:
            entry["replicated"] = "not run: %.1f GiB of tables" % (rep_bytes / 2.0 ** 30)
        for us in sets.values():
            us.loglikes(dm)
        ctx.sync()
        lat = args.lattices and name == "simple"
        times, last = time_paths(ctx, dtm, sets, hubs if name == "simple" else [], args.reps, with_faster=name == "faster", lattices=lat)
        for p in sets:
            entry[p].update({k: med(v) for k, v in times[p].items()})
        key = ("shared", "faster") if name == "faster" else ("shared", "simple", hubs[0])
        entry["succeeded_share"] = float(((last[key]["status"] & 1) != 0).mean())
        same = all(last[key][f].tobytes() == r[f].tobytes() for r in last.values() for f in ("ali", "like", "status", "words", "words_off"))
        entry["all_paths_and_thresholds_identical"] = bool(same)
        if lat:
            raws = [r for k, r in last.items() if k[1] == "raw"]
            fields = ("state_off", "arc_off", "start", "frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel",
                      "graph_cost", "acoustic_cost", "nextstate")
            entry["lattices_identical_across_paths_and_thresholds"] = bool(all(raws[0][f].tobytes() == r[f].tobytes() for r in raws for f in fields))
            h = hubs[-1]
            r = last[("shared", "raw", h)]
            entry["lattices"] = lattice_sizes(np.diff(r["state_off"]), np.diff(r["arc_off"]), times["shared"]["raw_download_hub_%d" % h])
            entry["lattices"]["device_bytes"] = int(r["device_bytes"])
            ctx.set_option("k2s_hub", h)
            try:
                k_old = kernel_ms(ctx, lambda: sh.decode_lattice_simple(dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1))
                k_new = kernel_ms(ctx, lambda: sh.raw_lattice_simple(dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1))
            finally:
                ctx.set_option("k2s_hub", out["hub_default"])
            entry["lattices"].update(emission_summary(k_old, k_new), hub=h)
            if args.sweep or args.prune_beam is not None or args.post:
                d = sh.raw_lattices_simple_device(dtm, beam=13.0, lattice_beam=6.0, acoustic_scale=0.1)
                entry["lattice_ops"] = lattice_ops(ctx, d["lattices"], args.sweep, args.prune_beam, args.reps, args.post)
                d["lattices"].close()
        if args.check > 0:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
            import lattice_faster_ref as fref
            import lattice_simple_ref as sref
            am, tmh = synth.host_objects(m)
            n = min(args.check, U)
            fl = [feats[fo[u]: fo[u + 1]] for u in range(n)]
            if name == "faster":
                chk = khg.decode_lattice_faster_batch(am, tmh, dg, fl, khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0), 0.1,
                                                      return_scores=True)
            else:
                chk = khg.decode_lattice_simple_batch(am, tmh, dg, fl, khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0), 0.1, return_scores=True)
            match = 0
            for u, r in enumerate(chk):
                ll = fref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, 0.1)
                if name == "faster":
                    want = fref.decode_utterance_lattice_faster(fref.Graph.from_dict(gg), fref.Config(max_active=7000, beam=13.0, lattice_beam=6.0), ll, len(fl[u]))
                else:
                    want = sref.decode_utterance_lattice_simple(fref.Graph.from_dict(gg), sref.Config(beam=13.0, lattice_beam=6.0), ll, len(fl[u]))
                match += (r["succeeded"], r["alignment"], r["words"], r["like"]) == (want["succeeded"], want["alignment"], want["words"], want["like"]) \
                    and last[key]["ali"][fo[u]: fo[u + 1]].tolist() == r["alignment"]
            entry.update(checked_against_restatement=n, restatement_matches=match)
        if args.lmrescore and name == "faster":
            # lattice-lmrescore on the lattices the shared set leaves on the device, beside decoding that set again
            dec = dict(beam=13.0, max_active=7000, lattice_beam=6.0, acoustic_scale=0.1)
            L = sh.raw_lattices_faster_device(dtm, **dec)["lattices"]
            t_dec = []
            for _ in range(max(args.reps, 3)):
                ctx.sync(); t0 = time.time()
                sh.raw_lattices_faster_device(dtm, **dec)["lattices"].close()
                t_dec.append(time.time() - t0)
            bp = L.best_path(np.ones(1, np.float32), np.ones(1, np.float32))
            wo = bp["words_off"]
            transcripts = [bp["words"][wo[u]: wo[u + 1]].tolist() for u in range(U)]
            entry["lmrescore"] = lmrescore_bench(ctx, L, transcripts, range(1, args.words + 1), args.lmrescore, args.reps, med(t_dec))
            L.close()
        if (args.oracle or args.score) and name == "faster":
            # scoring the lattices the shared set leaves on the device against the words that were said; again at a wider lattice beam
            entry["score"] = {}
            for lb in (6.0, args.dense_lattice_beam):
                L = sh.raw_lattices_faster_device(dtm, beam=13.0, max_active=7000, lattice_beam=lb, acoustic_scale=0.1)["lattices"]
                entry["score"]["lattice_beam_%g" % lb] = score_bench(ctx, L, [p + 1 for p in picks], args.score, args.oracle, args.reps)
                L.close()
        if args.mbr and name == "faster":
            # minimum Bayes risk decoding of the lattices the shared set leaves on the device; again at a wider lattice beam
            entry["mbr"] = {}
            for lb in (6.0, args.dense_lattice_beam):
                L = sh.raw_lattices_faster_device(dtm, beam=13.0, max_active=7000, lattice_beam=lb, acoustic_scale=0.1)["lattices"]
                entry["mbr"]["lattice_beam_%g" % lb] = mbr_bench(ctx, L, args.reps)
                L.close()
        if args.det and name == "faster":
            # determinizing the lattices the shared set leaves on the device, each set at its own lattice beam (what GetLattice does)
            entry["det"] = {}
            for lb in (6.0, args.dense_lattice_beam):
                L = sh.raw_lattices_faster_device(dtm, beam=13.0, max_active=7000, lattice_beam=lb, acoustic_scale=0.1)["lattices"]
                entry["det"]["lattice_beam_%g" % lb] = det_bench(ctx, L, args.reps, lb if args.det_beam is None else args.det_beam)
                L.close()
        if args.nbest and name == "faster":
            # the n-best lists of the lattices the shared set leaves on the device, determinized, each set at its own lattice beam
            entry["nbest"] = {}
            for lb in (6.0, args.dense_lattice_beam):
                L = sh.raw_lattices_faster_device(dtm, beam=13.0, max_active=7000, lattice_beam=lb, acoustic_scale=0.1)["lattices"]
                entry["nbest"]["lattice_beam_%g" % lb] = nbest_bench(ctx, L, args.reps, args.nbest, lb if args.det_beam is None else args.det_beam)
                L.close()
        for us in sets.values():
            us.close()
        dg.close()
        res[name] = entry
    out.update(res)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shared-graph", action="store_true")
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--hub", default="0,32", help="thresholds of the simple decoder's hub form to time (0 = off)")
    ap.add_argument("--no-replicated", action="store_true")
    ap.add_argument("--loop-states", type=int, default=1, help="copies of the loop state the words' in-arcs are divided among")
    ap.add_argument("--yesno", action="store_true")
    ap.add_argument("--utts", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--decoder", choices=("faster", "simple"), default="faster")
    ap.add_argument("--check", type=int, default=0)
    ap.add_argument("--lattices", action="store_true", help="also time the raw-lattice call of --decoder and report the lattices")
    ap.add_argument("--sweep", default=None, metavar="LO:HI", help="with --lattices: best paths at the integer LM weights LO..HI in one call")
    ap.add_argument("--prune-beam", type=float, default=None, help="with --lattices: prune the resident lattices to this beam")
    ap.add_argument("--post", action="store_true", help="with --lattices: forward-backward posteriors of the resident lattices")
    ap.add_argument("--acc", action="store_true", help="with --lattices --post: GMM statistics from those posteriors (khg_acc_stats_post)")
    ap.add_argument("--mpe", action="store_true", help="with --lattices (--decoder faster): MPE / sMBR posteriors beside posteriors(), and "
                    "khg_acc_stats_post2 beside khg_acc_stats_post")
    ap.add_argument("--criterion", choices=("mpe", "smbr"), default="smbr", help="with --mpe")
    ap.add_argument("--rescore", action="store_true", help="with --lattices (--decoder faster): khg_lattices_rescore on the resident lattices, and "
                    "one MMI iteration's denominator side with it against decoding again")
    ap.add_argument("--boost", type=float, default=0.0, metavar="B", help="with --rescore: also khg_lattices_boost at this b")
    ap.add_argument("--lmrescore", type=int, nargs="?", const=2, default=0, metavar="ORDER", help="with --lattices (--decoder faster): "
                    "khg_lattices_lm_rescore on the resident lattices with an n-gram of this order (2) estimated from the decoded words")
    ap.add_argument("--oracle", action="store_true", help="with --lattices (--decoder faster): DeviceLattices.oracle on the resident lattices beside the "
                    "download and a loop of the host form Lattice.oracle (DESIGN.md 7s)")
    ap.add_argument("--score", default=None, metavar="LO:HI", help="with --lattices (--decoder faster): DeviceLattices.wer at the LM weights LO..HI x "
                    "penalties {0, 0.5, 1} beside add_penalty + best_path + the host's khg_edit_distance; add_penalty beside a device copy")
    ap.add_argument("--mbr", action="store_true", help="with --lattices (--decoder faster): DeviceLattices.mbr on the resident lattices beside the "
                    "download and a loop of the host form Lattice.mbr (DESIGN.md 7t)")
    ap.add_argument("--det", action="store_true", help="with --shared-graph --lattices (--decoder faster): DeviceLattices.determinize on the resident "
                    "lattices beside the download and a loop of the host form Lattice.determinize (DESIGN.md 7u)")
    ap.add_argument("--nbest", type=int, default=0, metavar="N", help="with --shared-graph --lattices (--decoder faster): DeviceLattices.nbest(N) on the "
                    "resident lattices, determinized, beside their download and a loop of the host form Lattice.nbest (DESIGN.md 7v)")
    ap.add_argument("--det-beam", type=float, default=None, metavar="B", help="with --det: the determinization beam (default: each set's lattice beam)")
    ap.add_argument("--dense-lattice-beam", type=float, default=12.0, help="with --shared-graph --oracle / --score / --mbr / --det: the second, denser set's lattice beam")
    args = ap.parse_args()
    if args.nbest and (not args.lattices or args.decoder != "faster" or not args.shared_graph or args.yesno or not 1 <= args.nbest <= 1024):
        ap.error("--nbest N needs --shared-graph --lattices with --decoder faster, 1 <= N <= 1024 (and is not timed with --yesno)")
    if args.det and (not args.lattices or args.decoder != "faster" or not args.shared_graph or args.yesno):
        ap.error("--det needs --shared-graph --lattices with --decoder faster (and is not timed with --yesno)")
    if args.mbr and (not args.lattices or args.decoder != "faster" or args.yesno):
        ap.error("--mbr needs --lattices with --decoder faster (and is not timed with --yesno)")
    if (args.oracle or args.score) and (not args.lattices or args.decoder != "faster" or args.yesno):
        ap.error("--oracle / --score need --lattices with --decoder faster (and are not timed with --yesno)")
    if (args.sweep or args.prune_beam is not None or args.post) and not args.lattices:
        ap.error("--sweep / --prune-beam / --post need --lattices")
    if args.rescore and (not args.lattices or args.decoder != "faster" or args.shared_graph or args.yesno):
        ap.error("--rescore needs --lattices with --decoder faster (and is not timed with --shared-graph / --yesno)")
    if args.mpe and (not args.lattices or args.decoder != "faster" or args.shared_graph or args.yesno):
        ap.error("--mpe needs --lattices with --decoder faster (and is not timed with --shared-graph / --yesno)")
    if args.lmrescore and (not args.lattices or args.decoder != "faster" or args.yesno):
        ap.error("--lmrescore needs --lattices with --decoder faster (and is not timed with --yesno)")
    if args.acc and (not args.post or args.shared_graph):
        ap.error("--acc needs --lattices --post (and is not timed with --shared-graph)")
    if args.shared_graph or args.yesno:
        shared_graph_main(args)
        return
    m = synth.make_model(5000, 64, 40, seed=args.seed)
    am, tm = synth.host_objects(m)
    ut = synth.make_utts(m, args.utts, seed=args.seed + 1000)
    if args.decoder == "simple":
        fsts = [with_eps_self_loops(ut.graphs, u) for u in range(args.utts)]
    else:
        fsts = [synth.utt_fst(ut.graphs, u) for u in range(args.utts)]
    feats = [ut.feats[ut.frame_off[u]: ut.frame_off[u + 1]] for u in range(args.utts)]
    frames = int(ut.frame_off[-1])
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    lat_s, ali_s, res = [], [], None
    if args.decoder == "simple":
        scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
        simple_s = []
        khg.decode_lattice_simple_batch(am, tm, fsts[:64], feats[:64], scfg, 0.1)          # warm-up
        raw_s, raw_dec_s, raw_dl_s, raw = [], [], [], None
        if args.lattices:
            khg.get_raw_lattice_simple_batch(am, tm, fsts[:64], feats[:64], scfg, 0.1)     # warm-up
        for _ in range(args.reps):
            t0 = time.time()
            res = khg.decode_lattice_simple_batch(am, tm, fsts, feats, scfg, 0.1)
            simple_s.append(time.time() - t0)
            if args.lattices:
                t0 = time.time()
                raw, t = khg.get_raw_lattice_simple_batch(am, tm, fsts, feats, scfg, 0.1, return_times=True)
                raw_s.append(time.time() - t0); raw_dec_s.append(t["decode_s"]); raw_dl_s.append(t["download_s"])
    for _ in range(args.reps):
        t0 = time.time()
        fres = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
        lat_s.append(time.time() - t0)
        t0 = time.time()
        khg.align_batch(am, tm, fsts, feats, khg.AlignConfig(beam=13.0), 0.1,
                        decoder_opts=khg.FasterDecoderOptions(beam=13.0, max_active=7000))
        ali_s.append(time.time() - t0)
    if res is None:
        res = fres
    if args.lattices and args.decoder == "faster":
        # the raw-lattice call of the lattice-faster decoder (get_raw_lattice_faster_batch) beside the plain call, as for --decoder simple
        from kaldi_hmm_gmm_amd import _gpu
        ctx = _gpu.default_context()
        khg.get_raw_lattice_faster_batch(am, tm, fsts[:64], feats[:64], cfg, 0.1)           # warm-up
        raw_s, raw_dec_s, raw_dl_s, raw = [], [], [], None
        for _ in range(args.reps):
            t0 = time.time()
            raw, t = khg.get_raw_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1, return_times=True)
            raw_s.append(time.time() - t0); raw_dec_s.append(t["decode_s"]); raw_dl_s.append(t["download_s"])
        flat = lattice_sizes([r["lattice"].num_states for r in raw], [r["lattice"].num_arcs_total for r in raw], raw_dl_s)
        flat.update(raw_call=med(raw_s), raw_decode_call=med(raw_dec_s),
                    same_best_paths_as_old_call=sum(1 for a, b in zip(fres, raw) if all(a[k] == b[k] for k in a)))
        k_old = kernel_ms(ctx, lambda: khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1))
        k_new = kernel_ms(ctx, lambda: khg.get_raw_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1))
        dec_old, dec_new = k_old.get("k2_lattice_faster", 0.0), k_new.get("k2_lattice_faster", 0.0)
        emit = sum(v for k, v in k_new.items() if k.startswith("k2_lattice_faster_raw"))
        flat.update(old_call_kernels_ms=k_old, raw_call_kernels_ms=k_new, k2_lattice_faster_ms=dec_old, decoder_lane_extra_ms=dec_new - dec_old,
                    emission_kernels_ms=emit, emission_over_decoder=(emit + dec_new - dec_old) / dec_old if dec_old else None)
        faster_lat = flat
        faster_ops = None
        if args.sweep or args.prune_beam is not None or args.post or args.rescore or args.mpe or args.lmrescore or args.oracle or args.score or args.mbr:
            _, dl = khg.get_raw_lattice_faster_device_batch(am, tm, fsts, feats, cfg, 0.1)
            faster_ops = {}
            if args.sweep or args.prune_beam is not None or args.post:
                faster_ops = lattice_ops(ctx, dl, args.sweep, args.prune_beam, args.reps, args.post)
            if args.acc:
                faster_ops["acc_stats_post"] = acc_from_post(ctx, dl, am, tm, feats, [r["alignment"] for r in fres], args.reps)
            if args.mpe:
                faster_ops["mpe"] = mpe_bench(ctx, dl, am, tm, feats, [r["alignment"] for r in fres], args.criterion, args.reps)
            if args.rescore:
                faster_ops["rescore"] = rescore_bench(ctx, dl, am, tm, fsts, feats, [r["alignment"] for r in fres], cfg, args.reps, args.boost)
            if args.lmrescore:
                vocab = sorted(set(int(w) for w in np.unique(ut.graphs["olabel"]) if w > 0))
                faster_ops["lmrescore"] = lmrescore_bench(ctx, dl, [r["words"] for r in fres], vocab, args.lmrescore, args.reps, flat["raw_decode_call"])
            if args.oracle or args.score:
                faster_ops["score"] = score_bench(ctx, dl, [r["words"] for r in fres], args.score, args.oracle, args.reps)
            if args.mbr:
                faster_ops["mbr"] = mbr_bench(ctx, dl, args.reps)
            dl.close()
    st = [r["status"] for r in res]
    out = {"decoder": args.decoder,"utterances": args.utts, "frames": frames, "lattice_s": min(lat_s), "lattice_frames_per_s": frames / min(lat_s),
           "faster_decoder_s": min(ali_s), "ratio": min(lat_s) / min(ali_s),
           "succeeded": sum(1 for s in st if s & 1), "partial": sum(1 for s in st if s & 2), "scratch": sum(1 for s in st if s & 4)}
    out["lattice"] = med(lat_s)
    out["lattice_faster_output_sha1"] = hashlib.sha1(repr([(r["status"], r["alignment"], r["words"], r["like"]) for r in fres]).encode()).hexdigest()
    if args.lattices and args.decoder == "faster":
        out["lattices"] = faster_lat
        if faster_ops is not None:
            out["lattice_ops"] = faster_ops
    if args.decoder == "simple":
        out.update(simple_s=min(simple_s), simple_frames_per_s=frames / min(simple_s), simple_over_lattice_faster=min(simple_s) / min(lat_s),
                   simple_over_faster_decoder=min(simple_s) / min(ali_s),
                   same_best_paths_as_lattice_faster=sum(1 for a, b in zip(res, fres) if a["alignment"] == b["alignment"]))
        out["simple"] = med(simple_s)
        if args.lattices:
            from kaldi_hmm_gmm_amd import _gpu
            ctx = _gpu.default_context()
            lat = lattice_sizes([r["lattice"].num_states for r in raw], [r["lattice"].num_arcs_total for r in raw], raw_dl_s)
            lat.update(raw_call=med(raw_s), raw_decode_call=med(raw_dec_s),
                       same_best_paths_as_old_call=sum(1 for a, b in zip(res, raw) if all(a[k] == b[k] for k in a)))
            k_old = kernel_ms(ctx, lambda: khg.decode_lattice_simple_batch(am, tm, fsts, feats, scfg, 0.1))
            k_new = kernel_ms(ctx, lambda: khg.get_raw_lattice_simple_batch(am, tm, fsts, feats, scfg, 0.1))
            lat.update(emission_summary(k_old, k_new))
            out["lattices"] = lat
            if args.sweep or args.prune_beam is not None or args.post:
                _, dl = khg.get_raw_lattice_simple_device_batch(am, tm, fsts, feats, scfg, 0.1)
                out["lattice_ops"] = lattice_ops(ctx, dl, args.sweep, args.prune_beam, args.reps, args.post)
                if args.acc:
                    out["lattice_ops"]["acc_stats_post"] = acc_from_post(ctx, dl, am, tm, feats, [r["alignment"] for r in res], args.reps)
                dl.close()
        if args.check > 0:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
            import lattice_simple_ref as ref
            n = min(args.check, args.utts)
            chk = khg.decode_lattice_simple_batch(am, tm, fsts[:n], feats[:n], scfg, 0.1, return_scores=True)
            match = 0
            for u, r in enumerate(chk):
                g = fsts[u].to_csr()
                want = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(beam=13.0, lattice_beam=6.0),
                                                           ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, 0.1), len(feats[u]))
                match += (r["succeeded"], r["alignment"], r["words"], r["like"]) == (want["succeeded"], want["alignment"], want["words"],
                                                                                      want["like"]) and (res[u]["alignment"] == r["alignment"])
            out.update(checked_against_restatement=n, restatement_matches=match)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
