/* include/khg_hip.h -- C-ABI of the MI355X (gfx950) HMM-GMM EM hot path.
 *
 * Drop-in boundary for csukuangfj/kaldi-hmm-gmm's align + acc-stats + M-step path.  Every
 * entry point names the reference interface it replaces (paths relative to
 * /root/reference/kaldi-hmm-gmm/, "csrc/" = the core library, "python/csrc/" = the pybind11
 * layer a maintainer would bind these from).
 *
 * Conventions: plain pointers and sizes only; `_h` = host pointer, `_d` = device pointer;
 * every function returns 0 on success or a negative KHG_E_* code, with the message available
 * from khg_last_error() (thread-local).  Reference KHG_ERR / KHG_ASSERT (csrc/log.h:46-83,
 * std::runtime_error) map to KHG_E_RUNTIME.  Handles are opaque; work is stream-ordered on the
 * context's HIP stream; there is no hidden CPU fallback: without a usable GPU every compute
 * entry point fails with KHG_E_HIP.
 */
#ifndef KHG_HIP_H_
#define KHG_HIP_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KHG_OK 0
#define KHG_E_ARG (-1)      /* invalid argument / shape mismatch                              */
#define KHG_E_HIP (-2)      /* HIP runtime error (no device, OOM, launch failure)             */
#define KHG_E_RUNTIME (-3)  /* the reference would throw std::runtime_error here              */
#define KHG_E_UNSUPPORTED (-4)
/* largest feature dimension: a 64-frame chunk of rows must fit LDS next to a pdf's posteriors.  D <= 80 runs the MFMA
 * kernels; 80 < D <= KHG_MAX_DIM the vector-ALU forms of K1 and K3 (correct, not tuned). */
#define KHG_MAX_DIM 512

typedef struct khg_ctx khg_ctx;
typedef struct khg_model khg_model;
typedef struct khg_tm khg_tm;
typedef struct khg_utts khg_utts;
typedef struct khg_accs khg_accs;

const char *khg_last_error(void);
int khg_version(void);

/* ---- per-device context ------------------------------------------------------------- */
/* stream: a hipStream_t owned by the caller (e.g. torch's current stream) or NULL to let the
 * context create its own non-blocking stream. */
int khg_ctx_create(int device, void *stream, khg_ctx **out);
/* Waits for the context's streams.  Handles made on the context (models, tables, utterance sets, statistics blocks) may be destroyed
 * after it; their device memory stays valid until then (a statistics block can still be read through another context), and every
 * entry point that is given the destroyed context returns KHG_E_ARG. */
int khg_ctx_destroy(khg_ctx *ctx);
/* Waits for the stream and reports kernel-side errors deferred by the asynchronous entry points
 * (khg_loglikes, khg_align without host outputs, khg_acc_stats): KHG_E_RUNTIME where the reference
 * would have thrown (NaN/Inf log-likelihood, pdf-id out of range). */
int khg_ctx_sync(khg_ctx *ctx);
/* Measurement aid: when on, every kernel launch is bracketed by HIP events on the
 * context's stream; khg_ctx_get_timings drains (name, ms) pairs, names '\n'-separated. */
int khg_ctx_set_timing(khg_ctx *ctx, int on);
int khg_ctx_get_timings(khg_ctx *ctx, char *names, int64_t names_cap, float *ms, int32_t cap,
                        int32_t *n_out);

/* Which arithmetic K1 (khg_loglikes*) runs in.  All forms evaluate decodable-am-diag-gmm.cc:55-61 to fp32 accuracy
 * (|error| <= 1e-5 + 1e-6 B against an fp64 evaluation, B = |gconst| + sum |M x| + sum |V x^2| / 2; the reference's own
 * Eigen gemv fixes no summation order either):
 *   KHG_K1_F16X2S    (what AUTO selects; csrc/khg_k1_f16x2s.hip.inc) both operands rescaled per contraction index by an exact
 *                    power of two (feature columns and the largest weight column peak in [2^14, 2^15)) and split into two fp16
 *                    pieces v1 + v2, v1 = fp16(v), v2 = fp16(v - v1): 11 + 11 significant bits, |v - (v1 + v2)| <=
 *                    max(2^-23 |v|, 2^-25) in scaled units; the three partial products w1 x1, w1 x2, w2 x1 on
 *                    v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator (the dropped w2 x2 is <= 2^-22 of the term: worst case
 *                    2^-21 per term plus an absolute floor, measured 2.1e-7 B against fp64).  Used while the split forms'
 *                    common domain holds (max |gconst| + sum_k max |w_k| max |x_k| <= 2^28) and the floor, summed at the column
 *                    maxima, stays <= 2e-6; otherwise khg_loglikes runs KHG_K1_F16X2, then KHG_K1_FP32_PDF / _UTT, by itself;
 *   KHG_K1_F16X2     the same three products with the residual pieces pre-scaled by 2^11 (v = v1 + v2 2^-11: no subnormal
 *                    residuals, |v - (v1 + v2 2^-11)| <= 2^-23 |v|) and two accumulators (main + cross, combined by one fma per
 *                    Gaussian): worst case 2^-21 per term, measured error BELOW the fp32 chain's (profiles/r2_probe_f16x2.txt);
 *                    same common domain;
 *   (value 1, KHG_K1_BF16X3 of rounds 2-5 -- three exact bf16 pieces, six products -- was removed in round 6: KHG_E_ARG)
 *   KHG_K1_FP32_PDF / KHG_K1_FP32_UTT   fp32 MFMA (v_mfma_f32_16x16x4_f32), pdf-major / utterance-major tiling: bit for bit the
 *                    per-Gaussian chain s = gconst; s = fmaf(M[d], x[d], s) ...; s = fmaf(-V[d]/2, x[d]^2, s) ... in k order.
 * The environment variable KHG_K1 = f16x2s | f16x2 | pdf | utt seeds the setting at khg_ctx_create (A/B runs). */
#define KHG_K1_AUTO 0
#define KHG_K1_FP32_PDF 2
#define KHG_K1_FP32_UTT 3
#define KHG_K1_F16X2 4
#define KHG_K1_F16X2S 5
int khg_ctx_set_k1_form(khg_ctx *ctx, int form);     /* = khg_ctx_set_option(ctx, KHG_OPT_K1_FORM, form) */

/* Every switch of the library that is not an argument of an entry point: kernel forms and experiment knobs (what the reference
 * has no counterpart for -- its kernels are Eigen expressions).  Values are validated (KHG_E_ARG).  An option takes effect at the
 * next call that plans or launches the kernel it names; plans already built for an utterance set (chunk order, K1P slices) are
 * kept.  The environment variables in brackets only seed the defaults, once, at khg_ctx_create (A/B runs of an unmodified caller). */
#define KHG_OPT_K1_FORM 0        /* KHG_K1_* above                                                              [KHG_K1=f16x2s|f16x2|pdf|utt] */
#define KHG_OPT_K1_ORDER 1       /* launch order of K1 workgroups: 0 frame tiles x pdfs descending, 1 utterance order, 2 ascending,
                                    3 frame tiles descending, 4 the chunks of one utterance eight positions apart (one XCD)  [KHG_K1_ORDER=desc|none|asc|tiles|xcd] */
#define KHG_OPT_K1_NF 2          /* fp32 utterance-major K1: 16-frame tiles per wave at D <= 40 (0 = 6, or 5)     [KHG_K1_NF] */
#define KHG_OPT_K1P_TS 3         /* fp32 pdf-major K1: tiles per workgroup slice (default 1024)                  [KHG_K1P_TS] */
#define KHG_OPT_K1_INTERLEAVE 4  /* fp32 utterance-major K1: frame tiles dealt round-robin (-1 auto, 0, 1)        [KHG_K1_INTERLEAVE] */
#define KHG_OPT_K1_DBG 5         /* experiment bit mask (bits 1-8: the tile-major split forms, results may be WRONG; 16: no packing of
                                    small pdfs; 32 / 64: K1s band form without shifted tiles / 16-frame shift only)  [KHG_K1B_DBG] */
#define KHG_OPT_K2_INORDER 6     /* 1: K2 workgroups in utterance order instead of longest first                  [KHG_K2_INORDER] */
#define KHG_OPT_K2_KS 7          /* states per thread on K2's register-resident path: 0 auto, 2, 4; 3 = the general three-slot kernel also where the two-slot one applies [KHG_K2_KS] */
#define KHG_OPT_K2_SERIAL 8      /* 1: the one-lane order-faithful decoder also where the wave form applies;
                                    2: the wave form with its graph tables in HBM scratch also where they fit LDS;
                                    3: the general wave form also where the chain form (no epsilon arcs, <= 1000 states,
                                       out-degree <= 4) applies                                                      [KHG_K2_SERIAL] */
#define KHG_OPT_K2_PROF 9        /* 1: per-utterance cycle stamps of K2 to stderr                                 [KHG_K2_PROF] */
#define KHG_OPT_K3_BUCKET 10     /* frames by pdf: 0 stable radix sort of (pdf, frame) pairs (rocPRIM; reproducible sums), 1 atomic cursor scatter, 2 the library's own stable counting sort (same order as 0, slower) [KHG_K3_BUCKET=sort|atomic|count] */
#define KHG_OPT_K3_FORM 11       /* 0 auto, 1 the chunk-per-block MFMA form for every shape, 2 the VALU form      [KHG_K3_FORM=block, KHG_K3_VALU=1] */
#define KHG_OPT_K3_PHASE_B 12    /* gamma . x: 0 on the fp64 matrix pipe (exact products), 1 as 0 and, in the wave form, the fp32 phase A chain with it (the fp32-pipe form of rounds 3-5 was removed in round 6), 2 (DEFAULT) on the fp16 matrix cores (operands split into two fp16 pieces, 32-frame fp32 partial sums added in fp64; pdfs of 33..64 Gaussians, D <= 40, else as 0) [KHG_K3_PHASEB=f32|f16] */
#define KHG_OPT_K3_NY 13         /* workgroups per pdf in K3 (0 auto)                                             [KHG_K3_NY] */
#define KHG_OPT_DEBUG 14         /* 1: planning statistics to stderr                                              [KHG_DEBUG] */
#define KHG_OPT_K3_PHASE_A 15    /* per-Gaussian log-likelihoods of K3's wave form: 0 on the fp16 matrix cores in K1's f16x2s arithmetic where the model-derived scales hold, 1 the fp32 MFMA chain [KHG_K3_PHASEA=f32] */
#define KHG_OPT_K2_SPLIT 16      /* an asynchronous khg_align (no host outputs) on a set of > 64 utterances lets the order-faithful decoders write to a
                                    second alignment buffer, so that khg_acc_stats can accumulate the certified utterances while they still
                                    run and add the others in a second pass: 0 (DEFAULT) on, 1 off                       [KHG_K2_SPLIT=off] */
#define KHG_OPT_K2S_HUB 17       /* khg_decode_lattice_simple: a state with more than this many in-arcs (out-arcs in the backward pass) has its arc
                                    loops strided over by a whole wave instead of walked by one lane (a word loop's hub state); same results
                                    bit for bit.  0: off (every state on one lane).  Default 32                              [KHG_K2S_HUB] */
#define KHG_OPT_LAT_OPS_LDS 18   /* khg_lattices_best_path / khg_lattices_prune / khg_lattices_posteriors: 0 (DEFAULT) an utterance's lattice is staged into LDS when it takes
                                    at most 48 KiB there, 1 never (every lattice is read from its HBM arrays); same results bit for
                                    bit.  khg_lattices_oracle: 0 the rows of two frames are kept in LDS when they fit, 1 never (read
                                    back from the HBM table); khg_lattices_wer: 0 a table of at most 48 KiB stays in LDS, 1 never;
                                    same results bit for bit.  khg_lattices_nbest: 0 an utterance's running lists (52 n bytes) are
                                    kept in LDS when the device gives that much, 1 never (HBM rows); same results bit for
                                    bit                                                                              [KHG_LAT_OPS_LDS] */
#define KHG_OPT_K1_LAUNCH 19     /* launch shape of the default (f16x2s) K1: 1 one workgroup per chunk of frame tiles; 2 persistent -- one workgroup per
                                    CU takes chunks from a counter, in the same order, and copies the next chunk's frame tiles into LDS under
                                    the tail of the current one; 0 (DEFAULT) automatic: persistent where it measured faster, never for a small
                                    set or the packed small-pdf kernels; same scores bit for bit             [KHG_K1_LAUNCH=auto|chunk|persistent] */
#define KHG_OPT_K1_PGRID 20      /* persistent K1: at most this many workgroups (tests: more chunks than workgroups on a small set);
                                    0 (DEFAULT) as many as the chip holds at once, by the occupancy query                  [KHG_K1_PGRID] */
#define KHG_OPT_K1_PROF 21       /* 1: boundary stamps of every K1 chunk (entry, barrier, first / last wave out of work), summed per CU,
                                    to stderr; the call waits for the kernel                                              [KHG_K1_PROF] */
#define KHG_OPT_K2_LADDER 22     /* K2's exact DP on batches of chain-ordered graphs (every in-arc of state s from s or s - 1, <= 256 states): 0 (DEFAULT)
                                    the ladder form -- costs move between lanes in registers, one workgroup barrier per eight layers --, 1 the
                                    general body; same results bit for bit                                            [KHG_K2_LADDER=on|off] */
#define KHG_OPT_K3_PLANES 23     /* K3's wave form with both phases on the fp16 matrix cores (KHG_OPT_K3_PHASE_B = 2) reads the features as split fp16
                                    records kept on the utterance set (320 B per frame, made once per set and set of model-derived exponents)
                                    instead of splitting the raw features in every pass: 0 (DEFAULT) automatic -- where the records fit half of
                                    the free device memory at the first pass, never for a small set; 1 off; 2 on (still the in-loop split when
                                    the allocation fails); same statistics bit for bit                          [KHG_K3_PLANES=auto|off|on] */
#define KHG_OPT_K2_TAIL 24       /* the single-wave tail of K2's exact DP (trace-back and forward replay of the best path): 0 (DEFAULT) the trace-back
                                    decodes one packed source word per cell (in-degree <= 3, one state per thread, <= 256 states) and the
                                    replay's fp64 cost chain runs as a wave scan wherever that is exact, 1 the loops they replaced; same
                                    results bit for bit                                                                 [KHG_K2_TAIL=on|off] */
#define KHG_OPT_NBEST_ARENA 25   /* khg_lattices_nbest: the lists of the utterances of ONE launch may take this many KiB together (an utterance above it is a
                                    launch of its own); a chunk whose lists take more runs in several launches (tests: more than one launch on
                                    small lattices).  0 (DEFAULT): 1 GiB; same results bit for bit                          [KHG_NBEST_ARENA] */
#define KHG_OPT_COUNT 26
/* Read-only figures (khg_ctx_get_option only): the per-call scratch block behind small utterance sets (DESIGN.md "per-utterance calls"). */
#define KHG_INFO_SCRATCH_BYTES 100   /* bytes of the block in use (its top), 0 before the first small set */
#define KHG_INFO_SCRATCH_BLOCKS 101  /* live allocations inside it */
int khg_ctx_set_option(khg_ctx *ctx, int option, int value);
int khg_ctx_get_option(const khg_ctx *ctx, int option, int *value);
/* The validation behind khg_ctx_set_option, without a context (no device needed): KHG_OK or KHG_E_ARG. */
int khg_option_check(int option, int value);
/* What khg_ctx_create makes of the environment variable `name` when it is set to `text`: KHG_OK and the (option, value) it seeds, or
 * KHG_E_ARG -- no such variable, an unknown word, a value outside the option's range (khg_ctx_create then keeps the default). */
int khg_option_from_env(const char *name, const char *text, int *option, int *value);

/* ---- acoustic model ------------------------------------------------------------------- */
/* AmDiagGmm (csrc/am-diag-gmm.h:96) as flat ragged arrays: pdf p owns Gaussians
 * [gauss_off[p], gauss_off[p+1]) with DiagGmm's exponential-form parameters
 * (csrc/diag-gmm.h:243-256).  gconsts must be valid (khg_compute_gconsts).  Uploads the
 * MFMA tile image used by K1 and the row-major copy used by K3. */
int khg_model_create(khg_ctx *ctx, int32_t num_pdfs, int32_t dim, const int32_t *gauss_off_h,
                     const float *gconsts_h, const float *means_invvars_h,
                     const float *inv_vars_h, khg_model **out);
int khg_model_destroy(khg_model *m);
/* Measurement / consistency aid: drops what the handle caches PER PARAMETER VERSION -- the fp16 / bf16 K1 images, the BAND form's
 * per-pdf upper bounds, the column maxima and scale exponents -- as every in-place update (khg_model_mle_update, _split, _merge,
 * _scale_weights) does, without touching the parameters: the next khg_loglikes / khg_acc_stats derive them again.  One EM iteration of
 * the reference changes the parameters once (scripts/gmm_est.py:8-96), so a benchmark step that is to pay what a real iteration
 * pays calls this once per step (bench.py). */
int khg_model_invalidate(khg_model *m);

/* ---- transition information ------------------------------------------------------------ */
/* TransitionInformation::TransitionIdToPdf table (csrc/transition-information.h:71-73,
 * csrc/transition-model.cc:278-302): id2pdf_h[0..num_tids], entry 0 unused. */
int khg_tm_create(khg_ctx *ctx, int32_t num_tids, const int32_t *id2pdf_h, khg_tm **out);
/* AddTransitionProbs (csrc/hmm-utils.cc:465-493): trans_cost_h[tid] = -GetScaledTransitionLogProb
 * (:442-463), added to every arc carrying that tid when khg_align runs (the resident graphs keep
 * their base weights, as scripts/gmm_align_compiled.py:36-41 does on a copy per call).
 * NULL resets to "no transition probs added". */
int khg_tm_set_trans_cost(khg_tm *tm, const float *trans_cost_h);
int khg_tm_destroy(khg_tm *tm);

/* ---- utterances: features + decoding graphs, resident in HBM --------------------------- */
/* feats: [frame_off[n_utt]][dim] float32 row-major, either host (feats_h) or already on the
 * device (feats_d, borrowed: must outlive the handle).  Graphs: fst::VectorFst<StdArc> per
 * utterance (the `fst` argument of python/csrc/decoder-wrappers.cc:25-47) concatenated as CSR
 * by source state: utterance u owns states [state_off[u], state_off[u+1]); global state s owns
 * arcs [arc_off[s], arc_off[s+1]); nextstate is utterance-local; start_h[u] = -1 for an empty
 * FST; final_h[s] = +inf for non-final (TropicalWeight::Zero()).  Pass n_states_total = 0 and
 * NULL graph arrays for a features-only set (log-likes / acc-stats without alignment).
 * The reference's per-utterance calls (scripts/gmm_align_compiled.py:36-79, gmm_acc_stats_ali.py:46-58) become one set of ONE
 * utterance per call: a set of <= 16 utterances (<= 16 384 frames) takes all its device scratch from a per-context arena mirrored in
 * pinned host memory -- no hipMalloc / hipFree, its tables reach the device in one staged copy, khg_align's results come back in
 * one -- so create / khg_loglikes_reachable / khg_align / destroy of a 300-frame utterance is ~0.35 ms at 5000 x 64 x 40. */
int khg_utts_create(khg_ctx *ctx, const khg_tm *tm, int32_t n_utt, int32_t dim,
                    const int64_t *frame_off_h, const float *feats_h, const float *feats_d,
                    const int64_t *state_off_h, const int32_t *start_h, const int64_t *arc_off_h,
                    const int32_t *ilabel_h, const int32_t *olabel_h, const float *weight_h,
                    const int32_t *nextstate_h, const float *final_h, khg_utts **out);
int khg_utts_destroy(khg_utts *u);
/* ---- one decoding graph shared by many utterances ---------------------------------------
 * Decoding (egs/yesno/decode.py:143-179: one HCLG, one decoder object, every utterance) is the opposite of training: ONE graph,
 * many utterances.  khg_graph_create plans a graph once (in-arc CSR, pdf list, first / last useful frames) and uploads its tables
 * once; khg_utts_create_on_graph builds a set whose utterances all decode on it and that stores, per utterance, only what depends
 * on its length.  The graph is in the CSR-by-source layout of khg_utts_create for a single graph (arc_off_h[0] = 0, nextstate
 * graph-local, final_h[s] = +inf for non-final, start = -1 for an empty FST); argument checks as there.
 * Limits: khg_utts_create refuses a state with more than 254 incoming arcs and a graph of more than 65 535 states, which are the exact-DP
 * aligner's (one-byte back-pointers, 16-bit arc sources).  A khg_graph may exceed both: the lattice decoders take any in-degree and
 * any state count their scratch checks admit, and khg_align on such a set returns KHG_E_UNSUPPORTED naming the limit and leaves
 * the set usable.  More than 32 767 distinct pdfs on the graph: KHG_E_UNSUPPORTED, as in khg_utts_create.
 * Lifetime: every set holds a reference to its graph, so khg_graph_destroy before khg_utts_destroy is legal; the tables are freed
 * with the last holder.  Several live sets may share one graph.  A graph belongs to the context that created it (KHG_E_ARG from
 * khg_utts_create_on_graph otherwise); its tables are never taken from the per-context arena.  Every entry point that takes a
 * khg_utts works on such a set and gives the results of the same utterances on U copies of the graph, bit for bit. */
typedef struct khg_graph khg_graph;
int khg_graph_create(khg_ctx *ctx, const khg_tm *tm, int32_t num_states, int32_t start, const int64_t *arc_off_h,
                     const int32_t *ilabel_h, const int32_t *olabel_h, const float *weight_h,
                     const int32_t *nextstate_h, const float *final_h, khg_graph **out);
int khg_graph_destroy(khg_graph *g);
/* any output may be NULL; device_bytes: the graph tables in HBM (independent of how many utterances decode on it) */
int khg_graph_info(const khg_graph *g, int64_t *num_states, int64_t *num_arcs, int32_t *num_pdfs,
                   int32_t *max_in_degree, int64_t *device_bytes);
/* khg_utts_create with every utterance decoding on `g` (features as there) */
int khg_utts_create_on_graph(khg_ctx *ctx, const khg_tm *tm, khg_graph *g, int32_t n_utt, int32_t dim,
                             const int64_t *frame_off_h, const float *feats_h, const float *feats_d, khg_utts **out);
/* device bytes of graph tables this set owns itself: 0 for a set created on a khg_graph, and for a features-only set */
int khg_utts_graph_bytes(const khg_utts *u, int64_t *bytes);
/* number of distinct pdfs on each utterance's graph, and the list itself (sorted) */
int khg_utts_num_pdfs(const khg_utts *u, int64_t *pdf_off_h /* [n_utt+1] */);
int khg_utts_pdfs(const khg_utts *u, int32_t *pdfs_h /* [pdf_off[n_utt]] */);
/* What khg_align would launch for this set under the context's current options (read-only: launches and allocates nothing; for
 * tests): out = { KS, DEG, FAST, GMEM, SC -- the template arguments of the exact-DP kernel k2_viterbi_dp --, threads per block,
 * dynamic LDS bytes, order-faithful decoder for what the DP cannot certify: 0 one-lane LDS, 1 one-lane HBM, 2 wave LDS, 3 wave HBM,
 * 4 chain }.  The generic form is KS = DEG = 1, FAST = 0. */
int khg_utts_k2_plan(khg_ctx *ctx, const khg_utts *u, int32_t out[8]);
/* ... and whether it would run the ladder form of that kernel (KHG_OPT_K2_LADDER): *out = 1, else 0. */
int khg_utts_k2_ladder(khg_ctx *ctx, const khg_utts *u, int32_t *out);
/* After a khg_align under KHG_OPT_K2_PROF: per utterance, how many 64-entry batches of the exact DP's replay ran their cost chain as a
   wave scan (out[2 u]) and how many as the serial loop (out[2 u + 1]) -- KHG_OPT_K2_TAIL; zeros for an utterance the kernel left
   before its replay.  cap: int32 entries of out, >= 2 * utterances.  KHG_E_ARG without such a call. */
int khg_utts_k2_tail(const khg_utts *u, int32_t *out, int64_t cap);
/* K3's split feature records on the set (KHG_OPT_K3_PLANES): *bytes of the buffer (0: none), *packs = how often it was filled so far,
 * *used = 1 when the last khg_acc_stats pass read it.  Launches nothing. */
int khg_utts_k3_planes(const khg_utts *u, int64_t *bytes, int64_t *packs, int32_t *used);
/* The accumulate kernels of the statistics pass (K3), by variant: the wave form with the fp32 / fp64 phase B, the wave form with both
 * phases on the fp16 matrix cores splitting the features in its loop / reading the set's split feature records, the wave forms' fold
 * (k3_wave_finalize, launched behind each of them), the chunk-per-block fp32 + fp64 MFMA form, its fp16 form, the VALU form. */
#define KHG_K3V_WAVE 0
#define KHG_K3V_WAVE16 1
#define KHG_K3V_WAVE16P 2
#define KHG_K3V_FINALIZE 3
#define KHG_K3V_MFMA 4
#define KHG_K3V_BLOCK16 5
#define KHG_K3V_VALU 6
/* Every instantiation the pass can launch: rows[i] = { variant, KQ, Gaussian blocks, waves per block, POST, fp16 phase A } -- the
 * library's own table, for tests; needs no context and no device.  *n = the number of rows; rows == NULL: *n alone; cap: rows of 6
 * int32 that `rows` holds (KHG_E_ARG when fewer than *n). */
int khg_k3_forms(int32_t *rows, int32_t cap, int32_t *n);
/* What the LAST statistics pass over this set launched (khg_acc_stats -- in split mode its second pass --, khg_acc_stats_post /
 * _post2, the K3 pass of khg_acc_mllt_stats_post), written where the pass decided it: *nruns = 0 (before any pass, after a pass over
 * zero frames), 1, or 2 for a model whose pdfs go to two forms; per run out[i] = { variant, KQ, Gaussian blocks, waves per block,
 * POST, fp16 phase A, fp16 phase B, 1 when the split feature records were read, slices per pdf, cls_lo, cls_hi (the run takes the
 * pdfs of cls_lo < Gaussians <= cls_hi), dynamic LDS bytes }.  Launches nothing. */
int khg_utts_k3_last(const khg_utts *u, int32_t out[2][12], int32_t *nruns);
/* What the LAST khg_loglikes / _reachable / _band call on this set chose and launched (K1), written on the host from the call's plan
 * before anything is launched and cleared at the start of every such call (a call that fails leaves the form at NONE):
 *   out[0]  1 once a call was made (0: none yet, the rest is zero)
 *   out[1]  the form that ran: KHG_K1L_NONE (no frames or no pdfs: nothing launched), _F16X2S, _F16X2, _PDF, _UTT, _WIDE (D > 80)
 *   out[2]  the form the option asked for, same codes (KHG_K1_AUTO asks for f16x2s)
 *   out[3]  why earlier forms handed over, a bit mask: 1 outside the split forms' domain, 2 f16x2s: the common scale or the absolute
 *           part of its error bound (> 2e-6), 4 f16x2: no scaling fits fp16, 8 pdf-major: a pdf of more than 128 Gaussians
 *   out[4]  KS (5 / 10) of the split forms, KQ (10 / 20) of the fp32 forms, 0 for the wide form
 *   out[5]  cells: 0 all, 1 from a pdf's first needed tile on, 2 the band between its first and last needed tile
 *   out[6]  f16x2s: pdfs per MFMA tile (4 / 2 / 1); other forms 0
 *   out[7]  f16x2s: 1 when the persistent kernel ran;  out[8] workgroups of the main launch (pdf-major: summed over its launches)
 *   out[9]  work units planned (chunks -- the empty ones of order 4 included --, pdf-major: slices);  out[10] the cap a unit was cut to
 *           (32-frame tiles for the split forms, 16-frame tiles for the fp32 forms, frames for the wide form)
 *   out[11] the effective KHG_OPT_K1_ORDER of the split forms (4 when f16x2s chose it by itself)
 *   out[12] f16x2s: 1 when _reachable ran the shifted-tile form;  out[13] its shift mode (0 none, 1 sixteen frames only, 2 any)
 *   out[14] utterance-major: 16-frame tiles per wave;  out[15] 1 for its aligned loads;  out[16] 1 when tiles are dealt round-robin
 *   out[17 .. 24]  pdf-major: slices of the pdfs of 1 .. 8 blocks of sixteen Gaussians
 *   out[25] bit 1: this call packed the set's feature planes, bit 2: it packed the model's image
 *   out[26] 1 when khg_align's repair launch recomputed band scores since (cleared by the next khg_loglikes* call)
 * Launches nothing, copies nothing to or from the device. */
#define KHG_K1_LAST_WORDS 27
#define KHG_K1L_NONE 0
#define KHG_K1L_F16X2S 1
#define KHG_K1L_F16X2 2
#define KHG_K1L_PDF 3
#define KHG_K1L_UTT 4
#define KHG_K1L_WIDE 5
int khg_utts_k1_last(const khg_utts *u, int32_t out[KHG_K1_LAST_WORDS]);
/* per listed pdf: the first frame a decoder token can read it at (fewest emitting arcs from the start state
 * to an arc carrying it; INT32_MAX if never; 0 for sets without graphs) -- what khg_loglikes_reachable uses */
int khg_utts_pdf_first(const khg_utts *u, int32_t *first_h /* [pdf_off[n_utt]] */);

/* ---- K1: log-likelihoods --------------------------------------------------------------- */
/* DecodableAmDiagGmmUnmapped::LogLikelihoodZeroBased (csrc/decodable-am-diag-gmm.cc:29-71) for
 * every (frame, pdf on the utterance's graph); DiagGmm::LogLikelihood (csrc/diag-gmm.cc:150-165)
 * when a pdf list is given explicitly.  Result layout per utterance: ll[j * tpad + t],
 * tpad = T rounded up to 32, j = index into the utterance's pdf list.  KHG_E_RUNTIME if any
 * value is NaN/Inf (the reference throws, :63-65). */
int khg_loglikes(khg_ctx *ctx, const khg_model *m, khg_utts *u);
/* Same, restricted to the (frame, pdf) cells the decoder can read: DecodableAmDiagGmmScaled only
 * evaluates LogLikelihood(frame, tid) for tokens that exist (csrc/faster-decoder.cc:208), and no token
 * can sit in a state before as many frames as the fewest emitting arcs from the start state lead to
 * it.  Cells of a pdf before its first readable frame are unspecified (whole tiles in front of it are
 * left untouched, and a pdf's tiles may start at that very frame); alignments are identical to
 * khg_loglikes + khg_align.  Sets without graphs: same as khg_loglikes. */
int khg_loglikes_reachable(khg_ctx *ctx, const khg_model *m, khg_utts *u);
/* The BAND form: additionally leaves out what only tokens that can no longer reach a final state read -- a (pdf, 32-frame tile)
 * past the last frame at which an arc carrying the pdf still leads to a final state by the utterance's end (fewest emitting arcs
 * to a final state, khg_utts_pdf_last).  Those cells are FILLED with an upper bound of the pdf's log-likelihood, so the exact DP
 * of khg_align sees such tokens at costs no higher than the reference decoder would -- its beam certificate stays sound and the
 * best path is untouched.  An utterance whose certificate fails is recomputed without the band by khg_align itself before the
 * order-faithful decoder reads it: EVERY khg_align on these scores needs the model handle alive and at the parameter version the scores
 * were computed with -- a handle destroyed or updated in between makes khg_align return KHG_E_ARG (checked by handle serial and
 * version, never by dereferencing a stale pointer); a handle whose fp16 image was merely re-packed for another set's feature
 * exponents makes khg_align score the set again first.  Alignments are identical to khg_loglikes + khg_align at any beam.  Worth it when the beam is wide (few certificates fail): ~21 % fewer cells at
 * the benchmark's shape.  Cells of a pdf BEFORE its first readable frame are unspecified (as with khg_loglikes_reachable, here to
 * the frame: a band's 32-frame tiles may start at that frame instead of on the 32-frame grid).  Default K1 form only (f16x2s, pdfs
 * of more than 16 Gaussians); anything else: khg_loglikes_reachable. */
int khg_loglikes_band(khg_ctx *ctx, const khg_model *m, khg_utts *u);
/* per listed pdf: the last frame at which an arc carrying it can still lead to a final state by the utterance's end (-1: never;
 * INT32_MAX for sets without graphs) */
int khg_utts_pdf_last(const khg_utts *u, int32_t *last_h /* [pdf_off[n_utt]] */);
/* total floats of the resident ll buffer and per-utterance offsets [n_utt+1] */
int khg_loglikes_layout(const khg_utts *u, int64_t *ll_off_h, int64_t *total);
int khg_loglikes_download(khg_ctx *ctx, const khg_utts *u, float *ll_h);
/* test hook: overwrite the resident ll buffer (lets K2 be checked bit-exactly on given scores) */
int khg_loglikes_upload(khg_ctx *ctx, khg_utts *u, const float *ll_h);
/* features-only sets: give every utterance the same explicit pdf list */
int khg_utts_set_pdf_list(khg_utts *u, int32_t n, const int32_t *pdfs_h);
/* Borrowed device features (feats_d of khg_utts_create) are otherwise IMMUTABLE for the life of the handle: the default K1 keeps
 * per-set data derived from them (column maxima, fp16 planes packed once).  A caller that rewrites them in place calls this
 * before the next khg_loglikes; K3 and the fp32 K1 forms read feats_d live. */
int khg_utts_features_changed(khg_utts *u);

/* ---- K2: Viterbi forced alignment ------------------------------------------------------ */
typedef struct {
  float beam;        /* AlignConfig (csrc/decoder-wrappers.h:23-37): 200 */
  float retry_beam;  /* 0 */
  int32_t careful;   /* 0; careful alignment = graphs passed through khg_careful_graph by the caller before khg_utts_create */
  float acoustic_scale;
  /* FasterDecoderOptions (csrc/faster-decoder.h:24-49); AlignUtteranceWrapper keeps defaults */
  int32_t max_active; /* INT32_MAX */
  int32_t min_active; /* 20 */
  float beam_delta;   /* 0.5 */
  float hash_ratio;   /* 2.0 */
  /* divisor of `like` (decoder-wrappers.cc:95) when it differs from the scale the scores are multiplied by: the reference scales
   * scores inside the decodable (its own `scale`) and divides `like` by AlignUtteranceWrapper's acoustic_scale argument.
   * 0 = acoustic_scale (the scripts pass the same value for both). */
  float like_scale;
} khg_align_config;
void khg_align_config_default(khg_align_config *c);

/* per-utterance status bits */
#define KHG_ALIGN_DONE 0
#define KHG_ALIGN_ERROR 1     /* num_error++ (empty graph / no final state reached)            */
#define KHG_ALIGN_RETRIED 2   /* num_retried++                                                 */
#define KHG_ALIGN_EXACT_DP 4  /* info: produced by the exact-DP kernel under a beam certificate */
#define KHG_ALIGN_FALLBACK 8  /* info: produced by the order-faithful FasterDecoder kernel     */

/* ModifyGraphForCarefulAlignment (csrc/decoder-wrappers.cc:111-140: fst := Concat(fst, fst_rhs), fst_rhs = a copy of fst
 * without final weights, entered through a new final start state by an epsilon arc) on ONE graph in the CSR-by-source
 * layout of khg_utts_create (host arrays; nextstate graph-local).  OpenFst's Concat semantics: every final state s of the
 * left copy loses its final weight w and gains an epsilon arc (0:0 / w) to the right copy's start, appended after its own
 * arcs.  Result: 2 S + 1 states (left copy 0..S-1, right copy S..2S-1, the pre-initial state 2S, final with weight 0),
 * 2 A + 1 + (#final states) arcs; the caller sizes the output arrays for that ([2S+2] arc_off, [2A+1+S] arc arrays,
 * [2S+1] final).  An empty graph (num_states == 0) is returned unchanged.  Host only. */
int khg_careful_graph(int32_t num_states, int32_t start, const int64_t *arc_off_h, const int32_t *ilabel_h,
                      const int32_t *olabel_h, const float *weight_h, const int32_t *nextstate_h, const float *final_h,
                      int32_t *out_num_states, int32_t *out_start, int64_t *out_arc_off_h, int32_t *out_ilabel_h,
                      int32_t *out_olabel_h, float *out_weight_h, int32_t *out_nextstate_h, float *out_final_h);

/* AlignUtteranceWrapper (csrc/decoder-wrappers.cc:16-108) + FasterDecoder (csrc/faster-decoder.cc)
 * + DecodableAmDiagGmmScaled (csrc/decodable-am-diag-gmm.h:83-103) for every utterance of the
 * set.  Requires khg_loglikes() (or khg_loglikes_upload) first.  Outputs (host, may be NULL):
 *   ali_h[frame_off[n_utt]]  transition-ids, 0 for failed utterances
 *   words_h / words_off_h[n_utt+1]: olabels != 0 along the best path (words_cap = capacity)
 *   like_h[n_utt]   float `like` of decoder-wrappers.cc:95
 *   status_h[n_utt] KHG_ALIGN_* bits.
 * The alignment also stays resident on the device for khg_acc_stats.  With every host output NULL the call is asynchronous: the exact
 * DP runs on the context's stream, the order-faithful decoders for the utterances it could not certify on a side stream; on a set of
 * more than 64 utterances those write to a second alignment buffer that the next consumer merges (KHG_OPT_K2_SPLIT). */
int khg_align(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_align_config *cfg,
              int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
              float *like_h, int32_t *status_h);
/* replace the resident alignment (e.g. an initial equal-align, egs/yesno/train.py:86-108) */
int khg_ali_upload(khg_ctx *ctx, khg_utts *u, const int32_t *ali_h);
/* the resident alignment back (0 on the frames of utterances that failed to align) */
int khg_ali_download(khg_ctx *ctx, khg_utts *u, int32_t *ali_h);

/* ---- K2L: LatticeFasterDecoder + DecodeUtteranceLatticeFaster ------------------------------------------------------------------ */
typedef struct {
  /* LatticeFasterDecoderConfig (csrc/lattice-faster-decoder.h:45-105; pybind defaults python/csrc/lattice-faster-decoder.cc:20-31) */
  float beam;             /* 16 */
  int32_t max_active;     /* INT32_MAX */
  int32_t min_active;     /* 200 */
  float lattice_beam;     /* 10 */
  int32_t prune_interval; /* 25 */
  float beam_delta;       /* 0.5 */
  float hash_ratio;       /* 2 */
  float prune_scale;      /* 0.1 */
  /* DecodableAmDiagGmmScaled's scale (csrc/decodable-am-diag-gmm.h:83-103): the score read for (frame, tid) is
   * acoustic_scale * loglike(frame, id2pdf[tid]); 1 for scores that were scaled before khg_loglikes_upload */
  float acoustic_scale;   /* 1 */
  /* DecodeUtteranceLatticeFaster's allow_partial (csrc/decoder-wrappers.cc:200-211) */
  int32_t allow_partial;  /* 1 */
  /* forward-link / token scratch per utterance and frame.  0: min(num_states, 256) tokens and min(num_arcs, 1024) links per frame,
   * plus one frame's worth, and every utterance that runs out of that is decoded again with room for all states and arcs on every
   * frame (a frame never holds more), so only the queue / sort bounds can still give KHG_LAT_SCRATCH.  > 0: exactly that many
   * tokens and links per frame, no second pass; an utterance that runs out gets KHG_LAT_SCRATCH and no output */
  int32_t scratch_per_frame; /* 0 */
} khg_lattice_faster_config;
void khg_lattice_faster_config_default(khg_lattice_faster_config *c);

/* per-utterance status bits of khg_decode_lattice_faster */
#define KHG_LAT_SUCCEEDED 1  /* DecodeUtteranceLatticeFaster returned true: alignment, words and like are valid          */
#define KHG_LAT_PARTIAL 2    /* no final state reached (ReachedFinal() false); output only with allow_partial            */
#define KHG_LAT_SCRATCH 4    /* out of token / forward-link scratch (scratch_per_frame): decoding stopped, no output       */
#define KHG_LAT_NO_PATH 8    /* Decode() false: no token survived to the last frame (lattice-faster-decoder.cc:97)         */
#define KHG_LAT_EPS_LOOP 16  /* an epsilon cycle among one frame's tokens (TopSortTokens, :1004-1006)                      */
#define KHG_LAT_WORDS 32     /* more words on the best path than frames + states + 64: no output                          */
#define KHG_LAT_NO_TRACEBACK 64 /* GetBestPath failed after a successful Decode (decoder-wrappers.cc:213-215)             */

/* LatticeFasterDecoder::Decode (csrc/lattice-faster-decoder.cc:86-98) + GetBestPath (:101-192: GetRawLattice + OpenFst ShortestPath)
 * + DecodeUtteranceLatticeFaster (csrc/decoder-wrappers.cc:186-224) for every utterance of the set, each on a fresh decoder
 * (HashList size 1000, :36).  Requires khg_loglikes(), khg_loglikes_reachable() or khg_loglikes_upload first -- not
 * khg_loglikes_band, whose cells past the band hold bounds, not scores (KHG_E_ARG); the graphs' own weights are used (plus the
 * table's trans_cost when one is set, as in khg_align).  Outputs (host, may be NULL):
 *   ali_h[frame_off[n_utt]]  transition-ids of the best path, 0 where the utterance has no output
 *   words_h / words_off_h[n_utt+1]: olabels != 0 along the best path (words_cap = capacity)
 *   like_h[n_utt]   double `like` = -(Value1 + Value2) of the path's LatticeWeight (float sum), not divided by any scale
 *   status_h[n_utt] KHG_LAT_* bits.
 * Synchronous.  Does not touch the set's resident alignment. */
int khg_decode_lattice_faster(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_lattice_faster_config *cfg,
                              int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
                              double *like_h, int32_t *status_h);

/* ---- K2S: LatticeSimpleDecoder + DecodeUtteranceLatticeSimple --------------------------------------------------------------- */
typedef struct {
  /* LatticeSimpleDecoderConfig (csrc/lattice-simple-decoder.h:26-79; pybind defaults python/csrc/lattice-simple-decoder.cc:15-21) */
  float beam;             /* 16 */
  float lattice_beam;     /* 10 */
  int32_t prune_interval; /* 25 */
  float prune_scale;      /* 0.1 (interval pruning never changes the answer; kept for the reference's Check and ToString) */
  /* DecodableAmDiagGmmScaled's scale, as in khg_lattice_faster_config */
  float acoustic_scale;   /* 1 */
  /* DecodeUtteranceLatticeSimple's allow_partial (csrc/decoder-wrappers.cc:142-182): accepted and ignored -- Decode() is false
   * whenever no final state is live on the last frame, and the wrapper stops there (no partial output) */
  int32_t allow_partial;  /* 1 */
  /* the most live tokens one frame may hold: an utterance with a frame over it gets KHG_LAT_SCRATCH and no output.  0: no limit
   * (the per-frame rows are dense, so an utterance never runs out) */
  int32_t scratch_per_frame; /* 0 */
} khg_lattice_simple_config;
void khg_lattice_simple_config_default(khg_lattice_simple_config *c);

/* further status bits of khg_decode_lattice_simple (with KHG_LAT_SUCCEEDED, _SCRATCH, _NO_PATH, _EPS_LOOP, _WORDS, _NO_TRACEBACK,
 * which mean here: _NO_PATH Decode() false, no final state live on the last frame (lattice-simple-decoder.cc:160-164), or no start
 * state (start < 0; the reference asserts start_state != kNoStateId, :52);
 * _EPS_LOOP a negative-cost epsilon cycle, on which the reference's ProcessNonemitting never ends; _NO_TRACEBACK also a zero-frame
 * utterance whose start closure is final: GetRawLattice's KHG_ASSERT(num_frames > 0), "Check failed!" (:680)) */
#define KHG_LAT_NO_EPS_TOKEN 128 /* "Error in ProcessNonEmitting: no surviving tokens: frame is <err_frame>" (:95-101)       */
#define KHG_LAT_NAN 256          /* a NaN forward link reached PruneForwardLinks' KHG_ASSERT (:261): "Check failed!"       */

/* LatticeSimpleDecoder::Decode (csrc/lattice-simple-decoder.cc:144-165) + GetBestPath (:644-735: GetRawLattice + OpenFst
 * ShortestPath) + DecodeUtteranceLatticeSimple (csrc/decoder-wrappers.cc:142-182) for every utterance of the set, each on a fresh
 * decoder.  Scores as for khg_decode_lattice_faster (KHG_E_ARG for khg_loglikes_band).  Outputs (host, may be NULL) as there, plus
 *   err_frame_h[n_utt]  the frame of KHG_LAT_NO_EPS_TOKEN's message (-1 at InitDecoding), -1 otherwise.
 * Synchronous.  Does not touch the set's resident alignment. */
int khg_decode_lattice_simple(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_lattice_simple_config *cfg,
                              int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
                              double *like_h, int32_t *status_h, int32_t *err_frame_h);

/* ---- K2R: the raw lattice of the lattice-simple decoder ------------------------------------------------------------------------ */
/* The raw lattices of one batch, resident on the device: what LatticeSimpleDecoder::GetRawLattice (csrc/lattice-simple-decoder.cc:
 * 654-735) builds as an fst::VectorFst<LatticeArc> per utterance, as flat arrays.  The reference's lattice depends on the order its
 * unordered_maps are walked in; this is the order-independent one (a subset of every walk's, equal to it whenever the walk kept no
 * emitting link of cost >= its frame's fl(best + beam)):
 *   states  one per (frame f in 0..T, graph state s) whose token survived FinalizeDecoding, numbered by frame, then by graph state
 *           (:684-690); each carries frame, graph_state, tot_cost, extra_cost, final_cost (+inf unless f == T and s is final, :723-733)
 *           and arc_begin, the index of its first arc among the utterance's (its arcs end where the next state's begin)
 *   arcs    one per surviving forward link (:700-722), per state in the order of the graph's arcs in that state: ilabel (the
 *           transition-id, 0 for epsilon), olabel, graph_cost (with the table's trans_cost when one is set), acoustic_cost (0 for
 *           epsilon), nextstate (a state number of the same utterance)
 *   start   the state of (0, graph start); -1 for an empty lattice
 * An utterance whose status lacks KHG_LAT_SUCCEEDED has an empty lattice (GetRawLattice is only reached when Decode() is true). */
typedef struct khg_lattices khg_lattices;

/* khg_decode_lattice_simple (same arguments, same outputs) that also keeps the raw lattice of every utterance (GetRawLattice, :654-735)
 * in *out: emitted on the device from the decoder's rows, while they are alive, with one more synchronisation per <= 4 GiB chunk of
 * scratch slices.  An utterance whose lattice has more than 2^31 - 1 states or arcs: KHG_E_ARG, naming it.  Scores from
 * khg_loglikes_band are refused (KHG_E_ARG).  Free *out with khg_lattices_destroy. */
int khg_decode_lattice_simple_raw(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_lattice_simple_config *cfg,
                                  int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
                                  double *like_h, int32_t *status_h, int32_t *err_frame_h, khg_lattices **out);
/* NumStates / the arc count of every utterance's lattice (:684-690, :700-722) as offsets into the flat arrays:
 * state_off_h[n_utt + 1], arc_off_h[n_utt + 1] (either may be NULL) */
int khg_lattices_sizes(const khg_lattices *l, int64_t *state_off_h, int64_t *arc_off_h);
/* the lattices to host arrays (any may be NULL): per state (state_off[n_utt] entries) frame, graph_state, tot_cost, extra_cost,
 * final_cost (Final(s).Value1(), :723-733; +inf: not final), arc_begin; per arc (arc_off[n_utt] entries) ilabel, olabel, graph_cost,
 * acoustic_cost, nextstate (:700-722); per utterance start (SetStart, :691-692).  Synchronous. */
int khg_lattices_download(khg_ctx *ctx, const khg_lattices *l, int32_t *frame_h, int32_t *graph_state_h, float *tot_cost_h,
                          float *extra_cost_h, float *final_cost_h, int32_t *arc_begin_h, int32_t *ilabel_h, int32_t *olabel_h,
                          float *graph_cost_h, float *acoustic_cost_h, int32_t *nextstate_h, int32_t *start_h);
/* device bytes the handle owns */
int khg_lattices_device_bytes(const khg_lattices *l, int64_t *bytes);
int khg_lattices_destroy(khg_lattices *l);

/* ---- K2F: the raw lattice of the lattice-faster decoder ------------------------------------------------------------------------- */
/* khg_decode_lattice_faster (same arguments, same outputs) that also keeps the raw lattice of every utterance in *out: what
 * LatticeFasterDecoder::GetRawLattice (csrc/lattice-faster-decoder.cc:101-192) builds, the FST whose best path the call returns.  An
 * ordinary khg_lattices handle (khg_lattices_sizes / _download / _device_bytes / _best_path / _prune / _num_chunks / _chunk_utts):
 *   states  one per token that survives FinalizeDecoding, numbered by frame, then in TopSortTokens order inside the frame with the
 *           gaps removed (its unordered_map walked in creation order, its reprocess set in insertion order); each carries frame,
 *           graph_state (the graph state the token was created for), tot_cost (Token::tot_cost as stored: cost offsets included),
 *           extra_cost (after the final pruning), final_cost (last frame: final_costs_[tok], +inf without an entry, 0 on every token
 *           when no final state was reached -- KHG_LAT_PARTIAL with allow_partial; +inf before the last frame) and arc_begin
 *   arcs    one per surviving forward link, per state in the link list's order (head first: the link made last comes first): ilabel,
 *           olabel, graph_cost (with the table's trans_cost when one is set), acoustic_cost (fl(link.acoustic_cost -
 *           cost_offsets[frame]) for an emitting link, 0 for an epsilon link), nextstate
 *   start   state 0; -1 for an empty lattice
 * Unlike K2R's, this lattice is not independent of order: it is the one of the order-faithful decoder (HashList order as the
 * reference's, the two TopSortTokens choices above).  It is acyclic and top-sorted.  An utterance whose status lacks
 * KHG_LAT_SUCCEEDED has an empty lattice and keeps its status.  Emitted on the device from the decoder's scratch slices while they are
 * alive, with one more synchronisation per <= 4 GiB launch of slices; the handle's chunks are the first pass's launches (a chunk
 * holding utterances of the second pass -- scratch_per_frame = 0 -- is gathered on the device from both passes' blocks).  An utterance
 * whose lattice has more than 2^31 - 1 states or arcs: KHG_E_ARG, naming it.  Free *out with khg_lattices_destroy. */
int khg_decode_lattice_faster_raw(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_lattice_faster_config *cfg,
                                  int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
                                  double *like_h, int32_t *status_h, khg_lattices **out);

/* ---- K2O: best path under scales and beam pruning of resident lattices ---------------------------------------------------------- */
/* A handle from host arrays, in the layout khg_lattices_download writes: state_off_h / arc_off_h [n_utt + 1], the six per-state and
 * five per-arc arrays, start_h[n_utt].  Every utterance is checked (KHG_E_ARG names the utterance and the check): one arc_begin per
 * state running from 0, monotone, within the arcs; states ordered by frame; nextstate in range; start in range (-1 for an empty
 * lattice) and on frame 0; an emitting arc (ilabel != 0) goes from frame f to frame f + 1, an epsilon arc stays in its frame.
 * khg_lattices_validate runs the checks alone (no device).  Free *out with khg_lattices_destroy. */
int khg_lattices_validate(int32_t n_utt, const int64_t *state_off_h, const int64_t *arc_off_h, const int32_t *frame_h,
                          const int32_t *graph_state_h, const float *tot_cost_h, const float *extra_cost_h, const float *final_cost_h,
                          const int32_t *arc_begin_h, const int32_t *ilabel_h, const int32_t *olabel_h, const float *graph_cost_h,
                          const float *acoustic_cost_h, const int32_t *nextstate_h, const int32_t *start_h);
int khg_lattices_upload(khg_ctx *ctx, int32_t n_utt, const int64_t *state_off_h, const int64_t *arc_off_h, const int32_t *frame_h,
                        const int32_t *graph_state_h, const float *tot_cost_h, const float *extra_cost_h, const float *final_cost_h,
                        const int32_t *arc_begin_h, const int32_t *ilabel_h, const int32_t *olabel_h, const float *graph_cost_h,
                        const float *acoustic_cost_h, const int32_t *nextstate_h, const int32_t *start_h, khg_lattices **out);
/* the number of utterances of a handle; the layout of khg_lattices_best_path's alignments: ali_off_h[n_utt + 1], utterance u owns
 * ali_off_h[u + 1] - ali_off_h[u] = the frame of its last state (0 for an empty lattice) entries of every pair's row */
int khg_lattices_num_utts(const khg_lattices *l, int32_t *n_utt);
int khg_lattices_ali_layout(khg_ctx *ctx, const khg_lattices *l, int64_t *ali_off_h);
/* the launches (chunks of at most 4 GiB of decoder scratch) the handle's lattices were emitted in: a handle from khg_lattices_upload
 * has one (none when it has no utterance), a pruned handle its input's.  first_utt_h[n_chunks + 1]: the first utterance of every
 * chunk, n_utt last.  Every operation runs once per chunk.  Read-only, no device work. */
int khg_lattices_num_chunks(const khg_lattices *l, int32_t *n_chunks);
int khg_lattices_chunk_utts(const khg_lattices *l, int32_t *first_utt_h);
/* lattice-scale | lattice-best-path for n_scales (graph_scale, acoustic_scale) pairs in one call (finite, >= 0; else KHG_E_ARG): an
 * arc weighs (fl(graph_scale * graph_cost), fl(acoustic_scale * acoustic_cost)), a final state (fl(graph_scale * final_cost), 0), and
 * the best path is OpenFst ShortestPath by the decoder kernel's tie rule (float, no contraction; at (1, 1) the decoder's own path).
 * Outputs (host, may be NULL), pair k, utterance u at index k * n_utt + u:
 *   ali_h[n_scales][sum over utterances of the last state's frame]   the path's transition-ids by frame, 0 without a path
 *   words_h / words_off_h[n_scales * n_utt + 1]  its olabels != 0 (words_cap = capacity; an entry that does not fit gets KHG_LAT_WORDS
 *                                                and no words)
 *   weight_h[n_scales * n_utt][2]  the path's two sums, float, left to right from One(), the final weight last (+inf without a path)
 *   status_h[n_scales * n_utt]     KHG_LAT_SUCCEEDED, or KHG_LAT_NO_PATH (an empty lattice, no final state reached), KHG_LAT_EPS_LOOP
 *                                  (a negative-cost epsilon cycle under these scales), KHG_LAT_WORDS
 * Synchronous.  The handle's lattices are not changed. */
int khg_lattices_best_path(khg_ctx *ctx, const khg_lattices *l, int32_t n_scales, const float *graph_scale, const float *acoustic_scale,
                           int32_t *ali_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap, float *weight_h, int32_t *status_h);
/* lattice-prune under one scale pair: a new handle with the states and arcs whose best path through them costs at most
 * fl(best + beam) (beam >= 0, +inf allowed), plus the best path itself; states and arcs keep their order, nextstate / start are
 * renumbered, every cost is copied as stored (unscaled).  An utterance without a path (KHG_LAT_NO_PATH) or with a negative epsilon
 * cycle (KHG_LAT_EPS_LOOP) gets an empty lattice.  status_h[n_utt] (may be NULL).  Synchronous; the input is untouched. */
int khg_lattices_prune(khg_ctx *ctx, const khg_lattices *l, float graph_scale, float acoustic_scale, float beam, int32_t *status_h,
                       khg_lattices **out);
/* LatticeForwardBackward / lattice-to-post under one scale pair (finite, >= 0; else KHG_E_ARG), all in float64: an
 * arc's log-likelihood is -(graph_scale * graph_cost + acoustic_scale * acoustic_cost) (no acoustic term on an epsilon arc), a final
 * state's -graph_scale * final_cost on the last frame.  *out is a new handle resident on the device (free it with
 * khg_posteriors_destroy) holding every arc's posterior in the lattice handle's arc order and, per frame t in 0 .. T - 1, the
 * posteriors of the emitting arcs that leave frame t merged by ilabel (the transition-id), ascending; an id is listed unless every
 * arc behind it is unreachable from one side (a weight that underflows to 0.0 stays listed).
 *   status_h[n_utt]    KHG_LAT_SUCCEEDED; KHG_LAT_EPS_LOOP: an epsilon arc that does not go to a higher state number (the
 *                      lattice-simple decoder's lattices have such self-loops); KHG_LAT_NO_PATH: empty, or no final state reached.
 *                      An utterance without KHG_LAT_SUCCEEDED has no frames and no entries, and its arc posteriors are 0.
 *   tot_like_h[n_utt]  log of the sum over all paths; -inf without KHG_LAT_SUCCEEDED.
 * The first call on a handle builds its in-arc index on the device and keeps it there.  Synchronous; the input is untouched. */
typedef struct khg_posteriors khg_posteriors;
int khg_lattices_posteriors(khg_ctx *ctx, const khg_lattices *l, float graph_scale, float acoustic_scale, int32_t *status_h,
                            double *tot_like_h, khg_posteriors **out);
/* frame_off_h / entry_off_h [n_utt + 1]: utterance u owns frames frame_off[u] .. frame_off[u + 1] and entries entry_off[u] .. */
int khg_posteriors_sizes(const khg_posteriors *p, int64_t *frame_off_h, int64_t *entry_off_h);
/* entry_begin_h[frames + 1] (frame f owns entries entry_begin[f] .. entry_begin[f + 1]), tid_h / weight_h [entries],
 * arc_post_h [arcs of the lattice handle, its arc order]; any may be NULL */
int khg_posteriors_download(khg_ctx *ctx, const khg_posteriors *p, int64_t *entry_begin_h, int32_t *tid_h, double *weight_h,
                            double *arc_post_h);
int khg_posteriors_device_bytes(const khg_posteriors *p, int64_t *bytes);
int khg_posteriors_destroy(khg_posteriors *p);
/* A handle from host arrays -- the ones khg_posteriors_sizes (frame_off_h[n_utt + 1]) and khg_posteriors_download
 * (entry_begin_h[frames + 1], absolute; tid_h / weight_h [entry_begin_h[frames]]) give back: how ali-to-post, weight-silence-post and
 * hand-made posteriors get in.  The handle has no arc posteriors; an utterance without frames counts as KHG_LAT_NO_PATH, every other
 * as KHG_LAT_SUCCEEDED.  The ids of a frame may come in any order and may repeat; the handle records the largest.  Refused with
 * KHG_E_ARG (khg_posteriors_validate, host only: n_entries = the length of tid_h / weight_h): frame_off_h or entry_begin_h not
 * starting at 0 or decreasing, entry_begin_h not ending at n_entries, an id < 1, a weight that is not finite (any sign is taken).
 * Synchronous. */
int khg_posteriors_validate(int32_t n_utt, const int64_t *frame_off_h, const int64_t *entry_begin_h, int64_t n_entries,
                            const int32_t *tid_h, const double *weight_h);
int khg_posteriors_upload(khg_ctx *ctx, int32_t n_utt, const int64_t *frame_off_h, const int64_t *entry_begin_h,
                          const int32_t *tid_h, const double *weight_h, khg_posteriors **out);

/* ---- K2X: rescoring and boosting resident lattices (gmm-rescore-lattice, lattice-boost-ali) ------------------------ */
/* Both operations return a NEW handle, as khg_lattices_prune does: the input is untouched, the result is an ordinary khg_lattices
 * with the input's chunks.  If the input has its in-arc index (khg_lattices_posteriors made it) and no utterance was emptied, the
 * index is copied: the structure is the same. */
#define KHG_LAT_NO_REF 512       /* the utterance has nothing to be compared with: khg_lattices_boost -- no alignment (length 0, a
                                    failed utterance), an alignment whose length is not the lattice's frame count or that holds an id
                                    outside 1 .. num_tids; khg_lattices_rescore FROM_LL -- an arc names a pdf that is not on the
                                    utterance's pdf list.  Its lattice in the result is EMPTY */
#define KHG_RESCORE_CELLS 0      /* scores computed from the set's features and the model, for the distinct (frame, pdf) cells the
                                    lattices name and nothing else: no resident ll buffer, no graph needed (a features-only set works) */
#define KHG_RESCORE_FROM_LL 1    /* scores gathered from the set's resident ll buffer (khg_loglikes, _reachable, _upload; not _band) */
typedef struct { int64_t arcs, emitting_arcs, cells; } khg_rescore_stats;   /* arcs of the input; those with ilabel != 0; the distinct
                                    (feature row, pdf) cells among them.  The last two are counted by the CELLS pipeline (FROM_LL: 0) */
/* gmm-rescore-lattice.  Every arc with ilabel != 0 of a non-empty lattice of utterance u, leaving a state of frame t:
 *   acoustic_cost := -(acoustic_scale * ll(u, t, id2pdf[ilabel]))        one float multiply and a sign
 * Epsilon arcs keep their acoustic_cost; ilabel, olabel, graph_cost, nextstate, every per-state array and start are copied as stored
 * (tot_cost / extra_cost are the decoder's diagnostics under the OLD scores: stale, and no operation reads them).  acoustic_scale = 1
 * gives Kaldi's unscaled costs; the caller then takes khg_lattices_posteriors(1, kappa).
 * KHG_RESCORE_CELLS: ll is the fp32 log-sum-exp over the pdf's Gaussians of the chain s = gconst; then, for d in steps of two,
 * s = fmaf(M[d], x[d], s); s = fmaf(M[d+1], x[d+1], s); s = fmaf(-V[d]/2, fl(x[d]^2), s); s = fmaf(-V[d+1]/2, fl(x[d+1]^2), s) --
 * the strict-fp32 K1's (KHG_K1_FP32_PDF) per-Gaussian value bit for bit -- reduced in a fixed order that depends on the pdf's number of
 * Gaussians only: a cell's value depends on (feature row, pdf, model) and on nothing else (not on the batch, not on the lattice).
 * |error| <= 1e-5 + 1e-6 B against fp64, as every K1 form.  Arcs that share a cell get the same bits.  A NaN / Inf value:
 * KHG_E_RUNTIME.  An ilabel outside 1 .. num_tids: KHG_E_RUNTIME (pdf-id out of range).
 * KHG_RESCORE_FROM_LL: ll is read from the resident buffer, ll[j * tpad + t] with j found by binary search in the utterance's sorted
 * pdf list; an utterance with an arc whose pdf is not listed gets KHG_LAT_NO_REF and an empty lattice.
 * KHG_E_ARG before anything is launched (naming the utterance where there is one): a handle of another context; n_utt differing
 * between set and lattices; a non-empty lattice whose frame count (khg_lattices_ali_layout) is not the set's for that utterance;
 * model / set dimension mismatch; a transition table that names pdfs the model lacks; non-finite acoustic_scale; unknown mode;
 * FROM_LL without resident scores, or with khg_loglikes_band's.
 * stats (may be NULL): host counts, on the synchronisation the call has anyway (cells: CELLS mode only, else 0).  Synchronous. */
int khg_lattices_rescore(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, const khg_lattices *l,
                         float acoustic_scale, int mode, khg_rescore_stats *stats, khg_lattices **out);
/* Per-utterance KHG_LAT_* bits of the khg_lattices_rescore / khg_lattices_boost / khg_lattices_lm_rescore call that made `l`
 * (status_h[n_utt]): KHG_LAT_SUCCEEDED, KHG_LAT_NO_PATH for an utterance whose input lattice was empty, KHG_LAT_NO_REF; from
 * khg_lattices_lm_rescore also KHG_LAT_EPS_LOOP, KHG_LAT_LM_OOV, KHG_LAT_SCRATCH.  A handle made otherwise: KHG_E_ARG. */
int khg_lattices_op_status(const khg_lattices *l, int32_t *status_h);
/* lattice-boost-ali (Kaldi's LatticeBoost).  Every arc with ilabel != 0 leaving a state of frame t of utterance u, with
 * ref = tid2phone[ali[u][t]] and ph = tid2phone[ilabel]:  e = 0 if ph == ref; max_silence_error if ph != ref and ph is a silence phone;
 * 1 otherwise;  graph_cost := fl(graph_cost + fl(-b * e)).  Everything else is copied.  tid2phone_h[num_tids + 1] (entry 0 unused).
 * The alignment: EITHER host arrays (ali_off_h[n_utt + 1], ali_h[ali_off_h[n_utt]]) OR, both NULL, ali_set -- the alignment the last
 * khg_align / khg_ali_upload left resident in that set (same context, same n_utt).  Anything else: KHG_E_ARG.
 * status_h[n_utt] (may be NULL): KHG_LAT_SUCCEEDED; KHG_LAT_NO_PATH for an empty input (stays empty); KHG_LAT_NO_REF (above; such an
 * utterance gets an EMPTY lattice, as lattice-boost-ali skips it).
 * KHG_E_ARG: non-finite b or max_silence_error, a lattice ilabel above num_tids, a silence phone that no id maps to.
 * Boosting changes graph costs only: it commutes with rescoring and is done once, after the decode.  Synchronous. */
int khg_lattices_boost(khg_ctx *ctx, const khg_lattices *l, int32_t num_tids, const int32_t *tid2phone_h,
                       int32_t n_sil, const int32_t *silence_phones_h, const int64_t *ali_off_h, const int32_t *ali_h,
                       const khg_utts *ali_set, float b, float max_silence_error, int32_t *status_h, khg_lattices **out);

/* ---- K2N: rescoring resident lattices with a backoff n-gram language model (lattice-lmrescore) -------------------- */
/* The LM is a deterministic backoff automaton in flat arrays.  States 0 .. n_states - 1 are histories, state 0 the empty one:
 *   backoff_h[n_states]       backoff_h[0] = -1; for h > 0, 0 <= backoff_h[h] < h (every backoff chain ends in state 0)
 *   backoff_cost_h[n_states]  the cost of taking that step (entry 0 is unused but finite)
 *   arc_begin_h[n_states + 1] state h owns arcs arc_begin_h[h] .. arc_begin_h[h + 1]; from 0, monotone
 *   word_h / cost_h / next_h [arc_begin_h[n_states]]   word > 0, strictly ascending inside a state; cost = -ln P; next a state
 *   final_cost_h[n_states]    the cost of the sentence end from h, already resolved through the backoff chain
 *   start                     the state of the history <s>
 * Every float is finite.  khg_lm_validate (host only) checks all of this; KHG_E_ARG names the state or arc and the check.
 * advance(h, w), w > 0, all float, one rounding per addition:  c = +0; search w among the arcs of h (binary); found: c = fl(c + cost),
 * the result is (next, c); else h == 0: w is out of vocabulary; else c = fl(c + backoff_cost[h]), h = backoff[h], search again. */
typedef struct khg_lm khg_lm;
int khg_lm_validate(int32_t n_states, const int32_t *backoff_h, const float *backoff_cost_h, const int32_t *arc_begin_h,
                    const int32_t *word_h, const float *cost_h, const int32_t *next_h, const float *final_cost_h, int32_t start);
/* khg_lm_validate, then the arrays to the device.  The handle belongs to `ctx`.  Synchronous.  Free it with khg_lm_destroy. */
int khg_lm_create(khg_ctx *ctx, int32_t n_states, const int32_t *backoff_h, const float *backoff_cost_h, const int32_t *arc_begin_h,
                  const int32_t *word_h, const float *cost_h, const int32_t *next_h, const float *final_cost_h, int32_t start,
                  khg_lm **out);
int khg_lm_destroy(khg_lm *lm);
int khg_lm_num_states(const khg_lm *lm, int32_t *n_states);
int khg_lm_device_bytes(const khg_lm *lm, int64_t *bytes);
/* Host only: the cost of the sentence words_h[n_words] (<s> implied, the sentence end added).  h = start, t = +0; per word
 * (h, c) = advance(h, w), t = fl(t + c); at the end t = fl(t + final_cost[h]).  The arrays are validated first.  KHG_E_ARG for a word
 * <= 0 or out of vocabulary, naming its position. */
int khg_lm_score(int32_t n_states, const int32_t *backoff_h, const float *backoff_cost_h, const int32_t *arc_begin_h,
                 const int32_t *word_h, const float *cost_h, const int32_t *next_h, const float *final_cost_h, int32_t start,
                 int32_t n_words, const int32_t *words_h, float *cost_out);
#define KHG_LAT_LM_OOV 1024      /* khg_lattices_lm_rescore: a reachable arc carries a word the LM does not have.  EMPTY lattice */
typedef struct { int64_t in_states, in_arcs, out_states, out_arcs, max_hist; } khg_lm_rescore_stats;   /* states and arcs of the
                                    input and of the result; the largest |H(s)| among the utterances that succeeded */
/* lattice-lmrescore: a NEW handle (the input is untouched; the result keeps the input's chunks, as khg_lattices_prune's does) in
 * which every state is split by LM history and every arc with a word carries fl(scale * the LM's cost of the word) more graph cost.
 * scale is finite, of either sign: -1 removes an LM whose costs the graph costs hold.  Per utterance, in this order:
 *   empty input                                 KHG_LAT_NO_PATH, stays empty
 *   an arc that does not go to a higher state   KHG_LAT_EPS_LOOP, empty (the lattice-simple decoder's lattices; those of the
 *                                               lattice-faster decoder and what prune / rescore / boost make of them are admissible)
 *   H(start) = {lm start}; for the states d in ascending order H(d) = the set of h' over the in-arcs (s -> d, olabel w) and the
 *   h in H(s): h' = h when w == 0, else the state of advance(h, w).  Sorted ascending, unique.
 *   a word out of vocabulary among them         KHG_LAT_LM_OOV, empty (an arc that leaves an unreachable state is never looked at)
 *   the sets of the states 0 .. d together hold more than min(hist_factor * states, 2^31 - 1) entries: KHG_LAT_SCRATCH, empty (the
 *                                               decoders' convention: call again with a larger hist_factor)
 *   otherwise                                   KHG_LAT_SUCCEEDED
 * Result: for old s ascending, for h in H(s) ascending, one state (a state with an empty H -- unreachable -- is dropped) with
 * frame, graph_state, tot_cost, extra_cost of s (the last two stale, as after khg_lattices_rescore) and final_cost +inf where s has
 * +inf, else fl(final_cost + fl(scale * lm final_cost[h])).  Its arcs are the arcs of s in their order: ilabel, olabel and
 * acoustic_cost copied, nextstate the new number of (d, h'), graph_cost copied when olabel == 0, else fl(graph_cost + fl(scale * c)),
 * c from advance.  start: the new number of (start, lm start).  The result is top-sorted, as the input was.
 * status_h[n_utt], stats (either may be NULL); khg_lattices_op_status answers for the handle.  An utterance whose result has more
 * than 2^31 - 1 states or arcs: KHG_E_ARG.  KHG_E_ARG before anything is launched: a handle or LM of another context, a scale that
 * is not finite, hist_factor < 1.  The first call on a handle builds its in-arc index (as khg_lattices_posteriors does) and keeps it.
 * Synchronous: one synchronisation per chunk sizes the output. */
int khg_lattices_lm_rescore(khg_ctx *ctx, const khg_lattices *l, const khg_lm *lm, float scale, int32_t hist_factor,
                            int32_t *status_h, khg_lm_rescore_stats *stats, khg_lattices **out);

/* ---- K2D: determinizing resident lattices (lattice-determinize-pruned) ------------------------------------------- */
typedef struct {
  int64_t in_states, in_arcs;      /* of the input */
  int64_t pruned_states;           /* of X, the beam-pruned input (every utterance that reached step 2) */
  int64_t det_states;              /* determinized states D, summed over the utterances that succeeded */
  int64_t out_states, out_arcs;    /* of the result */
  int64_t max_subset, max_closure; /* the largest |K| and the largest closure among the utterances that succeeded */
} khg_det_stats;
/* lattice-determinize-pruned: a NEW, ordinary handle in which, under the pair (graph_scale, acoustic_scale), every word sequence of
 * the beam-pruned input has exactly ONE path, the cheapest one it has there, and every arc is a copy of an input arc (a path costs in
 * the result, bit for bit, what it costs in the input).  No compact lattice and no string repository: every input state s is split
 * by the determinized states D whose closure holds it, and an element (D, s) keeps its single best in-arc.
 * Everything is float, one rounding per operation, no contraction.  A weight is a pair (a, b); (a, b) is BETTER than (a', b') when
 * fl(a + b) < fl(a' + b'), or they are equal and a < a' (khg_lattices_best_path's order).  An arc weighs (fl(gs * graph_cost),
 * fl(as * acoustic_cost)), the second 0 on an arc with ilabel 0, as for best_path; sums are taken component by component.
 * Per utterance, in this order:
 *   empty input                                 KHG_LAT_NO_PATH, stays empty
 *   an arc that does not go to a higher state   KHG_LAT_EPS_LOOP, empty (as khg_lattices_lm_rescore)
 *   1. X = khg_lattices_prune(l, gs, as, beam); without a path its status (KHG_LAT_NO_PATH), empty.  T = the frame of X's last state.
 *   2. An ARRIVAL is a set I = {s -> cost}.  Normalise: subtract, component by component, the best cost of I (ties: the lowest s).
 *      Closure, over the states s of X in ascending number: the incumbent of s is its normalised initial cost if it has one; then every
 *      in-arc of s with olabel == 0 whose source p is in the closure is tried in ascending arc number, its candidate being
 *      (fl(E[p].a + w.a), fl(E[p].b + w.b)); a candidate replaces the incumbent only when BETTER (always when there is none).  A state
 *      with an incumbent is in the closure: E[s], and pred[s] = the arc that gave it, or "external".  An initial state whose pred is an
 *      arc is DOMINATED.  K = the other initial states ascending, R = their E.  The arrival IS the lowest-numbered D with the same K and
 *      fabs(fl(R_i.a - R'_i.a)) <= delta and the same for .b, for every i; otherwise it becomes a new D, the next number, which keeps
 *      K, R, E and pred.
 *   3. D0 = the arrival of {start: (0, 0)}.  For the D in ascending number: every arc (p -> dest, olabel w != 0) of the closure states
 *      p, ascending arc number, is a candidate fl(E[p] + weight) for (w, dest), kept only when BETTER than the one kept before.  For
 *      w ascending, the kept {dest -> cost} is an arrival D'; for each of its dest that is not dominated the kept arc becomes the
 *      arc (D, p) -> (D', dest) of the result.
 *      Scratch: the elements (D, s) of all closures together number more than min(state_factor * states(X), 2^31 - 1), or their
 *      states' arcs more than min(state_factor * arcs(X), 2^31 - 1): KHG_LAT_SCRATCH, empty (call again with a larger state_factor).
 *   4. Per D, the closure state of frame T with a final cost that has the best (fl(E[s].a + fl(gs * final_cost)), E[s].b) (ties: the
 *      lowest s) keeps its final_cost; every other element's becomes +inf.
 *   5. Y: one state per element, ordered by (s, D); frame, graph_state, tot_cost, extra_cost of s (the last two stale).  The arcs of
 *      (D, p) are those arcs of p, in p's order, that are kept: one with olabel == 0 iff pred_D[dest] is that arc (to (D, dest)), one
 *      with a word iff step 3 made it.  Fields copied, nextstate renumbered.  start = (start, D0).  Y is top-sorted.
 *   6. The result is khg_lattices_prune(Y, gs, as, beam): it trims the dead ends and the finals that lost.  KHG_LAT_SUCCEEDED.
 * graph_scale / acoustic_scale as for khg_lattices_prune; beam and delta finite and >= 0; state_factor >= 1; otherwise KHG_E_ARG.
 * status_h[n_utt], stats (either may be NULL); khg_lattices_op_status answers for the handle.  The result does not depend on the
 * batch and repeats from run to run.  Synchronous: the two prunes and one synchronisation per chunk that sizes Y. */
int khg_lattices_determinize(khg_ctx *ctx, const khg_lattices *l, float graph_scale, float acoustic_scale, float beam, float delta,
                             int32_t state_factor, int32_t *status_h, khg_det_stats *stats, khg_lattices **out);

/* ---- K2W: scoring resident lattices (lattice-add-penalty, lattice-oracle, score.sh's sweep, compute-wer) ---------- */
/* lattice-add-penalty: a NEW handle, as khg_lattices_prune and khg_lattices_boost return one (the input is untouched; the chunks, the
 * device offsets and the in-arc index go along).  Every arc with olabel != 0 gets graph_cost := fl(graph_cost + word_ins_penalty), one
 * float add; every other field is copied (tot_cost / extra_cost are then stale, as after khg_lattices_rescore).  The penalty is finite,
 * of either sign; otherwise KHG_E_ARG.  An empty lattice stays empty.  Synchronous. */
int khg_lattices_add_penalty(khg_ctx *ctx, const khg_lattices *l, float word_ins_penalty, khg_lattices **out);
/* lattice-oracle: per utterance the path of the lattice with the fewest word errors against a reference, by a dynamic program over
 * (lattice state, reference position).  ref_h / ref_off_h[n_utt + 1]: the reference words of utterance u are
 * ref_h[ref_off_h[u] .. ref_off_h[u + 1]), every word > 0 (an empty reference is legal).  The costs of the arcs are ignored.
 * THE RULE.  R is the reference's length; E[s][q], q = 0 .. R, is an int32; values >= INF = 2^30 mean unreachable, and a candidate from
 * an unreachable cell is skipped.  The states are visited in ascending number.  For a state s:
 *   C[s][q] = INF, except 0 at (start, 0).
 *   Every in-arc is tried in ascending arc number (source state, then arc: the in-arc index's order); it comes from p with olabel w:
 *     w == 0:             the candidate E[p][q]                                   (move EPS)
 *     w != 0, q >= 1:     first the candidate E[p][q-1] + (w != ref[q-1])         (move DIAG)
 *     w != 0:             then the candidate E[p][q] + 1                          (move INS: a word of the lattice the reference lacks)
 *     a candidate replaces the incumbent only when strictly smaller.
 *   Then for q = 1 .. R ascending E[s][q] = min(C[s][q], E[s][q-1] + 1), the deletion (move DEL) taken only when strictly smaller
 *   (E[s][0] = C[s][0]).
 * The end state is the final state -- as khg_lattices_best_path takes final states: a state of the last frame with final_cost != +inf --
 * with the least E[f][R]; the lowest state number wins ties.  The trace-back follows the recorded moves to (start, 0):
 *   words = the path's olabels != 0; ali = its ilabels != 0, by the frame of the arc's source; substitutions = DIAG moves with a
 *   mismatch, insertions = INS moves, deletions = DEL moves, errors = their sum = E[f][R].
 * The split into insertions, deletions and substitutions among paths and alignments of equal errors is THIS rule's; the total is unique.
 * Outputs (host; any may be NULL):
 *   counts_h[n_utt][4]   errors, insertions, deletions, substitutions
 *   words_h / words_off_h[n_utt + 1] / words_cap   khg_lattices_best_path's convention, KHG_LAT_WORDS included
 *   ali_h                khg_lattices_ali_layout's layout: the oracle path's transition-ids by frame, 0 without a path
 *   status_h[n_utt]      KHG_LAT_SUCCEEDED; KHG_LAT_NO_PATH: the lattice is empty or no final state is reachable; KHG_LAT_EPS_LOOP: an arc
 *                        does not go to a higher state number (the lattice-simple decoder's epsilon self-loops: the refusal of
 *                        khg_lattices_posteriors and khg_lattices_lm_rescore); KHG_LAT_SCRATCH: the utterance's own table --
 *                        8 * states * (R + 1) bytes -- exceeds scratch_bytes.  With any of these three the counts are (R, 0, R, 0) and
 *                        there are no words, so that sums over a set mean what compute-wer --mode=all means.
 * scratch_bytes: the tables of one launch stay within it (a chunk is split into as many launches as that takes); 0: 1 GiB.
 * The rows of the current frame and the one before are kept in LDS when they fit, unless KHG_OPT_LAT_OPS_LDS = 1; same results bit for bit.
 * KHG_E_ARG before any launch: n_utt is not the handle's utterance count; scratch_bytes < 0; a reference word <= 0 (naming the
 * utterance); an utterance with states + R >= 2^29, or with more than 2^31 - 4 arcs.  The first call on a handle builds its in-arc
 * index (as khg_lattices_posteriors does) and keeps it.  Synchronous; the input is untouched. */
int khg_lattices_oracle(khg_ctx *ctx, const khg_lattices *l, int32_t n_utt, const int32_t *ref_h, const int64_t *ref_off_h,
                        int64_t scratch_bytes, int32_t *counts_h, int32_t *words_h, int64_t *words_off_h, int64_t words_cap,
                        int32_t *ali_h, int32_t *status_h);
/* score.sh's sweep in one call: for n_points triples (graph_scale, acoustic_scale, word_ins_penalty) -- scales finite and >= 0, the
 * penalty finite -- the best path as khg_lattices_best_path finds it, with w1 = fl(fl(graph_scale * graph_cost) + word_ins_penalty) on
 * the arcs with olabel != 0 (scale first, then penalty: the order of lattice-scale | lattice-add-penalty), and then the edit distance of
 * the path's words against the reference by khg_edit_distance's rule, all on the device.  Only the counts come back:
 *   counts_h[n_points * n_utt][4], nwords_h[n_points * n_utt] (the hypothesis's length), status_h[n_points * n_utt] (best_path's);
 *   entry k * n_utt + u is point k of utterance u.  An utterance without a path counts as an empty hypothesis: (R, 0, R, 0).
 * At penalty 0 the words scored are khg_lattices_best_path's at the same pair; at graph_scale 1 they are those of
 * khg_lattices_add_penalty(p) followed by khg_lattices_best_path(1, acoustic_scale).  References as for khg_lattices_oracle.  Synchronous. */
int khg_lattices_wer(khg_ctx *ctx, const khg_lattices *l, int32_t n_utt, const int32_t *ref_h, const int64_t *ref_off_h, int32_t n_points,
                     const float *graph_scale, const float *acoustic_scale, const float *word_ins_penalty, int32_t *counts_h,
                     int32_t *nwords_h, int32_t *status_h);
/* compute-wer's core, host only (no context, no device): counts_h[n_pairs][4] = errors, insertions, deletions, substitutions of
 * hyp_h[hyp_off_h[i] .. hyp_off_h[i + 1]) against ref_h[ref_off_h[i] .. ref_off_h[i + 1]).  The rule is khg_lattices_oracle's on the
 * chain of the hypothesis words: per cell DIAG, then INS, then DEL, a candidate winning only when strictly better -- so the oracle of a
 * single-path lattice and the edit distance of that path give the same four counts.  KHG_E_ARG: a NULL array, offsets that do not
 * start at 0 or decrease, a pair whose lengths reach 2^29 together. */
int khg_edit_distance(int32_t n_pairs, const int32_t *ref_h, const int64_t *ref_off_h, const int32_t *hyp_h, const int64_t *hyp_off_h,
                      int32_t *counts_h);

/* ---- K2B: minimum Bayes risk decoding and word confidences of resident lattices (lattice-mbr-decode, the confidence column of
 *      lattice-to-ctm-conf: Kaldi's MinimumBayesRisk) ------------------------------------------------------------- */
#define KHG_LAT_NOT_CONVERGED 2048 /* khg_lattices_mbr: max_iter updates were made and the next one would still change the hypothesis;
                                      set together with KHG_LAT_SUCCEEDED, the outputs are those of the last accumulation */
/* Per utterance: the hypothesis of least expected word error under one (graph_scale, acoustic_scale) pair (as for
 * khg_lattices_posteriors), a confidence per word, and the confusion bins ("sausages").  All arithmetic is float64.
 * decode_mbr == 0: one accumulation on the initial hypothesis (confidences only).  max_iter >= 0 bounds the updates.
 * init_h / init_off_h[n_utt + 1] / init_given_h[n_utt]: the initial hypothesis of utterance u is init_h[init_off_h[u] ..
 * init_off_h[u + 1]) (words > 0; empty is legal) when init_off_h is not NULL and init_given_h is NULL or init_given_h[u] != 0;
 * otherwise it is the words of khg_lattices_best_path at the same pair (none when that finds no path).
 * THE RULE.
 * Weights.  alpha, tot and the arc log-likelihood w_a are khg_lattices_posteriors' (DESIGN.md 7g).  For every arc a: s -> d with
 *   alpha[s] finite (and alpha[d], which follows when the costs are finite) p_a = exp((alpha[s] + w_a) - alpha[d]); otherwise p_a = 0.
 *   For every final state f of the last frame with alpha[f] finite pf_f = exp((alpha[f] + fin_f) - tot); otherwise 0.  A virtual end
 *   state N (the real states are 0 .. N - 1) has one in-arc per state f of the last frame, ascending, with word 0 and weight pf_f.  An
 *   arc of weight 0 is skipped everywhere below.  The weights are the ONLY place where exp enters; everything after them is +, *, <
 *   and <= on doubles in the written order, without contraction.
 * Hypothesis.  The words h_1 .. h_W are normalised to r(1 .. Q), Q = 2 W + 1: r(q) = 0 (epsilon) for odd q, r(2 i) = h_i.
 *   sub(w, x) = 0 if w == x else 1;  del(w) = 0 if w == 0 else 1 + 1e-5 (Kaldi's delta);  ins(x) = 0 if x == 0 else 1.
 * Forward.  AD[n][0 .. Q], the states in ascending order.  AD[start][0] = 0, AD[start][q] = AD[start][q-1] + ins(r(q)); every other
 *   row starts at 0.  For each in-arc of n in the in-arc index's order (ascending arc number), with source s, word w and weight p:
 *     arc[0] = AD[s][0] + del(w);  for q >= 1:  a1 = AD[s][q-1] + sub(w, r(q)),  a2 = AD[s][q] + del(w),  a3 = arc[q-1] + ins(r(q));
 *     b[q] = 1 if a1 <= a2 and a1 <= a3;  b[q] = 2 if a2 < a1 and a2 <= a3;  otherwise b[q] = 3;  arc[q] is the chosen value;
 *     then AD[n][q] = fl(AD[n][q] + fl(p * arc[q])) for every q.
 *   The virtual state N comes last.  bayes_risk = AD[N][Q].
 * Backward.  BD is 0 except BD[N][Q] = 1; gamma[q][word], q = 1 .. Q, is 0.  The states go N down to 0 without the start; a state's
 *   in-arcs in ascending order; the arc row and b are recomputed from AD.  With ba[Q+1] = 0, for q = Q .. 1:
 *     ba[q] = (b[q+1] == 3 ? ba[q+1] : 0) + p * BD[n][q];
 *     b[q] == 1: BD[s][q-1] += ba[q], gamma[q][w] += ba[q];   b[q] == 2: BD[s][q] += ba[q];   b[q] == 3: gamma[q][0] += ba[q].
 *   Finally ba[0] = (b[1] == 3 ? ba[1] : 0) + p * BD[n][0] and BD[s][0] += ba[0].  A cell BD[s][q] can receive two additions from
 *   one arc: first the move-1 term from q + 1, then the move-2 term from q.  After all states the start row is drained:
 *   for q = Q .. 1, ba[q] = ba[q+1] + BD[start][q] and gamma[q][0] += ba[q].
 * Update.  pick(q) is the word of largest gamma[q][.], the lowest word id among equals (epsilon is 0); h' is the picks that are not 0,
 *   in order.  If decode_mbr == 0 or h' == h: stop.  If max_iter updates have been made: stop with KHG_LAT_NOT_CONVERGED.  If h' is
 *   longer than the cap: KHG_LAT_WORDS.  Otherwise h = h' and the rule repeats from Hypothesis.  The outputs always belong to the
 *   last accumulation.  The cap on W is max_words if > 0, else max(the initial hypothesis's length, the greatest number of words on
 *   any path from the start to a final state of the last frame: an int32 pass over the states); at most 2047 either way.
 * Statuses.  KHG_LAT_NO_PATH and KHG_LAT_EPS_LOOP exactly as khg_lattices_posteriors gives them; then KHG_LAT_WORDS: the initial
 *   hypothesis (or a later one) is longer than the cap, or the cap is above 2047; then KHG_LAT_SCRATCH: the utterance's table --
 *   8 * (2 * (states + 1) + len(vocab)) * (2 * cap + 2) bytes -- exceeds scratch_bytes (0: 1 GiB; the tables of one launch stay within
 *   it, as for khg_lattices_oracle); otherwise KHG_LAT_SUCCEEDED, with KHG_LAT_NOT_CONVERGED beside it where that applies.  An
 *   utterance without KHG_LAT_SUCCEEDED has no words and no table, and bayes_risk = +inf.
 * The result is a handle resident on the device (free it with khg_mbr_destroy).  khg_mbr_sizes: words_off_h / vocab_off_h /
 * gamma_off_h [n_utt + 1], any may be NULL -- utterance u owns words (and confidences) words_off[u] .. words_off[u + 1], vocabulary
 * entries vocab_off[u] .. and table cells gamma_off[u] .. .  khg_mbr_download (any output may be NULL): status_h / iters_h (the
 * number of updates made) / bayes_risk_h [n_utt]; words_h and conf_h (conf[i] = gamma[2 i][h_i]); vocab_h: the utterance's distinct
 * olabels ascending with 0 first; gamma_h: per utterance gamma[Q][len(vocab)], dense, row q - 1 for position q; arc_cond_h [arcs, the
 * lattice handle's arc order] and final_cond_h [states]: the weights p_a and pf_f that were used (0 for a refused utterance).
 * Handing the weights back is part of the interface: the rule takes an arg-min at every (arc, position) and an arg-max at every
 * position, expected distances cluster at integers, and one ulp in a weight can move a tie; so the device form and the host form
 * (Lattice::Mbr) agree BIT FOR BIT given the same weights, and only the weights are compared under a tolerance.
 * Nothing depends on the batch, on scratch_bytes or on timing: no atomics.
 * Cost: the vocabulary of an utterance is found by one wave with a scan that is quadratic in the utterance's arcs that carry a word
 * (1.4 ms for 2000 utterances of 167 arcs); on lattices of about 10^4 arcs that step dominates the call.
 * KHG_E_ARG before any launch: scales not finite or negative; max_iter < 0; max_words outside 0 .. 2047; scratch_bytes < 0; n_utt
 * not the handle's utterance count; init_off_h not starting at 0 or decreasing; an initial word <= 0 (naming the utterance).  The
 * first call on a handle builds its in-arc index (as khg_lattices_posteriors does) and keeps it.  Synchronous; the input is untouched. */
typedef struct khg_mbr khg_mbr;
int khg_lattices_mbr(khg_ctx *ctx, const khg_lattices *l, float graph_scale, float acoustic_scale, int32_t decode_mbr,
                     int32_t max_iter, int32_t n_utt, const int32_t *init_h, const int64_t *init_off_h, const int32_t *init_given_h,
                     int32_t max_words, int64_t scratch_bytes, khg_mbr **out);
int khg_mbr_sizes(const khg_mbr *m, int64_t *words_off_h, int64_t *vocab_off_h, int64_t *gamma_off_h);
int khg_mbr_download(khg_ctx *ctx, const khg_mbr *m, int32_t *status_h, int32_t *iters_h, double *bayes_risk_h, int32_t *words_h,
                     double *conf_h, int32_t *vocab_h, double *gamma_h, double *arc_cond_h, double *final_cond_h);
int khg_mbr_device_bytes(const khg_mbr *m, int64_t *bytes);
int khg_mbr_destroy(khg_mbr *m);

/* ---- K2N: the n best paths of resident lattices (lattice-to-nbest | nbest-to-linear) ---------------------------- */
#define KHG_NBEST_MAX 1024
/* The n cheapest paths of every utterance under the pair (graph_scale, acoustic_scale) = (gs, as), each with its alignment, its words,
 * its weight pair and its total.  On a handle made by khg_lattices_determinize every word sequence has one path, so the entries are
 * the n best DISTINCT word sequences (Kaldi's n-best on a CompactLattice); on a raw lattice they are the n best alignments.  The
 * reference has no n-best code: this text is the specification.
 * Everything is float, one rounding per operation, no contraction.  gs and as finite and >= 0, 1 <= n <= KHG_NBEST_MAX; otherwise
 * KHG_E_ARG.  Per utterance, in this order:
 *   empty lattice                               KHG_LAT_NO_PATH, 0 entries
 *   an arc that does not go to a higher state   KHG_LAT_EPS_LOOP, 0 entries (the test of khg_lattices_lm_rescore and _determinize; it
 *                                               refuses the lattices of the lattice-simple decoder)
 *   An arc weighs wa = fl(gs * graph_cost) and wb = fl(as * acoustic_cost), wb = 0 on an arc with ilabel 0 (as in
 *   khg_lattices_best_path); its scalar cost is c = fl(wa + wb).
 *   A PREFIX at state s is (t, a, b, nw, e, j): t the ordering key, (a, b) the two sums khg_lattices_best_path reports, nw the words so
 *   far, e the in-arc it came through (the utterance's arc number), j its rank in the list of e's source.  The list of the start
 *   state is the one prefix (0, 0, 0, 0, none, 0); the in-arcs of the start are not looked at (their sources lie below it, and nothing
 *   reaches them).  For every other state s, ascending: every in-arc e of s, from p, and every rank j of A[p] give the candidate
 *   t' = fl(A[p][j].t + c), a' = fl(a + wa), b' = fl(b + wb), nw' = nw + (olabel != 0); a candidate whose t' is not < +inf is dropped
 *   (NaN and +inf); A[s] is the n least candidates under the key (t', e, j), lexicographic, ascending (floats compare as floats:
 *   -0 == +0), fewer when there are fewer.
 *   T = the frame of the last state.  Every state s of frame T with a finite final_cost, and every rank j of A[s], give a complete
 *   path: total = fl(t + fw), fw = fl(gs * final_cost), dropped unless < +inf; weight (fl(a + fw), b).  The ENTRIES are the n least
 *   under (total, s, j), ascending.  None: KHG_LAT_NO_PATH; otherwise KHG_LAT_SUCCEEDED with 1 to n entries.
 *   An utterance whose lists together hold more than 2^31 - 1 elements: KHG_LAT_SCRATCH, 0 entries.
 * Two facts make this the right rule.
 *   1. A scalar key survives rounding: x <= y implies fl(x + c) <= fl(y + c).  So a state's list extended along an arc is still sorted
 *      under (t', j), cutting every list at n loses nothing, and the sorted totals of the result are EXACTLY the n least totals over all
 *      paths, each total taken left to right (tested with ==).  The pair order of khg_lattices_best_path -- fl(a + b), then a -- does
 *      not have this property after a component-wise add; that is why the key is the scalar t and the pair is only carried.
 *   2. The result is a function of the lattice alone: the key (t', e, j) is total, so it does not matter in which order arcs are
 *      merged; a serial loop that sorts (Lattice::Nbest) and the device's parallel merge by rank give the same lists, bit for bit.
 * Entry 0 is the best path under t, NOT under khg_lattices_best_path's pair order.  The two can differ only when two paths lie within
 * the accumulated rounding of each other; when entry 0 is best_path's path, its weight pair is best_path's bit for bit (the same sums
 * in the same order).
 * An entry's outputs, laid out as khg_lattices_best_path's: its non-zero ilabels by frame (T of them: the ilabel of the arc leaving
 * a state of frame f at position f, 0 where the path has none), its non-zero olabels, its weight pair, its total.
 * The result is a handle resident on the device (free it with khg_nbest_destroy); khg_lattices_op_status is not involved, the status
 * comes back through status_h [n_utt] (may be NULL).  khg_nbest_sizes: entry_off_h [n_utt + 1] -- utterance u owns the entries
 * entry_off[u] .. entry_off[u + 1] -- and words_off_h [entries + 1]; either may be NULL.  The alignments follow from
 * khg_lattices_ali_layout (T_u = ali_off[u + 1] - ali_off[u]) and the entry counts: entry k of utterance u owns the T_u cells from
 * sum over v < u of (entry_off[v + 1] - entry_off[v]) * T_v, plus k * T_u.  khg_nbest_download: ali_h, words_h, weight_h [entries][2],
 * total_h [entries]; any may be NULL.
 * The running lists of an utterance live in LDS (52 n bytes), or in HBM rows when the device gives less or KHG_OPT_LAT_OPS_LDS = 1:
 * the same bits.  Nothing depends on the batch or on timing: no atomics.  The first call on a handle builds its in-arc index (as
 * khg_lattices_posteriors does) and keeps it.  Synchronous: one synchronisation per chunk sizes the lists, one per launch sizes the
 * entries, and one ends the launch before its lists are freed (a chunk is one launch unless its lists exceed 1 GiB, or
 * KHG_OPT_NBEST_ARENA KiB when that is set). */
typedef struct khg_nbest khg_nbest;
int khg_lattices_nbest(khg_ctx *ctx, const khg_lattices *l, float graph_scale, float acoustic_scale, int32_t n, int32_t *status_h,
                       khg_nbest **out);
int khg_nbest_sizes(const khg_nbest *nb, int64_t *entry_off_h, int64_t *words_off_h);
int khg_nbest_download(khg_ctx *ctx, const khg_nbest *nb, int32_t *ali_h, int32_t *words_h, float *weight_h, float *total_h);
int khg_nbest_device_bytes(const khg_nbest *nb, int64_t *bytes);
int khg_nbest_destroy(khg_nbest *nb);

/* ---- K2M: MPE / sMBR posteriors of resident lattices (lattice-to-mpe-post, lattice-to-smbr-post) ------------------- */
#define KHG_MPE_MPFE 0           /* an arc is correct when its phone is the reference's at that frame */
#define KHG_MPE_SMBR 1           /* ... when its pdf is (needs tid2pdf_h) */
/* LatticeForwardBackwardMpeVariants under one (graph_scale, acoustic_scale) pair.  The likelihood part -- statuses, tot_like_h, which
 * arcs are live, the frames and ids listed -- is khg_lattices_posteriors', bit for bit.  Beside it runs the expected frame accuracy:
 * acc(arc) = 1 where the arc's class (phone or pdf of its ilabel) is the class of the reference id of its frame and, with
 * one_silence_class == 0, the arc's phone is no silence phone; with one_silence_class != 0 also where both phones are silence phones.
 * avg_acc_h[n_utt]: the expected accuracy of a path (0 without KHG_LAT_SUCCEEDED).  The handle's arc values and weights are SIGNED:
 * d(arc) = posterior(arc) * (expected accuracy of the paths through the arc - avg_acc); a frame's weights sum to zero.  Feed it to
 * khg_acc_stats_post2.  tid2phone_h / tid2pdf_h [num_tids + 1] (entry 0 unused; tid2pdf_h may be NULL for KHG_MPE_MPFE).  The
 * reference is given as khg_lattices_boost takes it, and KHG_LAT_NO_REF applies under the same three conditions; such an utterance has
 * no frames and no entries, tot_like = -inf and avg_acc = 0 (the input handle is untouched: nothing is emptied).
 * KHG_E_ARG before anything is launched: khg_lattices_boost's and khg_lattices_posteriors' refusals, an unknown criterion,
 * KHG_MPE_SMBR without tid2pdf_h.  Synchronous. */
int khg_lattices_mpe_posteriors(khg_ctx *ctx, const khg_lattices *l, int32_t num_tids, const int32_t *tid2phone_h,
                                const int32_t *tid2pdf_h, int32_t n_sil, const int32_t *silence_phones_h,
                                const int64_t *ali_off_h, const int32_t *ali_h, const khg_utts *ali_set, int32_t criterion,
                                int32_t one_silence_class, float graph_scale, float acoustic_scale, int32_t *status_h,
                                double *tot_like_h, double *avg_acc_h, khg_posteriors **out);

/* ---- K3: sufficient statistics ---------------------------------------------------------- */
/* AccumAmDiagGmm (csrc/mle-am-diag-gmm.h:93-96) + transition stats (csrc/transition-model.h:176-189)
 * as ONE contiguous fp64 device buffer (a single RCCL all-reduce sums it across GPUs =
 * AccumAmDiagGmm::Add, csrc/mle-am-diag-gmm.cc:119-128):
 *   [ occ: sumG | mean_acc: sumG*dim | var_acc: sumG*dim | trans_acc: num_tids+1 |
 *     total_frames, total_log_like, 6 spare ]                                                  */
int khg_accs_create(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_accs **out);
int khg_accs_destroy(khg_accs *a);
int khg_accs_zero(khg_ctx *ctx, khg_accs *a);
int khg_accs_size(const khg_accs *a, int64_t *num_doubles);
int khg_accs_device_ptr(const khg_accs *a, void **ptr_d);
int khg_accs_download(khg_ctx *ctx, const khg_accs *a, double *buf_h);
int khg_accs_upload(khg_ctx *ctx, khg_accs *a, const double *buf_h);

/* scripts/gmm_acc_stats_ali.py:46-56 for every frame of every utterance with a resident
 * alignment: AccumAmDiagGmm::AccumulateForGmm (csrc/mle-am-diag-gmm.cc:41-52) ->
 * AccumDiagGmm::AccumulateFromDiag/FromPosteriors (csrc/mle-diag-gmm.cc:123-158) ->
 * DiagGmm::ComponentPosteriors (csrc/diag-gmm.cc:368-392), plus tacc[tid] += 1.
 * Asynchronous on the context's stream.  Right behind an asynchronous khg_align on a large set the call waits ONCE for the exact DP
 * (not for the order-faithful decoders, not for its own kernels) to learn whether any utterance was left to those decoders; if so
 * the certified utterances are accumulated at once and the others in a second pass when the decoders are done (the statistics are
 * additive, csrc/mle-am-diag-gmm.cc:41-52; KHG_OPT_K2_SPLIT = 1: one pass after the decoders). */
int khg_acc_stats(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, float weight,
                  khg_accs *a);
/* gmm-acc-stats: the same statistics from posteriors resident on the device.  Every entry (utterance u, frame t,
 * transition-id tid, weight w64) of `p` adds what AccumulateForGmm(am, x[u][t], id2pdf[tid], w) and TransitionModel::Accumulate(w,
 * tid) add, with w = (float)((double)scale * w64); entries are independent (two ids of one frame that share a pdf are not merged), an
 * entry whose w is 0 is skipped.  Utterance u of `p` is utterance u of the set; one without frames in `p` adds nothing.  No resident
 * alignment is needed or touched.  Asynchronous on the context's stream; adds into the same block as khg_acc_stats.  KHG_E_ARG,
 * before anything is launched (the block stays as it was): a handle of another context, another n_utt, an utterance whose
 * posterior has frames but not the set's number of them, model / accumulator / feature dimensions that do not match, a scale that
 * is not finite, an uploaded handle with an id above the transition model's.  (An id above it in a handle made from lattices, and
 * an entry whose scale * weight overflows a float, are dropped on the device and raise the context's error word: the next
 * synchronising call answers KHG_E_RUNTIME.) */
int khg_acc_stats_post(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, const khg_posteriors *p, float scale,
                       khg_accs *a);
/* gmm-acc-stats2: signed posteriors into two blocks.  With w = (float)((double)scale * w64), an entry with w > 0 adds
 * to `num` what khg_acc_stats_post adds with weight w, one with w < 0 adds to `den` with weight -w (statistics, transition counts and
 * scalars alike: TransitionModel::Accumulate(fabs(w), tid) into the matching block).  khg_acc_stats_post's refusals, for both blocks;
 * num == den: KHG_E_ARG.  Asynchronous on the context's stream. */
int khg_acc_stats_post2(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, const khg_posteriors *p, float scale,
                        khg_accs *num, khg_accs *den);

/* Elementwise operations on whole blocks (what Kaldi's gmm-sum-accs and gmm-ismooth-stats do on files), asynchronous on the context's
 * stream.  Two blocks of one call must belong to `ctx` and have the same layout (Gaussians, dim, transition-ids), and the factor must
 * be finite: KHG_E_ARG otherwise, before anything is launched.  dst and src may be the same block.
 *   add:    dst += (double)scale * src over occupancies, mean / variance rows, transition counts and the scalars -- AccumAmDiagGmm::Add
 *           (csrc/mle-am-diag-gmm.cc:119-128) plus the transition sum of gmm-sum-accs;
 *   scale:  dst *= (double)f (AccumAmDiagGmm::Scale, :130-138);
 *   smooth_with_accum: AccumDiagGmm::SmoothWithAccum (csrc/mle-diag-gmm.cc:209-226) for every Gaussian: where src.occ != 0, dst.occ +=
 *           tau and the mean / variance rows += src row * tau / src.occ; other Gaussians are untouched.  `m` gives the layout the blocks
 *           must have.  untouched_out (may be NULL) receives the number of Gaussians with src.occ == 0; asking for it synchronises. */
int khg_accs_add(khg_ctx *ctx, khg_accs *dst, float scale, const khg_accs *src);
int khg_accs_scale(khg_ctx *ctx, khg_accs *dst, float f);
int khg_accs_smooth_with_accum(khg_ctx *ctx, khg_accs *dst, float tau, const khg_accs *src, const khg_model *m,
                               int32_t *untouched_out);

/* ---- C1: cross-GPU sum of the accumulator block (one process per GPU) -------------------- */
/* AccumAmDiagGmm::Add across jobs (csrc/mle-am-diag-gmm.cc:119-128; what Kaldi's gmm-sum-accs does on
 * files): ONE in-place ncclAllReduce(sum, fp64) of the whole block [occ | mean_acc | var_acc | trans_acc |
 * scalars], enqueued on the context's stream right behind khg_acc_stats -- no host synchronisation
 * between K3, the exchange and khg_model_mle_update.  `comm` is an RCCL ncclComm_t for the context's
 * device: the caller's own (ncclCommInitRank) or one made with khg_comm_create.  The library does not
 * link RCCL: it binds ncclAllReduce & co. from the librccl already loaded into the process (torch's, the
 * caller's) or loads librccl.so.1 itself.  comm == NULL: a one-rank job, nothing to exchange. */
int khg_accs_allreduce(khg_ctx *ctx, khg_accs *a, void *comm);
/* The same sum for the accumulator rows of pdfs [first_pdf, first_pdf + n_pdf) only -- the three contiguous pieces occ / mean_acc /
 * var_acc of their Gaussians, one RCCL group -- or, with first_pdf < 0, for the transition counts and scalars behind them.  The
 * ranges of a partition of the pdfs plus the tail add up to khg_accs_allreduce. */
int khg_accs_allreduce_range(khg_ctx *ctx, khg_accs *a, const khg_model *m, int32_t first_pdf, int32_t n_pdf, void *comm);
/* khg_acc_stats with C1 PIPELINED behind it: the pdfs are cut into `nparts` ranges (<= 0: 4); while the accumulate kernels of
 * range i + 1 run on the context's stream, the rows of range i are all-reduced on a second stream of the context; the context's
 * stream waits for the last piece, so the caller goes on exactly as after khg_acc_stats + khg_accs_allreduce.  For the LAST
 * khg_acc_stats of a pass only (the block must be complete); comm == NULL: plain khg_acc_stats.  On two ranks the result is
 * bit-identical to the unpipelined exchange (a + b has one order); on more, each form is reproducible run to run. */
int khg_acc_stats_reduce(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, float weight, khg_accs *a,
                         void *comm, int32_t nparts);
/* BASELINE.json configs[4] "fp32 stats vs CPU tolerance check": the same exchange with the block
 * rounded to fp32 for the wire (convert -> ncclAllReduce(sum, fp32) -> widen back into the block):
 * half the xGMI bytes, per-rank partial sums lose their low 29 bits.  comm == NULL: only the rounding. */
int khg_accs_allreduce_f32(khg_ctx *ctx, khg_accs *a, void *comm);
/* communicator helpers for callers without their own RCCL plumbing: rank 0 calls khg_comm_unique_id,
 * ships the 128 bytes to the other ranks by any means (a file, MPI, torch.distributed's store), every
 * rank then calls khg_comm_create (collective; blocks until all `nranks` ranks have called it). */
#define KHG_COMM_ID_BYTES 128
int khg_comm_unique_id(void *id_out /* [KHG_COMM_ID_BYTES] */);
int khg_comm_create(khg_ctx *ctx, int32_t nranks, int32_t rank, const void *id, void **comm_out);
int khg_comm_destroy(void *comm);
/* what RCCL reports for a communicator (any of the outputs may be NULL): ncclCommCount, ncclCommUserRank, ncclGetVersion
 * (comm == NULL: only the version) -- lets a multi-GPU run state on its own record how many ranks the collective really spanned */
int khg_comm_info(void *comm, int32_t *nranks, int32_t *rank, int32_t *version);

/* ---- host-side M-step and helpers (no GPU needed) --------------------------------------- */
/* DiagGmm::ComputeGconsts (csrc/diag-gmm.cc:103-147) for a ragged model; num_bad_out may be NULL */
int khg_compute_gconsts(int32_t num_pdfs, int32_t dim, const int32_t *gauss_off,
                        const float *weights, const float *inv_vars, const float *means_invvars,
                        float *gconsts, int32_t *num_bad_out);

typedef struct {
  float min_gaussian_weight;          /* MleDiagGmmOptions (csrc/mle-diag-gmm.h:23-45): 1e-5 */
  float min_gaussian_occupancy;       /* 10 */
  double min_variance;                /* 1e-3 */
  int32_t remove_low_count_gaussians; /* 1 */
  /* variance_floor_vector (csrc/mle-diag-gmm.h:26-28, used at csrc/mle-diag-gmm.cc:311-322): per-dimension floor, host
   * pointer to `dim` doubles, NULL = not supplied (then min_variance floors every dimension) */
  const double *variance_floor_vector;
} khg_mle_options;
void khg_mle_options_default(khg_mle_options *o);

/* MleAmDiagGmmUpdate (csrc/mle-am-diag-gmm.cc:153-202) over flat arrays.  In: accumulator
 * arrays laid out like the model (gauss_off); in/out: weights, gconsts, means_invvars, inv_vars
 * compacted in place when Gaussians are removed; out: new_gauss_off[num_pdfs+1],
 * objf_change, count (floats, as the reference returns them). */
int khg_mle_am_diag_gmm_update(const khg_mle_options *o, int32_t num_pdfs, int32_t dim,
                               const int32_t *gauss_off, const double *occ, const double *mean_acc,
                               const double *var_acc, uint16_t acc_flags, uint16_t flags,
                               float *weights, float *gconsts, float *means_invvars,
                               float *inv_vars, int32_t *new_gauss_off, float *objf_change,
                               float *count, int32_t *floored_elems, int32_t *floored_gauss,
                               int32_t *removed);

/* DiagGmm::Merge (csrc/diag-gmm.cc:557-759, MergedComponentsLogdet :761-778) on one pdf's flat arrays: greedy merging of
 * the pair whose union loses the least likelihood, down to target_components (1: the global mean and variance); arrays are
 * compacted in place, gconsts recomputed; history_out (may be NULL) receives the merged pairs (kept, removed) in order --
 * what python/csrc/diag-gmm.cc:79-85 returns from DiagGmm.merge.  AmDiagGmm::MergeByCount (csrc/am-diag-gmm.cc:91-108) =
 * this per pdf with the targets of GetSplitTargets.  Host only. */
int khg_diag_gmm_merge(int32_t *num_gauss, int32_t dim, int32_t target_components, float *weights, float *gconsts,
                       float *means_invvars, float *inv_vars, int32_t *history_out, int32_t *num_history_out);

/* ---- Extended Baum-Welch update (MMI-style discriminative training) -------- */
/* Kaldi's gmm-est-gmm-ebw / gmm-est-weights-ebw on a numerator and a denominator block of statistics.  The reference has no EBW
 * update: the rule in DESIGN.md 7i is the specification (tests/ebw_ref.py restates it).  Per Gaussian, with occ = occ_n - occ_d,
 * x = x_n - x_d, x2 = x2_n - x2_d and the fp64 normal form (mu, var) of the float parameters: D = (tau + E occ_d) / 2 (or
 * -1.0001 occ + 1e-10 when D + occ <= 0); mu' = (x + D mu) / (occ + D), var' = (x2 + D (var + mu^2)) / (occ + D) - mu'^2; D grows by
 * 1.1 until every var' > 0, is then doubled, and the values at the doubled D are written back through the float conversion of the
 * ML update.  A Gaussian with occ_n == occ_d == 0 is skipped; one still failing after 100 tries is left as it was.  Per pdf (flag w)
 * 50 rounds of w <- n + (k_max - d / w_orig) w, floored and renormalised, unless sum n < min_num_count_weight_update.  gconsts are
 * recomputed; no Gaussian is removed.  All arithmetic is IEEE fp64 in one fixed order: host and device forms give bit-identical
 * weights, inv_vars and means_invvars; gconsts go through logf (a few ulps) and the two diagnostics through log and a sum. */
typedef struct {
  double E;   /* 2.0: D starts at E occ_den / 2 */
  double tau; /* 0.0: added to E occ_den before halving (I-smoothing belongs on the numerator block: khg_accs_smooth_with_accum) */
} khg_ebw_options;
typedef struct {
  double min_num_count_weight_update; /* 10.0: pdfs whose numerator count is below keep their weights */
  double min_gaussian_weight;         /* 1e-5: floor inside every round */
  double tau;                         /* 0.0: n[g] = occ_n[g] + tau w_orig[g] */
} khg_ebw_weight_options;
typedef struct {
  double auxf_impr_gauss;   /* sum over the updated Gaussians of Q(new) - Q(old) on the smoothed statistics */
  double count;             /* sum of the numerator occupancies */
  double auxf_impr_weights; /* sum over the updated pdfs of sum_g n log(w' / w) - d (w' - w) / w */
  int32_t floored;          /* Gaussians that needed a larger D than the first */
  int32_t failed;           /* Gaussians left unchanged after 100 tries */
  int32_t skipped;          /* Gaussians without numerator and denominator counts */
  int32_t weights_skipped;  /* pdfs below min_num_count_weight_update */
} khg_ebw_results;
void khg_ebw_options_default(khg_ebw_options *o);
void khg_ebw_weight_options_default(khg_ebw_weight_options *o);
/* The host form over flat arrays laid out like the model (gauss_off); the two accumulator triples are (occ[sumG], mean_acc[sumG][dim],
 * var_acc[sumG][dim]).  flags: m = 1, v = 2, w = 4 of GmmUpdateFlags (t is ignored; v without m is allowed).  In/out: weights,
 * means_invvars, inv_vars; out: gconsts, *res (may be NULL).  The four mean / variance accumulators may be NULL when flags has neither
 * m nor v (a weights-only update reads the occupancies alone).  KHG_E_ARG for an option that is not finite. */
int khg_ebw_am_diag_gmm_update(const khg_ebw_options *o, const khg_ebw_weight_options *wo, int32_t num_pdfs, int32_t dim,
                               const int32_t *gauss_off, const double *num_occ, const double *num_mean_acc,
                               const double *num_var_acc, const double *den_occ, const double *den_mean_acc,
                               const double *den_var_acc, uint16_t flags, float *weights, float *gconsts,
                               float *means_invvars, float *inv_vars, khg_ebw_results *res);

/* ---- K4: the same M-step on the device ---------------------------------- */
/* MleAmDiagGmmUpdate (csrc/mle-am-diag-gmm.cc:153-202; per pdf MleDiagGmmUpdate,
 * csrc/mle-diag-gmm.cc:243-390, DiagGmmNormal csrc/diag-gmm-normal.cc:14-48, ComputeGconsts
 * csrc/diag-gmm.cc:103-147, RemoveComponents :853-938) run on the (all-reduced) accumulators where K3
 * left them: no 205 MB accumulator download, no host update, no parameter upload.  The model handle is
 * updated IN PLACE (row-major parameters, the K1 tile image, gauss_off when Gaussians were removed --
 * then call khg_accs_relayout before the next khg_acc_stats).  weights, inv_vars and means_invvars are
 * bit-identical to khg_mle_am_diag_gmm_update; gconsts / objf_change go through logf and may differ from
 * the host's in the last place.  The mixture weights (which khg_model_create does not take; K1-K3 only
 * need gconsts) must have been set with khg_model_set_weights. */
int khg_model_set_weights(khg_ctx *ctx, khg_model *m, const float *weights_h);
int khg_model_mle_update(khg_ctx *ctx, khg_model *m, const khg_accs *a, const khg_mle_options *o,
                         uint16_t flags, float *objf_change, float *count, int32_t *floored_elems,
                         int32_t *floored_gauss, int32_t *removed);
/* The SHARDED M-step of a multi-GPU job (MleAmDiagGmmUpdate is independent per pdf, csrc/mle-am-diag-gmm.cc:153-202): rank r of
 * nranks owns the pdfs [P r / nranks, P (r + 1) / nranks).  `a` holds the rank's LOCAL sums (no khg_accs_allreduce before): its
 * mean / variance rows are ncclReduce'd to their owners by pdf range, the occupancies all-reduced (every rank's mixing-up targets need
 * them; the transition counts and scalars are NOT touched: khg_accs_allreduce_range with first_pdf < 0), every rank updates its own
 * pdfs, the rewritten rows and per-pdf results are ncclBroadcast from their owners, and every rank finishes on the complete model
 * (compaction when Gaussians were removed, images): bit-identical to khg_model_mle_update on the all-reduced block on two ranks
 * (and with one), (nranks - 1) / nranks x (accumulator + parameter bytes) on the wire per rank instead of 2 (nranks - 1) / nranks x
 * accumulator bytes.  comm == NULL: khg_model_mle_update. */
int khg_model_mle_update_sharded(khg_ctx *ctx, khg_model *m, khg_accs *a, const khg_mle_options *o, uint16_t flags, void *comm,
                                 int32_t nranks, int32_t rank, float *objf_change, float *count, int32_t *floored_elems,
                                 int32_t *floored_gauss, int32_t *removed);
/* Its pieces, for callers that move the rows themselves (ranks that cannot share device buffers): the update of pdfs [first_pdf,
 * first_pdf + n_pdf) alone (rows rewritten in place in the old layout, one 32-byte result per pdf kept on the handle); the rows of a
 * range + its results to / from the host (any pointer may be NULL); the finish on the complete rows and results. */
int khg_model_mle_update_range(khg_ctx *ctx, khg_model *m, const khg_accs *a, const khg_mle_options *o, uint16_t flags,
                               int32_t first_pdf, int32_t n_pdf);
int khg_model_mle_rows_download(khg_ctx *ctx, khg_model *m, int32_t first_pdf, int32_t n_pdf, float *weights_h, float *gconsts_h,
                                float *means_invvars_h, float *inv_vars_h, void *results_h /* 32 n_pdf bytes */);
int khg_model_mle_rows_upload(khg_ctx *ctx, khg_model *m, int32_t first_pdf, int32_t n_pdf, const float *weights_h,
                              const float *gconsts_h, const float *means_invvars_h, const float *inv_vars_h, const void *results_h);
int khg_model_mle_update_finish(khg_ctx *ctx, khg_model *m, float *objf_change, float *count, int32_t *floored_elems,
                                int32_t *floored_gauss, int32_t *removed);
/* The Extended Baum-Welch update above on the device: one workgroup per pdf reads the numerator and denominator blocks where K3 left
 * them and rewrites the handle IN PLACE (row-major parameters, gconsts, then the K1 tile image and per-parameter-version data, as
 * khg_model_mle_update does); gauss_off does not change.  Both blocks must belong to `ctx` and be laid out for the handle
 * (KHG_E_ARG before anything is launched otherwise, as for an option that is not finite or dim > 256).  weights, inv_vars and
 * means_invvars are bit-identical to khg_ebw_am_diag_gmm_update and so are the counters; gconsts within a few float ulps, the two
 * diagnostics to the rounding of log and of a reordered fp64 sum.  Synchronous (the results come back). */
int khg_model_ebw_update(khg_ctx *ctx, khg_model *m, const khg_accs *num, const khg_accs *den, const khg_ebw_options *o,
                         const khg_ebw_weight_options *wo, uint16_t flags, khg_ebw_results *res);
/* Mixing up on the handle: AmDiagGmm::SplitByCount's per-pdf DiagGmm::Split (csrc/am-diag-gmm.cc:72-90, csrc/diag-gmm.cc:780-851)
 * to targets_h[p] >= current components (the caller computes them with GetSplitTargets, csrc/model-common.cc:29-70, from
 * the per-pdf occupancies -- khg_accs_download_range(0, sumG)).  The reference draws the perturbations from the process-global
 * rand(); here they are INJECTED: randn_h holds n_randn >= (sum of new components) x dim standard normal deviates, consumed pdf
 * by pdf in split order (KHG_E_ARG when there are fewer), so every rank of a multi-GPU job (and the host form) perturbs identically.  Parameters bit-identical to
 * the host form, gconsts through logf.  The handle is updated in place (call khg_accs_relayout afterwards). */
int khg_model_split(khg_ctx *ctx, khg_model *m, const int32_t *targets_h, float perturb_factor, const float *randn_h,
                    int64_t n_randn);
/* Mixing down on the handle: AmDiagGmm::MergeByCount's per-pdf DiagGmm::Merge (csrc/am-diag-gmm.cc:91-108, csrc/diag-gmm.cc:557-759,
 * MergedComponentsLogdet :761-778) to 1 <= targets_h[p] <= current components (GetSplitTargets again, with "can't merge below 1"
 * applied by the caller).  One workgroup per pdf, float arithmetic in the order of khg_diag_gmm_merge; the pair merged at each
 * step is the first maximum of the lower triangle in (i, j < i) order, whatever the thread count.  The handle is updated in
 * place (call khg_accs_relayout afterwards). */
int khg_model_merge(khg_ctx *ctx, khg_model *m, const int32_t *targets_h);
/* total Gaussians and (gauss_off_h may be NULL) the current gauss_off[num_pdfs+1] of the handle */
int khg_model_num_gauss(const khg_model *m, int64_t *total, int32_t *gauss_off_h);
/* parameters back to the host (AmDiagGmm::Write needs them); any pointer may be NULL */
int khg_model_download(khg_ctx *ctx, const khg_model *m, float *weights_h, float *gconsts_h,
                       float *means_invvars_h, float *inv_vars_h);
/* re-lay the accumulator block for the handle's current gauss_off and zero it */
int khg_accs_relayout(khg_ctx *ctx, khg_accs *a, const khg_model *m);
/* only the transition statistics [num_tids+1] and the 8 scalars (what TransitionModel::MleUpdate and the
 * log line of scripts/gmm_acc_stats_ali.py need) -- a few kB instead of the whole block */
int khg_accs_download_trans(khg_ctx *ctx, const khg_accs *a, double *trans_h, double *scalars_h);

/* any slice [first, first+count) of the fp64 block (e.g. occ = [0, sumG) for the mix-up targets of
 * scripts/gmm_est.py:66-70) */
int khg_accs_download_range(khg_ctx *ctx, const khg_accs *a, int64_t first, int64_t count,
                            double *dst_h);
/* scripts/gmm_boost_silence.py:10-45 on the handle: weights of the listed pdfs *= scale, their gconsts
 * recomputed (DiagGmm::SetWeights + ComputeGconsts, csrc/diag-gmm.cc:103-147), tile image repacked */
int khg_model_scale_weights(khg_ctx *ctx, khg_model *m, int32_t n, const int32_t *pdfs_h,
                            float scale);

/* TransitionModel::MleUpdate (csrc/transition-model.cc:657-750) + ComputeDerivedOfProbs (:339-359) */
int khg_transition_mle_update(int32_t num_tstates, const int32_t *state2id,
                              const int32_t *self_loop_of, const double *stats, float floor_,
                              float mincount, float *log_probs, float *non_self_loop_log_probs,
                              float *objf_impr, float *count);

/* GetScaledTransitionLogProb (csrc/hmm-utils.cc:442-463) negated, for every tid:
 * out_cost[0..num_tids] (entry 0 = 0). */
int khg_scaled_trans_cost(int32_t num_tids, const float *log_probs,
                          const float *non_self_loop_log_probs, const int32_t *id2state,
                          const uint8_t *is_self_loop, float transition_scale,
                          float self_loop_scale, float *out_cost);

/* ---- fMLLR speaker adaptation (gmm-est-fmllr, transform-feats) --------------------------------------------------- */
/* The reference has no fMLLR: the rule in DESIGN.md 7l is the specification (tests/fmllr_ref.py restates it).  Notation: x+ = [x, 1],
 * W is dim x (dim + 1), A = W[:, :dim].  Feature dimensions up to KHG_FMLLR_MAX_DIM (the MFMA range of K1 / K3); above: KHG_E_UNSUPPORTED. */
#define KHG_FMLLR_MAX_DIM 80
#define KHG_FMLLR_OK 0           /* the transform was estimated                                                        */
#define KHG_FMLLR_LOW_COUNT 1    /* beta < min_count: W = [I | 0]                                                      */
#define KHG_FMLLR_SINGULAR 2     /* a pivot of some G[d] (or of A) not finite or not > 0: W = [I | 0]                  */
/* Kaldi's FmllrDiagGmmAccs for n_spk speakers, resident on the device, all fp64: per speaker beta, K[dim][dim + 1] and G[dim], each
 * G[d] the symmetric (dim + 1) x (dim + 1) matrix as Kaldi's packed lower triangle ((i, j <= i) at i (i + 1) / 2 + j):
 * (dim + 1)(dim + 2) / 2 doubles.  Host layout of download / upload: beta_h[n_spk], K_h[n_spk][dim][dim + 1], G_h[n_spk][dim][packed];
 * download takes NULL for an array that is not wanted and synchronises (deferred kernel errors: KHG_E_RUNTIME), upload needs all
 * three.  add: dst += (double)scale * src elementwise (one product, one add), asynchronous; the handles must agree in speakers and
 * dimension and belong to `ctx` (KHG_E_ARG). */
typedef struct khg_fmllr_stats khg_fmllr_stats;
int khg_fmllr_stats_create(khg_ctx *ctx, int32_t n_spk, int32_t dim, khg_fmllr_stats **out);
int khg_fmllr_stats_destroy(khg_fmllr_stats *s);
int khg_fmllr_stats_zero(khg_ctx *ctx, khg_fmllr_stats *s);
int khg_fmllr_stats_download(khg_ctx *ctx, const khg_fmllr_stats *s, double *beta_h, double *K_h, double *G_h);
int khg_fmllr_stats_upload(khg_ctx *ctx, khg_fmllr_stats *s, const double *beta_h, const double *K_h, const double *G_h);
int khg_fmllr_stats_add(khg_ctx *ctx, khg_fmllr_stats *dst, float scale, const khg_fmllr_stats *src);
/* The accumulation's scratch is bounded by a chunk of `frames` frames (default 2^18; at least one 1024-frame slice, at most 2^24):
 * frames x (8 dim + 12) bytes of frame vectors plus min(2 max(1, frames / 1024) parked slice images of a speaker's block, 256 MiB), beside 4 bytes
 * per frame of the set, one more block per speaker for the call's sums and (8 dim + 8) bytes per entry of a chunk (at most 2 x frames
 * entries plus one slice's utterances').  The statistics do not depend on it, bit for bit.
 * num_chunks: how many chunks the last accumulation into the handle ran (tests). */
int khg_fmllr_stats_set_chunk_frames(khg_fmllr_stats *s, int64_t frames);
int khg_fmllr_stats_num_chunks(const khg_fmllr_stats *s, int32_t *n_chunks);
/* gmm-est-fmllr's accumulation from posteriors resident on the device.  Every entry (utterance u, frame t, transition-id, weight w64)
 * of `p` with utt2spk_h[u] = s >= 0 counts for speaker s with w = (float)((double)scale * w64), as in khg_acc_stats_post.  Per entry,
 * fp32: the component posteriors gamma_g of the entry's pdf at x as K3's POST forms compute them, ea[d] = sum_g gamma_g inv_var[g][d],
 * eb[d] = sum_g gamma_g mean_invvar[g][d], ec = sum_g gamma_g, in Gaussian order.  Per frame: a_t, b_t the float sums of the frame's
 * entries in entry order, c_t their double sum.  Per speaker, fp64, over its frames in set order: beta += c_t, K[d][j] += b_t[d] x+[j],
 * G[d][i][j] += a_t[d] (x+[i] x+[j]) for j <= i (the product of two floats is exact in a double; the order of the sum is fixed by the
 * speaker's own frame list: 1024-frame slices on the fp64 matrix pipe, added in slice order).  The statistics of a speaker have the
 * same bits whatever else is in the call, whatever the chunk size, and from run to run.  An entry with w == 0, an utterance with
 * utt2spk < 0 and an utterance without frames in `p` add nothing; negative weights are taken as they are.  Adds into `stats`;
 * asynchronous on the context's stream once the plan is uploaded.  khg_acc_stats_post's refusals (KHG_E_ARG before anything is
 * launched), and KHG_E_ARG for a utt2spk value >= n_spk or statistics of another dimension. */
int khg_acc_fmllr_stats_post(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, const khg_posteriors *p, float scale,
                             const int32_t *utt2spk_h, khg_fmllr_stats *stats);
typedef struct {
  double min_count;   /* 500: speakers with beta below it keep W = [I | 0] */
  int32_t num_iters;  /* 40: sweeps over the rows of W */
} khg_fmllr_options;
void khg_fmllr_options_default(khg_fmllr_options *o);
/* Kaldi's ComputeFmllrMatrixDiagGmmFull (update type "full") on host arrays laid out as khg_fmllr_stats_download gives them; needs no
 * device.  Per speaker: invG[d] by Gauss-Jordan without pivoting; from W = [I | 0], num_iters sweeps of the row update of DESIGN.md 7l
 * (c = row d of (A^T)^-1 by Gauss-Jordan with partial pivoting, the two roots of the quadratic, the one with the larger auxiliary
 * value).  All fp64, one operation at a time in index order.  Outputs (any may be NULL, but one of W_h / W64_h is needed):
 * W_h[n_spk][dim][dim + 1] floats, W64_h the same before narrowing, objf_impr_h[n_spk] = Q(W) - Q([I | 0]), count_h[n_spk] = beta,
 * status_h[n_spk] KHG_FMLLR_*.  o == NULL: the defaults.  Speakers run on up to 16 threads; results do not depend on that. */
int khg_fmllr_compute(const khg_fmllr_options *o, int32_t n_spk, int32_t dim, const double *beta_h, const double *K_h, const double *G_h,
                      float *W_h, double *W64_h, double *objf_impr_h, double *count_h, int32_t *status_h);
/* The same estimate on the device, on the statistics where the accumulation left them: one kernel inverts the n_spk x dim matrices
 * G[d] into HBM scratch (one workgroup per matrix), one runs one workgroup per speaker for the sweeps.  Every operation is the host
 * form's, in its order, with contraction off: W, the statuses and the counts are bit-identical to khg_fmllr_compute on the downloaded
 * statistics wherever the two roots do not tie; objf_impr agrees to the rounding of log.  W_h (host) and / or W_d (a
 * caller-owned device buffer that keeps the transforms resident for khg_utts_transform_feats), [n_spk][dim][dim + 1] floats, and the
 * other outputs may each be NULL.  o == NULL: the defaults.  Synchronous. */
int khg_fmllr_stats_estimate(khg_ctx *ctx, const khg_fmllr_stats *stats, const khg_fmllr_options *o, float *W_h, float *W_d,
                             double *objf_impr_h, double *count_h, int32_t *status_h);
/* ali-to-post on the device: a posteriors handle (free it with khg_posteriors_destroy) with one entry of weight 1 per frame from the
 * set's resident alignment (khg_align, khg_ali_upload), so an SAT loop never brings the ids down.  An utterance whose alignment failed
 * (ids 0) gets no frames.  One flag per utterance is read back: synchronous.  KHG_E_ARG without a resident alignment. */
int khg_posteriors_from_ali(khg_ctx *ctx, khg_utts *u, khg_posteriors **out);
/* transform-feats on the set's resident rows: y = A x + b with W = [A | b] of the utterance's speaker, in float -- y[d] = b[d], then
 * y[d] = fmaf(A[d][j], x[j], y[d]) for j = 0 .. dim - 1.  An utterance with utt2spk_h[u] < 0 is copied.  Exactly one of W_h (host) and
 * W_d (a caller-owned device buffer: the transforms stay resident) is given, [n_spk][dim][dim + 1] floats.  With out_d the rows go
 * to that device buffer (the set's size) and the set is untouched; with out_d == NULL the set's own rows are rewritten in place
 * (borrowed device features included) and the set is told so, as by khg_utts_features_changed.  KHG_E_ARG for a utt2spk value
 * >= n_spk.  Synchronous. */
int khg_utts_transform_feats(khg_ctx *ctx, khg_utts *u, int32_t n_spk, const int32_t *utt2spk_h, const float *W_h, const float *W_d,
                             float *out_d);

/* ---- MLLT / semi-tied covariance (gmm-acc-mllt, est-mllt, gmm-transform-means) ------------------------------------- */
/* The reference has no MLLT: the rule in DESIGN.md 7m is the specification (tests/mllt_ref.py restates it).  One global dim x dim
 * matrix M that makes the diagonal-covariance assumption fit: features become M x, means M mu.  Feature dimensions up to
 * KHG_MLLT_MAX_DIM (the MFMA range of the fMLLR Gram kernel); above: KHG_E_UNSUPPORTED. */
#define KHG_MLLT_MAX_DIM 80
#define KHG_MLLT_OK 0            /* the transform was estimated                                                         */
#define KHG_MLLT_SINGULAR 1      /* beta <= 0, or a pivot of some G[d] (or of A) not finite or not > 0: M = I           */
/* Kaldi's MlltAccs resident on the device, all fp64: beta and G[dim], each G[d] a symmetric dim x dim matrix as Kaldi's packed lower
 * triangle ((i, j <= i) at i (i + 1) / 2 + j): dim (dim + 1) / 2 doubles.  Host layout of download / upload: *beta_h, G_h[dim][packed];
 * download takes NULL for what is not wanted and synchronises (deferred kernel errors: KHG_E_RUNTIME), upload needs both.
 * add: dst += (double)scale * src elementwise (one product, one add), asynchronous; the handles must agree in dimension and belong
 * to `ctx` (KHG_E_ARG). */
typedef struct khg_mllt_stats khg_mllt_stats;
int khg_mllt_stats_create(khg_ctx *ctx, int32_t dim, khg_mllt_stats **out);
int khg_mllt_stats_destroy(khg_mllt_stats *s);
int khg_mllt_stats_zero(khg_ctx *ctx, khg_mllt_stats *s);
int khg_mllt_stats_download(khg_ctx *ctx, const khg_mllt_stats *s, double *beta_h, double *G_h);
int khg_mllt_stats_upload(khg_ctx *ctx, khg_mllt_stats *s, const double *beta_h, const double *G_h);
int khg_mllt_stats_add(khg_ctx *ctx, khg_mllt_stats *dst, float scale, const khg_mllt_stats *src);
/* The frame side's scratch is bounded by a chunk of `frames` frames exactly as khg_fmllr_stats_set_chunk_frames bounds fMLLR's (the
 * per-frame and per-entry vectors are the same; a parked slice image is dim^2 (dim + 1) / 2 + 1 doubles here).  The statistics do not
 * depend on it, bit for bit.  num_chunks: how many chunks the last accumulation into the handle ran (tests). */
int khg_mllt_stats_set_chunk_frames(khg_mllt_stats *s, int64_t frames);
int khg_mllt_stats_num_chunks(const khg_mllt_stats *s, int32_t *n_chunks);
/* gmm-acc-mllt from posteriors resident on the device, over ALL the data (no random pruning).  Every entry of `p` counts with
 * w = (float)((double)scale * w64) and the component posteriors gamma_g of its pdf at x as khg_acc_fmllr_stats_post defines them:
 * beta += sum_g gamma_g, G[d] += sum_g gamma_g inv_var[g][d] (x - mu_g)(x - mu_g)^T.  Computed as a frame side minus a Gaussian side,
 * both shifted by c = the (float) mean of the model's means so that the terms do not cancel:
 *   frame side     S[d][i][j] = sum_t a_t[d] (x'[i] x'[j]), x' = (double)x - (double)c (exact), a_t fMLLR's frame vector: fMLLR's Gram sum for one
 *                  speaker who owns every utterance, 1024-frame slices of the call's frame list in set order, added in slice order;
 *   Gaussian side  C[d][i][j] = sum_g inv_var[g][d] (m'_g[i] mu'_g[j] + mu'_g[i] m'_g[j] - occ_g mu'_g[i] mu'_g[j]) with occ_g / m_g
 *                  the call's own occupancies and mean sums as khg_acc_stats_post computes them for the same entries -- here with
 *                  ONE workgroup per pdf however many entries the pdf has, which fixes the order of its sums --, shifted in fp64;
 *                  1024-Gaussian slices of the model in (pdf, g) order on the fp64 matrix pipe, added in slice order;
 *   G += S - C, beta += sum_t c_t.
 * The kernels of this call use no atomics, and the fp64 atomics that end khg_acc_stats_post's workgroups have one writer per cell
 * here: the same bits from run to run and whatever the chunk size.  The price is that the pdf with the most entries is one
 * workgroup's walk (DESIGN.md 7m has the figures).  Calls under ONE model add; a handle accumulated under two
 * models is the caller's error.  Scratch owned by the handle, allocated on first use and kept: one accumulator block in khg_accs
 * layout for the call's occ_g / m_g (8 (sumG (2 dim + 1) + num_tids + 9) bytes, zeroed per call), the fMLLR chunk scratch above, two
 * blocks of the handle's size for the call's S and C, and parked slice images shared by the two sides (at most 256 MiB).
 * khg_acc_stats_post's refusals, before anything is launched (the handle keeps its bits): KHG_E_ARG, KHG_E_ARG too for statistics of
 * another dimension, and KHG_E_UNSUPPORTED for 2^31 - 1 or more entries or frames and for a model khg_acc_stats_post cannot take: a pdf
 * too wide for its any-size form, whose 64 (row pitch + Gaussians + 5) floats of LDS end at 160 KiB: 596 Gaussians and more at
 * dim <= 40, 556 and more at dim <= 80 (khg_acc_fmllr_stats_post accepts such models; this call does not).  Asynchronous on the context's stream once the plan is uploaded. */
int khg_acc_mllt_stats_post(khg_ctx *ctx, const khg_model *m, const khg_tm *tm, khg_utts *u, const khg_posteriors *p, float scale,
                            khg_mllt_stats *stats);
typedef struct {
  int32_t num_iters;  /* 200: sweeps over the rows of A */
} khg_mllt_options;
void khg_mllt_options_default(khg_mllt_options *o);
/* Kaldi's MlltAccs::Update on host arrays laid out as khg_mllt_stats_download gives them; needs no device (one dim x dim problem per
 * training iteration is not worth a kernel).  invG[d] by Gauss-Jordan without pivoting; from A = I, num_iters sweeps over the rows:
 * c = row d of (A^T)^-1 by Gauss-Jordan with partial pivoting, v = invG[d] c, A[d] = v sqrt(beta / (c . v)).  All fp64, one operation
 * at a time in index order.  Outputs (any may be NULL, but one of M_h / M64_h is needed): M_h[dim][dim] floats, M64_h the same before
 * narrowing, *objf_impr = Q(A) - Q(I) with Q(A) = beta log |det A| - 1/2 sum_d A[d] G[d] A[d]^T, *count = beta, *status KHG_MLLT_*.
 * o == NULL: the defaults.  KHG_E_UNSUPPORTED for dim > KHG_MLLT_MAX_DIM, KHG_E_ARG for num_iters < 0 or nowhere to put M. */
int khg_mllt_compute(const khg_mllt_options *o, int32_t dim, double beta, const double *G_h, float *M_h, double *M64_h,
                     double *objf_impr, double *count, int32_t *status);
/* gmm-transform-means on the handle: per Gaussian, in float, mu = means_invvars / inv_vars, y[d] = 0 then y[d] = fmaf(M[d][j], mu[j],
 * y[d]) for j = 0 .. dim - 1, means_invvars = y * inv_vars (DiagGmm::SetMeans); weights and variances stay, gconsts are recomputed
 * (within a few float ulps of the host's: logf).  M_h: dim x dim floats on the host.  The handle is rewritten IN PLACE as
 * khg_model_ebw_update does it (row-major parameters, gconsts, the K1 tile image and per-parameter-version data).  The mixture weights
 * must have been set (khg_model_set_weights).  Synchronous.  KHG_E_RUNTIME when a recomputed gconst is not a number: the handle then
 * holds the transformed parameters, all its images consistent with one another, and is the caller's to replace. */
int khg_model_transform_means(khg_ctx *ctx, khg_model *m, const float *M_h);

/* ---- LDA on spliced features (splice-feats, acc-lda, est-lda, transform-feats) ------------------------------------ */
/* The reference has no LDA: the rule in DESIGN.md 7n is the specification (tests/lda_ref.py restates it).  Notation: dim = the set's
 * feature dimension, left / right >= 0 the context, Dz = dim (left + right + 1) the spliced dimension; the spliced frame is
 * z_t[k dim + j] = x[clamp(t + k - left, 0, T - 1)][j], k = 0 .. left + right: edge frames are replicated inside the utterance, a
 * neighbouring utterance's row is never read.  The spliced matrix is never written to device memory.  Dz up to
 * KHG_LDA_MAX_SPLICED_DIM: the second-order kernel stages 64 spliced rows of 16 ceil(Dz / 16) + 1 floats in LDS (129 KiB of the 160 at
 * 512); its registers do not depend on Dz.  Above: KHG_E_UNSUPPORTED. */
#define KHG_LDA_MAX_SPLICED_DIM 512
#define KHG_LDA_TRANSFORM_LDS_BYTES 147456   /* what khg_utts_splice_transform_feats stages: 4 ((64 + left + right) dim + out_dim ((Dz + 1) | 1)) bytes */
#define KHG_LDA_OK 0             /* the transform was estimated                                                         */
#define KHG_LDA_SINGULAR 1       /* N <= 0, a Cholesky pivot not finite or not > 0, or Jacobi not converged: M = [I | 0] */
/* Kaldi's LdaEstimate accumulators resident on the device, all fp64, in Kaldi's layout: zero_acc[num_classes],
 * first_acc[num_classes][Dz], total_second_acc as Kaldi's packed lower triangle ((i, j <= i) at i (i + 1) / 2 + j): Dz (Dz + 1) / 2
 * doubles.  download takes NULL for what is not wanted and synchronises (deferred kernel errors: KHG_E_RUNTIME), upload needs all
 * three.  add: dst += (double)scale * src elementwise (one product, one add), asynchronous; the handles must agree in classes,
 * dimension and context and belong to `ctx` (KHG_E_ARG). */
typedef struct khg_lda_stats khg_lda_stats;
int khg_lda_stats_create(khg_ctx *ctx, int32_t num_classes, int32_t dim, int32_t left, int32_t right, khg_lda_stats **out);
int khg_lda_stats_destroy(khg_lda_stats *s);
int khg_lda_stats_zero(khg_ctx *ctx, khg_lda_stats *s);
int khg_lda_stats_download(khg_ctx *ctx, const khg_lda_stats *s, double *zero_h, double *first_h, double *second_h);
int khg_lda_stats_upload(khg_ctx *ctx, khg_lda_stats *s, const double *zero_h, const double *first_h, const double *second_h);
int khg_lda_stats_add(khg_ctx *ctx, khg_lda_stats *dst, float scale, const khg_lda_stats *src);
/* The second-order sum parks one image of Dz (Dz + 1) / 2 doubles per 1024-frame slice; a chunk of `frames` frames (default 2^18, at
 * least one slice, at most 2^24) holds min(frames / 1024, 256 MiB of images) slices.  The statistics do not depend on it, bit for bit.
 * num_chunks: how many chunks the last accumulation into the handle ran (tests). */
int khg_lda_stats_set_chunk_frames(khg_lda_stats *s, int64_t frames);
int khg_lda_stats_num_chunks(const khg_lda_stats *s, int32_t *n_chunks);
/* acc-lda from posteriors resident on the device.  No model is involved: the transition model alone names the class.  Every entry
 * (utterance u, frame t, transition-id, weight w64) of `p` counts with w = (float)((double)scale * w64), as in khg_acc_stats_post, for
 * class c = id2pdf[transition-id]: zero_acc[c] += w, first_acc[c] += w z_t, total_second_acc += w z_t z_t^T.  Computed form: the
 * second-order term is sum_t (W_t z_t[i]) z_t[j] with W_t the double sum of the frame's w in entry order, W_t z_t[i] rounded once in
 * double, over 1024-frame slices of the call's frame list (the utterances with frames in `p`, in set order) on the fp64 matrix pipe,
 * the slices added in slice order; the class sums run over the call's entries bucketed by class with K3's stable sort, one chain per
 * (class, element) in sorted order over slices of <= 1024 entries, added in slice order.  No atomics: the same bits from run to run
 * and whatever the chunk size.  An entry with w == 0, an utterance without frames in `p` and a frame without entries add nothing;
 * negative weights are taken as they are; there is no random pruning.  Adds into `stats`.  khg_acc_stats_post's refusals, before
 * anything is launched (the handle keeps its bits): KHG_E_ARG, KHG_E_ARG too for statistics of another dimension or context or whose
 * class count is not the transition model's number of pdfs, KHG_E_UNSUPPORTED for 2^31 - 1 or more entries or frames.  One word per
 * class is read back for the class plan (synchronises once); the rest is asynchronous on the context's stream. */
int khg_acc_lda_stats_post(khg_ctx *ctx, const khg_tm *tm, khg_utts *u, const khg_posteriors *p, float scale, khg_lda_stats *stats);
typedef struct {
  int32_t target_dim;          /* 40: rows of M */
  int32_t remove_offset;       /* 0; otherwise a last column -M mu is appended */
  double within_class_factor;  /* 1.0; f != 1 scales row i by sqrt((f + lambda_i) / (1 + lambda_i)) */
} khg_lda_options;
void khg_lda_options_default(khg_lda_options *o);
/* Kaldi's LdaEstimate::Estimate on host arrays laid out as khg_lda_stats_download gives them; needs no device (one Dz x Dz problem per
 * training stage).  All fp64, one operation at a time, sums in index order: N = sum zero, mu = sum_c first[c] / N, Tc = second / N - mu
 * mu^T, Bc = sum_{c: zero[c] != 0} first[c] first[c]^T / (N zero[c]) - mu mu^T, Wc = Tc - Bc = Lc Lc^T (Cholesky), P = Lc^-1 Bc Lc^-T,
 * its eigen-decomposition by cyclic Jacobi (stops when a full sweep rotates nothing; 64 sweeps without that: SINGULAR), eigenvalues
 * descending (ties by original index), M_full = U^T Lc^-1, the within_class_factor scaling, every row's sign fixed so that its element
 * of largest magnitude (lowest index among equals) is positive, M = the first target_dim rows, with remove_offset a last column -M mu.
 * Outputs (any may be NULL, but one of M_h / M64_h is needed): M_h[target_dim][dim_z + remove_offset] floats, M64_h the same before
 * narrowing, Mfull64_h[dim_z][dim_z], eig_h[dim_z], *count = N, *status KHG_LDA_*.  SINGULAR gives M = [I_target | 0], M_full = I and
 * zero eigenvalues.  o == NULL: the defaults.  KHG_E_ARG for target_dim < 1 or > dim_z, an option that is not finite, nowhere to put
 * M; KHG_E_UNSUPPORTED for dim_z > KHG_LDA_MAX_SPLICED_DIM. */
int khg_lda_compute(const khg_lda_options *o, int32_t num_classes, int32_t dim_z, const double *zero_h, const double *first_h,
                    const double *second_h, float *M_h, double *M64_h, double *Mfull64_h, double *eig_h, double *count, int32_t *status);
/* splice-feats | transform-feats on the set's resident rows, out of place: y_t[r] = M[r][Dz] with an offset column (has_offset), 0
 * without, then y_t[r] = fmaf(M[r][c], z_t[c], y_t[r]) for c = 0 .. Dz - 1, in float (7l's transform rule).  M_h: out_dim x
 * (Dz + has_offset) floats on the host; M_h == NULL is splice-feats: out_dim must be Dz and the spliced rows are copied.  out_d: a
 * caller-owned device buffer of [rows of the set][out_dim] floats; the set is untouched.  KHG_E_UNSUPPORTED, naming the limit, for
 * Dz > KHG_LDA_MAX_SPLICED_DIM or when the matrix and the rows do not fit KHG_LDA_TRANSFORM_LDS_BYTES.  Synchronous. */
int khg_utts_splice_transform_feats(khg_ctx *ctx, khg_utts *u, int32_t left, int32_t right, int32_t out_dim, int32_t has_offset,
                                    const float *M_h, float *out_d);

/* ---- Decision-tree building (acc-tree-stats, build-tree) ------------------------------------------------------------ */
/* The reference has no tree training: the rule in DESIGN.md 7o is the specification (tests/tree_ref.py restates it).  An event is
 * (window[0 .. N), pdf-class): the phones of the N-wide context window with the central phone at position P, 0 where the window
 * reaches outside the utterance.  Supported: N in 1 .. KHG_TREE_MAX_CONTEXT, 0 <= P < N, phones 1 .. KHG_TREE_MAX_PHONE, pdf-classes
 * 0 .. KHG_TREE_MAX_PDF_CLASS, fewer than 2^31 - 1 frames in a set; anything else is KHG_E_ARG before any launch. */
#define KHG_TREE_MAX_CONTEXT 3
#define KHG_TREE_MAX_PHONE 65535
#define KHG_TREE_MAX_PDF_CLASS 255
#define KHG_TREE_TID_SELF_LOOP 1   /* tid_flags: the transition-id is a self-loop                                       */
#define KHG_TREE_TID_FINAL 2       /* tid_flags: the transition-id enters the final state of its phone's topology       */
#define KHG_TREE_STATUS_NO_ALI 1   /* status bits of an utterance khg_acc_tree_stats skipped: an id outside 1 .. num_tids (a failed khg_align leaves 0) */
#define KHG_TREE_STATUS_MIXED_PHONES 2 /* ... two phones inside one segment                                              */
#define KHG_TREE_STATUS_OPEN_END 4 /* ... the last segment does not end in a final transition-id followed by self-loops only */
/* The statistics: the distinct events seen, ascending in (window[0], .., window[N - 1], pdf-class), each with count, x[dim] and
 * x2[dim] in fp64, resident on the device.  zero empties the handle.  download: keys_h[num_keys][N + 1] int32 (the window, then the
 * pdf-class), count_h[num_keys], x_h / x2_h[num_keys][dim]; NULL for what is not wanted; synchronises.  upload replaces the contents;
 * the keys must ascend strictly (KHG_E_ARG).  add: dst = dst + (double)scale * src over the union of the keys -- a key of both gets
 * a + scale b (one product, one add, not fused), a key of one side a or scale b; the handles must agree in dim, N, P and belong to
 * `ctx`.  Synchronous. */
typedef struct khg_tree_stats khg_tree_stats;
int khg_tree_stats_create(khg_ctx *ctx, int32_t dim, int32_t N, int32_t P, khg_tree_stats **out);
int khg_tree_stats_destroy(khg_tree_stats *s);
int khg_tree_stats_zero(khg_ctx *ctx, khg_tree_stats *s);
int khg_tree_stats_num_keys(khg_ctx *ctx, const khg_tree_stats *s, int64_t *num_keys);
int khg_tree_stats_download(khg_ctx *ctx, const khg_tree_stats *s, int32_t *keys_h, double *count_h, double *x_h, double *x2_h);
int khg_tree_stats_upload(khg_ctx *ctx, khg_tree_stats *s, int64_t num_keys, const int32_t *keys_h, const double *count_h, const double *x_h,
                          const double *x2_h);
int khg_tree_stats_add(khg_ctx *ctx, khg_tree_stats *dst, float scale, const khg_tree_stats *src);
/* acc-tree-stats from the set's resident alignment (khg_align, khg_ali_upload) and feature rows; no model, no posteriors.
 * tid2phone_h / tid2pdf_class_h / tid_flags_h: [num_tids + 1], index 0 unused.  ci_phones_h[n_ci]: context-independent phones.
 * Segments: an utterance's ids are cut where a non-self-loop id follows a final one as its nearest preceding non-self-loop id (and at
 * frame 0) -- Kaldi's SplitToPhones for reordered graphs.  Segment i of S has the phone of its ids; a frame of it has
 * window[j] = phone of segment i - P + j (0 outside 0 .. S - 1; 0 for every j != P when the central phone is context-independent) and
 * the pdf-class of its own id, and adds count += 1, x += row, x2 += row^2 with the float row widened to double (exact products).
 * An utterance with KHG_TREE_STATUS_* set in status_h[n_utt] (may be NULL) adds nothing; the others add what they add without it, bit
 * for bit.  The sum of a key with n entries, in sorted (utterance, frame) order: slices of 1024 consecutive entries; in a slice, with
 * R = 256 / dim chains (1 for dim > 256), chain r adds entries r, r + R, .. in order, the chains are added in order 0 .. R - 1; the
 * slices are added in slice order (for n <= R that is 0 + x_0 + .. + x_(n-1) in entry order).  No atomics: the bits depend on the key's own entry list only.  A call into a handle that holds
 * keys merges as khg_tree_stats_add(handle, 1, the call's sums).  Reads back the key ranges for its work plan (synchronises). */
int khg_acc_tree_stats(khg_ctx *ctx, khg_utts *u, int32_t num_tids, const int32_t *tid2phone_h, const int32_t *tid2pdf_class_h,
                       const int32_t *tid_flags_h, int32_t n_ci, const int32_t *ci_phones_h, khg_tree_stats *stats, int32_t *status_h);
/* Kaldi's BuildTree on host statistics laid out as khg_tree_stats_download gives them; needs no device.  Questions: for question key
 * qkey_h[i] (-1 = the pdf-class, 0 .. N - 1 a window position; ascending, each once) the sets number qkey_off_h[i] ..
 * qkey_off_h[i + 1]; set q holds q_vals_h[q_off_h[q] .. q_off_h[q + 1]).  Roots: phone set r holds set_phones_h[set_off_h[r] ..
 * set_off_h[r + 1]) (sorted), with share_roots_h[r] and do_split_h[r]; phone2num_pdf_classes_h[num_phones].  GetStubMap, then
 * best-first splitting (improvement Objf(yes) + Objf(no) - Objf(leaf) of the diagonal Gaussian with variance floor var_floor, in
 * double; a question with an empty side is no candidate; first candidate wins ties; stops at improvement <= thresh or at max_leaves
 * leaves, max_leaves <= 0: no limit), then merging of leaves under one stub leaf while the smallest loss is < cluster_thresh
 * (cluster_thresh < 0: the smallest improvement split on; the merged leaf keeps the lower id) and renumbering.  The tree is written
 * as Kaldi's binary ContextDependency stream: *tree_bytes is always set; the stream is copied when tree_h holds tree_cap >= that.
 * Nothing is kept between calls: a call with tree_h == NULL (or too small a buffer) is a size query that costs a full build, so a
 * caller that can bound the stream -- <= 48 + 4 (largest question) bytes a split, 8 a leaf, the stub's nodes -- passes that once.
 * *objf_impr: the improvements split on, summed; *cluster_loss: the losses merged on, summed; *num_leaves; *num_removed merges.
 * KHG_E_ARG for malformed arguments and for statistics whose central phone is in no phone set. */
int khg_build_tree(int32_t N, int32_t P, int32_t dim, int64_t num_keys, const int32_t *keys_h, const double *count_h, const double *x_h,
                   const double *x2_h, int32_t num_qkeys, const int32_t *qkey_h, const int64_t *qkey_off_h, const int64_t *q_off_h,
                   const int32_t *q_vals_h, int32_t num_sets, const int64_t *set_off_h, const int32_t *set_phones_h,
                   const int32_t *share_roots_h, const int32_t *do_split_h, int32_t num_phones, const int32_t *phone2num_pdf_classes_h,
                   double thresh, int32_t max_leaves, double cluster_thresh, double var_floor, unsigned char *tree_h, int64_t tree_cap,
                   int64_t *tree_bytes, double *objf_impr, double *cluster_loss, int32_t *num_leaves, int32_t *num_removed);

/* ---- CMVN and delta features (compute-cmvn-stats, apply-cmvn, add-deltas) ------------------------------------------- */
/* The reference has no feature pipeline: the rule in DESIGN.md 7p is the specification (tests/feat_ref.py restates it).  Notation:
 * dim = the set's feature dimension, utt2spk_h[u] = s in [0, n_spk) or < 0 for "no speaker" (per-utterance CMVN: utt2spk = 0 ..
 * n_utt - 1).  The delta kernel stages 64 rows of an utterance with a halo of order x window rows each side in LDS:
 * 4 (64 + 2 order window) dim bytes, at most KHG_FEAT_TILE_LDS_BYTES (dim 128, order 3, window 4 take 44 KiB); above:
 * KHG_E_UNSUPPORTED. */
#define KHG_FEAT_TILE_LDS_BYTES 65536
#define KHG_CMVN_OK 0            /* the normaliser was computed                                                          */
#define KHG_CMVN_NO_DATA 1       /* count < 1: offset 0, scale 1                                                         */
#define KHG_CMVN_NONFINITE 2     /* a scale or an offset that is NaN or infinite: offset 0, scale 1                      */
/* Kaldi's CMVN statistics for n_spk speakers, resident on the device, fp64, in Kaldi's layout stats[n_spk][2][dim + 1]:
 * [s][0][d] = sum x[d], [s][0][dim] = the frame count, [s][1][d] = sum x[d] x[d], [s][1][dim] = 0.  download synchronises (deferred
 * kernel errors: KHG_E_RUNTIME); upload replaces the contents.  add: dst += (double)scale * src elementwise (one product, one add),
 * asynchronous; the handles must agree in speakers and dimension and belong to `ctx` (KHG_E_ARG). */
typedef struct khg_cmvn_stats khg_cmvn_stats;
int khg_cmvn_stats_create(khg_ctx *ctx, int32_t n_spk, int32_t dim, khg_cmvn_stats **out);
int khg_cmvn_stats_destroy(khg_cmvn_stats *s);
int khg_cmvn_stats_zero(khg_ctx *ctx, khg_cmvn_stats *s);
int khg_cmvn_stats_download(khg_ctx *ctx, const khg_cmvn_stats *s, double *stats_h);
int khg_cmvn_stats_upload(khg_ctx *ctx, khg_cmvn_stats *s, const double *stats_h);
int khg_cmvn_stats_add(khg_ctx *ctx, khg_cmvn_stats *dst, float scale, const khg_cmvn_stats *src);
/* One 1024-frame slice of a speaker parks 2 dim doubles; a chunk of `frames` frames (default and most 2^24, at least one slice) holds
 * frames / 1024 slices, short ones counting as whole.  The statistics do not depend on it, bit for bit.
 * num_chunks: how many chunks the last accumulation into the handle ran (tests). */
int khg_cmvn_stats_set_chunk_frames(khg_cmvn_stats *s, int64_t frames);
int khg_cmvn_stats_num_chunks(const khg_cmvn_stats *s, int32_t *n_chunks);
/* compute-cmvn-stats on the set's resident rows.  Every row of an utterance with utt2spk_h[u] = s >= 0 adds, widened to double,
 * x[d] and x[d] x[d] (exact in a double) to speaker s, and 1 to its count.  The order of the sum is fixed by the speaker's own frame
 * list (its utterances in set order, frames ascending), cut every 1024 frames into slices.  A slice of n frames, with R = 256 / dim
 * chains (1 for dim > 256): chain r starts at +0 and adds frames r, r + R, .. of the slice in order; the R chains are added in order
 * 0 .. R - 1; the slices are added in slice order, starting from +0.  No atomics: a speaker's statistics have the same bits whatever
 * else is in the call, whatever the chunk size, and from run to run.  An utterance with utt2spk < 0 and one without frames add
 * nothing.  Adds the call's sums into `stats`; asynchronous on the context's stream once the plan is uploaded.  Before anything is
 * launched (the handle keeps its bits): KHG_E_ARG for a utt2spk value >= n_spk, statistics of another dimension or context. */
int khg_acc_cmvn_stats(khg_ctx *ctx, khg_utts *u, const int32_t *utt2spk_h, khg_cmvn_stats *stats);
/* Kaldi's ApplyCmvn normaliser from host statistics laid out as khg_cmvn_stats_download gives them; needs no device.  In double, one
 * operation at a time: count = stats[s][0][dim], mean = stats[s][0][d] / count; without norm_vars scale = 1, offset = -mean; with it
 * var = stats[s][1][d] / count - mean mean, raised to the floor 1e-20, scale = 1 / sqrt(var), offset = -(mean scale); with reverse
 * scale = sqrt(var) (1 without norm_vars), offset = mean.  norm_means == 0 (Kaldi's --norm-means=false) leaves the mean in: the
 * offset is 0 and the scale and the status are what they are with norm_means (the variance is taken about the true mean).  Both narrowed to float: norm_h[n_spk][2][dim], [s][0][d] = offset, [s][1][d] =
 * scale.  status_h[n_spk] (may be NULL): KHG_CMVN_*; a speaker that is not OK gets offset 0 and scale 1 and is to be treated as
 * utt2spk < 0 (khg_utts_apply_cmvn and khg_utts_add_deltas do so when given the statuses). */
int khg_cmvn_compute(int32_t n_spk, int32_t dim, const double *stats_h, int32_t norm_means, int32_t norm_vars, int32_t reverse,
                     float *norm_h, int32_t *status_h);
/* Kaldi's DeltaFeatures coefficient tables, in float: scales[0] = [1]; for order i, with prev = scales[i - 1] of half-width po, cur
 * of half-width po + window starts at 0, normalizer = 0; for j = -window .. window ascending: normalizer += (float)(j j), and for
 * k = -po .. po ascending: cur[j + k] += (float)j * prev[k] (one float product, one float add); then every element is multiplied by
 * (float)(1.0 / normalizer).  scales_h: the tables one after the other, table i of 2 i window + 1 floats at offset
 * i + window i (i - 1): (order + 1) + window order (order + 1) floats.  KHG_E_ARG for order < 0 or window < 1.  Host only. */
int khg_delta_scales(int32_t order, int32_t window, float *scales_h);
/* apply-cmvn on the set's resident rows: y = fl(fl(x scale) + offset) in float, two roundings, never fused, with the normaliser
 * norm_h[n_spk][2][dim] of the utterance's speaker.  An utterance with utt2spk_h[u] < 0, or whose speaker's status_h (may be NULL:
 * every speaker OK) is not KHG_CMVN_OK, is copied bit for bit.  With out_d the rows go to that device buffer (the set's size) and
 * the set is untouched; with out_d == NULL the set's own rows are rewritten in place (borrowed device features included) and the
 * set is told so, as by khg_utts_features_changed.  It stages nothing: any dim.  KHG_E_ARG for a utt2spk value >= n_spk.
 * Synchronous. */
int khg_utts_apply_cmvn(khg_ctx *ctx, khg_utts *u, int32_t n_spk, const int32_t *utt2spk_h, const float *norm_h, const int32_t *status_h,
                        float *out_d);
/* add-deltas on the set's resident rows, out of place: for frame t of an utterance of T frames, block i = 0 .. order, H_i = i window:
 * out[t][i dim + d] = y with y = 0, then for j = -H_i .. H_i ascending and scales[i][j] != 0: y = fmaf(scales[i][j],
 * v[clamp(t + j, 0, T - 1)][d], y) -- zero coefficients are skipped, not multiplied; the clamp is inside the utterance, a
 * neighbouring utterance's row is never read.  v = x, or with norm_h != NULL the CMVN value of x as khg_utts_apply_cmvn forms it
 * (n_spk, utt2spk_h, status_h as there; all ignored with norm_h == NULL), applied while the tile is staged and never written to
 * memory.  out_d: a caller-owned device buffer of [rows of the set][dim (order + 1)] floats; the set is untouched.  KHG_E_ARG for
 * order < 0, window < 1, a utt2spk value >= n_spk; KHG_E_UNSUPPORTED, naming the limit, above KHG_FEAT_TILE_LDS_BYTES.  Synchronous. */
int khg_utts_add_deltas(khg_ctx *ctx, khg_utts *u, int32_t order, int32_t window, int32_t n_spk, const int32_t *utt2spk_h,
                        const float *norm_h, const int32_t *status_h, float *out_d);

/* ---- MFCC and filterbank features from waveforms (compute-mfcc-feats, compute-fbank-feats) --------------------------- */
#define KHG_FE_MFCC 0
#define KHG_FE_FBANK 1
#define KHG_WIN_POVEY 0
#define KHG_WIN_HAMMING 1
#define KHG_WIN_HANNING 2
#define KHG_WIN_RECTANGULAR 3
#define KHG_WIN_BLACKMAN 4
#define KHG_WAVE_F32 0           /* samples are float (Kaldi's scale: +-32768)                                           */
#define KHG_WAVE_I16 1           /* samples are int16, converted exactly                                                 */
#define KHG_FE_TILE_FRAMES 16    /* frames of one utterance that one workgroup takes                                     */
/* One struct for both tools, Kaldi's option names.  Refused with KHG_E_UNSUPPORTED, naming the option: dither != 0,
 * round_to_power_of_two == 0, vtln_warp != 1, htk_compat != 0, a padded window outside {256, 512, 1024}, num_mel_bins outside
 * 3 .. 128, num_ceps > num_mel_bins (MFCC).  KHG_E_ARG for values that make no sense (an unknown kind or window, a frame shift
 * below one sample, a frame below two, low_freq / high_freq outside 0 .. Nyquist or crossed, a value that is not finite). */
typedef struct khg_frontend_opts {
  int32_t kind;                  /* KHG_FE_MFCC                                                                           */
  float samp_freq;               /* 16000                                                                                 */
  float frame_length_ms;         /* 25                                                                                    */
  float frame_shift_ms;          /* 10                                                                                    */
  float preemph_coeff;           /* 0.97                                                                                  */
  int32_t remove_dc_offset;      /* 1                                                                                     */
  int32_t window_type;           /* KHG_WIN_POVEY                                                                         */
  float blackman_coeff;          /* 0.42                                                                                  */
  int32_t snip_edges;            /* 1                                                                                     */
  int32_t round_to_power_of_two; /* 1 (0: refused)                                                                        */
  float dither;                  /* 0 (Kaldi: 1; anything else than 0 is refused -- dither is random)                     */
  int32_t num_mel_bins;          /* 23                                                                                    */
  float low_freq;                /* 20                                                                                    */
  float high_freq;               /* 0: Nyquist; <= 0: Nyquist is added                                                    */
  float vtln_warp;               /* 1 (anything else: refused)                                                            */
  int32_t htk_compat;            /* 0 (1: refused)                                                                        */
  int32_t num_ceps;              /* 13 (MFCC)                                                                             */
  float cepstral_lifter;         /* 22 (MFCC; 0: none)                                                                    */
  int32_t use_energy;            /* 0: MFCC keeps C0, FBANK has no energy column; 1: column 0 is the log-energy           */
  int32_t raw_energy;            /* 1: the energy before pre-emphasis and windowing                                       */
  float energy_floor;            /* 0: none                                                                               */
  int32_t use_log_fbank;         /* 1 (FBANK)                                                                             */
  int32_t use_power;             /* 1 (FBANK; 0: the magnitude spectrum)                                                  */
} khg_frontend_opts;
void khg_frontend_opts_default(khg_frontend_opts *o);
/* The sizes the options imply; host only.  dims_h[8]: L (samples of a frame), S (samples of a shift), N (the padded window), the
 * number of mel bins, of cepstra (0 for FBANK), of output columns, of mel weights (the sum of the filters' lengths), 0. */
int khg_frontend_dims(const khg_frontend_opts *o, int32_t *dims_h);
/* Frames of an utterance of n_samples; host only.  snip_edges: 0 below L, else 1 + (n - L) / S; otherwise (n + S / 2) / S. */
int khg_frontend_num_frames(const khg_frontend_opts *o, int64_t n_samples, int64_t *num_frames);
/* The tables of DESIGN.md 7q, computed in double and narrowed once; host only.  Every buffer may be NULL.  window_h[L], mel_off_h /
 * mel_len_h[bins] (a filter's first spectrum bin and its run), mel_w_h[sum of the lengths], dct_h[num_ceps][bins], lifter_h[num_ceps],
 * twiddle_h[N / 2][2] (cos, -sin of 2 pi k / N). */
int khg_frontend_tables(const khg_frontend_opts *o, float *window_h, int32_t *mel_off_h, int32_t *mel_len_h, float *mel_w_h, float *dct_h,
                        float *lifter_h, float *twiddle_h);
/* The tables resident on the device. */
typedef struct khg_frontend khg_frontend;
int khg_frontend_create(khg_ctx *ctx, const khg_frontend_opts *o, khg_frontend **out);
int khg_frontend_destroy(khg_frontend *fe);
/* Features of n_utt waveforms: utterance u owns samples [sample_off_h[u], sample_off_h[u + 1]) of samples_h (host) or samples_d
 * (device) -- exactly one of the two is given --, of sample_type KHG_WAVE_*.  frame_off_h[n_utt + 1] (out): the rows' prefix sums
 * (khg_frontend_num_frames of every utterance); out_d: a caller-owned device buffer of [rows][output columns] floats.  With
 * out_d == NULL only frame_off_h is filled, so that the caller can size the buffer.  A frame depends on its own samples only
 * (reflected inside its utterance without snip_edges): its bits are the same alone and in any batch.  Every refusal comes before
 * any launch and leaves out_d untouched.  Synchronous. */
int khg_frontend_compute(khg_ctx *ctx, khg_frontend *fe, int32_t n_utt, const int64_t *sample_off_h, const void *samples_h, const void *samples_d,
                         int32_t sample_type, int64_t *frame_off_h, float *out_d);

#ifdef __cplusplus
}
#endif
#endif /* KHG_HIP_H_ */
