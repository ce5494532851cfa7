"""kaldi_hmm_gmm_amd -- MI355X-native HMM-GMM EM hot path (K1 log-likes on the fp16 matrix cores at fp32 accuracy, K2 Viterbi
forced alignment, K3 sufficient statistics (posteriors on fp16 / fp32 MFMA, sums on fp64 MFMA), K4 device M-step, C1 RCCL sum) behind the names of the reference's
pybind11 module `kaldi_hmm_gmm` (python/kaldi_hmm_gmm/__init__.py) and of its scripts/*.py.

Importing this package loads libkhg_hip.so; there is no CPU fallback."""
from . import _lib  # noqa: F401  (fails loudly when libkhg_hip.so is missing)
from ._lib import KhgError  # noqa: F401
from .align import (AlignConfig, DecodableAmDiagGmmScaled, DecodableAmDiagGmmUnmapped, DecodableInterface, FasterDecoder,  # noqa: F401
                    FasterDecoderOptions, LatticeArc, LatticeWeight, LinearLattice, add_transition_probs, align_batch,
                    align_utterance_wrapper)
from .align import (DeterminizeLatticePhonePrunedOptions, LatticeFasterDecoder, LatticeFasterDecoderConfig,  # noqa: F401
                    LatticeFasterDecoderStdVectorFst, decode_lattice_faster_batch, decode_utterance_lattice_faster)
from .align import (DecodableCtc, LatticeSimpleDecoder, LatticeSimpleDecoderConfig, decode_lattice_simple_batch,  # noqa: F401
                    decode_utterance_lattice_simple)
from .align import Lattice, get_raw_lattice_simple_batch  # noqa: F401
from .align import DeviceLattices, get_raw_lattice_simple_device_batch  # noqa: F401
from .align import DevicePosteriors  # noqa: F401
from .align import DeviceLm  # noqa: F401
from .lm import NgramLm, estimate_ngram_lm  # noqa: F401
from .score import (compute_wer, edit_distance_counts, lattice_add_penalty, lattice_add_penalty_batch, lattice_oracle,  # noqa: F401
                    lattice_oracle_batch, score_lattices)
from .score import lattice_mbr_decode, lattice_mbr_decode_batch, mbr_utterances  # noqa: F401
from .align import get_raw_lattice_faster_batch, get_raw_lattice_faster_device_batch  # noqa: F401
from .determinize import (get_lattice_faster_batch, get_lattice_faster_device_batch, lattice_determinize_pruned,  # noqa: F401
                          lattice_determinize_pruned_batch)
from .nbest import KHG_NBEST_MAX, DeviceNbest, NbestList, lattice_to_nbest, lattice_to_nbest_batch  # noqa: F401
from .context_dep import (ContextDependency, ContextDependencyInterface, monophone_context_dependency,  # noqa: F401
                          monophone_context_dependency_shared)
from .device import (ALIGN_DONE, ALIGN_ERROR, ALIGN_EXACT_DP, ALIGN_FALLBACK, ALIGN_RETRIED, Comm, Context, DeviceAccs,  # noqa: F401
                     DecodingGraph, DeviceCmvnStats, DeviceFmllrStats, DeviceLdaStats, DeviceMlltStats, DeviceModel, DeviceTransitions, DeviceTreeStats,
                     UtteranceSet, k3_forms)
from .diag_gmm import AmDiagGmm, DiagGmm  # noqa: F401
from .fst import StdArc, StdVectorFst, modify_graph_for_careful_alignment  # noqa: F401
from .hmm_topology import HmmState, HmmTopology  # noqa: F401
from .mle import (kGmmAll, kGmmMeans, kGmmTransitions, kGmmVariances, kGmmWeights)  # noqa: F401  (py::enum_::export_values, model-common.cc:12-20)
from .mle import (AccumAmDiagGmm, AccumDiagGmm, GmmUpdateFlags, MapDiagGmmOptions, MleDiagGmmOptions, augment_gmm_flags,  # noqa: F401
                  get_split_targets, gmm_flags_to_str, map_am_diag_gmm_update, map_diag_gmm_update, ml_objective, mle_am_diag_gmm_update,
                  mle_am_diag_gmm_update_device, mle_diag_gmm_update,
                  str_to_gmm_flags)
from .mle import (EbwOptions, EbwWeightOptions, ebw_am_diag_gmm_update_device, update_ebw_am_diag_gmm, update_ebw_diag_gmm,  # noqa: F401
                  update_ebw_weights_am_diag_gmm, update_ebw_weights_diag_gmm)
from .resident import ResidentEm  # noqa: F401
from .posterior import ali_to_post, arrays_to_posts, posts_to_arrays  # noqa: F401
from .fmllr import (FMLLR_LOW_COUNT, FMLLR_MAX_DIM, FMLLR_OK, FMLLR_SINGULAR, compose_transforms, fmllr_compute, gmm_est_fmllr,  # noqa: F401
                    gmm_est_fmllr_batch, spk2utt, transform_feats, transform_feats_batch, utt2spk_ids, weight_silence_post)
from .mllt import (MLLT_MAX_DIM, MLLT_OK, MLLT_SINGULAR, est_mllt, gmm_acc_mllt, gmm_acc_mllt_batch, gmm_transform_means,  # noqa: F401
                   mllt_compute)
from .lda import (LDA_MAX_SPLICED_DIM, LDA_OK, LDA_SINGULAR, acc_lda, acc_lda_batch, compose_with_lda, est_lda, lda_compute,  # noqa: F401
                  splice_feats, splice_transform_feats, splice_transform_feats_batch)
from .feat import (CMVN_NO_DATA, CMVN_NONFINITE, CMVN_OK, FEAT_TILE_LDS_BYTES, add_deltas, add_deltas_batch, apply_cmvn,  # noqa: F401
                   apply_cmvn_batch, cmvn_compute, compute_cmvn_stats, compute_cmvn_stats_batch, delta_scales)
from .wave import (FE_FBANK, FE_MFCC, FE_TILE_FRAMES, WAVE_F32, WAVE_I16, WIN_BLACKMAN, WIN_HAMMING, WIN_HANNING, WIN_POVEY,  # noqa: F401
                   WIN_RECTANGULAR, DeviceFrontend, FrontendOptions, compute_fbank_feats, compute_fbank_feats_batch, compute_mfcc_feats,
                   compute_mfcc_feats_batch, frame_offsets, frame_starts, frontend_dims, frontend_tables, num_frames)
from .tree import (TREE_MAX_CONTEXT, TREE_MAX_PDF_CLASS, TREE_MAX_PHONE, TREE_STATUS_MIXED_PHONES, TREE_STATUS_NO_ALI,  # noqa: F401
                   TREE_STATUS_OPEN_END, acc_tree_stats, acc_tree_stats_batch, build_tree, convert_ali, gmm_init_model, leaf_stats,
                   pdf_class_questions, split_to_phones, tid_tables)
from .scripts import (gmm_acc_stats, gmm_acc_stats_ali, gmm_acc_stats_ali_batch, gmm_acc_stats_batch, gmm_align_compiled,  # noqa: F401
                      gmm_align_compiled_batch, gmm_boost_silence, gmm_est, gmm_est_gmm_ebw, gmm_est_weights_ebw, gmm_info, gmm_init_mono,
                      gmm_ismooth_stats, gmm_rescore_lattice, gmm_rescore_lattice_batch, gmm_sum_accs, lattice_boost_ali,
                      lattice_boost_ali_batch, gmm_acc_stats2, gmm_acc_stats2_batch, lattice_to_mpe_post, lattice_to_mpe_post_batch,
                      lattice_to_smbr_post, lattice_to_smbr_post_batch, lattice_lmrescore, lattice_lmrescore_batch)
from .training_graph import (TrainingGraphCompiler, TrainingGraphCompilerOptions, equal_align, generate_hmm_topo,  # noqa: F401
                             make_lexicon_fst_with_silence)
from .transition_model import (MleTransitionUpdateConfig, TransitionInformation, TransitionModel, TransitionModelTuple,  # noqa: F401
                               get_pdfs_for_phones)
