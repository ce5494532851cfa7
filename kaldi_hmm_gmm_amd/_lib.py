"""ctypes binding of libkhg_hip.so (C-ABI: include/khg_hip.h).

The library is the product: there is no Python/CPU fallback.  If it is missing the import
fails loudly; if no gfx950 GPU is present every compute call raises (khg_ctx_create fails).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KHG_LIBRARY") or os.path.join(_HERE, "libkhg_hip.so")   # KHG_LIBRARY: A/B builds (ctypes binding only)


class KhgError(RuntimeError):
    """Mirror of the reference's std::runtime_error -> Python RuntimeError (csrc/log.h:46-53)."""


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). kaldi_hmm_gmm_amd has no CPU fallback."
        )
    # One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same
    # SONAME as /opt/rocm's, which this library is linked against).  Loaded torch-first, the dynamic linker resolves
    # our libamdhip64.so.7 to the copy already in the process and everything shares one runtime (streams, RCCL
    # tensors aliasing our buffers).  Loaded the other way round, torch later brings in its bundled copy as a SECOND
    # runtime, whose HSA layer cannot open the device any more ("No HIP GPUs are available").  So when torch is
    # installed, let it load its runtime first; without torch the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    return C.CDLL(LIB_PATH)


lib = _load()

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_u8p = C.POINTER(C.c_uint8)
vp = C.c_void_p


class AlignConfigC(C.Structure):
    _fields_ = [
        ("beam", C.c_float),
        ("retry_beam", C.c_float),
        ("careful", C.c_int32),
        ("acoustic_scale", C.c_float),
        ("max_active", C.c_int32),
        ("min_active", C.c_int32),
        ("beam_delta", C.c_float),
        ("hash_ratio", C.c_float),
        ("like_scale", C.c_float),
    ]


class LatticeFasterConfigC(C.Structure):
    _fields_ = [
        ("beam", C.c_float),
        ("max_active", C.c_int32),
        ("min_active", C.c_int32),
        ("lattice_beam", C.c_float),
        ("prune_interval", C.c_int32),
        ("beam_delta", C.c_float),
        ("hash_ratio", C.c_float),
        ("prune_scale", C.c_float),
        ("acoustic_scale", C.c_float),
        ("allow_partial", C.c_int32),
        ("scratch_per_frame", C.c_int32),
    ]


class LatticeSimpleConfigC(C.Structure):
    _fields_ = [
        ("beam", C.c_float),
        ("lattice_beam", C.c_float),
        ("prune_interval", C.c_int32),
        ("prune_scale", C.c_float),
        ("acoustic_scale", C.c_float),
        ("allow_partial", C.c_int32),
        ("scratch_per_frame", C.c_int32),
    ]


class MleOptionsC(C.Structure):
    _fields_ = [
        ("min_gaussian_weight", C.c_float),
        ("min_gaussian_occupancy", C.c_float),
        ("min_variance", C.c_double),
        ("remove_low_count_gaussians", C.c_int32),
        ("variance_floor_vector", C.POINTER(C.c_double)),
    ]


class EbwOptionsC(C.Structure):
    _fields_ = [("E", C.c_double), ("tau", C.c_double)]


class EbwWeightOptionsC(C.Structure):
    _fields_ = [("min_num_count_weight_update", C.c_double), ("min_gaussian_weight", C.c_double), ("tau", C.c_double)]


class EbwResultsC(C.Structure):
    _fields_ = [("auxf_impr_gauss", C.c_double), ("count", C.c_double), ("auxf_impr_weights", C.c_double), ("floored", C.c_int32),
                ("failed", C.c_int32), ("skipped", C.c_int32), ("weights_skipped", C.c_int32)]


class FmllrOptionsC(C.Structure):
    _fields_ = [("min_count", C.c_double), ("num_iters", C.c_int32)]


class MlltOptionsC(C.Structure):
    _fields_ = [("num_iters", C.c_int32)]


class LdaOptionsC(C.Structure):
    _fields_ = [("target_dim", C.c_int32), ("remove_offset", C.c_int32), ("within_class_factor", C.c_double)]


class FrontendOptsC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("samp_freq", C.c_float), ("frame_length_ms", C.c_float), ("frame_shift_ms", C.c_float), ("preemph_coeff", C.c_float),
                ("remove_dc_offset", C.c_int32), ("window_type", C.c_int32), ("blackman_coeff", C.c_float), ("snip_edges", C.c_int32),
                ("round_to_power_of_two", C.c_int32), ("dither", C.c_float), ("num_mel_bins", C.c_int32), ("low_freq", C.c_float), ("high_freq", C.c_float),
                ("vtln_warp", C.c_float), ("htk_compat", C.c_int32), ("num_ceps", C.c_int32), ("cepstral_lifter", C.c_float), ("use_energy", C.c_int32),
                ("raw_energy", C.c_int32), ("energy_floor", C.c_float), ("use_log_fbank", C.c_int32), ("use_power", C.c_int32)]


class RescoreStatsC(C.Structure):
    _fields_ = [("arcs", C.c_int64), ("emitting_arcs", C.c_int64), ("cells", C.c_int64)]


class LmRescoreStatsC(C.Structure):
    _fields_ = [("in_states", C.c_int64), ("in_arcs", C.c_int64), ("out_states", C.c_int64), ("out_arcs", C.c_int64), ("max_hist", C.c_int64)]


class DetStatsC(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("in_states", "in_arcs", "pruned_states", "det_states", "out_states", "out_arcs", "max_subset", "max_closure")]


# every symbol include/khg_hip.h declares: (restype, argtypes)
SIGNATURES = {
    "khg_last_error": (C.c_char_p, []),
    "khg_version": (C.c_int, []),
    "khg_ctx_create": (C.c_int, [C.c_int, vp, C.POINTER(vp)]),
    "khg_ctx_destroy": (C.c_int, [vp]),
    "khg_ctx_sync": (C.c_int, [vp]),
    "khg_ctx_set_timing": (C.c_int, [vp, C.c_int]),
    "khg_ctx_set_k1_form": (C.c_int, [vp, C.c_int]),
    "khg_ctx_set_option": (C.c_int, [vp, C.c_int, C.c_int]),
    "khg_ctx_get_option": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
    "khg_option_check": (C.c_int, [C.c_int, C.c_int]),
    "khg_option_from_env": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "khg_ctx_get_timings": (C.c_int, [vp, C.c_char_p, C.c_int64, c_f32p, C.c_int32, c_i32p]),
    "khg_model_create": (C.c_int, [vp, C.c_int32, C.c_int32, c_i32p, c_f32p, c_f32p, c_f32p, C.POINTER(vp)]),
    "khg_model_destroy": (C.c_int, [vp]),
    "khg_tm_create": (C.c_int, [vp, C.c_int32, c_i32p, C.POINTER(vp)]),
    "khg_tm_set_trans_cost": (C.c_int, [vp, c_f32p]),
    "khg_tm_destroy": (C.c_int, [vp]),
    "khg_utts_create": (
        C.c_int,
        [vp, vp, C.c_int32, C.c_int32, c_i64p, c_f32p, vp, c_i64p, c_i32p, c_i64p, c_i32p, c_i32p, c_f32p, c_i32p,
         c_f32p, C.POINTER(vp)],
    ),
    "khg_utts_destroy": (C.c_int, [vp]),
    "khg_graph_create": (C.c_int, [vp, vp, C.c_int32, C.c_int32, c_i64p, c_i32p, c_i32p, c_f32p, c_i32p, c_f32p, C.POINTER(vp)]),
    "khg_graph_destroy": (C.c_int, [vp]),
    "khg_graph_info": (C.c_int, [vp, c_i64p, c_i64p, c_i32p, c_i32p, c_i64p]),
    "khg_utts_create_on_graph": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, c_i64p, c_f32p, vp, C.POINTER(vp)]),
    "khg_utts_graph_bytes": (C.c_int, [vp, c_i64p]),
    "khg_utts_num_pdfs": (C.c_int, [vp, c_i64p]),
    "khg_utts_pdfs": (C.c_int, [vp, c_i32p]),
    "khg_utts_k2_plan": (C.c_int, [vp, vp, c_i32p]),
    "khg_utts_k2_ladder": (C.c_int, [vp, vp, c_i32p]),
    "khg_utts_k3_planes": (C.c_int, [vp, c_i64p, c_i64p, c_i32p]),
    "khg_k3_forms": (C.c_int, [c_i32p, C.c_int32, c_i32p]),
    "khg_utts_k3_last": (C.c_int, [vp, c_i32p, c_i32p]),
    "khg_utts_k1_last": (C.c_int, [vp, c_i32p]),
    "khg_utts_k2_tail": (C.c_int, [vp, c_i32p, C.c_int64]),
    "khg_utts_pdf_first": (C.c_int, [vp, c_i32p]),
    "khg_loglikes": (C.c_int, [vp, vp, vp]),
    "khg_loglikes_reachable": (C.c_int, [vp, vp, vp]),
    "khg_loglikes_band": (C.c_int, [vp, vp, vp]),
    "khg_utts_pdf_last": (C.c_int, [vp, c_i32p]),
    "khg_loglikes_layout": (C.c_int, [vp, c_i64p, c_i64p]),
    "khg_loglikes_download": (C.c_int, [vp, vp, c_f32p]),
    "khg_loglikes_upload": (C.c_int, [vp, vp, c_f32p]),
    "khg_utts_set_pdf_list": (C.c_int, [vp, C.c_int32, c_i32p]),
    "khg_utts_features_changed": (C.c_int, [vp]),
    "khg_comm_info": (C.c_int, [vp, c_i32p, c_i32p, c_i32p]),
    "khg_align_config_default": (None, [C.POINTER(AlignConfigC)]),
    "khg_align": (C.c_int, [vp, vp, vp, C.POINTER(AlignConfigC), c_i32p, c_i32p, c_i64p, C.c_int64, c_f32p, c_i32p]),
    "khg_ali_upload": (C.c_int, [vp, vp, c_i32p]),
    "khg_lattice_faster_config_default": (None, [C.POINTER(LatticeFasterConfigC)]),
    "khg_decode_lattice_faster": (C.c_int, [vp, vp, vp, C.POINTER(LatticeFasterConfigC), c_i32p, c_i32p, c_i64p, C.c_int64, c_f64p,
                                            c_i32p]),
    "khg_lattice_simple_config_default": (None, [C.POINTER(LatticeSimpleConfigC)]),
    "khg_decode_lattice_simple": (C.c_int, [vp, vp, vp, C.POINTER(LatticeSimpleConfigC), c_i32p, c_i32p, c_i64p, C.c_int64, c_f64p,
                                            c_i32p, c_i32p]),
    "khg_decode_lattice_simple_raw": (C.c_int, [vp, vp, vp, C.POINTER(LatticeSimpleConfigC), c_i32p, c_i32p, c_i64p, C.c_int64, c_f64p,
                                                c_i32p, c_i32p, C.POINTER(vp)]),
    "khg_decode_lattice_faster_raw": (C.c_int, [vp, vp, vp, C.POINTER(LatticeFasterConfigC), c_i32p, c_i32p, c_i64p, C.c_int64, c_f64p,
                                                c_i32p, C.POINTER(vp)]),
    "khg_lattices_sizes": (C.c_int, [vp, c_i64p, c_i64p]),
    "khg_lattices_download": (C.c_int, [vp, vp, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p, c_f32p, c_f32p, c_i32p,
                                        c_i32p]),
    "khg_lattices_device_bytes": (C.c_int, [vp, c_i64p]),
    "khg_lattices_destroy": (C.c_int, [vp]),
    "khg_lattices_validate": (C.c_int, [C.c_int32, c_i64p, c_i64p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p, c_f32p,
                                        c_f32p, c_i32p, c_i32p]),
    "khg_lattices_upload": (C.c_int, [vp, C.c_int32, c_i64p, c_i64p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p, c_f32p,
                                      c_f32p, c_i32p, c_i32p, C.POINTER(vp)]),
    "khg_lattices_num_utts": (C.c_int, [vp, c_i32p]),
    "khg_lattices_ali_layout": (C.c_int, [vp, vp, c_i64p]),
    "khg_lattices_num_chunks": (C.c_int, [vp, c_i32p]),
    "khg_lattices_chunk_utts": (C.c_int, [vp, c_i32p]),
    "khg_lattices_best_path": (C.c_int, [vp, vp, C.c_int32, c_f32p, c_f32p, c_i32p, c_i32p, c_i64p, C.c_int64, c_f32p, c_i32p]),
    "khg_lattices_prune": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_float, c_i32p, C.POINTER(vp)]),
    "khg_lattices_posteriors": (C.c_int, [vp, vp, C.c_float, C.c_float, c_i32p, c_f64p, C.POINTER(vp)]),
    "khg_lattices_rescore": (C.c_int, [vp, vp, vp, vp, vp, C.c_float, C.c_int, C.POINTER(RescoreStatsC), C.POINTER(vp)]),
    "khg_lattices_op_status": (C.c_int, [vp, c_i32p]),
    "khg_lattices_boost": (C.c_int, [vp, vp, C.c_int32, c_i32p, C.c_int32, c_i32p, c_i64p, c_i32p, vp, C.c_float, C.c_float, c_i32p,
                                     C.POINTER(vp)]),
    "khg_lm_validate": (C.c_int, [C.c_int32, c_i32p, c_f32p, c_i32p, c_i32p, c_f32p, c_i32p, c_f32p, C.c_int32]),
    "khg_lm_create": (C.c_int, [vp, C.c_int32, c_i32p, c_f32p, c_i32p, c_i32p, c_f32p, c_i32p, c_f32p, C.c_int32, C.POINTER(vp)]),
    "khg_lm_destroy": (C.c_int, [vp]),
    "khg_lm_num_states": (C.c_int, [vp, c_i32p]),
    "khg_lm_device_bytes": (C.c_int, [vp, c_i64p]),
    "khg_lm_score": (C.c_int, [C.c_int32, c_i32p, c_f32p, c_i32p, c_i32p, c_f32p, c_i32p, c_f32p, C.c_int32, C.c_int32, c_i32p, c_f32p]),
    "khg_lattices_lm_rescore": (C.c_int, [vp, vp, vp, C.c_float, C.c_int32, c_i32p, C.POINTER(LmRescoreStatsC), C.POINTER(vp)]),
    "khg_lattices_determinize": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, c_i32p, C.POINTER(DetStatsC), C.POINTER(vp)]),
    "khg_lattices_add_penalty": (C.c_int, [vp, vp, C.c_float, C.POINTER(vp)]),
    "khg_lattices_oracle": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_i64p, C.c_int64, c_i32p, c_i32p, c_i64p, C.c_int64, c_i32p, c_i32p]),
    "khg_lattices_wer": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_i64p, C.c_int32, c_f32p, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p]),
    "khg_edit_distance": (C.c_int, [C.c_int32, c_i32p, c_i64p, c_i32p, c_i64p, c_i32p]),
    "khg_lattices_mbr": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_i64p, c_i32p, C.c_int32, C.c_int64,
                                   C.POINTER(vp)]),
    "khg_mbr_sizes": (C.c_int, [vp, c_i64p, c_i64p, c_i64p]),
    "khg_mbr_download": (C.c_int, [vp, vp, c_i32p, c_i32p, c_f64p, c_i32p, c_f64p, c_i32p, c_f64p, c_f64p, c_f64p]),
    "khg_mbr_device_bytes": (C.c_int, [vp, c_i64p]),
    "khg_mbr_destroy": (C.c_int, [vp]),
    "khg_lattices_nbest": (C.c_int, [vp, vp, C.c_float, C.c_float, C.c_int32, c_i32p, C.POINTER(vp)]),
    "khg_nbest_sizes": (C.c_int, [vp, c_i64p, c_i64p]),
    "khg_nbest_download": (C.c_int, [vp, vp, c_i32p, c_i32p, c_f32p, c_f32p]),
    "khg_nbest_device_bytes": (C.c_int, [vp, c_i64p]),
    "khg_nbest_destroy": (C.c_int, [vp]),
    "khg_lattices_mpe_posteriors": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_i32p, C.c_int32, c_i32p, c_i64p, c_i32p, vp, C.c_int32, C.c_int32,
                                              C.c_float, C.c_float, c_i32p, c_f64p, c_f64p, C.POINTER(vp)]),
    "khg_posteriors_sizes": (C.c_int, [vp, c_i64p, c_i64p]),
    "khg_posteriors_download": (C.c_int, [vp, vp, c_i64p, c_i32p, c_f64p, c_f64p]),
    "khg_posteriors_device_bytes": (C.c_int, [vp, c_i64p]),
    "khg_posteriors_destroy": (C.c_int, [vp]),
    "khg_posteriors_validate": (C.c_int, [C.c_int32, c_i64p, c_i64p, C.c_int64, c_i32p, c_f64p]),
    "khg_posteriors_upload": (C.c_int, [vp, C.c_int32, c_i64p, c_i64p, c_i32p, c_f64p, C.POINTER(vp)]),
    "khg_ali_download": (C.c_int, [vp, vp, c_i32p]),
    "khg_accs_create": (C.c_int, [vp, vp, vp, C.POINTER(vp)]),
    "khg_accs_destroy": (C.c_int, [vp]),
    "khg_accs_zero": (C.c_int, [vp, vp]),
    "khg_accs_size": (C.c_int, [vp, c_i64p]),
    "khg_accs_device_ptr": (C.c_int, [vp, C.POINTER(vp)]),
    "khg_accs_download": (C.c_int, [vp, vp, c_f64p]),
    "khg_accs_upload": (C.c_int, [vp, vp, c_f64p]),
    "khg_acc_stats": (C.c_int, [vp, vp, vp, vp, C.c_float, vp]),
    "khg_acc_stats_post": (C.c_int, [vp, vp, vp, vp, vp, C.c_float, vp]),
    "khg_acc_stats_post2": (C.c_int, [vp, vp, vp, vp, vp, C.c_float, vp, vp]),
    "khg_accs_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_accs_scale": (C.c_int, [vp, vp, C.c_float]),
    "khg_accs_smooth_with_accum": (C.c_int, [vp, vp, C.c_float, vp, vp, c_i32p]),
    "khg_accs_allreduce": (C.c_int, [vp, vp, vp]),
    "khg_accs_allreduce_range": (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, vp]),
    "khg_acc_stats_reduce": (C.c_int, [vp, vp, vp, vp, C.c_float, vp, vp, C.c_int32]),
    "khg_accs_allreduce_f32": (C.c_int, [vp, vp, vp]),
    "khg_comm_unique_id": (C.c_int, [vp]),
    "khg_comm_create": (C.c_int, [vp, C.c_int32, C.c_int32, vp, C.POINTER(vp)]),
    "khg_comm_destroy": (C.c_int, [vp]),
    "khg_compute_gconsts": (C.c_int, [C.c_int32, C.c_int32, c_i32p, c_f32p, c_f32p, c_f32p, c_f32p, c_i32p]),
    "khg_mle_options_default": (None, [C.POINTER(MleOptionsC)]),
    "khg_mle_am_diag_gmm_update": (
        C.c_int,
        [C.POINTER(MleOptionsC), C.c_int32, C.c_int32, c_i32p, c_f64p, c_f64p, c_f64p, C.c_uint16, C.c_uint16, c_f32p,
         c_f32p, c_f32p, c_f32p, c_i32p, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p],
    ),
    "khg_ebw_options_default": (None, [C.POINTER(EbwOptionsC)]),
    "khg_ebw_weight_options_default": (None, [C.POINTER(EbwWeightOptionsC)]),
    "khg_ebw_am_diag_gmm_update": (
        C.c_int,
        [C.POINTER(EbwOptionsC), C.POINTER(EbwWeightOptionsC), C.c_int32, C.c_int32, c_i32p, c_f64p, c_f64p, c_f64p, c_f64p, c_f64p,
         c_f64p, C.c_uint16, c_f32p, c_f32p, c_f32p, c_f32p, C.POINTER(EbwResultsC)],
    ),
    "khg_model_ebw_update": (C.c_int, [vp, vp, vp, vp, C.POINTER(EbwOptionsC), C.POINTER(EbwWeightOptionsC), C.c_uint16,
                                      C.POINTER(EbwResultsC)]),
    "khg_careful_graph": (C.c_int, [C.c_int32, C.c_int32, c_i64p, c_i32p, c_i32p, c_f32p, c_i32p, c_f32p, c_i32p, c_i32p, c_i64p, c_i32p,
                                    c_i32p, c_f32p, c_i32p, c_f32p]),
    "khg_diag_gmm_merge": (C.c_int, [c_i32p, C.c_int32, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, c_i32p, c_i32p]),
    "khg_model_set_weights": (C.c_int, [vp, vp, c_f32p]),
    "khg_model_mle_update": (C.c_int, [vp, vp, vp, C.POINTER(MleOptionsC), C.c_uint16, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p]),
    "khg_model_mle_update_sharded": (C.c_int, [vp, vp, vp, C.POINTER(MleOptionsC), C.c_uint16, vp, C.c_int32, C.c_int32, c_f32p, c_f32p,
                                              c_i32p, c_i32p, c_i32p]),
    "khg_model_mle_update_range": (C.c_int, [vp, vp, vp, C.POINTER(MleOptionsC), C.c_uint16, C.c_int32, C.c_int32]),
    "khg_model_mle_rows_download": (C.c_int, [vp, vp, C.c_int32, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, vp]),
    "khg_model_mle_rows_upload": (C.c_int, [vp, vp, C.c_int32, C.c_int32, c_f32p, c_f32p, c_f32p, c_f32p, vp]),
    "khg_model_mle_update_finish": (C.c_int, [vp, vp, c_f32p, c_f32p, c_i32p, c_i32p, c_i32p]),
    "khg_model_split": (C.c_int, [vp, vp, c_i32p, C.c_float, c_f32p, C.c_int64]),
    "khg_model_merge": (C.c_int, [vp, vp, c_i32p]),
    "khg_model_num_gauss": (C.c_int, [vp, C.POINTER(C.c_int64), c_i32p]),
    "khg_model_invalidate": (C.c_int, [vp]),
    "khg_model_download": (C.c_int, [vp, vp, c_f32p, c_f32p, c_f32p, c_f32p]),
    "khg_accs_relayout": (C.c_int, [vp, vp, vp]),
    "khg_accs_download_trans": (C.c_int, [vp, vp, c_f64p, c_f64p]),
    "khg_accs_download_range": (C.c_int, [vp, vp, C.c_int64, C.c_int64, c_f64p]),
    "khg_model_scale_weights": (C.c_int, [vp, vp, C.c_int32, c_i32p, C.c_float]),
    "khg_transition_mle_update": (
        C.c_int,
        [C.c_int32, c_i32p, c_i32p, c_f64p, C.c_float, C.c_float, c_f32p, c_f32p, c_f32p, c_f32p],
    ),
    "khg_scaled_trans_cost": (C.c_int, [C.c_int32, c_f32p, c_f32p, c_i32p, c_u8p, C.c_float, C.c_float, c_f32p]),
    "khg_fmllr_stats_create": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "khg_fmllr_stats_destroy": (C.c_int, [vp]),
    "khg_fmllr_stats_zero": (C.c_int, [vp, vp]),
    "khg_fmllr_stats_download": (C.c_int, [vp, vp, c_f64p, c_f64p, c_f64p]),
    "khg_fmllr_stats_upload": (C.c_int, [vp, vp, c_f64p, c_f64p, c_f64p]),
    "khg_fmllr_stats_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_fmllr_stats_set_chunk_frames": (C.c_int, [vp, C.c_int64]),
    "khg_fmllr_stats_num_chunks": (C.c_int, [vp, c_i32p]),
    "khg_acc_fmllr_stats_post": (C.c_int, [vp, vp, vp, vp, vp, C.c_float, c_i32p, vp]),
    "khg_fmllr_options_default": (None, [C.POINTER(FmllrOptionsC)]),
    "khg_fmllr_compute": (C.c_int, [C.POINTER(FmllrOptionsC), C.c_int32, C.c_int32, c_f64p, c_f64p, c_f64p, c_f32p, c_f64p, c_f64p, c_f64p,
                                    c_i32p]),
    "khg_fmllr_stats_estimate": (C.c_int, [vp, vp, C.POINTER(FmllrOptionsC), c_f32p, vp, c_f64p, c_f64p, c_i32p]),
    "khg_posteriors_from_ali": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "khg_utts_transform_feats": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_f32p, vp, vp]),
    "khg_mllt_stats_create": (C.c_int, [vp, C.c_int32, C.POINTER(vp)]),
    "khg_mllt_stats_destroy": (C.c_int, [vp]),
    "khg_mllt_stats_zero": (C.c_int, [vp, vp]),
    "khg_mllt_stats_download": (C.c_int, [vp, vp, c_f64p, c_f64p]),
    "khg_mllt_stats_upload": (C.c_int, [vp, vp, c_f64p, c_f64p]),
    "khg_mllt_stats_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_mllt_stats_set_chunk_frames": (C.c_int, [vp, C.c_int64]),
    "khg_mllt_stats_num_chunks": (C.c_int, [vp, c_i32p]),
    "khg_acc_mllt_stats_post": (C.c_int, [vp, vp, vp, vp, vp, C.c_float, vp]),
    "khg_mllt_options_default": (None, [C.POINTER(MlltOptionsC)]),
    "khg_mllt_compute": (C.c_int, [C.POINTER(MlltOptionsC), C.c_int32, C.c_double, c_f64p, c_f32p, c_f64p, c_f64p, c_f64p, c_i32p]),
    "khg_model_transform_means": (C.c_int, [vp, vp, c_f32p]),
    "khg_lda_stats_create": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "khg_lda_stats_destroy": (C.c_int, [vp]),
    "khg_lda_stats_zero": (C.c_int, [vp, vp]),
    "khg_lda_stats_download": (C.c_int, [vp, vp, c_f64p, c_f64p, c_f64p]),
    "khg_lda_stats_upload": (C.c_int, [vp, vp, c_f64p, c_f64p, c_f64p]),
    "khg_lda_stats_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_lda_stats_set_chunk_frames": (C.c_int, [vp, C.c_int64]),
    "khg_lda_stats_num_chunks": (C.c_int, [vp, c_i32p]),
    "khg_acc_lda_stats_post": (C.c_int, [vp, vp, vp, vp, C.c_float, vp]),
    "khg_lda_options_default": (None, [C.POINTER(LdaOptionsC)]),
    "khg_lda_compute": (C.c_int, [C.POINTER(LdaOptionsC), C.c_int32, C.c_int32, c_f64p, c_f64p, c_f64p, c_f32p, c_f64p, c_f64p, c_f64p, c_f64p,
                                  c_i32p]),
    "khg_utts_splice_transform_feats": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f32p, vp]),
    "khg_tree_stats_create": (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "khg_tree_stats_destroy": (C.c_int, [vp]),
    "khg_tree_stats_zero": (C.c_int, [vp, vp]),
    "khg_tree_stats_num_keys": (C.c_int, [vp, vp, C.POINTER(C.c_int64)]),
    "khg_tree_stats_download": (C.c_int, [vp, vp, c_i32p, c_f64p, c_f64p, c_f64p]),
    "khg_tree_stats_upload": (C.c_int, [vp, vp, C.c_int64, c_i32p, c_f64p, c_f64p, c_f64p]),
    "khg_tree_stats_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_acc_tree_stats": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_i32p, c_i32p, C.c_int32, c_i32p, vp, c_i32p]),
    "khg_build_tree": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, c_i32p, c_f64p, c_f64p, c_f64p, C.c_int32, c_i32p, c_i64p, c_i64p, c_i32p, C.c_int32,
                                 c_i64p, c_i32p, c_i32p, c_i32p, C.c_int32, c_i32p, C.c_double, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_ubyte), C.c_int64,
                                 C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), c_i32p, c_i32p]),
    "khg_cmvn_stats_create": (C.c_int, [vp, C.c_int32, C.c_int32, C.POINTER(vp)]),
    "khg_cmvn_stats_destroy": (C.c_int, [vp]),
    "khg_cmvn_stats_zero": (C.c_int, [vp, vp]),
    "khg_cmvn_stats_download": (C.c_int, [vp, vp, c_f64p]),
    "khg_cmvn_stats_upload": (C.c_int, [vp, vp, c_f64p]),
    "khg_cmvn_stats_add": (C.c_int, [vp, vp, C.c_float, vp]),
    "khg_cmvn_stats_set_chunk_frames": (C.c_int, [vp, C.c_int64]),
    "khg_cmvn_stats_num_chunks": (C.c_int, [vp, c_i32p]),
    "khg_acc_cmvn_stats": (C.c_int, [vp, vp, c_i32p, vp]),
    "khg_cmvn_compute": (C.c_int, [C.c_int32, C.c_int32, c_f64p, C.c_int32, C.c_int32, C.c_int32, c_f32p, c_i32p]),
    "khg_delta_scales": (C.c_int, [C.c_int32, C.c_int32, c_f32p]),
    "khg_utts_apply_cmvn": (C.c_int, [vp, vp, C.c_int32, c_i32p, c_f32p, c_i32p, vp]),
    "khg_utts_add_deltas": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32, c_i32p, c_f32p, c_i32p, vp]),
    "khg_frontend_opts_default": (None, [C.POINTER(FrontendOptsC)]),
    "khg_frontend_dims": (C.c_int, [C.POINTER(FrontendOptsC), c_i32p]),
    "khg_frontend_num_frames": (C.c_int, [C.POINTER(FrontendOptsC), C.c_int64, c_i64p]),
    "khg_frontend_tables": (C.c_int, [C.POINTER(FrontendOptsC), c_f32p, c_i32p, c_i32p, c_f32p, c_f32p, c_f32p, c_f32p]),
    "khg_frontend_create": (C.c_int, [vp, C.POINTER(FrontendOptsC), C.POINTER(vp)]),
    "khg_frontend_destroy": (C.c_int, [vp]),
    "khg_frontend_compute": (C.c_int, [vp, vp, C.c_int32, c_i64p, vp, vp, C.c_int32, c_i64p, vp]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here == header/library mismatch
    _fn.restype = _res
    _fn.argtypes = _args


def check(rc):
    if rc != 0:
        raise KhgError(lib.khg_last_error().decode("utf-8", "replace"))


def ptr(a, ctype):
    """numpy array -> typed pointer (None passes NULL); the caller keeps `a` alive."""
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


def as_np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)
