"""Alignment API -- the C++ of csrc/khg_host_align.{hpp,cpp} and csrc/khg_host_fst.{hpp,cpp} (mirrors of
csrc/decoder-wrappers.{h,cc}, csrc/faster-decoder.{h,cc}, csrc/decodable-am-diag-gmm.h, csrc/decodable-itf.h,
csrc/hmm-utils.cc:465-493) under their pybind names (python/csrc/decoder-wrappers.cc, faster-decoder.cc,
decodable-am-diag-gmm.cc, decodable-itf.cc, hmm-utils.cc): AlignConfig, FasterDecoderOptions, DecodableInterface,
DecodableAmDiagGmmUnmapped / Scaled, add_transition_probs, align_utterance_wrapper, the batched align_batch, and FasterDecoder with
its linear best-path lattice; LatticeFasterDecoder + decode_utterance_lattice_faster (csrc/lattice-faster-decoder.{h,cc},
decoder-wrappers.cc:186-224) and the batched decode_lattice_faster_batch; LatticeSimpleDecoder + decode_utterance_lattice_simple
(csrc/lattice-simple-decoder.{h,cc}, decoder-wrappers.cc:142-182), the batched decode_lattice_simple_batch and DecodableCtc
(csrc/decodable-ctc.{h,cc}).  The work is done by K1 (log-likes) + K2 (Viterbi / the
lattice decoder) through the C-ABI.  This module re-exports them."""
from . import device  # noqa: F401
from ._kaldi_hmm_gmm_amd import (AlignConfig, DecodableAmDiagGmmScaled, DecodableAmDiagGmmUnmapped, DecodableInterface,  # noqa: F401
                                 FasterDecoder, FasterDecoderOptions, LatticeArc, LatticeWeight, LinearLattice,
                                 add_transition_probs, align_batch, align_utterance_wrapper)
from ._kaldi_hmm_gmm_amd import (DeterminizeLatticePhonePrunedOptions, LatticeFasterDecoder, LatticeFasterDecoderConfig,  # noqa: F401
                                 LatticeFasterDecoderStdVectorFst, decode_lattice_faster_batch, decode_utterance_lattice_faster)
from ._kaldi_hmm_gmm_amd import (DecodableCtc, LatticeSimpleDecoder, LatticeSimpleDecoderConfig, decode_lattice_simple_batch,  # noqa: F401
                                 decode_utterance_lattice_simple)
from ._kaldi_hmm_gmm_amd import Lattice, get_raw_lattice_simple_batch  # noqa: F401
from ._kaldi_hmm_gmm_amd import DeviceLattices, get_raw_lattice_simple_device_batch  # noqa: F401
from ._kaldi_hmm_gmm_amd import DevicePosteriors  # noqa: F401
from ._kaldi_hmm_gmm_amd import DeviceLm  # noqa: F401
from ._kaldi_hmm_gmm_amd import get_raw_lattice_faster_batch, get_raw_lattice_faster_device_batch  # noqa: F401
from .device import ALIGN_ERROR, ALIGN_RETRIED, INT32_MAX  # noqa: F401
