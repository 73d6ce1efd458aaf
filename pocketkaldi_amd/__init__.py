"""pocketkaldi_amd -- MI355X-native acoustic scoring behind pocketkaldi's own interfaces.

The product is the C-ABI shared library ``libpk_mi355.so`` (HIP kernels for gfx950 +
the reference-compatible ``pk_decodable_*`` functions; see ``include/pk_mi355.h``).
This package is the thin Python host side over that ABI used by the tests and the
benchmark; it mirrors the reference's class names and argument meaning:

    Fbank().compute(wave)                    fbank.h:47-53   Fbank::Compute
    CMVN(global_stats, raw).get_frames()     cmvn.h:17-26    CMVN::GetFrame, all frames
    AcousticModel(layers, prior, ...)        am.h:23-52      AcousticModel
    AcousticModel.propagate(x)               nnet.h:96       Nnet::Propagate
    Decodable(am, prob_scale, feats)         decodable.h:22-41
    BatchScorer(am, global_stats, ...)       pocketkaldi.cc:176-218 stages, batched
    OnlineScorer(am, global_stats, ...)      the same stages on live PCM chunks, frame by frame as frames become final
    Fst(path)                                fst.h           Fst::Read, CountArcs
    Decoder(fst, am, max_utts)               decoder.h       Decoder::Decode + BestPath, batched on the GPU
    OnlineDecoder(fst, am, max_streams)      the same search frame by frame across calls, partial hypotheses
    SymbolTable(path)                        symbol_table.h  pk_symboltable_read / _get
    Recognizer(config, ...).process(waves)   pocketkaldi.cc:72-248  pk_load + pk_process: waves to text

There is no CPU fallback: if the library is missing or no gfx950 device is usable,
every compute call raises ``PkError``.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import build as _build

__all__ = ["PkError", "lib", "lib_path", "read_wav", "read_wave", "resample", "resample_table", "resample_num_output", "ResampleTable", "process_acoustic", "Fbank", "CMVN", "AcousticModel", "Decodable",
           "BatchScorer", "OnlineScorer", "Fst", "Decoder", "OnlineDecoder", "SymbolTable", "Recognizer", "OnlineRecognizer", "Result", "Segment", "NormSpec", "OnlineCmvnSpec", "parse_norm", "cmvn_normalize", "cmvn_online", "kaldi_cmvn_stats", "DeltaSpec", "parse_deltas", "delta_scales", "add_deltas", "TransformSpec", "parse_transform", "transform_feats", "splice_feats", "num_frames", "LINEAR", "RELU", "NORMALIZE", "SOFTMAX", "ADD", "MUL", "SIGMOID", "TANH", "PNORM", "TIME_SPLICE", "ONLINE_TIME_SPLICE_REFUSAL", "apply_layer", "time_splice", "write_nnet", "KINDS"]

LINEAR, RELU, NORMALIZE, SOFTMAX = 0, 1, 2, 3
TIME_SPLICE = 9                                      # a splice between hidden layers
# what every online create says of a model with time-splice layers (csrc/capi_batch.hip: CheckCreate; recognize.py turns it
# into a usage error; tests/test_gpu_time_splice.py holds the two texts together)
ONLINE_TIME_SPLICE_REFUSAL = "time-splice layers are not supported by the online scorers yet"
ADD, MUL, SIGMOID, TANH, PNORM = 4, 5, 6, 7, 8      # 4 and 5: the reference's numbers (nnet.h:18-19); 6 to 8: ours
KINDS = ("fbank", "cmvn", "gemm", "tail", "other")

_HERE = os.path.dirname(os.path.abspath(__file__))


class PkError(RuntimeError):
    pass


class pk_matrix_t(C.Structure):          # matrix.h:20-24
    _fields_ = [("ncol", C.c_int), ("nrow", C.c_int), ("data", C.POINTER(C.c_float))]


class pk_vector_t(C.Structure):          # vector.h:39-42
    _fields_ = [("dim", C.c_int), ("data", C.POINTER(C.c_float))]


class pk_decodable_t(C.Structure):       # decodable.h:15-18
    _fields_ = [("log_prob", pk_matrix_t), ("am", C.c_void_p)]


class pk_mi355_word_t(C.Structure):      # one word segment of a best path (include/pk_mi355.h)
    _fields_ = [("word", C.c_int32), ("start_frame", C.c_int32), ("num_frames", C.c_int32), ("graph_cost", C.c_float),
                ("acoustic_cost", C.c_float)]


class pk_mi355_endpoint_rule_t(C.Structure):     # one endpoint rule, in frames (include/pk_mi355.h)
    _fields_ = [("must_contain_nonsilence", C.c_int), ("min_trailing_silence_frames", C.c_int),
                ("max_relative_cost", C.c_float), ("min_utterance_frames", C.c_int)]


class pk_mi355_utterance_t(C.Structure):         # one utterance of an endpointed stream (include/pk_mi355.h)
    _fields_ = [("first_frame", C.c_int), ("num_frames", C.c_int), ("rule", C.c_int), ("ok", C.c_int), ("num_words", C.c_int),
                ("num_word_segments", C.c_int), ("weight", C.c_float), ("loglikelihood_per_frame", C.c_float)]


class pk_mi355_endpoint_t(C.Structure):          # a slot's endpoint record (include/pk_mi355.h)
    _fields_ = [("valid", C.c_int), ("frames", C.c_int), ("trailing_silence_frames", C.c_int), ("num_final", C.c_int),
                ("rule", C.c_int), ("best_cost", C.c_float), ("final_cost", C.c_float), ("relative_cost", C.c_float)]


_lib = None

# every symbol include/pk_mi355.h declares (tests check the library exports all of them)
class pk_mi355_frontend_spec_t(C.Structure):     # a front-end specification (include/pk_mi355.h)
    _fields_ = [("kind", C.c_int32), ("num_mel_bins", C.c_int32), ("num_ceps", C.c_int32), ("window", C.c_int32),
                ("low_freq", C.c_float), ("high_freq", C.c_float), ("cepstral_lifter", C.c_float)]


class pk_mi355_norm_spec_t(C.Structure):         # a normalisation specification (include/pk_mi355.h)
    _fields_ = [("mode", C.c_int32), ("norm_means", C.c_int32), ("norm_vars", C.c_int32)]


class pk_mi355_online_cmvn_spec_t(C.Structure):  # an online CMVN specification (include/pk_mi355.h)
    _fields_ = [("cmn_window", C.c_int32), ("speaker_frames", C.c_int32), ("global_frames", C.c_int32), ("norm_vars", C.c_int32)]


class pk_mi355_deltas_spec_t(C.Structure):       # a delta-features specification (include/pk_mi355.h)
    _fields_ = [("order", C.c_int32), ("window", C.c_int32)]


class pk_mi355_transform_spec_t(C.Structure):    # a feature-transform specification (include/pk_mi355.h)
    _fields_ = [("left_context", C.c_int32), ("right_context", C.c_int32), ("in_dim", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("matrix", C.POINTER(C.c_float))]


EXPORTS = [
    "pk_mi355_last_error", "pk_mi355_set_device", "pk_decodable_init", "pk_decodable_destroy",
    "pk_decodable_loglikelihood", "pk_decodable_islastframe", "pk_mi355_am_create",
    "pk_mi355_am_destroy", "pk_mi355_am_add_linear", "pk_mi355_am_add_layer",
    "pk_mi355_am_finalize", "pk_mi355_am_set_precision", "pk_mi355_am_precision", "pk_mi355_am_set_softmax", "pk_mi355_am_softmax", "pk_mi355_am_read", "pk_mi355_load", "pk_mi355_am_num_pdfs", "pk_mi355_am_input_dim", "pk_mi355_am_feat_dim",
    "pk_mi355_am_transition_to_pdf", "pk_mi355_am_blob_device_ptr", "pk_mi355_am_blob_bytes",
    "pk_mi355_nnet_propagate", "pk_mi355_num_frames", "pk_mi355_fbank_compute",
    "pk_mi355_cmvn_apply", "pk_mi355_batch_create", "pk_mi355_batch_destroy",
    "pk_mi355_batch_set_waves", "pk_mi355_batch_set_waves_i16", "pk_mi355_batch_set_waves_device",
    "pk_mi355_batch_score", "pk_mi355_batch_synchronize", "pk_mi355_batch_num_utts",
    "pk_mi355_batch_num_frames", "pk_mi355_batch_total_frames", "pk_mi355_batch_loglik_device",
    "pk_mi355_batch_fetch", "pk_mi355_batch_fetch_all", "pk_mi355_batch_fetch_fbank", "pk_mi355_batch_fetch_cmvn", "pk_mi355_test_logf",
    "pk_mi355_test_srfft512", "pk_mi355_am_broadcast", "pk_mi355_am_broadcast_from",
    "pk_mi355_batch_gather_loglik", "pk_mi355_device_malloc", "pk_mi355_device_free", "pk_mi355_memcpy",
    "pk_mi355_host_malloc", "pk_mi355_host_free",
    "pk_mi355_batch_stream", "pk_mi355_batch_enable_timing", "pk_mi355_batch_get_timing",
    "pk_mi355_am_flops_per_frame", "pk_mi355_16kpcm_read", "pk_mi355_process_acoustic",
    "pk_mi355_device_count", "pk_mi355_version",
    "pk_mi355_am_get_exponents", "pk_mi355_am_set_input_exponents", "pk_mi355_am_calibrate", "pk_mi355_batch_calibrate",
    "pk_mi355_fst_read", "pk_mi355_fst_destroy", "pk_mi355_fst_num_states", "pk_mi355_fst_num_arcs", "pk_mi355_fst_start",
    "pk_mi355_fst_arc_range", "pk_mi355_decoder_create", "pk_mi355_decoder_destroy", "pk_mi355_decoder_set_beam",
    "pk_mi355_decoder_decode_batch", "pk_mi355_decoder_decode", "pk_mi355_decoder_synchronize", "pk_mi355_decoder_result",
    "pk_mi355_decoder_best_path_arcs", "pk_mi355_decoder_active_bound", "pk_mi355_last_error_code",
    "pk_mi355_decoder_set_trace_gc", "pk_mi355_decoder_trace_stats",
    "pk_mi355_stream_create", "pk_mi355_stream_destroy", "pk_mi355_stream_open", "pk_mi355_stream_push",
    "pk_mi355_stream_push_i16", "pk_mi355_stream_close", "pk_mi355_stream_step", "pk_mi355_stream_synchronize",
    "pk_mi355_stream_loglik_device", "pk_mi355_stream_fetch",
    "pk_mi355_online_decoder_create", "pk_mi355_online_decoder_destroy", "pk_mi355_online_decoder_set_beam",
    "pk_mi355_online_decoder_open", "pk_mi355_online_decoder_advance", "pk_mi355_online_decoder_advance_host",
    "pk_mi355_online_decoder_synchronize", "pk_mi355_online_decoder_partial", "pk_mi355_online_decoder_result",
    "pk_mi355_online_decoder_best_path_arcs", "pk_mi355_online_decoder_active_bound",
    "pk_mi355_decoder_set_alignment", "pk_mi355_decoder_alignment", "pk_mi355_decoder_word_segments",
    "pk_mi355_online_decoder_word_segments",
    "pk_mi355_symtab_read", "pk_mi355_symtab_destroy", "pk_mi355_symtab_size", "pk_mi355_symtab_get",
    "pk_mi355_recognizer_load", "pk_mi355_recognizer_destroy", "pk_mi355_recognizer_am", "pk_mi355_recognizer_batch",
    "pk_mi355_recognizer_decoder", "pk_mi355_recognizer_symtab", "pk_mi355_recognizer_process", "pk_mi355_recognizer_hyp",
    "pk_mi355_recognizer_loglikelihood_per_frame",
    "pk_mi355_online_decoder_set_alignment", "pk_mi355_online_decoder_alignment", "pk_mi355_online_decoder_num_frames",
    "pk_mi355_online_recognizer_load", "pk_mi355_online_recognizer_destroy", "pk_mi355_online_recognizer_am",
    "pk_mi355_online_recognizer_stream", "pk_mi355_online_recognizer_decoder", "pk_mi355_online_recognizer_symtab",
    "pk_mi355_online_recognizer_open", "pk_mi355_online_recognizer_push", "pk_mi355_online_recognizer_push_i16",
    "pk_mi355_online_recognizer_close", "pk_mi355_online_recognizer_step", "pk_mi355_online_recognizer_partial",
    "pk_mi355_online_recognizer_finished", "pk_mi355_online_recognizer_hyp",
    "pk_mi355_online_recognizer_loglikelihood_per_frame",
    "pk_mi355_online_decoder_set_commit", "pk_mi355_online_decoder_committed", "pk_mi355_online_decoder_trace_stats",
    "pk_mi355_online_recognizer_stable",
    "pk_mi355_resample_plan", "pk_mi355_resample_table", "pk_mi355_resample_num_output", "pk_mi355_resample",
    "pk_mi355_resample_set_waves", "pk_mi355_wave_read", "pk_mi355_recognizer_process_rates",
    "pk_mi355_stream_open_rate", "pk_mi355_stream_rate", "pk_mi355_online_recognizer_open_rate",
    "pk_mi355_endpoint_default_rules", "pk_mi355_endpoint_eval", "pk_mi355_online_decoder_set_endpointing",
    "pk_mi355_online_decoder_endpoint", "pk_mi355_online_decoder_finish",
    "pk_mi355_online_recognizer_set_endpointing", "pk_mi355_online_recognizer_num_utterances",
    "pk_mi355_online_recognizer_utterance", "pk_mi355_online_recognizer_utterance_hyp",
    "pk_mi355_online_recognizer_utterance_words", "pk_mi355_online_recognizer_utterance_word_segments",
    "pk_mi355_ark_open", "pk_mi355_ark_next", "pk_mi355_ark_key", "pk_mi355_ark_matrix", "pk_mi355_ark_close", "pk_mi355_ark_read_object",
    "pk_mi355_features_batch_create", "pk_mi355_features_batch_create_stats", "pk_mi355_features_stream_create_stats", "pk_mi355_features_set", "pk_mi355_features_set_device",
    "pk_mi355_features_dim", "pk_mi355_recognizer_process_features",
    "pk_mi355_features_stream_create", "pk_mi355_stream_open_features", "pk_mi355_stream_push_features",
    "pk_mi355_stream_feat_dim", "pk_mi355_stream_slot_kind",
    "pk_mi355_online_recognizer_open_features", "pk_mi355_online_recognizer_push_features",
    "pk_mi355_frontend_check", "pk_mi355_frontend_dim", "pk_mi355_frontend_default", "pk_mi355_frontend_tables",
    "pk_mi355_frontend_compute", "pk_mi355_frontend_batch_create",
    "pk_mi355_frontend_stream_create", "pk_mi355_load_stats", "pk_mi355_frontend_recognizer_load", "pk_mi355_frontend_online_recognizer_load",
    "pk_mi355_norm_check", "pk_mi355_norm_apply", "pk_mi355_norm_set", "pk_mi355_norm_set_speaker_stats", "pk_mi355_norm_fetch_stats",
    "pk_mi355_ark_matrix_f64",
    "pk_mi355_online_cmvn_check", "pk_mi355_online_cmvn_apply", "pk_mi355_norm_set_online_cmvn",
    "pk_mi355_stream_norm_set", "pk_mi355_stream_norm_set_online_cmvn", "pk_mi355_stream_norm_set_speaker_stats",
    "pk_mi355_stream_norm_fetch_stats",
    "pk_mi355_deltas_check", "pk_mi355_deltas_dim", "pk_mi355_deltas_scales", "pk_mi355_deltas_apply",
    "pk_mi355_deltas_batch_create", "pk_mi355_deltas_base_dim", "pk_mi355_deltas_recognizer_load",
    "pk_mi355_deltas_stream_create", "pk_mi355_stream_base_dim", "pk_mi355_deltas_online_recognizer_load",
    "pk_mi355_transform_check", "pk_mi355_transform_out_dim", "pk_mi355_transform_apply", "pk_mi355_transform_batch_create",
    "pk_mi355_transform_in_dim", "pk_mi355_transform_set_utt", "pk_mi355_transform_recognizer_load",
    "pk_mi355_transform_stream_create", "pk_mi355_stream_in_dim", "pk_mi355_stream_transform_set_slot",
    "pk_mi355_transform_online_recognizer_load",
    "pk_mi355_am_add_vector_layer", "pk_mi355_am_add_pnorm", "pk_mi355_layer_apply_host",
    "pk_mi355_am_add_time_splice", "pk_mi355_am_time_context", "pk_mi355_time_splice_host",
]


def lib_path():
    """The product library: always the in-tree build."""
    return os.path.join(_HERE, "libpk_mi355.so")


def lib():
    """Load libpk_mi355.so, (re)building it in-tree first whenever the sources it was built from
    differ from the sources in the tree (content hash, build.py).  A stale library is never
    loaded silently: where no compiler exists the load fails instead."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if _build._stale():
        if not _build.have_compiler():
            raise PkError("libpk_mi355.so is %s and there is no hipcc here to build it"
                          % ("stale (sources changed since it was built)" if os.path.exists(path) else "missing"))
        try:
            _build.build()
        except Exception as e:
            raise PkError("libpk_mi355.so cannot be built: %s" % e)
    L = C.CDLL(path)
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.pk_mi355_last_error.restype = C.c_char_p
    L.pk_mi355_version.restype = C.c_char_p
    L.pk_mi355_set_device.argtypes = [C.c_int]
    L.pk_decodable_init.restype = None
    L.pk_decodable_init.argtypes = [C.POINTER(pk_decodable_t), C.c_void_p, C.c_float,
                                    C.POINTER(pk_matrix_t)]
    L.pk_decodable_destroy.restype = None
    L.pk_decodable_destroy.argtypes = [C.POINTER(pk_decodable_t)]
    L.pk_decodable_loglikelihood.restype = C.c_float
    L.pk_decodable_loglikelihood.argtypes = [C.POINTER(pk_decodable_t), C.c_int, C.c_int]
    L.pk_decodable_islastframe.restype = C.c_bool
    L.pk_decodable_islastframe.argtypes = [C.POINTER(pk_decodable_t), C.c_int]
    L.pk_mi355_am_create.restype = C.c_void_p
    L.pk_mi355_am_destroy.restype = None
    L.pk_mi355_am_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_am_add_linear.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p]
    L.pk_mi355_am_add_layer.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_am_add_vector_layer.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p]
    L.pk_mi355_am_add_pnorm.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pk_mi355_layer_apply_host.argtypes = [C.c_int, f32p, C.c_int, C.c_int, f32p, C.c_int, f32p]
    L.pk_mi355_am_add_time_splice.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int]
    L.pk_mi355_am_time_context.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_time_splice_host.argtypes = [f32p, C.c_int, C.c_int, i32p, C.c_int, f32p]
    L.pk_mi355_am_set_precision.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_am_precision.argtypes = [C.c_void_p]
    L.pk_mi355_am_finalize.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int, i32p, C.c_int]
    L.pk_mi355_am_read.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int,
                                   C.c_int]
    L.pk_mi355_am_set_softmax.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_am_softmax.argtypes = [C.c_void_p]
    L.pk_mi355_load.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), f32p]
    L.pk_mi355_am_num_pdfs.argtypes = [C.c_void_p]
    L.pk_mi355_am_input_dim.argtypes = [C.c_void_p]
    L.pk_mi355_am_transition_to_pdf.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_am_blob_device_ptr.restype = C.c_void_p
    L.pk_mi355_am_blob_device_ptr.argtypes = [C.c_void_p]
    L.pk_mi355_am_blob_bytes.restype = C.c_size_t
    L.pk_mi355_am_blob_bytes.argtypes = [C.c_void_p]
    L.pk_mi355_am_flops_per_frame.restype = C.c_double
    L.pk_mi355_am_flops_per_frame.argtypes = [C.c_void_p]
    L.pk_mi355_nnet_propagate.argtypes = [C.c_void_p, C.POINTER(pk_matrix_t), C.POINTER(pk_matrix_t)]
    L.pk_mi355_num_frames.argtypes = [C.c_int]
    L.pk_mi355_fbank_compute.argtypes = [C.POINTER(pk_vector_t), C.POINTER(pk_matrix_t)]
    L.pk_mi355_cmvn_apply.argtypes = [C.POINTER(pk_vector_t), C.POINTER(pk_matrix_t),
                                      C.POINTER(pk_matrix_t)]
    L.pk_mi355_batch_create.restype = C.c_void_p
    L.pk_mi355_batch_create.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64]
    L.pk_mi355_batch_destroy.restype = None
    L.pk_mi355_batch_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_batch_set_waves.argtypes = [C.c_void_p, C.POINTER(pk_vector_t), C.c_int]
    L.pk_mi355_batch_set_waves_i16.argtypes = [C.c_void_p, C.POINTER(C.c_int16), C.POINTER(C.c_int),
                                               C.c_int]
    L.pk_mi355_batch_set_waves_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.pk_mi355_batch_score.argtypes = [C.c_void_p, C.c_float, C.c_int]
    L.pk_mi355_batch_synchronize.argtypes = [C.c_void_p]
    L.pk_mi355_batch_num_utts.argtypes = [C.c_void_p]
    L.pk_mi355_batch_num_frames.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_batch_total_frames.restype = C.c_int64
    L.pk_mi355_batch_total_frames.argtypes = [C.c_void_p]
    L.pk_mi355_batch_loglik_device.restype = C.c_void_p
    L.pk_mi355_batch_loglik_device.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_batch_fetch.argtypes = [C.c_void_p, C.c_int, C.POINTER(pk_decodable_t)]
    L.pk_mi355_batch_fetch_all.argtypes = [C.c_void_p, C.POINTER(pk_decodable_t), C.c_int, C.c_int]
    L.pk_mi355_batch_fetch_fbank.argtypes = [C.c_void_p, C.c_int, f32p]
    L.pk_mi355_batch_fetch_cmvn.argtypes = [C.c_void_p, C.c_int, f32p]
    L.pk_mi355_test_logf.argtypes = [f32p, C.c_int, f32p]
    L.pk_mi355_test_srfft512.argtypes = [f32p, C.c_int, f32p]
    L.pk_mi355_am_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.pk_mi355_am_broadcast_from.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.pk_mi355_batch_gather_loglik.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.pk_mi355_device_malloc.restype = C.c_void_p
    L.pk_mi355_device_malloc.argtypes = [C.c_size_t]
    L.pk_mi355_device_free.restype = None
    L.pk_mi355_device_free.argtypes = [C.c_void_p]
    L.pk_mi355_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.pk_mi355_host_malloc.restype = C.c_void_p
    L.pk_mi355_host_malloc.argtypes = [C.c_size_t]
    L.pk_mi355_host_free.restype = None
    L.pk_mi355_host_free.argtypes = [C.c_void_p]
    L.pk_mi355_batch_stream.restype = C.c_void_p
    L.pk_mi355_batch_stream.argtypes = [C.c_void_p]
    L.pk_mi355_batch_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_batch_get_timing.argtypes = [C.c_void_p, f32p, C.POINTER(C.c_int)]
    L.pk_mi355_16kpcm_read.argtypes = [C.c_char_p, C.POINTER(pk_vector_t)]
    L.pk_mi355_process_acoustic.argtypes = [C.c_void_p, C.POINTER(pk_vector_t), C.POINTER(pk_vector_t), C.c_float,
                                            C.POINTER(pk_decodable_t), C.c_int]
    L.pk_mi355_am_get_exponents.argtypes = [C.c_void_p, i32p, i32p, C.c_int]
    L.pk_mi355_am_set_input_exponents.argtypes = [C.c_void_p, i32p, C.c_int]
    L.pk_mi355_am_calibrate.argtypes = [C.c_void_p, C.POINTER(pk_matrix_t)]
    L.pk_mi355_batch_calibrate.argtypes = [C.c_void_p]
    L.pk_mi355_last_error_code.argtypes = []
    L.pk_mi355_fst_read.restype = C.c_void_p
    L.pk_mi355_fst_read.argtypes = [C.c_char_p]
    L.pk_mi355_fst_destroy.restype = None
    L.pk_mi355_fst_destroy.argtypes = [C.c_void_p]
    for f in ("num_states", "num_arcs", "start"):
        getattr(L, "pk_mi355_fst_" + f).argtypes = [C.c_void_p]
    L.pk_mi355_fst_arc_range.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_decoder_create.restype = C.c_void_p
    L.pk_mi355_decoder_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64]
    L.pk_mi355_decoder_destroy.restype = None
    L.pk_mi355_decoder_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_decoder_set_beam.argtypes = [C.c_void_p, C.c_float, C.c_int]
    L.pk_mi355_decoder_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.pk_mi355_decoder_decode.argtypes = [C.c_void_p, C.POINTER(pk_decodable_t), C.c_int, C.c_int]
    L.pk_mi355_decoder_synchronize.argtypes = [C.c_void_p]
    L.pk_mi355_decoder_result.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int, f32p, C.POINTER(C.c_int)]
    L.pk_mi355_decoder_best_path_arcs.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int]
    L.pk_mi355_decoder_active_bound.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_decoder_set_trace_gc.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_decoder_trace_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int)]
    L.pk_mi355_stream_create.restype = C.c_void_p
    L.pk_mi355_stream_create.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64]
    L.pk_mi355_stream_destroy.restype = None
    L.pk_mi355_stream_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_stream_open.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_stream_push.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int]
    L.pk_mi355_stream_push_i16.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int16), C.c_int]
    L.pk_mi355_stream_close.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_stream_step.argtypes = [C.c_void_p, C.c_float, C.c_int]
    L.pk_mi355_stream_synchronize.argtypes = [C.c_void_p]
    L.pk_mi355_stream_loglik_device.restype = C.c_void_p
    L.pk_mi355_stream_loglik_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_stream_fetch.argtypes = [C.c_void_p, C.c_int, C.POINTER(pk_decodable_t), C.POINTER(C.c_int)]
    L.pk_mi355_online_decoder_create.restype = C.c_void_p
    L.pk_mi355_online_decoder_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64]
    L.pk_mi355_online_decoder_destroy.restype = None
    L.pk_mi355_online_decoder_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_online_decoder_set_beam.argtypes = [C.c_void_p, C.c_float, C.c_int]
    L.pk_mi355_online_decoder_open.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_advance.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_advance_host.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(pk_decodable_t),
                                                       C.POINTER(C.c_int), C.c_int, C.c_int]
    L.pk_mi355_online_decoder_synchronize.argtypes = [C.c_void_p]
    L.pk_mi355_online_decoder_partial.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int, f32p]
    L.pk_mi355_online_decoder_result.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int, f32p, C.POINTER(C.c_int)]
    L.pk_mi355_online_decoder_best_path_arcs.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int]
    L.pk_mi355_online_decoder_active_bound.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_decoder_set_alignment.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_decoder_alignment.argtypes = [C.c_void_p, C.c_int, i32p, i32p, f32p, C.c_int]
    L.pk_mi355_decoder_word_segments.argtypes = [C.c_void_p, C.c_int, C.POINTER(pk_mi355_word_t), C.c_int]
    L.pk_mi355_online_decoder_word_segments.argtypes = [C.c_void_p, C.c_int, C.POINTER(pk_mi355_word_t), C.c_int]
    L.pk_mi355_symtab_read.restype = C.c_void_p
    L.pk_mi355_symtab_read.argtypes = [C.c_char_p]
    L.pk_mi355_symtab_destroy.restype = None
    L.pk_mi355_symtab_destroy.argtypes = [C.c_void_p]
    L.pk_mi355_symtab_size.argtypes = [C.c_void_p]
    L.pk_mi355_symtab_get.restype = C.c_char_p
    L.pk_mi355_symtab_get.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_recognizer_load.restype = C.c_void_p
    L.pk_mi355_recognizer_load.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int64, C.c_int64]
    L.pk_mi355_recognizer_destroy.restype = None
    L.pk_mi355_recognizer_destroy.argtypes = [C.c_void_p]
    for f in ("am", "batch", "decoder", "symtab"):
        getattr(L, "pk_mi355_recognizer_" + f).restype = C.c_void_p
        getattr(L, "pk_mi355_recognizer_" + f).argtypes = [C.c_void_p]
    L.pk_mi355_recognizer_process.argtypes = [C.c_void_p, C.POINTER(pk_vector_t), C.c_int]
    L.pk_mi355_recognizer_hyp.restype = C.c_char_p
    L.pk_mi355_recognizer_hyp.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_recognizer_loglikelihood_per_frame.restype = C.c_float
    L.pk_mi355_recognizer_loglikelihood_per_frame.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_set_alignment.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_alignment.argtypes = [C.c_void_p, C.c_int, i32p, i32p, f32p, C.c_int]
    L.pk_mi355_online_decoder_num_frames.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_load.restype = C.c_void_p
    L.pk_mi355_online_recognizer_load.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int64]
    L.pk_mi355_online_recognizer_destroy.restype = None
    L.pk_mi355_online_recognizer_destroy.argtypes = [C.c_void_p]
    for f in ("am", "stream", "decoder", "symtab"):
        getattr(L, "pk_mi355_online_recognizer_" + f).restype = C.c_void_p
        getattr(L, "pk_mi355_online_recognizer_" + f).argtypes = [C.c_void_p]
    for f in ("open", "close", "finished"):
        getattr(L, "pk_mi355_online_recognizer_" + f).argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_push.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int]
    L.pk_mi355_online_recognizer_push_i16.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int16), C.c_int]
    L.pk_mi355_online_recognizer_step.argtypes = [C.c_void_p]
    L.pk_mi355_online_recognizer_partial.restype = C.c_char_p
    L.pk_mi355_online_recognizer_partial.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_hyp.restype = C.c_char_p
    L.pk_mi355_online_recognizer_hyp.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_loglikelihood_per_frame.restype = C.c_float
    L.pk_mi355_online_recognizer_loglikelihood_per_frame.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_set_commit.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_decoder_committed.argtypes = [C.c_void_p, C.c_int, i32p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_online_decoder_trace_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                                      C.POINTER(C.c_int64)]
    L.pk_mi355_online_recognizer_stable.restype = C.c_char_p
    L.pk_mi355_online_recognizer_stable.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_resample_plan.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_resample_table.argtypes = [C.c_int, i32p, i32p, f32p]
    L.pk_mi355_resample_num_output.restype = C.c_int64
    L.pk_mi355_resample_num_output.argtypes = [C.c_int, C.c_int64]
    L.pk_mi355_resample.argtypes = [C.POINTER(pk_vector_t), C.c_int, C.POINTER(pk_vector_t)]
    L.pk_mi355_resample_set_waves.argtypes = [C.c_void_p, C.POINTER(pk_vector_t), C.POINTER(C.c_int), C.c_int]
    L.pk_mi355_wave_read.argtypes = [C.c_char_p, C.c_int, C.POINTER(pk_vector_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pk_mi355_recognizer_process_rates.argtypes = [C.c_void_p, C.POINTER(pk_vector_t), C.POINTER(C.c_int), C.c_int]
    L.pk_mi355_stream_open_rate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pk_mi355_stream_rate.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_open_rate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    rulep = C.POINTER(pk_mi355_endpoint_rule_t)
    L.pk_mi355_endpoint_default_rules.argtypes = [rulep, C.c_int]
    L.pk_mi355_endpoint_eval.argtypes = [rulep, C.c_int, C.c_int, C.c_int, C.c_float]
    L.pk_mi355_online_decoder_set_endpointing.argtypes = [C.c_void_p, i32p, C.c_int, rulep, C.c_int]
    L.pk_mi355_online_decoder_endpoint.argtypes = [C.c_void_p, C.c_int, C.POINTER(pk_mi355_endpoint_t)]
    L.pk_mi355_online_decoder_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
    L.pk_mi355_online_recognizer_set_endpointing.argtypes = [C.c_void_p, i32p, C.c_int, rulep, C.c_int]
    L.pk_mi355_online_recognizer_num_utterances.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_utterance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(pk_mi355_utterance_t)]
    L.pk_mi355_online_recognizer_utterance_hyp.restype = C.c_char_p
    L.pk_mi355_online_recognizer_utterance_hyp.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pk_mi355_online_recognizer_utterance_words.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, C.c_int]
    L.pk_mi355_online_recognizer_utterance_word_segments.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(pk_mi355_word_t),
                                                                     C.c_int]
    L.pk_mi355_features_batch_create.restype = C.c_void_p
    L.pk_mi355_features_batch_create.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64]
    L.pk_mi355_features_batch_create_stats.restype = C.c_void_p
    L.pk_mi355_features_batch_create_stats.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_features_stream_create_stats.restype = C.c_void_p
    L.pk_mi355_features_stream_create_stats.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_am_feat_dim.argtypes = [C.c_void_p]
    L.pk_mi355_ark_open.restype = C.c_void_p
    L.pk_mi355_ark_open.argtypes = [C.c_char_p]
    L.pk_mi355_ark_read_object.restype = C.c_void_p
    L.pk_mi355_ark_read_object.argtypes = [C.c_char_p]
    L.pk_mi355_ark_next.argtypes = [C.c_void_p]
    L.pk_mi355_ark_key.restype = C.c_char_p
    L.pk_mi355_ark_key.argtypes = [C.c_void_p]
    L.pk_mi355_ark_matrix.argtypes = [C.c_void_p, C.POINTER(pk_matrix_t)]
    L.pk_mi355_ark_close.restype = None
    L.pk_mi355_ark_close.argtypes = [C.c_void_p]
    L.pk_mi355_features_set.argtypes = [C.c_void_p, C.POINTER(pk_matrix_t), C.c_int, C.c_int]
    L.pk_mi355_features_set_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int]
    L.pk_mi355_features_dim.argtypes = [C.c_void_p]
    L.pk_mi355_recognizer_process_features.argtypes = [C.c_void_p, C.POINTER(pk_matrix_t), C.c_int, C.c_int]
    L.pk_mi355_features_stream_create.restype = C.c_void_p
    L.pk_mi355_features_stream_create.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int64]
    L.pk_mi355_stream_open_features.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pk_mi355_stream_push_features.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int]
    L.pk_mi355_stream_feat_dim.argtypes = [C.c_void_p]
    L.pk_mi355_stream_slot_kind.argtypes = [C.c_void_p, C.c_int]
    L.pk_mi355_online_recognizer_open_features.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pk_mi355_online_recognizer_push_features.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int]
    specp = C.POINTER(pk_mi355_frontend_spec_t)
    L.pk_mi355_frontend_check.argtypes = [specp]
    L.pk_mi355_frontend_dim.argtypes = [specp]
    L.pk_mi355_frontend_default.argtypes = [specp]
    L.pk_mi355_frontend_tables.argtypes = [specp, f32p, i32p, i32p, f32p, f32p, f32p]
    L.pk_mi355_frontend_compute.argtypes = [specp, C.POINTER(pk_vector_t), C.POINTER(pk_matrix_t)]
    L.pk_mi355_frontend_batch_create.restype = C.c_void_p
    L.pk_mi355_frontend_batch_create.argtypes = [C.c_void_p, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_frontend_stream_create.restype = C.c_void_p
    L.pk_mi355_frontend_stream_create.argtypes = [C.c_void_p, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_load_stats.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), f32p, C.c_int, C.POINTER(C.c_int)]
    L.pk_mi355_frontend_recognizer_load.restype = C.c_void_p
    L.pk_mi355_frontend_recognizer_load.argtypes = [C.c_char_p, specp, C.c_int, C.c_int, C.c_int64, C.c_int64]
    L.pk_mi355_frontend_online_recognizer_load.restype = C.c_void_p
    L.pk_mi355_frontend_online_recognizer_load.argtypes = [C.c_char_p, specp, C.c_int, C.c_int64, C.c_int64]
    normp, f64p = C.POINTER(pk_mi355_norm_spec_t), C.POINTER(C.c_double)
    L.pk_mi355_norm_check.argtypes = [normp]
    L.pk_mi355_norm_apply.argtypes = [normp, f32p, C.c_int, C.c_int, f64p, f32p, f64p]
    L.pk_mi355_norm_set.argtypes = [C.c_void_p, normp]
    L.pk_mi355_norm_set_speaker_stats.argtypes = [C.c_void_p, f64p, C.c_int]
    L.pk_mi355_norm_fetch_stats.argtypes = [C.c_void_p, C.c_int, f64p]
    onlinep = C.POINTER(pk_mi355_online_cmvn_spec_t)
    L.pk_mi355_online_cmvn_check.argtypes = [onlinep, f64p, C.c_int]
    L.pk_mi355_online_cmvn_apply.argtypes = [onlinep, f32p, C.c_int, C.c_int, f64p, f64p, f32p, f64p]
    L.pk_mi355_norm_set_online_cmvn.argtypes = [C.c_void_p, onlinep, f64p]
    L.pk_mi355_stream_norm_set.argtypes = [C.c_void_p, normp]
    L.pk_mi355_stream_norm_set_online_cmvn.argtypes = [C.c_void_p, onlinep, f64p]
    L.pk_mi355_stream_norm_set_speaker_stats.argtypes = [C.c_void_p, C.c_int, f64p]
    L.pk_mi355_stream_norm_fetch_stats.argtypes = [C.c_void_p, C.c_int, f64p]
    L.pk_mi355_ark_matrix_f64.argtypes = [C.c_void_p, f64p, C.c_int]
    deltasp = C.POINTER(pk_mi355_deltas_spec_t)
    L.pk_mi355_deltas_check.argtypes = [deltasp]
    L.pk_mi355_deltas_dim.argtypes = [deltasp, C.c_int]
    L.pk_mi355_deltas_scales.argtypes = [deltasp, f32p]
    L.pk_mi355_deltas_apply.argtypes = [deltasp, f32p, C.c_int, C.c_int, f32p]
    L.pk_mi355_deltas_batch_create.restype = C.c_void_p
    L.pk_mi355_deltas_batch_create.argtypes = [C.c_void_p, deltasp, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_deltas_base_dim.argtypes = [C.c_void_p]
    L.pk_mi355_deltas_recognizer_load.restype = C.c_void_p
    L.pk_mi355_deltas_recognizer_load.argtypes = [C.c_char_p, specp, deltasp, C.c_int, C.c_int, C.c_int64, C.c_int64]
    L.pk_mi355_deltas_stream_create.restype = C.c_void_p
    L.pk_mi355_deltas_stream_create.argtypes = [C.c_void_p, deltasp, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_stream_base_dim.argtypes = [C.c_void_p]
    L.pk_mi355_deltas_online_recognizer_load.restype = C.c_void_p
    L.pk_mi355_deltas_online_recognizer_load.argtypes = [C.c_char_p, specp, deltasp, C.c_int, C.c_int64, C.c_int64]
    xformp = C.POINTER(pk_mi355_transform_spec_t)
    L.pk_mi355_transform_check.argtypes = [xformp]
    L.pk_mi355_transform_out_dim.argtypes = [xformp]
    L.pk_mi355_transform_apply.argtypes = [xformp, f32p, C.c_int, f32p]
    L.pk_mi355_transform_batch_create.restype = C.c_void_p
    L.pk_mi355_transform_batch_create.argtypes = [C.c_void_p, xformp, deltasp, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_transform_in_dim.argtypes = [C.c_void_p]
    L.pk_mi355_transform_set_utt.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int, C.c_int]
    L.pk_mi355_transform_recognizer_load.restype = C.c_void_p
    L.pk_mi355_transform_recognizer_load.argtypes = [C.c_char_p, specp, deltasp, xformp, C.c_int, C.c_int, C.c_int64, C.c_int64]
    L.pk_mi355_transform_stream_create.restype = C.c_void_p
    L.pk_mi355_transform_stream_create.argtypes = [C.c_void_p, xformp, deltasp, specp, f32p, C.c_int, C.c_int, C.c_int64]
    L.pk_mi355_stream_in_dim.argtypes = [C.c_void_p]
    L.pk_mi355_stream_transform_set_slot.argtypes = [C.c_void_p, C.c_int, f32p, C.c_int, C.c_int]
    L.pk_mi355_transform_online_recognizer_load.restype = C.c_void_p
    L.pk_mi355_transform_online_recognizer_load.argtypes = [C.c_char_p, specp, deltasp, xformp, C.c_int, C.c_int64, C.c_int64]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise PkError(lib().pk_mi355_last_error().decode() or "pk_mi355 error %d" % rc)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _as_matrix(a):
    """[T][D] frame-major numpy array -> pk_matrix_t{ncol=T, nrow=D} (borrowed)."""
    m = pk_matrix_t()
    m.ncol, m.nrow = a.shape
    m.data = _fp(a)
    return m


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _take_matrix(m):
    """Copy a library-allocated pk_matrix_t into numpy [ncol][nrow] and free it."""
    if m.ncol == 0 or m.nrow == 0 or not m.data:
        out = np.zeros((m.ncol, m.nrow), dtype=np.float32)
    else:
        out = np.ctypeslib.as_array(m.data, shape=(m.ncol, m.nrow)).copy()
    _libc.free(m.data)
    return out


def set_device(device):
    _check(lib().pk_mi355_set_device(int(device)))


def num_frames(num_samples):
    """Fbank::CalcNumFrames (fbank.cc:35-42)."""
    return lib().pk_mi355_num_frames(int(num_samples))


def read_wav(path):
    """pk_16kpcm_read (pcm_reader.cc:45-220) -> float32 samples (unscaled)."""
    v = pk_vector_t(0, None)
    _check(lib().pk_mi355_16kpcm_read(path.encode(), C.byref(v)))
    out = np.ctypeslib.as_array(v.data, shape=(max(v.dim, 1),))[:v.dim].copy()
    _libc.free(v.data)
    return out


def _take_vector(v):
    out = np.ctypeslib.as_array(v.data, shape=(max(v.dim, 1),))[:v.dim].copy()
    _libc.free(v.data)
    return out


def read_wave(path, channel=0):
    """pk_mi355_wave_read: any sample rate, 1 .. 8 channels -> (float32 samples of `channel`, unscaled; the rate)."""
    v, rate = pk_vector_t(0, None), C.c_int()
    _check_code(lib().pk_mi355_wave_read(os.fspath(path).encode(), int(channel), C.byref(v), C.byref(rate), None))
    return _take_vector(v), rate.value


ResampleTable = collections.namedtuple("ResampleTable", "Q P max_taps first count weights")


def resample_table(rate):
    """The polyphase table of `rate` -> 16000 (pk_mi355_resample_table; host only): Q input samples per unit, P phases,
    first[P], count[P] and weights[P][max_taps] (zero-padded).  PkCodeError (-1) names an unsupported rate."""
    q, p, taps = C.c_int(), C.c_int(), C.c_int()
    _check_code(lib().pk_mi355_resample_plan(int(rate), C.byref(q), C.byref(p), C.byref(taps)))
    first, count = np.zeros(p.value, np.int32), np.zeros(p.value, np.int32)
    weights = np.zeros((p.value, taps.value), np.float32)
    i32p = C.POINTER(C.c_int32)
    _check_code(lib().pk_mi355_resample_table(int(rate), first.ctypes.data_as(i32p), count.ctypes.data_as(i32p), _fp(weights)))
    return ResampleTable(q.value, p.value, taps.value, first, count, weights)


def resample_num_output(rate, num_samples):
    """floor(num_samples * P / Q): the 16 kHz samples `num_samples` samples at `rate` give."""
    return _check_code(lib().pk_mi355_resample_num_output(int(rate), int(num_samples)))


def resample(wave, rate):
    """One wave at `rate` Hz -> float32 samples at 16 kHz, converted on the GPU (pk_mi355_resample)."""
    w = _f32(wave).ravel()
    v, out = pk_vector_t(w.shape[0], _fp(w) if w.size else None), pk_vector_t(0, None)
    _check_code(lib().pk_mi355_resample(C.byref(v), int(rate), C.byref(out)))
    return _take_vector(out)


def _rates_array(rates, n):
    """rates (None: 16000 throughout) -> a C int array, or None where every rate is 16000."""
    if rates is None:
        return None
    rates = [int(r) for r in rates]
    if len(rates) != n:
        raise PkCodeError(-1, "%d rates for %d waves" % (len(rates), n))
    return (C.c_int * max(n, 1))(*rates)


def process_acoustic(am, global_stats, wave, prob_scale=0.1, verbose=False):
    """Stages 1-3 of pk_process (pocketkaldi.cc:186-218) fused on the device -> Decodable."""
    g, w = _f32(global_stats), _f32(wave)
    gv = pk_vector_t(g.shape[0], _fp(g))
    wv = pk_vector_t(w.shape[0], _fp(w) if w.size else None)
    d = pk_decodable_t()
    _check(lib().pk_mi355_process_acoustic(am.handle, C.byref(gv), C.byref(wv), float(prob_scale),
                                           C.byref(d), 1 if verbose else 0))
    return Decodable._from_struct(d, am)


class Fbank:
    """fbank.h:47-53.  compute(wave) -> [T][40] log-mel features."""

    def compute(self, wave):
        wave = _f32(wave)
        v = pk_vector_t(wave.shape[0], _fp(wave))
        m = pk_matrix_t(0, 0, None)
        _check(lib().pk_mi355_fbank_compute(C.byref(v), C.byref(m)))
        return _take_matrix(m)


FRONTEND_KINDS = {"fbank": 0, "mfcc": 1}             # PK_MI355_FRONTEND_*
FRONTEND_WINDOWS = {"hamming": 0, "povey": 1}        # PK_MI355_WINDOW_*


class FrontendSpec:
    """A front-end specification (pk_mi355_frontend_spec_t): log-mel fbank with num_mel_bins bins between low_freq and
    high_freq (<= 0: that much below 8000 Hz), or MFCC -- its first num_ceps cepstra, liftered (0: not) -- on top of it.
    The defaults are the reference's front-end.  kind and window also take the header's integers; nothing is checked
    here: the library refuses a bad spec (PkCodeError, the field named) wherever one is used."""

    def __init__(self, kind="fbank", num_mel_bins=40, num_ceps=None, window="hamming", low_freq=20.0, high_freq=0.0,
                 cepstral_lifter=22.0):
        self.kind = FRONTEND_KINDS.get(kind, kind)
        self.window = FRONTEND_WINDOWS.get(window, window)
        self.num_mel_bins, self.low_freq, self.high_freq = num_mel_bins, low_freq, high_freq
        self.num_ceps = num_ceps if num_ceps is not None else (13 if self.kind == 1 else 0)
        self.cepstral_lifter = cepstral_lifter

    def struct(self):
        try:
            return pk_mi355_frontend_spec_t(int(self.kind), int(self.num_mel_bins), int(self.num_ceps), int(self.window),
                                            float(self.low_freq), float(self.high_freq), float(self.cepstral_lifter))
        except (TypeError, ValueError) as e:
            raise PkCodeError(-1, "front-end spec: %s" % e)

    def check(self):
        _check_code(lib().pk_mi355_frontend_check(C.byref(self.struct())))

    @property
    def dim(self):
        """num_mel_bins for fbank, num_ceps for MFCC."""
        return _check_code(lib().pk_mi355_frontend_dim(C.byref(self.struct())))

    def __repr__(self):
        return "FrontendSpec(kind=%r, num_mel_bins=%r, num_ceps=%r, window=%r, low_freq=%r, high_freq=%r, cepstral_lifter=%r)" % (
            self.kind, self.num_mel_bins, self.num_ceps, self.window, self.low_freq, self.high_freq, self.cepstral_lifter)


def parse_frontend(text):
    """A FrontendSpec from "key=value,key=value,...": the keys are FrontendSpec's field names (kind: fbank | mfcc, window:
    hamming | povey, the others numbers), omitted keys take its defaults.  ValueError, the key named, for an unknown key
    or a value that does not parse.  Nothing else is checked here: the library refuses a bad spec where it is used."""
    fields = {"kind": FRONTEND_KINDS, "window": FRONTEND_WINDOWS, "num_mel_bins": int, "num_ceps": int, "low_freq": float,
              "high_freq": float, "cepstral_lifter": float}
    given = {}
    for item in [t.strip() for t in text.split(",") if t.strip()]:
        key, eq, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if key not in fields:
            raise ValueError("front-end spec: unknown key '%s' (the keys are %s)" % (key, ", ".join(sorted(fields))))
        if key in given:
            raise ValueError("front-end spec: key '%s' given twice" % key)
        how = fields[key]
        try:
            if not eq:
                raise ValueError
            given[key] = how[value] if isinstance(how, dict) else how(value)
            if given[key] != given[key]:                     # (nan parses as a float)
                raise ValueError
        except (KeyError, ValueError):
            raise ValueError("front-end spec: bad value '%s' for key '%s'%s" % (
                value, key, " (one of %s)" % ", ".join(sorted(how)) if isinstance(how, dict) else ""))
    return FrontendSpec(**given)


def frontend_default():
    """The reference's configuration (pk_mi355_frontend_default)."""
    st = pk_mi355_frontend_spec_t()
    _check_code(lib().pk_mi355_frontend_default(C.byref(st)))
    return FrontendSpec(st.kind, st.num_mel_bins, st.num_ceps, st.window, st.low_freq, st.high_freq, st.cepstral_lifter)


FrontendTables = collections.namedtuple("FrontendTables", "window mel_off mel_len mel_weights dct lifter")


def frontend_tables(spec):
    """The tables of a spec (pk_mi355_frontend_tables; host only): window[400], mel_off[B], mel_len[B], mel_weights (a list
    of B arrays: bin b's taps, for FFT bins mel_off[b] ...), dct[num_ceps][B] and lifter[num_ceps] (MFCC; fbank: empty)."""
    st = spec.struct()
    _check_code(lib().pk_mi355_frontend_check(C.byref(st)))
    B, K = st.num_mel_bins, st.num_ceps
    i32p = C.POINTER(C.c_int32)
    window, off, length = np.zeros(400, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    packed, dct, lifter = np.zeros(512, np.float32), np.zeros((K, B), np.float32), np.zeros(K, np.float32)
    _check_code(lib().pk_mi355_frontend_tables(C.byref(st), _fp(window), off.ctypes.data_as(i32p), length.ctypes.data_as(i32p), _fp(packed),
                                               _fp(dct) if K else None, _fp(lifter) if K else None))
    base = np.concatenate([[0], np.cumsum(length)])
    return FrontendTables(window, off, length, [packed[base[b]:base[b + 1]].copy() for b in range(B)], dct, lifter)


class Frontend:
    """The front-end at a spec for one wave: compute(wave) -> [T][spec.dim] (pk_mi355_frontend_compute)."""

    def __init__(self, spec):
        self.spec = spec

    def compute(self, wave):
        wave = _f32(wave).ravel()
        v = pk_vector_t(wave.shape[0], _fp(wave) if wave.size else None)
        m = pk_matrix_t(0, 0, None)
        _check_code(lib().pk_mi355_frontend_compute(C.byref(self.spec.struct()), C.byref(v), C.byref(m)))
        return _take_matrix(m)


NORM_MODES = {"sliding": 0, "none": 1, "utterance": 2, "speaker": 3}      # PK_MI355_NORM_*


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class NormSpec:
    """A normalisation specification (pk_mi355_norm_spec_t): mode "sliding" (cmvn.cc's rule, the default), "none",
    "utterance" or "speaker" (Kaldi's apply-cmvn on the utterance's own or on the caller's statistics), and the two
    switches.  mode also takes the header's integer; nothing is checked here: the library refuses a bad spec
    (PkCodeError, the field named) wherever one is used."""

    def __init__(self, mode="sliding", norm_means=True, norm_vars=False):
        self.mode = NORM_MODES.get(mode, mode)
        self.norm_means, self.norm_vars = norm_means, norm_vars

    def struct(self):
        try:
            return pk_mi355_norm_spec_t(int(self.mode), int(self.norm_means), int(self.norm_vars))
        except (TypeError, ValueError) as e:
            raise PkCodeError(-1, "norm spec: %s" % e)

    def check(self):
        _check_code(lib().pk_mi355_norm_check(C.byref(self.struct())))

    def __repr__(self):
        return "NormSpec(mode=%r, norm_means=%r, norm_vars=%r)" % (self.mode, self.norm_means, self.norm_vars)


class OnlineCmvnSpec:
    """An online CMVN specification (pk_mi355_online_cmvn_spec_t): Kaldi's OnlineCmvn -- a window
    of cmn_window frames, smoothed by at most speaker_frames of the speaker's statistics and then at most global_frames
    of the global ones while it is not full; means always, variance with norm_vars.  Nothing is checked here: the
    library refuses a bad spec (PkCodeError, the field named) wherever one is used."""

    def __init__(self, cmn_window=600, speaker_frames=600, global_frames=200, norm_vars=False):
        self.cmn_window, self.speaker_frames, self.global_frames, self.norm_vars = cmn_window, speaker_frames, global_frames, norm_vars

    def struct(self):
        try:
            return pk_mi355_online_cmvn_spec_t(int(self.cmn_window), int(self.speaker_frames), int(self.global_frames), int(self.norm_vars))
        except (TypeError, ValueError, OverflowError) as e:
            raise PkCodeError(-1, "online cmvn spec: %s" % e)

    def check(self, global_stats=None, dim=None):
        """global_stats: the 2 x (D + 1) record, or None; dim: D when there is no record to take it from."""
        g = None if global_stats is None else _global_record(global_stats, dim)
        D = dim if g is None else g.shape[1] - 1
        _check_code(lib().pk_mi355_online_cmvn_check(C.byref(self.struct()), None if g is None else _dp(g), int(D or 0)))

    def __repr__(self):
        return "OnlineCmvnSpec(cmn_window=%r, speaker_frames=%r, global_frames=%r, norm_vars=%r)" % (
            self.cmn_window, self.speaker_frames, self.global_frames, self.norm_vars)


def _global_record(stats, dim=None):
    """One 2 x (D + 1) record of doubles; another shape is refused here."""
    try:
        a = np.ascontiguousarray(stats, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise PkCodeError(-1, "global statistics are not numbers: %s" % e)
    if a.ndim != 2 or a.shape[0] != 2 or a.shape[1] < 2 or (dim is not None and a.shape[1] != dim + 1):
        raise PkCodeError(-1, "global statistics have shape %s, expected [2][%s]" % (a.shape, "D + 1" if dim is None else dim + 1))
    return a


ONLINE_CMVN_KEYS = ("cmn_window", "speaker_frames", "global_frames")


def parse_norm(text):
    """A NormSpec from "key=value,key=value,...": mode (sliding | none | utterance | speaker), norm_means and norm_vars
    (true | false | 1 | 0); omitted keys take NormSpec's defaults.  mode=online gives an OnlineCmvnSpec instead, with the
    keys cmn_window, speaker_frames, global_frames (integers) and norm_vars.  ValueError, the key named, for an unknown
    key, a value that does not parse, or a key that does not go with the mode.  Nothing else is checked here: the
    library refuses a bad spec where it is used."""
    switch = {"true": True, "false": False, "1": True, "0": False}
    modes = dict(NORM_MODES, online="online")
    fields = {"mode": modes, "norm_means": switch, "norm_vars": switch}
    keys = sorted(list(fields) + list(ONLINE_CMVN_KEYS))
    given = {}
    for item in [t.strip() for t in text.split(",") if t.strip()]:
        key, eq, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if key not in keys:
            raise ValueError("norm spec: unknown key '%s' (the keys are %s)" % (key, ", ".join(keys)))
        if key in given:
            raise ValueError("norm spec: key '%s' given twice" % key)
        if key in ONLINE_CMVN_KEYS:
            try:
                given[key] = int(value) if eq else None
            except ValueError:
                given[key] = None
            if given[key] is None:
                raise ValueError("norm spec: bad value '%s' for key '%s' (an integer)" % (value, key))
            continue
        if not eq or value not in fields[key]:
            raise ValueError("norm spec: bad value '%s' for key '%s' (one of %s)" % (value, key, ", ".join(sorted(fields[key]))))
        given[key] = fields[key][value]
    if given.get("mode") == "online":
        if "norm_means" in given:
            raise ValueError("norm spec: key 'norm_means' does not go with mode=online (online CMVN always normalises the means)")
        del given["mode"]
        return OnlineCmvnSpec(**given)
    for key in ONLINE_CMVN_KEYS:
        if key in given:
            raise ValueError("norm spec: key '%s' needs mode=online" % key)
    return NormSpec(**given)


def _stats_records(stats, n, dim):
    """n records of 2 x (dim + 1) doubles -> one float64 array [n][2][dim + 1]; another shape is refused here."""
    try:
        a = np.ascontiguousarray(stats, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise PkCodeError(-1, "speaker statistics are not numbers: %s" % e)
    if a.shape != (n, 2, dim + 1):
        raise PkCodeError(-1, "speaker statistics have shape %s, expected [%d][2][%d]" % (a.shape, n, dim + 1))
    return a


def cmvn_normalize(feats, spec, stats=None):
    """The rule of a NormSpec on the host for one [T][D] matrix (pk_mi355_norm_apply: the restatement the GPU path is
    held to) -> (normalised float32 [T][D], the 2 x (D + 1) float64 record an "utterance" call accumulated, else None).
    stats: the 2 x (D + 1) record of mode "speaker".  Mode "sliding" is CMVN's rule and refused here."""
    x = _f32(feats)
    if x.ndim != 2 or x.shape[1] < 1:
        raise PkCodeError(-1, "features have shape %s, expected [T][D]" % (x.shape,))
    T, D = x.shape
    st = spec.struct()
    rec = None if stats is None else _stats_records([stats], 1, D)
    y, acc = np.zeros((T, D), np.float32), np.zeros((2, D + 1), np.float64)
    _check_code(lib().pk_mi355_norm_apply(C.byref(st), _fp(x), T, D, None if rec is None else _dp(rec), _fp(y), _dp(acc)))
    return y, (acc if st.mode == NORM_MODES["utterance"] else None)


def cmvn_online(feats, spec, global_stats=None, speaker_stats=None, return_state=False):
    """The rule of an OnlineCmvnSpec on the host for one [T][D] matrix (pk_mi355_online_cmvn_apply: the restatement the
    GPU path is held to) -> normalised float32 [T][D].  global_stats, speaker_stats: 2 x (D + 1) records or None.
    return_state: also the 2 x (D + 1) float64 window state behind the last frame (sums and frames seen, sums of
    squares and 0)."""
    x = _f32(feats)
    if x.ndim != 2 or x.shape[1] < 1:
        raise PkCodeError(-1, "features have shape %s, expected [T][D]" % (x.shape,))
    T, D = x.shape
    st = spec.struct()
    g = None if global_stats is None else _global_record(global_stats, D)
    spk = None if speaker_stats is None else _stats_records([speaker_stats], 1, D)
    y, state = np.zeros((T, D), np.float32), np.zeros((2, D + 1), np.float64)
    _check_code(lib().pk_mi355_online_cmvn_apply(C.byref(st), _fp(x), T, D, None if g is None else _dp(g), None if spk is None else _dp(spk),
                                                 _fp(y), _dp(state)))
    return (y, state) if return_state else y


class DeltaSpec:
    """A delta-features specification (pk_mi355_deltas_spec_t): Kaldi's add-deltas, order 1 to 3
    and window 1 to 8 (Kaldi's defaults 2 and 2).  Nothing is checked here: the library refuses a bad spec (PkCodeError,
    the field named) wherever one is used."""

    def __init__(self, order=2, window=2):
        self.order, self.window = order, window

    def struct(self):
        try:
            return pk_mi355_deltas_spec_t(int(self.order), int(self.window))
        except (TypeError, ValueError, OverflowError) as e:
            raise PkCodeError(-1, "deltas spec: %s" % e)

    def check(self):
        _check_code(lib().pk_mi355_deltas_check(C.byref(self.struct())))

    def dim(self, base):
        """The output dimension for `base` input features: (order + 1) * base."""
        n = lib().pk_mi355_deltas_dim(C.byref(self.struct()), int(base))
        _check_code(min(n, 0))
        return n

    def __repr__(self):
        return "DeltaSpec(order=%r, window=%r)" % (self.order, self.window)


def parse_deltas(text):
    """A DeltaSpec from "order=2,window=2"; omitted keys take DeltaSpec's defaults.  ValueError, the key named, for an
    unknown key, a key given twice or a value that is not an integer.  The ranges are the library's to refuse."""
    given = {}
    for item in [t.strip() for t in text.split(",") if t.strip()]:
        key, eq, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if key not in ("order", "window"):
            raise ValueError("deltas spec: unknown key '%s' (the keys are order, window)" % key)
        if key in given:
            raise ValueError("deltas spec: key '%s' given twice" % key)
        try:
            given[key] = int(value) if eq else None
        except ValueError:
            given[key] = None
        if given[key] is None:
            raise ValueError("deltas spec: bad value '%s' for key '%s' (an integer)" % (value, key))
    return DeltaSpec(**given)


def delta_scales(spec):
    """The scale table of a DeltaSpec, float32 [order + 1][2 * order * window + 1]: row i holds block i's scales centred
    (entry j at column order * window + j), zeros around them."""
    st = spec.struct()
    _check_code(lib().pk_mi355_deltas_check(C.byref(st)))
    out = np.zeros((st.order + 1, 2 * st.order * st.window + 1), np.float32)
    _check_code(lib().pk_mi355_deltas_scales(C.byref(st), _fp(out)))
    return out


def add_deltas(feats, spec):
    """The rule of a DeltaSpec on the host for one [T][Db] matrix (pk_mi355_deltas_apply: the restatement the GPU path is
    held to) -> float32 [T][(order + 1) * Db]."""
    x = _f32(feats)
    if x.ndim != 2 or x.shape[1] < 1:
        raise PkCodeError(-1, "features have shape %s, expected [T][D]" % (x.shape,))
    st = spec.struct()
    _check_code(lib().pk_mi355_deltas_check(C.byref(st)))
    T, D = x.shape
    y = np.zeros((T, (st.order + 1) * D), np.float32)
    _check_code(lib().pk_mi355_deltas_apply(C.byref(st), _fp(x), T, D, _fp(y)))
    return y


class TransformSpec:
    """A feature-transform specification (pk_mi355_transform_spec_t): Kaldi's splice-feats with
    left_context / right_context frames, then transform-feats with `matrix` [rows][cols] -- cols = (left + right + 1) *
    in_dim (linear) or one more (affine: the last column is the offset).  in_dim is required when left_context =
    right_context = 0 (a 41-column matrix may be 41 -> linear or 40 -> affine) and when matrix is None (no global stage:
    the scorer then takes per-utterance matrices only); otherwise it is derived from cols.  The ranges and the matrix
    entries are the library's to refuse (PkCodeError, the field named) wherever the spec is used."""

    def __init__(self, matrix=None, left_context=0, right_context=0, in_dim=None):
        self.matrix = None if matrix is None else _f32(matrix)
        self.left_context, self.right_context = left_context, right_context
        if self.matrix is not None and self.matrix.ndim != 2:
            raise PkCodeError(-1, "transform spec: the matrix has shape %s, expected [rows][cols]" % (self.matrix.shape,))
        if in_dim is None:
            try:
                w = int(left_context) + int(right_context) + 1
            except (TypeError, ValueError) as e:
                raise PkCodeError(-1, "transform spec: %s" % e)
            if self.matrix is None:
                raise PkCodeError(-1, "transform spec: in_dim is required without a matrix")
            cols = self.matrix.shape[1]
            if w <= 1:
                raise PkCodeError(-1, "transform spec: in_dim is required when left_context = right_context = 0 (a %d-column matrix "
                                  "may be %d -> linear or %d -> affine)" % (cols, cols, cols - 1))
            # w > 1: at most one of cols and cols - 1 is a multiple of w; neither: the library names both numbers
            in_dim = (cols - 1) // w if cols % w else cols // w
        self.in_dim = in_dim

    def struct(self):
        try:
            m = self.matrix
            return pk_mi355_transform_spec_t(int(self.left_context), int(self.right_context), int(self.in_dim), 0 if m is None else m.shape[0],
                                             0 if m is None else m.shape[1], None if m is None else _fp(m))
        except (TypeError, ValueError, OverflowError) as e:
            raise PkCodeError(-1, "transform spec: %s" % e)

    def check(self):
        _check_code(lib().pk_mi355_transform_check(C.byref(self.struct())))

    @property
    def out_dim(self):
        """The output dimension: the matrix's rows, or in_dim without a matrix."""
        return _check_code(lib().pk_mi355_transform_out_dim(C.byref(self.struct())))

    def __repr__(self):
        return "TransformSpec(matrix=%s, left_context=%r, right_context=%r, in_dim=%r)" % (
            None if self.matrix is None else "<%d x %d>" % self.matrix.shape, self.left_context, self.right_context, self.in_dim)


def parse_transform(text):
    """A TransformSpec from "matrix=final.mat,left_context=3,right_context=3[,in_dim=13]"; the matrix is read with
    read_kaldi_matrix.  ValueError, the key named, for an unknown key, a key given twice, a context or in_dim that is not
    an integer, or no matrix."""
    given = {}
    for item in [t.strip() for t in text.split(",") if t.strip()]:
        key, eq, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if key not in ("matrix", "left_context", "right_context", "in_dim"):
            raise ValueError("transform spec: unknown key '%s' (the keys are matrix, left_context, right_context, in_dim)" % key)
        if key in given:
            raise ValueError("transform spec: key '%s' given twice" % key)
        if key == "matrix":
            if not eq or not value:
                raise ValueError("transform spec: bad value '%s' for key 'matrix' (a file)" % value)
            given[key] = value
            continue
        try:
            given[key] = int(value) if eq else None
        except ValueError:
            given[key] = None
        if given[key] is None:
            raise ValueError("transform spec: bad value '%s' for key '%s' (an integer)" % (value, key))
    if "matrix" not in given:
        raise ValueError("transform spec: no matrix (matrix=FILE)")
    given["matrix"] = read_kaldi_matrix(given["matrix"])
    return TransformSpec(**given)


def transform_feats(feats, spec):
    """The rule of a TransformSpec on the host for one [T][in_dim] matrix (pk_mi355_transform_apply: the restatement the
    GPU path is held to) -> float32 [T][out_dim]."""
    x = _f32(feats)
    st = spec.struct()
    _check_code(lib().pk_mi355_transform_check(C.byref(st)))
    if x.ndim != 2 or x.shape[1] != st.in_dim:
        raise PkCodeError(-1, "features have shape %s, the transform reads [T][%d]" % (x.shape, st.in_dim))
    T = x.shape[0]
    y = np.zeros((T, spec.out_dim), np.float32)
    _check_code(lib().pk_mi355_transform_apply(C.byref(st), _fp(x), T, _fp(y)))
    return y


def splice_feats(feats, left, right):
    """Kaldi's splice-feats on the host: [T][D] -> [T][(left + right + 1) * D], frame t the frames t - left .. t + right with
    the first and last frame repeated at the edges.  A copy; no arithmetic."""
    x = _f32(feats)
    if x.ndim != 2:
        raise PkCodeError(-1, "features have shape %s, expected [T][D]" % (x.shape,))
    if left < 0 or right < 0:
        raise PkCodeError(-1, "splice: negative context (%d, %d)" % (left, right))
    T = x.shape[0]
    if T == 0:
        return np.zeros((0, (left + right + 1) * x.shape[1]), np.float32)
    idx = np.clip(np.arange(T)[:, None] + np.arange(-left, right + 1)[None, :], 0, T - 1)
    return np.ascontiguousarray(x[idx].reshape(T, -1))


class CMVN:
    """cmvn.h:17-26.  Sliding-window mean normalisation with a global prior."""

    def __init__(self, global_stats, raw_feats):
        self.global_stats = _f32(global_stats)
        self.raw = _f32(raw_feats)

    def get_frames(self):
        g = pk_vector_t(self.global_stats.shape[0], _fp(self.global_stats))
        raw = _as_matrix(self.raw) if self.raw.size else pk_matrix_t(0, 40, None)
        out = pk_matrix_t(0, 0, None)
        _check(lib().pk_mi355_cmvn_apply(C.byref(g), C.byref(raw), C.byref(out)))
        return _take_matrix(out)


class AcousticModel:
    """am.h:23-52 + nnet.h:88-104.

    layers: list of ("linear", W[out][in], b[out]) | ("relu",) | ("normalize",) | ("softmax",)
            | ("sigmoid",) | ("tanh",) | ("pnorm", out_dim) | ("add", v[dim]) | ("mul", v[dim])   (f32 precision only)
            | ("splice", [offsets])   a time-splice between hidden layers (f32 only; the whole-utterance scorers)
    prior:  pdf prior probabilities (the log is taken at load, am.cc:43)
    """
    _KIND = {"relu": RELU, "normalize": NORMALIZE, "softmax": SOFTMAX, "sigmoid": SIGMOID, "tanh": TANH}

    PRECISIONS = {"f32": 0, "f16x3": 1, "f16": 2}

    def __init__(self, layers=None, prior=None, left_context=0, right_context=0, tid2pdf=None,
                 num_pdfs=None, precision="f32"):
        L = lib()
        self._h = L.pk_mi355_am_create()
        _check(L.pk_mi355_am_set_precision(self._h, self.PRECISIONS[precision]))
        if layers is not None:
            width = 0                        # what the layers so far leave (a p-norm's input width)
            for l in layers:
                if l[0] == "linear":
                    W, b = _f32(l[1]), _f32(l[2])
                    _check(L.pk_mi355_am_add_linear(self._h, W.shape[1], W.shape[0], _fp(W), _fp(b)))
                    width = W.shape[0]
                elif l[0] in ("add", "mul"):
                    v = _f32(l[1]).ravel()
                    _check(L.pk_mi355_am_add_vector_layer(self._h, _LAYER_KIND[l[0]], v.shape[0], _fp(v)))
                    width = v.shape[0]
                elif l[0] == "pnorm":
                    if width <= 0:
                        raise PkError("a p-norm layer needs a layer in front of it that states the width")
                    _check(L.pk_mi355_am_add_pnorm(self._h, width, int(l[1])))
                    width = int(l[1])
                elif l[0] == "splice":
                    if width <= 0:
                        raise PkError("network must start with a linear layer when splicing")
                    o = np.ascontiguousarray(l[1], dtype=np.int32).ravel()
                    _check(L.pk_mi355_am_add_time_splice(self._h, width, o.ctypes.data_as(C.POINTER(C.c_int32)), o.shape[0]))
                    width *= o.shape[0]
                else:
                    _check(L.pk_mi355_am_add_layer(self._h, self._KIND[l[0]]))
            pr = None if prior is None else _f32(prior)
            n = int(num_pdfs) if num_pdfs is not None else (0 if pr is None else pr.shape[0])
            tid = None if tid2pdf is None else np.ascontiguousarray(tid2pdf, dtype=np.int32)
            _check(L.pk_mi355_am_finalize(
                self._h, None if pr is None else _fp(pr), n, left_context, right_context,
                None if tid is None else tid.ctypes.data_as(C.POINTER(C.c_int32)),
                0 if tid is None else tid.shape[0]))

    @classmethod
    def read(cls, nnet_path, prior_path, tid2pdf_path, left_context, right_context, num_pdfs,
             precision="f32"):
        """AcousticModel::Read (am.cc:23-63) from the converted model files."""
        self = cls(precision=precision)
        _check(lib().pk_mi355_am_read(self._h, nnet_path.encode(), prior_path.encode(),
                                      None if tid2pdf_path is None else tid2pdf_path.encode(),
                                      left_context, right_context, num_pdfs))
        return self

    @classmethod
    def load(cls, config_path, precision="f32"):
        """pk_load's model part (pocketkaldi.cc:72-144): the reference's key = value model file.
        Returns (model, cmvn_global_stats[41])."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        stats = np.zeros(41, dtype=np.float32)
        self._h = None
        _check(lib().pk_mi355_load(config_path.encode(), cls.PRECISIONS[precision], C.byref(h), _fp(stats)))
        self._h = h.value
        return self, stats

    @classmethod
    def load_stats(cls, config_path, precision="f32", stats_cap=129):
        """load for a model of any feature dimension (pk_mi355_load_stats): (model, cmvn_global_stats[feat_dim + 1])."""
        self = cls.__new__(cls)
        h, n = C.c_void_p(), C.c_int()
        stats = np.zeros(max(int(stats_cap), 1), dtype=np.float32)
        self._h = None
        _check_code(lib().pk_mi355_load_stats(os.fspath(config_path).encode(), cls.PRECISIONS[precision], C.byref(h), _fp(stats), int(stats_cap),
                                              C.byref(n)))
        self._h = h.value
        return self, stats[:n.value].copy()

    def set_softmax(self, mode):
        """"stable" (default): overflow-safe log-softmax; "reference": the reference's operations one by one."""
        _check(lib().pk_mi355_am_set_softmax(self._h, {"stable": 0, "reference": 1}[mode]))
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_am_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def num_pdfs(self):
        return lib().pk_mi355_am_num_pdfs(self._h)

    def feat_dim(self):
        """The per-frame feature dimension; 0 until the model is finalized."""
        return lib().pk_mi355_am_feat_dim(self._h)

    def input_dim(self):
        return lib().pk_mi355_am_input_dim(self._h)

    def time_context(self):
        """(Lh, Rh): the frames the time-splice layers consume together on the left and on the right; (0, 0) without any."""
        l, r = C.c_int(), C.c_int()
        _check(lib().pk_mi355_am_time_context(self._h, C.byref(l), C.byref(r)))
        return l.value, r.value

    def transition_id_to_pdf_id(self, tid):
        return lib().pk_mi355_am_transition_to_pdf(self._h, int(tid))

    def flops_per_frame(self):
        return lib().pk_mi355_am_flops_per_frame(self._h)

    def blob(self):
        """(device pointer, bytes) of the packed weights, for the RCCL broadcast."""
        return lib().pk_mi355_am_blob_device_ptr(self._h), lib().pk_mi355_am_blob_bytes(self._h)

    def broadcast(self, rccl_comm, root=0, stream=None, src=None):
        """pk_mi355_am_broadcast[_from]: one ncclBroadcast into this model's blob over the caller's ncclComm_t
        (an integer handle); with src, the root sends that model's blob instead of its own."""
        _check(lib().pk_mi355_am_broadcast_from(self._h, None if src is None else src.handle, C.c_void_p(rccl_comm),
                                                int(root), None if stream is None else C.c_void_p(stream)))

    def exponents(self):
        """f16x3 / f16: (w_exp, x_exp) per affine layer -- the exact power-of-two operand scalings."""
        w = np.zeros(64, dtype=np.int32)
        x = np.zeros(64, dtype=np.int32)
        n = lib().pk_mi355_am_get_exponents(self._h, w.ctypes.data_as(C.POINTER(C.c_int32)),
                                            x.ctypes.data_as(C.POINTER(C.c_int32)), 64)
        if n < 0:
            _check(n)
        return w[:n].copy(), x[:n].copy()

    def set_input_exponents(self, x_exp):
        x = np.ascontiguousarray(x_exp, dtype=np.int32)
        _check(lib().pk_mi355_am_set_input_exponents(self._h, x.ctypes.data_as(C.POINTER(C.c_int32)), x.shape[0]))

    def calibrate(self, feats):
        """f16x3 / f16: set every operand's exponent from CMVN'd features [T][feat_dim] (pk_mi355_am_calibrate)."""
        feats = _f32(feats)
        m = _as_matrix(feats)
        _check(lib().pk_mi355_am_calibrate(self._h, C.byref(m)))
        return self

    def propagate(self, x):
        """Nnet::Propagate (nnet.cc:149-163): x [T][in_dim] -> [T][out_dim]."""
        x = _f32(x)
        m_in = _as_matrix(x) if x.size else pk_matrix_t(0, x.shape[1], None)
        m_out = pk_matrix_t(0, 0, None)
        _check(lib().pk_mi355_nnet_propagate(self._h, C.byref(m_in), C.byref(m_out)))
        return _take_matrix(m_out)


_LAYER_KIND = {"linear": LINEAR, "relu": RELU, "normalize": NORMALIZE, "softmax": SOFTMAX, "add": ADD, "mul": MUL, "sigmoid": SIGMOID,
               "tanh": TANH, "pnorm": PNORM, "splice": TIME_SPLICE}


def apply_layer(kind, x, param=None):
    """The rule of one layer of kind "add" / "mul" (param: the vector), "sigmoid" / "tanh" or "pnorm" (param: out_dim) on the
    host for rows x [T][dim] (pk_mi355_layer_apply_host: the restatement the GPU layers are held to) -> float32 rows."""
    x = _f32(x)
    if x.ndim != 2:
        raise PkCodeError(-1, "rows have shape %s, expected [T][dim]" % (x.shape,))
    k = _LAYER_KIND[kind] if isinstance(kind, str) else int(kind)
    T, D = x.shape
    v, O = None, D
    if k == PNORM:
        O = int(param)
    elif k in (ADD, MUL):
        v = _f32(param).ravel()
        if v.shape[0] != D:
            raise PkCodeError(-1, "the vector has %d entries, the rows %d" % (v.shape[0], D))
    y = np.zeros((T, max(O, 0)), np.float32)
    _check_code(lib().pk_mi355_layer_apply_host(k, _fp(x), T, D, None if v is None else _fp(v), O, _fp(y)))
    return y


def time_splice(x, offsets):
    """The time-splice layer's rule on the host in its shrinking form (pk_mi355_time_splice_host): rows x [T][dim] ->
    [T - lo - hi][n dim], row r = the input frames r + lo + o_c side by side, every bit kept."""
    x = _f32(x)
    if x.ndim != 2:
        raise PkCodeError(-1, "rows have shape %s, expected [T][dim]" % (x.shape,))
    o = np.ascontiguousarray(offsets, dtype=np.int32).ravel()
    T, D = x.shape
    lo, hi = (max(0, -int(o[0])), max(0, int(o[-1]))) if o.size else (0, 0)
    y = np.zeros((max(T - lo - hi, 0), max(o.size * D, 1)), np.float32)
    _check_code(lib().pk_mi355_time_splice_host(_fp(x), T, D, o.ctypes.data_as(C.POINTER(C.c_int32)), o.shape[0], _fp(y)))
    return y[:, :o.size * D]


def write_nnet(path, layers):
    """The NNT0 model file of `layers` (AcousticModel's list; all nine kinds), as tool/convert_am.py of the reference
    writes kinds 0 to 3 and 5: LAY0 sections, a Linear's W as MAT0 of VEC0 rows and its bias, an add / mul layer's
    vector as one VEC0, a p-norm's in_dim and out_dim as two int32 (in_dim: the width the layers in front leave), a
    time-splice's in_dim, n and its n offsets as int32."""
    import struct

    def vec(v):
        v = _f32(v).ravel()
        return b"VEC0" + struct.pack("<ii", 4 * v.shape[0] + 4, v.shape[0]) + v.tobytes()

    out = [b"NNT0" + struct.pack("<ii", 4, len(layers))]
    width = 0
    for l in layers:
        kind = _LAYER_KIND[l[0]]
        out.append(b"LAY0" + struct.pack("<ii", 4, kind))
        if kind == LINEAR:
            W, b = _f32(l[1]), _f32(l[2])
            out.append(b"MAT0" + struct.pack("<iii", 8, W.shape[0], W.shape[1]) + b"".join(vec(r) for r in W) + vec(b))
            width = W.shape[0]
        elif kind in (ADD, MUL):
            out.append(vec(l[1]))
            width = _f32(l[1]).size
        elif kind == PNORM:
            if width <= 0:
                raise PkError("a p-norm layer needs a layer in front of it that states the width")
            out.append(struct.pack("<ii", width, int(l[1])))
            width = int(l[1])
        elif kind == TIME_SPLICE:
            if width <= 0:
                raise PkError("network must start with a linear layer when splicing")
            o = [int(v) for v in l[1]]
            out.append(struct.pack("<ii%di" % len(o), width, len(o), *o))
            width *= len(o)
    with open(path, "wb") as f:
        f.write(b"".join(out))


def device_logf(x):
    """The front-end kernel's logf on an array (parity-test hook)."""
    x = _f32(x).ravel()
    out = np.empty_like(x)
    _check(lib().pk_mi355_test_logf(_fp(x), x.shape[0], _fp(out)))
    return out


def device_srfft512(frames):
    """The front-end kernel's 512-point real FFT on [n][512] frames (parity-test hook)."""
    x = _f32(frames).reshape(-1, 512)
    out = np.empty_like(x)
    _check(lib().pk_mi355_test_srfft512(_fp(x), x.shape[0], _fp(out)))
    return out


class _Pinned:
    def __init__(self, nbytes):
        self.ptr = lib().pk_mi355_host_malloc(max(int(nbytes), 1))
        if not self.ptr:
            raise PkError(lib().pk_mi355_last_error().decode())

    def __del__(self):
        try:
            lib().pk_mi355_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


def pinned_i16(n):
    """An int16 numpy array of n samples in page-locked host memory (pk_mi355_host_malloc)."""
    owner = _Pinned(2 * int(n))
    buf = (C.c_int16 * int(n)).from_address(owner.ptr)
    arr = np.frombuffer(buf, dtype=np.int16)
    arr = arr.view(_OwnedArray)
    arr._owner = owner
    return arr


class _OwnedArray(np.ndarray):
    _owner = None

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


FEATURE_KINDS = {"normalized": 0, "raw": 1}         # PK_MI355_FEATS_*


def _feature_kind(kind):
    if kind not in FEATURE_KINDS:
        raise PkCodeError(-1, "feature kind %r (one of %s)" % (kind, ", ".join(sorted(FEATURE_KINDS))))
    return FEATURE_KINDS[kind]


def _feature_matrices(feats, feat_dim):
    """A list of [T][feat_dim] arrays -> (pk_matrix_t array, the float32 arrays it borrows)."""
    keep = []
    for i, f in enumerate(feats):
        try:
            f = _f32(f)
        except (TypeError, ValueError) as e:
            raise PkCodeError(-1, "features %d are not a float matrix: %s" % (i, e))
        if f.ndim != 2 or f.shape[1] != feat_dim:
            raise PkCodeError(-1, "features %d have shape %s, expected [T][%d]" % (i, f.shape, feat_dim))
        keep.append(f)
    arr = (pk_matrix_t * max(len(keep), 1))()
    for i, f in enumerate(keep):
        arr[i] = _as_matrix(f)
    return arr, keep


def _feature_frames(frames, feat_dim):
    """[n][feat_dim] -> a float32 array the library may read; another shape is refused here, by name."""
    try:
        f = _f32(frames)
    except (TypeError, ValueError) as e:
        raise PkCodeError(-1, "frames are not a float matrix: %s" % e)
    if f.ndim != 2 or f.shape[1] != feat_dim:
        raise PkCodeError(-1, "frames have shape %s, expected [n][%d]" % (f.shape, feat_dim))
    return f


class Decodable:
    """decodable.h:15-41 over the C ABI (what decoder.cc consumes)."""

    def __init__(self, am, prob_scale, feats):
        feats = _f32(feats)
        self._d = pk_decodable_t()
        self._am = am
        m = _as_matrix(feats)
        lib().pk_decodable_init(C.byref(self._d), am.handle, float(prob_scale), C.byref(m))
        if feats.shape[0] > 0 and self._d.log_prob.ncol != feats.shape[0]:
            raise PkError(lib().pk_mi355_last_error().decode() or "pk_decodable_init failed")

    @classmethod
    def _from_struct(cls, d, am):
        self = cls.__new__(cls)
        self._d, self._am = d, am
        return self

    def loglikelihood(self, frame, trans_id):
        return lib().pk_decodable_loglikelihood(C.byref(self._d), int(frame), int(trans_id))

    def is_last_frame(self, frame):
        return bool(lib().pk_decodable_islastframe(C.byref(self._d), int(frame)))

    def log_prob(self):
        """The host matrix as numpy [T][num_pdfs] (a copy)."""
        lp = self._d.log_prob
        if lp.ncol == 0:
            return np.zeros((0, lp.nrow), dtype=np.float32)
        return np.ctypeslib.as_array(lp.data, shape=(lp.ncol, lp.nrow)).copy()

    def destroy(self):
        if self._d is not None:
            lib().pk_decodable_destroy(C.byref(self._d))
            self._d = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _raise_last():
    """The library's last error as a PkCodeError."""
    raise PkCodeError(lib().pk_mi355_last_error_code(), lib().pk_mi355_last_error().decode())


def _byref(spec):
    return None if spec is None else C.byref(spec.struct())


def _check_spec_types(transform, deltas, frontend=None):
    """with_transform's arguments: a TransformSpec, and a DeltaSpec / FrontendSpec where one is given."""
    for name, spec, kind in (("transform", transform, TransformSpec), ("deltas", deltas, DeltaSpec), ("frontend", frontend, FrontendSpec)):
        if (spec is not None or kind is TransformSpec) and not isinstance(spec, kind):
            raise TypeError("%s must be a %s, not %s" % (name, kind.__name__, type(spec).__name__))


def _stats_route(am, global_stats):
    """(statistics or None, True when they go to the _create_stats entries).  41 entries: the 40-dim entries, with every
    refusal of theirs; feat_dim + 1: the entries that take the model's own dimension; anything else is refused here."""
    if global_stats is None:
        return None, False
    g = _f32(global_stats)
    if g.shape == (41,):
        return g, False
    dim = lib().pk_mi355_am_feat_dim(am.handle)
    if dim > 0 and g.shape == (dim + 1,):
        return g, True
    raise PkError("global_stats must have 41 entries, or feat_dim + 1 = %d for this model (got %s)"
                  % (dim + 1, "x".join(str(n) for n in g.shape)))


def _create_scorer(live, audio, am, global_stats, count, capacity, frontend=None, deltas=None, transform=None):
    """The handle of a scorer: the one choice among the library's create entries.  live: an online scorer of `count` slots,
    else a batch of `count` utterances; audio: `capacity` in samples and a front-end (the default FrontendSpec when deltas
    or a transform come without one), else in frames and global_stats may be None."""
    L = lib()
    count, capacity = int(count), int(capacity)
    if transform is not None or deltas is not None or frontend is not None:
        g = _f32(global_stats) if audio or global_stats is not None else None
        if audio and frontend is None:
            frontend = FrontendSpec()
        if transform is not None:
            make, specs = (L.pk_mi355_transform_stream_create if live else L.pk_mi355_transform_batch_create), (transform, deltas, frontend)
        elif deltas is not None:
            make, specs = (L.pk_mi355_deltas_stream_create if live else L.pk_mi355_deltas_batch_create), (deltas, frontend)
        else:
            make, specs = (L.pk_mi355_frontend_stream_create if live else L.pk_mi355_frontend_batch_create), (frontend,)
        stats = (None, 0) if g is None else (_fp(g.ravel()), g.size)
        h = make(am.handle, *[_byref(spec) for spec in specs], *stats, count, capacity)
    elif audio:                             # the reference's 40-bin front-end and 41 statistics
        g = _f32(global_stats)
        if g.shape != (41,):
            raise PkError("global_stats must have 41 entries")
        h = (L.pk_mi355_stream_create if live else L.pk_mi355_batch_create)(am.handle, _fp(g), count, capacity)
        if not h and not live:              # (a BatchScorer's oldest failures carry no code)
            raise PkError(L.pk_mi355_last_error().decode())
    else:
        g, own_dim = _stats_route(am, global_stats)
        if own_dim:
            h = (L.pk_mi355_features_stream_create_stats if live else L.pk_mi355_features_batch_create_stats)(am.handle, _fp(g), g.shape[0], count, capacity)
        else:
            h = (L.pk_mi355_features_stream_create if live else L.pk_mi355_features_batch_create)(am.handle, None if g is None else _fp(g), count, capacity)
    if not h:
        _raise_last()
    return h


class BatchScorer:
    """Many utterances in flight: PCM -> fbank -> CMVN -> nnet -> log-likelihoods, all in HBM."""

    def __init__(self, am, global_stats, max_utts, max_total_samples, frontend=None, deltas=None, transform=None):
        """frontend: a FrontendSpec of the model's feature dimension (pk_mi355_frontend_batch_create; global_stats: that
        many sums, then the count).  Without it: the reference's 40-bin front-end and 41 statistics.
        deltas: a DeltaSpec (pk_mi355_deltas_batch_create): the front-end (the default FrontendSpec when none is given),
        the statistics and the normalisation are then at base_dim() = feat_dim / (order + 1).
        transform: a TransformSpec (pk_mi355_transform_batch_create) whose out_dim is the model's feat_dim: the front-end,
        the statistics and the normalisation are then at base_dim() = in_dim() / (order + 1), in_dim() without deltas."""
        self._am = am
        self._keep = None
        self._h = _create_scorer(False, True, am, global_stats, max_utts, max_total_samples, frontend, deltas, transform)

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_waves(self, waves, rates=None):
        """rates: the sample rate of every wave (None: 16000); the others are converted on the GPU on the way in."""
        waves = [_f32(w) for w in waves]
        arr = (pk_vector_t * max(len(waves), 1))()
        for i, w in enumerate(waves):
            arr[i].dim, arr[i].data = w.shape[0], _fp(w)
        if rates is None:
            _check(lib().pk_mi355_batch_set_waves(self._h, arr, len(waves)))
        else:
            _check_code(lib().pk_mi355_resample_set_waves(self._h, arr, _rates_array(rates, len(waves)), len(waves)))

    def set_waves_i16(self, waves):
        waves = [np.ascontiguousarray(w, dtype=np.int16) for w in waves]
        cat = np.concatenate(waves) if waves else np.zeros(0, np.int16)
        ns = (C.c_int * max(len(waves), 1))(*[w.shape[0] for w in waves])
        _check(lib().pk_mi355_batch_set_waves_i16(self._h, cat.ctypes.data_as(C.POINTER(C.c_int16)), ns,
                                                  len(waves)))

    def set_waves_i16_raw(self, samples, num_samples):
        """Concatenated int16 samples (e.g. a pinned_i16() array) + per-utterance counts; no host copy."""
        ns = (C.c_int * max(len(num_samples), 1))(*[int(n) for n in num_samples])
        self._keep = samples
        _check(lib().pk_mi355_batch_set_waves_i16(self._h, samples.ctypes.data_as(C.POINTER(C.c_int16)), ns,
                                                  len(num_samples)))

    def set_waves_device(self, device_ptr, num_samples, keep_alive=None):
        """PCM already in HBM: device_ptr -> concatenated float samples."""
        ns = (C.c_int * max(len(num_samples), 1))(*[int(n) for n in num_samples])
        self._keep = keep_alive
        _check(lib().pk_mi355_batch_set_waves_device(self._h, C.c_void_p(device_ptr), ns, len(num_samples)))

    def feat_dim(self):
        return lib().pk_mi355_features_dim(self._h)

    def base_dim(self):
        """The dimension in front of the deltas -- the front-end's, raw rows', statistics' -- on a scorer made with
        deltas=; feat_dim() on every other."""
        return lib().pk_mi355_deltas_base_dim(self._h)

    def in_dim(self):
        """The width of the rows the transform reads on a scorer made with transform=; feat_dim() on every other."""
        return lib().pk_mi355_transform_in_dim(self._h)

    def set_utt_transforms(self, matrices):
        """A scorer made with transform=: one [feat_dim][feat_dim] (linear) or [feat_dim][feat_dim + 1] (affine) matrix per
        utterance of the next score call, which consumes them; applied behind the global matrix."""
        n = len(matrices)
        a = np.ascontiguousarray(np.stack([_f32(m) for m in matrices])) if n else np.zeros((0, self.feat_dim(), self.feat_dim()), np.float32)
        if a.ndim != 3:
            raise PkCodeError(-1, "per-utterance transforms have shape %s, expected [utterances][rows][cols]" % (a.shape,))
        _check_code(lib().pk_mi355_transform_set_utt(self._h, _fp(a) if n else None, a.shape[1], a.shape[2], n))

    def set_features(self, feats, kind="normalized"):
        """Features instead of audio: one [T][feat_dim] matrix per utterance.  kind "normalized": ready for the splice
        (what Decodable takes); "raw": features the scorer's normalisation is applied to first -- the sliding-window CMVN
        (40-dim log-mel fbank, or the model's own dimension on a FeatureScorer made with feat_dim + 1 statistics) or
        what set_norm selected (any scorer, statistics or not)."""
        k = _feature_kind(kind)
        arr, keep = _feature_matrices(feats, self.base_dim() if k == FEATURE_KINDS["raw"] else self.feat_dim())
        _check_code(lib().pk_mi355_features_set(self._h, arr, len(keep), k))

    def set_features_device(self, device_ptr, num_frames, kind="normalized", keep_alive=None):
        """Features already in HBM: device_ptr -> the utterances' rows one after the other, [sum T][feat_dim] floats."""
        ns = (C.c_int * max(len(num_frames), 1))(*[int(n) for n in num_frames])
        self._keep = keep_alive
        _check_code(lib().pk_mi355_features_set_device(self._h, C.c_void_p(device_ptr), ns, len(num_frames), _feature_kind(kind)))

    def score(self, prob_scale=0.1, sync=True):
        _check(lib().pk_mi355_batch_score(self._h, float(prob_scale), 1 if sync else 0))

    def synchronize(self):
        _check(lib().pk_mi355_batch_synchronize(self._h))

    def calibrate(self):
        """f16x3 / f16: calibrate the model's operand exponents on the utterances currently set."""
        _check(lib().pk_mi355_batch_calibrate(self._h))

    def num_utts(self):
        return lib().pk_mi355_batch_num_utts(self._h)

    def num_frames(self, utt):
        return lib().pk_mi355_batch_num_frames(self._h, utt)

    def total_frames(self):
        return lib().pk_mi355_batch_total_frames(self._h)

    def stream(self):
        return lib().pk_mi355_batch_stream(self._h)

    def loglik_device(self, utt):
        return lib().pk_mi355_batch_loglik_device(self._h, utt)

    def fetch(self, utt):
        d = pk_decodable_t()
        _check(lib().pk_mi355_batch_fetch(self._h, utt, C.byref(d)))
        return Decodable._from_struct(d, self._am)

    def fetch_all(self, sync=True):
        """Every utterance's decodable from one transfer into the batch's page-locked arena (views)."""
        n = self.num_utts()
        arr = (pk_decodable_t * max(n, 1))()
        _check(lib().pk_mi355_batch_fetch_all(self._h, arr, n, 1 if sync else 0))
        out = [Decodable._from_struct(arr[u], self._am) for u in range(n)]
        for d in out:
            d._owner = self          # a view must not outlive the batch whose arena it points into
        return out

    def fetch_fbank(self, utt):
        out = np.zeros((self.num_frames(utt), self.base_dim()), dtype=np.float32)     # (the front-end's dimension)
        _check_code(lib().pk_mi355_batch_fetch_fbank(self._h, utt, _fp(out)))
        return out

    def fetch_cmvn(self, utt):
        """What the first layer reads, [T][feat_dim]."""
        out = np.zeros((self.num_frames(utt), self.feat_dim()), dtype=np.float32)
        _check_code(lib().pk_mi355_batch_fetch_cmvn(self._h, utt, _fp(out)))
        return out

    def set_norm(self, spec, global_stats=None):
        """The normalisation between the front-end (or raw features) and the first layer: a NormSpec, or an
        OnlineCmvnSpec with the 2 x (feat_dim + 1) global record it smooths with (None with global_frames = 0).  It
        holds until it is set again.  Anything but "sliding" also lets a FeatureScorer made without statistics take
        kind "raw"."""
        if isinstance(spec, OnlineCmvnSpec):
            g = None if global_stats is None else _global_record(global_stats, self.base_dim())
            _check_code(lib().pk_mi355_norm_set_online_cmvn(self._h, C.byref(spec.struct()), None if g is None else _dp(g)))
            return
        if global_stats is not None:
            raise PkCodeError(-1, "global statistics go with an OnlineCmvnSpec, not with a NormSpec")
        _check_code(lib().pk_mi355_norm_set(self._h, C.byref(spec.struct())))

    def set_speaker_stats(self, stats):
        """Mode "speaker" (required) and online CMVN (optional; a count of 0: no prior for that utterance): one
        2 x (feat_dim + 1) record per utterance of the next score call, which consumes them."""
        n = len(stats)
        a = _stats_records(stats, n, self.base_dim())
        _check_code(lib().pk_mi355_norm_set_speaker_stats(self._h, _dp(a) if n else None, n))

    def norm_stats(self, utt):
        """The 2 x (feat_dim + 1) float64 record the last score call computed for utterance utt in mode "utterance"."""
        out = np.zeros((2, self.base_dim() + 1), np.float64)
        _check_code(lib().pk_mi355_norm_fetch_stats(self._h, utt, _dp(out)))
        return out

    def gather_loglik(self, utt, d_frames, d_trans_ids, n, d_out):
        """Device-side loglikelihood(frame, trans_id) for n pairs (all pointers are device pointers)."""
        _check(lib().pk_mi355_batch_gather_loglik(self._h, utt, C.c_void_p(d_frames), C.c_void_p(d_trans_ids),
                                                  int(n), C.c_void_p(d_out)))

    def enable_timing(self, on=True):
        _check(lib().pk_mi355_batch_enable_timing(self._h, 1 if on else 0))

    def timing(self):
        ms = (C.c_float * 5)()
        n = (C.c_int * 5)()
        _check(lib().pk_mi355_batch_get_timing(self._h, ms, n))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(KINDS)}


class FeatureScorer(BatchScorer):
    """A BatchScorer without a front-end, fed by set_features / set_features_device: any model (any feature
    dimension), capacity in frames.  global_stats (feat_dim sums, then the count: 41 floats for a 40-dim model)
    enables kind "raw"."""

    def __init__(self, am, max_utts, max_total_frames, global_stats=None, deltas=None, transform=None):
        """deltas: a DeltaSpec (pk_mi355_deltas_batch_create without a front-end): kind "raw" then takes [T][base_dim()]
        rows, and global_stats, when given, holds base_dim() sums and the count.
        transform: a TransformSpec (pk_mi355_transform_batch_create without a front-end), alone or behind deltas."""
        self._am = am
        self._keep = None
        self._h = _create_scorer(False, False, am, global_stats, max_utts, max_total_frames, None, deltas, transform)


class OnlineScorer:
    """Live PCM in chunks per slot: every step() scores the frames that became final since the last one (frames
    [a, n - R) of an open slot, the rest after close()), bit for bit what BatchScorer gives on the whole wave.  A slot
    opened with open_features takes [n][40] frames through push_features instead (OnlineFeatureScorer: any dimension)."""

    _has_deltas = False                     # made with deltas=: "raw" slots are then base_dim() wide

    def __init__(self, am, global_stats, max_streams, max_step_samples, frontend=None, deltas=None):
        """frontend: a FrontendSpec of the model's feature dimension (pk_mi355_frontend_stream_create; global_stats: that
        many sums, then the count).  Feature slots then take [n][dim] frames.
        deltas: a DeltaSpec (pk_mi355_deltas_stream_create): the front-end (the default FrontendSpec when none is given),
        the statistics, the normalisation and "raw" slots are then at base_dim() = feat_dim / (order + 1), and a live
        slot looks order * window + R frames ahead."""
        self._am = am
        self._max_streams = int(max_streams)
        self._has_deltas = deltas is not None
        self._h = _create_scorer(True, True, am, global_stats, max_streams, max_step_samples, frontend, deltas)

    @classmethod
    def with_transform(cls, am, global_stats, max_streams, max_step_samples, transform, frontend=None, deltas=None):
        """A scorer with a TransformSpec in front of the splice (pk_mi355_transform_stream_create), behind deltas when a
        DeltaSpec is given: the front-end (the default FrontendSpec when none is given), the statistics, the normalisation
        and "raw" slots are then at base_dim() = in_dim() / (order + 1), and a live slot looks order * window +
        right_context + R frames ahead.  set_slot_transform hands an open slot its own matrix."""
        _check_spec_types(transform, deltas, frontend)
        return cls._made_with_transform(am, max_streams, _create_scorer(True, True, am, global_stats, max_streams, max_step_samples, frontend, deltas, transform))

    @classmethod
    def _made_with_transform(cls, am, max_streams, handle):
        self = cls.__new__(cls)
        self._am = am
        self._max_streams = int(max_streams)
        self._has_deltas = True             # "raw" slots are base_dim() wide, as behind deltas
        self._h = handle
        return self

    def in_dim(self):
        """The width of the rows the transform reads on a scorer made by with_transform; feat_dim() on every other."""
        return _check_code(lib().pk_mi355_stream_in_dim(self._h))

    def set_slot_transform(self, slot, matrix):
        """A scorer made by with_transform: the open slot's own [feat_dim][feat_dim] (linear) or [feat_dim][feat_dim + 1]
        (affine) matrix, before its first transform frame is computed; applied behind the global matrix until the slot is
        opened again.  A slot without one passes its rows on as they are."""
        m = _f32(matrix)
        if m.ndim != 2:
            raise PkCodeError(-1, "a slot's transform has shape %s, expected [rows][cols]" % (m.shape,))
        _check_code(lib().pk_mi355_stream_transform_set_slot(self._h, int(slot), _fp(m), m.shape[0], m.shape[1]))

    def destroy(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def set_norm(self, spec, global_stats=None):
        """The normalisation of the audio and "raw" slots, while no slot is in use: a NormSpec of mode
        "sliding" (the default), "none" or "speaker", or an OnlineCmvnSpec with the 2 x (feat_dim + 1) global record it
        smooths with (None with global_frames = 0).  Every row is then the BatchScorer's under the same spec."""
        if isinstance(spec, OnlineCmvnSpec):
            g = None if global_stats is None else _global_record(global_stats, self.base_dim())
            _check_code(lib().pk_mi355_stream_norm_set_online_cmvn(self._h, C.byref(spec.struct()), None if g is None else _dp(g)))
            return
        if global_stats is not None:
            raise PkCodeError(-1, "global statistics go with an OnlineCmvnSpec, not with a NormSpec")
        _check_code(lib().pk_mi355_stream_norm_set(self._h, C.byref(spec.struct())))

    def set_speaker_stats(self, slot, stats):
        """The speaker's 2 x (feat_dim + 1) record of an open slot, before its first frame is computed: required in mode
        "speaker", optional under online CMVN."""
        a = _stats_records([stats], 1, self.base_dim())
        _check_code(lib().pk_mi355_stream_norm_set_speaker_stats(self._h, int(slot), _dp(a)))

    def norm_stats(self, slot):
        """Mode "speaker" and online CMVN: the 2 x (feat_dim + 1) float64 record of all frames of the slot since it was
        opened -- BatchScorer.norm_stats' bits on the whole input."""
        out = np.zeros((2, self.base_dim() + 1), np.float64)
        _check_code(lib().pk_mi355_stream_norm_fetch_stats(self._h, int(slot), _dp(out)))
        return out

    def open(self, slot, rate=16000, speaker_stats=None):
        """rate: the sample rate of what will be pushed to the slot; converted to 16 kHz on the GPU step by step.
        speaker_stats: set_speaker_stats on the opened slot."""
        if rate == 16000:
            _check_code(lib().pk_mi355_stream_open(self._h, int(slot)))
        else:
            _check_code(lib().pk_mi355_stream_open_rate(self._h, int(slot), int(rate)))
        if speaker_stats is not None:
            self.set_speaker_stats(slot, speaker_stats)

    def rate(self, slot):
        return _check_code(lib().pk_mi355_stream_rate(self._h, int(slot)))

    def open_features(self, slot, kind="normalized", speaker_stats=None):
        """The slot takes features instead of audio: kind "normalized" (ready for the splice) or "raw" (40-dim log-mel
        fbank; the scorer's normalisation -- the sliding-window CMVN unless set_norm chose another -- is applied first,
        carried from step to step).  speaker_stats: set_speaker_stats on the opened slot."""
        _check_code(lib().pk_mi355_stream_open_features(self._h, int(slot), _feature_kind(kind)))
        if speaker_stats is not None:
            self.set_speaker_stats(slot, speaker_stats)

    def push_features(self, slot, frames):
        """[n][feat_dim] frames, n >= 0 ([n][base_dim] for a "raw" slot of a scorer made with deltas=)."""
        f = _feature_frames(frames, self._push_dim(slot) if self._has_deltas else self.feat_dim())
        _check_code(lib().pk_mi355_stream_push_features(self._h, int(slot), _fp(f) if f.size else None, f.shape[0]))

    def feat_dim(self):
        return _check_code(lib().pk_mi355_stream_feat_dim(self._h))

    def base_dim(self):
        """The dimension in front of the deltas -- the front-end's, raw slots', statistics' -- on a scorer made with
        deltas=; feat_dim() on every other."""
        return _check_code(lib().pk_mi355_stream_base_dim(self._h))

    def _push_dim(self, slot):
        """The width of the frames push_features takes for slot: feat_dim(), or base_dim() for a "raw" slot of a scorer
        made with deltas=."""
        if self._has_deltas and lib().pk_mi355_stream_slot_kind(self._h, int(slot)) == FEATURE_KINDS["raw"]:
            return self.base_dim()
        return self.feat_dim()

    def slot_kind(self, slot):
        """None for an audio slot, else "normalized" / "raw": what the slot was last opened as."""
        if not 0 <= int(slot) < self._max_streams:     # (the entry's -1 is both "audio" and PK_MI355_E_INVALID)
            raise PkCodeError(-1, "slot %d out of range [0, %d)" % (int(slot), self._max_streams))
        code = lib().pk_mi355_stream_slot_kind(self._h, int(slot))
        return None if code < 0 else {v: k for k, v in FEATURE_KINDS.items()}[code]

    def push(self, slot, samples):
        """float sample values (as read_wav gives them); an int16 array goes through push_i16."""
        if isinstance(samples, np.ndarray) and samples.dtype == np.int16:
            return self.push_i16(slot, samples)
        x = _f32(samples)
        _check_code(lib().pk_mi355_stream_push(self._h, int(slot), _fp(x) if x.size else None, x.shape[0]))

    def push_i16(self, slot, samples):
        x = np.ascontiguousarray(samples, dtype=np.int16)
        _check_code(lib().pk_mi355_stream_push_i16(self._h, int(slot),
                                                   x.ctypes.data_as(C.POINTER(C.c_int16)) if x.size else None, x.shape[0]))

    def close(self, slot):
        _check_code(lib().pk_mi355_stream_close(self._h, int(slot)))

    def step(self, prob_scale=0.1, sync=True):
        _check_code(lib().pk_mi355_stream_step(self._h, float(prob_scale), 1 if sync else 0))

    def synchronize(self):
        _check_code(lib().pk_mi355_stream_synchronize(self._h))

    def loglik_device(self, slot):
        """(device pointer or None, first frame, count) of the rows the last step scored for slot."""
        first, count = C.c_int(), C.c_int()
        p = lib().pk_mi355_stream_loglik_device(self._h, int(slot), C.byref(first), C.byref(count))
        return p, first.value, count.value

    def fetch(self, slot):
        """(first frame, float32 [count][num_pdfs]) of the rows the last step scored for slot."""
        d, first = pk_decodable_t(), C.c_int()
        _check_code(lib().pk_mi355_stream_fetch(self._h, int(slot), C.byref(d), C.byref(first)))
        if d.log_prob.ncol == 0:
            return first.value, np.zeros((0, self._am.num_pdfs()), dtype=np.float32)
        return first.value, _take_matrix(d.log_prob)


class OnlineFeatureScorer(OnlineScorer):
    """An OnlineScorer without a front-end, fed by open_features / push_features: any model (any feature dimension),
    capacity in frames pushed between two steps.  global_stats (feat_dim sums, then the count: 41 floats for a 40-dim
    model) enables kind "raw".  The audio entries (open, push, push_i16) fail on it."""

    def __init__(self, am, max_streams, max_step_frames, global_stats=None, deltas=None):
        """deltas: a DeltaSpec (pk_mi355_deltas_stream_create without a front-end): "raw" slots then take [n][base_dim()]
        frames, and global_stats, when given, holds base_dim() sums and the count."""
        self._am = am
        self._max_streams = int(max_streams)
        self._has_deltas = deltas is not None
        self._h = _create_scorer(True, False, am, global_stats, max_streams, max_step_frames, None, deltas)

    @classmethod
    def with_transform(cls, am, max_streams, max_step_frames, transform, global_stats=None, deltas=None):
        """OnlineScorer.with_transform without a front-end: "raw" slots take [n][base_dim()] frames, and global_stats, when
        given, holds base_dim() sums and the count."""
        _check_spec_types(transform, deltas)
        return cls._made_with_transform(am, max_streams, _create_scorer(True, False, am, global_stats, max_streams, max_step_frames, None, deltas, transform))


class PkCodeError(PkError):
    """A PkError that carries the library's negative status code."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _check_code(rc):
    if rc < 0:
        raise PkCodeError(rc, lib().pk_mi355_last_error().decode() or "pk_mi355 error %d" % rc)
    return rc


def _ark_view(handle):
    m = pk_matrix_t()
    _check_code(lib().pk_mi355_ark_matrix(handle, C.byref(m)))
    if m.ncol == 0 or m.nrow == 0:
        return np.zeros((m.ncol, m.nrow), np.float32)
    return np.ctypeslib.as_array(m.data, shape=(m.ncol, m.nrow)).copy()


class ArkReader:
    """A Kaldi archive or script file of float matrices (pk_mi355_ark_*): iterable over (key, float32 [T][D]), read entry
    by entry.  spec: "ark:<path>", "scp:<path>" or a bare path (a ".scp" suffix means a script file)."""

    def __init__(self, spec):
        self._h = lib().pk_mi355_ark_open(os.fspath(spec).encode())
        if not self._h:
            raise PkCodeError(lib().pk_mi355_last_error_code(), lib().pk_mi355_last_error().decode(errors="replace"))

    def __iter__(self):
        return self

    def __next__(self):
        if not self._h:
            raise StopIteration
        rc = lib().pk_mi355_ark_next(self._h)
        if rc < 0:
            raise PkCodeError(rc, lib().pk_mi355_last_error().decode(errors="replace"))
        if rc == 0:
            self.close()
            raise StopIteration
        return lib().pk_mi355_ark_key(self._h).decode(errors="surrogateescape"), _ark_view(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_ark_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_kaldi_matrix(rx):
    """One keyless Kaldi matrix object from "path" or "path:offset" -> float32 [rows][cols]."""
    h = lib().pk_mi355_ark_read_object(os.fspath(rx).encode())
    if not h:
        raise PkCodeError(lib().pk_mi355_last_error_code(), lib().pk_mi355_last_error().decode(errors="replace"))
    try:
        return _ark_view(h)
    finally:
        lib().pk_mi355_ark_close(h)


def kaldi_global_stats(rx):
    """A global CMVN statistics file (a 2 x (D + 1) matrix: sums and count, then the sums of squares) -> its row 0 as
    float32 [D + 1], what FeatureScorer / OnlineFeatureScorer take as global_stats."""
    m = read_kaldi_matrix(rx)
    if m.shape[0] != 2 or m.shape[1] < 2:
        raise PkCodeError(-1, "%s holds a %d x %d matrix; global CMVN statistics are 2 x (D + 1)" % (rx, m.shape[0], m.shape[1]))
    return np.ascontiguousarray(m[0])


def _ark_stats(handle, what):
    """The current entry of a reader as a 2 x (D + 1) float64 statistics record (pk_mi355_ark_matrix_f64)."""
    m = pk_matrix_t()
    _check_code(lib().pk_mi355_ark_matrix(handle, C.byref(m)))
    if m.ncol != 2 or m.nrow < 2:
        raise PkCodeError(-1, "%s holds a %d x %d matrix; CMVN statistics are 2 x (D + 1)" % (what, m.ncol, m.nrow))
    out = np.zeros((2, m.nrow), np.float64)
    _check_code(lib().pk_mi355_ark_matrix_f64(handle, _dp(out), out.size))
    return out


def kaldi_cmvn_stats(rx):
    """A CMVN statistics file (compute-cmvn-stats' 2 x (D + 1) matrix) from "path" or "path:offset" -> float64
    [2][D + 1], the doubles as the file holds them: what set_speaker_stats and cmvn_normalize take."""
    h = lib().pk_mi355_ark_read_object(os.fspath(rx).encode())
    if not h:
        raise PkCodeError(lib().pk_mi355_last_error_code(), lib().pk_mi355_last_error().decode(errors="replace"))
    try:
        return _ark_stats(h, rx)
    finally:
        lib().pk_mi355_ark_close(h)


def read_cmvn_stats_archive(spec):
    """An archive or script file of CMVN statistics ("ark:", "scp:" or a path, as ArkReader) -> {key: float64 [2][D + 1]}."""
    out = {}
    with ArkReader(spec) as r:
        while True:
            rc = lib().pk_mi355_ark_next(r._h)
            if rc < 0:
                raise PkCodeError(rc, lib().pk_mi355_last_error().decode(errors="replace"))
            if rc == 0:
                return out
            key = lib().pk_mi355_ark_key(r._h).decode(errors="surrogateescape")
            out[key] = _ark_stats(r._h, "%s key '%s'" % (spec, key))


class Fst:
    """fst.h: the reference's pk::fst_0 graph, read on the host (pk_mi355_fst_read)."""

    def __init__(self, path):
        self._h = lib().pk_mi355_fst_read(os.fspath(path).encode())
        if not self._h:
            msg = lib().pk_mi355_last_error().decode()
            raise PkCodeError(lib().pk_mi355_last_error_code(), msg)

    @property
    def handle(self):
        return self._h

    def num_states(self):
        return lib().pk_mi355_fst_num_states(self._h)

    def num_arcs(self):
        return lib().pk_mi355_fst_num_arcs(self._h)

    def start(self):
        return lib().pk_mi355_fst_start(self._h)

    def arc_range(self, state):
        """Fst::CountArcs (fst.cc:94-110): (first arc, count) of a state."""
        first, count = C.c_int(), C.c_int()
        _check_code(lib().pk_mi355_fst_arc_range(self._h, int(state), C.byref(first), C.byref(count)))
        return first.value, count.value

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_fst_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


Segment = collections.namedtuple("Segment", "word start_frame num_frames graph_cost acoustic_cost")
Result = collections.namedtuple("Result", "text words weight ok loglikelihood_per_frame segments")


def _segments(entry, handle, index):
    n = _check_code(entry(handle, int(index), None, 0))
    out = (pk_mi355_word_t * max(n, 1))()
    _check_code(entry(handle, int(index), out, n))
    return [Segment(s.word, s.start_frame, s.num_frames, s.graph_cost, s.acoustic_cost) for s in out[:n]]


class Decoder:
    """decoder.h: Decoder::Decode + BestPath on the GPU, one workgroup per utterance.  trace_gc: every utterance of
    a call owns trace_capacity // n backtrace records and compacts them as they fill (same results, bit for bit)."""

    def __init__(self, fst, am, max_utts, trace_capacity=0, trace_gc=False):
        self._fst, self._am = fst, am
        self._h = lib().pk_mi355_decoder_create(fst.handle, am.handle, int(max_utts), int(trace_capacity))
        if not self._h:
            msg = lib().pk_mi355_last_error().decode()
            raise PkCodeError(lib().pk_mi355_last_error_code(), msg)
        self._keep = None
        if trace_gc:
            self.set_trace_gc(True)

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_beam(self, beam=16.0, max_active=30000):
        _check_code(lib().pk_mi355_decoder_set_beam(self._h, float(beam), int(max_active)))

    def set_trace_gc(self, on=True):
        """From the next call on: a slice of the backtrace arena per utterance, compacted as it fills."""
        _check_code(lib().pk_mi355_decoder_set_trace_gc(self._h, 1 if on else 0))

    def decode_batch(self, batch, sync=True):
        """Every utterance of a scored BatchScorer, read where it lies in HBM."""
        self._keep = batch
        _check_code(lib().pk_mi355_decoder_decode_batch(self._h, batch._h, 1 if sync else 0))

    def decode(self, logliks, sync=True):
        """Host log-likelihood arrays, each float32 [T][num_pdfs] (or Decodable objects)."""
        arrs, arr = [], (pk_decodable_t * max(len(logliks), 1))()
        for i, x in enumerate(logliks):
            if isinstance(x, Decodable):
                arr[i] = x._d
                arrs.append(x)
                continue
            a = _f32(x)
            if a.ndim != 2:
                raise PkError("log-likelihoods must be [T][num_pdfs]")
            arrs.append(a)
            arr[i].log_prob.ncol, arr[i].log_prob.nrow = a.shape
            arr[i].log_prob.data = _fp(a) if a.size else None
            arr[i].am = self._am.handle
        self._keep = (arrs, arr)
        _check_code(lib().pk_mi355_decoder_decode(self._h, arr, len(logliks), 1 if sync else 0))

    def synchronize(self):
        _check_code(lib().pk_mi355_decoder_synchronize(self._h))

    def result(self, utt):
        """(words in spoken order, weight, ok) -- pk_process's hyp and Hypothesis::weight()."""
        weight, ok = C.c_float(), C.c_int()
        n = _check_code(lib().pk_mi355_decoder_result(self._h, int(utt), None, 0, C.byref(weight), C.byref(ok)))
        words = np.zeros(max(n, 1), np.int32)
        _check_code(lib().pk_mi355_decoder_result(self._h, int(utt), words.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                  C.byref(weight), C.byref(ok)))
        return [int(w) for w in words[:n]], weight.value, ok.value

    def best_path_arcs(self, utt):
        n = _check_code(lib().pk_mi355_decoder_best_path_arcs(self._h, int(utt), None, 0))
        arcs = np.zeros(max(n, 1), np.int32)
        lib().pk_mi355_decoder_best_path_arcs(self._h, int(utt), arcs.ctypes.data_as(C.POINTER(C.c_int32)), n)
        return [int(a) for a in arcs[:n]]

    def active_bound(self, utt):
        return _check_code(lib().pk_mi355_decoder_active_bound(self._h, int(utt)))

    def set_alignment(self, on=True):
        """From the next call on: one more launch writes, per frame, the best path's emitting arc and its acoustic cost."""
        _check_code(lib().pk_mi355_decoder_set_alignment(self._h, 1 if on else 0))

    def alignment(self, utt):
        """(arc ids int32 [frames], transition-ids int32 [frames], acoustic costs float32 [frames]) of the best path;
        empty for an utterance without one.  Raises (PK_MI355_E_STATE) when the call ran with alignment off."""
        n = _check_code(lib().pk_mi355_decoder_alignment(self._h, int(utt), None, None, None, 0))
        arcs, tids, ac = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        if n:
            _check_code(lib().pk_mi355_decoder_alignment(self._h, int(utt), arcs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         tids.ctypes.data_as(C.POINTER(C.c_int32)), _fp(ac), n))
        return arcs, tids, ac

    def word_segments(self, utt):
        """[Segment(word, start_frame, num_frames, graph_cost, acoustic_cost)] of the best path (pk_mi355_word_t)."""
        return _segments(lib().pk_mi355_decoder_word_segments, self._h, utt)

    def trace_stats(self, utt):
        """(peak records, slice records, compactions) of the last call: per utterance with trace gc on; with it off
        the records the whole call wrote, trace_capacity and 0."""
        peak, size, n = C.c_int64(), C.c_int64(), C.c_int()
        _check_code(lib().pk_mi355_decoder_trace_stats(self._h, int(utt), C.byref(peak), C.byref(size), C.byref(n)))
        return peak.value, size.value, n.value


EndpointRule = collections.namedtuple("EndpointRule",
                                      "must_contain_nonsilence min_trailing_silence max_relative_cost min_utterance_length")
EndpointRule.__doc__ = """One endpoint rule, times in seconds (a frame is 10 ms: int(round(s * 100)) frames)."""
Utterance = collections.namedtuple("Utterance", "result first_frame num_frames rule")
Endpoint = collections.namedtuple("Endpoint",
                                  "valid frames trailing_silence_frames num_final rule best_cost final_cost relative_cost")


def _rules_array(rules):
    arr = (pk_mi355_endpoint_rule_t * max(len(rules), 1))()
    for i, r in enumerate(rules):
        r = EndpointRule(*r)
        arr[i].must_contain_nonsilence = 1 if r.must_contain_nonsilence else 0
        arr[i].min_trailing_silence_frames = int(round(r.min_trailing_silence * 100))
        arr[i].max_relative_cost = float(r.max_relative_cost)
        arr[i].min_utterance_frames = int(round(r.min_utterance_length * 100))
    return arr


def endpoint_default_rules():
    """The five usual rules (pk_mi355_endpoint_default_rules), as EndpointRule in seconds."""
    arr = (pk_mi355_endpoint_rule_t * 5)()
    n = lib().pk_mi355_endpoint_default_rules(arr, 5)
    return [EndpointRule(bool(r.must_contain_nonsilence), r.min_trailing_silence_frames / 100.0, r.max_relative_cost,
                         r.min_utterance_frames / 100.0) for r in arr[:n]]


def endpoint_eval(rules, frames, trailing, relative_cost):
    """1 + the index of the first of `rules` (EndpointRule) that fires for an utterance of `frames` frames that ends in
    `trailing` frames of silence and whose best final token costs `relative_cost` more than its best token; 0 if none."""
    rules = list(rules)
    return lib().pk_mi355_endpoint_eval(_rules_array(rules), len(rules), int(frames), int(trailing), float(relative_cost))


class OnlineDecoder:
    """Decoder::Decode frame-synchronous across calls: open(slot), advance(scorer) after every OnlineScorer.step (or
    advance_host with log-likelihood chunks), partial(slot) after every call, result(slot) once the slot is finished."""

    def __init__(self, fst, am, max_streams, trace_capacity=0):
        self._fst, self._am = fst, am
        self._h = lib().pk_mi355_online_decoder_create(fst.handle, am.handle, int(max_streams), int(trace_capacity))
        if not self._h:
            _raise_last()
        self._keep = None

    def destroy(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_online_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def set_beam(self, beam=16.0, max_active=30000):
        _check_code(lib().pk_mi355_online_decoder_set_beam(self._h, float(beam), int(max_active)))

    def open(self, slot):
        _check_code(lib().pk_mi355_online_decoder_open(self._h, int(slot)))

    def advance(self, scorer, sync=True):
        """The rows of the OnlineScorer's last step, slot for slot, read in HBM."""
        self._keep = scorer
        _check_code(lib().pk_mi355_online_decoder_advance(self._h, scorer._h, 1 if sync else 0))

    def advance_host(self, chunks, sync=True):
        """chunks: {slot: (loglik [frames][num_pdfs], final)}."""
        items = sorted(chunks.items())
        n = len(items)
        slots = (C.c_int * max(n, 1))(*[s for s, _ in items])
        fin = (C.c_int * max(n, 1))(*[1 if f else 0 for _, (_, f) in items])
        arr, keep = (pk_decodable_t * max(n, 1))(), []
        for i, (_, (x, _)) in enumerate(items):
            a = _f32(x).reshape(-1, self._am.num_pdfs())
            keep.append(a)
            arr[i].log_prob.ncol, arr[i].log_prob.nrow = a.shape
            arr[i].log_prob.data = _fp(a) if a.size else None
            arr[i].am = self._am.handle
        _check_code(lib().pk_mi355_online_decoder_advance_host(self._h, slots, arr, fin, n, 1 if sync else 0))

    def synchronize(self):
        _check_code(lib().pk_mi355_online_decoder_synchronize(self._h))

    def partial(self, slot):
        """(words in spoken order, cost) of the best token's path after the slot's last call."""
        cost = C.c_float()
        n = _check_code(lib().pk_mi355_online_decoder_partial(self._h, int(slot), None, 0, C.byref(cost)))
        words = np.zeros(max(n, 1), np.int32)
        lib().pk_mi355_online_decoder_partial(self._h, int(slot), words.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(cost))
        return [int(w) for w in words[:n]], cost.value

    def result(self, slot):
        """(words in spoken order, weight, ok) of a finished slot, as Decoder.result."""
        weight, ok = C.c_float(), C.c_int()
        n = _check_code(lib().pk_mi355_online_decoder_result(self._h, int(slot), None, 0, C.byref(weight), C.byref(ok)))
        words = np.zeros(max(n, 1), np.int32)
        lib().pk_mi355_online_decoder_result(self._h, int(slot), words.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                             C.byref(weight), C.byref(ok))
        return [int(w) for w in words[:n]], weight.value, ok.value

    def best_path_arcs(self, slot):
        n = _check_code(lib().pk_mi355_online_decoder_best_path_arcs(self._h, int(slot), None, 0))
        arcs = np.zeros(max(n, 1), np.int32)
        lib().pk_mi355_online_decoder_best_path_arcs(self._h, int(slot), arcs.ctypes.data_as(C.POINTER(C.c_int32)), n)
        return [int(a) for a in arcs[:n]]

    def active_bound(self, slot):
        return _check_code(lib().pk_mi355_online_decoder_active_bound(self._h, int(slot)))

    def word_segments(self, slot):
        """Segments of the slot's current path (partial while live, final after close); acoustic_cost is NaN with
        alignment off."""
        return _segments(lib().pk_mi355_online_decoder_word_segments, self._h, slot)

    def set_alignment(self, on=True):
        """While no slot is open: every trace record also keeps its arc's acoustic cost, so that alignment() and the
        segments' acoustic_cost are the batch decoder's."""
        _check_code(lib().pk_mi355_online_decoder_set_alignment(self._h, 1 if on else 0))

    def alignment(self, slot):
        """(arc ids int32 [frames], transition-ids int32 [frames], acoustic costs float32 [frames]) of the slot's current
        path, as Decoder.alignment.  Raises (PK_MI355_E_STATE) with alignment off."""
        n = _check_code(lib().pk_mi355_online_decoder_alignment(self._h, int(slot), None, None, None, 0))
        arcs, tids, ac = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        if n:
            _check_code(lib().pk_mi355_online_decoder_alignment(self._h, int(slot), arcs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                tids.ctypes.data_as(C.POINTER(C.c_int32)), _fp(ac), n))
        return arcs, tids, ac

    def num_frames(self, slot):
        """The frames the slot has decoded."""
        return _check_code(lib().pk_mi355_online_decoder_num_frames(self._h, int(slot)))

    def set_commit(self, on=True):
        """While no slot is open: at the end of every launch the arcs that all of a slot's tokens share leave the device
        for a host list, so that a stream may be longer than trace_capacity.  No result changes."""
        _check_code(lib().pk_mi355_online_decoder_set_commit(self._h, 1 if on else 0))

    def committed(self, slot):
        """(words, num_arcs, num_frames) of the committed prefix of the slot's path: final whatever audio follows.
        ([], 0, 0) with the commit mode off."""
        arcs, frames = C.c_int(), C.c_int()
        n = _check_code(lib().pk_mi355_online_decoder_committed(self._h, int(slot), None, 0, C.byref(arcs), C.byref(frames)))
        words = np.zeros(max(n, 1), np.int32)
        lib().pk_mi355_online_decoder_committed(self._h, int(slot), words.ctypes.data_as(C.POINTER(C.c_int32)), n, None, None)
        return [int(w) for w in words[:n]], arcs.value, frames.value

    def trace_stats(self, slot):
        """(records in use after the last launch, peak since open, capacity) of the slot's backtrace arena."""
        in_use, peak, cap = C.c_int64(), C.c_int64(), C.c_int64()
        _check_code(lib().pk_mi355_online_decoder_trace_stats(self._h, int(slot), C.byref(in_use), C.byref(peak), C.byref(cap)))
        return in_use.value, peak.value, cap.value

    def set_endpointing(self, silence_pdfs, rules=None):
        """While no slot is open: after every advance a second kernel works out, per slot, the silence that ends the best
        partial path (in frames whose pdf is in silence_pdfs) and the best final token's cost relative to the best
        token's; endpoint(slot) tries `rules` (EndpointRule, default endpoint_default_rules()) on them.  rules=[]: off."""
        rules = endpoint_default_rules() if rules is None else list(rules)
        sil = np.ascontiguousarray(silence_pdfs, dtype=np.int32).ravel()
        _check_code(lib().pk_mi355_online_decoder_set_endpointing(
            self._h, sil.ctypes.data_as(C.POINTER(C.c_int32)) if sil.size else None, sil.shape[0], _rules_array(rules), len(rules)))

    def endpoint(self, slot):
        """The slot's Endpoint record after its last advance; .rule is 1 + the first rule that fires, 0 for none."""
        e = pk_mi355_endpoint_t()
        _check_code(lib().pk_mi355_online_decoder_endpoint(self._h, int(slot), C.byref(e)))
        return Endpoint(e.valid, e.frames, e.trailing_silence_frames, e.num_final, e.rule, e.best_cost, e.final_cost,
                        e.relative_cost)

    def finish(self, slots, sync=True):
        """End the open slots now, with no new frame: result(slot) is then Decoder.decode's on the rows the slot has seen,
        and the slot can be opened again."""
        slots = [int(s) for s in slots]
        arr = (C.c_int * max(len(slots), 1))(*slots)
        _check_code(lib().pk_mi355_online_decoder_finish(self._h, arr, len(slots), 1 if sync else 0))


class SymbolTable:
    """symbol_table.h: the reference's SYM0 word list, read on the host (pk_mi355_symtab_read).  len(), [id] -> str."""

    def __init__(self, path):
        self._owner = None
        self._h = lib().pk_mi355_symtab_read(os.fspath(path).encode())
        if not self._h:
            _raise_last()

    @classmethod
    def _borrowed(cls, handle, owner):
        self = cls.__new__(cls)
        self._h, self._owner = handle, owner
        return self

    def __len__(self):
        return _check_code(lib().pk_mi355_symtab_size(self._h))

    def __getitem__(self, symbol_id):
        s = lib().pk_mi355_symtab_get(self._h, int(symbol_id))
        if s is None:
            raise IndexError(lib().pk_mi355_last_error().decode())
        return s.decode()

    def close(self):
        if getattr(self, "_h", None) and self._owner is None:
            lib().pk_mi355_symtab_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Borrowed:
    """An AcousticModel / BatchScorer / Decoder over a handle the Recognizer owns: every method, nothing to free."""

    @staticmethod
    def of(cls, handle, owner, free="close", **fields):
        """free: the name of cls's method that frees the handle (close, or destroy where close(slot) means a slot)."""
        self = cls.__new__(cls)
        self._h, self._owner, self._keep = handle, owner, None
        for k, v in fields.items():
            setattr(self, k, v)
        setattr(self, free, lambda: None)
        return self


def _load_recognizer(live, config, precision, count, capacity, trace_capacity, frontend=None, deltas=None, transform=None):
    """The handle of a Recognizer (live: of an OnlineRecognizer, which takes no precision): the one choice among the
    library's load entries; the default FrontendSpec when deltas or a transform come without a front-end."""
    L = lib()
    if frontend is None and (deltas is not None or transform is not None):
        frontend = FrontendSpec()
    if transform is not None:
        load, specs = (L.pk_mi355_transform_online_recognizer_load if live else L.pk_mi355_transform_recognizer_load), (frontend, deltas, transform)
    elif deltas is not None:
        load, specs = (L.pk_mi355_deltas_online_recognizer_load if live else L.pk_mi355_deltas_recognizer_load), (frontend, deltas)
    elif frontend is not None:
        load, specs = (L.pk_mi355_frontend_online_recognizer_load if live else L.pk_mi355_frontend_recognizer_load), (frontend,)
    else:
        load, specs = (L.pk_mi355_online_recognizer_load if live else L.pk_mi355_recognizer_load), ()
    h = load(os.fspath(config).encode(), *[_byref(spec) for spec in specs], *([] if live else [AcousticModel.PRECISIONS[precision]]),
             int(count), int(capacity), int(trace_capacity))
    if not h:
        _raise_last()
    return h


class Recognizer:
    """pk_load + pk_process (pocketkaldi.cc:72-248): the model file's graph, symbol table and acoustic model, a batch
    scorer and a decoder with alignment on.  .am / .batch / .decoder / .symbols are the owned objects (beam, trace gc,
    softmax mode and calibration are set through them); process(waves) -> [Result]."""

    def __init__(self, config, precision="f32", max_utts=8, max_total_samples=16000 * 60, trace_capacity=0, frontend=None, deltas=None,
                 transform=None):
        """frontend: a FrontendSpec; the model file is then one of that feature dimension (pk_mi355_frontend_recognizer_load).
        deltas: a DeltaSpec; the model file is then one of (order + 1) x the front-end's dimension whose cmvn_stats are at
        the front-end's (pk_mi355_deltas_recognizer_load; the default FrontendSpec when only deltas is given).
        transform: a TransformSpec, alone or behind deltas; the model file is then one of the transform's out_dim whose
        cmvn_stats are at the front-end's dimension (pk_mi355_transform_recognizer_load)."""
        self._h = _load_recognizer(False, config, precision, max_utts, max_total_samples, trace_capacity, frontend, deltas, transform)
        self.max_utts, self.max_total_samples = int(max_utts), int(max_total_samples)
        L = lib()
        self.am = _Borrowed.of(AcousticModel, L.pk_mi355_recognizer_am(self._h), self)
        self.batch = _Borrowed.of(BatchScorer, L.pk_mi355_recognizer_batch(self._h), self, _am=self.am)
        self.decoder = _Borrowed.of(Decoder, L.pk_mi355_recognizer_decoder(self._h), self, _am=self.am, _fst=None)
        self.symbols = SymbolTable._borrowed(L.pk_mi355_recognizer_symtab(self._h), self)

    def close(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_recognizer_destroy(self._h)
            self._h = None
            for part in (self.am, self.batch, self.decoder, self.symbols):
                part._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _process_call(self, waves, rates=None):
        arr = (pk_vector_t * max(len(waves), 1))()
        for i, w in enumerate(waves):
            arr[i].dim, arr[i].data = w.shape[0], (_fp(w) if w.size else None)
        if rates is None:
            _check_code(lib().pk_mi355_recognizer_process(self._h, arr, len(waves)))
        else:
            _check_code(lib().pk_mi355_recognizer_process_rates(self._h, arr, _rates_array(rates, len(waves)), len(waves)))
        return self._results(len(waves))

    def _results(self, n):
        out = []
        for u in range(n):
            words, weight, ok = self.decoder.result(u)
            out.append(Result(lib().pk_mi355_recognizer_hyp(self._h, u).decode(), words, weight, ok,
                              lib().pk_mi355_recognizer_loglikelihood_per_frame(self._h, u), self.decoder.word_segments(u)))
        return out

    def _speaker_stats(self, speaker_stats, n):
        return None if speaker_stats is None else _stats_records(speaker_stats, n, self.batch.base_dim())

    def _utt_transforms(self, utt_transforms, n):
        if utt_transforms is None:
            return None
        if len(utt_transforms) != n:
            raise PkCodeError(-1, "%d per-utterance transforms for %d utterances" % (len(utt_transforms), n))
        return list(utt_transforms)

    def process_features(self, feats, kind="raw", speaker_stats=None, utt_transforms=None):
        """pk_process from features: one [T][feat_dim] matrix per utterance (kind: as BatchScorer.set_features).  A list
        that does not fit max_utts or the frames the recognizer holds is split into as many calls as it needs; a
        single matrix that cannot fit is refused.  speaker_stats: one record per utterance for a batch whose norm
        (self.batch.set_norm) is in mode "speaker"; they are split with the list.  utt_transforms: one matrix per
        utterance (BatchScorer.set_utt_transforms) on a recognizer made with transform=; split with the list too."""
        code = _feature_kind(kind)
        arr, keep = _feature_matrices(feats, self.batch.base_dim() if code == FEATURE_KINDS["raw"] else self.batch.feat_dim())
        spk = self._speaker_stats(speaker_stats, len(keep))
        mats = self._utt_transforms(utt_transforms, len(keep))
        cap = self.max_total_samples // 160 + self.max_utts       # the frames pk_mi355_batch_create makes room for
        for i, f in enumerate(keep):
            if f.shape[0] > cap:
                raise PkCodeError(-1, "features %d have %d frames, the recognizer holds %d" % (i, f.shape[0], cap))
        out, first, frames = [], 0, 0
        for i in range(len(keep) + 1):
            if i == len(keep) or i - first == self.max_utts or frames + keep[i].shape[0] > cap:
                if i > first:
                    sub = (pk_matrix_t * (i - first))(*[arr[j] for j in range(first, i)])
                    if spk is not None:
                        self.batch.set_speaker_stats(spk[first:i])
                    if mats is not None:
                        self.batch.set_utt_transforms(mats[first:i])
                    _check_code(lib().pk_mi355_recognizer_process_features(self._h, sub, i - first, code))
                    out += self._results(i - first)
                first, frames = i, 0
            if i < len(keep):
                frames += keep[i].shape[0]
        return out

    def process(self, waves, rates=None, speaker_stats=None, utt_transforms=None):
        """pk_process for every wave (float sample values as read_wav gives them; rates: the sample rate of every wave,
        None for 16000 -- the others are converted on the GPU).  A list that does not fit max_utts / max_total_samples
        (counted at 16 kHz) is split into as many calls as it needs; a single wave that cannot fit is refused.
        speaker_stats, utt_transforms: as process_features."""
        waves = [_f32(w).ravel() for w in waves]
        spk = self._speaker_stats(speaker_stats, len(waves))
        mats = self._utt_transforms(utt_transforms, len(waves))
        if rates is None:
            sizes = [w.shape[0] for w in waves]
        else:
            _rates_array(rates, len(waves))
            sizes = [resample_num_output(r, w.shape[0]) for w, r in zip(waves, rates)]
        for i, n in enumerate(sizes):
            if n > self.max_total_samples:
                raise PkCodeError(-1, "wave %d has %d samples, the recognizer holds %d" % (i, n, self.max_total_samples))
        out, call, samples = [], [], 0

        def flush():
            first = len(out)
            if spk is not None:
                self.batch.set_speaker_stats(spk[first:first + len(call)])
            if mats is not None:
                self.batch.set_utt_transforms(mats[first:first + len(call)])
            return self._process_call(call, None if rates is None else rates[first:first + len(call)])
        for w, n in zip(waves, sizes):
            if call and (len(call) == self.max_utts or samples + n > self.max_total_samples):
                out += flush()
                call, samples = [], 0
            call.append(w)
            samples += n
        if call:
            out += flush()
        return out


class OnlineRecognizer:
    """pk_load + a live pk_process: the model file's graph, symbol table and acoustic model, an online scorer and an
    online decoder with alignment on.  .am / .scorer / .decoder / .symbols are the owned objects (beam and softmax mode
    are set through them).  open(slot), push(slot, samples) ..., step() after every round of pushes, partial(slot)
    while live; close(slot), one more step(), then result(slot) -> Result, as Recognizer.process yields.  Open, push,
    close and step through the recognizer, not through .scorer / .decoder: a slot closed behind its back is never
    reported finished."""

    def __init__(self, config, max_streams=8, max_step_samples=16000 * 8, trace_capacity=0, frontend=None, deltas=None):
        """frontend: a FrontendSpec; the model file is then one of that feature dimension
        (pk_mi355_frontend_online_recognizer_load).
        deltas: a DeltaSpec; the model file is then one of (order + 1) x the front-end's dimension whose cmvn_stats are at
        the front-end's (pk_mi355_deltas_online_recognizer_load; the default FrontendSpec when only deltas is given)."""
        self._h = _load_recognizer(True, config, None, max_streams, max_step_samples, trace_capacity, frontend, deltas)
        self._adopt(max_streams, max_step_samples, deltas is not None)

    @classmethod
    def with_transform(cls, config, transform, max_streams=8, max_step_samples=16000 * 8, trace_capacity=0, frontend=None, deltas=None):
        """A recognizer whose scorer is OnlineScorer.with_transform's (pk_mi355_transform_online_recognizer_load): the model
        file is one of the transform's output dimension whose cmvn_stats are at the front-end's (the default FrontendSpec
        when none is given).  A slot's own matrix: self.scorer.set_slot_transform(slot, matrix) once the slot is open; with
        endpointing every utterance cut from that opening uses it."""
        _check_spec_types(transform, deltas, frontend)
        self = cls.__new__(cls)
        self._h = _load_recognizer(True, config, None, max_streams, max_step_samples, trace_capacity, frontend, deltas, transform)
        self._adopt(max_streams, max_step_samples, True)
        return self

    def _adopt(self, max_streams, max_step_samples, base_dim_slots):
        """The owned objects of a loaded recognizer.  base_dim_slots: "raw" slots are the scorer's base_dim() wide."""
        self.max_streams, self.max_step_samples = int(max_streams), int(max_step_samples)
        L = lib()
        self.am = _Borrowed.of(AcousticModel, L.pk_mi355_online_recognizer_am(self._h), self)
        self.scorer = _Borrowed.of(OnlineScorer, L.pk_mi355_online_recognizer_stream(self._h), self, free="destroy", _am=self.am,
                                   _max_streams=int(max_streams), _has_deltas=bool(base_dim_slots))
        self.decoder = _Borrowed.of(OnlineDecoder, L.pk_mi355_online_recognizer_decoder(self._h), self, free="destroy",
                                    _am=self.am, _fst=None)
        self.symbols = SymbolTable._borrowed(L.pk_mi355_online_recognizer_symtab(self._h), self)

    def destroy(self):
        if getattr(self, "_h", None):
            lib().pk_mi355_online_recognizer_destroy(self._h)
            self._h = None
            for part in (self.am, self.scorer, self.decoder, self.symbols):
                part._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def open(self, slot, rate=16000, speaker_stats=None):
        """rate: the sample rate of what will be pushed to the slot.  speaker_stats: the slot's record under the norm set
        on self.scorer (OnlineScorer.set_norm, set_speaker_stats)."""
        if rate == 16000:
            _check_code(lib().pk_mi355_online_recognizer_open(self._h, int(slot)))
        else:
            _check_code(lib().pk_mi355_online_recognizer_open_rate(self._h, int(slot), int(rate)))
        if speaker_stats is not None:
            self.scorer.set_speaker_stats(slot, speaker_stats)

    def push(self, slot, samples):
        """float sample values (as read_wav gives them); an int16 array goes through push_i16."""
        if isinstance(samples, np.ndarray) and samples.dtype == np.int16:
            return self.push_i16(slot, samples)
        x = _f32(samples).ravel()
        _check_code(lib().pk_mi355_online_recognizer_push(self._h, int(slot), _fp(x) if x.size else None, x.shape[0]))

    def push_i16(self, slot, samples):
        x = np.ascontiguousarray(samples, dtype=np.int16).ravel()
        _check_code(lib().pk_mi355_online_recognizer_push_i16(self._h, int(slot),
                                                              x.ctypes.data_as(C.POINTER(C.c_int16)) if x.size else None,
                                                              x.shape[0]))

    def open_features(self, slot, kind="raw", speaker_stats=None):
        """The slot takes 40-dim features instead of audio: "raw" log-mel fbank (what a front-end of the caller's makes)
        or "normalized" (CMVN already applied).  speaker_stats: as open."""
        _check_code(lib().pk_mi355_online_recognizer_open_features(self._h, int(slot), _feature_kind(kind)))
        if speaker_stats is not None:
            self.scorer.set_speaker_stats(slot, speaker_stats)

    def push_features(self, slot, frames):
        """[n][dim] frames, n >= 0 (dim: OnlineScorer.push_features')."""
        f = _feature_frames(frames, self.scorer._push_dim(slot))
        _check_code(lib().pk_mi355_online_recognizer_push_features(self._h, int(slot), _fp(f) if f.size else None, f.shape[0]))

    def close(self, slot):
        """No more samples for slot: the next step() finishes it."""
        _check_code(lib().pk_mi355_online_recognizer_close(self._h, int(slot)))

    def step(self):
        _check_code(lib().pk_mi355_online_recognizer_step(self._h))

    def partial(self, slot):
        """The slot's current hypothesis as text (valid until the next step)."""
        s = lib().pk_mi355_online_recognizer_partial(self._h, int(slot))
        if s is None:
            _raise_last()
        return s.decode()

    def stable(self, slot):
        """The words of partial(slot) that are final now, as text; "" unless decoder.set_commit(True) was called."""
        s = lib().pk_mi355_online_recognizer_stable(self._h, int(slot))
        if s is None:
            _raise_last()
        return s.decode()

    def finished(self, slot):
        return bool(_check_code(lib().pk_mi355_online_recognizer_finished(self._h, int(slot))))

    def result(self, slot):
        """The Result of a finished slot: what Recognizer.process gives on the whole wave."""
        text = lib().pk_mi355_online_recognizer_hyp(self._h, int(slot))
        if text is None:
            _raise_last()
        words, weight, ok = self.decoder.result(slot)
        return Result(text.decode(), words, weight, ok,
                      lib().pk_mi355_online_recognizer_loglikelihood_per_frame(self._h, int(slot)),
                      self.decoder.word_segments(slot))

    def set_endpointing(self, silence_pdfs, rules=None):
        """While no slot is open: OnlineDecoder.set_endpointing on the owned decoder, and every step() ends the utterance
        of each live slot whose rule fired and starts the next one at the scorer's next row; utterances(slot) lists them.
        rules=[]: off."""
        rules = endpoint_default_rules() if rules is None else list(rules)
        sil = np.ascontiguousarray(silence_pdfs, dtype=np.int32).ravel()
        _check_code(lib().pk_mi355_online_recognizer_set_endpointing(
            self._h, sil.ctypes.data_as(C.POINTER(C.c_int32)) if sil.size else None, sil.shape[0], _rules_array(rules), len(rules)))

    def utterances(self, slot):
        """The utterances the slot's stream was cut into since open(slot), in order: Utterance(result, first_frame,
        num_frames, rule).  result is what Decoder.decode gives on the scorer's rows [first_frame, first_frame +
        num_frames), segment frames relative to first_frame; rule is 1 + the rule that ended it, 0 for the last one,
        which is there once the slot is finished."""
        L, slot = lib(), int(slot)
        out = []
        for i in range(_check_code(L.pk_mi355_online_recognizer_num_utterances(self._h, slot))):
            u = pk_mi355_utterance_t()
            _check_code(L.pk_mi355_online_recognizer_utterance(self._h, slot, i, C.byref(u)))
            words = np.zeros(max(u.num_words, 1), np.int32)
            _check_code(L.pk_mi355_online_recognizer_utterance_words(self._h, slot, i, words.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                     u.num_words))
            segs = (pk_mi355_word_t * max(u.num_word_segments, 1))()
            _check_code(L.pk_mi355_online_recognizer_utterance_word_segments(self._h, slot, i, segs, u.num_word_segments))
            result = Result(L.pk_mi355_online_recognizer_utterance_hyp(self._h, slot, i).decode(),
                            [int(w) for w in words[:u.num_words]], u.weight, u.ok, u.loglikelihood_per_frame,
                            [Segment(s.word, s.start_frame, s.num_frames, s.graph_cost, s.acoustic_cost)
                             for s in segs[:u.num_word_segments]])
            out.append(Utterance(result, u.first_frame, u.num_frames, u.rule))
        return out
