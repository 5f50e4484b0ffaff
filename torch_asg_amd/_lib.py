"""ctypes binding of libasg_hip.so (C ABI: include/asg_hip.h).

There is NO fallback: if the HIP library is missing or fails to load, importing this module's
`lib()` raises.  The product path never routes through oracle/ or any CPU implementation.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ASG_HIP_LIB") or os.path.join(_HERE, "csrc", "libasg_hip.so")

ASG_DTYPE_F32, ASG_DTYPE_F64, ASG_DTYPE_BF16 = 0, 1, 2
FLAG_STREAMS, FLAG_SINGLE_LAUNCH, FLAG_ALPHA_SCORES = 1, 2, 8
FLAG_DECODE_GRAPH_STREAMING, FLAG_DECODE_GRAPH_RESIDENT = 16, 32
FLAG_GRAPH_LOSS_KEEP_ALPHA, FLAG_GRAPH_LOSS_STREAMING, FLAG_GRAPH_LOSS_RESIDENT = 64, 128, 256
FLAG_BEAM_LOSS_ACCUMULATE = 512

# every symbol include/asg_hip.h declares
SYMBOLS = ["asg_hip_version", "asg_hip_strerror", "asg_ctx_create", "asg_ctx_destroy", "asg_stream_capture_id", "asg_state_bytes",
           "asg_scratch_bytes", "asg_full_forward", "asg_full_backward", "asg_aligned_forward",
           "asg_aligned_backward", "asg_forward", "asg_forward_only", "asg_backward", "asg_loss_forward",
           "asg_loss_backward", "asg_viterbi_work_bytes", "asg_viterbi", "asg_loss_fused_supported",
           "asg_loss_fused_scratch_bytes", "asg_loss_fused_sync_bytes", "asg_loss_fused_forward",
           "asg_loss_fused_backward", "asg_cluster_timeouts", "asg_reload_env", "asg_loss_forward_only", "asg_loss_forward_only_scores_bytes",
           "asg_viterbi_decode_work_bytes", "asg_viterbi_decode", "asg_viterbi_decode_graph_work_bytes",
           "asg_viterbi_decode_graph", "asg_graph_full_work_bytes", "asg_graph_full_scratch_bytes", "asg_graph_full_forward",
           "asg_graph_full_backward", "asg_graph_target_scores", "asg_beam_decode_graph_work_bytes", "asg_beam_decode_graph",
           "asg_beam_graph_full_work_bytes", "asg_beam_graph_full_scratch_bytes", "asg_beam_graph_full_forward",
           "asg_beam_graph_full_backward", "asg_beam_decode_graph_nbest_work_bytes", "asg_beam_decode_graph_nbest",
           "asg_beam_stream_state_bytes", "asg_beam_stream_reset", "asg_beam_stream_advance", "asg_beam_stream_result",
           "asg_beam_window_state_bytes", "asg_beam_window_reset", "asg_beam_window_advance", "asg_beam_window_result",
           "asg_beam_decode_words_work_bytes", "asg_beam_decode_words", "asg_beam_decode_words_la",
           "asg_beam_word_stream_state_bytes", "asg_beam_word_stream_reset", "asg_beam_word_stream_advance",
           "asg_beam_word_stream_result", "asg_beam_decode_words_nbest_work_bytes", "asg_beam_decode_words_nbest",
           "asg_beam_word_stream_nbest_work_bytes", "asg_beam_word_stream_nbest",
           "asg_beam_word_window_state_bytes", "asg_beam_word_window_reset", "asg_beam_word_window_advance",
           "asg_beam_word_window_result", "asg_beam_word_stream_advance_la", "asg_beam_word_stream_result_la",
           "asg_beam_word_window_advance_la", "asg_beam_word_window_result_la",
           "asg_beam_words_full_work_bytes", "asg_beam_words_full_scratch_bytes", "asg_beam_words_full_forward",
           "asg_beam_words_full_backward", "asg_words_target_scores", "asg_beam_words_full_forward_la",
           "asg_beam_decode_words_nbest_la", "asg_beam_word_stream_nbest_la",
           "asg_beam_words_confidence_work_bytes", "asg_beam_words_confidence", "asg_beam_words_confidence_la",
           "asg_beam_words_nbest_confidence_work_bytes", "asg_beam_words_nbest_confidence", "asg_beam_words_nbest_confidence_la",
           "asg_beam_graph_confidence_work_bytes", "asg_beam_graph_confidence",
           "asg_beam_graph_nbest_confidence_work_bytes", "asg_beam_graph_nbest_confidence",
           "asg_beam_stream_nbest_work_bytes", "asg_beam_stream_nbest", "asg_beam_window_nbest_work_bytes", "asg_beam_window_nbest",
           "asg_beam_word_window_nbest_work_bytes", "asg_beam_word_window_nbest", "asg_beam_word_window_nbest_la",
           "asg_beam_conf_stream_state_bytes", "asg_beam_conf_stream_reset", "asg_beam_conf_stream_advance",
           "asg_beam_conf_stream_result", "asg_beam_conf_stream_nbest_work_bytes", "asg_beam_conf_stream_nbest",
           "asg_beam_conf_stream_confidence",
           "asg_beam_conf_window_state_bytes", "asg_beam_conf_window_reset", "asg_beam_conf_window_advance",
           "asg_beam_conf_window_result", "asg_beam_conf_window_nbest_work_bytes", "asg_beam_conf_window_nbest",
           "asg_beam_conf_window_confidence",
           "asg_beam_word_conf_stream_state_bytes", "asg_beam_word_conf_stream_reset", "asg_beam_word_conf_stream_advance",
           "asg_beam_word_conf_stream_advance_la", "asg_beam_word_conf_stream_result", "asg_beam_word_conf_stream_result_la",
           "asg_beam_word_conf_stream_nbest_work_bytes", "asg_beam_word_conf_stream_nbest", "asg_beam_word_conf_stream_nbest_la",
           "asg_beam_word_conf_stream_confidence", "asg_beam_word_conf_stream_confidence_la"]
ABI_VERSION = 230        # include/asg_hip.h: ASG_HIP_VERSION this package was written against


class AsgProblem(ctypes.Structure):
    _fields_ = [("inputs", ctypes.c_void_p), ("inputs_strides", ctypes.c_int64 * 3),
                ("transition", ctypes.c_void_p), ("transition_strides", ctypes.c_int64 * 2),
                ("targets", ctypes.c_void_p), ("targets_strides", ctypes.c_int64 * 2),
                ("input_lengths", ctypes.c_void_p), ("target_lengths", ctypes.c_void_p),
                ("T", ctypes.c_int64), ("B", ctypes.c_int64), ("N", ctypes.c_int64), ("S", ctypes.c_int64),
                ("dtype", ctypes.c_int32), ("inputs_dtype", ctypes.c_int32)]


class AsgTokenGraph(ctypes.Structure):
    _fields_ = [("Q", ctypes.c_int64), ("E", ctypes.c_int64), ("N", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("label", ctypes.c_void_p), ("state", ctypes.c_void_p), ("row", ctypes.c_void_p), ("src", ctypes.c_void_p),
                ("src_label", ctypes.c_void_p), ("start_w", ctypes.c_void_p), ("final_w", ctypes.c_void_p),
                ("edge_w", ctypes.c_void_p)]


class AsgTokenGraphLoss(ctypes.Structure):
    _fields_ = [("graph", ctypes.POINTER(AsgTokenGraph)), ("S", ctypes.c_int64), ("start", ctypes.c_int32),
                ("reserved", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in ("tgt", "orow", "oedge", "lrow", "lq", "pkey", "pedge",
                                                                               "next", "arcw", "finw")]


class AsgTokenGraphBeam(ctypes.Structure):
    _fields_ = [("graph", ctypes.POINTER(AsgTokenGraph)), ("num_start", ctypes.c_int64), ("max_out", ctypes.c_int32),
                ("reserved", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in ("orow", "oarc", "ow", "start_q")]


class AsgTokenGraphBeamLoss(ctypes.Structure):
    _fields_ = [("beam", ctypes.POINTER(AsgTokenGraphBeam)), ("S", ctypes.c_int64), ("start", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("next", ctypes.c_void_p)]


class AsgWordLM(ctypes.Structure):
    _fields_ = [("H", ctypes.c_int64), ("A", ctypes.c_int64), ("V", ctypes.c_int64), ("S", ctypes.c_int64),
                ("start", ctypes.c_int32), ("separator", ctypes.c_int32), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)] + [
                    (n, ctypes.c_void_p) for n in ("row", "word", "next", "backoff", "lw", "bw", "ew", "word_of_state")]


class AsgWordLookahead(ctypes.Structure):
    _fields_ = [("S", ctypes.c_int64), ("H", ctypes.c_int64), ("A", ctypes.c_int64), ("levels", ctypes.c_int32),
                ("dtype", ctypes.c_int32)] + [(n, ctypes.c_void_p) for n in ("rlo", "rhi", "la_state", "krow", "krank", "tab", "dense0")]


_LIB = None


def lib():
    """Load libasg_hip.so once; fail loudly if it is not there."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "torch_asg_amd: %s not found. Build it with `python torch_asg_amd/csrc/build.py` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    pp = ctypes.POINTER(AsgProblem)
    L.asg_hip_version.restype = ci
    if int(L.asg_hip_version()) != ABI_VERSION:
        raise RuntimeError("torch_asg_amd: %s reports ABI version %d, this package needs %d -- rebuild it with "
                           "`python torch_asg_amd/csrc/build.py`" % (LIB_PATH, int(L.asg_hip_version()), ABI_VERSION))
    L.asg_cluster_timeouts.restype = ctypes.c_uint
    L.asg_cluster_timeouts.argtypes = []
    L.asg_reload_env.restype = None
    L.asg_reload_env.argtypes = []
    L.asg_hip_strerror.restype = ctypes.c_char_p
    L.asg_hip_strerror.argtypes = [ci]
    L.asg_ctx_create.argtypes = [ctypes.POINTER(vp)]
    L.asg_ctx_destroy.argtypes = [vp]
    L.asg_stream_capture_id.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.asg_state_bytes.restype = sz
    L.asg_state_bytes.argtypes = [pp]
    L.asg_scratch_bytes.restype = sz
    L.asg_scratch_bytes.argtypes = [pp]
    L.asg_full_forward.argtypes = [pp, vp, sz, vp, ci, vp]
    L.asg_aligned_forward.argtypes = [pp, vp, sz, vp, ci, vp]
    L.asg_full_backward.argtypes = [pp, vp, sz, vp, vp, sz, vp, vp, vp]
    L.asg_aligned_backward.argtypes = [pp, vp, sz, vp, vp, sz, vp, vp, vp]
    L.asg_forward.argtypes = [vp, pp, vp, sz, vp, vp, ci, vp]
    L.asg_forward_only.argtypes = [vp, pp, vp, sz, vp, vp, ci, vp]
    L.asg_backward.argtypes = [vp, pp, vp, sz, vp, vp, vp, sz, vp, vp, ci, vp]
    L.asg_loss_forward.argtypes = [vp, pp, vp, sz, ci, vp, vp, ci, vp]
    L.asg_loss_backward.argtypes = [vp, pp, vp, sz, ci, vp, vp, sz, vp, vp, ci, vp]
    L.asg_loss_forward_only_scores_bytes.restype = sz
    L.asg_loss_forward_only_scores_bytes.argtypes = [pp]
    L.asg_loss_forward_only.argtypes = [vp, pp, vp, sz, ci, vp, vp, sz, ci, vp]
    L.asg_viterbi_work_bytes.restype = sz
    L.asg_viterbi_work_bytes.argtypes = [pp]
    L.asg_viterbi.argtypes = [vp, pp, vp, sz, vp, vp, ci, vp]
    L.asg_viterbi_decode_work_bytes.restype = sz
    L.asg_viterbi_decode_work_bytes.argtypes = [pp]
    L.asg_viterbi_decode.argtypes = [vp, pp, vp, sz, vp, vp, vp, vp, ci, vp]
    gp = ctypes.POINTER(AsgTokenGraph)
    L.asg_viterbi_decode_graph_work_bytes.restype = sz
    L.asg_viterbi_decode_graph_work_bytes.argtypes = [pp, gp]
    L.asg_viterbi_decode_graph.argtypes = [vp, pp, gp, vp, sz, vp, vp, vp, vp, vp, ci, vp]
    bp = ctypes.POINTER(AsgTokenGraphBeam)
    L.asg_beam_decode_graph_work_bytes.restype = sz
    L.asg_beam_decode_graph_work_bytes.argtypes = [pp, bp, ci]
    L.asg_beam_decode_graph.argtypes = [vp, pp, bp, ci, ctypes.c_double, vp, sz, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_decode_graph_nbest_work_bytes.restype = sz
    L.asg_beam_decode_graph_nbest_work_bytes.argtypes = [pp, bp, ci, ci]
    L.asg_beam_decode_graph_nbest.argtypes = [vp, pp, bp, ci, ctypes.c_double, ci, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    i64 = ctypes.c_int64
    L.asg_beam_stream_state_bytes.restype = sz
    L.asg_beam_stream_state_bytes.argtypes = [bp, i64, ci, ci, i64]
    L.asg_beam_stream_reset.argtypes = [vp, bp, i64, ci, i64, vp, sz, vp, ci, vp]
    L.asg_beam_stream_advance.argtypes = [vp, pp, bp, ci, ctypes.c_double, i64, vp, sz, ci, vp]
    L.asg_beam_stream_result.argtypes = [vp, bp, i64, ci, i64, vp, sz, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_window_state_bytes.restype = sz
    L.asg_beam_window_state_bytes.argtypes = [bp, i64, ci, ci, i64, i64]
    L.asg_beam_window_reset.argtypes = [vp, bp, i64, ci, i64, i64, vp, sz, vp, ci, vp]
    L.asg_beam_window_advance.argtypes = [vp, pp, bp, ci, ctypes.c_double, i64, i64, vp, sz, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_window_result.argtypes = [vp, bp, i64, ci, i64, i64, vp, sz, ci, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_stream_nbest_work_bytes.restype = sz
    L.asg_beam_stream_nbest_work_bytes.argtypes = [bp, i64, ci, ci, i64, ci]
    L.asg_beam_stream_nbest.argtypes = [vp, bp, i64, ci, i64, vp, sz, ci, ci, vp, sz] + [vp] * 9 + [ci, vp]
    L.asg_beam_window_nbest_work_bytes.restype = sz
    L.asg_beam_window_nbest_work_bytes.argtypes = [bp, i64, ci, ci, i64, i64, ci]
    L.asg_beam_window_nbest.argtypes = [vp, bp, i64, ci, i64, i64, vp, sz, ci, ci, vp, sz] + [vp] * 9 + [ci, vp]
    wp = ctypes.POINTER(AsgWordLM)
    L.asg_beam_decode_words_work_bytes.restype = sz
    L.asg_beam_decode_words_work_bytes.argtypes = [pp, bp, wp, ci]
    L.asg_beam_decode_words.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_decode_words_la.argtypes = [vp, pp, bp, wp, ctypes.POINTER(AsgWordLookahead), ci, ctypes.c_double, vp, sz, vp, vp, vp,
                                           vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_word_stream_state_bytes.restype = sz
    L.asg_beam_word_stream_state_bytes.argtypes = [bp, wp, i64, ci, ci, i64]
    L.asg_beam_word_stream_reset.argtypes = [vp, bp, wp, i64, ci, i64, vp, sz, vp, ci, vp]
    L.asg_beam_word_stream_advance.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, i64, vp, sz, ci, vp]
    L.asg_beam_word_stream_result.argtypes = [vp, bp, wp, i64, ci, i64, vp, sz, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_decode_words_nbest_work_bytes.restype = sz
    L.asg_beam_decode_words_nbest_work_bytes.argtypes = [pp, bp, wp, ci, ci]
    L.asg_beam_decode_words_nbest.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, ci, vp, sz] + [vp] * 12 + [ci, vp]
    L.asg_beam_word_stream_nbest_work_bytes.restype = sz
    L.asg_beam_word_stream_nbest_work_bytes.argtypes = [bp, wp, i64, ci, ci, i64, ci]
    L.asg_beam_word_stream_nbest.argtypes = [vp, bp, wp, i64, ci, i64, vp, sz, ci, ci, vp, sz] + [vp] * 13 + [ci, vp]
    L.asg_beam_word_window_state_bytes.restype = sz
    L.asg_beam_word_window_state_bytes.argtypes = [bp, wp, i64, ci, ci, i64, i64]
    L.asg_beam_word_window_reset.argtypes = [vp, bp, wp, i64, ci, i64, i64, vp, sz, vp, ci, vp]
    L.asg_beam_word_window_advance.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, i64, i64, vp, sz] + [vp] * 8 + [ci, vp]
    L.asg_beam_word_window_result.argtypes = [vp, bp, wp, i64, ci, i64, i64, vp, sz, ci] + [vp] * 11 + [ci, vp]
    L.asg_beam_word_window_nbest_work_bytes.restype = sz
    L.asg_beam_word_window_nbest_work_bytes.argtypes = [bp, wp, i64, ci, ci, i64, i64, ci]
    L.asg_beam_word_window_nbest.argtypes = [vp, bp, wp, i64, ci, i64, i64, vp, sz, ci, ci, vp, sz] + [vp] * 12 + [ci, vp]
    # the lattice-keeping word stream: the plain word stream's calls over the wider state, and _confidence
    L.asg_beam_word_conf_stream_state_bytes.restype = sz
    L.asg_beam_word_conf_stream_state_bytes.argtypes = L.asg_beam_word_stream_state_bytes.argtypes
    L.asg_beam_word_conf_stream_reset.argtypes = L.asg_beam_word_stream_reset.argtypes
    L.asg_beam_word_conf_stream_advance.argtypes = L.asg_beam_word_stream_advance.argtypes
    L.asg_beam_word_conf_stream_result.argtypes = L.asg_beam_word_stream_result.argtypes
    L.asg_beam_word_conf_stream_nbest_work_bytes.restype = sz
    L.asg_beam_word_conf_stream_nbest_work_bytes.argtypes = L.asg_beam_word_stream_nbest_work_bytes.argtypes
    L.asg_beam_word_conf_stream_nbest.argtypes = L.asg_beam_word_stream_nbest.argtypes
    L.asg_beam_word_conf_stream_confidence.argtypes = [vp, bp, wp, i64, ci, i64, vp, sz, vp, ctypes.POINTER(i64), ci,
                                                       ci] + [vp] * 13 + [ci, vp]
    for name in ("asg_beam_word_stream_advance", "asg_beam_word_stream_result", "asg_beam_word_window_advance",
                 "asg_beam_word_window_result", "asg_beam_decode_words_nbest",
                 "asg_beam_word_stream_nbest", "asg_beam_word_window_nbest", "asg_beam_word_conf_stream_advance",
                 "asg_beam_word_conf_stream_result", "asg_beam_word_conf_stream_nbest",
                 "asg_beam_word_conf_stream_confidence"):                          # the plain call with the look-ahead behind the LM
        plain = getattr(L, name).argtypes
        at = plain.index(wp) + 1
        getattr(L, name + "_la").argtypes = plain[:at] + [ctypes.POINTER(AsgWordLookahead)] + plain[at:]
    blp = ctypes.POINTER(AsgTokenGraphBeamLoss)
    L.asg_beam_graph_full_work_bytes.restype = sz
    L.asg_beam_graph_full_work_bytes.argtypes = [pp, blp, ci, ci]
    L.asg_beam_graph_full_scratch_bytes.restype = sz
    L.asg_beam_graph_full_scratch_bytes.argtypes = [pp, blp, ci]
    L.asg_beam_graph_full_forward.argtypes = [vp, pp, blp, ci, ctypes.c_double, vp, sz, vp, ci, vp]
    L.asg_beam_graph_full_backward.argtypes = [vp, pp, blp, ci, vp, sz, vp, vp, vp, vp, vp, sz, ci, vp]
    L.asg_beam_graph_confidence_work_bytes.restype = sz
    L.asg_beam_graph_confidence_work_bytes.argtypes = [pp, blp, ci]
    L.asg_beam_graph_confidence.argtypes = [vp, pp, blp, ci, ctypes.c_double, ci, vp, sz] + [vp] * 8 + [ci, vp]
    L.asg_beam_conf_stream_state_bytes.restype = sz
    L.asg_beam_conf_stream_state_bytes.argtypes = [blp, i64, ci, ci, i64]
    L.asg_beam_conf_stream_reset.argtypes = [vp, blp, i64, ci, i64, vp, sz, vp, ci, vp]
    L.asg_beam_conf_stream_advance.argtypes = [vp, pp, blp, ci, ctypes.c_double, i64, vp, sz, ci, vp]
    L.asg_beam_conf_stream_result.argtypes = [vp, blp, i64, ci, i64, vp, sz, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    L.asg_beam_conf_stream_nbest_work_bytes.restype = sz
    L.asg_beam_conf_stream_nbest_work_bytes.argtypes = [blp, i64, ci, ci, i64, ci]
    L.asg_beam_conf_stream_nbest.argtypes = [vp, blp, i64, ci, i64, vp, sz, ci, ci, vp, sz] + [vp] * 9 + [ci, vp]
    L.asg_beam_conf_stream_confidence.argtypes = [vp, blp, i64, ci, i64, vp, sz, vp, ctypes.POINTER(i64), ci, ci] + [vp] * 10 + [ci, vp]
    shape = [i64, i64, ci, i64]                                                    # W, P, frame_tolerance, max_chunk
    L.asg_beam_conf_window_state_bytes.restype = sz
    L.asg_beam_conf_window_state_bytes.argtypes = [blp, i64, ci, ci] + shape
    L.asg_beam_conf_window_reset.argtypes = [vp, blp, i64, ci] + shape + [vp, sz, vp, ci, vp]
    L.asg_beam_conf_window_advance.argtypes = [vp, pp, blp, ci, ctypes.c_double] + shape + [vp, sz] + [vp] * 7 + [ci, vp]
    L.asg_beam_conf_window_result.argtypes = [vp, blp, i64, ci] + shape + [vp, sz, ci] + [vp] * 8 + [ci, vp]
    L.asg_beam_conf_window_nbest_work_bytes.restype = sz
    L.asg_beam_conf_window_nbest_work_bytes.argtypes = [blp, i64, ci, ci] + shape + [ci]
    L.asg_beam_conf_window_nbest.argtypes = [vp, blp, i64, ci] + shape + [vp, sz, ci, ci, vp, sz] + [vp] * 9 + [ci, vp]
    L.asg_beam_conf_window_confidence.argtypes = ([vp, blp, i64, ci] + shape + [vp, sz, vp, ctypes.POINTER(i64), ci] + [vp] * 11 +
                                                  [ci, vp])
    L.asg_beam_graph_nbest_confidence_work_bytes.restype = sz
    L.asg_beam_graph_nbest_confidence_work_bytes.argtypes = [pp, blp, ci, ci]
    L.asg_beam_graph_nbest_confidence.argtypes = [vp, pp, blp, ci, ctypes.c_double, ci, ci, vp, sz] + [vp] * 11 + [ci, vp]
    L.asg_beam_words_full_work_bytes.restype = sz
    L.asg_beam_words_full_work_bytes.argtypes = [pp, bp, wp, ci, ci]
    L.asg_beam_words_full_scratch_bytes.restype = sz
    L.asg_beam_words_full_scratch_bytes.argtypes = [pp, bp, wp, ci]
    L.asg_beam_words_full_forward.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, vp, sz, vp, ci, vp]
    L.asg_beam_words_full_forward_la.argtypes = [vp, pp, bp, wp, ctypes.POINTER(AsgWordLookahead), ci, ctypes.c_double, vp, sz, vp,
                                                 ci, vp]
    L.asg_beam_words_full_backward.argtypes = [vp, pp, bp, wp, ci, vp, sz, vp, vp, vp, vp, vp, sz, ci, vp]
    L.asg_words_target_scores.argtypes = [vp, pp, bp, wp, vp, vp]
    L.asg_beam_words_confidence_work_bytes.restype = sz
    L.asg_beam_words_confidence_work_bytes.argtypes = [pp, bp, wp, ci]
    L.asg_beam_words_confidence.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, ci, vp, sz] + [vp] * 11 + [ci, vp]
    L.asg_beam_words_confidence_la.argtypes = [vp, pp, bp, wp, ctypes.POINTER(AsgWordLookahead), ci, ctypes.c_double, ci, vp,
                                               sz] + [vp] * 11 + [ci, vp]
    L.asg_beam_words_nbest_confidence_work_bytes.restype = sz
    L.asg_beam_words_nbest_confidence_work_bytes.argtypes = [pp, bp, wp, ci, ci]
    L.asg_beam_words_nbest_confidence.argtypes = [vp, pp, bp, wp, ci, ctypes.c_double, ci, ci, vp, sz] + [vp] * 15 + [ci, vp]
    L.asg_beam_words_nbest_confidence_la.argtypes = [vp, pp, bp, wp, ctypes.POINTER(AsgWordLookahead), ci, ctypes.c_double, ci,
                                                     ci, vp, sz] + [vp] * 15 + [ci, vp]
    lp = ctypes.POINTER(AsgTokenGraphLoss)
    L.asg_graph_full_work_bytes.restype = sz
    L.asg_graph_full_work_bytes.argtypes = [pp, lp, ci]
    L.asg_graph_full_scratch_bytes.restype = sz
    L.asg_graph_full_scratch_bytes.argtypes = [pp, lp]
    L.asg_graph_full_forward.argtypes = [vp, pp, lp, vp, sz, vp, ci, vp]
    L.asg_graph_full_backward.argtypes = [vp, pp, lp, vp, sz, vp, vp, vp, vp, vp, sz, ci, vp]
    L.asg_graph_target_scores.argtypes = [vp, pp, lp, vp, vp]
    L.asg_loss_fused_supported.argtypes = [pp]
    L.asg_loss_fused_scratch_bytes.restype = sz
    L.asg_loss_fused_scratch_bytes.argtypes = [pp]
    L.asg_loss_fused_sync_bytes.restype = sz
    L.asg_loss_fused_sync_bytes.argtypes = [pp]
    L.asg_loss_fused_forward.argtypes = [pp, vp, sz, ci, vp, vp, vp, sz, vp, vp, ci, vp]
    L.asg_loss_fused_backward.argtypes = [pp, vp, sz, ci, vp, vp, sz, vp, vp, ci, vp]
    for name in SYMBOLS:
        getattr(L, name)
    _LIB = L
    return L


def check(status, what):
    if status != 0:
        msg = lib().asg_hip_strerror(int(status)).decode()
        raise RuntimeError("torch_asg_amd: %s failed: %s (status %d)" % (what, msg, status))


# what the C++ fast path of ASGLossFunction (csrc/binding.cpp) calls, in the order its init() expects
BINDING_SYMBOLS = ["asg_state_bytes", "asg_scratch_bytes", "asg_loss_fused_scratch_bytes", "asg_loss_fused_sync_bytes",
                   "asg_loss_fused_supported", "asg_stream_capture_id", "asg_hip_strerror", "asg_loss_forward",
                   "asg_loss_backward", "asg_loss_fused_forward", "asg_loss_fused_backward", "asg_cluster_timeouts",
                   "asg_loss_forward_only"]
BINDING_PATH = os.path.join(_HERE, "_binding.so")


def binding(backend):
    """The C++ host fast path (torch_asg_amd/_binding.so), one object per backend, initialised with the entry points of the library that
    `lib()` loaded (so ASG_HIP_LIB variants are honoured), or None when it has not been built or ASG_NO_BINDING=1 --
    the Python statements in asg.py then do the same work, only slower (host time)."""
    if os.environ.get("ASG_NO_BINDING", "0") not in ("", "0") or not os.path.exists(BINDING_PATH):
        return None
    L = lib()
    try:
        # a stale or ABI-mismatched _binding.so (torch upgraded, other C++ ABI, missing libtorch_hip) must not take the package
        # down: the Python statements do the same work
        from . import _binding
        return _binding.Fast([ctypes.cast(getattr(L, n), ctypes.c_void_p).value for n in BINDING_SYMBOLS], backend)
    except (ImportError, OSError, RuntimeError, AttributeError) as e:
        import warnings
        warnings.warn("torch_asg_amd: the C++ host fast path (_binding.so) is unusable (%s: %s); using the Python path -- rebuild "
                      "with `python torch_asg_amd/csrc/build.py --binding`" % (type(e).__name__, e))
        return None
