"""ASGLoss / autograd surface for the MI355X-native ASG hot path.

Mirrors the reference's Python interface (/root/reference/torch_asg/asg.py) so it is a drop-in:

    ASGLoss(num_labels, reduction='mean', forward_only=False, gpu_no_stream_impl=False)   asg.py:100-107
    .forward(inputs[T,B,N], targets[B,S], input_lengths=None, target_lengths=None)        asg.py:109-142
    .transition : nn.Parameter[N,N], zero-initialised, transition[i,j] = score of j -> i  asg.py:105
    FCC, FAC, ASGGPUFast, ASGGPUFastForwardOnly autograd Functions                         asg.py:7-97
    (same argument orders, same (grad_transition, grad_inputs, None...) return conventions)

All numerical work happens in hand-written HIP kernels behind the C ABI of include/asg_hip.h.
CPU tensors are rejected: this package has no CPU fallback by design.
"""
import collections
import ctypes
import os
import threading

import torch
import torch.autograd
import torch.nn as nn

from . import _lib


class _NullGuard:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL_GUARD = _NullGuard()

# torch.cuda.current_stream() builds a Stream object (4 us per call on the training path); the raw handle is a C call away
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_is_capturing = getattr(torch._C, "_cuda_isCurrentStreamCapturing", None)


def _current_stream_handle(idx):
    if _raw_stream is not None:
        return int(_raw_stream(idx))
    return int(torch.cuda.current_stream(idx).cuda_stream)


def _on_device(t, dev, contiguous):
    if t is None:
        return None
    if t.device != dev:
        t = t.to(dev, non_blocking=True)
    if contiguous and not t.is_contiguous():
        t = t.contiguous()
    return t


class HipBackend:
    """Thin tensor <-> C-ABI adapter.  Every method launches HIP kernels on the current stream."""

    def __init__(self):
        self._ctx = {}
        self._sizes = {}
        self._cus = {}
        self._lock = threading.Lock()
        self._tickets = {}
        self._pools = {}
        self._pool_keep = []
        self._retired = []            # contexts evicted from _ctx: destroyed in release(), never while a call may still hold them
        self._faults = 0              # resident-slice launches that timed out, as last seen (asg_cluster_timeouts)
        self.binding = _lib.binding(self)        # C++ fast path of ASGLossFunction, or None (csrc/binding.cpp)

    def check_faults(self):
        """How many resident-slice forward launches (256 < N <= 2048 in fp32, <= 1024 in fp64) of this process have run out of
        their bounded waits since the last look; a RuntimeWarning says so once per look.  Nothing is wrong with the results: the
        call that contained such a launch repaired itself in stream (fwd_repair_kernel redoes the recursion without
        co-residency, tens of milliseconds), and the library takes the launch-per-frame kernels from then on (2-3x slower than
        the resident route) -- the warning is about speed.  Host-pinned counter, no synchronisation."""
        n = int(_lib.lib().asg_cluster_timeouts())
        new = n - self._faults
        if new:
            self._faults = n
            import warnings
            warnings.warn("torch_asg_amd: %d resident-slice forward launch(es) timed out (part of the grid never became resident: "
                          "another process on the device, a CU-masked stream?).  The affected call(s) were repaired in stream and "
                          "are exact; the library takes the launch-per-frame kernels from now on (slower)." % new, RuntimeWarning)
        return new

    def _cu_count(self, idx):
        cus = self._cus.get(idx)
        if cus is None:
            cus = self._cus[idx] = int(torch.cuda.get_device_properties(idx).multi_processor_count)
        return cus

    def _bytes(self, p):
        """(state_bytes, scratch_bytes) of a problem shape, cached per (dtype, T, B, N, S)."""
        key = (p.dtype, p.T, p.B, p.N, p.S)
        v = self._sizes.get(key)
        if v is None:
            L = _lib.lib()
            v = (L.asg_state_bytes(ctypes.byref(p)), L.asg_scratch_bytes(ctypes.byref(p)))
            self._sizes[key] = v
        return v

    # -- helpers ---------------------------------------------------------------------------
    @staticmethod
    def _check(inputs, transition, targets, input_lengths, target_lengths):
        if not inputs.is_cuda:
            raise RuntimeError("torch_asg_amd: inputs must live on a ROCm device (got %s); "
                               "there is no CPU implementation in this package" % inputs.device)
        bf16 = inputs.dtype == torch.bfloat16 and transition.dtype == torch.float32     # bf16 in, fp32 accumulate
        if inputs.dtype not in (torch.float32, torch.float64) and not bf16:
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % inputs.dtype)
        if inputs.dim() != 3:
            raise RuntimeError("torch_asg_amd: inputs must be [T,B,N]")
        if (transition.dtype != inputs.dtype and not bf16) or transition.device != inputs.device:
            raise RuntimeError("torch_asg_amd: transition must have the dtype/device of inputs")
        N = inputs.shape[2]
        if tuple(transition.shape) != (N, N):
            raise RuntimeError("torch_asg_amd: transition must be [%d,%d]" % (N, N))
        for name, t in (("targets", targets), ("input_lengths", input_lengths), ("target_lengths", target_lengths)):
            if t is not None and t.dtype != torch.int64:
                # the reference asserts kLong (utils.cpp:28,46) and uses accessor<int64_t>
                raise RuntimeError("torch_asg_amd: expected scalar type Long but found %s for %s" % (t.dtype, name))
        B = inputs.shape[1]
        if targets is not None and (targets.dim() != 2 or targets.shape[0] != B or targets.shape[1] < 1):
            # the kernels index targets[b][s] for every b < B: a short or mis-shaped tensor would be read out of bounds
            raise RuntimeError("torch_asg_amd: targets must be [B=%d, S>=1] but got %s" % (B, tuple(targets.shape)))

    @staticmethod
    def device_args(dev, targets, input_lengths, target_lengths):
        """targets / lengths as the kernels read them: on `dev`, lengths contiguous."""
        return _on_device(targets, dev, False), _on_device(input_lengths, dev, True), _on_device(target_lengths, dev, True)

    @staticmethod
    def _problem(inputs, transition, targets, input_lengths, target_lengths):
        T, B, N = inputs.shape
        dev = inputs.device
        p = _lib.AsgProblem()
        p.inputs = inputs.data_ptr()
        st = inputs.stride()
        ps = p.inputs_strides
        ps[0], ps[1], ps[2] = st[0], st[1], st[2]
        p.transition = transition.data_ptr()
        st = transition.stride()
        ps = p.transition_strides
        ps[0], ps[1] = st[0], st[1]
        keep = [inputs, transition]
        if targets is not None:
            if targets.device != dev:
                targets = targets.to(dev, non_blocking=True)
            p.targets = targets.data_ptr()
            st = targets.stride()
            ps = p.targets_strides
            ps[0], ps[1] = st[0], st[1]
            p.S = targets.shape[1]
            keep.append(targets)
        else:
            p.targets = None
            p.S = 1
        for name, t in (("input_lengths", input_lengths), ("target_lengths", target_lengths)):
            if t is not None:
                if t.device != dev:
                    t = t.to(dev, non_blocking=True)
                if not t.is_contiguous():
                    t = t.contiguous()
                if t.shape != (B,):
                    raise RuntimeError("torch_asg_amd: %s must have shape [%d]" % (name, B))
                keep.append(t)
                setattr(p, name, t.data_ptr())
            else:
                setattr(p, name, None)
        p.T, p.B, p.N = T, B, N
        if inputs.dtype == torch.bfloat16:
            p.dtype, p.inputs_dtype = _lib.ASG_DTYPE_F32, _lib.ASG_DTYPE_BF16
        else:
            p.dtype = _lib.ASG_DTYPE_F32 if inputs.dtype == torch.float32 else _lib.ASG_DTYPE_F64
        return p, keep

    MAX_CONTEXTS = 64
    MAX_RETIRED = 64          # evicted contexts kept alive; the oldest beyond this is destroyed (it left the cache >= 64 evictions ago)

    def _context(self, device):
        """Side stream + fork/join events of the 'streams' launch mode, ONE SET PER CALLING STREAM: calls issued on
        different streams (other threads, other modules, a capture in progress) never share an event pair."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, _current_stream_handle(idx))
        h = self._ctx.get(key)
        if h is None:
            with self._lock:
                h = self._ctx.get(key)
                if h is None:
                    h = ctypes.c_void_p()
                    if len(self._ctx) >= self.MAX_CONTEXTS:
                        # streams come and go in long runs: forget the handle that was created first.  It is NOT destroyed here --
                        # another thread may be inside a call that holds it (ctypes releases the GIL) -- but moved to a retire
                        # list that release() empties; a context is a stream and two events
                        old = next(iter(self._ctx))
                        self._retired.append(self._ctx.pop(old))
                        # ... and the list is bounded: a handle that was evicted MAX_RETIRED evictions ago (each eviction means
                        # MAX_CONTEXTS newer calling streams exist) is not inside a call any more
                        while len(self._retired) > self.MAX_RETIRED:
                            _lib.lib().asg_ctx_destroy(self._retired.pop(0))
                        if self.binding is not None:
                            self.binding.reset()
                    with torch.cuda.device(idx):
                        _lib.check(_lib.lib().asg_ctx_create(ctypes.byref(h)), "asg_ctx_create")
                    self._ctx[key] = h
        return h

    @staticmethod
    def _guard(device):
        """Device guard that costs nothing when the tensor's device is already current."""
        idx = device.index
        if idx is None or idx == torch.cuda.current_device():
            return _NULL_GUARD
        return torch.cuda.device(idx)

    @staticmethod
    def _stream(device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return ctypes.c_void_p(_current_stream_handle(idx))

    def _state_bytes(self, p):
        """Size of the state buffer of problem p, a whole number of 256-byte units (a tail behind it stays 256-byte aligned)."""
        return (max(int(self._bytes(p)[0]), 256) + 255) // 256 * 256

    @staticmethod
    def _buf(nbytes, device):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)

    # -- granular (reference "serial" route) ---------------------------------------------------
    def full_forward(self, inputs, transition, input_lengths, flags=0, tail_bytes=0):
        if inputs.shape[2] > 256:
            self.check_faults()          # (resident-slice route: a launch that timed out was repaired in stream; say that the route is gone)
        self._check(inputs, transition, None, input_lengths, None)
        L = _lib.lib()
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, None, input_lengths, None)
            state = self._buf(self._state_bytes(p) + tail_bytes, inputs.device)      # (tail: room the caller wants behind the state)
            scores = torch.empty(inputs.shape[1], dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_full_forward(ctypes.byref(p), state.data_ptr(), state.numel(), scores.data_ptr(),
                                          flags, self._stream(inputs.device)), "asg_full_forward")
        return scores, state

    def full_backward(self, state, grad_out, inputs, transition, input_lengths):
        L = _lib.lib()
        T, B, N = inputs.shape
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, None, input_lengths, None)
            g = grad_out.to(inputs.dtype).contiguous()
            scratch = self._buf(self._bytes(p)[1], inputs.device)
            gtr = torch.empty(N, N, dtype=inputs.dtype, device=inputs.device)
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_full_backward(ctypes.byref(p), state.data_ptr(), state.numel(), g.data_ptr(),
                                           scratch.data_ptr(), scratch.numel(), gtr.data_ptr(), gin.data_ptr(),
                                           self._stream(inputs.device)), "asg_full_backward")
        return gtr, gin

    def aligned_forward(self, inputs, targets, transition, input_lengths, target_lengths, flags=0, tail_bytes=0):
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        L = _lib.lib()
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            state = self._buf(self._state_bytes(p) + tail_bytes, inputs.device)
            scores = torch.empty(inputs.shape[1], dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_aligned_forward(ctypes.byref(p), state.data_ptr(), state.numel(), scores.data_ptr(),
                                             flags, self._stream(inputs.device)), "asg_aligned_forward")
        return scores, state

    def aligned_backward(self, state, grad_out, inputs, targets, transition, input_lengths, target_lengths):
        L = _lib.lib()
        T, B, N = inputs.shape
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            g = grad_out.to(inputs.dtype).contiguous()
            scratch = self._buf(self._bytes(p)[1], inputs.device)
            gtr = torch.empty(N, N, dtype=inputs.dtype, device=inputs.device)
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_aligned_backward(ctypes.byref(p), state.data_ptr(), state.numel(), g.data_ptr(),
                                              scratch.data_ptr(), scratch.numel(), gtr.data_ptr(), gin.data_ptr(),
                                              self._stream(inputs.device)), "asg_aligned_backward")
        return gtr, gin

    # -- fused (reference GPU fast route) --------------------------------------------------------
    def forward(self, inputs, targets, transition, input_lengths, target_lengths, flags=_lib.FLAG_STREAMS, tail_bytes=0):
        if inputs.shape[2] > 256:
            self.check_faults()          # (resident-slice route: a launch that timed out was repaired in stream; say that the route is gone)
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        L = _lib.lib()
        B = inputs.shape[1]
        k = 2 if flags & _lib.FLAG_ALPHA_SCORES else 1
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            state = self._buf(self._state_bytes(p) + tail_bytes, inputs.device)
            scores = torch.empty(2, k * B, dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_forward(self._context(inputs.device), ctypes.byref(p), state.data_ptr(), state.numel(),
                                     scores[0].data_ptr(), scores[1].data_ptr(), flags,
                                     self._stream(inputs.device)), "asg_forward")
        return scores[0], scores[1], state

    def forward_only(self, inputs, targets, transition, input_lengths, target_lengths, flags=_lib.FLAG_STREAMS):
        if inputs.shape[2] > 256:
            self.check_faults()          # (resident-slice route: a launch that timed out was repaired in stream; say that the route is gone)
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        L = _lib.lib()
        T, B, N = inputs.shape
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            state = None
            if N > 64 or p.S > 64:
                state = self._buf(self._bytes(p)[0], inputs.device)
            scores = torch.empty(2, B, dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_forward_only(self._context(inputs.device), ctypes.byref(p),
                                          state.data_ptr() if state is not None else None,
                                          state.numel() if state is not None else 0,
                                          scores[0].data_ptr(), scores[1].data_ptr(), flags,
                                          self._stream(inputs.device)), "asg_forward_only")
        return scores[0], scores[1]

    def viterbi(self, inputs, targets, transition, input_lengths, target_lengths):
        """Best-path force alignment -> (scores[B], positions[B,T] int64); see include/asg_hip.h::asg_viterbi."""
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        L = _lib.lib()
        T, B, N = inputs.shape
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            work = self._buf(int(L.asg_viterbi_work_bytes(ctypes.byref(p))), inputs.device)
            scores = torch.empty(B, dtype=inputs.dtype, device=inputs.device)
            path = torch.empty(B, T, dtype=torch.int64, device=inputs.device)
            # (no context: asg_viterbi ignores it and runs on one stream; nothing is created here, so it may run under capture)
            _lib.check(L.asg_viterbi(None, ctypes.byref(p), work.data_ptr(), work.numel(),
                                     scores.data_ptr(), path.data_ptr(), 0, self._stream(inputs.device)),
                       "asg_viterbi")
        return scores, path

    def viterbi_decode(self, inputs, transition, input_lengths):
        """Best label path over the full lattice -> (scores[B], path[B,T], tokens[B,T], token_lengths[B]); see
        include/asg_hip.h::asg_viterbi_decode."""
        self._check(inputs, transition, None, input_lengths, None)
        if inputs.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % inputs.dtype)
        L = _lib.lib()
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            p, keep = self._problem(inputs, transition, None, input_lengths, None)
            work = self._buf(int(L.asg_viterbi_decode_work_bytes(ctypes.byref(p))), dev)
            scores = torch.empty(B, dtype=inputs.dtype, device=dev)
            out = torch.empty(2, B, T, dtype=torch.int64, device=dev)
            token_lengths = torch.empty(B, dtype=torch.int64, device=dev)
            # (no context: the call runs on one stream; nothing is created here, so it may run under capture)
            _lib.check(L.asg_viterbi_decode(None, ctypes.byref(p), work.data_ptr(), work.numel(),
                                            scores.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                            token_lengths.data_ptr(), 0, self._stream(dev)), "asg_viterbi_decode")
        return scores, out[0], out[1], token_lengths

    def viterbi_decode_graph(self, inputs, transition, graph, input_lengths, lm_weight=1.0, token_score=0.0,
                             max_work_bytes=1 << 30, flags=0):
        """Best path over the lattice composed with a token automaton -> (scores[B], path[B,T], tokens[B,T],
        token_lengths[B], states[B,T]); see include/asg_hip.h::asg_viterbi_decode_graph.  Utterances are decoded in
        consecutive groups whose workspace fits `max_work_bytes` (at least one utterance per group)."""
        from . import graph as _graph
        L = _lib.lib()

        def view(dev, dtype):
            compiled = graph.compile(dev, dtype, lm_weight, token_score)
            return _graph.abi_graph(compiled), compiled["Q"]

        def work_bytes(p, g):
            return L.asg_viterbi_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(g))

        def call(p, g, work, nbytes, scores, path, tokens, token_lengths, states, stream):
            return L.asg_viterbi_decode_graph(None, ctypes.byref(p), ctypes.byref(g), work, nbytes, scores, path, tokens,
                                              token_lengths, states, flags, stream)
        return self._decode_graph(inputs, transition, graph, input_lengths, max_work_bytes, view, work_bytes, call,
                                  "asg_viterbi_decode_graph")

    def beam_decode_graph(self, inputs, transition, graph, input_lengths, beam_size, beam_threshold=float("inf"), lm_weight=1.0,
                          token_score=0.0, max_work_bytes=1 << 30, flags=0):
        """Beam-pruned best path over the lattice composed with a token automaton -> the five tensors of
        `viterbi_decode_graph`; see include/asg_hip.h::asg_beam_decode_graph.  Grouped under `max_work_bytes` likewise."""
        from . import graph as _graph
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        L = _lib.lib()

        def view(dev, dtype):
            compiled = graph.compile_beam(dev, dtype, lm_weight, token_score)
            return _graph.abi_graph_beam(compiled), compiled["Q"]

        def work_bytes(p, g):
            return L.asg_beam_decode_graph_work_bytes(ctypes.byref(p), ctypes.byref(g), beam_size)

        def call(p, g, work, nbytes, scores, path, tokens, token_lengths, states, stream):
            return L.asg_beam_decode_graph(None, ctypes.byref(p), ctypes.byref(g), beam_size, beam_threshold, work, nbytes, scores,
                                           path, tokens, token_lengths, states, flags, stream)
        return self._decode_graph(inputs, transition, graph, input_lengths, max_work_bytes, view, work_bytes, call,
                                  "asg_beam_decode_graph")

    def _decode_graph(self, inputs, transition, graph, input_lengths, max_work_bytes, view, work_bytes, call, what):
        """What the two graph decoders share: the checks, the utterance groups under `max_work_bytes`, the outputs.  `view`
        compiles the graph for (device, dtype) -> its C view and its number of product states."""
        self._check_graph_inputs(inputs, transition, graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            g, Q = view(dev, inputs.dtype)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            groups = self._groups(p, B, max_work_bytes, lambda: work_bytes(p, g), Q,
                                  lambda: _lib.check(call(p, g, None, 0, None, None, None, None, None, None), what),
                                  inputs, input_lengths=input_lengths)
            scores = torch.empty(B, dtype=inputs.dtype, device=dev)
            out = torch.empty(3, B, T, dtype=torch.int64, device=dev)        # path, tokens, states
            token_lengths = torch.empty(B, dtype=torch.int64, device=dev)
            stream = self._stream(dev)
            # (no context: the call runs on one stream; nothing is created here once the graph is compiled, so it may run
            # under capture)
            for b0, b1, work in groups:
                _lib.check(call(p, g, work.data_ptr(), work.numel(), scores[b0:].data_ptr(), out[0, b0].data_ptr(),
                                out[1, b0].data_ptr(), token_lengths[b0:].data_ptr(), out[2, b0].data_ptr(), stream), what)
        return scores, out[0], out[1], token_lengths, out[2]

    def beam_decode_words(self, inputs, transition, lexicon, word_lm, input_lengths, beam_size, beam_threshold=float("inf"),
                          lm_weight=1.0, word_score=0.0, token_score=0.0, max_work_bytes=1 << 30, lookahead=None):
        """Beam search over (LM history, lexicon product state) pairs -> BeamWords; see
        include/asg_hip.h::asg_beam_decode_words and, with a `WordLookahead`, asg_beam_decode_words_la.  Grouped under
        `max_work_bytes` as `_decode_graph` does."""
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if lookahead is not None:
            _wordlm.check_lookahead(lookahead, lexicon, word_lm)
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        L = _lib.lib()
        self._check_graph_inputs(inputs, transition, lexicon.graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            g, w, (lex, _) = _wordlm.abi_words(lexicon, word_lm, dev, inputs.dtype, lm_weight, word_score, token_score)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            what = "asg_beam_decode_words"
            if lookahead is not None:
                what = "asg_beam_decode_words_la"
                la_dev = lookahead.compile(dev, inputs.dtype, lm_weight, word_score)
                la = _wordlm.abi_lookahead(la_dev)

            def call(work, nbytes, *outs):
                if lookahead is not None:
                    return L.asg_beam_decode_words_la(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), ctypes.byref(la),
                                                      beam_size, beam_threshold, work, nbytes, *outs)
                return L.asg_beam_decode_words(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size, beam_threshold,
                                               work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_decode_words_work_bytes(ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size), lex["Q"],
                lambda: _lib.check(call(None, 0, *(None,) * 8, 0, None), what),
                inputs, input_lengths=input_lengths)
            scores = torch.empty(B, dtype=inputs.dtype, device=dev)
            out = torch.empty(5, B, T, dtype=torch.int64, device=dev)      # path, tokens, states, lm_states, words
            lengths = torch.empty(2, B, dtype=torch.int64, device=dev)     # token_lengths, word_lengths
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), scores[b0:].data_ptr(), out[0, b0].data_ptr(),
                                out[1, b0].data_ptr(), lengths[0, b0:].data_ptr(), out[2, b0].data_ptr(), out[3, b0].data_ptr(),
                                out[4, b0].data_ptr(), lengths[1, b0:].data_ptr(), 0, stream), what)
        return BeamWords(scores, out[0], out[1], lengths[0], out[2], out[3], out[4], lengths[1])

    def beam_decode_words_confidence(self, inputs, transition, lexicon, word_lm, input_lengths, beam_size,
                                     beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                     frame_tolerance=0, max_work_bytes=1 << 30, lookahead=None):
        """`beam_decode_words` with the end frame and the lattice posterior of every word of the hypothesis -> BeamWordsConfidence;
        see include/asg_hip.h::asg_beam_words_confidence and, with a `WordLookahead`, asg_beam_words_confidence_la.  Grouped under
        `max_work_bytes` as `_decode_graph` does."""
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if lookahead is not None:
            _wordlm.check_lookahead(lookahead, lexicon, word_lm)
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        tol = max(-1, min(int(frame_tolerance), (1 << 31) - 1))
        L = _lib.lib()
        self._check_graph_inputs(inputs, transition, lexicon.graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            g, w, (lex, _) = _wordlm.abi_words(lexicon, word_lm, dev, inputs.dtype, lm_weight, word_score, token_score)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            what = "asg_beam_words_confidence"
            if lookahead is not None:
                what = "asg_beam_words_confidence_la"
                la_dev = lookahead.compile(dev, inputs.dtype, lm_weight, word_score)
                la = _wordlm.abi_lookahead(la_dev)

            def call(work, nbytes, *outs):
                if lookahead is not None:
                    return L.asg_beam_words_confidence_la(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), ctypes.byref(la),
                                                          beam_size, beam_threshold, tol, work, nbytes, *outs)
                return L.asg_beam_words_confidence(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size,
                                                   beam_threshold, tol, work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_words_confidence_work_bytes(ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size),
                lex["Q"], lambda: _lib.check(call(None, 0, *(None,) * 11, 0, None), what),
                inputs, input_lengths=input_lengths)
            real = torch.empty(2, B, dtype=inputs.dtype, device=dev)       # scores, normalisers
            conf = torch.empty(B, T, dtype=inputs.dtype, device=dev)
            out = torch.empty(6, B, T, dtype=torch.int64, device=dev)      # path, tokens, states, lm_states, words, word_frames
            lengths = torch.empty(2, B, dtype=torch.int64, device=dev)     # token_lengths, word_lengths
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), real[0, b0:].data_ptr(), out[0, b0].data_ptr(),
                                out[1, b0].data_ptr(), lengths[0, b0:].data_ptr(), out[2, b0].data_ptr(), out[3, b0].data_ptr(),
                                out[4, b0].data_ptr(), lengths[1, b0:].data_ptr(), out[5, b0].data_ptr(), conf[b0].data_ptr(),
                                real[1, b0:].data_ptr(), 0, stream), what)
        return BeamWordsConfidence(real[0], out[0], out[1], lengths[0], out[2], out[3], out[4], lengths[1], out[5], conf, real[1])

    def beam_decode_words_nbest(self, inputs, transition, lexicon, word_lm, input_lengths, beam_size, nbest,
                                beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                return_alignments=False, max_work_bytes=1 << 30, lookahead=None):
        """The n best hypotheses of the search over pairs with their score split three ways -> BeamWordsNbest; see
        include/asg_hip.h::asg_beam_decode_words_nbest and, with a `WordLookahead`, asg_beam_decode_words_nbest_la (the same
        workspace).  Grouped under `max_work_bytes` as `_decode_graph` does."""
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if lookahead is not None:
            _wordlm.check_lookahead(lookahead, lexicon, word_lm)
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        nbest = min(int(nbest), (1 << 31) - 1)
        L = _lib.lib()
        self._check_graph_inputs(inputs, transition, lexicon.graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            g, w, (lex, _) = _wordlm.abi_words(lexicon, word_lm, dev, inputs.dtype, lm_weight, word_score, token_score)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            what = "asg_beam_decode_words_nbest"
            if lookahead is not None:
                what = "asg_beam_decode_words_nbest_la"
                la_dev = lookahead.compile(dev, inputs.dtype, lm_weight, word_score)
                la = _wordlm.abi_lookahead(la_dev)

            def call(work, nbytes, *outs):
                if lookahead is not None:
                    return L.asg_beam_decode_words_nbest_la(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w),
                                                            ctypes.byref(la), beam_size, beam_threshold, nbest, work, nbytes, *outs)
                return L.asg_beam_decode_words_nbest(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size,
                                                     beam_threshold, nbest, work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_decode_words_nbest_work_bytes(ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size, nbest),
                lex["Q"], lambda: _lib.check(call(None, 0, *(None,) * 12, 0, None), what),
                inputs, input_lengths=input_lengths)
            sc = torch.empty(4, B, nbest, dtype=inputs.dtype, device=dev)      # scores, emission, graph and LM scores
            wide = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev)  # tokens, words
            align = torch.empty(3, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else (None,) * 3
            lengths = torch.empty(2, B, nbest, dtype=torch.int64, device=dev)  # token_lengths, word_lengths
            num_hyps = torch.empty(B, dtype=torch.int64, device=dev)
            al = lambda i, b0: align[i, b0:].data_ptr() if return_alignments else None      # noqa: E731
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), sc[0, b0:].data_ptr(), sc[1, b0:].data_ptr(), sc[2, b0:].data_ptr(),
                                sc[3, b0:].data_ptr(), al(0, b0), wide[0, b0:].data_ptr(), lengths[0, b0:].data_ptr(), al(1, b0),
                                al(2, b0), wide[1, b0:].data_ptr(), lengths[1, b0:].data_ptr(), num_hyps[b0:].data_ptr(), 0, stream),
                           what)
        return BeamWordsNbest(sc[0], sc[1], sc[2], sc[3], wide[0], lengths[0], wide[1], lengths[1], num_hyps, align[0], align[1],
                              align[2])

    def beam_decode_words_nbest_confidence(self, inputs, transition, lexicon, word_lm, input_lengths, beam_size, nbest,
                                           beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                           frame_tolerance=0, return_alignments=False, max_work_bytes=1 << 30, lookahead=None):
        """`beam_decode_words_nbest` with the end frame and the lattice posterior of every word of every row, from one search
        -> BeamWordsNbestConfidence; see include/asg_hip.h::asg_beam_words_nbest_confidence and, with a `WordLookahead`,
        asg_beam_words_nbest_confidence_la.  Grouped under `max_work_bytes` as `_decode_graph` does."""
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if lookahead is not None:
            _wordlm.check_lookahead(lookahead, lexicon, word_lm)
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        nbest = min(int(nbest), (1 << 31) - 1)
        tol = max(-1, min(int(frame_tolerance), (1 << 31) - 1))
        L = _lib.lib()
        self._check_graph_inputs(inputs, transition, lexicon.graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            g, w, (lex, _) = _wordlm.abi_words(lexicon, word_lm, dev, inputs.dtype, lm_weight, word_score, token_score)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            what = "asg_beam_words_nbest_confidence"
            if lookahead is not None:
                what = "asg_beam_words_nbest_confidence_la"
                la_dev = lookahead.compile(dev, inputs.dtype, lm_weight, word_score)
                la = _wordlm.abi_lookahead(la_dev)

            def call(work, nbytes, *outs):
                if lookahead is not None:
                    return L.asg_beam_words_nbest_confidence_la(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w),
                                                                ctypes.byref(la), beam_size, beam_threshold, nbest, tol, work, nbytes,
                                                                *outs)
                return L.asg_beam_words_nbest_confidence(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size,
                                                         beam_threshold, nbest, tol, work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_words_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), beam_size,
                                                                     nbest),
                lex["Q"], lambda: _lib.check(call(None, 0, *(None,) * 15, 0, None), what),
                inputs, input_lengths=input_lengths)
            sc = torch.empty(4, B, nbest, dtype=inputs.dtype, device=dev)      # scores, emission, graph and LM scores
            wide = torch.empty(3, B, nbest, T, dtype=torch.int64, device=dev)  # tokens, words, word_frames
            conf = torch.empty(B, nbest, T, dtype=inputs.dtype, device=dev)
            align = torch.empty(3, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else (None,) * 3
            lengths = torch.empty(2, B, nbest, dtype=torch.int64, device=dev)  # token_lengths, word_lengths
            num_hyps = torch.empty(B, dtype=torch.int64, device=dev)
            norm = torch.empty(B, dtype=inputs.dtype, device=dev)
            al = lambda i, b0: align[i, b0:].data_ptr() if return_alignments else None      # noqa: E731
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), sc[0, b0:].data_ptr(), sc[1, b0:].data_ptr(), sc[2, b0:].data_ptr(),
                                sc[3, b0:].data_ptr(), al(0, b0), wide[0, b0:].data_ptr(), lengths[0, b0:].data_ptr(), al(1, b0),
                                al(2, b0), wide[1, b0:].data_ptr(), lengths[1, b0:].data_ptr(), num_hyps[b0:].data_ptr(),
                                wide[2, b0:].data_ptr(), conf[b0:].data_ptr(), norm[b0:].data_ptr(), 0, stream), what)
        return BeamWordsNbestConfidence(sc[0], sc[1], sc[2], sc[3], wide[0], lengths[0], wide[1], lengths[1], num_hyps, align[0],
                                        align[1], align[2], wide[2], conf, norm)

    def _check_graph_inputs(self, inputs, transition, graph, input_lengths, targets=None, target_lengths=None):
        """The argument checks of every entry point that takes a token automaton."""
        from . import graph as _graph
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        if inputs.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % inputs.dtype)
        if not isinstance(graph, _graph.TokenGraph):
            raise TypeError("torch_asg_amd: graph must be a torch_asg_amd.TokenGraph")
        T, B, N = inputs.shape
        if graph.N != N:
            raise RuntimeError("torch_asg_amd: the graph is over %d tokens but the emissions have N = %d" % (graph.N, N))
        if input_lengths is not None and tuple(input_lengths.shape) != (B,):
            raise RuntimeError("torch_asg_amd: input_lengths must have shape [%d]" % B)

    def _device_problem(self, inputs, transition, targets, input_lengths, target_lengths):
        """(p, targets, input_lengths, target_lengths): the problem block and the batch-indexed tensors it points at, as
        `_groups` slices them (on the device, lengths contiguous)."""
        targets, input_lengths, target_lengths = self.device_args(inputs.device, targets, input_lengths, target_lengths)
        p, _ = self._problem(inputs, transition, targets, input_lengths, target_lengths)
        return p, targets, input_lengths, target_lengths

    @staticmethod
    def _group_problem(p, b0, b1, inputs, targets, input_lengths, target_lengths):
        """Point problem `p` at the utterances b0 .. b1 of the batch (lengths on the device, contiguous)."""
        p.inputs = inputs[:, b0:b1].data_ptr()
        p.B = b1 - b0
        if targets is not None:
            p.targets = targets[b0:b1].data_ptr()
        if input_lengths is not None:
            p.input_lengths = input_lengths[b0:b1].data_ptr()
        if target_lengths is not None:
            p.target_lengths = target_lengths[b0:b1].data_ptr()

    def _groups(self, p, B, max_work_bytes, work_bytes, Q, refused, inputs, targets=None, input_lengths=None,
                target_lengths=None, store=False, saved=None):
        """The consecutive utterance groups of one call whose workspace fits `max_work_bytes` (at least one utterance per
        group) -> an iterator of (b0, b1, work) that has pointed problem `p` at utterances b0 .. b1 (`_group_problem`) when
        it yields them.  `work_bytes()` is the library's workspace size for `p` as it stands.  A size of 0 for one utterance
        of an automaton with product states (Q > 0; with none there is nothing to keep) is the library refusing the
        arguments: `refused()`, the entry point's own call without buffers, raises with its status -- here and not in the
        iterator, so before the caller sizes outputs by those arguments.  One workspace of the first (largest) group's size
        serves every group; with `store` every group gets its own, sized for it, for the caller to keep.  A batch that fits one
        group is the problem as it stands: nothing is sliced (host time of the common call).  With `saved`, the
        [(b0, b1, work)] such a call kept, nothing is sized: the iterator points `p` at those groups again (the backward
        passes)."""
        if saved is None:
            def sized(nb):
                p.B = nb
                return int(work_bytes())
            per = sized(1)
            if per == 0 and Q:
                p.B = B
                refused()
            whole = sized(B)
            if whole <= max_work_bytes:          # (B * per overstates it: the parts behind the utterances are rounded once)
                return ((0, B, self._buf(whole, inputs.device)),)
            gsz = max(1, min(B, int(max_work_bytes) // max(per, 1)))
            while gsz > 1 and sized(gsz) > max_work_bytes:
                gsz -= 1
            if gsz == B:
                return ((0, B, self._buf(sized(B), inputs.device)),)

        def walk():
            if saved is not None:
                for b0, b1, work in saved:
                    self._group_problem(p, b0, b1, inputs, targets, input_lengths, target_lengths)
                    yield b0, b1, work
                return
            work = None
            for b0 in range(0, B, gsz):
                b1 = min(B, b0 + gsz)
                if store or work is None:
                    work = self._buf(sized(b1 - b0), inputs.device)
                self._group_problem(p, b0, b1, inputs, targets, input_lengths, target_lengths)
                yield b0, b1, work
        return walk()

    def beam_decode_graph_nbest(self, inputs, transition, graph, input_lengths, beam_size, nbest, beam_threshold=float("inf"),
                                lm_weight=1.0, token_score=0.0, return_alignments=False, max_work_bytes=1 << 30):
        """The n best final hypotheses of the beam search with their score split -> (scores, emission_scores, graph_scores
        [B,nbest], tokens [B,nbest,T], token_lengths [B,nbest], num_hyps [B], path, states [B,nbest,T] or None); see
        include/asg_hip.h::asg_beam_decode_graph_nbest.  Grouped under `max_work_bytes` as `_decode_graph` does."""
        from . import graph as _graph
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        nbest = min(int(nbest), (1 << 31) - 1)
        L = _lib.lib()
        self._check_graph_inputs(inputs, transition, graph, input_lengths)
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            compiled = graph.compile_beam(dev, inputs.dtype, lm_weight, token_score)
            g = _graph.abi_graph_beam(compiled)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)

            def call(work, nbytes, *outs):
                return L.asg_beam_decode_graph_nbest(None, ctypes.byref(p), ctypes.byref(g), beam_size, beam_threshold, nbest,
                                                     work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_decode_graph_nbest_work_bytes(ctypes.byref(p), ctypes.byref(g), beam_size, nbest), compiled["Q"],
                lambda: _lib.check(call(None, 0, *(None,) * 8, 0, None), "asg_beam_decode_graph_nbest"),
                inputs, input_lengths=input_lengths)
            sc = torch.empty(3, B, nbest, dtype=inputs.dtype, device=dev)      # scores, emission_scores, graph_scores
            tokens = torch.empty(B, nbest, T, dtype=torch.int64, device=dev)
            align = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else None
            token_lengths = torch.empty(B, nbest, dtype=torch.int64, device=dev)
            num_hyps = torch.empty(B, dtype=torch.int64, device=dev)
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), sc[0, b0:].data_ptr(), sc[1, b0:].data_ptr(), sc[2, b0:].data_ptr(),
                                align[0, b0:].data_ptr() if return_alignments else None, tokens[b0:].data_ptr(),
                                token_lengths[b0:].data_ptr(), align[1, b0:].data_ptr() if return_alignments else None,
                                num_hyps[b0:].data_ptr(), 0, stream), "asg_beam_decode_graph_nbest")
        return BeamNbest(sc[0], sc[1], sc[2], tokens, token_lengths, num_hyps,
                         align[0] if return_alignments else None, align[1] if return_alignments else None)

    def _lattice_forward(self, entry, sizer, prepare, size_args, call_args, inputs, transition, targets, input_lengths,
                         target_lengths, store, max_work_bytes, flags=0):
        """The forward of the graph loss and of the two beam-pruned losses -> (scores[B], saved).  `entry` / `sizer` name the
        library's *_full_forward / *_full_work_bytes; `prepare()`, called under the device guard, checks the family's
        arguments and returns (the ctypes views that follow the problem in both calls, Q, what those views point into) and,
        as an optional fourth element, the views that follow those in the forward alone (a look-ahead: it sizes nothing);
        `size_args` / `call_args` are what follows the views in the size call (before `store`) and in the forward (before the
        workspace)."""
        L = _lib.lib()
        forward, work_bytes = getattr(L, entry), getattr(L, sizer)
        dev = inputs.device
        B = inputs.shape[1]
        with self._guard(dev):
            views, Q, keep, *only = prepare()
            p, targets, input_lengths, target_lengths = self._device_problem(inputs, transition, targets, input_lengths,
                                                                             target_lengths)
            fl = flags | (_lib.FLAG_GRAPH_LOSS_KEEP_ALPHA if store else 0)
            head = [ctypes.byref(p)] + [ctypes.byref(v) for v in views]
            tail = [ctypes.byref(v) for v in (only[0] if only else ())]

            def call(work, nbytes, scores, stream):
                return forward(None, *head, *tail, *call_args, work, nbytes, scores, fl, stream)
            groups = self._groups(p, B, max_work_bytes, lambda: work_bytes(*head, *size_args, int(store)), Q,
                                  lambda: _lib.check(call(None, 0, None, None), entry),
                                  inputs, targets, input_lengths, target_lengths, store=store)
            scores = torch.empty(B, dtype=inputs.dtype, device=dev)
            stream = self._stream(dev)
            saved = []
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), scores[b0:].data_ptr(), stream), entry)
                saved.append((b0, b1, work))
        return scores, (saved if store else None)

    def _lattice_backward(self, entry, sizer, prepare, size_args, saved, scores, grad_scores, inputs, transition, targets,
                          input_lengths, target_lengths):
        """The backward of the two beam-pruned losses -> (grad_transition[N,N], grad_inputs[T,B,N]); `entry` / `sizer` name
        the library's *_full_backward / *_full_scratch_bytes, `prepare` and `size_args` are `_lattice_forward`'s.  The groups
        add into one grad_transition in batch order (ASG_FLAG_BEAM_LOSS_ACCUMULATE from the second on)."""
        L = _lib.lib()
        backward, scratch_bytes = getattr(L, entry), getattr(L, sizer)
        dev = inputs.device
        T, B, N = inputs.shape
        with self._guard(dev):
            views, _, keep = prepare()
            p, targets, input_lengths, target_lengths = self._device_problem(inputs, transition, targets, input_lengths,
                                                                             target_lengths)
            head = [ctypes.byref(p)] + [ctypes.byref(v) for v in views]
            gs = grad_scores.to(inputs.dtype).contiguous()
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=dev)
            gtr = torch.empty(N, N, dtype=inputs.dtype, device=dev)
            stream = self._stream(dev)
            groups = self._groups(p, B, None, None, None, None, inputs, targets, input_lengths, target_lengths, saved=saved)
            for n, (b0, b1, work) in enumerate(groups):
                nb = b1 - b0
                scratch = self._buf(scratch_bytes(*head, *size_args), dev)
                gin_g = gin if nb == B else torch.empty(T, nb, N, dtype=inputs.dtype, device=dev)
                _lib.check(backward(None, *head, *size_args, work.data_ptr(), work.numel(), scores[b0:].data_ptr(),
                                    gs[b0:].data_ptr(), gin_g.data_ptr(), gtr.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                    _lib.FLAG_BEAM_LOSS_ACCUMULATE if n else 0, stream), entry)
                if nb != B:
                    gin[:, b0:b1].copy_(gin_g)
        return gtr, gin

    def _graph_loss_args(self, inputs, transition, graph, input_lengths, lm_weight, token_score, targets=None,
                         target_lengths=None):
        """Checks shared by the graph-loss entry points -> the compiled graph and its asg_token_graph_loss view."""
        from . import graph as _graph
        self._check_graph_inputs(inputs, transition, graph, input_lengths, targets, target_lengths)
        compiled = graph.compile_loss(inputs.device, inputs.dtype, lm_weight, token_score)
        return compiled, _graph.abi_graph_loss(compiled)

    def graph_full_forward(self, inputs, transition, graph, input_lengths, lm_weight=1.0, token_score=0.0, store=False,
                           max_work_bytes=1 << 30, flags=0):
        """Full score of the lattice composed with a token automaton -> (scores[B], saved); see
        include/asg_hip.h::asg_graph_full_forward.  Utterances run in consecutive groups whose workspace fits `max_work_bytes`.
        With `store`, saved = [(b0, b1, work)]: each group's stored alpha, for graph_full_backward; None otherwise."""
        def prepare():
            compiled, gl = self._graph_loss_args(inputs, transition, graph, input_lengths, lm_weight, token_score)
            return (gl,), compiled["Q"], compiled
        return self._lattice_forward("asg_graph_full_forward", "asg_graph_full_work_bytes", prepare, (), (), inputs, transition,
                                     None, input_lengths, None, store, max_work_bytes, flags)

    def graph_full_backward(self, saved, scores, grad_scores, inputs, transition, graph, input_lengths, lm_weight=1.0,
                            token_score=0.0, flags=0):
        """(grad_transition[N,N], grad_inputs[T,B,N]) of sum_b grad_scores[b] * scores[b] from graph_full_forward's saved alpha."""
        L = _lib.lib()
        dev = inputs.device
        T, B, N = inputs.shape
        with self._guard(dev):
            compiled, gl = self._graph_loss_args(inputs, transition, graph, input_lengths, lm_weight, token_score)
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)
            gs = grad_scores.to(inputs.dtype).contiguous()
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=dev)
            gtr = None
            stream = self._stream(dev)
            for b0, b1, work in self._groups(p, B, None, None, None, None, inputs, input_lengths=input_lengths, saved=saved):
                nb = b1 - b0
                scratch = self._buf(L.asg_graph_full_scratch_bytes(ctypes.byref(p), ctypes.byref(gl)), dev)
                gin_g = gin if nb == B else torch.empty(T, nb, N, dtype=inputs.dtype, device=dev)
                gtr_g = torch.empty(N, N, dtype=inputs.dtype, device=dev)
                _lib.check(L.asg_graph_full_backward(None, ctypes.byref(p), ctypes.byref(gl), work.data_ptr(), work.numel(),
                                                     scores[b0:].data_ptr(), gs[b0:].data_ptr(), gin_g.data_ptr(),
                                                     gtr_g.data_ptr(), scratch.data_ptr(), scratch.numel(), flags, stream),
                           "asg_graph_full_backward")
                if nb != B:
                    gin[:, b0:b1].copy_(gin_g)
                gtr = gtr_g if gtr is None else gtr + gtr_g
        return gtr, gin

    def _beam_loss_args(self, inputs, transition, graph, input_lengths, targets, target_lengths, lm_weight, token_score):
        """Checks shared by the beam-pruned loss entry points -> ((the asg_token_graph_beam_loss view,), Q, the compiled graph it
        points into): `_lattice_forward`'s `prepare`."""
        from . import graph as _graph
        self._check_graph_inputs(inputs, transition, graph, input_lengths, targets, target_lengths)
        compiled = graph.compile_beam_loss(inputs.device, inputs.dtype, lm_weight, token_score)
        return (_graph.abi_graph_beam_loss(compiled),), compiled["Q"], compiled

    def beam_graph_full_forward(self, inputs, transition, graph, input_lengths, beam_size, beam_threshold=float("inf"),
                                lm_weight=1.0, token_score=0.0, targets=None, target_lengths=None, store=False,
                                max_work_bytes=1 << 30):
        """Beam-pruned full score of the lattice composed with a token automaton -> (scores[B], saved); see
        include/asg_hip.h::asg_beam_graph_full_forward.  Utterances run in consecutive groups whose workspace fits
        `max_work_bytes`.  With `store`, saved = [(b0, b1, work)] for beam_graph_full_backward; None otherwise."""
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        return self._lattice_forward(
            "asg_beam_graph_full_forward", "asg_beam_graph_full_work_bytes",
            lambda: self._beam_loss_args(inputs, transition, graph, input_lengths, targets, target_lengths, lm_weight, token_score),
            (beam_size,), (beam_size, beam_threshold), inputs, transition, targets, input_lengths, target_lengths, store,
            max_work_bytes)

    def beam_graph_full_backward(self, saved, scores, grad_scores, inputs, transition, graph, input_lengths, beam_size,
                                 lm_weight=1.0, token_score=0.0, targets=None, target_lengths=None):
        """(grad_transition[N,N], grad_inputs[T,B,N]) of sum_b grad_scores[b] * scores[b] from beam_graph_full_forward's saved
        lattices.  The groups add into one grad_transition in batch order, so the result does not depend on the grouping."""
        beam_size = min(int(beam_size), (1 << 31) - 1)
        return self._lattice_backward(
            "asg_beam_graph_full_backward", "asg_beam_graph_full_scratch_bytes",
            lambda: self._beam_loss_args(inputs, transition, graph, input_lengths, targets, target_lengths, lm_weight, token_score),
            (beam_size,), saved, scores, grad_scores, inputs, transition, targets, input_lengths, target_lengths)

    def beam_decode_graph_confidence(self, inputs, transition, graph, input_lengths, beam_size, beam_threshold=float("inf"),
                                     lm_weight=1.0, token_score=0.0, frame_tolerance=0, max_work_bytes=1 << 30):
        """`beam_decode_graph` with the start frame and the lattice posterior of every token of the hypothesis ->
        BeamGraphConfidence; see include/asg_hip.h::asg_beam_graph_confidence.  The graph goes through the compile of the
        beam-pruned loss (`_beam_loss_args`, cached on it); grouped under `max_work_bytes` as `_decode_graph` does."""
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        tol = max(-1, min(int(frame_tolerance), (1 << 31) - 1))
        L = _lib.lib()
        what = "asg_beam_graph_confidence"
        from . import graph as _graph
        if not isinstance(graph, _graph.TokenGraph):                           # the graph is checked before the device
            raise TypeError("torch_asg_amd: graph must be a torch_asg_amd.TokenGraph")
        if inputs.dim() == 3 and graph.N != inputs.shape[2]:
            raise RuntimeError("torch_asg_amd: the graph is over %d tokens but the emissions have N = %d" % (graph.N, inputs.shape[2]))
        dev = inputs.device
        with self._guard(dev):
            (gl,), Q, keep = self._beam_loss_args(inputs, transition, graph, input_lengths, None, None, lm_weight, token_score)
            T, B, N = inputs.shape
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)

            def call(work, nbytes, *outs):
                return L.asg_beam_graph_confidence(None, ctypes.byref(p), ctypes.byref(gl), beam_size, beam_threshold, tol, work,
                                                   nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes, lambda: L.asg_beam_graph_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), beam_size),
                Q, lambda: _lib.check(call(None, 0, *(None,) * 8, 0, None), what), inputs, input_lengths=input_lengths)
            real = torch.empty(2, B, dtype=inputs.dtype, device=dev)       # scores, normalisers
            conf = torch.empty(B, T, dtype=inputs.dtype, device=dev)
            out = torch.empty(4, B, T, dtype=torch.int64, device=dev)      # path, tokens, states, token_frames
            token_lengths = torch.empty(B, dtype=torch.int64, device=dev)
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), real[0, b0:].data_ptr(), out[0, b0].data_ptr(),
                                out[1, b0].data_ptr(), token_lengths[b0:].data_ptr(), out[2, b0].data_ptr(), out[3, b0].data_ptr(),
                                conf[b0].data_ptr(), real[1, b0:].data_ptr(), 0, stream), what)
        return BeamGraphConfidence(real[0], out[0], out[1], token_lengths, out[2], out[3], conf, real[1])

    def beam_decode_graph_nbest_confidence(self, inputs, transition, graph, input_lengths, beam_size, nbest,
                                           beam_threshold=float("inf"), lm_weight=1.0, token_score=0.0, return_alignments=False,
                                           frame_tolerance=0, max_work_bytes=1 << 30):
        """`beam_decode_graph_nbest` with the start frame and the lattice posterior of every token of every row, from one
        search -> BeamNbestConfidence; see include/asg_hip.h::asg_beam_graph_nbest_confidence.  The graph goes through the
        compile of the beam-pruned loss (`_beam_loss_args`, cached on it); grouped under `max_work_bytes` as `_decode_graph`
        does."""
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        nbest = min(int(nbest), (1 << 31) - 1)
        tol = max(-1, min(int(frame_tolerance), (1 << 31) - 1))
        L = _lib.lib()
        what = "asg_beam_graph_nbest_confidence"
        from . import graph as _graph
        if not isinstance(graph, _graph.TokenGraph):                           # the graph is checked before the device
            raise TypeError("torch_asg_amd: graph must be a torch_asg_amd.TokenGraph")
        if inputs.dim() == 3 and graph.N != inputs.shape[2]:
            raise RuntimeError("torch_asg_amd: the graph is over %d tokens but the emissions have N = %d" % (graph.N, inputs.shape[2]))
        dev = inputs.device
        with self._guard(dev):
            (gl,), Q, keep = self._beam_loss_args(inputs, transition, graph, input_lengths, None, None, lm_weight, token_score)
            T, B, N = inputs.shape
            p, _, input_lengths, _ = self._device_problem(inputs, transition, None, input_lengths, None)

            def call(work, nbytes, *outs):
                return L.asg_beam_graph_nbest_confidence(None, ctypes.byref(p), ctypes.byref(gl), beam_size, beam_threshold, nbest,
                                                         tol, work, nbytes, *outs)
            groups = self._groups(
                p, B, max_work_bytes,
                lambda: L.asg_beam_graph_nbest_confidence_work_bytes(ctypes.byref(p), ctypes.byref(gl), beam_size, nbest),
                Q, lambda: _lib.check(call(None, 0, *(None,) * 11, 0, None), what), inputs, input_lengths=input_lengths)
            sc = torch.empty(3, B, nbest, dtype=inputs.dtype, device=dev)      # scores, emission_scores, graph_scores
            wide = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev)  # tokens, token_frames
            conf = torch.empty(B, nbest, T, dtype=inputs.dtype, device=dev)
            align = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else (None,) * 2
            token_lengths = torch.empty(B, nbest, dtype=torch.int64, device=dev)
            num_hyps = torch.empty(B, dtype=torch.int64, device=dev)
            norm = torch.empty(B, dtype=inputs.dtype, device=dev)
            al = lambda i, b0: align[i, b0:].data_ptr() if return_alignments else None      # noqa: E731
            stream = self._stream(dev)
            for b0, b1, work in groups:
                _lib.check(call(work.data_ptr(), work.numel(), sc[0, b0:].data_ptr(), sc[1, b0:].data_ptr(), sc[2, b0:].data_ptr(),
                                al(0, b0), wide[0, b0:].data_ptr(), token_lengths[b0:].data_ptr(), al(1, b0),
                                num_hyps[b0:].data_ptr(), wide[1, b0:].data_ptr(), conf[b0:].data_ptr(), norm[b0:].data_ptr(), 0,
                                stream), what)
        return BeamNbestConfidence(sc[0], sc[1], sc[2], wide[0], token_lengths, num_hyps, align[0], align[1], wide[1], conf, norm)

    def graph_target_scores(self, inputs, transition, graph, targets, target_lengths, lm_weight=1.0, token_score=0.0):
        """[B]: the automaton's score of every target sequence (consecutive repeats merged), -inf where it rejects it; see
        include/asg_hip.h::asg_graph_target_scores."""
        L = _lib.lib()
        dev = inputs.device
        with self._guard(dev):
            compiled, gl = self._graph_loss_args(inputs, transition, graph, None, lm_weight, token_score, targets, target_lengths)
            p, keep = self._problem(inputs, transition, targets, None, target_lengths)
            out = torch.empty(inputs.shape[1], dtype=inputs.dtype, device=dev)
            _lib.check(L.asg_graph_target_scores(None, ctypes.byref(p), ctypes.byref(gl), out.data_ptr(), self._stream(dev)),
                       "asg_graph_target_scores")
        return out

    def _word_loss_args(self, inputs, transition, lexicon, word_lm, input_lengths, targets, target_lengths, weights,
                        lookahead=None):
        """Checks shared by the pair-loss entry points -> ((the lexicon's asg_token_graph_beam view, the asg_word_lm view), Q,
        the compiled dicts they point into), through the caches of `Lexicon.compile_words` and `WordLM.compile`:
        `_lattice_forward`'s `prepare`.  With a `WordLookahead`, checked before anything looks at the device and compiled with
        the call's lm_weight and word_score through its own cache, a fourth element: (the asg_word_lookahead view,)."""
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if lookahead is not None:
            _wordlm.check_lookahead(lookahead, lexicon, word_lm)
        self._check_graph_inputs(inputs, transition, lexicon.graph, input_lengths, targets, target_lengths)
        g, w, keep = _wordlm.abi_words(lexicon, word_lm, inputs.device, inputs.dtype, *weights)
        if lookahead is None:
            return (g, w), keep[0]["Q"], keep
        la_dev = lookahead.compile(inputs.device, inputs.dtype, weights[0], weights[1])
        return (g, w), keep[0]["Q"], keep + (la_dev,), (_wordlm.abi_lookahead(la_dev),)

    def beam_words_full_forward(self, inputs, transition, lexicon, word_lm, input_lengths, beam_size, beam_threshold=float("inf"),
                                lm_weight=1.0, word_score=0.0, token_score=0.0, targets=None, target_lengths=None, store=False,
                                max_work_bytes=1 << 30, lookahead=None):
        """Beam-pruned full score over the pairs `beam_decode_words` keeps -> (scores[B], saved); see
        include/asg_hip.h::asg_beam_words_full_forward and, with a `WordLookahead` (the sets of
        `beam_decode_words(..., lookahead=)`), asg_beam_words_full_forward_la.  Grouped and saved as `beam_graph_full_forward`
        does; `beam_words_full_backward` serves both."""
        beam_size, beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        return self._lattice_forward(
            "asg_beam_words_full_forward" if lookahead is None else "asg_beam_words_full_forward_la",
            "asg_beam_words_full_work_bytes",
            lambda: self._word_loss_args(inputs, transition, lexicon, word_lm, input_lengths, targets, target_lengths,
                                         (lm_weight, word_score, token_score), lookahead),
            (beam_size,), (beam_size, beam_threshold), inputs, transition, targets, input_lengths, target_lengths, store,
            max_work_bytes)

    def beam_words_full_backward(self, saved, scores, grad_scores, inputs, transition, lexicon, word_lm, input_lengths, beam_size,
                                 lm_weight=1.0, word_score=0.0, token_score=0.0, targets=None, target_lengths=None):
        """(grad_transition[N,N], grad_inputs[T,B,N]) of sum_b grad_scores[b] * scores[b] from beam_words_full_forward's saved
        lattices.  The groups add into one grad_transition in batch order, so the result does not depend on the grouping."""
        beam_size = min(int(beam_size), (1 << 31) - 1)
        return self._lattice_backward(
            "asg_beam_words_full_backward", "asg_beam_words_full_scratch_bytes",
            lambda: self._word_loss_args(inputs, transition, lexicon, word_lm, input_lengths, targets, target_lengths,
                                         (lm_weight, word_score, token_score)),
            (beam_size,), saved, scores, grad_scores, inputs, transition, targets, input_lengths, target_lengths)

    def words_target_scores(self, inputs, transition, lexicon, word_lm, targets, target_lengths, lm_weight=1.0, word_score=0.0,
                            token_score=0.0):
        """[B]: the lexicon + LM score of every target sequence (consecutive repeats merged), end terms included, -inf where
        either rejects it; see include/asg_hip.h::asg_words_target_scores."""
        L = _lib.lib()
        dev = inputs.device
        with self._guard(dev):
            (g, w), _, keep = self._word_loss_args(inputs, transition, lexicon, word_lm, None, targets, target_lengths,
                                                   (lm_weight, word_score, token_score))
            p, keep_p = self._problem(inputs, transition, targets, None, target_lengths)
            out = torch.empty(inputs.shape[1], dtype=inputs.dtype, device=dev)
            _lib.check(L.asg_words_target_scores(None, ctypes.byref(p), ctypes.byref(g), ctypes.byref(w), out.data_ptr(),
                                                 self._stream(dev)), "asg_words_target_scores")
        return out

    def backward(self, state, grad_full, grad_aligned, inputs, targets, transition, input_lengths, target_lengths,
                 flags=0):
        L = _lib.lib()
        T, B, N = inputs.shape
        with self._guard(inputs.device):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            g = torch.stack([grad_full.to(inputs.dtype), grad_aligned.to(inputs.dtype)]).contiguous()
            scratch = self._buf(self._bytes(p)[1], inputs.device)
            gtr = torch.empty(N, N, dtype=inputs.dtype, device=inputs.device)
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=inputs.device)
            _lib.check(L.asg_backward(self._context(inputs.device), ctypes.byref(p), state.data_ptr(), state.numel(),
                                      g[0].data_ptr(), g[1].data_ptr(), scratch.data_ptr(), scratch.numel(),
                                      gtr.data_ptr(), gin.data_ptr(), flags, self._stream(inputs.device)),
                       "asg_backward")
        return gtr, gin


    # -- whole loss: full - aligned, reduction and their gradients inside the kernels -----------------------
    _RED = {"none": 0, "sum": 1, "mean": 2}

    def _sync(self, device, nbytes):
        """Zeroed device memory for the cross-workgroup words of a fused launch (include/asg_hip.h: zero on entry,
        left zero).  Calls that are ordered on one stream may share a region, so there is one region per calling
        stream for eager calls and one per (capture, stream) for calls recorded into a hipGraph -- graphs that may be
        replayed concurrently never share one, and a capture of many steps consumes one region, not one per step.
        Regions are carved from pools that are allocated and zeroed EAGERLY: never while a capture is in progress
        (the pool would come out of the graph's private memory and its zero-fill would become a graph node)."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        stream = _current_stream_handle(idx)
        capturing = bool(_is_capturing()) if _is_capturing is not None else torch.cuda.is_current_stream_capturing()
        cap = 0
        if capturing:
            cid = ctypes.c_ulonglong(0)
            _lib.check(_lib.lib().asg_stream_capture_id(ctypes.c_void_p(stream), ctypes.byref(cid)), "asg_stream_capture_id")
            cap = int(cid.value) or -1
        key = (idx, stream, cap)
        t = self._tickets.get(key)
        if t is not None and t.numel() >= nbytes:
            return t
        nbytes = (int(nbytes) + 255) // 256 * 256
        with self._lock:
            pool = self._pools.get(idx)
            if pool is None or pool[1] + nbytes > pool[0].numel():
                if capturing:
                    raise RuntimeError(
                        "torch_asg_amd: the fused step needs a zeroed sync region and its pool cannot be created while "
                        "a hipGraph is being captured -- run one warm-up step (or torch_asg_amd.reserve(device)) "
                        "before the capture")
                pool = [torch.zeros(max(self.POOL_BYTES, 4 * nbytes), dtype=torch.uint8, device=device), 0]
                self._pools[idx] = pool
                self._pool_keep.append(pool[0])       # regions handed to captured graphs must outlive the pool's turn
            t = pool[0][pool[1]: pool[1] + nbytes]
            pool[1] += nbytes
            if len(self._tickets) > 4096:             # long runs that keep creating streams / captures
                self._tickets.clear()
            self._tickets[key] = t
        return t

    POOL_BYTES = 1 << 20

    def reserve(self, device, nbytes=0):
        """Create the sync pool of `device` now (e.g. before a capture whose first fused call would need it)."""
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        with self._lock:
            pool = self._pools.get(idx)
            if pool is None or pool[1] + nbytes > pool[0].numel():
                pool = [torch.zeros(max(self.POOL_BYTES, 4 * int(nbytes)), dtype=torch.uint8, device=torch.device("cuda", idx)), 0]
                self._pools[idx] = pool
                self._pool_keep.append(pool[0])

    def release(self):
        """Destroy the side-stream contexts and drop the sync pools (call when no launch of this process is in flight)."""
        with self._lock:
            for h in list(self._ctx.values()) + self._retired:
                _lib.lib().asg_ctx_destroy(h)
            self._ctx.clear()
            self._retired.clear()
            self._tickets.clear()
            self._pools.clear()
            self._pool_keep.clear()
            if self.binding is not None:
                self.binding.reset()

    def fused_supported(self, p):
        return bool(_lib.lib().asg_loss_fused_supported(ctypes.byref(p)))

    def fused_preferred(self, p, device):
        """The fused step gives every utterance three compute units of its own (latency regime: it is what makes the
        cfg-3 step fast); once 3 B exceeds the compute units the launch runs in rounds and the stand-alone kernels,
        which pack one chain per wavefront, are faster (measured on MI355X, 256 CUs, T=400 N=40: B=80 68 us fused;
        B=96 117 us fused vs ~85 stand-alone; B=128 125 vs ~90; tools/batch_sweep.py)."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        cus = self._cu_count(idx)
        # the launch places utterances 2x, 2x+1 on XCD x mod 8 (asg_fused.hip): the fullest XCD must hold its workgroups
        pairs = (int(p.B) + 1) // 2
        return ((pairs + 7) // 8) * 2 * 3 <= cus // 8

    def loss_forward(self, inputs, targets, transition, input_lengths, target_lengths, reduction,
                     flags=_lib.FLAG_STREAMS):
        """loss = reduce(full - aligned).  Returns (loss, saved): `saved` is what loss_backward needs --
        saved.tensors (device buffers, to go through ctx.save_for_backward) and host-side bookkeeping.

        With launch mode 'single' and a supported shape this is the FUSED step: the launch also assembles the
        gradients (for an upstream gradient of 1) into saved.tensors; otherwise the recursion kernels run alone and
        the assembly kernels run in loss_backward."""
        self._check(inputs, transition, targets, input_lengths, target_lengths)
        L = _lib.lib()
        T, B, N = inputs.shape
        if N > 256:
            self.check_faults()          # (resident-slice route: a launch that timed out was repaired in stream; say that the route is gone)
        red = self._RED[reduction]
        dev = inputs.device
        with self._guard(dev):
            p, keep = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            state_bytes = self._bytes(p)[0]
            loss = torch.empty((B,) if red == 0 else (), dtype=transition.dtype, device=dev)
            use_fused = (flags & _lib.FLAG_SINGLE_LAUNCH) and self.fused_supported(p) and self.fused_preferred(p, dev)
            if inputs.dtype == torch.bfloat16 and not use_fused:
                raise RuntimeError("torch_asg_amd: bfloat16 emissions are taken by the fused training step only "
                                   "(ASGLoss upcasts them itself when that route does not apply)")
            if use_fused:
                key = ("fs", p.T, p.B, p.N, p.S, p.inputs_dtype)
                fsz = self._sizes.get(key)
                if fsz is None:
                    fsz = (int(L.asg_loss_fused_scratch_bytes(ctypes.byref(p))), int(L.asg_loss_fused_sync_bytes(ctypes.byref(p))))
                    self._sizes[key] = fsz
                fs, sync_bytes = fsz
                # one workspace: [scores 2B | state | scratch]
                sc_bytes = (2 * B * 4 + 255) // 256 * 256
                ws = torch.empty(sc_bytes + state_bytes + fs, dtype=torch.uint8, device=dev)
                gin = torch.empty(T, B, N, dtype=inputs.dtype, device=dev)
                base = ws.data_ptr()
                _lib.check(L.asg_loss_fused_forward(ctypes.byref(p), base + sc_bytes, state_bytes, red, loss.data_ptr(),
                                                    base, base + sc_bytes + state_bytes, fs, gin.data_ptr(),
                                                    self._sync(dev, sync_bytes).data_ptr(), 0, self._stream(dev)),
                           "asg_loss_fused_forward")
                return loss, _Saved("fused", (ws, gin), p, keep, (sc_bytes, state_bytes, fs))
            state = self._buf(state_bytes, dev)
            scores = torch.empty(2, B, dtype=inputs.dtype, device=dev)
            _lib.check(L.asg_loss_forward(self._context(dev), ctypes.byref(p), state.data_ptr(),
                                          state.numel(), red, loss.data_ptr(), scores.data_ptr(),
                                          flags & ~_lib.FLAG_ALPHA_SCORES, self._stream(dev)),
                       "asg_loss_forward")
        return loss, _Saved("split", (state,), p, keep, None)

    def loss_backward(self, saved, tensors, grad_loss, inputs, targets, transition, input_lengths, target_lengths,
                      reduction):
        """(grad_transition, grad_inputs) of the reduced loss.  `tensors` are saved.tensors as autograd handed them
        back (they may have travelled through saved-tensor hooks)."""
        L = _lib.lib()
        T, B, N = inputs.shape
        dev = inputs.device
        with self._guard(dev):
            p = saved.problem
            if (p is None or p.inputs != inputs.data_ptr() or p.transition != transition.data_ptr() or p.targets != targets.data_ptr()
                    or (p.input_lengths or 0) != (input_lengths.data_ptr() if input_lengths is not None else 0)
                    or (p.target_lengths or 0) != (target_lengths.data_ptr() if target_lengths is not None else 0)):
                # the saved tensors came back at other addresses (saved-tensor hooks): rebuild the problem block
                p, _ = self._problem(inputs, transition, targets, input_lengths, target_lengths)
            g = grad_loss
            if g.dtype != transition.dtype:
                g = g.to(transition.dtype)
            if not g.is_contiguous():
                g = g.contiguous()
            gtr = torch.empty(N, N, dtype=transition.dtype, device=dev)
            if saved.mode == "fused":
                ws, gin = tensors
                sc_bytes, state_bytes, fs = saved.sizes
                base = ws.data_ptr()
                _lib.check(L.asg_loss_fused_backward(ctypes.byref(p), base + sc_bytes, state_bytes, self._RED[reduction],
                                                     g.data_ptr(), base + sc_bytes + state_bytes, fs, gin.data_ptr(),
                                                     gtr.data_ptr(), 0, self._stream(dev)), "asg_loss_fused_backward")
                return gtr, gin
            (state,) = tensors
            scratch = self._buf(self._bytes(p)[1], dev)
            gin = torch.empty(T, B, N, dtype=inputs.dtype, device=dev)
            _lib.check(L.asg_loss_backward(self._context(dev), ctypes.byref(p), state.data_ptr(),
                                           state.numel(), self._RED[reduction], g.data_ptr(), scratch.data_ptr(),
                                           scratch.numel(), gtr.data_ptr(), gin.data_ptr(), 0,
                                           self._stream(dev)), "asg_loss_backward")
        return gtr, gin


    def loss_backward_tensors(self, mode, sc_bytes, state_bytes, fs, red, buf0, buf1, grad_loss, inputs, transition, targets,
                              input_lengths, target_lengths):
        """Backward of a step whose forward ran in csrc/binding.cpp (AsgLossNode) when what autograd handed back is not the
        plain case any more (saved-tensor hooks that return CPU or strided tensors): convert, then the same entry points."""
        dev = transition.device
        inputs = inputs.to(dev)
        targets, input_lengths, target_lengths = self.device_args(dev, targets, input_lengths, target_lengths)
        saved = _Saved("fused" if mode else "split", None, None, None, (sc_bytes, state_bytes, fs))
        tensors = (buf0.to(dev), buf1.to(dev)) if mode else (buf0.to(dev),)
        reduction = [k for k, v in self._RED.items() if v == red][0]
        return self.loss_backward(saved, tensors, grad_loss.to(dev), inputs, targets, transition, input_lengths, target_lengths,
                                  reduction)


class _Saved:
    """Host-side record of one loss_forward call: which route ran, the device buffers it filled, the C problem block."""
    __slots__ = ("mode", "tensors", "problem", "keep", "sizes", "consumed", "rec")

    def __init__(self, mode, tensors, problem, keep, sizes):
        self.mode, self.tensors, self.problem, self.keep, self.sizes = mode, tensors, problem, keep, sizes
        self.consumed = False
        self.rec = None               # (mode, sc_bytes, state_bytes, scratch_bytes, reduction) when csrc/binding.cpp ran the forward


_backend = None
# ASG_NO_CPP_NODE=1: keep the autograd node in Python (ASGLossFunction) -- the A/B switch of tools/host_pieces2.py and of
# tests/test_hip_host.py::test_cpp_node_python_function_and_python_path_are_the_same_call
_CPP_NODE = os.environ.get("ASG_NO_CPP_NODE", "0") in ("", "0")


def native():
    """The native binding used by the autograd Functions (the HIP library; nothing else ships)."""
    global _backend
    if _backend is None:
        _lib.lib()            # fail loudly here if libasg_hip.so is missing
        _backend = HipBackend()
    return _backend


def _check_beam(beam_size, beam_threshold):
    if int(beam_size) < 1:
        raise ValueError("torch_asg_amd: beam_size must be >= 1, got %d" % int(beam_size))
    if not float(beam_threshold) >= 0.0:
        raise ValueError("torch_asg_amd: beam_threshold must be >= 0 (inf: none), got %r" % (beam_threshold,))


def _widen(inputs, transition):
    """float16 / bfloat16 emissions widened to the dtype of `transition`; every other dtype as it is."""
    if inputs.dtype in (torch.float16, torch.bfloat16):
        return inputs.to(transition.dtype)
    return inputs


def _plain(inputs, transition):
    """(emissions, transition) as a decoder takes them: half precision widened, no autograd history."""
    return _widen(inputs, transition).detach(), transition.detach()


def viterbi_align(inputs, targets, transition, input_lengths=None, target_lengths=None):
    """Best-path (Viterbi) force alignment of `targets` to `inputs` under the ASG transition model -- the
    force-aligned lattice of the loss (force_aligned_lattice.cpp:84-111) with max instead of logsumexp
    (doc/tech_report.tex:84-88; a TODO in the reference, README.md:33).  No gradient.

    inputs [T,B,N] (time-major emissions), targets [B,S] int64, transition [N,N], lengths int64 [B] or None.  float16 /
    bfloat16 emissions are widened to the dtype of `transition` first, as the decoders do (so the tokens of `viterbi_decode`
    align against the emissions they were decoded from); the scores then have the dtype of `transition`.
    Returns (scores [B], positions [B,T] int64, labels [B,T] int64): the score of the best alignment, the target
    position occupied at every frame and the label emitted there; -1 for frames >= input_lengths[b] and for
    utterances that have no finite alignment (score -inf).  Same defaults and S > T truncation as ASGLoss.forward.
    """
    T, B, N = inputs.shape
    S = targets.shape[1]
    if target_lengths is None:
        target_lengths = targets.new_full((B,), S)
    if input_lengths is None:
        input_lengths = target_lengths.new_full((B,), T)
    if S > T:
        targets = targets[:, :T]
        target_lengths = torch.clamp(target_lengths, max=T)
    with torch.no_grad():
        inputs, transition = _plain(inputs, transition)
        scores, pos = native().viterbi(inputs, targets, transition, input_lengths, target_lengths)
        labels = torch.where(pos >= 0, torch.gather(targets.to(pos.device), 1, pos.clamp(min=0)), pos)
    return scores, pos, labels


def viterbi_decode(inputs, transition, input_lengths=None):
    """Viterbi decoding over the fully-connected ASG lattice (wav2letter's viterbiPath): the best label path under
    `transition`, and its tokens.  No gradient.

    inputs [T,B,N] emissions (time-major; a transposed [B,T,N] tensor is fine), transition [N,N] (transition[i,j] scores
    the move from label j to label i), input_lengths int64 [B] or None (= T; clamped to [0, T]).  float16 / bfloat16
    emissions are widened to the dtype of `transition` first.  Returns (scores [B] in the dtype of the emissions,
    path [B,T] int64: the label of every frame, -1 for frames >= input_lengths[b], tokens [B,T] int64: the path with
    consecutive repeats collapsed, padded with -1, token_lengths [B] int64).  Ties go to the smallest label index.  An
    utterance of length 0, or one without a finite path, has score -inf, all -1 and no tokens.

    The path is unchanged when a constant is added to every emission of a frame (so a model trained with
    input_is_logits=True decodes its raw logits and their log_softmax to the same path); the score shifts by that
    constant.
    """
    with torch.no_grad():
        return native().viterbi_decode(*_plain(inputs, transition), input_lengths)


def viterbi_decode_graph(inputs, transition, graph, input_lengths=None, lm_weight=1.0, token_score=0.0,
                         max_work_bytes=1 << 30):
    """Exact Viterbi decoding over the ASG lattice composed with a token automaton `graph` (a `TokenGraph`, e.g. an n-gram
    LM from `TokenGraph.from_ngram`).  No pruning and no gradient.

    Every move to a new label is a token: it takes the automaton's arc for that token and adds
    lm_weight * weight + token_score; the end adds lm_weight * final.  Repeated labels are one token and leave the automaton
    where it is.  Arithmetic is in the dtype of the emissions (lm_weight and token_score rounded to it, then folded into the
    arcs on the host); ties go to the smallest product-state index.  Inputs, strides, float16 / bfloat16 widening and errors
    are those of `viterbi_decode`.  Returns (scores [B], path [B,T] int64 labels, tokens [B,T] int64, token_lengths [B] int64,
    states [B,T] int64: the automaton state after every frame); integer outputs are padded with -1, and an utterance of
    length 0 or without a finite path has score -inf, all -1 and no tokens.  With a one-state automaton of zero weights
    and token_score = 0 the first four equal `viterbi_decode` bit for bit.

    The graph is compiled for the device, dtype, lm_weight and token_score on first use and cached on it; later calls copy
    nothing to the device and do not synchronise, so they can be captured.  The batch is decoded in consecutive groups of
    utterances whose workspace (int32 back-pointers, T * Q * 4 bytes per utterance) fits `max_work_bytes`.
    """
    with torch.no_grad():
        return native().viterbi_decode_graph(*_plain(inputs, transition), graph, input_lengths, lm_weight, token_score,
                                             max_work_bytes)


def beam_decode_graph(inputs, transition, graph, input_lengths=None, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                      token_score=0.0, max_work_bytes=1 << 30):
    """Beam-pruned Viterbi decoding over the ASG lattice composed with a token automaton `graph`: `viterbi_decode_graph` that
    keeps at most `beam_size` product states per frame, so the work per frame follows the beam and its outgoing arcs and not
    the size of the automaton -- the decoder for large automata (`TokenGraph.from_lexicon`, high-order n-grams).  No gradient.

    The search is specified exactly (include/asg_hip.h::asg_beam_decode_graph).  The candidates of a frame come only from the
    states kept at the frame before; each target keeps its largest candidate (the smallest source index on a tie); with m the
    largest of the frame's values, the states kept are the first `beam_size` in (value descending, product-state index
    ascending) order whose value is >= m - beam_threshold.  The score is the largest value + final weight over the states kept at
    the last frame.  Arithmetic, folding of lm_weight / token_score, inputs, strides, float16 / bfloat16 widening, outputs,
    padding and errors are those of `viterbi_decode_graph`; with beam_size >= the number of product states and beam_threshold =
    inf every output equals it bit for bit.  Otherwise the score is <= the exact one and, when finite, exactly the score of the
    returned path; an utterance whose beam dies out, or ends in no accepting state, has score -inf, all -1 and no tokens.
    Results are bit-identical run to run.  beam_size < 1 and a negative or NaN beam_threshold raise ValueError.

    The graph is compiled for the device, dtype, lm_weight and token_score on first use and cached on it; later calls copy
    nothing to the device and do not synchronise, so they can be captured.  The batch is decoded in consecutive groups of
    utterances whose workspace (about T * beam_size * 8 bytes of back-pointers plus 12-16 bytes per product state and
    utterance) fits `max_work_bytes`.
    """
    _check_beam(beam_size, beam_threshold)
    with torch.no_grad():
        return native().beam_decode_graph(*_plain(inputs, transition), graph, input_lengths, beam_size, beam_threshold, lm_weight,
                                          token_score, max_work_bytes)


BeamGraphConfidence = collections.namedtuple("BeamGraphConfidence", ["scores", "path", "tokens", "token_lengths", "states",
                                                                     "token_frames", "token_confidences", "normalisers"])


def beam_decode_graph_confidence(inputs, transition, graph, input_lengths=None, beam_size=256, beam_threshold=float("inf"),
                                 lm_weight=1.0, token_score=0.0, frame_tolerance=0, max_work_bytes=1 << 30):
    """`beam_decode_graph` that also says where every token of its hypothesis starts and how sure the search is of it: what
    pseudo-label filters, highlighting of doubtful characters and token time stamps need beside the tokens.  No gradient.

    The search is `beam_decode_graph`'s, run once.  The sets of product states it kept span a lattice (the one
    `beam_graph_full_score` sums without targets); a lattice path starts a token with label i at frame t when it stands in a
    state with that label at t = 0, or takes an edge (anything but the stay) into such a state at t >= 1.  P(i, t) is the share
    of the lattice's probability mass, exp(weight - Z_K), on the paths with that event, whatever their automaton state
    (include/asg_hip.h::asg_beam_graph_confidence).  -> BeamGraphConfidence: the five tensors of `beam_decode_graph`, bit for
    bit, and
      token_frames      [B, T] int64  the frame s_k at which token k of the hypothesis starts, -1 behind the tokens
      token_confidences [B, T] dtype  the sum of P(tokens[k], t) over |t - s_k| <= frame_tolerance, 0 behind the tokens
      normalisers       [B]    dtype  Z_K, bit-equal to `beam_graph_full_score` without targets
    With frame_tolerance = 0 a confidence is a probability, between exp(scores - normalisers) and 1 up to rounding.  With a
    tolerance it is the expected number of starts of that label inside the window: it can pass 1 ("a b a" inside one window)
    and is returned unclipped.  With a `TokenGraph.from_lexicon` graph the confidence of a separator token is the confidence of
    a word boundary.  A narrow beam keeps little competing mass, so its confidences are high: they are posteriors given what
    the search kept.  Utterances without a path have score and normaliser -inf, integer outputs -1 and confidences 0; there is
    never a NaN.  frame_tolerance < 0 or > 64 is refused by the library (RuntimeError).

    Results are bit-identical run to run and for any `max_work_bytes`; inputs, widening, caching, capture and the utterance
    groups are those of `beam_decode_graph` (the graph is compiled once more, for `beam_graph_full_score`'s kernels, and cached
    on it), with a workspace about T * beam_size * (12 + 4 or 8) bytes per utterance (back-pointers, the sorted sets and alpha)
    plus the search's 12-16 bytes per product state.
    """
    _check_beam(beam_size, beam_threshold)
    with torch.no_grad():
        return native().beam_decode_graph_confidence(*_plain(inputs, transition), graph, input_lengths, beam_size, beam_threshold,
                                                     lm_weight, token_score, frame_tolerance, max_work_bytes)


BeamWords = collections.namedtuple("BeamWords", ["scores", "path", "tokens", "token_lengths", "states", "lm_states", "words",
                                                 "word_lengths"])


def beam_decode_words(inputs, transition, lexicon, word_lm, input_lengths=None, beam_size=256, beam_threshold=float("inf"),
                      lm_weight=1.0, word_score=0.0, token_score=0.0, max_work_bytes=1 << 30, lookahead=None):
    """Beam decoding over the ASG lattice composed with a `Lexicon` and a word n-gram LM (`WordLM`), the LM composed on the fly:
    the decoder for letter models with a word-level language model.  No gradient.

    The search is `beam_decode_graph`'s over pairs (LM history h, product state q of `lexicon.graph`) that exist only while the
    search holds them, so nothing is sized by the vocabulary, the LM or their product.  Inside a word the history stays; the
    separator edge out of a word-end node walks the LM for that word -- backing off while the history has no arc for it, adding
    lm_weight * bow per step, then lm_weight * logp + word_score -- and moves to the arc's next history.  The end adds
    lm_weight * log p(</s> | h), after one more LM step when the path ends in a word-end node without its separator; a path
    that ends mid-word does not count.  Every rule of `beam_decode_graph` holds with "pair order" (h, then q) in place of the
    product-state index; the specification is include/asg_hip.h::asg_beam_decode_words.  token_score is added per token as in
    `beam_decode_graph` (the lexicon graph is compiled with lm_weight 1, so `word_scores` of the lexicon count once).
    Arithmetic is in the dtype of the emissions, weights folded on the host; float16 / bfloat16 emissions are widened to the
    dtype of `transition`.  Results are bit-identical run to run.

    Returns BeamWords(scores [B], path [B,T], tokens [B,T], token_lengths [B], states [B,T], lm_states [B,T], words [B,T],
    word_lengths [B]): path, tokens, token_lengths and states as `beam_decode_graph`; lm_states the LM history at every frame;
    words the word ids of the path in order, padded with -1.  An utterance of length 0, one whose beam dies out, or one
    without a finite end has score -inf, every integer output -1 and no tokens or words.  beam_size < 1 and a negative or NaN
    beam_threshold raise ValueError; beam_size > 8192 is refused by the library (there is no clamp: pairs are not bounded by the
    number of product states).

    Lexicon and LM are compiled for the device, dtype and weights on first use and cached on them; later calls copy nothing to
    the device and do not synchronise, so they can be captured.  The batch is decoded in consecutive groups of utterances whose
    workspace (about T * beam_size * 12 bytes of back-pointers plus 60-80 bytes per candidate a frame can have, beam_size *
    (largest out-degree + 1)) fits `max_work_bytes`.

    `lookahead`, a `WordLookahead(lexicon, word_lm, order)`, adds LM look-ahead: inside a word a pair's value also carries the
    best LM score any word below its trie node can get after the history (the history truncated to `order`), so that a narrow
    beam ranks partial words by more than acoustics; a node below which the LM accepts no word is pruned when it is entered.
    The term is taken back when the word ends, so a complete hypothesis sums the same terms as without it: with a beam that
    prunes nothing the result is the same path, and the score differs only by the rounding of terms that cancel
    (include/asg_hip.h::asg_beam_decode_words_la).  None is the search without it, byte for byte.  The word streams and
    `beam_decode_words_nbest` take the same keyword.
    """
    _check_beam(beam_size, beam_threshold)
    with torch.no_grad():
        return native().beam_decode_words(*_plain(inputs, transition), lexicon, word_lm, input_lengths, beam_size, beam_threshold,
                                          lm_weight, word_score, token_score, max_work_bytes, lookahead)


BeamWordsConfidence = collections.namedtuple("BeamWordsConfidence", BeamWords._fields + ("word_frames", "word_confidences",
                                                                                       "normalisers"))


def beam_decode_words_confidence(inputs, transition, lexicon, word_lm, input_lengths=None, beam_size=256,
                                 beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0, frame_tolerance=0,
                                 max_work_bytes=1 << 30, lookahead=None):
    """`beam_decode_words` that also says where every word of its hypothesis ends and how sure the search is of it: what
    captions, keyword hits and pseudo-labels need beside the words.  No gradient.

    The search is `beam_decode_words`', run once.  The sets of pairs it kept span a lattice (the one `beam_words_full_score`
    sums without targets); a lattice path completes word w at frame t when it takes a separator edge out of a word-end node of
    w into frame t, or, at t = len, when it ends in such a node.  P(w, t) is the share of the lattice's probability mass,
    exp(weight - Z_K), on the paths with that event, whatever their LM history
    (include/asg_hip.h::asg_beam_words_confidence).  -> BeamWordsConfidence: the eight fields of `BeamWords`, bit for bit, and
      word_frames      [B, T] int64  the frame t_k at which word k of the hypothesis ends (len for a word ended by the end of
                                     the utterance), -1 behind the words
      word_confidences [B, T] dtype  the sum of P(words[k], t) over |t - t_k| <= frame_tolerance, 0 behind the words
      normalisers      [B]    dtype  Z_K, bit-equal to `beam_words_full_score` without targets
    With frame_tolerance = 0 a confidence is a probability, between exp(scores - normalisers) and 1 up to rounding.  With a
    tolerance it is the expected number of completions of the word inside the window: it can pass 1 where a path completes a
    short word twice within it, and is returned unclipped.  A narrow beam keeps little competing mass, so its confidences are
    high: they are posteriors given what the search kept.  Utterances without a path have score and normaliser -inf, integer
    outputs -1 and confidences 0; there is never a NaN.  frame_tolerance < 0 or > 64 is refused by the library (RuntimeError).

    Results are bit-identical run to run and for any `max_work_bytes`; inputs, widening, caching, capture and the utterance
    groups are those of `beam_decode_words`, with a workspace about T * beam_size * (24 + 8 or 16) bytes per utterance.
    `lookahead` takes the sets and the hypothesis of `beam_decode_words(..., lookahead=)`; the lattice keeps the plain weights,
    as `beam_words_full_score(..., lookahead=)` does.
    """
    _check_beam(beam_size, beam_threshold)
    with torch.no_grad():
        return native().beam_decode_words_confidence(*_plain(inputs, transition), lexicon, word_lm, input_lengths, beam_size,
                                                     beam_threshold, lm_weight, word_score, token_score, frame_tolerance,
                                                     max_work_bytes, lookahead)


BeamWordsNbest = collections.namedtuple("BeamWordsNbest", ["scores", "emission_scores", "graph_scores", "lm_scores", "tokens",
                                                           "token_lengths", "words", "word_lengths", "num_hyps", "path", "states",
                                                           "lm_states"])


def beam_decode_words_nbest(inputs, transition, lexicon, word_lm, input_lengths=None, beam_size=256, nbest=10,
                            beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0, return_alignments=False,
                            max_work_bytes=1 << 30, lookahead=None):
    """The `nbest` best hypotheses of `beam_decode_words`' search, each with its words and its score split into the acoustic
    part (emissions and transitions), the lexicon part (automaton weights, token_score, final weight) and the LM part (every
    LM step and the end of the sentence, lm_weight and word_score folded in): what n-best rescoring with a stronger LM and the
    tuning of lm_weight / word_score without decoding again need.  No gradient.

    The search is `beam_decode_words`', unchanged.  The pairs kept at the last frame are ranked by their end (descending, pair
    order -- LM history, then product state -- on a tie) and the first `nbest` with a finite end are returned, each with the
    best path the pruned search found for it (include/asg_hip.h::asg_beam_decode_words_nbest).  -> a named tuple
      scores, emission_scores, graph_scores, lm_scores  [B, nbest]     dtype of the emissions; -inf in the padding rows
      tokens, words                                     [B, nbest, T]  int64, -1 behind the data
      token_lengths, word_lengths                       [B, nbest]     int64
      num_hyps                                          [B]            int64, min(nbest, pairs with a finite end)
      path, states, lm_states                           [B, nbest, T]  int64 per frame with `return_alignments`, else None
    Row 0 equals `beam_decode_words`' result bit for bit.  `scores` is the search's own sum; the three parts add the same terms
    in another order and agree with it to rounding; lm_scores = lm_weight * (raw LM score) + word_score * word_lengths up to
    rounding.  Lexicon and LM are deterministic, so the rows are distinct token sequences; the same WORD sequence can appear
    twice, with and without a closing separator -- the better one comes first, rows are not merged.  Inputs, widening, caching,
    capture and the utterance groups under `max_work_bytes` are those of `beam_decode_words`.  nbest < 1 raises ValueError,
    nbest > 8192 RuntimeError; nbest > beam_size only adds padding rows.

    `lookahead`, a `WordLookahead(lexicon, word_lm, order)`, ranks the list of `beam_decode_words(..., lookahead=)`'s search
    (include/asg_hip.h::asg_beam_decode_words_nbest_la): row 0 equals that call's result bit for bit, `scores` is that search's
    own end, and the three parts are the sums above, term for term -- no look-ahead term enters them, since every estimate the
    search adds is taken back before a path ends.  They mean what they mean without look-ahead and are re-weighted the same
    way; `scores` agrees with their sum up to the rounding of the terms that cancel.  The workspace is the same with and
    without it.  None is the call without it, byte for byte.
    """
    _check_beam(beam_size, beam_threshold)
    if int(nbest) < 1:
        raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
    with torch.no_grad():
        return native().beam_decode_words_nbest(*_plain(inputs, transition), lexicon, word_lm, input_lengths, beam_size, nbest,
                                                beam_threshold, lm_weight, word_score, token_score, return_alignments,
                                                max_work_bytes, lookahead)


BeamWordsNbestConfidence = collections.namedtuple("BeamWordsNbestConfidence", BeamWordsNbest._fields + (
    "word_frames", "word_confidences", "normalisers"))


def beam_decode_words_nbest_confidence(inputs, transition, lexicon, word_lm, input_lengths=None, beam_size=256, nbest=10,
                                       beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                       frame_tolerance=0, return_alignments=False, max_work_bytes=1 << 30, lookahead=None):
    """`beam_decode_words_nbest` that also says, for every word of EVERY row, where it ends and how sure the search is of it:
    what rescoring with a per-word posterior as a feature, confusion-network or ROVER-style combination of the rows and
    pseudo-labelling on the words the rows agree on need.  One search serves both.  No gradient.

    The quantity is `beam_decode_words_confidence`'s: P(w, t), the share of the kept lattice's probability mass on the paths
    that complete word w at frame t, does not depend on the hypothesis; a row only selects which (word, frame) cells are read
    (include/asg_hip.h::asg_beam_words_nbest_confidence).  -> BeamWordsNbestConfidence: the twelve fields of `BeamWordsNbest`,
    bit for bit (path, states and lm_states are None unless `return_alignments`), and
      word_frames      [B, nbest, T] int64  the frame at which word k of row r ends (len for a word ended by the end of the
                                            utterance), -1 behind the words and in the padding rows
      word_confidences [B, nbest, T] dtype  the sum of P(words[r][k], t) over |t - word_frames[r][k]| <= frame_tolerance, 0
                                            behind the words and in the padding rows
      normalisers      [B]           dtype  Z_K, bit-equal to `beam_words_full_score` without targets
    Row 0's frames and confidences are `beam_decode_words_confidence`'s, bit for bit, and rows that hold the same word ending
    at the same frame carry the same bits.  With frame_tolerance = 0 a confidence lies between exp(scores[r] - normalisers)
    and 1 up to rounding; with a tolerance it is an expected count, returned unclipped.  Utterances without a path have
    num_hyps 0, normaliser -inf, frames -1 and confidences 0; there is never a NaN.  frame_tolerance < 0 or > 64, nbest < 1
    or > 8192, and a min(nbest, beam_size) * (2 * frame_tolerance + 2) whose accumulators do not fit the LDS beside a frame's
    lattice set are refused by the library (RuntimeError).

    Results are bit-identical run to run and for any `max_work_bytes`; inputs, widening, caching, capture and the utterance
    groups are those of `beam_decode_words_nbest`.  `lookahead` takes the sets and the rows of
    `beam_decode_words_nbest(..., lookahead=)`; the lattice keeps the plain weights.
    """
    _check_beam(beam_size, beam_threshold)
    if int(nbest) < 1:
        raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
    with torch.no_grad():
        return native().beam_decode_words_nbest_confidence(*_plain(inputs, transition), lexicon, word_lm, input_lengths, beam_size,
                                                           nbest, beam_threshold, lm_weight, word_score, token_score,
                                                           frame_tolerance, return_alignments, max_work_bytes, lookahead)


BeamNbest = collections.namedtuple("BeamNbest", ["scores", "emission_scores", "graph_scores", "tokens", "token_lengths",
                                                 "num_hyps", "path", "states"])


def beam_decode_graph_nbest(inputs, transition, graph, input_lengths=None, beam_size=256, nbest=10, beam_threshold=float("inf"),
                            lm_weight=1.0, token_score=0.0, return_alignments=False, max_work_bytes=1 << 30):
    """The `nbest` best final hypotheses of `beam_decode_graph`'s search, each with its score split into the acoustic part
    (emissions and transitions) and the graph part (automaton weights, token_score and the final weight): what n-best
    rescoring with a stronger model and the tuning of lm_weight / token_score need.  No gradient.

    The search is `beam_decode_graph`'s, unchanged.  The token automaton is deterministic, so the states kept at the last
    frame carry different transcripts; they are ranked by value + final weight (descending, product-state index ascending on a
    tie) and the first `nbest` with a finite score are returned, each with the best path the pruned search found for it
    (include/asg_hip.h::asg_beam_decode_graph_nbest).  -> a named tuple
      scores, emission_scores, graph_scores  [B, nbest]     dtype of the emissions; -inf in the padding rows
      tokens                                 [B, nbest, T]  int64, -1 behind each transcript
      token_lengths                          [B, nbest]     int64
      num_hyps                               [B]            int64, min(nbest, final states with a finite score)
      path, states                           [B, nbest, T]  int64 label and automaton state per frame with `return_alignments`,
                                                            else None (they then take no memory)
    Row 0 equals `beam_decode_graph`'s result bit for bit.  `scores` is the search's own sum; emission_scores + graph_scores
    adds the same terms in another order and agrees with it to rounding.  Inputs, widening, caching, capture and the
    utterance groups under `max_work_bytes` are those of `beam_decode_graph`.  nbest < 1 raises ValueError, nbest > 8192
    RuntimeError.
    """
    _check_beam(beam_size, beam_threshold)
    if int(nbest) < 1:
        raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
    with torch.no_grad():
        return native().beam_decode_graph_nbest(*_plain(inputs, transition), graph, input_lengths, beam_size, nbest,
                                                beam_threshold, lm_weight, token_score, return_alignments, max_work_bytes)


BeamNbestConfidence = collections.namedtuple("BeamNbestConfidence",
                                             BeamNbest._fields + ("token_frames", "token_confidences", "normalisers"))


def beam_decode_graph_nbest_confidence(inputs, transition, graph, input_lengths=None, beam_size=256, nbest=10,
                                       beam_threshold=float("inf"), lm_weight=1.0, token_score=0.0, return_alignments=False,
                                       frame_tolerance=0, max_work_bytes=1 << 30):
    """`beam_decode_graph_nbest` that also says, for EVERY row of the list, where each token starts and how sure the search is of
    it: what rescoring with a per-token posterior, ROVER-style combination of the rows and pseudo-labelling on the tokens the
    rows agree on need -- from one search instead of `beam_decode_graph_nbest` plus `beam_decode_graph_confidence`, which
    would search twice and still give posteriors for row 0 only.  No gradient.

    Nothing is re-defined.  The search, the candidates, their order and `num_hyps` are `beam_decode_graph_nbest`'s; the lattice
    of the kept sets, the token events P(i, t) and Z_K are `beam_decode_graph_confidence`'s
    (include/asg_hip.h::asg_beam_graph_nbest_confidence).  P(i, t) does not depend on the hypothesis: a row only selects which
    (frame, label) cells are read.  -> BeamNbestConfidence: the eight fields of `BeamNbest`, bit for bit, and
      token_frames      [B, nbest, T] int64  the frame at which token k of row r starts, -1 behind the tokens and in padding rows
      token_confidences [B, nbest, T] dtype  the sum of P(tokens[r][k], t) over |t - frame| <= frame_tolerance, 0 there
      normalisers       [B]           dtype  Z_K, bit-equal to `beam_graph_full_score` without targets
    Row 0's frames and confidences are `beam_decode_graph_confidence`'s bit for bit; rows that start the same label at the same
    frame carry the same bits.  With frame_tolerance = 0 a confidence lies between exp(scores[r] - normalisers) and 1 up to
    rounding.  Utterances without a path have num_hyps 0, scores and normaliser -inf, frames -1 and confidences 0; there is
    never a NaN.  nbest < 1 raises ValueError; nbest > 8192, frame_tolerance outside 0 .. 64, and a combination of beam_size,
    nbest and frame_tolerance whose open cells do not fit the LDS beside a frame's lattice set
    (12 * P2(min(nbest, K) * (2 * frame_tolerance + 2)) bytes, see the header) are refused by the library (RuntimeError).

    Results are bit-identical run to run and for any `max_work_bytes`; inputs, widening, caching, capture and the utterance
    groups are those of `beam_decode_graph_confidence`, with min(nbest, K) * T * 28 bytes per utterance on top for the rows,
    their cells and the cells' sums.
    """
    _check_beam(beam_size, beam_threshold)
    if int(nbest) < 1:
        raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
    with torch.no_grad():
        return native().beam_decode_graph_nbest_confidence(*_plain(inputs, transition), graph, input_lengths, beam_size, nbest,
                                                           beam_threshold, lm_weight, token_score, return_alignments,
                                                           frame_tolerance, max_work_bytes)


class GraphFullScore(torch.autograd.Function):
    """Full score of the ASG lattice composed with a token automaton, [B] (asg_graph_full_forward / _backward).  alpha is
    stored only when a gradient w.r.t. inputs or transition is needed."""

    @staticmethod
    def forward(ctx, inputs, transition, graph, input_lengths, lm_weight, token_score, max_work_bytes, flags):
        store = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        scores, saved = native().graph_full_forward(inputs, transition, graph, input_lengths, lm_weight, token_score, store,
                                                    max_work_bytes, flags)
        ctx.save_for_backward(inputs, transition, input_lengths, scores)
        ctx.saved, ctx.graph, ctx.args = saved, graph, (lm_weight, token_score, flags)
        return scores

    @staticmethod
    def backward(ctx, grad):
        inputs, transition, input_lengths, scores = ctx.saved_tensors
        lw, ts, flags = ctx.args
        gtr, gin = native().graph_full_backward(ctx.saved, scores, grad, inputs, transition, ctx.graph, input_lengths, lw, ts,
                                                flags)
        return gin, gtr, None, None, None, None, None, None


def graph_full_score(inputs, transition, graph, input_lengths=None, lm_weight=1.0, token_score=0.0, max_work_bytes=1 << 30):
    """logsumexp over every label path of the ASG lattice composed with a token automaton `graph` (a `TokenGraph`): each path
    scores its emissions and transitions plus the automaton's score of its tokens (lm_weight * weight + token_score per token,
    lm_weight * final at the end; -inf if the automaton rejects them) -- the log-semiring counterpart of `viterbi_decode_graph`.
    Differentiable w.r.t. `inputs` and `transition` (the automaton, lm_weight and token_score are constants).  Returns [B] in the
    dtype of the emissions; -inf for an utterance of length 0 or without any accepted path.  Inputs, strides, widening of
    float16 / bfloat16 and the grouping under `max_work_bytes` (alpha, T * Q * e bytes per utterance when a gradient is
    needed) are those of `viterbi_decode_graph`."""
    return GraphFullScore.apply(_widen(inputs, transition), transition, graph, input_lengths, lm_weight, token_score,
                                max_work_bytes, 0)


def _guarded_targets(targets, target_lengths, N):
    """(targets with every label outside [0, N) replaced by 0, ok[B]): ok[b] is False where targets[b, :target_lengths[b]] holds
    such a label.  The force-aligned kernels index emissions and transitions with the label as given, so they only ever see the
    first; the caller turns the aligned score of an utterance with ok False into -inf.  On the device, no synchronisation."""
    outside = (targets < 0) | (targets >= N)
    pos = torch.arange(targets.shape[1], device=targets.device).unsqueeze(0) < target_lengths.to(targets.device).unsqueeze(1)
    return targets.masked_fill(outside, 0), ~(outside & pos).any(dim=1)


def _graph_loss(inputs, targets, transition, graph, input_lengths, target_lengths, lm_weight, token_score, max_work_bytes,
                reduction, beam=None, weights=None, words=None, lookahead=None):
    """What the graph losses share.  [B] losses full - (FAC + A(collapse(target))), then `weights(inputs, input_lengths,
    target_lengths)` (None: none) and the reduction; `full` is the exact normaliser (`GraphFullScore`), or with beam =
    (beam_size, beam_threshold) the beam-pruned one with the target forced into the lattice (`BeamGraphFullScore`).  With
    words = (word_lm, word_score), `graph` is a `Lexicon`, the normaliser runs over the pairs of `beam_decode_words`
    (`BeamWordsFullScore`; `beam` is required; with `lookahead` the pairs of `beam_decode_words(..., lookahead=)`) and A is
    the lexicon + LM score of the target (`words_target_scores`, which no look-ahead enters).  A loss is
    +inf (never NaN) where the target has no alignment, the automaton rejects it or it holds a label outside [0, N)
    (`_guarded_targets`), and then only the normaliser's posterior reaches the gradients.  Defaults, S > T truncation and
    widening as `ASGLoss.forward`."""
    inputs = _widen(inputs, transition)
    targets, input_lengths, target_lengths = ASGLoss._canonical(inputs, targets, input_lengths, target_lengths)
    if words is not None:
        full = BeamWordsFullScore.apply(inputs, transition, graph, words[0], input_lengths, *beam, lm_weight, words[1],
                                        token_score, targets, target_lengths, max_work_bytes, lookahead)
    elif beam is None:
        full = GraphFullScore.apply(inputs, transition, graph, input_lengths, lm_weight, token_score, max_work_bytes, 0)
    else:
        full = BeamGraphFullScore.apply(inputs, transition, graph, input_lengths, *beam, lm_weight, token_score, targets,
                                        target_lengths, max_work_bytes)
    with torch.no_grad():
        if words is not None:
            walk = native().words_target_scores(inputs.detach(), transition.detach(), graph, words[0], targets, target_lengths,
                                                lm_weight, words[1], token_score)
        else:
            walk = native().graph_target_scores(inputs.detach(), transition.detach(), graph, targets, target_lengths, lm_weight,
                                                token_score)
    safe, inside = _guarded_targets(targets, target_lengths, inputs.shape[2])
    aligned = FAC.apply(transition, inputs, safe, input_lengths, target_lengths) + walk
    aligned = torch.where(inside.to(aligned.device), aligned, torch.full_like(aligned, float("-inf")))
    fd, ad = full.detach(), aligned.detach()
    ok_f, ok_a = torch.isfinite(fd), torch.isfinite(ad)
    zero = torch.zeros_like(fd)
    value = torch.where(ok_a, fd - ad, torch.full_like(fd, float("inf")))
    # value carries the numbers; the two zero-valued terms carry the gradients, masked where a score is infinite
    per = value + torch.where(ok_f, full - fd, zero) - torch.where(ok_a, aligned - ad, zero)
    w = weights(inputs, input_lengths, target_lengths) if weights is not None else None
    if w is not None:
        per = per * w
    return _reduce(per, reduction)


def _reduce(per_utt, reduction):
    if reduction == 'mean':
        return per_utt.mean()
    if reduction == 'sum':
        return per_utt.sum()
    return per_utt


def graph_asg_loss(inputs, targets, transition, graph, input_lengths=None, target_lengths=None, lm_weight=1.0,
                   token_score=0.0, reduction='none', max_work_bytes=1 << 30):
    """ASG loss whose normaliser is the lattice composed with a token automaton `graph`:
    loss[b] = graph_full_score[b] - (S_aligned[b] + A(collapse(targets[b]))), where S_aligned is the force-aligned score (`FAC`)
    and A the automaton's score of the target with consecutive repeats merged.  exp(-loss) is the probability of the target
    under the composed model.  +inf where the target cannot be aligned (target_length > input_length, length 0) or the automaton
    rejects it, or it holds a label outside [0, N); those utterances' gradient rows hold only the full-graph posterior.
    Defaults and S > T truncation as `ASGLoss.forward`; reduction 'none' (default), 'sum' or 'mean'."""
    return _graph_loss(inputs, targets, transition, graph, input_lengths, target_lengths, lm_weight, token_score, max_work_bytes,
                       reduction)


class BeamGraphFullScore(torch.autograd.Function):
    """Beam-pruned full score of the ASG lattice composed with a token automaton, [B] (asg_beam_graph_full_forward /
    _backward).  The kept sets are constants of the gradient; alpha is stored only when a gradient w.r.t. inputs or transition
    is needed.  Once differentiable."""

    @staticmethod
    def forward(ctx, inputs, transition, graph, input_lengths, beam_size, beam_threshold, lm_weight, token_score, targets,
                target_lengths, max_work_bytes):
        store = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        scores, saved = native().beam_graph_full_forward(inputs, transition, graph, input_lengths, beam_size, beam_threshold,
                                                         lm_weight, token_score, targets, target_lengths, store, max_work_bytes)
        ctx.save_for_backward(inputs, transition, input_lengths, targets, target_lengths, scores)
        ctx.saved, ctx.graph, ctx.args = saved, graph, (beam_size, lm_weight, token_score)
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        inputs, transition, input_lengths, targets, target_lengths, scores = ctx.saved_tensors
        K, lw, ts = ctx.args
        gtr, gin = native().beam_graph_full_backward(ctx.saved, scores, grad, inputs, transition, ctx.graph, input_lengths, K, lw,
                                                     ts, targets, target_lengths)
        return (gin, gtr) + (None,) * 9


def beam_graph_full_score(inputs, transition, graph, input_lengths=None, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                          token_score=0.0, targets=None, target_lengths=None, max_work_bytes=1 << 30):
    """`graph_full_score` over the lattice that `beam_decode_graph`'s search keeps: the logsumexp over the label paths that
    stay, at every frame, inside the beam's active set of that frame (the sets of `beam_decode_graph` for the same arguments,
    bit for bit) -- and, when `targets` is given, inside those sets united with the product states every alignment of the
    target passes through (include/asg_hip.h::asg_beam_graph_full_forward).  Work and memory follow beam_size, not the size of
    the automaton.  Differentiable w.r.t. `inputs` and `transition` with the sets held constant; <= `graph_full_score`, equal to
    it when beam_size >= the number of product states and beam_threshold = inf; without targets >= `beam_decode_graph`'s score.
    Bit-identical run to run and for any `max_work_bytes`.  targets / target_lengths are taken as given (no defaults or
    truncation here: `beam_graph_asg_loss` applies those)."""
    _check_beam(beam_size, beam_threshold)
    return BeamGraphFullScore.apply(_widen(inputs, transition), transition, graph, input_lengths, beam_size, beam_threshold,
                                    lm_weight, token_score, targets, target_lengths, max_work_bytes)


def beam_graph_asg_loss(inputs, targets, transition, graph, input_lengths=None, target_lengths=None, beam_size=256,
                        beam_threshold=float("inf"), lm_weight=1.0, token_score=0.0, reduction='none', max_work_bytes=1 << 30):
    """`graph_asg_loss` with the beam-pruned normaliser: loss[b] = beam_graph_full_score[b] - (S_aligned[b] +
    A(collapse(targets[b]))), the target forced into the beam's lattice, so every finite loss is >= 0 (up to rounding) for any
    beam and equals `graph_asg_loss` once the beam holds every product state.  +inf exactly where `graph_asg_loss` is +inf -- no
    alignment, a target the automaton rejects, a label outside [0, N) within the target's length; then only the normaliser's
    posterior reaches the gradients.  Defaults and S > T truncation as `ASGLoss.forward`."""
    _check_beam(beam_size, beam_threshold)
    return _graph_loss(inputs, targets, transition, graph, input_lengths, target_lengths, lm_weight, token_score, max_work_bytes,
                       reduction, (beam_size, beam_threshold))


class BeamWordsFullScore(torch.autograd.Function):
    """Beam-pruned full score of the ASG lattice composed with a lexicon and a word LM over the pairs `beam_decode_words`
    keeps, [B] (asg_beam_words_full_forward / _backward) -- with `lookahead`, the pairs `beam_decode_words(..., lookahead=)`
    keeps (asg_beam_words_full_forward_la; the backward reads the stored lattice and does not need it).  The kept sets are
    constants of the gradient; alpha is stored only when a gradient w.r.t. inputs or transition is needed.  Once
    differentiable."""

    @staticmethod
    def forward(ctx, inputs, transition, lexicon, word_lm, input_lengths, beam_size, beam_threshold, lm_weight, word_score,
                token_score, targets, target_lengths, max_work_bytes, lookahead=None):
        store = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        scores, saved = native().beam_words_full_forward(inputs, transition, lexicon, word_lm, input_lengths, beam_size,
                                                         beam_threshold, lm_weight, word_score, token_score, targets,
                                                         target_lengths, store, max_work_bytes, lookahead)
        ctx.save_for_backward(inputs, transition, input_lengths, targets, target_lengths, scores)
        ctx.saved, ctx.words, ctx.args = saved, (lexicon, word_lm), (beam_size, lm_weight, word_score, token_score)
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        inputs, transition, input_lengths, targets, target_lengths, scores = ctx.saved_tensors
        K, lw, ws, ts = ctx.args
        gtr, gin = native().beam_words_full_backward(ctx.saved, scores, grad, inputs, transition, *ctx.words, input_lengths, K,
                                                     lw, ws, ts, targets, target_lengths)
        return (gin, gtr) + (None,) * 12


def beam_words_full_score(inputs, transition, lexicon, word_lm, input_lengths=None, beam_size=256, beam_threshold=float("inf"),
                          lm_weight=1.0, word_score=0.0, token_score=0.0, targets=None, target_lengths=None,
                          max_work_bytes=1 << 30, lookahead=None):
    """`beam_graph_full_score` over the pairs (LM history, lexicon product state) that `beam_decode_words`' search keeps: the
    logsumexp over the label paths whose pair stays, at every frame, inside the kept set of that frame (the sets of
    `beam_decode_words` for the same arguments without look-ahead, bit for bit) -- and, when `targets` is given, inside those
    sets united with the pairs every alignment of the target passes through (include/asg_hip.h::asg_beam_words_full_forward).
    A path's score is `beam_decode_words`': emissions, transitions, the lexicon's weights, the LM walk of every word and the
    end of the sentence.  Work and memory follow beam_size, never the sizes of the lexicon or the LM.  Differentiable w.r.t.
    `inputs` and `transition` with the sets held constant; without targets >= `beam_decode_words`' score.  Bit-identical run to
    run and for any `max_work_bytes`.  targets / target_lengths are taken as given (`beam_words_asg_loss` applies defaults and
    truncation).

    With `lookahead`, a `WordLookahead(lexicon, word_lm, order)`, the sets are those of `beam_decode_words(..., lookahead=)`
    for the same arguments, bit for bit (asg_beam_words_full_forward_la): the lattice a look-ahead decoder searches at test
    time.  Only the sets change: a path's score stays the plain one above -- along a complete path the look-ahead terms cancel
    -- so without targets the score is >= the plain score of the look-ahead decoder's best path, which is that call's score up
    to the rounding of the cancelling terms.  Work and memory are unchanged; the look-ahead is compiled with the call's
    lm_weight and word_score through its cache, so a warm call copies nothing."""
    _check_beam(beam_size, beam_threshold)
    return BeamWordsFullScore.apply(_widen(inputs, transition), transition, lexicon, word_lm, input_lengths, beam_size,
                                    beam_threshold, lm_weight, word_score, token_score, targets, target_lengths, max_work_bytes,
                                    lookahead)


def beam_words_asg_loss(inputs, targets, transition, lexicon, word_lm, input_lengths=None, target_lengths=None, beam_size=256,
                        beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0, reduction='none',
                        max_work_bytes=1 << 30, lookahead=None):
    """ASG loss against what `beam_decode_words` searches (without look-ahead, bit for bit; with `lookahead`, a
    `WordLookahead`, what `beam_decode_words(..., lookahead=)` searches): loss[b] = beam_words_full_score[b] - (S_aligned[b] +
    the lexicon + LM score of targets[b] with consecutive repeats merged), the target forced into the beam's lattice, so every
    finite loss is >= 0 (up to rounding) for any beam, with or without look-ahead.  `targets` are token labels that spell words of the lexicon, each followed by the
    separator or ending the sequence.  +inf (never NaN) where the target cannot be aligned, the lexicon or the LM rejects it,
    it ends mid-word, or it holds a label outside [0, N) within its length; then only the normaliser's posterior reaches the
    gradients.  Defaults and S > T truncation as `ASGLoss.forward`; reduction 'none' (default), 'sum' or 'mean'."""
    _check_beam(beam_size, beam_threshold)
    return _graph_loss(inputs, targets, transition, lexicon, input_lengths, target_lengths, lm_weight, token_score,
                       max_work_bytes, reduction, (beam_size, beam_threshold), None, (word_lm, word_score), lookahead)


class FAC(torch.autograd.Function):
    """Force-aligned lattice score S_aligned[b]; same signature as the reference's FAC (asg.py:7-34)."""

    @staticmethod
    def forward(ctx, transition, inputs, targets, input_lengths, target_lengths):
        scores, state = native().aligned_forward(inputs, targets, transition, input_lengths, target_lengths)
        ctx.save_for_backward(state, inputs, targets, input_lengths, target_lengths, transition)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        state, inputs, targets, input_lengths, target_lengths, transition = ctx.saved_tensors
        grad_transition, grad_inputs = native().aligned_backward(state, grad_out, inputs, targets, transition,
                                                                 input_lengths, target_lengths)
        return grad_transition, grad_inputs, None, None, None


class FCC(torch.autograd.Function):
    """Fully-connected lattice score S_full[b]; same signature as the reference's FCC (asg.py:37-55)."""

    @staticmethod
    def forward(ctx, transition, inputs, targets, input_lengths, target_lengths):
        scores, state = native().full_forward(inputs, transition, input_lengths)
        ctx.save_for_backward(state, inputs, input_lengths, transition)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        state, inputs, input_lengths, transition = ctx.saved_tensors
        grad_transition, grad_inputs = native().full_backward(state, grad_out, inputs, transition, input_lengths)
        return grad_transition, grad_inputs, None, None, None


class ASGGPUFastForwardOnly(torch.autograd.Function):
    """beta-only evaluation route (asg.py:58-68): returns full - aligned, no gradient."""

    @staticmethod
    def forward(ctx, inputs, outputs, transition, input_lengths, output_lengths, flags=_lib.FLAG_STREAMS):
        full, aligned = native().forward_only(inputs, outputs, transition, input_lengths, output_lengths, flags)
        result = full - aligned
        ctx.mark_non_differentiable(result)
        return result

    @staticmethod
    def backward(ctx, *grad_outputs):
        return None


class ASGGPUFast(torch.autograd.Function):
    """Fused training route (asg.py:71-97): (full_scores, aligned_scores), gradients assembled non-recursively."""

    @staticmethod
    def forward(ctx, inputs, transition, outputs, input_lengths, output_lengths, flags=_lib.FLAG_STREAMS):
        full, aligned, state = native().forward(inputs, outputs, transition, input_lengths, output_lengths, flags)
        ctx.save_for_backward(state, inputs, outputs, input_lengths, output_lengths, transition)
        return full, aligned

    @staticmethod
    def backward(ctx, grad_full, grad_aligned):
        state, inputs, outputs, input_lengths, output_lengths, transition = ctx.saved_tensors
        grad_transition, grad_inputs = native().backward(state, grad_full, grad_aligned, inputs, outputs, transition,
                                                         input_lengths, output_lengths)
        return grad_inputs, grad_transition, None, None, None, None


class ASGLossFunction(torch.autograd.Function):
    """The whole criterion in one Function: loss = reduce(full - aligned) (asg.py:128,136-142) with the subtraction,
    the reduction and their gradients done inside the kernels (no PyTorch glue launches).

    On the fused route (launch mode 'single', float32, N < 64, S <= 64) forward ALSO assembles the gradients for an
    upstream gradient of 1 -- the reference's "no recursion in backward" (README.md:17-20) taken one step further --
    and backward is one small launch that multiplies by the actual upstream gradient and reduces the per-utterance
    transition-gradient tiles."""

    @staticmethod
    def forward(ctx, inputs, transition, outputs, input_lengths, output_lengths, reduction, flags):
        be = native()
        r = None
        bd = getattr(be, "binding", None)
        if inputs.dim() == 3 and inputs.shape[2] > 256:
            be.check_faults()            # (resident-slice route: a launch that timed out was repaired in stream; say that the route is gone)
        if bd is not None:
            # the plain case (everything on the device, contiguous lengths) entirely in C++; None = not that case
            r = bd.try_loss_forward(inputs, transition, outputs, input_lengths, output_lengths,
                                    HipBackend._RED[reduction], flags)
        if r is not None:
            loss, mode, buf0, buf1, sc_bytes, state_bytes, fs = r
            saved = _Saved("fused" if mode else "split", (buf0, buf1) if mode else (buf0,), None, None,
                           (sc_bytes, state_bytes, fs))
            saved.rec = (mode, sc_bytes, state_bytes, fs, HipBackend._RED[reduction])
        else:
            # The problem block built by loss_forward is reused by loss_backward: everything it points at must be one of
            # the tensors autograd saves.  CPU (the reference accepts them on its GPU route, streamlined_fast_gpu.cpp:40)
            # or strided lengths / targets are therefore converted HERE, and the converted tensors are the saved ones.
            outputs, input_lengths, output_lengths = HipBackend.device_args(inputs.device, outputs, input_lengths, output_lengths)
            loss, saved = be.loss_forward(inputs, outputs, transition, input_lengths, output_lengths, reduction, flags)
        ctx.save_for_backward(inputs, outputs, input_lengths, output_lengths, transition, *saved.tensors)
        saved.tensors = None          # autograd owns them now (and frees them after backward)
        saved.keep = None             # (every tensor the block points at is in ctx.saved_tensors)
        ctx.reduction = reduction
        ctx.flags = flags
        ctx.saved = saved
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        inputs, outputs, input_lengths, output_lengths, transition, *tensors = ctx.saved_tensors
        be = native()
        saved = ctx.saved
        if saved.consumed and saved.mode == "fused":
            # backward through a retained graph a second time: the gradient buffers of the first pass were handed to
            # autograd (and rescaled in place), so the step is recomputed
            with torch.no_grad():
                _, saved = be.loss_forward(inputs, outputs, transition, input_lengths, output_lengths, ctx.reduction,
                                           ctx.flags)
            tensors = saved.tensors
        r = None
        bd = getattr(be, "binding", None)
        if bd is not None:
            rec = saved.rec
            if rec is None:             # the forward ran in Python: same buffers, same sizes
                rec = (1,) + saved.sizes if saved.mode == "fused" else (0, 0, 0, 0)
                rec += (HipBackend._RED[ctx.reduction],)
            r = bd.try_loss_backward(rec, tensors[0], tensors[1] if rec[0] else None, grad_loss, inputs, transition,
                                     outputs, input_lengths, output_lengths)
        if r is None:
            r = be.loss_backward(saved, tensors, grad_loss, inputs, outputs, transition, input_lengths, output_lengths,
                                 ctx.reduction)
        grad_transition, grad_inputs = r
        ctx.saved.consumed = True
        return grad_inputs, grad_transition, None, None, None, None, None


class ASGLoss(nn.Module):
    """Auto Segmentation Criterion.  Constructor arguments, `forward` signature, the `transition` parameter and the
    routing between the serial / evaluation / training implementations follow the reference module
    (/root/reference/torch_asg/asg.py:100-142) so that checkpoints and call sites carry over unchanged.

    Extra, optional keyword arguments (not in the reference):
      launch_mode  how the fused route issues the four recursions --
        'single' (default)   ONE kernel launch: all four recursions are co-resident, which is the overlap the reference
                             builds from 4 CUDA streams (streamlined_fast_gpu.cpp:121-129); measured fastest on MI355X
        'streams'            full-lattice and force-aligned passes on two HIP streams with event fork/join
        'serial'             two launches on the caller's stream
      scale_mode   the wav2letter criterion scaling that the reference dropped (README.md:93-94, vestiges at
                   test_asg.py:169-173): every utterance's loss is multiplied by 1/len or 1/sqrt(len) of its input or
                   target before the reduction -- 'none' (default, = the reference), 'input_size', 'input_size_sqrt',
                   'target_size', 'target_size_sqrt' (SURVEY.md 8(f)4).
      input_is_logits   the acoustic model's final `log_softmax` fused away: pass the UNNORMALISED
                   logits and get the loss and gradients of `ASGLoss(...)(log_softmax(inputs, dim=2), ...)` without the
                   [T,B,N] round trips of that op and of its backward.  No kernel has anything to do for it: shifting
                   every emission of a frame by the same amount (here -logsumexp of the frame) shifts the full-lattice
                   and the force-aligned score of every path through that frame by that amount, so `full - aligned` does
                   not change; and the gradient of the loss w.r.t. the log-probabilities sums to 0 over the labels of
                   every frame (both posteriors sum to 1), so the softmax Jacobian's correction term vanishes and
                   d loss / d logits = d loss / d log-probs.  The flag records the caller's intent and is what the
                   parity test pins (tests/test_hip_parity.py::test_input_is_logits); the individual scores returned by
                   FCC / FAC are NOT shift-invariant and take log-probabilities as in the reference.
                   EXCEPTION: an utterance with target_length > input_length has no alignment: its loss is +inf and, as
                   in the reference, its `inputs.grad` rows hold only the full-lattice posterior (they sum to the
                   upstream gradient g, not to 0), so for that utterance d loss / d logits differs from what autograd
                   through log_softmax would give by softmax * g (tests/test_hip_host.py pins this).
    bfloat16 `inputs` (with the float32 `transition`): "bf16 in, fp32 accumulate"  -- the fused training step
    reads them as they are and returns a bfloat16 `inputs.grad`; every other route widens them first.  float16 `inputs` are
    always widened to the dtype of `transition` (and `inputs.grad` comes back as float16 through autograd's cast).  The loss and
    `transition.grad` are float32 and match a float32 run on the same (bf16-representable) values to 1e-4; `inputs.grad`
    is rounded to bfloat16 on store (8 bits of mantissa: 4e-3 relative).
    `gpu_no_stream_impl=True` selects the reference's "serial" route (separate FAC and FCC Functions).
    Batch-major activations need no copy: pass `acts.transpose(0, 1)` ([B,T,N] -> a [T,B,N] view); the kernels take
    arbitrary strides.
    """
    SCALE_MODES = ('none', 'input_size', 'input_size_sqrt', 'target_size', 'target_size_sqrt')
    _LAUNCH_FLAGS = {'streams': _lib.FLAG_STREAMS, 'single': _lib.FLAG_SINGLE_LAUNCH, 'serial': 0}

    def __init__(self, num_labels, reduction='mean', forward_only=False, gpu_no_stream_impl=False,
                 launch_mode='single', scale_mode='none', input_is_logits=False):
        super().__init__()
        if scale_mode not in self.SCALE_MODES:
            raise ValueError("scale_mode must be one of %s" % (self.SCALE_MODES,))
        if launch_mode not in self._LAUNCH_FLAGS:
            raise ValueError("launch_mode must be one of %s" % (tuple(self._LAUNCH_FLAGS),))
        self.num_labels = num_labels
        self.reduction = reduction
        self.forward_only = forward_only
        self.gpu_no_stream_impl = gpu_no_stream_impl
        self.launch_mode = launch_mode
        self.scale_mode = scale_mode
        self.input_is_logits = bool(input_is_logits)
        # transition[i, j] scores the move from label j to label i; starts at zero like the reference's (asg.py:105)
        self.transition = nn.Parameter(torch.zeros(num_labels, num_labels))

    def _flags(self):
        return self._LAUNCH_FLAGS[self.launch_mode]

    def viterbi_align(self, inputs, targets, input_lengths=None, target_lengths=None):
        """Best-path force alignment under this module's transition matrix: see `torch_asg_amd.viterbi_align`."""
        return viterbi_align(inputs, targets, self.transition, input_lengths, target_lengths)

    def viterbi_decode(self, inputs, input_lengths=None):
        """Viterbi decoding under this module's transition matrix: see `torch_asg_amd.viterbi_decode`."""
        return viterbi_decode(inputs, self.transition, input_lengths)

    def viterbi_decode_graph(self, inputs, graph, input_lengths=None, lm_weight=1.0, token_score=0.0, max_work_bytes=1 << 30):
        """Viterbi decoding with a token automaton under this module's transition matrix: see
        `torch_asg_amd.viterbi_decode_graph`."""
        return viterbi_decode_graph(inputs, self.transition, graph, input_lengths, lm_weight, token_score, max_work_bytes)

    def beam_decode_graph(self, inputs, graph, input_lengths=None, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                          token_score=0.0, max_work_bytes=1 << 30):
        """Beam-pruned decoding under this criterion's transitions composed with a token automaton; see
        `torch_asg_amd.beam_decode_graph`."""
        return beam_decode_graph(inputs, self.transition, graph, input_lengths, beam_size, beam_threshold, lm_weight, token_score,
                                 max_work_bytes)

    def beam_decode_graph_confidence(self, inputs, graph, input_lengths=None, beam_size=256, beam_threshold=float("inf"),
                                     lm_weight=1.0, token_score=0.0, frame_tolerance=0, max_work_bytes=1 << 30):
        """`beam_decode_graph` under this criterion's transitions with the start frame and the lattice posterior of every token;
        see `torch_asg_amd.beam_decode_graph_confidence`."""
        return beam_decode_graph_confidence(inputs, self.transition, graph, input_lengths, beam_size, beam_threshold, lm_weight,
                                            token_score, frame_tolerance, max_work_bytes)

    def beam_decode_words(self, inputs, lexicon, word_lm, input_lengths=None, beam_size=256, beam_threshold=float("inf"),
                          lm_weight=1.0, word_score=0.0, token_score=0.0, max_work_bytes=1 << 30, lookahead=None):
        """Beam decoding with a lexicon and a word n-gram LM under this criterion's transitions; see
        `torch_asg_amd.beam_decode_words`."""
        return beam_decode_words(inputs, self.transition, lexicon, word_lm, input_lengths, beam_size, beam_threshold, lm_weight,
                                 word_score, token_score, max_work_bytes, lookahead)

    def beam_decode_words_confidence(self, inputs, lexicon, word_lm, input_lengths=None, beam_size=256,
                                     beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                     frame_tolerance=0, max_work_bytes=1 << 30, lookahead=None):
        """`beam_decode_words` under this criterion's transitions with the end frame and the lattice posterior of every word;
        see `torch_asg_amd.beam_decode_words_confidence`."""
        return beam_decode_words_confidence(inputs, self.transition, lexicon, word_lm, input_lengths, beam_size, beam_threshold,
                                            lm_weight, word_score, token_score, frame_tolerance, max_work_bytes, lookahead)

    def beam_decode_words_nbest_confidence(self, inputs, lexicon, word_lm, input_lengths=None, beam_size=256, nbest=10,
                                           beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                           frame_tolerance=0, return_alignments=False, max_work_bytes=1 << 30, lookahead=None):
        """`beam_decode_words_nbest` under this criterion's transitions with the end frame and the lattice posterior of every
        word of every row; see `torch_asg_amd.beam_decode_words_nbest_confidence`."""
        return beam_decode_words_nbest_confidence(inputs, self.transition, lexicon, word_lm, input_lengths, beam_size, nbest,
                                                  beam_threshold, lm_weight, word_score, token_score, frame_tolerance,
                                                  return_alignments, max_work_bytes, lookahead)

    def beam_decode_words_nbest(self, inputs, lexicon, word_lm, input_lengths=None, beam_size=256, nbest=10,
                                beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0,
                                return_alignments=False, max_work_bytes=1 << 30, lookahead=None):
        """The n best hypotheses of `beam_decode_words` under this module's transitions, with the score split: see
        `torch_asg_amd.beam_decode_words_nbest`."""
        return beam_decode_words_nbest(inputs, self.transition, lexicon, word_lm, input_lengths, beam_size, nbest, beam_threshold,
                                       lm_weight, word_score, token_score, return_alignments, max_work_bytes, lookahead)

    def beam_decode_graph_nbest(self, inputs, graph, input_lengths=None, beam_size=256, nbest=10, beam_threshold=float("inf"),
                                lm_weight=1.0, token_score=0.0, return_alignments=False, max_work_bytes=1 << 30):
        """The n best hypotheses of the beam search under this criterion's transitions, with their score split; see
        `torch_asg_amd.beam_decode_graph_nbest`."""
        return beam_decode_graph_nbest(inputs, self.transition, graph, input_lengths, beam_size, nbest, beam_threshold, lm_weight,
                                       token_score, return_alignments, max_work_bytes)

    def beam_decode_graph_nbest_confidence(self, inputs, graph, input_lengths=None, beam_size=256, nbest=10,
                                           beam_threshold=float("inf"), lm_weight=1.0, token_score=0.0, return_alignments=False,
                                           frame_tolerance=0, max_work_bytes=1 << 30):
        """The n best hypotheses under this criterion's transitions with the start frame and the lattice posterior of every
        token of every row; see `torch_asg_amd.beam_decode_graph_nbest_confidence`."""
        return beam_decode_graph_nbest_confidence(inputs, self.transition, graph, input_lengths, beam_size, nbest, beam_threshold,
                                                  lm_weight, token_score, return_alignments, frame_tolerance, max_work_bytes)

    def beam_stream(self, graph, batch_size, max_frames, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                    token_score=0.0, keep_lattice=False):
        """A streaming beam decoder under this module's transition matrix (read again at every chunk): see
        `torch_asg_amd.BeamStream`.  `keep_lattice=True`: the stream keeps its lattice and has `result_confidence`."""
        return BeamStream(self.transition, graph, batch_size, max_frames, beam_size, beam_threshold, lm_weight, token_score,
                          self.transition.dtype, self.transition.device, keep_lattice)

    def beam_word_stream(self, lexicon, word_lm, batch_size, max_frames, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                         word_score=0.0, token_score=0.0, lookahead=None, keep_lattice=False):
        """A streaming beam decoder with a lexicon and a word n-gram LM under this module's transition matrix (read again at
        every chunk): see `torch_asg_amd.BeamWordStream`.  `keep_lattice=True`: the stream keeps its lattice and has
        `result_confidence`."""
        return BeamWordStream(self.transition, lexicon, word_lm, batch_size, max_frames, beam_size, beam_threshold, lm_weight,
                              word_score, token_score, self.transition.dtype, self.transition.device, lookahead, keep_lattice)

    def beam_window_stream(self, graph, batch_size, window, commit_every=None, beam_size=256, beam_threshold=float("inf"),
                           lm_weight=1.0, token_score=0.0, keep_lattice=False, frame_tolerance=0, max_chunk=None):
        """A streaming beam decoder in bounded memory under this module's transition matrix (read again at every chunk): see
        `torch_asg_amd.BeamWindowStream`.  `keep_lattice=True`: `advance` also returns a confidence and a start frame for every
        token it commits, and the stream has `result_confidence`."""
        return BeamWindowStream(self.transition, graph, batch_size, window, commit_every, beam_size, beam_threshold, lm_weight,
                                token_score, self.transition.dtype, self.transition.device, keep_lattice, frame_tolerance, max_chunk)

    def beam_word_window_stream(self, lexicon, word_lm, batch_size, window, commit_every=None, beam_size=256,
                                beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0, lookahead=None):
        """A streaming beam decoder with a lexicon and a word n-gram LM in bounded memory under this module's transition matrix
        (read again at every chunk): see `torch_asg_amd.BeamWordWindowStream`."""
        return BeamWordWindowStream(self.transition, lexicon, word_lm, batch_size, window, commit_every, beam_size, beam_threshold,
                                    lm_weight, word_score, token_score, self.transition.dtype, self.transition.device, lookahead)

    def graph_loss(self, inputs, targets, graph, input_lengths=None, target_lengths=None, lm_weight=1.0, token_score=0.0,
                   max_work_bytes=1 << 30):
        """`torch_asg_amd.graph_asg_loss` under this module's transition matrix, reduction and scale_mode.  float16 / bfloat16
        emissions are widened to the dtype of `transition`; batch-major views ([B,T,N] transposed) need no copy."""
        return _graph_loss(inputs, targets, self.transition, graph, input_lengths, target_lengths, lm_weight, token_score,
                           max_work_bytes, self.reduction, None, self._utterance_weights)

    def beam_graph_loss(self, inputs, targets, graph, input_lengths=None, target_lengths=None, lm_weight=1.0, token_score=0.0,
                        max_work_bytes=1 << 30, beam_size=256, beam_threshold=float("inf")):
        """`torch_asg_amd.beam_graph_asg_loss` under this module's transition matrix, reduction and scale_mode."""
        _check_beam(beam_size, beam_threshold)
        return _graph_loss(inputs, targets, self.transition, graph, input_lengths, target_lengths, lm_weight, token_score,
                           max_work_bytes, self.reduction, (beam_size, beam_threshold), self._utterance_weights)

    def beam_word_loss(self, inputs, targets, lexicon, word_lm, input_lengths=None, target_lengths=None, lm_weight=1.0,
                       word_score=0.0, token_score=0.0, max_work_bytes=1 << 30, beam_size=256, beam_threshold=float("inf"),
                       lookahead=None):
        """`torch_asg_amd.beam_words_asg_loss` under this module's transition matrix, reduction and scale_mode; `lookahead`
        takes the sets of `beam_decode_words(..., lookahead=)`."""
        _check_beam(beam_size, beam_threshold)
        return _graph_loss(inputs, targets, self.transition, lexicon, input_lengths, target_lengths, lm_weight, token_score,
                           max_work_bytes, self.reduction, (beam_size, beam_threshold), self._utterance_weights,
                           (word_lm, word_score), lookahead)

    @staticmethod
    def _canonical(inputs, targets, input_lengths, target_lengths):
        """Missing lengths mean "the whole axis" (asg.py:113-117); a target axis longer than the time axis is cut to T
        frames and the lengths clipped with it (asg.py:119-122)."""
        T, B = inputs.shape[0], inputs.shape[1]
        S = targets.shape[1]
        if target_lengths is None:
            target_lengths = targets.new_full((B,), S)
        if input_lengths is None:
            input_lengths = target_lengths.new_full((B,), T)
        if S > T:
            targets = targets[:, :T]
            target_lengths = target_lengths.clamp(max=T)
        return targets, input_lengths, target_lengths

    def _utterance_weights(self, inputs, input_lengths, target_lengths):
        if self.scale_mode == 'none':
            return None
        n = input_lengths if self.scale_mode.startswith('input') else target_lengths
        n = n.to(device=inputs.device, dtype=inputs.dtype).clamp(min=1)
        return (n.rsqrt() if self.scale_mode.endswith('sqrt') else n.reciprocal())

    def _bf16_direct(self, inputs, targets):
        """bfloat16 emissions go to the kernels as they are (bf16 in, fp32 accumulate, bf16 gradient out: half the
        compulsory read and write of SURVEY.md 8(d)) on the fused training route; everywhere else they are widened here.
        Whether the fused route takes the problem is asked of the library (asg_loss_fused_supported), not re-stated."""
        if (self.gpu_no_stream_impl or self.forward_only or not self.training or self.scale_mode != 'none'
                or self.launch_mode != 'single' or self.reduction not in ('mean', 'sum', 'none')):
            return False
        if not inputs.is_cuda or self.transition.dtype != torch.float32 or inputs.dim() != 3 or targets.dim() != 2:
            return False
        be = native()
        tg = targets[:, :inputs.shape[0]] if targets.shape[1] > inputs.shape[0] else targets
        try:
            p, _ = be._problem(inputs, self.transition, tg if tg.is_cuda else None, None, None)
        except RuntimeError:
            return False
        if not tg.is_cuda:                       # only the shape of the targets matters to the check
            p.targets, p.S = inputs.data_ptr(), tg.shape[1]
        return be.fused_supported(p) and be.fused_preferred(p, inputs.device)

    # The small-alphabet kernels address state and gradient rows with 32-bit byte offsets (asg_api.hip:check_problem):
    # T * B * max(N, S) * itemsize must stay below this.  Larger batches are split along B here.
    OFFSET_LIMIT = 2 ** 32

    def _batch_chunk(self, inputs, targets):
        """Utterances per call so that the 32-bit offset limit of the small-alphabet kernels holds (0 = no split)."""
        T, B, N = inputs.shape
        if N > 64:
            return 0
        w = 8 if inputs.dtype == torch.float64 else 4
        per_utt = T * max(N, min(targets.shape[1], T)) * w
        if per_utt * B < self.OFFSET_LIMIT:
            return 0
        return max(1, (self.OFFSET_LIMIT - 1) // per_utt)

    def _per_utterance(self, inputs, targets, input_lengths, target_lengths):
        """[B] unreduced losses through the route the module's settings select."""
        args = (targets, input_lengths, target_lengths)
        if self.gpu_no_stream_impl:
            # "serial" route: two independent Functions, difference taken by autograd (asg.py:124-128)
            return FCC.apply(self.transition, inputs, *args) - FAC.apply(self.transition, inputs, *args)
        if self.forward_only or not self.training:
            # evaluation route: beta recursions only, nothing saved, no gradient (asg.py:129-131)
            return ASGGPUFastForwardOnly.apply(inputs, targets, self.transition, input_lengths, target_lengths,
                                               self._flags())
        if self.reduction not in ('mean', 'sum', 'none'):
            # an unknown reduction string behaves like the reference: the unreduced loss falls through (asg.py:141-142)
            full, aligned = ASGGPUFast.apply(inputs, self.transition, *args, self._flags())
            return full - aligned
        return ASGLossFunction.apply(inputs, self.transition, *args, 'none', self._flags())

    def forward(self, inputs, targets, input_lengths=None, target_lengths=None):
        dt = inputs.dtype
        if dt is torch.float16 or (dt is torch.bfloat16 and not self._bf16_direct(inputs, targets)):
            # 16-bit emissions the kernels do not read as they are: widened here (autograd casts the gradient back).  bfloat16 on the
            # fused training step is read directly (_bf16_direct); float16 always widens -- its 5-bit exponent cannot hold log-probabilities
            # below -65504 ("log zero" masks), so a direct route would buy nothing a caller can rely on
            inputs = inputs.to(self.transition.dtype)
        if (_CPP_NODE and input_lengths is not None and target_lengths is not None and self.scale_mode == 'none'
                and not self.gpu_no_stream_impl and (self.forward_only or not self.training)):
            # the evaluation route as one C++ call and one launch: beta recursions, `full - aligned` and the reduction inside the
            # kernels, no autograd graph (asg.py:129-131, 58-68: ASGGPUFastForwardOnly marks its result non-differentiable)
            red = HipBackend._RED.get(self.reduction)
            bd = getattr(_backend or native(), "binding", None)
            if red is not None and bd is not None:
                loss = bd.eval_apply(inputs, self.transition, targets, input_lengths, target_lengths, red,
                                     self._LAUNCH_FLAGS[self.launch_mode])
                if loss is not None:
                    return loss
        elif (_CPP_NODE and self.training and input_lengths is not None and target_lengths is not None
                and self.scale_mode == 'none' and not (self.gpu_no_stream_impl or self.forward_only)):
            # the plain training step: forward, autograd node and backward in C++ (csrc/binding.cpp: Fast.loss_apply); None =
            # not the plain case (CPU or strided arguments, S > T, a batch to split ...), and the statements below take it
            red = HipBackend._RED.get(self.reduction)
            bd = getattr(_backend or native(), "binding", None)
            if red is not None and bd is not None:
                loss = bd.loss_apply(inputs, self.transition, targets, input_lengths, target_lengths, red,
                                     self._LAUNCH_FLAGS[self.launch_mode])
                if loss is not None:
                    return loss
        targets, input_lengths, target_lengths = self._canonical(inputs, targets, input_lengths, target_lengths)
        weights = self._utterance_weights(inputs, input_lengths, target_lengths)
        chunk = self._batch_chunk(inputs, targets) if inputs.dim() == 3 else 0

        if chunk:
            # the batch exceeds what one launch can address: the same routes on slices of it (views: no copy of the
            # emissions; transition.grad accumulates over the slices through autograd)
            B = inputs.shape[1]
            per_utt = torch.cat([self._per_utterance(inputs[:, b0:b0 + chunk], targets[b0:b0 + chunk],
                                                     input_lengths[b0:b0 + chunk], target_lengths[b0:b0 + chunk])
                                 for b0 in range(0, B, chunk)])
        elif (weights is None and self.reduction in ('mean', 'sum', 'none') and self.training
              and not (self.gpu_no_stream_impl or self.forward_only)):
            # training route: subtraction, reduction and their gradients are inside the kernels
            return ASGLossFunction.apply(inputs, self.transition, targets, input_lengths, target_lengths,
                                         self.reduction, self._flags())
        else:
            per_utt = self._per_utterance(inputs, targets, input_lengths, target_lengths)

        if weights is not None:
            per_utt = per_utt * weights
        if self.reduction == 'mean':
            return per_utt.mean()
        if self.reduction == 'sum':
            return per_utt.sum()
        return per_utt


# the streaming decoders (stream.py looks this module's `native` up at every call, so it is imported once the module stands)
from .stream import (BeamStream, BeamStreamResult, BeamWordStream, BeamWordStreamResult, BeamWordStreamNbest,  # noqa: E402,F401
                     BeamWindowStream, BeamWindowCommit, BeamWindowResult, BeamWordWindowStream, BeamWordWindowCommit,
                     BeamWordWindowResult, BeamStreamNbest, BeamWindowNbest, BeamWordWindowNbest, BeamStreamConfidence,
                     BeamWordStreamConfidence, BeamWindowConfCommit, BeamWindowConfidence)
