"""The streaming beam decoders (`BeamStream`, `BeamWordStream`, `BeamWindowStream`, `BeamWordWindowStream`) on one private base
class.

The four families of C entry points (include/asg_hip.h::asg_beam_stream_*, asg_beam_word_stream_*, asg_beam_window_*,
asg_beam_word_window_*) take their arguments in one order,

    (ctx, [p], views..., [B], K, [theta], shape..., state, nbytes, ..., flags, stream)

where `views` is the automaton ((g,), or (g, w) with a word LM) and `shape` what sizes the state ((max_frames,) or
(window, commit_every)).  `_Stream` owns everything that follows from that: the constructor checks, the state, `reset`, the
chunk preamble, the host's bound and the launch of `advance`, the outputs of `result`.  A subclass names its entry points
(`_API`), checks and compiles its automaton, checks its shape, and says what `result` (and `advance`, if anything) returns.
A word stream with LM look-ahead (`lookahead=`) calls the `_la` forms of `_advance` and `_result`, which take one more view
behind the automaton's (`_look`); state size and reset are the plain calls'.
The backend is looked up at every call (`asg.native()`), so that what replaces it in `torch_asg_amd.asg` is what the streams
use.
"""
import collections
import ctypes

import torch

from . import _lib
from . import asg as _asg


class _Stream:
    _API = None                  # "asg_beam_stream": the prefix of _state_bytes, _reset, _advance and _result
    _WIDE = _NARROW = 0          # the number of [B, frames] and of [B] int64 outputs of _result
    max_frames = None            # set by a subclass whose state holds a fixed number of frames: the host's bound of `advance`
    lookahead = None             # set by a word stream: its WordLookahead, or None
    _look = ()                   # ... and the view of it that `_advance_la` and `_result_la` take behind `_views`

    def __init__(self, transition, automaton, batch_size, shape, beam_size, beam_threshold, dtype, device):
        _asg._check_beam(beam_size, beam_threshold)
        graph = self._check_automaton(*automaton)
        self._shape = self._check_shape(batch_size, *shape)
        if dtype not in (torch.float32, torch.float64):
            raise RuntimeError("torch_asg_amd: expected scalar type Float or Double but found %s" % dtype)
        device = torch.device(device) if device is not None else transition.device
        if device.type != "cuda":
            raise RuntimeError("torch_asg_amd: a %s must live on a ROCm device (got %s); "
                               "there is no CPU implementation in this package" % (type(self).__name__, device))
        if transition.dtype != dtype or transition.device != device or tuple(transition.shape) != (graph.N, graph.N):
            raise RuntimeError("torch_asg_amd: transition must be [%d,%d] with the dtype/device of the stream" % (graph.N, graph.N))
        self.transition, self.graph, self.batch_size = transition, graph, int(batch_size)
        self.beam_size, self.beam_threshold = min(int(beam_size), (1 << 31) - 1), float(beam_threshold)
        self.dtype, self.device = dtype, device
        be = _asg.native()
        L = _lib.lib()
        # (entry point, its name for error messages) of the three calls
        la = "" if self.lookahead is None else "_la"
        self._c_reset, self._c_advance, self._c_result = ((getattr(L, self._API + s), self._API + s)
                                                          for s in ("_reset", "_advance" + la, "_result" + la))
        with be._guard(device):
            self._compiled = self._compile()                   # (the views point into it)
            self._views = tuple(ctypes.byref(v) for v in self._compiled[0])
            abi_dtype = _lib.ASG_DTYPE_F32 if dtype == torch.float32 else _lib.ASG_DTYPE_F64
            nbytes = int(getattr(L, self._API + "_state_bytes")(*self._views, self.batch_size, abi_dtype, self.beam_size,
                                                                *self._shape))
            if nbytes == 0:                                    # the library refuses the arguments: its call says why
                reset, what = self._c_reset
                _lib.check(reset(None, *self._views, self.batch_size, self.beam_size, *self._shape, None, 0, None, 0, None), what)
            self._state = be._buf(nbytes, device)
        self._reset(None)

    def _check_automaton(self, graph):
        """The type checks of the constructor's automaton -> the TokenGraph the emissions are checked against."""
        from . import graph as _graph
        if not isinstance(graph, _graph.TokenGraph):
            raise TypeError("torch_asg_amd: graph must be a torch_asg_amd.TokenGraph")
        return graph

    def _check_shape(self, batch_size, max_frames):
        """The range checks of batch_size and of what sizes the state -> the shape tuple of the entry points."""
        if int(batch_size) < 1 or int(max_frames) < 1:
            raise ValueError("torch_asg_amd: batch_size and max_frames must be >= 1, got %d and %d"
                             % (int(batch_size), int(max_frames)))
        return (int(max_frames),)

    def _compile(self):
        """(the C views of the automaton in the entry points' order, what they point into), for self.device and self.dtype."""
        from . import graph as _graph
        compiled = self.graph.compile_beam(self.device, self.dtype, self.lm_weight, self.token_score)
        return (_graph.abi_graph_beam(compiled),), compiled

    def _reset(self, mask):
        be = _asg.native()
        m = None
        if mask is not None:
            if tuple(mask.shape) != (self.batch_size,):
                raise RuntimeError("torch_asg_amd: mask must have shape [%d]" % self.batch_size)
            m = mask.to(self.device).ne(0).to(torch.uint8).contiguous()
        reset, what = self._c_reset
        with be._guard(self.device):
            _lib.check(reset(None, *self._views, self.batch_size, self.beam_size, *self._shape, self._state.data_ptr(),
                             self._state.numel(), m.data_ptr() if m is not None else None, 0, be._stream(self.device)), what)
        if mask is None:
            self._fed = 0                                      # frames offered since the last full reset (the host's bound)

    def _advance(self, chunk, chunk_lengths):
        """`advance`: the chunk as the kernels read it, checked; the host's bound of a stream whose state holds `max_frames`
        frames; one launch on the current stream, which also fills `_commit_outputs` -> those outputs."""
        be = _asg.native()
        transition = self.transition           # (the launch reads pointers, strides, dtype and device: there is no autograd
        if chunk.dtype in (torch.float16, torch.bfloat16):               # history to cut, except of the widening copy)
            chunk = chunk.detach().to(transition.dtype)
        be._check_graph_inputs(chunk, transition, self.graph, chunk_lengths)
        Tc, B, N = chunk.shape
        if chunk.dtype != self.dtype or chunk.device != self.device or B != self.batch_size:
            raise RuntimeError("torch_asg_amd: the stream takes chunks [Tc,%d,%d] of %s on %s, got %s of %s on %s"
                               % (self.batch_size, N, self.dtype, self.device, tuple(chunk.shape), chunk.dtype, chunk.device))
        _asg._check_beam(self.beam_size, self.beam_threshold)
        if self.max_frames is not None and self._fed + Tc > self.max_frames:
            raise ValueError("torch_asg_amd: %d frames since the last reset() plus a chunk of %d exceed max_frames = %d"
                             % (self._fed, Tc, self.max_frames))
        advance, what = self._c_advance
        with be._guard(self.device):
            outs = self._commit_outputs(Tc)
            p, keep = be._problem(chunk, transition, None, chunk_lengths, None)
            _lib.check(advance(None, ctypes.byref(p), *self._views, *self._look, self.beam_size, float(self.beam_threshold),
                               *self._shape, self._state.data_ptr(), self._state.numel(),
                               *[t.data_ptr() for t in outs] if outs else outs, 0, be._stream(self.device)), what)
        self._fed += Tc
        return outs

    @staticmethod
    def _commit_outputs(Tc):
        """The output tensors of `_advance` for a chunk of Tc frames, in the entry point's order."""
        return ()

    def _result(self, final):
        """One `_result` launch into fresh outputs: scores [B], _WIDE tensors [B, shape[0]] and _NARROW tensors [B], handed to
        `_outputs`, whose named tuple lists them in the order in which the entry point takes them."""
        be = _asg.native()
        B, dev = self.batch_size, self.device
        with be._guard(dev):
            scores = torch.empty(B, dtype=self.dtype, device=dev)
            wide = torch.empty(self._WIDE, B, self._shape[0], dtype=torch.int64, device=dev)
            narrow = torch.empty(self._NARROW, B, dtype=torch.int64, device=dev)
            res = self._outputs(scores, wide, narrow)
            result, what = self._c_result
            _lib.check(result(None, *self._views, *self._look, B, self.beam_size, *self._shape, self._state.data_ptr(),
                              self._state.numel(), 1 if final else 0, *[t.data_ptr() for t in res], 0, be._stream(dev)), what)
        return res

    def _token_nbest(self, nbest, final, return_alignments, graph_scores):
        """`result_nbest` of the two token-graph streams: one `_API + "_nbest"` launch over the state, which it only reads ->
        (scores, graph_scores or None, tokens, token_lengths, num_hyps, path, states, narrow), `narrow` the [B] int64 outputs
        behind num_hyps (frames, [committed,] status).  The wide outputs are [B, nbest, shape[0]].  The scratch is allocated
        once per `nbest` and kept on the stream (it is not part of the state), so a captured call replays."""
        if int(nbest) < 1:
            raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
        nbest = min(int(nbest), (1 << 31) - 1)
        be = _asg.native()
        L = _lib.lib()
        B, dev, T = self.batch_size, self.device, self._shape[0]
        n_narrow = self._NARROW - 1                            # `_result`'s narrow outputs without token_lengths
        with be._guard(dev):
            what = self._API + "_nbest"
            fn = getattr(L, what)

            def call(work, nbytes, *outs):
                return fn(None, *self._views, B, self.beam_size, *self._shape, self._state.data_ptr(), self._state.numel(),
                          1 if final else 0, nbest, work, nbytes, *outs)
            work = self._nbest_work.get(nbest)
            if work is None:
                abi_dtype = _lib.ASG_DTYPE_F32 if self.dtype == torch.float32 else _lib.ASG_DTYPE_F64
                nbytes = int(getattr(L, what + "_work_bytes")(*self._views, B, abi_dtype, self.beam_size, *self._shape, nbest))
                if nbytes == 0:                                # the library refuses the arguments: its call says why
                    _lib.check(call(None, 0, *(None,) * 9, 0, None), what)
                work = self._nbest_work[nbest] = be._buf(nbytes, dev)
            sc = torch.empty(2 if graph_scores else 1, B, nbest, dtype=self.dtype, device=dev)
            tokens = torch.empty(B, nbest, T, dtype=torch.int64, device=dev)
            align = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else (None, None)
            token_lengths = torch.empty(B, nbest, dtype=torch.int64, device=dev)
            narrow = torch.empty(1 + n_narrow, B, dtype=torch.int64, device=dev)     # num_hyps, frames, [committed,] status
            al = lambda i: align[i].data_ptr() if return_alignments else None      # noqa: E731
            _lib.check(call(work.data_ptr(), work.numel(), *[t.data_ptr() for t in sc], al(0), tokens.data_ptr(),
                            token_lengths.data_ptr(), al(1), *[t.data_ptr() for t in narrow], 0, be._stream(dev)), what)
        return sc[0], (sc[1] if graph_scores else None), tokens, token_lengths, narrow[0], align[0], align[1], narrow[1:]


BeamStreamResult = collections.namedtuple("BeamStreamResult", ["scores", "path", "tokens", "token_lengths", "states", "frames",
                                                               "status"])
BeamStreamNbest = collections.namedtuple("BeamStreamNbest", ["scores", "graph_scores", "tokens", "token_lengths", "num_hyps", "path",
                                                             "states", "frames", "status"])
BeamStreamConfidence = collections.namedtuple("BeamStreamConfidence", ["scores", "path", "tokens", "token_lengths", "states",
                                                                       "token_frames", "token_confidences", "normalisers", "frames",
                                                                       "status"])


class BeamStream(_Stream):
    """`beam_decode_graph` for an utterance that arrives in chunks: the beam search carried from one chunk to the next, for
    `batch_size` utterance slots at a time.  No gradient.

        s = BeamStream(transition, graph, batch_size, max_frames, beam_size=256)
        for chunk in chunks:                 # [Tc, B, N] each
            s.advance(chunk)
            partial = s.result()             # the best prefix hypothesis so far; the stream goes on
        final = s.result(final=True)         # what beam_decode_graph returns for the whole utterance, bit for bit

    The search is `beam_decode_graph`'s, frame by frame, with the same device code (include/asg_hip.h::asg_beam_stream_advance):
    for any way of cutting an utterance of at most `max_frames` frames into chunks, `result(final=True)` equals the one-shot
    decode of the whole utterance -- scores and token_lengths bit for bit, path / tokens / states on the one-shot's columns and
    -1 beyond.  `transition` (a tensor or Parameter of dtype `dtype`; it is read again at every `advance`), `beam_threshold`,
    `lm_weight` and `token_score` are those of `beam_decode_graph`; the attribute `beam_threshold` may be changed between chunks.

    The state lives in one device buffer (about max_frames * beam_size * 8 bytes of back-pointers plus 12-16 bytes per product
    state, per slot).  The graph is compiled in the constructor; `advance`, `result` and `reset` are one kernel launch each, copy
    nothing and do not synchronise, so they can be captured in a graph and replayed with new chunk contents and lengths.
    `result_nbest` gives the n best hypotheses or prefixes from the same state, with the graph part of each score: the list
    `beam_decode_graph_nbest` returns for the whole utterance, without keeping the emissions or searching twice.

    `keep_lattice=True` makes the state keep the lattice of the search as well (include/asg_hip.h::asg_beam_conf_stream_*: the
    kept sets, the emissions and, lazily, alpha -- about max_frames * (N + 2 * beam_size) values more per slot), and then
    `result_confidence` gives a confidence and a start frame per token at any point of the stream.  `advance`, `result`,
    `result_nbest` and `reset` return what they return without it, byte for byte.
    """
    _API, _WIDE, _NARROW = "asg_beam_stream", 3, 3

    def __init__(self, transition, graph, batch_size, max_frames, beam_size=256, beam_threshold=float("inf"), lm_weight=1.0,
                 token_score=0.0, dtype=torch.float32, device=None, keep_lattice=False):
        self.lm_weight, self.token_score = lm_weight, token_score
        self.keep_lattice = bool(keep_lattice)
        if self.keep_lattice:
            self._API = "asg_beam_conf_stream"                 # the same calls in the same order over the wider state
        self._nbest_work = {}                                  # nbest -> the scratch of result_nbest (not part of the state)
        super().__init__(transition, (graph,), batch_size, (max_frames,), beam_size, beam_threshold, dtype, device)
        (self.max_frames,) = self._shape

    def reset(self, mask=None):
        """Start new utterances: in every slot (mask None), or in the slots where `mask` (bool or integer [B]) is not zero --
        the other slots go on.  After a masked reset `advance`'s host-side check of `max_frames` is not tightened; the device
        clamps and `result().status` reports it."""
        self._reset(mask)

    def advance(self, chunk, chunk_lengths=None):
        """Consume `chunk` [Tc, B, N]: slot b takes its first clamp(chunk_lengths[b], 0, Tc) frames (all Tc when
        `chunk_lengths` is None) as the next frames of its utterance.  Chunk dtype, strides and float16 / bfloat16 widening as in
        `beam_decode_graph`.  ValueError, without touching the device, once the Tc offered since the last full `reset()` exceed
        `max_frames`."""
        self._advance(chunk, chunk_lengths)

    def result(self, final=False):
        """The best hypothesis of every slot over the frames consumed so far, without changing the state -> a named tuple
          scores [B]; path, tokens, states [B, max_frames] int64, -1 behind the data; token_lengths [B]; frames [B], the frames
          consumed; status [B], 1 where frames beyond max_frames were offered and dropped.
        final=True adds the final weights (the transcript of a finished utterance: `beam_decode_graph`'s result); final=False is
        the best prefix hypothesis, largest value without a final weight.  A slot without frames or with an empty beam: -inf, -1, 0."""
        return self._result(final)

    def result_nbest(self, nbest, final=False, return_alignments=False):
        """The `nbest` best hypotheses of every slot over the frames consumed so far, without changing the state -> a named tuple
          scores, graph_scores [B, nbest]; tokens [B, nbest, max_frames] int64, -1 behind the data; token_lengths [B, nbest];
          num_hyps [B]; path, states [B, nbest, max_frames] with `return_alignments`, else None; frames, status [B] as `result`.
        final=True: `beam_decode_graph_nbest`'s rows for the utterance so far, bit for bit, for any chunking.  final=False: the n
        best PREFIXES -- the kept states by value -- with graph_scores without a final weight.  Row 0 equals `result(final)`.
        Rows behind num_hyps: -inf, -1, 0.  The state keeps no emissions, so there is no emission_scores: a caller who kept the
        frames has `beam_decode_graph_nbest`, the others have scores - graph_scores up to rounding.  One launch
        (include/asg_hip.h::asg_beam_stream_nbest); the scratch it needs is allocated once per `nbest` and kept on the stream,
        so a captured call replays.  nbest < 1 raises ValueError, nbest > 8192 RuntimeError."""
        scores, gscores, tokens, tlen, nh, path, states, (frames, status) = self._token_nbest(nbest, final, return_alignments, True)
        return BeamStreamNbest(scores, gscores, tokens, tlen, nh, path, states, frames, status)

    def result_confidence(self, frame_tolerance=0, final=False):
        """`result(final)` with a confidence and a start frame for every token, from the lattice the stream kept
        (`keep_lattice=True`; RuntimeError without it, without touching the device) -> a named tuple
          scores, path, tokens, token_lengths, states, frames, status as `result(final)` returns them;
          token_frames [B, max_frames] int64, the frame at which token k starts, -1 behind the tokens;
          token_confidences [B, max_frames], the posterior, over the paths through the kept sets, that a token with this label
          starts within `frame_tolerance` frames of that frame, 0 behind the tokens; normalisers [B], log of the mass of all paths.
        final=True: `beam_decode_graph_confidence`'s result for the utterance so far, bit for bit, for any chunking and wherever
        `result_confidence` was called in between.  final=False: paths may end in any kept state of the last frame, without a
        final weight.  `transition` must not change within an utterance.  Two launches, no synchronisation: the call captures and
        replays.  The first of them brings the stored alpha rows up to the frames consumed -- the only write to the state from a
        result call; every frame's alpha is computed once.  frame_tolerance < 0 raises ValueError, > 64 RuntimeError."""
        if not self.keep_lattice:
            raise RuntimeError("torch_asg_amd: result_confidence needs the lattice of the search: build the stream with "
                               "keep_lattice=True")
        if int(frame_tolerance) < 0:
            raise ValueError("torch_asg_amd: frame_tolerance must be >= 0, got %d" % int(frame_tolerance))
        tol = min(int(frame_tolerance), (1 << 31) - 1)
        be = _asg.native()
        L = _lib.lib()
        B, dev, T = self.batch_size, self.device, self.max_frames
        transition = self.transition
        with be._guard(dev):
            real = torch.empty(2, B, dtype=self.dtype, device=dev)                 # scores, normalisers
            wide = torch.empty(4, B, T, dtype=torch.int64, device=dev)             # path, tokens, states, token_frames
            conf = torch.empty(B, T, dtype=self.dtype, device=dev)
            narrow = torch.empty(3, B, dtype=torch.int64, device=dev)              # token_lengths, frames, status
            ts = (ctypes.c_int64 * 2)(*transition.stride())
            _lib.check(L.asg_beam_conf_stream_confidence(
                None, *self._views, B, self.beam_size, T, self._state.data_ptr(), self._state.numel(), transition.data_ptr(), ts,
                1 if final else 0, tol, real[0].data_ptr(), wide[0].data_ptr(), wide[1].data_ptr(), narrow[0].data_ptr(),
                wide[2].data_ptr(), wide[3].data_ptr(), conf.data_ptr(), real[1].data_ptr(), narrow[1].data_ptr(),
                narrow[2].data_ptr(), 0, be._stream(dev)), "asg_beam_conf_stream_confidence")
        return BeamStreamConfidence(real[0], wide[0], wide[1], narrow[0], wide[2], wide[3], conf, real[1], narrow[1], narrow[2])

    def _compile(self):
        if not self.keep_lattice:
            return super()._compile()
        from . import graph as _graph
        compiled = self.graph.compile_beam_loss(self.device, self.dtype, self.lm_weight, self.token_score)
        return (_graph.abi_graph_beam_loss(compiled),), compiled

    @staticmethod
    def _outputs(scores, wide, narrow):
        path, tokens, states = wide
        token_lengths, frames, status = narrow
        return BeamStreamResult(scores, path, tokens, token_lengths, states, frames, status)


BeamWordStreamResult = collections.namedtuple("BeamWordStreamResult", ["scores", "path", "tokens", "token_lengths", "states",
                                                                       "lm_states", "words", "word_lengths", "frames", "status"])


BeamWordStreamNbest = collections.namedtuple("BeamWordStreamNbest", ["scores", "graph_scores", "lm_scores", "tokens", "token_lengths",
                                                                     "words", "word_lengths", "num_hyps", "path", "states",
                                                                     "lm_states", "frames", "status"])
BeamWordStreamConfidence = collections.namedtuple("BeamWordStreamConfidence", ["scores", "path", "tokens", "token_lengths", "states",
                                                                               "lm_states", "words", "word_lengths", "word_frames",
                                                                               "word_confidences", "normalisers", "frames",
                                                                               "status"])


class BeamWordStream(_Stream):
    """`beam_decode_words` for an utterance that arrives in chunks: the beam search over pairs (LM history, lexicon product
    state), the word LM composed on the fly, carried from one chunk to the next for `batch_size` utterance slots at a time.
    No gradient.

        s = BeamWordStream(transition, lexicon, word_lm, batch_size, max_frames, beam_size=256)
        for chunk in chunks:                 # [Tc, B, N] each
            s.advance(chunk)
            partial = s.result()             # the best prefix hypothesis so far, its words included; the stream goes on
        final = s.result(final=True)         # what beam_decode_words returns for the whole utterance, bit for bit

    The search is `beam_decode_words`', frame by frame, with the same device code
    (include/asg_hip.h::asg_beam_word_stream_advance): for any way of cutting an utterance of at most `max_frames` frames into
    chunks, `result(final=True)` equals the one-shot decode of the whole utterance -- scores, token_lengths and word_lengths bit
    for bit, path / tokens / states / lm_states / words on the one-shot's columns and -1 beyond.  `transition` (a tensor or
    Parameter of dtype `dtype`; it is read again at every `advance`), `beam_threshold`, `lm_weight`, `word_score` and
    `token_score` are those of `beam_decode_words`; the attribute `beam_threshold` may be changed between chunks.  beam_size >
    8192 is refused by the library (there is no clamp to the number of product states).

    The state lives in one device buffer (about max_frames * beam_size * 12 bytes of back-pointers plus 60-80 bytes per
    candidate a frame can have, per slot; nothing is sized by the vocabulary or the LM).  Lexicon and LM are compiled in the
    constructor; `advance`, `result` and `reset` are one kernel launch each, copy nothing and do not synchronise, so they can be
    captured in a graph and replayed with new chunk contents and lengths.  `result_nbest` gives the n best hypotheses or
    prefixes with their score split.  The windowed form with a committed prefix is `BeamWordWindowStream`.

    `lookahead`, a `WordLookahead(lexicon, word_lm, order)`, makes every frame `beam_decode_words(..., lookahead=)`'s
    (include/asg_hip.h::asg_beam_word_stream_advance_la): `result(final=True)` then equals that call, bit for bit, for any
    chunking, and a prefix result takes the estimate that has not cancelled yet back (see `result`).  The stream is bound to
    its look-ahead for life -- the values in the state carry it -- and the state has the same size with or without.

    `keep_lattice=True` makes the state keep the lattice of the search as well (include/asg_hip.h::asg_beam_word_conf_stream_*:
    the kept pair sets, the emissions and, lazily, alpha -- about max_frames * (N + 4 * beam_size) values more per slot), and then
    `result_confidence` gives a confidence and an end frame per word at any point of the stream, with or without a look-ahead.
    `advance`, `result`, `result_nbest` and `reset` return what they return without it, byte for byte.  The lattice pass keeps a
    frame's set in LDS, so beam_size is bounded as for `beam_decode_words_confidence` (8179 float32, 6816 float64).
    Not here: a loss over a stream (the one-shot loss over pairs is `beam_words_asg_loss`); the public `result_nbest` of a
    stream with a look-ahead still raises (the library call, asg_beam_word_stream_nbest_la, is there and `_result_nbest` reaches
    it).
    """
    _API, _WIDE, _NARROW = "asg_beam_word_stream", 5, 4

    def __init__(self, transition, lexicon, word_lm, batch_size, max_frames, beam_size=256, beam_threshold=float("inf"),
                 lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=torch.float32, device=None, lookahead=None,
                 keep_lattice=False):
        self.lm_weight, self.word_score, self.token_score, self.lookahead = lm_weight, word_score, token_score, lookahead
        self.keep_lattice = bool(keep_lattice)
        if self.keep_lattice:
            self._API = "asg_beam_word_conf_stream"            # the same calls in the same order over the wider state
        self._nbest_work = {}                                  # nbest -> the scratch of result_nbest (not part of the state)
        super().__init__(transition, (lexicon, word_lm), batch_size, (max_frames,), beam_size, beam_threshold, dtype, device)
        (self.max_frames,) = self._shape

    def _check_automaton(self, lexicon, word_lm):
        from . import wordlm as _wordlm
        _wordlm.check_words(lexicon, word_lm)
        if self.lookahead is not None:
            _wordlm.check_lookahead(self.lookahead, lexicon, word_lm)
        self.lexicon, self.word_lm = lexicon, word_lm
        return lexicon.graph

    def _compile(self):
        from . import wordlm as _wordlm
        g, w, keep = _wordlm.abi_words(self.lexicon, self.word_lm, self.device, self.dtype, self.lm_weight, self.word_score,
                                       self.token_score)
        if self.lookahead is not None:                         # with the stream's weights, through the look-ahead's own cache
            la_dev = self.lookahead.compile(self.device, self.dtype, self.lm_weight, self.word_score)
            la = _wordlm.abi_lookahead(la_dev)
            self._look = (ctypes.byref(la),)
            keep = (keep, la, la_dev)
        return (g, w), keep

    def reset(self, mask=None):
        """Start new utterances: in every slot (mask None), or in the slots where `mask` (bool or integer [B]) is not zero --
        the other slots go on.  After a masked reset `advance`'s host-side check of `max_frames` is not tightened; the device
        clamps and `result().status` reports it."""
        self._reset(mask)

    def advance(self, chunk, chunk_lengths=None):
        """Consume `chunk` [Tc, B, N]: slot b takes its first clamp(chunk_lengths[b], 0, Tc) frames (all Tc when
        `chunk_lengths` is None) as the next frames of its utterance.  Chunk dtype, strides and float16 / bfloat16 widening as in
        `beam_decode_words`.  ValueError, without touching the device, once the Tc offered since the last full `reset()` exceed
        `max_frames`."""
        self._advance(chunk, chunk_lengths)

    def result(self, final=False):
        """The best hypothesis of every slot over the frames consumed so far, without changing the state -> a named tuple
          scores [B]; path, tokens, states, lm_states, words [B, max_frames] int64, -1 behind the data; token_lengths,
          word_lengths [B]; frames [B], the frames consumed; status [B], 1 where frames beyond max_frames were offered and dropped.
        final=True is the end of `beam_decode_words` (final weight, the LM's end of the sentence, after one more LM step for a
        path that ends in a word-end node, whose word is appended; a path that ends mid-word does not count).  final=False is the
        best prefix hypothesis, the largest value without any end term: it may end mid-word, and `words` holds the words whose
        separator the path has passed.  With a look-ahead the value of a prefix is taken without the estimate it still carries
        (v - L(h, node)), so a prefix score means what it means without look-ahead and a beam that prunes nothing returns the
        plain stream's prefix.  A slot without frames, with an empty beam or without a finite score: -inf, -1, 0."""
        return self._result(final)

    def result_nbest(self, nbest, final=False, return_alignments=False):
        """The `nbest` best hypotheses of every slot over the frames consumed so far, without changing the state -> a named tuple
          scores, graph_scores, lm_scores [B, nbest]; tokens, words [B, nbest, max_frames] int64, -1 behind the data;
          token_lengths, word_lengths [B, nbest]; num_hyps [B]; path, states, lm_states [B, nbest, max_frames] with
          `return_alignments`, else None; frames, status [B] as `result`.
        final=True: `beam_decode_words_nbest`'s rows for the utterance so far, bit for bit, for any chunking.  final=False: the n
        best PREFIXES -- the kept pairs by value, mid-word ones included; graph_scores without a final weight, lm_scores without
        the end of the sentence, no final word.  Row 0 equals `result(final)`.  The state keeps no emissions, so there is no
        emission_scores: scores - (graph_scores + lm_scores) is it up to rounding.  One launch; the scratch it needs is allocated
        once per `nbest` and kept on the stream, so a captured call replays.  nbest < 1 raises ValueError, nbest > 8192
        RuntimeError.  A stream built with a look-ahead still raises NotImplementedError here: the rule for its list exists
        (include/asg_hip.h::asg_beam_word_stream_nbest_la: the three parts take no look-ahead term) and `_result_nbest` runs it,
        but the public method keeps the raise its tests pin until they change with it."""
        if self.lookahead is not None:
            raise NotImplementedError("torch_asg_amd: result_nbest of a stream with a look-ahead is not there (the public method "
                                      "is not opened yet; `_result_nbest` runs asg_beam_word_stream_nbest_la); build the stream "
                                      "without `lookahead`")
        return self._result_nbest(nbest, final, return_alignments)

    def _result_nbest(self, nbest, final, return_alignments):
        """`result_nbest` behind its look-ahead check.  With a look-ahead the stream's own view goes behind the LM
        (asg_beam_word_stream_nbest_la): candidates by the end of `result(final)` -- in prefix mode v - L(h, node) -- row 0
        equal to `result(final)`, final rows equal to `beam_decode_words_nbest(..., lookahead=)`'s, graph_scores and lm_scores
        without any look-ahead term."""
        if int(nbest) < 1:
            raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
        nbest = min(int(nbest), (1 << 31) - 1)
        be = _asg.native()
        L = _lib.lib()
        B, dev, T = self.batch_size, self.device, self.max_frames
        with be._guard(dev):
            what = self._API + "_nbest" + ("" if self.lookahead is None else "_la")
            fn = getattr(L, what)

            def call(work, nbytes, *outs):
                return fn(None, *self._views, *self._look, B, self.beam_size, T, self._state.data_ptr(), self._state.numel(),
                          1 if final else 0, nbest, work, nbytes, *outs)
            work = self._nbest_work.get(nbest)
            if work is None:
                abi_dtype = _lib.ASG_DTYPE_F32 if self.dtype == torch.float32 else _lib.ASG_DTYPE_F64
                nbytes = int(getattr(L, self._API + "_nbest_work_bytes")(*self._views, B, abi_dtype, self.beam_size, T, nbest))
                if nbytes == 0:                                # the library refuses the arguments: its call says why
                    _lib.check(call(None, 0, *(None,) * 13, 0, None), what)
                work = self._nbest_work[nbest] = be._buf(nbytes, dev)
            sc = torch.empty(3, B, nbest, dtype=self.dtype, device=dev)        # scores, graph and LM scores
            wide = torch.empty(2, B, nbest, T, dtype=torch.int64, device=dev)  # tokens, words
            align = torch.empty(3, B, nbest, T, dtype=torch.int64, device=dev) if return_alignments else (None,) * 3
            lengths = torch.empty(2, B, nbest, dtype=torch.int64, device=dev)  # token_lengths, word_lengths
            narrow = torch.empty(3, B, dtype=torch.int64, device=dev)          # num_hyps, frames, status
            al = lambda i: align[i].data_ptr() if return_alignments else None      # noqa: E731
            _lib.check(call(work.data_ptr(), work.numel(), sc[0].data_ptr(), sc[1].data_ptr(), sc[2].data_ptr(), al(0),
                            wide[0].data_ptr(), lengths[0].data_ptr(), al(1), al(2), wide[1].data_ptr(), lengths[1].data_ptr(),
                            narrow[0].data_ptr(), narrow[1].data_ptr(), narrow[2].data_ptr(), 0, be._stream(dev)), what)
        return BeamWordStreamNbest(sc[0], sc[1], sc[2], wide[0], lengths[0], wide[1], lengths[1], narrow[0], align[0], align[1],
                                   align[2], narrow[1], narrow[2])

    def result_confidence(self, frame_tolerance=0, final=False):
        """`result(final)` with a confidence and an end frame for every word, from the lattice the stream kept
        (`keep_lattice=True`; RuntimeError without it, without touching the device) -> a named tuple
          scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, frames, status as `result(final)` returns
          them;
          word_frames [B, max_frames] int64, the frame at which word k ends (the frame of its separator, or the number of frames
          for the word of the final step), -1 behind the words;
          word_confidences [B, max_frames], the posterior, over the paths through the kept pair sets, that this word ends within
          `frame_tolerance` frames of that frame, 0 behind the words; normalisers [B], log of the mass of all paths.
        final=True: `beam_decode_words_confidence`'s result (with the stream's look-ahead, if it has one) for the utterance so
        far, bit for bit, for any chunking and wherever `result_confidence` was called in between.  final=False: paths may end in
        any kept pair of the last frame, mid-word ones included, without any end term; the words are those whose separator the
        path has passed, and no word ends at the last frame by the end rule.  With a look-ahead the sets are the look-ahead
        search's and the lattice is weighed plainly, as in `beam_decode_words_confidence`.  `transition` must not change within
        an utterance.  Two launches, no synchronisation: the call captures and replays.  The first of them brings the stored
        alpha rows up to the frames consumed -- the only write to the state from a result call; every frame's alpha is computed
        once.  frame_tolerance < 0 raises ValueError, > 64 RuntimeError."""
        if not self.keep_lattice:
            raise RuntimeError("torch_asg_amd: result_confidence needs the lattice of the search: build the stream with "
                               "keep_lattice=True")
        if int(frame_tolerance) < 0:
            raise ValueError("torch_asg_amd: frame_tolerance must be >= 0, got %d" % int(frame_tolerance))
        tol = min(int(frame_tolerance), (1 << 31) - 1)
        be = _asg.native()
        L = _lib.lib()
        B, dev, T = self.batch_size, self.device, self.max_frames
        transition = self.transition
        what = "asg_beam_word_conf_stream_confidence" + ("" if self.lookahead is None else "_la")
        with be._guard(dev):
            real = torch.empty(2, B, dtype=self.dtype, device=dev)                 # scores, normalisers
            wide = torch.empty(6, B, T, dtype=torch.int64, device=dev)             # path, tokens, states, lm_states, words, frames
            conf = torch.empty(B, T, dtype=self.dtype, device=dev)
            narrow = torch.empty(4, B, dtype=torch.int64, device=dev)              # two lengths, frames, status
            ts = (ctypes.c_int64 * 2)(*transition.stride())
            _lib.check(getattr(L, what)(
                None, *self._views, *self._look, B, self.beam_size, T, self._state.data_ptr(), self._state.numel(),
                transition.data_ptr(), ts, 1 if final else 0, tol, real[0].data_ptr(), wide[0].data_ptr(), wide[1].data_ptr(),
                narrow[0].data_ptr(), wide[2].data_ptr(), wide[3].data_ptr(), wide[4].data_ptr(), narrow[1].data_ptr(),
                wide[5].data_ptr(), conf.data_ptr(), real[1].data_ptr(), narrow[2].data_ptr(), narrow[3].data_ptr(), 0,
                be._stream(dev)), what)
        return BeamWordStreamConfidence(real[0], wide[0], wide[1], narrow[0], wide[2], wide[3], wide[4], narrow[1], wide[5], conf,
                                        real[1], narrow[2], narrow[3])

    @staticmethod
    def _outputs(scores, wide, narrow):
        path, tokens, states, lm_states, words = wide
        token_lengths, word_lengths, frames, status = narrow
        return BeamWordStreamResult(scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, frames, status)


BeamWindowCommit = collections.namedtuple("BeamWindowCommit", ["path", "states", "tokens", "token_lengths", "frames"])
BeamWindowResult = collections.namedtuple("BeamWindowResult", ["scores", "path", "tokens", "token_lengths", "states", "frames",
                                                               "committed", "status"])
BeamWindowNbest = collections.namedtuple("BeamWindowNbest", ["scores", "tokens", "token_lengths", "num_hyps", "path", "states",
                                                             "frames", "committed", "status"])
BeamWindowConfCommit = collections.namedtuple("BeamWindowConfCommit", BeamWindowCommit._fields + ("token_frames",
                                                                                                  "token_confidences"))
BeamWindowConfidence = collections.namedtuple("BeamWindowConfidence", ["scores", "path", "tokens", "token_lengths", "states",
                                                                       "token_frames", "token_confidences", "normalisers", "frames",
                                                                       "committed", "status"])


class BeamWindowStream(_Stream):
    """`BeamStream` in bounded memory, for utterances without an end in sight: the same beam search, the back-pointers kept only
    for a window of `window` frames, and the prefix of the transcript on which all surviving hypotheses agree COMMITTED -- handed
    out by the `advance` that finds it, never to change.  No gradient.

        s = BeamWindowStream(transition, graph, batch_size, window=128, beam_size=256)
        for chunk in chunks:                 # [Tc, B, N] each, for as long as the microphone is open
            new = s.advance(chunk)           # new.tokens[b, :new.token_lengths[b]]: append them to slot b's transcript
            tail = s.result()                # the best hypothesis for the frames that are not committed yet
        last = s.result(final=True)          # the committed tokens + last.tokens are the transcript

    After every frame whose count is a multiple of `commit_every` (default max(1, window // 4)) the device looks for the latest
    frame at which all hypotheses of the beam share one ancestor and commits everything up to it; if the uncommitted frames would
    not leave room for the next `commit_every` frames in the window, it commits the oldest ones along the best hypothesis and sets
    bit 0 of `status` (include/asg_hip.h::asg_beam_window_advance).  Scores are `BeamStream`'s and `beam_decode_graph`'s bit for
    bit, for every window; while bit 0 of `status` is clear the committed frames followed by the tail are `beam_decode_graph`'s
    path, and the same for the tokens.  What is committed does not depend on how the frames were cut into chunks.

    The state is one device buffer of about window * beam_size * 8 bytes of back-pointers plus 12-16 bytes per product state,
    per slot, whatever the length of the utterance; `result` walks at most `window` frames.  `advance`, `result` and `reset` are
    one kernel launch each, copy nothing and do not synchronise, so they can be captured and replayed.  The other arguments are
    `BeamStream`'s; there is no bound on the number of frames.  `result_nbest` gives the n best hypotheses as their uncommitted
    tails, with `BeamStream.result_nbest`'s scores.

    `keep_lattice=True` makes the state keep the lattice of the search in a ring of window + frame_tolerance + 1 + max_chunk
    frames (include/asg_hip.h::asg_beam_conf_window_*: the kept sets, the emissions and alpha -- about that many times
    N + 2 * beam_size values more per slot, whatever the length of the stream).  `advance` then returns a
    `BeamWindowConfCommit`: the five fields and, for every token it commits, `token_frames` (the absolute frame at which the
    token starts) and `token_confidences` (the posterior, at the moment of the commit, that a token with this label starts within
    `frame_tolerance` frames of that frame: `BeamStream(keep_lattice=True).result_confidence(frame_tolerance)`'s value at that
    position, bit for bit while bit 0 of `status` is clear), -1 and 0 behind the tokens; it is three launches and still captures.
    `result_confidence` gives the same for the uncommitted tail.  `frame_tolerance` (0 .. 64) and `max_chunk` (default `window`;
    a longer chunk raises ValueError) size the state and are fixed for the life of the stream.  The five fields, `result`,
    `result_nbest` and `reset` return what they return without `keep_lattice`, byte for byte.  alpha and the normaliser grow with
    the stream, as the scores do: float32 loses resolution in a posterior as they pass about 1e5, so streams of hours want
    float64.
    """
    _API, _WIDE, _NARROW = "asg_beam_window", 3, 4

    def __init__(self, transition, graph, batch_size, window, commit_every=None, beam_size=256, beam_threshold=float("inf"),
                 lm_weight=1.0, token_score=0.0, dtype=torch.float32, device=None, keep_lattice=False, frame_tolerance=0,
                 max_chunk=None):
        self.lm_weight, self.token_score = lm_weight, token_score
        self.keep_lattice = bool(keep_lattice)
        shape = (window, commit_every)
        if self.keep_lattice:
            self._API = "asg_beam_conf_window"                 # the same calls in the same order over the wider state, whose
            shape += (frame_tolerance, max_chunk)              # shape has two more parameters
        self._nbest_work = {}                                  # nbest -> the scratch of result_nbest (not part of the state)
        super().__init__(transition, (graph,), batch_size, shape, beam_size, beam_threshold, dtype, device)
        self.window, self.commit_every = self._shape[:2]
        self.frame_tolerance, self.max_chunk = self._shape[2:] if self.keep_lattice else (None, None)

    def _check_shape(self, batch_size, window, commit_every, frame_tolerance=None, max_chunk=None):
        if int(batch_size) < 1 or int(window) < 1:
            raise ValueError("torch_asg_amd: batch_size and window must be >= 1, got %d and %d" % (int(batch_size), int(window)))
        commit_every = max(1, int(window) // 4) if commit_every is None else int(commit_every)
        if not 1 <= commit_every <= int(window):
            raise ValueError("torch_asg_amd: commit_every must be in 1 .. window = %d, got %d" % (int(window), commit_every))
        if frame_tolerance is None:
            return int(window), commit_every
        if int(frame_tolerance) < 0:
            raise ValueError("torch_asg_amd: frame_tolerance must be >= 0, got %d" % int(frame_tolerance))
        max_chunk = int(window) if max_chunk is None else int(max_chunk)
        if max_chunk < 1:
            raise ValueError("torch_asg_amd: max_chunk must be >= 1, got %d" % max_chunk)
        return int(window), commit_every, min(int(frame_tolerance), (1 << 31) - 1), max_chunk

    def _compile(self):
        if not self.keep_lattice:
            return super()._compile()
        from . import graph as _graph
        compiled = self.graph.compile_beam_loss(self.device, self.dtype, self.lm_weight, self.token_score)
        return (_graph.abi_graph_beam_loss(compiled),), compiled

    def reset(self, mask=None):
        """Start new utterances: in every slot (mask None), or in the slots where `mask` (bool or integer [B]) is not zero --
        the other slots go on."""
        self._reset(mask)

    def advance(self, chunk, chunk_lengths=None):
        """Consume `chunk` [Tc, B, N] as `BeamStream.advance` does -> what this call committed, a named tuple
          path, states, tokens [B, window + Tc] int64, -1 behind the data: label and automaton state of every newly committed
          frame, and the tokens they add to the transcript (the collapse goes on across calls); token_lengths [B]; frames [B],
          the number of frames committed by this call."""
        if self.keep_lattice:
            if chunk.dim() == 3 and chunk.shape[0] > self.max_chunk:       # (the ring holds max_chunk frames behind an attempt)
                raise ValueError("torch_asg_amd: a chunk of %d frames exceeds max_chunk = %d" % (chunk.shape[0], self.max_chunk))
            path, states, tokens, frames, token_lengths, token_frames, conf = self._advance(chunk, chunk_lengths)
            return BeamWindowConfCommit(path, states, tokens, token_lengths, frames, token_frames, conf)
        path, states, tokens, frames, token_lengths = self._advance(chunk, chunk_lengths)
        return BeamWindowCommit(path, states, tokens, token_lengths, frames)

    def _commit_outputs(self, Tc):
        B, cols, dev = self.batch_size, self.window + Tc, self.device
        path, states, tokens = torch.empty(3, B, cols, dtype=torch.int64, device=dev)
        frames, token_lengths = torch.empty(2, B, dtype=torch.int64, device=dev)
        if not self.keep_lattice:
            return path, states, tokens, frames, token_lengths
        return (path, states, tokens, frames, token_lengths, torch.empty(B, cols, dtype=torch.int64, device=dev),
                torch.empty(B, cols, dtype=self.dtype, device=dev))

    def result(self, final=False):
        """The best hypothesis of every slot for the frames that are not committed yet, without changing the state -> a named tuple
          scores [B], the score of the whole hypothesis; path, tokens, states [B, window] int64, -1 behind the data: the
          uncommitted tail (a first label that repeats the last committed one is no token); token_lengths [B]; frames [B], the
          frames consumed; committed [B], the frames committed; status [B]: bit 0 = frames were committed before the hypotheses
          agreed on them, bit 1 = the beam is empty.
        final as for `BeamStream.result`.  A slot without frames or with an empty beam: -inf, -1, 0."""
        return self._result(final)

    def result_nbest(self, nbest, final=False, return_alignments=False):
        """The `nbest` best hypotheses of every slot, each as its uncommitted TAIL, without changing the state -> a named tuple
          scores [B, nbest], the scores of the whole hypotheses: `BeamStream.result_nbest`'s at equal position, bit for bit;
          tokens [B, nbest, window] int64, -1 behind the data: the collapse of the row's tail, started from the last committed
          label; token_lengths [B, nbest]; num_hyps [B]; path, states [B, nbest, window] with `return_alignments`, else None: the
          frames committed .. frames-1 on the row's own chain; frames, committed, status [B] as `result`.
        While bit 0 of `status` is clear, what `advance` has committed followed by a row's tail is that row of
        `BeamStream.result_nbest` -- a commit by convergence is an ancestor of every later hypothesis; after a forced commit the
        rows are still their own chains, but need not continue the committed prefix.  A tail may be empty (everything is
        committed): the row still counts.  There is no graph_scores: the edge into the first tail frame needs the state of the
        frame before it, which the window may have dropped.  One launch (include/asg_hip.h::asg_beam_window_nbest), at most
        `window` steps per row; the scratch is kept on the stream per `nbest`, so a captured call replays.  nbest < 1 raises
        ValueError, nbest > 8192 RuntimeError."""
        scores, _, tokens, tlen, nh, path, states, (frames, committed, status) = self._token_nbest(nbest, final, return_alignments,
                                                                                                   False)
        return BeamWindowNbest(scores, tokens, tlen, nh, path, states, frames, committed, status)

    def result_confidence(self, final=False):
        """`result(final)` with a confidence and a start frame for every token of the uncommitted tail, from the lattice ring
        (`keep_lattice=True`; RuntimeError without it, without touching the device) -> a named tuple
          scores, path, tokens, token_lengths, states, frames, committed, status as `result(final)` returns them;
          token_frames [B, window] int64, the absolute frame at which tail token k starts, -1 behind the tokens;
          token_confidences [B, window], the posterior that a token with this label starts within the stream's `frame_tolerance`
          of that frame, over the paths through the kept sets of all frames consumed, 0 behind the tokens; normalisers [B].
        final=True ends the paths with the final weights: while bit 0 of `status` is clear the values are
        `beam_decode_graph_confidence`'s for those tokens, bit for bit.  Two launches, no synchronisation; it only reads the
        state (`advance` has already brought the alpha rows up to the frames consumed)."""
        if not self.keep_lattice:
            raise RuntimeError("torch_asg_amd: result_confidence needs the lattice of the search: build the stream with "
                               "keep_lattice=True")
        be = _asg.native()
        L = _lib.lib()
        B, dev, W = self.batch_size, self.device, self.window
        transition = self.transition
        with be._guard(dev):
            real = torch.empty(2, B, dtype=self.dtype, device=dev)                 # scores, normalisers
            wide = torch.empty(4, B, W, dtype=torch.int64, device=dev)             # path, tokens, states, token_frames
            conf = torch.empty(B, W, dtype=self.dtype, device=dev)
            narrow = torch.empty(4, B, dtype=torch.int64, device=dev)              # token_lengths, frames, committed, status
            ts = (ctypes.c_int64 * 2)(*transition.stride())
            _lib.check(L.asg_beam_conf_window_confidence(
                None, *self._views, B, self.beam_size, *self._shape, self._state.data_ptr(), self._state.numel(),
                transition.data_ptr(), ts, 1 if final else 0, real[0].data_ptr(), wide[0].data_ptr(), wide[1].data_ptr(),
                narrow[0].data_ptr(), wide[2].data_ptr(), wide[3].data_ptr(), conf.data_ptr(), real[1].data_ptr(),
                narrow[1].data_ptr(), narrow[2].data_ptr(), narrow[3].data_ptr(), 0, be._stream(dev)),
                "asg_beam_conf_window_confidence")
        return BeamWindowConfidence(real[0], wide[0], wide[1], narrow[0], wide[2], wide[3], conf, real[1], narrow[1], narrow[2],
                                    narrow[3])

    @staticmethod
    def _outputs(scores, wide, narrow):
        path, tokens, states = wide
        token_lengths, frames, committed, status = narrow
        return BeamWindowResult(scores, path, tokens, token_lengths, states, frames, committed, status)


BeamWordWindowCommit = collections.namedtuple("BeamWordWindowCommit", ["path", "states", "lm_states", "tokens", "token_lengths",
                                                                       "words", "word_lengths", "frames"])
BeamWordWindowResult = collections.namedtuple("BeamWordWindowResult", ["scores", "path", "tokens", "token_lengths", "states",
                                                                       "lm_states", "words", "word_lengths", "frames", "committed",
                                                                       "status"])


BeamWordWindowNbest = collections.namedtuple("BeamWordWindowNbest", ["scores", "tokens", "token_lengths", "words", "word_lengths",
                                                                     "num_hyps", "path", "states", "lm_states", "frames",
                                                                     "committed", "status"])


class BeamWordWindowStream(_Stream):
    """`BeamWordStream` in bounded memory, for utterances without an end in sight: the beam search over pairs (LM history,
    lexicon product state) with the word LM composed on the fly, the back-pointers kept only for a window of `window` frames,
    and the prefix of the transcript on which all surviving hypotheses agree COMMITTED -- handed out, in tokens and in WORDS, by
    the `advance` that finds it, never to change.  No gradient.

        s = BeamWordWindowStream(transition, lexicon, word_lm, batch_size, window=128, beam_size=256)
        for chunk in chunks:                 # [Tc, B, N] each, for as long as the microphone is open
            new = s.advance(chunk)           # new.words[b, :new.word_lengths[b]]: append them to slot b's transcript
            tail = s.result()                # the best hypothesis for the frames that are not committed yet
        last = s.result(final=True)          # the committed words + last.words are the transcript

    The commit rule is `BeamWindowStream`'s over the kept pairs (include/asg_hip.h::asg_beam_word_window_advance): after every
    frame whose count is a multiple of `commit_every` (default max(1, window // 4)) the device looks for the latest frame at
    which all hypotheses of the beam share one ancestor and commits everything up to it; if the uncommitted frames would not
    leave room for the next `commit_every` frames in the window, it commits the oldest ones along the best prefix hypothesis
    and sets bit 0 of `status`.  A word is committed with the frame of its separator, exactly once, wherever commits and calls
    cut the utterance.  Scores are `BeamWordStream`'s and `beam_decode_words`' bit for bit, for every window; while bit 0 of
    `status` is clear the committed frames followed by the tail are `beam_decode_words`' path, and the same for states,
    lm_states, tokens and words.  What is committed does not depend on how the frames were cut into chunks.

    The state is one device buffer of about window * beam_size * 12 bytes of back-pointers plus 60-80 bytes per candidate a
    frame can have, per slot, whatever the length of the utterance; `result` walks at most `window` frames.  `advance`, `result`
    and `reset` are one kernel launch each, copy nothing and do not synchronise, so they can be captured and replayed.  The other
    arguments are `BeamWordStream`'s (`dtype` None: the transition's), `lookahead` included
    (include/asg_hip.h::asg_beam_word_window_advance_la: the forced commit then follows the best prefix by value minus
    look-ahead, everything above holds with `beam_decode_words(..., lookahead=)` in the place of `beam_decode_words`); there is
    no bound on the number of frames.  `result_nbest` gives the n best hypotheses as their uncommitted tails, with
    `BeamWordStream.result_nbest`'s scores, with or without a look-ahead.
    """
    _API, _WIDE, _NARROW = "asg_beam_word_window", 5, 5
    _check_automaton, _compile = BeamWordStream._check_automaton, BeamWordStream._compile      # the automaton is BeamWordStream's,
    _check_shape = BeamWindowStream._check_shape                                               # the shape BeamWindowStream's

    def __init__(self, transition, lexicon, word_lm, batch_size, window, commit_every=None, beam_size=256,
                 beam_threshold=float("inf"), lm_weight=1.0, word_score=0.0, token_score=0.0, dtype=None, device=None,
                 lookahead=None):
        self.lm_weight, self.word_score, self.token_score, self.lookahead = lm_weight, word_score, token_score, lookahead
        self._nbest_work = {}                                  # nbest -> the scratch of result_nbest (not part of the state)
        super().__init__(transition, (lexicon, word_lm), batch_size, (window, commit_every), beam_size, beam_threshold,
                         transition.dtype if dtype is None else dtype, device)
        self.window, self.commit_every = self._shape

    def reset(self, mask=None):
        """Start new utterances: in every slot (mask None), or in the slots where `mask` (bool or integer [B]) is not zero --
        the other slots go on."""
        self._reset(mask)

    def advance(self, chunk, chunk_lengths=None):
        """Consume `chunk` [Tc, B, N] as `BeamWordStream.advance` does, without a bound on the frames -> what this call
        committed, a named tuple
          path, states, lm_states, tokens, words [B, window + Tc] int64, -1 behind the data: label, automaton state and LM state
          of every newly committed frame, and the tokens and words they add to the transcript (both go on across calls);
          token_lengths, word_lengths [B]; frames [B], the number of frames committed by this call."""
        path, states, lm_states, tokens, words, frames, token_lengths, word_lengths = self._advance(chunk, chunk_lengths)
        return BeamWordWindowCommit(path, states, lm_states, tokens, token_lengths, words, word_lengths, frames)

    def _commit_outputs(self, Tc):
        wide = torch.empty(5, self.batch_size, self.window + Tc, dtype=torch.int64, device=self.device)
        narrow = torch.empty(3, self.batch_size, dtype=torch.int64, device=self.device)
        return tuple(wide) + tuple(narrow)                     # path, states, lm_states, tokens, words; frames, two lengths

    def result(self, final=False):
        """The best hypothesis of every slot for the frames that are not committed yet, without changing the state -> a named
        tuple
          scores [B], the score of the whole hypothesis; path, tokens, states, lm_states, words [B, window] int64, -1 behind the
          data: the uncommitted tail (a first label that repeats the last committed one is no token; a separator behind the
          last committed label ends a word); token_lengths, word_lengths [B]; frames [B], the frames consumed; committed [B],
          the frames committed; status [B]: bit 0 = frames were committed before the hypotheses agreed on them, bit 1 = the beam
          is empty.
        final as for `BeamWordStream.result`: final=True appends the word of a path that ends in a word-end node.  A slot
        without frames, with an empty beam or without a finite score: -inf, -1, 0."""
        return self._result(final)

    def result_nbest(self, nbest, final=False, return_alignments=False):
        """The `nbest` best hypotheses of every slot, each as its uncommitted TAIL, without changing the state -> a named tuple
          scores [B, nbest], the scores of the whole hypotheses: `BeamWordStream.result_nbest`'s at equal position, bit for bit
          (with a look-ahead a prefix score is taken without the estimate it still carries, as in `result`); tokens, words
          [B, nbest, window] int64, -1 behind the data: the tokens and words of the row's tail, started from the last committed
          label and automaton state -- a separator on the first uncommitted frame gives its word here, once -- and with
          final=True the word of a row that ends in a word-end node, also behind an empty tail; token_lengths, word_lengths
          [B, nbest]; num_hyps [B]; path, states, lm_states [B, nbest, window] with `return_alignments`, else None: the frames
          committed .. frames-1 on the row's own chain; frames, committed, status [B] as `result`.
        Row 0 equals `result(final)`.  While bit 0 of `status` is clear, what `advance` has committed followed by a row's tail is
        that row of `BeamWordStream.result_nbest` -- a commit by convergence is an ancestor of every later hypothesis; after a
        forced commit the rows are still their own chains, but need not continue the committed prefix.  A tail may be empty
        (everything is committed): the row still counts.  There are no graph_scores or lm_scores: the sums of the committed part
        are gone, and the edge into the first tail frame needs the pair of the frame before it, which the window does not keep.
        One launch (include/asg_hip.h::asg_beam_word_window_nbest, with a look-ahead asg_beam_word_window_nbest_la), at most
        `window` steps per row; the scratch is kept on the stream per `nbest`, so a captured call replays.  nbest < 1 raises
        ValueError, nbest > 8192 RuntimeError."""
        if int(nbest) < 1:
            raise ValueError("torch_asg_amd: nbest must be >= 1, got %d" % int(nbest))
        nbest = min(int(nbest), (1 << 31) - 1)
        be = _asg.native()
        L = _lib.lib()
        B, dev, W = self.batch_size, self.device, self.window
        with be._guard(dev):
            what = "asg_beam_word_window_nbest" + ("" if self.lookahead is None else "_la")
            fn = getattr(L, what)

            def call(work, nbytes, *outs):
                return fn(None, *self._views, *self._look, B, self.beam_size, *self._shape, self._state.data_ptr(),
                          self._state.numel(), 1 if final else 0, nbest, work, nbytes, *outs)
            work = self._nbest_work.get(nbest)
            if work is None:
                abi_dtype = _lib.ASG_DTYPE_F32 if self.dtype == torch.float32 else _lib.ASG_DTYPE_F64
                nbytes = int(L.asg_beam_word_window_nbest_work_bytes(*self._views, B, abi_dtype, self.beam_size, *self._shape,
                                                                     nbest))
                if nbytes == 0:                                # the library refuses the arguments: its call says why
                    _lib.check(call(None, 0, *(None,) * 12, 0, None), what)
                work = self._nbest_work[nbest] = be._buf(nbytes, dev)
            scores = torch.empty(B, nbest, dtype=self.dtype, device=dev)
            wide = torch.empty(2, B, nbest, W, dtype=torch.int64, device=dev)  # tokens, words
            align = torch.empty(3, B, nbest, W, dtype=torch.int64, device=dev) if return_alignments else (None,) * 3
            lengths = torch.empty(2, B, nbest, dtype=torch.int64, device=dev)  # token_lengths, word_lengths
            narrow = torch.empty(4, B, dtype=torch.int64, device=dev)          # num_hyps, frames, committed, status
            al = lambda i: align[i].data_ptr() if return_alignments else None      # noqa: E731
            _lib.check(call(work.data_ptr(), work.numel(), scores.data_ptr(), al(0), wide[0].data_ptr(), lengths[0].data_ptr(),
                            al(1), al(2), wide[1].data_ptr(), lengths[1].data_ptr(), *[t.data_ptr() for t in narrow], 0,
                            be._stream(dev)), what)
        return BeamWordWindowNbest(scores, wide[0], lengths[0], wide[1], lengths[1], narrow[0], align[0], align[1], align[2],
                                   narrow[1], narrow[2], narrow[3])

    @staticmethod
    def _outputs(scores, wide, narrow):
        path, tokens, states, lm_states, words = wide
        token_lengths, word_lengths, frames, committed, status = narrow
        return BeamWordWindowResult(scores, path, tokens, token_lengths, states, lm_states, words, word_lengths, frames, committed,
                                    status)
