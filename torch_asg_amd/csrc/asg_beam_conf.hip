// torch_asg_amd/csrc/asg_beam_conf.hip -- TOKEN CONFIDENCES and START FRAMES of the token-graph beam decoder's hypothesis, from the
// lattice its own search kept, on gfx950.  The specification is include/asg_hip.h::asg_beam_graph_confidence;
// tests/beam_conf_ref.py restates it in numpy.
//
// Five launches on one stream:
//   1 - 4  launch_beam_loss_lattice (asg_beam_loss.hip), the forward of the beam-pruned loss without targets and with alpha stored
//      for every frame: beam_graph_kernel as the decoder runs it -- asked for |A_t| of every frame, and writing the CALLER's five
//      decoder outputs, so they have asg_beam_decode_graph's bits --, the target walk (there is no target: it writes the header's
//      0), beam_loss_sets<TokenSets> and beam_loss_fwd -> U_t = A_t sorted, alpha, Z_K (the normalisers).  Unchanged kernels.
//   5  beam_conf_bwd: first token_frames from the path the search just wrote (one wavefront, the ballot / popcount walk of
//      collapse_tokens, so token k's frame is the frame its label was kept at).  Then beam_loss_bwd's beta pull through
//      TokenLat<R> (one 1024-thread workgroup per utterance, frames len-1 .. 1, U_{t+1} with its beta in LDS, G = subgroup(|U_t|)
//      lanes per source state, a max pass and a sum pass, beta handed on through two workspace rows) with the same adds in the same
//      order, and without label posteriors, (i, j) tile, grad_inputs and reduction launch.  The sum pass also forms the
//      posterior exp((alpha[t-1][p] + c) - Z_K) of every edge that is NOT the stay -- the event "a token with the label of the
//      edge's target starts at frame t" -- and, behind the last frame of the loop, exp((alpha[0][q] + beta[0][q]) - Z_K) of every
//      state of U_0: the tokens that start at frame 0.  An event goes to HypSink (asg_beam_conf_sink.h, the sink of the word
//      confidences): the tokens of the hypothesis whose window [s_k - tol, s_k + tol] holds the frame are one index range that
//      only moves down, an event is added as a 64-bit fixed-point integer with 54 fractional bits to every token of the range
//      that has its label, slot k mod 256 of a ring in LDS; a token that leaves the range is converted, stored and its slot
//      zeroed.  Integer adds only, no float atomics: no order of arrival changes a bit.  Every output and every workspace word
//      that is read is written by these kernels: no memset, no host synchronisation, the call captures and replays.
// The pull (asg_beam_conf_pull.h, a template over the sink: asg_beam_nbest_conf.hip compiles it with the rows' sink) is a
// sibling of beam_word_conf_pull (asg_beam_word_conf_pull.h), not that template over another lattice type: what an
// event is (every edge but the stay, named by the target's label, against a separator edge named by the source's word), the
// final step (none here) and the step at frame 0 (none there) all differ; the sink, the ring and 2^54 are shared.
#include "asg_common.h"
#include "asg_kernels.h"
#include "asg_beam_common.h"
#include "asg_beam_lattice.h"     // the helpers of the lattice pass: subgroup, find_sorted, the butterflies, to_fixed
#include "asg_beam_token_lat.h"   // TokenLat: how a product state's edges are walked (shared with asg_beam_loss.hip)
#include "asg_beam_conf_sink.h"   // HypSink, the ring and 2^54 (shared with asg_beam_word_conf.hip)
#include "asg_beam_conf_pull.h"   // the beta pull over a sink (shared with asg_beam_nbest_conf.hip)

namespace asg {

namespace {

static_assert(kBeamConfMaxTol == kBeamWordConfMaxTol, "the ring of HypSink is sized by the word call's tolerance");

inline size_t conf_lds(int elem, int M) { return bwd_front(elem, 4, M) + (size_t) kConfRing * 8; }

// 5.  Dynamic LDS: [nb R M][nq int M][pad to 16][ring u64 256].
template <typename R>
__global__ void __launch_bounds__(kBL) beam_conf_bwd(Problem P, typename TokenLat<R>::Args args, char *work, size_t beta_off,
                                                     const R *Zs, const long long *path, const long long *tokens,
                                                     const long long *tlen, int tol, long long *tframes, R *conf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int M = args.lay.M, T = P.T;
    R *nb = (R *) lds;                                                         // [M] beta[t] of U_t
    int *nq = (int *) (lds + (size_t) M * sizeof(R));                          // [M] U_t
    unsigned long long *ring = (unsigned long long *) (lds + bwd_front(sizeof(R), 4, M));
    const int b = blockIdx.x;
    const int len = clamp_len(P.in_len, b, T);
    const R Z = Zs[b];
    const long long *pb = path + (int64_t) b * T;
    long long *tf = tframes + (int64_t) b * T;
    R *cf = conf + (int64_t) b * T;
    int n = 0;
    if (len >= 1) {
        const long long l = tlen[b];
        n = (int) (l < 0 ? 0 : (l > len ? len : l));                           // (a path of len frames starts at most len tokens)
    }
    beam_conf_tokens<R>(P, args, work + (size_t) b * args.lay.per, beta_off, Z, len, n, T, tol, pb, tokens + (int64_t) b * T, tf, cf,
                        ring, nq, nb);
}

}  // namespace

BeamConfLayout beam_conf_layout(int elem, int T, int Q, int K, int cap) {
    BeamConfLayout l{};
    l.lat = beam_loss_layout(elem, T, Q, K, cap, 0, true);
    l.beta = l.lat.per;
    l.per = l.beta + a256(2 * (size_t) l.lat.M * elem);
    l.lat.per = l.per;
    return l;
}

size_t beam_conf_work_bytes(int elem, int T, int B, int Q, int K, int cap) {
    return (size_t) B * beam_conf_layout(elem, T, Q, K, cap).per;
}

template <typename R>
hipError_t launch_beam_conf(const Problem &P0, const GraphArgs &G, const BeamGraphArgs &BG, const BeamLossArgs &L, int K, double theta,
                            int tol, void *work, void *scores, long long *path, long long *tokens, long long *tlen,
                            long long *states, long long *token_frames, void *token_conf, void *normalisers, hipStream_t stream) {
    Problem P = P0;
    P.targets = nullptr;                                                         // the lattice of the search alone: U_t = A_t
    P.tg_len = nullptr;
    const int cap = beam_graph_cap(G.Q, K, BG.max_out, BG.num_start);
    const BeamConfLayout lay = beam_conf_layout(sizeof(R), P.T, G.Q, K, cap);
    hipError_t e = launch_beam_loss_lattice<R>(P, G, BG, L, lay.lat, K, theta, true, work, normalisers, scores, path, tokens, tlen,
                                               states, 0, stream);
    if (e != hipSuccess) return e;
    const size_t dyn = conf_lds(sizeof(R), lay.lat.M);
    set_lds((const void *) beam_conf_bwd<R>, dyn);
    hipLaunchKernelGGL((beam_conf_bwd<R>), dim3(P.B), dim3(kBL), dyn, stream, P, typename TokenLat<R>::Args{G, BG, lay.lat},
                       (char *) work, lay.beta, (const R *) normalisers, (const long long *) path, (const long long *) tokens,
                       (const long long *) tlen, tol, token_frames, (R *) token_conf);
    return hipGetLastError();
}

#define ASG_BEAM_CONF_INST(R)                                                                                                  \
    template hipError_t launch_beam_conf<R>(const Problem &, const GraphArgs &, const BeamGraphArgs &, const BeamLossArgs &, int, \
                                            double, int, void *, void *, long long *, long long *, long long *, long long *,   \
                                            long long *, void *, void *, hipStream_t);
ASG_BEAM_CONF_INST(float)
ASG_BEAM_CONF_INST(double)
#undef ASG_BEAM_CONF_INST

}  // namespace asg
