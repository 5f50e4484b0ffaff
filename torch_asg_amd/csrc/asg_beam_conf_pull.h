// torch_asg_amd/csrc/asg_beam_conf_pull.h -- the beta pull with a TOKEN-EVENT SINK, the text asg_beam_conf.hip (confidences of the
// one best) and asg_beam_nbest_conf.hip (of every row of the n-best list, 5aa) both compile: beam_loss_bwd's pull
// through TokenLat<R> (one 1024-thread workgroup per utterance, frames len-1 .. 1, U_{t+1} with its beta in LDS, G lanes per
// source state, a max pass and a sum pass) without label posteriors, (i, j) tile and transition gradient.  The sum pass forms the
// posterior exp((alpha[t-1][p] + c) - Z_K) of every edge that is NOT the stay -- the event "a token with the label of the edge's
// target starts at frame t" -- and, behind the last frame of the loop, exp((alpha[0][q] + beta[0][q]) - Z_K) of every state of
// U_0, and hands each to the sink.  The adds and their order do not depend on the sink: beta and every event's value are the
// same bits under both.  A Sink is what asg_beam_word_conf_pull.h says it is, with "label" for "word": HypSink
// (asg_beam_conf_sink.h) or RowSink (asg_beam_row_sink.h).
#pragma once
#include "asg_beam_lattice.h"     // the helpers of the lattice pass: subgroup, find_sorted, the butterflies, to_fixed
#include "asg_beam_token_lat.h"   // TokenLat: how a product state's edges are walked (shared with asg_beam_loss.hip)
#include "asg_beam_conf_sink.h"   // HypSink, the ring and 2^54 (shared with the word confidences)

namespace asg {

namespace {

// Where the lattice rows of a frame lie.  FlatRows: frame t in row t, and the pull ends with the frame-0 term -- every caller
// with a workspace or a state of T rows.  A state that keeps its rows in a ring (asg_beam_conf_window.hip) passes a policy of its
// own: row(t) of the frames 0 .. len-1 it is called with, and first() -- whether its frame 0 is the utterance's.  (kFlat: the
// row of the top frame is chosen by a constant, not by a call of row() -- with the call the flat callers' kernels came out with
// another register allocation; this way their listings are the ones they had before there was a policy)
struct FlatRows {
    static constexpr bool kFlat = true;
    __device__ __forceinline__ int row(int t) const { return t; }
    __device__ __forceinline__ bool first() const { return true; }
};

// The beta pull with the token-event sink.  nb [M] / nq [M]: the dynamic LDS in front of the sink's ring (bwd_front).
// Lat: TokenLat<R>, or a lattice with its edges and labels and an end term of its own (the prefix mode of the lattice-keeping
// stream, asg_beam_stream_conf.hip); Lat::Args starts with TokenLat<R>::Args' members.  Rows: see FlatRows.
template <typename R, typename Sink, typename Lat = TokenLat<R>, typename Rows = FlatRows>
__device__ __forceinline__ void beam_conf_pull(const Problem &P, const typename Lat::Args &args, char *wb, size_t beta_off,
                                               R Z, int len, int last, int *nq, R *nb, Sink &sink, Rows rows = Rows{}) {
    using KeyT = int;
    const int M = args.lay.M, tid = threadIdx.x, b = blockIdx.x;
    const R NINF = Num<R>::ninf();
    const KeyT *U = (const KeyT *) (wb + args.lay.U);
    const int *nu = (const int *) (wb + args.lay.nu);
    const R *A = (const R *) (wb + args.lay.A);
    R *Bv = (R *) (wb + beta_off);                                             // [2][M]
    const R *in = (const R *) P.inputs + (int64_t) b * P.is1;
    const R *trm = (const R *) P.transition;
    Lat lat;
    lat.bind(args);
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };

    int top = len - 1;                                                         // the row of the last frame
    if constexpr (!Rows::kFlat) top = rows.row(len - 1);
    int mt = nu[top];
    for (int x = tid; x < mt; x += kBL) {
        const KeyT p = U[(int64_t) top * M + x];
        R e;
        lat.end(p, e);
        nq[x] = p;
        nb[x] = e;
    }
    for (int t = len - 1; t >= 1; --t) {
        __syncthreads();                                                       // nq, nb, the sink's LDS and the adds of frame t + 1
        sink.window(t);
        if constexpr (Sink::kBarrier) __syncthreads();
        const bool open = sink.open();
        const int mp = nu[rows.row(t - 1)];
        const KeyT *Up = U + (int64_t) rows.row(t - 1) * M;
        const R *Ap = A + (int64_t) rows.row(t - 1) * M;
        R *Brow = Bv + (int64_t) ((t - 1) & 1) * M;
        const R *xt = in + (int64_t) rows.row(t) * P.is0;
        const int G = subgroup(mp), per = kBL / G;
        for (int k0 = 0; k0 < mp; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mp;
            const KeyT pp = act ? Up[k] : (KeyT) 0;
            const int ip = act ? lat.label(pp) : 0;
            // every surviving candidate out of pp that this lane owns: f(value, label of the target, is it an edge)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_sorted(nq, mt, pp);
                    if (pos >= 0) f((nb[pos] + tr(ip, ip)) + xt[(int64_t) ip * P.is2], ip, false);
                }
                lat.for_each_out(pp, lg, G, [&](KeyT tp, auto w, int i) {
                    const int pos = find_sorted(nq, mt, tp);
                    if (pos >= 0) f(((nb[pos] + tr(i, ip)) + w()) + xt[(int64_t) i * P.is2], i, true);
                });
            };
            R mx = NINF;
            visit([&](R c, int, bool) { mx = bmax(mx, c); });
            mx = group_max(mx, G);
            R s = R(0);
            if (mx > NINF) {
                const R a = Ap[k];
                visit([&](R c, int i, bool edge) {
                    s += bexp(c - mx);
                    if (edge && open) sink.add(i, (a + c) - Z);
                });
            }
            s = group_sum(s, G);
            if (act && lg == 0) dev_store(Brow + k, mx > NINF ? mx + blog(s) : NINF);
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mp; x += kBL) { nq[x] = Up[x]; nb[x] = dev_load(Brow + x); }
        mt = mp;
    }
    // frame 0: every state of U_0 starts a token with its label
    __syncthreads();
    sink.window(0);
    if constexpr (Sink::kBarrier) __syncthreads();
    if (rows.first() && sink.open())
        for (int x = tid; x < mt; x += kBL) sink.add(lat.label(nq[x]), (A[x] + nb[x]) - Z);
    __syncthreads();
    sink.window(last);                                                         // every window is closed
}

// The tail of a one-best confidence kernel (beam_conf_bwd of asg_beam_conf.hip, beam_stream_conf_bwd of asg_beam_stream_conf.hip),
// behind the hypothesis -- pb: its path of len frames, tk: its n tokens -- and Z: token_frames from the path (one wavefront, the
// ballot / popcount walk of collapse_tokens, so token k's frame is the frame its label was kept at), the zero fill of the
// confidences, the ring, HypSink and the pull.  nb [M] / nq [M] / ring: the dynamic LDS (bwd_front, then kConfRing words).
template <typename R, typename Lat = TokenLat<R>>
__device__ __forceinline__ void beam_conf_tokens(const Problem &P, const typename Lat::Args &args, char *wb, size_t beta_off, R Z,
                                                 int len, int n, int T, int tol, const long long *pb, const long long *tk,
                                                 long long *tf, R *cf, unsigned long long *ring, int *nq, R *nb) {
    const int tid = threadIdx.x;
    // ---- where the tokens start: the frames at which collapse_tokens kept a label
    for (int k = n + tid; k < T; k += kBL) tf[k] = -1;
    if (tid < 64 && n > 0) {
        int base = 0;
        long long carry = -1;
        for (int c0 = 0; c0 < len; c0 += 64) {
            const int t = c0 + tid;
            const long long cur = t < len ? pb[t] : -1;
            long long prv = __shfl_up(cur, 1);
            if (tid == 0) prv = carry;
            const bool keep = t < len && cur != prv;
            const unsigned long long m = __ballot(keep);
            const int pre = base + __popcll(m & ((1ull << tid) - 1ull));
            if (keep && pre < n) tf[pre] = t;
            base += __popcll(m);
            carry = __shfl(cur, 63);
        }
    }
    const int nw = Z > Num<R>::ninf() ? n : 0;
    for (int k = nw + tid; k < T; k += kBL) cf[k] = R(0);
    if (nw == 0) return;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    __threadfence();                                                           // the frames, for the windows of every wavefront
    HypSink<R> sink;
    sink.wd = tk; sink.wf = tf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = nw;
    beam_conf_pull<R, HypSink<R>, Lat>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink);
}

}  // namespace

}  // namespace asg
