// torch_asg_amd/csrc/asg_beam_word_conf_pull.h -- the beta pull with a WORD-EVENT SINK, the text asg_beam_word_conf.hip
// (confidences of the one best), asg_beam_word_nbest_conf.hip (of every row of the n-best list, 5y) and
// asg_beam_word_stream_conf.hip (of a stream's hypothesis or prefix, 5ae) all compile:
// beam_loss_bwd's pull (one 1024-thread workgroup per utterance, frames len-1 .. 1, U_{t+1} with its beta in LDS, G lanes per
// source pair, a max pass and a sum pass) without label posteriors, (i, j) tile and transition gradient.  The sum pass forms the
// posterior exp((alpha + c) - Z_K) of every SEPARATOR edge -- the event "word w ends at frame t" -- and, before the first frame,
// the posteriors of the final step, and hands each to the sink.  The adds and their order do not depend on the sink: beta and
// every event's value are the same bits under both.  A Sink has
//   kBarrier          whether `window` writes LDS that `add` reads (then a barrier follows it)
//   window(t)         every thread, frames descending from len, at last with a t whose windows are all closed: moves the open
//                     range to frame t and finishes what leaves it
//   open()            whether anything is open at the frame the sink stands at (the same in every thread)
//   add(w, x)         word w completed with posterior exp(x) at that frame
// nq [M] / nb [M]: the dynamic LDS in front of the sink's own (bwd_front).  beta[t-1] crosses from the lanes that sum it to the
// workgroup through the utterance's two rows in the workspace at beta_off, as in beam_loss_bwd.
#pragma once
#include "asg_beam_lattice.h"
#include "asg_beam_word_lat.h"
#include "asg_beam_conf_sink.h"   // kConfScale: the fixed point of every sink

namespace asg {

namespace {

// Lat: WordLat<R>, or a lattice with its edges and labels, an end term of its own and its own answer to whether the event of
// frame len exists (the prefix mode of the lattice-keeping stream, asg_beam_word_stream_conf.hip); Lat::Args starts with
// WordLat<R>::Args' members.
template <typename R, typename Sink, typename Lat = WordLat<R>>
__device__ __forceinline__ void beam_word_conf_pull(const Problem &P, const typename Lat::Args &args, char *wb, size_t beta_off,
                                                    R Z, int len, int last, unsigned long long *nq, R *nb, Sink &sink) {
    using KeyT = unsigned long long;
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
    const int sep = lat.f.sep;
    auto tr = [&](int i, int j) -> R { return trm[(int64_t) i * P.ts0 + (int64_t) j * P.ts1]; };
    __syncthreads();                                                           // the sink's LDS is ready

    // frame len: the final step out of the word-end nodes of the last set
    sink.window(len);
    if constexpr (Sink::kBarrier) __syncthreads();
    int mt = nu[len - 1];
    for (int x = tid; x < mt; x += kBL) {
        const KeyT p = U[(int64_t) (len - 1) * M + x];
        R e;
        lat.end(p, e);
        nq[x] = p;
        nb[x] = e;
        const int s = lat.f.state[(int) (p & lat.qmask)];
        if (lat.end_event() && sink.open() && s != 0 && e > NINF) sink.add(lat.f.wos[s], (A[(int64_t) (len - 1) * M + x] + e) - Z);
    }
    for (int t = len - 1; t >= 1; --t) {
        __syncthreads();                                                       // nq, nb and the adds of frame t + 1
        sink.window(t);
        if constexpr (Sink::kBarrier) __syncthreads();
        const bool open = sink.open();
        const int mp = nu[t - 1];
        const KeyT *Up = U + (int64_t) (t - 1) * M;
        const R *Ap = A + (int64_t) (t - 1) * M;
        R *Brow = Bv + (int64_t) ((t - 1) & 1) * M;
        const R *xt = in + (int64_t) t * P.is0;
        const int G = subgroup(mp), per = kBL / G;
        for (int k0 = 0; k0 < mp; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mp;
            const KeyT pp = act ? Up[k] : (KeyT) 0;
            const int ip = act ? lat.label(pp) : 0;
            // every surviving candidate out of pp that this lane owns: f(value, is it a separator edge)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_sorted(nq, mt, pp);
                    if (pos >= 0) f((nb[pos] + tr(ip, ip)) + xt[(int64_t) ip * P.is2], false);
                }
                lat.for_each_out(pp, lg, G, [&](KeyT tp, auto w, int i) {
                    const int pos = find_sorted(nq, mt, tp);
                    if (pos >= 0) f(((nb[pos] + tr(i, ip)) + w()) + xt[(int64_t) i * P.is2], i == sep);
                });
            };
            R mx = NINF;
            visit([&](R c, bool) { mx = bmax(mx, c); });
            mx = group_max(mx, G);
            R s = R(0);
            if (mx > NINF) {
                const R a = Ap[k];
                const int w = open ? lat.f.wos[lat.f.state[(int) (pp & lat.qmask)]] : -1;
                visit([&](R c, bool word) {
                    s += bexp(c - mx);
                    if (word && open) sink.add(w, (a + c) - Z);
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
    __syncthreads();
    sink.window(last);                                                         // every window is closed
}

// Where the words of a hypothesis end, behind word_backtrace (pb: its path of len frames, *wlen: its word count): the frames of
// the separator edges word_backtrace read its words from, then len for the word of a final step (the one word it appended behind
// them; a prefix has none: its word count is the separator count).  Every thread of the search's or the pull's workgroup.
static_assert(kBT == kBL, "word_end_frames strides by either workgroup");
__device__ __forceinline__ void word_end_frames(const long long *pb, int sep, int len, int T, const long long *wlen, long long *wf) {
    for (int u = threadIdx.x; u < T; u += kBL) wf[u] = -1;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        int nw = 0;
        for (int u = 1; u < len; ++u)
            if (pb[u] == sep && pb[u - 1] != sep) wf[nw++] = u;
        if (nw < (int) *wlen) wf[nw] = len;
    }
}

// The tail of a one-best confidence kernel (beam_word_conf_bwd of asg_beam_word_conf.hip, beam_word_stream_conf_bwd of
// asg_beam_word_stream_conf.hip), behind Z and the count nw of the hypothesis' words that get a confidence: the zero fill, the ring,
// HypSink over the words wd and their frames wf, and the pull.  nq [M] / nb [M] / ring: the dynamic LDS (bwd_front, then kConfRing
// words).
template <typename R, typename Lat = WordLat<R>>
__device__ __forceinline__ void beam_word_conf_words(const Problem &P, const typename Lat::Args &args, char *wb, size_t beta_off, R Z,
                                                     int len, int nw, int T, int tol, const long long *wd, const long long *wf, R *cf,
                                                     unsigned long long *ring, unsigned long long *nq, R *nb) {
    const int tid = threadIdx.x;
    for (int k = nw + tid; k < T; k += kBL) cf[k] = R(0);
    if (nw == 0) return;
    for (int x = tid; x < kConfRing; x += kBL) ring[x] = 0ull;
    HypSink<R> sink;
    sink.wd = wd; sink.wf = wf; sink.cf = cf; sink.ring = ring; sink.tol = tol;
    sink.ka = sink.kb = nw;
    beam_word_conf_pull<R, HypSink<R>, Lat>(P, args, wb, beta_off, Z, len, -tol - 1, nq, nb, sink);
}

}  // namespace

}  // namespace asg
