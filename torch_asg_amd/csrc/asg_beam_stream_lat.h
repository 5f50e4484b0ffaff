// torch_asg_amd/csrc/asg_beam_stream_lat.h -- what a growing beam stream's PLAIN state and its LATTICE-KEEPING state share besides
// the frame body, for both families (product states: asg_beam_stream.hip / asg_beam_stream_conf.hip; pairs:
// asg_beam_word_stream.hip / asg_beam_word_stream_conf.hip).  DESIGN.md 5af.
//   - the header of a slot and the clamped reads of it;
//   - the KEEP POLICY of the advance kernel: there is one advance kernel per family, a template over what it keeps besides the
//     search's own rows.  KeepNone keeps nothing and is empty: the plain kernel has no argument, branch or LDS byte for it.
//     KeepLattice carries the slot's cnt / em offsets and adds three writes (the chunk's emissions, |A_t| of every frame, 0 for
//     the frames an empty beam skips).  "The same sets and values" under both is therefore the text, not a promise;
//   - the hypothesis of a slot (winner, score, backtrace, collapse, padding), which a stream's result kernel and the confidence
//     kernel of its lattice-keeping state both start with;
//   - the front of the catch-up: frames [apos, pos) from the header, and U_t = the keys of A_t sorted, nu[t] = |A_t|.
#pragma once
#include "asg_beam_word_frame.h"  // (and asg_beam_frame.h): the ends and backtraces of both searches
#include "asg_beam_lattice.h"     // kBL, bitonic_sort_wg

namespace asg {

namespace {

// The header of a slot: int32 pos (frames consumed), |A| (size of the stored set), overflow, apos (the frames whose U / nu / A
// rows are valid; a plain state has no such rows and never reads the word).  A reset zeroes all four.
constexpr int kHdrWords = 4;
constexpr int kHdrApos = 3;

// A state that was reset holds 0 <= pos <= max_frames, 0 <= |A| <= K (nothing before the first frame) and 0 <= apos <= pos.
__device__ __forceinline__ int stream_pos(const int *hdr, int max_frames) {
    const int pos = hdr[0];
    return pos < 0 ? 0 : (pos > max_frames ? max_frames : pos);
}
__device__ __forceinline__ int stream_na(const int *hdr, int pos, int K) {
    const int na = pos >= 1 ? hdr[1] : 0;
    return na < 0 ? 0 : (na > K ? K : na);
}
__device__ __forceinline__ int stream_apos(const int *hdr, int pos) {
    const int a = hdr[kHdrApos];
    return a < 0 ? 0 : (a > pos ? pos : a);
}

// What the advance kernel keeps of a chunk besides the rows of the search.  chunk: before the frames, the chunk's n frames
// at rows pos .. pos+n-1; frame: behind frame gt, which left na states; skipped: behind the loop, which ran t of the n frames.
struct KeepNone {
    template <typename R> __device__ __forceinline__ void chunk(char *, const R *, const Problem &, int, int) const {}
    __device__ __forceinline__ void frame(char *, int, int) const {}
    __device__ __forceinline__ void skipped(char *, int, int, int) const {}
};
struct KeepLattice {
    size_t cnt, em;              // byte offsets in the slot: int32 [max_frames], emissions [max_frames][N]
    // (coalesced, the whole workgroup; nothing reads the rows before the next launch)
    template <typename R> __device__ __forceinline__ void chunk(char *wb, const R *in, const Problem &P, int pos, int n) const {
        R *e = (R *) (wb + em);
        const int N = P.N;
        for (int64_t x = threadIdx.x; x < (int64_t) n * N; x += kBT) {
            const int64_t t = x / N, i = x % N;
            e[(int64_t) pos * N + x] = in[t * P.is0 + i * P.is2];
        }
    }
    __device__ __forceinline__ void frame(char *wb, int gt, int na) const {
        if (threadIdx.x == 0) ((int *) (wb + cnt))[gt] = na;
    }
    __device__ __forceinline__ void skipped(char *wb, int pos, int t, int n) const {
        for (int u = t + threadIdx.x; u < n; u += kBT) ((int *) (wb + cnt))[pos + u] = 0;
    }
};

// The hypothesis of slot blockIdx.x of a token-graph stream: frames and status, the best end over the stored set (with the final
// weights or without), the score from the winner's own sum (the key folds -0 into +0), the backtrace over len frames, the token
// collapse, the padding.  It only reads the state.  Returns the winner's key: 0 where there is no frame yet, an empty set or no
// finite end -- then the outputs say "no path".
template <typename R>
__device__ __forceinline__ typename Key<R>::U beam_stream_hyp(Ctl<typename Key<R>::U> &ctl, const GraphArgs &g, int K, int cap, int T,
                                                              const char *wb, const BeamStreamLayout &lay, int final, R *scores,
                                                              long long *path, long long *tokens, long long *tlen,
                                                              long long *states, long long *frames, long long *status, int &len) {
    using U = typename Key<R>::U;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int *hdr = (const int *) (wb + lay.hdr);
    const R *set_v = (const R *) (wb + lay.set);
    const int *set_q = (const int *) (set_v + K);
    const BeamWorkLayout wl = beam_work_layout(sizeof(R), T, g.Q, K, cap);
    const int *bq = (const int *) (wb + wl.bq), *bs = (const int *) (wb + wl.bs);             // [max_frames][K]
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    len = stream_pos(hdr, T);
    const int na = stream_na(hdr, len, K);
    if (tid == 0) { frames[b] = len; status[b] = hdr[2] != 0; }
    const R *fw = final ? (const R *) g.final_w : nullptr;
    U bkey;
    int bqq, bk;
    beam_best_end<R>(ctl, set_q, set_v, na, fw, bkey, bqq, bk);
    if (bkey == 0) {
        beam_no_path(T, pb, tk, st, tlen + b);
        if (tid == 0) scores[b] = Num<R>::ninf();
        return bkey;
    }
    if (tid == 0) scores[b] = fw ? set_v[bk] + fw[bqq] : set_v[bk];
    beam_backtrace(bq, bs, K, len, T, bk, g.label, g.state, pb, tk, st, tlen + b);
    return bkey;
}

// The same for a stream over pairs: the end of the one-shot decoder or the best prefix, the backtrace, the words, the token
// collapse, the padding.  f: bound here to the graph, the LM, the look-ahead and the slot's rows (only read).
template <typename R, bool LA>
__device__ __forceinline__ typename Key<R>::U beam_word_stream_hyp(BeamWordFrame<R, LA> &f, WordCtl &wctl, const GraphArgs &g,
                                                                   const WordLmArgs &lm, const WordLookParam<LA> &la, int K, int cap,
                                                                   int tbits, int T, char *wb, const BeamStreamLayout &lay,
                                                                   bool final, R *scores, long long *path, long long *tokens,
                                                                   long long *tlen, long long *states, long long *lm_states,
                                                                   long long *words, long long *wlen, long long *frames,
                                                                   long long *status, int &len) {
    using U = typename Key<R>::U;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int *hdr = (const int *) (wb + lay.hdr);
    const R *set_v = (const R *) (wb + lay.set);
    const int *set_q = (const int *) (set_v + K);
    const int *set_h = set_q + K;
    long long *pb = path + (int64_t) b * T, *tk = tokens + (int64_t) b * T, *st = states + (int64_t) b * T;
    long long *ls = lm_states + (int64_t) b * T, *wd = words + (int64_t) b * T;
    f.ctl = nullptr; f.wctl = &wctl; f.cur_v = nullptr; f.cur_q = nullptr; f.cur_h = nullptr; f.trs = nullptr; f.tr = nullptr;
    f.ts0 = 0; f.ts1 = 0; f.N = 0; f.theta = (R) 0;
    bind_graph<R>(f, g, BeamGraphArgs{}, lm, K, cap, tbits);
    bind_look<R>(f, la);
    int *bq, *bh, *bs;
    f.bind_work(wb, T, bq, bh, bs);
    len = stream_pos(hdr, T);
    const int na = stream_na(hdr, len, K);
    if (tid == 0) { frames[b] = len; status[b] = hdr[2] != 0; }
    const R *fw = (const R *) g.final_w;
    U bkey;
    int bk;
    word_best_end<R, LA>(f, fw, final, set_h, set_q, set_v, na, bkey, bk);
    if (bkey == 0) {
        word_no_path(T, pb, tk, st, ls, wd, tlen + b, wlen + b);
        if (tid == 0) scores[b] = Num<R>::ninf();
        return bkey;
    }
    word_backtrace<R, LA>(f, fw, final, set_h, set_q, set_v, bk, bq, bh, bs, len, T, scores + b, pb, tk, st, ls, wd, tlen + b,
                          wlen + b);
    return bkey;
}

// The front of a catch-up, frames [a0, L): U_t = the keys of A_t ascending (bitonic in LDS: v holds P2(K) keys; the kept members
// of a frame are distinct, so the ascending list is what beam_loss_sets leaves without targets), nu[t] = |A_t|.  key_of(t, x):
// the key of slot x of frame t; pad: a key above all of them.
template <typename KeyT, typename KeyOf>
__device__ __forceinline__ void stream_lat_sets(int a0, int L, int K, const int *cnt, KeyT *v, KeyT pad, KeyT *U, int *nu,
                                                KeyOf key_of) {
    const int tid = threadIdx.x;
    for (int t = a0; t < L; ++t) {
        int na = cnt[t];
        na = na < 0 ? 0 : (na > K ? K : na);
        int p2 = 2;
        while (p2 < na) p2 *= 2;
        for (int x = tid; x < p2; x += kBL) v[x] = x < na ? key_of(t, x) : pad;
        __syncthreads();
        bitonic_sort_wg<KeyT, kBL>(v, p2);
        KeyT *Ut = U + (int64_t) t * K;
        for (int x = tid; x < na; x += kBL) Ut[x] = v[x];
        if (tid == 0) nu[t] = na;
        __syncthreads();                                 // v is the next frame's
    }
    __threadfence();
    __syncthreads();
}

}  // namespace

}  // namespace asg
