// torch_asg_amd/csrc/asg_beam_common.h -- what every beam unit shares: the order-preserving unsigned key of a value, the clamped
// length of an utterance, the 256-byte rounding of a workspace part (a256), and the ONE description per family of a search's
// workspace (beam_work for product states, beam_word_work for pairs), which the host sizes with and the kernels bind with
// (DESIGN.md 5q.1).
#pragma once
#include "asg_common.h"

namespace asg {

template <typename R> struct Key;
template <> struct Key<float> {
    using U = unsigned int;
    static constexpr int kBits = 32;
    static __device__ __forceinline__ U enc(float x) {
        const U b = __float_as_uint(x + 0.0f);              // -0 and +0 compare equal: one key (x + 0 is +0 for both)
        return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    static __device__ __forceinline__ float dec(U k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
};
template <> struct Key<double> {
    using U = unsigned long long;
    static constexpr int kBits = 64;
    static __device__ __forceinline__ U enc(double x) {
        const U b = (U) __double_as_longlong(x + 0.0);
        return (b >> 63) ? ~b : (b | (1ull << 63));
    }
    static __device__ __forceinline__ double dec(U k) {
        return __longlong_as_double((long long) ((k >> 63) ? (k & ~(1ull << 63)) : ~k));
    }
};

__device__ __forceinline__ int clamp_len(const int64_t *in_len, int b, int T) {
    if (!in_len) return T;
    const int64_t l = in_len[b];
    return (int) (l < 0 ? 0 : (l > T ? T : l));
}

// Every part of a workspace or a state starts on a multiple of 256 bytes.
__host__ __device__ inline size_t a256(size_t x) { return (x + 255) & ~(size_t) 255; }

constexpr int kResetBlocks = 64;   // workgroups of 256 threads per slot in a stream's reset of n entries
inline unsigned reset_blocks(size_t n) { return (unsigned) (n < 256 ? 1 : (n > 256 * (size_t) kResetBlocks ? kResetBlocks : (n + 255) / 256)); }

// The workspace of ONE utterance of the search over product states (asg_kernels.h, BeamGraphArgs), the one place its order and
// sizes are written down: the [T][K] lists bq (product state of each slot) and bs (its source's slot at t-1), arg u64 [Q], val
// key [Q], ckey key [cap], the touched list tl int32 [cap], and where it ends.  elem: the bytes of a key.  From base = (size_t) 0
// these are byte offsets and `end` is the size; from a workspace's address (char *) they are what a kernel binds.
template <typename P>
struct BeamWork {
    P bq, bs, arg, val, ckey, tl, end;
};
template <typename P>
__host__ __device__ inline BeamWork<P> beam_work(P base, int elem, int T, int Q, int K, int cap) {
    BeamWork<P> l;
    size_t off = 0;
    l.bq = base + off;    off += a256((size_t) T * K * 4);
    l.bs = base + off;    off += a256((size_t) T * K * 4);
    l.arg = base + off;   off += a256((size_t) Q * 8);
    l.val = base + off;   off += a256((size_t) Q * elem);
    l.ckey = base + off;  off += a256((size_t) cap * elem);
    l.tl = base + off;    off += a256((size_t) cap * 4);
    l.end = base + off;
    return l;
}

using BeamWorkLayout = BeamWork<size_t>;
__host__ __device__ inline BeamWorkLayout beam_work_layout(int elem, int T, int Q, int K, int cap) { return beam_work<size_t>(0, elem, T, Q, K, cap); }

// The same for the search over pairs (asg_kernels.h, WordLmArgs): the [T][K] lists bq, bh (LM state of each slot) and bs, the
// table of C = 1 << tbits slots -- tkey u64 [C], arg u64 [C], val key [C] --, ckey key [cap], cpair u64 [cap], tl int32 [cap].
template <typename P>
struct BeamWordWork {
    P bq, bh, bs, tkey, arg, val, ckey, cpair, tl, end;
};
template <typename P>
__host__ __device__ inline BeamWordWork<P> beam_word_work(P base, int elem, int T, int K, int cap, int tbits) {
    const size_t C = (size_t) 1 << tbits;
    BeamWordWork<P> l;
    size_t off = 0;
    l.bq = base + off;    off += a256((size_t) T * K * 4);
    l.bh = base + off;    off += a256((size_t) T * K * 4);
    l.bs = base + off;    off += a256((size_t) T * K * 4);
    l.tkey = base + off;  off += a256(C * 8);
    l.arg = base + off;   off += a256(C * 8);
    l.val = base + off;   off += a256(C * elem);
    l.ckey = base + off;  off += a256((size_t) cap * elem);
    l.cpair = base + off; off += a256((size_t) cap * 8);
    l.tl = base + off;    off += a256((size_t) cap * 4);
    l.end = base + off;
    return l;
}

using BeamWordWorkLayout = BeamWordWork<size_t>;
__host__ __device__ inline BeamWordWorkLayout beam_word_work_layout(int elem, int T, int K, int cap, int tbits) {
    return beam_word_work<size_t>(0, elem, T, K, cap, tbits);
}

}  // namespace asg
