// torch_asg_amd/csrc/asg_beam_common.h -- device helpers shared by the beam search (asg_beam_graph.hip) and the n-best stage
// behind it (asg_beam_nbest.hip): the order-preserving unsigned key of a value, and the clamped length of an utterance.
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

}  // namespace asg
