// torch_asg_amd/csrc/asg_beam_conf_sink.h -- the EVENT SINK of one hypothesis that the confidence calls share: the words of
// asg_beam_word_conf.hip and the tokens of asg_beam_conf.hip (5z) are both a list of (item, frame) in strictly
// ascending frame order, an event is "item w at the frame the pull stands at", and an item's accumulator is a slot of a ring of
// 64-bit fixed-point integers in LDS.  Integer adds only: no order of arrival changes a bit.
#pragma once
#include "asg_beam_lattice.h"    // kBL, to_fixed, bexp

namespace asg {

namespace {

constexpr double kConfScale = 18014398509481984.0;            // 2^54: a word sums at most 129 completions of at most 1 (+ rounding)

constexpr int kConfRing = 256;                                // >= 2 * kBeamWordConfMaxTol + 2, a power of two
static_assert(kConfRing >= 2 * kBeamWordConfMaxTol + 2 && (kConfRing & (kConfRing - 1)) == 0, "ring");

// 5x's sink: the words of ONE hypothesis in frame order.  The words whose window holds the frame the workgroup stands at are
// [ka, kb), the same in every thread; a word's accumulator is slot k mod 256 of the ring.
template <typename R>
struct HypSink {
    static constexpr bool kBarrier = false;
    const long long *wd, *wf;
    R *cf;
    unsigned long long *ring;
    int tol, ka, kb;
    // moves the range to frame t (frames descend) and finishes the words that leave it: no later event can reach them
    __device__ __forceinline__ void window(int t) {
        const int tid = threadIdx.x;
        int nkb = kb;
        while (nkb > 0 && wf[nkb - 1] > (long long) t + tol) --nkb;
        for (int k = nkb + tid; k < kb; k += kBL) {
            unsigned long long &slot = ring[k & (kConfRing - 1)];
            cf[k] = (R) ((double) slot * (1.0 / kConfScale));
            slot = 0ull;
        }
        kb = nkb;
        if (ka > kb) ka = kb;
        while (ka > 0 && wf[ka - 1] >= (long long) t - tol) --ka;
    }
    __device__ __forceinline__ bool open() const { return ka < kb; }
    // word w completed with posterior exp(x) at the frame the window stands at
    __device__ __forceinline__ void add(int w, R x) {
        unsigned long long fx = 0ull;
        bool have = false;
        for (int k = ka; k < kb; ++k) {
            if (wd[k] != (long long) w) continue;
            if (!have) { fx = to_fixed((double) bexp(x), kConfScale); have = true; }
            if (fx) atomicAdd(&ring[k & (kConfRing - 1)], fx);
        }
    }
};

}  // namespace

}  // namespace asg
