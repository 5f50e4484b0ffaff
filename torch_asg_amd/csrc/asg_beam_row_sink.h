// torch_asg_amd/csrc/asg_beam_row_sink.h -- the ROW SINK and the CELL machinery that the two n-best confidence calls share: the
// words of asg_beam_word_nbest_conf.hip and the tokens of asg_beam_nbest_conf.hip (5aa).  Every row of an n-best
// list is a list of (frame, id) in strictly ascending frame order; the posterior of "id at frame" does not depend on the row,
// so the rows only select CELLS.  Here, once:
//   - sort_u64: the bitonic network over the rows' queries frame << 32 | id, in LDS or over the workspace;
//   - (asg_beam_cells.inc, included inside the two prep kernels: the distinct queries in order -- the cells --, their number,
//     and the first cell of every frame;)
//   - RowSink: the sink of the beta pulls (asg_beam_word_conf_pull.h, asg_beam_conf_pull.h) that adds an event into the cells
//     whose window holds the frame the pull stands at -- accumulators in an LDS ring, an id mirror, a 256-bit id filter.
// Integer adds only: no order of arrival changes a bit, and a cell shared by rows has one value.
#pragma once
#include "asg_beam_lattice.h"     // kBL, to_fixed, bexp, bwd_front
#include "asg_beam_conf_sink.h"   // kConfScale: the fixed point of every sink

namespace asg {

namespace {

constexpr int kNP = 1024;                                     // prep / fill workgroup
constexpr int kSinkFixed = 1024;                              // window offsets int32 [2 * 64 + 2], then the filter u32 [8]
constexpr int kSinkFiltOff = 768;
static_assert((2 * kBeamWordConfMaxTol + 2) * 4 <= kSinkFiltOff && kSinkFiltOff + 32 <= kSinkFixed, "sink head");

// ascending bitonic network over v[0 .. P2), LDS or workspace (the workgroup's own stores are visible to it behind a barrier)
__device__ void sort_u64(unsigned long long *v, int P2) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < P2; x += kNP) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned long long a = v[x], c = v[y];
                    if ((a > c) == ((x & k) == 0)) { v[x] = c; v[y] = a; }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
}

// The row sink: the cells of EVERY row in (frame, word) order.  The cells whose window holds the frame the workgroup stands at
// are [ca, cb), the cells of nfr frames, the same in every thread; a cell's accumulator is slot (cell index & ring_mask) of the
// ring, its word sits in the same slot of the mirror mw, and fo holds the first cell of each open frame.
struct RowSink {
    static constexpr bool kBarrier = true;
    const int *foff;
    const unsigned long long *cells;
    unsigned long long *acc, *ring;
    int *mw, *fo;
    const unsigned *filt;
    int tol, T, ring_mask, ca, cb, nfr;
    // moves the range to frame t (frames descend), stores the cells that leave it -- no later event can reach them -- and
    // mirrors the words of those that enter
    __device__ __forceinline__ void window(int t) {
        const int tid = threadIdx.x;
        const int lo = t - tol < 0 ? 0 : (t - tol > T + 1 ? T + 1 : t - tol);
        const int hi = t + tol + 1 < 0 ? 0 : (t + tol + 1 > T + 1 ? T + 1 : t + tol + 1);
        const int nca = foff[lo], ncb = foff[hi];
        for (int c = ncb + tid; c < cb; c += kBL) {
            unsigned long long &slot = ring[c & ring_mask];
            acc[c] = slot;
            slot = 0ull;
        }
        for (int c = nca + tid; c < ca; c += kBL) mw[c & ring_mask] = (int) (unsigned) cells[c];
        nfr = hi - lo;
        for (int j = tid; j <= nfr; j += kBL) fo[j] = foff[lo + j];
        ca = nca;
        cb = ncb;
    }
    __device__ __forceinline__ bool open() const { return ca < cb; }
    // word w completed with posterior exp(x) at the frame the window stands at.  Within a frame the cells ascend in their
    // word, and a frame holds a word once: a binary search per open frame.
    template <typename R>
    __device__ __forceinline__ void add(int w, R x) {
        if (!((filt[((unsigned) w & 255u) >> 5] >> ((unsigned) w & 31u)) & 1u)) return;
        unsigned long long fx = 0ull;
        bool have = false;
        for (int j = 0; j < nfr; ++j) {
            int lo = fo[j];
            const int e1 = fo[j + 1];
            int hi = e1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mw[mid & ring_mask] < w) lo = mid + 1; else hi = mid;
            }
            if (lo < e1 && mw[lo & ring_mask] == w) {
                if (!have) { fx = to_fixed((double) bexp(x), kConfScale); have = true; }
                if (fx) atomicAdd(&ring[lo & ring_mask], fx);
            }
        }
    }
};

// the dynamic LDS of a pull with the row sink: the pull's front, the sink's head, ring (u64) and mirror (int32)
inline size_t sink_lds(int elem, int key, int M, size_t ring) { return bwd_front(elem, key, M) + kSinkFixed + ring * 12; }

inline size_t p2_size(size_t n) {
    size_t r = 2;
    while (r < n) r *= 2;
    return r;
}

}  // namespace

}  // namespace asg
