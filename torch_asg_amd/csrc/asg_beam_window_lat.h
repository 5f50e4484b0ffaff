// torch_asg_amd/csrc/asg_beam_window_lat.h -- what the token window stream's PLAIN state and its LATTICE-KEEPING state
// (asg_beam_conf_window.hip) share besides the search and the commit attempt: the KEEP POLICY of
// beam_window_advance_kernel, as asg_beam_stream_lat.h has it for the growing streams (5af).  WinKeepNone keeps nothing and is
// empty: the plain kernel has no argument, branch or LDS byte for it.  WinKeepLattice carries the offsets of the slot's lattice
// RING -- RW rows, frame t in row t mod RW, computed in 64 bits -- and the call's new_token_frames, and adds
//   - the chunk's emissions and |A_t| of every frame (0 for the frames an empty beam skips), as KeepLattice does;
//   - the kept states of a frame, UNSORTED, into the frame's U row: the search's own ring bq has only W rows, and a commit attempt
//     reads up to tol + 1 frames below the oldest live one (the catch-up sorts the row in place);
//   - one entry of the ATTEMPT LOG per commit attempt that committed a token: p1 (pos, counting the attempt's frame), the base
//     before the attempt, and the tokens' range in this call's output row;
//   - the padding of new_token_frames and the number of logged attempts.
// The header words of the lattice-keeping state sit in the slot's 256-byte header behind TokenWinHdr, which stays as it is.
#pragma once
#include "asg_beam_frame.h"

namespace asg {

namespace {

constexpr size_t kConfWinHdrOff = 64;        // ConfWinHdr inside the slot's header block (TokenWinHdr is 32 bytes)
// apos: the frames whose U / nu / A rows are valid (0 <= pos - apos <= max_chunk between calls); nlog: the attempts the last
// advance logged.
struct ConfWinHdr {
    long long apos;
    int nlog;
};
static_assert(kConfWinHdrOff + sizeof(ConfWinHdr) <= 256, "header");

// One logged attempt: the lattice ends at frame p1 - 1, the attempt found base b0 and committed tokens [k0, k1) of the call.
struct WinAttempt {
    long long p1, b0;
    int k0, k1;
};

// chunk: before the frames, n frames at pos ..; frame: behind frame gt, which left na states in `bqrow`; skipped: behind the
// loop, which ran t of the n frames; attempt: behind a commit attempt; done: behind everything, ntok tokens committed.
struct WinKeepNone {
    static constexpr bool kLattice = false;
    template <typename R> __device__ __forceinline__ void chunk(char *, const R *, const Problem &, long long, int) const {}
    __device__ __forceinline__ void frame(char *, long long, int, const int *, int) const {}
    __device__ __forceinline__ void skipped(char *, long long, int, int) const {}
    __device__ __forceinline__ void attempt(char *, int, long long, long long, int, int) const {}
    __device__ __forceinline__ void done(char *, int, int, long long) const {}
};
struct WinKeepLattice {
    static constexpr bool kLattice = true;
    size_t hdr, cnt, em, U, log;     // byte offsets in the slot: the header block, int32 [RW], emissions [RW][N], int32 [RW][K], log
    int RW, nlog;                    // rows of the ring; entries of the log
    long long *tf;                   // new_token_frames [B][cols]
    __device__ __forceinline__ int row(long long t) const { return (int) (t % RW); }
    // (apos <= pos: a reset leaves pos = 0, and the rows of the utterance before it are nobody's)
    template <typename R> __device__ __forceinline__ void chunk(char *wb, const R *in, const Problem &P, long long pos, int n) const {
        if (threadIdx.x == 0) {
            ConfWinHdr *h = (ConfWinHdr *) (wb + hdr + kConfWinHdrOff);
            const long long a = h->apos;
            h->apos = a < 0 ? 0 : (a > pos ? pos : a);
        }
        R *e = (R *) (wb + em);
        const int N = P.N;
        for (int64_t x = threadIdx.x; x < (int64_t) n * N; x += kBT) {
            const int64_t t = x / N, i = x % N;
            e[(int64_t) row(pos + t) * N + i] = in[t * P.is0 + i * P.is2];
        }
    }
    __device__ __forceinline__ void frame(char *wb, long long gt, int na, const int *bqrow, int K) const {
        const int r = row(gt);
        int *u = (int *) (wb + U) + (int64_t) r * K;
        for (int x = threadIdx.x; x < na; x += kBT) u[x] = bqrow[x];
        if (threadIdx.x == 0) ((int *) (wb + cnt))[r] = na;
    }
    __device__ __forceinline__ void skipped(char *wb, long long pos, int t, int n) const {
        for (int u = t + threadIdx.x; u < n; u += kBT) ((int *) (wb + cnt))[row(pos + u)] = 0;
    }
    __device__ __forceinline__ void attempt(char *wb, int at, long long p1, long long b0, int k0, int k1) const {
        if (threadIdx.x == 0 && at < nlog) {
            WinAttempt *a = (WinAttempt *) (wb + log) + at;
            a->p1 = p1; a->b0 = b0; a->k0 = k0; a->k1 = k1;
        }
    }
    __device__ __forceinline__ void done(char *wb, int logged, int ntok, long long cols) const {
        long long *row_tf = tf + (int64_t) blockIdx.x * cols;
        for (long long x = ntok + threadIdx.x; x < cols; x += kBT) row_tf[x] = -1;
        if (threadIdx.x == 0) ((ConfWinHdr *) (wb + hdr + kConfWinHdrOff))->nlog = logged < nlog ? logged : nlog;
    }
};

}  // namespace

}  // namespace asg
