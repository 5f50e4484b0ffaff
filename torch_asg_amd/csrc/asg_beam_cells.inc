// torch_asg_amd/csrc/asg_beam_cells.inc -- the tail of the two prep kernels of the n-best confidence calls (nbest_conf_prep in
// asg_beam_word_nbest_conf.hip, beam_nbest_conf_prep in asg_beam_nbest_conf.hip), included INSIDE the kernel so that both compile
// one text: from the sorted queries v[0 .. nq) to the cells, their number in hdr[0] and the first cell of every frame in foff.
// In scope at the point of inclusion: tid, lane, wave (of a workgroup of kNP threads), v, nq, cells, hdr, foff, T, and the
// kernel's __shared__ int wsum[kNP / 64], run_s.
    // ---- the distinct queries, in order: a ballot per wavefront, the wavefronts' counts through LDS, strips of 1024
    if (tid == 0) run_s = 0;
    __syncthreads();
    for (int x0 = 0; x0 < nq; x0 += kNP) {
        const int x = x0 + tid;
        const unsigned long long me = x < nq ? v[x] : ~0ull;
        const bool head = x < nq && me != ~0ull && (x == 0 || v[x - 1] != me);
        const unsigned long long m = __ballot(head);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int pre = run_s;
        for (int s = 0; s < wave; ++s) pre += wsum[s];
        if (head) cells[pre + __popcll(m & ((1ull << lane) - 1ull))] = me;
        __syncthreads();
        if (tid == kNP - 1) run_s = pre + __popcll(m);
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    const int nc = run_s;
    if (tid == 0) hdr[0] = nc;
    // ---- the first cell of every frame 0 .. T + 1 (the words live at frames 1 .. len, the tokens at 0 .. len - 1)
    for (int u = tid; u < T + 2; u += kNP) {
        const unsigned long long key = (unsigned long long) u << 32;
        int lo = 0, hi = nc;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cells[mid] < key) lo = mid + 1; else hi = mid;
        }
        foff[u] = lo;
    }
