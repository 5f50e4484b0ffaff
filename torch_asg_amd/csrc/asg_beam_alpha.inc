// torch_asg_amd/csrc/asg_beam_alpha.inc -- the FRAME BODY of the alpha pull over the kept sets of the token-graph family: the text
// that beam_loss_fwd (asg_beam_loss.hip: all frames of an utterance in one launch) and the catch-up of the lattice-keeping stream
// (asg_beam_stream_conf.hip: the frames [apos, pos) of a slot, resumed from the stored rows) both compile, as asg_beam_frame.h is
// the frame body of the search for the one-shot decoder and the streams (DESIGN.md 5l, 5ad).  It is included INSIDE the frame
// loop, as asg_beam_cells.inc is included inside its kernels: as a function the same statements gave beam_loss_fwd another register
// allocation, as text they give the parent's listing line for line.  Same adds, same order, whoever includes it: the same bits.
// One 1024-thread workgroup per utterance; in scope: tid, NINF, P (is2: the label stride of xt), g, ew = g.edge_w, tr(i, j), the
// LDS arrays pq / pa with U_{t-1} and its alphas, mp = |U_{t-1}|, and the frame's Ut [mt], Arow and xt.  G lanes per target q pull
// through q's incoming CSR row and find each source in U_{t-1} by binary search in LDS; when the row is longer than |U_{t-1}| they
// walk U_{t-1} instead and binary-search each kept source in the row.  Max pass, then sum pass; the partial results of the G lanes
// meet in a fixed butterfly.  The alpha of the frame goes to Arow and comes back into LDS with device-scope loads; mp = mt.
        const int G = subgroup(mt), per = kBL / G;
        for (int k0 = 0; k0 < mt; k0 += per) {
            const int k = k0 + tid / G, lg = tid % G;
            const bool act = k < mt;
            const int q = act ? Ut[k] : 0;
            const int i = act ? g.label[q] : 0;
            const int e0 = act ? g.row[q] : 0, e1 = act ? g.row[q + 1] : 0;
            const bool by_row = e1 - e0 <= mp;
            // every surviving candidate of q that this lane owns, in ascending source order: f(value)
            auto visit = [&](auto f) {
                if (!act) return;
                if (lg == 0) {
                    const int pos = find_sorted(pq, mp, q);
                    if (pos >= 0) f(pa[pos] + tr(i, i));
                }
                if (by_row) {
                    for (int e = e0 + lg; e < e1; e += G) {
                        const int pos = find_sorted(pq, mp, g.src[e]);
                        if (pos >= 0) f((pa[pos] + tr(i, g.src_label[e])) + ew[e]);
                    }
                } else {
                    for (int p = lg; p < mp; p += G) {
                        const int pos = find_sorted(g.src + e0, e1 - e0, pq[p]);
                        if (pos >= 0) f((pa[p] + tr(i, g.src_label[e0 + pos])) + ew[e0 + pos]);
                    }
                }
            };
            R mx = NINF;
            visit([&](R c) { mx = bmax(mx, c); });
            mx = group_max(mx, G);
            R s = R(0);
            if (mx > NINF) visit([&](R c) { s += bexp(c - mx); });
            s = group_sum(s, G);
            if (act && lg == 0) {
                const R x = mx > NINF ? (mx + blog(s)) + xt[(int64_t) i * P.is2] : NINF;
                dev_store(Arow + k, x);
            }
        }
        __threadfence();
        __syncthreads();
        for (int x = tid; x < mt; x += kBL) { pq[x] = Ut[x]; pa[x] = dev_load(Arow + x); }
        mp = mt;
        __syncthreads();
