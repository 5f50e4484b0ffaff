// torch_asg_amd/csrc/asg_beam_word_alpha.inc -- the FRAME BODY of the alpha push over the kept sets of the word-LM family: the text
// that beam_word_loss_fwd (asg_beam_word_loss.hip: all frames of an utterance in one launch) and the catch-up of the
// lattice-keeping word stream (asg_beam_word_stream_conf.hip: the frames [apos, pos) of a slot, resumed from the stored rows) both
// compile, as asg_beam_alpha.inc is for the token-graph family (DESIGN.md 5ad, 5ae).  It is included INSIDE the frame loop: as
// text it gives beam_word_loss_fwd the parent's listing line for line.  Same adds, same order, whoever includes it: the same bits.
// One 1024-thread workgroup per utterance; in scope: tid, NINF, P (is2: the label stride of xt), the walk frame f with qmask,
// tr(i, j), KT / KU, the LDS arrays ut / sm / mk, mp = |U_{t-1}|, and the frame's mt, Up / Ut (rows t-1 and t of U), Ap (alpha of
// row t-1, read with device-scope loads), Arow and xt.  G lanes per pair of U_{t-1} PUSH along the outgoing row of its q (lane 0
// adds the stay, a separator edge walks the LM) into U_t in LDS: a max pass (integer atomicMax on the order-preserving key),
// then a sum pass (64-bit fixed point, 48 fractional bits).  The alpha of the frame goes to Arow; mp = mt.
        for (int x = tid; x < mt; x += kBL) { ut[x] = Ut[x]; sm[x] = 0ull; mk[x] = (KU) 0; }
        __syncthreads();
        const int G = subgroup(mp), per = kBL / G;
        for (int pass = 0; pass < 2; ++pass) {
            for (int k0 = 0; k0 < mp; k0 += per) {
                const int k = k0 + tid / G, lg = tid % G;
                if (k >= mp) continue;
                const R a = dev_load(Ap + k);
                if (!(a > NINF)) continue;
                const unsigned long long p = Up[k];
                const int qs = (int) (p & qmask), hs = (int) (p >> f.qbits);
                const int j = f.label[qs];
                auto offer = [&](unsigned long long tp, R c) {
                    if (!(c > NINF)) return;
                    const int pos = find_sorted(ut, mt, tp);
                    if (pos < 0) return;
                    if (pass == 0) atomicMax(mk + pos, KT::enc(c));
                    else {
                        const unsigned long long fx = to_fixed((double) bexp(c - KT::dec(mk[pos])), kBSumScale);
                        if (fx) atomicAdd(sm + pos, fx);
                    }
                };
                if (lg == 0) offer(p, a + tr(j, j));
                const int e1 = f.orow[qs + 1];
                for (int e = f.orow[qs] + lg; e < e1; e += G) {
                    const int2 arc = f.oarc[e];
                    int th = hs;
                    R w = f.ow[e];
                    if (arc.y == f.sep) {                             // a word ends: the LM moves
                        R add;
                        int h2;
                        if (!f.step(hs, f.wos[f.state[qs]], h2, add)) continue;
                        th = h2;
                        w = w + add;
                    }
                    offer(f.pair(th, arc.x), (a + tr(arc.y, j)) + w);
                }
            }
            __syncthreads();
        }
        for (int x = tid; x < mt; x += kBL) {
            const KU key = mk[x];
            R v = NINF;
            if (key != 0 && sm[x] != 0ull) {
                const R s = (R) ((double) sm[x] * (1.0 / kBSumScale));
                v = (KT::dec(key) + blog(s)) + xt[(int64_t) f.label[(int) (ut[x] & qmask)] * P.is2];
            }
            dev_store(Arow + x, v);
        }
        __threadfence();
        __syncthreads();
        mp = mt;
