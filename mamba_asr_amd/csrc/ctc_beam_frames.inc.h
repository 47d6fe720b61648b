// ctc_beam_frames.inc.h — the frame loop of the CTC beam search as TEXT: the four kernels (ctc_beam.hip, ctc_beam_lm.hip and, through
// ctc_beam_stream_impl.h, ctc_beam_stream.hip and ctc_beam_lm_stream.hip) include this file in the middle of their bodies, so they run the same statements and the whole-utterance kernel
// compiles to the ISA it had when the loop stood in it (every function boundary tried around this register-starved loop moved its
// time by 1 - 2 %).
// In scope at the include: p (the argument struct), sh (Shared), b, tid, lane, wave, V, K, n (frames of log_probs[b] to consume;
// row t + 1 is fetched only while t + 1 < n, nothing past row n - 1 is read), hist (one row of K entries per processed frame is
// written at hist[steps * K]), lbuf / gbuf (sort arrays in LDS / global memory), nb0 and steps0 (live beams in sh.bm[0] -- the
// first barrier below publishes them -- and processed frames so far).  Declared here and left to the includer: nb, cur, steps (the
// search after the n frames) and bad (-1, or the first of the n frames holding a NaN: the search then stands as before it).
// Ends on a __syncthreads.
// The LM switch: Lm, the includer's policy type (ctc_beam_impl.h), and lb (Lm::Lds).  With NoLm lb is an empty constant and nothing
// below reads it.  Under `if constexpr (Lm::on)` lb holds the LM states of the beams in sh.bm, double-buffered by the same cur /
// nxt (those of the nb0 initial beams in lb[0]), and the text calls lm_load, lm_extend (which reads p's LM tables and p.tok_len)
// and lm_store of ctc_beam_lm_impl.h: the rank sort then runs on cand_total, and a surviving beam's score is the folded acoustic one.
    for (int c = 0; c < VCH; ++c)
        if (c * NT + tid < V && n > 0) sh.row[0][c * NT + tid] = load_lp(p, b, 0, c * NT + tid);
    int nb = nb0, cur = 0, steps = steps0, bad = -1;
    float pf[VCH];

    for (int t = 0; t < n; ++t) {
        const float *row = sh.row[t & 1];
        // prefetch frame t + 1 while t is processed; stored into the other row at the end of the frame
        const bool more = t + 1 < n;
#pragma unroll
        for (int c = 0; c < VCH; ++c) pf[c] = (more && c * NT + tid < V) ? load_lp(p, b, t + 1, c * NT + tid) : 0.f;
        cm_lds_barrier();
        // NaN check and first argmax
        uint64_t best = 0;
        bool nan = false;
        for (int v = tid; v < V; v += NT) {
            const float x = row[v];
            nan |= x != x;
            const uint64_t k = argmax_key(x, v);
            best = k > best ? k : best;
        }
        best = dpp_max_u64_row(best);
        const uint64_t nanmask = __ballot(nan);
        if ((lane & 15) == 0) sh.red[tid >> 4] = best;
        if (lane == 0) sh.nan_wave[wave] = nanmask != 0;
        cm_lds_barrier();
        bool any_nan = false;
        for (int w = 0; w < NT / 64; ++w) any_nan |= sh.nan_wave[w] != 0;
        if (any_nan) { bad = t; break; }
        for (int r = 0; r < NT / 16; ++r) best = sh.red[r] > best ? sh.red[r] : best;
        const int amax = (int)(~(uint32_t)best);
        const bool skip = (double)row[p.blank] > p.blank_skip_log;
        if (!skip) {
            // selected tokens in ascending order: a ballot prefix per chunk of NT tokens
            int nsel = 0;
            for (int c0 = 0; c0 < V; c0 += NT) {
                const int v = c0 + tid;
                const bool s = v < V && ((double)row[v] > p.token_prune_min_logp || v == amax);
                const uint64_t m = __ballot(s);
                if (lane == 0) sh.cnt_wave[wave] = __popcll(m);
                cm_lds_barrier();
                int off = nsel;
                for (int w = 0; w < wave; ++w) off += sh.cnt_wave[w];
                off += __popcll(m & ((1ull << lane) - 1));
                if (s) sh.sel[off] = (uint16_t)v;
                for (int w = 0; w < NT / 64; ++w) nsel += sh.cnt_wave[w];
                cm_lds_barrier();
            }
            const int ncand = nsel * nb, n2 = pow2_at_least(ncand);
            const int nxt = cur ^ 1;
            auto gen = [&](const Buf bf) {
                for (int i = tid; i < n2; i += NT) {
                    if (i < ncand) {
                        const int j = i / nb, r = i - j * nb, v = sh.sel[j];
                        const State s = load_state(sh.bm, cur, r);
                        uint64_t h[2];
                        if (v == p.blank || v == sh.bm.last[cur][r]) canonical(p, s, h);
                        else canonical(p, extend(p, s, v, p.tok_class[v]), h);
                        bf.k1[i] = h[0]; bf.k2[i] = h[1]; bf.k3[i] = ((uint64_t)(uint32_t)v << 32) | (uint32_t)i;
                    } else {
                        bf.k1[i] = bf.k2[i] = bf.k3[i] = KEY_MAX;
                    }
                }
            };
            auto cand_score = [&](int idx) {
                const int j = idx / nb, r = idx - j * nb;
                return sh.bm.score[cur][r] + (double)row[sh.sel[j]];
            };
            // under an LM the rank sort runs on acoustic + LM(text) + partial_score(partial) of the candidate's state, as below
            const auto cand_total = [&] {
                if constexpr (Lm::on) {
                    return [&](int idx, double acoustic) {
                        const int j = idx / nb, r = idx - j * nb, v = sh.sel[j];
                        typename Lm::State nl = lm_load(lb, cur, r);
                        if (!(v == p.blank || v == sh.bm.last[cur][r])) {
                            const State s = load_state(sh.bm, cur, r);
                            const int cls = p.tok_class[v];
                            nl = lm_extend(p, nl, s, extend(p, s, v, cls), v, cls);
                        }
                        return acoustic + nl.lm + nl.ps;
                    };
                } else {
                    return NoTotal{};
                }
            }();
            int kept;
            if (n2 <= LDS_CAP) {
                gen(lbuf);
                cm_lds_barrier();
                kept = merge_rank<false>(sh, lbuf, ncand, n2, K, p.beam_prune_logp, cand_score, cand_total);
            } else {
                gen(gbuf);
                __syncthreads();
                kept = merge_rank<true>(sh, gbuf, ncand, n2, K, p.beam_prune_logp, cand_score, cand_total);
            }
            const Buf rb = n2 <= LDS_CAP ? lbuf : gbuf;
            // the new beams, in rank order; under an LM k1 ranks by the total and the folded acoustic score waits at the head's position
            State ns;
            typename Lm::State nl;
            double nscore = 0.0;
            int nlast = -1, entry = 0;
            if (tid < kept) {
                const int idx = (int)rb.k2[tid], j = idx / nb, r = idx - j * nb, v = sh.sel[j];
                const State s = load_state(sh.bm, cur, r);
                const bool same = v == p.blank || v == sh.bm.last[cur][r];
                ns = same ? s : extend(p, s, v, p.tok_class[v]);
                if constexpr (Lm::on) {
                    nl = lm_load(lb, cur, r);
                    if (!same) nl = lm_extend(p, nl, s, ns, v, p.tok_class[v]);
                    nscore = rb.sc[min(max((int)rb.k3[tid], 0), n2 - 1)] + 0.0;
                } else {
                    nscore = key_score(rb.k1[tid]);
                }
                nlast = v;
                entry = (r << 16) | (same ? 0 : v + 1);
                store_state(sh.bm, nxt, tid, ns, nscore, nlast);
                if constexpr (Lm::on) lm_store(lb, nxt, tid, nl);
            }
            __syncthreads();
            int slot = tid;
            if (p.prune_history) {
                // keep the first beam per (last word of text, partial, last token)
                bool keep = tid < kept;
                if (keep) {
                    const bool te = ns.flags & F_TEXT_EMPTY;
                    for (int q = 0; q < tid && keep; ++q) {
                        const int fq = sh.bm.flags[nxt][q];
                        keep = !(sh.bm.last[nxt][q] == nlast && (fq == ns.flags) && sh.bm.hp[nxt][0][q] == ns.hp[0] &&
                                 sh.bm.hp[nxt][1][q] == ns.hp[1] && (te || (sh.bm.hw[nxt][0][q] == ns.hw[0] && sh.bm.hw[nxt][1][q] == ns.hw[1])));
                    }
                }
                if (tid < KMAX) sh.keep[tid] = keep;
                __syncthreads();
                slot = 0;
                for (int q = 0; q < tid && q < kept; ++q) slot += sh.keep[q];
                int total = 0;
                for (int q = 0; q < kept; ++q) total += sh.keep[q];
                __syncthreads();
                if (keep) {
                    store_state(sh.bm, nxt, slot, ns, nscore, nlast);
                    if constexpr (Lm::on) lm_store(lb, nxt, slot, nl);
                }
                if (!keep) slot = -1;
                kept = total;
            }
            if (tid < K && slot >= 0 && slot < kept) hist[(int64_t)steps * K + slot] = entry;
            nb = kept;
            cur = nxt;
            ++steps;
        }
        // frame t + 1 into the other row (its last readers finished at this frame's first barrier)
#pragma unroll
        for (int c = 0; c < VCH; ++c)
            if (more && c * NT + tid < V) sh.row[(t + 1) & 1][c * NT + tid] = pf[c];
        __syncthreads();
    }
    __syncthreads();
