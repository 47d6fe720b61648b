// ctc_beam_finish.inc.h — the finish and backtrack of the CTC beam search as TEXT (see ctc_beam_frames.inc.h; the same four
// kernels include it): on the sort buffers only, beams and history stay as they are.  In scope at the include, behind a __syncthreads that covers beams and history: p, sh,
// b, tid, K, nb, cur, steps, hist, lbuf, tok_stride (row stride of p.tokens), status_out / status (the word thread 0 writes beside
// num_hyps) and the constant guard_history (the history is caller memory written by earlier launches: clamp each parent slot below
// K, so that a damaged slab cannot lead the backtrack out of it).
// The LM switch, as in the frame loop: Lm and lb (the LM states of the beams in sh.bm[cur]).  Under `if constexpr (Lm::on)` the
// text calls lm_load, lm_commit and lm_cond, reads p.lm_eos and p.alpha_ln10, ranks by final_total and also writes p.lm_scores.
    // finish: text = join(text, partial); merge by text; prune; rank; first topk
    for (int i = tid; i < LDS_CAP; i += NT) {
        if (i < nb) {
            const State s = load_state(sh.bm, cur, i);
            uint64_t h[2];
            bool empty;
            joined(p, s, h, &empty);
            sh.k1[i] = h[0]; sh.k2[i] = h[1]; sh.k3[i] = ((uint64_t)empty << 32) | (uint32_t)i;
        } else if (i < KMAX) {
            sh.k1[i] = sh.k2[i] = sh.k3[i] = KEY_MAX;
        }
    }
    __syncthreads();
    // under an LM: the partial becomes a word; total = acoustic + LM(text) (+ the </s> term), which prunes and ranks
    const auto final_total = [&] {
        if constexpr (Lm::on) {
            return [&](int idx, double acoustic) {
                const State s = load_state(sh.bm, cur, idx);
                typename Lm::State l = lm_load(lb, cur, idx);
                if (!(s.flags & F_PART_EMPTY)) lm_commit(p, l, s.hp[0], s.hp[1]);
                double total = acoustic + l.lm;
                if (p.lm_eos >= 0) {
                    int32_t next[Lm::CTX];
                    total += p.alpha_ln10 * lm_cond(p, l.ctx, p.lm_eos, next);
                }
                return total;
            };
        } else {
            return NoTotal{};
        }
    }();
    const int nh = merge_rank<false>(sh, lbuf, nb, pow2_at_least(nb), p.topk, p.beam_prune_logp,
                                     [&](int idx) { return sh.bm.score[cur][idx]; }, final_total);
    if (tid == 0) { p.num_hyps[b] = nh; status_out[b] = status; }
    for (int h = tid; h < nh; h += NT) {
        int slot = (int)sh.k2[h], len = 0;
        int32_t *out = p.tokens + ((int64_t)b * p.topk + h) * tok_stride;
        for (int s = steps - 1; s >= 0; --s) {
            const int e = hist[(int64_t)s * K + slot];
            if (e & 0xffff) out[len++] = (e & 0xffff) - 1;
            slot = e >> 16;
            if constexpr (guard_history) slot = min(max(slot, 0), K - 1);
        }
        for (int i = 0; i < len / 2; ++i) { const int x = out[i]; out[i] = out[len - 1 - i]; out[len - 1 - i] = x; }
        p.token_len[(int64_t)b * p.topk + h] = len;
        if constexpr (Lm::on) {
            // k1 ranks by the total; the folded acoustic score stayed at the head's position
            p.scores[(int64_t)b * p.topk + h] = sh.sc[min(max((int)sh.k3[h], 0), KMAX - 1)] + 0.0;
            p.lm_scores[(int64_t)b * p.topk + h] = key_score(sh.k1[h]);
        } else {
            p.scores[(int64_t)b * p.topk + h] = key_score(sh.k1[h]);
        }
    }
