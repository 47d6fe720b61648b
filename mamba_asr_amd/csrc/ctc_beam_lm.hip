// ctc_beam_lm.hip — CTC beam search over whole utterances with a backoff n-gram LM fused into the frame loop (contract:
// cm_ctc_beam_lm_search; speechbrain.decoders.ctc.CTCBeamSearcher with kenlm_model_path).  The LM-free kernels
// (ctc_beam.hip, ctc_beam_stream.hip and the two text fragments they include) are tuned as text and stay as they are: this file
// shares their helpers (ctc_beam_impl.h) and carries its own frame loop and finish, the LM-free statements with three changes --
// every beam also holds an LM state (ctc_beam_lm_impl.h), the rank sort runs on acoustic + LM(text) + partial_score(partial)
// (merge_rank_lm) and the surviving beam fetches its folded acoustic score from the position the sort carried along.
// One workgroup of 256 threads per utterance; LDS: Shared 115,888 B + LmBeams 18,432 B = 134,320 B of the 160 KB a workgroup may hold.
#include "ctc_beam_lm_impl.h"

namespace {

static_assert(sizeof(Shared) + sizeof(LmBeams) <= 160 * 1024, "the LM search's LDS must fit one workgroup");

__global__ __launch_bounds__(NT) void ctc_beam_lm_kernel(const cm_ctc_beam_lm_args p, int64_t slab_bytes, int64_t hist_bytes, int n2max) {
    __shared__ Shared sh;
    __shared__ LmBeams lb;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, V = p.V, K = p.beam_size;
    const int n = min(max(p.lengths[b], 0), T);
    char *slab = static_cast<char *>(p.workspace) + (int64_t)b * slab_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(slab);
    const Buf gbuf = global_buf(slab + hist_bytes, n2max);
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    if (tid == 0) { store_initial_beam(sh.bm, 0); lm_store_initial(p, lb, 0); }
    for (int c = 0; c < VCH; ++c)
        if (c * NT + tid < V && n > 0) sh.row[0][c * NT + tid] = load_lp(p, b, 0, c * NT + tid);
    int nb = 1, cur = 0, steps = 0, bad = -1;
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
            // a candidate's beam and LM state: the parent's, or the parent's after the text-changing token (a committed word probes)
            auto cand_state = [&](int idx, State *ns, LmState *nl, int *entry, int *last) {
                const int j = idx / nb, r = idx - j * nb, v = sh.sel[j];
                const State s = load_state(sh.bm, cur, r);
                const bool same = v == p.blank || v == sh.bm.last[cur][r];
                const int cls = p.tok_class[v];
                *ns = same ? s : extend(p, s, v, cls);
                *nl = lm_load(lb, cur, r);
                if (!same) *nl = lm_extend(p, *nl, s, *ns, v, cls);
                *entry = (r << 16) | (same ? 0 : v + 1);
                *last = v;
            };
            auto cand_total = [&](int idx, double acoustic) {
                State ns;
                LmState nl;
                int entry, last;
                cand_state(idx, &ns, &nl, &entry, &last);
                return acoustic + nl.lm + nl.ps;
            };
            int kept;
            if (n2 <= LDS_CAP) {
                gen(lbuf);
                cm_lds_barrier();
                kept = merge_rank_lm<false>(sh, lbuf, ncand, n2, K, p.beam_prune_logp, cand_score, cand_total);
            } else {
                gen(gbuf);
                __syncthreads();
                kept = merge_rank_lm<true>(sh, gbuf, ncand, n2, K, p.beam_prune_logp, cand_score, cand_total);
            }
            const Buf rb = n2 <= LDS_CAP ? lbuf : gbuf;
            // the new beams, in rank order; the acoustic score waits at the head's position
            State ns;
            LmState nl;
            double nscore = 0.0;
            int nlast = -1, entry = 0;
            if (tid < kept) {
                cand_state((int)rb.k2[tid], &ns, &nl, &entry, &nlast);
                const int pos = min(max((int)rb.k3[tid], 0), n2 - 1);
                nscore = rb.sc[pos] + 0.0;
                store_state(sh.bm, nxt, tid, ns, nscore, nlast);
                lm_store(lb, nxt, tid, nl);
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
                if (keep) { store_state(sh.bm, nxt, slot, ns, nscore, nlast); lm_store(lb, nxt, slot, nl); }
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
    if (bad >= 0) {
        if (tid == 0) { p.bad_frame[b] = bad; p.num_hyps[b] = 0; }
        return;
    }

    // finish: the partial becomes a word; merge by text, folding the acoustic score; total = acoustic + LM(text) (+ the </s> term);
    // prune and rank by total; first topk
    for (int i = tid; i < KMAX; i += NT) {
        if (i < nb) {
            const State s = load_state(sh.bm, cur, i);
            uint64_t h[2];
            bool empty;
            joined(p, s, h, &empty);
            sh.k1[i] = h[0]; sh.k2[i] = h[1]; sh.k3[i] = ((uint64_t)empty << 32) | (uint32_t)i;
        } else {
            sh.k1[i] = sh.k2[i] = sh.k3[i] = KEY_MAX;
        }
    }
    __syncthreads();
    const int nh = merge_rank_lm<false>(
        sh, lbuf, nb, pow2_at_least(nb), p.topk, p.beam_prune_logp, [&](int idx) { return sh.bm.score[cur][idx]; },
        [&](int idx, double acoustic) {
            const State s = load_state(sh.bm, cur, idx);
            LmState l = lm_load(lb, cur, idx);
            if (!(s.flags & F_PART_EMPTY)) lm_commit(p, l, s.hp[0], s.hp[1]);
            double total = acoustic + l.lm;
            if (p.lm_eos >= 0) {
                int32_t next[LM_CTX];
                total += p.alpha_ln10 * lm_cond(p, l.ctx, p.lm_eos, next);
            }
            return total;
        });
    if (tid == 0) { p.num_hyps[b] = nh; p.bad_frame[b] = -1; }
    for (int h = tid; h < nh; h += NT) {
        int slot = (int)sh.k2[h], len = 0;
        int32_t *out = p.tokens + ((int64_t)b * p.topk + h) * T;
        for (int s = steps - 1; s >= 0; --s) {
            const int e = hist[(int64_t)s * K + slot];
            if (e & 0xffff) out[len++] = (e & 0xffff) - 1;
            slot = e >> 16;
        }
        for (int i = 0; i < len / 2; ++i) { const int x = out[i]; out[i] = out[len - 1 - i]; out[len - 1 - i] = x; }
        p.token_len[(int64_t)b * p.topk + h] = len;
        p.scores[(int64_t)b * p.topk + h] = sh.sc[min(max((int)sh.k3[h], 0), KMAX - 1)] + 0.0;
        p.lm_scores[(int64_t)b * p.topk + h] = key_score(sh.k1[h]);
    }
}

// per-utterance workspace slab, as the LM-free search lays it out: history (T x K int32, rounded to 16 B), then the sort arrays
// when the candidates can outgrow LDS
void slab_layout(const cm_ctc_beam_lm_args &a, int64_t *slab, int64_t *hist, int *n2max) {
    *hist = ((int64_t)a.T * a.beam_size * 4 + 15) / 16 * 16;
    *n2max = sort_entries(a.beam_size, a.V);
    *slab = *hist + 4 * 8 * (int64_t)*n2max;
}

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace

extern "C" int64_t cm_ctc_beam_lm_workspace_bytes(const cm_ctc_beam_lm_args *args) {
    if (!args || args->batch <= 0 || args->T <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX)
        return 0;
    int64_t slab, hist;
    int n2max;
    slab_layout(*args, &slab, &hist, &n2max);
    return slab * args->batch;
}

extern "C" int cm_ctc_beam_lm_search(const cm_ctc_beam_lm_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_lm_search: args is NULL");
    cm_ctc_beam_lm_args a = *args;
    CM_REQUIRE(a.batch > 0 && a.T > 0 && a.V > 1, CM_EINVAL, "ctc_beam_lm_search: bad sizes batch=%d T=%d V=%d", a.batch, a.T, a.V);
    CM_REQUIRE(a.V <= VMAX, CM_EUNSUPPORTED, "ctc_beam_lm_search: at most %d tokens (got %d)", VMAX, a.V);
    CM_REQUIRE(a.T <= TMAX, CM_EUNSUPPORTED, "ctc_beam_lm_search: T=%d too long", a.T);
    CM_REQUIRE(a.beam_size >= 1 && a.beam_size <= KMAX, CM_EINVAL, "ctc_beam_lm_search: beam_size %d not in [1, %d]", a.beam_size, KMAX);
    CM_REQUIRE(a.topk >= 1, CM_EINVAL, "ctc_beam_lm_search: topk %d < 1", a.topk);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "ctc_beam_lm_search: blank %d out of range", a.blank);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "ctc_beam_lm_search: log_probs must be fp32 or bf16");
    CM_REQUIRE(a.lp_bs >= 0 && a.lp_ts >= a.V, CM_EINVAL, "ctc_beam_lm_search: bad log_probs strides bs=%lld ts=%lld",
               (long long)a.lp_bs, (long long)a.lp_ts);
    CM_REQUIRE(a.log_probs && a.lengths && a.tok_class && a.tok_hash && a.tok_pow && a.tok_len && a.tokens && a.token_len && a.scores &&
                   a.lm_scores && a.num_hyps && a.bad_frame && a.workspace, CM_EINVAL, "ctc_beam_lm_search: NULL pointer");
    CM_REQUIRE(a.word_keys && a.word_ids && a.prefix_keys && a.ngram_keys && a.ngram_vals && a.lm_prob && a.lm_backoff, CM_EINVAL,
               "ctc_beam_lm_search: NULL LM table pointer");
    CM_REQUIRE(a.hash_base[0] > 1 && a.hash_base[0] < P61 && a.hash_base[1] > 1 && a.hash_base[1] < P61 && a.hash_sep < P61,
               CM_EINVAL, "ctc_beam_lm_search: hash bases / separator must lie in (1, 2^61 - 1)");
    CM_REQUIRE(!std::isnan(a.beam_prune_logp) && !std::isnan(a.token_prune_min_logp) && a.blank_skip_threshold > 0.0,
               CM_EINVAL, "ctc_beam_lm_search: thresholds must not be NaN and blank_skip_threshold must be > 0");
    CM_REQUIRE(a.order >= 1 && a.order <= LM_ORDER_MAX, CM_EINVAL, "ctc_beam_lm_search: LM order %d not in [1, %d]", a.order, LM_ORDER_MAX);
    CM_REQUIRE(pow2(a.word_cap) && pow2(a.prefix_cap) && pow2(a.ngram_cap), CM_EINVAL,
               "ctc_beam_lm_search: table capacities must be powers of two (word %lld, prefix %lld, n-gram %lld)",
               (long long)a.word_cap, (long long)a.prefix_cap, (long long)a.ngram_cap);
    CM_REQUIRE(a.n_words >= 1 && a.n_entries >= a.n_words && a.n_entries < (1ll << 31), CM_EINVAL,
               "ctc_beam_lm_search: need 1 <= n_words (%d) <= n_entries (%lld) < 2^31", a.n_words, (long long)a.n_entries);
    CM_REQUIRE(a.lm_bos >= -1 && a.lm_bos < a.n_words && a.lm_eos >= -1 && a.lm_eos < a.n_words && a.lm_unk >= -1 && a.lm_unk < a.n_words,
               CM_EINVAL, "ctc_beam_lm_search: lm_bos / lm_eos / lm_unk must be -1 or a word id below %d", a.n_words);
    CM_REQUIRE(std::isfinite(a.alpha) && std::isfinite(a.beta) && std::isfinite(a.unk_score_offset), CM_EINVAL,
               "ctc_beam_lm_search: alpha, beta and unk_score_offset must be finite");
    CM_REQUIRE(a.workspace_bytes >= cm_ctc_beam_lm_workspace_bytes(&a), CM_EINVAL,
               "ctc_beam_lm_search: workspace smaller than cm_ctc_beam_lm_workspace_bytes()");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    a.alpha_ln10 = a.alpha * std::log(10.0);
    int64_t slab, hist;
    int n2max;
    slab_layout(a, &slab, &hist, &n2max);
    hipLaunchKernelGGL(ctc_beam_lm_kernel, dim3(a.batch), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a, slab, hist, n2max);
    return cm_launch_status("cm_ctc_beam_lm_search");
}
