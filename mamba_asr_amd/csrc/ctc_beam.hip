// ctc_beam.hip — LM-free CTC beam search (contract: cm_ctc_beam_search; replaces speechbrain.decoders.ctc.CTCBeamSearcher, call
// sites reference train_CTC.py:309-310 and 411-414, settings hparams/CTC/conmamba_large.yaml:168-172, 232-237).  The algorithm is
// stated in mamba_asr_amd/ctc_decode.py and DESIGN.md §4b; in short, per processed frame:
//   select tokens {v : lp[v] > token_prune_min_logp} U {first argmax}, ascending;  candidates (token outer, beam rank inner) with
//   score + lp[v];  merge equal (canonical text hash, last token): survivor = earliest candidate, score = left logaddexp fold in
//   candidate order;  drop below max + beam_prune_logp;  rank by (score desc, earliest candidate);  keep beam_size;  optionally keep
//   the first beam per (last word, partial word, last token).
// One workgroup of 256 threads per utterance runs the frame loop; scores, merges and ranking are float64.  A beam's identity is two
// polynomial hashes mod 2^61 - 1 of its canonical symbol string (code point + 1 per character, hash_sep after every completed word,
// then the partial word) plus its last token; extending by a piece of any length is O(1) from the host's per-token H(clean) and
// base^len(clean).  Merging is a bitonic sort of (hash1, hash2, last | candidate index) and a walk of each run of equal keys;
// ranking is a second bitonic sort of (order-preserving score key, candidate index).  Up to LDS_CAP candidates sort in LDS, more
// (user thresholds: up to beam_size x V) in the utterance's own global workspace slab, same code.  History: per (processed frame,
// beam slot) the parent slot and the text-changing token; the finished hypotheses are backtracked on the device.
// Nothing is shared between workgroups (no atomics, no cross-workgroup traffic): results do not depend on batch composition.
#include <cmath>
#include <type_traits>

#include "cm_common.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int KMAX = 256;          // beam_size limit
constexpr int VMAX = 4096;         // vocabulary limit (16 row chunks per thread)
constexpr int VCH = VMAX / NT;
constexpr int LDS_CAP = 1024;      // candidates sorted in LDS; more go through the workspace
constexpr uint64_t P61 = (1ull << 61) - 1;
constexpr uint64_t KEY_MAX = ~0ull;
constexpr int F_TEXT_EMPTY = 1, F_PART_EMPTY = 2;

__device__ __forceinline__ uint64_t mod_add(uint64_t a, uint64_t b) {
    uint64_t r = a + b;
    return r >= P61 ? r - P61 : r;
}

__device__ __forceinline__ uint64_t mod_mul(uint64_t a, uint64_t b) {
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    uint64_t r = (lo & P61) + ((lo >> 61) | (hi << 3));
    return r >= P61 ? r - P61 : r;
}

// contract: logaddexp(a, b) = max + log1p(exp(-|a - b|)), -inf when both are -inf
__device__ __forceinline__ double lae(double a, double b) {
    if (a == -__builtin_inf() && b == -__builtin_inf()) return a;
    return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

// order-preserving map of a double to uint64 (larger score -> smaller key: ascending sort = score descending); -0 counts as +0
__device__ __forceinline__ uint64_t score_key(double s) {
    const uint64_t u = (uint64_t)__double_as_longlong(s + 0.0);
    const uint64_t ord = (u >> 63) ? ~u : (u | (1ull << 63));
    return ~ord;
}
__device__ __forceinline__ double key_score(uint64_t k) {
    const uint64_t ord = ~k;
    return __longlong_as_double((long long)((ord >> 63) ? (ord & ~(1ull << 63)) : ~ord));
}

// one beam's identity state (struct-of-arrays in LDS, double-buffered)
struct Beams {
    double score[2][KMAX];
    uint64_t ht[2][2][KMAX];       // text: completed words joined by sep (no trailing sep)
    uint64_t hp[2][2][KMAX];       // partial word
    uint64_t pp[2][2][KMAX];       // base^len(partial)
    uint64_t hw[2][2][KMAX];       // last completed word (prune_history)
    int32_t last[2][KMAX];         // -1: none
    int32_t flags[2][KMAX];
};

struct State {
    uint64_t ht[2], hp[2], pp[2], hw[2];
    int32_t flags;
};

struct Shared {
    Beams bm;
    uint64_t k1[LDS_CAP], k2[LDS_CAP], k3[LDS_CAP];
    double sc[LDS_CAP];
    float row[2][VMAX];
    uint16_t sel[VMAX];
    uint64_t red[NT / 16];
    int32_t nan_wave[NT / 64], cnt_wave[NT / 64];
    int32_t keep[KMAX];
    int32_t nsel, nkeep;
};

struct Buf {
    uint64_t *k1, *k2, *k3;
    double *sc;
};

__device__ __forceinline__ State load_state(const Beams &bm, int buf, int r) {
    State s;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        s.ht[h] = bm.ht[buf][h][r]; s.hp[h] = bm.hp[buf][h][r]; s.pp[h] = bm.pp[buf][h][r]; s.hw[h] = bm.hw[buf][h][r];
    }
    s.flags = bm.flags[buf][r];
    return s;
}

__device__ __forceinline__ void store_state(Beams &bm, int buf, int r, const State &s, double score, int last) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        bm.ht[buf][h][r] = s.ht[h]; bm.hp[buf][h][r] = s.hp[h]; bm.pp[buf][h][r] = s.pp[h]; bm.hw[buf][h][r] = s.hw[h];
    }
    bm.flags[buf][r] = s.flags;
    bm.score[buf][r] = score;
    bm.last[buf][r] = last;
}

// hash of join(text, partial) as a word sequence (sep between words); h[0] = h[1] = 0 and *empty when both are empty
__device__ __forceinline__ void joined(const cm_ctc_beam_args &p, const State &s, uint64_t h[2], bool *empty) {
    const bool te = s.flags & F_TEXT_EMPTY, pe = s.flags & F_PART_EMPTY;
    *empty = te && pe;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (pe) h[k] = te ? 0 : s.ht[k];
        else if (te) h[k] = s.hp[k];
        else h[k] = mod_add(mod_mul(mod_add(mod_mul(s.ht[k], p.hash_base[k]), p.hash_sep), s.pp[k]), s.hp[k]);
    }
}

// the state after token v (class cls) when v changes the text: char appends to partial, word-start commits partial and restarts it
__device__ __forceinline__ State extend(const cm_ctc_beam_args &p, const State &s, int v, int cls) {
    State n = s;
    const uint64_t *th = p.tok_hash + 2 * (int64_t)v, *tp = p.tok_pow + 2 * (int64_t)v;
    if (cls == 1) {
        if (!(s.flags & F_PART_EMPTY)) {
            bool e;
            joined(p, s, n.ht, &e);
            n.hw[0] = s.hp[0]; n.hw[1] = s.hp[1];
            n.flags &= ~F_TEXT_EMPTY;
        }
        n.hp[0] = th[0]; n.hp[1] = th[1]; n.pp[0] = tp[0]; n.pp[1] = tp[1];
        n.flags = (n.flags & ~F_PART_EMPTY) | ((tp[0] == 1 && tp[1] == 1) ? F_PART_EMPTY : 0);
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) { n.hp[k] = mod_add(mod_mul(s.hp[k], tp[k]), th[k]); n.pp[k] = mod_mul(s.pp[k], tp[k]); }
        if (!(tp[0] == 1 && tp[1] == 1)) n.flags &= ~F_PART_EMPTY;
    }
    return n;
}

// hash of the canonical string (each completed word followed by sep, then the partial word)
__device__ __forceinline__ void canonical(const cm_ctc_beam_args &p, const State &s, uint64_t h[2]) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
        h[k] = (s.flags & F_TEXT_EMPTY) ? s.hp[k]
                                         : mod_add(mod_mul(mod_add(mod_mul(s.ht[k], p.hash_base[k]), p.hash_sep), s.pp[k]), s.hp[k]);
}

template <bool G> __device__ __forceinline__ void barrier() {
    if constexpr (G) __syncthreads();
    else cm_lds_barrier();
}

__device__ __forceinline__ bool key_less(uint64_t a1, uint64_t a2, uint64_t a3, uint64_t b1, uint64_t b2, uint64_t b3) {
    return a1 != b1 ? a1 < b1 : (a2 != b2 ? a2 < b2 : a3 < b3);
}

// ascending bitonic sort of (k1, k2, k3) over n2 (a power of two) entries
template <bool G> __device__ void bitonic(const Buf b, int n2) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < (n2 >> 1); q += NT) {
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const uint64_t a1 = b.k1[i], a2 = b.k2[i], a3 = b.k3[i], c1 = b.k1[l], c2 = b.k2[l], c3 = b.k3[l];
                const bool up = (i & k) == 0;
                if (up ? key_less(c1, c2, c3, a1, a2, a3) : key_less(a1, a2, a3, c1, c2, c3)) {
                    b.k1[i] = c1; b.k2[i] = c2; b.k3[i] = c3;
                    b.k1[l] = a1; b.k2[l] = a2; b.k3[l] = a3;
                }
            }
            barrier<G>();
        }
}

// Merge + prune + rank over n candidates whose keys (k1, k2 = hashes, k3 = group tag << 32 | candidate index) are in b, padded to
// n2 with KEY_MAX.  score(idx) gives a candidate's score.  On return positions 0 .. *kept-1 hold the survivors in rank order:
// k1 = score_key(score), k2 = candidate index.
template <bool G, class ScoreFn>
__device__ int merge_rank(Shared &sh, const Buf b, int n, int n2, int limit, double prune, ScoreFn score) {
    const int tid = threadIdx.x;
    bitonic<G>(b, n2);
    // fold each run of equal (k1, k2, tag) in candidate order into its first entry
    for (int i = tid; i < n2; i += NT) {
        double s = 0.0;
        bool head = false;
        if (i < n) {
            const uint64_t a1 = b.k1[i], a2 = b.k2[i], a3 = b.k3[i];
            head = i == 0 || b.k1[i - 1] != a1 || b.k2[i - 1] != a2 || (b.k3[i - 1] >> 32) != (a3 >> 32);
            if (head) {
                s = score((int)(uint32_t)a3);
                for (int j = i + 1; j < n && b.k1[j] == a1 && b.k2[j] == a2 && (b.k3[j] >> 32) == (a3 >> 32); ++j)
                    s = lae(s, score((int)(uint32_t)b.k3[j]));
            }
        }
        b.sc[i] = head ? s : __builtin_nan("");
    }
    barrier<G>();
    for (int i = tid; i < n2; i += NT) {
        const double s = b.sc[i];
        const bool alive = s == s;
        const uint64_t idx = (uint32_t)b.k3[i];
        b.k1[i] = alive ? score_key(s) : KEY_MAX;
        b.k2[i] = alive ? idx : KEY_MAX;
        b.k3[i] = 0;
    }
    barrier<G>();
    bitonic<G>(b, n2);
    // survivors are a prefix (dead entries sort last); keep those >= max + prune, at most limit
    const double thr = key_score(b.k1[0]) + prune;
    if (tid == 0) sh.nkeep = 0;
    barrier<G>();
    for (int i = tid; i < n2; i += NT) {
        auto ok = [&](int x) { return x < n2 && b.k1[x] != KEY_MAX && key_score(b.k1[x]) >= thr; };
        if (ok(i) && !ok(i + 1)) sh.nkeep = i + 1;        // the single boundary of a monotone predicate: one writer
    }
    barrier<G>();
    return min(sh.nkeep, limit);
}

__device__ __forceinline__ int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ float load_lp(const cm_ctc_beam_args &p, int b, int t, int v) {
    const int64_t off = (int64_t)b * p.lp_bs + (int64_t)t * p.lp_ts + v;
    if (p.dtype == CM_BF16) return cm_elem<cm_bf16>::from_bits(static_cast<const uint16_t *>(p.log_probs)[off]);
    return static_cast<const float *>(p.log_probs)[off];
}

// (orderable float bits << 32) | (~v): the maximum is the largest value at the lowest index
__device__ __forceinline__ uint64_t argmax_key(float x, int v) {
    const uint32_t u = __float_as_uint(x);
    const uint32_t ord = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((uint64_t)ord << 32) | (uint32_t)(~v);
}

__device__ __forceinline__ uint64_t dpp_max_u64_row(uint64_t k) {
    auto step = [](uint64_t a, uint64_t o) { return o > a ? o : a; };
    auto sh = [](uint64_t a, auto ctrl) {
        const float lo = cm_dpp<decltype(ctrl)::value>(__uint_as_float((uint32_t)a));
        const float hi = cm_dpp<decltype(ctrl)::value>(__uint_as_float((uint32_t)(a >> 32)));
        return ((uint64_t)__float_as_uint(hi) << 32) | __float_as_uint(lo);
    };
    k = step(k, sh(k, std::integral_constant<int, CM_DPP_QUAD(1, 0, 3, 2)>{}));
    k = step(k, sh(k, std::integral_constant<int, CM_DPP_QUAD(2, 3, 0, 1)>{}));
    k = step(k, sh(k, std::integral_constant<int, CM_DPP_ROW_HALF_MIRROR>{}));
    k = step(k, sh(k, std::integral_constant<int, CM_DPP_ROW_MIRROR>{}));
    return k;
}

__global__ __launch_bounds__(NT) void ctc_beam_kernel(const cm_ctc_beam_args p, int64_t slab_bytes, int64_t hist_bytes, int n2max) {
    __shared__ Shared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, V = p.V, K = p.beam_size;
    const int n = min(max(p.lengths[b], 0), T);
    char *slab = static_cast<char *>(p.workspace) + (int64_t)b * slab_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(slab);
    const Buf gbuf{reinterpret_cast<uint64_t *>(slab + hist_bytes), reinterpret_cast<uint64_t *>(slab + hist_bytes) + n2max,
                   reinterpret_cast<uint64_t *>(slab + hist_bytes) + 2 * (int64_t)n2max,
                   reinterpret_cast<double *>(slab + hist_bytes) + 3 * (int64_t)n2max};
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    // the single initial beam ("", "", none, 0)
    if (tid == 0) {
        State s0;
        s0.ht[0] = s0.ht[1] = s0.hp[0] = s0.hp[1] = s0.hw[0] = s0.hw[1] = 0;
        s0.pp[0] = s0.pp[1] = 1;
        s0.flags = F_TEXT_EMPTY | F_PART_EMPTY;
        store_state(sh.bm, 0, 0, s0, 0.0, -1);
    }
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
            int kept;
            if (n2 <= LDS_CAP) {
                gen(lbuf);
                cm_lds_barrier();
                kept = merge_rank<false>(sh, lbuf, ncand, n2, K, p.beam_prune_logp, cand_score);
            } else {
                gen(gbuf);
                __syncthreads();
                kept = merge_rank<true>(sh, gbuf, ncand, n2, K, p.beam_prune_logp, cand_score);
            }
            const Buf rb = n2 <= LDS_CAP ? lbuf : gbuf;
            // the new beams, in rank order
            State ns;
            double nscore = 0.0;
            int nlast = -1, entry = 0;
            if (tid < kept) {
                const int idx = (int)rb.k2[tid], j = idx / nb, r = idx - j * nb, v = sh.sel[j];
                const State s = load_state(sh.bm, cur, r);
                const bool same = v == p.blank || v == sh.bm.last[cur][r];
                ns = same ? s : extend(p, s, v, p.tok_class[v]);
                nscore = key_score(rb.k1[tid]);
                nlast = v;
                entry = (r << 16) | (same ? 0 : v + 1);
                store_state(sh.bm, nxt, tid, ns, nscore, nlast);
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
                if (keep) store_state(sh.bm, nxt, slot, ns, nscore, nlast);
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
    const int nh = merge_rank<false>(sh, lbuf, nb, pow2_at_least(nb), p.topk, p.beam_prune_logp,
                                     [&](int idx) { return sh.bm.score[cur][idx]; });
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
        p.scores[(int64_t)b * p.topk + h] = key_score(sh.k1[h]);
    }
}

// per-utterance workspace slab: history (T x K int32, rounded to 16 B), then the sort arrays when the candidates can outgrow LDS
void slab_layout(const cm_ctc_beam_args &a, int64_t *slab, int64_t *hist, int *n2max) {
    *hist = ((int64_t)a.T * a.beam_size * 4 + 15) / 16 * 16;
    int64_t m = (int64_t)a.beam_size * a.V, q = 1;
    while (q < m) q <<= 1;
    *n2max = q > LDS_CAP ? (int)q : 0;
    *slab = *hist + 4 * 8 * (int64_t)*n2max;
}

}  // namespace

extern "C" int64_t cm_ctc_beam_workspace_bytes(const cm_ctc_beam_args *args) {
    if (!args || args->batch <= 0 || args->T <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX)
        return 0;
    int64_t slab, hist;
    int n2max;
    slab_layout(*args, &slab, &hist, &n2max);
    return slab * args->batch;
}

extern "C" int cm_ctc_beam_search(const cm_ctc_beam_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_search: args is NULL");
    cm_ctc_beam_args a = *args;
    CM_REQUIRE(a.batch > 0 && a.T > 0 && a.V > 1, CM_EINVAL, "ctc_beam_search: bad sizes batch=%d T=%d V=%d", a.batch, a.T, a.V);
    CM_REQUIRE(a.V <= VMAX, CM_EUNSUPPORTED, "ctc_beam_search: at most %d tokens (got %d)", VMAX, a.V);
    CM_REQUIRE(a.T <= 0x7fff0000 / KMAX, CM_EUNSUPPORTED, "ctc_beam_search: T=%d too long", a.T);
    CM_REQUIRE(a.beam_size >= 1 && a.beam_size <= KMAX, CM_EINVAL, "ctc_beam_search: beam_size %d not in [1, %d]", a.beam_size, KMAX);
    CM_REQUIRE(a.topk >= 1, CM_EINVAL, "ctc_beam_search: topk %d < 1", a.topk);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "ctc_beam_search: blank %d out of range", a.blank);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "ctc_beam_search: log_probs must be fp32 or bf16");
    CM_REQUIRE(a.lp_bs >= 0 && a.lp_ts >= a.V, CM_EINVAL, "ctc_beam_search: bad log_probs strides bs=%lld ts=%lld",
               (long long)a.lp_bs, (long long)a.lp_ts);
    CM_REQUIRE(a.log_probs && a.lengths && a.tok_class && a.tok_hash && a.tok_pow && a.tokens && a.token_len && a.scores &&
                   a.num_hyps && a.bad_frame && a.workspace, CM_EINVAL, "ctc_beam_search: NULL pointer");
    CM_REQUIRE(a.hash_base[0] > 1 && a.hash_base[0] < P61 && a.hash_base[1] > 1 && a.hash_base[1] < P61 && a.hash_sep < P61,
               CM_EINVAL, "ctc_beam_search: hash bases / separator must lie in (1, 2^61 - 1)");
    CM_REQUIRE(!std::isnan(a.beam_prune_logp) && !std::isnan(a.token_prune_min_logp) && a.blank_skip_threshold > 0.0,
               CM_EINVAL, "ctc_beam_search: thresholds must not be NaN and blank_skip_threshold must be > 0");
    CM_REQUIRE(a.workspace_bytes >= cm_ctc_beam_workspace_bytes(&a), CM_EINVAL,
               "ctc_beam_search: workspace smaller than cm_ctc_beam_workspace_bytes()");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    int64_t slab, hist;
    int n2max;
    slab_layout(a, &slab, &hist, &n2max);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(a.batch), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a, slab, hist, n2max);
    return cm_launch_status("cm_ctc_beam_search");
}
