// ctc_beam_impl.h — what the whole-utterance CTC beam search (ctc_beam.hip, cm_ctc_beam_search), the streamed one
// (ctc_beam_stream.hip, cm_ctc_beam_stream), the LM-fused one (ctc_beam_lm.hip, cm_ctc_beam_lm_search) and the streamed LM-fused one
// (ctc_beam_lm_stream.hip, cm_ctc_beam_lm_stream; its kernel is the streamed one's template, ctc_beam_stream_impl.h) share: constants, the LDS
// layout, hashing, merge_rank, the host-side argument check and slab layout and, as text all four kernels include in their
// bodies, the frame loop (ctc_beam_frames.inc.h) and the finish with its backtrack (ctc_beam_finish.inc.h).  The kernels run
// exactly these statements per frame, so a search fed chunk by chunk returns the bits of the search fed at once, and the LM search
// differs from the LM-free one only in what the fragments say under their LM switch (NoLm below).  The
// algorithm is stated in mamba_asr_amd/ctc_decode.py and DESIGN.md §4b; in short, per processed frame:
//   select tokens {v : lp[v] > token_prune_min_logp} U {first argmax}, ascending;  candidates (token outer, beam rank inner) with
//   score + lp[v];  merge equal (canonical text hash, last token): survivor = earliest candidate, score = left logaddexp fold in
//   candidate order;  drop below max + beam_prune_logp;  rank by (score desc, earliest candidate);  keep beam_size;  optionally keep
//   the first beam per (last word, partial word, last token).
// One workgroup of 256 threads per utterance runs the frame loop; scores, merges and ranking are float64.  A beam's identity is two
// polynomial hashes mod 2^61 - 1 of its canonical symbol string (code point + 1 per character, hash_sep after every completed word,
// then the partial word) plus its last token; extending by a piece of any length is O(1) from the host's per-token H(clean) and
// base^len(clean).  Merging is a bitonic sort of (hash1, hash2, last | candidate index) and a walk of each run of equal keys;
// ranking is a second bitonic sort of (order-preserving score key, candidate index).  Up to LDS_CAP candidates sort in LDS, more
// (user thresholds: up to beam_size x V) in the utterance's own global workspace slab, same code; the choice depends on the frame's
// candidate count alone.  History: per (processed frame, beam slot) the parent slot and the text-changing token; the finished
// hypotheses are backtracked on the device.
// Nothing is shared between workgroups (no atomics, no cross-workgroup traffic): results do not depend on batch composition.
#pragma once
#include <cmath>
#include <type_traits>

#include "cm_common.h"

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int KMAX = 256;          // beam_size limit
constexpr int VMAX = 4096;         // vocabulary limit (16 row chunks per thread)
constexpr int VCH = VMAX / NT;
constexpr int LDS_CAP = 1024;      // candidates sorted in LDS; more go through the workspace
constexpr int TMAX = 0x7fff0000 / KMAX;   // frames per utterance
constexpr uint64_t P61 = (1ull << 61) - 1;
constexpr uint64_t KEY_MAX = ~0ull;
constexpr int F_TEXT_EMPTY = 1, F_PART_EMPTY = 2;

// The helpers that read search parameters (joined, extend, canonical, load_lp) are templates over the argument struct P,
// cm_ctc_beam_args, cm_ctc_beam_stream_args, cm_ctc_beam_lm_args or cm_ctc_beam_lm_stream_args, and the two text fragments name it p:
// the fields they read carry the same names in all four structs (log_probs, lp_bs, lp_ts, dtype, V, the token tables, the hash constants, blank, beam_size, topk, prune_history,
// beam_prune_logp, token_prune_min_logp, blank_skip_log; the finish also num_hyps, tokens, token_len, scores; under the LM switch
// also tok_len, the LM tables and constants, lm_scores).

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

// The LM switch of the two text fragments.  Every kernel that includes them is a template over a policy type Lm (and over its
// argument struct), so that what the fragments say under `if constexpr (Lm::on)` is dependent and is never instantiated for the
// LM-free kernels.  Lm::Lds is the type of the includer's `lb` (the per-beam LM state beside sh.bm), Lm::State one beam's LM
// state in registers, Lm::CTX its context length.  NoLm holds nothing: its `lb` is an empty constant, no LDS.  The n-gram policy,
// NgramLm, is in ctc_beam_lm_impl.h with the lm_* functions the fragments call under the switch.
struct NoLm {
    static constexpr bool on = false;
    struct Lds {};
    struct State {};
    static constexpr int STREAM_BYTES = 0;      // per beam in a stream slab (ctc_beam_stream_impl.h)
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

// the single initial beam ("", "", none, 0) into slot 0 of buffer buf (one thread calls it)
__device__ __forceinline__ void store_initial_beam(Beams &bm, int buf) {
    State s0;
    s0.ht[0] = s0.ht[1] = s0.hp[0] = s0.hp[1] = s0.hw[0] = s0.hw[1] = 0;
    s0.pp[0] = s0.pp[1] = 1;
    s0.flags = F_TEXT_EMPTY | F_PART_EMPTY;
    store_state(bm, buf, 0, s0, 0.0, -1);
}

// hash of join(text, partial) as a word sequence (sep between words); h[0] = h[1] = 0 and *empty when both are empty
template <class P> __device__ __forceinline__ void joined(const P &p, const State &s, uint64_t h[2], bool *empty) {
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
template <class P> __device__ __forceinline__ State extend(const P &p, const State &s, int v, int cls) {
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
template <class P> __device__ __forceinline__ void canonical(const P &p, const State &s, uint64_t h[2]) {
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

// merge_rank without a total: prune and rank by the folded score itself
struct NoTotal {};

// Merge + prune + rank over n candidates whose keys (k1, k2 = hashes, k3 = group tag << 32 | candidate index) are in b, padded to
// n2 with KEY_MAX.  score(idx) gives a candidate's score; the scores of a run of equal keys fold into b.sc at the position of the
// run's head.  On return positions 0 .. kept-1 hold the survivors in rank order: k1 = score_key(score), k2 = candidate index.
// With a total functor (the LM search) each head gets total(idx, folded score) and prune, rank and limit act on the totals:
// k1 = score_key(total), and k3 = the position in b.sc where the folded score stays.
template <bool G, class ScoreFn, class TotalFn = NoTotal>
__device__ int merge_rank(Shared &sh, const Buf b, int n, int n2, int limit, double prune, ScoreFn score, TotalFn total = {}) {
    constexpr bool totals = !std::is_same_v<TotalFn, NoTotal>;
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
        if constexpr (totals) {
            b.k1[i] = alive ? score_key(total((int)idx, s)) : KEY_MAX;
            b.k2[i] = alive ? idx : KEY_MAX;
            b.k3[i] = (uint64_t)i;
        } else {
            b.k1[i] = alive ? score_key(s) : KEY_MAX;
            b.k2[i] = alive ? idx : KEY_MAX;
            b.k3[i] = 0;
        }
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

template <class P> __device__ __forceinline__ float load_lp(const P &p, int b, int t, int v) {
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

// the sort arrays in global memory: entries when beam_size x V candidates can outgrow LDS_CAP, else 0
inline int sort_entries(int beam_size, int V) {
    int64_t m = (int64_t)beam_size * V, q = 1;
    while (q < m) q <<= 1;
    return q > LDS_CAP ? (int)q : 0;
}

__device__ __forceinline__ Buf global_buf(char *base, int n2max) {
    uint64_t *k = reinterpret_cast<uint64_t *>(base);
    return Buf{k, k + n2max, k + 2 * (int64_t)n2max, reinterpret_cast<double *>(base) + 3 * (int64_t)n2max};
}

// per-utterance workspace slab of the whole-utterance searches: history (T x K int32, rounded to 16 B), then the sort arrays when
// the candidates can outgrow LDS
template <class A> void slab_layout(const A &a, int64_t *slab, int64_t *hist, int *n2max) {
    *hist = ((int64_t)a.T * a.beam_size * 4 + 15) / 16 * 16;
    *n2max = sort_entries(a.beam_size, a.V);
    *slab = *hist + 4 * 8 * (int64_t)*n2max;
}

// the body of cm_ctc_beam_workspace_bytes and cm_ctc_beam_lm_workspace_bytes: 0 for sizes outside the limits
template <class A> int64_t whole_workspace_bytes(const A *args) {
    if (!args || args->batch <= 0 || args->T <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX)
        return 0;
    int64_t slab, hist;
    int n2max;
    slab_layout(*args, &slab, &hist, &n2max);
    return slab * args->batch;
}

// The argument checks the three entry points share, in the order each of them always made them; `who` prefixes the messages.
// max_frames is NULL for a whole-utterance entry (T in [1, TMAX]), else the streamed entry's, whose chunk of T rows may be empty
// (then no log_probs and no strides) and must fit *max_frames.  pointers: the entry's own "none of my pointers is NULL".
template <class A> int check_beam_args(const A &a, const char *who, const int32_t *max_frames, bool pointers) {
    const bool whole = max_frames == nullptr;
    CM_REQUIRE(a.batch > 0 && a.T >= (whole ? 1 : 0) && a.V > 1, CM_EINVAL, "%s: bad sizes batch=%d T=%d V=%d", who, a.batch, a.T, a.V);
    CM_REQUIRE(a.V <= VMAX, CM_EUNSUPPORTED, "%s: at most %d tokens (got %d)", who, VMAX, a.V);
    CM_REQUIRE(!whole || a.T <= TMAX, CM_EUNSUPPORTED, "%s: T=%d too long", who, a.T);
    CM_REQUIRE(a.beam_size >= 1 && a.beam_size <= KMAX, CM_EINVAL, "%s: beam_size %d not in [1, %d]", who, a.beam_size, KMAX);
    CM_REQUIRE(whole || (*max_frames >= 1 && *max_frames <= TMAX), CM_EINVAL, "%s: max_frames %d not in [1, %d]", who, *max_frames, TMAX);
    CM_REQUIRE(whole || a.T <= *max_frames, CM_EINVAL, "%s: a chunk of T=%d rows exceeds max_frames=%d", who, a.T, *max_frames);
    CM_REQUIRE(a.topk >= 1, CM_EINVAL, "%s: topk %d < 1", who, a.topk);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "%s: blank %d out of range", who, a.blank);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "%s: log_probs must be fp32 or bf16", who);
    CM_REQUIRE(a.T == 0 || (a.lp_bs >= 0 && a.lp_ts >= a.V), CM_EINVAL, "%s: bad log_probs strides bs=%lld ts=%lld", who,
               (long long)a.lp_bs, (long long)a.lp_ts);
    CM_REQUIRE(pointers, CM_EINVAL, "%s: NULL pointer", who);
    CM_REQUIRE(a.hash_base[0] > 1 && a.hash_base[0] < P61 && a.hash_base[1] > 1 && a.hash_base[1] < P61 && a.hash_sep < P61,
               CM_EINVAL, "%s: hash bases / separator must lie in (1, 2^61 - 1)", who);
    CM_REQUIRE(!std::isnan(a.beam_prune_logp) && !std::isnan(a.token_prune_min_logp) && a.blank_skip_threshold > 0.0,
               CM_EINVAL, "%s: thresholds must not be NaN and blank_skip_threshold must be > 0", who);
    return CM_OK;
}

}  // namespace
