// ctc_beam_lm_impl.h — what the LM-fused CTC beam searches (ctc_beam_lm.hip, cm_ctc_beam_lm_search; ctc_beam_lm_stream.hip,
// cm_ctc_beam_lm_stream) add to ctc_beam_impl.h: the
// per-beam LM state in LDS, the table probes, ARPA backoff, the word and partial-word scores, and NgramLm, the policy that turns on
// the LM switch of the shared frame loop and finish, which call these functions; for the streamed search also the LM state's
// place in a stream slab, and the entries' shared LM argument checks.  Contract: DESIGN.md §4p, §4q.
// Probes read global memory from a few divergent lanes; each loop runs at most `capacity` steps and every id a table returns is
// range-checked before it indexes anything.
#pragma once
#include "ctc_beam_impl.h"

namespace {

constexpr int LM_ORDER_MAX = 5, LM_CTX = LM_ORDER_MAX - 1;
constexpr uint64_t LM_EMPTY = ~0ull;

// one beam's LM state (struct-of-arrays in LDS, double-buffered like Beams, whose score holds the acoustic score here): 18 KB
struct LmBeams {
    double lm[2][KMAX];                // LM(text): the sum of word_score over the completed words, in word order
    double ps[2][KMAX];                // partial_score(partial word)
    int32_t ctx[2][LM_CTX][KMAX];      // ctx[k - 1]: entry of the last k words as a k-gram, -1 when not stored
    int32_t plen[2][KMAX];             // code points of the partial word
};

struct LmState {
    double lm, ps;
    int32_t ctx[LM_CTX];
    int32_t plen;
};

__device__ __forceinline__ LmState lm_load(const LmBeams &lb, int buf, int r) {
    LmState s;
    s.lm = lb.lm[buf][r]; s.ps = lb.ps[buf][r]; s.plen = lb.plen[buf][r];
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) s.ctx[k] = lb.ctx[buf][k][r];
    return s;
}

__device__ __forceinline__ void lm_store(LmBeams &lb, int buf, int r, const LmState &s) {
    lb.lm[buf][r] = s.lm; lb.ps[buf][r] = s.ps; lb.plen[buf][r] = s.plen;
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) lb.ctx[buf][k][r] = s.ctx[k];
}

// splitmix64 finaliser; the host packs with the same function (mamba_asr_amd/ngram_lm.py)
__device__ __forceinline__ uint64_t lm_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// position of the hash pair (h0, h1) in an open-addressing table of cap slots (keys (cap, 2)), -1 when absent
__device__ __forceinline__ int64_t lm_find_pair(const uint64_t *keys, int64_t cap, uint64_t h0, uint64_t h1) {
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t s = lm_mix(h0 * 0x9E3779B97F4A7C15ull + h1) & mask;
    for (int64_t n = 0; n < cap; ++n, s = (s + 1) & mask) {
        const uint64_t k0 = keys[2 * s];
        if (k0 == LM_EMPTY) return -1;
        if (k0 == h0 && keys[2 * s + 1] == h1) return (int64_t)s;
    }
    return -1;
}

template <class P> __device__ __forceinline__ int lm_word(const P &p, uint64_t h0, uint64_t h1) {
    const int64_t s = lm_find_pair(p.word_keys, p.word_cap, h0, h1);
    if (s < 0) return -1;
    const int id = p.word_ids[s];
    return id >= 0 && id < p.n_words ? id : -1;
}

// entry of the n-gram (context entry ctx, word w), -1 when not stored
template <class P> __device__ __forceinline__ int lm_ngram(const P &p, int ctx, int w) {
    const uint64_t key = ((uint64_t)(uint32_t)ctx << 32) | (uint32_t)w, mask = (uint64_t)p.ngram_cap - 1;
    uint64_t s = lm_mix(key) & mask;
    for (int64_t n = 0; n < p.ngram_cap; ++n, s = (s + 1) & mask) {
        const uint64_t k = p.ngram_keys[s];
        if (k == LM_EMPTY) return -1;
        if (k == key) {
            const int e = p.ngram_vals[s];
            return e >= 0 && e < p.n_entries ? e : -1;
        }
    }
    return -1;
}

// log10 p(w | ctx) by ARPA backoff for the word id w, and the context after w.  e[k] is the entry of (last k words, w): the
// longest stored one gives the probability, every longer context adds its backoff when it is stored.  The probes are independent.
template <class P> __device__ __forceinline__ double lm_cond(const P &p, const int32_t ctx[LM_CTX], int w, int32_t next[LM_CTX]) {
    int32_t e[LM_ORDER_MAX];
    e[0] = w;
#pragma unroll
    for (int k = 1; k < LM_ORDER_MAX; ++k) e[k] = (k < p.order && ctx[k - 1] >= 0) ? lm_ngram(p, ctx[k - 1], w) : -1;
    int hit = 0;
#pragma unroll
    for (int k = 1; k < LM_ORDER_MAX; ++k) hit = e[k] >= 0 ? k : hit;
    int32_t eh = e[0];
#pragma unroll
    for (int k = 1; k < LM_ORDER_MAX; ++k) eh = hit == k ? e[k] : eh;
    double lw = (double)p.lm_prob[eh];
#pragma unroll
    for (int j = 1; j < LM_ORDER_MAX; ++j)
        if (j > hit && j < p.order && ctx[j - 1] >= 0) lw += (double)p.lm_backoff[ctx[j - 1]];
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) next[k] = k + 1 < p.order ? e[k] : -1;
    return lw;
}

// the word with hashes (h0, h1) is completed: LM(text) grows by its word_score, the context moves on
template <class P> __device__ __forceinline__ void lm_commit(const P &p, LmState &s, uint64_t h0, uint64_t h1) {
    const int w = lm_word(p, h0, h1);
    int32_t next[LM_CTX];
    double lw;
    if (w >= 0) {
        lw = lm_cond(p, s.ctx, w, next);
    } else if (p.lm_unk >= 0) {
        lw = lm_cond(p, s.ctx, p.lm_unk, next) + p.unk_score_offset;
    } else {
        lw = p.unk_score_offset;
#pragma unroll
        for (int k = 0; k < LM_CTX; ++k) next[k] = -1;
    }
    s.lm += p.alpha_ln10 * lw + p.beta;
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) s.ctx[k] = next[k];
}

// the LM state of beam state `par` (LM state l) after the text-changing token v of class cls gave the beam state `now`
template <class P> __device__ __forceinline__ LmState lm_extend(const P &p, LmState l, const State &par, const State &now, int v, int cls) {
    if (cls == 1) {
        if (!(par.flags & F_PART_EMPTY)) lm_commit(p, l, par.hp[0], par.hp[1]);
        l.plen = p.tok_len[v];
    } else {
        l.plen += p.tok_len[v];
    }
    if ((now.flags & F_PART_EMPTY) || lm_find_pair(p.prefix_keys, p.prefix_cap, now.hp[0], now.hp[1]) >= 0) l.ps = 0.0;
    else l.ps = p.alpha_ln10 * p.unk_score_offset * fmax(1.0, (double)l.plen / 6.0);
    return l;
}

// the single initial beam's LM state into slot 0 of buffer buf (one thread calls it)
template <class P> __device__ __forceinline__ void lm_store_initial(const P &p, LmBeams &lb, int buf) {
    LmState s;
    s.lm = s.ps = 0.0;
    s.plen = 0;
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) s.ctx[k] = -1;
    if (p.order >= 2) s.ctx[0] = p.lm_bos;
    lm_store(lb, buf, 0, s);
}

// The LM block of a stream slab (ctc_beam_stream_impl.h; `block` is 8-byte aligned), K beams: lm K f64 | ps K f64 | ctx LM_CTX x K
// i32 | plen K i32.  The slab is caller memory and ctx indexes lm_backoff (lm_cond), so a load clamps every ctx to -1 unless it is
// an entry of p's tables and plen to >= 0: a damaged slab gives wrong scores, no read outside the tables.
constexpr int LM_STREAM_BYTES = 2 * 8 + LM_CTX * 4 + 4;

template <class P> __device__ __forceinline__ LmState lm_slab_load(const P &p, const char *block, int K, int r) {
    const double *d = reinterpret_cast<const double *>(block);
    const int32_t *w = reinterpret_cast<const int32_t *>(d + 2 * K);
    LmState s;
    s.lm = d[r]; s.ps = d[K + r];
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) {
        const int32_t e = w[k * K + r];
        s.ctx[k] = (e >= 0 && (int64_t)e < p.n_entries) ? e : -1;
    }
    s.plen = max(w[LM_CTX * K + r], 0);
    return s;
}

__device__ __forceinline__ void lm_slab_store(char *block, int K, int r, const LmState &s) {
    double *d = reinterpret_cast<double *>(block);
    int32_t *w = reinterpret_cast<int32_t *>(d + 2 * K);
    d[r] = s.lm; d[K + r] = s.ps;
#pragma unroll
    for (int k = 0; k < LM_CTX; ++k) w[k * K + r] = s.ctx[k];
    w[LM_CTX * K + r] = s.plen;
}

// the LM switch of the text fragments (ctc_beam_impl.h, NoLm) for this LM
struct NgramLm {
    static constexpr bool on = true;
    using Lds = LmBeams;
    using State = LmState;
    static constexpr int CTX = LM_CTX;
    static constexpr int STREAM_BYTES = LM_STREAM_BYTES;
};

inline bool lm_pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

// The LM argument checks cm_ctc_beam_lm_search and cm_ctc_beam_lm_stream share, behind check_beam_args and in the order the
// first always made them; `who` prefixes the messages.
template <class A> int check_lm_args(const A &a, const char *who) {
    CM_REQUIRE(a.word_keys && a.word_ids && a.prefix_keys && a.ngram_keys && a.ngram_vals && a.lm_prob && a.lm_backoff, CM_EINVAL,
               "%s: NULL LM table pointer", who);
    CM_REQUIRE(a.order >= 1 && a.order <= LM_ORDER_MAX, CM_EINVAL, "%s: LM order %d not in [1, %d]", who, a.order, LM_ORDER_MAX);
    CM_REQUIRE(lm_pow2(a.word_cap) && lm_pow2(a.prefix_cap) && lm_pow2(a.ngram_cap), CM_EINVAL,
               "%s: table capacities must be powers of two (word %lld, prefix %lld, n-gram %lld)", who,
               (long long)a.word_cap, (long long)a.prefix_cap, (long long)a.ngram_cap);
    CM_REQUIRE(a.n_words >= 1 && a.n_entries >= a.n_words && a.n_entries < (1ll << 31), CM_EINVAL,
               "%s: need 1 <= n_words (%d) <= n_entries (%lld) < 2^31", who, a.n_words, (long long)a.n_entries);
    CM_REQUIRE(a.lm_bos >= -1 && a.lm_bos < a.n_words && a.lm_eos >= -1 && a.lm_eos < a.n_words && a.lm_unk >= -1 && a.lm_unk < a.n_words,
               CM_EINVAL, "%s: lm_bos / lm_eos / lm_unk must be -1 or a word id below %d", who, a.n_words);
    CM_REQUIRE(std::isfinite(a.alpha) && std::isfinite(a.beta) && std::isfinite(a.unk_score_offset), CM_EINVAL,
               "%s: alpha, beta and unk_score_offset must be finite", who);
    return CM_OK;
}

}  // namespace
