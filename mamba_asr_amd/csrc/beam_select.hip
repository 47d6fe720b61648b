// beam_select.hip — the per-token selection of the S2S beam search (include/conmamba_hip.h cm_beam_select).
//
// Every candidate (beam slot k, token c) of an utterance gets one 64-bit word that is unique within the utterance:
//   high half: its joint score s as an order-preserving 32-bit key (NaN -> -inf, -0 -> +0)
//   low half:  0xffffffff - (k * V + c), so that among equal scores the lower flat index is the larger word
// "The B best under (s descending, flat index ascending)" is then "the B largest words", and 0 is free to mean "no candidate".
//
//   beam_rows_kernel   one workgroup per (row, chunk of CHUNK tokens): the chunk's scores are computed once into registers, an
//                      8-bit radix select over LDS histograms finds its min(B, length) largest words, and they go to the
//                      workspace (in no particular order) with their increments.
//   beam_merge_kernel  one workgroup per utterance: the same radix select over the utterance's B * chunks * B words, then
//                      the B survivors are ranked by counting and written as (score, inc, parent, token).
// An utterance's B best hold at most B candidates of one row, and a row's B best at most B of one chunk: the split is exact.
// The select stops as soon as a bucket boundary falls exactly behind the K-th word (after 2-3 passes for distinct scores; a row of
// equal scores takes all 8).  Histogram counts are integers: the order of the LDS atomics does not reach the result.
#include "cm_common.h"

#include <math.h>

namespace {

constexpr int MAX_B = CM_BEAM_SELECT_MAX_B;
constexpr int NT1 = 256;                       // beam_rows_kernel: threads
constexpr int ITEMS = 20;                      // tokens per thread, in registers
constexpr int CHUNK = NT1 * ITEMS;             // tokens per workgroup: one chunk covers the recipes' 5000-token vocabulary
constexpr int NT2 = 512;                       // beam_merge_kernel: threads
static_assert(CHUNK == CM_BEAM_SELECT_CHUNK, "the header states the chunk");
static_assert(CHUNK >= MAX_B, "a dead row's B best lie in its first chunk");

struct Select {                                // the radix select's workgroup state
    unsigned hist[256];
    unsigned digit, need, done, count;
};

__device__ __forceinline__ uint32_t score_key(float s) {
    if (!(s == s)) s = -INFINITY;              // NaN ranks as -inf
    if (s == 0.f) s = 0.f;                     // -0 ties with +0
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

// After a pass's histogram is complete: the first wave finds the digit d with  #(digits above d) < need <= #(digits >= d)  and
// leaves d, the count still to take inside d's bucket, and whether the bucket is taken whole.  Lane l owns digits 255-4l .. 252-4l.
__device__ __forceinline__ void pick_digit(Select &st, int tid, unsigned need) {
    if (tid < 64) {
        unsigned h[4], tot = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { h[q] = st.hist[255 - 4 * tid - q]; tot += h[q]; }
        unsigned incl = tot;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 64);
            if (tid >= d) incl += o;
        }
        unsigned above = incl - tot;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (above < need && need <= above + h[q]) {
                st.digit = 255 - 4 * tid - q;
                st.need = need - above;
                st.done = above + h[q] == need;
            }
            above += h[q];
        }
    }
}

__device__ __forceinline__ void joint_score(float a, bool has_delta, float d, float weight, float alive, float &inc, float &s) {
    // three separately rounded fp32 operations: what torch computes with the same three, and what the greedy searcher
    // accumulates.  The library is built with -ffp-contract=fast, under which the backend fuses a multiply into the add behind it
    // whatever the pragma says (it gave v_fma_f32 here): the product is therefore pinned in a register before it is added.
#pragma clang fp contract(off)
    inc = a;
    if (has_delta) {
        float m = weight * d;
        asm("" : "+v"(m));
        inc = a + m;
    }
    s = alive + inc;
}

__global__ __launch_bounds__(NT1) void beam_rows_kernel(cm_beam_select_args p, uint64_t *wcomp, float *winc, int nch) {
    __shared__ Select st;
    const int row = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int B = p.B, V = p.V;
    const int u = row / B, k = row - u * B;
    const int c0 = chunk * CHUNK;
    const int len = min(CHUNK, V - c0);
    const int K = min(B, len);
    const float alive = p.alive[row];
    const bool blocked = p.eos_blocked != nullptr && p.eos_blocked[u] != 0;
    const float *att = p.att + (int64_t)row * V + c0;
    const float *del = p.delta ? p.delta + (int64_t)row * V + c0 : nullptr;
    const uint32_t low0 = 0xffffffffu - (uint32_t)(k * V + c0);      // B * V < 2^31: no wrap

    uint32_t key[ITEMS];
    float inc[ITEMS];
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int i = j * NT1 + tid;
        key[j] = 0;
        inc[j] = 0.f;
        if (i < len) {
            float a = att[i];
            if (blocked && c0 + i == p.eos) a = -INFINITY;
            float s;
            joint_score(a, del != nullptr, del ? del[i] : 0.f, p.weight, alive, inc[j], s);
            key[j] = score_key(s);
        }
    }

    // radix select of the K largest words, most significant byte first
    uint64_t prefix = 0;
    unsigned need = K;
    int shift = 64;
    for (int pass = 0; pass < 8; ++pass) {
        shift -= 8;
        st.hist[tid] = 0;                       // NT1 == 256 bins
        __syncthreads();
        unsigned run = 0, run_digit = 0;        // equal digits in a row cost one atomic: a thread's tokens mostly share the top bytes
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int i = j * NT1 + tid;
            if (i < len) {
                const uint64_t w = ((uint64_t)key[j] << 32) | (low0 - (uint32_t)i);
                if (pass == 0 || (w >> (shift + 8)) == prefix) {
                    const unsigned d = (unsigned)(w >> shift) & 255u;
                    if (run && d != run_digit) { atomicAdd(&st.hist[run_digit], run); run = 0; }
                    run_digit = d;
                    ++run;
                }
            }
        }
        if (run) atomicAdd(&st.hist[run_digit], run);
        __syncthreads();
        pick_digit(st, tid, need);
        __syncthreads();
        prefix = (prefix << 8) | st.digit;
        need = st.need;
        if (st.done) break;                     // uniform: every thread reads the same word
    }
    if (tid == 0) st.count = 0;
    __syncthreads();
    const int64_t base = ((int64_t)row * nch + chunk) * B;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int i = j * NT1 + tid;
        if (i < len) {
            const uint64_t w = ((uint64_t)key[j] << 32) | (low0 - (uint32_t)i);
            if ((w >> shift) >= prefix) {
                const unsigned pos = atomicAdd(&st.count, 1u);
                if (pos < (unsigned)K) { wcomp[base + pos] = w; winc[base + pos] = inc[j]; }
            }
        }
    }
    for (int i = K + tid; i < B; i += NT1) { wcomp[base + i] = 0; winc[base + i] = 0.f; }   // no candidate
}

__global__ __launch_bounds__(NT2) void beam_merge_kernel(cm_beam_select_args p, const uint64_t *wcomp, const float *winc, int nch) {
    __shared__ Select st;
    __shared__ uint64_t best[MAX_B];
    __shared__ int best_src[MAX_B];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int B = p.B, V = p.V;
    const int n = B * nch * B;                  // <= 128 * 128 * 65535 < 2^31
    const uint64_t *comp = wcomp + (int64_t)u * n;

    uint64_t prefix = 0;
    unsigned need = B;
    int shift = 64;
    for (int pass = 0; pass < 8; ++pass) {
        shift -= 8;
        if (tid < 256) st.hist[tid] = 0;
        __syncthreads();
        unsigned run = 0, run_digit = 0;
        for (int i = tid; i < n; i += NT2) {
            const uint64_t w = comp[i];
            if (w != 0 && (pass == 0 || (w >> (shift + 8)) == prefix)) {
                const unsigned d = (unsigned)(w >> shift) & 255u;
                if (run && d != run_digit) { atomicAdd(&st.hist[run_digit], run); run = 0; }
                run_digit = d;
                ++run;
            }
        }
        if (run) atomicAdd(&st.hist[run_digit], run);
        __syncthreads();
        pick_digit(st, tid, need);
        __syncthreads();
        prefix = (prefix << 8) | st.digit;
        need = st.need;
        if (st.done) break;
    }
    if (tid == 0) st.count = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT2) {
        const uint64_t w = comp[i];
        if (w != 0 && (w >> shift) >= prefix) {
            const unsigned pos = atomicAdd(&st.count, 1u);
            if (pos < (unsigned)B) { best[pos] = w; best_src[pos] = i; }
        }
    }
    __syncthreads();
    const int got = min((int)st.count, B);      // == B: at least B words of an utterance are candidates
    if (tid < got) {
        const uint64_t w = best[tid];
        int rank = 0;
        for (int i = 0; i < got; ++i) rank += best[i] > w;           // the words are distinct
        const uint32_t flat = 0xffffffffu - (uint32_t)w;
        const int64_t o = (int64_t)u * B + rank;
        p.score[o] = key_score((uint32_t)(w >> 32));
        p.inc[o] = winc[(int64_t)u * n + best_src[tid]];
        p.parent[o] = (int32_t)(flat / (uint32_t)V);
        p.token[o] = (int32_t)(flat % (uint32_t)V);
    }
}

// chunks per row, or 0 for sizes the entry point refuses
int64_t chunks_of(int32_t U, int32_t B, int32_t V) {
    if (U < 1 || B < 1 || B > MAX_B || V < 1 || (int64_t)B * V >= (int64_t)1 << 31 || (int64_t)U * B > 0x7fffffff) return 0;
    const int64_t nch = ((int64_t)V + CHUNK - 1) / CHUNK;
    return nch <= 65535 ? nch : 0;
}

}  // namespace

extern "C" int64_t cm_beam_select_workspace_bytes(int32_t U, int32_t B, int32_t V) {
    return (int64_t)U * B * chunks_of(U, B, V) * B * (int64_t)(sizeof(uint64_t) + sizeof(float));
}

extern "C" int cm_beam_select(const cm_beam_select_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "beam_select: args is NULL");
    const cm_beam_select_args a = *args;
    CM_REQUIRE(a.U >= 1 && a.B >= 1 && a.B <= MAX_B && a.V >= 1 && (int64_t)a.B * a.V < (int64_t)1 << 31 &&
                   (int64_t)a.U * a.B <= 0x7fffffff, CM_EINVAL,
               "beam_select: bad sizes U=%d B=%d V=%d (1 <= B <= %d, B * V < 2^31)", a.U, a.B, a.V, MAX_B);
    const int64_t nch = chunks_of(a.U, a.B, a.V);
    CM_REQUIRE(nch > 0, CM_EUNSUPPORTED, "beam_select: V=%d needs more than 65535 chunks of %d tokens", a.V, CHUNK);
    CM_REQUIRE(a.att && a.alive && a.score && a.inc && a.parent && a.token && a.workspace, CM_EINVAL, "beam_select: NULL pointer");
    CM_REQUIRE(cm_aligned(a.att, 4) && cm_aligned(a.delta, 4) && cm_aligned(a.alive, 4) && cm_aligned(a.eos_blocked, 4) &&
                   cm_aligned(a.score, 4) && cm_aligned(a.inc, 4) && cm_aligned(a.parent, 4) && cm_aligned(a.token, 4) &&
                   cm_aligned(a.workspace, 8), CM_EINVAL, "beam_select: misaligned pointer (4 bytes; workspace 8)");
    const int64_t slots = (int64_t)a.U * a.B * nch * a.B;
    CM_REQUIRE(a.workspace_bytes >= cm_beam_select_workspace_bytes(a.U, a.B, a.V), CM_EINVAL,
               "beam_select: workspace of %lld bytes, need %lld", (long long)a.workspace_bytes,
               (long long)cm_beam_select_workspace_bytes(a.U, a.B, a.V));
    uint64_t *wcomp = static_cast<uint64_t *>(a.workspace);
    float *winc = reinterpret_cast<float *>(wcomp + slots);
    hipStream_t stream = reinterpret_cast<hipStream_t>(a.stream);
    hipLaunchKernelGGL(beam_rows_kernel, dim3((unsigned)(a.U * a.B), (unsigned)nch), dim3(NT1), 0, stream, a, wcomp, winc, (int)nch);
    hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)a.U), dim3(NT2), 0, stream, a, wcomp, winc, (int)nch);
    return cm_launch_status("cm_beam_select");
}
