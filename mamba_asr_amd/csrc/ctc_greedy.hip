// ctc_greedy.hip — greedy CTC decode (contract: cm_ctc_greedy; mamba_asr_amd/ctc_decode.py): the arg-max of every
// frame, repeats collapsed, blanks removed, with every kept token's frames and log-probability.  Compares, integer arithmetic and
// fp64 adds in a fixed order only: the bits are those of tests/ctc_score_ref.py.
// Two kernels behind one host entry:
//   argmax   grid (frame tiles, batch), 4 waves per workgroup, one wave per frame, lanes striding V.  The only pass over log_probs:
//            a scalar head up to the row's first 16-byte boundary, 16-byte loads over the body, a scalar tail -- whatever the row's
//            element offset and V.  A lane keeps (value, index), lower index on equal values; six xor-shuffle steps fold the wave.
//            best[t] goes to the workspace, -1 for a frame that holds a NaN.  Frames at and past n are never touched.
//   compact  one workgroup per utterance: keep flags and run ends from best, a block prefix sum over T in thread-strided blocks with
//            a running carry, compaction of tokens / starts / ends, then one thread per token folds its own frames in fp64.
#include "cm_common.h"

namespace {

constexpr int AM_WAVES = 4;               // waves per argmax workgroup
constexpr int AM_TILE = 16;               // frames per argmax workgroup
constexpr int CP_THREADS = 256;

struct best_t {
    float v;
    int i;
    bool nan;
};

__device__ __forceinline__ void take(best_t &b, float v, int i) {
    b.nan = b.nan || v != v;
    const bool better = v > b.v || (v == b.v && i < b.i);
    b.v = better ? v : b.v, b.i = better ? i : b.i;
}

template <bool BF16> struct row_io;
template <> struct row_io<false> {
    static constexpr int ES = 4, VEC = 4;
    static __device__ __forceinline__ float one(const char *p) { return *reinterpret_cast<const float *>(p); }
    static __device__ __forceinline__ void vec(best_t &b, const char *p, int i) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        take(b, __uint_as_float(q.x), i), take(b, __uint_as_float(q.y), i + 1), take(b, __uint_as_float(q.z), i + 2), take(b, __uint_as_float(q.w), i + 3);
    }
};
template <> struct row_io<true> {
    static constexpr int ES = 2, VEC = 8;
    static __device__ __forceinline__ float one(const char *p) { return __uint_as_float((uint32_t)*reinterpret_cast<const unsigned short *>(p) << 16); }
    static __device__ __forceinline__ void vec(best_t &b, const char *p, int i) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p);
        take(b, cm_bf16_lo(q.x), i), take(b, cm_bf16_hi(q.x), i + 1), take(b, cm_bf16_lo(q.y), i + 2), take(b, cm_bf16_hi(q.y), i + 3);
        take(b, cm_bf16_lo(q.z), i + 4), take(b, cm_bf16_hi(q.z), i + 5), take(b, cm_bf16_lo(q.w), i + 6), take(b, cm_bf16_hi(q.w), i + 7);
    }
};

// grid (ceil(T / AM_TILE), batch); block AM_WAVES * 64
template <bool BF16> __global__ __launch_bounds__(AM_WAVES * 64) void ctc_argmax_kernel(const cm_ctc_greedy_args p) {
    typedef row_io<BF16> IO;
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = max(min(p.input_lengths[b], p.T), 0);
    int32_t *best = reinterpret_cast<int32_t *>(p.workspace) + (int64_t)b * p.T;
    const char *lp = reinterpret_cast<const char *>(p.log_probs) + (int64_t)b * p.lp_bs * IO::ES;
    const int V = p.V;
    for (int t = blockIdx.x * AM_TILE + wave; t < min(n, (int)(blockIdx.x + 1) * AM_TILE); t += AM_WAVES) {
        const char *row = lp + (int64_t)t * p.lp_ts * IO::ES;
        // elements in front of the first 16-byte boundary (rows are aligned to their element size)
        const int head = min(V, (int)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / IO::ES));
        const int nvec = (V - head) / IO::VEC, tail0 = head + nvec * IO::VEC;
        best_t acc = {-__builtin_huge_valf(), 0x7fffffff, false};
        if (lane < head) take(acc, IO::one(row + (int64_t)lane * IO::ES), lane);
        const char *body = row + (int64_t)head * IO::ES;
#pragma unroll 4
        for (int k = lane; k < nvec; k += 64) IO::vec(acc, body + (int64_t)k * 16, head + k * IO::VEC);
        if (tail0 + lane < V) take(acc, IO::one(row + (int64_t)(tail0 + lane) * IO::ES), tail0 + lane);
        // fold the wave: every lane ends with the same (value, index)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(acc.v, m, 64);
            const int oi = __shfl_xor(acc.i, m, 64);
            const bool better = ov > acc.v || (ov == acc.v && oi < acc.i);
            acc.v = better ? ov : acc.v, acc.i = better ? oi : acc.i;
        }
        const bool any_nan = __ballot(acc.nan) != 0;
        if (lane == 0) best[t] = any_nan ? -1 : acc.i;
    }
}

// grid (batch); block CP_THREADS
template <bool BF16> __global__ __launch_bounds__(CP_THREADS) void ctc_compact_kernel(const cm_ctc_greedy_args p) {
    typedef row_io<BF16> IO;
    constexpr int NW = CP_THREADS / 64;
    __shared__ int wsum[NW];
    const int b = blockIdx.x, j = threadIdx.x, wave = j >> 6, lane = j & 63;
    const int n = max(min(p.input_lengths[b], p.T), 0), T = p.T;
    const int32_t *best = reinterpret_cast<const int32_t *>(p.workspace) + (int64_t)b * T;
    int32_t *tokens = p.tokens + (int64_t)b * T, *starts = p.starts + (int64_t)b * T, *ends = p.ends + (int64_t)b * T;
    double *logp = p.token_logp + (int64_t)b * T;

    int bad = 0;
    for (int t = j; t < n; t += CP_THREADS) bad |= best[t] < 0;
    const int any_nan = __syncthreads_or(bad);
    int carry = 0;
    if (!any_nan) {
        for (int base = 0; base < n; base += CP_THREADS) {
            const int t = base + j;
            const bool in = t < n;
            const int cur = in ? best[t] : -1, prev = (in && t > 0) ? best[t - 1] : -1, next = (in && t + 1 < n) ? best[t + 1] : -1;
            const bool keep = in && cur != p.blank && (t == 0 || cur != prev);
            const bool last = in && cur != p.blank && (t == n - 1 || next != cur);
            int x = keep ? 1 : 0;                                    // inclusive prefix sum inside the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d, 64);
                x += lane >= d ? y : 0;
            }
            if (lane == 63) wsum[wave] = x;
            __syncthreads();
            int off = 0, total = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) off += w < wave ? wsum[w] : 0, total += wsum[w];
            const int k = carry + off + x - 1;                       // the token this frame's run is
            if (keep) tokens[k] = cur, starts[k] = t;
            if (last) ends[k] = t + 1;
            carry += total;
            __syncthreads();
        }
    }
    const int len = carry;
    if (j == 0) p.token_len[b] = len, p.status[b] = any_nan ? 2 : 0;
    for (int k = len + j; k < T; k += CP_THREADS) tokens[k] = -1, starts[k] = -1, ends[k] = -1, logp[k] = 0.0;
    __syncthreads();                                                 // starts / ends of this workgroup are visible
    const char *lp = reinterpret_cast<const char *>(p.log_probs) + (int64_t)b * p.lp_bs * IO::ES;
    for (int k = j; k < len; k += CP_THREADS) {
        const int t0 = starts[k], t1 = ends[k];
        const char *col = lp + (int64_t)tokens[k] * IO::ES;
        double acc = (double)IO::one(col + (int64_t)t0 * p.lp_ts * IO::ES);
        for (int t = t0 + 1; t < t1; ++t) acc += (double)IO::one(col + (int64_t)t * p.lp_ts * IO::ES);
        logp[k] = acc;
    }
}

}  // namespace

extern "C" int64_t cm_ctc_greedy_workspace_bytes(const cm_ctc_greedy_args *a) {
    if (a == nullptr || a->batch <= 0 || a->T <= 0) return 0;
    return (int64_t)a->batch * a->T * 4;
}

extern "C" int cm_ctc_greedy(const cm_ctc_greedy_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_greedy: args is NULL");
    const cm_ctc_greedy_args a = *args;
    CM_REQUIRE(a.batch > 0 && a.T > 0 && a.V > 0, CM_EINVAL, "ctc_greedy: bad sizes batch=%d T=%d V=%d", a.batch, a.T, a.V);
    CM_REQUIRE(a.batch <= 65535, CM_EUNSUPPORTED, "ctc_greedy: at most 65535 utterances per launch (got %d)", a.batch);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "ctc_greedy: dtype %d is neither CM_F32 nor CM_BF16", a.dtype);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "ctc_greedy: blank %d out of range", a.blank);
    const int es = a.dtype == CM_BF16 ? 2 : 4;
    CM_REQUIRE(a.lp_ts >= a.V && a.lp_bs >= 0, CM_EINVAL, "ctc_greedy: bad strides lp_bs=%lld lp_ts=%lld", (long long)a.lp_bs, (long long)a.lp_ts);
    CM_REQUIRE(((int64_t)(a.T - 1) * a.lp_ts + a.V) * es <= 0x7ffffff0ll, CM_EUNSUPPORTED, "ctc_greedy: one row of log_probs spans more than 2 GiB");
    CM_REQUIRE(a.log_probs && a.input_lengths && a.tokens && a.starts && a.ends && a.token_len && a.token_logp && a.status && a.workspace,
               CM_EINVAL, "ctc_greedy: NULL tensor");
    CM_REQUIRE(cm_aligned(a.log_probs, es) && cm_aligned(a.input_lengths, 4) && cm_aligned(a.tokens, 4) && cm_aligned(a.starts, 4) &&
                   cm_aligned(a.ends, 4) && cm_aligned(a.token_len, 4) && cm_aligned(a.token_logp, 8) && cm_aligned(a.status, 4) &&
                   cm_aligned(a.workspace, 16),
               CM_EALIGN, "ctc_greedy: a tensor is not aligned to its element size (workspace: 16 bytes)");
    const int64_t need = (int64_t)a.batch * a.T * 4;
    CM_REQUIRE(a.workspace_bytes >= need, CM_EINVAL, "ctc_greedy: workspace smaller than cm_ctc_greedy_workspace_bytes() (%lld < %lld)",
               (long long)a.workspace_bytes, (long long)need);
    hipStream_t st = reinterpret_cast<hipStream_t>(a.stream);
    const dim3 grid((a.T + AM_TILE - 1) / AM_TILE, a.batch);
    if (a.dtype == CM_BF16) {
        hipLaunchKernelGGL(ctc_argmax_kernel<true>, grid, dim3(AM_WAVES * 64), 0, st, a);
        hipLaunchKernelGGL(ctc_compact_kernel<true>, dim3(a.batch), dim3(CP_THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL(ctc_argmax_kernel<false>, grid, dim3(AM_WAVES * 64), 0, st, a);
        hipLaunchKernelGGL(ctc_compact_kernel<false>, dim3(a.batch), dim3(CP_THREADS), 0, st, a);
    }
    return cm_launch_status("cm_ctc_greedy");
}
