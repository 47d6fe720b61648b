// attn_step.hip — one decoding step of multi-head self-attention over a KV cache that is never moved (include/conmamba_hip.h
// cm_attn_step; modules/TransformerLM.py).
//
// A beam search reorders its hypotheses every token.  Instead of gathering the (positions, rows, D) caches by the chosen parents,
// the cache stays where it was written and anc[s][r] names the row that holds hypothesis r's prefix token of position s.
//
// One wave per (row r, head h); a workgroup is 1, 2 or 4 independent waves (no barrier, no shared data between them).
//   0. the wave's q | k | v slices go to its LDS strip as fp32, and k, v are copied bit for bit to kc[t][r], vc[t][r]
//   1. lanes along s: lane l scores positions l, l + 64, ... < t, each a dh-long fma chain in ascending d against
//      K[s][anc[s][r]]; the clamped row and the score go to LDS.  Position t is scored from the LDS strip: a row reads only cache
//      lines written by earlier launches, so no ordering between workgroups is needed.
//   2. softmax in fp32: maximum and sum folded across lanes in a fixed butterfly (ds_bpermute; an fp32 add commutes, so both
//      partners of an exchange hold the same bits), position t's share added last; p = e / sum is written back to LDS
//   3. lanes along the head dimension: lane d accumulates p[s] * V[s][row[s]][d] for s = 0 .. t in ascending order
// No atomics and a fixed summation order: bit-identical from run to run, and a row's result depends on nothing but its own
// q | k | v, its ancestry column and the cache lines that column names.
#include "cm_common.h"

#include <math.h>

namespace {

constexpr int MAX_T = CM_ATTN_STEP_MAX_T;      // positions whose scores fit the LDS strip
constexpr int MAX_H = CM_ATTN_STEP_MAX_H;

template <typename T> struct Vec;              // 16-byte pieces of a K slice
template <> struct Vec<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float *p, float (&f)[4]) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
};
template <> struct Vec<cm_bf16> {
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const cm_bf16 *p, float (&f)[8]) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        f[0] = cm_bf16_lo(v.x); f[1] = cm_bf16_hi(v.x); f[2] = cm_bf16_lo(v.y); f[3] = cm_bf16_hi(v.y);
        f[4] = cm_bf16_lo(v.z); f[5] = cm_bf16_hi(v.z); f[6] = cm_bf16_lo(v.w); f[7] = cm_bf16_hi(v.w);
    }
};

template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_step_kernel(cm_attn_step_args p, int cap) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * waves + wave;       // (row, head)
    if (unit >= (int64_t)p.R * p.H) return;                        // whole waves only; nothing below is shared between waves
    const int r = (int)(unit / p.H), h = (int)(unit - (int64_t)r * p.H);
    const int R = p.R, D = p.D, t = p.t;

    float *sc = lds + (size_t)wave * (2 * cap + 3 * 64);           // scores, then probabilities, of positions 0 .. t
    int *rw = reinterpret_cast<int *>(sc + cap);                   // the clamped cache row of each position
    float *own = sc + 2 * cap;                                     // q | k | v of this step, 64 floats each
    const T *qkv = static_cast<const T *>(p.qkv) + (int64_t)r * 3 * D + h * DH;
    T *kc = static_cast<T *>(p.kc);
    T *vc = static_cast<T *>(p.vc);
    const int64_t slice = (int64_t)r * D + h * DH;                 // of row r inside one position

    if (lane < DH) {
        const T q = qkv[lane], k = qkv[D + lane], v = qkv[2 * D + lane];
        own[lane] = cm_elem<T>::load(&q);
        own[64 + lane] = cm_elem<T>::load(&k);
        own[128 + lane] = cm_elem<T>::load(&v);
        kc[(int64_t)t * p.kv_stride + slice + lane] = k;           // the bits that came in
        vc[(int64_t)t * p.kv_stride + slice + lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // the strip is written before any lane reads it

    float q[DH];
#pragma unroll
    for (int d = 0; d < DH; ++d) q[d] = own[d];
    const float scale = 1.0f / sqrtf((float)DH);

    // 1. scores of the cached positions
    float m = -INFINITY;
    for (int s = lane; s < t; s += 64) {
        const int a = p.anc[(int64_t)s * R + r];
        const bool ok = a >= 0 && a < R;
        const int row = min(max(a, 0), R - 1);                     // an entry outside [0, R) loads row 0 or R - 1 and scores -inf
        const T *kp = kc + (int64_t)s * p.kv_stride + (int64_t)row * D + h * DH;
        float dot = 0.f;
#pragma unroll
        for (int d0 = 0; d0 < DH; d0 += Vec<T>::N) {
            float f[Vec<T>::N];
            Vec<T>::load(kp + d0, f);
#pragma unroll
            for (int j = 0; j < Vec<T>::N; ++j) dot = fmaf(q[d0 + j], f[j], dot);
        }
        const float x = ok ? dot * scale : -INFINITY;
        sc[s] = x;
        rw[s] = row;
        m = fmaxf(m, x);
    }
    float dot_t = 0.f;                                             // position t: the same chain on this step's own k, in every lane
#pragma unroll
    for (int d = 0; d < DH; ++d) dot_t = fmaf(q[d], own[64 + d], dot_t);
    const float x_t = dot_t * scale;

    // 2. softmax
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    m = fmaxf(m, x_t);                                             // finite unless the step's own score is NaN / inf
    float sum = 0.f;
    for (int s = lane; s < t; s += 64) {
        const float e = expf(sc[s] - m);                           // -inf -> 0
        sc[s] = e;
        sum += e;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    const float e_t = expf(x_t - m);
    sum += e_t;
    for (int s = lane; s < t; s += 64) sc[s] = sc[s] / sum;
    const float p_t = e_t / sum;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // 3. p . V, lanes along the head dimension
    if (lane < DH) {
        const T *vbase = vc + h * DH + lane;
        float acc = 0.f;
#pragma unroll 8
        for (int s = 0; s < t; ++s) {
            const float ps = sc[s];
            const T raw = vbase[(int64_t)s * p.kv_stride + (int64_t)rw[s] * D];
            const float v = cm_elem<T>::load(&raw);
            acc = fmaf(ps, ps == 0.f ? 0.f : v, acc);              // a position without weight contributes nothing, whatever it holds
        }
        acc = fmaf(p_t, own[128 + lane], acc);
        cm_elem<T>::store(static_cast<T *>(p.out) + slice + lane, acc);
    }
}

template <typename T>
void launch(const cm_attn_step_args &a, int dh, dim3 grid, int waves, int cap, size_t lds_bytes, hipStream_t stream) {
    if (dh == 32) hipLaunchKernelGGL((attn_step_kernel<T, 32>), grid, dim3(64 * waves), lds_bytes, stream, a, cap);
    else hipLaunchKernelGGL((attn_step_kernel<T, 64>), grid, dim3(64 * waves), lds_bytes, stream, a, cap);
}

}  // namespace

extern "C" int cm_attn_step(const cm_attn_step_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "attn_step: args is NULL");
    const cm_attn_step_args a = *args;
    CM_REQUIRE(a.R >= 1 && a.D >= 1 && a.H >= 1 && a.D % a.H == 0 && a.t >= 0, CM_EINVAL,
               "attn_step: bad sizes R=%d D=%d H=%d t=%d (R, D, H >= 1, D a multiple of H, t >= 0)", a.R, a.D, a.H, a.t);
    CM_REQUIRE(a.Lcap > a.t, CM_EINVAL, "attn_step: the caches hold %d positions, position t=%d does not fit", a.Lcap, a.t);
    const int dh = a.D / a.H;
    CM_REQUIRE(a.io_dtype == CM_F32 || a.io_dtype == CM_BF16, CM_EUNSUPPORTED, "attn_step: io dtype %d unsupported (fp32 / bf16)",
               a.io_dtype);
    CM_REQUIRE(dh == 32 || dh == 64, CM_EUNSUPPORTED, "attn_step: head dimension %d unsupported (32 or 64)", dh);
    CM_REQUIRE(a.H <= MAX_H, CM_EUNSUPPORTED, "attn_step: %d heads unsupported (at most %d)", a.H, MAX_H);
    CM_REQUIRE(a.t < MAX_T, CM_EUNSUPPORTED, "attn_step: t=%d unsupported (the scores of at most %d positions fit in LDS)", a.t, MAX_T);
    CM_REQUIRE(a.qkv && a.kc && a.vc && a.anc && a.out, CM_EINVAL, "attn_step: NULL pointer");
    const int64_t item = a.io_dtype == CM_F32 ? 4 : 2;
    CM_REQUIRE(cm_aligned(a.qkv, 16) && cm_aligned(a.kc, 16) && cm_aligned(a.vc, 16) && cm_aligned(a.out, 16) && cm_aligned(a.anc, 4),
               CM_EINVAL, "attn_step: misaligned pointer (qkv / kc / vc / out 16 bytes, anc 4)");
    CM_REQUIRE(a.kv_stride >= (int64_t)a.R * a.D && (a.kv_stride * item) % 16 == 0, CM_EINVAL,
               "attn_step: position stride %lld (elements) must be at least R * D = %lld and a multiple of 16 bytes",
               (long long)a.kv_stride, (long long)a.R * a.D);
    const int64_t units = (int64_t)a.R * a.H;
    const int cap = (a.t + 1 + 63) / 64 * 64;
    const int waves = cap <= 1024 ? 4 : cap <= 2048 ? 2 : 1;       // 2 * cap + 192 floats per wave: at most 36 KiB per workgroup
    const int64_t blocks = (units + waves - 1) / waves;
    CM_REQUIRE(blocks <= 0x7fffffff, CM_EINVAL, "attn_step: R * H = %lld is too large", (long long)units);
    const size_t lds_bytes = (size_t)waves * (2 * cap + 3 * 64) * sizeof(float);
    hipStream_t stream = reinterpret_cast<hipStream_t>(a.stream);
    if (a.io_dtype == CM_F32) launch<float>(a, dh, dim3((unsigned)blocks), waves, cap, lds_bytes, stream);
    else launch<cm_bf16>(a, dh, dim3((unsigned)blocks), waves, cap, lds_bytes, stream);
    return cm_launch_status("cm_attn_step");
}
