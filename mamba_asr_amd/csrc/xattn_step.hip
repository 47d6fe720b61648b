// xattn_step.hip — one decoding step of multi-head cross-attention: R hypothesis rows over the encoder memory of their utterance
// (include/conmamba_hip.h cm_xattn_step; modules/Transformer.py).
//
// K and V of an utterance were projected once and are shared by every beam of it: nothing is tiled, copied or written here.
// The key count is the utterance's full length from the first token on, so the sum over frames is the whole cost.
//
// One wave per (row r, head h); a workgroup is 1, 2 or 4 independent waves (no barrier, no shared data between them).
//   1. lanes along s: lane l scores frames l, l + 64, ... < n, each a dh-long fma chain in ascending d against K[u][s][h];
//      the scores go to the wave's LDS strip
//   2. softmax in fp32: maximum and sum folded across lanes in a fixed butterfly (ds_bpermute; an fp32 add commutes, so both
//      partners of an exchange hold the same bits); e = exp(x - max) is written back to LDS
//   3. lanes along (frame group g, piece j of a V row): LPR = dh / N lanes cover one V row with one 16- or 8-byte load each,
//      G = 64 / LPR groups take frames g, g + G, ... in ascending order; the G partial sums go to LDS and lane d < dh adds
//      them in ascending g, then divides by the softmax denominator
// Frames at or beyond n = min(enc_len[u], T) are never loaded.  No atomics and a fixed summation order: bit-identical from run
// to run, and a row's result depends on nothing but its own q and its utterance's K / V.
#include "cm_common.h"

#include <math.h>

namespace {

constexpr int MAX_T = CM_XATTN_STEP_MAX_T;     // frames whose scores fit the LDS strip
constexpr int MAX_H = CM_XATTN_STEP_MAX_H;
constexpr int PART = 512;                      // floats of partial sums per wave: G * dh <= 64 * N <= 512

template <typename T, int N> struct Piece;     // N elements of a head slice in one load
template <> struct Piece<float, 4> {
    static __device__ __forceinline__ void load(const float *p, float (&f)[4]) {
        const float4 v = *reinterpret_cast<const float4 *>(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    }
};
template <> struct Piece<cm_bf16, 8> {
    static __device__ __forceinline__ void load(const cm_bf16 *p, float (&f)[8]) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        f[0] = cm_bf16_lo(v.x); f[1] = cm_bf16_hi(v.x); f[2] = cm_bf16_lo(v.y); f[3] = cm_bf16_hi(v.y);
        f[4] = cm_bf16_lo(v.z); f[5] = cm_bf16_hi(v.z); f[6] = cm_bf16_lo(v.w); f[7] = cm_bf16_hi(v.w);
    }
};
template <> struct Piece<cm_bf16, 4> {         // the slices of a 36-wide bf16 head are 8-byte aligned only
    static __device__ __forceinline__ void load(const cm_bf16 *p, float (&f)[4]) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        f[0] = cm_bf16_lo(v.x); f[1] = cm_bf16_hi(v.x); f[2] = cm_bf16_lo(v.y); f[3] = cm_bf16_hi(v.y);
    }
};

template <typename T, int DH, int N>
__global__ __launch_bounds__(256) void xattn_step_kernel(cm_xattn_step_args p, int cap) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int LPR = DH / N;                                    // lanes per V row
    constexpr int G = 64 / LPR;                                    // frame groups of step 3
    static_assert(DH % N == 0 && G >= 1 && G * DH <= PART, "piece / partial-sum layout");
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    const int64_t unit = (int64_t)blockIdx.x * waves + wave;       // (row, head)
    if (unit >= (int64_t)p.R * p.H) return;                        // whole waves only; nothing below is shared between waves
    const int r = (int)(unit / p.H), h = (int)(unit - (int64_t)r * p.H);
    const int D = p.D;

    float *sc = lds + (size_t)wave * (cap + PART);                 // scores, then exponentials, of frames 0 .. n - 1
    float *part = sc + cap;                                        // G partial sums of dh floats
    T *out = static_cast<T *>(p.out) + (int64_t)r * D + h * DH;

    const int u = p.row_utt[r];
    int n = 0;
    if (u >= 0 && u < p.U) n = min(p.enc_len[u], p.T);
    if (n < 1) {                                                   // the same for every lane of the wave
        if (lane < DH) cm_elem<T>::store(out + lane, 0.f);
        return;
    }
    const T *kb = static_cast<const T *>(p.k) + (int64_t)u * p.k_utt_stride + h * DH;
    const T *vb = static_cast<const T *>(p.v) + (int64_t)u * p.v_utt_stride + h * DH;
    const T *qp = static_cast<const T *>(p.q) + (int64_t)r * D + h * DH;

    float q[DH];
#pragma unroll
    for (int d0 = 0; d0 < DH; d0 += N) {
        float f[N];
        Piece<T, N>::load(qp + d0, f);
#pragma unroll
        for (int j = 0; j < N; ++j) q[d0 + j] = f[j];
    }
    const float scale = 1.0f / sqrtf((float)DH);

    // 1. scores
    float m = -INFINITY;
    for (int s = lane; s < n; s += 64) {
        const T *kp = kb + (int64_t)s * p.k_frame_stride;
        float dot = 0.f;
#pragma unroll
        for (int d0 = 0; d0 < DH; d0 += N) {
            float f[N];
            Piece<T, N>::load(kp + d0, f);
#pragma unroll
            for (int j = 0; j < N; ++j) dot = fmaf(q[d0 + j], f[j], dot);
        }
        const float x = dot * scale;
        sc[s] = x;
        m = fmaxf(m, x);
    }

    // 2. softmax
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    float sum = 0.f;
    for (int s = lane; s < n; s += 64) {
        const float e = expf(sc[s] - m);
        sc[s] = e;
        sum += e;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");             // every lane's exponentials are written before any lane reads them

    // 3. e . V: G interleaved partial sums
    const int g = lane / LPR, j = lane - g * LPR;
    if (g < G) {
        float acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.f;
        const T *vp = vb + j * N;
#pragma unroll 4
        for (int s = g; s < n; s += G) {
            const float e = sc[s];
            float f[N];
            Piece<T, N>::load(vp + (int64_t)s * p.v_frame_stride, f);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] = fmaf(e, f[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) part[lane * N + i] = acc[i];   // = part[g * DH + j * N + i]
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < DH) {
        float o = 0.f;
#pragma unroll
        for (int gg = 0; gg < G; ++gg) o += part[gg * DH + lane];
        cm_elem<T>::store(out + lane, o / sum);
    }
}

template <typename T, int DH, int N>
void launch(const cm_xattn_step_args &a, dim3 grid, int waves, int cap, size_t lds_bytes, hipStream_t stream) {
    hipLaunchKernelGGL((xattn_step_kernel<T, DH, N>), grid, dim3(64 * waves), lds_bytes, stream, a, cap);
}

}  // namespace

extern "C" int cm_xattn_step(const cm_xattn_step_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "xattn_step: args is NULL");
    const cm_xattn_step_args a = *args;
    CM_REQUIRE(a.R >= 1 && a.U >= 1 && a.T >= 1 && a.D >= 1 && a.H >= 1 && a.D % a.H == 0, CM_EINVAL,
               "xattn_step: bad sizes R=%d U=%d T=%d D=%d H=%d (all >= 1, D a multiple of H)", a.R, a.U, a.T, a.D, a.H);
    const int dh = a.D / a.H;
    CM_REQUIRE(a.io_dtype == CM_F32 || a.io_dtype == CM_BF16, CM_EUNSUPPORTED, "xattn_step: io dtype %d unsupported (fp32 / bf16)",
               a.io_dtype);
    CM_REQUIRE(dh == 32 || dh == 36 || dh == 64, CM_EUNSUPPORTED, "xattn_step: head dimension %d unsupported (32, 36 or 64)", dh);
    CM_REQUIRE(a.H <= MAX_H, CM_EUNSUPPORTED, "xattn_step: %d heads unsupported (at most %d)", a.H, MAX_H);
    CM_REQUIRE(a.T < MAX_T, CM_EUNSUPPORTED, "xattn_step: T=%d unsupported (the scores of fewer than %d frames fit in LDS)", a.T, MAX_T);
    CM_REQUIRE(a.q && a.k && a.v && a.row_utt && a.enc_len && a.out, CM_EINVAL, "xattn_step: NULL pointer");
    const int64_t item = a.io_dtype == CM_F32 ? 4 : 2;
    CM_REQUIRE(cm_aligned(a.q, 16) && cm_aligned(a.k, 16) && cm_aligned(a.v, 16) && cm_aligned(a.out, 16) && cm_aligned(a.row_utt, 4)
                   && cm_aligned(a.enc_len, 4),
               CM_EINVAL, "xattn_step: misaligned pointer (q / k / v / out 16 bytes, row_utt / enc_len 4)");
    CM_REQUIRE(((int64_t)a.D * item) % 16 == 0, CM_EINVAL, "xattn_step: a row of D=%d elements is no multiple of 16 bytes", a.D);
    const int64_t fs[2] = {a.k_frame_stride, a.v_frame_stride}, us[2] = {a.k_utt_stride, a.v_utt_stride};
    for (int i = 0; i < 2; ++i) {
        CM_REQUIRE(fs[i] >= a.D && (fs[i] * item) % 16 == 0, CM_EINVAL,
                   "xattn_step: frame stride %lld (elements) of %s must be at least D = %d and a multiple of 16 bytes", (long long)fs[i],
                   i ? "v" : "k", a.D);
        CM_REQUIRE(us[i] >= (int64_t)(a.T - 1) * fs[i] + a.D && (us[i] * item) % 16 == 0, CM_EINVAL,
                   "xattn_step: utterance stride %lld (elements) of %s must be at least (T - 1) * frame stride + D = %lld and a multiple "
                   "of 16 bytes", (long long)us[i], i ? "v" : "k", (long long)((int64_t)(a.T - 1) * fs[i] + a.D));
    }
    const int64_t units = (int64_t)a.R * a.H;
    const int cap = (a.T + 63) / 64 * 64;
    const int waves = cap <= 1024 ? 4 : cap <= 2048 ? 2 : 1;       // cap + 512 floats per wave: at most 34 KiB per workgroup
    const int64_t blocks = (units + waves - 1) / waves;
    CM_REQUIRE(blocks <= 0x7fffffff, CM_EINVAL, "xattn_step: R * H = %lld is too large", (long long)units);
    const size_t lds_bytes = (size_t)waves * (cap + PART) * sizeof(float);
    hipStream_t stream = reinterpret_cast<hipStream_t>(a.stream);
    const dim3 grid((unsigned)blocks);
    if (a.io_dtype == CM_F32) {
        if (dh == 32) launch<float, 32, 4>(a, grid, waves, cap, lds_bytes, stream);
        else if (dh == 36) launch<float, 36, 4>(a, grid, waves, cap, lds_bytes, stream);
        else launch<float, 64, 4>(a, grid, waves, cap, lds_bytes, stream);
    } else {
        if (dh == 32) launch<cm_bf16, 32, 8>(a, grid, waves, cap, lds_bytes, stream);
        else if (dh == 36) launch<cm_bf16, 36, 4>(a, grid, waves, cap, lds_bytes, stream);
        else launch<cm_bf16, 64, 8>(a, grid, waves, cap, lds_bytes, stream);
    }
    return cm_launch_status("cm_xattn_step");
}
