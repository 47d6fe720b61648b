// mamba_step.hip — one decoding step of a Mamba mixer between in_proj and out_proj as ONE launch for gfx950 (contract:
// cm_mamba_step in include/conmamba_hip.h; reference modules/mamba/bimamba.py:331-362).  state_update.hip holds the two
// per-stage kernels this one fuses with the x_proj / dt_proj GEMVs that sat between them: five launches and the copies
// of torch.split / chunk per mixer step become one, which is what a token loop pays for (two mixers per decoder layer).
//
// One workgroup of 8 waves per batch row; four phases separated by workgroup barriers:
//   1  thread per channel: conv-state shift + append (one 16-byte load and store), conv + bias + SiLU -> x in LDS (fp32)
//   2  wave per x_proj output row: lanes stride the row in 16-byte pieces against x in LDS; the 64 lane partials go to LDS
//      (row stride 65: the summing thread of each row then hits its own bank) and ONE thread per row adds them in lane
//      order -- a fixed summation order, no atomics, no cross-lane instructions
//   3  thread per channel: dt_proj row (dt_rank <= 32 terms) + bias + softplus, then the 16 states of the channel, D skip
//      and the SiLU(z) gate; the state row is read and written once as four 16-byte vectors
// Latency-bound: the row reads (dt_rank + 32 + dt_rank) * dim weights from L2 and 20 * dim state floats.
#include "cm_common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 4096;          // x of one row in LDS (16 KiB)
constexpr int kMaxOut = 64;            // dt_rank (<= 32) + B (16) + C (16)
constexpr int kPartStride = 65;        // 64 lane partials per output row + 1: rows start on consecutive banks

template <typename IO>
__global__ __launch_bounds__(kThreads) void mamba_step_kernel(const cm_mamba_step_args p) {
    __shared__ __attribute__((aligned(16))) float s_x[kMaxDim];
    __shared__ float s_part[kMaxOut * kPartStride];
    __shared__ float s_xdbl[kMaxOut];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = p.dim, R = p.dt_rank, J = R + 32;
    const IO *xz = reinterpret_cast<const IO *>(p.xz) + (int64_t)b * 2 * E;

    // 1: conv state (oldest sample first) shifted left by one with the new sample appended; conv + bias + SiLU
    float *cs = p.conv_state + (int64_t)b * E * 4;
    for (int c = tid; c < E; c += kThreads) {
        const float4 old = *reinterpret_cast<const float4 *>(cs + 4 * c);
        const float4 w = *reinterpret_cast<const float4 *>(p.conv_weight + 4 * c);
        const float4 s = {old.y, old.z, old.w, cm_elem<IO>::load(xz + c)};
        *reinterpret_cast<float4 *>(cs + 4 * c) = s;
        float acc = p.conv_bias ? p.conv_bias[c] : 0.f;
        acc = fmaf(w.x, s.x, acc);
        acc = fmaf(w.y, s.y, acc);
        acc = fmaf(w.z, s.z, acc);
        acc = fmaf(w.w, s.w, acc);
        s_x[c] = acc * cm_sigmoid(acc);
    }
    __syncthreads();

    // 2: x_dbl = Wx x
    for (int j = wave; j < J; j += kWaves) {
        const float *wr = p.x_proj_weight + (int64_t)j * E;
        float acc = 0.f;
        for (int c = lane * 4; c < E; c += 256) {
            const float4 w = *reinterpret_cast<const float4 *>(wr + c);
            const float4 x = *reinterpret_cast<const float4 *>(s_x + c);
            acc = fmaf(w.x, x.x, acc);
            acc = fmaf(w.y, x.y, acc);
            acc = fmaf(w.z, x.z, acc);
            acc = fmaf(w.w, x.w, acc);
        }
        s_part[j * kPartStride + lane] = acc;
    }
    __syncthreads();
    if (tid < J) {
        float acc = 0.f;
#pragma unroll 16
        for (int i = 0; i < 64; ++i) acc += s_part[tid * kPartStride + i];
        s_xdbl[tid] = acc;
    }
    __syncthreads();

    // 3: dt = softplus(Wdt x_dbl[:R] + bias); state update, skip, gate
    float *ss = p.ssm_state + (int64_t)b * E * 16;
    IO *out = reinterpret_cast<IO *>(p.out) + (int64_t)b * E;
    for (int c = tid; c < E; c += kThreads) {
        const float *wd = p.dt_proj_weight + (int64_t)c * R;
        float dt = 0.f;
        for (int r = 0; r < R; ++r) dt = fmaf(wd[r], s_xdbl[r], dt);
        dt = cm_softplus(dt + (p.dt_bias ? p.dt_bias[c] : 0.f));
        const float x = s_x[c], dtx = dt * x;
        float y = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 h = *reinterpret_cast<const float4 *>(ss + 16 * c + 4 * q);
            const float4 a = *reinterpret_cast<const float4 *>(p.A + 16 * c + 4 * q);
            const float *Bm = s_xdbl + R + 4 * q, *Cm = s_xdbl + R + 16 + 4 * q;
            h.x = fmaf(cm_exp2(dt * a.x * CM_LOG2E), h.x, dtx * Bm[0]);
            h.y = fmaf(cm_exp2(dt * a.y * CM_LOG2E), h.y, dtx * Bm[1]);
            h.z = fmaf(cm_exp2(dt * a.z * CM_LOG2E), h.z, dtx * Bm[2]);
            h.w = fmaf(cm_exp2(dt * a.w * CM_LOG2E), h.w, dtx * Bm[3]);
            *reinterpret_cast<float4 *>(ss + 16 * c + 4 * q) = h;
            y = fmaf(h.x, Cm[0], y);
            y = fmaf(h.y, Cm[1], y);
            y = fmaf(h.z, Cm[2], y);
            y = fmaf(h.w, Cm[3], y);
        }
        if (p.D) y = fmaf(p.D[c], x, y);
        const float z = cm_elem<IO>::load(xz + E + c);
        cm_elem<IO>::store(out + c, y * (z * cm_sigmoid(z)));
    }
}

}  // namespace

extern "C" int cm_mamba_step(const cm_mamba_step_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "mamba_step: args is NULL");
    const cm_mamba_step_args &a = *args;
    CM_REQUIRE(a.batch > 0 && a.dim > 0 && a.dstate > 0 && a.dconv > 0 && a.dt_rank > 0, CM_EINVAL,
               "mamba_step: bad sizes batch=%d dim=%d dstate=%d dconv=%d dt_rank=%d", a.batch, a.dim, a.dstate, a.dconv, a.dt_rank);
    CM_REQUIRE(a.xz && a.conv_state && a.ssm_state && a.conv_weight && a.x_proj_weight && a.dt_proj_weight && a.A && a.out, CM_EINVAL,
               "mamba_step: NULL tensor");
    CM_REQUIRE(a.dstate == 16 && a.dconv == 4, CM_EUNSUPPORTED, "mamba_step: dstate %d / dconv %d unsupported (16 / 4 only)", a.dstate, a.dconv);
    CM_REQUIRE(a.dt_rank <= 32, CM_EUNSUPPORTED, "mamba_step: dt_rank %d unsupported (<= 32)", a.dt_rank);
    CM_REQUIRE(a.dim % 8 == 0 && a.dim <= kMaxDim, CM_EUNSUPPORTED, "mamba_step: dim %d unsupported (a multiple of 8, <= %d)", a.dim, kMaxDim);
    CM_REQUIRE(a.io_dtype == CM_F32 || a.io_dtype == CM_BF16, CM_EUNSUPPORTED, "mamba_step: unsupported dtype %d", a.io_dtype);
    CM_REQUIRE(cm_aligned(a.conv_state, 16) && cm_aligned(a.ssm_state, 16) && cm_aligned(a.conv_weight, 16) &&
               cm_aligned(a.x_proj_weight, 16) && cm_aligned(a.A, 16), CM_EALIGN, "mamba_step: fp32 tensors must be 16-byte aligned");
    hipStream_t st = reinterpret_cast<hipStream_t>(a.stream);
    if (a.io_dtype == CM_BF16) hipLaunchKernelGGL(mamba_step_kernel<cm_bf16>, dim3((unsigned)a.batch), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(mamba_step_kernel<float>, dim3((unsigned)a.batch), dim3(kThreads), 0, st, a);
    return cm_launch_status("cm_mamba_step");
}
