// conv_xproj.hip — both BiMamba directions' depthwise conv + SiLU AND their x_proj GEMMs in one pass over x
// (contract: cm_conv_xproj in include/conmamba_hip.h; reference bimamba.py:223-248 for the two convolutions,
// selective_scan_interface.py:182-186 for conv -> x_dbl = conv_out @ x_proj.weight^T).
//
// Separately this was conv_cl_kernel (read x, write u_fwd | u_bwd) followed by a library GEMM that read the 2E-wide u
// rows back to produce 96 numbers per row.  Here a workgroup owns 16 steps x all channels of one utterance:
//   phase 1: every thread convolves 4 channels x 8 steps from a 14-row register window (8-byte loads, 512 B per
//            wave-instruction), applies SiLU, stores u_fwd / u_bwd to HBM (the scan reads them) and keeps a bf16 copy
//            in LDS, token-major with a 32-byte row pad (conflict-free 16-byte fragment reads);
//   phase 2: wave w < 2 = direction multiplies the 16-token tile by that direction's x_proj weight
//            (48 x E: [dt rows zero-padded to 16 | B | C]) with v_mfma_f32_16x16x32_bf16, weights as the A operand
//            straight from their packed image in L2 (cm_ffn_pack_weights layout, 1 KB per fragment), so a lane ends
//            up with 4 consecutive features of one token = one 8-byte store into the x_dbl row.
// HBM traffic: x once (+ a 6-row halo per 16, served by the XCD's L2), u twice E per step written, 192 B of x_dbl per step.
//
// cm_conv_xproj_uni is the same kernel with the backward direction compiled out (the causal encoder's UniMamba mixer) and a
// history input: the three rows in front of the chunk come from x_hist instead of the zero padding, and the last three rows of
// [x_hist | x] leave as x_hist_out, so a stream of chunks convolves exactly like the whole sequence.
#include "cm_common.h"

#include <type_traits>


namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// steps per workgroup: TT (template), steps per thread TT / 2.  TT = 32 streams each x_proj weight fragment from L2 once per
// TWO token tiles (at TT = 16 the 96 KB of weights per workgroup are more L2 traffic than the kernel's HBM bytes) and reads
// 22 rows per 16 outputs instead of 14 per 8; its LDS tiles (67 KB) leave two workgroups per CU.
constexpr int W = 4;            // conv width
constexpr int PF = 8;           // weight-fragment ring depth

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

__device__ __forceinline__ uint32_t pack2(float a, float b) {         // one v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ float silu(float a) { return a * cm_sigmoid(a); }

// cm_debug_set(18): per-phase s_memtime stamps of one mid-grid workgroup (waves 0 and 3), read back with cm_debug_read_stamps_cx
__device__ unsigned long long g_cx_stamps[16];
__device__ __forceinline__ bool cm_ksplit_ok(int stamp) { return stamp != 2; }     // cm_debug_set(19): one wave per direction (A / B)
__device__ __forceinline__ unsigned long long cx_now() {
    unsigned long long t;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// the single-direction launch's arguments inside this file: cm_conv_xproj_args' fields (the backward ones unused) + the history rows
struct cx_uni_args : cm_conv_xproj_args {
    const void *x_hist;
    void *x_hist_out;
};
// ... and of its per-slot form (cm_conv_xproj_uni_slots): utterance b has lens[b] valid rows, clamped to [0, seqlen]
struct cx_slot_args : cx_uni_args {
    const int32_t *lens;
};
// the two-direction launch on whole utterances of different lengths (cm_conv_xproj_lens): utterance b has lens[b] rows, clamped to
// [0, seqlen]; every descriptor and the x_dbl store are cut behind its last row, tiles past it exit
struct cx_lens_args : cm_conv_xproj_args {
    const int32_t *lens;
};

// NB: 16-column bands of x_dbl per direction: 3 = [dt16 | B | C], 4 = [dt32 | B | C] (dt_rank 17..32: the S2S-large encoder)
template <int TT, int NB, typename P = cm_conv_xproj_args>
__global__ __launch_bounds__(256, (TT == 16 && NB == 3) ? 4 : 2) void conv_xproj_kernel(const P p, const int ntile, const int stamp_arg = 0) {
    constexpr bool UNI = std::is_base_of<cx_uni_args, P>::value;  // one direction, rows in front of the chunk from p.x_hist
    constexpr bool SLOT = std::is_same<P, cx_slot_args>::value;   // the new history is cut behind row lens[b] - 1, not behind row T - 1
    constexpr bool LENS = std::is_same<P, cx_lens_args>::value;   // T below is the utterance's own row count
    constexpr int HR = UNI ? 0 : W - 1;                           // rows behind a step that its outputs read
    constexpr int NR = (W - 1) + HR, NWIN = NR + 1;               // halo rows per run of steps; rows of the sliding window
#ifdef CM_ABLATE
    const int stamp = stamp_arg;
#else
    constexpr int stamp = 0;                                          // product build: no stamps, no A / B variant
#endif
    const bool st_wg = stamp == 1 && blockIdx.x == gridDim.x / 2 + 3;
    unsigned long long ts_[6] = {0, 0, 0, 0, 0, 0};
    if (st_wg) ts_[0] = cx_now();
    constexpr int TH = TT / 2;
    constexpr int NP = NB * 16;                                   // x_dbl columns per direction
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int E = p.dim;
    int T = p.seqlen;
    const int XS = E + 16;                                        // LDS row stride in bf16 elements
    uint16_t *ut[2] = {reinterpret_cast<uint16_t *>(smem), reinterpret_cast<uint16_t *>(smem) + TT * XS};
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // consecutive step tiles of an utterance share halo rows: keep them on one XCD (workgroup ids are dealt round-robin
    // to the 8 XCDs)
    const int total = gridDim.x;
    int id = blockIdx.x;
    if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
    const int b = id / ntile, t0 = (id % ntile) * TT;
    if constexpr (LENS) {
        T = min(max(p.lens[b], 0), T);
        if (t0 >= T) return;                                      // the whole workgroup: nothing to read or write (T == 0 forms no descriptor)
    }
    // buffer descriptors over this utterance's slices: rows outside [0, T) fall outside the buffer (reads return 0 = the
    // conv's zero padding, stores are dropped) and per-row addresses are an SGPR offset, so no per-access address math
    const int x_ts = (int)p.x_ts * 2, yf_ts = (int)p.yf_ts * 2, yb_ts = (int)p.yb_ts * 2;      // row strides in bytes
    auto rsrc = [&](const void *base, int64_t bs, int row_bytes) {
        const int64_t bytes = (int64_t)(T - 1) * row_bytes + (int64_t)E * 2;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(reinterpret_cast<const uint16_t *>(base) + (int64_t)b * bs), 0,
                                                 bytes > 0x7fffffff ? 0x7fffffff : (int)bytes, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t xr = rsrc(p.x, p.x_bs, x_ts), fr = rsrc(p.y_fwd, p.yf_bs, yf_ts), br = rsrc(UNI ? p.y_fwd : p.y_bwd, UNI ? p.yf_bs : p.yb_bs, UNI ? yf_ts : yb_ts);
    __amdgpu_buffer_rsrc_t hr = xr;                               // UNI: this utterance's (3, E) history rows; NULL = an empty buffer (zeros)
    if constexpr (UNI) {
        hr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t *>(reinterpret_cast<const uint16_t *>(p.x_hist) + (int64_t)b * (W - 1) * E), 0,
                                               p.x_hist ? (W - 1) * E * 2 : 0, 0x00020000);
        // the last W-1 rows of [x_hist | x], by the workgroup of the utterance's last tile (x_hist_out never aliases x_hist: checked at entry)
        // SLOT: of [x_hist | x[:lens[b]]], by the workgroup whose tile holds row lens[b] - 1 (tile 0 for an idle slot, which so carries
        // its history over into the spare buffer); rows at and past lens[b] are not read here
        int TL = T, writer = ntile - 1;
        if constexpr (SLOT) {
            TL = min(max(p.lens[b], 0), T);
            writer = TL > 0 ? (TL - 1) / TT : 0;
        }
        if (p.x_hist_out && id % ntile == writer) {
            uint16_t *ho = reinterpret_cast<uint16_t *>(p.x_hist_out) + (int64_t)b * (W - 1) * E;
            for (int idx = tid; idx < (W - 1) * (E / 4); idx += 256) {
                const int j = idx / (E / 4), c0 = (idx % (E / 4)) * 4, t = TL - (W - 1) + j;
                const u32x2 v = t >= 0 ? __builtin_amdgcn_raw_buffer_load_b64(xr, c0 * 2, t * x_ts, 0)
                                       : __builtin_amdgcn_raw_buffer_load_b64(hr, c0 * 2, (t + W - 1) * E * 2, 0);
                *reinterpret_cast<u32x2 *>(ho + j * E + c0) = v;
            }
        }
    }

    // ---- phase 2's operands, set up first: wave = (direction, K half); the 32-step build requests its weights now
    constexpr bool EARLY = TT == 32 || NB == 4;              // builds with a 256-VGPR budget
    constexpr int NTL = TT / 16;                                  // token tiles per workgroup
    const int l15 = lane & 15, lq = lane >> 4;
    const int nks = E / 32;
    const int dir = UNI ? 0 : wave & 1, kh = UNI ? wave : wave >> 1;          // UNI: waves 0 and 1 split K, waves 2 and 3 only convolve
    const bool ksplit = (nks & 1) == 0 && cm_ksplit_ok(stamp);
    const bool idle = UNI && kh >= 2;
    const int ks_lo = ksplit && !idle ? kh * (nks / 2) : 0, ks_hi = idle ? 0 : (ksplit ? ks_lo + nks / 2 : (kh == 0 ? nks : 0));
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void *>(dir ? p.wx_b : p.wx_f), 0, NP * E * 2, 0x00020000);
    const int vl = lane * 16;
    bf16x8 wq[PF][NB];
    auto wload = [&](int ks, bf16x8(&dst)[NB]) {                   // fragment (band mt, k-tile ks) = 1 KB at (mt*nks + ks)*1024
#pragma unroll
        for (int mt = 0; mt < NB; ++mt)
            dst[mt] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, vl, (mt * nks + ks) * 1024, 0));
    };
    bool wq_requested = !EARLY;

    // ---- phase 1: conv + SiLU, both directions.  thread = (4-channel group, half of the tile's steps)
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);
    const int ts = t0 + TH * half;                                // first step of this thread (wave-uniform)
    for (int cg = tid & 127; cg < E / 4; cg += 128) {
        const int c0 = cg * 4;
        u32x2 raw[TH + NR];                                       // rows ts-3 .. ts+TH+2 (UNI: .. ts+TH-1), all loads issued first
#pragma unroll
        for (int r = 0; r < TH + NR; ++r) {
            if constexpr (UNI) {
                const int row = ts - (W - 1) + r;                 // wave-uniform
                raw[r] = row < 0 ? __builtin_amdgcn_raw_buffer_load_b64(hr, c0 * 2, (row + W - 1) * E * 2, 0)
                                 : __builtin_amdgcn_raw_buffer_load_b64(xr, c0 * 2, row * x_ts, 0);
            } else {
                raw[r] = __builtin_amdgcn_raw_buffer_load_b64(xr, c0 * 2, (ts - (W - 1) + r) * x_ts, 0);
            }
        }
        if (!wq_requested) {                                      // behind the rows (HBM) in the in-order return queue: phase 1 waits
            wq_requested = true;                                  // for the rows only, the L2-resident weights land during it
#pragma unroll
            for (int s = 0; s < PF; ++s)
                if (ks_lo + s < ks_hi) wload(ks_lo + s, wq[s]);
        }
        if (st_wg) ts_[1] = cx_now();                             // rows have arrived
        // two channel PAIRS per thread: a staged dword is one pair, so taps, bias and SiLU run as v_pk_*_f32 on (lo, hi),
        // and every staged row is widened to fp32 once, when it enters the 7-row window (the scalar form widened each
        // element at each of its 8 uses: as many shifts as multiply-adds)
        f32x2 wf[2][W], wb[2][W], bf[2], bb[2];
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const float4 f0 = *reinterpret_cast<const float4 *>(p.weight_f + (c0 + 2 * pr) * W);
            const float4 f1 = *reinterpret_cast<const float4 *>(p.weight_f + (c0 + 2 * pr + 1) * W);
            const float4 g0 = UNI ? f0 : *reinterpret_cast<const float4 *>(p.weight_b + (c0 + 2 * pr) * W);
            const float4 g1 = UNI ? f1 : *reinterpret_cast<const float4 *>(p.weight_b + (c0 + 2 * pr + 1) * W);
            wf[pr][0] = f32x2{f0.x, f1.x}; wf[pr][1] = f32x2{f0.y, f1.y}; wf[pr][2] = f32x2{f0.z, f1.z}; wf[pr][3] = f32x2{f0.w, f1.w};
            wb[pr][0] = f32x2{g0.x, g1.x}; wb[pr][1] = f32x2{g0.y, g1.y}; wb[pr][2] = f32x2{g0.z, g1.z}; wb[pr][3] = f32x2{g0.w, g1.w};
            bf[pr] = p.bias_f ? f32x2{p.bias_f[c0 + 2 * pr], p.bias_f[c0 + 2 * pr + 1]} : f32x2{0.f, 0.f};
            bb[pr] = !UNI && p.bias_b ? f32x2{p.bias_b[c0 + 2 * pr], p.bias_b[c0 + 2 * pr + 1]} : f32x2{0.f, 0.f};
        }
        auto widen = [&](int r, int pr) -> f32x2 { return f32x2{cm_bf16_lo(raw[r][pr]), cm_bf16_hi(raw[r][pr])}; };
        auto silu2 = [](f32x2 a) -> f32x2 {                       // a / (1 + 2^(-a log2 e))
            const f32x2 e = a * f32x2{-CM_LOG2E, -CM_LOG2E};
            const f32x2 d = f32x2{cm_exp2(e.x), cm_exp2(e.y)} + f32x2{1.0f, 1.0f};
            return a * f32x2{cm_rcp(d.x), cm_rcp(d.y)};
        };
        f32x2 xw[NWIN][2];                                        // rows i .. i+6 (UNI: i+3) of the window, [row][pair]
#pragma unroll
        for (int r = 0; r < NR; ++r) { xw[r][0] = widen(r, 0); xw[r][1] = widen(r, 1); }
#pragma unroll
        for (int i = 0; i < TH; ++i) {
            xw[NR][0] = widen(i + NR, 0);
            xw[NR][1] = widen(i + NR, 1);
            u32x2 pf, pb;
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                f32x2 af = bf[pr], ab = bb[pr];
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    af = __builtin_elementwise_fma(wf[pr][k], xw[k][pr], af);                     // x[t-(W-1)+k]
                    if constexpr (!UNI) ab = __builtin_elementwise_fma(wb[pr][k], xw[NR - k][pr], ab);   // x[t+(W-1)-k]
                }
                const f32x2 of = silu2(af), ob = UNI ? of : silu2(ab);
                pf[pr] = pack2(of.x, of.y);
                pb[pr] = pack2(ob.x, ob.y);
            }
            const int tl = TH * half + i;
            *reinterpret_cast<u32x2 *>(ut[0] + tl * XS + c0) = pf;
            if constexpr (!UNI) *reinterpret_cast<u32x2 *>(ut[1] + tl * XS + c0) = pb;
            __builtin_amdgcn_raw_buffer_store_b64(pf, fr, c0 * 2, (ts + i) * yf_ts, 0);     // steps >= T: out of range, dropped
            if constexpr (!UNI) __builtin_amdgcn_raw_buffer_store_b64(pb, br, c0 * 2, (ts + i) * yb_ts, 0);
#pragma unroll
            for (int r = 0; r < NR; ++r) { xw[r][0] = xw[r + 1][0]; xw[r][1] = xw[r + 1][1]; }   // slide (register renaming)
        }
    }
    if (!wq_requested) {                                          // lanes without a channel group (dim < 512) skipped the loop
#pragma unroll
        for (int s = 0; s < PF; ++s)
            if (ks_lo + s < ks_hi) wload(ks_lo + s, wq[s]);
    }
    if (st_wg) {
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");      // phase 1 issued (stores still in flight)
        ts_[2] = t;
    }
    cm_lds_barrier();                                             // the u stores to HBM stay in flight under phase 2
    if (st_wg) {
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        ts_[3] = t;
        if (wave == 3 && lane == 0) { for (int i = 0; i < 4; ++i) g_cx_stamps[8 + i] = ts_[i]; }
    }

    // ---- phase 2: x_dbl[token][dir*48 + f] = sum_c W_dir[f][c] u_dir[token][c].  All four waves: wave = (direction, K half);
    // the halves meet through LDS (the token tiles are dead by then).  In-kernel stamps of the version with one wave per
    // direction: phase 1 9.8 k ticks, phase 2 10.7 k (96 MFMAs = 1.5 k of them: the rest was the wave waiting on its own
    // 48 KB weight stream from L2) -- so the weights of the 32-step build are requested BEFORE phase 1 (96 VGPRs held across
    // it, 232 in all) and phase 2 is MFMAs and fragment reads only.
    // an OFFSET into the shared array, not ut[dir]: indexing the pointer array with a run-time value loses the LDS address space, the
    // fragment reads became flat_load + s_waitcnt vmcnt(0) lgkmcnt(0) and every k-step drained the weight ring it was meant to overlap
    const uint16_t *frag = reinterpret_cast<const uint16_t *>(smem) + dir * (TT * XS) + l15 * XS + lq * 8;
    f32x4 acc[NTL][NB];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
        for (int mt = 0; mt < NB; ++mt) acc[nt][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!EARLY) {
#pragma unroll
        for (int s = 0; s < PF; ++s) wload(ks_lo + s, wq[s]);     // past-the-end fragments read as zeros (buffer bounds)
    }
    for (int ks0 = ks_lo; ks0 < ks_hi; ks0 += PF) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            const int ks = ks0 + s;
            if (ks < ks_hi) {
#pragma unroll
                for (int nt = 0; nt < NTL; ++nt) {
                    const bf16x8 tok = *reinterpret_cast<const bf16x8 *>(frag + nt * 16 * XS + ks * 32);
#pragma unroll
                    for (int mt = 0; mt < NB; ++mt)
                        acc[nt][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[s][mt], tok, acc[nt][mt], 0, 0, 0);
                }
                if (ks + PF < ks_hi) wload(ks + PF, wq[s]);
            }
        }
    }
    if (st_wg) {
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");      // MFMA loop issued
        ts_[4] = t;
    }
    if (ksplit) {
        cm_lds_barrier();                                         // every wave is done with the token tiles
        float *xch = reinterpret_cast<float *>(smem) + (dir * 64 + lane) * (NTL * NB * 4);
        if (kh == 1) {
#pragma unroll
            for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
                for (int mt = 0; mt < NB; ++mt) *reinterpret_cast<f32x4 *>(xch + (nt * NB + mt) * 4) = acc[nt][mt];
        }
        cm_lds_barrier();
        if (UNI ? kh != 0 : kh == 1) return;
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int mt = 0; mt < NB; ++mt) acc[nt][mt] += *reinterpret_cast<const f32x4 *>(xch + (nt * NB + mt) * 4);
    } else if (UNI ? kh != 0 : kh == 1) {
        return;
    }
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        const int t = t0 + 16 * nt + l15;
        if (t < T) {
            uint16_t *xo = reinterpret_cast<uint16_t *>(p.xdbl) + (int64_t)b * p.xdbl_bs + (int64_t)t * p.xdbl_ts + dir * NP + lq * 4;
#pragma unroll
            for (int mt = 0; mt < NB; ++mt)
                *reinterpret_cast<uint2 *>(xo + mt * 16) = uint2{pack2(acc[nt][mt][0], acc[nt][mt][1]), pack2(acc[nt][mt][2], acc[nt][mt][3])};
        }
    }
    if (st_wg && wave == 0) {
        ts_[5] = cx_now();                                        // everything of this wave has landed
        if (lane == 0) { for (int i = 0; i < 6; ++i) g_cx_stamps[i] = ts_[i]; }
    }
}

template <int TT, int NB, typename P>
int launch_cx(const P &a) {
    constexpr int ND = std::is_base_of<cx_uni_args, P>::value ? 1 : 2;
    // the token tiles, and at least the K halves' exchange area that overlays them (64 lanes x TT / 16 x NB accumulators per direction)
    const size_t tiles = (size_t)ND * TT * (a.dim + 16) * sizeof(uint16_t), xch = (size_t)ND * 64 * (TT / 16) * NB * 16;
    const size_t smem = tiles > xch ? tiles : xch;
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_xproj_kernel<TT, NB, P>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) {
            cm_set_error("conv_xproj: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
            return (int)e;
        }
        attr_done = true;
    }
    const int ntile = (a.seqlen + TT - 1) / TT;
    CM_REQUIRE((long)ntile * a.batch < (1L << 31), CM_EINVAL, "conv_xproj: grid too large");
    hipLaunchKernelGGL((conv_xproj_kernel<TT, NB, P>), dim3((unsigned)(ntile * a.batch)), dim3(256), smem, reinterpret_cast<hipStream_t>(a.stream), a, ntile, cm_debug_get() == 18 ? 1 : (cm_debug_get() == 19 ? 2 : 0));
    return cm_launch_status(std::is_same<P, cx_slot_args>::value ? "cm_conv_xproj_uni_slots" : ND == 1 ? "cm_conv_xproj_uni"
                            : std::is_same<P, cx_lens_args>::value ? "cm_conv_xproj_lens" : "cm_conv_xproj");
}

}  // namespace

#ifdef CM_ABLATE
extern "C" int cm_debug_read_stamps_cx(unsigned long long *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cx_stamps), sizeof(unsigned long long) * 16);
}
#endif

// cm_conv_xproj (lens == NULL) and cm_conv_xproj_lens: one set of checks, one choice of tile shape
static int conv_xproj_entry(const cm_conv_xproj_args &a, const int32_t *lens) {
    CM_REQUIRE(a.batch > 0 && a.seqlen > 0 && a.dim > 0 && a.x && a.weight_f && a.weight_b && a.wx_f && a.wx_b && a.y_fwd &&
                   a.y_bwd && a.xdbl, CM_EINVAL, "conv_xproj: bad sizes or NULL tensor");
    CM_REQUIRE(a.width == W, CM_EUNSUPPORTED, "conv_xproj: conv width %d unsupported (4 only)", a.width);
    CM_REQUIRE(a.dim % 32 == 0 && a.dim <= 2048, CM_EUNSUPPORTED, "conv_xproj: dim %d must be a multiple of 32, at most 2048", a.dim);
    CM_REQUIRE(cm_aligned(a.x, 8) && cm_aligned(a.y_fwd, 8) && cm_aligned(a.y_bwd, 8) && cm_aligned(a.xdbl, 8) &&
                   cm_aligned(a.weight_f, 16) && cm_aligned(a.weight_b, 16) && cm_aligned(a.wx_f, 16) && cm_aligned(a.wx_b, 16) &&
                   a.x_bs % 4 == 0 && a.x_ts % 4 == 0 && a.yf_bs % 4 == 0 && a.yf_ts % 4 == 0 && a.yb_bs % 4 == 0 &&
                   a.yb_ts % 4 == 0 && a.xdbl_bs % 4 == 0 && a.xdbl_ts % 4 == 0,
               CM_EALIGN, "conv_xproj: tensors must be 8-byte aligned (weights 16) with strides that are multiples of 4 elements");
    // 32-step tiles when the LDS tiles fit twice per CU and the sequence is long enough to fill the chip with them
    const bool wide = a.variant != 1 && (size_t)2 * 32 * (a.dim + 16) * 2 <= 72 * 1024 && (long)a.batch * ((a.seqlen + 31) / 32) >= 512;
    CM_REQUIRE(a.dt_pad == 0 || a.dt_pad == 16 || a.dt_pad == 32, CM_EUNSUPPORTED, "conv_xproj: dt_pad %d (16 or 32)", a.dt_pad);
    if (a.dt_pad == 32)
        CM_REQUIRE((size_t)2 * 16 * (a.dim + 16) * 2 <= 80 * 1024, CM_EUNSUPPORTED, "conv_xproj: dim %d too wide for 64-column rows", a.dim);
    if (lens) {
        cx_lens_args s{};
        static_cast<cm_conv_xproj_args &>(s) = a;
        s.lens = lens;
        if (a.dt_pad == 32) return wide ? launch_cx<32, 4>(s) : launch_cx<16, 4>(s);
        return wide ? launch_cx<32, 3>(s) : launch_cx<16, 3>(s);
    }
    if (a.dt_pad == 32) return wide ? launch_cx<32, 4>(a) : launch_cx<16, 4>(a);
    return wide ? launch_cx<32, 3>(a) : launch_cx<16, 3>(a);
}

extern "C" int cm_conv_xproj(const cm_conv_xproj_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "conv_xproj: args is NULL");
    return conv_xproj_entry(*args, nullptr);
}

extern "C" int cm_conv_xproj_lens(const cm_conv_xproj_args *args, const int32_t *lens) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "conv_xproj_lens: args is NULL");
    CM_REQUIRE(lens != nullptr, CM_EINVAL, "conv_xproj_lens: lens is NULL (cm_conv_xproj is the form without lengths)");
    CM_REQUIRE(cm_aligned(lens, 4), CM_EALIGN, "conv_xproj_lens: lens must be 4-byte aligned");
    return conv_xproj_entry(*args, lens);
}

// cm_conv_xproj_uni (lens == NULL) and cm_conv_xproj_uni_slots: one set of checks, one choice of tile shape
static int conv_xproj_uni_entry(const cm_conv_xproj_uni_args &u, const int32_t *lens) {
    CM_REQUIRE(u.batch > 0 && u.seqlen > 0 && u.dim > 0 && u.x && u.weight && u.wx && u.y && u.xdbl, CM_EINVAL,
               "conv_xproj_uni: bad sizes or NULL tensor");
    CM_REQUIRE(u.width == W, CM_EUNSUPPORTED, "conv_xproj_uni: conv width %d unsupported (4 only)", u.width);
    CM_REQUIRE(u.dim % 32 == 0 && u.dim <= 2048, CM_EUNSUPPORTED, "conv_xproj_uni: dim %d must be a multiple of 32, at most 2048", u.dim);
    CM_REQUIRE(cm_aligned(u.x, 8) && cm_aligned(u.y, 8) && cm_aligned(u.xdbl, 8) && cm_aligned(u.weight, 16) && cm_aligned(u.wx, 16) &&
                   (!u.x_hist || cm_aligned(u.x_hist, 8)) && (!u.x_hist_out || cm_aligned(u.x_hist_out, 8)) && u.x_bs % 4 == 0 &&
                   u.x_ts % 4 == 0 && u.y_bs % 4 == 0 && u.y_ts % 4 == 0 && u.xdbl_bs % 4 == 0 && u.xdbl_ts % 4 == 0,
               CM_EALIGN, "conv_xproj_uni: tensors must be 8-byte aligned (weights 16) with strides that are multiples of 4 elements");
    CM_REQUIRE(u.dt_pad == 0 || u.dt_pad == 16 || u.dt_pad == 32, CM_EUNSUPPORTED, "conv_xproj_uni: dt_pad %d (16 or 32)", u.dt_pad);
    if (u.x_hist && u.x_hist_out) {                               // other workgroups of the launch still read x_hist when the last one writes
        const char *hi = reinterpret_cast<const char *>(u.x_hist), *ho = reinterpret_cast<const char *>(u.x_hist_out);
        const int64_t bytes = (int64_t)u.batch * (W - 1) * u.dim * 2;
        CM_REQUIRE(ho + bytes <= hi || hi + bytes <= ho, CM_EINVAL, "conv_xproj_uni: x_hist_out must not overlap x_hist");
    }
    cx_uni_args a{};
    a.batch = u.batch, a.seqlen = u.seqlen, a.dim = u.dim, a.width = u.width;
    a.x = u.x, a.weight_f = u.weight, a.bias_f = u.bias, a.wx_f = u.wx, a.y_fwd = u.y, a.xdbl = u.xdbl;
    a.x_bs = u.x_bs, a.x_ts = u.x_ts, a.yf_bs = u.y_bs, a.yf_ts = u.y_ts, a.xdbl_bs = u.xdbl_bs, a.xdbl_ts = u.xdbl_ts;
    a.stream = u.stream, a.dt_pad = u.dt_pad, a.variant = u.variant;
    a.x_hist = u.x_hist, a.x_hist_out = u.x_hist_out;
    // tile shape by cm_conv_xproj's rule, on one direction's LDS tile
    const bool wide = a.variant != 1 && (size_t)32 * (a.dim + 16) * 2 <= 36 * 1024 && (long)a.batch * ((a.seqlen + 31) / 32) >= 512;
    if (lens) {
        cx_slot_args s{};
        static_cast<cx_uni_args &>(s) = a;
        s.lens = lens;
        if (a.dt_pad == 32) return wide ? launch_cx<32, 4>(s) : launch_cx<16, 4>(s);
        return wide ? launch_cx<32, 3>(s) : launch_cx<16, 3>(s);
    }
    if (a.dt_pad == 32) return wide ? launch_cx<32, 4>(a) : launch_cx<16, 4>(a);
    return wide ? launch_cx<32, 3>(a) : launch_cx<16, 3>(a);
}

extern "C" int cm_conv_xproj_uni(const cm_conv_xproj_uni_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "conv_xproj_uni: args is NULL");
    return conv_xproj_uni_entry(*args, nullptr);
}

extern "C" int cm_conv_xproj_uni_slots(const cm_conv_xproj_uni_args *args, const int32_t *lens) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "conv_xproj_uni_slots: args is NULL");
    CM_REQUIRE(lens != nullptr, CM_EINVAL, "conv_xproj_uni_slots: lens is NULL (cm_conv_xproj_uni is the lock-step form)");
    CM_REQUIRE(cm_aligned(lens, 4), CM_EALIGN, "conv_xproj_uni_slots: lens must be 4-byte aligned");
    return conv_xproj_uni_entry(*args, lens);
}
