// fused_d144.hip — cm_ffn_fused and cm_ln_pw_glu at d_model = 144 (the ConMamba-small recipes): sibling kernels of ffn_fused.hip and
// ln_pw_glu.hip, which stay as they are for d_model 256.  Inference forward, bf16, weights in the 16-row x 32-column fragment image
// (cm_ffn_pack_weights), v_mfma_f32_16x16x32_bf16 with the weights as the A operand and tokens as the B operand, 64 tokens per
// workgroup, four waves, the hidden slab in LDS -- as there.  What the width changes:
//   * K = 144 is 4.5 k-tiles of 32: the token tile in LDS and the images of W1 (hidden, 144), proj_w (P, 144) and the pointwise weight
//     (288, 144) are padded to KP = 160 columns.  The weight pads are zeros (ops.PackedWeight(pad=...)); the kernel writes the token
//     tile's columns 144 .. 159 as zeros itself, every time it fills the tile (0 x uninitialised LDS may be NaN).
//   * the output width is 9 feature tiles of 16.  GEMM 1 keeps "wave = 64 hidden units x 64 tokens"; for GEMM 2 and the epilogue a wave
//     owns a token half x a feature half: 32 tokens x 5 feature tiles, features 80 fh + 16 mb + 4 lq + j.  Tile 4 of the upper half is
//     features 144 .. 159: W2's image is padded to 160 rows with zeros, and that tile is never stored, never enters a LayerNorm sum
//     and stays exactly zero in registers (it is what zeroes the pad columns of the projection's token tile).
//   * LayerNorm statistics are over the 144 real features: phase 0 sums 36 float4 pieces per token over a row of 16 lanes (pieces
//     32 .. 35 in lanes 0 .. 3, the rest of the third round is zero and masked out of the variance); the epilogue sums a lane's valid
//     tiles, the four lane groups, and the two feature halves through LDS.
//   * the projection epilogue takes proj_dim as a multiple of 64 (576 = 2 d_inner of the recipe): a wave owns proj_dim / 4 output
//     features, three 16-row bands at a time.
// The weight stream is double-buffered per GEMM (W1: 4 fragments x 2, W2: 5 fragments x 2); the first two steps of the next GEMM are
// requested while the current one runs.
#include "cm_common.h"
#include "ffn_tile.h"
#include <type_traits>


namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int D = 144;        // d_model
constexpr int KP = 160;       // K padded to whole k-tiles
constexpr int KT = KP / 32;   // k-tiles
constexpr int C4 = D / 4;     // float4 pieces per row
constexpr int TOK = 64;       // tokens per workgroup
constexpr int NT = 256;       // threads per workgroup
constexpr int XS = 264;       // cm_ffn_fused: LDS row stride in bf16 elements (528 bytes), token tile and hidden slab
constexpr int XG = 168;       // cm_ln_pw_glu: LDS row stride of the token tile (336 bytes: 8 rows' 16-byte pieces cover all banks)
constexpr int CH = 256;       // hidden slab
constexpr int SR = 148;       // floats per staged fp32 row (592 bytes)
static_assert(TOK * SR * 4 <= 2 * TOK * XS * 2, "the fp32 staging rows overlay the two bf16 tiles");

// Phase 0's LayerNorm.  v[rd][i] = float4 piece l15 + 16 i of token 4 rd + lq of the wave's 16 (a row of 16 lanes holds one token);
// piece 32 + l15 exists for l15 < 4 only and holds zeros elsewhere.  Returns the normalised rows in bf16, pad pieces as zeros.
__device__ __forceinline__ void ln_rows144(float4 (&v)[4][3], const float *g_, const float *b_, float eps, int l15, uint2 (&pk)[4][3]) {
    const bool real2 = l15 < C4 - 32;
#pragma unroll
    for (int rd = 0; rd < 4; ++rd) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) s += (v[rd][i].x + v[rd][i].y) + (v[rd][i].z + v[rd][i].w);
        const float mean = group_sum16_fenced(s) * (1.f / D);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float m = (i < 2 || real2) ? mean : 0.f;         // the pad pieces stay zero: they are not part of the variance
            v[rd][i].x -= m; v[rd][i].y -= m; v[rd][i].z -= m; v[rd][i].w -= m;
            q = fmaf(v[rd][i].x, v[rd][i].x, fmaf(v[rd][i].y, v[rd][i].y, fmaf(v[rd][i].z, v[rd][i].z, fmaf(v[rd][i].w, v[rd][i].w, q))));
        }
        const float rstd = rsqrtf(group_sum16_fenced(q) * (1.f / D) + eps);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int col = (l15 + 16 * i) * 4;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f), b = g;
            if (i < 2 || real2) {
                g = *reinterpret_cast<const float4 *>(g_ + col);
                b = *reinterpret_cast<const float4 *>(b_ + col);
            }
            pk[rd][i].x = pack2(fmaf(v[rd][i].x * rstd, g.x, b.x), fmaf(v[rd][i].y * rstd, g.y, b.y));
            pk[rd][i].y = pack2(fmaf(v[rd][i].z * rstd, g.z, b.z), fmaf(v[rd][i].w * rstd, g.w, b.w));
        }
    }
}

// the normalised rows into a token tile of row stride `xs`: columns 0 .. 159, the pad columns 144 .. 159 as the zeros ln_rows144 made
__device__ __forceinline__ void store_rows144(uint16_t *tile, int xs, int row0, int l15, int lq, const uint2 (&pk)[4][3]) {
#pragma unroll
    for (int rd = 0; rd < 4; ++rd)
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < 2 || l15 < KP / 4 - 32) *reinterpret_cast<uint2 *>(tile + (row0 + rd * 4 + lq) * xs + (l15 + 16 * i) * 4) = pk[rd][i];
}

// ---------------------------------------------------------------------------------------------------------------- cm_ffn_fused
// PROJ: the projection epilogue (proj_out = LN2(r) @ proj_w^T (+ proj_b), h is not stored).  RACC: the residual rows are fetched once
// and start the second GEMM's accumulators as xin / alpha (alpha a power of two); false: they are loaded again behind the last GEMM.
template <bool ADD, bool PROJ, bool RACC>
__global__ __launch_bounds__(NT, 2) void ffn144_kernel(const cm_ffn_args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t *xn = reinterpret_cast<uint16_t *>(smem);            // [TOK][XS] normalised tokens, columns 0 .. 159
    uint16_t *hc = xn + TOK * XS;                                 // [TOK][XS] hidden slab
    float *red = reinterpret_cast<float *>(hc + TOK * XS);        // [2][TOK] LayerNorm partial sums of the two feature halves
    float *b1s = red + 2 * TOK;                                   // [hidden] first bias
    float *stg = reinterpret_cast<float *>(smem);                 // [TOK][SR] fp32 rows, over both tiles while they are dead
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);    // phase 0: tokens 16 wave ..; GEMM 1: hidden units 64 wave ..
    const int fh = wave & 1, th2 = wave >> 1;                     // GEMM 2 / epilogue: feature half, token half
    const int nmb = fh ? 4 : 5;                                   // real feature tiles of this half (tile 4 of the upper half is the pad)
    const int l15 = lane & 15, lq = lane >> 4;
    const int t0 = blockIdx.x * TOK, M = p.rows, F = p.hidden;
    const int nch = F / CH;
    const uint16_t *addend = reinterpret_cast<const uint16_t *>(p.addend);

    // ---- weight stream: W1's image is (hidden, 160): band (c CH + 64 wave) / 16 + mb, k-tile s; W2's image is (160, hidden): band
    // 5 fh + mb, k-tile 8 c + j.  One buffer load = the 1 KB image of one MFMA operand fragment.
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w1), 0, F * KP * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w2), 0, KP * F * 2, 0x00020000);
    const int vl = lane * 16;
    const int kt2 = F / 32;
    auto w1load = [&](int c, int s, bf16x8(&dst)[4]) {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
            dst[mb] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r1, vl, (((c * CH + wave * 64) / 16 + mb) * KT + s) * 1024, 0));
    };
    auto w2load = [&](int c, int j, bf16x8(&dst)[5]) {
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
            dst[mb] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r2, vl, ((fh * 5 + mb) * kt2 + c * (CH / 32) + j) * 1024, 0));
    };
    bf16x8 wa[4], wb[4], wc[5], we[5];                            // W1 / proj_w steps (even, odd), W2 steps (even, odd)
    w1load(0, 0, wa);
    w1load(0, 1, wb);

    float4 b1r[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i4 = (tid + NT * k) * 4;
        b1r[k] = i4 < F ? *reinterpret_cast<const float4 *>(p.b1 + i4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    f32x4 acc2[5][2];
    const int f0 = fh * 80 + lq * 4;

    // ---- phase 0: xin = x (+ add_scale * addend); xn = LayerNorm_pre(xin) in bf16
    auto load_x4 = [&](int tok, int col) {
        float4 v = *reinterpret_cast<const float4 *>(p.x + (int64_t)tok * D + col);
        if constexpr (ADD) {
            const uint2 a = *reinterpret_cast<const uint2 *>(addend + (int64_t)tok * D + col);
            v.x = fmaf(p.add_scale, cm_bf16_lo(a.x), v.x);
            v.y = fmaf(p.add_scale, cm_bf16_hi(a.x), v.y);
            v.z = fmaf(p.add_scale, cm_bf16_lo(a.y), v.z);
            v.w = fmaf(p.add_scale, cm_bf16_hi(a.y), v.w);
        }
        return v;
    };
    {
        float4 v[4][3];
#pragma unroll
        for (int rd = 0; rd < 4; ++rd) {
            const int tok = min(t0 + wave * 16 + rd * 4 + lq, M - 1);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                v[rd][i] = (i < 2 || l15 < C4 - 32) ? load_x4(tok, (l15 + 16 * i) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {                             // loads return in order: this waits for the bias, not for the rows
            const int i4 = (tid + NT * k) * 4;
            if (i4 < F) *reinterpret_cast<float4 *>(b1s + i4) = b1r[k];
        }
        if constexpr (RACC) {                                     // xin, whole rows, over the two token tiles (both still free)
#pragma unroll
            for (int rd = 0; rd < 4; ++rd)
#pragma unroll
                for (int i = 0; i < 3; ++i)
                    if (i < 2 || l15 < C4 - 32)
                        *reinterpret_cast<float4 *>(stg + (wave * 16 + rd * 4 + lq) * SR + (l15 + 16 * i) * 4) = v[rd][i];
        }
        uint2 pk0[4][3];
        ln_rows144(v, p.pre_g, p.pre_b, p.pre_eps, l15, pk0);
        if constexpr (RACC) {
            // into the accumulator layout (lane = token 32 th2 + 16 nb + l15, features 80 fh + 16 mb + 4 lq + j), scaled by 1 / alpha
            lds_barrier();
            const float inva = 1.f / p.alpha;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int mb = 0; mb < 5; ++mb) {
                    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (mb < nmb) xv = *reinterpret_cast<const float4 *>(stg + (th2 * 32 + nb * 16 + l15) * SR + f0 + mb * 16);
                    acc2[mb][nb] = f32x4{xv.x * inva, xv.y * inva, xv.z * inva, xv.w * inva};
                }
            lds_barrier();                                        // every wave has its residual: the tile becomes xn
        }
        store_rows144(xn, XS, wave * 16, l15, lq, pk0);
    }
    lds_barrier();
    w2load(0, 0, wc);                                             // (requested here: beside phase 0's rows they would spill)
    w2load(0, 1, we);

    if constexpr (!RACC) {
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc2[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const uint16_t *xfrag = xn + l15 * XS + lq * 8;                       // GEMM 1 / projection: all 64 tokens
    const uint16_t *hfrag = hc + (th2 * 32 + l15) * XS + lq * 8;          // GEMM 2: this wave's token half
    uint16_t *hdst = hc + l15 * XS + wave * 64 + lq * 4;

    auto read_frags4 = [&](int ks, bf16x8(&bf)[4]) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) bf[nb] = *reinterpret_cast<const bf16x8 *>(xfrag + nb * 16 * XS + ks * 32);
    };
    auto read_frags2 = [&](int ks, bf16x8(&bf)[2]) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) bf[nb] = *reinterpret_cast<const bf16x8 *>(hfrag + nb * 16 * XS + ks * 32);
    };
    // one hidden slab; the last one is peeled (LAST): it does not request the next slab's weights
    auto slab = [&](const int c, auto last_tag) {
        constexpr bool LAST = decltype(last_tag)::value;
        f32x4 acc1[4][4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) acc1[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        // GEMM 1: this wave's 64 hidden units x 64 tokens, K = 160
        {
            bf16x8 bfa[4], bfb[4];
            read_frags4(0, bfa);
#pragma unroll
            for (int s = 0; s < KT; ++s) {
                bf16x8(&cur)[4] = (s & 1) ? bfb : bfa;
                bf16x8(&nxt)[4] = (s & 1) ? bfa : bfb;
                bf16x8(&w)[4] = (s & 1) ? wb : wa;
                if (s + 1 < KT) read_frags4(s + 1, nxt);
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) acc1[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[mb], cur[nb], acc1[mb][nb], 0, 0, 0);
                if (s + 2 < KT) w1load(c, s + 2, w);
                __builtin_amdgcn_sched_barrier(0);                // keep the refill here (see cm_ffn_fused at 256)
            }
        }
        // bias + GELU -> bf16 slab in LDS (token-major, hidden contiguous)
        if (c > 0) lds_barrier();                                 // every wave is done reading the previous slab
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) {
            const float4 bv = *reinterpret_cast<const float4 *>(b1s + c * CH + wave * 64 + mb * 16 + lq * 4);
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                uint2 pk;
                pk.x = cm_gelu_bf16_pack2(acc1[mb][nb][0] + bv.x, acc1[mb][nb][1] + bv.y);
                pk.y = cm_gelu_bf16_pack2(acc1[mb][nb][2] + bv.z, acc1[mb][nb][3] + bv.w);
                *reinterpret_cast<uint2 *>(hdst + nb * 16 * XS + mb * 16) = pk;
            }
        }
        if constexpr (!LAST) {                                    // the next slab's first W1 steps travel under GEMM 2
            w1load(c + 1, 0, wa);
            w1load(c + 1, 1, wb);
            __builtin_amdgcn_sched_barrier(0);
        }
        lds_barrier();
        // GEMM 2: this wave's 80 output features x 32 tokens, K = this slab
        {
            bf16x8 bfa[2], bfb[2];
            read_frags2(0, bfa);
#pragma unroll
            for (int j = 0; j < CH / 32; ++j) {
                bf16x8(&cur)[2] = (j & 1) ? bfb : bfa;
                bf16x8(&nxt)[2] = (j & 1) ? bfa : bfb;
                bf16x8(&w)[5] = (j & 1) ? we : wc;
                if (j + 1 < CH / 32) read_frags2(j + 1, nxt);
#pragma unroll
                for (int mb = 0; mb < 5; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) acc2[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[mb], cur[nb], acc2[mb][nb], 0, 0, 0);
                if (j + 2 < CH / 32) w2load(c, j + 2, w);
                else if constexpr (!LAST) w2load(c + 1, j + 2 - CH / 32, w);     // the next slab's first W2 steps
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    for (int c = 0; c + 1 < nch; ++c) slab(c, std::false_type{});
    slab(nch - 1, std::true_type{});

    // ---- epilogue: r = xin + alpha (acc2 + b2); optional LN1 -> stream; optional LN2 -> h_out / the projection.
    // Lane holds token 32 th2 + 16 nb + l15, features 80 fh + 16 mb + 4 lq + j; tiles mb >= nmb are the pad and stay zero.
    float r[2][5][4];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int j = 0; j < 4; ++j) r[nb][mb][j] = 0.f;
    if constexpr (!RACC) {
        // the residual rows again, as whole rows (36 float4 pieces each), through LDS into the accumulator layout
        constexpr int NP = TOK * C4 / NT;                         // 9 pieces per thread
        float4 rows_[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + NT * i;
            rows_[i] = load_x4(min(t0 + idx / C4, M - 1), (idx % C4) * 4);
        }
        lds_barrier();                                            // every wave is done with the last GEMM's fragments
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int idx = tid + NT * i;
            *reinterpret_cast<float4 *>(stg + (idx / C4) * SR + (idx % C4) * 4) = rows_[i];
        }
        lds_barrier();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
                if (mb < nmb) {
                    const float4 xv = *reinterpret_cast<const float4 *>(stg + (th2 * 32 + nb * 16 + l15) * SR + f0 + mb * 16);
                    const float4 bv = *reinterpret_cast<const float4 *>(p.b2 + f0 + mb * 16);
                    r[nb][mb][0] = fmaf(p.alpha, acc2[mb][nb][0] + bv.x, xv.x);
                    r[nb][mb][1] = fmaf(p.alpha, acc2[mb][nb][1] + bv.y, xv.y);
                    r[nb][mb][2] = fmaf(p.alpha, acc2[mb][nb][2] + bv.z, xv.z);
                    r[nb][mb][3] = fmaf(p.alpha, acc2[mb][nb][3] + bv.w, xv.w);
                }
    } else {
        // the residual rode in the accumulators: r = alpha (xin / alpha + W2 g + b2)
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
            if (mb < nmb) {
                const float4 bv = *reinterpret_cast<const float4 *>(p.b2 + f0 + mb * 16);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    r[nb][mb][0] = p.alpha * (acc2[mb][nb][0] + bv.x);
                    r[nb][mb][1] = p.alpha * (acc2[mb][nb][1] + bv.y);
                    r[nb][mb][2] = p.alpha * (acc2[mb][nb][2] + bv.z);
                    r[nb][mb][3] = p.alpha * (acc2[mb][nb][3] + bv.w);
                }
            }
    }
    // sum over a token's 144 features: the lane's real tiles, 4 lane groups, 2 feature halves (through LDS)
    auto token_sums = [&](float (&v)[2]) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            v[nb] += __shfl_xor(v[nb], 16, 64);
            v[nb] += __shfl_xor(v[nb], 32, 64);
        }
        lds_barrier();                                            // previous use of red is over
        if (lq == 0) {
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) red[fh * TOK + th2 * 32 + nb * 16 + l15] = v[nb];
        }
        lds_barrier();
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int t = th2 * 32 + nb * 16 + l15;
            v[nb] = red[t] + red[TOK + t];
        }
    };
    auto layer_norm = [&](const float *g, const float *b, float eps) {
        float s[2], q[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            s[nb] = 0.f;
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
                if (mb < nmb) s[nb] += (r[nb][mb][0] + r[nb][mb][1]) + (r[nb][mb][2] + r[nb][mb][3]);
        }
        token_sums(s);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            s[nb] *= (1.f / D);
            q[nb] = 0.f;
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
                if (mb < nmb) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float d = r[nb][mb][j] - s[nb]; q[nb] = fmaf(d, d, q[nb]); }
                }
        }
        token_sums(q);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) q[nb] = rsqrtf(q[nb] * (1.f / D) + eps);
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
            if (mb < nmb) {
                const float4 gv = *reinterpret_cast<const float4 *>(g + f0 + mb * 16);
                const float4 bv = *reinterpret_cast<const float4 *>(b + f0 + mb * 16);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    r[nb][mb][0] = fmaf((r[nb][mb][0] - s[nb]) * q[nb], gv.x, bv.x);
                    r[nb][mb][1] = fmaf((r[nb][mb][1] - s[nb]) * q[nb], gv.y, bv.y);
                    r[nb][mb][2] = fmaf((r[nb][mb][2] - s[nb]) * q[nb], gv.z, bv.z);
                    r[nb][mb][3] = fmaf((r[nb][mb][3] - s[nb]) * q[nb], gv.w, bv.w);
                }
            }
    };
    if (p.n1_g) layer_norm(p.n1_g, p.n1_b, p.n1_eps);
    if (p.x_out) {
        // the stream rows leave through LDS (both tiles are dead) as whole 576-byte rows
        lds_barrier();                                            // every wave is done with the last GEMM's fragments / the staged rows
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 5; ++mb)
                if (mb < nmb)
                    *reinterpret_cast<float4 *>(stg + (th2 * 32 + nb * 16 + l15) * SR + f0 + mb * 16) =
                        make_float4(r[nb][mb][0], r[nb][mb][1], r[nb][mb][2], r[nb][mb][3]);
        lds_barrier();
#pragma unroll
        for (int i = 0; i < TOK * C4 / NT; ++i) {
            const int idx = tid + NT * i, row = idx / C4, chunk = idx % C4;
            const float4 v = *reinterpret_cast<const float4 *>(stg + row * SR + chunk * 4);
            if (t0 + row < M) *reinterpret_cast<float4 *>(p.x_out + (int64_t)(t0 + row) * D + chunk * 4) = v;
        }
    }
    if constexpr (PROJ) {
        // ---- projection epilogue.  h = LN2(r) goes to the token tile in bf16 (its pad columns from the pad tile's zeros); a wave then
        // owns proj_dim / 4 output features = nb4 16-row bands of proj_w's (proj_dim, 160) image, three bands x 64 tokens at a time.
        const int nb4 = p.proj_dim / 64, pd4 = nb4 * 16, ncq = (nb4 + 2) / 3;
        const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.proj_w), 0, p.proj_dim * KP * 2, 0x00020000);
        auto pload = [&](int cq, int s, bf16x8(&dst)[4]) {       // bands past the wave's own (clamped to the image's last) are loaded and dropped
#pragma unroll
            for (int mb = 0; mb < 3; ++mb)
                dst[mb] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rp, vl, (min(wave * nb4 + cq * 3 + mb, 4 * nb4 - 1) * KT + s) * 1024, 0));
        };
        pload(0, 0, wa);                                          // in flight under the LayerNorm below
        pload(0, 1, wb);
        if (p.n2_g) layer_norm(p.n2_g, p.n2_b, p.n2_eps);
        lds_barrier();                                            // the staged stream rows have been read out
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int mb = 0; mb < 5; ++mb) {
                uint2 pk;
                pk.x = pack2(r[nb][mb][0], r[nb][mb][1]);
                pk.y = pack2(r[nb][mb][2], r[nb][mb][3]);
                *reinterpret_cast<uint2 *>(xn + (th2 * 32 + nb * 16 + l15) * XS + f0 + mb * 16) = pk;
            }
        lds_barrier();
        uint16_t *po = reinterpret_cast<uint16_t *>(p.proj_out);
        uint16_t *pdst = hc + l15 * XS + wave * 48 + lq * 4;
        for (int cq = 0; cq < ncq; ++cq) {
            f32x4 acc[3][4];
#pragma unroll
            for (int mb = 0; mb < 3; ++mb)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
            bf16x8 bfa[4], bfb[4];
            read_frags4(0, bfa);
#pragma unroll
            for (int s = 0; s < KT; ++s) {
                bf16x8(&cur)[4] = (s & 1) ? bfb : bfa;
                bf16x8(&nxt)[4] = (s & 1) ? bfa : bfb;
                bf16x8(&w)[4] = (s & 1) ? wb : wa;
                if (s + 1 < KT) read_frags4(s + 1, nxt);
#pragma unroll
                for (int mb = 0; mb < 3; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[mb], cur[nb], acc[mb][nb], 0, 0, 0);
                if (s + 2 < KT) pload(cq, s + 2, w);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (cq + 1 < ncq) {                                   // the next three bands' first steps travel under the stores below
                pload(cq + 1, 0, wa);
                pload(cq + 1, 1, wb);
                __builtin_amdgcn_sched_barrier(0);
            }
            // bias, bf16, and out through the free hidden-slab tile: 48 columns per wave, stored as 96-byte row segments
            if (cq > 0) lds_barrier();                            // the previous bands' rows have been read out
#pragma unroll
            for (int mb = 0; mb < 3; ++mb) {
                float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.proj_b && cq * 3 + mb < nb4) bv = *reinterpret_cast<const float4 *>(p.proj_b + wave * pd4 + (cq * 3 + mb) * 16 + lq * 4);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    uint2 pk;
                    pk.x = pack2(acc[mb][nb][0] + bv.x, acc[mb][nb][1] + bv.y);
                    pk.y = pack2(acc[mb][nb][2] + bv.z, acc[mb][nb][3] + bv.w);
                    *reinterpret_cast<uint2 *>(pdst + nb * 16 * XS + mb * 16) = pk;
                }
            }
            lds_barrier();
#pragma unroll
            for (int i = 0; i < TOK * 24 / NT; ++i) {             // 64 rows x 4 waves x 6 pieces of 16 bytes
                const int idx = tid + NT * i, row = idx / 24, rem = idx % 24, w_ = rem / 6, col = cq * 48 + (rem % 6) * 8;
                const uint4 v = *reinterpret_cast<const uint4 *>(hc + row * XS + w_ * 48 + (rem % 6) * 8);
                if (t0 + row < M && col < pd4) *reinterpret_cast<uint4 *>(po + (int64_t)(t0 + row) * p.proj_dim + w_ * pd4 + col) = v;
            }
        }
        return;
    }
    if (p.h_out) {
        if (p.n2_g) layer_norm(p.n2_g, p.n2_b, p.n2_eps);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int tok = t0 + th2 * 32 + nb * 16 + l15;
            if (tok < M) {
#pragma unroll
                for (int mb = 0; mb < 5; ++mb)
                    if (mb < nmb) {
                        if (p.h_dtype == CM_F32) {
                            *reinterpret_cast<float4 *>(reinterpret_cast<float *>(p.h_out) + (int64_t)tok * D + f0 + mb * 16) =
                                make_float4(r[nb][mb][0], r[nb][mb][1], r[nb][mb][2], r[nb][mb][3]);
                        } else {
                            uint2 pk;
                            pk.x = pack2(r[nb][mb][0], r[nb][mb][1]);
                            pk.y = pack2(r[nb][mb][2], r[nb][mb][3]);
                            *reinterpret_cast<uint2 *>(reinterpret_cast<uint16_t *>(p.h_out) + (int64_t)tok * D + f0 + mb * 16) = pk;
                        }
                    }
            }
        }
    }
}

template <bool ADD, bool PROJ, bool RACC>
int launch_ffn(const cm_ffn_args &a) {
    const size_t smem = (size_t)2 * TOK * XS * sizeof(uint16_t) + (size_t)2 * TOK * sizeof(float) + (size_t)a.hidden * sizeof(float);
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&ffn144_kernel<ADD, PROJ, RACC>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) {
            cm_set_error("ffn_fused: hipFuncSetAttribute failed: %s", hipGetErrorString(e));
            return (int)e;
        }
        attr_done = true;
    }
    hipLaunchKernelGGL((ffn144_kernel<ADD, PROJ, RACC>), dim3((a.rows + TOK - 1) / TOK), dim3(NT), smem, reinterpret_cast<hipStream_t>(a.stream), a);
    return cm_launch_status("cm_ffn_fused");
}

template <bool ADD, bool RACC>
int launch_ffn(const cm_ffn_args &a) {
    return a.proj_w ? launch_ffn<ADD, true, RACC>(a) : launch_ffn<ADD, false, RACC>(a);
}

// ---------------------------------------------------------------------------------------------------------------- cm_ln_pw_glu
// x <- x + alpha y; xn = LayerNorm(x) (bf16, LDS); g = (xn W_a^T + b_a) * sigmoid(xn W_g^T + b_g).  The weight's image is (288, 160):
// value feature f is row f, its gate row 144 + f -- 9 bands further on, so one lane holds both and the GLU stays in registers.  A wave
// owns a token half x a feature half (32 tokens x 5 tiles, both halves of the GLU); step s = 2 k-tile + (value | gate).  The upper
// feature half's tile 4 is the pad: its value band is a gate band, its gate band (clamped to the image's last) another, and it is dropped.
__global__ __launch_bounds__(NT, 2) void ln_pw_glu144_kernel(const cm_ln_pw_glu_args p) {
    __shared__ __attribute__((aligned(16))) uint16_t xn[TOK * XG];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fh = wave & 1, th2 = wave >> 1;
    const int nmb = fh ? 4 : 5;
    const int l15 = lane & 15, lq = lane >> 4;
    const int t0 = blockIdx.x * TOK, M = p.rows;
    const uint16_t *yv = reinterpret_cast<const uint16_t *>(p.y);

    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p.w), 0, 2 * D * KP * 2, 0x00020000);
    const int vl = lane * 16;
    auto wload = [&](int s, bf16x8(&dst)[5]) {
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
            dst[mb] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, vl, (min((s & 1) * (D / 16) + fh * 5 + mb, 2 * D / 16 - 1) * KT + (s >> 1)) * 1024, 0));
    };
    bf16x8 wa[5], wb[5];
    wload(0, wa);
    wload(1, wb);

    // ---- phase 0: x <- x + alpha y (written back), xn = LayerNorm(x) in bf16, pad columns zero
    {
        float4 v[4][3];
#pragma unroll
        for (int rd = 0; rd < 4; ++rd) {
            const int tok = min(t0 + wave * 16 + rd * 4 + lq, M - 1);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float4 x4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < 2 || l15 < C4 - 32) {
                    const int col = (l15 + 16 * i) * 4;
                    x4 = *reinterpret_cast<const float4 *>(p.x + (int64_t)tok * D + col);
                    if (yv) {
                        const uint2 a = *reinterpret_cast<const uint2 *>(yv + (int64_t)tok * D + col);
                        x4.x = fmaf(p.alpha, cm_bf16_lo(a.x), x4.x);
                        x4.y = fmaf(p.alpha, cm_bf16_hi(a.x), x4.y);
                        x4.z = fmaf(p.alpha, cm_bf16_lo(a.y), x4.z);
                        x4.w = fmaf(p.alpha, cm_bf16_hi(a.y), x4.w);
                    }
                }
                v[rd][i] = x4;
            }
        }
        if (p.x_out) {
#pragma unroll
            for (int rd = 0; rd < 4; ++rd) {
                const int tok = t0 + wave * 16 + rd * 4 + lq;
                if (tok < M) {
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (i < 2 || l15 < C4 - 32) *reinterpret_cast<float4 *>(p.x_out + (int64_t)tok * D + (l15 + 16 * i) * 4) = v[rd][i];
                }
            }
        }
        uint2 pk[4][3];
        ln_rows144(v, p.ln_g, p.ln_b, p.eps, l15, pk);
        store_rows144(xn, XG, wave * 16, l15, lq, pk);
    }
    lds_barrier();

    const uint16_t *xfrag = xn + (th2 * 32 + l15) * XG + lq * 8;
    auto read_frags = [&](int ks, bf16x8(&bf)[2]) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) bf[nb] = *reinterpret_cast<const bf16x8 *>(xfrag + nb * 16 * XG + ks * 32);
    };
    f32x4 acc[2][5][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[h][mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 bfa[2], bfb[2];
    read_frags(0, bfa);
#pragma unroll
    for (int s = 0; s < 2 * KT; ++s) {
        const int ks = s >> 1;
        bf16x8(&cur)[2] = (ks & 1) ? bfb : bfa;
        bf16x8(&nxt)[2] = (ks & 1) ? bfa : bfb;
        bf16x8(&w)[5] = (s & 1) ? wb : wa;
        if ((s & 1) == 0 && ks + 1 < KT) read_frags(ks + 1, nxt);
#pragma unroll
        for (int mb = 0; mb < 5; ++mb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[s & 1][mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[mb], cur[nb], acc[s & 1][mb][nb], 0, 0, 0);
        if (s + 2 < 2 * KT) wload(s + 2, w);
        __builtin_amdgcn_sched_barrier(0);                        // keep the refill here (see cm_ffn_fused)
    }
    // GLU in registers; the gated rows leave through the dead token tile as whole 288-byte rows
    const int f0 = fh * 80 + lq * 4;
    lds_barrier();                                                // every wave has read its last token fragments
#pragma unroll
    for (int mb = 0; mb < 5; ++mb)
        if (mb < nmb) {
            const float4 ba = *reinterpret_cast<const float4 *>(p.bias + f0 + mb * 16);
            const float4 bg = *reinterpret_cast<const float4 *>(p.bias + D + f0 + mb * 16);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const float o0 = (acc[0][mb][nb][0] + ba.x) * cm_sigmoid(acc[1][mb][nb][0] + bg.x);
                const float o1 = (acc[0][mb][nb][1] + ba.y) * cm_sigmoid(acc[1][mb][nb][1] + bg.y);
                const float o2 = (acc[0][mb][nb][2] + ba.z) * cm_sigmoid(acc[1][mb][nb][2] + bg.z);
                const float o3 = (acc[0][mb][nb][3] + ba.w) * cm_sigmoid(acc[1][mb][nb][3] + bg.w);
                *reinterpret_cast<uint2 *>(xn + (th2 * 32 + nb * 16 + l15) * XG + f0 + mb * 16) = uint2{pack2(o0, o1), pack2(o2, o3)};
            }
        }
    lds_barrier();
    uint16_t *out = reinterpret_cast<uint16_t *>(p.out);
    constexpr int PR = D / 8;                                     // 16-byte pieces per output row
#pragma unroll
    for (int i = 0; i < (TOK * PR + NT - 1) / NT; ++i) {
        const int idx = tid + NT * i, row = idx / PR, chunk = idx % PR;
        if (idx < TOK * PR && t0 + row < M)
            *reinterpret_cast<uint4 *>(out + (int64_t)(t0 + row) * D + chunk * 8) = *reinterpret_cast<const uint4 *>(xn + row * XG + chunk * 8);
    }
}

}  // namespace

// cm_ffn_fused at dim 144: the arguments are checked by cm_ffn_fused (ffn_fused.hip); racc as there
int cm_ffn_fused144_launch(const cm_ffn_args &a, bool racc) {
    if (racc) return a.addend ? launch_ffn<true, true>(a) : launch_ffn<false, true>(a);
    return a.addend ? launch_ffn<true, false>(a) : launch_ffn<false, false>(a);
}

// cm_ln_pw_glu at dim 144: the arguments are checked by cm_ln_pw_glu (ln_pw_glu.hip)
int cm_ln_pw_glu144_launch(const cm_ln_pw_glu_args &a) {
    hipLaunchKernelGGL(ln_pw_glu144_kernel, dim3((a.rows + TOK - 1) / TOK), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a);
    return cm_launch_status("cm_ln_pw_glu");
}
