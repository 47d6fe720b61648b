// cnn_front.hip — both blocks of the CNN front end in ONE kernel (contract: cm_cnn_front in include/conmamba_hip.h;
// reference hparams/CTC/conmamba_large.yaml:187-194 -> speechbrain ConvolutionFrontEnd, 2 x [Conv2d 3x3 stride 2 ->
// LayerNorm(freq, channel) -> LeakyReLU], channels (64, 32), on 80 mel bins).
//
// cm_cnn_block1 wrote its (batch, T/2 + 2, 42, 64) bf16 output to HBM (688 MB at 64 x 40 s) and cm_cnn_block2 read it
// back: 1.19 ms per step for ~50 GFLOP.  Block 1 is cheap to compute (one input channel, 9 taps), so here its rows are
// produced straight into the LDS tile block 2's implicit GEMM reads, and the intermediate never exists in memory:
//   * a persistent workgroup (8 waves) walks CONSECUTIVE tiles of 4 output steps of one utterance.  A tile needs 9
//     block-1 rows (stride 2, 3 taps); the last row of a tile is the first of the next and stays in LDS, so each tile
//     computes exactly 8 new rows = one per wave;
//   * a wave computes its block-1 row alone: 3 reflect-padded feature rows in a private LDS patch (prefetched into
//     registers one tile ahead), lane = (channel pair, frequency parity), 40 conv outputs per lane in registers,
//     LayerNorm statistics by wave reduction (no workgroup barrier), LeakyReLU, bf16 pair stores into the padded
//     [row][42][64 + 4] tile including the reflected frequency border;
//   * block 2 is cm_cnn_block2's scheme: v_mfma_f32_16x16x32_bf16 with the 32 x 576 weights as A
//     operands (fragment images staged once in LDS), positions as B operands read from the tile, conv outputs to LDS in fp32, then one wave per output
//     step does LayerNorm over 20 x 32 values + LeakyReLU and writes the bf16 row.
// HBM traffic: the features once (each input row is read by the 1-2 waves that need it) and the output once.
#include "cm_common.h"
#include "front_plan.h"

#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int F0 = 80;                    // mel bins
constexpr int C1 = 64, F1 = 40, F1P = 42; // block 1: channels, output bins, padded bins
constexpr int C2 = 32, F2 = 20;           // block 2
constexpr int TT = 4;                     // block-2 output steps per tile
constexpr int NR = 2 * TT + 1;            // block-1 rows per tile
constexpr int CS = 68;                    // tile column stride in bf16 elements (136 bytes: conflict-free fragments)
constexpr int OTS = 36;                   // block-2 output-tile row stride in floats
constexpr int FW = 84;                    // floats per staged feature row (82 used)
constexpr int NB = (TT * F2 + 15) / 16;   // waves with MFMA work (5)

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ __forceinline__ float wave_sum64(float v) {
    v = cm_group_sum<16>(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ uint32_t pack2(float a, float b) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));
}

struct front_lds {
    uint16_t rows[NR][F1P][CS];           // block-1 output tile (bf16), slot = padded row index mod NR
    float ot[NB * 16][OTS];               // block-2 conv outputs of the tile
    float fin[8][3][2][FW];               // per-wave reflect-padded feature rows, twice: copy 1 is copy 0 shifted by two bins,
                                          // so that a lane of either frequency parity reads its 3-tap window 16-byte aligned
    float ln1[2][F1 * C1];                // block-1 LayerNorm weight / bias
    bf16x8 wfrag[2][18][64];              // block-2 weights as MFMA A-operand fragment images (36 KB; in registers they
};                                        // cost 144 VGPRs and pushed the block-1 row computation into scratch)

constexpr int T_OPEN = 1 << 29;           // cm_cnn_front_stream: T / T1 while the utterance's end is unknown: no index reflects against it

// STREAM (cm_cnn_front_stream; ARGS = cm_cnn_front_stream_args): the launch produces rows [r0, r0 + nr) of utterances whose feature
// frames arrive in chunks; T2 is then r0 + nr, T / T1 are T_OPEN unless the call ends the utterance, and the tile walk starts at
// row r0 (tile k = rows r0 + 4 k ..: a slot is the padded row index mod NR, whatever the start).  Only the feature addresses,
// the clamp of the padded row index and the output row differ: block1_row, the MFMA chain and both LayerNorms are the same
// statements for both instantiations, so a row has the same bits.
//
// Per slot (cm_cnn_front_stream_slots; ARGS = cf_slot_args): f0, nf, r0, nr and T_total of stream b come from row b of the (batch, 8)
// int32 plan table of the front end's per-slot entry points (front_plan.h: PL_F0 .. PL_TTOTAL); the struct's nf and nr are then the maxima over the
// slots, the row strides of feats and out, and the launch's T / T1 / T2 / tiles_per_utt are replaced per stream.  Chunks of tiles
// past a stream's own rows are skipped.
struct cf_slot_args : cm_cnn_front_stream_args {
    const int32_t *plan;
};

// Whole utterances of different lengths (cm_cnn_front_lens; ARGS = cf_lens_args, STREAM = false): utterance b has frames[b] feature
// frames, clamped to [0, p.T]; T / T1 / T2 / tiles_per_utt are replaced per utterance, so both reflections happen at its own ends and
// its rows past T2 are not computed.  p.T stays the row stride of feats, ceil(ceil(p.T / 2) / 2) that of out.  Under 5 frames the
// utterance is skipped.
struct cf_lens_args : cm_cnn_front_args {
    const int32_t *frames;
};

template <bool STREAM, typename ARGS>
__global__ __launch_bounds__(512) void cnn_front_kernel(const ARGS p, int T, int T1, int T2, int tiles_per_utt, int chunk, int chunks_per_utt,
                                                        int nchunks) {
    constexpr bool SLOT = std::is_same<ARGS, cf_slot_args>::value;
    constexpr bool LENS = std::is_same<ARGS, cf_lens_args>::value;
    [[maybe_unused]] int f0s = 0, nfs = 1;                        // SLOT: this stream's first frame and frame count
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    front_lds &L = *reinterpret_cast<front_lds *>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    int rbase, tp_last;                                           // first row of the launch; last padded block-1 row a fetch may name
    if constexpr (STREAM) { rbase = p.r0; tp_last = 2 * T2; }     // (row T2 - 1 reads the padded rows up to 2 T2)
    else { rbase = 0; tp_last = T1 + 1; }

    // ---- constants held in registers for the whole kernel
    const uint16_t *W2 = reinterpret_cast<const uint16_t *>(p.w2);                    // (32, 3, 3, 64) bf16
    for (int i = tid; i < 2 * 18 * 64; i += 512) {
        const int cb = i / (18 * 64), ks = (i / 64) % 18, ln = i % 64;
        L.wfrag[cb][ks][ln] = *reinterpret_cast<const bf16x8 *>(W2 + ((int64_t)(cb * 16 + (ln & 15)) * 9 + (ks >> 1)) * C1 + (ks & 1) * 32 + (ln >> 4) * 8);
    }
    float4 bias2[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
        bias2[cb] = p.b2 ? *reinterpret_cast<const float4 *>(p.b2 + cb * 16 + lq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int cp = lane & 31, fh = lane >> 5;                     // block 1: channel pair, frequency parity
    f32x2 w1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w1[k] = f32x2{p.w1[(2 * cp) * 9 + k], p.w1[(2 * cp + 1) * 9 + k]};
    const float b1a = p.b1 ? p.b1[2 * cp] : 0.f, b1b = p.b1 ? p.b1[2 * cp + 1] : 0.f;
    for (int i = tid; i < F1 * C1; i += 512) { L.ln1[0][i] = p.ln1_g[i]; L.ln1[1][i] = p.ln1_b[i]; }

    // this lane's block-2 output position inside a tile (clamped duplicates past the tile are not used)
    const int pidx = min(wave * 16 + l15, TT * F2 - 1);
    const int pr = pidx / F2, pf = pidx % F2;
    uint16_t *out = reinterpret_cast<uint16_t *>(p.out);

    // feature rows of padded block-1 row tp of utterance b: 3 rows x 82 reflect-padded bins, 4 values per lane
    [[maybe_unused]] const float *hist = nullptr;                 // STREAM: the utterance's FH feature rows in front of feats
    auto fetch_rows = [&](const float *feats, int tp, float (&r)[4]) {
        const int t1 = reflect_idx(min(tp, tp_last) - 1, T1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = lane + 64 * k;
            r[k] = 0.f;
            if (idx < 3 * 82) {
                const int rr = idx / 82, fc = idx - rr * 82;
                const int fr = reflect_idx(2 * t1 + rr - 1, T), bin = reflect_idx(fc - 1, F0);
                if constexpr (STREAM) {
                    // frame fr of the utterance: in this call's rows from f0 on, in the history behind it.  The clamps hold the address
                    // inside the two arrays for any argument; the entry point's checks make them idle
                    int c, nfl;
                    if constexpr (SLOT) { c = fr - f0s; nfl = nfs; }
                    else { c = fr - p.f0; nfl = p.nf; }
                    r[k] = (c >= 0 || !hist) ? feats[(int64_t)min(max(c, 0), nfl - 1) * F0 + bin] : hist[(int64_t)max(c + FH, 0) * F0 + bin];
                } else {
                    r[k] = feats[(int64_t)fr * F0 + bin];
                }
            }
        }
    };
    auto stage_rows = [&](const float (&r)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = lane + 64 * k;
            if (idx < 3 * 82) {
                const int rr = idx / 82, fc = idx % 82;
                L.fin[wave][rr][0][fc] = r[k];
                if (fc >= 2) L.fin[wave][rr][1][fc - 2] = r[k];
            }
        }
    };
    // one block-1 row (from this wave's staged feature rows) -> tile slot
    auto block1_row = [&](int slot) {
        float v[2 * (F1 / 2)];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < F1 / 2; ++i) {
            // output bin f1 = 2 i + fh reads bins 2 f1 .. 2 f1 + 2 of the padded rows = floats 4 i .. 4 i + 2 of copy fh: one
            // 16-byte read per input row (the lanes of one parity share the address: broadcast), both channels of the
            // lane's pair per v_pk_fma_f32
            f32x2 a2 = {b1a, b1b};
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) {
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(&L.fin[wave][dt][fh][4 * i]);
#pragma unroll
                for (int df = 0; df < 3; ++df) a2 = __builtin_elementwise_fma(w1[dt * 3 + df], f32x2{xv[df], xv[df]}, a2);
            }
            v[2 * i] = a2.x; v[2 * i + 1] = a2.y;
            s += a2.x + a2.y;
            if (i & 1) __builtin_amdgcn_sched_barrier(0);        // keeps the compiler from hoisting all 60 LDS reads (spills)
        }
        const float mean = wave_sum64(s) * (1.f / (F1 * C1));
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < F1; ++i) { v[i] -= mean; sq = fmaf(v[i], v[i], sq); }
        const float rstd = rsqrtf(wave_sum64(sq) * (1.f / (F1 * C1)) + p.eps1);
#pragma unroll
        for (int i = 0; i < F1 / 2; ++i) {
            const int f1 = 2 * i + fh, o = f1 * C1 + 2 * cp;
            const float2 g = *reinterpret_cast<const float2 *>(&L.ln1[0][o]);
            const float2 bt = *reinterpret_cast<const float2 *>(&L.ln1[1][o]);
            float y0 = fmaf(v[2 * i] * rstd, g.x, bt.x), y1 = fmaf(v[2 * i + 1] * rstd, g.y, bt.y);
            y0 = y0 > 0.f ? y0 : p.slope * y0;
            y1 = y1 > 0.f ? y1 : p.slope * y1;
            const uint32_t pk = pack2(y0, y1);
            *reinterpret_cast<uint32_t *>(&L.rows[slot][f1 + 1][2 * cp]) = pk;
            if (f1 == 1) *reinterpret_cast<uint32_t *>(&L.rows[slot][0][2 * cp]) = pk;              // reflected borders
            if (f1 == F1 - 2) *reinterpret_cast<uint32_t *>(&L.rows[slot][F1P - 1][2 * cp]) = pk;
        }
    };

    for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int b = ch / chunks_per_utt, tile0 = (ch % chunks_per_utt) * chunk;
        [[maybe_unused]] int out_rows = 0;                        // SLOT / LENS: rows of out per stream (the widest one's)
        if constexpr (SLOT) {
            const int32_t *s = p.plan + (int64_t)b * PL_W;
            const int nr = s[PL_NR], Tt = s[PL_TTOTAL];
            f0s = s[PL_F0], nfs = max(s[PL_NF], 1), rbase = s[PL_R0];
            T = Tt >= 0 ? Tt : T_OPEN, T1 = Tt >= 0 ? (Tt + 1) / 2 : T_OPEN, T2 = rbase + nr, tp_last = 2 * T2;
            tiles_per_utt = (nr + TT - 1) / TT;
            out_rows = p.nr;
            if (tile0 >= tiles_per_utt) continue;                 // uniform over the workgroup: b depends on ch only
        }
        if constexpr (LENS) {
            const int Tb = min(max(p.frames[b], 0), p.T);
            T = Tb, T1 = (Tb + 1) / 2, T2 = (T1 + 1) / 2, tp_last = T1 + 1;
            tiles_per_utt = (T2 + TT - 1) / TT;
            out_rows = ((p.T + 1) / 2 + 1) / 2;
            if (Tb < 5 || tile0 >= tiles_per_utt) continue;       // uniform over the workgroup: b depends on ch only
        }
        const int tile1 = min(tile0 + chunk, tiles_per_utt);
        const float *feats;
        if constexpr (LENS) {
            feats = p.feats + (int64_t)b * p.T * F0;
        } else if constexpr (STREAM) {
            feats = p.feats + (int64_t)b * p.nf * F0;
            hist = p.feat_hist ? p.feat_hist + (int64_t)b * FH * F0 : nullptr;
        } else {
            feats = p.feats + (int64_t)b * T * F0;
        }
        float pre[4];
        __syncthreads();                                          // previous chunk's tile is dead (and ln1 is staged)
        // chunk prologue: padded row 8*tile0 (the row every later tile inherits) by wave 0
        const int tpc = 2 * (rbase + TT * tile0);
        if (wave == 0) {
            fetch_rows(feats, tpc, pre);
            stage_rows(pre);
            block1_row(tpc % NR);
        }
        fetch_rows(feats, tpc + 1 + wave, pre);
        for (int tile = tile0; tile < tile1; ++tile) {
            const int r0 = rbase + TT * tile, tp0 = 2 * r0;
            // ---- block 1: wave w -> padded row tp0 + 1 + w
            stage_rows(pre);
            if (tile + 1 < tile1) fetch_rows(feats, tp0 + 2 * TT + 1 + wave, pre);      // next tile's rows, one tile ahead
            block1_row((tp0 + 1 + wave) % NR);
            cm_lds_barrier();
            // ---- block 2: implicit GEMM, 16 positions x 32 channels per wave
            if (wave < NB) {
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                const uint16_t *fr[3];
#pragma unroll
                for (int dt = 0; dt < 3; ++dt) fr[dt] = &L.rows[(tp0 + 2 * pr + dt) % NR][2 * pf][lq * 8];
#pragma unroll
                for (int ks = 0; ks < 18; ++ks) {
                    const int tap = ks >> 1, dt = tap / 3, df = tap % 3;
                    const bf16x8 bfr = *reinterpret_cast<const bf16x8 *>(fr[dt] + df * CS + (ks & 1) * 32);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L.wfrag[0][ks][lane], bfr, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(L.wfrag[1][ks][lane], bfr, acc1, 0, 0, 0);
                }
                float *o = &L.ot[wave * 16 + l15][lq * 4];
                *reinterpret_cast<float4 *>(o) = make_float4(acc0[0] + bias2[0].x, acc0[1] + bias2[0].y, acc0[2] + bias2[0].z, acc0[3] + bias2[0].w);
                *reinterpret_cast<float4 *>(o + 16) = make_float4(acc1[0] + bias2[1].x, acc1[1] + bias2[1].y, acc1[2] + bias2[1].z, acc1[3] + bias2[1].w);
            }
            cm_lds_barrier();
            // ---- LayerNorm over (freq, channel) + LeakyReLU, one wave per output step
            if (wave < TT && r0 + wave < T2) {
                constexpr int nfeat = F2 * C2;
                const float *orow = &L.ot[wave * F2][0];
                float2 vv[nfeat / 128];
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < nfeat / 128; ++k) {
                    const int i = lane + 64 * k;
                    vv[k] = *reinterpret_cast<const float2 *>(orow + (i >> 4) * OTS + 2 * (i & 15));
                    s += vv[k].x + vv[k].y;
                }
                const float mean = wave_sum64(s) * (1.f / nfeat);
                float sq = 0.f;
#pragma unroll
                for (int k = 0; k < nfeat / 128; ++k) {
                    vv[k].x -= mean; vv[k].y -= mean;
                    sq = fmaf(vv[k].x, vv[k].x, fmaf(vv[k].y, vv[k].y, sq));
                }
                const float rstd = rsqrtf(wave_sum64(sq) * (1.f / nfeat) + p.eps2);
                uint16_t *dst = out + ((int64_t)b * (SLOT || LENS ? out_rows : T2 - rbase) + (r0 - rbase) + wave) * nfeat;
#pragma unroll
                for (int k = 0; k < nfeat / 128; ++k) {
                    const int i = lane + 64 * k;
                    const float2 g = *reinterpret_cast<const float2 *>(p.ln2_g + 2 * i);
                    const float2 bt = *reinterpret_cast<const float2 *>(p.ln2_b + 2 * i);
                    float y0 = fmaf(vv[k].x * rstd, g.x, bt.x), y1 = fmaf(vv[k].y * rstd, g.y, bt.y);
                    y0 = y0 > 0.f ? y0 : y0 * p.slope;
                    y1 = y1 > 0.f ? y1 : y1 * p.slope;
                    *reinterpret_cast<uint32_t *>(dst + 2 * i) = pack2(y0, y1);
                }
            }
            // the next tile overwrites 8 of the 9 row slots and ot: everyone must be done reading them
            cm_lds_barrier();
        }
    }
}

// ---- host side.  The four entry points keep their own pointer checks and say what the kernel gets; the rest is written once.  `sym` is
// an entry point's symbol, `who` = sym + 3 the name its messages begin with (no "cm_").

// What cm_cnn_front_args and cm_cnn_front_stream_args have in common, in one order for every entry: NULL / sizes (`counts`: the entry's
// own condition on its counts), then the shape, then the alignment.
template <typename A>
int cnn_front_check(const A &a, bool counts, const char *who) {
    CM_REQUIRE(a.batch > 0 && counts && a.feats && a.w1 && a.ln1_g && a.ln1_b && a.w2 && a.ln2_g && a.ln2_b && a.out, CM_EINVAL,
               "%s: bad sizes or NULL tensor", who);
    CM_REQUIRE(a.F == F0 && a.C1 == C1 && a.C2 == C2, CM_EUNSUPPORTED, "%s: only 80 bins, channels (64, 32) (got F %d, C %d, %d)", who, a.F,
               a.C1, a.C2);
    CM_REQUIRE(cm_aligned(a.w2, 16) && cm_aligned(a.out, 4) && cm_aligned(a.ln1_g, 8) && cm_aligned(a.ln1_b, 8) && cm_aligned(a.ln2_g, 8) &&
                   cm_aligned(a.ln2_b, 8) && (!a.b2 || cm_aligned(a.b2, 16)),
               CM_EALIGN, "%s: w2 / b2 must be 16-byte aligned, LayerNorm parameters 8-byte aligned", who);
    return CM_OK;
}

// The grid and the chunks are those of `rows` output rows per utterance (the widest one's: a chunk past an utterance's own tiles is
// skipped); T / T1 / T2 are the kernel's, replaced per utterance by the lens and per-slot instantiations.
template <bool STREAM, typename ARGS>
int cnn_front_launch(const ARGS &k, int rows, int T, int T1, int T2, const char *sym) {
    const int tiles_per_utt = (rows + TT - 1) / TT;
    const int chunk = 16;
    const int chunks_per_utt = (tiles_per_utt + chunk - 1) / chunk;
    const int64_t nchunks = (int64_t)k.batch * chunks_per_utt;
    CM_REQUIRE(nchunks <= 2147483647, CM_EINVAL, "%s: too many chunks", sym + 3);
    static bool attr_done = false;                                // one per instantiation
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(cnn_front_kernel<STREAM, ARGS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        if (e != hipSuccess) {
            cm_set_error("%s: hipFuncSetAttribute failed: %s", sym + 3, hipGetErrorString(e));
            return (int)e;
        }
        attr_done = true;
    }
    const int64_t grid = nchunks < 256 ? nchunks : 256;
    hipLaunchKernelGGL((cnn_front_kernel<STREAM, ARGS>), dim3((unsigned)grid), dim3(512), sizeof(front_lds),
                       reinterpret_cast<hipStream_t>(k.stream), k, T, T1, T2, tiles_per_utt, chunk, chunks_per_utt, (int)nchunks);
    return cm_launch_status(sym);
}

// ": slot b" behind the entry's name in a per-slot refusal, nothing for slot < 0; built where a message is, on the failing path only
struct slot_tag {
    char s[24];
    explicit slot_tag(int slot) {
        s[0] = 0;
        if (slot >= 0) snprintf(s, sizeof s, ": slot %d", slot);
    }
};

// The conditions of the streamed form on one stream's counts: cm_cnn_front_stream's own scalars (slot -1), or row `slot` of the per-slot
// plan.
int cnn_front_stream_check(int64_t f0, int64_t nf, int64_t r0, int64_t nr, int64_t Tt, bool hist, const char *who, int slot) {
    const int64_t fend = f0 + nf, rend = r0 + nr;
    if (Tt >= 0) {                                                // the call ends the utterance: rows up to T2 - 1, reflected at T and T1
        CM_REQUIRE(Tt >= 5 && Tt == fend, CM_EINVAL, "%s%s: T_total must be f0 + nf and at least 5", who, slot_tag(slot).s);
        CM_REQUIRE(rend <= ((Tt + 1) / 2 + 1) / 2, CM_EINVAL, "%s%s: row %d is past the utterance's last", who, slot_tag(slot).s, (int)rend - 1);
    } else {
        CM_REQUIRE(4 * (rend - 1) + 3 < fend, CM_EINVAL, "%s%s: row %d needs frames that have not arrived", who, slot_tag(slot).s, (int)rend - 1);
    }
    // the lowest frame a row of the launch names: 4 r0 - 3 (reflected at 0), or T - 5 through the reflections at the end
    const int64_t lowest = std::min<int64_t>(std::max<int64_t>(4 * r0 - 3, 0), Tt >= 0 ? Tt - 5 : fend);
    CM_REQUIRE(lowest >= (hist ? f0 - FH : f0), CM_EINVAL, "%s%s: row %d reaches behind the feature history", who, slot_tag(slot).s, (int)r0);
    return CM_OK;
}

}  // namespace

extern "C" int cm_cnn_front(const cm_cnn_front_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "cnn_front: args is NULL");
    const cm_cnn_front_args &a = *args;
    if (int rc = cnn_front_check(a, a.T >= 5, "cnn_front")) return rc;
    const int T1 = (a.T + 1) / 2, T2 = (T1 + 2 - 3) / 2 + 1;
    return cnn_front_launch<false>(a, T2, a.T, T1, T2, "cm_cnn_front");
}

extern "C" int cm_cnn_front_lens(const cm_cnn_front_args *args, const int32_t *frames) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "cnn_front_lens: args is NULL");
    CM_REQUIRE(frames != nullptr, CM_EINVAL, "cnn_front_lens: frames is NULL (cm_cnn_front is the form without lengths)");
    CM_REQUIRE(cm_aligned(frames, 4), CM_EALIGN, "cnn_front_lens: frames must be 4-byte aligned");
    const cm_cnn_front_args &a = *args;
    if (int rc = cnn_front_check(a, a.T >= 5, "cnn_front_lens")) return rc;
    cf_lens_args k{};
    static_cast<cm_cnn_front_args &>(k) = a;
    k.frames = frames;
    const int T1 = (a.T + 1) / 2, T2 = (T1 + 2 - 3) / 2 + 1;       // of the widest utterance
    return cnn_front_launch<false>(k, T2, a.T, T1, T2, "cm_cnn_front_lens");
}

extern "C" int cm_cnn_front_stream(const cm_cnn_front_stream_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "cnn_front_stream: args is NULL");
    const cm_cnn_front_stream_args &a = *args;
    if (int rc = cnn_front_check(a, a.nf > 0 && a.nr > 0 && a.f0 >= 0 && a.r0 >= 0, "cnn_front_stream")) return rc;
    CM_REQUIRE((int64_t)a.f0 + a.nf < T_OPEN, CM_EUNSUPPORTED, "cnn_front_stream: frame index too large");
    if (int rc = cnn_front_stream_check(a.f0, a.nf, a.r0, a.nr, a.T_total, a.feat_hist != nullptr, "cnn_front_stream", -1)) return rc;
    const int T = a.T_total >= 0 ? a.T_total : T_OPEN, T1 = a.T_total >= 0 ? (T + 1) / 2 : T_OPEN;
    return cnn_front_launch<true>(a, a.nr, T, T1, a.r0 + a.nr, "cm_cnn_front_stream");
}

// The struct's nf and nr are the maxima over the slots; its f0 / r0 / T_total are not read.  A slot without rows is not checked further.
extern "C" int cm_cnn_front_stream_slots(const cm_cnn_front_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "cnn_front_stream_slots: args is NULL");
    CM_REQUIRE(plan_host != nullptr && plan_dev != nullptr, CM_EINVAL, "cnn_front_stream_slots: plan is NULL (host copy and device copy)");
    CM_REQUIRE(cm_aligned(plan_host, 4) && cm_aligned(plan_dev, 4), CM_EALIGN, "cnn_front_stream_slots: plan must be 4-byte aligned");
    const cm_cnn_front_stream_args &a = *args;
    if (int rc = cnn_front_check(a, a.nf > 0 && a.nr > 0, "cnn_front_stream_slots")) return rc;
    for (int b = 0; b < a.batch; ++b) {
        const int32_t *s = plan_host + (int64_t)b * PL_W;
        const int64_t f0 = s[PL_F0], nf = s[PL_NF], r0 = s[PL_R0], nr = s[PL_NR];
        CM_REQUIRE(f0 >= 0 && nf >= 0 && r0 >= 0 && nr >= 0 && nf <= a.nf && nr <= a.nr, CM_EINVAL,
                   "cnn_front_stream_slots: slot %d: counts below 0 or above the maxima (nf %d of %d, nr %d of %d)", b, (int)nf, a.nf, (int)nr, a.nr);
        if (nr == 0) continue;
        CM_REQUIRE(nf > 0 && f0 + nf < T_OPEN, CM_EINVAL, "cnn_front_stream_slots: slot %d has rows but no frames, or a frame index too large", b);
        if (int rc = cnn_front_stream_check(f0, nf, r0, nr, s[PL_TTOTAL], a.feat_hist != nullptr, "cnn_front_stream_slots", b)) return rc;
    }
    cf_slot_args k{};
    static_cast<cm_cnn_front_stream_args &>(k) = a;
    k.plan = plan_dev;
    return cnn_front_launch<true>(k, a.nr, T_OPEN, T_OPEN, 0, "cm_cnn_front_stream_slots");
}
