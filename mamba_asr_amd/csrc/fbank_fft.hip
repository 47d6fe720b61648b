// fbank_fft.hip — waveform -> log-mel features in ONE kernel (contract: cm_fbank_wav in include/conmamba_hip.h;
// speechbrain Fbank semantics as restated in SURVEY Appendix A: STFT(n_fft 512, Hamming window centred in the frame,
// hop, center=True with zero padding) -> power -> triangular mel -> 10 log10 (floor amin); cm_fbank_finish then
// applies top_db and the global normalisation).
//
// Through the vendor FFT this stage was: pad kernel, frame+window kernel (524 MB written at 64 x 40 s), rocFFT (two
// kernels + per-chunk copies), then cm_fbank_mel_db reading the 526 MB complex spectrum: ~1.6 ms per 64-utterance step
// for 6 GFLOP.  Here a wave owns a frame end to end and nothing but the waveform (read ~3.2x through L1/L2: frames
// overlap) and the 80 log-mel values per frame touch memory:
//   * real FFT of 512 points = complex FFT of 256 points on z[m] = x[2m] + i x[2m+1] + one split step;
//   * complex FFT-256 = four radix-4 decimation-in-frequency stages, one butterfly per lane per stage, in place in a
//     2 KB per-wave LDS buffer (a wave's LDS operations execute in order: no barriers); stage 0 takes its inputs
//     straight from global memory (8-byte loads, window applied in registers) and the lane's twiddles for the three
//     twiddled stages stay in registers across frames;
//   * outputs land in base-4 digit-reversed order, so lane l finds Z[l + 64 i], i = 0..3, in 32 contiguous bytes;
//   * |X[k]|^2 goes to the [bin][frame] power tile in LDS and the mel / dB stage of cm_fbank_mel_db runs unchanged.
#include "cm_common.h"
#include "front_plan.h"

#include <type_traits>

namespace {

constexpr int FT = 16;            // frames per workgroup (4 per wave)
constexpr int PWS = FT + 1;       // power-tile row stride (odd: conflict-free mel loop)
constexpr int NF = 512;           // n_fft
constexpr int NH = NF / 2;        // complex FFT length
constexpr int HS = NF;            // cm_fbank_wav_stream: samples of history per stream (a frame reaches back fewer than n_fft)
constexpr int BWCAP = 1024;       // band weights staged in LDS (triangular filters: <= 2 per bin = 514 for 257 bins); a larger
                                  // table is read from global memory instead.  4 KB instead of the table's 16 KB bound: a
                                  // workgroup holds 32.5 KB of LDS and four of them (16 waves) share a CU

// 8-byte aligned: LDS accesses are ds_read_b64 / ds_write_b64 (a 4-byte aligned pair compiles to ds_read2_b32, whose two
// dword accesses are banked separately modulo 32 dwords: every element access of the padded layouts below was 2-way)
struct __attribute__((aligned(8))) cf { float re, im; };
__device__ __forceinline__ cf operator+(cf a, cf b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cf operator-(cf a, cf b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cf cmul(cf a, cf b) { return {fmaf(a.re, b.re, -a.im * b.im), fmaf(a.re, b.im, a.im * b.re)}; }
__device__ __forceinline__ cf mul_mi(cf a) { return {a.im, -a.re}; }      // a * (-i)

// radix-4 DIF butterfly: y_q = sum_r a_r (-i)^{q r}
__device__ __forceinline__ void bfly4(cf &a0, cf &a1, cf &a2, cf &a3) {
    const cf b0 = a0 + a2, b1 = a0 - a2, b2 = a1 + a3, b3 = mul_mi(a1 - a3);
    a0 = b0 + b2; a2 = b0 - b2; a1 = b1 + b3; a3 = b1 - b3;
}

// LDS position of FFT element p: 4 pad elements per 16 spread the strided butterflies of stages 1 and 2 over the banks
__device__ __forceinline__ int zp(int p) { return p + 4 * (p >> 4); }
// ... and from the output of stage 2 on, one pad element per 4: stage 3 and the split step have every lane walk FOUR
// CONSECUTIVE elements (lane stride 4 elements = 32 bytes: 4-way conflicts on the 8-byte accesses under zp -- rocprofv3
// counted 70 % of this kernel's LDS cycles as bank conflicts and the LDS array busy 85 % of its duration); with a lane
// stride of 5 elements the 32 lanes of a ds_read_b64 group hit 32 different 8-byte slots.  Stage 2 reads under zp and
// writes under zq: a wave's LDS instructions execute in order and its four reads cover the whole buffer before the first write.
__device__ __forceinline__ int zq(int p) { return p + (p >> 2); }
constexpr int ZN = NH + NH / 4;       // padded work-buffer length (both paddings)

__device__ __forceinline__ int rev4_8bit(int k) {                     // reverse the four base-4 digits of k < 256
    return ((k & 3) << 6) | ((k & 12) << 2) | ((k >> 2) & 12) | (k >> 6);
}

// floor_db = 10 log10(amin) rounded once from double on the host: log10f is an ulp or two off, and silence must sit ON the floor
//
// STREAM (cm_fbank_wav_stream; ARGS = cm_fbank_stream_args): the launch covers frames [f0, f0 + nf) of an utterance whose samples
// arrive in chunks.  Only the sample fetch, the store addresses and the per-frame maxima differ: the window, the four stages,
// the split step and the mel loop below are the same statements for both instantiations, so a frame has the same bits.
//
// Per slot (cm_fbank_wav_stream_slots; ARGS = fb_slot_args): n, consumed, total, f0 and nf of stream b come from row b of a (batch, 8)
// int32 plan table instead of the struct, whose n and nf are then the maxima over the slots: the widths of chunk and of db / fmax
// and the size of the grid.  Workgroups past a slot's own frames exit; workgroup 0 rolls the sample history of every slot, idle or not.
struct fb_slot_args : cm_fbank_stream_args {
    const int32_t *plan;
};
// Whole utterances of different lengths (cm_fbank_wav_lens; ARGS = fb_lens_args, STREAM = false): utterance b has nsamp[b] samples,
// clamped to [0, samples] -- the waveform's descriptor ends there, so what lies behind reads as zero -- and 1 + nsamp[b] / hop frames
// (none for 0 samples).  Frames past them are not computed and stay out of the tile maxima; the struct's frames is the row stride of db.
struct fb_lens_args : cm_fbank_args {
    const int32_t *nsamp;
};
// the arguments with the counts of row b of a plan table (front_plan.h) in place of the struct's own
template <typename ARGS>
__host__ __device__ __forceinline__ ARGS fb_row_view(const ARGS &pk, const int32_t *plan, int b) {
    ARGS q = pk;
    const int32_t *s = plan + (int64_t)b * PL_W;
    q.n = s[PL_N], q.consumed = s[PL_CONSUMED], q.total = s[PL_TOTAL], q.f0 = s[PL_F0], q.nf = s[PL_NF];
    return q;
}
template <typename ARGS>
__device__ __forceinline__ ARGS fb_view(const ARGS &pk, int b) {      // the arguments as stream b sees them
    if constexpr (std::is_same<ARGS, fb_slot_args>::value) return fb_row_view(pk, pk.plan, b);
    else return pk;
}

template <bool STREAM, typename ARGS>
__global__ __launch_bounds__(256) void fbank_wav_kernel(const ARGS pk, const float floor_db) {
    extern __shared__ float sm[];
    constexpr bool SLOT = std::is_same<ARGS, fb_slot_args>::value;
    constexpr bool LENS = std::is_same<ARGS, fb_lens_args>::value;
    const int b = blockIdx.y;
    const ARGS p = fb_view(pk, b);
    int t0, T;                                                    // first frame of this workgroup, end of the valid frames
    [[maybe_unused]] int nsv = 0;                                 // LENS: this utterance's samples
    if constexpr (STREAM) { t0 = p.f0 + blockIdx.x * FT; T = p.f0 + p.nf; }
    else if constexpr (LENS) {
        nsv = min(max(p.nsamp[b], 0), p.samples);
        t0 = blockIdx.x * FT; T = nsv > 0 ? 1 + nsv / p.hop : 0;
        if (t0 >= T) {                                            // the whole workgroup, before any barrier: no frame of the utterance here
            if (threadIdx.x == 0) p.umax_part[(int64_t)b * gridDim.x + blockIdx.x] = -INFINITY;
            return;
        }
    }
    else { t0 = blockIdx.x * FT; T = p.frames; }
    const int F = NH + 1, M = p.n_mels;
    float *pw = sm;                                               // [F][PWS] power tile
    int *band = reinterpret_cast<int *>(pw + F * PWS);            // [3 M + 1]
    float *bw = reinterpret_cast<float *>(band + 3 * M + 1);      // [BWCAP] packed band weights
    cf *zb = reinterpret_cast<cf *>(bw + BWCAP + ((3 * M + 1 + F * PWS) & 1));  // [4 waves][ZN] FFT work buffers (padded), 8-byte aligned
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // sample s of the utterance (STREAM): zero in front of it and past its end, else from [hist | chunk]; an index neither
    // array holds reads as zero too, so that no address outside them is ever formed
    [[maybe_unused]] auto sample = [&](int s) -> unsigned int {
        if constexpr (STREAM) {
            if (s < 0 || (p.total >= 0 && s >= p.total)) return 0u;
            const int c = s - p.consumed;
            if (c >= 0) return c < p.n ? __float_as_uint(p.chunk[(int64_t)b * p.chunk_bs + c]) : 0u;
            return c >= -HS ? __float_as_uint(p.hist[(int64_t)b * HS + c + HS]) : 0u;
        } else {
            return 0u;
        }
    };
    if constexpr (STREAM) {
        if (blockIdx.x == 0)                                      // the next call's history: the last HS samples of [hist | chunk]
            for (int j = tid; j < HS; j += 256) p.hist_out[(int64_t)b * HS + j] = __uint_as_float(sample(p.consumed + p.n - HS + j));
        if (p.nf == 0 || (SLOT && t0 >= T)) return;
    }
    for (int m = tid; m < M; m += 256) { band[m] = p.band_lo[m]; band[M + m] = p.band_hi[m]; }
    for (int m = tid; m <= M; m += 256) band[2 * M + m] = p.band_off[m];
    const int bw_total = p.band_off[M];
    const bool bw_lds = bw_total <= BWCAP;
    if (bw_lds)
        for (int i = tid; i < bw_total; i += 256) bw[i] = p.band_w[i];

    // ---- per-lane constants
    const cf *tw = reinterpret_cast<const cf *>(p.twiddle);       // tw[k] = exp(-2 pi i k / 512)
    cf w0[3], w1[3], w2[3];                                       // twiddles of stages 0..2: W_L^{q j}, q = 1..3
    {
        const int j0 = lane, j1 = lane & 15, j2 = lane & 3;
#pragma unroll
        for (int q = 1; q <= 3; ++q) {
            w0[q - 1] = tw[2 * ((q * j0) & 255)];                 // L = 256: W_256^{q j} = tw[2 q j]
            w1[q - 1] = tw[2 * ((4 * q * j1) & 255)];             // L = 64
            w2[q - 1] = tw[2 * ((16 * q * j2) & 255)];            // L = 16
        }
    }
    float2 win[4];                                                // window at samples 2m, 2m+1 for m = lane + 64 q
#pragma unroll
    for (int q = 0; q < 4; ++q) win[q] = *reinterpret_cast<const float2 *>(p.window + 2 * (lane + 64 * q));
    // split-step constants for k = lane + 64 i: position of Z[(256 - k) & 255] and exp(-2 pi i k / 512)
    int ppos[4];
    cf wk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;
        ppos[i] = zq(rev4_8bit((NH - k) & (NH - 1)));
        wk[i] = tw[k];
    }
    const int r3 = ((lane & 3) << 4) | (lane & 12) | (lane >> 4);  // Z[lane + 64 i] sits at position 4 r3 + i
    __amdgpu_buffer_rsrc_t wr;
    if constexpr (!STREAM)
        wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wav + (int64_t)b * p.wav_bs), 0, (LENS ? nsv : p.samples) * 4, 0x00020000);
    cf *z = zb + wave * ZN;

    // positions (padded) of this lane's butterfly operands in stages 0..3 and of its split-step reads
    int p0[4], p1[4], p2[4], p2w[4], p3[4], ps[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        p0[q] = zp(lane + 64 * q);
        p1[q] = zp(64 * (lane >> 4) + (lane & 15) + 16 * q);
        p2[q] = zp(16 * (lane >> 2) + (lane & 3) + 4 * q);
        p2w[q] = zq(16 * (lane >> 2) + (lane & 3) + 4 * q);
        p3[q] = zq(4 * lane + q);
        ps[q] = zq(4 * r3 + q);
    }
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    // frame t covers samples t*hop - 256 .. +255 (center=True); outside [0, samples) the buffer load returns 0.
    // The 8-byte load never straddles the start: t*hop - 256 and 2m are even.
    auto fetch = [&](int t, u32x2(&raw)[4]) {
        const int s0 = t * p.hop - NH;
        if constexpr (STREAM) {
            // 4-byte loads: a chunk boundary at an odd sample leaves no 8-byte alignment to rely on.  Frames past the launch's
            // last are not fetched (their samples may not have arrived)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int s = s0 + 2 * (lane + 64 * q);
                raw[q] = t < T ? u32x2{sample(s), sample(s + 1)} : u32x2{0u, 0u};
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) raw[q] = __builtin_amdgcn_raw_buffer_load_b64(wr, (s0 + 2 * (lane + 64 * q)) * 4, 0, 0);
        }
    };
    u32x2 raw[4], nxt[4];
    fetch(t0 + wave * (FT / 4), raw);
    for (int fi = 0; fi < FT / 4; ++fi) {
        const int j = wave * (FT / 4) + fi, t = t0 + j;           // frame (wave-uniform)
        if (fi + 1 < FT / 4) fetch(t + 1, nxt);                   // next frame's samples arrive under this frame's FFT
        if (t < T) {
            cf a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = cf{__uint_as_float(raw[q][0]) * win[q].x, __uint_as_float(raw[q][1]) * win[q].y};
            // stage 0 (L = 256): positions lane + 64 q
            bfly4(a[0], a[1], a[2], a[3]);
            z[p0[0]] = a[0];
            z[p0[1]] = cmul(a[1], w0[0]);
            z[p0[2]] = cmul(a[2], w0[1]);
            z[p0[3]] = cmul(a[3], w0[2]);
            // stage 1 (L = 64): block = lane / 16, j = lane % 16
            a[0] = z[p1[0]]; a[1] = z[p1[1]]; a[2] = z[p1[2]]; a[3] = z[p1[3]];
            bfly4(a[0], a[1], a[2], a[3]);
            z[p1[0]] = a[0]; z[p1[1]] = cmul(a[1], w1[0]); z[p1[2]] = cmul(a[2], w1[1]); z[p1[3]] = cmul(a[3], w1[2]);
            // stage 2 (L = 16): block = lane / 4, j = lane % 4
            a[0] = z[p2[0]]; a[1] = z[p2[1]]; a[2] = z[p2[2]]; a[3] = z[p2[3]];
            bfly4(a[0], a[1], a[2], a[3]);
            z[p2w[0]] = a[0]; z[p2w[1]] = cmul(a[1], w2[0]); z[p2w[2]] = cmul(a[2], w2[1]); z[p2w[3]] = cmul(a[3], w2[2]);
            // stage 3 (L = 4): positions 4 lane .. 4 lane + 3, no twiddles
            a[0] = z[p3[0]]; a[1] = z[p3[1]]; a[2] = z[p3[2]]; a[3] = z[p3[3]];
            bfly4(a[0], a[1], a[2], a[3]);
            z[p3[0]] = a[0]; z[p3[1]] = a[1]; z[p3[2]] = a[2]; z[p3[3]] = a[3];
            // split step: X[k] = E + (-i) W_512^k O,  E = (Z[k] + conj Z[N-k]) / 2,  O = (Z[k] - conj Z[N-k]) / 2
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const cf A = z[ps[i]], Bc = z[ppos[i]];
                const cf E = {0.5f * (A.re + Bc.re), 0.5f * (A.im - Bc.im)};
                const cf O = {0.5f * (A.re - Bc.re), 0.5f * (A.im + Bc.im)};
                const cf X = E + mul_mi(cmul(O, wk[i]));
                pw[(lane + 64 * i) * PWS + j] = fmaf(X.re, X.re, X.im * X.im);
            }
            if (lane == 0) {                                      // Nyquist bin: X[256] = Re Z[0] - Im Z[0]
                const cf A = z[0];
                const float x = A.re - A.im;
                pw[NH * PWS + j] = x * x;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[q] = nxt[q];
    }
    __syncthreads();

    // ---- mel projection + dB.  thread = (mel band, frame) with the FRAME fastest: a wave's 64 lanes are 4 bands x 16
    // frames, so a power-tile read is 16 consecutive floats per band (at most 2-way bank conflicts between the two bands of a
    // 32-lane group; with the band fastest, bands whose first bins are 8 apart met on 4 banks: 8-way), the weight read is
    // a broadcast per band, and the loop length is that of 4 neighbouring bands, not of the 64 widest.
    // dB values pass through LDS so that the global stores are whole 320-byte frame rows.
    float local_max = -INFINITY;
    static_assert(FT == 16, "the mel stage maps 16 frames to 16 lanes");
    float *dbt = reinterpret_cast<float *>(zb);                  // [FT][M] dB tile; the FFT buffers are dead (barrier above)
    for (int o = tid; o < FT * M; o += 256) {
        const int m = o >> 4, j = o & 15;
        float acc = 0.f;
        const int lo = band[m], hi = band[M + m];
        if (bw_lds) {                                             // (two loops: one address space per pointer)
            const float *wm = bw + band[2 * M + m] - lo;
            for (int f = lo; f < hi; ++f) acc = fmaf(pw[f * PWS + j], wm[f], acc);
        } else {
            const float *wm = p.band_w + band[2 * M + m] - lo;
            for (int f = lo; f < hi; ++f) acc = fmaf(pw[f * PWS + j], wm[f], acc);
        }
        const float db = fmaxf(10.f * log10f(fmaxf(acc, p.amin)), floor_db);
        dbt[j * M + m] = db;
        if (t0 + j < T) local_max = fmaxf(local_max, db);
    }
    __syncthreads();
    {
        const int nrow = min(FT, T - t0);                         // rows t0 .. t0 + nrow - 1 are contiguous in db: one linear copy
        float *dst;
        if constexpr (STREAM) dst = p.db + ((int64_t)b * pk.nf + (t0 - p.f0)) * M;
        else dst = p.db + ((int64_t)b * (LENS ? p.frames : T) + t0) * M;
        for (int i = tid; i < nrow * M; i += 256) dst[i] = dbt[i];
    }
    if constexpr (STREAM) {
        // the causal clamp wants the maximum of every frame, not of the tile: wave w reduces the rows 4 w .. 4 w + 3 of the dB tile
        for (int j = wave * (FT / 4); j < (wave + 1) * (FT / 4); ++j) {
            float mx = -INFINITY;
            for (int m = lane; m < M; m += 64) mx = fmaxf(mx, dbt[j * M + m]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            if (lane == 0 && t0 + j < T) p.fmax[(int64_t)b * pk.nf + (t0 - p.f0) + j] = mx;
        }
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) local_max = fmaxf(local_max, __shfl_xor(local_max, off, 64));
    __syncthreads();
    if (lane == 0) pw[wave] = local_max;
    __syncthreads();
    if constexpr (!STREAM)
        if (tid == 0) p.umax_part[(int64_t)b * gridDim.x + blockIdx.x] = fmaxf(fmaxf(pw[0], pw[1]), fmaxf(pw[2], pw[3]));
}

// cm_fbank_finish / cm_fbank_finish_lens, grid (chunks, batch): a workgroup first reduces its utterance's tile maxima (when umax_part is
// given; cm_fbank_mel_db without it left the maximum in umax), then clamps and normalises its slice of the utterance.  ARGS =
// fb_lens_args: the utterance's own frame count -- the maximum over the tiles that hold its frames [0, T_b) (fbank_wav_kernel<false,
// fb_lens_args> kept the frames behind them out of the last one), the clamp and the normalisation on those frames only.
template <typename ARGS>
__global__ __launch_bounds__(256) void fbank_finish_kernel(const ARGS p, int ntiles) {
    constexpr bool LENS = std::is_same<ARGS, fb_lens_args>::value;
    __shared__ float red[4];
    const int b = blockIdx.y;
    int Tb = p.frames, nt = ntiles;                               // the utterance's frames and the tiles that hold them
    if constexpr (LENS) {
        const int nsv = min(max(p.nsamp[b], 0), p.samples);
        Tb = nsv > 0 ? 1 + nsv / p.hop : 0;
        if (Tb == 0) return;
        nt = (Tb + FT - 1) / FT;
    }
    float um;
    if (LENS || p.umax_part) {
        float mx = -INFINITY;
        for (int i = threadIdx.x; i < nt; i += blockDim.x) mx = fmaxf(mx, p.umax_part[(int64_t)b * ntiles + i]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        um = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (blockIdx.x == 0 && threadIdx.x == 0) p.umax[b] = um;
    } else {
        um = p.umax[b];
    }
    const float floor_db = um - p.top_db;
    const int64_t per_utt = (int64_t)Tb * p.n_mels;
    float *db = p.db + (int64_t)b * p.frames * p.n_mels;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per_utt; i += (int64_t)gridDim.x * blockDim.x) {
        float v = fmaxf(db[i], floor_db);
        if (p.mean) { const int m = (int)(i % p.n_mels); v = (v - p.mean[m]) / p.std[m]; }
        db[i] = v;
    }
}

// cm_fbank_finish_stream: one workgroup per stream.  Thread = (frame group g, mel bin m): every thread carries the prefix maximum
// over all frames (nf broadcast loads) and clamps / normalises the frames of its group; no atomics, no second pass.
__global__ __launch_bounds__(256) void fbank_finish_stream_kernel(const cm_fbank_stream_args p) {
    const int b = blockIdx.x, M = p.n_mels, nf = p.nf;
    const int G = 256 / M, g = threadIdx.x / M, m = threadIdx.x - g * M;
    float run = p.umax[b];
    __syncthreads();                                              // everyone holds the carried maximum before thread 0 replaces it
    const float *fm = p.fmax + (int64_t)b * nf;
    float *db = p.db + (int64_t)b * nf * M;
    const float mean = p.mean && g < G ? p.mean[m] : 0.f, sd = p.mean && g < G ? p.std[m] : 1.f;
    for (int i = 0; i < nf; ++i) {
        run = fmaxf(run, fm[i]);
        if (g < G && i % G == g) {
            float v = fmaxf(db[(int64_t)i * M + m], run - p.top_db);
            if (p.mean) v = (v - mean) / sd;
            db[(int64_t)i * M + m] = v;
            if (p.feat_hist_out && i >= nf - FH) p.feat_hist_out[((int64_t)b * FH + (i - (nf - FH))) * M + m] = v;
        }
    }
    if (p.feat_hist_out && g < G)                                 // rows the call did not fill: the old history moved up, zeros in front of frame 0
        for (int j = g; j < FH - nf; j += G)
            p.feat_hist_out[((int64_t)b * FH + j) * M + m] = (p.feat_hist && p.f0 + nf - FH + j >= 0) ? p.feat_hist[((int64_t)b * FH + j + nf) * M + m] : 0.f;
    if (threadIdx.x == 0) p.umax[b] = run;
}

// cm_fbank_finish_stream_slots: the same per stream with f0 and nf from the plan table; db and fmax rows are pk.nf (the maximum) apart.
// A slot without frames still rolls its feature history: the loop below then copies feat_hist to feat_hist_out.
__global__ __launch_bounds__(256) void fbank_finish_slots_kernel(const fb_slot_args pk) {
    const int b = blockIdx.x;
    const fb_slot_args p = fb_view(pk, b);
    const int M = p.n_mels, nf = p.nf;
    const int G = 256 / M, g = threadIdx.x / M, m = threadIdx.x - g * M;
    float run = p.umax[b];
    __syncthreads();
    const float *fm = p.fmax + (int64_t)b * pk.nf;
    float *db = p.db + (int64_t)b * pk.nf * M;
    const float mean = p.mean && g < G ? p.mean[m] : 0.f, sd = p.mean && g < G ? p.std[m] : 1.f;
    for (int i = 0; i < nf; ++i) {
        run = fmaxf(run, fm[i]);
        if (g < G && i % G == g) {
            float v = fmaxf(db[(int64_t)i * M + m], run - p.top_db);
            if (p.mean) v = (v - mean) / sd;
            db[(int64_t)i * M + m] = v;
            if (p.feat_hist_out && i >= nf - FH) p.feat_hist_out[((int64_t)b * FH + (i - (nf - FH))) * M + m] = v;
        }
    }
    if (p.feat_hist_out && g < G)
        for (int j = g; j < FH - nf; j += G)
            p.feat_hist_out[((int64_t)b * FH + j) * M + m] = (p.feat_hist && p.f0 + nf - FH + j >= 0) ? p.feat_hist[((int64_t)b * FH + j + nf) * M + m] : 0.f;
    if (threadIdx.x == 0) p.umax[b] = run;
}

// ---- host side.  `sym` is an entry point's symbol, `who` = sym + 3 the name its messages begin with (no "cm_").

size_t fbank_wav_smem(int n_mels) {                               // power tile, band table, band weights, four FFT buffers
    return (size_t)(NH + 1) * PWS * 4 + (size_t)(3 * n_mels + 1) * 4 + (size_t)BWCAP * 4 + (size_t)4 * ZN * 8 + 4;
}
float fbank_floor_db(float amin) { return (float)(10.0 * log10((double)amin)); }

template <typename ARGS>
int fbank_wav_launch(const ARGS &k, const char *sym) {
    dim3 grid((k.frames + FT - 1) / FT, k.batch);
    hipLaunchKernelGGL((fbank_wav_kernel<false, ARGS>), grid, dim3(256), fbank_wav_smem(k.n_mels), reinterpret_cast<hipStream_t>(k.stream), k,
                       fbank_floor_db(k.amin));
    return cm_launch_status(sym);
}

// cm_fbank_wav (nsamp == NULL) and cm_fbank_wav_lens: one set of checks, under the name of the form without lengths
int fbank_wav_entry(const cm_fbank_args &a, const int32_t *nsamp) {
    CM_REQUIRE(a.batch > 0 && a.frames > 0 && a.n_mels > 0 && a.wav && a.window && a.twiddle && a.db && a.umax_part && a.band_lo &&
                   a.band_hi && a.band_off && a.band_w, CM_EINVAL, "fbank_wav: bad sizes or NULL tensor");
    CM_REQUIRE(a.n_fft == NF && a.n_freq == NH + 1, CM_EUNSUPPORTED, "fbank_wav: n_fft %d unsupported (512 only)", a.n_fft);
    CM_REQUIRE(a.hop > 0 && a.hop % 2 == 0 && a.samples > 0 && a.samples < (1 << 29) && a.wav_bs % 2 == 0 && cm_aligned(a.wav, 8) &&
                   cm_aligned(a.window, 8) && cm_aligned(a.twiddle, 8), CM_EALIGN,
               "fbank_wav: hop and the batch stride must be even, wav / window / twiddle 8-byte aligned");
    CM_REQUIRE(a.frames == 1 + a.samples / a.hop, CM_EINVAL, "fbank_wav: frames must be 1 + samples / hop (center=True)");
    CM_REQUIRE(a.batch <= 65535 && a.n_mels <= 128, CM_EUNSUPPORTED, "fbank_wav: batch / n_mels too large");
    if (!nsamp) return fbank_wav_launch(a, "cm_fbank_wav");
    fb_lens_args k{};
    static_cast<cm_fbank_args &>(k) = a;
    k.nsamp = nsamp;
    return fbank_wav_launch(k, "cm_fbank_wav_lens");
}

// cm_fbank_finish (nsamp == NULL; umax_part optional) and cm_fbank_finish_lens (umax_part required, and the frame count it is read by)
int fbank_finish_entry(const cm_fbank_args &a, const int32_t *nsamp, const char *sym) {
    const char *who = sym + 3;
    CM_REQUIRE(a.batch > 0 && a.frames > 0 && a.n_mels > 0 && a.db && a.umax && (!nsamp || a.umax_part), CM_EINVAL, "%s: bad sizes or NULL tensor%s",
               who, nsamp ? " (umax_part included)" : "");
    CM_REQUIRE(!nsamp || (a.hop > 0 && a.samples > 0 && a.frames == 1 + a.samples / a.hop), CM_EINVAL, "%s: frames must be 1 + samples / hop", who);
    CM_REQUIRE(!a.mean || a.std, CM_EINVAL, "%s: mean without std", who);
    CM_REQUIRE(a.batch <= 65535, CM_EINVAL, "%s: batch %d exceeds the grid limit", who, a.batch);
    const int64_t per_utt = (int64_t)a.frames * a.n_mels;
    int64_t chunks = (per_utt + 256 * 8 - 1) / (256 * 8);
    if (chunks > 256) chunks = 256;
    const dim3 grid((unsigned)chunks, a.batch);
    const int ntiles = (a.frames + FT - 1) / FT;
    if (nsamp) {
        fb_lens_args k{};
        static_cast<cm_fbank_args &>(k) = a;
        k.nsamp = nsamp;
        hipLaunchKernelGGL(fbank_finish_kernel<fb_lens_args>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(a.stream), k, ntiles);
    } else {
        hipLaunchKernelGGL(fbank_finish_kernel<cm_fbank_args>, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(a.stream), a, ntiles);
    }
    return cm_launch_status(sym);
}

bool overlap(const void *a, const void *b, size_t bytes) {
    const char *x = static_cast<const char *>(a), *y = static_cast<const char *>(b);
    return x < y + bytes && y < x + bytes;
}

// The checks on one stream's counts that the stream entry points share (cm_fbank_finish_stream reads no sample: the sample counts are
// cm_fbank_wav_stream's): the struct's own scalars, or a row of the per-slot plan in their place.  Nothing is launched before they pass.
int fbank_stream_check(const cm_fbank_stream_args &a, const char *who, bool samples) {
    CM_REQUIRE(a.batch > 0 && a.n_mels > 0 && a.nf >= 0 && a.f0 >= 0, CM_EINVAL, "%s: bad sizes", who);
    CM_REQUIRE(a.n_fft == NF, CM_EUNSUPPORTED, "%s: n_fft %d unsupported (512 only)", who, a.n_fft);
    CM_REQUIRE(a.n_mels <= 128 && a.batch <= 65535, CM_EUNSUPPORTED, "%s: batch / n_mels too large", who);
    if (!samples) return CM_OK;
    CM_REQUIRE(a.n >= 0 && a.consumed >= 0 && a.hop > 0, CM_EINVAL, "%s: bad sample counts", who);
    CM_REQUIRE(a.hop % 2 == 0, CM_EUNSUPPORTED, "%s: hop must be even", who);
    CM_REQUIRE((int64_t)a.consumed + a.n < (1 << 30) && (a.total < 0 || a.total == a.consumed + a.n), CM_EINVAL,
               "%s: total must be -1 or consumed + n, below 2^30", who);
    // every frame of the launch lies inside what has arrived: its last sample index is below consumed + n unless the utterance ends here
    CM_REQUIRE(a.nf == 0 || a.total >= 0 || (int64_t)a.hop * (a.f0 + a.nf - 1) + NH <= (int64_t)a.consumed + a.n, CM_EINVAL,
               "%s: frame %d needs samples that have not arrived", who, a.f0 + a.nf - 1);
    CM_REQUIRE(a.nf == 0 || (int64_t)a.hop * a.f0 - NH >= (int64_t)a.consumed - HS, CM_EINVAL, "%s: frame %d reaches behind the history", who, a.f0);
    return CM_OK;
}

// What the per-slot entry points ask first: the plan's two copies, then every slot's counts through fbank_stream_check and under the
// struct's maxima
int fbank_slots_check(const cm_fbank_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev, const char *who, bool samples) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "%s: args is NULL", who);
    CM_REQUIRE(plan_host != nullptr && plan_dev != nullptr, CM_EINVAL, "%s: plan is NULL (host copy and device copy)", who);
    CM_REQUIRE(cm_aligned(plan_host, 4) && cm_aligned(plan_dev, 4), CM_EALIGN, "%s: plan must be 4-byte aligned", who);
    const cm_fbank_stream_args &a = *args;
    CM_REQUIRE(a.batch > 0 && (!samples || (a.n >= 0 && a.nf >= 0)), CM_EINVAL, "%s: bad sizes", who);
    for (int b = 0; b < a.batch; ++b) {
        const cm_fbank_stream_args q = fb_row_view(a, plan_host, b);
        if (int rc = fbank_stream_check(q, who, samples)) return rc;
        if (samples) CM_REQUIRE(q.n <= a.n && q.nf <= a.nf, CM_EINVAL, "%s: slot %d has n %d / nf %d above the maxima %d / %d", who, b, q.n, q.nf, a.n, a.nf);
        else CM_REQUIRE(q.nf <= a.nf, CM_EINVAL, "%s: slot %d has nf %d above the maximum %d", who, b, q.nf, a.nf);
    }
    return CM_OK;
}

// cm_fbank_wav_stream and its per-slot form behind their own checks of the counts
template <typename ARGS>
int fbank_wav_stream_run(const ARGS &k, const char *sym) {
    const cm_fbank_stream_args &a = k;
    const char *who = sym + 3;
    CM_REQUIRE(a.hist && a.hist_out && (a.n == 0 || a.chunk), CM_EINVAL, "%s: NULL chunk / hist / hist_out", who);
    CM_REQUIRE(!overlap(a.hist, a.hist_out, (size_t)a.batch * HS * 4), CM_EINVAL, "%s: hist_out overlaps hist", who);
    CM_REQUIRE(a.nf == 0 || (a.window && a.twiddle && a.db && a.fmax && a.band_lo && a.band_hi && a.band_off && a.band_w), CM_EINVAL,
               "%s: NULL tensor", who);
    CM_REQUIRE(a.nf == 0 || (cm_aligned(a.window, 8) && cm_aligned(a.twiddle, 8)), CM_EALIGN, "%s: window / twiddle must be 8-byte aligned", who);
    dim3 grid(a.nf ? (a.nf + FT - 1) / FT : 1, a.batch);
    hipLaunchKernelGGL((fbank_wav_kernel<true, ARGS>), grid, dim3(256), fbank_wav_smem(a.n_mels), reinterpret_cast<hipStream_t>(a.stream), k,
                       fbank_floor_db(a.amin));
    return cm_launch_status(sym);
}

// ... and cm_fbank_finish_stream and its per-slot form
template <typename ARGS>
int fbank_finish_stream_run(const ARGS &k, const char *sym) {
    const cm_fbank_stream_args &a = k;
    const char *who = sym + 3;
    CM_REQUIRE(a.nf > 0 && a.db && a.fmax && a.umax, CM_EINVAL, "%s: no frames or NULL db / fmax / umax", who);
    CM_REQUIRE(!a.mean == !a.std, CM_EINVAL, "%s: mean and std go together", who);
    CM_REQUIRE(!a.feat_hist_out || !a.feat_hist || !overlap(a.feat_hist, a.feat_hist_out, (size_t)a.batch * FH * a.n_mels * 4), CM_EINVAL,
               "%s: feat_hist_out overlaps feat_hist", who);
    CM_REQUIRE(a.feat_hist_out || !a.feat_hist, CM_EINVAL, "%s: feat_hist without feat_hist_out", who);
    if constexpr (std::is_same<ARGS, fb_slot_args>::value)
        hipLaunchKernelGGL(fbank_finish_slots_kernel, dim3(a.batch), dim3(256), 0, reinterpret_cast<hipStream_t>(a.stream), k);
    else
        hipLaunchKernelGGL(fbank_finish_stream_kernel, dim3(a.batch), dim3(256), 0, reinterpret_cast<hipStream_t>(a.stream), k);
    return cm_launch_status(sym);
}

fb_slot_args fb_with_plan(const cm_fbank_stream_args &a, const int32_t *plan_dev) {
    fb_slot_args k{};
    static_cast<cm_fbank_stream_args &>(k) = a;
    k.plan = plan_dev;
    return k;
}

}  // namespace

extern "C" int cm_fbank_wav(const cm_fbank_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_wav: args is NULL");
    return fbank_wav_entry(*args, nullptr);
}

extern "C" int cm_fbank_wav_lens(const cm_fbank_args *args, const int32_t *n_samples) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_wav_lens: args is NULL");
    CM_REQUIRE(n_samples != nullptr, CM_EINVAL, "fbank_wav_lens: n_samples is NULL (cm_fbank_wav is the form without lengths)");
    CM_REQUIRE(cm_aligned(n_samples, 4), CM_EALIGN, "fbank_wav_lens: n_samples must be 4-byte aligned");
    return fbank_wav_entry(*args, n_samples);
}

extern "C" int cm_fbank_finish(const cm_fbank_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_finish: args is NULL");
    return fbank_finish_entry(*args, nullptr, "cm_fbank_finish");
}

extern "C" int cm_fbank_finish_lens(const cm_fbank_args *args, const int32_t *n_samples) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_finish_lens: args is NULL");
    CM_REQUIRE(n_samples != nullptr, CM_EINVAL, "fbank_finish_lens: n_samples is NULL (cm_fbank_finish is the form without lengths)");
    CM_REQUIRE(cm_aligned(n_samples, 4), CM_EALIGN, "fbank_finish_lens: n_samples must be 4-byte aligned");
    return fbank_finish_entry(*args, n_samples, "cm_fbank_finish_lens");
}

extern "C" int cm_fbank_wav_stream(const cm_fbank_stream_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_wav_stream: args is NULL");
    if (int rc = fbank_stream_check(*args, "fbank_wav_stream", true)) return rc;
    return fbank_wav_stream_run(*args, "cm_fbank_wav_stream");
}

extern "C" int cm_fbank_finish_stream(const cm_fbank_stream_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "fbank_finish_stream: args is NULL");
    if (int rc = fbank_stream_check(*args, "fbank_finish_stream", false)) return rc;
    return fbank_finish_stream_run(*args, "cm_fbank_finish_stream");
}

extern "C" int cm_fbank_wav_stream_slots(const cm_fbank_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev) {
    if (int rc = fbank_slots_check(args, plan_host, plan_dev, "fbank_wav_stream_slots", true)) return rc;
    return fbank_wav_stream_run(fb_with_plan(*args, plan_dev), "cm_fbank_wav_stream_slots");
}

extern "C" int cm_fbank_finish_stream_slots(const cm_fbank_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev) {
    if (int rc = fbank_slots_check(args, plan_host, plan_dev, "fbank_finish_stream_slots", false)) return rc;
    return fbank_finish_stream_run(fb_with_plan(*args, plan_dev), "cm_fbank_finish_stream_slots");
}
