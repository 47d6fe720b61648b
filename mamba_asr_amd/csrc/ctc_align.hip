// ctc_align.hip — CTC forced alignment (contract: cm_ctc_align; mamba_asr_amd/ctc_decode.py): the best path of a
// known label sequence through the CTC trellis.  On the extended sequence e (blank, y0, blank, ..., y(L-1), blank), E = 2 L + 1:
//   D_0(s) = x_0(s) for s in {0, 1};  D_t(s) = x_t(s) + max(D_{t-1}(s), D_{t-1}(s-1), D_{t-1}(s-2) if s odd, s >= 3, e[s] != e[s-2])
// with x_t(s) = (double) lp[t][e[s]], strict compares in the order (0, 1, 2) so that ties keep the smaller move, the end at E-1 unless
// E-2 is strictly better, and a backtrace s_{t-1} = s_t - move_t(s_t).  Every operation is an fp64 add or compare: the bits are those
// of tests/ctc_align_ref.py whatever -ffp-contract does.
// One workgroup per utterance, three phases in one launch:
//   forward    thread j owns the pair (blank 2 j, label 2 j + 1) in registers; from outside it needs D_{t-1}(2 j - 1) alone, one fp64
//              through LDS per step, double-buffered, one LDS-only barrier per step.  No score table: the moves go to the workspace at
//              2 bits per cell, each thread's two states of 16 steps in one 8-byte word, stored coalesced.
//   backtrace  wave 0.  Over a 16-step block the state falls by at most 32, i.e. 16 threads' words: the 64 lanes load the words below
//              the block's top state in one coalesced load, issued one block ahead, and the 16 steps run on scalar registers
//              (v_readlane of the word that holds the state) -- about n / 16 dependent global loads instead of n.
//   spans      starts / ends from the states in parallel over t; label_logp by one thread per label over its own frames in order.
#include "cm_common.h"

namespace {

constexpr double NEG_INF = -__builtin_huge_val();
constexpr int PF = 8;                     // steps the gathers run ahead
constexpr int BLK = 16;                   // steps per move word
constexpr int OOB = 0x7fffffff;           // a buffer offset outside every descriptor: loads return 0, stores are dropped

template <bool BF16> struct lp_io;
template <> struct lp_io<false> {
    typedef uint32_t raw;
    static __device__ __forceinline__ raw load(const __amdgpu_buffer_rsrc_t r, int vo, int so) { return __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0); }
    static __device__ __forceinline__ float value(raw v) { return __uint_as_float(v); }
};
template <> struct lp_io<true> {
    typedef unsigned short raw;
    static __device__ __forceinline__ raw load(const __amdgpu_buffer_rsrc_t r, int vo, int so) { return __builtin_amdgcn_raw_buffer_load_b16(r, vo, so, 0); }
    static __device__ __forceinline__ float value(raw v) { return __uint_as_float((uint32_t)v << 16); }
};

// words of moves per 16-step block of one utterance: (2 S + 1 rounded up to 64) / 2 >= S + 1 threads
__host__ __device__ inline int align_words(int S) { return ((2 * S + 1 + 63) / 64) * 32; }

// grid (batch); block = S + 1 rounded up to 64 threads (<= 1024)
template <bool BF16> __global__ __launch_bounds__(1024) void ctc_align_kernel(const cm_ctc_align_args p) {
    typedef lp_io<BF16> IO;
    constexpr int ES = BF16 ? 2 : 4;
    __shared__ double nbr[2][1024 + 1];                              // D(2 j + 1) of thread j at [j + 1]; [0] = -inf
    __shared__ int sh_end, sh_status;
    const int b = blockIdx.x, j = threadIdx.x, nthr = blockDim.x, lane = j & 63;
    const int n = max(min(p.input_lengths[b], p.T), 0), L = max(min(p.target_lengths[b], p.S), 0);
    const int64_t row = p.rows ? (int64_t)p.rows[b] : (int64_t)b;
    const bool row_ok = row >= 0 && row < p.lp_rows;
    int32_t *states = p.states + (int64_t)b * p.T;
    int32_t *starts = p.starts + (int64_t)b * p.S, *ends = p.ends + (int64_t)b * p.S;
    double *label_logp = p.label_logp + (int64_t)b * p.S;
    const bool has_lab = j < L;                                      // state 2 j + 1 exists; state 2 j exists when j <= L
    const int lab = has_lab ? (int)min(max(p.targets[(int64_t)b * p.S + j], (int64_t)-1), (int64_t)p.V) : -1;
    const bool lab_ok = has_lab && lab >= 0 && lab < p.V;            // an id outside the vocabulary scores -inf

    // ---- forward ----
    const int W = align_words(p.S), nblk = (n + BLK - 1) / BLK;
    uint64_t *moves = reinterpret_cast<uint64_t *>(p.workspace) + (int64_t)b * ((p.T + BLK - 1) / BLK) * W;
    double d0 = NEG_INF, d1 = NEG_INF;                               // D_{t-1}(2 j), D_{t-1}(2 j + 1)
    bool saw_nan = false;
    if (n > 0 && row_ok) {
        const char *lp = reinterpret_cast<const char *>(p.log_probs) + row * p.lp_bs * ES;
        // wave-uniform descriptors: the utterance's frames < n, the utterance's move words
        const __amdgpu_buffer_rsrc_t rlp = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(lp), 0, (int)(((int64_t)(n - 1) * p.lp_ts + p.V) * ES), 0x00020000);
        const __amdgpu_buffer_rsrc_t rmv = __builtin_amdgcn_make_buffer_rsrc(moves, 0, (int)((int64_t)nblk * W * 8), 0x00020000);
        const int vo_blank = j <= L ? p.blank * ES : OOB, vo_lab = lab_ok ? lab * ES : OOB, vo_mv = j <= L ? j * 8 : OOB;
        const int ts = (int)p.lp_ts * ES;
        // the two gathers of a step come from a fresh row every step: requested PF steps ahead, and the loop body is branch-free (dead
        // lanes and the steps past n address outside the descriptors) so that the compiler counts the outstanding loads exactly --
        // csrc/ctc.hip's ctc_alpha_beta_kernel says what the alternatives cost
        auto x_at = [&](int t, int vo) { const bool in = t < n; return IO::load(rlp, in ? vo : OOB, in ? t * ts : 0); };
        const int lab_below = (j >= 1 && j - 1 < L) ? (int)min(max(p.targets[(int64_t)b * p.S + j - 1], (int64_t)-1), (int64_t)p.V) : -1;   // y(j-1)
        const bool skip_ok = has_lab && j >= 1 && lab != lab_below;
        typename IO::raw q0[PF], q1[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) q0[i] = x_at(i, vo_blank), q1[i] = x_at(i, vo_lab);
        // D_{-1}: -0.0 at state 0 (x + -0.0 is x, bit for bit), so that step 0 is the general step: D_0(0) = x_0(0), D_0(1) = x_0(1)
        if (j == 0) d0 = -0.0;
        nbr[0][j + 1] = NEG_INF, nbr[1][j + 1] = NEG_INF;
        if (j == 0) nbr[0][0] = NEG_INF, nbr[1][0] = NEG_INF;
        __syncthreads();
        for (int blk = 0; blk < nblk; ++blk) {
            uint64_t word = 0;
#pragma unroll
            for (int i = 0; i < BLK; ++i) {
                const int t = blk * BLK + i;
                const bool in = t < n;                               // uniform
                const float f0 = IO::value(q0[i % PF]), f1 = IO::value(q1[i % PF]);
                q0[i % PF] = x_at(t + PF, vo_blank), q1[i % PF] = x_at(t + PF, vo_lab);
                const double x0 = (double)f0, x1 = lab_ok ? (double)f1 : NEG_INF;
                saw_nan = saw_nan || (in && ((j <= L && x0 != x0) || (has_lab && x1 != x1)));
                const double below = nbr[(t + 1) & 1][j];            // D_{t-1}(2 j - 1)
                double best0 = d0, best1 = d1;
                uint32_t m0 = 0, m1 = 0;
                if (below > best0) best0 = below, m0 = 1;
                if (d0 > best1) best1 = d0, m1 = 1;
                if (skip_ok && below > best1) best1 = below, m1 = 2;
                const double n0 = j <= L ? best0 + x0 : NEG_INF, n1 = has_lab ? best1 + x1 : NEG_INF;
                d0 = in ? n0 : d0, d1 = in ? n1 : d1;
                word |= (uint64_t)(m0 | (m1 << 2)) << (4 * i);
                nbr[t & 1][j + 1] = d1;
                cm_lds_barrier();                                    // LDS only: __syncthreads() would wait for the prefetched gathers too
            }
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)word, (uint32_t)(word >> 32)}, rmv, vo_mv, blk * W * 8, 0);
        }
    }

    // ---- end state, score, status ----
    __syncthreads();
    nbr[0][j + 1] = d1;
    const int any_nan = __syncthreads_or(saw_nan ? 1 : 0);               // (a barrier: the stores of the moves and of nbr[0] are visible)
    if (j == L) {
        int end = 2 * L, status = 0;
        double score = d0;
        if (n == 0) score = L == 0 ? 0.0 : NEG_INF;
        else if (L >= 1 && nbr[0][L] > d0) end = 2 * L - 1, score = nbr[0][L];
        if (any_nan || score != score) status = 2, score = __builtin_nan("");
        else if (score == NEG_INF) status = 1;
        p.score[b] = score;
        p.status[b] = status;
        sh_end = end, sh_status = status;
    }
    __syncthreads();
    const int status = sh_status;
    for (int t = (status == 0 ? n : 0) + j; t < p.T; t += nthr) states[t] = -1;
    for (int k = j; k < p.S; k += nthr) starts[k] = -1, ends[k] = -1, label_logp[k] = 0.0;      // labels < L: overwritten below
    if (status != 0 || n == 0) return;

    // ---- backtrace: wave 0 ----
    if (j < 64) {
        int s = __builtin_amdgcn_readfirstlane(sh_end);
        auto window = [&](int blk, int top) -> uint64_t {            // lane l: the word of thread top - l of block blk
            const int jj = top - lane;
            return jj >= 0 ? moves[(int64_t)blk * W + jj] : 0;
        };
        int base = s >> 1;
        uint64_t w = window(nblk - 1, base);
        for (int blk = nblk - 1; blk >= 0; --blk) {
            const int nbase = s >> 1;
            // the block below ends at most 32 states, 16 words, under this block's top: lanes 0 .. 32 of a window cover both
            const uint64_t wn = blk > 0 ? window(blk - 1, nbase) : 0;
            const uint32_t wlo = (uint32_t)w, whi = (uint32_t)(w >> 32);
            int mine = -1;
            for (int i = min(BLK - 1, n - 1 - blk * BLK); i >= 0; --i) {
                mine = lane == i ? s : mine;
                const int idx = (base - (s >> 1)) & 63;
                const uint32_t half = i < 8 ? (uint32_t)__builtin_amdgcn_readlane((int)wlo, idx) : (uint32_t)__builtin_amdgcn_readlane((int)whi, idx);
                const int mv = (half >> (4 * (i & 7) + 2 * (s & 1))) & 3;
                s = __builtin_amdgcn_readfirstlane(max(s - mv, 0));
            }
            const int t = blk * BLK + lane;
            if (lane < BLK && t < n) states[t] = mine;
            base = nbase, w = wn;
        }
    }
    __syncthreads();

    // ---- spans, in parallel over t ----
    for (int t = j; t < n; t += nthr) {
        const int s = states[t];
        if (s & 1) {
            if (t == 0 || states[t - 1] != s) starts[s >> 1] = t;
            if (t == n - 1 || states[t + 1] != s) ends[s >> 1] = t + 1;
        }
    }
    __syncthreads();

    // ---- label_logp: one thread per label, its own frames in increasing t ----
    const int t0 = has_lab ? starts[j] : -1, t1 = has_lab ? ends[j] : -1;
    if (lab_ok && t0 >= 0 && t1 <= n) {
        const char *lp = reinterpret_cast<const char *>(p.log_probs) + (row * p.lp_bs + lab) * ES;
        auto x = [&](int t) -> double {
            const char *q = lp + (int64_t)t * p.lp_ts * ES;
            return (double)IO::value(*reinterpret_cast<const typename IO::raw *>(q));
        };
        double acc = x(t0);
        for (int t = t0 + 1; t < t1; ++t) acc += x(t);
        label_logp[j] = acc;
    }
}

int64_t workspace_bytes(int64_t batch, int64_t T, int S) { return batch * ((T + BLK - 1) / BLK) * align_words(S) * 8; }

}  // namespace

extern "C" int64_t cm_ctc_align_workspace_bytes(const cm_ctc_align_args *a) {
    if (a == nullptr || a->batch <= 0 || a->T <= 0 || a->S < 0) return 0;
    return workspace_bytes(a->batch, a->T, a->S);
}

extern "C" int cm_ctc_align(const cm_ctc_align_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_align: args is NULL");
    const cm_ctc_align_args a = *args;
    CM_REQUIRE(a.batch > 0 && a.T > 0 && a.V > 0 && a.S >= 0, CM_EINVAL, "ctc_align: bad sizes batch=%d T=%d V=%d S=%d", a.batch, a.T, a.V, a.S);
    CM_REQUIRE(a.S <= 1023, CM_EUNSUPPORTED, "ctc_align: at most 1023 labels per utterance (got %d)", a.S);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "ctc_align: dtype %d is neither CM_F32 nor CM_BF16", a.dtype);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "ctc_align: blank %d out of range", a.blank);
    const int es = a.dtype == CM_BF16 ? 2 : 4;
    CM_REQUIRE(a.lp_rows > 0 && (a.rows || a.lp_rows >= a.batch), CM_EINVAL, "ctc_align: lp_rows=%lld does not cover the batch", (long long)a.lp_rows);
    CM_REQUIRE(a.lp_ts >= a.V && a.lp_bs >= 0, CM_EINVAL, "ctc_align: bad strides lp_bs=%lld lp_ts=%lld", (long long)a.lp_bs, (long long)a.lp_ts);
    // a row's frames are addressed by 32-bit byte offsets behind one buffer descriptor
    CM_REQUIRE(((int64_t)(a.T - 1) * a.lp_ts + a.V) * es <= 0x7ffffff0ll, CM_EUNSUPPORTED, "ctc_align: one row of log_probs spans more than 2 GiB");
    // S == 0 (every target empty): targets and the per-label outputs are never touched -- an empty tensor has no address
    CM_REQUIRE(a.log_probs && a.input_lengths && a.target_lengths && a.score && a.status && a.states && a.workspace, CM_EINVAL, "ctc_align: NULL tensor");
    CM_REQUIRE((a.targets != nullptr) == (a.S > 0), CM_EINVAL, "ctc_align: targets must be NULL exactly when S == 0");
    CM_REQUIRE(a.S == 0 || (a.starts && a.ends && a.label_logp), CM_EINVAL, "ctc_align: NULL starts / ends / label_logp");
    CM_REQUIRE(cm_aligned(a.log_probs, es) && cm_aligned(a.targets, 8) && cm_aligned(a.input_lengths, 4) && cm_aligned(a.target_lengths, 4) &&
                   cm_aligned(a.rows, 4) && cm_aligned(a.score, 8) && cm_aligned(a.status, 4) && cm_aligned(a.states, 4) && cm_aligned(a.starts, 4) &&
                   cm_aligned(a.ends, 4) && cm_aligned(a.label_logp, 8) && cm_aligned(a.workspace, 16),
               CM_EALIGN, "ctc_align: a tensor is not aligned to its element size (workspace: 16 bytes)");
    const int64_t need = workspace_bytes(a.batch, a.T, a.S);
    CM_REQUIRE(workspace_bytes(1, a.T, a.S) <= 0x7ffffff0ll, CM_EUNSUPPORTED, "ctc_align: the moves of one utterance exceed 2 GiB");
    CM_REQUIRE(a.workspace_bytes >= need, CM_EINVAL, "ctc_align: workspace smaller than cm_ctc_align_workspace_bytes() (%lld < %lld)",
               (long long)a.workspace_bytes, (long long)need);
    hipStream_t st = reinterpret_cast<hipStream_t>(a.stream);
    const int threads = (a.S + 1 + 63) / 64 * 64;
    if (a.dtype == CM_BF16) hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(a.batch), dim3(threads), 0, st, a);
    else hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(a.batch), dim3(threads), 0, st, a);
    return cm_launch_status("cm_ctc_align");
}
