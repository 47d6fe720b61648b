// ctc_prefix.hip — CTC prefix scores for joint CTC/attention S2S decoding (include/conmamba_hip.h cm_ctc_prefix_*).
//
//   cm_ctc_prefix_score    psi(g + c) - psi(g) for every candidate c of every hypothesis row: a log-sum-exp over time of
//                          phi[t-1] + logp[t, c].  One workgroup per (row, tile of TILE_C candidates): lanes run along c (the
//                          logp[u, t, c..] loads coalesce), the NW waves split the frames in groups of TG and are folded in wave
//                          order at the end.  The row's phi (r_b for c == last, lae(r_n, r_b) otherwise) is built once per
//                          workgroup in LDS, TCHUNK frames at a time.  Each lane keeps a running maximum and a sum scaled by it.
//   cm_ctc_prefix_advance  the chosen token's new (r_n, r_b): two first-order recurrences h' = lae(h + a_t, b_t) over time, one
//                          wave per row, 64 frames per pass: an inclusive scan of the pairs (a, b) under
//                          (a1, b1) . (a2, b2) = (a1 + a2, lae(b1 + a2, b2)), applied to the carry of the pass before.
//
// No +inf ever enters (log-probabilities are <= 0 or -inf), so -inf + x and lae() below cannot produce NaN.
#include "cm_common.h"

#include <math.h>

namespace {

constexpr int TILE_C = CM_CTC_PREFIX_TILE_C;   // candidates per workgroup = one wave's lanes
constexpr int TCHUNK = CM_CTC_PREFIX_TCHUNK;   // frames of phi in LDS at a time
constexpr int NW = 8;                          // waves per workgroup: they split the frames
constexpr int TG = 8;                          // frames per group: loads in flight per lane, one rescale per group
constexpr int NT = NW * 64;
static_assert(TILE_C == 64, "one candidate per lane of a wave");
static_assert(TCHUNK % (NW * TG) == 0, "a chunk is a whole number of rounds of the waves");

#define NEG_INF (-INFINITY)

__device__ __forceinline__ float lae(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + CM_LN2 * cm_log2(1.0f + cm_exp2(-CM_LOG2E * fabsf(a - b)));
}

__global__ __launch_bounds__(NT) void ctc_prefix_score_kernel(cm_ctc_prefix_args p) {
    __shared__ float phi_d[TCHUNK], phi_s[TCHUNK];      // lae(r_n, r_b) and r_b of frames [chunk, chunk + TCHUNK)
    __shared__ float part_m[NW][TILE_C], part_s[NW][TILE_C];
    const int row = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ncol = p.K > 0 ? p.K : p.V;
    const int col = tile * TILE_C + lane;
    float *out = p.out + (int64_t)row * ncol;
    const int u = p.row_utt[row];
    if (u < 0 || u >= p.U) {                            // uniform over the workgroup
        if (w == 0 && col < ncol) out[col] = NEG_INF;
        return;
    }
    const int n = min(max(p.n_u[u], 0), p.T);
    const int lastc = p.last[row];
    int c = -1;
    if (col < ncol) c = p.candidates ? p.candidates[(int64_t)row * p.K + col] : col;
    const bool valid = c >= 0 && c < p.V;
    const bool same = c == lastc;
    const float *lp = p.logp + (int64_t)u * p.T * p.V + (valid ? c : 0);   // an invalid lane reads column 0 and drops the result
    const float *rn = p.r_n + (int64_t)row * p.T, *rb = p.r_b + (int64_t)row * p.T;

    // psi(c) = lae over t = 1 .. n-1 of phi[t-1] + logp[t, c]; j = t - 1 below
    float m = NEG_INF, s = 0.f;
    for (int j0 = 0; j0 < n - 1; j0 += TCHUNK) {
        const int cnt = min(TCHUNK, n - 1 - j0);
        __syncthreads();                                // the chunk before has been read
        for (int i = tid; i < cnt; i += NT) {
            const float a = rn[j0 + i], b = rb[j0 + i];
            phi_d[i] = lae(a, b);
            phi_s[i] = b;
        }
        __syncthreads();
        for (int g = w * TG; g < cnt; g += NW * TG) {
            float x[TG];
#pragma unroll
            for (int k = 0; k < TG; ++k) {
                const int i = g + k;
                x[k] = NEG_INF;
                if (i < cnt) x[k] = (same ? phi_s[i] : phi_d[i]) + lp[(int64_t)(j0 + i + 1) * p.V];
            }
            float gm = x[0];
#pragma unroll
            for (int k = 1; k < TG; ++k) gm = fmaxf(gm, x[k]);
            const float mn = fmaxf(m, gm);
            if (mn > NEG_INF) {
                float acc = s * cm_exp2(CM_LOG2E * (m - mn));
#pragma unroll
                for (int k = 0; k < TG; ++k) acc += cm_exp2(CM_LOG2E * (x[k] - mn));
                s = acc;
                m = mn;
            }
        }
    }
    part_m[w][lane] = m;
    part_s[w][lane] = s;
    __syncthreads();
    if (w != 0 || col >= ncol) return;
    // fold the waves' partial sums in wave order
    float M = part_m[0][lane];
#pragma unroll
    for (int k = 1; k < NW; ++k) M = fmaxf(M, part_m[k][lane]);
    float psi = NEG_INF;
    if (M > NEG_INF) {
        float S = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) S += part_s[k][lane] * cm_exp2(CM_LOG2E * (part_m[k][lane] - M));
        psi = M + CM_LN2 * cm_log2(S);
    }
    if (lastc < 0 && n >= 1) psi = lae(psi, lp[0]);                          // the empty prefix: c may start at frame 0
    if (c == p.eos) psi = n >= 1 ? lae(rn[n - 1], rb[n - 1]) : NEG_INF;     // the prefix itself, all frames used
    if (!valid || c == p.blank || n < 1) psi = NEG_INF;
    out[col] = psi == NEG_INF ? NEG_INF : psi - p.psi_g[row];
}

struct Pair { float a, b; };                            // h -> lae(h + a, b)
__device__ __forceinline__ Pair then(Pair l, Pair r) { return {l.a + r.a, lae(l.b + r.a, r.b)}; }

// inclusive scan over the wave's lanes (lane order = time order)
__device__ __forceinline__ Pair wave_scan(Pair v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Pair l = {__shfl_up(v.a, d, 64), __shfl_up(v.b, d, 64)};
        if (lane >= d) v = then(l, v);
    }
    return v;
}

__global__ __launch_bounds__(64) void ctc_prefix_advance_kernel(cm_ctc_prefix_args p) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const int T = p.T;
    const float *rn = p.r_n + (int64_t)row * T, *rb = p.r_b + (int64_t)row * T;
    float *on = p.r_n_out + (int64_t)row * T, *ob = p.r_b_out + (int64_t)row * T;
    const int u = p.row_utt[row];
    const int c = p.tokens[row];
    const int lastc = p.last[row];
    if (c == p.eos) {                                   // a finished row keeps its state
        for (int t = lane; t < T; t += 64) { on[t] = rn[t]; ob[t] = rb[t]; }
        if (lane == 0) { p.psi_out[row] = p.psi_g[row]; p.last_out[row] = lastc; }
        return;
    }
    if (lane == 0) p.last_out[row] = c;
    const bool possible = u >= 0 && u < p.U && c >= 0 && c < p.V && c != p.blank;
    const int n = possible ? min(max(p.n_u[u], 0), T) : 0;
    const bool same = c == lastc, empty = lastc < 0;
    const float *lpc = p.logp + (int64_t)(possible ? u : 0) * T * p.V + (possible ? c : 0);
    const float *lpb = p.logp + (int64_t)(possible ? u : 0) * T * p.V + p.blank;
    float carry_n = NEG_INF, carry_b = NEG_INF;         // r_n'[t0 - 1], r_b'[t0 - 1]
    float m = NEG_INF, s = 0.f;                         // this lane's share of psi(c), frames lane, lane + 64, ...
    for (int t0 = 0; t0 < n; t0 += 64) {
        const int t = t0 + lane;
        const bool live = t < n;
        Pair e = {0.f, NEG_INF};                        // past the end: the identity
        float lb = 0.f;
        if (live) {
            const float lc = lpc[(int64_t)t * p.V];
            lb = lpb[(int64_t)t * p.V];
            if (t == 0) {
                e = {NEG_INF, empty ? lc : NEG_INF};    // frame 0 forgets what came before
            } else {
                const float a = rn[t - 1], b = rb[t - 1];
                e = {lc, (same ? b : lae(a, b)) + lc};
            }
            const float mn = fmaxf(m, e.b);             // e.b is this frame's term of psi(c)
            if (mn > NEG_INF) {
                s = s * cm_exp2(CM_LOG2E * (m - mn)) + cm_exp2(CM_LOG2E * (e.b - mn));
                m = mn;
            }
        }
        const Pair sn = wave_scan(e, lane);
        const float new_n = lae(carry_n + sn.a, sn.b);  // r_n'[t]
        float prev_n = __shfl_up(new_n, 1, 64);         // r_n'[t - 1]
        if (lane == 0) prev_n = carry_n;
        Pair f = {0.f, NEG_INF};
        if (live) f = t == 0 ? Pair{NEG_INF, NEG_INF} : Pair{lb, prev_n + lb};
        const Pair sb = wave_scan(f, lane);
        const float new_b = lae(carry_b + sb.a, sb.b);  // r_b'[t]
        if (live) { on[t] = new_n; ob[t] = new_b; }
        carry_n = __shfl(new_n, 63, 64);                // lanes past the end hold the last live value (identity elements)
        carry_b = __shfl(new_b, 63, 64);
    }
    for (int t = n + lane; t < T; t += 64) { on[t] = NEG_INF; ob[t] = NEG_INF; }
    // psi(c): fold the lanes' shares in a fixed butterfly
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float om = __shfl_xor(m, d, 64), os = __shfl_xor(s, d, 64);
        const float mn = fmaxf(m, om);
        if (mn > NEG_INF) {
            // the lower lane's share first, so both partners compute the same bits
            const bool lo = (lane & d) == 0;
            const float a = (lo ? s : os) * cm_exp2(CM_LOG2E * ((lo ? m : om) - mn));
            const float b = (lo ? os : s) * cm_exp2(CM_LOG2E * ((lo ? om : m) - mn));
            s = a + b;
            m = mn;
        }
    }
    if (lane == 0) p.psi_out[row] = m > NEG_INF ? m + CM_LN2 * cm_log2(s) : NEG_INF;
}

int check_common(const cm_ctc_prefix_args &a, const char *what) {
    CM_REQUIRE(a.U > 0 && a.T > 0 && a.V > 1 && a.rows > 0, CM_EINVAL, "%s: bad sizes U=%d T=%d V=%d rows=%d", what, a.U, a.T, a.V, a.rows);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V && a.eos >= 0 && a.eos < a.V && a.blank != a.eos, CM_EINVAL,
               "%s: blank %d / eos %d must be two tokens of [0, %d)", what, a.blank, a.eos, a.V);
    CM_REQUIRE(a.logp && a.n_u && a.row_utt && a.last && a.r_n && a.r_b && a.psi_g, CM_EINVAL, "%s: NULL pointer", what);
    return CM_OK;
}

}  // namespace

extern "C" int cm_ctc_prefix_score(const cm_ctc_prefix_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_prefix_score: args is NULL");
    const cm_ctc_prefix_args a = *args;
    if (int rc = check_common(a, "ctc_prefix_score")) return rc;
    CM_REQUIRE(a.K >= 0 && (a.K > 0) == (a.candidates != nullptr), CM_EINVAL,
               "ctc_prefix_score: K=%d and candidates must be given together", a.K);
    CM_REQUIRE(a.out != nullptr, CM_EINVAL, "ctc_prefix_score: NULL pointer");
    const int64_t tiles = ((int64_t)(a.K > 0 ? a.K : a.V) + TILE_C - 1) / TILE_C;
    CM_REQUIRE(tiles <= 65535, CM_EUNSUPPORTED, "ctc_prefix_score: at most %d candidates per row", 65535 * TILE_C);
    hipLaunchKernelGGL(ctc_prefix_score_kernel, dim3(a.rows, (unsigned)tiles), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a);
    return cm_launch_status("cm_ctc_prefix_score");
}

extern "C" int cm_ctc_prefix_advance(const cm_ctc_prefix_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_prefix_advance: args is NULL");
    const cm_ctc_prefix_args a = *args;
    if (int rc = check_common(a, "ctc_prefix_advance")) return rc;
    CM_REQUIRE(a.tokens && a.r_n_out && a.r_b_out && a.psi_out && a.last_out, CM_EINVAL, "ctc_prefix_advance: NULL pointer");
    CM_REQUIRE(a.r_n_out != a.r_n && a.r_b_out != a.r_b && a.r_n_out != a.r_b && a.r_b_out != a.r_n && a.r_n_out != a.r_b_out &&
                   a.psi_out != a.psi_g && a.last_out != a.last, CM_EINVAL, "ctc_prefix_advance: the outputs must not alias the inputs");
    hipLaunchKernelGGL(ctc_prefix_advance_kernel, dim3(a.rows), dim3(64), 0, reinterpret_cast<hipStream_t>(a.stream), a);
    return cm_launch_status("cm_ctc_prefix_advance");
}
