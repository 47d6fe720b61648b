// edit_distance.hip — edit distance with alignment counts (contract: cm_edit_distance; mamba_asr_amd/metrics.py).
// For reference a (R tokens) and hypothesis b (H tokens): D[i][0] = i, D[0][j] = j, sub = D[i-1][j-1] + (a[i-1] != b[j-1]),
// del = D[i-1][j] + 1, ins = D[i][j-1] + 1; the move is diagonal if sub < ins && sub < del, else delete if del < ins, else insert.
// int32 adds and compares only: the bits are those of tests/ctc_score_ref.py.
// One workgroup per pair, three phases in one launch:
//   forward    thread j owns hypothesis column j + 1 and walks the anti-diagonals: at step s it fills cell (s - j + 1, j + 1).  Its
//              own previous value is D[i-1][j], its left neighbour's previous value is D[i][j-1] -- one int through LDS per step,
//              double-buffered, one LDS-only barrier per step -- and what it read from the left one step ago is D[i-1][j-1].  The
//              reference sits in LDS.  No score table: the moves (0 hit, 1 substitution, 2 delete, 3 insert) go to the workspace at
//              2 bits per cell, each thread's 32 steps in one 8-byte word, stored coalesced.
//   backtrace  wave 0.  Over a 32-step block the column falls by at most 31 before the last lookup: the 64 lanes load the words of
//              the columns below the block's top in one coalesced load and the steps run on scalar registers (v_readlane of the
//              word that holds the column); lane q keeps the block's q-th operation, written backwards into the workspace.
//   ops        the path turned into forward order, by all threads.
#include "cm_common.h"

namespace {

constexpr int MAXLEN = CM_EDIT_MAX_LEN;
constexpr int BLK = 32;                   // steps per move word

__host__ __device__ inline int ed_threads(int SH) { return SH <= 0 ? 64 : (SH + 63) / 64 * 64; }
__host__ __device__ inline int64_t ed_blocks(int SR, int SH) { return ((int64_t)SR + SH + BLK - 1) / BLK; }
__host__ __device__ inline int64_t ed_tmp_bytes(int SR, int SH) { return ((int64_t)SR + SH + 15) / 16 * 16; }
// per pair: the move words of every block, then SR + SH bytes for the backwards path
__host__ __device__ inline int64_t ed_pair_bytes(int SR, int SH) { return ed_blocks(SR, SH) * ed_threads(SH) * 8 + ed_tmp_bytes(SR, SH); }

// grid (N); block = SH rounded up to 64 threads (<= 1024)
__global__ __launch_bounds__(1024) void edit_distance_kernel(const cm_edit_distance_args p) {
    __shared__ int nbr[2][MAXLEN + 1];                               // D of thread j's column at [j + 1]
    __shared__ int ref[MAXLEN];
    __shared__ int sh_dist, sh_nops;
    const int pr = blockIdx.x, j = threadIdx.x, Wd = blockDim.x, lane = j & 63;
    const int r = p.ref_index[pr];
    int32_t *counts = p.counts + (int64_t)pr * 4;
    const int wide = p.SR + p.SH;
    int8_t *ops = p.ops ? p.ops + (int64_t)pr * wide : nullptr;
    if (r < 0 || r >= p.NR) {                                        // uniform
        if (j < 4) counts[j] = 0;
        if (j == 0) {
            p.dist[pr] = 0, p.status[pr] = 1;
            if (ops) p.n_ops[pr] = 0;
        }
        if (ops)
            for (int m = j; m < wide; m += Wd) ops[m] = 0;
        return;
    }
    const int R = max(min(p.ref_len[r], p.SR), 0), H = max(min(p.hyp_len[pr], p.SH), 0);
    char *ws = reinterpret_cast<char *>(p.workspace) + (int64_t)pr * ed_pair_bytes(p.SR, p.SH);
    uint64_t *moves = reinterpret_cast<uint64_t *>(ws);
    int8_t *tmp = reinterpret_cast<int8_t *>(ws + ed_blocks(p.SR, p.SH) * Wd * 8);
    const int nsteps = (R > 0 && H > 0) ? R + H - 1 : 0, nblk = (nsteps + BLK - 1) / BLK;

    // ---- forward ----
    int up = j + 1, diag = j;                                        // D[0][j + 1], D[0][j]
    if (nsteps > 0) {
        for (int i = j; i < R; i += Wd) ref[i] = p.refs[(int64_t)r * p.SR + i];
        const int bj = j < H ? p.hyps[(int64_t)pr * p.SH + j] : 0;
        nbr[0][j + 1] = up, nbr[1][j + 1] = up;
        if (j == 0) nbr[0][0] = 0, nbr[1][0] = 0;
        __syncthreads();
        for (int blk = 0; blk < nblk; ++blk) {
            uint64_t word = 0;
#pragma unroll 4
            for (int q = 0; q < BLK; ++q) {
                const int s = blk * BLK + q, i = s - j + 1;
                const bool act = j < H && i >= 1 && i <= R;
                const int left = j == 0 ? i : nbr[(s + 1) & 1][j];   // D[i][j]: column 0, or thread j - 1 one step ago
                const int a = ref[min(max(i - 1, 0), R - 1)];
                const int ne = a != bj ? 1 : 0;
                const int sub = diag + ne, del = up + 1, ins = left + 1;
                int v, mv;
                if (sub < ins && sub < del) v = sub, mv = ne;
                else if (del < ins) v = del, mv = 2;
                else v = ins, mv = 3;
                if (act) diag = left, up = v, word |= (uint64_t)mv << (2 * q);
                nbr[s & 1][j + 1] = up;
                cm_lds_barrier();
            }
            moves[(int64_t)blk * Wd + j] = word;
        }
    }
    __syncthreads();
    if (j == max(H, 1) - 1) sh_dist = nsteps > 0 ? up : max(R, H);
    __syncthreads();

    // ---- backtrace: wave 0 ----
    if (j < 64) {
        int i = R, c = H, n_ins = 0, n_del = 0, n_sub = 0, n_hit = 0, kbase = 0;
        for (int it = 0; it < nblk && i > 0 && c > 0; ++it) {
            const int blk = (i + c - 2) >> 5, jtop = c - 1;
            const int jj = jtop - lane;                              // lane l: the word of column thread jtop - l
            const uint64_t w = jj >= 0 ? moves[(int64_t)blk * Wd + jj] : 0;
            const uint32_t wlo = (uint32_t)w, whi = (uint32_t)(w >> 32);
            int mine = 0, q = 0;
            for (; q < BLK && i > 0 && c > 0 && ((i + c - 2) >> 5) == blk; ++q) {
                const int s = i + c - 2;
                const int idx = __builtin_amdgcn_readfirstlane((jtop - (c - 1)) & 63);
                const uint32_t half = (s & 16) ? (uint32_t)__builtin_amdgcn_readlane((int)whi, idx) : (uint32_t)__builtin_amdgcn_readlane((int)wlo, idx);
                const int mv = (half >> (2 * (s & 15))) & 3;
                const int code = mv == 0 ? '=' : mv == 1 ? 'S' : mv == 2 ? 'D' : 'I';
                mine = lane == q ? code : mine;
                n_hit += mv == 0, n_sub += mv == 1, n_del += mv == 2, n_ins += mv == 3;
                i = __builtin_amdgcn_readfirstlane(i - (mv != 3 ? 1 : 0));
                c = __builtin_amdgcn_readfirstlane(c - (mv != 2 ? 1 : 0));
            }
            if (ops && lane < q) tmp[kbase + lane] = (int8_t)mine;
            kbase += q;
        }
        // row 0: inserts; column 0: deletes (at most one of the two is left)
        if (ops)
            for (int m = lane; m < i + c; m += 64) tmp[kbase + m] = (int8_t)(i > 0 ? 'D' : 'I');
        n_del += i, n_ins += c;
        if (j == 0) {
            counts[0] = n_ins, counts[1] = n_del, counts[2] = n_sub, counts[3] = n_hit;
            p.dist[pr] = sh_dist, p.status[pr] = 0;
            sh_nops = kbase + i + c;
            if (ops) p.n_ops[pr] = kbase + i + c;
        }
    }
    __syncthreads();

    // ---- ops in forward order ----
    if (ops) {
        const int K = sh_nops;
        for (int m = j; m < wide; m += Wd) ops[m] = m < K ? tmp[K - 1 - m] : (int8_t)0;
    }
}

int64_t workspace_bytes(int64_t N, int SR, int SH) { return N * ed_pair_bytes(SR, SH); }

}  // namespace

extern "C" int64_t cm_edit_distance_workspace_bytes(const cm_edit_distance_args *a) {
    if (a == nullptr || a->N <= 0 || a->SR < 0 || a->SH < 0 || a->SR > MAXLEN || a->SH > MAXLEN) return 0;
    return workspace_bytes(a->N, a->SR, a->SH);
}

extern "C" int cm_edit_distance(const cm_edit_distance_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "edit_distance: args is NULL");
    const cm_edit_distance_args a = *args;
    CM_REQUIRE(a.N > 0 && a.NR > 0 && a.SR >= 0 && a.SH >= 0, CM_EINVAL, "edit_distance: bad sizes N=%d NR=%d SR=%d SH=%d", a.N, a.NR, a.SR, a.SH);
    CM_REQUIRE(a.SR <= MAXLEN && a.SH <= MAXLEN, CM_EUNSUPPORTED, "edit_distance: at most %d tokens per sequence (got SR=%d SH=%d)", MAXLEN, a.SR, a.SH);
    CM_REQUIRE(a.ref_len && a.hyp_len && a.ref_index && a.counts && a.dist && a.status && a.workspace, CM_EINVAL, "edit_distance: NULL tensor");
    CM_REQUIRE((a.refs || a.SR == 0) && (a.hyps || a.SH == 0), CM_EINVAL, "edit_distance: refs / hyps may be NULL only at width 0");
    CM_REQUIRE(a.ops == nullptr || a.n_ops != nullptr, CM_EINVAL, "edit_distance: ops needs n_ops");
    CM_REQUIRE(cm_aligned(a.refs, 4) && cm_aligned(a.ref_len, 4) && cm_aligned(a.hyps, 4) && cm_aligned(a.hyp_len, 4) && cm_aligned(a.ref_index, 4) &&
                   cm_aligned(a.counts, 4) && cm_aligned(a.dist, 4) && cm_aligned(a.status, 4) && cm_aligned(a.n_ops, 4) && cm_aligned(a.workspace, 16),
               CM_EALIGN, "edit_distance: a tensor is not aligned to its element size (workspace: 16 bytes)");
    const int64_t need = workspace_bytes(a.N, a.SR, a.SH);
    CM_REQUIRE(a.workspace_bytes >= need, CM_EINVAL, "edit_distance: workspace smaller than cm_edit_distance_workspace_bytes() (%lld < %lld)",
               (long long)a.workspace_bytes, (long long)need);
    hipStream_t st = reinterpret_cast<hipStream_t>(a.stream);
    hipLaunchKernelGGL(edit_distance_kernel, dim3(a.N), dim3(ed_threads(a.SH)), 0, st, a);
    return cm_launch_status("cm_edit_distance");
}
