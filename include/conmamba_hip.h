/* conmamba_hip.h — C ABI of libconmamba_hip.so (MI355X / gfx950 native kernels for the
 * ConMamba ASR encoder hot path).
 *
 * This is the drop-in boundary: the entry points below are what the reference's Python
 * binds where it today imports the CUDA-only extension modules
 *     selective_scan_cuda   (reference modules/mamba/selective_scan_interface.py:16)
 *     causal_conv1d_cuda    (reference modules/mamba/selective_scan_interface.py:15)
 * Plain pointers and sizes only — no torch types.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (outputs and scratch included);
 *     the library never allocates, frees or retains memory;
 *   - calls are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and use the caller's current device; no device synchronisation inside;
 *   - return value: CM_OK (0) on success, a negative CM_E* code for rejected arguments, a
 *     positive value = hipError_t from the launch; cm_last_error() returns a thread-local
 *     message; nothing aborts or throws across this boundary;
 *   - re-entrant, callable from any thread (autograd backward threads included);
 *   - "time-contiguous" tensors are laid out (batch, dim, seqlen) with element stride 1 along
 *     seqlen, as the reference makes them before calling its kernels
 *     (selective_scan_interface.py:24-35, 177-178); batch/dim strides are passed in elements so
 *     that x / z (and dx / dz) may be the two halves of one xz tensor (:180, :249-256);
 *   - fp32 reduction outputs (dA, dD, ddelta_bias, dB, dC, dweight, dbias) are ACCUMULATED
 *     into: the caller zero-initialises them (or passes running sums on purpose).
 *
 * This file is also the source of the Python binding: mamba_asr_amd/_native.py parses it at import and derives every
 * ctypes structure, every prototype and every CM_* constant from it (there is no second copy to keep in step), and it
 * refuses a declaration it does not understand.  So the header stays inside this subset of C:
 *   - conditionals: the include guard, the __cplusplus block and #ifdef CM_ABLATE ... #endif only;
 *   - `typedef struct cm_x { ... } cm_x;` with fields of type int, int32_t, uint32_t, int64_t, uint64_t, float, double, an
 *     earlier struct by value, or a pointer; several declarators per declaration and [N] arrays are fine; no bit-fields,
 *     unions or function pointers;
 *   - `typedef enum { A = 0, ... } name;` and `#define CM_X <integer>` (parentheses, sign, hex, u / l suffixes);
 *   - prototypes returning int, int32_t, int64_t or const char *, taking those integer types and pointers.
 * tests/test_abi.py checks the derived layouts against the C compiler's sizeof / offsetof.
 */
#ifndef CONMAMBA_HIP_H
#define CONMAMBA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CM_ABI_VERSION 12

/* error codes */
#define CM_OK            0
#define CM_EINVAL       (-1)   /* inconsistent sizes / null required pointer           */
#define CM_EUNSUPPORTED (-2)   /* valid request this build has no kernel for           */
#define CM_EALIGN       (-3)   /* pointer/stride violates a documented alignment rule  */

/* element types of activation tensors */
typedef enum { CM_F32 = 0, CM_BF16 = 1, CM_F16 = 2 } cm_dtype;

/* timesteps per scan checkpoint: the `x` tensor of the scan holds the recurrent state at the
 * end of every chunk of this many steps (the role of selective_scan_cuda.fwd's second return
 * value, selective_scan_interface.py:42-45: last_state = x[:, :, -1, 1::2]). */
#define CM_SCAN_CHUNK 64

int         cm_abi_version(void);
const char *cm_last_error(void);
/* number of checkpoint chunks for a sequence length: ceil(seqlen / CM_SCAN_CHUNK) */
int         cm_scan_num_chunks(int seqlen);
#ifdef CM_ABLATE
/* Ablation build only (make -C mamba_asr_amd/csrc ablate -> lib/libconmamba_hip_ablate.so, loaded by the tools through
 * CM_LIB_PATH): a process-wide switch selecting timing-only kernel variants with one stage removed (results are then WRONG by
 * construction; tools/bench_scan.py, bench_ffn.py produce DESIGN.md's ablation tables with it).  The product library is
 * compiled without CM_ABLATE: it has no such switch, no ablation kernels and no process-global mutable state. */
int         cm_debug_set(int ablation);
int         cm_debug_get(void);
#endif

/* ---------------------------------------------------------------------------------------
 * Selective scan forward — replaces selective_scan_cuda.fwd
 *   (call sites selective_scan_interface.py:42, 218, 359, 504, 508; spec = selective_scan_ref
 *    :91-157).  Real A, input-dependent B/C with one group: B, C are (batch, 1, dstate, seqlen).
 *
 *   delta' = delta + delta_bias[d]            (if delta_bias)
 *   delta' = softplus(delta')                 (if delta_softplus; threshold 20)
 *   h_t = exp(delta'_t A[d,n]) h_{t-1} + delta'_t B[n,t] u_t ,  h_{-1} = 0
 *   out_t   = sum_n C[n,t] h_t[n] + D[d] u_t  (D optional)
 *   out_z_t = out_t * silu(z_t)               (z optional)
 * reverse_time != 0 runs the recurrence from t = seqlen-1 down to 0 on the tensors as stored —
 * numerically what the reference obtains by .flip(-1) on every input and on the output
 * (modules/mamba/bimamba.py:237, 253) without materialising the flips.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_scan_fwd_args {
    int32_t batch, dim, seqlen, dstate;
    int32_t io_dtype;        /* cm_dtype of u, delta, z, out, out_z                       */
    int32_t bc_dtype;        /* cm_dtype of B, C                                          */
    int32_t delta_softplus;  /* bool                                                      */
    int32_t reverse_time;    /* bool                                                      */
    const void  *u;          /* (batch, dim, seqlen)                                      */
    const void  *delta;      /* (batch, dim, seqlen)                                      */
    const float *A;          /* (dim, dstate) fp32, contiguous                            */
    const void  *B;          /* (batch, 1, dstate, seqlen)                                */
    const void  *C;          /* (batch, 1, dstate, seqlen)                                */
    const float *D;          /* (dim) fp32 or NULL                                        */
    const void  *z;          /* (batch, dim, seqlen) or NULL                              */
    const float *delta_bias; /* (dim) fp32 or NULL                                        */
    void        *out;        /* (batch, dim, seqlen) pre-gate output; may be NULL if z    */
    void        *out_z;      /* gated output; required iff z != NULL                      */
    float       *x;          /* (batch, dim, nchunks, 2*dstate) fp32 checkpoints or NULL:
                                [2n] = product of exp(delta' A) over the chunk, [2n+1] = h at
                                the chunk's last processed step                            */
    int64_t u_bs, u_ds;          /* batch / dim strides in elements (time stride is 1)    */
    int64_t delta_bs, delta_ds;
    int64_t z_bs, z_ds;
    int64_t out_bs, out_ds;      /* shared by out and out_z                               */
    int64_t B_bs, B_ns;          /* batch / state strides of B                            */
    int64_t C_bs, C_ns;
    void   *stream;
    const float *h0;         /* (batch, dim, dstate) fp32, contiguous, or NULL: the state the
                                recurrence starts from instead of zero (in scan order: before
                                step 0, or behind step seqlen-1 with reverse_time).  Forward only
                                (cm_selective_scan_bwd rejects it).  With it, a sequence cut into
                                time shards gives the unsplit result: shard k starts from shard
                                k-1's last state x[:, :, last chunk, 1::2] -- the carry the
                                time-split scan across GPUs exchanges (no
                                reference counterpart: the reference has no sequence parallelism,
                                SURVEY.md §5)                                               */
    int32_t lanes_per_channel; /* tuning: lanes one channel's states are split over (1, 2, 4, 8, 16; backward: 4, 8,
                                16); 0 = the library's choice from the problem size.  Results do not depend on it
                                beyond fp32 summation order                                  */
    int32_t pad4_;
} cm_scan_fwd_args;

int cm_selective_scan_fwd(const cm_scan_fwd_args *args);

/* ---------------------------------------------------------------------------------------
 * Selective scan backward — replaces selective_scan_cuda.bwd
 *   (call sites selective_scan_interface.py:67, 252, 394, 546, 553).
 * Inputs as forward plus dout (gradient of out_z if z else of out) and the forward's x.
 * du, ddelta, dz have io_dtype; dz may alias a slice of a larger tensor (the reference writes
 * it into dxz, :249-256).  dA (dim,dstate), dD (dim), ddelta_bias (dim), dB, dC
 * (batch,1,dstate,seqlen) are fp32 and ACCUMULATED into.  If out_z != NULL (and z != NULL) the
 * gated forward output is recomputed into it (the reference's recompute_out_z flag).
 * ------------------------------------------------------------------------------------- */
typedef struct cm_scan_bwd_args {
    cm_scan_fwd_args fwd;    /* same tensors as forward; fwd.out / fwd.out_z: see above;
                                fwd.x = checkpoints written by the forward (required)      */
    const void *dout;        /* (batch, dim, seqlen), io_dtype                            */
    int64_t dout_bs, dout_ds;
    void  *du;               /* (batch, dim, seqlen), io_dtype                            */
    void  *ddelta;
    void  *dz;               /* or NULL when z == NULL                                    */
    int64_t du_bs, du_ds, ddelta_bs, ddelta_ds, dz_bs, dz_ds;
    float *dA;               /* (dim, dstate)                                             */
    float *dB;               /* (batch, 1, dstate, seqlen) contiguous fp32                */
    float *dC;
    float *dD;               /* (dim) or NULL                                             */
    float *ddelta_bias;      /* (dim) or NULL                                             */
    void  *workspace;        /* optional scratch of cm_selective_scan_bwd_workspace_bytes()
                                bytes (16-byte aligned), or NULL.  With it every reduction
                                across workgroups (dB / dC over channel tiles; dA, dD,
                                ddelta_bias over the batch) is a per-workgroup partial + a
                                second kernel that sums in a FIXED order: gradients are
                                bit-identical from run to run.  Without it they are fp32
                                atomics, as in the CUDA kernels the reference binds          */
    int64_t workspace_bytes; /* size of workspace; 0 with NULL                            */
} cm_scan_bwd_args;

int cm_selective_scan_bwd(const cm_scan_bwd_args *args);
/* bytes of workspace the deterministic path needs for these sizes (uses batch, dim, seqlen, dstate only) */
int64_t cm_selective_scan_bwd_workspace_bytes(const cm_scan_bwd_args *args);

/* ---------------------------------------------------------------------------------------
 * Causal depthwise conv1d (+ optional SiLU) — replaces causal_conv1d_cuda.causal_conv1d_fwd /
 * causal_conv1d_bwd (call sites selective_scan_interface.py:182, 244, 286, 323, 385, 430; the
 * reference's own definition of the op: modules/mamba/bimamba.py:83-91, 278-279).
 *   y[b,d,t] = act( bias[d] + sum_{k<width} weight[d,k] * x[b,d,t-(width-1)+k] ),  x[<0] = 0
 * reverse_time != 0 mirrors the time axis (anti-causal conv), i.e. conv(flip(x)) flipped back.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_conv_args {
    int32_t batch, dim, seqlen, width;     /* width 2..4                                   */
    int32_t io_dtype;                      /* cm_dtype of x, y, dy, dx                      */
    int32_t silu;                          /* bool                                          */
    int32_t reverse_time;                  /* bool                                          */
    const void  *x;                        /* (batch, dim, seqlen)                          */
    const float *weight;                   /* (dim, width) fp32 contiguous                  */
    const float *bias;                     /* (dim) fp32 or NULL                            */
    void        *y;                        /* forward output (fwd only)                     */
    int64_t x_bs, x_ds, y_bs, y_ds;
    /* backward only */
    const void  *dy;                       /* (batch, dim, seqlen)                          */
    void        *dx;                       /* may alias a slice of a larger tensor          */
    float       *dweight;                  /* (dim, width) fp32, accumulated                */
    float       *dbias;                    /* (dim) fp32 or NULL, accumulated               */
    int64_t dy_bs, dy_ds, dx_bs, dx_ds;
    void   *stream;
    float  *workspace;                     /* backward, optional: batch * dim * (width + 1) floats, or NULL.  With it the
                                              per-(batch, channel) partial sums of dweight / dbias are stored and summed over
                                              the batch in a fixed order by a second kernel (bit-identical from run to run);
                                              without it they are fp32 atomics                                          */
} cm_conv_args;

int cm_causal_conv1d_fwd(const cm_conv_args *args);
int cm_causal_conv1d_bwd(const cm_conv_args *args);


/* ---------------------------------------------------------------------------------------
 * Channels-last selective scan forward — the MI355X-native layout of the fused BiMamba path.
 * Same math as cm_selective_scan_fwd, but activations are (batch, seqlen, dim) with the channel
 * axis contiguous (what the in_proj GEMM writes: reference bimamba.py:192-196 produces the same
 * numbers transposed), B/C are fp32 (dstate, batch, seqlen) with time contiguous, and up to two
 * independent directions (the two halves of BiMamba v2, reference bimamba.py:223-248) run in ONE
 * launch: direction d uses its own u/delta/A/B/C/D/delta_bias/out and walks time forward
 * (reverse[d] == 0) or backward.  z is shared.  Row (time) and batch strides are in elements, so
 * z / out may be column slices of wider buffers ([x|z], [y_fwd|y_bwd]).
 * B/C rows must be readable up to the next multiple of 16 steps past seqlen (pad the allocation).
 * ------------------------------------------------------------------------------------- */
typedef struct cm_scan_cl_dir {
    const void  *u;          /* (batch, seqlen, dim)  conv+SiLU output                      */
    const void  *delta;      /* (batch, seqlen, dim)  pre-bias, pre-softplus; ignored when dt_low is set */
    const float *A;          /* (dim, dstate)                                               */
    const float *B;          /* (dstate, batch, seqlen) fp32                                */
    const float *C;
    const float *dt_low;     /* optional (dt_rank, batch, seqlen) fp32, same strides as B/C: the low-rank
                                time-step features x_dbl[:, :dt_rank]; when given the kernel forms
                                delta = dt_weight @ dt_low itself (the reference's dt_proj GEMM,
                                selective_scan_interface.py:187) and no delta tensor is read          */
    const float *dt_weight;  /* (dim, dt_rank) fp32, required with dt_low; dt_rank <= 16           */
    const float *D;          /* (dim) or NULL                                               */
    const float *delta_bias; /* (dim) or NULL                                               */
    void        *out;        /* (batch, seqlen, dim)  gated output                          */
    int64_t u_bs, u_ts, delta_bs, delta_ts, out_bs, out_ts;
    int64_t bc_ns, bc_bs;    /* state / batch strides of B and C                            */
    int32_t reverse_time;
    int32_t dt_rank;
    const void *xdbl;        /* optional (batch, seqlen, P + 32) in the I/O dtype: the x_proj GEMM's output rows as it
                                wrote them, columns [0,P) = dt features zero-padded to P, [P,P+16) = B_t, [P+16,P+32)
                                = C_t (selective_scan_interface.py:186, 192-215 without the transposed copies), where
                                P = 16 when dt_rank <= 16 and P = 32 when 16 < dt_rank <= 32 (bf16 only; the S2S-large
                                encoder, d_model 512).  When set for every direction, B / C / dt_low / delta are
                                ignored, dt_weight must be (dim, P) fp32 zero-padded, dim a multiple of 8 (bf16) /
                                4 (fp32), and the row-group kernel (csrc/scan_rows_fwd.hip) runs                    */
    int64_t xdbl_bs, xdbl_ts;/* batch / step strides of xdbl in elements (multiples of 8 for bf16, 4 for fp32)       */
    /* xdbl mode only, all optional, (batch, dim, 16) fp32 contiguous -- the carry interface of the time-split scan
       (no reference counterpart): */
    const float *h0;         /* state the recurrence starts from (in this direction's scan order) instead of zero     */
    float       *h_last;     /* out: state after the last processed step                                               */
    float       *decay;      /* out: product over the sequence of exp(delta' A), i.e. what a state entering this shard
                                is multiplied by on its way through it                                                */
    /* xdbl mode only, optional: what the training forward saves for cm_scan_cl_bwd (the role of the checkpoint tensor `x`
       of selective_scan_cuda.fwd, selective_scan_interface.py:42, on this kernel's 16-step blocks) */
    float       *ckpt;       /* out: (batch, 2 ceil(seqlen / 16), dim, 16) fp32: the state the recurrence ENTERS each half
                                block of 8 steps [8 m, 8 m + 8) with, in this direction's scan order (m < 2 ceil(seqlen/16);
                                steps past seqlen pass the state through)                                            */
    void        *ypre;       /* out: (batch, seqlen, dim), I/O dtype: the pre-gate output sum_n C h + D u              */
    int64_t ypre_bs, ypre_ts;
} cm_scan_cl_dir;

typedef struct cm_scan_cl_args {
    int32_t batch, seqlen, dim, dstate;
    int32_t io_dtype;        /* CM_BF16 or CM_F32: u, delta, z, out                         */
    int32_t delta_softplus;
    int32_t ndir;            /* 1 or 2                                                      */
    int32_t time_chunks;     /* xdbl mode only: 0 / 1 = one workgroup per (sequence, 64 channels); C > 1 = cut every
                                sequence into C chunks of whole 16-step blocks that run in parallel -- a summary pass
                                (per-chunk decay product and zero-state end state), a carry fold in scan order, and an
                                output pass from each chunk's entry state: SURVEY.md §8f row 3's algebra inside one
                                GPU, for batches too small to fill the chip (cm_scan_cl_fwd_auto_chunks).  Outputs
                                differ from the unchunked launch by fp32 rounding only.  Needs `workspace`.           */
    const void *z;           /* (batch, seqlen, dim) or NULL                                */
    int64_t z_bs, z_ts;
    cm_scan_cl_dir dir[2];
    void *stream;
    void   *workspace;       /* time_chunks > 1: cm_scan_cl_fwd_workspace_bytes(args) bytes, 16-byte aligned, caller owned */
    int64_t workspace_bytes;
    int32_t lanes_per_channel; /* tuning: lanes a channel's 16 states are spread over.  State-split kernel (no xdbl): 4, 8 or
                                  16; xdbl mode: 4 (scan_rows_fwd.hip) or 8 (scan_rows_fwd2.hip: z + softplus, dt_rank <= 16,
                                  unchunked; measured slower at every size, never chosen automatically); 0 = automatic  */
    int32_t pad5_;
} cm_scan_cl_args;

int cm_scan_cl_fwd(const cm_scan_cl_args *args);
/* The same launch with per-slot lengths: sequence b runs its first min(max(lens[b], 0), seqlen) steps from h0 and
 * leaves the state behind them in h_last; lens[b] == 0: h_last = h0 (zeros without h0), decay = 1.  The steps it runs give the
 * bits of cm_scan_cl_fwd on that sequence alone with seqlen = lens[b]; inputs at and past step lens[b] are not loaded, `out` rows
 * there are not written.  lens: `batch` int32 in DEVICE memory, read by the kernel (no host read-back).  xdbl mode, one
 * direction in forward time, unchunked (time_chunks <= 1), lanes_per_channel 0 or 4, no ckpt; anything else, NULL lens
 * included, is refused before anything is launched. */
int cm_scan_cl_fwd_slots(const cm_scan_cl_args *args, const int32_t *lens);
/* Whole utterances of different lengths in one batch: sequence b has L = min(max(lens[b], 0), seqlen) steps, and
 * every direction of the launch runs exactly the steps [0, L) -- forward time from step 0, reverse time from step L - 1, each from a
 * zero state, over the 16-step blocks of a launch with seqlen = L.  The `out` rows [0, L) carry the bits of cm_scan_cl_fwd
 * (time_chunks = 1) on that sequence alone with seqlen = L; inputs at and past step L are not loaded, `out` rows there are not
 * written; L == 0 reads nothing and writes nothing.  lens: `batch` int32 in DEVICE memory, read by the kernel (no host read-back).
 * xdbl mode, one or two directions, unchunked (time_chunks <= 1), lanes_per_channel 0 or 4, no ckpt / ypre / h0 / h_last / decay;
 * anything else, NULL lens included, is refused before anything is launched (CM_EUNSUPPORTED / CM_EINVAL). */
int cm_scan_cl_fwd_lens(const cm_scan_cl_args *args, const int32_t *lens);
/* bytes of workspace the launch described by args needs (0 unless time_chunks > 1) */
int64_t cm_scan_cl_fwd_workspace_bytes(const cm_scan_cl_args *args);
/* the chunk count that fills 256 CUs for this problem size (1 = do not chunk); a pure function of the sizes */
int32_t cm_scan_cl_fwd_auto_chunks(int32_t batch, int32_t seqlen, int32_t dim, int32_t ndir);
/* Both BiMamba directions folded into ONE output tensor (reference bimamba.py:251-253 adds the directions in front
 * of out_proj, and both are gated by the same SiLU(z)): dir[0].out (batch, seqlen, dim) receives
 *     out[t] = io((hi + float(io(p_first[t] - hi)) + p_second[t]) * SiLU(z[t])),  hi = float(io(p_first[t])),
 * p = sum_n C h + D u the pre-gate value of one direction (p_first is carried as two I/O-dtype pieces: one rounding, the result's),
 * where "first" is the direction that reaches row t first: with L the sequence's step count and mid = 16 * (ceil(L / 16) / 2), forward
 * time for t < mid and reverse time for t >= mid -- a function of t and L alone.  Two launches of one grid in args->stream: the first
 * runs forward time over [0, mid) and reverse time over [mid, L) from zero states, stores p in the I/O dtype into `out`, and what
 * that rounding dropped and each direction's state into the workspace; the second carries both recurrences on from there (the same values in the same order as an
 * uncut run), adds, gates once and stores in place.  args->workspace: cm_scan_cl_fwd_fold_workspace_bytes(args) bytes ((2, batch, dim,
 * 16) fp32 states, then (batch, seqlen, dim) in the I/O dtype), 16-byte aligned, caller owned.  Requires: xdbl mode, two directions of opposite time, z and softplus, bf16 I/O,
 * dt_rank <= 16, time_chunks <= 1, lanes_per_channel 0 or 4, no ckpt / ypre / h0 / h_last / decay, dir[1].out NULL or equal to
 * dir[0].out (dir[1]'s out strides are ignored); anything else is refused before anything is launched (CM_EUNSUPPORTED / CM_EINVAL /
 * CM_EALIGN).  cm_scan_cl_fwd_fold: L = seqlen.  cm_scan_cl_fwd_fold_lens: L = min(max(lens[b], 0), seqlen) with the semantics of
 * cm_scan_cl_fwd_lens -- rows at and past L are neither read nor written, L == 0 reads and writes nothing, rows [0, L) carry the bits
 * of cm_scan_cl_fwd_fold on that sequence alone with seqlen = L; lens: `batch` int32 in DEVICE memory, NULL is refused. */
int cm_scan_cl_fwd_fold(const cm_scan_cl_args *args);
int cm_scan_cl_fwd_fold_lens(const cm_scan_cl_args *args, const int32_t *lens);
/* bytes of workspace the fold needs: 2 * batch * dim * 16 * sizeof(float) for the states plus batch * seqlen * dim * 2 for the
 * remainders of the first launch's bf16 roundings; a pure function of the sizes */
int64_t cm_scan_cl_fwd_fold_workspace_bytes(const cm_scan_cl_args *args);

/* ---------------------------------------------------------------------------------------
 * Channels-last selective scan BACKWARD, both BiMamba directions in one launch (csrc/scan_rows_bwd.hip): the gradient
 * of cm_scan_cl_fwd's xdbl mode with z and softplus -- selective_scan_cuda.bwd (selective_scan_interface.py:252-256)
 * together with the dt_proj part of MambaInnerFnNoOutProj.backward (:258-283: ddelta -> d dt_proj.weight and the dt
 * columns of dx_dbl), on the forward's layout: rows (batch * time, channels), x_dbl rows as the x_proj GEMM wrote them,
 * no transposed copy.  Per direction:
 *   in : u, xdbl, A, dt_weight (dim, P) fp32 zero padded, D, delta_bias (as the forward), ckpt and ypre written by the
 *        forward, dout = gradient of the gated output; shared z
 *   out: du (gradient w.r.t. u through the scan only: the x_proj path is added by the caller), dz (THIS direction's
 *        share of dz: the caller adds the two), dxdbl (batch, seqlen, P + 32) in the I/O dtype = [d dt (P) | dB | dC],
 *        and fp32 dA (dim, 16), ddt_weight (dim, P), dD (dim), ddelta_bias (dim), ACCUMULATED into.
 * Every cross-workgroup sum (dxdbl over the channel groups, the parameter gradients over the batch) goes through the
 * caller-owned workspace and a fixed-order second pass: bit-identical results from run to run.
 * dim: multiple of 8 (bf16) / 4 (fp32); dstate 16; dt_rank <= 16, or <= 32 with bf16 I/O; strides in elements.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_scan_cl_bwd_dir {
    const void  *u;          /* (batch, seqlen, dim)                                         */
    const void  *xdbl;       /* (batch, seqlen, P + 32)                                      */
    const float *A;          /* (dim, 16)                                                    */
    const float *dt_weight;  /* (dim, P) fp32, zero padded                                   */
    const float *D;          /* (dim) or NULL                                                */
    const float *delta_bias; /* (dim) or NULL                                                */
    const float *ckpt;       /* (batch, 2 ceil(seqlen / 16), dim, 16) from the forward      */
    const void  *ypre;       /* (batch, seqlen, dim) from the forward                       */
    const void  *dout;       /* (batch, seqlen, dim)                                         */
    void        *du, *dz;    /* (batch, seqlen, dim)                                         */
    void        *dxdbl;      /* (batch, seqlen, P + 32)                                      */
    float       *dA, *ddt_weight, *dD, *ddelta_bias;   /* dD / ddelta_bias may be NULL      */
    int64_t u_bs, u_ts, xdbl_bs, xdbl_ts, ypre_bs, ypre_ts, dout_bs, dout_ts, du_bs, du_ts, dz_bs, dz_ts, dxdbl_bs, dxdbl_ts;
    int32_t reverse_time;
    int32_t dt_rank;         /* P: 16 or 32                                                  */
} cm_scan_cl_bwd_dir;

typedef struct cm_scan_cl_bwd_args {
    int32_t batch, seqlen, dim, dstate;
    int32_t io_dtype;        /* CM_BF16 or CM_F32                                            */
    int32_t ndir;            /* 1 or 2                                                       */
    const void *z;           /* (batch, seqlen, dim), required                               */
    int64_t z_bs, z_ts;
    int32_t time_chunks;     /* 0: automatic (launches under 512 workgroups are cut along time: adjoint summaries per chunk,
                                a carry fold, then the full pass per chunk from its carried-in adjoint); 1: never; n: n chunks */
    int32_t overwrite;       /* 1: dA / ddt_weight / dD / ddelta_bias are written, not accumulated into */
    cm_scan_cl_bwd_dir dir[2];
    void   *stream;
    void   *workspace;       /* cm_scan_cl_bwd_workspace_bytes(args) bytes, 16-byte aligned  */
    int64_t workspace_bytes;
    int32_t da_log;          /* 1: dA is the gradient w.r.t. A_log of the reference's A = -exp(A_log) (bimamba.py:116-128), i.e. dA * A,
                                formed in the reduce pass (one element-wise launch per direction less in the caller)      */
    int32_t reserved0;
} cm_scan_cl_bwd_args;

int64_t cm_scan_cl_bwd_workspace_bytes(const cm_scan_cl_bwd_args *args);
/* the chunk count time_chunks = 0 resolves to */
int cm_scan_cl_bwd_auto_chunks(int batch, int seqlen, int dim, int ndir);
int cm_scan_cl_bwd(const cm_scan_cl_bwd_args *args);

/* ---------------------------------------------------------------------------------------
 * Channels-last causal conv, both BiMamba directions in one pass over x.
 *   y_fwd[b,t,c] = silu(bias_f[c] + sum_k w_f[c,k] x[b,t-(W-1)+k,c])      (causal,  bimamba.py:223-235)
 *   y_bwd[b,t,c] = silu(bias_b[c] + sum_k w_b[c,k] x[b,t+(W-1)-k,c])      (the reference's flipped branch,
 *                                                                           bimamba.py:236-248, un-flipped)
 * x, y_fwd, y_bwd: (batch, seqlen, dim), channel axis contiguous, strides in elements; width 4.
 * y_bwd / weight_b / bias_b may be NULL for a single (causal) direction.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_conv_cl_args {
    int32_t batch, seqlen, dim, width;
    int32_t io_dtype;            /* CM_BF16 or CM_F32 */
    int32_t silu;
    const void  *x;
    const float *weight_f, *bias_f, *weight_b, *bias_b;   /* (dim, width) / (dim); bias may be NULL */
    void *y_fwd, *y_bwd;
    int64_t x_bs, x_ts, yf_bs, yf_ts, yb_bs, yb_ts;
    void *stream;
} cm_conv_cl_args;

int cm_conv_cl_fwd(const cm_conv_cl_args *args);

/* Backward of cm_conv_cl_fwd / the conv half of cm_conv_xproj (both directions in one pass; replaces
 * causal_conv1d_cuda.causal_conv1d_bwd, selective_scan_interface.py:286-288, run once per direction by the reference):
 *   dx = dx_fwd + dx_bwd (the two directions share x: reference bimamba.py:223-248), pre-activations recomputed from x;
 *   dz = dz_f + dz_b (the two directions' shares of the gate gradient, cm_scan_cl_bwd) when dz != NULL;
 *   dweight_* (dim, 4), dbias_* (dim) fp32, ACCUMULATED into, summed in a fixed order through `workspace`.
 * du_b == NULL: one direction (the unidirectional mixer of the Mamba decoder).  Strides in elements. */
typedef struct cm_conv_cl_bwd_args {
    int32_t batch, seqlen, dim, width;
    int32_t io_dtype, pad_;
    const void  *x;                                       /* (batch, seqlen, dim) view                       */
    const float *weight_f, *bias_f, *weight_b, *bias_b;   /* (dim, 4) / (dim); biases may be NULL           */
    const void  *du_f, *du_b;                             /* gradients of u_fwd / u_bwd                      */
    const void  *dz_f, *dz_b;                             /* optional                                        */
    void *dx, *dz;                                        /* outputs; dz optional                            */
    float *dweight_f, *dbias_f, *dweight_b, *dbias_b;
    int64_t x_bs, x_ts, duf_bs, duf_ts, dub_bs, dub_ts, dzf_bs, dzf_ts, dzb_bs, dzb_ts, dx_bs, dx_ts, dz_bs, dz_ts;
    void *stream;
    float *workspace;                                     /* cm_conv_cl_bwd_workspace_floats() floats       */
    int64_t workspace_floats;
    int32_t overwrite;                                    /* 1: the parameter gradients are written, not accumulated into */
    int32_t reserved0;
} cm_conv_cl_bwd_args;

/* CTC loss + gradient (csrc/ctc.hip; replaces torch.nn.functional.ctc_loss behind speechbrain.nnet.losses.ctc_loss, reference
 * train_CTC.py:405): log_probs (batch, T, V) fp32 contiguous (log-softmax outputs), targets (batch, S) int64 padded, lengths int32.
 * nll[b] = negative log-likelihood (0 where no alignment exists: zero_infinity); grad (batch, T, V) fp32 = exp(lp) - posteriors
 * for t < input_lengths[b], 0 elsewhere -- the gradient torch returns for a unit upstream gradient per utterance (the caller
 * scales by grad_out / batch).  S <= 511; targets may be NULL exactly when S == 0 (every target empty: it is never read).
 * Deterministic (fixed summation order). */
typedef struct cm_ctc_args {
    int32_t batch, T, V, S, blank, Sx_max;   /* Sx_max: set by the library (2 S + 1)                          */
    const float   *log_probs;
    const int64_t *targets;
    const int32_t *input_lengths, *target_lengths;
    float *nll, *grad;
    float *workspace;                         /* cm_ctc_workspace_floats(batch, T, S) floats                    */
    int64_t workspace_floats;
    float *alpha, *beta;                      /* set by the library (views of workspace)                        */
    void *stream;
} cm_ctc_args;

int64_t cm_ctc_workspace_floats(int32_t batch, int32_t T, int32_t S);
int cm_ctc_loss(const cm_ctc_args *args);

/* CTC forced alignment (csrc/ctc_align.hip; contract: mamba_asr_amd/ctc_decode.py): the Viterbi path of a known
 * label sequence through the CTC trellis -- cm_ctc_loss's alpha recurrence with max for logsumexp, in float64 adds and strict
 * compares only, plus a backtrace.  One workgroup per utterance; bit-reproducible and independent of batch composition.
 * log_probs: lp_rows rows of (T, V) fp32 or bf16 with unit vocabulary stride, lp_bs / lp_ts elements apart; utterance b reads row
 * rows[b] (rows NULL: row b, and lp_rows >= batch), so hypotheses of one utterance share its frames; a row outside [0, lp_rows)
 * gives status 1.  targets (batch, S) int64 padded, NULL exactly when S == 0; ids at or past target_lengths[b] are never read; an
 * id outside [0, V) scores -inf.  n = min(input_lengths[b], T) frames and L = min(target_lengths[b], S) labels are aligned (negative
 * lengths count as 0).  S <= 1023.
 * Outputs: status[b] 0 aligned / 1 no alignment (score -inf) / 2 NaN on the lattice (score NaN); score (batch) fp64; states
 * (batch, T) int32 = the extended-sequence state of every frame < n, -1 elsewhere and wherever status != 0; starts / ends
 * (batch, S) int32 = first frame and one past the last frame of label j in state 2 j + 1, -1 for j >= L or status != 0;
 * label_logp (batch, S) fp64 = the left fold of the label's own frames' log-probabilities, 0 where starts is -1.
 * workspace: cm_ctc_align_workspace_bytes() bytes, 16-byte aligned (the moves, 2 bits per trellis cell).  Arguments are validated
 * on the host before any launch (CM_EINVAL / CM_EUNSUPPORTED / CM_EALIGN). */
typedef struct cm_ctc_align_args {
    int32_t batch, T, V, S, blank, dtype;     /* dtype: CM_F32 or CM_BF16                                       */
    int64_t lp_rows, lp_bs, lp_ts;            /* rows of log_probs; element strides of row and time             */
    const void *log_probs;
    const int64_t *targets;                   /* (batch, S)                                                     */
    const int32_t *input_lengths, *target_lengths;   /* (batch)                                                 */
    const int32_t *rows;                      /* (batch) or NULL                                                */
    double *score;                            /* (batch)                                                        */
    int32_t *status;                          /* (batch)                                                        */
    int32_t *states;                          /* (batch, T)                                                     */
    int32_t *starts, *ends;                   /* (batch, S); may be NULL when S == 0                            */
    double *label_logp;                       /* (batch, S); may be NULL when S == 0                            */
    void *workspace;                          /* cm_ctc_align_workspace_bytes() bytes                           */
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_align_args;

int64_t cm_ctc_align_workspace_bytes(const cm_ctc_align_args *args);
int cm_ctc_align(const cm_ctc_align_args *args);

/* Greedy CTC decode (csrc/ctc_greedy.hip; contract: mamba_asr_amd/ctc_decode.py): per frame the arg-max, repeats
 * collapsed, blanks removed, with the frames and the log-probability of every kept token.  Two kernels behind this one entry: the
 * arg-max of every frame < n on a grid over (utterance, frame tile), one wave per frame -- the only pass over log_probs -- and one
 * workgroup per utterance for keep flags, prefix sum, compaction, ends and the per-token sums.
 * log_probs: batch rows of (T, V) fp32 or bf16 with unit vocabulary stride, lp_bs / lp_ts elements apart, lp_ts >= V; any element
 * alignment (16-byte loads wherever the row allows, scalar head and tail).  n = min(input_lengths[b], T), negative counts as 0;
 * frames at and past n are never read.  No cap on T or V beyond one row spanning less than 2 GiB.
 * best[t] = the lowest index attaining the frame's maximum (-inf is an ordinary value: an all -inf frame gives 0).  Frame t is kept
 * when best[t] != blank and (t == 0 or best[t] != best[t-1]).  A NaN in any frame < n: status 2, token_len 0, every row entry -1 / 0.
 * Outputs: tokens / starts / ends (batch, T) int32 = kept token k, its first frame and one past the last frame of its run, -1 past
 * token_len[b]; token_logp (batch, T) fp64 = the left fold in increasing t of (double) lp[t][token] over the run, 0.0 past
 * token_len[b]; status (batch) int32 0 / 2.  workspace: cm_ctc_greedy_workspace_bytes() bytes, 16-byte aligned (the arg-max of every
 * frame).  Arguments are validated on the host before any launch (CM_EINVAL / CM_EUNSUPPORTED / CM_EALIGN). */
typedef struct cm_ctc_greedy_args {
    int32_t batch, T, V, blank, dtype;        /* dtype: CM_F32 or CM_BF16                                       */
    int64_t lp_bs, lp_ts;                     /* element strides of row and time                                */
    const void *log_probs;
    const int32_t *input_lengths;             /* (batch)                                                        */
    int32_t *tokens, *starts, *ends;          /* (batch, T)                                                     */
    int32_t *token_len;                       /* (batch)                                                        */
    double *token_logp;                       /* (batch, T)                                                     */
    int32_t *status;                          /* (batch)                                                        */
    void *workspace;                          /* cm_ctc_greedy_workspace_bytes() bytes                          */
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_greedy_args;

int64_t cm_ctc_greedy_workspace_bytes(const cm_ctc_greedy_args *args);
int cm_ctc_greedy(const cm_ctc_greedy_args *args);

/* Edit distance with alignment counts (csrc/edit_distance.hip; contract: mamba_asr_amd/metrics.py).  Pair p is
 * (refs[ref_index[p]][0 .. R), hyps[p][0 .. H)), R = ref_len[ref_index[p]] and H = hyp_len[p] clamped to [0, SR] / [0, SH]; ids at
 * or past a length are never read; many hypotheses may share a reference.  ref_index[p] outside [0, NR): status 1, everything 0.
 *   D[i][0] = i, D[0][j] = j; sub = D[i-1][j-1] + (a[i-1] != b[j-1]), del = D[i-1][j] + 1, ins = D[i][j-1] + 1;
 *   move: diagonal if sub < ins && sub < del, else delete if del < ins, else insert; D[i][j] = the move's value.
 * Backtrace from (R, H): diagonal -> (i-1, j-1), a hit when the tokens are equal, else a substitution; delete -> (i-1, j);
 * insert -> (i, j-1); row 0 is all inserts, column 0 all deletes.  All arithmetic is int32.
 * Outputs: counts (N, 4) int32 = [ins, del, sub, hits]; dist (N) int32 = D[R][H]; status (N) int32; with ops != NULL also ops
 * (N, SR + SH) int8 = the path in forward order as the characters '=', 'I', 'D', 'S' (0 past n_ops[p]) and n_ops (N) int32.
 * One workgroup per pair: thread j owns hypothesis column j + 1 and walks the anti-diagonals; moves at 2 bits per cell in the
 * workspace; wave 0 backtraces.  Limits: 0 <= SR <= CM_EDIT_MAX_LEN and 0 <= SH <= CM_EDIT_MAX_LEN, anything longer is
 * CM_EUNSUPPORTED.  workspace: cm_edit_distance_workspace_bytes() bytes, 16-byte aligned.  Arguments are validated on the host
 * before any launch (CM_EINVAL / CM_EUNSUPPORTED / CM_EALIGN). */
#define CM_EDIT_MAX_LEN 1024
typedef struct cm_edit_distance_args {
    int32_t N, NR, SR, SH;
    const int32_t *refs, *ref_len;            /* (NR, SR), (NR); refs may be NULL when SR == 0                  */
    const int32_t *hyps, *hyp_len;            /* (N, SH), (N); hyps may be NULL when SH == 0                    */
    const int32_t *ref_index;                 /* (N)                                                            */
    int32_t *counts;                          /* (N, 4)                                                         */
    int32_t *dist, *status;                   /* (N)                                                            */
    int8_t *ops;                              /* (N, SR + SH) or NULL                                           */
    int32_t *n_ops;                           /* (N); required with ops                                         */
    void *workspace;                          /* cm_edit_distance_workspace_bytes() bytes                       */
    int64_t workspace_bytes;
    void *stream;
} cm_edit_distance_args;

int64_t cm_edit_distance_workspace_bytes(const cm_edit_distance_args *args);
int cm_edit_distance(const cm_edit_distance_args *args);

/* LM-free CTC beam search (csrc/ctc_beam.hip; replaces speechbrain.decoders.ctc.CTCBeamSearcher, reference train_CTC.py:309-310,
 * 411-414 and 1155-1161).  The algorithm (mamba_asr_amd/ctc_decode.py): per processed frame select tokens, extend
 * every beam, merge equal (text, partial word, last token), prune by beam_prune_logp, rank, keep beam_size, optionally prune the
 * history; finish by merging equal texts.  Scores are float64.  One workgroup per utterance; bit-reproducible and independent of
 * batch composition.  log_probs (batch, T, V) fp32 or bf16 with unit vocabulary stride; lengths[b] = frames to decode (<= T).
 * Token classes and hashes come from the host: tok_class[v] = 1 for a word-start piece, 0 otherwise (blank's entry is ignored);
 * tok_hash[v][k] = H_k(clean piece) and tok_pow[v][k] = base_k^len(clean piece), H_k(s) = sum_i (cp_i + 1) base_k^(n-1-i) mod
 * 2^61 - 1 over the piece's code points.  hash_sep is the separator symbol (a value above every code point + 1).
 * Outputs per utterance: num_hyps[b] hypotheses (<= topk), for each its text-changing tokens tokens[b][h][0 .. token_len[b][h])
 * and its score; bad_frame[b] = first frame < lengths[b] holding a NaN (then num_hyps[b] = 0), else -1.
 * cm_ctc_beam_search validates its arguments on the host before any launch. */
typedef struct cm_ctc_beam_args {
    int32_t batch, T, V, dtype;               /* dtype: CM_F32 or CM_BF16; V <= 4096                           */
    int64_t lp_bs, lp_ts;                     /* log_probs element strides of batch and time                    */
    const void *log_probs;
    const int32_t *lengths;                   /* (batch) frames to decode                                       */
    const int32_t *tok_class;                 /* (V)                                                            */
    const uint64_t *tok_hash, *tok_pow;       /* (V, 2)                                                         */
    uint64_t hash_base[2], hash_sep;
    int32_t blank, beam_size, topk, prune_history;   /* beam_size <= 256                                        */
    double beam_prune_logp, token_prune_min_logp, blank_skip_threshold;   /* skip frame if lp[blank] > log(threshold) */
    double blank_skip_log;                    /* set by the library                                             */
    int32_t *tokens;                          /* (batch, topk, T)                                               */
    int32_t *token_len;                       /* (batch, topk)                                                  */
    double *scores;                           /* (batch, topk)                                                  */
    int32_t *num_hyps, *bad_frame;            /* (batch)                                                        */
    void *workspace;                          /* cm_ctc_beam_workspace_bytes() bytes                            */
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_beam_args;

int64_t cm_ctc_beam_workspace_bytes(const cm_ctc_beam_args *args);
int cm_ctc_beam_search(const cm_ctc_beam_args *args);

/* CTC beam search with a backoff n-gram LM fused into the frame loop (csrc/ctc_beam_lm.hip; speechbrain's CTCBeamSearcher with
 * kenlm_model_path; contract: mamba_asr_amd/ctc_decode.py).  Everything cm_ctc_beam_search takes, with the same
 * meaning, plus the packed LM (mamba_asr_amd/ngram_lm.py builds it from an ARPA file) and tok_len[v], the code points of token v's
 * clean piece.  Steps 1 - 3 of the frame (select, extend, merge) act on the acoustic score; prune, rank and the beam_size cut act
 * on total = acoustic + LM(text) + partial_score(partial word).
 * Tables, all open addressing with linear probing from lm slot(key) & (cap - 1), caps powers of two, empty key = all ones:
 *   word table    word_keys (word_cap, 2) = the two 61-bit hashes H_k(word) (as tok_hash), word_ids (word_cap) -> word id < n_words;
 *   prefix set    prefix_keys (prefix_cap, 2): the hashes of every non-empty prefix of every unigram-list word;
 *   n-gram table  ngram_keys (ngram_cap) = (entry of the context as an n-gram << 32) | word id, ngram_vals -> entry < n_entries.
 * lm_prob / lm_backoff (n_entries) hold log10 p and the backoff weight (0 when the file has none) of every entry; the unigram of
 * word id w is entry w.  slot(key) = mix(key) for the n-gram table and mix(h0 * 0x9E3779B97F4A7C15 + h1) for the hash pairs, mix
 * being the splitmix64 finaliser.  A beam's LM state is the entries of its last 1 .. order-1 words (-1: not stored).
 * lm_bos: word id that starts every context (<s> when the boundary is scored and listed), lm_eos: word id scored at the finish
 * without beta (</s>, likewise), lm_unk: word id of <unk>; each -1 when absent.  word_score = alpha ln(10) lw + beta.
 * Outputs as cm_ctc_beam_search: scores = the acoustic score of each hypothesis, lm_scores = its total, by which they are ranked.
 * Every probe loop is bounded by its table's capacity and every id read from a table is range-checked, so a damaged table gives
 * wrong scores but neither spins nor reads out of bounds.  Arguments are validated on the host before any launch. */
typedef struct cm_ctc_beam_lm_args {
    int32_t batch, T, V, dtype;               /* dtype: CM_F32 or CM_BF16; V <= 4096                           */
    int64_t lp_bs, lp_ts;                     /* log_probs element strides of batch and time                    */
    const void *log_probs;
    const int32_t *lengths;                   /* (batch) frames to decode                                       */
    const int32_t *tok_class;                 /* (V)                                                            */
    const uint64_t *tok_hash, *tok_pow;       /* (V, 2)                                                         */
    const int32_t *tok_len;                   /* (V) code points of the clean piece                             */
    uint64_t hash_base[2], hash_sep;
    int32_t blank, beam_size, topk, prune_history;   /* beam_size <= 256                                        */
    double beam_prune_logp, token_prune_min_logp, blank_skip_threshold;
    double blank_skip_log;                    /* set by the library                                             */
    int32_t order, n_words;                   /* order in [1, 5]                                                */
    int32_t lm_bos, lm_eos, lm_unk, reserved0;
    int64_t n_entries, word_cap, prefix_cap, ngram_cap;
    const uint64_t *word_keys;                /* (word_cap, 2)                                                  */
    const int32_t *word_ids;                  /* (word_cap)                                                     */
    const uint64_t *prefix_keys;              /* (prefix_cap, 2)                                                */
    const uint64_t *ngram_keys;               /* (ngram_cap)                                                    */
    const int32_t *ngram_vals;                /* (ngram_cap)                                                    */
    const float *lm_prob, *lm_backoff;        /* (n_entries)                                                    */
    double alpha, beta, unk_score_offset;     /* finite                                                         */
    double alpha_ln10;                        /* set by the library                                             */
    int32_t *tokens;                          /* (batch, topk, T)                                               */
    int32_t *token_len;                       /* (batch, topk)                                                  */
    double *scores, *lm_scores;               /* (batch, topk)                                                  */
    int32_t *num_hyps, *bad_frame;            /* (batch)                                                        */
    void *workspace;                          /* cm_ctc_beam_lm_workspace_bytes() bytes                         */
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_beam_lm_args;

int64_t cm_ctc_beam_lm_workspace_bytes(const cm_ctc_beam_lm_args *args);
int cm_ctc_beam_lm_search(const cm_ctc_beam_lm_args *args);

/* The same search carried across streaming chunks (csrc/ctc_beam_stream.hip): one call consumes the next chunk of
 * every stream of a batch from a caller-owned state and runs the frame body of cm_ctc_beam_search on it (csrc/ctc_beam_impl.h,
 * shared), so after n frames in any chunking the hypotheses carry the bits cm_ctc_beam_search returns for lengths = n.
 * State: one slab of cm_ctc_beam_stream_state_bytes(beam_size, max_frames) bytes per slot, state_stride_bytes apart (a multiple of
 * 16, as the state pointer): a 16-byte header (live beams, processed frames, frames consumed, NaN frame + 1), the beam_size beams
 * as a struct of arrays (80 bytes each) and the history (max_frames x beam_size int32, (parent << 16) | (token + 1)); plain memory
 * without pointers -- copying a slab copies a stream.  An all-zero slab is a slot that was never reset.  The function returns 0
 * outside beam_size in [1, 256], max_frames in [1, 0x7fff0000 / 256].
 * Per call and slot b: reset[b] != 0 (reset may be NULL) starts the slot from the single initial beam; then chunk_len[b] (clamped
 * to [0, T]) rows of log_probs[b] are consumed -- no row past chunk_len[b] - 1 is read; then emit[b] != 0 (emit may be NULL)
 * writes the hypotheses as cm_ctc_beam_search does, tokens being (batch, topk, max_frames), without changing beams or history.  A
 * slot that neither consumes, resets nor emits returns at once: its output rows and status[b] are left unwritten.  T == 0 is a
 * reset / emit-only call (log_probs may then be NULL).
 * status[b]: -1 ok;  f >= 0: the first frame holding a NaN, counted from the reset -- stored in the state until the next reset, the
 * slot consumes nothing more and an emit gives num_hyps[b] = 0;  -2: the chunk was refused and the state left unchanged, because
 * it would take the slot past max_frames or because the slot was never reset (an emit then still returns what the state holds,
 * nothing for a slot never reset).
 * workspace: cm_ctc_beam_stream_workspace_bytes() bytes per call, the candidate sorts that outgrow LDS (0, and workspace may be
 * NULL, when beam_size x V <= 1024).  Arguments are validated on the host before any launch. */
typedef struct cm_ctc_beam_stream_args {
    int32_t batch, T, V, dtype;               /* batch: slots; T: rows per slot in this chunk; dtype CM_F32 or CM_BF16; V <= 4096 */
    int64_t lp_bs, lp_ts;                     /* log_probs element strides of slot and time                     */
    const void *log_probs;                    /* (batch, T, V)                                                  */
    const int32_t *chunk_len;                 /* (batch) rows of this chunk to consume; 0: idle                 */
    const int32_t *reset, *emit;              /* (batch) or NULL                                                */
    const int32_t *tok_class;                 /* (V)                                                            */
    const uint64_t *tok_hash, *tok_pow;       /* (V, 2)                                                         */
    uint64_t hash_base[2], hash_sep;
    int32_t blank, beam_size, topk, prune_history;   /* beam_size <= 256                                        */
    double beam_prune_logp, token_prune_min_logp, blank_skip_threshold;
    double blank_skip_log;                    /* set by the library                                             */
    void *state;                              /* batch slabs                                                    */
    int64_t state_stride_bytes;
    int32_t max_frames, reserved0;            /* frames per utterance (between two resets)                      */
    int32_t *tokens;                          /* (batch, topk, max_frames)                                      */
    int32_t *token_len;                       /* (batch, topk)                                                  */
    double *scores;                           /* (batch, topk)                                                  */
    int32_t *num_hyps, *status;               /* (batch)                                                        */
    void *workspace;
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_beam_stream_args;

int64_t cm_ctc_beam_stream_state_bytes(int32_t beam_size, int32_t max_frames);
int64_t cm_ctc_beam_stream_workspace_bytes(const cm_ctc_beam_stream_args *args);
int cm_ctc_beam_stream(const cm_ctc_beam_stream_args *args);

/* The LM-fused search carried across streaming chunks (csrc/ctc_beam_lm_stream.hip): cm_ctc_beam_stream's kernel
 * with the LM switch of cm_ctc_beam_lm_search on, so after n frames in any chunking the hypotheses carry the bits
 * cm_ctc_beam_lm_search returns for lengths = n: tokens, lengths, counts, scores (acoustic) and lm_scores (the total, which ranks).
 * Everything cm_ctc_beam_stream takes, with the same meaning -- reset, consume, emit, idle slots, T == 0, status -1 / NaN frame /
 * -2 as described there -- plus tok_len and the packed LM of cm_ctc_beam_lm_search with its constants.
 * State: one slab of cm_ctc_beam_lm_stream_state_bytes(beam_size, max_frames) bytes per slot = (16 + 116 beam_size + 4 beam_size
 * max_frames) rounded up to 16: the 16-byte header and the beam block of cm_ctc_beam_stream (80 bytes per beam), then the LM block
 * -- lm beam_size f64, ps beam_size f64, ctx 4 x beam_size int32, plen beam_size int32 (LM(text), partial_score, the entries of the
 * last 1 .. 4 words, the partial word's code points) -- then the history.  Plain memory without pointers, copying a slab copies a
 * stream, an all-zero slab is a slot that was never reset; a reset stores the initial LM state (ctx[0] = lm_bos when order >= 2)
 * beside the initial beam.  ctx holds entry numbers of the LM tables: a slab belongs to the tables (and lm_bos) it was advanced
 * with, and continuing it with others gives wrong scores -- nothing detects that.  Whatever a slab holds, no load or store leaves
 * it or the tables: on load every ctx outside [0, n_entries) reads as -1 and plen is clamped to >= 0.  The function returns 0
 * outside the limits of cm_ctc_beam_stream_state_bytes.
 * An emit of a reset slot without frames gives one hypothesis of no tokens, score 0 and lm_score = LM("") (the </s> term alone).
 * workspace: cm_ctc_beam_lm_stream_workspace_bytes() bytes, the rule of cm_ctc_beam_stream_workspace_bytes.  Arguments are validated
 * on the host before any launch: those of cm_ctc_beam_stream, the LM checks of cm_ctc_beam_lm_search, the state, the workspace. */
typedef struct cm_ctc_beam_lm_stream_args {
    int32_t batch, T, V, dtype;               /* batch: slots; T: rows per slot in this chunk; dtype CM_F32 or CM_BF16; V <= 4096 */
    int64_t lp_bs, lp_ts;                     /* log_probs element strides of slot and time                     */
    const void *log_probs;                    /* (batch, T, V)                                                  */
    const int32_t *chunk_len;                 /* (batch) rows of this chunk to consume; 0: idle                 */
    const int32_t *reset, *emit;              /* (batch) or NULL                                                */
    const int32_t *tok_class;                 /* (V)                                                            */
    const uint64_t *tok_hash, *tok_pow;       /* (V, 2)                                                         */
    const int32_t *tok_len;                   /* (V) code points of the clean piece                             */
    uint64_t hash_base[2], hash_sep;
    int32_t blank, beam_size, topk, prune_history;   /* beam_size <= 256                                        */
    double beam_prune_logp, token_prune_min_logp, blank_skip_threshold;
    double blank_skip_log;                    /* set by the library                                             */
    int32_t order, n_words;                   /* order in [1, 5]                                                */
    int32_t lm_bos, lm_eos, lm_unk, reserved0;
    int64_t n_entries, word_cap, prefix_cap, ngram_cap;
    const uint64_t *word_keys;                /* (word_cap, 2)                                                  */
    const int32_t *word_ids;                  /* (word_cap)                                                     */
    const uint64_t *prefix_keys;              /* (prefix_cap, 2)                                                */
    const uint64_t *ngram_keys;               /* (ngram_cap)                                                    */
    const int32_t *ngram_vals;                /* (ngram_cap)                                                    */
    const float *lm_prob, *lm_backoff;        /* (n_entries)                                                    */
    double alpha, beta, unk_score_offset;     /* finite                                                         */
    double alpha_ln10;                        /* set by the library                                             */
    void *state;                              /* batch slabs                                                    */
    int64_t state_stride_bytes;
    int32_t max_frames, reserved1;            /* frames per utterance (between two resets)                      */
    int32_t *tokens;                          /* (batch, topk, max_frames)                                      */
    int32_t *token_len;                       /* (batch, topk)                                                  */
    double *scores, *lm_scores;               /* (batch, topk)                                                  */
    int32_t *num_hyps, *status;               /* (batch)                                                        */
    void *workspace;
    int64_t workspace_bytes;
    void *stream;
} cm_ctc_beam_lm_stream_args;

int64_t cm_ctc_beam_lm_stream_state_bytes(int32_t beam_size, int32_t max_frames);
int64_t cm_ctc_beam_lm_stream_workspace_bytes(const cm_ctc_beam_lm_stream_args *args);
int cm_ctc_beam_lm_stream(const cm_ctc_beam_lm_stream_args *args);

/* CTC prefix scores for joint CTC/attention S2S decoding (csrc/ctc_prefix.hip; what speechbrain's CTCScorer adds to the decoder's
 * log-probabilities, the reference S2S recipes' `ctc_weight_decode`; DESIGN.md §4d holds the contract).  logp (U, T, V) fp32
 * contiguous CTC log-posteriors; n_u[u] frames of utterance u to use (clamped to [0, T] in the kernels).  Hypothesis row r belongs
 * to utterance row_utt[r]; its state is r_n / r_b (rows, T) (log-probability that frames 0..t emit exactly the prefix and end in a
 * non-blank / in a blank), psi_g (rows) (the prefix's log prefix probability) and last (rows) (its last token, -1 = empty prefix).
 *   cm_ctc_prefix_score    out[r][j] = psi(prefix + c) - psi_g[r] for c = j (K == 0, out is (rows, V)) or c = candidates[r][j]
 *                          (out is (rows, K)); -inf for blank, for a candidate outside [0, V) and for an impossible extension,
 *                          never NaN; for c == eos the prefix's own CTC log-likelihood.  No per-(row, c) state is stored.
 *   cm_ctc_prefix_advance  the state of prefix + tokens[r] into r_n_out / r_b_out / psi_out / last_out (not in place: the outputs
 *                          must not alias the inputs); tokens[r] == eos copies the row's state; blank or a token outside
 *                          [0, V) gives the impossible prefix (all -inf).
 * Fixed summation order, no atomics: a row's results do not depend on the other rows of the launch.  row_utt, n_u, last and
 * tokens are read on the device; a row whose row_utt lies outside [0, U) reads nothing and gets -inf.  The workgroup of
 * cm_ctc_prefix_score covers CM_CTC_PREFIX_TILE_C candidates and stages the row's phi in LDS CM_CTC_PREFIX_TCHUNK frames at a time. */
#define CM_CTC_PREFIX_TILE_C 64
#define CM_CTC_PREFIX_TCHUNK 512
typedef struct cm_ctc_prefix_args {
    int32_t U, T, V, rows;
    int32_t blank, eos, K, reserved0;         /* K: candidates per row; 0 = every token                         */
    const float *logp;                        /* (U, T, V)                                                      */
    const int32_t *n_u;                       /* (U)                                                            */
    const int32_t *row_utt;                   /* (rows)                                                         */
    const int32_t *last;                      /* (rows)                                                         */
    const float *r_n, *r_b;                   /* (rows, T)                                                      */
    const float *psi_g;                       /* (rows)                                                         */
    const int32_t *candidates;                /* score: (rows, K) or NULL                                       */
    float *out;                               /* score: (rows, K ? K : V)                                       */
    const int32_t *tokens;                    /* advance: (rows)                                                */
    float *r_n_out, *r_b_out, *psi_out;       /* advance: (rows, T) x 2, (rows)                                 */
    int32_t *last_out;                        /* advance: (rows)                                                */
    void *stream;
} cm_ctc_prefix_args;

int cm_ctc_prefix_score(const cm_ctc_prefix_args *args);
int cm_ctc_prefix_advance(const cm_ctc_prefix_args *args);

/* Per-token selection of an S2S beam search (csrc/beam_select.hip; s2s_decode.S2SBeamSearcher; DESIGN.md §4e holds the contract).
 * Hypothesis row r = u * B + k is beam slot k of utterance u.  Candidate (u, k, c), flat index k * V + c within its utterance:
 *   a   = -inf if c == eos and eos_blocked[u] != 0, else att[r][c]
 *   inc = a                          (delta == NULL)        or  a + weight * delta[r][c]
 *   s   = alive[r] + inc
 * as separately rounded fp32 operations (a multiply, then two adds; never an FMA).  A NaN s ranks as -inf; +0 and -0 tie.  Output
 * slot j of utterance u is the j-th candidate under (s descending, flat index ascending): a total order, so all B slots are always
 * filled -- with fewer than B finite candidates by -inf ones in index order (their score is -inf, whatever inc holds).
 * Two launches: every (row, chunk of CM_BEAM_SELECT_CHUNK tokens) keeps its best min(B, chunk length) in the workspace, then one
 * workgroup per utterance ranks them.  Integer LDS histograms only: bit-identical from run to run, and an utterance's result does
 * not depend on the other utterances of the launch.  Nothing is read on the host; an eos outside [0, V) never matches. */
#define CM_BEAM_SELECT_MAX_B 128
#define CM_BEAM_SELECT_CHUNK 5120
typedef struct cm_beam_select_args {
    int32_t U, B, V, eos;                     /* 1 <= B <= CM_BEAM_SELECT_MAX_B, V >= 1, B * V < 2^31           */
    const float *att;                         /* (U * B, V) decoder log-probabilities                           */
    const float *delta;                       /* (U * B, V) CTC prefix scores, or NULL                          */
    const float *alive;                       /* (U * B) running scores; -inf: dead slot                        */
    const int32_t *eos_blocked;               /* (U) or NULL                                                    */
    float weight;                             /* of delta                                                       */
    int32_t reserved0;
    float *score, *inc;                       /* out (U, B)                                                     */
    int32_t *parent, *token;                  /* out (U, B): parent slot in [0, B), token in [0, V)             */
    void *workspace;                          /* cm_beam_select_workspace_bytes(U, B, V) bytes, 8-byte aligned  */
    int64_t workspace_bytes;
    void *stream;
} cm_beam_select_args;

int64_t cm_beam_select_workspace_bytes(int32_t U, int32_t B, int32_t V);   /* 0 for sizes cm_beam_select refuses */
int cm_beam_select(const cm_beam_select_args *args);

/* One decoding step of multi-head self-attention over a KV cache addressed through a beam-ancestry table (csrc/attn_step.hip;
 * modules/TransformerLM.py; DESIGN.md §4f holds the contract).  dh = D / H.  For hypothesis row r and head h:
 *   kc[t][r], vc[t][r] <- this step's k, v (the bits of qkv)
 *   x[s] = q . K[s][anc[s][r]] / sqrt(dh) for s < t,  x[t] = q . k;   p = softmax(x) in fp32;   out = sum over s of p[s] * V[s][..]
 * with position t's k and v taken from this launch's own copy, never from the cache: a row reads only cache lines written by
 * earlier launches.  anc[t][.] is not read.  An anc entry outside [0, R) is clamped for the load and scores -inf: it adds
 * nothing and is no out-of-bounds access.  fp32 arithmetic for both I/O dtypes; each dot product is an fma chain in ascending d,
 * the sum over s runs in ascending s; no atomics: bit-identical from run to run, and row r's result depends only on qkv[r],
 * anc[.][r] and the cache lines it names.  One launch; nothing is read on the host.
 * CM_EUNSUPPORTED (before any launch): io_dtype other than CM_F32 / CM_BF16, dh not 32 or 64, H > CM_ATTN_STEP_MAX_H,
 * t >= CM_ATTN_STEP_MAX_T (the scores live in LDS).  CM_EINVAL: NULL or misaligned pointers (16 bytes; anc 4), Lcap <= t,
 * kv_stride below R * D or not a multiple of 16 bytes. */
#define CM_ATTN_STEP_MAX_T 4096
#define CM_ATTN_STEP_MAX_H 32
typedef struct cm_attn_step_args {
    int32_t R, D, H, t;                       /* rows, model dimension, heads, positions cached so far          */
    int32_t Lcap, io_dtype;                   /* positions the caches and anc hold (> t); CM_F32 or CM_BF16     */
    int64_t kv_stride;                        /* elements between consecutive positions of kc and of vc         */
    const void *qkv;                          /* (R, 3 D) io: q | k | v of this step, bias added                */
    void *kc, *vc;                            /* (Lcap, R, D) io, position stride kv_stride                     */
    const int32_t *anc;                       /* (Lcap, R) contiguous                                           */
    void *out;                                /* (R, D) io                                                      */
    void *stream;
} cm_attn_step_args;

int cm_attn_step(const cm_attn_step_args *args);

/* One decoding step of multi-head CROSS-attention: R hypothesis rows over the encoder memory of their utterance
 * (csrc/xattn_step.hip; modules/Transformer.py; DESIGN.md §4g holds the contract).  K and V were projected once per utterance
 * and are shared by all rows of that utterance; nothing is written but out.  dh = D / H, u = row_utt[r], n = min(enc_len[u], T):
 *   out[r, h] = sum over s < n of softmax_s(q[r, h] . K[u, s, h] / sqrt(dh)) * V[u, s, h]
 * Frames s >= n are never loaded.  A row whose row_utt lies outside [0, U), or whose n < 1, gets zeros and loads nothing.
 * fp32 arithmetic for both I/O dtypes; each score is an fma chain in ascending d; the sum over s is formed in 64 / (lanes per
 * V row) interleaved partial sums, each in ascending s, folded in ascending order, then divided by the softmax denominator;
 * no atomics: bit-identical from run to run, and row r's result depends only on q[r] and on K / V of its utterance, not on R
 * or on the other rows of the launch.  One launch; nothing is read on the host.
 * k and v are (U, T, .) views: element strides per utterance and per frame, the frame stride at least D (K and V may be the
 * two halves of one (U, T, 2 D) projection).
 * CM_EUNSUPPORTED (before any launch): io_dtype other than CM_F32 / CM_BF16, dh not 32, 36 or 64, H > CM_XATTN_STEP_MAX_H,
 * T >= CM_XATTN_STEP_MAX_T (the fp32 scores of one (row, head) live in the LDS strip of its wave: T floats + 2 KiB of partial
 * sums, inside the 64 KiB a workgroup may ask for).  CM_EINVAL: NULL or misaligned pointers (16 bytes; row_utt / enc_len 4),
 * sizes below 1, D no multiple of H, a frame stride below D, an utterance stride below (T - 1) * frame stride + D, strides
 * that are no multiple of 16 bytes. */
#define CM_XATTN_STEP_MAX_T 8192
#define CM_XATTN_STEP_MAX_H 32
typedef struct cm_xattn_step_args {
    int32_t R, U, T, D, H, io_dtype;          /* rows, utterances, frames K / V hold, model dimension, heads; CM_F32 / CM_BF16 */
    int64_t k_utt_stride, k_frame_stride;     /* elements between utterances / frames of k                      */
    int64_t v_utt_stride, v_frame_stride;     /* the same of v                                                  */
    const void *q;                            /* (R, D) io, contiguous                                          */
    const void *k, *v;                        /* (U, T, D) io views with the strides above                      */
    const int32_t *row_utt;                   /* (R): the utterance of each row                                 */
    const int32_t *enc_len;                   /* (U): valid frames of each utterance                            */
    void *out;                                /* (R, D) io, contiguous                                          */
    void *stream;
} cm_xattn_step_args;

int cm_xattn_step(const cm_xattn_step_args *args);

/* Element-wise stages of a feed-forward / convolution module's training step on (rows, dim) tensors (csrc/ffn_train.hip; the
 * reference leaves them to torch: reference modules/Conmamba.py:597-617):
 *   cm_bias_act_dropout_fwd   y = dropout(act(a + bias))  [I/O dtype]      or, with res:  y = res + alpha * dropout(a + bias)  [fp32]
 *   cm_bias_act_dropout_bwd   da = alpha * dy * mask / (1 - p) * act'(a + bias)  [I/O dtype];  dbias += column sums of da (fixed order)
 * act: 0 none, 1 GELU (erf form), 2 GLU (a and da are (rows, 2 dim), bias / dbias (2 dim); no dropout, no residual).  mask: one byte per element, NULL = no dropout (eval, or p == 0); the forward draws it from a
 * counter hash of (seed, element index).  dim: multiple of 8, <= 2048; tensors contiguous, 16-byte aligned. */
#define CM_SEED_EPOCH_MUL 0x9E3779B97F4A7C15ull
typedef struct cm_ffn_elem_args {
    int64_t rows;
    int32_t dim, io_dtype, act, dy_f32;      /* dy_f32: backward's dy is fp32 although io_dtype is bf16 (the residual stream)   */
    const void  *a;                           /* (rows, dim) I/O dtype: the GEMM output without bias (backward: needed when act)  */
    const float *bias;                        /* (dim) or NULL                                                                     */
    const float *res;                         /* forward, optional: (rows, dim) fp32 residual                                      */
    void        *y;                           /* forward out: I/O dtype, or fp32 with res                                          */
    uint8_t     *mask;                        /* (rows, dim) bytes or NULL.  p > 0 drops with or without it: forward stores the
                                                 decisions there when given; backward reads them, or re-derives them from seed     */
    const void  *dy;                          /* backward in                                                                       */
    void        *da;                          /* backward out, I/O dtype                                                           */
    float       *dbias;                       /* backward, optional: (dim) fp32, ACCUMULATED into                                  */
    float       *dbias_part;                  /* cm_bias_act_dropout_bwd_workspace_floats(rows, dim) floats, required with dbias   */
    float p, alpha;
    uint64_t seed;                            /* dropout stream (cm_dropout.h): element e of the (rows, dim) tensor                */
    void *stream;
    void        *act_out;                     /* backward, optional (act 1, bf16): dropout(GELU(a + bias)) recomputed -- what the
                                                 training forward of cm_ffn_fused fed to its second GEMM                            */
    int32_t overwrite;                        /* 1: dbias is written, not accumulated into (no memset in front of the call)        */
    int32_t reserved0;
    const uint64_t *seed_epoch;               /* optional DEVICE word: the stream's seed is seed + *seed_epoch * CM_SEED_EPOCH_MUL
                                                 (mod 2^64), read when the kernel runs -- a captured hipGraph whose first node
                                                 advances the word draws fresh decisions at every replay                            */
} cm_ffn_elem_args;

int64_t cm_bias_act_dropout_bwd_workspace_floats(int64_t rows, int32_t dim);
int cm_bias_act_dropout_fwd(const cm_ffn_elem_args *args);
int cm_bias_act_dropout_bwd(const cm_ffn_elem_args *args);

/* out[j] = sum over b < nbatch of in[b * n + j], fp32 accumulation in a fixed order: folds the per-utterance weight-gradient
 * products of the training step (the reference forms them as one K = batch * time GEMM inside autograd).  in / out dtype:
 * CM_F32 or CM_BF16; n a multiple of 8 (bf16 in) / 4 (fp32 in); 16-byte aligned. */
int cm_sum_leading(const void *in, void *out, int32_t nbatch, int64_t n, int32_t in_dtype, int32_t out_dtype, void *stream);

/* Reflect padding by `pad` of the time and frequency axes of a dense channels-last (batch, time, freq, channels) tensor -- the 'same'
 * padding in front of every Conv2d of the reference's front end (speechbrain ConvolutionFrontEnd, hparams/CTC/conmamba_large.yaml:187-194).
 *   backward = 0: dst (batch, time + 2 pad, freq + 2 pad, channels) = padded src
 *   backward = 1: src is the padded tensor's gradient, dst (batch, time, freq, channels) its fold back onto the source positions
 * dtype CM_F32 / CM_BF16; 1 <= pad, 2 pad < time, freq. */
int cm_reflect_pad_tf(const void *src, void *dst, int32_t batch, int32_t time, int32_t freq, int32_t channels, int32_t pad,
                      int32_t dtype, int32_t backward, void *stream);

/* ---------------------------------------------------------------------------------------
 * Weight gradient of a Linear: out (m, n) fp32 = sum over rows k of a[k, :m]^T b[k, :n]  (dW = dY^T X; the reference leaves it to
 * autograd: one GEMM with K = batch x time per Linear, modules/Conmamba.py:597-650, selective_scan_interface.py:262-284).
 * a (rows, m), b (rows, n) bf16, row strides lda / ldb in elements (multiples of 8); m, n multiples of 128.  Split over row chunks into
 * workspace (cm_wgrad_workspace_floats floats), folded in a fixed order: deterministic.  out is WRITTEN.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_wgrad_args {
    int32_t rows, m, n;
    int32_t variant;             /* 0: the library picks; 1: tiles travel through registers (2 buffers); 2: global -> LDS directly
                                    (LDS-DMA) through a 4-stage ring, three 32-row steps in flight; 3: LDS-DMA, 2 buffers of 64 rows */
    const void *a, *b;
    int64_t lda, ldb;
    float *out;
    float *workspace;
    int64_t workspace_floats;
    void *stream;
} cm_wgrad_args;

int cm_wgrad_supported(int32_t rows, int32_t m, int32_t n);
int64_t cm_wgrad_workspace_floats(int32_t rows, int32_t m, int32_t n);
int cm_wgrad_bf16(const cm_wgrad_args *args);

int64_t cm_conv_cl_bwd_workspace_floats(int32_t batch, int32_t seqlen, int32_t dim);
int cm_conv_cl_bwd(const cm_conv_cl_bwd_args *args);

/* ---------------------------------------------------------------------------------------
 * cm_conv_cl_fwd for both directions fused with both directions' x_proj GEMMs (bf16 only):
 *   y_fwd, y_bwd as cm_conv_cl_fwd (SiLU applied), and
 *   xdbl[b,t, 0:48]  = y_fwd[b,t,:] @ Wx_f^T      xdbl[b,t,48:96] = y_bwd[b,t,:] @ Wx_b^T
 * where Wx_* is the direction's x_proj.weight re-rowed to (48, dim) = [dt rows zero-padded to 16 | B rows | C rows]
 * (reference selective_scan_interface.py:186 followed by the split of :187-215), bf16, in the fragment-tiled image
 * cm_ffn_pack_weights produces.  xdbl (batch, seqlen, 96) bf16 is what cm_scan_cl_fwd's xdbl mode reads.
 * dim: multiple of 32.  Strides in elements, multiples of 4.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_conv_xproj_args {
    int32_t batch, seqlen, dim, width;
    const void  *x;
    const float *weight_f, *bias_f, *weight_b, *bias_b;   /* (dim, 4) / (dim); biases may be NULL */
    const void  *wx_f, *wx_b;                             /* packed (dt_pad + 32, dim) bf16       */
    void *y_fwd, *y_bwd, *xdbl;
    int64_t x_bs, x_ts, yf_bs, yf_ts, yb_bs, yb_ts, xdbl_bs, xdbl_ts;
    void *stream;
    int32_t dt_pad;                                       /* 0 / 16: x_dbl rows [dt16 | B | C] per direction (96 columns in all);
                                                             32: [dt32 | B | C] (128 columns), the layout cm_scan_cl_fwd's xdbl
                                                             mode takes for 16 < dt_rank <= 32                                   */
    int32_t variant;                                      /* tuning: 0 = tile shape chosen from the problem size; 1 = always the
                                                             16-step tiles (the shape small launches get)                        */
} cm_conv_xproj_args;

int cm_conv_xproj(const cm_conv_xproj_args *args);
/* Whole utterances of different lengths in one batch: utterance b has L = min(max(lens[b], 0), seqlen) rows.  The
 * buffer descriptors of x, y_fwd and y_bwd of utterance b end behind row L - 1, so the backward direction's taps past the last row
 * read the conv's zero padding and stores past it are dropped; xdbl rows at and past L are not written; tiles past row L - 1 exit.
 * Rows [0, L) of y_fwd, y_bwd and xdbl carry the bits of cm_conv_xproj on that utterance alone with seqlen = L under the same tile
 * shape; L == 0 reads nothing and writes nothing.  The tile shape follows cm_conv_xproj's rule on (batch, seqlen): at
 * batch * ceil(seqlen / 32) >= 512 the 32-step tiles run, whose xdbl differs from a batch-1 call's (16-step tiles) within bf16
 * rounding; y_fwd / y_bwd are the same bits under either shape.  lens: `batch` int32 in DEVICE memory; NULL is refused. */
int cm_conv_xproj_lens(const cm_conv_xproj_args *args, const int32_t *lens);

/* ---------------------------------------------------------------------------------------
 * ONE causal direction of cm_conv_xproj with a history input (bf16 only): the UniMamba mixer of the causal encoder
 * (reference modules/Conmamba.py:580-584), whole utterances or a stream of chunks.
 *   y[b,t,:]    = SiLU(conv4([x_hist | x])[b,t,:])      xdbl[b,t, 0:dt_pad+32] = y[b,t,:] @ Wx^T
 * x_hist (batch, 3, dim) contiguous holds the three rows in front of this chunk; NULL = zeros (the start of an
 * utterance).  x_hist_out (batch, 3, dim) contiguous, optional, receives the last three rows of [x_hist | x] (right for
 * seqlen 1 and 2 too): the next chunk's x_hist.  x_hist_out must not overlap x_hist -- other workgroups of the launch
 * still read it -- so a caller keeps two buffers and swaps them (CM_EINVAL otherwise).  Chunked or whole, y and xdbl
 * come out bit for bit the same.  dim, strides, alignment: as cm_conv_xproj; x_hist / x_hist_out 8-byte aligned.
 * Every check is made before anything is launched.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_conv_xproj_uni_args {
    int32_t batch, seqlen, dim, width;
    const void  *x;
    const float *weight, *bias;                           /* (dim, 4) / (dim) or NULL             */
    const void  *wx;                                      /* packed (dt_pad + 32, dim) bf16       */
    void *y, *xdbl;                                       /* (batch, seqlen, dim) / (batch, seqlen, dt_pad + 32) */
    const void *x_hist;                                   /* (batch, 3, dim) or NULL              */
    void *x_hist_out;                                     /* (batch, 3, dim) or NULL              */
    int64_t x_bs, x_ts, y_bs, y_ts, xdbl_bs, xdbl_ts;
    void *stream;
    int32_t dt_pad;                                       /* 0 / 16 or 32, as cm_conv_xproj_args.dt_pad */
    int32_t variant;                                      /* as cm_conv_xproj_args.variant        */
} cm_conv_xproj_uni_args;

int cm_conv_xproj_uni(const cm_conv_xproj_uni_args *args);
/* The same launch with per-slot lengths: x_hist_out[b] receives the last three rows of [x_hist[b] | x[b, :L]],
 * L = min(max(lens[b], 0), seqlen) -- x_hist[b] itself for L == 0 -- written by the workgroup whose tile holds row L - 1.  y and
 * xdbl are computed for all seqlen rows as by cm_conv_xproj_uni; rows at and past L are unspecified, and nothing at or past row
 * L of x reaches a row in front of it or x_hist_out.  lens: `batch` int32 in DEVICE memory; NULL is refused (CM_EINVAL).
 * The tile shape follows cm_conv_xproj_uni's rule on (batch, seqlen): at batch * ceil(seqlen / 32) >= 512 the 32-step tiles run, and
 * xdbl then carries the bits of cm_conv_xproj_uni at the same (batch, seqlen), which differ from those of a batch-1 call (16-step
 * tiles) within bf16 rounding; y and x_hist_out are the same bits under either shape. */
int cm_conv_xproj_uni_slots(const cm_conv_xproj_uni_args *args, const int32_t *lens);

/* ---------------------------------------------------------------------------------------
 * Residual add + LayerNorm(s) over the last axis (rows x dim), fused:
 *   r   = x + alpha * y                       (y optional; x fp32 residual stream)
 *   if norm1: r1 = LN(r; g1, b1, eps1) else r1 = r
 *   if x_out: x_out = r1 (fp32)               -- new residual stream (may alias x)
 *   if norm2: out = LN(r1; g2, b2, eps2) else out = r1;  written in out_dtype if out != NULL
 * Covers the four residual/normalisation seams of ConmambaEncoderLayer.forward
 * (reference modules/Conmamba.py:638-649) and the encoder's final norm (:725).
 * dim: a multiple of 4, at most 1024.  Every check is made before anything is launched.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_add_ln_args {
    int64_t rows;
    int32_t dim;
    int32_t y_dtype;             /* dtype of y: CM_F32 or CM_BF16 (read when y != NULL); anything else, CM_F16 included: CM_EUNSUPPORTED */
    int32_t out_dtype;           /* dtype of out: CM_F32 or CM_BF16 (read when out != NULL); anything else: CM_EUNSUPPORTED             */
    int32_t out_act;             /* activation applied to `out`: 0 none, 1 LeakyReLU(0.01); other values: CM_EUNSUPPORTED */
    const float *x;              /* (rows, dim) fp32, 16-byte aligned (CM_EALIGN), or NULL (treated as zeros)            */
    const void  *y;              /* (rows, dim) y_dtype, or NULL; x and y both NULL: CM_EINVAL */
    float alpha;
    float eps1, eps2;
    int32_t pad2_;
    const float *g1, *b1;        /* first LN (applied to the residual) or NULL  */
    const float *g2, *b2;        /* second LN (produces `out`) or NULL          */
    float *x_out;                /* (rows, dim) fp32, 16-byte aligned (CM_EALIGN), or NULL */
    void  *out;                  /* (rows, dim) out_dtype or NULL               */
    void  *stream;
} cm_add_ln_args;

int cm_add_layernorm(const cm_add_ln_args *args);

/* ---------------------------------------------------------------------------------------
 * ConvolutionModule core, channels-last (reference modules/Conmamba.py:441-449 between the two
 * GEMMs): GLU over the channel axis -> depthwise conv over time (kernel K odd, 'same' zero padding)
 * + bias -> LayerNorm(dim) -> GELU.   in: (batch, seqlen, 2*dim)  out: (batch, seqlen, dim)
 * ------------------------------------------------------------------------------------- */
typedef struct cm_glu_dwconv_args {
    int32_t batch, seqlen, dim, ksize;
    int32_t io_dtype;
    int32_t glu_done;            /* 0: in is (batch, seqlen, 2*dim) and the GLU is applied here;
                                    1: in is (batch, seqlen, dim), already gated (cm_ln_pw_glu)      */
    const void  *in;             /* (batch, seqlen, 2*dim), contiguous               */
    const float *weight;         /* (dim, ksize) depthwise taps                       */
    const float *bias;           /* (dim) or NULL                                      */
    const float *ln_g, *ln_b;    /* (dim)                                              */
    float eps;
    int32_t variant;             /* tuning: 0 = kernel chosen from dtype / dim; 1 = always the generic 16-step kernel  */
    void *out;                   /* (batch, seqlen, dim), contiguous                   */
    void *stream;
    const float *weight_t;       /* optional (ksize, dim) copy of the taps: per-channel reads become coalesced */
    const void  *lin_w;          /* optional: the module's closing Linear(dim, dim) (reference Conmamba.py:156-158) applied to
                                    the tile before it is stored: (dim, dim) bf16 in cm_ffn_pack_weights' image; bf16 rows of
                                    dim 256 only.  out = GELU(LayerNorm(conv)) @ lin_w^T + lin_b                          */
    const float *lin_b;          /* (dim) fp32, required with lin_w                                                       */
} cm_glu_dwconv_args;

int cm_glu_dwconv_ln_gelu(const cm_glu_dwconv_args *args);
/* Whole utterances of different lengths in one batch (the non-causal 'same'-padding form, every kernel of it, with
 * and without the Linear epilogue): utterance b has L = min(max(lens[b], 0), seqlen) rows.  Staged rows t >= L are zero -- the
 * 'same' padding starts behind the utterance's own last row -- rows of `out` at and past L are not written, tiles past row L - 1
 * exit.  Rows [0, L) carry the bits of cm_glu_dwconv_ln_gelu on that utterance alone with seqlen = L; L == 0 reads nothing and
 * writes nothing.  lens: `batch` int32 in DEVICE memory; NULL is refused (CM_EINVAL). */
int cm_glu_dwconv_ln_gelu_lens(const cm_glu_dwconv_args *args, const int32_t *lens);

/* ---------------------------------------------------------------------------------------
 * The same core for ConvolutionModule(causal=True) (reference modules/Conmamba.py:230-238, :445-446: pad both sides by
 * ksize - 1, chomp the tail = all ksize - 1 padding rows in front), with a history input for a stream of chunks.
 * Fields as cm_glu_dwconv_args, and:
 *   hist     (batch, ksize - 1, dim) contiguous, I/O dtype: the GATED rows (the GLU's outputs) in front of this chunk;
 *            NULL = zeros (the start of an utterance);
 *   hist_out (batch, ksize - 1, dim) contiguous, optional: the last ksize - 1 rows of [hist | this chunk's gated rows]
 *            (right for seqlen < ksize - 1 too): the next chunk's hist.  It must not overlap hist -- other workgroups of
 *            the launch still read it -- so a caller keeps two buffers and swaps them (CM_EINVAL otherwise).
 * Chunked or whole, `out` comes out bit for bit the same.  hist: 16-byte aligned where rows are whole 16-byte pieces,
 * else 4; hist_out: 4-byte aligned.  Every check is made before anything is launched.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_glu_dwconv_causal_args {
    int32_t batch, seqlen, dim, ksize;
    int32_t io_dtype;
    int32_t glu_done;
    const void  *in;
    const float *weight;
    const float *bias;
    const float *ln_g, *ln_b;
    float eps;
    int32_t variant;
    void *out;
    void *stream;
    const float *weight_t;
    const void  *lin_w;
    const float *lin_b;
    const void  *hist;
    void        *hist_out;
} cm_glu_dwconv_causal_args;

int cm_glu_dwconv_ln_gelu_causal(const cm_glu_dwconv_causal_args *args);
/* The same launch with per-slot lengths: hist_out[b] receives the last ksize - 1 rows of
 * [hist[b] | gated rows [0, L) of utterance b], L = min(max(lens[b], 0), seqlen) -- hist[b] itself for L == 0 -- written by the
 * workgroup whose tile holds gated row L - 1 from its staged rows.  `out` is computed for all seqlen rows; rows at and past L are
 * unspecified, and nothing at or past row L of `in` reaches a row in front of it or hist_out.  lens: `batch` int32 in DEVICE
 * memory; NULL is refused (CM_EINVAL). */
int cm_glu_dwconv_ln_gelu_causal_slots(const cm_glu_dwconv_causal_args *args, const int32_t *lens);

/* ---------------------------------------------------------------------------------------
 * Single-step (decode-time) updates of a Mamba mixer: the two calls of bimamba.Mamba.step (reference
 * modules/mamba/bimamba.py:320-365).  All tensors contiguous; states are fp32 and updated IN PLACE.
 *   cm_causal_conv1d_update (causal_conv1d.causal_conv1d_update, :337-343 / fallback :331-336):
 *     conv_state (batch, dim, width) <- shifted left by one with x (batch, dim) appended;
 *     out[b,c] = [silu](bias[c] + sum_k weight[c,k] * conv_state[b,c,k])
 *   cm_selective_state_update (mamba_ssm selective_state_update, :360-362 / fallback :350-358):
 *     dt' = [softplus](dt + dt_bias);  state[b,c,n] <- state * exp(dt' * A[c,n]) + dt' * B[b,n] * x[b,c];
 *     out[b,c] = (sum_n state[b,c,n] * C[b,n] + D[c] * x[b,c]) * [silu(z[b,c])]
 * ------------------------------------------------------------------------------------- */
typedef struct cm_conv_update_args {
    int32_t batch, dim, width;
    int32_t io_dtype;            /* x, out                                          */
    int32_t silu;
    int32_t pad_;
    const void  *x;              /* (batch, dim)                                    */
    float       *conv_state;     /* (batch, dim, width) fp32, in place              */
    const float *weight;         /* (dim, width)                                    */
    const float *bias;           /* (dim) or NULL                                   */
    void        *out;            /* (batch, dim)                                    */
    void *stream;
} cm_conv_update_args;

typedef struct cm_state_update_args {
    int32_t batch, dim, dstate;
    int32_t io_dtype;            /* x, dt, B, C, z, out                             */
    int32_t dt_softplus;
    int32_t pad_;
    float       *state;          /* (batch, dim, dstate) fp32, in place             */
    const void  *x, *dt;         /* (batch, dim)                                    */
    const float *A;              /* (dim, dstate)                                   */
    const void  *B, *C;          /* (batch, dstate)                                 */
    const float *D;              /* (dim) or NULL                                   */
    const void  *z;              /* (batch, dim) or NULL                            */
    const float *dt_bias;        /* (dim) or NULL                                   */
    void        *out;            /* (batch, dim)                                    */
    void *stream;
} cm_state_update_args;

int cm_causal_conv1d_update(const cm_conv_update_args *args);
int cm_selective_state_update(const cm_state_update_args *args);

/* ---------------------------------------------------------------------------------------
 * One decoding step of a Mamba mixer between in_proj and out_proj in ONE launch (mamba_step.hip): what UniMamba.step
 * otherwise does with cm_causal_conv1d_update, the x_proj GEMM, the dt_proj GEMM and cm_selective_state_update
 * (reference modules/mamba/bimamba.py:331-362).  Per batch row b, with x_in = xz[b, :dim] and z = xz[b, dim:]:
 *   conv_state[b,c,:] <- (conv_state[b,c,1:], x_in[c]);  x[c] = silu(conv_bias[c] + sum_k conv_weight[c,k] conv_state[b,c,k])
 *   x_dbl[j] = sum_c x_proj_weight[j,c] x[c]                    j < dt_rank + 2 * 16:  [dt_low | B | C]
 *   dt[c]    = softplus(dt_bias[c] + sum_r dt_proj_weight[c,r] x_dbl[r])
 *   ssm_state[b,c,n] <- ssm_state[b,c,n] exp(dt[c] A[c,n]) + dt[c] B[n] x[c]
 *   out[b,c] = (sum_n ssm_state[b,c,n] C[n] + D[c] x[c]) silu(z[c])
 * All arithmetic between the loads and the stores is fp32; only xz and out are in io_dtype.  One workgroup per batch row, the
 * x_proj reduction through LDS in a fixed order: no atomics, bit-identical from run to run.  Both states are updated IN PLACE.
 * Built for dstate 16, dconv 4, dim a multiple of 8 up to 4096, 1 <= dt_rank <= 32, fp32 / bf16 I/O; anything else returns
 * CM_EUNSUPPORTED and launches nothing.  All tensors contiguous; the fp32 tensors 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_mamba_step_args {
    int32_t batch, dim, dstate, dconv, dt_rank;
    int32_t io_dtype;              /* xz, out                                         */
    const void  *xz;               /* (batch, 2 * dim): in_proj's output [x | z]      */
    float       *conv_state;       /* (batch, dim, dconv) fp32, in place, oldest first */
    float       *ssm_state;        /* (batch, dim, dstate) fp32, in place             */
    const float *conv_weight;      /* (dim, dconv)                                    */
    const float *conv_bias;        /* (dim) or NULL                                   */
    const float *x_proj_weight;    /* (dt_rank + 2 * dstate, dim)                     */
    const float *dt_proj_weight;   /* (dim, dt_rank)                                  */
    const float *dt_bias;          /* (dim) or NULL                                   */
    const float *A;                /* (dim, dstate), = -exp(A_log)                    */
    const float *D;                /* (dim) or NULL                                   */
    void        *out;              /* (batch, dim)                                    */
    void *stream;
} cm_mamba_step_args;

int cm_mamba_step(const cm_mamba_step_args *args);

/* ---------------------------------------------------------------------------------------
 * Depthwise Conv1d over time, forward and backward, on the module API's (batch, dim, seqlen) time-contiguous layout:
 * the ConvolutionModule's depthwise stage (reference modules/Conmamba.py:271-284, called at :443; nn.Conv1d with
 * groups = dim, stride 1, zero padding).  Output length = seqlen.
 *   y[b,c,t]  = bias[c] + sum_k weight[c,k] * x[b,c,t + k - pad_left]        (x = 0 outside [0, seqlen))
 *   dx[b,c,s] = sum_k weight[c,k] * dy[b,c,s - k + pad_left]
 *   dweight[c,k] += sum_{b,t} dy[b,c,t] * x[b,c,t + k - pad_left];   dbias[c] += sum_{b,t} dy[b,c,t]
 * pad_left = ksize/2 for 'same' padding, ksize-1 for the causal variant (padding then chomp, :445-446).
 * ksize <= 32.  dweight / dbias are fp32 and accumulated into (caller zero-initialises); deterministic (no atomics).
 * ------------------------------------------------------------------------------------- */
typedef struct cm_dwconv1d_args {
    int32_t batch, dim, seqlen, ksize, pad_left;
    int32_t io_dtype;            /* CM_BF16 or CM_F32: x, y, dy, dx                     */
    const void  *x;
    const float *weight;         /* (dim, ksize)                                        */
    const float *bias;           /* (dim) or NULL                                       */
    void        *y;              /* forward only                                        */
    const void  *dy;             /* backward only                                       */
    void        *dx;
    float       *dweight;        /* (dim, ksize)                                        */
    float       *dbias;          /* (dim) or NULL                                       */
    int64_t x_bs, x_ds, y_bs, y_ds, dy_bs, dy_ds, dx_bs, dx_ds;   /* batch / channel strides in elements */
    void *stream;
} cm_dwconv1d_args;

int cm_dwconv1d_fwd(const cm_dwconv1d_args *args);
int cm_dwconv1d_bwd(const cm_dwconv1d_args *args);

/* The same operator on CHANNELS-LAST rows (batch, seqlen, dim), channel axis contiguous, strides in elements: with it
 * the ConvolutionModule stays in the (batch, time, channel) layout end to end (pointwise conv = GEMM on rows, GLU over
 * the last axis), without transposing copies.  Same formulas as cm_dwconv1d_*.  The backward writes per-workgroup
 * partial tap gradients to `partial` (cm_dwconv_cl_workspace_floats(batch, seqlen, dim) fp32, caller-owned) and sums
 * them in a fixed order (deterministic); dweight / dbias are accumulated into. */
typedef struct cm_dwconv_cl_args {
    int32_t batch, dim, seqlen, ksize, pad_left;
    int32_t io_dtype;
    const void  *x;
    const float *weight;         /* (dim, ksize) */
    const float *bias;           /* (dim) or NULL */
    void        *y;              /* forward only  */
    const void  *dy;             /* backward only */
    void        *dx;
    float       *dweight;
    float       *dbias;
    float       *partial;        /* backward workspace */
    int64_t x_bs, x_ts, y_bs, y_ts, dy_bs, dy_ts, dx_bs, dx_ts;
    void *stream;
    int32_t overwrite;           /* backward: 1 = dweight / dbias are written, not accumulated into */
    int32_t reserved0;
} cm_dwconv_cl_args;

int64_t cm_dwconv_cl_workspace_floats(int32_t batch, int32_t seqlen, int32_t dim);
int cm_dwconv_cl_fwd(const cm_dwconv_cl_args *args);
int cm_dwconv_cl_bwd(const cm_dwconv_cl_args *args);

/* ---------------------------------------------------------------------------------------
 * LayerNorm over the last axis with saved statistics, forward and backward (training path).  Replaces torch's
 * LayerNorm behind the reference's normalisations: modules/Conmamba.py:262, :287 (ConvolutionModule), :597-620
 * (feed-forward pre-norms, norm1, norm2), :687 (final norm) -- under autocast torch runs them in fp32 whatever the
 * input type, so x may be bf16 while y is fp32.
 *   fwd: y = (x - mean) * rstd * gamma + beta over rows of `dim` (multiple of 4, <= 4096: the CNN front end normalises
 *        over (frequency, channel) = 2560), contiguous; mean / rstd
 *        (rows) fp32 are written when given (both or neither).
 *   bwd: dx (x_dtype, may be NULL) and dgamma / dbeta (dim, OVERWRITTEN) from dy (y_dtype), x, mean, rstd, gamma;
 *        workspace: cm_layernorm_bwd_workspace_floats(rows, dim) fp32, caller-owned; fixed summation order.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_layernorm_args {
    int64_t rows;
    int32_t dim;
    int32_t x_dtype, y_dtype;    /* CM_F32 or CM_BF16 */
    float   eps;
    const void  *x;
    const float *gamma, *beta;
    void  *y;                    /* forward  */
    float *mean, *rstd;          /* forward: written (optional); backward: read */
    const void *dy;              /* backward */
    void  *dx;
    float *dgamma, *dbeta;
    float *workspace;
    void  *stream;
    const float *dres;           /* backward, optional: (rows, dim) fp32 added to dx (the residual branch's gradient: the
                                    pre-norm block's dx = dres + LayerNorm'(dy) in one pass); fp32 x and dim <= 1024 only */
    /* optional epilogue y = act(LN(x)) * chan_mask[row / mask_rows][col % mask_c] -- the front end's Conv2d block tail (LayerNorm over
       (freq, channel) -> LeakyReLU -> Dropout2d, one keep / (1 - p) factor per (sample, channel)); the backward recomputes LN's
       output for the activation's derivative and needs beta then */
    int32_t act;                 /* 0 none, 1 LeakyReLU(act_slope)                                                          */
    float   act_slope;
    const float *chan_mask;      /* (rows / mask_rows, mask_c) fp32 or NULL; mask_c a multiple of 4 dividing dim            */
    int32_t mask_rows, mask_c;
} cm_layernorm_args;

int64_t cm_layernorm_bwd_workspace_floats(int64_t rows, int32_t dim);
int cm_layernorm_fwd(const cm_layernorm_args *args);
int cm_layernorm_bwd(const cm_layernorm_args *args);

/* ---------------------------------------------------------------------------------------
 * Mixer -> convolution-module seam in one kernel (bf16 GEMM operands, d_model 256):
 *   x_out = x + alpha * y;  h = LayerNorm(x_out; ln_g, ln_b, eps);  pw = h @ W^T + bias  (W: (2*dim, dim));
 *   out = pw[:, :dim] * sigmoid(pw[:, dim:])                  (reference modules/Conmamba.py:639-640, 441-443)
 * x (rows, 256) fp32; y (rows, 256) bf16 or NULL; w: the pointwise Conv1d weight (512, 256) bf16 packed with
 * cm_ffn_pack_weights; bias (512) fp32; x_out (rows, 256) fp32 (may alias x) or NULL; out (rows, 256) bf16, which
 * cm_glu_dwconv_ln_gelu takes with glu_done = 1.
 * dim = 144 (the ConMamba-small recipes) is taken too, with 144 / 288 for 256 / 512: w is then the image of the (288, 144)
 * weight padded with zero columns to (288, 160) -- whole 32-column tiles; the kernel zeroes the matching columns of its token
 * tile itself, and the LayerNorm statistics are over the 144 features.  Any other dim: CM_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_ln_pw_glu_args {
    int32_t rows, dim;
    const float *x;
    const void  *y;
    const float *ln_g, *ln_b;
    const void  *w;
    const float *bias;
    float *x_out;
    void  *out;
    float alpha, eps;
    void *stream;
} cm_ln_pw_glu_args;

int cm_ln_pw_glu(const cm_ln_pw_glu_args *args);

/* The same seam with the mixer's out_proj in front: y = ycat @ proj_w^T is formed inside the kernel (rounded to bf16 as a
 * GEMM's output would be) and never reaches memory.  ycat (rows, proj_k) bf16 contiguous; proj_w (256, proj_k) bf16 packed
 * with cm_ffn_pack_weights; proj_k a multiple of 128, at most 8192.  The other fields are cm_ln_pw_glu_args'.  out and
 * x_out may overlap no input, except x_out == x.  dim 256 only (CM_EUNSUPPORTED otherwise). */
typedef struct cm_ln_pw_glu_mix_args {
    int32_t rows, dim;
    const float *x;
    const float *ln_g, *ln_b;
    const void  *w;
    const float *bias;
    float *x_out;
    void  *out;
    float alpha, eps;
    void *stream;
    const void *ycat;
    const void *proj_w;
    int32_t proj_k;
} cm_ln_pw_glu_mix_args;

int cm_ln_pw_glu_mix(const cm_ln_pw_glu_mix_args *args);

/* ---------------------------------------------------------------------------------------
 * First block of the CNN front end (speechbrain ConvolutionFrontEnd as configured at reference
 * hparams/CTC/conmamba_large.yaml:187-194): Conv2d(1 -> C, 3x3, stride 2 in time and frequency, reflect
 * 'same' padding) -> LayerNorm over (freq, channel) -> LeakyReLU(0.01), fused, channels-last.
 *   in : feats (batch, T, F) fp32
 *   out: (batch, T1 + 2*pad_out, F1 + 2*pad_out, C) io_dtype, T1 = ceil(T/2), F1 = ceil(F/2); with pad_out = 1 the
 *        reflect border the NEXT 3x3 stride-2 block needs is written as well, so that block runs unpadded.
 *   T >= 5 and F >= 5 (that border reflects over three output rows / bins): fewer -> CM_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_cnn_block1_args {
    int32_t batch, T, F, C;
    int32_t io_dtype;            /* output dtype                                           */
    int32_t pad_out;             /* 0 or 1                                                 */
    const float *feats;          /* (batch, T, F)                                          */
    const float *weight;         /* (C, 1, 3, 3)                                           */
    const float *bias;           /* (C)                                                    */
    const float *ln_g, *ln_b;    /* (F1, C)                                                */
    float eps, slope;
    void *out;
    void *stream;
} cm_cnn_block1_args;

int cm_cnn_block1(const cm_cnn_block1_args *args);

/* ---------------------------------------------------------------------------------------
 * Second block of the CNN front end (same reference lines as cm_cnn_block1): Conv2d(64 -> 32, 3x3, stride 2,
 * no padding -- the reflect border is already in the input) -> LayerNorm over (freq, channel) -> LeakyReLU, bf16.
 *   in    : (batch, T_in, F_in, 64) bf16 channels-last  (cm_cnn_block1's output with pad_out = 1)
 *   weight: (32, 3, 3, 64) bf16 -- output channel, tap row, tap column, input channel (a torch Conv2d weight in
 *           channels_last memory format)
 *   out   : (batch, T2, F2 * 32) bf16,  T2 = (T_in - 3) / 2 + 1,  F2 = (F_in - 3) / 2 + 1
 * ------------------------------------------------------------------------------------- */
typedef struct cm_cnn_block2_args {
    int32_t batch, T_in, F_in, C_in, C_out;
    int32_t pad_;
    const void  *in;
    const void  *weight;
    const float *bias;           /* (32) or NULL                                           */
    const float *ln_g, *ln_b;    /* (F2, 32)                                               */
    float eps, slope;
    void *out;
    void *stream;
} cm_cnn_block2_args;

int cm_cnn_block2(const cm_cnn_block2_args *args);

/* ---------------------------------------------------------------------------------------
 * Both CNN front-end blocks in one kernel: cm_cnn_block1 (pad_out = 1) followed by cm_cnn_block2, without the
 * (batch, T/2 + 2, F/2 + 2, 64) intermediate ever reaching memory.  F = 80 bins, channels (64, 32).
 *   feats: (batch, T, 80) fp32      out: (batch, T2, 20 * 32) bf16,  T1 = ceil(T/2),  T2 = (T1 - 1) / 2 + 1
 *   w1 (64, 1, 3, 3) fp32, b1 (64), ln1_g / ln1_b (40, 64);  w2 (32, 3, 3, 64) bf16 (OHWI), b2 (32) fp32, ln2 (20, 32)
 * ------------------------------------------------------------------------------------- */
typedef struct cm_cnn_front_args {
    int32_t batch, T, F, C1, C2;
    int32_t pad_;
    const float *feats;
    const float *w1, *b1, *ln1_g, *ln1_b;
    const void  *w2;
    const float *b2, *ln2_g, *ln2_b;
    float eps1, eps2, slope;
    int32_t pad2_;
    void *out;
    void *stream;
} cm_cnn_front_args;

int cm_cnn_front(const cm_cnn_front_args *args);
/* Whole utterances of different lengths in one batch: utterance b has T_b = min(max(frames[b], 0), T) feature
 * frames, T1_b = ceil(T_b / 2) block-1 rows and T2_b = ceil(T1_b / 2) output rows.  Both reflections happen at the utterance's own
 * ends (T_b and T1_b), rows at and past T2_b are not computed or written, feature frames at and past T_b are never read.  Rows
 * [0, T2_b) carry the bits of cm_cnn_front on that utterance alone with T = T_b.  T_b < 5 (0 included) reads nothing and writes
 * nothing.  feats (batch, T, 80) and out (batch, ceil(ceil(T / 2) / 2), 640) keep the strides of the struct's T.
 * frames: `batch` int32 in DEVICE memory; NULL is refused (CM_EINVAL). */
int cm_cnn_front_lens(const cm_cnn_front_args *args, const int32_t *frames);

/* ---------------------------------------------------------------------------------------
 * bf16 MFMA GEMM with fused epilogues for the ConMamba layer's projections:
 *     acc[m, n] = sum_k A[m, k] * W[n, k]            (A: activations, W: nn.Linear weight layout)
 *   epilogue 0:  out = acc + bias                                          -> bf16   (in_proj, pointwise conv)
 *   epilogue 1:  out = gelu(acc + bias)   (erf form, nn.GELU default)      -> bf16   (FFN up-projection)
 *   epilogue 2:  r = x + alpha * (acc + bias);  r1 = LN1(r) if g1 else r;  x = r1 (fp32, in place);
 *                out = LN2(r1) if g2 (bf16, optional)                                (FFN down-projection, out_proj and
 *                the conv-module Linear: the residual/LayerNorm seams of reference modules/Conmamba.py:638-649)
 * Requirements: K % 64 == 0, N % 256 == 0 (epilogue 2: N == 256 so that one workgroup owns whole rows),
 * A/W/out 16-byte aligned with leading dimensions multiples of 8 elements.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_gemm_args {
    int32_t M, N, K;
    int32_t epilogue;
    const void  *A;  int64_t lda;      /* (M, K) bf16                                       */
    const void  *W;  int64_t ldw;      /* (N, K) bf16                                       */
    const float *bias;                 /* (N) fp32 or NULL                                  */
    void        *out; int64_t ldo;     /* (M, N) bf16; optional for epilogue 2              */
    float       *x;                    /* epilogue 2: (M, N) fp32 residual stream, in place */
    float alpha, eps1, eps2;
    int32_t pad_;
    const float *g1, *b1, *g2, *b2;    /* epilogue 2 LayerNorm parameters (N) or NULL       */
    void *stream;
} cm_gemm_args;

int cm_gemm_bf16(const cm_gemm_args *args);

/* ---------------------------------------------------------------------------------------
 * Position-wise feed-forward module of a ConMamba layer, one kernel (reference modules/Conmamba.py:631-650 around
 * speechbrain's PositionalwiseFeedForward: LayerNorm -> Linear(256, hidden) -> GELU -> Linear(hidden, 256), scaled
 * residual, then the layer's next LayerNorm).  d_model is 256; hidden a multiple of 256.
 *     xin   = x + add_scale * addend                (addend optional: the previous module's bf16 output)
 *     r     = xin + alpha * (W2 gelu(W1 LN_pre(xin) + b1) + b2)
 *     r     = LN_1(r)          if n1_g             (the layer's closing norm2)
 *     x_out = r                if x_out            (fp32 residual stream; may alias x)
 *     h_out = LN_2(r)          if h_out            (LN_2 skipped when n2_g is NULL), dtype h_dtype (bf16 or f32)
 * The hidden activations stay in LDS; GEMM operands are bf16 with fp32 accumulation.
 * w1 / w2 are passed in the PACKED layout produced by cm_ffn_pack_weights (once per weight update): the (R, K) matrix
 * cut into 16-row x 32-column tiles, each stored as the 1 KB register image of an MFMA operand fragment -- element
 * (r, k) of tile (r/16, k/32) sits at 16-bit index  tile*512 + ((k%32)/8*16 + r%16)*8 + k%8,  tile = (r/16)*(K/32) + k/32.
 * cm_ffn_pack_weights needs rows % 16 == 0 and cols % 32 == 0; a matrix that is no whole number of tiles is padded with zeros
 * by the caller first.
 * dim = 144 (the ConMamba-small recipes; inference forward, layout 0 only -- layout 1, tokens = 32 or any training field:
 * CM_EUNSUPPORTED) reads 144 for 256 above, with every image padded to whole tiles: w1 = image of (hidden, 144) padded with
 * zero columns to (hidden, 160), w2 = image of (144, hidden) padded with zero rows to (160, hidden), proj_w = image of
 * (proj_dim, 144) padded to (proj_dim, 160).  proj_dim is then a multiple of 64 (576 = 2 d_inner of the recipe) instead of 256.
 * The kernel writes the pad columns of its token tiles as zeros itself; the padded output features are never stored and never
 * enter a LayerNorm sum.  hidden stays a multiple of 256, at most 2048.  Any other dim: CM_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------- */
int cm_ffn_pack_weights(const void *w /* (rows, cols) bf16 row-major */, int32_t rows, int32_t cols,
                        void *out /* rows*cols bf16 */, void *stream);

typedef struct cm_ffn_args {
    int32_t rows, dim, hidden;
    int32_t h_dtype;                    /* CM_BF16 or CM_F32                                 */
    const float *x;                     /* (rows, dim) fp32; dim = 256 or 144                */
    const void  *addend;                /* (rows, dim) bf16 or NULL                          */
    const float *pre_g, *pre_b;         /* (dim) LayerNorm in front of the first Linear      */
    const void  *w1;                    /* (hidden, dim) bf16, packed (144: 160 columns)     */
    const float *b1;                    /* (hidden) fp32                                     */
    const void  *w2;                    /* (dim, hidden) bf16, packed (144: 160 rows)        */
    const float *b2;                    /* (dim) fp32                                        */
    const float *n1_g, *n1_b;           /* optional LayerNorm applied to the stream          */
    const float *n2_g, *n2_b;           /* optional LayerNorm producing h_out                */
    float       *x_out;                 /* (rows, dim) fp32 or NULL                          */
    void        *h_out;                 /* (rows, dim) h_dtype or NULL                       */
    float add_scale, alpha, pre_eps, n1_eps, n2_eps;
    int32_t proj_dim;                   /* rows of proj_w (a multiple of 256 -- of 64 at dim 144 --, <= 4096); 0 without a projection */
    void *stream;
    /* optional: the Linear that consumes h, applied to the tile in the same kernel -- the BiMamba in_proj behind the
       layer's first feed-forward module (reference bimamba.py:192-200):  proj_out = LN2(r) @ proj_w^T (+ proj_b), bf16;
       h_out must be NULL then (h is not stored) */
    const void  *proj_w;                /* (proj_dim, dim) bf16, cm_ffn_pack_weights' image (144: 160 columns)             */
    const float *proj_b;                /* (proj_dim) fp32 or NULL                                                          */
    void        *proj_out;              /* (rows, proj_dim) bf16                                                            */
    /* optional, the TRAINING forward of the module (reference modules/Conmamba.py:597-617 with its two Dropouts live):
         x_out = x + alpha * drop_p2( W2 drop_p1( GELU( bf16(W1 LN(x) + b1) ) ) + b2 )
       with what the backward needs stored on the way: pre_out = bf16(W1 LN(x) + b1) and xn_out = bf16(LN(x)).  Dropout
       decisions are cm_dropout.h's function of (seed, element index in the (rows, hidden) / (rows, 256) tensor): no mask is
       stored, cm_bias_act_dropout_bwd re-derives it.  Requires x_out, no addend / n1 / n2 / projection / h_out. */
    void        *pre_out;               /* (rows, hidden) bf16 or NULL                                                      */
    void        *xn_out;                /* (rows, 256) bf16 or NULL                                                         */
    float p1, p2;                       /* dropout probabilities behind the activation / behind the second Linear           */
    uint64_t seed1, seed2;
    float       *stats_out;             /* (2, rows) fp32 or NULL: mean, 1/std of LN(x)'s rows, as cm_layernorm_bwd reads them */
    int32_t layout;                     /* 0: w1 / w2 / proj_w in cm_ffn_pack_weights' image (16-row x 32-column tiles, v_mfma_f32_16x16x32_bf16);
                                           1: in cm_ffn_pack_weights32's (32 x 16 tiles, v_mfma_f32_32x32x16_bf16; inference forward only) */
    int32_t tokens;                     /* layout 1: tokens per workgroup, 0 / 64 or 32 (32: for launches of fewer than ~400 64-token
                                           workgroups, which leave CUs idle) */
    const uint64_t *seed_epoch;         /* optional device word added into seed1 / seed2 (cm_ffn_elem_args.seed_epoch)       */
    int32_t flags;                      /* CM_FFN_* bits                                                                  */
    int32_t reserved_;
} cm_ffn_args;
/* cm_ffn_args.flags.  Without it, when alpha is a power of two, the inference forward (layout 0) fetches the residual rows once and
   carries them in the second GEMM's accumulators (scaled by 1 / alpha, which is exact); with it, or any other alpha, the rows are
   loaded a second time behind the last GEMM, as before.  The results differ in the order of the fp32 residual add only. */
#define CM_FFN_RELOAD_RESIDUAL 1

int cm_ffn_fused(const cm_ffn_args *args);
/* row-major (rows, cols) bf16 -> the 32-row x 16-column fragment-tile image of cm_ffn_args.layout = 1 (rows % 32 == 0, cols % 16 == 0) */
int cm_ffn_pack_weights32(const void *w, int32_t rows, int32_t cols, void *out, void *stream);

/* The data-gradient chain of the same module's backward (what autograd does over modules/Conmamba.py:597-617 with two Dropout, two
 * addmm and one GELU backward), for the forward cm_ffn_fused's training variant ran (same dropout seeds):
 *   da2 = alpha * dout * keep2 / (1 - p2);  dg = da2 @ W2;  da1 = dg * keep1 / (1 - p1) * GELU'(pre);  act = drop1(GELU(pre));
 *   dh = da1 @ W1;  db2 = column sums of da2;  db1 = column sums of da1 (fixed order: deterministic)
 * w2t = W2^T (hidden, 256), w1t = W1^T (256, hidden): bf16 in cm_ffn_pack_weights' image.  da2 / da1 / act are stored for the weight
 * gradients (cm_wgrad_bf16), dh (bf16) for the LayerNorm backward in front of the module.  d_model 256, hidden a multiple of 256. */
typedef struct cm_ffn_bwd_args {
    int32_t rows, dim, hidden, reserved0;
    const float *dout;                  /* (rows, 256) fp32: gradient of the module's output (the residual stream)          */
    const void  *w2t, *w1t;
    const void  *pre;                   /* (rows, hidden) bf16: cm_ffn_args.pre_out of the forward                          */
    void *da2;                          /* (rows, 256) bf16 out                                                             */
    void *da1, *act;                    /* (rows, hidden) bf16 out                                                          */
    void *dh;                           /* (rows, 256) bf16 out                                                             */
    float *db1, *db2;                   /* (hidden), (256) fp32 out (written); db2 = db1 + hidden: ONE (hidden + 256) buffer     */
    float alpha, p1, p2;
    float reserved1;
    uint64_t seed1, seed2;
    float *workspace;                   /* cm_ffn_bwd_workspace_floats(rows, hidden) floats                                  */
    int64_t workspace_floats;
    void *stream;
    float *db1_part, *db2_part;         /* internal (set by the library)                                                    */
    const uint64_t *seed_epoch;         /* the forward's (cm_ffn_args.seed_epoch): same device word, same value at run time */
} cm_ffn_bwd_args;

int64_t cm_ffn_bwd_workspace_floats(int32_t rows, int32_t hidden);
int cm_ffn_bwd_fused(const cm_ffn_bwd_args *args);

/* ---------------------------------------------------------------------------------------
 * Fbank back end (speechbrain Fbank semantics as used at reference train_CTC.py:285 and configured at
 * hparams/CTC/conmamba_large.yaml:322-326): STFT (re, im) -> power -> triangular mel filterbank -> 10*log10 with
 * floor `amin`, plus the per-utterance maximum needed by the top_db clamp.
 *   spec : (batch, n_freq, frames, 2) fp32  -- torch.stft(..., return_complex=True) viewed as real
 *   fbank: (n_freq, n_mels) fp32
 *   db   : (batch, frames, n_mels) fp32  (out)      umax : (batch) fp32, initialised to -inf by the caller (out)
 * cm_fbank_finish then applies  db = max(db, umax[b] - top_db)  and optionally the global normalisation
 * (db - mean[m]) / std[m]  (speechbrain InputNormalization, train_CTC.py:287) in place.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_fbank_args {
    int32_t batch, n_freq, frames, n_mels;
    const float *spec;
    const float *fbank;
    float *db;
    float *umax;
    float amin, top_db;
    const float *mean, *std;     /* (n_mels) or NULL: used by cm_fbank_finish            */
    const int32_t *band_lo, *band_hi;   /* optional (n_mels): filter m is non-zero only on bins [lo, hi) */
    const int32_t *band_off;            /* optional (n_mels + 1): offsets into band_w                    */
    const float   *band_w;              /* optional: filter m's weights for bins lo..hi-1, packed (sum of band widths
                                           <= 4096 floats); staged in LDS instead of reading the dense matrix */
    int64_t spec_bs, spec_fs, spec_ts;  /* strides of spec in complex elements (batch, frequency, frame); all 0 =
                                           contiguous (batch, n_freq, frames).  torch.stft hands out a transposed view
                                           of a (batch, frames, n_freq) buffer: passing its strides avoids a 260 MB copy */
    void *stream;
    float *umax_part;            /* optional (batch, ceil(frames / 16)) scratch: cm_fbank_mel_db stores per-tile maxima
                                    there instead of issuing atomics on umax, and cm_fbank_finish reduces them into
                                    umax; pass the same args to both calls */
    /* cm_fbank_wav only: the STFT is computed in-kernel from the waveform (spec / spec_* are ignored) */
    const float *wav;            /* (batch, samples) fp32                                                        */
    const float *window;         /* (n_fft) fp32: the analysis window zero-padded (centred) to n_fft             */
    const float *twiddle;        /* (n_fft, 2) fp32: exp(-2 pi i k / n_fft), k = 0 .. n_fft - 1                  */
    int64_t wav_bs;              /* batch stride of wav in elements (even)                                        */
    int32_t samples, hop, n_fft; /* frames must equal 1 + samples / hop (center=True, zero padding); n_fft 512    */
    int32_t pad3_;
} cm_fbank_args;

int cm_fbank_mel_db(const cm_fbank_args *args);
int cm_fbank_finish(const cm_fbank_args *args);
/* waveform -> log-mel (before top_db / normalisation: follow with cm_fbank_finish on the same args).  Requires
 * umax_part and the packed band tables (band_lo, band_hi, band_off, band_w).  In-LDS radix-4 real FFT, n_fft = 512. */
int cm_fbank_wav(const cm_fbank_args *args);
/* Whole utterances of different lengths in one batch: utterance b has n_b = min(max(n_samples[b], 0), samples)
 * samples and T_b = 1 + n_b / hop frames (0 frames for n_b == 0).  cm_fbank_wav_lens: samples at and past n_b read as zero (the
 * waveform's buffer descriptor ends there), frames [0, T_b) are computed and the per-tile maxima in umax_part run over them only;
 * tiles past T_b store -inf.  cm_fbank_finish_lens (same args, same n_samples): the top_db maximum of utterance b runs over the
 * tiles of frames [0, T_b) only -- frames T_b and T_b + 1 of the padded batch still overlap real samples and can be the loudest --
 * and frames [0, T_b) are clamped and normalised.  Those frames carry the bits of cm_fbank_wav + cm_fbank_finish on that utterance
 * alone with samples = n_b; frames at and past T_b are unspecified (not written).  db (batch, frames, n_mels) and umax_part keep the
 * strides of the struct's frames.  n_samples: `batch` int32 in DEVICE memory; NULL is refused (CM_EINVAL). */
int cm_fbank_wav_lens(const cm_fbank_args *args, const int32_t *n_samples);
int cm_fbank_finish_lens(const cm_fbank_args *args, const int32_t *n_samples);

/* ---------------------------------------------------------------------------------------
 * The Fbank and the CNN front end as a stream: waveform chunks in, encoder rows out.  All `batch` streams
 * advance in lock step; every count below is host arithmetic on the number of samples handed over so far.
 *
 * cm_fbank_wav_stream: frames [f0, f0 + nf) of every stream, cm_fbank_wav's arithmetic per frame (same bits).  Frame f reads the
 * samples [hop f - 256, hop f + 256) by their index in the utterance: index s < 0 and, at the end of the utterance
 * (total >= 0), s >= total read as zero; consumed <= s < consumed + n comes from chunk[b, s - consumed]; consumed - 512 <= s <
 * consumed from hist[b, s - consumed + 512].  Nothing else is read, and no sample outside those two arrays ever is.
 *   chunk    : (batch, n) fp32, batch stride chunk_bs elements; NULL when n = 0
 *   hist     : (batch, 512) fp32, the last 512 samples in front of the chunk (zeros in front of the utterance)
 *   hist_out : (batch, 512) fp32, receives the last 512 samples of [hist | chunk]; must not overlap hist (other workgroups
 *              of the launch still read it: CM_EINVAL) -- the caller swaps the two, the protocol of cm_conv_xproj_uni
 *   db       : (batch, nf, n_mels) fp32, the dB values before the top_db clamp (out)
 *   fmax     : (batch, nf) fp32, the maximum of each frame (out)
 * nf = 0 only rolls the history.  n_fft 512, n_mels <= 128, hop even; consumed + n < 2^30.
 *
 * cm_fbank_finish_stream (same args, after cm_fbank_wav_stream): the causal top_db clamp, the floor of frame f being
 * max(umax[b], fmax[b, f0 .. f]) - top_db, and the optional normalisation (v - mean[m]) / std[m], in place on db; umax[b]
 * (-inf at the start of an utterance) is updated in place to the maximum over all frames so far.  With feat_hist / feat_hist_out
 * it also rolls the feature history cm_cnn_front_stream reads: feat_hist_out (batch, 8, n_mels) receives the last 8 rows
 * of [feat_hist | db] (zeros in front of frame 0); the two must not overlap.
 * ------------------------------------------------------------------------------------- */
typedef struct cm_fbank_stream_args {
    int32_t batch, n_mels, n_fft, hop;
    int32_t n;                          /* samples per stream in this call, >= 0                                    */
    int32_t consumed;                   /* samples per stream handed over by earlier calls                          */
    int32_t total;                      /* samples of the whole utterance when this call ends it, else -1            */
    int32_t f0, nf;                     /* first frame and number of frames this call produces                      */
    int32_t pad_;
    const float *chunk;  int64_t chunk_bs;
    const float *hist;
    float *hist_out;
    const float *window;                /* (512) fp32: the analysis window zero-padded (centred) to n_fft           */
    const float *twiddle;               /* (512, 2) fp32: exp(-2 pi i k / 512)                                      */
    const int32_t *band_lo, *band_hi;   /* (n_mels): filter m is non-zero only on bins [lo, hi)                     */
    const int32_t *band_off;            /* (n_mels + 1): offsets into band_w                                        */
    const float *band_w;                /* the filters' weights on their bands, packed                              */
    float *db;
    float *fmax;
    float amin, top_db;
    float *umax;                        /* (batch) fp32, in / out: cm_fbank_finish_stream only                      */
    const float *mean, *std;            /* (n_mels) or NULL: cm_fbank_finish_stream only                            */
    const float *feat_hist;             /* (batch, 8, n_mels) or NULL: cm_fbank_finish_stream only                  */
    float *feat_hist_out;               /* (batch, 8, n_mels) or NULL                                               */
    void *stream;
} cm_fbank_stream_args;

int cm_fbank_wav_stream(const cm_fbank_stream_args *args);
int cm_fbank_finish_stream(const cm_fbank_stream_args *args);

/* cm_cnn_front's rows [r0, r0 + nr) of every stream, with its block-1 row routine, MFMA chain and LayerNorms (same bits).  Row r
 * reads the feature frames 4r - 3 .. 4r + 3 by their index in the utterance: frame f >= f0 comes from feats[b, f - f0], f0 - 8 <=
 * f < f0 from feat_hist[b, f - f0 + 8].  Index -1 reflects to 1 (features and block-1 rows); the reflection at the end,
 * T -> T - 2 and T1 -> T1 - 2, is taken only when the number of frames of the utterance is known (T_total >= 5, else -1).
 * The caller guarantees 4 (r0 + nr - 1) + 3 < f0 + nf, or T_total = f0 + nf, and 4 r0 - 3 >= f0 - 8.
 *   feats (batch, nf, 80) fp32, feat_hist (batch, 8, 80) fp32 (NULL: nothing in front of feats), out (batch, nr, 640) bf16;
 *   weights as cm_cnn_front_args. */
typedef struct cm_cnn_front_stream_args {
    int32_t batch, F, C1, C2;
    int32_t f0, nf;                     /* first frame of feats, frames in feats                                    */
    int32_t r0, nr;                     /* first row and number of rows this call produces                          */
    int32_t T_total;                    /* frames of the whole utterance when this call ends it, else -1            */
    int32_t pad_;
    const float *feats;
    const float *feat_hist;
    const float *w1, *b1, *ln1_g, *ln1_b;
    const void  *w2;
    const float *b2, *ln2_g, *ln2_b;
    float eps1, eps2, slope;
    int32_t pad2_;
    void *out;
    void *stream;
} cm_cnn_front_stream_args;

int cm_cnn_front_stream(const cm_cnn_front_stream_args *args);

/* The three streamed front-end launches with per-slot counts: every stream of the batch is at its own sample, ends
 * its utterance in its own call and may idle.  plan is a (batch, 8) int32 table, row b = {n, consumed, total, f0, nf, r0, nr,
 * T_total} of stream b with the meanings of the struct fields of the same names; the structs' own n, nf and nr are then the MAXIMA
 * over the streams -- the widths of chunk (batch, n), db (batch, nf, n_mels), fmax (batch, nf), feats (batch, nf, 80) and out
 * (batch, nr, 640) -- and their consumed / total / f0 / r0 / T_total are ignored.  plan_host is the table in host memory, checked
 * here stream by stream with the lock-step entry point's conditions before anything is launched; plan_dev is the same table in
 * DEVICE memory, read by the kernels.  Grids are sized by the maxima; workgroups past a stream's own frames or rows exit; rows of
 * db / out past a stream's own count are not written.  A stream with n = 0 or nf = 0 still has its sample history (and, when
 * cm_fbank_finish_stream_slots runs, its feature history) carried into the spare buffer.  Samples of chunk[b] at and past n[b] are
 * never read.  Per frame and per row the arithmetic and its bits are those of the lock-step kernels. */
int cm_fbank_wav_stream_slots(const cm_fbank_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev);
int cm_fbank_finish_stream_slots(const cm_fbank_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev);
int cm_cnn_front_stream_slots(const cm_cnn_front_stream_args *args, const int32_t *plan_host, const int32_t *plan_dev);

/* ---------------------------------------------------------------------------------------
 * SpecAugment masking (speechbrain SpectrogramDrop, reference hparams/CTC/conmamba_large.yaml:273-320 and
 * train_CTC.py:291): feats[b, t, f] = fill for every (b, t, f) covered by one of the utterance's masks along
 * `dim` (1 = time, 2 = frequency).  Mask starts/lengths are drawn by the host RNG: int32 (batch, n_masks).
 * ------------------------------------------------------------------------------------- */
typedef struct cm_spec_drop_args {
    int32_t batch, frames, n_mels, n_masks;
    int32_t dim;                 /* 1 = time masks, 2 = frequency masks                   */
    int32_t pad_;
    float *feats;                /* (batch, frames, n_mels) fp32, in place                */
    const int32_t *start;        /* (batch, n_masks)                                      */
    const int32_t *length;       /* (batch, n_masks)                                      */
    const float *fill;           /* device scalar: the replacement value (tensor mean)    */
    void *stream;
} cm_spec_drop_args;

int cm_spec_drop(const cm_spec_drop_args *args);

#ifdef __cplusplus
}
#endif
#endif /* CONMAMBA_HIP_H */
