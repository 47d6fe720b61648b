// ctc_beam_stream.hip — the CTC beam search carried across streaming chunks (contract: cm_ctc_beam_stream).  One
// workgroup per slot loads the slot's beams from its state slab into LDS, runs the frame loop of ctc_beam_impl.h -- the text
// cm_ctc_beam_search and cm_ctc_beam_lm_search run, here with the LM switch off (NoLm) -- over the chunk's rows, appending to the history inside the slab, stores the beams back and, when asked,
// finishes on the sort buffers and backtracks: an emit changes neither beams nor history.  Loading and storing the state moves the
// live beams only (plain vector loads and stores); nothing is shared between workgroups.
//
// Slab: int32 header {live beams, processed frames, frames consumed, NaN frame + 1} | score K f64 | ht, hp, pp, hw 2 x K u64 each |
// last, flags K i32 each | history max_frames x K i32.  Live beams == 0 is a slot that was never reset (an all-zero slab).
#include "ctc_beam_impl.h"

namespace {

constexpr int HDR_BYTES = 16;
constexpr int BEAM_BYTES = 8 + 4 * 2 * 8 + 2 * 4;      // score, four hash pairs, last and flags

int64_t state_bytes(int beam_size, int max_frames) {
    return (HDR_BYTES + (int64_t)BEAM_BYTES * beam_size + 4 * (int64_t)beam_size * max_frames + 15) / 16 * 16;
}

// the arrays of one slab
struct Slab {
    int32_t *hdr;
    double *score;
    uint64_t *ht, *hp, *pp, *hw;       // [2][K]
    int32_t *last, *flags, *hist;
};

__device__ __forceinline__ Slab slab_of(char *base, int K) {
    Slab s;
    s.hdr = reinterpret_cast<int32_t *>(base);
    s.score = reinterpret_cast<double *>(base + HDR_BYTES);
    s.ht = reinterpret_cast<uint64_t *>(s.score + K);
    s.hp = s.ht + 2 * K; s.pp = s.hp + 2 * K; s.hw = s.pp + 2 * K;
    s.last = reinterpret_cast<int32_t *>(s.hw + 2 * K);
    s.flags = s.last + K;
    s.hist = s.flags + K;
    return s;
}

template <class Lm, class P>
__global__ __launch_bounds__(NT) void ctc_beam_stream_kernel(const P p, int64_t ws_bytes, int n2max) {
    __shared__ Shared sh;
    [[maybe_unused]] constexpr typename Lm::Lds lb{};      // NoLm: no per-beam LM state (the slab holds none yet)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, K = p.beam_size, F = p.max_frames;
    const int asked = min(max(p.chunk_len[b], 0), p.T);
    const bool do_reset = p.reset && p.reset[b] != 0, do_emit = p.emit && p.emit[b] != 0;
    if (asked == 0 && !do_reset && !do_emit) return;
    const Slab st = slab_of(static_cast<char *>(p.state) + (int64_t)b * p.state_stride_bytes, K);
    int32_t *hist = st.hist;
    const Buf gbuf = global_buf(static_cast<char *>(p.workspace) + (int64_t)b * ws_bytes, n2max);
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    // the slot's search so far, its beams into sh.bm[0]; header values are clamped to the slab, whatever the memory holds
    int nb0 = 1, steps0 = 0, frames = 0, nan_frame = -1;
    const bool live = do_reset || st.hdr[0] > 0;
    if (do_reset) {
        if (tid == 0) store_initial_beam(sh.bm, 0);
    } else if (live) {
        nb0 = min(st.hdr[0], K);
        frames = min(max(st.hdr[2], 0), F);
        steps0 = min(max(st.hdr[1], 0), frames);
        nan_frame = min(max(st.hdr[3], 0), F) - 1;
        if (tid < nb0) {
            State s;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                s.ht[h] = st.ht[h * K + tid]; s.hp[h] = st.hp[h * K + tid]; s.pp[h] = st.pp[h * K + tid]; s.hw[h] = st.hw[h * K + tid];
            }
            s.flags = st.flags[tid];
            store_state(sh.bm, 0, tid, s, st.score[tid], st.last[tid]);
        }
    }
    // the chunk is consumed whole or refused: a slot never reset or past max_frames takes nothing, one that met a NaN nothing more
    const bool refused = asked > 0 && (!live || (nan_frame < 0 && frames + asked > F));
    const int n = (live && !refused && nan_frame < 0) ? asked : 0;
    // the frame loop, as text, at function scope (n == 0: no frame, one barrier): it reads p, sh, b, tid, lane, wave, V, K, n, hist,
    // lbuf, gbuf, nb0, steps0 and declares nb, cur, steps (the search after the chunk) and bad (NaN frame within the chunk, or -1)
#include "ctc_beam_frames.inc.h"
    if (bad >= 0) nan_frame = frames + bad;
    frames += bad >= 0 ? bad : n;
    if (do_reset || n > 0) {
        if (tid == 0) { st.hdr[0] = nb; st.hdr[1] = steps; st.hdr[2] = frames; st.hdr[3] = nan_frame + 1; }
        if (tid < nb) {
            const State s = load_state(sh.bm, cur, tid);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                st.ht[h * K + tid] = s.ht[h]; st.hp[h * K + tid] = s.hp[h]; st.pp[h * K + tid] = s.pp[h]; st.hw[h * K + tid] = s.hw[h];
            }
            st.flags[tid] = s.flags;
            st.score[tid] = sh.bm.score[cur][tid];
            st.last[tid] = sh.bm.last[cur][tid];
        }
    }
    int32_t *const status_out = p.status;
    const int status = refused ? -2 : nan_frame;
    if (do_emit && live && nan_frame < 0) {
        // the finish, as text, in a scope of its own: it reads p, sh, b, tid, K, nb, cur, steps, hist, lbuf, status_out, status and
        // the two names below; the condition is the same for the whole workgroup, as the barriers inside need
        constexpr bool guard_history = true;
        const int tok_stride = F;
#include "ctc_beam_finish.inc.h"
    } else if (tid == 0) {
        if (do_emit) p.num_hyps[b] = 0;
        status_out[b] = status;
    }
}

bool in_limits(int beam_size, int max_frames) {
    return beam_size >= 1 && beam_size <= KMAX && max_frames >= 1 && max_frames <= TMAX;
}

}  // namespace

extern "C" int64_t cm_ctc_beam_stream_state_bytes(int32_t beam_size, int32_t max_frames) {
    return in_limits(beam_size, max_frames) ? state_bytes(beam_size, max_frames) : 0;
}

extern "C" int64_t cm_ctc_beam_stream_workspace_bytes(const cm_ctc_beam_stream_args *args) {
    if (!args || args->batch <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX) return 0;
    return 4 * 8 * (int64_t)sort_entries(args->beam_size, args->V) * args->batch;
}

extern "C" int cm_ctc_beam_stream(const cm_ctc_beam_stream_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_stream: args is NULL");
    cm_ctc_beam_stream_args a = *args;
    const bool pointers = (a.log_probs || a.T == 0) && a.chunk_len && a.tok_class && a.tok_hash && a.tok_pow && a.state && a.tokens &&
                          a.token_len && a.scores && a.num_hyps && a.status;
    if (const int rc = check_beam_args(a, "ctc_beam_stream", &a.max_frames, pointers)) return rc;
    CM_REQUIRE(a.state_stride_bytes >= state_bytes(a.beam_size, a.max_frames) && a.state_stride_bytes % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(a.state) % 16 == 0, CM_EINVAL,
               "ctc_beam_stream: state_stride_bytes %lld must be a multiple of 16 and at least cm_ctc_beam_stream_state_bytes() = %lld, "
               "the state 16-byte aligned", (long long)a.state_stride_bytes, (long long)state_bytes(a.beam_size, a.max_frames));
    const int64_t ws = cm_ctc_beam_stream_workspace_bytes(&a);
    CM_REQUIRE(a.workspace_bytes >= ws && (a.workspace || ws == 0) && reinterpret_cast<uintptr_t>(a.workspace) % 8 == 0, CM_EINVAL,
               "ctc_beam_stream: workspace smaller than cm_ctc_beam_stream_workspace_bytes() or not 8-byte aligned");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    hipLaunchKernelGGL((ctc_beam_stream_kernel<NoLm, cm_ctc_beam_stream_args>), dim3(a.batch), dim3(NT), 0,
                       reinterpret_cast<hipStream_t>(a.stream), a, ws / a.batch, sort_entries(a.beam_size, a.V));
    return cm_launch_status("cm_ctc_beam_stream");
}
