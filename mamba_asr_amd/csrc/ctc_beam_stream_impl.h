// ctc_beam_stream_impl.h — the CTC beam search carried across streaming chunks, as a template over the LM policy: the slab layout
// and the kernel that cm_ctc_beam_stream (ctc_beam_stream.hip, NoLm) and cm_ctc_beam_lm_stream
// (ctc_beam_lm_stream.hip, NgramLm) instantiate.  One
// workgroup per slot loads the slot's beams from its state slab into LDS, runs the frame loop of ctc_beam_impl.h -- the text
// cm_ctc_beam_search and cm_ctc_beam_lm_search run -- over the chunk's rows, appending to the history inside the slab, stores the beams back and, when asked,
// finishes on the sort buffers and backtracks: an emit changes neither beams nor history.  Loading and storing the state moves the
// live beams only (plain vector loads and stores); nothing is shared between workgroups.
//
// Slab: int32 header {live beams, processed frames, frames consumed, NaN frame + 1} | score K f64 | ht, hp, pp, hw 2 x K u64 each |
// last, flags K i32 each | the LM block, Lm::STREAM_BYTES per beam (NoLm: none; NgramLm: lm K f64 | ps K f64 | ctx 4 x K i32 |
// plen K i32, ctc_beam_lm_impl.h) | history max_frames x K i32.  Live beams == 0 is a slot that was never reset (an all-zero slab).
// An includer that instantiates the kernel with NgramLm includes ctc_beam_lm_impl.h as well.
#pragma once
#include "ctc_beam_impl.h"

namespace {

constexpr int HDR_BYTES = 16;
constexpr int BEAM_BYTES = 8 + 4 * 2 * 8 + 2 * 4;      // score, four hash pairs, last and flags

template <class Lm> int64_t state_bytes(int beam_size, int max_frames) {
    return (HDR_BYTES + (int64_t)(BEAM_BYTES + Lm::STREAM_BYTES) * beam_size + 4 * (int64_t)beam_size * max_frames + 15) / 16 * 16;
}

// the arrays of one slab
struct Slab {
    int32_t *hdr;
    double *score;
    uint64_t *ht, *hp, *pp, *hw;       // [2][K]
    int32_t *last, *flags, *hist;
    char *lm;                          // the LM block (Lm::STREAM_BYTES x K bytes; 8-byte aligned)
};

template <class Lm> __device__ __forceinline__ Slab slab_of(char *base, int K) {
    Slab s;
    s.hdr = reinterpret_cast<int32_t *>(base);
    s.score = reinterpret_cast<double *>(base + HDR_BYTES);
    s.ht = reinterpret_cast<uint64_t *>(s.score + K);
    s.hp = s.ht + 2 * K; s.pp = s.hp + 2 * K; s.hw = s.pp + 2 * K;
    s.last = reinterpret_cast<int32_t *>(s.hw + 2 * K);
    s.flags = s.last + K;
    s.lm = reinterpret_cast<char *>(s.flags + K);
    s.hist = s.flags + K + (Lm::STREAM_BYTES / 4) * K;
    return s;
}

// the includer's `lb` of the two text fragments: the workgroup's LM beams in LDS, or NoLm's empty constant
template <class Lm> __device__ __forceinline__ decltype(auto) stream_lm_lds() {
    if constexpr (Lm::on) {
        __shared__ typename Lm::Lds lds;
        return (lds);
    } else {
        return typename Lm::Lds{};
    }
}

template <class Lm, class P>
__global__ __launch_bounds__(NT) void ctc_beam_stream_kernel(const P p, int64_t ws_bytes, int n2max) {
    __shared__ Shared sh;
    [[maybe_unused]] auto &&lb = stream_lm_lds<Lm>();      // NoLm: no per-beam LM state, in LDS or in the slab
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, K = p.beam_size, F = p.max_frames;
    const int asked = min(max(p.chunk_len[b], 0), p.T);
    const bool do_reset = p.reset && p.reset[b] != 0, do_emit = p.emit && p.emit[b] != 0;
    if (asked == 0 && !do_reset && !do_emit) return;
    const Slab st = slab_of<Lm>(static_cast<char *>(p.state) + (int64_t)b * p.state_stride_bytes, K);
    int32_t *hist = st.hist;
    const Buf gbuf = global_buf(static_cast<char *>(p.workspace) + (int64_t)b * ws_bytes, n2max);
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    // the slot's search so far, its beams into sh.bm[0]; header values are clamped to the slab, whatever the memory holds
    int nb0 = 1, steps0 = 0, frames = 0, nan_frame = -1;
    const bool live = do_reset || st.hdr[0] > 0;
    if (do_reset) {
        if (tid == 0) {
            store_initial_beam(sh.bm, 0);
            if constexpr (Lm::on) lm_store_initial(p, lb, 0);
        }
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
            // the LM state, its table indices clamped to the tables (lm_slab_load): the slab is caller memory
            if constexpr (Lm::on) lm_store(lb, 0, tid, lm_slab_load(p, st.lm, K, tid));
        }
    }
    // the chunk is consumed whole or refused: a slot never reset or past max_frames takes nothing, one that met a NaN nothing more
    const bool refused = asked > 0 && (!live || (nan_frame < 0 && frames + asked > F));
    const int n = (live && !refused && nan_frame < 0) ? asked : 0;
    // the frame loop, as text, at function scope (n == 0: no frame, one barrier): it reads p, sh, lb, b, tid, lane, wave, V, K, n, hist,
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
            if constexpr (Lm::on) lm_slab_store(st.lm, K, tid, lm_load(lb, cur, tid));
        }
    }
    int32_t *const status_out = p.status;
    const int status = refused ? -2 : nan_frame;
    if (do_emit && live && nan_frame < 0) {
        // the finish, as text, in a scope of its own: it reads p, sh, lb, b, tid, K, nb, cur, steps, hist, lbuf, status_out, status and
        // the two names below; the condition is the same for the whole workgroup, as the barriers inside need
        constexpr bool guard_history = true;
        const int tok_stride = F;
#include "ctc_beam_finish.inc.h"
    } else if (tid == 0) {
        if (do_emit) p.num_hyps[b] = 0;
        status_out[b] = status;
    }
}

inline bool stream_in_limits(int beam_size, int max_frames) {
    return beam_size >= 1 && beam_size <= KMAX && max_frames >= 1 && max_frames <= TMAX;
}

// the body of cm_ctc_beam_stream_workspace_bytes and cm_ctc_beam_lm_stream_workspace_bytes: the candidate sorts that outgrow LDS
template <class A> int64_t stream_workspace_bytes(const A *args) {
    if (!args || args->batch <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX) return 0;
    return 4 * 8 * (int64_t)sort_entries(args->beam_size, args->V) * args->batch;
}

}  // namespace
