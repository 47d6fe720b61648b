// ctc_beam_lm.hip — CTC beam search over whole utterances with a backoff n-gram LM fused into the frame loop (contract:
// cm_ctc_beam_lm_search; speechbrain.decoders.ctc.CTCBeamSearcher with kenlm_model_path).  The search is the
// LM-free one: this kernel is ctc_beam.hip's with the NgramLm policy, so it includes the same two text fragments and runs what
// they say under `if constexpr (Lm::on)` -- every beam also holds an LM state (ctc_beam_lm_impl.h), the rank sort runs on
// acoustic + LM(text) + partial_score(partial) (merge_rank's total functor) and the surviving beam fetches its folded acoustic
// score from the position the sort carried along.  This file holds the kernel's setup and the entry point (the LM table checks are
// check_lm_args of ctc_beam_lm_impl.h).
// One workgroup of 256 threads per utterance; LDS: Shared 115,888 B + LmBeams 18,432 B = 134,320 B of the 160 KB a workgroup may hold.
#include "ctc_beam_lm_impl.h"

namespace {

static_assert(sizeof(Shared) + sizeof(LmBeams) <= 160 * 1024, "the LM search's LDS must fit one workgroup");

template <class Lm, class P>
__global__ __launch_bounds__(NT) void ctc_beam_lm_kernel(const P p, int64_t slab_bytes, int64_t hist_bytes, int n2max) {
    __shared__ Shared sh;
    __shared__ typename Lm::Lds lb;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, V = p.V, K = p.beam_size;
    const int n = min(max(p.lengths[b], 0), T);
    char *slab = static_cast<char *>(p.workspace) + (int64_t)b * slab_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(slab);
    const Buf gbuf = global_buf(slab + hist_bytes, n2max);
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    if (tid == 0) { store_initial_beam(sh.bm, 0); lm_store_initial(p, lb, 0); }
    // the frame loop, as text: it reads p, sh, lb, b, tid, lane, wave, V, K, n, hist, lbuf, gbuf, nb0, steps0 and declares nb, cur,
    // steps, bad
    constexpr int nb0 = 1, steps0 = 0;
#include "ctc_beam_frames.inc.h"
    if (bad >= 0) {
        if (tid == 0) { p.bad_frame[b] = bad; p.num_hyps[b] = 0; }
        return;
    }
    // the finish, as text: it reads p, sh, lb, b, tid, K, nb, cur, steps, hist, lbuf and the four names below
    constexpr bool guard_history = false;       // the history is this launch's own
    int32_t *const status_out = p.bad_frame;
    constexpr int status = -1;
    const int tok_stride = T;
#include "ctc_beam_finish.inc.h"
}

}  // namespace

extern "C" int64_t cm_ctc_beam_lm_workspace_bytes(const cm_ctc_beam_lm_args *args) { return whole_workspace_bytes(args); }

extern "C" int cm_ctc_beam_lm_search(const cm_ctc_beam_lm_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_lm_search: args is NULL");
    cm_ctc_beam_lm_args a = *args;
    const bool pointers = a.log_probs && a.lengths && a.tok_class && a.tok_hash && a.tok_pow && a.tok_len && a.tokens && a.token_len &&
                          a.scores && a.lm_scores && a.num_hyps && a.bad_frame && a.workspace;
    if (const int rc = check_beam_args(a, "ctc_beam_lm_search", nullptr, pointers)) return rc;
    if (const int rc = check_lm_args(a, "ctc_beam_lm_search")) return rc;
    CM_REQUIRE(a.workspace_bytes >= cm_ctc_beam_lm_workspace_bytes(&a), CM_EINVAL,
               "ctc_beam_lm_search: workspace smaller than cm_ctc_beam_lm_workspace_bytes()");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    a.alpha_ln10 = a.alpha * std::log(10.0);
    int64_t slab, hist;
    int n2max;
    slab_layout(a, &slab, &hist, &n2max);
    hipLaunchKernelGGL((ctc_beam_lm_kernel<NgramLm, cm_ctc_beam_lm_args>), dim3(a.batch), dim3(NT), 0,
                       reinterpret_cast<hipStream_t>(a.stream), a, slab, hist, n2max);
    return cm_launch_status("cm_ctc_beam_lm_search");
}
