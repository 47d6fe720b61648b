// ctc_beam.hip — LM-free CTC beam search over whole utterances (contract: cm_ctc_beam_search; replaces
// speechbrain.decoders.ctc.CTCBeamSearcher, call sites reference train_CTC.py:309-310 and 411-414, settings
// hparams/CTC/conmamba_large.yaml:168-172, 232-237).  The search itself -- frame loop, finish, backtrack -- is ctc_beam_impl.h and
// the two text fragments it names, which the streamed entry point (ctc_beam_stream.hip) and the LM-fused one (ctc_beam_lm.hip) run
// too; this file holds the one-launch kernel with the LM switch off (NoLm), which starts every utterance from the single initial
// beam, keeps the history in its workspace slab and finishes at once.
#include "ctc_beam_impl.h"

namespace {

template <class Lm, class P>
__global__ __launch_bounds__(NT) void ctc_beam_kernel(const P p, int64_t slab_bytes, int64_t hist_bytes, int n2max) {
    __shared__ Shared sh;
    [[maybe_unused]] constexpr typename Lm::Lds lb{};      // NoLm: no per-beam LM state
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, V = p.V, K = p.beam_size;
    const int n = min(max(p.lengths[b], 0), T);
    char *slab = static_cast<char *>(p.workspace) + (int64_t)b * slab_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(slab);
    const Buf gbuf = global_buf(slab + hist_bytes, n2max);
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    if (tid == 0) store_initial_beam(sh.bm, 0);
    // the frame loop, as text: it reads p, sh, b, tid, lane, wave, V, K, n, hist, lbuf, gbuf, nb0, steps0 (and names Lm and lb)
    // and declares nb, cur, steps, bad
    constexpr int nb0 = 1, steps0 = 0;
#include "ctc_beam_frames.inc.h"
    if (bad >= 0) {
        if (tid == 0) { p.bad_frame[b] = bad; p.num_hyps[b] = 0; }
        return;
    }
    // the finish, as text: it reads p, sh, b, tid, K, nb, cur, steps, hist, lbuf and the four names below
    constexpr bool guard_history = false;       // the history is this launch's own
    int32_t *const status_out = p.bad_frame;
    constexpr int status = -1;
    const int tok_stride = T;
#include "ctc_beam_finish.inc.h"
}

}  // namespace

extern "C" int64_t cm_ctc_beam_workspace_bytes(const cm_ctc_beam_args *args) { return whole_workspace_bytes(args); }

extern "C" int cm_ctc_beam_search(const cm_ctc_beam_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_search: args is NULL");
    cm_ctc_beam_args a = *args;
    const bool pointers = a.log_probs && a.lengths && a.tok_class && a.tok_hash && a.tok_pow && a.tokens && a.token_len && a.scores &&
                          a.num_hyps && a.bad_frame && a.workspace;
    if (const int rc = check_beam_args(a, "ctc_beam_search", nullptr, pointers)) return rc;
    CM_REQUIRE(a.workspace_bytes >= cm_ctc_beam_workspace_bytes(&a), CM_EINVAL,
               "ctc_beam_search: workspace smaller than cm_ctc_beam_workspace_bytes()");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    int64_t slab, hist;
    int n2max;
    slab_layout(a, &slab, &hist, &n2max);
    hipLaunchKernelGGL((ctc_beam_kernel<NoLm, cm_ctc_beam_args>), dim3(a.batch), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a,
                       slab, hist, n2max);
    return cm_launch_status("cm_ctc_beam_search");
}
