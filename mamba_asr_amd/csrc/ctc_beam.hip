// ctc_beam.hip — LM-free CTC beam search over whole utterances (contract: cm_ctc_beam_search; replaces
// speechbrain.decoders.ctc.CTCBeamSearcher, call sites reference train_CTC.py:309-310 and 411-414, settings
// hparams/CTC/conmamba_large.yaml:168-172, 232-237).  The search itself -- frame loop, finish, backtrack -- is ctc_beam_impl.h and
// the two text fragments it names, which the streamed entry point (ctc_beam_stream.hip) runs too; this file holds the one-launch
// kernel, which starts every utterance from the single initial beam, keeps the history in its workspace slab and finishes at once.
#include "ctc_beam_impl.h"

namespace {

__global__ __launch_bounds__(NT) void ctc_beam_kernel(const cm_ctc_beam_args p, int64_t slab_bytes, int64_t hist_bytes, int n2max) {
    __shared__ Shared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, V = p.V, K = p.beam_size;
    const int n = min(max(p.lengths[b], 0), T);
    char *slab = static_cast<char *>(p.workspace) + (int64_t)b * slab_bytes;
    int32_t *hist = reinterpret_cast<int32_t *>(slab);
    const Buf gbuf{reinterpret_cast<uint64_t *>(slab + hist_bytes), reinterpret_cast<uint64_t *>(slab + hist_bytes) + n2max,
                   reinterpret_cast<uint64_t *>(slab + hist_bytes) + 2 * (int64_t)n2max,
                   reinterpret_cast<double *>(slab + hist_bytes) + 3 * (int64_t)n2max};
    const Buf lbuf{sh.k1, sh.k2, sh.k3, sh.sc};

    if (tid == 0) store_initial_beam(sh.bm, 0);
    // the frame loop, as text: it reads p, sh, b, tid, lane, wave, V, K, n, hist, lbuf, gbuf, nb0, steps0 and declares nb, cur, steps, bad
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

// per-utterance workspace slab: history (T x K int32, rounded to 16 B), then the sort arrays when the candidates can outgrow LDS
void slab_layout(const cm_ctc_beam_args &a, int64_t *slab, int64_t *hist, int *n2max) {
    *hist = ((int64_t)a.T * a.beam_size * 4 + 15) / 16 * 16;
    *n2max = sort_entries(a.beam_size, a.V);
    *slab = *hist + 4 * 8 * (int64_t)*n2max;
}

}  // namespace

extern "C" int64_t cm_ctc_beam_workspace_bytes(const cm_ctc_beam_args *args) {
    if (!args || args->batch <= 0 || args->T <= 0 || args->V <= 1 || args->V > VMAX || args->beam_size <= 0 || args->beam_size > KMAX)
        return 0;
    int64_t slab, hist;
    int n2max;
    slab_layout(*args, &slab, &hist, &n2max);
    return slab * args->batch;
}

extern "C" int cm_ctc_beam_search(const cm_ctc_beam_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_search: args is NULL");
    cm_ctc_beam_args a = *args;
    CM_REQUIRE(a.batch > 0 && a.T > 0 && a.V > 1, CM_EINVAL, "ctc_beam_search: bad sizes batch=%d T=%d V=%d", a.batch, a.T, a.V);
    CM_REQUIRE(a.V <= VMAX, CM_EUNSUPPORTED, "ctc_beam_search: at most %d tokens (got %d)", VMAX, a.V);
    CM_REQUIRE(a.T <= TMAX, CM_EUNSUPPORTED, "ctc_beam_search: T=%d too long", a.T);
    CM_REQUIRE(a.beam_size >= 1 && a.beam_size <= KMAX, CM_EINVAL, "ctc_beam_search: beam_size %d not in [1, %d]", a.beam_size, KMAX);
    CM_REQUIRE(a.topk >= 1, CM_EINVAL, "ctc_beam_search: topk %d < 1", a.topk);
    CM_REQUIRE(a.blank >= 0 && a.blank < a.V, CM_EINVAL, "ctc_beam_search: blank %d out of range", a.blank);
    CM_REQUIRE(a.dtype == CM_F32 || a.dtype == CM_BF16, CM_EUNSUPPORTED, "ctc_beam_search: log_probs must be fp32 or bf16");
    CM_REQUIRE(a.lp_bs >= 0 && a.lp_ts >= a.V, CM_EINVAL, "ctc_beam_search: bad log_probs strides bs=%lld ts=%lld",
               (long long)a.lp_bs, (long long)a.lp_ts);
    CM_REQUIRE(a.log_probs && a.lengths && a.tok_class && a.tok_hash && a.tok_pow && a.tokens && a.token_len && a.scores &&
                   a.num_hyps && a.bad_frame && a.workspace, CM_EINVAL, "ctc_beam_search: NULL pointer");
    CM_REQUIRE(a.hash_base[0] > 1 && a.hash_base[0] < P61 && a.hash_base[1] > 1 && a.hash_base[1] < P61 && a.hash_sep < P61,
               CM_EINVAL, "ctc_beam_search: hash bases / separator must lie in (1, 2^61 - 1)");
    CM_REQUIRE(!std::isnan(a.beam_prune_logp) && !std::isnan(a.token_prune_min_logp) && a.blank_skip_threshold > 0.0,
               CM_EINVAL, "ctc_beam_search: thresholds must not be NaN and blank_skip_threshold must be > 0");
    CM_REQUIRE(a.workspace_bytes >= cm_ctc_beam_workspace_bytes(&a), CM_EINVAL,
               "ctc_beam_search: workspace smaller than cm_ctc_beam_workspace_bytes()");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    int64_t slab, hist;
    int n2max;
    slab_layout(a, &slab, &hist, &n2max);
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(a.batch), dim3(NT), 0, reinterpret_cast<hipStream_t>(a.stream), a, slab, hist, n2max);
    return cm_launch_status("cm_ctc_beam_search");
}
