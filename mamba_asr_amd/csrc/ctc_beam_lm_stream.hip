// ctc_beam_lm_stream.hip — the LM-fused CTC beam search carried across streaming chunks (contract: cm_ctc_beam_lm_stream, DESIGN.md
// §4q): the NgramLm instantiation of the streamed kernel (ctc_beam_stream_impl.h), so it includes the two text fragments that
// cm_ctc_beam_lm_search runs and emits through the shared finish, which reads the LM state without writing it.  Every live beam's
// LM state (ctc_beam_lm_impl.h: lm, ps, ctx[4], plen) is loaded from and stored to the slab's LM block beside its identity state.
// One workgroup of 256 threads per slot; LDS: Shared + LmBeams, as the whole-utterance LM kernel.
#include "ctc_beam_lm_impl.h"
#include "ctc_beam_stream_impl.h"

static_assert(sizeof(Shared) + sizeof(LmBeams) <= 160 * 1024, "the streamed LM search's LDS must fit one workgroup");

extern "C" int64_t cm_ctc_beam_lm_stream_state_bytes(int32_t beam_size, int32_t max_frames) {
    return stream_in_limits(beam_size, max_frames) ? state_bytes<NgramLm>(beam_size, max_frames) : 0;
}

extern "C" int64_t cm_ctc_beam_lm_stream_workspace_bytes(const cm_ctc_beam_lm_stream_args *args) {
    return stream_workspace_bytes(args);
}

extern "C" int cm_ctc_beam_lm_stream(const cm_ctc_beam_lm_stream_args *args) {
    CM_REQUIRE(args != nullptr, CM_EINVAL, "ctc_beam_lm_stream: args is NULL");
    cm_ctc_beam_lm_stream_args a = *args;
    const bool pointers = (a.log_probs || a.T == 0) && a.chunk_len && a.tok_class && a.tok_hash && a.tok_pow && a.tok_len && a.state &&
                          a.tokens && a.token_len && a.scores && a.lm_scores && a.num_hyps && a.status;
    if (const int rc = check_beam_args(a, "ctc_beam_lm_stream", &a.max_frames, pointers)) return rc;
    if (const int rc = check_lm_args(a, "ctc_beam_lm_stream")) return rc;
    CM_REQUIRE(a.state_stride_bytes >= state_bytes<NgramLm>(a.beam_size, a.max_frames) && a.state_stride_bytes % 16 == 0 &&
                   reinterpret_cast<uintptr_t>(a.state) % 16 == 0, CM_EINVAL,
               "ctc_beam_lm_stream: state_stride_bytes %lld must be a multiple of 16 and at least cm_ctc_beam_lm_stream_state_bytes() = "
               "%lld, the state 16-byte aligned", (long long)a.state_stride_bytes, (long long)state_bytes<NgramLm>(a.beam_size, a.max_frames));
    const int64_t ws = cm_ctc_beam_lm_stream_workspace_bytes(&a);
    CM_REQUIRE(a.workspace_bytes >= ws && (a.workspace || ws == 0) && reinterpret_cast<uintptr_t>(a.workspace) % 8 == 0, CM_EINVAL,
               "ctc_beam_lm_stream: workspace smaller than cm_ctc_beam_lm_stream_workspace_bytes() or not 8-byte aligned");
    a.blank_skip_log = std::log(a.blank_skip_threshold);
    a.alpha_ln10 = a.alpha * std::log(10.0);
    hipLaunchKernelGGL((ctc_beam_stream_kernel<NgramLm, cm_ctc_beam_lm_stream_args>), dim3(a.batch), dim3(NT), 0,
                       reinterpret_cast<hipStream_t>(a.stream), a, ws / a.batch, sort_entries(a.beam_size, a.V));
    return cm_launch_status("cm_ctc_beam_lm_stream");
}
