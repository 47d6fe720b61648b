"""CPU checks of the streamed LM-fused CTC beam search's boundary (cm_ctc_beam_lm_stream, ops.ctc_beam_lm_stream_state,
ctc_decode.StreamingCTCBeamLMSearcher): the state's size, host-side argument validation in its documented order and the searcher's
constructor and host bookkeeping.  Nothing here launches a kernel."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_lm_data as LD  # noqa: E402

TMAX = 0x7fff0000 // 256


def lm_state_bytes(beam_size, max_frames):
    """16-byte header, 80 + 36 bytes per beam, 4 bytes per (frame, beam) of history, rounded up to 16."""
    return (16 + 116 * beam_size + 4 * beam_size * max_frames + 15) // 16 * 16


def test_symbols_exported_and_abi_unchanged():
    import mamba_asr_amd._native as N
    names = {s[0] for s in N.SYMBOLS}
    assert {"cm_ctc_beam_lm_stream", "cm_ctc_beam_lm_stream_state_bytes", "cm_ctc_beam_lm_stream_workspace_bytes"} <= names
    handle = C.CDLL(N.LIB_PATH)
    for name in ("cm_ctc_beam_lm_stream", "cm_ctc_beam_lm_stream_state_bytes", "cm_ctc_beam_lm_stream_workspace_bytes"):
        assert hasattr(handle, name), name
    assert N.ABI_VERSION == 12 == N.lib().cm_abi_version()
    assert N.CtcBeamLmStreamArgs is N.HEADER.structs["cm_ctc_beam_lm_stream_args"]
    fields = {f for f, _ in N.CtcBeamLmStreamArgs._fields_}
    stream = {f for f, _ in N.CtcBeamStreamArgs._fields_}
    lm = {f for f, _ in N.CtcBeamLmArgs._fields_}
    assert stream <= fields and {"tok_len", "lm_scores", "alpha_ln10", "lm_backoff", "n_entries"} <= fields
    assert lm - {"lengths", "bad_frame"} <= fields             # the whole-utterance fields that the stream's chunk_len / status replace


def test_state_bytes_formula_and_limits():
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    f, free = N.lib().cm_ctc_beam_lm_stream_state_bytes, N.lib().cm_ctc_beam_stream_state_bytes
    assert f(100, 1500) == lm_state_bytes(100, 1500) == 611616 and free(100, 1500) == 608016
    for beam, frames in ((100, 1500), (7, 33), (1, 1), (256, TMAX), (3, 5), (64, 16)):
        assert f(beam, frames) == lm_state_bytes(beam, frames) and f(beam, frames) % 16 == 0
        # 36 bytes of LM state per beam on top of the LM-free size before rounding: the difference of the two roundings
        raw = 16 + 80 * beam + 4 * beam * frames
        assert f(beam, frames) == (raw + 36 * beam + 15) // 16 * 16 and free(beam, frames) == (raw + 15) // 16 * 16
    for beam in (4, 8, 100, 256):                               # 36 x beam a multiple of 16: exactly that much more
        assert f(beam, 10) - free(beam, 10) == 36 * beam
    for beam, frames in ((0, 10), (257, 10), (8, 0), (8, TMAX + 1), (-1, -1)):
        assert f(beam, frames) == 0, (beam, frames)
    st = ops.ctc_beam_lm_stream_state(3, 7, 33, "cpu")
    assert st.shape == (3, lm_state_bytes(7, 33)) and st.dtype == torch.uint8 and not bool(st.any())
    with pytest.raises(RuntimeError, match="max_frames"):
        ops.ctc_beam_lm_stream_state(3, 7, 0, "cpu")
    a = N.CtcBeamLmStreamArgs()
    a.batch, a.V, a.beam_size = 2, 31, 100
    assert N.lib().cm_ctc_beam_lm_stream_workspace_bytes(C.byref(a)) == 2 * 4 * 8 * 4096      # the LM-free stream's rule
    a.V = 4
    assert N.lib().cm_ctc_beam_lm_stream_workspace_bytes(C.byref(a)) == 0
    assert N.lib().cm_ctc_beam_lm_stream_workspace_bytes(None) == 0


def _valid_args(N, keep):
    """Arguments that pass every host check (the pointers are host memory: nothing here may reach a launch, and every call below
    breaks one of them)."""
    a = N.CtcBeamLmStreamArgs()
    a.batch, a.T, a.V, a.dtype, a.lp_bs, a.lp_ts = 2, 8, 31, N.CM_F32, 8 * 31, 31
    a.beam_size, a.topk, a.blank, a.max_frames = 100, 1, 0, 16
    a.hash_base[0], a.hash_base[1], a.hash_sep = 1000003, 1000033, 0x110001
    a.beam_prune_logp, a.token_prune_min_logp, a.blank_skip_threshold = -12.0, -1.2, 1.0
    a.order, a.n_words, a.n_entries, a.word_cap, a.prefix_cap, a.ngram_cap = 3, 10, 30, 32, 64, 64
    a.lm_bos, a.lm_eos, a.lm_unk = 1, 2, 0
    a.alpha, a.beta, a.unk_score_offset = 0.5, 1.5, -10.0
    a.state_stride_bytes = lm_state_bytes(100, 16)
    a.workspace_bytes = 2 * 4 * 8 * 4096
    buf = (C.c_char * 64)()
    keep.append(buf)
    p = (C.addressof(buf) + 15) // 16 * 16
    for name, t in a._fields_:
        if t is C.c_void_p and name not in ("stream", "reset", "emit"):
            setattr(a, name, p)
    return a, p


def test_entry_point_validates_on_the_host():
    import mamba_asr_amd._native as N
    lib, keep = N.lib(), []
    assert lib.cm_ctc_beam_lm_stream(None) == -1 and b"NULL" in lib.cm_last_error()
    assert lib.cm_ctc_beam_lm_stream(C.byref(N.CtcBeamLmStreamArgs())) == -1 and b"bad sizes" in lib.cm_last_error()

    def refused(msg, **fields):
        a, p = _valid_args(N, keep)
        for k, v in fields.items():
            setattr(a, k, v(a, p) if callable(v) else v)
        assert lib.cm_ctc_beam_lm_stream(C.byref(a)) == -1, fields
        err = lib.cm_last_error()
        assert msg in err and err.startswith(b"ctc_beam_lm_stream: "), (fields, err)

    refused(b"NULL pointer", tok_len=None)
    refused(b"NULL pointer", lm_scores=None)
    refused(b"NULL pointer", status=None)
    refused(b"exceeds max_frames", T=17)
    refused(b"NULL LM table", ngram_keys=None)
    refused(b"NULL LM table", lm_backoff=None)
    refused(b"NULL LM table", word_ids=None)
    refused(b"order", order=0)
    refused(b"order", order=6)
    refused(b"powers of two", word_cap=33)
    refused(b"powers of two", prefix_cap=0)
    refused(b"n_entries", n_entries=5)
    refused(b"n_entries", n_entries=1 << 31)
    refused(b"word id", lm_bos=10)
    refused(b"word id", lm_unk=-2)
    refused(b"word id", lm_eos=10)
    refused(b"finite", alpha=float("nan"))
    refused(b"finite", beta=float("inf"))
    refused(b"NaN", beam_prune_logp=float("nan"))
    refused(b"state_stride_bytes", state_stride_bytes=lm_state_bytes(100, 16) - 1)
    refused(b"state_stride_bytes", state_stride_bytes=lm_state_bytes(100, 16) - 16)
    assert int(lib.cm_ctc_beam_stream_state_bytes(100, 16)) < lm_state_bytes(100, 16)
    refused(b"state_stride_bytes", state_stride_bytes=int(lib.cm_ctc_beam_stream_state_bytes(100, 16)))    # an LM-free slab
    refused(b"state_stride_bytes", state_stride_bytes=lm_state_bytes(100, 16) + 8)
    refused(b"16-byte aligned", state=lambda a, p: p + 8)
    refused(b"workspace", workspace_bytes=2 * 4 * 8 * 4096 - 1)
    refused(b"workspace", workspace=None)
    # the order of the checks: beam arguments, LM arguments, state, workspace
    refused(b"beam_size", beam_size=0, order=0, state_stride_bytes=0, workspace_bytes=0)
    refused(b"order", order=0, state_stride_bytes=0, workspace_bytes=0)
    refused(b"state_stride_bytes", state_stride_bytes=0, workspace_bytes=0)


def _searcher(tmp_path, **kw):
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamLMSearcher
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=1)
    return StreamingCTCBeamLMSearcher(**{**D.RECIPE, "vocab_list": D.SPM_VOCAB, "kenlm_model_path": path, **kw})


def test_searcher_constructor(tmp_path):
    from mamba_asr_amd import ctc_decode as M
    s = _searcher(tmp_path, alpha=0.4, max_frames=10)
    assert isinstance(s, M.StreamingCTCBeamSearcher) and isinstance(s, M.CTCBeamSearcher)
    assert s.lm.order == 3 and (s.alpha, s.beta, s.unk_score_offset, s.score_boundary, s.max_frames) == (0.4, 1.5, -10.0, True, 10)
    assert _searcher(tmp_path).max_frames == 1500
    with pytest.raises(ValueError, match="kenlm_model_path is required"):
        M.StreamingCTCBeamLMSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB)
    with pytest.raises(ValueError, match="kenlm_model_path is required"):
        M.StreamingCTCBeamLMSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=None)
    with pytest.raises(NotImplementedError, match="word-start piece"):
        _searcher(tmp_path, vocab_list=["<b>", "A", "B"])
    with pytest.raises(ValueError, match="beta must be finite"):
        _searcher(tmp_path, beta=float("nan"))
    with pytest.raises(ValueError, match="line 1"):
        _searcher(tmp_path, kenlm_model_path=LD.write_text(tmp_path / "bad.arpa", "hello\n"))
    with pytest.raises(ValueError, match="max_frames"):
        _searcher(tmp_path, max_frames=0)
    # the LM-free streamed searcher still refuses a path, and now says where the feature lives
    with pytest.raises(NotImplementedError, match="streamed") as e:
        M.StreamingCTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=str(tmp_path / "m.arpa"))
    assert "StreamingCTCBeamLMSearcher" in str(e.value)


def test_searcher_host_bookkeeping(tmp_path):
    s = _searcher(tmp_path, max_frames=10, beam_size=8)
    st = s.make_state(3, "cpu")
    assert st.slab.shape == (3, lm_state_bytes(8, 10)) and st.fed == [None, None, None]
    lp = torch.zeros(3, 4, 31)
    with pytest.raises(ValueError, match="slot 1 was never reset"):
        s.step(lp, st, lengths=[0, 4, 0])
    with pytest.raises(ValueError, match=r"log_probs must be \(3, t, 31\)"):
        s.step(torch.zeros(2, 4, 31), st, reset=[0, 1, 2])
    with pytest.raises(RuntimeError, match="GPU only"):       # only after the bookkeeping passed, and the counters stay
        s.step(lp, st, reset=[0, 1, 2])
    assert st.fed == [None, None, None]
    with pytest.raises(RuntimeError, match="GPU only"):
        st.reset([0])
    with pytest.raises(RuntimeError, match="GPU only"):
        s.hypotheses(st)
    st.fed = [8, 0, 6]
    with pytest.raises(ValueError, match=r"slot 0 would hold 12 frames, more than max_frames=10"):
        s.step(lp, st)
    with pytest.raises(RuntimeError, match="GPU only"):       # 8 + 2, 0 + 4, 6 + 4: all within 10
        s.step(lp, st, lengths=[2, 4, 4])
    assert st.fed == [8, 0, 6]
