"""CPU checks of the streamed CTC beam search's boundary (cm_ctc_beam_stream, ops.ctc_beam_stream_state,
ctc_decode.StreamingCTCBeamSearcher): exported symbols, the state's size, host-side argument validation and the searcher's host
bookkeeping.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TMAX = 0x7fff0000 // 256


def state_bytes(beam_size, max_frames):
    """16-byte header, 80 bytes per beam, 4 bytes per (frame, beam) of history, rounded up to 16."""
    return (16 + 80 * beam_size + 4 * beam_size * max_frames + 15) // 16 * 16


def test_symbols_exported_and_abi_unchanged():
    import mamba_asr_amd._native as N
    names = {s[0] for s in N.SYMBOLS}
    assert {"cm_ctc_beam_stream", "cm_ctc_beam_stream_state_bytes", "cm_ctc_beam_stream_workspace_bytes"} <= names
    handle = C.CDLL(N.LIB_PATH)
    for name in ("cm_ctc_beam_stream", "cm_ctc_beam_stream_state_bytes", "cm_ctc_beam_stream_workspace_bytes", "cm_ctc_beam_search"):
        assert hasattr(handle, name), name
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    assert int(re.search(r"#define CM_ABI_VERSION (\d+)", hdr).group(1)) == 12 == N.ABI_VERSION == N.lib().cm_abi_version()
    assert "cm_ctc_beam_stream_args" in N.HEADER.structs and N.CtcBeamStreamArgs is N.HEADER.structs["cm_ctc_beam_stream_args"]


def test_state_bytes_formula_and_limits():
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    f = N.lib().cm_ctc_beam_stream_state_bytes
    assert f(100, 1500) == state_bytes(100, 1500) == 608016
    assert f(7, 33) == state_bytes(7, 33) == 1504            # 16 + 560 + 924 = 1500, rounded up
    assert f(256, TMAX) == state_bytes(256, TMAX)
    for beam, frames in ((0, 10), (257, 10), (8, 0), (8, TMAX + 1), (-1, -1)):
        assert f(beam, frames) == 0, (beam, frames)
    st = ops.ctc_beam_stream_state(3, 7, 33, "cpu")
    assert st.shape == (3, 1504) and st.dtype == torch.uint8 and not bool(st.any())
    with pytest.raises(RuntimeError, match="max_frames"):
        ops.ctc_beam_stream_state(3, 7, 0, "cpu")
    # the sorts that outgrow LDS: 4 arrays of 8 bytes over the next power of two of beam_size x V, per slot; none up to 1024
    a = N.CtcBeamStreamArgs()
    a.batch, a.V, a.beam_size = 2, 31, 100
    assert N.lib().cm_ctc_beam_stream_workspace_bytes(C.byref(a)) == 2 * 4 * 8 * 4096
    a.V = 4
    assert N.lib().cm_ctc_beam_stream_workspace_bytes(C.byref(a)) == 0
    assert N.lib().cm_ctc_beam_stream_workspace_bytes(None) == 0


def _valid_args(N, keep):
    """Arguments that pass every host check (the pointers are host memory: nothing here may reach a launch, and every call below
    breaks one of them)."""
    a = N.CtcBeamStreamArgs()
    a.batch, a.T, a.V, a.dtype, a.lp_bs, a.lp_ts = 2, 8, 31, N.CM_F32, 8 * 31, 31
    a.beam_size, a.topk, a.blank, a.max_frames = 100, 1, 0, 16
    a.hash_base[0], a.hash_base[1], a.hash_sep = 1000003, 1000033, 0x110001
    a.beam_prune_logp, a.token_prune_min_logp, a.blank_skip_threshold = -12.0, -1.2, 1.0
    a.state_stride_bytes = state_bytes(100, 16)
    a.workspace_bytes = 2 * 4 * 8 * 4096
    buf = (C.c_char * 64)()
    keep.append(buf)
    p = (C.addressof(buf) + 15) // 16 * 16
    for name in ("log_probs", "chunk_len", "tok_class", "tok_hash", "tok_pow", "state", "tokens", "token_len", "scores", "num_hyps",
                 "status", "workspace"):
        setattr(a, name, p)
    return a


def test_entry_point_validates_on_the_host():
    import mamba_asr_amd._native as N
    lib, keep = N.lib(), []
    assert lib.cm_ctc_beam_stream(None) == -1 and b"NULL" in lib.cm_last_error()
    a = N.CtcBeamStreamArgs()
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.T = 17
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"exceeds max_frames" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.state_stride_bytes -= 16
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"state_stride_bytes" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.state_stride_bytes += 8                                   # long enough, but the next slab's 64-bit arrays would be misaligned
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"state_stride_bytes" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.beam_prune_logp = float("nan")
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"NaN" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.status = None
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"NULL pointer" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.workspace_bytes -= 1
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"workspace" in lib.cm_last_error()
    a = _valid_args(N, keep)
    a.max_frames = TMAX + 1
    assert lib.cm_ctc_beam_stream(C.byref(a)) == -1 and b"max_frames" in lib.cm_last_error()


def _searcher(**kw):
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamSearcher
    return StreamingCTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a", "▁b"], **kw)


def test_searcher_host_bookkeeping():
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    s = _searcher(max_frames=10, beam_size=8)
    assert isinstance(s, CTCBeamSearcher) and s.max_frames == 10 and _searcher().max_frames == 1500
    assert s.compose([2, 1, 2]) == "ba b"                      # the classification and compose are the whole-utterance searcher's
    with pytest.raises(ValueError, match="max_frames"):
        _searcher(max_frames=0)
    st = s.make_state(3, "cpu")
    assert st.slab.shape == (3, state_bytes(8, 10)) and st.fed == [None, None, None]
    lp = torch.zeros(3, 4, 3)
    with pytest.raises(ValueError, match="slot 1 was never reset"):
        s.step(lp, st, lengths=[0, 4, 0])
    with pytest.raises(ValueError, match="slot 2 was never reset"):
        s.step(lp, st, reset=[0, 1])
    with pytest.raises(ValueError, match=r"lengths must be 3 frame counts in \[0, 4\]"):
        s.step(lp, st, lengths=[0, 5, 0], reset=[0, 1, 2])
    with pytest.raises(ValueError, match=r"log_probs must be \(3, t, 3\)"):
        s.step(torch.zeros(2, 4, 3), st, reset=[0, 1, 2])
    # a CPU tensor raises only after the bookkeeping passed, and leaves the counters alone
    with pytest.raises(RuntimeError, match="GPU only"):
        s.step(lp, st, reset=[0, 1, 2])
    assert st.fed == [None, None, None]
    with pytest.raises(RuntimeError, match="GPU only"):
        st.reset([0])
    with pytest.raises(RuntimeError, match="GPU only"):
        s.hypotheses(st)
    with pytest.raises(ValueError, match="slot 3 outside"):
        s.hypotheses(st, rows=[3])
    # overflow of max_frames, from the host's own count of frames fed
    st.fed = [8, 0, 6]
    with pytest.raises(ValueError, match=r"slot 0 would hold 12 frames, more than max_frames=10"):
        s.step(lp, st)
    with pytest.raises(ValueError, match=r"slot 0 would hold 11 frames"):
        s.step(lp, st, lengths=[3, 4, 4])
    with pytest.raises(RuntimeError, match="GPU only"):       # 8 + 2, 0 + 4, 6 + 4: all within 10
        s.step(lp, st, lengths=[2, 4, 4])
    with pytest.raises(RuntimeError, match="GPU only"):       # the reset empties slot 0 first
        s.step(lp, st, reset=[0])
    assert st.fed == [8, 0, 6]
