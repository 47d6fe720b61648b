"""Ragged batches through the whole-utterance route, the host side: the six `_lens` entry points are declared in
include/conmamba_hip.h, exported, and refuse bad arguments before anything is launched (every native call here is made with HOST
pointers and is refused by a host check); the row / frame arithmetic; the conversion of relative lengths; the refusals of the Python
layers; the route without native kernels -- every utterance alone, scattered -- on a CPU model; CTCBeamSearcher without ``lengths``."""
import ctypes as C
import inspect
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 160
ENTRY = {"cm_conv_xproj_lens": "ConvXprojArgs", "cm_scan_cl_fwd_lens": "ScanClArgs", "cm_glu_dwconv_ln_gelu_lens": "GluDwconvArgs",
         "cm_cnn_front_lens": "CnnFrontArgs", "cm_fbank_wav_lens": "FbankArgs", "cm_fbank_finish_lens": "FbankArgs"}


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


class Host:
    """A zeroed host allocation handed out in 256-byte aligned pieces."""

    def __init__(self, nbytes=1 << 21):
        self.buf = C.create_string_buffer(nbytes + 256)
        self.at = (C.addressof(self.buf) + 255) // 256 * 256
        self.end = C.addressof(self.buf) + nbytes + 256

    def take(self, nbytes):
        p = self.at
        self.at = (p + nbytes + 255) // 256 * 256
        assert self.at <= self.end
        return p


def refused(native, rc, code, text):
    msg = native.lib().cm_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_symbols_declared_and_exported(native):
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12      # additive: the ABI stays
    declared = {s[0]: s for s in native.SYMBOLS}
    handle = C.CDLL(native.LIB_PATH)
    for name, args in ENTRY.items():
        assert name in declared, f"{name} is not declared in conmamba_hip.h"
        assert hasattr(handle, name), f"{name} is not exported"
        _, res, argtypes = declared[name]
        assert res is C.c_int and argtypes == [C.POINTER(getattr(native, args)), C.c_void_p]   # the struct of the form without lengths + the array


def test_every_entry_point_refuses_null_and_misaligned_lengths(native):
    h = Host()
    lens = h.take(64)
    for name, args in ENTRY.items():
        fn, a = getattr(native.lib(), name), getattr(native, args)()
        refused(native, fn(None, lens), native.CM_EINVAL, "args is NULL")
        refused(native, fn(C.byref(a), None), native.CM_EINVAL, "is NULL")
        refused(native, fn(C.byref(a), lens + 2), native.CM_EALIGN, "4-byte aligned")
        assert fn(C.byref(a), lens) == native.CM_EINVAL, name                    # a zeroed struct: bad sizes, nothing launched


def scan_args(native, h, batch=2, seqlen=8, dim=64):
    a = native.ScanClArgs()
    a.batch, a.seqlen, a.dim, a.dstate, a.io_dtype, a.delta_softplus, a.ndir, a.time_chunks = batch, seqlen, dim, 16, native.CM_BF16, 1, 2, 1
    a.z, a.z_bs, a.z_ts = h.take(batch * seqlen * dim * 2), seqlen * dim, dim
    for i, d in enumerate(a.dir):
        d.u, d.out, d.xdbl = h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * 48 * 2)
        d.A, d.dt_weight = h.take(dim * 64), h.take(dim * 64)
        d.u_bs, d.u_ts, d.out_bs, d.out_ts, d.xdbl_bs, d.xdbl_ts, d.dt_rank, d.reverse_time = seqlen * dim, dim, seqlen * dim, dim, seqlen * 48, 48, 16, i
    return a


def test_scan_cl_fwd_lens_refusals(native):
    fn, h = native.lib().cm_scan_cl_fwd_lens, Host()
    lens = h.take(64)
    a = scan_args(native, h)
    a.time_chunks = 2
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "time_chunks 2")
    a.time_chunks, a.lanes_per_channel = 1, 8
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "lanes_per_channel 8")
    a.lanes_per_channel = 0
    state = h.take(2 * 64 * 64)
    for field in ("h0", "h_last", "decay", "ckpt", "ypre"):
        setattr(a.dir[1], field, state)
        refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "no carried state")
        setattr(a.dir[1], field, None)
    xdbl, a.dir[1].xdbl = a.dir[1].xdbl, None                                   # the state-split kernel has no form with lengths
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "xdbl mode")
    a.dir[1].xdbl = xdbl
    a.dir[0].u += 8
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "16-byte aligned")
    a.dir[0].u -= 8
    a.ndir = 3
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "ndir must be 1 or 2")
    a.ndir, a.seqlen = 2, 0
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "bad sizes")


def test_conv_and_dwconv_lens_keep_the_checks_of_the_form_without_lengths(native):
    h = Host()
    lens = h.take(64)
    a = native.ConvXprojArgs()
    batch, seqlen, dim = 2, 8, 64
    a.batch, a.seqlen, a.dim, a.width, a.dt_pad = batch, seqlen, dim, 4, 16
    a.x, a.y_fwd, a.y_bwd, a.xdbl = (h.take(batch * seqlen * dim * 2) for _ in range(4))
    a.weight_f, a.weight_b, a.wx_f, a.wx_b = h.take(dim * 16), h.take(dim * 16), h.take(48 * dim * 2), h.take(48 * dim * 2)
    a.x_bs, a.x_ts, a.yf_bs, a.yf_ts, a.yb_bs, a.yb_ts, a.xdbl_bs, a.xdbl_ts = seqlen * dim, dim, seqlen * dim, dim, seqlen * dim, dim, seqlen * 96, 96
    fn = native.lib().cm_conv_xproj_lens
    a.width = 3
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "conv width 3")
    a.width, a.x = 4, a.x + 2
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "8-byte aligned")
    d = native.GluDwconvArgs()
    d.batch, d.seqlen, d.dim, d.ksize, d.io_dtype, d.glu_done, d.eps = 2, 8, 256, 15, native.CM_BF16, 1, 1e-5
    d.in_, d.out = h.take(2 * 8 * 256 * 2), h.take(2 * 8 * 256 * 2)
    d.weight, d.ln_g, d.ln_b = (h.take(256 * 31 * 4) for _ in range(3))
    refused(native, native.lib().cm_glu_dwconv_ln_gelu_lens(C.byref(d), lens), native.CM_EUNSUPPORTED, "kernel size 15")


def test_row_and_frame_arithmetic():
    """T_b = 1 + n // hop, rows_b = ceil(ceil(T_b / 2) / 2) = frontend_rows_total(n, hop), for every n over two hops; and the rows the
    torch front end really returns for a sample of them."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    model = ConMambaASR(ASRConfig("t", d_model=64, d_ffn=128, num_encoder_layers=1, n_fft=400, seed=1)).eval()
    assert model.compute_features.hop == HOP
    wav = 0.1 * torch.randn(1, 4 * HOP + 2 * HOP + 1, generator=torch.Generator().manual_seed(3))
    for n in range(4 * HOP, 6 * HOP + 1):
        t = 1 + n // HOP
        assert fused.frontend_rows_total(n, HOP) == -(-(-(-t // 2)) // 2) == ((t + 1) // 2 + 1) // 2
        assert fused.ragged_sample_counts([n], n, HOP) == [n]
        if n % 16 == 0 or n % HOP in (0, 1, HOP - 1):
            with torch.no_grad():
                rows = model.CNN(model.compute_features(wav[:, :n]))
            assert rows.shape[1] == fused.frontend_rows_total(n, HOP), (n, rows.shape)


def test_relative_lengths_become_sample_counts():
    from mamba_asr_amd import fused
    S = 16000
    assert fused.ragged_sample_counts(torch.tensor([1.0, 0.5, 0.3333, 640 / S]), S, HOP) == [16000, 8000, 5333, 640]
    assert fused.ragged_sample_counts(torch.tensor([16000, 8000, 641]), S, HOP) == [16000, 8000, 641]        # integer tensor: absolute counts
    assert fused.ragged_sample_counts([16000, 640], S, HOP) == [16000, 640]
    n = [9977, 5283, 12346]
    assert fused.ragged_sample_counts(torch.tensor([x / S for x in n]), S, HOP) == n                         # round(), not floor()
    for bad, text in ((torch.tensor([1.0, 639 / S]), "at least 5"), ([16000, 0], "at least 5"), (torch.tensor([1.01]), "outside"), ([-1], "outside")):
        with pytest.raises(ValueError, match=text):
            fused.ragged_sample_counts(bad, S, HOP)


def test_python_layers_take_the_new_keywords():
    """The new keyword arguments default to today's call."""
    from mamba_asr_amd import fused, ops
    from mamba_asr_amd.asr import ConMambaASR
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    for fn in (ops.conv_xproj, ops.scan_cl_fwd, ops.glu_dwconv_ln_gelu, ops.cnn_front, ops.fbank_from_wav, fused.encoder_forward):
        p = inspect.signature(fn).parameters
        assert "lens" in p and p["lens"].default is None, fn.__qualname__
    assert list(inspect.signature(fused.encoder_forward).parameters) == ["encoder", "src", "dtype", "streams", "lens"]
    assert inspect.signature(fused.asr_encode).parameters["n_samples"].default is None
    assert inspect.signature(ConMambaASR.encode).parameters["ragged"].default is False
    assert inspect.signature(ConMambaASR.transcribe_s2s).parameters["ragged"].default is False
    p = inspect.signature(CTCBeamSearcher.__call__).parameters
    assert list(p) == ["self", "log_probs", "wav_lens", "lengths"] and p["lengths"].default is None


def test_ops_refuse_a_malformed_lens():
    """Non-int32, wrong shape, non-contiguous, another device: refused by the one check every wrapper makes; CPU tensors are refused by
    the wrappers before that."""
    from mamba_asr_amd import fused, ops
    dev = torch.device("cpu")
    good = torch.zeros(4, dtype=torch.int32)
    assert ops.slot_lens(good, 4, dev).ptr == good.data_ptr()
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(4), torch.zeros(3, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.int32),
                torch.zeros(8, dtype=torch.int32)[::2], [0, 1, 2, 3]):
        with pytest.raises(RuntimeError, match="lens must be a contiguous int32"):
            ops.slot_lens(bad, 4, dev)
    with pytest.raises(RuntimeError, match="lens must be a contiguous int32"):
        ops.slot_lens(good, 4, torch.device("cuda", 0))                          # a CPU tensor for a GPU launch
    x = torch.zeros(2, 8, 64, dtype=torch.bfloat16)
    lens = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.conv_xproj(x, torch.zeros(64, 4), None, torch.zeros(64, 4), None, None, None, x.clone(), x.clone(), lens=lens)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.scan_cl_fwd([dict(u=x), dict(u=x)], lens=lens)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.glu_dwconv_ln_gelu(x, torch.zeros(64, 31), None, torch.zeros(64), torch.zeros(64), glu_done=True, lens=lens)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cnn_front(torch.zeros(2, 8, 80), torch.zeros(64, 1, 3, 3), None, torch.zeros(2560), torch.zeros(2560), 1e-5,
                      torch.zeros(32, 3, 3, 64, dtype=torch.bfloat16), None, torch.zeros(640), torch.zeros(640), 1e-5, lens=lens)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.fbank_from_wav(torch.zeros(2, 800), torch.zeros(400), 512, 160, torch.zeros(257, 80), lens=lens)
    with pytest.raises(RuntimeError, match="lens must be a contiguous int32"):
        fused.encoder_forward(None, torch.zeros(2, 8, 64), torch.float32, lens=torch.zeros(2, dtype=torch.int64))


def _cpu_model():
    """A CPU ConMambaASR whose front end is the torch route; the encoder (HIP only) is replaced by a stand-in that mixes time in both
    directions, so padding behind an utterance reaches all of its rows unless every utterance is encoded alone."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    model = ConMambaASR(ASRConfig("t", d_model=64, d_ffn=128, num_encoder_layers=1, n_fft=400, seed=1)).eval()
    model.Transformer.encode = lambda src, wav_lens=None: (src.flatten(2).cumsum(1) + src.flatten(2).flip(1).cumsum(1).flip(1))[..., :64]
    return model


def test_fallback_route_on_a_cpu_model_equals_every_utterance_alone():
    from mamba_asr_amd import fused
    model = _cpu_model()
    n = [4000, 2013, 1200, 640]
    wav = 0.1 * torch.randn(len(n), n[0], generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        model.calibrate(wav, torch.ones(len(n)))
        enc, row_lens = model.encode(wav, torch.tensor([x / n[0] for x in n]), ragged=True)
        assert isinstance(row_lens, fused.RowLens) and list(row_lens) == [fused.frontend_rows_total(x, HOP) for x in n]
        assert row_lens.dev.dtype == torch.int32 and row_lens.dev.tolist() == list(row_lens) and enc.shape == (len(n), row_lens[0], 64)
        padded = model.encode(wav, torch.ones(len(n)))
        for b, x in enumerate(n):
            alone = model.encode(wav[b:b + 1, :x], torch.ones(1))
            assert torch.equal(enc[b, :row_lens[b]], alone[0]), b
            if x < n[0]:
                assert not torch.allclose(padded[b, :row_lens[b]], alone[0], atol=1e-3), "the stand-in encoder must see the padding"
        with pytest.raises(ValueError, match="at least 5"):
            model.encode(wav, torch.tensor([1.0, 0.5, 0.1, 0.5]), ragged=True)
    with pytest.raises(ValueError, match="inference path"):
        model.encode(wav, torch.ones(len(n)), ragged=True)                      # grad enabled


def test_transcribe_s2s_hands_the_searcher_lengths_that_round_to_row_lens():
    """The S2S searchers take relative lengths and round T * rel in fp32: what transcribe_s2s(ragged=True) hands them gives row_lens
    back for every row count, and the rows behind an utterance's own are zeros (the Mamba decoder reads the whole memory)."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    for T in range(1, 200):
        rel = torch.tensor([min(1.0, (r + 0.25) / T) for r in range(1, T + 1)], dtype=torch.float32)
        assert torch.round(T * rel).tolist() == list(range(1, T + 1)), T
    model = ConMambaASR(ASRConfig("s", d_model=64, d_ffn=128, num_encoder_layers=1, num_decoder_layers=1, output_neurons=20, n_fft=400, seed=2)).eval()
    model.Transformer.encode = lambda src, wav_lens=None: src.flatten(2).cumsum(1)[..., :64] + 1.0
    n = [4000, 2013, 700]
    wav = 0.1 * torch.randn(len(n), n[0], generator=torch.Generator().manual_seed(0))
    model.calibrate(wav, torch.ones(len(n)))
    enc, rel = model.transcribe_s2s(wav, torch.tensor(n), searcher=lambda e, r: (e, r), ragged=True)
    rows = [7, 4, 2]
    assert torch.round(enc.shape[1] * rel).tolist() == rows and enc.shape == (3, 7, 64)
    for b, r in enumerate(rows):
        assert not bool(enc[b, r:].any()) and bool((enc[b, :r] != 0).any())
    plain = model.transcribe_s2s(wav, torch.ones(3), searcher=lambda e, r: (e, r))      # ragged=False: the call of before
    assert plain[0].shape == (3, 7, 64) and torch.equal(plain[1], torch.ones(3))


def test_ctc_beam_searcher_frame_counts_are_unchanged_without_lengths():
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    s = CTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a", "b"])
    assert s.frame_counts(25, None, 3) == [25, 25, 25]
    rel = torch.tensor([1.0, 0.62, 0.33, 0.0, 1.7])
    assert s.frame_counts(25, rel, 5) == [25, 16, 8, 0, 25] == [min(max(int(round(r * 25)), 0), 25) for r in rel.tolist()]
    with pytest.raises(RuntimeError, match="GPU only"):
        s(torch.zeros(2, 5, 3), lengths=[5, 4])
