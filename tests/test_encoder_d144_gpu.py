"""The d_model-144 ConMamba-small encoder on the fused kernels (cm_ffn_fused and cm_ln_pw_glu at width 144, csrc/fused_d144.hip).

  * the launch sequence: six native launches and two library GEMMs (out_proj, the convolution module's closing Linear) per layer,
    no cm_add_layernorm; with CM_FUSED_D144 off the sequence the encoder took at this width before (library feed-forward GEMMs and
    cm_add_layernorm seams);
  * the numbers: against the fp32 oracle (C scan) at the tolerance of every bf16 encoder comparison here, and no further from it than
    the switched-off route; the joined route over three streams gives the single stream's bits.
"""
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
LAYERS, BATCH, FRAMES, D = 3, 17, 75, 144         # test_encoder_routes_gpu.py's shapes: uneven parts, no multiple of 16 or 64
ALL = BATCH * FRAMES

FUSED = ["cm_ffn_fused", "cm_conv_xproj", "cm_scan_cl_fwd", "cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu", "cm_ffn_fused"]
LIBRARY_FFN = ["cm_add_layernorm", "cm_add_layernorm", "cm_conv_xproj", "cm_scan_cl_fwd", "cm_add_layernorm", "cm_glu_dwconv_ln_gelu",
               "cm_add_layernorm", "cm_add_layernorm"]


def at(names, rows):
    return [(n, rows * (2 if n == "cm_scan_cl_fwd" else 1)) for n in names]


def _encoder():
    """A fresh encoder per run: the layer caches read the switches."""
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(11)
    enc = ConmambaEncoder(num_layers=LAYERS, d_model=D, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    return enc, torch.randn(BATCH, FRAMES, D, device=DEV)


class _LibraryGemms(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.count += func.overloadpacket.__name__ in ("mm", "addmm", "_addmm_activation", "bmm")
        return func(*args, **(kwargs or {}))


def _run_logged(monkeypatch, on, streams=1):
    """-> (encoder, input, output, [(kernel, units), ...] in launch order, fused._out_proj calls, library GEMMs)."""
    from mamba_asr_amd import fused, ops
    monkeypatch.setattr(fused, "USE_FUSED_D144", on)
    for sw in ("USE_FUSED_FFN", "USE_LN_PW_GLU", "USE_CONV_XPROJ", "USE_SCAN_ROWS", "USE_FFN_INPROJ"):   # "everything on"
        monkeypatch.setattr(fused, sw, True)
    monkeypatch.setattr(fused, "USE_NATIVE_GEMM", False)
    monkeypatch.setattr(ops, "FFN_LAYOUT", 16)
    monkeypatch.setattr(fused, "STREAM_MODE", "join")
    enc, x = _encoder()
    calls = []
    real = fused._out_proj
    monkeypatch.setattr(fused, "_out_proj", lambda c, ycat: (calls.append(1), real(c, ycat))[1])
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad(), _LibraryGemms() as gemms:
            out = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=streams)
        torch.cuda.synchronize()
        log = [(e[0], e[3]) for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    monkeypatch.setattr(fused, "_out_proj", real)
    return enc, x, out, log, len(calls), gemms.count


@pytest.fixture(scope="module")
def oracle_output():
    """The fp32 oracle (C scan) on the test's encoder and input, once."""
    from oracle import conmamba_oracle as O
    enc, x = _encoder()
    p = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    return O.encoder(p, x.cpu(), LAYERS, scan=O.selective_scan_c)


def test_launch_sequence_with_the_switch_on_and_off(monkeypatch):
    from mamba_asr_amd import fused, ops
    enc, _, _, log, out_projs, gemms = _run_logged(monkeypatch, True)
    assert log == at(FUSED, ALL) * LAYERS, log                       # six native launches per layer, no cm_add_layernorm
    assert (out_projs, gemms) == (LAYERS, 2 * LAYERS)                # out_proj and the convolution module's closing Linear
    c = fused._cache(enc.layers[0], torch.bfloat16)
    assert c.ffn_native and c.all_native and c.out_packed is None and c.lin_packed is None
    assert c.in_packed.shape == (576, 144) and c.in_packed.padded == (576, 160) and c.pw_packed.padded == (288, 160)
    assert c.ffn1["w1p"].padded == (1024, 160) and c.ffn1["w2p"].padded == (160, 1024) and "w1s" not in c.ffn1
    enc, _, _, log, out_projs, gemms = _run_logged(monkeypatch, False)            # CM_FUSED_D144=0
    assert log == at(LIBRARY_FFN, ALL) * LAYERS + at(["cm_add_layernorm"], ALL), log
    assert (out_projs, gemms) == (LAYERS, 8 * LAYERS)
    c = fused._cache(enc.layers[0], torch.bfloat16)
    assert not c.ffn_native and c.in_packed is None and c.pw_packed is None and "w1p" not in c.ffn1


def test_output_against_the_oracle_beside_the_switched_off_route(monkeypatch, oracle_output):
    _, _, on, _, _, _ = _run_logged(monkeypatch, True)
    _, _, off, _, _, _ = _run_logged(monkeypatch, False)
    want = oracle_output
    assert on.dtype == torch.float32 and on.shape == (BATCH, FRAMES, D)
    torch.testing.assert_close(on.cpu(), want, rtol=3e-2, atol=5e-2)
    torch.testing.assert_close(off.cpu(), want, rtol=3e-2, atol=5e-2)
    e_on, e_off = (on.cpu() - want).abs().mean().item(), (off.cpu() - want).abs().mean().item()
    print(f"mean|err| vs the fp32 oracle: fused {e_on:.3e}, library feed-forward route {e_off:.3e}")
    assert e_on <= 1.2 * e_off


def test_three_streams_joined_give_the_single_stream_bits(monkeypatch):
    _, _, one, log1, _, _ = _run_logged(monkeypatch, True, streams=1)
    _, _, three, log3, _, _ = _run_logged(monkeypatch, True, streams=3)
    assert sum(n == "cm_scan_cl_fwd" for n, _ in log3) == LAYERS     # the joined route: one scan per layer on the whole batch
    assert sum(n == "cm_ffn_fused" for n, _ in log3) == 3 * sum(n == "cm_ffn_fused" for n, _ in log1)
    assert torch.equal(three, one)
