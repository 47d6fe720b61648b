"""fp64 reference of the CAUSAL ConMamba encoder (test infrastructure), composed from the oracle's pieces -- ffn_module,
mamba_uni, _ln -- and a front-padded depthwise conv: ConmambaEncoderLayer(causal=True) is the layer of
oracle.encoder_layer with the unidirectional mixer (reference modules/Conmamba.py:580-584) and a convolution module
whose k - 1 padding rows are all in front (:230-238 pads both sides by k - 1, :445-446 chomps the tail).  Restates nothing of
the product; tests/test_streaming_cpu.py holds it to the reference's own output (golden g_causal_large)."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import conmamba_oracle as O   # noqa: E402

CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}


def causal_conv_module(p, x, prefix, kernel_size=31):
    g = lambda k: p[prefix + k].to(x.dtype)
    out = O._ln(x, g("layer_norm.weight"), g("layer_norm.bias"), 1e-5).transpose(1, 2)
    out = F.glu(F.conv1d(out, g("bottleneck.0.weight"), g("bottleneck.0.bias")), dim=1)
    out = F.conv1d(F.pad(out, (kernel_size - 1, 0)), g("conv.weight"), g("conv.bias"), groups=out.shape[1])
    out = F.gelu(O._ln(out.transpose(1, 2), g("after_conv.0.weight"), g("after_conv.0.bias"), 1e-5))
    return F.linear(out, g("after_conv.2.weight"), g("after_conv.2.bias"))


def causal_encoder(p, x, num_layers, kernel_size=31):
    """p: state_dict of ConmambaEncoder(causal=True) (reference key names); x (B, T, D) -> (B, T, D) float64."""
    p = {k: v.detach().double().cpu() for k, v in p.items()}
    x = x.detach().double().cpu()
    for i in range(num_layers):
        pre = f"layers.{i}."
        g = lambda k: p[pre + k]
        x = x + 0.5 * O.ffn_module(p, x, pre + "ffn_module1.")
        x = x + O.mamba_uni(p, O._ln(x, g("norm1.norm.weight"), g("norm1.norm.bias"), 1e-5), prefix=pre + "mamba.")
        x = x + causal_conv_module(p, x, pre + "convolution_module.", kernel_size)
        x = x + 0.5 * O.ffn_module(p, x, pre + "ffn_module2.")
        x = O._ln(x, g("norm2.norm.weight"), g("norm2.norm.bias"), 1e-5)
    return O._ln(x, p["norm.norm.weight"], p["norm.norm.bias"], 1e-6)


def _synth():
    import importlib.util
    spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(os.path.dirname(__file__), "golden", "synth.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    return S


def causal_large(num_layers=2):
    """The golden case's encoder (this package's module, synth weights) and input (4, 96, 256)."""
    import torch.nn as nn
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    S = _synth()
    enc = ConmambaEncoder(num_layers=num_layers, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True, dropout=0.0,
                          causal=True, mamba_config=dict(CFG))
    enc.load_state_dict(S.synth_like(enc, 256), strict=True)
    return enc.eval(), S.synth_input("g_causal.x", (4, 96, 256), 256)


_REF = {}


def causal_large_ref():
    """causal_encoder on the golden case, computed once per session; callers leave it unchanged."""
    if "y" not in _REF:
        enc, x = causal_large()
        _REF["y"] = causal_encoder(enc.state_dict(), x, 2)
    return _REF["y"]
