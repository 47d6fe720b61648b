#!/usr/bin/env python3
"""Golden vector of the CAUSAL encoder, produced by running the REFERENCE's own Python (build container only):

    python tests/golden/make_golden_causal.py

Same mechanism as make_golden.py (whose loaders this imports): the reference's modules are imported with empty stubs for
the CUDA wheels; nothing of the reference is copied, the fixture holds tensors.

  g_causal_large  reference ConmambaEncoder(causal=True) (modules/Conmamba.py:653-727: mamba_ssm.Mamba mixers :580-584,
                  front-padded + chomped ConvolutionModule :230-238, :445-446), 2 layers at the CTC-large width (d_model 256,
                  d_ffn 1024), input (4, 96, 256): the encoder's output.  Parameters and input come from tests/golden/synth.py
                  (seeded), only the reference's output is stored.
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference, load_reference_conmamba, save   # noqa: E402
from synth import synth_input, synth_like                               # noqa: E402

CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}


def make_g_causal_large(cm):
    enc = cm.ConmambaEncoder(num_layers=2, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                             dropout=0.1, causal=True, mamba_config=dict(CFG))
    enc.load_state_dict(synth_like(enc, 256), strict=True)
    enc.eval()
    x = synth_input("g_causal.x", (4, 96, 256), 256)
    with torch.no_grad():
        y, _ = enc(x)
        y_prefix, _ = enc(x[:, :37])
    assert (y[:, :37] - y_prefix).abs().max() < 1e-5, "the reference's causal encoder is not prefix-causal"
    save("g_causal_large", y_enc=y)


if __name__ == "__main__":
    ssi, bim = load_reference()
    make_g_causal_large(load_reference_conmamba(ssi, bim))
