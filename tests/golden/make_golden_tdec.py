#!/usr/bin/env python3
"""Golden vectors of the Transformer decoder, produced by running the REFERENCE's own Python (build container only):

    python tests/golden/make_golden_tdec.py

Same mechanism as make_golden_r3.py (whose loader this imports): the reference's modules are imported from the reference tree
with empty stubs for the CUDA wheels and restated stand-ins for the speechbrain names; nothing of the reference is copied,
the fixture holds tensors only.

  g_tdec_forward  reference TransformerASR (modules/TransformerASR.py: constructor :674-743, forward :745-819 with the masks of
                  :367-425, decode :821-866) with encoder_module 'conmamba' + decoder_module 'transformer' -- the factory's
                  TransformerDecoder (modules/Transformer.py:764-777, :1347-1647; regularMHA, causal) -- at d_model 128, 4 heads,
                  2 ConMamba encoder layers + 2 decoder layers, d_ffn 256, vocabulary 53, normalize_before True, GELU,
                  attention_type 'RelPosMHAXL' for the encoder (what the conmamba_{small,large} S2S recipes set), eval mode.
                  src (3, 41, 20, 32), tgt (3, 11) token ids with padding, wav_len [1.0, 0.8, 0.6].  Stored: encoder_out and
                  decoder_out of forward(); decode(tgt, encoder_out, enc_len = round(wav_len * 41))'s prediction and
                  last-layer cross-attention weights; and, from a train-mode pass with dropout 0 that takes the stored
                  encoder_out as a leaf, decoder_out_train and the gradients of sum(decoder_out * w) w.r.t. encoder_out and
                  three decoder parameters (self-attention in_proj_weight of layer 0, cross-attention out_proj.weight of
                  layer 1, pos_ffn.ffn.0.weight of layer 0).  Parameters come from tests/golden/synth.py (seeded).

speechbrain stand-ins added by this file (speechbrain 1.0.0 is neither in the reference tree nor installable here, so their
semantics are restated and PARITY FOR THEM IS UNPINNED, as DESIGN.md says of the others):
  nnet.attention.MultiheadAttention     torch's nn.MultiheadAttention under ``.att``, batch-first by two permutes, returning
                                        (output, head-averaged attention weights); attn_mask and key_padding_mask handed through
  nnet.attention.PositionalwiseFeedForward, nnet.normalization.LayerNorm    make_golden.py's (Linear-act-Dropout-Linear under
                                        ``.ffn``; nn.LayerNorm under ``.norm``)
"""
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference, save                                      # noqa: E402
from make_golden_r3 import CFG, load_reference_transformer_asr, synth_params     # noqa: E402
from synth import synth_input                                                    # noqa: E402


class MultiheadAttention(nn.Module):              # speechbrain.nnet.attention.MultiheadAttention, restated
    def __init__(self, nhead, d_model, dropout=0.0, bias=True, add_bias_kv=False, add_zero_attn=False, kdim=None, vdim=None):
        super().__init__()
        self.att = nn.MultiheadAttention(embed_dim=d_model, num_heads=nhead, dropout=dropout, bias=bias, add_bias_kv=add_bias_kv,
                                         add_zero_attn=add_zero_attn, kdim=kdim, vdim=vdim)

    def forward(self, query, key, value, attn_mask=None, key_padding_mask=None, return_attn_weights=True, pos_embs=None):
        query, key, value = query.permute(1, 0, 2), key.permute(1, 0, 2), value.permute(1, 0, 2)
        if key_padding_mask is not None and attn_mask is not None and attn_mask.dtype != torch.bool:
            key_padding_mask = torch.zeros_like(key_padding_mask, dtype=attn_mask.dtype).masked_fill(key_padding_mask, float("-inf"))
        out, weights = self.att(query, key, value, attn_mask=attn_mask, key_padding_mask=key_padding_mask,
                                need_weights=return_attn_weights)
        return out.permute(1, 0, 2), weights


def make_tdec_forward(tasr):
    sys.modules["speechbrain.nnet.attention"].MultiheadAttention = MultiheadAttention
    kw = dict(tgt_vocab=53, input_size=640, d_model=128, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=256,
              activation=nn.GELU, encoder_module="conmamba", decoder_module="transformer", attention_type="RelPosMHAXL",
              normalize_before=True, causal=False, mamba_config=dict(CFG))
    model = tasr.TransformerASR(dropout=0.1, **kw)
    missing = model.load_state_dict(synth_params(model, 1290), strict=False)
    assert not missing.unexpected_keys and all(k.endswith(".pe") for k in missing.missing_keys), missing
    model.eval()
    src = synth_input("g_tdec.src", (3, 41, 20, 32), 1290)
    gen = torch.Generator().manual_seed(1291)
    tgt = torch.randint(1, 53, (3, 11), generator=gen)
    tgt[1, 8:] = 0                                             # padding
    tgt[2, 5:] = 0
    wav_len = torch.tensor([1.0, 0.8, 0.6])
    enc_len = torch.round(wav_len * 41).long()
    with torch.no_grad():
        enc, dec = model(src, tgt, wav_len)
        pred, attn = model.decode(tgt, enc, enc_len)
    assert attn.shape == (3, 11, 41)
    # gradients: train mode with dropout 0 (same parameters), the stored encoder_out as the memory
    mt = tasr.TransformerASR(dropout=0.0, **kw)
    mt.load_state_dict(synth_params(mt, 1290), strict=False)
    mt.train()
    import modules.TransformerASR as T
    mem = enc.clone().requires_grad_(True)
    t = mt.custom_tgt_module(tgt)
    t = t + mt.positional_encoding_decoder(t)
    kpm_src, kpm_tgt, _, tgt_mask = T.make_transformer_src_tgt_masks(src.reshape(3, 41, 640), tgt, wav_len, causal=False, pad_idx=0)
    d2, _, _ = mt.decoder(tgt=t, memory=mem, memory_mask=None, tgt_mask=tgt_mask, tgt_key_padding_mask=kpm_tgt,
                          memory_key_padding_mask=kpm_src)
    w = synth_input("g_tdec.w", tuple(d2.shape), 1290)
    names = ["decoder.layers.0.self_attn.att.in_proj_weight", "decoder.layers.1.multihead_attn.att.out_proj.weight",
             "decoder.layers.0.pos_ffn.ffn.0.weight"]
    pd = dict(mt.named_parameters())
    grads = torch.autograd.grad((d2 * w).sum(), [mem] + [pd[n] for n in names])
    cases = dict(tgt=tgt.to(torch.int32), wav_len=wav_len, enc_len=enc_len.to(torch.int32), encoder_out=enc, decoder_out=dec,
                 decode_prediction=pred, decode_attn=attn, decoder_out_train=d2, dmemory=grads[0])
    for n, g in zip(names, grads[1:]):
        cases["g." + n] = g
    # the key set as text, one character code per element (save() stores every tensor as fp32: codes below 2^24 are exact)
    cases["keys"] = torch.tensor([ord(c) for c in "\n".join(model.state_dict().keys())], dtype=torch.int32)
    save("g_tdec_forward", **cases)


if __name__ == "__main__":
    ssi, bim = load_reference()
    tasr, cm = load_reference_transformer_asr(ssi, bim)
    make_tdec_forward(tasr)
