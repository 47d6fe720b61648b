"""The Transformer decoder the ``conmamba_{small,large}`` S2S recipes pair with the ConMamba encoder (reference
hparams/S2S/conmamba_large.yaml: ``decoder_module`` left at 'transformer', 6 layers, d_model 512, 8 heads, d_ffn 2048;
conmamba_small.yaml: 4 layers, d_model 144, 4 heads, d_ffn 1024; both ``normalize_before: True``, GELU), with a stepped route
for the S2S searchers.

Structure of reference modules/Transformer.py:1347-1647 (TransformerDecoderLayer / TransformerDecoder), whose factory always
builds the decoder with ``regularMHA`` (:774): per layer
  pre-norm:   x = x + drop(self_attn(norm1(x)));  x = x + drop(multihead_attn(norm2(x), memory));  x = x + drop(pos_ffn(norm3(x)))
  post-norm:  x = norm1(x + drop(self_attn(x)));  x = norm2(x + drop(multihead_attn(x, memory)));  x = norm3(x + drop(pos_ffn(x)))
then the decoder's final ``norm``; LayerNorm eps 1e-6.  Keys and values of the cross-attention are the raw memory in both
forms.  Parameter names follow speechbrain's nesting (layers.N.self_attn.att.in_proj_weight, layers.N.multihead_attn.att.out_proj.*,
layers.N.pos_ffn.ffn.{0,3}.*, layers.N.normK.norm.*, norm.norm.*).  speechbrain is not in the reference tree: its
MultiheadAttention is restated here as the parameters of torch's nn.MultiheadAttention applied directly.

``forward`` is plain torch with autograd (the training path).  ``init_state`` / ``step`` / ``TransformerDecoderState.reorder``
decode one token per hypothesis row:
  * the cross-attention's K and V are ONE projection of the memory per layer, made at ``init_state`` for the U utterances and
    never tiled or copied per beam; ``ops.xattn_step`` (cm_xattn_step) reads them through ``row_utt`` with a length per
    utterance;
  * the self-attention's K and V caches are modules/TransformerLM.py's LMState: written once at the position of the step and
    never moved, addressed through a (positions, rows) ancestry table by ``ops.attn_step`` (cm_attn_step).
A reorder touches ``row_utt`` and the ancestry table only.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import sb_compat as sb
from .TransformerLM import LMState, _Attention

LAYER_NORM_EPS = 1e-6


class _CrossAttention(_Attention):
    """nn.MultiheadAttention's parameters (in_proj_weight (3 D, D), in_proj_bias, out_proj) applied to any query / key / value
    with masks, attention-probability dropout and head-averaged weights: what nn.MultiheadAttention.forward returns by default."""

    def __init__(self, d_model, nhead, dropout=0.0):
        super().__init__(d_model, nhead)
        self.dropout = float(dropout)

    def forward(self, query, key, value, attn_mask=None, key_padding_mask=None):
        """query (batch, L, D), key / value (batch, S, D); attn_mask (L, S) bool (True: masked) or additive float;
        key_padding_mask (batch, S) bool, True: ignored -> (out (batch, L, D), weights (batch, L, S))."""
        b, L, D = query.shape
        S, H = key.shape[1], self.num_heads
        dh = D // H
        w, bias = self.in_proj_weight, self.in_proj_bias
        if key is query and value is query:
            q, k, v = F.linear(query, w, bias).split(D, dim=-1)
        else:
            q = F.linear(query, w[:D], bias[:D])
            if value is key:
                k, v = F.linear(key, w[D:], bias[D:]).split(D, dim=-1)
            else:
                k, v = F.linear(key, w[D:2 * D], bias[D:2 * D]), F.linear(value, w[2 * D:], bias[2 * D:])
        q, k, v = q.view(b, L, H, dh).transpose(1, 2), k.view(b, S, H, dh).transpose(1, 2), v.view(b, S, H, dh).transpose(1, 2)
        scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh)                      # (batch, H, L, S)
        if attn_mask is not None:
            if attn_mask.dtype == torch.bool:
                scores = scores.masked_fill(attn_mask, float("-inf"))
            else:
                scores = scores + attn_mask.to(scores.dtype)
        if key_padding_mask is not None:
            scores = scores.masked_fill(key_padding_mask.bool().view(b, 1, 1, S), float("-inf"))
        p = torch.softmax(scores, dim=-1)
        if self.dropout > 0.0 and self.training:
            p = F.dropout(p, self.dropout)
        out = torch.matmul(p, v).transpose(1, 2).reshape(b, L, D)
        return self.out_proj(out), p.mean(dim=1)


class MultiheadAttention(nn.Module):
    """speechbrain.nnet.attention.MultiheadAttention (``regularMHA``): the attention under ``.att``, batch first."""

    def __init__(self, nhead, d_model, dropout=0.0, kdim=None, vdim=None):
        super().__init__()
        if (kdim is not None and kdim != d_model) or (vdim is not None and vdim != d_model):
            raise NotImplementedError(f"MultiheadAttention: kdim {kdim} / vdim {vdim} other than d_model {d_model} are not provided")
        self.att = _CrossAttention(d_model, nhead, dropout)

    def forward(self, query, key, value, attn_mask=None, key_padding_mask=None, pos_embs=None):
        return self.att(query, key, value, attn_mask=attn_mask, key_padding_mask=key_padding_mask)


class TransformerDecoderLayer(nn.Module):
    def __init__(self, d_ffn, nhead, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU, normalize_before=False,
                 attention_type="regularMHA", causal=None):
        super().__init__()
        if attention_type != "regularMHA":
            raise NotImplementedError(f"TransformerDecoderLayer: attention_type={attention_type!r}; the reference's factory builds "
                                      "its decoder with 'regularMHA' only")
        self.nhead = nhead
        self.self_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.multihead_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.pos_ffn = sb.PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout, activation=activation)
        self.norm1 = sb.LayerNorm(d_model, eps=LAYER_NORM_EPS)
        self.norm2 = sb.LayerNorm(d_model, eps=LAYER_NORM_EPS)
        self.norm3 = sb.LayerNorm(d_model, eps=LAYER_NORM_EPS)
        self.dropout1, self.dropout2, self.dropout3 = nn.Dropout(dropout), nn.Dropout(dropout), nn.Dropout(dropout)
        self.normalize_before = normalize_before

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None, memory_key_padding_mask=None,
                pos_embs_tgt=None, pos_embs_src=None):
        pre = self.normalize_before
        x = self.norm1(tgt) if pre else tgt
        y, self_attn = self.self_attn(x, x, x, attn_mask=tgt_mask, key_padding_mask=tgt_key_padding_mask)
        tgt = tgt + self.dropout1(y)
        if not pre:
            tgt = self.norm1(tgt)
        x = self.norm2(tgt) if pre else tgt
        y, cross_attn = self.multihead_attn(x, memory, memory, attn_mask=memory_mask, key_padding_mask=memory_key_padding_mask)
        tgt = tgt + self.dropout2(y)
        if not pre:
            tgt = self.norm2(tgt)
        x = self.norm3(tgt) if pre else tgt
        tgt = tgt + self.dropout3(self.pos_ffn(x))
        if not pre:
            tgt = self.norm3(tgt)
        return tgt, self_attn, cross_attn


class TransformerDecoderState:
    """What a stepped TransformerDecoder carries from token to token, for U utterances and R hypothesis rows.
      ck / cv   per layer (U, T, D): the cross-attention's K and V, the two halves of one (U, T, 2 D) projection of the memory;
                per utterance, shared by its beams, never modified
      row_utt   (R) int32: the utterance of each row;  enc_len (U) int32: its valid memory frames
      cache     the self-attention's LMState (per layer (Lcap, R, D) K / V caches and the (Lcap, R) ancestry table), sized by
                the first step: a searcher widens the U rows of ``init_state`` to U x beam rows by a reorder at position 0
      position  tokens consumed so far
    Bytes: 2 * layers * U * T * D for the memory projections + 2 * layers * Lcap * R * D for the caches (Lcap starts at
    min(max_steps, initial_capacity) and doubles, one copy, when full)."""

    def __init__(self, ck: List[torch.Tensor], cv: List[torch.Tensor], row_utt: torch.Tensor, enc_len: torch.Tensor,
                 max_steps: int, initial_capacity: int):
        self.ck, self.cv, self.row_utt, self.enc_len = ck, cv, row_utt, enc_len
        self.max_steps, self.initial_capacity = int(max_steps), int(initial_capacity)
        self.cache: Optional[LMState] = None
        self.grouped: Optional[bool] = None                        # row_utt == arange(U).repeat_interleave(B)?  None: not looked at

    @property
    def position(self) -> int:
        return 0 if self.cache is None else self.cache.t

    @property
    def rows(self) -> int:
        return self.row_utt.shape[0]

    def reorder(self, index) -> "TransformerDecoderState":
        """New row i continues old row index[i]: row_utt follows, and the ancestry columns follow the parents.  No K or V is
        moved.  Before the first step ``index`` may have any length (the widening to beams); afterwards it keeps the row count,
        the caches being sized for it."""
        index = torch.as_tensor(index, device=self.row_utt.device).long()
        if self.cache is not None:
            if index.shape[0] != self.rows:
                raise ValueError(f"TransformerDecoderState.reorder: {index.shape[0]} rows for caches of {self.rows}; the row count "
                                 "can change before the first step only")
            self.cache.reorder(index)
        self.row_utt = self.row_utt.index_select(0, index)
        self.grouped = None
        return self


class TransformerDecoder(nn.Module):
    """``forward`` as the reference's; ``init_state(memory, enc_lens=None)`` / ``step(tgt_t, state)`` the stepped route.

    ``xattn_fn``: the stepped cross-attention, ``ops.xattn_step``'s signature; default ops.xattn_step (cm_xattn_step), or
    ``ops.xattn_step_torch`` with CM_XATTN_STEP=0 in the environment (read here, at construction).  ``attn_fn``: the stepped
    self-attention, ``ops.attn_step``'s signature; default ops.attn_step (cm_attn_step) where the head dimension is one it
    has (32 / 64), else -- or with CM_ATTN_STEP=0 -- ``ops.attn_step_torch``.  ``max_length``: positions a state may reach (the
    length of the positional table of the model around this decoder).  ``initial_capacity``: positions of the first cache
    allocation."""

    def __init__(self, num_layers, nhead, d_ffn, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU,
                 normalize_before=False, causal=False, attention_type="regularMHA", xattn_fn: Optional[Callable] = None,
                 attn_fn: Optional[Callable] = None, max_length: int = 2500, initial_capacity: int = 64):
        super().__init__()
        self.layers = nn.ModuleList([
            TransformerDecoderLayer(d_ffn=d_ffn, nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                    activation=activation, normalize_before=normalize_before, causal=causal,
                                    attention_type=attention_type)
            for _ in range(num_layers)])
        self.norm = sb.LayerNorm(d_model, eps=LAYER_NORM_EPS)
        self.d_model, self.nhead = int(d_model), int(nhead)
        self.max_length, self.initial_capacity = int(max_length), int(initial_capacity)
        from .. import ops
        if xattn_fn is None:
            xattn_fn = ops.xattn_step_torch if os.environ.get("CM_XATTN_STEP", "1") == "0" else ops.xattn_step
        if attn_fn is None:
            native = os.environ.get("CM_ATTN_STEP", "1") != "0" and self.d_model // self.nhead in (32, 64)
            attn_fn = ops.attn_step if native else ops.attn_step_torch
        self.xattn_fn, self.attn_fn = xattn_fn, attn_fn

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos_embs_tgt=None, pos_embs_src=None):
        out = tgt
        self_attns, multihead_attns = [], []
        for layer in self.layers:
            out, self_attn, multihead_attn = layer(out, memory, tgt_mask=tgt_mask, memory_mask=memory_mask,
                                                   tgt_key_padding_mask=tgt_key_padding_mask,
                                                   memory_key_padding_mask=memory_key_padding_mask,
                                                   pos_embs_tgt=pos_embs_tgt, pos_embs_src=pos_embs_src)
            self_attns.append(self_attn)
            multihead_attns.append(multihead_attn)
        return self.norm(out), self_attns, multihead_attns

    # ------------------------------------------------------------------------------------------------------- stepped route
    def _io_dtype(self, device):
        if device.type == "cuda" and torch.is_autocast_enabled("cuda"):
            return torch.get_autocast_dtype("cuda")                  # what the projection GEMMs return under autocast
        return self.norm.norm.weight.dtype

    @torch.no_grad()
    def init_state(self, memory, enc_lens=None) -> TransformerDecoderState:
        """memory (U, T, d_model), the encoder output; enc_lens (U): its valid frames per utterance (None: all T) -> the state
        of one row per utterance at position 0.  Runs each layer's K | V projection of the memory, once."""
        from .. import ops
        U, T, D = memory.shape
        dev = memory.device
        if self.xattn_fn is ops.xattn_step and T >= ops.N.CM_XATTN_STEP_MAX_T:
            raise ValueError(f"TransformerDecoder.init_state: {T} memory frames; cm_xattn_step takes fewer than "
                             f"{ops.N.CM_XATTN_STEP_MAX_T} (CM_XATTN_STEP=0 selects the torch route)")
        max_steps = self.max_length
        if self.attn_fn is ops.attn_step:
            max_steps = min(max_steps, ops.N.CM_ATTN_STEP_MAX_T)
        dtype = self._io_dtype(dev)
        if enc_lens is None:
            enc_len = torch.full((U,), T, dtype=torch.int32, device=dev)
        else:
            enc_len = torch.as_tensor(enc_lens).to(device=dev, dtype=torch.float64).round().clamp(0, T).to(torch.int32).contiguous()
            if tuple(enc_len.shape) != (U,):
                raise ValueError(f"TransformerDecoder.init_state: enc_lens must hold one length per utterance, got {tuple(enc_len.shape)}")
        ck, cv = [], []
        mem = memory if memory.dtype == self.norm.norm.weight.dtype else memory.to(self.norm.norm.weight.dtype)
        for layer in self.layers:
            att = layer.multihead_attn.att
            kv = F.linear(mem, att.in_proj_weight[D:], att.in_proj_bias[D:]).to(dtype)        # (U, T, 2 D): K | V
            ck.append(kv[..., :D])
            cv.append(kv[..., D:])
        return TransformerDecoderState(ck, cv, torch.arange(U, dtype=torch.int32, device=dev), enc_len, max_steps,
                                       self.initial_capacity)

    def _self_cache(self, state: TransformerDecoderState) -> LMState:
        R, dev, dtype = state.rows, state.row_utt.device, state.ck[0].dtype
        cap = max(1, min(state.max_steps, state.initial_capacity))
        n = len(self.layers)
        kc = [torch.empty((cap, R, self.d_model), dtype=dtype, device=dev) for _ in range(n)]
        vc = [torch.empty((cap, R, self.d_model), dtype=dtype, device=dev) for _ in range(n)]
        return LMState(kc, vc, torch.zeros((cap, R), dtype=torch.int32, device=dev), state.max_steps)

    @torch.no_grad()
    def step(self, tgt_t, state: TransformerDecoderState):
        """tgt_t (R, 1, d_model), the embedded target position ``state.position`` of every row -> (R, 1, d_model): row
        ``state.position`` of what ``forward`` gives for the row's whole prefix.  ``state`` is updated in place."""
        assert not self.training, "step() is the inference path: call eval() first (dropout is the identity)"
        assert tgt_t.dim() == 3 and tgt_t.shape[1] == 1
        from .. import ops
        if tgt_t.shape[0] != state.rows:
            raise ValueError(f"TransformerDecoder.step: {tgt_t.shape[0]} tokens for a state of {state.rows} rows")
        if state.cache is None:
            state.cache = self._self_cache(state)                    # sized now: after a searcher's widening reorder
        cache = state.cache
        t = cache.t
        if t >= state.max_steps:
            raise RuntimeError(f"TransformerDecoder.step: position {t} is beyond the {state.max_steps} positions this decoder steps "
                               "(max_length and cm_attn_step's limit)")
        if t >= cache.capacity:
            cache.grow()
        H, D, dtype = self.nhead, self.d_model, state.ck[0].dtype
        kw = {}
        if self.xattn_fn is ops.xattn_step_torch:
            if state.grouped is None:                                # one host read per token, on the torch route only
                U, R = state.enc_len.shape[0], state.rows
                state.grouped = R % U == 0 and torch.equal(
                    state.row_utt, torch.arange(U, dtype=torch.int32, device=state.row_utt.device).repeat_interleave(R // U))
            kw["grouped"] = state.grouped
        x = tgt_t[:, 0]
        for i, layer in enumerate(self.layers):
            pre = layer.normalize_before
            att = layer.self_attn.att
            qkv = F.linear(layer.norm1(x) if pre else x, att.in_proj_weight, att.in_proj_bias).to(dtype)
            o = self.attn_fn(qkv.contiguous(), cache.kc[i], cache.vc[i], cache.anc, t, H)
            x = x + att.out_proj(o)
            if not pre:
                x = layer.norm1(x)
            att = layer.multihead_attn.att
            q = F.linear(layer.norm2(x) if pre else x, att.in_proj_weight[:D], att.in_proj_bias[:D]).to(dtype)
            o = self.xattn_fn(q.contiguous(), state.ck[i], state.cv[i], state.row_utt, state.enc_len, H, **kw)
            x = x + att.out_proj(o)
            if not pre:
                x = layer.norm2(x)
            x = x + layer.pos_ffn(layer.norm3(x) if pre else x)
            if not pre:
                x = layer.norm3(x)
        cache.anc[t].copy_(cache.rows)                               # position t lives in the row's own cache row until a reorder says
        cache.t = t + 1                                              # otherwise (a greedy search never reorders)
        return self.norm(x).unsqueeze(1)
