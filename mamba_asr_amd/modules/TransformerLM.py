"""The language model the S2S recipes fuse into their test-stage beam search (reference hparams/S2S/conmamba_large.yaml,
conmambamamba_large.yaml: ``lm_model: TransformerLM``, 12 layers, d_model 768, 12 heads, d_ffn 3072, GELU,
``normalize_before: False``, ``num_decoder_layers: 0``, 5000 tokens), with a stepped route for beam search.

speechbrain's TransformerLM is not in the reference tree.  What is written here is its structure as the recipes configure it:
an encoder-only post-norm transformer with ``regularMHA``,
  x = emb(tokens) * sqrt(d_model) + pe[:L]
  per layer:  x = norm1(x + self_att(x)),  x = norm2(x + ffn(x))          (LayerNorm eps 1e-6, causal mask)
  x = encoder.norm(x);  logits = Linear(LayerNorm(Linear(x)))             (output_proj)
and parameter names in speechbrain's nesting (custom_src_module.emb.Embedding.weight, encoder.layers.N.self_att.att.in_proj_*,
...).  Key names and the padding rule are NOT pinned against speechbrain: see DESIGN.md §4f.

``forward(tokens)`` is the full causal forward.  It applies no key-padding mask: a token equal to the pad index inside a
prefix is attended like any other (speechbrain's masks every key equal to pad_idx 0; prefixes of a search hold no pad token).

``init_state`` / ``step`` / ``LMState.reorder`` decode one token per hypothesis row.  The per-layer K and V caches are written
once, at the position of the step, and never moved: ``LMState.anc[s, r]`` is the row in which row r's prefix token of
position s was cached, and ``ops.attn_step`` (cm_attn_step) follows it.  A reorder by the parents a beam search chose touches
that (positions, rows) int32 table only.
"""
from __future__ import annotations

import math
import os
from typing import Callable, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import sb_compat as sb


class _Embedding(nn.Module):
    """speechbrain.nnet.embedding.Embedding: nn.Embedding under ``.Embedding``."""

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.Embedding = nn.Embedding(num_embeddings, embedding_dim)

    def forward(self, x):
        return self.Embedding(x.long())


class NormalizedEmbedding(nn.Module):
    """emb(x) * sqrt(d_model) (keys emb.Embedding.weight)."""

    def __init__(self, d_model, vocab):
        super().__init__()
        self.emb = _Embedding(vocab, d_model)
        self.d_model = d_model

    def forward(self, x):
        return self.emb(x) * math.sqrt(self.d_model)


class PositionalEncoding(nn.Module):
    """Fixed sinusoidal positions: pe[pos, 2i] = sin(pos / 10000^(2i / d)), pe[pos, 2i + 1] = cos(same); buffer ``pe``
    (1, max_len, d).  The table is evaluated in fp64 and rounded once to the buffer's dtype, also when the module is cast."""

    def __init__(self, input_size, max_len=2500):
        super().__init__()
        if input_size % 2:
            raise ValueError(f"PositionalEncoding needs an even size, got {input_size}")
        self.input_size, self.max_len = input_size, max_len
        self.register_buffer("pe", self._table(torch.get_default_dtype(), None))

    def _table(self, dtype, device):
        pos = torch.arange(self.max_len, dtype=torch.float64).unsqueeze(1)
        div = torch.exp(torch.arange(0, self.input_size, 2, dtype=torch.float64) * -(math.log(10000.0) / self.input_size))
        pe = torch.zeros(self.max_len, self.input_size, dtype=torch.float64)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        return pe.unsqueeze(0).to(device=device, dtype=dtype)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.pe = self._table(self.pe.dtype, self.pe.device)       # not the old rounding rounded again
        return self

    def forward(self, x):
        return self.pe[:, :x.shape[1]]


class _Attention(nn.Module):
    """The parameters of nn.MultiheadAttention (in_proj_weight (3 D, D), in_proj_bias, out_proj), applied directly."""

    def __init__(self, d_model, nhead):
        super().__init__()
        if d_model % nhead:
            raise ValueError(f"d_model {d_model} is no multiple of nhead {nhead}")
        self.embed_dim, self.num_heads = d_model, nhead
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)

    def forward(self, x):
        """Causal self-attention over (batch, L, D)."""
        b, L, D = x.shape
        H = self.num_heads
        q, k, v = F.linear(x, self.in_proj_weight, self.in_proj_bias).view(b, L, 3, H, D // H).permute(2, 0, 3, 1, 4)
        scores = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(D // H)
        future = torch.ones(L, L, dtype=torch.bool, device=x.device).triu(1)
        p = torch.softmax(scores.masked_fill(future, float("-inf")), dim=-1)
        return self.out_proj(torch.matmul(p, v).transpose(1, 2).reshape(b, L, D))


class MultiheadAttention(nn.Module):
    """speechbrain.nnet.attention.MultiheadAttention (``regularMHA``): the attention under ``.att``."""

    def __init__(self, nhead, d_model):
        super().__init__()
        self.att = _Attention(d_model, nhead)

    def forward(self, x):
        return self.att(x)


class TransformerLMLayer(nn.Module):
    """One post-norm encoder layer: x = norm1(x + self_att(x)); x = norm2(x + pos_ffn(x))."""

    def __init__(self, d_ffn, nhead, d_model, activation=nn.GELU):
        super().__init__()
        self.self_att = MultiheadAttention(nhead, d_model)
        self.pos_ffn = sb.PositionalwiseFeedForward(d_ffn, input_size=d_model, dropout=0.0, activation=activation)
        self.norm1 = sb.LayerNorm(d_model, eps=1e-6)
        self.norm2 = sb.LayerNorm(d_model, eps=1e-6)

    def forward(self, x):
        x = self.norm1(x + self.self_att(x))
        return self.norm2(x + self.pos_ffn(x))


class TransformerLMEncoder(nn.Module):
    def __init__(self, num_layers, nhead, d_ffn, d_model, activation=nn.GELU):
        super().__init__()
        self.layers = nn.ModuleList([TransformerLMLayer(d_ffn, nhead, d_model, activation) for _ in range(num_layers)])
        self.norm = sb.LayerNorm(d_model, eps=1e-6)

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return self.norm(x)


class LMState:
    """The stepped LM's state for R hypothesis rows.
      t      positions cached so far (a host int)
      kc/vc  per layer (Lcap, R, D): row r of position s holds the k / v of the token that row r consumed at step s
      anc    (Lcap, R) int32: anc[s, r] for s < t is the cache row of row r's prefix token of position s
    Bytes of the caches: 2 * layers * Lcap * R * D * itemsize; Lcap starts at min(max_steps, 64) and doubles (one copy) when
    full."""

    def __init__(self, kc: List[torch.Tensor], vc: List[torch.Tensor], anc: torch.Tensor, max_steps: int):
        self.kc, self.vc, self.anc, self.t, self.max_steps = kc, vc, anc, 0, int(max_steps)
        self.rows = torch.arange(anc.shape[1], dtype=torch.int32, device=anc.device)

    @property
    def capacity(self) -> int:
        return self.anc.shape[0]

    def grow(self):
        """Double the capacity: one copy of every cache and of anc."""
        def doubled(x):
            y = torch.empty((2 * x.shape[0],) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            y[:x.shape[0]].copy_(x)
            return y
        self.kc, self.vc = [doubled(x) for x in self.kc], [doubled(x) for x in self.vc]
        anc = torch.zeros((2 * self.capacity, self.anc.shape[1]), dtype=torch.int32, device=self.anc.device)
        anc[:self.capacity].copy_(self.anc)
        self.anc = anc

    def reorder(self, rows) -> "LMState":
        """New row i continues old row rows[i].  The position just written is its own row's; then the ancestry columns follow the
        parents.  K and V are not touched."""
        if self.t == 0:
            return self
        rows = torch.as_tensor(rows, device=self.anc.device).long()
        self.anc[self.t - 1].copy_(self.rows)
        self.anc[:self.t] = self.anc[:self.t].index_select(1, rows)
        return self


class TransformerLM(nn.Module):
    """``TransformerLM(vocab, d_model=768, nhead=12, num_encoder_layers=12, d_ffn=3072)``: the recipes' language model.

      forward(tokens (batch, L)) -> logits (batch, L, vocab)            the full causal forward
      init_state(R, max_steps) -> LMState
      step(tokens (R,), state) -> logits (R, vocab)                     consumes one token per row at position state.t
      state.reorder(rows)

    ``attn_fn``: the stepped attention, ``ops.attn_step``'s signature; default ops.attn_step (cm_attn_step), or
    ``ops.attn_step_torch`` with CM_ATTN_STEP=0 in the environment.  ``initial_capacity`` caps the first cache allocation
    (default 64 positions)."""

    def __init__(self, vocab, d_model=768, nhead=12, num_encoder_layers=12, d_ffn=3072, activation=nn.GELU, max_len=2500,
                 attn_fn: Optional[Callable] = None, initial_capacity: int = 64):
        super().__init__()
        self.vocab, self.d_model, self.nhead = int(vocab), int(d_model), int(nhead)
        self.initial_capacity = int(initial_capacity)
        self.custom_src_module = NormalizedEmbedding(d_model, vocab)
        self.positional_encoding = PositionalEncoding(d_model, max_len)
        self.encoder = TransformerLMEncoder(num_encoder_layers, nhead, d_ffn, d_model, activation)
        self.output_proj = sb.ModuleList(sb.Linear(d_model, input_size=d_model), sb.LayerNorm(d_model, eps=1e-6),
                                         sb.Linear(vocab, input_size=d_model))
        for p in self.parameters():                                 # speechbrain's _reset_params
            if p.dim() > 1:
                nn.init.xavier_normal_(p)
        if attn_fn is None:
            from .. import ops
            attn_fn = ops.attn_step_torch if os.environ.get("CM_ATTN_STEP", "1") == "0" else ops.attn_step
        self.attn_fn = attn_fn

    def forward(self, tokens):
        x = self.custom_src_module(tokens)
        x = x + self.positional_encoding(x)
        return self.output_proj(self.encoder(x))

    # ------------------------------------------------------------------------------------------------------- stepped route
    def _io_dtype(self, device):
        if device.type == "cuda" and torch.is_autocast_enabled("cuda"):
            return torch.get_autocast_dtype("cuda")                  # what the in_proj GEMM returns under autocast
        return self.custom_src_module.emb.Embedding.weight.dtype

    def init_state(self, R: int, max_steps: int) -> LMState:
        """Caches for R rows and up to max_steps tokens; the first allocation holds min(max_steps, initial_capacity) positions."""
        w = self.custom_src_module.emb.Embedding.weight
        max_steps = max(int(max_steps), 1)
        if max_steps > self.positional_encoding.max_len:
            raise ValueError(f"TransformerLM: {max_steps} steps exceed the {self.positional_encoding.max_len} positions of pe")
        cap = max(1, min(max_steps, self.initial_capacity))
        dtype, n = self._io_dtype(w.device), len(self.encoder.layers)
        kc = [torch.empty((cap, R, self.d_model), dtype=dtype, device=w.device) for _ in range(n)]
        vc = [torch.empty((cap, R, self.d_model), dtype=dtype, device=w.device) for _ in range(n)]
        return LMState(kc, vc, torch.zeros((cap, R), dtype=torch.int32, device=w.device), max_steps)

    def _add_norm(self, x, y, norm):
        """norm(x + y) -> (fp32 / parameter-dtype residual stream, the same rounded for the next GEMM or None)."""
        ln = norm.norm
        if x.is_cuda and x.dtype == torch.float32 and y.dtype in (torch.float32, torch.bfloat16) and ln.weight.shape[0] <= 1024 \
                and ln.weight.shape[0] % 4 == 0:
            from .. import ops                                        # cm_add_layernorm: the add, the norm and the operand rounding
            low = y.dtype == torch.bfloat16
            x_out, out = ops.add_layernorm(x, y=y.contiguous(), norm1=(ln.weight, ln.bias, ln.eps), x_out=torch.empty_like(x),
                                           out_dtype=torch.bfloat16, want_out=low)
            return x_out, out
        return norm(x + y), None

    @torch.no_grad()
    def step(self, tokens, state: LMState):
        """tokens (R,) -> logits (R, vocab) of the next token of every row, whose prefix is what ``state`` has cached."""
        t = state.t
        if t >= state.max_steps:
            raise RuntimeError(f"TransformerLM.step: the state was made for {state.max_steps} steps")
        if t >= state.capacity:
            state.grow()
        x = self.custom_src_module(tokens) + self.positional_encoding.pe[0, t]
        low = None                                                   # x rounded to the GEMMs' operand dtype, where a kernel made it
        for i, layer in enumerate(self.encoder.layers):
            att = layer.self_att.att
            qkv = F.linear(x if low is None else low, att.in_proj_weight, att.in_proj_bias)
            o = self.attn_fn(qkv.contiguous(), state.kc[i], state.vc[i], state.anc, t, self.nhead)
            x, low = self._add_norm(x, att.out_proj(o), layer.norm1)
            x, low = self._add_norm(x, layer.pos_ffn(x if low is None else low), layer.norm2)
        state.t = t + 1
        return self.output_proj(self.encoder.norm(x))
