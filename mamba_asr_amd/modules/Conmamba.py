"""ConMamba encoder / Mamba decoder modules — drop-in for the reference's modules/Conmamba.py:
same class names, constructor signatures, forward signatures/returns and state_dict keys
(SURVEY.md §8b), with the Mamba mixers running on the HIP operator API.

    ConvolutionModule      reference :182-454  (non-chunked path :439-449)
    ConmambaEncoderLayer   reference :457-650
    ConmambaEncoder        reference :653-727
    MambaDecoderLayer      reference :730-953
    MambaDecoder           reference :956-1031
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

import os

from .. import ops
from ..sb_compat import LayerNorm, PositionalwiseFeedForward, RowsLayerNorm, RowsLinear, Swish, linear_rows
from .mamba.bimamba import Mamba as BiMamba
from .mamba.bimamba import UniMamba as Mamba

FFN_RESIDUAL_SCALE = 0.5          # reference ConMambaConstants :161
FINAL_NORM_EPS = 1e-6             # reference ConMambaConstants :166


# depthwise stage of the ConvolutionModule on cm_dwconv1d_fwd / _bwd when on the GPU; CM_NATIVE_DWCONV=0 = nn.Conv1d
USE_NATIVE_DWCONV = os.environ.get("CM_NATIVE_DWCONV", "1") == "1"


class ConvolutionModule(nn.Module):
    """LayerNorm -> pointwise conv (D -> 2D) -> GLU -> depthwise conv k -> [chomp if causal] -> LayerNorm ->
    activation -> Linear -> Dropout.  The dynamic-chunk branch of the reference (:314-437) is not reached by
    ConMamba (the encoder layer has no streaming config) and raises here."""

    def __init__(self, input_size, kernel_size=31, bias=True, activation=Swish, dropout=0.0, causal=False,
                 dilation=1):
        super().__init__()
        self.kernel_size, self.causal, self.dilation = kernel_size, causal, dilation
        span = (kernel_size - 1) * 2 ** (dilation - 1)
        self.padding = span if causal else span // 2
        self.layer_norm = RowsLayerNorm(input_size)
        self.bottleneck = nn.Sequential(nn.Conv1d(input_size, 2 * input_size, kernel_size=1, stride=1, bias=bias),
                                        nn.GLU(dim=1))
        self.conv = nn.Conv1d(input_size, input_size, kernel_size=kernel_size, stride=1, padding=self.padding,
                              dilation=dilation, groups=input_size, bias=bias)
        self.after_conv = nn.Sequential(RowsLayerNorm(input_size), activation(),
                                        RowsLinear(input_size, input_size, bias=bias), nn.Dropout(dropout))

    def forward(self, x, mask: Optional[torch.Tensor] = None, dynchunktrain_config=None):
        if dynchunktrain_config is not None:
            raise NotImplementedError("dynamic chunk training is not used on the ConMamba path")
        if x.is_cuda and USE_NATIVE_DWCONV and self.dilation == 1 and self.kernel_size <= 32:
            # channels-last all the way: the pointwise conv (kernel 1) is a GEMM on (batch, time, channel) rows, GLU runs
            # over the last axis and the depthwise conv + its autograd are cm_dwconv_cl_fwd / _bwd -- no transposing
            # copies.  'same' zero padding, or all padding in front for the causal variant (= the reference's
            # pad-then-chomp).
            pw = self.bottleneck[0]
            out = F.glu(linear_rows(self.layer_norm(x), pw.weight.squeeze(-1), pw.bias), dim=-1)
            if out.dtype in (torch.bfloat16, torch.float32):
                out = ops.DepthwiseConvClFn.apply(out, self.conv.weight, self.conv.bias,
                                                  self.kernel_size - 1 if self.causal else self.kernel_size // 2)
            else:
                out = self.conv(out.transpose(1, 2))
                out = (out[..., : -self.padding] if self.causal else out).transpose(1, 2)
            out = self.after_conv(out)
            if mask is not None:
                out.masked_fill_(mask, 0.0)
            return out
        out = self.conv(self.bottleneck(self.layer_norm(x).transpose(1, 2)))
        if self.causal:
            out = out[..., : -self.padding]
        out = self.after_conv(out.transpose(1, 2))
        if mask is not None:
            out.masked_fill_(mask, 0.0)
        return out


class ConmambaEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, kernel_size=31, activation=Swish, bias=True, dropout=0.0, causal=False,
                 mamba_config=None):
        super().__init__()
        assert mamba_config is not None
        bidirectional = mamba_config.pop("bidirectional")           # shared mutable dict, reference :579-591
        try:
            if causal or not bidirectional:
                self.mamba = Mamba(d_model=d_model, **mamba_config)
            else:
                self.mamba = BiMamba(d_model=d_model, bimamba_type="v2", **mamba_config)
        finally:
            mamba_config["bidirectional"] = bidirectional
        self.convolution_module = ConvolutionModule(d_model, kernel_size, bias, activation, dropout, causal=causal)

        def ffn():
            return nn.Sequential(RowsLayerNorm(d_model),
                                 PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout,
                                                           activation=activation),
                                 nn.Dropout(dropout))

        self.ffn_module1 = ffn()
        self.ffn_module2 = ffn()
        self.norm1 = LayerNorm(d_model)
        self.norm2 = LayerNorm(d_model)
        # these four norms feed a projection and nothing else (feed-forward Linear, BiMamba in_proj, pointwise conv): under
        # autocast their kernel stores the projection's operand dtype itself (sb_compat.RowsLayerNorm.low_out)
        for ln in (self.ffn_module1[0], self.ffn_module2[0], self.norm1.norm, self.convolution_module.layer_norm):
            ln.low_out = True
        self.drop = nn.Dropout(dropout)

    def _ffn(self, mod, x):
        """x + 0.5 * ffn_module(x): one autograd node on rows where its kernels apply (modules/ffn_rows.py), else the module tree."""
        from . import ffn_rows
        ln, pff, drop = mod[0], mod[1], mod[2]
        if ffn_rows.supported(x, ln, pff.ffn[0], pff.ffn[1], pff.ffn[3]):
            return ffn_rows.ffn_rows(x, ln, pff.ffn[0], pff.ffn[2], pff.ffn[3], drop, FFN_RESIDUAL_SCALE)
        return x + FFN_RESIDUAL_SCALE * mod(x)

    def forward(self, x, src_mask=None, src_key_padding_mask=None, pos_embs=None, dynchunktrain_config=None):
        # the reference computes a conv mask and then discards it (:631-635): padding is NOT masked
        x = self._ffn(self.ffn_module1, x)
        from .mamba import mixer_rows
        if mixer_rows.block_supported(self.mamba, self.norm1.norm, x):
            x = mixer_rows.mixer_rows(self.mamba, x, ln=self.norm1.norm)                # x + mamba(norm1(x)) as one node on rows
        else:
            x = self.mamba(self.norm1(x)) + x
        from . import convmod_rows
        if dynchunktrain_config is None and convmod_rows.supported(self.convolution_module, x):
            x = convmod_rows.convmod_rows(self.convolution_module, x)         # x + convolution_module(x) as one node on rows
        else:
            x = x + self.convolution_module(x, None, dynchunktrain_config=dynchunktrain_config)
        return self.norm2(self._ffn(self.ffn_module2, x))


class ConmambaEncoderLayerStreamingContext:
    """What one causal ConmambaEncoderLayer carries from one chunk of frames to the next, per stream (batch slot):
    ssm_state (B, E, 16) fp32, the selective scan's state; conv_state (B, 3, E), the mixer conv's last three input rows;
    dw_state (B, 30, D), the last 30 GLU output rows in front of the k = 31 depthwise conv -- the two row histories in the
    compute dtype.  Constant size.  conv_spare / dw_spare are the second buffers the native kernels write the new history
    into (a launch may not overwrite rows its other workgroups still read); ``swap`` makes them current."""

    def __init__(self, ssm_state, conv_state, dw_state):
        self.ssm_state, self.conv_state, self.dw_state = ssm_state, conv_state, dw_state
        self.conv_spare, self.dw_spare = torch.zeros_like(conv_state), torch.zeros_like(dw_state)

    def swap(self):
        self.conv_state, self.conv_spare = self.conv_spare, self.conv_state
        self.dw_state, self.dw_spare = self.dw_spare, self.dw_state

    def reset(self, rows=None):
        for t in (self.ssm_state, self.conv_state, self.dw_state):
            if rows is None:
                t.zero_()
            else:
                t.index_fill_(0, torch.as_tensor(rows, dtype=torch.long, device=t.device), 0)


class ConmambaEncoderStreamingContext:
    """Streaming state of a ConmambaEncoder: one ConmambaEncoderLayerStreamingContext per layer (the reference's
    ConformerEncoderStreamingContext shape: a ``layers`` list)."""

    def __init__(self, layers):
        self.layers = list(layers)

    @property
    def batch_size(self):
        return self.layers[0].ssm_state.shape[0]

    def reset(self, rows=None):
        """Zero the state of every batch slot, or of the slots ``rows`` (indices): the start of a new utterance there."""
        for layer in self.layers:
            layer.reset(rows)


class ConmambaEncoder(nn.Module):
    def __init__(self, num_layers, d_model, d_ffn, kernel_size=31, activation=Swish, bias=True, dropout=0.0,
                 causal=False, mamba_config=None):
        super().__init__()
        self.layers = nn.ModuleList([
            ConmambaEncoderLayer(d_model=d_model, d_ffn=d_ffn, dropout=dropout, activation=activation,
                                 kernel_size=kernel_size, bias=bias, causal=causal, mamba_config=mamba_config)
            for _ in range(num_layers)])
        self.norm = LayerNorm(d_model, eps=FINAL_NORM_EPS)

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos_embs=None, dynchunktrain_config=None):
        if (not torch.is_grad_enabled()) and (not self.training) and src.is_cuda and dynchunktrain_config is None:
            from .. import fused
            if all(fused.supports(layer) for layer in self.layers):
                return fused.encoder_forward(self, src), None            # fused channels-last inference path
        out = src
        for layer in self.layers:
            out = layer(out, src_mask=src_mask, src_key_padding_mask=src_key_padding_mask, pos_embs=pos_embs,
                        dynchunktrain_config=dynchunktrain_config)
        return self.norm(out), None

    def _require_causal(self, what):
        if not all(layer.convolution_module.causal and isinstance(layer.mamba, Mamba) for layer in self.layers):
            raise ValueError(f"{what}: a bidirectional encoder cannot be streamed (build it with causal=True)")

    def make_streaming_context(self, dynchunktrain_config=None, *, batch_size, device=None, dtype=None):
        """A zero ConmambaEncoderStreamingContext for ``batch_size`` streams.  ``dynchunktrain_config`` is accepted and ignored
        (the reference's TransformerASR.make_streaming_context hands it over; a state-space encoder has no chunk size).  ``dtype``:
        the compute dtype of the streamed forward (default: the autocast dtype when enabled, else the parameters')."""
        self._require_causal("make_streaming_context")
        p = self.norm.norm.weight
        device = p.device if device is None else device
        if dtype is None:
            dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else p.dtype
        z = lambda *shape, dt: torch.zeros(shape, dtype=dt, device=device)
        return ConmambaEncoderStreamingContext(
            [ConmambaEncoderLayerStreamingContext(z(batch_size, l.mamba.d_inner, l.mamba.d_state, dt=torch.float32),
                                                  z(batch_size, l.mamba.d_conv - 1, l.mamba.d_inner, dt=dtype),
                                                  z(batch_size, l.convolution_module.kernel_size - 1, l.mamba.d_model, dt=dtype))
             for l in self.layers])

    def forward_streaming(self, src, context, pos_embs=None, lens=None):
        """src (B, t, D), the next t >= 1 frames of B streams -> (out (B, t, D) fp32, None); ``context`` (make_streaming_context)
        is updated in place.  Concatenating the outputs over an utterance's chunks gives ``forward`` on the whole utterance.
        Eval mode, no grad, GPU (fused.forward_streaming).  ``pos_embs`` is ignored, as in ``forward``.  ``lens``: a device int32
        (B,) tensor, slot b advances by its first lens[b] <= t rows only (0: the slot idles and keeps its state); output rows at
        and past lens[b] are unspecified.  None: every slot advances by t rows."""
        self._require_causal("forward_streaming")
        if len(context.layers) != len(self.layers) or context.batch_size != src.shape[0]:
            raise ValueError(f"forward_streaming: the context holds {context.batch_size} streams of {len(context.layers)} layers, "
                             f"src has {src.shape[0]} of {len(self.layers)}")
        if self.training or torch.is_grad_enabled():
            raise RuntimeError("forward_streaming is the inference path: call eval() and run it under torch.no_grad()")
        from .. import fused
        if not all(fused.supports(layer) for layer in self.layers):
            raise NotImplementedError("forward_streaming: a layer is outside the fused path (fused.supports)")
        return fused.forward_streaming(self, src, context, lens), None


class MambaDecoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, activation=nn.ReLU, dropout=0.0, normalize_before=False, mamba_config=None):
        super().__init__()
        assert mamba_config is not None
        bidirectional = mamba_config.pop("bidirectional")
        try:
            self.self_mamba = Mamba(d_model=d_model, **mamba_config)
            self.cross_mamba = Mamba(d_model=d_model, **mamba_config)
        finally:
            mamba_config["bidirectional"] = bidirectional
        self.pos_ffn = PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout,
                                                 activation=activation)
        self.norm1 = LayerNorm(d_model, eps=FINAL_NORM_EPS)
        self.norm2 = LayerNorm(d_model, eps=FINAL_NORM_EPS)
        self.norm3 = LayerNorm(d_model, eps=FINAL_NORM_EPS)
        self.dropout1, self.dropout2, self.dropout3 = nn.Dropout(dropout), nn.Dropout(dropout), nn.Dropout(dropout)
        self.normalize_before = normalize_before

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos_embs_tgt=None, pos_embs_src=None):
        pre = self.normalize_before
        h = self.norm1(tgt) if pre else tgt
        tgt = tgt + self.dropout1(self.self_mamba(h))
        if not pre:
            tgt = self.norm1(tgt)
        h = self.norm2(tgt) if pre else tgt
        # "cross attention": one causal scan over [memory ; tgt], keep the tgt positions (reference :934)
        tgt = tgt + self.dropout2(self.cross_mamba(torch.cat([memory, h], dim=1))[:, -h.shape[1]:])
        if not pre:
            tgt = self.norm2(tgt)
        from . import ffn_rows
        if pre and ffn_rows.supported(tgt, self.norm3.norm, self.pos_ffn.ffn[0], self.pos_ffn.ffn[1], self.pos_ffn.ffn[3]):
            return ffn_rows.ffn_rows(tgt, self.norm3.norm, self.pos_ffn.ffn[0], self.pos_ffn.ffn[2], self.pos_ffn.ffn[3], self.dropout3, 1.0), None, None
        h = self.norm3(tgt) if pre else tgt
        tgt = tgt + self.dropout3(self.pos_ffn(h))
        if not pre:
            tgt = self.norm3(tgt)
        return tgt, None, None

    def step(self, tgt_t, self_state, cross_state):
        """The body of ``forward`` (pre-norm, dropout = identity) for ONE target position: tgt_t (batch, 1, d_model);
        self_state / cross_state are the (conv_state, ssm_state) pairs of the two mixers, updated in place.  The cross
        mixer's states already hold the scan over ``memory`` (MambaDecoder.init_state), so this position continues the
        scan over [memory ; tgt] that ``forward`` restarts from scratch."""
        tgt = tgt_t + self.self_mamba.step(self.norm1(tgt_t), *self_state)[0]
        tgt = tgt + self.cross_mamba.step(self.norm2(tgt), *cross_state)[0]
        from . import ffn_rows
        if ffn_rows.supported(tgt, self.norm3.norm, self.pos_ffn.ffn[0], self.pos_ffn.ffn[1], self.pos_ffn.ffn[3]):
            return ffn_rows.ffn_rows(tgt, self.norm3.norm, self.pos_ffn.ffn[0], self.pos_ffn.ffn[2], self.pos_ffn.ffn[3], self.dropout3, 1.0)
        return tgt + self.pos_ffn(self.norm3(tgt))


class DecoderState:
    """What a stepped MambaDecoder carries from token to token: per layer the (conv_state (batch, d_inner, d_conv),
    ssm_state (batch, d_inner, d_state)) pairs, fp32, of the self mixer and of the cross mixer, and ``position``, the
    number of steps taken.  Constant size: nothing grows with the number of tokens or of memory frames."""

    def __init__(self, self_states, cross_states, position=0):
        self.self_states, self.cross_states, self.position = self_states, cross_states, position

    @property
    def batch(self):
        return self.self_states[0][0].shape[0]

    def tensors(self):
        return [t for pairs in (self.self_states, self.cross_states) for pair in pairs for t in pair]

    def reorder(self, index):
        """A NEW state whose batch row i is this state's row index[i] (index_select on the batch axis of every state
        tensor): what a searcher does when hypotheses are re-ranked or duplicated."""
        dev = self.self_states[0][0].device
        index = torch.as_tensor(index, dtype=torch.long, device=dev)
        pick = lambda pairs: [tuple(t.index_select(0, index) for t in pair) for pair in pairs]
        return DecoderState(pick(self.self_states), pick(self.cross_states), self.position)


class MambaDecoder(nn.Module):
    def __init__(self, num_layers, d_model, d_ffn, activation=nn.ReLU, dropout=0.0, normalize_before=False,
                 mamba_config=None):
        super().__init__()
        self.layers = nn.ModuleList([
            MambaDecoderLayer(d_model=d_model, d_ffn=d_ffn, activation=activation, dropout=dropout,
                              normalize_before=normalize_before, mamba_config=mamba_config)
            for _ in range(num_layers)])
        self.norm = LayerNorm(d_model, eps=FINAL_NORM_EPS)

    def forward(self, tgt, memory, tgt_mask=None, memory_mask=None, tgt_key_padding_mask=None,
                memory_key_padding_mask=None, pos_embs_tgt=None, pos_embs_src=None):
        out = tgt
        for layer in self.layers:
            out, _, _ = layer(out, memory, tgt_mask=tgt_mask, memory_mask=memory_mask,
                              tgt_key_padding_mask=tgt_key_padding_mask,
                              memory_key_padding_mask=memory_key_padding_mask, pos_embs_tgt=pos_embs_tgt,
                              pos_embs_src=pos_embs_src)
        return self.norm(out), [None], [None]

    @torch.no_grad()
    def init_state(self, memory) -> DecoderState:
        """State of a stepped decode over ``memory`` (batch, T, d_model), the encoder output: zero states for every layer's
        self mixer, and for every layer's cross mixer the states after a scan over memory (UniMamba.prefill) -- the
        [memory ; ...] prefix of the concatenation ``forward`` scans.  As in ``forward``, the cross mixer sees the RAW
        memory (norm2 applies to the target half only) and ALL T rows of it, padding frames included: the reference
        scans them too, and there is no length argument here for the same reason ``TransformerASR.decode`` ignores
        enc_len."""
        assert self.layers[0].normalize_before, "the stepped decoder is built for normalize_before=True (the ConMamba recipes)"
        b = memory.shape[0]
        return DecoderState([layer.self_mamba.allocate_inference_cache(b) for layer in self.layers],
                            [layer.cross_mamba.prefill(memory) for layer in self.layers])

    @torch.no_grad()
    def step(self, tgt_t, state: DecoderState):
        """tgt_t (batch, 1, d_model), the embedded target position ``state.position`` -> out_t (batch, 1, d_model): row
        ``state.position`` of what ``forward`` gives for the whole prefix.  ``state`` is updated in place."""
        assert not self.training, "step() is the inference path: call eval() first (dropout is the identity)"
        assert tgt_t.dim() == 3 and tgt_t.shape[1] == 1
        out = tgt_t
        for layer, s_self, s_cross in zip(self.layers, state.self_states, state.cross_states):
            out = layer.step(out, s_self, s_cross)
        state.position += 1
        return self.norm(out)
