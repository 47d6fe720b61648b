"""ASR wrapper around the ConMamba encoder (and a Mamba or Transformer decoder) — the ConMamba/Mamba branches of the
reference's modules/TransformerASR.py (:674-743 constructor, :745-819 forward, :821-866 decode, :868-929 encode,
:1051-1054 Xavier re-init, :1057-1105 EncoderWrapper) and of the factory in modules/Transformer.py
(:740-758 encoder_module == 'conmamba', :764-777 decoder_module == 'transformer', :778-787 decoder_module == 'mamba').

Only these branches are provided: the attention model families' encoders (transformer / conformer / branchformer)
are out of the hot path and raise NotImplementedError.
state_dict keys follow the reference: custom_src_module.layers.0.w.{weight,bias}, encoder.*, decoder.*,
custom_tgt_module.layers.0.emb.Embedding.weight.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from ..sb_compat import Linear, ModuleList, Swish
from .Conmamba import ConmambaEncoder, MambaDecoder
from .Transformer import TransformerDecoder


class PositionalEncoding(nn.Module):
    """Fixed sinusoidal table (reference modules/Transformer.py:796-1022); returns (1, T, D)."""

    def __init__(self, input_size, max_len=2500):
        super().__init__()
        pe = torch.zeros(max_len, input_size)
        pos = torch.arange(0, max_len).unsqueeze(1).float()
        den = torch.exp(torch.arange(0, input_size, 2).float() * -(math.log(10000.0) / input_size))
        pe[:, 0::2] = torch.sin(pos * den)
        pe[:, 1::2] = torch.cos(pos * den)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return self.pe[:, : x.size(1)].clone().detach()


class _Embedding(nn.Module):
    def __init__(self, num_embeddings, embedding_dim, blank_id=0):
        super().__init__()
        self.Embedding = nn.Embedding(num_embeddings, embedding_dim, padding_idx=blank_id)

    def forward(self, x):
        return self.Embedding(x.long())


class NormalizedEmbedding(nn.Module):
    """Embedding scaled by sqrt(d_model) (reference modules/Transformer.py:1650-1860)."""

    def __init__(self, d_model, vocab):
        super().__init__()
        self.emb = _Embedding(num_embeddings=vocab, embedding_dim=d_model, blank_id=0)
        self.d_model = d_model

    def forward(self, x):
        return self.emb(x) * math.sqrt(self.d_model)


def length_to_mask(length, max_len=None):
    max_len = int(length.max()) if max_len is None else max_len
    return torch.arange(max_len, device=length.device)[None, :] < length[:, None]


def lookahead_mask(padded_input):
    """(L, L) bool, True above the diagonal: position i does not see positions > i (reference Transformer.py:1902-1933, there an
    additive 0 / -inf matrix)."""
    L = padded_input.shape[1]
    return torch.ones(L, L, dtype=torch.bool, device=padded_input.device).triu(1)


class TransformerASRStreamingContext:
    """Streaming state of a TransformerASR (reference :151-336): the configuration it was made with and the encoder's context."""

    def __init__(self, dynchunktrain_config, encoder_context):
        self.dynchunktrain_config, self.encoder_context = dynchunktrain_config, encoder_context


class TransformerASR(nn.Module):
    def __init__(self, tgt_vocab, input_size, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6,
                 d_ffn=2048, dropout=0.1, activation=nn.ReLU, positional_encoding="fixed_abs_sine",
                 normalize_before=False, kernel_size: Optional[int] = 31, bias: Optional[bool] = True,
                 encoder_module: Optional[str] = "transformer", decoder_module: Optional[str] = "transformer",
                 conformer_activation=Swish, branchformer_activation=nn.GELU, attention_type: Optional[str] = "regularMHA",
                 max_length: Optional[int] = 2500, causal: Optional[bool] = True, csgu_linear_units=3072,
                 gate_activation=nn.Identity, use_linear_after_conv=False, mamba_config=None):
        super().__init__()
        assert num_encoder_layers + num_decoder_layers > 0
        if attention_type != "RelPosMHAXL":
            # every ConMamba recipe sets RelPosMHAXL (hparams/CTC/conmamba_large.yaml:164), whose branch adds no
            # positional encoding to src (reference :777-778 computes RelPosEncXL and ConMamba discards it); the
            # fixed_abs_sine branch (reference :779-781, 797-800) would add one and is not built: fail loudly
            raise NotImplementedError(f"attention_type={attention_type!r}: only 'RelPosMHAXL' (the ConMamba recipes' setting) "
                                      "is implemented; other types add sinusoidal positions to src in the reference")
        self.causal, self.attention_type, self.positional_encoding_type = causal, attention_type, positional_encoding
        self.num_decoder_layers, self.decoder_module = num_decoder_layers, decoder_module
        if encoder_module != "conmamba":
            raise NotImplementedError(f"encoder_module={encoder_module!r}: only 'conmamba' is on the MI355X hot path")
        assert normalize_before, "normalize_before must be True for Conmamba"          # reference Transformer.py:752
        # the factory hands branchformer_activation (GELU by default) to ConMamba, reference Transformer.py:746
        self.encoder = ConmambaEncoder(num_layers=num_encoder_layers, d_model=d_model, d_ffn=d_ffn, dropout=dropout,
                                       activation=branchformer_activation, kernel_size=kernel_size, bias=bias,
                                       causal=causal, mamba_config=mamba_config)
        if num_decoder_layers > 0:
            if decoder_module == "transformer":
                # the factory builds its decoder with regularMHA and causal=True whatever the encoder uses, reference :765-777
                self.decoder = TransformerDecoder(num_layers=num_decoder_layers, nhead=nhead, d_ffn=d_ffn, d_model=d_model,
                                                  dropout=dropout, activation=activation, normalize_before=normalize_before,
                                                  causal=True, attention_type="regularMHA", max_length=max_length)
            elif decoder_module == "mamba":
                self.decoder = MambaDecoder(num_layers=num_decoder_layers, d_ffn=d_ffn, d_model=d_model,
                                            activation=activation, dropout=dropout, normalize_before=normalize_before,
                                            mamba_config=mamba_config)
            else:
                raise NotImplementedError(f"decoder_module={decoder_module!r}: 'mamba' and 'transformer' are provided")
            self.positional_encoding_decoder = PositionalEncoding(d_model, max_length)
            self.custom_tgt_module = ModuleList(NormalizedEmbedding(d_model, tgt_vocab))
        self.custom_src_module = ModuleList(Linear(input_size=input_size, n_neurons=d_model, bias=True,
                                                   combine_dims=False), nn.Dropout(dropout))
        self._init_params()

    def _init_params(self):
        # reference :1051-1054 — overwrites every >=2-D parameter, including A_log / conv / dt_proj weights
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)

    def _prep_src(self, src):
        if src.dim() == 4:
            b, t, c1, c2 = src.shape
            src = src.reshape(b, t, c1 * c2)
        return self.custom_src_module(src)

    def encode(self, src, wav_len=None, pad_idx=0, dynchunktrain_config=None):
        """(B, T, F[, C]) -> encoder_out (B, T, D).  ConMamba ignores masks and positional embeddings (the
        reference computes RelPosEncXL here and discards it, :915-916; that dead work is skipped)."""
        out, _ = self.encoder(src=self._prep_src(src), src_mask=None, src_key_padding_mask=None, pos_embs=None,
                              dynchunktrain_config=dynchunktrain_config)
        return out

    def encode_streaming(self, src, context: TransformerASRStreamingContext, lens=None):
        """The next chunk of frames (B, t, F[, C]) of the streams in ``context`` -> encoder_out (B, t, D) (reference :931-1022);
        ``context`` is updated in place.  Causal ConMamba encoders only (ConmambaEncoder.forward_streaming).  ``lens``: per-slot
        row counts, a device int32 (B,) tensor (ConmambaEncoder.forward_streaming)."""
        out, _ = self.encoder.forward_streaming(src=self._prep_src(src), pos_embs=None, context=context.encoder_context, lens=lens)
        return out

    def make_streaming_context(self, dynchunktrain_config=None, encoder_kwargs={}):
        """A blank streaming context (reference :1024-1049).  ``encoder_kwargs`` go to the encoder's make_streaming_context:
        batch_size (required), device, dtype."""
        return TransformerASRStreamingContext(dynchunktrain_config=dynchunktrain_config,
                                              encoder_context=self.encoder.make_streaming_context(dynchunktrain_config, **encoder_kwargs))

    def forward(self, src, tgt, wav_len=None, pad_idx=0):
        encoder_out = self.encode(src, wav_len, pad_idx)
        if self.num_decoder_layers == 0:
            return encoder_out, None
        t = self.custom_tgt_module(tgt)
        t = t + self.positional_encoding_decoder(t)                      # attention_type RelPosMHAXL branch, :793-796
        if self.decoder_module == "transformer":
            # reference make_transformer_src_tgt_masks, :367-425, handed over at :805-814 (the Mamba decoder ignores them)
            memory_kpm = None
            if wav_len is not None:
                T = encoder_out.shape[1]
                memory_kpm = ~length_to_mask(torch.round(wav_len.to(encoder_out.device) * T), T)
            decoder_out, _, _ = self.decoder(tgt=t, memory=encoder_out, memory_mask=None, tgt_mask=lookahead_mask(tgt),
                                             tgt_key_padding_mask=tgt.eq(pad_idx), memory_key_padding_mask=memory_kpm)
            return encoder_out, decoder_out
        decoder_out, _, _ = self.decoder(tgt=t, memory=encoder_out)
        return encoder_out, decoder_out

    @torch.no_grad()
    def decode(self, tgt, encoder_out, enc_len=None):
        """-> (prediction (batch, L, d_model), the last layer's cross-attention weights (batch, L, T) or None), reference
        :821-866.  The Transformer decoder masks the future and the memory frames at or beyond ``enc_len``; the Mamba decoder
        takes neither and returns no weights."""
        t = self.custom_tgt_module(tgt)
        t = t + self.positional_encoding_decoder(t)
        if self.decoder_module == "transformer":
            memory_kpm = None
            if enc_len is not None:
                memory_kpm = ~length_to_mask(torch.as_tensor(enc_len).to(encoder_out.device), encoder_out.shape[1])
            prediction, _, attn = self.decoder(t, encoder_out, tgt_mask=lookahead_mask(tgt), memory_key_padding_mask=memory_kpm)
            return prediction, attn[-1]
        prediction, _, attn = self.decoder(t, encoder_out)
        return prediction, attn[-1]

    @torch.no_grad()
    def init_decode_state(self, encoder_out, enc_lens=None):
        """The state ``decode_step`` advances.  Mamba decoder: MambaDecoder.init_state over encoder_out (batch, T, d_model), all
        T rows (``enc_lens`` is not used: the reference's Mamba decoder scans the padding too).  Transformer decoder:
        TransformerDecoder.init_state, which projects encoder_out once per layer and masks the frames at or beyond
        ``enc_lens`` (batch,) (None: none)."""
        if self.decoder_module == "transformer":
            return self.decoder.init_state(encoder_out, enc_lens)
        return self.decoder.init_state(encoder_out)

    @torch.no_grad()
    def decode_step(self, tokens_t, state):
        """tokens_t (batch,) or (batch, 1): the target token at position ``state.position`` -> (batch, 1, d_model), the row
        ``decode`` computes for that position from the whole prefix, at a cost that depends neither on the prefix length
        nor on the number of encoder frames."""
        t = self.custom_tgt_module(tokens_t.reshape(-1, 1))
        pos = state.position
        assert pos < self.positional_encoding_decoder.pe.shape[1], "decode_step: position beyond max_length"
        t = t + self.positional_encoding_decoder.pe[:, pos:pos + 1]
        return self.decoder.step(t, state)


class EncoderWrapper(nn.Module):
    def __init__(self, transformer, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.transformer = transformer

    def forward(self, x, wav_lens=None, pad_idx=0, **kwargs):
        return self.transformer.encode(x, wav_lens, pad_idx, **kwargs)

    def forward_streaming(self, x, context, lens=None):
        return self.transformer.encode_streaming(x, context, lens)

    def make_streaming_context(self, *args, **kwargs):
        return self.transformer.make_streaming_context(*args, **kwargs)
