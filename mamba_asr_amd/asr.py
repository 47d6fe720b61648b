"""Recipe-level assembly of the CTC / S2S ConMamba models, mirroring what the reference's YAML files
instantiate (hparams/CTC/conmamba_large.yaml:146-225, 322-326; hparams/S2S/conmamba_small.yaml:229-259;
hparams/S2S/conmambamamba_large.yaml:251-257) and what train_CTC.py's compute_forward / compute_objectives
do with them (train_CTC.py:281-312, 392-422)."""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import sb_compat as sb
from .modules.TransformerASR import TransformerASR


@dataclass
class ASRConfig:
    name: str
    d_model: int = 256
    d_ffn: int = 1024
    num_encoder_layers: int = 18
    num_decoder_layers: int = 0
    output_neurons: int = 31
    n_fft: int = 512
    win_length: int = 25            # ms
    n_mels: int = 80
    sample_rate: int = 16000
    transformer_dropout: float = 0.1
    d_state: int = 16
    expand: int = 2
    d_conv: int = 4
    bidirectional: bool = True
    seed: int = 3402
    blank_index: int = 0
    bos_index: int = 1              # hparams/S2S/conmambamamba_large.yaml:266-267
    eos_index: int = 2
    min_decode_ratio: float = 0.0   # :270-271
    max_decode_ratio: float = 1.0
    decoder_module: str = "mamba"   # "transformer": hparams/S2S/conmamba_{small,large}.yaml leave the default decoder
    nhead: int = 4                  # heads of the Transformer decoder (the ConMamba encoder and the Mamba decoder have none)
    causal: bool = False            # True: UniMamba mixers + front-padded conv modules -- the encoder that can be streamed (encode_streaming)


CONFIGS = {
    # hparams/CTC/conmamba_large.yaml:58, 102-105, 153-183
    "conmamba_large_ctc": ASRConfig("conmamba_large_ctc"),
    # derived as SURVEY.md §8d row 1: CTC recipe + encoder dims of hparams/S2S/conmamba_small.yaml:129,188-189,229-233
    "conmamba_small_ctc": ASRConfig("conmamba_small_ctc", d_model=144, d_ffn=1024, num_encoder_layers=12, n_fft=400,
                                    seed=7775),
    # hparams/S2S/conmambamamba_large.yaml:251-257 (encoder + Mamba decoder, 5000-piece vocabulary)
    "conmambamamba_large_s2s": ASRConfig("conmambamamba_large_s2s", d_model=512, d_ffn=2048, num_encoder_layers=12,
                                         num_decoder_layers=6, output_neurons=5000, win_length=32),
    # hparams/S2S/conmamba_large.yaml:121, 178-180, 220-229 (encoder + the default Transformer decoder, 8 heads)
    "conmamba_large_s2s": ASRConfig("conmamba_large_s2s", d_model=512, d_ffn=2048, num_encoder_layers=12, num_decoder_layers=6,
                                    output_neurons=5000, n_fft=512, win_length=32, seed=3407, decoder_module="transformer",
                                    nhead=8),
    # hparams/S2S/conmamba_small.yaml:129, 188, 229-236 (win_length left at Fbank's 25 ms)
    "conmamba_small_s2s": ASRConfig("conmamba_small_s2s", d_model=144, d_ffn=1024, num_encoder_layers=12, num_decoder_layers=4,
                                    output_neurons=5000, n_fft=400, win_length=25, seed=7775, decoder_module="transformer",
                                    nhead=4),
}


class ConMambaASR(nn.Module):
    """modules dict of the recipe (CNN, Transformer, ctc_lin[, seq_lin], normalize) + feature extractor."""

    def __init__(self, cfg: ASRConfig):
        super().__init__()
        self.cfg = cfg
        torch.manual_seed(cfg.seed)                                        # `__set_seed` in the YAML
        self.compute_features = sb.Fbank(sample_rate=cfg.sample_rate, n_fft=cfg.n_fft, n_mels=cfg.n_mels,
                                         win_length=cfg.win_length)
        self.normalize = sb.InputNormalization(norm_type="global", update_until_epoch=4)
        self.CNN = sb.ConvolutionFrontEnd(input_shape=(8, 10, cfg.n_mels), num_blocks=2, num_layers_per_block=1,
                                          out_channels=(64, 32), kernel_sizes=(3, 3), strides=(2, 2),
                                          residuals=(False, False))
        mamba_config = {"d_state": cfg.d_state, "expand": cfg.expand, "d_conv": cfg.d_conv,
                        "bidirectional": cfg.bidirectional}
        self.Transformer = TransformerASR(
            input_size=(cfg.n_mels // 4) * 32, tgt_vocab=cfg.output_neurons, d_model=cfg.d_model, nhead=cfg.nhead,
            num_encoder_layers=cfg.num_encoder_layers, num_decoder_layers=cfg.num_decoder_layers, d_ffn=cfg.d_ffn,
            dropout=cfg.transformer_dropout, activation=nn.GELU, encoder_module="conmamba",
            decoder_module=cfg.decoder_module, attention_type="RelPosMHAXL", normalize_before=True, causal=cfg.causal,
            mamba_config=mamba_config)
        self.ctc_lin = sb.Linear(input_size=cfg.d_model, n_neurons=cfg.output_neurons)
        if cfg.num_decoder_layers > 0:
            self.seq_lin = sb.Linear(input_size=cfg.d_model, n_neurons=cfg.output_neurons)
        from . import ops
        self.register_load_state_dict_post_hook(lambda module, incompatible: ops.invalidate_caches(module))

    # -- train_CTC.py:285-298 -------------------------------------------------------------
    def features(self, wavs, wav_lens, epoch=0, augment=None):
        feats = self.compute_features(wavs)                                # (B, T, 80), fp32
        feats = self.normalize(feats, wav_lens, epoch=epoch)
        if augment is not None and self.training:
            feats, _ = augment(feats, wav_lens)
        return feats

    @torch.no_grad()
    def calibrate(self, wavs, wav_lens):
        """Fill the global normalisation statistics from one batch outside training (the reference gets them from its
        first training batches, train_CTC.py:287; benchmarks / parity runs on random-init models call this once)."""
        self.normalize.update_statistics(self.compute_features(wavs), wav_lens)

    def encode(self, wavs, wav_lens, epoch=0, augment=None, feats=None, ragged=False):
        """wav (B, samples) -> encoder output (B, ceil(T/4), d_model): the path the headline metric times.
        ``feats``: features() of the batch computed by the caller (a graphed training step keeps Fbank, the running
        normalisation statistics and the host-drawn augmentation outside its hipGraph, brain.Brain.graph_prologue).
        ``ragged=True`` (inference): every utterance is encoded as if alone -> (enc, row_lens).  ``wav_lens`` gives the
        utterances' lengths, relative (floating: round(rel * samples) samples) or absolute (integer sample counts); utterance b's rows
        [0, row_lens[b]) are those of encode on wavs[b:b+1, :n[b]] alone, rows past them are unspecified; row_lens is a fused.RowLens
        (a host list whose .dev is the device tensor).  An utterance under the front end's 5 frames raises ValueError.  The default
        keeps the reference's semantics: wav_lens is ignored and padding reaches every utterance of the batch."""
        if ragged:
            return self._encode_ragged(wavs, wav_lens, epoch)
        if feats is not None:
            return self.Transformer.encode(self.CNN(feats), wav_lens)
        if (not torch.is_grad_enabled()) and (not self.training) and wavs.is_cuda and augment is None \
                and self.normalize.count > 0:
            from . import fused
            if all(fused.supports(layer) for layer in self.Transformer.encoder.layers):
                return fused.asr_encode(self, wavs, wav_lens)                    # native inference path
        src = self.CNN(self.features(wavs, wav_lens, epoch, augment))
        return self.Transformer.encode(src, wav_lens)

    def _encode_ragged(self, wavs, wav_lens, epoch=0):
        from . import fused
        if torch.is_grad_enabled() or self.training:
            raise ValueError("encode(ragged=True) is the inference path: call eval() and run under torch.no_grad()")
        n = fused.ragged_sample_counts(wav_lens, wavs.shape[1], self.compute_features.hop)
        if wavs.is_cuda and self.normalize.count > 0 and all(fused.supports(layer) for layer in self.Transformer.encoder.layers):
            return fused.asr_encode(self, wavs, wav_lens, n_samples=n)
        # no native path (CPU, statistics not calibrated, another layer): each utterance alone through encode, scattered
        rows = [fused.frontend_rows_total(x, self.compute_features.hop) for x in n]
        one = torch.ones(1, device=wavs.device)
        outs = [self.encode(wavs[b:b + 1, :x], one, epoch) for b, x in enumerate(n)]
        enc = torch.zeros((len(n), max(rows), outs[0].shape[-1]), dtype=outs[0].dtype, device=wavs.device)
        for b, e in enumerate(outs):
            assert e.shape[1] == rows[b], (e.shape, rows[b])
            enc[b, :rows[b]] = e[0]
        return enc, fused.RowLens(rows, torch.tensor(rows, dtype=torch.int32).to(wavs.device))

    def encode_streaming(self, src, context, lens=None):
        """The next chunk of the CNN front end's output rows (B, t, F, C) or (B, t, F * C) of the streams in ``context``
        (self.Transformer.make_streaming_context(None, dict(batch_size=B))) -> encoder output (B, t, d_model).  The rows come
        from the whole-utterance front end or, chunk by chunk from the waveform, from frontend_streaming; encode_wav_streaming
        does both steps.  ``lens``: a device int32 (B,) tensor, slot b advances by its first lens[b] <= t rows only (0: it idles);
        output rows at and past lens[b] are unspecified (fused.forward_streaming)."""
        return self.Transformer.encode_streaming(src, context, lens)

    def make_streaming_context(self, batch_size, dtype=None, per_slot=False):
        """A blank context for streaming ``batch_size`` utterances in lock step from the waveform: ``.frontend``
        (fused.FrontEndStreamingContext) and ``.encoder`` (self.Transformer.make_streaming_context(None, dict(batch_size=B))), with
        ``reset()`` for the start of the next utterance on all streams.  ``dtype``: the compute dtype of both (default: the
        autocast dtype when enabled, else the parameters')."""
        from . import fused
        p = self.ctc_lin.w.weight
        if dtype is None:
            dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else p.dtype
        enc = self.Transformer.make_streaming_context(None, dict(batch_size=batch_size, dtype=dtype))
        if per_slot:       # every slot at its own sample, ending and restarting on its own: encode_wav_slots / log_probs_wav_slots, reset(rows)
            return fused.SlotASRStreamingContext(fused.SlotFrontEndStreamingContext(batch_size, p.device, dtype), enc)
        return fused.ASRStreamingContext(fused.FrontEndStreamingContext(batch_size, p.device, dtype), enc)

    def frontend_streaming(self, wav_chunk, ctx, last=False):
        """The next samples (B, n), any n >= 0, of the streams in ``ctx`` (make_streaming_context) -> the CNN front end's rows that
        became final, (B, t, 640) with t = 0 allowed; ``last`` ends the utterance and flushes its remaining rows
        (fused.frontend_streaming: the look-ahead is 46 ms at the CTC-large settings, and the top_db clamp is the causal one of
        sb_compat.Fbank(causal_top_db=True))."""
        from . import fused
        return fused.frontend_streaming(self, wav_chunk, ctx.frontend, last)

    def encode_wav_streaming(self, wav_chunk, ctx, last=False):
        """frontend_streaming's rows through encode_streaming -> (B, t, d_model); no encoder launch when no row is ready."""
        rows = self.frontend_streaming(wav_chunk, ctx, last)
        if rows.shape[1] == 0:
            return torch.zeros((rows.shape[0], 0, self.cfg.d_model), dtype=torch.float32, device=rows.device)
        return self.encode_streaming(rows, ctx.encoder)

    def encode_wav_slots(self, wav_chunk, n_valid, ctx, last=False):
        """Every slot at its own pace from the waveform: fused.frontend_streaming_slots (wav_chunk (B, n_max), slot b hands over its
        first n_valid[b] samples, last[b] ends its utterance) through encode_streaming with the per-slot row counts ->
        (enc (B, t_max, d_model), row_lens); rows at and past row_lens[b] are unspecified.  ``ctx``: make_streaming_context(B,
        per_slot=True).  No encoder launch when no slot has a row."""
        from . import fused
        rows, row_lens = fused.frontend_streaming_slots(self, wav_chunk, n_valid, ctx.frontend, last)
        if rows.shape[1] == 0:
            return torch.zeros((rows.shape[0], 0, self.cfg.d_model), dtype=torch.float32, device=rows.device), row_lens
        return self.encode_streaming(rows, ctx.encoder, lens=row_lens.dev), row_lens

    def log_probs_wav_slots(self, wav_chunk, n_valid, ctx, last=False):
        """encode_wav_slots through the CTC head -> (log-probabilities (B, t_max, vocab), row_lens):
        StreamingCTCBeamSearcher.step(lp, state, lengths=row_lens) takes both as they are."""
        enc, row_lens = self.encode_wav_slots(wav_chunk, n_valid, ctx, last)
        return torch.log_softmax(self.ctc_lin(enc), dim=-1), row_lens

    def log_probs_wav_streaming(self, wav_chunk, ctx, last=False):
        """encode_wav_streaming's chunk through the CTC head, (B, t, vocab): what ctc_decode.StreamingCTCBeamSearcher.step consumes."""
        return torch.log_softmax(self.ctc_lin(self.encode_wav_streaming(wav_chunk, ctx, last)), dim=-1)

    def log_probs_streaming(self, src, context, lens=None):
        """encode_streaming's chunk through the CTC head: log_softmax(ctc_lin(encode_streaming(src, context))), (B, t, vocab) --
        what ctc_decode.StreamingCTCBeamSearcher.step consumes; with ``lens`` (per-slot row counts) hand the same tensor to it as
        ``lengths``."""
        return torch.log_softmax(self.ctc_lin(self.encode_streaming(src, context, lens)), dim=-1)

    def forward_ctc(self, wavs, wav_lens, epoch=0, augment=None, feats=None):
        """-> log-probabilities (B, T', vocab), train_CTC.py:296-302."""
        enc = self.encode(wavs, wav_lens, epoch, augment, feats=feats)
        return torch.log_softmax(self.ctc_lin(enc), dim=-1)

    def forward_s2s(self, wavs, wav_lens, tokens_bos, epoch=0, augment=None, pad_idx=0, feats=None):
        """train_S2S.py:285-320: features -> CNN -> Transformer(src, <bos> tokens) -> (p_ctc over encoder steps,
        p_seq over decoder steps), both log-probabilities."""
        assert self.cfg.num_decoder_layers > 0, "forward_s2s needs a decoder (S2S configuration)"
        src = self.CNN(self.features(wavs, wav_lens, epoch, augment) if feats is None else feats)
        enc_out, pred = self.Transformer(src, tokens_bos, wav_lens, pad_idx=pad_idx)
        return torch.log_softmax(self.ctc_lin(enc_out), dim=-1), torch.log_softmax(self.seq_lin(pred), dim=-1)

    @torch.no_grad()
    def transcribe_s2s(self, wavs, wav_lens, searcher=None, ctc_weight=None, beam_size=None, length_normalization=True,
                       temperature=1.0, topk=1, lm_scorer=None, lm_weight=None, ragged=False):
        """wav (B, samples) -> (hyps, lengths, scores, log_probs) of the S2S searcher (s2s_decode.S2SGreedySearcher with the
        config's bos / eos indices and decode ratios unless ``searcher`` is given): frontend -> encode -> token loop on
        the stepped decoder (Mamba, or Transformer with the memory frames beyond each utterance's length masked).  What train_S2S.py:382-394 does at its VALID / TEST stages.  ``ctc_weight`` (the recipes'
        ``ctc_weight_decode``, 0.40): joint CTC/attention decoding, the CTC prefix score of log_softmax(ctc_lin(encoder
        output)) added with this weight to every token's log-probability; None: the decoder alone.  ``beam_size`` (the recipes'
        valid_beam_size 10 / test_beam_size 66): s2s_decode.S2SBeamSearcher with ``length_normalization``, ``temperature`` and
        ``topk``; None: the greedy searcher.  ``lm_scorer`` / ``lm_weight`` (the recipes' TransformerLMScorer at lm_weight 0.60):
        a language model as a second scorer of the beam search (s2s_decode.TransformerLMScorer); both need ``beam_size``.
        ``ragged=True``: encode(..., ragged=True), every utterance encoded as if alone, and the searcher gets relative lengths that
        reproduce row_lens exactly (row_lens[b] / rows of the batch)."""
        assert self.cfg.num_decoder_layers > 0, "transcribe_s2s needs a decoder (S2S configuration)"
        assert not self.training, "transcribe_s2s is the inference path: call eval() first"
        if searcher is not None and ctc_weight is not None:
            raise ValueError("transcribe_s2s: give either a searcher or ctc_weight (a searcher carries its own)")
        if searcher is not None and (beam_size is not None or length_normalization is not True or temperature != 1.0 or topk != 1):
            raise ValueError("transcribe_s2s: give either a searcher or beam_size / length_normalization / temperature / topk "
                             "(a searcher carries its own)")
        if searcher is not None and (lm_scorer is not None or lm_weight is not None):
            raise ValueError("transcribe_s2s: give either a searcher or lm_scorer / lm_weight (a searcher carries its own)")
        if searcher is None and beam_size is None and (lm_scorer is not None or lm_weight is not None):
            raise ValueError("transcribe_s2s: lm_scorer / lm_weight belong to the beam search: give beam_size")
        if searcher is None and beam_size is None and (length_normalization is not True or temperature != 1.0 or topk != 1):
            raise ValueError("transcribe_s2s: length_normalization / temperature / topk belong to the beam search: give beam_size")
        if searcher is None:
            from .s2s_decode import S2SBeamSearcher, S2SGreedySearcher
            args = dict(bos_index=self.cfg.bos_index, eos_index=self.cfg.eos_index, min_decode_ratio=self.cfg.min_decode_ratio,
                        max_decode_ratio=self.cfg.max_decode_ratio)
            modules = [self.Transformer, self.seq_lin]
            if ctc_weight is not None:
                modules.append(self.ctc_lin)
                args.update(ctc_weight=ctc_weight, blank_index=self.cfg.blank_index)
            if beam_size is None:
                searcher = S2SGreedySearcher(modules=modules, **args)
            else:
                searcher = S2SBeamSearcher(modules=modules, beam_size=beam_size, length_normalization=length_normalization,
                                           temperature=temperature, topk=topk, lm_scorer=lm_scorer,
                                           lm_weight=0.0 if lm_weight is None else lm_weight, **args)
        if ragged:
            enc, row_lens = self.encode(wavs, wav_lens, ragged=True)
            # the searchers round rel * rows: (r + 0.25) / rows rounds to r for every 0 < r <= rows (no tie, no float edge)
            rel = torch.tensor([min(1.0, (r + 0.25) / enc.shape[1]) for r in row_lens], dtype=torch.float32, device=enc.device)
            # rows past an utterance's own are unspecified (NaN included) and the Mamba decoder reads the whole memory: zeros there
            own = torch.arange(enc.shape[1], device=enc.device)[None, :, None] < row_lens.dev.to(enc.device)[:, None, None]
            return searcher(torch.where(own, enc, torch.zeros((), dtype=enc.dtype, device=enc.device)), rel)
        return searcher(self.encode(wavs, wav_lens), wav_lens)

    @property
    def row_seconds(self) -> float:
        """Nominal duration of one encoder row: hop x (product of the CNN's time strides) / sample_rate (0.04 s in the recipe)."""
        stride = 1
        for blk in self.CNN.blocks:
            stride *= int(blk.conv.stride[0])
        return self.compute_features.hop * stride / float(self.cfg.sample_rate)

    @torch.no_grad()
    def align(self, wavs, wav_lens, targets, target_lens, aligner):
        """CTC forced alignment of known transcripts: encode(..., ragged=True), the CTC head, then ``aligner`` (a
        ctc_decode.CTCAligner) with lengths=row_lens -> List[CTCAlignment] with token_times / word_times filled, (start, end) in
        seconds.  Runs in eval mode (the caller's mode is restored).  The times are NOMINAL row times, frame x row_seconds: row r is
        taken to cover [r, r + 1) x row_seconds although the front end's receptive field is wider and centred frames start half a
        window early; a span's end is clipped to the utterance's duration."""
        from . import fused
        was_training = self.training
        self.eval()
        try:
            enc, row_lens = self.encode(wavs, wav_lens, ragged=True)
            lp = torch.log_softmax(self.ctc_lin(enc), dim=-1)
            out = aligner(lp, targets, target_lens, lengths=row_lens)
        finally:
            self.train(was_training)
        n = fused.ragged_sample_counts(wav_lens, wavs.shape[1], self.compute_features.hop)
        rs = self.row_seconds
        for al, samples in zip(out, n):
            dur = samples / float(self.cfg.sample_rate)
            al.token_times = [(a * rs, min(z * rs, dur)) for a, z in al.token_frames]
            al.word_times = [(a * rs, min(z * rs, dur)) for a, z in al.word_frames]
        return out

    def s2s_objective(self, p_ctc, p_seq, tokens, tokens_lens, tokens_eos, tokens_eos_lens, wav_lens, ctc_weight=0.3,
                      label_smoothing=0.1, pad_idx=0):
        """train_S2S.py:518-529: ctc_weight * CTC(p_ctc, tokens) + (1 - ctc_weight) * label-smoothed KL(p_seq, tokens_eos)."""
        loss_seq = sb.kldiv_loss(p_seq, tokens_eos, length=tokens_eos_lens, label_smoothing=label_smoothing, pad_idx=pad_idx,
                                 reduction="batchmean")
        loss_ctc = sb.ctc_loss(p_ctc, tokens, wav_lens, tokens_lens, self.cfg.blank_index, reduction="batchmean")
        return ctc_weight * loss_ctc + (1.0 - ctc_weight) * loss_seq

    def ctc_objective(self, p_ctc, tokens, wav_lens, tokens_lens):
        """train_CTC.py:405 with loss_reduction batchmean."""
        return sb.ctc_loss(p_ctc, tokens, wav_lens, tokens_lens, self.cfg.blank_index, reduction="batchmean")


def synthetic_wavs(batch: int, n_samples: int, seed: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """16 kHz waveforms 0.1*N(0,1) clipped to [-1, 1], all utterances full length."""
    g = torch.Generator().manual_seed(seed)
    wav = (0.1 * torch.randn(batch, n_samples, generator=g)).clamp_(-1.0, 1.0)
    return wav.to(device), torch.ones(batch, device=device)


def samples_for_frames(n_frames: int, hop: int = 160) -> int:
    """Fbank with centre padding yields 1 + floor(samples / hop) frames."""
    return (n_frames - 1) * hop
