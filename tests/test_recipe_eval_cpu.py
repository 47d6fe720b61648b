"""The CTC recipe's evaluation stages with the YAML's own wer_computer / cer_computer, on the CPU: a RecipeBrain subclass that does
what the reference's script does with them (train_CTC.py:407-420 append in compute_objectives, :625-626 summarize("error_rate") in
on_stage_end, write_stats after the TEST stage) -- VALID decodes greedily (CTCGreedyDecoder), TEST by beam search -- on a
two-layer model, four synthetic utterances and a toy vocabulary.  WER and CER equal tests/ctc_score_ref.py's on the same token lists.

Two parts of the recipe have no host implementation, and on the CPU the brain takes their references instead: the forward from
waveform to log-probabilities is the fp64 oracle over the recipe's own weights (tests/test_dropout_live_step._oracle_logp), and the
TEST stage searches with tests/ctc_beam_ref.py under the recipe's keywords (the reference the GPU searcher is pinned to).  The
loss, the greedy decode and the scoring are the package's.  tests/test_recipe_eval_gpu.py runs the same brain on the GPU."""
import io
import os

import torch

import ctc_beam_data as D
import ctc_beam_ref as BR
import ctc_score_ref as SR
import test_dropout_live_step as L                          # its fp64 oracle forward over the recipe's modules
from recipe_brain import RecipeBrain, load_recipe
from mamba_asr_amd.brain import Stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = os.path.join(ROOT, "tests", "golden", "conmamba_large_ctc.yaml")
TRANSCRIPTS = ["THE CAT SAT", "A DOG", "IT'S HERE NOW", "OH"]


class EvalBrain(RecipeBrain):
    """batch = (wavs, wav_lens, tokens, tokens_lens, ids, wrd).  ``scorer_device``: where the YAML's scorers score (None: host);
    ``also_host``: a second pair of host scorers fed the same words."""

    def __init__(self, hp, run_opts=None, vocab_list=None, scorer_device=None, also_host=False):
        super().__init__(hp, run_opts=run_opts, vocab_list=vocab_list)
        self.scorer_device, self.also_host = scorer_device, also_host
        self.greedy, self.stats, self.seen, self.report = None, {}, {}, {}

    def on_stage_start(self, stage, epoch=None):
        if stage != Stage.TRAIN:
            kw = {} if self.scorer_device is None else {"device": self.scorer_device}
            self.cer_metric, self.wer_metric = self.hparams.cer_computer(**kw), self.hparams.wer_computer(**kw)
            if self.also_host:
                self.host_cer, self.host_wer = self.hparams.cer_computer(), self.hparams.wer_computer()
            self.seen[stage] = ([], [])

    def compute_forward(self, batch, stage):
        if stage == Stage.TRAIN or (stage == Stage.TEST and self.device.type == "cuda"):
            return super().compute_forward(batch, stage)
        wavs, wav_lens = batch[0].to(self.device), batch[1].to(self.device)
        if self.device.type == "cuda":                                       # RecipeBrain's forward, without its own VALID decode
            src = self.modules.CNN(self._features(wavs, wav_lens, stage))
            enc_out, _ = self.modules.Transformer(src, tgt=None, wav_len=wav_lens)
            p_ctc = self.hparams.log_softmax(self.modules.ctc_lin(enc_out))
        else:                                                                # the Mamba mixer has no host path: the fp64 oracle forward
            p_ctc = L._oracle_logp(self.oracle_cfg, self.modules, wavs, None)[1].detach().float()
        if stage == Stage.VALID:
            if self.greedy is None:
                from mamba_asr_amd.ctc_decode import CTCGreedyDecoder
                self.greedy = CTCGreedyDecoder(self.hparams.blank_index, self.vocab_list)
            return p_ctc, wav_lens, self.greedy.tokens(p_ctc, wav_lens)
        kw = dict(self.hparams.test_beam_search)
        blank = kw.pop("blank_index")
        steps = p_ctc.shape[1]
        texts = [BR.beam_search(p_ctc[b].double().tolist(), int(round(rel * steps)), self.vocab_list, blank=blank, **kw)[0][0]
                 for b, rel in enumerate(wav_lens.tolist())]
        return p_ctc, wav_lens, texts

    def compute_objectives(self, predictions, batch, stage):
        loss = super().compute_objectives(predictions, batch, stage)
        if stage == Stage.TRAIN:
            return loss
        predicted = predictions[2]
        if stage == Stage.VALID:                                             # the tokenizer's decode_from_list
            predicted_words = [self.greedy.compose(tok).split(" ") for tok in predicted]
        else:
            predicted_words = [(hyp if isinstance(hyp, str) else hyp[0].text).split(" ") for hyp in predicted]
        ids, target_words = batch[4], [wrd.split(" ") for wrd in batch[5]]
        metrics = [self.wer_metric, self.cer_metric] + ([self.host_wer, self.host_cer] if self.also_host else [])
        for m in metrics:
            m.append(ids, predicted_words, target_words)
        self.seen[stage][0].extend(predicted_words)
        self.seen[stage][1].extend(target_words)
        return loss

    def on_stage_end(self, stage, stage_loss, epoch=None):
        if stage == Stage.TRAIN:
            return
        self.stats[stage] = {"loss": stage_loss, "CER": self.cer_metric.summarize("error_rate"), "WER": self.wer_metric.summarize("error_rate")}
        if stage == Stage.TEST:
            buf = io.StringIO()
            self.wer_metric.write_stats(buf)
            self.report[stage] = buf.getvalue()


def make_batches(device, seed=41):
    """Two batches of two utterances: synthetic audio, the transcripts' pieces as CTC targets."""
    from mamba_asr_amd.asr import samples_for_frames, synthetic_wavs
    piece = {p: k for k, p in enumerate(D.SPM_VOCAB)}
    batches = []
    for k in range(2):
        wavs, _ = synthetic_wavs(2, samples_for_frames(120), seed + k, device)
        lens = torch.tensor([1.0, 0.7], device=device)
        wavs[1, int(round(0.7 * wavs.shape[1])):] = 0.0
        wrd = TRANSCRIPTS[2 * k:2 * k + 2]
        toks = [[piece[c] for c in "▁" + w.replace(" ", "▁")] for w in wrd]
        width = max(len(t) for t in toks)
        tokens = torch.tensor([t + [0] * (width - len(t)) for t in toks])
        tok_lens = torch.tensor([len(t) / width for t in toks])
        batches.append((wavs, lens, tokens, tok_lens, [f"utt{2 * k}", f"utt{2 * k + 1}"], wrd))
    return batches


def make_brain(device, **kw):
    from dataclasses import replace
    from mamba_asr_amd.asr import CONFIGS
    hp = load_recipe(LARGE, num_encoder_layers=L.LAYERS)
    br = EvalBrain(hp, run_opts={"device": device, "precision": "fp32"}, vocab_list=D.SPM_VOCAB, **kw)
    br.oracle_cfg = replace(CONFIGS["conmamba_large_ctc"], num_encoder_layers=L.LAYERS, transformer_dropout=hp["transformer_dropout"])
    with torch.no_grad():
        hp["ctc_lin"].w.weight.mul_(3.0)          # a freshly initialised head is near uniform: sharpen it so that tokens come out
        hp["ctc_lin"].w.bias[D.SPM_VOCAB.index("▁")] += 5.0      # ... and word boundaries among them
    return hp, br


def run_stages(br, batches):
    """VALID as Brain.fit runs it, then Brain.evaluate (TEST)."""
    br.modules.eval()
    br.on_stage_start(Stage.VALID, 1)
    total = sum(float(br.evaluate_batch(b, Stage.VALID)) for b in batches)
    br.on_stage_end(Stage.VALID, total / len(batches), 1)
    br.evaluate(batches)


def check_against_the_reference(br):
    chars = lambda rows: [list("_".join(r)) for r in rows]
    for stage in (Stage.VALID, Stage.TEST):
        hyps, refs = br.seen[stage]
        assert len(hyps) == len(refs) == 4 and refs == [t.split(" ") for t in TRANSCRIPTS]
        wer, cer = SR.error_rates(refs, hyps), SR.error_rates(chars(refs), chars(hyps))
        assert br.stats[stage]["WER"] == wer[0] and br.stats[stage]["CER"] == cer[0], (stage, br.stats[stage], wer, cer)
        assert wer[2] == 9 and cer[2] == sum(len(t) for t in TRANSCRIPTS) and br.stats[stage]["loss"] > 0
        print(f"{stage}: WER {wer[0]:.2f} {wer[1]} / {wer[2]}, CER {cer[0]:.2f} {cer[1]} / {cer[2]}; hypotheses {[' '.join(h) for h in hyps]}")
    m = br.wer_metric.summarize()
    wer = SR.error_rates(br.seen[Stage.TEST][1], br.seen[Stage.TEST][0])
    head = br.report[Stage.TEST].split("\n")[0]
    assert head == f"%WER {wer[0]:.2f} [ {sum(wer[1])} / 9, {wer[1][0]} ins, {wer[1][1]} del, {wer[1][2]} sub ]" and m["num_scored_sents"] == 4
    assert br.report[Stage.TEST].count("\nref: ") == 4


def test_valid_and_test_stages_score_with_the_yamls_own_objects():
    from mamba_asr_amd import metrics
    hp, br = make_brain("cpu")
    batches = make_batches("cpu")
    run_stages(br, batches)
    assert isinstance(br.wer_metric, metrics.ErrorRateStats) and br.cer_metric.split_tokens and br.wer_metric.device is None
    check_against_the_reference(br)
    assert any(w != [""] for w in br.seen[Stage.VALID][0]), "the greedy decode produced no token at all"
    # the greedy stage's tokens are dataio.ctc_greedy_decode's
    from mamba_asr_amd import dataio
    with torch.no_grad():
        p_ctc, wav_lens, tokens = br.compute_forward(batches[0], Stage.VALID)
    assert tokens == dataio.ctc_greedy_decode(p_ctc, wav_lens, hp["blank_index"])
