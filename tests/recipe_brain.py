"""The CTC recipe's own objects driven in training order (helper of tests/test_recipe_surface_{cpu,gpu}.py; not a test file).

``load_recipe`` turns a recipe YAML into live objects through mamba_asr_amd.hparams.load_hparams; ``RecipeBrain`` is the
brain.Brain subclass a CTC training script writes on top of them.  The call sequence restates what the reference's CTC script
does with its hparams (train_CTC.py:281-312 compute_forward, :392-422 compute_objectives, on_fit_batch_end's Noam step); every
object it touches comes out of the YAML, none is built by hand."""
import torch

from mamba_asr_amd import brain, dataio
from mamba_asr_amd.brain import Stage
from mamba_asr_amd.hparams import load_hparams


def load_recipe(path, **overrides):
    """Recipe file -> the load_hparams dict.  ``data_folder`` (a !PLACEHOLDER in every recipe) defaults to a dummy path."""
    over = {"data_folder": "/nowhere"}
    over.update(overrides)
    with open(path) as f:
        return load_hparams(f, overrides=over)


class RecipeBrain(brain.Brain):
    """batch = (wavs, wav_lens, tokens, tokens_lens).  ``vocab_list``: the tokenizer's pieces, needed by the TEST stage's beam
    search only (the training script reads them from its tokenizer)."""

    def __init__(self, hp, run_opts=None, vocab_list=None):
        super().__init__(modules=hp["modules"], opt_class=hp["model_opt_class"], hparams=hp, run_opts=run_opts)
        self.vocab_list = vocab_list
        self.test_searcher = None

    def _augments(self, stage):
        return stage == Stage.TRAIN and hasattr(self.hparams, "fea_augment")

    def _features(self, wavs, wav_lens, stage):
        """Steps 1-3: Fbank, running normalisation at the counter's epoch, SpecAugment in training."""
        feats = self.hparams.compute_features(wavs)
        feats = self.modules.normalize(feats, wav_lens, epoch=self.hparams.epoch_counter.current)
        if self._augments(stage):
            feats, _ = self.hparams.fea_augment(feats, wav_lens)
        return feats

    def graph_prologue(self, batch):
        # SpectrogramDrop / Augmenter draw on the host and read .max(), the normaliser updates Python state: all of it stays
        # eager; the captured region starts at the CNN
        wavs, wav_lens, tokens, tokens_lens = (t.to(self.device) for t in batch)
        with torch.no_grad():
            feats = self._features(wavs, wav_lens, Stage.TRAIN)
        return (feats, wav_lens, tokens, tokens_lens)

    def compute_forward(self, batch, stage):
        wavs, wav_lens = batch[0].to(self.device), batch[1].to(self.device)
        # a 3-d first tensor is graph_prologue's: features already normalised and augmented
        feats = wavs if wavs.dim() == 3 else self._features(wavs, wav_lens, stage)
        src = self.modules.CNN(feats)
        enc_out, _ = self.modules.Transformer(src, tgt=None, wav_len=wav_lens)
        p_ctc = self.hparams.log_softmax(self.modules.ctc_lin(enc_out))
        p_tokens = None
        if stage == Stage.VALID:
            p_tokens = dataio.ctc_greedy_decode(p_ctc, wav_lens, self.hparams.blank_index)
        elif stage == Stage.TEST:
            if self.test_searcher is None:
                from mamba_asr_amd.ctc_decode import CTCBeamSearcher
                self.test_searcher = CTCBeamSearcher(vocab_list=self.vocab_list, **self.hparams.test_beam_search)
            p_tokens = self.test_searcher(p_ctc, wav_lens)
        return p_ctc, wav_lens, p_tokens

    def compute_objectives(self, predictions, batch, stage):
        p_ctc, wav_lens, _ = predictions
        tokens, tokens_lens = batch[2].to(self.device), batch[3].to(self.device)
        if self._augments(stage):
            tokens = self.hparams.fea_augment.replicate_labels(tokens)
            tokens_lens = self.hparams.fea_augment.replicate_labels(tokens_lens)
        return self.hparams.ctc_cost(p_ctc, tokens, wav_lens, tokens_lens).sum()

    def on_fit_batch_end(self, batch, outputs, loss, should_step):
        if should_step:
            self.hparams.noam_annealing(self.optimizer)
