"""CPU checks of the CTC beam search: the tests' host restatement against brute-force enumeration and fp64 CTC, and the
token tables CTCBeamSearcher builds for the kernel (class, H(clean), base^len(clean))."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_ref as R  # noqa: E402

INF = math.inf
VOCABS = {
    "space": ["<b>", "a", " ", "b"],
    "spm": ["<b>", "a", "▁b", "▁"],
    "plain": ["<b>", "a", "b", "c"],
}


def _logp(T, V, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn(T, V, generator=g, dtype=torch.float64) * scale, dim=-1)


def _unpruned(lp, vocab, n=None):
    T = lp.shape[0]
    return R.beam_search(lp.tolist(), T if n is None else n, vocab, blank=0, beam_size=10 ** 9, beam_prune_logp=-INF,
                         token_prune_min_logp=-INF, prune_history=False, topk=10 ** 9)


@pytest.mark.parametrize("name", sorted(VOCABS))
@pytest.mark.parametrize("T,seed", [(1, 0), (3, 1), (5, 2), (6, 3)])
def test_restatement_matches_brute_force(name, T, seed):
    vocab = VOCABS[name]
    lp = _logp(T, len(vocab), seed)
    got = dict(_unpruned(lp, vocab))
    want = R.brute_force(lp.tolist(), vocab)
    assert set(got) == set(want)
    for text, s in want.items():
        assert abs(got[text] - s) <= 1e-12, (text, got[text], s)
    if name == "plain":
        # no word-start piece: every hypothesis is a CTC label sequence, its score the CTC log-likelihood
        for text, s in got.items():
            tg = torch.tensor([[vocab.index(c) for c in text]], dtype=torch.long)
            nll = F.ctc_loss(lp.unsqueeze(1), tg.reshape(-1) if tg.numel() else tg.reshape(1, 0),
                             torch.tensor([T]), torch.tensor([tg.shape[1]]), blank=0, reduction="none")
            assert abs(-nll.item() - s) <= 1e-12, (text, s, -nll.item())


def test_restatement_edge_cases():
    vocab = VOCABS["plain"]
    lp = _logp(4, 4, 9)
    assert R.beam_search(lp.tolist(), 0, vocab) == [("", 0.0)]
    bad = lp.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError):
        R.beam_search(bad.tolist(), 4, vocab)
    R.beam_search(bad.tolist(), 2, vocab)          # NaN past n_b is not decoded


def _expect_hash(s):
    out = []
    for base in _searcher_mod().HASH_BASE:
        h, p = 0, 1
        for ch in s:
            h = (h * base + ord(ch) + 1) % ((1 << 61) - 1)
            p = p * base % ((1 << 61) - 1)
        out.append((h, p))
    return out


def _searcher_mod():
    from mamba_asr_amd import ctc_decode
    return ctc_decode


def _check_tables(s, want):
    """want: per token (class 0 char / 1 word-start / -1 blank, clean part)."""
    assert [c for c in s.classes] == [c for c, _ in want]
    assert s.clean == [c for _, c in want]
    assert s.tok_class.tolist() == [1 if c == 1 else 0 for c, _ in want]
    for v, (_, clean) in enumerate(want):
        (h1, p1), (h2, p2) = _expect_hash(clean)
        assert s.tok_hash[v].tolist() == [h1, h2] and s.tok_pow[v].tolist() == [p1, p2]
        assert 0 <= h1 < (1 << 61) - 1 and 0 <= h2 < (1 << 61) - 1


def test_token_tables():
    M = _searcher_mod()
    spm = ["<unk>", "<s>", "</s>", "▁", "E", "▁THE", "'"]
    s = M.CTCBeamSearcher(blank_index=0, vocab_list=spm, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2,
                          prune_history=False)
    assert s.is_spm
    _check_tables(s, [(-1, ""), (0, "<s>"), (0, "</s>"), (1, ""), (0, "E"), (1, "THE"), (0, "'")])
    assert s.compose([5, 4, 3, 4, 6, 3, 3]) == "THEE E'"
    sp = M.CTCBeamSearcher(blank_index=0, vocab_list=["-", "a", " ", "bc", "<unk>"], beam_size=8)
    assert not sp.is_spm
    _check_tables(sp, [(-1, ""), (0, "a"), (1, ""), (0, "bc"), (0, "<unk>")])
    assert sp.compose([2, 1, 2, 2, 3, 1, 2]) == "a bca"
    pl = M.CTCBeamSearcher(blank_index=2, vocab_list=["x", "y", "<b>"], beam_size=1)
    _check_tables(pl, [(0, "x"), (0, "y"), (-1, "")])
    assert pl.compose([0, 1, 0]) == "xyx"
    # the recipe's test_beam_search keys (hparams/CTC/conmamba_large.yaml:232-237) are all accepted
    recipe = dict(blank_index=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=False)
    r = M.CTCBeamSearcher(**recipe, vocab_list=spm)
    assert (r.beam_size, r.beam_prune_logp, r.token_prune_min_logp, r.prune_history, r.topk) == (100, -12.0, -1.2, False, 1)


def test_searcher_rejects_what_it_cannot_do():
    M = _searcher_mod()
    with pytest.raises(ValueError, match="duplicate"):
        M.CTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a", "a"])
    with pytest.raises(NotImplementedError):
        M.CTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a"], kenlm_model_path="lm.arpa")
    with pytest.raises(ValueError):
        M.CTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a"], beam_size=257)
    s = M.CTCBeamSearcher(blank_index=0, vocab_list=["<b>", "a"])
    with pytest.raises(RuntimeError, match="GPU"):
        s(torch.zeros(1, 3, 2), torch.ones(1))


def test_abi_validates_without_gpu():
    import ctypes as C
    import mamba_asr_amd._native as N
    lib = N.lib()
    a = N.CtcBeamArgs()
    assert lib.cm_ctc_beam_search(C.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    assert lib.cm_ctc_beam_search(None) == -1
    a.batch, a.T, a.V, a.beam_size, a.topk, a.lp_ts = 2, 10, 31, 100, 1, 31
    assert lib.cm_ctc_beam_search(C.byref(a)) == -1 and b"NULL" in lib.cm_last_error()
    # history T x K int32 per utterance, then (K x V -> 4096 entries) x 4 sort arrays of 8 bytes
    assert lib.cm_ctc_beam_workspace_bytes(C.byref(a)) == 2 * (10 * 100 * 4 + 4 * 8 * 4096)
    a.V = 4
    assert lib.cm_ctc_beam_workspace_bytes(C.byref(a)) == 2 * (10 * 100 * 4)
    a.beam_size = 257
    assert lib.cm_ctc_beam_workspace_bytes(C.byref(a)) == 0


def test_short_token_tables_are_refused_before_launch():
    """The preparation all three beam search wrappers share refuses token tables that do not cover the V tokens of log_probs (the
    kernels index them by token); host tensors, nothing is launched."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    V = 5
    lp = torch.zeros(2, 3, V)
    tables = dict(tok_class=torch.zeros(V, dtype=torch.int32), tok_hash=torch.zeros(V, 2, dtype=torch.int64),
                  tok_pow=torch.ones(V, 2, dtype=torch.int64))
    settings = dict(tok_len=None, hash_base=(3, 5), hash_sep=1, blank=0, beam_size=4, topk=1, prune_history=False, beam_prune_logp=-10.0,
                    token_prune_min_logp=-5.0, blank_skip_threshold=1.0)
    for what, args in (("ctc_beam_search", N.CtcBeamArgs), ("ctc_beam_stream", N.CtcBeamStreamArgs), ("ctc_beam_search_lm", N.CtcBeamLmArgs)):
        a = args()
        ops._ctc_beam_args(what, a, lp, None, **tables, **settings)
        assert (a.T, a.V, a.beam_size) == (3, V, 4)
        for name in tables:
            short = dict(tables, **{name: tables[name][:V - 1]})
            with pytest.raises(RuntimeError, match=f"{what}: token tables must cover the {V} tokens"):
                ops._ctc_beam_args(what, args(), lp, None, **short, **settings)
