"""SequenceScorer's host logic without a GPU: K.score_targets is replaced by a torch stand-in (the kernel has its own tests) and the
models are toys that return fixed logits.  What is checked is what the class itself does: eval mode and its restoration, the
reference's slices (pad stripping, start_indices, tgt_len), the result's keys and shapes, and its refusals."""
import math

import pytest
import torch

from fbk_fairseq_st_amd import sequence_scorer as SS
from fbk_fairseq_st_amd.data import Dictionary

PAD, EOS = 1, 2
V = 23


def _standin(calls):
    def score_targets(logits_list, target):
        calls.append(len(logits_list))
        lp = torch.stack([torch.log_softmax(x.double(), -1).gather(2, target.unsqueeze(-1))[..., 0] for x in logits_list])
        return (torch.logsumexp(lp, 0) - math.log(len(logits_list))).float()
    return score_targets


class Toy:
    """a model: fixed logits [B, L, V] per call, records the mode it was run in and the keyword arguments it got"""

    def __init__(self, seed, B, L, dtype=torch.float32, training=True, Ts=5):
        g = torch.Generator().manual_seed(seed)
        self.logits = (torch.randn(B, L, V, generator=g) * 2).to(dtype)
        self.attn = torch.softmax(torch.randn(B, L, Ts, generator=g), -1)
        self.training = training
        self.seen_mode, self.seen_kw = [], []

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self

    def __call__(self, src_tokens, src_lengths, prev_output_tokens, **kw):
        self.seen_mode.append(self.training)
        self.seen_kw.append(kw)
        return self.logits, {"attn": [self.attn if kw.get("need_attn") else None], "inner_states": None}


class ToyPair(Toy):
    def __call__(self, *a, **kw):
        out = super().__call__(*a, **kw)
        return (out[0], out[1]), (out[0], out[1])


def _sample(lens, L):
    B = len(lens)
    g = torch.Generator().manual_seed(7)
    target = torch.full((B, L), PAD, dtype=torch.int64)
    for b, n in enumerate(lens):
        target[b, :n - 1] = torch.randint(4, V, (n - 1,), generator=g)
        target[b, n - 1] = EOS
    return dict(net_input=dict(src_tokens=torch.zeros(B, 9, 80), src_lengths=torch.full((B,), 9), prev_output_tokens=target.clone()),
                target=target)


@pytest.fixture
def calls(monkeypatch):
    c = []
    monkeypatch.setattr(SS.K, "score_targets", _standin(c))
    return c


def _expect(models, target):
    lp = torch.stack([torch.log_softmax(m.logits.double(), -1).gather(2, target.unsqueeze(-1))[..., 0] for m in models])
    return torch.logsumexp(lp, 0) - math.log(len(models))


def test_result_fields_pad_stripping_and_one_launch(calls):
    lens, L = [6, 1, 4], 6
    sample = _sample(lens, L)
    models = [Toy(1, 3, L), Toy(2, 3, L)]
    hyps = SS.SequenceScorer(Dictionary.synthetic(V)).generate(models, sample)
    assert calls == [2], "all members go into one K.score_targets call"
    exp = _expect(models, sample["target"])
    assert len(hyps) == 3
    for b, hs in enumerate(hyps):
        assert len(hs) == 1 and sorted(hs[0]) == ["alignment", "attention", "positional_scores", "score", "tokens"]
        h = hs[0]
        n = lens[b]
        assert torch.equal(h["tokens"], sample["target"][b, :n]) and not bool((h["tokens"] == PAD).any())
        assert h["positional_scores"].shape == (n,) and h["positional_scores"].dtype == torch.float32
        assert torch.allclose(h["positional_scores"].double(), exp[b, :n], atol=1e-6)
        assert torch.is_tensor(h["score"]) and h["score"].dim() == 0 and h["score"].dtype == torch.float32
        assert abs(float(h["score"]) - float(exp[b, :n].sum() / n)) < 1e-5
        assert h["attention"] is None and h["alignment"] is None
    assert all(kw == {} for m in models for kw in m.seen_kw), "need_attn is asked for only with compute_alignment"


def test_start_indices_follow_the_reference_slices(calls):
    lens, L = [6, 1, 4], 6
    sample = _sample(lens, L)
    sample["start_indices"] = [2, 0, 3]
    m = Toy(3, 3, L)
    hyps = SS.SequenceScorer(Dictionary.synthetic(V)).generate([m], sample)
    exp = _expect([m], sample["target"])
    for b, (st, n) in enumerate(zip(sample["start_indices"], lens)):
        h = hyps[b][0]
        assert torch.equal(h["tokens"], sample["target"][b, st:n])
        assert torch.allclose(h["positional_scores"].double(), exp[b, st:n], atol=1e-6)
        assert abs(float(h["score"]) - float(exp[b, st:n].sum() / (n - st))) < 1e-5
    assert hyps[1][0]["tokens"].tolist() == [EOS] and hyps[2][0]["positional_scores"].shape == (1,)


def test_modes_are_set_for_the_call_and_restored(calls):
    sample = _sample([3, 2], 3)
    a, b = Toy(1, 2, 3, training=True), Toy(2, 2, 3, training=False)
    SS.SequenceScorer(Dictionary.synthetic(V)).generate([a, b], sample)
    assert a.seen_mode == [False] and b.seen_mode == [False], "every member runs in eval mode"
    assert a.training is True and b.training is False, "the flags are put back"
    bad = ToyPair(3, 2, 3, training=True)
    with pytest.raises(TypeError):
        SS.SequenceScorer(Dictionary.synthetic(V)).generate([bad], sample)
    assert bad.training is True, "restored after a refusal too"


def test_refusals(calls):
    sample = _sample([3, 2], 3)
    sc = SS.SequenceScorer(Dictionary.synthetic(V))
    with pytest.raises(ValueError, match="1..8"):
        sc.generate([Toy(i, 2, 3) for i in range(9)], sample)
    with pytest.raises(ValueError, match="1..8"):
        sc.generate([], sample)
    with pytest.raises(ValueError, match=r"float32.*bfloat16"):
        sc.generate([Toy(1, 2, 3), Toy(2, 2, 3, dtype=torch.bfloat16)], sample)
    with pytest.raises(TypeError, match="ToyPair"):
        sc.generate([ToyPair(1, 2, 3)], sample)
    assert calls == [], "nothing was scored"
    sc.generate([Toy(i, 2, 3) for i in range(8)], sample)
    assert calls == [8]


def test_softmax_batch_is_accepted_and_ignored(calls):
    sample = _sample([5, 3], 5)
    m = Toy(4, 2, 5)
    d = Dictionary.synthetic(V)
    a = SS.SequenceScorer(d).generate([m], sample)
    b = SS.SequenceScorer(d, softmax_batch=2).generate([m], sample)                  # smaller than B * L: the reference would chunk
    assert calls == [1, 1]
    for x, y in zip(a, b):
        assert torch.equal(x[0]["positional_scores"], y[0]["positional_scores"]) and torch.equal(x[0]["score"], y[0]["score"])


def test_alignment_on_request(calls):
    lens, L = [5, 3], 5
    sample = _sample(lens, L)
    models = [Toy(5, 2, L, Ts=6), Toy(6, 2, L, Ts=6)]
    sc = SS.SequenceScorer(Dictionary.synthetic(V), compute_alignment=True)
    hyps = sc.generate(models, sample)
    assert all(kw == {"need_attn": True} for m in models for kw in m.seen_kw)
    avg = (models[0].attn + models[1].attn) / 2
    for b, n in enumerate(lens):
        h = hyps[b][0]
        assert h["attention"].shape == (6, n) and torch.allclose(h["attention"], avg[b, :n].t(), atol=1e-6)
        want = [(int(avg[b, t].argmax()), t) for t in range(n) if int(sample["target"][b, t]) not in (PAD, EOS)]
        assert h["alignment"] == want
    with pytest.raises(ValueError, match="differ in length"):
        sc.generate([Toy(5, 2, L, Ts=6), Toy(6, 2, L, Ts=7)], sample)
    short = Toy(6, 2, L, Ts=6)                                   # the same width, but sentence 0 ends one frame earlier
    short.attn[0, :, -1] = 0
    with pytest.raises(ValueError, match="differ in length"):
        sc.generate([Toy(5, 2, L, Ts=6), short], sample)


def test_generator_keeps_its_alignment_rule():
    """the rule moved into sequence_generator.hard_alignment: SequenceGenerator._hard_alignment still answers as before"""
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator, hard_alignment
    attn = torch.tensor([[0.1, 0.7, 0.2], [0.6, 0.1, 0.3], [0.3, 0.2, 0.5]])          # Ts x tgt_len
    toks = torch.tensor([5, 6, EOS])
    gen = SequenceGenerator.__new__(SequenceGenerator)
    gen.pad, gen.eos = PAD, EOS
    assert gen._hard_alignment(attn, 3, toks) == hard_alignment(attn, toks, PAD, EOS) == [(1, 0), (0, 1)]
    assert hard_alignment(attn[:, :0], toks[:0], PAD, EOS) == []
