"""SequenceScorer on the GPU: against fairseq's own SequenceScorer (tests/golden/scorer.npz, made by tests/golden/make_scorer_fixture.py),
against the device-resident search (teacher forcing a hypothesis reproduces its scores), in bf16 against the existing route on the very
logits of the same forward, and with compute_alignment."""
import math

import numpy as np
import pytest
import torch

from helpers import load_golden
from score_ref import assert_scores, log_softmax_bound, score_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, EOS = 1, 2
U = 2.0 ** -24
_MODELS = {}


def models(dtype):
    """model_a and model_b of the golden fixtures (tests/test_model_gpu.py builds them), once per dtype"""
    if dtype not in _MODELS:
        import test_model_gpu as TM
        built = [TM.build(name, dtype) for name in ("model_a", "model_b")]
        _MODELS[dtype] = ([b[5] for b in built], [b[1] for b in built], [b[0]["meta"] for b in built])
    return _MODELS[dtype]


def fixture_sample(g):
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    return dict(net_input=dict(src_tokens=t("src_tokens"), src_lengths=t("src_lengths"), prev_output_tokens=t("prev_output_tokens")),
                target=t("target"))


def tgt_dict():
    from fbk_fairseq_st_amd.data import Dictionary
    return Dictionary.synthetic(96)


# ------------------------------------------------------------------ (a) the reference's scorer
@pytest.mark.parametrize("case", ["one", "ens", "start"])
def test_matches_the_reference_scorer(case):
    """f32 engine against fairseq/sequence_scorer.py on the CPU in f32: tokens exact, positional scores and score within 1e-4 absolute
    (the tolerance the generator fixtures and the teacher top-k dump are held to in f32).  `ens` / `start`: the reference averages
    probabilities, this class combines in log space; the fixture's maker asserted every averaged probability > 1e-30."""
    from fbk_fairseq_st_amd.sequence_scorer import SequenceScorer
    g = load_golden("scorer")
    ms, _, metas = models(torch.float32)
    assert np.array_equal(g["meta_a"], metas[0]) and np.array_equal(g["meta_b"], metas[1]), "the fixture was made for other models"
    sample = fixture_sample(g)
    if case == "start":
        sample["start_indices"] = [int(v) for v in g["start_indices"]]
    hyps = SequenceScorer(tgt_dict()).generate(ms[:1] if case == "one" else ms, sample)
    assert len(hyps) == g["target"].shape[0]
    for b, hs in enumerate(hyps):
        n = int(g[case + "_len"][b])
        h = hs[0]
        assert h["tokens"].tolist() == g[case + "_tokens"][b, :n].tolist()
        assert h["positional_scores"].shape == (n,) and h["positional_scores"].dtype == torch.float32 and h["positional_scores"].is_cuda
        err = np.abs(h["positional_scores"].cpu().numpy().astype(np.float64) - g[case + "_pos"][b, :n])
        print("%s sentence %d: positional |err| max %.3g, score |err| %.3g" % (case, b, err.max(), abs(float(h["score"]) - g[case + "_score"][b])))
        assert err.max() <= 1e-4, (case, b, err)
        assert abs(float(h["score"]) - float(g[case + "_score"][b])) <= 1e-4
        assert h["attention"] is None and h["alignment"] is None


# ------------------------------------------------------------------ (b) teacher forcing reproduces the search
def test_scoring_the_best_hypothesis_reproduces_its_scores():
    """the best hypothesis of every sentence of generate fixture case `c`, found by the device-resident search in f32, scored as the
    target: the scorer's positional scores are the hypothesis' own within 2e-4 (both sides are held to the reference at 1e-4)"""
    import test_model_gpu as TM
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    from fbk_fairseq_st_amd.sequence_scorer import SequenceScorer
    task, model, src, lens, opts, exp, _ = TM.build_gen("c")
    gen = SequenceGenerator([model], task.target_dictionary, **opts)
    hyps = gen.generate([model], dict(net_input=dict(src_tokens=src, src_lengths=lens)))
    assert "launches_per_step" in gen.last_stats, "the search did not take the device route"
    best = [hs[0] for hs in hyps]
    B, L = len(best), max(int(h["tokens"].numel()) for h in best)
    target = torch.full((B, L), PAD, dtype=torch.int64, device=DEV)
    prev = torch.full((B, L), PAD, dtype=torch.int64, device=DEV)
    for b, h in enumerate(best):
        n = int(h["tokens"].numel())
        assert int(h["tokens"][-1]) == EOS
        target[b, :n] = h["tokens"]
        prev[b, 0] = EOS
        prev[b, 1:n] = h["tokens"][:-1]
    sample = dict(net_input=dict(src_tokens=src, src_lengths=lens, prev_output_tokens=prev), target=target)
    scored = SequenceScorer(task.target_dictionary).generate([model], sample)
    for b, h in enumerate(best):
        s = scored[b][0]
        assert torch.equal(s["tokens"], h["tokens"])
        err = (s["positional_scores"].double() - h["positional_scores"].double().to(DEV)).abs()
        print("sentence %d (%d tokens): |err| max %.3g" % (b, h["tokens"].numel(), float(err.max())))
        assert float(err.max()) <= 2e-4, (b, err.tolist())


# ------------------------------------------------------------------ (c) bf16 engine: the same logits, both routes
@pytest.mark.parametrize("n", [1, 2])
def test_bf16_engine_equals_the_existing_route_on_the_same_logits(n, monkeypatch):
    """no model-level tolerance: the logits the scorer handed to K.score_targets are caught, and its output is compared with the
    gather of get_normalized_probs (n = 1) / the log of the mean of the members' gathered probabilities in float64 (n = 2) of those
    very tensors, within the kernel's bound (score_ref) plus the bound K.log_softmax is held to"""
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.sequence_scorer import SequenceScorer
    ms, _, _ = models(torch.bfloat16)
    ms = ms[:n]
    sample = fixture_sample(load_golden("scorer"))
    seen = {}
    real = K.score_targets

    def spy(logits_list, target):
        seen["logits"] = list(logits_list)
        seen["out"] = real(logits_list, target)
        return seen["out"]
    monkeypatch.setattr(K, "score_targets", spy)
    hyps = SequenceScorer(tgt_dict()).generate(ms, sample)
    logits, target = seen["logits"], sample["target"]
    assert len(logits) == n and all(x.dtype == torch.bfloat16 for x in logits)
    ref, bound = score_ref(logits, target)
    assert_scores(seen["out"], ref, bound, "bf16 engine, n=%d, against float64 of the same logits" % n)
    gathered, gb = [], []
    for m, x in zip(ms, logits):
        lp = m.get_normalized_probs((x, None), log_probs=True)
        assert lp.dtype == torch.float32 and lp.shape == x.shape
        gathered.append(lp.gather(2, target.unsqueeze(-1))[..., 0].double())
        gb.append(log_softmax_bound(x.double()).gather(2, target.unsqueeze(-1))[..., 0])
    old = gathered[0] if n == 1 else torch.logsumexp(torch.stack(gathered), 0) - math.log(n)
    old_bound = torch.stack(gb).max(0).values
    err = (seen["out"].double() - old).abs()
    assert bool((err <= bound + old_bound).all()), "worst %.3g" % float((err / (bound + old_bound)).max())
    for b, hs in enumerate(hyps):                               # and the class slices that tensor
        k = int(hs[0]["tokens"].numel())
        assert torch.equal(hs[0]["positional_scores"], seen["out"][b, :k])


# ------------------------------------------------------------------ (d) compute_alignment
def test_compute_alignment():
    """attention is Ts x tgt_len with columns that sum to 1 -- within 2 (29 + heads) u, the floor of the per-row bound
    tests/test_attention_modes_gpu.py holds s2t_attn_probs_avg to (its terms for the scores' and the logarithms' errors left out:
    never wider than that bound), plus 2u for the average over members; alignment is the arg-max rule recomputed here; members whose
    encoder lengths differ are refused"""
    from fbk_fairseq_st_amd.sequence_scorer import SequenceScorer
    ms, cfgs, _ = models(torch.float32)
    g = load_golden("scorer")
    sample = fixture_sample(g)
    sc = SequenceScorer(tgt_dict(), compute_alignment=True)
    hyps = sc.generate(ms[:1], sample)
    plain = SequenceScorer(tgt_dict()).generate(ms[:1], sample)
    for b, hs in enumerate(hyps):
        h = hs[0]
        n = int(g["one_len"][b])
        att = h["attention"]
        assert att.dim() == 2 and att.shape[1] == n and att.dtype == torch.float32
        sums = att.double().sum(0)
        assert float((sums - 1).abs().max()) <= 2 * (29 + cfgs[0]["heads"]) * U + 2 * U, sums.tolist()
        want = [(int(att[:, t].argmax()), t) for t in range(n) if int(h["tokens"][t]) not in (PAD, EOS)]
        assert h["alignment"] == want
        assert torch.equal(h["positional_scores"], plain[b][0]["positional_scores"]), "asking for attention changed the scores"
    # model_a and model_b compress the same utterances to different lengths (CTC compression): their maps cannot be averaged
    with pytest.raises(ValueError, match="differ in length"):
        sc.generate(ms, sample)
