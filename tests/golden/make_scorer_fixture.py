#!/usr/bin/env python3
"""Capture tests/golden/scorer.npz from the REAL reference (build container only; never at test time):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_scorer_fixture.py [--check]

fairseq/sequence_scorer.py SequenceScorer.generate on the CPU in float32 (generate.py --score-reference) over the models of the
model_a / model_b fixtures (same configurations, same weight seeds: the weights are rebuilt from the seeds and not stored), on one
batch of three ragged utterances whose right-padded targets have the lengths 7, 1 and 4 (one token, and the full width L = 7).
Three cases:

  one   model_a alone (log-probabilities gathered from log_softmax);
  ens   the ensemble model_a + model_b (probabilities averaged, log at the end);
  start the same ensemble with per-sentence `start_indices`.

Kept: the inputs (src_tokens, src_lengths, prev_output_tokens, target, start_indices), the two models' meta rows (as model_*.npz), and
per case `<case>_pos` [B, L] (positional_scores, NaN beyond a sentence's tgt_len), `<case>_score` [B], `<case>_len` [B] and
`<case>_tokens` [B, L] (-1 beyond the length).  The reference returns attention = alignment = None for these models (its
torch.is_tensor test meets the decoder's list): asserted here, nothing stored.

Every averaged target probability must exceed 1e-30 (asserted): the reference's probability-space average is then a normal f32 number
and a log-space combine must agree with it.  --check recomputes everything and compares with the stored file (exact for integers,
1e-6 for the scores) without writing.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and applies the shims listed there)

import torch  # noqa: E402
from fairseq.sequence_scorer import SequenceScorer  # noqa: E402
from oracle import s2t_ref  # noqa: E402

MIN_PROB = 1e-30
#            D   H  Ff   EL DL ctc seed     (make_golden.py: run_model_case("model_a" / "model_b"), both with --ctc-compress-out)
MODELS = [(64, 2, 128, 3, 2, 2, 100), (128, 2, 256, 2, 1, 1, 200)]
LENS, TGT_LENS, TR_LENS, SAMPLE_SEED = [45, 37, 29], [7, 1, 4], [5, 3, 4], 4242
START = [2, 0, 1]


def build_model(i, D, H, Ff, EL, DL, ctc_layer, seed):
    args, task, model, crit, V_src, V_tgt = MG.build("scorer%d" % i, D, H, Ff, EL, DL, ctc_layer, True)
    cfg = s2t_ref.default_cfg(D=D, heads=H, ffn=Ff, enc_layers=EL, dec_layers=DL, ctc_layer=ctc_layer)
    W = s2t_ref.make_weights(s2t_ref.param_shapes(cfg, V_src, V_tgt, criterion_fc=True), seed)
    MG.load_weights(model, crit, W)
    model.eval()
    blank = task.source_dictionary.index("<ctc_blank>")
    return task, model, np.array([D, H, Ff, EL, DL, ctc_layer, 1, V_src, V_tgt, blank, seed], np.int64)


def run_case(task, models, sample, start):
    s = dict(sample)
    if start is not None:
        s["start_indices"] = list(start)
    with torch.no_grad():
        hyps = SequenceScorer(task.target_dictionary).generate(models, s)
        # the condition on the inputs: every averaged target probability is far inside the normal range
        p = sum(torch.softmax(m(**s["net_input"])[0].float(), -1).gather(2, s["target"].unsqueeze(-1))[..., 0] for m in models) / len(models)
    assert float(p.min()) > MIN_PROB, "an averaged target probability of %g: choose other inputs" % float(p.min())
    B, L = s["target"].shape
    pos = np.full((B, L), np.nan, np.float32)
    tok = np.full((B, L), -1, np.int64)
    score, length = np.zeros((B,), np.float32), np.zeros((B,), np.int64)
    for b, hs in enumerate(hyps):
        assert len(hs) == 1 and hs[0]["attention"] is None and hs[0]["alignment"] is None
        n = int(hs[0]["tokens"].numel())
        assert tuple(hs[0]["positional_scores"].shape) == (n,)
        pos[b, :n], tok[b, :n], score[b], length[b] = hs[0]["positional_scores"].numpy(), hs[0]["tokens"].numpy(), float(hs[0]["score"]), n
    return {"pos": pos, "tokens": tok, "score": score, "len": length}


def cases():
    built = [build_model(i, *m) for i, m in enumerate(MODELS)]
    task = built[0][0]
    V_src, V_tgt, blank = int(built[0][2][7]), int(built[0][2][8]), int(built[0][2][9])
    assert all(int(b[2][8]) == V_tgt for b in built)
    s = MG.make_sample(SAMPLE_SEED, LENS, TGT_LENS, TR_LENS, V_src, V_tgt, blank)
    sample = MG.to_ref_sample(s)
    L = max(TGT_LENS)
    assert 1 in TGT_LENS and L in TGT_LENS and all(st + 1 <= n for st, n in zip(START, TGT_LENS))
    out = {"src_tokens": s["src_tokens"], "src_lengths": s["src_lengths"], "prev_output_tokens": s["prev_output_tokens"],
           "target": s["target"], "start_indices": np.array(START, np.int64), "meta_a": built[0][2], "meta_b": built[1][2]}
    models = [b[1] for b in built]
    for tag, ms, start in (("one", models[:1], None), ("ens", models, None), ("start", models, START)):
        for k, v in run_case(task, ms, sample, start).items():
            out["%s_%s" % (tag, k)] = v
    return out


if __name__ == "__main__":
    res = cases()
    path = os.path.join(MG.OUT, "scorer.npz")
    if "--check" in sys.argv:
        old = dict(np.load(path, allow_pickle=False))
        assert sorted(old) == sorted(res), (sorted(old), sorted(res))
        for k, v in res.items():
            if v.dtype.kind == "f":
                assert old[k].shape == v.shape and np.allclose(old[k], v, rtol=0, atol=1e-6, equal_nan=True), "scorer.npz is stale: " + k
            else:
                assert np.array_equal(old[k], v), "scorer.npz is stale: " + k
        print("scorer fixture up to date")
    else:
        np.savez_compressed(path, **res)
        print("wrote", path, {k: res[k].tolist() for k in ("one_score", "ens_score", "start_score", "start_len")})
