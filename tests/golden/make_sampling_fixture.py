#!/usr/bin/env python3
"""Capture tests/golden/sampling.npz from the REAL reference (build container only; never at test time):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sampling_fixture.py

fairseq/search.py Sampling.step (:164-278) on the CPU in float32, with torch.multinomial replaced by a recorder that keeps the
probabilities it is handed and returns FORCED positions (the reference's random stream is not part of what is reproduced; its kept sets,
its step-0 rule, its beams and its scores are).  `n_step` cases: step 0 and later steps; the plain, top-k and top-p modes; k = 1 and
k >= the number of finite columns; P so small that one column is kept and P >= the total mass; rows with -inf columns.  Per case i:

  s<i>_lprobs [B, beam, V] (after the score rules: -inf columns, not renormalised), s<i>_cum [B, beam] (the cumulative scores of the step
  before; zeros at step 0), s<i>_par = [step, sampling_topk, sampling_topp],
  s<i>_support bool [rows, V]: the columns multinomial may return for each row it is handed (rows = B at step 0, B * beam later), as
  token ids (positions mapped through the reference's own top-k / top-p index tensors),
  s<i>_pos [B, beam] the forced positions, s<i>_out_scores / _out_tokens / _out_beams [B, beam] what step() returned for them.

For a top-p case the generator asserts that P lies at least 1e-4 away from every cumulative mass of every row (float64), so that no
kept set hangs on a rounding.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and applies the shims listed there)

import torch  # noqa: E402
from fairseq import search  # noqa: E402

MIN_P_MARGIN = 1e-4


class _Dict:
    def __init__(self, V):
        self.V = V

    def pad(self):
        return 1

    def eos(self):
        return 2

    def unk(self):
        return 3

    def __len__(self):
        return self.V


class _Recorded(search.Sampling):
    """the reference class, keeping the index tensor of its top-p branch"""
    idx = None

    def _sample_topp(self, lprobs):
        p, idx = super()._sample_topp(lprobs)
        self.idx = idx.clone()
        return p, idx


def run_case(rs, B, beam, V, step, topk, topp, conc, n_inf):
    for attempt in range(50):                                    # (top-p: inputs are drawn again until P is clear of every cumulative mass)
        lp = torch.log_softmax(torch.from_numpy(rs.randn(B, beam, V).astype(np.float32) * conc), -1)
        lp[:, :, 1] = -float("inf")                              # pad, as the generator's score rules leave it
        for b in range(B):
            for j in range(beam):
                lp[b, j, torch.from_numpy(rs.choice(np.arange(4, V), n_inf, replace=False))] = -float("inf")
        if step == 0:
            lp[:, 1:] = lp[:, :1]                                # a search's first step: every slot holds the same <bos> hypothesis
        rows = lp[:, 0, :] if step == 0 else lp.reshape(B * beam, V)
        margin = min(np.abs(np.cumsum(np.sort(np.exp(r.astype(np.float64)))[::-1]) - topp).min() for r in rows.numpy())
        if topp <= 0 or margin >= MIN_P_MARGIN:
            break
    assert topp <= 0 or margin >= MIN_P_MARGIN, "P sits on a cumulative mass"
    cum = (rs.randn(B, beam).astype(np.float32) - 3) if step else np.zeros((B, beam), np.float32)
    scores = torch.zeros(B, beam, max(step, 1))
    scores[:, :, step - 1] = torch.from_numpy(cum)
    strat = _Recorded(_Dict(V), topk, topp)
    seen = {}
    real_multinomial, real_topk = torch.multinomial, torch.Tensor.topk

    def multinomial(probs, num, replacement=True):
        assert replacement and "probs" not in seen
        seen["probs"] = probs.clone()
        pos = torch.zeros(probs.shape[0], num, dtype=torch.int64)
        for r in range(probs.shape[0]):
            sup = torch.nonzero(probs[r] > 0).view(-1).numpy()
            pick = list(rs.choice(sup, num))
            if num >= 2:
                pick[0], pick[1] = sup[0], sup[-1]                   # the edges of the support
            elif r % 3 == 0:
                pick[0] = sup[-1]
            pos[r] = torch.from_numpy(np.array(pick))
        seen["pos"] = pos.clone()
        return pos

    def topk_rec(self, k, *a, **kw):
        out = real_topk(self, k, *a, **kw)
        seen["topk_idx"] = out[1].clone()
        return out
    torch.multinomial, torch.Tensor.topk = multinomial, topk_rec
    try:
        s, t, b = strat.step(step, lp.clone(), scores if step else None)
    finally:
        torch.multinomial, torch.Tensor.topk = real_multinomial, real_topk
    probs = seen["probs"]
    nrow = probs.shape[0]
    idx = strat.idx if topp > 0 else (seen["topk_idx"] if topk > 0 else None)
    support = np.zeros((nrow, V), bool)
    for r in range(nrow):
        cols = torch.nonzero(probs[r] > 0).view(-1)
        support[r, (idx.reshape(nrow, -1)[r][cols] if idx is not None else cols).numpy()] = True
    return {"lprobs": lp.numpy(), "cum": cum, "par": np.array([step, topk, topp], np.float64), "support": support,
            "pos": seen["pos"].view(B, beam).numpy(), "out_scores": s.numpy().astype(np.float32), "out_tokens": t.numpy().astype(np.int64),
            "out_beams": b.numpy().astype(np.int64)}


def cases():
    rs = np.random.RandomState(4711)
    #        B  beam V   step topk topp  conc n_inf
    plan = [(2, 3, 40, 0, -1, -1.0, 1.0, 4), (2, 3, 40, 3, -1, -1.0, 1.0, 4), (2, 4, 50, 0, 5, -1.0, 2.0, 6), (2, 4, 50, 2, 5, -1.0, 2.0, 6),
            (1, 5, 33, 1, 1, -1.0, 2.0, 3), (2, 3, 40, 0, 40, -1.0, 1.0, 8), (2, 3, 40, 2, 40, -1.0, 1.0, 8), (2, 4, 64, 0, -1, 0.5, 2.0, 5),
            (2, 4, 64, 3, -1, 0.8, 2.0, 5), (1, 4, 45, 2, -1, 1e-6, 1.0, 3), (2, 3, 40, 4, -1, 2.0, 1.0, 6), (2, 3, 48, 1, 7, 0.9, 1.0, 30),
            (1, 6, 60, 5, 3, -1.0, 6.0, 2), (2, 2, 36, 0, -1, 0.999, 3.0, 20)]
    out = {"n_step": np.int64(len(plan))}
    for i, c in enumerate(plan):
        for k, v in run_case(rs, *c).items():
            out["s%d_%s" % (i, k)] = v
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(MG.OUT, "sampling.npz"), **cases())
