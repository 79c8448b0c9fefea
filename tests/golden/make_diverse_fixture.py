#!/usr/bin/env python3
"""Capture tests/golden/diverse.npz from the REAL reference (build container only; never at test time):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_diverse_fixture.py

Two kinds of data, both from fairseq/search.py DiverseBeamSearch (:103-161) on the CPU in float32:

* per-step: `n_step` random (lprobs, scores) inputs of ONE sentence -- step 0 (identical rows, as in a search) and later steps, G = 1, G = beam, peaked rows so that the
  groups collide on tokens, strength 0 -- with the (scores, tokens, beams) `DiverseBeamSearch.step` returns:
  s<i>_lprobs [beam, V], s<i>_scores [beam] (the cumulative scores of the step before; zeros at step 0), s<i>_par = [step, G, strength],
  s<i>_out_scores / _out_tokens / _out_beams [2 beam].
* whole searches: the reference's SequenceGenerator(search_strategy=DiverseBeamSearch(...)) on models built as make_golden.run_generate_case
  builds them: `dc` (case c's shape, beam 4, G 2, strength 0.5), `dd` (case d's shape, beam 6, G 3, strength 1.0, every score option set),
  `da` (case a's shape: 32-wide heads, which only the step-by-step route takes).  Keys as generate_wide.npz plus <tag>_div = [G, strength];
  the inputs are those of generate_wide.npz case c / d and generate.npz case a (same sample seed and lengths) and are not stored again.

Every search is also run with the model in float64: the tokens must agree with the float32 run, and in the float32 run the cut of every
group at every step -- the last candidate it takes against the first it leaves -- must exceed 1e-3, so that no test of the 1e-4 bound
hangs on a near-tie.  A case that fails takes the next weight seed (recorded in <tag>_meta).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and applies the shims listed there)

import torch  # noqa: E402
from fairseq import search  # noqa: E402
from fairseq.sequence_generator import SequenceGenerator  # noqa: E402

from oracle import s2t_ref  # noqa: E402

MIN_CUT = 1e-3


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


def step_cases():
    rs = np.random.RandomState(2024)
    #        beam G  V   strength step peaked
    plan = [(4, 2, 40, 0.5, 0, 1.0), (4, 2, 40, 0.5, 3, 6.0), (6, 3, 50, 1.0, 0, 6.0), (6, 3, 50, 1.0, 2, 6.0), (6, 1, 40, 0.5, 2, 1.0),
            (4, 4, 40, 2.0, 1, 6.0), (4, 4, 40, 2.0, 0, 6.0), (16, 8, 60, 8.0, 4, 6.0), (16, 2, 60, 0.5, 4, 6.0), (8, 4, 33, 0.0, 2, 6.0),
            (8, 2, 45, 3.0, 5, 1.0), (12, 3, 64, 0.25, 1, 6.0)]
    out = {"n_step": np.int64(len(plan))}
    for i, (beam, G, V, lam, step, conc) in enumerate(plan):
        base = rs.randn(V).astype(np.float32) * conc
        lp = torch.log_softmax(torch.from_numpy(base[None, :] + rs.randn(beam, V).astype(np.float32)), -1)
        lp[:, 1] = -float("inf")
        if step == 0:
            lp[1:] = lp[0]                                       # a search's first step: every slot holds the same <bos> hypothesis
        cum = (rs.randn(beam).astype(np.float32) - 3) if step else np.zeros(beam, np.float32)
        scores = torch.zeros(1, beam, max(step, 1))
        scores[0, :, step - 1] = torch.from_numpy(cum)
        s, t, b = search.DiverseBeamSearch(_Dict(V), G, lam).step(step, lp.clone()[None], scores if step else None)
        out.update({"s%d_lprobs" % i: lp.numpy(), "s%d_scores" % i: cum, "s%d_par" % i: np.array([step, G, lam], np.float64),
                    "s%d_out_scores" % i: s[0].numpy().astype(np.float32), "s%d_out_tokens" % i: t[0].numpy().astype(np.int64),
                    "s%d_out_beams" % i: b[0].numpy().astype(np.int64)})
    return out


CUTS = []


class _CutBeam(search.BeamSearch):
    """BeamSearch.step that also records the smallest finite gap between the last candidate taken and the first one left"""

    def step(self, step, lprobs, scores):
        out = super().step(step, lprobs, scores)
        bsz, beam, V = lprobs.shape
        flat = (lprobs[:, ::beam, :] if step == 0 else lprobs + scores[:, :, step - 1].unsqueeze(-1)).reshape(bsz, -1)
        k = out[0].shape[1]
        top = torch.topk(flat, k + 1)[0]
        a, b = top[:, k - 1], top[:, k]
        fin = torch.isfinite(a) & torch.isfinite(b)
        if bool(fin.any()):
            CUTS.append(float((a - b)[fin].min()))
        return out


def _search(m, g, G, lam, seed, dtype):
    crit = ("ctc_multi_loss", "--underlying-criterion", "label_smoothed_cross_entropy") if m["compress"] else \
           ("label_smoothed_cross_entropy", "--label-smoothing", "0.1")
    args, task, model, criterion, V_src, V_tgt = MG.build("div", m["D"], m["H"], m["Ff"], m["EL"], m["DL"], m["ctc_layer"], m["compress"],
                                                          criterion=crit)
    cfg = s2t_ref.default_cfg(D=m["D"], heads=m["H"], ffn=m["Ff"], enc_layers=m["EL"], dec_layers=m["DL"],
                              ctc_layer=m["ctc_layer"] if m["compress"] else 0)
    W = s2t_ref.make_weights(s2t_ref.param_shapes(cfg, V_src, V_tgt, criterion_fc=m["compress"]), seed)
    W["decoder.output_projection.weight"][2] *= 4.0          # as run_generate_case: <eos> competitive
    MG.load_weights(model, criterion, W)
    s = MG.make_sample(m["seed"] + 1, m["lens"], [4] * len(m["lens"]), [3] * len(m["lens"]), V_src, V_tgt, V_src - 1)
    sample = MG.to_ref_sample(s)
    model.eval()
    if dtype == torch.float64:
        model.double()
        sample["net_input"]["src_tokens"] = sample["net_input"]["src_tokens"].double()
    strat = search.DiverseBeamSearch(task.target_dictionary, G, lam)
    strat.beam = _CutBeam(task.target_dictionary)
    del CUTS[:]
    hyps = SequenceGenerator([model], task.target_dictionary, search_strategy=strat, **g).generate([model], sample)
    return hyps, s, V_src, V_tgt, (min(CUTS) if CUTS else float("inf"))


def search_cases():
    cases = [("dc", dict(D=256, H=4, Ff=256, EL=2, DL=2, ctc_layer=1, compress=True, seed=610, lens=[61, 50, 37]),
              dict(beam_size=4, max_len_a=0, max_len_b=12, min_len=1), 2, 0.5),
             ("dd", dict(D=256, H=4, Ff=384, EL=2, DL=2, ctc_layer=0, compress=False, seed=710, lens=[48, 48]),
              dict(beam_size=6, max_len_a=0.1, max_len_b=5, min_len=2, len_penalty=0.6, unk_penalty=0.5, temperature=1.5), 3, 1.0),
             ("da", dict(D=64, H=2, Ff=128, EL=3, DL=2, ctc_layer=2, compress=True, seed=600, lens=[61, 50, 37]),
              dict(beam_size=4, max_len_a=0, max_len_b=12, min_len=1), 2, 0.5)]
    out = {}
    for tag, m, g, G, lam in cases:
        for seed in range(m["seed"], m["seed"] + 20):
            hyps, s, V_src, V_tgt, cut = _search(m, g, G, lam, seed, torch.float32)
            hyps64 = _search(m, g, G, lam, seed, torch.float64)[0]
            same = all(len(a) == len(b) and all(x["tokens"].tolist() == y["tokens"].tolist() for x, y in zip(a, b)) for a, b in zip(hyps, hyps64))
            print("div", tag, "seed", seed, "cut %.3g" % cut, "float64 agrees" if same else "float64 DIFFERS")
            if same and cut > MIN_CUT:
                break
        else:
            raise SystemExit("no seed of case %s passes the float64 / cut checks" % tag)
        B, beam = len(hyps), g["beam_size"]
        Lmax = max(len(h["tokens"]) for hs in hyps for h in hs)
        tok = np.full((B, beam, Lmax), -1, np.int64); sc = np.full((B, beam), np.nan, np.float64)
        ps = np.zeros((B, beam, Lmax), np.float32); nh = np.zeros((B,), np.int64)
        for b, hs in enumerate(hyps):
            nh[b] = len(hs)
            for i, h in enumerate(hs):
                n = len(h["tokens"])
                tok[b, i, :n] = h["tokens"].numpy(); sc[b, i] = float(h["score"]); ps[b, i, :n] = h["positional_scores"].numpy()
        out.update({tag + "_tokens": tok, tag + "_scores": sc, tag + "_pos_scores": ps, tag + "_nhyp": nh,
                    tag + "_meta": np.array([m["D"], m["H"], m["Ff"], m["EL"], m["DL"], m["ctc_layer"], int(m["compress"]), V_src, V_tgt,
                                             V_src - 1, seed], np.int64),
                    tag + "_gen": np.array([g["beam_size"], g["max_len_a"], g["max_len_b"], g["min_len"], g.get("len_penalty", 1.0),
                                            g.get("unk_penalty", 0.0), g.get("temperature", 1.0)], np.float64),
                    tag + "_div": np.array([G, lam], np.float64)})
        print("div", tag, [[(len(h["tokens"]), round(float(h["score"]), 4)) for h in hs] for hs in hyps])
    return out


if __name__ == "__main__":
    out = step_cases()
    out.update(search_cases())
    np.savez_compressed(os.path.join(MG.OUT, "diverse.npz"), **out)
