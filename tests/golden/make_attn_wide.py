#!/usr/bin/env python3
"""Capture tests/golden/attn_wide.npz from the REAL reference (build container only; never at test time):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_attn_wide.py

fairseq's SequenceGenerator (fairseq/sequence_generator.py:198-600) on the CPU in float32 over the configuration of generate_wide.npz
case `c` (64-wide heads, D 256, CTC compression after layer 1, three ragged sentences, beam 5; same weight seed, same sample seed and
lengths: the inputs are those of generate_wide.npz and are not stored again) built WITH `layernorm_embedding`, and with min_len 5 (with
the fixture's own min_len 1 this model ends every hypothesis after one token: nothing for an attention matrix to show).  The reference records the
last decoder layer's head-averaged encoder attention of every step (:286-292) and hands every hypothesis its `attention`, src_len x
tgt_len (:510-560).  Kept per sentence for the TWO best hypotheses:

  tokens [B, 2, Lmax] (-1 beyond the length), scores [B, 2], attention [B, 2, Ts, Lmax] (0 beyond a hypothesis' length; Ts = the
  batch's encoder length after compression), src_len [B] = Ts, enc_lengths [B] the encoder's own valid lengths, meta / gen as
  generate_wide.npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and applies the shims listed there)

import torch  # noqa: E402
from fairseq.sequence_generator import SequenceGenerator  # noqa: E402
from oracle import s2t_ref  # noqa: E402

KEEP = 2


def main():
    m = dict(D=256, H=4, Ff=256, EL=2, DL=2, ctc_layer=1, compress=True, seed=610, lens=[61, 50, 37])
    g = dict(beam_size=5, max_len_a=0, max_len_b=12, min_len=5)
    crit = ("ctc_multi_loss", "--underlying-criterion", "label_smoothed_cross_entropy")
    args, task, model, criterion, V_src, V_tgt = MG.build("attnwide", m["D"], m["H"], m["Ff"], m["EL"], m["DL"], m["ctc_layer"], True,
                                                          criterion=crit, set_args=dict(layernorm_embedding=True))
    assert model.decoder.layernorm_embedding is not None
    cfg = s2t_ref.default_cfg(D=m["D"], heads=m["H"], ffn=m["Ff"], enc_layers=m["EL"], dec_layers=m["DL"], ctc_layer=m["ctc_layer"],
                              layernorm_embedding=True)
    W = s2t_ref.make_weights(s2t_ref.param_shapes(cfg, V_src, V_tgt, criterion_fc=True), m["seed"])
    W["decoder.output_projection.weight"][2] *= 4.0          # as make_golden.run_generate_case
    MG.load_weights(model, criterion, W)
    s = MG.make_sample(m["seed"] + 1, m["lens"], [4] * 3, [3] * 3, V_src, V_tgt, V_src - 1)
    sample = MG.to_ref_sample(s)
    model.eval()
    with torch.no_grad():
        eo = model.encoder(sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
    hyps = SequenceGenerator([model], task.target_dictionary, **g).generate([model], sample)
    B = len(hyps)
    Lmax = max(len(h["tokens"]) for hs in hyps for h in hs[:KEEP])
    Ts = int(hyps[0][0]["attention"].shape[0])
    tok = np.full((B, KEEP, Lmax), -1, np.int64)
    sc = np.zeros((B, KEEP), np.float64)
    att = np.zeros((B, KEEP, Ts, Lmax), np.float32)
    for b, hs in enumerate(hyps):
        assert len(hs) >= KEEP
        for i, h in enumerate(hs[:KEEP]):
            n = len(h["tokens"])
            assert tuple(h["attention"].shape) == (Ts, n)
            tok[b, i, :n] = h["tokens"].numpy(); sc[b, i] = float(h["score"]); att[b, i, :, :n] = h["attention"].numpy()
    out = dict(tokens=tok, scores=sc, attention=att, src_len=np.full((B,), Ts, np.int64),
               enc_lengths=np.asarray([int(v) for v in eo.src_lengths], np.int64), src_lengths=s["src_lengths"],
               meta=np.array([m["D"], m["H"], m["Ff"], m["EL"], m["DL"], m["ctc_layer"], 1, V_src, V_tgt, V_src - 1, m["seed"]], np.int64),
               gen=np.array([g["beam_size"], g["max_len_a"], g["max_len_b"], g["min_len"], 1.0, 0.0, 1.0], np.float64))
    np.savez_compressed(os.path.join(MG.OUT, "attn_wide.npz"), **out)
    print("attn_wide", Ts, out["enc_lengths"].tolist(), [[(int((t >= 0).sum()), round(float(v), 4)) for t, v in zip(tb, sb)] for tb, sb in zip(tok, sc)])


if __name__ == "__main__":
    main()
