#!/usr/bin/env python3
"""Capture tests/golden/dropout.npz from the REAL reference (build container only; never at test time):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dropout_fixture.py

One train-mode ctc_multi_loss update of a model_a-sized conv_transformer WITH dropout -- rates all non-zero and all different
(dropout 0.2, attention 0.1, relu / activation 0.15; the subsampler's own rate is max(dropout, 0.1) = 0.2) -- once plain (case
`relu`) and once with layernorm_embedding (case `lne`: the masks of both embeddings move behind their LayerNorm).  What is pinned
is WHERE every mask sits, not the reference's random stream: F.dropout is replaced (from outside the tree) by a recorder that
draws each call's keep mask from a seeded torch.Generator, applies x * keep / (1 - p) and appends (shape, p, keep) in call order.
torch's fused scaled_dot_product_attention draws its dropout in C++ where no patch reaches, so the glue below also replaces it by
the same arithmetic written out (softmax(q k^T / sqrt(d) + mask), F.dropout on the probabilities, times v): the attention sites of
the layers that return no weights are recorded like every other.

Per case <c> the file holds the inputs (as make_golden.py stores them), <c>_n_calls, <c>_mask_bits (np.packbits of all keep masks,
concatenated in call order), <c>_mask_shapes [n, 4] (trailing zeros = fewer dimensions), <c>_mask_p [n], the loss, sample size and
logged scalars, every gradient norm and the full gradients make_golden.py keeps.  tests/test_oracle_golden.py maps call order to the
oracle's site names (oracle.s2t_ref.drop_sites) and asserts that the two counts agree.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the reference on sys.path and applies the shims listed there)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle import s2t_ref  # noqa: E402

RATES = dict(dropout=0.2, attention_dropout=0.1, relu_dropout=0.15, activation_dropout=0.15)
D, H, FF, EL, DL, CTC_LAYER, SEED = 64, 2, 128, 3, 2, 2, 100            # model_a of make_golden.py
LENS, TGT_LENS, TR_LENS = [61, 50, 37], [7, 5, 6], [6, 4, 5]


class Recorder:
    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.calls = []

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return x
        keep = torch.rand(x.shape, generator=self.gen) >= p
        self.calls.append((tuple(x.shape), float(p), keep.numpy().copy()))
        return x * keep.to(x.dtype) / (1.0 - p)


def sdpa(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False, scale=None, **kw):
    """scaled_dot_product_attention written out, so that its dropout goes through F.dropout (the recorder)"""
    assert not is_causal and not kw
    s = torch.matmul(q, k.transpose(-2, -1)) * (1.0 / math.sqrt(q.shape[-1]) if scale is None else scale)
    if attn_mask is not None:
        s = s.masked_fill(~attn_mask, float("-inf")) if attn_mask.dtype == torch.bool else s + attn_mask
    p = torch.softmax(s, dim=-1)
    if dropout_p > 0.0:
        p = F.dropout(p, p=dropout_p)
    return torch.matmul(p, v)


def run_case(tag, lne, gen_seed):
    args, task, model, crit, V_src, V_tgt = MG.build("dropout_" + tag, D, H, FF, EL, DL, CTC_LAYER, True,
                                                     set_args=dict(RATES, layernorm_embedding=lne))
    assert (model.encoder.layernorm_embedding is not None) == lne
    blank = task.source_dictionary.index("<ctc_blank>")
    cfg = s2t_ref.default_cfg(D=D, heads=H, ffn=FF, enc_layers=EL, dec_layers=DL, ctc_layer=CTC_LAYER, layernorm_embedding=lne)
    W = s2t_ref.make_weights(s2t_ref.param_shapes(cfg, V_src, V_tgt, criterion_fc=True), SEED)
    MG.load_weights(model, crit, W)
    s = MG.make_sample(SEED + 1, LENS, TGT_LENS, TR_LENS, V_src, V_tgt, blank)
    sample = MG.to_ref_sample(s)
    out = {("in_" + k): v for k, v in s.items() if isinstance(v, np.ndarray)}
    out["in_ntokens"] = np.int64(s["ntokens"])
    out["meta"] = np.array([D, H, FF, EL, DL, CTC_LAYER, 1, V_src, V_tgt, blank, SEED], np.int64)
    out["rates"] = np.array([RATES["dropout"], RATES["attention_dropout"], RATES["activation_dropout"]], np.float64)
    rec = Recorder(gen_seed)
    saved = (F.dropout, F.scaled_dot_product_attention)
    F.dropout, F.scaled_dot_product_attention = rec.dropout, sdpa
    try:
        model.train(); crit.train()
        model.zero_grad(); crit.zero_grad()
        loss, sample_size, log = crit(model, sample)
        loss.backward()
    finally:
        F.dropout, F.scaled_dot_product_attention = saved
    out["n_calls"] = np.int64(len(rec.calls))
    out["mask_shapes"] = np.array([list(shp) + [0] * (4 - len(shp)) for shp, _, _ in rec.calls], np.int64)
    out["mask_p"] = np.array([p for _, p, _ in rec.calls], np.float64)
    out["mask_bits"] = np.packbits(np.concatenate([k.reshape(-1) for _, _, k in rec.calls]))
    out["train_loss"] = np.float64(loss.item())
    out["train_sample_size"] = np.int64(sample_size)
    for k, v in log.items():
        out["train_log_" + k] = np.float64(float(v))
    gn = {}
    for k, p in list(model.named_parameters()) + [("criterion." + k, p) for k, p in crit.named_parameters()]:
        g = p.grad if p.grad is not None else torch.zeros_like(p)
        gn[k] = float(g.norm())
        if k in MG.GRAD_KEYS:
            out["grad_" + k] = g.numpy().copy()
    out["gradnorm_keys"] = np.array(sorted(gn))
    out["gradnorm_vals"] = np.array([gn[k] for k in sorted(gn)], np.float64)
    print(tag, "loss", loss.item(), "calls", len(rec.calls), "kept", float(np.unpackbits(out["mask_bits"]).mean()))
    return {"%s_%s" % (tag, k): v for k, v in out.items()}


if __name__ == "__main__":
    out = run_case("relu", False, 20250)
    out.update(run_case("lne", True, 20251))
    path = os.path.join(MG.OUT, "dropout.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
