"""A whole training step WITH dropout, HIP path against the CPU oracle given the engine's own masks.

Every other comparison of a step with the oracle runs at rate zero.  Here the rates are on, and the oracle (oracle/s2t_ref.py,
whose dropout sites are pinned to the real reference's F.dropout calls by tests/test_oracle_golden.py on fixture dropout.npz) is
handed the keep decisions the engine made, the way `relu_masks` hands it the ReLU active sets and `pred_override` the CTC arg-max:
what is left of the comparison is floating-point arithmetic.  The masks are NOT read out of the engine's buffers.  The engine's
FORWARD records, per site, (p, seed, shape of the index space) of the launch it made (engine.dropout_record); `site_mask` below
rebuilds each mask from that with s2t_dropout on a tensor of ones -- the one definition every fused epilogue is pinned to kernel by
kernel (test_routes_gpu.py, test_attention_modes_gpu.py, test_update_tail_gpu.py) -- and permutes it to the oracle's layout.  The
backward never sees the record: it re-derives every (p, seed) by hand (c["seed"] + k, the six-seed tuples of csrc/layer.hip), and
a wrong offset, a 1/(1-p) applied twice or not at all, a wrong alpha behind the ReLU record, a mask on the wrong side of the
embedding LayerNorm or a subsampler rate other than max(p, 0.1) all show as a gradient (or loss) off its bound.

Model (the tests/test_engine_gpu.py build): D 128, ffn 512, 2 heads of 64, 3 encoder + 2 decoder layers, CTC compression after
encoder layer 2, vocabularies 304 / 205 with a few boosted CTC biases (the batch really compresses), three ragged utterances of
600 / 455 / 333 frames (T4 = 150: in bf16 the second-generation attention, T4 >= 128; 12 decoder rows: the short-query kernels;
64 channels: the direct conv2 kernels with their fused masks), 12 target tokens.

  case  dtype / path                 act   dropout / attention / activation
  a     fp32, per-kernel             relu  0.2 / 0.1 / 0.15 (subsampler max(0.2, 0.1) = 0.2); ReLU decisions shared via relu_record
  b     fp32                         relu  0.05 / 0.1 / 0    subsampler must record 0.1; the activation sites record nothing
  c     fp32                         gelu  0.2 / 0.1 / 0.15  the separate K.dropout(da) of the GELU backward
  d     fp32, layernorm_embedding    relu  as a; both embedding masks sit behind their LayerNorm
  e     bf16, per-kernel schedule    relu  as a
  f     bf16, one call per layer     relu  as a; the record comes from layer_fwd's seed tuple

Bounds.  fp32 (a-d): the project's own, unchanged -- loss, ctc_loss, nll_loss 1e-4 relative; per-tensor gradient norm
FP32_NORTH_STAR = 1e-4 and cosine 0.9999 on every tensor compare_grads considers; arg-max path and compressed lengths equal to
the oracle's own.  A dropout site adds one exact multiplication per element, nothing that would widen them.  The oracle's own
f32 evaluation of this step (ReLU, masks of case a's shapes and rates, ReLU decisions shared) lies within 4.2e-7
(worst per-tensor gradient norm, encoder.convolutions.1.bias; worst cosine 1 - 2.6e-11) and 7.2e-8 (loss, ctc_loss, nll_loss) of its
float64 evaluation, measured once on the host: more than 200 times below 1e-4, so a miss of the bound is the engine's.
bf16 (e, f), free-running against the f32 oracle with `pred_override`: bounds = twice the worst MEASURED on an MI355X, rounded up to one digit
(tests/golden/parity_measured.json holds the figures, the 1.3x tripwire guards them):
                                   loss error   worst gradient-norm error            worst 1 - cosine
  e  per-kernel schedule           3.93e-4      1.415e-2 (encoder.bn.0.bias)         3.54e-3 (encoder.convolutions.0.weight)
  f  one call per layer            3.93e-4      1.411e-2 (encoder.bn.0.bias)         3.55e-3 (encoder.convolutions.0.weight)
  the same model, all rates zero   2.91e-4      1.427e-2 (encoder.convolutions.1.bias)  2.75e-3 (encoder.convolutions.0.weight)
  bound                            8e-4         3e-2                                 8e-3 (cosine >= 0.992)
Dropout adds nothing to the gradient-norm error of this model and about a third to the loss and direction errors; e and f give the
identical loss (asserted, as tests/test_engine_gpu.py does) and differ in the gradients by the order of f32 atomics only.

Conditions that keep a case from passing vacuously: every recorded site's kept fraction within 6 binomial standard deviations
of 1 - p; 3 + 4 enc_layers + 1 + 6 dec_layers sites when all rates are positive; the batch compresses; the loss differs from the
zero-rate loss of the same step by more than 1e-3 relative.

Negative control (case a, one engine step shared): for one site of each class -- subsampler, encoder input, self-attention
probabilities, block output, activation, decoder embedding, encoder-attention probabilities -- the site's mask is rebuilt from
seed + 1 and the oracle runs again: the comparison must then miss a bound, and the test names which (measured on the five
classes above the CTC tap or in the decoder: 105 .. 145 bounds missed each, worst loss-term error 9e-4 .. 4e-3, worst gradient-norm
error 4e-2 .. 2e-1; the engine's arg-max path is handed to these oracle runs, so that a mask swapped below the tap cannot change the
compressed lengths the other masks were drawn for).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import int_ref, s2t_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENGTHS = [600, 455, 333]
RATES_A = (0.2, 0.1, 0.15)
FP32_NORTH_STAR = 1e-4
TOL_F32 = dict(loss=1e-4, grad=FP32_NORTH_STAR, cos=0.9999)
TOL_BF16 = dict(loss=8e-4, grad=3e-2, cos=0.992)         # 2x the measured worst, rounded up to one digit (module docstring)


def to_dev(s):
    if torch.is_tensor(s):
        return s.to(DEV)
    if isinstance(s, dict):
        return {k: to_dev(v) for k, v in s.items()}
    if isinstance(s, (list, tuple)):
        return type(s)(to_dev(v) for v in s)
    return s


def build(dtype, act="relu", rates=RATES_A, lne=False, seed=31):
    """the tests/test_engine_gpu.py model with the oracle's deterministic weights (as tests/test_configs_gpu.build loads them)"""
    from fbk_fairseq_st_amd import conv_transformer, criterions, tasks  # noqa: F401
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.registry import apply_arch, namespace
    p, pa, pact = rates
    a = namespace(arch="conv_transformer", criterion="ctc_multi_loss", underlying_criterion="label_smoothed_cross_entropy", label_smoothing=0.1,
                  ctc_compress_out=True, ctc_encoder_layer=2, ctc_weight=1.0, encoder_embed_dim=128, encoder_ffn_embed_dim=512,
                  encoder_attention_heads=2, encoder_layers=3, decoder_layers=2, decoder_embed_dim=128, decoder_ffn_embed_dim=512,
                  decoder_attention_heads=2, no_attn_2d=True, input_feat_per_channel=80, dropout=p, attention_dropout=pa, activation_dropout=pact,
                  relu_dropout=pact, activation_fn=act, sentence_avg=False, layernorm_embedding=lne, seed=7)
    apply_arch(a)
    tgt, src = Dictionary.synthetic(300), Dictionary.synthetic(200)
    src.add_symbol("<ctc_blank>")
    task = tasks.SpeechTranslationCTCTask(a, tgt, src)
    model, crit = task.build_model(a), task.build_criterion(a)
    cfg = s2t_ref.default_cfg(D=128, heads=2, ffn=512, enc_layers=3, dec_layers=2, ctc_layer=2, conv_ch=64, act=act, layernorm_embedding=lne)
    W = s2t_ref.make_weights(s2t_ref.param_shapes(cfg, len(src), len(tgt), criterion_fc=True), seed)
    blank = src.index("<ctc_blank>")
    W["encoder.ctc_fc.bias"][[7, 19, 123, 180, blank]] += 6.0          # runs of equal arg-max: the compression really shortens
    model.load_state_dict({k: v for k, v in W.items() if not k.startswith("criterion.")})
    with torch.no_grad():
        crit.ctc_aware_model.fc_out.weight.copy_(W["criterion.ctc_aware_model.fc_out.weight"])
        crit.ctc_aware_model.fc_out.bias.copy_(W["criterion.ctc_aware_model.fc_out.bias"])
    assert model.hp.sub_dropout is None                                 # the subsampler's rate stays max(dropout, 0.1)
    hp = model.hp
    assert (hp.dropout, hp.attention_dropout, hp.activation_dropout) == rates, (hp.dropout, hp.attention_dropout, hp.activation_dropout)
    model.materialize(DEV, dtype, extra=crit.arena_params())
    model._ensure_engine(DEV)
    return task, model, crit, cfg, W, blank


def make_sample(task, blank):
    from fbk_fairseq_st_amd.data import synthetic_batch
    return synthetic_batch(len(LENGTHS), max(LENGTHS), 12, 10, len(task.target_dictionary), blank, seed=5, lengths=LENGTHS)


def oracle_grads(W, run):
    Wg = {k: v.clone().requires_grad_(v.dtype.is_floating_point and "running" not in k) for k, v in W.items()}
    out = run(Wg)
    out[0].backward()
    return out, {k: v.grad for k, v in Wg.items() if v.grad is not None}


def engine_grads(model):
    from fbk_fairseq_st_amd.conv_transformer import fused_to_reference
    return fused_to_reference({n: model.arena.g(n).detach().float().cpu().clone() for n in model.arena.slices})


def rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-12)


def compare_grads(mine, ref, tol, cos_min, what=""):
    """tests/test_configs_gpu.compare_grads, collecting instead of asserting: per-tensor gradient norms, relative (tensors whose
    exact gradient is zero -- the key bias of an attention -- against the tolerance times their weight gradient's norm, plus a
    floor of 1e-6 of the largest norm), and the cosine of every tensor whose norm is above 1e-3 of the largest.
    Returns (violations, worst norm error, worst cosine)."""
    bad = []
    worst, wcos = (0.0, None), (1.0, None)
    floor = 1e-6 * max(float(g.norm()) for g in ref.values())
    big = 1e-3 * max(float(g.norm()) for g in ref.values())
    for k, g in ref.items():
        if k.endswith("_float_tensor"):
            continue
        assert k in mine, k
        a, b = float(mine[k].norm()), float(g.norm())
        if k.endswith("k_proj.bias"):
            wn = float(ref[k[:-4] + "weight"].norm())
            if not a <= tol * wn + floor:
                bad.append("%s gradient norm of %s: %.6g above %.1e of its weight gradient's %.6g" % (what, k, a, tol, wn))
            continue
        err = abs(a - b) / max(b, floor)
        if err > worst[0]:
            worst = (err, k)
        if not err <= tol:
            bad.append("%s gradient norm of %s: %.6g vs oracle %.6g (rel %.3e > %.1e)" % (what, k, a, b, err, tol))
        if b < big:
            continue
        c = float(torch.nn.functional.cosine_similarity(mine[k].reshape(1, -1).double(), g.reshape(1, -1).double()))
        if c < wcos[0]:
            wcos = (c, k)
        if not c >= cos_min:
            bad.append("%s gradient direction of %s: cosine %.6f < %.6f" % (what, k, c, cos_min))
    return bad, worst, wcos


# ---- tripwire (tests/test_configs_gpu.tripwire): the bf16 bounds are ~2x the measured worst case; a bf16 figure more than 1.3x (plus a
# floor for run-to-run noise) above what the committed build measured (tests/golden/parity_measured.json) fails.
_MEASURED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parity_measured.json")
_MEASURED = json.load(open(_MEASURED_PATH)) if os.path.exists(_MEASURED_PATH) else {}
_FLOOR = dict(grad=2e-3, one_minus_cos=1e-3, loss=3e-4, flips=0.005, gen=1e-2)


def tripwire(what, **figures):
    if "bfloat16" not in what and "bf16" not in what:
        return
    case = os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" ")[0]
    key = "%s | %s" % (case, what)
    out = os.environ.get("S2T_WRITE_MEASURED")
    if out:
        rec = json.load(open(out)) if os.path.exists(out) else {}
        rec.setdefault(key, {}).update({k: float(v) for k, v in figures.items()})
        json.dump(rec, open(out, "w"), indent=1, sort_keys=True)
        return
    base = _MEASURED.get(key)
    if base is None:
        return
    for k, v in figures.items():
        if k in base:
            assert float(v) <= 1.3 * base[k] + _FLOOR[k], "%s: %s %.3e against %.3e measured by the committed build (tripwire 1.3x)" % (key, k, v, base[k])


# ---- the engine's record -> the oracle's masks
def site_mask(site, p, seed, shape):
    """keep mask of one recorded site in the oracle's layout: s2t_dropout's decisions on the index space the launch hashed"""
    from fbk_fairseq_st_amd import kernels as K
    if site.endswith(".probs"):
        B, H, Tq, Tk = shape
        Tk4 = (Tk + 3) & ~3                                             # drop_index's row pitch (tests/test_attention_modes_gpu.py)
        return (K.dropout(torch.ones(B, H, Tq, Tk4, dtype=torch.float32, device=DEV), p, seed) != 0)[..., :Tk].cpu()
    keep = K.dropout(torch.ones(shape, dtype=torch.float32, device=DEV), p, seed) != 0
    if site == "encoder.conv0.drop":
        keep = keep.permute(0, 3, 1, 2)                                 # (B,T2,F2,C) -> (B,C,T2,F2), as relu_record
    elif site == "encoder.conv1.drop":
        keep = keep.permute(1, 3, 0, 2)                                 # (T4,B,F4,C) -> (B,C,T4,F4)
    elif site.endswith("embed.drop") and not site.startswith("encoder."):
        keep = keep.permute(1, 0, 2)                                    # (L,B,D) -> (B,L,D)
    return keep.contiguous().cpu()


def masks_of(record, reseed=None):
    return {s: (site_mask(s, p, seed + (1 if s == reseed else 0), shape), p) for s, (p, seed, shape) in record.items()}


def expected_rate(site, rates):
    p, pa, pact = rates
    return pa if site.endswith(".probs") else pact if site.endswith("ffn.act") else max(p, 0.1) if ".conv" in site else p


def check_record(record, masks, cfg, rates):
    """the conditions: which sites recorded, at which rate, and that each mask is a mask of that rate"""
    sites = s2t_ref.drop_sites(cfg)
    want = [s for s in sites if expected_rate(s, rates) > 0]
    assert sorted(record) == sorted(want), (sorted(set(want) - set(record)), sorted(set(record) - set(want)))
    if min(rates) > 0:
        assert len(record) == 3 + 4 * cfg["enc_layers"] + 1 + 6 * cfg["dec_layers"]
    assert len({seed for _, seed, _ in record.values()}) == len(record), "two sites share a seed"
    for s, (p, seed, shape) in record.items():
        assert p == expected_rate(s, rates), (s, p, expected_rate(s, rates))
        keep = masks[s][0]
        n = keep.numel()
        frac = float(keep.float().mean())
        assert abs(frac - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / n) + 2.0 ** -16, "%s: kept %.5f of %d, p = %g" % (s, frac, n, p)


# ---- one engine step and its oracle run
def engine_step(model, crit, sample, composite, seed=11, want_relu=False):
    eng = model.engine
    eng.composite = composite
    eng.dropout_record = {}
    eng.relu_record = {} if want_relu else None
    model.train(); crit.train()
    model.set_seed(seed)
    model.arena.zero_grad()
    loss, ss, log = crit(model, to_dev(sample))
    loss.backward()
    torch.cuda.synchronize()
    record, relu = eng.dropout_record, eng.relu_record
    eng.dropout_record = eng.relu_record = None
    last = model.encoder._last
    x_ctc = last["ctc_out"].detach().float().cpu()
    pred_ref = int_ref.argmax_first_np(torch.softmax(x_ctc, dim=-1).transpose(0, 1).contiguous().numpy())
    pred = last["pred"].detach().cpu().numpy()
    len4 = np.asarray(last["ctc_lengths_host"])
    assert all(np.array_equal(pred[b, :len4[b]], pred_ref[b, :len4[b]]) for b in range(len(len4))), "arg-max over the engine's own logits"
    runs = int_ref.ctc_rle_np(pred_ref, len4)
    assert [len(r) for r in runs] == [int(v) for v in last["lengths_host"]], "new lengths after the run-length collapse"
    assert min(len(r) for r in runs) < int(len4.max()), "the case must actually compress"
    return dict(loss=float(loss), ss=ss, log={k: float(v) for k, v in log.items()}, grads=engine_grads(model), record=record,
                relu=None if relu is None else {k: v.cpu() for k, v in relu.items()}, pred=pred, pred_ref=pred_ref, len4=len4,
                new_lengths=[int(v) for v in last["lengths_host"]])


def oracle_step(W, cfg, sample, blank, masks, relu=None, pred_override=None):
    cfg_m = dict(cfg, drop_masks=masks)
    if relu is not None:
        cfg_m["relu_masks"] = relu
    (oloss, oss, olog, enc, _, _), ograds = oracle_grads(W, lambda Wg: s2t_ref.ctc_multi_loss(Wg, cfg_m, sample, 0.1, 1.0, blank, training=True,
                                                                                           pred_override=pred_override))
    return dict(loss=float(oloss), ss=oss, log=olog, enc=enc, grads=ograds)


def violations(e, o, tol, what):
    """every bound the engine step `e` misses against the oracle step `o`; also (worst loss error, worst norm error, worst cosine)"""
    bad = []
    lerr = 0.0
    for k, a, b in (("loss", e["loss"], o["loss"]), ("ctc_loss", e["log"]["ctc_loss"], o["log"]["ctc_loss"]),
                    ("nll_loss", e["log"]["nll_loss"], o["log"]["nll_loss"])):
        r = rel(a, b)
        lerr = max(lerr, r)
        if not r <= tol["loss"]:
            bad.append("%s %s: %.6f vs oracle %.6f (rel %.3e > %.1e)" % (what, k, a, b, r, tol["loss"]))
    gbad, worst, wcos = compare_grads(e["grads"], o["grads"], tol["grad"], tol["cos"], what)
    print("MEASURED %s: loss error %.3e, worst gradient-norm error %.3e (%s), worst cosine %.6f = 1 - %.3e (%s)" %
          (what, lerr, worst[0], worst[1], wcos[0], 1.0 - wcos[0], wcos[1]))
    return bad + gbad, (lerr, worst[0], wcos[0])


def zero_rate_loss(W, cfg, sample, blank, pred_override=None):
    with torch.no_grad():
        return float(s2t_ref.ctc_multi_loss(W, cfg, sample, 0.1, 1.0, blank, training=True, pred_override=pred_override)[0])


def fp32_case(act="relu", rates=RATES_A, lne=False):
    task, model, crit, cfg, W, blank = build(torch.float32, act, rates, lne)
    sample = make_sample(task, blank)
    e = engine_step(model, crit, sample, composite=False, want_relu=(act == "relu"))
    del model, crit
    masks = masks_of(e["record"])
    check_record(e["record"], masks, cfg, rates)
    if act == "relu":
        assert len(e["relu"]) == 3 + cfg["enc_layers"] + cfg["dec_layers"], sorted(e["relu"])
        for s, (keep, p) in masks.items():
            if s.endswith("ffn.act"):                                   # a > 0 means active AND kept: the ReLU record lies inside the keep mask
                assert not bool((e["relu"][s[:-4]] & ~keep.view_as(e["relu"][s[:-4]])).any()), s
    return dict(e=e, masks=masks, cfg=cfg, W=W, blank=blank, sample=sample, rates=rates, act=act)


def check_fp32(c):
    e = c["e"]
    o = oracle_step(c["W"], c["cfg"], c["sample"], c["blank"], c["masks"], relu=e["relu"])
    enc = o["enc"]
    opred, len4 = enc.ctc_pred.numpy(), e["len4"]
    assert all(np.array_equal(e["pred"][b, :len4[b]], opred[b, :len4[b]]) for b in range(len(len4))), "fp32: arg-max differs from the oracle's own forward"
    assert [int(v) for v in enc.new_lengths] == e["new_lengths"]
    assert min(e["new_lengths"]) < int(len4.max())
    assert e["ss"] == o["ss"]
    for k in ("ntokens", "nsentences", "sample_size", "nframes", "ctc_total", "ctc_errors"):
        assert float(e["log"][k]) == float(o["log"][k]), k
    bad, _ = violations(e, o, TOL_F32, "dropout fp32 %s %s" % (c["act"], c["rates"]))
    assert not bad, "\n".join(bad)
    zl = zero_rate_loss(c["W"], c["cfg"], c["sample"], c["blank"])
    assert rel(e["loss"], zl) > 1e-3, ("the masks do not move the loss", e["loss"], zl)


@pytest.fixture(scope="module")
def case_a():
    return fp32_case()


def test_fp32_relu_step_with_the_engines_masks(case_a):
    """case a"""
    check_fp32(case_a)


def test_fp32_low_rates_subsampler_floor_and_a_site_at_rate_zero():
    """case b: dropout 0.05 -> the subsampler's masks are drawn at max(0.05, 0.1) = 0.1; activation rate 0 -> those sites record nothing"""
    c = fp32_case(rates=(0.05, 0.1, 0.0))
    rec = c["e"]["record"]
    assert rec["encoder.conv0.drop"][0] == 0.1 and rec["encoder.conv1.drop"][0] == 0.1 and rec["encoder.embed.drop"][0] == 0.05
    assert not [s for s in rec if s.endswith("ffn.act")] and len(rec) == 3 + 3 * 3 + 1 + 5 * 2
    check_fp32(c)


def test_fp32_gelu_step_with_the_engines_masks():
    """case c: the GELU backward's own K.dropout(da, pact, seed + 3); no discrete decision in the comparison"""
    check_fp32(fp32_case(act="gelu"))


def test_fp32_layernorm_embedding_masks_behind_the_layernorm():
    """case d"""
    check_fp32(fp32_case(lne=True))


NEGATIVE_SITES = {"subsampler": "encoder.conv1.drop", "encoder_input": "encoder.embed.drop",
                  "self_attention_probabilities": "encoder.layers.1.self_attn.probs", "block_output": "encoder.layers.2.ffn.out",
                  "activation": "decoder.layers.0.ffn.act", "decoder_embedding": "decoder.embed.drop",
                  "encoder_attention_probabilities": "decoder.layers.1.encoder_attn.probs"}


@pytest.mark.parametrize("cls", sorted(NEGATIVE_SITES))
def test_negative_control_a_mask_from_another_seed_misses_the_bounds(case_a, cls):
    """case a's engine step against the oracle with ONE site's mask rebuilt from seed + 1: if that can pass, the test cannot see
    that site's seed"""
    c, site = case_a, NEGATIVE_SITES[cls]
    assert site in c["e"]["record"]
    masks = dict(c["masks"])
    p, seed, shape = c["e"]["record"][site]
    masks[site] = (site_mask(site, p, seed + 1, shape), p)
    assert not torch.equal(masks[site][0], c["masks"][site][0])
    # (the engine's arg-max path is handed over too: a mask swapped below the CTC tap may move the oracle's own compressed lengths,
    # and the masks above the compression have the engine's shapes)
    o = oracle_step(c["W"], c["cfg"], c["sample"], c["blank"], masks, relu=c["e"]["relu"], pred_override=c["e"]["pred_ref"])
    bad, _ = violations(c["e"], o, TOL_F32, "negative control %s" % site)
    print("negative control %s: %d bounds missed, first: %s" % (site, len(bad), bad[:3]))
    assert bad, "a mask of seed + 1 at %s passes every bound: the comparison does not see that site's seed" % site


# ---- bf16: the per-kernel schedule (e) and the one-call-per-layer path (f), one model, one oracle run
@pytest.fixture(scope="module")
def bf16_steps():
    task, model, crit, cfg, W, blank = build(torch.bfloat16)
    assert model.engine.composite, "D 128 / ffn 512 / 2 heads must be a shape csrc/layer.hip takes"
    sample = make_sample(task, blank)
    e = engine_step(model, crit, sample, composite=False)
    f = engine_step(model, crit, sample, composite=True)
    del model, crit
    masks = masks_of(f["record"])
    o = oracle_step(W, cfg, sample, blank, masks, pred_override=f["pred_ref"])
    zl = zero_rate_loss(W, cfg, sample, blank, pred_override=f["pred_ref"])
    return dict(per_kernel=e, layer_calls=f, masks=masks, o=o, cfg=cfg, zero=zl)


@pytest.mark.parametrize("path", ["per_kernel", "layer_calls"])
def test_bf16_step_with_the_engines_masks(bf16_steps, path):
    """cases e and f"""
    s = bf16_steps
    e, o = s[path], s["o"]
    # both paths record the same (p, seed, shape) per site -- layer_fwd from its seed tuple, the blocks from their own arithmetic --
    # and make the same decisions, so the one oracle run (masks of the layer calls' record) serves both
    assert e["record"] == s["layer_calls"]["record"]
    assert np.array_equal(e["pred_ref"], s["layer_calls"]["pred_ref"]) and e["new_lengths"] == s["layer_calls"]["new_lengths"]
    assert s["per_kernel"]["loss"] == s["layer_calls"]["loss"], "the two schedules must give the identical loss"
    check_record(e["record"], s["masks"], s["cfg"], RATES_A)
    assert e["ss"] == o["ss"]
    for k in ("ntokens", "nsentences", "sample_size", "nframes", "ctc_total"):
        assert float(e["log"][k]) == float(o["log"][k]), k
    bad, (lerr, gerr, cos) = violations(e, o, TOL_BF16, "dropout bf16 %s" % path)
    tripwire("dropout bf16", loss=lerr, grad=gerr, one_minus_cos=1.0 - cos)
    assert not bad, "\n".join(bad)
    assert rel(e["loss"], s["zero"]) > 1e-3, ("the masks do not move the loss", e["loss"], s["zero"])
