"""The CTC loss beyond the limits of s2t_ctc_loss (transcripts of more than 511 units, vocabularies of more than 40,704 entries):
s2t_ctc_loss_any, reached through K.ctc_loss by shape or with route="any", against torch's float64 F.ctc_loss (the reference's call,
CTC_loss.py:143-151), and ctc_multi_loss end to end at such sizes against the oracle."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
K = None
CTC_MAX_VOCAB = 40704              # S2T_CTC_MAX_VOCAB: the largest vocabulary of the fixed-limit kernels


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K
    from fbk_fairseq_st_amd import kernels
    K = kernels
    K._lib()
    yield


def rel_err(a, b):
    a = a.detach().float().cpu().double(); b = b.detach().float().cpu().double()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def make_case(Lm, T, B, V, seed, dtype=torch.float32):
    """ragged frame counts, a long run of one unit, one empty and one infeasible transcript (the last utterance)"""
    assert B >= 3
    blank = V - 1
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(T, B, V, generator=g) * 2.0).to(dtype)
    tgt = torch.randint(0, blank, (B, Lm), generator=g)
    tgt[0, Lm // 4: Lm // 4 + Lm // 3] = 7                             # a run of equal units: a blank between every two
    tl = [Lm, 0] + [max(Lm - 37 * k, 1) for k in range(1, B - 2)] + [Lm]
    il = [T, T // 2] + [T - 5 * k for k in range(1, B - 2)] + [Lm // 2]  # the last: fewer frames than units -> infeasible
    return logits, tgt, torch.tensor(tl), torch.tensor(il), blank


def reference(logits, tgt, tl, il, blank):
    lp = torch.log_softmax(logits.double(), -1).requires_grad_(True)
    ref = torch.nn.functional.ctc_loss(lp, tgt, il, tl, blank=blank, reduction="sum", zero_infinity=True)
    ref.backward()
    gl = lp.grad - lp.detach().exp() * lp.grad.sum(-1, keepdim=True)   # d/dlogits from d/dlog-probs
    per = torch.nn.functional.ctc_loss(lp.detach(), tgt, il, tl, blank=blank, reduction="none", zero_infinity=False)
    return ref.detach(), gl, per


def on_dev(logits, tgt, tl, il):
    return logits.to(DEV), tgt.to(DEV), tl.to(DEV), il.to(torch.int32).to(DEV)


def check_against_float64(logits, tgt, tl, il, blank, dtype, route="auto"):
    ref, gl, per = reference(logits.float(), tgt, tl, il, blank)
    loss, grad, nll = K.ctc_loss(*on_dev(logits, tgt, tl, il), blank, route=route)
    lt, gt = (1e-5, 1e-4) if dtype == torch.float32 else (2e-3, 1e-2)
    T, V = logits.shape[0], logits.shape[2]
    if dtype == torch.float32 and (T > 1100 or V > CTC_MAX_VOCAB):
        # beyond the shapes the existing tests cover, f32 rounding of the recursion grows with the frame count and the emissions'
        # size (the values between two offsets reach four emissions, ~64 in log2 at V = 50,001: one ulp is 7.6e-6); measured on an
        # MI355X: 1.1e-4 at T = 4,200, 3.1e-4 at T = 6,150, 1.1e-4 at V = 50,001 / T = 1,200.  The loss stays within 1e-5.
        gt = 6e-4
    assert abs(float(loss) - float(ref)) < lt * abs(float(ref)), (float(loss), float(ref))
    assert rel_err(grad, gl) < gt, rel_err(grad, gl)
    ok = torch.isfinite(per)
    assert not bool(ok.all()) and not math.isfinite(float(nll[-1])) and math.isfinite(float(nll[1]))
    assert torch.allclose(nll.cpu()[ok].double(), per[ok], rtol=1e-5 if dtype == torch.float32 else 2e-3, atol=1e-4)
    assert float(grad[:, -1].float().abs().max()) == 0.0                      # infeasible: zero gradient
    for b in range(len(il)):                                                   # frames beyond the utterance: zero gradient
        assert float(grad[int(il[b]):, b].float().abs().sum()) == 0.0
    return loss, grad, nll


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lm,T,B", [(512, 1100, 3), (700, 1500, 4), (1023, 2150, 5), (2047, 4200, 4), (3000, 6150, 6)])
def test_ctc_loss_long_transcripts(Lm, T, B, dtype):
    V = 50
    logits, tgt, tl, il, blank = make_case(Lm, T, B, V, seed=Lm, dtype=dtype)
    check_against_float64(logits, tgt, tl, il, blank, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,Lm,T", [(40705, 60, 150), (65537, 100, 230), (50001, 800, 1200)])
def test_ctc_loss_large_vocabularies(V, Lm, T, dtype):
    logits, tgt, tl, il, blank = make_case(Lm, T, 3, V, seed=V, dtype=dtype)
    check_against_float64(logits, tgt, tl, il, blank, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ctc_loss_any_phases(dtype):
    """loss-only + gradient from the workspaces == one call, bit for bit; the upstream device scalar scales; lse from the arg-max pass"""
    logits, tgt, tl, il, blank = make_case(1200, 2500, 4, 50, seed=5, dtype=dtype)
    args = on_dev(logits, tgt, tl, il)
    loss, grad, nll = K.ctc_loss(*args, blank)
    loss2, ws, nll2 = K.ctc_loss(*args, blank, defer_grad=True)
    assert ws[-1] == "any"
    assert torch.equal(loss2, loss) and torch.equal(nll2, nll)
    g1 = K.ctc_loss_grad(ws, torch.ones(1, device=DEV))
    assert torch.equal(g1, grad)
    g2 = K.ctc_loss_grad(ws, torch.full((1,), 0.25, device=DEV))
    _, gl, _ = reference(logits.float(), tgt, tl, il, blank)
    assert rel_err(g2, 0.25 * gl) < (1e-4 if dtype == torch.float32 else 1e-2)
    _, _, lse = K.ctc_argmax(args[0], want_lse=True)
    loss3, grad3, nll3 = K.ctc_loss(*args, blank, lse=lse)
    assert abs(float(loss3) - float(loss)) <= 1e-6 * abs(float(loss)) and rel_err(grad3, grad) < 1e-6
    loss4, ws4, _ = K.ctc_loss(*args, blank, defer_grad=True, lse=lse)
    assert torch.equal(K.ctc_loss_grad(ws4, torch.ones(1, device=DEV)), grad3)


@pytest.mark.parametrize("Lm,T", [(20, 70), (40, 130), (100, 330), (200, 520), (400, 900), (511, 1100)])
def test_ctc_loss_any_route_where_the_fixed_route_applies(Lm, T):
    """the shapes of test_ctc_loss_transcript_lengths_of_every_lane_width on the forced new route: float64 at the same tolerance, and
    the old route within 1e-5"""
    B, V = 6, 50
    logits, tgt, tl, il, blank = make_case(Lm, T, B, V, seed=Lm)
    loss, grad, nll = check_against_float64(logits, tgt, tl, il, blank, torch.float32, route="any")
    loss0, grad0, nll0 = K.ctc_loss(*on_dev(logits, tgt, tl, il), blank)
    assert abs(float(loss) - float(loss0)) <= 1e-5 * abs(float(loss0))
    assert rel_err(grad, grad0) < 1e-5
    ok = torch.isfinite(nll0)
    assert torch.equal(ok, torch.isfinite(nll)) and torch.allclose(nll[ok], nll0[ok], rtol=1e-5)


def test_ctc_multi_loss_long_transcripts_large_vocabulary(monkeypatch):
    """ctc_multi_loss with --ctc-compress-out, a 45,000-unit source dictionary and transcripts of 600 / 300 units, against the oracle;
    then one Adam update of a trainer at the same sizes"""
    import test_configs_gpu as C
    from oracle import s2t_ref
    monkeypatch.setattr(C, "V_SRC", 45000)
    dtype = torch.float32
    a, task, model, crit, cfg, W = C.build("s2t_transformer_xs", dtype, ctc_layer=4)
    src = task.source_dictionary
    blank = src.index("<ctc_blank>")
    assert len(src) > K.CTC_MAX_VOCAB
    sample = C.batch(task, 2, 3600, 20, 600, seed=7)
    tr, trl = sample["transcript_target"], sample["transcript_target_lengths"]
    tr[1, 300:] = src.pad()
    tr[1, 299] = 2
    trl[1] = 300
    model.train(); crit.train()
    model.arena.zero_grad()
    loss, ss, log = crit(model, C.to_dev(sample))
    loss.backward()
    torch.cuda.synchronize()
    assert int(model.encoder._last["ctc_lengths_host"][0]) >= 900
    (oloss, oss, olog, _, _, _), ograds = C.oracle_grads(W, lambda Wg: s2t_ref.ctc_multi_loss(Wg, cfg, sample, 0.1, 1.0, blank, training=True))
    t = C.TOL[dtype]
    assert ss == oss
    assert C.rel(loss, oloss) <= t["loss"], (float(loss), float(oloss))
    assert C.rel(log["ctc_loss"], olog["ctc_loss"]) <= t["loss"]
    for k in ("ctc_total", "ctc_errors"):
        assert float(log[k]) == float(olog[k]), k
    C.compare_grads(C.engine_grads(model), ograds, t["grad"], t["cos"], what="s2t_transformer_xs ctc_any")

    from fbk_fairseq_st_amd.registry import apply_arch, namespace, setup_task
    from fbk_fairseq_st_amd.trainer import Trainer
    a = namespace(arch="s2t_transformer_xs", task="dummy_s2t", criterion="ctc_multi_loss", underlying_criterion="label_smoothed_cross_entropy",
                  label_smoothing=0.1, sentence_avg=False, ctc_compress_out=True, ctc_encoder_layer=4, ctc_weight=1.0,
                  input_feat_per_channel=80, no_attn_2d=True, dict_size=96, src_dict_size=45001, batch_size=2, frames=3600,
                  tgt_len=12, transcript_len=600, lr=[1e-3], adam_betas="(0.9, 0.98)", clip_norm=20.0, warmup_updates=1,
                  warmup_init_lr=1e-3, seed=3)
    apply_arch(a)
    task = setup_task(a)
    torch.manual_seed(0)
    model, crit = task.build_model(a), task.build_criterion(a)
    trainer = Trainer(a, task, model, crit, device="cuda:0", compute_dtype=dtype)
    trainer.train_step([trainer.prepare(task.dummy_batch(seed=1, lengths=[3600, 3400]))])
    st = trainer.reduce_stats()
    assert np.isfinite(st["loss"]) and np.isfinite(st["gnorm"]), st
