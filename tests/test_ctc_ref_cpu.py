"""tests/ctc_ref.py and the element bound of tests/test_ctc_loss_elements_gpu.py, checked without a GPU.

  * the reference agrees with torch's float64 F.ctc_loss (the reference implementation's call) to 1e-9;
  * the bound is achievable: the same recursion run in float32 stays inside it against its float64 run;
  * the bound is sharp enough: five deliberately wrong references, each one plausible kernel bug, violate it, even with the wider
    output-rounding term of bf16.
"""
import math

import numpy as np
import pytest
import torch

import ctc_ref as R

U32 = 2.0 ** -24                 # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)


def make_case(T, B, V, Lmax, scale, blank, seed):
    """ragged frame counts; utterance 0 the full width, utterance 1 with every third unit repeated, one empty transcript and (B >= 4)
    one that cannot fit its frames"""
    g = np.random.default_rng(seed)
    logits = g.standard_normal((T, B, V)) * scale
    units = np.array([c for c in range(V) if c != blank])
    tgt = units[g.integers(0, len(units), (B, Lmax))]
    tgt[1, 1::3] = tgt[1, 0:-1:3][: len(tgt[1, 1::3])]
    tl = np.array([Lmax, (2 * Lmax) // 3, 0, Lmax][:B])
    il = np.array([T, T - 7, T // 2, Lmax // 2][:B])
    return logits, tgt, il, tl


def torch_reference(logits, tgt, il, tl, blank):
    """nll [B] and the gradient w.r.t. the logits of the zero_infinity sum, float64 (the conversion of tests/test_ctc_any_gpu.py)"""
    lp = torch.log_softmax(torch.from_numpy(logits).double(), -1).requires_grad_(True)
    tt, ti, tg = torch.from_numpy(tl), torch.from_numpy(il), torch.from_numpy(tgt)
    ref = torch.nn.functional.ctc_loss(lp, tg, ti, tt, blank=blank, reduction="sum", zero_infinity=True)
    ref.backward()
    gl = lp.grad - lp.detach().exp() * lp.grad.sum(-1, keepdim=True)   # d/dlogits from d/dlog-probs
    per = torch.nn.functional.ctc_loss(lp.detach(), tg, ti, tt, blank=blank, reduction="none", zero_infinity=False)
    return per.numpy(), gl.numpy()


@pytest.mark.parametrize("T,B,V,Lmax,blank", [(12, 3, 5, 3, 0), (40, 4, 21, 12, 20), (70, 4, 50, 20, 25)])
def test_reference_against_torch(T, B, V, Lmax, blank):
    logits, tgt, il, tl = make_case(T, B, V, Lmax, 2.0, blank, seed=T)
    per, gl = torch_reference(logits, tgt, il, tl, blank)
    nll, occ, sm = R.ctc_forward_backward(logits, tgt, il, tl, blank)
    ok = np.isfinite(per)
    assert np.array_equal(ok, np.isfinite(nll)) and ok.any() and (B < 4 or not ok.all())
    assert np.all(nll[~ok] == math.inf)
    assert float(np.abs(nll[ok] - per[ok]).max()) <= 1e-9
    g = R.gradient(nll, occ, sm, il)
    assert float(np.abs(g - gl).max()) <= 1e-9
    live = R.live_mask(nll, il, T)
    assert float(np.abs(occ.sum(-1)[live] - 1.0).max()) <= 1e-12 and float(np.abs(occ[~live]).max(initial=0.0)) == 0.0


@pytest.mark.parametrize("T,Lmax,scale", [(40, 12, 2.0), (40, 12, 8.0), (330, 100, 8.0), (1100, 400, 6.0)])
def test_float32_run_stays_inside_the_bound(T, Lmax, scale):
    """the bound is achievable by f32 arithmetic: the float32 run of the same recursion against its float64 run.  Both see the same
    f32 logits."""
    V, blank = 21, 20
    logits, tgt, il, tl = make_case(T, 3, V, Lmax, scale, blank, seed=T + Lmax)
    logits = logits.astype(np.float32)
    nll, occ, sm = R.ctc_forward_backward(logits, tgt, il, tl, blank)
    nll32, occ32, sm32 = R.ctc_forward_backward(logits, tgt, il, tl, blank, dtype=np.float32)
    g = R.gradient(nll, occ, sm, il)
    g32 = R.gradient(nll32, occ32, sm32, il).astype(np.float64)
    assert np.isfinite(nll).all() and np.isfinite(nll32).all()
    bound = R.grad_bound(occ, sm, g, il, 1.0, U32)
    ratio = float((np.abs(g32 - g) / bound).max())
    nratio = float((np.abs(nll32 - nll) / R.nll_bound(nll, il, T)).max())
    print("T %d Lmax %d scale %g: worst gradient err/bound %.3g, worst nll err/bound %.3g" % (T, Lmax, scale, ratio, nratio))
    assert ratio <= 1.0 and nratio <= 1.0


def test_float32_run_where_the_states_lie_far_below_the_maximum():
    """why ctc_ref.A_COEF is not 1: with the transcript's columns 80 below the rest, four emissions reach -480 in log2 and one f32
    ulp there is 2^-15; the float32 run then needs more than the coefficient-1 bound, and stays inside the bound as it stands"""
    T, V, blank = 40, 21, 20
    logits, tgt, il, tl = make_case(T, 3, V, 12, 2.0, blank, seed=5)
    for b in range(3):
        logits[:, b, np.unique(tgt[b][: tl[b]])] -= 80.0
    logits = logits.astype(np.float32)
    nll, occ, sm = R.ctc_forward_backward(logits, tgt, il, tl, blank)
    nll32, occ32, sm32 = R.ctc_forward_backward(logits, tgt, il, tl, blank, dtype=np.float32)
    g = R.gradient(nll, occ, sm, il)
    err = np.abs(R.gradient(nll32, occ32, sm32, il) - g)
    ratio = float((err / R.grad_bound(occ, sm, g, il, 1.0, U32)).max())
    ratio1 = float((err / R.grad_bound(occ, sm, g, il, 1.0, U32, coef=1.0)).max())
    print("columns lowered by 80: worst gradient err/bound %.3g (%.3g at coefficient 1)" % (ratio, ratio1))
    assert ratio <= 1.0 < ratio1


# ------------------------------------------------------------------ wrong references
def wrong_reference(kind, logits, tgt, il, tl, blank):
    """gs * gradient (gs = 1 except for "scaled_twice", where the caller expects 0.25) of a forward-backward with one deliberate error"""
    T, B, V = logits.shape
    lp = R.log_softmax(logits.astype(np.float64))
    sm = np.exp(lp)
    occ = np.zeros((T, B, V))
    nll = np.full(B, math.inf)
    for b in range(B):
        Tb = min(int(il[b]), T)
        ext, skip = R.extended_target(tgt[b][: int(tl[b])], blank)
        if kind == "skip_equal":
            skip[3::2] = True                                   # the s-2 skip allowed across equal labels
        nll[b], post = R.utterance_posteriors(lp[:Tb, b], ext, skip)
        if kind == "drop_repeat":                               # the posterior of the second occurrence of a repeated unit dropped
            seen = set()
            for s in range(1, len(ext), 2):
                if int(ext[s]) in seen:
                    post[:, s] = 0
                    break
                seen.add(int(ext[s]))
        occ[:Tb, b] = R.occupancy(post, ext, V)
        if kind == "frame_shift" and Tb >= 4:                   # one frame's posteriors taken from frame t+1
            occ[Tb // 2, b] = occ[Tb // 2 + 1, b]
    g = R.gradient(nll, occ, sm, il)
    if kind == "tail_columns":                                  # columns V - V % 8 ... V-1 left as softmax
        live = R.live_mask(nll, il, T)
        g[..., V - V % 8:] = np.where(live[:, :, None], sm[..., V - V % 8:], 0)
    if kind == "scaled_twice":                                  # the upstream scalar 0.25 applied twice
        g = g * 0.25 * 0.25
    return g


@pytest.mark.parametrize("kind", ["skip_equal", "drop_repeat", "frame_shift", "tail_columns", "scaled_twice"])
def test_wrong_references_violate_the_bound(kind):
    T, Lmax, V, blank = 40, 12, 21, 20
    logits, tgt, il, tl = make_case(T, 3, V, Lmax, 8.0 if kind == "skip_equal" else 2.0, blank, seed=11)
    logits = logits.astype(np.float32)
    gs = 0.25 if kind == "scaled_twice" else 1.0
    nll, occ, sm = R.ctc_forward_backward(logits, tgt, il, tl, blank)
    g = R.gradient(nll, occ, sm, il)
    wrong = wrong_reference(kind, logits, tgt, il, tl, blank)
    err = np.abs(wrong - gs * g)
    for r in (U32, UBF):
        bound = R.grad_bound(occ, sm, g, il, gs, r)
        ratio = float((err / bound).max())
        print("%s, r = 2^%d: worst err/bound %.3g (%d elements outside)" % (kind, round(math.log2(r)), ratio, int((err > bound).sum())))
        assert R.A_COEF <= 4.0 and ratio > 4.0 / R.A_COEF, ratio   # outside even at the largest coefficient the GPU test may take
    assert float(np.abs(wrong_reference(None, logits, tgt, il, tl, blank) - g).max()) == 0.0     # the harness itself adds no error
