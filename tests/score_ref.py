"""float64 restatement of s2t_score_targets (include/s2t_hip.h) and the per-element error bound of its f32 arithmetic.

Contract, per member j and position (b, t) with x = logits_j[b][t][0..V) and c = target[b][t]:
    m_j = max_v x_v;  s_j = sum_v exp(x_v - m_j);  lp_j = x_c - (m_j + log s_j)
    n == 1: out = lp_0;  n > 1: M = max_j lp_j; -inf if M is, else M + log(sum_j exp(lp_j - M)) - log n;  c outside [0, V): NaN.

Error model (the conventions of tests/test_loss_rows_gpu.py: u = 2^-24; every first-order term is doubled (SAFETY) to cover the
second-order terms and the libm ulp figures; expf / logf <= 4 ulp; fl(a - b) before expf adds u |a - b| of relative error).  The
reference is taken from the exact values the kernel received (bf16 -> f32 is exact), so the inputs carry no rounding; a caller whose
reference comes from unrounded values adds `input_rounding` below.

The kernel (csrc/score.hip) keeps a running (max, sum) pair per slot, a row being split over 256 slots, and merges the slots' pairs by a
64-lane butterfly (6 merges) and a serial merge of four groups (3).  For one term exp(x_v - m):
  * it is evaluated against the running maximum c >= x_v of its slot through the hardware exp2, as exp2(fma(x_v, L2E, -fl(c L2E)))
    with L2E = log2(e) rounded to f32 -- the form and the bound of lsce_kernel (test_loss_rows_gpu.py, "exp2 path"): relative error
    <= u (|x_v| + 2|c| + |x_v - c| + 2).  c is one of the row's finite logits, so |x_v| + 2|c| <= 3 xmax with xmax = max over the
    finite x_v of |x_v|: like there, rows of large logits get proportionally wider bounds;
  * it is later multiplied by expf(c - c'), expf(c' - c''), ... up to the row's m (rescales and merges): the exponents' subtraction
    roundings are u times (c' - c) + (c'' - c') + ..., and with the |x_v - c| above that is u (m - x_v) <= u spread, the differences
    being of one sign (the maxima only grow); spread = max over the finite x_v of (m - x_v);
  * the steps it lives through, with k = ceil(V / 256): at most k + 15 additions into its slot's sum (a slot holds whole vectors of
    up to 8 values and a tail of up to 7) at u each; at most k + 8 rescales of that sum (one per vector or tail element; the scalar
    form has k of them) at 5u each (expf 4u + product u); the 9 merges at 6u each (expf 4u, product u, addition u):
        steps(V) = (k + 15) + 5 (k + 8) + 6 * 9 = 6 k + 109   units of u.
  relative error of s:  rel_s = u (3 xmax + spread + 2 + steps(V))
  lse = m + logf(s):    dlse = rel_s + 4u max(|ln s|, 1) + u |lse|           (lse_err of test_loss_rows_gpu.py)
  lp = x_c - lse:       e = SAFETY (dlse + u |lp|)                           (x_c = -inf: lp = -inf exactly)
Combine (n > 1), the bound of test_loss_rows_gpu.py::test_ensemble_lse for exact inputs, with m = max_j lp_j, s = sum_j exp(lp_j - m):
    SAFETY (u (max_j |lp_j - m| + 4 + n) + 4u max(|ln s|, 1) + u (|m| + |ln s|) + 2u ln n + u |out|)
plus the members' own errors: d out / d lp_j = softmax_j(lp) >= 0 sums to one, so they pass through as at most max_j e_j (members at
-inf are exact and carry weight 0).  TINY covers results below the normal range.
"""
import math

import torch

U = 2.0 ** -24
UBF = 2.0 ** -8
TINY = 2.0 ** -126
SAFETY = 2.0


def steps(V):
    return 6 * math.ceil(V / 256) + 109


def member_lp(x, target):
    """x: float64 [B, L, V] (the exact values the kernel reads), target int64 [B, L] ->
    (lp [B, L] float64 with NaN where the target is outside [0, V), its bound e [B, L], valid [B, L])"""
    V = x.shape[-1]
    valid = (target >= 0) & (target < V)
    c = torch.where(valid, target, torch.zeros_like(target))
    m = x.max(-1).values
    d = x - m[..., None]
    s = torch.exp(d).sum(-1)
    lse = m + torch.log(s)
    xc = x.gather(-1, c[..., None])[..., 0]
    lp = xc - lse
    spread = torch.where(torch.isfinite(d), -d, torch.zeros_like(d)).max(-1).values
    xmax = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).max(-1).values
    rel_s = U * (3 * xmax + spread + 2 + steps(V))
    dlse = rel_s + 4 * U * torch.log(s).abs().clamp_min(1.0) + U * lse.abs()
    e = SAFETY * (dlse + U * lp.abs())
    e = torch.where(torch.isfinite(lp), e, torch.zeros_like(e))
    lp = torch.where(valid, lp, torch.full_like(lp, math.nan))
    return lp, e, valid


def score_ref(xs, target):
    """xs: list of n [B, L, V] tensors (any float dtype, any device), target int64 [B, L] -> (ref, bound) float64 [B, L].
    ref is NaN where the target is out of range and -inf where the contract says so; bound is finite everywhere and meaningful where ref
    is finite."""
    n = len(xs)
    target = target.to(xs[0].device)
    lps, es = [], []
    for x in xs:
        lp, e, valid = member_lp(x.double(), target)
        lps.append(lp)
        es.append(e)
    if n == 1:
        return lps[0], es[0] + TINY
    X = torch.stack(lps)                                        # [n, B, L]
    E = torch.stack(es)
    m = X.max(0).values
    dead = torch.isneginf(m)
    ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    t = torch.exp(X - ms)
    s = t.sum(0)
    out = ms + torch.log(s) - math.log(n)
    out = torch.where(dead, torch.full_like(out, -math.inf), out)
    out = torch.where(valid, out, torch.full_like(out, math.nan))
    fin = torch.isfinite(X)
    spread = torch.where(fin, (X - ms).abs(), torch.zeros_like(X)).max(0).values
    ls = torch.where(s > 0, torch.log(s.clamp_min(1e-300)), torch.zeros_like(s))
    oa = torch.where(torch.isfinite(out), out.abs(), torch.zeros_like(out))
    comb = SAFETY * (U * (spread + 4 + n) + 4 * U * ls.abs().clamp_min(1.0) + U * (ms.abs() + ls.abs()) + 2 * U * math.log(n) + U * oa)
    passed = torch.where(fin, E, torch.zeros_like(E)).max(0).values
    return out, comb + passed + TINY


def log_softmax_bound(x):
    """the bound tests/test_loss_rows_gpu.py::test_softmax_rows_temperature holds K.log_softmax to at temperature 1 (restated: the
    three-pass log_softmax_kernel, sum depth ceil(V/256) + 19), for every element of float64 rows x [..., V] -> [..., V]"""
    V = x.shape[-1]
    m = x.max(-1, keepdim=True).values
    s = torch.exp(x - m).sum(-1, keepdim=True)
    lse = m + torch.log(s)
    lp = x - lse
    d = x - m
    spread = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d)).amax(-1, keepdim=True)
    xa = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x))
    dlse = U * xa.amax(-1, keepdim=True) + U * (spread + 4) + (math.ceil(V / 256) + 19) * U
    dlse = dlse + 4 * U * torch.log(s).abs().clamp_min(1.0) + U * lse.abs()
    lpa = torch.where(torch.isfinite(lp), lp.abs(), torch.zeros_like(lp))
    return SAFETY * (U * xa + dlse + U * lpa)


def ensemble_lse_bound(X):
    """the bound of tests/test_loss_rows_gpu.py::test_ensemble_lse for K.ensemble_lse on exact float64 inputs X [n, ...] (restated)"""
    n = X.shape[0]
    m = X.max(0).values
    ms = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    fin = torch.isfinite(X)
    s = torch.exp(X - ms).sum(0)
    ls = torch.where(s > 0, torch.log(s.clamp_min(1e-300)), torch.zeros_like(s))
    out = ms + ls - math.log(n)
    spread = torch.where(fin, (X - ms).abs(), torch.zeros_like(X)).max(0).values
    return SAFETY * (U * (spread + 4 + n) + 4 * U * ls.abs().clamp_min(1.0) + U * (ms.abs() + ls.abs()) + 2 * U * math.log(n) + U * out.abs())


def input_rounding(x, unit=UBF):
    """what rounding the logits to a format of unit roundoff `unit` adds to a log-probability computed from the unrounded values:
    |d lse| <= max_v unit |x_v| (lse is a weighted mean of perturbations) and |d x_c| <= unit |x_c| <= the same maximum"""
    return 2 * unit * x.double().abs().amax(-1)


def assert_scores(out, ref, bound, what):
    """out (f32 [B, L]) against (ref, bound): NaN exactly where ref is NaN, -inf exactly where ref is -inf, within bound elsewhere; a
    failure names the worst element"""
    o = out.detach().double().to(ref.device)
    nan = torch.isnan(ref)
    assert bool((torch.isnan(o) == nan).all()), "%s: NaN at %s, expected at %s" % (
        what, torch.isnan(o).nonzero().tolist()[:8], nan.nonzero().tolist()[:8])
    ninf = torch.isneginf(ref)
    assert bool((torch.isneginf(o) == ninf).all()), "%s: -inf at %s, expected at %s" % (
        what, torch.isneginf(o).nonzero().tolist()[:8], ninf.nonzero().tolist()[:8])
    live = ~(nan | ninf)
    err = torch.where(live, (o - ref).abs(), torch.zeros_like(ref))
    bad = live & ~(err <= bound)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound, torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: out %.9g ref %.9g |err| %.3g bound %.3g (%.3gx)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(o[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx])))
