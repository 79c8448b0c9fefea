"""The row kernels of csrc/loss_embed.hip against float64 references: the training loss and its gradient (s2t_lsce, s2t_kd_loss), the
generator's rows (s2t_log_softmax, s2t_softmax_probs, s2t_softmax_bwd, s2t_ensemble_lse), the teacher dump (s2t_topk) and the decoder
embedding (s2t_embed_fwd, s2t_embed_bwd).

Conventions of tests/test_routes_gpu.py: inputs are generated on the host from fixed seeds; every reference is computed in float64
from the exact values the kernel received (the bf16- or f32-rounded inputs, eps / lambda / grad_scale / 1/temperature as the f32
the C ABI passes); every output ELEMENT is compared with a bound derived from the arithmetic, and a failure names the worst element.
These kernels record no launch family in `prof`, so each case cites the dispatch condition it relies on (file:line of loss_embed.hip).

Error model (u = 2^-24; r = 2^-8 for a bf16 output, u for f32).  Every first-order term below is doubled (SAFETY) to cover the
second-order terms and the libm ulp figures; the final rounding to the output dtype (r |v|) carries no margin.
  * exp2 path (lsce): exp(x - c) is evaluated as exp2(fma(x, L2E, -fl(c L2E))) with L2E = log2(e) rounded to f32.  The argument
    errs by u log2e (|x| + 2|c|) (L2E's rounding seen through x and c, and the product's rounding) plus u |arg| (the fma's
    rounding); exp2 turns an absolute argument error into ln2 times that relative error, and v_exp_f32 adds one ulp: relative
    error <= u (|x| + 2|c| + |x - c| + 2).  The error grows with |x| and |c|: rows of large logits get proportionally wider bounds.
  * expf / logf (the other kernels): <= 4 ulp; fl(a - b) before expf adds u |a - b| of relative error.
  * a sum of n terms of one sign in f32: <= depth u sum|t| in any order of that depth.  The row kernels give each of the 256 lanes
    ceil(V / 256) terms (plus at most 8 of a 16-byte vector and one tail element), then a 64-lane butterfly (6) and a serial sum
    of the 4 waves (4): depth ceil(V/256) + 19.  Loss partials: ceil(rows/1024) rows per workgroup, ceil(1024/256) partials per
    lane of lsce_finish_kernel, the same butterfly and 4-wave sum (10) and the "+=" into the caller's sum (1).
    Atomics (embed_bwd): n + 1 terms in any order.
  * lse = m + logf(s): the relative error of s, 4u max(|ln s|, 1) for logf and u |lse| for the add.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
U = 2.0 ** -24                   # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF, F32 = torch.bfloat16, torch.float32
TINY = 2.0 ** -126               # f32 results below the normal range (flushed or denormal)
SAFETY = 2.0
EINVAL = -22
PAD = 1


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield


# ------------------------------------------------------------------ shared tools
def f32(v):
    """the f32 value a float argument of the C ABI arrives as"""
    return float(torch.tensor(float(v), dtype=F32))


def rout(dtype):
    return UBF if dtype == BF else U


def d64(t):
    return t.detach().to(DEV).double()


def assert_close(out, ref, bound, what):
    """|out - ref| <= bound element by element (ref, bound float64); on failure: the worst element, its value, ref and bound"""
    o = d64(out)
    err = (o - ref).abs()
    bad = ~(err <= bound)                  # NaN counts as bad
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: out %.9g ref %.9g |err| %.3g bound %.3g (%.3gx)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(o[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx]) if float(bound[idx]) > 0 else math.inf))


def assert_scalar(out, ref, bound, what):
    err = abs(float(out) - ref)
    assert err <= bound, "%s: out %.9g ref %.9g |err| %.3g bound %.3g" % (what, float(out), ref, err, bound)


def rows_buffer(x_host, dtype, layout):
    """device [rows, V] of `dtype` holding x_host: 'padded' = kernels.alloc_rows (every row 16-byte aligned), 'dense' = row stride V
    (odd V: aligned and unaligned rows in one buffer, as the criteria's lt.contiguous() fallback makes them)"""
    rows, V = x_host.shape
    x = K.alloc_rows((rows,), V, dtype, DEV) if layout == "padded" else torch.empty((rows, V), dtype=dtype, device=DEV)
    x.copy_(x_host.to(dtype))
    return x


def nan_rows_like(x):
    """an output buffer with x's row stride, filled with NaN (also in the stride's padding): an element no kernel wrote stays NaN"""
    return torch.full((x.shape[0], x.stride(0)), math.nan, dtype=x.dtype, device=DEV)


def sum_depth(V):
    return math.ceil(V / 256) + 19


def part_depth(rows):
    return math.ceil(rows / 1024) + 4 + 10 + 1


def lse_err(rel_s, s, lse):
    """absolute error of m + logf(s) when s carries relative error rel_s (all float64 tensors)"""
    return rel_s + 4 * U * torch.log(s).abs().clamp_min(1.0) + U * lse.abs()


def targets_with_pads(rows, V, seed):
    """targets in [0, V) \\ {PAD}; ~6 % pad rows, and with more than four rows: every row of workgroup 3 (grid = min(rows, 1024),
    rows 3, 3 + grid, ...) is pad, and the LAST row of workgroup 0 is pad (its first row is not, when it has two)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (rows,), generator=g)
    t[t == PAD] = 0
    if rows > 4:
        t[torch.rand(rows, generator=g) < 0.06] = PAD
        grid = min(rows, 1024)
        t[3::grid] = PAD
        t[0] = 0
        t[(rows - 1) // grid * grid] = PAD
    return t


# ------------------------------------------------------------------ s2t_lsce
def lsce_raw(x, tgt, eps, gs, want_grad, init):
    sums = torch.tensor(init, dtype=F32, device=DEV)
    dl = nan_rows_like(x) if want_grad else None
    dlv = dl[:, :x.shape[1]] if want_grad else None
    rc = K._lib().s2t_lsce(L.dt(x), L.ptr(x), L.ptr(tgt), L.ptr(dlv), L.ptr(sums), x.shape[0], x.shape[1], K._row_ld(x), float(eps),
                           PAD, float(gs), L.stream())
    assert rc == 0, rc
    return sums, dl


def check_lsce(x, tgt_h, eps, gs, want_grad=True, result=None):
    """s2t_lsce on device rows x against float64 (header of loss_embed.hip:8-11):
        lse = logsumexp(x);  nll = lse - x_y;  smooth = V lse - sum(x);  loss += (1-eps) nll + eps/V smooth;  nll_sum += nll
        dlogits_v = gs (softmax_v - eps/V - (1-eps)[v == y]),  exactly 0 on pad rows.
    Bounds (module docstring): per row  r_se = max_v exp2rel(x_v, m) + depth u,  dlse = lse_err(r_se);
      gradient  |gs| SAFETY [p (exp2rel(x, lse) + dlse) + u (eps/V + (1-eps)[y]) + 3u (p + eps/V + (1-eps)[y])] + r |g|;
      nll       dlse + u |nll|;   smooth  V dlse + u V |lse| + depth u sum|x| + u |smooth|;
      row term  (1-eps) dnll + eps/V dsmooth + 4u |term|;  sums: their sum + part_depth u sum|terms| + u |init + total|."""
    rows, V = x.shape
    tgt = tgt_h.to(DEV)
    eps, gs = f32(eps), f32(gs)
    init = [3.25, -1.5]
    sums, dl = result if result is not None else lsce_raw(x, tgt, eps, gs, want_grad, init)
    xd = d64(x)
    live = tgt != PAD
    ty = torch.where(live, tgt, torch.zeros_like(tgt)).clamp_max(V - 1)
    m = xd.max(1, keepdim=True).values
    e = torch.exp(xd - m)
    s = e.sum(1, keepdim=True)
    lse = m + torch.log(s)
    p = e / s
    xy = xd.gather(1, ty[:, None])
    nll = (lse - xy)[:, 0]
    smooth = V * lse[:, 0] - xd.sum(1)
    term = (1 - eps) * nll + eps / V * smooth
    ev = eps / V
    ds = sum_depth(V)
    exp2rel = lambda c: U * (xd.abs() + 2 * c.abs() + (xd - c).abs() + 2)
    r_se = exp2rel(m).max(1, keepdim=True).values + ds * U
    dlse = lse_err(r_se, s, lse)
    dnll = dlse[:, 0] + U * nll.abs()
    dsmooth = V * dlse[:, 0] + U * V * lse[:, 0].abs() + ds * U * xd.abs().sum(1) + U * smooth.abs()
    dterm = SAFETY * ((1 - eps) * dnll + ev * dsmooth + 4 * U * term.abs())
    pd = part_depth(rows)
    tot, ntot = float(term[live].sum()), float(nll[live].sum())
    b0 = float(dterm[live].sum()) + SAFETY * pd * U * float(term[live].abs().sum()) + U * abs(init[0] + tot)
    b1 = float(SAFETY * dnll[live].sum()) + SAFETY * pd * U * float(nll[live].abs().sum()) + U * abs(init[1] + ntot)
    what = "lsce %s V=%d rows=%d ld=%d eps=%g" % (x.dtype, V, rows, K._row_ld(x), eps)
    assert_scalar(float(sums[0]) - init[0], tot, b0, what + " loss (+= into a non-zero sum)")
    assert_scalar(float(sums[1]) - init[1], ntot, b1, what + " nll (+= into a non-zero sum)")
    if not want_grad:
        return
    onehot = torch.zeros_like(xd).scatter_(1, ty[:, None], 1.0)
    g = gs * (p - ev - (1 - eps) * onehot)
    bound = abs(gs) * SAFETY * (p * (exp2rel(lse) + dlse) + U * (ev + (1 - eps) * onehot) + 3 * U * (p + ev + (1 - eps) * onehot))
    bound = bound + rout(x.dtype) * g.abs() + TINY
    assert_close(dl[live][:, :V], g[live], bound[live], what + " dlogits")
    assert bool((dl[~live][:, :V] == 0).all()), what + ": gradient rows of pad targets are not exactly 0"
    assert bool(dl[:, V:].isnan().all()), what + ": the kernel wrote into the row stride's padding"


def logits_host(rows, V, seed, scale=2.0):
    return torch.randn(rows, V, generator=torch.Generator().manual_seed(seed)) * scale


# V on every side of both register-row thresholds (loss_embed.hip:131-132: bf16 V <= 8192 and f32 V <= 4096 -> lsce_kernel<T, 4>,
# longer rows -> <T, 0>) and every scalar-tail length (V mod 8 / mod 4); 'dense' odd V mixes vector and scalar rows (the `vec`
# test of loss_embed.hip:34 is per row)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V", [1, 7, 100, 4096, 4097, 8000, 8192, 8193, 8200, 40000])
@pytest.mark.parametrize("layout", ["padded", "dense"])
def test_lsce_vocab_routes(dtype, V, layout):
    x = rows_buffer(logits_host(37, V, seed=V), dtype, layout)
    check_lsce(x, targets_with_pads(37, V, seed=V + 1), eps=0.1, gs=0.37)


# the per-workgroup row loop (loss_embed.hip:25: grid = min(rows, 1024), rows blockIdx.x + k gridDim.x) and its partials
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("rows", [1, 37, 1024, 1025, 3079])
@pytest.mark.parametrize("V", [101, 8193])
def test_lsce_row_loop(dtype, rows, V):
    x = rows_buffer(logits_host(rows, V, seed=rows), dtype, "dense")
    check_lsce(x, targets_with_pads(rows, V, seed=rows + 7), eps=0.1, gs=1.0)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("eps,gs,want_grad", [(0.0, 1.0, True), (0.0, 2.5, True), (0.1, 1.0, False), (0.0, 1.0, False)])
def test_lsce_eps_scale_and_sums_only(dtype, eps, gs, want_grad):
    x = rows_buffer(logits_host(1025, 1003, seed=11, scale=3.0), dtype, "dense")
    check_lsce(x, targets_with_pads(1025, 1003, seed=12), eps=eps, gs=gs, want_grad=want_grad)


# ------------------------------------------------------------------ s2t_kd_loss
def teacher(rows, V, Kt, tgt, seed):
    """indices with repeats (the target, a duplicated entry) and teacher logits; returns (int64 [rows, Kt], f32 [rows, Kt])"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, V, (rows, Kt), generator=g)
    idx[:, 0] = torch.where(tgt == PAD, torch.zeros_like(tgt), tgt).clamp_max(V - 1)
    if Kt >= 2:
        idx[:, Kt - 1] = idx[:, 0]
    if Kt >= 4:
        idx[:, 2] = idx[:, 1]
    return idx, (torch.randn(rows, Kt, generator=g) * 3).float()


def kd_raw(x, tgt, idx, tl, lam, tau, gs, init):
    s = torch.tensor([init], dtype=F32, device=DEV)
    dl = nan_rows_like(x)
    Kt = idx.shape[1] if idx is not None else 0
    rc = K._lib().s2t_kd_loss(L.dt(x), L.ptr(x), L.ptr(tgt), L.ptr(idx), L.ptr(tl), L.ptr(dl[:, :x.shape[1]]), L.ptr(s), x.shape[0],
                              x.shape[1], K._row_ld(x), Kt, float(lam), float(tau), PAD, float(gs), L.stream())
    assert rc == 0, rc
    return s, dl


def check_kd(x, tgt_h, Kt, lam, tau, gs, seed, stream_out=None):
    """s2t_kd_loss against float64 autograd of knowledge_distillation.py:44-96 (summed over non-pad rows):
        loss = sum_rows (1-lam) (-log_softmax(x)[y]) + lam (-sum_k softmax(tl/tau)_k log_softmax(x/tau)[idx_k])
    times grad_scale for the gradient; lam = 0 runs without teacher tensors (Kt = 0).
    Kernel (loss_embed.hip:316-374): per element d = (1-lam)(expf(x - lse1) - [v==y]) + lam it expf(x it - lset), rounded once to
    the output dtype, then thread 0 subtracts lam it w_k gs for k = 0..Kt-1 IN ORDER, re-rounding the element each time.
    Bounds (module docstring; p1 = softmax(x), pt = softmax(x/tau), w = softmax(tl/tau)):
    (it = fl(1/tau) is the kernel's: its rounding and the product's give 2u |. it| wherever a value is scaled by it)
      dlse1 = lse_err(u (max|x-m| + 4) + depth u),  dlset = lse_err(u (2 it max|x-m| + 4) + depth u) + 2u |m it|
      e1 = dlse1 + u (|x - lse1| + 4),  et = dlset + u (2|x it| + |x it - lset| + 4),  ew = u (2|tl it| + |tl it - max| + 14)
      element  |gs| SAFETY [(1-lam) p1 e1 + lam it pt et + 6u ((1-lam)(p1 + [y]) + lam it pt)] + r |g_0|
               + per fix-up k:  SAFETY |gs| lam it w_k (ew + 3u) + SAFETY u |g_k| + r |g_k|
      (g_0 the main term, g_k the element after the k-th fix-up in the kernel's order: the second rounding in bf16)
      row      (1-lam)(dlse1 + u |truth|) + lam sum_k w_k [(ew + 3u)|x_k it - lset| + dlset + 2u |x_k it|] + (Kt + 3) u |term|
      sum      SAFETY (rows) + part_depth u sum|terms| + u |init + total|."""
    rows, V = x.shape
    tgt = tgt_h.to(DEV)
    lam, tau, gs = f32(lam), f32(tau), f32(gs)
    it = 1.0 / tau                                        # exact here; the kernel's fl(1/tau) is in the bound
    if lam > 0:
        idx_h, tl_h = teacher(rows, V, Kt, tgt_h, seed)
        idx, tl = idx_h.to(DEV), tl_h.to(DEV)
    else:
        idx = tl = None
        Kt = 0
    init = -0.75
    if stream_out is not None:
        s, dl = stream_out
    else:
        s, dl = kd_raw(x, tgt, idx, tl, lam, tau, gs, init)
    live = tgt != PAD
    ty = torch.where(live, tgt, torch.zeros_like(tgt)).clamp_max(V - 1)
    xd = d64(x)
    xr = xd.clone().requires_grad_(True)
    loss_rows = torch.zeros(rows, dtype=torch.float64, device=DEV)
    if lam > 0:
        lpt = torch.log_softmax(xr / tau, -1)
        w = torch.softmax(d64(tl) / tau, -1)
        loss_rows = loss_rows + lam * (-(lpt.gather(1, idx) * w).sum(-1))
    if lam < 1:
        lp1 = torch.log_softmax(xr, -1)
        loss_rows = loss_rows + (1 - lam) * (-lp1.gather(1, ty[:, None])[:, 0])
    loss_rows = loss_rows * live
    loss_rows.sum().backward()
    g = gs * xr.grad
    term = loss_rows.detach()

    m = xd.max(1, keepdim=True).values
    ds = sum_depth(V)
    s1 = torch.exp(xd - m).sum(1, keepdim=True)
    lse1 = m + torch.log(s1)
    st = torch.exp((xd - m) * it).sum(1, keepdim=True)
    lset = m * it + torch.log(st)
    dx = (xd - m).abs().max(1, keepdim=True).values
    dlse1 = lse_err(U * (dx + 4) + ds * U, s1, lse1)
    dlset = lse_err(U * (2 * it * dx + 4) + ds * U, st, lset) + 2 * U * (m * it).abs()
    p1, pt = torch.exp(xd - lse1), torch.exp(xd * it - lset)
    onehot = torch.zeros_like(xd).scatter_(1, ty[:, None], 1.0)
    e1 = dlse1 + U * ((xd - lse1).abs() + 4)
    et = dlset + U * (2 * (xd * it).abs() + (xd * it - lset).abs() + 4)
    r = rout(x.dtype)
    bound = abs(gs) * SAFETY * ((1 - lam) * p1 * e1 + lam * it * pt * et + 6 * U * ((1 - lam) * (p1 + onehot) + lam * it * pt))
    g0 = gs * ((1 - lam) * (p1 - onehot) + lam * it * pt)
    bound = bound + r * g0.abs() + TINY
    truth = (lse1 - xd.gather(1, ty[:, None]))[:, 0]
    brow = (1 - lam) * (dlse1[:, 0] + U * truth.abs()) if lam < 1 else torch.zeros_like(truth)
    if lam > 0:
        tv = d64(tl) * it
        ew = U * (2 * tv.abs() + (tv - tv.max(1, keepdim=True).values).abs() + 14)
        xk = xd.gather(1, idx) * it
        brow = brow + lam * (w * ((ew + 3 * U) * (xk - lset).abs() + dlset + 2 * U * xk.abs())).sum(1)
        cur = g0.clone()
        rr = torch.arange(rows, device=DEV)
        for k in range(Kt):
            c = idx[:, k]
            cur[rr, c] = cur[rr, c] - lam * it * w[:, k] * gs
            bound[rr, c] += SAFETY * abs(gs) * lam * it * w[:, k] * (ew[:, k] + 3 * U) + (SAFETY * U + r) * cur[rr, c].abs()
        assert_close(cur[live], g[live], torch.full_like(g[live], 1e-9 * max(1.0, float(g.abs().max()))),
                     "kd reference: the fix-up order replays autograd")
    brow = SAFETY * (brow + (Kt + 3) * U * term.abs())
    tot = float(term[live].sum())
    b = float(brow[live].sum()) + SAFETY * part_depth(rows) * U * float(term[live].abs().sum()) + U * abs(init + tot)
    what = "kd %s V=%d rows=%d ld=%d Kt=%d lam=%g tau=%g" % (x.dtype, V, rows, K._row_ld(x), Kt, lam, tau)
    assert_scalar(float(s[0]) - init, tot, b, what + " loss (+= into a non-zero sum)")
    assert_close(dl[live][:, :V], g[live], bound[live], what + " dlogits")
    assert bool((dl[~live][:, :V] == 0).all()), what + ": gradient rows of pad targets are not exactly 0"
    assert bool(dl[:, V:].isnan().all()), what + ": the kernel wrote into the row stride's padding"


# kd_kernel has one route (loss_embed.hip:387-388); lambda selects the terms at loss_embed.hip:352-353 / 360-361 / 365
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("tau", [1.0, 2.0])
def test_kd_lambda_tau(dtype, lam, tau):
    x = rows_buffer(logits_host(37, 1003, seed=21), dtype, "dense")
    check_kd(x, targets_with_pads(37, 1003, seed=22), Kt=8, lam=lam, tau=tau, gs=0.6, seed=23)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Kt,rows,V,layout,lam,tau", [(1, 37, 1003, "dense", 0.3, 2.0), (64, 37, 1003, "dense", 0.3, 2.0),
                                                      (8, 1500, 517, "dense", 0.3, 2.0), (64, 1025, 2000, "padded", 1.0, 2.0),
                                                      (64, 3079, 301, "dense", 0.5, 1.5), (8, 1024, 40, "dense", 0.7, 1.0)])
def test_kd_teacher_width_and_rows(dtype, Kt, rows, V, layout, lam, tau):
    x = rows_buffer(logits_host(rows, V, seed=rows + Kt), dtype, layout)
    check_kd(x, targets_with_pads(rows, V, seed=rows + 1), Kt=Kt, lam=lam, tau=tau, gs=1.0, seed=rows + 2)


def test_kd_refuses_bad_arguments():
    """loss_embed.hip:380-381: Kt > 64 with lambda > 0, and tau <= 0, are S2T_EINVAL (nothing is launched)"""
    rows, V = 4, 100
    x = torch.zeros(rows, V, device=DEV)
    tgt = torch.zeros(rows, dtype=torch.long, device=DEV)
    s = torch.zeros(1, device=DEV)
    dl = torch.zeros(rows, V, device=DEV)
    for Kt, lam, tau in [(65, 0.5, 1.0), (8, 0.5, 0.0), (8, 0.5, -1.0), (8, 0.0, 0.0)]:
        idx = torch.zeros(rows, Kt, dtype=torch.long, device=DEV)
        tl = torch.zeros(rows, Kt, device=DEV)
        rc = K._lib().s2t_kd_loss(L.dt(x), L.ptr(x), L.ptr(tgt), L.ptr(idx), L.ptr(tl), L.ptr(dl), L.ptr(s), rows, V, V, Kt,
                                  float(lam), float(tau), PAD, 1.0, L.stream())
        assert rc == EINVAL, (Kt, lam, tau, rc)


# ------------------------------------------------------------------ two streams
def test_lsce_and_kd_on_two_streams():
    """The partial-sum scratch of s2t_lsce / s2t_kd_loss is per (device, stream) (prof.hpp, s2t_scratch): the same entry point on two
    streams at once must not share partials.  Each stream runs lsce then kd on its own rows; both are checked against their own
    references (the first calls on each stream only allocate the scratch, so that the timed-together launches do not wait on it)."""
    rows, V = 3079, 8193
    xs = [rows_buffer(logits_host(rows, V, seed=90 + i), BF, "dense") for i in range(4)]
    tg = [targets_with_pads(rows, V, seed=95 + i) for i in range(4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    tdev = [t.to(DEV) for t in tg]
    Kt, lam, tau = 8, 0.3, 2.0
    tch = [teacher(rows, V, Kt, tg[i], seed=97 + i) for i in range(4)]
    tch = [(a.to(DEV), b.to(DEV)) for a, b in tch]
    torch.cuda.synchronize()
    for st in streams:
        with torch.cuda.stream(st):
            lsce_raw(xs[0], tdev[0], 0.1, 1.0, False, [0.0, 0.0])
            kd_raw(xs[0], tdev[0], tch[0][0], tch[0][1], lam, tau, 1.0, 0.0)
    torch.cuda.synchronize()
    out = {}
    for rep in range(2):                                  # issue order interleaves the streams: lsce | lsce, then kd | kd
        for j, st in enumerate(streams):
            with torch.cuda.stream(st):
                i = 2 * j + rep
                if rep == 0:
                    out[i] = lsce_raw(xs[i], tdev[i], 0.1, 1.0, True, [3.25, -1.5])
                else:
                    out[i] = kd_raw(xs[i], tdev[i], tch[i][0], tch[i][1], lam, tau, 1.0, -0.75)
    torch.cuda.synchronize()
    for i in (0, 2):
        check_lsce(xs[i], tg[i], eps=0.1, gs=1.0, result=out[i])
    for i in (1, 3):
        check_kd(xs[i], tg[i], Kt, lam, tau, 1.0, seed=97 + i, stream_out=out[i])


# ------------------------------------------------------------------ s2t_log_softmax, s2t_softmax_probs, s2t_softmax_bwd
def softmax_rows(V, seed):
    """logits spread uniformly over +-80, one dominant logit (+40), all logits equal, two rows of randn * 3"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(5, V, generator=g) * 3
    x[0] = (torch.rand(V, generator=g) * 2 - 1) * 80
    x[1, V // 2] += 40
    x[2] = 2.75
    return x


# one route per direction (log_softmax_kernel / softmax_bwd_kernel, loss_embed.hip:436-460); `ld` is the row stride of the input
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 8000])
@pytest.mark.parametrize("layout", ["padded", "dense"])
@pytest.mark.parametrize("temperature", [1.0, 0.7, 1.5])
def test_softmax_rows_temperature(dtype, V, layout, temperature):
    """out = log_softmax(x it) / softmax(x it) in f32, it = f32(1/temperature) as passed; backward from the saved output y and an
    upstream gradient g:  log: dx = it (g - exp(y) sum g);  probs: dx = it y (g - sum g y), rounded to the logits' dtype.
    Forward (z = x it, m = max z):  dlse = u max|z| (z rounded) + u (max|z - m| + 4) + depth u + 4u max(|ln s|, 1) + u |lse|;
      log-prob  SAFETY (u |z| + dlse + u |lp|);  prob  p (that + SAFETY 4u) + TINY -- relative to each probability, not to the row's
      largest one.
    Backward:  dS = depth u sum|g| (log) or (depth + 1) u sum|g y| (probs);
      log    SAFETY (|it| (p dS + 4u p |S| + 6u (|g| + p |S|)) + u |dx|) + r |dx|
      probs  SAFETY (|it| (|y| (dS + u (|g| + |S|)) + 2u |y (g - S)|) + u |dx|) + r |dx|."""
    x = rows_buffer(softmax_rows(V, seed=V), dtype, layout)
    rows = x.shape[0]
    it = f32(1.0 / temperature)
    lp = K.log_softmax(x, temperature)
    pr = K.softmax_probs(x, temperature)
    z = d64(x) * it
    m = z.max(1, keepdim=True).values
    s = torch.exp(z - m).sum(1, keepdim=True)
    lse = m + torch.log(s)
    lp_ref = z - lse
    p_ref = torch.exp(lp_ref)
    dlse = U * z.abs().max(1, keepdim=True).values + U * ((z - m).abs().max(1, keepdim=True).values + 4) + sum_depth(V) * U
    dlse = lse_err(dlse, s, lse)
    blp = SAFETY * (U * z.abs() + dlse + U * lp_ref.abs())
    what = "%s V=%d ld=%d T=%g" % (dtype, V, K._row_ld(x), temperature)
    assert_close(lp, lp_ref, blp, "log_softmax " + what)
    assert_close(pr, p_ref, p_ref * (blp + SAFETY * 4 * U) + TINY, "softmax_probs " + what)

    gout = (torch.randn(rows, V, generator=torch.Generator().manual_seed(V + 3))).to(DEV)
    gd = d64(gout)
    ds = sum_depth(V)
    for log_probs, y in ((True, lp), (False, pr)):
        dx = K.softmax_bwd(y, gout, dtype, log_probs, temperature)
        yd = d64(y)
        if log_probs:
            p = torch.exp(yd)
            S = gd.sum(1, keepdim=True)
            ref = it * (gd - p * S)
            dS = ds * U * gd.abs().sum(1, keepdim=True)
            e = abs(it) * (p * dS + 4 * U * p * S.abs() + 6 * U * (gd.abs() + p * S.abs()))
        else:
            S = (gd * yd).sum(1, keepdim=True)
            ref = it * yd * (gd - S)
            dS = (ds + 1) * U * (gd * yd).abs().sum(1, keepdim=True)
            e = abs(it) * (yd.abs() * (dS + U * (gd.abs() + S.abs())) + 2 * U * (yd * (gd - S)).abs())
        bound = SAFETY * (e + U * ref.abs()) + rout(dtype) * ref.abs() + TINY
        assert_close(dx, ref, bound, "softmax_bwd log_probs=%d " % log_probs + what)


# ------------------------------------------------------------------ s2t_topk
def topk_rows(rows, V, dtype, seed):
    """values on a coarse grid (bf16: 13 levels, f32: steps of 1/16) so that ties are common, ~8 % -inf entries, and with three or
    more rows one row that is -inf throughout"""
    g = torch.Generator().manual_seed(seed)
    if dtype == BF:
        x = torch.randint(-6, 7, (rows, V), generator=g).float() / 4
    else:
        x = torch.round(torch.randn(rows, V, generator=g) * 16) / 16
    x[torch.rand(rows, V, generator=g) < 0.08] = -math.inf
    if rows >= 3:
        x[rows // 2] = -math.inf
    return x


TOPK = sorted({(V, k) for V in (1, 63, 64, 65, 5001) for k in (1, 5, 64, V) if k <= V})


# one route (topk_kernel, loss_embed.hip:529-531: four rows per workgroup, rows beyond `rows` return at :505)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V,k", TOPK)
def test_topk_exact_order(dtype, V, k):
    """a selection: values bit-equal and columns equal to a stable float64 sort on (-value, column) (ties: lower column first)"""
    import numpy as np
    for rows, layout in ((1, "dense"), (3, "padded"), (5, "dense"), (1001, "padded")):
        x = rows_buffer(topk_rows(rows, V, dtype, seed=rows * 7 + V + k), dtype, layout)
        vals, idx = K.topk(x, k)
        xv = x.float().cpu().double().numpy()
        cols = np.broadcast_to(np.arange(V), xv.shape)
        order = np.lexsort((cols, -xv), axis=-1)[:, :k]
        ref_v = np.take_along_axis(xv, order, axis=-1)
        what = "topk %s rows=%d V=%d k=%d ld=%d" % (dtype, rows, V, k, K._row_ld(x))
        got_v, got_i = vals.cpu().double().numpy(), idx.cpu().numpy()
        bad = np.argwhere((got_v != ref_v) | (got_i != order))
        assert bad.size == 0, "%s: %d entries differ; first at %s: got (%r, col %d), want (%r, col %d)" % (
            what, len(bad), tuple(bad[0]), got_v[tuple(bad[0])], got_i[tuple(bad[0])], ref_v[tuple(bad[0])], order[tuple(bad[0])])


# ------------------------------------------------------------------ s2t_ensemble_lse
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_ensemble_lse(n):
    """out = log(mean_j exp(lp_j)) element-wise.  numel = 263 x 4001 = 1,052,263: above the 4096 x 256 threads of the capped grid
    (loss_embed.hip:489-490, so the loop strides) and not a multiple of 256.  Members are -inf at common elements (all -inf: the
    result must be exactly -inf, the `m > -INFINITY` guard of loss_embed.hip:476) and at their own (partly -inf: finite).
    Bound (m = max_j, s = sum_j exp(lp_j - m), -inf members contribute an exact 0):
      SAFETY (u (max_j|lp_j - m| + 4 + n) + 4u max(|ln s|, 1) + u (|m| + |ln s|) + 2u ln n + u |out|)."""
    rows, V = 263, 4001
    g = torch.Generator().manual_seed(40 + n)
    common = torch.rand(rows, V, generator=g) < 0.01
    mem = []
    for _ in range(n):
        lp = torch.log_softmax(torch.randn(rows, V, generator=g) * 3, -1)
        lp[common] = -math.inf
        lp[torch.rand(rows, V, generator=g) < 0.05] = -math.inf
        mem.append(lp.float().to(DEV))
    out = K.ensemble_lse(mem)
    X = torch.stack([d64(t) for t in mem])
    dead = torch.isneginf(X).all(0)
    assert bool(dead.any()) and (n == 1 or bool((torch.isneginf(X).any(0) & ~dead).any()))
    assert bool(torch.isneginf(out[dead]).all()), "ensemble n=%d: %d all-(-inf) elements are not -inf (NaN: %d)" % (
        n, int((~torch.isneginf(out[dead])).sum()), int(out[dead].isnan().sum()))
    live = ~dead
    Xl = X[:, live]
    m = Xl.max(0).values
    ref = torch.logsumexp(Xl, 0) - math.log(n)
    s = torch.exp(Xl - m).sum(0)
    spread = torch.where(torch.isneginf(Xl), torch.zeros_like(Xl), (Xl - m).abs()).max(0).values
    bound = SAFETY * (U * (spread + 4 + n) + 4 * U * torch.log(s).abs().clamp_min(1.0) + U * (m.abs() + torch.log(s))
                      + 2 * U * math.log(n) + U * ref.abs())
    assert_close(out[live], ref, bound, "ensemble_lse n=%d" % n)


def test_ensemble_refuses_nine_members():
    """loss_embed.hip:486: at most 8 members (EnsPtrs), n = 9 is S2T_EINVAL before anything is launched"""
    t = [torch.zeros(300, device=DEV) for _ in range(9)]
    out = torch.zeros(300, device=DEV)
    arr = (ctypes.c_void_p * 9)(*[L.ptr(x) for x in t])
    assert K._lib().s2t_ensemble_lse(9, ctypes.addressof(arr), L.ptr(out), 300, L.stream()) == EINVAL


# ------------------------------------------------------------------ s2t_embed_fwd, s2t_embed_bwd
HOT = 5


def embed_tokens(B, Ln, vocab, seed):
    """row 0 without pads, row 1 with trailing pads, row 2 with pads between tokens, row 3 all pad; token HOT fills about half"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, vocab, (B, Ln), generator=g)
    tok[tok == PAD] = 2
    tok[torch.rand(B, Ln, generator=g) < 0.5] = HOT
    tok[1, (Ln + 1) // 2:] = PAD
    tok[2, 1::3] = PAD
    tok[3] = PAD
    return tok


# one route per direction (loss_embed.hip:184-185 grid (B, ceil(L/8)), 195-196 grid (L, B)); L > 1024 refused at :182
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("Ln", [1, 7, 8, 9, 17, 1024])
@pytest.mark.parametrize("D", [64, 320])
def test_embedding_positions_and_accumulate(dtype, Ln, D):
    """forward: out[l][b] = scale W[tok] + table[pos], pos = PAD + #non-pad tokens up to l (PAD for a pad token);
      bound  SAFETY u (|scale W| + |out|) + r |out|  (one product, one add, one rounding to the dtype).
    pos_offset (decoder_step, engine.py): embed_fwd(tokens[:, t:t+1], pos_offset=t) equals row t of the full call, bit for bit, in
      every batch row with no pad before t.
    backward: dW[c] += scale dout[l][b] over the non-pad positions holding token c, by f32 atomics into a dW that has contents;
      with n_c of them:  SAFETY u (n_c + 2) (|dW0| + sum |scale dout|);  the pad row is unchanged, bit for bit."""
    B, vocab = 4, 50
    tok_h = embed_tokens(B, Ln, vocab, seed=Ln * 3 + D)
    tok = tok_h.to(DEV)
    g = torch.Generator().manual_seed(Ln + D)
    W = (torch.randn(vocab, D, generator=g)).to(dtype).to(DEV)
    table_h = torch.randn(PAD + 2 + 2 * Ln, D, generator=g)
    table_h[PAD] = 0
    table = table_h.to(DEV)
    scale = f32(math.sqrt(D))
    out = K.embed_fwd(tok, W, table, scale, PAD)
    mask = tok != PAD
    pos = torch.where(mask, PAD + torch.cumsum(mask.long(), 1), torch.full_like(tok, PAD))
    sw = scale * d64(W)[tok]
    ref = (sw + d64(table)[pos]).transpose(0, 1)
    swt = sw.transpose(0, 1)
    what = "embed_fwd %s L=%d D=%d" % (dtype, Ln, D)
    assert_close(out, ref, SAFETY * U * (swt.abs() + ref.abs()) + rout(dtype) * ref.abs(), what)
    ts = range(Ln) if Ln <= 17 else (0, 1, 7, 8, 9, 500, 511, 512, 1023)
    for t in ts:
        o = K.embed_fwd(tok[:, t:t + 1].contiguous(), W, table, scale, PAD, pos_offset=t)
        for b in range(B):
            if bool(mask[b, :t].all()) or not bool(mask[b, t]):
                assert torch.equal(o[0, b], out[t, b]), "%s: pos_offset=%d, batch row %d differs from the full call" % (what, t, b)

    dout = torch.randn(Ln, B, D, generator=g).to(dtype).to(DEV)
    dW0 = torch.randn(vocab, D, generator=g).to(DEV)
    dW = dW0.clone()
    K.embed_bwd(tok, dout, dW, scale, PAD)
    live = mask.t().reshape(-1)
    rows_tok = tok.t().reshape(-1)[live]
    contrib = scale * d64(dout).reshape(-1, D)[live]
    ref = d64(dW0).index_add(0, rows_tok, contrib)
    absum = d64(dW0).abs().index_add(0, rows_tok, contrib.abs())
    n = torch.zeros(vocab, dtype=torch.float64, device=DEV).index_add(0, rows_tok, torch.ones_like(rows_tok, dtype=torch.float64))
    assert Ln < 1024 or int(n[HOT]) >= 100
    ref[PAD] = d64(dW0)[PAD]
    assert_close(dW, ref, SAFETY * U * (n[:, None] + 2) * absum, "embed_bwd %s L=%d D=%d" % (dtype, Ln, D))
    assert torch.equal(dW[PAD], dW0[PAD]), "embed_bwd: the pad row changed"


def test_embedding_refuses_long_rows():
    """loss_embed.hip:182: L > 1024 is S2T_EINVAL (positions are counted by one wave per chunk, up to L <= 1024)"""
    D = 64
    tok = torch.full((1, 1025), 3, dtype=torch.long, device=DEV)
    W = torch.zeros(50, D, device=DEV)
    table = torch.zeros(1100, D, device=DEV)
    out = torch.zeros(1025, 1, D, device=DEV)
    assert K._lib().s2t_embed_fwd(L.dt(W), L.ptr(tok), L.ptr(W), L.ptr(table), L.ptr(out), 1, 1025, D, 8.0, PAD, 0, L.stream()) == EINVAL
