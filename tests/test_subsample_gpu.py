"""The subsampler kernels of csrc/subsample.hip against float64 references: conv1 forward with its BatchNorm statistics
(s2t_conv1_fwd), the conv1 weight / bias gradient alone (s2t_conv1_bwd) and fused with the BatchNorm backward (s2t_conv1_bwd_bn, both
forms), the per-channel sums (s2t_chan_sums), BatchNorm finalize / apply / backward (s2t_bn_finalize, s2t_bn_apply,
s2t_bn_bwd_apply), and the whole chain through Engine.subsample_fwd / subsample_bwd with its conv2 routes and weight permutes.

Conventions of tests/test_routes_gpu.py: every reference is computed in float64 from the exact values the kernel received (its stored
y / pre / dyn, the f32 mean / rstd and the double sums it was given); every output ELEMENT is compared with a bound derived from the
arithmetic the kernel does, and a failure names the worst element.  These kernels record no launch family in `prof`, so each case
that depends on a size switch cites the dispatch condition (file:line of subsample.hip).

Error model (u = 2^-24; r = 2^-8 for a bf16 output, u for f32; gamma_n = n u / (1 - n u)).
  * conv1 forward: the f32 MFMA is an exact fmaf chain (the bias is the accumulators' start, then nine products, three zero
    taps): |acc - conv| <= gamma_9 (|b| + sum |w||x|).  ReLU is 1-Lipschitz; the stored value adds r |y|.
  * gelu_f (common.hpp) = 0.5 x (1 + erff(x / sqrt 2)): the argument's rounding moves erf by at most (2/sqrt(pi)) t e^-t^2 u <=
    0.5 u, erff errs by <= 4 u (absolute, values <= 1), 1 + erf and the two products add 3 u relative: |gelu_f(x) - gelu(x)| <=
    0.5 |x| 7.5 u + 2 u |gelu| <= 6 u |x|; the tests use 8 u |x|.  gelu_grad_f = 0.5 (1 + erff) + x expf(-x^2/2) / sqrt(2 pi): the
    cdf part errs by <= 3 u, the pdf part by |x| pdf (x^2/2 + 4) u <= 1.3 u: <= 8 u absolute with the final add.
  * a sum of terms t in f32 along a chain of depth d (serial adds, shuffle-tree levels, MFMA accumulation, the "+=" into an
    existing value) errs by <= d u sum |t|; double sums and double atomics add <= 2^-40 sum |t| at these sizes.  Each bound below
    states its depth from the kernel's own counts.
  * dpre of the BatchNorm backward is formed from three per-channel f32 constants, ka = gamma rstd, kb = -ka m2 rstd,
    kc = ka (m2 rstd mean - m1) (m1, m2 = sums / n rounded to f32): each constant carries <= 6 u of the magnitudes it is made of, and
    the two fmas round once each, so |r - r64| <= 8 u M with M = |ka dyn| + |ka m2 rstd y| + |ka| (|m2 rstd mean| + |m1|) -- the
    magnitudes the kernel adds (subsample.hip:337,422), not |dpre|: kb y and kc cancel when |mean| >> std.  The activation derivative
    multiplies that by <= 1.13 and GELU's adds 8 u |r| <= 8 u M: e_p = 8 u M (ReLU), 18 u M (GELU).
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
U = 2.0 ** -24                   # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF, F32 = torch.bfloat16, torch.float32
EINVAL = -22
DSLACK = 2.0 ** -40              # double sums / double atomics, relative to the sum of magnitudes
WORST = {}                       # kernel -> worst |err| / bound seen (printed at the end of the module: pytest -s shows it)


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    if WORST:
        print("\nworst |err| / bound per kernel: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


# ------------------------------------------------------------------ shared tools
def rout(dtype):
    return UBF if dtype == BF else U


def gam(n):
    return n * U / (1 - n * U)


def d64(t, dev=DEV):
    return t.detach().to(dev).double()


def assert_close(out, ref, bound, what, kernel=None):
    """|out - ref| <= bound element by element (ref, bound float64); on failure: the worst element, its value, ref and bound"""
    o = d64(out, ref.device)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device).expand_as(ref)
    err = (o - ref).abs()
    if kernel is not None and err.numel():
        ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        WORST[kernel] = max(WORST.get(kernel, 0.0), float(ratio.max()))
    bad = ~(err <= bound)                  # NaN counts as bad
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: out %.9g ref %.9g |err| %.3g bound %.3g (%.3gx)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(o[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx]) if float(bound[idx]) > 0 else math.inf))


@contextlib.contextmanager
def launches(*families):
    """launch counts of the given kernel families for everything run inside the block (the library's event-bracketed profiler)"""
    from fbk_fairseq_st_amd import kernels as k      # (tests/test_conv2_gpu.py imports this helper: no use of this module's K)
    counts = {}
    torch.cuda.synchronize()
    k.prof_reset()
    k.prof_enable(1)
    try:
        yield counts
    finally:
        torch.cuda.synchronize()
        for f in families:
            counts[f] = k.prof_read(f)["launches"]
        k.prof_enable(0)
        k.prof_reset()


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(*shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=gen(seed), device=DEV) * scale).to(dtype)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def cdiv(a, b):
    return -(-a // b)


def chunks(B, T2, F2, maxpix=1 << 21):
    """(b, t2a, t2b, p0, p1): runs of output rows of one utterance, contiguous in the pixel index p = (b T2 + t2) F2 + f2"""
    rows = max(1, maxpix // F2)
    for b in range(B):
        for ta in range(0, T2, rows):
            tb = min(T2, ta + rows)
            yield b, ta, tb, (b * T2 + ta) * F2, (b * T2 + tb) * F2


def taps(xp, b, ta, tb, F2):
    """the nine window values of the output pixels (b, ta..tb, all f2) from the zero-padded float64 input xp [B][T+2][F+2]"""
    return torch.stack([xp[b, 2 * ta + kh:2 * tb + kh:2, kw:kw + 2 * F2:2] for kh in range(3) for kw in range(3)], -1).reshape(-1, 9)


def _act(name):
    return K.ACT_GELU if name == "gelu" else K.ACT_RELU


# ------------------------------------------------------------------ conv1 forward
def conv1_inputs(B, T, Fq, C, seed, wscale=0.5):
    """x ~ N(0, 1); w ~ N(0, wscale^2); positive biases (0.05 .. 0.25): a pad pixel counted in the statistics would add relu(bias)"""
    x = randn(B, T, Fq, seed=seed)
    w = randn(C, 9, seed=seed + 1, scale=wscale)
    bias = 0.05 + 0.2 * torch.rand(C, generator=gen(seed + 2), device=DEV)
    return x, w, bias


def fwd_serial(P):
    """per-lane serial count of conv1_mfma_fwd_kernel's statistics: units of 16 pixels over grid * 8 waves (subsample.hip:779)"""
    units = cdiv(P, 16)
    grid = cdiv(units, 8) if units < 8 * 512 else 512
    return cdiv(units, grid * 8)


def check_conv1_fwd(x, w, bias, C, dtype, act, y, pre, sums, what, maxpix=1 << 21):
    """y (and pre) per element, sums[c] / sums[C+c] against float64 sums of the STORED y.
    Statistics depth: the lane's serial count + the 16-lane xor tree (4) (+1 for y*y); then the 8 waves and the atomics in double."""
    B, T, Fq = x.shape
    T2, F2 = (T + 1) // 2, (Fq + 1) // 2
    P, r = B * T2 * F2, rout(dtype)
    xp = Fn.pad(x.double(), (1, 1, 1, 1))
    w64, b64 = w.double().view(C, 9), bias.double()
    yv = y.view(P, C)
    pv = pre.view(P, C) if pre is not None else None
    s1 = torch.zeros(C, dtype=torch.float64, device=DEV)
    s2, a1 = torch.zeros_like(s1), torch.zeros_like(s1)
    for b, ta, tb, p0, p1 in chunks(B, T2, F2, maxpix):
        X = taps(xp, b, ta, tb, F2)
        acc = X @ w64.t() + b64
        e_acc = gam(9) * (X.abs() @ w64.abs().t() + b64.abs())
        del X
        if act == "relu":
            yref = acc.clamp_min(0.0)
            bound = e_acc + r * (yref + e_acc)
        else:
            assert_close(pv[p0:p1], acc, e_acc + r * (acc.abs() + e_acc), what + " pre", "conv1_fwd")
            p64 = d64(pv[p0:p1])
            yref = gelu64(p64)
            bound = 8 * U * p64.abs() + r * (yref.abs() + 8 * U * p64.abs())
        del acc, e_acc
        assert_close(yv[p0:p1], yref, bound, what + " y", "conv1_fwd")
        del yref, bound
        ys = d64(yv[p0:p1])
        s1 += ys.sum(0); s2 += (ys * ys).sum(0); a1 += ys.abs().sum(0)
    d = fwd_serial(P) + 4
    assert_close(sums[:C], s1, 1.01 * (d * U + DSLACK) * a1, what + " sums[c]", "conv1_fwd_sums")
    assert_close(sums[C:], s2, 1.01 * ((d + 1) * U + DSLACK) * s2, what + " sums[C+c]", "conv1_fwd_sums")


SHAPES = [(1, 1, 3), (3, 37, 81), (4, 999, 80)]      # one partial unit; odd F with P % 16 = 1; 5,000 units


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_conv1_fwd_against_fp64(C, act, dtype, shape):
    """NT = C / 16 = 2, 4, 8; (1, 1, 3): P = 2, 14 pad pixels in the one unit; (3, 37, 81): P = 2,337 = 146 * 16 + 1;
    (4, 999, 80): 5,000 units, more than the 4,096 waves of the 512-workgroup grid (subsample.hip:779), two per lane."""
    B, T, Fq = shape
    x, w, bias = conv1_inputs(B, T, Fq, C, seed=10 + C)
    y, sums, pre = K.conv1_fwd(x, w, bias, C, dtype, _act(act))
    assert (pre is not None) == (act == "gelu")
    check_conv1_fwd(x, w, bias, C, dtype, act, y, pre, sums, "conv1_fwd C=%d %s %s %s" % (C, act, dtype, shape))


# ------------------------------------------------------------------ BatchNorm backward + conv1 weight gradient
def bwd_inputs(P, C, dtype, act, seed):
    """stored y (and pre for GELU) with per-channel means and spreads, channel 1 dead (ReLU: y = 0; GELU: pre = -10), channel 2 at
    |mean| = 50 std; dyn ~ N(0, 1).  mean / rstd are the f32 batch statistics of y, as bn_finalize would give them."""
    mu = 0.5 * randn(C, seed=seed)
    sd = 0.5 + torch.rand(C, generator=gen(seed + 1), device=DEV)
    mu[2], sd[2] = 5.0, 0.1
    z = randn(P, C, seed=seed + 2) * sd + mu
    if act == "gelu":
        z[:, 1] = -10.0
        pre = z.to(dtype)
        y = gelu64(pre.double()).to(dtype)
    else:
        pre = None
        z[:, 1] = -1.0
        y = z.clamp_min(0.0).to(dtype)
    y64 = y.double()
    mean = y64.mean(0).float()
    rstd = (y64.var(0, unbiased=False) + 1e-5).rsqrt().float()
    dyn = randn(P, C, seed=seed + 3, dtype=dtype)
    return y, pre, dyn, mean, rstd


def dyn_sums(dyn, y, mean, rstd):
    """sums[c] = sum dyn, sums[C+c] = sum dyn * xhat in double: the values s2t_chan_sums mode 1 estimates (any values will do)"""
    d = dyn.double()
    return torch.cat([d.sum(0), (d * (y.double() - mean.double()) * rstd.double()).sum(0)])


def dpre_ref(dyn, y, pre, mean, rstd, gamma, sums, count, training):
    """float64 dpre of the given (exact) inputs and its per-element error bound e_p (module docstring)"""
    C = y.shape[-1]
    D, Y = d64(dyn), d64(y)
    ka = gamma.double() * rstd.double()
    rs, mu = rstd.double(), mean.double()
    m1 = sums[:C].double() / count if training else torch.zeros_like(ka)
    m2 = sums[C:].double() / count if training else torch.zeros_like(ka)
    r = ka * (D - m1 - (Y - mu) * rs * m2)
    M = (ka * D).abs() + (ka * m2 * rs * Y).abs() + ka.abs() * ((m2 * rs * mu).abs() + m1.abs())
    if pre is None:
        return r * (Y > 0), 8 * U * M
    return r * gelu_grad64(d64(pre)), 18 * U * M


def wgrad_ref(x, dpre_fn, B, T, Fq, C, maxpix=1 << 21):
    """dw [C][9], db [C] = sums over pixels of dpre * window; also sum |dpre| |x|, sum e_p |x| and the same for db.
    dpre_fn(p0, p1) -> (dpre rows p0..p1 in float64, e_p)"""
    T2, F2 = (T + 1) // 2, (Fq + 1) // 2
    xp = Fn.pad(x.double(), (1, 1, 1, 1))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    dw, mw, ew, db, mb, eb = z(C, 9), z(C, 9), z(C, 9), z(C), z(C), z(C)
    for b, ta, tb, p0, p1 in chunks(B, T2, F2, maxpix):
        X = taps(xp, b, ta, tb, F2)
        g, e = dpre_fn(p0, p1)
        dw += g.t() @ X; mw += g.abs().t() @ X.abs(); ew += e.t() @ X.abs()
        db += g.sum(0); mb += g.abs().sum(0); eb += e.sum(0)
    return dw, mw, ew, db, mb, eb


def mfma_depth(P):
    """conv1_bwd_bn_mfma_kernel (subsample.hip:814-832): a lane's MFMA chain adds 16 products per unit over ceil(units / (4 nwg))
    units; the 4 waves (2), chan_partials_f32_kernel's serial count ceil(nwg / 256) and block_sum (6 + 4), the "+=" (1)"""
    units = cdiv(P, 16)
    nwg = cdiv(units, 4) if units < 4 * 1024 else 1024
    return 16 * cdiv(units, 4 * nwg) + 2 + cdiv(nwg, 256) + 10 + 1


def plain_depth(P, C, per_wg):
    """conv1_bwd_kernel / conv1_bwd_bn_kernel: a thread's serial count over ppb pixels in 256 / (C/8) slots (+1: the product, if not
    fused), the lane tree log2(512 / C), the 4 waves, one f32 atomic per workgroup and the existing value"""
    ppb = max(256, cdiv(P, per_wg))
    nblk = cdiv(P, ppb)
    return cdiv(ppb, 2048 // C) + 1 + int(math.log2(512 // C)) + 4 + nblk + 1


def check_wgrad(dw, db, dw0, db0, ref, depth, what, kernel):
    rdw, mw, ew, rdb, mb, eb = ref
    dw0, db0 = d64(dw0), d64(db0)
    assert_close(dw, dw0 + rdw, 1.01 * (ew + depth * U * (mw + ew + dw0.abs()) + DSLACK * mw), what + " dw", kernel)
    assert_close(db, db0 + rdb, 1.01 * (eb + depth * U * (mb + eb + db0.abs()) + DSLACK * mb), what + " db", kernel)


def check_bn_param_grads(dg, dbt, dg0, dbt0, sums, C, what, kernel):
    """dbeta += (float) sums[c], dgamma += (float) sums[C+c] (block 0): the cast and the add round once each"""
    s = sums.double()
    for out, init, add, n in ((dbt, dbt0, s[:C], "dbeta"), (dg, dg0, s[C:], "dgamma")):
        ref = d64(init) + add
        assert_close(out, ref, 2.02 * U * (d64(init).abs() + add.abs()), what + " " + n, kernel)


def run_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, sums, count, training, C, seed):
    """s2t_conv1_bwd_bn into non-zero gradients; returns the outputs and their initial values"""
    g0 = [randn(C, 9, seed=seed), randn(C, seed=seed + 1), randn(C, seed=seed + 2), randn(C, seed=seed + 3)]
    dw, db, dg, dbt = [t.clone() for t in g0]
    K.conv1_bwd_bn(x, dyn.view(-1, C), y.view(-1, C), mean, rstd, gamma, sums, dw, db, dg, dbt, count, training,
                   pre=None if pre is None else pre.view(-1, C))
    return (dw, db, dg, dbt), g0


def check_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, sums, count, training, C, outs, g0, depth, what, kernel, maxpix=1 << 21):
    B, T, Fq = x.shape
    yv, dv = y.view(-1, C), dyn.view(-1, C)
    pv = None if pre is None else pre.view(-1, C)
    fn = lambda p0, p1: dpre_ref(dv[p0:p1], yv[p0:p1], None if pv is None else pv[p0:p1], mean, rstd, gamma, sums, count, training)
    ref = wgrad_ref(x, fn, B, T, Fq, C, maxpix)
    dw, db, dg, dbt = outs
    check_wgrad(dw, db, g0[0], g0[1], ref, depth, what, kernel)
    check_bn_param_grads(dg, dbt, g0[2], g0[3], sums, C, what, kernel)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_conv1_bwd_bn_mfma_against_fp64(C, act, dtype, shape, training):
    """The matrix-core form (P < 2^24, subsample.hip:814) for NT = 2, 4, 8, both activations, training 1 and 0, accumulating into
    non-zero dw / db / dgamma / dbeta through chan_partials_f32_kernel's "+=".  GELU with P % 16 != 0 stages rows past P as zeros,
    whose gelu'(0) = 0.5 would add 0.5 kc to db without the `p0 + pix < P` select (subsample.hip:518).  f32 + GELU + 128 channels
    is the largest dynamic LDS, 4 x 3 x 16 x (512 + 16) = 101,376 bytes."""
    B, T, Fq = shape
    T2, F2 = (T + 1) // 2, (Fq + 1) // 2
    P = B * T2 * F2
    s = 100 + C + 7 * len(act) + (3 if dtype == BF else 0)
    x = randn(B, T, Fq, seed=s)
    y, pre, dyn, mean, rstd = bwd_inputs(P, C, dtype, act, seed=s + 1)
    gamma = 1 + 0.2 * randn(C, seed=s + 2)
    sums = dyn_sums(dyn, y, mean, rstd)
    outs, g0 = run_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, sums, P, training, C, seed=s + 3)
    check_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, sums, P, training, C, outs, g0, mfma_depth(P),
                 "conv1_bwd_bn C=%d %s %s %s training=%d" % (C, act, dtype, shape, training), "conv1_bwd_bn_mfma")


def test_conv1_bwd_bn_on_two_streams():
    """The partials of the matrix-core form live in per-stream scratch (S2T_SCRATCH_CONV1_BWD, subsample.hip:822): the same entry point
    on two streams at once must not share them.  The first call on each stream only allocates the scratch."""
    C, dtype, act, (B, T, Fq) = 64, BF, "gelu", (4, 999, 80)
    P = B * ((T + 1) // 2) * ((Fq + 1) // 2)
    cases = []
    for i in range(2):
        s = 300 + 10 * i
        x = randn(B, T, Fq, seed=s)
        y, pre, dyn, mean, rstd = bwd_inputs(P, C, dtype, act, seed=s + 1)
        gamma = 1 + 0.2 * randn(C, seed=s + 2)
        cases.append((x, y, pre, dyn, mean, rstd, gamma, dyn_sums(dyn, y, mean, rstd)))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for st in streams:
        with torch.cuda.stream(st):
            run_bwd_bn(*cases[0], P, 1, C, seed=400)
    torch.cuda.synchronize()
    res = []
    for i, st in enumerate(streams):
        with torch.cuda.stream(st):
            res.append(run_bwd_bn(*cases[i], P, 1, C, seed=410 + 10 * i))
    torch.cuda.synchronize()
    for i in range(2):
        outs, g0 = res[i]
        check_bwd_bn(*cases[i], P, 1, C, outs, g0, mfma_depth(P), "conv1_bwd_bn stream %d" % i, "conv1_bwd_bn_mfma")


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("shape", [(3, 37, 81), (2, 1, 5), (4, 999, 80)])
def test_conv1_bwd_against_fp64(shape, C, dtype):
    """s2t_conv1_bwd (dpre given): odd F puts the last output column on the right border of the row, where conv1_window_finish
    shifts the triple by one (subsample.hip:93-99); T = 1 masks both outer window rows.  ppb = max(256, ceil(P / 768))
    (subsample.hip:796)."""
    B, T, Fq = shape
    T2, F2 = (T + 1) // 2, (Fq + 1) // 2
    P = B * T2 * F2
    x = randn(B, T, Fq, seed=500 + C)
    dpre = randn(P, C, seed=501 + C, dtype=dtype)
    dw0, db0 = randn(C, 9, seed=502), randn(C, seed=503)
    dw, db = dw0.clone(), db0.clone()
    K.conv1_bwd(x, dpre, dw, db)
    fn = lambda p0, p1: (d64(dpre[p0:p1]), torch.zeros(p1 - p0, C, dtype=torch.float64, device=DEV))
    ref = wgrad_ref(x, fn, B, T, Fq, C)
    check_wgrad(dw, db, dw0, db0, ref, plain_depth(P, C, 768), "conv1_bwd C=%d %s %s" % (C, dtype, shape), "conv1_bwd")


# ------------------------------------------------------------------ both sides of 2^24 pixels
BIG = [((10, 83885, 79), BF, "gelu"),       # P = 2^24 - 16: divmod_small (subsample.hip:182,193) and the matrix-core backward (:814)
       ((1, 838861, 79), BF, "gelu"),       # P = 2^24 + 24, a partial unit: the true-division path and the plain FMA backward
       ((1, 838861, 79), F32, "relu")]


@pytest.mark.parametrize("shape,dtype,act", BIG)
def test_conv1_around_2_pow_24_pixels(shape, dtype, act):
    """32 channels, F = 79: odd F (the shifted window of the plain form) and F2 = 40, not a power of two, so divmod_small's
    correction step is exercised near its limit (n < 2^24).  conv1_fwd, then s2t_conv1_bwd_bn on its outputs with training 1 and 0.
    References run in float64 on the device, in chunks of 2^21 pixels (~1.5 GB of float64 each)."""
    B, T, Fq = shape
    C = 32
    T2, F2 = (T + 1) // 2, (Fq + 1) // 2
    P = B * T2 * F2
    assert P == (1 << 24) - 16 or P == (1 << 24) + 24
    what = "P=%d %s %s" % (P, dtype, act)
    x, w, bias = conv1_inputs(B, T, Fq, C, seed=600)
    y, sums, pre = K.conv1_fwd(x, w, bias, C, dtype, _act(act))
    check_conv1_fwd(x, w, bias, C, dtype, act, y, pre, sums, "conv1_fwd " + what)
    gamma, beta = 1 + 0.2 * randn(C, seed=601), 0.1 * randn(C, seed=602)
    rm, rv, nb = torch.zeros(C, device=DEV), torch.ones(C, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    mean, rstd, _, _ = K.bn_finalize(sums, gamma, beta, rm, rv, nb, P, True)
    dyn = randn(P, C, seed=603, dtype=dtype)
    s = K.chan_sums(y.view(-1, C), C, dyn=dyn, mean=mean, rstd=rstd)
    mfma = P < (1 << 24)
    depth = mfma_depth(P) if mfma else plain_depth(P, C, 512)
    for training in (1, 0):
        outs, g0 = run_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, s, P, training, C, seed=610 + training)
        check_bwd_bn(x, y, pre, dyn, mean, rstd, gamma, s, P, training, C, outs, g0, depth,
                     "conv1_bwd_bn %s training=%d" % (what, training), "conv1_bwd_bn_mfma" if mfma else "conv1_bwd_bn_plain")
        del outs


# ------------------------------------------------------------------ per-channel sums
def chan_depth(P, C):
    """chan_sums_kernel (subsample.hip:856-868): a thread's serial count over ppb rows in NW * 64 / (C/8) slots, then the lane tree
    log2(512 / C); waves and atomics in double"""
    if P >= 256 * 1024:
        ppb, nslot = cdiv(P, 256), 16 * 64 * 8 // C
    else:
        ppb, nslot = max(256, cdiv(P, 256)), 4 * 64 * 8 // C
    return cdiv(ppb, nslot) + int(math.log2(512 // C))


@pytest.mark.parametrize("P", [1, 4097, 262143, 262144])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_chan_sums_both_modes(C, dtype, P):
    """mode 0: (sum y, sum y^2); mode 1: (sum dyn, sum dyn (y - mean) rstd), whose product rounds three times (+3).
    P = 262,143 is the last 4-wave size, 262,144 the first 16-wave one (subsample.hip:856)."""
    y = (randn(P, C, seed=700 + C) * 0.7 + 0.3).to(dtype)
    dyn = randn(P, C, seed=701 + C, dtype=dtype)
    mean, rstd = 0.3 + 0.1 * randn(C, seed=702), 1 + 0.3 * torch.rand(C, generator=gen(703), device=DEV)
    d = chan_depth(P, C)
    what = "chan_sums C=%d %s P=%d" % (C, dtype, P)
    Y, D = d64(y), d64(dyn)
    s = K.chan_sums(y, C)
    assert_close(s[:C], Y.sum(0), 1.01 * (d * U + DSLACK) * Y.abs().sum(0), what + " mode 0 sum y", "chan_sums")
    assert_close(s[C:], (Y * Y).sum(0), 1.01 * ((d + 1) * U + DSLACK) * (Y * Y).sum(0), what + " mode 0 sum y^2", "chan_sums")
    s = K.chan_sums(y, C, dyn=dyn, mean=mean, rstd=rstd)
    t = D * (Y - mean.double()) * rstd.double()
    assert_close(s[:C], D.sum(0), 1.01 * (d * U + DSLACK) * D.abs().sum(0), what + " mode 1 sum dyn", "chan_sums")
    assert_close(s[C:], t.sum(0), 1.01 * ((d + 3) * U + DSLACK) * t.abs().sum(0), what + " mode 1 sum dyn xhat", "chan_sums")


# ------------------------------------------------------------------ BatchNorm finalize
def finalize_ref(sums, gamma, beta, rm, rv, count, training, mom, eps):
    """float64 restatement of bn_finalize_kernel with its bounds.  mean and var are the f32 roundings of the double statistics; the
    double E[y^2] - m^2 itself errs by <= 3 2^-53 (s2/n + m^2) (dv).  rstd = rsqrtf(var + eps): the rounding of var, of the add and
    rsqrtf's ulp: <= (0.5 (dv + 2 u (var + eps)) / (var + eps) + 2 u) rstd.  The momentum updates are three f32 operations on
    values of known size (5 u); scale = gamma rstd and shift = beta - mean gamma rstd round two and three times more."""
    C = gamma.numel()
    g, bt, m0, v0 = gamma.double(), beta.double(), rm.double(), rv.double()
    mf = torch.tensor(mom, dtype=F32).double().item()
    if training:
        m = sums[:C] / count
        s2n = sums[C:] / count
        v = (s2n - m * m).clamp_min(0.0)
        dv = 3 * 2.0 ** -53 * (s2n.abs() + m * m)
        mu, var = m.float().double(), v.float().double()
        unb = (v * (count / (count - 1.0)) if count > 1 else v).float().double()
        new_rm = (1 - mf) * m0 + mf * mu
        new_rv = (1 - mf) * v0 + mf * unb
        b_rm = 5 * U * ((1 - mf) * m0.abs() + mf * mu.abs())
        b_rv = 5 * U * ((1 - mf) * v0.abs() + mf * unb.abs())
    else:
        mu, var, dv = m0, v0, torch.zeros_like(m0)
        new_rm, new_rv, b_rm, b_rv = m0, v0, 0.0, 0.0
    epsf = torch.tensor(eps, dtype=F32).double().item()
    rstd = (var + epsf).rsqrt()
    b_rs = (0.5 * (dv + 2 * U * (var + epsf)) / (var + epsf) + 2 * U) * rstd
    scale, shift = g * rstd, bt - mu * g * rstd
    b_sc = 2 * U * scale.abs() + g.abs() * b_rs
    b_sh = 4 * U * ((mu * g * rstd).abs() + bt.abs()) + (mu * g).abs() * b_rs
    return dict(mean=(mu, 0.0), rstd=(rstd, b_rs), scale=(scale, b_sc), shift=(shift, b_sh), run_mean=(new_rm, b_rm),
                run_var=(new_rv, b_rv))


@pytest.mark.parametrize("case", ["train", "train_no_num_batches", "eval", "count1"])
@pytest.mark.parametrize("C", [4, 32, 96, 128])
def test_bn_finalize_against_fp64(C, case):
    """Channel 0 constant (E[y^2] - m^2 < 0 in double -> clamped to 0, rstd = eps^-1/2), channel 1 dead (sums 0), channel 2 at
    |mean| = 50 std, the rest random.  count 7 makes the unbiased factor n/(n-1) = 7/6 visible in run_var; count = 1 has none.
    Eval reads the running statistics and leaves them and num_batches untouched.  C = 4 and 96 are not multiples of 64."""
    training = case != "eval"
    count = 1 if case == "count1" else 7
    g = gen(800 + C)
    m = torch.randn(C, generator=g, device=DEV, dtype=torch.float64)
    v = torch.rand(C, generator=g, device=DEV, dtype=torch.float64) + 0.1
    m[2], v[2] = 5.0, 0.01
    sums = torch.cat([m * count, (v + m * m) * count])
    sums[0], sums[C] = 3.0 * count, 9.0 * count * (1 - 1e-9)          # var = -9e-9: without the clamp, rstd moves by 4.5e-4
    sums[1 % C], sums[C + 1 % C] = 0.0, 0.0
    if count == 1:
        sums[C + 3 % C] = sums[3 % C] ** 2 + 0.25
    gamma, beta = 1 + 0.2 * randn(C, seed=801), 0.1 * randn(C, seed=802)
    rm0, rv0 = 0.1 * randn(C, seed=803), 0.5 + torch.rand(C, generator=gen(804), device=DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nb = None if case == "train_no_num_batches" else torch.full((1,), 5, dtype=torch.int64, device=DEV)
    out = dict(zip(("mean", "rstd", "scale", "shift"), K.bn_finalize(sums if training else None, gamma, beta, rm, rv, nb, count,
                                                                      training)))
    out.update(run_mean=rm, run_var=rv)
    ref = finalize_ref(sums, gamma, beta, rm0, rv0, count, training, 0.1, 1e-5)
    for k, (r, b) in ref.items():
        assert_close(out[k], r, b, "bn_finalize C=%d %s %s" % (C, case, k), "bn_finalize")
    if not training:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    if nb is not None:
        assert int(nb) == (6 if training else 5)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_bn_finalize_rstd_of_a_channel_far_from_zero(dtype):
    """At (4, 999, 80), 64 channels: channel 5 of conv1's output has |mean| ~ 50 std (small weights, bias 1).  Its variance comes
    from the f32 partials of conv1_fwd as E[y^2] - m^2: the sums err by <= d u sum y and (d + 1) u sum y^2 (d = lane count + 4,
    check_conv1_fwd), so var errs by <= (d + 1) u (sum y^2 / n) + 2 |m| d u (sum |y| / n), and rstd by half that over var, plus the
    finalize rounding.  The measured error is printed; the reference is the two-pass float64 variance of the stored y."""
    B, T, Fq, C = 4, 999, 80, 64
    x, w, bias = conv1_inputs(B, T, Fq, C, seed=900)
    w[5] = 0.0067 * torch.sign(w[5])
    bias[5] = 1.0
    y, sums, _ = K.conv1_fwd(x, w, bias, C, dtype, K.ACT_RELU)
    P = y.numel() // C
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, rstd, _, _ = K.bn_finalize(sums, gamma, beta, rm, rv, None, P, True)
    Y = d64(y.view(P, C))
    m = Y.mean(0)
    var = ((Y - m) ** 2).mean(0)
    assert float(m[5] / var[5].sqrt()) > 30
    d = fwd_serial(P) + 4
    dvar = (d + 1) * U * (Y * Y).mean(0) + 2 * m.abs() * d * U * Y.abs().mean(0)
    ref = (var + 1e-5).rsqrt()
    bound = (0.5 * dvar / (var + 1e-5) + 4 * U) * ref
    assert_close(rstd, ref, bound, "rstd after conv1_fwd %s" % dtype, "bn_finalize_rstd")
    assert_close(mean, m, d * U * Y.abs().mean(0) + U * m.abs(), "mean after conv1_fwd %s" % dtype, "bn_finalize_rstd")
    rel = float((d64(rstd) - ref).abs()[5] / ref[5])
    print("\nrstd of the |mean| = %.1f std channel, %s: relative error %.3g (bound %.3g)"
          % (float(m[5] / var[5].sqrt()), dtype, rel, float(bound[5] / ref[5])))
    assert rel < 1e-3


# ------------------------------------------------------------------ BatchNorm apply
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C,P", [(32, 3), (64, 1001), (128, 70313)])
def test_bn_apply_against_fp64(C, P, dtype):
    """yn = y scale + shift: one fma or a product and an add (2 u of |y scale| + |shift|), then the rounding to the dtype.
    128 x 70,313 = 9,000,064 elements: 1,125,008 vectors of 8 over a grid capped at 4,096 x 256 (subsample.hip:765), so threads loop
    and rely on the grid stride being a multiple of C/8."""
    y = (randn(P, C, seed=1000 + C) * 2 + 0.5).to(dtype)
    scale, shift = 0.5 + torch.rand(C, generator=gen(1001), device=DEV), randn(C, seed=1002)
    yn = K.bn_apply(y, scale, shift)
    Y = d64(y)
    ref = Y * scale.double() + shift.double()
    e = 2 * U * ((Y * scale.double()).abs() + shift.double().abs())
    assert_close(yn, ref, e + rout(dtype) * (ref.abs() + e), "bn_apply C=%d P=%d %s" % (C, P, dtype), "bn_apply")


def test_bn_apply_refusals():
    """C = 24 (256 % (C/8) != 0), n % C != 0 and p_drop = 1 are refused (subsample.hip:886) and leave the output untouched.  Every
    buffer is big enough for what the kernel would touch without the guard: a regressed guard gives a wrong answer, never an
    out-of-bounds access."""
    n = 24 * 64
    y = randn(n, seed=1100)
    scale, shift = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    lib = K._lib()
    for C, nn, p in ((24, n, 0.0), (64, n - 8, 0.0), (64, n, 1.0)):
        yn = torch.full((n,), 7.0, device=DEV)
        rc = lib.s2t_bn_apply(L.F32, L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(yn), nn, C, p, 0, L.stream())
        torch.cuda.synchronize()
        assert rc == EINVAL, (C, nn, p, rc)
        assert bool((yn == 7.0).all()), (C, nn, p)


# ------------------------------------------------------------------ BatchNorm backward apply
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("C,P", [(32, 37), (64, 2337), (128, 20000)])
def test_bn_bwd_apply_against_fp64(C, P, act, dtype, training):
    """dpre = act' gamma rstd (dyn - m1 - xhat m2), xhat = (y - mean) rstd: five roundings on the magnitudes |k1| (|dyn| + |m1| +
    |xhat m2|) (8 u with m1, m2's casts), GELU's derivative as in the module docstring, then the output rounding; with training = 0,
    m1 = m2 = 0.  dgamma / dbeta accumulate into non-zero values."""
    s = 1200 + C + 5 * len(act) + (1 if dtype == BF else 0)
    y, pre, dyn, mean, rstd = bwd_inputs(P, C, dtype, act, seed=s)
    gamma = 1 + 0.2 * randn(C, seed=s + 5)
    sums = dyn_sums(dyn, y, mean, rstd)
    dg0, dbt0 = randn(C, seed=s + 6), randn(C, seed=s + 7)
    dg, dbt = dg0.clone(), dbt0.clone()
    dpre = K.bn_bwd_apply(dyn, y, mean, rstd, gamma, sums, dg, dbt, P, training, pre=pre)
    k1, rs, mu = gamma.double() * rstd.double(), rstd.double(), mean.double()
    m1 = sums[:C] / P if training else torch.zeros_like(k1)
    m2 = sums[C:] / P if training else torch.zeros_like(k1)
    D, Y = d64(dyn), d64(y)
    xh = (Y - mu) * rs
    r = k1 * (D - m1 - xh * m2)
    e = 8 * U * k1.abs() * (D.abs() + m1.abs() + (xh * m2).abs())
    if pre is None:
        ref, e = r * (Y > 0), e
    else:
        ref, e = r * gelu_grad64(d64(pre)), 1.13 * e + 8 * U * r.abs()
    what = "bn_bwd_apply C=%d P=%d %s %s training=%d" % (C, P, act, dtype, training)
    assert_close(dpre, ref, e + rout(dtype) * (ref.abs() + e), what, "bn_bwd_apply")
    check_bn_param_grads(dg, dbt, dg0, dbt0, sums, C, what, "bn_bwd_apply")


# ------------------------------------------------------------------ the subsampler chain through the engine
def build_model(C, act, feat, dtype):
    """a small model the way tests/test_engine_gpu.py builds one, with the subsampler's channels, activation and feature count;
    the subsampler's dropout off (tests/test_model_gpu.py parity mode)"""
    from fbk_fairseq_st_amd import conv_transformer, criterions, tasks  # noqa: F401
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.registry import apply_arch, namespace
    a = namespace(arch="conv_transformer", criterion="ctc_multi_loss", underlying_criterion="label_smoothed_cross_entropy",
                  label_smoothing=0.1, ctc_compress_out=True, ctc_encoder_layer=1, ctc_weight=1.0, encoder_embed_dim=128, encoder_ffn_embed_dim=256,
                  encoder_attention_heads=2, encoder_layers=1, decoder_layers=1, decoder_embed_dim=128, decoder_ffn_embed_dim=256,
                  decoder_attention_heads=2, no_attn_2d=True, input_feat_per_channel=feat, dropout=0.0, attention_dropout=0.0,
                  activation_dropout=0.0, relu_dropout=0.0, activation_fn=act, sentence_avg=False, seed=7,
                  encoder_convolutions="[(%d, 3, 3), (%d, 3, 3)]" % (C, C))
    apply_arch(a)
    tgt, src = Dictionary.synthetic(100), Dictionary.synthetic(50)
    src.add_symbol("<ctc_blank>")
    task = tasks.SpeechTranslationCTCTask(a, tgt, src)
    torch.manual_seed(3)
    model, crit = task.build_model(a), task.build_criterion(a)
    model.hp.sub_dropout = 0.0
    model.materialize(DEV, dtype, extra=crit.arena_params())
    assert model.hp.conv_ch == C and model.hp.act == act
    return model


SUB = ["encoder.convolutions.0.weight", "encoder.convolutions.0.bias", "encoder.convolutions.1.weight", "encoder.convolutions.1.bias",
       "encoder.bn.0.weight", "encoder.bn.0.bias", "encoder.bn.1.weight", "encoder.bn.1.bias", "encoder.fc3.weight", "encoder.fc3.bias"]


def product_ref(X, W, bias):
    """float64 X W^T + b and the accumulation bound 4 K u (|X| |W|^T + |b|) of tests/test_routes_gpu.py's Gemm (any order, split-K
    and the bias add; bf16 x bf16 and the f32 MFMA products are exact in f32)"""
    acc = X @ W.t() + bias
    return acc, 4 * X.shape[1] * U * (X.abs() @ W.abs().t() + bias.abs())


def check_act_out(out, pre, acc, e_acc, act, dtype, what, kernel="chain"):
    """out = act(acc) stored (and pre = acc stored for GELU).  GELU's value may come from the f32 accumulator or from the stored
    pre-activation: the bound takes the rounding of pre (r |acc|) as one more input error, slope <= 1.13, and gelu_f's 8 u |x|.
    `kernel`: the name the worst ratio is recorded under (tests/test_conv2_gpu.py passes its own)."""
    r = rout(dtype)
    if act == "relu":
        ref = acc.clamp_min(0.0)
        assert_close(out, ref, e_acc + r * (ref.abs() + e_acc), what, kernel)
        return
    assert_close(pre, acc, e_acc + r * (acc.abs() + e_acc), what + " pre", kernel)
    ref = gelu64(acc)
    e = 1.13 * (e_acc + r * (acc.abs() + e_acc)) + 8 * U * (acc.abs() + e_acc)
    assert_close(out, ref, e + r * (ref.abs() + e), what, kernel)


def check_bn_stage(y, mean, rstd, gamma, beta, yn, bufs0, bufs, pfx, depth, dtype, what):
    """batch statistics of the STORED y: mean, rstd (the f32-partial bound of test_bn_finalize_rstd_of_a_channel_far_from_zero),
    the momentum updates of the running buffers (unbiased variance), num_batches; then yn = y scale + shift from the given mean / rstd"""
    n = y.shape[0]
    Y = d64(y)
    m = Y.mean(0)
    var = ((Y - m) ** 2).mean(0)
    dm = depth * U * Y.abs().mean(0)
    dvar = (depth + 1) * U * (Y * Y).mean(0) + 2 * m.abs() * dm
    assert_close(mean, m, dm + U * m.abs(), what + " mean", "chain")
    rs = (var + 1e-5).rsqrt()
    assert_close(rstd, rs, (0.5 * dvar / (var + 1e-5) + 4 * U) * rs, what + " rstd", "chain")
    mom = torch.tensor(0.1, dtype=F32).double().item()
    rm0, rv0 = d64(bufs0[pfx + "running_mean"]), d64(bufs0[pfx + "running_var"])
    unb = var * n / (n - 1)
    assert_close(bufs[pfx + "running_mean"], (1 - mom) * rm0 + mom * m,
                 5 * U * ((1 - mom) * rm0.abs() + mom * m.abs()) + mom * (dm + U * m.abs()), what + " running_mean", "chain")
    assert_close(bufs[pfx + "running_var"], (1 - mom) * rv0 + mom * unb,
                 5 * U * ((1 - mom) * rv0.abs() + mom * unb) + mom * (dvar + U * var) * n / (n - 1), what + " running_var", "chain")
    assert int(bufs[pfx + "num_batches_tracked"]) == int(bufs0[pfx + "num_batches_tracked"]) + 1
    sc = gamma.double() * rstd.double()
    ref = (Y - mean.double()) * sc + beta.double()
    e = 4 * U * ((Y * sc).abs() + (mean.double() * sc).abs() + beta.double().abs())
    assert_close(yn, ref, e + rout(dtype) * (ref.abs() + e), what + " normalised", "chain")


CHAIN = [(C, dtype, act, feat) for C in (32, 64, 128) for dtype in (F32, BF) for act, feat in (("relu", 80), ("gelu", 81))] + \
        [(64, BF, "relu", 81), (64, BF, "gelu", 80)] + \
        [(64, BF, act, feat) for feat in (89, 91, 95, 97) for act in ("relu", "gelu")]      # F2 = 45, 46, 48, 49: the direct kernels' limits


@pytest.mark.parametrize("C,dtype,act,feat", CHAIN)
def test_subsample_chain_against_fp64(C, dtype, act, feat):
    """Engine.subsample_fwd (training) stage by stage against float64 of the previous STORED stage, then subsample_bwd +
    flush_wgrad against float64 autograd of oracle.s2t_ref.subsample run in double.
    Routes: bf16 with 64 channels takes the direct conv2 kernels of csrc/conv2.hip (engine.py:360,444,457); every other case the
    implicit GEMM over the row maps, the nine gathered TN GEMMs for the weight gradient and the four parity-class products for
    the data gradient.  permute_conv_w mode 0 (w2p) is checked bit for bit; fc3's reference flattens channel-major with the master
    weight (conv_transformer.py:225-226), so a wrong permute_cf order fails h3, and modes 1 / 2 of the two permutes are checked
    through the gradients.
    The three direct kernels have three limits: the forward takes F2 <= 48 (conv2.hip:142), the data gradient F2 <= 47 (conv2.hip:273),
    the weight gradient F2 <= 45 (subsample.hip:1100), and the engine falls back per kernel.  feat = 89 / 91 / 95 / 97 (F2 = 45 / 46 /
    48 / 49) run all three direct; the weight gradient gathered; only the forward direct; none direct -- a step that mixes direct and
    gathered kernels on the same tensors.  Which route ran is asserted: conv2_fwd / conv2_dgrad record a launch family, the weight
    gradient records none and is probed with a direct K.conv2_wgrad call at the step's geometry.
    Gradient bounds, normwise per parameter: f32, the README's parity contract 1e-3 of |g_ref|.  bf16: every stored activation (y1,
    y1n, z2, z2n, h3), both compute-dtype weights (w2p, w3p) and every stored gradient (dh3, dz2n, dpre2, dy1n) is rounded to bf16
    once: 12 roundings of relative size <= 2^-8 on the path to a gradient, 12 x 2^-8 = 0.047 -> 0.05, relative to the sums of
    |terms| (ref_grads), not to |g_ref|: the BatchNorm backward cancels most of each sum (|terms| / |g| is 3 to 100 here)."""
    from oracle import s2t_ref
    model = build_model(C, act, feat, dtype)
    eng, A = model.engine, model.arena
    B, T = 3, 61
    lens = torch.tensor([T, T - 13, T - 40])
    x = randn(B, T, feat, seed=1300 + C)
    for b in range(B):
        x[b, int(lens[b]):] = 0.0
    len4 = ((lens + 1) // 2 + 1) // 2
    bufs0 = {k: v.clone() for k, v in eng.bn_buffers.items()}
    A.zero_grad()
    with launches("conv2_fwd", "gemm_gather") as ran:
        xe, c = eng.subsample_fwd(x, len4.to(torch.int32).to(DEV), True, 5)
    T2, F2, T4, F4 = c["T2"], c["F2"], c["T4"], c["F4"]
    direct = C == 64 and dtype == BF
    assert (ran["conv2_fwd"], ran["gemm_gather"]) == ((1, 0) if direct and F2 <= 48 else (0, 1)), (F2, ran)
    what = "chain C=%d %s %s F=%d" % (C, dtype, act, feat)
    Pm = lambda n: A.p(n)
    # conv1 + BN1
    xp = Fn.pad(x.double(), (1, 1, 1, 1))
    X1 = torch.cat([taps(xp, b, 0, T2, F2) for b in range(B)])
    acc, e = product_ref(X1, Pm("encoder.convolutions.0.weight").double().view(C, 9), Pm("encoder.convolutions.0.bias").double())
    check_act_out(c["y1"].view(-1, C), None if c["pre1"] is None else c["pre1"].view(-1, C), acc, e, act, dtype, what + " y1")
    check_bn_stage(c["y1"].view(-1, C), c["mean1"], c["rstd1"], Pm("encoder.bn.0.weight"), Pm("encoder.bn.0.bias"), c["y1n"].view(-1, C),
                   bufs0, eng.bn_buffers, "encoder.bn.0.", fwd_serial(B * T2 * F2) + 4, dtype, what + " bn0")
    # conv2 + BN2: w2p = permute_conv_w mode 0, bit for bit; the reference uses the master weight rounded to the compute dtype
    w2 = Pm("encoder.convolutions.1.weight").to(dtype).double()                           # [co][ci][kh][kw]
    assert torch.equal(c["w2p"], Pm("encoder.convolutions.1.weight").view(C, C, 9).permute(0, 2, 1).reshape(C, 9 * C).to(dtype))
    Yp = Fn.pad(d64(c["y1n"]).view(B, T2, F2, C), (0, 0, 1, 1, 1, 1))
    X2 = torch.stack([Yp[:, kh:kh + 2 * T4:2, kw:kw + 2 * F4:2, :] for kh in range(3) for kw in range(3)], 3)
    X2 = X2.permute(1, 0, 2, 3, 4).reshape(T4 * B * F4, 9 * C)                            # rows (t4, b, f4), columns (tap, ci)
    acc, e = product_ref(X2, w2.permute(0, 2, 3, 1).reshape(C, 9 * C), Pm("encoder.convolutions.1.bias").double())
    check_act_out(c["z2"].view(-1, C), None if c["pre2"] is None else c["pre2"].view(-1, C), acc, e, act, dtype, what + " z2")
    check_bn_stage(c["z2"].view(-1, C), c["mean2"], c["rstd2"], Pm("encoder.bn.1.weight"), Pm("encoder.bn.1.bias"), c["z2n"].view(-1, C),
                   bufs0, eng.bn_buffers, "encoder.bn.1.", chan_depth(T4 * B * F4, C), dtype, what + " bn1")
    # fc3 on the channel-major flatten, master weight rounded to the compute dtype; positions
    Z = d64(c["z2n"]).view(T4 * B, F4, C).permute(0, 2, 1).reshape(T4 * B, C * F4)
    acc, e = product_ref(Z, Pm("encoder.fc3.weight").to(dtype).double(), Pm("encoder.fc3.bias").double())
    check_act_out(c["h3"], c["pre3"], acc, e, act, dtype, what + " h3")
    tab = d64(eng.table(T4 + 1, 0))
    t = torch.arange(T4).view(T4, 1)
    pos = torch.where(t < len4.view(1, B), t + 1, torch.zeros_like(t)).to(DEV)
    ref = d64(c["h3"]).view(T4, B, -1) + tab[pos]
    e = U * ref.abs() + U * (d64(c["h3"]).view(T4, B, -1).abs() + tab[pos].abs())
    assert_close(xe, ref, e + rout(dtype) * (ref.abs() + e), what + " xe", "chain")
    # backward against float64 autograd of the reference subsampler
    dx = randn(T4 * B, model.hp.D, seed=1400 + C, dtype=dtype)
    with launches("conv2_dgrad", "gemm_gather") as ran:
        eng.subsample_bwd(c, dx)
        eng.flush_wgrad()
    wgrad_direct = K.conv2_wgrad(torch.zeros(T4 * B * F4, C, dtype=dtype, device=DEV), c["y1n"].view(-1, C),
                                 torch.zeros(C, 9 * C, device=DEV), B, T2, F2, C)
    assert wgrad_direct == (direct and F2 <= 45), (F2, wgrad_direct)
    # gathered launches: nine per-tap products of the weight gradient, one per pixel-parity class of the data gradient
    # (F2 >= 2 and T2 >= 2 here: all four classes have pixels)
    want = ((1, 0) if direct and F2 <= 47 else (0, 4))
    assert (ran["conv2_dgrad"], ran["gemm_gather"]) == (want[0], want[1] + (0 if wgrad_direct else 9)), (F2, ran)
    W = {n: A.p(n).detach().double().cpu().requires_grad_(True) for n in SUB}
    for n in ("encoder.bn.0.", "encoder.bn.1."):
        W[n + "running_mean"], W[n + "running_var"] = bufs0[n + "running_mean"].double().cpu(), bufs0[n + "running_var"].double().cpu()
    cfg = s2t_ref.default_cfg(D=model.hp.D, conv_ch=C, feat=feat, act=act)
    ref, mag = ref_grads(s2t_ref, W, cfg, x.double().cpu(), lens, dx.double().cpu().view(T4, B, -1))
    for n in SUB:
        g = d64(A.g(n), "cpu").view(-1)
        err = float((g - ref[n].view(-1)).norm())
        if dtype == F32:
            bound, of = 1e-3 * float(ref[n].norm()), "|g_ref|"
        else:
            bound, of = 0.05 * float(mag[n].norm()), "|sum of |terms||"
        WORST["chain_grad_" + ("f32" if dtype == F32 else "bf16")] = max(WORST.get("chain_grad_" + ("f32" if dtype == F32 else "bf16"), 0.0),
                                                                         err / bound)
        assert err <= bound, "%s grad %s: normwise error %.3g > %.3g (%s)" % (what, n, err, bound, of)


def ref_grads(s2t_ref, W, cfg, x, lens, dx):
    """float64 autograd of oracle.s2t_ref.subsample, and per parameter the same sums over |terms| (what the rounding of each term
    is relative to): conv weights sum |dpre| |input window|, biases sum |dpre|, BatchNorm dgamma sum |dyn xhat| and dbeta sum |dyn|.
    The convolutions' and fc3's outputs are recorded on the way (their gradients are dpre), the BatchNorm outputs come from `trace`."""
    outs, conv2d, linear = [], Fn.conv2d, Fn.linear

    def rec(f):
        def g(*a, **k):
            o = f(*a, **k)
            o.retain_grad()
            outs.append((a[0], o))
            return o
        return g
    Fn.conv2d, Fn.linear = rec(conv2d), rec(linear)
    tr = {}
    try:
        out, _, _ = s2t_ref.subsample(W, cfg, x, lens, training=True, trace=tr)
    finally:
        Fn.conv2d, Fn.linear = conv2d, linear
    assert len(outs) == 3
    for k in ("conv0", "conv1"):
        tr[k].retain_grad()
    out.backward(dx)
    ref = {n: W[n].grad for n in SUB}
    mag = {}
    for i in range(2):
        a, o = outs[i]
        w = W["encoder.convolutions.%d.weight" % i]
        mag["encoder.convolutions.%d.weight" % i] = torch.nn.grad.conv2d_weight(a.detach().abs(), w.shape, o.grad.abs(), stride=2, padding=1)
        mag["encoder.convolutions.%d.bias" % i] = o.grad.abs().sum((0, 2, 3))
        yb = tr["conv%d" % i]
        xhat = (yb.detach() - W["encoder.bn.%d.bias" % i].detach()[None, :, None, None]) / W["encoder.bn.%d.weight" % i].detach()[None, :, None, None]
        mag["encoder.bn.%d.weight" % i] = (yb.grad * xhat).abs().sum((0, 2, 3))
        mag["encoder.bn.%d.bias" % i] = yb.grad.abs().sum((0, 2, 3))
    a, o = outs[2]
    a2, g2 = a.detach().abs().reshape(-1, a.shape[-1]), o.grad.abs().reshape(-1, o.shape[-1])
    mag["encoder.fc3.weight"], mag["encoder.fc3.bias"] = g2.t() @ a2, g2.sum(0)
    return ref, mag
