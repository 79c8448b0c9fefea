"""The update tail and the element-wise helpers against float64 / exact references: s2t_grad_norm_clip, s2t_grad_norm_clip_div,
s2t_adam_step (both kernel forms), s2t_cast, s2t_scale_by_device_scalar (csrc/norm_optim.hip) and s2t_add_inplace, s2t_act_bwd,
s2t_dropout (csrc/loss_embed.hip).

Every reference is computed on the CPU from the exact values the kernel was given (bf16 widened exactly, hyper-parameters as the f32
the C ABI passes).  Every tolerance is exact equality, a bound whose derivation stands next to it (u = 2^-24, one f32 rounding), or a
multiple of a CPU float32 yardstick measured against fp64 in the same test."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

K = None
L = None


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield


DEV = "cuda"
U = 2.0 ** -24                    # unit roundoff of f32
UB = 2.0 ** -8                    # one rounding to bf16's 8 significant bits, as the bounds below state it
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
HALF = {F32: U, BF: UB}                      # unit roundoff of the type: half an ulp, relative to the value
GUARD = 77.0
SIZES = [1, 255, 256, 257, 4096 * 256 + 5]   # around one workgroup, and past the 4,096-workgroup cap of the grid-stride loops


def f32(v):
    """the f32 value a float argument of the C ABI arrives as"""
    return float(np.float32(v))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).numpy()


def d64(t):
    return t.detach().cpu().to(torch.float64)


def rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def place(host, lead):
    """host -> a device view that starts `lead` elements into an allocation filled with GUARD (lead 8: 16-byte aligned; lead 1: not)"""
    n = host.numel()
    buf = torch.full((n + 2 * lead,), GUARD, dtype=host.dtype, device=DEV)
    v = buf[lead:lead + n]
    v.copy_(host.to(DEV))
    assert (v.data_ptr() % 16 == 0) == (lead % 8 == 0)
    return v, buf


def guards_intact(buf, lead, what):
    n = buf.numel() - 2 * lead
    want = bits(torch.full((lead,), GUARD, dtype=buf.dtype))
    assert np.array_equal(bits(buf[:lead]), want) and np.array_equal(bits(buf[lead + n:]), want), what + ": wrote outside its range"


# ------------------------------------------------------------------ B1: gradient norm and clip coefficient
@pytest.mark.parametrize("mag", [1e-3, 1e3])
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1023, 2 ** 20 + 3, 3 * 10 ** 7 + 1])
def test_grad_norm_and_clip_coefficient(n, mag):
    """||g||_2 over f32 g against fp64, for the plain and the divisor entry points.  n = 3e7 + 1 > 2,048 x 256 x 4: the grid-stride
    loop of sumsq_kernel turns.  Bounds: the kernel squares in f32 (u), adds the squares in pairs in f32 (u) and continues in double,
    so acc_ws[0] is within 2 u of the fp64 sum of squares (asserted: 4 u); sqrt halves that, and the conversion to f32, the product
    with scale, (scale / divisor rounded to f32), gn + 1e-6, the division and the last product each round once: at most six f32
    roundings on out2[0] and on out2[1] (asserted: 16 u)."""
    lib = K._lib()
    g = rnd(max(n, 4), seed=n % 1000 + 1, scale=mag)[:max(n, 4)]
    gd = g.to(DEV)                                                  # n = 0 still passes a valid pointer: the call must not read it
    ss = float((g[:n].double() ** 2).sum())
    ws = torch.zeros(1, dtype=torch.float64, device=DEV)
    out2 = torch.zeros(2, device=DEV)
    seen_above = False
    for scale, max_norm, div in itertools.product((1.0, 1.0 / 15), (0.0, 0.5, 1e9), (None, 0.25, 1.0, 4096.0)):
        ws.fill_(-1.0); out2.fill_(float("nan"))
        if div is None:
            rc = lib.s2t_grad_norm_clip(L.ptr(gd), n, L.ptr(ws), scale, max_norm, L.ptr(out2), L.stream())
        else:
            dv = torch.tensor([div], dtype=torch.float64, device=DEV)
            rc = lib.s2t_grad_norm_clip_div(L.ptr(gd), n, L.ptr(ws), scale, L.ptr(dv), max_norm, L.ptr(out2), L.stream())
        assert rc == 0
        acc, (gn, coef) = float(ws.cpu()), out2.cpu().tolist()
        s = f32(scale) if div is None else f32(np.float64(f32(scale)) / max(div, 1.0))       # a divisor below 1 is clamped to 1
        gn64 = s * math.sqrt(ss)
        tag = (n, mag, scale, max_norm, div)
        assert abs(acc - ss) <= 4 * U * ss, tag
        assert abs(gn - gn64) <= 16 * U * gn64, tag
        if max_norm == 0.0:
            assert np.float32(coef) == np.float32(s), tag                                   # no clipping: exactly `scale`
            continue
        ratio = f32(max_norm) / (gn64 + f32(1e-6))
        assert abs(ratio - 1.0) > 1e-3, "a case on the clipping threshold decides nothing"
        seen_above = seen_above or (max_norm == 0.5 and ratio < 1.0)
        c64 = s * min(ratio, 1.0)
        assert abs(coef - c64) <= 16 * U * c64, tag
        if max_norm == 1e9:
            assert ratio > 1.0 and np.float32(coef) == np.float32(s), tag                   # a norm below max_norm: exactly `scale`
        if n == 0:
            assert gn == 0.0 and np.float32(coef) == np.float32(s), tag
    if n >= 1023 and mag == 1e3:
        assert seen_above, "max_norm = 0.5 must meet a norm above it"


# ------------------------------------------------------------------ B2: Adam, both kernel forms
def adam_ref(p, g, m, v, mult, lr, b1, b2, eps, wd, step):
    """adam_one (norm_optim.hip) in fp64 on the f32 inputs and the f32-rounded hyper-parameters; returns the new p, m, v and the
    per-element bounds (u = 2^-24):
      m: g' = g mult rounds once (exact when mult is NULL), (1 - b1) g' once, the sum once; b1 m once and the sum once:
         3 u (|b1 m| + |(1 - b1) g'|).
      v: b2 v and the sum: 2 u on the first term.  (1 - b2) g' g' is two products and the sum: 3 u when g' is exact (mult NULL),
         inside the stated 4 u (|b2 v| + |(1 - b2) g'^2|).  With a clip coefficient g' carries its own rounding and enters squared:
         2 u more, 5 u on the second term -- the counting that replaces the stated 4 there.
      p: the weight-decay step rounds wd lr, its product with p (both relative to wd lr |p| <= 1e-5 |p|) and the subtraction (u |p|);
         the last subtraction rounds once more (u (|p| + |D|)): 2 u |p| + u |D|.  D = step_size m' / (sqrt(v') + eps): sqrt(v')
         carries half of v's 5 u and sqrtf's own rounding (<= 2 u), the sum with eps, the product step_size m' and the division
         round once each: 2.5 + 2 + 1 + 1 + 1 + 1 (the subtraction's share) = 8.5 u |D|, asserted as 13 u |D|.  m' adds its own
         3 u: relative to |m'| where b1 m and (1 - b1) g' have one sign -- the stated u (2 |p| + 16 |D|) -- and relative to the
         magnitudes it is made of where they cancel, so that part is written as step_size bound_m / (sqrt(v') + eps)."""
    lrf, b1f, b2f, epsf, wdf = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    ss = f32(lrf * math.sqrt(1.0 - b2f ** step) / (1.0 - b1f ** step))               # as s2t_adam_step computes it, in double
    omb1, omb2 = float(np.float32(1.0) - np.float32(b1)), float(np.float32(1.0) - np.float32(b2))
    gp = g * (1.0 if mult is None else f32(mult))
    t1m, t2m = b1f * m, omb1 * gp
    t1v, t2v = b2f * v, omb2 * gp * gp
    mn, vn = t1m + t2m, t1v + t2v
    p1 = p - (wdf * lrf) * p if wd != 0.0 else p
    den = np.sqrt(vn) + epsf
    delta = ss * mn / den
    pn = p1 - delta
    bm = 3 * U * (np.abs(t1m) + np.abs(t2m))
    bv = U * (4 * np.abs(t1v) + (4 if mult is None else 5) * np.abs(t2v))
    bp = U * (2 * np.abs(p) + 13 * np.abs(delta)) + ss * bm / den
    return pn, mn, vn, bm, bv, bp


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1021, 2 ** 20 + 3])
@pytest.mark.parametrize("form", ["vector", "elementwise_offset_views", "elementwise_unaligned_shadow"])
def test_adam_both_forms(form, n):
    """adam_kernel<true> on 16-byte aligned tensors and adam_kernel<false> on views one element into their allocations / with a
    shadow that is only 2-byte aligned (the sub-ranges frozen parameters leave), over {mult2 NULL, given} x {shadow NULL, given} x
    {wd 0, 1e-2} x step {1, 7, 1e6}, element by element against adam_ref; the elements around the updated range stay untouched"""
    lead = 1 if form == "elementwise_offset_views" else 8
    lead_sh = 8 if form == "vector" else 1
    p0, g0, m0, v0 = rnd(n, 1), rnd(n, 2, 0.1), rnd(n, 3, 0.01), torch.rand(n, generator=torch.Generator().manual_seed(4)) * 1e-3
    zero, tiny = ([], []) if n < 3 else ([n - 1], [1]) if n < 16 else ([5, 6, 7, n - 1], [9, 10, 11, n - 2])
    for i in zero:
        g0[i] = m0[i] = v0[i] = 0.0                                 # must stay finite, unchanged but for weight decay
    for k, i in enumerate(tiny):
        v0[i] = 1e-30
        if k < 2:
            g0[i] = 0.0                                             # v' stays ~1e-30: sqrt(v') far below eps
    lr, b1, b2, eps = 1e-3, 0.9, 0.98, 1e-8
    for mult, with_shadow, wd, step in itertools.product((None, 0.37), (False, True), (0.0, 1e-2), (1, 7, 10 ** 6)):
        if form == "elementwise_unaligned_shadow" and not with_shadow:
            continue
        tag = "%s n=%d mult=%s shadow=%s wd=%g step=%d" % (form, n, mult, with_shadow, wd, step)
        (p, pb), (g, gb), (m, mb), (v, vb) = [place(t, lead) for t in (p0, g0, m0, v0)]
        sh, shb = place(torch.full((n,), 3.0, dtype=BF), lead_sh) if with_shadow else (None, None)
        if sh is not None:
            assert (sh.data_ptr() % 8 == 0) == (form == "vector")
        mult2 = None if mult is None else torch.tensor([123.0, mult], device=DEV)      # [0] is the norm: a decoy here
        K.adam_step(p, g, m, v, sh, mult2, lr, b1, b2, eps, wd, step)
        torch.cuda.synchronize()
        pn, mn, vn, bm, bv, bp = adam_ref(p0.double().numpy(), g0.double().numpy(), m0.double().numpy(), v0.double().numpy(),
                                          mult, lr, b1, b2, eps, wd, step)
        for name, got, ref, bound in (("m", m, mn, bm), ("v", v, vn, bv), ("p", p, pn, bp)):
            got = d64(got).numpy()
            assert np.isfinite(got).all(), tag
            err = np.abs(got - ref)
            bad = err > bound
            assert not bad.any(), (tag, name, int(bad.sum()), int(np.argmax(err - bound)), float((err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(bits(g), bits(g0)), tag
        for i in zero:
            assert float(m[i]) == 0.0 and float(v[i]) == 0.0, tag
            if wd == 0.0:
                assert np.array_equal(bits(p[i:i + 1]), bits(p0[i:i + 1])), tag
        for name, buf in (("p", pb), ("g", gb), ("m", mb), ("v", vb)):
            guards_intact(buf, lead, tag + " " + name)
        if sh is not None:
            assert np.array_equal(bits(sh), bits(p.cpu().to(BF))), tag + ": shadow != bf16(p)"
            guards_intact(shb, lead_sh, tag + " shadow")


# ------------------------------------------------------------------ B3: casts
def special_f32():
    """halfway cases of both parities and signs, their neighbours, +-0, the largest finite f32 (rounds to inf), subnormals, +-inf, NaNs"""
    b = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,
         0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,
         0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x80000001, 0x80018000, 0x00800000,
         0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF]
    return torch.from_numpy(np.array(b, np.uint32).view(np.float32).copy())


def f32_vector(n, seed):
    x = rnd(n, seed) * torch.pow(10.0, torch.randint(-30, 30, (n,), generator=torch.Generator().manual_seed(seed + 1)).float())
    sp = special_f32()
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 4 * sp.numel():
        x[-sp.numel():] = sp                                        # again where another workgroup (or the grid-stride turn) handles them
    return x


def bf16_vector(n):
    """every bf16 bit pattern, repeated / truncated to n"""
    pat = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return pat.repeat((n + 65535) // 65536)[:n].view(BF)


def assert_same_bits_nan_aware(got, want, what):
    gn, wn = torch.isnan(got.float()).numpy(), torch.isnan(want.float()).numpy()
    assert np.array_equal(gn, wn), what + ": NaN must stay NaN (and nothing else may become one)"
    assert np.array_equal(bits(got)[~wn], bits(want)[~wn]), what


@pytest.mark.parametrize("n", SIZES)
def test_cast_all_four_directions(n):
    """f32 -> bf16 bit-equal to torch's round-to-nearest-even; bf16 -> f32 and the two same-type copies bit-exact"""
    x = f32_vector(n, seed=n)
    xb = bf16_vector(n)
    assert_same_bits_nan_aware(K.cast(x.to(DEV), torch.empty(n, dtype=BF, device=DEV)).cpu(), x.to(BF), "f32 -> bf16")
    assert_same_bits_nan_aware(K.cast(xb.to(DEV), torch.empty(n, dtype=F32, device=DEV)).cpu(), xb.float(), "bf16 -> f32")
    assert_same_bits_nan_aware(K.cast(x.to(DEV), torch.empty(n, dtype=F32, device=DEV)).cpu(), x, "f32 -> f32")
    assert_same_bits_nan_aware(K.cast(xb.to(DEV), torch.empty(n, dtype=BF, device=DEV)).cpu(), xb, "bf16 -> bf16")


# ------------------------------------------------------------------ B4: scale by a device scalar, y += x
def mixed(n, seed, dtype):
    x = rnd(n, seed) * torch.pow(10.0, torch.randint(-6, 6, (n,), generator=torch.Generator().manual_seed(seed + 1)).float())
    return x.to(dtype)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_scale_by_device_scalar(dtype, n):
    """x *= *scalar, one rounding: bit-equal to torch's x * f (f32) / (x.float() * f).to(bf16).  The scalar lives on the device and
    changes between two calls with no host synchronisation in between: each call must see the value of its own place in the stream"""
    x = mixed(n, n, dtype)
    f1, f2 = f32(0.37), f32(-2.5e-3)
    s = torch.tensor([f1], device=DEV)
    a, b = x.to(DEV), x.to(DEV)
    torch.cuda.synchronize()
    K.scale_by_device_scalar(a, s)
    s.fill_(f2)
    K.scale_by_device_scalar(b, s)
    torch.cuda.synchronize()
    for got, f in ((a, f1), (b, f2)):
        want = (x.float() * torch.tensor(f, dtype=F32)).to(dtype)
        assert np.array_equal(bits(got), bits(want)), (dtype, n, f)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_inplace(dtype, n):
    """y += x, one rounding: bit-equal to torch's y + x (f32) / (y.float() + x.float()).to(bf16); x is not written"""
    x, y = mixed(n, n, dtype), mixed(n, n + 7, dtype)
    xd, yd = x.to(DEV), y.to(DEV)
    K.add_inplace(xd, yd)
    assert np.array_equal(bits(yd), bits((y.float() + x.float()).to(dtype))), (dtype, n)
    assert np.array_equal(bits(xd), bits(x))


# ------------------------------------------------------------------ B5: act_bwd against the derivative itself
def raw_act_bwd(dy, y, out, act, p, seed):
    return K._lib().s2t_act_bwd(L.dt(dy), L.ptr(dy), L.ptr(y), L.ptr(out), dy.numel(), act, p, seed, L.stream())


def raw_dropout(x, y, p, seed):
    return K._lib().s2t_dropout(L.dt(x), L.ptr(x), L.ptr(y), x.numel(), p, seed, L.stream())


def act_inputs(n, dtype):
    """y over [-12, 12] with +-8 and beyond (phi underflows next to Phi), +-0 and the smallest positive value of the type; dy ~ N(0, 1)"""
    y = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 24.0 - 12.0)
    tiny = 2.0 ** -133 if dtype == BF else 2.0 ** -149               # smallest positive (subnormal) value of the type
    sp = torch.tensor([0.0, -0.0, tiny, -tiny, 8.0, -8.0, 8.5, -8.5, 12.0, -12.0, 1e-3, -1e-3, 0.5, -0.5], dtype=torch.float64)
    if n >= 7:
        k = min(n, sp.numel())
        y[n - k:] = sp[:k].float()                                   # 2^-133 and 2^-149 are exact in f32
    y = y.to(dtype)
    dy = rnd(n, n + 1).to(dtype)
    return dy, y


def inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


@pytest.mark.parametrize("lead", [8, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 2 ** 20 + 3])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_bwd_relu(dtype, p, n, lead):
    """act 1: exactly dy (dropped out and rescaled first when p > 0) where y > 0, else +0 -- y = +0, -0 and the smallest positive
    value of the type included; aligned tensors take the 16-byte path, views one element into an allocation the element-wise one"""
    act_bwd_relu(dtype, p, n, lead, 1234 + n)


HIGH_SEED = (5 << 32) | 7          # a seed whose upper word is in use


@pytest.mark.parametrize("lead", [8, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_bwd_relu_seed_above_32_bits(dtype, lead):
    act_bwd_relu(dtype, 0.3, 1000, lead, HIGH_SEED)


def act_bwd_relu(dtype, p, n, lead, seed):
    dy, y = act_inputs(n, dtype)
    (dyd, _), (yd, _), (out, ob) = place(dy, lead), place(y, lead), place(torch.full((n,), float("nan"), dtype=dtype), lead)
    assert raw_act_bwd(dyd, yd, out, 1, p, seed) == 0
    g = dy
    if p > 0:
        keep = (K.dropout(torch.ones(n, dtype=dtype, device=DEV), p, seed) != 0).cpu()
        g = torch.where(keep, (dy.float() * torch.tensor(inv_keep(p), dtype=F32)).to(dtype), torch.zeros((), dtype=dtype))
    want = torch.where(y.double() > 0, g, torch.zeros((), dtype=dtype))
    assert np.array_equal(bits(out), bits(want)), (dtype, p, n, lead)
    guards_intact(ob, lead, "act_bwd relu")
    if p > 0:
        # the kept elements: the p = 0 result times 1 / (1 - p), to one rounding of the type (for bf16 the f32 product rounds first: + u)
        out0 = torch.empty(n, dtype=dtype, device=DEV)
        assert raw_act_bwd(dy.to(DEV), y.to(DEV), out0, 1, 0.0, seed) == 0
        r0 = d64(out0) * inv_keep(p)
        assert bool(((d64(out) - r0).abs()[keep] <= (HALF[dtype] + 2 * U) * r0.abs()[keep] + 1e-40).all())
        assert bool((d64(out)[~keep] == 0).all())


def gelu_grad64(y64):
    return 0.5 * (1.0 + torch.erf(y64 / math.sqrt(2.0))) + y64 * torch.exp(-0.5 * y64 * y64) / math.sqrt(2.0 * math.pi)


def gelu_yardstick(g, y):
    """torch's own float32 gelu backward on the CPU against fp64 on the same (exactly widened) inputs: largest |error| / |g|"""
    g64 = g.double()
    yy = y.float().clone().requires_grad_(True)
    F.gelu(yy).backward(g.float())
    nz = g64 != 0
    return float(((yy.grad.double() - g64 * gelu_grad64(y.double())).abs()[nz] / g64.abs()[nz]).max()) if bool(nz.any()) else 0.0


_YARD = {}


def gelu_yardstick_sample(dtype):
    """the yardstick over the 2^20 + 3 inputs of this file: a largest error is a property of a sample, and a vector of 1 .. 1,000
    elements is too small a sample to stand for the float32 evaluation's error"""
    if dtype not in _YARD:
        _YARD[dtype] = gelu_yardstick(*act_inputs(2 ** 20 + 3, dtype))
    return _YARD[dtype]


@pytest.mark.parametrize("lead", [8, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [1, 7, 8, 1000, 2 ** 20 + 3])
@pytest.mark.parametrize("p", [0.0, 0.3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_bwd_gelu(dtype, p, n, lead):
    """act 2: g (Phi(y) + y phi(y)) in fp64 with erf, g = dy (dropped out and rescaled first when p > 0).  The yardstick is torch's
    own float32 gelu backward on the CPU against that fp64 value on the same inputs, relative to |g|; the kernel gets twice the
    yardstick's largest error, plus 2^-8 |ref| for a bf16 output.

    The yardstick is the larger of the one on this case's inputs and the one on the 2^20 + 3 inputs (gelu_yardstick_sample).

    Measured on MI355X (n = 2^20 + 3, the MEASURED lines), largest |error| / |g|: f32 yardstick 2.8e-07, kernel 1.8e-07 (p = 0) and
    1.7e-07 (p = 0.3), aligned and offset alike; bf16 yardstick 2.3e-07, kernel 4.4e-03 (the output's rounding to bf16)."""
    act_bwd_gelu(dtype, p, n, lead, 4321 + n)


@pytest.mark.parametrize("lead", [8, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_act_bwd_gelu_seed_above_32_bits(dtype, lead):
    act_bwd_gelu(dtype, 0.3, 1000, lead, HIGH_SEED)


def act_bwd_gelu(dtype, p, n, lead, seed):
    dy, y = act_inputs(n, dtype)
    (dyd, _), (yd, _), (out, ob) = place(dy, lead), place(y, lead), place(torch.full((n,), float("nan"), dtype=dtype), lead)
    assert raw_act_bwd(dyd, yd, out, 2, p, seed) == 0
    g = dy
    keep = torch.ones(n, dtype=torch.bool)
    if p > 0:
        keep = (K.dropout(torch.ones(n, dtype=dtype, device=DEV), p, seed) != 0).cpu()
        g = torch.where(keep, (dy.float() * torch.tensor(inv_keep(p), dtype=F32)).to(dtype), torch.zeros((), dtype=dtype))
    g64, y64 = g.double(), y.double()
    ref = g64 * gelu_grad64(y64)
    nz = g64 != 0
    yard = max(gelu_yardstick(g, y), gelu_yardstick_sample(dtype))
    got = d64(out)
    assert bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    bound = 2.0 * yard * g64.abs() + (UB * ref.abs() if dtype == BF else 0.0)
    worst = float((err[nz] / g64.abs()[nz]).max()) if bool(nz.any()) else 0.0
    if n > 10 ** 6:
        print("MEASURED act_bwd gelu: %s p=%g %s: torch float32 yardstick max |err| / |g| %.3e, kernel %.3e (allowed 2 x yardstick%s)"
              % (dtype, p, "aligned" if lead == 8 else "offset", yard, worst, " + 2^-8 |ref|" if dtype == BF else ""))
    assert bool((err <= bound).all()), (dtype, p, n, lead, yard, worst, int((err > bound).sum()))
    assert bool((got[~keep] == 0).all())
    guards_intact(ob, lead, "act_bwd gelu")
    if p > 0:
        # the kept elements against the kernel's own p = 0 result times 1 / (1 - p): dy / (1 - p) rounds to the type, the product
        # with gelu' rounds to the type, and the p = 0 result was itself rounded to the type: three roundings of the type (the
        # f32 products inside add at most 4 u for a bf16 output), relative to the result; 1e-40 covers results below the normal range
        out0 = torch.empty(n, dtype=dtype, device=DEV)
        assert raw_act_bwd(dy.to(DEV), y.to(DEV), out0, 2, 0.0, seed) == 0
        r0 = d64(out0) * inv_keep(p)
        tol = (3 * HALF[dtype] + 4 * U) * 1.02 * r0.abs() + 1e-40
        assert bool(((got - r0).abs()[keep] <= tol[keep]).all())


# ------------------------------------------------------------------ B6: the dropout mask is a function of (seed, index)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_mask_is_a_function_of_seed_and_index(dtype):
    n, p, seed = 2 ** 20 + 3, 0.25, 77
    ones = torch.ones(n, dtype=dtype)
    al = K.dropout(ones.to(DEV), p, seed)
    assert al.data_ptr() % 16 == 0
    (xo, _), (yo, yb) = place(ones, 1), place(torch.zeros(n, dtype=dtype), 1)
    assert raw_dropout(xo, yo, p, seed) == 0
    assert np.array_equal(bits(al), bits(yo)), "the element-wise path draws another mask than the 16-byte path"
    guards_intact(yb, 1, "dropout")
    kept = (ones.float() * torch.tensor(inv_keep(p), dtype=F32)).to(dtype)[0]
    vals = set(np.unique(bits(al)).tolist())
    assert vals == {0, int(bits(kept.view(1))[0])}, "kept elements are x / (1 - p) rounded once, dropped ones +0"
    for n1 in (1, 8, 1000, 1001, 4099):                             # the first n1 elements of the longer call = a call of n1 elements
        short = K.dropout(ones[:n1].to(DEV), p, seed)
        assert np.array_equal(bits(short), bits(al[:n1])), n1
        (xs, _), (ys, _) = place(ones[:n1], 1), place(torch.zeros(n1, dtype=dtype), 1)
        assert raw_dropout(xs, ys, p, seed) == 0
        assert np.array_equal(bits(ys), bits(al[:n1])), n1
    assert not np.array_equal(bits(K.dropout(ones.to(DEV), p, seed + 1)), bits(al))


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_keep_rate(dtype, p):
    """the keep decision compares a 16-bit field with floor(p 65536): the keep rate over N = 2^22 elements is within 4 standard
    deviations sqrt(q (1 - q) / N) of q = 1 - floor(p 65536) / 65536"""
    N = 2 ** 22
    y = K.dropout(torch.ones(N, dtype=dtype, device=DEV), p, 2024)
    rate = float((y != 0).double().mean())
    q = 1.0 - math.floor(f32(p) * 65536.0) / 65536.0
    assert abs(rate - q) <= 4.0 * math.sqrt(q * (1.0 - q) / N), (rate, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dropout_identity_and_refusals(dtype):
    n = 4099
    x = mixed(n, 5, dtype)
    x[:4] = torch.tensor([0.0, -0.0, float("inf"), -float("inf")]).to(dtype)
    for lead in (8, 1):
        (xd, _), (yd, yb) = place(x, lead), place(torch.full((n,), float("nan"), dtype=dtype), lead)
        assert raw_dropout(xd, yd, 0.0, 9) == 0
        assert np.array_equal(bits(yd), bits(x)), "p = 0 is the identity, bit for bit"
        guards_intact(yb, lead, "dropout p=0")
    xd, yd = x.to(DEV), torch.full((n,), 5.0, dtype=dtype, device=DEV)
    assert raw_dropout(xd, yd, 1.0, 9) == -22 and raw_dropout(xd, yd, -0.1, 9) == -22
    torch.cuda.synchronize()
    assert bool((yd == 5.0).all()), "a refused call must write nothing"
