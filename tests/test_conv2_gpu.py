"""The three direct kernels of the second subsampling convolution (Conv2d(64, 64, 3, stride 2, padding 1), bf16) element by element
against float64: s2t_conv2_fwd and s2t_conv2_dgrad (csrc/conv2.hip) and s2t_conv2_wgrad (the end of csrc/subsample.hip).

Conventions of tests/test_subsample_gpu.py (whose tools are imported): every reference is float64 of the exact bf16 values the
kernel received -- the y1n / dpre it was handed and the w2p / w2q that K.permute_conv_w produced, themselves checked bit for bit
against the plain permutation of the rounded master weight (modes 0 and 1) --, built from the nine strided tap views of the
zero-padded tensor and ONE float64 matmul (never an fp64 conv2d call); every output ELEMENT is compared with a bound derived from
the kernel's arithmetic, a failure names the worst element, and the worst |err| / bound per kernel is printed at the module's end.

Layouts.  y1n [B][T2][F2][64]; w2p [co][tap * 64 + ci] (tap = 3 kh + kw); z2 / pre / dpre rows (t4, b, f4), T4 = ceil(T2 / 2),
F4 = ceil(F2 / 2); w2q [ci][slot * 64 + co] with slot = TAP_SLOT[tap] (subsample.hip:700); dy1n rows (b, t2, f2); gw [co][tap * 64 + ci]
in f32, accumulated into.

Bounds (u = 2^-24; r = 2^-8; gamma_n = n u / (1 - n u)).
  * forward: the accumulator starts at the bias (conv2.hip:84) and adds 9 taps x 2 halves x 32 = 576 exact bf16 x bf16 products in
    f32 (conv2.hip:86-99): |acc - conv| <= e_acc = gamma_577 (|b| + sum |w| |x|).  The stored value adds r |.|.  ReLU is
    1-Lipschitz; GELU is taken of the STORED pre-activation (conv2.hip:118), as check_act_out models it: pre within e_acc + r (|acc|
    + e_acc), the value within 1.13 x that + 8 u |acc| of gelu(acc), then its own rounding.
  * data gradient: an element of parity class (t2 & 1, f2 & 1) sums 64 x (1, 2, 2, 4) products (conv2.hip:230, two 32-deep MFMA
    steps per tap :238-241), a depth d = 64 (1 + (t2 & 1)) (1 + (f2 & 1)) <= 256, from zero: e = gamma_d sum |dpre| |w|; then ONE
    rounding to bf16: e + r (|ref| + e).  With dropout the f32 sum is multiplied by 1 / (1 - p) before that rounding
    (conv2.hip:250): kept elements are compared with ref / (1 - p) (p as the f32 the kernel receives) with e' = (e + u (|ref| + e))
    / (1 - p); dropped elements are exactly 0.
  * weight gradient: a (t4, b) group is ONE 32-deep MFMA step per accumulator (subsample.hip:1079; the f4 axis padded to 32), the
    register accumulators are kept over groups_per_wg = max(8, ceil(T4 B / 512)) groups (subsample.hip:1061,1103-1104), and each of the
    nwg = ceil(T4 B / groups_per_wg) workgroups adds its accumulator to gw with one f32 atomic (subsample.hip:1093): depth
    d = 32 groups_per_wg + nwg, + 1 for the existing content of gw.  |gw - (gw0 + dW)| <= d u (sum |dpre| |y1n| + |gw0|), the sum over
    the same taps as dW.

Sensitivity.  Each edge family is also checked against a deliberately wrong REFERENCE (the kernel is never changed), and the check
must reject it: the last input column dropped (odd F2), the last input row dropped (odd T2), one tap's weights zeroed, the pixel
pair (16, 17) swapped, a parity class of the data gradient missing its last tap, a (t4, b) group missing from the weight gradient.
Before the kernel's output is consulted the two references alone are required to differ by more than the sum of their bounds at
some element (`separated`), so that no output can pass both: that part holds on any device.

Data: y1n ~ N(0, 1), w ~ N(0, 0.06^2), bias ~ N(0, 0.2^2), dpre ~ N(0, 0.3^2), gw0 ~ N(0, 1), drawn on the host from fixed seeds
(the references do not depend on the device they are computed on).
"""
import pytest
import torch
import torch.nn.functional as Fn

import test_subsample_gpu as S
from test_subsample_gpu import BF, U, UBF, assert_close, cdiv, check_act_out, d64, gam, launches

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
C = 64
ENOTSUP = -95
TAP_SLOT = (5, 3, 6, 1, 0, 2, 7, 4, 8)          # tap (3 kh + kw) -> class-major slot of w2q (subsample.hip:700)
CLASS_LAST_TAP = {1: 5, 2: 7, 3: 8}             # the last slot of class 2 pt + pf holds tap (1,2) / (2,1) / (2,2) (conv2.hip:170)


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    K.prof_enable(0)
    mine = {k: S.WORST.pop(k) for k in sorted(S.WORST) if k.startswith("conv2_")}
    if mine:
        print("\nWORST |err| / bound per kernel: " + ", ".join("%s %.3g" % kv for kv in mine.items()))


# ------------------------------------------------------------------ data
def rnd(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def geom(T2, F2):
    return (T2 + 1) // 2, (F2 + 1) // 2


def master_w(seed):
    return rnd(C, C, 3, 3, seed=seed, scale=0.06, dtype=torch.float32)


def off8(t):
    """the same values in a view that starts 8 bytes into a larger buffer"""
    k = 8 // t.element_size()
    buf = torch.zeros(t.numel() + 32, dtype=t.dtype, device=t.device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 8
    return v


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32).clone()


# ------------------------------------------------------------------ float64 references (any device)
def windows(Y, T4, F4):
    """[B][T2][F2][C] -> rows (t4, b, f4), columns (tap, ci): the nine strided tap views of the zero-padded tensor"""
    B = Y.shape[0]
    Yp = Fn.pad(Y, (0, 0, 1, 1, 1, 1))
    X = torch.stack([Yp[:, kh:kh + 2 * T4:2, kw:kw + 2 * F4:2, :] for kh in range(3) for kw in range(3)], 3)
    return X.permute(1, 0, 2, 3, 4).reshape(T4 * B * F4, 9 * C)


def fwd_ref(Y, W, b):
    """Y [B][T2][F2][C], W [co][tap * C + ci], b [co] in float64 -> the accumulator and e_acc = gamma_577 (|b| + sum |w| |x|)"""
    T4, F4 = geom(Y.shape[1], Y.shape[2])
    X = windows(Y, T4, F4)
    return X @ W.t() + b, gam(577) * (X.abs() @ W.abs().t() + b.abs())


def relu_out(acc, e_acc):
    """the stored ReLU output and its bound (check_act_out's)"""
    ref = acc.clamp_min(0.0)
    return ref, e_acc + UBF * (ref.abs() + e_acc)


def w_from_w2q(w2q):
    """w2q [ci][slot * C + co] -> [co][tap * C + ci] in float64"""
    Wq = w2q.double().view(C, 9, C)[:, list(TAP_SLOT), :]               # [ci][tap][co]
    return Wq.permute(2, 1, 0).reshape(C, 9 * C)


def dgrad_ref(G, W, T2, F2):
    """G [T4][B][F4][co], W [co][tap * C + ci] in float64 -> dy1n rows (b, t2, f2) and e = gamma_d sum |dpre| |w|: one matmul, then
    the nine tap slices are added into the strided views of the zero-padded result"""
    T4, B, F4, _ = G.shape
    Gb = G.permute(1, 0, 2, 3).reshape(-1, C)
    D = (Gb @ W).view(B, T4, F4, 9, C)
    M = (Gb.abs() @ W.abs()).view(B, T4, F4, 9, C)
    out = torch.zeros(2, B, T2 + 2, F2 + 2, C, dtype=torch.float64, device=G.device)
    for tap in range(9):
        kh, kw = divmod(tap, 3)
        out[0, :, kh:kh + 2 * T4:2, kw:kw + 2 * F4:2] += D[:, :, :, tap]
        out[1, :, kh:kh + 2 * T4:2, kw:kw + 2 * F4:2] += M[:, :, :, tap]
    out = out[:, :, 1:T2 + 1, 1:F2 + 1]
    t2 = torch.arange(T2, device=G.device).view(1, T2, 1, 1)
    f2 = torch.arange(F2, device=G.device).view(1, 1, F2, 1)
    depth = (64 * (1 + (t2 & 1)) * (1 + (f2 & 1))).double()
    e = depth * U / (1 - depth * U) * out[1]
    return out[0].reshape(-1, C), e.reshape(-1, C)


def dgrad_out(ref, e, p=0.0):
    """the stored value of a KEPT element and its bound"""
    if p > 0:
        inv = 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32)))
        ref, e = ref * inv, (e + U * (ref.abs() + e)) * inv
    return ref, e + UBF * (ref.abs() + e)


def wgrad_depth(ngroups):
    gpw = max(8, cdiv(ngroups, 512))
    return 32 * gpw + cdiv(ngroups, gpw) + 1


def wgrad_ref(G, Y, gw0):
    """G [T4][B][F4][co], Y [B][T2][F2][ci], gw0 [co][tap * C + ci] in float64 -> gw0 + dW and its bound"""
    T4, B, F4, _ = G.shape
    X = windows(Y, T4, F4)
    Gr = G.reshape(-1, C)
    return gw0 + Gr.t() @ X, wgrad_depth(T4 * B) * U * (Gr.abs().t() @ X.abs() + gw0.abs())


def separated(ref, bound, mref, mbound):
    """no output can be within `bound` of ref AND within `mbound` of mref"""
    return bool(((mref - ref).abs() > bound + mbound).any())


# ------------------------------------------------------------------ reference mutations (in place, on float64 clones)
def drop_last_col(Y, W):
    Y[:, :, -1] = 0.0


def drop_last_row(Y, W):
    Y[:, -1] = 0.0


def zero_tap(tap):
    def f(Y, W):
        W[:, tap * C:(tap + 1) * C] = 0.0
    f.__name__ = "zero_tap_%d" % tap
    return f


def swap_pair_16_17(Y, W):
    Y[:, :, [16, 17]] = Y[:, :, [17, 16]]


# the same on dpre [T4][B][F4][C]: its last column / row are what the data gradient's last taps read
def drop_last_dcol(G, W):
    G[:, :, -1] = 0.0


def drop_last_drow(G, W):
    G[-1] = 0.0


def swap_dpair_16_17(G, W):
    G[:, :, [16, 17]] = G[:, :, [17, 16]]


def drop_group(t4, b):
    def f(G, Y):
        G[t4, b] = 0.0
    f.__name__ = "drop_group_%d_%d" % (t4, b)
    return f


# ------------------------------------------------------------------ forward
def run_fwd(B, T2, F2, act, seed=1):
    """-> (y1n, w2p, bias) on the device and (z2, pre); the weight permute is checked bit for bit, the launch family counted"""
    y1n = rnd(B, T2, F2, C, seed=seed).to(DEV)
    w = master_w(seed + 1).to(DEV)
    bias = rnd(C, seed=seed + 2, scale=0.2, dtype=torch.float32).to(DEV)
    w2p = K.permute_conv_w(w, torch.empty((C, 9 * C), dtype=BF, device=DEV), C, C, 0)
    assert torch.equal(w2p, w.view(C, C, 9).permute(0, 2, 1).reshape(C, 9 * C).to(BF))
    with launches("conv2_fwd") as ran:
        out = K.conv2_fwd(y1n, w2p, bias, B, T2, F2, C, K.ACT_GELU if act == "gelu" else K.ACT_RELU)
    assert out is not None and ran["conv2_fwd"] == 1, (out is None, ran)
    z2, pre = out
    assert (pre is not None) == (act == "gelu")
    return (y1n, w2p, bias), (z2, pre)


def check_fwd(ins, outs, act, what, mutate=None):
    y1n, w2p, bias = ins
    Y, W = d64(y1n), d64(w2p)
    if mutate is not None:
        Y, W = Y.clone(), W.clone()
        mutate(Y, W)
    acc, e_acc = fwd_ref(Y, W, d64(bias))
    check_act_out(outs[0], outs[1], acc, e_acc, act, BF, what, "conv2_fwd" if mutate is None else None)     # WORST: true references only


WIDTHS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 41, 47, 48]
HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 9]


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("F2", WIDTHS)
def test_fwd_width_sweep(F2, act):
    """B = 2, T2 = 5 (two units per utterance, the second with one output row).  F2 < 16: whole m-tiles are clamped
    (conv2.hip:70); 15 / 16 / 17 and 31 / 32 / 33: pix_slot's pair swap switches on at column 16 and off at 32 (conv2.hip:24);
    odd F2: the last tap column is the zero pixel; 48 = the last accepted width (2 F4 <= 48, conv2.hip:142)."""
    ins, outs = run_fwd(2, 5, F2, act)
    check_fwd(ins, outs, act, "conv2_fwd (2, 5, %d) %s" % (F2, act))


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("F2", [9, 40])
@pytest.mark.parametrize("T2", HEIGHTS)
def test_fwd_height_sweep(T2, F2, act):
    """B = 3.  A unit is two output rows = five input rows (conv2.hip:29): T2 = 1 .. 4 leave the only unit with one or two output
    rows and input rows past T2 that must be staged as zeros (conv2.hip:59); T2 = 5, 6, 7, 9 do the same to the last of 2 or 3 units."""
    ins, outs = run_fwd(3, T2, F2, act, seed=10 + T2)
    check_fwd(ins, outs, act, "conv2_fwd (3, %d, %d) %s" % (T2, F2, act))


@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_fwd_stage_reuse(act):
    """(200, 30, 9): 200 x 8 = 1,600 units on 768 workgroups (conv2.hip:147): 64 workgroups do three iterations and overwrite the
    stage they read in their first (conv2.hip:81), the others two."""
    ins, outs = run_fwd(200, 30, 9, act, seed=30)
    check_fwd(ins, outs, act, "conv2_fwd (200, 30, 9) %s" % act)


FWD_MUT = [((2, 5, 33), drop_last_col), ((2, 5, 33), drop_last_row), ((2, 5, 33), zero_tap(0)), ((2, 5, 33), zero_tap(8)),
           ((2, 5, 33), swap_pair_16_17), ((200, 30, 9), drop_last_col), ((200, 30, 9), zero_tap(5))]


@pytest.mark.parametrize("shape,mutate", FWD_MUT, ids=lambda v: v.__name__ if callable(v) else "x".join(map(str, v)))
def test_fwd_check_rejects_a_wrong_reference(shape, mutate):
    """ReLU.  (2, 5, 33): odd T2 and F2, columns 16 / 17 exist.  Plain N(0, 1) data separates every mutation: each removes or moves
    at least 64 of the at most 576 products of the elements it touches, against a bound of r = 2^-8 of the result."""
    B, T2, F2 = shape
    ins, outs = run_fwd(B, T2, F2, "relu", seed=40)
    what = "conv2_fwd %s %s" % (shape, mutate.__name__)
    check_fwd(ins, outs, "relu", what)
    Y, W, b = d64(ins[0]), d64(ins[1]), d64(ins[2])
    ref, bound = relu_out(*fwd_ref(Y, W, b))
    mutate(Y, W)
    assert separated(ref, bound, *relu_out(*fwd_ref(Y, W, b))), what + ": the mutated reference is within the bounds of the true one"
    with pytest.raises(AssertionError, match="out of bound"):
        check_fwd(ins, outs, "relu", what, mutate)


# ------------------------------------------------------------------ data gradient
def run_dgrad(B, T2, F2, p=0.0, dseed=0, seed=1):
    """-> (dpre, w2q) on the device and dy1n, written into a NaN-filled tensor"""
    T4, F4 = geom(T2, F2)
    dpre = rnd(T4, B, F4, C, seed=seed, scale=0.3).to(DEV)
    w = master_w(seed + 1).to(DEV)
    w2q = K.permute_conv_w(w, torch.empty((C, 9 * C), dtype=BF, device=DEV), C, C, 1)
    plain = w.view(C, C, 9)[:, :, [TAP_SLOT.index(s) for s in range(9)]].permute(1, 2, 0).reshape(C, 9 * C).to(BF)     # [ci][slot][co]
    assert torch.equal(w2q, plain)
    dy = torch.full((B * T2 * F2, C), float("nan"), dtype=BF, device=DEV)
    with launches("conv2_dgrad") as ran:
        ok = K.conv2_dgrad(dpre.view(-1, C), w2q, dy, B, T2, F2, C, p, dseed)
    assert ok and ran["conv2_dgrad"] == 1, (ok, ran)
    return (dpre, w2q), dy


def check_dgrad(ins, dy, T2, F2, what, p=0.0, dseed=0, mutate=None):
    dpre, w2q = ins
    G, W = d64(dpre), w_from_w2q(w2q)
    if mutate is not None:
        G, W = G.clone(), W.clone()
        mutate(G, W)
    ref, e = dgrad_ref(G, W, T2, F2)
    assert not bool(torch.isnan(dy.float()).any()), what + ": elements left unwritten"
    ref, bound = dgrad_out(ref, e, p)
    if p > 0:
        # the mask of K.dropout(ones, p, seed) on dy1n's shape: what bn_apply applied to y1n with the same seed (engine.py:356,457)
        keep = K.dropout(torch.ones_like(dy), p, dseed) != 0
        assert bool((ref != 0).all())                                   # a kept element is never an exact zero
        assert bool((dy[~keep] == 0).all()), what + ": a dropped element is not 0"
        assert torch.equal(dy != 0, keep), what + ": keep mask differs from K.dropout's in %d places" % int(((dy != 0) != keep).sum())
        ref, bound = ref * keep, bound * keep
    assert_close(dy, ref, bound, what, "conv2_dgrad" if mutate is None else None)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("F2", [f for f in WIDTHS if f <= 47])
def test_dgrad_width_sweep(F2, p):
    """B = 2, T2 = 5 (two units of four input rows, the second with one).  F2 = 1: the odd-column classes are empty
    (conv2.hip:219,223); F4 crosses 8 and 16 at F2 = 15 / 16 / 17 and 31 / 32 / 33, where dpx_slot's swap of the odd octets
    (conv2.hip:171) switches on and off; 47 = the last accepted width (conv2.hip:273)."""
    ins, dy = run_dgrad(2, 5, F2, p, 77)
    check_dgrad(ins, dy, 5, F2, "conv2_dgrad (2, 5, %d) p=%g" % (F2, p), p, 77)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("F2", [9, 40])
@pytest.mark.parametrize("T2", HEIGHTS)
def test_dgrad_height_sweep(T2, F2, p):
    """B = 3.  A unit is four input rows <- three dpre rows (conv2.hip:193): the last unit has one, two or three valid rows, and
    dpre rows past T4 must be staged as zeros (conv2.hip:199,235)."""
    ins, dy = run_dgrad(3, T2, F2, p, 5, seed=10 + T2)
    check_dgrad(ins, dy, T2, F2, "conv2_dgrad (3, %d, %d) p=%g" % (T2, F2, p), p, 5)


def test_dgrad_half_dropped():
    """p = 0.5 at (3, 7, 33): the scale 1 / (1 - p) = 2 and a mask that keeps every second element"""
    ins, dy = run_dgrad(3, 7, 33, 0.5, 123, seed=20)
    check_dgrad(ins, dy, 7, 33, "conv2_dgrad (3, 7, 33) p=0.5", 0.5, 123)
    assert 0.45 < float((dy != 0).float().mean()) < 0.55


def test_dgrad_dropout_seed_above_32_bits():
    """the same case at a seed whose upper 32 bits are set: the keep mask is K.dropout's at that seed, and not the one of its low word"""
    seed = (5 << 32) | 7
    ins, dy = run_dgrad(3, 7, 33, 0.5, seed, seed=20)
    check_dgrad(ins, dy, 7, 33, "conv2_dgrad (3, 7, 33) p=0.5, 64-bit seed", 0.5, seed)
    assert not torch.equal(dy != 0, K.dropout(torch.ones_like(dy), 0.5, seed & 0xFFFFFFFF) != 0)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dgrad_stage_reuse(p):
    """(200, 30, 9): 200 x 8 = 1,600 units on 768 workgroups (conv2.hip:278): some do two iterations, some three (conv2.hip:214)"""
    ins, dy = run_dgrad(200, 30, 9, p, 9, seed=30)
    check_dgrad(ins, dy, 30, 9, "conv2_dgrad (200, 30, 9) p=%g" % p, p, 9)


DGRAD_MUT = [((2, 5, 35), drop_last_dcol), ((2, 5, 35), drop_last_drow), ((2, 5, 35), zero_tap(4)), ((2, 5, 35), swap_dpair_16_17)] + \
            [((2, 5, 35), zero_tap(t)) for t in CLASS_LAST_TAP.values()] + \
            [((200, 30, 9), drop_last_dcol), ((200, 30, 9), zero_tap(8))]


@pytest.mark.parametrize("shape,mutate", DGRAD_MUT, ids=lambda v: v.__name__ if callable(v) else "x".join(map(str, v)))
def test_dgrad_check_rejects_a_wrong_reference(shape, mutate):
    """(2, 5, 35): odd T2 and F2, F4 = 18 so that dpre's columns 16 / 17 exist.  zero_tap(4) is the centre tap (the whole of class
    0); taps 5, 7 and 8 are the LAST taps of classes 1, 2 and 3 (each tap belongs to one class, conv2.hip:170), so zeroing one is
    that class missing its last tap.  N(0, 0.3^2) data separates all of them: each removes at least 64 of at most 256 products."""
    B, T2, F2 = shape
    ins, dy = run_dgrad(B, T2, F2, seed=40)
    what = "conv2_dgrad %s %s" % (shape, mutate.__name__)
    check_dgrad(ins, dy, T2, F2, what)
    G, W = d64(ins[0]), w_from_w2q(ins[1])
    ref, bound = dgrad_out(*dgrad_ref(G, W, T2, F2))
    mutate(G, W)
    assert separated(ref, bound, *dgrad_out(*dgrad_ref(G, W, T2, F2))), what + ": the mutated reference is within the bounds of the true one"
    with pytest.raises(AssertionError, match="out of bound"):
        check_dgrad(ins, dy, T2, F2, what, mutate=mutate)


# ------------------------------------------------------------------ weight gradient
def run_wgrad(B, T2, F2, accumulate, seed=1):
    """-> (dpre, y1n, gw0) on the device and gw.  The kernel records no launch family: the dispatch is s2t_conv2_wgrad's own
    (subsample.hip:1100-1106), and K.conv2_wgrad returns whether it ran."""
    T4, F4 = geom(T2, F2)
    dpre = rnd(T4, B, F4, C, seed=seed, scale=0.3).to(DEV)
    y1n = rnd(B, T2, F2, C, seed=seed + 1).to(DEV)
    gw0 = rnd(C, 9 * C, seed=seed + 2, dtype=torch.float32).to(DEV) if accumulate else torch.zeros(C, 9 * C, device=DEV)
    gw = gw0.clone()
    assert K.conv2_wgrad(dpre.view(-1, C), y1n.view(-1, C), gw, B, T2, F2, C)
    return (dpre, y1n, gw0), gw


def check_wgrad(ins, gw, what, mutate=None):
    dpre, y1n, gw0 = ins
    G, Y = d64(dpre), d64(y1n)
    if mutate is not None:
        G, Y = G.clone(), Y.clone()
        mutate(G, Y)
    ref, bound = wgrad_ref(G, Y, d64(gw0))
    assert_close(gw, ref, bound, what, "conv2_wgrad" if mutate is None else None)


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("F2", [f for f in WIDTHS if f <= 45])
def test_wgrad_width_sweep(F2, accumulate):
    """B = 2, T2 = 5: six groups in one workgroup.  Odd F2: the last position's kw = 2 tap reads window row F2 + 1, which only the
    kernel's initial zero fill ever writes (subsample.hip:1015,1074); F2 = 41: the staging loop's five pieces of 256 are all used
    (3 x 8 x 41 + 8 x 21 = 1,152, subsample.hip:1027-1032)."""
    ins, gw = run_wgrad(2, 5, F2, accumulate)
    check_wgrad(ins, gw, "conv2_wgrad (2, 5, %d) %s" % (F2, "accumulate" if accumulate else "fresh"))


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("F2", [9, 40])
@pytest.mark.parametrize("T2", HEIGHTS)
def test_wgrad_height_sweep(T2, F2, accumulate):
    """B = 3: 3 .. 15 groups, so one or two workgroups of eight groups, the second partial; odd T2 leaves the last t4 without its
    kh = 2 row, T2 = 1 without both outer rows (subsample.hip:1038)."""
    ins, gw = run_wgrad(3, T2, F2, accumulate, seed=10 + T2)
    check_wgrad(ins, gw, "conv2_wgrad (3, %d, %d) %s" % (T2, F2, "accumulate" if accumulate else "fresh"))


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
def test_wgrad_nine_groups_per_workgroup(accumulate):
    """(300, 30, 9): 4,500 groups > 4,096, so groups_per_wg = ceil(4500 / 512) = 9 (subsample.hip:1103), which does not divide
    4,500 evenly into the 500 workgroups' ranges the way 8 would: the bound's depth is 32 x 9 + 500 + 1."""
    assert max(8, cdiv(15 * 300, 512)) == 9 and wgrad_depth(4500) == 789
    ins, gw = run_wgrad(300, 30, 9, accumulate, seed=30)
    check_wgrad(ins, gw, "conv2_wgrad (300, 30, 9) %s" % ("accumulate" if accumulate else "fresh"))


WGRAD_MUT = [((2, 5, 33), drop_last_col), ((2, 5, 33), drop_last_row), ((2, 5, 33), swap_pair_16_17), ((2, 5, 33), drop_group(2, 1)),
             ((300, 30, 9), drop_last_col), ((300, 30, 9), drop_group(7, 123)), ((300, 30, 9), drop_group(14, 299))]


def _wmut(mutate):
    """the weight-gradient mutations act on (dpre, y1n): those written for (y1n, w) get y1n in their first argument"""
    if mutate.__name__.startswith("drop_group"):
        return mutate
    return lambda G, Y: mutate(Y, None)


@pytest.mark.parametrize("shape,mutate", WGRAD_MUT, ids=lambda v: v.__name__ if callable(v) else "x".join(map(str, v)))
def test_wgrad_check_rejects_a_wrong_reference(shape, mutate):
    """(2, 5, 33): odd T2 and F2, columns 16 / 17 exist.  (300, 30, 9): an element sums 22,500 products and the bound is 789 u of
    their magnitudes, ~0.2 for this data; one missing group removes five products of size ~0.3 |N| |N| from every element, and
    over the 36,864 elements the largest such change is several times the bound: plain data separates the references (asserted
    below before the kernel's output is consulted), no boundary scaling is needed."""
    B, T2, F2 = shape
    ins, gw = run_wgrad(B, T2, F2, False, seed=40)
    what = "conv2_wgrad %s %s" % (shape, mutate.__name__)
    check_wgrad(ins, gw, what)
    G, Y, g0 = d64(ins[0]), d64(ins[1]), d64(ins[2])
    ref, bound = wgrad_ref(G, Y, g0)
    _wmut(mutate)(G, Y)
    assert separated(ref, bound, *wgrad_ref(G, Y, g0)), what + ": the mutated reference is within the bounds of the true one"
    with pytest.raises(AssertionError, match="out of bound"):
        check_wgrad(ins, gw, what, _wmut(mutate))


@pytest.mark.parametrize("tap", [0, 4, 8])
def test_wgrad_check_rejects_a_missing_tap(tap):
    """one tap's 64 x 64 block of the reference zeroed, at (2, 5, 33)"""
    ins, gw = run_wgrad(2, 5, 33, False, seed=40)
    ref, bound = wgrad_ref(d64(ins[0]), d64(ins[1]), d64(ins[2]))
    assert_close(gw, ref, bound, "conv2_wgrad tap %d" % tap, "conv2_wgrad")
    mref = ref.clone()
    mref[:, tap * C:(tap + 1) * C] = 0.0
    assert separated(ref, bound, mref, bound)
    with pytest.raises(AssertionError, match="out of bound"):
        assert_close(gw, mref, bound, "conv2_wgrad without tap %d" % tap)


# ------------------------------------------------------------------ limits and refusals
def raw_fwd(y1n, w2p, bias, z2, pre, B, T2, F2, act):
    rc = K._lib().s2t_conv2_fwd(L.BF16, L.ptr(y1n), L.ptr(w2p), L.ptr(bias), L.ptr(z2), L.ptr(pre), B, T2, F2, C, act, L.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_fwd_width_limit(act):
    """F2 = 48 is the last width of three 16-pixel m-tiles per unit (conv2.hip:142) and is checked element-wise at (3, 7, 48); F2 = 49
    is refused: the wrapper returns None (engine.py:360 then takes the gathered GEMM) and NaN-filled outputs keep their bits."""
    ins, outs = run_fwd(3, 7, 48, act, seed=50)
    check_fwd(ins, outs, act, "conv2_fwd (3, 7, 48) %s" % act)
    B, T2, F2 = 3, 7, 49
    T4, F4 = geom(T2, F2)
    y1n = rnd(B, T2, F2, C, seed=51).to(DEV)
    A = K.ACT_GELU if act == "gelu" else K.ACT_RELU
    assert K.conv2_fwd(y1n, ins[1], ins[2], B, T2, F2, C, A) is None
    z2 = torch.full((T4 * B * F4, C), float("nan"), dtype=BF, device=DEV)
    pre = z2.clone()
    z0 = bits(z2)
    assert raw_fwd(y1n, ins[1], ins[2], z2, pre, B, T2, F2, A) == ENOTSUP
    assert torch.equal(bits(z2), z0) and torch.equal(bits(pre), z0)


def test_dgrad_width_limit():
    """F2 = 47 is the last width whose class rows fit three m-tiles (F2 + 1 <= 48, conv2.hip:273), checked at (3, 7, 47) with and
    without dropout; F2 = 48 is refused (engine.py:457 then runs the four gathered products) and leaves dy1n untouched."""
    for p in (0.0, 0.1):
        ins, dy = run_dgrad(3, 7, 47, p, 3, seed=52)
        check_dgrad(ins, dy, 7, 47, "conv2_dgrad (3, 7, 47) p=%g" % p, p, 3)
    B, T2, F2 = 3, 7, 48
    T4, F4 = geom(T2, F2)
    dpre = rnd(T4 * B * F4, C, seed=53, scale=0.3).to(DEV)
    dy = torch.full((B * T2 * F2, C), float("nan"), dtype=BF, device=DEV)
    d0 = bits(dy)
    with launches("conv2_dgrad") as ran:
        assert K.conv2_dgrad(dpre, ins[1], dy, B, T2, F2, C) is False
        assert K.conv2_dgrad(dpre, ins[1], dy, B, T2, F2, C, 0.1, 3) is False
    assert ran["conv2_dgrad"] == 0 and torch.equal(bits(dy), d0)


def test_wgrad_width_limit():
    """F2 = 45 is the last width whose window and dpre rows fit the five staging pieces (3 x 8 x 45 + 8 x 23 = 1,264 <= 1,280,
    subsample.hip:1100), checked at (3, 7, 45) fresh and accumulating; F2 = 46 (1,288) is refused (engine.py:444 then runs the nine
    gathered products) and leaves a known pattern in gw untouched."""
    for accumulate in (False, True):
        ins, gw = run_wgrad(3, 7, 45, accumulate, seed=54)
        check_wgrad(ins, gw, "conv2_wgrad (3, 7, 45) accumulate=%d" % accumulate)
    B, T2, F2 = 3, 7, 46
    T4, F4 = geom(T2, F2)
    dpre = rnd(T4 * B * F4, C, seed=55, scale=0.3).to(DEV)
    y1n = rnd(B * T2 * F2, C, seed=56).to(DEV)
    gw = torch.arange(C * 9 * C, dtype=torch.float32, device=DEV).view(C, 9 * C) * 0.25 - 1000.0
    g0 = bits(gw)
    assert K.conv2_wgrad(dpre, y1n, gw, B, T2, F2, C) is False
    torch.cuda.synchronize()
    assert torch.equal(bits(gw), g0)


def test_operands_off_16_byte_alignment_are_refused():
    """Each kernel moves its operands in 16-byte pieces (the LDS-DMA of conv2.hip:63,203, the weight fragments :45,:186, the staging
    loads of subsample.hip:1038,1041) and refuses a pointer that is not a multiple of 16 (conv2.hip:140,271, subsample.hip:1101):
    every bf16 operand in turn is a view 8 bytes into a larger buffer; the call returns not-covered and the outputs keep their bits.
    The buffers are large enough for what the kernels would touch without the guard.
    Regression (weight gradient): s2t_conv2_wgrad had no such guard and ran its 16-byte loads on the shifted pointers."""
    B, T2, F2 = 2, 5, 9
    T4, F4 = geom(T2, F2)
    y1n = rnd(B * T2 * F2, C, seed=60).to(DEV)
    dpre = rnd(T4 * B * F4, C, seed=61, scale=0.3).to(DEV)
    w = master_w(62).to(DEV)
    bias = rnd(C, seed=63, scale=0.2, dtype=torch.float32).to(DEV)
    w2p = K.permute_conv_w(w, torch.empty((C, 9 * C), dtype=BF, device=DEV), C, C, 0)
    w2q = K.permute_conv_w(w, torch.empty((C, 9 * C), dtype=BF, device=DEV), C, C, 1)
    nan = lambda rows: torch.full((rows, C), float("nan"), dtype=BF, device=DEV)
    # forward: y1n, w2p, z2, pre
    assert K.conv2_fwd(off8(y1n), w2p, bias, B, T2, F2, C, K.ACT_GELU) is None
    assert K.conv2_fwd(y1n, off8(w2p), bias, B, T2, F2, C, K.ACT_RELU) is None
    for which in range(4):
        ops = [y1n, w2p, nan(T4 * B * F4), nan(T4 * B * F4)]
        ops[which] = off8(ops[which])
        z0 = bits(ops[2])
        with launches("conv2_fwd") as ran:
            rc = raw_fwd(ops[0], ops[1], bias, ops[2], ops[3], B, T2, F2, K.ACT_GELU)
        assert rc == ENOTSUP and ran["conv2_fwd"] == 0, (which, rc, ran)
        assert torch.equal(bits(ops[2]), z0) and torch.equal(bits(ops[3]), z0), which
    # data gradient: dpre, w2q, dy1n
    for which in range(3):
        ops = [dpre, w2q, nan(B * T2 * F2)]
        ops[which] = off8(ops[which])
        d0 = bits(ops[2])
        with launches("conv2_dgrad") as ran:
            assert K.conv2_dgrad(ops[0], ops[1], ops[2], B, T2, F2, C) is False, which
            assert K.conv2_dgrad(ops[0], ops[1], ops[2], B, T2, F2, C, 0.1, 7) is False, which
        assert ran["conv2_dgrad"] == 0 and torch.equal(bits(ops[2]), d0), which
    # weight gradient: dpre, y1n
    for which in range(2):
        ops = [dpre, y1n]
        ops[which] = off8(ops[which])
        gw = torch.arange(C * 9 * C, dtype=torch.float32, device=DEV).view(C, 9 * C) * 0.25 - 1000.0
        g0 = bits(gw)
        assert K.conv2_wgrad(ops[0], ops[1], gw, B, T2, F2, C) is False, which
        torch.cuda.synchronize()
        assert torch.equal(bits(gw), g0), which
    # the same operands, aligned, are accepted
    assert K.conv2_fwd(y1n, w2p, bias, B, T2, F2, C, K.ACT_GELU) is not None
    assert K.conv2_dgrad(dpre, w2q, nan(B * T2 * F2), B, T2, F2, C)
    assert K.conv2_wgrad(dpre, y1n, torch.zeros(C, 9 * C, device=DEV), B, T2, F2, C)
