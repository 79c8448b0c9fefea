"""csrc/attention.hip beyond d = 64 plain softmax: head width 32, the distance penalty, LSE, the dropout mask itself, the
head-averaged probabilities (s2t_attn_probs_avg) and the layouts that leave the second-generation kernels, against float64.

Conventions of tests/test_routes_gpu.py (attn_check, which this file generalises to d, scale and dist_penalty; the tools are
copied here, no test module imports another): every reference is float64 of the exact values the kernel received, every output
ELEMENT has a bound derived from the arithmetic, a failure names the worst element.  u = 2^-24; r = 2^-8 for a bf16 output, u for
f32; r_p = the rounding of P (and dS) to the MFMA operand type, 2^-8 for the bf16 kernels, u for f32.

Error model of one attention call (q [Tq, B, H d], k / v [Tk, B, H d], per head):
  * scores  s_ij = scale q_i . k_j - pen_ij, pen_ij = max(0, ln|i - j|) with the distance penalty (local_attention.py:131-133, zero
    for |i - j| <= 1), else 0.  The dot product is an f32 sum of d exact (bf16) or once-rounded (f32) products in some order:
    <= d u scale (|q| |k|^T); twice that, 2 d u scale (|q| |k|^T), also covers the product by scale (by scale log2 e in the
    second generation) and the rounding of the subtraction on the |scale q.k| side.
    e_pen: the first-generation kernels subtract __logf(x) = v_log_f32(x) * ln 2 (attention.hip:141-144) for the exact integer
    x = |i - j|: v_log_f32 is documented to 1 ulp (<= 2 u relative), ln 2 is a rounded constant (u), the product rounds (u):
    4 u ln x; the subtraction rounds the penalised score once more: + u ln x on the penalty's side.  The second generation
    subtracts v_log_f32(x) itself from scale log2 e q.k (attention.hip:145-148, 458, 950, 1119): 2 u log2 x, the subtraction's u,
    and the way back to natural units is exact in the model (the factor ln 2 of LSE is counted there): 3 u ln x.  Both are within
        e_pen_ij = 6 u max(1, ln|i - j|),      e_s[i] = max over the unmasked j of (2 d u scale (|q| |k|^T)_ij + e_pen_ij).
  * LSE[i] = logsumexp_j s_ij (natural log; m + logf(l) at attention.hip:253, m ln 2 + logf(l) at :544).  A shift of every score by
    <= e_s moves it by <= e_s.  l = sum_j exp(s_j - m): each __expf / v_exp_f32 term is (|s_j - m| + 2) u relative
    (tests/test_attn2d_gpu.py's model: the argument's product by log2 e rounds, the hardware exp is 1 ulp), weighted by its share
    P_j of l: sum_j P_j |s_j - smax| u + 2 u; the Tk terms add in some order: Tk u; every 64-key tile rescales the running l by
    exp(m_old - m_new) and rounds (the exponents add up to <= R = the row's range of unmasked scores): (R + 3 nt) u, nt = Tk / 64
    rounded up; logf(l) with 1 <= l <= Tk: 2 u ln Tk; m carries the product by scale (log2 e) and, second generation, by ln 2:
    3 u |smax|; the final add u |lse|.  Dropout does not enter (l sums the probabilities before the mask), so the same bound holds
    with p_drop > 0:
        e_lse[i] = e_s[i] + 2 u (sum_j P_ij |s_ij - smax_i| + 2 + Tk + R_i + 3 nt + 2 ln Tk + 3 |smax_i| + |lse_i|).
  * O, dQ, dK, dV: attn_check's bounds with d, scale and e_s as above (its docstring has the derivation):
        |dO|  <= 2 (2 e_s + r_p + (Tk + d) u) (P |V|) + r |O|
        |ddV| <= 2 (2 max_i e_s + r_p + Tq u) (P^T |dO|) + r |dV|
        e_p = 2 d u (|dO| |V|^T),  e_D = (d u + r) sum |dO O|,  E = |dS| (2 e_s + 2 r_p) + P (e_p + e_D)
        |ddQ| <= 2 scale (E |K| + (Tk u + r_p) |dS| |K|) + r |dQ|,   dK likewise with Q and Tq.
    The backward is checked from the kernel's own O and LSE (the inputs it is defined on).  The penalty is a constant additive
    bias: the backward sees it only through P.
  * dropout adjoint identity <dO, O(V2)> = <dV, V2> per (head, column): attn_dropout_adjoint of test_routes_gpu.py, |z| <= 6, and
    its negative control (a backward with the mask of another seed must give an RMS z above 6).

The mask, extracted (test_dropout_mask_*): with q = 0 every unmasked probability is positive, so with the one-hot values
V_g[j, c] = [j == g d + c] the forward's O_g[i, c] is non-zero exactly where pair (i, g d + c) was kept.  The mask must equal
K.dropout(ones[B, H, Tq, Tk4], p, seed) != 0 on j < Tk (Tk4 = (Tk + 3) & ~3: drop_index, attention.hip:118-126, and
dropout_kernel, loss_embed.hip:205-222, hash the same flat index and compare the same 16-bit field with th >> 16; the second
generation's drop_pair does that comparison in packed 16-bit arithmetic).  Independence is a condition, not a measurement: two
independent masks agree on a fraction a = (1 - p)^2 + p^2 of n pairs with sd sqrt(a (1 - a) / n); the shapes give n >= 2.5 * 10^4
per compared set, so 6 sd < 0.02.  The keep probability is 1 - (th >> 16) / 65536, within 2^-16 of 1 - p: far below one sd.

s2t_attn_probs_avg (attention.hip:1311-1376): out[b, i, j] = mean over the first heads_used heads of softmax_j(scale q_h . k_h),
0 past klen[b].  Per head: the score is a serial f32 sum of dh products of (q scale, rounded) and k: e_s = (dh + 2) u scale
(|q| . |k|), row maximum E; p moves by 2 E relative; expf (|ln p| + 2) u; the normaliser is 8 serial adds per thread, a 64-lane
and a 4-wave tree: 24 u; 1 / (l heads_used) and the product: 3 u; the heads add serially: heads_used u.  Bound = twice
sum_h p_h / heads_used (2 E_h + (|ln p_h| + 29 + heads_used) u) + 1e-37 (results below 2^-126 may flush).

Layouts (test_layout_*): s2t_attn_fwd leaves attn_fwd2_kernel when o_st % 4, o_sb % 4 or O & 7 (attention.hip:1268) or when
span32 fails for K / V (:1269, :1171-1173); bwd_launch (:1196-1199) drops dq2 / dkv2 on `al` (dQ / dK / dV strides % 4, pointers
& 7), on span32 of the staged operands and, dq2 only, on o_st % 8, o_sb % 8, O & 15.  The profiler counts families, not kernels,
so these cases cite the gates and hold every mix to the same float64 bounds and the same extracted mask.
"""
import contextlib
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
DEV = "cuda"
U32 = 2.0 ** -24                 # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF, F32 = torch.bfloat16, torch.float32
FAMILIES = ("attn_fwd", "attn_bwd")
P_DROP = 0.3


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K
    from fbk_fairseq_st_amd import kernels
    K = kernels
    K._lib()
    yield
    K.prof_enable(0)


# ------------------------------------------------------------------ shared tools (copies of test_routes_gpu.py's)
@contextlib.contextmanager
def set_option(key, value):
    """s2t_set_option for the duration of a `with` block; the previous value is restored even when the block fails"""
    old = K.set_option(key, value)
    try:
        yield old
    finally:
        K.set_option(key, old)


@contextlib.contextmanager
def launches():
    """launch counts per kernel family of everything run inside the block (the library's event-bracketed profiler)"""
    counts = {}
    torch.cuda.synchronize()
    K.prof_reset()
    K.prof_enable(1)
    try:
        yield counts
    finally:
        torch.cuda.synchronize()
        for f in FAMILIES:
            counts[f] = K.prof_read(f)["launches"]
        K.prof_enable(0)
        K.prof_reset()


def d64(t, dev="cpu"):
    return t.detach().to(dev).double()


def r_of(dtype):
    return UBF if dtype == BF else U32


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound (inf for NaN)"""
    ratio = (d64(out, ref.device) - ref).abs() / bound.clamp_min(1e-300)
    return float(torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio).max())


def assert_close(out, ref, bound, what):
    """|out - ref| <= bound element by element (ref, bound float64); on failure: the worst element, its value, ref and bound"""
    o = d64(out, ref.device)
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


def heads(t, H):
    """[T, B, H d] tensor -> float64 [B, H, T, d]"""
    T, B, D = t.shape
    return d64(t).reshape(T, B, H, D // H).permute(1, 2, 0, 3)


def allowed_pairs(B, Tq, Tk, klen, causal):
    """bool [B, 1, Tq, Tk]: the pairs the softmax runs over (keys below klen[b], and not above the diagonal when causal)"""
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if causal:
        ok = ok & ~torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), 1)
    if klen is not None:
        ok = ok & (torch.arange(Tk)[None, :] < klen.cpu().long()[:, None])[:, None, None, :]
    return ok


# ------------------------------------------------------------------ float64 reference and bounds of one attention call
def reference(q, k, v, H, klen, causal, scale, pen):
    """float64 scores, P, LSE and the score error e_s of the module docstring; every tensor [B, H, Tq, .] on the CPU"""
    Q, Kh, V = heads(q, H), heads(k, H), heads(v, H)
    B, _, Tq, d = Q.shape
    Tk = Kh.shape[2]
    ok = allowed_pairs(B, Tq, Tk, klen, causal).expand(B, H, Tq, Tk)
    s = scale * Q @ Kh.transpose(-1, -2)
    e = 2 * d * U32 * scale * (Q.abs() @ Kh.abs().transpose(-1, -2))
    if pen:
        dist = (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).abs().double()
        ln = dist.clamp_min(1).log()                                     # max(0, ln|i - j|), 0 for |i - j| <= 1
        s = s - ln
        e = e + 6 * U32 * ln.clamp_min(1)
    s = s.masked_fill(~ok, -math.inf)
    es = e.masked_fill(~ok, 0).amax(-1, keepdim=True)
    lse = torch.logsumexp(s, -1, keepdim=True)
    P = torch.softmax(s, -1)
    smax = s.amax(-1, keepdim=True)
    smin = s.masked_fill(~ok, math.inf).amin(-1, keepdim=True)
    px = (P * (s - smax).masked_fill(~ok, 0).abs()).sum(-1, keepdim=True)
    nt = (Tk + 63) // 64
    bL = es + 2 * U32 * (px + 2 + Tk + (smax - smin) + 3 * nt + 2 * math.log(Tk) + 3 * smax.abs() + lse.abs())
    return types.SimpleNamespace(Q=Q, K=Kh, V=V, P=P, s=s, es=es, lse=lse, bL=bL, ok=ok, B=B, H=H, Tq=Tq, Tk=Tk, d=d,
                                 scale=scale)


def o_bound(R, dtype):
    rp = r_of(dtype)
    Oref = R.P @ R.V
    return Oref, 2 * (2 * R.es + rp + (R.Tk + R.d) * U32) * (R.P @ R.V.abs()) + r_of(dtype) * Oref.abs()


def check_fwd(R, dtype, o, lse, what, ratios=None):
    Oref, bO = o_bound(R, dtype)
    got = heads(o, R.H)
    if ratios is not None:
        ratios["O"] = max(ratios.get("O", 0.0), worst_ratio(got, Oref, bO))
        ratios["LSE"] = max(ratios.get("LSE", 0.0), worst_ratio(lse.unsqueeze(-1), R.lse, R.bL))
    assert_close(got, Oref, bO, what + " O")
    assert_close(lse.unsqueeze(-1), R.lse, R.bL, what + " LSE")


def check_lse(R, lse, what):
    assert_close(lse.unsqueeze(-1), R.lse, R.bL, what + " LSE")


def check_bwd(R, dtype, o, do, dq, dk, dv, what, ratios=None):
    """dQ, dK, dV against float64 from the kernel's own O (attn_check's bounds with d and scale as parameters)"""
    r, rp, d, scale, Tq, Tk = r_of(dtype), r_of(dtype), R.d, R.scale, R.Tq, R.Tk
    P, es, V, Q, Kh = R.P, R.es, R.V, R.Q, R.K
    dO, O = heads(do, R.H), heads(o, R.H)
    dVr = P.transpose(-1, -2) @ dO
    bV = 2 * (2 * es.amax(-2, keepdim=True) + rp + Tq * U32) * (P.transpose(-1, -2) @ dO.abs()) + r * dVr.abs()
    dP = dO @ V.transpose(-1, -2)
    Dl = (dO * O).sum(-1, keepdim=True)
    dS = P * (dP - Dl)
    ep = 2 * d * U32 * (dO.abs() @ V.abs().transpose(-1, -2))
    eD = (d * U32 + r) * (dO * O).abs().sum(-1, keepdim=True)
    E = dS.abs() * (2 * es + 2 * rp) + P * (ep + eD)
    dQr = scale * dS @ Kh
    dKr = scale * dS.transpose(-1, -2) @ Q
    bQ = 2 * scale * (E @ Kh.abs() + (Tk * U32 + rp) * (dS.abs() @ Kh.abs())) + r * dQr.abs()
    bK = 2 * scale * (E.transpose(-1, -2) @ Q.abs() + (Tq * U32 + rp) * (dS.abs().transpose(-1, -2) @ Q.abs())) + r * dKr.abs()
    for name, got, ref, b in (("dV", dv, dVr, bV), ("dK", dk, dKr, bK), ("dQ", dq, dQr, bQ)):
        if ratios is not None:
            ratios[name] = max(ratios.get(name, 0.0), worst_ratio(heads(got, R.H), ref, b))
        assert_close(heads(got, R.H), ref, b, what + " " + name)


def adjoint_z(R, dtype, do, o2, v2, dv, p):
    """z per (b, h, column) of <dO, O(V2)> - <dV, V2> (attn_dropout_adjoint of test_routes_gpu.py: the variance model is there)"""
    r, rp = r_of(dtype), r_of(dtype)
    dO, O2, V2, dV = heads(do, R.H), heads(o2, R.H), heads(v2, R.H), heads(dv, R.H)
    P2e = R.P ** 2 / (1 - p) * (2 * R.es + rp) ** 2
    rO, rV = r + 4 * (R.Tk + R.d) * U32, r + 4 * (R.Tq + R.d) * U32
    lhs = (dO * O2).sum(-2)
    varO = P2e @ (V2 * V2) + (rO * O2) ** 2
    varV = P2e.transpose(-1, -2) @ (dO * dO) + (rV * dV) ** 2
    sd = ((dO * dO * varO).sum(-2) + (V2 * V2 * varV).sum(-2)).sqrt()
    return (lhs - (dV * V2).sum(-2)) / sd


def check_adjoint(R, dtype, do, o2, v2, dv_same, dv_other, p, what):
    z = adjoint_z(R, dtype, do, o2, v2, dv_same, p)
    i = int(z.abs().reshape(-1).argmax())
    assert float(z.abs().max()) <= 6, "%s: <dO, O(V2)> != <dV, V2> for (b, h, c) %s: z = %.3g" % (
        what, tuple(int(x) for x in torch.unravel_index(torch.tensor(i), z.shape)), float(z.reshape(-1)[i]))
    zw = adjoint_z(R, dtype, do, o2, v2, dv_other, p)
    rms = float((zw * zw).mean().sqrt())
    assert rms > 6, "%s: a backward with another dropout mask passes the check (rms z %.3g)" % (what, rms)


# ------------------------------------------------------------------ one case on the device
def inputs(dtype, d, H, B, Tq, Tk, seed=None):
    """q, k, v as slices of one fused [T, B, 3 H d] buffer (the layout the engine passes), dO contiguous"""
    D = H * d
    g = torch.Generator().manual_seed(Tq * 7 + Tk if seed is None else seed)
    qkv = (torch.randn(max(Tq, Tk), B, 3 * D, generator=g) * 0.7).to(dtype).to(DEV)
    do = torch.randn(Tq, B, D, generator=g).to(dtype).to(DEV)
    return qkv[:Tq, :, :D], qkv[:Tk, :, D:2 * D], qkv[:Tk, :, 2 * D:], do


def ragged_klen(B, Tk):
    """full, a few short, ..., and klen = 1 last"""
    return torch.tensor([1 if i == B - 1 else max(1, Tk - 5 * i) for i in range(B)], dtype=torch.int32)


class Layout:
    """where the outputs of a case live; the default is what the wrappers allocate (contiguous, aligned)"""
    def out(self, q):
        return torch.empty_like(q, memory_format=torch.contiguous_format)

    def grads(self, q, k, v):
        c = torch.contiguous_format
        return torch.empty_like(q, memory_format=c), torch.empty_like(k, memory_format=c), torch.empty_like(v, memory_format=c)

    def kv(self, k, v):
        return k, v


class OutOffset(Layout):
    """O is a view that starts `off` elements into its buffer"""
    def __init__(self, off):
        self.off = off

    def out(self, q):
        buf = torch.empty(q.numel() + 16, dtype=q.dtype, device=q.device)
        assert buf.data_ptr() % 16 == 0
        return buf[self.off:self.off + q.numel()].view(q.shape)


class GradStride(Layout):
    """dQ, dK, dV are the [:, :, :D] slices of [T, B, D + 2] buffers: a batch stride of D + 2 elements"""
    def grads(self, q, k, v):
        return tuple(torch.empty(t.shape[0], t.shape[1], t.shape[2] + 2, dtype=t.dtype, device=t.device)[:, :, :t.shape[2]]
                     for t in (q, k, v))


class FarRows(Layout):
    """K and V rows 2^23 elements (16 MiB) apart in one buffer: past span32's 24-bit row stride"""
    STRIDE = 1 << 23

    def kv(self, k, v):
        Tk, B, D = k.shape
        big = torch.empty((Tk - 1) * self.STRIDE + 2 * B * D, dtype=k.dtype, device=k.device)
        kf = torch.as_strided(big, (Tk, B, D), (self.STRIDE, 2 * D, 1), 0)
        vf = torch.as_strided(big, (Tk, B, D), (self.STRIDE, 2 * D, 1), D)
        kf.copy_(k)
        vf.copy_(v)
        return kf, vf


def attn_case(dtype, d, H, B, Tq, Tk, klen, causal, scale, pen, what, layout=None, ratios=None, drop_seed=77):
    """forward + backward element by element against float64, LSE with and without dropout, the dropout adjoint identity with
    its negative control, and (pen) the negative control of the penalty.  Returns the launch counts of the plain fwd + bwd."""
    layout = layout or Layout()
    q, k0, v0, do = inputs(dtype, d, H, B, Tq, Tk)
    k, v = layout.kv(k0, v0)
    kl = klen.to(DEV) if klen is not None else None
    kw = dict(klen=kl, causal=causal, scale=scale, dist_penalty=pen)
    with launches() as c:
        o, lse = K.attn_fwd(q, k, v, H, out=layout.out(q), **kw)
        dq, dk, dv = layout.grads(q, k0, v0)
        K.attn_bwd(q, k, v, o, do, lse, H, dq, dk, dv, **kw)
    assert c["attn_fwd"] == 1 and c["attn_bwd"] == 1, c
    R = reference(q, k0, v0, H, klen, causal, scale, pen)
    check_fwd(R, dtype, o, lse, what, ratios)
    check_bwd(R, dtype, o, do, dq, dk, dv, what, ratios)
    if pen:                                                  # the bound sees the penalty: the unpenalised reference must miss it
        R0 = reference(q, k0, v0, H, klen, causal, scale, False)
        Oref0, bO0 = o_bound(R0, dtype)
        assert bool(((heads(o, H) - Oref0).abs() > bO0).any()), what + ": outputs with the penalty pass the unpenalised O bound"
    # dropout: same LSE, and forward and backward drop the same pairs
    seed = drop_seed
    g = torch.Generator().manual_seed(77)
    v2c = (torch.randn(v0.shape, generator=g) * 0.7).to(dtype).to(DEV)
    _, v2 = layout.kv(k0, v2c)
    o1, lse1 = K.attn_fwd(q, k, v, H, out=layout.out(q), p_drop=P_DROP, seed=seed, **kw)
    o2, lse2 = K.attn_fwd(q, k, v2, H, out=layout.out(q), p_drop=P_DROP, seed=seed, **kw)
    check_lse(R, lse1, what + " p=%.1f" % P_DROP)
    check_lse(R, lse2, what + " p=%.1f (V2)" % P_DROP)

    def dv_of(bseed):
        gq, gk, gv = layout.grads(q, k0, v0)
        K.attn_bwd(q, k, v, o1, do, lse1, H, gq, gk, gv, p_drop=P_DROP, seed=bseed, **kw)
        return gv
    check_adjoint(R, dtype, do, o2, v2c, dv_of(seed), dv_of(seed + 1), P_DROP, what)
    return c


# ------------------------------------------------------------------ 1. head width 32, element-wise
D32_SHAPES = [
    # Tq, Tk, ragged, causal
    (64, 64, False, False),            # a single 64-row tile
    (63, 65, True, False), (65, 63, False, False), (64, 63, True, False), (63, 64, False, False),
    (65, 65, True, True),
    (33, 61, False, False), (70, 66, True, False),          # Tk % 4 = 1, 2: the dropout quad padding (Tk + 3) & ~3
    (9, 200, True, False), (257, 129, True, False),         # cross-attention shapes
    (130, 130, True, True),
]


@pytest.mark.parametrize("unit_scale", [False, True], ids=["scale_rsqrt_d", "scale_1"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("idx", range(len(D32_SHAPES)), ids=["Tq%d_Tk%d%s%s" % (s[0], s[1], "_ragged" if s[2] else "",
                                                                                  "_causal" if s[3] else "") for s in D32_SHAPES])
def test_d32_elementwise(idx, dtype, unit_scale):
    """ACfg<T, 32> (attn_fwd_kernel, attn_delta_kernel, attn_bwd_dkv_kernel, attn_bwd_dq_kernel: every d = 32 call runs the first
    generation, attention.hip:1268 needs head_dim == 64) with scale = d^-1/2 and scale = 1 (the ConvAttention2D call), H 4 / 8,
    every element of O, LSE, dQ, dK, dV and the dropout adjoint identity"""
    Tq, Tk, ragged, causal = D32_SHAPES[idx]
    H, B = (4, 3) if idx % 2 == 0 else (8, 3)
    klen = ragged_klen(B, Tk) if ragged else None
    attn_case(dtype, 32, H, B, Tq, Tk, klen, causal, 1.0 if unit_scale else 32 ** -0.5, False,
              "d32 %s H%d Tq%d Tk%d" % ("bf16" if dtype == BF else "f32", H, Tq, Tk))


# ------------------------------------------------------------------ 2. distance penalty
PEN_CASES = [
    # id, dtype, d, H, B, Tq, Tk, ragged, causal, attn_v1
    ("bf16_d64_gen2", BF, 64, 4, 2, 200, 200, True, False, 0),
    ("bf16_d64_gen2_Tq256_Tk130", BF, 64, 4, 2, 256, 130, True, False, 0),
    ("bf16_d64_gen2_causal", BF, 64, 2, 3, 130, 130, True, True, 0),
    ("bf16_d64_fwd2_dq2_with_gen1_dkv", BF, 64, 4, 2, 200, 100, True, False, 0),
    ("bf16_d64_attn_v1", BF, 64, 4, 2, 200, 200, True, False, 1),
    ("bf16_d64_T_below_128", BF, 64, 2, 3, 100, 90, True, False, 0),
    ("f32_d64", F32, 64, 4, 2, 200, 200, True, False, 0),
    ("f32_d64_causal_Tq70_Tk130", F32, 64, 2, 3, 70, 130, False, True, 0),
    ("bf16_d32", BF, 32, 4, 2, 200, 200, True, False, 0),
    ("bf16_d32_causal", BF, 32, 4, 2, 65, 63, False, True, 0),
    ("f32_d32_Tq130_Tk257", F32, 32, 8, 2, 130, 257, True, False, 0),
]


@pytest.mark.parametrize("case", PEN_CASES, ids=[c[0] for c in PEN_CASES])
def test_distance_penalty(case):
    """every kernel that reads dist_pen.  bf16 d = 64 takes attn_fwd2_kernel when Tq >= 128 || (Tq >= attn_v2_min_tq && Tk >= 128)
    and attn_v1 == 0 (attention.hip:1268-1269), where the penalty makes `plain` false (:372: the non-FAST softmax) and the
    backward's `generic` true (:892, :1079: the EDGE tiles); dq2 follows the forward's rule, dkv2 needs Tk >= 128 (:1198-1199), so
    Tq 200 / Tk 100 runs the second-generation forward and dQ with the first-generation dK/dV in one call.  attn_v1 = 1, T < 128,
    f32 and d = 32 run the first generation (__logf at :199, :633, :733).  One launch of each family per call; every element of
    O, LSE, dQ, dK, dV, the dropout adjoint identity at p = 0.3, and the unpenalised reference as negative control"""
    name, dtype, d, H, B, Tq, Tk, ragged, causal, v1 = case
    klen = ragged_klen(B, Tk) if ragged else None
    with set_option("attn_v1", v1):
        attn_case(dtype, d, H, B, Tq, Tk, klen, causal, d ** -0.5, True, "penalty " + name)


# ------------------------------------------------------------------ 3. the dropout mask, extracted
def extract_mask(dtype, d, H, B, Tq, Tk, p, seed, klen=None, causal=False, pen=False, layout=None):
    """keep[b, h, i, j] read off the forward's output (module docstring); bool on the CPU"""
    layout = layout or Layout()
    D = H * d
    q = torch.zeros(Tq, B, D, dtype=dtype, device=DEV)
    k0 = torch.zeros(Tk, B, D, dtype=dtype, device=DEV)
    kl = klen.to(DEV) if klen is not None else None
    keep = torch.zeros(B, H, Tq, Tk, dtype=torch.bool)
    for g in range((Tk + d - 1) // d):
        j = torch.arange(g * d, min(Tk, (g + 1) * d))
        v0 = torch.zeros(Tk, B, H, d, dtype=dtype, device=DEV)
        v0[j, :, :, j - g * d] = 1
        k, v = layout.kv(k0, v0.view(Tk, B, D))
        o, _ = K.attn_fwd(q, k, v, H, klen=kl, causal=causal, p_drop=p, seed=seed, dist_penalty=pen, out=layout.out(q))
        keep[:, :, :, j] = (o.view(Tq, B, H, d)[..., :len(j)] != 0).permute(1, 2, 0, 3).cpu()
    return keep


def expected_mask(B, H, Tq, Tk, p, seed):
    """s2t_dropout's keep decisions on the flat index space [B, H, Tq, Tk4] of drop_index, restricted to j < Tk"""
    Tk4 = (Tk + 3) & ~3
    ones = torch.ones(B, H, Tq, Tk4, dtype=F32, device=DEV)
    return (K.dropout(ones, p, seed) != 0)[..., :Tk].cpu()


def binomial_ok(frac, expect, n, what):
    sd = math.sqrt(expect * (1 - expect) / n)
    assert abs(frac - expect) <= 6 * sd, "%s: fraction %.5f, expected %.5f +- %.5f (6 sd, n = %d)" % (what, frac, expect, 6 * sd, n)


def agreement(a, b, what, p=P_DROP):
    """two independent masks agree on (1 - p)^2 + p^2 of their pairs, within 6 binomial standard deviations"""
    n = a.numel()
    assert n >= 25000, (what, n)
    binomial_ok(float((a == b).double().mean()), (1 - p) ** 2 + p ** 2, n, what)


def independence(keep, what, p=P_DROP):
    B, H, Tq, Tk = keep.shape
    for b in range(B):
        for h in range(H):
            binomial_ok(float(keep[b, h].double().mean()), 1 - p, Tq * Tk, "%s keep fraction of (b, h) = (%d, %d)" % (what, b, h))
    for h in range(H - 1):
        agreement(keep[:, h], keep[:, h + 1], "%s heads %d / %d" % (what, h, h + 1), p)
    for b in range(B - 1):
        agreement(keep[b], keep[b + 1], "%s batch entries %d / %d" % (what, b, b + 1), p)
    agreement(keep[:, :, :-1], keep[:, :, 1:], what + " neighbouring query rows", p)
    agreement(keep[:, :, 0::2][:, :, :Tq // 2], keep[:, :, 1::2][:, :, :Tq // 2], what + " even / odd query rows", p)
    agreement(keep[..., :-1], keep[..., 1:], what + " neighbouring keys", p)


def test_dropout_mask_is_one_definition_across_kernels_and_s2t_dropout():
    """f32 first generation, bf16 first generation (attn_v1 = 1) and bf16 second generation (B H = 8: head_xcd_remap's permuted
    head order) at one seed: the three extracted masks are equal, equal s2t_dropout's on the same flat index, every allowed pair is
    seen without dropout, and heads, batch entries, query rows, keys and seeds are independent"""
    B, H, Tq, Tk, d, seed = 2, 4, 192, 192, 64, 1234
    full = allowed_pairs(B, Tq, Tk, None, False).expand(B, H, Tq, Tk)
    assert bool((extract_mask(BF, d, H, B, Tq, Tk, 0.0, seed) == full).all()), "without dropout every pair must be visible"
    want = expected_mask(B, H, Tq, Tk, P_DROP, seed)
    m_f32 = extract_mask(F32, d, H, B, Tq, Tk, P_DROP, seed)
    with set_option("attn_v1", 1):
        m_bf1 = extract_mask(BF, d, H, B, Tq, Tk, P_DROP, seed)
    m_bf2 = extract_mask(BF, d, H, B, Tq, Tk, P_DROP, seed)
    assert bool((m_bf1 == m_bf2).all()), "bf16 first- and second-generation masks differ in %d pairs" % int((m_bf1 != m_bf2).sum())
    for name, m in (("f32 first generation", m_f32), ("bf16 first generation", m_bf1), ("bf16 second generation", m_bf2)):
        assert bool((m == want).all()), "%s: %d pairs differ from s2t_dropout's mask" % (name, int((m != want).sum()))
    independence(m_bf2, "bf16 second generation")
    other = extract_mask(BF, d, H, B, Tq, Tk, P_DROP, seed + 1)
    assert bool((other == expected_mask(B, H, Tq, Tk, P_DROP, seed + 1)).all())
    agreement(m_bf2, other, "seeds %d / %d" % (seed, seed + 1))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_dropout_mask_d32(dtype):
    """head width 32 (six key groups of 32), H = 8"""
    B, H, Tq, Tk, seed = 2, 8, 160, 192, 99
    m = extract_mask(dtype, 32, H, B, Tq, Tk, P_DROP, seed)
    want = expected_mask(B, H, Tq, Tk, P_DROP, seed)
    assert bool((m == want).all()), "%d pairs differ from s2t_dropout's mask" % int((m != want).sum())
    independence(m, "d32")


@pytest.mark.parametrize("v1", [0, 1])
def test_dropout_mask_with_penalty_ragged_keys_and_tk_not_a_multiple_of_4(v1):
    """Tk = 190 (row pitch Tk4 = 192 in the index), ragged klen, the distance penalty (second generation: the non-FAST softmax
    with drop_hash4 on the full quad index, attention.hip:490): the mask is s2t_dropout's on the allowed pairs, and keys past
    klen[b] give exact zeros"""
    B, H, Tq, Tk, d, seed = 2, 4, 192, 190, 64, 5
    klen = torch.tensor([Tk, 101], dtype=torch.int32)
    ok = allowed_pairs(B, Tq, Tk, klen, False).expand(B, H, Tq, Tk)
    want = expected_mask(B, H, Tq, Tk, P_DROP, seed) & ok
    with set_option("attn_v1", v1):
        for pen in (False, True):
            assert bool((extract_mask(BF, d, H, B, Tq, Tk, 0.0, seed, klen=klen, pen=pen) == ok).all()), "pen=%d: visibility" % pen
            m = extract_mask(BF, d, H, B, Tq, Tk, P_DROP, seed, klen=klen, pen=pen)
            assert bool((m == want).all()), "pen=%d: %d pairs differ from s2t_dropout's mask" % (pen, int((m != want).sum()))
    m = extract_mask(F32, d, H, B, Tq, Tk, P_DROP, seed, klen=klen, pen=True)
    assert bool((m == want).all()), "f32: %d pairs differ from s2t_dropout's mask" % int((m != want).sum())
    independence(want[:1], "Tk 190, full-length batch entry")


@pytest.mark.parametrize("dtype,v1", [(F32, 0), (BF, 0), (BF, 1)], ids=["f32", "bf16_gen2", "bf16_gen1"])
def test_dropout_mask_causal(dtype, v1):
    """causal: future keys give exact zeros, the rest is s2t_dropout's mask (second generation: `plain` is false, :372)"""
    B, H, Tq, Tk, d, seed = 2, 2, 130, 130, 64, 31
    ok = allowed_pairs(B, Tq, Tk, None, True).expand(B, H, Tq, Tk)
    want = expected_mask(B, H, Tq, Tk, P_DROP, seed) & ok
    with set_option("attn_v1", v1):
        m = extract_mask(dtype, d, H, B, Tq, Tk, P_DROP, seed, causal=True)
    assert bool((m == want).all()), "%d pairs differ from s2t_dropout's mask" % int((m != want).sum())


HIGH_SEED = (5 << 32) | 7          # the seed is a 64-bit argument: its upper word must reach the hash in every kernel
HIGH_SEED_CASES = [
    # id, dtype, d, attn_v1, penalty, causal
    ("f32_gen1", F32, 64, 0, False, False), ("bf16_gen1", BF, 64, 1, False, False), ("bf16_gen2_fast_index", BF, 64, 0, False, False),
    ("bf16_gen2_general_index", BF, 64, 0, True, False), ("bf16_gen2_causal", BF, 64, 0, False, True), ("bf16_d32", BF, 32, 0, False, False),
]


@pytest.mark.parametrize("case", HIGH_SEED_CASES, ids=[c[0] for c in HIGH_SEED_CASES])
def test_dropout_mask_seed_above_32_bits(case):
    """the kernels take the seed's scramble and its upper word once per launch or tile (drop_seed_key / drop_high_mix) where s2t_dropout
    takes them per quad: at a seed above 2^32 the extracted mask is still s2t_dropout's, and is not the mask of the seed's low word.
    The shape of test_dropout_mask_causal, the smallest above"""
    _, dtype, d, v1, pen, causal = case
    B, H, Tq, Tk = 2, 2, 130, 130
    ok = allowed_pairs(B, Tq, Tk, None, causal).expand(B, H, Tq, Tk)
    want = expected_mask(B, H, Tq, Tk, P_DROP, HIGH_SEED) & ok
    with set_option("attn_v1", v1):
        m = extract_mask(dtype, d, H, B, Tq, Tk, P_DROP, HIGH_SEED, causal=causal, pen=pen)
    assert bool((m == want).all()), "%d pairs differ from s2t_dropout's mask" % int((m != want).sum())
    low = expected_mask(B, H, Tq, Tk, P_DROP, HIGH_SEED & 0xFFFFFFFF) & ok
    assert not bool((m == low).all()), "the seed's upper word does not reach the mask"


ADJOINT_HIGH_SEED = [
    # id, dtype, d, attn_v1, Tq, Tk
    ("f32_gen1", F32, 64, 0, 130, 130), ("bf16_gen1", BF, 64, 1, 130, 130), ("bf16_gen2", BF, 64, 0, 130, 130),
    ("bf16_fwd2_dq2_with_gen1_dkv", BF, 64, 0, 200, 100), ("bf16_d32", BF, 32, 0, 65, 63),
]


@pytest.mark.parametrize("case", ADJOINT_HIGH_SEED, ids=[c[0] for c in ADJOINT_HIGH_SEED])
def test_backward_drops_the_forwards_pairs_at_a_seed_above_32_bits(case):
    """attn_case with the dropout seed above 2^32: dQ and dK/dV kernels of both generations take the upper word as the forward does
    (the adjoint identity holds with the forward's seed and fails with another)"""
    name, dtype, d, v1, Tq, Tk = case
    with set_option("attn_v1", v1):
        attn_case(dtype, d, 2, 2, Tq, Tk, None, False, d ** -0.5, False, "64-bit seed " + name, drop_seed=HIGH_SEED)


# ------------------------------------------------------------------ 4. s2t_attn_probs_avg
def probs_ref(q, k, H, klen, scale, hu):
    """float64 mean over the first hu heads of the key-masked softmax, and its bound (module docstring); [B, Tq, Tk]"""
    Q, Kh = heads(q, H)[:, :hu], heads(k, H)[:, :hu]
    B, _, Tq, dh = Q.shape
    Tk = Kh.shape[2]
    ok = allowed_pairs(B, Tq, Tk, klen, False).expand(B, hu, Tq, Tk)
    s = (scale * Q @ Kh.transpose(-1, -2)).masked_fill(~ok, -math.inf)
    E = ((dh + 2) * U32 * scale * (Q.abs() @ Kh.abs().transpose(-1, -2))).masked_fill(~ok, 0).amax(-1, keepdim=True)
    P = torch.softmax(s, -1)
    P = torch.where(ok, P, torch.zeros_like(P))                      # klen = 0: softmax of an empty row is NaN; the kernel gives 0
    lnp = torch.where(P > 0, P.clamp_min(1e-300).log().abs(), torch.zeros_like(P))
    bound = 2 * (P / hu * (2 * E + (lnp + 29 + hu) * U32)).sum(1) + 1e-37
    return P.sum(1) / hu, bound


def probs_case(dtype, dh, H, B, Tq, Tk, hu, klen, scale, what, ratios=None):
    D = H * dh
    g = torch.Generator().manual_seed(Tk * 3 + Tq + hu)
    qkv = (torch.randn(Tq, B, 3 * D, generator=g) * 0.9).to(dtype).to(DEV)          # Q = a slice of a fused QKV buffer
    kv = (torch.randn(Tk, B, 2 * D, generator=g) * 0.9).to(dtype).to(DEV)           # K = the [:, :, :D] slice of a [Tk, B, 2D] buffer
    q, k = qkv[:, :, :D], kv[:, :, :D]
    kl = klen.to(DEV) if klen is not None else None
    out = K.attn_probs_avg(q, k, H, klen=kl, scale=scale, heads_used=hu)
    assert out.shape == (B, Tq, Tk) and out.dtype == F32
    assert not bool(torch.isnan(out).any()), what + ": NaN in the output (an element not written, or 0 / 0)"
    ref, bound = probs_ref(q, k, H, klen, dh ** -0.5 if scale is None else scale, hu)
    if ratios is not None:
        ratios["probs"] = max(ratios.get("probs", 0.0), worst_ratio(out, ref, bound))
    assert_close(out, ref, bound, what)
    o = d64(out)
    lens = klen.long() if klen is not None else torch.full((B,), Tk)
    for b in range(B):
        n = int(lens[b])
        assert bool((o[b, :, n:] == 0).all()), "%s: non-zero probability past klen[%d] = %d" % (what, b, n)
        if n == 0:
            assert bool((o[b] == 0).all()), "%s: klen = 0 must give an all-zero block" % what
        else:
            assert bool(((o[b].sum(-1) - 1).abs() <= bound[b].sum(-1)).all()), "%s: rows of batch entry %d do not sum to 1" % (what, b)
    return out


@pytest.mark.parametrize("Tk", [1, 255, 256, 257, 375, 2048])
@pytest.mark.parametrize("Tq", [1, 40])
@pytest.mark.parametrize("dtype,dh", [(F32, 64), (BF, 64), (F32, 32), (BF, 32)], ids=["f32_dh64", "bf16_dh64", "f32_dh32", "bf16_dh32"])
def test_attn_probs_avg(dtype, dh, Tq, Tk):
    """the keys-per-thread boundaries (256 i) and the 2048 limit, a decode step (Tq = 1) and a block of 40 queries; heads_used 1,
    H - 1 and H; strided Q / K views; the default and an explicit scale; ragged klen with klen[b] = 0 and klen[b] = 1"""
    H, B = 4, 3
    for hu in (1, H - 1, H):
        probs_case(dtype, dh, H, B, Tq, Tk, hu, None, None, "probs hu=%d" % hu)
    klen = torch.tensor([Tk, max(1, Tk - 7) if Tk > 1 else 0, 0 if Tk > 1 else 1], dtype=torch.int32)
    probs_case(dtype, dh, H, B, Tq, Tk, H - 1, klen, 0.37, "probs ragged, scale 0.37")
    if Tk > 256:
        klen = torch.tensor([256, 257, 1], dtype=torch.int32)
        probs_case(dtype, dh, H, B, Tq, Tk, H, klen, None, "probs klen at the thread boundary")


def test_attn_probs_avg_writes_every_element():
    """the wrapper's output comes from torch.empty: run the C entry point on a buffer pre-filled with NaN"""
    from fbk_fairseq_st_amd import lib as L
    H, dh, B, Tq, Tk = 4, 64, 2, 3, 300
    D = H * dh
    q = (torch.randn(Tq, B, D) * 0.9).to(BF).to(DEV)
    k = (torch.randn(Tk, B, D) * 0.9).to(BF).to(DEV)
    klen = torch.tensor([Tk, 17], dtype=torch.int32, device=DEV)
    out = torch.full((B, Tq, Tk), math.nan, dtype=F32, device=DEV)
    L.check(K._lib().s2t_attn_probs_avg(L.dt(q), dh, B, H, Tq, Tk, L.ptr(q), q.stride(0), q.stride(1), L.ptr(k), k.stride(0),
                                        k.stride(1), L.ptr(klen), H, float(dh ** -0.5), L.ptr(out), L.stream()), "s2t_attn_probs_avg")
    assert not bool(torch.isnan(out).any()), "%d elements were not written" % int(torch.isnan(out).sum())
    ref, bound = probs_ref(q, k, H, klen.cpu(), dh ** -0.5, H)
    assert_close(out, ref, bound, "probs into a NaN buffer")


def test_attn_probs_avg_refuses_more_than_2048_keys():
    """eight keys per thread of 256: Tk = 2049 is an error (S2T_ENOTSUP through L.check), not a truncated answer"""
    from fbk_fairseq_st_amd import lib as L
    q = torch.zeros(1, 1, 128, dtype=F32, device=DEV)
    k = torch.zeros(2049, 1, 128, dtype=F32, device=DEV)
    with pytest.raises(L.S2THipError, match="not supported"):
        K.attn_probs_avg(q, k, 2)


# ------------------------------------------------------------------ 5. layouts that leave the second generation
def test_layout_aligned_baseline():
    """the shape of the layout cases with everything aligned: the second generation throughout"""
    attn_case(BF, 64, 4, 2, 256, 256, ragged_klen(2, 256), False, 64 ** -0.5, False, "aligned")


@pytest.mark.parametrize("off", [4, 2])
def test_layout_o_offset(off):
    """O starts 4 elements (8 bytes) into its buffer: the forward stays on attn_fwd2_kernel (O & 7 == 0, attention.hip:1268) and the
    backward loses dq2 (O & 15, :1199): attn_delta_kernel + first-generation dQ next to dkv2.  2 elements (4 bytes): the forward
    leaves too.  Same bounds, same mask"""
    B, H, Tq, Tk = 2, 4, 256, 256
    attn_case(BF, 64, H, B, Tq, Tk, ragged_klen(B, Tk), False, 64 ** -0.5, False, "O + %d elements" % off, layout=OutOffset(off))
    m = extract_mask(BF, 64, H, B, Tq, Tk, P_DROP, 8, layout=OutOffset(off))
    want = expected_mask(B, H, Tq, Tk, P_DROP, 8)
    assert bool((m == want).all()), "%d pairs differ from s2t_dropout's mask" % int((m != want).sum())


def test_layout_gradient_batch_stride_not_a_multiple_of_4():
    """dQ / dK / dV with a batch stride of D + 2 elements fail `al` (attention.hip:1194-1195): the whole backward runs the first
    generation after a second-generation forward; the padding columns of the gradient buffers stay untouched"""
    B, H, Tq, Tk = 2, 4, 256, 256
    attn_case(BF, 64, H, B, Tq, Tk, ragged_klen(B, Tk), False, 64 ** -0.5, False, "grad stride D + 2", layout=GradStride())
    q, k, v, do = inputs(BF, 64, H, B, Tq, Tk)
    o, lse = K.attn_fwd(q, k, v, H)
    bufs = [torch.full((T, B, H * 64 + 2), 7.0, dtype=BF, device=DEV) for T in (Tq, Tk, Tk)]
    K.attn_bwd(q, k, v, o, do, lse, H, *[b[:, :, :H * 64] for b in bufs])
    for b in bufs:
        assert bool((b[:, :, H * 64:] == 7.0).all()), "a gradient kernel wrote outside its [:, :, :D] view"


def test_layout_kv_rows_16_mib_apart():
    """K / V time stride 2^23 elements: span32 (attention.hip:1171-1173) fails, so the forward and dQ run the first generation (64-bit
    row addresses) while dkv2 (which stages Q / dO) stays.  Tk = 128: a 2 GiB buffer"""
    B, H, Tq, Tk = 2, 4, 256, 128
    try:
        probe = torch.empty((Tk - 1) * FarRows.STRIDE + 2 * B * H * 64, dtype=BF, device=DEV)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a 2 GiB K / V buffer on this device")
    del probe
    attn_case(BF, 64, H, B, Tq, Tk, ragged_klen(B, Tk), False, 64 ** -0.5, False, "K/V rows 16 MiB apart", layout=FarRows())
    m = extract_mask(BF, 64, H, B, Tq, Tk, P_DROP, 8, layout=FarRows())
    want = expected_mask(B, H, Tq, Tk, P_DROP, 8)
    assert bool((m == want).all()), "%d pairs differ from s2t_dropout's mask" % int((m != want).sum())


def test_layout_strides_that_fail_strides_ok_are_refused():
    """q / k / v / dO strides must be multiples of a 16-byte vector (strides_ok, attention.hip:1174-1178): S2T_EINVAL, no launch"""
    from fbk_fairseq_st_amd import lib as L
    B, H, Tq, Tk, D = 2, 4, 256, 256, 256
    q, k, v, do = inputs(BF, 64, H, B, Tq, Tk)
    qbad = torch.zeros(Tq, B, D + 4, dtype=BF, device=DEV)[:, :, :D]
    with launches() as c:
        with pytest.raises(L.S2THipError, match="invalid argument"):
            K.attn_fwd(qbad, k, v, H)
        o, lse = K.attn_fwd(q, k, v, H)
        dq, dk, dv = torch.empty_like(o), torch.empty_like(o), torch.empty_like(o)
        dobad = torch.zeros(Tq, B, D + 4, dtype=BF, device=DEV)[:, :, :D]
        with pytest.raises(L.S2THipError, match="invalid argument"):
            K.attn_bwd(q, k, v, o, dobad, lse, H, dq, dk, dv)
        f32bad = torch.zeros(Tq, B, D + 2, dtype=F32, device=DEV)[:, :, :D]
        with pytest.raises(L.S2THipError, match="invalid argument"):
            K.attn_fwd(f32bad, f32bad, f32bad, H)
    assert c["attn_fwd"] == 1 and c["attn_bwd"] == 0, c
