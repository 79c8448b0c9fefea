"""The ConvAttention2D kernels of csrc/attn2d.hip against float64 references: the grouped BatchNorm statistics
(s2t_a2d_chan_stats), BN + ReLU (+ residual) (s2t_a2d_bn_act), its backward (s2t_a2d_bn_bwd, s2t_a2d_param_grads), the weight
packing (s2t_a2d_pack_w), the VALU time attention (s2t_a2d_time_fwd / _bwd), the frequency attention (s2t_a2d_freq_fwd / _bwd),
the one-pass weight gradient of the two 3x3 convolutions (s2t_a2d_conv_wgrad), the plane layout change of the MFMA time-attention
route (s2t_a2d_planes), and one whole block through Engine.attn2d_block_fwd / attn2d_block_bwd on both time-attention routes.

Conventions of tests/test_subsample_gpu.py: every reference is float64 of the exact values the kernel received (its stored bf16 /
f32 tensors, the f32 lse / A / BatchNorm constants and the double sums it was given); every output ELEMENT is compared with a bound
derived from the arithmetic the kernel does, and a failure names the worst element.  The time attention records the launch family
"attn2d", the MFMA route "attn_fwd" / "attn_bwd" (K.prof_read); the BatchNorm pieces choose their vectorised or scalar form at
a2d_vec_ok (attn2d.hip:702, used at the dispatches of s2t_a2d_chan_stats / bn_act / bn_bwd), which each case forces by its row
stride or by a pointer that is not 16-byte aligned.

Error model (u = 2^-24; r = 2^-8 for a bf16 output, u for f32; gamma_n = n u / (1 - n u)).  A sum of terms t along an f32 chain of
depth d errs by <= gamma_d sum |t|; the double sums add <= 2^-40 sum |t|.  Every bound below is TWICE the derived one (first-order
terms only are derived), plus the output rounding r (|ref| + e).
  * a2d_chan_stats: f32 runs of <= 64 rows per thread, then double: mode 0 terms x = prescale z (1 rounding) and x^2 (2 more):
    66 u sum |x|, 68 u sum x^2.  Mode 1 terms g = dy [x sc + sf > 0] and g (x - mean) rstd: 64 u sum |g|, 69 u sum |g| rstd
    (|x - mean| + |x|).  The ReLU mask is a comparison of an f32 value: where |x sc + sf| <= 8 u (|x sc| + |sf|) the f32 and the
    float64 decision may differ, and the inputs zero dy there (the tests build no ambiguous element).
  * a2d_bn_act: x sc + sf with prescale: 3 roundings, 3 u (|z ps sc| + |sf|); the residual add u (|relu| + |res|).
  * a2d_bn_bwd: m0, m1 = sums / count rounded to f32, x = ps z, (x - mean), two products, two subtractions:
    e_o = 4 u (|g| + |m0| + rstd |m1| (|x - mean| + |x|)); then two products by sc and ps: |sc ps| e_o + 2 u |o sc ps|.
  * time attention (one thread per query, attn2d.hip:289-454): scores s = q.k over F in four chains: e_s = gamma_F sum |q k|.
    __expf(x) = 2^(x log2 e): the product's rounding moves the result by |x| u relative, the hardware exp by 2 u: (|x| + 2) u.
    lse (online max / normaliser, T serial terms, <= T rescales whose exponents add up to <= the row's score range R):
    e_lse = max_j e_s + (3T + 2R + 8 + 3 |lse| + 20) u.  With the kernel's OWN lse as the reference's input, P = exp(s - lse)
    errs by eps = e_s + (|s - lse| + 3) u relative (+ 2 u for 1 / (1 - p)), and O = sum_j P v along T serial terms:
    e_O = sum_j eps P |v| + (T + 1) u sum_j P |v|.  delta = dO . O over F: gamma_F sum |dO O|.  dS = P (dP kf - delta) with
    e_dS = P (eps |dP kf - delta| + kf (e_dP + 2 u |dP|) + e_delta + 2 u (|dP kf| + |delta|)), e_dP = gamma_F sum |dO v|;
    dq = sum_j dS k, dk = sum_i dS q, dv = sum_i P kf dO, each along T serial terms: + (T + 1) u of the sum of |terms|.
  * frequency attention (one workgroup per plane, attn2d.hip:483-569): S = sum_t q k along all T frames in ONE serial chain:
    e_S = gamma_T sum_t |q k|.  Large T makes S large (hundreds at T = 1000) and A close to one-hot, but the softmax of S + delta
    with |delta| <= E1 = max_f2 e_S moves every A entry by <= 2 E1 relative, whatever the spread; exp adds (|S - m| + 2) u, the
    normaliser (sum_f2 A |S - m|) + F u, the division u: eps_A = 2 E1 + (|S - m| + sum A |S - m| + F + 6) u, plus 1e-37 absolute
    (exp results below 2^-126 may flush).  out = sum_f2 Ad v over F: (F + 3) u sum |Ad v|, Ad = A kf from the kernel's A.
    Backward: dAd = sum_t dO v: gamma_T; dA = kf dAd (+ u); rs = sum dA A: sum A e_dA + (F + 1) u sum |dA A|;
    dS = A (dA - rs): A (e_dA + e_rs + 2 u (|dA| + |rs|)); dq, dk, dv over F: + (F + 2) u of the sums of |terms|; the add into
    the time attention's dqkv rounds once more: u |ref| in f32, and the bf16 store r.
  * a2d_conv_wgrad: a thread's 48 accumulators run over its workgroup's units (upg = ceil(units / grid) of them), each
    ceil(TT / PS) frames of F pixels; then the PS frame subsets add up in LDS, the reduce kernel sums 32 groups in four chains of 8
    plus 2 adds, and the slices' atomics (ceil(grid / 32)) add to dW: depth d = upg ceil(6 / PS) F + PS + 12 + ceil(grid / 32):
    gamma_d sum |dY X| + u |ref|.
  * a2d_pack_w, a2d_planes: permutations plus a round-to-nearest cast (and one f32 add in pack_w mode 2): bit for bit.
  * whole block: forward stage by stage (z, qkv, cat, y, out from the engine's stored inputs) with the bounds above and the gathered
    GEMMs' gamma_K (K = 9 * channels + 1 with the bias); the MFMA time-attention route rounds P to the compute dtype before its
    PV product: + 2 r sum P |v|.  Gradients normwise against float64 autograd of oracle.s2t_ref.conv_attention_2d: f32 1e-3 of
    |g_ref| (the README's parity contract), bf16 0.3 of |g_ref|; for the convolutions' weights and biases, whose exact gradients
    cancel (bias ~0) behind training-mode BatchNorm, of the sums of |terms| when those are larger.  Both add 8 E1, E1 = gamma_T
    max sum_t |q k|: the frequency scores' own f32 error moves A by 2 E1 relative (above), and at T4 = 375 that, not the
    rounding of the rest, is what the bn_q gradients carry (1.4e-3 of |g_ref| in f32, measured).  The bf16 tolerance is wide:
    about 15 bf16 roundings lie on the path to a gradient (stored z, qkv, cat, y, the four packed weights, dy, dcat, dqkv twice,
    dz), and the training-mode BatchNorm backward subtracts two projections from dqkv and dout, so the relative error of dz, dy and
    the bn_q sums is several times that of their inputs (measured up to 0.26 of |g_ref|, bn_q.bias at T4 = 375).  The kernel
    cases above hold each piece to its element-wise bound; this case checks that the engine wires them together.
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
U = 2.0 ** -24
UBF = 2.0 ** -8
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
EINVAL, ENOTSUP = -22, -95
DSLACK = 2.0 ** -40
H = 4
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    K.prof_enable(0)
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
    bad = ~(err <= bound)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: out %.9g ref %.9g |err| %.3g bound %.3g (%.3gx)"
                             % (what, int(bad.sum()), bad.numel(), idx, float(o[idx]), float(ref[idx]), float(err[idx]),
                                float(bound[idx]), float(err[idx] / bound[idx]) if float(bound[idx]) > 0 else math.inf))


def out_bound(e, ref, dtype):
    """twice the derived arithmetic bound e, plus the output rounding"""
    return 2 * e + rout(dtype) * (ref.abs() + 2 * e)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(*shape, seed, scale=1.0, dtype=F32):
    return (torch.randn(*shape, generator=gen(seed), device=DEV) * scale).to(dtype)


def cdiv(a, b):
    return -(-a // b)


def rows(M, ld, dtype, offset=0, fill=0.0):
    """[M, ld] row view of a flat buffer that starts `offset` elements in (offset 1: not 16-byte aligned)"""
    flat = torch.full((M * ld + offset + 8,), fill, dtype=dtype, device=DEV)
    return flat[offset:offset + M * ld].view(M, ld)


@contextlib.contextmanager
def launches(families):
    counts = {}
    torch.cuda.synchronize()
    K.prof_reset()
    K.prof_enable(1)
    try:
        yield counts
    finally:
        torch.cuda.synchronize()
        for f in families:
            counts[f] = K.prof_read(f)["launches"]
        K.prof_enable(0)
        K.prof_reset()


def planes(t, B, T, Fq, ch0):
    """channels ch0 .. ch0+3 of [M, ld] rows (t, b, f) -> float64 [B*4, T, F], plane bh = 4 b + h"""
    ld = t.shape[1]
    return d64(t).view(T, B, Fq, ld)[..., ch0:ch0 + H].permute(1, 3, 0, 2).reshape(B * H, T, Fq)


def unplanes(p, B, T, Fq):
    """[B*4, T, F] -> [M, 4] rows (t, b, f)"""
    return p.view(B, H, T, Fq).permute(2, 0, 3, 1).reshape(T * B * Fq, H)


def make_qkv(B, T, Fq, dtype, seed, scale=0.8):
    """q, k, v in channels 0-11 as after the BN + ReLU (non-negative, many zeros), padding channels 12-15 zero"""
    qkv = torch.zeros(T * B * Fq, 16, device=DEV)
    qkv[:, :12] = torch.relu(randn(T * B * Fq, 12, seed=seed, scale=scale) + 0.2)
    return qkv.to(dtype)


def time_mask(B, T, p, seed):
    """keep[bh, i, j] of the time attention: dropout_keep(seed, (bh T + i) Tp + j), the hash of s2t_dropout's flat index"""
    if p == 0.0:
        return None
    Tp = (T + 3) & ~3
    m = K.dropout(torch.ones(B * H * T * Tp, device=DEV), p, seed) != 0
    return m.view(B * H, T, Tp)[:, :, :T].double()


def freq_mask(B, Fq, p, seed):
    if p == 0.0:
        return None
    return (K.dropout(torch.ones(B * H * Fq * Fq, device=DEV), p, seed) != 0).view(B * H, Fq, Fq).double()


# ------------------------------------------------------------------ references of the two attentions
def time_fwd_ref(qkv, lse_k, B, T, Fq, p, seed, mfma_dtype=None):
    """O (float64 [B*4,T,F]) from the stored q, k, v and the kernel's lse, with its bound; lse's own reference and bound"""
    q, k, v = planes(qkv, B, T, Fq, 0), planes(qkv, B, T, Fq, H), planes(qkv, B, T, Fq, 2 * H)
    S = q @ k.transpose(1, 2)
    eS = gam(Fq) * (q.abs() @ k.abs().transpose(1, 2))
    lse_ref = torch.logsumexp(S, -1)
    R = S.amax(-1) - S.amin(-1)
    e_lse = eS.amax(-1) + (3 * T + 2 * R + 28 + 3 * lse_ref.abs()) * U
    lk = d64(lse_k).view(B * H, T, 1)
    P = torch.exp(S - lk)
    keep = time_mask(B, T, p, seed)
    kf = torch.ones_like(P) if keep is None else keep / (1.0 - p)
    eps = eS + ((S - lk).abs() + 5) * U
    Pk = P * kf
    O = Pk @ v
    eO = (eps * Pk) @ v.abs() + (T + 1) * U * (Pk @ v.abs())
    if mfma_dtype is not None:
        eO = eO + 2 * rout(mfma_dtype) * (Pk @ v.abs())
    return O, eO, lse_ref, e_lse


def time_bwd_ref(qkv, cat, dcat, lse_k, B, T, Fq, p, seed):
    q, k, v = planes(qkv, B, T, Fq, 0), planes(qkv, B, T, Fq, H), planes(qkv, B, T, Fq, 2 * H)
    O, dO = planes(cat, B, T, Fq, 0), planes(dcat, B, T, Fq, 0)
    S = q @ k.transpose(1, 2)
    eS = gam(Fq) * (q.abs() @ k.abs().transpose(1, 2))
    lk = d64(lse_k).view(B * H, T, 1)
    P = torch.exp(S - lk)
    eps = eS + ((S - lk).abs() + 3) * U
    keep = time_mask(B, T, p, seed)
    kf = torch.ones_like(P) if keep is None else keep / (1.0 - p)
    if keep is not None:
        eps = eps + 2 * U
    delta = (dO * O).sum(-1, keepdim=True)
    e_delta = gam(Fq) * (dO.abs() * O.abs()).sum(-1, keepdim=True)
    dP = dO @ v.transpose(1, 2)
    e_dP = gam(Fq) * (dO.abs() @ v.abs().transpose(1, 2))
    dPk = dP * kf
    dS = P * (dPk - delta)
    e_dS = P * (eps * (dPk - delta).abs() + kf * (e_dP + 2 * U * dP.abs()) + e_delta + 2 * U * (dPk.abs() + delta.abs()))
    aS = dS.abs()
    Pk = P * kf
    dq = dS @ k
    e_dq = e_dS @ k.abs() + (T + 1) * U * (aS @ k.abs())
    dk = dS.transpose(1, 2) @ q
    e_dk = e_dS.transpose(1, 2) @ q.abs() + (T + 1) * U * (aS.transpose(1, 2) @ q.abs())
    dv = Pk.transpose(1, 2) @ dO
    e_dv = ((eps + 2 * U) * Pk).transpose(1, 2) @ dO.abs() + (T + 1) * U * (Pk.transpose(1, 2) @ dO.abs())
    return delta.squeeze(-1), e_delta.squeeze(-1), (dq, e_dq), (dk, e_dk), (dv, e_dv)


def freq_fwd_ref(qkv, A_k, B, T, Fq, p, seed):
    q, k, v = planes(qkv, B, T, Fq, 0), planes(qkv, B, T, Fq, H), planes(qkv, B, T, Fq, 2 * H)
    S = q.transpose(1, 2) @ k
    eS = gam(T) * (q.abs().transpose(1, 2) @ k.abs())
    A_ref = torch.softmax(S, -1)
    m = S.amax(-1, keepdim=True)
    E1 = eS.amax(-1, keepdim=True)
    lw = (A_ref * (S - m).abs()).sum(-1, keepdim=True)
    eA = (2 * E1 + ((S - m).abs() + lw + Fq + 6) * U) * A_ref + 1e-37
    keep = freq_mask(B, Fq, p, seed)
    Ad = d64(A_k) * (1.0 if keep is None else keep / (1.0 - p))
    out = v @ Ad.transpose(1, 2)
    e_out = (Fq + 3) * U * (v.abs() @ Ad.abs().transpose(1, 2))
    return A_ref, eA, out, e_out


def freq_bwd_ref(qkv, dcat, A_k, B, T, Fq, p, seed):
    q, k, v = planes(qkv, B, T, Fq, 0), planes(qkv, B, T, Fq, H), planes(qkv, B, T, Fq, 2 * H)
    dO = planes(dcat, B, T, Fq, H)
    A = d64(A_k)
    keep = freq_mask(B, Fq, p, seed)
    kf = torch.ones_like(A) if keep is None else keep / (1.0 - p)
    Ad = A * kf
    dAd = dO.transpose(1, 2) @ v
    e_dAd = gam(T) * (dO.abs().transpose(1, 2) @ v.abs())
    dA = dAd * kf
    e_dA = kf * (e_dAd + U * dAd.abs()) + U * dA.abs()
    rs = (dA * A).sum(-1, keepdim=True)
    e_rs = (A * e_dA).sum(-1, keepdim=True) + (Fq + 1) * U * (dA * A).abs().sum(-1, keepdim=True)
    dS = A * (dA - rs)
    e_dS = A * (e_dA + e_rs + 2 * U * (dA.abs() + rs.abs()))
    dq = k @ dS.transpose(1, 2)
    e_dq = k.abs() @ e_dS.transpose(1, 2) + (Fq + 2) * U * (k.abs() @ dS.abs().transpose(1, 2))
    dk = q @ dS
    e_dk = q.abs() @ e_dS + (Fq + 2) * U * (q.abs() @ dS.abs())
    dv = dO @ Ad
    e_dv = (Fq + 2) * U * (dO.abs() @ Ad.abs())
    return (dq, e_dq), (dk, e_dk), (dv, e_dv)


# ------------------------------------------------------------------ 5. VALU time attention
TIME_T = [1, 3, 63, 64, 65, 127, 128, 129, 375]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Fq", [10, 20, 21])
@pytest.mark.parametrize("T", TIME_T)
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_time_attention_against_fp64(dtype, Fq, T, p):
    """O, lse, delta, dq, dk, dv of the one-thread-per-frame kernels: key tiles of KT = 64 (full, ragged, single), query grids of
    128 (one, several), and with dropout the exact keep mask of the padded index (bh T + i) Tp + j, Tp = (T + 3) & ~3"""
    time_attention_case(dtype, Fq, T, p, 1000 + T)


HIGH_SEED = (5 << 32) | 7          # a dropout seed whose upper word is set


@pytest.mark.parametrize("dtype", DTYPES)
def test_time_and_frequency_attention_dropout_seed_above_32_bits(dtype):
    """both attentions, forward and backward, at F = 10 with the upper word of the seed set: T = 65 for the time kernels (two key tiles,
    the second with one key; T = 1 and 3 have too few pairs to tell masks apart) and T = 1 for the frequency kernels"""
    time_attention_case(dtype, 10, 65, 0.3, 1000 + 65, HIGH_SEED)
    frequency_attention_case(dtype, 10, 1, 0.3, 2000 + 1, HIGH_SEED)
    assert not torch.equal(time_mask(2, 65, 0.3, HIGH_SEED), time_mask(2, 65, 0.3, HIGH_SEED & 0xFFFFFFFF))
    assert not torch.equal(freq_mask(2, 10, 0.3, HIGH_SEED), freq_mask(2, 10, 0.3, HIGH_SEED & 0xFFFFFFFF))


def time_attention_case(dtype, Fq, T, p, data_seed, drop_seed=None):
    B, seed = 2, data_seed
    M = T * B * Fq
    qkv = make_qkv(B, T, Fq, dtype, seed=T * 7 + Fq)
    cat = rows(M, 8, dtype, fill=float("nan"))
    drop_seed = seed if drop_seed is None else drop_seed
    with launches(["attn2d"]) as n:
        lse = K.a2d_time_fwd(qkv, cat, B, T, Fq, p, drop_seed)
    assert n["attn2d"] == 1
    what = "time F=%d T=%d %s p=%g" % (Fq, T, dtype, p)
    O, eO, lse_ref, e_lse = time_fwd_ref(qkv, lse, B, T, Fq, p, drop_seed)
    assert_close(lse, lse_ref, 2 * e_lse, what + " lse", "time_lse")
    assert_close(planes(cat, B, T, Fq, 0), O, out_bound(eO, O, dtype), what + " O", "time_fwd")
    assert torch.isnan(cat[:, H:].float()).all()                # the frequency half is not the time kernel's
    dcat = randn(M, 8, seed=seed + 1, dtype=dtype)
    dqkv = torch.zeros(M, 16, dtype=dtype, device=DEV)
    with launches(["attn2d"]) as n:
        delta = K.a2d_time_bwd(qkv, cat, dcat, lse, dqkv, B, T, Fq, p, drop_seed)
    assert n["attn2d"] == 1
    d_ref, e_d, dq, dk, dv = time_bwd_ref(qkv, cat, dcat, lse, B, T, Fq, p, drop_seed)
    assert_close(delta, d_ref, 2 * e_d + 1e-300, what + " delta", "time_delta")
    for (ref, e), ch, nm in ((dq, 0, "dq"), (dk, H, "dk"), (dv, 2 * H, "dv")):
        assert_close(planes(dqkv, B, T, Fq, ch), ref, out_bound(e, ref, dtype), what + " " + nm, "time_" + nm)
    assert float(dqkv[:, 12:].float().abs().max()) == 0.0


# ------------------------------------------------------------------ 6. frequency attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Fq", [10, 20, 21])
@pytest.mark.parametrize("T", [1, 64, 375, 1000])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_frequency_attention_against_fp64(dtype, Fq, T, p):
    """A and the output; dq, dk, dv ADDED to a non-zero dqkv (what the time backward wrote), mask index (bh F + f1) F + f2"""
    frequency_attention_case(dtype, Fq, T, p, 2000 + T)


def frequency_attention_case(dtype, Fq, T, p, data_seed, drop_seed=None):
    B, seed = 2, data_seed
    M = T * B * Fq
    qkv = make_qkv(B, T, Fq, dtype, seed=T * 5 + Fq, scale=0.5)
    cat = rows(M, 8, dtype, fill=float("nan"))
    drop_seed = seed if drop_seed is None else drop_seed
    A = K.a2d_freq_fwd(qkv, cat, B, T, Fq, p, drop_seed)
    what = "freq F=%d T=%d %s p=%g" % (Fq, T, dtype, p)
    A_ref, eA, out, e_out = freq_fwd_ref(qkv, A, B, T, Fq, p, drop_seed)
    assert_close(A, A_ref, 2 * eA, what + " A", "freq_A")
    assert_close(planes(cat, B, T, Fq, H), out, out_bound(e_out, out, dtype), what + " out", "freq_fwd")
    assert torch.isnan(cat[:, :H].float()).all()
    dcat = randn(M, 8, seed=seed + 1, dtype=dtype)
    d0 = randn(M, 16, seed=seed + 2, dtype=dtype)
    dqkv = d0.clone()
    K.a2d_freq_bwd(qkv, dcat, A, dqkv, B, T, Fq, p, drop_seed)
    dq, dk, dv = freq_bwd_ref(qkv, dcat, A, B, T, Fq, p, drop_seed)
    for (d, e), ch, nm in ((dq, 0, "dq"), (dk, H, "dk"), (dv, 2 * H, "dv")):
        ref = planes(d0, B, T, Fq, ch) + d
        e = e + U * ref.abs()
        assert_close(planes(dqkv, B, T, Fq, ch), ref, out_bound(e, ref, dtype), what + " " + nm, "freq_" + nm)
    assert torch.equal(dqkv[:, 12:], d0[:, 12:])


# ------------------------------------------------------------------ 1. grouped BatchNorm statistics
def sums_index(C, Cg):
    c = torch.arange(C)
    i0 = (c // Cg) * 2 * Cg + c % Cg
    return i0.to(DEV), (i0 + Cg).to(DEV)


def bn_consts(C, seed, dead=None):
    """f32 mean, rstd, scale, shift (one channel's shift so negative that the ReLU kills it)"""
    mean = 0.3 * randn(C, seed=seed)
    rstd = 1.0 / (0.5 + torch.rand(C, generator=gen(seed + 1), device=DEV))
    gamma = 1.0 + 0.2 * randn(C, seed=seed + 2)
    beta = 0.2 * randn(C, seed=seed + 3)
    scale = gamma * rstd
    shift = beta - mean * scale
    if dead is not None:
        shift[dead] = -1e3
    return mean, rstd, scale, shift


def safe_dy(z, dy, C, ps, scale, shift):
    """zero dy where the f32 ReLU decision of x sc + sf could differ from float64 (see the module docstring)"""
    x = d64(z[:, :C]) * ps[:C].double()
    pre = x * scale.double() + shift.double()
    amb = pre.abs() <= 8 * U * ((x * scale.double()).abs() + shift.double().abs())
    dy[:, :C][amb] = 0
    return dy


FORMS = ["vec", "scalar"]
# (C, Cg, ld): the qkv BatchNorms (three groups of 4 in rows of 16) and bn_out (one group of 64)
GROUPS = [(12, 4, 16), (64, 64, 64)]


def bn_rows(M, C, ld, form, dtype, seed, scale=1.5):
    """[M, ld] rows in the form's layout: vec = ld in {8,16,32,64}, 16-byte aligned; scalar = the same ld from a pointer 1 element
    in (C = 64) or rows of ld + 4 (C < 64): both fail a2d_vec_ok (attn2d.hip:702)"""
    if form == "vec":
        t = rows(M, ld, dtype)
    elif C == 64:
        t = rows(M, ld, dtype, offset=1)
    else:
        t = rows(M, ld + 4, dtype)
    t[:, :C] = (randn(M, C, seed=seed, scale=scale) + 0.3).to(dtype)
    t[:, C:] = float("nan")                                # padding channels must not be read
    return t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [200, 5000, 300001])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,Cg,ld", GROUPS)
def test_chan_stats_against_fp64(C, Cg, ld, form, M, dtype):
    """mode 0 without and with prescale, mode 1 (sums behind the ReLU mask, one channel killed); M < 256, a few blocks, and
    rpb = ceil(M / 1024) > 256 with a ragged last block"""
    z = bn_rows(M, C, ld, form, dtype, seed=M + C)
    dy = bn_rows(M, C, ld, form, dtype, seed=M + C + 1, scale=1.0)
    ps = torch.ones(64, device=DEV)
    ps[:min(4, C)] = 0.125
    i0, i1 = sums_index(C, Cg)
    what = "chan_stats C=%d %s M=%d %s" % (C, form, M, dtype)
    for pre in (None, ps):
        s = K.a2d_chan_stats(z, C, Cg, prescale=pre)
        x = d64(z[:, :C]) * (1.0 if pre is None else pre[:C].double())
        r0, r1 = x.sum(0), (x * x).sum(0)
        e0 = (66 * U + DSLACK) * x.abs().sum(0)
        e1 = (68 * U + DSLACK) * (x * x).sum(0)
        assert_close(s[i0], r0, 2 * e0, what + " mode 0 s0 ps=%s" % (pre is not None), "chan_stats")
        assert_close(s[i1], r1, 2 * e1, what + " mode 0 s1 ps=%s" % (pre is not None), "chan_stats")
    mean, rstd, scale, shift = bn_consts(C, seed=M + 7, dead=C - 1)
    dy = safe_dy(z, dy, C, ps, scale, shift)
    s = K.a2d_chan_stats(z, C, Cg, prescale=ps, dy=dy, bn=(mean, rstd, scale, shift))
    x = d64(z[:, :C]) * ps[:C].double()
    g = torch.where(x * scale.double() + shift.double() > 0, d64(dy[:, :C]), torch.zeros_like(x))
    xh = (x - mean.double()) * rstd.double()
    r0, r1 = g.sum(0), (g * xh).sum(0)
    e0 = (64 * U + DSLACK) * g.abs().sum(0)
    e1 = (69 * U + DSLACK) * (g.abs() * rstd.double() * ((x - mean.double()).abs() + x.abs())).sum(0)
    assert_close(s[i0], r0, 2 * e0, what + " mode 1 s0", "chan_stats")
    assert_close(s[i1], r1, 2 * e1, what + " mode 1 s1", "chan_stats")
    assert float(s[i0][C - 1]) == 0.0 and float(s[i1][C - 1]) == 0.0


# ------------------------------------------------------------------ 2. BN + ReLU (+ residual)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [200, 300001])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,ld", [(12, 16), (5, 8), (64, 64)])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_act_against_fp64(C, ld, form, M, dtype, with_res):
    """y = relu(ps z sc + sf) [+ res] with prescale; M ld / 8 and M ld past the 4096-block grid cap (grid-stride loops).
    Padding channels C..ld-1 of y: both forms write whole rows, res there (zero without res)"""
    off = 1 if form == "scalar" else 0                      # a pointer 1 element in fails a2d_vec_ok: the scalar form
    z = rows(M, ld, dtype, offset=off)
    z[:, :C] = randn(M, C, seed=M + C, scale=1.5, dtype=dtype)
    z[:, C:] = float("nan")
    res = None
    if with_res:
        res = rows(M, ld, dtype, offset=off)
        res.copy_(randn(M, ld, seed=M + C + 1, dtype=dtype))
    y = rows(M, ld, dtype, offset=off, fill=7.0)
    ps = torch.ones(64, device=DEV)
    ps[:min(4, C)] = 0.125
    _, _, scale, shift = bn_consts(C, seed=C + 11)
    K.a2d_bn_act(z, C, scale, shift, prescale=ps, res=res, out=y)
    x = d64(z[:, :C]) * ps[:C].double()
    a = x * scale.double()
    ref = torch.relu(a + shift.double())
    e = 3 * U * (a.abs() + shift.double().abs())
    if res is not None:
        e = e + U * (ref.abs() + d64(res[:, :C]).abs())
        ref = ref + d64(res[:, :C])
    what = "bn_act C=%d ld=%d %s M=%d %s res=%s" % (C, ld, form, M, dtype, with_res)
    assert_close(y[:, :C], ref, out_bound(e, ref, dtype), what, "bn_act")
    pad = res[:, C:] if res is not None else torch.zeros_like(y[:, C:])
    assert torch.equal(y[:, C:], pad), what + ": padding channels"


def test_bn_act_refusals():
    z = torch.zeros(16, 16, device=DEV)
    s = torch.ones(16, device=DEV)
    lib = K._lib()
    assert lib.s2t_a2d_bn_act(L.dt(z), L.ptr(z), 0, L.ptr(s), L.ptr(s), 0, L.ptr(z), 16, 17, 16, 16, L.stream()) == EINVAL
    assert lib.s2t_a2d_bn_act(L.dt(z), L.ptr(z), 0, L.ptr(s), L.ptr(s), 0, L.ptr(z), 16, 12, 16, 8, L.stream()) == EINVAL


# ------------------------------------------------------------------ 3. BN backward and parameter gradients
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [200, 300001])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,Cg,ld", GROUPS)
@pytest.mark.parametrize("training", [1, 0])
def test_bn_bwd_against_fp64(C, Cg, ld, form, M, dtype, training):
    """dz = ps sc (dyn - m0 - xhat m1) (training) or ps sc dyn (eval) from the given double sums, one channel killed by the
    ReLU; then dgamma / dbeta accumulated into non-zero buffers per group"""
    z = bn_rows(M, C, ld, form, dtype, seed=M + 3 * C)
    dy = bn_rows(M, C, ld, form, dtype, seed=M + 3 * C + 1, scale=1.0)
    ps = torch.ones(64, device=DEV)
    ps[:min(4, C)] = 0.125
    mean, rstd, scale, shift = bn_consts(C, seed=M + 5, dead=1)
    dy = safe_dy(z, dy, C, ps, scale, shift)
    bn = (mean, rstd, scale, shift)
    sums = K.a2d_chan_stats(z, C, Cg, prescale=ps, dy=dy, bn=bn)
    dz = K.a2d_bn_bwd(dy, z, C, Cg, bn, sums, M, training, prescale=ps)
    i0, i1 = sums_index(C, Cg)
    m0, m1 = sums[i0] / M, sums[i1] / M
    x = d64(z[:, :C]) * ps[:C].double()
    g = torch.where(x * scale.double() + shift.double() > 0, d64(dy[:, :C]), torch.zeros_like(x))
    mu, rs, sc, psd = mean.double(), rstd.double(), scale.double(), ps[:C].double()
    if training:
        o = g - m0 - (x - mu) * rs * m1
        e_o = 4 * U * (g.abs() + m0.abs() + rs * m1.abs() * ((x - mu).abs() + x.abs()))
    else:
        o = g
        e_o = torch.zeros_like(g)
    ref = o * sc * psd
    e = (sc * psd).abs() * e_o + 2 * U * ref.abs()
    what = "bn_bwd C=%d %s M=%d %s training=%d" % (C, form, M, dtype, training)
    assert_close(dz[:, :C], ref, out_bound(e, ref, dtype), what, "bn_bwd")
    assert bool((dz[:, 1] == 0).all()) and bool((dz[:, C:] == 0).all())
    for gi in range(C // Cg):
        dg0, db0 = randn(Cg, seed=gi + 40), randn(Cg, seed=gi + 50)
        dg, db = dg0.clone(), db0.clone()
        K.a2d_param_grads(sums[2 * Cg * gi:2 * Cg * (gi + 1)], dg, db)
        for got, init, s, nm in ((dg, dg0, sums[2 * Cg * gi + Cg:2 * Cg * (gi + 1)], "dgamma"), (db, db0, sums[2 * Cg * gi:2 * Cg * gi + Cg], "dbeta")):
            ref = init.double() + s
            assert_close(got, ref, 2 * U * (s.abs() + ref.abs()), what + " %s group %d" % (nm, gi), "param_grads")


# ------------------------------------------------------------------ 4. weight packing
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Co,Ci,CP,pad_ld", [(12, 64, 64, 0), (64, 8, 8, 0), (12, 60, 64, 8), (64, 8, 12, 5)])
def test_pack_w_bit_exact(Co, Ci, CP, pad_ld, dtype):
    """mode 0 dst[co][j CP + ci] = W[co][ci][j], mode 1 dst[ci][(8 - j) CP + co] = W[co][ci][j], mode 2 W[co][ci][j] +=
    src[co][j CP + ci]; pad rows / columns (CP > Ci, ld > 9 CP) stay zero, mode 2 ignores them"""
    lib = K._lib()
    w = randn(Co, Ci, 3, 3, seed=Co + Ci)
    wj = w.view(Co, Ci, 9)
    for mode, nrows, cp, inner in ((0, Co + 4, max(CP, Ci), Ci), (1, Ci + 4, max(CP, Co), Co)):
        ld = 9 * cp + pad_ld
        dst = torch.zeros(nrows, ld, dtype=dtype, device=DEV)
        assert lib.s2t_a2d_pack_w(L.dt(dst), L.ptr(w), L.ptr(dst), 0, Co, Ci, cp, ld, mode, L.stream()) == 0
        exp = torch.zeros(nrows, ld, dtype=dtype, device=DEV)
        for j in range(9):
            if mode == 0:
                exp[:Co, j * cp:j * cp + Ci] = wj[:, :, j].to(dtype)
            else:
                exp[:Ci, (8 - j) * cp:(8 - j) * cp + Co] = wj[:, :, j].t().to(dtype)
        assert torch.equal(dst, exp), "pack_w mode %d Co=%d Ci=%d CP=%d ld=%d %s" % (mode, Co, Ci, cp, ld, dtype)
    ld = 9 * CP + pad_ld
    src = randn(Co, ld, seed=77)
    g0 = randn(Co, Ci, 3, 3, seed=78)
    g = g0.clone()
    assert lib.s2t_a2d_pack_w(L.F32, L.ptr(src), 0, L.ptr(g), Co, Ci, CP, ld, 2, L.stream()) == 0
    exp = g0 + torch.stack([src[:, j * CP:j * CP + Ci] for j in range(9)], -1).view(Co, Ci, 3, 3)
    assert torch.equal(g, exp), "pack_w mode 2 Co=%d Ci=%d CP=%d ld=%d" % (Co, Ci, CP, ld)
    assert lib.s2t_a2d_pack_w(L.F32, L.ptr(src), L.ptr(g), 0, Co, Ci, Ci - 1, ld, 0, L.stream()) == EINVAL
    assert lib.s2t_a2d_pack_w(L.F32, L.ptr(src), L.ptr(g), 0, Co, Ci, CP, 9 * CP - 1, 0, L.stream()) == EINVAL


# ------------------------------------------------------------------ 7. one-pass convolution weight gradient
WG_SHAPES = {"in_proj": (12, 16, 64, 64), "out_proj": (64, 64, 8, 8)}          # (CO real, ld_dy, CI, ld_x)


def wgrad_case(shape, dtype, B, T, Fq, seed):
    CO, ldy, CI, ldx = WG_SHAPES[shape]
    M = T * B * Fq
    x = randn(M, ldx, seed=seed, dtype=dtype)
    dy = torch.full((M, ldy), float("nan"), dtype=dtype, device=DEV)        # padding channels 12..15 of in_proj: garbage
    dy[:, :CO] = randn(M, CO, seed=seed + 1, dtype=dtype)
    g0 = randn(CO, CI, 3, 3, seed=seed + 2)
    return CO, CI, x, dy, g0


def wgrad_ref(x, dy, CO, CI, B, T, Fq, g0):
    X = d64(x[:, :CI]).view(T, B, Fq, CI).permute(1, 3, 0, 2)
    D = d64(dy[:, :CO]).view(T, B, Fq, CO).permute(1, 3, 0, 2)
    ref = torch.nn.grad.conv2d_weight(X, (CO, CI, 3, 3), D, padding=1)
    mag = torch.nn.grad.conv2d_weight(X.abs(), (CO, CI, 3, 3), D.abs(), padding=1)
    return g0.double() + ref, mag


WG_CASES = [(2, 13, f) for f in (1, 5, 9, 10, 13, 14, 20, 21)] + [(3, 4, 20), (2, 6, 10), (16, 375, 20)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", list(WG_SHAPES))
@pytest.mark.parametrize("B,T,Fq", WG_CASES)
def test_conv_wgrad_against_fp64(shape, dtype, B, T, Fq):
    """dW += sum dY X over the nine taps, accumulated into a non-zero dW: T not a multiple of TT = 6, T < 6, F from 1 (the
    reduction area larger than the staging area) to 21, and B ceil(T / 6) = 1008 units on the 512-workgroup cap"""
    CO, CI, x, dy, g0 = wgrad_case(shape, dtype, B, T, Fq, seed=B * T + Fq)
    g = g0.clone()
    assert K.a2d_conv_wgrad(dy, x, g, B, T, Fq)
    ref, mag = wgrad_ref(x, dy, CO, CI, B, T, Fq, g0)
    units = B * cdiv(T, 6)
    grid = min(units, 512)
    PS = max(1, 256 // ((CI // 4) * (max(CO, 16) // 4) * 3))
    depth = cdiv(units, grid) * cdiv(6, PS) * Fq + PS + 12 + cdiv(grid, 32)
    e = gam(depth) * mag + U * ref.abs()
    assert_close(g, ref, 2 * e, "conv_wgrad %s %s B=%d T=%d F=%d" % (shape, dtype, B, T, Fq), "conv_wgrad")


def test_conv_wgrad_refusals():
    """odd row strides, pointers off 16 bytes and shapes not built are refused (ENOTSUP: the caller falls back) and dW is untouched"""
    B, T, Fq = 2, 7, 20
    M = T * B * Fq
    g = torch.ones(12, 64, 3, 3, device=DEV)
    x = randn(M, 64, seed=1)
    assert not K.a2d_conv_wgrad(torch.zeros(M, 18, device=DEV)[:, :16], x, g, B, T, Fq)               # f32 ld 18
    xb = randn(M, 68, seed=2, dtype=BF)
    assert not K.a2d_conv_wgrad(torch.zeros(M, 16, dtype=BF, device=DEV), xb[:, :64], g, B, T, Fq)   # bf16 ld 68
    xm = rows(M, 64, F32, offset=1)
    assert not K.a2d_conv_wgrad(torch.zeros(M, 16, device=DEV), xm, g, B, T, Fq)                        # X off 16 bytes
    g2 = torch.ones(32, 8, 3, 3, device=DEV)
    assert not K.a2d_conv_wgrad(torch.zeros(M, 32, device=DEV), randn(M, 8, seed=3), g2, B, T, Fq)      # (32, 8) not built
    g3 = torch.ones(64, 16, 3, 3, device=DEV)
    assert not K.a2d_conv_wgrad(torch.zeros(M, 64, device=DEV), randn(M, 16, seed=4), g3, B, T, Fq)     # (64, 16) not built
    assert bool((g == 1).all()) and bool((g2 == 1).all()) and bool((g3 == 1).all())


# ------------------------------------------------------------------ 8. planes of the MFMA time-attention route
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G,ch0,ld", [(1, 0, 16), (3, 0, 16), (1, 4, 8), (2, 4, 16)])
@pytest.mark.parametrize("Fq", [21, 32])
def test_planes_bit_exact(G, ch0, ld, Fq, dtype):
    """dir 0: pl[g][t][b][32 h + f] = chl[(t B + b) F + f][ch0 + 4 g + h], zero for f >= F; dir 1 writes back only f < F and
    channels ch0 + 4 g + h: sentinels elsewhere survive"""
    B, T = 3, 5
    M = T * B * Fq
    chl = randn(M, ld, seed=G * 10 + ch0, dtype=dtype)
    pl = torch.full((G, T, B, 128), 9.0, dtype=dtype, device=DEV)
    K.a2d_planes(chl, pl, ch0, B, T, Fq, True)
    src = chl.view(T, B, Fq, ld)[..., ch0:ch0 + 4 * G].reshape(T, B, Fq, G, H).permute(3, 0, 1, 4, 2)     # [G,T,B,H,F]
    exp = torch.zeros(G, T, B, H, 32, dtype=dtype, device=DEV)
    exp[..., :Fq] = src
    assert torch.equal(pl, exp.reshape(G, T, B, 128)), "planes dir 0 G=%d ch0=%d F=%d" % (G, ch0, Fq)
    pl2 = randn(G, T, B, 128, seed=5, dtype=dtype)
    out = torch.full((M, ld), 3.0, dtype=dtype, device=DEV)
    K.a2d_planes(out, pl2, ch0, B, T, Fq, False)
    exp = torch.full((M, ld), 3.0, dtype=dtype, device=DEV)
    back = pl2.view(G, T, B, H, 32)[..., :Fq].permute(1, 2, 4, 0, 3).reshape(M, 4 * G)
    exp[:, ch0:ch0 + 4 * G] = back
    assert torch.equal(out, exp), "planes dir 1 G=%d ch0=%d F=%d" % (G, ch0, Fq)


def test_planes_refusals():
    lib = K._lib()
    chl = torch.zeros(4 * 33 * 16, 16, device=DEV)
    pl = torch.zeros(1, 4, 1, 128, device=DEV)
    assert lib.s2t_a2d_planes(L.F32, L.ptr(chl), L.ptr(pl), 1, 0, 16, 1, 4, 33, 0, L.stream()) == EINVAL      # F > 32
    assert lib.s2t_a2d_planes(L.F32, L.ptr(chl), L.ptr(pl), 1, 13, 16, 1, 4, 20, 0, L.stream()) == EINVAL     # ch0 + 4G > ld
    assert lib.s2t_a2d_planes(L.F32, L.ptr(chl), L.ptr(pl), 3, 8, 16, 1, 4, 20, 1, L.stream()) == EINVAL
    assert lib.s2t_a2d_planes(L.F32, L.ptr(chl), L.ptr(pl), 1, 0, 16, 1, 4, 20, 2, L.stream()) == EINVAL      # no direction 2


# ------------------------------------------------------------------ 9. one block through the engine
_MODELS = {}


def attn2d_model(dtype):
    if dtype not in _MODELS:
        from fbk_fairseq_st_amd import conv_transformer, criterions, tasks  # noqa: F401
        from fbk_fairseq_st_amd.data import Dictionary
        from fbk_fairseq_st_amd.registry import apply_arch, namespace
        a = namespace(arch="conv_transformer", criterion="ctc_multi_loss", underlying_criterion="label_smoothed_cross_entropy",
                      label_smoothing=0.1, ctc_compress_out=True, ctc_encoder_layer=1, ctc_weight=1.0, encoder_embed_dim=128,
                      encoder_ffn_embed_dim=256, encoder_attention_heads=2, encoder_layers=1, decoder_layers=1, decoder_embed_dim=128,
                      decoder_ffn_embed_dim=256, decoder_attention_heads=2, no_attn_2d=False, input_feat_per_channel=80, dropout=0.0,
                      attention_dropout=0.0, activation_dropout=0.0, relu_dropout=0.0, sentence_avg=False, seed=7)
        apply_arch(a)
        tgt, src = Dictionary.synthetic(100), Dictionary.synthetic(50)
        src.add_symbol("<ctc_blank>")
        task = tasks.SpeechTranslationCTCTask(a, tgt, src)
        torch.manual_seed(3)
        model, crit = task.build_model(a), task.build_criterion(a)
        model.materialize(DEV, dtype, extra=crit.arena_params())
        assert model.hp.attn_2d and model.hp.conv_ch == 64
        _MODELS[dtype] = model
    return _MODELS[dtype]


BLOCK = ["in_proj_weight", "in_proj_bias", "bn_q.weight", "bn_q.bias", "bn_k.weight", "bn_k.bias", "bn_v.weight", "bn_v.bias",
         "out_proj.weight", "out_proj.bias", "bn_out.weight", "bn_out.bias"]


def img(t, B, T, Fq, C):
    """[M, ld] rows (t, b, f) -> float64 [B, C, T, F] of the first C channels"""
    return d64(t)[:, :C].reshape(T, B, Fq, C).permute(1, 3, 0, 2)


def unimg(x):
    B, C, T, Fq = x.shape
    return x.permute(2, 0, 3, 1).reshape(T * B * Fq, C)


def conv_stage(x, w, b, B, T, Fq, Ci):
    ref = unimg(Fn.conv2d(img(x, B, T, Fq, Ci), w, b, padding=1))
    mag = unimg(Fn.conv2d(img(x, B, T, Fq, Ci).abs(), w.abs(), b.abs(), padding=1))
    return ref, gam(9 * Ci + 1) * mag


def bn_act_stage(z, C, bn, ps, res=None):
    x = d64(z[:, :C]) * (1.0 if ps is None else ps[:C].double())
    a = x * bn[2].double()
    ref = torch.relu(a + bn[3].double())
    e = 3 * U * (a.abs() + bn[3].double().abs())
    if res is not None:
        e = e + U * (ref.abs() + d64(res[:, :C]).abs())
        ref = ref + d64(res[:, :C])
    return ref, e


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,T4,F4", [(2, 23, 10), (2, 31, 20), (1, 17, 21), (1, 375, 20)])
def test_block_against_fp64(B, T4, F4, training, mfma, dtype):
    """Engine.attn2d_block_fwd stage by stage from its stored inputs (z, qkv, cat, y, out), then attn2d_block_bwd's dx and every
    parameter gradient against float64 autograd of oracle.s2t_ref.conv_attention_2d, on the time-attention route `mfma`
    (planes + attn_fwd / attn_bwd) or the VALU kernels (launch family "attn2d")"""
    from oracle import s2t_ref
    model = attn2d_model(dtype)
    eng, A = model.engine, model.arena
    C, M, p = 64, T4 * B * F4, "encoder.attn_2d.0."
    x = randn(M, C, seed=T4 + F4, dtype=dtype)
    bufs0 = {k: v.clone() for k, v in eng.bn_buffers.items()}
    A.zero_grad()
    old = eng.a2d_time_mfma
    eng.a2d_time_mfma = mfma
    try:
        with launches(["attn2d", "attn_fwd", "attn_bwd"]) as n:
            out, c = eng.attn2d_block_fwd(0, x, B, T4, F4, training, 5)
            dout = randn(M, C, seed=T4 + F4 + 1, dtype=dtype)
            dx = eng.attn2d_block_bwd(c, dout)
            if hasattr(eng, "flush_wgrad"):
                eng.flush_wgrad()
    finally:
        eng.a2d_time_mfma = old
        for k, v in bufs0.items():
            eng.bn_buffers[k].copy_(v)
    if mfma:
        assert n["attn_fwd"] == 1 and n["attn_bwd"] == 1 and n["attn2d"] == 0, n
    else:
        assert n["attn2d"] == 2 and n["attn_fwd"] == 0 and n["attn_bwd"] == 0, n
    what = "block B=%d T4=%d F4=%d training=%s mfma=%s %s" % (B, T4, F4, training, mfma, dtype)
    Pm = lambda nm: A.p(p + nm).detach()
    # z = conv(x, in_proj) with the weights rounded to the compute dtype; padding channels 12..15 exactly zero
    ref, e = conv_stage(x, Pm("in_proj_weight").to(dtype).double(), Pm("in_proj_bias").double(), B, T4, F4, C)
    assert_close(c["z"][:, :12], ref, out_bound(e, ref, dtype), what + " z", "block_z")
    assert float(c["z"][:, 12:].float().abs().max()) == 0.0
    ps = eng._a2d_prescale
    ref, e = bn_act_stage(c["z"], 12, c["bn_qkv"], ps)
    assert_close(c["qkv"][:, :12], ref, out_bound(e, ref, dtype), what + " qkv", "block_qkv")
    if training:                                            # the grouped statistics behind bn_qkv: mean of ps z
        xz = d64(c["z"][:, :12]) * ps[:12].double()
        e_m = (66 * U + DSLACK) * xz.abs().mean(0) + 2 * U * xz.mean(0).abs()
        assert_close(c["bn_qkv"][0], xz.mean(0), 2 * e_m, what + " bn_qkv mean", "block_bn_mean")
    O, eO, _, _ = time_fwd_ref(c["qkv"], c["lse"], B, T4, F4, 0.0, 0, mfma_dtype=dtype if mfma else None)
    assert_close(planes(c["cat"], B, T4, F4, 0), O, out_bound(eO, O, dtype), what + " cat (time)", "block_cat_time")
    _, _, Of, eOf = freq_fwd_ref(c["qkv"], c["A"], B, T4, F4, 0.0, 0)
    assert_close(planes(c["cat"], B, T4, F4, H), Of, out_bound(eOf, Of, dtype), what + " cat (freq)", "block_cat_freq")
    ref, e = conv_stage(c["cat"], Pm("out_proj.weight").to(dtype).double(), Pm("out_proj.bias").double(), B, T4, F4, 8)
    assert_close(c["y"], ref, out_bound(e, ref, dtype), what + " y", "block_y")
    ref, e = bn_act_stage(c["y"], C, c["bn_o"], None, res=x)
    assert_close(out, ref, out_bound(e, ref, dtype), what + " out", "block_out")
    # backward against float64 autograd, weights as the engine used them (conv weights rounded to the compute dtype)
    W = {}
    for nm in BLOCK:
        t = A.p(p + nm).detach()
        if nm in ("in_proj_weight", "out_proj.weight"):
            t = t.to(dtype)
        W[p + nm] = t.double().cpu().requires_grad_(True)
    for bn_name in ("bn_q.", "bn_k.", "bn_v.", "bn_out."):
        W[p + bn_name + "running_mean"] = bufs0[p + bn_name + "running_mean"].double().cpu()
        W[p + bn_name + "running_var"] = bufs0[p + bn_name + "running_var"].double().cpu()
    cfg = dict(bn_momentum=model.hp.bn_momentum, bn_eps=model.hp.bn_eps)
    xi = img(x, B, T4, F4, C).cpu().requires_grad_(True)
    convs, conv2d = [], Fn.conv2d

    def rec(a, *args, **kw):                                # the two convolutions' inputs and outputs (their gradients)
        o = conv2d(a, *args, **kw)
        o.retain_grad()
        convs.append((a, o))
        return o
    Fn.conv2d = rec
    try:
        yr = xi + s2t_ref.conv_attention_2d(W, p, xi, cfg, training, {})
    finally:
        Fn.conv2d = conv2d
    yr.backward(img(dout, B, T4, F4, C).cpu())
    # sums of |terms| of the convolutions' parameter gradients: with training-mode BatchNorm after them, the exact bias gradients
    # are ~0 and the weight gradients cancel, so their error is measured against these
    mag = {}
    for (a, o), nm in zip(convs, ("in_proj", "out_proj")):
        wn = "in_proj_weight" if nm == "in_proj" else "out_proj.weight"
        bn_ = "in_proj_bias" if nm == "in_proj" else "out_proj.bias"
        mag[wn] = torch.nn.grad.conv2d_weight(a.detach().abs(), W[p + wn].shape, o.grad.abs(), padding=1)
        mag[bn_] = o.grad.abs().sum((0, 2, 3))
    qp, kp = planes(c["qkv"], B, T4, F4, 0), planes(c["qkv"], B, T4, F4, H)
    E1 = gam(T4) * float((qp.abs().transpose(1, 2) @ kp.abs()).max())     # the frequency scores' f32 error (see e_S above)
    tol = (1e-3 if dtype == F32 else 0.3) + 8 * E1
    key = "block_grad_" + ("f32" if dtype == F32 else "bf16")
    checks = [("dx", d64(dx, "cpu"), unimg(xi.grad))] + [(nm, d64(A.g(p + nm), "cpu").view(-1), W[p + nm].grad.view(-1)) for nm in BLOCK]
    for nm, got, ref in checks:
        err = float((got - ref).norm())
        bound = tol * max(float(ref.norm()), float(mag[nm].norm()) if nm in mag else 0.0)
        WORST[key] = max(WORST.get(key, 0.0), err / bound)
        assert err <= bound, "%s grad %s: normwise error %.3g > %.3g (%g of |g_ref| or |sum of |terms||)" % (what, nm, err, bound, tol)
