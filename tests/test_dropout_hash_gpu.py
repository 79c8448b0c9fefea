"""s2t_dropout (csrc/loss_embed.hip) against the host statement of the rule in tests/dropout_ref.py, bit for bit: which elements are
kept, what a kept element becomes (f32(x) / (1 - p) rounded once to the type) and what a dropped one becomes (+0), for both types,
the 16-byte and the element-wise path, sizes around a quad and past the grid's cap, seeds that use all 64 bits and rates at the
threshold's edges.  Every other kernel's mask is tested for equality with s2t_dropout at the same seed, so this file is what ties all
of them to a statement of the bits; the direct case at the end does the same for the 128-wide GEMM epilogue's two index forms.

Indices >= 2^34 (where the index's own high word enters the hash) need a tensor of 32 GB and more: that term is covered on the CPU
only (test_dropout_ref_cpu.py), no test here reaches it."""
import numpy as np
import pytest
import torch

import dropout_ref as R

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
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
GUARD = 77.0
LEADS = pytest.mark.parametrize("lead", [8, 1], ids=["aligned", "offset"])
HIGH = (5 << 32) | 7
GRID_N = {F32: 4096 * 256 * 4 + 5, BF: 4096 * 256 * 8 + 5}      # past the 4,096-workgroup cap of the 16-byte path: a second grid-stride turn
TOP_P = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # the largest f32 below 1


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32).numpy()


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


def assert_same_bits_nan_aware(got, want, what):
    gn, wn = torch.isnan(got.float()).numpy(), torch.isnan(want.float()).numpy()
    assert np.array_equal(gn, wn), "%s: NaN must stay NaN where it is kept, and nothing else may become one" % (what,)
    bad = np.nonzero(bits(got)[~wn] != bits(want)[~wn])[0]
    assert bad.size == 0, "%s: %d elements differ from the rule, the first at %d" % (what, bad.size, int(np.nonzero(~wn)[0][bad[0]]))


def raw_dropout(x, y, p, seed):
    return K._lib().s2t_dropout(L.dt(x), L.ptr(x), L.ptr(y), x.numel(), p, seed, L.stream())


def mixed(n, seed, dtype):
    """magnitudes over twelve decades; +-0, +-inf, NaN, the smallest positive (subnormal) and the largest finite value of the type
    (which overflows once rescaled) and their negatives planted at the front and, when there is room, again at the very end"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-6, 6, (n,), generator=g).float())).to(dtype)
    fi = torch.finfo(dtype)
    tiny = 2.0 ** -133 if dtype == BF else 2.0 ** -149
    sp = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), tiny, -tiny, fi.max, -fi.max, fi.tiny], dtype=torch.float64).to(dtype)
    k = min(n, sp.numel())
    x[:k] = sp[:k]
    if n >= 4 * sp.numel():
        x[-sp.numel():] = sp
    return x


def check(dtype, n, lead, p, seed, in_place=False):
    x = mixed(n, n + 11, dtype)
    xd, xb = place(x, lead)
    yd, yb = (xd, xb) if in_place else place(torch.full((n,), float("nan"), dtype=dtype), lead)
    assert raw_dropout(xd, yd, p, seed) == 0
    what = "s2t_dropout %s n=%d %s p=%r seed=%#x%s" % (dtype, n, "aligned" if lead == 8 else "offset", p, seed, " in place" if in_place else "")
    assert_same_bits_nan_aware(yd.cpu(), R.apply(x, seed, p), what)
    guards_intact(yb, lead, what)
    if not in_place:
        assert_same_bits_nan_aware(xd.cpu(), x, what + ": the input was written")


@LEADS
@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 8, 9, 1000, 4099])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_sizes(dtype, n, lead):
    check(dtype, n, lead, 0.25, 77)


@LEADS
@pytest.mark.parametrize("dtype", DTYPES)
def test_grid_stride(dtype, lead):
    """16 MB of input per type: 4,096 workgroups x 256 threads x one 16-byte access, and five elements more"""
    check(dtype, GRID_N[dtype], lead, 0.25, 77)


@LEADS
@pytest.mark.parametrize("seed", [0, 77, 1000002999, 2 ** 32 - 1, 2 ** 32, HIGH, 2 ** 64 - 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_seeds_of_all_64_bits(dtype, seed, lead):
    check(dtype, 4099, lead, 0.25, seed)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_package_entry_carries_a_64_bit_seed(dtype):
    """K.dropout hands its seed through int() and the generated binding: 2^64 - 1 and a seed with only high bits must arrive whole"""
    x = mixed(4099, 3, dtype)
    for seed in (2 ** 64 - 1, HIGH, 1 << 63):
        y = K.dropout(x.to(DEV), 0.25, seed)
        assert_same_bits_nan_aware(y.cpu(), R.apply(x, seed, 0.25), "K.dropout seed=%#x" % seed)
    assert not np.array_equal(bits(K.dropout(x.to(DEV), 0.25, 1 << 63)), bits(K.dropout(x.to(DEV), 0.25, 0)))


@LEADS
@pytest.mark.parametrize("p", [2.0 ** -17, 2.0 ** -16, 0.1, 0.3, 0.5, 0.999, TOP_P], ids=["2^-17", "2^-16", "0.1", "0.3", "0.5", "0.999", "below1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rates(dtype, p, lead):
    """th16 = 0 (everything kept, rescaled by 1 / (1 - 2^-17)), 1, the model's rates, 65470 and 65535 (1 / (1 - p) = 2^24)"""
    check(dtype, 4099, lead, p, 77)


@LEADS
@pytest.mark.parametrize("n", [7, 4099])
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place(dtype, n, lead):
    check(dtype, n, lead, 0.25, HIGH, in_place=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_negative_control(dtype):
    """on the case for which test_dropout_ref_cpu.py asserts that every twin differs from the rule: the device's mask is the rule's
    and is none of the twins' (fields in another order, the seed's high word ignored, a full multiply, > for >=)"""
    n, p, seed = R.CONTROL["n"], R.CONTROL["p"], R.CONTROL["seed"]
    ones = torch.ones(n, dtype=dtype)
    for lead in (8, 1):
        (xd, _), (yd, _) = place(ones, lead), place(torch.zeros(n, dtype=dtype), lead)
        assert raw_dropout(xd, yd, p, seed) == 0
        mask = (yd != 0).cpu().numpy()
        assert np.array_equal(mask, R.keep_range(seed, n, p))
        for name, twin in R.TWINS.items():
            assert not np.array_equal(mask, twin.keep_range(seed, n, p)), "the device draws the mask of the wrong twin " + name


# ------------------------------------------------------------------ the 128-wide GEMM epilogue, directly against the rule
@pytest.mark.parametrize("seed", [77, HIGH], ids=["low", "high"])
@pytest.mark.parametrize("N", [64, 70, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogue_mask_is_the_rule(dtype, N, seed):
    """out = dropout(A W^T + 8) on the flat output index row * N + col.  N = 64 takes the epilogue's quad form; at N = 70 and 3 a
    hash quad straddles two output rows and the per-element form runs.  |A W^T| stays far below the bias of 8, so no kept output is
    zero and out != 0 is the mask"""
    M, Kd, p = 77, 72, 0.25
    g = torch.Generator().manual_seed(N)
    a = (torch.rand(M, Kd, generator=g) - 0.5).to(dtype).to(DEV)
    w = (torch.rand(N, Kd, generator=g) * 0.1).to(dtype).to(DEV)
    bias = torch.full((N,), 8.0, device=DEV)
    assert float((a.double() @ w.double().t()).abs().max()) < 4.0
    out = K.gemm(a, w, bias=bias, p_drop=p, seed=seed)
    assert out.shape == (M, N) and out.is_contiguous()
    mask = (out != 0).cpu().numpy().reshape(-1)
    want = R.keep(seed, np.arange(M * N, dtype=np.uint64), p)
    assert np.array_equal(mask, want), "%d of %d decisions differ from the rule" % (int((mask != want).sum()), M * N)
    # a kept output is the f32 sum times 1 / (1 - p), rounded once; the plain output it is compared with was rounded once as well, and
    # the f32 product rounds in between: 2 roundings of the type and one of f32, relative to the value
    plain = K.gemm(a, w, bias=bias)
    inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    kept = torch.from_numpy(want).reshape(M, N)
    tol = (2 * (2.0 ** -24 if dtype == F32 else 2.0 ** -8) + 2.0 ** -24) * 1.01
    ref = plain.cpu().double() * inv
    assert bool(((out.cpu().double() - ref).abs()[kept] <= tol * ref.abs()[kept]).all())
