"""Every kernel route of include/s2t_hip.h's s2t_set_option, on both sides of its switch, against float64 references.

The header promises that the route options change nothing beyond rounding.  Each case here
  * pins its route with `set_option` (a context manager: the old value comes back in `finally`, so a failed case cannot leak a
    route into the rest of the suite),
  * proves the route ran: a launch count of the kernel family (K.prof_read), gemm256's tile count (K.relu_mask_bytes / 8192), or,
    where the library has no witness, the dispatch rule it relies on, cited by file and condition,
  * checks every output ELEMENT against a float64 reference of the same exact inputs with a bound derived from the arithmetic
    (derivations in the docstrings), and reports the worst element, its value and its bound when it fails.

A missing or doubled k-tile, a tile written by the wrong workgroup or a dropped ragged row misses these bounds by orders of
magnitude; rounding stays well inside them.  tests/test_route_options_cpu.py checks that every option key is set somewhere here.
Attention here is d = 64 with the default scale; tests/test_attention_modes_gpu.py has d = 32, the distance penalty, LSE, the dropout
mask itself, s2t_attn_probs_avg and the layouts that leave the second-generation kernels.
"""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
DEV = "cuda"
U32 = 2.0 ** -24                 # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF, F32 = torch.bfloat16, torch.float32
FAMILIES = ("gemm_nt", "gemm_nt_small", "gemm_nn", "gemm_nn_small", "gemm_tn", "gemm_tn_small", "gemm256_nt", "gemm256_nn",
            "gemm_gather", "wgrad_group", "wgrad_group_f32", "attn_fwd", "attn_bwd")


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K
    from fbk_fairseq_st_amd import kernels
    K = kernels
    K._lib()
    yield
    K.prof_enable(0)


# ------------------------------------------------------------------ shared tools
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


def only(counts, fam):
    """the GEMM launches of a block were all of family `fam`"""
    ran = {f: n for f, n in counts.items() if n and f.startswith("gemm")}
    assert set(ran) == {fam}, "expected only %s launches, saw %s" % (fam, ran)


def rnd(*shape, dtype=F32, seed=0, scale=1.0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def ref_dev(flops):
    """float64 references run on the CPU; the few products above ~10 GFLOP use float64 on the device"""
    return DEV if flops > 1e10 else "cpu"


def d64(t, dev="cpu"):
    return t.detach().to(dev).double()


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


def op(t, trans):
    return t.t() if trans else t


class Gemm:
    """float64 reference of C = epi(alpha op(A) op(B)) and its error bound.

    Accumulation: every MFMA form multiplies bf16 x bf16 exactly in f32 (f32 x f32: the exact-f32 MFMA, one rounding per product)
    and adds K products in some f32 order; any order errs by at most (K - 1) u sum_k |a_ik b_kj| (u = 2^-24), plus u per product
    rounding, alpha's scaling, the bias add and the K-tail / split-K partial sums (each at most one more u |.| on a partial sum of the
    same terms).  So  |acc - ref| <= 4 K u (|A| |B|)_ij  (the issue's bound; the factor 4 covers those few extra roundings).
    Epilogue: an activation with slope <= s scales that by s (ReLU 1, erf-GELU 1.13, the backward masks 1, gelu' <= 1.13) and adds
    the f32 evaluation error of the function (erf / exp: a few u of |pre|, bounded by 2^-20 |pre|); every rounding of a value v to
    the output dtype adds r |v| with r = 2^-8 (bf16) or 2^-24 (f32) -- once for the activated value, once more for a residual or an
    accumulate (the epilogue rounds, adds the old value, rounds again), and 1/(1-p) scales kept values under dropout.
    K tail (gemm.hip gemm_run: K % BK != 0, K >= 8 BK, no epilogue): the whole k-tiles and the tail are two launches, the second
    accumulating into the first one's OUTPUT, so each partial product is rounded to the output dtype: + r (|P_main| + |P_tail|)."""

    def __init__(self, a, b, ta, tb, alpha=1.0, bias=None):
        self.M = a.shape[1] if ta else a.shape[0]
        self.K_ = a.shape[0] if ta else a.shape[1]
        self.N = b.shape[1] if tb else b.shape[0]
        self.dev = ref_dev(4.0 * self.M * self.N * self.K_)
        A, B = op(d64(a, self.dev), ta), op(d64(b, self.dev), not tb)
        self.acc = alpha * (A @ B)
        self.accb = 4 * self.K_ * U32 * abs(alpha) * (A.abs() @ B.abs())
        if bias is not None:
            self.acc = self.acc + d64(bias, self.dev)
            self.accb = self.accb + U32 * self.acc.abs()

    def t(self, x):
        return d64(x, self.dev)

    def tail_rounding(self, a, b, ta, tb, r):
        """r (|P_main| + |P_tail|) where gemm_run splits off a K tail (plain products only), else 0"""
        bk = 64 if a.dtype == BF else 32
        tail = self.K_ % bk
        if not tail or self.K_ < 8 * bk:
            return torch.zeros_like(self.acc)
        A, B = op(d64(a, self.dev), ta), op(d64(b, self.dev), not tb)
        km = self.K_ - tail
        return r * ((A[:, :km] @ B[:km]).abs() + (A[:, km:] @ B[km:]).abs())


def r_of(dtype):
    return UBF if dtype == BF else U32


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def check_epilogues(a, b, ta, tb, odt, fam, what, out_view=False):
    """bias, residual, ReLU, GELU with aux_out, ACT_RELU_BWD / ACT_GELU_BWD with alpha, accumulate and dropout on one product;
    every launch must be of family `fam` (None: no family check).  Every epilogue runs on every layout (NT, NN, TN), also those
    the model never combines: the C ABI accepts them all, so every kernel a product can reach must apply them."""
    r = r_of(odt)
    M = a.shape[1] if ta else a.shape[0]
    N = b.shape[1] if tb else b.shape[0]
    bias = rnd(N, seed=11, scale=0.5)
    g = Gemm(a, b, ta, tb, bias=bias)
    res = rnd(M, N, dtype=odt, seed=12)
    with launches() as c:
        if out_view:                   # a padded output row stride: C is a view of a wider buffer
            wide = torch.full((M, N + 13), 7.0, dtype=odt, device=DEV)
            out = K.gemm(a, b, ta, tb, bias=bias, out=wide[:, :N])
            assert_close(out, g.acc, g.accb + r * g.acc.abs(), what + " bias (ldc view)")
            assert bool((wide[:, N:] == 7.0).all()), what + ": a store landed in the row padding"
        out = K.gemm(a, b, ta, tb, bias=bias, out_dtype=odt)
        assert_close(out, g.acc, g.accb + r * g.acc.abs(), what + " bias")
        out = K.gemm(a, b, ta, tb, bias=bias, residual=res, out_dtype=odt)
        ref = g.acc + g.t(res)
        assert_close(out, ref, g.accb + r * (g.acc.abs() + ref.abs()), what + " bias+residual")
        out = K.gemm(a, b, ta, tb, bias=bias, act=K.ACT_RELU, out_dtype=odt)
        ref = g.acc.clamp_min(0)
        assert_close(out, ref, g.accb + r * ref.abs(), what + " bias+relu")
        out = K.gemm(a, b, ta, tb, bias=bias, act=K.ACT_RELU, residual=res, out_dtype=odt)
        ref = g.acc.clamp_min(0) + g.t(res)
        assert_close(out, ref, g.accb + r * (g.acc.abs() + ref.abs()), what + " bias+relu+residual")
        pre = torch.empty(M, N, dtype=odt, device=DEV)
        out = K.gemm(a, b, ta, tb, bias=bias, act=K.ACT_GELU, aux_out=pre, out_dtype=odt)
        assert_close(pre, g.acc, g.accb + r * g.acc.abs(), what + " gelu aux_out")
        ref = gelu64(g.acc)
        assert_close(out, ref, 1.13 * g.accb + 2.0 ** -20 * g.acc.abs() + r * ref.abs(), what + " bias+gelu")
        # dropout: the keep pattern is the standalone s2t_dropout's on the same [M, N] index space, on every form
        p = 0.25
        out = K.gemm(a, b, ta, tb, bias=bias, p_drop=p, seed=1234, out_dtype=odt)
        keep = K.dropout(torch.ones(M, N, dtype=odt, device=DEV), p, 1234) != 0
        ref = torch.where(keep.to(g.dev), g.acc / (1 - p), torch.zeros_like(g.acc))
        assert_close(out, ref, (g.accb + r * g.acc.abs()) / (1 - p), what + " dropout")
        sure = (g.acc.abs() > 2 * g.accb).to(DEV)          # values that cannot round to zero
        assert torch.equal((out != 0) & sure, keep & sure), what + ": dropout keep pattern differs from s2t_dropout's"
        g0 = Gemm(a, b, ta, tb, alpha=1.25)
        aux = rnd(M, N, dtype=odt, seed=13)
        out = K.gemm(a, b, ta, tb, act=K.ACT_RELU_BWD, aux=aux, alpha=1.25, out_dtype=odt)
        ref = torch.where(g0.t(aux) > 0, g0.acc, torch.zeros_like(g0.acc))
        assert_close(out, ref, g0.accb + r * ref.abs(), what + " relu_bwd alpha")
        out = K.gemm(a, b, ta, tb, act=K.ACT_GELU_BWD, aux=aux, alpha=1.25, out_dtype=odt)
        ref = g0.acc * gelu_grad64(g0.t(aux))
        assert_close(out, ref, 1.13 * g0.accb + 2.0 ** -20 * g0.acc.abs() + r * ref.abs(), what + " gelu_bwd alpha")
        base = rnd(M, N, dtype=odt, seed=14)
        acc = base.clone()
        g1 = Gemm(a, b, ta, tb)
        K.gemm(a, b, ta, tb, out=acc, accumulate=True)
        ref = g1.acc + g1.t(base)
        bound = g1.accb + r * (g1.acc.abs() + ref.abs()) + g1.tail_rounding(a, b, ta, tb, r)
        assert_close(acc, ref, bound, what + " accumulate")
    if fam is not None:
        only(c, fam)


# ------------------------------------------------------------------ bf16 64 x 64 form: gemm_deep on / off, k-tile counts around the depth
# gemm.hip: BK = 128 / sizeof(bf16) = 64; DEPTH = 8 (NT) / 4 (NN, TN) for the 64 x 64 four-wave bf16 form; the deep loop runs when
# gemm_deep != 0 and nk % DEPTH == 0 (gemm_fast_kernel), the two-set loop otherwise.  K = 9 x 64 + 17 >= 8 k-tiles with a ragged tail:
# gemm_run sends whole k-tiles to the fast kernel and the tail to a second launch.
DEEP_CASES = [
    # layout, M, N, K
    ("nt", 997, 701, 7 * 64), ("nt", 997, 701, 8 * 64), ("nt", 997, 701, 9 * 64 + 17), ("nt", 203, 131, 16 * 64),
    ("nn", 501, 299, 3 * 64), ("nn", 501, 299, 4 * 64), ("nn", 501, 299, 5 * 64), ("nn", 501, 299, 9 * 64 + 17), ("nn", 77, 90, 8 * 64),
    ("tn", 509, 261, 3 * 64), ("tn", 509, 261, 4 * 64), ("tn", 509, 261, 12 * 64),
]


def _operands(layout, M, N, K_, dtype, seed=1, pad=0):
    """A, B for op(A)[M,K] op(B)[K,N] of the layout; pad > 0: both are views of wider buffers (row stride + pad, rounded to 8)"""
    shp_a = (K_, M) if layout == "tn" else (M, K_)
    shp_b = (N, K_) if layout == "nt" else (K_, N)

    def mk(shp, s, sc):
        cols = shp[1]
        ld = cols if not pad and (layout == "nt" or cols % 8 == 0) else (cols + pad + 7) // 8 * 8
        buf = rnd(shp[0], ld, dtype=dtype, seed=s, scale=sc)
        return buf[:, :cols]
    return mk(shp_a, seed, 1.0), mk(shp_b, seed + 1, K_ ** -0.5)


def _ta_tb(layout):
    return layout == "tn", layout != "nt"


@pytest.mark.parametrize("layout,M,N,K_", DEEP_CASES)
def test_gemm64_deep_prefetch_both_loops(layout, M, N, K_):
    """gemm_deep 1 and 0 on the 64 x 64 form (gemm_nt_small / gemm_nn_small / gemm_tn_small): fp64 bound, identical bits between the
    two loops (include/s2t_hip.h: "bit-identical results"), and identical bits over 5 launches of each (a cheap net for LDS races
    like the deep loop's missing end barrier)"""
    ta, tb = _ta_tb(layout)
    a, b = _operands(layout, M, N, K_, BF, pad=8)
    odt = F32 if layout == "tn" else BF
    g = Gemm(a, b, ta, tb)
    res = {}
    for deep in (1, 0):
        with set_option("gemm_deep", deep), launches() as c:
            outs = [K.gemm(a, b, ta, tb, out_dtype=odt) for _ in range(5)]
        only(c, "gemm_%s_small" % layout)
        for o in outs[1:]:
            assert torch.equal(o, outs[0]), "gemm_deep=%d: reruns differ (race?)" % deep
        bound = g.accb + r_of(odt) * g.acc.abs() + g.tail_rounding(a, b, ta, tb, r_of(odt))
        assert_close(outs[0], g.acc, bound, "%s deep=%d" % (layout, deep))
        res[deep] = outs[0]
    assert torch.equal(res[0], res[1]), "gemm_deep 0 and 1 disagree"


def test_gemm64_deep_epilogues():
    """every epilogue on the deep loop (NT: nk = 8, NN: nk = 4), gemm_deep on"""
    with set_option("gemm_deep", 1):
        a, b = _operands("nt", 997, 701, 512, BF)
        check_epilogues(a, b, False, False, BF, "gemm_nt_small", "nt64 deep", out_view=True)
        a, b = _operands("nn", 501, 299, 256, BF, pad=8)
        check_epilogues(a, b, False, True, BF, "gemm_nn_small", "nn64 deep")
        a, b = _operands("tn", 509, 261, 256, BF, pad=8)
        check_epilogues(a, b, True, True, F32, "gemm_tn_small", "tn64 deep")


# ------------------------------------------------------------------ thresholds and forms
# gemm.hip gemm_run: t128 = ceil(M/128) ceil(N/128) splitk; small = t128 < gemm_small_nt (NT) / gemm_small_kt (NN, TN) for bf16,
# gemm_f32_small_nt / _kt for f32; narrow (128 x 64) = !small && (N <= 64 || (f32 && t128 < gemm_f32_narrow)); big (gemm256) =
# bf16 && !trans_a && !small && the gates of s2t_gemm256_try (>= 160 tiles of 192 rows).  The narrow form reports as the 128-wide
# family: there the rule above is the witness.
FORMS = [
    # id, dtype, out dtype, layout, M, N, K, family
    ("bf16_nt_192tiles_128", BF, BF, "nt", 1531, 2045, 512, "gemm_nt"),          # 12 x 16 = 192 tiles: at the threshold
    ("bf16_nt_180tiles_64", BF, BF, "nt", 1531, 1917, 512, "gemm_nt_small"),     # 12 x 15 = 180
    ("bf16_nt_batch8_128", BF, BF, "nt", 3000, 2048, 512, "gemm_nt"),            # 384 tiles; 16 x 8 = 128 tiles of 192 rows < 160
    ("bf16_nn_40tiles_128", BF, BF, "nn", 637, 1021, 320, "gemm_nn"),            # 5 x 8 = 40
    ("bf16_nn_35tiles_64", BF, BF, "nn", 637, 893, 320, "gemm_nn_small"),        # 5 x 7 = 35
    ("bf16_nn_96tiles_128", BF, BF, "nn", 1531, 1021, 512, "gemm_nn"),           # 96 tiles
    ("bf16_nt_narrow", BF, BF, "nt", 30000, 64, 512, "gemm_nt"),                 # N <= 64, 235 tiles: 128 x 64
    ("bf16_nt_narrow_ragged", BF, BF, "nt", 29999, 61, 200, "gemm_nt"),          # ragged K: guarded 128 x 64 kernel
    ("bf16_f32out_nt_128", BF, F32, "nt", 1531, 2045, 512, "gemm_nt"),
    ("bf16_f32out_nt_64", BF, F32, "nt", 997, 701, 512, "gemm_nt_small"),
    ("bf16_f32out_nt_narrow", BF, F32, "nt", 30000, 64, 512, "gemm_nt"),
    ("bf16_f32out_nn_128", BF, F32, "nn", 637, 1021, 320, "gemm_nn"),
    ("bf16_f32out_nn_64", BF, F32, "nn", 637, 893, 320, "gemm_nn_small"),
    ("f32_nt_1008tiles_64", F32, F32, "nt", 8060, 2045, 256, "gemm_nt_small"),   # 63 x 16 = 1,008 < 1,024
    ("f32_nt_1024tiles_128", F32, F32, "nt", 8190, 2045, 256, "gemm_nt"),        # 64 x 16 = 1,024
    ("f32_nn_512tiles_128", F32, F32, "nn", 2045, 4093, 96, "gemm_nn"),          # 16 x 32 = 512
    ("f32_nn_496tiles_64", F32, F32, "nn", 2045, 3965, 96, "gemm_nn_small"),     # 16 x 31 = 496
    ("bf16_tn_40tiles_128", BF, BF, "tn", 637, 1021, 320, "gemm_tn"),            # 5 x 8 = 40 (gemm_small_kt)
    ("bf16_tn_35tiles_64", BF, BF, "tn", 637, 893, 320, "gemm_tn_small"),        # 5 x 7 = 35
    ("bf16_f32out_tn_128", BF, F32, "tn", 637, 1021, 320, "gemm_tn"),            # fast, K >= 4 x 64: the two-slice dW kernel's shape
    ("bf16_f32out_tn_64", BF, F32, "tn", 637, 893, 320, "gemm_tn_small"),
    ("bf16_f32out_tn_128_ragged_k", BF, F32, "tn", 637, 1021, 300, "gemm_tn"),   # guarded kernel
    ("f32_tn_512tiles_128", F32, F32, "tn", 2045, 4093, 96, "gemm_tn"),          # 16 x 32 = 512 (gemm_f32_small_kt)
    ("f32_tn_496tiles_64", F32, F32, "tn", 2045, 3965, 96, "gemm_tn_small"),
]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_gemm_forms_epilogues(form):
    """each GEMM form under the default thresholds, every epilogue, ragged M / N (and K where named), fp64 bound"""
    name, dt, odt, layout, M, N, K_, fam = form
    ta, tb = _ta_tb(layout)
    a, b = _operands(layout, M, N, K_, dt, pad=0 if layout == "nt" else 8)
    check_epilogues(a, b, ta, tb, odt, fam, name, out_view=(layout == "nt"))


def test_gemm_f32_narrow_form():
    """gemm_f32_narrow above the tile count sends f32 products to the 128 x 64 form (with gemm_f32_small_nt / _kt at 0 so that they are
    not small); the family is the 128-wide one (gemm.hip: narrow = !small && (... || (f32in && t128 < g_s2t_opt_f32_narrow)))"""
    with set_option("gemm_f32_small_nt", 0), set_option("gemm_f32_small_kt", 0), set_option("gemm_f32_narrow", 1 << 20):
        a, b = _operands("nt", 1000, 701, 256, F32)
        check_epilogues(a, b, False, False, F32, "gemm_nt", "f32 nt narrow", out_view=True)
        a, b = _operands("nn", 637, 893, 96, F32, pad=8)
        check_epilogues(a, b, False, True, F32, "gemm_nn", "f32 nn narrow")
        a, b = _operands("tn", 637, 893, 96, F32, pad=8)
        check_epilogues(a, b, True, True, F32, "gemm_tn", "f32 tn narrow")


@pytest.mark.parametrize("M,N,K_", [(5, 3, 8), (77, 100, 72), (130, 70, 136), (1, 257, 64)])
def test_gemm_small_thresholds_zero_sends_tiny_products_to_128_wide(M, N, K_):
    """gemm_small_nt / gemm_small_kt = 0: nothing is small, the 128-wide kernels (128 x 64 where N <= 64) run tiny ragged products"""
    with set_option("gemm_small_nt", 0), set_option("gemm_small_kt", 0):
        a, b = _operands("nt", M, N, K_, BF)
        check_epilogues(a, b, False, False, BF, "gemm_nt", "nt tiny 128")
        a, b = _operands("nn", M, N, K_, BF, pad=8)
        check_epilogues(a, b, False, True, BF, "gemm_nn", "nn tiny 128")
        a, b = _operands("tn", M, N, K_, BF, pad=8)
        check_epilogues(a, b, True, True, F32, "gemm_tn", "tn tiny 128")


def test_gemm_small_thresholds_huge_send_m24000_to_64_wide():
    """gemm_small_nt / _kt very large: the 64 x 64 form runs the encoder's M = 24,000 products (NT with epilogues, NN, TN)"""
    with set_option("gemm_small_nt", 1 << 30), set_option("gemm_small_kt", 1 << 30):
        a, b = _operands("nt", 24000, 512, 512, BF)
        check_epilogues(a, b, False, False, BF, "gemm_nt_small", "nt M=24000 small")
        a, b = _operands("nn", 24000, 512, 512, BF)
        check_epilogues(a, b, False, True, BF, "gemm_nn_small", "nn M=24000 small")


# ------------------------------------------------------------------ TN (linear_wgrad, split-K)
@pytest.mark.parametrize("dt,n_out,n_in,tokens,split,fam", [
    (BF, 509, 637, 2000, 1, "gemm_tn_small"),        # 4 x 5 = 20 tiles x 1 < 40
    (BF, 509, 637, 2000, 2, "gemm_tn"),              # 20 x 2 = 40
    (BF, 509, 637, 3001, 4, "gemm_tn"),              # ragged tokens: guarded kernel
    (BF, 2045, 517, 24000, 3, "gemm_tn"),
    (F32, 2045, 2045, 1000, 1, "gemm_tn_small"),     # 256 tiles < 512
    (F32, 2045, 2045, 1000, 2, "gemm_tn"),           # 256 x 2 = 512
    (F32, 2048, 2044, 1024, 1, "gemm_tn_small"),     # aligned: fast 64 x 64
    (F32, 2048, 2044, 1024, 2, "gemm_tn"),           # aligned: fast 128 x 128
])
def test_linear_wgrad_tn_routes(dt, n_out, n_in, tokens, split, fam):
    """dW += dY^T X (f32, split-K atomics) and db += colsum(dY) on both sides of the TN thresholds; the bound adds split partial sums
    (one u per partial) -- inside 4 K u (|A| |B|) -- and for db: tokens u sum |dy| + the same for the split"""
    dy = rnd(tokens, n_out, dtype=dt, seed=1)
    x = rnd(tokens, n_in, dtype=dt, seed=2)
    dw0 = rnd(n_out, n_in, seed=3)
    db0 = rnd(n_out, seed=4)
    g = Gemm(dy, x, True, True)
    dw, db = dw0.clone(), db0.clone()
    with launches() as c:
        K.linear_wgrad(dy, x, dw, db, splitk=split)
    only(c, fam)
    ref = g.acc + g.t(dw0)
    assert_close(dw, ref, g.accb + U32 * ref.abs() * split, "dW")
    dyd = d64(dy)
    refb = dyd.sum(0) + d64(db0)
    assert_close(db, refb, 4 * tokens * U32 * dyd.abs().sum(0) + U32 * refb.abs() * split, "db")


# ------------------------------------------------------------------ gemm256, reserve_cus
def _g256_tiles(M, N, K_):
    return K.relu_mask_bytes(M, N, K_) // 8192


def _tiles_expected(M, N, cus):
    """gemm256.hip g256_tiles restated: the row height that needs fewer rows x rounds on `cus` workgroups (ties to 256)"""
    tn = (N + 255) // 256
    t256, t192 = (M + 255) // 256 * tn, (M + 191) // 192 * tn
    use192 = (t192 + cus - 1) // cus * 192 < (t256 + cus - 1) // cus * 256
    return t192 if use192 else t256


RESERVES = [0, 1, 16, 100, 128]
G256_SHAPES = [(24000, 2048, 512), (6211, 1536, 512), (12000, 768, 128)]


@pytest.mark.parametrize("M,N,K_", G256_SHAPES)
def test_gemm256_reserve_cus(M, N, K_):
    """reserve_cus in {0, 1, 16, 100, 128}: gemm256 launches 256 - value workgroups and picks the row-tile height for that many
    (fc1 at 24,000 x 2,048 x 512: 752 tiles of 256 rows at 256 CUs, 1,000 of 192 at 240).  NT with bias + ReLU and with bias +
    residual, NN with accumulate, each against fp64; bit-identical across reserve values of the same tile height (one workgroup
    computes a tile in one K order); across heights only the bound is required (the bits are reported)."""
    a, b = _operands("nt", M, N, K_, BF, seed=5)
    bias = rnd(N, seed=6, scale=0.5)
    res = rnd(M, N, dtype=BF, seed=7)
    g = Gemm(a, b, False, False, bias=bias)
    wt = rnd(N, K_, dtype=BF, seed=8, scale=N ** -0.5)        # NN: dX[M, K_] = dY[M, N] W, W as it lies in memory [N][K_]
    dy = rnd(M, N, dtype=BF, seed=9)
    base = rnd(M, K_, dtype=BF, seed=10)
    gn = Gemm(dy, wt, False, True)
    by_height, notes = {}, []
    for rsv in RESERVES:
        with set_option("reserve_cus", rsv):
            tiles = _g256_tiles(M, N, K_)
            assert tiles == _tiles_expected(M, N, 256 - rsv), (rsv, tiles)
            nn_big = _g256_tiles(M, K_, N) > 0                 # the NN product [M, K_] over N: on gemm256 where it has the tiles
            with launches() as c:
                o1 = K.gemm(a, b, bias=bias, act=K.ACT_RELU)
                o2 = K.gemm(a, b, bias=bias, residual=res)
                acc = base.clone()
                K.gemm(dy, wt, trans_b=True, out=acc, accumulate=True)
            assert c["gemm256_nt"] == 2 and c["gemm256_nn"] == int(nn_big) and c["gemm_nn"] == 1 - int(nn_big), c
        ref = g.acc.clamp_min(0)
        assert_close(o1, ref, g.accb + UBF * ref.abs(), "relu reserve=%d" % rsv)
        ref = g.acc + g.t(res)
        assert_close(o2, ref, g.accb + UBF * (g.acc.abs() + ref.abs()), "residual reserve=%d" % rsv)
        ref = gn.acc + gn.t(base)
        assert_close(acc, ref, gn.accb + UBF * (gn.acc.abs() + ref.abs()), "nn accumulate reserve=%d" % rsv)
        cur = (o1, o2, acc)
        h = tiles
        if h in by_height:
            for x, y in zip(by_height[h], cur):
                assert torch.equal(x, y), "reserve %d: bits differ from another reserve value with the same %d tiles" % (rsv, h)
        else:
            if by_height:
                first = next(iter(by_height.values()))
                notes.append("reserve %d (%d tiles) bit-identical to the first height: %s"
                             % (rsv, h, all(torch.equal(x, y) for x, y in zip(first, cur))))
            by_height[h] = cur
    if M == 24000 and N == 2048:
        assert set(by_height) == {752, 1000}, by_height.keys()
    for n in notes:
        print(n)


def test_gemm256_relu_record_follows_reserve_cus():
    """the 1-bit ReLU record (ACT_RELU_MASK forward, ACT_RELU_BWD_MASK backward) at reserve 16, where fc1's tile height flips to
    192 rows: K.relu_mask_bytes follows the option (kernels.py keys its cache on OPTION_EPOCH); forward == ACT_RELU bit for bit and
    within the fp64 bound, backward == ACT_RELU_BWD bit for bit and within its bound"""
    M, N, K_ = 24000, 2048, 512
    nb0 = K.relu_mask_bytes(M, N, K_)
    assert nb0 == 752 * 8192
    x, w = _operands("nt", M, N, K_, BF, seed=21)
    bias = rnd(N, seed=22, scale=0.1)
    dy = rnd(M, K_, dtype=BF, seed=23)
    w2 = rnd(K_, N, dtype=BF, seed=24, scale=0.05)
    with set_option("reserve_cus", 16):
        nb = K.relu_mask_bytes(M, N, K_)
        assert nb == 1000 * 8192, nb
        rec = torch.full((nb,), 0xA5, dtype=torch.uint8, device=DEV)
        with launches() as c:
            a = K.gemm(x, w, bias=bias, act=K.ACT_RELU_MASK, aux_out=rec)
            da = K.gemm(dy, w2, trans_b=True, act=K.ACT_RELU_BWD_MASK, aux=rec, alpha=1.25)
        assert c["gemm256_nt"] == 1 and c["gemm256_nn"] == 1, c
        assert torch.equal(a, K.gemm(x, w, bias=bias, act=K.ACT_RELU))
        assert torch.equal(da, K.gemm(dy, w2, trans_b=True, act=K.ACT_RELU_BWD, aux=a, alpha=1.25))
    assert K.relu_mask_bytes(M, N, K_) == nb0
    g = Gemm(x, w, False, False, bias=bias)
    ref = g.acc.clamp_min(0)
    assert_close(a, ref, g.accb + UBF * ref.abs(), "relu mask fwd reserve 16")
    gd = Gemm(dy, w2, False, True, alpha=1.25)
    ref = torch.where(d64(a, gd.dev) > 0, gd.acc, torch.zeros_like(gd.acc))      # the decision the forward recorded
    assert_close(da, ref, gd.accb + UBF * ref.abs(), "relu mask bwd reserve 16")


def test_gemm256_takes_m24000_n512_k512():
    """24,000 x 512 x 512 (250 tiles of 192 rows) runs as one gemm256_nt launch; fp64 bound.  (997 x 701 x 512 on gemm_nt_small:
    test_gemm64_deep_prefetch_both_loops, test_gemm64_deep_epilogues)"""
    a, b = _operands("nt", 24000, 512, 512, BF)
    g = Gemm(a, b, False, False)
    with launches() as c:
        out = K.gemm(a, b)
    only(c, "gemm256_nt")
    assert c["gemm256_nt"] == 1, c
    assert_close(out, g.acc, g.accb + UBF * g.acc.abs(), "gemm256 24000 x 512 x 512")


def test_gemm256_min_tiles_and_off_switch():
    """gemm256_min_tiles above a product's 192-row tile count and gemm256 = 0 both keep it on the 128 x 128 kernel; same bound"""
    a, b = _operands("nt", 6211, 1536, 512, BF, seed=31)     # 33 x 6 = 198 tiles of 192 rows
    g = Gemm(a, b, False, False)
    with launches() as c:
        out = K.gemm(a, b)
    only(c, "gemm256_nt")
    assert_close(out, g.acc, g.accb + UBF * g.acc.abs(), "default")
    with set_option("gemm256_min_tiles", 199), launches() as c:
        out = K.gemm(a, b)
    only(c, "gemm_nt")
    assert_close(out, g.acc, g.accb + UBF * g.acc.abs(), "gemm256_min_tiles 199")
    with set_option("gemm256", 0), launches() as c:
        out = K.gemm(a, b)
    only(c, "gemm_nt")
    assert_close(out, g.acc, g.accb + UBF * g.acc.abs(), "gemm256 0")
    with set_option("gemm256_min_tiles", 198):
        assert _g256_tiles(6211, 1536, 512) > 0


# ------------------------------------------------------------------ wgrad_group under reserve_cus
def _wg_items(dt, t_long, t_short, n_long, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def mk(tokens, n_out, n_in, has_b=True):
        dy = (torch.randn(tokens, n_out, device=DEV, generator=g) * 0.5).to(dt)
        x = (torch.randn(tokens, n_in, device=DEV, generator=g) * 0.5).to(dt)
        return (dy, x, torch.randn(n_out, n_in, device=DEV, generator=g), torch.randn(n_out, device=DEV, generator=g) if has_b else None)
    items = [mk(t_long, 1024, 512) for _ in range(n_long)]
    for _ in range(2):
        items += [mk(t_short, 1536, 512), mk(t_short, 512, 512), mk(t_short, 512, 2048)]
    items.append(mk(t_short, 1000, 512, has_b=False))
    return items


def _wg_check(items, init, what):
    """a tile's token range may be cut into pieces (at most one per K-tile, nk) that meet in f32 atomics on top of the initial dW:
    each add rounds once, (nk + 1) u (|dW0| + |ref|) on top of the accumulation bound"""
    for k, ((dy, x, dw, db), (w0, b0)) in enumerate(zip(items, init)):
        g = Gemm(dy, x, True, True)
        ref = g.acc + g.t(w0)
        nk = (dy.shape[0] + 63) // 64
        assert_close(dw, ref, g.accb + (nk + 1) * U32 * (g.t(w0).abs() + ref.abs()), "%s item %d dW" % (what, k))
        if db is not None:
            dyd = d64(dy, g.dev)
            refb = dyd.sum(0) + g.t(b0)
            assert_close(db, refb, 4 * dy.shape[0] * U32 * dyd.abs().sum(0) + 2 * U32 * refb.abs(), "%s item %d db" % (what, k))


@pytest.mark.parametrize("dt,fam", [(BF, "wgrad_group"), (F32, "wgrad_group_f32")])
def test_wgrad_group_reserve_cus(dt, fam):
    """grouped weight gradients with mixed reduction lengths at reserve 0 -> 16 -> 0 on the SAME item list: the bf16 list is re-planned
    for 240 workgroups and again for 256 (wgrad_group.hip: the cached lists are dropped when s2t_persistent_cus() changes); every pass
    against fp64 (the tail-round pieces meet in f32 atomics: 2 u |.| per element on top of the accumulation bound)"""
    items = _wg_items(dt, 6001, 333, 2, seed=17)
    init = [(dw.clone(), None if db is None else db.clone()) for _, _, dw, db in items]
    for rsv in (0, 16, 100, 0):
        for (_, _, dw, db), (w0, b0) in zip(items, init):
            dw.copy_(w0)
            if db is not None:
                db.copy_(b0)
        with set_option("reserve_cus", rsv), launches() as c:
            K.wgrad_group(items)
        assert c[fam] == 1, c
        _wg_check(items, init, "reserve %d" % rsv)


def test_wgrad_group_replans_when_reserve_cus_changes():
    """a list of exactly 256 tiles (16 x dW 2048 x 512) fills one round of 256 workgroups: no token cuts, no atomics, the same bits every
    launch.  At reserve 16 (240 workgroups) the re-planned list cuts the tail round along the tokens, whose pieces meet in f32
    atomics: the bits change (were the 256-workgroup list kept, they would not), the fp64 bound holds; back at 0, the first list
    and its bits return"""
    g = torch.Generator(device=DEV).manual_seed(3)
    dy = torch.randn(3000, 2048, device=DEV, generator=g).to(BF)
    x = torch.randn(3000, 512, device=DEV, generator=g).to(BF)
    items = [(dy, x, torch.zeros(2048, 512, device=DEV), None) for _ in range(16)]
    ref = Gemm(dy, x, True, True)

    def run(rsv):
        for it in items:
            it[2].zero_()
        with set_option("reserve_cus", rsv):
            K.wgrad_group(items)
        for k, it in enumerate(items):
            assert_close(it[2], ref.acc, ref.accb + 2 * U32 * ref.acc.abs(), "reserve %d item %d" % (rsv, k))
        return [it[2].clone() for it in items]
    r0 = run(0)
    assert all(torch.equal(t, r0[0]) for t in r0)
    r16 = run(16)
    assert not all(torch.equal(a, b) for a, b in zip(r0, r16)), "reserve 16 ran the 256-workgroup list (no re-plan)"
    r0b = run(0)
    assert all(torch.equal(a, b) for a, b in zip(r0, r0b)), "back at reserve 0 the list was not re-planned for 256 workgroups"


# ------------------------------------------------------------------ LayerNorm
def ln_ref(x, g, b, eps=1e-5):
    xd = d64(x)
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    return (xd - mu) * rstd * d64(g) + d64(b), mu.squeeze(-1), rstd.squeeze(-1)


def ln_check(x, gamma, beta, dy, dres, drop, what):
    """Forward.  mean and var are f32 sums of D terms: |dmu| <= D u mean|x|, |dvar| / var <= D u (mean x^2 / var + 1) (either the
    two-pass or the one-pass formula), so |dxhat| <= a (1 + |xhat|) with a = D u rstd (mean|x| + rstd mean x^2) + D u; y = g xhat + b
    adds u (|g xhat| + |b|) and the output rounding r |y|.  Bound: 4 |g| a (1 + |xhat|) + 2 u (|g xhat| + |b|) + r |y|.
    mean / rstd outputs (f32): 4 a / rstd and 4 a rstd.
    Backward, given the saved mean / rstd (the function it computes): xhat = (x - mean) rstd to 2 u |xhat|; g = dy gamma to u |g|;
    c1 = mean g, c2 = mean g xhat are D-term f32 sums (D u m1, D u m2 with m1 = mean|g|, m2 = mean|g xhat|); dx = rstd (g - c1 - xhat c2)
    (+ dres, one f32 add) -> |ddx| <= 4 rstd (u|g| + D u m1 + 2 u |xhat| |c2| + |xhat| D u m2) + 2 u |dx| + r |dx|.
    dgamma, dbeta: sums over the M rows in per-lane chains, an LDS reduction and one f32 atomic per workgroup (any order errs by at
    most depth u sum|terms|, depth <= M + 16 + 512), plus the recomputed xhat's 2 u |xhat| in every term and the final rounding:
    dgamma (M + 530) u sum|dy xhat| + 2 u sum |dy| |xhat| + u |dgamma|, dbeta (M + 530) u sum|dy| + u |dbeta|.
    dx_drop: the same bound times 1/(1-p) on kept elements, and its keep pattern is s2t_dropout's."""
    M, D = x.shape
    odt = x.dtype
    r = r_of(odt)
    y, mean, rstd = K.layernorm_fwd(x, gamma, beta)
    yr, mur, rsr = ln_ref(x, gamma, beta)
    xd = d64(x)
    a = D * U32 * rsr * (xd.abs().mean(-1) + rsr * (xd * xd).mean(-1)) + D * U32
    xh = (xd - mur[:, None]) * rsr[:, None]
    gd, bd = d64(gamma), d64(beta)
    assert_close(mean, mur, 4 * a / rsr, what + " mean")
    assert_close(rstd, rsr, 4 * a * rsr, what + " rstd")
    assert_close(y, yr, 4 * gd.abs() * a[:, None] * (1 + xh.abs()) + 2 * U32 * ((gd * xh).abs() + bd.abs()) + r * yr.abs(), what + " y")
    # backward with the kernel's statistics
    m, rs = d64(mean)[:, None], d64(rstd)[:, None]
    xh = (xd - m) * rs
    dyd = d64(dy)
    gg = dyd * gd
    c1, c2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    m1, m2 = gg.abs().mean(-1, keepdim=True), (gg * xh).abs().mean(-1, keepdim=True)
    dxr = rs * (gg - c1 - xh * c2)
    if dres is not None:
        dxr = dxr + d64(dres)
    bx = 4 * rs * (U32 * gg.abs() + D * U32 * m1 + 2 * U32 * xh.abs() * c2.abs() + xh.abs() * D * U32 * m2) + 2 * U32 * dxr.abs()
    dg = torch.zeros(D, device=DEV)
    db = torch.zeros(D, device=DEV)
    outs = K.layernorm_bwd(dy, x, mean, rstd, gamma, dg, db, dres=dres, drop=drop)
    dx = outs if drop is None else outs[0]
    assert_close(dx, dxr, bx + r * dxr.abs(), what + " dx")
    depth = M + 530
    refg = (dyd * xh).sum(0)
    assert_close(dg, refg, depth * U32 * (dyd * xh).abs().sum(0) + 2 * U32 * (dyd.abs() * xh.abs()).sum(0) + U32 * refg.abs(),
                 what + " dgamma")
    refb = dyd.sum(0)
    assert_close(db, refb, depth * U32 * dyd.abs().sum(0) + U32 * refb.abs(), what + " dbeta")
    if drop is not None:
        p, seed = drop
        keep = d64(K.dropout(torch.ones_like(x), p, seed)) != 0
        refd = torch.where(keep, dxr / (1 - p), torch.zeros_like(dxr))
        assert_close(outs[1], refd, (bx + r * dxr.abs()) / (1 - p) + r * refd.abs(), what + " dx_drop")
    return dx, bx


LN_MS = [1, 3, 8191, 8192, 24000]
LN_DS = [256, 512, 1024, 100]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", LN_DS)
@pytest.mark.parametrize("M", LN_MS)
def test_layernorm_rows_around_8192(M, D, dtype):
    """forward and backward across norm_optim.hip's row switch (big = M >= 8192: its own grid cap and row loop), with dres, and with
    dx_drop at the big sizes; D = 100 runs the element-wise form (ln_epl: epl = 0)"""
    x = rnd(M, D, dtype=dtype, seed=M + D, scale=2.0) + 0.5
    gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dy = rnd(M, D, dtype=dtype, seed=4)
    dres = rnd(M, D, dtype=dtype, seed=5) if M % 2 == 0 else None
    drop = (0.2, 99) if M >= 8191 else None
    ln_check(x, gamma, beta, dy, dres, drop, "LN M=%d D=%d" % (M, D))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [333, 24000])
def test_layernorm_unaligned_operands_take_the_elementwise_form(M, dtype):
    """D = 512 on operands offset by 2 elements: ln_epl's 16-byte alignment test fails, epl = 0 (the element-wise kernels)"""
    D = 512
    base = rnd(M * D + 2, dtype=dtype, seed=7, scale=2.0) + 0.5
    x = base[2:].view(M, D)
    gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dyb = rnd(M * D + 2, dtype=dtype, seed=8)
    assert x.data_ptr() % 16 != 0
    ln_check(x, gamma, beta, dyb[2:].view(M, D), None, None, "LN unaligned M=%d" % M)


@pytest.mark.parametrize("M", [1, 7, 2560, 3000, 8191])
def test_layernorm_bwd_small_kernel_both_settings(M):
    """ln_small 1 / 0 (bf16, D = 512, M < 8,192: ln_bwd_small_kernel vs ln_bwd_kernel): both within the fp64 bound, and within bf16
    rounding of each other (include/s2t_hip.h): one bf16 ulp plus twice the f32 evaluation bound of the element (the two kernels'
    f32 codegen differs, and where the row's terms cancel that error is larger than a ulp of the result: not bit for bit)"""
    D = 512
    x = rnd(M, D, dtype=BF, seed=M, scale=2.0) + 0.5
    gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dy = rnd(M, D, dtype=BF, seed=4)
    dres = rnd(M, D, dtype=BF, seed=5)
    outs = {}
    for s in (1, 0):
        with set_option("ln_small", s):
            outs[s] = ln_check(x, gamma, beta, dy, dres, (0.1, 5), "LN ln_small=%d M=%d" % (s, M))
    a, b = d64(outs[0][0]), d64(outs[1][0])
    big = torch.maximum(a.abs(), b.abs())
    ulp = torch.where(big == 0, torch.full_like(big, 2.0 ** -133), 2.0 ** (torch.floor(torch.log2(big.clamp_min(2.0 ** -126))) - 7))
    assert_close(outs[1][0], a, ulp + 2 * outs[0][1], "ln_small 1 vs 0")


def test_layernorm_bwd_small_kernel_both_settings_seed_above_32_bits():
    """the second output's keep pattern under both settings at a seed whose upper word is set (M = 7: the smallest M above with
    more than one row)"""
    M, D = 7, 512
    x = rnd(M, D, dtype=BF, seed=M, scale=2.0) + 0.5
    gamma, beta = 1 + 0.1 * rnd(D, seed=2), 0.1 * rnd(D, seed=3)
    dy, dres = rnd(M, D, dtype=BF, seed=4), rnd(M, D, dtype=BF, seed=5)
    for s in (1, 0):
        with set_option("ln_small", s):
            ln_check(x, gamma, beta, dy, dres, (0.1, (5 << 32) | 7), "LN ln_small=%d M=%d, 64-bit seed" % (s, M))


# ------------------------------------------------------------------ attention
def attn_check(dtype, H, B, Tq, Tk, klen, causal, what):
    """O = softmax(scale q k^T) V per head, and its backward, against float64.
    Forward: the scores are f32 sums of d = 64 bf16 / f32 products: |ds| <= 2 d u scale (|q| |k|^T) <= e_s (the row maximum); softmax
    with the row max subtracted and f32 exp keeps p to (2 e_s + Tk u) relative, and the bf16 kernels round P to bf16 for the P V
    MFMA (r_p = 2^-8, f32: u): |dO| <= 2 (2 e_s + r_p + (Tk + d) u) (P |V|) + r |O|.
    Backward: dV = P^T dO: 2 (2 e_s + r_p + Tq u) (P^T |dO|) + r |dV|.  dP = dO V^T to 2 d u (|dO| |V|^T) = e_p; Delta = rowsum(dO O)
    to (d u + r) sum|dO O| = e_D (O is the bf16 output passed in); dS = P (dP - Delta) to
    |dS| (2 e_s + r_p) + P (e_p + e_D) + r_p |dS| (the bf16 kernels round dS for its MFMAs) = E; dQ = scale dS K: scale (E |K| +
    (Tk u + r_p) |dS| |K|) + r |dQ|; dK = scale dS^T Q likewise.  Factor 2 of slack on the sums."""
    d = 64
    D = H * d
    scale = d ** -0.5
    g = torch.Generator().manual_seed(Tq * 7 + Tk)
    qkv = (torch.randn(max(Tq, Tk), B, 3 * D, generator=g) * 0.7).to(dtype).to(DEV)
    q, k, v = qkv[:Tq, :, :D], qkv[:Tk, :, D:2 * D], qkv[:Tk, :, 2 * D:]
    do = torch.randn(Tq, B, D, generator=g).to(dtype).to(DEV)
    kl = klen.to(DEV) if klen is not None else None
    with launches() as c:
        o, lse = K.attn_fwd(q, k, v, H, klen=kl, causal=causal)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        K.attn_bwd(q, k, v, o, do, lse, H, dq, dk, dv, klen=kl, causal=causal)
    assert c["attn_fwd"] == 1 and c["attn_bwd"] == 1, c
    dev = ref_dev(4 * 7 * B * H * Tq * Tk * d)
    r = r_of(dtype)
    rp = UBF if dtype == BF else U32

    def heads(t, T):
        return d64(t, dev).reshape(T, B, H, d).permute(1, 2, 0, 3)       # [B, H, T, d]
    Q, Kh, V, dO, O = heads(q, Tq), heads(k, Tk), heads(v, Tk), heads(do, Tq), heads(o, Tq)
    s = scale * Q @ Kh.transpose(-1, -2)
    mask = torch.zeros(Tq, Tk, dtype=torch.bool, device=dev)
    if causal:
        mask = mask | torch.triu(torch.ones(Tq, Tk, dtype=torch.bool, device=dev), 1)
    mask = mask[None, None].expand(B, H, Tq, Tk)
    if klen is not None:
        mask = mask | (torch.arange(Tk, device=dev)[None, :] >= klen.to(dev)[:, None])[:, None, None, :]
    s = s.masked_fill(mask, -math.inf)
    P = torch.softmax(s, -1)
    es = 2 * d * U32 * scale * (Q.abs() @ Kh.abs().transpose(-1, -2)).masked_fill(mask, 0).amax(-1, keepdim=True)
    Oref = P @ V
    bO = 2 * (2 * es + rp + (Tk + d) * U32) * (P @ V.abs()) + r * Oref.abs()
    assert_close(o.reshape(Tq, B, H, d).permute(1, 2, 0, 3), Oref, bO, what + " O")
    # backward from the kernel's O (the input the backward is defined on)
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
    perm = lambda t, T: t.reshape(T, B, H, d).permute(1, 2, 0, 3)  # noqa: E731
    assert_close(perm(dv, Tk), dVr, bV, what + " dV")
    assert_close(perm(dk, Tk), dKr, bK, what + " dK")
    assert_close(perm(dq, Tq), dQr, bQ, what + " dQ")
    ctx = dict(P=P, es=es, dev=dev, d=d, B=B, H=H, Tq=Tq, Tk=Tk, r=r, rp=rp)
    return q, k, v, do, kl, ctx


def attn_dropout_adjoint(q, k, v, do, kl, causal, ctx, what):
    """With dropout, O is linear in V for a fixed mask M: O(V2) = Pd V2 with Pd = P M / (1 - p), and the backward's dV = Pd^T dO, so
    for every head and every column c:  <dO[:, c], O(V2)[:, c]> = <dV[:, c], V2[:, c]>  -- if forward and backward drop the same pairs.
    Tolerance, per (head, column): a worst-case bound (sum of |terms|) would grow like the number of terms while the identity and a
    mask mismatch grow like its square root, so the rounding is estimated statistically instead.  Each Pd entry the kernels use
    carries a relative error of at most eps_i = 2 e_s + r_p (scores, exp, the bf16 rounding of P: attn_check), independent from entry
    to entry; each output element one more rounding r' = r + 4 (T + d) u (output dtype, the row normalisation).  With the unknown mask
    E[Pd^2] = P^2 / (1 - p), so
        var O2[i, c] = eps_i^2 sum_j P_ij^2 / (1-p) V2[j, c]^2 + (r' O2[i, c])^2,
        var dV[j, c] = sum_i eps_i^2 P_ij^2 / (1-p) dO[i, c]^2 + (r' dV[j, c])^2,
        sd^2 = sum_i dO[i, c]^2 var O2[i, c] + sum_j V2[j, c]^2 var dV[j, c]   (each error is dotted with an operand it does not
    depend on), and z = (lhs - rhs) / sd must stay within 6 for every (head, column).
    Power: a backward with another mask changes dV[j, c] by sum_i (+-P_ij / (1-p)) dO[i, c] on the flipped pairs, variance
    2 p / (1-p) sum_i P_ij^2 dO[i, c]^2, about (sqrt(p) / eps)^2 ~ (0.55 / 2^-8)^2 times the rounding variance: z of order 10^2.  The
    test asserts that a backward with the mask of another seed gives an RMS z above 6, i.e. that this check sees a mask mismatch."""
    p, seed = 0.3, 77
    H, d, B, Tq, Tk, dev = ctx["H"], ctx["d"], ctx["B"], ctx["Tq"], ctx["Tk"], ctx["dev"]
    g = torch.Generator().manual_seed(seed)
    v2 = (torch.randn(v.shape, generator=g) * 0.7).to(v.dtype).to(DEV)
    o1, lse = K.attn_fwd(q, k, v, H, klen=kl, causal=causal, p_drop=p, seed=seed)
    o2, _ = K.attn_fwd(q, k, v2, H, klen=kl, causal=causal, p_drop=p, seed=seed)

    def dv_of(bseed):
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        K.attn_bwd(q, k, v, o1, do, lse, H, dq, dk, dv, klen=kl, causal=causal, p_drop=p, seed=bseed)
        return dv

    def heads(t, T):
        return d64(t, dev).reshape(T, B, H, d).permute(1, 2, 0, 3)          # [B, H, T, d]
    dO, O2, V2 = heads(do, Tq), heads(o2, Tq), heads(v2, Tk)
    P2e = ctx["P"] ** 2 / (1 - p) * (2 * ctx["es"] + ctx["rp"]) ** 2           # [B, H, Tq, Tk]
    rO, rV = ctx["r"] + 4 * (Tk + d) * U32, ctx["r"] + 4 * (Tq + d) * U32
    lhs = (dO * O2).sum(-2)                                                    # [B, H, d]
    varO = P2e @ (V2 * V2) + (rO * O2) ** 2

    def z_of(dV):
        varV = P2e.transpose(-1, -2) @ (dO * dO) + (rV * dV) ** 2
        sd = ((dO * dO * varO).sum(-2) + (V2 * V2 * varV).sum(-2)).sqrt()
        return (lhs - (dV * V2).sum(-2)) / sd
    z = z_of(heads(dv_of(seed), Tk))
    i = int(z.abs().reshape(-1).argmax())
    assert float(z.abs().max()) <= 6, "%s: <dO, O(V2)> != <dV, V2> for (b, h, c) %s: z = %.3g" % (
        what, tuple(int(x) for x in torch.unravel_index(torch.tensor(i), z.shape)), float(z.reshape(-1)[i]))
    zw = z_of(heads(dv_of(seed + 1), Tk))
    rms = float((zw * zw).mean().sqrt())
    assert rms > 6, "%s: a backward with another dropout mask passes the check (rms z %.3g)" % (what, rms)


ATTN_CASES = [
    # dtype, H, B, Tq, Tk, ragged, causal
    (BF, 2, 3, 15, 200, True, False), (BF, 2, 3, 16, 200, True, False), (BF, 2, 3, 17, 200, False, False),
    (BF, 2, 3, 130, 130, True, True), (BF, 8, 16, 375, 375, True, False), (BF, 16, 6, 375, 375, False, False),
    (F32, 2, 3, 16, 200, True, False), (F32, 4, 2, 130, 257, True, True),
]


@pytest.mark.parametrize("v1", [0, 1])
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "%s_H%d_B%d_Tq%d_Tk%d%s%s" % (
    "bf16" if c[0] == BF else "f32", c[1], c[2], c[3], c[4], "_ragged" if c[5] else "", "_causal" if c[6] else ""))
def test_attention_routes(case, v1):
    """attn_v1 0 / 1 at Tq around attn_v2_min_tq (16): attention.hip's forward takes attn_fwd2_kernel when bf16, d = 64 and
    (Tq >= 128 || (Tq >= attn_v2_min_tq && Tk >= 128)) and attn_v1 == 0; the backward's dq2 / dkv2 kernels follow the same
    rule (bwd_launch); f32 always runs the first generation.  H 8 at B 16 (m preset) and H 16 (l preset) fill the grid."""
    dt, H, B, Tq, Tk, ragged, causal = case
    klen = torch.tensor([Tk - 3 * i if i % 2 else max(1, Tk - 37 * i) for i in range(B)], dtype=torch.int32) if ragged else None
    with set_option("attn_v1", v1):
        q, k, v, do, kl, ctx = attn_check(dt, H, B, Tq, Tk, klen, causal, "attn v1=%d" % v1)
        attn_dropout_adjoint(q, k, v, do, kl, causal, ctx, "attn v1=%d" % v1)


def test_attention_v2_min_tq_raised():
    """attn_v2_min_tq = 128: a Tq = 100, Tk = 300 block leaves the second-generation kernels (Tq >= attn_v2_min_tq fails); both
    settings against fp64"""
    klen = torch.tensor([300, 211, 1], dtype=torch.int32)
    for val in (16, 128):
        with set_option("attn_v2_min_tq", val):
            q, k, v, do, kl, ctx = attn_check(BF, 2, 3, 100, 300, klen, False, "attn_v2_min_tq=%d" % val)
            attn_dropout_adjoint(q, k, v, do, kl, False, ctx, "attn_v2_min_tq=%d" % val)


@pytest.mark.parametrize("Tq", [127, 128])
@pytest.mark.parametrize("Tk", [127, 128, 384, 385])
def test_attention_bwd_two_kernel_around_128_and_384_against_fp64(Tq, Tk):
    """the default backward (bwd_launch) for bf16, d = 64, no causal mask at Tq / Tk = 127 / 128, where the second-generation dq2 /
    dkv2 kernels' Tq >= 128 and Tk >= 128 gates flip, and at Tk = 384 / 385 around the encoder's 375 keys.  Every case against
    fp64, ragged keys, and the dropout adjoint identity"""
    B, H = 3, 8
    klen = torch.tensor([Tk, Tk - 5, max(1, Tk // 3)], dtype=torch.int32)
    q, k, v, do, kl, ctx = attn_check(BF, H, B, Tq, Tk, klen, False, "bwd Tq=%d Tk=%d" % (Tq, Tk))
    attn_dropout_adjoint(q, k, v, do, kl, False, ctx, "bwd Tq=%d Tk=%d" % (Tq, Tk))
