"""s2t_gemm_gather with row maps (mapA / periodA, mapB, mapC) element by element against float64, on every loader and tile form.

The implicit-GEMM convolutions (engine.py subsample_fwd / subsample_bwd, attn2d_block_fwd / _bwd) run on this route; the maps'
meaning is tied to a real convolution by tests/test_conv_maps_cpu.py, this file ties the kernels to the maps.  Conventions of
tests/test_routes_gpu.py: float64 references from the exact values the kernel received, every output element compared, every bound
derived, the route proven by a launch count or a cited dispatch condition, a failure names the worst element.

Reference (csrc/gemm_epilogue.hpp:12-14), built on the CPU by `gather_a64` / `gather_b64`:
    A(r, k) = Asrc[mapA[(k / period) * M + r]][k % period],   B(k, :) = Bsrc[mapB[k]],   -1 -> zeros,   C row mapC[r] <- row r.
Bound (class `Ref`, the `Gemm` bound of test_routes_gpu.py on the gathered operands; gathering moves values and rounds nothing):
    |acc - ref| <= 4 K u (|A| |B|)_ij, u = 2^-24: K products exact (bf16) or rounded once (f32) in f32, summed in some order
    ((K - 1) u sum|terms|), plus the few roundings of alpha, the bias and the partial sums of k-tiles / k-slices (factor 4);
    + r |v| for every rounding of a value v to the output dtype (r = 2^-8 bf16, 2^-24 f32): once for the activated value, once more
      for a residual or an accumulate;  x 1 / (1 - p) under dropout;
    split-K (f32 output, gemm_epilogue.hpp:145-153): each of the s slices leaves by one f32 atomic add onto the running value, whose
      magnitude is at most |old| + (|A| |B|)_ij (1 + K u): + s u (|old| + (|A| |B|)_ij).
Maps: random int32 in [-1, rows) with duplicates, one all -1 product row, one all -1 tap (mapA) or one all -1 k-quad run (mapB); the
sources have more rows than M (K), so an index error lands on another row's values and not on zeros.
Witness: gemm.hip gemm_run opens ProfScope "gemm_gather" for every product with mapA or mapB and the ordinary family otherwise
(mapC alone).  Tile form: gemm.hip:845 -- `f32in = in_dtype == S2T_F32 && !mapA && !mapB && !mapC`, so a mapped product NEVER uses the
f32 thresholds: small = t128 < gemm_small_nt (NT) / gemm_small_kt (NN, TN) for f32 and bf16 alike.  With the threshold at 0 the product
takes the 128-wide forms (128 x 64 when N <= 64, `narrow`, else 128 x 128); at its default (192 / 40 tiles) these tiny products
(t128 <= 12) take the 64 x 64 form.  The forms report as one family, so this rule is the witness of the form.
Loaders (gemm.hip StageDirect::load / StageTrans::load): branch-free when `map && vec && k0 + BK <= K` (and ncols % E == 0 for the
transposed stage), guarded otherwise; BK = 64 (bf16) / 32 (f32), vec = 16-byte aligned base and row stride.
"""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
U32 = 2.0 ** -24
UBF = 2.0 ** -8
BF, F32 = torch.bfloat16, torch.float32
FAMILIES = ("gemm_nt", "gemm_nt_small", "gemm_nn", "gemm_nn_small", "gemm_tn", "gemm_tn_small", "gemm256_nt", "gemm256_nn",
            "gemm_gather", "wgrad_group", "wgrad_group_f32", "attn_fwd", "attn_bwd")
DT3 = [(F32, F32), (BF, BF), (BF, F32)]
DT3_IDS = ["f32", "bf16", "bf16_f32out"]
SENT = 7.0                         # sentinel of rows / columns no store may touch (exact in bf16)


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    K.prof_enable(0)


# ------------------------------------------------------------------ shared tools (as in tests/test_routes_gpu.py)
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


def only(counts, fam, n):
    """the GEMM launches of a block were exactly n, all of family `fam`"""
    ran = {f: c for f, c in counts.items() if c and f.startswith("gemm")}
    assert ran == {fam: n}, "expected %d %s launches and nothing else, saw %s" % (n, fam, ran)


def form(key, wide):
    """threshold 0: the 128-wide forms; default: the 64 x 64 form (module docstring, gemm.hip:845-850)"""
    return set_option(key, 0) if wide else contextlib.nullcontext()


def rnd(*shape, dtype=F32, seed=0, scale=1.0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def d64(t):
    return t.detach().cpu().double()


def r_of(dtype):
    return UBF if dtype == BF else U32


def assert_close(out, ref, bound, what):
    """|out - ref| <= bound element by element (ref, bound float64 on the CPU); on failure: the worst element, its value, ref and bound"""
    o = d64(out)
    assert o.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(o.shape), tuple(ref.shape))
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


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------ operands, maps and the float64 reference (all of it runs on the CPU)
def make_src(rows, cols, dtype, kind, seed, dev=DEV):
    """[rows, cols] source matrix.  plain: contiguous, 16-byte aligned.  stride: a view whose row stride (cols + 1 elements) is no
    multiple of 16 bytes.  offset: contiguous rows behind a base pointer one element past an aligned address.  The last two make
    `vec` false: every tile of that operand goes through the guarded loader."""
    if kind == "plain":
        return rnd(rows, cols, dtype=dtype, seed=seed, dev=dev)
    if kind == "stride":
        t = rnd(rows, cols + 1, dtype=dtype, seed=seed, dev=dev)[:, :cols]
        assert (t.stride(0) * t.element_size()) % 16 != 0
        return t
    assert kind == "offset"
    t = rnd(rows * cols + 1, dtype=dtype, seed=seed, dev=dev)[1:].view(rows, cols)
    assert t.data_ptr() % 16 != 0
    return t


def make_map_a(taps, M, rows, seed):
    """[taps, M] int32 in [-1, rows): duplicates come with the draw; product row M // 2 is -1 in every tap (M > 1), tap taps // 2 is
    all -1 (taps > 1)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-1, rows, (taps, M), generator=g, dtype=torch.int32)
    if M > 1:
        m[:, M // 2] = -1
    if taps > 1:
        m[taps // 2, :] = -1
    return m


def make_map_b(K_, rows, seed):
    """[K] int32 in [-1, rows); eight consecutive k from K // 2 on are -1 (whole k-quads of zeros)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(-1, rows, (K_,), generator=g, dtype=torch.int32)
    m[K_ // 2:K_ // 2 + 8] = -1
    return m


def make_perm(M, out_rows, seed):
    """mapC: M distinct rows of out_rows > M (a permutation's first M entries), and the mask of the rows it leaves alone"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(out_rows, generator=g)[:M].to(torch.int32)
    untouched = torch.ones(out_rows, dtype=torch.bool)
    untouched[perm.long()] = False
    return perm, untouched


def gather_a64(src, maps, period, K_):
    """float64 [M, K]: A(r, k) = src[maps[k / period][r]][k % period], -1 -> zeros (gemm_epilogue.hpp:12)"""
    taps, M = maps.shape
    s = d64(src)
    assert s.shape[1] == period and (taps - 1) * period < K_ <= taps * period
    idx = maps.long()
    rows = s[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1)
    return rows.permute(1, 0, 2).reshape(M, taps * period)[:, :K_]


def gather_b64(src, map_b):
    """float64 [K, N]: B(k, :) = src[map_b[k]], -1 -> zeros (gemm_epilogue.hpp:13)"""
    idx = map_b.long()
    return d64(src)[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1)


class Ref:
    """float64 C = alpha A B (+ bias) of explicit operands A [M, K], B [K, N] and the accumulation bound of the module docstring"""

    def __init__(self, A, B, alpha=1.0, bias=None):
        self.K_ = A.shape[1]
        self.absab = A.abs() @ B.abs()
        self.acc = alpha * (A @ B)
        self.accb = 4 * self.K_ * U32 * abs(alpha) * self.absab
        if bias is not None:
            self.acc = self.acc + d64(bias)
            self.accb = self.accb + U32 * self.acc.abs()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def taps_of(K_, period):
    return (K_ + period - 1) // period


# ------------------------------------------------------------------ NT + mapA (convolution forward, engine.py:365, 503, 518, 548, 575)
# k-tiles (BK = 64 bf16 / 32 f32): K = 192, 576, 256 whole tiles only (branch-free loader alone); K = 144, 216 whole tiles and a ragged
# last one (both loaders in one product); K = 24, 40 (bf16) shorter than a tile (guarded alone).  Period 24: tap boundaries at 24,
# 48, 72, ... inside the k-tiles; period 128: the tiles at k = 64, 192 (and 32, 96, ... for f32) start inside a tap; K = 192 over
# period 128 and K = 40 over period 16 end inside a tap.  src kinds `stride` / `offset`: guarded loader for every tile.
NT_CASES = [
    # period, K, M, N, wide, src kind
    (16, 144, 65, 64, False, "plain"),
    (24, 144, 130, 72, False, "plain"),
    (8, 144, 63, 8, False, "plain"),
    (24, 192, 257, 16, True, "plain"),          # 128 x 64
    (64, 192, 64, 200, True, "plain"),          # 128 x 128
    (64, 576, 130, 64, True, "plain"),          # 128 x 64
    (24, 216, 257, 200, False, "plain"),
    (128, 256, 65, 72, True, "plain"),          # 128 x 128
    (128, 192, 130, 16, False, "plain"),        # K not a multiple of the period
    (16, 40, 1, 8, False, "plain"),             # K not a multiple of the period, one row
    (24, 24, 1, 16, True, "plain"),             # shorter than one k-tile
    (16, 144, 65, 64, False, "stride"),
    (64, 192, 130, 72, True, "offset"),
    (24, 216, 64, 8, True, "stride"),
]


@pytest.mark.parametrize("idt,odt", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("case", NT_CASES, ids=["p%d_k%d_m%d_n%d_%s_%s" % (c[0], c[1], c[2], c[3], "w128" if c[4] else "w64", c[5]) for c in NT_CASES])
def test_nt_map_a(case, idt, odt):
    """C = gather(src, mapA) W^T, plain and with bias + ReLU (the conv forward's epilogue): bound accb + r |v| (one output rounding);
    two products, two gemm_gather launches"""
    period, K_, M, N, wide, kind = case
    taps, rows = taps_of(K_, period), M + 9
    src = make_src(rows, period, idt, kind, seed=1)
    w = rnd(N, K_, dtype=idt, seed=2, scale=K_ ** -0.5)
    maps = make_map_a(taps, M, rows, seed=3)
    bias = rnd(N, seed=4, scale=0.5)
    A, B = gather_a64(src, maps, period, K_), d64(w).t()
    g, gb = Ref(A, B), Ref(A, B, bias=bias)
    r = r_of(odt)
    md = maps.to(DEV)
    with form("gemm_small_nt", wide), launches() as c:
        out = K.gemm(src, w, M=M, K=K_, map_a=md, period_a=period, out_dtype=odt)
        out2 = K.gemm(src, w, M=M, K=K_, map_a=md, period_a=period, bias=bias, act=K.ACT_RELU, out_dtype=odt)
    only(c, "gemm_gather", 2)
    assert_close(out, g.acc, g.accb + r * g.acc.abs(), "nt mapA")
    assert M == 1 or bool((out[M // 2] == 0).all()), "the all -1 product row is not zero"
    ref = gb.acc.clamp_min(0)
    assert_close(out2, ref, gb.accb + r * ref.abs(), "nt mapA bias+relu")


# ------------------------------------------------------------------ NN + mapA (convolution data gradient, engine.py:463)
# B is [K][N] (StageTrans) without a map; bf16 N = 12 is no multiple of 8: vecB is false and B takes StageTrans' guarded branch beside
# the gathered A
NN_CASES = [
    # period, K, M, N, wide, bf16 only
    (8, 72, 65, 64, False, False),
    (16, 144, 130, 72, True, False),
    (24, 96, 65, 72, False, False),
    (24, 216, 130, 64, False, False),
    (64, 128, 130, 64, True, False),
    (128, 256, 65, 72, True, False),
    (16, 144, 65, 12, False, True),
    (64, 192, 130, 12, True, True),
]
NN_PARAMS = [(c, dt) for c in NN_CASES for dt in DT3 if not (c[5] and dt[0] != BF)]


def _dt_id(dt):
    return DT3_IDS[DT3.index(dt)]


@pytest.mark.parametrize("case,dt", NN_PARAMS,
                         ids=["p%d_k%d_m%d_n%d_%s-%s" % (c[0], c[1], c[2], c[3], "w128" if c[4] else "w64", _dt_id(dt)) for c, dt in NN_PARAMS])
def test_nn_map_a(case, dt):
    """C = gather(src, mapA) B, plain and with a residual (engine.py:575's epilogue): accb + r |acc| and accb + r (|acc| + |ref|)"""
    period, K_, M, N, wide, _ = case
    idt, odt = dt
    taps, rows = taps_of(K_, period), M + 9
    src = make_src(rows, period, idt, "plain", seed=5)
    b = rnd(K_, N, dtype=idt, seed=6, scale=K_ ** -0.5)
    maps = make_map_a(taps, M, rows, seed=7)
    res = rnd(M, N, dtype=odt, seed=8)
    g = Ref(gather_a64(src, maps, period, K_), d64(b))
    r = r_of(odt)
    md = maps.to(DEV)
    with form("gemm_small_kt", wide), launches() as c:
        out = K.gemm(src, b, trans_b=True, M=M, K=K_, map_a=md, period_a=period, out_dtype=odt)
        out2 = K.gemm(src, b, trans_b=True, M=M, K=K_, map_a=md, period_a=period, residual=res, out_dtype=odt)
    only(c, "gemm_gather", 2)
    assert_close(out, g.acc, g.accb + r * g.acc.abs(), "nn mapA")
    ref = g.acc + d64(res)
    assert_close(out2, ref, g.accb + r * (g.acc.abs() + ref.abs()), "nn mapA residual")


# ------------------------------------------------------------------ TN + mapB (weight gradient per tap, engine.py:447, 544, 571)
# K = pixels.  K = 64, 256: whole k-tiles; K = 50, 1000: ragged tails (bf16: 50 is shorter than a tile).  bf16 N = 12: ncols % 8 != 0 and
# vecB false: guarded; N = 72: branch-free with column groups at gc >= 72 zeroed by the select; f32 N = 12: branch-free (12 % 4 == 0).
# split-K: nk = ceil(K / BK) k-tiles are dealt `per = ceil(nk / s)` to a slice; K = 50, 64 have nk = 1 (bf16) or 2 (f32), so s = 3, 4
# leave slices empty (gemm_kernel: `if (kt0 >= kt1) return`).
TN_CASES = [
    # K, M, N, wide
    (50, 12, 12, False),
    (64, 72, 64, False),
    (256, 130, 72, True),           # 128 x 128
    (1000, 64, 130, True),          # 128 x 128
    (256, 64, 12, True),            # 128 x 64
    (1000, 130, 64, False),
]


@pytest.mark.parametrize("idt,odt", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("case", TN_CASES, ids=["k%d_m%d_n%d_%s" % (c[0], c[1], c[2], "w128" if c[3] else "w64") for c in TN_CASES])
def test_tn_map_b(case, idt, odt):
    """C[:, slice] += dY^T gather(src, mapB) into a column slice of a wider, non-zero buffer (engine.py:447), split-K 1, 3, 4 for an f32
    output (a bf16 output takes no split-K: gemm.hip:809).  s = 1: accb + r (|acc| + |ref|) (accumulate: round, add the old value,
    round again); s > 1: accb + s u (|old| + |A| |B|) (module docstring).  The columns outside the slice keep their bits."""
    K_, M, N, wide = case
    rows = K_ + 9
    a = rnd(K_, M, dtype=idt, seed=9)
    src = rnd(rows, N, dtype=idt, seed=10, scale=K_ ** -0.5)
    mb = make_map_b(K_, rows, seed=11)
    g = Ref(d64(a).t(), gather_b64(src, mb))
    r = r_of(odt)
    md = mb.to(DEV)
    splits = (1, 3, 4) if odt == F32 else (1,)
    c0 = 16
    outs = []
    with form("gemm_small_kt", wide), launches() as c:
        for s in splits:
            base = rnd(M, c0 + N + 8, dtype=odt, seed=12 + s)
            buf = base.clone()
            K.gemm(a, src, trans_a=True, trans_b=True, K=K_, map_b=md, out=buf[:, c0:c0 + N], accumulate=True, splitk=s)
            outs.append((s, base, buf))
    only(c, "gemm_gather", len(splits))
    for s, base, buf in outs:
        old = d64(base[:, c0:c0 + N])
        ref = g.acc + old
        bound = g.accb + (r * (g.acc.abs() + ref.abs()) if s == 1 else s * U32 * (old.abs() + g.absab))
        assert_close(buf[:, c0:c0 + N], ref, bound, "tn mapB splitk=%d" % s)
        assert same_bits(buf[:, :c0], base[:, :c0]) and same_bits(buf[:, c0 + N:], base[:, c0 + N:]), \
            "splitk=%d: a store landed outside the column slice" % s


# ------------------------------------------------------------------ scatter (mapC) beside a gather
def sentinel_out(out_rows, N, odt, perm=None, base=None):
    out = torch.full((out_rows, N), SENT, dtype=odt, device=DEV)
    if base is not None:
        out[perm.long().to(DEV)] = base
    return out


def check_untouched(out, untouched, what):
    rest = out[untouched.to(DEV)]
    assert same_bits(rest, torch.full_like(rest, SENT)), what + ": a row outside mapC was written"


def drop_reference(M, N, K_, period, idt, odt, p):
    """operands, float64 reference and bound of the dropout case; everything but `src` / `b` / `maps` stays on the CPU, and the share of
    elements too small to tell a kept value from a dropped one comes from the reference alone"""
    taps, rows = taps_of(K_, period), M + 9
    src = make_src(rows, period, idt, "plain", seed=21, dev="cpu")
    b = rnd(K_, N, dtype=idt, seed=22, scale=K_ ** -0.5, dev="cpu")
    maps = make_map_a(taps, M, rows, seed=23)
    g = Ref(gather_a64(src, maps, period, K_), d64(b))
    bound = (g.accb + r_of(odt) * g.acc.abs()) / (1 - p)
    sure = (g.acc.abs() / (1 - p)) > 2 * bound           # a kept value cannot round to zero
    return src, b, maps, g, bound, sure


DROP_CASES = [(257, 64, 144, 16, False), (257, 10, 144, 16, True), (257, 64, 128, 64, True), (257, 10, 96, 24, False)]


@pytest.mark.parametrize("idt,odt", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("M,N,K_,period,wide", DROP_CASES, ids=["m%d_n%d_k%d_p%d_%s" % (c[0], c[1], c[2], c[3], "w128" if c[4] else "w64") for c in DROP_CASES])
def test_scatter_map_a_nn_dropout(M, N, K_, period, wide, idt, odt):
    """engine.py:463: NN + mapA + mapC + dropout.  N = 64: one hash per element quad; N = 10: N % 4 != 0, the per-element hash
    (gemm_epilogue.hpp:76-95).  C and the mask follow mapC[r]: the keep pattern equals K.dropout(ones(out_rows, N), p, seed)[mapC].
    Bound (accb + r |acc|) / (1 - p).  The pattern is compared where |acc| / (1 - p) > 2 bound; the rest (the all -1 product row, 1 / 257,
    and values that cancel to ~0) must be under 1 % of the elements -- checked here from the float64 reference before the kernel's
    output is looked at."""
    p, seed = 0.25, 1234
    src, b, maps, g, bound, sure = drop_reference(M, N, K_, period, idt, odt, p)
    share = 1.0 - float(sure.double().mean())
    assert share <= 0.01, "%.3f %% of the elements cannot witness the keep pattern" % (100 * share)
    out_rows = M + 11
    perm, untouched = make_perm(M, out_rows, seed=24)
    out = sentinel_out(out_rows, N, odt)
    with form("gemm_small_kt", wide), launches() as c:
        K.gemm(src.to(DEV), b.to(DEV), trans_b=True, M=M, K=K_, map_a=maps.to(DEV), period_a=period, map_c=perm.to(DEV), out=out,
               p_drop=p, seed=seed)
    only(c, "gemm_gather", 1)
    keep = (K.dropout(torch.ones(out_rows, N, dtype=odt, device=DEV), p, seed) != 0).cpu()[perm.long()]
    got = out[perm.long().to(DEV)]
    ref = torch.where(keep, g.acc / (1 - p), torch.zeros_like(g.acc))
    assert_close(got, ref, bound, "scatter nn mapA dropout")
    assert torch.equal((got.cpu() != 0) & sure, keep & sure), "the dropout mask does not follow the scattered row mapC[r]"
    check_untouched(out, untouched, "dropout")


@pytest.mark.parametrize("idt,odt", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("wide", [False, True], ids=["w64", "w128"])
def test_scatter_map_a_epilogues(wide, idt, odt):
    """mapC beside mapA with accumulate, bias + ReLU (NT), and residual, ACT_RELU_BWD with aux, GELU with aux_out (NN).  Index spaces
    (gemm_epilogue.hpp:42-115): C (and the old value of an accumulate) at mapC[r]; residual, aux and aux_out at the product row r.
    Bounds: accb + r |v| per output rounding, one more for residual / accumulate; GELU 1.13 accb + 2^-20 |pre| + r |gelu|."""
    M, N, K_, period = 130, 72, 216, 24
    taps, rows, out_rows = taps_of(K_, period), M + 9, M + 11
    r = r_of(odt)
    src = make_src(rows, period, idt, "plain", seed=31)
    maps = make_map_a(taps, M, rows, seed=32)
    md = maps.to(DEV)
    perm, untouched = make_perm(M, out_rows, seed=33)
    pd, pl = perm.to(DEV), perm.long().to(DEV)
    A = gather_a64(src, maps, period, K_)
    # NT
    w = rnd(N, K_, dtype=idt, seed=34, scale=K_ ** -0.5)
    bias = rnd(N, seed=35, scale=0.5)
    base = rnd(M, N, dtype=odt, seed=36)
    g, gb = Ref(A, d64(w).t()), Ref(A, d64(w).t(), bias=bias)
    with form("gemm_small_nt", wide), launches() as c:
        o_acc = sentinel_out(out_rows, N, odt, perm, base)
        K.gemm(src, w, M=M, K=K_, map_a=md, period_a=period, map_c=pd, out=o_acc, accumulate=True)
        o_relu = sentinel_out(out_rows, N, odt)
        K.gemm(src, w, M=M, K=K_, map_a=md, period_a=period, map_c=pd, out=o_relu, bias=bias, act=K.ACT_RELU)
    only(c, "gemm_gather", 2)
    ref = g.acc + d64(base)
    assert_close(o_acc[pl], ref, g.accb + r * (g.acc.abs() + ref.abs()), "scatter nt accumulate")
    check_untouched(o_acc, untouched, "accumulate")
    ref = gb.acc.clamp_min(0)
    assert_close(o_relu[pl], ref, gb.accb + r * ref.abs(), "scatter nt bias+relu")
    check_untouched(o_relu, untouched, "bias+relu")
    # NN
    b = rnd(K_, N, dtype=idt, seed=37, scale=K_ ** -0.5)
    res = rnd(M, N, dtype=odt, seed=38)
    aux = rnd(M, N, dtype=odt, seed=39)
    g = Ref(A, d64(b))
    pre = torch.full((M, N), SENT, dtype=odt, device=DEV)
    with form("gemm_small_kt", wide), launches() as c:
        o_res = sentinel_out(out_rows, N, odt)
        K.gemm(src, b, trans_b=True, M=M, K=K_, map_a=md, period_a=period, map_c=pd, out=o_res, residual=res)
        o_bwd = sentinel_out(out_rows, N, odt)
        K.gemm(src, b, trans_b=True, M=M, K=K_, map_a=md, period_a=period, map_c=pd, out=o_bwd, act=K.ACT_RELU_BWD, aux=aux)
        o_gelu = sentinel_out(out_rows, N, odt)
        K.gemm(src, b, trans_b=True, M=M, K=K_, map_a=md, period_a=period, map_c=pd, out=o_gelu, act=K.ACT_GELU, aux_out=pre)
    only(c, "gemm_gather", 3)
    ref = g.acc + d64(res)
    assert_close(o_res[pl], ref, g.accb + r * (g.acc.abs() + ref.abs()), "scatter nn residual (residual at the product row)")
    ref = torch.where(d64(aux) > 0, g.acc, torch.zeros_like(g.acc))
    assert_close(o_bwd[pl], ref, g.accb + r * ref.abs(), "scatter nn relu_bwd (aux at the product row)")
    assert_close(pre, g.acc, g.accb + r * g.acc.abs(), "scatter nn gelu aux_out (at the product row)")
    ref = gelu64(g.acc)
    assert_close(o_gelu[pl], ref, 1.13 * g.accb + 2.0 ** -20 * g.acc.abs() + r * ref.abs(), "scatter nn gelu")
    for o, what in ((o_res, "residual"), (o_bwd, "relu_bwd"), (o_gelu, "gelu")):
        check_untouched(o, untouched, what)


@pytest.mark.parametrize("idt", [F32, BF], ids=["f32", "bf16_f32out"])
@pytest.mark.parametrize("wide", [False, True], ids=["w64", "w128"])
def test_scatter_map_b_splitk(wide, idt):
    """TN + mapB + mapC, f32 output, split-K 3 and 4 on a non-zero start: the atomic path (gemm_epilogue.hpp:145-153) adds at row
    mapC[r]; bound accb + s u (|old| + |A| |B|)"""
    K_, M, N = 256, 130, 72
    rows, out_rows = K_ + 9, M + 11
    a = rnd(K_, M, dtype=idt, seed=41)
    src = rnd(rows, N, dtype=idt, seed=42, scale=K_ ** -0.5)
    mb = make_map_b(K_, rows, seed=43)
    perm, untouched = make_perm(M, out_rows, seed=44)
    base = rnd(M, N, seed=45)
    g = Ref(d64(a).t(), gather_b64(src, mb))
    outs = []
    with form("gemm_small_kt", wide), launches() as c:
        for s in (3, 4):
            out = sentinel_out(out_rows, N, F32, perm, base)
            K.gemm(a, src, trans_a=True, trans_b=True, K=K_, map_b=mb.to(DEV), map_c=perm.to(DEV), out=out, accumulate=True, splitk=s)
            outs.append((s, out))
    only(c, "gemm_gather", 2)
    for s, out in outs:
        assert_close(out[perm.long().to(DEV)], g.acc + d64(base), g.accb + s * U32 * (d64(base).abs() + g.absab), "scatter tn splitk=%d" % s)
        check_untouched(out, untouched, "splitk=%d" % s)


# ------------------------------------------------------------------ scatter on the fast kernels (mapC without a gather)
def plain_operands(layout, M, N, K_, dtype):
    """op(A) [M, K], op(B) [K, N] that satisfy fast_ok (gemm.hip:718-730): K % BK == 0, 16-byte aligned bases and row strides, and for
    a transposed operand whole 16-byte column chunks inside the row stride (M = 130 columns live in rows of 136)"""
    if layout == "tn":
        a = rnd(K_, (M + 7) // 8 * 8, dtype=dtype, seed=51)[:, :M]
    else:
        a = rnd(M, K_, dtype=dtype, seed=51)
    b = rnd(N, K_, dtype=dtype, seed=52, scale=K_ ** -0.5) if layout == "nt" else rnd(K_, N, dtype=dtype, seed=52, scale=K_ ** -0.5)
    A = d64(a).t() if layout == "tn" else d64(a)
    B = d64(b).t() if layout == "nt" else d64(b)
    return a, b, A, B


@pytest.mark.parametrize("idt,odt", DT3, ids=DT3_IDS)
@pytest.mark.parametrize("wide", [False, True], ids=["w64", "w128"])
@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
def test_scatter_without_gather_on_the_fast_kernels(layout, wide, idt, odt):
    """mapC alone: fast_ok (gemm.hip:718-730) does not look at mapC, so with K = 256 (a multiple of BK) and aligned operands the product
    runs on gemm_fast_kernel, whose epilogue is the shared one.  Family: the layout's ordinary one (`_small` on the 64 x 64 form),
    one launch per product.  Plain (accb + r |acc|) and accumulate on a non-zero start (accb + r (|acc| + |ref|))."""
    M, N, K_ = 130, 72, 256
    ta, tb = layout == "tn", layout != "nt"
    a, b, A, B = plain_operands(layout, M, N, K_, idt)
    g = Ref(A, B)
    r = r_of(odt)
    out_rows = M + 11
    perm, untouched = make_perm(M, out_rows, seed=53)
    pd, pl = perm.to(DEV), perm.long().to(DEV)
    base = rnd(M, N, dtype=odt, seed=54)
    with form("gemm_small_nt" if layout == "nt" else "gemm_small_kt", wide), launches() as c:
        out = sentinel_out(out_rows, N, odt)
        K.gemm(a, b, ta, tb, map_c=pd, out=out)
        o_acc = sentinel_out(out_rows, N, odt, perm, base)
        K.gemm(a, b, ta, tb, map_c=pd, out=o_acc, accumulate=True)
    only(c, "gemm_%s%s" % (layout, "" if wide else "_small"), 2)
    assert_close(out[pl], g.acc, g.accb + r * g.acc.abs(), "%s mapC" % layout)
    check_untouched(out, untouched, "plain")
    ref = g.acc + d64(base)
    assert_close(o_acc[pl], ref, g.accb + r * (g.acc.abs() + ref.abs()), "%s mapC accumulate" % layout)
    check_untouched(o_acc, untouched, "accumulate")


@pytest.mark.parametrize("splitk,K_", [(1, 256), (2, 512)])
def test_scatter_tn_f32out_128_stays_off_the_two_slice_kernel(splitk, K_):
    """bf16 -> f32 TN on 128 x 128 tiles, plain, K / 64 >= 4 splitk and splitk 1 or even: everything gemm_tn2_kernel asks for, whose
    store loop writes row r and ignores mapC.  gemm.hip:755 (`plain && !a.mapC && ...`) keeps a scattered product off it; both kernels
    count as gemm_tn, so the witness is the scatter itself: rows mapC[r] hold the product, every other row keeps the sentinel."""
    M, N = 130, 136
    a, b, A, B = plain_operands("tn", M, N, K_, BF)
    g = Ref(A, B)
    out_rows = M + 11
    perm, untouched = make_perm(M, out_rows, seed=55)
    base = rnd(M, N, seed=56)
    out = sentinel_out(out_rows, N, F32, perm, base)
    with set_option("gemm_small_kt", 0), launches() as c:
        K.gemm(a, b, True, True, map_c=perm.to(DEV), out=out, accumulate=True, splitk=splitk)
    only(c, "gemm_tn", 1)
    old = d64(base)
    ref = g.acc + old
    bound = g.accb + (U32 * (g.acc.abs() + ref.abs()) if splitk == 1 else splitk * U32 * (old.abs() + g.absab))
    assert_close(out[perm.long().to(DEV)], ref, bound, "tn 128x128 mapC splitk=%d" % splitk)
    check_untouched(out, untouched, "tn 128x128 splitk=%d" % splitk)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_alone():
    """gemm.hip:809-815: mapA with trans_a, periodA 0 / negative / no multiple of 8, mapB without trans_b, dropout with split-K:
    S2T_EINVAL (-22) before any launch, the output keeps its bits"""
    M, N, K_ = 16, 16, 32
    a = rnd(M + 9, K_, seed=61)
    sq = rnd(K_, K_, seed=62)
    w = rnd(N, K_, seed=63)
    ma = make_map_a(1, M, M + 9, seed=64).to(DEV)
    mb = make_map_b(K_, K_, seed=65).to(DEV)
    out = torch.full((K_, K_), SENT, device=DEV)

    def refused(**kw):
        with launches() as c:
            with pytest.raises(L.S2THipError, match=r"error -22"):
                K.gemm(out=out, **kw)
        assert not any(c.values()), "a refused product launched %s" % c
        assert same_bits(out, torch.full_like(out, SENT)), "a refused product wrote its output"

    refused(a=sq, b=sq, trans_a=True, trans_b=True, M=M, K=K_, map_a=ma, period_a=K_)
    for period in (0, -8, 12, 20):
        refused(a=a, b=w, M=M, K=K_, map_a=ma, period_a=period)
    refused(a=a[:M], b=sq[:N], K=K_, map_b=mb)                               # NT + mapB
    refused(a=sq, b=sq, trans_a=True, trans_b=False, K=K_, map_b=mb)         # mapB, A^T without B^T
    refused(a=sq, b=sq, trans_a=True, trans_b=True, K=K_, map_b=mb, splitk=2, p_drop=0.25, seed=1)
    refused(a=a, b=w, M=M, K=K_, map_a=ma, period_a=K_, splitk=2, p_drop=0.25, seed=1)
