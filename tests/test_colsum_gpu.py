"""s2t_colsum (csrc/gemm.hip colsum_kernel) per column against float64, on every lanes-per-row value and on the long-matrix branch.

out[n] += sum_m X[m][n].  Reference: the float64 column sums of the exact values the kernel read, plus the value `out` held before (the
kernel accumulates, so `out` starts non-zero).  Bound, with the depth counted from the kernel (`plan` below mirrors s2t_colsum,
gemm.hip:948-958, and colsum_kernel):
    a thread adds its rows one after the other into an f32 register: ceil(rows_of_a_block / (4 rpw)) adds, rpw = 64 / lpr rows per
      wave-instruction and 4 waves;
    the 256 / lpr partial sums of a column meet in LDS, added one after the other: 256 / lpr adds;
    every one of the gridDim.y row blocks leaves by one f32 atomic add onto the running out[n]: gridDim.y adds.
  Every add rounds a partial sum of magnitude <= S = |out0[n]| + sum_m |x[m][n]| (all terms of one sign at worst) by u = 2^-24 relative,
  and a value passes through at most d = thread adds + LDS adds + atomics of them:  |out - ref| <= d u S (1 + d u), written d u S
  with the (1 + d u) folded into counting the first add of each stage (which adds to an exact 0) as a rounding.  The bf16 -> f32
  conversion is exact.
Route: there is one kernel; its paths are picked by `vec` (16-byte aligned base and row stride, gemm.hip:952), by c0 + E <= N inside the
kernel (the element path for a ragged last lane), and by lpr / col_blocks / rows_per_block, which `plan` recomputes and the cases assert.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
DEV = "cuda"
U32 = 2.0 ** -24
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
DT_IDS = ["f32", "bf16"]


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K
    from fbk_fairseq_st_amd import kernels
    K = kernels
    K._lib()
    yield


def rnd(*shape, dtype=F32, seed=0, scale=1.0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def d64(t):
    return t.detach().cpu().double()


def elems(dtype):
    return 8 if dtype == BF else 4


def plan(M, N, dtype):
    """s2t_colsum's launch plan (gemm.hip:951-958): lanes per row, column blocks, rows per block, row blocks, and the depth d"""
    E = elems(dtype)
    lpr = 64
    while lpr > 1 and (lpr // 2) * E >= N:
        lpr //= 2
    col_blocks = (N + lpr * E - 1) // (lpr * E)
    rpb = max(256, (M * col_blocks + 1023) // 1024)
    row_blocks = (M + rpb - 1) // rpb
    rpw = 64 // lpr
    depth = (min(rpb, M) + 4 * rpw - 1) // (4 * rpw) + 256 // lpr + row_blocks
    return dict(lpr=lpr, col_blocks=col_blocks, rpb=rpb, row_blocks=row_blocks, depth=depth)


def assert_sums(out, ref, bound, what):
    o = d64(out)
    err = (o - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        i = int(ratio.argmax())
        raise AssertionError("%s: %d of %d columns out of bound; worst column %d: out %.9g ref %.9g |err| %.3g bound %.3g (%.3gx)"
                             % (what, int(bad.sum()), bad.numel(), i, float(o[i]), float(ref[i]), float(err[i]), float(bound[i]),
                                float(err[i] / bound[i]) if float(bound[i]) > 0 else math.inf))


def run(M, N, dtype, layout="plain", seed=1, expect=None):
    """one column-sum launch on an [M, N] matrix; layout: plain (contiguous, aligned), pad1 (row stride N + 1: ld % E != 0 when E
    divides N, and always a strided view), pad (row stride rounded up past N to a multiple of E: a strided view on the vector
    path), offset (base pointer one element past an aligned address: vec = 0).  `out` is the head of a longer buffer: the sums of the
    padding columns, and everything behind out[N - 1], must keep their bits."""
    E = elems(dtype)
    pl = plan(M, N, dtype)
    for k, v in (expect or {}).items():
        assert pl[k] == v, "the case was chosen for %s = %s, the plan gives %s" % (k, v, pl[k])
    if layout == "offset":
        x = rnd(M * N + 1, dtype=dtype, seed=seed)[1:].view(M, N)
        assert x.data_ptr() % 16 != 0
    else:
        ld = {"plain": N, "pad1": N + 1, "pad": (N + E) // E * E}[layout]
        x = rnd(M, ld, dtype=dtype, seed=seed)[:, :N]
        assert (x.stride(0) % E == 0) == (layout == "pad" or (layout == "plain" and N % E == 0))
    ld = x.stride(0)
    out0 = rnd(ld + 3, seed=seed + 1, scale=3.0)
    full = out0.clone()
    K.colsum(x, full[:N])
    torch.cuda.synchronize()
    xs = d64(x)
    ref = xs.sum(0) + d64(out0[:N])
    bound = pl["depth"] * U32 * (xs.abs().sum(0) + d64(out0[:N]).abs())
    what = "colsum %s M=%d N=%d %s (lpr %d, %d column blocks, %d rows per block, %d row blocks, depth %d)" % (
        "bf16" if dtype == BF else "f32", M, N, layout, pl["lpr"], pl["col_blocks"], pl["rpb"], pl["row_blocks"], pl["depth"])
    assert_sums(full[:N], ref, bound, what)
    assert torch.equal(full[N:].view(torch.int32), out0[N:].view(torch.int32)), what + ": a sum landed behind column N - 1"


# N on both sides of every halving of lpr (gemm.hip:954: lpr halves while (lpr / 2) E >= N): N = k E keeps lpr = k, N = k E + 1 needs 2k
LPR_STEPS = [(1, 1), (1, 2), (2, 2), (2, 4), (4, 4), (4, 8), (8, 8), (8, 16), (16, 16), (16, 32), (32, 32), (32, 64)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("k,lpr", LPR_STEPS, ids=["n%dE%s_lpr%d" % (k, "" if k == l else "+1", l) for k, l in LPR_STEPS])
def test_colsum_every_lanes_per_row(k, lpr, dtype):
    """lpr = 1 .. 64, N = k E (whole 16-byte lanes) and k E + 1 (the last lane takes the element path inside the vector kernel);
    M = 257: one row more than a block"""
    E = elems(dtype)
    N = k * E + (0 if k == lpr else 1)
    run(257, N, dtype, "plain" if N % E == 0 else "pad", expect=dict(lpr=lpr, col_blocks=1, row_blocks=2))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1025])
def test_colsum_row_counts_and_column_blocks(M, dtype):
    """M around the 256 rows of a block, with N = 65 E + 3: two column blocks (the second one ragged: E + 3 columns of 64 E) and a last
    lane on the element path; and N = 1 (one lane, one column)"""
    E = elems(dtype)
    run(M, 65 * E + 3, dtype, "pad", expect=dict(lpr=64, col_blocks=2))
    run(M, 1, dtype, "pad", expect=dict(lpr=1, col_blocks=1))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("layout", ["pad1", "offset", "pad"])
@pytest.mark.parametrize("k", [2, 9, 70])
def test_colsum_unaligned_and_strided(k, layout, dtype):
    """ld % E != 0 (pad1) and a base pointer off by one element (offset): vec = 0, every lane on the element path; pad: a strided view on
    the vector path.  N = k E.  The padding columns' sums and the buffer behind them keep their bits (checked in `run`)."""
    run(300, k * elems(dtype), dtype, layout)


BIG = [(262145, 1, F32), (262145, 4, F32), (262145, 8, BF), (600001, 4, F32), (600001, 5, BF), (300001, 64, BF)]


@pytest.mark.parametrize("M,N,dtype", BIG, ids=["m%d_n%d_%s" % (m, n, "bf16" if d == BF else "f32") for m, n, d in BIG])
def test_colsum_more_than_256_rows_per_block(M, N, dtype):
    """rows_per_block = ceil(M col_blocks / 1024) > 256 from M col_blocks > 262,144 on (gemm.hip:956-957): the branch every training step
    takes at engine.py:440.  N <= E keeps lpr = 1 and the matrices a few MB; one N = 64 bf16 case (lpr = 8) as the model has it."""
    pl = plan(M, N, dtype)
    assert pl["rpb"] > 256 and pl["row_blocks"] > 1000
    run(M, N, dtype, "plain" if N % elems(dtype) == 0 else "pad")
