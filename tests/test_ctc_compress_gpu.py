"""CTC compression kernels (csrc/ctc.hip: s2t_ctc_rle, s2t_ctc_compress_fwd / _bwd, and the pmax / lse values s2t_ctc_argmax hands
them) against float64, at the engine's shapes: T up to 1,500 frames, D up to 1,024, both dtypes, every strategy.

Every reference is computed here in numpy / torch float64 on the CPU from the exact operand values the kernel was given: bf16 operands
are widened exactly, `w` / `pmax` are the f32 values the previous kernel wrote.  Every tolerance is exact equality, a bound whose
derivation stands next to it (u = 2^-24, one f32 rounding), or a multiple of a CPU float32 yardstick measured in the same test."""
import numpy as np
import pytest
import torch

from oracle import int_ref

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
U = 2.0 ** -24                    # one f32 rounding (relative)
UB = 2.0 ** -8                    # one rounding to bf16's 8 significant bits, as the bounds below state it
DTYPES = [torch.float32, torch.bfloat16]
STRATEGIES = ("avg", "weighted", "softmax")


def f64(t):
    """exact widening of a device / host tensor to a float64 numpy array"""
    return t.detach().cpu().to(torch.float64).numpy()


def bits(t):
    """the raw bit patterns of a f32 / bf16 tensor, on the host"""
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


# ------------------------------------------------------------------ references
def rle_ref(pred, lens):
    """plain run-length pass over the first min(len, T) frames of every row: seg [B,T] (-1 past len), per-row arrays of starts / lengths"""
    B, T = pred.shape
    seg = np.full((B, T), -1, np.int32)
    starts, runs = [], []
    for b in range(B):
        Lb = int(min(T, max(int(lens[b]), 0)))
        s, n = [], []
        for t in range(Lb):
            if t == 0 or pred[b, t] != pred[b, t - 1]:
                s.append(t); n.append(0)
            n[-1] += 1
            seg[b, t] = len(s) - 1
        starts.append(np.array(s, np.int64)); runs.append(np.array(n, np.int64))
    return seg, starts, runs


def weights_ref(pmax, starts, runs, strategy, T):
    """fp64 weights from the f32 pmax [B,T]; also n_of[b,t] = length of the run frame t belongs to (0 past len)"""
    B = pmax.shape[0]
    w = np.zeros((B, T), np.float64)
    n_of = np.zeros((B, T), np.int64)
    p64 = pmax.astype(np.float64)
    for b in range(B):
        for s0, n in zip(starts[b], runs[b]):
            n_of[b, s0:s0 + n] = n
            if strategy == 0:
                w[b, s0:s0 + n] = 1.0 / n
                continue
            p = p64[b, s0:s0 + n]
            if strategy == 2:                         # softmax over the run, then divided by its own sum (conv_transformer.py:422-424)
                e = np.exp(p - p.max())
                p = e / e.sum()
            w[b, s0:s0 + n] = p / p.sum()
    return w, n_of


def check_rle(pred, lens, out, T):
    """exact comparison of seg / new_len / run_start / run_len (j < new_len) and of the frames past len; returns the reference runs"""
    seg, rs, rl, new_len, w = [t.cpu().numpy() for t in out]
    rseg, starts, runs = rle_ref(pred, lens)
    assert np.array_equal(seg, rseg)
    assert np.array_equal(new_len, np.array([len(s) for s in starts], np.int64))
    for b in range(pred.shape[0]):
        nl = len(starts[b])
        assert np.array_equal(rs[b, :nl], starts[b]), b
        assert np.array_equal(rl[b, :nl], runs[b]), b
    past = rseg < 0
    assert (seg[past] == -1).all()
    assert (w[past].view(np.uint32) == 0).all(), "w must be +0 past len"
    return rseg, starts, runs


def softmax_yardstick(pmax, starts, runs, wref, seg):
    """the reference's own arithmetic (numpy float32, int_ref.compress_weights_np) against fp64: largest relative error per run length"""
    yard = {}
    for b in range(pmax.shape[0]):
        if len(starts[b]) == 0:
            continue
        r = [(0, int(n)) for n in runs[b]]
        W = int_ref.compress_weights_np(pmax[b:b + 1, :, None], [r], "softmax", dtype=np.float32)[0]      # [T, new_len]
        Lb = int(runs[b].sum())
        w32 = W[np.arange(Lb), seg[b, :Lb]].astype(np.float64)
        rel = np.abs(w32 - wref[b, :Lb]) / wref[b, :Lb]
        for s0, n in zip(starts[b], runs[b]):
            yard[int(n)] = max(yard.get(int(n), 0.0), float(rel[s0:s0 + n].max()))
    return yard


def check_weights(pmax, w, starts, runs, seg, strategy, T, tag):
    """A2: strategy 0 bit-equal; 1 within (n + 2) u; 2 within twice the float32 yardstick of its run length, floored at (2n + 8) u"""
    wref, n_of = weights_ref(pmax, starts, runs, strategy, T)
    live = n_of > 0
    assert np.isfinite(w).all()
    if strategy == 0:
        assert np.array_equal(w[live].view(np.uint32), (1.0 / n_of[live]).astype(np.float32).view(np.uint32))
        return
    rel = np.zeros_like(wref)
    rel[live] = np.abs(w.astype(np.float64)[live] - wref[live]) / wref[live]
    if strategy == 1:
        # the kernel adds n positive f32 terms one after the other (n - 1 roundings, each relative to a partial sum of positive
        # terms, so at most (n - 1) u of the total) and divides once (1 rounding): n u, bounded here by the stated (n + 2) u
        bound = (n_of + 2) * U
        assert (rel[live] <= bound[live]).all(), (tag, float((rel[live] / bound[live]).max()))
        return
    yard = softmax_yardstick(pmax, starts, runs, wref, seg)
    worst_k = worst_y = worst_ratio = 0.0
    for n, y in sorted(yard.items()):
        allow = max(2.0 * y, (2 * n + 8) * U)            # twice the yardstick of this run length, floored at (2n + 8) u
        got = float(rel[n_of == n].max())
        worst_k, worst_y, worst_ratio = max(worst_k, got), max(worst_y, y), max(worst_ratio, got / allow)
        assert got <= allow, (tag, n, got, y, allow)
    print("MEASURED ctc weights softmax: %s run lengths %d..%d, numpy-f32 yardstick max rel err %.3e, kernel max rel err %.3e, "
          "kernel / allowed at worst %.3f" % (tag, min(yard), max(yard), worst_y, worst_k, worst_ratio))


# ------------------------------------------------------------------ A1 / A2 inputs
def rle_cases(T, seed):
    """utterances that exercise the 64-frame chunks of the ballot scan, the length edges and the frames past len; B >= 70"""
    rs = np.random.RandomState(seed)
    rows, lens, pm = [], [], []

    def add(p, ln, pmx=None):
        rows.append(np.asarray(p, np.int32)); lens.append(int(ln))
        pm.append(pmx if pmx is not None else (1.0 - rs.rand(T)).astype(np.float32))      # (0, 1]

    t = np.arange(T)
    for k in (64, 65, 128):                                   # boundaries 63|64, 64|65, 127|128
        add((t >= k).astype(np.int32), T)
    add((t >= 64).astype(np.int32) + (t >= 65) + (t >= 128), T)
    add(np.full(T, 7), T)                                     # one run covering the whole utterance
    add(t % 2, T)                                             # a new run on every frame
    add(t % 3, T, np.full(T, 0.5, np.float32))
    if T >= 4:
        add((t >= T - 3).astype(np.int32) * 5 + (t >= T - 1) * 2, T - 1)    # a run that ends exactly at len - 1, a new unit after it
    for ln in (0, 1, 63, 64, 65, T, T + 5):
        add(rs.randint(0, 3, T), ln)
        add(np.full(T, 4), ln)                                # frames past len would continue the last run if read
    add(np.full(T, 2), max(T // 2, 1), np.full(T, 0.25, np.float32))          # runs of equal values
    span = np.logspace(-30, 0, num=T).astype(np.float32)      # one run whose values span 1e-30 .. 1
    add(np.full(T, 1), T, span)
    add(np.full(T, 1), T, span[::-1].copy())
    add((t // 37) % 2, T, np.where(t % 37 == 5, 1.0, 1e-30).astype(np.float32))
    add((t >= 1).astype(np.int32), T)                         # a run of length 1 first
    while len(rows) < 72:                                     # random run lengths (geometric, mean 1.5 .. 40), random lengths
        mean = rs.choice([1.5, 4.0, 12.0, 40.0])
        p = np.cumsum(rs.rand(T) < 1.0 / mean) % 5
        add(p, rs.randint(0, T + 6))
    return np.stack(rows), np.array(lens, np.int64), np.stack(pm)


def run_rle(pred, pmax, lens, strategy):
    out = K.ctc_rle(torch.from_numpy(pred).to(DEV), torch.from_numpy(pmax).to(DEV), torch.from_numpy(lens).to(DEV), strategy)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("T", [1, 64, 65, 1500])
@pytest.mark.parametrize("strategy", [0, 1, 2])
def test_rle_runs_and_weights(T, strategy):
    """A1 + A2.  `pred` is built directly and `pmax` is random in (0, 1], so the arg-max is out of the picture: the run-length
    outputs must equal a plain Python pass and the weights must stay inside their bounds (check_weights).

    Strategy 2 measured on MI355X (the MEASURED lines), largest relative error of a weight against fp64:
      T = 64, run lengths 1..64:     numpy-f32 yardstick 2.6e-07, kernel 4.1e-07, kernel / allowed at worst 0.22
      T = 65, run lengths 1..65:     numpy-f32 yardstick 2.5e-07, kernel 5.7e-07, kernel / allowed at worst 0.15
      T = 1,500, run lengths 1..1500: numpy-f32 yardstick 3.1e-07, kernel 1.2e-05, kernel / allowed at worst 0.19
    The yardstick sums pairwise, the kernel serially: its error grows with the run length, as the floor (2n + 8) u does."""
    pred, lens, pmax = rle_cases(T, seed=100 + T)
    assert pred.shape[0] >= 70
    out = run_rle(pred, pmax, lens, strategy)
    seg, starts, runs = check_rle(pred, lens, out, T)
    w = out[4].cpu().numpy()
    check_weights(pmax, w, starts, runs, seg, strategy, T, "T=%d" % T)
    if strategy in (0, 1):                                    # a run of length 1 weighs exactly 1
        for b in range(pred.shape[0]):
            for s0 in starts[b][runs[b] == 1]:
                assert w[b, s0] == np.float32(1.0)


# ------------------------------------------------------------------ A3 / A4 inputs and checks
RUN_PATTERN = (1, 2, 3, 4, 5, 7, 8, 9)


def compress_case(T, B, seed):
    """pred with runs of 1, 2, 3, 4, 5, 7, 8, 9 frames and one of several hundred (where T allows), lengths that differ per utterance"""
    rs = np.random.RandomState(seed)
    pred = np.zeros((B, T), np.int32)
    for b in range(B):
        runs = list(np.roll(RUN_PATTERN, b))
        if T > 100:
            runs += [min(T // 2 + 37 * b, 700)] + list(np.roll(RUN_PATTERN, b + 3))
        while sum(runs) < T:
            runs.append(int(rs.choice(RUN_PATTERN)))
        pred[b] = np.repeat(np.arange(len(runs)) % 3, runs)[:T]
    lens = np.array([T, max(T - 1, 1), max(T // 2, 1), T + 5, min(T, 65)][:B], np.int64)
    pmax = (1.0 - rs.rand(B, T)).astype(np.float32)
    return pred, lens, pmax


def raw_fwd(x, w, rs, rl, new_len, out, Tout):
    T, B, D = x.shape
    return K._lib().s2t_ctc_compress_fwd(L.dt(x), L.ptr(x), L.ptr(w), L.ptr(rs), L.ptr(rl), L.ptr(new_len), L.ptr(out), T, B, D, Tout, L.stream())


def raw_bwd(dout, w, seg, dx, accumulate):
    T, B, D = dx.shape
    return K._lib().s2t_ctc_compress_bwd(L.dt(dx), L.ptr(dout), L.ptr(w), L.ptr(seg), L.ptr(dx), T, B, D, int(accumulate), L.stream())


def offset_view(shape, dtype, fill=None):
    """a contiguous tensor that starts one element into its allocation (never 16-byte aligned) and the allocation itself"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2, dtype=dtype, device=DEV)
    if fill is not None:
        buf.fill_(fill)
    v = buf[1:1 + n].view(*shape)
    assert v.data_ptr() % 16 != 0
    return v, buf


def fwd_ref(x64, w, starts, runs, Tout):
    """fp64 out[j][b] = sum_k w[b][s0+k] x[s0+k][b], the sum of magnitudes beside it and the run length of every output row"""
    T, B, D = x64.shape
    ref = np.zeros((Tout, B, D)); mag = np.zeros((Tout, B, D)); n_of = np.zeros((Tout, B), np.int64)
    w64 = w.astype(np.float64)
    for b in range(B):
        nl = len(starts[b])
        if nl == 0:
            continue
        Lb = int(runs[b].sum())
        prod = w64[b, :Lb, None] * x64[:Lb, b, :]
        ref[:nl, b] = np.add.reduceat(prod, starts[b], axis=0)
        mag[:nl, b] = np.add.reduceat(np.abs(prod), starts[b], axis=0)
        n_of[:nl, b] = runs[b]
    return ref, mag, n_of


def fwd_serial_f32(x32, w, starts, runs, Tout):
    """the same sum in numpy float32, one frame after the other (product rounded, then added)"""
    T, B, D = x32.shape
    acc = np.zeros((Tout, B, D), np.float32)
    for b in range(B):
        nl = len(starts[b])
        for k in range(int(runs[b].max()) if nl else 0):
            j = np.nonzero(runs[b] > k)[0]
            t = starts[b][j] + k
            acc[j, b] = acc[j, b] + w[b, t, None] * x32[t, b]
    return acc


def check_fwd(x, out_rle, starts, runs, dtype, tag):
    """A3 on one (x, weights) pair: NaN pre-fill, Tout = max(new_len) + 3 (capped at T), rows past new_len exactly zero, the
    derived per-element bound; returns (out, bound) for the adjoint check"""
    T, B, D = x.shape
    seg, rs, rl, new_len, w_dev = out_rle
    Tout = min(max(len(s) for s in starts) + 3, T)
    out = torch.full((Tout, B, D), float("nan"), dtype=dtype, device=DEV)
    assert raw_fwd(x, w_dev, rs, rl, new_len, out, Tout) == 0
    torch.cuda.synchronize()
    got = f64(out)
    assert not np.isnan(got).any(), tag
    ob = bits(out)
    for b in range(B):
        assert (ob[len(starts[b]):, b] == 0).all(), (tag, b)
    w = w_dev.cpu().numpy()
    ref, mag, n_of = fwd_ref(f64(x), w, starts, runs, Tout)
    # n products and n - 1 additions in f32 -- in any order, fused or not -- err by at most gamma_n sum |w x| <= (n + 1) u sum |w x|;
    # in the wave-split form a term passes through at most n/4 accumulations and the three additions of the partials, fewer still.
    # The stated bound is (n + 2) u sum |w x|.  A bf16 output is rounded once more: 2^-8 |ref|.
    bound = (n_of[:, :, None] + 2) * U * mag
    cpu = fwd_serial_f32(x.float().cpu().numpy(), w, starts, runs, Tout).astype(np.float64)
    assert (np.abs(cpu - ref) <= bound).all(), "the bound does not hold for a plain float32 evaluation: " + tag
    if dtype == torch.bfloat16:
        bound = bound + UB * np.abs(ref)
    err = np.abs(got - ref)
    assert (err <= bound).all(), (tag, float(err.max()), int((err > bound).sum()))
    return got, bound


def bwd_ref(dout64, w, seg, shape):
    T, B, D = shape
    ref = np.zeros(shape)
    w64 = w.astype(np.float64)
    for b in range(B):
        live = seg[b] >= 0
        ref[live, b] = w64[b, live, None] * dout64[seg[b, live], b]
    return ref


def check_bwd(dout, w_dev, seg_dev, seg, shape, dtype, accumulate, aligned, tag):
    """A4 on one (dout, weights) pair; returns (dx, bound) for the adjoint check"""
    T, B, D = shape
    w = w_dev.cpu().numpy()
    wd = bwd_ref(f64(dout), w, seg, shape)
    if aligned:
        dx, buf = torch.empty(shape, dtype=dtype, device=DEV), None
        assert dx.data_ptr() % 16 == 0
    else:
        dx, buf = offset_view(shape, dtype)
        buf[0] = 123.0; buf[-1] = 65.0
    if accumulate:
        o = torch.randn(shape, generator=torch.Generator().manual_seed(T * 31 + D)).to(dtype)
        dx.copy_(o.to(DEV))
    else:
        dx.fill_(float("nan"))
    assert raw_bwd(dout, w_dev, seg_dev, dx, accumulate) == 0
    torch.cuda.synchronize()
    got = f64(dx)
    assert not np.isnan(got).any(), tag
    if buf is not None:
        assert float(buf[0]) == 123.0 and float(buf[-1]) == 65.0
    if accumulate:
        o64 = f64(o)
        ref = o64 + wd
        # one rounding of the product and one of the sum, each at most u (|w dout| + |o|)
        bound = 2 * U * (np.abs(wd) + np.abs(o64))
        past = seg < 0                                              # [B, T]: those frames come back as they were, bit for bit
        gi, oi = bits(dx), bits(o)
        for b in range(B):
            assert np.array_equal(gi[past[b], b], oi[past[b], b]), (tag, b)
    else:
        ref = wd
        bound = U * np.abs(ref)                                     # one product, one rounding; exactly zero where seg < 0
    if dtype == torch.bfloat16:
        bound = bound + UB * np.abs(ref)
    err = np.abs(got - ref)
    assert (err <= bound).all(), (tag, float(err.max()), int((err > bound).sum()))
    return got, bound


def rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", [12, 333, 1500])
@pytest.mark.parametrize("D", [64, 256, 512, 1024, 100, 6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compress_fwd(dtype, D, T, B):
    """A3: the wave-split vector path with one (D <= 512 bf16 / 256 f32) and several d0 iterations, runs longer than four frames (all
    four LDS partials carry terms), and the element-wise path (D = 100 in bf16, D = 6), for all three strategies' weights"""
    pred, lens, pmax = compress_case(T, B, seed=T + D)
    seg, starts, runs = rle_ref(pred, lens)
    x = rnd((T, B, D), dtype, seed=7 * D + T).to(DEV)
    assert x.data_ptr() % 16 == 0
    for s in range(3):
        out_rle = run_rle(pred, pmax, lens, s)
        check_fwd(x, out_rle, starts, runs, dtype, "fwd %s D=%d T=%d B=%d %s" % (dtype, D, T, B, STRATEGIES[s]))


@pytest.mark.parametrize("D", [64, 512])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compress_fwd_unaligned_base(dtype, D):
    """a view that starts one element into its allocation, D a multiple of 8: the vector path's 16-byte accesses would be
    misaligned, so the call must take the element-wise path and still be right -- for an unaligned input and for an unaligned
    output, whose neighbouring elements must stay untouched"""
    T, B = 333, 5
    pred, lens, pmax = compress_case(T, B, seed=D)
    seg, starts, runs = rle_ref(pred, lens)
    x, xbuf = offset_view((T, B, D), dtype)
    x.copy_(rnd((T, B, D), dtype, seed=D).to(DEV))
    out_rle = run_rle(pred, pmax, lens, 1)
    check_fwd(x, out_rle, starts, runs, dtype, "fwd unaligned x %s D=%d" % (dtype, D))
    xa = x.clone()
    assert xa.data_ptr() % 16 == 0
    Tout = min(max(len(s) for s in starts) + 3, T)
    out, obuf = offset_view((Tout, B, D), dtype, fill=float("nan"))
    obuf[0] = 123.0; obuf[-1] = 65.0
    assert raw_fwd(xa, out_rle[4], out_rle[1], out_rle[2], out_rle[3], out, Tout) == 0
    torch.cuda.synchronize()
    got = f64(out)
    r64, mag, n_of = fwd_ref(f64(xa), out_rle[4].cpu().numpy(), starts, runs, Tout)
    bound = (n_of[:, :, None] + 2) * U * mag + (UB * np.abs(r64) if dtype == torch.bfloat16 else 0.0)      # as check_fwd
    assert not np.isnan(got).any() and (np.abs(got - r64) <= bound).all()
    assert float(obuf[0]) == 123.0 and float(obuf[-1]) == 65.0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("T,B", [(12, 1), (333, 5), (1500, 5)])
@pytest.mark.parametrize("D", [64, 512, 1024, 100])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compress_bwd_and_adjoint(dtype, D, T, B, accumulate):
    """A4: dx = w dout[seg] (+ o), zero / untouched past len, and <out, dout> = <x, dx> in fp64 on the kernels' own outputs"""
    pred, lens, pmax = compress_case(T, B, seed=T + D)
    seg, starts, runs = rle_ref(pred, lens)
    x = rnd((T, B, D), dtype, seed=7 * D + T).to(DEV)
    for s in ((1, 2) if accumulate else (0, 1, 2)):
        tag = "bwd %s D=%d T=%d B=%d %s acc=%d" % (dtype, D, T, B, STRATEGIES[s], accumulate)
        out_rle = run_rle(pred, pmax, lens, s)
        assert np.array_equal(out_rle[0].cpu().numpy(), seg)
        Tout = min(max(len(st) for st in starts) + 3, T)
        dout = rnd((Tout, B, D), dtype, seed=D + s).to(DEV)
        dx, bdx = check_bwd(dout, out_rle[4], out_rle[0], seg, (T, B, D), dtype, accumulate, True, tag)
        if accumulate:
            continue
        out, bout = check_fwd(x, out_rle, starts, runs, dtype, tag)
        # both inner products in fp64 on what the kernels returned.  In exact arithmetic <ref_out, dout> = <x, ref_dx>, so
        # <out, dout> - <x, dx> = <out - ref_out, dout> - <x, dx - ref_dx>: at most the two kernels' own bounds, each weighted by
        # the other factor.  (The fp64 summation itself errs by ~1e-16 of the sums of magnitudes: the 1e-12 term.)
        d64, x64 = f64(dout), f64(x)
        lhs, rhs = float((out * d64).sum()), float((x64 * dx).sum())
        slack = float((bout * np.abs(d64)).sum() + (bdx * np.abs(x64)).sum())
        assert abs(lhs - rhs) <= slack + 1e-12 * float(np.abs(out * d64).sum() + np.abs(x64 * dx).sum()), (tag, lhs, rhs, slack)


@pytest.mark.parametrize("dtype", DTYPES)
def test_compress_bwd_unaligned_base(dtype):
    """dx a view one element into its allocation: the same result, and the elements around it untouched"""
    T, B, D = 333, 5, 64
    pred, lens, pmax = compress_case(T, B, seed=D)
    seg, starts, runs = rle_ref(pred, lens)
    out_rle = run_rle(pred, pmax, lens, 2)
    Tout = min(max(len(st) for st in starts) + 3, T)
    dout = rnd((Tout, B, D), dtype, seed=3).to(DEV)
    for acc in (0, 1):
        check_bwd(dout, out_rle[4], out_rle[0], seg, (T, B, D), dtype, acc, False, "bwd unaligned %s acc=%d" % (dtype, acc))


# ------------------------------------------------------------------ A5: pmax / lse
def argmax_rows(T, B, V, dtype, seed):
    """logit rows: random at scale 3, some with a spread of 65 between largest and smallest (exp underflows), some near-uniform"""
    x = rnd((T, B, V), torch.float32, seed, scale=3.0)
    g = torch.Generator().manual_seed(seed + 1)
    for r in range(0, T, 5):
        x[r, 0] = torch.rand(V, generator=g) * 60.0 - 35.0
        i = (7 * r + 3) % V
        x[r, 0, i] = 30.0
        x[r, 0, (i + V // 2) % V] = -35.0
    for r in range(2, T, 7):
        x[r, B - 1] = torch.randn(V, generator=g) * 1e-3
    return x.to(dtype)


def check_pmax_lse(pred, pmax, lse, x_host, tag):
    """pmax against the fp64 softmax probability of the index the kernel chose, lse against the fp64 log-sum-exp; tolerances of
    test_ctc_argmax_padded_rows_single_pass_and_three_pass: 1e-5 relative for pmax, 1e-4 absolute for lse"""
    T, B, V = x_host.shape
    x64 = x_host.to(torch.float64)
    lse64 = torch.logsumexp(x64, -1)                                  # [T, B]
    idx = pred.cpu().long().t().unsqueeze(-1)                         # [T, B, 1]
    assert int(idx.min()) >= 0 and int(idx.max()) < V
    p64 = torch.exp(torch.gather(x64, 2, idx).squeeze(-1) - lse64)
    got_p = pmax.cpu().double().t()
    assert float(((got_p - p64).abs() / p64).max()) <= 1e-5, tag
    assert float((lse.cpu().double().view(T, B) - lse64).abs().max()) <= 1e-4, tag


@pytest.mark.parametrize("route", ["f32", "bf16_generic", "bf16_row4", "bf16_row10", "bf16_row16"])
def test_argmax_pmax_and_lse(route):
    """A5: the values the arg-max hands to the run-length pass (pmax) and to the CTC loss (lse), for the f32 kernel, the bf16
    three-pass kernel on dense rows of odd V (rows not 16-byte aligned) and the three register-resident widths of the single-pass
    kernel on padded rows; rows with a spread of 65 between the largest and the smallest logit among them"""
    T, B = 41, 3
    V = dict(f32=1003, bf16_generic=1003, bf16_row4=2001, bf16_row10=5001, bf16_row16=8001)[route]
    dtype = torch.float32 if route == "f32" else torch.bfloat16
    x = argmax_rows(T, B, V, dtype, seed=V)
    assert float(x[0, 0].float().max() - x[0, 0].float().min()) >= 60.0
    if route in ("f32", "bf16_generic"):
        xd = x.to(DEV)                                                # dense rows: odd V, so bf16 rows are not 16-byte aligned
        assert xd.stride(1) == V
    else:
        xd = K.alloc_rows((T, B), V, dtype, DEV)
        xd.copy_(x.to(DEV))
        assert xd.stride(1) % 8 == 0 and xd.data_ptr() % 16 == 0
    pred, pmax, lse = K.ctc_argmax(xd, want_lse=True)
    torch.cuda.synchronize()
    check_pmax_lse(pred, pmax, lse, x, route)


# ------------------------------------------------------------------ A6: the chain at an engine shape
@pytest.mark.parametrize("strategy", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_chain_at_engine_shape(dtype, strategy):
    """x [375, 4, 512] -> CTC head GEMM (V = 1,003, padded rows) -> arg-max with lse -> run-length pass -> compress forward ->
    backward, every stage against fp64 GIVEN the previous kernel's own output (the split oracle/s2t_ref.ctc_compress makes with
    pred_override): the weights come from the kernel's pmax, so the bounds of A2-A4 apply unchanged"""
    T, B, D, V = 375, 4, 512, 1003
    Wc = rnd((V, D), dtype, seed=12, scale=D ** -0.5)
    # the head's bias favours unit V-1; blocks of 50 frames whose input leans along that unit's weight row let it win there frame
    # after frame (long runs), the frames in between go to whichever unit the random input picks (short runs)
    bias = torch.zeros(V); bias[V - 1] = 2.0
    lean = ((torch.arange(T) // 50) % 2 == 0).float() * 18.0
    wrow = Wc[V - 1].float()
    x = (rnd((T, B, D), torch.float32, seed=11) + lean.view(T, 1, 1) * (wrow / wrow.norm() ** 2).view(1, 1, D)).to(dtype).to(DEV)
    logits2 = K.alloc_rows((T * B,), V, dtype, DEV)
    K.gemm(x.view(T * B, D), Wc.to(DEV), bias=bias.to(DEV), out=logits2)
    logits = logits2.view(T, B, V)
    pred, pmax, lse = K.ctc_argmax(logits, want_lse=True)
    torch.cuda.synchronize()
    check_pmax_lse(pred, pmax, lse, logits.cpu(), "chain")
    lens = np.array([T, T - 1, 200, 65], np.int64)
    out_rle = K.ctc_rle(pred, pmax, torch.from_numpy(lens).to(DEV), strategy)
    torch.cuda.synchronize()
    pred_np, pmax_np = pred.cpu().numpy(), pmax.cpu().numpy()
    seg, starts, runs = check_rle(pred_np, lens, out_rle, T)
    assert max(int(r.max()) for r in runs) >= 40, "the bias must produce long runs"
    assert min(int(r.min()) for r in runs) == 1
    tag = "chain %s %s" % (dtype, STRATEGIES[strategy])
    check_weights(pmax_np, out_rle[4].cpu().numpy(), starts, runs, seg, strategy, T, tag)
    check_fwd(x, out_rle, starts, runs, dtype, tag)
    Tout = min(max(len(s) for s in starts) + 3, T)
    dout = rnd((Tout, B, D), dtype, seed=13).to(DEV)
    for acc in (0, 1):
        check_bwd(dout, out_rle[4], out_rle[0], seg, (T, B, D), dtype, acc, True, tag)


# ------------------------------------------------------------------ A7: refusals and no-ops
def test_refusals_and_noops():
    """argument checks of s2t_ctc_rle / s2t_ctc_compress_fwd / _bwd: they return before any launch"""
    T, B, D = 12, 2, 8
    lib = K._lib()
    pred = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    pmax = torch.ones(B, T, device=DEV)
    lens = torch.full((B,), T, dtype=torch.int64, device=DEV)
    seg, rs, rl, new_len, w = K.ctc_rle(pred, pmax, lens, 0)
    x = torch.ones(T, B, D, device=DEV)
    out = torch.full((T, B, D), 5.0, device=DEV)
    st = L.stream()

    def rle(strategy, pred_=pred, B_=B, T_=T, w_=w):
        return lib.s2t_ctc_rle(L.ptr(pred_), L.ptr(pmax), L.ptr(lens), L.ptr(seg), L.ptr(rs), L.ptr(rl), L.ptr(new_len), L.ptr(w_), T_, B_, strategy, st)

    def fwd(dt=0, x_=x, Tout=3, B_=B, out_=out, w_=w):
        return lib.s2t_ctc_compress_fwd(dt, L.ptr(x_), L.ptr(w_), L.ptr(rs), L.ptr(rl), L.ptr(new_len), L.ptr(out_), T, B_, D, Tout, st)

    def bwd(dt=0, dout_=x, B_=B, T_=T, dx_=out, seg_=seg):
        return lib.s2t_ctc_compress_bwd(dt, L.ptr(dout_), L.ptr(w), L.ptr(seg_), L.ptr(dx_), T_, B_, D, 0, st)

    w_before = w.clone()
    assert rle(3) == -22 and rle(-1) == -22
    assert rle(0, pred_=None) == -22 and rle(0, w_=None) == -22
    assert fwd(Tout=T + 1) == -22
    assert fwd(x_=None) == -22 and fwd(out_=None) == -22 and fwd(w_=None) == -22
    assert bwd(dout_=None) == -22 and bwd(dx_=None) == -22 and bwd(seg_=None) == -22
    assert fwd(dt=2) == -95 and bwd(dt=2) == -95
    assert rle(0, B_=0) == 0 and rle(0, T_=0) == 0
    assert fwd(B_=0) == 0 and fwd(Tout=0) == 0
    assert bwd(B_=0) == 0 and bwd(T_=0) == 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused or empty call must write nothing"
    assert torch.equal(w, w_before)
