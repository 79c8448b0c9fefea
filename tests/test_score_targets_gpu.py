"""s2t_score_targets (csrc/score.hip) against the float64 contract of tests/score_ref.py, element by element.

Every call goes to the entry point with explicit pointers and row strides (the wrapper K.score_targets has its own tests at the
end): the logit buffers are time-major [L, B, ld] with the columns [V, ld) filled with NaN and +inf, so that a read past V shows in
the result, and the output starts as NaN, so that an element nobody wrote shows.  Bounds: score_ref's docstring.

Dispatch the cases rely on (score.hip): 16-byte loads when every member's base and row stride are multiples of 16 bytes, scalar loads
otherwise; a workgroup per row below 4,096 rows (SCORE_WAVE_MIN_ROWS), a wave per row from there."""
import ctypes
import math

import pytest
import torch

from score_ref import assert_scores, ensemble_lse_bound, log_softmax_bound, score_ref

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
PAD = 1
WAVE_MIN_ROWS = 4096


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield


# ------------------------------------------------------------------ tools
def member(values, dtype, ld):
    """time-major device buffer [L, B, ld] holding values [L, B, V] (host f32) in `dtype`, columns [V, ld) = NaN, +inf, NaN, ...;
    ld odd multiples make rows that are not 16-byte aligned"""
    Ln, B, V = values.shape
    buf = torch.full((Ln, B, ld), math.nan, dtype=dtype, device=DEV)
    buf[:, :, V + 1::2] = math.inf
    buf[:, :, :V] = values.to(DEV).to(dtype)
    return buf


def aligned_ld(V, dtype, extra=0):
    e = 8 if dtype == BF else 4
    return (V + e - 1) // e * e + extra * e


def unaligned_ld(V, dtype):
    """a row stride >= V + 1 that is odd: every second row (bf16) or three rows of four (f32) start off a 16-byte boundary"""
    return V + 1 + (V % 2)


def raw_call(bufs, target, V, stream=None):
    """s2t_score_targets on buffers [L, B, ld_j]; target int64 [B, L] on the device -> f32 [B, L] that started as NaN"""
    Ln, B = bufs[0].shape[:2]
    n = len(bufs)
    out = torch.full((B, Ln), math.nan, dtype=F32, device=DEV)
    parr = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    larr = (ctypes.c_int * n)(*[b.shape[2] for b in bufs])
    rc = K._lib().s2t_score_targets(L.dt(bufs[0]), n, ctypes.addressof(parr), ctypes.addressof(larr), target.data_ptr(), out.data_ptr(),
                                    B, Ln, V, L.stream() if stream is None else stream)
    assert rc == 0, rc
    return out


def check(bufs, target, V, what, out=None):
    """run (unless given) and compare with the float64 contract on the values the kernel received"""
    if out is None:
        out = raw_call(bufs, target, V)
    xs = [b[:, :, :V].transpose(0, 1) for b in bufs]             # (B, L, V) views
    ref, bound = score_ref(xs, target)
    assert_scores(out, ref, bound, what)
    return out


def logits_host(Ln, B, V, seed, scale=3.0):
    return torch.randn(Ln, B, V, generator=torch.Generator().manual_seed(seed)) * scale


def target_sets(B, Ln, V, seed):
    """targets [B, L]: random columns with the special placements -- column 0, column V-1, the pad index, and out of range (-1 and V)
    between in-range neighbours.  With fewer than eight positions: one tensor per placement."""
    g = torch.Generator().manual_seed(seed)
    rows = B * Ln
    base = torch.randint(0, V, (rows,), generator=g)
    special = [0, V - 1, min(PAD, V - 1), -1, V]
    if rows >= 8:
        t = base.clone()
        pos = [0, rows - 1, rows // 2, 2, rows - 3]               # 2 and rows - 3 have in-range neighbours on both sides
        for p, c in zip(pos, special):
            t[p] = c
        return [t.view(B, Ln).to(DEV)]
    out = []
    for i, c in enumerate(special):
        t = base.clone()
        t[i % rows] = c
        out.append(t.view(B, Ln).to(DEV))
    return out


VS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2049, 5001, 32776]
SHAPES = [(1, 1), (3, 5), (2, 129), (5, 1), (1, 300)]


# ------------------------------------------------------------------ shapes: every V against every (B, L), both load forms, n = 1 and 2
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V", VS)
def test_vocabulary_and_batch_shapes(dtype, V):
    """V below one 16-byte vector, one wave of scalars / of vectors, one workgroup of vectors, odd widths, past 32,768; (B, L) with one
    row, B or L = 1, and more rows than one wave-per-row workgroup would hold.  Per shape: one member in aligned rows (vector loads),
    one member in unaligned rows (scalar loads), two members with different aligned strides."""
    for k, (B, Ln) in enumerate(SHAPES):
        v0 = logits_host(Ln, B, V, seed=V * 10 + k)
        v1 = logits_host(Ln, B, V, seed=V * 10 + k + 5)
        a0 = member(v0, dtype, aligned_ld(V, dtype))
        a1 = member(v1, dtype, aligned_ld(V, dtype, extra=2))
        u0 = member(v0, dtype, unaligned_ld(V, dtype))
        for tgt in target_sets(B, Ln, V, seed=V + k):
            what = "%s V=%d B=%d L=%d" % (dtype, V, B, Ln)
            o_vec = check([a0], tgt, V, what + " n=1 vector loads")
            o_sca = check([u0], tgt, V, what + " n=1 scalar loads")
            check([a0, a1], tgt, V, what + " n=2 ld=%d,%d" % (a0.shape[2], a1.shape[2]))
            assert o_vec.shape == o_sca.shape == (B, Ln)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_members_with_different_strides(dtype, n):
    """n members, each with its own row stride; all aligned (vector loads), then with one unaligned member (the launch falls back to
    scalar loads for all)"""
    for V, (B, Ln) in ((9, (3, 5)), (513, (2, 129)), (5001, (3, 5))):
        vals = [logits_host(Ln, B, V, seed=100 * n + j + V) for j in range(n)]
        tgt = target_sets(B, Ln, V, seed=n + V)[0]
        al = [member(v, dtype, aligned_ld(V, dtype, extra=j)) for j, v in enumerate(vals)]
        check(al, tgt, V, "%s n=%d V=%d aligned strides %s" % (dtype, n, V, [b.shape[2] for b in al]))
        mixed = al[:-1] + [member(vals[-1], dtype, unaligned_ld(V, dtype))]
        check(mixed, tgt, V, "%s n=%d V=%d last member unaligned" % (dtype, n, V))


# ------------------------------------------------------------------ the grid switch
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V", [65, 513, 1100])
@pytest.mark.parametrize("n", [1, 2])
def test_both_sides_of_the_grid_switch_agree_bit_for_bit(dtype, V, n):
    """4,096 rows run a wave per row, 4,095 a workgroup per row (score.hip: SCORE_WAVE_MIN_ROWS).  With B = 1 the first 4,095 rows of
    both calls are the same rows: both are checked against float64, and they must hold the same bits (the reduction tree is fixed by
    column, not by the launch form).  V = 1100: more than 256 scalars and more than one vector per slot, with a tail."""
    rows = WAVE_MIN_ROWS
    vals = [logits_host(rows, 1, V, seed=V + 31 * j + n) for j in range(n)]
    tgt = target_sets(1, rows, V, seed=V)[0]
    for ldf, form in ((aligned_ld, "vector"), (unaligned_ld, "scalar")):
        bufs = [member(v, dtype, ldf(V, dtype)) for v in vals]
        what = "%s V=%d n=%d %s loads" % (dtype, V, n, form)
        wave = check(bufs, tgt, V, what + " 4096 rows (wave per row)")
        block = check([b[:rows - 1] for b in bufs], tgt[:, :rows - 1].contiguous(), V, what + " 4095 rows (workgroup per row)")
        assert torch.equal(wave[:, :rows - 1].view(torch.int32), block.view(torch.int32)), what + ": the two launch forms differ in bits"


@pytest.mark.parametrize("dtype", [F32, BF])
def test_wave_form_with_a_partly_filled_last_workgroup(dtype):
    """4,102 = 7 x 586 rows: the last workgroup of the wave-per-row form holds two rows (its other waves leave), B > 1 so that the
    row -> (b, t) mapping of the output matters"""
    B, Ln, V = 7, 586, 130
    vals = logits_host(Ln, B, V, seed=77)
    check([member(vals, dtype, aligned_ld(V, dtype))], target_sets(B, Ln, V, seed=78)[0], V, "%s 7 x 586 rows" % dtype)
    check([member(vals, dtype, unaligned_ld(V, dtype))], target_sets(B, Ln, V, seed=78)[0], V, "%s 7 x 586 rows, scalar loads" % dtype)


# ------------------------------------------------------------------ special rows
def special_values(V, dtype, seed):
    """rows [L = 8, B = 1, V] and targets: 0 a target logit of -inf; 1 all logits equal; 2 logits spread over +-80 (f32) / +-30
    (bf16); 3 one dominant logit, target elsewhere; 4 -inf at a quarter of the non-target columns; 5 the first 600 columns -inf (whole
    slots stay empty, others start empty: the running maximum leaves -inf late), target behind them; 6, 7 plain"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, 1, V, generator=g) * 3
    t = torch.randint(0, V, (8,), generator=g)
    big = 80.0 if dtype == F32 else 30.0
    x[0, 0, t[0]] = -math.inf
    x[1] = 2.75
    x[2, 0] = (torch.rand(V, generator=g) * 2 - 1) * big
    x[3, 0, (int(t[3]) + 1) % V] += 40
    hole = torch.rand(V, generator=g) < 0.25
    hole[t[4]] = False
    x[4, 0, hole] = -math.inf
    k = min(600, V - 1)
    x[5, 0, :k] = -math.inf
    t[5] = V - 1
    return x, t.view(1, 8).to(DEV)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("V", [65, 513, 2049])
def test_special_rows(dtype, V):
    x, tgt = special_values(V, dtype, seed=V)
    for ldf in (aligned_ld, unaligned_ld):
        buf = member(x, dtype, ldf(V, dtype))
        out = check([buf], tgt, V, "%s V=%d special rows ld=%d" % (dtype, V, buf.shape[2]))
        assert bool(torch.isneginf(out[0, 0])), "a target logit of -inf must give -inf"


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_members_at_minus_infinity(dtype, n):
    """n > 1: position 0 has ONE member at -inf at the target (finite result: that member contributes probability 0), position 1 has
    ALL members at -inf there (exactly -inf), position 2 has all but one; the other positions are plain"""
    V, Ln = 513, 6
    tgt = torch.randint(0, V, (1, Ln), generator=torch.Generator().manual_seed(n)).to(DEV)
    vals = [logits_host(Ln, 1, V, seed=50 * n + j) for j in range(n)]
    vals[n // 2][0, 0, tgt[0, 0]] = -math.inf
    for j in range(n):
        vals[j][1, 0, tgt[0, 1]] = -math.inf
        if j != 1:
            vals[j][2, 0, tgt[0, 2]] = -math.inf
    bufs = [member(v, dtype, aligned_ld(V, dtype, extra=j % 2)) for j, v in enumerate(vals)]
    out = check(bufs, tgt, V, "%s n=%d members at -inf" % (dtype, n))
    assert bool(torch.isfinite(out[0, 0])) and bool(torch.isneginf(out[0, 1])) and bool(torch.isfinite(out[0, 2]))


# ------------------------------------------------------------------ determinism, streams
@pytest.mark.parametrize("rows", [300, 4100])
def test_two_calls_give_the_same_bits(rows):
    V, n = 1003, 3
    bufs = [member(logits_host(rows, 1, V, seed=rows + j), BF, aligned_ld(V, BF)) for j in range(n)]
    tgt = target_sets(1, rows, V, seed=rows)[0]
    a = raw_call(bufs, tgt, V)
    b = raw_call(bufs, tgt, V)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_call_on_another_stream():
    B, Ln, V = 3, 40, 777
    bufs = [member(logits_host(Ln, B, V, seed=5 + j), BF, aligned_ld(V, BF)) for j in range(2)]
    tgt = target_sets(B, Ln, V, seed=6)[0]
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = raw_call(bufs, tgt, V)                           # raw_call takes torch's current stream: st
    st.synchronize()
    check(bufs, tgt, V, "non-default stream", out=out)


# ------------------------------------------------------------------ equivalence with the existing route on the same logits
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_equals_log_softmax_gather_and_ensemble_lse(dtype, n):
    """n = 1: K.log_softmax(rows).gather(target) within the sum of both kernels' bounds; n > 1: K.ensemble_lse of the members' gathered
    log-probabilities (its bound on exact inputs plus what the members' errors pass through, plus this kernel's bound)"""
    B, Ln, V = 3, 37, 1003
    bufs = [member(logits_host(Ln, B, V, seed=9 * n + j), dtype, aligned_ld(V, dtype)) for j in range(n)]
    tgt = torch.randint(0, V, (B, Ln), generator=torch.Generator().manual_seed(n)).to(DEV)
    out = check(bufs, tgt, V, "%s n=%d" % (dtype, n))
    col = tgt.t().reshape(-1, 1)                                 # time-major rows t*B + b
    gathered, gbound = [], []
    for b in bufs:
        flat = b.view(Ln * B, -1)[:, :V]
        gathered.append(K.log_softmax(flat).gather(1, col)[:, 0].contiguous())
        gbound.append(log_softmax_bound(flat.double()).gather(1, col)[:, 0])
    if n == 1:
        old, old_bound = gathered[0], gbound[0]
    else:
        old = K.ensemble_lse(gathered)
        old_bound = ensemble_lse_bound(torch.stack([g.double() for g in gathered])) + torch.stack(gbound).max(0).values
    old = old.view(Ln, B).t()
    old_bound = old_bound.view(Ln, B).t()
    _, bound = score_ref([b[:, :, :V].transpose(0, 1) for b in bufs], tgt)
    err = (out.double() - old.double()).abs()
    assert bool((err <= bound + old_bound).all()), "worst %.3g against %.3g" % (float(err.max()), float((bound + old_bound).min()))


# ------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("dtype", [F32, BF])
def test_wrapper_takes_time_major_views_and_copies_what_it_must(dtype):
    """K.score_targets on (B, L, V) views of time-major buffers (padded stride: taken as they are -- the NaN / +inf padding would show
    in a copy-free read past V only, and a copy would still be right), on a batch-major contiguous tensor (copied into time-major
    order), with B = 1 and with L = 1"""
    for B, Ln, V in ((3, 7, 101), (1, 9, 101), (4, 1, 101)):
        bufs = [member(logits_host(Ln, B, V, seed=B + Ln + j), dtype, aligned_ld(V, dtype, extra=j)) for j in range(2)]
        views = [b[:, :, :V].transpose(0, 1) for b in bufs]
        tgt = torch.randint(0, V, (B, Ln), generator=torch.Generator().manual_seed(B)).to(DEV)
        ref, bound = score_ref(views, tgt)
        out = K.score_targets(views, tgt)
        assert out.shape == (B, Ln) and out.dtype == F32
        assert_scores(out, ref, bound, "wrapper, time-major views B=%d L=%d" % (B, Ln))
        assert_scores(K.score_targets([v.contiguous() for v in views], tgt), ref, bound, "wrapper, batch-major tensors B=%d L=%d" % (B, Ln))
        assert_scores(K.score_targets(views[:1], tgt), *score_ref(views[:1], tgt), "wrapper, one member")
        assert torch.equal(out.view(torch.int32), raw_call(bufs, tgt, V).view(torch.int32))
    with pytest.raises(ValueError):
        K.score_targets([views[0]] * 9, tgt)
    assert K.score_targets([torch.empty((0, 5, 11), dtype=dtype, device=DEV)], torch.empty((0, 5), dtype=torch.int64, device=DEV)).shape == (0, 5)
