"""s2t_permute_cf, s2t_permute_conv_w, s2t_add_pos and s2t_augment (csrc/subsample.hip) bit for bit against their documented rules.

These kernels move values and round at most once, so every comparison is bit equality (`same_bits`) with an expectation built by
torch / numpy on the CPU from the values the kernel received:
  * a move into a bf16 destination is `from_f32<bf16>`, round to nearest even: torch's `.to(bfloat16)`;
  * an accumulating mode is one IEEE f32 add of the two values the kernel read: torch's f32 `+` on the CPU gives the same bits;
  * add_pos rounds `to_f32(src) + table` (one correctly rounded f32 add) once to the activation dtype: `(src.float() + table).to(dtype)`,
    for f32 the add itself.
There is one kernel per entry point; the paths inside (grid-stride loops beyond 4,096 x 256 work items, `nblocks` in subsample.hip; the
16-byte form of add_pos when D % E == 0 and all three pointers are 16-byte aligned, s2t_add_pos; the thread loop of augment for
F > 256) are reached by the sizes named at each case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
DT_IDS = ["f32", "bf16"]
K_TAP_SLOT = [5, 3, 6, 1, 0, 2, 7, 4, 8]          # subsample.hip kTapSlot: tap (kh*3+kw) -> class-major slot
EINVAL = -22


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield


def rnd(*shape, dtype=F32, seed=0, scale=1.0, dev=DEV):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def assert_same_bits(got, want, what):
    got = got.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s vs %s %s" % (what, got.dtype, tuple(got.shape), want.dtype, tuple(want.shape))
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        i = int(bad.reshape(-1).to(torch.int8).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), want.shape))
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %.9g want %.9g"
                             % (what, int(bad.sum()), bad.numel(), idx, float(got[idx]), float(want[idx])))


def refused(fn, *args, **kw):
    with pytest.raises(L.S2THipError, match=r"error -22"):
        fn(*args, **kw)


# ------------------------------------------------------------------ permute_cf
@pytest.mark.parametrize("N,C,F", [(1, 1, 1), (5, 64, 20), (3, 7, 5), (1024, 64, 20)])
def test_permute_cf(N, C, F):
    """mode 0: dst[n][f*C + c] = src[n][c*F + f], to f32 and to bf16 (= src.to(bfloat16) permuted); mode 1: dst[n][c*F + f] +=
    src[n][f*C + c] onto a non-zero f32 destination, refused for bf16.  (1024, 64, 20) is 1,310,720 elements > 4,096 x 256: the
    grid-stride loop takes a second trip."""
    src = rnd(N, C * F, seed=1)
    s = src.cpu()
    for dt in DTYPES:
        dst = torch.full((N, F * C), 7.0, dtype=dt, device=DEV)
        K.permute_cf(src, dst, N, C, F, 0)
        assert_same_bits(dst, s.to(dt).view(N, C, F).permute(0, 2, 1).reshape(N, F * C).contiguous(), "permute_cf mode 0 -> %s" % dt)
    dst0 = rnd(N, C * F, seed=2)
    dst = dst0.clone()
    K.permute_cf(src, dst, N, C, F, 1)
    assert_same_bits(dst, dst0.cpu() + s.view(N, F, C).permute(0, 2, 1).reshape(N, C * F), "permute_cf mode 1")
    keep = torch.full((N, C * F), 7.0, dtype=BF, device=DEV)
    refused(K.permute_cf, src, keep, N, C, F, 1)
    assert_same_bits(keep, torch.full((N, C * F), 7.0, dtype=BF), "permute_cf mode 1 refused for bf16")


# ------------------------------------------------------------------ permute_conv_w
def conv_w_mode1(w9, dt):
    """dst[ci][slot(tap)*Co + co] = w[co][ci][tap] written from the documented table kTapSlot"""
    Co, Ci, _ = w9.shape
    dst = torch.zeros(Ci, 9 * Co, dtype=dt)
    for tap in range(9):
        s = K_TAP_SLOT[tap]
        dst[:, s * Co:(s + 1) * Co] = w9[:, :, tap].t().to(dt)
    return dst


@pytest.mark.parametrize("Co,Ci", [(64, 64), (8, 16), (16, 8), (1, 1)])
def test_permute_conv_w(Co, Ci):
    """mode 0: dst[co][tap*Ci + ci] = w[co][ci][tap]; mode 1: dst[ci][slot(tap)*Co + co] = w[co][ci][tap] in the class-major order the
    data gradient's four class products slice (engine.py:462-463); both to f32 and to bf16.  mode 2: dst[co][ci][tap] += src[co][tap*Ci +
    ci], f32 only: mode 2 after mode 0 adds w itself onto a non-zero destination.  mode 2 to bf16 and mode 3 are refused."""
    from fbk_fairseq_st_amd.engine import _CLASS_SLOT0, _TAPS_BY_CLASS
    for c, (_, _, taps) in enumerate(_TAPS_BY_CLASS):          # the engine's slot table is kTapSlot
        for j, (kh, kw) in enumerate(taps):
            assert K_TAP_SLOT[3 * kh + kw] == _CLASS_SLOT0[c] + j
    w = rnd(Co, Ci, 3, 3, seed=3)
    w9 = w.cpu().view(Co, Ci, 9)
    for dt in DTYPES:
        d0 = torch.full((Co, 9 * Ci), 7.0, dtype=dt, device=DEV)
        K.permute_conv_w(w, d0, Co, Ci, 0)
        assert_same_bits(d0, w9.to(dt).permute(0, 2, 1).reshape(Co, 9 * Ci).contiguous(), "permute_conv_w mode 0 -> %s" % dt)
        d1 = torch.full((Ci, 9 * Co), 7.0, dtype=dt, device=DEV)
        K.permute_conv_w(w, d1, Co, Ci, 1)
        assert_same_bits(d1, conv_w_mode1(w9, dt), "permute_conv_w mode 1 -> %s" % dt)
    p0 = K.permute_conv_w(w, torch.empty((Co, 9 * Ci), device=DEV), Co, Ci, 0)
    g0 = rnd(Co, Ci, 3, 3, seed=4)
    g = g0.clone()
    K.permute_conv_w(p0, g, Co, Ci, 2)
    assert_same_bits(g, g0.cpu() + w.cpu(), "permute_conv_w mode 2 after mode 0")
    keep = torch.full((Co, Ci, 3, 3), 7.0, dtype=BF, device=DEV)
    refused(K.permute_conv_w, p0, keep, Co, Ci, 2)
    assert_same_bits(keep, torch.full((Co, Ci, 3, 3), 7.0, dtype=BF), "permute_conv_w mode 2 refused for bf16")
    keep = torch.full((Co, 9 * Ci), 7.0, device=DEV)
    refused(K.permute_conv_w, w, keep, Co, Ci, 3)
    refused(K.permute_conv_w, w, keep, Co, Ci, -1)
    assert_same_bits(keep, torch.full((Co, 9 * Ci), 7.0), "permute_conv_w mode 3 refused")


# ------------------------------------------------------------------ add_pos
def add_pos_expect(x, table, lens):
    """dst[t][b][:] = from_f32(to_f32(src[t][b][:]) + table[t + 1 if t < len[b] else 0][:])  (subsample.hip add_pos_kernel)"""
    T, B, D = x.shape
    t = torch.arange(T).view(T, 1)
    pos = torch.where(t < lens.view(1, B).long(), t + 1, torch.zeros_like(t))            # [T, B]
    return (x.float() + table[pos]).to(x.dtype)


def add_pos_lens(T, B):
    """lengths 0, 1, T and a value above T, in that order over the batch"""
    return torch.tensor([0, 1, T, T + 5][:B] + [max(1, T // 2)] * max(0, B - 4), dtype=torch.int32)


ADD_POS_SHAPES = [(5, 4, 6), (7, 4, 20), (9, 5, 64), (3, 4, 512)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("T,B,D", ADD_POS_SHAPES)
def test_add_pos(T, B, D, offset, dtype):
    """out of place and in place, without and with dropout.  The 16-byte form runs when D % E == 0 (E = 8 bf16 / 4 f32) and the
    pointers are aligned (s2t_add_pos): D = 64, 512 for both dtypes, D = 20 for f32; D = 6, D = 20 in bf16 and every `offset` case (src
    and dst one element past an aligned address) take the element-wise form.  The table's row 0 is random here (zeros in the model) so
    that a wrong row shows.  With p_drop: the same bits as K.dropout(K.add_pos(...)) -- the mask is s2t_dropout's on the flat index."""
    def buf(seed):
        if not offset:
            return rnd(T, B, D, dtype=dtype, seed=seed)
        t = rnd(T * B * D + 1, dtype=dtype, seed=seed)[1:].view(T, B, D)
        assert t.data_ptr() % 16 != 0
        return t
    x = buf(5)
    table = rnd(T + 3, D, seed=6)
    lens = add_pos_lens(T, B)
    ld = lens.to(DEV)
    want = add_pos_expect(x.cpu(), table.cpu(), lens)
    x0 = x.clone()
    out = buf(7)
    K.add_pos(x, table, ld, out=out)
    assert_same_bits(out, want, "add_pos out of place")
    assert_same_bits(x, x0.cpu(), "add_pos out of place changed its source")
    p, seed = 0.3, 77
    dropped = K.dropout(out.clone(), p, seed)                 # a fresh, aligned copy: s2t_dropout is not under test here
    out2 = buf(8)
    K.add_pos(x, table, ld, out=out2, p_drop=p, seed=seed)
    assert_same_bits(out2, dropped.cpu(), "add_pos with dropout, out of place")
    xi = buf(5)
    K.add_pos(xi, table, ld, p_drop=p, seed=seed)
    assert_same_bits(xi, dropped.cpu(), "add_pos with dropout, in place")
    xi = buf(5)
    K.add_pos(xi, table, ld)
    assert_same_bits(xi, want, "add_pos in place")


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
def test_add_pos_dropout_seed_above_32_bits(offset):
    """T, B, D = 9, 5, 64 in bf16, the 16-byte and the element-wise form: the dropout mask is s2t_dropout's also at a seed whose upper
    32 bits are set (the seed is a 64-bit argument; every other case here passes a small one)"""
    T, B, D, p, seed = 9, 5, 64, 0.3, (5 << 32) | 7
    def buf():
        t = rnd(T * B * D + 1, dtype=BF, seed=5)[1:].view(T, B, D) if offset else rnd(T, B, D, dtype=BF, seed=5)
        assert (t.data_ptr() % 16 != 0) == offset
        return t
    table = rnd(T + 3, D, seed=6)
    ld = add_pos_lens(T, B).to(DEV)
    plain = torch.empty(T, B, D, dtype=BF, device=DEV)
    K.add_pos(buf(), table, ld, out=plain)
    dropped = K.dropout(plain.clone(), p, seed)
    assert not torch.equal(bits(dropped), bits(K.dropout(plain.clone(), p, seed & 0xFFFFFFFF))), "the seed's upper word must move the mask"
    xi = buf()
    K.add_pos(xi, table, ld, p_drop=p, seed=seed)
    assert_same_bits(xi, dropped.cpu(), "add_pos with dropout, 64-bit seed")


def test_add_pos_grid_stride():
    """T = 600, B = 32, D = 512 in bf16: 1,228,800 16-byte items > 4,096 x 256, the vector form's grid-stride loop takes a second trip;
    with dropout against K.dropout(K.add_pos(...))"""
    T, B, D = 600, 32, 512
    x = rnd(T, B, D, dtype=BF, seed=9)
    table = rnd(T + 1, D, seed=10)
    g = torch.Generator().manual_seed(11)
    lens = torch.randint(0, T + 6, (B,), generator=g, dtype=torch.int32)
    lens[:4] = add_pos_lens(T, 4)
    out = torch.empty_like(x)
    K.add_pos(x, table, lens.to(DEV), out=out)
    assert_same_bits(out, add_pos_expect(x.cpu(), table.cpu(), lens), "add_pos grid stride")
    out2 = torch.empty_like(x)
    K.add_pos(x, table, lens.to(DEV), out=out2, p_drop=0.1, seed=5)
    assert torch.equal(bits(out2), bits(K.dropout(out, 0.1, 5))), "add_pos grid stride with dropout"


# ------------------------------------------------------------------ augment
def augment_loop(x, row_map, fmask, tmask, To):
    """the documented rule (subsample.hip:957-960) as a plain loop: out[b][t][f] = x[b][row_map[b][t]][f] (row_map absent: row t while
    t < T), zero where row_map is -1 / absent, inside a time mask [t0, t0 + w) or inside a frequency mask [f0, f0 + w)"""
    B, T, F = x.shape
    out = np.zeros((B, To, F), dtype=np.float32)
    for b in range(B):
        for t in range(To):
            src = int(row_map[b, t]) if row_map is not None else (t if t < T else -1)
            if tmask is not None and any(t0 <= t < t0 + w for t0, w in tmask[b]):
                src = -1
            if src < 0:
                continue
            for f in range(F):
                if fmask is not None and any(f0 <= f < f0 + w for f0, w in fmask[b]):
                    continue
                out[b, t, f] = x[b, src, f]
    return out


def augment_call(x, out, row_map, fmask, tmask, B, T, To, F, nF, nT):
    return L.load().s2t_augment(L.ptr(x), L.ptr(out), L.ptr(row_map), L.ptr(fmask), L.ptr(tmask), B, T, To, F, nF, nT, L.stream())


AUG_CASES = [
    # B, T, To, F, row map, nF, nT
    (3, 9, 12, 40, False, 3, 3), (3, 9, 9, 80, False, 3, 0), (3, 9, 6, 40, False, 0, 3), (2, 7, 11, 300, True, 3, 3),
    (1, 5, 8, 1, True, 0, 3), (1, 6, 6, 80, True, 0, 0), (3, 9, 12, 300, False, 0, 0),
]


@pytest.mark.parametrize("B,T,To,F,with_map,nF,nT", AUG_CASES)
def test_augment(B, T, To, F, with_map, nF, nT):
    """row_map absent with To > T, To == T, To < T (rows at or beyond T are zero); row_map with -1 entries and repeats; nF, nT at 0 and 3;
    the three masks of every utterance: one starting at 0 that overlaps the second, one of width 0, one running past F / To; F = 300 needs
    the thread loop (256 threads per row); B = 1"""
    g = torch.Generator().manual_seed(100 + B + T + To + F)
    x = rnd(B, T, F, seed=12)
    rm = None
    if with_map:
        rm = torch.randint(-1, T, (B, To), generator=g, dtype=torch.int32)
        rm[:, 0] = -1
        rm[:, 1:3] = T - 1                                 # a repeated source row
    fm = tm = None
    if nF:
        fm = torch.tensor([[[0, max(1, F // 4)], [F // 8, max(1, F // 4)], [F // 2, 0]]] * B, dtype=torch.int32)
        fm[-1, 2] = torch.tensor([F - 1 - (F > 1), 5])                                   # runs past F
        fm[0, 1, 0] = F // 3
    if nT:
        tm = torch.tensor([[[0, 2], [1, 2], [To // 2, 0]]] * B, dtype=torch.int32)
        tm[-1, 2] = torch.tensor([To - 2, 6])                                            # runs past To
    dev = lambda t: None if t is None else t.to(DEV)
    out = torch.full((B, To, F), 7.0, device=DEV)
    assert augment_call(x, out, dev(rm), dev(fm), dev(tm), B, T, To, F, nF, nT) == 0
    want = augment_loop(x.cpu().numpy(), None if rm is None else rm.numpy(), None if fm is None else fm.numpy().tolist(),
                        None if tm is None else tm.numpy().tolist(), To)
    assert_same_bits(out, torch.from_numpy(want), "augment")
    if not with_map and To > T and not nT:
        assert bool((out[:, T:] == 0).all())


def test_augment_refusals():
    """x == out, T <= 0 and a mask count without its table: S2T_EINVAL, the output keeps its bits"""
    B, T, F = 2, 5, 8
    x = rnd(B, T, F, seed=13)
    out = torch.full((B, T, F), 7.0, device=DEV)
    masks = torch.zeros(B, 1, 2, dtype=torch.int32, device=DEV)
    assert augment_call(x, x, None, None, None, B, T, T, F, 0, 0) == EINVAL
    assert augment_call(x, out, None, None, None, B, 0, T, F, 0, 0) == EINVAL
    assert augment_call(x, out, None, None, None, B, -1, T, F, 0, 0) == EINVAL
    assert augment_call(x, out, None, None, masks, B, T, T, F, 1, 0) == EINVAL
    assert augment_call(x, out, None, masks, None, B, T, T, F, 0, 1) == EINVAL
    torch.cuda.synchronize()
    assert_same_bits(out, torch.full((B, T, F), 7.0), "augment refusals")
    assert_same_bits(x, rnd(B, T, F, seed=13, dev="cpu"), "augment refusals changed x")
