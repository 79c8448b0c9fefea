"""engine.conv2_maps / engine.attn2d_maps against a real convolution, in float64 on the CPU (no kernel runs here).

The row maps give s2t_gemm_gather's operands their meaning (csrc/gemm_epilogue.hpp:12-14):
    A(r, k) = Asrc[mapA[(k / period) * M + r]][k % period],  B(k, :) = Bsrc[mapB[k]],  C row mapC[r] <- product row r,  -1 = zeros.
`gathered_a` / `gathered_b` below build exactly those operands with torch indexing, and every product is written the way the engine
calls it (engine.py subsample_fwd / subsample_bwd / attn2d_block_fwd / _bwd), with the weight layouts of s2t_permute_conv_w
(csrc/subsample.hip: mode 0 dst[co][tap*Ci+ci], mode 1 dst[ci][slot(tap)*Co+co], kTapSlot = {5,3,6,1,0,2,7,4,8}) and of
s2t_a2d_pack_w mode 1 (mirrored taps) written out in torch.  The result is compared with F.conv2d and its autograd.

Tolerance: both sides add the same <= 9 Ci (or P) float64 products in different orders; the difference is at most a few hundred
units of 2^-53 ~ 1e-16 of sum |terms|, so 1e-12 of the largest |reference| element is ample and a single misplaced map entry (an
O(1) error) is not.  tests/test_gemm_gather_gpu.py ties the kernels to this gathered formulation.
"""
import pytest
import torch
import torch.nn.functional as F

from fbk_fairseq_st_amd.engine import _CLASS_SLOT0, _TAPS_BY_CLASS, attn2d_maps, conv2_maps

K_TAP_SLOT = [5, 3, 6, 1, 0, 2, 7, 4, 8]          # csrc/subsample.hip kTapSlot: tap (kh*3+kw) -> class-major slot
SIZES = [1, 2, 3, 7, 8]
CI, CO = 3, 5                                     # different on purpose: a Ci / Co mix-up changes shapes or values


def rnd64(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def gathered_a(src, maps, period):
    """[M, taps*period]: A(r, k) = src[maps[k / period][r]][k % period], -1 -> zeros  (gemm_epilogue.hpp:12)"""
    taps, M = maps.shape
    assert src.shape[1] == period
    idx = maps.long()
    rows = src[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1)          # [taps, M, period]
    return rows.permute(1, 0, 2).reshape(M, taps * period)


def gathered_b(src, map_b):
    """[K, N]: B(k, :) = src[map_b[k]], -1 -> zeros  (gemm_epilogue.hpp:13)"""
    idx = map_b.long()
    return src[idx.clamp_min(0)] * (idx >= 0).unsqueeze(-1)


def close(got, ref, what):
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    tol = 1e-12 * max(1.0, float(ref.abs().max()))
    if not bool((err <= tol).all()):
        i = int(err.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: worst at %s: got %.17g ref %.17g |err| %.3g tol %.3g"
                             % (what, idx, float(got[idx]), float(ref[idx]), float(err[idx]), tol))


def test_tap_slot_tables_agree():
    """engine._TAPS_BY_CLASS / _CLASS_SLOT0 describe the same class-major order as kTapSlot: the j-th tap of class c sits in slot
    _CLASS_SLOT0[c] + j, the slots are a permutation of 0..8, and a tap's class is the parity of (kh + 1, kw + 1)"""
    seen = {}
    for c, (pt, pf, taps) in enumerate(_TAPS_BY_CLASS):
        for j, (kh, kw) in enumerate(taps):
            assert ((kh + 1) % 2, (kw + 1) % 2) == (pt, pf), "tap (%d, %d) is not of class (%d, %d)" % (kh, kw, pt, pf)
            assert K_TAP_SLOT[kh * 3 + kw] == _CLASS_SLOT0[c] + j, "tap (%d, %d): slot %d, table says %d" % (
                kh, kw, _CLASS_SLOT0[c] + j, K_TAP_SLOT[kh * 3 + kw])
            seen[kh * 3 + kw] = _CLASS_SLOT0[c] + j
    assert sorted(seen) == list(range(9)) and sorted(seen.values()) == list(range(9))


@pytest.mark.parametrize("F2", SIZES)
@pytest.mark.parametrize("T2", SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_conv2_maps_are_the_stride2_convolution(B, T2, F2):
    """Conv2d(3x3, stride 2, padding 1) over channels-last pixel rows: input rows (b*T2 + t2)*F2 + f2, output rows (t4*B + b)*F4 + f4
    (engine.py subsample_fwd): forward, per-tap weight gradient and the four class products of the data gradient"""
    mp = conv2_maps(B, T2, F2, "cpu")
    T4, F4 = mp["T4"], mp["F4"]
    assert (T4, F4) == ((T2 + 1) // 2, (F2 + 1) // 2)
    P1, P2 = B * T2 * F2, T4 * B * F4
    x = rnd64(P1, CI, seed=1)
    w = rnd64(CO, CI, 3, 3, seed=2)
    dy = rnd64(P2, CO, seed=3)
    xi = x.view(B, T2, F2, CI).permute(0, 3, 1, 2).clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    ref = F.conv2d(xi, wf, None, stride=2, padding=1)                  # [B, CO, T4, F4]
    assert ref.shape == (B, CO, T4, F4)
    ref.backward(dy.view(T4, B, F4, CO).permute(1, 3, 0, 2))
    fwd = mp["fwd"]
    assert fwd.dtype == torch.int32 and fwd.shape == (9, P2)
    assert int(fwd.min()) >= -1 and int(fwd.max()) < P1
    # forward: z = gather(x, fwd, Ci) @ w2p^T with the mode 0 layout w2p[co][tap*Ci + ci] = w[co][ci][tap]  (engine.py:365)
    w2p = w.reshape(CO, CI, 9).permute(0, 2, 1).reshape(CO, 9 * CI)
    z = gathered_a(x, fwd, CI) @ w2p.t()
    close(z, ref.detach().permute(2, 0, 3, 1).reshape(P2, CO), "forward")
    # weight gradient: gw2p[:, tap*Ci:(tap+1)*Ci] = dy^T @ x[fwd[tap]]  (engine.py:447), mode 2 back to [co][ci][tap]
    gw2p = torch.cat([dy.t() @ gathered_b(x, fwd[tap]) for tap in range(9)], dim=1)
    close(gw2p.view(CO, 9, CI).permute(0, 2, 1).reshape(CO, CI, 3, 3), wf.grad, "weight gradient")
    # data gradient: per parity class gather(dy, maps, Co) @ w2q[:, s0*Co:(s0+nt)*Co]^T scattered to `rows`  (engine.py:463) with the
    # mode 1 layout w2q[ci][slot(tap)*Co + co] = w[co][ci][tap]
    w2q = torch.zeros(CI, 9 * CO, dtype=torch.float64)
    for tap in range(9):
        w2q[:, K_TAP_SLOT[tap] * CO:(K_TAP_SLOT[tap] + 1) * CO] = w.reshape(CO, CI, 9)[:, :, tap].t()
    dx = torch.full((P1, CI), float("nan"), dtype=torch.float64)     # every input pixel must be written by exactly one class
    written = torch.zeros(P1, dtype=torch.int64)
    for c, (pt, pf, taps) in enumerate(_TAPS_BY_CLASS):
        n_rows = B * len(range(pt, T2, 2)) * len(range(pf, F2, 2))
        if n_rows == 0:
            assert mp["bwd"][c] is None, "an empty parity class must give None"
            continue
        rows, maps = mp["bwd"][c]
        assert rows.dtype == torch.int32 and maps.dtype == torch.int32
        assert rows.shape == (n_rows,) and maps.shape == (len(taps), n_rows)
        assert int(maps.min()) >= -1 and int(maps.max()) < P2
        s0, nt = _CLASS_SLOT0[c], len(taps)
        dx[rows.long()] = gathered_a(dy, maps, CO) @ w2q[:, s0 * CO:(s0 + nt) * CO].t()
        written[rows.long()] += 1
    assert bool((written == 1).all()), "the class rows do not partition the input pixels"
    close(dx, xi.grad.permute(0, 2, 3, 1).reshape(P1, CI), "data gradient")


@pytest.mark.parametrize("F4", SIZES)
@pytest.mark.parametrize("T4", SIZES)
@pytest.mark.parametrize("B", [1, 3])
def test_attn2d_maps_are_the_stride1_convolution(B, T4, F4):
    """3x3 / stride 1 / padding 1 over the pixel rows (t*B + b)*F4 + f (engine.py attn2d_block_fwd / _bwd): forward with
    w0[co][tap*Ci + ci] = w[co][ci][tap] (s2t_a2d_pack_w mode 0), per-tap weight gradient, and the data gradient through the SAME maps
    with mirrored taps w1[ci][tap*Co + co] = w[co][ci][8 - tap] (mode 1)"""
    mp = attn2d_maps(B, T4, F4, "cpu")
    M = T4 * B * F4
    assert mp.dtype == torch.int32 and mp.shape == (9, M) and int(mp.min()) >= -1 and int(mp.max()) < M
    x = rnd64(M, CI, seed=4)
    w = rnd64(CO, CI, 3, 3, seed=5)
    dy = rnd64(M, CO, seed=6)
    xi = x.view(T4, B, F4, CI).permute(1, 3, 0, 2).clone().requires_grad_(True)
    wf = w.clone().requires_grad_(True)
    ref = F.conv2d(xi, wf, None, padding=1)
    ref.backward(dy.view(T4, B, F4, CO).permute(1, 3, 0, 2))
    w9 = w.reshape(CO, CI, 9)
    w0 = w9.permute(0, 2, 1).reshape(CO, 9 * CI)
    close(gathered_a(x, mp, CI) @ w0.t(), ref.detach().permute(2, 0, 3, 1).reshape(M, CO), "forward")
    gp = torch.cat([dy.t() @ gathered_b(x, mp[tap]) for tap in range(9)], dim=1)
    close(gp.view(CO, 9, CI).permute(0, 2, 1).reshape(CO, CI, 3, 3), wf.grad, "weight gradient")
    w1 = w9.flip(2).permute(1, 2, 0).reshape(CI, 9 * CO)
    close(gathered_a(dy, mp, CO) @ w1.t(), xi.grad.permute(2, 0, 3, 1).reshape(M, CI), "data gradient")
