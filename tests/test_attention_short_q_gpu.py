"""The short-query attention kernels (csrc/attention.hip: attn_fwd_sq_kernel, attn_bwd_sq_kernel) against float64.

Route (sq_shape, attention.hip): bf16, d = 64, attn_v1 = 0, no distance penalty, Tq <= 64 and either Tq >= attn_v2_min_tq with
Tk >= 128 (the decoder's encoder-attention) or causal with Tq == Tk (its self-attention).  One workgroup owns all queries of a
(batch, head); the backward is one kernel that also makes Delta.  B = 2, H = 3 throughout: B H = 6 workgroups, not a multiple of 8.

Tools and bounds are those of tests/test_attention_modes_gpu.py (reference, check_fwd, check_bwd, check_adjoint: attn_check and
attn_dropout_adjoint of tests/test_routes_gpu.py with LSE added; copied, no test module imports another); nothing here has a
tolerance of its own.  Two uses of those bounds go beyond the originals:
  * Delta[b, h, i] = sum_c dO O is held to e_D = (d u + r) sum |dO O|, the error attn_check's docstring assigns to it;
  * with dropout the backward is also checked element by element: the mask M is known (s2t_dropout on drop_index's flat index
    space, as in test_dropout_mask_*), Pd = P M / (1 - p) replaces P in dV and in the weights of dP, and the same formulas bound
    the result -- the mask multiplies by an exact 0 or by a constant that rounds once (u, against the factor 2 of slack).
The mask itself is extracted from the forward (extract_mask) and must equal the first generation's (attn_v1 = 1) and
s2t_dropout's, the comparison test_dropout_mask_is_one_definition_across_kernels_and_s2t_dropout makes between generations.

Rows of dK / dV from klen[b] to Tk: attn_bwd_dkv_kernel stores `key < Tk` rows whose masked accumulators are zero,
attn_bwd_dkv2_kernel multiplies by kz = 0: both generations write exact zeros there, so the new kernel must too.
"""
import contextlib
import functools
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
U32 = 2.0 ** -24                 # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF = torch.bfloat16
FAMILIES = ("attn_fwd", "attn_bwd")
B, H, D_HEAD = 2, 3, 64
P_DROP = 0.1
SEED = 77


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    K.prof_enable(0)


# ------------------------------------------------------------------ shared tools (copies of test_attention_modes_gpu.py's)
@contextlib.contextmanager
def set_option(key, value):
    old = K.set_option(key, value)
    try:
        yield old
    finally:
        K.set_option(key, old)


@contextlib.contextmanager
def launches():
    counts = {}
    torch.cuda.synchronize()
    K.prof_reset()
    K.prof_enable(1)
    try:
        yield counts
    finally:
        torch.cuda.synchronize()
        for f in FAMILIES:
            r = K.prof_read(f)
            counts[f] = r["launches"]
            counts[f + "_flops"] = r["flops"]
        K.prof_enable(0)
        K.prof_reset()


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


def heads(t):
    """[T, B, H d] tensor -> float64 [B, H, T, d]"""
    T, Bn, D = t.shape
    return d64(t).reshape(T, Bn, H, D // H).permute(1, 2, 0, 3)


def allowed_pairs(Tq, Tk, klen, causal):
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool)
    if causal:
        ok = ok & ~torch.triu(torch.ones(Tq, Tk, dtype=torch.bool), 1)
    if klen is not None:
        ok = ok & (torch.arange(Tk)[None, :] < klen.cpu().long()[:, None])[:, None, None, :]
    return ok


def reference(q, k, v, klen, causal, pen=False):
    """float64 scores, P, LSE, the score error e_s and the LSE bound of test_attention_modes_gpu.py's docstring; pen: the distance
    penalty max(0, ln|i - j|) subtracted from the scaled scores, with that file's e_pen = 6 u max(1, ln|i - j|)"""
    Q, Kh, V = heads(q), heads(k), heads(v)
    Tq, Tk, d, scale = Q.shape[2], Kh.shape[2], D_HEAD, D_HEAD ** -0.5
    ok = allowed_pairs(Tq, Tk, klen, causal).expand(B, H, Tq, Tk)
    s = scale * Q @ Kh.transpose(-1, -2)
    e = 2 * d * U32 * scale * (Q.abs() @ Kh.abs().transpose(-1, -2))
    if pen:
        ln = (torch.arange(Tq)[:, None] - torch.arange(Tk)[None, :]).abs().double().clamp_min(1).log()
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
    return types.SimpleNamespace(Q=Q, K=Kh, V=V, P=P, es=es, lse=lse, bL=bL, ok=ok, Tq=Tq, Tk=Tk, d=d, scale=scale)


def o_bound(R):
    Oref = R.P @ R.V
    return Oref, 2 * (2 * R.es + UBF + (R.Tk + R.d) * U32) * (R.P @ R.V.abs()) + UBF * Oref.abs()


def check_fwd(R, o, lse, what):
    Oref, bO = o_bound(R)
    assert_close(heads(o), Oref, bO, what + " O")
    assert_close(lse.unsqueeze(-1), R.lse, R.bL, what + " LSE")


def check_bwd(R, o, do, delta, dq, dk, dv, what, keep=None, p=0.0):
    """Delta, dQ, dK, dV against float64 from the kernel's own O (check_bwd of test_attention_modes_gpu.py); keep = the dropout
    mask [B, H, Tq, Tk] of the call (module docstring)"""
    r = rp = UBF
    d, scale, Tq, Tk = R.d, R.scale, R.Tq, R.Tk
    P, es, V, Q, Kh = R.P, R.es, R.V, R.Q, R.K
    M = torch.ones_like(P) if keep is None else keep.double() / (1 - p)
    dO, O = heads(do), heads(o)
    Pd = P * M
    dVr = Pd.transpose(-1, -2) @ dO
    bV = 2 * (2 * es.amax(-2, keepdim=True) + rp + Tq * U32) * (Pd.transpose(-1, -2) @ dO.abs()) + r * dVr.abs()
    dP = (dO @ V.transpose(-1, -2)) * M
    Dl = (dO * O).sum(-1, keepdim=True)
    eD = (d * U32 + r) * (dO * O).abs().sum(-1, keepdim=True)
    assert_close(delta.unsqueeze(-1), Dl, eD, what + " Delta")
    dS = P * (dP - Dl)
    ep = 2 * d * U32 * (dO.abs() @ V.abs().transpose(-1, -2)) * M
    E = dS.abs() * (2 * es + 2 * rp) + P * (ep + eD)
    dQr = scale * dS @ Kh
    dKr = scale * dS.transpose(-1, -2) @ Q
    bQ = 2 * scale * (E @ Kh.abs() + (Tk * U32 + rp) * (dS.abs() @ Kh.abs())) + r * dQr.abs()
    bK = 2 * scale * (E.transpose(-1, -2) @ Q.abs() + (Tq * U32 + rp) * (dS.abs().transpose(-1, -2) @ Q.abs())) + r * dKr.abs()
    for name, got, ref, b in (("dV", dv, dVr, bV), ("dK", dk, dKr, bK), ("dQ", dq, dQr, bQ)):
        assert_close(heads(got), ref, b, what + " " + name)


def adjoint_z(R, do, o2, v2, dv, p):
    r = rp = UBF
    dO, O2, V2, dV = heads(do), heads(o2), heads(v2), heads(dv)
    P2e = R.P ** 2 / (1 - p) * (2 * R.es + rp) ** 2
    rO, rV = r + 4 * (R.Tk + R.d) * U32, r + 4 * (R.Tq + R.d) * U32
    lhs = (dO * O2).sum(-2)
    varO = P2e @ (V2 * V2) + (rO * O2) ** 2
    varV = P2e.transpose(-1, -2) @ (dO * dO) + (rV * dV) ** 2
    sd = ((dO * dO * varO).sum(-2) + (V2 * V2 * varV).sum(-2)).sqrt()
    return (lhs - (dV * V2).sum(-2)) / sd


def check_adjoint(R, do, o2, v2, dv_same, dv_other, p, what):
    z = adjoint_z(R, do, o2, v2, dv_same, p)
    i = int(z.abs().reshape(-1).argmax())
    assert float(z.abs().max()) <= 6, "%s: <dO, O(V2)> != <dV, V2> for (b, h, c) %s: z = %.3g" % (
        what, tuple(int(x) for x in torch.unravel_index(torch.tensor(i), z.shape)), float(z.reshape(-1)[i]))
    zw = adjoint_z(R, do, o2, v2, dv_other, p)
    rms = float((zw * zw).mean().sqrt())
    assert rms > 6, "%s: a backward with another dropout mask passes the check (rms z %.3g)" % (what, rms)


def expected_mask(Tq, Tk, p, seed):
    """s2t_dropout's keep decisions on the flat index space [B, H, Tq, Tk4] of drop_index, restricted to j < Tk"""
    Tk4 = (Tk + 3) & ~3
    ones = torch.ones(B, H, Tq, Tk4, dtype=torch.float32, device=DEV)
    return (K.dropout(ones, p, seed) != 0)[..., :Tk].cpu()


def extract_mask(Tq, Tk, p, seed, klen=None, causal=False):
    """keep[b, h, i, j] read off the forward's output: q = 0 makes every allowed probability positive, one-hot values V_g[j, c] =
    [j == g d + c] make O_g[i, c] non-zero exactly where pair (i, g d + c) was kept"""
    d, D = D_HEAD, H * D_HEAD
    q = torch.zeros(Tq, B, D, dtype=BF, device=DEV)
    k = torch.zeros(Tk, B, D, dtype=BF, device=DEV)
    kl = klen.to(DEV) if klen is not None else None
    keep = torch.zeros(B, H, Tq, Tk, dtype=torch.bool)
    for g in range((Tk + d - 1) // d):
        j = torch.arange(g * d, min(Tk, (g + 1) * d))
        v = torch.zeros(Tk, B, H, d, dtype=BF, device=DEV)
        v[j, :, :, j - g * d] = 1
        o, _ = K.attn_fwd(q, k, v.view(Tk, B, D), H, klen=kl, causal=causal, p_drop=p, seed=seed)
        keep[:, :, :, j] = (o.view(Tq, B, H, d)[..., :len(j)] != 0).permute(1, 2, 0, 3).cpu()
    return keep


# ------------------------------------------------------------------ one case on the device
def attn_bwd(q, k, v, o, do, lse, kl, causal, dist_penalty=False, p_drop=0.0, seed=0):
    """K.attn_bwd with the Delta buffer returned too (the wrapper allocates and drops it); outputs start as NaN so that an
    element the kernels do not write is seen"""
    Tq, Bn, D = q.shape
    Tk = k.shape[0]
    nan = lambda t: torch.full_like(t, math.nan, memory_format=torch.contiguous_format)  # noqa: E731
    dq, dk, dv = nan(q), nan(k), nan(v)
    delta = torch.full((Bn, H, Tq), math.nan, dtype=torch.float32, device=q.device)
    tb = lambda x: (x.stride(0), x.stride(1))  # noqa: E731
    rc = K._lib().s2t_attn_bwd(L.dt(q), D // H, Bn, H, Tq, Tk, L.ptr(q), *tb(q), L.ptr(k), *tb(k), L.ptr(v), *tb(v),
                               L.ptr(o), *tb(o), L.ptr(do), *tb(do), L.ptr(lse), L.ptr(delta),
                               L.ptr(dq), *tb(dq), L.ptr(dk), *tb(dk), L.ptr(dv), *tb(dv),
                               L.ptr(kl), int(causal), int(dist_penalty), float((D // H) ** -0.5), float(p_drop), int(seed), L.stream())
    L.check(rc, "s2t_attn_bwd")
    return delta, dq, dk, dv


@functools.lru_cache(maxsize=None)
def case_inputs(Tq, Tk, ragged, causal, pen=False):
    """q, k, v as slices of one fused [T, B, 3 H d] buffer (the layout the engine passes), dO, V2, klen and the float64 reference:
    made once per shape, shared by the tests, never modified"""
    D = H * D_HEAD
    g = torch.Generator().manual_seed(Tq * 7 + Tk)
    qkv = (torch.randn(max(Tq, Tk), B, 3 * D, generator=g) * 0.7).to(BF).to(DEV)
    do = torch.randn(Tq, B, D, generator=g).to(BF).to(DEV)
    v2 = (torch.randn(Tk, B, D, generator=g) * 0.7).to(BF).to(DEV)
    q, k, v = qkv[:Tq, :, :D], qkv[:Tk, :, D:2 * D], qkv[:Tk, :, 2 * D:]
    # ragged: one sentence shorter than a 64-key tile with a length that is no multiple of 4, the other 3 short of Tk
    klen = torch.tensor([min(37, Tk - 1), Tk - 3], dtype=torch.int32) if ragged else None
    return q, k, v, do, v2, klen, reference(q, k, v, klen, causal, pen)


def bwd_flop_factor(c, Tq, Tk, causal):
    """the backward's issued-FLOP count per B H Tq Tk d (halved when causal): s2t_attn_bwd reports 10 on the one-pass short-query
    route (S and dP made once) and 14 on the two-kernel routes -- the library's only witness of WHICH backward ran"""
    return c["attn_bwd_flops"] / (B * H * Tq * Tk * D_HEAD * (0.5 if causal else 1.0))


def run_case(Tq, Tk, ragged, causal, p, what, dist_penalty=False, sq=True, seed=SEED):
    """one forward + backward against float64; sq: whether the backward must have taken the short-query route"""
    q, k, v, do, v2, klen, R = case_inputs(Tq, Tk, ragged, causal, dist_penalty)
    kl = klen.to(DEV) if klen is not None else None
    kw = dict(klen=kl, causal=causal, dist_penalty=dist_penalty)
    if p == 0:
        with launches() as c:
            o, lse = K.attn_fwd(q, k, v, H, **kw)
            delta, dq, dk, dv = attn_bwd(q, k, v, o, do, lse, kl, causal, dist_penalty)
        check_fwd(R, o, lse, what)
        check_bwd(R, o, do, delta, dq, dk, dv, what)
        if dist_penalty:                                     # the bound sees the penalty: the unpenalised reference must miss it
            Oref0, bO0 = o_bound(case_inputs(Tq, Tk, ragged, causal, False)[6])
            assert bool(((heads(o) - Oref0).abs() > bO0).any()), what + ": outputs with the penalty pass the unpenalised O bound"
    else:
        o, lse = K.attn_fwd(q, k, v, H, p_drop=p, seed=seed, **kw)
        o2, lse2 = K.attn_fwd(q, k, v2, H, p_drop=p, seed=seed, **kw)
        assert_close(lse.unsqueeze(-1), R.lse, R.bL, what + " LSE with dropout")
        assert_close(lse2.unsqueeze(-1), R.lse, R.bL, what + " LSE with dropout (V2)")
        with launches() as c:
            K.attn_fwd(q, k, v, H, p_drop=p, seed=seed, **kw)
            delta, dq, dk, dv = attn_bwd(q, k, v, o, do, lse, kl, causal, dist_penalty, p, seed)
        dv_other = attn_bwd(q, k, v, o, do, lse, kl, causal, dist_penalty, p, seed + 1)[3]
        check_adjoint(R, do, o2, v2, dv, dv_other, p, what)
        keep = expected_mask(Tq, Tk, p, seed)
        check_bwd(R, o, do, delta, dq, dk, dv, what + " p=%.1f" % p, keep, p)
    assert c["attn_fwd"] == 1 and c["attn_bwd"] == 1, c
    f = bwd_flop_factor(c, Tq, Tk, causal)
    assert abs(f - (10 if sq else 14)) < 1e-6, "%s: the backward reports %.3f B H Tq Tk d FLOPs: %s route expected" % (
        what, f, "the short-query" if sq else "a two-kernel")
    # determinism: the same call again, bit for bit
    again = attn_bwd(q, k, v, o, do, lse, kl, causal, dist_penalty, p, seed)
    for name, a, b_ in zip(("Delta", "dQ", "dK", "dV"), (delta, dq, dk, dv), again):
        assert torch.equal(a, b_), what + ": two runs of the backward differ in " + name
    # rows of dK / dV from klen[b] to Tk are written, as exact zeros (module docstring)
    if klen is not None:
        for b in range(B):
            for name, t in (("dK", dk), ("dV", dv)):
                tail = t[int(klen[b]):, b]
                assert bool((tail == 0).all()), "%s: %s rows past klen[%d] = %d are not exact zeros" % (what, name, b, int(klen[b]))


# ------------------------------------------------------------------ the cases of the route
@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("Tk", [128, 131, 368])
@pytest.mark.parametrize("Tq", [16, 17, 40, 48, 64])
def test_cross_attention(Tq, Tk, ragged, p):
    """encoder-attention shapes: 1 to 4 query blocks of 16 with and without padding rows, key counts that are a multiple of the
    64-key tile, 3 past it and the decoder's 368 (5 tiles and 48 keys); ragged: klen 37 (less than a tile, no multiple of 4) and
    Tk - 3 (128 at Tk 131: the last tile is padding only).  O, LSE, Delta, dQ, dK, dV; the adjoint identity with dropout"""
    run_case(Tq, Tk, ragged, False, p, "cross Tq%d Tk%d%s p=%.1f" % (Tq, Tk, " ragged" if ragged else "", p))


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("T", [17, 40, 64])
def test_causal_self_attention(T, p):
    """decoder self-attention: Tq == Tk <= 64, one key tile, the causal triangle"""
    run_case(T, T, False, True, p, "self T%d p=%.1f" % (T, p))


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("case", [(40, 131, False), (40, 131, True), (40, 40, True), (64, 368, True)],
                         ids=lambda c: "Tq%d_Tk%d%s" % (c[0], c[1], "_ragged" if c[2] else ""))
def test_causal_with_more_keys_than_queries_and_ragged_keys(case, p):
    """sq_shape also takes causal calls with Tq < Tk (Tk >= 128) and causal calls with ragged keys: the key loop ends at
    min(klen, Tq), every key past it -- above the diagonal or padding -- gets zero dK / dV rows (whole tiles by the tail loop)"""
    Tq, Tk, ragged = case
    run_case(Tq, Tk, ragged, True, p, "causal Tq%d Tk%d%s p=%.1f" % (Tq, Tk, " ragged" if ragged else "", p))


@pytest.mark.parametrize("p", [0.0, P_DROP], ids=["p0", "p0.1"])
@pytest.mark.parametrize("edge", ["Tq65", "Tk127", "dist_pen", "attn_v1"])
def test_route_edges(edge, p):
    """just outside the route (sq_shape): 65 queries and the distance penalty stay with the second generation, 127 keys and
    attn_v1 = 1 with the first (the backward reports 14 B H Tq Tk d FLOPs, not 10); whatever runs meets the same bounds -- the
    penalised call against the penalised float64 reference, which the unpenalised one must miss (the short-query kernels ignore
    dist_pen: a call that reached them would give the unpenalised result)"""
    if edge == "Tq65":
        run_case(65, 131, True, False, p, "edge Tq65 p=%.1f" % p, sq=False)
    elif edge == "Tk127":
        run_case(40, 127, True, False, p, "edge Tk127 p=%.1f" % p, sq=False)
    elif edge == "attn_v1":
        with set_option("attn_v1", 1):
            run_case(40, 131, True, False, p, "edge attn_v1 p=%.1f" % p, sq=False)
    else:
        run_case(40, 131, True, False, p, "edge dist_pen p=%.1f" % p, dist_penalty=True, sq=False)


MASK_CASES = [(40, 368, True, False), (17, 131, False, False), (64, 128, True, False), (40, 40, False, True), (17, 17, False, True)]


@pytest.mark.parametrize("case", MASK_CASES, ids=lambda c: "Tq%d_Tk%d%s%s" % (c[0], c[1], "_ragged" if c[2] else "", "_causal" if c[3] else ""))
def test_dropout_mask_is_the_first_generations_and_s2t_dropouts(case):
    """the extracted mask of attn_fwd_sq_kernel equals the one of attn_fwd_kernel (attn_v1 = 1) and s2t_dropout's on the allowed
    pairs; without dropout every allowed pair is visible.  (The backward's use of the same mask: the adjoint identity and the
    element-wise dropout backward of the cases above.)"""
    Tq, Tk, ragged, causal = case
    klen = torch.tensor([min(37, Tk - 1), Tk - 3], dtype=torch.int32) if ragged else None
    ok = allowed_pairs(Tq, Tk, klen, causal).expand(B, H, Tq, Tk)
    assert bool((extract_mask(Tq, Tk, 0.0, SEED, klen, causal) == ok).all()), "without dropout every allowed pair must be visible"
    want = expected_mask(Tq, Tk, P_DROP, SEED) & ok
    new = extract_mask(Tq, Tk, P_DROP, SEED, klen, causal)
    with set_option("attn_v1", 1):
        old = extract_mask(Tq, Tk, P_DROP, SEED, klen, causal)
    assert bool((new == old).all()), "short-query and first-generation masks differ in %d pairs" % int((new != old).sum())
    assert bool((new == want).all()), "%d pairs differ from s2t_dropout's mask" % int((new != want).sum())


HIGH_SEED = (5 << 32) | 7          # the seed is a 64-bit argument: its upper word must reach the hash


@pytest.mark.parametrize("case", [(17, 131, False, False), (17, 17, False, True)], ids=["Tq17_Tk131", "Tq17_Tk17_causal"])
def test_dropout_mask_and_backward_at_a_seed_above_32_bits(case):
    """the two smallest mask cases at a seed whose upper word is set: attn_fwd_sq_kernel's extracted mask is s2t_dropout's at that seed
    and not its low word's, and the one-pass backward drops the same pairs (run_case: element-wise against float64 with that mask)"""
    Tq, Tk, ragged, causal = case
    ok = allowed_pairs(Tq, Tk, None, causal).expand(B, H, Tq, Tk)
    want = expected_mask(Tq, Tk, P_DROP, HIGH_SEED) & ok
    new = extract_mask(Tq, Tk, P_DROP, HIGH_SEED, None, causal)
    assert bool((new == want).all()), "%d pairs differ from s2t_dropout's mask" % int((new != want).sum())
    assert not bool((new == (expected_mask(Tq, Tk, P_DROP, HIGH_SEED & 0xFFFFFFFF) & ok)).all()), "the seed's upper word does not reach the mask"
    run_case(Tq, Tk, ragged, causal, P_DROP, "64-bit seed Tq%d Tk%d" % (Tq, Tk), seed=HIGH_SEED)


def test_attn_v2_min_tq_above_tq_leaves_the_route():
    """attn_v2_min_tq = 64 sends a Tq = 40 cross-attention block to the first generation, as before (14 B H Tq Tk d backward FLOPs
    against the route's 10); both settings meet the bounds"""
    for val in (16, 64):
        with set_option("attn_v2_min_tq", val):
            run_case(40, 131, True, False, 0.0, "attn_v2_min_tq=%d" % val, sq=val == 16)
