"""Both CTC loss routes of csrc/ctc.hip, every gradient element against float64, at the edges of the kernels.

s2t_ctc_loss (the recursion in one wave's registers at 1, 2, 4, 8 or 16 positions per lane, one f32 vocabulary row in LDS) and
s2t_ctc_loss_any (state in the workspace, fixed-point posteriors) are called directly, so that the test owns the row stride, the
gradient buffer, loss_sum, both scales and the phase.  Logits are generated in the compute dtype and tests/ctc_ref.py sees exactly
those values in float64.  The gradient buffer [T, B, ld] is prefilled with a NaN sentinel and loss_sum starts at 5.0.  Checked:

  * every live element:   |g - gs g_ref| <= gs (a(Tb) occ_ref + 2^-18 softmax_ref + 2^-22) + r gs |g_ref|,
    gs = |grad_scale upstream|, r = 2^-24 (f32) / 2^-8 (bf16), a(Tb) = 4 ln 2 (Tb 2^-19 + 2^-15)      (derivation, and why the
    coefficient is 4 and not 1: tests/ctc_ref.py; tests/test_ctc_ref_cpu.py shows that f32 arithmetic can meet the bound and that
    five plausible kernel bugs cannot);
  * every other element of a row (frames past in_len, utterances without an alignment) is exactly 0;
  * every column in [V, ld) still holds the sentinel;
  * nll per utterance: |nll - ref| <= a(Tb) + 2^-23 |ref| where the reference is finite, +inf elsewhere;
  * loss_sum = 5 + the finite nll, within the sum of those bounds plus (B + 1) 2^-24 (5 + sum |ref|).

Case groups: A lane-width borders of the fixed route (the last state in the wave's last occupied lane), B frame counts around
the emission chunks and the every-fourth-step shift at every lane width, C vocabulary sizes around the 256-thread stride, the 16-byte
vector loop and its tail, the 64 KiB dynamic-LDS switch and the largest fixed-route vocabulary, with padded, padded + 24 and dense
(unaligned: the scalar loop) rows and three blank positions, D the same through s2t_ctc_loss_any plus more states than threads, a
vocabulary beyond the fixed route and a transcript that needs the gradient pass's second sweep, E extreme values, F scales and
phases, G refusals.

Worst |err| / bound per group and dtype measured on an MI355X (gradient, nll; `pytest -s` prints them; the file took 7.2 s):
  A  f32 0.167 0.033   bf16 0.992 0.033        D  f32 0.166 0.314   bf16 0.993 0.076        E  f32 0.681 0.205   bf16 0.963 0.225
  B  f32 0.139 0.076   bf16 0.992 0.153        D2 f32 0.359 0.571   (the 4,096-unit cases)   F  f32 0.101 0.029   bf16 0.959 0.019
  C  f32 0.151 0.070   bf16 0.977 0.076
bf16 gradients sit just below 1 by construction: round to nearest uses up to all of r |g_ref| at the bottom of a binade.  At
coefficient 1 the same kernels measured 2.55 (E, transcript columns lowered by 80, both routes to the same bits) and 1.43 (D2):
f32 rounding of states far below the vector's maximum, which tests/ctc_ref.py's own float32 run shows too (1.9 and 1.2).  No
kernel bug was found.
"""
import math
import types

import numpy as np
import pytest
import torch

import ctc_ref as R

pytestmark = pytest.mark.gpu

K = L = None
DEV = "cuda"
U32 = 2.0 ** -24                 # unit roundoff of f32
UBF = 2.0 ** -8                  # unit roundoff of bf16 (round to nearest)
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
ROUTES = ["fixed", "any"]
EINVAL, ENOTSUP = -22, -95
SENTINEL = {BF: (torch.int16, 0x7FC1), F32: (torch.int32, 0x7FC00001)}       # NaNs with a payload no kernel produces
LOSS0 = 5.0
WORST = {}                       # group and dtype -> [worst gradient |err| / bound, worst nll |err| / bound]
_CACHE = {}                      # (builder, args) -> (case, reference): shared by the routes and tests that use the same case


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    _CACHE.clear()
    if WORST:
        print("\nworst |err| / bound per group and dtype (gradient, nll): " + ", ".join("%s %.3g %.3g" % (k, v[0], v[1]) for k, v in sorted(WORST.items())))


# ------------------------------------------------------------------ shared tools
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


def ctc_row(Lmax):
    """S2T_CTC_ROW(Lmax) of include/s2t_hip.h: the row stride of the fixed route's la / lb workspaces"""
    return next(r for r in (64, 128, 256, 512, 1024) if 2 * Lmax + 1 <= r)


def make_ld(kind, V, dtype):
    return {"pad": K.padded_cols(V, dtype), "dense": V, "pad+24": K.padded_cols(V, dtype) + 24}[kind]


def pick_units(g, n, V, blank, repeat_at=()):
    """n units != blank, no two neighbours equal except at the positions of repeat_at (a vocabulary of one unit repeats everywhere)"""
    out = np.zeros(n, dtype=np.int64)
    prev = -1
    for i in range(n):
        j = int(g.integers(0, V - 1))
        if i > 0 and i in repeat_at:
            j = prev
        elif j == prev and V > 2:
            j = (j + 1 + int(g.integers(0, V - 2))) % (V - 1)
        out[i] = prev = j
    return out + (out >= blank)


def make_case(T, V, Lmax, blank, tl, il, tgt, logits, ld):
    return types.SimpleNamespace(T=T, B=len(tl), V=V, Lmax=Lmax, blank=blank, tl=[int(v) for v in tl], il=[int(v) for v in il],
                                 tgt=torch.as_tensor(np.asarray(tgt), dtype=torch.int64).reshape(len(tl), Lmax), logits=logits, ld=ld)


def randn(g, shape, dtype, scale):
    return (torch.from_numpy(g.standard_normal(shape)) * scale).to(dtype)


def reference(c):
    """float64 reference of the case's exact logits: nll, occ, softmax, gradient (numpy)"""
    nll, occ, sm = R.ctc_forward_backward(c.logits.double().numpy(), c.tgt.numpy(), c.il, c.tl, c.blank)
    return types.SimpleNamespace(nll=nll, occ=occ, sm=sm, g=R.gradient(nll, occ, sm, c.il))


def cached(builder, *args):
    key = (builder.__name__,) + args
    if key not in _CACHE:
        c = builder(*args)
        _CACHE[key] = (c, reference(c))
    return _CACHE[key]


def run(route, c, dtype, grad_scale=1.0, upstream=None, phase=0, state=None, lse=None, ld_arg=None):
    """one call of s2t_ctc_loss / s2t_ctc_loss_any.  The logits live in a [T, B, ld] buffer whose padding columns hold 50.0 (a kernel
    that read them as part of the row would shift every softmax); the gradient buffer is all sentinel, loss_sum starts at LOSS0.
    `state` (of an earlier call) reuses that call's device buffers and workspaces: phase 2 after phase 1."""
    lib = K._lib()
    T, B, V, ld, Lmax = c.T, c.B, c.V, c.ld, c.Lmax
    if state is None:
        x = torch.full((T, B, ld), 50.0, dtype=dtype)
        x[..., :V] = c.logits
        st = types.SimpleNamespace(x=x.to(DEV), tgt=c.tgt.to(DEV), tl=torch.tensor(c.tl, dtype=torch.int64, device=DEV),
                                   il=torch.tensor(c.il, dtype=torch.int32, device=DEV),
                                   lse=lse if lse is not None else torch.full((T * B,), math.nan, dtype=F32, device=DEV),
                                   nll=torch.full((B,), math.nan, dtype=F32, device=DEV))
        if route == "fixed":
            st.la = torch.empty((B * T * ctc_row(min(Lmax, 511)),), dtype=F32, device=DEV)
            st.lb = torch.empty_like(st.la)
        else:
            nbytes = lib.s2t_ctc_loss_any_workspace(T, B, Lmax, V)
            assert nbytes == 4 * (2 * B * T * ((2 * Lmax + 1 + 63) // 64 * 64) + B * ((Lmax + 1 + 63) // 64 * 64))
            st.ws = torch.empty(((nbytes + 3) // 4,), dtype=F32, device=DEV)
    else:
        st = state
    it, bits = SENTINEL[dtype]
    grad = torch.full((T, B, ld), bits, dtype=it, device=DEV).view(dtype) if (phase & 3) != 1 else None
    loss = torch.full((1,), LOSS0, dtype=F32, device=DEV) if (phase & 3) != 2 else None
    up = None if upstream is None else torch.full((1,), upstream, dtype=F32, device=DEV)
    tail = (T, B, V, ld if ld_arg is None else ld_arg, Lmax, c.blank, float(grad_scale), phase, L.ptr(up), L.stream())
    if route == "fixed":
        rc = lib.s2t_ctc_loss(L.dt(st.x), L.ptr(st.x), L.ptr(st.tgt), L.ptr(st.tl), L.ptr(st.il), L.ptr(st.lse), L.ptr(st.la), L.ptr(st.lb),
                              L.ptr(st.nll), L.ptr(grad), L.ptr(loss), *tail)
    else:
        rc = lib.s2t_ctc_loss_any(L.dt(st.x), L.ptr(st.x), L.ptr(st.tgt), L.ptr(st.tl), L.ptr(st.il), L.ptr(st.lse), L.ptr(st.ws),
                                  L.ptr(st.nll), L.ptr(grad), L.ptr(loss), *tail)
    torch.cuda.synchronize()
    return types.SimpleNamespace(rc=rc, grad=None if grad is None else grad.cpu(), nll=st.nll.cpu(), state=st,
                                 loss=None if loss is None else float(loss))


def argmax_lse(c, dtype):
    """the rows' log-sum-exps as s2t_ctc_argmax writes them, for phase | 4"""
    x = torch.full((c.T, c.B, c.ld), 50.0, dtype=dtype)
    x[..., :c.V] = c.logits
    x = x.to(DEV)
    pred = torch.empty((c.B, c.T), dtype=torch.int32, device=DEV)
    pmax = torch.empty((c.B, c.T), dtype=F32, device=DEV)
    lse = torch.empty((c.T * c.B,), dtype=F32, device=DEV)
    assert K._lib().s2t_ctc_argmax(L.dt(x), L.ptr(x), L.ptr(pred), L.ptr(pmax), L.ptr(lse), c.T, c.B, c.V, c.ld, L.stream()) == 0
    return lse


def untouched(grad, dtype):
    it, bits = SENTINEL[dtype]
    return bool((grad.view(it) == bits).all())


def check(c, ref, res, dtype, group, what, scale=1.0):
    """the module docstring's checks of one call's results (gradient if the call produced one, nll and loss_sum if it ran the forward)"""
    assert res.rc == 0, "%s: return code %d" % (what, res.rc)
    w = WORST.setdefault("%s %s" % (group, name(dtype)), [0.0, 0.0])
    live = R.live_mask(ref.nll, c.il, c.T)
    assert live.any()
    if res.grad is not None:
        gs = abs(scale)
        assert untouched(res.grad[..., c.V:], dtype), "%s: a column in [V, ld) was written" % what
        bound = R.grad_bound(ref.occ, ref.sm, ref.g, c.il, gs, UBF if dtype == BF else U32) * live[:, :, None]     # 0 off the live rows
        want = torch.from_numpy(scale * ref.g)
        got = res.grad[..., :c.V]
        err = (d64(got) - want).abs().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(live[:, :, None] & (err > 0), err / bound, 0.0)
        if np.isfinite(ratio).all():
            w[0] = max(w[0], float(ratio.max()))
        dead = d64(got)[torch.from_numpy(~live)]
        assert bool((dead == 0).all()), "%s: %d elements of rows without a gradient are not 0" % (what, int((dead != 0).sum()))
        assert_close(got, want, torch.from_numpy(bound), what + " gradient")
    fin = np.isfinite(ref.nll)
    nll = res.nll.double().numpy()
    assert np.all(nll[~fin] == math.inf), "%s: nll %s where no alignment exists" % (what, nll[~fin])
    nb = R.nll_bound(ref.nll, c.il, c.T)
    if fin.any():
        w[1] = max(w[1], float((np.abs(nll[fin] - ref.nll[fin]) / nb[fin]).max()))
    assert_close(torch.from_numpy(nll[fin]), torch.from_numpy(ref.nll[fin]), torch.from_numpy(nb[fin]), what + " nll")
    if res.loss is not None:
        tot = float(ref.nll[fin].sum())
        lb = float(nb[fin].sum()) + (c.B + 1) * U32 * (LOSS0 + float(np.abs(ref.nll[fin]).sum()))
        assert abs(res.loss - (LOSS0 + tot)) <= lb, "%s: loss_sum %.9g, reference %.9g, bound %.3g" % (what, res.loss, LOSS0 + tot, lb)


def bits_equal(a, b):
    return a.dtype == b.dtype and bool((a.view(SENTINEL[a.dtype][0]) == b.view(SENTINEL[b.dtype][0])).all())


# ------------------------------------------------------------------ case builders
def case_a(Lmax, dtype):
    """lane-width borders: the full width, one unit less, a run of one unit (a blank between every two), an empty transcript"""
    V, blank = 21, 20
    T = 2 * Lmax + 8
    g = np.random.default_rng(1000 + Lmax)
    tl = [Lmax, max(Lmax - 1, 0), (Lmax + 1) // 2, 0]
    il = [T, T - 1, T - 3, 5]
    tgt = np.stack([pick_units(g, Lmax, V, blank, repeat_at=(3, Lmax - 1)), pick_units(g, Lmax, V, blank, repeat_at=(1,)),
                    np.full(Lmax, 7), pick_units(g, Lmax, V, blank)])
    return make_case(T, V, Lmax, blank, tl, il, tgt, randn(g, (T, 4, V), dtype, 2.0), K.padded_cols(V, dtype))


def chunk_frames(Lmax):
    """CTC_CH of ctc_alphabeta_kernel: frames of emissions staged per chunk at this transcript width"""
    return 16 if 2 * Lmax + 1 <= 256 else (8 if 2 * Lmax + 1 <= 512 else 4)


def case_b(Lmax, dtype):
    """frame counts around the chunk and the every-fourth-step shift, with transcripts of 0 to 3 units; one that cannot fit, one
    without frames, one of full width over all frames"""
    V, blank = 21, 20
    T = Lmax + 10
    ch = chunk_frames(Lmax)
    g = np.random.default_rng(2000 + Lmax)
    il = sorted({0, 1, 2, 3, 4, 5, ch - 1, ch, ch + 1, 2 * ch, 2 * ch + 1, 2 * ch + 3, T, T + 5})
    tl = [i % 4 for i in range(len(il))]
    il += [2, 0, T]
    tl += [3, 2, Lmax]
    tgt = np.stack([pick_units(g, Lmax, V, blank, repeat_at=(2,) if b == len(tl) - 1 else ()) for b in range(len(tl))])
    return make_case(T, V, Lmax, blank, tl, il, tgt, randn(g, (T, len(tl), V), dtype, 2.0), K.padded_cols(V, dtype))


def case_c(V, ldkind, blank, dtype):
    """T = 9, B = 3, Lmax = 4; the transcripts use the first and last columns, the columns either side of the 256-thread stride and
    the first column of the vector loop's tail"""
    T, Lmax = 9, 4
    g = np.random.default_rng(3000 + V)
    edge = [c for c in dict.fromkeys([0, V - 1, V - V % 8, V - V % 8 - 1, 255, 256, V // 2, 1]) if 0 <= c < V and c != blank]
    row0 = [edge[i % len(edge)] for i in range(4)]
    row1 = [edge[(i // 2 + 2) % len(edge)] for i in range(4)]          # pairs of equal units
    tgt = np.array([row0, row1, row0])
    return make_case(T, V, Lmax, blank, [4, 3, 0], [9, 8, 5], tgt, randn(g, (T, 3, V), dtype, 2.0), make_ld(ldkind, V, dtype))


def case_long(Lmax, dtype):
    """more states than the recursion's 1,024 threads: T = Lmax + 20 leaves room for twenty repeats"""
    V, blank = 21, 20
    T = Lmax + 20
    g = np.random.default_rng(4000 + Lmax)
    tgt = np.stack([pick_units(g, Lmax, V, blank, repeat_at=(5, 600, Lmax - 1)), np.full(Lmax, 3), pick_units(g, Lmax, V, blank)])
    return make_case(T, V, Lmax, blank, [Lmax, Lmax // 2, 0], [T, T - 2, 7], tgt, randn(g, (T, 3, V), dtype, 2.0), K.padded_cols(V, dtype))


def case_sweep(V):
    """a transcript of 4,096 units: label 4,096 (the last unit) falls into the second sweep of ctc_grad_any_kernel's 4,096 LDS
    slots.  Units cycle through 0 .. 10, no two neighbours equal.  V = 12: every unit has occurred within the first sweep (the
    second then finds only repeats); V = 13: the last unit of utterance 1 is unit 11, which occurs nowhere else, so the second sweep
    owns a column (that case has only this utterance: the reference takes 2.5 s per utterance here)."""
    T, Lmax, blank = 4200, 4096, V - 1
    g = np.random.default_rng(5000 + V)
    row = np.arange(Lmax) % 11
    if V == 13:
        row[Lmax - 1] = 11
        return make_case(T, V, Lmax, blank, [4096], [T - 3], [row], randn(g, (T, 1, V), F32, 2.0), K.padded_cols(V, F32))
    return make_case(T, V, Lmax, blank, [4095, 4096], [T, T - 3], [row, row], randn(g, (T, 2, V), F32, 2.0), K.padded_cols(V, F32))


def case_e(kind, dtype):
    T, V, Lmax, blank = 40, 21, 12, 20
    g = np.random.default_rng(6000)
    tl, il = [12, 7, 0], [40, 33, 20]
    tgt = np.stack([pick_units(g, Lmax, 16, 15, repeat_at=(4,)) for _ in range(3)])      # units 0 .. 14: 17 is in no transcript
    x = g.standard_normal((T, 3, V)) * (8.0 if kind == "scale8" else 2.0)
    if kind in ("peak_right", "peak_wrong"):
        for b in range(3):
            ext, _ = R.extended_target(tgt[b][: tl[b]], blank)
            for t in range(il[b]):
                x[t, b, ext[min(len(ext) - 1, t * len(ext) // il[b])] if kind == "peak_right" else 17] += 30.0
    elif kind == "lowered":
        for b in range(3):
            x[:, b, np.unique(tgt[b][: tl[b]])] -= 80.0
    elif kind == "equal_logits":
        x[:] = 1.5
    elif kind == "equal_units":
        tgt[:] = 3
    return make_case(T, V, Lmax, blank, tl, il, tgt, torch.from_numpy(x).to(dtype), K.padded_cols(V, dtype))


def case_f(dtype):
    T, V, Lmax, blank = 20, 21, 6, 20
    g = np.random.default_rng(7000)
    tgt = np.stack([pick_units(g, Lmax, V, blank, repeat_at=(2,)), pick_units(g, Lmax, V, blank), np.full(Lmax, 5), pick_units(g, Lmax, V, blank)])
    return make_case(T, V, Lmax, blank, [6, 3, 6, 0], [20, 13, 9, 17], tgt, randn(g, (T, 4, V), dtype, 2.0), K.padded_cols(V, dtype))   # utterance 2: 6 equal units need 11 frames


def name(dtype):
    return "bf16" if dtype == BF else "f32"


# ------------------------------------------------------------------ A: lane-width borders, fixed route
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Lmax", [1, 31, 32, 63, 64, 127, 128, 255, 256, 511])
def test_a_lane_width_borders(Lmax, dtype):
    c, ref = cached(case_a, Lmax, dtype)
    assert np.isfinite(ref.nll).all()
    check(c, ref, run("fixed", c, dtype), dtype, "A", "Lmax %d %s" % (Lmax, name(dtype)))


# ------------------------------------------------------------------ B: frame edges at every width
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Lmax", [5, 40, 100, 200, 300])
def test_b_frame_edges(Lmax, dtype):
    c, ref = cached(case_b, Lmax, dtype)
    fin = np.isfinite(ref.nll)
    assert not fin[-3] and not fin[-2] and fin[-1] and not fin[0] and fin[4]      # cannot fit, no frames, full width, in_len 0, in_len 4
    check(c, ref, run("fixed", c, dtype), dtype, "B", "Lmax %d %s" % (Lmax, name(dtype)))


# ------------------------------------------------------------------ C: vocabulary and stride, fixed route
C_CASES = [(2, "dense", 0), (2, "pad", 1), (7, "pad", 3), (7, "dense", 6), (8, "pad+24", 4), (9, "dense", 0), (255, "pad", 127),
           (255, "dense", 254), (256, "pad+24", 0), (257, "dense", 128), (257, "pad", 256), (1031, "pad+24", 515), (5001, "pad", 5000),
           (5001, "dense", 0), (16384, "pad", 8192), (16385, "pad", 16384), (16385, "dense", 0), (20011, "pad+24", 10005),
           (40704, "pad", 40703), (40704, "pad+24", 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("V,ldkind,blank", C_CASES)
def test_c_vocabulary_and_stride(V, ldkind, blank, dtype):
    c = case_c(V, ldkind, blank, dtype)
    esize = 2 if dtype == BF else 4
    assert ((c.ld * esize) % 16 != 0) == (ldkind == "dense")            # dense rows are unaligned (the scalar loop), the others take the vector loop
    check(c, reference(c), run("fixed", c, dtype), dtype, "C", "V %d ld %d blank %d %s" % (V, c.ld, blank, name(dtype)))


# ------------------------------------------------------------------ D: the `any` route
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Lmax", [1, 32, 511])
def test_d_any_lane_width_cases(Lmax, dtype):
    c, ref = cached(case_a, Lmax, dtype)
    check(c, ref, run("any", c, dtype), dtype, "D", "any, A Lmax %d %s" % (Lmax, name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_d_any_frame_edges(dtype):
    c, ref = cached(case_b, 5, dtype)
    check(c, ref, run("any", c, dtype), dtype, "D", "any, B Lmax 5 %s" % name(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("Lmax", [512, 1500])
def test_d_any_more_states_than_threads(Lmax, dtype):
    c = case_long(Lmax, dtype)
    check(c, reference(c), run("any", c, dtype), dtype, "D", "any, Lmax %d %s" % (Lmax, name(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_d_any_vocabulary_beyond_the_fixed_route(dtype):
    c = case_c(40705, "pad", 40704, dtype)
    check(c, reference(c), run("any", c, dtype), dtype, "D", "any, V 40705 %s" % name(dtype))


@pytest.mark.parametrize("V", [12, 13])
def test_d_any_second_sweep(V):
    c = case_sweep(V)
    ref = reference(c)
    assert np.isfinite(ref.nll).all()
    if V == 13:
        assert float(ref.occ[:, 0, 11].sum()) >= 1.0 - 1e-9                                      # the second sweep's own column
    check(c, ref, run("any", c, F32), F32, "D2", "any, 4,096 units, V %d" % V)


# ------------------------------------------------------------------ E: values
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", ["scale8", "peak_right", "peak_wrong", "lowered", "equal_logits", "equal_units"])
def test_e_values(kind, route, dtype):
    c, ref = cached(case_e, kind, dtype)
    assert np.isfinite(ref.nll).all()
    if kind == "lowered":
        assert ref.nll[0] > 1000.0
    check(c, ref, run(route, c, dtype), dtype, "E", "%s %s %s" % (kind, route, name(dtype)))


# ------------------------------------------------------------------ F: scales and phases
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("route", ROUTES)
def test_f_scales(route, dtype):
    c, ref = cached(case_f, dtype)
    assert list(np.isfinite(ref.nll)) == [True, True, False, True]
    for gscale in (1.0, -0.5, 3.0):
        for up in (None, 0.25):
            res = run(route, c, dtype, grad_scale=gscale, upstream=up)
            check(c, ref, res, dtype, "F", "%s %s grad_scale %g upstream %s" % (route, name(dtype), gscale, up), scale=gscale * (up or 1.0))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("route", ROUTES)
def test_f_phases(route, dtype):
    """phase 1 then phase 2 against phase 0, and phase | 4 on the log-sum-exps of s2t_ctc_argmax.  Bit equality where
    test_ctc_loss / test_ctc_loss_any_phases assert it: the gradient of phase 2 with a unit upstream scalar equals phase 0's; on
    the `any` route loss and nll too (one summing kernel in both phases; the fixed route's phase 0 adds the nll with f32 atomics, in
    any order: 1e-6 relative there); the deferred gradient on given log-sum-exps equals the one-call gradient on them.  The fixed
    route's gradient on given log-sum-exps equals phase 0's bit for bit where s2t_ctc_argmax computes them with row_lse_kernel's
    arithmetic: f32 (bf16 rows this wide take its single-pass kernel, whose sum uses the hardware exp2)."""
    c, ref = cached(case_f, dtype)
    tag = "%s %s " % (route, name(dtype))
    base = run(route, c, dtype)
    check(c, ref, base, dtype, "F", tag + "phase 0")
    p1 = run(route, c, dtype, phase=1)
    assert p1.grad is None
    check(c, ref, p1, dtype, "F", tag + "phase 1")
    if route == "any":
        assert p1.loss == base.loss and torch.equal(p1.nll, base.nll)
    else:
        assert abs(p1.loss - base.loss) <= 1e-6 * abs(base.loss)
    p2 = run(route, c, dtype, phase=2, state=p1.state, upstream=1.0)
    assert p2.loss is None
    check(c, ref, p2, dtype, "F", tag + "phase 2")
    assert bits_equal(p2.grad, base.grad), tag + "phase 2 differs from phase 0"
    p2s = run(route, c, dtype, grad_scale=3.0, phase=2, state=p1.state, upstream=0.25)
    check(c, ref, p2s, dtype, "F", tag + "phase 2, grad_scale 3, upstream 0.25", scale=0.75)
    lse = argmax_lse(c, dtype)
    r3 = run(route, c, dtype, phase=4, lse=lse)
    check(c, ref, r3, dtype, "F", tag + "phase 0 | 4")
    assert abs(r3.loss - base.loss) <= 1e-6 * abs(base.loss)
    if route == "fixed" and dtype == F32:
        assert bits_equal(r3.grad, base.grad), tag + "phase 0 | 4 differs from phase 0"
    p5 = run(route, c, dtype, phase=5, lse=lse.clone())
    check(c, ref, p5, dtype, "F", tag + "phase 1 | 4")
    p6 = run(route, c, dtype, phase=2, state=p5.state, upstream=1.0)
    assert bits_equal(p6.grad, r3.grad), tag + "phase 2 after phase 1 | 4 differs from phase 0 | 4"


# ------------------------------------------------------------------ G: refusals
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_g_refusals(dtype):
    """the limits of the fixed entry point are -95, a row stride below V and phase 3 are -22 on both; a refused call writes nothing"""
    def refused(res, rc, what):
        assert res.rc == rc, "%s: return code %d, expected %d" % (what, res.rc, rc)
        assert untouched(res.grad, dtype) and res.loss == LOSS0 and bool(torch.isnan(res.nll).all()), what + ": a refused call wrote"

    g = np.random.default_rng(8000)
    V, blank = 21, 20
    wide = make_case(3, V, 512, blank, [2], [3], pick_units(g, 512, V, blank), randn(g, (3, 1, V), dtype, 2.0), K.padded_cols(V, dtype))
    refused(run("fixed", wide, dtype), ENOTSUP, "fixed, Lmax 512")
    big = make_case(1, 40705, 1, 0, [1], [1], [[5]], randn(g, (1, 1, 40705), dtype, 2.0), K.padded_cols(40705, dtype))
    refused(run("fixed", big, dtype), ENOTSUP, "fixed, V 40705")
    c, _ = cached(case_f, dtype)
    for route in ROUTES:
        refused(run(route, c, dtype, ld_arg=c.V - 1), EINVAL, route + ", ld < V")
        refused(run(route, c, dtype, phase=3), EINVAL, route + ", phase 3")
