"""Thin tensor-level wrappers over the C ABI (one function per entry point of include/s2t_hip.h).

No arithmetic happens here: each wrapper validates shapes, allocates outputs with torch (device
memory is torch's job) and passes raw pointers to libs2t_hip.so on torch's current stream.
"""
import ctypes

import torch

from . import lib as L
from .lib import ACT_NONE, ACT_RELU, ACT_GELU, ACT_RELU_BWD, ACT_GELU_BWD, ACT_RELU_MASK, ACT_RELU_BWD_MASK  # noqa: F401


def _lib():
    return L.load()


_GEMM = None
_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16}
_RAW_STREAM = torch._C._cuda_getCurrentRawStream


def gemm(a, b, trans_a=False, trans_b=False, bias=None, residual=None, act=ACT_NONE, aux=None, aux_out=None,
         out=None, out_dtype=None, accumulate=False, splitk=1, alpha=1.0, M=None, N=None, K=None,
         map_a=None, period_a=0, map_b=None, map_c=None, out_rows=None, p_drop=0.0, seed=0):
    """C = epi(op(a) @ op(b)); a is [M,K] (or [K,M] if trans_a), b is [N,K] (or [K,N] if trans_b).

    The most frequent call of an update (~200 per step), written for host time: the bound C function and the dtype codes are
    looked up once, pointers are taken inline (a host tensor would be a GPU fault, so the operands are still checked)."""
    global _GEMM
    if _GEMM is None:
        _GEMM = _lib().s2t_gemm_gather
    if not (a.is_cuda and b.is_cuda):
        raise L.S2THipError("S2T kernels need device tensors: the hot path has no CPU fallback")
    sa0, sb0 = a.stride(0), b.stride(0)
    assert a.stride(1) == 1 and b.stride(1) == 1
    if M is None:
        M = a.shape[1] if trans_a else a.shape[0]
    if K is None:
        K = a.shape[0] if trans_a else a.shape[1]
    if N is None:
        N = b.shape[1] if trans_b else b.shape[0]
    if out is None:
        odt = out_dtype or a.dtype
        rows = out_rows if out_rows is not None else M
        out = (torch.zeros if (accumulate or splitk > 1 or map_c is not None) else torch.empty)(
            (rows, N), dtype=odt, device=a.device)
    ldaux = 0
    if act >= ACT_RELU_MASK:                 # aux / aux_out is the 1-bit record (relu_mask_bytes), not a tensor of the output's shape
        t = aux_out if act == ACT_RELU_MASK else aux
        assert t is not None and t.is_cuda and t.dtype == torch.uint8 and t.numel() == relu_mask_bytes(M, N, K) > 0
    elif residual is not None or aux is not None or aux_out is not None:
        for t in (residual, aux, aux_out):
            assert t is None or (t.dtype == out.dtype and t.stride(-1) == 1 and t.is_cuda)
        ldaux = aux.stride(0) if aux is not None else (aux_out.stride(0) if aux_out is not None else 0)
    rc = _GEMM(
        _DT[a.dtype], _DT[out.dtype], int(trans_a), int(trans_b), M, N, K, a.data_ptr(), sa0, b.data_ptr(), sb0,
        out.data_ptr(), out.stride(0), bias.data_ptr() if bias is not None else 0,
        residual.data_ptr() if residual is not None else 0, residual.stride(0) if residual is not None else 0,
        aux.data_ptr() if aux is not None else 0, aux_out.data_ptr() if aux_out is not None else 0, ldaux, act,
        int(accumulate), splitk, alpha,
        L.ptr(map_a), period_a, L.ptr(map_b), L.ptr(map_c), p_drop, seed, _RAW_STREAM(L.device_index()))
    if rc:
        L.check(rc, "s2t_gemm")
    return out


_MASK_BYTES = {}


def relu_mask_bytes(M, N, K):
    """Bytes of the 1-bit ReLU record of an [M, N] bf16 product over K (ACT_RELU_MASK / ACT_RELU_BWD_MASK); 0 = products of this
    shape keep the activations as the backward operand (ACT_RELU / ACT_RELU_BWD)."""
    key = (M, N, K, OPTION_EPOCH)           # the tile height, hence the record's size, follows the route options (reserve_cus, gemm256*)
    n = _MASK_BYTES.get(key)
    if n is None:
        if len(_MASK_BYTES) > 4096:
            _MASK_BYTES.clear()
        n = _MASK_BYTES[key] = int(_lib().s2t_gemm_relu_mask_bytes(M, N, K))
    return n


def linear_wgrad(dy, x, dw, db=None, splitk=1):
    """dw[n_out,n_in] += dy[tokens,n_out]^T x[tokens,n_in]; db[n_out] += column sums of dy (one pass over dy)."""
    L.require_cuda(dy, x)
    assert dy.dim() == 2 and x.dim() == 2 and dy.stride(1) == 1 and x.stride(1) == 1 and dy.shape[0] == x.shape[0]
    assert dw.dtype == torch.float32 and dw.stride(1) == 1 and (db is None or db.dtype == torch.float32)
    L.check(_lib().s2t_linear_wgrad(L.dt(dy), dy.shape[1], x.shape[1], dy.shape[0], L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0),
                                    L.ptr(dw), dw.stride(0), L.ptr(db), int(splitk), L.stream()), "s2t_linear_wgrad")
    return dw


WGRAD_GROUP_MAX = 4096


def wgrad_group(items):
    """items: list of (dy [tokens, n_out], x [tokens, n_in], dw [n_out, n_in] f32, db [n_out] f32 or None), bf16 operands:
    dw += dy^T x and db += column sums of dy for all of them in one launch (s2t_wgrad_group).  The operands were checked by
    wgrad_group_ok when they were queued; here only what the C side cannot see is re-checked (host time: this runs at the end of
    the decoder's backward, where the launch stream is what the GPU waits for)."""
    if not items:
        return
    fn = _lib().s2t_wgrad_group if items[0][0].dtype == torch.bfloat16 else _lib().s2t_wgrad_group_f32
    for i in range(0, len(items), WGRAD_GROUP_MAX):
        chunk = items[i:i + WGRAD_GROUP_MAX]
        arr = (L.WgradProblem * len(chunk))()
        for k, (dy, x, dw, db) in enumerate(chunk):
            if not (dy.is_cuda and x.is_cuda and dw.is_cuda and dw.dtype == torch.float32 and dy.shape[0] == x.shape[0]
                    and dw.shape[0] == dy.shape[1] and dw.shape[1] == x.shape[1] and dy.dtype == x.dtype == items[0][0].dtype):
                raise L.S2THipError("wgrad_group: item %d is not a (dy [tokens, n_out], x [tokens, n_in], f32 dw [n_out, n_in]) device triple" % k)
            p = arr[k]
            p.dY = dy.data_ptr(); p.X = x.data_ptr(); p.dW = dw.data_ptr(); p.db = db.data_ptr() if db is not None else None
            p.n_out = dy.shape[1]; p.n_in = x.shape[1]; p.tokens = dy.shape[0]
            p.ldy = dy.stride(0); p.ldx = x.stride(0); p.ldw = dw.stride(0)
        L.check(fn(len(chunk), ctypes.addressof(arr), L.stream()), "s2t_wgrad_group")


def wgrad_group_raw(n, items_addr):
    """launch n S2TWgradProblem entries of a host array the caller filled (engine: the products its layer calls appended)"""
    if n:
        L.check(_lib().s2t_wgrad_group(int(n), int(items_addr), L.stream()), "s2t_wgrad_group")


def layer_ws_bytes(desc, training):
    return int(_lib().s2t_layer_ws_bytes(ctypes.addressof(desc), int(training)))


def layer_tmp_bytes(desc):
    return int(_lib().s2t_layer_bwd_tmp_bytes(ctypes.addressof(desc)))


def layer_fwd(desc_addr, call_addr):
    rc = _lib().s2t_layer_fwd(desc_addr, call_addr, L.stream())
    if rc:
        L.check(rc, "s2t_layer_fwd")


def layer_bwd(desc_addr, call_addr):
    rc = _lib().s2t_layer_bwd(desc_addr, call_addr, L.stream())
    if rc:
        L.check(rc, "s2t_layer_bwd")


def wgrad_group_ok(dy, x):
    """shapes the grouped kernels take (otherwise: linear_wgrad): bf16 -> s2t_wgrad_group, f32 -> s2t_wgrad_group_f32"""
    if dy.dtype == torch.float32 and x.dtype == torch.float32:
        return (dy.stride(1) == 1 and x.stride(1) == 1 and dy.stride(0) % 4 == 0 and x.stride(0) % 4 == 0
                and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
                and (dy.shape[1] + 3) // 4 * 4 <= dy.stride(0) and (x.shape[1] + 3) // 4 * 4 <= x.stride(0))
    return (dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and dy.stride(1) == 1 and x.stride(1) == 1
            and dy.stride(0) % 8 == 0 and x.stride(0) % 8 == 0 and dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
            and dy.shape[1] >= 8 and x.shape[1] >= 8
            and (dy.shape[1] + 7) // 8 * 8 <= dy.stride(0) and (x.shape[1] + 7) // 8 * 8 <= x.stride(0))


def colsum(x, out):
    """out[n] += sum_m x[m, n] (f32)."""
    assert x.dim() == 2 and x.stride(1) == 1 and out.dtype == torch.float32
    L.check(_lib().s2t_colsum(L.dt(x), L.ptr(x), x.stride(0), x.shape[0], x.shape[1], L.ptr(out), L.stream()), "s2t_colsum")
    return out


def _tb(x):
    """(time stride, batch stride) in elements of a [T,B,...] view whose last dim is contiguous."""
    return x.stride(0), x.stride(1)


def attn_fwd(q, k, v, heads, klen=None, causal=False, scale=None, p_drop=0.0, seed=0, out=None, dist_penalty=False):
    """q [Tq,B,D'], k/v [Tk,B,D'] views (last dim contiguous, may be slices of a fused QKV buffer)."""
    Tq, B, D = q.shape
    Tk = k.shape[0]
    d = D // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((Tq, B, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device)
    rc = _lib().s2t_attn_fwd(L.dt(q), d, B, heads, Tq, Tk, L.ptr(q), *_tb(q), L.ptr(k), *_tb(k), L.ptr(v), *_tb(v),
                             L.ptr(out), *_tb(out), L.ptr(lse), L.ptr(klen), int(causal), int(bool(dist_penalty)), float(scale), float(p_drop),
                             int(seed), L.stream())
    L.check(rc, "s2t_attn_fwd")
    return out, lse


def attn_keep_bytes(d, B, heads, Tq, Tk, causal=False, dist_penalty=False, p_drop=0.0):
    """Bytes of the dropout keep-bit record of a bf16 attention call (s2t_attn_keep_bytes: layout in include/s2t_hip.h); 0 = the call
    does not take the second-generation kernels' plain path and its backward hashes.  Follows the attention route options."""
    return int(_lib().s2t_attn_keep_bytes(d, B, heads, Tq, Tk, int(causal), int(bool(dist_penalty)), float(p_drop)))


def attn_fwd_keep(q, k, v, heads, keep, klen=None, causal=False, scale=None, p_drop=0.0, seed=0, out=None, dist_penalty=False):
    """attn_fwd that also writes the keep-bit record `keep` (a device tensor of attn_keep_bytes bytes; None = attn_fwd exactly)"""
    Tq, B, D = q.shape
    Tk = k.shape[0]
    d = D // heads
    if scale is None:
        scale = d ** -0.5
    if out is None:
        out = torch.empty((Tq, B, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device)
    if keep is not None:
        L.require_cuda(keep)
        assert keep.is_contiguous() and keep.numel() * keep.element_size() >= attn_keep_bytes(d, B, heads, Tq, Tk, causal, dist_penalty, p_drop)
    rc = _lib().s2t_attn_fwd_keep(L.dt(q), d, B, heads, Tq, Tk, L.ptr(q), *_tb(q), L.ptr(k), *_tb(k), L.ptr(v), *_tb(v),
                                  L.ptr(out), *_tb(out), L.ptr(lse), L.ptr(klen), int(causal), int(bool(dist_penalty)), float(scale),
                                  float(p_drop), int(seed), L.ptr(keep), L.stream())
    L.check(rc, "s2t_attn_fwd_keep")
    return out, lse


def attn_bwd_keep(q, k, v, o, do, lse, heads, dq, dk, dv, keep, klen=None, causal=False, scale=None, p_drop=0.0, seed=0, dist_penalty=False):
    """attn_bwd reading the keep-bit record attn_fwd_keep wrote for this call (None = attn_bwd exactly)"""
    Tq, B, D = q.shape
    Tk = k.shape[0]
    d = D // heads
    if scale is None:
        scale = d ** -0.5
    delta = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device)
    if keep is not None:
        L.require_cuda(keep)
        assert keep.is_contiguous() and keep.numel() * keep.element_size() >= attn_keep_bytes(d, B, heads, Tq, Tk, causal, dist_penalty, p_drop)
    rc = _lib().s2t_attn_bwd_keep(L.dt(q), d, B, heads, Tq, Tk, L.ptr(q), *_tb(q), L.ptr(k), *_tb(k), L.ptr(v), *_tb(v),
                                  L.ptr(o), *_tb(o), L.ptr(do), *_tb(do), L.ptr(lse), L.ptr(delta),
                                  L.ptr(dq), *_tb(dq), L.ptr(dk), *_tb(dk), L.ptr(dv), *_tb(dv),
                                  L.ptr(klen), int(causal), int(bool(dist_penalty)), float(scale), float(p_drop), int(seed), L.ptr(keep), L.stream())
    L.check(rc, "s2t_attn_bwd_keep")
    return dq, dk, dv


def attn_probs_avg(q, k, heads, klen=None, scale=None, heads_used=None):
    """head-averaged attention probabilities of one layer, recomputed from q [Tq,B,D'] and k [Tk,B,D'] -> f32 [B, Tq, Tk]
    (transformer.py:756-782: what the decoder returns as `attn` for its alignment layer)"""
    Tq, B, D = q.shape
    Tk = k.shape[0]
    d = D // heads
    out = torch.empty((B, Tq, Tk), dtype=torch.float32, device=q.device)
    L.check(_lib().s2t_attn_probs_avg(L.dt(q), d, B, heads, Tq, Tk, L.ptr(q), *_tb(q), L.ptr(k), *_tb(k), L.ptr(klen),
                                      int(heads_used or heads), float(d ** -0.5 if scale is None else scale), L.ptr(out), L.stream()),
            "s2t_attn_probs_avg")
    return out


def attn_bwd(q, k, v, o, do, lse, heads, dq, dk, dv, klen=None, causal=False, scale=None, p_drop=0.0, seed=0, dist_penalty=False):
    Tq, B, D = q.shape
    Tk = k.shape[0]
    d = D // heads
    if scale is None:
        scale = d ** -0.5
    delta = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device)
    rc = _lib().s2t_attn_bwd(L.dt(q), d, B, heads, Tq, Tk, L.ptr(q), *_tb(q), L.ptr(k), *_tb(k), L.ptr(v), *_tb(v),
                             L.ptr(o), *_tb(o), L.ptr(do), *_tb(do), L.ptr(lse), L.ptr(delta),
                             L.ptr(dq), *_tb(dq), L.ptr(dk), *_tb(dk), L.ptr(dv), *_tb(dv),
                             L.ptr(klen), int(causal), int(bool(dist_penalty)), float(scale), float(p_drop), int(seed), L.stream())
    L.check(rc, "s2t_attn_bwd")
    return dq, dk, dv


_LN_FWD = _LN_BWD = None


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    """-> (y, mean, rstd).  88 calls per update, written for host time like gemm(): one allocation for both statistics, the bound C
    function looked up once, pointers taken inline (the operands are still checked: a host pointer would be a GPU fault)."""
    global _LN_FWD
    if _LN_FWD is None:
        _LN_FWD = _lib().s2t_layernorm_fwd
    if not (x.is_cuda and gamma.is_cuda and beta.is_cuda):
        raise L.S2THipError("S2T kernels need device tensors: the hot path has no CPU fallback")
    D = x.shape[-1]
    M = x.numel() // D
    assert x.is_contiguous()
    y = torch.empty_like(x)
    st = torch.empty((2, M), dtype=torch.float32, device=x.device)
    mean, rstd = st[0], st[1]
    rc = _LN_FWD(_DT[x.dtype], x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                 M, D, float(eps), _RAW_STREAM(L.device_index()))
    if rc:
        L.check(rc, "s2t_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma, dbeta, dres=None, drop=None):
    """drop = (p, seed) of the dropout that consumes dx next: returns (dx, dropout(dx, p, seed)) from one pass."""
    global _LN_BWD
    if _LN_BWD is None:
        _LN_BWD = _lib().s2t_layernorm_bwd
    if not (dy.is_cuda and x.is_cuda and mean.is_cuda and rstd.is_cuda and gamma.is_cuda and dgamma.is_cuda and dbeta.is_cuda
            and (dres is None or dres.is_cuda)):
        raise L.S2THipError("S2T kernels need device tensors: the hot path has no CPU fallback")
    D = x.shape[-1]
    M = x.numel() // D
    assert dy.is_contiguous() and x.is_contiguous() and (dres is None or dres.is_contiguous())
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if drop is not None else None
    p, seed = drop if drop is not None else (0.0, 0)
    rc = _LN_BWD(_DT[x.dtype], dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                 dres.data_ptr() if dres is not None else 0, dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), M, D,
                 dxd.data_ptr() if dxd is not None else 0, float(p), int(seed), _RAW_STREAM(L.device_index()))
    if rc:
        L.check(rc, "s2t_layernorm_bwd")
    return dx if drop is None else (dx, dxd)


def conv1_fwd(x, w, bias, C, dtype, act=ACT_RELU):
    """-> (y, sums, pre): pre = the pre-activation for GELU (None for ReLU, whose backward reads the mask off y)"""
    B, T, F = x.shape
    T2, F2 = (T + 1) // 2, (F + 1) // 2
    y = torch.empty((B, T2, F2, C), dtype=dtype, device=x.device)
    pre = torch.empty_like(y) if act == ACT_GELU else None
    sums = torch.zeros((2 * C,), dtype=torch.float64, device=x.device)
    L.check(_lib().s2t_conv1_fwd(L.dt(y), L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), L.ptr(pre), L.ptr(sums), B, T, F, C, act,
                                 L.stream()), "s2t_conv1_fwd")
    return y, sums, pre


def conv1_bwd(x, dpre, dw, db):
    B, T, F = x.shape
    C = dpre.shape[-1]
    L.check(_lib().s2t_conv1_bwd(L.dt(dpre), L.ptr(x), L.ptr(dpre), L.ptr(dw), L.ptr(db), B, T, F, C, L.stream()),
            "s2t_conv1_bwd")


def chan_sums(y, C, dyn=None, mean=None, rstd=None):
    P = y.numel() // C
    sums = torch.zeros((2 * C,), dtype=torch.float64, device=y.device)
    L.check(_lib().s2t_chan_sums(L.dt(y), L.ptr(y), L.ptr(dyn), L.ptr(mean), L.ptr(rstd), L.ptr(sums), P, C,
                                 0 if dyn is None else 1, L.stream()), "s2t_chan_sums")
    return sums


def conv1_bwd_bn(x, dyn, y, mean, rstd, gamma, sums, dw, db, dgamma, dbeta, count, training=True, pre=None):
    """bn_bwd_apply + conv1_bwd in one pass: the gradient w.r.t. conv1's output stays in registers"""
    B, T, F = x.shape
    C = y.shape[-1]
    L.check(_lib().s2t_conv1_bwd_bn(L.dt(y), L.ptr(x), L.ptr(dyn), L.ptr(y), L.ptr(pre), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(sums),
                                    L.ptr(dw), L.ptr(db), L.ptr(dgamma), L.ptr(dbeta), B, T, F, C, float(count), int(training), L.stream()),
            "s2t_conv1_bwd_bn")


def bn_finalize(sums, gamma, beta, run_mean, run_var, num_batches, count, training, momentum=0.1, eps=1e-5):
    C = gamma.numel()
    o = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    L.check(_lib().s2t_bn_finalize(L.ptr(sums), L.ptr(gamma), L.ptr(beta), L.ptr(run_mean), L.ptr(run_var),
                                   L.ptr(num_batches), L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]),
                                   float(count), C, int(training), float(momentum), float(eps), L.stream()), "s2t_bn_finalize")
    return o[0], o[1], o[2], o[3]            # mean, rstd, scale, shift


def bn_apply(y, scale, shift, p_drop=0.0, seed=0):
    """yn = dropout(y*scale + shift, p_drop, seed) in one pass (same bits as dropout(bn_apply(y)))"""
    yn = torch.empty_like(y)
    L.check(_lib().s2t_bn_apply(L.dt(y), L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(yn), y.numel(), scale.numel(), float(p_drop),
                                int(seed), L.stream()), "s2t_bn_apply")
    return yn


def bn_bwd_apply(dyn, y, mean, rstd, gamma, sums, dgamma, dbeta, count, training=True, pre=None):
    dpre = torch.empty_like(y)
    L.check(_lib().s2t_bn_bwd_apply(L.dt(y), L.ptr(dyn), L.ptr(y), L.ptr(pre), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(sums),
                                    L.ptr(dpre), L.ptr(dgamma), L.ptr(dbeta), y.numel(), gamma.numel(), float(count),
                                    int(training), L.stream()), "s2t_bn_bwd_apply")
    return dpre


def permute_cf(src, dst, N, C, F, mode):
    L.check(_lib().s2t_permute_cf(L.dt(dst), L.ptr(src), L.ptr(dst), N, C, F, mode, L.stream()), "s2t_permute_cf")
    return dst


def permute_conv_w(src, dst, Co, Ci, mode):
    L.check(_lib().s2t_permute_conv_w(L.dt(dst), L.ptr(src), L.ptr(dst), Co, Ci, mode, L.stream()), "s2t_permute_conv_w")
    return dst


def add_pos(x, table, len32, out=None, p_drop=0.0, seed=0):
    """out = dropout(x + positions) in one pass (out = None: in place)"""
    T, B, D = x.shape
    out = x if out is None else out
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and out.dtype == x.dtype
    assert table.shape[0] >= T + 1 and table.shape[1] == D
    L.check(_lib().s2t_add_pos(L.dt(x), L.ptr(x), L.ptr(out), L.ptr(table), L.ptr(len32), T, B, D, float(p_drop), int(seed), L.stream()),
            "s2t_add_pos")
    return out


def padded_cols(V, dtype):
    """row stride (elements) that keeps every row 16-byte aligned"""
    e = 8 if dtype == torch.bfloat16 else 4
    return (V + e - 1) // e * e


def alloc_rows(rows_shape, V, dtype, device, zero=False):
    """[..., V] view of a buffer whose row stride is padded (see padded_cols)."""
    ld = padded_cols(V, dtype)
    buf = (torch.zeros if zero else torch.empty)(tuple(rows_shape) + (ld,), dtype=dtype, device=device)
    return buf[..., :V]


def _row_ld(x):
    """row stride of a [T,B,V] / [rows,V] view with dense leading dims"""
    assert x.stride(-1) == 1
    ld = x.stride(-2)
    if x.dim() == 3:
        if x.shape[1] == 1:                    # batch of one: the stride torch reports for a size-1 dimension is arbitrary
            return x.stride(0) if x.shape[0] > 1 else max(ld, x.shape[2])
        assert x.shape[0] == 1 or x.stride(0) == x.shape[1] * ld
    return ld


def ctc_argmax(logits, want_lse=False):
    """(pred, pmax) [B, T]; want_lse: also the rows' log-sum-exps [T*B] (same pass), which ctc_loss(lse=...) reuses"""
    T, B, V = logits.shape
    pred = torch.empty((B, T), dtype=torch.int32, device=logits.device)
    pmax = torch.empty((B, T), dtype=torch.float32, device=logits.device)
    lse = torch.empty((T * B,), dtype=torch.float32, device=logits.device) if want_lse else None
    L.check(_lib().s2t_ctc_argmax(L.dt(logits), L.ptr(logits), L.ptr(pred), L.ptr(pmax), L.ptr(lse), T, B, V, _row_ld(logits), L.stream()),
            "s2t_ctc_argmax")
    return (pred, pmax, lse) if want_lse else (pred, pmax)


def ctc_rle(pred, pmax, len64, strategy=0):
    B, T = pred.shape
    dev = pred.device
    seg = torch.empty((B, T), dtype=torch.int32, device=dev)
    rs = torch.empty((B, T), dtype=torch.int32, device=dev)
    rl = torch.empty((B, T), dtype=torch.int32, device=dev)
    new_len = torch.empty((B,), dtype=torch.int64, device=dev)
    w = torch.empty((B, T), dtype=torch.float32, device=dev)
    L.check(_lib().s2t_ctc_rle(L.ptr(pred), L.ptr(pmax), L.ptr(len64), L.ptr(seg), L.ptr(rs), L.ptr(rl), L.ptr(new_len),
                               L.ptr(w), T, B, strategy, L.stream()), "s2t_ctc_rle")
    return seg, rs, rl, new_len, w


def ctc_compress_fwd(x, w, rs, rl, new_len, Tout):
    T, B, D = x.shape
    out = torch.empty((Tout, B, D), dtype=x.dtype, device=x.device)
    L.check(_lib().s2t_ctc_compress_fwd(L.dt(x), L.ptr(x), L.ptr(w), L.ptr(rs), L.ptr(rl), L.ptr(new_len), L.ptr(out),
                                        T, B, D, Tout, L.stream()), "s2t_ctc_compress_fwd")
    return out


def ctc_compress_bwd(dout, w, seg, dx, accumulate=False):
    T, B, D = dx.shape
    L.check(_lib().s2t_ctc_compress_bwd(L.dt(dx), L.ptr(dout), L.ptr(w), L.ptr(seg), L.ptr(dx), T, B, D, int(accumulate),
                                        L.stream()), "s2t_ctc_compress_bwd")
    return dx


CTC_MAX_TARGET, CTC_MAX_VOCAB = 511, 40704        # S2T_CTC_MAX_TARGET / S2T_CTC_MAX_VOCAB of include/s2t_hip.h


def ctc_loss(logits, targets, tgt_len, in_len32, blank, grad_scale=1.0, defer_grad=False, lse=None, route="auto"):
    """Returns (loss_sum f32[1], grad like logits, nll).  defer_grad: the forward pass only; the second result is then the workspace
    tuple for ctc_loss_grad (called from backward with the upstream gradient as a device scalar: no separate scaling pass).
    route "auto": s2t_ctc_loss within its limits (transcripts of at most CTC_MAX_TARGET units, vocabularies of at most
    CTC_MAX_VOCAB entries), s2t_ctc_loss_any beyond them; "any" runs s2t_ctc_loss_any whatever the shape."""
    T, B, V = logits.shape
    Lmax = targets.shape[1]
    if route not in ("auto", "any"):
        raise ValueError("ctc_loss route must be 'auto' or 'any', got %r" % (route,))
    if route == "auto":
        route = "fixed" if Lmax <= CTC_MAX_TARGET and V <= CTC_MAX_VOCAB else "any"
    dev = logits.device
    lse_given = lse is not None                     # row log-sum-exps of THESE logits from ctc_argmax(want_lse=True)
    if lse is None:
        lse = torch.empty((T * B,), dtype=torch.float32, device=dev)
    assert lse.numel() == T * B and lse.dtype == torch.float32
    nll = torch.empty((B,), dtype=torch.float32, device=dev)
    ld = _row_ld(logits)
    grad = None if defer_grad else torch.empty((T, B, ld), dtype=logits.dtype, device=dev)[..., :V]
    loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    phase = (1 if defer_grad else 0) | (4 if lse_given else 0)
    if route == "fixed":
        S = next(r for r in (64, 128, 256, 512, 1024) if 2 * Lmax + 1 <= r)      # S2T_CTC_ROW(Lmax), include/s2t_hip.h
        la = torch.empty((B * T * S,), dtype=torch.float32, device=dev)
        lb = torch.empty((B * T * S,), dtype=torch.float32, device=dev)
        L.check(_lib().s2t_ctc_loss(L.dt(logits), L.ptr(logits), L.ptr(targets), L.ptr(tgt_len), L.ptr(in_len32), L.ptr(lse),
                                    L.ptr(la), L.ptr(lb), L.ptr(nll), L.ptr(grad), L.ptr(loss), T, B, V, ld, Lmax, blank,
                                    float(grad_scale), phase, 0, L.stream()), "s2t_ctc_loss")
    else:
        nbytes = _lib().s2t_ctc_loss_any_workspace(T, B, Lmax, V)
        la = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=dev)      # the whole workspace; lb unused on this route
        lb = None
        L.check(_lib().s2t_ctc_loss_any(L.dt(logits), L.ptr(logits), L.ptr(targets), L.ptr(tgt_len), L.ptr(in_len32), L.ptr(lse),
                                        L.ptr(la), L.ptr(nll), L.ptr(grad), L.ptr(loss), T, B, V, ld, Lmax, blank,
                                        float(grad_scale), phase, 0, L.stream()), "s2t_ctc_loss_any")
    if defer_grad:
        return loss, (logits, targets, tgt_len, in_len32, lse, la, lb, nll, blank, float(grad_scale), route), nll
    return loss, grad, nll


def ctc_loss_grad(ws, upstream):
    """gradient w.r.t. the logits from the workspaces of ctc_loss(defer_grad=True), times the device scalar `upstream` (f32[1]),
    on the route that produced them"""
    logits, targets, tgt_len, in_len32, lse, la, lb, nll, blank, grad_scale, route = ws
    T, B, V = logits.shape
    ld = _row_ld(logits)
    grad = torch.empty((T, B, ld), dtype=logits.dtype, device=logits.device)[..., :V]
    assert upstream.dtype == torch.float32 and upstream.numel() == 1
    if route == "fixed":
        L.check(_lib().s2t_ctc_loss(L.dt(logits), L.ptr(logits), L.ptr(targets), L.ptr(tgt_len), L.ptr(in_len32), L.ptr(lse),
                                    L.ptr(la), L.ptr(lb), L.ptr(nll), L.ptr(grad), 0, T, B, V, ld, targets.shape[1], blank,
                                    grad_scale, 2, L.ptr(upstream), L.stream()), "s2t_ctc_loss")
    else:
        L.check(_lib().s2t_ctc_loss_any(L.dt(logits), L.ptr(logits), L.ptr(targets), L.ptr(tgt_len), L.ptr(in_len32), L.ptr(lse),
                                        L.ptr(la), L.ptr(nll), L.ptr(grad), 0, T, B, V, ld, targets.shape[1], blank,
                                        grad_scale, 2, L.ptr(upstream), L.stream()), "s2t_ctc_loss_any")
    return grad


def lsce(logits, target, eps, pad, want_grad=True, grad_scale=1.0):
    """logits [rows,V]; returns (sums f32[2] = loss, nll ; dlogits or None)."""
    rows, V = logits.shape
    assert target.numel() == rows
    ld = _row_ld(logits)
    sums = torch.zeros((2,), dtype=torch.float32, device=logits.device)
    dl = torch.empty((rows, ld), dtype=logits.dtype, device=logits.device)[:, :V] if want_grad else None
    L.check(_lib().s2t_lsce(L.dt(logits), L.ptr(logits), L.ptr(target), L.ptr(dl), L.ptr(sums), rows, V, ld, float(eps), pad,
                            float(grad_scale), L.stream()), "s2t_lsce")
    return sums, dl


def kd_loss(logits, target, teacher_idx, teacher_logits, lam, tau, pad, want_grad=True, grad_scale=1.0):
    """logits [rows,V]; teacher_idx/logits [rows,Kt]. Returns (loss f32[1], dlogits or None)."""
    rows, V = logits.shape
    ld = _row_ld(logits)
    s = torch.zeros((1,), dtype=torch.float32, device=logits.device)
    dl = torch.empty((rows, ld), dtype=logits.dtype, device=logits.device)[:, :V] if want_grad else None
    Kt = teacher_idx.shape[-1] if teacher_idx is not None else 0
    L.check(_lib().s2t_kd_loss(L.dt(logits), L.ptr(logits), L.ptr(target), L.ptr(teacher_idx), L.ptr(teacher_logits), L.ptr(dl),
                               L.ptr(s), rows, V, ld, Kt, float(lam), float(tau), pad, float(grad_scale), L.stream()), "s2t_kd_loss")
    return s, dl


def embed_fwd(tokens, W, table, scale, pad, pos_offset=0):
    B, Ln = tokens.shape
    D = W.shape[1]
    out = torch.empty((Ln, B, D), dtype=W.dtype, device=W.device)
    L.check(_lib().s2t_embed_fwd(L.dt(W), L.ptr(tokens), L.ptr(W), L.ptr(table), L.ptr(out), B, Ln, D, float(scale), pad,
                                 int(pos_offset), L.stream()), "s2t_embed_fwd")
    return out


def conv2_wgrad(dpre, y1n, gw, B, T2, F2, C):
    """all-taps conv2 weight gradient; returns False when the shape / dtype is not covered (caller uses the gathered GEMMs)"""
    rc = _lib().s2t_conv2_wgrad(L.dt(dpre), L.ptr(dpre), L.ptr(y1n), L.ptr(gw), B, T2, F2, C, L.stream())
    if rc == -95:
        return False
    L.check(rc, "s2t_conv2_wgrad")
    return True


def conv2_fwd(y1n, w2p, bias, B, T2, F2, C, act=ACT_RELU):
    """direct stride-2 3x3 convolution of the subsampler on channels-last rows: -> (z2 [T4*B*F4, C], pre or None), or None when the
    shape / dtype is not covered (caller uses the gathered GEMM)"""
    T4, F4 = (T2 + 1) // 2, (F2 + 1) // 2
    z2 = torch.empty((T4 * B * F4, C), dtype=y1n.dtype, device=y1n.device)
    pre = torch.empty_like(z2) if act == ACT_GELU else None
    rc = _lib().s2t_conv2_fwd(L.dt(y1n), L.ptr(y1n), L.ptr(w2p), L.ptr(bias), L.ptr(z2), L.ptr(pre), B, T2, F2, C, act, L.stream())
    if rc == -95:
        return None
    L.check(rc, "s2t_conv2_fwd")
    return z2, pre


def conv2_dgrad(dpre, w2q, dy1n, B, T2, F2, C, p_drop=0.0, seed=0):
    """data gradient of the stride-2 3x3 convolution into dy1n [B*T2*F2, C] (every element written), dropout mask of y1n applied;
    False when the shape / dtype is not covered (caller uses the four gathered products)"""
    rc = _lib().s2t_conv2_dgrad(L.dt(dpre), L.ptr(dpre), L.ptr(w2q), L.ptr(dy1n), B, T2, F2, C, float(p_drop), int(seed), L.stream())
    if rc == -95:
        return False
    L.check(rc, "s2t_conv2_dgrad")
    return True


def topk(logits, k):
    """[rows,V] (row stride may be padded) -> (f32 [rows,k] values descending, int32 [rows,k] columns)"""
    rows, V = logits.shape
    vals = torch.empty((rows, k), dtype=torch.float32, device=logits.device)
    idx = torch.empty((rows, k), dtype=torch.int32, device=logits.device)
    L.check(_lib().s2t_topk(L.dt(logits), L.ptr(logits), L.ptr(vals), L.ptr(idx), rows, V, _row_ld(logits), int(k), L.stream()), "s2t_topk")
    return vals, idx


def sample_rows(lprobs, draws, topk, topp, key, step):
    """the draws of the sampling search (include/s2t_hip.h s2t_sample_rows): f32 [rows, V] log-probabilities (row stride may be padded),
    row r / draw j = slot r * draws + j -> (int32 [rows, draws] tokens, f32 [rows, draws] their log-probabilities, int32 [rows] sizes
    of the kept sets)"""
    rows, V = lprobs.shape
    assert lprobs.dtype == torch.float32
    tok = torch.empty((rows, draws), dtype=torch.int32, device=lprobs.device)
    lp = torch.empty((rows, draws), dtype=torch.float32, device=lprobs.device)
    n_kept = torch.empty((rows,), dtype=torch.int32, device=lprobs.device)
    L.check(_lib().s2t_sample_rows(L.ptr(lprobs), rows, V, _row_ld(lprobs), int(draws), int(topk), float(topp), int(key), int(step),
                                   L.ptr(tok), L.ptr(lp), L.ptr(n_kept), L.stream()), "s2t_sample_rows")
    return tok, lp, n_kept


def log_softmax(logits, temperature=1.0):
    """[rows,V] (row stride may be padded) -> f32 [rows,V] log-probabilities"""
    rows, V = logits.shape
    out = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    L.check(_lib().s2t_log_softmax(L.dt(logits), L.ptr(logits), L.ptr(out), rows, V, _row_ld(logits), 1.0 / float(temperature),
                                   L.stream()), "s2t_log_softmax")
    return out


def softmax_probs(logits, temperature=1.0):
    """[rows,V] (row stride may be padded) -> f32 [rows,V] probabilities"""
    rows, V = logits.shape
    out = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    L.check(_lib().s2t_softmax_probs(L.dt(logits), L.ptr(logits), L.ptr(out), rows, V, _row_ld(logits), 1.0 / float(temperature),
                                     L.stream()), "s2t_softmax_probs")
    return out


def softmax_bwd(out, dout, dtype, log_probs, temperature=1.0):
    """gradient of log_softmax / softmax_probs w.r.t. the logits from the saved f32 output and its gradient -> [rows,V] of `dtype`"""
    rows, V = out.shape
    assert out.dtype == torch.float32 and dout.dtype == torch.float32 and out.is_contiguous() and dout.is_contiguous()
    dx = torch.empty((rows, V), dtype=dtype, device=out.device)
    L.check(_lib().s2t_softmax_bwd(L.dt(dx), L.ptr(out), L.ptr(dout), L.ptr(dx), rows, V, V, 1.0 / float(temperature), int(bool(log_probs)),
                                   L.stream()), "s2t_softmax_bwd")
    return dx


class NormalizedProbs(torch.autograd.Function):
    """log_softmax / softmax of logit rows with a gradient (get_normalized_probs for criteria that consume the (log-)probabilities:
    fairseq/models/fairseq_decoder.py:58-79); both directions are kernels of csrc/loss_embed.hip"""

    @staticmethod
    def forward(ctx, logits2d, log_probs):
        out = log_softmax(logits2d) if log_probs else softmax_probs(logits2d)
        ctx.save_for_backward(out)
        ctx.log_probs, ctx.dtype = bool(log_probs), logits2d.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        return softmax_bwd(out, dout.contiguous().float(), ctx.dtype, ctx.log_probs), None


def ensemble_lse(lprobs):
    """list of f32 [rows, V] log-probabilities (one per ensemble member) -> log of their mean probability, element-wise"""
    n = len(lprobs)
    assert 1 <= n <= 8 and all(t.dtype == torch.float32 and t.is_contiguous() and t.shape == lprobs[0].shape for t in lprobs)
    out = torch.empty_like(lprobs[0])
    arr = (ctypes.c_void_p * n)(*[L.ptr(t) for t in lprobs])
    L.check(_lib().s2t_ensemble_lse(n, ctypes.addressof(arr), L.ptr(out), out.numel(), L.stream()), "s2t_ensemble_lse")
    return out


def score_targets(logits_list, target):
    """log-probability of target[b][t] under each position's distribution, for one model or the log of the mean probability of up to
    eight (include/s2t_hip.h s2t_score_targets).  logits_list: (B, L, V) views of time-major buffers of one dtype, what
    `model(**net_input)[0]` is: their storage is taken as it is when rows t*B + b are evenly strided (any row stride >= V), else copied
    once into time-major order.  target: int64 [B, L].  Returns f32 [B, L]; a target outside [0, V) gives NaN."""
    n = len(logits_list)
    if not 1 <= n <= 8:
        raise ValueError("score_targets takes 1..8 members (s2t_score_targets), got %d" % n)
    B, Ln, V = logits_list[0].shape
    if tuple(target.shape) != (B, Ln) or target.dtype != torch.int64:
        raise ValueError("score_targets: target must be int64 [%d, %d], got %s %s" % (B, Ln, target.dtype, tuple(target.shape)))
    keep, ptrs, lds = [], [], []
    for x in logits_list:
        if tuple(x.shape) != (B, Ln, V) or x.dtype != logits_list[0].dtype:
            raise ValueError("score_targets: members differ in shape or dtype (%s %s against %s %s)"
                             % (x.dtype, tuple(x.shape), logits_list[0].dtype, (B, Ln, V)))
        lt = x.transpose(0, 1)
        # the check of criterions._KDFn.forward; the stride torch reports for a size-1 dimension is arbitrary (see _row_ld)
        ld = lt.stride(1) if B > 1 else (lt.stride(0) if Ln > 1 else V)
        if lt.stride(2) != 1 or ld < V or (B > 1 and Ln > 1 and lt.stride(0) != B * ld):
            lt, ld = lt.contiguous(), V
        keep.append(lt)
        ptrs.append(L.ptr(lt))
        lds.append(ld)
    target = target.contiguous()
    out = torch.empty((B, Ln), dtype=torch.float32, device=target.device)
    parr = (ctypes.c_void_p * n)(*ptrs)
    larr = (ctypes.c_int * n)(*lds)
    L.check(_lib().s2t_score_targets(L.dt(logits_list[0]), n, ctypes.addressof(parr), ctypes.addressof(larr), L.ptr(target), L.ptr(out),
                                     B, Ln, V, L.stream()), "s2t_score_targets")
    return out


def _ctc_decode_args(logits, in_len, what):
    if logits.dim() != 3 or logits.stride(-1) != 1:
        raise ValueError("%s: logits must be [T, B, V] with unit column stride, got %s" % (what, tuple(logits.shape)))
    T, B, V = logits.shape
    if tuple(in_len.shape) != (B,) or in_len.dtype != torch.int32:
        raise ValueError("%s: in_len must be int32 [%d], got %s %s" % (what, B, in_len.dtype, tuple(in_len.shape)))
    return T, B, V, in_len.contiguous()


def ctc_greedy(logits, in_len, blank):
    """best-path CTC transcripts of logits [T, B, V] (time-major, any row stride >= V; include/s2t_hip.h s2t_ctc_greedy).  in_len:
    int32 [B].  Returns device tensors (tokens int32 [B, T], n int32 [B], frames int32 [B, T, 2], tok_score f32 [B, T], score f32 [B]);
    of a sentence's rows only the first n[b] entries are written."""
    T, B, V, in_len = _ctc_decode_args(logits, in_len, "ctc_greedy")
    dev = logits.device
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    n = torch.zeros((B,), dtype=torch.int32, device=dev)
    frames = torch.empty((B, T, 2), dtype=torch.int32, device=dev)
    tok_score = torch.empty((B, T), dtype=torch.float32, device=dev)
    score = torch.zeros((B,), dtype=torch.float32, device=dev)
    if T * B == 0:
        return tokens, n, frames, tok_score, score
    ws = torch.empty((int(_lib().s2t_ctc_greedy_workspace(T, B)),), dtype=torch.uint8, device=dev)
    L.check(_lib().s2t_ctc_greedy(L.dt(logits), L.ptr(logits), L.ptr(in_len), L.ptr(ws), L.ptr(tokens), L.ptr(n), L.ptr(frames),
                                  L.ptr(tok_score), L.ptr(score), T, B, V, _row_ld(logits), int(blank), L.stream()), "s2t_ctc_greedy")
    return tokens, n, frames, tok_score, score


def ctc_prefix_beam(logits, in_len, blank, beam, cand, nbest):
    """CTC prefix beam search over logits [T, B, V] (include/s2t_hip.h s2t_ctc_prefix_beam): beam <= 16 live prefixes, the cand <= 16
    best non-blank symbols per frame, the nbest <= beam best hypotheses out.  Returns device tensors (tokens int32 [B, nbest, T],
    lens int32 [B, nbest], scores f32 [B, nbest], n_hyp int32 [B]), best first; a sentence may have fewer than nbest hypotheses."""
    T, B, V, in_len = _ctc_decode_args(logits, in_len, "ctc_prefix_beam")
    dev = logits.device
    beam, cand, nbest = int(beam), int(cand), int(nbest)
    tokens = torch.empty((B, nbest, T), dtype=torch.int32, device=dev)
    lens = torch.zeros((B, nbest), dtype=torch.int32, device=dev)
    scores = torch.full((B, nbest), float("-inf"), dtype=torch.float32, device=dev)
    n_hyp = torch.zeros((B,), dtype=torch.int32, device=dev)
    if T * B == 0:
        if B:                                          # no frames: the empty hypothesis, score 0
            n_hyp.fill_(1)
            scores[:, 0] = 0
        return tokens, lens, scores, n_hyp
    ws = torch.empty((int(_lib().s2t_ctc_prefix_beam_workspace(T, B, beam, cand, nbest)),), dtype=torch.uint8, device=dev)
    L.check(_lib().s2t_ctc_prefix_beam(L.dt(logits), L.ptr(logits), L.ptr(in_len), L.ptr(ws), L.ptr(tokens), L.ptr(lens), L.ptr(scores),
                                       L.ptr(n_hyp), T, B, V, _row_ld(logits), int(blank), beam, cand, nbest, L.stream()),
            "s2t_ctc_prefix_beam")
    return tokens, lens, scores, n_hyp


CTC_ALIGN_MAX_TARGET = 4095       # S2T_CTC_ALIGN_MAX_TARGET of include/s2t_hip.h


def ctc_align(logits, in_len, targets, tgt_len, blank):
    """forced CTC alignment of the transcripts `targets` (int64 [B, Lmax], the first tgt_len[b] entries of a row; tgt_len int64 [B]) to
    logits [T, B, V] (time-major, any row stride >= V; in_len int32 [B]): include/s2t_hip.h s2t_ctc_align states the rule.  Returns
    device tensors (states int32 [B, T], frames int32 [B, Lmax, 2], tok_score f32 [B, Lmax], score f32 [B], status int32 [B]);
    entries behind a transcript's length are not written."""
    T, B, V, in_len = _ctc_decode_args(logits, in_len, "ctc_align")
    if targets.dim() != 2 or targets.shape[0] != B or targets.dtype != torch.int64:
        raise ValueError("ctc_align: targets must be int64 [%d, Lmax], got %s %s" % (B, targets.dtype, tuple(targets.shape)))
    if tuple(tgt_len.shape) != (B,) or tgt_len.dtype != torch.int64:
        raise ValueError("ctc_align: tgt_len must be int64 [%d], got %s %s" % (B, tgt_len.dtype, tuple(tgt_len.shape)))
    Lmax = targets.shape[1]
    if Lmax > CTC_ALIGN_MAX_TARGET:
        raise ValueError("ctc_align: transcripts of at most %d tokens (S2T_CTC_ALIGN_MAX_TARGET), got a padded width of %d"
                         % (CTC_ALIGN_MAX_TARGET, Lmax))
    dev = logits.device
    targets, tgt_len = targets.contiguous(), tgt_len.contiguous()
    states = torch.full((B, T), -1, dtype=torch.int32, device=dev)
    frames = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    tok_score = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.zeros((B,), dtype=torch.float32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if T * B == 0:
        if B:                                          # no frames: only the empty transcript has a path
            status.copy_((tgt_len != 0).to(torch.int32) + ((tgt_len < 0) | (tgt_len > Lmax)).to(torch.int32))
            score.masked_fill_(status != 0, float("-inf"))
            own = (torch.arange(Lmax, device=dev)[None, :] < tgt_len[:, None]) & (status == 1)[:, None]
            frames[own] = -1
            tok_score[own] = float("-inf")
        return states, frames, tok_score, score, status
    ws = torch.empty((int(_lib().s2t_ctc_align_workspace(T, B, Lmax)),), dtype=torch.uint8, device=dev)
    # Lmax = 0: three empty tensors have no address, the entry point refuses NULL; nothing of them is read or written
    pad = torch.empty((2,), dtype=torch.int64, device=dev) if Lmax == 0 else None
    p = lambda t: L.ptr(t if Lmax else pad)
    L.check(_lib().s2t_ctc_align(L.dt(logits), L.ptr(logits), L.ptr(in_len), p(targets), L.ptr(tgt_len), L.ptr(ws), L.ptr(states),
                                 p(frames), p(tok_score), L.ptr(score), L.ptr(status), T, B, V, _row_ld(logits), Lmax, int(blank),
                                 L.stream()), "s2t_ctc_align")
    return states, frames, tok_score, score, status


CTC_SEGMENT_MAX_TARGET = 16383    # S2T_CTC_SEGMENT_MAX_TARGET of include/s2t_hip.h
CTC_SEGMENT_MAX_UTT = 4096        # S2T_CTC_SEGMENT_MAX_UTT
CTC_SEGMENT_MAX_WINDOW = 4096     # S2T_CTC_SEGMENT_MAX_WINDOW


def ctc_segment_workspace(T, B, Lmax, Umax):
    """bytes of workspace s2t_ctc_segment takes for this shape: 4*T*B*(3 + ceil((2*Lmax + 1) / 16)) rounded up to 256"""
    return int(_lib().s2t_ctc_segment_workspace(int(T), int(B), int(Lmax), int(Umax)))


def ctc_segment(logits, in_len, targets, tgt_len, utt_end, n_utt, blank, free_start=True, free_end=True, window=30):
    """CTC segmentation of recordings (include/s2t_hip.h s2t_ctc_segment states the rule): ctc_align's operands, plus the utterances
    of every transcript as cumulative end offsets utt_end (int64 [B, Umax], the first n_utt[b] entries of a row; n_utt int64 [B]).
    free_start / free_end: the outer blank states cost nothing; window: the frames of utt_conf_min's sliding mean.  Returns device
    tensors (states int32 [B, T], frames int32 [B, Lmax, 2], tok_score f32 [B, Lmax], score f32 [B], utt_frames int32 [B, Umax, 2],
    utt_score, utt_conf_mean, utt_conf_min f32 [B, Umax], status int32 [B]).  Entries behind a recording's lengths are not written,
    nor is anything but the status of a refused recording (status 2).  T = 0 launches nothing and validates nothing: every
    recording gets status 1 (no frames, no path) and the whole padded width of its outputs is filled with -1 / -inf, also for a
    recording the kernel would refuse."""
    T, B, V, in_len = _ctc_decode_args(logits, in_len, "ctc_segment")
    if targets.dim() != 2 or targets.shape[0] != B or targets.dtype != torch.int64:
        raise ValueError("ctc_segment: targets must be int64 [%d, Lmax], got %s %s" % (B, targets.dtype, tuple(targets.shape)))
    if utt_end.dim() != 2 or utt_end.shape[0] != B or utt_end.dtype != torch.int64:
        raise ValueError("ctc_segment: utt_end must be int64 [%d, Umax], got %s %s" % (B, utt_end.dtype, tuple(utt_end.shape)))
    for name, t in (("tgt_len", tgt_len), ("n_utt", n_utt)):
        if tuple(t.shape) != (B,) or t.dtype != torch.int64:
            raise ValueError("ctc_segment: %s must be int64 [%d], got %s %s" % (name, B, t.dtype, tuple(t.shape)))
    Lmax, Umax, window = targets.shape[1], utt_end.shape[1], int(window)
    if not 1 <= Lmax <= CTC_SEGMENT_MAX_TARGET:
        raise ValueError("ctc_segment: transcripts of 1 to %d tokens (S2T_CTC_SEGMENT_MAX_TARGET), got a padded width of %d"
                         % (CTC_SEGMENT_MAX_TARGET, Lmax))
    if not 1 <= Umax <= CTC_SEGMENT_MAX_UTT:
        raise ValueError("ctc_segment: 1 to %d utterances per recording (S2T_CTC_SEGMENT_MAX_UTT), got a padded width of %d"
                         % (CTC_SEGMENT_MAX_UTT, Umax))
    if not 1 <= window <= CTC_SEGMENT_MAX_WINDOW:
        raise ValueError("ctc_segment: window must lie in [1, %d] (S2T_CTC_SEGMENT_MAX_WINDOW), got %d" % (CTC_SEGMENT_MAX_WINDOW, window))
    dev = logits.device
    targets, tgt_len, utt_end, n_utt = targets.contiguous(), tgt_len.contiguous(), utt_end.contiguous(), n_utt.contiguous()
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    frames = torch.empty((B, Lmax, 2), dtype=torch.int32, device=dev)
    tok_score = torch.empty((B, Lmax), dtype=torch.float32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    utt_frames = torch.empty((B, Umax, 2), dtype=torch.int32, device=dev)
    utt_score, utt_mean, utt_min = (torch.empty((B, Umax), dtype=torch.float32, device=dev) for _ in range(3))
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    out = (states, frames, tok_score, score, utt_frames, utt_score, utt_mean, utt_min, status)
    if B == 0:
        return out
    if T == 0:                                         # no frames, no path: every transcript here has a token
        status.fill_(1)
        score.fill_(float("-inf"))
        frames.fill_(-1)
        utt_frames.fill_(-1)
        for t in (tok_score, utt_score, utt_mean, utt_min):
            t.fill_(float("-inf"))
        return out
    ws = torch.empty((ctc_segment_workspace(T, B, Lmax, Umax),), dtype=torch.uint8, device=dev)
    flags = (1 if free_start else 0) | (2 if free_end else 0)
    L.check(_lib().s2t_ctc_segment(L.dt(logits), L.ptr(logits), L.ptr(in_len), L.ptr(targets), L.ptr(tgt_len), L.ptr(utt_end), L.ptr(n_utt),
                                   L.ptr(ws), L.ptr(states), L.ptr(frames), L.ptr(tok_score), L.ptr(score), L.ptr(utt_frames),
                                   L.ptr(utt_score), L.ptr(utt_mean), L.ptr(utt_min), L.ptr(status), T, B, V, _row_ld(logits), Lmax, Umax,
                                   int(blank), flags, window, L.stream()), "s2t_ctc_segment")
    return out


EDIT_MAX_A = 32767                # S2T_EDIT_MAX_A of include/s2t_hip.h
EDIT_MAX_B = 4095                 # S2T_EDIT_MAX_B


def _token_rows(fn, na, a, a_len, nb, b, b_len):
    """the opening checks of the wrappers that take two token matrices `na` and `nb`: int32 / int64 [rows, width] each, each with
    lengths [rows] in its own dtype.  Returns the four contiguous.  (edit_align words both refusals for its one B and keeps them.)"""
    ints = (torch.int32, torch.int64)
    if a.dim() != 2 or b.dim() != 2 or a.dtype not in ints or b.dtype not in ints:
        raise ValueError("%s: %s and %s must be int32 / int64 [rows, width], got %s %s and %s %s"
                         % (fn, na, nb, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    if tuple(a_len.shape) != (a.shape[0],) or a_len.dtype != a.dtype or tuple(b_len.shape) != (b.shape[0],) or b_len.dtype != b.dtype:
        raise ValueError("%s: %s_len must be [%d] and %s_len [%d] in the dtype of their tokens, got %s %s and %s %s"
                         % (fn, na, a.shape[0], nb, b.shape[0], a_len.dtype, tuple(a_len.shape), b_len.dtype, tuple(b_len.shape)))
    return a.contiguous(), a_len.contiguous(), b.contiguous(), b_len.contiguous()


def _three_ids(fn, pad, eos, unk):
    """pad, eos and unk as ints; unk < 0 means there is none"""
    pad, eos, unk = int(pad), int(eos), int(unk)
    if pad == eos or (unk >= 0 and unk in (pad, eos)):
        raise ValueError("%s: pad, eos and unk must be three different ids, got %d, %d and %d" % (fn, pad, eos, unk))
    return pad, eos, unk


def _ptr_or(spare):
    """t -> the address of t, or of the caller's `spare` allocation for an empty t: an empty tensor has no address and the entry
    points refuse NULL; nothing of a zero-width operand is read or written"""
    return lambda t: L.ptr(t if t.numel() else spare)


def edit_align(a, a_len, b, b_len, costs=(1, 1, 1), collapse_blank=None, want_ops=False):
    """edit-distance alignment of the token rows a [B, Amax] (first a_len[b] entries) to b [B, Bmax] (first b_len[b]) under the
    integer costs (substitution, `a` token left alone, `b` token left alone): include/s2t_hip.h s2t_edit_align states the rule.
    Tokens int32 or int64 per side, a side's lengths in its tokens' dtype.  collapse_blank: a's rows are per-frame labels, collapsed
    (repeats, then that blank) in the same call.  Returns device tensors (counts int32 [B, 4] = matches, substitutions, b tokens left
    alone, a tokens left alone; cost int32 [B]; status int32 [B], 0 done / 2 refused; a_n int32 [B], the rows of each alignment;
    a_out [B, Amax] the collapsed tokens in a's dtype or None; ops uint8 [B, Amax + Bmax] and n_ops int32 [B], or None, None).
    counts, cost, a_n and n_ops of a refused sentence are 0; entries of ops behind n_ops and of a_out behind a_n are not written."""
    ints = (torch.int32, torch.int64)
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0] or a.dtype not in ints or b.dtype not in ints:
        raise ValueError("edit_align: a and b must be int32 / int64 [B, width] with one B, got %s %s and %s %s"
                         % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
    B, Amax, Bmax = a.shape[0], a.shape[1], b.shape[1]
    if tuple(a_len.shape) != (B,) or a_len.dtype != a.dtype or tuple(b_len.shape) != (B,) or b_len.dtype != b.dtype:
        raise ValueError("edit_align: a_len / b_len must be [%d] in the dtype of their tokens, got %s %s and %s %s"
                         % (B, a_len.dtype, tuple(a_len.shape), b_len.dtype, tuple(b_len.shape)))
    if Amax > EDIT_MAX_A or Bmax > EDIT_MAX_B:
        raise ValueError("edit_align: padded widths of at most %d (S2T_EDIT_MAX_A) and %d (S2T_EDIT_MAX_B), got %d and %d"
                         % (EDIT_MAX_A, EDIT_MAX_B, Amax, Bmax))
    cs, ca, cb = (int(c) for c in costs)
    if not all(1 <= c <= 255 for c in (cs, ca, cb)):
        raise ValueError("edit_align: costs must be integers in [1, 255], got %r" % (tuple(costs),))
    dev = a.device
    collapse = collapse_blank is not None
    counts = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    cost = torch.zeros((B,), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    a_n = torch.zeros((B,), dtype=torch.int32, device=dev)
    a_out = torch.empty((B, Amax), dtype=a.dtype, device=dev) if collapse else None
    ops = torch.empty((B, Amax + Bmax), dtype=torch.uint8, device=dev) if want_ops else None
    n_ops = torch.zeros((B,), dtype=torch.int32, device=dev) if want_ops else None
    if B == 0:
        return counts, cost, status, a_n, a_out, ops, n_ops
    a, a_len, b, b_len = a.contiguous(), a_len.contiguous(), b.contiguous(), b_len.contiguous()
    nbytes = int(_lib().s2t_edit_align_workspace(B, Amax, Bmax, 1)) if want_ops else 0
    ws = torch.empty((max(nbytes, 8),), dtype=torch.uint8, device=dev)
    p = _ptr_or(torch.empty((2,), dtype=torch.int64, device=dev))
    L.check(_lib().s2t_edit_align(p(a), L.ptr(a_len), a.element_size(), p(b), L.ptr(b_len), b.element_size(), B, Amax, Bmax, cs, ca, cb,
                                  int(collapse), int(collapse_blank) if collapse else 0, L.ptr(ws), L.ptr(counts), L.ptr(cost),
                                  L.ptr(status), L.ptr(a_n), p(a_out) if collapse else 0, p(ops) if want_ops else 0,
                                  L.ptr(n_ops) if want_ops else 0, L.stream()), "s2t_edit_align")
    return counts, cost, status, a_n, a_out, ops, n_ops


BLEU_MAX_LEN = 4095               # S2T_BLEU_MAX_LEN of include/s2t_hip.h
BLEU_WAVE_LEN = 64                # S2T_BLEU_WAVE_LEN: hypotheses up to this padded width take one wave each, wider ones a workgroup
BLEU_GROUP_LEN = 256              # S2T_BLEU_GROUP_LEN: of 256 threads up to this width, of 1,024 above


def bleu_stats(hyp, hyp_len, ref, ref_len, pad, eos, unk=-1, ref_row=None):
    """BLEU statistics of the token rows hyp [B, Hmax] (first hyp_len[b] entries) against ref [Rrows, Rmax] (first ref_len[r]):
    include/s2t_hip.h s2t_bleu_stats states the rule (trim by pad / eos, clipped n-gram matches of the orders 1 to 4, a reference
    `unk` never matches; unk < 0 switches that off).  Tokens int32 or int64 per side, a side's lengths in its tokens' dtype.
    ref_row: int32 [B], sentence b is scored against row ref_row[b]; None scores row b (then Rrows must be B).  Returns device
    tensors (stats int32 [B, 10] = reflen, predlen, match1, count1, ... match4, count4; status int32 [B], 0 done / 2 refused: a
    length outside its padded width or a ref_row entry outside [0, Rrows), the stats are zeros)."""
    hyp, hyp_len, ref, ref_len = _token_rows("bleu_stats", "hyp", hyp, hyp_len, "ref", ref, ref_len)
    B, Hmax, Rrows, Rmax = hyp.shape[0], hyp.shape[1], ref.shape[0], ref.shape[1]
    if ref_row is None:
        if Rrows != B:
            raise ValueError("bleu_stats: %d hypotheses and %d references need a ref_row map" % (B, Rrows))
    elif tuple(ref_row.shape) != (B,) or ref_row.dtype != torch.int32:
        raise ValueError("bleu_stats: ref_row must be int32 [%d], got %s %s" % (B, ref_row.dtype, tuple(ref_row.shape)))
    if Hmax > BLEU_MAX_LEN or Rmax > BLEU_MAX_LEN:
        raise ValueError("bleu_stats: padded widths of at most %d (S2T_BLEU_MAX_LEN), got %d and %d" % (BLEU_MAX_LEN, Hmax, Rmax))
    pad, eos, unk = _three_ids("bleu_stats", pad, eos, unk)
    dev = hyp.device
    stats = torch.zeros((B, 10), dtype=torch.int32, device=dev)
    status = torch.zeros((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return stats, status
    p = _ptr_or(torch.zeros((2,), dtype=torch.int64, device=dev))
    L.check(_lib().s2t_bleu_stats(p(hyp), L.ptr(hyp_len), hyp.element_size(), p(ref), p(ref_len), ref.element_size(),
                                  L.ptr(ref_row.contiguous()) if ref_row is not None else 0, B, Hmax, Rmax, Rrows, pad, eos, unk,
                                  L.ptr(stats), L.ptr(status), L.stream()), "s2t_bleu_stats")
    return stats, status


MBR_MAX_LEN = 1024                # S2T_MBR_MAX_LEN of include/s2t_hip.h: the padded widths of s2t_bleu_pairs
MBR_MAX_LIST = 256                # S2T_MBR_MAX_LIST: pseudo-references per sentence
MBR_WAVE_LEN = 64                 # S2T_MBR_WAVE_LEN: candidates up to this padded width take one wave each, wider ones a workgroup
MBR_GROUP_LEN = 256               # S2T_MBR_GROUP_LEN: of 256 threads up to this width, of 1,024 above
MBR_SLICE = 8                     # S2T_MBR_SLICE: the entries of a candidate's list one workgroup takes
MBR_CHUNK_BYTES = 32768           # S2T_MBR_CHUNK_BYTES: the LDS a workgroup fills with pseudo-references between two barriers


def bleu_pairs_chunk(Pmax, wide):
    """S2T_MBR_CHUNK: the pseudo-references of padded width Pmax a workgroup of s2t_bleu_pairs stages at once; wide: tokens are
    staged as 64-bit (either side int64)"""
    return min(MBR_CHUNK_BYTES // ((Pmax + 4) * (8 if wide else 4)), MBR_SLICE)


def bleu_pairs(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, max_list=None):
    """BLEU statistics of every candidate row of cand [Rc, Hmax] (first cand_len[c] entries) against every pseudo-reference of its
    sentence: cand_sent int32 [Rc] names the sentence, the rows ref_off[b] .. ref_off[b+1] - 1 of ref [Rr, Pmax] (ref_off int32
    [B + 1]) are sentence b's list.  include/s2t_hip.h s2t_bleu_pairs; the rule of a pair is s2t_bleu_stats's with the candidate as
    the hypothesis.  cand and ref may be the same tensor.  max_list: the widest list M, which the caller knows from its lists'
    shapes; None reads it from ref_off (a host read).  Returns device tensors (stats int32 [Rc, M, 10], status int32 [Rc, M]: 0 done,
    2 refused -- a length outside its padded width, a sentence outside [0, B), offsets that descend, leave [0, Rr] or span more than
    M rows; zeros, and zeros behind a sentence's list)."""
    cand, cand_len, ref, ref_len = _token_rows("bleu_pairs", "cand", cand, cand_len, "ref", ref, ref_len)
    Rc, Hmax, Rr, Pmax = cand.shape[0], cand.shape[1], ref.shape[0], ref.shape[1]
    if tuple(cand_sent.shape) != (Rc,) or cand_sent.dtype != torch.int32:
        raise ValueError("bleu_pairs: cand_sent must be int32 [%d], got %s %s" % (Rc, cand_sent.dtype, tuple(cand_sent.shape)))
    if ref_off.dim() != 1 or ref_off.shape[0] < 1 or ref_off.dtype != torch.int32:
        raise ValueError("bleu_pairs: ref_off must be int32 [sentences + 1], got %s %s" % (ref_off.dtype, tuple(ref_off.shape)))
    B = ref_off.shape[0] - 1
    if Hmax > MBR_MAX_LEN or Pmax > MBR_MAX_LEN:
        raise ValueError("bleu_pairs: padded widths of at most %d (S2T_MBR_MAX_LEN), got %d and %d" % (MBR_MAX_LEN, Hmax, Pmax))
    if max_list is None:
        max_list = int((ref_off[1:] - ref_off[:-1]).clamp(min=0, max=MBR_MAX_LIST).max()) if B else 0
    M = int(max_list)
    if not 0 <= M <= MBR_MAX_LIST:
        raise ValueError("bleu_pairs: lists of at most %d pseudo-references (S2T_MBR_MAX_LIST), got %d" % (MBR_MAX_LIST, M))
    pad, eos, unk = _three_ids("bleu_pairs", pad, eos, unk)
    dev = cand.device
    stats = torch.empty((Rc, M, 10), dtype=torch.int32, device=dev)      # the kernel writes every element
    status = torch.empty((Rc, M), dtype=torch.int32, device=dev)
    if Rc == 0 or M == 0:
        return stats, status
    p = _ptr_or(torch.zeros((2,), dtype=torch.int64, device=dev))
    L.check(_lib().s2t_bleu_pairs(p(cand), L.ptr(cand_len), cand.element_size(), p(ref), p(ref_len), ref.element_size(),
                                  L.ptr(cand_sent.contiguous()), L.ptr(ref_off.contiguous()), Rc, B, Hmax, Pmax, Rr, M, pad, eos, unk,
                                  L.ptr(stats), L.ptr(status), L.stream()), "s2t_bleu_pairs")
    return stats, status


CHRF_MAX_LEN = 1024               # S2T_CHRF_MAX_LEN of include/s2t_hip.h: the padded widths of s2t_chrf_stats, in tokens
CHRF_MAX_CHARS = 4095             # S2T_CHRF_MAX_CHARS: characters per side; a longer side is refused by the kernel (status 2)
CHRF_GROUP_LEN = 64               # S2T_CHRF_GROUP_LEN: hypotheses up to this padded width take 256 threads a pair, wider ones 1,024
CHRF_MAX_CHAR_ORDER = 6           # S2T_CHRF_MAX_CHAR_ORDER
CHRF_MAX_WORD_ORDER = 2           # S2T_CHRF_MAX_WORD_ORDER
CHRF_SEP = 0xffffffff             # S2T_CHRF_SEP: the word break inside a piece
CHRF_STATS = 24                   # (hyp, ref, match) of the character orders 1 .. 6, then of the word orders 1 .. 2


def chrf_stats(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk=-1, char_order=6, word_order=0, hyp_row=None, ref_row=None):
    """chrF statistics of pairs of token rows, hyp [Hrows, Hmax] (first hyp_len[r] entries) against ref [Rrows, Rmax]: include/s2t_hip.h
    s2t_chrf_stats states the rule.  Tokens int32 or int64 per side, a side's lengths in its tokens' dtype.  pieces (int32 or uint32
    code points, CHRF_SEP -- as int32, -1 -- for a word break) and piece_off (int32 [V + 2], entry V the reference-side rendering of
    unk) are the piece table of chrf_scorer.piece_table, on the device.  hyp_row / ref_row: int32 [P], pair p is row hyp_row[p]
    against row ref_row[p]; None means row p (without any map both sides have P rows).  Returns device tensors (stats int32 [P, 24]
    = hyp_n, ref_n, match_n of the character orders 1 .. 6 and the word orders 1 .. 2, zeros above the configured orders; status
    int32 [P], 0 done / 2 refused: a map entry outside its matrix, a length outside its padded width, a token outside [0, V), a side
    of more than CHRF_MAX_CHARS characters; the stats are zeros)."""
    hyp, hyp_len, ref, ref_len = _token_rows("chrf_stats", "hyp", hyp, hyp_len, "ref", ref, ref_len)
    Hrows, Hmax, Rrows, Rmax = hyp.shape[0], hyp.shape[1], ref.shape[0], ref.shape[1]
    for name, m in (("hyp_row", hyp_row), ("ref_row", ref_row)):
        if m is not None and (m.dim() != 1 or m.dtype != torch.int32):
            raise ValueError("chrf_stats: %s must be int32 [pairs], got %s %s" % (name, m.dtype, tuple(m.shape)))
    P = hyp_row.shape[0] if hyp_row is not None else ref_row.shape[0] if ref_row is not None else Hrows
    if (hyp_row is not None and hyp_row.shape[0] != P) or (ref_row is not None and ref_row.shape[0] != P):
        raise ValueError("chrf_stats: hyp_row and ref_row must both be int32 [%d], got %s and %s" % (P, tuple(hyp_row.shape), tuple(ref_row.shape)))
    if (hyp_row is None and Hrows != P) or (ref_row is None and Rrows != P):
        raise ValueError("chrf_stats: %d pairs of %d hypothesis rows and %d reference rows need a row map for the side that has not %d rows"
                         % (P, Hrows, Rrows, P))
    if Hmax > CHRF_MAX_LEN or Rmax > CHRF_MAX_LEN:
        raise ValueError("chrf_stats: padded widths of at most %d tokens (S2T_CHRF_MAX_LEN), got %d and %d" % (CHRF_MAX_LEN, Hmax, Rmax))
    char_order, word_order, unk = int(char_order), int(word_order), int(unk)
    if not 1 <= char_order <= CHRF_MAX_CHAR_ORDER:
        raise ValueError("chrf_stats: char_order from 1 to %d (S2T_CHRF_MAX_CHAR_ORDER), got %d" % (CHRF_MAX_CHAR_ORDER, char_order))
    if not 0 <= word_order <= CHRF_MAX_WORD_ORDER:
        raise ValueError("chrf_stats: word_order from 0 to %d (S2T_CHRF_MAX_WORD_ORDER), got %d" % (CHRF_MAX_WORD_ORDER, word_order))
    if pieces.dim() != 1 or pieces.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or piece_off.dim() != 1 or piece_off.dtype != torch.int32 \
            or piece_off.shape[0] < 2:
        raise ValueError("chrf_stats: the piece table is pieces (int32 / uint32 [n]) and piece_off (int32 [V + 2]), got %s %s and %s %s"
                         % (pieces.dtype, tuple(pieces.shape), piece_off.dtype, tuple(piece_off.shape)))
    V = piece_off.shape[0] - 2
    if unk >= V:
        raise ValueError("chrf_stats: unk must be a token of the table's %d (or negative), got %d" % (V, unk))
    dev = hyp.device
    stats = torch.empty((P, CHRF_STATS), dtype=torch.int32, device=dev)      # the kernel writes every element
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    if P == 0:
        return stats, status
    p = _ptr_or(torch.zeros((2,), dtype=torch.int64, device=dev))
    L.check(_lib().s2t_chrf_stats(p(hyp), p(hyp_len), hyp.element_size(), p(ref), p(ref_len), ref.element_size(),
                                  L.ptr(hyp_row.contiguous()) if hyp_row is not None else 0,
                                  L.ptr(ref_row.contiguous()) if ref_row is not None else 0, P, Hmax, Rmax, Hrows, Rrows,
                                  p(pieces.contiguous()), L.ptr(piece_off.contiguous()), pieces.shape[0], V, unk, char_order, word_order,
                                  L.ptr(stats), L.ptr(status), L.stream()), "s2t_chrf_stats")
    return stats, status


TEXT_MAX_UNITS = 4095             # S2T_TEXT_MAX_UNITS of include/s2t_hip.h: units per side, = EDIT_MAX_B = CHRF_MAX_CHARS
TEXT_MODES = {"word": 0, "char": 1, "char_nospace": 2}      # the `mode` of s2t_text_units


def text_units(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk, mode, hyp_width, ref_width, hyp_row=None, ref_row=None):
    """unit rows of pairs of token rows, hyp [Hrows, Hmax] (first hyp_len[r] entries) against ref [Rrows, Rmax]: include/s2t_hip.h
    s2t_text_units states the rule.  mode: 0 words (first-equal-occurrence ids over both sides of the pair), 1 characters with one
    space between words, 2 characters without (TEXT_MODES).  hyp_width / ref_width: the widths Uh / Ur of the unit rows, at most
    TEXT_MAX_UNITS.  Tokens, lengths, the piece table, unk and the row maps are those of `chrf_stats`.  Returns device tensors
    (hyp_units int32 [P, Uh], hyp_n int32 [P], ref_units int32 [P, Ur], ref_n int32 [P], status int32 [P]: 0 done / 2 refused --
    what chrf_stats refuses, or a side with more units than its width; hyp_n = ref_n = 0 then).  Entries of the unit rows behind
    hyp_n / ref_n are not written."""
    hyp, hyp_len, ref, ref_len = _token_rows("text_units", "hyp", hyp, hyp_len, "ref", ref, ref_len)
    Hrows, Hmax, Rrows, Rmax = hyp.shape[0], hyp.shape[1], ref.shape[0], ref.shape[1]
    for name, m in (("hyp_row", hyp_row), ("ref_row", ref_row)):
        if m is not None and (m.dim() != 1 or m.dtype != torch.int32):
            raise ValueError("text_units: %s must be int32 [pairs], got %s %s" % (name, m.dtype, tuple(m.shape)))
    P = hyp_row.shape[0] if hyp_row is not None else ref_row.shape[0] if ref_row is not None else Hrows
    if (hyp_row is not None and hyp_row.shape[0] != P) or (ref_row is not None and ref_row.shape[0] != P):
        raise ValueError("text_units: hyp_row and ref_row must both be int32 [%d], got %s and %s" % (P, tuple(hyp_row.shape), tuple(ref_row.shape)))
    if (hyp_row is None and Hrows != P) or (ref_row is None and Rrows != P):
        raise ValueError("text_units: %d pairs of %d hypothesis rows and %d reference rows need a row map for the side that has not %d rows"
                         % (P, Hrows, Rrows, P))
    if Hmax > CHRF_MAX_LEN or Rmax > CHRF_MAX_LEN:
        raise ValueError("text_units: padded widths of at most %d tokens (S2T_CHRF_MAX_LEN), got %d and %d" % (CHRF_MAX_LEN, Hmax, Rmax))
    mode, Uh, Ur, unk = int(mode), int(hyp_width), int(ref_width), int(unk)
    if mode not in TEXT_MODES.values():
        raise ValueError("text_units: mode is 0 (words), 1 (characters with spaces) or 2 (characters without), got %d" % mode)
    if not (0 <= Uh <= TEXT_MAX_UNITS and 0 <= Ur <= TEXT_MAX_UNITS):
        raise ValueError("text_units: unit widths from 0 to %d (S2T_TEXT_MAX_UNITS), got %d and %d" % (TEXT_MAX_UNITS, Uh, Ur))
    if pieces.dim() != 1 or pieces.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or piece_off.dim() != 1 or piece_off.dtype != torch.int32 \
            or piece_off.shape[0] < 2:
        raise ValueError("text_units: the piece table is pieces (int32 / uint32 [n]) and piece_off (int32 [V + 2]), got %s %s and %s %s"
                         % (pieces.dtype, tuple(pieces.shape), piece_off.dtype, tuple(piece_off.shape)))
    V = piece_off.shape[0] - 2
    if unk >= V:
        raise ValueError("text_units: unk must be a token of the table's %d (or negative), got %d" % (V, unk))
    dev = hyp.device
    hyp_units = torch.empty((P, Uh), dtype=torch.int32, device=dev)          # written up to hyp_n
    ref_units = torch.empty((P, Ur), dtype=torch.int32, device=dev)
    hyp_n = torch.empty((P,), dtype=torch.int32, device=dev)                 # the kernel writes every element of these three
    ref_n = torch.empty((P,), dtype=torch.int32, device=dev)
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    if P == 0:
        return hyp_units, hyp_n, ref_units, ref_n, status
    p = _ptr_or(torch.zeros((2,), dtype=torch.int64, device=dev))
    L.check(_lib().s2t_text_units(p(hyp), p(hyp_len), hyp.element_size(), p(ref), p(ref_len), ref.element_size(),
                                  L.ptr(hyp_row.contiguous()) if hyp_row is not None else 0,
                                  L.ptr(ref_row.contiguous()) if ref_row is not None else 0, P, Hmax, Rmax, Hrows, Rrows,
                                  p(pieces.contiguous()), L.ptr(piece_off.contiguous()), pieces.shape[0], V, unk, mode, Uh, Ur,
                                  p(hyp_units), p(ref_units), L.ptr(hyp_n), L.ptr(ref_n), L.ptr(status), L.stream()), "s2t_text_units")
    return hyp_units, hyp_n, ref_units, ref_n, status


FBANK_MAX_BINS = 128              # S2T_FBANK_MAX_BINS of include/s2t_hip.h
FBANK_TILE_ELEMS = 8192           # S2T_FBANK_TILE_ELEMS: a workgroup takes FBANK_TILE_ELEMS // N consecutive frames
FBANK_FFT_SIZES = (256, 512, 1024)


def fbank_frame_tile(N):
    """S2T_FBANK_FRAME_TILE(N): the frames one workgroup of s2t_fbank takes"""
    return FBANK_TILE_ELEMS // N


def fbank(waves, wave_len, window, twiddle, bank, weights, S, N, preemph=0.97, remove_dc=True):
    """log-mel filterbanks of the rows of waves [B, Nmax] (int16 or float32, unit stride inside a row, any row stride; the first
    wave_len[b] samples, wave_len int64 [B]): include/s2t_hip.h s2t_fbank states the rule.  window float32 [W], twiddle float64 [N],
    bank int32 [F, 3] and weights float32 [n] are the host-built tables (fbank.FbankFrontEnd makes them); S the shift in samples,
    N the FFT size.  Returns device tensors (out f32 [B, Tmax, F] with zeros behind a sentence's frames, out_len int32 [B], status
    int32 [B]: 0 done / 1 no frames / 2 refused)."""
    if waves.dim() != 2 or waves.dtype not in (torch.int16, torch.float32):
        raise ValueError("fbank: waves must be int16 or float32 [B, Nmax], got %s %s" % (waves.dtype, tuple(waves.shape)))
    B, Nmax = waves.shape
    if tuple(wave_len.shape) != (B,) or wave_len.dtype != torch.int64:
        raise ValueError("fbank: wave_len must be int64 [%d], got %s %s" % (B, wave_len.dtype, tuple(wave_len.shape)))
    S, N = int(S), int(N)
    if N not in FBANK_FFT_SIZES:
        raise ValueError("fbank: FFT sizes %s, got %d" % (FBANK_FFT_SIZES, N))
    if window.dim() != 1 or window.dtype != torch.float32 or not N // 2 < window.shape[0] <= N:
        raise ValueError("fbank: window must be float32 [W] with %d < W <= %d, got %s %s" % (N // 2, N, window.dtype, tuple(window.shape)))
    if tuple(twiddle.shape) != (N,) or twiddle.dtype != torch.float64:
        raise ValueError("fbank: twiddle must be float64 [%d], got %s %s" % (N, twiddle.dtype, tuple(twiddle.shape)))
    if bank.dim() != 2 or bank.shape[1] != 3 or bank.dtype != torch.int32 or not 1 <= bank.shape[0] <= FBANK_MAX_BINS:
        raise ValueError("fbank: bank must be int32 [F, 3] with 1 <= F <= %d (S2T_FBANK_MAX_BINS), got %s %s"
                         % (FBANK_MAX_BINS, bank.dtype, tuple(bank.shape)))
    if weights.dim() != 1 or weights.dtype != torch.float32 or weights.shape[0] > N:
        raise ValueError("fbank: weights must be float32 [n] with n <= %d, got %s %s" % (N, weights.dtype, tuple(weights.shape)))
    if S < 1:
        raise ValueError("fbank: a shift of at least one sample, got %d" % S)
    preemph = float(preemph)
    if not 0.0 <= preemph <= 1.0:
        raise ValueError("fbank: preemphasis in [0, 1], got %r" % (preemph,))
    W, F = window.shape[0], bank.shape[0]
    Tmax = 0 if Nmax < W else 1 + (Nmax - W) // S
    dev = waves.device
    out = torch.empty((B, Tmax, F), dtype=torch.float32, device=dev)
    out_len = torch.empty((B,), dtype=torch.int32, device=dev)       # both are written for every sentence
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out, out_len, status
    if Nmax > 1 and waves.stride(1) != 1:
        waves = waves.contiguous()
    row_stride = waves.stride(0) if B > 1 and Nmax else Nmax
    if row_stride < 0:
        waves, row_stride = waves.contiguous(), Nmax
    # an empty tensor has no address and the entry point refuses NULL; nothing of a zero-width operand is read or written
    fill = torch.zeros((2,), dtype=torch.float32, device=dev)
    p = lambda t: L.ptr(t if t.numel() else fill)
    L.check(_lib().s2t_fbank(p(waves), waves.element_size(), row_stride, L.ptr(wave_len.contiguous()), B, Nmax, W, S, N, F, Tmax,
                             L.ptr(window.contiguous()), L.ptr(twiddle.contiguous()), L.ptr(bank.contiguous()), p(weights.contiguous()),
                             weights.shape[0], int(bool(remove_dc)), preemph, p(out), L.ptr(out_len), L.ptr(status), L.stream()),
            "s2t_fbank")
    return out, out_len, status


def cmvn(x, lengths):
    """per-utterance mean / variance normalisation of x [B, Tmax, F] (float32, contiguous) over its first lengths[b] rows (int32 or
    int64 [B]), IN PLACE: include/s2t_hip.h s2t_cmvn states the rule.  Returns device tensors (out_len int32 [B], status int32 [B]:
    0 done / 1 fewer than two rows / 2 refused); rows at or behind out_len[b] are zeros."""
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("cmvn: x must be a contiguous float32 [B, Tmax, F], got %s %s" % (x.dtype, tuple(x.shape)))
    B, Tmax, F = x.shape
    if tuple(lengths.shape) != (B,) or lengths.dtype not in (torch.int32, torch.int64):
        raise ValueError("cmvn: lengths must be int32 / int64 [%d], got %s %s" % (B, lengths.dtype, tuple(lengths.shape)))
    if not 1 <= F <= FBANK_MAX_BINS:
        raise ValueError("cmvn: 1 to %d columns (S2T_FBANK_MAX_BINS), got %d" % (FBANK_MAX_BINS, F))
    dev = x.device
    out_len = torch.empty((B,), dtype=torch.int32, device=dev)       # both are written for every sentence
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out_len, status
    lengths = lengths.contiguous()
    fill = torch.zeros((2,), dtype=torch.float32, device=dev)      # Tmax = 0: nothing of x is read or written
    L.check(_lib().s2t_cmvn(L.ptr(x if x.numel() else fill), L.ptr(lengths), lengths.element_size(), B, Tmax, F, L.ptr(out_len),
                            L.ptr(status), L.stream()), "s2t_cmvn")
    return out_len, status


RESAMPLE_MAX_BANKS = 8            # S2T_RESAMPLE_MAX_BANKS of include/s2t_hip.h: the banks of one call's table
RESAMPLE_BANK_INTS = 7            # S2T_RESAMPLE_BANK_INTS: (in_unit, out_unit, taps, first_off, w_off, lo, extra)
RESAMPLE_REUSE = 4                # S2T_RESAMPLE_REUSE: outputs of one phase a thread produces from one read of the weights
RESAMPLE_TILE_ITEMS = 512         # S2T_RESAMPLE_TILE_ITEMS: (phase, unit group) pairs of a workgroup's tile
RESAMPLE_MAX_PHASES = 512         # S2T_RESAMPLE_MAX_PHASES: out_unit
RESAMPLE_MAX_BANK = 8192          # S2T_RESAMPLE_MAX_BANK: taps * out_unit, the weights of a bank
RESAMPLE_MAX_SPAN = 7672          # S2T_RESAMPLE_MAX_SPAN: the samples a workgroup stages


def resample_group(in_unit, out_unit, extra):
    """the unit groups G of a workgroup's tile of s2t_resample for a bank (0: the bank does not fit)"""
    if in_unit == out_unit:
        return RESAMPLE_TILE_ITEMS
    by_span = 0 if extra > RESAMPLE_MAX_SPAN else ((RESAMPLE_MAX_SPAN - extra) // in_unit + 1) // RESAMPLE_REUSE
    return min(RESAMPLE_TILE_ITEMS // out_unit, by_span)


def resample_tile(in_unit, out_unit, extra):
    """the outputs of a workgroup's tile of s2t_resample for a bank"""
    g = resample_group(in_unit, out_unit, extra)
    return RESAMPLE_REUSE * g * (1 if in_unit == out_unit else out_unit)


def resample_check_banks(banks, n_first, n_weights):
    """the limits of s2t_resample on a table's banks (int32 [R, RESAMPLE_BANK_INTS], host), as ValueErrors"""
    if banks.dim() != 2 or banks.shape[1] != RESAMPLE_BANK_INTS or banks.dtype != torch.int32 or banks.is_cuda or banks.shape[0] < 1:
        raise ValueError("resample: banks must be a host int32 [R, %d] with R >= 1, got %s %s" % (RESAMPLE_BANK_INTS, banks.dtype, tuple(banks.shape)))
    if banks.shape[0] > RESAMPLE_MAX_BANKS:
        raise ValueError("resample: at most %d banks in a table (S2T_RESAMPLE_MAX_BANKS), got %d" % (RESAMPLE_MAX_BANKS, banks.shape[0]))
    for r, (iu, ou, taps, f_off, w_off, lo, extra) in enumerate(banks.tolist()):
        if iu < 1 or ou < 1:
            raise ValueError("resample: bank %d: units of at least 1, got %d and %d" % (r, iu, ou))
        if iu == ou:
            continue
        if taps < 1 or extra < taps or f_off < 0 or w_off < 0 or f_off + ou > n_first or w_off + taps * ou > n_weights or abs(lo) >= 1 << 30:
            raise ValueError("resample: bank %d does not describe its tables: %r with %d firsts and %d weights"
                             % (r, (iu, ou, taps, f_off, w_off, lo, extra), n_first, n_weights))
        if ou > RESAMPLE_MAX_PHASES:
            raise ValueError("resample: bank %d: %d phases, at most %d (S2T_RESAMPLE_MAX_PHASES)" % (r, ou, RESAMPLE_MAX_PHASES))
        if taps * ou > RESAMPLE_MAX_BANK:
            raise ValueError("resample: bank %d: %d weights (%d phases of %d taps), at most %d (S2T_RESAMPLE_MAX_BANK)"
                             % (r, taps * ou, ou, taps, RESAMPLE_MAX_BANK))
        if resample_group(iu, ou, extra) < 1:
            raise ValueError("resample: bank %d: %d units span %d samples, at most %d are staged (S2T_RESAMPLE_MAX_SPAN)"
                             % (r, RESAMPLE_REUSE, (RESAMPLE_REUSE - 1) * iu + extra, RESAMPLE_MAX_SPAN))


def resample(waves, wave_len, banks, first, weights, Mmax, ratio_id=None):
    """sinc resampling of the rows of waves [B, Nmax] (int16 or float32, unit stride inside a row, any row stride; the first
    wave_len[b] samples, wave_len int32 or int64 [B]): include/s2t_hip.h s2t_resample states the rule.  banks is the HOST int32
    [R, RESAMPLE_BANK_INTS] table, first int32 [n] and weights float32 [n] its device arrays (resample.pack_table makes them);
    ratio_id int32 [B] picks a row's bank (None: bank 0); Mmax the width of the result.  Returns device tensors (out f32 [B, Mmax]
    with zeros behind a row's samples, out_len int64 [B], status int32 [B]: 0 done / 1 no samples / 2 refused)."""
    if waves.dim() != 2 or waves.dtype not in (torch.int16, torch.float32):
        raise ValueError("resample: waves must be int16 or float32 [B, Nmax], got %s %s" % (waves.dtype, tuple(waves.shape)))
    B, Nmax = waves.shape
    if tuple(wave_len.shape) != (B,) or wave_len.dtype not in (torch.int32, torch.int64):
        raise ValueError("resample: wave_len must be int32 / int64 [%d], got %s %s" % (B, wave_len.dtype, tuple(wave_len.shape)))
    if ratio_id is not None and (tuple(ratio_id.shape) != (B,) or ratio_id.dtype != torch.int32):
        raise ValueError("resample: ratio_id must be int32 [%d], got %s %s" % (B, ratio_id.dtype, tuple(ratio_id.shape)))
    if first.dim() != 1 or first.dtype != torch.int32 or weights.dim() != 1 or weights.dtype != torch.float32:
        raise ValueError("resample: first must be int32 [n] and weights float32 [n], got %s %s and %s %s"
                         % (first.dtype, tuple(first.shape), weights.dtype, tuple(weights.shape)))
    resample_check_banks(banks, first.shape[0], weights.shape[0])
    Mmax = int(Mmax)
    if not 0 <= Mmax < 1 << 31 or Nmax >= 1 << 31:
        raise ValueError("resample: widths below 2^31, got Nmax %d and Mmax %d" % (Nmax, Mmax))
    dev = waves.device
    out = torch.empty((B, Mmax), dtype=torch.float32, device=dev)
    out_len = torch.empty((B,), dtype=torch.int64, device=dev)       # both are written for every row
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out, out_len, status
    if Nmax > 1 and waves.stride(1) != 1:
        waves = waves.contiguous()
    row_stride = waves.stride(0) if B > 1 and Nmax else Nmax
    if row_stride < 0:
        waves, row_stride = waves.contiguous(), Nmax
    banks = banks.contiguous()
    # an empty tensor has no address and the entry point refuses NULL; nothing of a zero-width operand is read or written
    fill = torch.zeros((4,), dtype=torch.float32, device=dev)
    p = lambda t: L.ptr(t if t.numel() else fill)
    L.check(_lib().s2t_resample(p(waves), waves.element_size(), row_stride, L.ptr(wave_len.contiguous()), wave_len.element_size(),
                                L.ptr(ratio_id.contiguous()) if ratio_id is not None else 0, B, Nmax, Mmax, banks.data_ptr(), banks.shape[0],
                                p(first.contiguous()), first.shape[0], p(weights.contiguous()), weights.shape[0], p(out), L.ptr(out_len),
                                L.ptr(status), L.stream()), "s2t_resample")
    return out, out_len, status


def embed_bwd(tokens, dout, dW, scale, pad):
    B, Ln = tokens.shape
    D = dW.shape[1]
    L.check(_lib().s2t_embed_bwd(L.dt(dout), L.ptr(tokens), L.ptr(dout), L.ptr(dW), B, Ln, D, float(scale), pad, L.stream()),
            "s2t_embed_bwd")


def act_bwd(dy, y, act, p_drop=0.0, seed=0):
    """dropout(dy) * act'(y): the backward of act followed by a dropout, one pass"""
    assert dy.is_contiguous() and y.is_contiguous() and dy.dtype == y.dtype and dy.numel() == y.numel()
    out = torch.empty_like(dy)
    L.check(_lib().s2t_act_bwd(L.dt(dy), L.ptr(dy), L.ptr(y), L.ptr(out), dy.numel(), act, float(p_drop), int(seed), L.stream()), "s2t_act_bwd")
    return out


def add_inplace(x, y):
    """y += x"""
    assert x.numel() == y.numel() and x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous()
    L.check(_lib().s2t_add_inplace(L.dt(y), L.ptr(x), L.ptr(y), y.numel(), L.stream()), "s2t_add_inplace")
    return y


def dropout(x, p, seed, out=None):
    if out is None:
        out = torch.empty_like(x)
    L.check(_lib().s2t_dropout(L.dt(x), L.ptr(x), L.ptr(out), x.numel(), float(p), int(seed), L.stream()), "s2t_dropout")
    return out


def grad_norm_clip(g, scale, max_norm, ws, out2, divisor=None):
    """divisor: f64 device scalar the gradients are also divided by (max(divisor, 1)): the all-reduced sample size, never read by the host"""
    if divisor is not None:
        assert divisor.dtype == torch.float64 and divisor.numel() == 1
        L.check(_lib().s2t_grad_norm_clip_div(L.ptr(g), g.numel(), L.ptr(ws), float(scale), L.ptr(divisor), float(max_norm), L.ptr(out2),
                                              L.stream()), "s2t_grad_norm_clip_div")
        return out2
    L.check(_lib().s2t_grad_norm_clip(L.ptr(g), g.numel(), L.ptr(ws), float(scale), float(max_norm), L.ptr(out2), L.stream()),
            "s2t_grad_norm_clip")
    return out2


def adam_step(p, g, m, v, shadow, mult2, lr, beta1, beta2, eps, wd, step):
    L.check(_lib().s2t_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(shadow), p.numel(), L.ptr(mult2), float(lr),
                                 float(beta1), float(beta2), float(eps), float(wd), int(step), L.stream()), "s2t_adam_step")


def cast(src, dst):
    assert src.numel() == dst.numel()
    L.check(_lib().s2t_cast(L.dt(src), L.dt(dst), L.ptr(src), L.ptr(dst), src.numel(), L.stream()), "s2t_cast")
    return dst


def scale_by_device_scalar(x, scalar):
    d = x if x.is_contiguous() else x._base           # row-padded views: scale the whole backing buffer
    assert d is not None and d.is_contiguous()
    L.check(_lib().s2t_scale_by_device_scalar(L.dt(d), L.ptr(d), d.numel(), L.ptr(scalar), L.stream()), "s2t_scale")
    return x


def host_ctc_uer(pred_cpu, in_len_cpu, targets_cpu, tgt_len_cpu, blank):
    """HOST tensors (int32 pred [B,T], int64 others) -> (errors, total)."""
    B, T = pred_cpu.shape
    e, n = ctypes.c_double(0), ctypes.c_double(0)
    pred_cpu = pred_cpu.contiguous(); targets_cpu = targets_cpu.contiguous()
    L.check(_lib().s2t_host_ctc_uer(pred_cpu.data_ptr(), in_len_cpu.contiguous().data_ptr(), B, T, targets_cpu.data_ptr(),
                                    tgt_len_cpu.contiguous().data_ptr(), targets_cpu.shape[1], blank,
                                    ctypes.addressof(e), ctypes.addressof(n)), "s2t_host_ctc_uer")
    return e.value, n.value


OPTION_EPOCH = 0          # bumps with every set_option: sizes that depend on the kernel routes (the engine's cached workspace sizes) key on it


def set_option(key, value):
    """kernel-route option of the library (include/s2t_hip.h, s2t_set_option); returns the previous value"""
    global OPTION_EPOCH
    old = _lib().s2t_set_option(key.encode(), int(value))
    if old == -22:
        raise ValueError("unknown libs2t_hip option %r (or a value out of its range)" % key)
    OPTION_EPOCH += 1
    return old


def prof_enable(on):
    _lib().s2t_prof_enable(int(on))


def prof_reset():
    _lib().s2t_prof_reset()


def prof_read(family):
    ms, fl, by = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
    n = ctypes.c_longlong(0)
    _lib().s2t_prof_read(family.encode(), ctypes.addressof(ms), ctypes.addressof(n), ctypes.addressof(fl), ctypes.addressof(by))
    return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)


# ------------------------------------------------------------------ ConvAttention2D pieces (csrc/attn2d.hip)
def a2d_chan_stats(z, C, Cg, prescale=None, dy=None, bn=None):
    """z [M, ld] channels-last; returns double sums in groups of Cg ([Cg | Cg] each).  dy + bn=(mean, rstd, scale, shift): backward sums."""
    M = z.shape[0]
    sums = torch.zeros((2 * C,), dtype=torch.float64, device=z.device)
    mean, rstd, scale, shift = bn if bn is not None else (None, None, None, None)
    L.check(_lib().s2t_a2d_chan_stats(L.dt(z), L.ptr(z), L.ptr(dy), L.ptr(prescale), L.ptr(mean), L.ptr(rstd), L.ptr(scale), L.ptr(shift),
                                      L.ptr(sums), M, C, z.stride(0), dy.stride(0) if dy is not None else 0, Cg,
                                      0 if dy is None else 1, L.stream()), "s2t_a2d_chan_stats")
    return sums


def a2d_bn_act(z, C, scale, shift, prescale=None, res=None, out=None):
    M = z.shape[0]
    if out is None:
        out = torch.zeros_like(z) if res is None else torch.empty_like(res)
    assert res is None or res.stride(0) == out.stride(0)
    L.check(_lib().s2t_a2d_bn_act(L.dt(z), L.ptr(z), L.ptr(prescale), L.ptr(scale), L.ptr(shift), L.ptr(res), L.ptr(out), M, C,
                                  z.stride(0), out.stride(0), L.stream()), "s2t_a2d_bn_act")
    return out


def a2d_bn_bwd(dy, z, C, Cg, bn, sums, count, training, prescale=None):
    mean, rstd, scale, shift = bn
    dz = torch.zeros_like(z)
    L.check(_lib().s2t_a2d_bn_bwd(L.dt(z), L.ptr(dy), L.ptr(z), L.ptr(prescale), L.ptr(mean), L.ptr(rstd), L.ptr(scale), L.ptr(shift),
                                  L.ptr(sums), L.ptr(dz), z.shape[0], C, dy.stride(0), z.stride(0), Cg, float(count), int(training),
                                  L.stream()), "s2t_a2d_bn_bwd")
    return dz


def a2d_param_grads(sums, dgamma, dbeta):
    L.check(_lib().s2t_a2d_param_grads(L.ptr(sums), L.ptr(dgamma), L.ptr(dbeta), dgamma.numel(), L.stream()), "s2t_a2d_param_grads")


def a2d_pack_w(w, rows, CP, dtype, mode):
    """mode 0 / 1: packed operand [rows, 9*CP] of the forward / data-gradient gathered GEMM from nn.Conv2d weights [Co,Ci,3,3]."""
    Co, Ci = w.shape[0], w.shape[1]
    dst = torch.zeros((rows, 9 * CP), dtype=dtype, device=w.device)
    L.check(_lib().s2t_a2d_pack_w(L.dt(dst), L.ptr(w), L.ptr(dst), 0, Co, Ci, CP, dst.stride(0), mode, L.stream()), "s2t_a2d_pack_w")
    return dst


def a2d_unpack_wgrad(gp, grad, CP):
    """grad[Co,Ci,3,3] += gp[Co, 9*CP] (f32)"""
    Co, Ci = grad.shape[0], grad.shape[1]
    assert gp.dtype == torch.float32 and grad.dtype == torch.float32
    L.check(_lib().s2t_a2d_pack_w(L.F32, L.ptr(gp), 0, L.ptr(grad), Co, Ci, CP, gp.stride(0), 2, L.stream()), "s2t_a2d_pack_w")


def a2d_time_fwd(qkv, cat, B, T, F, p_drop=0.0, seed=0):
    lse = torch.empty((B * 4, T), dtype=torch.float32, device=qkv.device)
    L.check(_lib().s2t_a2d_time_fwd(L.dt(qkv), L.ptr(qkv), L.ptr(cat), L.ptr(lse), B, T, F, float(p_drop), int(seed), L.stream()),
            "s2t_a2d_time_fwd")
    return lse


def a2d_time_bwd(qkv, cat, dcat, lse, dqkv, B, T, F, p_drop=0.0, seed=0):
    delta = torch.empty_like(lse)
    L.check(_lib().s2t_a2d_time_bwd(L.dt(qkv), L.ptr(qkv), L.ptr(cat), L.ptr(dcat), L.ptr(lse), L.ptr(delta), L.ptr(dqkv), B, T, F,
                                    float(p_drop), int(seed), L.stream()), "s2t_a2d_time_bwd")
    return delta


def a2d_freq_fwd(qkv, cat, B, T, F, p_drop=0.0, seed=0):
    A = torch.empty((B * 4, F, F), dtype=torch.float32, device=qkv.device)
    L.check(_lib().s2t_a2d_freq_fwd(L.dt(qkv), L.ptr(qkv), L.ptr(cat), L.ptr(A), B, T, F, float(p_drop), int(seed), L.stream()),
            "s2t_a2d_freq_fwd")
    return A


def a2d_freq_bwd(qkv, dcat, A, dqkv, B, T, F, p_drop=0.0, seed=0):
    L.check(_lib().s2t_a2d_freq_bwd(L.dt(qkv), L.ptr(qkv), L.ptr(dcat), L.ptr(A), L.ptr(dqkv), B, T, F, float(p_drop), int(seed),
                                    L.stream()), "s2t_a2d_freq_bwd")


def a2d_conv_wgrad(dy, x, grad, B, T, F):
    """grad[Co,Ci,3,3] += conv-weight gradient from dy [M, >=Co] and x [M, Ci] (pixel rows (t, b, f)); False when the shape is not built"""
    Co, Ci = grad.shape[0], grad.shape[1]
    assert grad.dtype == torch.float32 and grad.is_contiguous() and dy.dtype == x.dtype
    ws = torch.empty((512, max(Co, 16) * Ci * 9), dtype=torch.float32, device=x.device)      # S2T_A2D_WGRAD_GROUPS partial sums
    rc = _lib().s2t_a2d_conv_wgrad(L.dt(x), L.ptr(dy), dy.stride(0), L.ptr(x), x.stride(0), L.ptr(grad), L.ptr(ws), Co, Ci, B, T, F,
                                   L.stream())
    if rc == -95:
        return False
    L.check(rc, "s2t_a2d_conv_wgrad")
    return True


def a2d_planes(chl, planes, ch0, B, T, F, to_planes):
    """chl [M, ld] channels-last pixel rows <-> planes [G, T, B, 128] (head-major, F columns of 32 used per head)"""
    G = planes.shape[0]
    assert planes.is_contiguous() and planes.shape[1:] == (T, B, 128) and chl.stride(1) == 1 and planes.dtype == chl.dtype
    L.check(_lib().s2t_a2d_planes(L.dt(chl), L.ptr(chl), L.ptr(planes), G, ch0, chl.stride(0), B, T, F, 0 if to_planes else 1, L.stream()),
            "s2t_a2d_planes")
    return planes if to_planes else chl
