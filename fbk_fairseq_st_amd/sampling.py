"""Host restatement (numpy) of the draw of the sampling search -- csrc/sample.hpp, described in include/s2t_hip.h: the hash and the
uniform bit for bit, the kept sets by sorting, the Gumbel keys in float32.  `Sampling.step` (sequence_generator.py) runs it on host
tensors; device tensors go through `kernels.sample_rows`, the device-resident search through the SAMPLE forms of csrc/decode.hip.

The reference (fairseq/search.py:164-278) draws with torch.multinomial, whose stream cannot be reproduced; what is the same is the
distribution: a token of the kept set with probability proportional to exp(lp).  Two stated deviations: the score of a token is lp
itself where the reference returns log(exp(lp)) (at most 1 ulp away), and a row without a finite column gives token 0 with score -inf
where the reference raises.
"""
import numpy as np

_M = np.uint64(0xFFFFFFFF)


def mix32(x):
    """csrc/common.hpp mix32 on uint64 arrays holding 32-bit values"""
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & _M
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & _M
    return x ^ (x >> np.uint64(16))


def make_key(seed, call):
    """the 64-bit key of one `generate` call: the seed in the high word, the call counter in the low one"""
    return ((int(seed) & 0xFFFFFFFF) << 32) | (int(call) & 0xFFFFFFFF)


def hash32(key, step, slot, col):
    """csrc/sample.hpp row_key + hash32; key a Python int (64 bits), the others broadcast as integer arrays -> uint32"""
    u = lambda v: np.asarray(v, dtype=np.int64).astype(np.uint64) & _M
    lo, hi = np.uint64(int(key) & 0xFFFFFFFF), np.uint64((int(key) >> 32) & 0xFFFFFFFF)
    step, slot, col = u(step), u(slot), u(col)
    a = mix32(lo ^ np.uint64(0x9E3779B9)); a = mix32((a + hi) & _M); a = mix32((a + step) & _M); a = mix32((a + slot) & _M)
    b = mix32(hi ^ np.uint64(0x85EBCA6B)); b = mix32((b + lo) & _M); b = mix32((b + slot) & _M); b = mix32((b + step) & _M)
    return mix32((mix32(col ^ a) + b) & _M).astype(np.uint32)


def uniform(h):
    """((h >> 9) + 0.5) * 2^-23 = (2k + 1) * 2^-24: exact in float32, never 0 or 1"""
    return ((h >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def kept_set(lp, topk, topp):
    """lp float32 [V] -> bool [V].  Order: value descending, column ascending.  topp > 0 first (a column is kept iff the mass strictly
    before it is < topp), else topk > 0 (the first topk), else everything; only finite columns."""
    lp = np.asarray(lp, np.float32)
    fin = lp > -np.inf
    keep = np.zeros(lp.shape, bool)
    order = np.lexsort((np.arange(lp.shape[0]), -lp.astype(np.float64)))
    order = order[fin[order]]
    if topp > 0:
        p = np.exp(lp[order]).astype(np.float32).astype(np.float64)
        before = np.concatenate([[0.0], np.cumsum(p)[:-1]]) if order.size else p
        order = order[before < np.float64(np.float32(topp))]
    elif topk > 0:
        order = order[:int(topk)]
    keep[order] = True
    return keep


def gumbel_keys(lp, key, step, slot):
    """lp float32 [V] -> float32 [V] keys lp + g, g = -log(-log(u)); -inf stays -inf"""
    lp = np.asarray(lp, np.float32)
    u = uniform(hash32(key, step, slot, np.arange(lp.shape[0])))
    with np.errstate(divide="ignore"):
        g = -np.log(-np.log(u))
    return (lp + g.astype(np.float32)).astype(np.float32)


def draw(lp, keep, key, step, slot):
    """the token of slot `slot`: arg-max of the keys over the kept columns (the smaller column on ties); 0 when nothing is kept"""
    if not keep.any():
        return 0
    k = np.where(keep, gumbel_keys(lp, key, step, slot), -np.inf)
    return int(np.argmax(k))                                              # numpy's arg-max returns the first of equal maxima
