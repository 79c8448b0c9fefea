"""The dropout rule, restated once on the host (numpy, uint64 arithmetic masked to 32 bits) from csrc/common.hpp (mix32,
drop_seed_key, drop_high_mix, drop_hash4_lo, drop_field, dropout_keep) and csrc/loss_embed.hip (dropout_kernel).  The tests hold the
device to THIS statement, bit for bit; nothing here is shared with tools/drop_hash_check.py, which test_dropout_ref_cpu.py uses as a
second statement by another hand.

    ks   = mix32(lo32(seed) * 0x9E3779B9 + 0x7F4A7C15)
    hw   = hi32(quad) + hi32(seed);  hwm = hw ^ hw << 13 ^ hw >> 7 ^ hw << 27
    a    = lo32(quad) ^ ks;  three rounds a = bitrev(a + (a mod 2^24) * C), the last one without the reversal;  a ^= a >> 16
    x    = a ^ hwm;  y = bitrev(x + ((x ^ 0x68E31DA4) mod 2^24) * 0xC2B2AE)
    element 4 quad + f draws field f:  f0 = y.lo, f1 = y.hi, f2 = x.lo, f3 = x.hi  (16 bits each)
    kept  <=>  field >= th16,  th16 = trunc(min(f32(p) * 2^32, 2^32)) >> 16, all of it in f32

Index bits >= 34 (quad bits >= 32) and seed bits >= 32 enter only through `x ^ hwm`, after the mixing: two masks that differ only
there are correlated (test_dropout_ref_cpu.py records by how much).  Indices >= 2^34 are evaluated here on the CPU only; no GPU test
allocates the 32 GB tensor that would reach them.

Four deliberately wrong twins (TWINS) serve as negative controls: each differs from the rule in one place where a kernel could."""
import numpy as np
import torch

M32 = np.uint64(0xFFFFFFFF)
M24 = np.uint64(0xFFFFFF)
M16 = np.uint64(0xFFFF)


def _u64(v):
    if isinstance(v, np.ndarray):
        return v.astype(np.uint64)
    return np.uint64(int(v))


def _sh(k):
    return np.uint64(k)


def mix32(x):
    x = _u64(x) & M32
    x = x ^ (x >> _sh(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> _sh(15)); x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> _sh(16))


def bitrev32(a):
    a = _u64(a) & M32
    for k, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0F0F0F0F), (8, 0x00FF00FF), (16, 0x0000FFFF)):
        m = np.uint64(m)
        a = ((a >> _sh(k)) & m) | ((a & m) << _sh(k))
    return a & M32


def seed_key(seed):
    lo = _u64(seed) & M32
    return mix32((lo * np.uint64(0x9E3779B9) + np.uint64(0x7F4A7C15)) & M32)


class Rule:
    """the rule; the keyword arguments switch on one deliberate mistake each (the twins)"""

    def __init__(self, name="rule", fields_x_first=False, ignore_seed_high=False, full_multiply=False, strict_greater=False):
        self.name = name
        self.fields_x_first, self.ignore_seed_high = fields_x_first, ignore_seed_high
        self.full_multiply, self.strict_greater = full_multiply, strict_greater

    def high_mix(self, seed, quad):
        sh = np.uint64(0) if self.ignore_seed_high else (_u64(seed) >> _sh(32))
        hw = ((_u64(quad) >> _sh(32)) + sh) & M32
        return hw ^ ((hw << _sh(13)) & M32) ^ (hw >> _sh(7)) ^ ((hw << _sh(27)) & M32)

    def _mad(self, a, c, add):
        """add + (a mod 2^24) * c in 32 bits (v_mad_u32_u24)"""
        m = a if self.full_multiply else (a & M24)
        return (m * np.uint64(c) + add) & M32

    def hash4_lo(self, ks, hwm, quad_lo):
        a = (_u64(quad_lo) & M32) ^ _u64(ks)
        a = bitrev32(self._mad(a, 0x3C6EF2, a))
        a = bitrev32(self._mad(a, 0x9E3778, a))
        a = self._mad(a, 0x85EBCA, a)
        a = a ^ (a >> _sh(16))
        x = a ^ _u64(hwm)
        y = bitrev32(self._mad(x ^ np.uint64(0x68E31DA4), 0xC2B2AE, x))
        return x, y

    def hash4(self, seed, quad):
        quad = _u64(quad)
        return self.hash4_lo(seed_key(seed), self.high_mix(seed, quad), quad & M32)

    def field(self, x, y, f):
        """16-bit uniform of element f (0..3) of the quad: f0 = y.lo, f1 = y.hi, f2 = x.lo, f3 = x.hi"""
        f = _u64(f)
        second = (f & np.uint64(2)) != 0
        w = np.where(second != self.fields_x_first, x, y)
        return np.where((f & np.uint64(1)) != 0, w >> _sh(16), w & M16)

    def fields(self, seed, idx):
        idx = _u64(np.asarray(idx))
        x, y = self.hash4(seed, idx >> _sh(2))
        return self.field(x, y, idx & np.uint64(3))

    def _cmp(self, fld, p):
        t = np.uint64(th16(p))
        return (fld > t) if self.strict_greater else (fld >= t)

    def keep(self, seed, idx, p):
        """keep decisions of the elements `idx` (any uint64 array, any order)"""
        return self._cmp(self.fields(seed, idx), p)

    def keep_range(self, seed, n, p):
        """keep(seed, arange(n), p), one hash per quad as the kernels evaluate it"""
        x, y = self.hash4(seed, np.arange((n + 3) // 4, dtype=np.uint64))
        f = np.stack([self.field(x, y, np.uint64(e)) for e in range(4)], 1).reshape(-1)[:n]
        return self._cmp(f, p)

    def apply(self, x, seed, p):
        """dropout_kernel on a flat f32 / bf16 host tensor: a kept element is f32(x) * (1 / (1 - p)), the product taken in f32 and
        rounded once to the type; a dropped element is +0, whatever x was (negative, infinite, NaN)"""
        assert x.dim() == 1 and x.dtype in (torch.float32, torch.bfloat16)
        kp = torch.from_numpy(self.keep_range(seed, x.numel(), p))
        inv = torch.tensor(float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), dtype=torch.float32)
        return torch.where(kp, (x.float() * inv).to(x.dtype), torch.zeros((), dtype=x.dtype))


def th16(p):
    """the 16-bit threshold of rate p: p as the f32 the ABI passes, times 2^32 in f32, clamped, truncated, >> 16"""
    t = np.float32(p) * np.float32(4294967296.0)
    t = min(t, np.float32(4294967295.0))                   # the f32 nearest to 2^32 - 1 is 2^32: reached by no p < 1
    return min(int(t), 0xFFFFFFFF) >> 16


RULE = Rule()
TWINS = {
    "fields_x_first": Rule("fields_x_first", fields_x_first=True),         # fields read as x.lo, x.hi, y.lo, y.hi
    "ignore_seed_high": Rule("ignore_seed_high", ignore_seed_high=True),   # seed >> 32 ignored
    "full_multiply": Rule("full_multiply", full_multiply=True),            # the 24-bit mask of the multiply-add dropped
    "strict_greater": Rule("strict_greater", strict_greater=True),         # > instead of >= against th16
}

# the case on which both test files separate the twins from the rule: a seed >= 2^32 for `ignore_seed_high`, and n = 2^20 at
# p = 0.25, where about 2^20 / 65536 = 16 fields equal th16, for `strict_greater` (test_dropout_ref_cpu.py asserts that there is one)
CONTROL = dict(n=2 ** 20, p=0.25, seed=(5 << 32) | 7)


# the rule's functions by name (RULE is looked up at call time)
def high_mix(seed, quad): return RULE.high_mix(seed, quad)
def hash4(seed, quad): return RULE.hash4(seed, quad)
def field(x, y, f): return RULE.field(x, y, f)
def keep(seed, idx, p): return RULE.keep(seed, idx, p)
def keep_range(seed, n, p): return RULE.keep_range(seed, n, p)
def apply(x, seed, p): return RULE.apply(x, seed, p)
