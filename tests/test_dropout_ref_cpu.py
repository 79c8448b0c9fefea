"""tests/dropout_ref.py, the host statement of the dropout rule that test_dropout_hash_gpu.py holds s2t_dropout to, checked on its
own: against the second statement of the per-quad hash in tools/drop_hash_check.py, at the threshold's edges, for its keep rate, as a
function of (seed, index), and against its four deliberately wrong twins, which must differ from it on the very arrays the GPU test
compares -- so that a GPU pass cannot be a twin's pass."""
import ast
import math
import os

import numpy as np
import pytest
import torch

import dropout_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 5, 6, 1000003000, 2 ** 32 + 5, (5 << 32) | 7, (1 << 63) | 12345, 2 ** 64 - 1]
RATES = [2.0 ** -17, 2.0 ** -16, 0.1, 0.25, 0.5, 0.999]


def tool_functions():
    """the definitions of tools/drop_hash_check.py, loaded by path without the report the file prints when it is run"""
    path = os.path.join(REPO, "tools", "drop_hash_check.py")
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom, ast.Assign, ast.FunctionDef))]
    ns = {}
    exec(compile(tree, path, "exec"), ns)
    return ns


def test_low_part_agrees_with_the_offline_tool():
    tool = tool_functions()["drop_hash4_lo"]
    rng = np.random.default_rng(20)
    q = rng.integers(0, 1 << 32, 10 ** 5, dtype=np.uint64)
    ks = rng.integers(0, 1 << 32, 10 ** 5, dtype=np.uint64)
    q[:4] = [0, 1, 0xFFFFFFFF, 0x00FFFFFF]
    ks[:4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    x, y = R.RULE.hash4_lo(ks, np.uint64(0), q)
    tx, ty = tool(q, ks)
    assert np.array_equal(x, tx) and np.array_equal(y, ty)
    assert int(x.max()) <= 0xFFFFFFFF and int(y.max()) <= 0xFFFFFFFF


def test_pieces_against_hand_evaluation():
    """mix32, the bit reversal, the seed key's use of the low word only and the high-word fold, on values small enough to follow"""
    assert int(R.mix32(0)) == 0
    x = 1 * 0x7feb352d & 0xFFFFFFFF
    x ^= x >> 15
    x = x * 0x846ca68b & 0xFFFFFFFF
    assert int(R.mix32(1)) == x ^ (x >> 16)
    v = np.array([1, 0x80000000, 0x12345678, 0xFFFFFFFF], dtype=np.uint64)
    assert [int(b) for b in R.bitrev32(v)] == [int("{:032b}".format(int(a))[::-1], 2) for a in v]
    assert int(R.seed_key(5)) == int(R.seed_key(2 ** 32 + 5)) == int(R.mix32((5 * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF))
    assert int(R.high_mix(5, np.uint64(123))) == 0
    assert int(R.high_mix(2 ** 32 + 5, np.uint64(123))) == (1 | 1 << 13 | 1 << 27)                 # hw = 1: bits 0, 13, 27 (1 >> 7 = 0)
    assert int(R.high_mix(5, np.uint64(2 ** 32 + 123))) == (1 | 1 << 13 | 1 << 27)                 # the index's high word folds the same way
    hw = 0xFFFFFFFF + 0xFFFFFFFF & 0xFFFFFFFF                                                       # the sum wraps in 32 bits
    assert int(R.high_mix(2 ** 64 - 1, np.uint64(2 ** 64 - 1))) == (hw ^ hw << 13 ^ hw >> 7 ^ hw << 27) & 0xFFFFFFFF
    xs, ys = np.array([0xAAAA5555], dtype=np.uint64), np.array([0x1234ABCD], dtype=np.uint64)
    assert [int(R.field(xs, ys, f)[0]) for f in range(4)] == [0xABCD, 0x1234, 0x5555, 0xAAAA]


def test_threshold():
    assert R.th16(2.0 ** -17) == 0 and bool(R.keep_range(3, 4099, 2.0 ** -17).all())
    assert R.th16(2.0 ** -16) == 1
    assert R.th16(0.1) == 6553
    assert R.th16(0.999) == 65470
    assert R.th16(0.0) == 0
    top = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert R.th16(top) == 65535
    ps = np.concatenate([np.random.default_rng(1).random(10 ** 4, dtype=np.float32), np.float32(1.0) - np.float32(2.0) ** -np.arange(1, 25)])
    ps = np.sort(ps[ps < 1])
    th = [R.th16(p) for p in ps]
    assert max(th) <= 65535 and th == sorted(th), "th16 is monotone in p, so the largest f32 below 1 bounds every p in [0, 1)"


@pytest.mark.parametrize("seed", SEEDS)
def test_keep_rate(seed):
    """over n = 2^20 the keep rate is within 6 standard deviations of q = 1 - th16 / 65536"""
    n = 2 ** 20
    f = R.RULE.fields(seed, np.arange(n, dtype=np.uint64))
    for p in RATES:
        q = 1.0 - R.th16(p) / 65536.0
        rate = float((f >= R.th16(p)).mean())
        assert abs(rate - q) <= 6.0 * math.sqrt(q * (1.0 - q) / n), (seed, p, rate, q)


@pytest.mark.parametrize("seed", [77, (5 << 32) | 7])
def test_prefix_gather_and_the_per_quad_form(seed):
    n, m, p = 4099, 1001, 0.25
    idx = np.arange(n, dtype=np.uint64)
    full = R.keep(seed, idx, p)
    assert np.array_equal(full[:m], R.keep(seed, np.arange(m, dtype=np.uint64), p))
    perm = np.random.default_rng(2).permutation(n)
    assert np.array_equal(R.keep(seed, idx[perm], p), full[perm])
    for k in (1, 3, 4, 5, 7, 8, 9, 1000, 4099):
        assert np.array_equal(R.keep_range(seed, k, p), full[:k]), k
    # indices past 2^34 (quad index past 2^32): the high word of the index folds where the seed's does
    far = np.uint64(2 ** 34) + idx
    assert np.array_equal(R.keep(seed, far, p), R.keep(seed + 2 ** 32, idx, p))
    assert not np.array_equal(R.keep(seed, far, p), full)


def test_apply_values():
    """kept = f32(x) * (1 / (1 - p)) rounded once to the type, dropped = +0 also for negative, infinite and NaN inputs"""
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.tensor([1.0, -2.0, float("inf"), -float("inf"), float("nan"), -0.0, 0.0, 3.0] * 8, dtype=dtype)
        y = R.apply(x, 77, 0.5)
        kp = torch.from_numpy(R.keep_range(77, x.numel(), 0.5))
        assert 0 < int(kp.sum()) < x.numel()
        iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
        assert bool((y[~kp].view(iv) == 0).all()), "a dropped element is +0, bit for bit"
        fin = kp & torch.isfinite(x)
        assert torch.equal(y[fin].double(), x[fin].double() * 2.0)
        assert bool(torch.isnan(y[kp & torch.isnan(x)]).all()) and bool(torch.isinf(y[kp & torch.isinf(x)]).all())
    third = R.apply(torch.full((64,), 3.0, dtype=torch.bfloat16), 77, 0.3)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))
    want = torch.tensor(float(np.float32(3.0) * inv)).to(torch.bfloat16)
    assert set(third.float().tolist()) == {0.0, float(want)}


def test_twins_differ_on_the_arrays_the_gpu_test_compares():
    n, p, seed = R.CONTROL["n"], R.CONTROL["p"], R.CONTROL["seed"]
    assert seed >= 2 ** 32
    rule = R.keep_range(seed, n, p)
    ties = int((R.RULE.fields(seed, np.arange(n, dtype=np.uint64)) == R.th16(p)).sum())
    print("MEASURED dropout rule: seed %#x, n = 2^20, p = 0.25: %d fields equal th16 = %d" % (seed, ties, R.th16(p)))
    assert ties >= 1, "no field equals th16 for this seed: pick another and record it in dropout_ref.CONTROL"
    assert len(R.TWINS) == 4
    for name, twin in R.TWINS.items():
        d = int((twin.keep_range(seed, n, p) != rule).sum())
        print("MEASURED dropout twin %s: differs from the rule on %d of %d elements" % (name, d, n))
        assert d >= 1, name
    assert int((R.TWINS["strict_greater"].keep_range(seed, n, p) != rule).sum()) == ties
    # below 2^32 the `ignore_seed_high` twin is the rule: only a seed with a high word can tell them apart
    assert np.array_equal(R.TWINS["ignore_seed_high"].keep_range(77, 4099, p), R.keep_range(77, 4099, p))


def test_high_word_is_a_weak_spot_not_an_identity():
    """a fact about the present hash, recorded and not bounded: the seed's high word enters through one xor after the mixing, so
    seeds 5 and 2^32 + 5 agree on more elements than independent masks would (0.625 at p = 0.25); seeds 5 and 6 do not"""
    n, p = 2 ** 20, 0.25
    a, hi, nb = R.keep_range(5, n, p), R.keep_range(2 ** 32 + 5, n, p), R.keep_range(6, n, p)
    print("MEASURED dropout high word: p = 0.25, n = 2^20: seeds 5 and 2^32 + 5 agree on %.4f of the elements, seeds 5 and 6 on %.4f "
          "(independent masks: 0.6250)" % (float((a == hi).mean()), float((a == nb).mean())))
    assert not np.array_equal(a, hi) and not np.array_equal(a, nb)
