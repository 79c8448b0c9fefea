"""The float64 restatement of the resampling rule (tests/resample_ref.py) against the numbers the rule was specified with: tap and
phase counts, lengths, scale invariance, a tone; its structure (symmetry, DC gain); and every wrong twin differs from the rule under
the file's own comparison.  The package's own bank builder (resample.make_bank) must build the same banks."""
import math

import numpy as np
import pytest

import resample_ref as R


@pytest.mark.parametrize("pair", R.PAIRS, ids=["%d-%d" % p for p in R.PAIRS])
def test_quoted_tap_and_phase_counts(pair):
    in_unit, out_unit, first, count, w = R.bank(*pair)
    assert (in_unit, out_unit) == R.reduce_pair(*pair)
    assert (out_unit, int(count.min()), int(count.max()), out_unit * w.shape[1]) == R.QUOTED[pair]
    for i in range(out_unit):
        assert (w[i, count[i]:] == 0).all()


def test_the_pair_that_must_be_refused_has_207987_weights():
    # counted without building the bank: phases x the widest tap count
    orig, new = 16000, 15999
    cutoff = 0.99 * 0.5 * new
    ww = 6 / (2.0 * cutoff)
    widest = max(math.floor((i / new + ww) * orig) - math.ceil((i / new - ww) * orig) + 1 for i in range(new))
    assert new * widest == 207987


def test_quoted_lengths_and_scale_invariance():
    assert [R.num_samples(n, 48000, 16000) for n in (4800, 4801, 1, 0)] == [1600, 1601, 1, 0]
    a, b = R.bank(11, 10), R.bank(176000, 160000)
    assert a[:2] == b[:2] == (11, 10) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.abs(a[4] - b[4]).max() <= 1e-15
    a, b = R.bank(48000, 16000), R.bank(3, 1)
    assert np.array_equal(a[2], b[2]) and np.abs(a[4] - b[4]).max() <= 1e-15


@pytest.mark.parametrize("pair", R.PAIRS, ids=["%d-%d" % p for p in R.PAIRS])
def test_num_samples_against_a_brute_force_count(pair):
    orig, new = R.reduce_pair(*pair)
    for n in range(3 * orig + 6):
        assert R.num_samples(n, *pair) == R.brute_samples(n, orig, new), n


def test_a_tone_is_a_tone():
    n = 4800
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 48000.0).astype(np.float32)
    y, _ = R.resample(x, n, 48000, 16000)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000.0)
    err = np.abs(y - want)[20:-20].max()
    assert len(y) == 1600 and err <= 1e-3 and err <= 4.0e-4, err


@pytest.mark.parametrize("pair", R.PAIRS, ids=["%d-%d" % p for p in R.PAIRS])
def test_phase_0_is_symmetric_and_every_phase_has_unit_dc_gain(pair):
    _, _, first, count, w = R.bank(*pair)
    c = int(count[0])
    assert first[0] == -(c - 1) // 2 and c % 2 == 1
    assert np.abs(w[0, :c] - w[0, :c][::-1]).max() <= 1e-15
    assert np.abs(w.sum(1) - 1.0).max() <= 1e-3


def noise(n, dtype, seed=5):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.int16, np.float32], ids=["int16", "float32"])
@pytest.mark.parametrize("pair", [(3, 1), (1, 2), (441, 160), (11, 10)], ids=lambda p: "%d-%d" % p)
def test_the_float32_restatement_is_within_the_bound(pair, dtype):
    n = 3 * R.reduce_pair(*pair)[0] + 200
    x = noise(n + 50, dtype)                        # 50 samples of junk behind n
    y32, _ = R.resample(x, n, *pair, dtype=np.float32)
    y64, S = R.resample(x, n, *pair)
    worst = float(R.units(y32, y64, S).max())
    assert worst <= 8.0 and R.within(y32, x, n, *pair), worst          # the bound allows 17 to 41


@pytest.mark.parametrize("twin", sorted(R.TWINS))
def test_every_twin_differs_from_the_rule(twin):
    kw = R.TWINS[twin]
    for pair in ((3, 1), (441, 160), (9, 10)):
        if twin == "outermost_tap_dropped":         # an edge tap is 1e-6 of the sum: only the exact comparison on impulses sees it
            rows, n = R.impulse_rows(*pair, np.int16)
            assert any(not np.array_equal(R.impulse_expected(r, n, *pair, **kw), R.impulse_expected(r, n, *pair)) for r in rows)
            continue
        orig = R.reduce_pair(*pair)[0]
        n = 4 * orig if twin == "length_floor_plus_1" else 4 * orig + 100      # the wrong length shows at exact multiples only
        x = noise(n + 60, np.int16)
        wrong, _ = R.resample(x, n, *pair, **kw)
        assert not R.within(wrong, x, n, *pair), (twin, pair)
        right, _ = R.resample(x, n, *pair, dtype=np.float32)
        assert R.within(right, x, n, *pair)
    if twin == "length_floor_plus_1":
        assert R.num_samples(4801, 48000, 16000, **kw) == R.num_samples(4801, 48000, 16000)


def test_impulse_rows_meet_every_tap_once():
    for pair in ((3, 1), (1, 2), (441, 160)):
        in_unit, out_unit, first, count, w = R.bank(*pair)
        rows, n = R.impulse_rows(*pair, np.int16)
        hit = np.zeros(w.shape, bool)
        m = R.num_samples(n, *pair)
        for row in rows:
            xs, phase = R._gather(row, n, first, in_unit, out_unit, w.shape[1], m, False)
            assert ((xs != 0).sum(1) <= 1).all()
            k, j = np.nonzero(xs)
            hit[phase[k], j] = True
        assert hit[w != 0].all()


def test_the_package_builds_the_same_banks():
    from fbk_fairseq_st_amd import resample as RS
    for pair in R.PAIRS + [(3, 1), (2, 1), (1, 2), (441, 320), (160, 147)]:
        in_unit, out_unit, first, count, w = R.bank(*pair)
        bk = RS.make_bank(*pair)
        assert (bk["in_unit"], bk["out_unit"], bk["taps"]) == (in_unit, out_unit, w.shape[1])
        assert np.array_equal(bk["first"], first) and np.abs(bk["weights"] - w).max() <= 1e-15
        assert np.array_equal(bk["weights"] == 0, w == 0)
        for n in (0, 1, in_unit - 1, in_unit, in_unit + 1, 12345):
            assert RS.num_samples(n, *pair) == R.num_samples(n, *pair)
