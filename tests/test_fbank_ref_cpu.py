"""The filterbank reference of the tests (tests/fbank_ref.py, the rule of DESIGN.md 5f in numpy) against formulations it shares
nothing with: a direct O(N^2) DFT, an analytic tone, frame counts at the edges, exact floors, the package's host CMVN; then the
wrong twins, each of which must lie outside the GPU test's bound on the GPU test's own cases (a comparison they pass would not see
the mistake they stand for)."""
import math

import numpy as np
import pytest
import torch

import fbank_ref as R
from fbk_fairseq_st_amd import indexed

LOG_FLOOR = math.log(2.0 ** -23)


def test_fft_formulation_equals_a_direct_dft():
    for case in (R.CASES[0], R.CASES[2], R.CASES[3]):
        x = R.case_samples(case)[:R.geometry(case["cfg"].get("sr", 16000), 25.0, 10.0)[0] * 3]
        a, b = R.fbank(x, **case["cfg"]), R.fbank(x, dft=True, **case["cfg"])
        assert a.shape == b.shape and a.shape[0] >= 5 and np.abs(a - b).max() < 1e-9, case["name"]


@pytest.mark.parametrize("k", [3, 40, 200, 255])
def test_a_tone_at_an_exact_bin(k):
    """W = N = 512, no window, no pre-emphasis, no DC removal: a tone at bin k has power (A N / 2)^2 there and nothing elsewhere, so
    e[j] = bank[j][k] (A N / 2)^2"""
    sr, N, A, F = 16000, 512, 1000.0, 80
    x = A * np.cos(2 * np.pi * k * np.arange(N + 3 * 160) / N + 0.7)
    got = R.fbank(x, sr=sr, frame_length=32.0, num_mel_bins=F, preemphasis=0.0, remove_dc_offset=False, window_type="rectangular")
    bank = R.mel_bank(F, N, sr)
    want = np.log(np.maximum(bank[:, k] * (A * N / 2) ** 2, R.FLOOR))
    assert got.shape == (4, F)
    hit = bank[:, k] > 0
    assert hit.any() and np.abs(got[:, hit] - want[hit]).max() < 1e-9
    assert (got[:, ~hit] < math.log(1e-12 * (A * N / 2) ** 2)).all(), "leakage of an exact bin is rounding only"


def test_frame_counts_at_the_edges():
    W, S, N = R.geometry(16000, 25.0, 10.0)
    assert (W, S, N) == (400, 160, 512) and R.geometry(8000, 25.0, 10.0) == (200, 80, 256) and R.geometry(22050, 25.0, 10.0) == (551, 220, 1024)
    x = R.signal("noise3000", W + S, 1)
    for n, m in ((W - 1, 0), (W, 1), (W + S - 1, 1), (W + S, 2), (0, 0)):
        assert R.num_frames(n, W, S) == m and R.fbank(x[:n]).shape == (m, 80), n
    two = R.fbank(x)
    assert np.abs(two[0] - R.fbank(x[:W])[0]).max() < 1e-12 and np.abs(two[1] - R.fbank(x[S:])[0]).max() < 1e-12, "frame t is the samples [tS, tS + W)"


def test_silence_and_a_constant_give_exactly_the_floor():
    for dtype in (np.float64, np.float32):
        for x in (np.zeros(1000, np.int16), np.full(1000, 1234, np.int16), np.zeros(1000, np.float32)):
            out = R.fbank(x, dtype=dtype)
            assert out.shape == (4, 80) and out.dtype == dtype and (out == dtype(LOG_FLOOR)).all()
    assert np.float32(LOG_FLOOR) == np.log(np.float32(2.0 ** -23)) == np.float32(-15.942384719848633)
    assert not (R.fbank(np.full(1000, 1234, np.int16), remove_dc_offset=False) == LOG_FLOOR).any(), "without DC removal a constant is a signal"


def test_cmvn_equals_the_package_host_function():
    rng = np.random.default_rng(5)
    x = rng.normal(15.0, 3.0, (130, 80))
    assert np.abs(R.cmvn(x) - indexed.apply_mv_norm(torch.from_numpy(x)).numpy()).max() < 1e-12
    x[:, 7] = 12.5                                                  # a constant column: the +1e-8 form, for every column
    want = indexed.apply_mv_norm(torch.from_numpy(x)).numpy()
    got = R.cmvn(x)
    assert np.abs(got - want).max() < 1e-12 and (got[:, 7] == 0).all()
    plain = (x - x.mean(0)) / np.where(x.std(0, ddof=1) > 0, x.std(0, ddof=1), 1)
    assert 0 < np.abs(got[:, 8] - plain[:, 8]).max() < 1e-6, "the switch changes the other columns, slightly"
    f32 = R.cmvn(x.astype(np.float32), dtype=np.float32)
    assert f32.dtype == np.float32 and np.abs(f32 - got).max() < 1e-4


def test_float32_restatement_and_radix2_formulation_stay_near_float64():
    """the yardstick itself: the float32 host restatement is off by up to 1e-3 in the lowest bins and by about 1e-6 in the top
    ones; an independent float32 radix-2 formulation stays inside 8 times the yardstick on these cases but comes close to it"""
    worst = 0.0
    for case in R.CASES[:4]:
        x, r64, r32 = R.case_refs(case)
        yard = np.abs(r32 - r64).max(0)
        assert yard.max() < 2e-3 and np.median(yard[len(yard) // 2:]) < 3e-6, case["name"]
        err, bound = R.compare(R.fbank_radix2_f32(x, **case["cfg"]), r64, r32)
        worst = max(worst, float((err / bound).max()))
    assert 0.05 < worst < 1.0


@pytest.mark.parametrize("twin", sorted(R.FBANK_TWINS))
def test_fbank_twins_lie_outside_the_bound(twin):
    if twin == "floor_1e-10":                                       # shows where the floor is reached: the exact comparisons
        for x in (np.zeros(1000, np.int16), np.full(1000, 1234, np.int16)):
            assert (R.fbank(x, **R.FBANK_TWINS[twin]) != R.fbank(x)).all()
        return
    seen = 0
    for case in R.CASES:
        if not R.twin_applies(twin, case["cfg"]):
            continue
        x, r64, r32 = R.case_refs(case)
        err, bound = R.compare(R.fbank(x, **dict(case["cfg"], **R.FBANK_TWINS[twin])), r64, r32)
        assert (err > bound).any(), (twin, case["name"])
        seen += 1
    assert seen >= 1


def test_biased_variance_lies_outside_the_cmvn_bound():
    for case in (R.CASES[0], R.CASES[5]):
        x, r64, _ = R.case_refs(case)
        feats = r64.astype(np.float32)
        assert feats.std(0, ddof=1).min() >= 0.1
        ref = R.cmvn(feats)
        assert R.cmvn_within(R.cmvn(feats, dtype=np.float32), ref).all()
        assert not R.cmvn_within(R.cmvn_biased(feats), ref).all()
