"""The filterbank and normalisation rules of DESIGN.md 5f in plain numpy: `fbank` and `cmvn` run in float64 (the reference of the
tests) or, with dtype=np.float32, in float32 with scipy's float32 FFT -- the arithmetic a float32 host library performs, and the
yardstick of the GPU test's tolerance.  `fbank_radix2_f32` is an independent float32 formulation (half-size radix-2 Stockham FFT,
even / odd split, sequential mel sums): what a device kernel may reasonably do.  The wrong twins, the GPU test's cases and its
comparison live here too, so that the CPU tests can check that each twin lies outside the GPU test's bound on its own cases."""
import math

import numpy as np
import scipy.fft

FLOOR = 2.0 ** -23
WINDOWS = ("povey", "hanning", "hamming")


def geometry(sr, frame_length, frame_shift):
    W, S = int(sr * frame_length * 0.001), int(sr * frame_shift * 0.001)
    return W, S, 1 << (W - 1).bit_length()


def num_frames(n, W, S):
    return 0 if n < W else 1 + (n - W) // S


def window(kind, W, power=0.85):
    a = 2.0 * math.pi * np.arange(W) / (W - 1)
    if kind == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    if kind == "hanning":
        return 0.5 - 0.5 * np.cos(a)
    if kind == "povey":
        return (0.5 - 0.5 * np.cos(a)) ** power
    if kind == "rectangular":                                       # the analytic anchor only: the kernel does not offer it
        return np.ones(W)
    raise ValueError(kind)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_bank(F, N, sr, low_freq=20.0, high_freq=0.0):
    """[F, N/2] float64"""
    hi = high_freq if high_freq > 0 else sr / 2.0 + high_freq
    delta = (mel(hi) - mel(low_freq)) / (F + 1)
    bank = np.zeros((F, N // 2))
    for j in range(F):
        left = mel(low_freq) + j * delta
        center = left + delta
        right = center + delta
        for k in range(N // 2):
            m = mel(k * sr / N)
            bank[j, k] = max(0.0, min((m - left) / delta, (right - m) / delta))
    return bank


_BANKS = {}


def cached_bank(F, N, sr, low_freq, high_freq):
    key = (F, N, sr, low_freq, high_freq)
    if key not in _BANKS:
        _BANKS[key] = mel_bank(F, N, sr, low_freq, high_freq)
    return _BANKS[key]


def frames_of(x, W, S, dtype):
    """[m, W] in dtype: samples at their value"""
    m = num_frames(len(x), W, S)
    idx = np.arange(m)[:, None] * S + np.arange(W)[None, :]
    return np.asarray(x)[idx].astype(dtype) if m else np.zeros((0, W), dtype)


def fbank(x, sr=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97,
          remove_dc_offset=True, window_type="povey", dtype=np.float64, floor=FLOOR, emphasise_edge=True, povey_power=0.85, dft=False):
    """x: 1-D samples of one utterance (int16 or float) -> [m, num_mel_bins] in dtype.  The keyword arguments behind `dtype` exist
    for the wrong twins and for the O(N^2) cross-check (dft=True)."""
    W, S, N = geometry(sr, frame_length, frame_shift)
    fr = frames_of(x, W, S, dtype)
    if remove_dc_offset:
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=dtype)
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    y = fr - dtype(preemphasis) * prev
    if not emphasise_edge:
        y[:, 0] = fr[:, 0]
    y = y * window(window_type, W, povey_power).astype(dtype)
    pad = np.zeros((len(y), N), dtype)
    pad[:, :W] = y
    if dft:
        k, n = np.arange(N // 2)[:, None], np.arange(N)[None, :]
        spec = pad.astype(np.float64) @ np.exp(-2j * np.pi * k * n / N).T
    else:
        spec = scipy.fft.rfft(pad, axis=1)[:, :N // 2]
        assert spec.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    e = power @ cached_bank(num_mel_bins, N, sr, low_freq, high_freq).astype(dtype).T
    return np.log(np.maximum(e, dtype(floor))).astype(dtype)


def cmvn(x, dtype=np.float64, ddof=1):
    """data_utils.apply_mv_norm on [m, F]"""
    x = np.asarray(x).astype(dtype)
    mean, var = x.mean(axis=0, dtype=dtype), x.var(axis=0, ddof=ddof, dtype=dtype)
    eps = dtype(1e-8)
    inv = dtype(1) / (np.sqrt(var) + eps) if (var < eps).any() else dtype(1) / np.sqrt(var)
    return ((x - mean) * inv).astype(dtype)


# ------------------------------------------------------------------ an independent float32 formulation
def fbank_radix2_f32(x, sr=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=80, low_freq=20.0, high_freq=0.0, preemphasis=0.97,
                     remove_dc_offset=True, window_type="povey"):
    """float32 throughout: the real frame packed as N/2 complex points, a radix-2 Stockham FFT with table twiddles, the even / odd
    split, and sequential mel sums over each bin's own range"""
    f32 = np.float32
    W, S, N = geometry(sr, frame_length, frame_shift)
    M = N // 2
    fr = frames_of(x, W, S, f32)
    if remove_dc_offset:
        fr = fr - (fr.sum(axis=1, keepdims=True, dtype=f32) / f32(W))
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    y = (fr - f32(preemphasis) * prev) * window(window_type, W).astype(f32)
    pad = np.zeros((len(y), N), f32)
    pad[:, :W] = y
    a = 2.0 * math.pi * np.arange(M) / N
    tw = (np.cos(a) - 1j * np.sin(a)).astype(np.complex64)          # exp(-2 pi i k / N), rounded once
    z = (pad[:, 0::2] + 1j * pad[:, 1::2]).astype(np.complex64)
    i = np.arange(M // 2)
    s = 1
    while s < M:
        q = i & (s - 1)
        k = i - q
        o = 2 * k + q
        u, v = z[:, i], z[:, i + M // 2]
        nz = np.empty_like(z)
        nz[:, o] = u + v
        nz[:, o + s] = (u - v) * tw[2 * k]
        z, s = nz, 2 * s
    k = np.arange(M)
    zm = np.conj(z[:, (M - k) % M])
    even, odd = f32(0.5) * (z + zm), (-0.5j * (z - zm)).astype(np.complex64)
    spec = even + tw[k] * odd
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(f32)
    bank = cached_bank(num_mel_bins, N, sr, low_freq, high_freq).astype(f32)
    e = np.zeros((len(power), num_mel_bins), f32)
    for j in range(num_mel_bins):
        for kk in np.nonzero(bank[j] > 0)[0]:
            e[:, j] = e[:, j] + bank[j, kk] * power[:, kk]
    return np.log(np.maximum(e, f32(FLOOR))).astype(f32)


# ------------------------------------------------------------------ the wrong twins: each is `fbank` or `cmvn` with one thing off
FBANK_TWINS = {
    "hann_without_the_power": dict(povey_power=1.0),               # povey cases
    "no_dc_removal": dict(remove_dc_offset=False),                  # cases with DC removal
    "preemphasis_095": dict(preemphasis=0.95),                      # cases with pre-emphasis 0.97
    "first_sample_not_emphasised": dict(emphasise_edge=False),      # cases with pre-emphasis
    "mel_edges_from_0": dict(low_freq=0.0),
    "floor_1e-10": dict(floor=1e-10),                               # shows only where the floor is reached: silence
}


def twin_applies(name, cfg):
    if name == "hann_without_the_power":
        return cfg.get("window_type", "povey") == "povey"
    if name == "no_dc_removal":                                     # one bin over the whole band does not see a mean of a few units
        return cfg.get("remove_dc_offset", True) and cfg.get("num_mel_bins", 80) > 1
    if name == "preemphasis_095":
        return cfg.get("preemphasis", 0.97) == 0.97
    if name == "first_sample_not_emphasised":                       # povey and hanning start at zero and hide the first sample
        return cfg.get("preemphasis", 0.97) > 0 and cfg.get("window_type", "povey") == "hamming"
    return name == "mel_edges_from_0"


def cmvn_biased(x, dtype=np.float64):
    return cmvn(x, dtype, ddof=0)


# ------------------------------------------------------------------ the GPU test's comparison
FACTOR, YARD_FLOOR = 8.0, 2e-6
CMVN_TOL = 1e-4


def per_bin_bound(ref64, ref32):
    """per mel bin: 8 x max(the float32 host restatement's worst error over the frames, 2e-6)"""
    yard = np.abs(ref32.astype(np.float64) - ref64).max(axis=0)
    return FACTOR * np.maximum(yard, YARD_FLOOR)


def compare(got, ref64, ref32):
    """-> (worst error per bin, bound per bin); the test asserts err <= bound in every bin"""
    assert got.shape == ref64.shape == ref32.shape and got.shape[0] >= 100, "at least 100 frames keep the per-bin maximum stable"
    return np.abs(np.asarray(got, dtype=np.float64) - ref64).max(axis=0), per_bin_bound(ref64, ref32)


def cmvn_within(got, ref64):
    return np.abs(np.asarray(got, dtype=np.float64) - ref64) <= CMVN_TOL * np.maximum(1.0, np.abs(ref64))


# ------------------------------------------------------------------ the GPU test's cases
def ms_for(samples, sr):
    """a duration in ms whose int(sr * ms * 0.001) is exactly `samples`"""
    ms = (samples + 0.5) * 1000.0 / sr
    assert int(sr * ms * 0.001) == samples
    return ms


def signal(kind, n, seed, sr=16000):
    """int16 or float32 samples of one utterance"""
    rng = np.random.default_rng(seed)
    if kind == "noise30":
        return np.clip(np.rint(rng.normal(0, 30, n)), -32768, 32767).astype(np.int16)
    if kind == "noise3000":
        return np.clip(np.rint(rng.normal(0, 3000, n)), -32768, 32767).astype(np.int16)
    if kind == "tone":
        t = np.arange(n) / sr
        return np.clip(np.rint(8000 * np.sin(2 * np.pi * 440.0 * t + 0.3) + rng.normal(0, 100, n)), -32768, 32767).astype(np.int16)
    if kind == "dc":
        return np.clip(np.rint(20000 + rng.normal(0, 300, n)), -32768, 32767).astype(np.int16)
    if kind == "float":
        return rng.normal(0, 0.1, n).astype(np.float32)
    if kind == "impulse":
        x = np.clip(np.rint(rng.normal(0, 3, n)), -32768, 32767).astype(np.int16)
        x[n // 3] = 30000
        return x
    raise ValueError(kind)


def _case(name, kind, frames=120, **cfg):
    return dict(name=name, kind=kind, frames=frames, cfg=cfg)


_W = lambda samples, sr: dict(sr=sr, frame_length=ms_for(samples, sr))
CASES = [
    _case("16k_80_noise3000", "noise3000"),
    _case("16k_80_noise30", "noise30"),
    _case("8k_23_tone", "tone", sr=8000, num_mel_bins=23),
    _case("22k_128_noise3000", "noise3000", sr=22050, num_mel_bins=128),
    _case("22k_80_float", "float", sr=22050),
    _case("16k_64_dc", "dc", num_mel_bins=64),
    _case("16k_65_float", "float", num_mel_bins=65),
    _case("8k_80_float_hamming", "float", sr=8000, window_type="hamming"),
    _case("16k_1_impulse_hanning", "impulse", num_mel_bins=1, window_type="hanning"),
    _case("16k_80_tone_no_preemphasis", "tone", preemphasis=0.0),
    _case("16k_80_noise30_no_dc_removal", "noise30", remove_dc_offset=False),
    _case("w129_of_256", "noise3000", num_mel_bins=23, frame_shift=5.0, **_W(129, 8000)),
    _case("w256_of_256", "dc", num_mel_bins=64, **_W(256, 8000)),
    _case("w257_of_512", "float", num_mel_bins=65, **_W(257, 16000)),
    _case("w512_of_512", "tone", **_W(512, 16000)),
    _case("w513_of_1024", "noise30", num_mel_bins=128, **_W(513, 16000)),
    _case("w1024_of_1024", "noise3000", frame_shift=20.0, **_W(1024, 16000)),
    _case("shift_beyond_window", "impulse", sr=8000, frame_shift=30.0, num_mel_bins=23),
]


def case_samples(case):
    cfg = case["cfg"]
    W, S, _ = geometry(cfg.get("sr", 16000), cfg.get("frame_length", 25.0), cfg.get("frame_shift", 10.0))
    n = W + (case["frames"] - 1) * S + S // 2
    return signal(case["kind"], n, seed=sum(map(ord, case["name"])), sr=cfg.get("sr", 16000))


_REFS = {}


def case_refs(case):
    """(samples, float64 reference, float32 host restatement), computed once"""
    if case["name"] not in _REFS:
        x = case_samples(case)
        _REFS[case["name"]] = (x, fbank(x, **case["cfg"]), fbank(x, dtype=np.float32, **case["cfg"]))
    return _REFS[case["name"]]
