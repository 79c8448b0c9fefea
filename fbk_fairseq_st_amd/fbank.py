"""From waveforms to the model's input, on the device: Kaldi log-mel filterbanks (`torchaudio.compliance.kaldi.fbank` with its
defaults, which the reference's asr_dataset.py:66-85 calls) and the per-utterance mean / variance normalisation that follows it
there (`data_utils.apply_mv_norm`).

`FbankFrontEnd(...)` holds a configuration; `features` takes a padded batch of waveforms (int16 as `read_wav` yields them, or
float32) with their lengths and returns the padded feature batch, `net_input` returns it as the `net_input` of
`task.inference_step`, `normalize_features` is the normalisation alone for features that were computed elsewhere.  Nothing is read
back to the host: lengths and statuses stay device tensors.

The hot path is csrc/fbank.hip (kernels.fbank, kernels.cmvn; include/s2t_hip.h states both rules): one launch each.  The window
and the sparse mel bank are built here in float64 and rounded once, the twiddles stay float64; all are cached per configuration and
device.
Not offered: dither, the energy column, snip_edges=False, VTLN, htk_compat, linear output.  Resampling to one of these rates, and
speed perturbation, are resample.WaveResampler and resample.SpeedPerturb: their result is what `features` takes.
"""
import math
import wave

import numpy as np
import torch

from . import kernels as K

MAX_BINS = K.FBANK_MAX_BINS             # S2T_FBANK_MAX_BINS
FFT_SIZES = K.FBANK_FFT_SIZES
WINDOWS = ("povey", "hanning", "hamming")
STATUS = {0: "done", 1: "no features: no frame, or one frame with normalisation on", 2: "refused: a length outside the padded width"}


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def make_window(window_type, W):
    """the symmetric window of W points, float64"""
    if window_type not in WINDOWS:
        raise ValueError("FbankFrontEnd: window types %s, got %r" % (WINDOWS, window_type))
    a = 2.0 * math.pi * np.arange(W, dtype=np.float64) / (W - 1)
    if window_type == "hamming":
        return 0.54 - 0.46 * np.cos(a)
    hann = 0.5 - 0.5 * np.cos(a)
    return hann ** 0.85 if window_type == "povey" else hann


def make_twiddle(N):
    """cos(2 pi k / N) for k < N/2, then -sin(2 pi k / N) for k < N/2, float64"""
    a = 2.0 * math.pi * np.arange(N // 2, dtype=np.float64) / N
    return np.concatenate([np.cos(a), -np.sin(a)])


def make_mel_bank(num_mel_bins, N, sample_rate, low_freq, high_freq):
    """the dense bank [num_mel_bins, N/2] over the FFT bins 0 .. N/2 - 1, float64 (the Nyquist bin has weight 0)"""
    hi = high_freq if high_freq > 0 else sample_rate / 2.0 + high_freq
    if not 0.0 <= low_freq < hi <= sample_rate / 2.0:
        raise ValueError("FbankFrontEnd: 0 <= low_freq < high_freq <= sample_rate / 2, got %r and %r at %r Hz" % (low_freq, hi, sample_rate))
    lo_m, hi_m = float(mel(low_freq)), float(mel(hi))
    delta = (hi_m - lo_m) / (num_mel_bins + 1)
    left = lo_m + np.arange(num_mel_bins, dtype=np.float64)[:, None] * delta
    center, right = left + delta, left + 2.0 * delta
    m = mel(np.arange(N // 2, dtype=np.float64) * sample_rate / N)[None, :]
    return np.maximum(0.0, np.minimum((m - left) / delta, (right - m) / delta))


def sparse_bank(dense):
    """dense [F, K] -> (bank int32 [F, 3] = first bin, count, offset into the weights; weights float32): each row's own contiguous
    range of non-zero weights, rounded to float32 once"""
    rows, weights, off = [], [], 0
    for r in dense:
        nz = np.nonzero(r > 0)[0]
        first, cnt = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if len(nz) else (0, 0)
        rows.append((first, cnt, off))
        weights.append(r[first:first + cnt])
        off += cnt
    return np.array(rows, dtype=np.int32).reshape(-1, 3), np.concatenate(weights).astype(np.float32)


def read_wav(path):
    """a 16-bit PCM wav file -> (int16 tensor of channel 0, sample rate).  Anything else is a ValueError."""
    try:
        with wave.open(path, "rb") as f:
            width, chans, rate, n = f.getsampwidth(), f.getnchannels(), f.getframerate(), f.getnframes()
            if width != 2 or f.getcomptype() != "NONE":
                raise ValueError("read_wav: %s holds %d-bit samples (%s); only 16-bit PCM is read" % (path, 8 * width, f.getcomptype()))
            raw = f.readframes(n)
    except (wave.Error, EOFError) as e:
        raise ValueError("read_wav: %s is not a PCM wav file (%s)" % (path, e))
    data = np.frombuffer(raw, dtype="<i2").reshape(-1, chans)[:, 0]
    return torch.from_numpy(data.astype(np.int16)), rate


class FbankFrontEnd:
    """torchaudio's kaldi.fbank defaults: dither 0, snip-edges, no energy column, log output.  Frame and shift in milliseconds."""

    def __init__(self, num_mel_bins=80, frame_length=25.0, frame_shift=10.0, sample_rate=16000, normalize=True, window_type="povey",
                 preemphasis=0.97, remove_dc_offset=True, low_freq=20.0, high_freq=0.0):
        self.num_mel_bins, self.sample_rate = int(num_mel_bins), sample_rate
        self.frame_length, self.frame_shift = float(frame_length), float(frame_shift)
        self.normalize, self.window_type = bool(normalize), window_type
        self.preemphasis, self.remove_dc_offset = float(preemphasis), bool(remove_dc_offset)
        self.low_freq, self.high_freq = float(low_freq), float(high_freq)
        self.W = int(sample_rate * self.frame_length * 0.001)
        self.S = int(sample_rate * self.frame_shift * 0.001)
        if self.W < 2 or self.S < 1:
            raise ValueError("FbankFrontEnd: a window of at least 2 samples and a shift of at least 1, got %d and %d" % (self.W, self.S))
        self.N = 1 << (self.W - 1).bit_length()
        if self.N not in FFT_SIZES:
            raise ValueError("FbankFrontEnd: windows of %d to %d samples (FFT sizes %s), got %d samples: %r ms at %r Hz"
                             % (FFT_SIZES[0] // 2 + 1, FFT_SIZES[-1], FFT_SIZES, self.W, frame_length, sample_rate))
        if not 1 <= self.num_mel_bins <= MAX_BINS:
            raise ValueError("FbankFrontEnd: 1 to %d mel bins (S2T_FBANK_MAX_BINS), got %d" % (MAX_BINS, self.num_mel_bins))
        if not 0.0 <= self.preemphasis <= 1.0:
            raise ValueError("FbankFrontEnd: preemphasis in [0, 1], got %r" % (preemphasis,))
        self._host = self._make_tables()
        self._tables = {}

    def _make_tables(self):
        bank, weights = sparse_bank(make_mel_bank(self.num_mel_bins, self.N, self.sample_rate, self.low_freq, self.high_freq))
        return (torch.from_numpy(make_window(self.window_type, self.W).astype(np.float32)),
                torch.from_numpy(make_twiddle(self.N)), torch.from_numpy(bank), torch.from_numpy(weights))

    def tables(self, device):
        """(window [W], twiddle [N], bank [F, 3], weights [n]) on `device`, made once"""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = tuple(t.to(device) for t in self._host)
        return self._tables[key]

    def num_frames(self, n):
        """frames of an utterance of n samples (snip-edges)"""
        return 0 if n < self.W else 1 + (n - self.W) // self.S

    @torch.no_grad()
    def features(self, waves, wave_len):
        """waves [B, Nmax] int16 or float32 (device; other floating dtypes are converted to float32), wave_len [B] the samples of
        each row.  Returns dict(features f32 [B, Tmax, num_mel_bins] with zeros behind a sentence's frames, lengths int64 [B],
        status int32 [B]: see STATUS; a sentence that is not done has length 0)."""
        if waves.dim() != 2:
            raise ValueError("FbankFrontEnd: waves must be [B, Nmax], got %s" % (tuple(waves.shape),))
        if waves.dtype not in (torch.int16, torch.float32):
            if waves.dtype in (torch.float64, torch.float16, torch.bfloat16):
                waves = waves.float()
            else:
                raise ValueError("FbankFrontEnd: waves must be int16 or floating point, got %s" % waves.dtype)
        dev = waves.device
        wave_len = torch.as_tensor(wave_len).to(device=dev, dtype=torch.int64)
        window, twiddle, bank, weights = self.tables(dev)
        x, out_len, status = K.fbank(waves, wave_len, window, twiddle, bank, weights, self.S, self.N, self.preemphasis, self.remove_dc_offset)
        if self.normalize:
            out_len, st2 = K.cmvn(x, out_len)
            status = torch.where(status != 0, status, st2)
        return {"features": x, "lengths": out_len.long(), "status": status}

    def net_input(self, waves, wave_len):
        """the `net_input` of task.inference_step: {"src_tokens": features, "src_lengths": lengths}"""
        out = self.features(waves, wave_len)
        return {"src_tokens": out["features"], "src_lengths": out["lengths"]}

    @torch.no_grad()
    def normalize_features(self, x, lengths):
        """the normalisation alone, on a copy of x [B, Tmax, F] (any float dtype; F up to S2T_FBANK_MAX_BINS) with lengths [B].
        Returns what `features` returns."""
        x = x.float().clone(memory_format=torch.contiguous_format)
        lengths = torch.as_tensor(lengths).to(x.device)
        if lengths.dtype not in (torch.int32, torch.int64):
            lengths = lengths.long()
        out_len, status = K.cmvn(x, lengths)
        return {"features": x, "lengths": out_len.long(), "status": status}
