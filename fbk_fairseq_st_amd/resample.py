"""Sample-rate conversion and speed perturbation of waveforms, on the device: Kaldi's `LinearResample`, a windowed-sinc polyphase
filter, as `torchaudio.compliance.kaldi.resample_waveform` restates it -- the companion of the `kaldi.fbank` that fbank.py restates.

`WaveResampler(orig_freq, new_freq)` holds one resampling; `resample` takes a padded batch of waveforms (int16 as `fbank.read_wav`
yields them, or float32) with their lengths and returns the padded resampled batch.  `SpeedPerturb(factors)` draws one factor per
utterance on the host, reproducibly per (seed, update), and resamples every row by its own factor in the same single launch.  Nothing
is read back to the host: lengths and statuses stay device tensors, and the result chains into
`FbankFrontEnd.features(out["waves"], out["lengths"])`.

The hot path is csrc/resample.hip (kernels.resample; include/s2t_hip.h states the rule): one launch.  The filter banks are built
here in float64 and rounded to float32 once; they are cached per device.
Compatibility rests on the restated rule (tests/resample_ref.py), not on a captured torchaudio result: torchaudio is not a dependency.
Not offered: other windows than Kaldi's Hann-windowed sinc, streaming (state across calls), resampling by a ratio whose reduced form
is outside the limits below (16000 -> 15999 has 207,987 weights).
"""
import math
from fractions import Fraction

import numpy as np
import torch

from . import kernels as K

MAX_BANKS = K.RESAMPLE_MAX_BANKS        # S2T_RESAMPLE_MAX_BANKS
MAX_PHASES = K.RESAMPLE_MAX_PHASES      # S2T_RESAMPLE_MAX_PHASES
MAX_BANK = K.RESAMPLE_MAX_BANK          # S2T_RESAMPLE_MAX_BANK
MAX_SPAN = K.RESAMPLE_MAX_SPAN          # S2T_RESAMPLE_MAX_SPAN
STATUS = {0: "done", 1: "no samples", 2: "refused: a length outside the padded width, a choice outside the factors, or a result wider than the batch's"}


def _rate(v, what):
    if isinstance(v, bool) or not (isinstance(v, (int, np.integer)) or (isinstance(v, float) and v.is_integer())):
        raise ValueError("resample: %s must be a positive integer, got %r" % (what, v))
    if int(v) < 1:
        raise ValueError("resample: %s must be a positive integer, got %r" % (what, v))
    return int(v)


def reduce_pair(orig, new):
    orig, new = _rate(orig, "orig_freq"), _rate(new, "new_freq")
    g = math.gcd(orig, new)
    return orig // g, new // g


def num_samples(n, orig, new):
    """samples of an utterance of n samples after resampling: ceil(n * new / orig), Kaldi's tick count"""
    orig, new = reduce_pair(orig, new)
    return -((-int(n) * new) // orig)


def make_bank(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """the filter bank of a resampling, float64: dict(in_unit, out_unit, taps, first int64 [out_unit], weights float64
    [out_unit, taps], zero behind a phase's own taps).  orig == new: a copy, no taps."""
    orig, new = reduce_pair(orig, new)
    width = _rate(lowpass_filter_width, "lowpass_filter_width")
    rolloff = float(rolloff)
    if not 0.0 < rolloff <= 1.0:
        raise ValueError("resample: rolloff in (0, 1], got %r" % (rolloff,))
    if orig == new:
        return dict(in_unit=1, out_unit=1, taps=0, first=np.zeros(1, np.int64), weights=np.zeros((1, 0)))
    cutoff = rolloff * 0.5 * min(orig, new)
    ww = width / (2.0 * cutoff)
    # the limits, before a bank of 200,000 weights is built: a phase has at most 2 ww orig + 1 taps
    if new > MAX_PHASES:
        raise ValueError("resample: %d -> %d has %d phases, at most %d (S2T_RESAMPLE_MAX_PHASES)" % (orig, new, new, MAX_PHASES))
    t = np.arange(new, dtype=np.float64) / new
    first = np.ceil((t - ww) * orig).astype(np.int64)
    last = np.floor((t + ww) * orig).astype(np.int64)
    taps = int((last - first).max()) + 1
    if taps * new > MAX_BANK:
        raise ValueError("resample: %d -> %d has %d weights (%d phases of %d taps), at most %d (S2T_RESAMPLE_MAX_BANK)"
                         % (orig, new, taps * new, new, taps, MAX_BANK))
    j = np.arange(taps, dtype=np.int64)[None, :]
    d = (first[:, None] + j) / float(orig) - t[:, None]
    safe = np.where(d == 0.0, 1.0, d)
    sinc = np.where(d == 0.0, 2.0 * cutoff, np.sin(2.0 * math.pi * cutoff * d) / (math.pi * safe))
    w = 0.5 * (1.0 + np.cos(2.0 * math.pi * cutoff / width * d)) * sinc / orig
    w = np.where((np.abs(d) < ww) & (first[:, None] + j <= last[:, None]), w, 0.0)
    return dict(in_unit=orig, out_unit=new, taps=taps, first=first, weights=w)


def pack_table(banks):
    """banks (make_bank's dicts) -> (banks int32 [R, 7] for the host, first int32 [n], weights float32 [n]): what kernels.resample
    takes.  Weights go tap-major, w[i][j] at w_off + j * out_unit + i, rounded to float32 here, once."""
    rows, firsts, weights, f_off, w_off = [], [np.zeros(0, np.int32)], [np.zeros(0, np.float32)], 0, 0
    for bk in banks:
        if bk["in_unit"] == bk["out_unit"]:
            rows.append((1, 1, 0, 0, 0, 0, 0))
            continue
        first, taps, ou = bk["first"], bk["taps"], bk["out_unit"]
        lo = int(first.min())
        rows.append((bk["in_unit"], ou, taps, f_off, w_off, lo, int(first.max()) - lo + taps))
        firsts.append(first.astype(np.int32))
        weights.append(np.ascontiguousarray(bk["weights"].T).astype(np.float32).reshape(-1))
        f_off += ou
        w_off += taps * ou
    table = (torch.tensor(rows, dtype=torch.int32).reshape(-1, K.RESAMPLE_BANK_INTS), torch.from_numpy(np.concatenate(firsts)),
             torch.from_numpy(np.concatenate(weights)))
    K.resample_check_banks(table[0], table[1].shape[0], table[2].shape[0])
    return table


def _waves(waves, who):
    if waves.dim() != 2:
        raise ValueError("%s: waves must be [B, Nmax], got %s" % (who, tuple(waves.shape)))
    if waves.dtype not in (torch.int16, torch.float32):
        if waves.dtype in (torch.float64, torch.float16, torch.bfloat16):
            return waves.float()
        raise ValueError("%s: waves must be int16 or floating point, got %s" % (who, waves.dtype))
    return waves


def _lengths(wave_len, dev):
    wave_len = torch.as_tensor(wave_len).to(dev)
    return wave_len if wave_len.dtype in (torch.int32, torch.int64) else wave_len.long()


class _Tables:
    """a packed table, host side, and its device arrays, made once per device"""

    def __init__(self, banks):
        self._host = pack_table(banks)
        self._tables = {}

    def tables(self, device):
        """(banks int32 [R, 7] on the host, first int32 [n] and weights float32 [n] on `device`)"""
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = (self._host[0], self._host[1].to(device), self._host[2].to(device))
        return self._tables[key]


class WaveResampler(_Tables):
    """torchaudio's resample_waveform: lowpass_filter_width 6, rolloff 0.99."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
        self.orig_freq, self.new_freq = _rate(orig_freq, "orig_freq"), _rate(new_freq, "new_freq")
        self.bank = make_bank(self.orig_freq, self.new_freq, lowpass_filter_width, rolloff)
        super().__init__([self.bank])

    def num_samples(self, n):
        return num_samples(n, self.orig_freq, self.new_freq)

    @torch.no_grad()
    def resample(self, waves, wave_len):
        """waves [B, Nmax] int16 or float32 (device; other floating dtypes are converted to float32), wave_len [B] the samples of
        each row.  Returns dict(waves f32 [B, num_samples(Nmax)] with zeros behind a row's samples, lengths int64 [B], status int32
        [B]: see STATUS; a row that is not done has length 0)."""
        waves = _waves(waves, "WaveResampler")
        out, out_len, status = K.resample(waves, _lengths(wave_len, waves.device), *self.tables(waves.device), self.num_samples(waves.shape[1]))
        return {"waves": out, "lengths": out_len, "status": status}


def parse_factor(f):
    """a speed factor -> Fraction p/q: the waveform plays p/q times faster, the resampling (p, q)"""
    try:
        if isinstance(f, bool) or (isinstance(f, float) and not math.isfinite(f)):
            raise ValueError
        fr = Fraction(f) if not isinstance(f, float) else Fraction(repr(f))
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("SpeedPerturb: a factor is a positive fraction such as '9/10', 1 or 1.1, got %r" % (f,))
    if fr <= 0:
        raise ValueError("SpeedPerturb: a factor is a positive fraction such as '9/10', 1 or 1.1, got %r" % (f,))
    return fr


class SpeedPerturb(_Tables):
    """Speed perturbation: every utterance is resampled by one of `factors` and keeps its sample rate's label."""

    def __init__(self, factors=("9/10", 1, "11/10"), seed=1):
        self.factors = tuple(parse_factor(f) for f in factors)
        if not 1 <= len(self.factors) <= MAX_BANKS:
            raise ValueError("SpeedPerturb: 1 to %d factors (S2T_RESAMPLE_MAX_BANKS), got %d" % (MAX_BANKS, len(self.factors)))
        self.seed = int(seed)
        self.pairs = tuple((f.numerator, f.denominator) for f in self.factors)
        self.banks = [make_bank(p, q) for p, q in self.pairs]
        super().__init__(self.banks)

    def num_samples(self, n, choice=None):
        """samples of an utterance of n samples under factor `choice`; None: under the slowest factor, the widest result"""
        pairs = self.pairs if choice is None else (self.pairs[choice],)
        return max(num_samples(n, p, q) for p, q in pairs)

    def draw(self, B, update):
        """one factor index per utterance, int32 [B] on the host: the same for the same (seed, update)"""
        rng = np.random.default_rng([self.seed, int(update)])
        return torch.from_numpy(rng.integers(0, len(self.factors), size=int(B)).astype(np.int32))

    @torch.no_grad()
    def apply(self, waves, wave_len, update, choice=None):
        """waves and wave_len as WaveResampler.resample takes them; `update` numbers the draw; `choice` [B] gives the factor index of
        each row instead of drawing it.  Returns dict(waves f32 [B, num_samples(Nmax)], lengths, status, choice int32 [B] on the
        device)."""
        waves = _waves(waves, "SpeedPerturb")
        dev = waves.device
        if choice is None:
            choice = self.draw(waves.shape[0], update)
        choice = torch.as_tensor(choice).to(device=dev, dtype=torch.int32)       # a host-to-device copy: nothing is read back
        out, out_len, status = K.resample(waves, _lengths(wave_len, dev), *self.tables(dev), self.num_samples(waves.shape[1]), ratio_id=choice)
        return {"waves": out, "lengths": out_len, "status": status, "choice": choice}
