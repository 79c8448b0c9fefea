#!/usr/bin/env python3
"""Time the resampler (csrc/resample.hip: K.resample through resample.WaveResampler and resample.SpeedPerturb) beside a
torch-on-device formulation of the same rule, on the same inputs, in the same process:

    python tools/resample_time.py [--rounds 7] [--calls 10] > profiles/resample.txt

Shapes, int16, every utterance at its full length: 16 utterances of 10 s at 48 kHz -> 16 kHz, 64 of 15 s at 44.1 kHz -> 16 kHz, 64 of
15 s at 16 kHz under SpeedPerturb with the factors 9/10, 1, 11/10 drawn per utterance, 1 of 60 s at 48 kHz -> 16 kHz.  The waveforms
are noise of amplitude 3,000 over a 200 Hz tone.
Device figures are device events around `calls` back-to-back calls as Python makes them, per call: the class's method (which
allocates its result) and the torch formulation -- the batch padded once, then one strided conv1d per phase written into its column
of the result, as torchaudio's resample_waveform does it; under SpeedPerturb once per factor on that factor's rows, the rows picked
by a host-known index.  Rounds alternate between the routes; every round is printed, then the median.  The first utterance of every
route is held to the bound of tests/test_resample_gpu.py against float64.  The floor: the bytes a call must move (samples read once,
result written once) over the rate of a device-to-device copy measured here.  Needs an MI355X; there is no pass / fail threshold on
the times."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_ref as R  # noqa: E402
from fbk_fairseq_st_amd import resample as RS  # noqa: E402

SHAPES = [("16 x 10 s, 48 k -> 16 k", 16, 10, 48000, (48000, 16000)), ("64 x 15 s, 44.1 k -> 16 k", 64, 15, 44100, (44100, 16000)),
          ("64 x 15 s at 16 k, SpeedPerturb 9/10, 1, 11/10", 64, 15, 16000, None), ("1 x 60 s, 48 k -> 16 k", 1, 60, 48000, (48000, 16000))]


def make_waves(B, seconds, sr):
    rng = np.random.default_rng(23)
    n = seconds * sr
    t = np.arange(n) / sr
    return np.clip(np.rint(rng.normal(0, 3000, (B, n)) + 2000 * np.sin(2 * np.pi * 200.0 * t)), -32768, 32767).astype(np.int16)


def torch_route(bank, Nmax):
    """waves [B, Nmax] -> f32 [B, ceil(Nmax out_unit / in_unit)]: one strided conv1d per phase"""
    iu, ou, taps, first = bank["in_unit"], bank["out_unit"], bank["taps"], bank["first"]
    if iu == ou:
        return lambda waves: waves.float()
    m = -((-Nmax * ou) // iu)
    units = -(-m // ou)
    w = torch.from_numpy(bank["weights"].astype(np.float32)).cuda()
    left = max(0, -int(first.min()))
    right = max(0, left + int(first.max()) + (units - 1) * iu + taps - (left + Nmax))
    length = (units - 1) * iu + taps

    def run(waves):
        x = F.pad(waves.float(), (left, right))[:, None, :]
        out = torch.empty((waves.shape[0], units, ou), dtype=torch.float32, device=waves.device)
        for i in range(ou):
            s = left + int(first[i])
            out[:, :, i] = F.conv1d(x[:, :, s:s + length], w[i][None, None, :], stride=iu)[:, 0, :]
        return out.reshape(waves.shape[0], -1)[:, :m]
    return run


def device_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def copy_rate():
    src = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    us = statistics.median(device_time(lambda: dst.copy_(src), 10) for _ in range(5))
    return 2 * src.numel() / us / 1e3          # GB/s, read + write


def within(y, x, n, pair):
    y64, S = R.resample(x, n, *pair)
    if len(y) != len(y64):
        return "False (length %d for %d)" % (len(y), len(y64))
    u = R.units(y, y64, S).max()
    return "%s (worst %.2f of %.0f units)" % (bool(u <= R.allowed(*pair)), u, R.allowed(*pair))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resample_time.py measures on the GPU"
    print("device:", torch.cuda.get_device_name(0))
    rate = copy_rate()
    print("device-to-device copy of 256 MiB: %.0f GB/s (read + write)" % rate)
    print("int16 in, float32 out; rounds %d x %d calls, alternating; us per call" % (a.rounds, a.calls))
    for tag, B, seconds, sr, pair in SHAPES:
        host = make_waves(B, seconds, sr)
        waves = torch.from_numpy(host).cuda()
        n = host.shape[1]
        lens = torch.full((B,), n, dtype=torch.int64, device="cuda")
        if pair is not None:
            rs = RS.WaveResampler(*pair)
            kernel = lambda: rs.resample(waves, lens)
            conv = torch_route(rs.bank, n)
            via_torch = lambda: conv(waves)
            first_pair, moved = pair, host.nbytes + B * rs.num_samples(n) * 4
            y_t = via_torch()[0]
        else:
            sp = RS.SpeedPerturb()
            choice = sp.draw(B, 0)
            dev_choice = choice.cuda()
            kernel = lambda: sp.apply(waves, lens, 0, choice=dev_choice)
            groups = [(torch.nonzero(choice == c).flatten().cuda(), torch_route(sp.banks[c], n)) for c in range(len(sp.factors))]
            via_torch = lambda: [conv(waves[idx]) for idx, conv in groups if idx.numel()]
            first_pair = sp.pairs[int(choice[0])]
            moved = host.nbytes + B * sp.num_samples(n) * 4       # the padded result is written whole
            y_t = [conv(waves[idx]) for idx, conv in groups if (idx == 0).any()][0][0]
            print("  factors drawn: %s" % " ".join("%s x %d" % (f, int((choice == c).sum())) for c, f in enumerate(sp.factors)))
        out = kernel()
        m = int(out["lengths"][0])
        print("%s: %d -> %d samples each; first utterance within the bound: kernel %s, torch formulation %s"
              % (tag, n, m, within(out["waves"][0, :m].cpu().numpy(), host[0], n, first_pair), within(y_t[:m].cpu().numpy(), host[0], n, first_pair)))
        routes = [("device  kernel (one launch)", kernel), ("device  torch formulation, a conv1d per phase", via_torch)]
        for _, fn in routes:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in routes]
        for _ in range(a.rounds):
            for i, (_, fn) in enumerate(routes):
                times[i].append(device_time(fn, a.calls))
        med = [statistics.median(ts) for ts in times]
        for (name, _), ts, v in zip(routes, times, med):
            print("  %-48s %s -> median %.1f us" % (name, " ".join("%.1f" % t for t in ts), v))
        floor = moved / rate / 1e3
        print("  %.1f MB moved at least: floor %.1f us at the copy rate; kernel = %.2f x the floor (%.0f GB/s); torch formulation / kernel = %.2f x"
              % (moved / 1e6, floor, med[0] / floor, moved / med[0] / 1e3, med[1] / med[0]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
