#!/usr/bin/env python3
"""Time the filterbank front end (csrc/fbank.hip: K.fbank, K.cmvn, fbank.FbankFrontEnd) beside a torch-on-device formulation of the
same rule and the float32 host restatement, on the same inputs, in the same process:

    python tools/fbank_time.py [--rounds 7] [--calls 10] > profiles/fbank.txt

Shapes, int16 at 16 kHz, 80 bins, 25 / 10 ms: 16 utterances of 10 s (1,000 frames each less two: the generation shape), 64 of 15 s,
1 of 60 s; every utterance has its full length.  The waveforms are noise of amplitude 3,000 over a 200 Hz tone.
Device figures are device events around `calls` back-to-back calls, per call: s2t_fbank alone (K.fbank, which allocates its result),
s2t_cmvn alone (in place on a buffer, which after the first call holds normalised features: the same work), both
(FbankFrontEnd.features: waves on the device to features on the device), and the torch formulation (unfold, torch.fft.rfft, dense
mel matmul, log, mean / var).  The host figure is the float32 numpy / scipy restatement
of tests/fbank_ref.py with its CMVN, wall-clock, from samples on the host to features on the host, once per round.  Rounds
alternate between the routes; every round is printed, then the median.  The first utterance of every route is held to the bound of
tests/test_fbank_gpu.py against float64.  Bytes: what a call must move (samples read once, features written once; CMVN reads its
batch twice more than it writes it) against the rate of a device-to-device copy measured here.  Needs an MI355X; there is no pass /
fail threshold on the times."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fbank_ref as R  # noqa: E402
from fbk_fairseq_st_amd import fbank as FB  # noqa: E402
from fbk_fairseq_st_amd import kernels as K  # noqa: E402

SHAPES = [(16, 10), (64, 15), (1, 60)]          # utterances, seconds


def make_waves(B, seconds, sr=16000):
    rng = np.random.default_rng(23)
    n = seconds * sr
    t = np.arange(n) / sr
    return np.clip(np.rint(rng.normal(0, 3000, (B, n)) + 2000 * np.sin(2 * np.pi * 200.0 * t)), -32768, 32767).astype(np.int16)


def torch_route(fe, dense):
    window = fe.tables("cuda")[0]

    def run(waves):
        fr = waves.float().unfold(1, fe.W, fe.S)
        fr = fr - fr.mean(-1, keepdim=True)
        y = (fr - fe.preemphasis * torch.cat([fr[..., :1], fr[..., :-1]], -1)) * window
        spec = torch.fft.rfft(y, n=fe.N)[..., :fe.N // 2]
        x = torch.log(torch.clamp((spec.real ** 2 + spec.imag ** 2) @ dense, min=R.FLOOR))
        return x, (x - x.mean(1, keepdim=True)) / x.var(1, keepdim=True).sqrt()
    return run


def host_route(waves):
    return [R.cmvn(R.fbank(w, dtype=np.float32), dtype=np.float32) for w in waves]


def device_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def wall_time(fn, calls):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e6


def copy_rate():
    src = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    us = statistics.median(device_time(lambda: dst.copy_(src), 10) for _ in range(5))
    return 2 * src.numel() / us / 1e3          # GB/s, read + write


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fbank_time.py measures on the GPU"
    print("device:", torch.cuda.get_device_name(0))
    rate = copy_rate()
    print("device-to-device copy of 256 MiB: %.0f GB/s (read + write)" % rate)
    print("16 kHz int16, 80 bins, 25 / 10 ms, povey; rounds %d x %d calls, alternating; us per call" % (a.rounds, a.calls))
    plain, both = FB.FbankFrontEnd(normalize=False), FB.FbankFrontEnd(normalize=True)
    dense = torch.from_numpy(FB.make_mel_bank(80, plain.N, 16000, 20.0, 0.0).T.astype(np.float32)).cuda()
    via_torch = torch_route(plain, dense)
    for B, seconds in SHAPES:
        host = make_waves(B, seconds)
        waves = torch.from_numpy(host).cuda()
        lens = torch.full((B,), host.shape[1], dtype=torch.int64, device="cuda")
        T = plain.num_frames(host.shape[1])
        feats = plain.features(waves, lens)["features"]
        scratch = feats.clone()
        frames = torch.full((B,), T, dtype=torch.int64, device="cuda")
        tables = plain.tables("cuda")
        r64, r32 = R.fbank(host[0]), R.fbank(host[0], dtype=np.float32)
        n64 = R.cmvn(feats[0].cpu().numpy())
        ok = []
        for got in (feats[0], via_torch(waves)[0][0]):
            err, bound = R.compare(got.cpu().numpy(), r64, r32)
            ok.append("%s (worst %.2f of the bound)" % (bool((err <= bound).all()), float((err / bound).max())))
        nk = bool(R.cmvn_within(both.features(waves, lens)["features"][0].cpu().numpy(), n64).all())
        print("%d x %d s: %d frames each; first utterance within the bound: kernel %s, torch formulation %s; kernel CMVN within 1e-4: %s"
              % (B, seconds, T, ok[0], ok[1], nk))
        moved_f = host.nbytes + feats.numel() * 4
        moved_c = feats.numel() * 4 * 4
        routes = [("device  s2t_fbank (K.fbank)", device_time, lambda: K.fbank(waves, lens, *tables, plain.S, plain.N), moved_f),
                  ("device  s2t_cmvn (K.cmvn, in place)", device_time, lambda: K.cmvn(scratch, frames), moved_c),
                  ("device  both: FbankFrontEnd.features, waves to features", device_time, lambda: both.features(waves, lens), moved_f + moved_c),
                  ("device  torch formulation, fbank and CMVN", device_time, lambda: via_torch(waves), None),
                  ("host    float32 numpy / scipy restatement, fbank and CMVN", wall_time, lambda: host_route(host), None)]
        for _, timer, fn, _ in routes[:4]:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in routes]
        for _ in range(a.rounds):
            for i, (_, timer, fn, _) in enumerate(routes):
                if timer is wall_time and len(times[i]) >= 3:
                    continue                                        # the host route runs for seconds: three rounds
                times[i].append(timer(fn, a.calls))
        med = [statistics.median(ts) for ts in times]
        for (tag, _, _, moved), ts, m in zip(routes, times, med):
            extra = "" if moved is None else "; %.1f MB moved at least: %.0f GB/s, %.0f %% of the copy rate" % (moved / 1e6, moved / m / 1e3, 100 * moved / m / 1e3 / rate)
            print("  %-58s %s -> median %.1f us%s" % (tag, " ".join("%.1f" % v for v in ts), m, extra))
        print("  torch formulation / kernels: %.2f x; host / kernels: %.0f x" % (med[3] / med[2], med[4] / med[2]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
