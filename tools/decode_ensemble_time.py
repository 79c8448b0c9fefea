#!/usr/bin/env python3
"""ms per decode step of beam-5 generation at the Cfg5 shape (bench.py cfg5_beam5: s2t_transformer_m, 16 utterances x 1000 frames,
max_len_b 200, random-init weights) for ensembles of 1, 2 and 4 models, in ONE process:

  device  the device-resident search (n = 1: s2t_decode_step; n > 1: s2t_decode_step_ensemble)
  step    the step-by-step search (S2T_DEVICE_SEARCH=0) for the ensembles: the only route they had before the ensemble entry points

  python tools/decode_ensemble_time.py [--dtypes bf16,fp32] [--members 1,2,4] [--runs 3] [--no-step]

Per line: one warm-up call, then `runs` timed calls (one for the step route); a call's figure is search time / steps
(SequenceGenerator.record_stats: two host synchronisations around the search, the encoders are outside).  Every call's figure is
printed, so that the run-to-run spread is on the page beside the differences.  For the ensembles: the ratio of the step route to the
device route, and the ratio of the device route to n x the one-model step, which shows what the shared row and sentence launches cost
or save.  `--members 1` measures the same search as tools/decode_rules_time.py --variants a (which also runs on a tree that predates
this tool).  The members are separately built models of the same architecture and initialisation: the work per member is the same.
"""
import argparse
import os
import socket
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--members", default="1,2,4")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-step", dest="step", action="store_false", help="skip the step-by-step route")
    args = ap.parse_args()
    import bench
    from fbk_fairseq_st_amd import lib as L
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    B, T, BEAM, MAXLEN = 16, 1000, 5, 200
    dev = torch.device("cuda:0")
    counts = [int(v) for v in args.members.split(",")]
    print("# host %s, %s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0), L.load().s2t_build_info().decode()))
    print("# s2t_transformer_m, %d x %d frames, beam %d, max_len_b %d; ms per decode step = search time / steps" % (B, T, BEAM, MAXLEN))
    for dn in args.dtypes.split(","):
        dtype = torch.bfloat16 if dn == "bf16" else torch.float32
        built = [bench.build_all("s2t_transformer_m", B, T, 40, 0, 1e-9, dtype, dev, criterion="label_smoothed_cross_entropy",
                                 max_target_positions=1024) for _ in range(max(counts))]
        task, trainer = built[0][1], built[0][4]
        for b in built:
            b[2].eval()
        sample = trainer.prepare(task.dummy_batch(seed=100))
        net = {"net_input": {k: v for k, v in sample["net_input"].items() if k in ("src_tokens", "src_lengths")}}
        mean = {}
        for n in counts:
            models = [b[2] for b in built[:n]]
            for route in (("device", "step") if n > 1 and args.step else ("device",)):
                os.environ["S2T_DEVICE_SEARCH"] = "1" if route == "device" else "0"
                gen = SequenceGenerator(models, task.target_dictionary, beam_size=BEAM, max_len_a=0.0, max_len_b=MAXLEN, min_len=1)
                gen.record_stats = True
                gen.generate(models, net)
                ms, steps, launches = [], 0, None
                for _ in range(args.runs if route == "device" else 1):
                    gen.last_stats = {}
                    gen.generate(models, net)
                    st = gen.last_stats
                    assert ("launches_per_step" in st) == (route == "device"), "%d members took the other route" % n
                    steps, launches = st["steps"], st.get("launches_per_step")
                    ms.append(st["search_s"] * 1e3 / steps)
                mean[(n, route)] = sum(ms) / len(ms)
                print("%-5s n %d %-6s steps %3d  launches/step %-4s ms/step %s  mean %.4f" % (
                    dn, n, route, steps, launches if launches else "-", " ".join("%.4f" % m for m in ms), mean[(n, route)]))
        os.environ["S2T_DEVICE_SEARCH"] = "1"
        for n in counts:
            if n > 1 and (n, "step") in mean:
                print("%-5s n %d: step route / device route %.2fx" % (dn, n, mean[(n, "step")] / mean[(n, "device")]))
            if n > 1 and (1, "device") in mean:
                print("%-5s n %d: device route / (n x one-model step) %.3f" % (dn, n, mean[(n, "device")] / (n * mean[(1, "device")])))
        del built, trainer, task, models, gen
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
