#!/usr/bin/env python3
"""ms per decode step of generation at the Cfg5 shape (bench.py cfg5_beam5: s2t_transformer_m, 16 utterances x 1000 frames, max_len_b 200,
random-init weights) with group-diverse beam search (--diverse-beam-groups), on ONE box in one job:

  (a) plain beam search at beam 6, another build of the library (--parent-lib: the parent commit's libs2t_hip.so) against this one,
      alternating, each call of a build in a process of its own (a process loads one library; both through S2T_HIP_LIB, i.e. the
      ctypes binding): the diverse form is a template parameter of the per-sentence kernel and may not cost the plain one anything;
  (b) diverse search beam 6 / 3 groups and beam 4 / 2 groups beside the plain search at the same beam, one process;
  (c) the same diverse searches on the step-by-step route (S2T_DEVICE_SEARCH=0): what (b) replaces.

  python tools/decode_diverse_time.py [--parent-lib PATH] [--dtypes bf16,fp32] [--runs 3] [--rounds 3]

A call's figure is search time / steps (SequenceGenerator.record_stats: two host synchronisations around the search, the encoder is
outside).  Every call's figure is printed, so that the run-to-run spread is on the page beside the differences.
"""
import argparse
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, T, MAXLEN = 16, 1000, 200
#            name             device route  beam groups strength
VARIANTS = {"plain6": ("plain b6", True, 6, 0, 0.0), "div6": ("diverse b6/G3", True, 6, 3, 0.5), "plain4": ("plain b4", True, 4, 0, 0.0),
            "div4": ("diverse b4/G2", True, 4, 2, 0.5), "step6": ("step-route diverse b6/G3", False, 6, 3, 0.5),
            "step4": ("step-route diverse b4/G2", False, 4, 2, 0.5)}


def child(args):
    import torch
    import bench
    from fbk_fairseq_st_amd import lib as L
    from fbk_fairseq_st_amd import sequence_generator as SG
    dev = torch.device("cuda:0")
    print("# %s: host %s, %s, %s" % (args.label, socket.gethostname(), torch.cuda.get_device_name(0), L.load().s2t_build_info().decode()), flush=True)
    for dn in args.dtypes.split(","):
        dtype = torch.bfloat16 if dn == "bf16" else torch.float32
        a, task, model, crit, trainer, _ = bench.build_all("s2t_transformer_m", B, T, 40, 0, 1e-9, dtype, dev,
                                                           criterion="label_smoothed_cross_entropy", max_target_positions=1024)
        model.eval()
        sample = trainer.prepare(task.dummy_batch(seed=100))
        net = {"net_input": {k: v for k, v in sample["net_input"].items() if k in ("src_tokens", "src_lengths")}}
        for v in args.variants.split(","):
            name, device_route, beam, groups, strength = VARIANTS[v]
            os.environ["S2T_DEVICE_SEARCH"] = "1" if device_route else "0"
            kw = dict(search_strategy=SG.DiverseBeamSearch(task.target_dictionary, groups, strength)) if groups else {}
            gen = SG.SequenceGenerator([model], task.target_dictionary, beam_size=beam, max_len_a=0.0, max_len_b=MAXLEN, min_len=1, **kw)
            gen.record_stats = True
            gen.generate([model], net)
            ms, steps = [], 0
            for _ in range(args.runs if device_route else 1):
                gen.last_stats = {}
                gen.generate([model], net)
                st = gen.last_stats
                assert ("launches_per_step" in st) == device_route, "variant %s took the other route" % name
                steps = st["steps"]
                ms.append(st["search_s"] * 1e3 / steps)
            print("%-5s %-8s %-26s steps %3d  ms/step %s  mean %.4f" % (dn, args.label, name, steps, " ".join("%.4f" % m for m in ms),
                                                                       sum(ms) / len(ms)), flush=True)
        del trainer, model, crit, task
        torch.cuda.empty_cache()


def run_child(label, lib, variants, args):
    """one fresh process per call of a build: the library is loaded once per process"""
    env = dict(os.environ)
    if lib:
        env["S2T_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--variants", variants, "--dtypes", args.dtypes,
           "--runs", str(args.runs)]
    res = subprocess.run(cmd, env=env, timeout=args.child_timeout)
    if res.returncode != 0:
        raise SystemExit("%s: child exited with %d; nothing more is started" % (label, res.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--variants", default="plain6,div6,plain4,div4,step6,step4")
    args = ap.parse_args()
    if args.child:
        return child(args)
    print("# s2t_transformer_m, %d x %d frames, max_len_b %d; ms per decode step = search time / steps" % (B, T, MAXLEN), flush=True)
    if args.parent_lib:
        from fbk_fairseq_st_amd import lib as L           # the path only: nothing is loaded in this process
        this = os.path.join(os.path.dirname(L.__file__), "libs2t_hip.so")
        print("# (a) plain beam 6: parent build / this build, alternating, one process per call", flush=True)
        for _ in range(args.rounds):
            run_child("parent", os.path.abspath(args.parent_lib), "plain6", args)
            run_child("this", this, "plain6", args)
    print("# (b) diverse beside plain at the same beam, (c) the step-by-step route; one process", flush=True)
    run_child("this", "", args.variants, args)


if __name__ == "__main__":
    main()
