#!/usr/bin/env python3
"""tests/golden/bleu_stats.npz: what the reference's own BLEU code gives on about 300 small token pairs (build container only: needs
/root/reference and g++).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bleu_fixture.py [--check]

The reference's clib/libbleu is compiled into a temporary directory (as tests/golden/make_cli_fixture.py does) and its
fairseq/bleu.py is loaded on top of it; nothing compiled is kept.  Recorded: the token matrices and lengths, pad / eos / unk, the ten
numbers `bleu_add` adds for every pair on its own (`Scorer.add` after `reset()`), and `Scorer.result_string()` over the whole set and
over three subsets.  The pairs hold alphabets of 2, 3 and 50 symbols, noisy copies, leading and trailing pads, pad and eos in the
interior, [eos] alone, runs of one symbol against a shorter run, and unk on either side.  No side is empty after the left trim: the
reference reads out of bounds there.
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "bleu_stats.npz")
PAD, EOS, UNK = 1, 2, 3
WIDTH = 40
FIELDS = ("reflen", "predlen", "match1", "count1", "match2", "count2", "match3", "count3", "match4", "count4")
SUBSETS = {"all": None, "first": (0, 60), "small_alphabets": (60, 180), "quirks": (180, None)}


def reference_bleu():
    """the reference's fairseq.bleu over its libbleu built in a scratch directory, without importing the rest of fairseq"""
    sys.dont_write_bytecode = True
    tmp = tempfile.mkdtemp(prefix="s2t_bleu_")
    so = os.path.join(tmp, "libbleu" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-shared", "-fPIC", "-O2", "-w", "-I", sysconfig.get_paths()["include"],
                           REF + "/fairseq/clib/libbleu/libbleu.cpp", REF + "/fairseq/clib/libbleu/module.cpp", "-o", so])
    spec = importlib.util.spec_from_file_location("fairseq.libbleu", so)
    lib = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lib)
    pkg = type(sys)("fairseq")
    pkg.__path__ = []
    pkg.libbleu = lib
    sys.modules["fairseq"], sys.modules["fairseq.libbleu"] = pkg, lib
    spec = importlib.util.spec_from_file_location("fairseq.bleu", REF + "/fairseq/bleu.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pairs():
    rng = np.random.default_rng(20261020)
    out = []
    sym = lambda k, n: (4 + rng.integers(0, k, n)).tolist()

    def noisy(ref, k):
        hyp = []
        for t in ref:
            u = rng.random()
            if u < 0.15:
                continue
            hyp.append(int(4 + rng.integers(0, k)) if u < 0.3 else t)
            if u > 0.9:
                hyp.append(int(4 + rng.integers(0, k)))
        return hyp[:WIDTH - 1] or sym(k, 1)

    # 0 .. 59: sentences as a search returns them (eos at the end), 50 symbols, noisy copies
    for _ in range(60):
        ref = sym(50, int(rng.integers(1, WIDTH)))
        out.append((noisy(ref, 50) + [EOS], ref + [EOS]))
    # 60 .. 179: alphabets of 2 and 3, every length, clipping decides
    for q in range(120):
        k = 2 + q % 2
        out.append((sym(k, int(rng.integers(1, WIDTH + 1))), sym(k, int(rng.integers(1, WIDTH + 1)))))
    # 180 ..: the quirks
    for q in range(30):                                            # leading pads, trailing eos and pads
        k = (2, 3, 50)[q % 3]
        ref = sym(k, int(rng.integers(1, 20)))
        hyp = noisy(ref, k)[:19]
        lead, trail = [PAD] * int(rng.integers(0, 5)), [(EOS, PAD)[int(rng.integers(0, 2))] for _ in range(int(rng.integers(0, 6)))]
        out.append((lead + hyp + trail, [PAD] * int(rng.integers(0, 4)) + ref + [EOS] * int(rng.integers(0, 4)) + [PAD] * int(rng.integers(0, 4))))
    for q in range(30):                                            # pad and eos in the interior
        k = (2, 3)[q % 2]
        ref, hyp = sym(k, 12), sym(k, 12)
        for s in (ref, hyp):
            for at in rng.integers(1, 11, 3):
                s[int(at)] = (PAD, EOS)[int(rng.integers(0, 2))]
        out.append((hyp + [EOS], ref + [EOS, PAD]))
    out += [([EOS], [EOS]), ([EOS], [4, 5, EOS]), ([4, 5, EOS], [EOS]), ([EOS, EOS, EOS], [EOS, EOS]), ([PAD, EOS], [EOS, PAD, PAD]),
            ([EOS, PAD, EOS], [EOS, 4]), ([PAD, PAD, EOS, EOS], [4, EOS]), ([EOS, 4, EOS], [EOS, 4, EOS]), ([4], [4]), ([4], [5])]
    for n, m in ((1, 1), (5, 2), (2, 5), (7, 7), (40, 3), (3, 40), (40, 39), (4, 4), (4, 3), (3, 4), (6, 1), (1, 6)):
        out.append(([4] * n, [4] * m))                             # runs of one symbol
        out.append(([4] * min(n, WIDTH - 1) + [5], [5] + [4] * min(m, WIDTH - 1)))
    for q in range(40):                                            # unk on either side
        k = (2, 3, 50)[q % 3]
        ref = sym(k, int(rng.integers(2, 25)))
        hyp = noisy(ref, k)
        for s, p in ((ref, (0.0, 0.3, 0.3, 0.6)[q % 4]), (hyp, (0.3, 0.0, 0.3, 0.6)[q % 4])):
            for at in range(len(s)):
                if rng.random() < p:
                    s[at] = UNK
        out.append((hyp, ref + [EOS] * (q % 2)))
    out += [([UNK], [UNK]), ([UNK, UNK, UNK, UNK, UNK], [UNK, UNK, UNK, UNK, UNK]), ([4, UNK, 5], [4, UNK, 5]), ([UNK, EOS], [4, EOS])]
    assert all(1 <= len(h) <= WIDTH and 1 <= len(r) <= WIDTH for h, r in out)
    assert all(any(t != PAD for t in h) and any(t != PAD for t in r) for h, r in out), "a side empty after the left trim"
    return out


def run():
    import torch
    bleu = reference_bleu()
    ps = pairs()
    N = len(ps)
    hyp, ref = np.full((N, WIDTH), PAD, np.int32), np.full((N, WIDTH), PAD, np.int32)
    hyp_len, ref_len, stats = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros((N, 10), np.int32)
    one = bleu.Scorer(PAD, EOS, UNK)
    for s, (h, r) in enumerate(ps):
        hyp[s, :len(h)], ref[s, :len(r)], hyp_len[s], ref_len[s] = h, r, len(h), len(r)
        one.reset()
        one.add(torch.IntTensor(r), torch.IntTensor(h))
        stats[s] = [getattr(one.stat, f) for f in FIELDS]
    res = {"hyp": hyp, "hyp_len": hyp_len, "ref": ref, "ref_len": ref_len, "stats": stats,
           "pad": np.int32(PAD), "eos": np.int32(EOS), "unk": np.int32(UNK)}
    for name, span in SUBSETS.items():
        lo, hi = span or (0, None)
        idx = np.arange(N)[lo:hi]
        sc = bleu.Scorer(PAD, EOS, UNK)
        for s in idx:
            sc.add(torch.IntTensor(ps[s][1]), torch.IntTensor(ps[s][0]))
        assert [getattr(sc.stat, f) for f in FIELDS] == stats[idx].sum(0).tolist()
        res["subset_" + name] = idx.astype(np.int32)
        res["string_" + name] = np.array(sc.result_string())
        res["string2_" + name] = np.array(sc.result_string(order=2))
        res["score_" + name] = np.float64(sc.score())
    return res


if __name__ == "__main__":
    res = run()
    if "--check" in sys.argv:
        old = dict(np.load(OUT))
        assert sorted(old) == sorted(res) and all(np.array_equal(old[k], res[k]) for k in res), "bleu_stats.npz is stale"
        print("BLEU fixture up to date")
    else:
        np.savez_compressed(OUT, **res)
        print("wrote %s: %d pairs, %d bytes; %s" % (OUT, len(res["hyp"]), os.path.getsize(OUT), res["string_all"]))
