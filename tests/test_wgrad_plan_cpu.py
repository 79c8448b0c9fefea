"""The work-list planners of the grouped weight-gradient kernels (fbk_fairseq_st_amd/csrc/wgrad_plan.hpp), checked on the host.

tests/host/wgrad_plan_check.cpp includes only that header; it is compiled here with the host C++ compiler and run.  It checks, on
every list it plans: every (problem, tm, tn) tile appears, its pieces along the tokens are disjoint and cover [0, nk) exactly, a
tile of several pieces is atomic on all of them, item fields are in range, 1 <= used <= G (bf16) / grid = min(items, 512) (f32),
the kernels' walk (slot s: s, s + used, ... up to the first empty item) reaches every non-empty item exactly once, the reported
makespan is load_of recomputed, the chosen bf16 layout is the lighter one, and the same input gives the same plan twice.

  * 20,000 seeded random lists per planner (four runs of 5,000), G from what reserve_cus can produce,
  * the edge lists (one 8 x 8 product of one token, 4,096 products, one product far above the fair share),
  * the named lists of tests/wgrad_lists.py: the table there is what the GPU cases of tests/test_wgrad_group_gpu.py cite for "this
    list has cut tiles" / "this list runs the fill layout".
"""
import os
import shutil
import subprocess

import pytest

import wgrad_lists

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "wgrad_plan_check.cpp")
INC = os.path.join(REPO, "fbk_fairseq_st_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-I", INC, SRC, "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    return exe


def run(exe, *args, stdin=""):
    r = subprocess.run([exe] + [str(a) for a in args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), "wgrad_plan_check %s:\n%s" % (" ".join(str(a) for a in args), r.stdout[-4000:])
    return dict(kv.split("=") for kv in r.stdout.split()[1:] if "=" in kv)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_invariants_on_random_lists(checker, seed):
    """5,000 lists per planner and seed; the counts prove that the random lists reach the fill layout and the cuts of both planners"""
    got = run(checker, "random", 5000, seed)
    assert int(got["lists_bf16"]) == 5000 and int(got["lists_f32"]) == 5000
    assert int(got["fill"]) >= 500 and int(got["cut"]) >= 1000 and int(got["cut_f32"]) >= 200, got


def test_invariants_on_edge_lists(checker):
    run(checker, "edges")


@pytest.mark.parametrize("row", wgrad_lists.PLANS, ids=[p[0].replace(" ", "_") for p in wgrad_lists.PLANS])
def test_named_lists_are_planned_as_stated(checker, row):
    name, shapes, planner, G, want = row
    got = run(checker, "plan", planner, G or 256, stdin="".join("1 %d %d %d\n" % s for s in shapes))
    assert got["layout"] == want["layout"], got
    for key in ("items", "cut_tiles", "atomic_items"):
        assert int(got[key]) == want[key], (key, got)
    if "pieces" in want:
        assert int(got["min_pieces"]) == int(got["max_pieces"]) == want["pieces"], got
    if "makespan" in want:
        assert int(got["makespan"]) == want["makespan"], got


def test_entry_points_use_the_header():
    """the planners exist once: neither kernel file keeps a copy of what the host program checks"""
    for f in ("wgrad_group.hip", "wgrad_f32.hip"):
        text = open(os.path.join(INC, f)).read()
        assert '#include "wgrad_plan.hpp"' in text and "stable_sort" not in text, f
    assert "wgrad_plan.hpp" in open(os.path.join(INC, "Makefile")).read()
