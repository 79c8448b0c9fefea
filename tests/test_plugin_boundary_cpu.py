"""The Python drop-in boundary: `--user-dir fbk_fairseq_st_amd` inside the reference's own CLI flow.

tests/golden/plugin_boundary.json was produced by tests/golden/make_plugin_fixture.py, which runs fairseq's UNCHANGED
`options.get_training_parser` -> `parse_args_and_arch` -> `tasks.setup_task` -> `task.build_model` / `build_criterion`
(fairseq/options.py:81-196, fairseq/utils.py:344-359, fairseq_cli/train.py:43-75) with this package as the user directory.
Here (no reference needed) the package's standalone registries are held to the same outcome: same names registered, same
namespace after the arch function, same classes, same parameter inventory.  Regenerating the fixture needs the reference
itself: `make_plugin_fixture.py --check` does it and must find it identical.
"""
import argparse
import json
import os
import sys

import pytest

from fbk_fairseq_st_amd import registry as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "plugin_boundary.json")))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_plugin_fixture as MPF  # noqa: E402  (argument lists only; nothing of the reference is imported by importing it)


def test_fixture_records_a_bound_plugin():
    assert FIX["registries_are_fairseqs"] and FIX["core_lsce_replaced"] and FIX["duplicate_model_raises"]
    for c in FIX["cases"].values():
        assert c["model_is_fairseq_model"] and c["encoder_is_fairseq_encoder"] and c["decoder_is_incremental"]
        assert c["criterion_is_fairseq_criterion"] and c["task_is_fairseq_task"]


def test_standalone_registries_hold_the_same_names():
    assert not R.inside_fairseq()
    assert sorted(R.ARCH_MODEL_REGISTRY) == FIX["archs_registered_in_fairseq"]
    assert sorted(R.TASK_REGISTRY) == FIX["tasks_registered_in_fairseq"]
    assert sorted(R.CRITERION_REGISTRY) == FIX["criteria_registered_in_fairseq"]


def _standalone_parse(flags):
    """the two-pass parse of options.parse_args_and_arch (options.py:124-192) over this package's own add_args"""
    argv = MPF.COMMON + flags
    base = argparse.ArgumentParser(allow_abbrev=False)
    base.add_argument("--arch"); base.add_argument("--task"); base.add_argument("--criterion")
    base.add_argument("--max-tokens", type=int); base.add_argument("--update-freq", type=lambda s: [int(s)])
    known, _ = base.parse_known_args(argv)
    grp = base.add_argument_group("model", argument_default=argparse.SUPPRESS)
    R.ARCH_MODEL_REGISTRY[known.arch].add_args(grp)
    R.CRITERION_REGISTRY[known.criterion].add_args(base)
    R.TASK_REGISTRY[known.task].add_args(base)
    known, _ = base.parse_known_args(argv)
    if getattr(known, "underlying_criterion", None):
        R.CRITERION_REGISTRY[known.underlying_criterion].add_args(base)
    args, _ = base.parse_known_args(argv)
    return R.apply_arch(args)


@pytest.mark.parametrize("case", sorted(MPF.CASES))
def test_standalone_flow_matches_the_fairseq_flow(case):
    exp = FIX["cases"][case]
    args = _standalone_parse(MPF.CASES[case])
    for k, v in exp["args"].items():
        if k in ("update_freq",):
            continue
        assert hasattr(args, k), k
        assert getattr(args, k) == v, (k, getattr(args, k), v)
    task = R.setup_task(args)
    model, crit = task.build_model(args), task.build_criterion(args)
    cls = lambda o: type(o).__module__ + "." + type(o).__name__
    assert (cls(task), cls(model), cls(crit)) == (exp["task_class"], exp["model_class"], exp["criterion_class"])
    assert sum(p.numel() for p in model.named_arena_params().values()) == exp["n_params"]
    assert len(model.state_dict()) == exp["n_state_keys"]
    assert (len(task.source_dictionary), len(task.target_dictionary)) == (exp["src_dict"], exp["tgt_dict"])
    assert list(model.max_positions()) == exp["max_positions"]
