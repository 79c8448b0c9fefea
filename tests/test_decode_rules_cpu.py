"""CPU checks of the device search's rule entry points (s2t_decode_step_rules, s2t_decode_graph_create_rules) and of the history
restatement the GPU tests rely on (tests/decode_rules_ref.py)."""
import ctypes
import math

import numpy as np
import torch

import decode_rules_ref as RR
from fbk_fairseq_st_amd import lib as L

EINVAL, ENOTSUP = -22, -95
NEW = ("s2t_decode_step_rules", "s2t_decode_graph_create_rules")


def _bindings():
    """(name, binding) of the ctypes handle and of the generated CPython module"""
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    L.load()
    return [("ctypes", L.load_ctypes()), ("fastcall", fast)]


def test_rule_entry_points_are_exported_and_bound():
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in L.SIGNATURES
    assert L.SIGNATURES["s2t_decode_step_rules"] == [L.P, L.P, L.P]
    assert L.SIGNATURES["s2t_decode_graph_create_rules"] == [L.P, L.P, ctypes.c_int, L.P]
    for what, b in _bindings():
        for name in NEW:
            assert hasattr(b, name), "%s: %s is not bound" % (what, name)
        assert b.s2t_abi_version() == 9, what
    assert ctypes.sizeof(L.DecodeRules) == 16 and L.DecodeRules.prefix.offset == 8        # two ints and a pointer


def test_rule_entry_points_check_their_arguments_before_any_launch():
    """the documented codes (include/s2t_hip.h), none of which needs a GPU: a null descriptor and malformed rules S2T_EINVAL, n-gram
    size 1 S2T_ENOTSUP, then the descriptor's own checks (an all-zero descriptor is outside the limits: S2T_ENOTSUP)"""
    d = L.DecodeDesc()
    da = ctypes.addressof(d)
    some = (ctypes.c_int * 4)()

    def rules(n=0, plen=0, prefix=None):
        r = L.DecodeRules()
        r.no_repeat_ngram, r.prefix_len, r.prefix = n, plen, prefix
        return r
    cases = [(None, None, EINVAL), (None, rules(2), EINVAL),
             (da, rules(-1), EINVAL), (da, rules(0, -1), EINVAL), (da, rules(0, 2, None), EINVAL), (da, rules(2, 3, None), EINVAL),
             (da, rules(1), ENOTSUP), (da, rules(1, 2, ctypes.addressof(some)), ENOTSUP),
             # well-formed rules: the answer is the descriptor's
             (da, None, ENOTSUP), (da, rules(), ENOTSUP), (da, rules(2), ENOTSUP), (da, rules(3, 2, ctypes.addressof(some)), ENOTSUP)]
    ex = ctypes.c_void_p(0)
    for what, b in _bindings():
        for dd, r, want in cases:
            ra = None if r is None else ctypes.addressof(r)
            assert b.s2t_decode_step_rules(dd, ra, None) == want, (what, "step", dd is not None, r and (r.no_repeat_ngram, r.prefix_len))
            assert b.s2t_decode_graph_create_rules(dd, ra, 8, ctypes.addressof(ex)) == want, (what, "graph")
            assert ex.value is None
        r = rules(2)
        assert b.s2t_decode_graph_create_rules(da, ctypes.addressof(r), 0, ctypes.addressof(ex)) == EINVAL
        assert b.s2t_decode_graph_create_rules(da, ctypes.addressof(r), 8, None) == EINVAL
        # the calls without rules answer as before
        assert b.s2t_decode_step(None, None) == EINVAL and b.s2t_decode_step(da, None) == ENOTSUP
        assert b.s2t_decode_graph_create(None, 8, ctypes.addressof(ex)) == EINVAL
        assert b.s2t_decode_graph_create(da, 8, ctypes.addressof(ex)) == ENOTSUP


def _simulate(B, beam, steps, V, seed):
    """a token table carried the way the step-by-step search carries it (rows re-ordered by the chosen parents, one token appended)
    next to the selection records the device search keeps instead"""
    rng = np.random.RandomState(seed)
    N = B * beam
    tokens = np.full((N, steps + 1), -1, np.int64)
    tokens[:, 0] = 2
    tok_hist = np.zeros((steps + 1, N), np.int32)
    par_hist = np.zeros((steps + 1, N), np.int32)
    tok_hist[0] = 2
    tables = [tokens.copy()]
    for t in range(steps):
        parent = (np.arange(N) // beam) * beam + rng.randint(0, beam, N)       # any slot of the same sentence
        tok = rng.randint(4, V, N)
        tokens[:, :t + 1] = tokens[parent][:, :t + 1]
        tokens[:, t + 1] = tok
        tok_hist[t + 1], par_hist[t + 1] = tok, parent
        tables.append(tokens.copy())
    return tables, tok_hist, par_hist


def test_history_from_the_records_equals_the_token_table():
    for B, beam, steps, V, seed in ((2, 4, 20, 9, 0), (1, 5, 40, 6, 1), (3, 2, 12, 5, 2)):
        tables, th, ph = _simulate(B, beam, steps, V, seed)
        for t in range(steps + 1):
            for n in range(B * beam):
                assert RR.history(th, ph, t, n) == tables[t][n, :t + 1].tolist(), (seed, t, n)


def test_bans_equal_the_step_search_rule():
    """banned_columns over the rebuilt histories against SequenceGenerator._no_repeat_ngram on the token table (small vocabularies:
    repeats are frequent); both restate fairseq/sequence_generator.py:617-650"""
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    hits = 0
    for ngram, (B, beam, steps, V, seed) in ((2, (2, 4, 20, 9, 0)), (3, (1, 5, 40, 6, 1)), (4, (3, 2, 30, 5, 2))):
        tables, th, ph = _simulate(B, beam, steps, V, seed)
        gen = SequenceGenerator.__new__(SequenceGenerator)
        gen.no_repeat_ngram_size = ngram
        for t in range(steps + 1):
            lprobs = torch.zeros(B * beam, V)
            gen._no_repeat_ngram(torch.from_numpy(tables[t]), lprobs, t)
            for n in range(B * beam):
                want = set(torch.nonzero(lprobs[n] == -math.inf).view(-1).tolist())
                assert RR.banned_columns(RR.history(th, ph, t, n), ngram) == want, (ngram, t, n)
                hits += len(want)
    assert hits > 50, "the simulation produced hardly any ban"
