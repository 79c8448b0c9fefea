"""CPU checks of the device search's ensemble entry points (s2t_decode_begin_ensemble, s2t_decode_step_ensemble,
s2t_decode_graph_create_ensemble): exported, in the signature table, bound by both bindings, and every return code
include/s2t_hip.h documents for arguments that are refused before any launch -- none of which needs a GPU."""
import ctypes

from fbk_fairseq_st_amd import lib as L

EINVAL, ENOTSUP = -22, -95
NEW = ("s2t_decode_begin_ensemble", "s2t_decode_step_ensemble", "s2t_decode_graph_create_ensemble")


def _bindings():
    """(name, binding) of the ctypes handle and of the generated CPython module"""
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    L.load()
    return [("ctypes", L.load_ctypes()), ("fastcall", fast)]


def _array(descs):
    """HOST array of descriptor addresses (None = a NULL entry); returns (array, its address)"""
    arr = (ctypes.c_void_p * max(len(descs), 1))(*[None if d is None else ctypes.addressof(d) for d in descs])
    return arr, ctypes.addressof(arr)


def _rules(n=0, plen=0, prefix=None):
    r = L.DecodeRules()
    r.no_repeat_ngram, r.prefix_len, r.prefix = n, plen, prefix
    return r


def test_ensemble_entry_points_are_exported_and_bound():
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in L.SIGNATURES
    assert L.SIGNATURES["s2t_decode_begin_ensemble"] == [L.P, ctypes.c_int, ctypes.c_int, L.P]
    assert L.SIGNATURES["s2t_decode_step_ensemble"] == [L.P, ctypes.c_int, L.P, L.P]
    assert L.SIGNATURES["s2t_decode_graph_create_ensemble"] == [L.P, ctypes.c_int, L.P, ctypes.c_int, L.P]
    for what, b in _bindings():
        for name in NEW:
            assert hasattr(b, name), "%s: %s is not bound" % (what, name)
        assert b.s2t_abi_version() == 9, what
    assert L.ABI_VERSION == 9
    assert ctypes.sizeof(L.DecodeRules) == 16                        # the layouts the calls share with the one-model ones


def _all(b, arr, n, r, bos=2):
    """the answers of the three calls for one argument set; graph_exec must be left NULL"""
    ex = ctypes.c_void_p(0)
    ra = None if r is None else ctypes.addressof(r)
    out = (b.s2t_decode_begin_ensemble(arr, n, bos, None), b.s2t_decode_step_ensemble(arr, n, ra, None),
           b.s2t_decode_graph_create_ensemble(arr, n, ra, 8, ctypes.addressof(ex)))
    assert ex.value is None, "graph_exec was written by a failed create"
    return out


def test_ensemble_entry_points_check_their_arguments_before_any_launch():
    """the documented order: the array (NULL, n outside 1..8, a NULL member) S2T_EINVAL; then the rules (malformed S2T_EINVAL, n-gram
    size 1 S2T_ENOTSUP); then the shared fields (S2T_EINVAL); then every member's own checks (an all-zero member is outside the limits:
    S2T_ENOTSUP)"""
    zero = [L.DecodeDesc() for _ in range(9)]
    some = (ctypes.c_int * 4)()
    for what, b in _bindings():
        # 1. the array
        _, a2 = _array(zero[:2])
        assert _all(b, None, 2, None) == (EINVAL,) * 3, what
        assert _all(b, a2, 0, None) == (EINVAL,) * 3, what
        assert _all(b, a2, -1, None) == (EINVAL,) * 3, what
        keep9, a9 = _array(zero)
        assert _all(b, a9, 9, None) == (EINVAL,) * 3, what
        keepn, an = _array([zero[0], None])
        assert _all(b, an, 2, None) == (EINVAL,) * 3, what
        # ... which comes before the rules: n-gram size 1 alone would be ENOTSUP
        assert _all(b, a9, 9, _rules(1))[1:] == (EINVAL,) * 2, what
        # 2. the rules, before the members are compared or checked (begin takes none)
        for r, want in ((_rules(-1), EINVAL), (_rules(0, -1), EINVAL), (_rules(0, 2, None), EINVAL), (_rules(1), ENOTSUP),
                        (_rules(1, 2, ctypes.addressof(some)), ENOTSUP)):
            for n in (1, 2, 8):
                assert _all(b, a9, n, r)[1:] == (want,) * 2, (what, n, r.no_repeat_ngram, r.prefix_len)
        mism = [L.DecodeDesc(), L.DecodeDesc()]
        mism[1].V = 100
        keepm, am = _array(mism)
        assert _all(b, am, 2, _rules(1))[1:] == (ENOTSUP,) * 2, what             # the rules answer before the mismatch does
        assert _all(b, am, 2, _rules(-1))[1:] == (EINVAL,) * 2, what
        # 3. members that disagree on a shared field: each alone, against an otherwise identical (all-zero) member
        assert _all(b, am, 2, None) == (EINVAL,) * 3, what
        for field, value in (("dtype", 1), ("B", 2), ("beam", 3), ("V", 96), ("ldv", 96), ("max_len", 5), ("min_len", 1), ("pad", 1), ("unk", 3),
                             ("eos", 2), ("step0_all_slots", 1), ("unk_penalty", 0.5), ("inv_temperature", 2.0),
                             ("steps", ctypes.addressof(some)), ("anc", ctypes.addressof(some)), ("tok_hist", ctypes.addressof(some)),
                             ("par_hist", ctypes.addressof(some)), ("cum_hist", ctypes.addressof(some)), ("blacklist", ctypes.addressof(some)),
                             ("nfin", ctypes.addressof(some)), ("finished", ctypes.addressof(some)), ("fin_step", ctypes.addressof(some)),
                             ("fin_row", ctypes.addressof(some)), ("fin_score", ctypes.addressof(some)), ("cand_val", ctypes.addressof(some)),
                             ("cand_idx", ctypes.addressof(some)), ("init_scores", ctypes.addressof(some))):
            pair = [L.DecodeDesc(), L.DecodeDesc(), L.DecodeDesc()]
            setattr(pair[2], field, value)
            keepp, ap = _array(pair)
            assert _all(b, ap, 3, None) == (EINVAL,) * 3, (what, field)
            assert _all(b, ap, 3, _rules(2))[1:] == (EINVAL,) * 2, (what, field)
            assert _all(b, ap, 2, None) == (ENOTSUP,) * 3, (what, field)         # the member that differs is not among the first two
        # fields that members may differ in do not make the ensemble malformed: the answer is the members' own (all outside the limits)
        free = [L.DecodeDesc(), L.DecodeDesc()]
        free[1].D, free[1].heads, free[1].layers, free[1].ffn, free[1].ffn_slices, free[1].Ts, free[1].Tsp, free[1].gelu = 512, 8, 2, 2048, 16, 300, 384, 1
        free[1].embed_scale, free[1].ln_eps, free[1].logits, free[1].x0 = 22.6, 1e-5, ctypes.addressof(some), ctypes.addressof(some)
        keepf, af = _array(free)
        assert _all(b, af, 2, None) == (ENOTSUP,) * 3, what
        # 4. the members' own checks: all-zero members, n = 1 .. 8, with and without well-formed rules
        for n in (1, 2, 8):
            assert _all(b, a9, n, None) == (ENOTSUP,) * 3, (what, n)
            assert _all(b, a9, n, _rules()) == (ENOTSUP,) * 3, (what, n)
            assert _all(b, a9, n, _rules(3, 2, ctypes.addressof(some))) == (ENOTSUP,) * 3, (what, n)
        # graph_create: graph_exec and n_steps first
        ex = ctypes.c_void_p(0)
        for steps in (0, -1, 65):
            assert b.s2t_decode_graph_create_ensemble(a9, 2, None, steps, ctypes.addressof(ex)) == EINVAL, (what, steps)
        assert b.s2t_decode_graph_create_ensemble(a9, 2, None, 8, None) == EINVAL, what
        assert b.s2t_decode_graph_create_ensemble(None, 2, None, 0, ctypes.addressof(ex)) == EINVAL, what
        assert ex.value is None
        # the one-model calls answer as before
        da = ctypes.addressof(zero[0])
        assert b.s2t_decode_begin(da, 2, None) == ENOTSUP and b.s2t_decode_step(da, None) == ENOTSUP
        assert b.s2t_decode_step_rules(da, None, None) == ENOTSUP and b.s2t_decode_step(None, None) == EINVAL
        assert b.s2t_decode_graph_create(da, 8, ctypes.addressof(ex)) == ENOTSUP and ex.value is None
