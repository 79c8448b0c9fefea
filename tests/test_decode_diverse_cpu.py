"""CPU checks of group-diverse beam search (--diverse-beam-groups): the host class and the numpy restatement of the device form against
outputs captured from the reference (tests/golden/diverse.npz, made by tests/golden/make_diverse_fixture.py), the descriptor ABI of the
new fields, and the construction of the generator."""
import ctypes

import numpy as np
import pytest
import torch

import decode_diverse_ref as DR
from helpers import load_golden
from fbk_fairseq_st_amd import lib as L

EINVAL, ENOTSUP = -22, -95
PAD, EOS, UNK = 1, 2, 3


class _Dict:
    def __init__(self, V):
        self.V = V

    def pad(self):
        return PAD

    def eos(self):
        return EOS

    def unk(self):
        return UNK

    def __len__(self):
        return self.V


def _step_cases():
    g = load_golden("diverse")
    out = []
    for i in range(int(g["n_step"])):
        step, G, lam = g["s%d_par" % i]
        out.append(dict(i=i, lprobs=g["s%d_lprobs" % i], cum=g["s%d_scores" % i], step=int(step), G=int(G), lam=float(lam),
                        scores=g["s%d_out_scores" % i], tokens=g["s%d_out_tokens" % i], beams=g["s%d_out_beams" % i]))
    return out


def test_fixture_covers_the_edges():
    cs = _step_cases()
    assert len(cs) >= 12
    assert any(c["step"] == 0 for c in cs) and any(c["step"] > 0 for c in cs)
    assert any(c["G"] == 1 for c in cs) and any(c["G"] == c["lprobs"].shape[0] for c in cs)
    assert any(c["lam"] == 0.0 and c["G"] > 1 for c in cs)
    # the groups do collide: some later group's candidates differ from what it would take without the penalty
    assert any(len(set(c["tokens"].tolist())) < len(c["tokens"]) for c in cs)


def test_host_class_reproduces_the_reference_step():
    from fbk_fairseq_st_amd.sequence_generator import DiverseBeamSearch
    for c in _step_cases():
        beam, V = c["lprobs"].shape
        lp = torch.from_numpy(c["lprobs"])[None]
        sc = torch.zeros(1, beam, max(c["step"], 1))
        sc[0, :, c["step"] - 1] = torch.from_numpy(c["cum"])
        s, t, b = DiverseBeamSearch(_Dict(V), c["G"], c["lam"]).step(c["step"], lp.clone(), sc)
        assert t[0].tolist() == c["tokens"].tolist(), c["i"]
        assert b[0].tolist() == c["beams"].tolist(), c["i"]
        np.testing.assert_allclose(s[0].numpy(), c["scores"], rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        DiverseBeamSearch(_Dict(40), 3, 0.5).step(1, torch.zeros(1, 4, 40), torch.zeros(1, 4, 1))


def _row_lists(c):
    """what dec_row_kernel leaves for dec_sent_kernel: every row's 2 beam best of log-probability + cumulative score (value descending,
    column ascending); at step 0 only the sentence's first row is live"""
    beam, V = c["lprobs"].shape
    K2 = 2 * beam
    cv = np.full((beam, K2), -np.inf, np.float32)
    ci = np.zeros((beam, K2), np.int64)
    for r in range(beam):
        if c["step"] == 0 and r > 0:
            v = np.full(V, -np.inf, np.float32)
        else:
            v = (c["lprobs"][r] + np.float32(c["cum"][r])).astype(np.float32)
        order = sorted(range(V), key=lambda col: (-v[col], col))[:K2]
        cv[r], ci[r] = v[order], order
    return cv, ci


def _restated(c, **wrong):
    cv, ci = _row_lists(c)
    beam, V = c["lprobs"].shape
    return DR.diverse_candidates(cv, ci, beam, V, c["G"], c["lam"], c["step"] == 0, **wrong)


def test_restatement_from_the_row_lists_reproduces_the_reference_step():
    """the sufficiency argument: a selection made only from the rows' 2 beam best gives the reference's candidates (which it takes from
    whole rows), tokens and beams exactly, scores to the rounding of a different order of additions"""
    for c in _step_cases():
        val, tok, slot = _restated(c)
        assert tok.tolist() == c["tokens"].tolist(), c["i"]
        assert slot.tolist() == c["beams"].tolist(), c["i"]
        np.testing.assert_allclose(val, c["scores"], rtol=0, atol=1e-5)


@pytest.mark.parametrize("wrong", [dict(count_all=False), dict(interleave=False), dict(sign=1.0)], ids=["count_first_mg", "concatenated", "added"])
def test_wrong_references_are_caught(wrong):
    bad = 0
    for c in _step_cases():
        val, tok, slot = _restated(c, **wrong)
        if tok.tolist() != c["tokens"].tolist() or slot.tolist() != c["beams"].tolist() or np.abs(val - c["scores"]).max() > 1e-5:
            bad += 1
    assert bad > 0, "the fixture does not tell this wrong reference from the right one"


def test_sent_step_diverse_keeps_the_bookkeeping_of_the_plain_step():
    """with G <= 1 the restatement IS decode_ref.sent_step; with G > 1 its records hold the ranked candidates' own values, tokens and
    parents, and EOS candidates among the first `beam` ranks are finalised"""
    import decode_ref as R
    c = [x for x in _step_cases() if x["G"] == 2 and x["step"] > 0][0]
    beam, V = c["lprobs"].shape
    cv, ci = _row_lists(c)
    st = R.new_state(1, beam, 8, EOS)
    st["steps"][0] = c["step"]
    val, tok, slot = _restated(c)
    DR.sent_step_diverse(st, cv, ci.astype(np.int32), beam, V, EOS, 8, c["G"], c["lam"])
    t = c["step"]
    pick = [i for i in range(2 * beam) if tok[i] != EOS][:beam]
    assert st["tok_hist"][t + 1].tolist() == [int(tok[i]) for i in pick]
    assert st["par_hist"][t + 1].tolist() == [int(slot[i]) for i in pick]
    assert st["cum_hist"][t + 1].view(np.int32).tolist() == val[pick].view(np.int32).tolist()
    assert int(st["nfin"][0]) == sum(1 for i in range(beam) if tok[i] == EOS) and int(st["steps"][0]) == t + 1


# ------------------------------------------------------------------ descriptor ABI
def _bindings():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    L.load()
    return [("ctypes", L.load_ctypes()), ("fastcall", fast)]


def test_the_new_fields_are_the_last_two_of_the_descriptor():
    names = [f[0] for f in L.DecodeDesc._fields_]
    assert names[-2:] == ["diverse_groups", "diverse_strength"]
    assert L.DecodeDesc.diverse_groups.offset == L.DecodeDesc.fin_score.offset + 8
    assert L.DecodeDesc.diverse_strength.offset == L.DecodeDesc.diverse_groups.offset + 4
    assert ctypes.sizeof(L.DecodeDesc) == L.DecodeDesc.diverse_groups.offset + 8
    assert ctypes.sizeof(L.DecodeRules) == 16                          # the rules did not grow


def test_every_entry_point_refuses_the_documented_combinations_before_any_launch():
    """on zeroed descriptors, which are themselves outside the limits (S2T_ENOTSUP): the diverse fields answer first"""
    def desc(**kw):
        d = L.DecodeDesc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = [(dict(diverse_groups=-1), EINVAL), (dict(diverse_groups=-3, diverse_strength=0.5), EINVAL),
             (dict(diverse_groups=2, beam=5, diverse_strength=0.5), EINVAL), (dict(diverse_groups=4, beam=6, diverse_strength=-1.0), EINVAL),
             (dict(diverse_groups=2, beam=4, diverse_strength=-0.5), ENOTSUP), (dict(diverse_groups=2, beam=4, diverse_strength=float("inf")), ENOTSUP),
             (dict(diverse_groups=2, beam=4, diverse_strength=float("nan")), ENOTSUP),
             (dict(diverse_groups=2, beam=4, diverse_strength=0.5, step0_all_slots=1), ENOTSUP),
             # plain: the strength is not looked at, the answer is the zeroed descriptor's own
             (dict(diverse_groups=0, diverse_strength=-1.0), ENOTSUP), (dict(diverse_groups=1, beam=5, diverse_strength=float("nan")), ENOTSUP),
             (dict(diverse_groups=2, beam=4, diverse_strength=0.5), ENOTSUP)]
    r = L.DecodeRules()
    r.no_repeat_ngram = 2
    ex = ctypes.c_void_p(0)
    for what, b in _bindings():
        for kw, want in cases:
            d = desc(**kw)
            da = ctypes.addressof(d)
            arr = (ctypes.c_void_p * 1)(da)
            aa = ctypes.addressof(arr)
            got = dict(step=b.s2t_decode_step(da, None), rules=b.s2t_decode_step_rules(da, ctypes.addressof(r), None),
                       ens=b.s2t_decode_step_ensemble(aa, 1, None, None), graph=b.s2t_decode_graph_create(da, 8, ctypes.addressof(ex)),
                       graph_rules=b.s2t_decode_graph_create_rules(da, ctypes.addressof(r), 8, ctypes.addressof(ex)),
                       graph_ens=b.s2t_decode_graph_create_ensemble(aa, 1, None, 8, ctypes.addressof(ex)))
            assert ex.value is None
            assert got == {k: want for k in got}, (what, kw, got)
        # ensemble members must agree on both fields
        for field, value in (("diverse_groups", 2), ("diverse_strength", 0.5)):
            pair = [L.DecodeDesc(), L.DecodeDesc()]
            setattr(pair[1], field, value)
            arr = (ctypes.c_void_p * 2)(*[ctypes.addressof(p) for p in pair])
            assert b.s2t_decode_step_ensemble(ctypes.addressof(arr), 2, None, None) == EINVAL, (what, field)
            assert b.s2t_decode_graph_create_ensemble(ctypes.addressof(arr), 2, None, 8, ctypes.addressof(ex)) == EINVAL, (what, field)


# ------------------------------------------------------------------ generator construction
class _Model:
    training = False

    def eval(self):
        return self


def _build(**kw):
    from fbk_fairseq_st_amd.registry import FairseqTask, namespace

    class T(FairseqTask):
        def __init__(self, tgt):
            self._tgt = tgt

        @property
        def target_dictionary(self):
            return self._tgt
    from fbk_fairseq_st_amd.data import Dictionary
    return T(Dictionary.synthetic(96)).build_generator([_Model()], namespace(beam=6, **kw))


def test_build_generator_builds_the_strategy():
    from fbk_fairseq_st_amd.sequence_generator import BeamSearch, DiverseBeamSearch
    gen = _build(diverse_beam_groups=3, diverse_beam_strength=1.5)
    assert type(gen.search) is DiverseBeamSearch and gen.search.num_groups == 3 and gen.search.diversity_strength == -1.5
    assert _build(diverse_beam_groups=2).search.diversity_strength == -0.5          # the reference's default strength
    assert type(_build().search) is BeamSearch and type(_build(diverse_beam_groups=-1).search) is BeamSearch


def test_build_generator_refuses_what_it_refused_and_exclusive_options():
    for kw in (dict(sampling=True, diverse_beam_groups=2), dict(diverse_beam_groups=2, diversity_rate=0.5),
               dict(match_source_len=True, diverse_beam_groups=2), dict(sampling=True, diversity_rate=0.5)):
        with pytest.raises(ValueError, match="mutually exclusive"):
            _build(**kw)
    for kw in (dict(sampling=True), dict(score_reference=True), dict(match_source_len=True)):
        with pytest.raises(NotImplementedError):
            _build(**kw)
    with pytest.raises(NotImplementedError, match="torch.div"):
        _build(diversity_rate=0.5)


def test_two_phase_generator_refuses_diverse_groups_by_name():
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.sequence_generator import DiverseBeamSearch, TwoPhaseSequenceGenerator
    d = Dictionary.synthetic(96)
    with pytest.raises(NotImplementedError, match="DiverseBeamSearch"):
        TwoPhaseSequenceGenerator([_Model()], d, d, beam_size=4, search_strategy=DiverseBeamSearch(d, 2, 0.5))
