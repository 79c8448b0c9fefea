"""n-gram blocking and prefix tokens on the device-resident beam search (s2t_decode_step_rules: dec_row_kernel<VPT, true> of csrc/decode.hip).

Step by step, in the manner of test_decode_gpu.test_device_search_step_by_step: one s2t_decode_step_rules at a time over
test_decode_gpu.DecEngine; after every step every row's 2 beam candidates against the float64 restatement of the row kernel WITH the
two rules on the device's own f32 logits (decode_rules_ref.row_reference_rules: the history of a row is rebuilt from tok_hist /
par_hist, not from the ancestor table the kernel gathers through), within decode_ref.row_reference's bound -- the rules only write
-inf, so there is nothing more to allow for -- and the sentence bookkeeping bit for bit against decode_ref.sent_step.

Whole searches through SequenceGenerator on s2t_transformer_s: the device route is taken, agrees with the step-by-step route and
with oracle/s2t_ref.beam_search (fp32: tokens exact, scores 1e-4, the project's generation bound), and in both dtypes every
hypothesis starts with its sentence's forced tokens and contains no repeated n-gram.  The searches that must stay on the step route
(a prefix with EOS, n-gram size 1) do, without a session being built.  The two-phase generator takes the device route in both of
its searches with n-gram blocking.
"""

import numpy as np
import pytest
import torch

import decode_ref as R
import decode_rules_ref as RR
import test_decode_gpu as TG
from test_decode_gpu import BF, BOS, DEV, EOS, F32, PAD, UNK

pytestmark = pytest.mark.gpu

P3 = [[17, 45, 9], [33, PAD, PAD], [PAD, PAD, PAD]]          # width 3, rows of length 3, 1 and 0: the shape of the generate_ext fixture


def _session(c):
    from fbk_fairseq_st_amd import decode as DEC
    torch.manual_seed(c.get("seed", 0))
    eng = TG.DecEngine(c["D"], 2 * c["D"], 1, c["V"], c["dtype"], c.get("seed", 0), "relu", c.get("eos_scale", 1.0), 1.0, 0)
    B, beam = c["B"], c["beam"]
    enc = torch.randn(100, B, c["D"], device=DEV)
    prefix = torch.tensor(c["prefix"], dtype=torch.int64) if c.get("prefix") is not None else None
    ses = DEC.BeamDecodeSession(eng, "decoder.", enc, None, beam, c["max_len"], c["min_len"], PAD, UNK, EOS, c["V"],
                                no_repeat_ngram_size=c["n"], prefix_tokens=prefix)
    assert ses.ok, "the session refused a shape the case is meant to run"
    assert ses.rules_addr, "the session carries no rules"
    return eng, ses


def run_rules_search(c):
    """the whole search, one checked step at a time; returns what the rules did: (bans, forced rows, rows a ban left empty)"""
    from fbk_fairseq_st_amd import lib as L
    eng, ses = _session(c)
    dtype, B, beam, V, max_len, min_len, ngram = c["dtype"], c["B"], c["beam"], c["V"], c["max_len"], c["min_len"], c["n"]
    prefix = np.asarray(c["prefix"], dtype=np.int64) if c.get("prefix") is not None else None
    N, K2, M2 = B * beam, 2 * beam, max_len + 2
    lib, st = L.load(), L.stream()
    L.check(lib.s2t_decode_begin(ses.addr, BOS, st), "s2t_decode_begin")
    host = R.new_state(B, beam, max_len, BOS)
    bans = forced = emptied = 0
    for t in range(max_len + 1):
        what = "%s step %d" % (c["id"], t)
        L.check(lib.s2t_decode_step_rules(ses.addr, ses.rules_addr, st), "s2t_decode_step_rules")
        torch.cuda.synchronize()
        base = torch.from_numpy(host["cum_hist"][t].astype(np.float64)).to(DEV) if t > 0 else torch.zeros(N, dtype=torch.float64, device=DEV)
        plain, _ = R.row_reference(ses.bufs["logits"], t, beam, PAD, UNK, EOS, max_len, min_len, 1.0, 0.0, base, False)
        rv, rb = RR.row_reference_rules(ses.bufs["logits"], t, beam, PAD, UNK, EOS, max_len, min_len, 1.0, 0.0, base, False,
                                        host["tok_hist"], host["par_hist"], ngram, prefix)
        live = torch.isfinite(plain).any(1)
        bans += int((torch.isfinite(plain) & torch.isneginf(rv)).sum()) if prefix is None or t >= prefix.shape[1] else 0
        if prefix is not None and t < prefix.shape[1]:
            forced += sum(int(prefix[n // beam][t] != PAD) for n in range(N) if bool(live[n]))
            emptied += int((live & ~torch.isfinite(rv).any(1)).sum())
        cv, ci = ses.view_f("cand_val").view(N, K2), ses.view_i("cand_idx").view(N, K2)
        TG._note("rows", dtype, R.check_row_candidates(cv, ci, rv, rb, what + ": candidates"))
        R.sent_step(host, cv.cpu().numpy(), ci.cpu().numpy(), beam, V, EOS, max_len, False)
        for k in ("blacklist", "nfin", "finished", "steps"):
            v = TG._host(ses, k)
            assert np.array_equal(v, host[k]), "%s: %s %s != %s" % (what, k, v.tolist(), host[k].tolist())
        th, ph, ch = TG._host(ses, "tok_hist", (M2, N)), TG._host(ses, "par_hist", (M2, N)), TG._host(ses, "cum_hist", (M2, N))
        assert np.array_equal(th[:t + 2], host["tok_hist"][:t + 2]), what + ": tok_hist"
        assert np.array_equal(ph[1:t + 2], host["par_hist"][1:t + 2]), what + ": par_hist"
        assert np.array_equal(ch[1:t + 2].view(np.int32), host["cum_hist"][1:t + 2].view(np.int32)), what + ": cum_hist"
        na = t + 1 if t < max_len else t
        assert np.array_equal(TG._host(ses, "anc", (N, max_len + 1))[:, :na], host["anc"][:, :na]), what + ": anc"
        fs, fr, fsc = TG._host(ses, "fin_step", (B, beam)), TG._host(ses, "fin_row", (B, beam)), TG._host(ses, "fin_score", (B, beam))
        for s in range(B):
            k = int(host["nfin"][s])
            got = (fs[s, :k].tolist(), fr[s, :k].tolist(), fsc[s, :k].view(np.int32).tolist())
            assert got == (host["fin_step"][s, :k].tolist(), host["fin_row"][s, :k].tolist(),
                           host["fin_score"][s, :k].view(np.int32).tolist()), "%s: finalisation records of sentence %d" % (what, s)
    return bans, forced, emptied


def C(id_, dtype, B, beam, V, n, prefix, max_len, min_len, **kw):
    c = dict(id=id_, dtype=dtype, D=256, B=B, beam=beam, V=V, n=n, prefix=prefix, max_len=max_len, min_len=min_len)
    c.update(kw)
    return pytest.param(c, id=id_)


CASES = [
    C("f32-b4-V200-n2", F32, 3, 4, 200, 2, None, 24, 8),                                      # base case
    C("f32-b4-V200-n3-prefix3", F32, 3, 4, 200, 3, P3, 24, 8),                                # the `elif` on min_len; ban after force
    C("bf16-b5-V5000-n2", BF, 2, 5, 5000, 2, None, 24, 8),                                    # bitmap beyond one word per thread
    C("f32-b2-V64-n2-hist300", F32, 2, 2, 64, 2, None, 300, 300),                             # histories past 64 and 256 entries
    C("f32-b2-V9000-n2", F32, 2, 2, 9000, 2, None, 24, 24),                                  # more than 256 words of ban bitmap
    C("f32-b16-V200-n2-prefix2", F32, 2, 16, 200, 2, [[17, 45], [33, PAD]], 12, 8),           # 16-row tiles
    # a ban that empties a forced row (step 2: the forced 17 would repeat the bigram 17 17): rows full of -inf from there on
    C("f32-b4-V200-n2-forced_repeat", F32, 3, 4, 200, 2, [[17, 17, 17], [33, PAD, PAD], [PAD, PAD, PAD]], 8, 4),
]


@pytest.mark.parametrize("c", CASES)
def test_rules_step_by_step(c):
    bans, forced, emptied = run_rules_search(c)
    print("%s: %d open columns banned, %d live rows forced, %d forced rows emptied" % (c["id"], bans, forced, emptied))
    if not c["id"].endswith("forced_repeat"):
        assert bans > 0, "no step of the case banned a column that was open"
    if c["prefix"] is not None:
        assert forced > 0, "no live row was forced"
    if c["id"].endswith("forced_repeat"):
        assert emptied > 0, "the ban did not reach the forced row"


# ------------------------------------------------------------------ whole searches
LENGTHS = [400, 250, 90]
OPTS = dict(beam_size=5, max_len_a=0.0, max_len_b=14, min_len=8, len_penalty=1.0, unk_penalty=0.0, temperature=1.0)
_CACHE = {}


def _model(dtype):
    """s2t_transformer_s as test_configs_gpu builds it, once per dtype"""
    import test_configs_gpu as TC
    if dtype not in _CACHE:
        a, task, model, crit, cfg, W = TC.build("s2t_transformer_s", dtype, criterion="label_smoothed_cross_entropy")
        sample = TC.batch(task, len(LENGTHS), max(LENGTHS), 8, 8, 9, lengths=LENGTHS)
        model.eval()
        _CACHE[dtype] = (task, model, cfg, W, sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
    return _CACHE[dtype]


def _oracle(W, cfg, src, lens, prefix):
    """oracle.s2t_ref.beam_search with the case's options (pinned to the reference by tests/test_oracle_golden.py), once per case"""
    from oracle import s2t_ref
    key = ("oracle", prefix is not None)
    if key not in _CACHE:
        _CACHE[key] = s2t_ref.beam_search(W, cfg, src, lens, 5, 0.0, 14, 8, 1.0, 0.0, 1.0, prefix_tokens=prefix, no_repeat_ngram_size=2)
    return _CACHE[key]


def _repeats(tokens, n):
    g = [EOS] + list(tokens)                                   # <bos> = EOS heads the history
    grams = [tuple(g[i:i + n]) for i in range(len(g) - n + 1)]
    return len(grams) != len(set(grams))


def _starts_with(tokens, row):
    forced = [int(v) for v in row if int(v) != PAD]
    return list(tokens[:len(forced)]) == forced


@pytest.mark.parametrize("with_prefix", [False, True], ids=["ngram2", "ngram2-prefix3"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_device_search_with_rules_equals_step_search(dtype, with_prefix, monkeypatch):
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    import test_configs_gpu as TC
    task, model, cfg, W, src, lens = _model(dtype)
    net = dict(net_input=dict(src_tokens=src.to(DEV), src_lengths=lens.to(DEV)))
    prefix = torch.tensor(P3, dtype=torch.int64) if with_prefix else None
    pdev = None if prefix is None else prefix.to(DEV)
    if with_prefix:
        forced = prefix[prefix != PAD]
        assert not bool((forced == EOS).any()) and forced.numel() == 4
    # what the rules are there to change: without them a best hypothesis repeats a bigram / does not start with the forced tokens
    free = SequenceGenerator([model], task.target_dictionary, **OPTS)
    free_h = free.generate([model], net)
    assert "launches_per_step" in free.last_stats
    assert any(_repeats(hs[0]["tokens"].tolist(), 2) for hs in free_h), "no best hypothesis repeats a bigram with blocking off"
    assert any(not _starts_with(hs[0]["tokens"].tolist(), P3[b]) for b, hs in enumerate(free_h)), "the prefix forces nothing"

    gen = SequenceGenerator([model], task.target_dictionary, no_repeat_ngram_size=2, **OPTS)
    dev_h = gen.generate([model], net, prefix_tokens=pdev)
    assert "launches_per_step" in gen.last_stats, "the device route was not taken"
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen2 = SequenceGenerator([model], task.target_dictionary, no_repeat_ngram_size=2, **OPTS)
    step_h = gen2.generate([model], net, prefix_tokens=pdev)
    assert "launches_per_step" not in gen2.last_stats, "the step route was not taken"
    assert len(dev_h) == len(step_h) == len(LENGTHS)
    for b, (hs, ss) in enumerate(zip(dev_h, step_h)):
        assert len(hs) == len(ss) == 5
        for h in hs:
            toks = h["tokens"].tolist()
            assert not _repeats(toks, 2), "sentence %d: a repeated bigram in %s" % (b, toks)
            if with_prefix:
                assert _starts_with(toks, P3[b]), "sentence %d: %s does not start with its forced tokens" % (b, toks)
        if dtype == F32:
            for h, s_ in zip(hs, ss):
                assert h["tokens"].tolist() == s_["tokens"].tolist()
                assert abs(float(h["score"]) - float(s_["score"])) < 1e-4
                np.testing.assert_allclose(h["positional_scores"].cpu().numpy(), s_["positional_scores"].cpu().numpy(), atol=1e-4)
        else:
            sc = [float(h["score"]) for h in hs]
            assert sc == sorted(sc, reverse=True)
            for h in hs:
                assert int(h["tokens"][-1]) == EOS and not bool((h["tokens"][:-1] == EOS).any())
            assert abs(sc[0] - float(ss[0]["score"])) < TC.BF16_GEN_ATOL
    if dtype == F32:
        orc = _oracle(W, cfg, src, lens, prefix)
        for hs, os_ in zip(dev_h, orc):
            assert len(hs) == len(os_) == 5
            for h, (ot, osc, ops) in zip(hs, os_):
                assert h["tokens"].tolist() == ot.tolist()
                assert abs(float(h["score"]) - osc) < 1e-4
                np.testing.assert_allclose(h["positional_scores"].cpu().numpy(), ops, atol=1e-4)


@pytest.mark.parametrize("what", ["prefix_with_eos", "ngram1"])
def test_searches_the_device_route_leaves_to_the_step_route(what, monkeypatch):
    """a prefix that holds EOS and n-gram size 1 take the step route, and no session is asked to run them.  With n = 1 the reference bans
    EOS through the <bos> column, so that search runs to the length limit and ends in the step route's `assert step < max_len`
    (sequence_generator.py:417 of the reference): every one of its steps ran there."""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    task, model, cfg, W, src, lens = _model(F32)
    net = dict(net_input=dict(src_tokens=src.to(DEV), src_lengths=lens.to(DEV)))

    def no_session(*a, **k):
        raise RuntimeError("a BeamDecodeSession was built for a search the device route does not handle")
    monkeypatch.setattr(DEC, "BeamDecodeSession", no_session)
    opts = dict(OPTS, max_len_b=6, min_len=1)
    if what == "ngram1":
        gen = SequenceGenerator([model], task.target_dictionary, no_repeat_ngram_size=1, **opts)
        with pytest.raises(AssertionError):
            gen.generate([model], net)
        assert gen.last_stats == {"steps": opts["max_len_b"] + 1}
        return
    else:
        gen = SequenceGenerator([model], task.target_dictionary, **opts)
        hyps = gen.generate([model], net, prefix_tokens=torch.tensor([[17, EOS], [33, PAD], [PAD, PAD]], device=DEV))
        assert hyps[0][0]["tokens"].tolist() == [17, EOS] and hyps[1][0]["tokens"].tolist()[0] == 33
    assert "launches_per_step" not in gen.last_stats and len(hyps) == len(LENGTHS)


def test_two_phase_generator_with_ngram_blocking_on_the_device_route(monkeypatch):
    """TwoPhaseSequenceGenerator on the twophase_wide configuration (64-wide heads, D 256) with no_repeat_ngram_size = 2: both of its
    searches run device-resident (the second with init scores), and give the step route's hypotheses"""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd.sequence_generator import TwoPhaseSequenceGenerator
    from test_model_gpu import _build_twophase
    task, args, model, src, lens, opts, exp, _ = _build_twophase("c")
    net = dict(net_input=dict(src_tokens=src, src_lengths=lens))
    opts = dict(opts, max_len_b=12, min_len=6, no_repeat_ngram_size=2)
    sessions = []
    real = DEC.BeamDecodeSession

    def counting(*a, **k):
        ses = real(*a, **k)
        sessions.append((ses.ok, bool(ses.rules_addr), k.get("init_scores") is not None))
        return ses
    monkeypatch.setattr(DEC, "BeamDecodeSession", counting)
    gen = TwoPhaseSequenceGenerator([model], task.source_dictionary, task.target_dictionary, **opts)
    dev_h = gen.generate([model], net)
    assert sessions == [(True, True, False), (True, True, True)], "both searches on the device route, with rules: %s" % sessions
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen2 = TwoPhaseSequenceGenerator([model], task.source_dictionary, task.target_dictionary, **opts)
    step_h = gen2.generate([model], net)
    assert len(sessions) == 2
    for hs, ss in zip(dev_h, step_h):
        assert len(hs) == len(ss) > 0
        for h, s_ in zip(hs, ss):
            assert h["tokens"].tolist() == s_["tokens"].tolist() and h["aux_tokens"].tolist() == s_["aux_tokens"].tolist()
            assert abs(float(h["score"]) - float(s_["score"])) < 1e-4
            assert not _repeats(h["tokens"].tolist(), 2) and not _repeats(h["aux_tokens"].tolist(), 2)
