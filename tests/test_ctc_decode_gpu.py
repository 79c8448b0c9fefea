"""The CTC decoding kernels (csrc/ctc_decode.hip) and CTCDecoder on the GPU against the float64 rules of tests/ctc_decode_ref.py, which
are fed the very values the kernels read (f32, or rounded to bf16).

Greedy: tokens, counts and frames exact and equal to a collapse of K.ctc_argmax's predictions; tok_score and score within 1e-4
relative (the project's fp32 bound; the worst-case f32 summation error T * 2^-24 stays below it for T <= 1,500).
Prefix beam search: on cases whose closest keep / drop decision in float64 is at least MIN_GAP away, token strings and their order
exact and scores within 1e-4 relative; nearer cases are skipped by name and counted.  The kernel must side with the reference
against the wrong twin (identity by parent entry) wherever the two differ.
`python tests/test_ctc_decode_gpu.py OUT.json` writes the worst score errors of a run (tests/golden/ctc_decode_measured.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import ctc_decode_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
REL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "ctc_decode_measured.json")
WORST = {}                            # (what, dtype name) -> worst relative score error seen in this process


def note(what, name, err):
    WORST[(what, name)] = max(WORST.get((what, name), 0.0), float(err))


def device_rows(x, name, ld):
    """x f32 [T, B, V] (already rounded to the dtype) -> device view [T, B, V] of a buffer with row stride ld, padding poisoned"""
    T, B, V = x.shape
    buf = torch.full((T, B, ld), float("nan"), dtype=DT[name], device=DEV)
    buf[..., :V] = torch.from_numpy(x).to(DEV).to(DT[name])
    v = buf[..., :V]
    assert torch.equal(v.float().cpu(), torch.from_numpy(x)), "the reference must see the values the kernel reads"
    return v


def rel_err(got, ref):
    return abs(float(got) - ref) / abs(ref) if ref != 0 else abs(float(got))


# ------------------------------------------------------------------ greedy
def greedy_batch(T, V, name, seed):
    """six sentences: random full length; random with one frame; blank on every frame; one token on every frame; `a _ a a b`;
    a run that crosses in_len.  Frame 0 of sentence 0 holds an arg-max tie (the first index wins)."""
    rng = np.random.default_rng(seed)
    blank = V - 1
    a, b = 0, min(1, V - 2)                                           # V = 2: one non-blank symbol
    x = (rng.standard_normal((T, 6, V)) * 3).astype(np.float32)
    lens = [T, 1, T, T, T, max(T - 2, 1)]
    top = np.abs(x).max() + 4
    x[:, 2, blank] = top
    x[:, 3, a] = top
    pat = [a, blank, a, a, b]
    for t in range(T):
        x[t, 4, pat[t % 5]] = top
    if T >= 4:
        x[T - 4:, 5, b] = top                                         # frames T-4 .. T-1, of which in_len = T - 2 keeps two
    x = R.round_to(x, name)
    j1, j2 = (0, 1) if V == 2 else (int(rng.integers(0, V - 1)), V - 1)
    x[0, 0, j1] = x[0, 0, j2] = x[0, 0].max() + 1
    x = R.round_to(x, name)
    assert x[0, 0, j1] == x[0, 0, j2] == x[0, 0].max()
    return x, lens, blank, j1


@pytest.mark.parametrize("name", ["f32", "bf16"])
@pytest.mark.parametrize("V,ld", [(2, 5), (12, 16), (257, 264), (5001, 5008), (5001, 5003)])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_greedy_element_by_element(T, V, ld, name):
    from fbk_fairseq_st_amd import kernels as K
    x, lens, blank, tie = greedy_batch(T, V, name, seed=T * 7 + V)
    logits = device_rows(x, name, ld)
    in_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tokens, n, frames, tok_score, score = [t.cpu() for t in K.ctc_greedy(logits, in_len, blank)]
    pred = K.ctc_argmax(logits)[0].cpu()                               # [B, T]
    worst = 0.0
    for b in range(6):
        tk, fr, ts, sc = R.greedy(x[:, b], lens[b], blank)
        k = int(n[b])
        assert k == len(tk), (b, k, len(tk))
        assert tokens[b, :k].tolist() == tk and frames[b, :k].tolist() == [list(f) for f in fr], b
        runs = R.collapse(pred[b, :lens[b]].tolist(), blank)
        assert tokens[b, :k].tolist() == [r[0] for r in runs] and frames[b, :k].tolist() == [[r[1], r[2]] for r in runs], \
            "differs from a collapse of K.ctc_argmax's predictions"
        errs = [rel_err(tok_score[b, j], ts[j]) for j in range(k)] + [rel_err(score[b], sc)]
        worst = max(worst, max(errs))
        assert max(errs) <= REL, (b, max(errs))
    note("greedy", name, worst)
    print("greedy %s T=%d V=%d ld=%d: worst relative score error %.3g" % (name, T, V, ld, worst))
    # what the crafted sentences are there for
    assert int(n[2]) == 0 and int(n[3]) == 1 and frames[3, 0].tolist() == [0, T]
    assert int(pred[0, 0]) == tie and tokens[0, 0] == tie, "an arg-max tie goes to the first index"
    if T >= 5 and V > 2:
        assert tokens[4, :3].tolist() == [0, 0, 1] and frames[4, :3].tolist() == [[0, 1], [2, 4], [4, 5]], "`a _ a` is two tokens, `a a` one"
    if T >= 4:
        k = int(n[5])
        assert frames[5, k - 1].tolist()[1] == T - 2, "a run that crosses in_len ends at in_len"


def test_greedy_refuses_and_handles_empty():
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.lib import S2THipError
    x = torch.randn(4, 2, 12, device=DEV)
    with pytest.raises(S2THipError, match="invalid argument"):
        K.ctc_greedy(x, torch.tensor([4, 4], dtype=torch.int32, device=DEV), 12)
    with pytest.raises(ValueError):
        K.ctc_greedy(x, torch.tensor([4, 4], dtype=torch.int64, device=DEV), 11)
    out = K.ctc_greedy(x[:0], torch.zeros(2, dtype=torch.int32, device=DEV), 11)
    assert out[1].tolist() == [0, 0] and out[4].tolist() == [0.0, 0.0]
    tokens, n, frames, tok_score, score = K.ctc_greedy(x, torch.tensor([0, -3], dtype=torch.int32, device=DEV), 11)
    assert n.tolist() == [0, 0] and score.tolist() == [0.0, 0.0], "no frames: no tokens, score 0"


# ------------------------------------------------------------------ prefix beam search
def run_prefix(x, lens, blank, beam, cand, nbest, name, ld=None):
    """x f32 [T, B, V] rounded -> per sentence [(token tuple, score)]"""
    from fbk_fairseq_st_amd import kernels as K
    T, B, V = x.shape
    logits = device_rows(x, name, ld or V + 3)
    in_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    tokens, ln, scores, n_hyp = [t.cpu() for t in K.ctc_prefix_beam(logits, in_len, blank, beam, cand, nbest)]
    assert bool((ln[torch.arange(nbest)[None, :] >= n_hyp[:, None]] == 0).all())
    return [[(tuple(tokens[b, i, :int(ln[b, i])].tolist()), float(scores[b, i])) for i in range(int(n_hyp[b]))] for b in range(B)]


def assert_hyps(got, want, name, what):
    """token strings and order exact, scores within REL relative; returns the worst relative error"""
    assert [h[0] for h in got] == [h[0] for h in want], (what, got[:3], want[:3])
    worst = max([rel_err(g[1], w[1]) for g, w in zip(got, want)] + [0.0])
    assert worst <= REL, (what, worst)
    note("prefix", name, worst)
    return worst


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_prefix_random_cases(name):
    seeds = R.GPU_SEEDS if name == "f32" else R.GPU_SEEDS_BF16
    skipped, worst, twin_cases = [], 0.0, 0
    for seed in seeds:
        c, x, right, wrong = R.case_reference(seed, name)
        what = "seed%d-T%d-V%d-beam%d-cand%d" % (seed, c["T"], c["V"], c["beam"], c["cand"])
        if right["gap"] < R.MIN_GAP:
            skipped.append(what)
            continue
        got = run_prefix(x[:, None, :], [c["T"]], c["blank"], c["beam"], c["cand"], c["beam"], name)[0]
        worst = max(worst, assert_hyps(got, right["hyps"], name, what))
        if not R.same_hyps(right["hyps"], wrong["hyps"]):
            twin_cases += 1
            assert not R.same_hyps(got, wrong["hyps"], rel=REL), "%s: the kernel agrees with the wrong twin" % what
    print("prefix %s: %d cases, worst relative score error %.3g, %d where the twin differs; skipped for a float64 margin below %g: %s"
          % (name, len(seeds) - len(skipped), worst, twin_cases, R.MIN_GAP, ", ".join(skipped) or "none"))
    assert twin_cases >= 1
    if name == "f32":
        assert len(skipped) <= R.MAX_SKIPPED * len(seeds), skipped
    else:
        assert len(seeds) - len(skipped) >= R.MIN_KEPT_BF16, skipped


def big_case(name):
    """T = 375, V = 5001 as a trained head looks: every segment of 1 to 3 frames has one symbol (the blank in 6 of 10) 22 above
    randn x 3, 0.3 noise on top.  At this length totals of about -200 (the generator's recipe as it is) leave no seed with a float64
    margin of 1e-5 at every one of the 375 keep / drop decisions; seed 92 of this recipe has one in both roundings (9.5e-5, 2.1e-4).
    The second sentence of the batch has no frames."""
    rng = np.random.default_rng(92)
    T, V = 375, 5001
    rows = []
    while len(rows) < T:
        r = rng.standard_normal(V) * 3
        r[V - 1 if rng.random() < 0.6 else int(rng.integers(0, V - 1))] += 22
        rows += [r] * int(rng.integers(1, 4))
    x = (np.stack(rows[:T]) + 0.3 * rng.standard_normal((T, V))).astype(np.float32)
    return R.round_to(np.stack([x, np.zeros_like(x)], 1), name), [T, 0], V - 1


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_prefix_at_the_flagship_shape(name):
    x, lens, blank = big_case(name)
    got = run_prefix(x, lens, blank, 16, 16, 4, name, ld=5008)
    want = R.prefix_beam(x[:, 0], lens[0], blank, 16, 16, 4)
    assert want["gap"] >= R.MIN_GAP, "the case was chosen with a clear margin"
    worst = assert_hyps(got[0], want["hyps"], name, "flagship")
    print("prefix %s T=375 V=5001 beam=16 cand=16: best has %d tokens, worst relative score error %.3g" % (name, len(got[0][0][0]), worst))
    assert got[1] == [((), 0.0)]


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_prefix_candidate_boundary_tie_goes_to_the_lower_index(name):
    """columns 3 and 7 hold the same logit, second and third highest of every frame: with cand = 2 the candidates are {best, 3}"""
    rng = np.random.default_rng(0)
    T, V, blank = 9, 12, 11
    x = rng.standard_normal((T, 1, V)).astype(np.float32)
    for t in range(T):
        x[t, 0, [0, 5, 9][t % 3]] = 4.0 + rng.random()
        x[t, 0, 3] = x[t, 0, 7] = 2.0 + rng.random()
        x[t, 0, blank] = 1.0 + rng.random()
    x = R.round_to(x, name)
    assert all(r[3] == r[7] == sorted(r)[-2] == sorted(r)[-3] for r in x[:, 0])
    want = R.prefix_beam(x[:, 0], T, blank, 8, 2, 4)
    assert want["gap"] >= R.MIN_GAP and any(3 in h[0] for h in want["hyps"]) and not any(7 in h[0] for h in want["hyps"])
    got = run_prefix(x, [T], blank, 8, 2, 4, name)[0]
    assert_hyps(got, want["hyps"], name, "cand-tie")


@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_prefix_ragged_batch_few_prefixes_and_no_frames(name):
    """in_len 0: the empty hypothesis with score 0; in_len 1 with cand = 1: two prefixes exist, nbest = 3 writes two"""
    c, x1, _, _ = R.case_reference(7, name)
    T, V, blank = c["T"], c["V"], c["blank"]
    lens = [T, 0, min(17, T), 1]
    x = np.repeat(x1[:, None, :], 4, axis=1).copy()
    x[:, 2] = x1[::-1]
    got = run_prefix(x, lens, blank, 4, 1, 3, name, ld=V + 8)
    assert got[1] == [((), 0.0)]
    assert len(got[3]) == 2, "T = 1, one candidate: the empty prefix and the candidate"
    for b in (0, 2, 3):
        want = R.prefix_beam(x[:, b], lens[b], blank, 4, 1, 3)
        if want["gap"] >= R.MIN_GAP:
            assert_hyps(got[b], want["hyps"], name, "ragged-b%d" % b)
    one = R.prefix_beam(np.zeros((1, 2), np.float32), 1, 0, 2, 1, 2)["hyps"]           # T = 1, V = 2
    got = run_prefix(np.zeros((1, 1, 2), np.float32) + np.array([0.0, 0.5], np.float32), [1], 0, 2, 1, 2, name)[0]
    assert len(one) == len(got) == 2 and [h[0] for h in got] == [(1,), ()]


def test_prefix_refusals():
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.lib import S2THipError
    x = torch.randn(4, 2, 12, device=DEV)
    n = torch.tensor([4, 4], dtype=torch.int32, device=DEV)
    for beam, cand, nbest, msg in ((17, 4, 1, "not supported"), (4, 17, 1, "not supported"), (4, 12, 1, "not supported"),
                                   (4, 4, 5, "invalid argument")):
        with pytest.raises(S2THipError, match=msg):
            K.ctc_prefix_beam(x, n, 11, beam, cand, nbest)


# ------------------------------------------------------------------ end to end
_BUILT = {}


def tiny_model(name):
    """model_a (built with --ctc-compress-out) / model_c (without) of tests/helpers.py model_case, in f32, once"""
    if name not in _BUILT:
        import test_model_gpu as TM
        g, cfg, W, sample, meta, model, crit = TM.build(name, torch.float32)
        _BUILT[name] = (model, TM.to_dev(sample), meta, crit)
    return _BUILT[name]


def transcript_dict(meta):
    from fbk_fairseq_st_amd.data import Dictionary
    d = Dictionary.synthetic(meta["V_src"] - 5)
    d.add_symbol("<ctc_blank>")
    assert len(d) == meta["V_src"] and d.index("<ctc_blank>") == meta["blank"]
    return d


@pytest.mark.parametrize("strategy", ["greedy", "prefix"])
def test_end_to_end_on_a_ctc_compress_model(strategy):
    """generate == decode_logits on the encoder's own ctc_out and lengths, and both equal the float64 rule on those logits; the
    training flag is restored; a model built without the option is refused with a pointer to decode_logits"""
    from fbk_fairseq_st_amd.ctc_decoder import CTCDecoder
    model, sample, meta, _ = tiny_model("model_a")
    assert meta["compress"]
    dec = CTCDecoder(transcript_dict(meta), strategy=strategy, beam_size=4, cand=4, nbest=2 if strategy == "prefix" else 1)
    assert dec.blank == meta["blank"]
    for training in (True, False):
        model.train(training)
        hyps = dec.generate([model], sample)
        assert model.training is training
    model.eval()
    ni = sample["net_input"]
    with torch.no_grad():
        enc = model.encoder(src_tokens=ni["src_tokens"], src_lengths=ni["src_lengths"])
    T, B, V = enc.ctc_out.shape
    assert V == meta["V_src"]
    in_len = (~enc.ctc_padding_mask).sum(1) if enc.ctc_padding_mask is not None else torch.full((B,), T, device=DEV)
    again = dec.decode_logits(enc.ctc_out, in_len)
    assert len(hyps) == len(again) == B
    x = enc.ctc_out.float().cpu().numpy()
    for b in range(B):
        assert len(hyps[b]) == len(again[b]) >= 1
        for h, a in zip(hyps[b], again[b]):
            assert torch.equal(h["tokens"], a["tokens"]) and torch.equal(h["score"], a["score"])
            assert h["tokens"].dtype == torch.int64 and h["tokens"].is_cuda and dec.blank not in h["tokens"].tolist()
            assert h["score"].dtype == torch.float32 and h["score"].dim() == 0 and h["score"].is_cuda
        if strategy == "greedy":
            tk, fr, ts, sc = R.greedy(x[:, b], int(in_len[b]), dec.blank)
            assert hyps[b][0]["tokens"].tolist() == tk and hyps[b][0]["frames"].tolist() == [list(f) for f in fr]
            assert rel_err(hyps[b][0]["score"], sc) <= REL
        else:
            want = R.prefix_beam(x[:, b], int(in_len[b]), dec.blank, 4, 4, 2)
            if want["gap"] >= R.MIN_GAP:
                assert_hyps([(tuple(h["tokens"].tolist()), float(h["score"])) for h in hyps[b]], want["hyps"], "f32", "model_a-b%d" % b)
    plain, psample, pmeta, _ = tiny_model("model_c")
    assert not pmeta["compress"]
    plain.train()
    with pytest.raises(ValueError, match="decode_logits"):
        dec.generate([plain], psample)
    assert plain.training is True
    with pytest.raises(ValueError, match="exactly one model"):
        dec.generate([model, plain], sample)


def test_measured_file_records_both_dtypes_within_the_bound():
    """tests/golden/ctc_decode_measured.json: the worst score errors of a run of this file on an MI355X (written by running the file as
    a script); the README quotes it.  It sets no bound -- the bound is the issue's 1e-4 -- but it must lie within it."""
    with open(MEASURED) as f:
        m = json.load(f)
    for name in DT:
        assert m[name]["bound"] == REL and 0 < m[name]["greedy_worst"] <= REL and 0 < m[name]["prefix_worst"] <= REL


def measured():
    return {name: {"greedy_worst": WORST.get(("greedy", name)), "prefix_worst": WORST.get(("prefix", name)), "bound": REL} for name in DT}


if __name__ == "__main__":
    rc = pytest.main([os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"])
    out = sys.modules["test_ctc_decode_gpu"].measured()              # the module pytest imported holds the run's figures
    out["note"] = ("worst relative error of tok_score / score (greedy) and of the hypotheses' scores (prefix) against float64 over the "
                   "cases of tests/test_ctc_decode_gpu.py on an MI355X; the tests hold both to `bound`")
    if rc == 0 and len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))


