"""The forced-alignment kernels (csrc/ctc_align.hip) and CTCAligner on the GPU against the float64 rule of tests/ctc_align_ref.py, which
is fed the very values the kernels read (f32, or rounded to bf16).

Every sentence of every case, none skipped: `states` is a valid path for the transcript, `frames` are exactly those of the returned
states, `score` and `tok_score` agree with float64 sums along the returned path within 1e-4 * max(1, |x|), and the float64 score of
the returned path is within 1e-4 * max(1, |optimum|) of the float64 optimum (1e-4: the project's contract bound).  Planted cases
(N(0, 1) logits with a bonus along a drawn path, R.planted_case) must have a float64 margin of at least 1e-4 at the closest decision on
their best path -- asserted, never skipped -- and then `states` must equal the reference path.  Outputs are filled with sentinels first:
what the rule calls "not written" must still hold them.  Targets are padded with out-of-range junk, rows with 1e30.
`python tests/test_ctc_align_gpu.py OUT.json` writes the worst errors of a run (tests/golden/ctc_align_measured.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import ctc_align_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAMES = ["f32", "bf16"]
REL = 1e-4
MIN_MARGIN = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "ctc_align_measured.json")
WORST = {}                            # (what, dtype name) -> worst relative error seen in this process
JUNK = (10 ** 12, -5, 2 ** 31)        # what pads the targets beyond tgt_len
S_INT, S_STATE = -7, -9               # sentinels of frames / status and of states


def note(what, name, err):
    WORST[(what, name)] = max(WORST.get((what, name), 0.0), float(err))


def err_of(got, ref):
    return abs(float(got) - ref) / max(1.0, abs(ref))


def device_rows(x, name, ld, unaligned=False):
    """x f32 [T, B, V] (already rounded to the dtype) -> device view [T, B, V] of a buffer with row stride ld, the padding filled with
    1e30; unaligned: the view starts one element into the allocation"""
    T, B, V = x.shape
    flat = torch.full((T * B * ld + 1,), 1e30, dtype=DT[name], device=DEV)
    buf = flat[1:] if unaligned else flat[:-1]
    buf = buf.view(T, B, ld)
    buf[..., :V] = torch.from_numpy(x).to(DEV).to(DT[name])
    v = buf[..., :V]
    assert torch.equal(v.float().cpu(), torch.from_numpy(x)), "the reference must see the values the kernel reads"
    assert (v.data_ptr() % 16 != 0) == unaligned or T * B == 0
    return v


def call_align(logits, in_len, targets, tgt_len, blank):
    """s2t_ctc_align on sentinel-filled outputs (kernels.ctc_align allocates its own: test_kernels_entry covers it)"""
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd import lib as L
    T, B, V = logits.shape
    Lmax = targets.shape[1]
    assert Lmax >= 1 and T * B > 0
    states = torch.full((B, T), S_STATE, dtype=torch.int32, device=DEV)
    frames = torch.full((B, Lmax, 2), S_INT, dtype=torch.int32, device=DEV)
    tok_score = torch.full((B, Lmax), float("nan"), dtype=torch.float32, device=DEV)
    score = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    status = torch.full((B,), S_INT, dtype=torch.int32, device=DEV)
    lib = L.load()
    ws = torch.empty((int(lib.s2t_ctc_align_workspace(T, B, Lmax)),), dtype=torch.uint8, device=DEV)
    L.check(lib.s2t_ctc_align(L.dt(logits), L.ptr(logits), L.ptr(in_len), L.ptr(targets), L.ptr(tgt_len), L.ptr(ws), L.ptr(states),
                              L.ptr(frames), L.ptr(tok_score), L.ptr(score), L.ptr(status), T, B, V, K._row_ld(logits), Lmax, int(blank),
                              L.stream()), "s2t_ctc_align")
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (states, frames, tok_score, score, status)]


def run(sents, name, blank, Lmax=None, ld=None, unaligned=False, T=None):
    """sents: dicts with x [n_b, V] (rounded), y, and optionally n (frames used, default all of x) and tgt_len (default len(y)).
    Shorter sentences are padded to T frames with N(0, 1) rows.  Returns (outputs, x [T, B, V], in_len)."""
    V = sents[0]["x"].shape[1]
    T = T or max(s["x"].shape[0] for s in sents)
    Lmax = Lmax or max(1, max(len(s["y"]) for s in sents))
    rng = np.random.default_rng(5)
    x = R.round_to(rng.standard_normal((T, len(sents), V)).astype(np.float32), name)
    targets = np.empty((len(sents), Lmax), np.int64)
    for b, s in enumerate(sents):
        x[:s["x"].shape[0], b] = s["x"]
        targets[b] = [JUNK[(b + i) % 3] for i in range(Lmax)]
        targets[b, :len(s["y"])] = s["y"]
    in_len = [s.get("n", s["x"].shape[0]) for s in sents]
    tgt_len = [s.get("tgt_len", len(s["y"])) for s in sents]
    out = call_align(device_rows(x, name, ld or V + 3, unaligned), torch.tensor(in_len, dtype=torch.int32, device=DEV),
                     torch.from_numpy(targets).to(DEV), torch.tensor(tgt_len, dtype=torch.int64, device=DEV), blank)
    return out, x, in_len


@functools.lru_cache(maxsize=None)
def reference(key):
    """the float64 rule for a registered sentence, computed once per process"""
    x, n, y, blank = _REGISTRY[key]
    return R.align(x, n, y, blank)


_REGISTRY = {}


def ref_of(x, n, y, blank):
    key = (x.shape, n, tuple(y), blank, hash(x[:n].tobytes()))
    _REGISTRY[key] = (x, n, list(y), blank)
    return reference(key)


def check_aligned(out, b, x, n, y, blank, name, exact, what):
    """checks (a) of the module docstring for sentence b, and with `exact` the equality with the reference path"""
    states, frames, tok_score, score, status = out
    T, L, Lmax = states.shape[1], len(y), frames.shape[1]
    n = min(max(n, 0), T)
    assert status[b] == 0, (what, b, status[b])
    st = states[b, :n]
    assert R.is_valid_path(st, y, n), (what, b, st[:20])
    assert (states[b, n:] == -1).all(), (what, b)
    ref = ref_of(x[:, b], n, y, blank)
    assert ref["status"] == 0
    s64, f64, t64 = R.path_sums(ref["lp"], st.astype(np.int64), y, blank)
    assert frames[b, :L].tolist() == f64.tolist(), (what, b, "frames are not those of the returned states")
    assert (frames[b, L:] == S_INT).all() and np.isnan(tok_score[b, L:]).all(), (what, b, "entries behind the transcript were written")
    e_sum = max([err_of(score[b], s64)] + [err_of(tok_score[b, i], t64[i]) for i in range(L)])
    e_opt = abs(s64 - ref["score"]) / max(1.0, abs(ref["score"]))
    print("%s b=%d %s n=%d L=%d: sums %.3g, path against the optimum %.3g, margin %.3g" % (what, b, name, n, L, e_sum, e_opt, ref["margin"]))
    assert e_sum <= REL and e_opt <= REL, (what, b, e_sum, e_opt)
    note("sums", name, e_sum)
    note("optimum", name, e_opt)
    if exact:
        assert ref["margin"] >= MIN_MARGIN, (what, b, ref["margin"], "raise the bonus of this shape")
        assert st.tolist() == ref["states"].tolist(), (what, b, "not the reference path")


def check_failed(out, b, code, L, what):
    """status 1 / 2: states -1 throughout, score -inf, (-1, -1) / -inf for the first L tokens (L None: nothing written)"""
    states, frames, tok_score, score, status = out
    assert status[b] == code and (states[b] == -1).all() and score[b] == -np.inf, (what, b, status[b], score[b])
    k = 0 if L is None else L
    assert (frames[b, :k] == -1).all() and np.isneginf(tok_score[b, :k]).all(), (what, b)
    assert (frames[b, k:] == S_INT).all() and np.isnan(tok_score[b, k:]).all(), (what, b, "entries behind the transcript were written")


def check_empty(out, b, what):
    """no frames, no tokens: score 0, status 0"""
    states, frames, tok_score, score, status = out
    assert status[b] == 0 and score[b] == 0.0 and (states[b] == -1).all(), (what, b)
    assert (frames[b] == S_INT).all() and np.isnan(tok_score[b]).all(), (what, b)


def planted(seed, T, V, L, name, **kw):
    c = R.planted_case(seed, T, V, L, name, **kw)
    return dict(x=c["x"], y=c["y"], path=c["path"])


def unique_path_sentence(seed, V, L, name):
    """a transcript on exactly L + repeats frames: one path exists"""
    y = R.draw_transcript(np.random.default_rng(seed), L, V, V - 1)
    return planted(seed, R.min_frames(y), V, L, name)


# ------------------------------------------------------------------ (b) transcript lengths around every switch
# form A takes 1, 2, 4, 8, 16 states per lane up to L = 31, 63, 127, 255, 511; form B from 512
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("L", [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 511, 512, 513, 1024])
def test_planted_paths_around_every_width(L, name):
    """four sentences with ragged in_len: the full width; half of it on fewer frames; the full width on exactly L + repeats frames
    (one path); no frames and no tokens"""
    V = 40
    T = 2 * L + 9
    a = planted(1000 + L, T, V, L, name)
    b = planted(2000 + L, T - 5, V, L // 2, name)
    c = unique_path_sentence(3000 + L, V, L, name) if L else planted(3000, 3, V, 0, name)
    d = dict(x=a["x"], y=[], n=0)
    out, x, in_len = run([a, b, c, d], name, V - 1, Lmax=max(L, 1), T=T)
    for i, s in enumerate((a, b, c)):
        check_aligned(out, i, x, in_len[i], s["y"], V - 1, name, True, "L%d" % L)
    assert out[0][2, :in_len[2]].tolist() == c["path"].tolist(), "on L + repeats frames the planted path is the only one"
    check_empty(out, 3, "L%d" % L)


@pytest.mark.parametrize("name", NAMES)
def test_planted_path_at_the_limit(name):
    """Lmax = 4,095 on T = 4,200 frames: tokens repeat with probability 0.01 here (at 0.2 the transcript would need 4,900 frames)"""
    L, T, V = 4095, 4200, 20
    a = planted(7, T, V, L, name, p_repeat=0.01)
    out, x, in_len = run([a], name, V - 1)
    check_aligned(out, 0, x, T, a["y"], V - 1, name, True, "limit")


# ------------------------------------------------------------------ (b) frame counts around the backward walk's blocks
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_planted_paths_around_the_walk_block(T, name):
    V = 12
    sents = [planted(10 + T, T, V, min(5, T), name), planted(20 + T, T, V, 0, name), planted(30 + T, T, V, min(20, T // 3), name)]
    out, x, in_len = run(sents, name, V - 1)
    for i, s in enumerate(sents):
        check_aligned(out, i, x, T, s["y"], V - 1, name, True, "T%d" % T)


@pytest.mark.parametrize("name", NAMES)
def test_planted_paths_around_the_staged_half_block_of_the_workgroup_form(name):
    """a padded width of 513 takes the workgroup form, which stages 32 frames of back-pointers at a time inside the 64-frame block"""
    V = 12
    lens = [1, 31, 32, 33, 63, 64, 65, 97]
    sents = [planted(40 + n, n, V, min(6, n), name) for n in lens]
    out, x, in_len = run(sents, name, V - 1, Lmax=513)
    for i, s in enumerate(sents):
        check_aligned(out, i, x, lens[i], s["y"], V - 1, name, True, "halfblock-n%d" % lens[i])


# ------------------------------------------------------------------ (b) vocabularies
@pytest.mark.parametrize("name", NAMES)
def test_two_symbol_vocabulary(name):
    """V = 2 with the blank at 0: every token repeats, so every blank between tokens is forced"""
    sents = [planted(50, 25, 2, 10, name, blank=0), planted(51, 19, 2, 10, name, blank=0), planted(52, 25, 2, 1, name, blank=0)]
    assert sents[1]["path"].tolist() == list(range(1, 20))
    out, x, in_len = run(sents, name, 0)
    for i, s in enumerate(sents):
        check_aligned(out, i, x, in_len[i], s["y"], 0, name, True, "V2")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ld,unaligned", [(5008, False), (5003, True)])
def test_flagship_vocabulary_padded_rows_unaligned_base(ld, unaligned, name):
    V = 5001
    sents = [planted(60, 130, V, 60, name), planted(61, 100, V, 33, name)]
    out, x, in_len = run(sents, name, V - 1, ld=ld, unaligned=unaligned)
    for i, s in enumerate(sents):
        check_aligned(out, i, x, in_len[i], s["y"], V - 1, name, True, "V5001-ld%d" % ld)


# ------------------------------------------------------------------ (c) status, beside ordinary sentences
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Lmax", [12, 600])
def test_status_beside_ordinary_sentences(Lmax, name):
    """sentences 0, 3 and 7 are ordinary; their results must be bit-for-bit those of a batch in which the others are ordinary too"""
    V, T, blank = 30, 40, 29
    ok = [planted(70 + i, T, V, 9, name) for i in range(8)]
    few = dict(ok[1], n=R.min_frames(ok[1]["y"]) - 1)                                  # one frame short: no path
    xz = ok[2]["x"].copy()
    xz[:, ok[2]["y"][4]] = -np.inf                                                     # a needed column is -inf on every frame
    dead = dict(ok[2], x=xz)
    yb = list(ok[4]["y"])
    yb[3] = blank
    yo = list(ok[5]["y"])
    yo[8] = V
    yn = list(ok[6]["y"])
    yn[0] = -1
    bad = [ok[0], few, dead, ok[3], dict(ok[4], y=yb), dict(ok[5], y=yo), dict(ok[6], y=yn), ok[7],
           dict(ok[0], tgt_len=Lmax + 1), dict(ok[0], tgt_len=-1), dict(ok[0], n=0)]
    out, x, in_len = run(bad, name, blank, Lmax=Lmax)
    plain, _, _ = run(ok + [ok[0]] * 3, name, blank, Lmax=Lmax)
    for b in (0, 3, 7):
        check_aligned(out, b, x, T, ok[b]["y"], blank, name, True, "status-Lmax%d" % Lmax)
        for got, want in zip(out, plain):
            assert got[b].tobytes() == want[b].tobytes(), (b, "an ordinary sentence changed beside refused ones")
    for b, code, L in ((1, 1, 9), (2, 1, 9), (4, 2, 9), (5, 2, 9), (6, 2, 9), (8, 2, None), (9, 2, None), (10, 1, 9)):
        check_failed(out, b, code, L, "status-Lmax%d" % Lmax)
    assert ref_of(x[:, 1], in_len[1], few["y"], blank)["status"] == 1 and ref_of(x[:, 2], T, dead["y"], blank)["status"] == 1


# ------------------------------------------------------------------ (d) batch independence
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("L,others", [(20, 20), (20, 100), (100, 700), (600, 600)])
def test_a_sentence_alone_and_inside_a_batch_gives_identical_bits(L, others, name):
    """member 3 of a batch of 5 with other lengths and frame counts; `others` also moves the batch to a wider form of the sentence
    phase (more states per lane, or the workgroup form): the sums are taken in one order in all of them"""
    V, T = 25, 2 * max(L, others) + 30
    s = planted(80, T - 11, V, L, name)
    rest = [planted(81 + i, T - 3 * i, V, max(others - 7 * i, 1), name) for i in range(4)]
    alone, x1, _ = run([s], name, V - 1, T=T)
    batch, x5, in_len = run(rest[:3] + [s] + rest[3:], name, V - 1, T=T)
    check_aligned(batch, 3, x5, T - 11, s["y"], V - 1, name, True, "batch")
    assert alone[0][0].tobytes() == batch[0][3].tobytes()
    assert alone[1][0, :L].tobytes() == batch[1][3, :L].tobytes() and alone[2][0, :L].tobytes() == batch[2][3, :L].tobytes()
    assert alone[3][0].tobytes() == batch[3][3].tobytes() and alone[4][0] == batch[4][3] == 0


# ------------------------------------------------------------------ (e) against the greedy decoder
@pytest.mark.parametrize("name", NAMES)
def test_aligning_the_greedy_transcript_gives_the_greedy_path(name):
    """the best unconstrained path is the best path of its own transcript: frames exact and scores within 1e-4 on f32 inputs; with
    bf16-rounded inputs exact logit ties can make the two tie rules disagree, so scores only"""
    from fbk_fairseq_st_amd import kernels as K
    V, T, blank = 300, 130, 299
    sents = [planted(90, 130, V, 40, name), planted(91, 111, V, 25, name), planted(92, 64, V, 30, name)]
    x = np.stack([np.concatenate([s["x"], R.round_to(np.random.default_rng(9).standard_normal((T - len(s["x"]), V)), name)]) for s in sents], 1)
    logits = device_rows(x, name, V + 4)
    in_len = torch.tensor([130, 111, 64], dtype=torch.int32, device=DEV)
    tokens, n, frames, tok_score, score = K.ctc_greedy(logits, in_len, blank)
    counts = n.tolist()
    Lmax = max(counts)
    assert min(counts) >= 20
    targets = tokens[:, :Lmax].long()
    st, fr, ts, sc, status = K.ctc_align(logits, in_len, targets, n.long(), blank)
    assert status.tolist() == [0, 0, 0]
    for b, k in enumerate(counts):
        assert err_of(sc[b], float(score[b])) <= REL
        if name == "f32":
            assert fr[b, :k].tolist() == frames[b, :k].tolist(), b
            assert max(err_of(ts[b, i], float(tok_score[b, i])) for i in range(k)) <= REL
            assert R.is_valid_path(st[b, :int(in_len[b])].cpu().numpy(), targets[b, :k].tolist(), int(in_len[b]))


# ------------------------------------------------------------------ (f) against the wrong twins
@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_contradicts_both_wrong_twins(name):
    blank = R.TWIN_BLANK
    for make, twin in ((R.twin_case_equal_tokens, dict(skip_equal=True)), (R.twin_case_ends_in_a_token, dict(end_last_only=True))):
        x, y = make()
        x = R.round_to(x, name)
        n = x.shape[0]
        out, xb, _ = run([dict(x=x, y=y)], name, blank)
        right, wrong = R.align(x, n, y, blank), R.align(x, n, y, blank, **twin)
        assert right["states"].tolist() != wrong["states"].tolist()
        check_aligned(out, 0, xb, n, y, blank, name, True, "twin")
        assert out[0][0, :n].tolist() == right["states"].tolist() != wrong["states"].tolist()


# ------------------------------------------------------------------ kernels.ctc_align, and (g) end to end
def test_kernels_entry_allocates_refuses_and_handles_empty():
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.lib import S2THipError
    s = planted(95, 30, 12, 6, "f32")
    x = torch.from_numpy(s["x"][:, None, :]).to(DEV)
    n, y, ln = torch.tensor([30], dtype=torch.int32, device=DEV), torch.tensor([s["y"]], device=DEV), torch.tensor([6], device=DEV)
    st, fr, ts, sc, status = K.ctc_align(x, n, y, ln, 11)
    assert status.tolist() == [0] and st[0].tolist() == ref_of(s["x"], 30, s["y"], 11)["states"].tolist()
    with pytest.raises(S2THipError, match="invalid argument"):
        K.ctc_align(x, n, y, ln, 12)
    st, fr, ts, sc, status = K.ctc_align(x, n, y[:, :0], torch.tensor([0], device=DEV), 11)      # a padded width of 0
    assert status.tolist() == [0] and st[0].tolist() == [0] * 30 and tuple(fr.shape) == (1, 0, 2)
    assert err_of(sc[0], float(R.log_softmax64(s["x"])[:, 11].sum())) <= REL
    st, fr, ts, sc, status = K.ctc_align(x, torch.tensor([0], dtype=torch.int32, device=DEV), y, ln, 11)
    assert status.tolist() == [1] and sc.tolist() == [float("-inf")] and st[0].tolist() == [-1] * 30


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


def test_end_to_end_on_a_ctc_compress_model():
    """generate == align_logits on the encoder's own ctc_out and lengths, and both follow the float64 rule on those logits; the
    training flag is restored; a model built without the option is refused with a pointer to align_logits"""
    from fbk_fairseq_st_amd.ctc_aligner import CTCAligner
    model, sample, meta, _ = tiny_model("model_a")
    assert meta["compress"]
    al = CTCAligner(transcript_dict(meta))
    assert al.blank == meta["blank"]
    for training in (True, False):
        model.train(training)
        hyps = al.generate([model], sample)
        assert model.training is training
    model.eval()
    ni = sample["net_input"]
    with torch.no_grad():
        enc = model.encoder(src_tokens=ni["src_tokens"], src_lengths=ni["src_lengths"])
    T, B, V = enc.ctc_out.shape
    in_len = (~enc.ctc_padding_mask).sum(1) if enc.ctc_padding_mask is not None else torch.full((B,), T, device=DEV)
    # the sample's transcripts, shortened where the utterance has too few frames for them so that paths exist
    tr, tr_len = sample["transcript_target"], sample["transcript_target_lengths"]
    short = torch.minimum(tr_len, (in_len.to(tr_len.device) // 2).to(tr_len.dtype))
    x = enc.ctc_out.float().cpu().numpy()
    aligned = 0
    for lens, got in ((tr_len, hyps), (short, al.align_logits(enc.ctc_out, in_len, tr, short))):
        again = al.align_logits(enc.ctc_out, in_len, tr, lens)
        assert len(got) == len(again) == B
        for b in range(B):
            h, a = got[b][0], again[b][0]
            assert len(got[b]) == 1 and h["status"] == a["status"]
            for k in ("tokens", "score", "positional_scores", "frames", "states"):
                assert torch.equal(h[k], a[k]), (b, k)
            y, n = tr[b, :int(lens[b])].tolist(), int(in_len[b])
            assert h["tokens"].tolist() == y and h["tokens"].is_cuda and h["score"].is_cuda and h["score"].dim() == 0
            r = R.align(x[:, b], n, y, al.blank) if not any(c == al.blank for c in y) else dict(status=2)
            assert h["status"] == r["status"], (b, h["status"], r["status"])
            if r["status"] == 0:
                aligned += 1
                st = h["states"].cpu().numpy().astype(np.int64)
                assert R.is_valid_path(st, y, n)
                s64, f64, t64 = R.path_sums(r["lp"], st, y, al.blank)
                assert h["frames"].tolist() == f64.tolist() and err_of(h["score"], s64) <= REL
                assert abs(s64 - r["score"]) <= REL * max(1.0, abs(r["score"]))
    assert aligned >= B, "the shortened transcripts were to have paths"
    plain, psample, pmeta, _ = tiny_model("model_c")
    assert not pmeta["compress"]
    plain.train()
    with pytest.raises(ValueError, match="align_logits"):
        al.generate([plain], psample)
    assert plain.training is True
    with pytest.raises(ValueError, match="exactly one model"):
        al.generate([model, plain], sample)


def test_measured_file_records_both_dtypes_within_the_bound():
    """tests/golden/ctc_align_measured.json: the worst errors of a run of this file on an MI355X (written by running the file as a
    script); the README quotes it.  It sets no bound -- the bound is the contract's 1e-4 -- but it must lie within it."""
    with open(MEASURED) as f:
        m = json.load(f)
    for name in DT:
        assert m[name]["bound"] == REL and 0 < m[name]["sums_worst"] <= REL and 0 <= m[name]["optimum_worst"] <= REL


def measured():
    return {name: {"sums_worst": WORST.get(("sums", name)), "optimum_worst": WORST.get(("optimum", name)), "bound": REL} for name in DT}


if __name__ == "__main__":
    me = os.path.abspath(__file__)                                   # the test of the file this run writes is left to the suite
    rc = pytest.main([me, "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not test_measured_file_records"])
    out = sys.modules["test_ctc_align_gpu"].measured()               # the module pytest imported holds the run's figures
    out["note"] = ("worst error, relative to max(1, |x|), of score / tok_score against float64 sums along the returned path "
                   "(sums_worst) and of the returned path's float64 score against the float64 optimum (optimum_worst) over the cases "
                   "of tests/test_ctc_align_gpu.py on an MI355X; the tests hold both to `bound`")
    if rc == 0 and len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))
