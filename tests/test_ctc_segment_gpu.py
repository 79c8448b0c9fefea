"""The segmentation kernels (csrc/ctc_segment.hip) and CTCSegmenter on the GPU against the float64 rule of tests/ctc_segment_ref.py,
which is fed the very values the kernels read (f32, or rounded to bf16).

Every recording of every case, none skipped: `states` is a valid path, `frames` and `utt_frames` are exactly those of the returned
states, `score`, `tok_score`, `utt_score` and the two confidences agree with float64 sums along the RETURNED path, and -- where the
float64 recursion is run -- the returned path's float64 value is within twice the bound of the float64 optimum.  Bounds: 1e-4 relative
to max(1, |x|) where n <= 2,048 (the project's), u = (n + 8) 2^-24 sum max(1, |lp|) over the frames summed for longer sums
(ctc_segment_ref.bound_u).  Planted recordings (noise, then N(0, 1) logits with a bonus along a drawn path, then noise) must come
back state for state; at the large sizes the planted path and float64 sums along it are the reference, no float64 recursion runs.
Outputs are filled with sentinels first: what the rule calls "not written" must still hold them.  Targets and offsets are padded with
junk, rows with 1e30.  `python tests/test_ctc_segment_gpu.py OUT.json` writes the worst errors of a run
(tests/golden/ctc_segment_measured.json)."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import ctc_align_ref as A
import ctc_segment_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAMES = ["f32", "bf16"]
REL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
MEASURED = os.path.join(HERE, "golden", "ctc_segment_measured.json")
WORST = {}                            # (unit, dtype name) -> worst error seen in this process, in units of the bound
JUNK = (10 ** 12, -5, 2 ** 31)        # what pads targets and offsets beyond their lengths
S_INT, S_STATE = -7, -9               # sentinels of the integer outputs and of states
OUT = ("states", "frames", "tok_score", "score", "utt_frames", "utt_score", "utt_conf_mean", "utt_conf_min", "status")


def device_rows(x, name, ld, unaligned=False):
    """x f32 [T, B, V] (already rounded to the dtype) -> device view [T, B, V] of a buffer with row stride ld, the padding filled with
    1e30; unaligned: the view starts one element into the allocation"""
    T, B, V = x.shape
    flat = torch.full((T * B * ld + 1,), 1e30, dtype=DT[name], device=DEV)
    buf = (flat[1:] if unaligned else flat[:-1]).view(T, B, ld)
    buf[..., :V] = torch.from_numpy(x).to(DEV).to(DT[name])
    v = buf[..., :V]
    assert torch.equal(v.float().cpu(), torch.from_numpy(x)), "the reference must see the values the kernel reads"
    assert (v.data_ptr() % 16 != 0) == unaligned
    return v


def call_segment(logits, in_len, targets, tgt_len, utt_end, n_utt, blank, flags, window):
    """s2t_ctc_segment on sentinel-filled outputs; a dict of numpy arrays"""
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd import lib as L
    T, B, V = logits.shape
    Lmax, Umax = targets.shape[1], utt_end.shape[1]
    i32 = lambda shape, fill: torch.full(shape, fill, dtype=torch.int32, device=DEV)
    f32 = lambda shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    out = dict(states=i32((B, T), S_STATE), frames=i32((B, Lmax, 2), S_INT), tok_score=f32((B, Lmax)), score=f32((B,)),
               utt_frames=i32((B, Umax, 2), S_INT), utt_score=f32((B, Umax)), utt_conf_mean=f32((B, Umax)), utt_conf_min=f32((B, Umax)),
               status=i32((B,), S_INT))
    lib = L.load()
    ws = torch.empty((int(lib.s2t_ctc_segment_workspace(T, B, Lmax, Umax)),), dtype=torch.uint8, device=DEV)
    L.check(lib.s2t_ctc_segment(L.dt(logits), L.ptr(logits), L.ptr(in_len), L.ptr(targets), L.ptr(tgt_len), L.ptr(utt_end), L.ptr(n_utt),
                                L.ptr(ws), *[L.ptr(out[k]) for k in OUT], T, B, V, K._row_ld(logits), Lmax, Umax, int(blank), flags, window,
                                L.stream()), "s2t_ctc_segment")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(recs, name, blank, flags=3, window=30, Lmax=None, Umax=None, ld=None, unaligned=False, T=None):
    """recs: dicts with x [n_b, V] (rounded), utts, and optionally n (frames used), tgt_len, n_utt, utt_end (overrides).  Shorter
    recordings are padded to T frames with N(0, 1) rows.  Returns (outputs, x [T, B, V], in_len)."""
    V = recs[0]["x"].shape[1]
    T = T or max(r["x"].shape[0] for r in recs)
    ys = [[c for u in r["utts"] for c in u] for r in recs]
    Lmax = Lmax or max(len(y) for y in ys)
    Umax = Umax or max(len(r["utts"]) for r in recs)
    x = A.round_to(np.random.default_rng(5).standard_normal((T, len(recs), V)).astype(np.float32), name)
    targets, utt_end = np.empty((len(recs), Lmax), np.int64), np.empty((len(recs), Umax), np.int64)
    for b, r in enumerate(recs):
        x[:r["x"].shape[0], b] = r["x"]
        targets[b] = [JUNK[(b + i) % 3] for i in range(Lmax)]
        targets[b, :len(ys[b])] = ys[b]
        utt_end[b] = [JUNK[(b + i + 1) % 3] for i in range(Umax)]
        ends = r.get("utt_end", np.cumsum([len(u) for u in r["utts"]]).tolist())
        utt_end[b, :len(ends)] = ends
    in_len = [r.get("n", r["x"].shape[0]) for r in recs]
    tgt_len = [r.get("tgt_len", len(y)) for r, y in zip(recs, ys)]
    n_utt = [r.get("n_utt", len(r["utts"])) for r in recs]
    dev = lambda a, dt: torch.tensor(a, dtype=dt, device=DEV)
    out = call_segment(device_rows(x, name, ld or V + 3, unaligned), dev(in_len, torch.int32), torch.from_numpy(targets).to(DEV),
                       dev(tgt_len, torch.int64), torch.from_numpy(utt_end).to(DEV), dev(n_utt, torch.int64), blank, flags, window)
    return out, x, in_len


@functools.lru_cache(maxsize=None)
def _reference(key):
    x, n, utts, blank, fs, fe = _REGISTRY[key]
    return R.segment(x, n, utts, blank, 30, fs, fe)


_REGISTRY = {}


def ref_of(x, n, utts, blank, flags):
    """the float64 recursion for a recording, once per process"""
    key = (x.shape, n, tuple(tuple(u) for u in utts), blank, flags, hash(x[:n].tobytes()))
    _REGISTRY[key] = (x, n, [list(u) for u in utts], blank, bool(flags & 1), bool(flags & 2))
    return _reference(key)


def note(name, err, bound, rel):
    """remember an error in units of its bound and, for the record, relative to max(1, |x|)"""
    WORST[("u", name)] = max(WORST.get(("u", name), 0.0), err / bound)
    WORST[("rel", name)] = max(WORST.get(("rel", name), 0.0), rel)


def close(got, ref, name, n, vals, what):
    """|got - ref| within the bound of a sum over the emissions `vals` (the terms summed) of a recording of n frames"""
    bound = R.bound_short(ref) if n <= 2048 else R.bound_u(len(vals), vals)
    err = abs(float(got) - ref)
    assert err <= bound, (what, float(got), ref, err, bound)
    note(name, err, bound, err / max(1.0, abs(ref)))


def check(out, b, x, n, utts, blank, name, what, flags=3, window=30, path=None, optimum=True, utt_ref=None):
    """everything the module docstring lists for recording b.  path: the planted path the states must equal; optimum: run the float64
    recursion and compare values; utt_ref: (utt_frames, utt_conf_min) of a reference the outputs must match instead of the rule's
    (the wrong twins go through here)"""
    T, Lmax, Umax = out["states"].shape[1], out["frames"].shape[1], out["utt_frames"].shape[1]
    y = [c for u in utts for c in u]
    L, U = len(y), len(utts)
    assert out["status"][b] == 0, (what, b, out["status"][b])
    st = out["states"][b, :n].astype(np.int64)
    assert R.is_valid_path(st, y, n), (what, b, st[:20])
    assert (out["states"][b, n:] == -1).all(), (what, b)
    if path is not None:
        assert st.tolist() == list(path), (what, b, "not the planted path", int(np.argmax(st != np.asarray(path))))
    lp = A.log_softmax64(x[:n, b])
    vals = R.values_on_path(lp, st, y, blank, bool(flags & 1), bool(flags & 2))
    s64, f64, t64 = R.sums_of_values(vals, st, L)
    assert out["frames"][b, :L].tolist() == f64.tolist(), (what, b, "frames are not those of the returned states")
    for k, cut in (("frames", L), ("tok_score", L), ("utt_frames", U), ("utt_score", U), ("utt_conf_mean", U), ("utt_conf_min", U)):
        rest = out[k][b, cut:]
        assert (np.isnan(rest) if rest.dtype == np.float32 else rest == S_INT).all(), (what, b, k, "entries behind the length were written")
    close(out["score"][b], s64, name, n, vals, (what, b, "score"))
    for i in range(L):
        close(out["tok_score"][b, i], t64[i], name, n, vals[f64[i, 0]:f64[i, 1]], (what, b, "tok_score", i))
    ufr, usc, umean, umin = R.utterances(vals, st, np.cumsum([len(u) for u in utts]), window)
    if utt_ref is not None:
        ufr, umin = utt_ref
    assert out["utt_frames"][b, :U].tolist() == np.asarray(ufr).tolist(), (what, b, "utt_frames are not those of the returned states")
    for u in range(U):
        f0, f1 = int(ufr[u][0]), int(ufr[u][1])
        close(out["utt_score"][b, u], usc[u], name, n, vals[f0:f1], (what, b, "utt_score", u))
        close(out["utt_conf_mean"][b, u] * (f1 - f0), umean[u] * (f1 - f0), name, n, vals[f0:f1], (what, b, "utt_conf_mean", u))
        w = min(window, f1 - f0)
        worst = max(np.convolve(np.maximum(1.0, np.abs(vals[f0:f1])), np.ones(w), "valid"))      # the heaviest window's bound holds for the lowest
        close(out["utt_conf_min"][b, u] * w, umin[u] * w, name, n, np.full(w, worst / w), (what, b, "utt_conf_min", u))
    if optimum:
        ref = ref_of(x[:, b], n, utts, blank, flags)
        assert ref["status"] == 0
        bound = 2 * (R.bound_short(ref["score"]) if n <= 2048 else R.bound_u(n, vals))
        assert abs(s64 - ref["score"]) <= bound, (what, b, "the returned path against the optimum", s64, ref["score"])
        note(name, abs(s64 - ref["score"]), bound, abs(s64 - ref["score"]) / max(1.0, abs(ref["score"])))


def untouched(out, b, what):
    """a refused recording: status 2 and nothing else written"""
    assert out["status"][b] == 2, (what, b, out["status"][b])
    for k in OUT[:-1]:
        v = out[k][b]
        assert (np.isnan(v) if v.dtype == np.float32 else (v == (S_STATE if k == "states" else S_INT))).all(), (what, b, k, "was written")


def planted(seed, T, V, L, U, name, pre, post, **kw):
    return R.planted_recording(seed, T, V, L, U, name, pre, post, **kw)


def random_recording(seed, n, V, L, U, name, scale=2.0):
    rng = np.random.default_rng(seed)
    y = A.draw_transcript(rng, L, V, V - 1)
    lens = R.split_utterances(rng, L, U)
    ends = np.cumsum(lens)
    return dict(x=A.round_to((rng.standard_normal((n, V)) * scale).astype(np.float32), name), utts=[y[e - c:e] for e, c in zip(ends, lens)])


# ------------------------------------------------------------------ both ends pinned: the aligner's bits
# padded width -> (frames, tokens, utterances) per recording.  The width picks the form on either side: the aligner's wave forms with
# K = 1, 2, 4, 8, 16 states per lane up to 31, 63, 127, 255, 511 tokens and its block form beyond, up to its limit of 4,095; the
# segmenter's K = 2, 4, 8 states per thread up to 1,023, 2,047, 4,095.  The longest transcript fills the width, every recording has
# at least 1.5 frames per token: a drawn transcript has a path.
PINNED = {31: ((56, 31, 4), (30, 12, 1), (9, 1, 1)),
          63: ((110, 63, 5), (64, 40, 40), (20, 3, 1)),
          127: ((200, 127, 6), (120, 64, 1), (199, 17, 17)),
          255: ((400, 255, 7), (260, 130, 2), (77, 1, 1)),
          511: ((1100, 511, 9), (700, 200, 1), (1037, 37, 37), (90, 1, 1)),
          512: ((800, 512, 9), (500, 300, 1), (790, 33, 33)),
          1024: ((1600, 1024, 9), (1000, 600, 3)),
          2048: ((3100, 2048, 9), (1500, 1000, 1)),
          4095: ((6200, 4095, 9), (2000, 1300, 2))}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("width", sorted(PINNED))
def test_pinned_ends_give_the_bits_of_ctc_align(width, name):
    """states, frames and the bytes of tok_score and score of the two kernels are equal for every pairing of their forms; the float64
    check of the segmenter's outputs runs for the recordings of at most 2,048 frames.  At widths 2,048 and 4,095 the recording that
    fills the width has 3,100 / 6,200 frames: it is compared with the aligner only, its shorter companion also with float64."""
    from fbk_fairseq_st_amd import kernels as K
    V, T = 16, PINNED[width][0][0]
    recs = [random_recording(100 + i, n, V, L, U, name) for i, (n, L, U) in enumerate(PINNED[width])]
    out, x, in_len = run(recs, name, V - 1, flags=0, T=T, ld=V)
    ys = [[c for u in r["utts"] for c in u] for r in recs]
    assert max(len(y) for y in ys) == width
    targets = torch.zeros((len(recs), width), dtype=torch.int64)
    for b, y in enumerate(ys):
        targets[b, :len(y)] = torch.tensor(y)
    lens = torch.tensor([len(y) for y in ys])
    al = K.ctc_align(device_rows(x, name, V), torch.tensor(in_len, dtype=torch.int32, device=DEV), targets.to(DEV), lens.to(DEV), V - 1)
    states, frames, tok_score, score, status = [t.cpu().numpy() for t in al]
    assert status.tolist() == [0] * len(recs) == out["status"].tolist()
    for b, y in enumerate(ys):
        n, L = in_len[b], len(y)
        assert np.array_equal(out["states"][b], states[b]), (b, "states")
        assert np.array_equal(out["frames"][b, :L], frames[b, :L]), (b, "frames")
        assert out["tok_score"][b, :L].tobytes() == tok_score[b, :L].tobytes(), (b, "tok_score")
        assert out["score"][b].tobytes() == score[b].tobytes(), (b, "score")
        if n <= 2048:
            check(out, b, x, n, recs[b]["utts"], V - 1, name, "pinned", flags=0)


# ------------------------------------------------------------------ free ends, planted paths
# the recording phase takes 2, 4, 8, 16, 32 states per thread up to L = 1,023, 2,047, 4,095, 8,191, 16,383 tokens
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("L", [1, 2, 31, 32, 1023, 1024, 2047, 2048, 4095, 4096, 4097, 8191, 8192])
def test_planted_paths_around_every_switch(L, name):
    """noise, the text, noise: the planted path state for state.  Tokens repeat with probability 0.05; a second recording of a third
    of the tokens shares the launch"""
    V = 6
    y_frames = L + L // 8 + 150
    a = planted(1000 + L, y_frames + 130, V, L, min(L, 7), name, 70, 60, p_repeat=0.05)
    b = planted(2000 + L, y_frames // 2, V, max(L // 3, 1), min(max(L // 3, 1), 3), name, 11, 0, p_repeat=0.05)
    out, x, in_len = run([a, b], name, V - 1)
    for i, r in enumerate((a, b)):
        check(out, i, x, in_len[i], r["utts"], V - 1, name, "L%d" % L, path=r["path"], optimum=L <= 32)


@pytest.mark.parametrize("name", NAMES)
def test_planted_path_at_the_limit(name):
    """16,383 tokens on the frames they force plus a few hundred"""
    L, V = 16383, 6
    rng = np.random.default_rng(77)
    y = A.draw_transcript(rng, L, V, V - 1, p_repeat=0.02)
    T = A.min_frames(y) + 300
    a = planted(77, T, V, L, 150, name, 120, 90, p_repeat=0.02)       # the same generator, the same first draws: the same transcript
    assert a["y"] == y
    out, x, in_len = run([a], name, V - 1)
    check(out, 0, x, T, a["utts"], V - 1, name, "limit", path=a["path"], optimum=False)


# ------------------------------------------------------------------ free ends, random logits
@pytest.mark.parametrize("flags", [3, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_random_logits_against_the_float64_optimum(name, flags):
    V = 24
    recs = [random_recording(300 + i, n, V, L, U, name) for i, (n, L, U) in enumerate(((1500, 600, 40), (700, 100, 7), (64, 5, 1), (333, 150, 150)))]
    out, x, in_len = run(recs, name, V - 1, flags=flags, window=30 if flags == 3 else 7)
    for b, r in enumerate(recs):
        check(out, b, x, in_len[b], r["utts"], V - 1, name, "random", flags=flags, window=30 if flags == 3 else 7)


# ------------------------------------------------------------------ window and span edge cases
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [2, 63, 64, 65, 127, 128, 129, 200])
def test_frame_counts_around_the_walk_block(n, name):
    V = 8
    recs = [planted(400 + n, n, V, min(6, n // 2), 2 if n > 3 else 1, name, n // 4, n // 5), random_recording(500 + n, n, V, min(20, n // 3 + 1), 1, name)]
    out, x, in_len = run(recs, name, V - 1, window=3)
    check(out, 0, x, n, recs[0]["utts"], V - 1, name, "n%d" % n, window=3, path=recs[0]["path"])
    check(out, 1, x, n, recs[1]["utts"], V - 1, name, "n%d" % n, window=3)


@pytest.mark.parametrize("name", NAMES)
def test_windows_against_span_lengths(name):
    """spans shorter than, equal to and one longer than the window; window 1; one utterance only; utterances of one token"""
    V = 8
    p = planted(600, 260, V, 30, 4, name, 40, 30)
    one = planted(601, 120, V, 9, 9, name, 10, 10)                    # nine utterances of one token
    single = planted(602, 120, V, 9, 1, name, 10, 10)
    ref = R.segment(p["x"], 260, p["utts"], V - 1)
    spans = sorted({int(b - a) for a, b in ref["utt_frames"]})
    for window in sorted({1, 2} | {max(1, s + d) for s in spans for d in (-1, 0, 1)}):
        out, x, in_len = run([p, one, single], name, V - 1, window=window)
        for b, r in enumerate((p, one, single)):
            check(out, b, x, in_len[b], r["utts"], V - 1, name, "window%d" % window, window=window, path=r["path"])
    assert all(len(u) == 1 for u in one["utts"]) and len(single["utts"]) == 1


@pytest.mark.parametrize("name", NAMES)
def test_the_widest_window(name):
    """window = 4,096 inside spans of more and of fewer frames"""
    V = 5
    # a bonus of 16: with free ends a stretch of 4,200 well-matched frames must still cost less than one misplaced token
    recs = [planted(610, 4300, V, 3, 1, name, 50, 50, bonus=16.0), planted(611, 4300, V, 40, 2, name, 50, 50, bonus=16.0)]
    out, x, in_len = run(recs, name, V - 1, window=4096)
    for b, r in enumerate(recs):
        check(out, b, x, 4300, r["utts"], V - 1, name, "window4096", window=4096, path=r["path"], optimum=False)
    spans = out["utt_frames"][:, :, 1] - out["utt_frames"][:, :, 0]
    assert spans[0, 0] >= 4096 > spans[1, 0], spans


@pytest.mark.parametrize("name", NAMES)
def test_equal_tokens_across_an_utterance_boundary(name):
    """... a | a ...: the blank the repeat forces belongs to neither utterance"""
    V = 6
    p = planted(620, 90, V, 12, 1, name, 8, 8, p_repeat=0.0)
    y = list(p["y"])
    y[6] = y[5]
    z, _ = A.extended(y, V - 1)
    rng = np.random.default_rng(620)
    path = R.draw_free_path(rng, y, 90, 8, 8)
    x = rng.standard_normal((90, V)).astype(np.float32)
    text = (path > 0) & (path < 2 * len(y))
    x[np.nonzero(text)[0], z[path[text]]] += 8.0
    rec = dict(x=A.round_to(x, name), utts=[y[:6], y[6:]])
    out, xb, in_len = run([rec], name, V - 1, window=4)
    check(out, 0, xb, 90, rec["utts"], V - 1, name, "boundary", window=4, path=path)
    (a0, a1), (b0, b1) = out["utt_frames"][0, :2].tolist()
    assert b0 > a1 and (out["states"][0, a1:b0] == 12).all(), "the forced blank (state 12) lies between the spans"


# ------------------------------------------------------------------ layout and inputs
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("ld,unaligned", [(5008, False), (5003, True)])
def test_flagship_vocabulary_padded_rows_unaligned_base(ld, unaligned, name):
    V = 5001
    recs = [planted(630, 200, V, 60, 4, name, 30, 20, bonus=14.0), planted(631, 150, V, 33, 2, name, 0, 25, bonus=14.0)]
    out, x, in_len = run(recs, name, V - 1, ld=ld, unaligned=unaligned, Lmax=77, Umax=9)
    for b, r in enumerate(recs):
        check(out, b, x, in_len[b], r["utts"], V - 1, name, "V5001-ld%d" % ld, path=r["path"])


def test_both_integer_dtypes_for_lengths_and_tokens():
    from fbk_fairseq_st_amd.ctc_segmenter import CTCSegmenter
    from fbk_fairseq_st_amd.data import Dictionary
    d = Dictionary.synthetic(3)
    d.add_symbol("<ctc_blank>")
    V = len(d)
    recs = [planted(640 + i, 80 - 9 * i, V, 7 + i, 2, "f32", 9, 6) for i in range(3)]
    x = np.zeros((80, 3, V), np.float32)
    for b, r in enumerate(recs):
        x[:r["T"], b] = r["x"]
    xd = torch.from_numpy(x).to(DEV)
    seg = CTCSegmenter(d, window=4)
    # int32 lengths with device token tensors, int64 lengths with host token tensors
    res = [seg.segment_logits(xd, torch.tensor([r["T"] for r in recs], dtype=dt), [[torch.tensor(u, dtype=dt, device=where) for u in r["utts"]] for r in recs])
           for dt, where in ((torch.int32, DEV), (torch.int64, "cpu"))]
    for r, a, b in zip(recs, *res):
        assert a["status"] == b["status"] == 0 and a["states"].tolist() == b["states"].tolist() == r["path"].tolist()
        assert float(a["score"]) == float(b["score"]) and a["utterances"][1]["frames"].tolist() == b["utterances"][1]["frames"].tolist()
        ref = R.segment(r["x"], r["T"], r["utts"], V - 1, window=4)
        assert [u["frames"].tolist() for u in a["utterances"]] == ref["utt_frames"].tolist()
        assert a["utterances"][0]["tokens"].dtype == torch.int64 and a["utterances"][0]["frames"].is_cuda


# ------------------------------------------------------------------ statuses, beside ordinary recordings
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("Lmax", [14, 1100])
def test_statuses_beside_ordinary_recordings(Lmax, name):
    """recordings 0, 3 and 9 are ordinary: bit for bit those of a batch in which the others are ordinary too"""
    V, T, blank = 12, 60, 11
    ok = [planted(700 + i, T, V, 9, 3, name, 7, 5) for i in range(10)]
    y = lambda r: [c for u in r["utts"] for c in u]

    def with_token(r, i, c):
        t = y(r)
        t[i] = c
        return dict(r, utts=[t[:4], t[4:]])
    few = dict(ok[1], n=A.min_frames(y(ok[1])) - 1)                     # one frame short: no path
    none = dict(ok[2], n=0)
    bad = [ok[0], few, none, ok[3], with_token(ok[4], 3, blank), with_token(ok[5], 8, V), with_token(ok[6], 0, -1),
           dict(ok[7], tgt_len=Lmax + 1), dict(ok[8], tgt_len=0), ok[9], dict(ok[0], n_utt=0), dict(ok[0], n_utt=8),
           dict(ok[0], utt_end=[4, 4, 9]), dict(ok[0], utt_end=[0, 4, 9]), dict(ok[0], utt_end=[3, 5, 8]), dict(ok[0], utt_end=[5, 3, 9])]
    out, x, in_len = run(bad, name, blank, Lmax=Lmax, Umax=7, window=5)
    plain, _, _ = run(ok + [ok[0]] * 6, name, blank, Lmax=Lmax, Umax=7, window=5)
    for b in (0, 3, 9):
        check(out, b, x, T, bad[b]["utts"], blank, name, "status", window=5, path=bad[b]["path"])
        for k in OUT:
            assert out[k][b].tobytes() == plain[k][b].tobytes(), (b, k)
    for b in (1, 2):
        U = len(bad[b]["utts"])
        assert out["status"][b] == 1 and out["score"][b] == -np.inf and (out["states"][b] == -1).all(), b
        assert (out["frames"][b, :9] == -1).all() and np.isneginf(out["tok_score"][b, :9]).all() and (out["frames"][b, 9:] == S_INT).all()
        assert (out["utt_frames"][b, :U] == -1).all() and (out["utt_frames"][b, U:] == S_INT).all()
        for k in ("utt_score", "utt_conf_mean", "utt_conf_min"):
            assert np.isneginf(out[k][b, :U]).all() and np.isnan(out[k][b, U:]).all(), (b, k)
    for b in (4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15):
        untouched(out, b, "refused")


# ------------------------------------------------------------------ batch independence
@pytest.mark.parametrize("name", NAMES)
def test_a_recording_alone_and_in_a_batch_of_eight(name):
    V = 14
    recs = [random_recording(800 + i, 900 - 17 * i, V, 20 + 60 * i, 1 + i, name) for i in range(8)]
    out, x, in_len = run(recs, name, V - 1, ld=V + 1, window=9)
    for b in (0, 4, 7):
        alone, _, _ = run([recs[b]], name, V - 1, ld=V + 5, window=9, T=in_len[b] + 3)
        L, U, n = sum(len(u) for u in recs[b]["utts"]), len(recs[b]["utts"]), in_len[b]
        for k, cut in (("states", n), ("frames", L), ("tok_score", L), ("utt_frames", U), ("utt_score", U), ("utt_conf_mean", U), ("utt_conf_min", U)):
            assert out[k][b, :cut].tobytes() == alone[k][0, :cut].tobytes(), (b, k)
        assert out["score"][b].tobytes() == alone["score"][0].tobytes() and out["status"][b] == alone["status"][0] == 0
        check(out, b, x, n, recs[b]["utts"], V - 1, name, "batch", window=9)
        # the padded width selects the states per thread (2 up to 1,023 tokens, 4 up to 2,047, 8 up to 4,095): the same bits from each
        for Lmax in (1100, 2100):
            wide, _, _ = run([recs[b]], name, V - 1, ld=V + 2, window=9, Lmax=Lmax, Umax=U + 3)
            for k, cut in (("states", n), ("frames", L), ("tok_score", L), ("utt_frames", U), ("utt_score", U), ("utt_conf_mean", U), ("utt_conf_min", U)):
                assert wide[k][0, :cut].tobytes() == alone[k][0, :cut].tobytes(), (b, k, Lmax)
            assert wide["score"][0].tobytes() == alone["score"][0].tobytes() and wide["status"][0] == 0


# ------------------------------------------------------------------ the wrong twins
@pytest.mark.parametrize("name", NAMES)
def test_the_kernel_contradicts_every_twin(name):
    V = 5
    p = planted(3, 181, V, 15, 4, name, 19, 11)
    out, x, in_len = run([p], name, V - 1, window=8)
    right = R.segment(p["x"], 181, p["utts"], V - 1, window=8)
    assert right["states"].tolist() == p["path"].tolist()
    check(out, 0, x, 181, p["utts"], V - 1, name, "twin", window=8, path=right["states"], utt_ref=(right["utt_frames"], right["utt_conf_min"]))
    for twin in ("charge_free", "span_from_blanks", "window_leaves_span"):
        wrong = R.segment(p["x"], 181, p["utts"], V - 1, window=8, **{twin: True})
        assert wrong["states"].tolist() != right["states"].tolist() or wrong["utt_frames"].tolist() != right["utt_frames"].tolist() or \
            np.abs(wrong["utt_conf_min"] - right["utt_conf_min"]).max() > 1e-3, (twin, "this case does not tell the twin from the rule")
        with pytest.raises(AssertionError):
            check(out, 0, x, 181, p["utts"], V - 1, name, twin, window=8, path=wrong["states"],
                  utt_ref=(wrong["utt_frames"], wrong["utt_conf_min"]))


# ------------------------------------------------------------------ kernels.ctc_segment, and end to end
def test_kernels_entry_allocates_and_handles_empty():
    from fbk_fairseq_st_amd import kernels as K
    p = planted(900, 50, 9, 6, 2, "f32", 8, 8)
    x = torch.from_numpy(p["x"][:, None, :]).to(DEV)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)
    n = torch.tensor([50], dtype=torch.int32, device=DEV)
    args = (i64([p["y"]]), i64([6]), i64([np.cumsum([len(u) for u in p["utts"]]).tolist()]), i64([2]), 8)
    out = dict(zip(OUT, K.ctc_segment(x, n, *args, window=3)))
    ref = R.segment(p["x"], 50, p["utts"], 8, window=3)
    assert out["status"].tolist() == [0] and out["states"][0].tolist() == p["path"].tolist() == ref["states"].tolist()
    assert out["utt_frames"][0].tolist() == ref["utt_frames"].tolist()
    assert np.abs(out["utt_conf_min"][0].cpu().numpy() - ref["utt_conf_min"]).max() <= REL
    pinned = dict(zip(OUT, K.ctc_segment(x, n, *args, free_start=False, free_end=False)))
    assert float(pinned["score"]) < float(out["score"]) - 10
    empty = dict(zip(OUT, K.ctc_segment(x[:0], n, *args)))
    assert empty["status"].tolist() == [1] and empty["states"].shape == (1, 0)


_BUILT = {}


def tiny_model(name):
    """model_a (built with --ctc-compress-out) / model_c (without) of tests/helpers.py model_case, in f32, once"""
    if name not in _BUILT:
        import test_model_gpu as TM
        g, cfg, W, sample, meta, model, crit = TM.build(name, torch.float32)
        _BUILT[name] = (model, TM.to_dev(sample), meta, crit)
    return _BUILT[name]


def test_end_to_end_on_a_ctc_compress_model():
    """A recording made of the golden utterances' features with noise between them.  logits_of_recording with a window that holds the
    whole recording gives the logits of one un-windowed encoder call; with short windows every window's kept frames are those of an
    encoder call on that window alone (a transformer's output depends on what the window holds, so short windows are compared window
    by window); both within 1e-4.  generate is logits_of_recording followed by segment_logits, and the segmentation of those logits
    follows the float64 rule."""
    from fbk_fairseq_st_amd.ctc_segmenter import CTCSegmenter
    from fbk_fairseq_st_amd.data import Dictionary
    model, sample, meta, _ = tiny_model("model_a")
    assert meta["compress"]
    d = Dictionary.synthetic(meta["V_src"] - 5)
    d.add_symbol("<ctc_blank>")
    seg = CTCSegmenter(d, window=4)
    assert seg.blank == meta["blank"]
    ni = sample["net_input"]
    feats, lens = ni["src_tokens"], ni["src_lengths"].tolist()
    gen = torch.Generator().manual_seed(9)
    noise = lambda k: (torch.randn(k, feats.shape[2], generator=gen) * float(feats.std())).to(feats)
    parts = [noise(24)]
    for b in range(feats.shape[0]):
        parts += [feats[b, :lens[b]], noise(16)]
    rec = torch.cat(parts)
    n_in = rec.shape[0] - rec.shape[0] % 4
    rec = rec[:n_in]
    model.train()
    whole, n4 = seg.logits_of_recording(model, rec, n_in, window_frames=4 * ((n_in + 3) // 4) + 8, context_frames=0)
    assert model.training
    model.eval()
    with torch.no_grad():
        enc = model.encoder(src_tokens=rec[None], src_lengths=torch.tensor([n_in], device=rec.device))
    assert n4 == enc.ctc_out.shape[0] == n_in // 4 and tuple(whole.shape) == (n4, 1, enc.ctc_out.shape[2])
    err = lambda a, b: float(((a.float() - b.float()).abs() / b.float().abs().clamp(min=1)).max())
    assert err(whole[:, 0], enc.ctc_out[:, 0]) <= REL
    window, context = 64, 8
    cut, n4c = seg.logits_of_recording(model, rec, n_in, window_frames=window, context_frames=context, windows_per_call=3)
    plan = seg.window_plan(n_in, window, context)
    assert n4c == n4 and len(plan) >= 4
    at = 0
    for start, stop, lo, hi in plan:
        with torch.no_grad():
            one = model.encoder(src_tokens=rec[None, start:stop], src_lengths=torch.tensor([stop - start], device=rec.device)).ctc_out[:, 0]
        keep = one[lo:hi]
        assert at == start // 4 + lo and err(cut[at:at + keep.shape[0], 0], keep) <= REL, (start, stop)
        at += keep.shape[0]
    assert at == n4
    # what windowing itself changes (global attention sees less): reported, with no bound that could be derived for it
    far = (cut[:, 0].float() - enc.ctc_out[:, 0].float()).abs()
    print("windows of %d input frames with %d of context against the un-windowed call: largest difference of a logit %.3g, mean %.3g, "
          "frames whose arg-max differs %d of %d" % (window, context, float(far.max()), float(far.mean()),
                                                      int((cut[:, 0].argmax(-1) != enc.ctc_out[:, 0].argmax(-1)).sum()), n4))
    # the utterances: a few tokens each, few enough for the frames the recording has
    tr, tr_len = sample["transcript_target"], sample["transcript_target_lengths"].tolist()
    utts = [[c for c in tr[b, :min(tr_len[b], 3)].tolist() if c != seg.blank] or [4] for b in range(feats.shape[0])]
    big = {"net_input": {"src_tokens": rec[None], "src_lengths": torch.tensor([n_in], device=rec.device)}, "utterances": [utts]}
    got = seg.generate([model], big)
    again = seg.segment_logits(seg.logits_of_recording(model, rec, n_in)[0], torch.tensor([n4]), [utts])
    assert len(got) == 1 and got[0]["status"] == again[0]["status"] == 0 and torch.equal(got[0]["states"], again[0]["states"])
    x = whole[:, 0].float().cpu().numpy()
    ref = R.segment(x, n4, utts, seg.blank, window=4)
    st = got[0]["states"].cpu().numpy().astype(np.int64)
    y = [c for u in utts for c in u]
    assert R.is_valid_path(st, y, n4)
    vals = R.values_on_path(ref["lp"], st, y, seg.blank)
    assert abs(vals.sum() - ref["score"]) <= 2 * R.bound_short(ref["score"]) and abs(float(got[0]["score"]) - vals.sum()) <= R.bound_short(vals.sum())
    ufr, usc, umean, umin = R.utterances(vals, st, np.cumsum([len(u) for u in utts]), 4)
    assert [u["frames"].tolist() for u in got[0]["utterances"]] == ufr.tolist()
    for u, d_ in enumerate(got[0]["utterances"]):
        assert d_["tokens"].tolist() == utts[u] and abs(float(d_["conf_min"]) - umin[u]) <= R.bound_short(umin[u])
        assert abs(float(d_["score"]) - usc[u]) <= R.bound_short(usc[u])
    segs = seg.input_segments(got[0], n_in, pad_frames=8)
    assert segs.shape == (len(utts), 2) and int(segs.min()) >= 0 and int(segs.max()) <= n_in and bool((segs[1:, 0] >= segs[:-1, 1] - 16).all())
    plain, psample, pmeta, _ = tiny_model("model_c")
    with pytest.raises(ValueError, match="segment_logits"):
        seg.generate([plain], {"net_input": psample["net_input"], "utterances": [[[4]]] * psample["net_input"]["src_tokens"].shape[0]})


def test_measured_file_records_both_dtypes_within_the_bounds():
    """tests/golden/ctc_segment_measured.json: the worst errors of a run of this file on an MI355X (written by running the file as a
    script), in units of the bound that held for each comparison and relative to max(1, |x|).  It sets no bound, but must lie within."""
    with open(MEASURED) as f:
        m = json.load(f)
    for name in DT:
        assert 0 < m[name]["worst_in_units_of_the_bound"] <= 1 and 0 < m[name]["worst_in_units_of_1e-4"] <= 1


def measured():
    return {name: {"worst_in_units_of_the_bound": WORST.get(("u", name)), "worst_in_units_of_1e-4": WORST.get(("rel", name), 0.0) / REL}
            for name in DT}


if __name__ == "__main__":
    me = os.path.abspath(__file__)                                   # the test of the file this run writes is left to the suite
    rc = pytest.main([me, "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", "-k", "not test_measured_file_records"])
    out = sys.modules["test_ctc_segment_gpu"].measured()             # the module pytest imported holds the run's figures
    out["note"] = ("worst error of score / tok_score / utt_score / the confidences against float64 sums along the returned path, and of "
                   "the returned path's float64 value against the float64 optimum, over the cases of tests/test_ctc_segment_gpu.py on an "
                   "MI355X: in units of the bound that held for the comparison (1e-4 max(1, |x|) for n <= 2,048, u = (n + 8) 2^-24 "
                   "sum max(1, |lp|) above, twice that against the optimum) and, relative to max(1, |x|), in units of 1e-4")
    if rc == 0 and len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))
