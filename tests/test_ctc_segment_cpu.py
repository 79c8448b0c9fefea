"""The CTC segmenter without a GPU: the entry points are exported, bound and refuse bad arguments before anything is launched, in the
header's order; the workspace formula; and the host logic of CTCSegmenter -- concatenation of the utterances, the result's layout,
batch cutting at the workspace limit, input_segments' clipping, and the window arithmetic of logits_of_recording against a stub
encoder whose output frame j carries its global index -- with kernels.ctc_segment replaced by the float64 reference
(tests/ctc_segment_ref.py; the kernels have their own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ctc_segment_ref as R
from fbk_fairseq_st_amd import ctc_segmenter as CS
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd.data import Dictionary

NEW = ("s2t_ctc_segment_workspace", "s2t_ctc_segment")
FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
MAX_TARGET, MAX_UTT, MAX_WINDOW = 16383, 4096, 4096
POINTERS = ("logits", "in_len", "targets", "tgt_len", "utt_end", "n_utt", "ws", "states", "frames", "tok_score", "score", "utt_frames",
            "utt_score", "utt_conf_mean", "utt_conf_min", "status")
ARGS = (("dtype", 0),) + tuple((p, FAKE) for p in POINTERS) + (("T", 4), ("B", 2), ("V", 12), ("ld", 12), ("Lmax", 3), ("Umax", 2),
                                                                ("blank", 11), ("flags", 3), ("window", 30), ("stream", None))


def ws_bytes(T, B, Lmax):
    return (4 * T * B * (3 + (2 * Lmax + 1 + 15) // 16) + 255) // 256 * 256


def test_the_feature_is_there():
    """what fails without the feature: the module and the export"""
    import fbk_fairseq_st_amd.ctc_segmenter  # noqa: F401
    assert hasattr(ctypes.CDLL(L.LIB_PATH), "s2t_ctc_segment")


def test_exports_bindings_and_workspace_size():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name)
    assert "s2t_ctc_segment_workspace" in L._SIZE_T_RESULT
    assert len(L.SIGNATURES["s2t_ctc_segment"]) == len(ARGS) == 27 and len(L.SIGNATURES["s2t_ctc_segment_workspace"]) == 4
    for T, B, Lmax in ((375, 16, 60), (22500, 1, 5000), (22500, 1, 15000), (7500, 8, 2000), (1, 1, 1), (40000, 1, MAX_TARGET), (7, 3, 512)):
        assert lib.s2t_ctc_segment_workspace(T, B, Lmax, 7) == ws_bytes(T, B, Lmax) == CS.workspace_bytes(T, B, Lmax), (T, B, Lmax)
        assert K.ctc_segment_workspace(T, B, Lmax, MAX_UTT) == ws_bytes(T, B, Lmax)
    # no emission table: nothing in it is proportional to frames times tokens but the 2 bits of a back-pointer
    assert lib.s2t_ctc_segment_workspace(22500, 1, 15000, 150) < 22500 * (12 + (2 * 15000 + 16) // 4 + 4) < 1 << 30
    assert lib.s2t_ctc_segment_workspace(0, 16, 5, 1) == 0 and lib.s2t_ctc_segment_workspace(5, 0, 5, 1) == 0
    assert lib.s2t_ctc_segment_workspace(5, 5, 0, 1) == 0 and lib.s2t_ctc_segment_workspace(5, 5, MAX_TARGET + 1, 1) == 0
    assert lib.s2t_ctc_segment_workspace(5, 5, 5, 0) == 0 and lib.s2t_ctc_segment_workspace(5, 5, 5, MAX_UTT + 1) == 0
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    for name, value in (("TARGET", MAX_TARGET), ("UTT", MAX_UTT), ("WINDOW", MAX_WINDOW)):
        assert "#define S2T_CTC_SEGMENT_MAX_%s %d" % (name, value) in text
    assert (CS.MAX_TARGET, CS.MAX_UTT, CS.MAX_WINDOW) == (MAX_TARGET, MAX_UTT, MAX_WINDOW)


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    assert f(T=0) == 0 and f(B=0) == 0 and f(T=0, logits=None) == 0 and f(T=-1) == 0      # an empty problem: nothing looked at
    for name in POINTERS:
        assert f(**{name: None}) == -22, name
    assert f(V=1, ld=1, blank=0) == -22 and f(ld=11) == -22
    assert f(blank=12) == -22 and f(blank=-1) == -22
    assert f(Lmax=0) == -22 and f(Umax=0) == -22
    assert f(T=1 << 16, B=1 << 15) == -22, "T*B = 2^31"
    assert f(flags=4) == -22 and f(flags=-1) == -22
    assert f(dtype=2) == -95 and f(dtype=-1) == -95
    assert f(Lmax=MAX_TARGET + 1) == -95 and f(Umax=MAX_UTT + 1) == -95
    assert f(window=0) == -95 and f(window=MAX_WINDOW + 1) == -95
    # the order the header states: a malformed call is -22 even where it is also out of range
    assert f(dtype=2, logits=None) == -22 and f(Lmax=MAX_TARGET + 1, ld=11) == -22 and f(window=0, flags=4) == -22
    assert f(T=0, dtype=2, Lmax=MAX_TARGET + 1) == 0


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_ctc_segment)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        getattr(raw, name).argtypes = L.SIGNATURES[name]
    raw.s2t_ctc_segment_workspace.restype = ctypes.c_size_t
    check_refusals(fast.s2t_ctc_segment)
    check_refusals(raw.s2t_ctc_segment)
    for args in ((1 << 20, 4096, 511, 9), (40000, 1, MAX_TARGET, MAX_UTT), (0, 1, 1, 1)):
        assert fast.s2t_ctc_segment_workspace(*args) == raw.s2t_ctc_segment_workspace(*args) == (ws_bytes(*args[:3]) if args[0] else 0)
    assert fast.s2t_ctc_segment_workspace(1 << 20, 4096, 511, 9) > 1 << 32, "a size_t result, not an int"


def test_kernels_entry_refuses_without_a_launch():
    x, n = torch.zeros(4, 2, 12), torch.zeros(2, dtype=torch.int32)
    i64 = lambda *shape: torch.ones(shape, dtype=torch.int64)
    ok = dict(logits=x, in_len=n, targets=i64(2, 3), tgt_len=i64(2), utt_end=i64(2, 2), n_utt=i64(2), blank=11)
    bad = [dict(targets=i64(2, 3).int()), dict(targets=i64(3, 3)), dict(tgt_len=i64(2).int()), dict(utt_end=i64(2, 2).int()),
           dict(n_utt=i64(3)), dict(targets=i64(2, 0)), dict(targets=i64(2, MAX_TARGET + 1)), dict(utt_end=i64(2, 0)),
           dict(utt_end=i64(2, MAX_UTT + 1)), dict(window=0), dict(window=MAX_WINDOW + 1), dict(in_len=n.long())]
    for change in bad:
        with pytest.raises(ValueError):
            K.ctc_segment(**{**ok, **change})
    out = K.ctc_segment(**{**ok, "logits": x[:, :0], "in_len": n[:0], "targets": i64(0, 3), "tgt_len": i64(0), "utt_end": i64(0, 2), "n_utt": i64(0)})
    assert [t.shape[0] for t in out] == [0] * 9
    out = K.ctc_segment(**{**ok, "logits": x[:0]})                       # T = 0: no frames, no path
    assert out[-1].tolist() == [1, 1] and out[3].tolist() == [float("-inf")] * 2 and out[0].shape == (2, 0)


# ------------------------------------------------------------------ host logic
V = 9


def src_dict():
    d = Dictionary.synthetic(V - 5)                                   # 4 specials + (V - 5) words + the blank = V entries
    d.add_symbol("<ctc_blank>")
    assert len(d) == V
    return d


@pytest.fixture
def calls(monkeypatch):
    c = []

    def ctc_segment(logits, in_len, targets, tgt_len, utt_end, n_utt, blank, free_start=True, free_end=True, window=30):
        T, B, Vn = logits.shape
        Lmax, Umax = targets.shape[1], utt_end.shape[1]
        c.append(dict(shape=(T, B, Lmax, Umax), dtypes=(in_len.dtype, targets.dtype, tgt_len.dtype, utt_end.dtype, n_utt.dtype),
                      flags=(free_start, free_end, window), blank=blank))
        assert CS.workspace_bytes(T, B, Lmax) <= CS.WORKSPACE_LIMIT
        states = np.full((B, T), -9, np.int32)
        frames, tok = np.full((B, Lmax, 2), -7, np.int32), np.full((B, Lmax), np.nan, np.float32)
        uf, us = np.full((B, Umax, 2), -7, np.int32), np.full((3, B, Umax), np.nan, np.float32)
        score, status = np.full(B, np.nan, np.float32), np.zeros(B, np.int32)
        for b in range(B):
            Ln, U, n = int(tgt_len[b]), int(n_utt[b]), min(max(int(in_len[b]), 0), T)
            y = targets[b, :Ln].tolist()
            if any(t < 0 or t >= Vn or t == blank for t in y):
                status[b] = 2
                continue
            ends = [0] + utt_end[b, :U].tolist()
            r = R.segment(logits[:, b].double().numpy(), n, [y[a:e] for a, e in zip(ends, ends[1:])], blank, window, free_start, free_end)
            status[b], score[b] = r["status"], r["score"]
            if r["status"] == 0:
                states[b, :n], frames[b, :Ln], tok[b, :Ln] = r["states"], r["frames"], r["tok_score"]
                uf[b, :U], us[0, b, :U], us[1, b, :U], us[2, b, :U] = r["utt_frames"], r["utt_score"], r["utt_conf_mean"], r["utt_conf_min"]
        return tuple(torch.from_numpy(a) for a in (states, frames, tok, score, uf, us[0], us[1], us[2], status))
    monkeypatch.setattr(CS.K, "ctc_segment", ctc_segment)
    return c


def recordings(seeds, T):
    """planted recordings of different sizes in one [T, B, V] tensor, with their utterances"""
    cases = [R.planted_recording(s, T - 5 * i, V, 6 + 3 * i, 1 + i % 3, "f32", 4 + i, 3) for i, s in enumerate(seeds)]
    x = torch.randn(T, len(cases), V, generator=torch.Generator().manual_seed(3))
    for b, c in enumerate(cases):
        x[:c["T"], b] = torch.from_numpy(c["x"])
    return x, torch.tensor([c["T"] for c in cases]), cases


def test_segment_logits_concatenates_and_lays_out_the_result(calls):
    x, in_len, cases = recordings((1, 2, 3), 90)
    seg = CS.CTCSegmenter(src_dict(), window=5)
    utts = [[torch.tensor(u) if i % 2 else list(u) for i, u in enumerate(c["utts"])] for c in cases]      # tensors and lists
    out = seg.segment_logits(x, in_len, utts)
    assert len(calls) == 1 and calls[0]["shape"] == (90, 3, 12, 3) and calls[0]["flags"] == (True, True, 5) and calls[0]["blank"] == V - 1
    assert calls[0]["dtypes"] == (torch.int32,) + (torch.int64,) * 4
    for b, (c, o) in enumerate(zip(cases, out)):
        assert o["status"] == 0 and o["states"].tolist() == c["path"].tolist() and o["states"].dtype == torch.int32
        ref = R.segment(c["x"], c["T"], c["utts"], c["blank"], window=5)
        assert float(o["score"]) == pytest.approx(ref["score"], rel=1e-6)
        assert len(o["utterances"]) == len(c["utts"])
        lo = 0
        for u, d in enumerate(o["utterances"]):
            cnt = len(c["utts"][u])
            assert set(d) == {"tokens", "frames", "score", "conf_mean", "conf_min", "positional_scores", "token_frames"}
            assert d["tokens"].tolist() == c["utts"][u] and d["tokens"].dtype == torch.int64
            assert d["frames"].tolist() == ref["utt_frames"][u].tolist() and d["frames"].dtype == torch.int32 and d["frames"].shape == (2,)
            assert d["token_frames"].tolist() == ref["frames"][lo:lo + cnt].tolist()
            assert d["positional_scores"].tolist() == pytest.approx(ref["tok_score"][lo:lo + cnt].tolist(), rel=1e-6)
            assert float(d["conf_min"]) == pytest.approx(ref["utt_conf_min"][u], rel=1e-6) and float(d["conf_mean"]) <= 0
            lo += cnt


def test_statuses_and_integer_dtypes(calls):
    x, in_len, cases = recordings((4, 5, 6), 60)
    utts = [c["utts"] for c in cases]
    utts[1] = [[V - 1]] + utts[1]                                        # the blank inside a transcript: refused
    in_len = in_len.clone()
    in_len[2] = 3                                                        # too few frames: no path
    out = CS.CTCSegmenter(src_dict(), free_end=False).segment_logits(x, in_len.int(), utts)
    assert [o["status"] for o in out] == [0, 2, 1] and calls[0]["flags"] == (True, False, 30)
    assert out[1]["states"].numel() == 0 and out[2]["states"].numel() == 0
    assert float(out[1]["score"]) == float(out[2]["score"]) == float("-inf")
    assert out[1]["utterances"][0]["tokens"].tolist() == [V - 1] and out[1]["utterances"][0]["frames"] is None
    assert out[2]["utterances"][0]["conf_min"] is None


def test_batches_are_cut_at_the_workspace_limit(calls, monkeypatch):
    x, in_len, cases = recordings((1, 2, 3, 4, 5), 100)
    utts = [c["utts"] for c in cases]                                   # 6, 9, 12, 15, 18 tokens
    seg = CS.CTCSegmenter(src_dict())
    whole = seg.segment_logits(x, in_len, utts)
    assert [c["shape"][1] for c in calls] == [5]
    del calls[:]
    monkeypatch.setattr(CS, "WORKSPACE_LIMIT", CS.workspace_bytes(100, 2, 18))
    assert CS.CTCSegmenter.chunk_recordings(100, [6, 9, 12, 15, 18]) == [(0, 2), (2, 4), (4, 5)]
    cut = seg.segment_logits(x, in_len, utts)
    assert [c["shape"][:3] for c in calls] == [(100, 2, 9), (100, 2, 15), (100, 1, 18)]
    for a, b in zip(whole, cut):
        assert a["status"] == b["status"] == 0 and torch.equal(a["states"], b["states"]) and float(a["score"]) == float(b["score"])
        assert all(torch.equal(p["frames"], q["frames"]) and torch.equal(p["tokens"], q["tokens"]) for p, q in zip(a["utterances"], b["utterances"]))
    monkeypatch.setattr(CS, "WORKSPACE_LIMIT", CS.workspace_bytes(100, 1, 18) - 1)
    with pytest.raises(ValueError, match="recording 4 alone .100 frames, 18 tokens. needs %d bytes" % CS.workspace_bytes(100, 1, 18)):
        seg.segment_logits(x, in_len, utts)


def test_the_class_refuses_what_lies_outside_the_limits(calls):
    seg, x, n = CS.CTCSegmenter(src_dict()), torch.zeros(10, 1, V), torch.tensor([10])
    for bad in ([[]], [[[1], []]], [[[1]] * (MAX_UTT + 1)], [[[1] * (MAX_TARGET + 1)]], [[[1]], [[2]]]):
        with pytest.raises(ValueError):
            seg.segment_logits(x, n, bad)
    for window in (0, MAX_WINDOW + 1):
        with pytest.raises(ValueError):
            CS.CTCSegmenter(src_dict(), window=window)
    with pytest.raises(ValueError, match="no <ctc_blank> entry"):
        CS.CTCSegmenter(Dictionary.synthetic(5))
    assert not calls


def test_input_segments_clip_to_the_neighbours_and_the_recording():
    u = lambda a, b: {"frames": torch.tensor([a, b], dtype=torch.int32)}
    res = {"status": 0, "utterances": [u(2, 10), u(11, 20), u(20, 26)]}
    assert CS.CTCSegmenter.input_segments(res, 101).tolist() == [[8, 40], [44, 80], [80, 101]]
    assert CS.CTCSegmenter.input_segments(res, 200, pad_frames=3).tolist() == [[5, 43], [41, 80], [80, 107]]
    assert CS.CTCSegmenter.input_segments(res, 104, pad_frames=50).tolist() == [[0, 44], [40, 80], [80, 104]]
    assert CS.CTCSegmenter.input_segments({"status": 1, "utterances": []}, 10) is None


class StubEncoder:
    """feature 0 of input frame i is its global index i; CTC frame j of a window is input frame 4 j: its logits carry 4 j's global
    index in column 0 and the window's place in the call in column 1"""

    def __init__(self, ctc=True):
        self.calls, self.ctc = [], ctc

    def __call__(self, src_tokens, src_lengths):
        from fbk_fairseq_st_amd.registry import CTCAwareEncoderOut, EncoderOut
        self.calls.append((tuple(src_tokens.shape), src_lengths.tolist()))
        Bn, W, _ = src_tokens.shape
        T4 = -(-W // 4)
        out = torch.zeros(T4, Bn, 3)
        out[:, :, 0] = src_tokens[:, ::4, 0].t()
        out[:, :, 1] = torch.arange(Bn)[None, :]
        if not self.ctc:
            return EncoderOut(out, None, None, None, src_tokens, src_lengths)
        return CTCAwareEncoderOut(out, None, None, None, src_tokens, src_lengths, out, None)


class StubModel:
    def __init__(self, ctc=True):
        self.encoder, self.training, self.modes = StubEncoder(ctc), True, []

    def eval(self):
        self.training = False
        self.modes.append("eval")

    def train(self, mode=True):
        self.training = mode
        self.modes.append("train" if mode else "eval")


@pytest.mark.parametrize("length,window,context,per_call", [(1000, 400, 40, 8), (1003, 400, 40, 2), (400, 400, 40, 8), (401, 400, 40, 8),
                                                            (37, 400, 40, 8), (2000, 120, 0, 3), (721, 400, 40, 1), (4, 8, 0, 8)])
def test_window_arithmetic_of_logits_of_recording(length, window, context, per_call):
    feats = torch.zeros(length + 6, 2)
    feats[:, 0] = torch.arange(length + 6)
    model = StubModel()
    seg = CS.CTCSegmenter(src_dict())
    logits, n4 = seg.logits_of_recording(model, feats, length, window, context, windows_per_call=per_call)
    assert n4 == -(-length // 4) and logits.shape == (n4, 1, 3)
    assert logits[:, 0, 0].tolist() == [4.0 * j for j in range(n4)], "every CTC frame once, in order, from the frame it stands for"
    plan = CS.CTCSegmenter.window_plan(length, window, context)
    step = window - 2 * context
    assert [p[0] for p in plan] == [k * step for k in range(len(plan))] and plan[-1][1] == length
    assert all(stop - start == window for start, stop, _, _ in plan[:-1]) and (len(plan) == 1 or plan[-2][0] + window < length)
    for k, (start, stop, lo, hi) in enumerate(plan):
        assert lo == (context // 4 if k else 0) and hi == (None if k == len(plan) - 1 else (window - context) // 4)
    assert len(model.encoder.calls) == -(-len(plan) // per_call) and all(c[0][0] <= per_call for c in model.encoder.calls)
    assert sum(len(c[1]) for c in model.encoder.calls) == len(plan)
    assert model.modes == ["eval", "train"] and model.training


def test_logits_of_recording_refusals():
    seg = CS.CTCSegmenter(src_dict())
    with pytest.raises(ValueError, match="the encoder returned no ctc_out .a model built without --ctc-compress-out."):
        seg.logits_of_recording(StubModel(ctc=False), torch.zeros(50, 2), 50)
    for window, context in ((402, 40), (400, 42), (80, 40), (400, -4)):
        with pytest.raises(ValueError):
            seg.logits_of_recording(StubModel(), torch.zeros(50, 2), 50, window, context)


def test_generate_is_the_windowed_encoder_followed_by_segment_logits(calls, monkeypatch):
    seg = CS.CTCSegmenter(src_dict(), window=4)
    x, in_len, cases = recordings((7, 8), 70)
    made = []

    def logits_of_recording(model, features, length, *a, **k):
        b = len(made)
        made.append((tuple(features.shape), length))
        return x[:int(in_len[b]), b:b + 1], int(in_len[b])
    monkeypatch.setattr(seg, "logits_of_recording", logits_of_recording)
    sample = {"net_input": {"src_tokens": torch.zeros(2, 280, 5), "src_lengths": torch.tensor([280, 260])}, "utterances": [c["utts"] for c in cases]}
    out = seg.generate([object()], sample)
    assert made == [((280, 5), 280), ((280, 5), 260)] and calls[0]["shape"][:2] == (70, 2)
    assert [o["states"].tolist() for o in out] == [c["path"].tolist() for c in cases]
    with pytest.raises(ValueError, match="exactly one model"):
        seg.generate([object(), object()], sample)
