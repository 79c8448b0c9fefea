"""The CTC aligner without a GPU: the new entry points are exported, bound and refuse bad arguments before anything is launched, and
the host logic of CTCAligner -- result keys and dtypes, empty transcripts, sentences without a path and refused ones inside a batch,
eval mode and its restoration, the refusals, input_frames -- with kernels.ctc_align replaced by the float64 reference
(tests/ctc_align_ref.py; the kernels have their own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ctc_align_ref as R
from fbk_fairseq_st_amd import ctc_aligner as CA
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd.data import Dictionary
from fbk_fairseq_st_amd.registry import CTCAwareEncoderOut, EncoderOut

NEW = ("s2t_ctc_align_workspace", "s2t_ctc_align")
FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
MAX_TARGET = 4095
ARGS = (("dtype", 0), ("logits", FAKE), ("in_len", FAKE), ("targets", FAKE), ("tgt_len", FAKE), ("ws", FAKE), ("states", FAKE),
        ("frames", FAKE), ("tok_score", FAKE), ("score", FAKE), ("status", FAKE), ("T", 4), ("B", 2), ("V", 12), ("ld", 12), ("Lmax", 3),
        ("blank", 11), ("stream", None))


def ws_bytes(T, B, Lmax):
    W = 64 if 2 * Lmax + 1 <= 1024 else (2 * Lmax + 1 + 15) // 16
    return (4 * T * B * (Lmax + 1 + W) + 255) // 256 * 256


def test_exports_bindings_and_workspace_size():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name)
    assert "s2t_ctc_align_workspace" in L._SIZE_T_RESULT
    assert len(L.SIGNATURES["s2t_ctc_align"]) == 18 and len(L.SIGNATURES["s2t_ctc_align_workspace"]) == 3
    assert lib.s2t_abi_version() == 9
    for T, B, Lmax in ((375, 16, 60), (375, 16, 511), (1500, 4, 1024), (1, 1, 0), (4200, 1, MAX_TARGET), (7, 3, 512)):
        assert lib.s2t_ctc_align_workspace(T, B, Lmax) == ws_bytes(T, B, Lmax), (T, B, Lmax)
    # the emissions of a sentence: L + 1 floats per frame; its back-pointers: 2 bits per frame and state
    assert lib.s2t_ctc_align_workspace(9, 2, 2000) >= 4 * 9 * 2 * 2001 + 9 * 2 * (2 * 2000 + 1) // 4
    assert lib.s2t_ctc_align_workspace(0, 16, 5) == 0 and lib.s2t_ctc_align_workspace(5, 0, 5) == 0
    assert lib.s2t_ctc_align_workspace(5, 5, -1) == 0 and lib.s2t_ctc_align_workspace(5, 5, MAX_TARGET + 1) == 0
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        assert "#define S2T_CTC_ALIGN_MAX_TARGET %d" % MAX_TARGET in f.read()
    assert CA.MAX_TARGET == MAX_TARGET


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name, d in ARGS:
        if d == FAKE:
            assert f(**{name: None}) == -22, name                        # null pointers
    assert f(ld=11) == -22 and f(V=1, ld=1, blank=0) == -22
    assert f(blank=12) == -22 and f(blank=-1) == -22
    assert f(Lmax=-1) == -22
    assert f(T=1 << 16, B=1 << 15) == -22, "T*B = 2^31"
    assert f(dtype=2) == -95 and f(dtype=-1) == -95
    assert f(Lmax=MAX_TARGET + 1) == -95
    assert f(T=0) == 0 and f(B=0) == 0 and f(T=0, logits=None) == 0          # an empty problem: nothing to do, nothing looked at
    assert f(T=-1) == 0 and f(T=-2, B=-2) == 0


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_ctc_align)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        getattr(raw, name).argtypes = L.SIGNATURES[name]
    raw.s2t_ctc_align_workspace.restype = ctypes.c_size_t
    check_refusals(fast.s2t_ctc_align)
    check_refusals(raw.s2t_ctc_align)
    for args in ((1 << 20, 4096, 511), (4200, 1, MAX_TARGET), (0, 1, 1)):
        assert fast.s2t_ctc_align_workspace(*args) == raw.s2t_ctc_align_workspace(*args) == (ws_bytes(*args) if args[0] else 0)
    assert fast.s2t_ctc_align_workspace(1 << 20, 4096, 511) > 1 << 32, "a size_t result, not an int"


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

    def ctc_align(logits, in_len, targets, tgt_len, blank):
        c.append((logits.dtype, tuple(logits.shape), in_len.dtype, targets.dtype, tgt_len.dtype, blank))
        out = R.align_batch(logits.float().numpy(), in_len.tolist(), targets.numpy(), tgt_len.tolist(), blank)
        return tuple(torch.from_numpy(a) for a in out)
    monkeypatch.setattr(CA.K, "ctc_align", ctc_align)
    return c


def _logits(T, B, seed=0):
    return torch.randn(T, B, V, generator=torch.Generator().manual_seed(seed)) * 3


class ToyEncoder:
    def __init__(self, owner, logits, lens, compress=True, fail=False):
        self.owner, self.logits, self.lens, self.compress, self.fail = owner, logits, lens, compress, fail
        self.seen_mode, self.seen_keys = [], []

    def __call__(self, **kw):
        self.seen_mode.append(self.owner.training)
        self.seen_keys.append(sorted(kw))
        if self.fail:
            raise RuntimeError("encoder failed")
        T, B = self.logits.shape[:2]
        eo = torch.zeros(3, B, 4)
        if not self.compress:
            return EncoderOut(eo, None, None, None, None, None)
        mask = None if self.lens is None else torch.arange(T)[None, :] >= torch.tensor(self.lens)[:, None]
        return CTCAwareEncoderOut(eo, None, None, None, None, None, self.logits, mask)


class ToyModel:
    def __init__(self, logits, lens, training=True, **kw):
        self.training = training
        self.encoder = ToyEncoder(self, logits, lens, **kw)

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        self.training = mode
        return self


def _sample(targets, lengths):
    B = len(lengths)
    return dict(net_input=dict(src_tokens=torch.zeros(B, 40, 80), src_lengths=torch.full((B,), 40), prev_output_tokens=torch.zeros(B, 3).long(),
                               transcript_prev_output_tokens=torch.zeros(B, 3).long()), target=torch.zeros(B, 3).long(),
                transcript_target=torch.tensor(targets), transcript_target_lengths=torch.tensor(lengths))


KEYS = ["alignment", "attention", "frames", "positional_scores", "score", "states", "status", "tokens"]
BLANK = V - 1
# sentence 0: three tokens; 1: the empty transcript; 2: five frames for `a a a` (needs five: fits exactly); 3: two frames for three
# tokens (no path); 4: the blank as a token (refused); 5: a length beyond the padded width (refused)
TARGETS = [[4, 5, 4, 1], [1, 1, 1, 1], [6, 6, 6, 1], [4, 5, 6, 1], [4, BLANK, 5, 1], [4, 5, 6, 7]]
LENGTHS = [3, 0, 3, 3, 3, 5]
FRAMES = [11, 11, 5, 2, 11, 11]


def test_result_fields_statuses_and_empty_transcripts(calls):
    T, B = 11, 6
    x = _logits(T, B)
    m = ToyModel(x, FRAMES)
    al = CA.CTCAligner(src_dict())
    assert al.blank == BLANK
    sample = _sample(TARGETS, LENGTHS)
    hyps = al.generate([m], sample)
    assert calls == [(torch.float32, (T, B, V), torch.int32, torch.int64, torch.int64, BLANK)]
    assert m.encoder.seen_keys == [["src_lengths", "src_tokens"]], "only the audio keys reach the encoder"
    assert len(hyps) == B and [h[0]["status"] for h in hyps] == [0, 0, 0, 1, 2, 2]
    for b, hs in enumerate(hyps):
        assert len(hs) == 1 and sorted(hs[0]) == KEYS
        h = hs[0]
        L_ = LENGTHS[b] if LENGTHS[b] <= 4 else 0
        assert type(h["status"]) is int and h["attention"] is None and h["alignment"] is None
        assert h["tokens"].dtype == torch.int64 and h["tokens"].tolist() == TARGETS[b][:L_]
        assert torch.is_tensor(h["score"]) and h["score"].dim() == 0 and h["score"].dtype == torch.float32
        assert h["positional_scores"].dtype == torch.float32 and tuple(h["positional_scores"].shape) == (L_,)
        assert h["frames"].dtype == torch.int32 and tuple(h["frames"].shape) == (L_, 2)
        assert h["states"].dtype == torch.int32 and tuple(h["states"].shape) == ((FRAMES[b],) if h["status"] == 0 else (0,))
        if h["status"] == 0:
            r = R.align(x[:, b].numpy(), FRAMES[b], TARGETS[b][:L_], BLANK)
            assert h["states"].tolist() == r["states"].tolist() and h["frames"].tolist() == r["frames"].tolist()
            assert abs(float(h["score"]) - r["score"]) < 1e-4 * max(1, abs(r["score"]))
            assert np.allclose(h["positional_scores"].numpy(), r["tok_score"], atol=1e-4)
        else:
            assert float(h["score"]) == float("-inf")
            assert bool((h["frames"] == -1).all()) and bool(torch.isneginf(h["positional_scores"]).all())
    assert hyps[1][0]["tokens"].numel() == 0 and hyps[1][0]["states"].tolist() == [0] * 11, "the empty transcript: blanks throughout"
    assert hyps[2][0]["states"].tolist() == [1, 2, 3, 4, 5], "at L + repeats frames the path is the only one"
    # no padding mask: every sentence has all T frames; align_logits is the same alignment and takes any integer dtypes
    full = CA.CTCAligner(src_dict()).generate(ToyModel(x, None), sample)
    again = CA.CTCAligner(src_dict()).align_logits(x, torch.tensor([T] * B), torch.tensor(TARGETS, dtype=torch.int32),
                                                   torch.tensor(LENGTHS, dtype=torch.int32))
    for a, c in zip(full, again):
        assert torch.equal(a[0]["states"], c[0]["states"]) and torch.equal(a[0]["score"], c[0]["score"]) and a[0]["status"] == c[0]["status"]
    assert full[3][0]["status"] == 0, "with all 11 frames the three tokens fit"


def test_eval_mode_is_set_and_restored(calls):
    x = _logits(5, 6)
    sample = _sample(TARGETS, LENGTHS)
    for training in (True, False):
        m = ToyModel(x, None, training=training)
        CA.CTCAligner(src_dict()).generate([m], sample)
        assert m.encoder.seen_mode == [False] and m.training is training
    bad = ToyModel(x, None, training=True, fail=True)
    with pytest.raises(RuntimeError, match="encoder failed"):
        CA.CTCAligner(src_dict()).generate(bad, sample)
    assert bad.training is True, "restored after an exception"
    plain = ToyModel(x, None, training=True, compress=False)
    with pytest.raises(ValueError, match="returned no ctc_out"):
        CA.CTCAligner(src_dict()).generate([plain], sample)
    assert plain.training is True and len(calls) == 2


def test_value_errors(calls):
    x = _logits(5, 6)
    sample = _sample(TARGETS, LENGTHS)
    al = CA.CTCAligner(src_dict())
    with pytest.raises(ValueError, match="exactly one model"):
        al.generate([ToyModel(x, None), ToyModel(x, None)], sample)
    with pytest.raises(ValueError, match="exactly one model"):
        al.generate([], sample)
    with pytest.raises(ValueError, match=r"returned no ctc_out \(a model built without --ctc-compress-out\)"):
        al.generate([ToyModel(x, None, compress=False)], sample)
    with pytest.raises(ValueError, match="ctc_blank"):
        CA.CTCAligner(Dictionary.synthetic(5))
    with pytest.raises(ValueError, match="at most %d tokens" % MAX_TARGET):
        al.align_logits(x[:, :1], torch.tensor([5]), torch.zeros(1, MAX_TARGET + 1).long(), torch.tensor([3]))
    assert calls == [], "nothing was aligned"


def test_kernels_ctc_align_checks_its_operands():
    from fbk_fairseq_st_amd import kernels as K
    x = _logits(5, 2)
    n, y, ln = torch.tensor([5, 5], dtype=torch.int32), torch.zeros(2, 3).long(), torch.tensor([3, 3])
    for bad in (lambda: K.ctc_align(x[0], n, y, ln, BLANK), lambda: K.ctc_align(x, n.long(), y, ln, BLANK),
                lambda: K.ctc_align(x, n, y.int(), ln, BLANK), lambda: K.ctc_align(x, n, y[:1], ln, BLANK),
                lambda: K.ctc_align(x, n, y, ln.int(), BLANK), lambda: K.ctc_align(x, n, y, ln[:1], BLANK),
                lambda: K.ctc_align(x, n, torch.zeros(2, MAX_TARGET + 1).long(), ln, BLANK)):
        with pytest.raises(ValueError, match="ctc_align"):
            bad()
    # no frames: decided on the host, nothing is launched
    states, frames, tok, score, status = K.ctc_align(x[:0], n, y, torch.tensor([0, 2]), BLANK)
    assert status.tolist() == [0, 1] and score.tolist() == [0.0, float("-inf")] and tuple(states.shape) == (2, 0)
    assert frames[1, :2].tolist() == [[-1, -1], [-1, -1]] and tok[1, :2].tolist() == [float("-inf")] * 2


def test_input_frames():
    fr = torch.tensor([[[0, 2], [2, 3], [9, 11]], [[1, 4], [-1, -1], [4, 10]]], dtype=torch.int32)
    out = CA.input_frames(fr)
    assert out.dtype == torch.int32 and out.tolist() == [[[0, 8], [8, 12], [36, 44]], [[4, 16], [-1, -1], [16, 40]]]
    out = CA.input_frames(fr, torch.tensor([42, 38]))
    assert out.tolist() == [[[0, 8], [8, 12], [36, 42]], [[4, 16], [-1, -1], [16, 38]]], "clipped to each utterance's length"
    assert CA.input_frames(fr[0], 41).tolist() == [[0, 8], [8, 12], [36, 41]]
    assert CA.SUBSAMPLING == 4
