"""The CTC decoders without a GPU: the new entry points are exported, bound and refuse bad arguments before anything is launched, and
the host logic of CTCDecoder -- result keys and dtypes, empty transcripts, eval mode and its restoration, the refusals -- with the two
kernels.py calls replaced by the float64 reference (tests/ctc_decode_ref.py; the kernels have their own tests)."""
import ctypes

import pytest
import torch

import ctc_decode_ref as R
from fbk_fairseq_st_amd import ctc_decoder as CD
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd.data import Dictionary
from fbk_fairseq_st_amd.registry import CTCAwareEncoderOut, EncoderOut

NEW = ("s2t_ctc_greedy_workspace", "s2t_ctc_greedy", "s2t_ctc_prefix_beam_workspace", "s2t_ctc_prefix_beam")
FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing


def test_exports_bindings_and_workspace_sizes():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name)
    assert "s2t_ctc_greedy_workspace" in L._SIZE_T_RESULT and "s2t_ctc_prefix_beam_workspace" in L._SIZE_T_RESULT
    assert len(L.SIGNATURES["s2t_ctc_greedy"]) == 15 and len(L.SIGNATURES["s2t_ctc_prefix_beam"]) == 17
    assert lib.s2t_abi_version() == 9
    assert lib.s2t_ctc_greedy_workspace(375, 16) == 8 * 375 * 16 and lib.s2t_ctc_greedy_workspace(0, 16) == 0
    T, B, beam, cand = 375, 16, 16, 16
    assert lib.s2t_ctc_prefix_beam_workspace(T, B, beam, cand, 4) == (4 * T * B * (2 * beam + 2 * cand + 1) + 255) // 256 * 256
    # the trie of a sentence holds T * beam (parent, token) nodes
    assert lib.s2t_ctc_prefix_beam_workspace(7, 3, 5, 2, 1) >= 8 * 7 * 3 * 5 + 4 * 7 * 3 * (2 * 2 + 1)


def test_refusals_before_any_launch():
    lib = L.load()
    g = lambda **kw: lib.s2t_ctc_greedy(*[kw.get(k, d) for k, d in (
        ("dtype", 0), ("logits", FAKE), ("in_len", FAKE), ("ws", FAKE), ("tokens", FAKE), ("n", FAKE), ("frames", FAKE), ("tok_score", FAKE),
        ("score", FAKE), ("T", 4), ("B", 2), ("V", 12), ("ld", 12), ("blank", 11), ("stream", None))])
    p = lambda **kw: lib.s2t_ctc_prefix_beam(*[kw.get(k, d) for k, d in (
        ("dtype", 0), ("logits", FAKE), ("in_len", FAKE), ("ws", FAKE), ("tokens", FAKE), ("lens", FAKE), ("scores", FAKE), ("n_hyp", FAKE),
        ("T", 4), ("B", 2), ("V", 12), ("ld", 12), ("blank", 11), ("beam", 4), ("cand", 4), ("nbest", 1), ("stream", None))])
    for f, ptrs in ((g, ("logits", "in_len", "ws", "tokens", "n", "frames", "tok_score", "score")),
                    (p, ("logits", "in_len", "ws", "tokens", "lens", "scores", "n_hyp"))):
        for name in ptrs:
            assert f(**{name: None}) == -22, name                    # null pointers
        assert f(ld=11) == -22 and f(blank=12) == -22 and f(blank=-1) == -22 and f(V=1, ld=1, blank=0) == -22
        assert f(dtype=2) == -95
        assert f(T=0) == 0 and f(B=0) == 0 and f(T=0, logits=None) == 0      # an empty problem: nothing to do, nothing looked at
    assert p(beam=17) == -95 and p(cand=17, V=100, ld=100) == -95
    assert p(cand=12, V=12) == -95, "cand = V: at most V - 1 non-blank symbols exist"
    assert p(beam=0) == -22 and p(cand=0) == -22 and p(nbest=0) == -22 and p(beam=4, nbest=5) == -22


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        getattr(raw, name).argtypes = L.SIGNATURES[name]
    for name in ("s2t_ctc_greedy_workspace", "s2t_ctc_prefix_beam_workspace"):
        getattr(raw, name).restype = ctypes.c_size_t
    calls = [("s2t_ctc_greedy_workspace", (1 << 20, 4096)), ("s2t_ctc_prefix_beam_workspace", (1 << 20, 64, 16, 16, 16)),
             ("s2t_ctc_greedy", (0, None, None, None, None, None, None, None, None, 4, 2, 12, 12, 11, None)),
             ("s2t_ctc_prefix_beam", (0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 2, 12, 12, 11, 17, 4, 1, None))]
    for name, args in calls:
        assert getattr(fast, name)(*args) == getattr(raw, name)(*args), name
    assert fast.s2t_ctc_greedy_workspace(1 << 20, 4096) == 8 << 32, "a size_t result, not an int"


# ------------------------------------------------------------------ host logic
V = 9


def src_dict():
    d = Dictionary.synthetic(V - 5)                                   # 4 specials + (V - 5) words + the blank = V entries
    d.add_symbol("<ctc_blank>")
    assert len(d) == V
    return d


def _greedy_standin(calls):
    def ctc_greedy(logits, in_len, blank):
        calls.append(("greedy", logits.dtype, tuple(logits.shape), blank))
        T, B, _ = logits.shape
        tokens = torch.full((B, T), -7, dtype=torch.int32)
        frames = torch.full((B, T, 2), -7, dtype=torch.int32)
        tok_score = torch.full((B, T), float("nan"))
        n, score = torch.zeros(B, dtype=torch.int32), torch.zeros(B)
        for b in range(B):
            tk, fr, ts, sc = R.greedy(logits[:, b].float().numpy(), int(in_len[b]), blank)
            n[b], score[b] = len(tk), sc
            tokens[b, :len(tk)] = torch.tensor(tk, dtype=torch.int32)
            frames[b, :len(tk)] = torch.tensor(fr, dtype=torch.int32).reshape(-1, 2)
            tok_score[b, :len(tk)] = torch.tensor(ts)
        return tokens, n, frames, tok_score, score
    return ctc_greedy


def _prefix_standin(calls):
    def ctc_prefix_beam(logits, in_len, blank, beam, cand, nbest):
        calls.append(("prefix", beam, cand, nbest))
        T, B, _ = logits.shape
        tokens = torch.full((B, nbest, T), -7, dtype=torch.int32)
        lens = torch.zeros((B, nbest), dtype=torch.int32)
        scores = torch.full((B, nbest), float("-inf"))
        n_hyp = torch.zeros(B, dtype=torch.int32)
        for b in range(B):
            hyps = R.prefix_beam(logits[:, b].float().numpy(), int(in_len[b]), blank, beam, cand, nbest)["hyps"]
            n_hyp[b] = len(hyps)
            for i, (s, tot) in enumerate(hyps):
                lens[b, i], scores[b, i] = len(s), tot
                tokens[b, i, :len(s)] = torch.tensor(s, dtype=torch.int32)
        return tokens, lens, scores, n_hyp
    return ctc_prefix_beam


@pytest.fixture
def calls(monkeypatch):
    c = []
    monkeypatch.setattr(CD.K, "ctc_greedy", _greedy_standin(c))
    monkeypatch.setattr(CD.K, "ctc_prefix_beam", _prefix_standin(c))
    return c


def _logits(T, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, V, generator=g) * 3
    x[:, 1] = -4.0
    x[:, 1, V - 1] = 4.0                                              # sentence 1: blank on every frame
    return x


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


def _sample(B):
    return dict(net_input=dict(src_tokens=torch.zeros(B, 40, 80), src_lengths=torch.full((B,), 40), prev_output_tokens=torch.zeros(B, 3).long(),
                               transcript_prev_output_tokens=torch.zeros(B, 3).long()), target=torch.zeros(B, 3).long())


KEYS = ["alignment", "attention", "frames", "positional_scores", "score", "tokens"]


def test_greedy_result_fields_and_empty_transcripts(calls):
    T, B, lens = 11, 3, [11, 11, 4]
    x = _logits(T, B)
    m = ToyModel(x, lens)
    dec = CD.CTCDecoder(src_dict())
    assert dec.blank == V - 1
    hyps = dec.generate([m], _sample(B))
    assert calls == [("greedy", torch.float32, (T, B, V), V - 1)]
    assert m.encoder.seen_keys == [["src_lengths", "src_tokens"]], "only the audio keys reach the encoder"
    assert len(hyps) == B
    for b, hs in enumerate(hyps):
        tk, fr, ts, sc = R.greedy(x[:, b].numpy(), lens[b], V - 1)
        assert len(hs) == 1 and sorted(hs[0]) == KEYS
        h = hs[0]
        assert h["tokens"].dtype == torch.int64 and h["tokens"].tolist() == tk and V - 1 not in tk
        assert torch.is_tensor(h["score"]) and h["score"].dim() == 0 and h["score"].dtype == torch.float32 and abs(float(h["score"]) - sc) < 1e-4
        assert h["positional_scores"].dtype == torch.float32 and h["positional_scores"].shape == (len(tk),)
        assert torch.allclose(h["positional_scores"].double(), torch.tensor(ts, dtype=torch.float64).reshape(-1), atol=1e-5)
        assert h["frames"].dtype == torch.int32 and tuple(h["frames"].shape) == (len(tk), 2) and h["frames"].tolist() == [list(f) for f in fr]
        assert h["attention"] is None and h["alignment"] is None
    assert hyps[1][0]["tokens"].numel() == 0 and tuple(hyps[1][0]["frames"].shape) == (0, 2), "an all-blank sentence: the empty transcript"
    assert all(int(h[0]["frames"].max()) <= n for h, n in zip(hyps, lens) if h[0]["frames"].numel())
    # no padding mask: every sentence has all T frames; decode_logits is the same decoding
    full = CD.CTCDecoder(src_dict()).generate(ToyModel(x, None), _sample(B))
    again = CD.CTCDecoder(src_dict()).decode_logits(x, torch.tensor([T] * B))
    for a, c in zip(full, again):
        assert torch.equal(a[0]["tokens"], c[0]["tokens"]) and torch.equal(a[0]["score"], c[0]["score"])


def test_prefix_result_fields(calls):
    T, B, lens = 9, 3, [9, 9, 0]
    x = _logits(T, B, seed=3)
    dec = CD.CTCDecoder(src_dict(), strategy="prefix", beam_size=4, cand=16, nbest=3)
    hyps = dec.generate(ToyModel(x, lens), _sample(B))
    assert calls == [("prefix", 4, V - 1, 3)], "cand is capped at the V - 1 non-blank symbols"
    for b, hs in enumerate(hyps):
        want = R.prefix_beam(x[:, b].numpy(), lens[b], V - 1, 4, V - 1, 3)["hyps"]
        assert len(hs) == len(want)
        for h, (s, tot) in zip(hs, want):
            assert sorted(h) == KEYS and h["tokens"].dtype == torch.int64 and h["tokens"].tolist() == list(s)
            assert h["score"].dim() == 0 and h["score"].dtype == torch.float32 and abs(float(h["score"]) - tot) < 1e-4 * max(1, abs(tot))
            assert h["positional_scores"] is None and h["frames"] is None and h["attention"] is None and h["alignment"] is None
    assert len(hyps[2]) == 1 and hyps[2][0]["tokens"].numel() == 0 and float(hyps[2][0]["score"]) == 0.0, "no frames: the empty hypothesis"


def test_eval_mode_is_set_and_restored(calls):
    x = _logits(5, 3)
    for training in (True, False):
        m = ToyModel(x, None, training=training)
        CD.CTCDecoder(src_dict()).generate([m], _sample(3))
        assert m.encoder.seen_mode == [False] and m.training is training
    bad = ToyModel(x, None, training=True, fail=True)
    with pytest.raises(RuntimeError, match="encoder failed"):
        CD.CTCDecoder(src_dict()).generate(bad, _sample(3))
    assert bad.training is True, "restored after an exception"
    plain = ToyModel(x, None, training=True, compress=False)
    with pytest.raises(ValueError, match="decode_logits"):
        CD.CTCDecoder(src_dict()).generate([plain], _sample(3))
    assert plain.training is True and calls and all(c[0] == "greedy" for c in calls)


def test_value_errors(calls):
    x = _logits(5, 3)
    dec = CD.CTCDecoder(src_dict())
    with pytest.raises(ValueError, match="exactly one model"):
        dec.generate([ToyModel(x, None), ToyModel(x, None)], _sample(3))
    with pytest.raises(ValueError, match="exactly one model"):
        dec.generate([], _sample(3))
    with pytest.raises(ValueError, match="decode_logits"):
        dec.generate([ToyModel(x, None, compress=False)], _sample(3))
    with pytest.raises(ValueError, match="nbest"):
        CD.CTCDecoder(src_dict(), strategy="greedy", nbest=2)
    with pytest.raises(ValueError, match="strategy"):
        CD.CTCDecoder(src_dict(), strategy="viterbi")
    with pytest.raises(ValueError, match="beam_size"):
        CD.CTCDecoder(src_dict(), strategy="prefix", beam_size=17)
    with pytest.raises(ValueError, match="beam_size"):
        CD.CTCDecoder(src_dict(), strategy="prefix", beam_size=2, nbest=3)
    with pytest.raises(ValueError, match="ctc_blank"):
        CD.CTCDecoder(Dictionary.synthetic(5))
    assert calls == [], "nothing was decoded"
