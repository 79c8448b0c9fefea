"""Host side of the device search's two S2TDecodeExtras options -- hypothesis attention and --layernorm-embedding models -- where there
is no GPU: the ABI of the three *_ex calls (exported, bound twice, refusing in the documented order), the row walk that tells
`hypotheses` where a hypothesis' attention records lie, and the generator's routing (stand-in decoders; the sessions are recorders)."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from fbk_fairseq_st_amd import decode as DEC
from fbk_fairseq_st_amd import lib as L

PAD, EOS, UNK = 1, 2, 3
EINVAL, ENOTSUP = -22, -95
NEW = ("s2t_decode_begin_ex", "s2t_decode_step_ex", "s2t_decode_graph_create_ex")


# ------------------------------------------------------------------ ABI
def _bindings():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    L.load()
    return [("ctypes", L.load_ctypes()), ("fastcall", fast)]


def test_new_symbols_abi_version_and_struct_sizes():
    assert L.load().s2t_abi_version() == 9 and L.ABI_VERSION == 9
    assert ctypes.sizeof(L.DecodeDesc) == L.DecodeDesc.diverse_groups.offset + 8
    assert ctypes.sizeof(L.DecodeRules) == 16 and ctypes.sizeof(L.DecodeSample) == 16
    assert ctypes.sizeof(L.DecodeExtras) == 18 * 8 and L.DecodeExtras.lne_b.offset == 64 and L.DecodeExtras.attn_part.offset == 128
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(raw, name)
        for what, b in _bindings():
            assert hasattr(b, name), (what, name)
    assert L.SIGNATURES["s2t_decode_step_ex"] == [L.P, ctypes.c_int, L.P, L.P, L.P, L.P]


def test_ex_calls_refuse_in_the_documented_order():
    """on a zeroed descriptor (outside the limits: S2T_ENOTSUP, looked at last) no call launches anything; both bindings agree"""
    ex = ctypes.c_void_p(0)
    exa = ctypes.addressof(ex)
    A = ctypes.addressof
    buf = (ctypes.c_float * 4)()
    p = A(buf)
    for what, b in _bindings():
        d = L.DecodeDesc()
        arr = (ctypes.c_void_p * 1)(A(d))
        aa = A(arr)
        pair = [L.DecodeDesc(), L.DecodeDesc()]
        parr = (ctypes.c_void_p * 2)(*[A(q) for q in pair])
        ok_s, bad_s = L.DecodeSample(), L.DecodeSample()
        ok_s.topk, bad_s.topk = 5, -1
        r1, rneg = L.DecodeRules(), L.DecodeRules()
        r1.no_repeat_ngram, rneg.no_repeat_ngram = 1, -1

        def X(**kw):
            x = L.DecodeExtras()
            for k, v in kw.items():
                if k in ("attn_part", "attn_hist"):
                    setattr(x, k, v)
                else:
                    getattr(x, k[:5])[int(k[5:])] = v              # lne_g3=p -> x.lne_g[3]
            return x

        def all3(dv, n, r, s, x):
            xa = A(x) if x is not None else None
            got = (b.s2t_decode_begin_ex(dv, n, r, s, xa, EOS, None), b.s2t_decode_step_ex(dv, n, r, s, xa, None),
                   b.s2t_decode_graph_create_ex(dv, n, r, s, xa, 8, exa))
            assert ex.value is None and got[0] == got[1] == got[2], (what, got)
            return got[0]
        # 1. the extras on their own: a pointer of a pair without the other, for the attention and for any member
        assert all3(None, 1, None, None, X(attn_part=p)) == EINVAL and all3(aa, 1, None, None, X(attn_hist=p)) == EINVAL
        assert all3(aa, 1, A(r1), None, X(lne_g0=p)) == EINVAL and all3(aa, 1, None, A(bad_s), X(lne_b7=p)) == EINVAL
        # 2. attention with more than one member, before the members are looked at
        assert all3(A(parr), 2, A(rneg), None, X(attn_part=p, attn_hist=p)) == ENOTSUP
        assert all3(A(parr), 2, None, A(bad_s), X(attn_part=p, attn_hist=p, lne_g1=p, lne_b1=p)) == ENOTSUP
        # 3. then what s2t_decode_step_sample (s given) or s2t_decode_step_ensemble checks, in their order, with every kind of x
        pair[1].beam = 3
        for x in (None, X(), X(lne_g0=p, lne_b0=p), X(attn_part=p, attn_hist=p), X(attn_part=p, attn_hist=p, lne_g0=p, lne_b0=p)):
            attn = x is not None and bool(x.attn_part)
            assert all3(aa, 1, A(r1), A(bad_s), x) == EINVAL                    # the sample struct first
            assert all3(None, 1, None, None, x) == EINVAL and all3(aa, 0, None, A(ok_s), x) == EINVAL
            assert all3(aa, 9, A(r1), None, x) == (ENOTSUP if attn else EINVAL)
            assert all3(aa, 1, A(rneg), None, x) == EINVAL and all3(aa, 1, A(r1), A(ok_s), x) == ENOTSUP
            assert all3(A(parr), 2, None, None, x) == (ENOTSUP if attn else EINVAL)       # members that disagree on the beam
            dneg = L.DecodeDesc()
            dneg.diverse_groups = -1
            assert all3(A((ctypes.c_void_p * 1)(A(dneg))), 1, None, None, x) == EINVAL
            assert all3(aa, 1, None, None, x) == ENOTSUP and all3(aa, 1, None, A(ok_s), x) == ENOTSUP
        # graph_exec and n_steps before everything
        bad = X(attn_part=p)
        assert b.s2t_decode_graph_create_ex(aa, 1, None, None, A(bad), 8, None) == EINVAL
        assert b.s2t_decode_graph_create_ex(aa, 1, None, None, None, 0, exa) == EINVAL
        assert b.s2t_decode_graph_create_ex(aa, 1, None, None, None, 65, exa) == EINVAL


# ------------------------------------------------------------------ the row walk
def _random_records(rs):
    """a random but consistent record set: every slot of every arrangement has a parent in its own sentence; sentences finalise
    1..beam hypotheses at ragged steps"""
    beam, B = int(rs.randint(1, 7)), int(rs.randint(1, 4))
    max_len = int(rs.randint(1, 12))
    N, M2 = B * beam, max_len + 2
    tok_h = rs.randint(4, 50, (M2, N)).astype(np.int32)
    cum_h = rs.randn(M2, N).astype(np.float32)
    par_h = np.zeros((M2, N), np.int32)
    for i in range(1, M2):
        for s in range(B):
            par_h[i, s * beam:(s + 1) * beam] = s * beam + rs.randint(0, beam, beam)
    nfin = rs.randint(0, beam + 1, B).astype(np.int32)
    fin_step = rs.randint(0, max_len + 1, (B, beam)).astype(np.int32)
    fin_row = np.stack([s * beam + rs.randint(0, beam, beam) for s in range(B)]).astype(np.int32)
    fin_score = rs.randn(B, beam).astype(np.float32)
    return beam, B, max_len, tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score


def test_slot_walk_against_a_per_hypothesis_parent_walk():
    rs = np.random.RandomState(5)
    seen_ragged = 0
    for _ in range(200):
        beam, B, max_len, tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score = _random_records(rs)
        args = (tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score, beam, PAD, EOS, True, 1.0)
        sent, tok, pos, score, origin, length, slots = DEC.walk_records_slots(*args)
        old = DEC.walk_records(*args)
        assert len(old) == 6
        for a, b in zip(old, (sent, tok, pos, score, origin, length)):
            assert np.array_equal(a, b)
        f = 0
        steps = set()
        for s in range(B):
            for k in range(int(nfin[s])):
                st, row = int(fin_step[s, k]), int(fin_row[s, k])
                steps.add(st)
                want_slot, want_tok = [0] * (st + 1), [0] * (st + 1)
                want_slot[st], want_tok[st] = row, EOS
                for i in range(st, 0, -1):                              # this hypothesis alone, link by link
                    want_tok[i - 1] = int(tok_h[i][row])
                    row = int(par_h[i][row])
                    want_slot[i - 1] = row
                assert int(sent[f]) == s and int(length[f]) == st + 1
                assert slots[f, :st + 1].tolist() == want_slot and tok[f, :st + 1].tolist() == want_tok
                assert all(s * beam <= v < (s + 1) * beam for v in want_slot)
                assert not slots[f, st + 1:].any()
                assert int(origin[f]) == want_slot[0] % beam
                f += 1
        assert f == sent.shape[0] and slots.shape == tok.shape
        seen_ragged += len(steps) > 1
    assert seen_ragged > 100, "the record sets were meant to finish at ragged steps"


# ------------------------------------------------------------------ routing
class _Dict:
    def __init__(self, V):
        self.V = V

    def pad(self):
        return PAD

    def unk(self):
        return UNK

    def eos(self):
        return EOS

    def __len__(self):
        return self.V


class _Enc:
    """an encoder output that says it lives on the device (the stand-in engine's tensors are host tensors, which the device route leaves
    to the step route before it looks at anything else)"""

    def __init__(self, t):
        self.t, self.is_cuda, self.shape, self.device = t, True, t.shape, t.device

    def contiguous(self):
        return self


class _ToyDecoder:
    def __init__(self, V, seed, lne=False):
        self.table = torch.from_numpy(np.random.RandomState(seed).randn(V, V).astype(np.float32) * 2)
        self.table[:, EOS] = 3.0
        enc = types.SimpleNamespace(reorder_encoder_out=lambda e, order: e)
        self.owner = types.SimpleNamespace(training=False, encoder=enc, hp=types.SimpleNamespace(dec_layers=1))
        self.engine = types.SimpleNamespace(hp=types.SimpleNamespace(layernorm_embedding=lne), dtype=torch.float32)
        self.pfx = "decoder."

    def begin_incremental(self, enc, n):
        return {"attn": None}

    def reorder_incremental(self, st, order):
        pass

    def step_incremental(self, st, last):
        return self.table[last].clone()


def _route(monkeypatch, n_dec, lne=False, **gen_kw):
    """run _beam_search over stand-in decoders with recorder sessions that refuse (ok False: the step route then serves the search);
    returns the sessions that were built as (class name, engines, keyword arguments)"""
    from cpu_stubs import cpu_kernels
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    V, B, beam, max_len = 40, 2, 3, 6
    built = []

    def recorder(name):
        class Ses:
            ok = False

            def __init__(self, *a, **kw):
                engines = [a[0]] if name == "beam" else [m[0] for m in a[0]]
                built.append((name, engines, kw))
        return Ses
    monkeypatch.setattr(DEC, "BeamDecodeSession", recorder("beam"))
    monkeypatch.setattr(DEC, "EnsembleDecodeSession", recorder("ensemble"))
    monkeypatch.setattr(K, "ensemble_lse", lambda ms: torch.logsumexp(torch.stack(ms), 0) - math.log(len(ms)))
    monkeypatch.delenv("S2T_DEVICE_SEARCH", raising=False)
    model = types.SimpleNamespace(training=False, eval=lambda: None, train=lambda t=True: None, max_decoder_positions=lambda: 1024)
    gen = SequenceGenerator([model] * n_dec, _Dict(V), beam_size=beam, max_len_b=max_len, **gen_kw)
    decs = [_ToyDecoder(V, 1 + j, lne) for j in range(n_dec)]
    encs = [types.SimpleNamespace(encoder_out=_Enc(torch.zeros(5, B, 8)), encoder_padding_mask=None, src_lengths=None) for _ in decs]
    with cpu_kernels():
        hyps = gen._beam_search(decs if n_dec > 1 else decs[0], encs if n_dec > 1 else encs[0], B, torch.device("cpu"), max_len,
                                gen.search, None, PAD, UNK, EOS, V)
    assert len(hyps) == B and all(len(hs) == beam for hs in hyps), "the step route served the search the recorder refused"
    assert "launches_per_step" not in gen.last_stats
    return built, decs


def test_one_decoder_with_print_alignment_asks_for_an_attention_session(monkeypatch):
    built, decs = _route(monkeypatch, 1, print_alignment=True)
    assert len(built) == 1 and built[0][0] == "beam" and built[0][1] == [decs[0].engine]
    assert built[0][2]["retain_attention"] is True
    built, _ = _route(monkeypatch, 1)
    assert len(built) == 1 and built[0][2]["retain_attention"] is False


def test_two_decoders_with_attention_build_no_session(monkeypatch):
    built, _ = _route(monkeypatch, 2, retain_attention=True)
    assert built == []
    built, _ = _route(monkeypatch, 2)
    assert len(built) == 1 and built[0][0] == "ensemble" and "retain_attention" not in built[0][2]


def test_layernorm_embedding_engines_build_sessions(monkeypatch):
    built, decs = _route(monkeypatch, 1, lne=True)
    assert len(built) == 1 and built[0][0] == "beam" and built[0][1][0].hp.layernorm_embedding
    built, _ = _route(monkeypatch, 2, lne=True)
    assert len(built) == 1 and built[0][0] == "ensemble" and all(e.hp.layernorm_embedding for e in built[0][1])


def test_session_refuses_before_it_allocates():
    """attention for two members, and records beyond the cap: `ok` False with no member built (nothing was allocated)"""
    hp = types.SimpleNamespace(layernorm_embedding=False)
    eng = types.SimpleNamespace(hp=hp, dtype=torch.float32, dev=torch.device("cpu"))
    enc = torch.zeros(4, 2, 256)
    two = DEC.EnsembleDecodeSession([(eng, "decoder.", enc, None)] * 2, 2, 8, 1, PAD, UNK, EOS, 96, retain_attention=True)
    assert two.ok is False and two.members == [] and two.attn_hist is None
    big = torch.zeros(1, 1, 256).expand(4096, 8, 256)                          # Ts 4096 x N 128 x 1024 steps x 4 bytes = 2 GiB
    over = DEC.BeamDecodeSession(eng, "decoder.", big, None, 16, 1023, 1, PAD, UNK, EOS, 96, retain_attention=True)
    assert over.ok is False and over.members == [] and over.attn_hist is None
    assert (1023 + 1) * 128 * 4096 * 4 > DEC.ATTN_HIST_CAP == 1 << 30
