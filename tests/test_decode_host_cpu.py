"""Host logic of the device-resident beam search (fbk_fairseq_st_amd/decode.py): rebuilding the hypotheses from the per-step selection
records.  The records are produced here by a numpy re-enactment of the reference's bookkeeping (fairseq/sequence_generator.py:417-446:
the tokens / scores buffers re-ordered by the chosen parents every step), so the walk over parent links must give back exactly the
buffers' rows."""
import numpy as np
import pytest

from fbk_fairseq_st_amd.decode import _pick_hidden_slice, walk_records


def test_walk_records_rebuilds_the_reordered_buffers():
    rs = np.random.RandomState(5)
    B, beam, steps, V, pad, eos = 3, 4, 9, 50, 1, 2
    N = B * beam
    tokens = np.full((N, steps + 2), pad, np.int64); tokens[:, 0] = eos
    scores = np.zeros((N, steps + 1), np.float32)
    origin = np.tile(np.arange(beam), B)
    tok_h = np.zeros((steps + 2, N), np.int32); par_h = np.zeros((steps + 2, N), np.int32); cum_h = np.zeros((steps + 2, N), np.float32)
    nfin = np.zeros(B, np.int32); fin_step = np.zeros((B, beam), np.int32); fin_row = np.zeros((B, beam), np.int32)
    fin_score = np.zeros((B, beam), np.float32)
    expected = [[] for _ in range(B)]
    for t in range(steps + 1):
        # some hypotheses end at this step (finalised from the arrangement BEFORE the re-ordering, as the reference does)
        for s in range(B):
            if rs.rand() < 0.35 and nfin[s] < beam:
                r = s * beam + rs.randint(beam)
                sc = np.float32(scores[r, t - 1] - rs.rand()) if t else np.float32(-rs.rand())
                k = nfin[s]
                fin_step[s, k], fin_row[s, k], fin_score[s, k] = t, r, sc
                nfin[s] += 1
                cum = np.concatenate([scores[r, :t], [sc]]).astype(np.float32)
                pos = cum.copy(); pos[1:] = cum[1:] - cum[:-1]
                expected[s].append((np.concatenate([tokens[r, 1:t + 1], [eos]]), pos, sc / np.float32((t + 1) ** 0.8), origin[r]))
        if t == steps:
            break
        parent = (np.arange(B)[:, None] * beam + rs.randint(beam, size=(B, beam))).reshape(-1)
        newtok = rs.randint(4, V, size=N)
        newsc = (scores[parent, t - 1] if t else 0) - rs.rand(N).astype(np.float32)
        tokens[:, :t + 1] = tokens[parent, :t + 1]; tokens[:, t + 1] = newtok
        scores[:, :t] = scores[parent, :t]; scores[:, t] = newsc
        origin = origin[parent]
        tok_h[t + 1], par_h[t + 1], cum_h[t + 1] = newtok, parent, newsc
    sent, tok, pos, score, org, length = walk_records(tok_h, par_h, cum_h, nfin, fin_step, fin_row, fin_score, beam, pad, eos, True, 0.8)
    assert sent.shape[0] == int(nfin.sum()) > 0
    seen = [0] * B
    for f in range(sent.shape[0]):
        s = int(sent[f]); et, ep, es, eo = expected[s][seen[s]]; seen[s] += 1
        n = int(length[f])
        assert tok[f, :n].tolist() == et.tolist()
        np.testing.assert_array_equal(pos[f, :n], ep)
        assert score[f] == es and int(org[f]) == int(eo)


@pytest.mark.parametrize("seed,B,beam,V,max_len,min_len,unk_pen,temp,eos_scale,lenpen", [
    (1, 2, 3, 11, 6, 1, 0.0, 1.0, 4.0, 1.0),           # EOS-rich: sentences finalise at different steps, slots get black-listed
    (2, 3, 2, 9, 5, 3, 0.5, 1.3, 3.0, 0.7),            # min_len, unk penalty, temperature
    (3, 1, 4, 9, 4, 4, 0.0, 1.0, 1.0, 1.0),            # min_len = max_len: every hypothesis ends at the forced-EOS step; V = 2 beam + 1
    (4, 2, 1, 13, 7, 1, 0.0, 0.8, 5.0, 1.0),           # beam 1
])
def test_restated_bookkeeping_reproduces_the_oracle_search(seed, B, beam, V, max_len, min_len, unk_pen, temp, eos_scale, lenpen):
    """tests/decode_ref.sent_step (the GPU test's restatement of dec_sent_kernel) driven by oracle/s2t_ref.py's own fp32 log-probs:
    every row's 2 beam best (value descending, column ascending), then the restated merge / finalisation / next beam; the records
    walked back by decode.walk_records must give s2t_ref's hypotheses (tokens exact, scores to f32 rounding)."""
    import math
    import torch
    import decode_ref as R
    from oracle import s2t_ref
    D, pad, eos, unk = 64, 1, 2, 3
    cfg = s2t_ref.default_cfg(D=D, heads=1, ffn=64, enc_layers=0, dec_layers=1)
    W = s2t_ref.make_weights({k: v for k, v in s2t_ref.param_shapes(cfg, 8, V).items() if k.startswith("decoder.")}, seed)
    W["decoder.output_projection.weight"][eos] *= eos_scale
    rs = np.random.RandomState(seed)
    n = [int(v) for v in rs.randint(3, 9, size=B)]
    eo = [torch.from_numpy(rs.randn(n[b], 1, D).astype(np.float32)) for b in range(B)]
    N, K2 = B * beam, 2 * beam
    st = R.new_state(B, beam, max_len, eos)
    prefix = [[eos] for _ in range(N)]
    for t in range(max_len + 1):
        if bool(st["finished"].all()):
            break
        cand_val = np.full((N, K2), -np.inf, np.float32)
        cand_idx = np.tile(np.arange(K2, dtype=np.int32), (N, 1))     # idle slots of the first step: -inf in column order
        for b in range(B):
            toks = torch.tensor([prefix[b * beam + j] for j in range(beam)], dtype=torch.long)
            lp = torch.log_softmax(s2t_ref.decoder_forward(W, cfg, toks, eo[b].expand(n[b], beam, D), None)[:, -1, :] / temp, dim=-1)
            lp[lp != lp] = -math.inf
            lp[:, pad] = -math.inf
            lp[:, unk] -= unk_pen
            if t >= max_len:
                keep = lp[:, eos].clone(); lp[:] = -math.inf; lp[:, eos] = keep
            elif t < min_len:
                lp[:, eos] = -math.inf
            for j in range(beam if t > 0 else 1):
                r = b * beam + j
                v = (lp[j] + torch.from_numpy(st["cum_hist"][t, r:r + 1])).numpy() if t > 0 else lp[j].numpy()
                order = np.lexsort((np.arange(V), -v.astype(np.float64)))[:K2]
                cand_val[r], cand_idx[r] = v[order], order
        R.sent_step(st, cand_val, cand_idx, beam, V, eos, max_len, False)
        prefix = [prefix[int(st["par_hist"][t + 1, r])] + [int(st["tok_hist"][t + 1, r])] for r in range(N)]
    sent, tok, pos, score, _, length = walk_records(st["tok_hist"], st["par_hist"], st["cum_hist"], st["nfin"], st["fin_step"],
                                                    st["fin_row"], st["fin_score"], beam, pad, eos, True, lenpen)
    for b in range(B):
        exp = s2t_ref._beam_search_sentence(W, cfg, eo[b], n[b], beam, max_len, min_len, lenpen, unk_pen, temp, True, eos, unk)
        mine = [f for f in range(sent.shape[0]) if int(sent[f]) == b]
        mine = [mine[i] for i in reversed(sorted(range(len(mine)), key=lambda i: float(score[mine[i]])))]
        assert len(mine) == len(exp) == beam
        for f, (et, esc, eps, _) in zip(mine, exp):
            assert tok[f, :int(length[f])].tolist() == et.tolist()
            assert abs(float(score[f]) - esc) <= 1e-5 * max(1.0, abs(esc))
            np.testing.assert_allclose(pos[f, :int(length[f])], eps.numpy(), rtol=0, atol=1e-5)


def test_hidden_slice_choice():
    assert _pick_hidden_slice(2048, 16) == 128 and _pick_hidden_slice(2048, 1) == 64 and _pick_hidden_slice(768, 16) in (64, 128, 256)
    assert _pick_hidden_slice(100, 4) == 0


def test_implicit_attention_request_is_dropped_for_long_inputs():
    """eval-mode forwards return the encoder attention by default (transformer.py:700-703), but a source longer than the
    attention-probability kernel takes must not make validation / generation fail when nobody asked for the attention"""
    import types
    from fbk_fairseq_st_amd.conv_transformer import TransformerDecoder
    dec = TransformerDecoder.__new__(TransformerDecoder)
    dec.owner = types.SimpleNamespace(hp=types.SimpleNamespace(dec_layers=6))
    dec.training = False
    assert dec._alignment_request(None, None, None, src_frames=375) == (5, None)
    assert dec._alignment_request(None, None, None, src_frames=4000) == (None, None)          # implicit: dropped
    assert dec._alignment_request(None, None, True, src_frames=4000) == (5, None)             # asked for: kept (the kernel will refuse)
    assert dec._alignment_request(2, 4, None, src_frames=4000) == (2, 4)
    dec.training = True
    assert dec._alignment_request(None, None, None, src_frames=100) == (None, None)
