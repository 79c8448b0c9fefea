"""chrF's n-gram matching held to BLEU's on the GPU: csrc/chrf_stats.hip holds its own loops for the rule that
csrc/ngram_match.hpp states and csrc/bleu_stats.hip takes its loops from, and nothing else ties the two.
With a piece table in which token t is the one code point 93 + t without a break, a row's characters are its tokens, so the
character statistics of the orders 1 to 4 are BLEU's: the same clipped matches, the same totals.  pad and eos lie outside the tokens
used (nothing is trimmed) and unk is off.  The identity belongs to the rule -- tests/bleu_ref.py and tests/chrf_ref.py agree on every
pair used here (tests/ngram_cases.py), which tests/test_chrf_ref_cpu.py checks without a GPU -- so each side is also compared with
its own reference; all of it is exact integers.
Hypothesis lengths sit on both sides of the 64- and 256-position boundaries of both kernels' waves and workgroups, and the three calls
have padded widths of 64, 256 and 257 tokens: BLEU's one-wave, 256-thread and 1,024-thread forms, chrF's 256- and 1,024-thread forms.
Rows are padded behind their lengths with tokens of the alphabet, the same on both sides: a read past a length would find matches."""
import numpy as np
import pytest
import torch

from ngram_cases import EOS, FIRST, HYP_LENS, PAD, REF_LENS, V, case

pytestmark = pytest.mark.gpu

DEV = "cuda"


def padded(rows, dtype):
    width = max(len(r) for r in rows)
    out = np.empty((len(rows), width), dtype)
    for s, r in enumerate(rows):
        out[s] = [FIRST + (s + i) % 2 for i in range(width)]
        out[s, :len(r)] = r
    return torch.from_numpy(out).to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.from_numpy(out).dtype, device=DEV)


@pytest.mark.parametrize("dtype", (np.int32, np.int64), ids=("int32", "int64"))
@pytest.mark.parametrize("call", range(len(HYP_LENS)), ids=("width64", "width256", "width257"))
def test_chrf_characters_match_as_bleu_tokens(call, dtype):
    from fbk_fairseq_st_amd import kernels as K
    hyps, refs, want_bleu, want_chrf = case(call)
    hyp, hyp_len = padded(hyps, dtype)
    ref, ref_len = padded(refs, dtype)
    assert hyp.shape[1] == max(HYP_LENS[call]) and ref.shape[1] == max(REF_LENS)
    pieces = torch.arange(93, 93 + V + 1, dtype=torch.int32, device=DEV)
    piece_off = torch.arange(V + 2, dtype=torch.int32, device=DEV)
    chrf, chrf_status = K.chrf_stats(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk=-1, char_order=6, word_order=0)
    bleu, bleu_status = K.bleu_stats(hyp, hyp_len, ref, ref_len, PAD, EOS, unk=-1)
    chrf, bleu = chrf.cpu().numpy(), bleu.cpu().numpy()
    assert not chrf_status.cpu().numpy().any() and not bleu_status.cpu().numpy().any()
    # each kernel against its own reference
    assert (bleu == want_bleu).all(), np.nonzero((bleu != want_bleu).any(1))[0][:5]
    assert (chrf == want_chrf).all(), np.nonzero((chrf != want_chrf).any(1))[0][:5]
    # and against each other
    for k in range(4):
        assert (chrf[:, 3 * k + 2] == bleu[:, 2 + 2 * k]).all(), (k, "match")
        assert (chrf[:, 3 * k] == bleu[:, 3 + 2 * k]).all(), (k, "hyp_n / count")
    assert (chrf[:, 0] == bleu[:, 1]).all() and (chrf[:, 1] == bleu[:, 0]).all()
