"""The pairs on which chrF's character statistics must equal BLEU's (tests/test_ngram_match_gpu.py on the kernels,
tests/test_chrf_ref_cpu.py on the two Python references): rows of tokens FIRST .. FIRST + alphabet - 1, where token t stands for the
one code point 93 + t, pad and eos outside them, in three calls whose padded widths are their longest rows."""
import numpy as np

import bleu_ref
import chrf_ref

PAD, EOS, FIRST, V = 0, 1, 2, 8       # the tokens used are FIRST .. FIRST + alphabet - 1
HYP_LENS = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64), (65, 255, 256), (257,))       # one call each: the width is the longest
REF_LENS = (0, 1, 3, 5, 64, 65, 300)
ALPHABETS = (2, 5)                    # small: repeats on both sides, so that clipping decides
_CASES = {}


def case(call):
    """the pairs of one call, every hypothesis length x reference length x alphabet, with both references' statistics: made once"""
    if call not in _CASES:
        rng = np.random.default_rng(20 + call)
        hyps, refs = [], []
        for hl in HYP_LENS[call]:
            for rl in REF_LENS:
                for a in ALPHABETS:
                    hyps.append((FIRST + rng.integers(0, a, hl)).tolist())
                    refs.append((FIRST + rng.integers(0, a, rl)).tolist())
        text = lambda row: "".join(chr(93 + t) for t in row)
        bleu = np.array([bleu_ref.stats_counter(h, r, PAD, EOS, -1) for h, r in zip(hyps, refs)], np.int32)
        chrf = np.array([chrf_ref.pair_stats(text(h), text(r), 6, 0) for h, r in zip(hyps, refs)], np.int32)
        _CASES[call] = (hyps, refs, bleu, chrf)
    return _CASES[call]
