// Clipped n-gram matching by positions, as BLEU of one pair (bleu_stats.hip), BLEU of a candidate against a list (bleu_pairs.hip) and
// chrF (chrf_stats.hip) apply it: the rule and the slack contract, stated once, and the window step and the two loops that the two
// BLEU kernels share.
//   * The rule: hypothesis position i matches at order n iff rank_n(i) < cref_n(i), where rank_n counts the earlier hypothesis
//     positions and cref_n the reference positions that hold the same n-gram.  Summed over i this is the clipped match count, and
//     n-grams are compared element by element: no hash, no map.
//   * A lane owns position i with its window h[0 .. N) in registers and walks the other side's positions with wave-uniform loops:
//     every lane reads the same window x (LDS broadcasts, one new element per step).  The common prefix of the two windows serves
//     the N orders at once: a pair is an order-n hit for every n up to its length.
//   * The slack contract: N - 1 readable slots lie behind each staged side, and they may hold anything.  The window of position i
//     is cut at the hypothesis' end (and, for BLEU, at its first unk) by the caller's `clip`, once, after the loops, so what the
//     lanes read beyond it does not count.  The reference's end cuts the last N - 1 windows of the cref loop, which is uniform and
//     runs as a tail of its own.  In the rank loop nothing is cut: k < i keeps window k inside the sentence wherever window i is,
//     and k <= H - 2, so the reads stay inside the slack.
//   * What stays with the callers: the trims (ballots on global rows in bleu_stats.hip, a scan in LDS in bleu_pairs.hip), staging
//     and the width of the staged elements, the window load and `clip` with its unk cut, which positions a thread owns and how often
//     it takes their ranks (per position, or once per thread for a whole list), the reductions, and every launch rule.
//     bleu_pairs.hip's one-wave store also keeps its own form: there lane l of the wave writes number l of the record, ten lanes
//     in one store, where bleu_record is one thread's ten stores.
//   * The step and the loops are text (BLEU_TALLY, BLEU_CREF, BLEU_RANK), not functions.  As function templates for N orders the
//     two BLEU kernels missed their timing bound at rows of 200 tokens, by 0.05 to 1.2 % in two spellings of the rank loop
//     (profiles/ngram_match_ab.txt, sections 3 and 4), and even the files' macro and loops moved verbatim into two functions did
//     not compile to the files' instruction streams; as text they do.  The price: the macros read the includer's locals by name.
//     A file that uses them must have the element type T and this lane's window h0 .. h3 (of type T) in scope, must not use the
//     names x0 .. x3, full, kend, j, k or a for anything the arguments mention, and the macros stay defined to its end.
//   * chrf_stats.hip (N = 6 on characters, N = 2 on word ids) applies the same rule under the same contract in loops of its own,
//     chrf_matches: on the function templates it was 15 to 35 % slower at rows of 60 tokens (same profile, section 2), and the text
//     here is for four orders.  tests/test_ngram_match_gpu.py holds chrF's numbers to BLEU's.
#pragma once
#include "common.hpp"

// One step of a loop below: n1 .. n4 += whether the uniform window x0 .. x3 equals this lane's h0 .. h3 in its first 1 .. 4 tokens.
// lim: the tokens window x has (uniform); ok: this lane takes part.
#define BLEU_TALLY(n1, n2, n3, n4, lim, ok)                         \
    {                                                               \
        int a = (int)(h0 == x0) & (int)(ok);                        \
        n1 += a;                                                    \
        a &= (int)(h1 == x1) & (int)((lim) >= 2);                   \
        n2 += a;                                                    \
        a &= (int)(h2 == x2) & (int)((lim) >= 3);                   \
        n3 += a;                                                    \
        a &= (int)(h3 == x3) & (int)((lim) >= 4);                   \
        n4 += a;                                                    \
    }

// cref, one statement: c1 .. c4 += the positions of rs[0 .. R) that hold this lane's window at the orders 1 .. 4 (R uniform).  The
// last three windows, cut by the reference's end, run as a tail of their own.  The includer's element type is T.
#define BLEU_CREF(rs, R, c1, c2, c3, c4)                                                \
    {                                                                                   \
        T x0 = (rs)[0], x1 = (rs)[1], x2 = (rs)[2];                                     \
        const int full = max((R) - 3, 0);                                               \
        _Pragma("clang loop vectorize(disable) unroll_count(4)")                        \
        for (int j = 0; j < full; ++j) {                                                \
            const T x3 = (rs)[j + 3];                                                   \
            BLEU_TALLY(c1, c2, c3, c4, 4, true)                                         \
            x0 = x1; x1 = x2; x2 = x3;                                                  \
        }                                                                               \
        _Pragma("clang loop vectorize(disable) unroll(disable)")                        \
        for (int j = full; j < (R); ++j) {                                              \
            const T x3 = (rs)[j + 3];                                                   \
            BLEU_TALLY(c1, c2, c3, c4, (R) - j, true)                                   \
            x0 = x1; x1 = x2; x2 = x3;                                                  \
        }                                                                               \
    }

// rank, one statement: r1 .. r4 += the positions k < i of hs[0 .. H) that hold this lane's window, for the lanes i = q0 .. q0 + 63 of
// a wave (q0 and H uniform): the positions in front of the wave without a test, the wave's own under k < i.  k <= H - 2, so the
// reads stay inside the slack.
#define BLEU_RANK(hs, H, q0, i, r1, r2, r3, r4)                                         \
    {                                                                                   \
        T x0 = (hs)[0], x1 = (hs)[1], x2 = (hs)[2];                                     \
        const int kend = min((q0) + 63, (H) - 1);                                       \
        _Pragma("clang loop vectorize(disable) unroll_count(4)")                        \
        for (int k = 0; k < (q0); ++k) {                                                \
            const T x3 = (hs)[k + 3];                                                   \
            BLEU_TALLY(r1, r2, r3, r4, 4, true)                                         \
            x0 = x1; x1 = x2; x2 = x3;                                                  \
        }                                                                               \
        _Pragma("clang loop vectorize(disable) unroll_count(4)")                        \
        for (int k = (q0); k < kend; ++k) {                                             \
            const T x3 = (hs)[k + 3];                                                   \
            BLEU_TALLY(r1, r2, r3, r4, 4, k < (i))                                      \
            x0 = x1; x1 = x2; x2 = x3;                                                  \
        }                                                                               \
    }

// The ten numbers of a BLEU pair (include/s2t_hip.h: s2t_bleu_stats): reflen, predlen, then match_n and count_n of the orders 1 to 4.
// m12 = match1 | match2 << 16, m34 = match3 | match4 << 16.
__device__ __forceinline__ void bleu_record(int* o, int R, int H, uint32_t m12, uint32_t m34) {
    o[0] = R; o[1] = H;
    o[2] = (int)(m12 & 0xffff); o[3] = H;
    o[4] = (int)(m12 >> 16);    o[5] = max(H - 1, 0);
    o[6] = (int)(m34 & 0xffff); o[7] = max(H - 2, 0);
    o[8] = (int)(m34 >> 16);    o[9] = max(H - 3, 0);
}
