// The text of a token row on the device (include/s2t_hip.h: s2t_chrf_stats states "Text of a row"), as chrf_stats.hip and
// text_units.hip stage it: the functions both kernels call, stated once.
//   * A thread takes a run of consecutive tokens of a side, looks up their pieces and counts the characters that are not
//     S2T_CHRF_SEP (chrf_measure); one workgroup scan (chrf_scan3) gives every thread the character offset of its run, whether the
//     text in front of it ended in a break, and the side's totals (characters, tokens outside the table).  Then the threads walk
//     their pieces again and write the characters into LDS, SEP dropped (chrf_expand).
//   * The first character of a word may carry a mark (bit 31; code points have 21 bits).  chrf_starts lists the marked positions
//     of a staged side in order; the caller wipes the marks when it has its lists.
//   * chrf_first_ids gives every word the index of its first equal occurrence in the list "hypothesis words, then reference
//     words" (lengths and code points compared: no hash), written as the caller's element type: 16-bit ids into LDS for chrF's
//     word n-grams, 32-bit ids into global memory for s2t_text_units.
//   * What stays with the callers: the pair's rows and every refusal, the LDS carve (CHRF_CAP elements per staged array), the
//     barriers between these steps, chrF's punctuation split and its matching loops, and every launch rule.
// Every function here is called by all threads of a workgroup of NT = 64 NW threads, under uniform control flow.  `Args` is the
// caller's kernel-argument struct: the functions read its piece table by name -- pieces (uint32 code points), piece_off (int32
// [V + 2]), unk (long long), V and n_pieces -- so that each kernel keeps the argument layout it had (chrF's is the one it was
// timed with).
#pragma once
#include "common.hpp"
#include "s2t_hip.h"

namespace {

constexpr int CHRF_SLACK = 9;                                       // slots behind a staged side that windows may read
constexpr int CHRF_CAP = S2T_CHRF_MAX_CHARS + CHRF_SLACK;           // 4,104 elements per array
constexpr uint32_t CHRF_START = 0x80000000u;                        // mark: this character begins a word
constexpr uint32_t CHRF_CODE = 0x001fffffu;
constexpr int CHRF_OVER = S2T_CHRF_MAX_CHARS + 1;                   // a thread's count saturates here: the side is refused anyway

// the piece of a token: [a, b) of pieces; false for a token outside [0, V) or offsets that are no range of the table
template <typename Args>
__device__ __forceinline__ bool chrf_piece(const Args& p, long long tok, bool ref_side, int& a, int& b) {
    if (tok < 0 || tok >= p.V) return false;
    const int e = (ref_side && p.unk >= 0 && tok == p.unk) ? p.V : (int)tok;
    a = p.piece_off[e]; b = p.piece_off[e + 1];
    return a >= 0 && b >= a && b <= p.n_pieces;
}

// exclusive scan over the threads, in thread order, of three things at once: n (sum), bad (sum) and flag (the last one that is not
// 0).  Returns this thread's prefixes and the totals of n and bad.  Two barriers; s_w is free again behind the second.
template <int NW>
__device__ __forceinline__ void chrf_scan3(int n, int bad, int flag, int (*s_w)[3], int& n_before, int& flag_before, int& n_all, int& bad_all) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ni = n, bi = bad, fi = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int tn = __shfl_up(ni, o), tb = __shfl_up(bi, o), tf = __shfl_up(fi, o);
        if (lane >= o) { ni += tn; bi += tb; fi = fi ? fi : tf; }
    }
    int fe = __shfl_up(fi, 1);
    if (lane == 0) fe = 0;
    __syncthreads();                                                // whoever read s_w last is done
    if (lane == 63) { s_w[wave][0] = ni; s_w[wave][1] = bi; s_w[wave][2] = fi; }
    __syncthreads();
    int nb = 0, fb = 0;
    n_all = 0; bad_all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int xn = s_w[w][0], xb = s_w[w][1], xf = s_w[w][2];
        if (w < wave) { nb += xn; fb = xf ? xf : fb; }
        n_all += xn; bad_all += xb;
    }
    n_before = nb + ni - n;
    flag_before = fe ? fe : fb;
}

// first walk over a side's pieces: this thread's run of tokens -> its characters (saturating), bad tokens, and how its text ends
// (0: no text, 1: in a character, 2: in a break)
template <int NT, typename Args>
__device__ __forceinline__ void chrf_measure(const Args& p, const char* row, int es, int len, bool ref_side, int& n, int& bad, int& flag) {
    const int ipt = (len + NT - 1) / NT, t0 = min((int)threadIdx.x * ipt, len), t1 = min(t0 + ipt, len);
    n = 0; bad = 0; flag = 0;
    for (int t = t0; t < t1; ++t) {
        int a, b;
        if (!chrf_piece(p, int_at(row, es, t), ref_side, a, b)) { ++bad; continue; }
        for (int j = a; j < b && n < CHRF_OVER; ++j) {
            const bool sep = p.pieces[j] == S2T_CHRF_SEP;
            n += sep ? 0 : 1;
            flag = sep ? 2 : 1;
        }
    }
}

// second walk: write the characters at `at`; `flag` is how the text in front of this thread ended (0 counts as a break)
template <int NT, typename Args>
__device__ __forceinline__ void chrf_expand(const Args& p, const char* row, int es, int len, bool ref_side, int at, int flag, bool words,
                                            uint32_t* out) {
    const int ipt = (len + NT - 1) / NT, t0 = min((int)threadIdx.x * ipt, len), t1 = min(t0 + ipt, len);
    bool brk = flag != 1;
    for (int t = t0; t < t1; ++t) {
        int a, b;
        if (!chrf_piece(p, int_at(row, es, t), ref_side, a, b)) continue;        // cannot happen: such a pair was refused
        for (int j = a; j < b; ++j) {
            const uint32_t c = p.pieces[j];
            if (c == S2T_CHRF_SEP) { brk = true; continue; }
            if (at < S2T_CHRF_MAX_CHARS) out[at] = (c & CHRF_CODE) | (words && brk ? CHRF_START : 0u);
            ++at; brk = false;
        }
    }
}

// list the marked positions of xs[0 .. n) in order into st, close the list with n; returns their number
template <int NW>
__device__ __forceinline__ int chrf_starts(const uint32_t* xs, int n, uint16_t* st, int (*s_w)[3]) {
    constexpr int NT = 64 * NW;
    const int ipt = (n + NT - 1) / NT, i0 = min((int)threadIdx.x * ipt, n), i1 = min(i0 + ipt, n);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += (int)(xs[i] >> 31);
    int at, f, total, b;
    chrf_scan3<NW>(mine, 0, 0, s_w, at, f, total, b);
    for (int i = i0; i < i1; ++i)
        if (xs[i] >> 31) st[at++] = (uint16_t)i;
    if (threadIdx.x == 0) st[total] = (uint16_t)n;
    return total;
}

// a word's id: the index of its first equal occurrence in "hypothesis words, then reference words".  hs / rs: the staged sides,
// marks wiped; hst / rst: their closed start lists (Wh + 1 and Wr + 1 entries); the ids go to hid[0 .. Wh) and rid[0 .. Wr).
// Wave w takes the words 64 w + lane (+ NT, ...) and walks the words in front of them with wave-uniform loops.  lane, wave: the
// caller's threadIdx.x & 63 and its uniform threadIdx.x >> 6 (handed in: chrF's kernel then compiles to the instructions it had).
template <int NT, typename Out>
__device__ __forceinline__ void chrf_first_ids(int lane, int wave, const uint32_t* hs, const uint16_t* hst, int Wh, const uint32_t* rs, const uint16_t* rst, int Wr,
                                               Out* hid, Out* rid) {
    const int Wt = Wh + Wr;
    for (int q0 = 64 * wave; q0 < Wt; q0 += NT) {                   // wave-uniform
        const int w = q0 + lane;
        const bool act = w < Wt;
        const bool mine_h = w < Wh;
        const uint32_t* ms = mine_h ? hs : rs;
        const int s = !act ? 0 : mine_h ? (int)hst[w] : (int)rst[w - Wh];
        const int len = !act ? -1 : (mine_h ? (int)hst[w + 1] : (int)rst[w - Wh + 1]) - s;
        const uint32_t c0 = act ? ms[s] : 0u;
        int id = w;
        const int uend = min(q0 + 63, Wt - 1);                      // u < w <= q0 + 63
#define CHRF_FIRST(xs, xst, base, count)                            \
        {                                                           \
            int sp = (int)(xst)[0];                                 \
            _Pragma("clang loop vectorize(disable)")                \
            for (int u = 0; u < (count); ++u) {                     \
                const int se = (int)(xst)[u + 1];                   \
                if (id == w && (base) + u < w && se - sp == len && (xs)[sp] == c0) { \
                    int k = 1;                                      \
                    while (k < len && (xs)[sp + k] == ms[s + k]) ++k; \
                    if (k == len) id = (base) + u;                  \
                }                                                   \
                sp = se;                                            \
            }                                                       \
        }
        CHRF_FIRST(hs, hst, 0, min(uend, Wh))
        CHRF_FIRST(rs, rst, Wh, uend - Wh)
#undef CHRF_FIRST
        if (act) { if (mine_h) hid[w] = (Out)id; else rid[w - Wh] = (Out)id; }
    }
}

}  // namespace
