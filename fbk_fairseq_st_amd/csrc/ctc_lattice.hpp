// The Viterbi lattice over the 2 L + 1 CTC states of a transcript, as far as forced alignment (ctc_align.hip) and segmentation
// (ctc_segment.hip) share it: the frame step, the outputs of a sentence without a path, and what a walked block of frames gives.
// Both sentence phases call these and nothing else for the recursion and the sums, so the tie rule and the order of every sum are
// one statement, and segmentation with both ends pinned returns the aligner's bits as long as the two feed the step the same masks.
// What differs stays with the callers: where the emissions come from, how the previous frame's values travel between runs, and
// how the back-pointers are staged for the backward walk.  So do the loops that build a run's skip / live masks, although they
// say the same (ctc_align.hip: align_run_bits; ctc_segment.hip: the loop that also sets `zero`): these two copies can still
// drift apart, and test_pinned_ends_give_the_bits_of_ctc_align, which pairs every form of one kernel with one of the other, is what
// holds them together.  With the segmenter's `zero` bit set in a loop of its own behind a shared mask function, its recording
// kernel's register allocation moved and the frame loop was 2.0 to 2.5 % slower at 32 states per thread (profiles/ctc_lattice_ab.txt).
#pragma once
#include "ctc_rows.hpp"

// One frame of the recursion for a run of K consecutive states held in v (v[j] = state s0 + j; K >= 2: s0 is even, odd j = token
// j / 2 of the run), in place from the top state down so that every state still sees the previous frame below it.  p1 / p2: the
// previous frame's values of states s0 - 1 / s0 - 2.  eb / et: the frame's emissions of the blank and of the run's tokens (K = 1:
// et[0] is the one token, `odd0` says the state is one).  skip / live: bit j = state s0 + j may take s0 + j - 2 / exists; zero: bit
// j = the state is a free outer blank, its emission is 0 (the aligner has none: 0).  Among equal values the higher predecessor wins
// (strict >).  bits: the run's back-pointers, 2 per state, 16 states per dword: 0 stay, 1 advance, 2 skip.
template <int K>
__device__ __forceinline__ void lattice_step(float (&v)[K], float p1, float p2, const float (&et)[K == 1 ? 1 : K / 2], float eb, uint32_t skip,
                                             uint32_t live, uint32_t zero, uint32_t (&bits)[(K + 15) / 16], bool odd0 = false) {
#pragma unroll
    for (int w = 0; w < (K + 15) / 16; ++w) bits[w] = 0;
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
        const float a1 = j >= 1 ? v[j >= 1 ? j - 1 : 0] : p1;
        const float a2 = j >= 2 ? v[j >= 2 ? j - 2 : 0] : (j == 1 ? p1 : p2);
        float best = v[j]; uint32_t k = 0;
        if (a1 > best) { best = a1; k = 1; }
        if (((skip >> j) & 1) && a2 > best) { best = a2; k = 2; }
        float e;
        if constexpr (K == 1) e = odd0 ? et[0] : eb;
        else e = (j & 1) ? et[j >> 1] : eb;
        if ((zero >> j) & 1) e = 0.f;
        v[j] = ((live >> j) & 1) ? e + best : -INFINITY;
        bits[j >> 4] |= k << (2 * (j & 15));
    }
}

// what a sentence or recording without a path gets: states -1, and -- when its length L is usable -- (-1, -1) / -inf for its L tokens
__device__ inline void lattice_fail(int code, int L, int* __restrict__ st, int* __restrict__ fr, float* __restrict__ ts,
                                    float* __restrict__ score, int* __restrict__ status, int Tn, int tid, int nt) {
    for (int t = tid; t < Tn; t += nt) st[t] = -1;
    for (int i = tid; i < L; i += nt) { fr[2 * i] = fr[2 * i + 1] = -1; ts[i] = -INFINITY; }
    if (tid == 0) { *score = -INFINITY; *status = code; }
}

// Everything the path gives for the block of frames t0 .. t0 + cnt - 1 (cnt <= 64), lane i holding the state of frame t0 + i in `mine`
// (-1 behind cnt) and that frame's emission of it in lp (0 behind cnt).  In: s = the state of frame t0 - 1, s_after = that of frame
// t0 + cnt (-1 at the end), carry = the sum of lp over the run of s_after from t0 + cnt on.  Out: s_after / carry for the block before
// this one.  A token's frames are one run of equal states, so its score is a segmented suffix sum and the run's first frame writes
// it.  Blocks are 64 frames for every caller: the sums are taken in one order whatever the padded width.
__device__ __forceinline__ void lattice_emit_block(float lp, int t0, int cnt, int lane, int mine, int s, int& s_after, float& carry,
                                                   float& total, int* __restrict__ st, int* __restrict__ fr, float* __restrict__ ts) {
    const bool valid = lane < cnt;
    const int t = t0 + lane;
    if (valid) st[t] = mine;
    int prev = __shfl_up(mine, 1), next = __shfl_down(mine, 1);
    if (lane == 0) prev = t0 > 0 ? s : -2;
    if (lane == cnt - 1) next = s_after;
    float sv = lp;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ov = __shfl_down(sv, o); const int om = __shfl_down(mine, o);
        if (lane + o < 64 && om == mine) sv += ov;
    }
    if (valid && mine == s_after) sv += carry;
    if (valid && (mine & 1)) {
        const int i = mine >> 1;
        if (mine != prev) { fr[2 * i] = t; ts[i] = sv; }
        if (mine != next) fr[2 * i + 1] = t + 1;
    }
    carry = __shfl(sv, 0); s_after = __shfl(mine, 0);
    total += lp;
}
