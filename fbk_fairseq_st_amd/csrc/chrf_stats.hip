// chrF / chrF++ statistics of detokenised token rows (include/s2t_hip.h: s2t_chrf_stats states the rule): per pair the character
// n-gram totals and clipped matches of the orders 1 to 6 and the word n-gram ones of the orders 1 and 2, as exact integers.
// One launch, one pair per workgroup, no atomics, no host read, no memset; every output element is written.
//   * Text: a thread takes a run of consecutive tokens of a side, looks up their pieces and counts the characters that are not
//     S2T_CHRF_SEP; one workgroup scan gives every thread the character offset of its run, whether the text in front of it ended
//     in a break, and the side's totals (characters, tokens outside the table).  A pair that must be refused leaves here, the same
//     in every thread.  Then the threads walk their pieces again and write the characters into LDS, SEP dropped.  These functions,
//     the list of word starts and the first-occurrence ids below live in text_rows.hpp, which text_units.hip shares.
//   * Words (word_order > 0 only): the first character of a word carries a mark (bit 31; code points have 21 bits).  The
//     punctuation split adds marks: each position decides for itself from the marks and characters it reads, the decisions are
//     written behind a barrier.  A second scan lists the word starts, the marks are wiped, and every word gets the index of its
//     first equal occurrence in the list "hypothesis words, then reference words" (lengths and code points compared: no hash), so
//     word n-grams are n-grams of 16-bit ids.
//   * Matches, for characters (N = 6 on 32-bit code points) and for word ids (N = 2 on 16-bit ids) alike: the position-wise
//     counting that ngram_match.hpp states (the rule, why the windows may read the slack slots), in loops of its own for N orders,
//     chrf_matches: on functions shared with the BLEU kernels this kernel was 15 to 35 % slower at 60-token rows
//     (profiles/ngram_match_ab.txt, section 2).  tests/test_ngram_match_gpu.py holds its numbers to bleu_stats.hip's.  The
//     hypothesis' end cuts the orders of a position once, after the loops.
//   * Threads: 256 for hypotheses up to S2T_CHRF_GROUP_LEN tokens wide, 1,024 above (the width is what the host knows without a
//     read).  Inside, wave w takes the positions 64 w + lane (+ threads, ...): a wave without positions skips the loops, so the
//     work follows the character count in steps of 64.
//   * LDS (dynamic): two sides of (S2T_CHRF_MAX_CHARS + 9) code points, 32.8 KB; with words four more 16-bit arrays (starts and
//     ids of both sides), 65.6 KB in all.
#include "common.hpp"
#include "s2t_hip.h"
#include "text_rows.hpp"

namespace {

struct ChrfArgs {
    const void* hyp; const void* hyp_len; const void* ref; const void* ref_len;
    const int* hyp_row; const int* ref_row;
    const uint32_t* pieces; const int* piece_off;
    int* stats; int* status;
    long long unk;
    int hyp_elem, ref_elem, Hmax, Rmax, Hrows, Rrows, V, n_pieces, char_order, word_order;
};

__device__ __forceinline__ bool chrf_punct(uint32_t c) {            // Python's string.punctuation
    return (c >= 33 && c <= 47) || (c >= 58 && c <= 64) || (c >= 91 && c <= 96) || (c >= 123 && c <= 126);
}

// which of this thread's positions (tid + NT q, bit q) begin a word through the punctuation split; reads only
template <int NT>
__device__ __forceinline__ uint32_t chrf_split(const uint32_t* xs, int n) {
    uint32_t marks = 0;
    int q = 0;
    for (int i = threadIdx.x; i < n; i += NT, ++q) {
        const uint32_t c = xs[i];
        if (c & CHRF_START) continue;                               // i is inside a word of at least two characters
        const bool last = i + 1 == n || (xs[i + 1] & CHRF_START);
        if (last && chrf_punct(c & CHRF_CODE)) {                    // the last-character rule comes first
            marks |= 1u << q;
        } else if ((xs[i - 1] & CHRF_START) && chrf_punct(xs[i - 1] & CHRF_CODE)) {   // i is the second character, the first is one
            int j = i;
            while (j + 1 < n && !(xs[j + 1] & CHRF_START)) ++j;     // the word's last character
            if (!chrf_punct(xs[j] & CHRF_CODE)) marks |= 1u << q;
        }
    }
    return marks;
}

// m[k] += the positions of hs[0 .. H) that match at order k + 1 against rs[0 .. R), summed over this thread's positions
template <typename T, int N, int NT>
__device__ __forceinline__ void chrf_matches(const T* hs, int H, const T* rs, int R, int (&m)[N]) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int q0 = 64 * wave; q0 < H; q0 += NT) {                    // wave-uniform
        const int i = q0 + lane;
        const bool act = i < H;
        const int ii = act ? i : 0;
        T h[N], x[N];
        int c[N], r[N];
#pragma unroll
        for (int k = 0; k < N; ++k) { h[k] = hs[ii + k]; c[k] = 0; r[k] = 0; }
        const int clip = act ? min(N, H - i) : 0;                   // the orders this position has
        // lim: the elements window x has (uniform); ok: this lane takes part
#define CHRF_TALLY(cnt, lim, ok)                                    \
        {                                                           \
            int a = (int)(ok);                                      \
            _Pragma("unroll") for (int k = 0; k < N; ++k) {         \
                a &= (int)(h[k] == x[k]) & (int)((lim) > k);        \
                cnt[k] += a;                                        \
            }                                                       \
            _Pragma("unroll") for (int k = 0; k + 1 < N; ++k) x[k] = x[k + 1]; \
        }
        {   // reference positions j: cref
#pragma unroll
            for (int k = 0; k + 1 < N; ++k) x[k] = rs[k];
            const int full = max(R - (N - 1), 0);
#pragma clang loop vectorize(disable) unroll_count(4)
            for (int j = 0; j < full; ++j) {
                x[N - 1] = rs[j + N - 1];
                CHRF_TALLY(c, N, true)
            }
#pragma clang loop vectorize(disable) unroll(disable)
            for (int j = full; j < R; ++j) {                        // the last windows: cut by the reference's end
                x[N - 1] = rs[j + N - 1];
                CHRF_TALLY(c, R - j, true)
            }
        }
        {   // hypothesis positions k < i: rank.  k <= H - 2, so the reads stay inside the slack
#pragma unroll
            for (int k = 0; k + 1 < N; ++k) x[k] = hs[k];
            const int kend = min(q0 + 63, H - 1);
#pragma clang loop vectorize(disable) unroll_count(4)
            for (int j = 0; j < q0; ++j) {                          // in front of every position of this wave
                x[N - 1] = hs[j + N - 1];
                CHRF_TALLY(r, N, true)
            }
#pragma clang loop vectorize(disable) unroll_count(4)
            for (int j = q0; j < kend; ++j) {
                x[N - 1] = hs[j + N - 1];
                CHRF_TALLY(r, N, j < i)
            }
        }
#undef CHRF_TALLY
#pragma unroll
        for (int k = 0; k < N; ++k) m[k] += (int)(clip > k && r[k] < c[k]);
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void chrf_stats_kernel(const ChrfArgs p) {
    extern __shared__ __attribute__((aligned(16))) char chrf_smem[];
    __shared__ int s_w[NW][3];
    __shared__ int s_red[NW][8];
    constexpr int NT = 64 * NW;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* out = p.stats + (size_t)b * 24;
    const bool words = p.word_order > 0;

    // ---- the pair's rows
    const long long hrow_i = p.hyp_row ? (long long)p.hyp_row[b] : (long long)b;
    const long long rrow_i = p.ref_row ? (long long)p.ref_row[b] : (long long)b;
    bool refused = hrow_i < 0 || hrow_i >= p.Hrows || rrow_i < 0 || rrow_i >= p.Rrows;
    const long long hq = refused ? 0 : int_at(p.hyp_len, p.hyp_elem, hrow_i);
    const long long rq = refused ? 0 : int_at(p.ref_len, p.ref_elem, rrow_i);
    refused = refused || hq < 0 || hq > p.Hmax || rq < 0 || rq > p.Rmax;
    int H = 0, R = 0, hat = 0, hflag = 0, rat = 0, rflag = 0;
    const char* hrow = nullptr;
    const char* rrow = nullptr;
    if (!refused) {                                                 // the same in every thread of the workgroup
        hrow = reinterpret_cast<const char*>(p.hyp) + (size_t)hrow_i * p.Hmax * p.hyp_elem;
        rrow = reinterpret_cast<const char*>(p.ref) + (size_t)rrow_i * p.Rmax * p.ref_elem;
        int n, bad, flag, hbad, rbad;
        chrf_measure<NT>(p, hrow, p.hyp_elem, (int)hq, false, n, bad, flag);
        chrf_scan3<NW>(n, bad, flag, s_w, hat, hflag, H, hbad);
        chrf_measure<NT>(p, rrow, p.ref_elem, (int)rq, true, n, bad, flag);
        chrf_scan3<NW>(n, bad, flag, s_w, rat, rflag, R, rbad);
        refused = hbad > 0 || rbad > 0 || H > S2T_CHRF_MAX_CHARS || R > S2T_CHRF_MAX_CHARS;
    }
    if (refused) {
        if (tid < 24) out[tid] = 0;
        if (tid == 0) p.status[b] = 2;
        return;
    }
    H = __builtin_amdgcn_readfirstlane(H);                          // the same in every lane: said so, for scalar loop counters
    R = __builtin_amdgcn_readfirstlane(R);

    // ---- stage the characters
    uint32_t* hs = reinterpret_cast<uint32_t*>(chrf_smem);
    uint32_t* rs = hs + CHRF_CAP;
    uint16_t* hst = reinterpret_cast<uint16_t*>(rs + CHRF_CAP);     // with words only: starts and ids, CHRF_CAP each
    uint16_t* rst = hst + CHRF_CAP;
    uint16_t* hid = rst + CHRF_CAP;
    uint16_t* rid = hid + CHRF_CAP;
    chrf_expand<NT>(p, hrow, p.hyp_elem, (int)hq, false, hat, hflag, words, hs);
    chrf_expand<NT>(p, rrow, p.ref_elem, (int)rq, true, rat, rflag, words, rs);
    if (tid < CHRF_SLACK) { hs[H + tid] = 0; rs[R + tid] = 0; }
    __syncthreads();

    int mw[2] = {0, 0};
    int Wh = 0, Wr = 0;
    if (words) {                                                    // uniform
        // ---- the punctuation split: decide, then write
        const uint32_t hmarks = chrf_split<NT>(hs, H), rmarks = chrf_split<NT>(rs, R);
        __syncthreads();
        {
            int q = 0;
            for (int i = tid; i < H; i += NT, ++q) if (hmarks >> q & 1) hs[i] |= CHRF_START;
            q = 0;
            for (int i = tid; i < R; i += NT, ++q) if (rmarks >> q & 1) rs[i] |= CHRF_START;
        }
        __syncthreads();
        // ---- the words' starts, then the marks go
        Wh = __builtin_amdgcn_readfirstlane(chrf_starts<NW>(hs, H, hst, s_w));
        Wr = __builtin_amdgcn_readfirstlane(chrf_starts<NW>(rs, R, rst, s_w));
        __syncthreads();
        for (int i = tid; i < H; i += NT) hs[i] &= CHRF_CODE;
        for (int i = tid; i < R; i += NT) rs[i] &= CHRF_CODE;
        if (tid < 4) { hid[Wh + tid] = 0; rid[Wr + tid] = 0; }
        __syncthreads();
        // ---- a word's id: the index of its first equal occurrence in "hypothesis words, then reference words"
        chrf_first_ids<NT>(lane, wave, hs, hst, Wh, rs, rst, Wr, hid, rid);
        __syncthreads();
        chrf_matches<uint16_t, 2, NT>(hid, Wh, rid, Wr, mw);
    }

    // ---- characters
    int mc[6] = {0, 0, 0, 0, 0, 0};
    chrf_matches<uint32_t, 6, NT>(hs, H, rs, R, mc);

    // ---- sum
    int m[8] = {mc[0], mc[1], mc[2], mc[3], mc[4], mc[5], mw[0], mw[1]};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[k] += __shfl_xor(m[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_red[wave][k] = m[k];
    }
    __syncthreads();
    if (tid < 8) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_red[w][tid];
        const bool on = tid < 6 ? tid < p.char_order : tid - 6 < p.word_order;
        const int k = tid < 6 ? tid : tid - 6;
        const int nh = tid < 6 ? H : Wh, nr = tid < 6 ? R : Wr;
        out[3 * tid + 0] = on ? max(nh - k, 0) : 0;
        out[3 * tid + 1] = on ? max(nr - k, 0) : 0;
        out[3 * tid + 2] = on ? sum : 0;
    }
    if (tid == 0) p.status[b] = 0;
}

template <int NW>
int chrf_launch(hipStream_t st, int P, const ChrfArgs& p) {
    const size_t lds = (size_t)2 * CHRF_CAP * sizeof(uint32_t) + (p.word_order > 0 ? (size_t)4 * CHRF_CAP * sizeof(uint16_t) : 0);
    if (lds > 60000) {                                              // with words: asked for on every such call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&chrf_stats_kernel<NW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return S2T_EHIP(e);
    }
    hipLaunchKernelGGL((chrf_stats_kernel<NW>), dim3(P), dim3(64 * NW), lds, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

}  // namespace

extern "C" int s2t_chrf_stats(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                              const int* hyp_row, const int* ref_row, int P, int Hmax, int Rmax, int Hrows, int Rrows,
                              const unsigned int* pieces, const int* piece_off, int n_pieces, int V, long long unk, int char_order,
                              int word_order, int* stats, int* status, void* stream) {
    if (P <= 0) return S2T_OK;
    if (!hyp || !hyp_len || !ref || !ref_len || !pieces || !piece_off || !stats || !status) return S2T_EINVAL;
    if (Hmax < 0 || Rmax < 0 || V < 0 || n_pieces < 0) return S2T_EINVAL;
    if ((hyp_elem != 4 && hyp_elem != 8) || (ref_elem != 4 && ref_elem != 8)) return S2T_EINVAL;
    if (hyp_row ? Hrows < 0 : Hrows != P) return S2T_EINVAL;
    if (ref_row ? Rrows < 0 : Rrows != P) return S2T_EINVAL;
    if (unk >= V) return S2T_EINVAL;
    if (char_order < 1 || char_order > S2T_CHRF_MAX_CHAR_ORDER || word_order < 0 || word_order > S2T_CHRF_MAX_WORD_ORDER) return S2T_EINVAL;
    if (Hmax > S2T_CHRF_MAX_LEN || Rmax > S2T_CHRF_MAX_LEN) return S2T_ENOTSUP;
    ChrfArgs p;
    p.hyp = hyp; p.hyp_len = hyp_len; p.ref = ref; p.ref_len = ref_len; p.hyp_row = hyp_row; p.ref_row = ref_row;
    p.pieces = pieces; p.piece_off = piece_off; p.stats = stats; p.status = status;
    p.unk = unk;
    p.hyp_elem = hyp_elem; p.ref_elem = ref_elem; p.Hmax = Hmax; p.Rmax = Rmax; p.Hrows = Hrows; p.Rrows = Rrows;
    p.V = V; p.n_pieces = n_pieces; p.char_order = char_order; p.word_order = word_order;
    hipStream_t st = (hipStream_t)stream;
    return Hmax <= S2T_CHRF_GROUP_LEN ? chrf_launch<4>(st, P, p) : chrf_launch<16>(st, P, p);
}
