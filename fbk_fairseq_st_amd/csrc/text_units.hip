// Comparable unit rows of detokenised token rows (include/s2t_hip.h: s2t_text_units states the rule): per pair the words of both
// texts as first-equal-occurrence ids, or their code points with or without one space between words, ready for s2t_edit_align.
// One launch, one pair per workgroup, no atomics, no host read, no memset.
//   * Text: the functions of text_rows.hpp, as chrf_stats.hip calls them: measure, scan, refuse, expand into LDS with the first
//     character of every word marked (no punctuation split: that is chrF++'s rule, not WER's).
//   * Units.  Words: the word starts are listed, the marks wiped, and chrf_first_ids writes the ids straight to global memory.
//     Characters with spaces: no second expansion, word w that starts at character s goes to out[s + w ..], U+0020 to
//     out[s + w - 1] for w > 0; a wave takes a word at a time, its lanes the word's characters.  Characters without spaces: the
//     staged code points as they are (expanded without marks, no start lists).
//   * A side with more units than its width is refused before anything but status and the two counts is written: every refusal
//     is decided the same in every thread, behind the last scan.
//   * Threads: 256 for rows up to S2T_CHRF_GROUP_LEN tokens wide on both sides, 1,024 above.
//   * LDS (dynamic): two sides of CHRF_CAP code points and two start lists of CHRF_CAP 16-bit entries, 49.2 KB.
#include "common.hpp"
#include "s2t_hip.h"
#include "text_rows.hpp"

namespace {

struct UnitArgs {
    const void* hyp; const void* hyp_len; const void* ref; const void* ref_len;
    const int* hyp_row; const int* ref_row;
    const uint32_t* pieces; const int* piece_off;
    int* hyp_units; int* ref_units; int* hyp_n; int* ref_n; int* status;
    long long unk;
    int hyp_elem, ref_elem, Hmax, Rmax, Hrows, Rrows, V, n_pieces, mode, Uh, Ur;
};

// characters with one U+0020 between consecutive words: xs[0 .. n) with its closed start list st (W + 1 entries) -> out
template <int NW>
__device__ __forceinline__ void text_spaced(const uint32_t* xs, const uint16_t* st, int W, int* out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int w = wave; w < W; w += NW) {                            // wave-uniform
        const int s = (int)st[w], e = (int)st[w + 1];
        if (w > 0 && lane == 0) out[s + w - 1] = 0x20;
        for (int k = s + lane; k < e; k += 64) out[k + w] = (int)(xs[k] & CHRF_CODE);
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void text_units_kernel(const UnitArgs p) {
    extern __shared__ __attribute__((aligned(16))) char text_smem[];
    __shared__ int s_w[NW][3];
    constexpr int NT = 64 * NW;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

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
    int Wh = 0, Wr = 0, nh = 0, nr = 0;
    uint32_t* hs = reinterpret_cast<uint32_t*>(text_smem);
    uint32_t* rs = hs + CHRF_CAP;
    uint16_t* hst = reinterpret_cast<uint16_t*>(rs + CHRF_CAP);
    uint16_t* rst = hst + CHRF_CAP;
    const bool words = p.mode != 2;
    if (!refused) {
        H = __builtin_amdgcn_readfirstlane(H);
        R = __builtin_amdgcn_readfirstlane(R);
        // ---- stage the characters, list the words' starts
        chrf_expand<NT>(p, hrow, p.hyp_elem, (int)hq, false, hat, hflag, words, hs);
        chrf_expand<NT>(p, rrow, p.ref_elem, (int)rq, true, rat, rflag, words, rs);
        __syncthreads();
        if (words) {                                                // uniform
            Wh = __builtin_amdgcn_readfirstlane(chrf_starts<NW>(hs, H, hst, s_w));
            Wr = __builtin_amdgcn_readfirstlane(chrf_starts<NW>(rs, R, rst, s_w));
            __syncthreads();
        }
        nh = p.mode == 0 ? Wh : H + (p.mode == 1 ? max(Wh - 1, 0) : 0);
        nr = p.mode == 0 ? Wr : R + (p.mode == 1 ? max(Wr - 1, 0) : 0);
        refused = nh > p.Uh || nr > p.Ur;
    }
    if (refused) {                                                  // nothing was written so far
        if (tid == 0) { p.hyp_n[b] = 0; p.ref_n[b] = 0; p.status[b] = 2; }
        return;
    }

    // ---- the units: nh <= Uh and nr <= Ur entries of this pair's rows
    int* hu = p.hyp_units + (size_t)b * p.Uh;
    int* ru = p.ref_units + (size_t)b * p.Ur;
    if (p.mode == 0) {
        for (int i = tid; i < H; i += NT) hs[i] &= CHRF_CODE;
        for (int i = tid; i < R; i += NT) rs[i] &= CHRF_CODE;
        __syncthreads();
        chrf_first_ids<NT>(lane, wave, hs, hst, Wh, rs, rst, Wr, hu, ru);
    } else if (p.mode == 1) {
        text_spaced<NW>(hs, hst, Wh, hu);
        text_spaced<NW>(rs, rst, Wr, ru);
    } else {
        for (int i = tid; i < H; i += NT) hu[i] = (int)hs[i];
        for (int i = tid; i < R; i += NT) ru[i] = (int)rs[i];
    }
    if (tid == 0) { p.hyp_n[b] = nh; p.ref_n[b] = nr; p.status[b] = 0; }
}

template <int NW>
int text_units_launch(hipStream_t st, int P, const UnitArgs& p) {
    const size_t lds = (size_t)2 * CHRF_CAP * sizeof(uint32_t) + (size_t)2 * CHRF_CAP * sizeof(uint16_t);
    hipLaunchKernelGGL((text_units_kernel<NW>), dim3(P), dim3(64 * NW), lds, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

}  // namespace

extern "C" int s2t_text_units(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                              const int* hyp_row, const int* ref_row, int P, int Hmax, int Rmax, int Hrows, int Rrows,
                              const unsigned int* pieces, const int* piece_off, int n_pieces, int V, long long unk, int mode, int Uh,
                              int Ur, int* hyp_units, int* ref_units, int* hyp_n, int* ref_n, int* status, void* stream) {
    if (P <= 0) return S2T_OK;
    if (!hyp || !hyp_len || !ref || !ref_len || !pieces || !piece_off || !hyp_units || !ref_units || !hyp_n || !ref_n || !status)
        return S2T_EINVAL;
    if (Hmax < 0 || Rmax < 0 || V < 0 || n_pieces < 0) return S2T_EINVAL;
    if ((hyp_elem != 4 && hyp_elem != 8) || (ref_elem != 4 && ref_elem != 8)) return S2T_EINVAL;
    if (hyp_row ? Hrows < 0 : Hrows != P) return S2T_EINVAL;
    if (ref_row ? Rrows < 0 : Rrows != P) return S2T_EINVAL;
    if (unk >= V) return S2T_EINVAL;
    if (mode < 0 || mode > 2) return S2T_EINVAL;
    if (Uh < 0 || Uh > S2T_TEXT_MAX_UNITS || Ur < 0 || Ur > S2T_TEXT_MAX_UNITS) return S2T_EINVAL;
    if (Hmax > S2T_CHRF_MAX_LEN || Rmax > S2T_CHRF_MAX_LEN) return S2T_ENOTSUP;
    UnitArgs p;
    p.hyp = hyp; p.hyp_len = hyp_len; p.ref = ref; p.ref_len = ref_len; p.hyp_row = hyp_row; p.ref_row = ref_row;
    p.pieces = pieces; p.piece_off = piece_off; p.unk = unk; p.V = V; p.n_pieces = n_pieces;
    p.hyp_units = hyp_units; p.ref_units = ref_units; p.hyp_n = hyp_n; p.ref_n = ref_n; p.status = status;
    p.hyp_elem = hyp_elem; p.ref_elem = ref_elem; p.Hmax = Hmax; p.Rmax = Rmax; p.Hrows = Hrows; p.Rrows = Rrows;
    p.mode = mode; p.Uh = Uh; p.Ur = Ur;
    hipStream_t st = (hipStream_t)stream;
    return (Hmax > Rmax ? Hmax : Rmax) <= S2T_CHRF_GROUP_LEN ? text_units_launch<4>(st, P, p) : text_units_launch<16>(st, P, p);
}
