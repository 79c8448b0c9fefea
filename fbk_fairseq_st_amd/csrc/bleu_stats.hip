// BLEU n-gram statistics of token-sequence pairs (include/s2t_hip.h: s2t_bleu_stats states the rule): the trimmed lengths and, for
// the orders 1 to 4, the clipped n-gram matches and the hypothesis' n-gram totals -- bleu_add of the reference's libbleu without its
// map of hashes: n-grams are compared token by token.
// One launch, one sentence per workgroup, no atomics, no host read.
//   * Prologue: both sides are trimmed inside their lengths (ballots give the first non-pad token and the last token that is
//     neither eos nor pad) and the trimmed tokens are staged in LDS, four zeroed slots behind each side.
//   * Position-wise matching, the loops of ngram_match.hpp (which states the rule and why the windows may read the slack slots): a
//     lane owns position i with hyp[i .. i+3] in registers and takes cref over all reference positions (BLEU_CREF), then rank over
//     the hypothesis positions in front of it (BLEU_RANK).
//   * Clipping: the window of position i is cut at the hypothesis' end and at its first `unk` (an n-gram with an unk in the
//     hypothesis can only equal one with an unk in the reference, which never matches); that cut is applied once, after the loops.
//   * Wave form (Hmax <= 64): one wave, lane = position.  Workgroup form: 256 threads up to Hmax = 256, 1,024 threads above (thread
//     t owns the positions t + 1,024 q); the waves never meet between the staging barrier and the final sum.  A wave's loop waits
//     for its LDS broadcast every step, so a long hypothesis wants several waves on each of the CU's four SIMDs.
//   * Tokens are staged as 32-bit when both sides are int32 and as 64-bit otherwise (dynamic LDS, up to 2 x 4,099 x 8 bytes).
#include "ngram_match.hpp"
#include "s2t_hip.h"

namespace {

struct BleuArgs {
    const void* hyp; const void* hyp_len; const void* ref; const void* ref_len;
    const int* ref_row;
    int* stats; int* status;
    long long pad, eos, unk;
    int hyp_elem, ref_elem, Hmax, Rmax, Rrows;
};

constexpr int BLEU_SLACK = 4;                                       // zeroed slots behind a staged side: windows may read them

// what one wave sees of a side: the first index that is not pad (len if none) and the last that is neither eos nor pad (-1 if none)
template <int NW>
__device__ __forceinline__ void bleu_scan(const char* row, int es, int len, long long pad, long long eos, int& first, int& last) {
    const int tid = threadIdx.x, wave = tid >> 6;
    first = len; last = -1;
    for (int t0 = 0; t0 < len; t0 += 64 * NW) {
        const int t = t0 + tid;
        const long long x = t < len ? int_at(row, es, t) : pad;
        const unsigned long long np = __ballot(t < len && x != pad);
        const unsigned long long kp = __ballot(t < len && x != pad && x != eos);
        const int base = t0 + 64 * wave;
        if (np && first == len) first = base + __ffsll(np) - 1;
        if (kp) last = base + 63 - __clzll(kp);
    }
}

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void bleu_stats_kernel(const BleuArgs p) {
    extern __shared__ __attribute__((aligned(16))) char bleu_smem[];
    __shared__ int s_red[NW][4];
    constexpr int NT = 64 * NW;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* out = p.stats + (size_t)b * 10;

    const long long hq = int_at(p.hyp_len, p.hyp_elem, b);
    const long long rowq = p.ref_row ? (long long)p.ref_row[b] : (long long)b;
    bool refused = hq < 0 || hq > p.Hmax || rowq < 0 || rowq >= p.Rrows;
    const long long rq = refused ? 0 : int_at(p.ref_len, p.ref_elem, rowq);
    refused = refused || rq < 0 || rq > p.Rmax;
    if (refused) {                                                  // the same in every thread of the workgroup
        if (tid < 10) out[tid] = 0;
        if (tid == 0) p.status[b] = 2;
        return;
    }
    const char* hrow = reinterpret_cast<const char*>(p.hyp) + (size_t)b * p.Hmax * p.hyp_elem;
    const char* rrow = reinterpret_cast<const char*>(p.ref) + (size_t)rowq * p.Rmax * p.ref_elem;

    // ---- trim
    int hf, hl, rf, rl;
    bleu_scan<NW>(hrow, p.hyp_elem, (int)hq, p.pad, p.eos, hf, hl);
    bleu_scan<NW>(rrow, p.ref_elem, (int)rq, p.pad, p.eos, rf, rl);
    if (NW > 1) {
        if (lane == 0) { s_red[wave][0] = hf; s_red[wave][1] = hl; s_red[wave][2] = rf; s_red[wave][3] = rl; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            hf = min(hf, s_red[w][0]); hl = max(hl, s_red[w][1]);
            rf = min(rf, s_red[w][2]); rl = max(rl, s_red[w][3]);
        }
    }
    // a side that is only pads is empty; otherwise the first remaining token is kept whatever it is
    // (the same in every lane: said so, for scalar loop counters)
    const int H = __builtin_amdgcn_readfirstlane(hf >= (int)hq ? 0 : max(hl, hf) - hf + 1);
    const int R = __builtin_amdgcn_readfirstlane(rf >= (int)rq ? 0 : max(rl, rf) - rf + 1);

    // ---- stage the trimmed tokens
    T* hs = reinterpret_cast<T*>(bleu_smem);
    T* rs = hs + p.Hmax + BLEU_SLACK;
    for (int t = tid; t < H + BLEU_SLACK; t += NT) hs[t] = t < H ? (T)int_at(hrow, p.hyp_elem, hf + t) : (T)0;
    for (int t = tid; t < R + BLEU_SLACK; t += NT) rs[t] = t < R ? (T)int_at(rrow, p.ref_elem, rf + t) : (T)0;
    __syncthreads();

    // ---- matches
    const bool unk_on = p.unk >= 0;
    uint32_t m12 = 0, m34 = 0;                                      // match1 | match2 << 16, match3 | match4 << 16 of this lane
    for (int q0 = 64 * wave; q0 < H; q0 += NT) {                    // wave-uniform
        const int i = q0 + lane;
        const bool act = i < H;
        const int ii = act ? i : 0;
        const T h0 = hs[ii], h1 = hs[ii + 1], h2 = hs[ii + 2], h3 = hs[ii + 3];
        int clip = act ? min(4, H - i) : 0;                         // the orders this position has
        if (unk_on) {
            const int u = (long long)h0 == p.unk ? 0 : (long long)h1 == p.unk ? 1 : (long long)h2 == p.unk ? 2 : (long long)h3 == p.unk ? 3 : 4;
            clip = min(clip, u);
        }
        int c1 = 0, c2 = 0, c3 = 0, c4 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
        BLEU_CREF(rs, R, c1, c2, c3, c4)                            // reference positions j
        BLEU_RANK(hs, H, q0, i, r1, r2, r3, r4)                     // hypothesis positions k < i
        m12 += (uint32_t)(clip >= 1 && r1 < c1) + ((uint32_t)(clip >= 2 && r2 < c2) << 16);
        m34 += (uint32_t)(clip >= 3 && r3 < c3) + ((uint32_t)(clip >= 4 && r4 < c4) << 16);
    }
    // ---- sum: at most 4,095 per order, the halves do not carry into each other
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m12 += __shfl_xor(m12, o); m34 += __shfl_xor(m34, o); }
    if (NW > 1) {
        __syncthreads();                                            // s_red was read by the trim
        if (lane == 0) { s_red[wave][0] = (int)m12; s_red[wave][1] = (int)m34; }
        __syncthreads();
        m12 = 0; m34 = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { m12 += (uint32_t)s_red[w][0]; m34 += (uint32_t)s_red[w][1]; }
    }
    if (tid == 0) {
        bleu_record(out, R, H, m12, m34);
        p.status[b] = 0;
    }
}

template <typename T, int NW>
int bleu_launch(hipStream_t st, int B, const BleuArgs& p) {
    const size_t lds = ((size_t)p.Hmax + p.Rmax + 2 * BLEU_SLACK) * sizeof(T);
    if (lds > 60000) {                                              // only 64-bit tokens near both limits: asked for on every such call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&bleu_stats_kernel<T, NW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)((2 * S2T_BLEU_MAX_LEN + 2 * BLEU_SLACK) * sizeof(T)));
        if (e != hipSuccess) return S2T_EHIP(e);
    }
    hipLaunchKernelGGL((bleu_stats_kernel<T, NW>), dim3(B), dim3(64 * NW), lds, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

}  // namespace

extern "C" int s2t_bleu_stats(const void* hyp, const void* hyp_len, int hyp_elem, const void* ref, const void* ref_len, int ref_elem,
                              const int* ref_row, int B, int Hmax, int Rmax, int Rrows, long long pad, long long eos, long long unk,
                              int* stats, int* status, void* stream) {
    if (B <= 0) return S2T_OK;
    if (!hyp || !hyp_len || !ref || !ref_len || !stats || !status) return S2T_EINVAL;
    if (Hmax < 0 || Rmax < 0) return S2T_EINVAL;
    if ((hyp_elem != 4 && hyp_elem != 8) || (ref_elem != 4 && ref_elem != 8)) return S2T_EINVAL;
    if (ref_row ? Rrows < 0 : Rrows != B) return S2T_EINVAL;
    if (pad == eos || (unk >= 0 && (unk == pad || unk == eos))) return S2T_EINVAL;
    if (Hmax > S2T_BLEU_MAX_LEN || Rmax > S2T_BLEU_MAX_LEN) return S2T_ENOTSUP;
    BleuArgs p;
    p.hyp = hyp; p.hyp_len = hyp_len; p.ref = ref; p.ref_len = ref_len; p.ref_row = ref_row;
    p.stats = stats; p.status = status;
    p.pad = pad; p.eos = eos; p.unk = unk;
    p.hyp_elem = hyp_elem; p.ref_elem = ref_elem; p.Hmax = Hmax; p.Rmax = Rmax; p.Rrows = Rrows;
    hipStream_t st = (hipStream_t)stream;
    const bool narrow = hyp_elem == 4 && ref_elem == 4;
    if (Hmax <= S2T_BLEU_WAVE_LEN) return narrow ? bleu_launch<int, 1>(st, B, p) : bleu_launch<long long, 1>(st, B, p);
    if (Hmax <= S2T_BLEU_GROUP_LEN) return narrow ? bleu_launch<int, 4>(st, B, p) : bleu_launch<long long, 4>(st, B, p);
    return narrow ? bleu_launch<int, 16>(st, B, p) : bleu_launch<long long, 16>(st, B, p);
}
