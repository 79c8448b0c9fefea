// BLEU n-gram statistics of every candidate against every pseudo-reference of its sentence (include/s2t_hip.h: s2t_bleu_pairs; the
// rule of a pair is s2t_bleu_stats's): the pairwise step of minimum-Bayes-risk selection over n-best lists.
// One launch, one candidate position per thread, no atomics, no host read, no memset.  A workgroup takes one candidate row
// (blockIdx.x) and a slice of S2T_MBR_SLICE entries of its list (blockIdx.y): one workgroup per candidate for the whole list is one
// wave per SIMD at 16 x 64 hypotheses of 60 tokens, and a wave's loop waits for its LDS broadcast every step; the slice costs the
// candidate's half of the work once more per slice (measured: DESIGN.md 5i).
//   * What bleu_stats.hip does per pair is split here into the half that depends on the candidate only and the half that depends on
//     the pair (ngram_match.hpp states the rule and holds the loops both files run): rank_n(i) needs the candidate alone,
//     cref_n(i, r) the pseudo-reference r.  The candidate is staged and trimmed once per workgroup and every thread takes its four
//     ranks once (BLEU_RANK); they stay in registers while the workgroup walks its slice.
//   * Staging: rows are copied to LDS as they lie in memory (a chunk of pseudo-references is one span of the matrix, copied in whole
//     padded rows: no load waits for a length or for another load); the trim is taken afterwards, in LDS, as a first index and a
//     length (a scan from both ends that usually ends after a step or two), so nothing is moved and no ballot is needed.
//     Windows may read up to three tokens behind a trimmed row: those are inside the row's four slack slots, which are not
//     zeroed here (ngram_match.hpp: they may hold anything).
//   * The slice is walked in chunks of S2T_MBR_CHUNK pseudo-references (the header's switch: as many padded rows as
//     S2T_MBR_CHUNK_BYTES hold, at most the slice).  Per chunk: every thread copies its share of the chunk's rows; barrier;
//     lane g of every wave trims row g (each wave for itself: the lengths come out of a lane by v_readlane, nothing is exchanged);
//     every wave that holds candidate positions runs BLEU_CREF, the j loop of bleu_stats.hip, over each row, with wave-uniform
//     bounds and LDS broadcasts, and turns its lanes' four match bits into counts by ballots.  One wave (Hmax <= 64) writes the ten
//     numbers from there.  Several waves leave their counts in LDS; behind a second barrier thread g sums row g's and writes its
//     ten numbers while the others already copy the next chunk, if there is one: the rows are free once every wave is past that
//     barrier, and the counts are read before their reader arrives at the next chunk's first barrier.
//   * A candidate `unk` cuts the window of its position (`clip`), as in bleu_stats.hip: an n-gram with an unk can only equal one
//     with an unk on the reference side, which never matches.
//   * Tokens are staged as 32-bit when both sides are int32 and as 64-bit otherwise.
#include "ngram_match.hpp"
#include "s2t_hip.h"

#ifndef MBR_SLICE                                                   // a measurement twin is built with another (tools/mbr_time.py)
#define MBR_SLICE S2T_MBR_SLICE
#endif

namespace {

struct PairArgs {
    const void* cand; const void* cand_len; const void* ref; const void* ref_len;
    const int* cand_sent; const int* ref_off;
    int* stats; int* status;
    long long pad, eos, unk;
    int cand_elem, ref_elem, B, Hmax, Pmax, Rr, M, chunk;
};

constexpr int MBR_SLACK = 4;                                        // slots behind a staged row: windows may read three of them

// the trim of a staged row of `len` tokens: the first index that is not pad and the length up to the last token that is neither eos
// nor pad, never less than 1; 0 for a row of pads
template <typename T>
__device__ __forceinline__ void pair_trim(const T* row, int len, long long pad, long long eos, int& first, int& n) {
    int f = 0;
    while (f < len && (long long)row[f] == pad) ++f;
    int l = len - 1;
    while (l > f && ((long long)row[l] == eos || (long long)row[l] == pad)) --l;
    first = f;
    n = f >= len ? 0 : l - f + 1;
}

template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void bleu_pairs_kernel(const PairArgs p) {
    extern __shared__ __attribute__((aligned(16))) char pair_smem[];
    __shared__ uint32_t s_part[NW > 1 ? MBR_SLICE : 1][NW][2];
    constexpr int NT = 64 * NW;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = p.M;
    int* out = p.stats + (size_t)c * M * 10;
    int* st = p.status + (size_t)c * M;

    // ---- the candidate's list; what is refused (the same in every thread of the workgroup)
    const long long hq = int_at(p.cand_len, p.cand_elem, c);
    const int sent = p.cand_sent[c];
    int lo = 0, n = -1;                                             // n: the list's length, -1 for a row without a list
    if (sent >= 0 && sent < p.B) {
        lo = p.ref_off[sent];
        const int hi = p.ref_off[sent + 1];
        if (lo >= 0 && hi >= lo && hi <= p.Rr && hi - lo <= M) n = hi - lo;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);                        // the same in every lane: said so, for scalar loop counters
    n = __builtin_amdgcn_readfirstlane(n);
    const bool cand_bad = hq < 0 || hq > p.Hmax;
    const int k0 = blockIdx.y * MBR_SLICE, k1 = min(k0 + MBR_SLICE, M);   // this workgroup's slice of the M entries
    if (n < 0 || cand_bad) {
        const int bad = n < 0 ? M : n;
        for (int t = k0 * 10 + tid; t < k1 * 10; t += NT) out[t] = 0;
        for (int t = k0 + tid; t < k1; t += NT) st[t] = t < bad ? 2 : 0;
        return;
    }
    for (int t = max(n, k0) * 10 + tid; t < k1 * 10; t += NT) out[t] = 0;   // behind the list
    for (int t = max(n, k0) + tid; t < k1; t += NT) st[t] = 0;
    const int gend = min(n, k1);
    if (k0 >= gend) return;

    // ---- the candidate: staged as it lies, trimmed in LDS (every thread takes the same steps: LDS broadcasts)
    const int hstride = p.Hmax + MBR_SLACK, rstride = p.Pmax + MBR_SLACK;
    T* hs = reinterpret_cast<T*>(pair_smem);
    T* rs = hs + hstride;
    {
        const char* hrow = reinterpret_cast<const char*>(p.cand) + (size_t)c * p.Hmax * p.cand_elem;
        for (int t = tid; t < (int)hq; t += NT) hs[t] = (T)int_at(hrow, p.cand_elem, t);
    }
    __syncthreads();
    int hf, H;
    pair_trim(hs, (int)hq, p.pad, p.eos, hf, H);
    hf = __builtin_amdgcn_readfirstlane(hf);
    H = __builtin_amdgcn_readfirstlane(H);
    const T* ht = hs + hf;

    // ---- this thread's position: its window, the orders it has, its four ranks
    const int q0 = 64 * wave, i = tid;
    const bool act = i < H;
    const int ii = act ? i : 0;
    const T h0 = ht[ii], h1 = ht[ii + 1], h2 = ht[ii + 2], h3 = ht[ii + 3];
    int clip = act ? min(4, H - i) : 0;
    if (p.unk >= 0) {
        const int u = (long long)h0 == p.unk ? 0 : (long long)h1 == p.unk ? 1 : (long long)h2 == p.unk ? 2 : (long long)h3 == p.unk ? 3 : 4;
        clip = min(clip, u);
    }
    int r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    if (q0 < H) BLEU_RANK(ht, H, q0, i, r1, r2, r3, r4)             // candidate positions k < i, once for the whole list

    // ---- the list, a chunk at a time
    for (int g0 = k0; g0 < gend; g0 += p.chunk) {                   // uniform
        const int G = min(p.chunk, gend - g0);
        // copy: the chunk's rows are one span of the matrix; whole padded rows, so that no load waits for a length
        {
            const char* span = reinterpret_cast<const char*>(p.ref) + (size_t)(lo + g0) * p.Pmax * p.ref_elem;
            const int total = G * p.Pmax;
#pragma clang loop unroll_count(8)
            for (int e = tid; e < total; e += NT) {
                const int g = e / p.Pmax;
                rs[e + g * MBR_SLACK] = (T)int_at(span, p.ref_elem, e);
            }
        }
        __syncthreads();
        // trim: lane g of every wave takes row g
        int rf = 0, R = 0;
        bool rbad = false;
        if (lane < G) {
            const long long rq = int_at(p.ref_len, p.ref_elem, (size_t)(lo + g0 + lane));
            rbad = rq < 0 || rq > p.Pmax;
            if (!rbad) pair_trim(rs + lane * rstride, (int)rq, p.pad, p.eos, rf, R);
        }
        for (int g = 0; g < G; ++g) {                               // uniform
            const int Rg = __builtin_amdgcn_readlane(R, g);
            uint32_t m12 = 0, m34 = 0;                              // match1 | match2 << 16, match3 | match4 << 16 of this wave
            if (q0 < H) {
                const T* rt = rs + g * rstride + __builtin_amdgcn_readlane(rf, g);
                int c1 = 0, c2 = 0, c3 = 0, c4 = 0;
                BLEU_CREF(rt, Rg, c1, c2, c3, c4)
                m12 = (uint32_t)__popcll(__ballot(clip >= 1 && r1 < c1)) | ((uint32_t)__popcll(__ballot(clip >= 2 && r2 < c2)) << 16);
                m34 = (uint32_t)__popcll(__ballot(clip >= 3 && r3 < c3)) | ((uint32_t)__popcll(__ballot(clip >= 4 && r4 < c4)) << 16);
            }
            if (NW > 1) {
                if (lane == 0) { s_part[g][wave][0] = m12; s_part[g][wave][1] = m34; }
            } else {
                const bool bad = __builtin_amdgcn_readlane((int)rbad, g) != 0;
                // bleu_record's ten numbers, one per lane: lane 0 reflen, lane 1 predlen; lanes 2 n and 2 n + 1 match_n and count_n
                const int ord = lane >> 1;
                const int v = lane & 1 ? (lane == 1 ? H : max(H - ord + 1, 0))
                                       : lane == 0 ? Rg : ord == 1 ? (int)(m12 & 0xffff) : ord == 2 ? (int)(m12 >> 16) : ord == 3 ? (int)(m34 & 0xffff) : (int)(m34 >> 16);
                int* o = out + (size_t)(g0 + g) * 10;
                if (lane < 10) o[lane] = bad ? 0 : v;
                if (lane == 10) st[g0 + g] = bad ? 2 : 0;
            }
        }
        if (NW > 1) {
            __syncthreads();
            if (tid < G) {                                          // wave 0, lane g: it holds row g's trim
                uint32_t m12 = 0, m34 = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) { m12 += s_part[tid][w][0]; m34 += s_part[tid][w][1]; }
                int* o = out + (size_t)(g0 + tid) * 10;
                if (rbad) {
#pragma unroll
                    for (int q = 0; q < 10; ++q) o[q] = 0;
                } else {
                    bleu_record(o, R, H, m12, m34);
                }
                st[g0 + tid] = rbad ? 2 : 0;
            }
        }
    }
}

template <typename T, int NW>
int pairs_launch(hipStream_t st, int Rc, PairArgs& p) {
    p.chunk = min(S2T_MBR_CHUNK_BYTES / ((p.Pmax + MBR_SLACK) * (int)sizeof(T)), (int)MBR_SLICE);           // S2T_MBR_CHUNK
    const size_t lds = ((size_t)p.Hmax + MBR_SLACK + (size_t)p.chunk * (p.Pmax + MBR_SLACK)) * sizeof(T);   // at most 8 KiB + 32 KiB
    hipLaunchKernelGGL((bleu_pairs_kernel<T, NW>), dim3(Rc, (p.M + MBR_SLICE - 1) / MBR_SLICE), dim3(64 * NW), lds, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

}  // namespace

extern "C" int s2t_bleu_pairs(const void* cand, const void* cand_len, int cand_elem, const void* ref, const void* ref_len, int ref_elem,
                              const int* cand_sent, const int* ref_off, int Rc, int B, int Hmax, int Pmax, int Rr, int M, long long pad,
                              long long eos, long long unk, int* stats, int* status, void* stream) {
    if (Rc <= 0 || M == 0) return S2T_OK;
    if (!cand || !cand_len || !ref || !ref_len || !cand_sent || !ref_off || !stats || !status) return S2T_EINVAL;
    if (Hmax < 0 || Pmax < 0 || B < 0 || Rr < 0 || M < 0) return S2T_EINVAL;
    if ((cand_elem != 4 && cand_elem != 8) || (ref_elem != 4 && ref_elem != 8)) return S2T_EINVAL;
    if (pad == eos || (unk >= 0 && (unk == pad || unk == eos))) return S2T_EINVAL;
    if (Hmax > S2T_MBR_MAX_LEN || Pmax > S2T_MBR_MAX_LEN || M > S2T_MBR_MAX_LIST) return S2T_ENOTSUP;
    PairArgs p;
    p.cand = cand; p.cand_len = cand_len; p.ref = ref; p.ref_len = ref_len; p.cand_sent = cand_sent; p.ref_off = ref_off;
    p.stats = stats; p.status = status;
    p.pad = pad; p.eos = eos; p.unk = unk;
    p.cand_elem = cand_elem; p.ref_elem = ref_elem; p.B = B; p.Hmax = Hmax; p.Pmax = Pmax; p.Rr = Rr; p.M = M; p.chunk = 1;
    hipStream_t st = (hipStream_t)stream;
    const bool narrow = cand_elem == 4 && ref_elem == 4;
    if (Hmax <= S2T_MBR_WAVE_LEN) return narrow ? pairs_launch<int, 1>(st, Rc, p) : pairs_launch<long long, 1>(st, Rc, p);
    if (Hmax <= S2T_MBR_GROUP_LEN) return narrow ? pairs_launch<int, 4>(st, Rc, p) : pairs_launch<long long, 4>(st, Rc, p);
    return narrow ? pairs_launch<int, 16>(st, Rc, p) : pairs_launch<long long, 16>(st, Rc, p);
}
