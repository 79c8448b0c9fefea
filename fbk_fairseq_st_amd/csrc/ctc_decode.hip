// CTC decoding: transcripts from the encoder's CTC logits (include/s2t_hip.h: s2t_ctc_greedy, s2t_ctc_prefix_beam).
// Greedy is the best path (per-frame arg-max, runs collapsed, blanks dropped) with the frames and the score of every token; the
// prefix beam search is Hannun et al. 2014 ("First-pass large vocabulary continuous speech recognition using bi-directional
// recurrent DNNs") without a language model, in natural-log space.
//
// Both follow the device search's split:
//   * a row phase, one wave per (t, b) row with 16-byte loads: the row's maximum and its first index, the sum of exp over the
//     OTHER columns (so that log-probabilities near 0 keep their relative precision: lp = (x - m) - log1p(R); ctc_rows.hpp's
//     row_max_lse, the statistic ctc_align.hip and ctc_segment.hip take too), the blank's lp and
//     -- for the beam search -- the `cand` non-blank columns of highest logit, one more sweep of the L2-resident row for each;
//   * a sentence phase, one wave per sentence, that walks the frames.  No atomics, no host read between the two launches.
// A prefix of the beam search is identified by its token STRING (a 64-bit hash of the string plus its length), never by the entry
// it was extended from: the extension of p and the blank / repeat updates of a live p+c are one entry, also when p itself was
// pruned and re-created from its own parent while p+c stayed live.  The strings themselves live in a trie of (parent, token) nodes
// in the workspace, at most T*beam per sentence, read back once at the end.
#include "common.hpp"
#include "ctc_rows.hpp"
#include "s2t_hip.h"

namespace {

constexpr int CTCD_MAX_BEAM = 16, CTCD_MAX_CAND = 16;
constexpr int CTCD_SLOTS = (CTCD_MAX_BEAM * (CTCD_MAX_CAND + 1) + 63) / 64;        // candidate entries per lane: 272 over 64 lanes

// ------------------------------------------------------------------ row phase
// arg / arg_lp [T*B]: first index of the row's maximum and its log-probability (greedy; may be NULL);
// cidx / clp [T*B][cand], lpb [T*B]: the cand best non-blank columns, best first, and the blank's log-probability (beam search).
// Rows t >= in_len[b] are skipped: nothing reads them.
template <typename T>
__global__ __launch_bounds__(256) void ctc_decode_row_kernel(const T* __restrict__ logits, const int* __restrict__ in_len,
                                                             int* __restrict__ arg, float* __restrict__ arg_lp, int* __restrict__ cidx,
                                                             float* __restrict__ clp, float* __restrict__ lpb, int Tn, int B, int V, int ld,
                                                             int blank, int cand) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)Tn * B) return;                               // whole waves leave: nothing below synchronises the workgroup
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    if (t >= in_len[b]) return;
    const T* x = logits + row * ld;
    const RowStat st = row_max_lse<T, false>(x, V, lane);
    if (lane == 0) {
        if (arg) { arg[row] = st.mi; arg_lp[row] = -st.lse1; }
        if (lpb) lpb[row] = (to_f32(x[blank]) - st.m) - st.lse1;
    }
    float pv = INFINITY; int pi = -1;                              // the previous pick: the next one comes strictly after it
    for (int r = 0; r < cand; ++r) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        row_for_each<T>(x, V, lane, [&](float v, int j) {
            if (j != blank && (v < pv || (v == pv && j > pi)) && (bi == 0x7fffffff || v > bv || (v == bv && j < bi))) { bv = v; bi = j; }
        });
        wave_best(bv, bi);
        const bool none = bi == 0x7fffffff;                        // fewer than cand comparable columns (NaN logits): no candidate
        if (lane == 0) { cidx[row * cand + r] = none ? -1 : bi; clp[row * cand + r] = none ? -INFINITY : (bv - st.m) - st.lse1; }
        pv = none ? -INFINITY : bv; pi = bi;                      // after `none` every later round finds none too: all cand slots are written
    }
}

// ------------------------------------------------------------------ greedy: collapse of one sentence by one wave
// 64 frames per step.  A run's score is a segmented inclusive scan inside the step plus the carry of a run that began in an
// earlier step; the run's last frame writes it.  Token j of a run = non-blank run heads seen so far - 1.
__global__ __launch_bounds__(64) void ctc_greedy_collapse_kernel(const int* __restrict__ arg, const float* __restrict__ arg_lp,
                                                                 const int* __restrict__ in_len, int* __restrict__ tokens,
                                                                 int* __restrict__ n_tok, int* __restrict__ frames,
                                                                 float* __restrict__ tok_score, float* __restrict__ score,
                                                                 int Tn, int B, int blank) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int L = min(max(in_len[b], 0), Tn);
    int* tk = tokens + (long)b * Tn; int* fr = frames + (long)b * Tn * 2; float* ts = tok_score + (long)b * Tn;
    const unsigned long long le = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull);
    int tbase = 0;
    float carry = 0.f, total = 0.f;
    for (int t0 = 0; t0 < L; t0 += 64) {
        const int t = t0 + lane;
        const bool valid = t < L;
        const int p = valid ? arg[(long)t * B + b] : -1;
        const float lp = valid ? arg_lp[(long)t * B + b] : 0.f;
        int prev = __shfl_up(p, 1), next = __shfl_down(p, 1);
        if (lane == 0) prev = t0 > 0 ? arg[(long)(t0 - 1) * B + b] : -2;
        if (lane == 63) next = t + 1 < L ? arg[(long)(t + 1) * B + b] : -1;
        const bool head = valid && p != prev, tail = valid && p != next;
        const unsigned long long heads = __ballot(head), tokheads = __ballot(head && p != blank);
        const int hc = valid ? __popcll(heads & le) : -1;          // 0: the run came in from the step before
        float v = lp;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_up(v, o); const int oh = __shfl_up(hc, o);
            if (lane >= o && oh == hc) v += ov;
        }
        if (hc == 0) v += carry;
        const int j = tbase + __popcll(tokheads & le) - 1;
        if (head && p != blank) { tk[j] = p; fr[2 * j] = t; }
        if (tail && p != blank) { fr[2 * j + 1] = t + 1; ts[j] = v; }
        carry = __shfl(v, 63);
        tbase += __popcll(tokheads);
        total += lp;
    }
    total = wave_sum(total);
    if (lane == 0) { score[b] = total; n_tok[b] = tbase; }
}

// ------------------------------------------------------------------ prefix beam search: one sentence, one wave
struct Live {                                                       // the live prefixes, best first
    unsigned long long hash[CTCD_MAX_BEAM], phash[CTCD_MAX_BEAM];   // of the string, of the string without its last token
    int len[CTCD_MAX_BEAM], last[CTCD_MAX_BEAM], node[CTCD_MAX_BEAM];                 // node: trie node of the string (0 = empty)
    float pb[CTCD_MAX_BEAM], pnb[CTCD_MAX_BEAM], tot[CTCD_MAX_BEAM];
};

__device__ __forceinline__ unsigned long long str_hash(unsigned long long h, int c) {
    h = (h ^ (unsigned long long)(unsigned)(c + 1)) * 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return h + 0x9E3779B97F4A7C15ull;
}
__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return m;
    return m + log1pf(expf(-fabsf(a - b)));
}

__global__ __launch_bounds__(64) void ctc_prefix_beam_kernel(const int* __restrict__ cidx, const float* __restrict__ clp,
                                                             const float* __restrict__ lpb, const int* __restrict__ in_len, int* trie,
                                                             int* __restrict__ tokens, int* __restrict__ lens, float* __restrict__ scores,
                                                             int* __restrict__ n_hyp, int Tn, int B, int beam, int cand, int nbest) {
    __shared__ Live lv[2];
    __shared__ int s_ci[CTCD_MAX_CAND];
    __shared__ float s_cl[CTCD_MAX_CAND];
    __shared__ float s_lpb;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int L = min(max(in_len[b], 0), Tn);
    int* tr = trie + (long)b * Tn * beam * 2;                       // node n >= 1 at tr[2 (n - 1)]: (parent node, token)
    const int C1 = cand + 1;
    if (lane == 0) {
        Live& r = lv[0];
        r.hash[0] = 0x243F6A8885A308D3ull; r.phash[0] = 0; r.len[0] = 0; r.last[0] = -1; r.node[0] = 0;
        r.pb[0] = 0.f; r.pnb[0] = -INFINITY; r.tot[0] = 0.f;
    }
    int nlive = 1, cur = 0;
    int r_ci = -1; float r_cl = -INFINITY, r_lpb = 0.f;            // the next frame's row, requested one frame ahead
    auto fetch = [&](int t) {
        const long row = (long)t * B + b;
        if (lane < cand) { r_ci = cidx[row * cand + lane]; r_cl = clp[row * cand + lane]; }
        if (lane == 0) r_lpb = lpb[row];
    };
    if (L > 0) fetch(0);
    for (int t = 0; t < L; ++t) {
        if (lane < cand) { s_ci[lane] = r_ci; s_cl[lane] = r_cl; }
        if (lane == 0) s_lpb = r_lpb;
        __syncthreads();
        if (t + 1 < L) fetch(t + 1);
        const Live& src = lv[cur];
        Live& dst = lv[cur ^ 1];
        // entry e = p * (cand + 1) + k: k = 0 the prefix p itself, k >= 1 its extension by candidate k - 1
        const int nent = nlive * C1;
        float epb[CTCD_SLOTS], epnb[CTCD_SLOTS], etot[CTCD_SLOTS];
#pragma unroll
        for (int s = 0; s < CTCD_SLOTS; ++s) {
            epb[s] = epnb[s] = etot[s] = -INFINITY;
            const int e = lane + 64 * s;
            if (e >= nent) continue;
            const int p = e / C1, k = e - p * C1;
            if (k == 0) {
                const int last = src.last[p];
                float lpl = -INFINITY;                              // lp of the prefix' last token if it is a candidate of this frame
                for (int j = 0; j < cand; ++j) if (s_ci[j] == last && last >= 0) lpl = s_cl[j];
                epb[s] = s_lpb + src.tot[p];
                if (lpl > -INFINITY) {
                    epnb[s] = lpl + src.pnb[p];
                    // the extension of the live parent string by `last` is this very prefix
                    for (int q = 0; q < nlive; ++q)
                        if (src.hash[q] == src.phash[p] && src.len[q] == src.len[p] - 1)
                            epnb[s] = logaddexp_f(epnb[s], lpl + (src.last[q] == last ? src.pb[q] : src.tot[q]));
                }
                etot[s] = logaddexp_f(epb[s], epnb[s]);
            } else {
                const int c = s_ci[k - 1];
                if (c < 0) continue;
                const unsigned long long h = str_hash(src.hash[p], c);
                bool dup = false;                                   // p + c is live: its own entry took this contribution above
                for (int q = 0; q < nlive; ++q) dup = dup || (src.hash[q] == h && src.len[q] == src.len[p] + 1);
                if (dup) continue;
                epnb[s] = s_cl[k - 1] + (c == src.last[p] ? src.pb[p] : src.tot[p]);
                etot[s] = epnb[s];
            }
        }
        // the beam highest totals, best first (exact float ties: the lower entry)
        int nnew = 0;
        for (int r = 0; r < beam; ++r) {
            float bv = -INFINITY; int bs = -1;
#pragma unroll
            for (int s = 0; s < CTCD_SLOTS; ++s) if (etot[s] > bv) { bv = etot[s]; bs = s; }
            int be = bs >= 0 ? lane + 64 * bs : 0x7fffffff;
            wave_best(bv, be);
            if (be == 0x7fffffff) break;                            // wave-uniform: fewer than beam prefixes exist
            if (lane == (be & 63)) {
                const int ws = be >> 6;
                float wpb = -INFINITY, wpnb = -INFINITY;
#pragma unroll
                for (int s = 0; s < CTCD_SLOTS; ++s) if (s == ws) { wpb = epb[s]; wpnb = epnb[s]; etot[s] = -INFINITY; }
                const int p = be / C1, k = be - p * C1;
                if (k == 0) {
                    dst.hash[r] = src.hash[p]; dst.phash[r] = src.phash[p]; dst.len[r] = src.len[p]; dst.last[r] = src.last[p];
                    dst.node[r] = src.node[p];
                } else {
                    const int c = s_ci[k - 1];
                    const int node = 1 + t * beam + r;
                    dst.hash[r] = str_hash(src.hash[p], c); dst.phash[r] = src.hash[p]; dst.len[r] = src.len[p] + 1; dst.last[r] = c;
                    dst.node[r] = node;
                    tr[2 * (node - 1)] = src.node[p]; tr[2 * (node - 1) + 1] = c;
                }
                dst.pb[r] = wpb; dst.pnb[r] = wpnb; dst.tot[r] = bv;
            }
            ++nnew;
        }
        __syncthreads();
        cur ^= 1; nlive = nnew;
    }
    __threadfence();                                                // the trie was written by other lanes of this wave
    __syncthreads();
    const Live& fin = lv[cur];
    const int count = min(nbest, nlive);
    if (lane == 0) n_hyp[b] = count;
    if (lane < nbest) {
        const long o = (long)b * nbest + lane;
        if (lane >= count) { lens[o] = 0; scores[o] = -INFINITY; }
        else {
            const int n = fin.len[lane];
            lens[o] = n; scores[o] = fin.tot[lane];
            int node = fin.node[lane];
            int* out = tokens + o * Tn;
            for (int i = n - 1; i >= 0 && node > 0; --i) {
                out[i] = __hip_atomic_load(tr + 2 * (node - 1) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                node = __hip_atomic_load(tr + 2 * (node - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// argument checks shared by both entry points: 1 = nothing to do, 0 = go on, < 0 = refused
int ctc_decode_check(int dtype, const void* logits, const int* in_len, const void* ws, int T, int B, int V, int ld, int blank) {
    if ((long)T * B <= 0 || T <= 0) return 1;
    if (!logits || !in_len || !ws || V < 2 || ld < V || blank < 0 || blank >= V) return S2T_EINVAL;
    if ((long)T * B > 0x7fffffffL) return S2T_EINVAL;
    if (dtype != S2T_F32 && dtype != S2T_BF16) return S2T_ENOTSUP;
    return 0;
}

void ctc_decode_rows(int dtype, const void* logits, const int* in_len, int* arg, float* arg_lp, int* cidx, float* clp, float* lpb,
                     int T, int B, int V, int ld, int blank, int cand, hipStream_t st) {
    const dim3 grid((unsigned)(((long)T * B + 3) / 4));
    if (dtype == S2T_BF16)
        hipLaunchKernelGGL(ctc_decode_row_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, in_len, arg, arg_lp, cidx, clp, lpb, T, B, V, ld, blank, cand);
    else
        hipLaunchKernelGGL(ctc_decode_row_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, in_len, arg, arg_lp, cidx, clp, lpb, T, B, V, ld, blank, cand);
}

}  // namespace

extern "C" size_t s2t_ctc_greedy_workspace(int T, int B) {
    if (T <= 0 || B <= 0) return 0;
    return (size_t)8 * (size_t)T * (size_t)B;
}

extern "C" int s2t_ctc_greedy(int dtype, const void* logits, const int* in_len, void* ws, int* tokens, int* n_tok, int* frames,
                              float* tok_score, float* score, int T, int B, int V, int ld, int blank, void* stream) {
    const int rc = ctc_decode_check(dtype, logits, in_len, ws, T, B, V, ld, blank);
    if (rc) return rc > 0 ? S2T_OK : rc;
    if (!tokens || !n_tok || !frames || !tok_score || !score) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* arg = (int*)ws;
    float* arg_lp = (float*)ws + (size_t)T * B;
    ctc_decode_rows(dtype, logits, in_len, arg, arg_lp, nullptr, nullptr, nullptr, T, B, V, ld, blank, 0, st);
    S2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_greedy_collapse_kernel, dim3(B), dim3(64), 0, st, arg, arg_lp, in_len, tokens, n_tok, frames, tok_score, score, T, B, blank);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" size_t s2t_ctc_prefix_beam_workspace(int T, int B, int beam, int cand, int nbest) {
    (void)nbest;
    if (T <= 0 || B <= 0 || beam < 1 || cand < 1) return 0;
    const size_t bytes = (size_t)4 * (size_t)T * (size_t)B * (size_t)(2 * beam + 2 * cand + 1);
    return (bytes + 255) / 256 * 256;
}

extern "C" int s2t_ctc_prefix_beam(int dtype, const void* logits, const int* in_len, void* ws, int* tokens, int* lens, float* scores,
                                   int* n_hyp, int T, int B, int V, int ld, int blank, int beam, int cand, int nbest, void* stream) {
    const int rc = ctc_decode_check(dtype, logits, in_len, ws, T, B, V, ld, blank);
    if (rc) return rc > 0 ? S2T_OK : rc;
    if (!tokens || !lens || !scores || !n_hyp || beam < 1 || cand < 1 || nbest < 1 || nbest > beam) return S2T_EINVAL;
    if (beam > CTCD_MAX_BEAM || cand > CTCD_MAX_CAND || cand > V - 1) return S2T_ENOTSUP;
    if ((long)T * beam > 0x3fffffffL) return S2T_ENOTSUP;          // trie node ids are ints
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)T * B;
    int* trie = (int*)ws;                                           // [B][T*beam][2]
    int* cidx = trie + rows * beam * 2;                             // [rows][cand]
    float* clp = (float*)(cidx + rows * cand);                      // [rows][cand]
    float* lpb = clp + rows * cand;                                 // [rows]
    ctc_decode_rows(dtype, logits, in_len, nullptr, nullptr, cidx, clp, lpb, T, B, V, ld, blank, cand, st);
    S2T_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_prefix_beam_kernel, dim3(B), dim3(64), 0, st, cidx, clp, lpb, in_len, trie, tokens, lens, scores, n_hyp, T, B, beam, cand, nbest);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
