// Edit-distance alignment of token-sequence pairs (include/s2t_hip.h: s2t_edit_align): cost, the numbers of matches,
// substitutions and tokens left alone on either side, and optionally the path itself, by the rule of wer_utils.EditDistance(False)
// -- diagonal first, then left, then up, both comparisons strict -- under any three integer costs.
// One launch.  A sentence is a pair a (n tokens, the rows) / b (m tokens, the columns 1 .. m; column 0 and row 0 are the borders).
//   * Register form (Bmax + 1 <= 1024): one wave per sentence, lane l owns the K = 1, 2, 4, 8 or 16 consecutive columns
//     l K + 1 .. l K + K in registers.  Rows are skewed across lanes: at step s lane l works on row s - l, so the value left of its
//     run (the last cell lane l - 1 made one step earlier) and the row's `a` token arrive by one lane shift per step; the diagonal
//     value is the left value of the step before.  No barrier and no LDS in the loop.
//   * Workgroup form (Bmax <= S2T_EDIT_MAX_B): the same skew over the 256 threads of one workgroup with K = 16; between waves the
//     shifted values cross through a double-buffered LDS slot, one LDS-only barrier per step.
// Counts without a matrix: a cell carries (cost, M | S << 16 | B << 32 | A << 48); the counts of the predecessor the rule chooses,
// plus one, are the cell's counts.  The choice is a function of the three neighbouring costs only, so the counts carried to (n, m)
// are those of the path a back-trace from (n, m) would walk.
// Path output: the 2-bit steps of a row travel with the row through the lanes and are stored one dword per 16 columns; after the
// recursion one wave walks them back from (n, m) through LDS, a block of rows at a time, and writes the codes in forward order
// (the path's length is known from the counts before the walk starts).  Collapse mode: a prologue of the same launch collapses
// repeats and drops the blank, 64 frames at a time (ballot + prefix).  No atomics, no host read.
#include "common.hpp"
#include "s2t_hip.h"

namespace {

constexpr int EDT_STAGE = 4096;                                     // dwords of LDS the backward walk stages steps in (16 KiB)
constexpr int EDT_WALK_ROWS = 64;                                   // rows per block of the walk while a row has <= 64 dwords

struct EditArgs {
    const void* a; const void* a_len; const void* b; const void* b_len;
    void* a_store;                                                  // collapse mode: [B][Amax] collapsed tokens (a_out or workspace)
    uint32_t* bp;                                                   // [B][Amax + 1][W] steps, NULL without `ops`
    int* counts; int* cost; int* status; int* a_n; unsigned char* ops; int* n_ops;
    long long blank;
    int a_elem, b_elem, Amax, Bmax, W, cs, ca, cb, collapse;
};

__device__ __forceinline__ unsigned long long shfl_up_u64(unsigned long long x) {
    const uint32_t lo = __shfl_up((uint32_t)x, 1), hi = __shfl_up((uint32_t)(x >> 32), 1);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long x, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, l), hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

constexpr unsigned long long ONE_M = 1ull, ONE_S = 1ull << 16, ONE_B = 1ull << 32, ONE_A = 1ull << 48;

// NW = 1: the register form (one wave).  NW = 4: the workgroup form (K = 16).
template <int K, int NW>
__global__ __launch_bounds__(64 * NW) void edit_align_kernel(const EditArgs p) {
    __shared__ uint32_t s_bp[EDT_STAGE];
    __shared__ int s_fin[6];
    __shared__ uint32_t s_x[NW][2][6];                              // what lane 63 of a wave hands to lane 0 of the next
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long nq = int_at(p.a_len, p.a_elem, b), mq = int_at(p.b_len, p.b_elem, b);
    if (nq < 0 || nq > p.Amax || mq < 0 || mq > p.Bmax) { if (tid == 0) p.status[b] = 2; return; }
    int n = (int)nq;
    const int m = (int)mq;
    const char* arow = reinterpret_cast<const char*>(p.a) + (size_t)b * p.Amax * p.a_elem;
    const char* brow = reinterpret_cast<const char*>(p.b) + (size_t)b * p.Bmax * p.b_elem;

    // ---- collapse mode: repeats collapsed, then the blank dropped; wave 0, 64 frames at a time
    if (p.collapse) {
        char* dst = reinterpret_cast<char*>(p.a_store) + (size_t)b * p.Amax * p.a_elem;
        if (wave == 0) {
            int base = 0;
            unsigned long long last = 0;
            for (int t0 = 0; t0 < n; t0 += 64) {
                const int t = t0 + lane;
                const unsigned long long x = t < n ? (unsigned long long)int_at(arow, p.a_elem, t) : 0ull;
                unsigned long long prev = shfl_up_u64(x);
                if (lane == 0) prev = last;
                const bool keep = t < n && (t == 0 || x != prev) && (long long)x != p.blank;
                const unsigned long long mask = __ballot(keep);
                if (keep) {
                    const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (p.a_elem == 4) reinterpret_cast<int*>(dst)[at] = (int)x;
                    else reinterpret_cast<long long*>(dst)[at] = (long long)x;
                }
                base += __popcll(mask);
                last = readlane_u64(x, 63);
            }
            if (lane == 0) s_fin[0] = base;
        }
        __threadfence();                                            // the tokens were written by other lanes: complete the stores
        __syncthreads();
        n = s_fin[0];
        __syncthreads();
        arow = dst;
    }
    if (tid == 0 && p.a_n) p.a_n[b] = n;

    int cost = n * p.ca + m * p.cb;                                 // an empty side: the other side's tokens left alone
    int cM = 0, cS = 0, cB = m, cA = n;
    if (n > 0 && m > 0) {
        const int j0 = tid * K;                                     // this thread's columns: j0 + 1 .. j0 + K
        long long bt[K];
        int v[K];
        unsigned long long c[K];
#pragma unroll
        for (int k = 0; k < K; ++k) { bt[k] = j0 + k < m ? int_at(brow, p.b_elem, j0 + k) : 0; v[k] = 0; c[k] = 0; }
        int o_cost = 0, pl_cost = 0;
        unsigned long long o_cnt = 0, o_tok = 0, pl_cnt = 0;
        uint32_t o_acc = 0;
        const int fin_thread = (m - 1) / K, fin_slot = (m - 1) % K;
        // the last thread that has work: with `ops` the one that completes the last dword of 16 columns
        const int steps = n + (p.bp ? ((m - 1) | 15) / K : fin_thread);
        // wave 0 holds the a tokens of 64 steps in a register, one per lane, and requests the next 64 a group ahead
        unsigned long long acur = 0, anxt = 0;
        if (wave == 0) {
            if (lane >= 1 && lane - 1 < n) acur = (unsigned long long)int_at(arow, p.a_elem, lane - 1);
            if (63 + lane < n) anxt = (unsigned long long)int_at(arow, p.a_elem, 63 + lane);
        }
        for (int s = 0; s <= steps; ++s) {
            int in_cost = __shfl_up(o_cost, 1);
            unsigned long long in_cnt = shfl_up_u64(o_cnt), in_tok = shfl_up_u64(o_tok);
            uint32_t in_acc = (K < 16) ? __shfl_up(o_acc, 1) : 0u;
            if (NW > 1 && lane == 0 && wave > 0) {
                const uint32_t* x = s_x[wave - 1][(s + 1) & 1];     // written at step s - 1
                in_cost = (int)x[0];
                in_cnt = ((unsigned long long)x[2] << 32) | x[1];
                in_tok = ((unsigned long long)x[4] << 32) | x[3];
            }
            if (wave == 0) {
                if (s > 0 && (s & 63) == 0) {
                    acur = anxt;
                    anxt = s + 63 + lane < n ? (unsigned long long)int_at(arow, p.a_elem, s + 63 + lane) : 0ull;
                }
                const unsigned long long t0 = readlane_u64(acur, s & 63);     // a[s - 1]
                if (lane == 0) { in_cost = s * p.ca; in_cnt = (unsigned long long)s * ONE_A; in_tok = t0; in_acc = 0; }
            }
            const int i = s - tid;
            if (i == 0) {
#pragma unroll
                for (int k = 0; k < K; ++k) { v[k] = (j0 + k + 1) * p.cb; c[k] = (unsigned long long)(j0 + k + 1) * ONE_B; }
            } else if (i >= 1 && i <= n) {
                int left = in_cost, diag = pl_cost;
                unsigned long long leftc = in_cnt, diagc = pl_cnt;
                uint32_t bits = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int up = v[k];
                    const unsigned long long upc = c[k];
                    const bool eq = (long long)in_tok == bt[k];
                    int best = diag + (eq ? 0 : p.cs);
                    unsigned long long bc = diagc + (eq ? ONE_M : ONE_S);
                    uint32_t code = eq ? 0u : 1u;
                    if (left + p.cb < best) { best = left + p.cb; bc = leftc + ONE_B; code = 2u; }
                    if (up + p.ca < best) { best = up + p.ca; bc = upc + ONE_A; code = 3u; }
                    diag = up; diagc = upc; left = best; leftc = bc;
                    v[k] = best; c[k] = bc;
                    bits |= code << (2 * k);
                }
                if (p.bp) {
                    uint32_t acc = (K == 16 || (j0 & 15) == 0) ? 0u : in_acc;
                    acc |= bits << (2 * (j0 & 15));
                    o_acc = acc;
                    if (((j0 + K) & 15) == 0 && (j0 >> 4) <= ((m - 1) >> 4))
                        p.bp[((size_t)b * (p.Amax + 1) + i) * p.W + (j0 >> 4)] = acc;
                }
                if (i == n && tid == fin_thread) {
                    int fc = 0; unsigned long long fq = 0;
#pragma unroll
                    for (int k = 0; k < K; ++k) if (k == fin_slot) { fc = v[k]; fq = c[k]; }
                    s_fin[0] = fc;
                    s_fin[1] = (int)(fq & 0xffff); s_fin[2] = (int)((fq >> 16) & 0xffff);
                    s_fin[3] = (int)((fq >> 32) & 0xffff); s_fin[4] = (int)((fq >> 48) & 0xffff);
                }
            }
            pl_cost = in_cost; pl_cnt = in_cnt;
            o_cost = v[K - 1]; o_cnt = c[K - 1]; o_tok = in_tok;
            if (NW > 1) {
                if (lane == 63) {
                    uint32_t* x = s_x[wave][s & 1];
                    x[0] = (uint32_t)o_cost;
                    x[1] = (uint32_t)o_cnt; x[2] = (uint32_t)(o_cnt >> 32);
                    x[3] = (uint32_t)o_tok; x[4] = (uint32_t)(o_tok >> 32);
                }
                lds_barrier();                                      // LDS only: the step stores stay in flight across it
            }
        }
        __threadfence();                                            // the steps were stored by other threads of this workgroup
        __syncthreads();
        cost = s_fin[0]; cM = s_fin[1]; cS = s_fin[2]; cB = s_fin[3]; cA = s_fin[4];
    }
    const int P = cM + cS + cB + cA;
    if (tid == 0) {
        p.cost[b] = cost;
        int* cn = p.counts + (size_t)b * 4;
        cn[0] = cM; cn[1] = cS; cn[2] = cB; cn[3] = cA;
        p.status[b] = 0;
        if (p.ops) p.n_ops[b] = P;
    }
    if (!p.ops) return;

    // ---- the path, in forward order
    unsigned char* op = p.ops + (size_t)b * ((size_t)p.Amax + p.Bmax);
    if (n == 0 || m == 0) {
        for (int q = tid; q < P; q += 64 * NW) op[q] = n == 0 ? 2 : 3;
        return;
    }
    const int Wm = ((m - 1) >> 4) + 1;                              // dwords of a row that hold steps of this sentence
    const int RB = Wm <= 64 ? EDT_WALK_ROWS : EDT_STAGE / Wm;
    int i = n, j = m, k = 0;
    uint32_t mine = 0;
    for (int t0 = n / RB * RB; t0 >= 0; t0 -= RB) {
        const int cnt = min(RB, n + 1 - t0);
        __syncthreads();
        for (int q = tid; q < cnt * Wm; q += 64 * NW) {
            const int r = q / Wm, g = q - r * Wm;                   // row 0 holds no steps: staged as zeros, never looked at
            s_bp[q] = t0 + r >= 1 ? p.bp[((size_t)b * (p.Amax + 1) + t0 + r) * p.W + g] : 0u;
        }
        __syncthreads();
        if (wave == 0) {
            while (i >= t0 && (i > 0 || j > 0)) {                   // every lane walks: the reads are LDS broadcasts
                const uint32_t code = i == 0 ? 2u : j == 0 ? 3u : (s_bp[(i - t0) * Wm + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
                if (lane == (k & 63)) mine = code;
                i -= code != 2u; j -= code != 3u;
                ++k;
                if ((k & 63) == 0) {                                // lanes hold steps k - 64 .. k - 1, counted from the path's end
                    const int at = P - 1 - (k - 64 + lane);
                    if (at >= 0) op[at] = (unsigned char)mine;
                }
            }
        }
    }
    if (wave == 0) {
        const int rem = k & 63, at = P - 1 - (k - rem + lane);
        if (lane < rem && at >= 0) op[at] = (unsigned char)mine;
    }
}

inline size_t round256(size_t x) { return (x + 255) / 256 * 256; }
inline size_t edit_tok_bytes(int B, int Amax) { return round256((size_t)8 * (size_t)B * (size_t)Amax); }
inline int edit_words(int Bmax) { return (Bmax + 1 + 15) / 16; }

template <int K, int NW>
void edit_launch(hipStream_t st, int B, const EditArgs& p) {
    hipLaunchKernelGGL((edit_align_kernel<K, NW>), dim3(B), dim3(64 * NW), 0, st, p);
}

}  // namespace

extern "C" size_t s2t_edit_align_workspace(int B, int Amax, int Bmax, int want_ops) {
    if (B <= 0 || Amax < 0 || Bmax < 0 || Amax > S2T_EDIT_MAX_A || Bmax > S2T_EDIT_MAX_B) return 0;
    size_t bytes = edit_tok_bytes(B, Amax);
    if (want_ops) bytes += round256((size_t)4 * (size_t)B * ((size_t)Amax + 1) * (size_t)edit_words(Bmax));
    return bytes;
}

extern "C" int s2t_edit_align(const void* a, const void* a_len, int a_elem, const void* b, const void* b_len, int b_elem, int B, int Amax,
                              int Bmax, int cs, int ca, int cb, int collapse, long long blank, void* ws, int* counts, int* cost,
                              int* status, int* a_n, void* a_out, unsigned char* ops, int* n_ops, void* stream) {
    if (B <= 0) return S2T_OK;
    if (!a || !a_len || !b || !b_len || !counts || !cost || !status) return S2T_EINVAL;
    if (cs < 1 || cs > 255 || ca < 1 || ca > 255 || cb < 1 || cb > 255 || Amax < 0 || Bmax < 0) return S2T_EINVAL;
    if ((a_elem != 4 && a_elem != 8) || (b_elem != 4 && b_elem != 8)) return S2T_EINVAL;
    if (collapse && !a_n) return S2T_EINVAL;
    if (ops && !n_ops) return S2T_EINVAL;
    if ((ops || (collapse && !a_out)) && !ws) return S2T_EINVAL;
    if (Amax > S2T_EDIT_MAX_A || Bmax > S2T_EDIT_MAX_B) return S2T_ENOTSUP;
    EditArgs p;
    p.a = a; p.a_len = a_len; p.b = b; p.b_len = b_len;
    p.a_store = collapse ? (a_out ? a_out : ws) : nullptr;
    p.bp = ops ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws) + edit_tok_bytes(B, Amax)) : nullptr;
    p.counts = counts; p.cost = cost; p.status = status; p.a_n = a_n; p.ops = ops; p.n_ops = n_ops;
    p.blank = blank;
    p.a_elem = a_elem; p.b_elem = b_elem; p.Amax = Amax; p.Bmax = Bmax; p.W = edit_words(Bmax);
    p.cs = cs; p.ca = ca; p.cb = cb; p.collapse = collapse ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (Bmax <= 64) edit_launch<1, 1>(st, B, p);
    else if (Bmax <= 128) edit_launch<2, 1>(st, B, p);
    else if (Bmax <= 256) edit_launch<4, 1>(st, B, p);
    else if (Bmax <= 512) edit_launch<8, 1>(st, B, p);
    else if (Bmax + 1 <= 1024) edit_launch<16, 1>(st, B, p);
    else edit_launch<16, 4>(st, B, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
