// Sampling search (fairseq/search.py:164-278: unrestricted, top-k and nucleus sampling) as a stateless function of
// (key, step, slot, column), shared by the stand-alone kernel (sample.hip: s2t_sample_rows) and the SAMPLE form of dec_row_kernel
// (decode.hip).  tests/decode_sampling_ref.py and fbk_fairseq_st_amd/sampling.py restate it.
//
// The draw.  torch.multinomial's stream cannot be reproduced, so the draw is defined here: every kept column v with a finite
// log-probability lp gets the key lp + g, g = -logf(-logf(u)) a standard Gumbel variate from the uniform u of hash32(key, step, slot, v),
// and the token is the arg-max of the keys (value descending, column ascending on ties): P(token = v) = p_v / sum of the kept p, with
// no sort, no scan and no dependence on a summation order.  u = ((h >> 9) + 0.5) * 2^-23 = (2k + 1) * 2^-24 is exact in f32 and never
// 0 or 1.  The hash is 32-bit integer arithmetic only (mix32 rounds): two words of row state from (key, step, slot), then two rounds
// per column.
//
// The kept set.  lp is the row after all score rules, not renormalised.  The order is value descending, column ascending.
//   top-p (P > 0; takes precedence, search.py:227-232): a column is kept iff the mass p = expf(lp) strictly before it is < P
//                (search.py:190-216: the `lt` mask plus one more column, clamped);  P >= the total mass keeps every finite column;
//   top-k (k > 0): the first k columns; k >= the number of finite columns keeps them all;
//   neither:       every finite column.
// A kept set is a prefix of that order, so it is (thr, cmax): lp > thr, or lp == thr and column <= cmax.  thr comes from a bisection
// on the order-preserving integer image of f32 (32 rounds, each a block-wide count or a block-wide sum of the p above the candidate),
// the number of columns kept AT thr from the rule itself, and cmax from a bisection on the column (only when the ties at thr are cut).
// Every block-wide sum adds the threads' partial sums in a fixed order: the result does not depend on scheduling; no atomics.
#pragma once
#include "common.hpp"

namespace smp {
// ---- hash, uniform, key
struct RowKey { uint32_t a, b; };
__device__ __forceinline__ RowKey row_key(unsigned long long key, int step, int slot) {
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    uint32_t a = mix32(lo ^ 0x9E3779B9u); a = mix32(a + hi); a = mix32(a + (uint32_t)step); a = mix32(a + (uint32_t)slot);
    uint32_t b = mix32(hi ^ 0x85EBCA6Bu); b = mix32(b + lo); b = mix32(b + (uint32_t)slot); b = mix32(b + (uint32_t)step);
    return RowKey{a, b};
}
__device__ __forceinline__ uint32_t hash32(RowKey k, int col) { return mix32(mix32((uint32_t)col ^ k.a) + k.b); }
__device__ __forceinline__ float uniform(uint32_t h) { return ((float)(h >> 9) + 0.5f) * 0x1p-23f; }
__device__ __forceinline__ float gumbel_key(float lp, float u) { return lp + -logf(-logf(u)); }

// order-preserving image of f32 (no NaN): x < y  <=>  ord(x) < ord(y)
__device__ __forceinline__ uint32_t ord(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unord(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
constexpr uint32_t ORD_NEG_INF = 0x007FFFFFu;

// ---- block-wide reductions: DPP inside the wave (every lane active), the waves' results through LDS, added by every thread in wave
// order.  Two buffers used in turn: one barrier per reduction (a buffer is rewritten two reductions later, behind the barrier between).
// (`turn`, the buffer of the next reduction, is a register of the caller that starts at 0 and is the same in every thread.)
struct Scratch { float f[2][48]; int i[2][16]; };
template <int CTRL> __device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int CTRL> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ float rl_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ float wave_sum64(float v) {
    v += dpp_f<0xB1>(v); v += dpp_f<0x4E>(v); v += dpp_f<0x141>(v); v += dpp_f<0x140>(v);
    return (rl_f(v, 0) + rl_f(v, 16)) + (rl_f(v, 32) + rl_f(v, 48));
}
__device__ __forceinline__ float wave_max64(float v) {
    v = fmaxf(v, dpp_f<0xB1>(v)); v = fmaxf(v, dpp_f<0x4E>(v)); v = fmaxf(v, dpp_f<0x141>(v)); v = fmaxf(v, dpp_f<0x140>(v));
    return fmaxf(fmaxf(rl_f(v, 0), rl_f(v, 16)), fmaxf(rl_f(v, 32), rl_f(v, 48)));
}
__device__ __forceinline__ int wave_min64(int v) {
    v = min(v, dpp_i<0xB1>(v)); v = min(v, dpp_i<0x4E>(v)); v = min(v, dpp_i<0x141>(v)); v = min(v, dpp_i<0x140>(v));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
// NV sums at once (counts are sums of 0.f / 1.f: exact up to 2^24)
template <int NT, int NV>
__device__ __forceinline__ void block_sums(float (&v)[NV], Scratch& sc, int& turn) {
    constexpr int NW = NT / 64;
    const int w = threadIdx.x >> 6;
    float* s = sc.f[turn];
    turn ^= 1;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const float r = wave_sum64(v[q]);
        if ((threadIdx.x & 63) == 0) s[q * 16 + w] = r;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        float r = 0.f;
#pragma unroll
        for (int i = 0; i < NW; ++i) r += s[q * 16 + i];
        v[q] = r;
    }
}
template <int NT> __device__ __forceinline__ float block_sum1(float v, Scratch& sc, int& turn) {
    float a[1] = {v};
    block_sums<NT, 1>(a, sc, turn);
    return a[0];
}

// ---- the kept set of a row held as VPT values per thread: lp[i] is column threadIdx.x + i * NT, -inf for a column >= V; no NaN, no -0
struct Kept { float thr; int cmax; int n; };
__device__ __forceinline__ bool is_kept(const Kept& k, float lp, int col) {
    return lp > -INFINITY && (lp > k.thr || (lp == k.thr && col <= k.cmax));
}
template <int VPT, int NT>
__device__ __forceinline__ Kept kept_set(const float (&lp)[VPT], int V, int topk, float topp, Scratch& sc, int& turn) {
    constexpr bool CACHE_P = VPT <= 32;                            // the probabilities beside the row while both fit in registers
    const int tid = threadIdx.x;
    float c = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) c += lp[i] > -INFINITY ? 1.f : 0.f;
    const int nfin = (int)block_sum1<NT>(c, sc, turn);
    Kept all{-INFINITY, 0x7fffffff, nfin};
    const bool nucleus = topp > 0.f;
    if (!nucleus && (topk <= 0 || topk >= nfin)) return all;
    uint32_t o[VPT];
    [[maybe_unused]] float p[CACHE_P ? VPT : 1];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        o[i] = ord(lp[i]);
        if constexpr (CACHE_P) p[i] = expf(lp[i]);
    }
    auto prob = [&](int i) { if constexpr (CACHE_P) return p[i]; else return expf(lp[i]); };
    uint32_t T;
    if (nucleus) {
        // the smallest T with sum(p : ord > T) < P; true at the top of the range (nothing lies above it)
        uint32_t lo = 0u, hi = 0xFFFFFFFFu;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < VPT; ++i) s += o[i] > mid ? prob(i) : 0.f;
            if (block_sum1<NT>(s, sc, turn) < topp) hi = mid; else lo = mid + 1u;
        }
        T = lo;
        if (T <= ORD_NEG_INF) return all;                          // P >= the total mass
    } else {
        // the largest T with count(ord >= T) >= k: the k-th largest value (finite: k < nfin)
        uint32_t lo = 0u, hi = 0xFFFFFFFFu;
        while (lo < hi) {
            const uint32_t d = hi - lo, mid = lo + (d >> 1) + (d & 1u);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < VPT; ++i) s += o[i] >= mid ? 1.f : 0.f;
            if (block_sum1<NT>(s, sc, turn) >= (float)topk) lo = mid; else hi = mid - 1u;
        }
        T = lo;
    }
    float r[3] = {0.f, 0.f, 0.f};                                  // mass above thr, columns above thr, columns at thr
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        r[0] += o[i] > T ? prob(i) : 0.f;
        r[1] += o[i] > T ? 1.f : 0.f;
        r[2] += o[i] == T ? 1.f : 0.f;
    }
    block_sums<NT, 3>(r, sc, turn);
    const int n_gt = (int)r[1], n_eq = (int)r[2];
    Kept k;
    k.thr = unord(T);
    int m;                                                         // columns kept at thr, in column order (>= 1)
    if (nucleus) {
        // tie i (0-based) has the mass r[0] + i * p(thr) before it: the product and the sum each rounded to f32
        const float pt = expf(k.thr);
        int lo = 1, hi = n_eq;                                     // tie 0 is kept (the bisection above); m = the first i that is not
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            float before = __fmul_rn((float)mid, pt);
            asm volatile("" : "+v"(before));                       // a value of its own: no fused multiply-add
            if (__fadd_rn(r[0], before) < topp) lo = mid + 1; else hi = mid;
        }
        m = lo;
    } else {
        m = topk - n_gt;
    }
    k.n = n_gt + m;
    k.cmax = 0x7fffffff;
    if (m < n_eq) {
        // the m-th column at thr: the smallest c with count(ord == T, column <= c) >= m
        int lo = 0, hi = V - 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < VPT; ++i) s += (o[i] == T && tid + i * NT <= mid) ? 1.f : 0.f;
            if (block_sum1<NT>(s, sc, turn) >= (float)m) hi = mid; else lo = mid + 1;
        }
        k.cmax = lo;
    }
    return k;
}

// ---- one draw from the kept set.  Every thread gets the token (0 when nothing is kept); `mine` is true in the one thread that holds
// the token's column, with its log-probability in lp_tok (nothing kept: thread 0, -inf).
template <int VPT, int NT>
__device__ __forceinline__ int draw(const float (&lp)[VPT], const Kept& k, RowKey rk, Scratch& sc, int& turn, bool& mine, float& lp_tok) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, w = tid >> 6;
    float bv = -INFINITY, bl = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = tid + i * NT;
        if (is_kept(k, lp[i], v)) {
            const float g = gumbel_key(lp[i], uniform(hash32(rk, v)));
            if (bi == 0x7fffffff || g > bv) { bv = g; bi = v; bl = lp[i]; }      // columns ascend: a tie keeps the smaller one
        }
    }
    const float mv = wave_max64(bv);
    const int mi = wave_min64(bv == mv ? bi : 0x7fffffff);
    float* sf = sc.f[turn];
    int* si = sc.i[turn];
    turn ^= 1;
    if ((tid & 63) == 0) { sf[w] = mv; si[w] = mi; }
    __syncthreads();
    float tv = sf[0];
    int ti = si[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
        const float ov = sf[i];
        const int oi = si[i];
        if (oi != 0x7fffffff && (ti == 0x7fffffff || ov > tv || (ov == tv && oi < ti))) { tv = ov; ti = oi; }
    }
    if (ti == 0x7fffffff) { mine = tid == 0; lp_tok = -INFINITY; return 0; }
    mine = bi == ti;
    lp_tok = bl;
    return ti;
}
}  // namespace smp
