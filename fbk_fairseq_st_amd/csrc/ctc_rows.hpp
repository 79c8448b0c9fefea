// Row helpers shared by the CTC inference kernels (ctc_decode.hip, ctc_align.hip, ctc_segment.hip): one wave sweeps one row of logits.
#pragma once
#include "common.hpp"

// f(value, column) for every column of a row, lane `lane` of the wave taking the 16-byte vectors lane, lane + 64, ... and the
// scalar tail (V % (16 / sizeof(T)), or the whole row when it does not start 16-byte aligned)
template <typename T, typename F>
__device__ __forceinline__ void row_for_each(const T* __restrict__ x, int V, int lane, F f) {
    constexpr int E = 16 / (int)sizeof(T);
    const int nv = (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? V / E : 0;
    for (int c = lane; c < nv; c += 64) {
        T v[E];
        *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(x + c * E);
#pragma unroll
        for (int e = 0; e < E; ++e) f(to_f32(v[e]), c * E + e);
    }
    for (int j = nv * E + lane; j < V; j += 64) f(to_f32(x[j]), j);
}

// row_for_each with ONE assignment of columns to lanes whether or not the row starts 16-byte aligned (an unaligned row is read by
// scalar loads in the vector sweep's order): a sum taken with it does not depend on where the row lies, so a sentence's result does
// not depend on its place in a batch whose row stride is no multiple of 16 bytes.
template <typename T, typename F>
__device__ __forceinline__ void row_for_each_fixed(const T* __restrict__ x, int V, int lane, F f) {
    constexpr int E = 16 / (int)sizeof(T);
    const int nv = V / E;
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) { row_for_each<T>(x, V, lane, f); return; }
    for (int c = lane; c < nv; c += 64) {
#pragma unroll
        for (int e = 0; e < E; ++e) f(to_f32(x[c * E + e]), c * E + e);
    }
    for (int j = nv * E + lane; j < V; j += 64) f(to_f32(x[j]), j);
}

// (value, column) of the wave's best: the higher value, among equal values the lower column; column INT_MAX = none
__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o); const int oi = __shfl_xor(i, o);
        if (oi != 0x7fffffff && (i == 0x7fffffff || ov > v || (ov == v && oi < i))) { v = ov; i = oi; }
    }
}

// The row statistic of all three row phases: the maximum m, its first column mi, and lse1 = log1p of the sum of exp(x - m) over the
// OTHER columns, i.e. the log of the row's sum of exp(x - m) with column mi counted as exactly 1, so that lp = (x - m) - lse1 keeps
// its relative precision near 0.  FIXED: sweep with row_for_each_fixed (alignment, segmentation) instead of row_for_each (decoding).
struct RowStat { float m; int mi; float lse1; };
template <typename T, bool FIXED>
__device__ __forceinline__ RowStat row_max_lse(const T* __restrict__ x, int V, int lane) {
    auto sweep = [&](auto f) { if constexpr (FIXED) row_for_each_fixed<T>(x, V, lane, f); else row_for_each<T>(x, V, lane, f); };
    float m = -INFINITY; int mi = 0x7fffffff;
    sweep([&](float v, int j) { if (mi == 0x7fffffff || v > m || (v == m && j < mi)) { m = v; mi = j; } });
    wave_best(m, mi);
    float s = 0.f;
    sweep([&](float v, int j) { if (j != mi) s += expf(v - m); });
    return {m, mi, log1pf(wave_sum(s))};
}
