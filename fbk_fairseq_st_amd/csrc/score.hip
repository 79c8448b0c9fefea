// Teacher-forced scoring: the log-probability of the target token of every row of a [L*B, V] logit buffer, for one model or the
// log of the mean probability of up to 8 (include/s2t_hip.h: s2t_score_targets).
// Reference: fairseq/sequence_scorer.py:42-92 (get_normalized_probs + gather_target_probs per member, probabilities summed and
// divided by the number of models, log at the end); here the members are combined in log space as ensemble_lse_kernel of
// loss_embed.hip combines them.
//
// Every logit is read once: a row is walked in 16-byte vectors (scalars when a member's rows are not 16-byte aligned) with a
// running (max, sum of exp) pair, and the target's logit is picked out of the vector that holds it as it passes.  Nothing of size
// [rows, V] is written: the output is one float per row.
//
// A row is always split over 256 "slots": slot q takes the vectors q, q + 256, q + 512, ... in ascending order, then (slot nv % 256
// only) the V % VEC tail elements one by one.  The slots' pairs are merged by a 64-lane xor butterfly inside each group of 64 slots
// and the four groups' results in order 0, 1, 2, 3.  Two launch forms evaluate exactly that:
//   * workgroup per row (few rows: 256 threads share a row, slot = thread, group = wave, the four results meet in LDS);
//   * wave per row (many rows: four rows per workgroup, lane l holds the slots l, l + 64, l + 128, l + 192 in four independent
//     accumulators -- four loads in flight per lane -- and the butterfly runs once per accumulator; no LDS, no barrier).
// The file is compiled without contraction of products into fused multiply-adds (the pragma below), so the merge is commutative bit
// for bit and both forms, and any grid, give the same bits for the same row.  No atomics.
#include "common.hpp"

// no product is fused into a following addition anywhere below: where the compiler would fuse depends on the code around it, and the
// two launch forms must round alike
#pragma clang fp contract(off)

namespace {

struct ScoreMembers { const void* p[8]; int ld[8]; };

template <typename T, int VEC> struct RowVec;
template <> struct RowVec<float, 4> { typedef f32x4 type; };
template <> struct RowVec<bf16, 8> { typedef bf16x8 type; };
template <> struct RowVec<float, 1> { typedef float type; };
template <> struct RowVec<bf16, 1> { typedef bf16 type; };

template <int VEC, typename V> __device__ __forceinline__ float vec_elem(const V& v, int i) {
    if constexpr (VEC == 1) return to_f32(v); else return to_f32(v[i]);
}

// (m, s) <- (m, s) with the VEC values of one vector added: s = sum exp(x - m) over everything seen, m their maximum
// (m = -inf while every value was -inf: the sum is then taken against 0 and stays 0)
// The per-logit exponential goes through the hardware exp2 as in lsce_kernel of loss_embed.hip: exp2(fma(x, log2 e, -fl(m log2 e))),
// two instructions per logit where expf takes a dozen (a bf16 row holds eight logits per 16 bytes: expf made the kernel
// instruction-bound); the rescales and merges, one per vector at most, keep expf.
template <int VEC> __device__ __forceinline__ void pair_add(const float (&x)[VEC], float& m, float& s) {
    constexpr float L2E = 1.44269504088896f;
    float vm = x[0];
#pragma unroll
    for (int i = 1; i < VEC; ++i) vm = fmaxf(vm, x[i]);
    const float nm = fmaxf(m, vm);
    s *= (nm == m) ? 1.f : expf(m - nm);
    m = nm;
    const float ml2 = ((m == -INFINITY) ? 0.f : m) * L2E;
#pragma unroll
    for (int i = 0; i < VEC; ++i) s += __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], L2E, -ml2));
}
// merge of two pairs; commutative bit for bit (two products and one addition, each rounded: contraction is off in this file)
__device__ __forceinline__ void pair_merge(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    const float mm = (nm == -INFINITY) ? 0.f : nm;
    const float a = s * expf(m - mm), b = s2 * expf(m2 - mm);
    s = a + b;
    m = nm;
}
__device__ __forceinline__ void pair_butterfly(float& m, float& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        pair_merge(m, s, m2, s2);
    }
}

// one vector of a slot: load -> f32 values, the target's logit if this vector holds column c
template <typename T, int VEC> __device__ __forceinline__ void slot_vector(const T* __restrict__ x, int idx, int c, float& m, float& s, float& xc) {
    typedef typename RowVec<T, VEC>::type V;
    const V v = *reinterpret_cast<const V*>(x + (long)idx * VEC);
    float f[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) f[i] = vec_elem<VEC>(v, i);
    const unsigned d = (unsigned)(c - idx * VEC);
    if (d < (unsigned)VEC) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) if (d == (unsigned)i) xc = f[i];
    }
    pair_add<VEC>(f, m, s);
}
// the V % VEC elements behind the last whole vector (the slot that would hold vector nv), one at a time
template <typename T, int VEC> __device__ __forceinline__ void slot_tail(const T* __restrict__ x, int nv, int V, int c, float& m, float& s, float& xc) {
    for (int v = nv * VEC; v < V; ++v) {
        const float f[1] = {to_f32(x[v])};
        if (v == c) xc = f[0];
        pair_add<1>(f, m, s);
    }
}

// log of the members' mean probability from their log-probabilities (ensemble_lse_kernel of loss_embed.hip: members in order)
__device__ __forceinline__ float combine_members(const float (&lp)[8], int n, float log_n) {
    if (n == 1) return lp[0];
    float M = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < n) M = fmaxf(M, lp[j]);
    if (!(M > -INFINITY)) return M;               // every member -inf: -inf; a NaN member (target out of range): NaN
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < n) s += expf(lp[j] - M);
    return M + logf(s) - log_n;
}
__device__ __forceinline__ void set_member(float (&lp)[8], int j, float v) {
#pragma unroll
    for (int k = 0; k < 8; ++k) if (k == j) lp[k] = v;         // static indices: the array stays in registers
}

// slot (0..255) that meets column c on its way: the vector's slot, or the tail's
template <int VEC> __device__ __forceinline__ int owner_slot(int c, int nv) {
    const int vi = c / VEC;
    return (vi < nv ? vi : nv) & 255;
}

// ---- workgroup per row
template <typename T, int VEC>
__global__ __launch_bounds__(256) void score_row_block_kernel(ScoreMembers mem, int n, const long long* __restrict__ target,
                                                              float* __restrict__ out, int B, int L, int V, float log_n) {
    __shared__ float sh[8];
    const int r = blockIdx.x, t = r / B, b = r - t * B;
    const long long c64 = target[(long)b * L + t];
    const bool valid = c64 >= 0 && c64 < V;
    const int c = valid ? (int)c64 : -1;
    const int nv = V / VEC, q = threadIdx.x, w = q >> 6;
    const int owner = valid ? owner_slot<VEC>(c, nv) : 0;
    float lp[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) lp[k] = -INFINITY;
    for (int j = 0; j < n; ++j) {
        const T* x = (const T*)mem.p[j] + (long)r * mem.ld[j];
        float m = -INFINITY, s = 0.f, xc = NAN;
#pragma unroll 4
        for (int idx = q; idx < nv; idx += 256) slot_vector<T, VEC>(x, idx, c, m, s, xc);
        if (VEC > 1 && q == (nv & 255)) slot_tail<T, VEC>(x, nv, V, c, m, s, xc);
        pair_butterfly(m, s);
        __syncthreads();                                       // the previous member's results have been read
        if ((q & 63) == 0) { sh[2 * w] = m; sh[2 * w + 1] = s; }
        __syncthreads();
        if (q == owner) {
            float M = sh[0], S = sh[1];
            pair_merge(M, S, sh[2], sh[3]);
            pair_merge(M, S, sh[4], sh[5]);
            pair_merge(M, S, sh[6], sh[7]);
            set_member(lp, j, xc - (M + logf(S)));
        }
    }
    if (q == owner) out[(long)b * L + t] = valid ? combine_members(lp, n, log_n) : NAN;
}

// ---- wave per row, four rows per workgroup
template <typename T, int VEC>
__global__ __launch_bounds__(256) void score_row_wave_kernel(ScoreMembers mem, int n, const long long* __restrict__ target,
                                                             float* __restrict__ out, int B, int L, int V, float log_n) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (long)B * L) return;                              // whole waves leave: nothing below synchronises the workgroup
    const int lane = threadIdx.x & 63;
    const int t = (int)(r / B), b = (int)(r - (long)t * B);
    const long long c64 = target[(long)b * L + t];
    const bool valid = c64 >= 0 && c64 < V;
    const int c = valid ? (int)c64 : -1;
    const int nv = V / VEC;
    const int owner = valid ? owner_slot<VEC>(c, nv) : 0;
    float lp[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) lp[k] = -INFINITY;
    for (int j = 0; j < n; ++j) {
        const T* x = (const T*)mem.p[j] + r * mem.ld[j];
        float m[4], s[4], xc = NAN;
#pragma unroll
        for (int a = 0; a < 4; ++a) { m[a] = -INFINITY; s[a] = 0.f; }
        for (int base = 0; base < nv; base += 256) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int idx = base + 64 * a + lane;
                if (idx < nv) slot_vector<T, VEC>(x, idx, c, m[a], s[a], xc);
            }
        }
        if (VEC > 1) {
            const int ts = nv & 255;                           // the tail's slot: lane ts & 63, accumulator ts >> 6
            if (lane == (ts & 63)) {
#pragma unroll
                for (int a = 0; a < 4; ++a) if (a == (ts >> 6)) slot_tail<T, VEC>(x, nv, V, c, m[a], s[a], xc);
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) pair_butterfly(m[a], s[a]);
        float M = m[0], S = s[0];
        pair_merge(M, S, m[1], s[1]);
        pair_merge(M, S, m[2], s[2]);
        pair_merge(M, S, m[3], s[3]);
        set_member(lp, j, xc - (M + logf(S)));
    }
    if (lane == (owner & 63)) out[(long)b * L + t] = valid ? combine_members(lp, n, log_n) : NAN;
}

// rows from which a wave per row fills the chip (1,024 workgroups of four rows: four per CU); below, a workgroup per row
constexpr long SCORE_WAVE_MIN_ROWS = 4096;

template <typename T, int VEC>
void score_launch(const ScoreMembers& mem, int n, const long long* target, float* out, int B, int L, int V, hipStream_t st) {
    const long rows = (long)B * L;
    const float log_n = logf((float)n);
    if (rows >= SCORE_WAVE_MIN_ROWS)
        hipLaunchKernelGGL((score_row_wave_kernel<T, VEC>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, mem, n, target, out, B, L, V, log_n);
    else
        hipLaunchKernelGGL((score_row_block_kernel<T, VEC>), dim3((unsigned)rows), dim3(256), 0, st, mem, n, target, out, B, L, V, log_n);
}

}  // namespace

extern "C" int s2t_score_targets(int dtype, int n, const void* const* logits, const int* ld, const long long* target, float* out,
                                 int B, int L, int V, void* stream) {
    if (B < 0 || L < 0) return S2T_EINVAL;
    if ((long)B * L == 0) return S2T_OK;
    if (n < 1 || n > 8 || !logits || !ld || !target || !out || V < 1) return S2T_EINVAL;
    if ((long)B * L > 0x7fffffffL) return S2T_EINVAL;          // one workgroup per row: the grid's x dimension
    if (dtype != S2T_BF16 && dtype != S2T_F32) return S2T_ENOTSUP;
    const size_t esz = dtype == S2T_BF16 ? 2 : 4;
    ScoreMembers mem;
    bool vec = true;                                           // 16-byte loads when every row of every member is 16-byte aligned
    for (int j = 0; j < 8; ++j) {
        mem.p[j] = nullptr; mem.ld[j] = 0;
        if (j >= n) continue;
        if (!logits[j] || ld[j] < V) return S2T_EINVAL;
        mem.p[j] = logits[j]; mem.ld[j] = ld[j];
        vec = vec && ((uintptr_t)logits[j] % 16 == 0) && (((size_t)ld[j] * esz) % 16 == 0);
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == S2T_BF16) { if (vec) score_launch<bf16, 8>(mem, n, target, out, B, L, V, st); else score_launch<bf16, 1>(mem, n, target, out, B, L, V, st); }
    else                   { if (vec) score_launch<float, 4>(mem, n, target, out, B, L, V, st); else score_launch<float, 1>(mem, n, target, out, B, L, V, st); }
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
