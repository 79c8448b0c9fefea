// Kaldi's LinearResample (torchaudio's resample_waveform) of padded batches of waveforms: include/s2t_hip.h, s2t_resample, states
// the rule.  One launch, no atomics, no host read.  A workgroup of four waves owns a tile of one row's outputs.
//   * The tile: RS_R * G consecutive units of the row's bank (a unit = in_unit inputs = out_unit outputs), G chosen by the entry
//     point per bank (resample_group) so that at most S2T_RESAMPLE_TILE_ITEMS (phase, unit) pairs and S2T_RESAMPLE_MAX_SPAN inputs
//     belong to it.  The grid has the tiles of the bank with the smallest tile; a workgroup past its row's last tile returns.
//   * Staging: the span of inputs the tile's outputs reach, [lo + U0 in_unit, + (RS_R G - 1) in_unit + extra), lands in LDS as
//     float once.  Inside [0, n) it is read with 16-byte (float32) or 8-byte (int16) loads of four samples per lane from the first
//     address that is so aligned, and written with one ds_write_b128 per lane: the LDS image is shifted by 0 .. 3 floats so that the
//     aligned body is 16-byte aligned there too.  The head in front of the body and the tail behind it go one sample per lane.
//     Positions outside [0, n) are written as zeros and never read from memory.
//   * The bank sits beside it tap-major, w[j][i] at j * out_unit + i: lanes on consecutive phases read consecutive addresses.
//     first[i] - lo is staged clamped to [0, extra - taps]: whatever the table holds, no read leaves the staged span.
//   * A thread takes a (phase i, unit group ug) pair and produces the RS_R outputs of phase i in the units ug, ug + G, ...: a weight
//     is read once for RS_R fused multiply-adds, (RS_R + 1) / RS_R LDS reads per FMA.  Lanes are consecutive in i, then in ug, so
//     an output store is unit-stride over the workgroup and with out_unit == 1 the input reads of a wave are in_unit apart (odd
//     in_unit: no bank conflict).  With out_unit == 1 the weights are the same in every lane: they are read through the
//     scalar cache from the table itself and LDS holds samples only.
//   * A sum starts at 0 and takes its taps in ascending j with fmaf: an output with one non-zero term is float(w) * x rounded once.
//   * What an output depends on: its own taps and samples.  Tile, batch, stride and alignment change no operation and no order.
// A bank with in_unit == out_unit copies (int16 becomes its float value).
#include "common.hpp"
#include "s2t_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_R = S2T_RESAMPLE_REUSE;

struct RsBank { int in_unit, out_unit, taps, first_off, w_off, lo, extra, G; };
struct RsArgs {
    const void* waves; const void* lengths; const int* ratio_id; const int* first; const float* weights;
    float* out; long long* out_len; int* status;
    long long row_stride;
    int Nmax, Mmax, tiles, n_banks, len_elem, bank_floats, phase_ints;
    RsBank bank[S2T_RESAMPLE_MAX_BANKS];
};

// the G of a bank: the unit groups of a tile.  0: the bank does not fit.
int resample_group(int in_unit, int out_unit, int extra) {
    if (in_unit == out_unit) return S2T_RESAMPLE_TILE_ITEMS;
    const long long by_items = S2T_RESAMPLE_TILE_ITEMS / out_unit;
    const long long by_span = extra > S2T_RESAMPLE_MAX_SPAN ? 0 : (((long long)S2T_RESAMPLE_MAX_SPAN - extra) / in_unit + 1) / RS_R;
    return (int)(by_items < by_span ? by_items : by_span);
}

template <typename TW> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<short> { typedef short4 type; };

template <typename TW>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const RsArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rs_dyn[];  // the bank, tap-major; first[] - lo; the span (shifted by sh)
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;

    const long long len = int_at(p.lengths, p.len_elem, b);
    const int rid = p.ratio_id ? p.ratio_id[b] : 0;
    bool refused = len < 0 || len > p.Nmax || rid < 0 || rid >= p.n_banks;
    RsBank d = p.bank[0];
#pragma unroll
    for (int r = 1; r < S2T_RESAMPLE_MAX_BANKS; ++r)
        if (!refused && r == rid) d = p.bank[r];
    long long m = refused ? 0 : (len * d.out_unit + d.in_unit - 1) / d.in_unit;
    if (m > p.Mmax) { refused = true; m = 0; }
    if (tile == 0 && tid == 0) {
        p.out_len[b] = m;
        p.status[b] = refused ? 2 : m == 0 ? 1 : 0;
    }
    const int tile_out = RS_R * d.G * d.out_unit;                   // <= RS_R * S2T_RESAMPLE_TILE_ITEMS
    float* outb = p.out + (size_t)b * p.Mmax;
    const TW* row = reinterpret_cast<const TW*>(p.waves) + (long long)b * p.row_stride;
    float* s_w = rs_dyn;
    int* s_first = reinterpret_cast<int*>(rs_dyn + p.bank_floats);
    float* s_x = rs_dyn + p.bank_floats + p.phase_ints;             // both counts are multiples of 4: 16-byte aligned
    const int OU = d.out_unit, IU = d.in_unit, taps = d.taps;
    const bool one_phase = OU == 1;

    const long long k0 = (long long)tile * tile_out;
    const long long k1 = min(k0 + tile_out, (long long)p.Mmax);
    for (long long k = max(m, k0) + tid; k < k1; k += RS_THREADS) outb[k] = 0.f;   // the padding behind the row's length
    if (k0 >= m) return;                                            // the same in every thread
    if (d.in_unit == d.out_unit) {
        const long long ke = min(k1, m);
        for (long long k = k0 + tid; k < ke; k += RS_THREADS) outb[k] = (float)row[k];
        return;
    }

    // ---- the bank
    if (!one_phase)
        for (int i = tid; i < taps * OU; i += RS_THREADS) s_w[i] = p.weights[d.w_off + i];
    for (int i = tid; i < OU; i += RS_THREADS) s_first[i] = min(max(p.first[d.first_off + i] - d.lo, 0), d.extra - taps);

    // ---- the span: element e is the sample g_lo + e of the row and lives at s_x[sh + e]
    const int span = (RS_R * d.G - 1) * IU + d.extra;               // <= S2T_RESAMPLE_MAX_SPAN
    const long long g_lo = (long long)d.lo + (long long)tile * (RS_R * d.G) * IU;
    const long long s0 = min(max(g_lo, 0LL), len), s1 = max(min(g_lo + span, len), s0);   // the part inside [0, n)
    const int e0 = (int)(s0 - g_lo), cnt = (int)(s1 - s0);          // e0 in [0, span] or the span lies outside: cnt = 0
    constexpr int VB = 4 * (int)sizeof(TW);                         // bytes of a four-sample load
    const unsigned long long addr = reinterpret_cast<unsigned long long>(row + s0);
    const int head = min((int)(((VB - (addr & (VB - 1))) & (VB - 1)) / sizeof(TW)), cnt);
    const int nvec = (cnt - head) / 4;
    const int sh = cnt > 0 ? (4 - ((e0 + head) & 3)) & 3 : 0;
    if (cnt < span) {                                               // the row's edges: zeros in front of 0 and behind n
        const int z0 = cnt > 0 ? e0 : span, z1 = cnt > 0 ? e0 + cnt : span;
        for (int e = tid; e < z0; e += RS_THREADS) s_x[sh + e] = 0.f;
        for (int e = z1 + tid; e < span; e += RS_THREADS) s_x[sh + e] = 0.f;
    }
    if (cnt > 0) {
        const TW* src = row + s0;
        float* dst = s_x + sh + e0;
        if (tid < head) dst[tid] = (float)src[tid];
        typedef typename Vec4<TW>::type V;
        const V* vsrc = reinterpret_cast<const V*>(src + head);
        float4* vdst = reinterpret_cast<float4*>(dst + head);
        for (int v = tid; v < nvec; v += RS_THREADS) {
            const V q = vsrc[v];
            vdst[v] = make_float4((float)q.x, (float)q.y, (float)q.z, (float)q.w);
        }
        const int t0 = head + 4 * nvec;
        if (tid < cnt - t0) dst[t0 + tid] = (float)src[t0 + tid];   // fewer than four
    }
    __syncthreads();

    // ---- a (phase, unit group) pair per thread: RS_R outputs that share their weights
    const int items = d.G * OU, step = d.G * IU;
    const float* wg = p.weights + d.w_off;
    for (int t = tid; t < items; t += RS_THREADS) {
        const int i = one_phase ? 0 : t % OU, ug = one_phase ? t : t / OU;
        const float* xp = s_x + sh + s_first[i] + ug * IU;
        float acc[RS_R];
#pragma unroll
        for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
        if (one_phase) {
#pragma unroll 4
            for (int j = 0; j < taps; ++j) {
                const float w = wg[j];                              // the same address in every lane
#pragma unroll
                for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(w, xp[r * step + j], acc[r]);
            }
        } else {
            const float* wp = s_w + i;
#pragma unroll 4
            for (int j = 0; j < taps; ++j) {
                const float w = wp[j * OU];
#pragma unroll
                for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(w, xp[r * step + j], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RS_R; ++r) {
            const long long k = k0 + (long long)r * items + t;      // unit r G + ug, phase i
            if (k < m) outb[k] = acc[r];
        }
    }
}

}  // namespace

extern "C" int s2t_resample(const void* waves, int wave_elem, long long row_stride, const void* lengths, int len_elem, const int* ratio_id,
                            int B, int Nmax, int Mmax, const int* banks, int n_banks, const int* first, int n_first,
                            const float* weights, int n_weights, float* out, long long* out_len, int* status, void* stream) {
    if (B <= 0) return S2T_OK;
    if (!waves || !lengths || !banks || !first || !weights || !out || !out_len || !status) return S2T_EINVAL;
    if (wave_elem != 2 && wave_elem != 4) return S2T_EINVAL;
    if (len_elem != 4 && len_elem != 8) return S2T_EINVAL;
    if (Nmax < 0 || Mmax < 0 || row_stride < 0 || n_first < 0 || n_weights < 0) return S2T_EINVAL;
    if (n_banks < 1) return S2T_EINVAL;
    if (n_banks > S2T_RESAMPLE_MAX_BANKS) return S2T_ENOTSUP;
    RsArgs p;
    int rc = S2T_OK, bank_floats = 0, phases = 0, span = 0, min_tile = RS_R * S2T_RESAMPLE_TILE_ITEMS;
    for (int r = 0; r < n_banks; ++r) {
        const int* h = banks + S2T_RESAMPLE_BANK_INTS * r;
        RsBank& d = p.bank[r];
        d.in_unit = h[0]; d.out_unit = h[1]; d.taps = h[2]; d.first_off = h[3]; d.w_off = h[4]; d.lo = h[5]; d.extra = h[6];
        if (d.in_unit < 1 || d.out_unit < 1) return S2T_EINVAL;
        if (d.in_unit == d.out_unit) {                              // a copy: nothing else of the bank is looked at
            d.in_unit = d.out_unit = 1;
            d.taps = d.first_off = d.w_off = d.lo = d.extra = 0;
            d.G = resample_group(1, 1, 0);
            continue;
        }
        if (d.taps < 1 || d.extra < d.taps || d.first_off < 0 || d.w_off < 0) return S2T_EINVAL;
        if ((long long)d.first_off + d.out_unit > n_first || (long long)d.w_off + (long long)d.taps * d.out_unit > n_weights) return S2T_EINVAL;
        if (d.lo < -0x3fffffff || d.lo > 0x3fffffff) return S2T_EINVAL;
        if (d.out_unit > S2T_RESAMPLE_MAX_PHASES || (long long)d.taps * d.out_unit > S2T_RESAMPLE_MAX_BANK) { rc = S2T_ENOTSUP; continue; }
        d.G = resample_group(d.in_unit, d.out_unit, d.extra);
        if (d.G < 1) { rc = S2T_ENOTSUP; continue; }
        const int tile_out = RS_R * d.G * d.out_unit;
        min_tile = tile_out < min_tile ? tile_out : min_tile;
        if (d.out_unit > 1 && d.taps * d.out_unit > bank_floats) bank_floats = d.taps * d.out_unit;
        phases = d.out_unit > phases ? d.out_unit : phases;
        const int s = (RS_R * d.G - 1) * d.in_unit + d.extra;
        span = s > span ? s : span;
    }
    if (rc != S2T_OK) return rc;
    for (int r = n_banks; r < S2T_RESAMPLE_MAX_BANKS; ++r) p.bank[r] = p.bank[0];
    const long long tiles = Mmax > 0 ? ((long long)Mmax + min_tile - 1) / min_tile : 1;   // a row without outputs still gets its status
    if ((long long)B * tiles > 0x7fffffffLL) return S2T_ENOTSUP;
    p.waves = waves; p.lengths = lengths; p.ratio_id = ratio_id; p.first = first; p.weights = weights;
    p.out = out; p.out_len = out_len; p.status = status; p.row_stride = row_stride;
    p.Nmax = Nmax; p.Mmax = Mmax; p.tiles = (int)tiles; p.n_banks = n_banks; p.len_elem = len_elem;
    p.bank_floats = (bank_floats + 3) & ~3; p.phase_ints = (phases + 3) & ~3;
    const size_t dyn = sizeof(float) * ((size_t)p.bank_floats + p.phase_ints + span + 4);   // at most 64 KiB: no attribute is needed
    hipStream_t st = (hipStream_t)stream;
    if (wave_elem == 2) hipLaunchKernelGGL((resample_kernel<short>), dim3((unsigned)(B * tiles)), dim3(RS_THREADS), dyn, st, p);
    else hipLaunchKernelGGL((resample_kernel<float>), dim3((unsigned)(B * tiles)), dim3(RS_THREADS), dyn, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
