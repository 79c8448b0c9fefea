// Kaldi log-mel filterbanks of waveforms and per-utterance mean / variance normalisation (include/s2t_hip.h: s2t_fbank and s2t_cmvn
// state the rules).
// s2t_fbank: one launch, no atomics, no host read.  A workgroup of four waves owns a tile of S2T_FBANK_TILE_ELEMS / N consecutive
// frames of one utterance.
//   * Staging: the tile's samples are read once (one element per lane: no alignment beyond the element's is assumed), converted to
//     float and kept in LDS; consecutive frames share W - S of them there.  With S > W nothing is shared and only each frame's own W
//     samples are staged.  A position at or behind the utterance's length is staged as 0 and never read from memory.  The window,
//     the twiddles and the sparse mel bank are staged beside them.
//   * A wave takes one frame at a time: mean (a fixed lane-strided sum and an xor tree), pre-emphasis and window while packing the
//     real frame as N/2 complex points z[n] = y[2n] + i y[2n+1]; a radix-2 Stockham FFT of those N/2 points between two LDS
//     buffers; the even / odd split X[k] = E[k] + w^k O[k] to the powers of the bins 0 .. N/2 - 1; a lane per mel bin sums its own
//     contiguous range of powers; log, store.
//   * Precision: everything between the staged float samples and the mel energy runs in float64, with float64 twiddles.  The
//     lowest mel bins hold one FFT bin that DC removal and pre-emphasis attenuate by about 30 dB, so in a frame where that bin is
//     small the rounding of a float32 transform of the whole frame shows: a float32 radix-2 restatement of this kernel reached
//     7.7 times the error of a float32 host library on one of the test's cases, against 8 allowed (tests/fbank_ref.py).  The
//     transform is a few per cent of an MI355X's float64 rate at any batch; what it costs is LDS, twice the bytes per point.
//   * LDS banking: real and imaginary parts are separate double arrays.  Butterfly i of every stage reads x[i] and x[i + N/4]
//     (consecutive lanes, consecutive 8-byte slots: a 32-lane group covers the 64 banks once) and writes y[q + 2sp] and
//     y[q + 2sp + s] (runs of s doubles with gaps of s: at most two addresses per bank in a 16-lane group of an 8-byte store, which
//     the store's own issue time covers); the split reads Z[k] and Z[N/2 - k], both unit stride.  Nothing is padded or swizzled
//     because no exchange has a power-of-two stride between lanes.
//   * What a frame's numbers depend on: its own W samples in LDS and the tables.  Which wave or tile it falls in changes no
//     operation and no order.
// s2t_cmvn: one launch, one workgroup of 1,024 threads per utterance; a thread owns one column of every G-th row.  Mean over the
// differences from the first frame, variance over the differences from that mean (a constant column gets exactly its value and
// exactly 0), then the scaling and the padding's zeros.
#include "common.hpp"
#include "s2t_hip.h"

namespace {

constexpr int FB_WAVES = 4;
constexpr int FB_THREADS = 64 * FB_WAVES;

struct FbankArgs {
    const void* waves; const long long* lengths;
    const float* window; const double* twiddle; const int* bank; const float* weights;
    float* out; int* out_len; int* status;
    long long row_stride;
    int Nmax, W, S, F, Tmax, tiles, n_weights, remove_dc;
    double preemph;
};

template <int N> constexpr size_t fbank_fft_lds() { return sizeof(double) * FB_WAVES * 4 * (N / 2); }   // dynamic LDS in front of the tile
template <int N> constexpr size_t fbank_static_lds() { return sizeof(double) * N + sizeof(float) * 2 * N + sizeof(int) * 3 * S2T_FBANK_MAX_BINS; }

template <int N, typename TW>
__global__ __launch_bounds__(FB_THREADS) void fbank_kernel(const FbankArgs p) {
    constexpr int M = N / 2;                                        // complex points of the half-size transform
    constexpr int FT = S2T_FBANK_TILE_ELEMS / N;                    // frames of a tile
    extern __shared__ __attribute__((aligned(16))) double fb_dyn[]; // per wave re, im of the two Stockham buffers; then the tile
    __shared__ double s_tw[N];                                      // cos(2 pi k / N), then -sin(2 pi k / N), k < N/2
    __shared__ float s_win[N];
    __shared__ float s_wt[N];                                       // the bank's weights, bin after bin
    __shared__ int s_bank[S2T_FBANK_MAX_BINS][3];                   // first power, count, offset into s_wt
    float* fb_tile = reinterpret_cast<float*>(fb_dyn + FB_WAVES * 4 * M);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / p.tiles, t0 = (blockIdx.x % p.tiles) * FT;
    const int W = p.W, S = p.S, F = p.F;

    const long long len = p.lengths[b];
    const bool refused = len < 0 || len > p.Nmax;
    int m = refused || len < W ? 0 : (int)(1 + (len - W) / S);
    m = min(m, p.Tmax);                                             // the entry point checked Tmax against Nmax: never cuts
    if (blockIdx.x % p.tiles == 0 && tid == 0) {
        p.out_len[b] = m;
        p.status[b] = refused ? 2 : m == 0 ? 1 : 0;
    }
    float* outb = p.out + (size_t)b * p.Tmax * F;
    {   // the collater's padding: rows of this tile at or behind m
        const int z0 = max(m, t0), z1 = min(t0 + FT, p.Tmax);
        for (int i = tid; i < (z1 - z0) * F; i += FB_THREADS) outb[(size_t)z0 * F + i] = 0.f;
    }
    if (t0 >= m) return;                                            // the same in every thread

    // ---- stage the tables and the tile
    for (int i = tid; i < N; i += FB_THREADS) {
        s_tw[i] = p.twiddle[i];
        s_win[i] = i < W ? p.window[i] : 0.f;
        s_wt[i] = i < p.n_weights ? p.weights[i] : 0.f;
    }
    for (int j = tid; j < F; j += FB_THREADS) {                     // whatever the table holds, no read leaves the staged arrays
        const int first = min(max(p.bank[3 * j], 0), M), off = min(max(p.bank[3 * j + 2], 0), p.n_weights);
        const int cnt = min(min(max(p.bank[3 * j + 1], 0), M - first), p.n_weights - off);
        s_bank[j][0] = first; s_bank[j][1] = cnt; s_bank[j][2] = off;
    }
    const int Sl = min(S, W);                                       // distance of two frames in the tile
    const int span = (FT - 1) * Sl + W;
    const TW* row = reinterpret_cast<const TW*>(p.waves) + (long long)b * p.row_stride;
    for (int i = tid; i < span; i += FB_THREADS) {
        const long long g = S <= W ? (long long)t0 * S + i : (long long)(t0 + i / W) * S + i % W;
        fb_tile[i] = g < len ? (float)row[g] : 0.f;
    }

    double* re0 = fb_dyn + (wave * 4 + 0) * M; double* im0 = re0 + M; double* re1 = im0 + M; double* im1 = re1 + M;
    const double c = p.preemph, w_d = (double)W;
    for (int f = wave; f < FT; f += FB_WAVES) {                     // the same count in every wave: the barriers are the workgroup's
        __syncthreads();                                            // the tile is staged; the last frame's powers were read
        const float* x = fb_tile + f * Sl;
        double mean = 0.0;
        if (p.remove_dc) {
            double acc = 0.0;
            for (int i = lane; i < W; i += 64) acc += (double)x[i];
            mean = wave_sum_d(acc) / w_d;
        }
#pragma unroll
        for (int r = 0; r < M / 64; ++r) {
            const int n = lane + 64 * r, i0 = 2 * n, i1 = i0 + 1;
            double y0 = 0.0, y1 = 0.0;
            if (i0 < W) {
                const double a = (double)x[i0] - mean, pa = (double)x[max(i0 - 1, 0)] - mean;
                y0 = (a - c * pa) * (double)s_win[i0];
                if (i1 < W) y1 = (((double)x[i1] - mean) - c * a) * (double)s_win[i1];
            }
            re0[n] = y0; im0[n] = y1;
        }
        double *xr = re0, *xi = im0, *yr = re1, *yi = im1;
#pragma unroll 1
        for (int s = 1; s < M; s <<= 1) {
            __syncthreads();
#pragma unroll
            for (int r = 0; r < M / 128; ++r) {
                const int i = lane + 64 * r;
                const int q = i & (s - 1), k = i - q, o = 2 * k + q;    // twiddle exp(-2 pi i k / M) = entry 2k of the table
                const double ar = xr[i], ai = xi[i], br = xr[i + M / 2], bi = xi[i + M / 2];
                const double wr = s_tw[2 * k], wi = s_tw[M + 2 * k];
                const double dr = ar - br, di = ai - bi;
                yr[o] = ar + br; yi[o] = ai + bi;
                yr[o + s] = dr * wr - di * wi; yi[o + s] = dr * wi + di * wr;
            }
            double* t;
            t = xr; xr = yr; yr = t; t = xi; xi = yi; yi = t;
        }
        __syncthreads();
        // ---- X[k] = E[k] + w^k O[k] from Z[k] and Z[M - k]; the power of bin k goes to yr[k]
#pragma unroll
        for (int r = 0; r < M / 64; ++r) {
            const int k = lane + 64 * r, km = (M - k) & (M - 1);
            const double zr = xr[k], zi = xi[k], mr = xr[km], mi = xi[km];
            const double er = 0.5 * (zr + mr), ei = 0.5 * (zi - mi);
            const double orr = 0.5 * (zi + mi), oi = -0.5 * (zr - mr);
            const double wr = s_tw[k], wi = s_tw[M + k];
            const double Xr = er + (wr * orr - wi * oi), Xi = ei + (wr * oi + wi * orr);
            yr[k] = Xr * Xr + Xi * Xi;
        }
        __syncthreads();
        const int t = t0 + f;
        if (t < m) {                                                // wave-uniform
            for (int j = lane; j < F; j += 64) {
                const int first = s_bank[j][0], cnt = s_bank[j][1], off = s_bank[j][2];
                double e = 0.0;
                for (int i = 0; i < cnt; ++i) e += (double)s_wt[off + i] * yr[first + i];
                // log(max(e, 2^-23)); at the floor the constant, float(-23 ln 2), whatever logf rounds to there
                const float ef = (float)e;
                outb[(size_t)t * F + j] = ef > 1.1920928955078125e-07f ? logf(ef) : -15.942384719848633f;
            }
        }
    }
}

template <int N, typename TW>
int fbank_launch(hipStream_t st, int B, const FbankArgs& p) {
    const int Sl = p.S < p.W ? p.S : p.W;
    const size_t dyn = fbank_fft_lds<N>() + sizeof(float) * ((size_t)(S2T_FBANK_TILE_ELEMS / N - 1) * Sl + p.W);
    if (fbank_static_lds<N>() + dyn > 60000) {                      // N = 1024, or N = 512 with a shift near the window: asked for on every such call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fbank_kernel<N, TW>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(fbank_fft_lds<N>() + sizeof(float) * S2T_FBANK_TILE_ELEMS));
        if (e != hipSuccess) return S2T_EHIP(e);
    }
    hipLaunchKernelGGL((fbank_kernel<N, TW>), dim3((unsigned)(B * p.tiles)), dim3(FB_THREADS), dyn, st, p);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

// ------------------------------------------------------------------ CMVN
constexpr int CM_THREADS = 1024;

template <int CW>
__global__ __launch_bounds__(CM_THREADS) void cmvn_kernel(float* x, const void* lengths, int len_elem, int Tmax, int F, int* out_len, int* status) {
    constexpr int G = CM_THREADS / CW;                              // row groups
    __shared__ float s_part[CM_THREADS];
    __shared__ float s_mean[CW], s_inv[CW];
    __shared__ int s_any;
    const int b = blockIdx.x, tid = threadIdx.x, c = tid % CW, g = tid / CW;
    const long long len = int_at(lengths, len_elem, b);
    const bool refused = len < 0 || len > Tmax;
    const int m = refused || len < 2 ? 0 : (int)len;                // one frame has no variance: no features
    float* xb = x + (size_t)b * Tmax * F;
    if (tid == 0) {
        out_len[b] = m;
        status[b] = refused ? 2 : m == 0 ? 1 : 0;
        s_any = 0;
    }
    const bool col = c < F;
    const float x0 = col && m ? xb[c] : 0.f;
    // ---- mean, over the differences from the first frame
    float acc = 0.f;
    if (col) {
#pragma unroll 4
        for (int t = g; t < m; t += G) acc += xb[(size_t)t * F + c] - x0;
    }
    s_part[tid] = acc;
    __syncthreads();
    if (tid < CW) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) sum += s_part[k * CW + tid];
        s_mean[tid] = x0 + sum / (float)max(m, 1);
    }
    __syncthreads();
    const float mean = s_mean[c];
    // ---- unbiased variance, over the differences from the mean
    acc = 0.f;
    if (col) {
#pragma unroll 4
        for (int t = g; t < m; t += G) { const float d = xb[(size_t)t * F + c] - mean; acc += d * d; }
    }
    s_part[tid] = acc;
    __syncthreads();
    float var = 0.f;
    if (tid < CW) {
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < G; ++k) sum += s_part[k * CW + tid];
        var = sum / (float)max(m - 1, 1);
        if (col && m && var < 1e-8f) s_any = 1;                     // every writer stores the same value
    }
    __syncthreads();
    if (tid < CW) s_inv[tid] = s_any ? 1.f / (sqrtf(var) + 1e-8f) : 1.f / sqrtf(var);
    __syncthreads();
    const float inv = s_inv[c];
    if (col) {
#pragma unroll 4
        for (int t = g; t < m; t += G) { const size_t i = (size_t)t * F + c; xb[i] = (xb[i] - mean) * inv; }
    }
    // ---- the padding
    const size_t z0 = (size_t)m * F, z1 = (size_t)Tmax * F;
    for (size_t i = z0 + tid; i < z1; i += CM_THREADS) xb[i] = 0.f;
}

}  // namespace

extern "C" int s2t_fbank(const void* waves, int wave_elem, long long row_stride, const long long* lengths, int B, int Nmax, int W, int S,
                         int N, int F, int Tmax, const float* window, const double* twiddle, const int* bank, const float* weights,
                         int n_weights, int remove_dc, double preemph, float* out, int* out_len, int* status, void* stream) {
    if (B <= 0) return S2T_OK;
    if (!waves || !lengths || !window || !twiddle || !bank || !weights || !out || !out_len || !status) return S2T_EINVAL;
    if (wave_elem != 2 && wave_elem != 4) return S2T_EINVAL;
    if (Nmax < 0 || row_stride < 0 || W < 1 || S < 1 || F < 1 || n_weights < 0) return S2T_EINVAL;
    if (Tmax != (Nmax < W ? 0 : 1 + (Nmax - W) / S)) return S2T_EINVAL;
    if (!(preemph == preemph) || preemph < 0.0 || preemph > 1.0) return S2T_EINVAL;
    if (N != 256 && N != 512 && N != 1024) return S2T_ENOTSUP;
    if (W <= N / 2 || W > N) return S2T_ENOTSUP;
    if (F > S2T_FBANK_MAX_BINS || n_weights > N) return S2T_ENOTSUP;
    const int FT = S2T_FBANK_TILE_ELEMS / N;
    const long long tiles = Tmax > 0 ? (Tmax + FT - 1) / FT : 1;    // an utterance without frames still gets its status and length
    if ((long long)B * tiles > 0x7fffffffLL) return S2T_ENOTSUP;
    FbankArgs p;
    p.waves = waves; p.lengths = lengths; p.window = window; p.twiddle = twiddle; p.bank = bank; p.weights = weights;
    p.out = out; p.out_len = out_len; p.status = status; p.row_stride = row_stride;
    p.Nmax = Nmax; p.W = W; p.S = S; p.F = F; p.Tmax = Tmax; p.tiles = (int)tiles; p.n_weights = n_weights; p.remove_dc = remove_dc != 0;
    p.preemph = preemph;
    hipStream_t st = (hipStream_t)stream;
    const bool i16 = wave_elem == 2;
    if (N == 256) return i16 ? fbank_launch<256, short>(st, B, p) : fbank_launch<256, float>(st, B, p);
    if (N == 512) return i16 ? fbank_launch<512, short>(st, B, p) : fbank_launch<512, float>(st, B, p);
    return i16 ? fbank_launch<1024, short>(st, B, p) : fbank_launch<1024, float>(st, B, p);
}

extern "C" int s2t_cmvn(float* x, const void* lengths, int len_elem, int B, int Tmax, int F, int* out_len, int* status, void* stream) {
    if (B <= 0) return S2T_OK;
    if (!x || !lengths || !out_len || !status) return S2T_EINVAL;
    if (len_elem != 4 && len_elem != 8) return S2T_EINVAL;
    if (Tmax < 0 || F < 1) return S2T_EINVAL;
    if (F > S2T_FBANK_MAX_BINS) return S2T_ENOTSUP;
    hipStream_t st = (hipStream_t)stream;
    if (F <= 32) hipLaunchKernelGGL((cmvn_kernel<32>), dim3(B), dim3(CM_THREADS), 0, st, x, lengths, len_elem, Tmax, F, out_len, status);
    else if (F <= 64) hipLaunchKernelGGL((cmvn_kernel<64>), dim3(B), dim3(CM_THREADS), 0, st, x, lengths, len_elem, Tmax, F, out_len, status);
    else hipLaunchKernelGGL((cmvn_kernel<128>), dim3(B), dim3(CM_THREADS), 0, st, x, lengths, len_elem, Tmax, F, out_len, status);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
