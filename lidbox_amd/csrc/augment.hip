// augment.hip -- the reference's two signal augmentations on ragged batches, gfx950.
//
// Replaces (reference file:line):
//   lidbox/features/audio.py:37-47     scipy_resample / pyfunc_resample  (scipy.signal.resample, Fourier method)
//   lidbox/features/audio.py:64-78     scipy_lfilter / random_gaussian_fir_filter  (scipy.signal.lfilter(f, 1, x))
//   lidbox/data/steps.py:331-368       random_signal_speed_change / random_signal_fir_filtering
//
// Resampling.  scipy.signal.resample(x, M) of a real x of N samples is irfft_M(Y) * M / N with Y = the first
// K = min(N, M)//2 + 1 bins of rfft_N(x) (bin min(N, M)/2 doubled when M < N, halved when M > N if min(N, M) is even).
// Both transforms are chirp-z (Bluestein) transforms, each a circular convolution of power-of-two length P done with
// three FFTs: stage 0 (P1 >= N + K - 1) turns N samples into K bins, stage 1 (P2 >= K + M - 1) turns K bins into M
// samples.  The chirp filter's transform is computed in the same batch (its own two passes), never on the host.
//
// Power-of-two FFTs: in-place radix-4 (plus one radix-2) decimation in frequency in LDS; the spectrum is left in
// digit-reversed order, the pointwise product is taken in that order, and the inverse is the exact adjoint of the
// forward stages, which returns natural order -- no permutation pass anywhere.  P <= 16384 is one workgroup in LDS.
// Larger P = N1 * N2 is a four-step transform in global memory, in 4096-point tiles (32 KiB of LDS, so several
// workgroups share a CU): a column pass (N1-point FFTs over a tile of columns, twiddle W_P^(n2 k1)), a row pass (N2-point FFT, product with the filter, inverse, conjugate twiddle) and an inverse
// column pass.  The chirp pre-multiply reads the input in the first pass; the chirp post-multiply, the Nyquist fix-up,
// the doubling of the half spectrum and the 1/N scale sit in the last pass; the 1/P of the convolution is folded into
// the filter.  Utterances are grouped by transform size on the host: launches scale with the number of distinct
// sizes (and with B / RS_GROUP), not with B.
//
// FIR: y[n] = sum_{k<K} f[k] x[n-k], summed in the fixed order k = 0, 1, ..., K-1 for every output, so a result does
// not depend on the batch it was computed in.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int RS_MAX_LOG_LEN = 21;           // N, M <= 2^21 samples
constexpr int RS_LDS_LOG = 14;               // P <= 16384 complex points (128 KiB): one workgroup per transform
constexpr int RS_TILE_LOG = 12;              // four-step tiles: 4096 points (32 KiB), several workgroups per CU
constexpr int RS_TILE_POINTS = 1 << RS_TILE_LOG;
constexpr int RS_TILE_THREADS = 256;
constexpr int RS_TW_LOG = 14;                // twiddle table: e^{-2 pi i t / 16384}, t < 16384
constexpr int RS_THREADS = 1024;
constexpr int RS_GROUP = 256;                // utterances per launch

struct RsArgs {
    const float* x;
    const int64_t* in_starts;
    const int64_t* in_lengths;
    float* y;
    const int64_t* out_starts;
    const int64_t* out_lengths;
    float2* ws;                // slot i of this launch: filter [P] then data [P] at ws + 2 P i
    const float2* tw;
    float2* spec;              // stage-0 output / stage-1 input: utterance b at spec + b * kmax
    long kmax;
    int stage, logP, log1, log2, count;
    int utt[RS_GROUP];
};

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

// e^{i sgn pi n^2 / L}: n^2 reduced mod 2L in 64-bit integers, so the fp32 phase is exact up to one rounding
__device__ __forceinline__ float2 chirp(long n, long L, float sgn) {
    const long r = (n * n) % (2 * L);
    float s, c;
    sincospif((float)r / (float)L, &s, &c);
    return make_float2(c, sgn * s);
}

// W_P^x = e^{-2 pi i x / P}, 0 <= x < P (x and 2x/P are exact in fp32)
__device__ __forceinline__ float2 twiddle_p(long x, int logP) {
    float s, c;
    sincospif(ldexpf((float)x, 1 - logP), &s, &c);
    return make_float2(c, -s);
}

// frequency held at position j after the forward stages below (radix-4 digits from the largest block down, then radix 2)
__device__ __forceinline__ int digit_perm(int j, int logn) {
    int k = 0, sh = 0, logm = logn;
    while (logm >= 2) {
        logm -= 2;
        k |= ((j >> logm) & 3) << sh;
        sh += 2;
    }
    if (logm == 1) k |= (j & 1) << sh;
    return k;
}

// `count` transforms of 2^logn points in LDS.  COLS: element e of transform t at a[e * count + t] (a tile of
// columns), else at a[t * n + e] (rows).  Ends with a barrier.
template <bool COLS, bool INV>
__device__ void radix4_stage(float2* a, int logn, int logcount, int logm, const float2* __restrict__ tw) {
    const int logq = logm - 2, q = 1 << logq, tws = RS_TW_LOG - logm;
    const int total = 1 << (logcount + logn - 2);
    for (int w = threadIdx.x; w < total; w += blockDim.x) {
        int t, bf;
        if (COLS) { t = w & ((1 << logcount) - 1); bf = w >> logcount; }
        else { bf = w & ((1 << (logn - 2)) - 1); t = w >> (logn - 2); }
        const int j = bf & (q - 1), base = ((bf >> logq) << logm) + j;
        const int stride = COLS ? (q << logcount) : q;
        float2* p = COLS ? a + ((long)base << logcount) + t : a + ((long)t << logn) + base;
        const float2 w1 = tw[j << tws], w2 = tw[(2 * j) << tws], w3 = tw[(3 * j) << tws];
        float2 x0 = p[0], x1 = p[stride], x2 = p[2 * stride], x3 = p[3 * stride];
        if (!INV) {
            const float2 s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = csub(x1, x3);
            p[0] = cadd(s02, s13);
            p[stride] = cmul(make_float2(d02.x + d13.y, d02.y - d13.x), w1);
            p[2 * stride] = cmul(csub(s02, s13), w2);
            p[3 * stride] = cmul(make_float2(d02.x - d13.y, d02.y + d13.x), w3);
        } else {
            x1 = cmulc(x1, w1);
            x2 = cmulc(x2, w2);
            x3 = cmulc(x3, w3);
            const float2 s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = csub(x1, x3);
            p[0] = cadd(s02, s13);
            p[stride] = make_float2(d02.x - d13.y, d02.y + d13.x);
            p[2 * stride] = csub(s02, s13);
            p[3 * stride] = make_float2(d02.x + d13.y, d02.y - d13.x);
        }
    }
    __syncthreads();
}

template <bool COLS>
__device__ void radix2_stage(float2* a, int logn, int logcount) {
    const int total = 1 << (logcount + logn - 1);
    for (int w = threadIdx.x; w < total; w += blockDim.x) {
        int t, bf;
        if (COLS) { t = w & ((1 << logcount) - 1); bf = w >> logcount; }
        else { bf = w & ((1 << (logn - 1)) - 1); t = w >> (logn - 1); }
        const int stride = COLS ? (1 << logcount) : 1;
        float2* p = COLS ? a + ((long)(2 * bf) << logcount) + t : a + ((long)t << logn) + 2 * bf;
        const float2 x0 = p[0], x1 = p[stride];
        p[0] = cadd(x0, x1);
        p[stride] = csub(x0, x1);
    }
    __syncthreads();
}

// forward: natural order in, digit-reversed out (unnormalised e^{-2 pi i nk/n}); inverse: the adjoint of forward
template <bool COLS, bool INV>
__device__ void lds_fft(float2* a, int logn, int logcount, const float2* __restrict__ tw) {
    if (!INV) {
        int logm = logn;
        for (; logm >= 2; logm -= 2) radix4_stage<COLS, false>(a, logn, logcount, logm, tw);
        if (logm == 1) radix2_stage<COLS>(a, logn, logcount);
    } else {
        if (logn & 1) radix2_stage<COLS>(a, logn, logcount);
        for (int logm = (logn & 1) + 2; logm <= logn; logm += 2) radix4_stage<COLS, true>(a, logn, logcount, logm, tw);
    }
}

struct Utt {
    long N, M, K, in, out, L;
    float s;
    int b;
};

__device__ __forceinline__ Utt utt_of(const RsArgs& a, int i) {
    Utt u;
    u.b = a.utt[i];
    u.N = a.in_lengths[u.b];
    u.M = a.out_lengths[u.b];
    u.K = min(u.N, u.M) / 2 + 1;
    if (a.stage == 0) { u.in = u.N; u.out = u.K; u.L = u.N; u.s = 1.f; }
    else { u.in = u.K; u.out = u.M; u.L = u.M; u.s = -1.f; }
    return u;
}

// chirp filter of the convolution: e^{i s pi d^2 / L} at d in [0, out) and at P - d for d in [1, in)
__device__ __forceinline__ float2 filter_at(const Utt& u, long n, long P) {
    const long d = n < u.out ? n : (n > P - u.in ? P - n : -1);
    return d >= 0 ? chirp(d, u.L, u.s) : make_float2(0.f, 0.f);
}

// convolution input: stage 0 = x * chirp, stage 1 = the premultiplied spectrum
__device__ __forceinline__ float2 input_at(const RsArgs& a, const Utt& u, long n) {
    if (a.stage == 0) {
        if (n >= u.N) return make_float2(0.f, 0.f);
        return cscale(chirp(n, u.N, -1.f), a.x[a.in_starts[u.b] + n]);
    }
    return n < u.K ? a.spec[u.b * a.kmax + n] : make_float2(0.f, 0.f);
}

// output n of the convolution (n < out): stage 0 -> bin n of Y, times the stage-1 chirp; stage 1 -> sample n
__device__ __forceinline__ void epilogue(const RsArgs& a, const Utt& u, long n, float2 v) {
    if (n >= u.out) return;
    if (a.stage == 0) {
        float2 t = cmul(v, chirp(n, u.N, -1.f));
        const long mn = min(u.N, u.M);
        if (n == 0) t.y = 0.f;                                           // irfft reads the real part of bin 0
        if ((mn & 1) == 0 && n == mn / 2) t = cscale(t, u.M < u.N ? 2.f : (u.M > u.N ? 0.5f : 1.f));
        if ((u.M & 1) == 0 && n == u.M / 2) t.y = 0.f;                   // ... and of bin M/2
        else if (n > 0) t = cscale(t, 2.f);                              // the half spectrum counts twice
        a.spec[u.b * a.kmax + n] = cmul(t, chirp(n, u.M, 1.f));
    } else {
        a.y[a.out_starts[u.b] + n] = cmul(v, chirp(n, u.M, 1.f)).x / (float)u.N;
    }
}

__global__ __launch_bounds__(256) void rs_twiddle_kernel(float2* tw) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (1 << RS_TW_LOG)) {
        double s, c;
        sincospi((double)t / (double)(1 << (RS_TW_LOG - 1)), &s, &c);
        tw[t] = make_float2((float)c, (float)-s);
    }
}

// four-step pass 1: N1-point FFTs over a tile of T columns; FILTER: the chirp filter, else the convolution input
template <bool FILTER>
__global__ __launch_bounds__(RS_THREADS) void rs_col_fwd_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* lds = reinterpret_cast<float2*>(smem);
    const int i = blockIdx.y;
    const Utt u = utt_of(a, i);
    const long P = 1L << a.logP;
    const int logT = RS_TILE_LOG - a.log1, N2 = 1 << a.log2;
    const long c0 = (long)blockIdx.x << logT;
    float2* dst = a.ws + 2 * P * i + (FILTER ? 0 : P);
    for (int idx = threadIdx.x; idx < RS_TILE_POINTS; idx += blockDim.x) {
        const long n = (long)(idx >> logT) * N2 + c0 + (idx & ((1 << logT) - 1));
        lds[idx] = FILTER ? filter_at(u, n, P) : input_at(a, u, n);
    }
    __syncthreads();
    lds_fft<true, false>(lds, a.log1, logT, a.tw);
    for (int idx = threadIdx.x; idx < RS_TILE_POINTS; idx += blockDim.x) {
        const int e = idx >> logT;
        const long c = c0 + (idx & ((1 << logT) - 1));
        dst[(long)e * N2 + c] = cmul(lds[idx], twiddle_p(c * digit_perm(e, a.log1), a.logP));
    }
}

// four-step pass 2 (or the whole transform when N1 = 1): N2-point FFTs over R rows.
// CONV = false: transform of the filter, scaled by 1/P, stored in place.
// CONV = true: forward, product with the filter, inverse; then the conjugate twiddle (N1 > 1) or the epilogue (N1 = 1).
template <bool CONV>
__global__ __launch_bounds__(RS_THREADS) void rs_row_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* lds = reinterpret_cast<float2*>(smem);
    const int i = blockIdx.y;
    const Utt u = utt_of(a, i);
    const long P = 1L << a.logP;
    const int logR = a.log1 ? RS_TILE_LOG - a.log2 : 0, N2 = 1 << a.log2;
    const long r0 = (long)blockIdx.x << logR;
    float2* filt = a.ws + 2 * P * i;
    float2* data = filt + P;
    const int elems = 1 << (logR + a.log2);
    for (int idx = threadIdx.x; idx < elems; idx += blockDim.x) {
        const long g = (r0 << a.log2) + idx;
        if (a.log1) lds[idx] = CONV ? data[g] : filt[g];
        else lds[idx] = CONV ? input_at(a, u, g) : filter_at(u, g, P);
    }
    __syncthreads();
    lds_fft<false, false>(lds, a.log2, logR, a.tw);
    if (!CONV) {
        const float inv_p = ldexpf(1.f, -a.logP);
        for (int idx = threadIdx.x; idx < elems; idx += blockDim.x) filt[(r0 << a.log2) + idx] = cscale(lds[idx], inv_p);
        return;
    }
    for (int idx = threadIdx.x; idx < elems; idx += blockDim.x) lds[idx] = cmul(lds[idx], filt[(r0 << a.log2) + idx]);
    __syncthreads();
    lds_fft<false, true>(lds, a.log2, logR, a.tw);
    for (int idx = threadIdx.x; idx < elems; idx += blockDim.x) {
        const long e = idx & (N2 - 1);
        if (a.log1) {
            const long r = r0 + (idx >> a.log2);
            data[(r << a.log2) + e] = cmulc(lds[idx], twiddle_p(e * digit_perm((int)r, a.log1), a.logP));
        } else {
            epilogue(a, u, e, lds[idx]);
        }
    }
}

// four-step pass 3: inverse N1-point FFTs over a tile of columns, then the epilogue
__global__ __launch_bounds__(RS_THREADS) void rs_col_inv_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* lds = reinterpret_cast<float2*>(smem);
    const int i = blockIdx.y;
    const Utt u = utt_of(a, i);
    const long P = 1L << a.logP;
    const int logT = RS_TILE_LOG - a.log1, N2 = 1 << a.log2;
    const long c0 = (long)blockIdx.x << logT;
    const float2* data = a.ws + 2 * P * i + P;
    for (int idx = threadIdx.x; idx < RS_TILE_POINTS; idx += blockDim.x)
        lds[idx] = data[(long)(idx >> logT) * N2 + c0 + (idx & ((1 << logT) - 1))];
    __syncthreads();
    lds_fft<true, true>(lds, a.log1, logT, a.tw);
    for (int idx = threadIdx.x; idx < RS_TILE_POINTS; idx += blockDim.x)
        epilogue(a, u, (long)(idx >> logT) * N2 + c0 + (idx & ((1 << logT) - 1)), lds[idx]);
}

// ------------------------------------------------------------------ FIR
constexpr int FIR_THREADS = 256, FIR_PER_LANE = 8, FIR_TILE = FIR_THREADS * FIR_PER_LANE;
constexpr int FIR_MAX_COEFS = 4096;

__device__ __forceinline__ int fir_halo(int K) { return (K + 2) / 4 * 4 + 4; }     // multiple of 4, >= K + 3

// one block per (utterance, tile stride); a lane computes 8 consecutive outputs from a sliding window of LDS float4s
__global__ __launch_bounds__(FIR_THREADS) void fir_kernel(const float* __restrict__ x, const int64_t* __restrict__ starts,
                                                           const int64_t* __restrict__ lengths, const float* __restrict__ coefs,
                                                           int K, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* f = reinterpret_cast<float*>(smem);
    const int H = fir_halo(K);
    float* xs = f + (K + 3) / 4 * 4;                   // xs[i] = x[t0 - H + i]
    const int b = blockIdx.x;
    const long n = lengths[b], s = starts[b];
    for (int k = threadIdx.x; k < K; k += FIR_THREADS) f[k] = coefs[(long)b * K + k];
    for (long t0 = (long)blockIdx.y * FIR_TILE; t0 < n; t0 += (long)gridDim.y * FIR_TILE) {
        __syncthreads();
        for (int i = threadIdx.x; i < H + FIR_TILE; i += FIR_THREADS) {
            const long g = t0 - H + i;
            xs[i] = (g >= 0 && g < n) ? x[s + g] : 0.f;
        }
        __syncthreads();
        const long j0 = t0 + FIR_PER_LANE * threadIdx.x;
        if (j0 >= n) continue;
        const int base = H + FIR_PER_LANE * threadIdx.x;                  // xs index of x[j0], a multiple of 4
        // window w[0..11] = xs[base - 4q - 4 .. base - 4q + 8) for the taps k = 4q .. 4q+3
        float w[12];
        *reinterpret_cast<float4*>(&w[0]) = *reinterpret_cast<const float4*>(&xs[base - 4]);
        *reinterpret_cast<float4*>(&w[4]) = *reinterpret_cast<const float4*>(&xs[base]);
        *reinterpret_cast<float4*>(&w[8]) = *reinterpret_cast<const float4*>(&xs[base + 4]);
        float acc[FIR_PER_LANE];
        const float f0 = f[0];
#pragma unroll
        for (int j = 0; j < FIR_PER_LANE; ++j) acc[j] = f0 * w[j + 4];
        int q = 0;
        for (; 4 * q + 4 <= K; ++q) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                if (q == 0 && kk == 0) continue;                           // tap 0 initialised acc
                const float fk = f[4 * q + kk];
#pragma unroll
                for (int j = 0; j < FIR_PER_LANE; ++j) acc[j] = fmaf(fk, w[j - kk + 4], acc[j]);
            }
#pragma unroll
            for (int i = 11; i >= 4; --i) w[i] = w[i - 4];
            *reinterpret_cast<float4*>(&w[0]) = *reinterpret_cast<const float4*>(&xs[base - 4 * q - 8]);
        }
#pragma unroll
        for (int kk = 0; kk < 3; ++kk) {                                   // the last K mod 4 taps
            if ((q == 0 && kk == 0) || 4 * q + kk >= K) continue;
            const float fk = f[4 * q + kk];
#pragma unroll
            for (int j = 0; j < FIR_PER_LANE; ++j) acc[j] = fmaf(fk, w[j - kk + 4], acc[j]);
        }
        float* out = y + s + j0;
        if (((s + j0) & 3) == 0 && j0 + FIR_PER_LANE <= n) {
            reinterpret_cast<float4*>(out)[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            reinterpret_cast<float4*>(out)[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
        } else {
#pragma unroll
            for (int j = 0; j < FIR_PER_LANE; ++j)
                if (j0 + j < n) out[j] = acc[j];
        }
    }
}

// ------------------------------------------------------------------ host planning
inline int ceil_log2(long v) {
    int l = 0;
    while ((1L << l) < v) ++l;
    return l;
}

struct RsPlan {
    std::vector<int> logP[2];       // per utterance and stage; -1 = nothing to do
    long kmax = 0;
    size_t region_pts = 0;          // float2 points of the larger stage's slots
    bool any = false;
};

int rs_make_plan(const int64_t* in_len, const int64_t* out_len, int B, RsPlan& p) {
    LBX_ARG(B >= 0, "B must be >= 0");
    LBX_ARG(B == 0 || (in_len && out_len), "host length arrays are required");
    p.logP[0].assign(B, -1);
    p.logP[1].assign(B, -1);
    size_t pts[2] = {0, 0};
    for (int b = 0; b < B; ++b) {
        const long N = in_len[b], M = out_len[b];
        if (N < 0 || M < 0 || N > (1L << RS_MAX_LOG_LEN) || M > (1L << RS_MAX_LOG_LEN)) {
            lidbox_set_error("lidbox_resample: utterance %d: %ld -> %ld samples is outside the supported range "
                             "0 .. 2^%d = %ld samples", b, N, M, RS_MAX_LOG_LEN, 1L << RS_MAX_LOG_LEN);
            return LIDBOX_E_INVALID;
        }
        if (N == 0 && M > 0) {
            lidbox_set_error("lidbox_resample: utterance %d: an empty signal cannot be resampled to %ld samples", b, M);
            return LIDBOX_E_INVALID;
        }
        if (N == 0 || M == 0) continue;
        const long K = std::min(N, M) / 2 + 1;
        p.logP[0][b] = ceil_log2(N + K - 1);
        p.logP[1][b] = ceil_log2(K + M - 1);
        for (int s = 0; s < 2; ++s) pts[s] += 2 * ((size_t)1 << p.logP[s][b]);
        p.kmax = std::max(p.kmax, K);
        p.any = true;
    }
    p.region_pts = std::max(pts[0], pts[1]);
    return 0;
}

// bytes: twiddles | spectra (B x kmax) | the slots of the larger stage
size_t rs_bytes(const RsPlan& p, int B) {
    if (!p.any) return 0;
    return ((size_t)1 << RS_TW_LOG) * sizeof(float2) + (size_t)B * p.kmax * sizeof(float2) + p.region_pts * sizeof(float2);
}

hipError_t rs_allow_large_lds() {
    const int big = 160 * 1024;
    hipError_t e = hipFuncSetAttribute((const void*)rs_col_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rs_col_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rs_row_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rs_row_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)rs_col_inv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, big);
    return e;
}

}  // namespace

extern "C" size_t lidbox_resample_workspace(const int64_t* in_lengths_host, const int64_t* out_lengths_host, int B) {
    RsPlan p;
    if (rs_make_plan(in_lengths_host, out_lengths_host, B, p) != 0) return 0;
    return rs_bytes(p, B);
}

extern "C" int lidbox_resample(const float* signals, const int64_t* in_starts, const int64_t* in_lengths, float* out,
                               const int64_t* out_starts, const int64_t* out_lengths, const int64_t* in_lengths_host,
                               const int64_t* out_lengths_host, int B, void* workspace, size_t workspace_bytes,
                               lidbox_stream_t stream) {
    RsPlan p;
    const int st = rs_make_plan(in_lengths_host, out_lengths_host, B, p);
    if (st != 0) return st;
    if (!p.any) return 0;
    LBX_ARG(signals && in_starts && in_lengths && out && out_starts && out_lengths, "null pointer");
    LBX_ARG(workspace && workspace_bytes >= rs_bytes(p, B), "workspace smaller than lidbox_resample_workspace()");
    LBX_ARG(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    static const hipError_t attr = rs_allow_large_lds();
    LBX_HIP(attr);
    hipStream_t s = (hipStream_t)stream;
    float2* tw = reinterpret_cast<float2*>(workspace);
    float2* spec = tw + (1 << RS_TW_LOG);
    float2* region = spec + (size_t)B * p.kmax;
    hipLaunchKernelGGL(rs_twiddle_kernel, dim3((1 << RS_TW_LOG) / 256), dim3(256), 0, s, tw);
    LBX_LAUNCH_OK();

    RsArgs a{};
    a.x = signals; a.in_starts = in_starts; a.in_lengths = in_lengths;
    a.y = out; a.out_starts = out_starts; a.out_lengths = out_lengths;
    a.tw = tw; a.spec = spec; a.kmax = p.kmax;
    std::vector<int> order;
    for (int stage = 0; stage < 2; ++stage) {
        const std::vector<int>& lp = p.logP[stage];
        order.clear();
        for (int b = 0; b < B; ++b)
            if (lp[b] >= 0) order.push_back(b);
        std::stable_sort(order.begin(), order.end(), [&](int u, int v) { return lp[u] < lp[v]; });
        a.stage = stage;
        size_t slot = 0;
        for (size_t g = 0; g < order.size();) {
            const int logP = lp[order[g]];
            int cnt = 0;
            while (g + cnt < order.size() && cnt < RS_GROUP && lp[order[g + cnt]] == logP) {
                a.utt[cnt] = order[g + cnt];
                ++cnt;
            }
            a.count = cnt;
            a.logP = logP;
            a.log1 = logP > RS_LDS_LOG ? logP / 2 : 0;
            a.log2 = logP - a.log1;
            a.ws = region + slot;
            if (a.log1) {
                const dim3 grid(1u << (logP - RS_TILE_LOG), cnt), block(RS_TILE_THREADS);
                const size_t lds = RS_TILE_POINTS * sizeof(float2);
                hipLaunchKernelGGL(rs_col_fwd_kernel<true>, grid, block, lds, s, a);
                hipLaunchKernelGGL(rs_row_kernel<false>, grid, block, lds, s, a);
                hipLaunchKernelGGL(rs_col_fwd_kernel<false>, grid, block, lds, s, a);
                hipLaunchKernelGGL(rs_row_kernel<true>, grid, block, lds, s, a);
                hipLaunchKernelGGL(rs_col_inv_kernel, grid, block, lds, s, a);
            } else {                                  // 8 points per thread, 64 .. 1024 threads
                const dim3 grid(1, cnt), block(std::min(RS_THREADS, std::max(64, (1 << logP) / 8)));
                const size_t lds = ((size_t)1 << logP) * sizeof(float2);
                hipLaunchKernelGGL(rs_row_kernel<false>, grid, block, lds, s, a);
                hipLaunchKernelGGL(rs_row_kernel<true>, grid, block, lds, s, a);
            }
            LBX_LAUNCH_OK();
            slot += (size_t)cnt * 2 << logP;
            g += cnt;
        }
    }
    return 0;
}

extern "C" int lidbox_fir_filter(const float* signals, const int64_t* starts, const int64_t* lengths, int B,
                                 long max_length, const float* coefs, int num_coefs, float* out, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && max_length >= 0, "B and max_length must be >= 0");
    LBX_ARG(num_coefs >= 1 && num_coefs <= FIR_MAX_COEFS, "num_coefs must be in 1 .. 4096");
    if (B == 0 || max_length == 0) return 0;
    LBX_ARG(signals && starts && lengths && coefs && out, "null pointer");
    const int tiles = (int)std::min<long>(lbx_cdiv(max_length, FIR_TILE), 64);
    const size_t lds = ((size_t)(num_coefs + 3) / 4 * 4 + (num_coefs + 2) / 4 * 4 + 4 + FIR_TILE) * sizeof(float);
    hipLaunchKernelGGL(fir_kernel, dim3(B, tiles), dim3(FIR_THREADS), lds, (hipStream_t)stream, signals, starts, lengths,
                       coefs, num_coefs, out);
    LBX_LAUNCH_OK();
    return 0;
}
