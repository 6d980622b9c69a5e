// conv2d.hip -- Keras Conv2D(padding="same", stride 1), BatchNormalization + MaxPool2D(2) and the kernels' L2 penalty, gfx950.
//
// Replaces (reference file:line): lidbox/models/crnn.py:36-41, one block of five:
//     Conv2D(f, k, activation="relu", padding="same", kernel_regularizer=l2(weight_decay)) -> BatchNormalization()
//     -> MaxPool2D(2)
// The reference convolves an image [B, F, T, C] (height = frequency, width = time).  Here images are stored time-major,
// [B, T, F, C] with channels innermost, so the model input [B, T, F] is already the first block's image and the last pool
// output [B, T5, F5, C] is already the BLSTM's input [B, T5, F5 * C] in Keras' feature order.  The kernel keeps the Keras
// layout W[kh][kw][C_in][C_out] with kh over frequency and kw over time:
//     y[b, t, f, co] = relu(bias[co] + sum_{kh, kw, ci} x[b, t + kw - p, f + kh - p, ci] W[kh, kw, ci, co]),  p = (k - 1) / 2
// with x zero outside the image (no halo in storage: the operand loaders test the bounds).
//
// Forward is an implicit GEMM on fp32 MFMA (v_mfma_f32_16x16x4_f32): rows are output pixels m = (b, t, f), the contraction
// runs over kidx = (kh, kw, ci) in the Keras order, so the B operand is W viewed as [k*k*C_in, C_out]; no im2col copy
// exists.  A workgroup (4 waves) owns 128 pixels x BN output channels (BN = 16, 32 or 64) and walks the contraction in
// chunks of 16 through LDS, loading the next chunk into registers while the current one feeds the MFMAs.  Every output is
// one k-chain in a fixed order that does not depend on the pixel's place in the batch: an utterance gives the same bits
// alone or inside a batch.
//
// dgrad (stride 1, same padding) is the same convolution of dY with the kernel rotated by 180 degrees and C_in / C_out
// swapped: a small launch writes that copy into the workspace and the forward kernel runs on it.
//
// wgrad: dW[kidx][co] = sum_m xshift[m][kidx] dY[m][co] is the same tile code with rows = kidx and the contraction over
// pixels.  The pixels are split into P fixed partitions (P depends on the shape only); each workgroup writes its partial
// tile to the workspace, workgroups of the first kidx tile also the partial column sums of dY (the bias gradient), and a
// second launch sums the partials in a fixed order.  No atomics: bit-identical from run to run.
//
// The stride-1 kernels and the strided ones further down (clstm's Conv2D) are one tile program: tile_clear, tile_pipeline
// (register-to-LDS staging and the double-buffered main loop), tile_walk (the 16x16 C/D map with the element store as a
// callable), wgrad_chunks (pipeline + bias column sums) and wgrad_store (partial tile + bias row) stand once; a kernel keeps
// its geometry, its row / tap decomposition and its load.  On the host with_tile_n turns the tile width into a template
// argument for all four launches and run_wgrad is the body of both wgrad entry points.
//
// BN-apply + MaxPool2D: one pass reads the conv output, applies the BatchNormalization scale / shift (gamma may be
// negative, so normalisation comes first) and takes the 2 x 2 maximum ("valid": an odd last row / column is dropped).
// Ties go to the FIRST maximum in the reference image's scan order -- lower frequency row first, then lower time column
// (TF's MaxPoolGrad and torch.nn.functional.max_pool2d) -- and the winner's code 2 * dfreq + dtime is kept for backward,
// which gathers: each input cell takes its window's gradient when it is the recorded winner, zero otherwise (and zero for
// the dropped cells).
//
// Ragged forward (inference on utterances of different lengths laid end to end): the forward kernels of both families and the
// pool once more at the end of the file, with the time bounds and T / 2 of each row's own utterance; nothing above them changed.
#include <stdint.h>

#include <type_traits>

#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CV_BM = 128;            // tile rows: 4 waves x 32
constexpr int CV_KC = 16;             // contraction elements per LDS chunk
constexpr int CV_LDA = CV_BM + 16;    // 16 (mod 64) banks between the 4 k rows a wave reads at once
template <int BN>
constexpr int cv_ldb() { return BN == 16 ? 16 : BN + 16; }

struct ConvGeom {
    int B, T, F, Cin, Cout, ks, pad;
    long M;          // B * T * F pixels
    int K;           // ks * ks * Cin
};

// the contraction index kidx = (kh, kw, ci) -> (time offset, frequency offset, element offset from the pixel's own x row)
struct KTap {
    int dt, df;
    long delta;
    bool ok;
};

__device__ __forceinline__ KTap ktap(const ConvGeom& g, int kidx) {
    KTap r;
    r.ok = kidx < g.K;
    const int kk = r.ok ? kidx : 0;
    const int ci = kk % g.Cin, q = kk / g.Cin;
    r.dt = q % g.ks - g.pad;            // kw: time
    r.df = q / g.ks - g.pad;            // kh: frequency
    r.delta = ((long)r.dt * g.F + r.df) * g.Cin + ci;
    return r;
}

// acc[i][j] += As[0..16)[rows w*32 + 16 i ..] . Bs[0..16)[16 j ..] over one LDS chunk
template <int BN>
__device__ __forceinline__ void mma_lds_chunk(f32x4 (&acc)[2][BN / 16], const float* As, const float* Bs, int w, int lane) {
    constexpr int LDB = cv_ldb<BN>();
    const int c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int kq = 0; kq < CV_KC; kq += 4) {
        const int k = kq + g;
        float a[2], b[BN / 16];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = As[k * CV_LDA + w * 32 + 16 * i + c];
#pragma unroll
        for (int j = 0; j < BN / 16; ++j) b[j] = Bs[k * LDB + 16 * j + c];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < BN / 16; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------- the tile pipeline
// One program for the four tile kernels below: a workgroup of 256 threads owns a 128 x BN tile, walks its contraction
// [lo, hi) in chunks of CV_KC through As [CV_KC][CV_LDA] and Bs [CV_KC][cv_ldb] and holds the next chunk in registers
// (av, bv) while the current one feeds the MFMAs.  A kernel brings its geometry and `load(c)`, which fills av and bv for the
// chunk at c (zeros outside the tile, the image or the contraction), and names the A layout that its load produces:
//     A_ROWS  thread (kk = tid & 15, r0 = tid >> 4) holds A[row r0 + 16 j][k kk]       (forward, dgrad: k is innermost in x)
//     A_KIDX  thread (kk = tid & 127, p0 = tid >> 7) holds A[row kk][k p0 + 2 j]       (wgrad: the row is innermost in x)
// B is the same in all four: element e = tid + 256 q of the chunk's [CV_KC][BN] block.
// Source forms that the compiled code depends on (docs/LAB_NOTEBOOK.md section 19): the kernel issues the first load itself
// and hands down its own tid, w and lane; tile_walk gets its row and column bases, and the store it calls captures by value,
// never a reference to a kernel argument.
enum ALayout { A_ROWS, A_KIDX };

template <ALayout L>
__device__ __forceinline__ void tile_stage_a(float (&As)[CV_KC * CV_LDA], const float (&av)[8], int tid) {
    if (L == A_ROWS) {
        const int kk = tid & 15, r0 = tid >> 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) As[kk * CV_LDA + r0 + 16 * j] = av[j];
    } else {
        const int kk = tid & 127, p0 = tid >> 7;
#pragma unroll
        for (int j = 0; j < 8; ++j) As[(p0 + 2 * j) * CV_LDA + kk] = av[j];
    }
}

template <int BN>
__device__ __forceinline__ void tile_stage_b(float (&Bs)[CV_KC * cv_ldb<BN>()], const float (&bv)[CV_KC * BN / 256], int tid) {
#pragma unroll
    for (int q = 0; q < CV_KC * BN / 256; ++q) {
        const int e = tid + 256 * q, kr = e / BN, n = e - kr * BN;
        Bs[kr * cv_ldb<BN>() + n] = bv[q];
    }
}

template <int BN>
__device__ __forceinline__ void tile_clear(f32x4 (&acc)[2][BN / 16]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < BN / 16; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

struct NoChunkHook {
    __device__ __forceinline__ void operator()(const float*) const {}
};

// acc += the chunks of [lo, hi) (I: int or long, the type load takes).  The caller has called load(lo) when the range is not
// empty.  hook(Bs) runs once per chunk between the prefetch of the next chunk and the MFMAs, with the current chunk in
// LDS: wgrad sums dY's columns there.
template <int BN, ALayout L, typename I, typename Load, typename Hook = NoChunkHook>
__device__ __forceinline__ void tile_pipeline(f32x4 (&acc)[2][BN / 16], const float (&av)[8],
                                              const float (&bv)[CV_KC * BN / 256], int tid, int w, int lane, I lo, I hi,
                                              const Load& load, const Hook& hook = Hook()) {
    __shared__ __attribute__((aligned(16))) float As[CV_KC * CV_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[CV_KC * cv_ldb<BN>()];
    for (I c = lo; c < hi; c += CV_KC) {
        __syncthreads();                                  // the previous chunk's LDS reads are done
        tile_stage_a<L>(As, av, tid);
        tile_stage_b<BN>(Bs, bv, tid);
        __syncthreads();
        if (c + CV_KC < hi) load(c + CV_KC);
        hook(Bs);
        mma_lds_chunk<BN>(acc, As, Bs, w, lane);
    }
}

// The 16x16 C/D map of the tile at (row0, col0): lane (c, q4) of wave w holds column col0 + 16 j + c of rows row0 + w * 32 +
// 16 i + 4 q4 + r.  store(row, col, v, t) gets each element with its place (row in R, int or long) and t = colv[col], the
// kernel's per-column term (the bias), or 0 when colv is NULL.
template <int BN, typename R, typename Store>
__device__ __forceinline__ void tile_walk(const f32x4 (&acc)[2][BN / 16], int w, int lane, R row0, int col0,
                                          const float* __restrict__ colv, const Store& store) {
    const int c = lane & 15, q4 = lane >> 4;
#pragma unroll
    for (int j = 0; j < BN / 16; ++j) {
        const int n = col0 + 16 * j + c;
        const float t = colv ? colv[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) store(row0 + w * 32 + 16 * i + 4 * q4 + r, n, acc[i][j][r], t);
    }
}

// wgrad, both families, grid (ceil(K / 128), Cout / BN, P): rows are kidx, the contraction runs over the pixels [mlo, mhi)
// of partition p = blockIdx.z.  Workgroups of the first kidx tile also sum dY's columns (the bias gradient) from the B chunk
// in LDS, one thread per column and chunk rows in order.
template <int BN, typename Load>
__device__ __forceinline__ void wgrad_chunks(f32x4 (&acc)[2][BN / 16], float& dbacc, const float (&av)[8],
                                             const float (&bv)[CV_KC * BN / 256], int tid, int w, int lane, long mlo, long mhi,
                                             const Load& load) {
    const bool bias_tile = blockIdx.x == 0;
    tile_pipeline<BN, A_KIDX>(acc, av, bv, tid, w, lane, mlo, mhi, load, [&dbacc, bias_tile, tid](const float* Bs) {
        if (bias_tile && tid < BN) {
#pragma unroll
            for (int pr = 0; pr < CV_KC; ++pr) dbacc += Bs[pr * cv_ldb<BN>() + tid];
        }
    });
}

// part[kidx][co][p] = the partial tile (rows < K), dbpart[co][p] = the partial column sums
template <int BN>
__device__ __forceinline__ void wgrad_store(const f32x4 (&acc)[2][BN / 16], float dbacc, int tid, int w, int lane,
                                            float* __restrict__ part, float* __restrict__ dbpart, int K, int Cout, int P) {
    const int k0 = blockIdx.x * CV_BM, n0 = blockIdx.y * BN, p = blockIdx.z;
    tile_walk<BN>(acc, w, lane, k0, n0, nullptr, [=](int kr, int n, float v, float) {
        if (kr < K) part[((long)kr * Cout + n) * P + p] = v;
    });
    if (blockIdx.x == 0 && tid < BN) dbpart[(long)(n0 + tid) * P + p] = dbacc;
}

// ---------------------------------------------------------------------------------------------- forward (and dgrad)
// grid (ceil(M / 128), Cout / BN); thread (kk = tid & 15, r0 = tid >> 4) loads A[r0 + 16 j][kk], j < 8
template <int BN>
__global__ __launch_bounds__(256) void conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                       const float* __restrict__ bias, int relu, float* __restrict__ y,
                                                       const ConvGeom g) {
    constexpr int BQ = CV_KC * BN / 256;      // B-operand loads per thread and chunk (1, 2 or 4)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long m0 = (long)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * BN;
    const int kk = tid & 15, r0 = tid >> 4;
    int tt[8], ff[8];
    bool rok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long m = m0 + r0 + 16 * j;
        rok[j] = m < g.M;
        const long mm = rok[j] ? m : 0;
        ff[j] = (int)(mm % g.F);
        tt[j] = (int)((mm / g.F) % g.T);
    }
    float av[8], bv[BQ];
    auto load = [&](int kc) {
        const KTap tp = ktap(g, kc + kk);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t2 = tt[j] + tp.dt, f2 = ff[j] + tp.df;
            const bool ok = rok[j] && tp.ok && (unsigned)t2 < (unsigned)g.T && (unsigned)f2 < (unsigned)g.F;
            av[j] = ok ? x[(m0 + r0 + 16 * j) * g.Cin + tp.delta] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, kr = e / BN, n = e - kr * BN;
            bv[q] = kc + kr < g.K ? W[(long)(kc + kr) * g.Cout + n0 + n] : 0.0f;
        }
    };
    f32x4 acc[2][BN / 16];
    tile_clear<BN>(acc);
    load(0);
    tile_pipeline<BN, A_ROWS>(acc, av, bv, tid, w, lane, 0, g.K, load);
    tile_walk<BN>(acc, w, lane, m0, n0, bias, [y, relu, M = g.M, Cout = g.Cout](long m, int n, float v, float bb) {
        if (m >= M) return;
        v += bb;
        if (relu) v = fmaxf(v, 0.0f);
        y[m * Cout + n] = v;
    });
}

// Wd[kh'][kw'][co][ci] = W[k-1-kh'][k-1-kw'][ci][co]: the kernel of the transposed convolution
__global__ __launch_bounds__(256) void conv_rot_kernel(const float* __restrict__ W, float* __restrict__ Wd, int ks, int Cin,
                                                       int Cout) {
    const long n = (long)ks * ks * Cin * Cout;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        long q = i / Cin;
        const int co = (int)(q % Cout);
        q /= Cout;
        const int kw = (int)(q % ks), kh = (int)(q / ks);
        Wd[i] = W[(((long)(ks - 1 - kh) * ks + (ks - 1 - kw)) * Cin + ci) * Cout + co];
    }
}

// ---------------------------------------------------------------------------------------------- wgrad
// grid (ceil(K / 128), Cout / BN, P).  Partition p covers pixels [p * per, min(M, (p + 1) * per)).  Thread (kk = tid & 127,
// p0 = tid >> 7) loads A[pixel p0 + 2 j][kidx kk], j < 8.
template <int BN>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         float* __restrict__ part, float* __restrict__ dbpart, long per,
                                                         int P, const ConvGeom g) {
    constexpr int BQ = CV_KC * BN / 256;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int k0 = blockIdx.x * CV_BM, n0 = blockIdx.y * BN, p = blockIdx.z;
    const long mlo = (long)p * per, mhi = min(g.M, mlo + per);
    const int kk = tid & 127, p0 = tid >> 7;
    const KTap tp = ktap(g, k0 + kk);
    float av[8], bv[BQ];
    auto load = [&](long mc) {
        // (t, f) of pixel mc + p0, then stepped by 2 pixels
        long m = mc + p0;
        int f = (int)(m % g.F), t = (int)((m / g.F) % g.T);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t2 = t + tp.dt, f2 = f + tp.df;
            const bool ok = m < mhi && tp.ok && (unsigned)t2 < (unsigned)g.T && (unsigned)f2 < (unsigned)g.F;
            av[j] = ok ? x[m * g.Cin + tp.delta] : 0.0f;
            m += 2;
            f += 2;
            while (f >= g.F) {
                f -= g.F;
                if (++t == g.T) t = 0;
            }
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, pr = e / BN, n = e - pr * BN;
            bv[q] = mc + pr < mhi ? dy[(mc + pr) * g.Cout + n0 + n] : 0.0f;
        }
    };
    f32x4 acc[2][BN / 16];
    float dbacc = 0.0f;
    tile_clear<BN>(acc);
    if (mlo < mhi) load(mlo);
    wgrad_chunks<BN>(acc, dbacc, av, bv, tid, w, lane, mlo, mhi, load);
    wgrad_store<BN>(acc, dbacc, tid, w, lane, part, dbpart, g.K, g.Cout, P);
}

// dW[i] = sum_p part[i][p] (i < K * Cout), db[co] = sum_p dbpart[co][p], in a fixed order.  Few partitions (P < 64): one
// thread per output, p in order.  Many: one wave per output, lane l sums p = l, l + 64, ... in order, then a fixed xor tree.
__device__ __forceinline__ const float* wgrad_src(const float* part, const float* dbpart, int P, long nw, long i) {
    return i < nw ? part + i * P : dbpart + (i - nw) * P;
}

__device__ __forceinline__ float* wgrad_dst(float* dW, float* db, long nw, long i) { return i < nw ? dW + i : db + (i - nw); }

__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbpart,
                                                                int P, long nw, long n, float* __restrict__ dW,
                                                                float* __restrict__ db) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const float* src = wgrad_src(part, dbpart, P, nw, i);
    float s = 0.0f;
    for (int p = 0; p < P; ++p) s += src[p];
    *wgrad_dst(dW, db, nw, i) = s;
}

__global__ __launch_bounds__(256) void conv_wgrad_reduce_wide_kernel(const float* __restrict__ part,
                                                                     const float* __restrict__ dbpart, int P, long nw, long n,
                                                                     float* __restrict__ dW, float* __restrict__ db) {
    const long i = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (i >= n) return;                                       // whole waves leave together: wave_sum stays uniform
    const int lane = threadIdx.x & 63;
    const float* src = wgrad_src(part, dbpart, P, nw, i);
    float s = 0.0f;
    for (int p = lane; p < P; p += 64) s += src[p];
    s = wave_sum(s);
    if (lane == 0) *wgrad_dst(dW, db, nw, i) = s;
}

// ---------------------------------------------------------------------------------------------- BN-apply + MaxPool2D
__global__ __launch_bounds__(256) void bn_maxpool_fwd_kernel(const float* __restrict__ x, int T, int F, int C,
                                                             const float* __restrict__ scale, const float* __restrict__ shift,
                                                             float* __restrict__ y, uint8_t* __restrict__ code, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int T2 = T / 2, F2 = F / 2;
    const int c = (int)(i % C);
    long q = i / C;
    const int f2 = (int)(q % F2);
    q /= F2;
    const int t2 = (int)(q % T2);
    const long b = q / T2;
    const float* p = x + (((b * T + 2 * t2) * F) + 2 * f2) * C + c;
    const float sc = scale[c], sh = shift[c];
    // the reference image's scan order: (freq 0, time 0), (freq 0, time 1), (freq 1, time 0), (freq 1, time 1)
    const long off[4] = {0, (long)F * C, C, (long)F * C + C};
    float best = p[off[0]] * sc + sh;
    int bc = 0;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
        const float v = p[off[e]] * sc + sh;
        if (v > best) {
            best = v;
            bc = e;
        }
    }
    y[i] = best;
    code[i] = (uint8_t)bc;
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ code, int T,
                                                          int F, int C, float* __restrict__ dx, long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int T2 = T / 2, F2 = F / 2;
    const int c = (int)(i % C);
    long q = i / C;
    const int f = (int)(q % F);
    q /= F;
    const int t = (int)(q % T);
    const long b = q / T;
    float v = 0.0f;
    if ((t >> 1) < T2 && (f >> 1) < F2) {
        const long o = ((b * T2 + (t >> 1)) * F2 + (f >> 1)) * C + c;
        if (code[o] == (uint8_t)(2 * (f & 1) + (t & 1))) v = dy[o];
    }
    dx[i] = v;
}

// ---------------------------------------------------------------------------------------------- L2 penalty
constexpr int L2_MAX = 16;
constexpr int L2_BLOCKS = 128;

struct L2Args {
    const float* w[L2_MAX];
    float* g[L2_MAX];
    long n[L2_MAX];
    float lam[L2_MAX];
    int count;
    float gscale;
    float* partial;      // [L2_BLOCKS] (NULL: no loss)
};

// workgroup b owns the slice [b per, (b + 1) per) of the tensors laid end to end: g += 2 lam gscale w there, and
// partial[b] = sum lam w^2 over it (per-thread strided sums, then a fixed tree)
__global__ __launch_bounds__(256) void l2_penalty_kernel(const L2Args a, long per) {
    __shared__ float red[4];
    const long blo = blockIdx.x * per, bhi = blo + per;
    float s = 0.0f;
    long base = 0;
    for (int t = 0; t < a.count; ++t) {
        const long lo = max(blo, base), hi = min(bhi, base + a.n[t]);
        const float* w = a.w[t] - base;
        float* g = a.g[t] ? a.g[t] - base : nullptr;
        const float lam = a.lam[t], k = 2.0f * lam * a.gscale;
        float st = 0.0f;
        for (long i = lo + threadIdx.x; i < hi; i += 256) {
            const float v = w[i];
            if (g) g[i] += k * v;
            st += v * v;
        }
        s += lam * st;
        base += a.n[t];
    }
    if (!a.partial) return;
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void l2_loss_kernel(const float* __restrict__ partial, float* __restrict__ loss) {
    if (threadIdx.x != 0) return;
    float s = 0.0f;
    for (int b = 0; b < L2_BLOCKS; ++b) s += partial[b];
    loss[0] += s;
}

int conv_check(const char* fn, int B, int T, int F, int Cin, int Cout, int ks) {
    // M = B * T * F < 2^31 keeps grid.x = ceil(M / 128) of the forward launch inside what a launch accepts
    if (B < 0 || T < 1 || F < 1 || Cin < 1 || Cout < 16 || Cout % 16 != 0 || ks < 1 || ks % 2 == 0 ||
        (long)B * T * F >= (1L << 31) || (long)B * T * F * (Cin > Cout ? Cin : Cout) >= (1L << 40) ||
        (long)ks * ks * (Cin > Cout ? Cin : Cout) > (1 << 20)) {
        lidbox_set_error("%s: invalid argument: B >= 0, T, F, C_in >= 1, C_out a multiple of 16, odd k, sizes in range", fn);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

ConvGeom geom(int B, int T, int F, int Cin, int Cout, int ks) {
    return ConvGeom{B, T, F, Cin, Cout, ks, (ks - 1) / 2, (long)B * T * F, ks * ks * Cin};
}

int conv_tile_n(int Cout) { return Cout % 64 == 0 ? 64 : Cout % 32 == 0 ? 32 : 16; }

// f(std::integral_constant<int, bn>): the one place that turns conv_tile_n's value into a template argument
template <typename F>
void with_tile_n(int bn, F&& f) {
    if (bn == 64)
        f(std::integral_constant<int, 64>());
    else if (bn == 32)
        f(std::integral_constant<int, 32>());
    else
        f(std::integral_constant<int, 16>());
}

int launch_fwd(const float* x, const float* W, const float* bias, int relu, float* y, const ConvGeom& g, hipStream_t st) {
    const int bn = conv_tile_n(g.Cout);
    const dim3 grid((unsigned)lbx_cdiv(g.M, CV_BM), (unsigned)(g.Cout / bn));
    with_tile_n(bn, [&](auto BN) { hipLaunchKernelGGL(conv_fwd_kernel<BN()>, grid, dim3(256), 0, st, x, W, bias, relu, y, g); });
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

// wgrad partitions: enough workgroups to cover the chip about four times, at least 512 pixels each, at most 1024 partitions
void wgrad_plan_kmn(long K, long M, int Cout, int* P, long* per) {
    const long tiles = lbx_cdiv(K, CV_BM) * (Cout / conv_tile_n(Cout));
    long p = lbx_cdiv(1024, tiles);
    p = p < lbx_cdiv(M, 512) ? p : lbx_cdiv(M, 512);
    p = p < 1024 ? p : 1024;
    p = p > 1 ? p : 1;
    const long chunks = lbx_cdiv(lbx_cdiv(M, CV_KC), p);
    *per = chunks * CV_KC;
    *P = (int)p;
}

// P partial tiles [K][Cout] and P partial bias rows [Cout]
size_t wgrad_workspace_bytes(long K, long M, int Cout) {
    int P;
    long per;
    wgrad_plan_kmn(K, M, Cout, &P, &per);
    return (size_t)P * ((size_t)K * Cout + Cout) * sizeof(float);
}

// Both wgrad entry points after their argument checks: dW [K][Cout] and db [Cout] (may be NULL) from M pixels.
// launch(BN, grid, part, dbpart, per, P) starts the family's tile kernel; the reduce kernels are shared.
template <typename Launch>
int run_wgrad(const char* fn, long K, long M, int Cout, float* dW, float* db, void* workspace, size_t workspace_bytes,
              hipStream_t st, Launch&& launch) {
    const long nw = K * Cout;
    if (M == 0) {
        LBX_HIP(hipMemsetAsync(dW, 0, nw * sizeof(float), st));
        if (db) LBX_HIP(hipMemsetAsync(db, 0, Cout * sizeof(float), st));
        return LIDBOX_OK;
    }
    if (!(workspace && workspace_bytes >= wgrad_workspace_bytes(K, M, Cout) && ((uintptr_t)workspace & 15) == 0)) {
        lidbox_set_error("%s: invalid argument: workspace >= %s_workspace() bytes, 16-byte aligned", fn, fn);
        return LIDBOX_E_INVALID;
    }
    int P;
    long per;
    wgrad_plan_kmn(K, M, Cout, &P, &per);
    float* part = (float*)workspace;
    float* dbpart = part + (long)P * nw;
    const int bn = conv_tile_n(Cout);
    const dim3 grid((unsigned)lbx_cdiv(K, CV_BM), (unsigned)(Cout / bn), (unsigned)P);
    with_tile_n(bn, [&](auto BN) { launch(BN, grid, part, dbpart, per, P); });
    LBX_LAUNCH_OK();
    const long nout = nw + (db ? Cout : 0);
    if (P >= 64)
        hipLaunchKernelGGL(conv_wgrad_reduce_wide_kernel, dim3((unsigned)lbx_cdiv(nout, 4)), dim3(256), 0, st, part, dbpart, P, nw,
                           nout, dW, db);
    else
        hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3((unsigned)lbx_cdiv(nout, 256)), dim3(256), 0, st, part, dbpart, P, nw, nout,
                           dW, db);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

// ============================================================================================== strided, rectangular Conv2D
// lidbox/models/clstm.py:51-60: Conv2D(C_out, (kt, kf), strides=(1, sf), padding="same") on the time-major image
// x [B][T][F][C_in]; explicit zero rows / columns before and after (pt0, pt1, pf0, pf1), so
//     y[b, to, fo, co] = bias[co] + sum_{i, j, ci} x[b, to + i - pt0, fo sf + j - pf0, ci] W[tap(i, j), ci, co]
// with To = T + pt0 + pt1 - kt + 1 and Fo = (F + pf0 + pf1 - kf) / sf + 1, and tap(i, j) = i kf + j when the Keras kernel's
// first axis is time (clstm) or j kt + i when it is frequency (crnn's order).  The tiles are the 128 x BN MFMA tiles above.
// Forward: a tile is 128 rows (b, to) of ONE output column fo, so its k-chain holds only the frequency taps that land
// inside the image for that column (at F = 40 conv2d_2 reads 5 of 9 taps per column) -- in the Keras order of the taps,
// one fixed chain per column: an utterance gives the same bits alone or inside a batch.
// dgrad: a tile is 128 rows (b, t) of one input column f; the taps that reach it are j = (f + pf0) mod sf + m sf with
// output column fo = (f + pf0 - j) / sf inside [0, Fo), one or two at sf = 6 -- a gather, no zero insertion.  The kernel
// is read through a per-tap transposed copy Wt[tap][co][ci] in the workspace (contiguous over the output channels ci).
// wgrad: rows = kidx (Keras order), contraction over pixels u = (fo, b, to) in fixed partitions as for stride 1; a
// (tile, partition) pair whose frequency taps all fall in the padding for every column of the partition skips its chunks
// (the bias tile never skips).  Partials are reduced by the stride-1 reduce kernels: bit-identical from run to run.
struct SGeom {
    int B, T, F, Cin, Cout;
    int To, Fo;
    int kt, kf, sf, pt, pf;
    int tfirst;
    int K;           // kt * kf * Cin
};

__device__ __forceinline__ int sg_tap(const SGeom& g, int i, int j) { return g.tfirst ? i * g.kf + j : j * g.kt + i; }

// forward: grid (ceil(B To / 128), Fo, Cout / BN).  dgrad (DG): grid (ceil(B T / 128), F, Cin / BN), W = Wt, y = dx.
template <int BN, bool DG>
__global__ __launch_bounds__(256) void sconv_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                    const float* __restrict__ bias, float* __restrict__ y, const SGeom g) {
    constexpr int BQ = CV_KC * BN / 256;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = blockIdx.y;                      // fo (forward) / f (dgrad)
    const int n0 = blockIdx.z * BN;
    const int Rt = DG ? g.T : g.To;                  // rows per utterance of this launch's output
    const long R = (long)g.B * Rt;
    const long r0t = (long)blockIdx.x * CV_BM;
    const int Ncol = DG ? g.Cin : g.Cout;            // output channels
    const int Kc = DG ? g.Cout : g.Cin;              // contraction channels per tap
    // the tile's taps: nj frequency taps (j = j0 + jstep * m, m < nj), each with all kt time taps
    int j0, jstep, nj, fo0 = 0;
    if (!DG) {
        const int f0 = col * g.sf - g.pf;
        j0 = max(0, -f0);
        nj = max(0, min(g.kf, g.F - f0) - j0);
        jstep = 1;
    } else {
        const int jf = (col + g.pf) % g.sf, q0 = (col + g.pf) / g.sf;
        const int mlo = max(0, q0 - g.Fo + 1), mhi = min((g.kf - jf + g.sf - 1) / g.sf, q0 + 1);
        nj = max(0, mhi - mlo);
        j0 = jf + mlo * g.sf;
        jstep = g.sf;
        fo0 = q0 - mlo;                              // output column of tap j0; tap m reads fo0 - m
    }
    const int Kv = g.kt * nj * Kc;
    const int kk = tid & 15, r0 = tid >> 4;
    int bb[8], tt[8];
    bool rok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long r = r0t + r0 + 16 * j;
        rok[j] = r < R;
        const long rr = rok[j] ? r : 0;
        bb[j] = (int)(rr / Rt);
        tt[j] = (int)(rr - (long)bb[j] * Rt);
    }
    // contraction index v -> (time tap i, frequency tap m, channel c) in the Keras order of the taps
    auto split = [&](int v, int& i, int& m, int& c) {
        c = v % Kc;
        const int q = v / Kc;
        if (g.tfirst) {
            i = q / nj;
            m = q - i * nj;
        } else {
            m = q / g.kt;
            i = q - m * g.kt;
        }
    };
    float av[8], bv[BQ];
    auto load = [&](int kc) {
        const int v = kc + kk;
        const bool vok = v < Kv;
        int i, m, c;
        split(vok ? v : 0, i, m, c);
        const int j = j0 + jstep * m;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (!DG) {
                const int t2 = tt[s] + i - g.pt, f2 = col * g.sf + j - g.pf;
                const bool ok = vok && rok[s] && (unsigned)t2 < (unsigned)g.T;
                av[s] = ok ? x[(((long)bb[s] * g.T + t2) * g.F + f2) * g.Cin + c] : 0.0f;
            } else {
                const int to = tt[s] - i + g.pt, fo = fo0 - m;
                const bool ok = vok && rok[s] && (unsigned)to < (unsigned)g.To;
                av[s] = ok ? x[(((long)bb[s] * g.To + to) * g.Fo + fo) * g.Cout + c] : 0.0f;
            }
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, kr = e / BN, n = e - kr * BN;
            const int v2 = kc + kr;
            float b = 0.0f;
            if (v2 < Kv) {
                int i2, m2, c2;
                split(v2, i2, m2, c2);
                const long tap = sg_tap(g, i2, j0 + jstep * m2);
                b = DG ? W[(tap * g.Cout + c2) * g.Cin + n0 + n] : W[(tap * g.Cin + c2) * g.Cout + n0 + n];
            }
            bv[q] = b;
        }
    };
    f32x4 acc[2][BN / 16];
    tile_clear<BN>(acc);
    if (Kv > 0) load(0);
    tile_pipeline<BN, A_ROWS>(acc, av, bv, tid, w, lane, 0, Kv, load);
    const int Fcol = DG ? g.F : g.Fo;
    tile_walk<BN>(acc, w, lane, r0t, n0, DG ? nullptr : bias, [y, R, Fcol, col, Ncol](long row, int n, float v, float bb0) {
        if (row >= R) return;
        y[(row * Fcol + col) * Ncol + n] = v + bb0;      // row = b Rt + t: pixel (b, t, col)
    });
}

// Wt[tap][co][ci] = W[tap][ci][co]
__global__ __launch_bounds__(256) void sconv_transpose_kernel(const float* __restrict__ W, float* __restrict__ Wt, int taps,
                                                              int Cin, int Cout) {
    const long n = (long)taps * Cin * Cout;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int ci = (int)(i % Cin);
        const long q = i / Cin;
        const int co = (int)(q % Cout);
        const long tap = q / Cout;
        Wt[i] = W[(tap * Cin + ci) * Cout + co];
    }
}

// grid (ceil(K / 128), Cout / BN, P); partition p covers pixels u in [p per, min(M, (p + 1) per)), u = (fo, b, to)
template <int BN>
__global__ __launch_bounds__(256) void sconv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          float* __restrict__ part, float* __restrict__ dbpart, long per,
                                                          int P, const SGeom g) {
    constexpr int BQ = CV_KC * BN / 256;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int k0 = blockIdx.x * CV_BM, n0 = blockIdx.y * BN, p = blockIdx.z;
    const long BTo = (long)g.B * g.To, M = BTo * g.Fo;
    const long mlo = (long)p * per, mhi = min(M, mlo + per);
    const int kk = tid & 127, p0 = tid >> 7;
    const bool bias_tile = blockIdx.x == 0;
    auto tap_of = [&](int kidx, int& i, int& j) {
        const int tap = kidx / g.Cin;
        if (g.tfirst) {
            i = tap / g.kf;
            j = tap - i * g.kf;
        } else {
            j = tap / g.kt;
            i = tap - j * g.kt;
        }
    };
    const int kidx = k0 + kk;
    const bool kok = kidx < g.K;
    int ti, tj;
    tap_of(kok ? kidx : 0, ti, tj);
    const int ci = (kok ? kidx : 0) % g.Cin;
    // skip: no frequency tap of this tile lands inside the image for any column of this partition
    bool live = bias_tile;
    if (!live && mlo < mhi) {
        int jmin = g.kf, jmax = -1;
        const int klast = min(g.K, k0 + CV_BM) - 1;
        for (int tap = k0 / g.Cin; tap <= klast / g.Cin; ++tap) {
            int i, j;
            tap_of(tap * g.Cin, i, j);
            jmin = min(jmin, j);
            jmax = max(jmax, j);
        }
        for (int fo = (int)(mlo / BTo); fo <= (int)((mhi - 1) / BTo) && !live; ++fo)
            live = fo * g.sf + jmax - g.pf >= 0 && fo * g.sf + jmin - g.pf < g.F;
    }
    float av[8], bv[BQ];
    auto load = [&](long mc) {
        long u = mc + p0;
        int fo = (int)(u / BTo);
        long r = u - (long)fo * BTo;
        int b = (int)(r / g.To), to = (int)(r - (long)b * g.To);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t2 = to + ti - g.pt, f2 = fo * g.sf + tj - g.pf;
            const bool ok = u < mhi && kok && (unsigned)t2 < (unsigned)g.T && (unsigned)f2 < (unsigned)g.F;
            av[j] = ok ? x[(((long)b * g.T + t2) * g.F + f2) * g.Cin + ci] : 0.0f;
            u += 2;
            to += 2;
            while (to >= g.To) {
                to -= g.To;
                if (++b == g.B) {
                    b = 0;
                    ++fo;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, pr = e / BN, n = e - pr * BN;
            const long uu = mc + pr;
            float v = 0.0f;
            if (uu < mhi) {
                const int fo2 = (int)(uu / BTo);
                const long r2 = uu - (long)fo2 * BTo;       // = b To + to
                v = dy[(r2 * g.Fo + fo2) * g.Cout + n0 + n];
            }
            bv[q] = v;
        }
    };
    f32x4 acc[2][BN / 16];
    float dbacc = 0.0f;
    tile_clear<BN>(acc);
    if (live) {
        if (mlo < mhi) load(mlo);
        wgrad_chunks<BN>(acc, dbacc, av, bv, tid, w, lane, mlo, mhi, load);
    }
    wgrad_store<BN>(acc, dbacc, tid, w, lane, part, dbpart, g.K, g.Cout, P);
}

// ---------------------------------------------------------------------------------------------- BN-apply + ReLU (+ max over F)
// v = x scale[c] + shift[c] (one fmaf, the same expression in every pass so forward and backward agree bit for bit)
__device__ __forceinline__ float bn_v(float x, float sc, float sh) { return fmaf(x, sc, sh); }

__global__ __launch_bounds__(256) void bn_relu_fwd_kernel(const float* __restrict__ x, long n, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, float* __restrict__ y) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const float v = bn_v(x[i], scale[c], shift[c]);
        y[i] = v > 0.0f ? v : 0.0f;
    }
}

// dx = dy * (x scale + shift > 0): ReLU's gradient dy (input > 0) with the BatchNormalization output as its input
__global__ __launch_bounds__(256) void bn_relu_bwd_kernel(const float* __restrict__ x, long n, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* dy, float* dx) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        dx[i] = bn_v(x[i], scale[c], shift[c]) > 0.0f ? dy[i] : 0.0f;
    }
}

// y[b][t][c] (ybs floats between utterances, rows of C) = max_f relu(x[b][t][f][c] scale + shift)
__global__ __launch_bounds__(256) void bn_relu_maxf_fwd_kernel(const float* __restrict__ x, int T, int F, int C,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               float* __restrict__ y, long ybs, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long r = i / C;                        // b T + t
        const long b = r / T;
        const float sc = scale[c], sh = shift[c];
        const float* p = x + r * F * C + c;
        float m = 0.0f;
        for (int f = 0; f < F; ++f) m = fmaxf(m, bn_v(p[(long)f * C], sc, sh));
        y[b * ybs + (r - b * T) * C + c] = m;
    }
}

// TF's _MinOrMaxGrad: dy split evenly over every f whose relu(v) equals the maximum (indicator / count * dy), then ReLU's
// gradient (v > 0); ties at zero therefore get nothing.  dx [B][T][F][C] = the gradient of the BatchNormalization output.
__global__ __launch_bounds__(256) void bn_relu_maxf_bwd_kernel(const float* __restrict__ x, int T, int F, int C,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ dy, long dbs, float* __restrict__ dx,
                                                               long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long r = i / C;
        const long b = r / T;
        const float sc = scale[c], sh = shift[c];
        const float* p = x + r * F * C + c;
        float m = 0.0f;
        for (int f = 0; f < F; ++f) m = fmaxf(m, bn_v(p[(long)f * C], sc, sh));
        int cnt = 0;
        for (int f = 0; f < F; ++f) {
            const float v = bn_v(p[(long)f * C], sc, sh);
            cnt += (v > 0.0f ? v : 0.0f) == m;
        }
        const float g = (1.0f / (float)cnt) * dy[b * dbs + (r - b * T) * C + c];
        float* q = dx + r * F * C + c;
        for (int f = 0; f < F; ++f) {
            const float v = bn_v(p[(long)f * C], sc, sh);
            q[(long)f * C] = (v > 0.0f && v == m) ? g : 0.0f;
        }
    }
}

int sconv_check(const char* fn, int B, int T, int F, int Cin, int Cout, const lidbox_conv2d_taps_t& k) {
    const long To = (long)T + k.pt0 + k.pt1 - k.kt + 1, Fo = F + k.pf0 + k.pf1 >= k.kf && k.sf >= 1 ? (F + k.pf0 + k.pf1 - k.kf) / k.sf + 1 : 0;
    const int cmax = Cin > Cout ? Cin : Cout;
    if (B < 0 || T < 1 || F < 1 || Cin < 1 || Cout < 16 || Cout % 16 != 0 || k.kt < 1 || k.kf < 1 || k.sf < 1 || k.pt0 < 0 ||
        k.pt1 < 0 || k.pf0 < 0 || k.pf1 < 0 || k.pt0 >= k.kt || k.pf0 >= k.kf || To < 1 || Fo < 1 || Fo > 65535 || F > 65535 ||
        (long)B * T * F >= (1L << 31) || (long)B * T * F * cmax >= (1L << 40) || (long)B * To * Fo * cmax >= (1L << 40) ||
        (long)k.kt * k.kf * cmax > (1 << 20)) {
        lidbox_set_error("%s: invalid argument: B >= 0, T, F, C_in >= 1, C_out a multiple of 16, taps / stride >= 1, pads >= 0 "
                         "and before < taps, at least one output row and column, sizes in range", fn);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

SGeom sgeom(int B, int T, int F, int Cin, int Cout, const lidbox_conv2d_taps_t& k) {
    SGeom g;
    g.B = B; g.T = T; g.F = F; g.Cin = Cin; g.Cout = Cout;
    g.To = T + k.pt0 + k.pt1 - k.kt + 1;
    g.Fo = (F + k.pf0 + k.pf1 - k.kf) / k.sf + 1;
    g.kt = k.kt; g.kf = k.kf; g.sf = k.sf; g.pt = k.pt0; g.pf = k.pf0;
    g.tfirst = k.time_first ? 1 : 0;
    g.K = k.kt * k.kf * Cin;
    return g;
}

template <bool DG>
int launch_sconv(const float* x, const float* W, const float* bias, float* y, const SGeom& g, hipStream_t st) {
    const int Ncol = DG ? g.Cin : g.Cout;
    const int bn = conv_tile_n(Ncol);
    const dim3 grid((unsigned)lbx_cdiv((long)g.B * (DG ? g.T : g.To), CV_BM), (unsigned)(DG ? g.F : g.Fo), (unsigned)(Ncol / bn));
    with_tile_n(bn, [&](auto BN) { hipLaunchKernelGGL((sconv_kernel<BN(), DG>), grid, dim3(256), 0, st, x, W, bias, y, g); });
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

// the two weight-copy launches (rotate, transpose): grid-stride over nw elements, at most 1024 workgroups
dim3 wcopy_grid(long nw) { return dim3((unsigned)(lbx_cdiv(nw, 256) < 1024 ? lbx_cdiv(nw, 256) : 1024)); }

int ew_blocks(long n) {
    const long b = lbx_cdiv(n, 256);
    return (int)(b < 8192 ? b : 8192);
}

// ============================================================================================== ragged forward (inference)
// The forward kernels above for B utterances of DIFFERENT lengths stored end to end: utterance b owns the image rows
// off[b] .. off[b + 1] of x and y (no gaps, no halo), off an int64 device array of B + 1 entries rising from 0 that the
// kernels trust.  Storage being contiguous, a pixel's address and its tap's offset are the dense ones with B = 1, T = total_T;
// what changes is the bound a tap's time index is tested against: its own utterance's [0, T_b), looked up in front of the
// contraction loop: one binary search of off per tile for its first row, from which each row steps over the borders in the tile.  Tiles, chunks and the k-chain of every output are the dense
// kernels', so an utterance gets bit for bit what the dense call gives it at B = 1, T = T_b, wherever it lies and whatever
// surrounds it; a tile may span several utterances and an utterance several tiles.  No atomics, nothing between workgroups.

// the utterance that owns row r: the last b with off[b] <= r (0 <= r < off[B]; empty utterances are stepped over)
__device__ __forceinline__ int rg_find(const long* __restrict__ off, int B, long r) {
    int lo = 0, hi = B;                                // off[lo] <= r < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// conv_fwd_kernel on [total_T][F][C]: g.B = utterances, g.T = total_T, g.M = total_T * F; grid (ceil(M / 128), Cout / BN)
template <int BN>
__global__ __launch_bounds__(256) void conv_ragged_fwd_kernel(const float* __restrict__ x, const long* __restrict__ off,
                                                              const float* __restrict__ W, const float* __restrict__ bias,
                                                              int relu, float* __restrict__ y, const ConvGeom g) {
    constexpr int BQ = CV_KC * BN / 256;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long m0 = (long)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * BN;
    const int kk = tid & 15, r0 = tid >> 4;
    int tt[8], tl[8], ff[8];                  // t inside the row's utterance, that utterance's length, f
    bool rok[8];
    // one search per tile, for its first image row (uniform: scalar loads); the thread's rows rise with j, so each steps on
    // from the one before it, over the utterance borders inside the tile
    int b = rg_find(off, g.B, m0 / g.F);
    long lo = off[b], hi = off[b + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long m = m0 + r0 + 16 * j;
        rok[j] = m < g.M;
        const long mm = rok[j] ? m : m0;
        const long row = mm / g.F;
        ff[j] = (int)(mm - row * g.F);
        while (row >= hi && b + 1 < g.B) {    // an empty utterance is stepped over
            ++b;
            lo = hi;
            hi = off[b + 1];
        }
        tt[j] = (int)(row - lo);
        tl[j] = (int)(hi - lo);
    }
    float av[8], bv[BQ];
    auto load = [&](int kc) {
        const KTap tp = ktap(g, kc + kk);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t2 = tt[j] + tp.dt, f2 = ff[j] + tp.df;
            const bool ok = rok[j] && tp.ok && (unsigned)t2 < (unsigned)tl[j] && (unsigned)f2 < (unsigned)g.F;
            av[j] = ok ? x[(m0 + r0 + 16 * j) * g.Cin + tp.delta] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, kr = e / BN, n = e - kr * BN;
            bv[q] = kc + kr < g.K ? W[(long)(kc + kr) * g.Cout + n0 + n] : 0.0f;
        }
    };
    f32x4 acc[2][BN / 16];
    tile_clear<BN>(acc);
    load(0);
    tile_pipeline<BN, A_ROWS>(acc, av, bv, tid, w, lane, 0, g.K, load);
    tile_walk<BN>(acc, w, lane, m0, n0, bias, [y, relu, M = g.M, Cout = g.Cout](long m, int n, float v, float bb) {
        if (m >= M) return;
        v += bb;
        if (relu) v = fmaxf(v, 0.0f);
        y[m * Cout + n] = v;
    });
}

// sconv_kernel<BN, false> for a time geometry that keeps the length (pt0 + pt1 == kt - 1): g.B = utterances, g.T = g.To =
// total_T; a tile is 128 rows (utterance, t) of one output column.  grid (ceil(total_T / 128), Fo, Cout / BN)
template <int BN>
__global__ __launch_bounds__(256) void sconv_ragged_kernel(const float* __restrict__ x, const long* __restrict__ off,
                                                           const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ y, const SGeom g) {
    constexpr int BQ = CV_KC * BN / 256;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = blockIdx.y;
    const int n0 = blockIdx.z * BN;
    const long R = g.To;
    const long r0t = (long)blockIdx.x * CV_BM;
    const int f0 = col * g.sf - g.pf;
    const int j0 = max(0, -f0), nj = max(0, min(g.kf, g.F - f0) - j0);
    const int Kv = g.kt * nj * g.Cin;
    const int kk = tid & 15, r0 = tid >> 4;
    int tt[8], tl[8];
    bool rok[8];
    int b = rg_find(off, g.B, r0t);           // one search per tile (uniform), then steps over the borders inside the tile
    long lo = off[b], hi = off[b + 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long r = r0t + r0 + 16 * j;
        rok[j] = r < R;
        const long rr = rok[j] ? r : r0t;
        while (rr >= hi && b + 1 < g.B) {
            ++b;
            lo = hi;
            hi = off[b + 1];
        }
        tt[j] = (int)(rr - lo);
        tl[j] = (int)(hi - lo);
    }
    auto split = [&](int v, int& i, int& m, int& c) {
        c = v % g.Cin;
        const int q = v / g.Cin;
        if (g.tfirst) {
            i = q / nj;
            m = q - i * nj;
        } else {
            m = q / g.kt;
            i = q - m * g.kt;
        }
    };
    float av[8], bv[BQ];
    auto load = [&](int kc) {
        const int v = kc + kk;
        const bool vok = v < Kv;
        int i, m, c;
        split(vok ? v : 0, i, m, c);
        const int f2 = col * g.sf + j0 + m - g.pf;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int t2 = tt[s] + i - g.pt;
            const bool ok = vok && rok[s] && (unsigned)t2 < (unsigned)tl[s];
            av[s] = ok ? x[((r0t + r0 + 16 * s + i - g.pt) * g.F + f2) * g.Cin + c] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < BQ; ++q) {
            const int e = tid + 256 * q, kr = e / BN, n = e - kr * BN;
            const int v2 = kc + kr;
            float wv = 0.0f;
            if (v2 < Kv) {
                int i2, m2, c2;
                split(v2, i2, m2, c2);
                const long tap = sg_tap(g, i2, j0 + m2);
                wv = W[(tap * g.Cin + c2) * g.Cout + n0 + n];
            }
            bv[q] = wv;
        }
    };
    f32x4 acc[2][BN / 16];
    tile_clear<BN>(acc);
    if (Kv > 0) load(0);
    tile_pipeline<BN, A_ROWS>(acc, av, bv, tid, w, lane, 0, Kv, load);
    tile_walk<BN>(acc, w, lane, r0t, n0, bias, [y, R, Fo = g.Fo, col, Cout = g.Cout](long row, int n, float v, float bb0) {
        if (row >= R) return;
        y[(row * Fo + col) * Cout + n] = v + bb0;
    });
}

// bn_maxpool_fwd_kernel per utterance: output row q of y [total_out][F / 2][C] belongs to the utterance b whose output
// segment oof[b] .. oof[b + 1] holds it, and is written when it is one of that utterance's T_b / 2 pooled rows (the rest of
// a segment is left alone).  code may be NULL.
__global__ __launch_bounds__(256) void bn_maxpool_ragged_fwd_kernel(const float* __restrict__ x, const long* __restrict__ iof,
                                                                    int B, int F, int C, const float* __restrict__ scale,
                                                                    const float* __restrict__ shift, float* __restrict__ y,
                                                                    const long* __restrict__ oof, uint8_t* __restrict__ code,
                                                                    long n) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= n) return;
    const int F2 = F / 2;
    const int c = (int)(i % C);
    long q = i / C;
    const int f2 = (int)(q % F2);
    q /= F2;
    // one search per workgroup, for the row of its first element (uniform), then steps on to this element's row
    int b = rg_find(oof, B, blockIdx.x * 256L / ((long)F2 * C));
    while (b + 1 < B && oof[b + 1] <= q) ++b;
    const long t2 = q - oof[b];
    const long ilo = iof[b];
    if (t2 < 0 || t2 >= (iof[b + 1] - ilo) / 2) return;
    const float* p = x + (((ilo + 2 * t2) * F) + 2 * f2) * C + c;
    const float sc = scale[c], sh = shift[c];
    const long off[4] = {0, (long)F * C, C, (long)F * C + C};
    float best = p[off[0]] * sc + sh;
    int bc = 0;
#pragma unroll
    for (int e = 1; e < 4; ++e) {
        const float v = p[off[e]] * sc + sh;
        if (v > best) {
            best = v;
            bc = e;
        }
    }
    y[i] = best;
    if (code) code[i] = (uint8_t)bc;
}

}  // namespace

extern "C" int lidbox_conv2d_fwd(const float* x, int B, int T, int F, int C_in, const float* W, int k, int C_out,
                                 const float* bias, int relu, float* y, lidbox_stream_t stream) {
    if (int e = conv_check(__func__, B, T, F, C_in, C_out, k)) return e;
    LBX_ARG(x && W && y, "x, W, y != NULL");
    if (B == 0) return LIDBOX_OK;
    return launch_fwd(x, W, bias, relu ? 1 : 0, y, geom(B, T, F, C_in, C_out, k), (hipStream_t)stream);
}

extern "C" size_t lidbox_conv2d_dgrad_workspace(int k, int C_in, int C_out) {
    if (k < 1 || C_in < 1 || C_out < 1) return 0;
    return (size_t)k * k * C_in * C_out * sizeof(float);
}

extern "C" int lidbox_conv2d_dgrad(const float* dy, int B, int T, int F, int C_in, int C_out, const float* W, int k, float* dx,
                                   void* workspace, size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = conv_check(__func__, B, T, F, C_out, C_in, k)) return e;
    LBX_ARG(dy && W && dx, "dy, W, dx != NULL");
    if (B == 0) return LIDBOX_OK;
    LBX_ARG(workspace && workspace_bytes >= lidbox_conv2d_dgrad_workspace(k, C_in, C_out) && ((uintptr_t)workspace & 15) == 0,
            "workspace >= lidbox_conv2d_dgrad_workspace() bytes, 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* Wd = (float*)workspace;
    const long nw = (long)k * k * C_in * C_out;
    hipLaunchKernelGGL(conv_rot_kernel, wcopy_grid(nw), dim3(256), 0, st, W, Wd, k, C_in, C_out);
    LBX_LAUNCH_OK();
    return launch_fwd(dy, Wd, nullptr, 0, dx, geom(B, T, F, C_out, C_in, k), st);
}

extern "C" size_t lidbox_conv2d_wgrad_workspace(int B, int T, int F, int C_in, int C_out, int k) {
    if (B < 1 || T < 1 || F < 1 || C_in < 1 || C_out < 16 || C_out % 16 != 0 || k < 1) return 0;
    const ConvGeom g = geom(B, T, F, C_in, C_out, k);
    return wgrad_workspace_bytes(g.K, g.M, C_out);
}

extern "C" int lidbox_conv2d_wgrad(const float* x, const float* dy, int B, int T, int F, int C_in, int C_out, int k, float* dW,
                                   float* db, void* workspace, size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = conv_check(__func__, B, T, F, C_in, C_out, k)) return e;
    LBX_ARG(x && dy && dW, "x, dy, dW != NULL");
    hipStream_t st = (hipStream_t)stream;
    const ConvGeom g = geom(B, T, F, C_in, C_out, k);
    return run_wgrad(__func__, g.K, g.M, C_out, dW, db, workspace, workspace_bytes, st,
                     [&](auto BN, dim3 grid, float* part, float* dbpart, long per, int P) {
                         hipLaunchKernelGGL(conv_wgrad_kernel<BN()>, grid, dim3(256), 0, st, x, dy, part, dbpart, per, P, g);
                     });
}

extern "C" int lidbox_bn_maxpool2d_fwd(const float* x, int B, int T, int F, int C, const float* scale, const float* shift,
                                       float* y, unsigned char* argmax, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 2 && F >= 2 && C >= 1 && (long)B * T * F * C < (1L << 40), "B >= 0, T >= 2, F >= 2, C >= 1");
    LBX_ARG(x && scale && shift && y && argmax, "pointers != NULL");
    const long n = (long)B * (T / 2) * (F / 2) * C;
    if (n == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_maxpool_fwd_kernel, dim3((unsigned)lbx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, T, F, C,
                       scale, shift, y, argmax, n);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_maxpool2d_bwd(const float* dy, const unsigned char* argmax, int B, int T, int F, int C, float* dx,
                                    lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 2 && F >= 2 && C >= 1 && (long)B * T * F * C < (1L << 40), "B >= 0, T >= 2, F >= 2, C >= 1");
    LBX_ARG(dy && argmax && dx, "pointers != NULL");
    const long n = (long)B * T * F * C;
    if (n == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)lbx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, argmax, T, F,
                       C, dx, n);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" size_t lidbox_l2_penalty_workspace(void) { return L2_BLOCKS * sizeof(float); }

extern "C" int lidbox_l2_penalty(const float* params, float* grads, int count, const long* offsets, const long* sizes,
                                 const float* lambdas, float grad_scale, float* loss, void* workspace, size_t workspace_bytes,
                                 lidbox_stream_t stream) {
    LBX_ARG(params && count >= 0 && count <= L2_MAX && (count == 0 || (offsets && sizes && lambdas)),
            "params != NULL, 0 <= count <= 16, offsets / sizes / lambdas != NULL");
    LBX_ARG(!loss || (workspace && workspace_bytes >= lidbox_l2_penalty_workspace() && ((uintptr_t)workspace & 3) == 0),
            "workspace >= lidbox_l2_penalty_workspace() bytes when loss != NULL");
    if (count == 0 || (!grads && !loss)) return LIDBOX_OK;
    L2Args a{};
    long total = 0;
    for (int t = 0; t < count; ++t) {
        LBX_ARG(offsets[t] >= 0 && sizes[t] >= 0, "offsets, sizes >= 0");
        a.w[t] = params + offsets[t];
        a.g[t] = grads ? grads + offsets[t] : nullptr;
        a.n[t] = sizes[t];
        a.lam[t] = lambdas[t];
        total += sizes[t];
    }
    a.count = count;
    a.gscale = grad_scale;
    a.partial = loss ? (float*)workspace : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(l2_penalty_kernel, dim3(L2_BLOCKS), dim3(256), 0, st, a, lbx_cdiv(total, L2_BLOCKS));
    LBX_LAUNCH_OK();
    if (loss) {
        hipLaunchKernelGGL(l2_loss_kernel, dim3(1), dim3(64), 0, st, (const float*)workspace, loss);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

// ---------------------------------------------------------------------------------------------- strided Conv2D entry points
extern "C" int lidbox_conv2d_strided_fwd(const float* x, int B, int T, int F, int C_in, const float* W, lidbox_conv2d_taps_t taps,
                                         int C_out, const float* bias, float* y, lidbox_stream_t stream) {
    if (int e = sconv_check(__func__, B, T, F, C_in, C_out, taps)) return e;
    LBX_ARG(x && W && y, "x, W, y != NULL");
    if (B == 0) return LIDBOX_OK;
    return launch_sconv<false>(x, W, bias, y, sgeom(B, T, F, C_in, C_out, taps), (hipStream_t)stream);
}

extern "C" size_t lidbox_conv2d_strided_dgrad_workspace(lidbox_conv2d_taps_t taps, int C_in, int C_out) {
    if (taps.kt < 1 || taps.kf < 1 || C_in < 1 || C_out < 1) return 0;
    return (size_t)taps.kt * taps.kf * C_in * C_out * sizeof(float);
}

extern "C" int lidbox_conv2d_strided_dgrad(const float* dy, int B, int T, int F, int C_in, int C_out, const float* W,
                                           lidbox_conv2d_taps_t taps, float* dx, void* workspace, size_t workspace_bytes,
                                           lidbox_stream_t stream) {
    if (int e = sconv_check(__func__, B, T, F, C_in, C_out, taps)) return e;
    LBX_ARG(C_in % 16 == 0, "C_in a multiple of 16");
    LBX_ARG(dy && W && dx, "dy, W, dx != NULL");
    if (B == 0) return LIDBOX_OK;
    LBX_ARG(workspace && workspace_bytes >= lidbox_conv2d_strided_dgrad_workspace(taps, C_in, C_out) &&
                ((uintptr_t)workspace & 15) == 0,
            "workspace >= lidbox_conv2d_strided_dgrad_workspace() bytes, 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* Wt = (float*)workspace;
    const long nw = (long)taps.kt * taps.kf * C_in * C_out;
    hipLaunchKernelGGL(sconv_transpose_kernel, wcopy_grid(nw), dim3(256), 0, st, W, Wt, taps.kt * taps.kf, C_in, C_out);
    LBX_LAUNCH_OK();
    return launch_sconv<true>(dy, Wt, nullptr, dx, sgeom(B, T, F, C_in, C_out, taps), st);
}

extern "C" size_t lidbox_conv2d_strided_wgrad_workspace(int B, int T, int F, int C_in, int C_out, lidbox_conv2d_taps_t taps) {
    if (B < 1 || sconv_check(__func__, B, T, F, C_in, C_out, taps) != LIDBOX_OK) return 0;
    const SGeom g = sgeom(B, T, F, C_in, C_out, taps);
    return wgrad_workspace_bytes(g.K, (long)B * g.To * g.Fo, C_out);
}

extern "C" int lidbox_conv2d_strided_wgrad(const float* x, const float* dy, int B, int T, int F, int C_in, int C_out,
                                           lidbox_conv2d_taps_t taps, float* dW, float* db, void* workspace,
                                           size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = sconv_check(__func__, B, T, F, C_in, C_out, taps)) return e;
    LBX_ARG(x && dy && dW, "x, dy, dW != NULL");
    hipStream_t st = (hipStream_t)stream;
    const SGeom g = sgeom(B, T, F, C_in, C_out, taps);
    return run_wgrad(__func__, g.K, (long)B * g.To * g.Fo, C_out, dW, db, workspace, workspace_bytes, st,
                     [&](auto BN, dim3 grid, float* part, float* dbpart, long per, int P) {
                         hipLaunchKernelGGL(sconv_wgrad_kernel<BN()>, grid, dim3(256), 0, st, x, dy, part, dbpart, per, P, g);
                     });
}

extern "C" int lidbox_bn_relu_fwd(const float* x, long R, int C, const float* scale, const float* shift, float* y,
                                  lidbox_stream_t stream) {
    LBX_ARG(R >= 0 && C >= 1 && R * C < (1L << 40), "R >= 0, C >= 1");
    LBX_ARG(x && scale && shift && y, "pointers != NULL");
    if (R == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_relu_fwd_kernel, dim3(ew_blocks(R * C)), dim3(256), 0, (hipStream_t)stream, x, R * C, C, scale, shift, y);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_bn_relu_bwd(const float* x, long R, int C, const float* scale, const float* shift, const float* dy,
                                  float* dx, lidbox_stream_t stream) {
    LBX_ARG(R >= 0 && C >= 1 && R * C < (1L << 40), "R >= 0, C >= 1");
    LBX_ARG(x && scale && shift && dy && dx, "pointers != NULL");
    if (R == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_relu_bwd_kernel, dim3(ew_blocks(R * C)), dim3(256), 0, (hipStream_t)stream, x, R * C, C, scale, shift, dy,
                       dx);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_bn_relu_maxf_fwd(const float* x, int B, int T, int F, int C, const float* scale, const float* shift,
                                       float* y, long y_batch_stride, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 1 && F >= 1 && C >= 1 && (long)B * T * F * C < (1L << 40), "B >= 0, T, F, C >= 1");
    LBX_ARG(y_batch_stride >= (long)T * C, "y_batch_stride >= T * C");
    LBX_ARG(x && scale && shift && y, "pointers != NULL");
    const long n = (long)B * T * C;
    if (n == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_relu_maxf_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, T, F, C, scale, shift, y,
                       y_batch_stride, n);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_bn_relu_maxf_bwd(const float* x, int B, int T, int F, int C, const float* scale, const float* shift,
                                       const float* dy, long dy_batch_stride, float* dx, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 1 && F >= 1 && C >= 1 && (long)B * T * F * C < (1L << 40), "B >= 0, T, F, C >= 1");
    LBX_ARG(dy_batch_stride >= (long)T * C, "dy_batch_stride >= T * C");
    LBX_ARG(x && scale && shift && dy && dx, "pointers != NULL");
    const long n = (long)B * T * C;
    if (n == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_relu_maxf_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, T, F, C, scale, shift, dy,
                       dy_batch_stride, dx, n);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

// ---------------------------------------------------------------------------------------------- ragged forward entry points
extern "C" int lidbox_conv2d_ragged_fwd(const float* x, const long* row_offsets, int B, int total_T, int F, int C_in,
                                        const float* W, int k, int C_out, const float* bias, int relu, float* y,
                                        lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && total_T >= 0, "B >= 0, total_T >= 0");
    if (int e = conv_check(__func__, 1, total_T > 0 ? total_T : 1, F, C_in, C_out, k)) return e;
    LBX_ARG(x && row_offsets && W && y, "x, row_offsets, W, y != NULL");
    if (B == 0 || total_T == 0) return LIDBOX_OK;
    const ConvGeom g{B, total_T, F, C_in, C_out, k, (k - 1) / 2, (long)total_T * F, k * k * C_in};
    const int bn = conv_tile_n(C_out), r = relu ? 1 : 0;
    const dim3 grid((unsigned)lbx_cdiv(g.M, CV_BM), (unsigned)(C_out / bn));
    hipStream_t st = (hipStream_t)stream;
    with_tile_n(bn, [&](auto BN) {
        hipLaunchKernelGGL(conv_ragged_fwd_kernel<BN()>, grid, dim3(256), 0, st, x, row_offsets, W, bias, r, y, g);
    });
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_conv2d_strided_ragged_fwd(const float* x, const long* row_offsets, int B, int total_T, int F, int C_in,
                                                const float* W, lidbox_conv2d_taps_t taps, int C_out, const float* bias,
                                                float* y, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && total_T >= 0, "B >= 0, total_T >= 0");
    if (int e = sconv_check(__func__, 1, total_T > 0 ? total_T : 1, F, C_in, C_out, taps)) return e;
    LBX_ARG(taps.pt0 + taps.pt1 == taps.kt - 1, "a time geometry that keeps the length: pt0 + pt1 == kt - 1");
    LBX_ARG(x && row_offsets && W && y, "x, row_offsets, W, y != NULL");
    if (B == 0 || total_T == 0) return LIDBOX_OK;
    SGeom g = sgeom(1, total_T, F, C_in, C_out, taps);
    g.B = B;
    const int bn = conv_tile_n(C_out);
    const dim3 grid((unsigned)lbx_cdiv(total_T, CV_BM), (unsigned)g.Fo, (unsigned)(C_out / bn));
    hipStream_t st = (hipStream_t)stream;
    with_tile_n(bn, [&](auto BN) {
        hipLaunchKernelGGL(sconv_ragged_kernel<BN()>, grid, dim3(256), 0, st, x, row_offsets, W, bias, y, g);
    });
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_bn_maxpool2d_ragged_fwd(const float* x, const long* in_offsets, int B, int F, int C, const float* scale,
                                              const float* shift, float* y, const long* out_offsets, long total_out,
                                              unsigned char* argmax, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && F >= 2 && C >= 1 && total_out >= 0 && total_out < (1L << 31) && total_out * (F / 2) * C < (1L << 38),
            "B >= 0, F >= 2, C >= 1, total_out >= 0, sizes in range");
    LBX_ARG(x && in_offsets && scale && shift && y && out_offsets, "pointers != NULL (argmax may be)");
    const long n = total_out * (F / 2) * C;
    if (B == 0 || n == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(bn_maxpool_ragged_fwd_kernel, dim3((unsigned)lbx_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x,
                       in_offsets, B, F, C, scale, shift, y, out_offsets, argmax, n);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}
