// backend.hip -- the embedding back-end between the extractor and the report (gfx950).
//
// Replaces (reference file:line):
//   lidbox/embed/sklearn_utils.py:230-244  predict_with_trained_classifier: StandardScaler.transform -> PLDA.transform ->
//                                          sklearn.preprocessing.normalize -> GaussianNB.predict_log_proba -> max(., -100)
//   lidbox/embed/sklearn_utils.py:103-111  get_lda_scores (LinearDiscriminantAnalysis / PLDA log-probabilities)
//   lidbox/embed/sklearn_utils.py:179-196  fit_classifier: the centring passes of the fits
//
// lidbox_backend_score: one launch per block of 64 rows does the affine map u = (x - mu) P + q on the fp32 MFMA pipe
// (v_mfma_f32_16x16x4_f32), the row norm, the diagonal-Gaussian class scores and the log-softmax; only v and out go to HBM.
//   workgroup   4 waves, 64 rows; wave w owns rows 16w .. 16w+15 and all RP = 16 NT columns (NT accumulator tiles, NT a
//               template parameter so the accumulators stay in registers)
//   K loop      chunks of BK = 32: X tile [64][32] (mu subtracted on load; rows >= N and columns >= D are zeros, so the
//               contraction tail adds exact zeros) and P tile [32][RP] go global -> registers -> LDS, the next chunk's
//               global loads are issued before the current chunk's MFMAs.  Xs rows are BK + 4 floats apart and Ps rows
//               PS = 16 (mod 64) floats apart: both operand reads are bank-conflict free.
//   after it    the staging area is dead and is overlaid by the u tile, per wave [RP][16 rows] (a row's 16 values of one
//               column are one 64-byte run: the class stage reads them as four broadcast ds_read_b128)
//   class stage lane = class (c = lane + 64 i, i < 4), all 16 rows of the wave at once, the difference form
//               (v - theta)^2 w summed over r in order; then max / sum butterflies over the lanes per row.
// Every sum has a fixed order that depends on (D, R, K) only, and a row never meets another row's data: a row's outputs are
// bit-identical whatever N, its position or the run.  No atomics.
// Roofline: N D 4 bytes of x once from HBM; 2 N D RP flop on the MFMA pipe + 3 N K R on the VALU.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int BM = 64, BK = 32, XS = BK + 4;

__host__ __device__ constexpr int ps_stride(int RP) { return RP + ((16 - RP % 64) + 64) % 64; }
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }

struct ScoreArgs {
    const float* x;
    long ldx, N;
    int D, R, K;
    const float *mu, *P, *q, *theta, *w, *c0;
    float* v;
    long ldv;
    float* out;
    long ldo;
    int flags, xvec;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));

// four consecutive elements k .. k+3 of row `row` of x - mu (zeros outside [0, N) x [0, D))
__device__ __forceinline__ void load_x4(const ScoreArgs& a, long row, int k, float (&o)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = 0.f;
    if (row >= a.N || k >= a.D) return;
    const float* p = a.x + row * a.ldx + k;
    if (a.xvec && k + 4 <= a.D) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        o[0] = t.x, o[1] = t.y, o[2] = t.z, o[3] = t.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < a.D) o[e] = p[e];
    }
    if (a.mu) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < a.D) o[e] -= a.mu[k + e];
    }
}

template <int NT>
__global__ __launch_bounds__(256) void backend_score_kernel(const ScoreArgs a) {
    constexpr int RP = 16 * NT, PS = ps_stride(RP);
    constexpr int STAGE = BM * XS + BK * PS, UT = 4 * RP * 16;
    __shared__ __attribute__((aligned(16))) float smem[imax(STAGE, UT)];
    float* Xs = smem;
    float* Ps = smem + BM * XS;

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int lc = lane & 15, lg = lane >> 4;
    const long row0 = (long)blockIdx.x * BM;
    const int R = a.R, D = a.D;

    // staging maps: X: float4 column xk of rows xr and xr + 32; P: elements t + 256 i of the [BK][RP] tile
    const int xk = (t & 7) * 4, xr = t >> 3;
    float xreg[2][4], preg[2 * NT];
    auto load_chunk = [&](int k0) {
        load_x4(a, row0 + xr, k0 + xk, xreg[0]);
        load_x4(a, row0 + xr + 32, k0 + xk, xreg[1]);
#pragma unroll
        for (int i = 0; i < 2 * NT; ++i) {
            const int idx = t + 256 * i, k = idx / RP, r = idx % RP;
            preg[i] = (k0 + k < D && r < R) ? a.P[(long)(k0 + k) * R + r] : 0.f;
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h)
            *reinterpret_cast<float4*>(Xs + (xr + 32 * h) * XS + xk) = make_float4(xreg[h][0], xreg[h][1], xreg[h][2], xreg[h][3]);
#pragma unroll
        for (int i = 0; i < 2 * NT; ++i) {
            const int idx = t + 256 * i;
            Ps[(idx / RP) * PS + idx % RP] = preg[i];
        }
    };

    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_chunk(0);
    for (int k0 = 0; k0 < D; k0 += BK) {
        store_chunk();
        __syncthreads();
        if (k0 + BK < D) load_chunk(k0 + BK);
        const float* xa = Xs + (wv * 16 + lc) * XS + lg;
        const float* pb = Ps + lg * PS + lc;
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            const float av = xa[kk * 4];
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, pb[kk * 4 * PS + 16 * j], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }

    // lane holds u[row 4 lg + e][column 16 j + lc], e = 0..3
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int r = 16 * j + lc;
        const float qv = (a.q && r < R) ? a.q[r] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[j][e] += qv;
            ss[e] = fmaf(acc[j][e], acc[j][e], ss[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) ss[e] += __shfl_xor(ss[e], o, 64);      // commutative butterfly: every lane the same sum
    }
    float* Uw = smem + wv * (RP * 16);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // a NaN or Inf in the row (or a norm that overflows fp32) poisons the whole row, whatever the flags
        const bool bad = !(ss[e] < INFINITY);
        const float nrm = (a.flags & LIDBOX_BACKEND_L2) && ss[e] > 0.f ? sqrtf(ss[e]) : 1.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j][e] = bad ? __builtin_nanf("") : acc[j][e] / nrm;
    }
    const long wrow = row0 + wv * 16 + lg * 4;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int r = 16 * j + lc;
        if (a.v && r < R) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (wrow + e < a.N) a.v[(wrow + e) * a.ldv + r] = acc[j][e];
        }
        *reinterpret_cast<f32x4*>(Uw + r * 16 + lg * 4) = acc[j];
    }
    if (!a.out) return;
    wave_lds_sync();

    const int K = a.K;
    const bool linear = a.flags & LIDBOX_BACKEND_LINEAR;
    float s[4][16];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
        if (ci * 64 >= K) break;
        const int c = min(ci * 64 + lane, K - 1);
        if (linear) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 u4 = *reinterpret_cast<const f32x4*>(Uw + c * 16 + g * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[ci][g * 4 + e] = u4[e];
            }
        } else {
            const float* th = a.theta + (long)c * R;
            const float* ww = a.w + (long)c * R;
            float d2[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) d2[i] = 0.f;
            for (int r = 0; r < R; ++r) {
                const float tv = th[r], wr = ww[r];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 u4 = *reinterpret_cast<const f32x4*>(Uw + r * 16 + g * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float d = u4[e] - tv;
                        d2[g * 4 + e] = fmaf(d * d, wr, d2[g * 4 + e]);
                    }
                }
            }
            const float cc = a.c0[c];
#pragma unroll
            for (int i = 0; i < 16; ++i) s[ci][i] = cc - 0.5f * d2[i];
        }
    }
    const bool normalised = a.flags & LIDBOX_BACKEND_NORMALISED;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float lse = 0.f;
        if (normalised) {
            // fmaxf drops a NaN, the sum does not: a NaN score makes the row's lse, and so its whole output, NaN
            float m = -INFINITY;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
                if (ci * 64 < K && ci * 64 + lane < K) m = fmaxf(m, s[ci][i]);
            m = wave_max(m);
            float z = 0.f;
#pragma unroll
            for (int ci = 0; ci < 4; ++ci)
                if (ci * 64 < K && ci * 64 + lane < K) z += expf(s[ci][i] - m);
            z = wave_sum(z);
            lse = m + logf(z);
        }
        const long row = row0 + wv * 16 + i;
        if (row >= a.N) continue;
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int c = ci * 64 + lane;
            if (ci * 64 < K && c < K) {
                float o = s[ci][i];
                if (normalised) {
                    o -= lse;
                    o = o < -100.f ? -100.f : o;         // keeps a NaN (fmaxf would not)
                }
                a.out[row * a.ldo + c] = o;
            }
        }
    }
}

// one step of center_rows on four columns: OP 0 subtracts, OP 1 multiplies.  Each step rounds once (__fsub_rn / __fmul_rn are
// never contracted into an FMA), so the 16-byte and the scalar path, and any host restatement in fp32, give the same bits.
template <int OP>
__device__ __forceinline__ void center_step(float (&v)[4], const float4 t) {
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = OP == 0 ? __fsub_rn(v[e], tv[e]) : __fmul_rn(v[e], tv[e]);
}

// out[i, :] = (x[i, :] - mu) * inv_scale - cm[seg(i), :], squared when `square`; one wave per row at a time
template <bool VEC>
__global__ __launch_bounds__(256) void backend_center_rows_kernel(const float* __restrict__ x, long N, int D, long ldx,
                                                                  const float* __restrict__ mu, const float* __restrict__ inv_scale,
                                                                  const float* __restrict__ cm, const int64_t* __restrict__ seg,
                                                                  int nseg, int square, float* __restrict__ out, long ldo) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
    for (long i = wave; i < N; i += nwaves) {
        const float* m = nullptr;
        if (cm) {
            int lo = 0, hi = nseg;                       // largest s with seg[s] <= i
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (seg[mid] <= i) lo = mid; else hi = mid;
            }
            m = cm + (long)lo * D;
        }
        const float* xi = x + i * ldx;
        float* oi = out + i * ldo;
        if (VEC) {
            for (int d = lane * 4; d < D; d += 256) {
                const float4 xv = *reinterpret_cast<const float4*>(xi + d);
                float v[4] = {xv.x, xv.y, xv.z, xv.w};
                if (mu) { const float4 t = *reinterpret_cast<const float4*>(mu + d); center_step<0>(v, t); }
                if (inv_scale) { const float4 t = *reinterpret_cast<const float4*>(inv_scale + d); center_step<1>(v, t); }
                if (m) { const float4 t = *reinterpret_cast<const float4*>(m + d); center_step<0>(v, t); }
                if (square) center_step<1>(v, make_float4(v[0], v[1], v[2], v[3]));
                *reinterpret_cast<float4*>(oi + d) = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int d = lane; d < D; d += 64) {
                float v = xi[d];
                if (mu) v = __fsub_rn(v, mu[d]);
                if (inv_scale) v = __fmul_rn(v, inv_scale[d]);
                if (m) v = __fsub_rn(v, m[d]);
                if (square) v = __fmul_rn(v, v);
                oi[d] = v;
            }
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int NT>
void launch_score(const ScoreArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(backend_score_kernel<NT>, dim3((unsigned)lbx_cdiv(a.N, BM)), dim3(256), 0, st, a);
}

}  // namespace

extern "C" int lidbox_backend_score(const float* x, long N, int D, long ldx, const float* mu, const float* P, const float* q,
                                    int R, const float* theta, const float* w, const float* c0, int K, int flags, float* v,
                                    long ldv, float* out, long ldo, lidbox_stream_t stream) {
    LBX_ARG(N >= 0 && N <= LIDBOX_BACKEND_MAX_ROWS, "N must be 0 .. LIDBOX_BACKEND_MAX_ROWS per call");
    LBX_ARG(D >= 1 && D <= 4096, "D must be 1 .. 4096");
    LBX_ARG(R >= 1 && R <= 255, "R must be 1 .. 255");
    LBX_ARG((flags & ~(LIDBOX_BACKEND_L2 | LIDBOX_BACKEND_NORMALISED | LIDBOX_BACKEND_LINEAR)) == 0, "unknown flag");
    const bool linear = flags & LIDBOX_BACKEND_LINEAR;
    if (linear) {
        LBX_ARG(!theta && !w && !c0, "LIDBOX_BACKEND_LINEAR takes no theta / w / c0");
        LBX_ARG(out != nullptr, "LIDBOX_BACKEND_LINEAR needs out");
        LBX_ARG(K == R, "LIDBOX_BACKEND_LINEAR needs K == R");
    } else if (theta) {
        LBX_ARG(w && c0, "theta without w / c0");
        LBX_ARG(out != nullptr, "class parameters without out");
    } else {
        LBX_ARG(!w && !c0, "w / c0 without theta");
        out = nullptr;                                    // transform only
    }
    if (out) {
        LBX_ARG(K >= 1 && K <= 256, "K must be 1 .. 256");
        LBX_ARG(ldo >= K, "ldo < K");
    }
    LBX_ARG(v || out, "nothing to write: v is NULL and there is no class stage");
    LBX_ARG(!v || ldv >= R, "ldv < R");
    LBX_ARG(ldx >= D, "ldx < D");
    if (N == 0) return LIDBOX_OK;
    LBX_ARG(x && P, "x / P is NULL");
    ScoreArgs a{x, ldx, N, D, R, out ? K : 0, mu, P, q, theta, w, c0, v, ldv, out, ldo, flags, al16(x) && ldx % 4 == 0};
    hipStream_t st = (hipStream_t)stream;
    switch ((R + 15) / 16) {
#define LBX_CASE(n) case n: launch_score<n>(a, st); break;
        LBX_CASE(1) LBX_CASE(2) LBX_CASE(3) LBX_CASE(4) LBX_CASE(5) LBX_CASE(6) LBX_CASE(7) LBX_CASE(8)
        LBX_CASE(9) LBX_CASE(10) LBX_CASE(11) LBX_CASE(12) LBX_CASE(13) LBX_CASE(14) LBX_CASE(15) LBX_CASE(16)
#undef LBX_CASE
    }
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_backend_center_rows(const float* x, long N, int D, long ldx, const float* mu, const float* inv_scale,
                                          const float* cm, const int64_t* segment_offsets, int num_segments, int square,
                                          float* out, long ldo, lidbox_stream_t stream) {
    LBX_ARG(N >= 0 && D >= 1, "N < 0 or D < 1");
    LBX_ARG(ldx >= D && ldo >= D, "row stride < D");
    LBX_ARG(!cm || (segment_offsets && num_segments >= 1), "cm without segment offsets");
    if (N == 0) return LIDBOX_OK;
    LBX_ARG(x && out, "x / out is NULL");
    const bool vec = D % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out) && al16(mu) && al16(inv_scale) && al16(cm);
    const unsigned grid = (unsigned)(lbx_cdiv(N, 4) < 16384 ? lbx_cdiv(N, 4) : 16384);
    hipStream_t st = (hipStream_t)stream;
    if (vec)
        hipLaunchKernelGGL(backend_center_rows_kernel<true>, dim3(grid), dim3(256), 0, st, x, N, D, ldx, mu, inv_scale, cm,
                           segment_offsets, num_segments, square, out, ldo);
    else
        hipLaunchKernelGGL(backend_center_rows_kernel<false>, dim3(grid), dim3(256), 0, st, x, N, D, ldx, mu, inv_scale, cm,
                           segment_offsets, num_segments, square, out, ldo);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}
