// gru.hip -- the Keras GRU layer's recurrence (TF2 defaults), gfx950.
//
// Replaces (reference file:line): tf.keras.layers.GRU as lidbox/models/bi_gru.py:33-34 builds it inside
// Bidirectional(merge_mode="concat") (reset_after=True, activation tanh, recurrent_activation sigmoid, use_bias, zero
// initial state, no dropout, no masking).
//
// Gate order in the 3H columns is z, r, h; bias [2][3H] = (input bias, recurrent bias).  One step:
//     x_z, x_r, x_h = x_t W + b_in           (the caller's GEMM: lidbox_gemm_nn, LIDBOX_EPI_BIAS, over all B*T rows)
//     q = h_{t-1} U + b_rec;  z = sig(x_z + q_z);  r = sig(x_r + q_r);  hh = tanh(x_h + r q_h);  h_t = z h_{t-1} + (1 - z) hh
// The weight gradients and dX are the caller's GEMMs too (dW = X^T dZx, dU = H_prev^T dZrec, dX = dZx W^T); this file holds
// only what walks through time.
//
// Buffers (all fp32, see lidbox_hip.h):
//     zg    [dirs][B][T][3H]   forward: X W + b_in in, (z, r, hh) out; backward: those in, dZx = (dz, dr, dhh) out
//     qh    [dirs][B][T][H]    forward: q_h (with its bias) out; backward: the h block of dZrec, dhh * r, out
//     hseq  [B][T+2][dirs*H]   h_t of direction d at row t+1; rows 0 and T+1 stay zero (as in rnn.hip)
//     carry [dirs][B][H]       backward's direct term z_{t+1} dh_{t+1} (workspace)
//
// One form, any H: one launch per time step covers both directions.  Grid = ceil(B / 64) row tiles x ceil(H / 16) unit
// slices x dirs; a workgroup is 4 waves, wave w owns rows 16w..16w+15 of its tile.  All three gates of unit j read only
// columns j, H+j and 2H+j of U, so a workgroup computes h_{t-1}[rows, :] U[:, {z, r, h} columns of its 16 units] with
// v_mfma_f32_16x16x4_f32 (exact fp32) into three accumulators whose (row, unit) positions coincide in every lane, and
// applies the cell in the same kernel.  Forward stages U's 48 columns of the slice into LDS in 256-row chunks; backward
// computes dh_rec = dZrec_{t+1} U^T for its units (K = 3H), staging U's 16 rows of the slice in 768-column chunks.  The
// A operand (h_{t-1} or dZrec_{t+1} rows) streams from global memory: lane (c, g) = (l & 15, l >> 4) loads row c, k =
// k0 + 8g .. k0 + 8g + 7, and MFMA e of the k0 block consumes element e -- a fixed permutation of the k order.
//
// No inter-workgroup communication, no atomics, no spin-waits: steps are ordered by the stream alone.  Every output element
// is one MFMA k-chain over its own row, in an order that depends on neither B nor the row's place in the batch, so a
// row's results are bit-identical whatever the batch.
#include <math.h>

#include "common.h"

// No a*b+c is contracted behind the source's back (as in rnn.hip): the cell is evaluated exactly as written.
#pragma clang fp contract(off)

namespace {

constexpr int GRU_ROWS = 64;     // batch rows per workgroup: 4 waves x 16
constexpr int GRU_UNITS = 16;    // hidden units per workgroup: 48 columns of U forward, 16 rows of U backward
constexpr int GRU_KCF = 256;     // forward: rows of U per LDS chunk (256 x 50 floats = 50 KiB)
constexpr int GRU_KCB = 768;     // backward: columns of U per LDS chunk (768 x 18 floats = 54 KiB)
// LDS row strides: 8 * ld = 16 (mod 64 banks), so the four k groups of a wave (rows k, k+8, k+16, k+24) hit disjoint banks
constexpr int GRU_LDF = 50;
constexpr int GRU_LDB = 18;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

struct GruArgs {
    const float* U[2];
    const float* brec[2];
    float* zg;
    float* hseq;
    float* qh;
    float* hlast;
    const float* dh_seq;
    long dh_bs;
    const float* dh_last;
    float* carry;
    int B, T, H, dirs;
};

// this lane's A values k .. k+7 of a chunk (zeros past klen or for a row past B)
template <bool VEC>
__device__ __forceinline__ void load_a(float (&av)[8], const float* __restrict__ arow, bool aok, int k, int klen) {
    if (VEC) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (aok && k < klen) v0 = *reinterpret_cast<const float4*>(arow + k);
        if (aok && k + 4 < klen) v1 = *reinterpret_cast<const float4*>(arow + k + 4);
        av[0] = v0.x; av[1] = v0.y; av[2] = v0.z; av[3] = v0.w;
        av[4] = v1.x; av[5] = v1.y; av[6] = v1.z; av[7] = v1.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = aok && k + e < klen ? arow[k + e] : 0.0f;
    }
}

// acc[g] += A[16 rows of this wave][kc .. kc+klen) . Bs[k][16 g + c].  arow: this lane's A row at the chunk start (row
// l & 15 of the wave; aok false: a row past B, which contributes zeros).  Bs holds kpad = klen rounded up to 32 rows, zero
// past klen.  VEC: klen % 4 == 0 and arow 16-byte aligned.  The next block's A values are loaded before this block's MFMAs.
template <int NG, bool VEC>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[NG], const float* __restrict__ arow, bool aok, int klen, int kpad,
                                          const float* Bs, int ldb, int lane) {
    const int c = lane & 15, kg = lane >> 4;
    float av[8], an[8];
    load_a<VEC>(an, arow, aok, 8 * kg, klen);
    for (int k0 = 0; k0 < kpad; k0 += 32) {
        const int k = k0 + 8 * kg;
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = an[e];
        if (k0 + 32 < kpad) load_a<VEC>(an, arow, aok, k + 32, klen);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float* br = Bs + (k + e) * ldb + c;
#pragma unroll
            for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], br[g * 16], acc[g], 0, 0, 0);
        }
    }
}

// LDS staging of n items by the workgroup's 256 threads: GRU_STAGE_BATCH loads in flight per thread before their stores
// (a load-store loop would wait out one memory latency per item)
constexpr int GRU_STAGE_BATCH = 12;

template <typename V, typename Load, typename Store>
__device__ __forceinline__ void stage(int n, Load load, Store store) {
    for (int base = threadIdx.x; base < n; base += 256 * GRU_STAGE_BATCH) {
        V v[GRU_STAGE_BATCH];
#pragma unroll
        for (int j = 0; j < GRU_STAGE_BATCH; ++j) {
            const int i = base + 256 * j;
            if (i < n) v[j] = load(i);
        }
#pragma unroll
        for (int j = 0; j < GRU_STAGE_BATCH; ++j) {
            const int i = base + 256 * j;
            if (i < n) store(i, v[j]);
        }
    }
}

// forward chunk: Bs[kk][16 g + c] = U[kc + kk][g H + u0 + c] (zero past klen / H); float4 loads along the units when VEC
template <bool VEC>
__device__ __forceinline__ void stage_fwd(float* Bs, const float* __restrict__ U, int H, int u0, int kc, int klen, int kpad) {
    const size_t H3 = 3 * (size_t)H;
    if (VEC) {
        stage<float4>(kpad * 12, [&](int e) {
            const int kk = e / 12, q = e - kk * 12, u = u0 + 4 * (q & 3);
            return kk < klen && u < H ? *reinterpret_cast<const float4*>(U + (kc + kk) * H3 + (q >> 2) * H + u)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            const int kk = e / 12, q = e - kk * 12;
            float* d = Bs + kk * GRU_LDF + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        });
    } else {
        stage<float>(kpad * 48, [&](int e) {
            const int kk = e / 48, j = e - kk * 48, u = u0 + (j & 15);
            return kk < klen && u < H ? U[(kc + kk) * H3 + (j >> 4) * H + u] : 0.0f;
        }, [&](int e, float v) {
            const int kk = e / 48, j = e - kk * 48;
            Bs[kk * GRU_LDF + j] = v;
        });
    }
}

// backward chunk of gate block q: Bs[kk][c] = U[u0 + c][q H + kc + kk] (zero past klen / H); float4 loads along k when VEC
template <bool VEC>
__device__ __forceinline__ void stage_bwd(float* Bs, const float* __restrict__ U, int H, int u0, int q, int kc, int klen,
                                          int kpad) {
    const size_t H3 = 3 * (size_t)H;
    if (VEC) {
        const int k4n = kpad / 4;
        stage<float4>(16 * k4n, [&](int e) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n), u = u0 + c;
            return k4 < klen && u < H ? *reinterpret_cast<const float4*>(U + u * H3 + q * H + kc + k4)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n);
            float* d = Bs + k4 * GRU_LDB + c;
            d[0] = v.x; d[GRU_LDB] = v.y; d[2 * GRU_LDB] = v.z; d[3 * GRU_LDB] = v.w;
        });
    } else {
        stage<float>(16 * kpad, [&](int e) {
            const int c = e / kpad, kk = e - c * kpad, u = u0 + c;
            return kk < klen && u < H ? U[u * H3 + q * H + kc + kk] : 0.0f;
        }, [&](int e, float v) {
            const int c = e / kpad, kk = e - c * kpad;
            Bs[kk * GRU_LDB + c] = v;
        });
    }
}

// one forward step s of both directions (direction d: t = s forward, T-1-s reverse)
template <bool VEC>
__global__ __launch_bounds__(256) void gru_fwd_step_kernel(const GruArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[GRU_KCF * GRU_LDF];
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H3 = 3 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * GRU_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int prow = d == 0 ? t : t + 2;                      // hseq row of h_{t-1} (forward) / h_{t+1} (reverse)
    const int rb = blockIdx.x * GRU_ROWS + w * 16;
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ra = rb + (lane & 15);
        const bool aok = ra < B;
        const float* arow = a.hseq + ((size_t)(aok ? ra : 0) * (T + 2) + prow) * ldo + d * H;
        const float* U = a.U[d];
        for (int kc = 0; kc < H; kc += GRU_KCF) {
            const int klen = min(GRU_KCF, H - kc), kpad = (klen + 31) & ~31;
            __syncthreads();                                  // the previous chunk's LDS reads are done
            stage_fwd<VEC>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<3, VEC>(acc, arow + kc, aok, klen, kpad, Bs, GRU_LDF, lane);
        }
    }
    // epilogue: lane (c, g) holds unit u0 + c of rows rb + 4g + i (the 16x16 C/D map: col = lane & 15, row = 4 (lane >> 4) + i)
    const int u = u0 + (lane & 15);
    if (u >= H) return;
    const float* br = a.brec[d];
    const float bz = br[u], brr = br[H + u], bh = br[2 * H + u];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        if (b >= B) continue;
        const size_t row = ((size_t)d * B + b) * T + t;
        float* gz = a.zg + row * H3 + u;
        const float qz = acc[0][i] + bz, qr = acc[1][i] + brr, qhv = acc[2][i] + bh;
        const float z = sigm(gz[0] + qz), r = sigm(gz[H] + qr);
        const float hh = tanhf(gz[2 * H] + r * qhv);
        const float hp = s > 0 ? a.hseq[((size_t)b * (T + 2) + prow) * ldo + d * H + u] : 0.0f;
        const float h = z * hp + (1.0f - z) * hh;
        gz[0] = z;
        gz[H] = r;
        gz[2 * H] = hh;
        a.qh[row * H + u] = qhv;
        a.hseq[((size_t)b * (T + 2) + t + 1) * ldo + d * H + u] = h;
        if (a.hlast && s == T - 1) a.hlast[(size_t)b * ldo + d * H + u] = h;
    }
}

// one backward step s (walked from T-1 down): dh_t = incoming + dZrec_{t+1} U^T + z_{t+1} dh_{t+1}, then the cell backward
template <bool VEC>
__global__ __launch_bounds__(256) void gru_bwd_step_kernel(const GruArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[GRU_KCB * GRU_LDB];
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H3 = 3 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * GRU_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int prow = d == 0 ? t : t + 2;
    const int rb = blockIdx.x * GRU_ROWS + w * 16;
    f32x4 acc[1];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s < T - 1) {                                          // the direction's last step has no later step
        const int tn = d == 0 ? t + 1 : t - 1;
        const int ra = rb + (lane & 15);
        const bool aok = ra < B;
        const size_t nrow = ((size_t)d * B + (aok ? ra : 0)) * T + tn;
        const float* U = a.U[d];
        for (int q = 0; q < 3; ++q) {                         // dZrec = (dz, dr) from zg, dhh * r from qh
            const float* arow = q < 2 ? a.zg + nrow * H3 + q * H : a.qh + nrow * H;
            for (int kc = 0; kc < H; kc += GRU_KCB) {
                const int klen = min(GRU_KCB, H - kc), kpad = (klen + 31) & ~31;
                __syncthreads();
                stage_bwd<VEC>(Bs, U, H, u0, q, kc, klen, kpad);
                __syncthreads();
                mma_chunk<1, VEC>(acc, arow + kc, aok, klen, kpad, Bs, GRU_LDB, lane);
            }
        }
    }
    const int u = u0 + (lane & 15);
    if (u >= H) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        if (b >= B) continue;
        const size_t row = ((size_t)d * B + b) * T + t;
        float* gz = a.zg + row * H3 + u;
        float* cy = a.carry + ((size_t)d * B + b) * H + u;
        float dh = acc[0][i];
        if (a.dh_seq) dh += a.dh_seq[(size_t)b * a.dh_bs + (size_t)t * ldo + d * H + u];
        if (a.dh_last && s == T - 1) dh += a.dh_last[(size_t)b * ldo + d * H + u];
        if (s < T - 1) dh += *cy;
        const float z = gz[0], r = gz[H], hh = gz[2 * H];
        const float qhv = a.qh[row * H + u];
        const float hp = s > 0 ? a.hseq[((size_t)b * (T + 2) + prow) * ldo + d * H + u] : 0.0f;
        const float dz = dh * (hp - hh) * z * (1.0f - z);
        const float dhh = dh * (1.0f - z) * (1.0f - hh * hh);
        const float dr = dhh * qhv * r * (1.0f - r);
        gz[0] = dz;
        gz[H] = dr;
        gz[2 * H] = dhh;
        a.qh[row * H + u] = dhh * r;
        *cy = dh * z;
    }
}

int check_common(const char* fn, const float* U0, const float* U1, int dirs, int B, int T, int H) {
    if (!(dirs == 1 || dirs == 2) || !U0 || (dirs == 2 && !U1) || B < 0 || T < 1 || H < 1) {
        lidbox_set_error("%s: invalid argument: dirs in {1, 2}, U0 (and U1 when dirs == 2) != NULL, B >= 0, T >= 1, H >= 1", fn);
        return LIDBOX_E_INVALID;
    }
    if (H > 65535 || (long)B * T * 3 * H > (1L << 40)) {
        lidbox_set_error("%s: invalid argument: H <= 65535, B * T * 3H <= 2^40", fn);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

// float4 operand loads: H % 4 == 0 and 16-byte aligned buffers (then every row and chunk start is aligned too)
inline bool vec_ok(int H, const void* U0, const void* U1, const void* zg, const void* hseq, const void* qh) {
    return H % 4 == 0 && (((uintptr_t)U0 | (uintptr_t)U1 | (uintptr_t)zg | (uintptr_t)hseq | (uintptr_t)qh) & 15) == 0;
}

inline dim3 step_grid(int B, int H, int dirs) {
    return dim3((unsigned)lbx_cdiv(B, GRU_ROWS), (unsigned)lbx_cdiv(H, GRU_UNITS), (unsigned)dirs);
}

}  // namespace

extern "C" size_t lidbox_gru_workspace(int B, int T, int H, int dirs) {
    if (B <= 0 || T < 1 || H < 1 || dirs < 1 || dirs > 2) return 0;
    return (size_t)dirs * B * H * sizeof(float);
}

extern "C" int lidbox_gru_fwd(const float* U0, const float* U1, const float* b_rec0, const float* b_rec1, int dirs, int B,
                              int T, int H, float* zg, float* hseq, float* qh, float* hlast, lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(b_rec0 && (dirs == 1 || b_rec1) && zg && hseq && qh, "b_rec0 (and b_rec1 when dirs == 2), zg, hseq, qh != NULL");
    if (B == 0) return LIDBOX_OK;
    GruArgs a{{U0, dirs == 2 ? U1 : U0}, {b_rec0, dirs == 2 ? b_rec1 : b_rec0}, zg, hseq, qh, hlast, nullptr, 0, nullptr,
              nullptr, B, T, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = step_grid(B, H, dirs);
    const bool vec = vec_ok(H, a.U[0], a.U[1], zg, hseq, qh);
    for (int s = 0; s < T; ++s) {
        if (vec)
            hipLaunchKernelGGL(gru_fwd_step_kernel<true>, grid, dim3(256), 0, st, a, s);
        else
            hipLaunchKernelGGL(gru_fwd_step_kernel<false>, grid, dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_gru_bwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, const float* hseq,
                              float* qh, const float* dh_seq, long dh_batch_stride, const float* dh_last, void* workspace,
                              size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && hseq && qh && (dh_seq || dh_last), "zg, hseq, qh != NULL; dh_seq or dh_last != NULL");
    LBX_ARG(!dh_seq || dh_batch_stride >= (long)T * dirs * H, "dh_batch_stride >= T * dirs * H");
    if (B == 0) return LIDBOX_OK;
    LBX_ARG(workspace && workspace_bytes >= lidbox_gru_workspace(B, T, H, dirs), "workspace >= lidbox_gru_workspace() bytes");
    GruArgs a{{U0, dirs == 2 ? U1 : U0}, {nullptr, nullptr}, zg, const_cast<float*>(hseq), qh, nullptr, dh_seq,
              dh_batch_stride, dh_last, (float*)workspace, B, T, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = step_grid(B, H, dirs);
    const bool vec = vec_ok(H, a.U[0], a.U[1], zg, hseq, qh);
    for (int s = T - 1; s >= 0; --s) {
        if (vec)
            hipLaunchKernelGGL(gru_bwd_step_kernel<true>, grid, dim3(256), 0, st, a, s);
        else
            hipLaunchKernelGGL(gru_bwd_step_kernel<false>, grid, dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}
