// lstm_step.hip -- the Keras LSTM layer's recurrence as one fused launch per time step, gfx950.
//
// Replaces (reference file:line): tf.keras.layers.LSTM(250, return_sequences=True) inside Bidirectional(merge_mode=
// "concat") as lidbox/models/spherespeaker.py:39-41 stacks it three times.  H = 250 is past rnn.hip's resident form (U must
// fit in LDS), whose stepped form spends two GEMM launches and a cell launch per step.  Same math, buffers and gate order
// (i, f, c, o) as rnn.hip; same structure as gru.hip.
//
// One step:  z = x_t W + b + h_{t-1} U,  c_t = sig(z_f) c_{t-1} + sig(z_i) tanh(z_c),  h_t = sig(z_o) tanh(c_t).
// X W + b of all B*T rows, the weight gradients and dX are the caller's GEMMs; this file holds only what walks through time.
//
// Buffers (all fp32, see lidbox_hip.h):
//     zg    [dirs][B][T][4H]          forward: X W + b in, (i, f, tanh z_c, o) out; backward: those in, dZ out
//     hseq  [B][T+2][h_row_stride]    h_t of direction d at row t+1, columns d*H.. of the pointer passed; rows 0 and T+1 zero
//     cseq  [dirs][B][T][H]           cell states
//     carry [dirs][B][H]              backward's carried dc (workspace)
// The row strides of hseq and dh_seq are arguments, so a layer can live in a column slice of a wider buffer.
//
// One form, any H: one launch per time step covers both directions.  Grid = ceil(B / 64) row tiles x ceil(H / 16) unit
// slices x dirs; a workgroup is 4 waves, wave w owns rows 16w..16w+15 of its tile.  The four gates of unit j read only
// columns j, H+j, 2H+j and 3H+j of U, so a workgroup computes h_{t-1}[rows, :] U[:, 4 x 16 columns of its units] with
// v_mfma_f32_16x16x4_f32 (exact fp32) into four accumulators whose (row, unit) positions coincide in every lane, and
// applies the cell in the same kernel.  Forward stages U's 64 columns of the slice into LDS in 256-row chunks.  Backward
// computes dh_rec = dZ_{t+1} U^T for its units: K = 4H runs over one contiguous row of dZ and of U, staged 16 rows of U x
// 1024 columns at a time.  The A operand (h_{t-1} or dZ_{t+1} rows) streams from global memory: lane (c, g) = (l & 15,
// l >> 4) loads row c, k = k0 + 8g .. k0 + 8g + 7, and MFMA e of the k0 block consumes element e -- a fixed permutation of
// the k order, the same for the 16-, 8- and 4-byte load paths.  Four 32-k blocks of A are fetched per trip to L2, the first
// trip and the cell's own operands (zg's slice, c, dh, dc) ahead of the product, whose latency then covers theirs.
//
// Load paths of forward (A rows start at column d*H of a row h_row_stride wide, U's gate blocks at multiples of H): float4
// when H % 4 == 0, float2 when H is even (H = 250, the model's own width), scalar otherwise; each also needs the row
// stride to be a multiple of its width and the pointers aligned to it.  Backward's K axis is 4H long and both operands'
// rows are 4H floats apart, so its float4 path needs only 16-byte aligned pointers.
//
// No inter-workgroup communication, no atomics, no spin-waits: steps are ordered by the stream alone.  Every output element
// is one MFMA k-chain over its own row, in an order that depends on neither B nor the row's place in the batch, so a
// row's results are bit-identical whatever the batch.
#include <math.h>

#include "common.h"

// No a*b+c is contracted behind the source's back (as in rnn.hip): the cell is evaluated exactly as written.
#pragma clang fp contract(off)

namespace {

constexpr int LS_ROWS = 64;      // batch rows per workgroup: 4 waves x 16
constexpr int LS_UNITS = 16;     // hidden units per workgroup: 64 columns of U forward, 16 rows of U backward
constexpr int LS_KCF = 256;      // forward: rows of U per LDS chunk (256 x 66 floats = 66 KiB)
constexpr int LS_KCB = 1024;     // backward: columns of U per LDS chunk (1024 x 18 floats = 72 KiB; 4H = 1000 is one chunk)
// LDS row strides: 8 * ld = 16 (mod 64 banks), so the four k groups of a wave (rows k, k+8, k+16, k+24) hit disjoint banks
constexpr int LS_LDF = 66;
constexpr int LS_LDB = 18;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

struct StepArgs {
    const float* U[2];
    float* zg;
    float* hseq;
    long h_rs;
    float* cseq;
    const float* dh_seq;
    long dh_bs, dh_rs;
    const float* dh_last;
    float* carry;
    int B, T, H, dirs;
};

// this lane's A values k .. k+7 of a chunk (zeros past klen or for a row past B); VW floats per load, klen % VW == 0
template <int VW>
__device__ __forceinline__ void load_a(float (&av)[8], const float* __restrict__ arow, bool aok, int k, int klen) {
    if (VW == 4) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (aok && k < klen) v0 = *reinterpret_cast<const float4*>(arow + k);
        if (aok && k + 4 < klen) v1 = *reinterpret_cast<const float4*>(arow + k + 4);
        av[0] = v0.x; av[1] = v0.y; av[2] = v0.z; av[3] = v0.w;
        av[4] = v1.x; av[5] = v1.y; av[6] = v1.z; av[7] = v1.w;
    } else if (VW == 2) {
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            float2 v = make_float2(0.f, 0.f);
            if (aok && k + e < klen) v = *reinterpret_cast<const float2*>(arow + k + e);
            av[e] = v.x; av[e + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = aok && k + e < klen ? arow[k + e] : 0.0f;
    }
}

// A blocks of 32 k in flight per lane ahead of the MFMAs that consume them: a step is bound by the latency of these loads
// (the MFMAs of a block take far less than one trip to L2), so LS_PF blocks are fetched per trip
constexpr int LS_PF = 4;

// an[j] = this lane's values of block k0 / 32 + j of the chunk (zeros past klen)
template <int VW>
__device__ __forceinline__ void load_group(float (&an)[LS_PF][8], const float* __restrict__ arow, bool aok, int k0, int klen,
                                           int lane) {
#pragma unroll
    for (int j = 0; j < LS_PF; ++j) load_a<VW>(an[j], arow, aok, k0 + 32 * j + 8 * (lane >> 4), klen);
}

// acc[g] += A[16 rows of this wave][kc .. kc+klen) . Bs[k][16 g + c].  arow: this lane's A row at the chunk start (row
// l & 15 of the wave; aok false: a row past B, which contributes zeros); an: the chunk's first group, load_group(.., 0, ..),
// which the caller issues ahead of the staging of Bs.  Bs holds kpad = klen rounded up to 32 rows, zero past klen.  The next
// group's A values are loaded before this group's MFMAs; the k order is block by block whatever LS_PF is.
template <int NG, int VW>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[NG], float (&an)[LS_PF][8], const float* __restrict__ arow, bool aok,
                                          int klen, int kpad, const float* Bs, int ldb, int lane) {
    const int c = lane & 15, kg = lane >> 4;
    float av[LS_PF][8];
    for (int k0 = 0; k0 < kpad; k0 += 32 * LS_PF) {
#pragma unroll
        for (int j = 0; j < LS_PF; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) av[j][e] = an[j][e];
        if (k0 + 32 * LS_PF < kpad) load_group<VW>(an, arow, aok, k0 + 32 * LS_PF, klen, lane);
#pragma unroll
        for (int j = 0; j < LS_PF; ++j) {
            const int k = k0 + 32 * j + 8 * kg;
            if (k0 + 32 * j >= kpad) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* br = Bs + (k + e) * ldb + c;
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][e], br[g * 16], acc[g], 0, 0, 0);
            }
        }
    }
}

// LDS staging of n items by the workgroup's 256 threads: 64 registers of loads in flight per thread before their stores
// (a load-store loop would wait out one memory latency per item)
template <typename V, typename Load, typename Store>
__device__ __forceinline__ void stage(int n, Load load, Store store) {
    constexpr int NB = sizeof(V) == 16 ? 16 : 32;
    for (int base = threadIdx.x; base < n; base += 256 * NB) {
        V v[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int i = base + 256 * j;
            if (i < n) v[j] = load(i);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int i = base + 256 * j;
            if (i < n) store(i, v[j]);
        }
    }
}

// forward chunk: Bs[kk][16 g + c] = U[kc + kk][g H + u0 + c] (zero past klen / H); VW floats per load along the units
template <int VW>
__device__ __forceinline__ void stage_fwd(float* Bs, const float* __restrict__ U, int H, int u0, int kc, int klen, int kpad) {
    const size_t H4 = 4 * (size_t)H;
    if (VW == 4) {
        stage<float4>(kpad * 16, [&](int e) {
            const int kk = e >> 4, q = e & 15, u = u0 + 4 * (q & 3);
            return kk < klen && u < H ? *reinterpret_cast<const float4*>(U + (kc + kk) * H4 + (q >> 2) * H + u)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            const int kk = e >> 4, q = e & 15;
            float* d = Bs + kk * LS_LDF + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        });
    } else if (VW == 2) {
        stage<float2>(kpad * 32, [&](int e) {
            const int kk = e >> 5, q = e & 31, u = u0 + 2 * (q & 7);
            return kk < klen && u < H ? *reinterpret_cast<const float2*>(U + (kc + kk) * H4 + (q >> 3) * H + u)
                                      : make_float2(0.f, 0.f);
        }, [&](int e, float2 v) {
            const int kk = e >> 5, q = e & 31;
            float* d = Bs + kk * LS_LDF + 2 * q;
            d[0] = v.x; d[1] = v.y;
        });
    } else {
        stage<float>(kpad * 64, [&](int e) {
            const int kk = e >> 6, j = e & 63, u = u0 + (j & 15);
            return kk < klen && u < H ? U[(kc + kk) * H4 + (j >> 4) * H + u] : 0.0f;
        }, [&](int e, float v) {
            const int kk = e >> 6, j = e & 63;
            Bs[kk * LS_LDF + j] = v;
        });
    }
}

// backward chunk: Bs[kk][c] = U[u0 + c][kc + kk] over the 4H columns of a row (zero past klen / H); float4 loads along k when VEC
template <bool VEC>
__device__ __forceinline__ void stage_bwd(float* Bs, const float* __restrict__ U, int H, int u0, int kc, int klen, int kpad) {
    const size_t H4 = 4 * (size_t)H;
    if (VEC) {
        const int k4n = kpad / 4;
        stage<float4>(16 * k4n, [&](int e) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n), u = u0 + c;
            return k4 < klen && u < H ? *reinterpret_cast<const float4*>(U + u * H4 + kc + k4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n);
            float* d = Bs + k4 * LS_LDB + c;
            d[0] = v.x; d[LS_LDB] = v.y; d[2 * LS_LDB] = v.z; d[3 * LS_LDB] = v.w;
        });
    } else {
        stage<float>(16 * kpad, [&](int e) {
            const int c = e / kpad, kk = e - c * kpad, u = u0 + c;
            return kk < klen && u < H ? U[u * H4 + kc + kk] : 0.0f;
        }, [&](int e, float v) {
            const int c = e / kpad, kk = e - c * kpad;
            Bs[kk * LS_LDB + c] = v;
        });
    }
}

// one forward step s of both directions (direction d: t = s forward, T-1-s reverse)
template <int VW>
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(const StepArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[LS_KCF * LS_LDF];
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H4 = 4 * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * LS_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int prow = d == 0 ? t : t + 2;                      // hseq row of h_{t-1} (forward) / h_{t+1} (reverse)
    const int rb = blockIdx.x * LS_ROWS + w * 16;
    // the cell's own operands (the step's slice of zg, c_{t-1}) do not depend on the product: they are fetched first, so that
    // their trip to HBM runs under it.  Lane (c, g) holds unit u0 + c of rows rb + 4g + i (the 16x16 C/D map: col = lane & 15,
    // row = 4 (lane >> 4) + i).
    const int u = u0 + (lane & 15);
    const int tp = d == 0 ? t - 1 : t + 1;
    float xz[4][4], cprev[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        const bool ok = u < H && b < B;
        const size_t row = ((size_t)d * B + (ok ? b : 0)) * T;
        const float* gz = a.zg + (row + t) * H4 + (ok ? u : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) xz[q][i] = ok ? gz[q * H] : 0.0f;
        cprev[i] = ok && s > 0 ? a.cseq[(row + tp) * H + u] : 0.0f;
    }
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ra = rb + (lane & 15);
        const bool aok = ra < B;
        const float* arow = a.hseq + ((size_t)(aok ? ra : 0) * (T + 2) + prow) * a.h_rs + d * H;
        const float* U = a.U[d];
        for (int kc = 0; kc < H; kc += LS_KCF) {
            const int klen = min(LS_KCF, H - kc), kpad = (klen + 31) & ~31;
            float an[LS_PF][8];
            load_group<VW>(an, arow + kc, aok, 0, klen, lane);   // in flight while U is staged
            __syncthreads();                                  // the previous chunk's LDS reads are done
            stage_fwd<VW>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<4, VW>(acc, an, arow + kc, aok, klen, kpad, Bs, LS_LDF, lane);
        }
    }
    if (u >= H) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        if (b >= B) continue;
        const size_t row = ((size_t)d * B + b) * T;
        float* gz = a.zg + (row + t) * H4 + u;
        const float ig = sigm(xz[0][i] + acc[0][i]), fg = sigm(xz[1][i] + acc[1][i]);
        const float gg = tanhf(xz[2][i] + acc[2][i]), og = sigm(xz[3][i] + acc[3][i]);
        const float c = fg * cprev[i] + ig * gg;
        gz[0] = ig;
        gz[H] = fg;
        gz[2 * H] = gg;
        gz[3 * H] = og;
        a.cseq[(row + t) * H + u] = c;
        a.hseq[((size_t)b * (T + 2) + t + 1) * a.h_rs + d * H + u] = og * tanhf(c);
    }
}

// cell backward of one (row, unit): gates v = {i, f, g, o}, returns dZ in v, updates dc (as rnn.hip's cell_bwd)
__device__ __forceinline__ void cell_bwd(float v[4], float ct, float cprev, float dh, float& dc) {
    const float ig = v[0], fg = v[1], gg = v[2], og = v[3];
    const float tc = tanhf(ct);
    const float dct = dc + dh * og * (1.0f - tc * tc);
    v[0] = dct * gg * ig * (1.0f - ig);
    v[1] = dct * cprev * fg * (1.0f - fg);
    v[2] = dct * ig * (1.0f - gg * gg);
    v[3] = dh * tc * og * (1.0f - og);
    dc = dct * fg;
}

// one backward step s (walked from T-1 down): dh_t = incoming + dZ_{t+1} U^T, dc carried, then the cell backward
template <bool VEC>
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(const StepArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[LS_KCB * LS_LDB];
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H4 = 4 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * LS_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int rb = blockIdx.x * LS_ROWS + w * 16;
    // the cell's own operands (gates, c_t, c_{t-1}, incoming dh, carried dc) are fetched ahead of the product, as in forward
    const int u = u0 + (lane & 15);
    const int tp = d == 0 ? t - 1 : t + 1;
    float v[4][4], ct[4], cprev[4], dhin[4], dc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        const bool ok = u < H && b < B;
        const size_t bo = ok ? b : 0, uo = ok ? u : 0;
        const size_t row = ((size_t)d * B + bo) * T;
        const float* gz = a.zg + (row + t) * H4 + uo;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[i][q] = ok ? gz[q * H] : 0.0f;
        ct[i] = ok ? a.cseq[(row + t) * H + uo] : 0.0f;
        cprev[i] = ok && s > 0 ? a.cseq[(row + tp) * H + uo] : 0.0f;
        float in = 0.0f;
        if (ok && a.dh_seq) in = a.dh_seq[bo * a.dh_bs + (size_t)t * a.dh_rs + d * H + uo];
        if (ok && a.dh_last && s == T - 1) in += a.dh_last[bo * ldo + d * H + uo];
        dhin[i] = in;
        dc[i] = ok && s < T - 1 ? a.carry[((size_t)d * B + bo) * H + uo] : 0.0f;
    }
    f32x4 acc[1];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s < T - 1) {                                          // the direction's last step has no later step
        const int tn = d == 0 ? t + 1 : t - 1;
        const int ra = rb + (lane & 15);
        const bool aok = ra < B;
        const float* arow = a.zg + (((size_t)d * B + (aok ? ra : 0)) * T + tn) * H4;
        const float* U = a.U[d];
        for (int kc = 0; kc < H4; kc += LS_KCB) {
            const int klen = min(LS_KCB, H4 - kc), kpad = (klen + 31) & ~31;
            float an[LS_PF][8];
            load_group<VEC ? 4 : 1>(an, arow + kc, aok, 0, klen, lane);
            __syncthreads();
            stage_bwd<VEC>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<1, VEC ? 4 : 1>(acc, an, arow + kc, aok, klen, kpad, Bs, LS_LDB, lane);
        }
    }
    if (u >= H) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = rb + 4 * (lane >> 4) + i;
        if (b >= B) continue;
        const size_t row = ((size_t)d * B + b) * T;
        float* gz = a.zg + (row + t) * H4 + u;
        float dz[4] = {v[i][0], v[i][1], v[i][2], v[i][3]};
        float dcv = dc[i];
        cell_bwd(dz, ct[i], cprev[i], acc[0][i] + dhin[i], dcv);
        gz[0] = dz[0];
        gz[H] = dz[1];
        gz[2 * H] = dz[2];
        gz[3 * H] = dz[3];
        a.carry[((size_t)d * B + b) * H + u] = dcv;
    }
}

int check_common(const char* fn, const float* U0, const float* U1, int dirs, int B, int T, int H) {
    if (!(dirs == 1 || dirs == 2) || !U0 || (dirs == 2 && !U1) || B < 0 || T < 1 || H < 1) {
        lidbox_set_error("%s: invalid argument: dirs in {1, 2}, U0 (and U1 when dirs == 2) != NULL, B >= 0, T >= 1, H >= 1", fn);
        return LIDBOX_E_INVALID;
    }
    if (H > 65535 || (long)B * T * 4 * H > (1L << 40)) {
        lidbox_set_error("%s: invalid argument: H <= 65535, B * T * 4H <= 2^40", fn);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

inline uintptr_t bits(const void* p) { return (uintptr_t)p; }

// widest forward load: 4 (float4), 2 (float2) or 1 floats -- H, the row stride of hseq and the pointers all multiples of it
inline int fwd_width(int H, long h_rs, const void* U0, const void* U1, const void* hseq) {
    const uintptr_t p = bits(U0) | bits(U1) | bits(hseq);
    if (H % 4 == 0 && h_rs % 4 == 0 && (p & 15) == 0) return 4;
    if (H % 2 == 0 && h_rs % 2 == 0 && (p & 7) == 0) return 2;
    return 1;
}

inline dim3 step_grid(int B, int H, int dirs) {
    return dim3((unsigned)lbx_cdiv(B, LS_ROWS), (unsigned)lbx_cdiv(H, LS_UNITS), (unsigned)dirs);
}

}  // namespace

extern "C" size_t lidbox_lstm_step_workspace(int B, int T, int H, int dirs) {
    if (B <= 0 || T < 1 || H < 1 || dirs < 1 || dirs > 2) return 0;
    return (size_t)dirs * B * H * sizeof(float);
}

extern "C" int lidbox_lstm_step_fwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, float* hseq,
                                    long h_row_stride, float* cseq, void* workspace, size_t workspace_bytes,
                                    lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && hseq && cseq, "zg, hseq, cseq != NULL");
    LBX_ARG(h_row_stride >= (long)dirs * H, "h_row_stride >= dirs * H");
    if (B == 0) return LIDBOX_OK;
    (void)workspace;                                          // forward carries nothing between steps
    (void)workspace_bytes;
    StepArgs a{{U0, dirs == 2 ? U1 : U0}, zg, hseq, h_row_stride, cseq, nullptr, 0, 0, nullptr, nullptr, B, T, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = step_grid(B, H, dirs);
    const int vw = fwd_width(H, h_row_stride, a.U[0], a.U[1], hseq);
    for (int s = 0; s < T; ++s) {
        if (vw == 4)
            hipLaunchKernelGGL(lstm_step_fwd_kernel<4>, grid, dim3(256), 0, st, a, s);
        else if (vw == 2)
            hipLaunchKernelGGL(lstm_step_fwd_kernel<2>, grid, dim3(256), 0, st, a, s);
        else
            hipLaunchKernelGGL(lstm_step_fwd_kernel<1>, grid, dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_lstm_step_bwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg,
                                    const float* cseq, const float* dh_seq, long dh_batch_stride, long dh_row_stride,
                                    const float* dh_last, void* workspace, size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && cseq && (dh_seq || dh_last), "zg, cseq != NULL; dh_seq or dh_last != NULL");
    LBX_ARG(!dh_seq || dh_row_stride >= (long)dirs * H, "dh_row_stride >= dirs * H");
    LBX_ARG(!dh_seq || dh_batch_stride >= (long)(T - 1) * dh_row_stride + (long)dirs * H,
            "dh_batch_stride >= (T - 1) * dh_row_stride + dirs * H");
    if (B == 0) return LIDBOX_OK;
    LBX_ARG(workspace && workspace_bytes >= lidbox_lstm_step_workspace(B, T, H, dirs),
            "workspace >= lidbox_lstm_step_workspace() bytes");
    StepArgs a{{U0, dirs == 2 ? U1 : U0}, zg, nullptr, 0, const_cast<float*>(cseq), dh_seq, dh_batch_stride, dh_row_stride,
               dh_last, (float*)workspace, B, T, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = step_grid(B, H, dirs);
    // K = 4H and rows 4H floats apart: float4 loads need aligned pointers only
    const bool vec = ((bits(a.U[0]) | bits(a.U[1]) | bits(zg)) & 15) == 0;
    for (int s = T - 1; s >= 0; --s) {
        if (vec)
            hipLaunchKernelGGL(lstm_step_bwd_kernel<true>, grid, dim3(256), 0, st, a, s);
        else
            hipLaunchKernelGGL(lstm_step_bwd_kernel<false>, grid, dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}
