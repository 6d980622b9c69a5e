// rnn_step.h -- the MFMA step pipeline shared by the fused recurrence kernels (gru.hip, lstm_step.hip), gfx950.
//
// Both walk a layer with one launch per time step that covers both directions.  Grid = ceil(B / 64) row tiles x
// ceil(H / 16) unit slices x dirs; a workgroup is 4 waves, wave w owns rows 16w..16w+15 of its tile.  The NG gates of unit j
// read only columns j, H+j, .. of U, so a workgroup computes h_{t-1}[rows, :] U[:, NG x 16 columns of its units] with
// v_mfma_f32_16x16x4_f32 (exact fp32) into NG accumulators whose (row, unit) positions coincide in every lane, and applies
// the cell in the same kernel.  Forward stages U's 16 NG columns of the slice into LDS in KCF-row chunks; backward computes
// dh_rec = dZ_{t+1} U^T for its units, staging U's 16 rows of the slice in KCB-column chunks.  The A operand (h_{t-1} or
// dZ_{t+1} rows) streams from global memory: lane (c, g) = (l & 15, l >> 4) loads row c, k = k0 + 8g .. k0 + 8g + 7, and
// MFMA e of the k0 block consumes element e -- a fixed permutation of the k order, the same for the 16-, 8- and 4-byte load
// paths, so all paths give the same bits.  PF 32-k blocks of A are fetched per trip to L2.
//
// What differs between the two recurrences is a parameter set (GruStep, LstmStep) and the kernels themselves: the cell,
// which of its operands are fetched ahead of the product, and where the first A trip of a chunk is issued.
//
// At the end: the row maps (DenseRows, RaggedRows) through which one forward kernel per recurrence serves the dense and the
// ragged walk, and the host checks of the ragged entry points (check_ragged_args, running).
#pragma once

#include <stdint.h>

#include "common.h"
#include "rnn_cell.h"

#pragma clang fp contract(off)

namespace {

constexpr int STEP_ROWS = 64;    // batch rows per workgroup: 4 waves x 16
constexpr int STEP_UNITS = 16;   // hidden units per workgroup: 16 NG columns of U forward, 16 rows of U backward

// NG: gates.  PF: A blocks of 32 k in flight per lane ahead of the MFMAs that consume them -- a step is bound by the latency
// of these loads (the MFMAs of a block take far less than one trip to L2).  NB4 / NB1: loads in flight per thread and
// staging trip, float4 / narrower (LSTM: 64 registers either way).  KCF: forward, rows of U per LDS chunk.  KCB: backward,
// columns of U per LDS chunk.
struct GruStep {                 // LDS: 256 x 50 floats = 50 KiB forward, 768 x 18 floats = 54 KiB backward
    static constexpr int NG = 3, PF = 1, NB4 = 12, NB1 = 12, KCF = 256, KCB = 768;
};
struct LstmStep {                // LDS: 256 x 66 floats = 66 KiB forward, 1024 x 18 floats = 72 KiB (4H = 1000 is one chunk)
    static constexpr int NG = 4, PF = 4, NB4 = 16, NB1 = 32, KCF = 256, KCB = 1024;
};

// LDS row strides: 8 * ld = 16 (mod 64 banks), so the four k groups of a wave (rows k, k+8, k+16, k+24) hit disjoint banks
template <typename P>
constexpr int STEP_LDF = 16 * P::NG + 2;
constexpr int STEP_LDB = 18;
static_assert(8 * STEP_LDF<GruStep> % 64 == 16 && 8 * STEP_LDF<LstmStep> % 64 == 16 && 8 * STEP_LDB % 64 == 16, "LDS stride");

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// an[j] = this lane's values of block k0 / 32 + j of the chunk (zeros past klen); k = k0 + 8 (lane >> 4), the lane's own k.
// The lane term comes in with k: added to k0 + 32 PF here instead, the GRU's loop carries one more address add per block.
// Block 0 stands outside the loop: as the one trip of an unrolled loop (PF = 1) its address arithmetic is placed
// differently, and with both forms as they are the GRU kernels compile to the code they had before the pipeline was shared.
template <int VW, int PF>
__device__ __forceinline__ void load_group(float (&an)[PF][8], const float* __restrict__ arow, bool aok, int k, int klen) {
    load_a<VW>(an[0], arow, aok, k, klen);
#pragma unroll
    for (int j = 1; j < PF; ++j) load_a<VW>(an[j], arow, aok, k + 32 * j, klen);
}

// acc[g] += A[16 rows of this wave][kc .. kc+klen) . Bs[k][16 g + c].  arow: this lane's A row at the chunk start (row
// l & 15 of the wave; aok false: a row past B, which contributes zeros); an: the chunk's first group, load_group(.., 8 (l >> 4), ..),
// which the caller issues (ahead of the staging of Bs, or after it).  Bs holds kpad = klen rounded up to 32 rows, zero past
// klen.  The next group's A values are loaded before this group's MFMAs; the k order is block by block whatever PF is.
template <int NG, int VW, int PF>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[NG], float (&an)[PF][8], const float* __restrict__ arow, bool aok,
                                          int klen, int kpad, const float* Bs, int ldb, int lane) {
    const int c = lane & 15, kg = lane >> 4;
    float av[PF][8];
    for (int k0 = 0; k0 < kpad; k0 += 32 * PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) av[j][e] = an[j][e];
        const int k = k0 + 8 * kg;
        if (k0 + 32 * PF < kpad) load_group<VW, PF>(an, arow, aok, k + 32 * PF, klen);
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            if (k0 + 32 * j >= kpad) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* br = Bs + (k + 32 * j + e) * ldb + c;
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][e], br[g * 16], acc[g], 0, 0, 0);
            }
        }
    }
}

// the same with the chunk's first group issued here, after the staging of Bs
template <int NG, int VW, int PF>
__device__ __forceinline__ void mma_chunk(f32x4 (&acc)[NG], const float* __restrict__ arow, bool aok, int klen, int kpad,
                                          const float* Bs, int ldb, int lane) {
    float an[PF][8];
    load_group<VW, PF>(an, arow, aok, 8 * (lane >> 4), klen);
    mma_chunk<NG, VW, PF>(acc, an, arow, aok, klen, kpad, Bs, ldb, lane);
}

// LDS staging of n items by the workgroup's 256 threads: NB loads in flight per thread before their stores (a load-store
// loop would wait out one memory latency per item)
template <int NB, typename V, typename Load, typename Store>
__device__ __forceinline__ void stage(int n, Load load, Store store) {
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

// e = N kk + q with 0 <= q < N, for e >= 0.  A power of two is written as shift and mask: the compiler cannot see that a
// staging index is never negative, and the sign handling of e / N changes the register allocation of whole kernels.
template <int N>
__device__ __forceinline__ void split(int e, int& kk, int& q) {
    if ((N & (N - 1)) == 0) {
        kk = e >> __builtin_ctz(N);
        q = e & (N - 1);
    } else {
        kk = e / N;
        q = e - kk * N;
    }
}

// forward chunk: Bs[kk][16 g + c] = U[kc + kk][g H + u0 + c] (zero past klen / H); VW floats per load along the units
template <typename P, int VW>
__device__ __forceinline__ void stage_fwd(float* Bs, const float* __restrict__ U, int H, int u0, int kc, int klen, int kpad) {
    constexpr int NG = P::NG, LD = STEP_LDF<P>;
    const size_t HG = NG * (size_t)H;
    if (VW == 4) {
        stage<P::NB4, float4>(kpad * 4 * NG, [&](int e) {
            int kk, q;
            split<4 * NG>(e, kk, q);
            const int u = u0 + 4 * (q & 3);
            return kk < klen && u < H ? *reinterpret_cast<const float4*>(U + (kc + kk) * HG + (q >> 2) * H + u)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            int kk, q;
            split<4 * NG>(e, kk, q);
            float* d = Bs + kk * LD + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        });
    } else if (VW == 2) {
        stage<P::NB1, float2>(kpad * 8 * NG, [&](int e) {
            int kk, q;
            split<8 * NG>(e, kk, q);
            const int u = u0 + 2 * (q & 7);
            return kk < klen && u < H ? *reinterpret_cast<const float2*>(U + (kc + kk) * HG + (q >> 3) * H + u)
                                      : make_float2(0.f, 0.f);
        }, [&](int e, float2 v) {
            int kk, q;
            split<8 * NG>(e, kk, q);
            float* d = Bs + kk * LD + 2 * q;
            d[0] = v.x; d[1] = v.y;
        });
    } else {
        stage<P::NB1, float>(kpad * 16 * NG, [&](int e) {
            int kk, j;
            split<16 * NG>(e, kk, j);
            const int u = u0 + (j & 15);
            return kk < klen && u < H ? U[(kc + kk) * HG + (j >> 4) * H + u] : 0.0f;
        }, [&](int e, float v) {
            int kk, j;
            split<16 * NG>(e, kk, j);
            Bs[kk * LD + j] = v;
        });
    }
}

// backward chunk: Bs[kk][c] = U[u0 + c][col0 + kk], rows NG H floats apart (zero past klen / H); float4 loads along k when VEC
template <typename P, bool VEC>
__device__ __forceinline__ void stage_bwd(float* Bs, const float* __restrict__ U, int H, int u0, int col0, int klen, int kpad) {
    const size_t HG = P::NG * (size_t)H;
    if (VEC) {
        const int k4n = kpad / 4;
        stage<P::NB4, float4>(16 * k4n, [&](int e) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n), u = u0 + c;
            return k4 < klen && u < H ? *reinterpret_cast<const float4*>(U + u * HG + col0 + k4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }, [&](int e, float4 v) {
            const int c = e / k4n, k4 = 4 * (e - c * k4n);
            float* d = Bs + k4 * STEP_LDB + c;
            d[0] = v.x; d[STEP_LDB] = v.y; d[2 * STEP_LDB] = v.z; d[3 * STEP_LDB] = v.w;
        });
    } else {
        stage<P::NB1, float>(16 * kpad, [&](int e) {
            const int c = e / kpad, kk = e - c * kpad, u = u0 + c;
            return kk < klen && u < H ? U[u * HG + col0 + kk] : 0.0f;
        }, [&](int e, float v) {
            const int c = e / kpad, kk = e - c * kpad;
            Bs[kk * STEP_LDB + c] = v;
        });
    }
}

// the arguments every entry point shares; ng: gates, for the bound on the size of zg
inline int check_step_args(const char* fn, int ng, const float* U0, const float* U1, int dirs, int B, int T, int H) {
    if (!(dirs == 1 || dirs == 2) || !U0 || (dirs == 2 && !U1) || B < 0 || T < 1 || H < 1) {
        lidbox_set_error("%s: invalid argument: dirs in {1, 2}, U0 (and U1 when dirs == 2) != NULL, B >= 0, T >= 1, H >= 1", fn);
        return LIDBOX_E_INVALID;
    }
    if (H > 65535 || (long)B * T * ng * H > (1L << 40)) {
        lidbox_set_error("%s: invalid argument: H <= 65535, B * T * %dH <= 2^40", fn, ng);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

// every pointer is a multiple of bytes (a power of two)
template <typename... Ptr>
inline bool aligned_to(unsigned bytes, Ptr... p) {
    return ((... | (uintptr_t)p) & (bytes - 1)) == 0;
}

inline dim3 step_grid(int B, int H, int dirs) {
    return dim3((unsigned)lbx_cdiv(B, STEP_ROWS), (unsigned)lbx_cdiv(H, STEP_UNITS), (unsigned)dirs);
}

// ---------------------------------------------------------------------------------------------------------------- row maps
// Where a row lives is all that differs between a forward walk over a dense batch and one over utterances of DIFFERENT
// lengths (forward only, inference; no reference counterpart: tf.data batches need one shape, and the Keras layers run
// without masking, so a padded batch starts every reverse direction inside the padding).  The forward kernels ask a map.
//
// Dense: zg / cseq / qh [dirs][B][T], hseq [B][T+2] with frame t at row t+1 and zero rows 0 and T+1, hlast [B].
//
// Ragged (the dense [B][T+2] convention with a per-utterance T; lidbox_hip.h has the buffers): utterance b with T_b frames owns
// the rows seg[b] .. seg[b+1] = seg[b] + T_b + 2 of every per-frame buffer of the layer.  Row seg[b] is a pad row, frame t sits at
// row seg[b] + 1 + t, row seg[b+1] - 1 is a pad row.  One row index serves hseq [rows][h_row_stride], zg [dirs][rows][NG H] and
// cseq / qh [dirs][rows][H], so a layer's input projection is ONE GEMM over all rows (the pad rows of zg receive the bias and are
// never read) and no utterance is ever moved in memory.
//
// The walk: step s = 0 .. T_max - 1 is one launch for both directions, over the n_s = #{b : T_b > s} utterances still running
// (dense: all B, every step).  Slot j of a ragged step is the j-th longest utterance (stable sort by length, descending), so the
// running ones are the slots 0 .. n_s - 1 of a device table `slots` [3][B] = (first row seg[b], length T_b, utterance index b);
// a dense slot is the batch row.  Grid = ceil(n_s / 64) x ceil(H / 16) x dirs: later ragged steps launch fewer row tiles.
// Direction 0 works on t = s, direction 1 on t = T_b - 1 - s.  In both layouts the neighbour state sits one row in front of
// (direction 0) resp. behind (direction 1) the frame's own row, in hseq and in cseq alike; in a ragged buffer that is inside the
// utterance's own segment.  The first step of a direction skips the product (h_{-1} = 0) and reads no neighbour.
//
// Every output element is one MFMA k-chain over its own row, so every utterance's gates, c / qh, h and hlast of a ragged walk
// are bit for bit what the dense walk gives it at B = 1, T = T_b, whatever its neighbours, its place in the batch and its slot.
//
// A kernel asks `at(j, d, s)` for a slot's At and the other members for its rows.  A ragged At is the frame's row, looked up in
// `slots`: LOOKUP tells a kernel that prefetches to keep it over the product, so that the dependent load runs under the product
// and not in front of the stores (0.9 us per step of the LSTM, LAB_NOTEBOOK section 32).  A dense At is the batch row itself,
// cheaper to form again than to keep in a kernel at the register limit.
struct DenseRows {
    int B, T;
    typedef int At;              // the batch row
    static constexpr bool LOOKUP = false;
    __device__ __forceinline__ At at(int j, int, int) const { return j; }
    __device__ __forceinline__ int t(int d, int s) const { return d == 0 ? s : T - 1 - s; }
    // row of the frame in zg / cseq / qh, and in hseq
    __device__ __forceinline__ size_t frame(At b, int d, int s) const { return ((size_t)d * B + b) * T + t(d, s); }
    __device__ __forceinline__ size_t hrow(At b, int d, int s) const { return (size_t)b * (T + 2) + t(d, s) + 1; }
    // is s the last step of slot j (t = T - 1 forward, t = 0 reverse), and its row of hlast
    __device__ __forceinline__ bool last(int, int s) const { return s == T - 1; }
    __device__ __forceinline__ size_t out(int j) const { return j; }
};

struct RaggedRows {
    const long* slots;           // [3][B]: first row, length, utterance index of slot j
    long rows;                   // rows per direction of zg and cseq / qh
    int B;
    typedef long At;             // the frame's row within a direction
    static constexpr bool LOOKUP = true;
    __device__ __forceinline__ At at(int j, int d, int s) const {
        return slots[j] + 1 + (d == 0 ? (long)s : slots[B + j] - 1 - s);
    }
    __device__ __forceinline__ size_t frame(At r, int d, int) const { return (size_t)d * rows + r; }
    __device__ __forceinline__ size_t hrow(At r, int, int) const { return r; }
    __device__ __forceinline__ bool last(int j, int s) const { return slots[B + j] == s + 1; }
    __device__ __forceinline__ size_t out(int j) const { return slots[2 * B + j]; }
};

// what a ragged walk asks of its arguments beyond check_step_args (B >= 1 here); ng: gates
inline int check_ragged_args(const char* fn, int ng, int dirs, int B, int H, long rows, const long* slots,
                             const long* sorted_lengths, const float* zg, const float* hseq, const float* aux, long h_rs) {
    if (!(slots && sorted_lengths && zg && hseq && aux)) {
        lidbox_set_error("%s: invalid argument: slots, sorted_lengths, zg, hseq and %s != NULL", fn, ng == 4 ? "cseq" : "qh");
        return LIDBOX_E_INVALID;
    }
    if (h_rs < (long)dirs * H) {
        lidbox_set_error("%s: invalid argument: h_row_stride >= dirs * H", fn);
        return LIDBOX_E_INVALID;
    }
    long total = 0;
    for (int j = 0; j < B; ++j) {
        if (sorted_lengths[j] < 1 || (j > 0 && sorted_lengths[j] > sorted_lengths[j - 1]) || sorted_lengths[j] > INT32_MAX - 2) {
            lidbox_set_error("%s: invalid argument: sorted_lengths must be >= 1 and non-increasing (entry %d is %ld)", fn, j,
                             sorted_lengths[j]);
            return LIDBOX_E_INVALID;
        }
        total += sorted_lengths[j];
    }
    if (rows < total + 2L * B || rows > (1L << 40) / ((long)ng * H)) {
        lidbox_set_error("%s: invalid argument: rows >= sum of lengths + 2 B (%ld), rows * %dH <= 2^40", fn, total + 2L * B, ng);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

// the slots of a ragged walk still running at step s, of the n that ran the step before: sorted_lengths is non-increasing
inline int running(const long* sorted_lengths, int n, int s) {
    while (n > 0 && sorted_lengths[n - 1] <= s) --n;
    return n;
}

}  // namespace
