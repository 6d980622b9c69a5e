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
// One form, any H: the step pipeline of rnn_step.h with its GruStep parameters (three gates: 48 columns of U per slice in
// 256-row chunks forward, 768-column chunks backward, one A block in flight, issued after the staging).  Backward's K = 3H
// runs over three sources -- (dz, dr) from zg and dhh * r from qh -- so U is staged one gate block at a time.
//
// Load paths: float4 when H % 4 == 0 and every buffer is 16-byte aligned (then every row and chunk start is aligned too),
// scalar otherwise; both feed the MFMAs in the same k order and give the same bits.
//
// The forward kernel is a template over a row map (rnn_step.h: DenseRows for the buffers above, RaggedRows for utterances of
// different lengths in one walk, lidbox_gru_ragged_fwd; layout and walk are described there).
//
// No inter-workgroup communication, no atomics, no spin-waits: steps are ordered by the stream alone.  Every output element
// is one MFMA k-chain over its own row, in an order that depends on neither B nor the row's place in the batch, so a
// row's results are bit-identical whatever the batch.
#include <math.h>

#include "rnn_step.h"

// No a*b+c is contracted behind the source's back (as in rnn.hip): the cell is evaluated exactly as written.
#pragma clang fp contract(off)

namespace {

// backward's arguments (brec and hlast are forward's: unused)
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

// forward's arguments; where a row lives is the map's business (rnn_step.h)
template <typename Rows>
struct FwdArgs {
    const float* U[2];
    const float* brec[2];
    float* zg;
    float* hseq;                 // rows dirs * H wide
    float* qh;
    float* hlast;                // may be NULL
    Rows rows;
    int H, dirs;
};

// one forward step s of both directions over the slots 0 .. n-1 (direction d: t = s forward, T-1-s reverse)
template <bool VEC, typename Rows>
__global__ __launch_bounds__(256) void gru_fwd_step_kernel(const FwdArgs<Rows> a, int s, int n) {
    __shared__ __attribute__((aligned(16))) float Bs[GruStep::KCF * STEP_LDF<GruStep>];
    constexpr int VW = VEC ? 4 : 1;
    const int H = a.H, d = blockIdx.z, H3 = 3 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const long nb = d == 0 ? -1 : 1;                          // the neighbour state's row: h_{t-1} (forward) / h_{t+1} (reverse)
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ja = rb + (lane & 15);
        const bool aok = ja < n;
        const float* arow = a.hseq + (a.rows.hrow(a.rows.at(aok ? ja : 0, d, s), d, s) + nb) * ldo + d * H;
        const float* U = a.U[d];
        for (int kc = 0; kc < H; kc += GruStep::KCF) {
            const int klen = min(GruStep::KCF, H - kc), kpad = (klen + 31) & ~31;
            __syncthreads();                                  // the previous chunk's LDS reads are done
            stage_fwd<GruStep, VW>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<3, VW, GruStep::PF>(acc, arow + kc, aok, klen, kpad, Bs, STEP_LDF<GruStep>, lane);
        }
    }
    // epilogue: lane (c, g) holds unit u0 + c of rows rb + 4g + i (the 16x16 C/D map: col = lane & 15, row = 4 (lane >> 4) + i)
    const int u = u0 + (lane & 15);
    if (u >= H) return;
    const float* br = a.brec[d];
    const float bz = br[u], brr = br[H + u], bh = br[2 * H + u];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = rb + 4 * (lane >> 4) + i;
        if (j >= n) continue;
        const typename Rows::At at = a.rows.at(j, d, s);
        const size_t row = a.rows.frame(at, d, s), hr = a.rows.hrow(at, d, s);
        float* gz = a.zg + row * H3 + u;
        const float qz = acc[0][i] + bz, qr = acc[1][i] + brr, qhv = acc[2][i] + bh;
        const float z = sigm(gz[0] + qz), r = sigm(gz[H] + qr);
        const float hh = tanhf(gz[2 * H] + r * qhv);
        const float hp = s > 0 ? a.hseq[(hr + nb) * ldo + d * H + u] : 0.0f;
        const float h = z * hp + (1.0f - z) * hh;
        gz[0] = z;
        gz[H] = r;
        gz[2 * H] = hh;
        a.qh[row * H + u] = qhv;
        a.hseq[hr * ldo + d * H + u] = h;
        if (a.hlast && a.rows.last(j, s))                     // the direction's final h: t = T - 1 forward, t = 0 reverse
            a.hlast[a.rows.out(j) * ldo + d * H + u] = h;
    }
}

// one backward step s (walked from T-1 down): dh_t = incoming + dZrec_{t+1} U^T + z_{t+1} dh_{t+1}, then the cell backward
template <bool VEC>
__global__ __launch_bounds__(256) void gru_bwd_step_kernel(const GruArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[GruStep::KCB * STEP_LDB];
    constexpr int VW = VEC ? 4 : 1;
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H3 = 3 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int prow = d == 0 ? t : t + 2;
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
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
            for (int kc = 0; kc < H; kc += GruStep::KCB) {
                const int klen = min(GruStep::KCB, H - kc), kpad = (klen + 31) & ~31;
                __syncthreads();
                stage_bwd<GruStep, VEC>(Bs, U + q * H, H, u0, kc, klen, kpad);   // gate block q: columns q H .. of U's rows
                __syncthreads();
                mma_chunk<1, VW, GruStep::PF>(acc, arow + kc, aok, klen, kpad, Bs, STEP_LDB, lane);
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

// float4 operand loads
inline bool vec_ok(int H, const void* U0, const void* U1, const void* zg, const void* hseq, const void* qh) {
    return H % 4 == 0 && aligned_to(16, U0, U1, zg, hseq, qh);
}

// the forward walk: T steps, step s over the running(s) slots still in it
template <typename Rows, typename Running>
int walk_fwd(const char* fn, const FwdArgs<Rows>& a, int T, Running running, hipStream_t st) {
    const bool vec = vec_ok(a.H, a.U[0], a.U[1], a.zg, a.hseq, a.qh);
    for (int s = 0; s < T; ++s) {
        const int n = running(s);
        const dim3 grid = step_grid(n, a.H, a.dirs);
        if (vec)
            hipLaunchKernelGGL((gru_fwd_step_kernel<true, Rows>), grid, dim3(256), 0, st, a, s, n);
        else
            hipLaunchKernelGGL((gru_fwd_step_kernel<false, Rows>), grid, dim3(256), 0, st, a, s, n);
        LBX_LAUNCH_OK_AS(fn);
    }
    return LIDBOX_OK;
}

}  // namespace

extern "C" size_t lidbox_gru_workspace(int B, int T, int H, int dirs) {
    if (B <= 0 || T < 1 || H < 1 || dirs < 1 || dirs > 2) return 0;
    return (size_t)dirs * B * H * sizeof(float);
}

extern "C" int lidbox_gru_fwd(const float* U0, const float* U1, const float* b_rec0, const float* b_rec1, int dirs, int B,
                              int T, int H, float* zg, float* hseq, float* qh, float* hlast, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 3, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(b_rec0 && (dirs == 1 || b_rec1) && zg && hseq && qh, "b_rec0 (and b_rec1 when dirs == 2), zg, hseq, qh != NULL");
    if (B == 0) return LIDBOX_OK;
    const FwdArgs<DenseRows> a{{U0, dirs == 2 ? U1 : U0}, {b_rec0, dirs == 2 ? b_rec1 : b_rec0}, zg, hseq, qh, hlast, {B, T},
                               H, dirs};
    return walk_fwd(__func__, a, T, [B](int) { return B; }, (hipStream_t)stream);
}

extern "C" int lidbox_gru_ragged_fwd(const float* U0, const float* U1, const float* b_rec0, const float* b_rec1, int dirs, int B,
                                     int H, long rows, const long* slots, const long* sorted_lengths, float* zg, float* hseq,
                                     float* qh, float* hlast, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 3, U0, U1, dirs, B, 1, H)) return e;
    LBX_ARG(b_rec0 && (dirs == 1 || b_rec1), "b_rec0 (and b_rec1 when dirs == 2) != NULL");
    if (B == 0) return LIDBOX_OK;
    if (int e = check_ragged_args(__func__, 3, dirs, B, H, rows, slots, sorted_lengths, zg, hseq, qh, (long)dirs * H)) return e;
    const FwdArgs<RaggedRows> a{{U0, dirs == 2 ? U1 : U0}, {b_rec0, dirs == 2 ? b_rec1 : b_rec0}, zg, hseq, qh, hlast,
                                {slots, rows, B}, H, dirs};
    int n = B;
    return walk_fwd(__func__, a, (int)sorted_lengths[0], [&](int s) { return n = running(sorted_lengths, n, s); },
                    (hipStream_t)stream);
}

extern "C" int lidbox_gru_bwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, const float* hseq,
                              float* qh, const float* dh_seq, long dh_batch_stride, const float* dh_last, void* workspace,
                              size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 3, U0, U1, dirs, B, T, H)) return e;
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
