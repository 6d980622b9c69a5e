// lstm_step.hip -- the Keras LSTM layer's recurrence as one fused launch per time step, gfx950.
//
// Replaces (reference file:line): tf.keras.layers.LSTM(250, return_sequences=True) inside Bidirectional(merge_mode=
// "concat") as lidbox/models/spherespeaker.py:39-41 stacks it three times.  H = 250 is past rnn.hip's resident form (U must
// fit in LDS), whose stepped form spends two GEMM launches and a cell launch per step.  Same math, buffers and gate order
// (i, f, c, o) as rnn.hip.
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
// One form, any H: the step pipeline of rnn_step.h with its LstmStep parameters (four gates: 64 columns of U per slice in
// 256-row chunks forward; backward's K = 4H runs over one contiguous row of dZ and of U, staged 16 rows of U x 1024 columns
// at a time).  Four 32-k blocks of A are fetched per trip to L2, the first trip of a chunk and the cell's own operands
// (zg's slice, c, dh, dc) ahead of the staging and the product, whose latency then covers theirs.
//
// Load paths of forward (A rows start at column d*H of a row h_row_stride wide, U's gate blocks at multiples of H): float4
// when H % 4 == 0, float2 when H is even (H = 250, the model's own width), scalar otherwise; each also needs the row
// stride to be a multiple of its width and the pointers aligned to it.  Backward's K axis is 4H long and both operands'
// rows are 4H floats apart, so its float4 path needs only 16-byte aligned pointers.
//
// The forward kernel is a template over a row map (rnn_step.h: DenseRows for the buffers above, RaggedRows for utterances of
// different lengths in one walk, lidbox_lstm_ragged_fwd; layout and walk are described there).
//
// No inter-workgroup communication, no atomics, no spin-waits: steps are ordered by the stream alone.  Every output element
// is one MFMA k-chain over its own row, in an order that depends on neither B nor the row's place in the batch, so a
// row's results are bit-identical whatever the batch.
#include <math.h>

#include "rnn_step.h"

// No a*b+c is contracted behind the source's back (as in rnn.hip): the cell is evaluated exactly as written.
#pragma clang fp contract(off)

namespace {

// backward's arguments (hseq and h_rs are forward's: unused)
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

// forward's arguments; where a row lives is the map's business (rnn_step.h)
template <typename Rows>
struct FwdArgs {
    const float* U[2];
    float* zg;
    float* hseq;
    long h_rs;
    float* cseq;
    float* hlast;                // may be NULL
    Rows rows;
    int H, dirs;
};

// one forward step s of both directions over the slots 0 .. n-1 (direction d: t = s forward, T-1-s reverse)
template <int VW, typename Rows>
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(const FwdArgs<Rows> a, int s, int n) {
    __shared__ __attribute__((aligned(16))) float Bs[LstmStep::KCF * STEP_LDF<LstmStep>];
    const int H = a.H, d = blockIdx.z, H4 = 4 * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const long nb = d == 0 ? -1 : 1;                          // the neighbour state's row: h_{t-1} (forward) / h_{t+1} (reverse)
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
    // the cell's own operands (the step's slice of zg, c_{t-1}) do not depend on the product: they are fetched first, so that
    // their trip to HBM runs under it.  Lane (c, g) holds unit u0 + c of the slots rb + 4g + i (the 16x16 C/D map:
    // col = lane & 15, row = 4 (lane >> 4) + i).
    const int u = u0 + (lane & 15);
    typename Rows::At at[4];
    float xz[4][4], cprev[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = rb + 4 * (lane >> 4) + i;
        const bool ok = u < H && j < n;
        at[i] = a.rows.at(ok ? j : 0, d, s);
        const size_t row = a.rows.frame(at[i], d, s);
        const float* gz = a.zg + row * H4 + (ok ? u : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) xz[q][i] = ok ? gz[q * H] : 0.0f;
        cprev[i] = ok && s > 0 ? a.cseq[(row + nb) * H + u] : 0.0f;
    }
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ja = rb + (lane & 15);
        const bool aok = ja < n;
        const float* arow = a.hseq + (a.rows.hrow(a.rows.at(aok ? ja : 0, d, s), d, s) + nb) * a.h_rs + d * H;
        const float* U = a.U[d];
        for (int kc = 0; kc < H; kc += LstmStep::KCF) {
            const int klen = min(LstmStep::KCF, H - kc), kpad = (klen + 31) & ~31;
            float an[LstmStep::PF][8];
            load_group<VW, LstmStep::PF>(an, arow + kc, aok, 8 * (lane >> 4), klen);   // in flight while U is staged
            __syncthreads();                                  // the previous chunk's LDS reads are done
            stage_fwd<LstmStep, VW>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<4, VW, LstmStep::PF>(acc, an, arow + kc, aok, klen, kpad, Bs, STEP_LDF<LstmStep>, lane);
        }
    }
    if (u >= H) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = rb + 4 * (lane >> 4) + i;
        if (j >= n) continue;
        const typename Rows::At ai = Rows::LOOKUP ? at[i] : a.rows.at(j, d, s);
        const size_t row = a.rows.frame(ai, d, s);
        float* gz = a.zg + row * H4 + u;
        const float ig = sigm(xz[0][i] + acc[0][i]), fg = sigm(xz[1][i] + acc[1][i]);
        const float gg = tanhf(xz[2][i] + acc[2][i]), og = sigm(xz[3][i] + acc[3][i]);
        const float c = fg * cprev[i] + ig * gg;
        gz[0] = ig;
        gz[H] = fg;
        gz[2 * H] = gg;
        gz[3 * H] = og;
        a.cseq[row * H + u] = c;
        const float h = og * tanhf(c);                        // behind the stores it does not feed: they leave under it
        a.hseq[a.rows.hrow(ai, d, s) * a.h_rs + d * H + u] = h;
        if (a.hlast && a.rows.last(j, s))                     // the direction's final h: t = T - 1 forward, t = 0 reverse
            a.hlast[a.rows.out(j) * (a.dirs * H) + d * H + u] = h;
    }
}

// one backward step s (walked from T-1 down): dh_t = incoming + dZ_{t+1} U^T, dc carried, then the cell backward
template <bool VEC>
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(const StepArgs a, int s) {
    __shared__ __attribute__((aligned(16))) float Bs[LstmStep::KCB * STEP_LDB];
    constexpr int VW = VEC ? 4 : 1;
    const int H = a.H, T = a.T, B = a.B, d = blockIdx.z, H4 = 4 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const int t = d == 0 ? s : T - 1 - s;
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
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
        for (int kc = 0; kc < H4; kc += LstmStep::KCB) {
            const int klen = min(LstmStep::KCB, H4 - kc), kpad = (klen + 31) & ~31;
            float an[LstmStep::PF][8];
            load_group<VW, LstmStep::PF>(an, arow + kc, aok, 8 * (lane >> 4), klen);
            __syncthreads();
            stage_bwd<LstmStep, VEC>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<1, VW, LstmStep::PF>(acc, an, arow + kc, aok, klen, kpad, Bs, STEP_LDB, lane);
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

// widest forward load: 4 (float4), 2 (float2) or 1 floats -- H, the row stride of hseq and the pointers all multiples of it
inline int fwd_width(int H, long h_rs, const void* U0, const void* U1, const void* hseq) {
    if (H % 4 == 0 && h_rs % 4 == 0 && aligned_to(16, U0, U1, hseq)) return 4;
    if (H % 2 == 0 && h_rs % 2 == 0 && aligned_to(8, U0, U1, hseq)) return 2;
    return 1;
}

// the forward walk: T steps, step s over the running(s) slots still in it
template <typename Rows, typename Running>
int walk_fwd(const char* fn, const FwdArgs<Rows>& a, int T, Running running, hipStream_t st) {
    const int vw = fwd_width(a.H, a.h_rs, a.U[0], a.U[1], a.hseq);
    for (int s = 0; s < T; ++s) {
        const int n = running(s);
        const dim3 grid = step_grid(n, a.H, a.dirs);
        if (vw == 4)
            hipLaunchKernelGGL((lstm_step_fwd_kernel<4, Rows>), grid, dim3(256), 0, st, a, s, n);
        else if (vw == 2)
            hipLaunchKernelGGL((lstm_step_fwd_kernel<2, Rows>), grid, dim3(256), 0, st, a, s, n);
        else
            hipLaunchKernelGGL((lstm_step_fwd_kernel<1, Rows>), grid, dim3(256), 0, st, a, s, n);
        LBX_LAUNCH_OK_AS(fn);
    }
    return LIDBOX_OK;
}

}  // namespace

extern "C" size_t lidbox_lstm_step_workspace(int B, int T, int H, int dirs) {
    if (B <= 0 || T < 1 || H < 1 || dirs < 1 || dirs > 2) return 0;
    return (size_t)dirs * B * H * sizeof(float);
}

extern "C" int lidbox_lstm_step_fwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, float* hseq,
                                    long h_row_stride, float* cseq, void* workspace, size_t workspace_bytes,
                                    lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 4, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && hseq && cseq, "zg, hseq, cseq != NULL");
    LBX_ARG(h_row_stride >= (long)dirs * H, "h_row_stride >= dirs * H");
    if (B == 0) return LIDBOX_OK;
    (void)workspace;                                          // forward carries nothing between steps
    (void)workspace_bytes;
    const FwdArgs<DenseRows> a{{U0, dirs == 2 ? U1 : U0}, zg, hseq, h_row_stride, cseq, nullptr, {B, T}, H, dirs};
    return walk_fwd(__func__, a, T, [B](int) { return B; }, (hipStream_t)stream);
}

extern "C" int lidbox_lstm_ragged_fwd(const float* U0, const float* U1, int dirs, int B, int H, long rows, const long* slots,
                                      const long* sorted_lengths, float* zg, float* hseq, long h_row_stride, float* cseq,
                                      float* hlast, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 4, U0, U1, dirs, B, 1, H)) return e;
    if (B == 0) return LIDBOX_OK;
    if (int e = check_ragged_args(__func__, 4, dirs, B, H, rows, slots, sorted_lengths, zg, hseq, cseq, h_row_stride)) return e;
    const FwdArgs<RaggedRows> a{{U0, dirs == 2 ? U1 : U0}, zg, hseq, h_row_stride, cseq, hlast, {slots, rows, B}, H, dirs};
    int n = B;
    return walk_fwd(__func__, a, (int)sorted_lengths[0], [&](int s) { return n = running(sorted_lengths, n, s); },
                    (hipStream_t)stream);
}

extern "C" int lidbox_lstm_step_bwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg,
                                    const float* cseq, const float* dh_seq, long dh_batch_stride, long dh_row_stride,
                                    const float* dh_last, void* workspace, size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 4, U0, U1, dirs, B, T, H)) return e;
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
    const bool vec = aligned_to(16, a.U[0], a.U[1], zg);
    for (int s = T - 1; s >= 0; --s) {
        if (vec)
            hipLaunchKernelGGL(lstm_step_bwd_kernel<true>, grid, dim3(256), 0, st, a, s);
        else
            hipLaunchKernelGGL(lstm_step_bwd_kernel<false>, grid, dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}
