// rnn.hip -- the Keras LSTM layer's recurrence (TF2 defaults), gfx950.
//
// Replaces (reference file:line): tf.keras.layers.LSTM as lidbox/models/lstm.py:16 and ap_lstm.py:32-35 build it
// (activation tanh, recurrent_activation sigmoid, use_bias, zero initial state, no dropout, no masking), and the
// Bidirectional(merge_mode="concat") wrapper of ap_lstm.py:33,35.
//
// Gate order in the 4H columns is i, f, c, o.  One step:
//     z = x_t W + h_{t-1} U + b,  c_t = sig(z_f) c_{t-1} + sig(z_i) tanh(z_c),  h_t = sig(z_o) tanh(c_t).
// The input projection X W + b of all B*T rows is one GEMM of the caller's (lidbox_gemm_nn, LIDBOX_EPI_BIAS), and so
// are the weight gradients and dX of backward; this file holds only what walks through time.
//
// Buffers (all fp32, see lidbox_hip.h):
//     zg    [dirs][B][T][4H]   forward: X W + b in, gate activations (i, f, tanh z_c, o) out; backward: those in, dZ out
//     hseq  [B][T+2][dirs*H]   h_t of direction d at row t+1, columns d*H..; rows 0 and T+1 stay zero, so h_{t-1} of the
//                              forward direction is row t and h_{t+1} of the reverse direction is row t+2: both are plain
//                              row descriptors for the dU = H_prev^T dZ GEMM
//     cseq  [dirs][B][T][H]    cell states
//
// Two forms, chosen by H (never by a caller option):
//   resident (H <= LSTM_RESIDENT_MAX_H): one launch per pass walks all T steps.  Workgroup = 4*RT batch rows of one
//     direction, 4*Hp threads (Hp = H rounded up to 16); grid = ceil(B / rows) x dirs.  U lives in LDS for the whole
//     launch as an [Hp][4Hp+1] zero-padded image (the odd row stride makes backward's column reads conflict-free), so
//     padded units stay exactly 0.  Thread (u, rq) owns hidden unit u of rows rq, rq+4, ..: its accumulators hold the
//     i, f, c, o pre-activations of those cells, c stays in registers, and h_{t-1} sits in a double-buffered LDS tile:
//     one barrier per step.  The next step's slice of the input projection is loaded before this step's FMAs.
//     Backward walks t downwards with the same thread layout: dh_t (incoming + recurrent) and the carried dc give dZ_t,
//     which goes to global memory and a double-buffered LDS tile; dh_rec = dZ_t U^T reads U's rows from the same image.
//   stepped (any H): per step and direction one lidbox_gemm_nn (LIDBOX_EPI_ACCUM) adds h_{t-1} U into the step's rows of
//     zg, then one cell kernel updates both directions; backward mirrors it with a cell-backward kernel and one
//     lidbox_gemm_nt per step and direction.
//
// No inter-workgroup communication of any kind.  Every sum runs in a fixed order (the resident dot products start from
// the projection and add j = 0, 1, .. in turn; no atomics), so in the resident form a row's results do not depend on B or
// on the row's position in the batch.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "rnn_cell.h"

// No a*b+c is contracted behind the source's back: whether it becomes an FMA could then depend on how the compiler
// vectorises the rows of a thread (RT), and a row's bits on B.  The FMAs that are meant are written as fmaf.
#pragma clang fp contract(off)

namespace {

constexpr int LSTM_RESIDENT_MAX_H = 80;   // LDS: U image 16 Hp^2 + 4 Hp bytes (102 720 B at Hp = 80) + backward's dZ tiles
constexpr int LSTM_LDS_BUDGET = 160 * 1024;

inline int pad16(int H) { return (H + 15) & ~15; }

struct LstmArgs {
    const float* U[2];
    float* zg;
    float* hseq;
    float* cseq;
    const float* dh_seq;
    long dh_bs;
    const float* dh_last;
    int B, T, H, Hp, dirs;
};

// resident LDS bytes: U image + the per-pass tiles (forward: h double buffer; backward: dZ double buffer)
inline size_t resident_lds(int Hp, int RT, bool bwd) {
    const size_t rw = 4 * (size_t)RT;
    const size_t u = (size_t)Hp * (4 * Hp + 1) * 4;
    const size_t tile = bwd ? 2 * rw * 4 * Hp * 4 : 2 * rw * (Hp + 4) * 4;
    return ((u + 15) & ~(size_t)15) + tile;
}

__device__ __forceinline__ void stage_u(float* Us, const float* __restrict__ U, int H, int Hp) {
    const int ldu = 4 * Hp + 1;
    for (int e = threadIdx.x; e < Hp * 4 * Hp; e += blockDim.x) {
        const int j = e / (4 * Hp), k = e - j * 4 * Hp;
        const int q = k / Hp, u = k - q * Hp;
        Us[j * ldu + k] = (j < H && u < H) ? U[(size_t)j * 4 * H + q * H + u] : 0.0f;
    }
}

template <int RT>
__global__ __launch_bounds__(4 * LSTM_RESIDENT_MAX_H) void lstm_resident_fwd_kernel(const LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, Hp = a.Hp, T = a.T, B = a.B;
    const int d = blockIdx.y;
    const int ldu = 4 * Hp + 1;
    const int ldh = Hp + 4;
    float* Us = reinterpret_cast<float*>(smem);
    float* hb = Us + (((size_t)Hp * ldu + 3) & ~(size_t)3);          // [2][4*RT][ldh]
    const int u = threadIdx.x % Hp, rq = threadIdx.x / Hp;
    const int H4 = 4 * H, ldo = a.dirs * H;

    stage_u(Us, a.U[d], H, Hp);
    for (int e = threadIdx.x; e < 2 * 4 * RT * ldh; e += blockDim.x) hb[e] = 0.0f;

    int b[RT];
    bool ok[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        b[i] = blockIdx.x * 4 * RT + rq + 4 * i;
        ok[i] = b[i] < B && u < H;
    }
    float c[RT];
    float xz[4][RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) c[i] = 0.0f;
    {
        const int t0 = d == 0 ? 0 : T - 1;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const float* src = a.zg + (((size_t)d * B + (ok[i] ? b[i] : 0)) * T + t0) * H4 + u;
#pragma unroll
            for (int q = 0; q < 4; ++q) xz[q][i] = ok[i] ? src[q * H] : 0.0f;
        }
    }
    __syncthreads();

    int p = 0;
    for (int s = 0; s < T; ++s) {
        const int t = d == 0 ? s : T - 1 - s;
        float acc[4][RT];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < RT; ++i) acc[q][i] = xz[q][i];
        if (s + 1 < T) {       // prefetch the next step's projection while this step's FMAs run
            const int tn = d == 0 ? s + 1 : T - 2 - s;
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                const float* src = a.zg + (((size_t)d * B + (ok[i] ? b[i] : 0)) * T + tn) * H4 + u;
#pragma unroll
                for (int q = 0; q < 4; ++q) xz[q][i] = ok[i] ? src[q * H] : 0.0f;
            }
        }
        const float* hp = hb + p * 4 * RT * ldh;
        for (int j = 0; j < Hp; j += 4) {
            float4 h4[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) h4[i] = *reinterpret_cast<const float4*>(hp + (rq + 4 * i) * ldh + j);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float* ur = Us + (j + jj) * ldu + u;
                float w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] = ur[q * Hp];
#pragma unroll
                for (int i = 0; i < RT; ++i) {
                    const float hv = jj == 0 ? h4[i].x : jj == 1 ? h4[i].y : jj == 2 ? h4[i].z : h4[i].w;
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q][i] = fmaf(hv, w[q], acc[q][i]);
                }
            }
        }
        float* hn = hb + (p ^ 1) * 4 * RT * ldh;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]), gg = tanhf(acc[2][i]), og = sigm(acc[3][i]);
            c[i] = fg * c[i] + ig * gg;
            const float h = og * tanhf(c[i]);
            hn[(rq + 4 * i) * ldh + u] = h;          // padded units / rows: exactly 0
            if (ok[i]) {
                float* gz = a.zg + (((size_t)d * B + b[i]) * T + t) * H4 + u;
                gz[0] = ig;
                gz[H] = fg;
                gz[2 * H] = gg;
                gz[3 * H] = og;
                a.cseq[(((size_t)d * B + b[i]) * T + t) * H + u] = c[i];
                a.hseq[((size_t)b[i] * (T + 2) + t + 1) * ldo + d * H + u] = h;
            }
        }
        __syncthreads();
        p ^= 1;
    }
}

template <int RT>
__global__ __launch_bounds__(4 * LSTM_RESIDENT_MAX_H) void lstm_resident_bwd_kernel(const LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int H = a.H, Hp = a.Hp, T = a.T, B = a.B;
    const int d = blockIdx.y;
    const int ldu = 4 * Hp + 1;
    const int ldz = 4 * Hp;
    float* Us = reinterpret_cast<float*>(smem);
    float* zb = Us + (((size_t)Hp * ldu + 3) & ~(size_t)3);          // [2][4*RT][ldz]
    const int u = threadIdx.x % Hp, rq = threadIdx.x / Hp;
    const int H4 = 4 * H, ldo = a.dirs * H;

    stage_u(Us, a.U[d], H, Hp);

    int b[RT];
    bool ok[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        b[i] = blockIdx.x * 4 * RT + rq + 4 * i;
        ok[i] = b[i] < B && u < H;
    }
    float dc[RT], dhr[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) dc[i] = dhr[i] = 0.0f;
    __syncthreads();

    // per-step operands of (row i): gates, c_t, c_{t-1}, incoming dh -- loaded one step ahead
    float g[4][RT], ct[RT], cp[RT], dhi[RT];
    auto load = [&](int s) {
        const int t = d == 0 ? s : T - 1 - s;
        const int tp = d == 0 ? t - 1 : t + 1;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const size_t row = ((size_t)d * B + (ok[i] ? b[i] : 0)) * T;
            const float* gz = a.zg + (row + t) * H4 + u;
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q][i] = ok[i] ? gz[q * H] : 0.0f;
            ct[i] = ok[i] ? a.cseq[(row + t) * H + u] : 0.0f;
            cp[i] = ok[i] && s > 0 ? a.cseq[(row + tp) * H + u] : 0.0f;
            float v = 0.0f;
            if (ok[i] && a.dh_seq) v = a.dh_seq[(size_t)b[i] * a.dh_bs + (size_t)t * ldo + d * H + u];
            if (ok[i] && a.dh_last && s == T - 1) v += a.dh_last[(size_t)b[i] * ldo + d * H + u];
            dhi[i] = v;
        }
    };
    load(T - 1);

    int p = 0;
    for (int s = T - 1; s >= 0; --s) {
        const int t = d == 0 ? s : T - 1 - s;
        float* zt = zb + p * 4 * RT * ldz;
        float dz[4][RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            float v[4] = {g[0][i], g[1][i], g[2][i], g[3][i]};
            cell_bwd(v, ct[i], cp[i], dhi[i] + dhr[i], dc[i]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dz[q][i] = ok[i] ? v[q] : 0.0f;
                zt[(rq + 4 * i) * ldz + q * Hp + u] = dz[q][i];
            }
        }
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            if (ok[i]) {
                float* gz = a.zg + (((size_t)d * B + b[i]) * T + t) * H4 + u;
#pragma unroll
                for (int q = 0; q < 4; ++q) gz[q * H] = dz[q][i];
            }
        }
        if (s > 0) load(s - 1);
        __syncthreads();
        // dh_rec = dZ_t U^T for the next (earlier) step: k = 0, 1, .., 4Hp-1 in order
#pragma unroll
        for (int i = 0; i < RT; ++i) dhr[i] = 0.0f;
        const float* ur = Us + u * ldu;
        for (int k = 0; k < ldz; k += 4) {
            float4 z4[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) z4[i] = *reinterpret_cast<const float4*>(zt + (rq + 4 * i) * ldz + k);
            const float w0 = ur[k], w1 = ur[k + 1], w2 = ur[k + 2], w3 = ur[k + 3];
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                float v = dhr[i];
                v = fmaf(z4[i].x, w0, v);
                v = fmaf(z4[i].y, w1, v);
                v = fmaf(z4[i].z, w2, v);
                v = fmaf(z4[i].w, w3, v);
                dhr[i] = v;
            }
        }
        p ^= 1;
    }
}

// ---- stepped form: cell kernels, one thread per (direction, row, unit)
__global__ __launch_bounds__(256) void lstm_cell_fwd_kernel(const LstmArgs a, int s) {
    const long n = (long)a.dirs * a.B * a.H;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int H = a.H, T = a.T, B = a.B;
    const int u = (int)(e % H);
    const long r = e / H;
    const int b = (int)(r % B), d = (int)(r / B);
    const int t = d == 0 ? s : T - 1 - s;
    const int tp = d == 0 ? t - 1 : t + 1;
    const size_t row = ((size_t)d * B + b) * T;
    float* gz = a.zg + (row + t) * 4 * H + u;
    const float ig = sigm(gz[0]), fg = sigm(gz[H]), gg = tanhf(gz[2 * H]), og = sigm(gz[3 * H]);
    const float cprev = s > 0 ? a.cseq[(row + tp) * H + u] : 0.0f;
    const float c = fg * cprev + ig * gg;
    gz[0] = ig;
    gz[H] = fg;
    gz[2 * H] = gg;
    gz[3 * H] = og;
    a.cseq[(row + t) * H + u] = c;
    a.hseq[((size_t)b * (T + 2) + t + 1) * a.dirs * H + d * H + u] = og * tanhf(c);
}

// dc: [dirs][B][H] carried cell gradient, dhr: [dirs][B][H] recurrent dh of the previous (later) step
__global__ __launch_bounds__(256) void lstm_cell_bwd_kernel(const LstmArgs a, int s, float* dc, const float* dhr) {
    const long n = (long)a.dirs * a.B * a.H;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int H = a.H, T = a.T, B = a.B, ldo = a.dirs * H;
    const int u = (int)(e % H);
    const long r = e / H;
    const int b = (int)(r % B), d = (int)(r / B);
    const int t = d == 0 ? s : T - 1 - s;
    const int tp = d == 0 ? t - 1 : t + 1;
    const size_t row = ((size_t)d * B + b) * T;
    float* gz = a.zg + (row + t) * 4 * H + u;
    float v[4] = {gz[0], gz[H], gz[2 * H], gz[3 * H]};
    float dh = 0.0f;
    if (a.dh_seq) dh = a.dh_seq[(size_t)b * a.dh_bs + (size_t)t * ldo + d * H + u];
    if (a.dh_last && s == T - 1) dh += a.dh_last[(size_t)b * ldo + d * H + u];
    float dcv = 0.0f;
    if (s < T - 1) {
        dh += dhr[e];
        dcv = dc[e];
    }
    cell_bwd(v, a.cseq[(row + t) * H + u], s > 0 ? a.cseq[(row + tp) * H + u] : 0.0f, dh, dcv);
    gz[0] = v[0];
    gz[H] = v[1];
    gz[2 * H] = v[2];
    gz[3 * H] = v[3];
    dc[e] = dcv;
}

// ---- sequence average pooling with a scale: out[b, c] = alpha * mean_t x[b, t, c] (ap_lstm.py:37-41)
__global__ __launch_bounds__(256) void seq_avg_pool_fwd_kernel(const float* __restrict__ x, int B, int T, int C, long bs,
                                                               long rs, float alpha, float* __restrict__ out, long ldo) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)B * C) return;
    const int b = (int)(e / C), c = (int)(e % C);
    const float* p = x + (size_t)b * bs + c;
    float s = 0.0f;
    for (int t = 0; t < T; ++t) s += p[(size_t)t * rs];
    out[(size_t)b * ldo + c] = alpha * (s / (float)T);
}

__global__ __launch_bounds__(256) void seq_avg_pool_bwd_kernel(const float* __restrict__ dout, long ldo, int B, int T, int C,
                                                               float alpha, float* __restrict__ dx, long bs, long rs,
                                                               int accumulate) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)B * T * C) return;
    const int c = (int)(e % C);
    const long bt = e / C;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const float g = alpha * dout[(size_t)b * ldo + c] / (float)T;
    float* p = dx + (size_t)b * bs + (size_t)t * rs + c;
    *p = accumulate ? *p + g : g;
}

// the same over utterances of different lengths, forward only: out[b, c] (ldo floats between rows) = alpha * mean over the
// lengths[b] rows from row first_rows[b] of x, in the summation order of ragged.hip's pools for EVERY length: 256 threads =
// 16 channels x 16 time groups; per group the rows g, g + 16, .. in order, then the 16 groups in order, / T, * alpha.
// Grid (ceil(C / 16), utterance blocks), utterances grid-strided.
__global__ __launch_bounds__(256) void seq_avg_pool_ragged_kernel(const float* __restrict__ x, long rs,
                                                                  const long* __restrict__ first_rows,
                                                                  const long* __restrict__ lengths, long B, int C, float alpha,
                                                                  float* __restrict__ out, long ldo) {
    __shared__ float red[16][17];
    const int cg = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + cg;
    const bool active = c < C;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        const long T = lengths[b];
        const float* xp = x + first_rows[b] * rs + c;
        float sum = 0.f;
        if (active)
            for (long t = g; t < T; t += 16) sum += xp[t * rs];
        red[g][cg] = sum;
        __syncthreads();
        if (active && g == 0) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) m += red[k][cg];
            out[b * ldo + c] = alpha * (m / (float)T);
        }
        __syncthreads();                                     // the next utterance writes red
    }
}

int pick_rt(int B, int dirs) {
    // fewest rows per workgroup that still fit one wave of workgroups on the 256 CUs: the walk through time is latency-bound
    for (int rt = 1; rt < 4; rt *= 2)
        if (lbx_cdiv(B, 4 * rt) * dirs <= 256) return rt;
    return 4;
}

int check_common(const char* fn, const float* U0, const float* U1, int dirs, int B, int T, int H) {
    if (!(dirs == 1 || dirs == 2) || !U0 || (dirs == 2 && !U1) || B < 0 || T < 1 || H < 1) {
        lidbox_set_error("%s: invalid argument: dirs in {1, 2}, U0 (and U1 when dirs == 2) != NULL, B >= 0, T >= 1, H >= 1", fn);
        return LIDBOX_E_INVALID;
    }
    if ((long)B > 65535L * 16 || H > 16384) {
        lidbox_set_error("%s: invalid argument: B <= 1048560, H <= 16384", fn);
        return LIDBOX_E_INVALID;
    }
    return LIDBOX_OK;
}

size_t stepped_ws(int B, int H, int dirs) {
    const size_t carry = 2 * (size_t)dirs * B * H * 4;
    const size_t g = std::max(lidbox_gemm_rows_workspace(B, 4 * H, H), lidbox_gemm_rows_workspace(B, H, 4 * H));
    return ((carry + 255) & ~(size_t)255) + g;
}

template <typename K>
hipError_t allow_lds(K kernel, size_t bytes) {
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               LSTM_LDS_BUDGET);
}

template <int RT>
int launch_resident(const LstmArgs& a, bool bwd, hipStream_t st) {
    const size_t lds = resident_lds(a.Hp, RT, bwd);
    const dim3 grid((unsigned)lbx_cdiv(a.B, 4 * RT), (unsigned)a.dirs), block((unsigned)(4 * a.Hp));
    if (bwd) {
        static const hipError_t raised = allow_lds(lstm_resident_bwd_kernel<RT>, LSTM_LDS_BUDGET);
        if (raised != hipSuccess) { lidbox_set_error("lidbox_lstm_bwd: hipFuncSetAttribute: %s", hipGetErrorString(raised)); return LIDBOX_E_LAUNCH; }
        hipLaunchKernelGGL(lstm_resident_bwd_kernel<RT>, grid, block, lds, st, a);
    } else {
        static const hipError_t raised = allow_lds(lstm_resident_fwd_kernel<RT>, LSTM_LDS_BUDGET);
        if (raised != hipSuccess) { lidbox_set_error("lidbox_lstm_fwd: hipFuncSetAttribute: %s", hipGetErrorString(raised)); return LIDBOX_E_LAUNCH; }
        hipLaunchKernelGGL(lstm_resident_fwd_kernel<RT>, grid, block, lds, st, a);
    }
    return LIDBOX_OK;
}

int run_resident(const LstmArgs& a, bool bwd, hipStream_t st) {
    switch (pick_rt(a.B, a.dirs)) {
        case 1: return launch_resident<1>(a, bwd, st);
        case 2: return launch_resident<2>(a, bwd, st);
        default: return launch_resident<4>(a, bwd, st);
    }
}

lidbox_rows_t step_rows(const float* base, long batch_stride, int B) {
    lidbox_rows_t r;
    r.base = base;
    r.batch_stride = batch_stride;
    r.row_stride = 0;
    r.batch = B;
    r.rows_per_batch = 1;
    return r;
}

}  // namespace

extern "C" int lidbox_lstm_resident_ok(int H) {
    return H >= 1 && H <= LSTM_RESIDENT_MAX_H && resident_lds(pad16(H), 4, true) <= (size_t)LSTM_LDS_BUDGET ? 1 : 0;
}

extern "C" size_t lidbox_lstm_workspace(int B, int T, int H, int dirs) {
    if (B <= 0 || T < 1 || H < 1 || dirs < 1 || dirs > 2 || lidbox_lstm_resident_ok(H)) return 0;
    return stepped_ws(B, H, dirs);
}

extern "C" int lidbox_lstm_fwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, float* hseq,
                               float* cseq, void* workspace, size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && hseq && cseq, "zg, hseq, cseq != NULL");
    if (B == 0) return LIDBOX_OK;
    LstmArgs a{{U0, dirs == 2 ? U1 : U0}, zg, hseq, cseq, nullptr, 0, nullptr, B, T, H, pad16(H), dirs};
    hipStream_t st = (hipStream_t)stream;
    if (lidbox_lstm_resident_ok(H)) {
        if (int e = run_resident(a, false, st)) return e;
        LBX_LAUNCH_OK();
        return LIDBOX_OK;
    }
    const size_t need = stepped_ws(B, H, dirs);
    LBX_ARG(workspace_bytes >= need && (workspace || need == 0), "workspace >= lidbox_lstm_workspace() bytes");
    const size_t carry = ((2 * (size_t)dirs * B * H * 4 + 255) & ~(size_t)255);
    void* gws = (char*)workspace + carry;
    const size_t gws_n = workspace_bytes - carry;
    const long ldo = (long)dirs * H;
    const unsigned nblk = (unsigned)lbx_cdiv((long)dirs * B * H, 256);
    for (int s = 0; s < T; ++s) {
        if (s > 0) {
            for (int d = 0; d < dirs; ++d) {
                const int t = d == 0 ? s : T - 1 - s;
                const int prow = d == 0 ? t : t + 2;             // row of h_{t-1} (forward) / h_{t+1} (reverse)
                lidbox_rows_t A = step_rows(hseq + (size_t)prow * ldo + d * H, (long)(T + 2) * ldo, B);
                lidbox_rows_t Cr = step_rows(zg + ((size_t)d * B * T + t) * 4 * H, (long)T * 4 * H, B);
                lidbox_rows_out_t C{const_cast<float*>(Cr.base), Cr.batch_stride, 0, B, 1};
                if (int e = lidbox_gemm_nn(A, a.U[d], 4 * H, C, H, 4 * H, LIDBOX_EPI_ACCUM, nullptr, gws, gws_n, stream)) return e;
            }
        }
        hipLaunchKernelGGL(lstm_cell_fwd_kernel, dim3(nblk), dim3(256), 0, st, a, s);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_lstm_bwd(const float* U0, const float* U1, int dirs, int B, int T, int H, float* zg, const float* cseq,
                               const float* dh_seq, long dh_batch_stride, const float* dh_last, void* workspace,
                               size_t workspace_bytes, lidbox_stream_t stream) {
    if (int e = check_common(__func__, U0, U1, dirs, B, T, H)) return e;
    LBX_ARG(zg && cseq && (dh_seq || dh_last), "zg, cseq != NULL; dh_seq or dh_last != NULL");
    LBX_ARG(!dh_seq || dh_batch_stride >= (long)T * dirs * H, "dh_batch_stride >= T * dirs * H");
    if (B == 0) return LIDBOX_OK;
    LstmArgs a{{U0, dirs == 2 ? U1 : U0}, zg, nullptr, const_cast<float*>(cseq), dh_seq, dh_batch_stride, dh_last,
               B, T, H, pad16(H), dirs};
    hipStream_t st = (hipStream_t)stream;
    if (lidbox_lstm_resident_ok(H)) {
        if (int e = run_resident(a, true, st)) return e;
        LBX_LAUNCH_OK();
        return LIDBOX_OK;
    }
    const size_t need = stepped_ws(B, H, dirs);
    LBX_ARG(workspace_bytes >= need && workspace, "workspace >= lidbox_lstm_workspace() bytes");
    float* dc = (float*)workspace;
    float* dhr = dc + (size_t)dirs * B * H;
    const size_t carry = ((2 * (size_t)dirs * B * H * 4 + 255) & ~(size_t)255);
    void* gws = (char*)workspace + carry;
    const size_t gws_n = workspace_bytes - carry;
    const unsigned nblk = (unsigned)lbx_cdiv((long)dirs * B * H, 256);
    for (int s = T - 1; s >= 0; --s) {
        hipLaunchKernelGGL(lstm_cell_bwd_kernel, dim3(nblk), dim3(256), 0, st, a, s, dc, dhr);
        LBX_LAUNCH_OK();
        if (s == 0) break;
        for (int d = 0; d < dirs; ++d) {
            const int t = d == 0 ? s : T - 1 - s;
            lidbox_rows_t A = step_rows(zg + ((size_t)d * B * T + t) * 4 * H, (long)T * 4 * H, B);
            lidbox_rows_out_t C{dhr + (size_t)d * B * H, 0, H, 1, B};
            if (int e = lidbox_gemm_nt(A, a.U[d], 4 * H, C, 4 * H, H, LIDBOX_EPI_NONE, nullptr, gws, gws_n, stream)) return e;
        }
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_seq_avg_pool_fwd(const float* x, int B, int T, int C, long batch_stride, long row_stride, float alpha,
                                       float* out, long ldo, lidbox_stream_t stream) {
    LBX_ARG(x && out && B >= 0 && T >= 1 && C >= 1 && ldo >= C, "x, out != NULL; T, C >= 1; ldo >= C");
    if (B == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(seq_avg_pool_fwd_kernel, dim3((unsigned)lbx_cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream,
                       x, B, T, C, batch_stride, row_stride, alpha, out, ldo);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_seq_avg_pool_ragged_fwd(const float* x, long row_stride, const long* first_rows, const long* lengths, long B,
                                              int C, float alpha, float* out, long ldo, lidbox_stream_t stream) {
    LBX_ARG(x && first_rows && lengths && out, "x, first_rows, lengths, out != NULL");
    LBX_ARG(B >= 0 && C >= 1 && row_stride >= C && ldo >= C, "B >= 0; C >= 1; row_stride >= C; ldo >= C");
    if (B == 0) return LIDBOX_OK;
    const unsigned by = (unsigned)(B > 8192 ? 8192 : B);      // the loop over utterances strides past it
    hipLaunchKernelGGL(seq_avg_pool_ragged_kernel, dim3((unsigned)lbx_cdiv(C, 16), by), dim3(256), 0, (hipStream_t)stream, x,
                       row_stride, first_rows, lengths, B, C, alpha, out, ldo);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_seq_avg_pool_bwd(const float* dout, long ldo, int B, int T, int C, float alpha, float* dx,
                                       long batch_stride, long row_stride, int accumulate, lidbox_stream_t stream) {
    LBX_ARG(dout && dx && B >= 0 && T >= 1 && C >= 1 && ldo >= C, "dout, dx != NULL; T, C >= 1; ldo >= C");
    if (B == 0) return LIDBOX_OK;
    hipLaunchKernelGGL(seq_avg_pool_bwd_kernel, dim3((unsigned)lbx_cdiv((long)B * T * C, 256)), dim3(256), 0,
                       (hipStream_t)stream, dout, ldo, B, T, C, alpha, dx, batch_stride, row_stride, accumulate ? 1 : 0);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}
