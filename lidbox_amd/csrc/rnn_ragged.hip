// rnn_ragged.hip -- the recurrences of gru.hip and lstm_step.hip walked over utterances of DIFFERENT lengths in one pass,
// forward only (inference), gfx950.  No reference counterpart: tf.data batches need one shape, and the Keras layers run without
// masking, so a padded batch starts every reverse direction inside the padding.
//
// Layout (the dense [B][T+2] convention with a per-utterance T; lidbox_hip.h has the buffers): utterance b with T_b frames owns
// the rows seg[b] .. seg[b+1] = seg[b] + T_b + 2 of every per-frame buffer of the layer.  Row seg[b] is a pad row, frame t sits at
// row seg[b] + 1 + t, row seg[b+1] - 1 is a pad row.  One row index serves hseq [rows][h_row_stride], zg [dirs][rows][NG H] and
// cseq / qh [dirs][rows][H], so a layer's input projection is ONE GEMM over all rows (the pad rows of zg receive the bias and are
// never read) and no utterance is ever moved in memory.
//
// The walk: step s = 0 .. T_max - 1 is one launch for both directions, over the n_s = #{b : T_b > s} utterances still running.
// Slot j of a step is the j-th longest utterance (stable sort by length, descending), so the running ones are the slots
// 0 .. n_s - 1 of a device table `slots` [3][B] = (first row seg[b], length T_b, utterance index b).  Grid = ceil(n_s / 64) x
// ceil(H / 16) x dirs: later steps launch fewer row tiles.  Direction 0 works on t = s, direction 1 on t = T_b - 1 - s; the
// neighbour state is the hseq row in front of (direction 0) resp. behind (direction 1) the frame's own row, inside the
// utterance's own segment.  The first step of a direction skips the product (h_{-1} = 0) and reads no neighbour.
//
// Arithmetic: the step pipeline of rnn_step.h with the parameters, chunk order and cell code of the dense kernels -- only where
// a row lives differs.  Every output element is one MFMA k-chain over its own row, so every utterance's gates, c / qh, h and
// hlast are bit for bit what lidbox_lstm_step_fwd / lidbox_gru_fwd give it at B = 1, T = T_b, whatever its neighbours, its
// place in the batch and its slot, and the 16-, 8- and 4-byte load paths agree bit for bit.
//
// No inter-workgroup communication, no atomics, no spin-waits: steps are ordered by the stream alone.
#include <math.h>
#include <stdint.h>

#include "rnn_step.h"

// No a*b+c is contracted behind the source's back (as in the dense kernels): the cell is evaluated exactly as written.
#pragma clang fp contract(off)

namespace {

struct RaggedArgs {
    const float* U[2];
    const float* brec[2];        // GRU only
    float* zg;
    float* hseq;
    long h_rs;
    float* aux;                  // cseq (LSTM) / qh (GRU)
    float* hlast;
    const long* slots;           // [3][B]: first row, length, utterance index of slot j
    long rows;                   // rows per direction of zg and aux
    int B, H, dirs;
};

// the row of the frame slot j works on at step s of direction d
__device__ __forceinline__ long frame_row(const RaggedArgs& a, int j, int d, int s) {
    const long first = a.slots[j];
    return first + 1 + (d == 0 ? (long)s : a.slots[a.B + j] - 1 - s);
}

// one forward step s of both directions over the slots 0 .. n-1; lstm_step_fwd_kernel with a row looked up per slot
template <int VW>
__global__ __launch_bounds__(256) void lstm_ragged_fwd_kernel(const RaggedArgs a, int s, int n) {
    __shared__ __attribute__((aligned(16))) float Bs[LstmStep::KCF * STEP_LDF<LstmStep>];
    const int H = a.H, d = blockIdx.z, H4 = 4 * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const long nb = d == 0 ? -1 : 1;                          // the neighbour state's row: h_{t-1} (forward) / h_{t+1} (reverse)
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
    // the cell's own operands are fetched ahead of the product, as in the dense kernel.  Lane (c, g) holds unit u0 + c of the
    // slots rb + 4g + i.
    const int u = u0 + (lane & 15);
    long fr[4];
    float xz[4][4], cprev[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = rb + 4 * (lane >> 4) + i;
        const bool ok = u < H && j < n;
        fr[i] = ok ? frame_row(a, j, d, s) : 1;
        const size_t row = (size_t)d * a.rows + fr[i];
        const float* gz = a.zg + row * H4 + (ok ? u : 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) xz[q][i] = ok ? gz[q * H] : 0.0f;
        cprev[i] = ok && s > 0 ? a.aux[(row + nb) * H + u] : 0.0f;
    }
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ja = rb + (lane & 15);
        const bool aok = ja < n;
        const long ra = aok ? frame_row(a, ja, d, s) : 1;
        const float* arow = a.hseq + (size_t)(ra + nb) * a.h_rs + d * H;
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
        const size_t row = (size_t)d * a.rows + fr[i];
        float* gz = a.zg + row * H4 + u;
        const float ig = sigm(xz[0][i] + acc[0][i]), fg = sigm(xz[1][i] + acc[1][i]);
        const float gg = tanhf(xz[2][i] + acc[2][i]), og = sigm(xz[3][i] + acc[3][i]);
        const float c = fg * cprev[i] + ig * gg;
        const float h = og * tanhf(c);
        gz[0] = ig;
        gz[H] = fg;
        gz[2 * H] = gg;
        gz[3 * H] = og;
        a.aux[row * H + u] = c;
        a.hseq[(size_t)fr[i] * a.h_rs + d * H + u] = h;
        if (a.hlast && a.slots[a.B + j] == s + 1)             // the direction's final h: t = T_b - 1 forward, t = 0 reverse
            a.hlast[(size_t)a.slots[2 * a.B + j] * (a.dirs * H) + d * H + u] = h;
    }
}

// the same for the GRU: gru_fwd_step_kernel with a row looked up per slot; hseq rows are dirs * H wide
template <bool VEC>
__global__ __launch_bounds__(256) void gru_ragged_fwd_kernel(const RaggedArgs a, int s, int n) {
    __shared__ __attribute__((aligned(16))) float Bs[GruStep::KCF * STEP_LDF<GruStep>];
    constexpr int VW = VEC ? 4 : 1;
    const int H = a.H, d = blockIdx.z, H3 = 3 * H, ldo = a.dirs * H;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int u0 = blockIdx.y * STEP_UNITS;
    const long nb = d == 0 ? -1 : 1;
    const int rb = blockIdx.x * STEP_ROWS + w * 16;
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                              // h_{-1} = 0: the first step's product is skipped
        const int ja = rb + (lane & 15);
        const bool aok = ja < n;
        const long ra = aok ? frame_row(a, ja, d, s) : 1;
        const float* arow = a.hseq + (size_t)(ra + nb) * ldo + d * H;
        const float* U = a.U[d];
        for (int kc = 0; kc < H; kc += GruStep::KCF) {
            const int klen = min(GruStep::KCF, H - kc), kpad = (klen + 31) & ~31;
            __syncthreads();                                  // the previous chunk's LDS reads are done
            stage_fwd<GruStep, VW>(Bs, U, H, u0, kc, klen, kpad);
            __syncthreads();
            mma_chunk<3, VW, GruStep::PF>(acc, arow + kc, aok, klen, kpad, Bs, STEP_LDF<GruStep>, lane);
        }
    }
    const int u = u0 + (lane & 15);
    if (u >= H) return;
    const float* br = a.brec[d];
    const float bz = br[u], brr = br[H + u], bh = br[2 * H + u];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = rb + 4 * (lane >> 4) + i;
        if (j >= n) continue;
        const long fr = frame_row(a, j, d, s);
        const size_t row = (size_t)d * a.rows + fr;
        float* gz = a.zg + row * H3 + u;
        const float qz = acc[0][i] + bz, qr = acc[1][i] + brr, qhv = acc[2][i] + bh;
        const float z = sigm(gz[0] + qz), r = sigm(gz[H] + qr);
        const float hh = tanhf(gz[2 * H] + r * qhv);
        const float hp = s > 0 ? a.hseq[(size_t)(fr + nb) * ldo + d * H + u] : 0.0f;
        const float h = z * hp + (1.0f - z) * hh;
        gz[0] = z;
        gz[H] = r;
        gz[2 * H] = hh;
        a.aux[row * H + u] = qhv;
        a.hseq[(size_t)fr * ldo + d * H + u] = h;
        if (a.hlast && a.slots[a.B + j] == s + 1)
            a.hlast[(size_t)a.slots[2 * a.B + j] * ldo + d * H + u] = h;
    }
}

// out[b, c] (ldo floats between rows) = alpha * mean over the lengths[b] rows from row first_rows[b] of x, in the summation
// order of ragged.hip's pools for EVERY length: 256 threads = 16 channels x 16 time groups; per group the rows g, g + 16, ..
// in order, then the 16 groups in order, / T, * alpha.  Grid (ceil(C / 16), utterance blocks), utterances grid-strided.
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

// what both walks ask of their arguments beyond check_step_args (B >= 1 here); ng: gates
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

// widest LSTM load, as lstm_step.hip's fwd_width
inline int lstm_width(int H, long h_rs, const void* U0, const void* U1, const void* hseq) {
    if (H % 4 == 0 && h_rs % 4 == 0 && aligned_to(16, U0, U1, hseq)) return 4;
    if (H % 2 == 0 && h_rs % 2 == 0 && aligned_to(8, U0, U1, hseq)) return 2;
    return 1;
}

// the slots still running at step s: sorted_lengths is non-increasing, n only shrinks
inline int running(const long* sorted_lengths, int n, int s) {
    while (n > 0 && sorted_lengths[n - 1] <= s) --n;
    return n;
}

}  // namespace

extern "C" int lidbox_lstm_ragged_fwd(const float* U0, const float* U1, int dirs, int B, int H, long rows, const long* slots,
                                      const long* sorted_lengths, float* zg, float* hseq, long h_row_stride, float* cseq,
                                      float* hlast, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 4, U0, U1, dirs, B, 1, H)) return e;
    if (B == 0) return LIDBOX_OK;
    if (int e = check_ragged_args(__func__, 4, dirs, B, H, rows, slots, sorted_lengths, zg, hseq, cseq, h_row_stride)) return e;
    RaggedArgs a{{U0, dirs == 2 ? U1 : U0}, {nullptr, nullptr}, zg, hseq, h_row_stride, cseq, hlast, slots, rows, B, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const int vw = lstm_width(H, h_row_stride, a.U[0], a.U[1], hseq);
    const int T = (int)sorted_lengths[0];
    int n = B;
    for (int s = 0; s < T; ++s) {
        n = running(sorted_lengths, n, s);
        const dim3 grid = step_grid(n, H, dirs);
        if (vw == 4)
            hipLaunchKernelGGL(lstm_ragged_fwd_kernel<4>, grid, dim3(256), 0, st, a, s, n);
        else if (vw == 2)
            hipLaunchKernelGGL(lstm_ragged_fwd_kernel<2>, grid, dim3(256), 0, st, a, s, n);
        else
            hipLaunchKernelGGL(lstm_ragged_fwd_kernel<1>, grid, dim3(256), 0, st, a, s, n);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_gru_ragged_fwd(const float* U0, const float* U1, const float* b_rec0, const float* b_rec1, int dirs, int B,
                                     int H, long rows, const long* slots, const long* sorted_lengths, float* zg, float* hseq,
                                     float* qh, float* hlast, lidbox_stream_t stream) {
    if (int e = check_step_args(__func__, 3, U0, U1, dirs, B, 1, H)) return e;
    LBX_ARG(b_rec0 && (dirs == 1 || b_rec1), "b_rec0 (and b_rec1 when dirs == 2) != NULL");
    if (B == 0) return LIDBOX_OK;
    if (int e = check_ragged_args(__func__, 3, dirs, B, H, rows, slots, sorted_lengths, zg, hseq, qh, (long)dirs * H)) return e;
    RaggedArgs a{{U0, dirs == 2 ? U1 : U0}, {b_rec0, dirs == 2 ? b_rec1 : b_rec0}, zg, hseq, (long)dirs * H, qh, hlast, slots,
                 rows, B, H, dirs};
    hipStream_t st = (hipStream_t)stream;
    const bool vec = H % 4 == 0 && aligned_to(16, a.U[0], a.U[1], zg, hseq, qh);   // as gru.hip's vec_ok
    const int T = (int)sorted_lengths[0];
    int n = B;
    for (int s = 0; s < T; ++s) {
        n = running(sorted_lengths, n, s);
        const dim3 grid = step_grid(n, H, dirs);
        if (vec)
            hipLaunchKernelGGL(gru_ragged_fwd_kernel<true>, grid, dim3(256), 0, st, a, s, n);
        else
            hipLaunchKernelGGL(gru_ragged_fwd_kernel<false>, grid, dim3(256), 0, st, a, s, n);
        LBX_LAUNCH_OK();
    }
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
