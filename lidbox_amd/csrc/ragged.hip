// ragged.hip -- the device kernels of the ragged model pass (models/ragged.py, SequentialTDNN.forward_ragged): utterances of
// different lengths concatenated into ONE row buffer per level, so that a `batch = 1` rows descriptor walks all of them and every
// Conv1D stays one call of the existing GEMMs (gfx950).
//
//   pack_rows_kernel     [total_T, C] frames -> the level-0 buffer: per segment `pad` zero rows, the frames, zeros up to the next
//                        segment; plus zero rows behind the last segment
//   zero_rows_kernel     the first `pad` rows of every segment back to zero (the GEMM in front wrote relu(bias)-like values there)
//   pool_ragged_kernel   GlobalMeanStddevPooling1D / GlobalAveragePooling1D per utterance, with the arithmetic of nnops.hip's
//                        pool_fwd_kernel for EVERY length: 16 time groups, combined through LDS in a fixed order
//
// All offsets are int64 device arrays and every loop over utterances is grid-strided: B has no 65 535 cap.
#include <float.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr float STDDEV_SQRT_MIN_CLIP = 1e-10f;    // xvector.py:22 (as nnops.hip)
constexpr unsigned MAX_GRID = 8192;               // blocks along the utterance axis: the loops stride past it

// V floats: one 16-byte access (V = 4, aligned by the launcher's test) or one scalar access
template <int V> struct vec_t;
template <> struct vec_t<4> { typedef float4 type; };
template <> struct vec_t<1> { typedef float type; };
template <int V> __device__ __forceinline__ typename vec_t<V>::type vec_zero();
template <> __device__ __forceinline__ float4 vec_zero<4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
template <> __device__ __forceinline__ float vec_zero<1>() { return 0.f; }

// One workgroup per segment (grid-strided); segment B is the tail: `tail_rows` zero rows behind the last segment.  Every row of
// every segment is written, and nothing outside seg_offsets[0] .. seg_offsets[B] + tail_rows: the frames are clamped to what the
// segment holds behind its pad.  CV = C / V.
template <int V>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ src, const long* __restrict__ src_offsets,
                                                        float* __restrict__ dst, const long* __restrict__ seg_offsets, long B,
                                                        long CV, long pad, long tail_rows) {
    typedef typename vec_t<V>::type T;
    const T* s = reinterpret_cast<const T*>(src);
    T* d = reinterpret_cast<T*>(dst);
    for (long b = blockIdx.x; b <= B; b += gridDim.x) {
        const long row0 = seg_offsets[b];
        long rows, frames, src0, p;
        if (b < B) {
            rows = seg_offsets[b + 1] - row0;
            src0 = src_offsets[b];
            frames = src_offsets[b + 1] - src0;
            p = pad;
        } else {
            rows = tail_rows; src0 = 0; frames = 0; p = 0;
        }
        const long lo = p * CV, hi = (p + frames) * CV, n = rows * CV;
        for (long i = threadIdx.x; i < n; i += 256)
            d[row0 * CV + i] = (i >= lo && i < hi) ? s[src0 * CV + (i - lo)] : vec_zero<V>();
    }
}

// thread i owns vector i % (pad * CV) of segment i / (pad * CV); rows past the segment's end are left alone
template <int V>
__global__ __launch_bounds__(256) void zero_rows_kernel(float* __restrict__ x, const long* __restrict__ seg_offsets, long B, long CV,
                                                        long pad) {
    typedef typename vec_t<V>::type T;
    T* d = reinterpret_cast<T*>(x);
    const long per = pad * CV, n = B * per;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long b = i / per, r = i - b * per;
        const long row0 = seg_offsets[b];
        if (r < (seg_offsets[b + 1] - row0) * CV) d[row0 * CV + r] = vec_zero<V>();
    }
}

// grid (ceil(C / (16*V)), utterance blocks); 256 threads = 16 channel groups of V channels x 16 time groups, as pool_fwd_kernel:
// per time group the rows g, g + 16, ... in order, then the 16 groups in order, / T; the second pass sums fma(d, d, .) the same way.
template <bool STATS, int V>
__global__ __launch_bounds__(256) void pool_ragged_kernel(const float* __restrict__ x, long rs, const long* __restrict__ seg_offsets,
                                                          const long* __restrict__ lengths, long B, int C, float* __restrict__ out) {
    __shared__ float red[16][16 * V + 1];
    const int tid = threadIdx.x, cg = tid & 15, g = tid >> 4;
    const int c = (blockIdx.x * 16 + cg) * V;
    const bool active = c < C;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        const long T = lengths[b];
        const float* xp = x + seg_offsets[b] * rs + c;
        float s[V];
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = 0.f;
        if (active)
            for (long t = g; t < T; t += 16) {
                if (V == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(xp + t * rs);
                    s[0] += q.x; s[1] += q.y; s[2] += q.z; s[3] += q.w;
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) s[v] += xp[t * rs + v];
                }
            }
#pragma unroll
        for (int v = 0; v < V; ++v) red[g][cg * V + v] = s[v];
        __syncthreads();
        float mean[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float m = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) m += red[k][cg * V + v];
            mean[v] = m / (float)T;
        }
        __syncthreads();                                     // red is written again: by the second pass or the next utterance
        if (!STATS) {
            if (active && g == 0)
#pragma unroll
                for (int v = 0; v < V; ++v) out[b * C + c + v] = mean[v];
            continue;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) s[v] = 0.f;
        if (active)
            for (long t = g; t < T; t += 16) {
                float xv[V];
                if (V == 4) {
                    const float4 q = *reinterpret_cast<const float4*>(xp + t * rs);
                    xv[0] = q.x; xv[1] = q.y; xv[2] = q.z; xv[3] = q.w;
                } else {
#pragma unroll
                    for (int v = 0; v < V; ++v) xv[v] = xp[t * rs + v];
                }
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = xv[v] - mean[v];
                    s[v] = fmaf(d, d, s[v]);
                }
            }
#pragma unroll
        for (int v = 0; v < V; ++v) red[g][cg * V + v] = s[v];
        __syncthreads();
        if (active && g == 0) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float var = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) var += red[k][cg * V + v];
                var /= (float)T;
                out[b * 2 * C + c + v] = mean[v];
                out[b * 2 * C + C + c + v] = sqrtf(fminf(fmaxf(var, STDDEV_SQRT_MIN_CLIP), FLT_MAX));
            }
        }
        __syncthreads();                                     // the next utterance writes red
    }
}

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

inline unsigned strided_grid(long n) { return (unsigned)(n < 1 ? 1 : (n > MAX_GRID ? MAX_GRID : n)); }

template <bool STATS>
int pool_ragged(const char* fn, const float* x, long rs, const long* seg_offsets, const long* lengths, long B, int C, float* out,
                hipStream_t st) {
    if (!(x && seg_offsets && lengths && out)) {
        lidbox_set_error("%s: invalid argument: x, seg_offsets, lengths, out != NULL", fn);
        return LIDBOX_E_INVALID;
    }
    if (!(B >= 0 && C >= 1 && rs >= C)) {
        lidbox_set_error("%s: invalid argument: B >= 0; C >= 1; row_stride >= C", fn);
        return LIDBOX_E_INVALID;
    }
    if (B == 0) return LIDBOX_OK;
    if (C % 4 == 0 && rs % 4 == 0 && aligned16(x))
        hipLaunchKernelGGL((pool_ragged_kernel<STATS, 4>), dim3((unsigned)lbx_cdiv(C, 64), strided_grid(B)), dim3(256), 0, st, x, rs,
                           seg_offsets, lengths, B, C, out);
    else
        hipLaunchKernelGGL((pool_ragged_kernel<STATS, 1>), dim3((unsigned)lbx_cdiv(C, 16), strided_grid(B)), dim3(256), 0, st, x, rs,
                           seg_offsets, lengths, B, C, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        lidbox_set_error("%s: kernel launch failed: %s", fn, hipGetErrorString(e));
        return LIDBOX_E_LAUNCH;
    }
    return LIDBOX_OK;
}

}  // namespace

extern "C" int lidbox_ragged_pack_rows(const float* src, const long* src_offsets, float* dst, const long* seg_offsets, long B, int C,
                                       int pad, long tail_rows, lidbox_stream_t stream) {
    LBX_ARG(src && src_offsets && dst && seg_offsets, "src, src_offsets, dst, seg_offsets != NULL");
    LBX_ARG(B >= 0 && C >= 1 && pad >= 0 && tail_rows >= 0, "B, pad, tail_rows >= 0; C >= 1");
    if (B == 0) return LIDBOX_OK;
    const unsigned grid = strided_grid(B + 1);
    if (C % 4 == 0 && aligned16(src) && aligned16(dst))
        hipLaunchKernelGGL(pack_rows_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, src_offsets, dst, seg_offsets, B,
                           (long)(C / 4), (long)pad, tail_rows);
    else
        hipLaunchKernelGGL(pack_rows_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, src_offsets, dst, seg_offsets, B,
                           (long)C, (long)pad, tail_rows);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_ragged_zero_rows(float* x, const long* seg_offsets, long B, int C, int pad, lidbox_stream_t stream) {
    LBX_ARG(x && seg_offsets, "x, seg_offsets != NULL");
    LBX_ARG(B >= 0 && C >= 1 && pad >= 0, "B, pad >= 0; C >= 1");
    if (B == 0 || pad == 0) return LIDBOX_OK;
    const bool vec = C % 4 == 0 && aligned16(x);
    const long CV = vec ? C / 4 : C;
    const unsigned grid = strided_grid(lbx_cdiv(B * pad * CV, 256));
    if (vec)
        hipLaunchKernelGGL(zero_rows_kernel<4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, seg_offsets, B, CV, (long)pad);
    else
        hipLaunchKernelGGL(zero_rows_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, seg_offsets, B, CV, (long)pad);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_stats_pool_ragged_fwd(const float* x, long row_stride, const long* seg_offsets, const long* lengths, long B,
                                            int C, float* out, lidbox_stream_t stream) {
    return pool_ragged<true>(__func__, x, row_stride, seg_offsets, lengths, B, C, out, (hipStream_t)stream);
}

extern "C" int lidbox_avg_pool_ragged_fwd(const float* x, long row_stride, const long* seg_offsets, const long* lengths, long B,
                                          int C, float* out, lidbox_stream_t stream) {
    return pool_ragged<false>(__func__, x, row_stride, seg_offsets, lengths, B, C, out, (hipStream_t)stream);
}
