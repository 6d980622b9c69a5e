// mla.hip -- kernels of the multi-level attention classifier (lidbox_amd.models.multilevel_attention, reference
// lidbox/models/multilevel_attention.py:21-85; Yu et al. 2018):
//   * the attention pooling of one level and its backward pass (lidbox_mla_attention_fwd / _bwd), and both on utterances of
//     different lengths that lie end to end (lidbox_mla_attention_ragged_fwd / _bwd: the same per-utterance code);
//   * BatchNormalization-apply + ReLU + Dropout over [R, C] activations in one pass, forward and backward
//     (lidbox_bn_relu_dropout_fwd / _bwd), bit-identical to lidbox_bn_relu_* composed with lidbox_dropout_rows.
//
// Attention pooling, per utterance b, on z [T, K] (the logits of the level's Dense(K)):
//   p = softmax_k(z)      c = clip(p, lo, hi)      s[k] = sum_t c[t,k]      v = sigmoid(z)
//   att[k] = sum_t (c / s) v = (sum_t c v) / s[k]
// with lo / hi the float32 roundings of 1e-7 and 1 - 1e-7 (what TensorFlow compares against).
//
// Work split.  A wave is cut into 64 / G row slots of G lanes (G a power of two); a slot owns whole rows t and its lanes sit
// across the columns k, VEC consecutive columns per lane and NJ such pieces (column (gl + G j) VEC + e), so a row's maximum
// and sum are shuffle reductions inside the slot and every lane keeps sum_t c and sum_t c v of its own columns in registers.
// K = 100 with 16-byte loads gives G = 32: two rows per wave instruction.  Forward: ONE workgroup per utterance; its row slots
// are combined by xor shuffles (G, 2G, .. 32) and its waves through LDS in wave order, so the summation order is a function
// of (T, K) alone: utterance b's values do not depend on B or on b's place in the batch, and no atomics are involved.
// Backward has no sum over t, so its rows are also spread over blockIdx.y; which workgroup computes a row changes no bit.
#include "common.h"

namespace {

constexpr float MLA_CLIP_LO = 1e-7f;               // float32(1e-7)
constexpr float MLA_CLIP_HI = 0.99999988079071044921875f;   // float32(1 - 1e-7) = 1 - 2^-23
constexpr int MLA_MAX_K = 1024;

template <int VEC>
struct VecT;
template <>
struct VecT<1> {
    typedef float type;
};
template <>
struct VecT<4> {
    typedef float4 type;
};

// reduction over the G lanes of a row slot (G a power of two <= 64; wave-uniform)
__device__ __forceinline__ float slot_max(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float slot_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one row of z into registers: zr[j][e] = z[row][(gl + G j) VEC + e], columns >= K (and rows that do not exist) read as 0
template <int VEC, int NJ>
__device__ __forceinline__ void load_row(const float* __restrict__ zrow, bool row_ok, int gl, int G, int K, float (&zr)[NJ][VEC]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = (gl + G * j) * VEC;
        if constexpr (VEC == 4) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row_ok && col < K) t = *reinterpret_cast<const float4*>(zrow + col);       // K % 4 == 0: all four or none
            zr[j][0] = t.x;
            zr[j][1] = t.y;
            zr[j][2] = t.z;
            zr[j][3] = t.w;
        } else {
            zr[j][0] = (row_ok && col < K) ? zrow[col] : 0.f;
        }
    }
}

// softmax of the row in registers: on return pr = p (0 in columns >= K)
template <int VEC, int NJ>
__device__ __forceinline__ void row_softmax(const float (&zr)[NJ][VEC], int gl, int G, int K, float (&pr)[NJ][VEC]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            if ((gl + G * j) * VEC + e < K) m = fmaxf(m, zr[j][e]);
    m = slot_max(m, G);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const bool ok = (gl + G * j) * VEC + e < K;
            pr[j][e] = ok ? expf(zr[j][e] - m) : 0.f;
            sum += pr[j][e];
        }
    sum = slot_sum(sum, G);
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) pr[j][e] = pr[j][e] / sum;
}

// v = sigmoid(x) and dv = v (1 - v) from u = exp(-|x|): dv = u / (1 + u)^2 keeps its relative accuracy where v rounds to 1
// (x = 30: 1 - v is 9e-14, below float32's spacing at 1)
__device__ __forceinline__ float sigmoidf_(float x, float* dv = nullptr) {
    const float u = expf(-fabsf(x));
    const float r = 1.f / (1.f + u);
    if (dv) *dv = u * r * r;
    return x >= 0.f ? r : u * r;
}

// acc + c v of the forward pass, with its rounding written down.  Under -ffp-contract=fast the compiler may fuse `acc += c * v`
// or not, and it chose per instantiation: one fma everywhere except in <4,2> and <4,4>, where the product is rounded first.
// Those are the bits the dense kernel has always given, so they are pinned here: the dense and the ragged kernel are separate
// compilations of the same function, and left to the optimiser they need not agree (nor stay as they were).
template <bool FUSED>
__device__ __forceinline__ float mla_acc_cv(float acc, float c, float v) {
    if constexpr (FUSED) {
        return fmaf(c, v, acc);
    } else {
#pragma clang fp contract(off)
        const float cv = c * v;
        return acc + cv;
    }
}

// One utterance's pooling, by the whole workgroup: zb [T, K] -> att_b [K] and, unless COLSUM_OPT and colsum_b is NULL, colsum_b [K].
// The dense and the ragged forward kernel both call it, so an utterance's bits are those of (T, K) in either.
// block NW * 64, dynamic LDS NW * 2 * K floats
template <int VEC, int NJ, bool COLSUM_OPT>
__device__ __forceinline__ void mla_attention_utterance(const float* __restrict__ zb, int T, int K, int G, float* __restrict__ att_b,
                                                        float* __restrict__ colsum_b) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
    const int rpw = 64 / G, slot = lane / G, gl = lane - slot * G;
    float zr[NJ][VEC], pr[NJ][VEC], accS[NJ][VEC], accV[NJ][VEC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) accS[j][e] = accV[j][e] = 0.f;
    for (int t0 = w * rpw; t0 < T; t0 += NW * rpw) {            // wave-uniform bound: every lane takes part in the shuffles
        const int t = t0 + slot;
        const bool row_ok = t < T;
        load_row<VEC, NJ>(zb + (long)t * K, row_ok, gl, G, K, zr);
        row_softmax<VEC, NJ>(zr, gl, G, K, pr);
        if (row_ok) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if ((gl + G * j) * VEC + e < K) {
                        const float c = fminf(fmaxf(pr[j][e], MLA_CLIP_LO), MLA_CLIP_HI);
                        accS[j][e] += c;
                        accV[j][e] = mla_acc_cv<!(VEC == 4 && NJ >= 2)>(accV[j][e], c, sigmoidf_(zr[j][e]));
                    }
        }
    }
    // the row slots of the wave (xor G, 2G, .. 32: every lane ends with the same sum), then the waves in order
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            for (int o = G; o < 64; o <<= 1) {
                accS[j][e] += __shfl_xor(accS[j][e], o, 64);
                accV[j][e] += __shfl_xor(accV[j][e], o, 64);
            }
            const int col = (gl + G * j) * VEC + e;
            if (slot == 0 && col < K) {
                lds[(w * 2 + 0) * K + col] = accS[j][e];
                lds[(w * 2 + 1) * K + col] = accV[j][e];
            }
        }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        float s = 0.f, sv = 0.f;
        for (int i = 0; i < NW; ++i) {
            s += lds[(i * 2 + 0) * K + k];
            sv += lds[(i * 2 + 1) * K + k];
        }
        att_b[k] = sv / s;
        if (!COLSUM_OPT || colsum_b) colsum_b[k] = s;
    }
}

// grid (B), block NW * 64 (16 waves, 8 for the widest rows: mla_plan), dynamic LDS NW * 2 * K floats
template <int VEC, int NJ>
__global__ __launch_bounds__(VEC * NJ >= 16 ? 512 : 1024) void mla_attention_fwd_kernel(const float* __restrict__ z, int T, int K, int G, float* __restrict__ att,
                                                                 long ld_att, float* __restrict__ colsum) {
    const int b = blockIdx.x;
    mla_attention_utterance<VEC, NJ, false>(z + (long)b * T * K, T, K, G, att + (long)b * ld_att, colsum + (long)b * K);
}

// the same on utterances that lie end to end: z [total_T, K], utterance b = rows row_offsets[b] .. row_offsets[b + 1] (at least
// one); colsum may be NULL.  grid (B), block and LDS as above
template <int VEC, int NJ>
__global__ __launch_bounds__(VEC * NJ >= 16 ? 512 : 1024) void mla_attention_ragged_fwd_kernel(const float* __restrict__ z, const long* __restrict__ row_offsets, int K, int G,
                                                                        float* __restrict__ att, long ld_att, float* __restrict__ colsum) {
    const int b = blockIdx.x;
    const long r0 = row_offsets[b];
    const int T = (int)(row_offsets[b + 1] - r0);
    mla_attention_utterance<VEC, NJ, true>(z + r0 * K, T, K, G, att + (long)b * ld_att, colsum ? colsum + (long)b * K : nullptr);
}

// dp = m g (v - att) / s,  dz = p (dp - sum_j dp_j p_j) + g (c / s) v (1 - v),  m = (lo <= p <= hi)
// One utterance's share of a backward workgroup: zb [T, K] -> dzb [T, K] from the utterance's att, colsum and datt rows.  The
// workgroup is blockIdx.y of gridDim.y over the rows.  The dense and the ragged backward kernel both call it, so a row's bits
// are those of (its z, att, colsum, datt, K) in either: there is no sum over t.
template <int VEC, int NJ>
__device__ __forceinline__ void mla_attention_bwd_rows(const float* __restrict__ zb, int T, int K, int G, const float* __restrict__ att_b,
                                                       const float* __restrict__ colsum_b, const float* __restrict__ datt_b,
                                                       float* __restrict__ dzb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, NW = blockDim.x >> 6;
    const int rpw = 64 / G, slot = lane / G, gl = lane - slot * G;
    float zr[NJ][VEC], pr[NJ][VEC], gs[NJ][VEC], at[NJ][VEC];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int col = (gl + G * j) * VEC + e;
            const bool ok = col < K;
            gs[j][e] = ok ? datt_b[col] / colsum_b[col] : 0.f;
            at[j][e] = ok ? att_b[col] : 0.f;
        }
    const int step = (int)gridDim.y * NW * rpw;
    for (int t0 = ((int)blockIdx.y * NW + w) * rpw; t0 < T; t0 += step) {
        const int t = t0 + slot;
        const bool row_ok = t < T;
        load_row<VEC, NJ>(zb + (long)t * K, row_ok, gl, G, K, zr);
        row_softmax<VEC, NJ>(zr, gl, G, K, pr);
        float dp[NJ][VEC], tail[NJ][VEC];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float p = pr[j][e];
                float dv;
                const float v = sigmoidf_(zr[j][e], &dv);
                const bool pass = p >= MLA_CLIP_LO && p <= MLA_CLIP_HI;
                const float c = fminf(fmaxf(p, MLA_CLIP_LO), MLA_CLIP_HI);
                dp[j][e] = pass ? gs[j][e] * (v - at[j][e]) : 0.f;
                tail[j][e] = gs[j][e] * c * dv;
                dot += dp[j][e] * p;                               // columns >= K: p = 0
            }
        dot = slot_sum(dot, G);
        if (row_ok) {
            float* drow = dzb + (long)t * K;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = (gl + G * j) * VEC;
                float o[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) o[e] = pr[j][e] * (dp[j][e] - dot) + tail[j][e];
                if constexpr (VEC == 4) {
                    if (col < K) *reinterpret_cast<float4*>(drow + col) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
                    if (col < K) drow[col] = o[0];
                }
            }
        }
    }
}

// grid (B, rows split), block NW * 64
template <int VEC, int NJ>
__global__ __launch_bounds__(512) void mla_attention_bwd_kernel(const float* __restrict__ z, const float* __restrict__ att, long ld_att,
                                                                const float* __restrict__ colsum, const float* __restrict__ datt,
                                                                long ld_datt, int T, int K, int G, float* __restrict__ dz) {
    const int b = blockIdx.x;
    mla_attention_bwd_rows<VEC, NJ>(z + (long)b * T * K, T, K, G, att + (long)b * ld_att, colsum + (long)b * K, datt + (long)b * ld_datt,
                                    dz + (long)b * T * K);
}

// the same on utterances that lie end to end: z, dz [total_T, K], utterance b = rows row_offsets[b] .. row_offsets[b + 1].
// grid (B, rows split of the longest utterance), block NW * 64; a workgroup whose first row lies behind its utterance's end
// leaves at once
template <int VEC, int NJ>
__global__ __launch_bounds__(512) void mla_attention_ragged_bwd_kernel(const float* __restrict__ z, const long* __restrict__ row_offsets,
                                                                       const float* __restrict__ att, long ld_att,
                                                                       const float* __restrict__ colsum, const float* __restrict__ datt,
                                                                       long ld_datt, int K, int G, float* __restrict__ dz) {
    const int b = blockIdx.x;
    const long r0 = row_offsets[b];
    const int T = (int)(row_offsets[b + 1] - r0);
    if ((int)blockIdx.y * (int)(blockDim.x >> 6) * (64 / G) >= T) return;
    mla_attention_bwd_rows<VEC, NJ>(z + r0 * K, T, K, G, att + (long)b * ld_att, colsum + (long)b * K, datt + (long)b * ld_datt, dz + r0 * K);
}

// counter-based uniform in [0, 1) and the BatchNormalization expression: the SAME expressions as nnops.hip's hash_uniform
// (lidbox_dropout_rows) and conv2d.hip's bn_v (lidbox_bn_relu_*), so the fused pass reproduces their bits
__device__ __forceinline__ float mla_hash_uniform(unsigned long long seed, unsigned long long step, unsigned b, unsigned c) {
    unsigned long long v = seed + 0x9E3779B97F4A7C15ull * (step + 1) + (((unsigned long long)b << 32) | c);
    v ^= v >> 30; v *= 0xBF58476D1CE4E5B9ull;
    v ^= v >> 27; v *= 0x94D049BB133111EBull;
    v ^= v >> 31;
    return (float)(v >> 40) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float mla_bn_v(float x, float sc, float sh) { return fmaf(x, sc, sh); }

// y = relu(x scale + shift) * mask(seed, step, r, c);  BWD: dx = (x scale + shift > 0) ? dy * mask : 0.
// VEC = 4: C % 4 == 0 and 16-byte aligned pointers, so the four elements of a load share their row.  n: R * C / VEC.
template <int VEC, bool BWD>
__global__ __launch_bounds__(256) void bn_relu_dropout_kernel(const float* __restrict__ x, long n, int C, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, float rate, unsigned long long seed,
                                                              const long long* __restrict__ step, const float* dy, float* out) {
    typedef typename VecT<VEC>::type V;
    const unsigned long long stp = step ? (unsigned long long)*step : 0ull;
    const float keep_scale = 1.f / (1.f - rate);
    const bool drop = rate > 0.f;
    const int CV = C / VEC;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / CV;
        const int c0 = (int)(i - r * CV) * VEC;
        float xv[VEC], gv[VEC], sc[VEC], sh[VEC], o[VEC];
        *reinterpret_cast<V*>(xv) = reinterpret_cast<const V*>(x)[i];
        *reinterpret_cast<V*>(sc) = *reinterpret_cast<const V*>(scale + c0);
        *reinterpret_cast<V*>(sh) = *reinterpret_cast<const V*>(shift + c0);
        if (BWD) *reinterpret_cast<V*>(gv) = reinterpret_cast<const V*>(dy)[i];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float v = mla_bn_v(xv[e], sc[e], sh[e]);
            float val = BWD ? gv[e] : (v > 0.0f ? v : 0.0f);
            if (drop) val *= mla_hash_uniform(seed, stp, (unsigned)r, (unsigned)(c0 + e)) >= rate ? keep_scale : 0.f;
            o[e] = BWD ? (v > 0.0f ? val : 0.0f) : val;
        }
        reinterpret_cast<V*>(out)[i] = *reinterpret_cast<V*>(o);
    }
}

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

struct MlaPlan {
    int vec, G, nj, nw;
};

// K <= MLA_MAX_K.  vec4: K % 4 == 0 (every row of z then starts 16-byte aligned when the base does)
inline MlaPlan mla_plan(int K, bool vec4) {
    MlaPlan p;
    p.vec = vec4 ? 4 : 1;
    const int kv = (K + p.vec - 1) / p.vec;
    p.G = 1;
    while (p.G < 64 && p.G < kv) p.G <<= 1;
    const int need = (kv + p.G - 1) / p.G;
    p.nj = 1;
    while (p.nj < need) p.nj <<= 1;
    p.nw = K <= 512 ? 16 : 8;          // forward's LDS: nw * 2 * K floats <= 64 KiB
    return p;
}

template <int VEC, int NJ>
void launch_fwd(const MlaPlan& p, hipStream_t st, const float* z, int B, int T, int K, float* att, long ld_att, float* colsum) {
    hipLaunchKernelGGL((mla_attention_fwd_kernel<VEC, NJ>), dim3((unsigned)B), dim3(p.nw * 64), (size_t)p.nw * 2 * K * sizeof(float), st, z,
                       T, K, p.G, att, ld_att, colsum);
}

template <int VEC, int NJ>
void launch_ragged_fwd(const MlaPlan& p, hipStream_t st, const float* z, const long* row_offsets, long B, int K, float* att, long ld_att,
                       float* colsum) {
    hipLaunchKernelGGL((mla_attention_ragged_fwd_kernel<VEC, NJ>), dim3((unsigned)B), dim3(p.nw * 64), (size_t)p.nw * 2 * K * sizeof(float), st,
                       z, row_offsets, K, p.G, att, ld_att, colsum);
}

template <int VEC, int NJ>
void launch_bwd(const MlaPlan& p, hipStream_t st, const float* z, const float* att, long ld_att, const float* colsum, const float* datt,
                long ld_datt, int B, int T, int K, float* dz) {
    const int nw = 8;
    const int rows_per_wg = nw * (64 / p.G);
    long gy = lbx_cdiv(T, rows_per_wg);
    const long want = lbx_cdiv(2048, B);          // enough workgroups to fill the device when B is small
    if (gy > want) gy = want;
    hipLaunchKernelGGL((mla_attention_bwd_kernel<VEC, NJ>), dim3((unsigned)B, (unsigned)gy), dim3(nw * 64), 0, st, z, att, ld_att, colsum,
                       datt, ld_datt, T, K, p.G, dz);
}

template <int VEC, int NJ>
void launch_ragged_bwd(const MlaPlan& p, hipStream_t st, const float* z, const long* row_offsets, long B, int max_T, const float* att,
                       long ld_att, const float* colsum, const float* datt, long ld_datt, int K, float* dz) {
    const int nw = 8;
    const int rows_per_wg = nw * (64 / p.G);
    long gy = lbx_cdiv(max_T, rows_per_wg);         // the dense rule on the longest utterance
    const long want = lbx_cdiv(2048, B);
    if (gy > want) gy = want;
    hipLaunchKernelGGL((mla_attention_ragged_bwd_kernel<VEC, NJ>), dim3((unsigned)B, (unsigned)gy), dim3(nw * 64), 0, st, z, row_offsets, att,
                       ld_att, colsum, datt, ld_datt, K, p.G, dz);
}

}  // namespace

extern "C" int lidbox_mla_attention_fwd(const float* z, int B, int T, int K, float* att, long ld_att, float* colsum,
                                        lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 1 && K >= 1, "B >= 0, T >= 1, K >= 1");
    LBX_ARG(K <= MLA_MAX_K, "K <= 1024");
    LBX_ARG(z && att && colsum, "z, att, colsum != NULL");
    LBX_ARG(ld_att >= K, "ld_att >= K");
    if (B == 0) return LIDBOX_OK;
    const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z));
    hipStream_t st = (hipStream_t)stream;
#define MLA_FWD(V, N) launch_fwd<V, N>(p, st, z, B, T, K, att, ld_att, colsum)
    if (p.vec == 4) {
        if (p.nj == 1) MLA_FWD(4, 1);
        else if (p.nj == 2) MLA_FWD(4, 2);
        else MLA_FWD(4, 4);
    } else {
        if (p.nj == 1) MLA_FWD(1, 1);
        else if (p.nj == 2) MLA_FWD(1, 2);
        else if (p.nj == 4) MLA_FWD(1, 4);
        else if (p.nj == 8) MLA_FWD(1, 8);
        else MLA_FWD(1, 16);
    }
#undef MLA_FWD
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_mla_attention_ragged_fwd(const float* z, const long* row_offsets, long B, int K, float* att, long ld_att,
                                               float* colsum, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && B <= 0x7fffffffL && K >= 1, "0 <= B < 2^31, K >= 1");
    LBX_ARG(K <= MLA_MAX_K, "K <= 1024");
    LBX_ARG(z && row_offsets && att, "z, row_offsets, att != NULL");
    LBX_ARG(ld_att >= K, "ld_att >= K");
    if (B == 0) return LIDBOX_OK;
    const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z));        // r0 K floats on: a multiple of 16 bytes when K % 4 == 0
    hipStream_t st = (hipStream_t)stream;
#define MLA_RFWD(V, N) launch_ragged_fwd<V, N>(p, st, z, row_offsets, B, K, att, ld_att, colsum)
    if (p.vec == 4) {
        if (p.nj == 1) MLA_RFWD(4, 1);
        else if (p.nj == 2) MLA_RFWD(4, 2);
        else MLA_RFWD(4, 4);
    } else {
        if (p.nj == 1) MLA_RFWD(1, 1);
        else if (p.nj == 2) MLA_RFWD(1, 2);
        else if (p.nj == 4) MLA_RFWD(1, 4);
        else if (p.nj == 8) MLA_RFWD(1, 8);
        else MLA_RFWD(1, 16);
    }
#undef MLA_RFWD
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_mla_attention_bwd(const float* z, const float* att, long ld_att, const float* colsum, const float* datt,
                                        long ld_datt, int B, int T, int K, float* dz, lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && T >= 1 && K >= 1, "B >= 0, T >= 1, K >= 1");
    LBX_ARG(K <= MLA_MAX_K, "K <= 1024");
    LBX_ARG(z && att && colsum && datt && dz, "z, att, colsum, datt, dz != NULL");
    LBX_ARG(ld_att >= K && ld_datt >= K, "ld_att, ld_datt >= K");
    if (B == 0) return LIDBOX_OK;
    const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z) && aligned16(dz));
    hipStream_t st = (hipStream_t)stream;
#define MLA_BWD(V, N) launch_bwd<V, N>(p, st, z, att, ld_att, colsum, datt, ld_datt, B, T, K, dz)
    if (p.vec == 4) {
        if (p.nj == 1) MLA_BWD(4, 1);
        else if (p.nj == 2) MLA_BWD(4, 2);
        else MLA_BWD(4, 4);
    } else {
        if (p.nj == 1) MLA_BWD(1, 1);
        else if (p.nj == 2) MLA_BWD(1, 2);
        else if (p.nj == 4) MLA_BWD(1, 4);
        else if (p.nj == 8) MLA_BWD(1, 8);
        else MLA_BWD(1, 16);
    }
#undef MLA_BWD
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_mla_attention_ragged_bwd(const float* z, const long* row_offsets, long B, int max_T, int K, const float* att,
                                               long ld_att, const float* colsum, const float* datt, long ld_datt, float* dz,
                                               lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && B <= 0x7fffffffL && K >= 1, "0 <= B < 2^31, K >= 1");
    LBX_ARG(K <= MLA_MAX_K, "K <= 1024");
    LBX_ARG(B == 0 || max_T >= 1, "max_T >= 1");
    LBX_ARG(z && row_offsets && att && colsum && datt && dz, "z, row_offsets, att, colsum, datt, dz != NULL");
    LBX_ARG(ld_att >= K && ld_datt >= K, "ld_att, ld_datt >= K");
    if (B == 0) return LIDBOX_OK;
    const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z) && aligned16(dz));        // every utterance's first row is then aligned
    hipStream_t st = (hipStream_t)stream;
#define MLA_RBWD(V, N) launch_ragged_bwd<V, N>(p, st, z, row_offsets, B, max_T, att, ld_att, colsum, datt, ld_datt, K, dz)
    if (p.vec == 4) {
        if (p.nj == 1) MLA_RBWD(4, 1);
        else if (p.nj == 2) MLA_RBWD(4, 2);
        else MLA_RBWD(4, 4);
    } else {
        if (p.nj == 1) MLA_RBWD(1, 1);
        else if (p.nj == 2) MLA_RBWD(1, 2);
        else if (p.nj == 4) MLA_RBWD(1, 4);
        else if (p.nj == 8) MLA_RBWD(1, 8);
        else MLA_RBWD(1, 16);
    }
#undef MLA_RBWD
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

namespace {

template <bool BWD>
int bn_relu_dropout(const float* x, long R, int C, const float* scale, const float* shift, float rate, unsigned long long seed,
                    const void* step_counter, const float* dy, float* out, hipStream_t st) {
    const bool vec4 = C % 4 == 0 && aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(out) && (!BWD || aligned16(dy));
    const long n = R * C / (vec4 ? 4 : 1);
    long g = lbx_cdiv(n, 256);
    if (g > 8192) g = 8192;
    const long long* step = (const long long*)step_counter;
    if (vec4)
        hipLaunchKernelGGL((bn_relu_dropout_kernel<4, BWD>), dim3((unsigned)g), dim3(256), 0, st, x, n, C, scale, shift, rate, seed, step, dy, out);
    else
        hipLaunchKernelGGL((bn_relu_dropout_kernel<1, BWD>), dim3((unsigned)g), dim3(256), 0, st, x, n, C, scale, shift, rate, seed, step, dy, out);
    return 0;
}

}  // namespace

extern "C" int lidbox_bn_relu_dropout_fwd(const float* x, long R, int C, const float* scale, const float* shift, float rate,
                                          unsigned long long seed, const void* step_counter, float* y, lidbox_stream_t stream) {
    LBX_ARG(R >= 0 && R <= 0x7fffffffL && C >= 1 && R * C < (1L << 40), "0 <= R < 2^31, C >= 1");
    LBX_ARG(rate >= 0.f && rate < 1.f, "0 <= rate < 1");
    LBX_ARG(x && scale && shift && y, "pointers != NULL");
    if (R == 0) return LIDBOX_OK;
    bn_relu_dropout<false>(x, R, C, scale, shift, rate, seed, step_counter, nullptr, y, (hipStream_t)stream);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}

extern "C" int lidbox_bn_relu_dropout_bwd(const float* x, long R, int C, const float* scale, const float* shift, float rate,
                                          unsigned long long seed, const void* step_counter, const float* dy, float* dx,
                                          lidbox_stream_t stream) {
    LBX_ARG(R >= 0 && R <= 0x7fffffffL && C >= 1 && R * C < (1L << 40), "0 <= R < 2^31, C >= 1");
    LBX_ARG(rate >= 0.f && rate < 1.f, "0 <= rate < 1");
    LBX_ARG(x && scale && shift && dy && dx, "pointers != NULL");
    if (R == 0) return LIDBOX_OK;
    bn_relu_dropout<true>(x, R, C, scale, shift, rate, seed, step_counter, dy, dx, (hipStream_t)stream);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}
