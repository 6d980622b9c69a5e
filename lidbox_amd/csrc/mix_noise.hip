// mix_noise.hip -- additive-noise augmentation from a device-resident noise bank, and signal tiling, gfx950.
//
// Replaces (reference file:line):
//   lidbox/data/steps.py:296-307       tile the drawn noise clip to the utterance's length, snr_mixer(...)[2]
//   lidbox/features/audio.py:128-148   snr_mixer (third return value only)
//   lidbox/data/steps.py:961-966       repeat_too_short_signals: tf.tile(signal, [repeats])
//
// Output j mixes utterance src[j] (n samples) with clip clip[j] (m samples) at snr_db[j].  The tiled noise
// noise_ext[i] = clip[i mod m] is never materialised: every kernel reads it through periodic_load4.  Neither are
// clean_norm and noisenewlevel of the dense lidbox_snr_mixer; only the mix is written.
//
// Work split, chosen from n ALONE (never from what else is in the launch):
//   n <= 65536    one 1024-thread workgroup per output; the utterance is read once into registers (4 or 8 float4 per
//                 thread; beyond 32768 samples the second half goes to 128 KiB of LDS), both RMS rounds and the mix come from there; the clip is read three times, from cache after the
//                 first (a clip is short and shared by many outputs).  Memory traffic: 4n read + clip + 4n written.
//   n <= 2^21     tiles of 8192 samples, one 256-thread workgroup per (output, tile): round-1 partial sums, round-2
//                 partial sums (every workgroup first adds up the round-1 partials of its output), then the mix (adds up
//                 both rounds).  The utterance is read three times; rounds two and three find it in L2 / MALL.
// Bit identity: a thread adds its elements in index order, a wave and a workgroup reduce over a fixed tree, the tile
// partials of an output are added over the same fixed tree by every workgroup that needs them, and which element a thread
// owns depends on the element's index in the utterance only.  So the result for (utterance, clip, snr) is the same bits
// alone or in any batch, from run to run.  No atomics.
#include <stdint.h>

#include <algorithm>

#include "common.h"

namespace {

constexpr int MIX_MAX_LOG_LEN = 21;                 // n <= 2^21 samples (131 s at 16 kHz), the limit lidbox_resample has
constexpr int MIX_LDS_NL = 8;                       // float4 per thread kept in LDS by the longest resident form: 128 KiB
constexpr long MIX_REG_MAX = 4096L * (8 + MIX_LDS_NL);  // longest utterance of the resident form
constexpr int MIX_TILE = 8192;                      // samples per workgroup of the tiled form: 256 threads x 8 float4
constexpr int MIX_TILE_NV = MIX_TILE / (256 * 4);
constexpr int MIX_MAX_TILES = (1 << MIX_MAX_LOG_LEN) / MIX_TILE;      // 256: one partial per thread in the finish
static_assert(MIX_MAX_TILES == 256, "the finish reads one tile partial per thread");

// x[(i + k) mod m] for k = 0..3, m >= 1, i >= 0: one 16-byte load where the four samples are contiguous and aligned
// (the wrap point of a clip generally is not), else four loads that step over the wrap
__device__ __forceinline__ float4 periodic_load4(const float* __restrict__ x, int64_t m, int64_t i) {
    int64_t p = i;
    if (i >= m) p = ((i | m) >> 31) ? i % m : (int64_t)((uint32_t)i % (uint32_t)m);
    const float* q = x + p;
    if (p + 3 < m && (((uintptr_t)q) & 15) == 0) return *reinterpret_cast<const float4*>(q);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = x[p];
        if (++p == m) p = 0;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// samples [o, o + 4) of a signal of n samples, zeros past its end
__device__ __forceinline__ float4 load4_bounded(const float* __restrict__ x, int64_t n, int64_t o, bool vec) {
    if (vec && o + 3 < n) return *reinterpret_cast<const float4*>(x + o);
    return make_float4(o < n ? x[o] : 0.f, o + 1 < n ? x[o + 1] : 0.f, o + 2 < n ? x[o + 2] : 0.f, o + 3 < n ? x[o + 3] : 0.f);
}

__device__ __forceinline__ float4 periodic4_bounded(const float* __restrict__ z, int64_t m, int64_t n, int64_t o) {
    if (o >= n) return make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v = periodic_load4(z, m, o);
    if (o + 1 >= n) v.y = 0.f;
    if (o + 2 >= n) v.z = 0.f;
    if (o + 3 >= n) v.w = 0.f;
    return v;
}

__device__ __forceinline__ void store4_bounded(float* __restrict__ y, int64_t n, int64_t o, float4 v, bool vec) {
    if (o >= n) return;
    if (vec && o + 3 < n) {
        *reinterpret_cast<float4*>(y + o) = v;
        return;
    }
    y[o] = v.x;
    if (o + 1 < n) y[o + 1] = v.y;
    if (o + 2 < n) y[o + 2] = v.z;
    if (o + 3 < n) y[o + 3] = v.w;
}

__device__ __forceinline__ float sumsq4(float4 v, float scale, float s) {
    const float x = scale * v.x, y = scale * v.y, u = scale * v.z, w = scale * v.w;
    s = fmaf(x, x, s); s = fmaf(y, y, s); s = fmaf(u, u, s); s = fmaf(w, w, s);
    return s;
}

// sum over the workgroup (WAVES waves), the same value in every thread; fixed order
template <int WAVES>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += red[w];
    return s;
}

// audio.py:134-148 from the four sums: the factors of clean and of the noise in the mix
struct MixScale {
    float sc, sz;         // -25 dBFS normalisation of clean and noise (:134-139)
};

__device__ __forceinline__ MixScale mix_norm(float sumsq_c, float sumsq_z, float fn) {
    const float lvl25 = __powf(10.0f, -25.0f / 20.0f);
    MixScale r;
    r.sc = lvl25 / sqrtf(sumsq_c / fn);
    r.sz = lvl25 / sqrtf(sumsq_z / fn);
    return r;
}

__device__ __forceinline__ float mix_noisescalar(float sumsq_cn, float sumsq_zn, float fn, float snr_db) {
    const float rmsclean = sqrtf(sumsq_cn / fn), rmsnoise = sqrtf(sumsq_zn / fn);
    const float level = __powf(10.0f, snr_db / 20.0f);                         // :143
    return sqrtf(rmsclean / level / rmsnoise);                                 // :144
}

__device__ __forceinline__ float4 mix4(float4 a, float4 w, float sc, float sz, float ns) {
    return make_float4(sc * a.x + ns * (sz * w.x), sc * a.y + ns * (sz * w.y), sc * a.z + ns * (sz * w.z),
                       sc * a.w + ns * (sz * w.w));
}

struct MixArgs {
    const float* signals;
    const int64_t* starts;
    const int64_t* lengths;
    const float* bank;
    const int64_t* bank_starts;
    const int64_t* bank_lengths;
    const int32_t* src;
    const int32_t* clip;
    const float* snr_db;
    float* out;
    const int64_t* out_starts;
    float2* partials;          // tiled form: round r, output j, tile t at partials[(r * J + j) * MIX_MAX_TILES + t]
    int J;
};

// ---- resident form: outputs with n in (n_lo, 4096 * (NV + NL)]; one 1024-thread workgroup per output ----
// A thread keeps NV float4 of the utterance in registers (4 or 8: 16 would spill at the 128-VGPR limit of a 1024-thread
// workgroup, as in snr_mixer_reg_kernel) and NL more in LDS slots of its own (16 KiB per unit of NL; no barrier needed,
// consecutive lanes hold consecutive float4: conflict-free 16-byte accesses).
template <int NV, int NL>
__global__ __launch_bounds__(1024) void mix_reg_kernel(const MixArgs a, int64_t n_lo) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[16];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int b = a.src[j], k = a.clip[j];
    const int64_t n = a.lengths[b];
    if (n <= n_lo || n > 4096L * (NV + NL)) return;             // another launch's output (uniform over the workgroup)
    const int64_t m = a.bank_lengths[k];
    const float* c = a.signals + a.starts[b];
    const float* z = a.bank + a.bank_starts[k];
    float* y = a.out + a.out_starts[j];
    const bool cvec = (((uintptr_t)c) & 15) == 0, yvec = (((uintptr_t)y) & 15) == 0;
    const float fn = (float)n;
    float4* mine = reinterpret_cast<float4*>(smem) + tid;       // this thread's slot i at mine[i * 1024]
    float4 cv[NV];
    float s1c = 0.f, s1z = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        cv[i] = load4_bounded(c, n, ((int64_t)i * 1024 + tid) * 4, cvec);
        s1c = sumsq4(cv[i], 1.f, s1c);
    }
    // every loop but those over cv stays rolled: unrolled, their loads are hoisted over the resident utterance and spill
#pragma unroll 2
    for (int i = 0; i < NL; ++i) {
        const float4 v = load4_bounded(c, n, ((int64_t)(NV + i) * 1024 + tid) * 4, cvec);
        mine[i * 1024] = v;
        s1c = sumsq4(v, 1.f, s1c);
    }
#pragma unroll 2
    for (int i = 0; i < NV + NL; ++i) s1z = sumsq4(periodic4_bounded(z, m, n, ((int64_t)i * 1024 + tid) * 4), 1.f, s1z);
    const MixScale sc = mix_norm(block_sum<16>(s1c, red), block_sum<16>(s1z, red), fn);
    float s2c = 0.f, s2z = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s2c = sumsq4(cv[i], sc.sc, s2c);
#pragma unroll 2
    for (int i = 0; i < NL; ++i) s2c = sumsq4(mine[i * 1024], sc.sc, s2c);
#pragma unroll 2
    for (int i = 0; i < NV + NL; ++i) s2z = sumsq4(periodic4_bounded(z, m, n, ((int64_t)i * 1024 + tid) * 4), sc.sz, s2z);
    const float ns = mix_noisescalar(block_sum<16>(s2c, red), block_sum<16>(s2z, red), fn, a.snr_db[j]);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int64_t o = ((int64_t)i * 1024 + tid) * 4;
        if (o < n) store4_bounded(y, n, o, mix4(cv[i], periodic_load4(z, m, o), sc.sc, sc.sz, ns), yvec);
        __builtin_amdgcn_sched_barrier(0);                     // one noise load in flight at a time, for the same reason
    }
#pragma unroll 2
    for (int i = 0; i < NL; ++i) {
        const int64_t o = ((int64_t)(NV + i) * 1024 + tid) * 4;
        if (o < n) store4_bounded(y, n, o, mix4(mine[i * 1024], periodic_load4(z, m, o), sc.sc, sc.sz, ns), yvec);
    }
}

// ---- tiled form: outputs with n > MIX_REG_MAX; grid (J, tiles of the longest output) ----
// sum of the tile partials of round `round` of output j, the same value in every thread
__device__ __forceinline__ float2 mix_finish(const MixArgs& a, int round, int j, int tiles, float* red) {
    const float2* p = a.partials + ((int64_t)round * a.J + j) * MIX_MAX_TILES;
    const float2 v = (int)threadIdx.x < tiles ? p[threadIdx.x] : make_float2(0.f, 0.f);
    float2 s;
    s.x = block_sum<4>(v.x, red);
    s.y = block_sum<4>(v.y, red);
    return s;
}

// PHASE 0: round-1 partials; 1: round-2 partials; 2: the mix
template <int PHASE>
__global__ __launch_bounds__(256) void mix_tile_kernel(const MixArgs a) {
    __shared__ float red[4];
    const int j = blockIdx.x, tile = blockIdx.y, tid = threadIdx.x;
    const int b = a.src[j], k = a.clip[j];
    const int64_t n = a.lengths[b];
    const int tiles = (int)((n + MIX_TILE - 1) / MIX_TILE);
    if (n <= MIX_REG_MAX || tile >= tiles) return;
    const int64_t m = a.bank_lengths[k];
    const float* c = a.signals + a.starts[b];
    const float* z = a.bank + a.bank_starts[k];
    const bool cvec = (((uintptr_t)c) & 15) == 0;
    const float fn = (float)n;
    MixScale sc{1.f, 1.f};
    float ns = 0.f;
    if (PHASE >= 1) {
        const float2 s1 = mix_finish(a, 0, j, tiles, red);
        sc = mix_norm(s1.x, s1.y, fn);
    }
    if (PHASE == 2) {
        const float2 s2 = mix_finish(a, 1, j, tiles, red);
        ns = mix_noisescalar(s2.x, s2.y, fn, a.snr_db[j]);
    }
    const int64_t t0 = (int64_t)tile * MIX_TILE;
    if (PHASE < 2) {
        float sc_ = 0.f, sz_ = 0.f;
#pragma unroll
        for (int i = 0; i < MIX_TILE_NV; ++i) {
            const int64_t o = t0 + ((int64_t)i * 256 + tid) * 4;
            sc_ = sumsq4(load4_bounded(c, n, o, cvec), sc.sc, sc_);
            sz_ = sumsq4(periodic4_bounded(z, m, n, o), sc.sz, sz_);
        }
        sc_ = block_sum<4>(sc_, red);
        sz_ = block_sum<4>(sz_, red);
        if (tid == 0) a.partials[((int64_t)PHASE * a.J + j) * MIX_MAX_TILES + tile] = make_float2(sc_, sz_);
    } else {
        float* y = a.out + a.out_starts[j];
        const bool yvec = (((uintptr_t)y) & 15) == 0;
#pragma unroll
        for (int i = 0; i < MIX_TILE_NV; ++i) {
            const int64_t o = t0 + ((int64_t)i * 256 + tid) * 4;
            if (o < n)
                store4_bounded(y, n, o, mix4(load4_bounded(c, n, o, cvec), periodic_load4(z, m, o), sc.sc, sc.sz, ns), yvec);
        }
    }
}

// ---- tile: out[b][i] = in[b][i mod n_b] for i < reps[b] * n_b; grid (B, strips of 4096 samples) ----
__global__ __launch_bounds__(256) void signal_tile_kernel(const float* __restrict__ signals,
                                                          const int64_t* __restrict__ starts,
                                                          const int64_t* __restrict__ lengths,
                                                          const int64_t* __restrict__ reps, float* __restrict__ out,
                                                          const int64_t* __restrict__ out_starts) {
    const int b = blockIdx.x;
    const int64_t n = lengths[b], total = n * reps[b];
    if (n <= 0 || total <= 0) return;
    const float* x = signals + starts[b];
    float* y = out + out_starts[b];
    const bool yvec = (((uintptr_t)y) & 15) == 0;
    for (int64_t o = ((int64_t)blockIdx.y * 256 + threadIdx.x) * 4; o < total; o += (int64_t)gridDim.y * 1024)
        store4_bounded(y, total, o, periodic_load4(x, n, o), yvec);
}

int mix_check(const int64_t* len_h, const int64_t* bank_len_h, const int32_t* src_h, const int32_t* clip_h, int B, int M,
              int J, long* max_len, bool* any_reg, bool* any_tiled) {
    *max_len = 0;
    *any_reg = *any_tiled = false;
    for (int j = 0; j < J; ++j) {
        if (src_h[j] < 0 || src_h[j] >= B) {
            lidbox_set_error("lidbox_mix_noise: invalid argument: output %d: utterance index %d is outside 0 .. %d", j,
                             src_h[j], B - 1);
            return LIDBOX_E_INVALID;
        }
        if (clip_h[j] < 0 || clip_h[j] >= M) {
            lidbox_set_error("lidbox_mix_noise: invalid argument: output %d: clip index %d is outside 0 .. %d", j, clip_h[j],
                             M - 1);
            return LIDBOX_E_INVALID;
        }
        if (bank_len_h[clip_h[j]] < 1) {
            lidbox_set_error("lidbox_mix_noise: invalid argument: output %d: noise clip %d is empty", j, clip_h[j]);
            return LIDBOX_E_INVALID;
        }
        const long n = len_h[src_h[j]];
        if (n < 0 || n > (1L << MIX_MAX_LOG_LEN)) {
            lidbox_set_error("lidbox_mix_noise: invalid argument: output %d: %ld samples is outside the supported range "
                             "0 .. 2^%d = %ld samples", j, n, MIX_MAX_LOG_LEN, 1L << MIX_MAX_LOG_LEN);
            return LIDBOX_E_INVALID;
        }
        *max_len = std::max(*max_len, n);
        if (n > MIX_REG_MAX) *any_tiled = true;
        else if (n > 0) *any_reg = true;
    }
    return LIDBOX_OK;
}

}  // namespace

extern "C" size_t lidbox_mix_noise_workspace(long max_length, int J) {
    if (J <= 0 || max_length <= MIX_REG_MAX) return 0;
    return (size_t)2 * J * MIX_MAX_TILES * sizeof(float2);
}

extern "C" int lidbox_mix_noise(const float* signals, const int64_t* starts, const int64_t* lengths, const float* bank,
                                const int64_t* bank_starts, const int64_t* bank_lengths, const int32_t* src,
                                const int32_t* clip, const float* snr_db, float* out, const int64_t* out_starts,
                                const int64_t* lengths_host, const int64_t* bank_lengths_host, const int32_t* src_host,
                                const int32_t* clip_host, int B, int M, int J, void* workspace, size_t workspace_bytes,
                                lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && M >= 0 && J >= 0, "B, M, J must be >= 0");
    if (J == 0) return LIDBOX_OK;
    LBX_ARG(lengths_host && bank_lengths_host && src_host && clip_host, "host arrays are required");
    long max_len;
    bool any_reg, any_tiled;
    const int st = mix_check(lengths_host, bank_lengths_host, src_host, clip_host, B, M, J, &max_len, &any_reg, &any_tiled);
    if (st != LIDBOX_OK) return st;
    if (max_len == 0) return LIDBOX_OK;
    LBX_ARG(signals && starts && lengths && bank && bank_starts && bank_lengths && src && clip && snr_db && out && out_starts,
            "null pointer");
    MixArgs a{signals, starts, lengths, bank, bank_starts, bank_lengths, src, clip, snr_db, out, out_starts, nullptr, J};
    hipStream_t s = (hipStream_t)stream;
    if (any_reg) {
        // one launch per register footprint that occurs; a workgroup whose output belongs to another launch returns at once
        bool need[3] = {false, false, false};
        for (int j = 0; j < J; ++j) {
            const long n = lengths_host[src_host[j]];
            if (n > 0 && n <= MIX_REG_MAX) need[n <= 4096L * 4 ? 0 : (n <= 4096L * 8 ? 1 : 2)] = true;
        }
        if (need[0]) hipLaunchKernelGGL((mix_reg_kernel<4, 0>), dim3(J), dim3(1024), 0, s, a, (int64_t)0);
        if (need[1]) hipLaunchKernelGGL((mix_reg_kernel<8, 0>), dim3(J), dim3(1024), 0, s, a, (int64_t)4096 * 4);
        if (need[2]) {
            const int lds = MIX_LDS_NL * 1024 * (int)sizeof(float4);
            static const hipError_t attr = hipFuncSetAttribute((const void*)mix_reg_kernel<8, MIX_LDS_NL>,
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            LBX_HIP(attr);
            hipLaunchKernelGGL((mix_reg_kernel<8, MIX_LDS_NL>), dim3(J), dim3(1024), lds, s, a, (int64_t)4096 * 8);
        }
        LBX_LAUNCH_OK();
    }
    if (any_tiled) {
        LBX_ARG(workspace && workspace_bytes >= lidbox_mix_noise_workspace(max_len, J),
                "workspace smaller than lidbox_mix_noise_workspace()");
        LBX_ARG(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
        a.partials = reinterpret_cast<float2*>(workspace);
        const dim3 grid(J, (unsigned)lbx_cdiv(max_len, MIX_TILE));
        hipLaunchKernelGGL(mix_tile_kernel<0>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mix_tile_kernel<1>, grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mix_tile_kernel<2>, grid, dim3(256), 0, s, a);
        LBX_LAUNCH_OK();
    }
    return LIDBOX_OK;
}

extern "C" int lidbox_signal_tile(const float* signals, const int64_t* starts, const int64_t* lengths, const int64_t* reps,
                                  float* out, const int64_t* out_starts, int B, long max_out_length,
                                  lidbox_stream_t stream) {
    LBX_ARG(B >= 0 && max_out_length >= 0, "B and max_out_length must be >= 0");
    if (B == 0 || max_out_length == 0) return LIDBOX_OK;
    LBX_ARG(signals && starts && lengths && reps && out && out_starts, "null pointer");
    const unsigned strips = (unsigned)std::min<long>(lbx_cdiv(max_out_length, 4096), 1024);
    hipLaunchKernelGGL(signal_tile_kernel, dim3(B, strips), dim3(256), 0, (hipStream_t)stream, signals, starts, lengths, reps,
                       out, out_starts);
    LBX_LAUNCH_OK();
    return LIDBOX_OK;
}
