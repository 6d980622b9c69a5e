"""
oracle.features_paths_np -- the plan and the dispatch of csrc/features.hip restated as plain functions, a float32
transcription of the fused tile, and per-element rounding bounds for every stage of the feature path.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Nothing under lidbox_amd/ imports this module, and this module imports
nothing from lidbox_amd/: the two host tables it needs from the library (the float32 mel matrix and the float32 Hann window,
neither of which needs a device) are fetched by the caller through the C ABI (`host_mel_matrix`, `host_window` take the
ctypes library as an argument).

1. THE PLAN (`make_plan`).  lidbox_feat_plan_create cuts the float32 mel matrix W[F][M] into per-band runs of non-zero
   weights (`start`, `cnt`, `nnz`), then looks for the smallest `seg_len` in 1 .. 32 for which the bands, each cut into
   ceil(cnt / seg_len) segments (a band without weights still takes one lane), fit the 64 lanes of a wave (`seg_ok`);
   `seg_steps` = ceil(log2(most segments of one band)).  `fused_ok` = fft_length 512, frame <= 512, M <= 64, nnz <= 1024,
   M ncoef <= 1024.  The MFCC runs: dct_runs = min(max(1, 64 // ncoef), M), dct_len = ceil(M / dct_runs), then dct_runs =
   ceil(M / dct_len).

2. THE DISPATCH (`dispatch`).  lidbox_extract_features_fwd_ex, in order: B = 0 or T = 0 -> nothing; fused plans take
   feat512_stream_kernel when the rows allow 16-byte loads (pointer, sig_stride, S, L multiples of 4 samples; 8 bytes for PCM),
   the plan is seg_ok (or the kind is the spectrogram) and a 16-bit source comes with power 2; otherwise fused_feat512_kernel
   (a 16-bit source is refused there); other plans take the generic kernels.  The streaming kernel runs one workgroup per
   `tiles_per_wg` = ceil(ntiles / CUs) consecutive tiles with min(waves the LDS holds, 16, tiles_per_wg) waves; the round-1
   kernel 4-wave workgroups of 4 `iters` tiles, iters = ceil(ceil(ntiles / 4) / (4 * 256 * FEAT_WAVES)).

3. BOUNDS, per element, u = 2^-24 (float32 unit roundoff), against float64 numpy on the same samples.
   Complex bin.  X_k = sum_n (w_n x_n) e^{-2 pi i n k / 512}.  Every path from a sample to a bin of the packed 256-point
   transform Z' passes: the window product (1 u); pass 1, a radix-16 DFT = two radix-4 stages, four levels of complex
   additions (4 u) and one multiplication by a constant twiddle (a complex product by a factor rounded from double:
   sqrt(2) gamma_2 + the factor's own error <= 2.83 u + 0.71 u = 3.6 u, Higham, Accuracy and Stability, 3.6); the W256 table
   twiddle (3.6 u); pass 2 (4 u + 3.6 u): c' = 19.8, relative to sum_n |z'_n| <= 1/2 sum |w x| (the 1/2 of the untangling is
   folded into the window table, exactly).  The untangling is X = Z'_k (1 - i w) + conj(Z'_{256-k}) (1 + i w), |w| = 1, and
   |1 - i w| + |1 + i w| <= 2 sqrt(2): the transform's error reaches X with at most sqrt(2) c' u sum |w x| = 28 u; its own
   operations (e and o one addition each, the W512 product 3.6 u on o, the final addition) add at most 5.6 u sum |w x|.
   C_FUSED = 34.  The device's window is the float32 table of lidbox_hann_window, the reference's is float64: their
   difference enters as sum_n |x_n| |w32_n - w64_n|, computed, not estimated.
   NL = 13 (frames <= 416 samples) changes no rounding: dft4_z3 is dft4 with the additions of an exact zero left out.
   Power.  P = re^2 + im^2: 2 |X| e + e^2 + 3 u P.        power != 2 goes through __powf, a fast-math intrinsic whose
   error no document of the toolchain states: those cases keep the project's tolerances (2e-5 of the utterance's largest value for spectrogram and
   mel, 1e-3 for log-mel and MFCC), see TOL_POWF_REL / TOL_POWF_LOG.
   Mel.  The reference sums the reference's P with the PLAN's float32 weights (the matrix itself is pinned against the
   oracle's in tests/test_abi_cpu.py): sum w e_P + (seg_len + seg_steps + 1) u sum w P -- a lane's fma chain of seg_len
   terms, seg_steps shuffle additions.  The CSR kernels (SEGMEL = false, generic) chain max(cnt) terms instead.
   Log-mel.  |ln(a + d) - ln(a)| <= -ln(1 - d / a): -log1p(-e_mel / (mel + 1e-6)), plus `ln_pos_bound` of the value:
   the float32 addition of 1e-6f (1.05 u in the log domain, 0.05 u of it the rounding of the constant), v_log_f32 with TWICE
   its claimed 1 ulp of log2 x (features.hip, comment of ln_pos), the product with the rounded ln 2 (2 u |ln x|).
   MFCC.  sum |d| e_logmel + (M + ceil(log2 dct_runs) + 1) u sum |d| (|logmel| + e_logmel); the + 1 is the table entry,
   rounded from double.
   Generic kernels (fft_length != 512, M > 64, frames > 512): a plain sum of Leff <= nfft products per component,
   sqrt(2) (Leff + 2) u sum |w x|.

4. EXACT RELATIONS the GPU module asserts, and why they are exact.
   shadow == bf16(out): the kernel converts the very registers it stores (store_mel_tile), the post pass reads `out` back.
   PCM == convert-then-float: an int16 is exact in float32, 1 / 32768 is a power of two, so (s * (w / 32768)) and
   ((s / 32768) * w) are the same float32 product whenever no factor is denormal (w = 0 or >= 2^-30 here).
   Batch and position independence: a tile's arithmetic reads nothing but its own samples and the tables; the wave, the
   workgroup and the batch only choose where it runs.  Hence bit identity alone / in any batch / from run to run.
   Gaps: the kernels store exactly T * C values per utterance.

5. THE TAIL.  A frame's lanes load 32 NL (416 or 512) consecutive samples, of which the frame owns the first L; the rest
   meet the zero part of the window table.  What they may be is bounded by (T - 1) S + L, the end of the last frame: a NaN /
   Inf behind it is read by no frame (tf.signal.frame drops the tail).  Inside it, a non-finite sample owned by a LATER
   frame also turns the earlier frames NaN whose loads reach it (`lost_frames`): the utterance fails either way.
"""
import ctypes
import math

import numpy as np

from . import features_np as fo

U = 2.0 ** -24
SPEC, MEL, LOGMEL, MFCC = 0, 1, 2, 3
KIND_NAMES = {SPEC: "SPECTROGRAM", MEL: "MEL", LOGMEL: "LOGMEL", MFCC: "MFCC"}
WAVE_SCRATCH = 9280
FEAT_WAVES = 3
LDS_BYTES = 160 * 1024
C_FUSED = 34.0
TOL_POWF_REL = 2e-5            # power != 2: of the utterance's largest value (spectrogram, mel)
TOL_POWF_LOG = 1e-3            # power != 2: log-mel, MFCC


# ------------------------------------------------------------------------------------------------ host tables (C ABI, no device)
def host_mel_matrix(lib, M, F, sample_rate, fmin, fmax):
    W = np.zeros((F, M), np.float32)
    rc = lib.lidbox_mel_weight_matrix(int(M), int(F), int(sample_rate), ctypes.c_float(fmin), ctypes.c_float(fmax),
                                      ctypes.c_void_p(W.ctypes.data))
    assert rc == 0
    return W


def host_window(lib, L):
    w = np.zeros(L, np.float32)
    rc = lib.lidbox_hann_window(int(L), ctypes.c_void_p(w.ctypes.data))
    assert rc == 0
    return w


def twiddles():
    """the plan's tw256[k1 * 16 + n2] = W256^(n2 k1) and tw512[k] = W512^k, rounded from double"""
    k1, n2 = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    a = -2.0 * np.pi * (n2 * k1) / 256.0
    tw256 = (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)
    a = -2.0 * np.pi * np.arange(256) / 512.0
    return tw256, (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


# ------------------------------------------------------------------------------------------------ 1. the plan
class Plan:
    pass


def mel_segments(W):
    """(start, cnt, nnz, seg_ok, seg_len, seg_steps, lanes, seg_w) of a float32 mel matrix W[F][M]; lanes = [(band, first bin,
    index in band, segments of band)] for the used lanes, seg_w[seg_len][64] zero padded"""
    F, M = W.shape
    start, cnt = np.zeros(M, int), np.zeros(M, int)
    for m in range(M):
        nz = np.flatnonzero(W[:, m] != 0)
        if nz.size:
            start[m], cnt[m] = nz[0], nz[-1] - nz[0] + 1
    nnz = int(cnt.sum())
    for sl in range(1, 33):
        ns = np.where(cnt > 0, -(-cnt // sl), 1)
        if ns.sum() > 64:
            continue
        steps = 0
        while (1 << steps) < ns.max():
            steps += 1
        lanes, seg_w = [], np.zeros((sl, 64), np.float32)
        for m in range(M):
            for i in range(ns[m]):
                b0 = start[m] + i * sl
                for j in range(sl):
                    if i * sl + j < cnt[m]:
                        seg_w[j, len(lanes)] = W[b0 + j, m]
                lanes.append((m, int(b0), i, int(ns[m])))
        return start, cnt, nnz, True, sl, steps, lanes, seg_w
    return start, cnt, nnz, False, 0, 0, [], np.zeros((1, 64), np.float32)


def make_plan(W, sample_rate, L, S, nfft=512, power=2.0, coef_begin=1, coef_end=13):
    """lidbox_feat_plan_create restated; W = host_mel_matrix(lib, M, nfft // 2 + 1, sample_rate, fmin, fmax)"""
    p = Plan()
    p.sample_rate, p.L, p.S, p.nfft, p.F, p.power = sample_rate, L, S, nfft, nfft // 2 + 1, float(power)
    assert W.shape[0] == p.F and W.dtype == np.float32
    p.W, p.M = W, W.shape[1]
    cb, ce = max(coef_begin, 0), min(coef_end, p.M)
    ce = max(ce, cb)
    p.coef_begin, p.coef_end, p.ncoef = cb, ce, ce - cb
    p.start, p.cnt, p.nnz, p.seg_ok, p.seg_len, p.seg_steps, p.lanes, p.seg_w = mel_segments(W)
    p.fused_ok = nfft == 512 and L <= 512 and p.M <= 64 and p.nnz <= 1024 and p.M * p.ncoef <= 1024
    runs = 1
    if p.ncoef > 0:
        runs = min(max(1, 64 // p.ncoef), p.M)
    p.dct_len = -(-p.M // runs)
    p.dct_runs = -(-p.M // p.dct_len)
    p.bs_m2 = 0
    Leff = min(L, nfft)
    if nfft >= 3 and nfft & (nfft - 1) and Leff + p.F - 1 <= 16384:
        p.bs_m2 = 1
        while p.bs_m2 < Leff + p.F - 1:
            p.bs_m2 <<= 1
    return p


def num_frames(N, L, S):
    return 0 if N < L else 1 + (N - L) // S


def stream_table_bytes(p, kind):
    floats = 1536 + (0 if kind == SPEC else 192 + p.seg_len * 64) + (p.M * p.ncoef if kind == MFCC else 0)
    return (floats * 4 + 4 + 15) & ~15


def stream_waves(p, kind):
    """waves of the streaming workgroup before the cut to tiles_per_wg"""
    return min(16, (LDS_BYTES - stream_table_bytes(p, kind)) // WAVE_SCRATCH)


def xcd_chunk_id(bid, nwg):
    xcd, idx, q, r = bid & 7, bid >> 3, nwg >> 3, nwg & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


# ------------------------------------------------------------------------------------------------ 2. the dispatch
def dispatch(p, kind, B, N, ncu, src16=False, sig_align=0, sig_stride=None, out16=False, out_align=0, out_bs=0):
    """What lidbox_extract_features_fwd_ex launches.  sig_align / out_align: the pointers' byte offsets from a multiple of 16;
    sig_stride in samples (None: N); out_bs in floats (0: dense).  Returns None when nothing is launched, else a dict:
    kernel, targs, nwg, tiles_per_wg, waves, iters, ntiles, store (per tile 'vec' / 'scalar', mel and log-mel only), shadow
    ('kernel' / 'post' / None), refused (the message's key word when the call is an argument error)."""
    T = num_frames(N, p.L, p.S)
    if B == 0 or T == 0:
        return None
    sig_stride = N if sig_stride is None else sig_stride
    chan = {SPEC: p.F, MEL: p.M, LOGMEL: p.M, MFCC: p.ncoef}[kind]
    out_bs = out_bs or T * chan
    r = dict(T=T, refused=None, store=None, shadow=None, iters=0)
    if not p.fused_ok:
        if src16:
            return dict(r, refused="fused")
        Leff = min(p.L, p.nfft)
        if p.nfft >= 4 and p.nfft & (p.nfft - 1) == 0:
            r["kernel"] = "pow2_fft_spectrogram_kernel"
        elif p.bs_m2:
            r["kernel"] = "bluestein_inplace_spectrogram_kernel" if p.bs_m2 > 8192 else "bluestein_spectrogram_kernel"
        else:
            r["kernel"] = "generic_spectrogram_kernel"
        r.update(targs=(), Leff=Leff, nwg=T * B, tiles_per_wg=1, waves=4, ntiles=T * B, shadow="post" if out16 else None)
        per = T * chan
        grid = min(-(-per // 256), 64)
        r["flag_trips"] = -(-per // (grid * 256))
        return r
    pow2 = p.power == 2.0
    tpu = -(-T // 8)
    ntiles = B * tpu
    segmel = p.seg_ok and kind != SPEC
    vec4 = (sig_align % (8 if src16 else 16) == 0) and sig_stride % 4 == 0 and p.S % 4 == 0 and p.L % 4 == 0
    r.update(ntiles=ntiles, tiles_per_utt=tpu, vec4=vec4)

    def stores(M):
        if kind not in (MEL, LOGMEL):
            return None
        out = []
        for tile in range(ntiles):
            b, t0 = divmod(tile, tpu)
            t0 *= 8
            total = min(8, T - t0) * M
            out.append("vec" if total % 4 == 0 and (out_align + 4 * (b * out_bs + t0 * M)) % 16 == 0 else "scalar")
        return out

    nw = stream_waves(p, kind)
    if vec4 and nw >= 8 and (segmel or kind == SPEC) and (not src16 or pow2):
        tpw = -(-ntiles // ncu)
        nwg = -(-ntiles // tpw)
        shadow_in = out16 and kind == LOGMEL and pow2
        NL = 16 if (not pow2 or p.L > 416) else 13
        r.update(kernel="feat512_stream_kernel", targs=(KIND_NAMES[kind], pow2, bool(shadow_in), bool(src16 and pow2), NL),
                 nwg=nwg, tiles_per_wg=tpw, waves=min(nw, tpw), store=stores(p.M),
                 shadow=("kernel" if shadow_in else "post") if out16 else None,
                 last_wg_tiles=ntiles - (nwg - 1) * tpw, reach=32 * NL)
        return r
    if src16:
        return dict(r, refused="streaming")
    dct_regs = kind == MFCC and segmel and p.dct_len <= 8
    iters = -(-(-(-ntiles // 4)) // (4 * 256 * FEAT_WAVES))
    r.update(kernel="fused_feat512_kernel", targs=(KIND_NAMES[kind], vec4, pow2, bool(segmel)), dct_regs=dct_regs, iters=iters,
             nwg=-(-ntiles // (4 * iters)), tiles_per_wg=4 * iters, waves=4, store=stores(p.M), shadow="post" if out16 else None)
    return r


def lost_frames(p, d, N, pos):
    """frames of one utterance the kernel of dispatch record d turns NaN for a non-finite sample at `pos`: the frames that own it
    and (section 5) the earlier ones whose loads reach it -- the streaming kernel loads d['reach'] samples per frame, the round-1
    kernel 512 in its interior tiles ((t0 + 7) S + 512 <= (T - 1) S + L) and the frame's own L in the others; nothing is read at
    or behind (T - 1) S + L."""
    T = num_frames(N, p.L, p.S)
    end = (T - 1) * p.S + p.L
    lost = set()
    for t in range(T):
        if d["kernel"] == "feat512_stream_kernel":
            reach = d["reach"]
        elif d["kernel"] == "fused_feat512_kernel":
            t0 = t - t % 8
            reach = 512 if d["vec4"] and (t0 + 7) * p.S + 512 <= end else p.L
        else:
            reach = min(p.L, p.nfft)
        reach = max(reach, min(p.L, p.nfft))
        if t * p.S <= pos < min(t * p.S + reach, end):
            lost.add(t)
    return lost


# ------------------------------------------------------------------------------------------------ float32 transcription of the tile
def _f32(x):
    return np.asarray(x, np.float32)


def _cmul(ar, ai, wr, wi):
    return _f32(_f32(ar * wr) - _f32(ai * wi)), _f32(_f32(ar * wi) + _f32(ai * wr))


def _dft4(x0, x1, x2, x3):
    t0 = (x0[0] + x2[0], x0[1] + x2[1])
    t1 = (x0[0] - x2[0], x0[1] - x2[1])
    t2 = (x1[0] + x3[0], x1[1] + x3[1])
    t3 = (x1[0] - x3[0], x1[1] - x3[1])
    return ((t0[0] + t2[0], t0[1] + t2[1]), (t1[0] + t3[1], t1[1] - t3[0]), (t0[0] - t2[0], t0[1] - t2[1]),
            (t1[0] - t3[1], t1[1] + t3[0]))


def dft16_f32(v):
    """features.hip dft16: v = list of 16 (re, im) float32 arrays in natural order -> X[k] in natural order"""
    C1, S1, H = np.float32(0.92387953251128674), np.float32(0.38268343236508977), np.float32(0.70710678118654752)
    v = list(v)
    for b in range(4):
        v[b], v[4 + b], v[8 + b], v[12 + b] = _dft4(v[b], v[4 + b], v[8 + b], v[12 + b])
    v[5] = _cmul(v[5][0], v[5][1], C1, -S1)
    v[9] = (_f32((v[9][0] + v[9][1]) * H), _f32((v[9][1] - v[9][0]) * H))
    v[13] = _cmul(v[13][0], v[13][1], S1, -C1)
    v[6] = (_f32((v[6][0] + v[6][1]) * H), _f32((v[6][1] - v[6][0]) * H))
    v[10] = (v[10][1], -v[10][0])
    v[14] = (_f32((v[14][1] - v[14][0]) * H), _f32(-(v[14][0] + v[14][1]) * H))
    v[7] = _cmul(v[7][0], v[7][1], S1, -C1)
    v[11] = (_f32((v[11][1] - v[11][0]) * H), _f32(-(v[11][0] + v[11][1]) * H))
    v[15] = _cmul(v[15][0], v[15][1], -C1, S1)
    for c in range(4):
        v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3] = _dft4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3])
    return [v[4 * (k & 3) + (k >> 2)] for k in range(16)]


def _bin_is_pk(k):
    """which member of its conjugate pair bin k is in fft512_power_tile: pk (own twiddle W512^k) or pm (the pair's)"""
    if k == 256:
        return False
    r = k % 16
    if r == 0:
        return k == 0 or k > 128
    if r == 8:
        return k < 128
    return r < 8


def tile_f32(frames, win32, tw256, tw512):
    """float32 transcription of steps 1-6 of a tile: frames [n, <= 512] float32 samples, win32 the plan's float32 Hann table
    (frame_length long).  Returns (Xre, Xim, P): the untangled bins [n, 257] (before squaring) and |X|^2, all float32, in the
    kernel's decomposition: packed 256-point transform as 16 x 16 with the plan's tables, then `untangle`.  (numpy rounds every
    operation; the compiler may contract a * b + c into one fma, so this agrees with the device to rounding, not to the bit.)"""
    n = frames.shape[0]
    x = np.zeros((n, 512), np.float32)
    x[:, :frames.shape[1]] = frames
    w = np.zeros(512, np.float32)
    w[:min(len(win32), 512)] = _f32(0.5) * win32[:512]
    y = x * w
    zr, zi = y[:, 0::2].reshape(n, 16, 16), y[:, 1::2].reshape(n, 16, 16)           # [n][n1][n2]
    A = dft16_f32([(zr[:, n1, :], zi[:, n1, :]) for n1 in range(16)])               # A[k1] -> [n][n2]
    Ar = np.stack([a[0] for a in A], 1)                                             # [n][k1][n2]
    Ai = np.stack([a[1] for a in A], 1)
    Ar, Ai = _cmul(Ar, Ai, tw256.real[None], tw256.imag[None])
    Z = dft16_f32([(Ar[:, :, n2], Ai[:, :, n2]) for n2 in range(16)])               # Z[k2] -> [n][k1]
    Zr = np.stack([z[0] for z in Z], 1).reshape(n, 256)                             # index k2 * 16 + k1 = the bin
    Zi = np.stack([z[1] for z in Z], 1).reshape(n, 256)
    j = np.arange(256)
    m = (256 - j) % 256
    er, ei = Zr[:, j] + Zr[:, m], Zi[:, j] - Zi[:, m]
    orr, oi = Zi[:, j] + Zi[:, m], Zr[:, m] - Zr[:, j]
    wr, wi = _cmul(orr, oi, tw512.real[None], tw512.imag[None])
    ar, ai, br, bi = er + wr, ei + wi, er - wr, ei - wi
    Xre, Xim = np.zeros((n, 257), np.float32), np.zeros((n, 257), np.float32)
    for k in range(257):
        if _bin_is_pk(k):
            Xre[:, k], Xim[:, k] = ar[:, k], ai[:, k]
        else:
            Xre[:, k], Xim[:, k] = br[:, 256 - k], -bi[:, 256 - k]           # pm is |conj(X[256 - j])|^2
    P = _f32(_f32(Xre * Xre) + _f32(Xim * Xim))
    return Xre, Xim, P


def _fma32(a, b, c):
    return _f32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def segmel_f32(p, P):
    """segmel_tile's order in float32: a lane's fma chain over its seg_len bins, then seg_steps shuffle additions; [n, M]"""
    n = P.shape[0]
    acc = np.zeros((n, 64), np.float32)
    for lane, (band, b0, idx, ns) in enumerate(p.lanes):
        for j in range(p.seg_len):
            acc[:, lane] = _fma32(P[:, min(b0 + j, 256)], np.broadcast_to(p.seg_w[j, lane], (n,)), acc[:, lane])
    for st in range(p.seg_steps):
        d = 1 << st
        new = acc.copy()
        for lane, (band, b0, idx, ns) in enumerate(p.lanes):
            if idx + d < ns:
                new[:, lane] = acc[:, lane] + acc[:, lane + d]
        acc = new
    out = np.zeros((n, p.M), np.float32)
    for lane, (band, b0, idx, ns) in enumerate(p.lanes):
        if idx == 0:
            out[:, band] = acc[:, lane]
    return out


def segdct_f32(p, logmel):
    """segdct_tile's order in float32 on a float32 log-mel tile [n, M] -> [n, ncoef]"""
    D = dct_table(p)
    n = logmel.shape[0]
    out = np.zeros((n, p.ncoef), np.float32)
    for c in range(p.ncoef):
        part = np.zeros((n, p.dct_runs), np.float32)
        for run in range(p.dct_runs):
            for j in range(p.dct_len):
                b = run * p.dct_len + j
                if b < p.M:
                    part[:, run] = _fma32(logmel[:, b], np.broadcast_to(D[b, c], (n,)), part[:, run])
        d = 1
        while d < p.dct_runs:
            new = part.copy()
            for run in range(p.dct_runs):
                if run + d < p.dct_runs:
                    new[:, run] = part[:, run] + part[:, run + d]
            part, d = new, d << 1
        out[:, c] = part[:, 0]
    return out


def dct_table(p):
    """the plan's float32 DCT rows [M][ncoef], rounded from double"""
    return fo.dct_matrix(p.M, np.float64)[:, p.coef_begin:p.coef_end].astype(np.float32)


# ------------------------------------------------------------------------------------------------ 3. reference and bounds
def ulp32(v):
    """the spacing of float32 at |v| (normal range)"""
    v = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 23)


def ln_pos_bound(v, claim=2.0):
    """error of ln_pos(acc + 1e-6f) against ln(acc + 1e-6), v = acc + 1e-6 in float64 (docstring section 3); claim = the
    multiple of v_log_f32's stated 1 ulp that is granted"""
    v = np.asarray(v, np.float64)
    return claim * ulp32(np.log2(v)) * math.log(2.0) + 2.0 * U * np.abs(np.log(v)) + 1.05 * U


class Ref:
    pass


def reference(p, x, win32, generic=False, csr=False):
    """float64 reference of every stage on samples x [B, N] (float64, the exact values of the device's samples) with the bound
    of every element.  generic: the kernels of non-fused plans; csr: the CSR mel order of SEGMEL = false."""
    r = Ref()
    Leff = min(p.L, p.nfft)
    fr = fo.frame(np.asarray(x, np.float64), p.L, p.S)[..., :Leff]
    w64 = fo.hann_window(p.L, True, np.float64)[:Leff]
    w32 = win32[:Leff].astype(np.float64)
    with np.errstate(invalid="ignore"):
        r.X = np.fft.rfft(fr * w64, n=p.nfft, axis=-1)
        s_abs = (np.abs(fr) * w32).sum(-1, keepdims=True)
        e_win = (np.abs(fr) * np.abs(w32 - w64)).sum(-1, keepdims=True)
        c = math.sqrt(2.0) * (Leff + 2) if generic else C_FUSED
        r.eX = np.broadcast_to(c * U * s_abs + e_win, r.X.shape)
        aX = np.abs(r.X)
        if p.power == 2.0:
            r.P = aX * aX
            r.eP = 2.0 * aX * r.eX + r.eX ** 2 + 3.0 * U * (aX + r.eX) ** 2
        else:
            r.P = aX ** p.power
            r.eP = None
        W = p.W.astype(np.float64)
        r.mel = r.P @ W
        r.logmel = np.log(r.mel + fo.LOG_EPS)
        D = fo.dct_matrix(p.M, np.float64)[:, p.coef_begin:p.coef_end]
        r.mfcc = r.logmel @ D
        if r.eP is not None:
            terms = (int(p.cnt.max()) if (generic or csr) else p.seg_len + p.seg_steps) + 1
            r.eMel = r.eP @ W + terms * U * ((r.P + r.eP) @ W)
            rel = r.eMel / (r.mel + fo.LOG_EPS)                  # < 1e-3 on every case of the suite; no bound is claimed past 1 / 2
            r.eLog = np.where(rel < 0.5, -np.log1p(-np.minimum(rel, 0.5)), np.inf) + ln_pos_bound(r.mel + fo.LOG_EPS)
            dterms = p.M + int(math.ceil(math.log2(max(p.dct_runs, 1)))) + 1
            r.eMfcc = r.eLog @ np.abs(D) + dterms * U * ((np.abs(r.logmel) + r.eLog) @ np.abs(D))
    return r


def stage(r, kind):
    """(reference, bound) of a kind"""
    return {SPEC: (r.P, r.eP), MEL: (r.mel, getattr(r, "eMel", None)), LOGMEL: (r.logmel, getattr(r, "eLog", None)),
            MFCC: (r.mfcc, getattr(r, "eMfcc", None))}[kind]


# ------------------------------------------------------------------------------------------------ data
def dataset(name, B, N, seed, sample_rate=16000):
    """'normal': 0.1 N(0, 1); 'tone': a 440 Hz tone at 0.5 plus noise at 1e-4 (80 dB between the peak and the floor)"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, N), dtype=np.float32)
    if name == "normal":
        return (np.float32(0.1) * g).astype(np.float32)
    assert name == "tone"
    t = np.arange(N, dtype=np.float64) / sample_rate
    ph = rng.uniform(0, 2 * np.pi, (B, 1))
    return (0.5 * np.sin(2 * np.pi * 440.0 * t[None] + ph) + 1e-4 * g).astype(np.float32)


DATASETS = ("normal", "tone")


# ------------------------------------------------------------------------------------------------ the PATHS table
def _plan_kw(**kw):
    d = dict(sample_rate=16000, L=400, S=160, nfft=512, power=2.0, M=40, fmin=0.0, fmax=8000.0, coef_begin=1, coef_end=13)
    d.update(kw)
    return d


CENSUS_PLAN = dict(M=64, fmax=64000.0)           # not seg_ok (test_oracle_features_paths.py: the census); fmax above Nyquist


def row(name, kind, B, N, expect, plan=None, **call):
    """B: an int or a function of the CU count.  call: src16, sig_misalign (one float / one int16 pair off), sig_stride, out16,
    out_shift (floats), gap (floats between utterances in out).  expect: the dispatch record's fields this row is there for;
    a callable value is a predicate of (field value)."""
    call.setdefault("sig_stride", N if B == 1 else (N + 3) // 4 * 4 + 4)       # rows 16-byte aligned, a gap of 4 to 7 samples behind each
    return dict(name=name, kind=kind, B=B, N=N, expect=expect, plan=_plan_kw(**(plan or {})), call=call)


def _stream(kind, pow2=True, shadow=False, src16=False, NL=13, **more):
    return dict(kernel="feat512_stream_kernel", targs=(KIND_NAMES[kind], pow2, shadow, src16, NL), **more)


def _round1(kind, vec4, pow2=True, segmel=True, **more):
    return dict(kernel="fused_feat512_kernel", targs=(KIND_NAMES[kind], vec4, pow2, segmel and kind != SPEC), **more)


N8 = 1520                       # T = 8 at L = 400, S = 160: one tile per utterance
PATHS = []
# streaming kernel: kinds x power
for _k in (SPEC, MEL, LOGMEL, MFCC):
    PATHS.append(row("stream_%s_p2" % KIND_NAMES[_k], _k, 2, 2000, _stream(_k)))
    PATHS.append(row("stream_%s_p1" % KIND_NAMES[_k], _k, 2, 2000, _stream(_k, pow2=False, NL=16), plan=dict(power=1.0)))
# frame lengths around the NL boundary, steps
for _L, _NL in ((4, 13), (416, 13), (420, 16), (512, 16)):
    PATHS.append(row("stream_L%d" % _L, LOGMEL, 2, _L + 9 * 160 + 3, _stream(LOGMEL, NL=_NL), plan=dict(L=_L)))
    PATHS.append(row("stream_L%d_mfcc" % _L, MFCC, 2, _L + 9 * 160 + 2, _stream(MFCC, NL=_NL), plan=dict(L=_L)))
for _S in (4, 512, 1000):
    PATHS.append(row("stream_S%d" % _S, LOGMEL, 2, 400 + 10 * _S + 1, _stream(LOGMEL), plan=dict(S=_S)))
PATHS.append(row("stream_S4_L512_spec", SPEC, 2, 512 + 10 * 4, _stream(SPEC, NL=16), plan=dict(L=512, S=4)))
# sources and shadows: NL 13 and 16 each
for _L, _NL in ((400, 13), (512, 16)):
    PATHS.append(row("stream_pcm_L%d" % _L, LOGMEL, 3, 2003, _stream(LOGMEL, src16=True, NL=_NL), plan=dict(L=_L), src16=True, sig_stride=2004))
    PATHS.append(row("stream_pcm_mfcc_L%d" % _L, MFCC, 3, 2003, _stream(MFCC, src16=True, NL=_NL), plan=dict(L=_L), src16=True, sig_stride=2004))
    PATHS.append(row("stream_shadow_L%d" % _L, LOGMEL, 3, 2003, _stream(LOGMEL, shadow=True, NL=_NL, shadow_by="kernel"), plan=dict(L=_L),
                     out16=True, sig_stride=2004))
    PATHS.append(row("stream_pcm_shadow_L%d" % _L, LOGMEL, 3, 2003, _stream(LOGMEL, shadow=True, src16=True, NL=_NL, shadow_by="kernel"),
                     plan=dict(L=_L), src16=True, out16=True, sig_stride=2004))
PATHS.append(row("stream_pcm_spec", SPEC, 2, 2000, _stream(SPEC, src16=True), src16=True))
PATHS.append(row("stream_pcm_mel", MEL, 2, 2000, _stream(MEL, src16=True), src16=True))
PATHS.append(row("stream_L512_mel", MEL, 2, 2000, _stream(MEL, NL=16), plan=dict(L=512)))
PATHS.append(row("stream_pcm_spec_L512", SPEC, 2, 2000, _stream(SPEC, src16=True, NL=16), plan=dict(L=512), src16=True))
PATHS.append(row("stream_pcm_mel_L512", MEL, 2, 2000, _stream(MEL, src16=True, NL=16), plan=dict(L=512), src16=True))
PATHS.append(row("stream_shadow_post_mel", MEL, 2, 2000, _stream(MEL, shadow_by="post"), out16=True))
PATHS.append(row("stream_shadow_post_mfcc", MFCC, 2, 2000, _stream(MFCC, shadow_by="post"), out16=True))
PATHS.append(row("stream_shadow_post_spec", SPEC, 2, 2000, _stream(SPEC, shadow_by="post"), out16=True))
PATHS.append(row("stream_shadow_post_p1", LOGMEL, 2, 2000, _stream(LOGMEL, pow2=False, NL=16, shadow_by="post"), plan=dict(power=1.0), out16=True))
# store_mel_tile: out one float off -> every tile scalar; aligned with T % 8 = 0 -> every tile vector; a last tile of 7 frames of
# 13 bands -> scalar by the count; one float off with a gap of 3 floats -> utterance 1 is 16-byte aligned again (vector stores, the
# shadow's 8-byte stores then 6 bytes past a multiple of 8)
PATHS.append(row("store_vec", LOGMEL, 2, N8 + 160 * 8, _stream(LOGMEL, shadow=True, shadow_by="kernel", store=lambda s: set(s) == {"vec"}), out16=True))
PATHS.append(row("store_misaligned_out", LOGMEL, 2, N8 + 160 * 8, _stream(LOGMEL, store=lambda s: set(s) == {"scalar"}), out_shift=1))
PATHS.append(row("store_misaligned_out_shadow", LOGMEL, 2, N8 + 160 * 8, _stream(LOGMEL, shadow=True, shadow_by="kernel", store=lambda s: set(s) == {"scalar"}),
                 out16=True, out_shift=1))
PATHS.append(row("store_realigned_shadow", LOGMEL, 2, N8 + 160 * 8, _stream(LOGMEL, shadow=True, shadow_by="kernel",
                                                                            store=lambda s: s == ["scalar", "scalar", "vec", "vec"]),
                 out16=True, out_shift=1, gap=3))
PATHS.append(row("store_odd_count", MEL, 2, 400 + 14 * 160, _stream(MEL, store=lambda s: s == ["vec", "scalar", "scalar", "scalar"]), plan=dict(M=13, coef_end=13)))
# T and N % 4
for _T, _r in ((1, 0), (7, 1), (8, 2), (9, 3), (17, 1)):
    PATHS.append(row("stream_T%d" % _T, LOGMEL, 3, 400 + (_T - 1) * 160 + _r, _stream(LOGMEL, T=_T), sig_stride=400 + (_T - 1) * 160 + 4))
    PATHS.append(row("stream_T%d_spec" % _T, SPEC, 3, 400 + (_T - 1) * 160 + _r, _stream(SPEC, T=_T), sig_stride=400 + (_T - 1) * 160 + 4))
# the work split at T = 8: tiles = utterances
PATHS.append(row("split_1", LOGMEL, 1, N8, _stream(LOGMEL, nwg=1, tiles_per_wg=1, waves=1)))
PATHS.append(row("split_ncu-1", LOGMEL, lambda ncu: ncu - 1, N8, _stream(LOGMEL, tiles_per_wg=1, waves=1, nwg=lambda v: v >= 1)))
PATHS.append(row("split_ncu", MFCC, lambda ncu: ncu, N8, _stream(MFCC, tiles_per_wg=1, waves=1, nwg=lambda v: v >= 1)))
PATHS.append(row("split_ncu+1", LOGMEL, lambda ncu: ncu + 1, N8, _stream(LOGMEL, tiles_per_wg=2, waves=2)))
PATHS.append(row("split_2ncu+3", MEL, lambda ncu: 2 * ncu + 3, N8, _stream(MEL, tiles_per_wg=3, waves=3)))
PATHS.append(row("split_16ncu+5", LOGMEL, lambda ncu: 16 * ncu + 5, N8, _stream(LOGMEL, tiles_per_wg=17, waves=16)))
PATHS.append(row("split_16ncu+5_spec", SPEC, lambda ncu: 16 * ncu + 5, N8, _stream(SPEC, tiles_per_wg=17, waves=16)))
# round-1 kernel: one float off (VEC4 false), L = 402 / S = 162 / sig_stride % 4 != 0
for _k in (SPEC, MEL, LOGMEL, MFCC):
    PATHS.append(row("r1_%s_p2" % KIND_NAMES[_k], _k, 2, 2000, _round1(_k, False), sig_misalign=True))
    PATHS.append(row("r1_%s_p1" % KIND_NAMES[_k], _k, 2, 2000, _round1(_k, False, pow2=False), plan=dict(power=1.0), sig_misalign=True))
PATHS.append(row("r1_L402", LOGMEL, 2, 2001, _round1(LOGMEL, False), plan=dict(L=402)))
PATHS.append(row("r1_S162", MFCC, 2, 2001, _round1(MFCC, False, dct_regs=True), plan=dict(S=162)))
PATHS.append(row("r1_stride", MEL, 3, 2000, _round1(MEL, False), sig_stride=2002))
PATHS.append(row("r1_dct_len9", MFCC, 2, 2000, _round1(MFCC, False, dct_regs=False), plan=dict(M=45, coef_end=13), sig_misalign=True))
PATHS.append(row("r1_shadow_post", LOGMEL, 2, 2000, _round1(LOGMEL, False, shadow_by="post"), sig_misalign=True, out16=True))
# SEGMEL = false: the census plan; aligned rows (VEC4 true, interior and guarded tiles: T = 17 has one interior tile) and misaligned
for _k in (MEL, LOGMEL, MFCC):
    PATHS.append(row("csr_vec4_%s" % KIND_NAMES[_k], _k, 2, 400 + 16 * 160 + 4, _round1(_k, True, segmel=False), plan=CENSUS_PLAN))
    PATHS.append(row("csr_vec4_%s_p1" % KIND_NAMES[_k], _k, 2, 400 + 16 * 160, _round1(_k, True, pow2=False, segmel=False),
                     plan=dict(CENSUS_PLAN, power=1.0)))
    PATHS.append(row("csr_scalar_%s" % KIND_NAMES[_k], _k, 2, 400 + 16 * 160 + 1, _round1(_k, False, segmel=False), plan=CENSUS_PLAN, sig_misalign=True))
for _k in (MEL, LOGMEL, MFCC):
    PATHS.append(row("csr_scalar_%s_p1" % KIND_NAMES[_k], _k, 2, 2000, _round1(_k, False, pow2=False, segmel=False),
                     plan=dict(CENSUS_PLAN, power=1.0), sig_misalign=True))
# iters = 2
PATHS.append(row("r1_iters2", LOGMEL, 12289, N8, _round1(LOGMEL, False, iters=2, tiles_per_wg=8), sig_misalign=True))
# mel plans: seg_len / seg_steps
# (found by the census of tests/test_oracle_features_paths.py; the last one has bands above Nyquist: cnt = 0, one idle lane each)
for _M, _sr, _fmin, _fmax, _sl, _st, _zero in ((1, 8000, 0.0, 1000.0, 1, 6, False), (64, 8000, 300.0, 1000.0, 2, 0, False),
                                              (64, 16000, 0.0, 2000.0, 4, 0, True), (23, 8000, 0.0, 2000.0, 5, 2, False),
                                              (45, 8000, 0.0, 4000.0, 11, 2, False), (64, 16000, 0.0, 8000.0, 20, 0, False),
                                              (64, 8000, 0.0, 32000.0, 32, 0, True)):
    for _k in (MEL, MFCC):
        PATHS.append(row("mel_M%d_seglen%d_%s" % (_M, _sl, KIND_NAMES[_k]), _k, 2, 2000,
                         _stream(_k, seg_len=_sl, seg_steps=_st, zero_bands=_zero),
                         plan=dict(M=_M, sample_rate=_sr, fmin=_fmin, fmax=_fmax, coef_begin=0, coef_end=min(13, _M))))
# DCT plans
for _nc, _M in ((1, 40), (12, 40), (20, 40), (13, 13), (40, 25), (64, 16)):
    for _cb in (0, 1):
        _ce = min(_cb + _nc, _M)
        PATHS.append(row("dct_%d_%d_cb%d" % (_nc, _M, _cb), MFCC, 2, 2000, _stream(MFCC), plan=dict(M=_M, coef_begin=_cb, coef_end=_ce)))
PATHS.append(row("dct_r1_%d_%d" % (20, 40), MFCC, 2, 2000, _round1(MFCC, False, dct_regs=False), plan=dict(M=40, coef_begin=0, coef_end=20), sig_misalign=True))
PATHS.append(row("dct_r1_%d_%d" % (64, 16), MFCC, 2, 2000, _round1(MFCC, False, dct_regs=True), plan=dict(M=16, coef_begin=0, coef_end=64), sig_misalign=True))
# fused_ok boundary
PATHS.append(row("fused_M64", LOGMEL, 2, 2000, _stream(LOGMEL), plan=dict(M=64)))
PATHS.append(row("generic_M65", LOGMEL, 2, 2000, dict(kernel="pow2_fft_spectrogram_kernel"), plan=dict(M=65)))
PATHS.append(row("fused_64x16", MFCC, 2, 2000, _stream(MFCC), plan=dict(M=64, coef_begin=0, coef_end=16)))
PATHS.append(row("generic_64x17", MFCC, 2, 2000, dict(kernel="pow2_fft_spectrogram_kernel"), plan=dict(M=64, coef_begin=0, coef_end=17)))
PATHS.append(row("fused_L512", SPEC, 2, 2000, _stream(SPEC, NL=16), plan=dict(L=512)))
PATHS.append(row("generic_L513", SPEC, 2, 2000, dict(kernel="pow2_fft_spectrogram_kernel", Leff=512), plan=dict(L=513)))
PATHS.append(row("generic_L600", MEL, 2, 2000, dict(kernel="pow2_fft_spectrogram_kernel", Leff=512), plan=dict(L=600)))


def reachable():
    """every (kernel, template arguments) lidbox_extract_features_fwd_ex can select for a fused plan, plus the generic transform the
    boundary rows take.  Streaming (launch_stream): POW2 = false only plain with NL = 16; POW2 = true with SRC16 and NL free, SHADOW
    on log-mel only: 4 + 16 + 4 = 24.  Round-1 (launch_fused): VEC4 = false with every kind, POW2 and (mel kinds) SEGMEL: 14; VEC4 =
    true only with SEGMEL = false on the mel kinds (an aligned signal of a seg_ok plan or of the spectrogram streams): 6."""
    out = {("pow2_fft_spectrogram_kernel",)}
    for k in KIND_NAMES.values():
        out.add(("feat512_stream_kernel", k, False, False, False, 16))
        for nl in (13, 16):
            for src16 in (False, True):
                out.add(("feat512_stream_kernel", k, True, False, src16, nl))
                if k == "LOGMEL":
                    out.add(("feat512_stream_kernel", k, True, True, src16, nl))
        for pow2 in (False, True):
            if k == "SPECTROGRAM":
                out.add(("fused_feat512_kernel", k, False, pow2, False))
            else:
                for segmel in (False, True):
                    out.add(("fused_feat512_kernel", k, False, pow2, segmel))
                out.add(("fused_feat512_kernel", k, True, pow2, False))
    return out


def resolve(r, lib, ncu):
    """(plan, dispatch record, B) of a PATHS row at a CU count"""
    kw = dict(r["plan"])
    W = host_mel_matrix(lib, kw.pop("M"), kw["nfft"] // 2 + 1, kw["sample_rate"], kw.pop("fmin"), kw.pop("fmax"))
    p = make_plan(W, **kw)
    B = r["B"](ncu) if callable(r["B"]) else r["B"]
    c = r["call"]
    src16 = bool(c.get("src16"))
    d = dispatch(p, r["kind"], B, r["N"], ncu, src16=src16, sig_align=(2 if src16 else 4) if c.get("sig_misalign") else 0,
                 sig_stride=c.get("sig_stride"), out16=bool(c.get("out16")), out_align=4 * c.get("out_shift", 0),
                 out_bs=(num_frames(r["N"], p.L, p.S) * {SPEC: p.F, MEL: p.M, LOGMEL: p.M, MFCC: p.ncoef}[r["kind"]] + c["gap"]) if c.get("gap") else 0)
    return p, d, B


def check_expect(r, p, d):
    """every field the row is there for; returns the list of mismatches"""
    bad = []
    for key, want in r["expect"].items():
        if key == "shadow_by":
            got = d["shadow"]
        elif key in ("seg_len", "seg_steps"):
            got = getattr(p, key)
        elif key == "zero_bands":
            got = bool((p.cnt == 0).any())
        else:
            got = d.get(key)
        ok = want(got) if callable(want) else got == want
        if not ok:
            bad.append((key, got))
    return bad
