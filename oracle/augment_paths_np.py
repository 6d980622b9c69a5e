"""
The augmentation kernels (csrc/augment.hip: lidbox_resample, lidbox_fir_filter; csrc/mix_noise.hip: lidbox_mix_noise,
lidbox_signal_tile) restated for their path tests: the host dispatch as plain functions, float64 references, a model of the
resampler's own pipeline that can carry one planted mistake, and the PATHS tables.  tests/test_oracle_augment_paths.py pins
all of it on the CPU, tests/test_augment_paths_gpu.py runs every row through the C ABI.  TEST INFRASTRUCTURE ONLY (see
oracle/__init__.py).

1. DISPATCH.  Every function quotes the source condition it restates.  Resample: rs_k, rs_logp, rs_stage (LDS or four-step
   form, log1 / log2, block threads, where the radix-2 stage sits, tile sizes, grid), rs_groups (stable sort by logP, at most
   RS_GROUP per launch, slot offsets), rs_workspace, digit_perm.  FIR: fir_plan, fir_trips, fir_store_vec.  Mix: mix_form,
   mix_tiles, mix_workspace, periodic_branch / mix_branches.  Tile: tile_plan.  Note on the tile loop: a strip block covers
   256 x 4 = 1024 samples per trip while the grid has cdiv(max_out, 4096) strips, so every output above 4096 samples takes
   four trips and one above 1024 x 4096 samples takes a fifth; tile_plan states what the code does.

2. REFERENCES (float64).  resample_ref: Y[:K] = rfft(x)[:K], bin min/2 doubled if M < N and halved if M > N when min(N, M) is
   even, irfft(Y, M) M / N (scipy.signal.resample's Fourier method).  fir_ref: the direct sum and the same sum on absolute
   values.  mix_ref: signal_np.snr_mixer on np.resize(clip, n).  Tile: np.tile.

3. MODEL.  rs_model(xs, ms, mut, dt) walks a batch through the kernel's pipeline with the kernel's memory layout: groups and
   slots of rs_groups inside one `region` array, the spectra in one `spec` array pitched by kmax; per utterance and stage the
   chirp pre-multiply, the zero-padded circular convolution of size P with the chirp filter (d in [0, out), P - d for d in
   [1, in)), the chirp post-multiply; the stage-0 epilogue (imaginary part of bin 0 and of bin M/2 dropped, Nyquist factor,
   half spectrum doubled); stage 1; / N.  P > 2^14 goes through the four-step factorisation (column transforms, twiddle
   W_P^(n2 k1), row transforms) in natural order: the kernel's digit-reversed order is a relabelling of the same products
   (digit_perm, pinned separately against a literal radix-4 / radix-2 walk).  dt = float64 is the model proper; dt = float32
   runs the same pipeline with complex64 data and a plain radix-2 transform, trigonometric values rounded from float64 (the
   device's sincospif is accurate to about an ulp).  It is what the issue's rule for replacing a bound refers to; no bound
   is replaced (RS_TOL_OVERRIDE is empty).
   MUTATIONS plants one mistake each: no_nyquist, no_double (one bin), keep_imag_m2, drop_last_tap, bad_twiddle, spec_pitch,
   slot_255.  tests/test_oracle_augment_paths.py shows for each that some row marked for it leaves the tolerance, or that none
   does, and then it is listed here:
   UNDETECTABLE.  keep_imag_m2 -- bin M/2 (present when M <= N, M even) is not doubled and meets the phase e^{i pi n} = +-1 in
   stage 1, so its imaginary part lands in the imaginary part of the output sample, which is dropped: the same reason for which
   the imaginary part of bin 0 cannot be seen.  slot_255 -- the launches of a group are complete before the next group's
   begin (one stream), so a next group that starts one slot early overwrites a slot nobody reads again; the values cannot
   show it.  (A slot offset that is too LARGE would leave the workspace, which the guard words of an exactly sized
   workspace show.)

4. TOLERANCES.  Resample: the project's relative L2 error <= 4e-6 and max error <= 4e-6 max|x| (tests/test_augment_gpu.py).
   FIR: conv2d_np.error_bound(S, K), S the sum on absolute values: one product and K - 1 fused multiply-adds in fixed order
   are K roundings.  Mix: the project's 2e-5 max|ref| (tests/test_dataset_steps_gpu.py).  Tile: bit-exact.

5. DATA.  draw(kind, n, seed): "normal" N(0, 1); "offset" 1 + 0.1 N(0, 1); "nyquist" (-1)^n + 1e-3 N(0, 1), resample only and
   for utterances with N even and M >= N (rs_kind_of).  For M < N the resampler removes bin N/2: what is left of the tone
   data set is the 1e-3 noise, against whose norm the rounding of a unit-amplitude input cannot be held to 4e-6; these
   utterances (and those with N odd) get "normal" in the third set.  FIR rows with K >= 4095 run a third set too, "sparse"
   (fir_coefs): error_bound(S, 4096) is 2.4e-4 S, about one whole term of a dense 4096-tap sum, so a single lost or misplaced
   sample of the halo hides inside it; with sixteen live taps S is that much smaller while the chain, its length and so the
   bound's form stay the same (a zero tap is an exact fused multiply-add), and one lost sample is a large multiple of it.
"""
import os
import re

import numpy as np

from oracle import signal_np
from oracle.conv2d_np import error_bound, gamma  # noqa: F401

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidbox_amd", "csrc")

RS_MAX_LOG_LEN, RS_LDS_LOG, RS_TILE_LOG, RS_TW_LOG = 21, 14, 12, 14
RS_TILE_THREADS, RS_THREADS, RS_GROUP = 256, 1024, 256
FIR_THREADS, FIR_PER_LANE, FIR_TILE, FIR_MAX_TILES, FIR_MAX_COEFS = 256, 8, 2048, 64, 4096
MIX_REG_MAX, MIX_TILE, MIX_MAX_TILES, MIX_MAX_LOG_LEN = 65536, 8192, 256, 21
TILE_STRIP, TILE_MAX_STRIPS, TILE_PER_TRIP = 4096, 1024, 1024
RS_TOL = 4e-6
MIX_TOL = 2e-5
RS_TOL_OVERRIDE = {}            # (row name, kind) -> 4 x the float32 model's error; empty: no row needed it
KINDS = ("normal", "offset")
RS_KINDS = ("normal", "offset", "nyquist")


def cdiv(a, b):
    return -(-a // b)


def ceil_log2(v):
    """`while ((1L << l) < v) ++l`"""
    l = 0
    while (1 << l) < v:
        l += 1
    return l


# ---------------------------------------------------------------------------------------------------- 1. dispatch: resample
def rs_k(N, M):
    """`K = std::min(N, M) / 2 + 1`"""
    return min(N, M) // 2 + 1


def rs_logp(N, M):
    """`if (N == 0 || M == 0) continue; logP[0] = ceil_log2(N + K - 1); logP[1] = ceil_log2(K + M - 1)`"""
    if N == 0 or M == 0:
        return None
    K = rs_k(N, M)
    return ceil_log2(N + K - 1), ceil_log2(K + M - 1)


def rs_stage(logP):
    """the launch of one group of transforms of 2^logP points"""
    four = logP > RS_LDS_LOG                                  # `a.log1 = logP > RS_LDS_LOG ? logP / 2 : 0`
    log1 = logP // 2 if four else 0
    log2 = logP - log1                                        # `a.log2 = logP - a.log1`
    if four:
        return dict(form="four", log1=log1, log2=log2,
                    threads=RS_TILE_THREADS,                   # `block(RS_TILE_THREADS)`
                    grid=1 << (logP - RS_TILE_LOG),           # `grid(1u << (logP - RS_TILE_LOG), cnt)`
                    col_tile=1 << (RS_TILE_LOG - log1),       # `logT = RS_TILE_LOG - a.log1` columns per workgroup
                    row_tile=1 << (RS_TILE_LOG - log2),       # `logR = RS_TILE_LOG - a.log2` rows per workgroup
                    lds=(1 << RS_TILE_LOG) * 8,
                    r2_cols=bool(log1 & 1), r2_rows=bool(log2 & 1),          # `if (logm == 1) radix2_stage`
                    kernels={"rs_col_fwd_kernel<true>", "rs_row_kernel<false>", "rs_col_fwd_kernel<false>",
                             "rs_row_kernel<true>", "rs_col_inv_kernel"})
    return dict(form="lds", log1=0, log2=log2,
                threads=min(RS_THREADS, max(64, (1 << logP) // 8)),          # `block(std::min(RS_THREADS, std::max(64, (1 << logP) / 8)))`
                grid=1, col_tile=None, row_tile=1,                          # `logR = a.log1 ? ... : 0`
                lds=(1 << logP) * 8, r2_cols=False, r2_rows=bool(logP & 1),
                kernels={"rs_row_kernel<false>", "rs_row_kernel<true>"})


def rs_groups(utts, stage, slot_count=None):
    """the launches of one stage: [(logP, [utterance indices], slot offset in points)].  `std::stable_sort` by logP, groups of
    `cnt < RS_GROUP` equal sizes, `slot += (size_t)cnt * 2 << logP`.  slot_count replaces cnt in that sum (a planted mistake)"""
    lp = [rs_logp(N, M) for N, M in utts]
    order = sorted((b for b in range(len(utts)) if lp[b] is not None), key=lambda b: lp[b][stage])       # sorted() is stable
    out, g, slot = [], 0, 0
    while g < len(order):
        logP = lp[order[g]][stage]
        cnt = 0
        while g + cnt < len(order) and cnt < RS_GROUP and lp[order[g + cnt]][stage] == logP:
            cnt += 1
        out.append((logP, order[g:g + cnt], slot))
        slot += ((cnt if slot_count is None else slot_count) * 2) << logP
        g += cnt
    return out


def rs_plan(utts):
    """kmax, the points of each stage's slots, the number of active utterances"""
    act = [(N, M) for N, M in utts if N and M]
    kmax = max([rs_k(N, M) for N, M in act], default=0)
    pts = [sum(2 << rs_logp(N, M)[s] for N, M in act) for s in (0, 1)]
    return kmax, pts, len(act)


def rs_workspace(utts):
    """`twiddles | spectra (B x kmax) | the slots of the larger stage`, 0 when no utterance has work"""
    kmax, pts, active = rs_plan(utts)
    if not active:
        return 0
    return (1 << RS_TW_LOG) * 8 + len(utts) * kmax * 8 + max(pts) * 8


def rs_select(utts):
    """what a batch launches"""
    sel = dict(kernels=set(), stages=[], groups=[])
    if any(N and M for N, M in utts):
        sel["kernels"].add("rs_twiddle_kernel")
    for stage in (0, 1):
        gs = rs_groups(utts, stage)
        sel["groups"].append([(logP, len(u), slot) for logP, u, slot in gs])
        sel["stages"].append(sorted({logP for logP, _, _ in gs}))
        for logP, _, _ in gs:
            sel["kernels"] |= rs_stage(logP)["kernels"]
    return sel


def digit_perm(j, logn):
    """the frequency held at position j after the forward stages (radix-4 digits from the largest block down, then radix 2)"""
    k, sh, logm = 0, 0, logn
    while logm >= 2:
        logm -= 2
        k |= ((j >> logm) & 3) << sh
        sh += 2
    if logm == 1:
        k |= (j & 1) << sh
    return k


def lds_fft_forward(a):
    """the forward stages of lds_fft walked literally in float64 (radix-4 from the largest block down, one radix-2 at the end
    when log n is odd): natural order in, the order of digit_perm out"""
    a = np.array(a, np.complex128)
    n = len(a)
    logn = ceil_log2(n)
    logm = logn
    while logm >= 2:
        m, q = 1 << logm, 1 << (logm - 2)
        for base in range(0, n, m):
            for j in range(q):
                x0, x1, x2, x3 = (a[base + j + i * q] for i in range(4))
                w = [np.exp(-2j * np.pi * i * j / m) for i in range(4)]
                s02, d02, s13, d13 = x0 + x2, x0 - x2, x1 + x3, x1 - x3
                a[base + j] = s02 + s13
                a[base + j + q] = (d02 - 1j * d13) * w[1]
                a[base + j + 2 * q] = (s02 - s13) * w[2]
                a[base + j + 3 * q] = (d02 + 1j * d13) * w[3]
        logm -= 2
    if logm == 1:
        for b in range(0, n, 2):
            a[b], a[b + 1] = a[b] + a[b + 1], a[b] - a[b + 1]
    return a


# ---------------------------------------------------------------------------------------------------- 1. dispatch: FIR
def fir_plan(max_len, K):
    tiles = min(cdiv(max_len, FIR_TILE), FIR_MAX_TILES)      # `std::min<long>(lbx_cdiv(max_length, FIR_TILE), 64)`
    halo = (K + 2) // 4 * 4 + 4                              # `fir_halo`
    return dict(tiles=tiles, halo=halo,
                lds=((K + 3) // 4 * 4 + halo + FIR_TILE) * 4,
                main=K // 4,                                  # `for (; 4 * q + 4 <= K; ++q)`
                tail=K % 4)                                   # `the last K mod 4 taps`


def fir_trips(n, tiles):
    """trips of block y = 0 through `for (t0 = blockIdx.y * FIR_TILE; t0 < n; t0 += gridDim.y * FIR_TILE)`"""
    return cdiv(n, tiles * FIR_TILE)


def fir_store_vec(s, j0, n):
    """`((s + j0) & 3) == 0 && j0 + FIR_PER_LANE <= n`: the two-float4 store"""
    return (s + j0) % 4 == 0 and j0 + FIR_PER_LANE <= n


def fir_stores(s, n):
    """the store forms the lanes of an utterance take"""
    return {"vec" if fir_store_vec(s, j0, n) else "scalar" for j0 in range(0, n, FIR_PER_LANE)}


# ---------------------------------------------------------------------------------------------------- 1. dispatch: mix, tile
MIX_FORMS = {"reg<4,0>": "mix_reg_kernel<4,0>", "reg<8,0>": "mix_reg_kernel<8,0>", "reg<8,8>": "mix_reg_kernel<8,8>"}


def mix_form(n):
    """`need[n <= 4096L * 4 ? 0 : (n <= 4096L * 8 ? 1 : 2)]`, `if (n > MIX_REG_MAX) *any_tiled = true`"""
    if n <= 0:
        return None
    if n > MIX_REG_MAX:
        return "tiled"
    return "reg<4,0>" if n <= 4096 * 4 else ("reg<8,0>" if n <= 4096 * 8 else "reg<8,8>")


def mix_kernels(ns):
    out = set()
    for n in ns:
        f = mix_form(n)
        if f == "tiled":
            out |= {"mix_tile_kernel<0>", "mix_tile_kernel<1>", "mix_tile_kernel<2>"}
        elif f:
            out.add(MIX_FORMS[f])
    return out


def mix_tiles(max_len):
    """`grid(J, lbx_cdiv(max_len, MIX_TILE))`"""
    return cdiv(max_len, MIX_TILE) if max_len > MIX_REG_MAX else 0


def mix_workspace(max_len, J):
    """`if (J <= 0 || max_length <= MIX_REG_MAX) return 0; return 2 * J * MIX_MAX_TILES * sizeof(float2)`"""
    return 0 if J <= 0 or max_len <= MIX_REG_MAX else 2 * J * MIX_MAX_TILES * 8


def periodic_branch(m, i, res):
    """periodic_load4 of a clip of m samples whose first sample sits `res` words past a 16-byte boundary, at index i:
    `if (p + 3 < m && (((uintptr_t)q) & 15) == 0)` one aligned 16-byte load ("vec"), else the wrapping loop ("loop")"""
    p = i % m if i >= m else i
    return "vec" if p + 3 < m and (res + p) % 4 == 0 else "loop"


def mix_branches(n, m, res):
    """both counts over the accesses o = 0, 4, .. < n of one output"""
    o = np.arange(0, n, 4, dtype=np.int64)
    p = o % m
    vec = (p + 3 < m) & ((res + p) % 4 == 0)
    return dict(vec=int(vec.sum()), loop=int((~vec).sum()))


def tile_plan(max_out, total):
    """`strips = std::min<long>(lbx_cdiv(max_out_length, 4096), 1024)`; trips of strip 0 through
    `for (o = (blockIdx.y * 256 + threadIdx.x) * 4; o < total; o += gridDim.y * 1024)`"""
    strips = min(cdiv(max_out, TILE_STRIP), TILE_MAX_STRIPS)
    return dict(strips=strips, trips=cdiv(total, strips * TILE_PER_TRIP) if strips else 0)


def launch_site_kernels():
    """the first argument of every hipLaunchKernelGGL of the two files, read from the source text; constants that appear as
    template arguments are replaced by their values"""
    out = {}
    for fn in ("augment.hip", "mix_noise.hip"):
        with open(os.path.join(CSRC, fn)) as f:
            src = f.read()
        consts = dict(re.findall(r"constexpr int (\w+) = (\d+);", src))
        names = set()
        for name in re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+(?:<[^>]*>)?)", src):
            name = name.replace(" ", "")
            for c, v in consts.items():
                name = re.sub(r"\b%s\b" % c, v, name)
            names.add(name)
        out[fn] = names
    return out


# ---------------------------------------------------------------------------------------------------- 2. references
def resample_ref(x, M):
    x = np.asarray(x, np.float32).astype(np.float64)
    N = len(x)
    if M == 0 or N == 0:
        return np.zeros(M)
    K, mn = rs_k(N, M), min(N, M)
    Y = np.fft.rfft(x)[:K].copy()
    if mn % 2 == 0:
        if M < N:
            Y[mn // 2] *= 2.0
        elif M > N:
            Y[mn // 2] *= 0.5
    return np.fft.irfft(Y, M) * M / N


def rs_errors(y, ref, x):
    """(relative L2 error, max error / max|x|)"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    if not len(ref):
        return 0.0, 0.0
    d = y - ref
    return float(np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-30)), float(np.abs(d).max() / np.abs(x).max())


def fir_ref(x, f):
    """(y, S): y[n] = sum_k f[k] x[n - k] and S[n] = sum_k |f[k]| |x[n - k]|"""
    x, f = np.asarray(x, np.float32).astype(np.float64), np.asarray(f, np.float32).astype(np.float64)
    n = len(x)
    return np.convolve(x, f)[:n], np.convolve(np.abs(x), np.abs(f))[:n]


def mix_ref(clean, clip, snr):
    clean = np.asarray(clean, np.float32).astype(np.float64)
    clip = np.asarray(clip, np.float32).astype(np.float64)
    return signal_np.snr_mixer(clean, np.resize(clip, len(clean)), snr)[2]


# ---------------------------------------------------------------------------------------------------- 3. the pipeline model
MUTATIONS = ("no_nyquist", "no_double", "keep_imag_m2", "drop_last_tap", "bad_twiddle", "spec_pitch", "slot_255")
UNDETECTABLE = ("keep_imag_m2", "slot_255")


def _cis(num, den, sgn, dt):
    """e^{i sgn pi num / den}: the ratio in dt, the trigonometric values rounded from float64"""
    a = (np.asarray(num).astype(dt) / dt(den)).astype(np.float64) * np.pi
    cdt = np.complex128 if dt is np.float64 else np.complex64
    return (np.cos(a) + 1j * sgn * np.sin(a)).astype(cdt)


def _chirp(n, L, sgn, dt):
    """`r = (n * n) % (2 * L); sincospif((float)r / (float)L)`"""
    n = np.asarray(n, np.int64)
    return _cis((n * n) % (2 * L), L, sgn, dt)


def _bitrev(n):
    r = np.zeros(1, np.int64)
    while len(r) < n:
        r = np.concatenate([2 * r, 2 * r + 1])
    return r


def _fft(a, inv, dt):
    """unnormalised transform along the last axis (e^{-..} forward, e^{+..} inverse); float32: radix 2 in complex64"""
    if dt is np.float64:
        return np.fft.ifft(a, axis=-1) * a.shape[-1] if inv else np.fft.fft(a, axis=-1)
    n = a.shape[-1]
    a = np.ascontiguousarray(a[..., _bitrev(n)], np.complex64)
    half = 1
    while half < n:
        w = _cis(np.arange(half), half, 1.0 if inv else -1.0, dt)
        v = a.reshape(a.shape[:-1] + (n // (2 * half), 2, half))
        t = v[..., 1, :] * w
        a = np.stack([v[..., 0, :] + t, v[..., 0, :] - t], axis=-2).reshape(a.shape)
        half *= 2
    return a


def _twiddle(log1, log2, dt, bad):
    """W_P^(k1 n2) as [N1, N2]; bad: row k1 = 5 takes the exponent of k1 = 4 (its lowest digit wrong)"""
    k1 = np.arange(1 << log1, dtype=np.int64)
    if bad:
        k1[5] = 4
    P = 1 << (log1 + log2)
    return _cis((k1[:, None] * np.arange(1 << log2, dtype=np.int64)[None, :]) % P, P // 2, -1.0, dt)


def _transform(a, logP, inv, dt, bad=False):
    """the kernel's transform of 2^logP points; the four-step form keeps its spectrum as [k1, k2] (X[k1 + N1 k2])"""
    st = rs_stage(logP)
    if st["form"] == "lds":
        return _fft(a, inv, dt)
    log1, log2 = st["log1"], st["log2"]
    if not inv:
        c = _fft(a.reshape(1 << log1, 1 << log2).T, False, dt).T                  # N1-point transforms down the columns
        return _fft(c * _twiddle(log1, log2, dt, bad), False, dt).reshape(-1)
    d = _fft(a.reshape(1 << log1, 1 << log2), True, dt) * np.conj(_twiddle(log1, log2, dt, False))
    return _fft(d.T, True, dt).T.reshape(-1)


def rs_model(xs, ms, mut=None, dt=np.float64):
    """the outputs of a batch through the kernel's pipeline and memory layout; mut: one of MUTATIONS"""
    assert mut is None or mut in MUTATIONS
    cdt = np.complex128 if dt is np.float64 else np.complex64
    utts = [(len(x), int(m)) for x, m in zip(xs, ms)]
    kmax, pts, _ = rs_plan(utts)
    spec = np.zeros(len(utts) * kmax, cdt)
    region = np.zeros(max(pts), cdt)
    ys = [np.zeros(M, dt) for _, M in utts]
    for stage in (0, 1):
        for logP, members, slot in rs_groups(utts, stage, 255 if mut == "slot_255" else None):
            P = 1 << logP
            for i, b in enumerate(members):                                       # the filter's transform, scaled by 1 / P
                N, M = utts[b]
                K = rs_k(N, M)
                nin, nout, L, s = (N, K, N, 1.0) if stage == 0 else (K, M, M, -1.0)
                filt = np.zeros(P, cdt)
                filt[:nout] = _chirp(np.arange(nout), L, s, dt)
                d = np.arange(1, nin - (1 if mut == "drop_last_tap" else 0))
                filt[P - d] = _chirp(d, L, s, dt)
                base = slot + 2 * P * i
                region[base:base + P] = _transform(filt, logP, False, dt) * dt(1.0 / P)
            for i, b in enumerate(members):
                N, M = utts[b]
                K = rs_k(N, M)
                nout = K if stage == 0 else M
                data = np.zeros(P, cdt)
                if stage == 0:
                    data[:N] = _chirp(np.arange(N), N, -1.0, dt) * np.asarray(xs[b], dt)
                else:
                    data[:K] = spec[b * kmax:b * kmax + K]
                base = slot + 2 * P * i
                region[base + P:base + 2 * P] = _transform(data, logP, False, dt, bad=(mut == "bad_twiddle"))
                region[base + P:base + 2 * P] *= region[base:base + P]
                v = _transform(region[base + P:base + 2 * P], logP, True, dt)[:nout]
                n = np.arange(nout)
                if stage == 1:
                    ys[b] = ((v * _chirp(n, M, 1.0, dt)).real / dt(N)).astype(dt)
                    continue
                t = v * _chirp(n, N, -1.0, dt)
                mn = min(N, M)
                t[0] = t[0].real
                if mn % 2 == 0 and mut != "no_nyquist":
                    t[mn // 2] *= dt(2.0 if M < N else (0.5 if M > N else 1.0))
                twice = n > 0
                if M % 2 == 0 and M // 2 < K:
                    twice[M // 2] = False
                    if mut != "keep_imag_m2":
                        t[M // 2] = t[M // 2].real
                if mut == "no_double" and twice.any():
                    twice[np.flatnonzero(twice)[twice.sum() // 2]] = False
                t[twice] *= dt(2.0)
                pitch = K if mut == "spec_pitch" else kmax
                spec[b * pitch:b * pitch + K] = t * _chirp(n, M, 1.0, dt)
    return ys


# ---------------------------------------------------------------------------------------------------- 5. data
def draw(kind, n, seed):
    rng = np.random.default_rng([seed, n, ("normal", "offset", "nyquist").index(kind)])
    g = rng.standard_normal(n)
    if kind == "offset":
        g = 1.0 + 0.1 * g
    elif kind == "nyquist":
        g = (-1.0) ** np.arange(n) + 1e-3 * g
    return g.astype(np.float32)


def fir_coefs(kind, K, seed):
    """the taps of one utterance; "sparse" (rows with K >= 4095): N(0, 1) on the first and the last four taps and on eight
    others, zero elsewhere"""
    if kind != "sparse":
        return draw(kind, K, seed)
    rng = np.random.default_rng([seed, K, 3])
    idx = np.unique(np.concatenate([np.arange(4), np.arange(K - 4, K), rng.integers(0, K, 8)]))
    f = np.zeros(K, np.float32)
    f[idx] = rng.standard_normal(len(idx)).astype(np.float32)
    return f


def fir_kinds(r):
    return KINDS + (("sparse",) if r["K"] >= 4095 else ())


def rs_kind_of(kind, N, M):
    """the data set of one utterance under the row's kind: the tone needs N even and survives only when M >= N"""
    return kind if kind != "nyquist" or (N % 2 == 0 and M >= N and N > 0) else "normal"


def rs_draw(r, kind):
    return [draw(rs_kind_of(kind, N, M), N, 1000 + b) for b, (N, M) in enumerate(r["utts"])]


def rs_kinds(r):
    """the data sets a row runs on: one for rows with logP >= 19, and the tone only where an utterance takes it"""
    if r["one_set"]:
        return ("normal",)
    tone = any(rs_kind_of("nyquist", N, M) == "nyquist" for N, M in r["utts"])
    return RS_KINDS if tone else KINDS


# ---------------------------------------------------------------------------------------------------- PATHS
def _rs(name, utts, why, expect, muts=()):
    """expect: the transform sizes of stage 0 and of stage 1, as the row claims them"""
    lps = [rs_logp(N, M) for N, M in utts if N and M]
    return dict(name=name, utts=list(utts), why=why, expect=expect, muts=tuple(muts),
                one_set=any(max(lp) >= 19 for lp in lps))


# the smallest N = M at which both stages have the size logP = 0, 2, 3, .. 22
_SMALLEST = (1, 2, 4, 6, 12, 22, 44, 86, 172, 342, 684, 1366, 2732, 5462, 10924, 21846, 43692, 87382, 174764, 349526, 699052,
             1398102)
_SHORT, _B600 = (12, 10), (9, 7)
RESAMPLE = (
    [_rs("eq_%d" % n, [(n, n)], "N = M: the smallest length with logP = %d in both stages" % lp, ([lp], [lp]),
         muts=("no_double", "drop_last_tap") if 4 <= n <= 2732 else (("bad_twiddle", "no_double") if n in (10924, 21846) else ()))
     for n, lp in zip(_SMALLEST, (0,) + tuple(range(2, 23)))]
    + [_rs("s0_logp1", [(2, 1)], "stage 0 at logP = 1 (needs N > M)", ([1], [0])),
       _rs("s1_logp1", [(1, 2)], "stage 1 at logP = 1 (needs M > N)", ([0], [1])),
       _rs("lds_down_ee", [(12, 10)], "LDS, M < N, min even, M even", ([5], [4]), muts=("no_nyquist", "keep_imag_m2", "drop_last_tap")),
       _rs("lds_down_oo", [(13, 9)], "LDS, M < N, min odd, M odd", ([5], [4])),
       _rs("lds_up_eo", [(10, 13)], "LDS, M > N, min even, M odd", ([4], [5]), muts=("no_nyquist", "no_double")),
       _rs("lds_up_oe", [(9, 12)], "LDS, M > N, min odd, M even", ([4], [4])),
       _rs("lds_eq_odd", [(11, 11)], "LDS, M = N odd", ([4], [4])),
       _rs("lds_eq_even_m2", [(700, 700)], "LDS, M = N even: bin M/2 is the input's Nyquist bin", ([11], [11]), muts=("keep_imag_m2",)),
       _rs("four_down_ee", [(30000, 27272)], "four-step, M < N, min even, M even", ([16], [16]), muts=("no_nyquist", "keep_imag_m2", "bad_twiddle")),
       _rs("four_down_oo", [(20001, 18181)], "four-step (7 + 8), M < N, min odd, M odd", ([15], [15])),
       _rs("four_up_eo", [(27272, 30001)], "four-step, M > N, min even, M odd", ([16], [16]), muts=("no_nyquist",)),
       _rs("four_up_oe", [(18181, 20000)], "four-step (7 + 8), M > N, min odd, M even", ([15], [15])),
       _rs("four_eq_odd", [(30001, 30001)], "four-step, M = N odd", ([16], [16]), muts=("bad_twiddle",)),
       _rs("four20_down", [(500000, 460001)], "logP = 20 in both stages with M < N, M odd", ([20], [20])),
       _rs("four19_up", [(240000, 262144)], "logP = 19 in both stages with M > N, min even", ([19], [19])),
       _rs("m0", [(5, 0)], "M = 0: nothing to do", ([], [])),
       _rs("n0_m0", [(0, 0)], "N = M = 0", ([], [])),
       _rs("b600", [_B600] * 600, "600 utterances of one size: groups of 256, 256 and 88", ([4], [4]), muts=("slot_255",)),
       _rs("boundary", [(44, 44)] * 2 + [_B600] * 256 + [(44, 44), (0, 0), (5, 0)],
           "the size changes exactly where the first group is full; the larger size comes first in the batch", ([4, 7], [4, 7]),
           muts=("slot_255", "spec_pitch")),
       _rs("long_among_short", [_SHORT] * 9 + [(21847, 20000)] + [_SHORT] * 11,
           "one long utterance among short ones: spec's B x kmax pitch and the larger-stage region", ([5, 15], [4, 15]), muts=("spec_pitch",))])


def _fir(name, K, ns, why):
    return dict(name=name, K=K, ns=list(ns), why=why)


_FIR_NS = (1, 7, 8, 9, 2047, 2048, 2049)
FIR = ([_fir("k%d" % K, K, _FIR_NS, "K = %d: main loop %d, tail %d; n on both sides of 8 and of a tile" % (K, K // 4, K % 4))
        for K in (1, 2, 3, 4, 5, 7, 8, 9)]
       + [_fir("k4095", 4095, (1, 9, 2049, 4099), "K = 4095: tail 3 under the largest halo"),
          _fir("k4096", 4096, (1, 8, 2047, 4099), "K = 4096: the largest halo, no tail"),
          _fir("long_k1", 1, (131072, 131073, 270000), "the stride loop: 1, 2 and 3 trips, bit-exact"),
          _fir("long_k5", 5, (131072, 131073, 270000), "the stride loop: 1, 2 and 3 trips"),
          _fir("long_k4096", 4096, (131073, 135000), "the second trip under the largest halo: one output, and most of two tiles")])


def fir_starts(ns, r0=0):
    """start offsets with residues r0, r0 + 1, .. modulo 4 and a gap of 4 .. 7 words between utterances"""
    starts, pos = [], 0
    for i, n in enumerate(ns):
        pos += (r0 + i - pos) % 4 + (4 if i else 0)
        starts.append(pos)
        pos += n
    return starts, pos + 3


def _mix(name, n, ms, why, res=(0, 0)):
    return dict(name=name, n=n, ms=[m for m in ms if m >= 1], why=why, res=res)


def _mix_ms(n):
    return sorted({1, 2, 3, 4, 5, 7, 8, n - 1, n, n + 1, 60001})


MIX_NS = (1, 3, 4, 5, 16384, 16385, 32768, 32769, 65536, 65537, 73728, 73729)
MIX = ([_mix("n%d" % n, n, _mix_ms(n), "%s%s" % (mix_form(n), ", %d tiles" % mix_tiles(n) if mix_tiles(n) else ""),
             res=(i % 4, (i // 2) % 4)) for i, n in enumerate(MIX_NS)]
       + [_mix("n2p21", 1 << 21, (60001, 7), "the longest utterance: all 256 tile partials")])


def _tile(name, items, why):
    return dict(name=name, items=list(items), why=why)


# items: (n, repeats)
TILE = [_tile("small", [(1, 1), (1, 9), (3, 1), (3, 5), (4, 1), (4, 3), (5, 2), (5, 1), (4099, 1), (4099, 3), (0, 4), (7, 0)],
              "n on both sides of 4; outputs on both sides of one strip; an empty signal and a zero repeat count"),
        _tile("above_cap", [(4099, 1100), (5, 3)], "4099 x 1100 = 4 508 900 > 1024 x 4096 samples: the fifth trip"),
        _tile("on_cap", [(4, 1048576), (3, 2)], "exactly 1024 x 4096 samples: four full trips")]

PATHS = dict(resample=RESAMPLE, fir=FIR, mix=MIX, tile=TILE)


def mix_one_set(r):
    return r["n"] >= 1 << 21


def tile_one_set(r):
    return max(n * k for n, k in r["items"]) > 4000000
