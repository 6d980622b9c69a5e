"""
The kernels that change the weights on every training step, restated for their path tests: the second half of csrc/nnops.hip
(lidbox_adam_step / _apply / _prepare_job, lidbox_sgd_step, lidbox_rmsprop_step, lidbox_spatial_dropout,
lidbox_input_noise_dropout, lidbox_dropout_rows, lidbox_cavg_result, lidbox_mean / _scale / _fill) and csrc/mla.hip
(lidbox_mla_attention_fwd / _bwd, lidbox_bn_relu_dropout_fwd / _bwd).  tests/test_oracle_update_paths.py pins all of it on the
CPU, tests/test_update_paths_gpu.py runs every row through the C ABI.  TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

1. DISPATCH.  Every function quotes the source condition it restates: ew_grid / ew_trips, adam_plan (float4 body, scalar
   tail), spatial_plan (also the noise kernel's), rows_plan, bnrd_plan (vector or scalar, per pointer), mla_plan / mla_fwd_plan
   / mla_bwd_plan, cavg_lds_pf.  Note on Adam's tail: it has at most three elements, taken by threads 0 .. 2 of block 0 after
   their body trips, so "the second trip of body and tail" is a thread that has made two body trips and then takes a tail
   element; adam_plan states what the code does.

2. THE COUNTER HASH.  hash_uniform(seed, step, b, c): the splitmix64 finaliser over seed + 0x9E3779B97F4A7C15 (step + 1) +
   (b << 32 | c) in uint64 arithmetic, top 24 bits times 2^-24 (exact in float32).  keep(u, rate) is `u >= rate` in float32;
   keep_scale(rate) is fl(1 / fl(1 - rate)) -- HIP's float division is correctly rounded, so the device value is this one and
   kept elements are fl(x keep_scale) bit for bit.  Masks are therefore predicted exactly; no element is excused.
   Rate 0: the three dropout calls return before any launch (`rate == 0.f` in the early-return line), so x AND a given
   mask_out are left as they were (the header now says so).

3. REFERENCES (float64) with their BOUNDS.  u = 2^-24.  g(k) = k u / (1 - k u) bounds k roundings of one term.
   Optimiser steps, one step from a float32 state, every `a * b + c` fused or not (the fused form has fewer roundings, so the
   unfused count bounds both), sums in absolute-value form:
     gr = g gs                                                   1 rounding
     Adam     m' = b1 m + (1 - b1) gr                            g(2) |b1 m| + g(4) |(1 - b1) gr|   (1 - b1 rounds too)
              v' = b2 v + (1 - b2) gr gr                         g(2) |b2 v| + g(6) (1 - b2) gr^2
              p' = p - lr_t m' / (sqrt(v') + eps)                D = sqrt(v') + eps lies within dD = sqrt(v' + bv) - sqrt(v' - bv)
                                                                 + u sqrt(v') + u D; q = lr_t m' / D within |q| (g(2) + dD / (D - dD))
                                                                 + lr_t bm / (D - dD); p' within that + u (|p| + |q|)
     SGD      p' = p - lr gr                                     g(2) |lr gr| + u (|p| + |lr gr|)
              v' = mu v - lr gr                                  g(2) |mu v| + g(3) |lr gr|
              p' = p + v'                                        bv + u (|p| + |v'|)
              p' = p + (mu v' - lr gr)    (nesterov)             mu bv + g(2) |mu v'| + g(3) |lr gr| + u (|p| + |mu v'| + |lr gr|)
     RMSprop  r' as Adam's v', a' (mean_grad) as Adam's m'; centred denom = r' - a'^2 within br + 2 |a'| ba + ba^2 + g(2) a'^2
              + u r'; with mom: t = lr gr / sqrt(denom + eps), the root within sqrt(s + bs) - sqrt(s - bs) + u sqrt(s), bs = bden +
              u s; mom' = mu mom + t within g(2) |mu mom| + |t| (g(3) + droot / (root - droot)) + u |t|; p' = p - mom' within
              that + u (|p| + |mom'|).  Without: p' = p - lr gr / (sqrt(denom) + eps), D as for Adam with g(3) for gr, product, division.
   lr_t is computed in double and rounded to float as the kernel does; the device value may differ by one float32 ulp (device pow
   against host pow); the reference step takes the PUBLISHED lr_t as its input, which is lidbox_adam_apply's contract.
   Box-Muller.  u1 = 1 - h1 in (0, 1] and u2 = h2 are exact.  n = R cos(TWO_PI32 u2), R = sqrt(-2 ln u1), TWO_PI32 the kernel's
   float32 constant (it defines the draw).  The product TWO_PI32 u2 < 8 rounds by at most 2^-22 < pi 2^-23, which moves
   R cos by at most pi 2^-23 R; logf, sqrtf, cosf and the two products R cos and stddev n are given 4 2^-23 max(1, R) together
   (eight half-ulps of a value of at most max(1, R)): (pi + 4) 2^-23 max(1, R) stddev, plus the two roundings of (x + stddev n) m.
   A float32 NumPy evaluation stays under half of it (tests/test_oracle_update_paths.py).
   Attention forward, relative (every term of sum c v / sum c is positive).  Per element: the exponent's argument z - max rounds
   by u |z - max|, expf is given 2 ulp, the row sum is a chain of VEC NJ adds and log2 G shuffles over terms with their own
   errors (weighted by p), the division rounds once: e_c[t, k].  v = sigmoid: 5 roundings, c v: one more.  The column sums run
   ceil(T / (nw 64 / G)) adds in a lane, log2(64 / G) shuffles, nw waves: chain L.  att[k] within (sum_t c v (e_c + 6 u) /
   sum_t c v + sum_t c e_c / sum_t c + 2 g(L) + u) att[k]; colsum[k] within (sum_t c e_c / sum_t c + g(L)) colsum[k].
   Attention backward, absolute, att and colsum being inputs: mla_bwd_ref returns the bound built on the absolute-value versions
   of dot = sum_j dp_j p_j and of p (dp - dot) + tail, as nnops_np.stats_pool_bwd_abs does for the pool.
   cavg_result: all terms are non-negative.  pm: one addition and one division per language, N additions, / N, two coefficient
   roundings and a product: g(N + 7).  pf: the inner sum over N languages (addition, division, N additions, / (N - 1)), then N
   additions, / N, the coefficient C_fa (1 - P_tar) and a product: g(2 N + 9) -- the N^2 divisions sit in N chains of length N,
   so the chain is 2 N long, not N^2.  c[th] within g(N + 7) pm-term + g(2 N + 9) pf-term + u c; out[0] within the largest of them.

4. MISTAKES.  Every reference takes mistake=...; MISTAKES maps each to the rows on which the CPU test shows the bound rejecting
   it.  UNDETECTABLE is empty: every planted mistake changes an output value on some row.

5. PATHS: ADAM, SGD, RMSPROP, SPATIAL, NOISE, ROWS, BNRD, MLA, CAVG, EW.  Each row carries the condition it exists for.
"""
import math
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lidbox_amd", "csrc")

U = 2.0 ** -24
EW_THREADS, EW_MAX_BLOCKS = 256, 2048
DROP_MAX_GX, ROWS_MAX_BLOCKS, BNRD_MAX_BLOCKS, DROP_MAX_B = 64, 4096, 8192, 65535
MLA_MAX_K, MLA_BWD_NW, MLA_BWD_WANT = 1024, 8, 2048
CAVG_THREADS, CAVG_LDS_TH, CAVG_LDS_BYTES = 1024, 512, 48 * 1024
LO = float(np.float32(1e-7))
HI = float(np.float32(1 - 1e-7))
GOLD, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
NOISE_SEED1, NOISE_SEED2 = 0x632BE59BD9B4E019, 0x8CB92BA72F3D8DD7
TWO_PI32 = float(np.float32(6.283185307179586))


def cdiv(a, b):
    return -(-a // b)


def g(k):
    return k * U / (1.0 - k * U)


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- 1. dispatch
def ew_grid(n):
    """`long g = lbx_cdiv(n, 256); return g < 1 ? 1 : (g > 2048 ? 2048 : g)`"""
    return min(max(cdiv(n, EW_THREADS), 1), EW_MAX_BLOCKS)


def ew_trips(n):
    """trips of thread 0 through `for (i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)`"""
    return cdiv(n, ew_grid(n) * EW_THREADS)


def adam_plan(n):
    """`n4 = n >> 2`, grid `ew_grid(n / 4 + 1)`; the tail starts at `(n4 << 2) + thread`"""
    n4 = n >> 2
    grid = ew_grid(n // 4 + 1)
    return dict(n4=n4, tail=n - 4 * n4, grid=grid, body_trips=cdiv(n4, grid * EW_THREADS), launch=n > 0)


def spatial_plan(B, T, C, rate, stddev=0.0):
    """`if (B == 0 || T == 0 || rate == 0.f) return` (noise: `rate == 0.f && stddev == 0.f`); `gx = lbx_cdiv(T * C, 256); if (gx >
    64) gx = 64`; grid (gx, B)"""
    if B == 0 or T == 0 or (rate == 0.0 and stddev == 0.0):
        return dict(launch=False, gx=0, trips=0, mask_blocks=0)
    gx = min(cdiv(T * C, 256), DROP_MAX_GX)
    return dict(launch=True, gx=gx, trips=cdiv(T * C, gx * 256),
                mask_blocks=min(cdiv(C, 256), gx),                       # blocks whose first trip holds an i < C
                mask_trips=cdiv(min(C, T * C), gx * 256))                 # trips on which some i < C is met


def spatial_accepts(B, T, C, bs, noise=False):
    """`B >= 0 && T >= 0 && C >= 1`, `batch_stride >= T * C` (noise: `&& T * C < 2^32`), `B <= 65535`"""
    return B >= 0 and T >= 0 and C >= 1 and bs >= T * C and B <= DROP_MAX_B and (not noise or T * C < 1 << 32)


def rows_plan(R, C, rate):
    """`if (R == 0 || rate == 0.f) return; g = lbx_cdiv(R * C, 256); if (g > 4096) g = 4096`"""
    if R == 0 or rate == 0.0:
        return dict(launch=False, grid=0, trips=0)
    grid = min(cdiv(R * C, 256), ROWS_MAX_BLOCKS)
    return dict(launch=True, grid=grid, trips=cdiv(R * C, grid * 256))


def bnrd_plan(R, C, addrs, bwd):
    """`vec4 = C % 4 == 0 && aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(out) && (!BWD || aligned16(dy))`;
    `n = R * C / (vec4 ? 4 : 1); g = lbx_cdiv(n, 256); if (g > 8192) g = 8192`.  addrs: dict x, scale, shift, out[, dy]"""
    names = ("x", "scale", "shift", "out") + (("dy",) if bwd else ())
    vec4 = C % 4 == 0 and all(addrs[k] % 16 == 0 for k in names)
    n = R * C // (4 if vec4 else 1)
    grid = min(cdiv(n, 256), BNRD_MAX_BLOCKS)
    return dict(vec=4 if vec4 else 1, n=n, grid=grid, trips=cdiv(n, grid * 256) if grid else 0,
                kernel="bn_relu_dropout_kernel<%d,%s>" % (4 if vec4 else 1, "BWD" if bwd else "FWD"))


def mla_plan(K, vec4):
    """mla_plan() of mla.hip; vec4 = `K % 4 == 0 && aligned16(z)` (backward: `&& aligned16(dz)`)"""
    vec = 4 if vec4 else 1
    kv = (K + vec - 1) // vec
    G = 1
    while G < 64 and G < kv:
        G <<= 1
    need = (kv + G - 1) // G
    nj = 1
    while nj < need:
        nj <<= 1
    return dict(vec=vec, G=G, nj=nj, nw=16 if K <= 512 else 8)


def mla_vec4(K, z_addr, dz_addr=0):
    return K % 4 == 0 and z_addr % 16 == 0 and dz_addr % 16 == 0


def mla_fwd_plan(T, K, vec4):
    """block `p.nw * 64`, dynamic LDS `p.nw * 2 * K * sizeof(float)`; a pass of the row loop covers nw * 64 / G rows"""
    p = mla_plan(K, vec4)
    rows = p["nw"] * (64 // p["G"])
    p.update(lds=p["nw"] * 2 * K * 4, pass_rows=rows, passes=cdiv(T, rows),
             chain=cdiv(T, rows) + int(math.log2(64 // p["G"])) + p["nw"],
             kernel="mla_attention_fwd_kernel<%d,%d>" % (p["vec"], p["nj"]))
    return p


def mla_bwd_plan(B, T, K, vec4):
    """`rows_per_wg = nw * (64 / p.G)` with nw = 8; `gy = lbx_cdiv(T, rows_per_wg); want = lbx_cdiv(2048, B); if (gy > want) gy = want`"""
    p = mla_plan(K, vec4)
    rpw = MLA_BWD_NW * (64 // p["G"])
    gy = min(cdiv(T, rpw), cdiv(MLA_BWD_WANT, B))
    p.update(rows_per_wg=rpw, gy=gy, trips=cdiv(T, gy * rpw), kernel="mla_attention_bwd_kernel<%d,%d>" % (p["vec"], p["nj"]))
    return p


def cavg_lds_pf(N, Th):
    """`lds = N * Th * sizeof(float); lds_pf = Th <= 512 && lds <= 48 * 1024`"""
    return Th <= CAVG_LDS_TH and N * Th * 4 <= CAVG_LDS_BYTES


def cavg_trips(Th):
    """`for (th = threadIdx.x; th < Th; th += 1024)`"""
    return cdiv(Th, CAVG_THREADS)


def launch_site_kernels():
    """the (VEC, NJ) pairs of the MLA_FWD / MLA_BWD launch sites and the instantiations of bn_relu_dropout_kernel, from the text"""
    with open(os.path.join(CSRC, "mla.hip")) as f:
        src = f.read()
    out = set()
    for d in ("FWD", "BWD"):
        for v, n in re.findall(r"MLA_%s\((\d+), (\d+)\);" % d, src):
            out.add("mla_attention_%s_kernel<%s,%s>" % (d.lower(), v, n))
    for v in re.findall(r"\(bn_relu_dropout_kernel<(\d), BWD>\)", src):
        out |= {"bn_relu_dropout_kernel<%s,FWD>" % v, "bn_relu_dropout_kernel<%s,BWD>" % v}
    return out


# ---------------------------------------------------------------------------------------------------- 2. the counter hash
HASH_MISTAKES = ("swap_bc", "step_not_plus1", "noise_key_c", "mask_key_i", "c_first_trip")


def hash_uniform(seed, step, b, c, mistake=None):
    """float32 uniforms in [0, 1); b, c broadcast (taken modulo 2^32 as the kernel's `(unsigned)` casts do)"""
    b = np.asarray(b, np.uint64) & np.uint64(0xFFFFFFFF)
    c = np.asarray(c, np.uint64) & np.uint64(0xFFFFFFFF)
    if mistake == "swap_bc":
        b, c = c, b
    k = (int(step) + (0 if mistake == "step_not_plus1" else 1)) & 0xFFFFFFFFFFFFFFFF
    base = np.uint64((int(seed) + GOLD * k) & 0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        v = base + ((b << np.uint64(32)) | c)
        v ^= v >> np.uint64(30)
        v *= np.uint64(MIX1)
        v ^= v >> np.uint64(27)
        v *= np.uint64(MIX2)
        v ^= v >> np.uint64(31)
    return (v >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep(u, rate):
    return np.asarray(u, np.float32) >= np.float32(rate)


def keep_scale(rate):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def spatial_mask(B, T, C, rate, seed, step, mistake=None):
    """the factor of every element, [B, T, C] float32 (keep_scale or 0); the kernel's is a function of (b, c) alone"""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    i = np.arange(T * C, dtype=np.uint64).reshape(1, T, C)
    c = i % np.uint64(C)
    if mistake == "mask_key_i":
        c = i
    elif mistake == "c_first_trip":
        p = spatial_plan(B, T, C, rate)
        c = (i % np.uint64(p["gx"] * 256)) % np.uint64(C)
    u = hash_uniform(seed, step, b, c, mistake if mistake in ("swap_bc", "step_not_plus1") else None)
    return np.where(keep(u, rate), keep_scale(rate), np.float32(0)).astype(np.float32) * np.ones((B, T, C), np.float32)


def spatial_ref(x, rate, seed, step, mistake=None):
    """(y, mask_out): y = fl(x m) in float32 -- exact, the sign of a zeroed negative included"""
    x = np.asarray(x, np.float32)
    B, T, C = x.shape
    m = spatial_mask(B, T, C, rate, seed, step, mistake)
    return x * m, (m[:, 0, :].copy() if T else np.zeros((B, C), np.float32))


def rows_mask(R, C, rate, seed, step, mistake=None):
    r = np.arange(R, dtype=np.uint64)[:, None]
    c = np.arange(C, dtype=np.uint64)[None, :]
    u = hash_uniform(seed, step, r, c, mistake)
    return np.where(keep(u, rate), keep_scale(rate), np.float32(0)).astype(np.float32)


def box_muller(B, T, C, seed, step, mistake=None):
    """(n float64 [B, T, C], R float64): the draw of element (b, i = t C + c)"""
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    i = np.arange(T * C, dtype=np.uint64).reshape(1, T, C)
    key = i % np.uint64(C) if mistake == "noise_key_c" else i
    hm = mistake if mistake in ("swap_bc", "step_not_plus1") else None
    u1 = np.float32(1.0) - hash_uniform((int(seed) + NOISE_SEED1) & 0xFFFFFFFFFFFFFFFF, step, b, key, hm)
    u2 = hash_uniform((int(seed) + NOISE_SEED2) & 0xFFFFFFFFFFFFFFFF, step, b, key, hm)
    R = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return R * np.cos(TWO_PI32 * u2.astype(np.float64)) * np.ones((B, 1, 1)), R * np.ones((B, 1, 1)), (u1, u2)


def box_muller32(u1, u2):
    """the kernel's expression in float32 NumPy"""
    u1, u2 = np.asarray(u1, np.float32), np.asarray(u2, np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(TWO_PI32) * u2)


def box_muller_bound(R, stddev):
    return (math.pi + 4.0) * 2.0 ** -23 * np.maximum(1.0, R) * stddev


def noise_ref(x, stddev, rate, seed, step, mistake=None):
    """(y float64, bound): y = (x + stddev n) m"""
    x = np.asarray(x, np.float32)
    B, T, C = x.shape
    m = spatial_mask(B, T, C, rate, seed, step, mistake if mistake in ("swap_bc", "step_not_plus1", "mask_key_i") else None).astype(np.float64)
    n, R, _ = box_muller(B, T, C, seed, step, mistake)
    v = f64(x) + stddev * n
    mag = np.abs(f64(x)) + stddev * np.abs(n)
    return v * m, (box_muller_bound(R, stddev) + 2 * U * mag) * m * (1 + 4 * U)


# ---------------------------------------------------------------------------------------------------- 3. optimiser steps
def lr_t_ref(lr, lr_now, step_before, b1=None, b2=None, mistake=None):
    """(step after, lr_t float32).  lr_now: a float32 VALUE whose bit pattern decides (`__float_as_uint(st->lr_now) != 0u`);
    b1 = None: SGD / RMSprop's opt_prepare_kernel (no bias correction).  mistake: no_bias"""
    t = int(step_before) + 1
    now = np.float32(lr_now)
    base = float(np.abs(now)) if now.view(np.uint32) != 0 else float(np.float32(lr))
    if b1 is None:
        return t, np.float32(base)
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    c = math.sqrt(1.0 - math.pow(b2, float(t))) / (1.0 - math.pow(b1, float(t)))
    return t, np.float32(base * (1.0 if mistake == "no_bias" else c))


def _root_spread(s, bs):
    return np.sqrt(s + bs) - np.sqrt(np.maximum(s - bs, 0.0))


def adam_ref(p, gr_, m, v, lr_t, b1, b2, eps, gs, mistake=None):
    """one step from the float32 state; returns dict name -> (value float64, bound).  mistake: eps_inside, no_bias (the latter
    acts on lr_t: see lr_t_ref; here it is the caller's lr_t that carries it)"""
    p, gr_, m, v = f64(p), f64(gr_), f64(m), f64(v)
    b1, b2, eps, gs, lr_t = (float(np.float32(a)) for a in (b1, b2, eps, gs, lr_t))
    gr = gr_ * gs
    t1, t2 = np.abs(b1 * m), np.abs((1 - b1) * gr)
    m1, bm = b1 * m + (1 - b1) * gr, g(2) * t1 + g(4) * t2
    s1, s2 = np.abs(b2 * v), (1 - b2) * gr * gr
    v1, bv = b2 * v + s2, g(2) * s1 + g(6) * s2
    if mistake == "eps_inside":
        D = np.sqrt(v1 + eps)
    else:
        D = np.sqrt(v1) + eps
    dD = _root_spread(v1, bv) + U * np.sqrt(v1) + U * D
    q = lr_t * m1 / D
    bq = np.abs(q) * (g(2) + dD / (D - dD)) + lr_t * bm / (D - dD)
    return dict(param=(p - q, (bq + U * (np.abs(p) + np.abs(q))) * (1 + 8 * U)), m=(m1, bm), v=(v1, bv))


def sgd_ref(p, gr_, vel, lr, mu, nesterov, gs, mistake=None):
    """vel None: plain.  mistake: nesterov_sign"""
    p, gr_ = f64(p), f64(gr_)
    lr, mu, gs = (float(np.float32(a)) for a in (lr, mu, gs))
    gr = gr_ * gs
    step = np.abs(lr * gr)
    if vel is None:
        return dict(param=(p - lr * gr, g(2) * step + U * (np.abs(p) + step)))
    vel = f64(vel)
    v1, bv = mu * vel - lr * gr, g(2) * np.abs(mu * vel) + g(3) * step
    if not nesterov:
        return dict(param=(p + v1, (bv + U * (np.abs(p) + np.abs(v1))) * (1 + 8 * U)), velocity=(v1, bv))
    inner = (-mu * v1 if mistake == "nesterov_sign" else mu * v1) - lr * gr
    bp = mu * bv + g(2) * np.abs(mu * v1) + g(3) * step + U * (np.abs(p) + np.abs(mu * v1) + step)
    return dict(param=(p + inner, bp * (1 + 8 * U)), velocity=(v1, bv))


def rmsprop_ref(p, gr_, rms, mg, mom, lr, rho, mu, eps, gs, mistake=None):
    """mg / mom None or given (centred / momentum form).  mistake: eps_swapped (inside the root without momentum, outside with)"""
    p, gr_, rms = f64(p), f64(gr_), f64(rms)
    lr, rho, mu, eps, gs = (float(np.float32(a)) for a in (lr, rho, mu, eps, gs))
    gr = gr_ * gs
    s2 = (1 - rho) * gr * gr
    r1, br = rho * rms + s2, g(2) * np.abs(rho * rms) + g(6) * s2
    out = dict(rms=(r1, br))
    den, bden = r1, br
    if mg is not None:
        mg = f64(mg)
        a1, ba = rho * mg + (1 - rho) * gr, g(2) * np.abs(rho * mg) + g(4) * np.abs((1 - rho) * gr)
        out["mean_grad"] = (a1, ba)
        den = r1 - a1 * a1
        bden = br + 2 * np.abs(a1) * ba + ba * ba + g(2) * a1 * a1 + U * r1
    inside = (mom is not None) != (mistake == "eps_swapped")
    if inside:
        s = den + eps
        bs = bden + U * np.abs(s)
        D, dD = np.sqrt(s), _root_spread(s, bs) + U * np.sqrt(s)
    else:
        D = np.sqrt(den) + eps
        dD = _root_spread(den, bden) + U * np.sqrt(den) + U * D
    t = lr * gr / D
    bt = np.abs(t) * (g(3) + dD / (D - dD))
    if mom is not None:
        mom = f64(mom)
        m1 = mu * mom + t
        bm = (g(2) * np.abs(mu * mom) + bt + U * np.abs(t)) * (1 + 8 * U)
        out["mom"] = (m1, bm)
        out["param"] = (p - m1, (bm + U * (np.abs(p) + np.abs(m1))) * (1 + 8 * U))
    else:
        out["param"] = (p - t, (bt + U * (np.abs(p) + np.abs(t))) * (1 + 8 * U))
    return out


def _f32(a):
    return np.asarray(a, np.float32)


def adam_emu32(p, gr_, m, v, lr_t, b1, b2, eps, gs):
    """the kernel's expressions in float32 NumPy, unfused"""
    p, gr_, m, v = (_f32(a) for a in (p, gr_, m, v))
    b1, b2, eps, gs, lr_t, one = (np.float32(a) for a in (b1, b2, eps, gs, lr_t, 1.0))
    gr = gr_ * gs
    m1 = b1 * m + (one - b1) * gr
    v1 = b2 * v + (one - b2) * gr * gr
    return dict(param=p - lr_t * m1 / (np.sqrt(v1) + eps), m=m1, v=v1)


def sgd_emu32(p, gr_, vel, lr, mu, nesterov, gs):
    p, gr_ = _f32(p), _f32(gr_)
    lr, mu, gs = (np.float32(a) for a in (lr, mu, gs))
    gr = gr_ * gs
    if vel is None:
        return dict(param=p - lr * gr)
    v1 = mu * _f32(vel) - lr * gr
    return dict(param=p + ((mu * v1 - lr * gr) if nesterov else v1), velocity=v1)


def rmsprop_emu32(p, gr_, rms, mg, mom, lr, rho, mu, eps, gs):
    p, gr_, rms = _f32(p), _f32(gr_), _f32(rms)
    lr, rho, mu, eps, gs, one = (np.float32(a) for a in (lr, rho, mu, eps, gs, 1.0))
    gr = gr_ * gs
    r1 = rho * rms + (one - rho) * gr * gr
    out = dict(rms=r1)
    den = r1
    if mg is not None:
        a1 = rho * _f32(mg) + (one - rho) * gr
        out["mean_grad"] = a1
        den = r1 - a1 * a1
    if mom is not None:
        m1 = mu * _f32(mom) + lr * gr / np.sqrt(den + eps)
        out["mom"] = m1
        out["param"] = p - m1
    else:
        out["param"] = p - lr * gr / (np.sqrt(den) + eps)
    return out


# ---------------------------------------------------------------------------------------------------- 3. attention pool
ATT_MISTAKES = ("drop_row_slot", "no_clip", "drop_wave", "pass_clipped")


def near_clip_bound(pn):
    """the band of tests/test_mla_ops_gpu.py: no p within relative 1e-3 of lo, no 1 - p between (1 - hi) / 4 and 4 (1 - hi)"""
    return (np.abs(pn - LO) <= 1e-3 * LO) | ((1 - pn >= (1 - HI) / 4) & (1 - pn <= 4 * (1 - HI)))


def _softmax_parts(z, plan):
    z = f64(z)
    mx = z.max(-1, keepdims=True)
    e = np.exp(z - mx)
    p = e / e.sum(-1, keepdims=True)
    e_exp = U * (np.abs(z - mx) + 4.0)
    chain = plan["vec"] * plan["nj"] + int(math.log2(plan["G"]))
    e_c = e_exp + (p * e_exp).sum(-1, keepdims=True) + g(chain) + U
    return z, p, e_c


def _sigmoid_parts(z):
    u = np.exp(-np.abs(z))
    r = 1.0 / (1.0 + u)
    return np.where(z >= 0, r, u * r), u * r * r


def mla_fwd_ref(z, plan, mistake=None):
    """z [B, T, K] -> att, colsum [B, K] float64, their relative bounds, and the share of clipped elements; asserts that no
    probability lies near a clip bound.  plan: mla_fwd_plan(T, K, vec4) (the summation order the bound counts)"""
    z, p, e_c = _softmax_parts(z, plan)
    B, T, K = z.shape
    assert not near_clip_bound(p).any(), "%d probabilities near a clip bound" % int(near_clip_bound(p).sum())
    c = p if mistake == "no_clip" else np.clip(p, LO, HI)
    v, _ = _sigmoid_parts(z)
    live = np.ones(T, bool)
    if mistake == "drop_row_slot":
        live[T - 1] = False
    elif mistake == "drop_wave":
        rpw = 64 // plan["G"]
        live[(np.arange(T) % plan["pass_rows"]) // rpw == plan["nw"] - 1] = False
    lv = live[None, :, None]
    s, sv = (c * lv).sum(1), (c * v * lv).sum(1)
    att = sv / s
    e_den = (c * e_c).sum(1) / c.sum(1)
    e_num = (c * v * (e_c + 6 * U)).sum(1) / (c * v).sum(1)
    L = plan["chain"]
    return dict(att=att, colsum=s, att_rel=e_num + e_den + 2 * g(L) + U, colsum_rel=e_den + g(L),
                clipped=float(((p < LO) | (p > HI)).mean()))


def mla_bwd_ref(z, att, colsum, datt, plan, mistake=None):
    """dz float64 and its absolute bound; att, colsum, datt are the float32 arrays the kernel reads"""
    z, p, e_c = _softmax_parts(z, plan)
    att, colsum, datt = f64(att)[:, None, :], f64(colsum)[:, None, :], f64(datt)[:, None, :]
    v, dv = _sigmoid_parts(z)
    c = np.clip(p, LO, HI)
    ok = np.ones_like(p, bool) if mistake == "pass_clipped" else (p >= LO) & (p <= HI)
    gs = datt / colsum
    dp = np.where(ok, gs * (v - att), 0.0)
    tail = gs * c * dv
    dot = (dp * p).sum(-1, keepdims=True)
    dz = p * (dp - dot) + tail
    # bounds
    b_dp = np.where(ok, np.abs(gs) * (5 * U * v + U * np.abs(v - att)) + 2 * U * np.abs(dp), 0.0)
    chain = plan["vec"] * plan["nj"] + int(math.log2(plan["G"]))
    adot = (np.abs(dp) * p).sum(-1, keepdims=True)
    b_dot = (b_dp * p + np.abs(dp) * p * (e_c + U)).sum(-1, keepdims=True) + g(chain) * adot
    inner = np.abs(dp) + adot
    b = p * e_c * inner + p * (b_dp + b_dot + U * inner) + U * p * inner + np.abs(tail) * (e_c + 12 * U)
    b += U * (p * inner + np.abs(tail))
    return dz, b * (1 + 8 * U)


# ---------------------------------------------------------------------------------------------------- 3. bn -> relu -> mask
def bnrd_ref(x, scale, shift, rate, seed, step, dy=None):
    """(y float64, dx float32 or None): y = relu(x scale + shift) m; dx = (x scale + shift > 0) ? fl(dy m) : 0 is exact"""
    x = np.asarray(x, np.float32)
    R, C = x.shape
    v = f64(x) * f64(scale)[None, :] + f64(shift)[None, :]
    m = rows_mask(R, C, rate, seed, step) if rate > 0 else np.ones((R, C), np.float32)
    y = np.maximum(v, 0.0) * m.astype(np.float64)
    dx = None
    if dy is not None:
        dx = np.where(v > 0, (np.asarray(dy, np.float32) * m) if rate > 0 else np.asarray(dy, np.float32), np.float32(0)).astype(np.float32)
    return y, dx


def bnrd_exact32(x, scale, shift, rate, seed, step):
    """y predicted bit for bit on the host: fmaf is ONE rounding (conv2d_np.fma32), the ReLU, one float32 product with the mask"""
    from oracle.conv2d_np import fma32
    x = np.asarray(x, np.float32)
    R, C = x.shape
    v = fma32(x, np.asarray(scale, np.float32)[None, :], np.asarray(shift, np.float32)[None, :])
    y = np.where(v > 0, v, np.float32(0)).astype(np.float32)
    return y * rows_mask(R, C, rate, seed, step) if rate > 0 else y


def ulp_distance(a, ref64):
    """|a - ref| in ulps, one ulp taken as 2^-23 |ref|: y = fl(fl(x scale + shift) keep_scale) carries two roundings of at most
    2^-24 relative each (the fused multiply-add and the product), and 2^-23 |ref| is the float32 spacing at the bottom of ref's
    binade.  In units of the spacing AT ref (spacing_distance) the same error can reach 2 just below a power of two, which is
    why that figure is recorded by the GPU test and not asserted.  0 where both are 0"""
    a, ref64 = np.asarray(a, np.float64), np.asarray(ref64, np.float64)
    d = np.abs(a - ref64)
    return np.where(d == 0, 0.0, d / np.maximum(2.0 ** -23 * (1 + 2.0 ** -23) * np.abs(ref64), 2.0 ** -149))


def spacing_distance(a, ref64):
    """|a - ref| in units of the float32 spacing at ref"""
    a, ref64 = np.asarray(a, np.float64), np.asarray(ref64, np.float64)
    return np.abs(a - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- 3. cavg_result
def _dnn(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def cavg_ref(tp, fn, fp, tn, C_miss, C_fa, P_tar, mistake=None):
    """tp, fn [N, Th]; fp, tn [N, N, Th] -> (c [Th] float64, bound [Th], min, its bound).  mistake: div_n, min_first_1024"""
    tp, fn, fp, tn = f64(tp), f64(fn), f64(fp), f64(tn)
    N, Th = tp.shape
    cm, cf, pt = (float(np.float32(a)) for a in (C_miss, C_fa, P_tar))
    pm = _dnn(fn, fn + tp).sum(0) / N
    inner = _dnn(fp, fp + tn).sum(1) / (N if mistake == "div_n" else N - 1)
    pf = inner.sum(0) / N
    a, b = cm * pt * pm, cf * (1 - pt) * pf
    c = a + b
    bound = g(N + 7) * a + g(2 * N + 9) * b + U * c
    cmin = c[:1024].min() if mistake == "min_first_1024" else c.min()
    return c, bound, cmin, bound.max()


def mean_ref(x):
    """(mean float64, bound): 256 lanes of ceil(n / 256) adds, 6 shuffles, 3 adds, one division, on absolute values"""
    x = f64(x)
    n = len(x)
    return x.mean(), g(cdiv(n, 256) + 6 + 3 + 1) * np.abs(x).mean()


# ---------------------------------------------------------------------------------------------------- 4. mistakes
MISTAKES = {
    "adam:eps_inside": ("adam", ("n1027", "zeroed", "n7")), "adam:no_bias": ("adam", ("n1027", "step1")),
    "rmsprop:eps_swapped": ("rmsprop", ("plain_n257", "momentum_n257", "centered_momentum_n257")),
    "sgd:nesterov_sign": ("sgd", ("nesterov_n257",)),
    "hash:swap_bc": ("spatial", ("b3t7c5", "b2t3c300")), "hash:step_not_plus1": ("spatial", ("b3t7c5",)),
    "hash:noise_key_c": ("noise", ("b3t7c5",)), "hash:mask_key_i": ("spatial", ("b3t7c5", "b2t65c253")),
    "spatial:c_first_trip": ("spatial", ("b2t65c253", "b2t2c16400")),
    "att:drop_row_slot": ("mla", ("k100", "k4_t1025")), "att:no_clip": ("mla", ("k100", "k512")),
    "att:drop_wave": ("mla", ("k100", "k64_trip2")), "att:pass_clipped": ("mla", ("k100", "k1023")),
    "cavg:div_n": ("cavg", ("n3th5", "n24th512")), "cavg:min_first_1024": ("cavg", ("n3th1025", "n2th2049")),
}
UNDETECTABLE = ()


# ---------------------------------------------------------------------------------------------------- 5. PATHS
def _row(name, why, **kw):
    return dict(name=name, why=why, **kw)


_ADAM_BIG = 2097152 + 1027
ADAM = ([_row("n%d" % n, "n = %d: %d float4 of body, tail %d" % (n, n >> 2, n & 3), n=n) for n in (0, 1, 3, 4, 5, 7, 1023, 1024, 1027)]
        + [_row("big", "n = 2 097 152 + 1027: threads 0 .. 255 make a second body trip, threads 0 .. 2 then take the tail", n=_ADAM_BIG),
           _row("gs05", "grad_scale 0.5", n=1027, gs=0.5),
           _row("zeroed", "zeroed m, v and state", n=1027, zero=True),
           _row("lr_now", "lr_now = 5e-4 replaces lr", n=1027, lr_now=5e-4),
           _row("neg_zero", "lr_now = -0.0f: a scheduled rate of exactly 0; param keeps its bits, m and v move, the step advances", n=1027,
                lr_now=-0.0),
           _row("neg_zero_n0", "n = 0 with lr_now = -0.0f", n=0, lr_now=-0.0)]
        + [_row("step%d" % s, "step preset to %d%s" % (s, ": the bias correction saturates" if s >= 10000 else ""), n=1027, step=s)
           for s in (0, 1, 10000, 1 << 33)])
for _r in ADAM:
    for _k, _v in (("gs", 1.0), ("zero", False), ("lr_now", 0.0), ("step", 3)):
        _r.setdefault(_k, _v)

OPT_NS = (0, 1, 255, 256, 257, 524288 + 300)
SGD_VARIANTS = dict(plain=dict(mu=0.0, nesterov=0), momentum=dict(mu=0.9, nesterov=0), nesterov=dict(mu=0.9, nesterov=1))
RMS_VARIANTS = dict(plain=dict(mu=0.0, centered=0), centered=dict(mu=0.0, centered=1), momentum=dict(mu=0.9, centered=0),
                    centered_momentum=dict(mu=0.9, centered=1))
SGD = [_row("%s_n%d" % (k, n), "%s, n = %d: %d trip(s)" % (k, n, ew_trips(n)), n=n, variant=k, gs=0.5 if n == 257 else 1.0,
            lr_now=(-0.0 if n == 255 else (5e-4 if n == 256 else 0.0))) for k in SGD_VARIANTS for n in OPT_NS]
RMSPROP = [_row("%s_n%d" % (k, n), "%s, n = %d: %d trip(s)" % (k, n, ew_trips(n)), n=n, variant=k, gs=0.5 if n == 257 else 1.0,
                lr_now=(-0.0 if n == 255 else (5e-4 if n == 256 else 0.0))) for k in RMS_VARIANTS for n in OPT_NS]

_SHAPES = ((1, 1, 1, "the smallest"), (3, 7, 5, "odd sizes, one block"), (2, 1, 257, "mask_out from two blocks"),
           (2, 3, 300, "mask_out from two blocks, T > 1"), (2, 65, 253, "T C = 16 445: the stride loop with 16 384 % C != 0"),
           (2, 2, 16400, "mask_out on the second trip"), (65535, 1, 1, "the largest B"), (2, 0, 5, "T = 0"), (0, 3, 5, "B = 0"))
SPATIAL = [_row("b%dt%dc%d" % (B, T, C), why, B=B, T=T, C=C, gap=3 if (B, T, C) in ((3, 7, 5), (2, 65, 253)) else 0)
           for B, T, C, why in _SHAPES]
NOISE = [dict(r) for r in SPATIAL]
DROP_STEPS = (None, 0, 1, (1 << 32) + 1)
DROP_RATES = (0.25, 0.4, 0.0)
NOISE_STDDEVS = (0.0, 0.01, 1.0)

ROWS = ([_row("c%d" % C, "batch = 1, C = %d" % C, batch=1, rpb=11, C=C, gap=0) for C in (1, 7, 64)]
        + [_row("b3_c%d" % C, "batch = 3, rows_per_batch = 5, gapped strides, C = %d" % C, batch=3, rpb=5, C=C, gap=3) for C in (1, 7, 64)]
        + [_row("trip2", "R C = 1 048 576 + 700: the second trip", batch=1, rpb=(1048576 + 700) // 4, C=4, gap=0),
           _row("trip2_b3", "the second trip through the batch > 1 addressing", batch=3, rpb=49967, C=7, gap=1)])

_BN_V, _BN_S = 4 * 8192 * 256, 8192 * 256
BNRD = ([_row("c%d" % C, "C = %d: %s" % (C, "vector" if C % 4 == 0 else "scalar (C % 4 != 0)"), R=37, C=C, off=None) for C in (4, 6, 100)]
        + [_row("off_%s" % k, "%s 4 bytes off: the scalar kernel" % k, R=37, C=100, off=k) for k in ("x", "scale", "shift", "out", "dy")]
        + [_row("cap_vec", "R C just above 4 x 8192 x 256 on the vector path: the second trip", R=_BN_V // 4 + 3, C=4, off=None),
           _row("cap_scalar", "R C just above 8192 x 256 on the scalar path: the second trip", R=_BN_S // 6 + 3, C=6, off=None)])


def _mla(name, K, T, why, B=2, off=(), ld=0):
    return _row(name, why, B=B, T=T, K=K, off=tuple(off), ld=ld)


def _pass(K, vec4):
    return mla_fwd_plan(1, K, vec4)["pass_rows"]


MLA = ([_mla("k%d" % K, K, 37, "K = %d: <%d,%d>" % (K, mla_plan(K, K % 4 == 0)["vec"], mla_plan(K, K % 4 == 0)["nj"]))
        for K in (4, 100, 256, 260, 516, 1, 3, 63, 127, 255, 511, 1023)]
       + [_mla("k512", 512, 9, "K = 512, T = 9: 16 waves, exactly 64 KiB of LDS, waves without a row"),
          _mla("k1024", 1024, 9, "K = 1024, T = 9: 8 waves, exactly 64 KiB of LDS")]
       + [_mla("k%d_zoff" % K, K, 9, "K = %d with z 4 bytes off: scalar" % K, off=("z",)) for K in (128, 512, 1024)]
       + [_mla("k128_dzoff", 128, 9, "backward with only dz 4 bytes off: forward vector, backward scalar", off=("dz",))]
       + [_mla("g_k%d" % K, K, 19, "G = %d, scalar" % mla_plan(K, False)["G"]) for K in (2, 5, 9, 17, 33)]
       + [_mla("g_k%d" % K, K, 19, "G = %d, vector" % mla_plan(K, True)["G"]) for K in (8, 12, 20, 36, 68, 132)]
       + [_mla("k%d_t%s" % (K, tag), K, max(1, _pass(K, K % 4 == 0) + d), "T = one pass %s: K = %d" % (tag, K))
          for K in (100, 3) for tag, d in (("m1", -1), ("eq", 0), ("p1", 1))]
       + [_mla("k100_t1", 100, 1, "T = 1: one row slot of one wave has a row"),
          _mla("k4_t1025", 4, 1025, "G = 1 at K = 4: 1024 rows in a pass, T = 1025"),
          _mla("k64_trip2", 64, 70, "B = 1024, T = 70, K = 64: gy = 2 of 3, the backward second trip with unequal shares", B=1024),
          _mla("k12_ld", 12, 23, "ld_att and ld_datt = 2 K + 3, at column offset K + 1", ld=27)])

CAVG_SHAPES = ((2, 1), (3, 5), (24, 512), (25, 512), (14, 513), (3, 1024), (3, 1025), (2, 2049))
CAVG = [_row("n%dth%d" % (N, Th), "N Th 4 = %d bytes: lds_pf %d, %d trip(s)" % (N * Th * 4, cavg_lds_pf(N, Th), cavg_trips(Th)), N=N, Th=Th)
        for N, Th in CAVG_SHAPES]
EW = [_row("n%d" % n, "%d trip(s)" % ew_trips(n), n=n) for n in (1, 255, 256, 257, 524288 + 300)]

PATHS = dict(adam=ADAM, sgd=SGD, rmsprop=RMSPROP, spatial=SPATIAL, noise=NOISE, rows=ROWS, bnrd=BNRD, mla=MLA, cavg=CAVG, ew=EW)


def by_name(table, name):
    return next(r for r in PATHS[table] if r["name"] == name)


# ---------------------------------------------------------------------------------------------------- data
def opt_state(n, seed, zero=False):
    """param, grad, and the optimiser slots of a step in flight: second moments above the squared first ones, so the centred
    denominator is well away from cancellation; grads random, not constant.  m doubles as RMSprop's mean_grad, v as its rms"""
    rng = np.random.default_rng([seed, n])
    d = dict(param=rng.standard_normal(n), grad=rng.standard_normal(n), m=0.3 * rng.standard_normal(n))
    d["v"] = d["m"] ** 2 + rng.uniform(0.1, 1.0, n)
    d["velocity"] = 0.1 * rng.standard_normal(n)
    d["mom"] = 0.1 * rng.standard_normal(n)
    if n >= 16:                                          # eight elements whose root is near epsilon: its placement shows there
        d["grad"][:8] *= 1e-5
        d["m"][:8] = 0.0
        d["v"][:8] = 1e-12
    if zero:
        for k in ("m", "v", "velocity", "mom"):
            d[k] = np.zeros(n)
    return {k: a.astype(np.float32) for k, a in d.items()}


def mla_inputs(B, T, K, seed):
    """tests/test_mla_ops_gpu.py's data: N(0, 1) with two entries at -30 in every third row and one at +30 in every fifth"""
    rng = np.random.default_rng([seed, B, T, K])
    z = rng.standard_normal((B * T, K)).astype(np.float32)
    for r in range(0, B * T, 3):
        z[r, r % K] = -30.0
        z[r, (r + 1) % K] = -30.0
    for r in range(0, B * T, 5):
        z[r, (r + 2) % K] = 30.0
    return z.reshape(B, T, K), rng.standard_normal((B, K)).astype(np.float32)


def cavg_counters(N, Th, seed):
    """hand-made integer counters with zeros: language 0 has no example (tp = fn = 0) and pair (1, 0) no trial (fp = tn = 0)"""
    rng = np.random.default_rng([seed, N, Th])
    tp, fn = rng.integers(0, 50, (N, Th)), rng.integers(0, 50, (N, Th))
    fp, tn = rng.integers(0, 50, (N, N, Th)), rng.integers(0, 50, (N, N, Th))
    tp[0] = fn[0] = 0
    fp[1, 0] = tn[1, 0] = 0
    if Th > 1024:                                        # the smallest cost sits behind the first 1024 thresholds
        fn[:, Th - 1], fp[:, :, Th - 1] = 0, 0
        tp[1:, Th - 1], tn[:, :, Th - 1] = 7, 9
    return tuple(a.astype(np.float32) for a in (tp, fn, fp, tn))


HP = dict(adam=dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-7), sgd=dict(lr=0.03), rmsprop=dict(lr=1e-3, rho=0.9, eps=1e-7))
CAVG_COST = dict(C_miss=1.0, C_fa=1.0, P_tar=0.5)
DROP_SEED = 0x1234567887654321


def opt_row_refs(kind, r, d, lr_t, mistake=None):
    """the references of one optimiser row on the data d = opt_state(...): dict name -> (value, bound)"""
    if kind == "adam":
        h = HP["adam"]
        return adam_ref(d["param"], d["grad"], d["m"], d["v"], lr_t, h["b1"], h["b2"], h["eps"], r["gs"], mistake)
    if kind == "sgd":
        k = SGD_VARIANTS[r["variant"]]
        return sgd_ref(d["param"], d["grad"], d["velocity"] if k["mu"] > 0 else None, lr_t, k["mu"], k["nesterov"], r["gs"], mistake)
    k, h = RMS_VARIANTS[r["variant"]], HP["rmsprop"]
    return rmsprop_ref(d["param"], d["grad"], d["v"], d["m"] if k["centered"] else None, d["mom"] if k["mu"] > 0 else None, lr_t,
                       h["rho"], k["mu"], h["eps"], r["gs"], mistake)


def opt_row_emu32(kind, r, d, lr_t):
    if kind == "adam":
        h = HP["adam"]
        return adam_emu32(d["param"], d["grad"], d["m"], d["v"], lr_t, h["b1"], h["b2"], h["eps"], r["gs"])
    if kind == "sgd":
        k = SGD_VARIANTS[r["variant"]]
        return sgd_emu32(d["param"], d["grad"], d["velocity"] if k["mu"] > 0 else None, lr_t, k["mu"], k["nesterov"], r["gs"])
    k, h = RMS_VARIANTS[r["variant"]], HP["rmsprop"]
    return rmsprop_emu32(d["param"], d["grad"], d["v"], d["m"] if k["centered"] else None, d["mom"] if k["mu"] > 0 else None, lr_t,
                         h["rho"], k["mu"], h["eps"], r["gs"])


def opt_row_lr_t(kind, r, mistake=None):
    """(step after, lr_t) of a row; SGD / RMSprop rows start at step 3"""
    if kind == "adam":
        h = HP["adam"]
        return lr_t_ref(h["lr"], r["lr_now"], r["step"], h["b1"], h["b2"], mistake)
    return lr_t_ref(HP[kind]["lr"], r["lr_now"], 3)


def mla_emu32(z, datt):
    """forward and backward in float32 NumPy (NumPy's own summation order)"""
    z = np.asarray(z, np.float32)
    one = np.float32(1)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True, dtype=np.float32)
    c = np.clip(p, np.float32(LO), np.float32(HI))
    u = np.exp(-np.abs(z))
    r = one / (one + u)
    v, dv = np.where(z >= 0, r, u * r), u * r * r
    s, sv = c.sum(1, dtype=np.float32), (c * v).sum(1, dtype=np.float32)
    att = sv / s
    gs = (np.asarray(datt, np.float32) / s)[:, None, :]
    dp = np.where((p >= np.float32(LO)) & (p <= np.float32(HI)), gs * (v - att[:, None, :]), np.float32(0))
    dot = (dp * p).sum(-1, keepdims=True, dtype=np.float32)
    return att, s, p * (dp - dot) + gs * c * dv


def cavg_emu32(tp, fn, fp, tn, C_miss, C_fa, P_tar):
    """the kernel's loops in float32, languages in order"""
    tp, fn, fp, tn = (np.asarray(a, np.float32) for a in (tp, fn, fp, tn))
    N, Th = tp.shape
    one = np.float32(1)

    def dnn(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(b != 0, a / b, np.float32(0)).astype(np.float32)
    pm, pf = np.zeros(Th, np.float32), np.zeros(Th, np.float32)
    for l in range(N):
        pm = pm + dnn(fn[l], fn[l] + tp[l])
        inner = np.zeros(Th, np.float32)
        for m in range(N):
            inner = inner + dnn(fp[l, m], fp[l, m] + tn[l, m])
        pf = pf + dnn(inner, np.float32(N - 1))
    pm, pf = pm / np.float32(N), pf / np.float32(N)
    cm, cf, pt = np.float32(C_miss), np.float32(C_fa), np.float32(P_tar)
    return cm * pt * pm + cf * (one - pt) * pf
