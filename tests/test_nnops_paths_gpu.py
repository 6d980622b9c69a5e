"""
Every kernel and template instantiation of the first half of csrc/nnops.hip (stats / average pooling, the softmax head, the
losses, l2_normalize and the angular-proximity kernels) on each side of each dispatch condition, against the float64 numpy
oracle (oracle/nnops_np.py), through the C ABI.

The shapes that select a path sit in one table per group (POOL_FWD, POOL_BWD, HEAD, LOSSES, L2), each row with the condition of
nnops.hip it is there for; tests/test_oracle_nnops.py proves on the CPU that every row selects what it says.  Every output lies
inside a larger NaN-filled buffer whose words before and after must still be NaN afterwards (tests/guarded.py), every output
starts as NaN, the gaps between pitched rows and batches hold NaN on the way in and on the way out, and the head's workspace
has exactly the size lidbox_softmax_head_workspace returns and starts as NaN.

How results are judged.  Sums: element by element against conv2d_np.error_bound(S, n) = gamma(n) S + n 2^-126 with S the same
operation on absolute values and n the longest chain of roundings:
    pool mean          T + 1 (register kernels: T rows in order, the division) or ceil(T / 16) + 16 + 1 (pool_fwd_kernel: a time
                       group's rows, the 16 groups, the division)
    pool stddev        an interval: the mean's bound goes into every d = x - mean, the bound of sum d d is propagated through
                       clip and sqrt (oracle stddev_interval)
    pool dx            8: 1 / T, dmean / T, dsd / (2 sd) (two), the factor 2 / T (two), x - mean, the fma
    head logits        ceil(K / 64) + 6 + 1 (a lane's chain, six butterfly steps, the bias), judged on logp[n] - logp[0] = z[n] -
                       z[0], which no expf or logf touches: two such bounds plus the rounding of the two subtractions z - lse
    head dW            ceil(B / 16) + 16;  db, mean loss ceil(B / 64) + 6 + 1;  dh NP + 1 -- all three from the DEVICE'S dz and
                       per-row losses (read back from the workspace), so that expf's error stays out of the comparison
    l2_normalize       ceil(D / 64) + 6 for the two sums, propagated through rsqrtf (2 ulp) (oracle l2_bounds)
Through expf / logf / acosf no bound can be derived; there the tolerances the project already asserts hold: log-probabilities
and losses 2e-5 absolute, probabilities 2e-6, cross-entropy gradients 1e-6 (with scale = 1 / B), angular-proximity loss 1e-4.
Masks, zeros, clipped values, bf16 shadows, refusals, run-to-run and fused-versus-separate identity are exact.  Each reduction
case runs on two data sets: N(0, 1) and 1 + 0.1 N(0, 1).
"""
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from lidbox_amd.testutil import device_copy
from oracle import model_np as mo
from oracle import nnops_np as no

pytestmark = pytest.mark.gpu

KINDS = ("normal", "offset")
WORST = {}                                           # group -> largest err / bound seen (printed by every case)

# ---------------------------------------------------------------------------------------------------- PATHS: pooling forward
# name -> (T, C, pitch, misaligned): pitch "dense" rs = C, bs = T rs | "pitched" rs = C + 4, bs = (T + 2) rs | "odd" rs = C + 1,
# bs = T rs; misaligned None | "x" | "out".  B = 3 everywhere.
POOL_B = 3
POOL_FWD = {}
# launch_pool_fwd_short: `T <= 8 / 16 / 24 / 32 / 36` else 40 -- each TMAX at its upper edge and one above the previous edge;
# C = 4: one live lane (`c >= C` returns 63 lanes); C = 260: a second x block that holds one lane
for _T in (1, 8, 9, 16, 17, 24, 25, 32, 33, 36, 37, 40):
    for _C in (4, 260):
        for _p in ("dense", "pitched"):
            POOL_FWD["reg_T%d_C%d_%s" % (_T, _C, _p)] = (_T, _C, _p, None)
# `vec && T <= 40` false -> pool_fwd_kernel<*, 4>: C = 68 is two x blocks (64 + 4 channels), 16 time groups with 2 or 3 (T = 41)
# and 6 or 7 (T = 100) rows each
POOL_FWD["lds4_T41"] = (41, 68, "dense", None)
POOL_FWD["lds4_T100"] = (100, 68, "pitched", None)
# `(out & 15) == 0` false with vec true -> pool_fwd_kernel<*, 4> at T = 5: time groups 5 - 15 idle (`t = g; t < T` never true)
POOL_FWD["lds4_T5_out"] = (5, 68, "dense", "out")
# vec false three ways -> pool_fwd_kernel<*, 1>: `C % 4`, `(x & 15)`, `rs % 4`
for _T in (1, 15, 16, 17, 100):
    POOL_FWD["lds1_T%d_C5" % _T] = (_T, 5, "dense", None)
    POOL_FWD["lds1_T%d_C17" % _T] = (_T, 17, "dense", None)
    POOL_FWD["lds1_T%d_x" % _T] = (_T, 8, "dense", "x")
    POOL_FWD["lds1_T%d_rs" % _T] = (_T, 8, "odd", None)
# a channel constant at 0.5 over T > 1 frames: `fmaxf(var, STDDEV_SQRT_MIN_CLIP)` takes the clip (register and LDS kernel); and a
# channel at 0.5 +- 2^-20, alternating: variance 2^-40 = 9e-13, clipped as well, but x - mean is NOT zero -- a backward that lets
# the clipped stddev pass a gradient multiplies these 1e-6 by dsd / (sd T) = 1e5 dsd / T
POOL_CONST = {"const_T7": (7, 8, "dense", None), "const_T50": (50, 8, "dense", None)}
CONST_CH, NEAR_CH = 3, 4

# ---------------------------------------------------------------------------------------------------- PATHS: pooling backward
# name -> (T, C, pitch, misaligned): misaligned None | "pooled" | "dout" | "dx"
POOL_BWD = {}
# `vec && T <= 48 && pooled, dout aligned` -> pool_bwd_rows_kernel<*, 12>: z = ceil(T / 12) = 1 .. 4 row blocks, the last one
# ragged unless T % 12 == 0 (`t0 + i < T` predicates the store, the load re-reads row T - 1)
for _T in (1, 11, 12, 13, 24, 47, 48):
    for _C in (4, 260):
        for _p in ("dense", "pitched"):
            POOL_BWD["rows_T%d_C%d_%s" % (_T, _C, _p)] = (_T, _C, _p, None)
POOL_BWD["loop4_T49"] = (49, 68, "pitched", None)          # `T <= 48` false -> pool_bwd_kernel<*, 4>, zs = 8 time splits
POOL_BWD["loop4_T5_pooled"] = (5, 68, "dense", "pooled")   # `(pooled & 15)` -> the same kernel with zs = T = 5
POOL_BWD["loop4_T5_dout"] = (5, 68, "dense", "dout")       # `(dout & 15)` -> likewise
POOL_BWD["loop1_T13_C5"] = (13, 5, "dense", None)          # `C % 4` -> pool_bwd_kernel<*, 1>
POOL_BWD["loop1_T13_dx"] = (13, 8, "dense", "dx")          # `(dx & 15)` -> pool_bwd_kernel<*, 1>
POOL_BWD["loop1_T49_C5"] = (49, 5, "dense", None)
POOL_BWD_CONST = {"const_T7": (7, 8, "dense", None), "const_T50": (50, 8, "dense", None)}

# ---------------------------------------------------------------------------------------------------- PATHS: softmax head
# name -> (N, K, B, W misaligned, relu, dh given, invalid labels).  NP, U = head_np_u(N); one trip of a lane covers 64 U values of k
HEAD = {}
for _NP, _U in ((4, 8), (8, 4), (16, 2), (32, 1)):
    # N == NP with an aligned W: `wvec` true (16-byte loads of W's rows).  K = 7: lanes 7 - 63 idle, `lane < K` skips emit;
    # K = 64 U: one full trip, no reload; K = 64 U + 1: only lane 0 takes a second trip (and reloads the first);
    # K = 2 * 64 U + 37: lanes 0 - 36 reload two trips, the others one
    for _K in (7, 64 * _U, 64 * _U + 1, 2 * 64 * _U + 37):
        HEAD["np%d_K%d" % (_NP, _K)] = (_NP, _K, 5, False, 1, True, _K == 7)
    # N == NP with a misaligned W: `wvec` false through the pointer test, scalar loads with stride N == NP
    HEAD["np%d_misW" % _NP] = (_NP, 2 * 64 * _U + 37, 5, True, 1, True, False)
# the lower edge of every NP: N = 1, 5, 9, 17 (`n < N` masks NP - N columns; `wvec` false through N != NP)
for _N, _U in ((1, 8), (5, 4), (9, 2), (17, 1)):
    HEAD["N%d" % _N] = (_N, 64 * _U + 1, 5, False, 1, True, False)
# B = 1: three idle waves (`r >= B`); B = 129: one row past the wgrad kernel's 128-row trip (`r0 += 16 * 8`), B % 4 = 1
HEAD["B1"] = (8, 257, 1, False, 1, True, False)
HEAD["B129_np8"] = (8, 257, 129, False, 1, True, True)
HEAD["B129_np32"] = (32, 165, 129, False, 0, True, True)
HEAD["B129_N3"] = (3, 7, 129, False, 1, True, False)
# `relu_mask` 0, and `dh == NULL` (`if (dh && lane < K)` false: no emit, no reload)
HEAD["norelu"] = (16, 293, 5, False, 0, True, False)
HEAD["nodh_np4"] = (4, 1061, 5, False, 1, False, False)
HEAD["nodh_np32"] = (32, 165, 5, False, 1, False, True)

# ---------------------------------------------------------------------------------------------------- PATHS: losses, l2 / AP
# log_softmax_kernel / softmax_kernel: `for (n = lane; n < N; n += 64)`: N = 63, 64 one trip (lane 63 idle / busy), 65 a second
# trip of lane 0, 130 three trips; nll_kernel / softmax_nll_kernel: `for (b = threadIdx.x; b < B; b += 256)`: B = 256 exactly
# one trip of every thread, 257 a second trip of thread 0
LOSS_N = (1, 63, 64, 65, 130)
LOSS_B = (1, 5, 256, 257)
L2_D = (1, 63, 64, 65)
# (B, D, N): D == N (no zero tail: `d = N + lane; d < D` never true), N = 100 > 64 with labels >= 64 (`n += 64` second trip owns
# the label), N = 1 (no other class: loss 0)
AP = [(5, 63, 3), (5, 64, 64), (5, 65, 17), (6, 100, 100), (5, 1, 1)]


# ---------------------------------------------------------------------------------------------------- plumbing
def _nv():
    from lidbox_amd import _native as nv
    return nv


def _draw(rng, kind, shape):
    z = rng.standard_normal(shape)
    return (z if kind == "normal" else 1.0 + 0.1 * z).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """bit for bit, NaN payloads included"""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _judge(group, what, got, ref, bound):
    got = np.asarray(got, np.float64)
    ref, bound = np.broadcast_to(ref, got.shape), np.broadcast_to(bound, got.shape)
    finite = np.isfinite(got)
    assert finite.all(), "%s: %d elements not written or not finite" % (what, (~finite).sum())
    err = np.abs(got - ref)
    worst = float((err / bound).max()) if got.size else 0.0
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("%-44s max err/bound=%.3e   [%s so far %.3e]" % (what, worst, group, WORST[group]))
    assert (err <= bound).all(), "%s: %d elements over the bound, worst %.3g x at %s" % (
        what, (err > bound).sum(), worst, np.unravel_index(np.argmax(err / bound), err.shape))


def _judge_abs(group, what, got, ref, tol):
    _judge(group, what, got, ref, np.full(np.shape(got), tol))


def _strides(T, C, pitch):
    if pitch == "dense":
        return T * C, C
    if pitch == "pitched":
        return (T + 2) * (C + 4), C + 4
    return T * (C + 1), C + 1


def _pitched(x, bs, rs):
    """x [B, T, C] laid out with row pitch rs and batch pitch bs, NaN in the gaps -> flat float32 [B * bs]"""
    B, T, C = x.shape
    flat = np.full(B * bs, np.nan, np.float32)
    for b in range(B):
        for t in range(T):
            flat[b * bs + t * rs:b * bs + t * rs + C] = x[b, t]
    return flat


def _unpitch(flat, B, T, C, bs, rs):
    """-> (payload [B, T, C], mask of the gap words)"""
    idx = (np.arange(B)[:, None, None] * bs + np.arange(T)[None, :, None] * rs + np.arange(C)[None, None, :])
    gap = np.ones(flat.shape, bool)
    gap[idx.ravel()] = False
    return flat[idx], gap


@functools.lru_cache(maxsize=None)
def _pool_case(T, C, kind, const):
    rng = np.random.default_rng([T, C, KINDS.index(kind), int(const)])
    x = _draw(rng, kind, (POOL_B, T, C))
    dout = _draw(rng, kind, (POOL_B, 2 * C))
    if const:
        x[:, :, CONST_CH] = 0.5
        x[:, :, NEAR_CH] = 0.5 + 2.0 ** -20 * (-1.0) ** np.arange(T)[None, :]
    x.setflags(write=False)
    dout.setflags(write=False)
    return x, dout


# ---------------------------------------------------------------------------------------------------- pooling forward
def _pool_fwd(fn, xflat, T, C, bs, rs, mis, width, x16=False):
    """one forward launch into a NaN-filled guarded [B, width] output (misaligned: one word past a 16-byte boundary)"""
    nv = _nv()
    out = Guarded((POOL_B, width), shift=1 if mis == "out" else 0)
    if x16:
        xd = torch.from_numpy(xflat).cuda().bfloat16()                  # NaN gaps stay NaN
    else:
        xd = device_copy(xflat, misalign=mis == "x")
    nv.check(fn(nv.ptr(xd), POOL_B, T, C, bs, rs, out.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return out.numpy()


def _check_pool_fwd(name, row, kind, const=False):
    nv = _nv()
    T, C, pitch, mis = row
    bs, rs = _strides(T, C, pitch)
    x, _ = _pool_case(T, C, kind, const)
    path = no.pool_fwd_path(T, C, bs, rs, 4 if mis == "x" else 0, 4 if mis == "out" else 0)
    n = no.pool_chain(T, path)
    xflat = _pitched(x, bs, rs)
    mean, var, ref = no.stats_pool_fwd(x)
    got = _pool_fwd(nv.lib.lidbox_stats_pool_fwd, xflat, T, C, bs, rs, mis, 2 * C)
    _judge("pool mean", "stats[%s] %s mean %s" % (name, kind, path), got[:, :C], mean, no.error_bound(no.pool_mean_abs(x), n))
    lo, hi = no.stddev_interval(x, n)
    sd = got[:, C:].astype(np.float64)
    assert np.isfinite(sd).all() and (sd >= lo).all() and (sd <= hi).all(), (name, kind, float((sd - hi).max()), float((lo - sd).max()))
    width = np.maximum(hi - lo, 1e-300)
    WORST["pool stddev"] = max(WORST.get("pool stddev", 0.0), float((np.abs(sd - ref[:, C:]) / width).max()))
    print("stats[%s] %s stddev: max |err| / interval width = %.3e" % (name, kind, float((np.abs(sd - ref[:, C:]) / width).max())))
    avg = _pool_fwd(nv.lib.lidbox_avg_pool_fwd, xflat, T, C, bs, rs, mis, C)
    assert _same(avg, got[:, :C])                                       # the same first pass, whichever kernel
    if T == 1:
        assert _same(got[:, :C], x[:, 0]) and (got[:, C:] == np.sqrt(np.float32(1e-10))).all()
    if const:
        assert (got[:, CONST_CH] == np.float32(0.5)).all() and (got[:, C + CONST_CH] == np.sqrt(np.float32(1e-10))).all()
        assert (got[:, C + NEAR_CH] == np.sqrt(np.float32(1e-10))).all() and 0 < var[:, NEAR_CH].max() < 1e-12
        assert (got[:, C:][:, ~np.isin(np.arange(C), (CONST_CH, NEAR_CH))] > 1e-3).all()
    # the same pooling over the bfloat16 shadow: bit-identical to the fp32 kernel fed the shadow's values
    if mis is None and no.pool_bf16_accepts(T, C, bs, rs, 0, 0):
        x16 = no.bf16_round(x)
        got16 = _pool_fwd(nv.lib.lidbox_stats_pool_fwd_bf16, _pitched(x16, bs, rs), T, C, bs, rs, None, 2 * C, x16=True)
        got32 = _pool_fwd(nv.lib.lidbox_stats_pool_fwd, _pitched(x16, bs, rs), T, C, bs, rs, None, 2 * C)
        assert path[0] == "reg" and _same(got16, got32)
        _judge("pool mean", "stats_bf16[%s] %s mean" % (name, kind), got16[:, :C], no.stats_pool_fwd(x16)[0],
               no.error_bound(no.pool_mean_abs(x16), n))
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(POOL_FWD))
def test_pool_forward(name, kind):
    """stats and average pooling of every POOL_FWD row, fp32 and (where the entry point takes the shape) bfloat16"""
    _check_pool_fwd(name, POOL_FWD[name], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(POOL_CONST))
def test_pool_forward_constant_channel_is_the_clipped_stddev(name, kind):
    """a channel constant at 0.5: mean exactly 0.5, every d exactly 0, stddev exactly sqrtf(1e-10f)"""
    _check_pool_fwd(name, POOL_CONST[name], kind, const=True)


def test_pool_forward_vector_and_scalar_kernels_agree_bit_for_bit():
    """pool_fwd_kernel<*, 4> and <*, 1> add the same rows in the same order (time group g takes t = g, g + 16, ...; the 16 groups
    are added k = 0 .. 15), so a misaligned x must not change one bit.  T = 41, C = 68."""
    nv = _nv()
    T, C = 41, 68
    x, _ = _pool_case(T, C, "normal", False)
    flat = _pitched(x, T * C, C)
    a = _pool_fwd(nv.lib.lidbox_stats_pool_fwd, flat, T, C, T * C, C, None, 2 * C)
    b = _pool_fwd(nv.lib.lidbox_stats_pool_fwd, flat, T, C, T * C, C, "x", 2 * C)
    assert _same(a, b)


# ---------------------------------------------------------------------------------------------------- pooling backward
def _pool_bwd(stats, xflat, pooled, dout, T, C, bs, rs, mis, mask, want_dx=True, shadow=None, x16=False):
    """one backward launch -> (dx flat [B * bs] or None, shadow flat as float32 or None); everything guarded and NaN-filled.
    shadow = (bs16, rs16) asks for the bf16 shadow; x16: lidbox_stats_pool_bwd_bf16 over a bfloat16 x"""
    nv = _nv()
    st = nv.current_stream()
    xd = torch.from_numpy(xflat).cuda().bfloat16() if x16 else device_copy(xflat)
    pd = None if pooled is None else device_copy(np.ascontiguousarray(pooled), misalign=mis == "pooled")
    dd = device_copy(np.ascontiguousarray(dout), misalign=mis == "dout")
    dx = Guarded((POOL_B * bs,), shift=1 if mis == "dx" else 0) if want_dx else None
    sh = Guarded((POOL_B * shadow[0],), torch.bfloat16) if shadow else None
    if x16:
        nv.check(nv.lib.lidbox_stats_pool_bwd_bf16(nv.ptr(xd), nv.ptr(pd), nv.ptr(dd), POOL_B, T, C, bs, rs, mask, sh.ptr, shadow[0],
                                                   shadow[1], st))
    elif shadow:
        nv.check(nv.lib.lidbox_stats_pool_bwd_shadow(nv.ptr(xd), nv.ptr(pd), nv.ptr(dd), POOL_B, T, C, bs, rs, mask,
                                                     dx.ptr if dx else None, sh.ptr, shadow[0], shadow[1], st))
    elif stats:
        nv.check(nv.lib.lidbox_stats_pool_bwd(nv.ptr(xd), nv.ptr(pd), nv.ptr(dd), POOL_B, T, C, bs, rs, mask, dx.ptr, st))
    else:
        nv.check(nv.lib.lidbox_avg_pool_bwd(nv.ptr(xd), nv.ptr(dd), POOL_B, T, C, bs, rs, mask, dx.ptr, st))
    torch.cuda.synchronize()
    return (dx.numpy() if dx else None), (sh.numpy() if sh else None)


def _check_pool_bwd(name, row, kind, const=False):
    T, C, pitch, mis = row
    bs, rs = _strides(T, C, pitch)
    x, dout = _pool_case(T, C, kind, const)
    xflat = _pitched(x, bs, rs)
    pooled = no.stats_pool_fwd(x)[2].astype(np.float32)                 # the forward's output, as fp32 input of the backward
    if const:
        assert (pooled[:, [C + CONST_CH, C + NEAR_CH]] == np.sqrt(np.float32(1e-10))).all()
    out = {}
    for mask in (0, 1):
        flat, _ = _pool_bwd(True, xflat, pooled, dout, T, C, bs, rs, mis, mask)
        dx, gap = _unpitch(flat, POOL_B, T, C, bs, rs)
        assert np.isnan(flat[gap]).all()                                # the gaps of dx stay untouched
        _judge("pool dx", "stats_bwd[%s] %s mask=%d" % (name, kind, mask), dx, no.stats_pool_bwd(x, pooled, dout, mask),
               no.error_bound(no.stats_pool_bwd_abs(x, pooled, dout), 8))
        if mask:
            assert not dx[~(x > 0)].any() and _same(dx[x > 0], out[0][x > 0])
        out[mask] = dx
        aflat, _ = _pool_bwd(False, xflat, None, dout[:, :C], T, C, bs, rs, mis if mis in ("dx", "dout") else None, mask)
        adx, gap = _unpitch(aflat, POOL_B, T, C, bs, rs)
        want = np.broadcast_to((dout[:, None, :C] * (np.float32(1) / np.float32(T))).astype(np.float32), x.shape)
        assert np.isnan(aflat[gap]).all() and _same(adx, np.where(x > 0, want, np.float32(0)) if mask else want)
        assert np.abs(adx - no.avg_pool_bwd(x, dout[:, :C], mask)).max() <= 2 * no.U * np.abs(dout).max() / T
    if const:
        a = (dout[:, CONST_CH] * (np.float32(1) / np.float32(T))).astype(np.float32)
        assert (out[0][:, :, CONST_CH] == a[:, None]).all() and (out[1][:, :, CONST_CH] == a[:, None]).all()   # 0.5 > 0
        assert np.abs(a - dout[:, CONST_CH].astype(np.float64) / T).max() <= 2 * no.U * np.abs(dout[:, CONST_CH]).max() / T
        a = (dout[:, NEAR_CH] * (np.float32(1) / np.float32(T))).astype(np.float32)
        assert (x[:, :, NEAR_CH] != pooled[:, None, NEAR_CH]).all() and np.abs(dout[:, C + NEAR_CH]).min() > 0.01
        assert (out[0][:, :, NEAR_CH] == a[:, None]).all() and (out[1][:, :, NEAR_CH] == a[:, None]).all()
    # the bf16 shadow of dx (row pitch C + 4: pitched), with and without the fp32 output
    if mis is None:
        bs16, rs16 = (T + 1) * (C + 4), C + 4
        for want_dx in (True, False):
            flat, sh = _pool_bwd(True, xflat, pooled, dout, T, C, bs, rs, None, 1, want_dx=want_dx, shadow=(bs16, rs16))
            got16, gap16 = _unpitch(sh, POOL_B, T, C, bs16, rs16)
            assert np.isnan(sh[gap16]).all() and _same(got16, no.bf16_round(out[1]))
            assert flat is None or _same(_unpitch(flat, POOL_B, T, C, bs, rs)[0], out[1])
        if no.pool_bf16_accepts(T, C, bs, rs, 0, 0):
            x16 = no.bf16_round(x)
            f16 = _pitched(x16, bs, rs)
            for mask in (0, 1):
                _, a = _pool_bwd(True, f16, pooled, dout, T, C, bs, rs, None, mask, shadow=(bs16, rs16), x16=True)
                _, b = _pool_bwd(True, f16, pooled, dout, T, C, bs, rs, None, mask, want_dx=False, shadow=(bs16, rs16))
                assert _same(a, b)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(POOL_BWD))
def test_pool_backward(name, kind):
    """stats and average pooling backward of every POOL_BWD row: relu_mask 0 and 1, the bf16 shadow with and without dx, and
    lidbox_stats_pool_bwd_bf16 where it takes the shape"""
    _check_pool_bwd(name, POOL_BWD[name], kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(POOL_BWD_CONST))
def test_pool_backward_constant_channel_gets_dmean_over_T(name, kind):
    """the clipped stddev passes no gradient: `sd > 1.0000001e-5f` is false for sd = sqrtf(1e-10f), dx = dmean * (1 / T) exactly"""
    _check_pool_bwd(name, POOL_BWD_CONST[name], kind, const=True)


def test_pool_backward_vector_and_scalar_kernels_agree_bit_for_bit():
    """pool_bwd_rows_kernel, pool_bwd_kernel<*, 4> and <*, 1> evaluate the same expression fma(k, x - mean, a) per element
    (no sum at all), so the kernel choice must not change one bit.  T = 13, C = 8: rows / misaligned pooled / misaligned dx."""
    T, C = 13, 8
    x, dout = _pool_case(T, C, "normal", False)
    pooled = no.stats_pool_fwd(x)[2].astype(np.float32)
    flat = _pitched(x, T * C, C)
    got = [_pool_bwd(True, flat, pooled, dout, T, C, T * C, C, mis, 1)[0] for mis in (None, "pooled", "dx")]
    assert _same(got[0], got[1]) and _same(got[0], got[2])


# ---------------------------------------------------------------------------------------------------- softmax head
@functools.lru_cache(maxsize=None)
def _head_case(name, kind):
    N, K, B, misW, relu, want_dh, bad = HEAD[name]
    rng = np.random.default_rng([N, K, B, KINDS.index(kind)])
    h, W, b = _draw(rng, kind, (B, K)), _draw(rng, kind, (K, N)), _draw(rng, kind, (N,))
    # logits of order 1 on both data sets (the absolute tolerances of the log-probabilities presume that): K terms of random sign
    # grow like sqrt(K), K terms of one sign like K
    W = (W / np.float32(np.sqrt(K) if kind == "normal" else K)).astype(np.float32)
    y = rng.integers(0, N, size=B).astype(np.int32)
    if bad:
        y[1], y[3] = N, -1
    return h, W, b, y


def _head_run(name, kind, force_dh=False):
    nv = _nv()
    N, K, B, misW, relu, want_dh, bad = HEAD[name]
    want_dh = want_dh or force_dh
    h, W, b, y = _head_case(name, kind)
    hd, Wd, bd, yd = device_copy(h), device_copy(W, misalign=misW), device_copy(b), torch.from_numpy(y).cuda()
    logp, loss, dW, db = Guarded((B, N)), Guarded((1,)), Guarded((K, N)), Guarded((N,))
    dh = Guarded((B, K)) if want_dh else None
    wsb = int(nv.lib.lidbox_softmax_head_workspace(B, K, N))
    ws = Guarded((wsb // 4,))
    nv.check(nv.lib.lidbox_softmax_head_fwd_bwd(nv.ptr(hd), nv.ptr(Wd), nv.ptr(bd), nv.ptr(yd), B, K, N, 1.0 / B, relu, logp.ptr,
                                                loss.ptr, dW.ptr, db.ptr, dh.ptr if dh else None, ws.ptr, wsb, nv.current_stream()))
    torch.cuda.synchronize()
    w = ws.numpy()
    return dict(logp=logp.numpy(), loss=loss.numpy(), dW=dW.numpy(), db=db.numpy(), dh=dh.numpy() if dh else None,
                dz=w[:B * N].reshape(B, N), rows=w[B * N:])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(HEAD))
def test_softmax_head(name, kind):
    nv = _nv()
    N, K, B, misW, relu, want_dh, bad = HEAD[name]
    h, W, b, y = _head_case(name, kind)
    NP, _ = no.head_np_u(N)
    assert nv.lib.lidbox_softmax_head_workspace(B, K, N) == no.head_workspace_bytes(B, K, N)
    got = _head_run(name, kind)
    ref = no.softmax_head(h, W, b, y, 1.0 / B, relu)
    ok = (y >= 0) & (y < N)
    tag = "head[%s] %s " % (name, kind)
    # logits, free of expf / logf: logp[n] - logp[0] = z[n] - z[0]
    lp = got["logp"].astype(np.float64)
    eb = no.error_bound(ref["S_z"], no.head_logit_chain(K))
    _judge("head logits", tag + "z[n] - z[0]", lp - lp[:, :1], ref["z"] - ref["z"][:, :1],
           eb + eb[:, :1] + 2 * no.U * (np.abs(lp) + np.abs(lp[:, :1])) + 2.0 ** -126)
    _judge_abs("head logp", tag + "logp", lp, ref["logp"], 2e-5)
    # loss and dz are functions of the log-probabilities: judged from the device's, as test_log_softmax_and_nll does
    _, ref_dz, ref_rows = no.nll(got["logp"], y, 1.0 / B)
    _judge_abs("head dz", tag + "dz", got["dz"], ref_dz, 1e-6)
    assert not got["dz"][~ok].any() and np.isnan(got["rows"][~ok]).all()
    _judge_abs("head loss", tag + "row losses", got["rows"][ok], ref_rows[ok], 2e-5)
    # the sums over dz, from the device's dz
    dW, S_dW, db, S_db, dh, S_dh = no.head_grads_from_dz(h, W, got["dz"], relu)
    _judge("head dW", tag + "dW", got["dW"], dW, no.error_bound(S_dW, no.head_dw_chain(B)))
    _judge("head db", tag + "db", got["db"], db, no.error_bound(S_db, no.head_db_chain(B)))
    if want_dh:
        _judge("head dh", tag + "dh", got["dh"], dh, no.error_bound(S_dh, NP + 1))
        if relu:
            assert not got["dh"][~(h > 0)].any()
    if bad:
        assert np.isnan(got["loss"][0])
    else:
        rows = got["rows"].astype(np.float64)
        _judge("head loss", tag + "mean loss", got["loss"], rows.sum() / B, no.error_bound(np.abs(rows).sum() / B, no.head_db_chain(B) + 1))
        _judge_abs("head loss", tag + "loss vs oracle", got["loss"], ref["loss"], 2e-5)
    again = _head_run(name, kind)                                        # fixed summation orders: run twice, identical bits
    for k, v in got.items():
        assert (v is None and again[k] is None) or _same(v, again[k]), k


def test_softmax_head_aligned_and_misaligned_W_agree_bit_for_bit():
    """`wvec` only changes how a row of W is loaded (one float4 per four classes instead of four floats); every sum runs in the same
    order, so np*_misW must reproduce np*_K<2 * 64 U + 37> bit for bit"""
    for NP, U in ((4, 8), (8, 4), (16, 2), (32, 1)):
        a, b = _head_run("np%d_K%d" % (NP, 2 * 64 * U + 37), "normal"), _head_run("np%d_misW" % NP, "normal")
        for k, v in a.items():
            assert _same(v, b[k]), (NP, k)


@pytest.mark.parametrize("name", ["nodh_np4", "nodh_np32"])
def test_softmax_head_without_dh_changes_nothing_else(name):
    """`dh == NULL` skips the emit / reload pass only: every other output keeps the bits of the run with dh"""
    a, b = _head_run(name, "normal"), _head_run(name, "normal", force_dh=True)
    assert a["dh"] is None and np.isfinite(b["dh"]).all()
    for k in ("logp", "dW", "db", "dz", "rows", "loss"):
        assert _same(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------- losses
@functools.lru_cache(maxsize=None)
def _loss_case(B, N, kind):
    rng = np.random.default_rng([B, N, KINDS.index(kind)])
    z = (3 * _draw(rng, kind, (B, N))).astype(np.float32)
    y = rng.integers(0, N, size=B).astype(np.int32)
    return z, y


def _row_op(fn, z):
    nv = _nv()
    B, N = z.shape
    out = Guarded((B, N))
    zd = device_copy(z)
    nv.check(fn(nv.ptr(zd), B, N, out.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return out.numpy()


def _loss_op(fn, z, y, with_probs, want_dz=True, want_probs=True):
    """nll (with_probs False) or softmax_nll -> (loss, dz or None, probs or None)"""
    nv = _nv()
    B, N = z.shape
    zd, yd = device_copy(z), torch.from_numpy(y).cuda()
    loss = Guarded((1,))
    dz = Guarded((B, N)) if want_dz else None
    pr = Guarded((B, N)) if with_probs and want_probs else None
    if with_probs:
        nv.check(fn(nv.ptr(zd), nv.ptr(yd), B, N, 1.0 / B, pr.ptr if pr else None, loss.ptr, dz.ptr if dz else None, nv.current_stream()))
    else:
        nv.check(fn(nv.ptr(zd), nv.ptr(yd), B, N, 1.0 / B, loss.ptr, dz.ptr if dz else None, nv.current_stream()))
    torch.cuda.synchronize()
    return loss.numpy(), dz.numpy() if dz else None, pr.numpy() if pr else None


def _bad_labels(y, N):
    y = y.copy()
    y[1], y[3] = N, -1
    return y


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", LOSS_B)
@pytest.mark.parametrize("N", LOSS_N)
def test_log_softmax_and_nll(N, B, kind):
    nv = _nv()
    z, y = _loss_case(B, N, kind)
    tag = "N=%d B=%d %s " % (N, B, kind)
    logp = _row_op(nv.lib.lidbox_log_softmax_fwd, z)
    _judge_abs("log-probabilities", tag + "log_softmax", logp, no.log_softmax(z), 2e-5)
    ref_loss, ref_dz, _ = no.nll(logp, y, 1.0 / B)                     # from the device's log-probabilities
    loss, dz, _ = _loss_op(nv.lib.lidbox_nll_fwd_bwd, logp, y, False)
    _judge_abs("losses", tag + "nll loss", loss, ref_loss, 2e-5)
    _judge_abs("ce gradients", tag + "nll dz", dz, ref_dz, 1e-6)
    loss2, none, _ = _loss_op(nv.lib.lidbox_nll_fwd_bwd, logp, y, False, want_dz=False)
    assert none is None and _same(loss, loss2)                          # `if (dz)` false: the same loss bits
    if B >= 5:
        yb = _bad_labels(y, N)
        loss, dz, _ = _loss_op(nv.lib.lidbox_nll_fwd_bwd, logp, yb, False)
        assert np.isnan(loss[0]) and not dz[1].any() and not dz[3].any()
        keep = np.ones(B, bool)
        keep[[1, 3]] = False
        _judge_abs("ce gradients", tag + "nll dz, invalid labels", dz[keep], ref_dz[keep], 1e-6)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", LOSS_B)
@pytest.mark.parametrize("N", LOSS_N)
def test_softmax_and_softmax_nll(N, B, kind):
    nv = _nv()
    z, y = _loss_case(B, N, kind)
    tag = "N=%d B=%d %s " % (N, B, kind)
    ref_p, ref_loss, ref_dz = no.softmax_nll(z, y, 1.0 / B)
    p = _row_op(nv.lib.lidbox_softmax_fwd, z)
    _judge_abs("probabilities", tag + "softmax", p, ref_p, 2e-6)
    loss, dz, pr = _loss_op(nv.lib.lidbox_softmax_nll_fwd_bwd, z, y, True)
    _judge_abs("probabilities", tag + "softmax_nll probs", pr, ref_p, 2e-6)
    _judge_abs("losses", tag + "softmax_nll loss", loss, ref_loss, 2e-5)
    _judge_abs("ce gradients", tag + "softmax_nll dz", dz, ref_dz, 1e-6)
    loss2, none, none2 = _loss_op(nv.lib.lidbox_softmax_nll_fwd_bwd, z, y, True, want_dz=False, want_probs=False)
    assert none is None and none2 is None and _same(loss, loss2)
    if B >= 5:
        loss, dz, pr2 = _loss_op(nv.lib.lidbox_softmax_nll_fwd_bwd, z, _bad_labels(y, N), True)
        assert np.isnan(loss[0]) and not dz[1].any() and not dz[3].any() and _same(pr, pr2)


def test_losses_stay_finite_when_only_the_maximum_survives():
    """one row at +-80: exp(-160) underflows, softmax is exactly (1, 0, ...), log_softmax exactly (0, -160, ...)"""
    nv = _nv()
    N = 65
    z = np.full((5, N), -80.0, np.float32)
    z[:, 0] = 80.0
    z[2] = np.linspace(-1, 1, N)
    y = np.array([0, 1, 7, 0, 64], np.int32)
    logp, p = _row_op(nv.lib.lidbox_log_softmax_fwd, z), _row_op(nv.lib.lidbox_softmax_fwd, z)
    for r in (0, 1, 3, 4):
        assert logp[r, 0] == 0.0 and (logp[r, 1:] == -160.0).all() and p[r, 0] == 1.0 and not p[r, 1:].any()
    loss, dz, _ = _loss_op(nv.lib.lidbox_nll_fwd_bwd, logp, y, False)
    ref_loss, ref_dz, rows = no.nll(logp, y, 0.2)
    # four of the five row losses are exactly 0 or 160 (the log-probabilities are, and logsumexp of (0, -160, ...) is 0); row 2
    # carries the 2e-5 of a loss through expf / logf, a fifth of it after the mean; the mean itself is a chain of one addition
    # per row of a thread (1), wave_sum's six steps, three across the waves and the division
    assert rows[0] == 0.0 and rows[1] == 160.0 and rows[3] == 0.0 and rows[4] == 160.0
    assert abs(float(loss[0]) - ref_loss) <= no.error_bound(np.abs(rows).sum() / 5, 11) + 2e-5 / 5
    assert np.abs(dz - ref_dz).max() <= 1e-6
    y0 = np.array([0, 0, 7, 0, 0], np.int32)                            # a loss of order 1: the plain 2e-5
    loss0, _, _ = _loss_op(nv.lib.lidbox_nll_fwd_bwd, logp, y0, False)
    assert abs(float(loss0[0]) - no.nll(logp, y0, 0.2)[0]) <= 2e-5
    loss, dz, pr = _loss_op(nv.lib.lidbox_softmax_nll_fwd_bwd, z, y, True)
    ref_p, ref_loss, ref_dz = no.softmax_nll(z, y, 0.2)
    assert np.isfinite(loss).all() and abs(float(loss[0]) - ref_loss) <= 2e-5 and np.abs(dz - ref_dz).max() <= 1e-6
    assert not dz[0].any() and not dz[1].any()                          # every probability of these rows is clipped: no gradient


def test_softmax_nll_clip_cases():
    """the saturated rows of test_model_gpu.py's loss check, here into NaN-filled outputs"""
    nv = _nv()
    rng = np.random.default_rng(11)
    z = rng.standard_normal((7, 6)).astype(np.float32) * 3
    z[0] = [40, 0, 0, 0, 0, 0]                                          # p_0 = 1 - O(1e-17): clipped, zero gradient row
    z[1] = [-30, 0, 0, 0, 0, 1]                                         # p_0 < 1e-7: its own term is clipped
    y = np.array([0, 0, 3, 1, 5, 2, 4], np.int32)
    loss, dz, pr = _loss_op(nv.lib.lidbox_softmax_nll_fwd_bwd, z, y, True)
    rl, rdz = mo.sparse_ce_from_probs(z, y)
    assert abs(float(loss[0]) - rl) <= 1e-5 * abs(rl) and np.abs(dz - rdz).max() <= 1e-6
    assert np.abs(dz[0]).max() <= 1e-9 and np.abs(pr - mo.softmax(z.astype(np.float64))).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- l2_normalize, angular proximity
def _l2(x, g=None):
    nv = _nv()
    B, D = x.shape
    out = Guarded((B, D))
    xd = device_copy(x)
    if g is None:
        nv.check(nv.lib.lidbox_l2_normalize_fwd(nv.ptr(xd), B, D, out.ptr, nv.current_stream()))
    else:
        gd = device_copy(g)
        nv.check(nv.lib.lidbox_l2_normalize_bwd(nv.ptr(xd), nv.ptr(gd), B, D, out.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return out.numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", L2_D)
def test_l2_normalize_forward_backward(D, kind):
    """B = 6 (a second workgroup of two rows); row 2 is all zero: `s < L2_EPS`, the clipped branch with k = 0 -- y = 0 and
    dx = g / sqrt(1e-12) = g * 1e6"""
    rng = np.random.default_rng([D, KINDS.index(kind)])
    x, g = _draw(rng, kind, (6, D)), _draw(rng, kind, (6, D))
    x[2] = 0.0
    y, dx = _l2(x), _l2(x, g)
    _judge("l2 norms", "l2_normalize D=%d %s" % (D, kind), y, no.l2_normalize(x), no.l2_bounds(x))
    _judge("l2 norms", "l2_normalize_bwd D=%d %s" % (D, kind), dx, no.l2_normalize_bwd(x, g), no.l2_bounds(x, g))
    assert not y[2].any() and np.abs(dx[2] - g[2].astype(np.float64) * 1e6).max() <= 8 * no.U * 1e6 * np.abs(g[2]).max()


def _ap_rows(B, D, N, rng):
    x = rng.standard_normal((B, D)).astype(np.float32)
    y = rng.integers(0, N, size=B).astype(np.int32)
    if N > 64:
        y[0], y[1] = 64, N - 1                                          # the label sits in a lane's second trip
    x[2] = 0.0                                                          # clipped normalisation
    if B > 5:
        y[5] = N                                                        # invalid label: NaN loss, zero gradient row
    return x, y


@pytest.mark.parametrize("B,D,N", AP)
def test_ap_head_is_the_four_separate_calls_bit_for_bit(B, D, N):
    nv = _nv()
    st = nv.current_stream()
    x, y = _ap_rows(B, D, N, np.random.default_rng([B, D, N]))
    xd, yd = device_copy(x), torch.from_numpy(y).cuda()
    zn, dzn, dx, per, sc = Guarded((B, D)), Guarded((B, D)), Guarded((B, D)), Guarded((B,)), Guarded((B, N))
    nv.check(nv.lib.lidbox_l2_normalize_fwd(nv.ptr(xd), B, D, zn.ptr, st))
    nv.check(nv.lib.lidbox_ap_loss_fwd_bwd(zn.ptr, nv.ptr(yd), B, D, N, 1.7, 1.0 / B, per.ptr, dzn.ptr, st))
    nv.check(nv.lib.lidbox_l2_normalize_bwd(nv.ptr(xd), dzn.ptr, B, D, dx.ptr, st))
    nv.check(nv.lib.lidbox_neg_acos(zn.ptr, B, D, N, sc.ptr, st))
    zn2, dx2, per2, sc2 = Guarded((B, D)), Guarded((B, D)), Guarded((B,)), Guarded((B, N))
    nv.check(nv.lib.lidbox_ap_head_fwd_bwd(nv.ptr(xd), nv.ptr(yd), B, D, N, 1.7, 1.0 / B, zn2.ptr, per2.ptr, dx2.ptr, sc2.ptr, st))
    torch.cuda.synchronize()
    z = zn.numpy()
    assert _same(zn2.numpy(), z) and _same(dx2.numpy(), dx.numpy()) and _same(sc2.numpy(), sc.numpy())
    assert _same(per2.numpy(), per.numpy())
    # against the oracle, from the device's normalised rows
    ok = (y >= 0) & (y < N)
    loss, dz = per.numpy(), dzn.numpy()
    assert np.isnan(loss[~ok]).all() and not dz[~ok].any() and not dz[:, N:].any()
    assert np.abs(loss[ok] - mo.ap_loss_per_example(y[ok], z[ok].astype(np.float64), N, 1.7)).max() <= 1e-4
    ref = mo.ap_loss_grad(y[ok], z[ok].astype(np.float64), N, 1.7) * ok.sum() / B
    assert np.abs(dz[ok] - ref).max() <= 1e-4 * max(1e-30, np.abs(ref).max())
    assert np.abs(sc.numpy() + np.arccos(z[:, :N].astype(np.float64))).max() <= 2e-6


def test_ap_loss_at_a_coordinate_of_exactly_one():
    """z = +-e_j: 1 - z^2 = 0 and the derivative of acos takes the AP_ACOS_CLAMP floor, rsqrt(1e-6) = 1000"""
    nv = _nv()
    B, D, N = 4, 8, 5
    z = np.zeros((B, D), np.float32)
    z[0, 0], z[1, 2], z[2, 1], z[3, 4] = 1.0, -1.0, 1.0, -1.0
    y = np.array([0, 2, 3, 0], np.int32)
    zd, yd = device_copy(z), torch.from_numpy(y).cuda()
    per, dz = Guarded((B,)), Guarded((B, D))
    nv.check(nv.lib.lidbox_ap_loss_fwd_bwd(nv.ptr(zd), nv.ptr(yd), B, D, N, 1.0, 0.25, per.ptr, dz.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    z64 = z.astype(np.float64)
    assert np.abs(per.numpy() - mo.ap_loss_per_example(y, z64, N, 1.0)).max() <= 1e-4
    ref = mo.ap_loss_grad(y, z64, N, 1.0, clamp=no.AP_ACOS_CLAMP)
    got = dz.numpy()
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() and np.abs(ref).max() > 10
