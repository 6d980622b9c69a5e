"""
Every kernel of csrc/batchnorm.hip and csrc/attention.hip on each side of each dispatch condition, against the float64 numpy
oracle (oracle/nnops_np.py), through the C ABI.

The shapes sit in tables (BN_SMALL, BN_LARGE, BN_ROWS, BN_TRIPS, ATTENTION), each row with the condition it is there for;
tests/test_oracle_nnops.py proves on the CPU that every row selects what it says.  Every output lies inside a larger NaN-filled
buffer whose words before and after must still be NaN afterwards (tests/guarded.py), every output starts as NaN, the gaps of a
rows descriptor hold NaN on the way in and on the way out, and the batch-norm workspace has exactly the size lidbox_bn_workspace
returns and starts as NaN -- a slice that owns no row must store zeros into it.

How results are judged.
  Batch-norm statistics are accumulated in float64 and rounded to fp32 once: a sum of R terms through at most DCHAIN = 200
    float64 additions (a thread's rows, four row groups, a thread's slices, the tree of 256) carries 200 * 2^-53 of its absolute
    sum, the rounding to fp32 one u:  |mean - ref| <= u |ref| + DNOISE mean |x|.  dbeta and dgamma likewise with
    conv2d_np.error_bound(S, n): n = 1 for dbeta, n = 3 for dgamma (xhat = (x - mean) invstd is formed in fp32: two roundings).
    invstd goes through sqrtf and a division: 2e-6 relative, the tolerance test_xvector2d_gpu.py asserts.  scale = gamma * invstd
    is one fp32 product of the device's invstd: exact.  shift = beta - mean * scale: two roundings or one (contracted), 2 u of
    |beta| + |mean scale|.  Momentum 0 and 1 make the moving statistics exact: mm * 0 + mean * 1 and mm * 1 + mean * 0.
  lidbox_bn_apply is one fused multiply-add per element: exact against conv2d_np.fma32.
  bn dx = k_dy (dy - mean_dy - xhat mean_dyx): ten roundings (three constants, two for xhat, two products, two differences, the
    final product): error_bound(S, 10) with S the expression on absolute values, plus |k_dy| (e_dbeta + |xhat| e_dgamma) / R for
    the error the two means inherit from their sums (oracle bn_dx_bound): mean_dyx = dgamma / R carries the error of a sum of R
    terms of random sign over fp32 xhat, which where dy, mean_dy and mean_dyx are all small is many times u |mean_dyx|.
  Attention weights go through expf: 2e-6 absolute (test_variants_gpu.py).  Hw = H * F[bin] and dH = dHw * F[bin] are one fp32
    product of the device's / the given F: exact.  dF is a chain of C / d_f fused multiply-adds: error_bound(S, C / d_f); dlogits
    = F (dF - sum F dF) propagates it (oracle freq_attention_dlogits_bound).
Each reduction case runs on two data sets, N(0, 1) and 1 + 0.1 N(0, 1); the statistics also on 1000 + N(0, 1), the
cancellation case the float64 accumulators are there for.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from lidbox_amd.testutil import device_copy
from oracle import nnops_np as no

pytestmark = pytest.mark.gpu

KINDS = ("normal", "offset")
EPS = 1e-3
DNOISE = 200 * 2.0 ** -53
WORST = {}

# ---------------------------------------------------------------------------------------------------- PATHS: batch norm
# bn_slices(R) = clamp(R / 256, 1, 1024), rows per slice = ceil(R / slices)
BN_R = (
    1,            # one row: `bessel && R > 1` false, the population variance (0) moves the running variance
    255, 256,     # one slice of 255 / 256 rows
    511,          # still one slice (511 / 256 = 1) of 511 rows
    512,          # two slices of 256
    513,          # two slices, 257 and 256 rows: a short last slice
)
BN_C = (1, 4, 63, 64, 65, 68)            # `c < C` at one column, both sides of BN_COLS = 64; C % 4 == 0 (vector apply) and not
BN_SMALL = [(R, C) for R in BN_R for C in BN_C]
BN_LARGE = [
    (65792, 4),       # 257 slices: bn_channel_sums' `for (k = t; k < slices; k += 256)` takes a second trip, of thread 0 only
    (262145, 4),      # the cap of 1024 slices, 257 rows each: slice 1020 holds 5 rows, slices 1021 - 1023 none
]
# y / dy through a rows descriptor: (batch, rows per batch, C, batch stride - rows per batch * C): `batch_stride % 4 == 0` keeps the
# vector kernel, % 4 == 2 selects the scalar one
BN_ROWS = [(3, 171, 4, 4), (3, 171, 4, 2), (3, 171, 68, 8), (3, 171, 68, 6), (2, 7, 5, 3)]
# grid-stride second trips: bn_grid() caps the grid at 8192 workgroups of 256
BN_TRIPS = [
    (4099, 2048),     # R C / 4 = 2 098 688 > 8192 * 256 float4: bn_apply_kernel<true>, bn_bwd_apply_kernel<true>
    (419431, 5),      # R C = 2 097 155 > 8192 * 256 floats with C % 4 != 0: the <false> kernels
]

# ---------------------------------------------------------------------------------------------------- PATHS: frequency attention
# (rows, C, d_f).  rows_grid() caps the grid at 2048 workgroups of 4 waves: 8192 rows per trip
ATTENTION = dict(
    one=(1, 8, 2),                 # three idle waves (`row < rows` false at once)
    five=(5, 8, 2),                # a second workgroup of one wave
    trip2_a=(8193, 8, 2),          # row 8192: a second trip for wave 0 of workgroup 0 -- the first `wave_lds_sync` now has a previous row
    trip2_b=(8197, 8, 2),          # ... for all four waves of workgroup 0 and wave 0 of workgroup 1
    df1_cb1=(5, 1, 1),             # d_f = 1: softmax of one logit is 1; C = 1
    df1_cb4=(5, 4, 1),
    df63_cb1=(5, 63, 63),          # lane 63 idle (`lane < d_f`), cb = 1: dF is one product; C % 4 != 0: scalar
    df63_cb4=(5, 252, 63),
    df64_cb1=(5, 64, 64),          # every lane holds a bin
    df64_cb4=(5, 256, 64),         # `c += 256` exactly one float4 trip
    scalar=(5, 7, 1),              # C % 4 != 0
    max_c=(3, 4096, 64),           # the backward's LDS maximum (MAX_C_BWD): 4 * 2 * 4096 floats + tables
)


# ---------------------------------------------------------------------------------------------------- plumbing
def _nv():
    from lidbox_amd import _native as nv
    return nv


def _draw(rng, kind, shape):
    z = rng.standard_normal(shape)
    return (z if kind == "normal" else (1000.0 + z) if kind == "far" else 1.0 + 0.1 * z).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
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


def _bn_workspace(R, C):
    """exactly lidbox_bn_workspace(R, C) bytes, NaN-filled, guarded"""
    nv = _nv()
    nbytes = int(nv.lib.lidbox_bn_workspace(R, C))
    assert nbytes == no.bn_workspace_bytes(R, C) and nbytes % 4 == 0
    return Guarded((nbytes // 4,)), nbytes


def _check_partials(ws, R, C, consts_written):
    """the [2][C][slices] float64 partials are all written, and the slices that own no row hold exact zeros; the three constant
    rows behind them are written by the backward only"""
    w = ws.numpy()
    slices = no.bn_slices(R)
    part = w[:slices * 2 * C * 2].view(np.float64).reshape(2 * C, slices)
    assert np.isfinite(part).all()
    empty = [s for s, n in enumerate(no.bn_slice_rows(R)) if n == 0]
    assert not part[:, empty].view(np.int64).any()
    tail = w[slices * 2 * C * 2:]
    assert tail.size == 3 * C and (np.isfinite(tail).all() if consts_written else np.isnan(tail).all())
    return part


def _rows_layout(a, batch, rpb, C, gap):
    """a [batch * rpb, C] with batch pitch rpb * C + gap, NaN in the gaps -> flat float32"""
    bs = rpb * C + gap
    flat = np.full(batch * bs, np.nan, np.float32)
    for b in range(batch):
        flat[b * bs:b * bs + rpb * C] = a[b * rpb:(b + 1) * rpb].ravel()
    return flat, bs


def _rows_payload(flat, batch, rpb, C, bs):
    idx = (np.arange(batch)[:, None] * bs + np.arange(rpb * C)[None, :]).ravel()
    gap = np.ones(flat.shape, bool)
    gap[idx] = False
    return flat[idx].reshape(batch * rpb, C), gap


# ---------------------------------------------------------------------------------------------------- batch norm: statistics
def _train_stats(x, gamma, beta, momentum, bessel, mm0, mv0):
    """-> dict of the six outputs (moving statistics None when mm0 is None) and the workspace's partials"""
    nv = _nv()
    R, C = x.shape
    xd, gd, bd = device_copy(x), device_copy(gamma), device_copy(beta)
    outs = {k: Guarded((C,)) for k in ("mean", "invstd", "scale", "shift")}
    mm = None if mm0 is None else Guarded((C,), init=torch.from_numpy(mm0).cuda())
    mv = None if mv0 is None else Guarded((C,), init=torch.from_numpy(mv0).cuda())
    ws, wsb = _bn_workspace(R, C)
    nv.check(nv.lib.lidbox_bn_train_stats_ex(nv.ptr(xd), R, C, nv.ptr(gd), nv.ptr(bd), EPS, momentum, bessel, mm.ptr if mm else None,
                                             mv.ptr if mv else None, outs["mean"].ptr, outs["invstd"].ptr, outs["scale"].ptr,
                                             outs["shift"].ptr, ws.ptr, wsb, nv.current_stream()))
    torch.cuda.synchronize()
    got = {k: v.numpy() for k, v in outs.items()}
    got["moving_mean"] = mm.numpy() if mm else None
    got["moving_var"] = mv.numpy() if mv else None
    got["partials"] = _check_partials(ws, R, C, consts_written=False)
    return got


@functools.lru_cache(maxsize=None)
def _bn_case(R, C, kind):
    rng = np.random.default_rng([R, C, ("normal", "offset", "far").index(kind)])
    x = _draw(rng, kind, (R, C))
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32) * rng.choice(np.float32([1, -1]), C)
    beta = rng.standard_normal(C).astype(np.float32)
    mm0, mv0 = rng.standard_normal(C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    dy = _draw(rng, "normal" if kind == "far" else kind, (R, C))
    for a in (x, gamma, beta, mm0, mv0, dy):
        a.setflags(write=False)
    return x, gamma, beta, mm0, mv0, dy


def _check_stats(R, C, kind):
    x, gamma, beta, mm0, mv0, _ = _bn_case(R, C, kind)
    tag = "bn_stats R=%d C=%d %s " % (R, C, kind)
    ax = np.abs(x.astype(np.float64))
    base = None
    for bessel, momentum in ((1, 0.0), (0, 0.0), (1, 1.0), (0, 1.0), (1, None)):
        got = _train_stats(x, gamma, beta, momentum or 0.0, bessel, None if momentum is None else mm0, None if momentum is None else mv0)
        ref = no.bn_train_stats(x, gamma, beta, EPS, momentum or 0.0, bessel, mm0, mv0)
        if base is None:
            base = got
            _judge("bn mean", tag + "mean", got["mean"], ref["mean"], no.U * np.abs(ref["mean"]) + DNOISE * ax.mean(axis=0) + 2.0 ** -126)
            _judge("bn invstd", tag + "invstd", got["invstd"], ref["invstd"], 2e-6 * ref["invstd"])
            assert _same(got["scale"], gamma * got["invstd"])
            ms = got["mean"].astype(np.float64) * got["scale"]
            _judge("bn shift", tag + "shift", got["shift"], beta - ms, 2 * no.U * (np.abs(beta) + np.abs(ms)) + 2.0 ** -126)
            # the partials are float64 sums of x and x^2 over each slice
            rps, slices = no.bn_rows_per_slice(R), no.bn_slices(R)
            x64 = x.astype(np.float64)
            want = np.stack([x64[s * rps:(s + 1) * rps].sum(axis=0) for s in range(slices)], axis=1)
            absw = np.stack([ax[s * rps:(s + 1) * rps].sum(axis=0) for s in range(slices)], axis=1)
            assert (np.abs(got["partials"][:C] - want) <= DNOISE * absw).all()
            want2 = np.stack([(x64[s * rps:(s + 1) * rps] ** 2).sum(axis=0) for s in range(slices)], axis=1)
            assert (np.abs(got["partials"][C:] - want2) <= DNOISE * want2).all()       # x^2 is exact in float64
        else:
            for k in ("mean", "invstd", "scale", "shift"):               # the statistics do not depend on the moving ones
                assert _same(got[k], base[k]), k
            assert np.array_equal(got["partials"].view(np.int64), base["partials"].view(np.int64))
        if momentum is None:
            assert got["moving_mean"] is None
        elif momentum == 1.0:
            assert _same(got["moving_mean"], mm0) and _same(got["moving_var"], mv0)
        else:
            assert _same(got["moving_mean"], got["mean"])
            target = ref["moving_var"]
            _judge("bn moving_var", tag + "moving_var bessel=%d" % bessel, got["moving_var"], target,
                   2 * no.U * target + 2 * DNOISE * (ax ** 2).mean(axis=0) * (R / max(R - 1.0, 1.0)) + 2.0 ** -126)
            if R == 1:
                assert not got["moving_var"].any() and _same(got["invstd"], np.full(C, np.float32(1) / np.sqrt(np.float32(EPS)), np.float32))


@pytest.mark.parametrize("kind", KINDS + ("far",))
@pytest.mark.parametrize("R,C", BN_SMALL + BN_LARGE)
def test_bn_train_stats(R, C, kind):
    """lidbox_bn_train_stats_ex: bessel 0 / 1, momentum 0 / 1, moving statistics given and NULL"""
    _check_stats(R, C, kind)


# ---------------------------------------------------------------------------------------------------- batch norm: apply
def _apply(x, scale, shift, mis=False, rows=None):
    """lidbox_bn_apply -> y [R, C]; rows = (batch, rows per batch, gap): through a rows descriptor with NaN gaps that must survive"""
    nv = _nv()
    R, C = x.shape
    mis = ("x",) if mis is True else (mis or ())
    xd, sd, hd = device_copy(x, misalign="x" in mis), device_copy(scale, misalign="scale" in mis), device_copy(shift, misalign="shift" in mis)
    if rows is None:
        y = Guarded((R, C), shift=1 if "y" in mis else 0)
        desc = nv.Rows(y.view.data_ptr(), 0, C, 1, R)
    else:
        batch, rpb, gap = rows
        bs = rpb * C + gap
        y = Guarded((batch * bs,))
        desc = nv.Rows(y.view.data_ptr(), bs, C, batch, rpb)
    nv.check(nv.lib.lidbox_bn_apply(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), desc, nv.current_stream()))
    torch.cuda.synchronize()
    if rows is None:
        return y.numpy()
    out, gapmask = _rows_payload(y.numpy(), batch, rpb, C, bs)
    assert np.isnan(y.numpy()[gapmask]).all()
    return out


def _bwd(x, dy, mean, invstd, gamma, mask, mis=False, rows=None):
    """lidbox_bn_bwd -> (dgamma, dbeta, dx); rows = (batch, rows per batch, gap): dy through a rows descriptor with NaN gaps"""
    nv = _nv()
    R, C = x.shape
    mis = ("x",) if mis is True else (mis or ())
    xd, md, sd, gd = (device_copy(x, misalign="x" in mis), device_copy(mean, misalign="mean" in mis),
                      device_copy(invstd, misalign="invstd" in mis), device_copy(gamma))
    if rows is None:
        dyd = device_copy(dy, misalign="dy" in mis)
        desc = nv.Rows(dyd.data_ptr(), 0, C, 1, R)
    else:
        batch, rpb, gap = rows
        flat, bs = _rows_layout(dy, batch, rpb, C, gap)
        dyd = device_copy(flat)
        desc = nv.Rows(dyd.data_ptr(), bs, C, batch, rpb)
    dgam, dbet, dx = Guarded((C,)), Guarded((C,)), Guarded((R, C), shift=1 if "dx" in mis else 0)
    ws, wsb = _bn_workspace(R, C)
    nv.check(nv.lib.lidbox_bn_bwd(nv.ptr(xd), desc, R, C, nv.ptr(md), nv.ptr(sd), nv.ptr(gd), mask, dgam.ptr, dbet.ptr, dx.ptr, ws.ptr,
                                  wsb, nv.current_stream()))
    torch.cuda.synchronize()
    part = _check_partials(ws, R, C, consts_written=True)
    # the partials are float64 sums of dy and of dy * xhat over each slice, xhat = (x - mean) * invstd formed in fp32
    rps, slices = no.bn_rows_per_slice(R), no.bn_slices(R)
    d64 = dy.astype(np.float64)
    t64 = d64 * ((x - mean).astype(np.float32) * invstd).astype(np.float32)
    for got, term in ((part[:C], d64), (part[C:], t64)):
        want = np.stack([term[s * rps:(s + 1) * rps].sum(axis=0) for s in range(slices)], axis=1)
        absw = np.stack([np.abs(term[s * rps:(s + 1) * rps]).sum(axis=0) for s in range(slices)], axis=1)
        assert (np.abs(got - want) <= DNOISE * absw).all()
    return dgam.numpy(), dbet.numpy(), dx.numpy()


def _consts(x, gamma, beta):
    """fp32 inputs of apply / backward: the oracle's statistics rounded to fp32"""
    s = no.bn_train_stats(x, gamma, beta, EPS, 0.0, 0)
    return tuple(s[k].astype(np.float32) for k in ("mean", "invstd", "scale", "shift"))


def _check_bwd(tag, x, dy, gamma, beta, mis=False, rows=None, masks=(0, 1)):
    mean, invstd, _, _ = _consts(x, gamma, beta)
    R = x.shape[0]
    out = {}
    for mask in masks:
        dgam, dbet, dx = _bwd(x, dy, mean, invstd, gamma, mask, mis, rows)
        ref = no.bn_bwd(x, dy, mean, invstd, gamma, mask)
        e_db, e_dg = no.error_bound(ref["S_dbeta"], 1) + DNOISE * ref["S_dbeta"], no.error_bound(ref["S_dgamma"], 3) + DNOISE * ref["S_dgamma"]
        _judge("bn dbeta", tag + "dbeta mask=%d" % mask, dbet, ref["dbeta"], e_db)
        _judge("bn dgamma", tag + "dgamma mask=%d" % mask, dgam, ref["dgamma"], e_dg)
        _judge("bn dx", tag + "dx mask=%d" % mask, dx, ref["dx"], no.bn_dx_bound(ref, R, e_db, e_dg))
        if mask:
            assert not dx[~(x > 0)].any()
        out[mask] = (dgam, dbet, dx)
    if len(out) == 2:                                                   # the mask only zeroes elements of dx
        assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1]) and _same(out[0][2][x > 0], out[1][2][x > 0])
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,C", BN_SMALL + BN_LARGE)
def test_bn_apply_and_backward_dense(R, C, kind):
    """lidbox_bn_apply (exact) and lidbox_bn_bwd with relu_mask 0 and 1 on every statistics row; at C % 4 == 0 also from a
    misaligned x: the scalar kernels evaluate the same per-element expressions, so not one bit may change"""
    x, gamma, beta, _, _, dy = _bn_case(R, C, kind)
    _, _, scale, shift = _consts(x, gamma, beta)
    y = _apply(x, scale, shift)
    assert _same(y, no.bn_apply(x, scale, shift))
    out = _check_bwd("bn_bwd R=%d C=%d %s " % (R, C, kind), x, dy, gamma, beta)
    if C % 4 == 0 and R <= 513:
        assert no.bn_apply_path(R, C, (4, 0, 0, 0), C, 1, 0)[0] is False
        assert _same(_apply(x, scale, shift, mis=True), y)
        mean, invstd, _, _ = _consts(x, gamma, beta)
        dgam, dbet, dx = _bwd(x, dy, mean, invstd, gamma, 1, mis=True)
        assert _same(dgam, out[1][0]) and _same(dbet, out[1][1]) and _same(dx, out[1][2])
        if (R, C) == (513, 68):                                         # each of the other pointers the host conditions test, alone
            for which in ("y", "scale", "shift"):
                assert no.bn_apply_path(R, C, (0, 4), C, 1, 0)[0] is False and _same(_apply(x, scale, shift, mis=(which,)), y), which
            for which in ("dy", "dx", "mean", "invstd"):
                got = _bwd(x, dy, mean, invstd, gamma, 1, mis=(which,))
                assert all(_same(u, v) for u, v in zip(got, out[1])), which


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("batch,rpb,C,gap", BN_ROWS)
def test_bn_apply_and_backward_through_a_rows_descriptor(batch, rpb, C, gap, kind):
    """y and dy with batch > 1: the gaps between batches hold NaN, are never read and never written; the results have the bits
    of the dense call"""
    R = batch * rpb
    x, gamma, beta, _, _, dy = _bn_case(R, C, kind)
    _, _, scale, shift = _consts(x, gamma, beta)
    assert _same(_apply(x, scale, shift, rows=(batch, rpb, gap)), no.bn_apply(x, scale, shift))
    a = _check_bwd("bn_bwd rows %s %s " % ((batch, rpb, C, gap), kind), x, dy, gamma, beta, rows=(batch, rpb, gap))
    mean, invstd, _, _ = _consts(x, gamma, beta)
    dense = _bwd(x, dy, mean, invstd, gamma, 1)
    assert all(_same(u, v) for u, v in zip(a[1], dense))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,C", BN_TRIPS)
def test_bn_apply_and_backward_second_grid_stride_trip(R, C, kind):
    """more elements than 8192 workgroups of 256 cover in one trip, for the vector and for the scalar kernels"""
    rng = np.random.default_rng([R, C, KINDS.index(kind)])
    x, dy = _draw(rng, kind, (R, C)), _draw(rng, kind, (R, C))
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    _, _, scale, shift = _consts(x, gamma, beta)
    assert _same(_apply(x, scale, shift), no.bn_apply(x, scale, shift))
    _check_bwd("bn_bwd R=%d C=%d %s " % (R, C, kind), x, dy, gamma, beta, masks=(1,))


# ---------------------------------------------------------------------------------------------------- frequency attention
@functools.lru_cache(maxsize=None)
def _att_case(name, kind):
    rows, C, d_f = ATTENTION[name]
    rng = np.random.default_rng([rows, C, d_f, KINDS.index(kind)])
    H = _draw(rng, kind, (rows, C))
    logits = (2 * _draw(rng, kind, (rows, d_f))).astype(np.float32)
    dHw = _draw(rng, kind, (rows, C))
    return H, logits, dHw


def _att_fwd(H, logits, d_f, mis=()):
    """F_out aliases logits, as the model calls it -> (F, Hw).  mis: which of "H", "Hw" sit one float past a 16-byte boundary"""
    nv = _nv()
    rows, C = H.shape
    hd = device_copy(H, misalign="H" in mis)
    F = Guarded((rows, d_f), init=torch.from_numpy(logits).cuda())
    Hw = Guarded((rows, C), shift=1 if "Hw" in mis else 0)
    nv.check(nv.lib.lidbox_freq_attention_fwd(nv.ptr(hd), F.ptr, rows, C, d_f, F.ptr, Hw.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return F.numpy(), Hw.numpy()


def _att_bwd(H, F, dHw, d_f, relu, mis=()):
    """mis: which of "H", "dHw", "dH" are misaligned"""
    nv = _nv()
    rows, C = H.shape
    hd, fd, dd = device_copy(H, misalign="H" in mis), device_copy(F), device_copy(dHw, misalign="dHw" in mis)
    dl, dH = Guarded((rows, d_f)), Guarded((rows, C), shift=1 if "dH" in mis else 0)
    nv.check(nv.lib.lidbox_freq_attention_bwd(nv.ptr(hd), nv.ptr(fd), nv.ptr(dd), rows, C, d_f, relu, dl.ptr, dH.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return dl.numpy(), dH.numpy()


def _bin_weights(F, C):
    return np.repeat(F, C // F.shape[1], axis=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(ATTENTION))
def test_freq_attention_forward_backward(name, kind):
    rows, C, d_f = ATTENTION[name]
    H, logits, dHw = _att_case(name, kind)
    tag = "attention[%s] %s " % (name, kind)
    F, Hw = _att_fwd(H, logits, d_f)
    refF, _ = no.freq_attention_fwd(H, logits)
    _judge("attention weights", tag + "F", F, refF, np.full(F.shape, 2e-6))
    assert _same(Hw, H * _bin_weights(F, C))                            # one fp32 product of the device's weights
    if d_f == 1:
        assert (F == 1.0).all()
    for relu in (0, 1):
        dl, dH = _att_bwd(H, F, dHw, d_f, relu)
        ref = no.freq_attention_bwd(H, F, dHw, relu)
        want = dHw * _bin_weights(F, C)
        assert _same(dH, np.where(H > 0, want, np.float32(0)) if relu else want)
        _judge("attention dlogits", tag + "dlogits relu=%d" % relu, dl, ref["dlogits"],
               no.freq_attention_dlogits_bound(F, ref["dF"], ref["S_dF"], C // d_f))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C,d_f", [(8, 2), (256, 64)])
def test_freq_attention_misaligned_rows_take_the_scalar_path_with_the_same_bits(C, d_f, kind):
    """C % 4 == 0 with H, Hw, dHw or dH one float past a 16-byte boundary, each alone and all together: the entry points must
    choose the scalar row loops whenever a pointer they move 16 bytes through is misaligned (H and Hw forward, H and dHw
    backward; dH is always stored float by float), and those loops multiply and add the same values in the same order (the
    bins' chains run over LDS either way)"""
    rng = np.random.default_rng([C, KINDS.index(kind)])
    rows = 9
    H, logits, dHw = _draw(rng, kind, (rows, C)), _draw(rng, kind, (rows, d_f)), _draw(rng, kind, (rows, C))
    F, Hw = _att_fwd(H, logits, d_f)
    for mis in (("H",), ("Hw",), ("H", "Hw")):
        F2, Hw2 = _att_fwd(H, logits, d_f, mis=mis)
        assert _same(F, F2) and _same(Hw, Hw2), mis
    for relu in (0, 1):
        a = _att_bwd(H, F, dHw, d_f, relu)
        for mis in (("H",), ("dHw",), ("dH",), ("H", "dHw", "dH")):
            b = _att_bwd(H, F, dHw, d_f, relu, mis=mis)
            assert _same(a[0], b[0]) and _same(a[1], b[1]), mis


def test_freq_attention_backward_refuses_more_than_4096_channels():
    nv = _nv()
    rows, C = 2, 4097
    H = np.ones((rows, C), np.float32)
    F, Hw = _att_fwd(H, np.zeros((rows, 1), np.float32), 1)             # the forward takes it
    assert (F == 1.0).all() and _same(Hw, H)
    hd, fd = device_copy(H), device_copy(F)
    dl, dH = Guarded((rows, 1)), Guarded((rows, C))
    with pytest.raises(ValueError):
        nv.check(nv.lib.lidbox_freq_attention_bwd(nv.ptr(hd), nv.ptr(fd), nv.ptr(hd), rows, C, 1, 0, dl.ptr, dH.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    assert np.isnan(dl.numpy()).all() and np.isnan(dH.numpy()).all()
