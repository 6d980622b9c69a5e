"""
Every kernel and template instantiation of csrc/conv2d.hip on each side of each dispatch condition and inner branch, against
the float64 numpy oracle (oracle/conv2d_np.py), through the C ABI.

The shapes that select a path sit in one table per group (STRIDE1, WGRAD1, STRIDED_*), each with the condition of conv2d.hip
it is there for; tests/test_oracle_conv2d.py proves on the CPU that every shape selects what its row says.  Every output
lies inside a larger NaN-filled buffer whose words before and after must still be NaN afterwards, every output starts as NaN
(an element that no workgroup writes is not a correct zero), and every workspace has exactly the size the _workspace function
returns and starts as NaN.

How convolution results are judged: element by element against a derived bound.  The kernels' chains are fp32 fused
multiply-adds with one rounding each (v_mfma_f32_16x16x4_f32 and the v_add / v_fma of the epilogues and reduces).  For a sum
of n terms accumulated in ANY order every partial sum carries a relative error of at most u = 2^-24 per addition it went
through, at most n of them, plus one for the bias add; the standard bound (Higham, Accuracy and Stability of Numerical
Algorithms, eq. 3.5 and section 4.2) is then
    |got - ref| <= gamma S + n 2^-126,   gamma = (n + 2) u / (1 - (n + 2) u),   S = sum |terms| of that element,
where the second term covers products or partial sums flushed below the smallest normal number.  S is the oracle's abs_bound
(the same operation on the absolute values) and n the longest chain of the launch:
    forward      K (= k k C_in, or kt kf C_in) + 1 for the bias
    dgrad        k k C_out; strided kt ceil(kf / sf) C_out
    wgrad, db    per + P: a partition's chain of `per` pixels, then the reduce over P partials
Each case runs on two data sets: standard normal, and 1 + 0.1 N(0, 1) for both operands (post-ReLU activations are not
zero-mean, and a sum of same-sign terms is where a lost or doubled term hides least).  On the zero-mean set the relative L2
error must also stay within REL = 1e-5, the limit of test_conv2d_gpu.py / test_conv2d_strided_gpu.py; on the offset set only
the derived bound decides and the relative L2 error is printed.  Everything else is exact.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import conv2d_np as co

pytestmark = pytest.mark.gpu

REL = 1e-5
KINDS = ("normal", "offset")

# ---------------------------------------------------------------------------------------------------- PATHS: stride 1
# (B, T, F, k, C_in, C_out).  M = B T F pixels, K = k k C_in, BN = conv_tile_n(C_out) (forward) / conv_tile_n(C_in) (dgrad)
STRIDE1 = dict(
    # conv_fwd_kernel: `for (kc = 0; kc < g.K; kc += CV_KC)` one trip, `if (kc + CV_KC < g.K) load(...)` never taken (K = 9, 1);
    # M = 1: `rok[j]` false for 127 of 128 rows; every off-centre tap fails `(unsigned)t2 < (unsigned)g.T`
    a3=(1, 1, 1, 3, 1, 16),
    a1=(1, 1, 1, 1, 1, 16),
    # M = 128 = CV_BM exactly, K = 16 = CV_KC exactly, `Cout % 32 == 0` -> conv_fwd_kernel<32>
    b=(2, 8, 8, 1, 16, 32),
    # M = 129: a second row tile of one pixel; K = 153 = 9 * 16 + 9: `kc + kr < g.K` fails in the last chunk with BQ = 2; 96 / 32 =
    # 3 column tiles
    c=(1, 43, 3, 3, 17, 96),
    # `Cout % 16` only -> conv_fwd_kernel<16> with blockIdx.y up to 2, in forward (C_out = 48) and in dgrad (C_in = 48); M = 135 and
    # T F = 45: rows of a tile cross utterances
    d=(3, 5, 9, 5, 48, 48),
    # k = 7 > T = 2 and > F = 3; `Cout % 64 == 0` -> conv_fwd_kernel<64>
    e=(2, 2, 3, 7, 16, 64),
    # K = 27 = 16 + 11: `kc + kr < g.K` fails in the last chunk with BN = 64 (BQ = 4); 3 column tiles
    f=(2, 9, 7, 3, 3, 192),
    # F = 1 / T = 1: ktap()'s `q / g.ks` taps all in the padding on one axis
    g_f1=(1, 300, 1, 3, 32, 16),
    g_t1=(1, 1, 300, 3, 32, 16),
)
# wgrad-only rows: (P, per) = wgrad_plan_kmn(K, M, C_out)
WGRAD1 = dict(
    # M = 15 < CV_KC: one ragged chunk, `m < mhi` fails for pixel 15
    i=(1, 3, 5, 3, 1, 16),
    # P = 7, per = 464; the last partition has 456 = 28 * 16 + 8 pixels (`mc + pr < mhi` fails in its last chunk);
    # `P >= 64` false -> conv_wgrad_reduce_kernel
    j=(3, 40, 27, 3, 3, 48),
    # P = 6: the shape of test_conv2d_wgrad_deterministic, here against the oracle
    k=(4, 33, 21, 5, 16, 32),
    # P = 130 -> conv_wgrad_reduce_wide_kernel: `for (p = lane; p < P; p += 64)` takes up to three trips, P % 64 = 2
    l=(13, 80, 64, 3, 1, 16),
    # tiles = 4 * 4 = 16 -> P = 64, per = 528: 63 * 528 = 33 264 > M = 33 152, partition 63 is empty (`mlo < mhi` false: it
    # stores zeros); conv_wgrad_kernel<64>; 4 K tiles: only `blockIdx.x == 0` accumulates and writes dbpart
    m=(8, 74, 56, 3, 48, 256),
)
# rows whose dW / db are computed twice and must come out bit-identical
WGRAD1_TWICE = ("l", "m")

# ---------------------------------------------------------------------------------------------------- PATHS: strided
# taps = (kt, kf, sf, pt0, pt1, pf0, pf1, time_first)
CLSTM_TAPS = (3, 9, 6, 1, 1, 4, 4, 1)              # clstm's Conv2D at F = 13: "same" pads (4, 4) on frequency, (1, 1) on time
# p: sconv_kernel `blockIdx.x > 0`: B To = 128 (one full tile), 129 (a tile of one row), 300 (three tiles); (C_in, C_out) =
# (16, 32): dgrad <16>, forward <32>;  (48, 96): three column tiles each
STRIDED_P = [(B, T, 13, ci, cout, CLSTM_TAPS) for (B, T) in ((2, 64), (3, 43), (3, 100)) for (ci, cout) in ((16, 32), (48, 96))]
STRIDED = dict(
    # q: Fo = 3 and column 2 starts at f0 = 4 >= F = 3: `nj = max(0, min(g.kf, g.F - f0) - j0)` = 0, `Kv == 0`, no load, no
    # chunk: y[:, :, 2] = bias.  Column 0 has Kv = 2, column 1 Kv = 1 (< CV_KC).  Both orientations of W.
    q_tf=(2, 5, 3, 1, 16, (1, 2, 2, 0, 0, 0, 4, 1)),
    q_ft=(2, 5, 3, 1, 16, (1, 2, 2, 0, 0, 0, 4, 0)),
    # r: sf = 3 > kf = 2: input columns f % 3 == 2 have `mhi = (kf - jf + sf - 1) / sf` = 0, column 9 has `mlo = q0 - Fo + 1` = 1 =
    # mhi: `nj == 0`, dgrad stores exact zeros there
    r=(2, 5, 10, 16, 16, (1, 2, 3, 0, 0, 0, 0, 1)),
)
# s - v: sconv_wgrad_kernel's `live` test.  K = 27 * 64 = 1728: 14 K tiles of two taps each, BN = 16, B To = 512 or 500, Fo = 2,
# P = 2, per = 512
STRIDED_WGRAD = dict(
    # partition 0 = column fo 0, where taps j < 4 read the left padding: tiles 1 - 5 (j <= 3) are skipped, tile 0 holds j = 0 only
    # but is the bias tile and never skips; partition 1 = column 1 skips nothing
    s=(8, 64, 12, 64, 16, (3, 9, 6, 1, 1, 4, 4, 0)),
    # F = 8: in column 1 taps j >= 6 fall past the image: tiles 9 - 13 are skipped on partition 1 (and 1 - 5 on partition 0)
    t=(8, 64, 8, 64, 16, (3, 9, 6, 1, 1, 4, 4, 0)),
    # time_first: tile t holds taps (2 t, 2 t + 1) with j = tap % 9: tile 1 (j = 2, 3) skips on partition 0, tile 2 (j = 4, 5)
    # does not, tile 6 (j = 3, 4) straddles the edge: jmax decides `>= 0`, jmin decides `< F`
    u=(8, 64, 12, 64, 16, (3, 9, 6, 1, 1, 4, 4, 1)),
    # B To = 500 < per = 512: partition 0 reaches 12 pixels into column 1, so nothing may be skipped
    v=(5, 100, 12, 64, 16, (3, 9, 6, 1, 1, 4, 4, 0)),
)

# ---------------------------------------------------------------------------------------------------- PATHS: element-wise
# ew_blocks(): `b < 8192 ? b : 8192` workgroups of 256: above 8192 * 256 = 2 097 152 elements the grid-stride loops take a second trip
BN_RELU = [(4099, 512), (7, 1), (11, 3)]                                  # (R, C): n = 2 098 688 / 7 / 33
# (B, T, F, C, gap): n = B T C = 2 099 200 / 18 / 480; gap = y_batch_stride - T C (NaN-filled)
BN_RELU_MAXF = [(8, 1025, 2, 256, 0), (2, 3, 1, 3, 0), (3, 5, 4, 32, 24)]
POOL = [(1, 2, 2, 1), (2, 3, 2, 5), (2, 65, 33, 24)]
assert BN_RELU[0][0] * BN_RELU[0][1] > co.EW_CAP and 8 * 1025 * 256 > co.EW_CAP
L2_BLOCKS = 128                                                           # l2_penalty_kernel's grid; per = cdiv(total, 128)
L2_LAYOUTS = dict(
    # total = 100 < 128: per = 1, workgroups 100 - 127 own nothing; 16 tensors (L2_MAX), sizes 0, 1 and 5 among them
    tiny=[0, 1, 5, 3, 7, 0, 11, 2, 13, 9, 1, 17, 4, 19, 6, 2],
    # total = 128 * 300 + 7: per = 301, slices straddle tensor boundaries and several tensors fall inside one slice
    straddle=[0, 1, 5, 300, 301, 7000, 2, 12000, 602, 0, 9000, 5000, 3000, 1, 1189, 6],
    # one tensor of 2^21: per = 16 384, 64 strided trips per thread
    big=[1 << 21],
)
assert sum(L2_LAYOUTS["tiny"]) == 100 and sum(L2_LAYOUTS["straddle"]) == 128 * 300 + 7 and len(L2_LAYOUTS["straddle"]) == 16


# ---------------------------------------------------------------------------------------------------- plumbing
def _nv():
    from lidbox_amd import _native as nv
    return nv


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _workspace(nbytes):
    """exactly nbytes, NaN-filled, guarded -> (Guarded or None, pointer, nbytes)"""
    if nbytes == 0:
        return None, None, 0
    assert nbytes % 4 == 0
    g = Guarded((nbytes // 4,))
    return g, g.ptr, nbytes


def _draw(rng, kind, shape):
    z = rng.standard_normal(shape)
    return (z if kind == "normal" else 1.0 + 0.1 * z).astype(np.float32)


def _judge(what, kind, got, ref, S, n):
    """element by element against gamma(n) S + n 2^-126 (module docstring); relative L2 <= REL on the zero-mean set"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = co.error_bound(S, n)
    err = np.abs(got - ref)
    rel = _rel(got, ref)
    finite = np.isfinite(got)
    worst = float((err[finite] / bound[finite]).max()) if finite.any() else float("nan")
    print("%-40s %-6s n=%-6d rel_l2=%.3e  max err/bound=%.3e  non-finite=%d" % (what, kind, n, rel, worst, (~finite).sum()))
    assert finite.all(), "%s: %d elements not written or not finite" % (what, (~finite).sum())
    bad = err > bound
    assert not bad.any(), "%s %s: %d elements over the bound, worst %.3g x at %s" % (
        what, kind, bad.sum(), worst, np.unravel_index(np.argmax(err / bound), err.shape))
    if kind == "normal":
        assert rel <= REL, (what, rel)


# ---------------------------------------------------------------------------------------------------- stride 1: device calls
def _fwd1(x, W, b, relu):
    nv = _nv()
    B, T, F, ci = x.shape
    y = Guarded((B, T, F, W.shape[3]))
    xd, Wd, bd = _dev(x), _dev(W), None if b is None else _dev(b)          # named: the pointers must outlive the launch
    nv.check(nv.lib.lidbox_conv2d_fwd(nv.ptr(xd), B, T, F, ci, nv.ptr(Wd), W.shape[0], W.shape[3], nv.ptr(bd), relu, y.ptr,
                                      nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy()


def _dgrad1(dy, W):
    nv = _nv()
    B, T, F, cout = dy.shape
    k, ci = W.shape[0], W.shape[2]
    dx = Guarded((B, T, F, ci))
    ws, wp, wb = _workspace(nv.lib.lidbox_conv2d_dgrad_workspace(k, ci, cout))
    dyd, Wd = _dev(dy), _dev(W)
    nv.check(nv.lib.lidbox_conv2d_dgrad(nv.ptr(dyd), B, T, F, ci, cout, nv.ptr(Wd), k, dx.ptr, wp, wb, nv.current_stream()))
    torch.cuda.synchronize()
    ws.numpy()
    return dx.numpy()


def _wgrad1(x, dy, k, shape=None, want_db=True):
    """-> (dW, db or None).  `shape` = (B, T, F, C_in, C_out) overrides the arrays' (for B = 0 with placeholder arrays)"""
    nv = _nv()
    B, T, F, ci, cout = shape or (x.shape + dy.shape[3:])
    dW = Guarded((k, k, ci, cout))
    db = Guarded((cout,)) if want_db else None
    ws, wp, wb = _workspace(nv.lib.lidbox_conv2d_wgrad_workspace(B, T, F, ci, cout, k))
    xd, dyd = _dev(x), _dev(dy)
    nv.check(nv.lib.lidbox_conv2d_wgrad(nv.ptr(xd), nv.ptr(dyd), B, T, F, ci, cout, k, dW.ptr, db.ptr if db else None, wp, wb,
                                        nv.current_stream()))
    torch.cuda.synchronize()
    if ws is not None:
        ws.numpy()
    return dW.numpy(), db.numpy() if db else None


@functools.lru_cache(maxsize=None)
def _case1(shape, kind):
    B, T, F, k, ci, cout = shape
    rng = np.random.default_rng([B, T, F, k, ci, cout, KINDS.index(kind)])
    return (_draw(rng, kind, (B, T, F, ci)), _draw(rng, kind, (k, k, ci, cout)), _draw(rng, kind, (cout,)),
            _draw(rng, kind, (B, T, F, cout)))


# ---------------------------------------------------------------------------------------------------- stride 1: tests
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", sorted(STRIDE1))
def test_stride1_forward(row, kind):
    """rows a - g: relu(conv + bias) into a NaN-filled y"""
    shape = STRIDE1[row]
    x, W, b, _ = _case1(shape, kind)
    k, ci = shape[3], shape[4]
    y = _fwd1(x, W, b, 1)
    _judge("fwd1[%s]" % row, kind, y, co.fwd(x, W, b, k, relu=True), co.abs_bound_fwd(x, W, b, k), k * k * ci + 1)


@pytest.mark.parametrize("kind", KINDS)
def test_stride1_forward_without_relu_and_bias(kind):
    """row h = row d with `relu = 0` and `bias = NULL`: `if (relu) v = fmaxf(v, 0.0f)` and `bias ? bias[n] : 0.0f`"""
    shape = STRIDE1["d"]
    x, W, _, _ = _case1(shape, kind)
    k, ci = shape[3], shape[4]
    ref = co.fwd(x, W, None, k)
    if kind == "normal":
        assert (ref < -1.0).sum() > ref.size // 4             # the zero-mean reference has outputs a ReLU would have cut
    _judge("fwd1[h] no relu, no bias", kind, _fwd1(x, W, None, 0), ref, co.abs_bound_fwd(x, W, None, k), k * k * ci)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", [r for r in sorted(STRIDE1) if STRIDE1[r][4] % 16 == 0])
def test_stride1_dgrad(row, kind):
    """rows b, d, e, g: conv_rot_kernel + conv_fwd_kernel<conv_tile_n(C_in)> with K = k k C_out"""
    shape = STRIDE1[row]
    B, T, F, k, ci, cout = shape
    _, W, _, dy = _case1(shape, kind)
    _judge("dgrad1[%s]" % row, kind, _dgrad1(dy, W), co.dgrad(dy, W, k, T, F), co.abs_bound_dgrad(dy, W, k, T, F), k * k * cout)


def _check_wgrad1(row, shape, kind, twice):
    B, T, F, k, ci, cout = shape
    x, _, _, dy = _case1(shape, kind)
    P, per = co.wgrad_plan(k * k * ci, B * T * F, cout)
    dW, db = _wgrad1(x, dy, k)
    _judge("wgrad1[%s] dW P=%d per=%d" % (row, P, per), kind, dW, co.wgrad(x, dy, k), co.abs_bound_wgrad(x, dy, k), per + P)
    _judge("wgrad1[%s] db" % row, kind, db, co.bias_grad(dy), co.abs_bound_bias_grad(dy), per + P)
    if twice:
        dW2, db2 = _wgrad1(x, dy, k)
        assert np.array_equal(dW.view(np.int32), dW2.view(np.int32)) and np.array_equal(db.view(np.int32), db2.view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", sorted(STRIDE1) + sorted(WGRAD1))
def test_stride1_wgrad_and_bias_grad(row, kind):
    """rows a - g and i - m: dW and db element by element; rows l and m twice with identical bits"""
    _check_wgrad1(row, STRIDE1.get(row) or WGRAD1[row], kind, row in WGRAD1_TWICE)


def test_stride1_wgrad_without_bias_grad():
    """row n = row j with `db = NULL`: `nout = nw + (db ? C_out : 0)`; dW has the bits of the run with db, and the words after
    dW (where a reduce that ignored the NULL would store db) stay untouched -- Guarded.numpy() checks them"""
    shape = WGRAD1["j"]
    x, _, _, dy = _case1(shape, "normal")
    with_db, _ = _wgrad1(x, dy, shape[3])
    without, none = _wgrad1(x, dy, shape[3], want_db=False)
    assert none is None and np.array_equal(with_db.view(np.int32), without.view(np.int32))


def test_stride1_empty_batch():
    """row o, B = 0: forward and dgrad return without a launch, wgrad stores exact zeros (`hipMemsetAsync`), with and without db"""
    nv = _nv()
    T, F, k, ci, cout = 5, 4, 3, 16, 32
    some = np.ones(16, np.float32)
    for want_db in (True, False):
        dW, db = _wgrad1(some, some, k, shape=(0, T, F, ci, cout), want_db=want_db)
        assert dW.shape == (k, k, ci, cout) and not dW.view(np.int32).any()
        assert db is None or (db.shape == (cout,) and not db.view(np.int32).any())
    y = Guarded((16,))
    d = _dev(some)
    nv.check(nv.lib.lidbox_conv2d_fwd(nv.ptr(d), 0, T, F, ci, nv.ptr(d), k, cout, nv.ptr(d), 1, y.ptr, nv.current_stream()))
    nv.check(nv.lib.lidbox_conv2d_dgrad(nv.ptr(d), 0, T, F, ci, cout, nv.ptr(d), k, y.ptr, None, 0, nv.current_stream()))
    torch.cuda.synchronize()
    assert np.isnan(y.numpy()).all()


# ---------------------------------------------------------------------------------------------------- strided: device calls
def _taps(t):
    return _nv().Conv2DTaps(*t)


def _sfwd(x, W, b, taps):
    nv = _nv()
    B, T, F, ci = x.shape
    To, Fo = co.out_size(T, F, taps)
    y = Guarded((B, To, Fo, W.shape[3]))
    xd, Wd, bd = _dev(x), _dev(W), None if b is None else _dev(b)
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(xd), B, T, F, ci, nv.ptr(Wd), _taps(taps), W.shape[3], nv.ptr(bd), y.ptr,
                                              nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy()


def _sdgrad(dy, W, taps, T, F):
    nv = _nv()
    B, ci, cout = dy.shape[0], W.shape[2], W.shape[3]
    dx = Guarded((B, T, F, ci))
    ws, wp, wb = _workspace(nv.lib.lidbox_conv2d_strided_dgrad_workspace(_taps(taps), ci, cout))
    dyd, Wd = _dev(dy), _dev(W)
    nv.check(nv.lib.lidbox_conv2d_strided_dgrad(nv.ptr(dyd), B, T, F, ci, cout, nv.ptr(Wd), _taps(taps), dx.ptr, wp, wb,
                                                nv.current_stream()))
    torch.cuda.synchronize()
    ws.numpy()
    return dx.numpy()


def _swgrad(x, dy, taps, shape=None, want_db=True):
    nv = _nv()
    B, T, F, ci, cout = shape or (x.shape + dy.shape[3:])
    t = co.as_taps(taps)
    dW = Guarded((t.kt, t.kf, ci, cout) if t.time_first else (t.kf, t.kt, ci, cout))
    db = Guarded((cout,)) if want_db else None
    ws, wp, wb = _workspace(nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, F, ci, cout, _taps(taps)))
    xd, dyd = _dev(x), _dev(dy)
    nv.check(nv.lib.lidbox_conv2d_strided_wgrad(nv.ptr(xd), nv.ptr(dyd), B, T, F, ci, cout, _taps(taps), dW.ptr,
                                                db.ptr if db else None, wp, wb, nv.current_stream()))
    torch.cuda.synchronize()
    if ws is not None:
        ws.numpy()
    return dW.numpy(), db.numpy() if db else None


@functools.lru_cache(maxsize=None)
def _scase(shape, kind):
    B, T, F, ci, cout, taps = shape
    t = co.as_taps(taps)
    To, Fo = co.out_size(T, F, t)
    rng = np.random.default_rng([B, T, F, ci, cout, KINDS.index(kind)] + list(taps))
    wshape = (t.kt, t.kf, ci, cout) if t.time_first else (t.kf, t.kt, ci, cout)
    return _draw(rng, kind, (B, T, F, ci)), _draw(rng, kind, wshape), _draw(rng, kind, (cout,)), _draw(rng, kind, (B, To, Fo, cout))


def _check_strided(name, shape, kind):
    """forward, dgrad (C_in % 16 == 0) and wgrad of one strided shape -> (y, dx or None, dW, db)"""
    B, T, F, ci, cout, taps = shape
    t = co.as_taps(taps)
    x, W, b, dy = _scase(shape, kind)
    y = _sfwd(x, W, b, taps)
    _judge("sfwd[%s]" % name, kind, y, co.fwd(x, W, b, t), co.abs_bound_fwd(x, W, b, t), t.kt * t.kf * ci + 1)
    dx = None
    if ci % 16 == 0:
        dx = _sdgrad(dy, W, taps, T, F)
        _judge("sdgrad[%s]" % name, kind, dx, co.dgrad(dy, W, t, T, F), co.abs_bound_dgrad(dy, W, t, T, F),
               t.kt * co.cdiv(t.kf, t.sf) * cout)
    To, Fo = co.out_size(T, F, t)
    P, per = co.wgrad_plan(t.kt * t.kf * ci, B * To * Fo, cout)
    dW, db = _swgrad(x, dy, taps)
    _judge("swgrad[%s] dW P=%d per=%d" % (name, P, per), kind, dW, co.wgrad(x, dy, t), co.abs_bound_wgrad(x, dy, t), per + P)
    _judge("swgrad[%s] db" % name, kind, db, co.bias_grad(dy), co.abs_bound_bias_grad(dy), per + P)
    return y, dx, dW, db


# ---------------------------------------------------------------------------------------------------- strided: tests
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", STRIDED_P, ids=lambda s: "B%dxT%d-%dto%d" % (s[0], s[1], s[3], s[4]))
def test_strided_more_than_one_row_tile(shape, kind):
    """row p: forward, dgrad and wgrad with B To = 128, 129 and 300"""
    _check_strided("p %s" % (shape[:5],), shape, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", ["q_tf", "q_ft"])
def test_strided_forward_column_without_a_tap_is_the_bias(row, kind):
    """row q: `Kv == 0` -- the column's outputs are bias[co], bit for bit, written into a NaN-filled y"""
    shape = STRIDED[row]
    y = _check_strided(row, shape, kind)[0]
    b = _scase(shape, kind)[2]
    assert y.shape[2] == 3
    assert np.array_equal(y[:, :, 2].view(np.int32), np.broadcast_to(b, y[:, :, 2].shape).view(np.int32))


@pytest.mark.parametrize("kind", KINDS)
def test_strided_dgrad_columns_no_tap_reaches_are_zero(kind):
    """row r: `sf > kf` -- dgrad stores exact zeros into input columns f % 3 == 2 and f = 9 of a NaN-filled dx"""
    dx = _check_strided("r", STRIDED["r"], kind)[1]
    for f in (2, 5, 8, 9):
        assert not dx[:, :, f].view(np.int32).any(), f
    assert all(dx[:, :, f].all() for f in (0, 1, 3, 4, 6, 7))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("row", sorted(STRIDED_WGRAD))
def test_strided_wgrad_skipped_tiles(row, kind):
    """rows s - v: dW element by element where sconv_wgrad_kernel's `live` test skips (tile, partition) pairs, and where it
    must not; the rows of the bias tile (kidx < 128), which never skips although its taps read padding, are finite"""
    shape = STRIDED_WGRAD[row]
    dW = _check_strided(row, shape, kind)[2]
    assert np.isfinite(dW.reshape(-1, shape[4])[:co.CV_BM]).all()


def test_strided_empty_batch_and_no_bias_grad():
    """row w: B = 0 -> exact zeros in dW and db, y untouched; `db = NULL` -> dW with the bits of the run with db"""
    nv = _nv()
    some = np.ones(16, np.float32)
    T, F, ci, cout = 6, 13, 16, 32
    for want_db in (True, False):
        dW, db = _swgrad(some, some, CLSTM_TAPS, shape=(0, T, F, ci, cout), want_db=want_db)
        assert dW.shape == (3, 9, ci, cout) and not dW.view(np.int32).any()
        assert db is None or (db.shape == (cout,) and not db.view(np.int32).any())
    y = Guarded((16,))
    d = _dev(some)
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(d), 0, T, F, ci, nv.ptr(d), _taps(CLSTM_TAPS), cout, nv.ptr(d), y.ptr,
                                              nv.current_stream()))
    nv.check(nv.lib.lidbox_conv2d_strided_dgrad(nv.ptr(d), 0, T, F, ci, cout, nv.ptr(d), _taps(CLSTM_TAPS), y.ptr, None, 0,
                                                nv.current_stream()))
    torch.cuda.synchronize()
    assert np.isnan(y.numpy()).all()
    shape = STRIDED_P[2]                                       # B To = 129: P = 1
    x, _, _, dy = _scase(shape, "normal")
    with_db, _ = _swgrad(x, dy, shape[5])
    without, none = _swgrad(x, dy, shape[5], want_db=False)
    assert none is None and np.array_equal(with_db.view(np.int32), without.view(np.int32))


# ---------------------------------------------------------------------------------------------------- BN-apply + ReLU (+ max over F)
def _bn_params(rng, C):
    scale = rng.standard_normal(C).astype(np.float32)         # gamma / sqrt(var + eps) of either sign
    shift = (0.5 * rng.standard_normal(C)).astype(np.float32)
    return scale, shift


@pytest.mark.parametrize("R,C", BN_RELU)
def test_bn_relu_forward_backward_exact(R, C):
    """bn_relu_fwd_kernel / bn_relu_bwd_kernel: y = max(fma(x, sc, sh), 0) and dx = where(fma(x, sc, sh) > 0, dy, 0), bit for
    bit; backward out of place and in place (`dx == dy`).  (4099, 512) forces the second grid-stride trip."""
    nv = _nv()
    st = nv.current_stream()
    rng = np.random.default_rng(R + C)
    x = rng.standard_normal((R, C)).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    scale, shift = _bn_params(rng, C)
    xd, sd, hd, dyd = (_dev(a) for a in (x, scale, shift, dy))
    y, dx, inplace = Guarded((R, C)), Guarded((R, C)), Guarded((R, C), init=dyd)
    nv.check(nv.lib.lidbox_bn_relu_fwd(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), y.ptr, st))
    nv.check(nv.lib.lidbox_bn_relu_bwd(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), nv.ptr(dyd), dx.ptr, st))
    nv.check(nv.lib.lidbox_bn_relu_bwd(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), inplace.ptr, inplace.ptr, st))
    torch.cuda.synchronize()
    want_y, want_dx = co.bn_relu(x, scale, shift), co.bn_relu_grad(x, scale, shift, dy)
    assert 0.2 < (want_y > 0).mean() < 0.8 or R * C < 64
    assert np.array_equal(y.numpy(), want_y)
    assert np.array_equal(dx.numpy(), want_dx)
    assert np.array_equal(inplace.numpy(), want_dx)
    assert np.array_equal(dyd.cpu().numpy(), dy)


@pytest.mark.parametrize("B,T,F,C,gap", BN_RELU_MAXF)
def test_bn_relu_maxf_forward_backward_exact(B, T, F, C, gap):
    """bn_relu_maxf_fwd_kernel / bn_relu_maxf_bwd_kernel: exact maximum, dy split evenly over ties ((1.0f / count) * dy in
    fp32), nothing for ties at zero; batch strides larger than T C with NaN in the gaps, which must survive and must not
    be read.  Planted: a two-way tie (F >= 2), a three-way tie (F >= 3) and an all-negative column, in the first and in the
    last (b, t) row -- at the large shape the last row belongs to the second grid-stride trip."""
    nv = _nv()
    st = nv.current_stream()
    rng = np.random.default_rng(B * T + F + C)
    x = rng.standard_normal((B, T, F, C)).astype(np.float32)
    scale, shift = _bn_params(rng, C)
    scale[:3], shift[:3] = 1.0, 0.0
    for (b, t) in ((0, 0), (B - 1, T - 1)):
        x[b, t, :, 0] = -2.0
        x[b, t, 0, 0] = x[b, t, F - 1, 0] = 3.0                # two-way positive tie (F = 1: a plain maximum)
        x[b, t, :, 1] = -1.0                                   # every relu output 0: a tie at zero gets nothing
        if F >= 3:
            x[b, t, :, 2] = -2.0
            x[b, t, 0, 2] = x[b, t, 2, 2] = x[b, t, F - 1, 2] = 5.0
    dy = rng.standard_normal((B, T, C)).astype(np.float32)
    stride = T * C + gap
    dy_rows = np.full((B, stride), np.nan, np.float32)
    dy_rows[:, :T * C] = dy.reshape(B, T * C)
    xd, sd, hd, dyd = (_dev(a) for a in (x, scale, shift, dy_rows))
    y, dx = Guarded((B, stride)), Guarded((B, T, F, C))
    nv.check(nv.lib.lidbox_bn_relu_maxf_fwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), y.ptr, stride, st))
    nv.check(nv.lib.lidbox_bn_relu_maxf_bwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), nv.ptr(dyd), stride, dx.ptr, st))
    torch.cuda.synchronize()
    got_y, got_dx = y.numpy(), dx.numpy()
    assert np.array_equal(got_y[:, :T * C].reshape(B, T, C), co.bn_relu_maxf(x, scale, shift))
    assert np.isnan(got_y[:, T * C:]).all()
    ref_dx, cnt = co.bn_relu_maxf_grad(x, scale, shift, dy)
    want = np.where(ref_dx != 0, ((np.float32(1) / cnt.astype(np.float32)) * dy)[:, :, None, :], np.float32(0)).astype(np.float32)
    assert np.array_equal(got_dx, want)
    assert np.abs(got_dx - ref_dx).max() <= 2 * co.U * np.abs(ref_dx).max()
    for (b, t) in ((0, 0), (B - 1, T - 1)):
        if F >= 2:
            assert cnt[b, t, 0] == 2 and got_dx[b, t, 0, 0] == got_dx[b, t, F - 1, 0] == np.float32(0.5) * dy[b, t, 0]
        assert cnt[b, t, 1] == F and not got_dx[b, t, :, 1].any()
        if F >= 3:
            n3 = len({0, 2, F - 1})
            assert cnt[b, t, 2] == n3 and got_dx[b, t, 0, 2] == np.float32(1.0) / np.float32(n3) * dy[b, t, 2] and got_dx[b, t, 1, 2] == 0


# ---------------------------------------------------------------------------------------------------- BN-apply + MaxPool2D
@pytest.mark.parametrize("B,T,F,C", POOL)
def test_bn_maxpool_forward_backward_exact(B, T, F, C):
    """bn_maxpool_fwd_kernel / maxpool_bwd_kernel on distinct integers (exact in fp32 after the scale): a single window with
    C = 1, odd T (a dropped frame), and more than one workgroup with odd T and F"""
    nv = _nv()
    st = nv.current_stream()
    rng = np.random.default_rng(B + T + F + C)
    n = B * T * F * C
    x = (rng.permutation(n) - n // 2).astype(np.float32).reshape(B, T, F, C)
    scale = rng.choice(np.array([1.0, -1.0, 2.0, -0.5], np.float32), C)
    shift = rng.integers(-3, 4, C).astype(np.float32)
    dp = rng.integers(-99, 100, (B, T // 2, F // 2, C)).astype(np.float32)
    want_y, want_code = co.bn_maxpool2d(x, scale, shift)
    y, code, dx = Guarded(want_y.shape), Guarded(want_y.shape, torch.uint8), Guarded((B, T, F, C))
    xd, sd, hd, dpd = (_dev(a) for a in (x, scale, shift, dp))
    nv.check(nv.lib.lidbox_bn_maxpool2d_fwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), y.ptr, code.ptr, st))
    nv.check(nv.lib.lidbox_maxpool2d_bwd(nv.ptr(dpd), code.ptr, B, T, F, C, dx.ptr, st))
    torch.cuda.synchronize()
    assert np.array_equal(y.numpy(), want_y.astype(np.float32))
    assert np.array_equal(code.numpy(), want_code)
    got_dx = dx.numpy()
    assert np.array_equal(got_dx, co.maxpool2d_grad(dp, want_code, T, F))
    assert (got_dx != 0).sum() == (dp != 0).sum()
    if T % 2:
        assert not got_dx[:, -1].any()
    if F % 2:
        assert not got_dx[:, :, -1].any()


# ---------------------------------------------------------------------------------------------------- L2 penalty
def _l2_layout(sizes, rng):
    """non-adjacent tensors (gaps of 1 - 4 words) of small integers, so that every product and every sum below is exact in
    fp32 in any order; NaN in the gaps of params and grads"""
    offs, pos = [], 3
    for n in sizes:
        offs.append(pos)
        pos += n + 1 + len(offs) % 4
    params = np.full(pos + 5, np.nan, np.float32)
    grads = np.full(pos + 5, np.nan, np.float32)
    hi = 2 if max(sizes) > 100000 else 4
    for o, n in zip(offs, sizes):
        params[o:o + n] = rng.integers(-hi + 1, hi, n)
        grads[o:o + n] = rng.integers(-8, 9, n)
    lams = [(1.0, 0.5, 0.25)[i % 3] for i in range(len(sizes))]
    return offs, params, grads, lams


def _l2_call(params, grads, offs, sizes, lams, gscale, loss, ws):
    nv = _nv()
    n = len(offs)
    arr = lambda ty, v: (ty * max(n, 1))(*v) if n else None                      # noqa: E731
    nv.check(nv.lib.lidbox_l2_penalty(nv.ptr(params), None if grads is None else grads.ptr, n, arr(ctypes.c_long, offs),
                                      arr(ctypes.c_long, sizes), arr(ctypes.c_float, lams), gscale, None if loss is None else loss.ptr,
                                      None if ws is None else ws.ptr, 0 if ws is None else ws.n * 4, nv.current_stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["both", "grads_only", "loss_only"])
@pytest.mark.parametrize("layout", sorted(L2_LAYOUTS))
def test_l2_penalty_layouts_exact(layout, mode):
    """l2_penalty_kernel / l2_loss_kernel: `lo = max(blo, base), hi = min(bhi, base + a.n[t])` over 16 tensors laid end to end.
    Integer data and power-of-two lambdas: loss and gradients are exact, whatever the order.  `loss = NULL`: no workspace, no
    l2_loss_kernel; `grads = NULL`: `if (g)` false."""
    nv = _nv()
    sizes = L2_LAYOUTS[layout]
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    offs, params, grads, lams = _l2_layout(sizes, rng)
    want_g, want_l = co.l2_penalty(params, grads, offs, sizes, lams, 0.5, loss0=0.75)
    assert want_l * 4 == int(want_l * 4) and want_l * 4 < 2 ** 24                # every partial sum is exact in fp32
    pd = _dev(params)
    gd = Guarded(grads.shape, init=_dev(grads)) if mode != "loss_only" else None
    loss = Guarded((1,), init=torch.tensor([0.75], device="cuda")) if mode != "grads_only" else None
    ws = Guarded((nv.lib.lidbox_l2_penalty_workspace() // 4,)) if loss is not None else None
    assert ws is None or ws.n == L2_BLOCKS
    _l2_call(pd, gd, offs, sizes, lams, 0.5, loss, ws)
    if gd is not None:
        got = gd.numpy()
        inside = ~np.isnan(want_g)
        assert inside.sum() == sum(sizes) and np.isnan(got[~inside]).all()
        assert np.array_equal(got[inside], want_g[inside].astype(np.float32))
    if loss is not None:
        assert float(loss.numpy()[0]) == want_l
        ws.numpy()


def test_l2_penalty_count_zero_touches_nothing():
    nv = _nv()
    pd = _dev(np.ones(8, np.float32))
    gd, loss, ws = Guarded((8,)), Guarded((1,)), Guarded((nv.lib.lidbox_l2_penalty_workspace() // 4,))
    _l2_call(pd, gd, [], [], [], 1.0, loss, ws)
    assert np.isnan(gd.numpy()).all() and np.isnan(loss.numpy()).all() and np.isnan(ws.numpy()).all()
