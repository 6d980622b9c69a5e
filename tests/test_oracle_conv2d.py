"""
Pins oracle/conv2d_np.py on the CPU, three ways:
  1. its convolutions (a loop over taps, no library convolution) against float64 torch.nn.functional.conv2d + autograd with an
     asymmetric F.pad, both kernel orientations; its pooling / max / fma forms against torch and exact rational arithmetic;
  2. its restatement of the wgrad partition plan against the library's own host functions lidbox_conv2d_wgrad_workspace /
     lidbox_conv2d_strided_wgrad_workspace (bytes = P (K C_out + C_out) 4), which need no GPU;
  3. for every row of the PATHS tables of tests/test_conv2d_paths_gpu.py, the property the row is there for, computed from
     the oracle's restatement of the conditions in conv2d.hip: a shape that stops selecting its path fails here.
"""
import fractions

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import test_conv2d_paths_gpu as paths
from oracle import conv2d_np as co


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native


# ---------------------------------------------------------------------------------------------------- 1. the oracle itself
def _torch_all(x, W, b, dy, t):
    """float64 torch: y, dx, dW, db of sum(conv(x) * dy) on the image [B, C, T, F] after an explicit pad"""
    xt, Wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, W, b))
    Wk = Wt.permute(3, 2, 0, 1) if t.time_first else Wt.permute(3, 2, 1, 0)          # [Co, Ci, kt, kf]
    xi = Fn.pad(xt.permute(0, 3, 1, 2), (t.pf0, t.pf1, t.pt0, t.pt1))
    y = Fn.conv2d(xi, Wk, bt, stride=(1, t.sf)).permute(0, 2, 3, 1)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), xt.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()


ORACLE_CASES = [(2, 5, 7, 3, 4, 3), (1, 2, 3, 2, 3, 7), (2, 4, 4, 1, 2, 1), (3, 6, 1, 2, 2, 5)] + [
    (2, 7, 13, 3, 4, (3, 9, 6, 1, 1, 4, 4, 1)), (2, 7, 13, 3, 4, (3, 9, 6, 1, 1, 4, 4, 0)), (3, 9, 17, 2, 5, (5, 3, 2, 2, 1, 0, 2, 0)),
    (2, 6, 11, 3, 2, (3, 9, 6, 0, 2, 3, 5, 1)), (2, 5, 3, 1, 2, (1, 2, 2, 0, 0, 0, 4, 1)), (2, 5, 10, 2, 3, (1, 2, 3, 0, 0, 0, 0, 0)),
    (1, 4, 12, 2, 2, (1, 4, 3, 0, 0, 1, 0, 0))]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=str)
def test_oracle_matches_torch_conv2d_and_autograd(case):
    B, T, F, ci, cout, k = case
    t = co.as_taps(k)
    rng = np.random.default_rng([B, T, F, ci, cout] + list(t))
    To, Fo = co.out_size(T, F, t)
    x = rng.standard_normal((B, T, F, ci))
    W = rng.standard_normal((t.kt, t.kf, ci, cout) if t.time_first else (t.kf, t.kt, ci, cout))
    b = rng.standard_normal(cout)
    dy = rng.standard_normal((B, To, Fo, cout))
    y, dx, dW, db = _torch_all(x, W, b, dy, t)
    assert y.shape == (B, To, Fo, cout)
    for got, want in ((co.fwd(x, W, b, k), y), (co.dgrad(dy, W, k, T, F), dx), (co.wgrad(x, dy, k), dW), (co.bias_grad(dy), db),
                      (co.fwd(x, W, b, k, relu=True), np.maximum(y, 0)), (co.fwd(x, W, None, k), y - b)):
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # abs_bound is the same operation on absolute values: it dominates the result and equals it for non-negative operands
    assert (co.abs_bound_fwd(x, W, b, k) >= np.abs(y) - 1e-12).all()
    assert (co.abs_bound_dgrad(dy, W, k, T, F) >= np.abs(dx) - 1e-12).all()
    assert (co.abs_bound_wgrad(x, dy, k) >= np.abs(dW) - 1e-12).all()
    assert (co.abs_bound_bias_grad(dy) >= np.abs(db) - 1e-12).all()
    assert np.array_equal(co.abs_bound_wgrad(np.abs(x), np.abs(dy), k), co.wgrad(np.abs(x), np.abs(dy), k))


def test_stride1_is_the_strided_form_in_keras_layout():
    """k (int) means W[kh][kw] with kh over frequency: taps (k, k, 1, p, p, p, p, time_first = 0)"""
    assert co.as_taps(5) == co.Taps(5, 5, 1, 2, 2, 2, 2, 0) and co.out_size(9, 4, 5) == (9, 4)
    x = np.zeros((1, 4, 5, 1))
    x[0, 1, 2, 0] = 1.0
    W = np.zeros((3, 3, 1, 1))
    W[2, 1, 0, 0] = 1.0                      # kh = 2: reads frequency + 1, kw = 1: the same frame
    y = co.fwd(x, W, None, 3)
    assert y[0, 1, 1, 0] == 1.0 and y.sum() == 1.0


def test_error_bound_formula():
    n = 1000
    g = (n + 2) * 2.0 ** -24 / (1 - (n + 2) * 2.0 ** -24)
    assert co.gamma(n) == g and np.array_equal(co.error_bound(np.array([0.0, 2.0]), n), [n * 2.0 ** -126, 2 * g + n * 2.0 ** -126])


def test_fma32_is_one_rounding():
    rng = np.random.default_rng(0)
    x, a, b = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    # the product 1 + 2^-11 + 2^-24 is an fp32 midpoint and the addend vanishes in float64: rounding the float64 sum again would
    # go to even (down) in both cases, one rounding goes up in the first
    x[0], a[0], b[0] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -80)
    x[1], a[1], b[1] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-2.0 ** -80)
    got = co.fma32(x, a, b)
    assert got[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and got[1] == np.float32(1 + 2.0 ** -11)
    for i in range(len(x)):
        exact = fractions.Fraction(float(x[i])) * fractions.Fraction(float(a[i])) + fractions.Fraction(float(b[i]))
        r = float(got[i])
        for other in (float(np.nextafter(got[i], np.float32(np.inf))), float(np.nextafter(got[i], np.float32(-np.inf)))):
            assert abs(exact - fractions.Fraction(r)) <= abs(exact - fractions.Fraction(other)), i
    assert np.array_equal(co.bn_relu(x, a, b), np.maximum(got, 0))
    dy = rng.standard_normal(2000).astype(np.float32)
    assert np.array_equal(co.bn_relu_grad(x, a, b, dy), np.where(got > 0, dy, 0))


def test_maxf_and_pool_forms_match_torch():
    rng = np.random.default_rng(1)
    B, T, F, C = 2, 7, 5, 4
    x = rng.integers(-3, 4, (B, T, F, C)).astype(np.float32)              # many ties, many zeros
    scale = np.array([1.0, -1.0, 2.0, -0.5], np.float32)
    shift = np.array([0.0, 1.0, -2.0, 0.0], np.float32)
    dy = rng.standard_normal((B, T, C))
    vt = torch.from_numpy(x.astype(np.float64) * scale + shift).requires_grad_(True)
    yt = torch.relu(vt).amax(dim=2)                                        # amax splits the gradient evenly over ties
    yt.backward(torch.from_numpy(dy))
    assert np.array_equal(co.bn_relu_maxf(x, scale, shift), yt.detach().numpy().astype(np.float32))
    dx, cnt = co.bn_relu_maxf_grad(x, scale, shift, dy)
    assert np.abs(dx - vt.grad.numpy()).max() <= 1e-15 and cnt.min() >= 1 and cnt.max() > 1
    # 2 x 2 pool: torch's image is [B, C, F, T] (height = frequency); its first maximum scans frequency rows, then time
    v = torch.from_numpy(x.astype(np.float64) * scale + shift).permute(0, 3, 2, 1).contiguous().requires_grad_(True)
    y, idx = Fn.max_pool2d(v, 2, return_indices=True)
    dp = rng.standard_normal((B, T // 2, F // 2, C))
    (y * torch.from_numpy(dp).permute(0, 3, 2, 1)).sum().backward()
    code_t = (2 * ((idx // T) % 2) + (idx % T) % 2).permute(0, 3, 2, 1).numpy()
    got_y, got_code = co.bn_maxpool2d(x, scale, shift)
    assert np.array_equal(got_y, y.permute(0, 3, 2, 1).detach().numpy()) and np.array_equal(got_code, code_t)
    assert len(np.unique(got_code)) == 4
    assert np.array_equal(co.maxpool2d_grad(dp, got_code, T, F), v.grad.permute(0, 3, 2, 1).numpy())


def test_l2_penalty_form():
    p = np.array([9.0, 1.0, 2.0, 9.0, 3.0])
    g, loss = co.l2_penalty(p, np.zeros(5), [1, 4], [2, 1], [0.5, 0.25], 0.5, loss0=1.0)
    assert np.array_equal(g, [0, 0.5, 1.0, 0, 0.75]) and loss == 1.0 + 0.5 * 5 + 0.25 * 9


# ---------------------------------------------------------------------------------------------------- 2. the plan, against the library
def test_wgrad_plan_matches_the_library(nv):
    shapes = list(paths.STRIDE1.values()) + list(paths.WGRAD1.values()) + [(16, 48, 48, 7, 1, 16), (1, 1, 1, 1, 1, 1024), (64, 198, 40, 3, 64, 128)]
    for (B, T, F, k, ci, cout) in shapes:
        want = co.wgrad_workspace_bytes(k * k * ci, B * T * F, cout)
        assert nv.lib.lidbox_conv2d_wgrad_workspace(B, T, F, ci, cout, k) == want, (B, T, F, k, ci, cout)
        P, per = co.wgrad_plan(k * k * ci, B * T * F, cout)
        assert 1 <= P <= 1024 and per % co.CV_KC == 0 and P * per >= B * T * F
    strided = paths.STRIDED_P + list(paths.STRIDED.values()) + list(paths.STRIDED_WGRAD.values()) + [(64, 198, 40, 128, 256, (3, 9, 6, 1, 1, 1, 2, 1))]
    for (B, T, F, ci, cout, taps) in strided:
        t = co.as_taps(taps)
        To, Fo = co.out_size(T, F, t)
        want = co.wgrad_workspace_bytes(t.kt * t.kf * ci, B * To * Fo, cout)
        assert nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, F, ci, cout, nv.Conv2DTaps(*taps)) == want, (B, T, F, ci, cout, taps)
    assert nv.lib.lidbox_conv2d_wgrad_workspace(0, 5, 4, 16, 32, 3) == 0
    assert nv.lib.lidbox_l2_penalty_workspace() == paths.L2_BLOCKS * 4


# ---------------------------------------------------------------------------------------------------- 3. what every PATHS row selects
def _mk(shape):
    B, T, F, k, ci, cout = shape
    return B * T * F, k * k * ci


def test_stride1_rows_select_their_paths():
    S = paths.STRIDE1
    assert _mk(S["a3"]) == (1, 9) and _mk(S["a1"]) == (1, 1)                        # a: M = 1, K < one chunk
    assert _mk(S["b"]) == (co.CV_BM, co.CV_KC) and co.conv_tile_n(S["b"][5]) == 32     # b
    M, K = _mk(S["c"])                                                              # c
    assert (M, K, K % co.CV_KC) == (129, 153, 9) and co.conv_tile_n(96) == 32 and 96 // 32 == 3
    B, T, F, k, ci, cout = S["d"]                                                   # d
    assert co.conv_tile_n(cout) == 16 == co.conv_tile_n(ci) and cout // 16 == 3 and ci // 16 == 3 and T * F < co.CV_BM < B * T * F
    B, T, F, k, ci, cout = S["e"]                                                   # e
    assert k > T and k > F and co.conv_tile_n(cout) == 64
    M, K = _mk(S["f"])                                                              # f
    assert (K, K % co.CV_KC) == (27, 11) and co.conv_tile_n(S["f"][5]) == 64 and S["f"][5] // 64 == 3
    assert S["g_f1"][2] == 1 and S["g_t1"][1] == 1 and S["g_f1"][1] == S["g_t1"][2] == 300      # g
    tiles_n = set()
    for name, (B, T, F, k, ci, cout) in S.items():
        assert k % 2 == 1 and cout % 16 == 0
        assert co.wgrad_plan(k * k * ci, B * T * F, cout)[0] == 1, name              # none of these splits the pixels
        tiles_n.add(co.conv_tile_n(cout))
        if ci % 16 == 0:
            tiles_n.add(("dgrad", co.conv_tile_n(ci)))
    assert tiles_n == {16, 32, 64, ("dgrad", 16), ("dgrad", 32)}
    # contraction tails meet every B-operand loader: BQ = BN / 16 = 1, 2, 4
    tails = {co.conv_tile_n(s[5]) for s in S.values() if (s[3] * s[3] * s[4]) % co.CV_KC}
    assert tails == {16, 32, 64}


def test_stride1_wgrad_rows_select_their_plans():
    W = paths.WGRAD1
    plan = {r: co.wgrad_plan(s[3] * s[3] * s[4], s[0] * s[1] * s[2], s[5]) for r, s in W.items()}
    M = {r: s[0] * s[1] * s[2] for r, s in W.items()}
    assert M["i"] == 15 < co.CV_KC and plan["i"] == (1, 16)
    assert plan["j"] == (7, 464) and co.partitions(M["j"], 7, 464)[-1] == (2784, 3240) and (3240 - 2784) % co.CV_KC == 8
    assert plan["k"][0] == 6
    assert plan["l"] == (130, 512) and plan["l"][0] > 128 and plan["l"][0] % 64 != 0 and all(hi > lo for lo, hi in co.partitions(M["l"], 130, 512))
    B, T, F, k, ci, cout = W["m"]
    assert co.cdiv(k * k * ci, co.CV_BM) == 4 and co.conv_tile_n(cout) == 64 and cout // 64 == 4
    assert plan["m"] == (64, 528) and M["m"] == 33152
    parts = co.partitions(M["m"], 64, 528)
    assert [p for p, (lo, hi) in enumerate(parts) if hi <= lo] == [63] and 63 * 528 > M["m"]
    # the narrow reduce (P < 64) and the wide one (P >= 64) both run, the wide one with one and with several lane trips
    assert {p < 64 for p, _ in plan.values()} == {True, False}
    assert all(r in W for r in paths.WGRAD1_TWICE)


def test_strided_rows_select_their_paths():
    assert sorted({s[0] * co.out_size(s[1], s[2], s[5])[0] for s in paths.STRIDED_P}) == [128, 129, 300]      # p
    assert {(co.conv_tile_n(s[4]), co.conv_tile_n(s[3])) for s in paths.STRIDED_P} == {(32, 16)}
    assert {(s[4] // 32, s[3] // 16) for s in paths.STRIDED_P} == {(1, 1), (3, 3)}
    for row in ("q_tf", "q_ft"):                                                                             # q
        B, T, F, ci, cout, taps = paths.STRIDED[row]
        assert co.out_size(T, F, taps) == (5, 3)
        kv = [co.as_taps(taps).kt * co.sconv_fwd_taps(F, taps, fo)[1] * ci for fo in range(3)]
        assert kv == [2, 1, 0]
    assert paths.STRIDED["q_tf"][5][7] == 1 and paths.STRIDED["q_ft"][5][7] == 0
    B, T, F, ci, cout, taps = paths.STRIDED["r"]                                                             # r
    assert taps[2] > taps[1] and co.out_size(T, F, taps) == (5, 3)
    assert [f for f in range(F) if co.sconv_dgrad_taps(F, taps, f)[1] == 0] == [2, 5, 8, 9]
    # every live tap the restatement reports reads inside the image / the output (the kernels' loads carry no frequency guard)
    for (B, T, F, ci, cout, taps) in paths.STRIDED_P + list(paths.STRIDED.values()) + list(paths.STRIDED_WGRAD.values()):
        t = co.as_taps(taps)
        To, Fo = co.out_size(T, F, t)
        assert To >= 1 and Fo >= 1 and t.pt0 < t.kt and t.pf0 < t.kf
        for fo in range(Fo):
            j0, nj = co.sconv_fwd_taps(F, t, fo)
            assert all(0 <= fo * t.sf + j - t.pf0 < F for j in range(j0, j0 + nj))
            assert nj == sum(0 <= fo * t.sf + j - t.pf0 < F for j in range(t.kf))
        for f in range(F):
            j0, nj, fo0 = co.sconv_dgrad_taps(F, t, f)
            reach = [j for j in range(t.kf) if (f + t.pf0 - j) % t.sf == 0 and 0 <= (f + t.pf0 - j) // t.sf < Fo]
            assert [j0 + t.sf * m for m in range(nj)] == reach and all((f + t.pf0 - j) // t.sf == fo0 - m for m, j in enumerate(reach))


def test_strided_wgrad_rows_skip_what_they_say():
    R = paths.STRIDED_WGRAD
    got = {}
    for row, (B, T, F, ci, cout, taps) in R.items():
        P, per, skipped, dead = co.sconv_wgrad_pairs(B, T, F, ci, cout, taps)
        assert co.cdiv(27 * ci, co.CV_BM) == 14 and (P, per) == (2, 512) and co.out_size(T, F, taps)[1] == 2
        assert skipped <= dead                                  # the kernel skips only what contributes nothing
        assert dead - skipped <= {(0, 0), (0, 1)}               # and everything that does, but for the bias tile
        got[row] = (skipped, dead)
    assert R["s"][0] * R["s"][1] == 512
    assert got["s"][0] == {(t, 0) for t in range(1, 6)} and got["s"][1] - got["s"][0] == {(0, 0)}
    assert got["t"][0] == {(t, 0) for t in range(1, 6)} | {(t, 1) for t in range(9, 14)}
    sk = got["u"][0]
    assert (1, 0) in sk and (2, 0) not in sk and (6, 0) not in sk and all(p == 0 for _, p in sk)
    assert sorted(j for _, j in co.sconv_wgrad_tile_taps(64, R["u"][5], 1)) == [2, 3]
    assert sorted(j for _, j in co.sconv_wgrad_tile_taps(64, R["u"][5], 2)) == [4, 5]
    assert sorted(j for _, j in co.sconv_wgrad_tile_taps(64, R["u"][5], 6)) == [3, 4]      # straddles the left edge: jmax decides
    assert R["v"][0] * R["v"][1] == 500 and got["v"][0] == set() and got["v"][1] == set()
    assert co.partitions(1000, 2, 512)[0] == (0, 512)           # partition 0 holds column 0 and 12 pixels of column 1


def test_elementwise_rows_select_their_paths():
    assert [r * c > co.EW_CAP for r, c in paths.BN_RELU] == [True, False, False]
    assert [b * t * c > co.EW_CAP for b, t, f, c, gap in paths.BN_RELU_MAXF] == [True, False, False]
    assert [s[2] for s in paths.BN_RELU_MAXF] == [2, 1, 4] and [s[4] > 0 for s in paths.BN_RELU_MAXF] == [False, False, True]
    assert paths.POOL[0] == (1, 2, 2, 1) and paths.POOL[1][1] % 2 == 1 and all(v % 2 for v in paths.POOL[2][1:3])
    L = paths.L2_LAYOUTS
    assert len(L["tiny"]) == 16 == len(L["straddle"]) and {0, 1, 5} <= set(L["tiny"]) and {0, 1, 5} <= set(L["straddle"])
    assert co.cdiv(sum(L["tiny"]), paths.L2_BLOCKS) == 1 and sum(L["tiny"]) < paths.L2_BLOCKS
    per = co.cdiv(sum(L["straddle"]), paths.L2_BLOCKS)
    ends = np.cumsum(L["straddle"])
    assert per == 301 and sum(1 for e in ends[:-1] if e % per) >= 10          # tensor boundaries inside slices
    assert L["big"] == [1 << 21]
