"""
Pins oracle/nnops_np.py on the CPU, four ways:
  1. every function against float64 torch (autograd where torch has the operation) to 1e-12;
  2. its restatement of the workspace sizes against the library's own host functions lidbox_bn_workspace and
     lidbox_softmax_head_workspace, which need no GPU;
  3. for every row of the PATHS tables of tests/test_nnops_paths_gpu.py and tests/test_bn_attention_paths_gpu.py, the property
     the row is there for, computed from the oracle's restatement of the conditions in nnops.hip / batchnorm.hip / attention.hip:
     a shape that stops selecting its path fails here;
  4. fp32 emulations of the kernels' summation orders stay inside the bounds the GPU modules assert, on both data sets -- and
     where those modules assert bit-identity between two kernels, the reason the order is the same is stated here.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import test_bn_attention_paths_gpu as bnp
import test_nnops_paths_gpu as paths
from oracle import nnops_np as no

TOL = 1e-12


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native


def _close(got, want, tol=TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())


def _t(a):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=True)


# ---------------------------------------------------------------------------------------------------- 1. the oracle itself
@pytest.mark.parametrize("B,T,C", [(2, 1, 3), (3, 7, 5), (2, 33, 8)])
def test_pooling_matches_torch_autograd(B, T, C):
    rng = np.random.default_rng(B + T + C)
    x = rng.standard_normal((B, T, C))
    x[0, :, 1] = 0.5                                                     # constant over T: the clipped stddev
    dout = rng.standard_normal((B, 2 * C))
    xt = _t(x)
    mean = xt.mean(dim=1)
    var = ((xt - mean[:, None, :]) ** 2).mean(dim=1)
    out = torch.cat([mean, torch.sqrt(torch.clamp(var, no.STDDEV_CLIP, float(np.finfo(np.float32).max)))], dim=1)
    (out * torch.tensor(dout)).sum().backward()
    m, v, pooled = no.stats_pool_fwd(x)
    _close(pooled, out.detach().numpy())
    _close(no.stats_pool_bwd(x, pooled, dout), xt.grad.numpy())
    assert pooled[0, C + 1] == np.sqrt(no.STDDEV_CLIP) and (T == 1 or (pooled[1:, C:] > 1e-3).all())
    _close(no.stats_pool_bwd(x, pooled, dout)[0, :, 1], np.full(T, dout[0, 1] / T))       # clipped: dmean / T only
    _close(no.stats_pool_bwd(x, pooled, dout, True), xt.grad.numpy() * (x > 0))
    assert (no.stats_pool_bwd_abs(x, pooled, dout) >= np.abs(no.stats_pool_bwd(x, pooled, dout)) - 1e-12).all()
    xt = _t(x)
    (torch.relu(xt).mean(dim=1) * torch.tensor(dout[:, :C])).sum().backward()
    _close(no.avg_pool_fwd(x), x.mean(axis=1))
    _close(no.avg_pool_bwd(x, dout[:, :C], True), xt.grad.numpy())
    _close(no.avg_pool_bwd(x, dout[:, :C]), np.broadcast_to(dout[:, None, :C] / T, x.shape))


def test_bf16_round_matches_torch():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(5000).astype(np.float32) * 100, np.float32([0, -0.0, 1.00390625, 1.01171875, 1e-30])])
    assert np.array_equal(no.bf16_round(a), torch.from_numpy(a).bfloat16().float().numpy())


@pytest.mark.parametrize("B,N", [(1, 1), (5, 7), (4, 65)])
def test_losses_match_torch_autograd(B, N):
    rng = np.random.default_rng(B + N)
    z = rng.standard_normal((B, N)) * 3
    y = rng.integers(0, N, size=B)
    _close(no.softmax(z), torch.softmax(torch.tensor(z), dim=1).numpy())
    _close(no.log_softmax(z), torch.log_softmax(torch.tensor(z), dim=1).numpy())
    # Keras applies the cross-entropy to the log-probabilities themselves: a second log_softmax
    lt = _t(no.log_softmax(z))
    loss = Fn.cross_entropy(lt, torch.tensor(y), reduction="sum") * 0.37
    loss.backward()
    got_loss, got_dz, rows = no.nll(lt.detach().numpy(), y, 0.37)
    _close(got_loss, loss.item() / 0.37 / B)
    _close(got_dz, lt.grad.numpy())
    _close(rows, Fn.cross_entropy(lt.detach(), torch.tensor(y), reduction="none").numpy())
    # clipped-probability form, with saturated rows
    if N >= 6:
        z[0, :] = 0
        z[0, 0] = 40
        z[1, 0] = -30
    zt = _t(z)
    q = torch.clamp(torch.softmax(zt, dim=1), no.KERAS_EPSILON, 1 - no.KERAS_EPSILON)
    per = torch.log(q.sum(dim=1)) - torch.log(q[torch.arange(B), torch.tensor(y)])
    (per.sum() * 0.37).backward()
    p, l2, dz = no.softmax_nll(z, y, 0.37)
    _close(p, torch.softmax(zt, dim=1).detach().numpy())
    _close(l2, per.mean().item())
    _close(dz, zt.grad.numpy())
    if B >= 5:                                                          # invalid labels: NaN loss, zero rows, the others untouched
        yb = y.copy()
        yb[1], yb[3] = N, -1
        l3, dz3, rows3 = no.nll(no.log_softmax(z), yb, 0.37)
        _, dz_ok, _ = no.nll(no.log_softmax(z), y, 0.37)
        assert np.isnan(l3) and np.isnan(rows3[[1, 3]]).all() and not dz3[[1, 3]].any() and np.array_equal(dz3[[0, 2, 4]], dz_ok[[0, 2, 4]])
        _, l4, dz4 = no.softmax_nll(z, yb, 0.37)
        assert np.isnan(l4) and not dz4[[1, 3]].any()


@pytest.mark.parametrize("B,K,N,relu", [(5, 7, 3, True), (4, 70, 8, False), (1, 3, 1, True)])
def test_softmax_head_matches_torch_autograd(B, K, N, relu):
    rng = np.random.default_rng(B + K + N)
    a = rng.standard_normal((B, K))                                      # pre-activation of the layer below
    W, b = rng.standard_normal((K, N)) / np.sqrt(K), rng.standard_normal(N)
    y = rng.integers(0, N, size=B)
    at, Wt, bt = _t(a), _t(W), _t(b)
    ht = torch.relu(at) if relu else at
    logp = torch.log_softmax(ht @ Wt + bt, dim=1)
    loss = Fn.cross_entropy(logp, torch.tensor(y), reduction="mean")
    loss.backward()
    h = ht.detach().numpy()
    got = no.softmax_head(h, W, b, y, 1.0 / B, relu)
    _close(got["logp"], logp.detach().numpy())
    _close(got["loss"], loss.item())
    _close(got["dW"], Wt.grad.numpy())
    _close(got["db"], bt.grad.numpy())
    _close(got["dh"], at.grad.numpy())
    dW, S_dW, db, S_db, dh, S_dh = no.head_grads_from_dz(h, W, got["dz"], relu)
    _close(dW, got["dW"])
    _close(db, got["db"])
    _close(dh, got["dh"])
    assert (S_dW >= np.abs(dW) - 1e-12).all() and (S_db >= np.abs(db) - 1e-12).all() and (S_dh >= np.abs(dh) - 1e-12).all()
    assert (got["S_z"] >= np.abs(got["z"]) - 1e-12).all()


def test_l2_normalize_matches_torch_autograd():
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((5, 9)), rng.standard_normal((5, 9))
    xt = _t(x)
    yt = xt / torch.sqrt(torch.clamp((xt * xt).sum(dim=1, keepdim=True), min=no.L2_EPS))
    (yt * torch.tensor(g)).sum().backward()
    _close(no.l2_normalize(x), yt.detach().numpy())
    _close(no.l2_normalize_bwd(x, g), xt.grad.numpy())
    x[2] = 0.0                                                           # clipped: y = x / sqrt(eps), dx = g / sqrt(eps)
    assert not no.l2_normalize(x)[2].any()
    _close(no.l2_normalize_bwd(x, g)[2], g[2] / np.sqrt(no.L2_EPS))


@pytest.mark.parametrize("R,C", [(1, 3), (2, 1), (37, 5)])
def test_batchnorm_matches_torch_autograd(R, C):
    rng = np.random.default_rng(R + C)
    x = rng.standard_normal((R, C)) * 2 + 1
    gam, bet = rng.uniform(0.5, 1.5, C), rng.standard_normal(C)
    mm0, mv0 = rng.standard_normal(C), rng.uniform(0.5, 2, C)
    dy = rng.standard_normal((R, C))
    for bessel in (0, 1):
        s = no.bn_train_stats(x, gam, bet, 1e-3, 0.9, bessel, mm0, mv0)
        rm, rv = torch.tensor(mm0), torch.tensor(mv0)
        if R > 1:
            # torch's batch_norm moves the running variance towards the UNBIASED estimate: the bessel = 1 form
            want = Fn.batch_norm(torch.tensor(x), rm, rv, torch.tensor(gam), torch.tensor(bet), True, 0.1, 1e-3)
            _close(no.f64(no.bn_apply(x, s["scale"], s["shift"])), want.numpy(), 1e-6)          # fp32 fma of float64 constants
            _close(x * s["scale"] + s["shift"], want.numpy())
            _close(s["moving_mean"], rm.numpy())
            if bessel:
                _close(s["moving_var"], rv.numpy())
        _close(s["var"], x.var(axis=0))
        target = x.var(axis=0, ddof=1) if bessel and R > 1 else x.var(axis=0)
        _close(s["moving_var"], mv0 * 0.9 + target * 0.1)
        _close(s["invstd"], 1 / np.sqrt(x.var(axis=0) + 1e-3))
    assert no.bn_train_stats(x, gam, bet, 1e-3, 0.9, 1)["moving_mean"] is None
    # backward through the batch statistics, with and without the ReLU in front
    for relu in (False, True):
        at, gt, bt = _t(x), _t(gam), _t(bet)
        ht = torch.relu(at) if relu else at
        yt = gt * (ht - ht.mean(0)) / torch.sqrt(ht.var(0, unbiased=False) + 1e-3) + bt
        (yt * torch.tensor(dy)).sum().backward()
        h = ht.detach().numpy()
        s = no.bn_train_stats(h, gam, bet, 1e-3, 0.0, 0)
        got = no.bn_bwd(h, dy, s["mean"], s["invstd"], gam, relu)
        _close(got["dgamma"], gt.grad.numpy())
        _close(got["dbeta"], bt.grad.numpy())
        _close(got["dx"], at.grad.numpy(), 1e-11)
        for k in ("dgamma", "dbeta", "dx"):
            assert (got["S_" + k] >= np.abs(got[k]) - 1e-12).all()


@pytest.mark.parametrize("rows,C,d_f", [(3, 8, 2), (2, 7, 7), (4, 6, 1)])
def test_frequency_attention_matches_torch_autograd(rows, C, d_f):
    rng = np.random.default_rng(rows + C + d_f)
    a, logits, dHw = rng.standard_normal((rows, C)), rng.standard_normal((rows, d_f)), rng.standard_normal((rows, C))
    for relu in (False, True):
        at, lt = _t(a), _t(logits)
        Ht = torch.relu(at) if relu else at
        Ft = torch.softmax(lt, dim=1)
        Hw = (Ht.reshape(rows, d_f, C // d_f) * Ft[:, :, None]).reshape(rows, C)
        (Hw * torch.tensor(dHw)).sum().backward()
        H = Ht.detach().numpy()
        F, got_Hw = no.freq_attention_fwd(H, logits)
        _close(F, Ft.detach().numpy())
        _close(got_Hw, Hw.detach().numpy())
        got = no.freq_attention_bwd(H, F, dHw, relu)
        _close(got["dlogits"], lt.grad.numpy())
        _close(got["dH"], at.grad.numpy())
        assert (got["S_dF"] >= np.abs(got["dF"]) - 1e-12).all()


# ---------------------------------------------------------------------------------------------------- 2. workspaces, against the library
def test_bn_slices_match_the_library(nv):
    for R in list(bnp.BN_R) + [r for r, _ in bnp.BN_LARGE + bnp.BN_TRIPS] + [0, 257, 65791, 262143, 262144, 10 ** 7]:
        for C in (1, 4, 68):
            assert nv.lib.lidbox_bn_workspace(R, C) == no.bn_workspace_bytes(R, C), (R, C)
    assert nv.lib.lidbox_bn_workspace(-1, 4) == 0 == nv.lib.lidbox_bn_workspace(5, 0)
    assert [no.bn_slices(r) for r in (1, 255, 256, 511, 512, 513, 65792, 262144, 262145)] == [1, 1, 1, 1, 2, 2, 257, 1024, 1024]


def test_head_workspace_matches_the_library(nv):
    for (N, K, B, *_rest) in paths.HEAD.values():
        assert nv.lib.lidbox_softmax_head_workspace(B, K, N) == no.head_workspace_bytes(B, K, N) == (B * N + B) * 4
        assert nv.lib.lidbox_softmax_head_supported(K, N) == 1
    assert nv.lib.lidbox_softmax_head_workspace(0, 5, 3) == 0 and nv.lib.lidbox_softmax_head_supported(5, 33) == 0


# ---------------------------------------------------------------------------------------------------- 3. what every PATHS row selects
def _fwd_path(row):
    T, C, pitch, mis = row
    bs, rs = paths._strides(T, C, pitch)
    return no.pool_fwd_path(T, C, bs, rs, 4 if mis == "x" else 0, 4 if mis == "out" else 0)


def test_pool_forward_rows_select_their_paths():
    P = paths.POOL_FWD
    reg = {n: _fwd_path(r) for n, r in P.items() if n.startswith("reg_")}
    assert all(p[0] == "reg" for p in reg.values())
    # every TMAX at its upper edge and one above the previous edge
    edges = {}
    for n, p in reg.items():
        edges.setdefault(p[1], set()).add(P[n][0])
    assert edges == {8: {1, 8}, 16: {9, 16}, 24: {17, 24}, 32: {25, 32}, 36: {33, 36}, 40: {37, 40}}
    for n in reg:
        T, C, pitch, _ = P[n]
        blocks, live, _, _ = no.pool_fwd_grid(T, C, reg[n])
        assert (blocks, live) == ((1, 1) if C == 4 else (2, 1))          # one live lane / a second x block of one lane
        bs, rs = paths._strides(T, C, pitch)
        assert no.pool_bf16_accepts(T, C, bs, rs, 0, 0)                  # every register row also runs over bfloat16
        if pitch == "pitched":
            assert rs == C + 4 and bs == (T + 2) * rs
    assert {(P[n][1], P[n][2]) for n in reg} == {(4, "dense"), (4, "pitched"), (260, "dense"), (260, "pitched")}
    # pool_fwd_kernel<*, 4>
    assert _fwd_path(P["lds4_T41"]) == ("lds", 4) == _fwd_path(P["lds4_T100"]) == _fwd_path(P["lds4_T5_out"])
    assert no.pool_fwd_grid(41, 68, ("lds", 4)) == (2, 1, 3, 2) and no.pool_fwd_grid(100, 68, ("lds", 4)) == (2, 1, 7, 6)
    assert no.pool_fwd_grid(5, 68, ("lds", 4))[2:] == (1, 0) and P["lds4_T5_out"][3] == "out"      # 11 idle time groups
    assert P["lds4_T100"][2] == "pitched"
    # pool_fwd_kernel<*, 1>, three ways, each at T = 1, 15, 16, 17, 100
    for T in (1, 15, 16, 17, 100):
        for why in ("C5", "C17", "x", "rs"):
            row = P["lds1_T%d_%s" % (T, why)]
            assert row[0] == T and _fwd_path(row) == ("lds", 1)
        assert P["lds1_T%d_x" % T][1] % 4 == 0 and P["lds1_T%d_x" % T][3] == "x"
        assert P["lds1_T%d_rs" % T][1] % 4 == 0 and paths._strides(T, 8, "odd")[1] % 4 == 1
        assert no.pool_fwd_grid(T, 17, ("lds", 1))[:2] == (2, 1)         # C = 17: a second x block of one channel
    assert _fwd_path(paths.POOL_CONST["const_T7"]) == ("reg", 8) and _fwd_path(paths.POOL_CONST["const_T50"]) == ("lds", 4)
    # every entry of the table is covered by one of the three families
    assert {n.split("_")[0] for n in P} == {"reg", "lds4", "lds1"}
    # why <*, 4> and <*, 1> may be compared bit for bit: time group g adds rows g, g + 16, ... and the groups are added 0 .. 15
    # in both -- the emulation has no V in it
    assert no.pool_chain(41, ("lds", 4)) == no.pool_chain(41, ("lds", 1)) == 3 + 16 + 1


def _bwd_path(row):
    T, C, pitch, mis = row
    bs, rs = paths._strides(T, C, pitch)
    return no.pool_bwd_path(T, C, bs, rs, 0, 4 if mis == "dx" else 0, 4 if mis == "pooled" else 0, 4 if mis == "dout" else 0)


def test_pool_backward_rows_select_their_paths():
    P = paths.POOL_BWD
    rows = {n: _bwd_path(r) for n, r in P.items() if n.startswith("rows_")}
    assert all(p[0] == "rows" for p in rows.values())
    assert {P[n][0]: rows[n][1] for n in rows} == {1: 1, 11: 1, 12: 1, 13: 2, 24: 2, 47: 4, 48: 4}        # z row blocks
    assert {P[n][0] % 12 for n in rows} == {0, 1, 11}                     # ragged and full last blocks
    for n in rows:
        T, C, pitch, _ = P[n]
        bs, rs = paths._strides(T, C, pitch)
        # the shadow the test asks for keeps the vector kernel, and the bf16 entry point takes the rows up to T = 40
        assert no.pool_bwd_path(T, C, bs, rs, 0, 0, 0, 0, shadow=((T + 1) * (C + 4), C + 4, 0)) == rows[n]
        assert no.pool_bf16_accepts(T, C, bs, rs, 0, 0) == (T <= 40)
    assert _bwd_path(P["loop4_T49"]) == ("loop", 4, 8) and P["loop4_T49"][2] == "pitched"
    assert _bwd_path(P["loop4_T5_pooled"]) == ("loop", 4, 5) == _bwd_path(P["loop4_T5_dout"])
    assert (P["loop4_T5_pooled"][3], P["loop4_T5_dout"][3]) == ("pooled", "dout")
    assert _bwd_path(P["loop1_T13_C5"]) == ("loop", 1, 8) == _bwd_path(P["loop1_T13_dx"]) == _bwd_path(P["loop1_T49_C5"])
    assert P["loop1_T13_dx"][1] % 4 == 0
    assert _bwd_path(paths.POOL_BWD_CONST["const_T7"]) == ("rows", 1) and _bwd_path(paths.POOL_BWD_CONST["const_T50"]) == ("loop", 4, 8)
    # the three paths of test_pool_backward_vector_and_scalar_kernels_agree_bit_for_bit: no sum, one expression per element
    assert [no.pool_bwd_path(13, 8, 104, 8, 0, d, p, 0) for p, d in ((0, 0), (4, 0), (0, 4))] == [("rows", 2), ("loop", 4, 8), ("loop", 1, 8)]


def test_head_rows_select_their_paths():
    H = paths.HEAD
    assert len(H) <= 60
    seen = set()
    for NP, U in ((4, 8), (8, 4), (16, 2), (32, 1)):
        assert no.head_np_u(NP) == (NP, U)
        k7, k1, k1p, k2 = (H["np%d_K%d" % (NP, K)] for K in (7, 64 * U, 64 * U + 1, 2 * 64 * U + 37))
        assert all(r[0] == NP and no.head_wvec(NP, 0) for r in (k7, k1, k1p, k2))
        assert no.head_trips(7, NP) == (1, 0, 0)                         # lanes 7 - 63 never enter the loop
        assert no.head_trips(64 * U, NP) == (1, 1, 0)                    # one full trip, nothing to reload
        assert no.head_trips(64 * U + 1, NP) == (2, 1, 1)                # lane 0 alone takes (and reloads) a second trip
        assert no.head_trips(2 * 64 * U + 37, NP) == (3, 2, 2)           # two reloaded trips
        mis = H["np%d_misW" % NP]
        assert mis[3] and not no.head_wvec(NP, 4) and mis[:3] == k2[:3]   # the same shape as the aligned run it is compared with
        seen.add(NP)
    assert seen == {4, 8, 16, 32}
    assert [no.head_np_u(H["N%d" % N][0]) for N in (1, 5, 9, 17)] == [(4, 8), (8, 4), (16, 2), (32, 1)]
    assert not any(no.head_wvec(H["N%d" % N][0], 0) for N in (1, 5, 9, 17))
    assert {r[0] for r in H.values()} >= {1, 4, 5, 8, 9, 16, 17, 32} and {r[2] for r in H.values()} == {1, 5, 129}
    assert 129 % 4 == 1 and no.cdiv(129, 128) == 2                       # wgrad: a second 128-row trip of one row
    assert {r[4] for r in H.values()} == {0, 1} and {r[5] for r in H.values()} == {True, False}
    assert any(r[6] for r in H.values()) and not all(r[6] for r in H.values())
    assert no.head_trips(H["nodh_np4"][1], 4)[2] == 2 and no.head_trips(H["nodh_np32"][1], 32)[2] == 2   # a reload that dh = NULL skips


def test_loss_and_l2_rows_select_their_paths():
    assert [no.row_lane_trips(N) for N in paths.LOSS_N] == [(1, 0), (1, 0), (1, 1), (2, 1), (3, 2)]
    assert [no.loss_trips(B) for B in paths.LOSS_B] == [(1, 0), (1, 0), (1, 1), (2, 1)]
    assert [no.row_lane_trips(D) for D in paths.L2_D] == [(1, 0), (1, 0), (1, 1), (2, 1)]
    assert any(D == N for _, D, N in paths.AP) and any(N > 64 for _, _, N in paths.AP) and any(N == 1 for _, _, N in paths.AP)
    assert all(D >= N for _, D, N in paths.AP)


def test_batchnorm_rows_select_their_paths():
    assert [(no.bn_slices(R), no.bn_rows_per_slice(R)) for R in bnp.BN_R] == [(1, 1), (1, 255), (1, 256), (1, 511), (2, 256), (2, 257)]
    assert no.bn_slice_rows(513) == [257, 256]
    (R1, C1), (R2, C2) = bnp.BN_LARGE
    assert no.bn_slices(R1) == 257 and no.bn_channel_sum_trips(R1) == 2 and no.bn_channel_sum_trips(R1 - 256) == 1
    rows = no.bn_slice_rows(R2)
    assert no.bn_slices(R2) == 1024 and no.bn_rows_per_slice(R2) == 257 and sum(rows) == R2
    assert rows[1020] == 5 and rows[1021:] == [0, 0, 0] and min(rows[:1020]) == 257
    assert {C % 4 == 0 for C in bnp.BN_C} == {True, False} and {C <= no.BN_COLS for C in bnp.BN_C} == {True, False}
    for batch, rpb, C, gap in bnp.BN_ROWS:
        bs = rpb * C + gap
        vec, trips = no.bn_apply_path(batch * rpb, C, (0, 0, 0, 0), C, batch, bs)
        assert vec == (C % 4 == 0 and gap % 4 == 0) and trips == 1 and batch > 1
    assert {(C % 4 == 0, gap % 4) for _, _, C, gap in bnp.BN_ROWS} >= {(True, 0), (True, 2)}
    (Rv, Cv), (Rs, Cs) = bnp.BN_TRIPS
    assert no.bn_apply_path(Rv, Cv, (0, 0, 0, 0), Cv, 1, 0) == (True, 2) and no.bn_apply_path(Rs, Cs, (0, 0, 0, 0), Cs, 1, 0) == (False, 2)
    assert no.bn_apply_path(Rv - 3, Cv, (0, 0, 0, 0), Cv, 1, 0) == (True, 1)
    # a misaligned x at C % 4 == 0 selects the scalar kernels; they evaluate the same expression per element (no sum), so the
    # GPU module may compare their bits with the vector kernels'
    assert no.bn_apply_path(513, 68, (4, 0, 0, 0), 68, 1, 0) == (False, 1)


def test_attention_rows_select_their_paths():
    A = bnp.ATTENTION
    assert [no.attention_grid(A[n][0]) for n in ("one", "five", "trip2_a", "trip2_b")] == [(1, 1), (2, 1), (2048, 2), (2048, 2)]
    assert A["trip2_a"][0] - 2048 * 4 == 1 and A["trip2_b"][0] - 2048 * 4 == 5          # one wave / four waves and one of the next block
    assert {(A[n][2], A[n][1] // A[n][2]) for n in A if n.startswith("df")} == {(d, cb) for d in (1, 63, 64) for cb in (1, 4)}
    assert not no.attention_vec(A["scalar"][1], (0, 0)) and no.attention_vec(A["max_c"][1], (0, 0))
    assert no.attention_bwd_accepts(4096, 64) and not no.attention_bwd_accepts(4097, 1)
    assert all(no.attention_bwd_accepts(C, d) for _, C, d in A.values())
    # the misaligned rows: C % 4 == 0 and yet scalar; the scalar and the vector loops move and multiply the same values and the
    # only sums (dF over a bin, in LDS order; the wave reductions) are shared code, hence the same bits
    assert not no.attention_vec(8, (4, 0)) and not no.attention_vec(256, (0, 4)) and no.attention_vec(8, (0, 0))


# ---------------------------------------------------------------------------------------------------- 4. the bounds hold for the kernels' orders
def _ratio(got, ref, bound):
    return float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())


@pytest.mark.parametrize("kind", paths.KINDS)
def test_pool_bounds_hold_for_an_fp32_emulation(kind):
    worst = 0.0
    for T, C, path in [(1, 4, ("reg", 8)), (33, 8, ("reg", 36)), (40, 8, ("reg", 40)), (5, 8, ("lds", 4)), (41, 8, ("lds", 4)),
                       (100, 8, ("lds", 1))]:
        x, _ = paths._pool_case(T, C, kind, False)
        n = no.pool_chain(T, path)
        mean, var, out = no.stats_pool_fwd(x)
        r = _ratio(no.emu_pool_mean(x, path), mean, no.error_bound(no.pool_mean_abs(x), n))
        lo, hi = no.stddev_interval(x, n)
        sd = no.emu_pool_std(x, path).astype(np.float64)
        assert r <= 1.0 and (sd >= lo).all() and (sd <= hi).all(), (T, C, path, r)
        worst = max(worst, r)
    print("pool mean, emulated order, %s: max err/bound = %.3e" % (kind, worst))
    # dx = fma(k, x - mean, a), a = dmean * (1 / T), k = (dsd / (2 sd)) * 2 * (1 / T), every operation rounded to fp32
    f = np.float32
    for T in (1, 13, 49):
        x, dout = paths._pool_case(T, 8, kind, False)
        pooled = no.stats_pool_fwd(x)[2].astype(f)
        invT = f(1) / f(T)
        a = (dout[:, :8] * invT).astype(f)
        k = (((dout[:, 8:] / (f(2) * pooled[:, 8:]).astype(f)).astype(f) * f(2)).astype(f) * invT).astype(f)
        k = np.where(pooled[:, 8:] > f(1.0000001e-5), k, f(0))
        d = (x - pooled[:, None, :8]).astype(f)
        g = no.fma32(np.broadcast_to(k[:, None, :], x.shape), d, np.broadcast_to(a[:, None, :], x.shape))
        r = _ratio(g, no.stats_pool_bwd(x, pooled, dout), no.error_bound(no.stats_pool_bwd_abs(x, pooled, dout), 8))
        assert r <= 1.0, (T, r)
    # a constant channel: every partial sum of 0.5 is exact, the mean exact, the stddev the clipped value
    x, _ = paths._pool_case(50, 8, kind, True)
    assert (no.emu_pool_mean(x, ("lds", 4))[:, paths.CONST_CH] == 0.5).all()
    assert (no.emu_pool_std(x, ("lds", 4))[:, [paths.CONST_CH, paths.NEAR_CH]] == np.sqrt(np.float32(1e-10))).all()
    # the nearly constant channel is clipped too, yet no x equals the mean: the oracle's backward gives it dmean / T alone, and a
    # backward without the clip rule would add dsd (x - mean) / (sd T) ~ 0.1 dsd / T
    _, dout = paths._pool_case(50, 8, kind, True)
    pooled = no.stats_pool_fwd(x)[2]
    dx = no.stats_pool_bwd(x, pooled, dout)
    assert np.abs(dx[:, :, paths.NEAR_CH] - dout[:, None, paths.NEAR_CH].astype(np.float64) / 50).max() == 0.0
    leak = np.abs(dout[:, None, 8 + paths.NEAR_CH] * (x[:, :, paths.NEAR_CH] - pooled[:, None, paths.NEAR_CH]) / (pooled[:, None, 8 + paths.NEAR_CH] * 50))
    assert leak.min() > 1e3 * no.error_bound(no.stats_pool_bwd_abs(x, pooled, dout), 8)[:, :, paths.NEAR_CH].max()


@pytest.mark.parametrize("kind", paths.KINDS)
def test_head_bounds_hold_for_an_fp32_emulation(kind):
    worst = {}
    for name in ("np4_K1061", "np32_K165", "B129_np8", "N17"):
        N, K, B, *_ = paths.HEAD[name]
        h, W, b, y = paths._head_case(name, kind)
        ref = no.softmax_head(h, W, b, y, 1.0 / B)
        z = no.emu_head_logits(h, W, b)
        worst["z"] = max(worst.get("z", 0), _ratio(z, ref["z"], no.error_bound(ref["S_z"], no.head_logit_chain(K))))
        dz = ref["dz"].astype(np.float32)
        dW, S_dW, db, S_db, _, _ = no.head_grads_from_dz(h, W, dz)
        worst["dW"] = max(worst.get("dW", 0), _ratio(no.emu_head_dw(h, dz), dW, no.error_bound(S_dW, no.head_dw_chain(B))))
        lanes = np.zeros((N, no.cdiv(B, 64) * 64), np.float32)
        lanes[:, :B] = dz.T
        acc = no.emu_sum_in_order(lanes.reshape(N, -1, 64), axis=1)
        worst["db"] = max(worst.get("db", 0), _ratio(no.emu_butterfly(acc), db, no.error_bound(S_db, no.head_db_chain(B))))
        # dh[r, k] = sum_n dz[r, n] W[k, n]: one lane chains the NP classes with fma (the columns beyond N hold zeros)
        _, _, _, _, dh, S_dh = no.head_grads_from_dz(h, W, dz)
        acc = np.zeros((B, K), np.float32)
        for n in range(N):
            acc = no.fma32(np.broadcast_to(dz[:, n:n + 1], (B, K)), np.broadcast_to(W[None, :, n], (B, K)), acc)
        worst["dh"] = max(worst.get("dh", 0), _ratio(acc, dh, no.error_bound(S_dh, no.head_np_u(N)[0] + 1)))
    print("head, emulated order, %s: %s" % (kind, worst))
    assert max(worst.values()) <= 1.0 and min(worst.values()) > 0.0


@pytest.mark.parametrize("kind", paths.KINDS)
def test_attention_and_l2_bounds_hold_for_an_fp32_emulation(kind):
    for name in ("df64_cb4", "max_c", "df63_cb1"):
        rows, C, d_f = bnp.ATTENTION[name]
        H, logits, dHw = bnp._att_case(name, kind)
        F = no.softmax(logits).astype(np.float32)
        ref = no.freq_attention_bwd(H, F, dHw)
        dF = no.emu_attention_dF(H, dHw, d_f)
        assert _ratio(dF, ref["dF"], no.error_bound(ref["S_dF"], C // d_f)) <= 1.0
        # dlogits = f (dF - wave_sum(f dF)) in fp32 from the emulated dF
        fd = (F * dF).astype(np.float32)
        lanes = np.zeros((rows, 64), np.float32)
        lanes[:, :d_f] = fd
        s = no.emu_butterfly(lanes, (32, 16, 8, 4, 2, 1))
        dl = (F * (dF - s[:, None]).astype(np.float32)).astype(np.float32)
        assert _ratio(dl, ref["dlogits"], no.freq_attention_dlogits_bound(F, ref["dF"], ref["S_dF"], C // d_f)) <= 1.0
    for D in paths.L2_D + (300,):
        rng = np.random.default_rng([D, paths.KINDS.index(kind)])
        x, g = paths._draw(rng, kind, (6, D)), paths._draw(rng, kind, (6, D))
        s = no.emu_l2_sum(x)
        assert _ratio(s, (x.astype(np.float64) ** 2).sum(axis=1), no.error_bound((x.astype(np.float64) ** 2).sum(axis=1), no.l2_chain(D))) <= 1.0
        # the whole forward and backward with a correctly rounded 1 / sqrt (the device's rsqrtf may add 2 ulp, which the bound allows)
        inv = (np.float32(1) / np.sqrt(np.maximum(s, np.float32(1e-12)))).astype(np.float32)
        y = (x * inv[:, None]).astype(np.float32)
        assert _ratio(y, no.l2_normalize(x), no.l2_bounds(x)) <= 1.0
        dot = no.emu_lane_dot(x, g, (32, 16, 8, 4, 2, 1))
        k = (((dot * inv).astype(np.float32) * inv).astype(np.float32) * inv).astype(np.float32)
        dx = ((g * inv[:, None]).astype(np.float32) - (x * k[:, None]).astype(np.float32)).astype(np.float32)
        assert _ratio(dx, no.l2_normalize_bwd(x, g), no.l2_bounds(x, g)) <= 1.0


@pytest.mark.parametrize("kind", bnp.KINDS + ("far",))
def test_batchnorm_bounds_hold_for_float64_accumulation_in_another_order(kind):
    """the kernels accumulate in float64: any order of at most DCHAIN additions stays inside DNOISE.  Here: a plain running sum
    over 513 rows (a chain of 513 > DCHAIN additions), E[x^2] - mean^2 as the kernel forms the variance"""
    x, gamma, beta, mm0, mv0, _ = bnp._bn_case(513, 4, kind)
    s0 = np.zeros(4)
    s1 = np.zeros(4)
    for r in range(513):
        s0 += x[r].astype(np.float64)
        s1 += x[r].astype(np.float64) ** 2
    mean = s0 / 513
    var = np.maximum(s1 / 513 - mean * mean, 0)
    ref = no.bn_train_stats(x, gamma, beta, bnp.EPS, 0.0, 0)
    ax = np.abs(x.astype(np.float64))
    assert (np.abs(mean.astype(np.float32) - ref["mean"]) <= no.U * np.abs(ref["mean"]) + bnp.DNOISE * ax.mean(axis=0)).all()
    is32 = np.float32(1) / np.sqrt(var.astype(np.float32) + np.float32(bnp.EPS))
    assert (np.abs(is32 - ref["invstd"]) <= 2e-6 * ref["invstd"]).all()
    assert (np.abs(var.astype(np.float32) - ref["var"]) <= 2 * no.U * ref["var"] + 2 * bnp.DNOISE * (ax ** 2).mean(axis=0)).all()


@pytest.mark.parametrize("kind", bnp.KINDS)
def test_batchnorm_dx_bound_holds_for_an_fp32_emulation(kind):
    """dx in fp32 in the kernel's association, with the subtraction of xhat * mean_dyx contracted into an fma and not, from
    float64 sums over fp32 xhat.  4099 rows: a channel's |dgamma| is ~sqrt(R) while sum |dy xhat| is ~R, so mean_dyx carries an
    error far above u |mean_dyx| -- the term bn_dx_bound adds for it is what keeps the small elements inside"""
    R, C = 4099, 256
    rng = np.random.default_rng([R, C, bnp.KINDS.index(kind)])
    x, dy = bnp._draw(rng, kind, (R, C)), bnp._draw(rng, kind, (R, C))
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    mean, invstd, _, _ = bnp._consts(x, gamma, np.zeros(C, np.float32))
    ref = no.bn_bwd(x, dy, mean, invstd, gamma, True)
    f = np.float32
    xh = ((x - mean).astype(f) * invstd).astype(f)
    s0, s1 = dy.astype(np.float64).sum(axis=0), (dy.astype(np.float64) * xh.astype(np.float64)).sum(axis=0)
    e_db = no.error_bound(ref["S_dbeta"], 1) + bnp.DNOISE * ref["S_dbeta"]
    e_dg = no.error_bound(ref["S_dgamma"], 3) + bnp.DNOISE * ref["S_dgamma"]
    assert (np.abs(s0.astype(f) - ref["dbeta"]) <= e_db).all() and (np.abs(s1.astype(f) - ref["dgamma"]) <= e_dg).all()
    kd, km, kx = (gamma * invstd).astype(f), (s0 / R).astype(f), (s1 / R).astype(f)
    bound = no.bn_dx_bound(ref, R, e_db, e_dg)
    for inner in (((dy - km).astype(f) - (xh * kx).astype(f)).astype(f), no.fma32(-xh, kx, (dy - km).astype(f))):
        g = np.where(x > 0, (kd * inner).astype(f), f(0))
        assert _ratio(g, ref["dx"], bound) <= 1.0
