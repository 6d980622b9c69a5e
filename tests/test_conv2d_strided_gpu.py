"""
GPU tests of the strided, rectangular Conv2D (lidbox_conv2d_strided_*) and the BatchNormalization -> ReLU (-> max over
frequency) passes of csrc/conv2d.hip against float64 torch: torch.nn.functional.conv2d on the image [B, C, T, F] after an
explicit (possibly asymmetric) F.pad, autograd for dgrad / wgrad, and torch.amax (which splits the gradient evenly over ties,
as TF's _MinOrMaxGrad does) for the maximum.

Tolerances, set from the first measured errors (MI355X) with a margin of about 10x: relative L2 at most 6.8e-7 on fwd /
dgrad / wgrad (C_in = 128, F = 64) -> TOL = 1e-5.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _same(n, k, s):
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return out, pad // 2, pad - pad // 2


def _torch_conv(x, W, taps, bias=None):
    """x [B, T, F, C] float64, W Keras layout -> y [B, To, Fo, Co]"""
    Wt = W.permute(3, 2, 0, 1) if taps.time_first else W.permute(3, 2, 1, 0)    # [Co, Ci, kt, kf]
    xi = Fn.pad(x.permute(0, 3, 1, 2), (taps.pf0, taps.pf1, taps.pt0, taps.pt1))
    return Fn.conv2d(xi, Wt, bias, stride=(1, taps.sf)).permute(0, 2, 3, 1)


def _run(x, W, b, dyv, taps, Co, dgrad=True):
    """device fwd / dgrad / wgrad -> numpy (y, dx, dW, db)"""
    nv = _nv()
    st = nv.current_stream()
    B, T, F, Ci = x.shape
    xd, Wd, bd = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda() for a in (x, W, b))
    y0 = _torch_conv(torch.from_numpy(x), torch.from_numpy(W), taps)
    y = torch.full(y0.shape, float("nan"), dtype=torch.float32, device="cuda")
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(xd), B, T, F, Ci, nv.ptr(Wd), taps, Co, nv.ptr(bd), nv.ptr(y), st))
    dyd = torch.from_numpy(dyv.astype(np.float32)).cuda()
    dx = None
    if dgrad:
        dx = torch.full_like(xd, float("nan"))
        wsb = nv.lib.lidbox_conv2d_strided_dgrad_workspace(taps, Ci, Co)
        ws = torch.empty(max(16, wsb), dtype=torch.uint8, device="cuda")
        nv.check(nv.lib.lidbox_conv2d_strided_dgrad(nv.ptr(dyd), B, T, F, Ci, Co, nv.ptr(Wd), taps, nv.ptr(dx), nv.ptr(ws), ws.numel(), st))
    dW, db = torch.full_like(Wd, float("nan")), torch.full_like(bd, float("nan"))
    wsb = nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, F, Ci, Co, taps)
    ws = torch.empty(max(16, wsb), dtype=torch.uint8, device="cuda")
    nv.check(nv.lib.lidbox_conv2d_strided_wgrad(nv.ptr(xd), nv.ptr(dyd), B, T, F, Ci, Co, taps, nv.ptr(dW), nv.ptr(db), nv.ptr(ws),
                                                ws.numel(), st))
    torch.cuda.synchronize()
    return y.cpu().numpy(), None if dx is None else dx.cpu().numpy(), dW.cpu().numpy(), db.cpu().numpy()


def _check(B, T, F, Ci, Co, taps, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, F, Ci))
    W = rng.standard_normal((taps.kt, taps.kf, Ci, Co) if taps.time_first else (taps.kf, taps.kt, Ci, Co)) / np.sqrt(taps.kt * taps.kf * Ci)
    b = rng.standard_normal(Co)
    xt, Wt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (x, W, b))
    yr = _torch_conv(xt, Wt, taps, bt)
    dyv = rng.standard_normal(tuple(yr.shape))
    yr.backward(torch.from_numpy(dyv))
    y, dx, dW, db = _run(x, W, b, dyv, taps, Co, dgrad=Ci % 16 == 0)
    errs = [_rel(y, yr.detach().numpy()), _rel(dW, Wt.grad.numpy()), _rel(db, bt.grad.numpy())]
    if dx is not None:
        errs.append(_rel(dx, xt.grad.numpy()))
    print("B=%d T=%d F=%d Ci=%d Co=%d taps=(%d,%d)/%d pads (%d,%d,%d,%d) tf=%d: errors %s" % (
        B, T, F, Ci, Co, taps.kt, taps.kf, taps.sf, taps.pt0, taps.pt1, taps.pf0, taps.pf1, taps.time_first, errs))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("F", [1, 6, 7, 13, 40, 64])
@pytest.mark.parametrize("Ci,Co", [(1, 128), (128, 256)])
def test_clstm_geometry_matches_torch(F, Ci, Co):
    nv = _nv()
    _, p0, p1 = _same(F, 9, 6)
    taps = nv.Conv2DTaps(3, 9, 6, 1, 1, p0, p1, 1)
    _check(2, 7, F, Ci, Co, taps, seed=F + Ci)


@pytest.mark.parametrize("taps", [(5, 3, 2, 2, 1, 0, 2, 0), (3, 9, 6, 0, 2, 3, 5, 1), (1, 4, 3, 0, 0, 1, 0, 0)])
def test_other_kernels_and_orientation(taps):
    nv = _nv()
    _check(3, 9, 17, 32, 48, nv.Conv2DTaps(*taps), seed=sum(taps))


def test_forward_batch_position_bit_identical():
    nv = _nv()
    rng = np.random.default_rng(5)
    B, T, Ci, Co = 5, 11, 128, 256
    taps = nv.Conv2DTaps(3, 9, 6, 1, 1, 4, 4, 1)
    x = torch.from_numpy(rng.standard_normal((B, T, 7, Ci)).astype(np.float32)).cuda()
    W = torch.from_numpy((rng.standard_normal((3, 9, Ci, Co)) / 60).astype(np.float32)).cuda()
    st = nv.current_stream()
    full = torch.zeros((B, T, 2, Co), device="cuda")
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(x), B, T, 7, Ci, nv.ptr(W), taps, Co, None, nv.ptr(full), st))
    one = torch.zeros((1, T, 2, Co), device="cuda")
    xb = x[3:4].contiguous()
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(xb), 1, T, 7, Ci, nv.ptr(W), taps, Co, None, nv.ptr(one), st))
    torch.cuda.synchronize()
    assert torch.equal(full[3:4], one)



def test_wgrad_and_dgrad_run_to_run_bit_identical():
    nv = _nv()
    rng = np.random.default_rng(9)
    B, T, F, Ci, Co = 8, 40, 7, 128, 256
    taps = nv.Conv2DTaps(3, 9, 6, 1, 1, 4, 4, 1)
    x = rng.standard_normal((B, T, F, Ci))
    W = rng.standard_normal((3, 9, Ci, Co)) / 60
    dy = rng.standard_normal((B, T, 2, Co))
    a = _run(x, W, np.zeros(Co), dy, taps, Co)
    b = _run(x, W, np.zeros(Co), dy, taps, Co)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


def _bn_max_ref(x, scale, shift, dy):
    xt = torch.from_numpy(x).requires_grad_(True)
    v = xt * torch.from_numpy(scale) + torch.from_numpy(shift)
    vt = v.detach().requires_grad_(True)
    y = torch.relu(vt).amax(dim=2)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), vt.grad.numpy()


def test_bn_relu_max_forward_backward_with_ties():
    nv = _nv()
    st = nv.current_stream()
    rng = np.random.default_rng(3)
    B, T, F, C = 3, 5, 4, 32
    x = rng.standard_normal((B, T, F, C)).astype(np.float32)
    x[0, 0, 1, 0] = x[0, 0, 3, 0] = 3.0            # a positive tie: the gradient is halved
    x[1, 2, :, 1] = -1.0                            # every relu output 0: ties at zero get nothing
    x[2, 4, 0, 2] = x[2, 4, 2, 2] = x[2, 4, 3, 2] = 5.0   # three-way tie
    scale = np.ones(C, np.float32)
    scale[5] = -0.5
    shift = rng.standard_normal(C).astype(np.float32) * 0.1
    shift[:3] = 0.0
    dy = rng.standard_normal((B, T, C)).astype(np.float32)
    yr, dvr = _bn_max_ref(x.astype(np.float64), scale.astype(np.float64), shift.astype(np.float64), dy.astype(np.float64))
    xd, sd, hd = (torch.from_numpy(a).cuda() for a in (x, scale, shift))
    # strided output rows: 2 pad rows ahead of each utterance's T rows, as in frame1's input
    y = torch.zeros((B, T + 2, C), device="cuda")
    nv.check(nv.lib.lidbox_bn_relu_maxf_fwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), ctypes.c_void_p(y.data_ptr() + 8 * C),
                                            (T + 2) * C, st))
    dyd = torch.zeros((B, T + 2, C), device="cuda")
    dyd[:, 2:] = torch.from_numpy(dy).cuda()
    dv = torch.full((B, T, F, C), 7.0, device="cuda")
    nv.check(nv.lib.lidbox_bn_relu_maxf_bwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), ctypes.c_void_p(dyd.data_ptr() + 8 * C),
                                            (T + 2) * C, nv.ptr(dv), st))
    torch.cuda.synchronize()
    y, dv = y.cpu().numpy(), dv.cpu().numpy()
    assert np.all(y[:, :2] == 0)
    assert np.abs(y[:, 2:] - yr).max() <= 1e-6
    assert np.abs(dv - dvr).max() <= 1e-6
    assert dv[0, 0, 1, 0] == dv[0, 0, 3, 0] == np.float32(0.5) * dy[0, 0, 0]
    assert np.all(dv[1, 2, :, 1] == 0)
    assert dv[2, 4, 0, 2] == np.float32(1.0 / 3.0) * dy[2, 4, 2] and dv[2, 4, 1, 2] == 0
    # BN-apply + ReLU and its backward
    R = B * T * F
    a = torch.zeros_like(xd)
    nv.check(nv.lib.lidbox_bn_relu_fwd(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), nv.ptr(a), st))
    g = torch.from_numpy(rng.standard_normal((B, T, F, C)).astype(np.float32)).cuda()
    dg = g.clone()
    nv.check(nv.lib.lidbox_bn_relu_bwd(nv.ptr(xd), R, C, nv.ptr(sd), nv.ptr(hd), nv.ptr(dg), nv.ptr(dg), st))
    torch.cuda.synchronize()
    v = torch.addcmul(hd, xd, sd)
    assert torch.allclose(a, torch.relu(v), atol=1e-6, rtol=0)
    assert torch.equal(dg, torch.where(v > 0, g, torch.zeros_like(g)))
