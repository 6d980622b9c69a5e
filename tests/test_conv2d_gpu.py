"""
GPU tests of csrc/conv2d.hip through the C ABI against float64 torch on the CPU: Conv2D(padding="same") forward, dgrad,
wgrad and bias grad at the five crnn block shapes, BatchNormalization-apply + MaxPool2D forward / backward (first-maximum
tie rule, dropped odd cells), and the L2 kernel penalty.  Images are stored time-major [B, T, F, C]; the oracle works on the
reference's image orientation [B, C, F, T] (height = frequency), so a transposition of the kernel's two axes is caught by the
non-square inputs.

Tolerances: the conv results are exact fp32 MFMA sums of up to 2304 products, so their relative L2 error against float64 is
of the order of 1e-7; the bound is 1e-5.  Pooling compares exactly: its inputs are integers scaled exactly in fp32.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

REL = 1e-5
SHAPES = [(7, 1, 16), (5, 16, 32), (3, 32, 64), (3, 64, 128), (3, 128, 256)]     # (k, C_in, C_out) of crnn.py's blocks


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _img(x):
    """[B, T, F, C] -> the reference image [B, C, F, T] (float64 torch)"""
    return torch.from_numpy(np.asarray(x, np.float64)).permute(0, 3, 2, 1)


def _unimg(t):
    return t.permute(0, 3, 2, 1).detach().numpy()


def _oracle(x, W, b, dy):
    """relu(conv) forward, and for the loss sum(conv(x) * dy) (no ReLU): dx, dW, db -- in this build's layouts"""
    k = W.shape[0]
    xi = _img(x).requires_grad_(True)
    Wt = torch.from_numpy(W.astype(np.float64)).permute(3, 2, 0, 1).contiguous().requires_grad_(True)   # [co, ci, kh, kw]
    bt = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    z = Fn.conv2d(xi, Wt, bt, padding=(k - 1) // 2)
    (z * _img(dy)).sum().backward()
    return (_unimg(torch.relu(z)), _unimg(xi.grad), Wt.grad.permute(2, 3, 1, 0).numpy(), bt.grad.numpy())


def _data(rng, B, T, F, k, cin, cout):
    x = rng.standard_normal((B, T, F, cin)).astype(np.float32)
    lim = np.sqrt(6.0 / (k * k * (cin + cout)))
    W = rng.uniform(-lim, lim, (k, k, cin, cout)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    dy = rng.standard_normal((B, T, F, cout)).astype(np.float32)
    return x, W, b, dy


def _run(x, W, b, dy, want_dgrad=True):
    nv = _nv()
    B, T, F, cin = x.shape
    k, cout = W.shape[0], W.shape[3]
    xd, Wd, bd, dyd = (torch.from_numpy(a).cuda() for a in (x, W, b, dy))
    y = torch.empty((B, T, F, cout), device="cuda")
    st = nv.current_stream()
    nv.check(nv.lib.lidbox_conv2d_fwd(nv.ptr(xd), B, T, F, cin, nv.ptr(Wd), k, cout, nv.ptr(bd), 1, nv.ptr(y), st))
    dx = None
    if want_dgrad:
        dx = torch.empty_like(xd)
        ws = torch.empty(nv.lib.lidbox_conv2d_dgrad_workspace(k, cin, cout), dtype=torch.uint8, device="cuda")
        nv.check(nv.lib.lidbox_conv2d_dgrad(nv.ptr(dyd), B, T, F, cin, cout, nv.ptr(Wd), k, nv.ptr(dx), nv.ptr(ws), ws.numel(), st))
    dW = torch.full_like(Wd, float("nan"))
    db = torch.full_like(bd, float("nan"))
    ws = torch.empty(max(16, nv.lib.lidbox_conv2d_wgrad_workspace(B, T, F, cin, cout, k)), dtype=torch.uint8, device="cuda")
    nv.check(nv.lib.lidbox_conv2d_wgrad(nv.ptr(xd), nv.ptr(dyd), B, T, F, cin, cout, k, nv.ptr(dW), nv.ptr(db), nv.ptr(ws),
                                        ws.numel(), st))
    torch.cuda.synchronize()
    return y.cpu().numpy(), None if dx is None else dx.cpu().numpy(), dW.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize("k,cin,cout", SHAPES)
@pytest.mark.parametrize("B,T,F", [(2, 13, 11), (1, 9, 16)])
def test_conv2d_matches_torch(k, cin, cout, B, T, F):
    rng = np.random.default_rng(k * 1000 + cin + B)
    x, W, b, dy = _data(rng, B, T, F, k, cin, cout)
    y, dx, dW, db = _run(x, W, b, dy, want_dgrad=cin % 16 == 0)
    ry, rdx, rdW, rdb = _oracle(x, W, b, dy)
    assert _rel(y, ry) <= REL, _rel(y, ry)
    if dx is not None:
        assert _rel(dx, rdx) <= REL, _rel(dx, rdx)
    assert _rel(dW, rdW) <= REL, _rel(dW, rdW)
    assert _rel(db, rdb) <= REL, _rel(db, rdb)


def test_conv2d_asymmetric_kernel_orientation():
    """a kernel that only looks one frequency bin up: catches a swapped (frequency, time) kernel index"""
    rng = np.random.default_rng(5)
    x, W, b, dy = _data(rng, 2, 10, 7, 3, 16, 16)
    W[:] = 0
    W[2, 1] = rng.standard_normal((16, 16)).astype(np.float32)       # kh = 2: frequency + 1, kw = 1: same frame
    y, dx, dW, db = _run(x, W, b, dy)
    ry, rdx, rdW, _ = _oracle(x, W, b, dy)
    assert _rel(y, ry) <= REL and _rel(dx, rdx) <= REL and _rel(dW, rdW) <= REL
    pre = np.einsum("btfc,cd->btfd", x[:, :, 1:, :].astype(np.float64), W[2, 1].astype(np.float64)) + b
    assert np.allclose(y[:, :, :-1], np.maximum(pre, 0), atol=1e-5)


def test_conv2d_utterance_bits_independent_of_batch():
    rng = np.random.default_rng(6)
    for k, cin, cout in SHAPES[:3]:
        x, W, b, dy = _data(rng, 5, 12, 10, k, cin, cout)
        y = _run(x, W, b, dy, want_dgrad=False)[0]
        y1 = _run(x[3:4].copy(), W, b, dy[3:4].copy(), want_dgrad=False)[0]
        assert np.array_equal(y[3:4], y1)


def test_conv2d_wgrad_deterministic():
    rng = np.random.default_rng(7)
    x, W, b, dy = _data(rng, 4, 33, 21, 5, 16, 32)
    a = _run(x, W, b, dy)
    c = _run(x, W, b, dy)
    for u, v in zip(a, c):
        assert np.array_equal(u, v)


def test_conv2d_wgrad_many_partitions():
    """block 1's shape at 36 864 pixels: wgrad splits them into P >= 64 partitions, whose partials are summed one wave per
    output (the path the full-size blocks 1-3 take)"""
    nv = _nv()
    B, T, F, k, cin, cout = 16, 48, 48, 7, 1, 16
    assert nv.lib.lidbox_conv2d_wgrad_workspace(B, T, F, cin, cout, k) >= 64 * (k * k * cin * cout + cout) * 4
    rng = np.random.default_rng(10)
    x, W, b, dy = _data(rng, B, T, F, k, cin, cout)
    a = _run(x, W, b, dy, want_dgrad=False)
    _, _, rdW, rdb = _oracle(x, W, b, dy)
    assert _rel(a[2], rdW) <= REL, _rel(a[2], rdW)
    assert _rel(a[3], rdb) <= REL, _rel(a[3], rdb)
    c = _run(x, W, b, dy, want_dgrad=False)
    assert np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])


# ---------------------------------------------------------------------------------------------------- BN-apply + MaxPool2D
def _pool(x, scale, shift, dp):
    nv = _nv()
    B, T, F, C = x.shape
    xd, sd, hd, dpd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, scale, shift, dp))
    y = torch.empty((B, T // 2, F // 2, C), device="cuda")
    code = torch.empty((B, T // 2, F // 2, C), dtype=torch.uint8, device="cuda")
    dx = torch.full_like(xd, float("nan"))
    st = nv.current_stream()
    nv.check(nv.lib.lidbox_bn_maxpool2d_fwd(nv.ptr(xd), B, T, F, C, nv.ptr(sd), nv.ptr(hd), nv.ptr(y), nv.ptr(code), st))
    nv.check(nv.lib.lidbox_maxpool2d_bwd(nv.ptr(dpd), nv.ptr(code), B, T, F, C, nv.ptr(dx), st))
    torch.cuda.synchronize()
    return y.cpu().numpy(), code.cpu().numpy(), dx.cpu().numpy()


def _pool_oracle(x, scale, shift, dp):
    v = _img(x.astype(np.float64) * scale + shift).requires_grad_(True)
    y, idx = Fn.max_pool2d(v, 2, return_indices=True)
    (y * _img(dp)).sum().backward()
    Wd = v.shape[3]
    code = 2 * ((idx // Wd) % 2) + (idx % Wd) % 2              # 2 * dfreq + dtime of torch's first-maximum winner
    return _unimg(y), _unimg(code), _unimg(v.grad)


@pytest.mark.parametrize("B,T,F,C", [(2, 13, 11, 16), (1, 8, 6, 32), (3, 7, 9, 48)])
def test_bn_maxpool_matches_torch_distinct_values(B, T, F, C):
    rng = np.random.default_rng(T * F + C)
    n = B * T * F * C
    x = (rng.permutation(n) - n // 2).astype(np.float32).reshape(B, T, F, C)          # distinct integers
    scale = rng.choice(np.array([1.0, -1.0, 2.0, -0.5], np.float32), C)             # negative gamma flips the maximum
    shift = rng.integers(-3, 4, C).astype(np.float32)
    dp = rng.standard_normal((B, T // 2, F // 2, C)).astype(np.float32)
    y, code, dx = _pool(x, scale, shift, dp)
    ry, rcode, rdx = _pool_oracle(x, scale, shift, dp)
    assert np.array_equal(y, ry.astype(np.float32))
    assert np.array_equal(code, rcode)
    assert np.array_equal(dx, rdx.astype(np.float32))
    if T % 2:
        assert not dx[:, -1].any()                    # the dropped last frame gets zero gradient
    if F % 2:
        assert not dx[:, :, -1].any()


def test_bn_maxpool_ties_take_first_maximum():
    rng = np.random.default_rng(8)
    B, T, F, C = 2, 9, 7, 16
    x = np.full((B, T, F, C), 3.0, np.float32)                      # a constant plane: every window is a four-way tie
    x[1] = np.maximum(rng.integers(-2, 3, (T, F, C)), 0).astype(np.float32)        # ReLU zeros: many partial ties
    scale = np.where(np.arange(C) % 2, -1.0, 1.0).astype(np.float32)
    shift = np.zeros(C, np.float32)
    dp = rng.standard_normal((B, T // 2, F // 2, C)).astype(np.float32)
    y, code, dx = _pool(x, scale, shift, dp)
    ry, rcode, rdx = _pool_oracle(x, scale, shift, dp)
    assert (code[0] == 0).all()                                    # (lowest frequency, earliest frame) wins
    assert np.array_equal(code, rcode) and np.array_equal(y, ry.astype(np.float32))
    assert np.array_equal(dx, rdx.astype(np.float32))
    # a tie between the two frames of the lower frequency row and nothing else: the earlier frame (code 0) wins,
    # a tie between the two frequency rows at the later frame only: the lower row (code 1) wins
    x2 = np.zeros((1, 2, 2, 16), np.float32)
    x2[0, :, 0, :] = 5.0
    assert (_pool(x2, np.ones(16, np.float32), shift, np.ones((1, 1, 1, 16), np.float32))[1] == 0).all()
    x3 = np.zeros((1, 2, 2, 16), np.float32)
    x3[0, 1, :, :] = 5.0
    assert (_pool(x3, np.ones(16, np.float32), shift, np.ones((1, 1, 1, 16), np.float32))[1] == 1).all()


# ---------------------------------------------------------------------------------------------------- L2 penalty
def test_l2_penalty_loss_and_gradient():
    import ctypes
    nv = _nv()
    rng = np.random.default_rng(9)
    flat = rng.standard_normal(5000).astype(np.float32)
    grad = rng.standard_normal(5000).astype(np.float32)
    offs, sizes, lams = [0, 1000, 3000], [784, 1500, 2000], [1e-3, 2e-3, 5e-4]
    fd, gd = torch.from_numpy(flat).cuda(), torch.from_numpy(grad).cuda()
    loss = torch.tensor([0.25], device="cuda")
    ws = torch.empty(nv.lib.lidbox_l2_penalty_workspace(), dtype=torch.uint8, device="cuda")
    n = len(offs)
    nv.check(nv.lib.lidbox_l2_penalty(nv.ptr(fd), nv.ptr(gd), n, (ctypes.c_long * n)(*offs), (ctypes.c_long * n)(*sizes),
                                      (ctypes.c_float * n)(*lams), 0.5, nv.ptr(loss), nv.ptr(ws), ws.numel(),
                                      nv.current_stream()))
    torch.cuda.synchronize()
    want_g = grad.astype(np.float64).copy()
    want_l = 0.25
    for o, s, lam in zip(offs, sizes, lams):
        w = flat[o:o + s].astype(np.float64)
        want_g[o:o + s] += 2 * lam * 0.5 * w
        want_l += lam * (w * w).sum()
    assert np.allclose(gd.cpu().numpy(), want_g, rtol=1e-6, atol=1e-7)
    assert abs(float(loss) - want_l) <= 1e-6 * want_l
    untouched = np.ones(5000, bool)
    for o, s in zip(offs, sizes):
        untouched[o:o + s] = False
    assert np.array_equal(gd.cpu().numpy()[untouched], grad[untouched])
    # loss only (what evaluate uses)
    loss.zero_()
    nv.check(nv.lib.lidbox_l2_penalty(nv.ptr(fd), None, n, (ctypes.c_long * n)(*offs), (ctypes.c_long * n)(*sizes),
                                      (ctypes.c_float * n)(*lams), 1.0, nv.ptr(loss), nv.ptr(ws), ws.numel(),
                                      nv.current_stream()))
    torch.cuda.synchronize()
    assert abs(float(loss) - (want_l - 0.25)) <= 1e-6 * want_l
