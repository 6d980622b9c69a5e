"""
GPU tests of csrc/mla.hip: the attention pooling of the multi-level attention classifier (lidbox_mla_attention_fwd / _bwd)
against a float64 torch restatement of reference lidbox/models/multilevel_attention.py:26-33 written below, and the fused
BatchNormalization-apply + ReLU + Dropout pass (lidbox_bn_relu_dropout_fwd / _bwd) against the two-call compositions it
replaces, bit for bit.

Attention inputs are standard normal with planted clip cases: every third row (of the B*T rows) gets two entries at -30, so
the lower clip bound is hit firmly, and every fifth row one entry at +30, so the upper bound is hit and the rest of that row
falls below the lower one.  The float64 reference asserts that no probability lies near a bound, so the pass mask is the same
in both precisions and no element is left out of the comparison: no p within relative 1e-3 of lo, and no 1 - p between a
quarter of and four times 1 - hi.  The upper bound is measured on 1 - p because hi = 1 - 2^-23: a relative band around hi on p
itself would hold every probability clipped from above (p = 1 for K = 1), and it is a factor of 4 rather than 1e-3 wide because
float32 numbers below 1 are 2^-24 apart, half of 1 - hi.

Tolerances: H_TOL = 5e-5 absolute on att, G_TOL = 1e-4 relative L2 on dz (tests/test_lstm_step_gpu.py).  float32 torch on
the CPU is within 2.0e-7 / 2.6e-7 of float64 on these inputs.  Measured maxima over the five shapes (MI355X):
2.8e-7 on att ((4, 198, 100)), 2.7e-7 on dz (same shape); 9.3e-14 and 5.1e-8 at (1, 1, 3), whose dz is of size 1e-13.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H_TOL = 5e-5
G_TOL = 1e-4
LO = float(np.float32(1e-7))
HI = float(np.float32(1 - 1e-7))
SHAPES = [(3, 17, 5), (4, 198, 100), (2, 10, 527), (2, 9, 1), (1, 1, 3)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _inputs(B, T, K, rng):
    z = rng.standard_normal((B * T, K)).astype(np.float32)
    for r in range(0, B * T, 3):
        z[r, r % K] = -30.0
        z[r, (r + 1) % K] = -30.0
    for r in range(0, B * T, 5):
        z[r, (r + 2) % K] = 30.0
    return z.reshape(B, T, K), rng.standard_normal((B, K)).astype(np.float32)


def _reference(z, g):
    """float64: (att, dz, share of clipped elements); asserts that no probability is near a clip bound (module docstring)"""
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    p = torch.softmax(zt, -1)
    pn = p.detach().numpy()
    band = (np.abs(pn - LO) <= 1e-3 * LO) | ((1 - pn >= (1 - HI) / 4) & (1 - pn <= 4 * (1 - HI)))
    assert not band.any(), "%d probabilities near a clip bound" % int(band.sum())
    c = torch.clamp(p, LO, HI)
    q = c / c.sum(1, keepdim=True)
    # sigmoid written out: autograd's torch.sigmoid backward is v (1 - v), which at z = 30 keeps 3 digits even in float64
    att = (q / (1 + torch.exp(-zt))).sum(1)
    (att * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return att.detach().numpy(), zt.grad.numpy(), float(((pn < LO) | (pn > HI)).mean())


def _attention(z, g, ld_att=None, col=0, att_buf=None, datt_buf=None):
    """runs forward and backward on the device; att / datt live at column `col` of buffers with row stride ld_att"""
    from lidbox_amd import _native as nv
    B, T, K = z.shape
    st = nv.current_stream()
    zd = torch.from_numpy(z).cuda()
    ld = ld_att or K
    att = att_buf if att_buf is not None else torch.zeros((B, ld), device="cuda")
    datt = datt_buf if datt_buf is not None else torch.zeros((B, ld), device="cuda")
    datt[:B, col:col + K] = torch.from_numpy(g).cuda()
    colsum = torch.zeros((B, K), device="cuda")
    dz = torch.zeros((B, T, K), device="cuda")
    nv.check(nv.lib.lidbox_mla_attention_fwd(nv.ptr(zd), B, T, K, ctypes.c_void_p(att.data_ptr() + 4 * col), ld, nv.ptr(colsum), st))
    nv.check(nv.lib.lidbox_mla_attention_bwd(nv.ptr(zd), ctypes.c_void_p(att.data_ptr() + 4 * col), ld, nv.ptr(colsum),
                                             ctypes.c_void_p(datt.data_ptr() + 4 * col), ld, B, T, K, nv.ptr(dz), st))
    torch.cuda.synchronize()
    return att[:B, col:col + K].cpu().numpy(), dz.cpu().numpy(), colsum.cpu().numpy()


@pytest.mark.parametrize("B,T,K", SHAPES)
def test_attention_forward_backward_match_float64(B, T, K):
    z, g = _inputs(B, T, K, np.random.default_rng(7))
    att_ref, dz_ref, clipped = _reference(z, g)
    att, dz, colsum = _attention(z, g)
    e_att, e_dz = float(np.abs(att - att_ref).max()), _rel(dz, dz_ref)
    print("mla attention (B, T, K) = (%d, %d, %d): %.1f %% clipped, |att - ref| = %.3e, rel L2 dz = %.3e"
          % (B, T, K, 100 * clipped, e_att, e_dz))
    assert clipped > 0.15
    assert np.isfinite(att).all() and np.isfinite(dz).all()
    assert e_att <= H_TOL
    assert e_dz <= G_TOL
    p = torch.softmax(torch.from_numpy(z.astype(np.float64)), -1).clamp(LO, HI).sum(1).numpy()
    assert np.abs(colsum - p).max() <= H_TOL * max(1.0, float(p.max()))


def test_attention_strides_leave_other_columns_alone():
    """two levels write column slices of one [B, 2K] buffer; a guard row behind it stays as it was"""
    rng = np.random.default_rng(8)
    B, T, K = 5, 23, 12
    z1, g1 = _inputs(B, T, K, rng)
    z2, g2 = _inputs(B, T, K, rng)
    dense1, dense2 = _attention(z1, g1), _attention(z2, g2)
    att = torch.full((B + 1, 2 * K), 777.0, device="cuda")
    datt = torch.full((B + 1, 2 * K), 555.0, device="cuda")
    a1, dz1, _ = _attention(z1, g1, ld_att=2 * K, col=0, att_buf=att, datt_buf=datt)
    assert (att[:B, K:] == 777.0).all() and (att[B] == 777.0).all()
    a2, dz2, _ = _attention(z2, g2, ld_att=2 * K, col=K, att_buf=att, datt_buf=datt)
    assert (att[B] == 777.0).all() and (datt[B] == 555.0).all()
    both = att[:B].cpu().numpy()
    assert np.array_equal(both[:, :K], dense1[0]) and np.array_equal(both[:, K:], dense2[0])
    assert np.array_equal(a1, dense1[0]) and np.array_equal(a2, dense2[0])
    assert np.array_equal(dz1, dense1[1]) and np.array_equal(dz2, dense2[1])          # datt read through ld_datt


@pytest.mark.parametrize("T,K", [(17, 5), (198, 100), (10, 527), (9, 1), (33, 64)])
def test_attention_rows_do_not_depend_on_the_batch(T, K):
    rng = np.random.default_rng(9)
    z1, g1 = _inputs(1, T, K, rng)
    alone = _attention(z1, g1)
    for B in (2, 7, 256):
        z, g = _inputs(B, T, K, rng)
        for pos in sorted({0, B // 2, B - 1}):
            z[pos], g[pos] = z1[0], g1[0]
        att, dz, colsum = _attention(z, g)
        for pos in sorted({0, B // 2, B - 1}):
            assert np.array_equal(att[pos], alone[0][0]), (B, pos)
            assert np.array_equal(dz[pos], alone[1][0]), (B, pos)
            assert np.array_equal(colsum[pos], alone[2][0]), (B, pos)


@pytest.mark.parametrize("B,T,K", [(4, 198, 100), (3, 17, 5)])
def test_attention_is_deterministic(B, T, K):
    z, g = _inputs(B, T, K, np.random.default_rng(10))
    a, b = _attention(z, g), _attention(z, g)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_attention_unaligned_base_takes_the_scalar_path():
    """K % 4 == 0 but z and dz start 4 bytes off a 16-byte boundary: the scalar kernels run, nothing in front of the buffers
    is touched, and the values agree with the aligned call to a few float32 roundings (att lies in [0, 1] and is a sum of 21
    terms; the other lane layout sums them in another order)"""
    from lidbox_amd import _native as nv
    B, T, K = 3, 21, 8
    z, g = _inputs(B, T, K, np.random.default_rng(11))
    want = _attention(z, g)
    st = nv.current_stream()
    zbuf = torch.zeros(B * T * K + 1, device="cuda")
    zbuf[1:] = torch.from_numpy(z).cuda().reshape(-1)
    dzbuf = torch.zeros(B * T * K + 1, device="cuda")
    att, colsum, datt = torch.zeros((B, K), device="cuda"), torch.zeros((B, K), device="cuda"), torch.from_numpy(g).cuda()
    nv.check(nv.lib.lidbox_mla_attention_fwd(ctypes.c_void_p(zbuf.data_ptr() + 4), B, T, K, nv.ptr(att), K, nv.ptr(colsum), st))
    nv.check(nv.lib.lidbox_mla_attention_bwd(ctypes.c_void_p(zbuf.data_ptr() + 4), nv.ptr(att), K, nv.ptr(colsum), nv.ptr(datt), K,
                                             B, T, K, ctypes.c_void_p(dzbuf.data_ptr() + 4), st))
    torch.cuda.synchronize()
    assert float(dzbuf[0]) == 0.0
    assert np.abs(att.cpu().numpy() - want[0]).max() <= 1e-6            # another lane layout: another summation order
    assert _rel(dzbuf[1:].cpu().numpy().reshape(B, T, K), want[1]) <= 1e-6


def test_attention_refusals_and_empty_batch():
    from lidbox_amd import _native as nv
    lib, st = nv.lib, nv.current_stream()
    buf = torch.full((64,), 3.0, device="cuda")
    p = nv.ptr(buf)
    assert lib.lidbox_mla_attention_fwd(p, 0, 3, 4, p, 4, p, st) == 0
    assert lib.lidbox_mla_attention_bwd(p, p, 4, p, p, 4, 0, 3, 4, p, st) == 0
    torch.cuda.synchronize()
    assert (buf == 3.0).all()
    for args in ((None, 2, 3, 4, p, 4, p), (p, 2, 3, 4, None, 4, p), (p, 2, 3, 4, p, 4, None), (p, 2, 0, 4, p, 4, p),
                 (p, 2, 3, 0, p, 4, p), (p, 2, -1, 4, p, 4, p), (p, 2, 3, -2, p, 4, p)):
        assert lib.lidbox_mla_attention_fwd(*args, st) == -1, args
        assert "lidbox_mla_attention_fwd" in nv.last_error()
    for args in ((None, p, 4, p, p, 4, 2, 3, 4, p), (p, None, 4, p, p, 4, 2, 3, 4, p), (p, p, 4, None, p, 4, 2, 3, 4, p),
                 (p, p, 4, p, None, 4, 2, 3, 4, p), (p, p, 4, p, p, 4, 2, 3, 4, None), (p, p, 4, p, p, 4, 2, 0, 4, p),
                 (p, p, 4, p, p, 4, 2, 3, 0, p)):
        assert lib.lidbox_mla_attention_bwd(*args, st) == -1, args
        assert "lidbox_mla_attention_bwd" in nv.last_error()
    with pytest.raises(ValueError):
        nv.check(lib.lidbox_mla_attention_fwd(p, 2, 0, 4, p, 4, p, st))
    torch.cuda.synchronize()
    assert (buf == 3.0).all()


# ---------------------------------------------------------------------------------------------------- fused pass
def _fused_case(R, C, rng):
    x = torch.from_numpy(rng.standard_normal((R, C)).astype(np.float32)).cuda()
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)).cuda()
    shift = torch.from_numpy((0.3 * rng.standard_normal(C)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.standard_normal((R, C)).astype(np.float32)).cuda()
    return x, scale, shift, dy


def _composed(x, scale, shift, dy, rate, seed, step):
    from lidbox_amd import _native as nv
    from lidbox_amd.models.tdnn import _rows
    R, C = x.shape
    st = nv.current_stream()
    y = torch.empty_like(x)
    nv.check(nv.lib.lidbox_bn_relu_fwd(nv.ptr(x), R, C, nv.ptr(scale), nv.ptr(shift), nv.ptr(y), st))
    nv.check(nv.lib.lidbox_dropout_rows(_rows(y.data_ptr(), 0, C, 1, R), C, rate, seed, nv.ptr(step), st))
    g = dy.clone()
    dx = torch.empty_like(x)
    nv.check(nv.lib.lidbox_dropout_rows(_rows(g.data_ptr(), 0, C, 1, R), C, rate, seed, nv.ptr(step), st))
    nv.check(nv.lib.lidbox_bn_relu_bwd(nv.ptr(x), R, C, nv.ptr(scale), nv.ptr(shift), nv.ptr(g), nv.ptr(dx), st))
    return y, dx


def _fused(x, scale, shift, dy, rate, seed, step, in_place=False):
    from lidbox_amd import _native as nv
    R, C = x.shape
    st = nv.current_stream()
    y = torch.empty_like(x)
    nv.check(nv.lib.lidbox_bn_relu_dropout_fwd(nv.ptr(x), R, C, nv.ptr(scale), nv.ptr(shift), rate, seed, nv.ptr(step), nv.ptr(y), st))
    g = dy.clone()
    dx = g if in_place else torch.empty_like(x)
    nv.check(nv.lib.lidbox_bn_relu_dropout_bwd(nv.ptr(x), R, C, nv.ptr(scale), nv.ptr(shift), rate, seed, nv.ptr(step), nv.ptr(g),
                                               nv.ptr(dx), st))
    return y, dx


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("R,C", [(30, 7), (1000, 512), (50688, 512)])
@pytest.mark.parametrize("rate", [0.4, 0.0])
def test_fused_pass_equals_the_two_call_compositions_bit_for_bit(R, C, rate):
    rng = np.random.default_rng(R + C)
    x, scale, shift, dy = _fused_case(R, C, rng)
    seed = 0x1234567887654321
    for step in (None, torch.tensor([12345], dtype=torch.int64, device="cuda")):
        y0, dx0 = _composed(x, scale, shift, dy, rate, seed, step)
        y1, dx1 = _fused(x, scale, shift, dy, rate, seed, step)
        _, dx2 = _fused(x, scale, shift, dy, rate, seed, step, in_place=True)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y0), _bits(y1))
        assert torch.equal(_bits(dx0), _bits(dx1))
        assert torch.equal(_bits(dx0), _bits(dx2))
    if rate == 0.0:
        from lidbox_amd import _native as nv
        y = torch.empty_like(x)
        nv.check(nv.lib.lidbox_bn_relu_fwd(nv.ptr(x), R, C, nv.ptr(scale), nv.ptr(shift), nv.ptr(y), nv.current_stream()))
        assert torch.equal(_bits(y), _bits(y1))


def test_fused_pass_unaligned_pointers_take_the_scalar_path():
    """C % 4 == 0 with x and y four bytes off a 16-byte boundary: still the composition's bits"""
    from lidbox_amd import _native as nv
    rng = np.random.default_rng(3)
    R, C = 40, 16
    x, scale, shift, dy = _fused_case(R, C, rng)
    y0, _ = _composed(x, scale, shift, dy, 0.4, 99, None)
    xb = torch.zeros(R * C + 1, device="cuda")
    xb[1:] = x.reshape(-1)
    yb = torch.zeros(R * C + 1, device="cuda")
    nv.check(nv.lib.lidbox_bn_relu_dropout_fwd(ctypes.c_void_p(xb.data_ptr() + 4), R, C, nv.ptr(scale), nv.ptr(shift), 0.4, 99, None,
                                               ctypes.c_void_p(yb.data_ptr() + 4), nv.current_stream()))
    torch.cuda.synchronize()
    assert float(yb[0]) == 0.0 and torch.equal(_bits(yb[1:].reshape(R, C)), _bits(y0))


def test_fused_pass_masks_follow_seed_and_step_and_keep_the_right_share():
    R, C, rate = 1000, 512, 0.4
    ones = torch.ones((R, C), device="cuda")
    scale, shift = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    step1 = torch.tensor([1], dtype=torch.int64, device="cuda")
    step2 = torch.tensor([2], dtype=torch.int64, device="cuda")
    masks = {}
    for tag, seed, step in (("a", 5, step1), ("a2", 5, step1), ("step", 5, step2), ("seed", 6, step1), ("null", 5, None)):
        masks[tag], _ = _fused(ones, scale, shift, ones, rate, seed, step)
    torch.cuda.synchronize()
    assert torch.equal(masks["a"], masks["a2"])
    n = R * C
    bound = 5 * np.sqrt(rate * (1 - rate) / n)            # 5 standard deviations of a binomial share
    for tag, m in masks.items():
        kept = float((m != 0).double().mean())
        assert abs(kept - (1 - rate)) <= bound, (tag, kept)
        vals = torch.unique(m).cpu().numpy()
        assert np.array_equal(vals, np.array([0.0, np.float32(1.0) / (np.float32(1.0) - np.float32(rate))], np.float32)), tag
    for tag in ("step", "seed", "null"):
        differ = float(((masks["a"] != 0) != (masks[tag] != 0)).double().mean())
        assert abs(differ - 2 * rate * (1 - rate)) <= 2 * bound, (tag, differ)       # independent masks differ at 2 r (1 - r)
