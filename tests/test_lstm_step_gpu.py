"""
GPU tests of the fused LSTM step kernels (csrc/lstm_step.hip: lidbox_lstm_step_fwd / _bwd) against a float64 torch.nn.LSTM
oracle on the CPU, set up as in tests/test_rnn_gpu.py (gate order i, f, g, o as Keras; weight_ih = W^T, weight_hh = U^T,
bias_ih = b, bias_hh = 0).  The input projection and the weight gradients are computed in float64 on the host, so what is
compared is the walk through time.

Tolerances: H_TOL = 5e-5 absolute on h and G_TOL = 1e-4 relative L2 on gradients, the project's bounds for this math against
this oracle (tests/test_rnn_gpu.py, tests/test_gru_gpu.py).  First measured maxima of these kernels (MI355X): over
LAYER_CASES (H in {1, 10, 81, 100, 250, 251, 1024}, T up to 198, B up to 256) 1.8e-7 absolute on h and 3.3e-7 relative L2 on
dX, dW, dU and db; over every test of this file 1.8e-7 and 9.6e-7 (dU of the H = 1 column-slice case, a gradient of four
numbers); against the stepped form at H = 250 1.2e-7 and 1.6e-7.  The bounds keep a margin of more than 100x.
H = 260 (4H = 1040) leaves backward's K a full LDS chunk and a 16-long tail; the scalar paths that only misaligned buffers
select at H % 4 == 0 are compared bit for bit with the float4 paths.  Both hold the same bounds.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H_TOL = 5e-5
G_TOL = 1e-4


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _params(rng, C, H, dirs):
    from lidbox_amd.models.rnn import orthogonal
    out = []
    for _ in range(dirs):
        lim = math.sqrt(6.0 / (C + 4 * H))
        W = rng.uniform(-lim, lim, (C, 4 * H)).astype(np.float32)
        U = np.ascontiguousarray(orthogonal((H, 4 * H), rng), dtype=np.float32)
        b = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
        b[H:2 * H] += 1.0
        out.append((W, U, b))
    return out


def _oracle(params, x, dh_seq=None, dh_last=None):
    """float64 torch.nn.LSTM: output sequence, dX and (dW, dU, db) per direction for the loss sum(out * dh_seq) +
    sum(final h * dh_last) (final h: t = T-1 forward, t = 0 reverse)"""
    B, T, C = x.shape
    dirs = len(params)
    H = params[0][1].shape[0]
    m = torch.nn.LSTM(C, H, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for d, (W, U, b) in enumerate(params):
            sfx = "_l0" + ("_reverse" if d else "")
            getattr(m, "weight_ih" + sfx).copy_(torch.from_numpy(W.T.astype(np.float64)))
            getattr(m, "weight_hh" + sfx).copy_(torch.from_numpy(U.T.astype(np.float64)))
            getattr(m, "bias_ih" + sfx).copy_(torch.from_numpy(b.astype(np.float64)))
            getattr(m, "bias_hh" + sfx).zero_()
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y, _ = m(xt)
    loss = 0.0
    if dh_seq is not None:
        loss = loss + (y * torch.from_numpy(dh_seq.astype(np.float64))).sum()
    if dh_last is not None:
        dl = torch.from_numpy(dh_last.astype(np.float64))
        loss = loss + (y[:, -1, :H] * dl[:, :H]).sum()
        if dirs == 2:
            loss = loss + (y[:, 0, H:] * dl[:, H:]).sum()
    loss.backward()
    grads = []
    for d in range(dirs):
        sfx = "_l0" + ("_reverse" if d else "")
        grads.append((getattr(m, "weight_ih" + sfx).grad.numpy().T, getattr(m, "weight_hh" + sfx).grad.numpy().T,
                      getattr(m, "bias_ih" + sfx).grad.numpy()))
    return y.detach().numpy(), xt.grad.numpy(), grads


SENTINEL = 12345.5


def _run_layer(params, x, dh_seq=None, dh_last=None, wide=1, col=0, stepped=False, misalign=False):
    """the recurrence through the C ABI.  wide / col: hseq and dh_seq rows are wide * dirs*H floats, the layer at column
    offset col, every other column pre-filled with SENTINEL (and checked afterwards).  stepped: lidbox_lstm_fwd / _bwd
    (dense strides only) instead of the fused step.  misalign: U of every direction and zg are not 16-byte aligned, which
    selects the scalar load paths whatever H is.  Returns h [B, T, dirs*H], dZ [dirs, B, T, 4H], hseq's slice
    [B, T+2, dirs*H]."""
    from lidbox_amd.testutil import device_copy
    nv = _nv()
    B, T, C = x.shape
    dirs = len(params)
    H = params[0][1].shape[0]
    D = dirs * H
    rs = wide * D
    dev = torch.device("cuda")
    zg = np.stack([(x.astype(np.float64) @ W.astype(np.float64) + b).astype(np.float32) for W, _, b in params])
    zg_d = device_copy(zg, misalign)
    hbuf = torch.full((B, T + 2, rs), SENTINEL, dtype=torch.float32, device=dev)
    hbuf[:, :, col:col + D] = 0.0
    cseq = torch.zeros((dirs, B, T, H), dtype=torch.float32, device=dev)
    Us = [device_copy(U, misalign) for _, U, _ in params]
    U1 = nv.ptr(Us[1]) if dirs == 2 else None
    st = nv.current_stream()
    dbuf = None
    if dh_seq is not None:
        dbuf = torch.full((B, T, rs), SENTINEL, dtype=torch.float32, device=dev)
        dbuf[:, :, col:col + D] = torch.from_numpy(dh_seq).to(dev)
    dla = None if dh_last is None else torch.from_numpy(dh_last).to(dev).contiguous()
    hp = ctypes.c_void_p(hbuf.data_ptr() + 4 * col)
    dp = None if dbuf is None else ctypes.c_void_p(dbuf.data_ptr() + 4 * col)
    if stepped:
        assert wide == 1 and col == 0
        ws = torch.empty(max(16, nv.lib.lidbox_lstm_workspace(B, T, H, dirs)), dtype=torch.uint8, device=dev)
        nv.check(nv.lib.lidbox_lstm_fwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), hp, nv.ptr(cseq), nv.ptr(ws), ws.numel(), st))
        h = hbuf[:, 1:T + 1, col:col + D].clone()
        nv.check(nv.lib.lidbox_lstm_bwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(cseq), dp, T * rs, nv.ptr(dla),
                                        nv.ptr(ws), ws.numel(), st))
    else:
        ws = torch.empty(max(16, nv.lib.lidbox_lstm_step_workspace(B, T, H, dirs)), dtype=torch.uint8, device=dev)
        nv.check(nv.lib.lidbox_lstm_step_fwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), hp, rs, nv.ptr(cseq), nv.ptr(ws),
                                             ws.numel(), st))
        h = hbuf[:, 1:T + 1, col:col + D].clone()
        nv.check(nv.lib.lidbox_lstm_step_bwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(cseq), dp, T * rs, rs,
                                             nv.ptr(dla), nv.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    hb = hbuf.cpu().numpy()
    if wide > 1:
        other = np.ones(rs, bool)
        other[col:col + D] = False
        assert (hb[:, :, other] == SENTINEL).all(), "hseq: columns outside the layer's slice were written"
        if dbuf is not None:
            db_ = dbuf.cpu().numpy()
            assert (db_[:, :, other] == SENTINEL).all(), "dh_seq: columns outside the layer's slice were written"
            assert np.array_equal(db_[:, :, col:col + D], dh_seq), "dh_seq was modified"
    return h.cpu().numpy(), zg_d.cpu().numpy(), hb[:, :, col:col + D]


def _grads_from_dz(params, x, dz, hseq):
    B, T, C = x.shape
    H = params[0][1].shape[0]
    X = x.reshape(B * T, C).astype(np.float64)
    out, dX = [], np.zeros((B * T, C))
    for d, (W, U, b) in enumerate(params):
        Z = dz[d].reshape(B * T, 4 * H).astype(np.float64)
        prow = 0 if d == 0 else 2
        Hp = hseq[:, prow:prow + T, d * H:(d + 1) * H].reshape(B * T, H).astype(np.float64)
        out.append((X.T @ Z, Hp.T @ Z, Z.sum(0)))
        dX += Z @ W.T.astype(np.float64)
    return out, dX.reshape(B, T, C)


def _check(params, x, h, dz, hseq, y, dx_ref, g_ref, tag):
    T = x.shape[1]
    eh = float(np.abs(h - y).max())
    g, dx = _grads_from_dz(params, x, dz, hseq)
    errs = {"dX": _rel(dx, dx_ref)}
    for d in range(len(params)):
        for name, a, r in zip(("dW", "dU", "db"), g[d], g_ref[d]):
            if np.abs(r).max() > 0:
                errs["%s[%d]" % (name, d)] = _rel(a, r)
    print("lstm_step %s: max |h - ref| = %.3e, max rel L2 gradient error = %.3e (%s)"
          % (tag, eh, max(errs.values()), max(errs, key=errs.get)))
    assert eh <= H_TOL, eh
    assert not hseq[:, 0].any() and not hseq[:, T + 1].any()
    for k, v in errs.items():
        assert v <= G_TOL, (k, v)


LAYER_CASES = [(H, dirs, B, T) for H in (1, 10, 81, 100, 250, 251) for dirs in (1, 2) for (B, T) in ((1, 1), (37, 198))] + \
              [(250, 2, 256, 198), (1024, 2, 3, 12),
               (260, 2, 3, 3)]     # backward chunks of 1024 columns: 4H = 1024 + 16


@pytest.mark.parametrize("H,dirs,B,T", LAYER_CASES)
def test_lstm_step_layer_matches_torch(H, dirs, B, T):
    rng = np.random.default_rng(H * 1000 + dirs * 100 + B)
    C = 7
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_seq=dh_seq)
    y, dx_ref, g_ref = _oracle(params, x, dh_seq=dh_seq)
    _check(params, x, h, dz, hseq, y, dx_ref, g_ref, "H=%d dirs=%d B=%d T=%d" % (H, dirs, B, T))


@pytest.mark.parametrize("H,dirs,B,T", [(H, dirs, 37, 50) for H in (1, 10, 100, 250, 251) for dirs in (1, 2)])
def test_lstm_step_layer_in_a_column_slice(H, dirs, B, T):
    """rows 3 * dirs*H floats wide (6H for a bidirectional layer), the layer at column offset dirs*H (2H): the neighbouring
    columns of hseq and dh_seq are untouched, results within the same bounds"""
    rng = np.random.default_rng(H * 10 + dirs)
    C = 6
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_seq=dh_seq, wide=3, col=dirs * H)
    y, dx_ref, g_ref = _oracle(params, x, dh_seq=dh_seq)
    _check(params, x, h, dz, hseq, y, dx_ref, g_ref, "strided H=%d dirs=%d" % (H, dirs))
    # the strides change where values live, not the values (every load path feeds the MFMAs in the same k order)
    h2, dz2, _ = _run_layer(params, x, dh_seq=dh_seq)
    assert np.array_equal(h, h2) and np.array_equal(dz, dz2)


@pytest.mark.parametrize("H,dirs,B,T", [(12, 2, 5, 4), (260, 2, 3, 3)])
def test_lstm_step_scalar_paths_of_misaligned_buffers_give_the_same_bits(H, dirs, B, T):
    """H % 4 == 0 takes the float4 kernels unless a buffer is not 16-byte aligned (backward's float4 path depends on the
    pointers alone): every load path feeds the MFMAs in the same k order, so every output is bit-identical"""
    rng = np.random.default_rng(H * 1000 + dirs * 100 + B)
    C = 7
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_seq=dh_seq)
    h2, dz2, hseq2 = _run_layer(params, x, dh_seq=dh_seq, misalign=True)
    assert np.array_equal(h, h2) and np.array_equal(dz, dz2) and np.array_equal(hseq, hseq2)
    y, dx_ref, g_ref = _oracle(params, x, dh_seq=dh_seq)
    _check(params, x, h, dz, hseq, y, dx_ref, g_ref, "aligned H=%d dirs=%d B=%d T=%d" % (H, dirs, B, T))


@pytest.mark.parametrize("dirs", [1, 2])
def test_lstm_step_final_state_only(dirs):
    """return_sequences=False: only each direction's final h (forward t = T-1, reverse t = 0) receives a gradient"""
    H = 100
    rng = np.random.default_rng(H + dirs)
    B, T, C = 9, 40, 5
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_last = rng.standard_normal((B, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_last=dh_last)
    y, dx_ref, g_ref = _oracle(params, x, dh_last=dh_last)
    _check(params, x, h, dz, hseq, y, dx_ref, g_ref, "dh_last H=%d dirs=%d" % (H, dirs))


@pytest.mark.parametrize("H", [100, 250, 251])
def test_lstm_step_rows_are_batch_independent(H):
    """one utterance's h and dZ are bit-identical alone, at every position of a batch of 37 and as the last row of a batch
    of 256 (one H per load path: float4, float2, scalar)"""
    rng = np.random.default_rng(H)
    C, T, dirs = 6, 24, 2
    params = _params(rng, C, H, dirs)
    one = rng.standard_normal((1, T, C)).astype(np.float32)
    d_one = rng.standard_normal((1, T, dirs * H)).astype(np.float32)
    h1, dz1, _ = _run_layer(params, one, dh_seq=d_one)
    for B, positions in ((37, range(37)), (256, (255,))):
        xb = rng.standard_normal((B, T, C)).astype(np.float32)
        db = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
        for pos in positions:
            x, d = xb.copy(), db.copy()
            x[pos], d[pos] = one[0], d_one[0]
            h, dz, _ = _run_layer(params, x, dh_seq=d)
            assert np.array_equal(h[pos], h1[0]), (B, pos)
            assert np.array_equal(dz[:, pos], dz1[:, 0]), (B, pos)


def test_lstm_step_agrees_with_stepped_form():
    """the same inputs through lidbox_lstm_fwd / _bwd (H = 250: the stepped form) agree within the bounds (not bitwise: the
    sums run in different orders)"""
    nv = _nv()
    H, dirs, B, T, C = 250, 2, 37, 60, 9
    assert not nv.lib.lidbox_lstm_resident_ok(H)
    rng = np.random.default_rng(17)
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_seq=dh_seq)
    hs, dzs, hseqs = _run_layer(params, x, dh_seq=dh_seq, stepped=True)
    eh = float(np.abs(h - hs).max())
    g, dx = _grads_from_dz(params, x, dz, hseq)
    gs, dxs = _grads_from_dz(params, x, dzs, hseqs)
    errs = [_rel(dx, dxs)] + [_rel(a, r) for d in range(dirs) for a, r in zip(g[d], gs[d])]
    print("lstm_step vs stepped form: max |dh| = %.3e, max rel L2 = %.3e" % (eh, max(errs)))
    assert eh <= H_TOL
    assert max(errs) <= G_TOL


def test_lstm_step_empty_batch_is_a_no_op():
    nv = _nv()
    dev = torch.device("cuda")
    U = torch.zeros((8, 32), device=dev)
    z = torch.zeros(16, device=dev)
    st = nv.current_stream()
    assert nv.lib.lidbox_lstm_step_fwd(nv.ptr(U), None, 1, 0, 5, 8, nv.ptr(z), nv.ptr(z), 8, nv.ptr(z), None, 0, st) == 0
    assert nv.lib.lidbox_lstm_step_bwd(nv.ptr(U), None, 1, 0, 5, 8, nv.ptr(z), nv.ptr(z), nv.ptr(z), 40, 8, None, None, 0, st) == 0
