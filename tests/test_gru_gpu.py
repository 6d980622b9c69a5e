"""
GPU tests of the GRU recurrence (csrc/gru.hip), the 2-D BatchNormalization statistics and the bi_gru model
(lidbox_amd.models.bi_gru) against float64 oracles on the CPU.  The layer oracle is torch.nn.GRU: its gates [r, z, n] are
Keras' [z, r, h] reordered, weight_ih = W^T, weight_hh = U^T, bias_ih = b[0], bias_hh = b[1], and its n gate is Keras'
reset_after form.  The model oracle is a float64 transcription of reference lidbox/models/bi_gru.py (GRU + BatchNormalization
+ Dense).

Tolerances: the first measured layer errors (MI355X; every case of LAYER_CASES: H in {1, 10, 62, 100, 512}, T up to 198,
B up to 256) were at most 3.1e-7 absolute on h and 5.1e-7 relative L2 on dX, dW, dU and both bias rows; the bounds below,
5e-5 and 1e-4, keep a margin of more than 100x.
H = 800 and 801 split backward's K per gate into two LDS chunks (float4 and scalar path); the scalar path that only
misaligned buffers select at H % 4 == 0 is compared bit for bit with the float4 path.  Both hold the same bounds.
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H_TOL = 5e-5
G_TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))


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
        lim = math.sqrt(6.0 / (C + 3 * H))
        W = rng.uniform(-lim, lim, (C, 3 * H)).astype(np.float32)
        U = np.ascontiguousarray(orthogonal((H, 3 * H), rng), dtype=np.float32)
        b = (rng.standard_normal((2, 3 * H)) * 0.1).astype(np.float32)
        out.append((W, U, b))
    return out


def _to_torch_order(m, H):
    """Keras columns [z, r, h] -> torch rows [r, z, n]"""
    return np.concatenate([m[..., H:2 * H], m[..., :H], m[..., 2 * H:]], axis=-1)


def _to_keras_order(m, H):
    return np.concatenate([m[..., H:2 * H], m[..., :H], m[..., 2 * H:]], axis=-1)


def _oracle(params, x, dh_seq=None, dh_last=None):
    """float64 torch.nn.GRU: output sequence, dX and (dW, dU, db) per direction in Keras layouts for the loss
    sum(out * dh_seq) + sum(final states * dh_last) (final state: t = T-1 forward, t = 0 reverse)"""
    B, T, C = x.shape
    dirs = len(params)
    H = params[0][1].shape[0]
    m = torch.nn.GRU(C, H, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for d, (W, U, b) in enumerate(params):
            sfx = "_l0" + ("_reverse" if d else "")
            getattr(m, "weight_ih" + sfx).copy_(torch.from_numpy(_to_torch_order(W, H).T.astype(np.float64)))
            getattr(m, "weight_hh" + sfx).copy_(torch.from_numpy(_to_torch_order(U, H).T.astype(np.float64)))
            getattr(m, "bias_ih" + sfx).copy_(torch.from_numpy(_to_torch_order(b[0], H).astype(np.float64)))
            getattr(m, "bias_hh" + sfx).copy_(torch.from_numpy(_to_torch_order(b[1], H).astype(np.float64)))
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
        gW = _to_keras_order(getattr(m, "weight_ih" + sfx).grad.numpy().T, H)
        gU = _to_keras_order(getattr(m, "weight_hh" + sfx).grad.numpy().T, H)
        gb = np.stack([_to_keras_order(getattr(m, "bias_ih" + sfx).grad.numpy(), H),
                       _to_keras_order(getattr(m, "bias_hh" + sfx).grad.numpy(), H)])
        grads.append((gW, gU, gb))
    return y.detach().numpy(), xt.grad.numpy(), grads


def _run_layer(params, x, dh_seq=None, dh_last=None, misalign=False):
    """the recurrence through the C ABI, with the input projection (and, from dZx / dZrec, the weight gradients) in float64
    on the host, so that what is compared is the walk through time.  misalign: U of every direction and zg are not 16-byte
    aligned, which selects the scalar load path whatever H is.  Returns h [B, T, dirs*H], hlast, dZx [dirs, B, T, 3H], the
    h block of dZrec [dirs, B, T, H] and hseq."""
    from lidbox_amd.testutil import device_copy
    nv = _nv()
    B, T, C = x.shape
    dirs = len(params)
    H = params[0][1].shape[0]
    dev = torch.device("cuda")
    zg = np.stack([(x.astype(np.float64) @ W.astype(np.float64) + b[0]).astype(np.float32) for W, _, b in params])
    zg_d = device_copy(zg, misalign)
    hseq = torch.zeros((B, T + 2, dirs * H), dtype=torch.float32, device=dev)
    qh = torch.zeros((dirs, B, T, H), dtype=torch.float32, device=dev)
    hlast = torch.zeros((B, dirs * H), dtype=torch.float32, device=dev)
    Us = [device_copy(U, misalign) for _, U, _ in params]
    brs = [torch.from_numpy(np.ascontiguousarray(b[1])).to(dev) for _, _, b in params]
    ws = torch.empty(max(16, nv.lib.lidbox_gru_workspace(B, T, H, dirs)), dtype=torch.uint8, device=dev)
    st = nv.current_stream()
    U1 = nv.ptr(Us[1]) if dirs == 2 else None
    b1 = nv.ptr(brs[1]) if dirs == 2 else None
    nv.check(nv.lib.lidbox_gru_fwd(nv.ptr(Us[0]), U1, nv.ptr(brs[0]), b1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(hseq), nv.ptr(qh),
                                   nv.ptr(hlast), st))
    h = hseq[:, 1:T + 1].clone()
    hl = hlast.clone()
    dsq = None if dh_seq is None else torch.from_numpy(dh_seq).to(dev).contiguous()
    dla = None if dh_last is None else torch.from_numpy(dh_last).to(dev).contiguous()
    nv.check(nv.lib.lidbox_gru_bwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(hseq), nv.ptr(qh), nv.ptr(dsq),
                                   T * dirs * H, nv.ptr(dla), nv.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    return h.cpu().numpy(), hl.cpu().numpy(), zg_d.cpu().numpy(), qh.cpu().numpy(), hseq.cpu().numpy()


def _grads_from_dz(params, x, dzx, dqh, hseq):
    B, T, C = x.shape
    H = params[0][1].shape[0]
    X = x.reshape(B * T, C).astype(np.float64)
    out, dX = [], np.zeros((B * T, C))
    for d, (W, U, b) in enumerate(params):
        Zx = dzx[d].reshape(B * T, 3 * H).astype(np.float64)
        Zr = np.concatenate([Zx[:, :2 * H], dqh[d].reshape(B * T, H).astype(np.float64)], axis=1)
        prow = 0 if d == 0 else 2
        Hp = hseq[:, prow:prow + T, d * H:(d + 1) * H].reshape(B * T, H).astype(np.float64)
        out.append((X.T @ Zx, Hp.T @ Zr, np.stack([Zx.sum(0), Zr.sum(0)])))
        dX += Zx @ W.T.astype(np.float64)
    return out, dX.reshape(B, T, C)


def _check_grads(g, dx, g_ref, dx_ref):
    assert _rel(dx, dx_ref) <= G_TOL, ("dX", _rel(dx, dx_ref))
    for d in range(len(g)):
        for name, a, r in zip(("dW", "dU", "db"), g[d], g_ref[d]):
            if name == "db":
                for row in range(2):
                    assert _rel(a[row], r[row]) <= G_TOL, ("db", row, d, _rel(a[row], r[row]))
            elif np.abs(r).max() > 0:
                assert _rel(a, r) <= G_TOL, (name, d, _rel(a, r))


LAYER_CASES = [(H, dirs, B, T) for H in (1, 10, 62, 100) for dirs in (1, 2) for (B, T) in ((1, 1), (37, 198), (256, 198))] + \
              [(512, dirs, B, T) for dirs in (1, 2) for (B, T) in ((1, 1), (37, 60), (256, 16))] + \
              [(800, 2, 3, 3), (801, 1, 3, 3)]     # backward chunks of 768 columns: 768 + 32 (float4), 768 + 33 (scalar)


@pytest.mark.parametrize("H,dirs,B,T", LAYER_CASES)
def test_gru_layer_matches_torch(H, dirs, B, T):
    rng = np.random.default_rng(H * 1000 + dirs * 100 + B)
    C = 7
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    _check_layer(params, x, dh_seq, *_run_layer(params, x, dh_seq=dh_seq))


def _check_layer(params, x, dh_seq, h, hl, dzx, dqh, hseq):
    T, dirs, H = x.shape[1], len(params), params[0][1].shape[0]
    y, dx_ref, g_ref = _oracle(params, x, dh_seq=dh_seq)
    assert np.abs(h - y).max() <= H_TOL, np.abs(h - y).max()
    assert not hseq[:, 0].any() and not hseq[:, T + 1].any()
    assert np.array_equal(hl[:, :H], h[:, -1, :H])
    if dirs == 2:
        assert np.array_equal(hl[:, H:], h[:, 0, H:])
    g, dx = _grads_from_dz(params, x, dzx, dqh, hseq)
    _check_grads(g, dx, g_ref, dx_ref)


def test_gru_scalar_path_of_misaligned_buffers_gives_the_same_bits():
    """H % 4 == 0 takes the float4 kernels unless a buffer is not 16-byte aligned: both load paths feed the MFMAs in the
    same k order, so every output is bit-identical"""
    H, dirs, B, T, C = 12, 2, 5, 4, 7
    rng = np.random.default_rng(H * 1000 + dirs * 100 + B)
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    aligned = _run_layer(params, x, dh_seq=dh_seq)
    scalar = _run_layer(params, x, dh_seq=dh_seq, misalign=True)
    for name, a, b in zip(("h", "hlast", "dZx", "qh", "hseq"), aligned, scalar):
        assert np.array_equal(a, b), name
    _check_layer(params, x, dh_seq, *aligned)


@pytest.mark.parametrize("H,dirs", [(10, 2), (100, 2), (62, 1)])
def test_gru_layer_final_state_only(H, dirs):
    """return_sequences=False: only each direction's final state (forward t = T-1, backward t = 0) receives a gradient"""
    rng = np.random.default_rng(H + dirs)
    B, T, C = 9, 40, 5
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_last = rng.standard_normal((B, dirs * H)).astype(np.float32)
    h, hl, dzx, dqh, hseq = _run_layer(params, x, dh_last=dh_last)
    y, dx_ref, g_ref = _oracle(params, x, dh_last=dh_last)
    ref_last = np.concatenate([y[:, -1, :H]] + ([y[:, 0, H:]] if dirs == 2 else []), axis=1)
    assert np.abs(hl - ref_last).max() <= H_TOL
    g, dx = _grads_from_dz(params, x, dzx, dqh, hseq)
    _check_grads(g, dx, g_ref, dx_ref)


@pytest.mark.parametrize("H", [62, 100])
def test_gru_rows_are_batch_independent(H):
    """one utterance's h, dZx and dZrec are bit-identical alone, at every position of a batch of 37 and inside B = 256"""
    rng = np.random.default_rng(H)
    C, T, dirs = 6, 30, 2
    params = _params(rng, C, H, dirs)
    one = rng.standard_normal((1, T, C)).astype(np.float32)
    d_one = rng.standard_normal((1, T, dirs * H)).astype(np.float32)
    h1, hl1, dz1, dq1, _ = _run_layer(params, one, dh_seq=d_one)
    for B, positions in ((37, range(37)), (256, (0, 63, 64, 200, 255))):
        xb = rng.standard_normal((B, T, C)).astype(np.float32)
        db = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
        for pos in positions:
            x, d = xb.copy(), db.copy()
            x[pos], d[pos] = one[0], d_one[0]
            h, hl, dz, dq, _ = _run_layer(params, x, dh_seq=d)
            assert np.array_equal(h[pos], h1[0]) and np.array_equal(hl[pos], hl1[0]), (B, pos)
            assert np.array_equal(dz[:, pos], dz1[:, 0]) and np.array_equal(dq[:, pos], dq1[:, 0]), (B, pos)


# ---------------------------------------------------------------------------------------------------- BatchNormalization
def test_bn_2d_stats_population_variance():
    """lidbox_bn_train_stats_ex(bessel=0): the moving variance moves towards the population batch variance; bessel=1 and the
    existing lidbox_bn_train_stats keep the Bessel-corrected target"""
    nv = _nv()
    rng = np.random.default_rng(0)
    R, C = 37, 20
    x = (rng.standard_normal((R, C)) * 2 + 0.5).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.standard_normal(C).astype(np.float32)
    mm0 = rng.standard_normal(C).astype(np.float32)
    mv0 = rng.uniform(0.5, 2.0, C).astype(np.float32)
    dev = torch.device("cuda")
    xd, gd, bd = (torch.from_numpy(a).to(dev) for a in (x, gamma, beta))
    ws = torch.empty(nv.lib.lidbox_bn_workspace(R, C), dtype=torch.uint8, device=dev)
    mean64, var64 = x.astype(np.float64).mean(0), x.astype(np.float64).var(0)
    results = {}
    for mode in ("pop", "bessel_flag", "legacy"):
        mm, mv = torch.from_numpy(mm0.copy()).to(dev), torch.from_numpy(mv0.copy()).to(dev)
        consts = torch.zeros((4, C), dtype=torch.float32, device=dev)
        cp = [nv.ptr(consts[j]) for j in range(4)]
        st = nv.current_stream()
        if mode == "legacy":
            nv.check(nv.lib.lidbox_bn_train_stats(nv.ptr(xd), R, C, nv.ptr(gd), nv.ptr(bd), 1e-3, 0.99, nv.ptr(mm), nv.ptr(mv),
                                                  *cp, nv.ptr(ws), ws.numel(), st))
        else:
            nv.check(nv.lib.lidbox_bn_train_stats_ex(nv.ptr(xd), R, C, nv.ptr(gd), nv.ptr(bd), 1e-3, 0.99, 0 if mode == "pop" else 1,
                                                     nv.ptr(mm), nv.ptr(mv), *cp, nv.ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        c = consts.cpu().numpy()
        assert np.abs(c[0] - mean64).max() <= 1e-5 * max(1.0, np.abs(mean64).max())
        assert np.abs(c[1] - 1 / np.sqrt(var64 + 1e-3)).max() <= 1e-5
        assert np.allclose(mm.cpu().numpy(), 0.99 * mm0 + 0.01 * mean64, rtol=1e-6, atol=1e-6)
        results[mode] = (mv.cpu().numpy(), c)
    assert np.allclose(results["pop"][0], 0.99 * mv0 + 0.01 * var64, rtol=1e-6, atol=1e-6)
    bessel = 0.99 * mv0 + 0.01 * var64 * R / (R - 1)
    assert np.allclose(results["legacy"][0], bessel, rtol=1e-6, atol=1e-6)
    assert np.array_equal(results["legacy"][0], results["bessel_flag"][0])
    assert not np.allclose(results["pop"][0], results["legacy"][0], rtol=1e-7, atol=0)
    for mode in ("pop", "bessel_flag"):
        assert np.array_equal(results[mode][1], results["legacy"][1])      # the normalisation does not depend on the flag


# ---------------------------------------------------------------------------------------------------- whole model
def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


def _torch_model(model, weights):
    """float64 transcription of bi_gru.py: returns (params dict of leaf tensors, fwd(x, training) -> (logits, fc_relu_1
    pre-activation, {bn name: (batch mean, population variance)}))"""
    p = {k: _t(v) for k, v in weights.items()}

    def gru(x, prefix, reverse):
        W, U, b = p[prefix + ".W"], p[prefix + ".U"], p[prefix + ".b"]
        B, T, _ = x.shape
        H = U.shape[0]
        xp = x @ W + b[0]
        h = torch.zeros((B, H), dtype=torch.float64)
        outs = [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            q = h @ U + b[1]
            z = torch.sigmoid(xp[:, t, :H] + q[:, :H])
            r = torch.sigmoid(xp[:, t, H:2 * H] + q[:, H:2 * H])
            hh = torch.tanh(xp[:, t, 2 * H:] + r * q[:, 2 * H:])
            h = z * h + (1 - z) * hh
            outs[t] = h
        return torch.stack(outs, 1), h

    def fwd(x, training):
        stats = {}

        def bn(v, name):
            if training:
                mean, var = v.mean(0), v.var(0, unbiased=False)
                stats[name] = (mean.detach().numpy(), var.detach().numpy())
            else:
                mean, var = p[name + ".moving_mean"].detach(), p[name + ".moving_variance"].detach()
            return (v - mean) / torch.sqrt(var + 1e-3) * p[name + ".gamma"] + p[name + ".beta"]

        x = torch.from_numpy(np.asarray(x, np.float64))
        s1 = torch.cat([gru(x, "BGRU_1_forward", False)[0], gru(x, "BGRU_1_backward", True)[0]], dim=2)
        h = torch.cat([gru(s1, "BGRU_2_forward", False)[1], gru(s1, "BGRU_2_backward", True)[1]], dim=1)
        h = bn(h, "BGRU_2_bn")
        pre1 = h @ p["fc_relu_1.W"] + p["fc_relu_1.b"]
        a = bn(torch.relu(pre1), "fc_relu_1_bn")
        a = bn(torch.relu(a @ p["fc_relu_2.W"] + p["fc_relu_2.b"]), "fc_relu_2_bn")
        return a @ p["output.W"] + p["output.b"], pre1, stats
    return p, fwd


def _small(seed=2, T=15, C=8, N=5, H=20, F=24):
    from lidbox_amd.models import bi_gru
    return bi_gru.create((T, C), N, seed=seed, num_units=H, num_fc_units=F)


def _randomise_state(model, rng):
    for n, (_, shape) in model.state_layout.items():
        v = rng.uniform(0.5, 1.5, shape) if n.endswith("variance") else rng.standard_normal(shape) * 0.3
        model.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    for n, (_, shape) in model.layout.items():
        if n.endswith(".gamma") or n.endswith(".beta") or (n.endswith(".b") and len(shape) == 2):
            base = 1.0 if n.endswith(".gamma") else 0.0
            model.param(n).copy_(torch.from_numpy((base + rng.standard_normal(shape) * 0.1).astype(np.float32)))


def test_bi_gru_model_train_forward_backward_matches_torch():
    rng = np.random.default_rng(3)
    B, T, C, N = 6, 15, 8, 5
    model = _small()
    _randomise_state(model, rng)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    G = rng.standard_normal((B, N)).astype(np.float32)
    w0 = model.get_weights()
    ws = model.workspace(B, T)
    model._load_input(ws, torch.from_numpy(x).cuda(), False)
    out = model.forward_ws(ws, training=True)
    logits = ws.h[-1].clone()
    ws.dh[-1].copy_(torch.from_numpy(G).cuda())
    model.backward_ws(ws)
    torch.cuda.synchronize()
    p, fwd = _torch_model(model, w0)
    ref, _, stats = fwd(x, True)
    (ref * torch.from_numpy(G.astype(np.float64))).sum().backward()
    assert np.abs(logits.cpu().numpy() - ref.detach().numpy()).max() <= H_TOL
    assert np.abs(out.cpu().numpy() - torch.log_softmax(ref.detach(), 1).numpy()).max() <= H_TOL
    for n in model.layout:
        assert _rel(model.param(n, grad=True).cpu().numpy(), p[n].grad.numpy()) <= G_TOL, (n, _rel(model.param(n, grad=True).cpu().numpy(), p[n].grad.numpy()))
    # one training pass moves the running statistics once, towards the population statistics
    w1 = model.get_weights()
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.99 * w0[name + ".moving_mean"] + 0.01 * mean, rtol=1e-5, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 * w0[name + ".moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-6), name


def test_bi_gru_model_inference_and_embedding_match_torch():
    from lidbox_amd.models import bi_gru
    rng = np.random.default_rng(4)
    B, T, C = 5, 15, 8
    model = _small(seed=5)
    _randomise_state(model, rng)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    w0 = model.get_weights()
    _, fwd = _torch_model(model, w0)
    ref, pre1, _ = fwd(x, False)
    got = model(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(got - torch.log_softmax(ref.detach(), 1).numpy()).max() <= H_TOL
    emb = bi_gru.as_embedding_extractor(model)(torch.from_numpy(x).cuda()).cpu().numpy()
    assert emb.shape == (B, 24)
    assert np.abs(emb - pre1.detach().numpy()).max() <= H_TOL
    assert (emb < 0).any()                              # the ReLU is not applied
    w1 = model.get_weights()
    assert all(np.array_equal(w0[n], w1[n]) for n in model.state_layout)      # inference leaves the statistics alone


# ---------------------------------------------------------------------------------------------------- training
def test_trainer_step_graph_equals_eager_and_matches_torch():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(9)
    B, T, C, N = 8, 15, 8, 5
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = []
    for graph in (True, False):
        m = _small(seed=1)
        w0 = m.get_weights()
        tr = Trainer(m, use_graph=graph)
        losses = [float(tr.train_step(xd, yd)) for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, m.get_weights()))
    (lg, wg), (le, we) = res
    assert lg == le
    for n in wg:
        assert np.array_equal(wg[n], we[n]), n
    _, fwd = _torch_model(_small(seed=1), w0)
    ref, _, stats = fwd(x, True)
    ref_loss = float(torch.nn.functional.cross_entropy(ref.detach(), torch.from_numpy(y.astype(np.int64))))
    assert abs(lg[0] - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))


def test_moving_statistics_advance_once_per_step_not_in_warmup():
    """the captured Trainer runs a warm-up pass before capture: the running statistics must show one update per real step"""
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(10)
    B, T, C, N = 8, 12, 8, 4
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    m = _small(seed=6, T=T, N=N)
    w0 = m.get_weights()
    tr = Trainer(m, use_graph=True)
    tr.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    w1 = m.get_weights()
    _, fwd = _torch_model(m, w0)
    _, _, stats = fwd(x, True)
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.01 * mean, rtol=1e-4, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 + 0.01 * var, rtol=1e-5, atol=1e-6), name


def test_loss_falls_on_separable_problem():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(11)
    B, T, C, N = 32, 20, 8, 4
    y = rng.integers(0, N, B).astype(np.int32)
    centres = rng.standard_normal((N, C)).astype(np.float32) * 2
    x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((B, T, C))).astype(np.float32)
    m = _small(seed=3, T=T, N=N)
    tr = Trainer(m, optimizer={"cls": "Adam", "lr": 3e-3})
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    losses = [float(tr.train_step(xd, yd)) for _ in range(30)]
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses


def test_keras_wrapper_trains_bi_gru(tmp_path):
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.gru_rnn import GRUModel
    rng = np.random.default_rng(12)
    T, C, N = 20, 12, 3
    data = []
    centres = rng.standard_normal((N, C)).astype(np.float32) * 2
    for _ in range(3):
        y = rng.integers(0, N, 16).astype(np.int32)
        x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((16, T, C))).astype(np.float32)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "bgru",
        "model": {"key": "bi_gru", "kwargs": {"num_units": 16, "num_fc_units": 32, "seed": 3}},
        "input_shape": [T, C], "output_shape": [N],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseCategoricalCrossentropy", "kwargs": {"from_logits": True}},
        "metrics": [], "callbacks": []}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, GRUModel)
    hist = w.fit(data, data[:1], {"epochs": 3, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 3 and np.isfinite(loss).all() and loss[-1] < loss[0]


# ---------------------------------------------------------------------------------------------------- HDF5
def test_hdf5_fixture_loads_into_bi_gru():
    import sys
    from lidbox_amd.models import bi_gru
    from lidbox_amd.models.keras_utils import read_weights_file, _set_weights_checked
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_bi_gru_h5 import BI_GRU_LAYERS, C, F, H, N, expected_name
    from make_keras_h5 import values
    path = os.path.join(HERE, "golden", "keras_bi_gru_weights.h5")
    model = bi_gru.create((20, C), N, seed=0, num_units=H, num_fc_units=F)
    _set_weights_checked(model, read_weights_file(path), path)
    got = model.get_weights()
    for _, vars_ in BI_GRU_LAYERS:
        for wname, shape in vars_:
            assert np.array_equal(got[expected_name(wname)], values(wname, shape)), wname
    x = np.random.default_rng(0).standard_normal((3, 20, C)).astype(np.float32)
    _, fwd = _torch_model(model, got)
    ref = torch.log_softmax(fwd(x, False)[0], 1).detach().numpy()
    out = model(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(out - ref).max() <= H_TOL
