"""
GPU tests of the LSTM recurrence (csrc/rnn.hip) and the recurrent models (lidbox_amd.models.lstm / ap_lstm) against a
float64 torch.nn.LSTM oracle on the CPU (gate order i, f, g, o as Keras; weight_ih = W^T, weight_hh = U^T, bias_ih = b,
bias_hh = 0).  The model-level oracle is a short transcription of reference lidbox/models/lstm.py and ap_lstm.py.

Tolerances: the first measured errors (MI355X; H in {1, 62, 80, 81, 100, 1024}, T up to 198) were at most 2.0e-7 absolute on
h and 5.9e-7 relative L2 on gradients; the bounds below, 5e-5 and 1e-4, keep a margin of more than 100x.
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
        lim = math.sqrt(6.0 / (C + 4 * H))
        W = rng.uniform(-lim, lim, (C, 4 * H)).astype(np.float32)
        U = np.ascontiguousarray(orthogonal((H, 4 * H), rng), dtype=np.float32)
        b = (rng.standard_normal(4 * H) * 0.1).astype(np.float32)
        b[H:2 * H] += 1.0
        out.append((W, U, b))
    return out


def _torch_lstm(params, C, H):
    dirs = len(params)
    m = torch.nn.LSTM(C, H, batch_first=True, bidirectional=dirs == 2).double()
    with torch.no_grad():
        for d, (W, U, b) in enumerate(params):
            sfx = "_l0" + ("_reverse" if d else "")
            getattr(m, "weight_ih" + sfx).copy_(torch.from_numpy(W.T.astype(np.float64)))
            getattr(m, "weight_hh" + sfx).copy_(torch.from_numpy(U.T.astype(np.float64)))
            getattr(m, "bias_ih" + sfx).copy_(torch.from_numpy(b.astype(np.float64)))
            getattr(m, "bias_hh" + sfx).zero_()
    return m


def _oracle(params, x, dh_seq=None, dh_last=None):
    """float64 torch: output sequence, gradients of sum(out * dh_seq) + sum(last h * dh_last)"""
    B, T, C = x.shape
    H = params[0][1].shape[0]
    m = _torch_lstm(params, C, H)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    y, (hn, _) = m(xt)
    loss = 0.0
    if dh_seq is not None:
        loss = loss + (y * torch.from_numpy(dh_seq.astype(np.float64))).sum()
    if dh_last is not None:
        loss = loss + (y[:, -1, :H] * torch.from_numpy(dh_last.astype(np.float64))).sum()
    loss.backward()
    grads = []
    for d in range(len(params)):
        sfx = "_l0" + ("_reverse" if d else "")
        grads.append((getattr(m, "weight_ih" + sfx).grad.numpy().T, getattr(m, "weight_hh" + sfx).grad.numpy().T,
                      getattr(m, "bias_ih" + sfx).grad.numpy()))
    return y.detach().numpy(), xt.grad.numpy(), grads


def _run_layer(params, x, dh_seq=None, dh_last=None):
    """the recurrence through the C ABI: the projection (and, from dZ, the weight gradients) in float64 on the host, so
    that what is compared is the walk through time.  Returns h [B, T, dirs*H], dZ [dirs, B, T, 4H], hseq."""
    nv = _nv()
    B, T, C = x.shape
    dirs = len(params)
    H = params[0][1].shape[0]
    dev = torch.device("cuda")
    zg = np.stack([(x.astype(np.float64) @ W.astype(np.float64) + b).astype(np.float32) for W, _, b in params])
    zg_d = torch.from_numpy(zg).to(dev).contiguous()
    hseq = torch.zeros((B, T + 2, dirs * H), dtype=torch.float32, device=dev)
    cseq = torch.zeros((dirs, B, T, H), dtype=torch.float32, device=dev)
    Us = [torch.from_numpy(U).to(dev) for _, U, _ in params]
    ws = torch.empty(max(16, nv.lib.lidbox_lstm_workspace(B, T, H, dirs)), dtype=torch.uint8, device=dev)
    st = nv.current_stream()
    U1 = nv.ptr(Us[1]) if dirs == 2 else None
    nv.check(nv.lib.lidbox_lstm_fwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(hseq), nv.ptr(cseq), nv.ptr(ws),
                                    ws.numel(), st))
    h = hseq[:, 1:T + 1].clone()
    dsq = None if dh_seq is None else torch.from_numpy(dh_seq).to(dev).contiguous()
    dla = None if dh_last is None else torch.from_numpy(dh_last).to(dev).contiguous()
    nv.check(nv.lib.lidbox_lstm_bwd(nv.ptr(Us[0]), U1, dirs, B, T, H, nv.ptr(zg_d), nv.ptr(cseq), nv.ptr(dsq), T * dirs * H,
                                    nv.ptr(dla), nv.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    return h.cpu().numpy(), zg_d.cpu().numpy(), hseq.cpu().numpy()


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


LAYER_CASES = [(H, dirs, B, T) for H in (1, 10, 62, 80, 81, 100) for dirs in (1, 2)
               for (B, T) in ((1, 1), (37, 198), (256, 198))] + [(1024, 1, 3, 12), (1024, 2, 2, 5)]


@pytest.mark.parametrize("H,dirs,B,T", LAYER_CASES)
def test_lstm_layer_matches_torch(H, dirs, B, T):
    nv = _nv()
    assert nv.lib.lidbox_lstm_resident_ok(80) == 1 and nv.lib.lidbox_lstm_resident_ok(81) == 0
    rng = np.random.default_rng(H * 1000 + dirs * 100 + B)
    C = 7
    params = _params(rng, C, H, dirs)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_seq = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_seq=dh_seq)
    y, dx_ref, g_ref = _oracle(params, x, dh_seq=dh_seq)
    assert np.abs(h - y).max() <= H_TOL
    assert not hseq[:, 0].any() and not hseq[:, T + 1].any()
    g, dx = _grads_from_dz(params, x, dz, hseq)
    assert _rel(dx, dx_ref) <= G_TOL
    for d in range(dirs):
        for name, a, r in zip(("dW", "dU", "db"), g[d], g_ref[d]):
            if np.abs(r).max() > 0:
                assert _rel(a, r) <= G_TOL, (name, d, _rel(a, r))


@pytest.mark.parametrize("H", [10, 62, 100])
def test_lstm_layer_last_state_only(H):
    """return_sequences=False: only the final h receives a gradient"""
    rng = np.random.default_rng(H)
    B, T, C = 9, 40, 5
    params = _params(rng, C, H, 1)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    dh_last = rng.standard_normal((B, H)).astype(np.float32)
    h, dz, hseq = _run_layer(params, x, dh_last=dh_last)
    y, dx_ref, g_ref = _oracle(params, x, dh_last=dh_last)
    assert np.abs(h[:, -1] - y[:, -1]).max() <= H_TOL
    g, dx = _grads_from_dz(params, x, dz, hseq)
    assert _rel(dx, dx_ref) <= G_TOL
    for a, r in zip(g[0], g_ref[0]):
        assert _rel(a, r) <= G_TOL


def test_resident_rows_are_batch_independent():
    """one utterance's h and dZ are bit-identical alone and at every position of a batch of 37 (and inside a batch large
    enough for more rows per workgroup)"""
    rng = np.random.default_rng(5)
    H, C, T, dirs = 62, 6, 50, 2
    assert _nv().lib.lidbox_lstm_resident_ok(H)
    params = _params(rng, C, H, dirs)
    one = rng.standard_normal((1, T, C)).astype(np.float32)
    d_one = rng.standard_normal((1, T, dirs * H)).astype(np.float32)
    h1, dz1, _ = _run_layer(params, one, dh_seq=d_one)
    B = 37
    xb = rng.standard_normal((B, T, C)).astype(np.float32)
    db = rng.standard_normal((B, T, dirs * H)).astype(np.float32)
    for pos in range(B):
        x = xb.copy()
        d = db.copy()
        x[pos], d[pos] = one[0], d_one[0]
        h, dz, _ = _run_layer(params, x, dh_seq=d)
        assert np.array_equal(h[pos], h1[0]), pos
        assert np.array_equal(dz[:, pos], dz1[:, 0]), pos
    big = 1100                                  # more rows per workgroup at this B
    x = np.concatenate([rng.standard_normal((big - 1, T, C)).astype(np.float32), one])
    d = np.concatenate([rng.standard_normal((big - 1, T, dirs * H)).astype(np.float32), d_one])
    h, dz, _ = _run_layer(params, x, dh_seq=d)
    assert np.array_equal(h[-1], h1[0]) and np.array_equal(dz[:, -1], dz1[:, 0])


def test_resident_and_stepped_forms_agree():
    """H = 80 runs resident, H = 81 stepped; an 81st unit with all-zero weights stays exactly 0, so both compute the same
    layer: equal within tolerance (not bitwise: the sums run in different orders)"""
    nv = _nv()
    assert nv.lib.lidbox_lstm_resident_ok(80) and not nv.lib.lidbox_lstm_resident_ok(81)
    rng = np.random.default_rng(11)
    C, T, B = 9, 60, 24
    p80 = _params(rng, C, 80, 2)
    p81 = []
    for W, U, b in p80:
        def widen(m, rows):
            out = np.zeros((rows, 4 * 81), np.float32)
            for q in range(4):
                out[:m.shape[0], q * 81:q * 81 + 80] = m[:, q * 80:(q + 1) * 80]
            return out
        p81.append((widen(W, C), widen(U, 81), widen(b[None], 1)[0]))
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    d80 = rng.standard_normal((B, T, 160)).astype(np.float32)
    d81 = np.zeros((B, T, 162), np.float32)
    d81[:, :, :80], d81[:, :, 81:161] = d80[:, :, :80], d80[:, :, 80:]
    h80, dz80, _ = _run_layer(p80, x, dh_seq=d80)
    h81, dz81, _ = _run_layer(p81, x, dh_seq=d81)
    assert not h81[:, :, 80].any() and not h81[:, :, 161].any()
    h81c = np.concatenate([h81[:, :, :80], h81[:, :, 81:161]], axis=2)
    assert np.abs(h80 - h81c).max() <= H_TOL
    for q in range(4):
        a = dz80[..., q * 80:(q + 1) * 80]
        b = dz81[..., q * 81:q * 81 + 80]
        assert _rel(a, b) <= G_TOL


# ---------------------------------------------------------------------------------------------------- whole models
def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


def _torch_model(model, weights):
    """float64 transcription of lstm.py / ap_lstm.py: returns (params dict of leaf tensors, forward(x) -> output before
    the final normalisation / activation)"""
    p = {k: _t(v) for k, v in weights.items()}

    def run_lstm(x, prefix, reverse):
        W, U, b = p[prefix + ".W"], p[prefix + ".U"], p[prefix + ".b"]
        B, T, _ = x.shape
        H = U.shape[0]
        h = torch.zeros((B, H), dtype=torch.float64)
        c = torch.zeros((B, H), dtype=torch.float64)
        outs = [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            z = x[:, t] @ W + h @ U + b
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            outs[t] = h
        return torch.stack(outs, 1)

    def fwd(x):
        x = torch.from_numpy(np.asarray(x, np.float64))
        if model.head == "avg_concat":
            seqs = []
            for l in model.lstms:
                x = torch.cat([run_lstm(x, l.prefixes[0], False), run_lstm(x, l.prefixes[1], True)], dim=2)
                seqs.append(x)
            return torch.cat([a * s.mean(1) for a, s in zip(model.alphas, seqs)], dim=1)
        l = model.lstms[0]
        y = run_lstm(x, l.prefixes[0], False)[:, -1]
        return y @ p["output.W"] + p["output.b"]
    return p, fwd


def _model_grads(model, x, G):
    """forward_ws + backward_ws with d loss / d output-before-activation = G; returns (output, grads dict)"""
    nv = _nv()
    ws = model.workspace(*x.shape[:2])
    model._load_input(ws, torch.from_numpy(x).cuda(), False)
    out = model.forward_ws(ws, training=True)
    pre = ws.h[-1].clone()
    ws.dh[-1].copy_(torch.from_numpy(G).cuda())
    model.backward_ws(ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), pre.cpu().numpy(), {n: model.param(n, grad=True).cpu().numpy() for n in model.layout}


@pytest.mark.parametrize("H", [16, 62, 90])
def test_ap_lstm_model_matches_torch(H):
    from lidbox_amd.models import ap_lstm
    rng = np.random.default_rng(H)
    B, T, C = 5, 30, 12
    model = ap_lstm.create((T, C), num_lstm_units=H, alpha1=0.7, alpha2=1.3, seed=H)
    assert model.output_dim == 4 * H and model.output_activation is None
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    G = rng.standard_normal((B, 4 * H)).astype(np.float32)
    _, pre, grads = _model_grads(model, x, G)
    p, fwd = _torch_model(model, model.get_weights())
    ref = fwd(x)
    (ref * torch.from_numpy(G.astype(np.float64))).sum().backward()
    assert np.abs(pre - ref.detach().numpy()).max() <= H_TOL
    for n in model.layout:
        assert _rel(grads[n], p[n].grad.numpy()) <= G_TOL, n
    z = model(torch.from_numpy(x).cuda()).cpu().numpy()
    zr = torch.nn.functional.normalize(ref.detach(), dim=1).numpy()
    assert np.abs(z - zr).max() <= H_TOL
    assert np.allclose(np.linalg.norm(z, axis=1), 1.0, atol=1e-5)


def test_lstm_model_matches_torch():
    from lidbox_amd.models import lstm
    rng = np.random.default_rng(3)
    B, T, C, N = 6, 25, 10, 5
    model = lstm.create((T, C), N, num_units=96, seed=2)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    G = rng.standard_normal((B, N)).astype(np.float32)
    out, pre, grads = _model_grads(model, x, G)
    p, fwd = _torch_model(model, model.get_weights())
    ref = fwd(x)
    (ref * torch.from_numpy(G.astype(np.float64))).sum().backward()
    assert np.abs(pre - ref.detach().numpy()).max() <= H_TOL
    assert np.abs(out - torch.log_softmax(ref.detach(), 1).numpy()).max() <= H_TOL
    for n in model.layout:
        assert _rel(grads[n], p[n].grad.numpy()) <= G_TOL, n


# ---------------------------------------------------------------------------------------------------- train step
def _ap_loss_t(z, y, N, delta_weight=1.0):
    zn = torch.nn.functional.normalize(z, dim=1)
    theta = torch.acos(zn[:, :N].clamp(-1.0, 1.0))
    th_l = theta.gather(1, torch.from_numpy(y.astype(np.int64))[:, None])
    s = torch.sigmoid(delta_weight * (th_l - theta))
    mask = 1.0 - torch.nn.functional.one_hot(torch.from_numpy(y.astype(np.int64)), N).double()
    return (mask * s).sum(1).mean()


def _keras_adam(p, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """one tf.keras Adam step from zero moments (t = 1) on float64 leaves with .grad"""
    lr_t = lr * math.sqrt(1 - b2) / (1 - b1)
    out = {}
    for n, t in p.items():
        g = t.grad.numpy()
        m, v = (1 - b1) * g, (1 - b2) * g * g
        out[n] = t.detach().numpy() - lr_t * m / (np.sqrt(v) + eps)
    return out


def _check_step(model, trainer_fn, x_in, y, loss_fn, feats=None):
    from lidbox_amd.train import Trainer  # noqa: F401
    w0 = model.get_weights()
    tr = trainer_fn(model)
    xd = torch.from_numpy(x_in).cuda()
    yd = torch.from_numpy(y.astype(np.int32)).cuda()
    loss = float(tr.train_step(xd, yd))
    torch.cuda.synchronize()
    p, fwd = _torch_model(model, w0)
    ref_loss = loss_fn(fwd(x_in if feats is None else feats))
    ref_loss.backward()
    ref = float(ref_loss.detach())
    assert abs(loss - ref) <= 1e-4 * max(1.0, abs(ref))
    want = _keras_adam(p)
    got = model.get_weights()
    for n in model.layout:
        step_ref = want[n] - w0[n]
        step = got[n] - w0[n]
        # an Adam step is ~lr * sign(g): compare where the gradient is not vanishingly small
        big = np.abs(p[n].grad.numpy()) > 1e-3 * max(1e-30, np.abs(p[n].grad.numpy()).max())
        assert np.abs(step - step_ref)[big].max() <= 2e-5, n
    return model.get_weights()


def test_trainer_step_ap_lstm_and_graph_equals_eager():
    from lidbox_amd.losses import SparseAngularProximity
    from lidbox_amd.models import ap_lstm
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(8)
    B, T, C, H, N = 8, 40, 40, 62, 4
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    loss = SparseAngularProximity(N=N, D=4 * H)
    mk = lambda: ap_lstm.create((T, C), num_lstm_units=H, seed=4)
    g = _check_step(mk(), lambda m: Trainer(m, loss=loss, use_graph=True), x, y, lambda z: _ap_loss_t(z, y, N))
    e = _check_step(mk(), lambda m: Trainer(m, loss=loss, use_graph=False), x, y, lambda z: _ap_loss_t(z, y, N))
    for n in g:
        assert np.array_equal(g[n], e[n]), n


def test_trainer_step_lstm_cross_entropy():
    from lidbox_amd.models import lstm
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(9)
    B, T, C, N = 8, 30, 20, 5
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    yt = torch.from_numpy(y.astype(np.int64))
    _check_step(lstm.create((T, C), N, num_units=64, seed=1), lambda m: Trainer(m), x, y,
                lambda z: torch.nn.functional.cross_entropy(torch.log_softmax(z, 1), yt))


def test_trainer_step_waveform_logmel_ap_lstm():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    from lidbox_amd.losses import SparseAngularProximity
    from lidbox_amd.models import ap_lstm
    from lidbox_amd.testutil import synthetic_batch
    from lidbox_amd.train import Trainer
    sig, y = synthetic_batch(4, num_labels=4, duration_s=0.5)
    plan = audio.get_plan(16000, 400, 160)
    feats = plan.run(nv.FEAT_LOGMEL, torch.from_numpy(sig).cuda()).cpu().numpy()
    T = feats.shape[1]
    loss = SparseAngularProximity(N=4, D=64)
    model = ap_lstm.create((T, 40), num_lstm_units=16, seed=6)
    _check_step(model, lambda m: Trainer(m, loss=loss, feature=dict(plan=plan, kind=nv.FEAT_LOGMEL)), sig, y,
                lambda z: _ap_loss_t(z, y, 4), feats=feats)


def test_optimizers_sgd_rmsprop_run():
    from lidbox_amd.models import lstm
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.standard_normal((4, 12, 6)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, 3, 4).astype(np.int32)).cuda()
    for opt in ({"cls": "SGD", "lr": 0.05, "momentum": 0.9}, {"cls": "RMSprop"}):
        m = lstm.create((12, 6), 3, num_units=20, seed=0)
        w0 = m.get_weights()
        tr = Trainer(m, optimizer=opt)
        losses = [float(tr.train_step(x, y)) for _ in range(5)]
        assert np.isfinite(losses).all() and losses[-1] < losses[0]
        assert any(not np.array_equal(w0[n], v) for n, v in m.get_weights().items())


# ---------------------------------------------------------------------------------------------------- KerasWrapper, HDF5
def test_keras_wrapper_trains_ap_lstm(tmp_path):
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.rnn import RecurrentModel
    from lidbox_amd.testutil import synthetic_batch
    plan = audio.get_plan(16000, 400, 160)
    data = []
    for seed in range(3):
        sig, y = synthetic_batch(16, num_labels=4, duration_s=0.5, seed=100 + seed)
        f = plan.run(nv.FEAT_LOGMEL, torch.from_numpy(sig).cuda()).cpu()
        data.append((f, torch.from_numpy(y.astype(np.int32))))
    T = data[0][0].shape[1]
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "ap", "model": {"key": "ap_lstm", "kwargs": {"num_lstm_units": 16, "seed": 3}},
        "input_shape": [T, 40], "output_shape": [4],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseAngularProximity", "kwargs": {"N": 4, "D": 64}},
        "metrics": [], "callbacks": []}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, RecurrentModel)
    hist = w.fit(data, data[:1], {"epochs": 2, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 2 and np.isfinite(loss).all() and loss[1] < loss[0]


def test_hdf5_fixture_loads_into_ap_lstm():
    import sys
    from lidbox_amd.models import ap_lstm
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_lstm_h5 import AP_LSTM_LAYERS, C, H
    from make_keras_h5 import values
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_ap_lstm_weights.h5"))
    model = ap_lstm.create((20, C), num_lstm_units=H, seed=0)
    model.set_weights(w)
    for _, vars_ in AP_LSTM_LAYERS:
        for wname, shape in vars_:
            parts = wname.split("/")
            key = parts[1] + {"kernel:0": ".W", "recurrent_kernel:0": ".U", "bias:0": ".b"}[parts[-1]]
            assert np.array_equal(model.get_weights()[key], values(wname, shape))
    x = np.random.default_rng(0).standard_normal((3, 20, C)).astype(np.float32)
    _, fwd = _torch_model(model, w)
    ref = torch.nn.functional.normalize(fwd(x), dim=1).detach().numpy()
    got = model(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(got - ref).max() <= H_TOL
