"""
GPU tests of the spherespeaker model (lidbox_amd.models.spherespeaker) against a float64 torch transcription of reference
lidbox/models/spherespeaker.py written below: three Bidirectional LSTMs whose output sequences are concatenated,
BatchNormalization over the B*T rows (batch mean, population variance, eps 1e-3, momentum 0.99), Dense + ReLU per frame, time
average, BatchNormalization over the B rows, L2 normalisation (x / sqrt(max(sum x^2, 1e-12))), Dense, log-softmax.

Tolerances: H_TOL = 5e-5 absolute on logits, log-probs and embeddings, G_TOL = 1e-4 relative L2 on every parameter gradient:
the bounds of the bi_gru model test (tests/test_gru_gpu.py), which also has the LSTM-like recurrence and two
BatchNormalization layers in front of the loss.  First measured maxima (MI355X): small model (20 units, embedding 24,
B = 6, T = 15) 1.5e-7 on logits, 2.9e-7 on log-probs, 1.14e-6 on gradients (blstm_1_backward.b); the reference's widths (250 /
1000, B = 4, T = 20) 2.6e-8, 3.4e-7 and 1.13e-6 (blstm_3_backward.b).  The gradient figure is 88x under the bound, not 100x:
it is about 10 fp32 ulps, on LSTM bias gradients, which are column sums over B*T rows of mixed sign of a gradient that has
come through the L2 normalisation and two BatchNormalization backward passes, each of which subtracts the projections
mean(dy) and xhat * mean(dy * xhat) from dy, so rounding errors made before the cancellation are measured against what is
left after it.  The layer on its own (tests/test_lstm_step_gpu.py) is at 3.3e-7.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H_TOL = 5e-5
G_TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


def _torch_model(weights):
    """float64 transcription of spherespeaker.py: returns (params dict of leaf tensors, fwd(x, training) -> (logits,
    l2_normalize output, {bn name: (batch mean, population variance)}))"""
    p = {k: _t(v) for k, v in weights.items()}

    def lstm(x, prefix, reverse):
        W, U, b = p[prefix + ".W"], p[prefix + ".U"], p[prefix + ".b"]
        B, T, _ = x.shape
        H = U.shape[0]
        xp = x @ W + b
        h = torch.zeros((B, H), dtype=torch.float64)
        c = torch.zeros((B, H), dtype=torch.float64)
        outs = [None] * T
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            z = xp[:, t] + h @ U
            i, f = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H])
            g, o = torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            outs[t] = h
        return torch.stack(outs, 1)

    def fwd(x, training):
        stats = {}

        def bn(v, name):
            flat = v.reshape(-1, v.shape[-1])
            if training:
                mean, var = flat.mean(0), flat.var(0, unbiased=False)
                stats[name] = (mean.detach().numpy(), var.detach().numpy())
            else:
                mean, var = p[name + ".moving_mean"].detach(), p[name + ".moving_variance"].detach()
            return (v - mean) / torch.sqrt(var + 1e-3) * p[name + ".gamma"] + p[name + ".beta"]

        s = torch.from_numpy(np.asarray(x, np.float64))
        seqs = []
        for i in (1, 2, 3):
            s = torch.cat([lstm(s, "blstm_%d_forward" % i, False), lstm(s, "blstm_%d_backward" % i, True)], dim=2)
            seqs.append(s)
        a = bn(torch.cat(seqs, dim=2), "blstm_bn")
        a = torch.relu(a @ p["fc_relu.W"] + p["fc_relu.b"]).mean(1)
        a = bn(a, "pool_bn")
        emb = a / torch.sqrt(torch.clamp((a * a).sum(1, keepdim=True), min=1e-12))
        return emb @ p["outputs.W"] + p["outputs.b"], emb, stats
    return p, fwd


def _small(seed=2, T=15, C=8, N=5, H=20, E=24, **kw):
    from lidbox_amd.models import spherespeaker
    return spherespeaker.create((T, C), N, embedding_dim=E, seed=seed, num_lstm_units=H, **kw)


def _randomise_state(model, rng):
    for n, (_, shape) in model.state_layout.items():
        v = rng.uniform(0.5, 1.5, shape) if n.endswith("variance") else rng.standard_normal(shape) * 0.3
        model.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    for n, (_, shape) in model.layout.items():
        if n.endswith(".gamma") or n.endswith(".beta"):
            base = 1.0 if n.endswith(".gamma") else 0.0
            model.param(n).copy_(torch.from_numpy((base + rng.standard_normal(shape) * 0.1).astype(np.float32)))


def _train_forward_backward(model, B, T, C, N, rng, tag):
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
    p, fwd = _torch_model(w0)
    ref, _, stats = fwd(x, True)
    (ref * torch.from_numpy(G.astype(np.float64))).sum().backward()
    e_logits = float(np.abs(logits.cpu().numpy() - ref.detach().numpy()).max())
    e_logp = float(np.abs(out.cpu().numpy() - torch.log_softmax(ref.detach(), 1).numpy()).max())
    errs = {n: _rel(model.param(n, grad=True).cpu().numpy(), p[n].grad.numpy()) for n in model.layout}
    worst = max(errs, key=errs.get)
    print("spherespeaker %s: |logits - ref| = %.3e, |logp - ref| = %.3e, max rel L2 gradient error = %.3e (%s)"
          % (tag, e_logits, e_logp, errs[worst], worst))
    assert e_logits <= H_TOL and e_logp <= H_TOL
    for n, e in errs.items():
        assert e <= G_TOL, (n, e)
    return w0, stats


def test_spherespeaker_train_forward_backward_matches_torch():
    rng = np.random.default_rng(3)
    B, T, C, N = 6, 15, 8, 5
    model = _small()
    _randomise_state(model, rng)
    w0, stats = _train_forward_backward(model, B, T, C, N, rng, "small")
    # one training pass moves the running statistics once, towards the population statistics
    w1 = model.get_weights()
    assert sorted(stats) == ["blstm_bn", "pool_bn"]
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.99 * w0[name + ".moving_mean"] + 0.01 * mean, rtol=1e-5, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 * w0[name + ".moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-6), name


def test_spherespeaker_real_size_forward_backward_matches_torch():
    """the reference's widths: 250 LSTM units (the 8-byte load path of the step kernel), embedding_dim 1000"""
    from lidbox_amd.models import spherespeaker
    rng = np.random.default_rng(5)
    B, T, C, N = 4, 20, 40, 10
    model = spherespeaker.create((T, C), N, seed=4)
    assert model.units == 250 and model.embedding_dim == 1000
    _randomise_state(model, rng)
    _train_forward_backward(model, B, T, C, N, rng, "250 / 1000")


def test_spherespeaker_inference_and_embedding_match_torch():
    from lidbox_amd.models import spherespeaker
    rng = np.random.default_rng(4)
    B, T, C = 5, 15, 8
    model = _small(seed=5)
    _randomise_state(model, rng)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    w0 = model.get_weights()
    _, fwd = _torch_model(w0)
    ref, emb_ref, _ = fwd(x, False)
    got = model(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.abs(got - torch.log_softmax(ref.detach(), 1).numpy()).max() <= H_TOL
    emb = spherespeaker.as_embedding_extractor(model)(torch.from_numpy(x).cuda()).cpu().numpy()
    assert emb.shape == (B, 24)
    assert np.abs(emb - emb_ref.detach().numpy()).max() <= H_TOL
    assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1).max() <= 1e-6          # unit norm
    w1 = model.get_weights()
    assert all(np.array_equal(w0[n], w1[n]) for n in model.state_layout)      # inference leaves the statistics alone
    # logits and probabilities
    for act, f in ((None, lambda z: z), ("softmax", lambda z: torch.softmax(z, 1))):
        m2 = _small(seed=5, output_activation=act)
        m2.set_weights({k: v for k, v in w0.items() if k in m2.layout})
        for n in m2.state_layout:
            m2.param(n).copy_(torch.from_numpy(w0[n]))
        assert np.abs(m2(torch.from_numpy(x).cuda()).cpu().numpy() - f(ref.detach()).numpy()).max() <= H_TOL


def test_spherespeaker_empty_batch_and_second_shape():
    """B = 0 is a no-op; a second (B, T) gets its own workspace and the first one still works"""
    rng = np.random.default_rng(6)
    C, N = 8, 5
    model = _small(seed=7)
    _randomise_state(model, rng)
    _, fwd = _torch_model(model.get_weights())
    assert tuple(model(torch.zeros((0, 15, C), device="cuda")).shape) == (0, N)
    ws = model.workspace(0, 15)
    model.forward_ws(ws, training=True)
    model.backward_ws(ws)
    outs = {}
    for B, T in ((3, 15), (5, 9), (3, 15)):
        x = np.random.default_rng(B * 100 + T).standard_normal((B, T, C)).astype(np.float32)
        got = model(torch.from_numpy(x).cuda()).cpu().numpy()
        ref = torch.log_softmax(fwd(x, False)[0].detach(), 1).numpy()
        assert np.abs(got - ref).max() <= H_TOL, (B, T)
        if (B, T) in outs:
            assert np.array_equal(outs[(B, T)], got)
        outs[(B, T)] = got
    assert len(model._ws) == 3


# ---------------------------------------------------------------------------------------------------- training
def _keras_adam(p, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """one tf.keras Adam step from zero moments (t = 1) on float64 leaves with .grad"""
    lr_t = lr * math.sqrt(1 - b2) / (1 - b1)
    out = {}
    for n, t in p.items():
        g = t.grad.numpy()
        m, v = (1 - b1) * g, (1 - b2) * g * g
        out[n] = t.detach().numpy() - lr_t * m / (np.sqrt(v) + eps)
    return out


def _check_step(layout, p, w0, w1):
    """the rule of tests/test_rnn_gpu.py: an Adam step is ~lr * sign(g), so compare where the gradient is not vanishingly small"""
    want = _keras_adam({n: p[n] for n in layout})
    for n in layout:
        g = p[n].grad.numpy()
        big = np.abs(g) > 1e-3 * max(1e-30, np.abs(g).max())
        assert np.abs((w1[n] - w0[n]) - (want[n] - w0[n]))[big].max() <= 2e-5, n


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
        losses, after_first = [], None
        for i in range(3):
            losses.append(float(tr.train_step(xd, yd)))
            if i == 0:
                torch.cuda.synchronize()
                after_first = m.get_weights()
        torch.cuda.synchronize()
        res.append((losses, m.get_weights(), after_first))
    (lg, wg, w1), (le, we, _) = res
    assert lg == le
    for n in wg:
        assert np.array_equal(wg[n], we[n]), n
    p, fwd = _torch_model(w0)
    ref, _, _ = fwd(x, True)
    loss = torch.nn.functional.cross_entropy(ref, torch.from_numpy(y.astype(np.int64)))
    loss.backward()
    ref_loss = float(loss.detach())
    assert abs(lg[0] - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
    _check_step(m.layout, p, w0, w1)


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
    _, fwd = _torch_model(w0)
    _, _, stats = fwd(x, True)
    assert sorted(stats) == ["blstm_bn", "pool_bn"]
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


def test_keras_wrapper_trains_spherespeaker(tmp_path):
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.spherespeaker import SphereSpeakerModel
    rng = np.random.default_rng(12)
    T, C, N = 20, 12, 3
    data = []
    centres = rng.standard_normal((N, C)).astype(np.float32) * 2
    for _ in range(3):
        y = rng.integers(0, N, 16).astype(np.int32)
        x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((16, T, C))).astype(np.float32)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "sphere",
        "model": {"key": "spherespeaker", "kwargs": {"num_lstm_units": 16, "embedding_dim": 32, "seed": 3}},
        "input_shape": [T, C], "output_shape": [N],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseCategoricalCrossentropy", "kwargs": {"from_logits": True}},
        "metrics": [], "callbacks": []}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, SphereSpeakerModel)
    hist = w.fit(data, data[:1], {"epochs": 2, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 2 and np.isfinite(loss).all() and loss[-1] < loss[0]


# ---------------------------------------------------------------------------------------------------- HDF5
def test_hdf5_fixture_loads_into_spherespeaker(tmp_path):
    import shutil
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models import spherespeaker
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_keras_spherespeaker_h5 as fx
    from make_keras_h5 import values
    path = os.path.join(HERE, "golden", "keras_spherespeaker_weights.h5")
    x = np.random.default_rng(0).standard_normal((3, 20, fx.C)).astype(np.float32)
    # through read_weights_file with the rule the model asks for ...
    model = spherespeaker.create((20, fx.C), fx.N, embedding_dim=fx.E, seed=0, num_lstm_units=fx.H)
    ku._set_weights_checked(model, ku.read_weights_file(path, blstm_by_wrapper=model.keras_blstm_by_wrapper), path)
    # ... and through KerasWrapper.load_weights, which passes the model's wish along
    ckpt = os.path.join(str(tmp_path), "epoch000007__val_loss0.500000000000.h5")
    shutil.copy(path, ckpt)
    wrapper = ku.KerasWrapper(spherespeaker.create((20, fx.C), fx.N, embedding_dim=fx.E, seed=1, num_lstm_units=fx.H),
                              "spherespeaker", [])
    wrapper.load_weights(ckpt)
    assert wrapper.initial_epoch == 7
    for m in (model, wrapper.keras_model):
        got = m.get_weights()
        for _, vars_ in fx.SPHERESPEAKER_LAYERS:
            for wname, shape in vars_:
                assert np.array_equal(got[fx.expected_name(wname)], values(wname, shape)), wname
        _, fwd = _torch_model(got)
        ref = torch.log_softmax(fwd(x, False)[0], 1).detach().numpy()
        out = m(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.abs(out - ref).max() <= H_TOL
