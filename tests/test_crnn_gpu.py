"""
GPU tests of the crnn model (lidbox_amd.models.crnn / conv_rnn) against a float64 transcription of reference
lidbox/models/crnn.py, built literally in the reference's image orientation: the input [B, T, F] is reshaped to [B, T, F, 1]
and permuted to an image with height = frequency and width = time, the Conv2D kernel [kh, kw, C_in, C_out] runs over
(frequency, time), MaxPool2D(2) pools that image, and the result is permuted back to [B, T5, F5 * C] for the BLSTM.  The
BLSTM is the Keras LSTM cell (gate order i, f, c, o), the loss Keras' SparseCategoricalCrossentropy(from_logits=False) on
the softmax output plus the l2(weight_decay) kernel penalties.

Tolerances, set from the first measured errors (MI355X) with a margin of about 10x: model outputs (probabilities) at most
5.2e-7 absolute (the HDF5 fixture's weights; 3.2e-7 for the random models at 37 x 33 and 100 x 70, both modes) -> H_TOL =
5e-6; gradients at most 6.4e-6 relative L2 over all parameters (blstm_backward.U at 100 x 70; 3.0e-6 at 37 x 33, 4.5e-6 for
the log_softmax case) -> G_TOL = 1e-4 (about 15x).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

H_TOL = 5e-6
G_TOL = 1e-4
HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = (7, 5, 3, 3, 3)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _torch_model(weights, weight_decay):
    """float64 transcription of crnn.py: (params dict of leaf tensors, fwd(x, training) -> (logits, penalty, {bn: (mean,
    Bessel-corrected variance)}))"""
    p = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in weights.items()}

    def lstm(x, prefix, reverse):
        W, U, b = p[prefix + ".W"], p[prefix + ".U"], p[prefix + ".b"]
        B, T, _ = x.shape
        H = U.shape[0]
        h = torch.zeros((B, H), dtype=torch.float64)
        c = torch.zeros((B, H), dtype=torch.float64)
        for t in (range(T - 1, -1, -1) if reverse else range(T)):
            z = x[:, t] @ W + h @ U + b
            i, f = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H])
            c = f * c + i * torch.tanh(z[:, 2 * H:3 * H])
            h = torch.sigmoid(z[:, 3 * H:]) * torch.tanh(c)
        return h

    def fwd(x, training):
        stats = {}
        x = torch.from_numpy(np.asarray(x, np.float64))
        B, T, F = x.shape
        img = x.reshape(B, T, F, 1).permute(0, 2, 1, 3)                # Reshape + Permute((2, 1, 3)): NHWC [B, F, T, 1]
        img = img.permute(0, 3, 1, 2)                                   # NCHW for torch: [B, 1, F, T]
        penalty = 0
        for i, k in enumerate(KERNELS, start=1):
            W = p["conv_%d.W" % i]                                      # [kh (frequency), kw (time), C_in, C_out]
            z = torch.relu(Fn.conv2d(img, W.permute(3, 2, 0, 1), p["conv_%d.b" % i], padding=(k - 1) // 2))
            name = "conv_%d_bn" % i
            if training:
                mean = z.mean((0, 2, 3))
                var = z.var((0, 2, 3), unbiased=False)
                n = z.numel() // z.shape[1]
                stats[name] = (mean.detach().numpy(), var.detach().numpy() * n / (n - 1))
            else:
                mean, var = p[name + ".moving_mean"].detach(), p[name + ".moving_variance"].detach()
            v = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + 1e-3)
            v = v * p[name + ".gamma"][None, :, None, None] + p[name + ".beta"][None, :, None, None]
            img = Fn.max_pool2d(v, 2)
            penalty = penalty + weight_decay * (W * W).sum()
        # Permute((2, 1, 3)) of NHWC [B, F5, T5, C] -> [B, T5, F5, C] -> Reshape [B, T5, F5 * C]
        nhwc = img.permute(0, 2, 3, 1)
        seq = nhwc.permute(0, 2, 1, 3).reshape(B, nhwc.shape[2], -1)
        h = torch.cat([lstm(seq, "blstm_forward", False), lstm(seq, "blstm_backward", True)], dim=1)
        return h @ p["output.W"] + p["output.b"], penalty, stats
    return p, fwd


def _small(T=37, F=33, N=5, seed=2, H=6, filters=(16, 16, 16, 32, 16), **kw):
    from lidbox_amd.models import crnn
    return crnn.create((T, F), N, seed=seed, num_units=H, filters=filters, **kw)


def _randomise(model, rng):
    for n, (_, shape) in model.state_layout.items():
        v = rng.uniform(0.5, 1.5, shape) if n.endswith("variance") else rng.standard_normal(shape) * 0.3
        model.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    for n, (_, shape) in model.layout.items():
        if n.endswith(".gamma") or n.endswith(".beta") or (n.startswith("conv_") and n.endswith(".b")):
            base = 1.0 if n.endswith(".gamma") else 0.0
            v = base + rng.standard_normal(shape) * 0.2
            if n.endswith(".gamma"):
                v[::3] *= -1                                          # negative gamma: the maximum does not commute with BN
            model.param(n).copy_(torch.from_numpy(v.astype(np.float32)))


def _probs_loss(logits, y):
    q = torch.softmax(logits, 1).clamp(1e-7, 1 - 1e-7)
    return -torch.log(q[torch.arange(len(y)), torch.from_numpy(y.astype(np.int64))]).mean()


# (T, F) of the whole-model comparisons: 37 x 33 pools down to T5 = F5 = 1; 100 x 70 leaves T5 = 3 and F5 = 2, so the BLSTM
# walks several steps (dU non-zero, the final-state rows and the h_prev offsets matter) and the flatten order f * C + c matters
SHAPES = [(37, 33), (100, 70)]


@pytest.mark.parametrize("T,F", SHAPES)
def test_crnn_forward_matches_reference_train_and_inference(T, F):
    rng = np.random.default_rng(3)
    B = 3
    model = _small(T=T, F=F)
    _randomise(model, rng)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    w0 = model.get_weights()
    _, fwd = _torch_model(w0, 0.001)
    for training in (False, True):
        ref = torch.softmax(fwd(x, training)[0], 1).detach().numpy()
        got = model(torch.from_numpy(x).cuda(), training=training).cpu().numpy()
        assert got.shape == (B, 5)
        print("forward T=%d F=%d training=%d max abs err %.3g" % (T, F, training, np.abs(got - ref).max()))
        assert np.abs(got - ref).max() <= H_TOL, (training, np.abs(got - ref).max())


@pytest.mark.parametrize("T,F", SHAPES)
def test_crnn_gradients_and_moving_statistics_match_reference(T, F):
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(4)
    B, N = 4, 5
    model = _small(T=T, F=F, seed=4)
    _randomise(model, rng)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    w0 = model.get_weights()
    tr = Trainer(model, loss="sparse_categorical_crossentropy_probs", use_graph=False)
    loss, g = tr.loss_and_grads(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    p, fwd = _torch_model(w0, 0.001)
    logits, penalty, stats = fwd(x, True)
    ref = _probs_loss(logits, y) + penalty
    ref.backward()
    assert abs(float(loss) - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    errs = {n: _rel(model.param(n, grad=True).cpu().numpy(), p[n].grad.numpy()) for n in model.layout}
    print("gradients T=%d F=%d max rel L2 err %.3g (%s)" % (T, F, max(errs.values()), max(errs, key=errs.get)))
    for n, e in errs.items():
        assert e <= G_TOL, (n, e)
    if model.workspace(B, T).T5 > 1:
        for half in ("blstm_forward", "blstm_backward"):
            assert np.abs(p[half + ".U"].grad.numpy()).max() > 1e-4      # the recurrence is exercised, not 0 against 0
    # one captured Trainer step: updated weights (Adam's first step) and moving statistics moved once
    tr = Trainer(model, loss="sparse_categorical_crossentropy_probs", use_graph=True)
    tr.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    w1 = model.get_weights()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-7
    lr_t = lr * np.sqrt(1 - b2) / (1 - b1)
    for n in model.layout:
        gr = p[n].grad.numpy()
        want = w0[n] - lr_t * ((1 - b1) * gr) / (np.sqrt((1 - b2) * gr * gr) + eps)
        big = np.abs(gr) > 1e-3 * np.abs(gr).max()                   # Adam's first step is ~lr sign(g): only where g is not tiny
        assert np.allclose(w1[n][big], want[big], rtol=0, atol=2e-6), n
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.99 * w0[name + ".moving_mean"] + 0.01 * mean, rtol=1e-5, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 * w0[name + ".moving_variance"] + 0.01 * var, rtol=1e-5,
                           atol=1e-6), name


def test_crnn_log_softmax_loss_and_no_regularizer():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(5)
    B, T, F, N = 3, 100, 70, 4
    model = _small(T=T, F=F, N=N, seed=5, output_activation="log_softmax", weight_decay=0)
    assert model.regularizers == []
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    w0 = model.get_weights()
    loss, _ = Trainer(model, use_graph=False).loss_and_grads(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    p, fwd = _torch_model(w0, 0.0)
    logits, _, _ = fwd(x, True)
    ref = Fn.cross_entropy(logits, torch.from_numpy(y.astype(np.int64)))
    ref.backward()
    assert abs(float(loss) - ref.item()) <= 1e-5 * max(1.0, ref.item())
    errs = {n: _rel(model.param(n, grad=True).cpu().numpy(), p[n].grad.numpy()) for n in model.layout}
    print("log_softmax gradients T=%d F=%d max rel L2 err %.3g (%s)" % (T, F, max(errs.values()), max(errs, key=errs.get)))
    for n, e in errs.items():
        assert e <= G_TOL, (n, e)


def test_crnn_captured_step_equals_uncaptured():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(6)
    B, T, F, N = 4, 40, 36, 3
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    res = []
    for graph in (True, False):
        m = _small(T=T, F=F, N=N, seed=1)
        tr = Trainer(m, loss="sparse_categorical_crossentropy_probs", use_graph=graph)
        losses = [float(tr.train_step(x, y)) for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, m.get_weights()))
    (lg, wg), (le, we) = res
    assert lg == le
    for n in wg:
        assert np.array_equal(wg[n], we[n]), n


def test_crnn_waveform_input_through_feature_trainer():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    from lidbox_amd.testutil import synthetic_batch
    from lidbox_amd.train import Trainer
    sig, y = synthetic_batch(4, num_labels=3, duration_s=0.5)
    plan = audio.get_plan(16000, 400, 160)
    sd, yd = torch.from_numpy(sig).cuda(), torch.from_numpy(y).cuda()
    feats = plan.run(nv.FEAT_LOGMEL, sd).contiguous()
    T, F = feats.shape[1], feats.shape[2]
    ma, mb = _small(T=T, F=F, N=3, seed=7), _small(T=T, F=F, N=3, seed=7)
    la, ga = Trainer(ma, loss="sparse_categorical_crossentropy_probs", feature=dict(plan=plan, kind=nv.FEAT_LOGMEL),
                     use_graph=False).loss_and_grads(sd, yd)
    lb, gb = Trainer(mb, loss="sparse_categorical_crossentropy_probs", use_graph=False).loss_and_grads(feats, yd)
    torch.cuda.synchronize()
    assert abs(float(la) - float(lb)) <= 1e-6 * abs(float(lb))
    assert _rel(ga.cpu().numpy(), gb.cpu().numpy()) <= 1e-5
    tr = Trainer(ma, loss="sparse_categorical_crossentropy_probs", feature=dict(plan=plan, kind=nv.FEAT_LOGMEL), use_graph=True)
    losses = [float(tr.train_step(sd, yd)) for _ in range(3)]
    assert np.isfinite(losses).all()


def test_crnn_keras_wrapper(tmp_path):
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.conv_rnn import ConvRecurrentModel
    rng = np.random.default_rng(12)
    T, F, N = 32, 32, 3
    centres = rng.standard_normal((N, F)).astype(np.float32) * 2
    data = []
    for _ in range(3):
        y = rng.integers(0, N, 8).astype(np.int32)
        x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((8, T, F))).astype(np.float32)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "crnn",
        "model": {"key": "crnn", "kwargs": {"num_units": 8, "filters": [16, 16, 16, 16, 16], "seed": 3}},
        "input_shape": [T, F], "output_shape": [N],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseCategoricalCrossentropy", "kwargs": {"from_logits": False}},
        "metrics": [], "callbacks": []}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, ConvRecurrentModel)
    hist = w.fit(data, data[:1], {"epochs": 3, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 3 and np.isfinite(loss).all() and loss[-1] < loss[0]
    # evaluate includes the kernel penalty, as Keras does
    logs = w.evaluate(data[:1])
    out = w.keras_model(data[0][0].cuda()).cpu()
    q = out.double().clamp(1e-7, 1 - 1e-7)
    ce = float(-torch.log(q[torch.arange(8), data[0][1].long()]).mean())
    pen = sum(0.001 * float((v.astype(np.float64) ** 2).sum()) for n, v in w.keras_model.get_weights().items()
              if n.startswith("conv_") and n.endswith(".W"))
    assert abs(logs["loss"] - (ce + pen)) <= 1e-4 * (ce + pen)


def test_hdf5_fixture_scores_like_reference():
    from lidbox_amd.models.keras_utils import read_weights_file, _set_weights_checked
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_crnn_h5 import FILTERS, F, H, N, T
    path = os.path.join(HERE, "golden", "keras_crnn_weights.h5")
    model = _small(T=T, F=F, N=N, H=H, filters=(FILTERS,) * 5)
    _set_weights_checked(model, read_weights_file(path), path)
    got_w = model.get_weights()
    # 100 frames: T5 = 3 BLSTM steps (the fixture's F = 32 fixes F5 = 1)
    x = np.random.default_rng(0).standard_normal((3, 100, F)).astype(np.float32)
    _, fwd = _torch_model(got_w, 0.001)
    ref = torch.softmax(fwd(x, False)[0], 1).detach().numpy()
    out = model(torch.from_numpy(x).cuda()).cpu().numpy()
    print("hdf5 fixture T=100 F=%d max abs err %.3g" % (F, np.abs(out - ref).max()))
    assert np.abs(out - ref).max() <= H_TOL


@pytest.mark.parametrize("seed", [0, 1])
def test_crnn_reference_property_random_shapes(seed):
    """reference tests/test_models.py:77 test_crnn: random inputs >= 32 x 32, N in 1..100, both modes"""
    rng = np.random.default_rng(100 + seed)
    T, F, N, B = int(rng.integers(32, 90)), int(rng.integers(32, 70)), int(rng.integers(1, 101)), int(rng.integers(1, 5))
    model = _small(T=T, F=F, N=N, seed=seed, H=16)
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).cuda()
    for training in (False, True):
        out = model(x, training=training)
        assert tuple(out.shape) == (B, N) and torch.isfinite(out).all()


def test_crnn_loss_falls_on_synthetic_logmels():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    from lidbox_amd.testutil import synthetic_batch
    from lidbox_amd.train import Trainer
    sig, y = synthetic_batch(16, num_labels=4, duration_s=0.5)
    plan = audio.get_plan(16000, 400, 160)
    feats = plan.run(nv.FEAT_LOGMEL, torch.from_numpy(sig).cuda()).contiguous()
    m = _small(T=feats.shape[1], F=feats.shape[2], N=4, seed=3)
    tr = Trainer(m, loss="sparse_categorical_crossentropy_probs", optimizer={"cls": "Adam", "lr": 3e-3})
    yd = torch.from_numpy(y).cuda()
    losses = [float(tr.train_step(feats, yd)) for _ in range(40)]
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses
