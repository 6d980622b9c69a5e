"""
GPU tests of the multilevel_attention model (lidbox_amd.models.multilevel_attention) against a float64 torch restatement of
reference lidbox/models/multilevel_attention.py written below: per level Dense on every frame, BatchNormalization over the
B*T rows (batch mean, population variance, eps 1e-3, momentum 0.99), ReLU, Dropout, and the attention pooling
softmax -> clip(1e-7, 1 - 1e-7) -> renormalise over time -> sigmoid-weighted sum over time; Concatenate, Dense, log-softmax.
The restatement takes the applied dropout masks as data: the same dropout call on a buffer of ones with the level's key.

Tolerances: H_TOL = 5e-5 absolute on logits and outputs, G_TOL = 1e-4 relative L2 on every parameter gradient: the bounds of
the bi_gru and spherespeaker model tests.  Measured maxima (MI355X): small model with dropout 0.4 2.2e-7 on logits, 2.0e-7 on
log-probs, 5.0e-7 on gradients (attention2_input.b); without dropout 9.6e-8 / 2.7e-7 / 3.8e-7; L = 3 2.7e-7 / 3.1e-7 / 3.4e-7;
H = 512 2.0e-7 / 2.8e-7 / 4.1e-7 (dense_block2_fc.W); K = 1 1.5e-7 / 0 / 2.3e-7.
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
LO = float(np.float32(1e-7))
HI = float(np.float32(1 - 1e-7))
HERE = os.path.dirname(os.path.abspath(__file__))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)


def _torch_model(weights, L):
    """float64 restatement: returns (params dict of leaf tensors, fwd(x, training, masks) -> (logits, {bn name: (batch mean,
    population variance)})); masks: per level the applied dropout factors [B*T, H], or None"""
    p = {k: _t(v) for k, v in weights.items()}
    pre_bn = {}            # bias name -> the Dense output it is added to (training passes): see _gradient_errors

    def fwd(x, training, masks=None):
        stats = {}
        pre_bn.clear()
        y = torch.from_numpy(np.asarray(x, np.float64))
        B, T, _ = y.shape
        atts = []
        for l in range(1, L + 1):
            a = y @ p["dense_block%d_fc.W" % l] + p["dense_block%d_fc.b" % l]
            if training:
                a.retain_grad()
                pre_bn["dense_block%d_fc.b" % l] = a
            name = "dense_block%d_bn" % l
            flat = a.reshape(B * T, -1)
            if training:
                mean, var = flat.mean(0), flat.var(0, unbiased=False)
                stats[name] = (mean.detach().numpy(), var.detach().numpy())
            else:
                mean, var = p[name + ".moving_mean"].detach(), p[name + ".moving_variance"].detach()
            y = torch.relu((a - mean) / torch.sqrt(var + 1e-3) * p[name + ".gamma"] + p[name + ".beta"])
            if training and masks is not None:
                y = y * torch.from_numpy(np.asarray(masks[l - 1], np.float64)).reshape(B, T, -1)
            z = y @ p["attention%d_input.W" % l] + p["attention%d_input.b" % l]
            c = torch.clamp(torch.softmax(z, -1), LO, HI)
            q = c / c.sum(1, keepdim=True)
            atts.append((q * torch.sigmoid(z)).sum(1))
        return torch.cat(atts, 1) @ p["outputs.W"] + p["outputs.b"], stats
    fwd.pre_bn = pre_bn
    return p, fwd


def _gradient_errors(model, p, pre_bn):
    """relative L2 error of every parameter gradient.  A `dense_block{l}_fc` bias is added in front of a training-mode
    BatchNormalization, which subtracts the batch mean again: its exact gradient is zero, the column sum over the B*T rows of
    a gradient da whose columns cancel, and what float64 returns for it is its own rounding noise.  A relative error against
    noise says nothing, so for these biases the scale is the norm of the same column sums without the cancellation,
    || sum_rows |da| ||, which is what the rounding error of a cancelling sum is proportional to."""
    errs = {}
    for n in model.layout:
        got, ref = model.param(n, grad=True).cpu().numpy().astype(np.float64), p[n].grad.numpy()
        if n in pre_bn:
            da = pre_bn[n].grad.numpy()
            scale = np.linalg.norm(np.abs(da).reshape(-1, da.shape[-1]).sum(0))
            errs[n] = float(np.linalg.norm(got - ref) / max(scale, 1e-30))
        else:
            errs[n] = _rel(got, ref)
    return errs


def _small(seed=2, T=15, D=8, K=5, H=24, L=2, **kw):
    from lidbox_amd.models import multilevel_attention
    return multilevel_attention.create((T, D), K, L=L, H=H, seed=seed, **kw)


def _randomise_state(model, rng):
    for n, (_, shape) in model.state_layout.items():
        v = rng.uniform(0.5, 1.5, shape) if n.endswith("variance") else rng.standard_normal(shape) * 0.3
        model.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    for n, (_, shape) in model.layout.items():
        if n.endswith(".gamma") or n.endswith(".beta"):
            base = 1.0 if n.endswith(".gamma") else 0.0
            model.param(n).copy_(torch.from_numpy((base + rng.standard_normal(shape) * 0.1).astype(np.float32)))


def _masks(model, R, step=None):
    """the dropout factors every level applies for the device step `step` (None: 0): lidbox_dropout_rows on ones with the key"""
    from lidbox_amd import _native as nv
    from lidbox_amd.models.tdnn import _rows
    if model.dropout_rate == 0:
        return None
    st = torch.tensor([step], dtype=torch.int64, device="cuda") if step is not None else None
    out = []
    for l in range(model.levels):
        ones = torch.ones((R, model.units), device="cuda")
        nv.check(nv.lib.lidbox_dropout_rows(_rows(ones.data_ptr(), 0, model.units, 1, R), model.units, model.dropout_rate,
                                            model.level_dropout_seed(l), nv.ptr(st), nv.current_stream()))
        out.append(ones.cpu().numpy())
    return out


def _train_forward_backward(model, B, T, rng, tag):
    D, K = model.input_dim, model.output_dim
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    G = rng.standard_normal((B, K)).astype(np.float32)
    w0 = model.get_weights()
    ws = model.workspace(B, T)
    model._load_input(ws, torch.from_numpy(x).cuda(), False)
    out = model.forward_ws(ws, training=True)
    logits = ws.h[-1].clone()
    ws.dh[-1].copy_(torch.from_numpy(G).cuda())
    model.backward_ws(ws)
    torch.cuda.synchronize()
    masks = _masks(model, B * T)
    p, fwd = _torch_model(w0, model.levels)
    ref, stats = fwd(x, True, masks)
    (ref * torch.from_numpy(G.astype(np.float64))).sum().backward()
    e_logits = float(np.abs(logits.cpu().numpy() - ref.detach().numpy()).max())
    e_logp = float(np.abs(out.cpu().numpy() - torch.log_softmax(ref.detach(), 1).numpy()).max())
    errs = _gradient_errors(model, p, fwd.pre_bn)
    worst = max(errs, key=errs.get)
    print("multilevel_attention %s: |logits - ref| = %.3e, |logp - ref| = %.3e, max rel L2 gradient error = %.3e (%s)"
          % (tag, e_logits, e_logp, errs[worst], worst))
    assert e_logits <= H_TOL and e_logp <= H_TOL
    for n, e in errs.items():
        assert e <= G_TOL, (n, e)
    return w0, stats, masks


@pytest.mark.parametrize("rate", [0.4, 0.0])
def test_train_forward_backward_matches_torch(rate):
    rng = np.random.default_rng(3)
    B, T = 6, 15
    model = _small(dropout_rate=rate)
    _randomise_state(model, rng)
    w0, stats, masks = _train_forward_backward(model, B, T, rng, "small, dropout %.1f" % rate)
    if rate > 0:
        kept = [float((m != 0).mean()) for m in masks]
        assert all(0.4 < k < 0.8 for k in kept) and not np.array_equal(masks[0], masks[1])
        ws = model.workspace(B, T)
        for l, m in enumerate(masks):                                  # the model applied exactly these masks
            assert (ws.y[l].cpu().numpy()[m == 0] == 0).all()
    # one training pass moves the running statistics once, towards batch mean / population variance
    w1 = model.get_weights()
    assert sorted(stats) == ["dense_block1_bn", "dense_block2_bn"]
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.99 * w0[name + ".moving_mean"] + 0.01 * mean, rtol=1e-5, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 * w0[name + ".moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-6), name
    # ... and inference not at all
    x = rng.standard_normal((B, T, 8)).astype(np.float32)
    model(torch.from_numpy(x).cuda())
    w2 = model.get_weights()
    assert all(np.array_equal(w1[n], w2[n]) for n in model.state_layout)


def test_three_levels_forward_backward_matches_torch():
    """L = 3: the middle level's output gradient is the attention branch plus the next level's Dense"""
    rng = np.random.default_rng(4)
    model = _small(seed=8, L=3)
    _randomise_state(model, rng)
    _train_forward_backward(model, 6, 15, rng, "L = 3")


def test_reference_widths_forward_backward_matches_torch():
    from lidbox_amd.models import multilevel_attention
    rng = np.random.default_rng(5)
    model = multilevel_attention.create((20, 40), 10, seed=4)
    assert model.units == 512 and model.levels == 2 and model.dropout_rate == 0.4
    _randomise_state(model, rng)
    _train_forward_backward(model, 4, 20, rng, "H = 512, L = 2")


def test_single_output_forward_backward_matches_torch():
    """K = 1: every softmax is 1, clipped from above, so only the sigmoid branch carries gradient"""
    rng = np.random.default_rng(6)
    model = _small(seed=9, K=1)
    _randomise_state(model, rng)
    _train_forward_backward(model, 6, 15, rng, "K = 1")


def test_inference_outputs_match_torch_for_every_activation():
    rng = np.random.default_rng(4)
    B, T, D = 5, 15, 8
    model = _small(seed=5)
    _randomise_state(model, rng)
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    w0 = model.get_weights()
    _, fwd = _torch_model(w0, 2)
    ref = fwd(x, False)[0].detach()
    got = model(torch.from_numpy(x).cuda()).cpu().numpy()
    assert got.shape == (B, 5)
    assert np.abs(got - torch.log_softmax(ref, 1).numpy()).max() <= H_TOL
    for act, f in ((None, lambda z: z), ("softmax", lambda z: torch.softmax(z, 1))):
        m2 = _small(seed=5, output_activation=act)
        m2.set_weights(w0)
        assert np.abs(m2(torch.from_numpy(x).cuda()).cpu().numpy() - f(ref).numpy()).max() <= H_TOL
    assert all(np.array_equal(w0[n], v) for n, v in model.get_weights().items())


def test_empty_batch_and_second_shape():
    """B = 0 is a no-op; a second (B, T) gets its own workspace and the first one still works"""
    rng = np.random.default_rng(6)
    D, K = 8, 5
    model = _small(seed=7)
    _randomise_state(model, rng)
    _, fwd = _torch_model(model.get_weights(), 2)
    assert tuple(model(torch.zeros((0, 15, D), device="cuda")).shape) == (0, K)
    ws = model.workspace(0, 15)
    model.forward_ws(ws, training=True)
    model.backward_ws(ws)
    outs = {}
    for B, T in ((3, 15), (5, 9), (3, 15), (2, 1)):
        x = np.random.default_rng(B * 100 + T).standard_normal((B, T, D)).astype(np.float32)
        got = model(torch.from_numpy(x).cuda()).cpu().numpy()
        ref = torch.log_softmax(fwd(x, False)[0].detach(), 1).numpy()
        assert np.abs(got - ref).max() <= H_TOL, (B, T)
        if (B, T) in outs:
            assert np.array_equal(outs[(B, T)], got)
        outs[(B, T)] = got
    assert len(model._ws) == 4


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
        if n.endswith("_fc.b"):
            # exact gradient zero (see _gradient_errors): Adam divides rounding noise by its own size, in either precision
            continue
        g = p[n].grad.numpy()
        big = np.abs(g) > 1e-3 * max(1e-30, np.abs(g).max())
        assert np.abs((w1[n] - w0[n]) - (want[n] - w0[n]))[big].max() <= 2e-5, n


def test_trainer_step_graph_equals_eager_and_matches_torch():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(9)
    B, T, D, K = 8, 15, 8, 5
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    y = rng.integers(0, K, B).astype(np.int32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    res = []
    for graph in (True, False):
        m = _small(seed=1)
        assert m.dropout_rate == 0.4
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
    # the first step reads the optimizer step 0
    p, fwd = _torch_model(w0, 2)
    ref, _ = fwd(x, True, _masks(m, B * T, step=0))
    loss = torch.nn.functional.cross_entropy(ref, torch.from_numpy(y.astype(np.int64)))
    loss.backward()
    ref_loss = float(loss.detach())
    assert abs(lg[0] - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
    _check_step(m.layout, p, w0, w1)


def test_dropout_masks_differ_between_graph_replays_and_between_levels():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(13)
    B, T, D, K = 8, 15, 8, 5
    xd = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
    yd = torch.from_numpy(rng.integers(0, K, B).astype(np.int32)).cuda()
    m = _small(seed=4, H=64)
    tr = Trainer(m, use_graph=True)
    ws = m.workspace(B, T)
    seen = []
    for step in range(3):
        tr.train_step(xd, yd)
        torch.cuda.synchronize()
        assert tr.step_count == step + 1
        ys = [t.cpu().numpy() for t in ws.y]
        masks = _masks(m, B * T, step=step)                   # the forward pass of this replay read the step before its update
        for l in range(2):
            assert (ys[l][masks[l] == 0] == 0).all(), (step, l)
            assert (ys[l][masks[l] != 0] > 0).mean() > 0.2, (step, l)
        seen.append(masks)
    for a, b in ((seen[0][0], seen[1][0]), (seen[1][0], seen[2][0]), (seen[0][1], seen[1][1]),      # replays
                 (seen[0][0], seen[0][1]), (seen[2][0], seen[2][1])):                              # levels
        differ = float(((a != 0) != (b != 0)).mean())
        assert 0.4 < differ < 0.56, differ                    # independent masks of rate 0.4 differ at 0.48 of the elements


def test_moving_statistics_advance_once_per_step_not_in_warmup():
    """the captured Trainer runs a warm-up pass before capture: the running statistics must show one update per real step"""
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(10)
    B, T, D, K = 8, 12, 8, 4
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    y = rng.integers(0, K, B).astype(np.int32)
    m = _small(seed=6, T=T, K=K)
    w0 = m.get_weights()
    tr = Trainer(m, use_graph=True)
    tr.train_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    w1 = m.get_weights()
    _, fwd = _torch_model(w0, 2)
    _, stats = fwd(x, True, _masks(m, B * T, step=0))
    assert sorted(stats) == ["dense_block1_bn", "dense_block2_bn"]
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.01 * mean, rtol=1e-4, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 + 0.01 * var, rtol=1e-5, atol=1e-6), name


def test_loss_falls_on_separable_problem():
    """the construction of the spherespeaker test (data, Adam at 3e-3, 30 steps, half the first loss), on the reference's
    width H = 512: the attention outputs are sigmoid-bounded, and the float64 restatement above under the same optimizer
    takes the loss from 1.44 to 0.40 at H = 512 but only from 1.50 to 1.01 at the H = 24 of the other tests"""
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(11)
    B, T, D, K = 32, 20, 8, 4
    y = rng.integers(0, K, B).astype(np.int32)
    centres = rng.standard_normal((K, D)).astype(np.float32) * 2
    x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((B, T, D))).astype(np.float32)
    m = _small(seed=3, T=T, K=K, H=512)
    tr = Trainer(m, optimizer={"cls": "Adam", "lr": 3e-3})
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    losses = [float(tr.train_step(xd, yd)) for _ in range(30)]
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses


def test_keras_wrapper_trains_and_checkpoints(tmp_path):
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.multilevel_attention import MultilevelAttentionModel
    rng = np.random.default_rng(12)
    T, D, K = 20, 12, 3
    data = []
    centres = rng.standard_normal((K, D)).astype(np.float32) * 2
    for _ in range(3):
        y = rng.integers(0, K, 16).astype(np.int32)
        x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((16, T, D))).astype(np.float32)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "mla",
        "model": {"key": "multilevel_attention", "kwargs": {"L": 2, "H": 32, "seed": 3}},
        "input_shape": [T, D], "output_shape": [K],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseCategoricalCrossentropy", "kwargs": {"from_logits": True}},
        "metrics": [], "callbacks": [{"cls": "ModelCheckpoint"}]}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, MultilevelAttentionModel) and w.keras_model.units == 32
    hist = w.fit(data, data[:1], {"epochs": 2, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 2 and np.isfinite(loss).all() and loss[-1] < loss[0]
    ckdir = os.path.join(ku.experiment_cache_from_config(cfg), "checkpoints")
    names = sorted(os.listdir(ckdir))
    assert len(names) == 2
    trained = w.keras_model.get_weights()
    w2 = ku.KerasWrapper.from_config(cfg)
    w2.load_weights(os.path.join(ckdir, names[-1]))
    assert w2.initial_epoch == 2
    loaded = w2.keras_model.get_weights()
    assert sorted(loaded) == sorted(trained)
    for n in trained:                                               # parameters and moving statistics
        assert np.array_equal(trained[n], loaded[n]), n
    x = data[0][0].cuda()
    assert torch.equal(w.keras_model(x), w2.keras_model(x))


# ---------------------------------------------------------------------------------------------------- HDF5
def test_hdf5_fixture_loads_into_model(tmp_path):
    import shutil
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models import multilevel_attention
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_keras_multilevel_attention_h5 as fx
    from make_keras_h5 import values
    path = os.path.join(HERE, "golden", "keras_multilevel_attention_weights.h5")
    x = np.random.default_rng(0).standard_normal((3, 20, fx.D)).astype(np.float32)
    model = multilevel_attention.create((20, fx.D), fx.K, L=fx.L, H=fx.H, seed=0)
    ku._set_weights_checked(model, ku.read_model_weights(model, path), path)
    ckpt = os.path.join(str(tmp_path), "epoch000007__val_loss0.500000000000.h5")
    shutil.copy(path, ckpt)
    wrapper = ku.KerasWrapper(multilevel_attention.create((20, fx.D), fx.K, L=fx.L, H=fx.H, seed=1), "multilevel_attention", [])
    wrapper.load_weights(ckpt)
    assert wrapper.initial_epoch == 7
    for m in (model, wrapper.keras_model):
        got = m.get_weights()
        for _, vars_ in fx.MULTILEVEL_ATTENTION_LAYERS:
            for wname, shape in vars_:
                assert np.array_equal(got[fx.expected_name(wname)], values(wname, shape)), wname
        _, fwd = _torch_model(got, fx.L)
        ref = torch.log_softmax(fwd(x, False)[0], 1).detach().numpy()
        out = m(torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.abs(out - ref).max() <= H_TOL
