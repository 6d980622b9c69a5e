"""
GPU tests of the clstm model (lidbox_amd.models.clstm) against a float64 torch transcription of reference
lidbox/models/clstm.py written below: GaussianNoise and the channel Dropout (training only; the test reads the perturbed
input back from the model's workspace and feeds it to the transcription), Reshape to an image [B, T, F, 1] with height = time,
two Conv2D(f, (3, 9), strides=(1, 6), padding="same") -> BatchNormalization (fused 4-D path: batch statistics, Bessel-corrected
moving variance) -> ReLU, reduce_max over frequency (torch.amax splits the gradient over ties as TF does), the causal frame
layers, LSTM(512) with the Keras cell (gates i, f, c, o), frequency_attention(d_f=60), mean + stddev pooling, the segment
layers, Dense and log_softmax, with Keras' sparse categorical cross-entropy.

Tolerances, set from the first measured errors (MI355X) with a margin of about 10x: outputs at most 2.7e-7 absolute over
all flag rows, both modes (1.1e-7 for the HDF5 fixture) -> H_TOL = 3e-6; gradients at most 2.4e-6 relative L2 per parameter
(conv2d_1_bn.gamma, use_conv2d at T = 20, F = 40) -> G_TOL = 3e-5; moving statistics 1e-5 absolute.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

H_TOL = 3e-6
G_TOL = 3e-5
S_TOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = {"none": {}, "conv2d": dict(use_conv2d=True), "lstm": dict(use_lstm=True), "attention": dict(use_attention=True),
         "all": dict(use_conv2d=True, use_lstm=True, use_attention=True)}


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _same(n, k, s):
    out = -(-n // s)
    pad = max((out - 1) * s + k - n, 0)
    return pad // 2, pad - pad // 2


def _transcription(weights, flags):
    """float64 clstm.py: (leaf tensors, fwd(x [B, T, F] already perturbed, training) -> (log-probs, {bn: (mean, var_bessel)}))"""
    p = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(not k.endswith(("moving_mean", "moving_variance")))
         for k, v in weights.items()}

    def bn(x, name, training, stats):
        axes = tuple(range(x.dim() - 1))
        if training:
            mean, var = x.mean(axes), x.var(axes, unbiased=False)
            n = int(np.prod([x.shape[a] for a in axes]))
            stats[name] = (mean.detach().numpy(), var.detach().numpy() * n / max(n - 1, 1))
        else:
            mean, var = p[name + ".moving_mean"], p[name + ".moving_variance"]
        return (x - mean) / torch.sqrt(var + 1e-3) * p[name + ".gamma"] + p[name + ".beta"]

    def frame(x, name, k, s):
        W = p[name + ".W"].permute(2, 1, 0)                       # [C_out, C_in, k]
        y = Fn.conv1d(Fn.pad(x.transpose(1, 2), (k - 1, 0)), W, p[name + ".b"], stride=s)
        return torch.relu(y).transpose(1, 2)

    def lstm(x):
        B, T, _ = x.shape
        H = p["lstm.U"].shape[0]
        h = torch.zeros((B, H), dtype=torch.float64)
        c = torch.zeros_like(h)
        out = []
        for t in range(T):
            z = x[:, t] @ p["lstm.W"] + h @ p["lstm.U"] + p["lstm.b"]
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out.append(h)
        return torch.stack(out, 1)

    def fwd(x, training):
        stats = {}
        h = torch.as_tensor(np.asarray(x, np.float64))
        if flags.get("use_conv2d"):
            img = h.unsqueeze(-1)                                  # [B, T, F, 1]
            for l in (1, 2):
                n = "conv2d_%d" % l
                p0, p1 = _same(img.shape[2], 9, 6)
                y = Fn.conv2d(Fn.pad(img.permute(0, 3, 1, 2), (p0, p1, 1, 1)), p[n + ".W"].permute(3, 2, 0, 1), p[n + ".b"],
                              stride=(1, 6)).permute(0, 2, 3, 1)
                img = torch.relu(bn(y, n + "_bn", training, stats))
            h = img.amax(dim=2)
        h = frame(h, "frame1", 5, 1)
        h = frame(h, "frame2", 3, 2)
        h = frame(h, "frame3", 3, 3)
        if flags.get("use_lstm"):
            h = lstm(h)
        h = frame(h, "frame4", 1, 1)
        h = frame(h, "frame5", 1, 1)
        if flags.get("use_attention"):
            B, T, C = h.shape
            fa = torch.softmax(torch.relu(h @ p["Wf_1.W"]) @ p["Wf_2.W"], -1)
            h = (h.reshape(B, T, 60, C // 60) * fa.unsqueeze(-1)).reshape(B, T, C)
        mean = h.mean(1)
        var = ((h - mean.unsqueeze(1)) ** 2).mean(1)
        h = torch.cat([mean, torch.sqrt(torch.clamp(var, min=1e-10))], 1)
        h = torch.relu(h @ p["segment1.W"] + p["segment1.b"])
        h = torch.relu(h @ p["segment2.W"] + p["segment2.b"])
        return torch.log_softmax(h @ p["output.W"] + p["output.b"], 1), stats

    return p, fwd


def _model(flags, T, F, N=4, seed=0, **kw):
    from lidbox_amd.models import clstm
    return clstm.create((T, F), N, seed=seed, **flags, **kw)


CASES = [(f, T, F) for f in FLAGS for (T, F) in ((20, 40), (6, 20))]


@pytest.mark.parametrize("flag,T,F", CASES)
def test_clstm_matches_transcription(flag, T, F):
    from lidbox_amd.train import Trainer
    flags = FLAGS[flag]
    rng = np.random.default_rng(T + F)
    B, N = 3, 4
    m = _model(flags, T, F, N, seed=T)
    w0 = m.get_weights()
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    y = rng.integers(0, N, B).astype(np.int32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    # inference: no noise, no dropout, moving statistics
    p, fwd = _transcription(w0, flags)
    out = m(xd).cpu().numpy()
    ref = fwd(x, False)[0].detach().numpy()
    e_inf = float(np.abs(out - ref).max())
    # training-mode output: the perturbed input read back from the workspace
    m2 = _model(flags, T, F, N, seed=T)
    out_t = m2(xd, training=True).cpu().numpy()
    xin = m2.workspace(B, T).input_view().cpu().numpy()
    assert not np.array_equal(xin, x)
    ref_t = fwd(xin, True)[0].detach().numpy()
    e_tr = float(np.abs(out_t - ref_t).max())
    # gradients (Trainer probe: noise keyed by its step counter) and the moving statistics after one real step
    m3 = _model(flags, T, F, N, seed=T)
    tr = Trainer(m3, use_graph=False)
    loss, g = tr.loss_and_grads(xd, yd)
    xin = m3.workspace(B, T).input_view().cpu().numpy()
    p, fwd = _transcription(w0, flags)
    logp, stats = fwd(xin, True)
    lref = -logp[torch.arange(B), torch.from_numpy(y).long()].mean()
    lref.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - lref.item()) <= 1e-5 * abs(lref.item()), (float(loss), lref.item())
    gerr = {}
    for name, t in p.items():
        if t.requires_grad:
            got = m3.param(name, grad=True).cpu().numpy()
            if name.startswith("conv2d_") and name.endswith(".b"):
                # a bias in front of BatchNormalization has a zero gradient: measure against the BN shift's gradient
                gerr[name] = float(np.linalg.norm(got - t.grad.numpy()) / np.linalg.norm(p[name[:-2] + "_bn.beta"].grad.numpy()))
            else:
                gerr[name] = _rel(got, t.grad.numpy())
    worst = max(gerr, key=gerr.get)
    print("%s T=%d F=%d: inference %.3g, training %.3g, worst gradient %s %.3g" % (flag, T, F, e_inf, e_tr, worst, gerr[worst]))
    assert e_inf <= H_TOL and e_tr <= H_TOL
    assert gerr[worst] <= G_TOL, gerr
    if flags.get("use_conv2d"):
        tr.train_step(xd, yd)
        torch.cuda.synchronize()
        xin = m3.workspace(B, T).input_view().cpu().numpy()
        _, stats = _transcription(w0, flags)[1](xin, True)
        for bn, (mean, var) in stats.items():
            assert np.abs(m3.param(bn + ".moving_mean").cpu().numpy() - 0.01 * mean).max() <= S_TOL
            assert np.abs(m3.param(bn + ".moving_variance").cpu().numpy() - (0.99 + 0.01 * var)).max() <= S_TOL


def test_noise_and_mask_statistics():
    from lidbox_amd import _native as nv
    B, T, C = 64, 200, 40
    st = nv.current_stream()
    step = torch.zeros(1, dtype=torch.int64, device="cuda")

    def draw(seed, stddev=0.01, rate=0.4, x=None):
        x = torch.zeros((B, T, C), device="cuda") if x is None else x.clone()
        nv.check(nv.lib.lidbox_input_noise_dropout(nv.ptr(x), B, T, C, T * C, stddev, rate, seed, nv.ptr(step), st))
        return x

    a = draw(11)
    kept = (a != 0).any(dim=1)                                   # [B, C]: a channel is kept or dropped for all frames
    assert torch.equal((a == 0).all(dim=1), ~kept)
    frac = 1.0 - float(kept.float().mean())
    assert abs(frac - 0.4) <= 4 * np.sqrt(0.4 * 0.6 / (B * C))
    v = a.permute(0, 2, 1)[kept].double() * 0.6 / 0.01             # standard normal draws
    n = v.numel()
    assert abs(float(v.mean())) <= 5 / np.sqrt(n) and abs(float(v.std()) - 1.0) <= 5 / np.sqrt(n / 2)
    assert torch.equal(a, draw(11))                                # same seed, same step
    step += 1
    assert not torch.equal(a, draw(11))                            # the next step draws afresh
    # stddev 0: the bits of lidbox_spatial_dropout
    x = torch.randn((B, T, C), device="cuda")
    ref = x.clone()
    nv.check(nv.lib.lidbox_spatial_dropout(nv.ptr(ref), B, T, C, T * C, 0.4, 5, nv.ptr(step), None, st))
    assert torch.equal(draw(5, stddev=0.0, x=x), ref)


def test_no_noise_in_inference_and_bf16_rejected():
    m = _model(FLAGS["all"], 20, 40)
    x = torch.randn((2, 20, 40), device="cuda")
    assert torch.equal(m(x), m(x))
    with pytest.raises(ValueError):
        _model({}, 20, 40, compute_dtype="bfloat16")


def test_captured_step_equals_uncaptured_and_buckets():
    from lidbox_amd.train import Trainer
    rng = np.random.default_rng(6)
    B, T, F, N = 4, 30, 40, 3
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    res = []
    for graph, nb in ((True, 2), (False, 2), (False, 1)):
        m = _model(FLAGS["all"], T, F, N, seed=1)
        tr = Trainer(m, use_graph=graph, num_buckets=nb)
        losses = [float(tr.train_step(x, y)) for _ in range(3)]
        torch.cuda.synchronize()
        res.append((losses, m.get_weights(), tr.splits))
    assert res[0][2] and not res[2][2]                  # the default plan does split the gradient
    for losses, w, _ in res[1:]:
        assert losses == res[0][0]
        for n in w:
            assert np.array_equal(w[n], res[0][1][n]), n


def test_waveform_input_through_feature_trainer_and_loss_falls():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    from lidbox_amd.testutil import synthetic_batch
    from lidbox_amd.train import Trainer
    sig, y = synthetic_batch(8, num_labels=4, duration_s=0.5)
    plan = audio.get_plan(16000, 400, 160)
    sd, yd = torch.from_numpy(sig).cuda(), torch.from_numpy(y).cuda()
    feats = plan.run(nv.FEAT_LOGMEL, sd).contiguous()
    T, F = feats.shape[1], feats.shape[2]
    ma, mb = _model(FLAGS["all"], T, F, 4, seed=7), _model(FLAGS["all"], T, F, 4, seed=7)
    la, ga = Trainer(ma, feature=dict(plan=plan, kind=nv.FEAT_LOGMEL), use_graph=False).loss_and_grads(sd, yd)
    lb, gb = Trainer(mb, use_graph=False).loss_and_grads(feats, yd)
    torch.cuda.synchronize()
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb))
    assert _rel(ga.cpu().numpy(), gb.cpu().numpy()) <= 1e-4
    m = _model(FLAGS["all"], T, F, 4, seed=3, filters=(16, 32), frame_units=(64, 64, 64, 64, 120), segment_units=(64, 64))
    tr = Trainer(m, feature=dict(plan=plan, kind=nv.FEAT_LOGMEL), optimizer={"cls": "Adam", "lr": 3e-3})
    losses = [float(tr.train_step(sd, yd)) for _ in range(40)]
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.5 * losses[0], losses


def test_clstm_keras_wrapper(tmp_path):
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models.clstm import CLSTM
    rng = np.random.default_rng(12)
    T, F, N = 24, 40, 3
    centres = rng.standard_normal((N, F)).astype(np.float32) * 2
    data = []
    for _ in range(3):
        y = rng.integers(0, N, 8).astype(np.int32)
        x = (centres[y][:, None, :] + 0.5 * rng.standard_normal((8, T, F))).astype(np.float32)
        data.append((torch.from_numpy(x), torch.from_numpy(y)))
    cfg = {"experiment": {
        "cache_directory": str(tmp_path), "name": "clstm",
        "model": {"key": "clstm", "kwargs": {"use_conv2d": True, "use_lstm": True, "use_attention": True, "seed": 3,
                                             "filters": [16, 16], "frame_units": [32, 32, 32, 32, 60], "segment_units": [32, 32]}},
        "input_shape": [T, F], "output_shape": [N],
        "optimizer": {"cls": "Adam", "kwargs": {"learning_rate": 3e-3}},
        "loss": {"cls": "SparseCategoricalCrossentropy", "kwargs": {"from_logits": True}},
        "metrics": [], "callbacks": []}}
    w = ku.KerasWrapper.from_config(cfg)
    assert isinstance(w.keras_model, CLSTM)
    hist = w.fit(data, data[:1], {"epochs": 3, "verbose": 0})
    loss = hist["history"]["loss"]
    assert len(loss) == 3 and np.isfinite(loss).all() and loss[-1] < loss[0]
    logs = w.evaluate(data[:1])
    out = w.keras_model(data[0][0].cuda()).cpu().double()
    ce = float(-out[torch.arange(8), data[0][1].long()].mean())
    assert abs(logs["loss"] - ce) <= 1e-4 * ce
    pred = w.keras_model.predict(data[0][0].cuda())
    assert torch.equal(pred.cpu(), w.keras_model(data[0][0].cuda()).cpu())


def test_hdf5_fixture_scores_like_transcription():
    from lidbox_amd.models.keras_utils import read_weights_file, _set_weights_checked
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_clstm_h5 import F, FILTERS, FRAME_UNITS, N, SEGMENT_UNITS
    path = os.path.join(HERE, "golden", "keras_clstm_weights.h5")
    flags = FLAGS["all"]
    model = _model(flags, 30, F, N, filters=FILTERS, frame_units=FRAME_UNITS, segment_units=SEGMENT_UNITS)
    _set_weights_checked(model, read_weights_file(path), path)
    w = model.get_weights()
    x = np.random.default_rng(0).standard_normal((3, 30, F)).astype(np.float32)
    out = model(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = _transcription(w, flags)[1](x, False)[0].detach().numpy()
    print("hdf5 fixture max abs err %.3g" % np.abs(out - ref).max())
    assert np.abs(out - ref).max() <= H_TOL
