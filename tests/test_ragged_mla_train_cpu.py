"""
Host side of the ragged train step of multilevel_attention (no GPU): lidbox_mla_attention_ragged_bwd in the header and the
ctypes table, its refusals in the no-compute form, the refusals of Trainer.train_step_ragged / loss_and_grads_ragged, the
register budget of the ragged backward kernels, and the float64 evidence for the feature: the restatement of the ragged
training computation (tests/ragged_mla_train_cases.py) equals the dense one at equal lengths, and a zero-padded batch gives
other gradients.
"""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import ragged_mla_cases as rc
import ragged_mla_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lidbox_mla_attention_ragged_bwd"


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


def test_symbol_declared_and_bound(nv):
    header = open(os.path.join(ROOT, "include", "lidbox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % SYMBOL, header)
    assert m and len(m.group(1).split(",")) == 12, SYMBOL
    assert SYMBOL in nv._SIGS and len(nv._SIGS[SYMBOL][1]) == 12
    assert getattr(nv.lib, SYMBOL).argtypes == nv._SIGS[SYMBOL][1]
    assert nv.lib.lidbox_hip_abi_version() == 1


def test_refusals_before_any_launch(nv):
    """no-compute form: host memory stands in for device buffers; every call below is refused, or returns for an empty batch,
    before anything touches a device"""
    buf = np.full(64, 3.0, np.float32)
    off = np.array([0, 2, 5], np.int64)
    p, o = buf.ctypes.data, off.ctypes.data

    def call(z=p, ro=o, B=2, max_T=3, K=4, att=p, ld_att=4, cs=p, datt=p, ld_datt=4, dz=p):
        return nv.lib.lidbox_mla_attention_ragged_bwd(z, ro, B, max_T, K, att, ld_att, cs, datt, ld_datt, dz, None)

    for kw in (dict(z=None), dict(ro=None), dict(att=None), dict(cs=None), dict(datt=None), dict(dz=None), dict(B=-1), dict(B=2 ** 31),
               dict(K=0), dict(K=-3), dict(K=1025, ld_att=1025, ld_datt=1025), dict(ld_att=3), dict(ld_datt=3), dict(max_T=0),
               dict(max_T=-1), dict(z=None, max_T=0)):
        assert call(**kw) == -1, kw
        assert SYMBOL in nv.last_error(), (kw, nv.last_error())
    with pytest.raises(ValueError):
        nv.check(call(ld_datt=3))
    assert call(B=0) == 0 and call(B=0, max_T=0) == 0
    assert (buf == 3.0).all() and off.tolist() == [0, 2, 5]


def test_trainer_refusals_are_raised_on_the_host(nv, monkeypatch):
    """the model lives on the CPU device and the one device check is stood in for (tests/test_ragged_mla_cpu.py), so a refusal
    that reached a launch would fail otherwise; no workspace exists afterwards and the step counter has not moved"""
    from lidbox_amd.models import multilevel_attention as mla
    from lidbox_amd.train import Trainer
    m = mla.create((50, 8), 5, H=24, device="cpu", seed=0)
    tr = Trainer(m)
    assert callable(m.forward_ragged_train) and callable(m.backward_ragged) and callable(m.ragged_train_workspace)
    X, y = torch.zeros((9, 8)), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(nv.LidboxHipError):
        tr.train_step_ragged(X, [0, 4, 9], y)
    monkeypatch.setattr(nv, "require_gpu_tensor", lambda t, name, dtype=None: t)
    for call in (tr.train_step_ragged, tr.loss_and_grads_ragged):
        with pytest.raises(ValueError, match="length 0"):
            call(X, [0, 9, 9], y)
        with pytest.raises(ValueError, match="row_offsets"):
            call(X, [0, 4], y)
        with pytest.raises(ValueError, match=r"\[total_T, 8\]"):
            call(torch.zeros((9, 7)), [0, 4, 9], y)
        with pytest.raises(ValueError, match="at least one utterance"):
            call(X[:0], [0], y[:0])
        with pytest.raises(ValueError, match="labels"):
            call(X, [0, 4, 9], torch.zeros(3, dtype=torch.int32))
        with pytest.raises(ValueError, match="labels"):
            call(X, [0, 4, 9], torch.zeros((2, 1), dtype=torch.int32))
        tr.sync.active = True
        with pytest.raises(ValueError, match="gradient exchange"):
            call(X, [0, 4, 9], y)
        tr.sync.active = False
        tr.feature = dict(plan=None, kind=0)
        with pytest.raises(ValueError, match="feature= front-end"):
            call(X, [0, 4, 9], y)
        tr.feature = None
        tr.model = types.SimpleNamespace(name="x-vector")
        with pytest.raises(ValueError, match="x-vector.*no ragged training pass"):
            call(X, [0, 4, 9], y)
        tr.model = m
    assert getattr(m, "_rtws", None) is None and tr.step_count == 0


def _resource_usage(build, tmp_path, name):
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, name + ".hip"),
                                         "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--offload-arch=gfx950" in cmd
    usage, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and fn:
            usage[fn] = int(m.group(1))
    return usage


def test_ragged_backward_kernels_build_for_gfx950_without_scratch(nv, tmp_path):
    """eight ragged beside the eight dense backward instantiations, one per (VEC, NJ) pair, none with scratch; the dispatch
    macro of the new entry point is not one the launch-site reader of the oracle takes for a dense site"""
    from lidbox_amd import build
    from oracle import update_paths_np as up
    usage = _resource_usage(build, tmp_path, "mla")
    pairs = lambda kernel: {tuple(int(v) for v in re.search(r"ILi(\d+)ELi(\d+)EEE", k).groups()): s
                            for k, s in usage.items() if re.search(r"\d%sI" % kernel, k)}
    ragged, dense = pairs("mla_attention_ragged_bwd_kernel"), pairs("mla_attention_bwd_kernel")
    assert set(ragged) == set(dense) == rc.ALL_PAIRS, sorted(usage)
    assert all(s == 0 for s in ragged.values()), ragged
    assert all(s == 0 for s in dense.values()), dense
    sites = {k for k in up.launch_site_kernels() if k.startswith("mla_attention_")}
    assert len(sites) == 16 and not any("ragged" in k for k in sites)
    # the K values of the device tests reach every pair (backward: vec4 also needs an aligned dz, which the tests give it)
    assert {(p["vec"], p["nj"]) for p in (up.mla_plan(K, K % 4 == 0 and not s) for K, s in rc.KERNEL_KS)} == rc.ALL_PAIRS


def test_the_capped_batch_takes_a_second_trip_of_the_row_loop():
    """256 utterances at K = 100, lengths 1 .. 298: gy = cdiv(2048, 256) = 8 workgroups of 16 rows cover 128 rows a trip"""
    from oracle import update_paths_np as up
    p = up.mla_bwd_plan(256, 298, 100, True)
    assert (p["vec"], p["nj"], p["rows_per_wg"], p["gy"], p["trips"]) == (4, 1, 16, 8, 3)
    assert up.mla_bwd_plan(7, 298, 100, True)["trips"] == 1


# ---------------------------------------------------------------------------------------------------- float64
_F64 = {}


def _ragged_case(case):
    """float64, dropout off: (weights, utterances, labels, leaves, loss, pre_bn, probs) of the ragged restatement on MODEL_LENGTHS"""
    if case not in _F64:
        c = rc.MODEL_CASES[case]
        w, xs, _, _ = rc.model_reference(case)
        y = tc.labels_for(len(xs), c["K"])
        p = tc.params64(tc.trainable(w))
        logits, _, pre_bn, probs = tc.ragged64(p, c["L"], np.concatenate(xs), tc.offsets([len(x) for x in xs]))
        loss = tc.mean_nll(logits, y)
        loss.backward()
        _F64[case] = (w, xs, y, p, float(loss.detach()), pre_bn, probs)
    return _F64[case]


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_inputs_keep_every_probability_away_from_the_clip_bounds(case):
    c = rc.MODEL_CASES[case]
    assert tc.away_from_the_clip_bounds(_ragged_case(case)[6])
    w = rc.model_weights(**c)
    p = tc.params64(tc.trainable(w))
    assert tc.away_from_the_clip_bounds(tc.dense64(p, c["L"], tc.equal_inputs(c["D"]))[3])


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_at_equal_lengths_the_ragged_restatement_is_the_dense_one(case):
    c = rc.MODEL_CASES[case]
    w = tc.trainable(rc.model_weights(**c))
    x, y = tc.equal_inputs(c["D"]), tc.labels_for(tc.EQ_B, c["K"])
    masks = [np.random.default_rng(l).choice([0.0, 1.0 / 0.6], (tc.EQ_B * tc.EQ_T, c["H"]), p=[0.4, 0.6]) for l in range(c["L"])]
    res = []
    for fn, arg in ((tc.dense64, (x,)), (tc.ragged64, (x.reshape(-1, c["D"]), tc.offsets([tc.EQ_T] * tc.EQ_B)))):
        p = tc.params64(w)
        logits, stats, _, _ = fn(p, c["L"], *arg, masks=masks)
        loss = tc.mean_nll(logits, y)
        loss.backward()
        res.append((logits.detach().numpy(), float(loss.detach()), {n: t.grad.numpy() for n, t in p.items()}, stats))
    (ld, sd, gd, std), (lr, sr, gr, str_) = res
    assert np.abs(ld - lr).max() <= 1e-12 and abs(sd - sr) <= 1e-12
    for n in gd:
        assert np.abs(gd[n] - gr[n]).max() <= 1e-12 * max(1.0, np.abs(gd[n]).max()), n
    for n in std:
        assert np.abs(std[n][0] - str_[n][0]).max() <= 1e-12 and np.abs(std[n][1] - str_[n][1]).max() <= 1e-12


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_a_zero_padded_batch_gives_other_gradients(case):
    """the point of the feature, in float64 alone: the gradients of the batch zero-padded to 298 frames against those of the
    ragged computation, relative L2 per parameter, far above the G_TOL the device is held to.  The `dense_block{l}_fc.b` are
    left out: their exact gradient is zero on both routes (the BatchNormalization subtracts the batch mean the bias moved),
    so both sides hold rounding noise there and a difference between two noises says nothing."""
    c = rc.MODEL_CASES[case]
    w, xs, y, p, loss, pre_bn, _ = _ragged_case(case)
    q = tc.params64(tc.trainable(w))
    logits, _, _, _ = tc.dense64(q, c["L"], tc.padded_batch(xs))
    pad_loss = tc.mean_nll(logits, y)
    pad_loss.backward()
    diffs = {n: tc.rel(q[n].grad.numpy(), p[n].grad.numpy()) for n in p if n not in pre_bn}
    worst = min(diffs, key=diffs.get)
    print("%s: zero-padded vs ragged float64 gradients, relative L2: smallest %.3e (%s), largest %.3e; loss %.6f vs %.6f"
          % (case, diffs[worst], worst, max(diffs.values()), float(pad_loss.detach()), loss))
    assert len(diffs) == len(p) - c["L"]
    for n, d in diffs.items():
        assert d > 100 * tc.G_TOL, (n, d)
    for n in pre_bn:                                      # exact zeros on both routes
        scale = np.linalg.norm(np.abs(pre_bn[n].grad.numpy()).sum(0))
        assert np.linalg.norm(p[n].grad.numpy()) <= 1e-12 * scale and np.linalg.norm(q[n].grad.numpy()) <= 1e-9
