"""
Every dispatch path of the kernels that change the weights on a training step -- the second half of csrc/nnops.hip (the Adam,
SGD and RMSprop updates, the three dropout kernels, lidbox_cavg_result, lidbox_mean / _scale / _fill) and csrc/mla.hip (the
attention pool forward and backward, bn -> relu -> dropout forward and backward) -- through the C ABI, against the float64
references and the host restatement of the counter hash in oracle/update_paths_np.py.

The shapes sit in that module's PATHS tables, each row with the condition it is there for; tests/test_oracle_update_paths.py
proves on the CPU that every row selects what it says, that the float32 emulations stay inside the bounds and that every
planted mistake leaves them.

Buffers.  Every buffer is a tests/guarded.py payload.  Outputs start as NaN wherever the kernel must write; gaps between
utterances and rows hold NaN going in and the same NaN coming out; read-only inputs (gradients, z, att, colsum, datt, scale,
shift, counters, step counters) are compared bit for bit with their host copies after the call; every row runs twice and
must repeat bit for bit.

Judging.  Optimisers: every output array within its per-element bound after ONE step from a known float32 state, the step
counter exact, lr_t within one float32 ulp of the host's double evaluation; a 5-step trajectory at the tolerances of
tests/test_ops_gpu.py as a second check.  Masks: bit for bit against the host hash on every element, kept values equal to
fl(x fl(1 / (1 - rate))) bit for bit (the device's keep_scale is the correctly rounded quotient at every rate used).  Noise: within the Box-Muller bound.
bn_relu_dropout: bit-identical to lidbox_bn_relu_fwd / _bwd composed with lidbox_dropout_rows and within 1 ulp of the float64
reference.  Attention: att, colsum (relative) and dz (absolute) within the derived bounds, H_TOL / G_TOL of
tests/test_mla_ops_gpu.py kept as an outer limit.  cavg_result: out[0] and every c_avg_out[th] within the bound.  Exact
identities: lidbox_adam_step == prepare job + lidbox_adam_apply on every Adam row; equal elements give equal body and equal tail
outputs; an utterance alone, first and last in a batch; stddev 0 == lidbox_spatial_dropout; the same mask on ones and on a
gradient; NULL and given c_avg_out; empty calls write nothing but the step; refusals return -1 with the function's name and
write nothing.

First measured (MI355X, one run, 172 cases in 5.4 s, the slowest 0.55 s: bn_relu_dropout on 8.4 M elements), largest err / bound
per group.  Optimisers (the bounds count roundings, so a half-ulp rounding of the last sum on a mantissa near 1 comes close to
them): Adam param 0.999, m 0.942, v 0.986; SGD param 0.989, velocity 0.949; RMSprop param 0.995, rms 0.951, mean_grad 0.495,
mom 0.969; lr_t 0 ulp from the host value on every row, 2^33 steps included.  Noise 0.844 (stddev 0.01, where the two roundings
of (x + stddev n) m are most of the bound) and 0.357 (stddev 1).  bn_relu_dropout 0.883 of an ulp of 2^-23 |ref| (1.23 spacings
of ref, recorded only: oracle/update_paths_np.py ulp_distance) and bit-equal to the host prediction.  Attention att 0.088,
colsum 0.146, dz 0.349 at most (<4,1>); the instantiations no test had launched: <4,2> 0.056 / 0.104 / 0.133, <4,4> 0.050 /
0.073 / 0.128, <1,2> 0.061 / 0.107 / 0.183, <1,4> 0.056 / 0.093 / 0.158, <1,8> 0.065 / 0.104 / 0.148; the 64 KiB rows K = 512
and K = 1024 2.3e-7 and 2.1e-7 absolute on att; the largest |att - ref| 3.8e-7 (H_TOL 5e-5).  Vector and scalar paths on the same
data are both inside the bounds and NOT bit-equal (another lane layout, another summation order).  cavg_result 0.139 with the
LDS pre-pass, 0.196 without.  mean 0.109.  Every mask, scale, fill and every identity: bit-equal.  Adam with equal elements:
body == tail bits for param and v, not for m (the compiler contracts b1 m + (1 - b1) gr differently in the two loops; both are
inside the bound, which allows either).  No defect was found.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import update_paths_np as up

pytestmark = pytest.mark.gpu

WORST = {}                                           # group -> largest err / bound seen
NAN32 = np.float32(np.nan)
H_TOL, G_TOL = 5e-5, 1e-4                            # tests/test_mla_ops_gpu.py: the outer limit
SEED = up.DROP_SEED


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the module: nothing more is launched on a device that has reported a fault"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error after a test of this module: %s" % e, returncode=3)


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """bit for bit, NaN payloads included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _note(group, q):
    q = float(np.max(q)) if np.size(q) else 0.0
    WORST[group] = max(WORST.get(group, 0.0), q)
    return q


def _g(a, shift=0):
    """a guarded device copy of a float32 host array"""
    a = np.ascontiguousarray(a, np.float32)
    return Guarded(a.shape, init=torch.from_numpy(a), shift=shift)


def _nan(shape, shift=0):
    return Guarded(shape, shift=shift)


def _off(g, words):
    return ctypes.c_void_p(g.view.data_ptr() + 4 * words)


def _step_dev(step):
    return None if step is None else torch.tensor([step], dtype=torch.int64, device="cuda")


def _sp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _refused(st, fn):
    assert st == -1, (fn, st)
    assert fn in _nv().last_error(), (fn, _nv().last_error())


# ---------------------------------------------------------------------------------------------------- optimisers
def _state(step, lr_now):
    h = np.zeros(4, np.int32)
    h[:2].view(np.int64)[0] = step
    h[2] = 0x7FC00000                                                # lr_t must be written
    h[3] = np.float32(lr_now).view(np.int32)
    return _g(h.view(np.float32)), h


def _read_state(g):
    s = g.numpy().view(np.int32)
    return int(s[:2].view(np.int64)[0]), s[2:3].view(np.float32)[0], int(s[3])


def _opt_slots(kind, r):
    """(output name, key in opt_state's dict, argument used by the kernel)"""
    if kind == "adam":
        return [("m", "m", True), ("v", "v", True)]
    if kind == "sgd":
        used = up.SGD_VARIANTS[r["variant"]]["mu"] > 0
        return [("velocity", "velocity", used)]
    k = up.RMS_VARIANTS[r["variant"]]
    return [("rms", "v", True), ("mean_grad", "m", bool(k["centered"])), ("mom", "mom", k["mu"] > 0)]


def run_opt(kind, r, d, how="step", state=None):
    """one step through the C ABI; returns (outputs by name, step after, lr_t, the state buffer)"""
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    n = r["n"]
    cap = max(n, 4)                                                  # n = 0 still passes real pointers; the payload must stay NaN

    def pad(a):
        h = np.full(cap, NAN32, np.float32)
        h[:n] = a[:n]
        return h
    hp, hg = pad(d["param"]), pad(d["grad"])
    P, Gd = _g(hp), _g(hg)
    slots, hosts = {}, {}
    for name, key, used in _opt_slots(kind, r):
        if used:
            hosts[name] = pad(d[key])
            slots[name] = _g(hosts[name])
        elif n == 256:                                               # given but unused: must stay untouched
            hosts[name] = np.full(cap, NAN32, np.float32)
            slots[name] = _g(hosts[name])
        else:
            slots[name] = None
    if state is None:
        state, _ = _state(r.get("step", 3), r["lr_now"])
    ptr = {k: (v.ptr if v is not None else None) for k, v in slots.items()}
    h = up.HP[kind]
    if kind == "adam":
        if how == "step":
            nv.check(lib.lidbox_adam_step(P.ptr, Gd.ptr, ptr["m"], ptr["v"], n, h["lr"], h["b1"], h["b2"], h["eps"], r["gs"], state.ptr, st))
        else:
            jobs = (nv.ReduceJob * 1)()
            nv.check(lib.lidbox_adam_prepare_job(state.ptr, h["lr"], h["b1"], h["b2"], jobs))
            nv.check(lib.lidbox_reduce_jobs_run(jobs, 1, st))
            nv.check(lib.lidbox_adam_apply(P.ptr, Gd.ptr, ptr["m"], ptr["v"], n, h["b1"], h["b2"], h["eps"], r["gs"], state.ptr, st))
    elif kind == "sgd":
        k = up.SGD_VARIANTS[r["variant"]]
        nv.check(lib.lidbox_sgd_step(P.ptr, Gd.ptr, ptr["velocity"], n, h["lr"], k["mu"], k["nesterov"], r["gs"], state.ptr, st))
    else:
        k = up.RMS_VARIANTS[r["variant"]]
        nv.check(lib.lidbox_rmsprop_step(P.ptr, Gd.ptr, ptr["rms"], ptr["mean_grad"], ptr["mom"], n, h["lr"], h["rho"], k["mu"], h["eps"],
                                         k["centered"], r["gs"], state.ptr, st))
    torch.cuda.synchronize()
    assert _same(Gd.numpy(), hg), "the gradient was modified"
    outs = {}
    for name, gbuf in [("param", P)] + list(slots.items()):
        if gbuf is None:
            continue
        a = gbuf.numpy()
        assert np.isnan(a[n:]).all(), "%s: written past n" % name
        used = name == "param" or dict((s[0], s[2]) for s in _opt_slots(kind, r))[name]
        if used:
            outs[name] = a[:n].copy()
        else:
            assert _same(a, hosts[name]), "%s is not used by this variant and was written" % name
    step, lr_t, now_bits = _read_state(state)
    assert now_bits == int(np.float32(r["lr_now"]).view(np.int32)), "lr_now was modified"
    return outs, step, lr_t, state


OPT_CASES = [(k, r) for k in ("adam", "sgd", "rmsprop") for r in up.PATHS[k]]


@pytest.mark.parametrize("kind,r", OPT_CASES, ids=["%s-%s" % (k, r["name"]) for k, r in OPT_CASES])
def test_optimiser_row(kind, r):
    n = r["n"]
    d = up.opt_state(n, 11, zero=r.get("zero", False))
    outs, step, lr_t, _ = run_opt(kind, r, d)
    want_step, want_lr = up.opt_row_lr_t(kind, r)
    assert step == want_step, (step, want_step)
    ulps = abs(float(lr_t) - float(want_lr)) / float(np.spacing(np.float32(abs(want_lr)))) if want_lr != 0 else float(lr_t != 0)
    _note("%s lr_t ulp" % kind, ulps)
    assert ulps <= 1.0, (lr_t, want_lr)
    if kind != "adam":
        assert _same(lr_t, want_lr)                                  # no pow: the rate itself
    refs = up.opt_row_refs(kind, r, d, lr_t)
    assert set(refs) == set(outs)
    worst = {}
    for name, (ref, bound) in refs.items():
        got = outs[name]
        assert got.shape == (n,) and np.isfinite(got).all(), "%s not fully written" % name
        if n:
            q = np.abs(got.astype(np.float64) - ref) / bound
            worst[name] = _note("%s %s" % (kind, name), q)
            assert (q <= 1.0).all(), "%s %s: %d over the bound, worst %.3g x at %d" % (r["name"], name, (q > 1).sum(), q.max(), int(np.argmax(q)))
    print("%-8s %-24s step %d lr_t %.9g  err/bound %s" % (kind, r["name"], step, lr_t, {k: "%.3f" % v for k, v in worst.items()}))
    if want_lr == 0 and set(outs) <= {"param", "m", "v", "rms", "mean_grad"}:       # with momentum the carried step still moves param
        assert _same(outs["param"], d["param"]), "a rate of exactly 0 moved param"
        for name in sorted(set(outs) - {"param"}):
            assert n == 0 or not _same(outs[name], d[{"rms": "v", "mean_grad": "m"}.get(name, name)]), "%s did not move" % name
    again, step2, lr2, _ = run_opt(kind, r, d)
    assert step2 == step and _same(lr2, lr_t) and all(_same(outs[k], again[k]) for k in outs), "a second run gives other bits"
    if kind == "adam":
        job, step3, lr3, _ = run_opt(kind, r, d, how="job")
        assert step3 == step and _same(lr3, lr_t), "the prepare job publishes another step or lr_t"
        assert all(_same(outs[k], job[k]) for k in outs), "prepare job + adam_apply differs from adam_step"


def test_equal_elements_give_equal_body_and_equal_tail_outputs():
    n = up._ADAM_BIG
    d = {k: np.full(n, v, np.float32) for k, v in (("param", 0.7), ("grad", -0.3), ("m", 0.02), ("v", 0.04))}
    outs, _, _, _ = run_opt("adam", dict(n=n, gs=0.5, lr_now=0.0, step=3), d)
    n4 = (n >> 2) << 2
    for name, a in outs.items():
        b = _bits(a)
        assert (b[:n4] == b[0]).all(), "%s: body elements differ" % name
        assert (b[n4:] == b[n4]).all(), "%s: tail elements differ" % name
        # body and tail are the same expression: whether the compiler contracted both alike is recorded, not required
        print("adam equal elements %-5s body == tail: %s" % (name, bool(b[0] == b[n4])))


def test_five_step_trajectories_keep_the_existing_tolerances():
    from oracle import model_np as mo
    n = 1027
    rng = np.random.default_rng(16)
    w0 = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) for _ in range(5)]
    p, m, v = {"w": w0.astype(np.float64)}, {"w": np.zeros(n)}, {"w": np.zeros(n)}
    d = dict(param=w0, m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    state, _ = _state(0, 0.0)
    for t, gr in enumerate(grads, 1):
        mo.adam_step(p, {"w": gr.astype(np.float64) * 0.5}, m, v, t)
        d["grad"] = gr
        outs, step, _, state = run_opt("adam", dict(n=n, gs=0.5, lr_now=0.0), d, state=state)
        d.update(param=outs["param"], m=outs["m"], v=outs["v"])
        assert step == t and np.abs(outs["param"] - p["w"]).max() < 2e-6
    for variant, kw in (("plain", dict(momentum=0.0, nesterov=False)), ("momentum", dict(momentum=0.9, nesterov=False)),
                        ("nesterov", dict(momentum=0.9, nesterov=True))):
        p, vel = {"w": w0.astype(np.float64)}, {"w": np.zeros(n)}
        d = dict(param=w0, velocity=np.zeros(n, np.float32))
        state, _ = _state(0, 0.0)
        for gr in grads:
            mo.sgd_step(p, {"w": 0.1 * gr.astype(np.float64)}, vel, lr=up.HP["sgd"]["lr"], **kw)
            d["grad"] = gr
            outs, step, _, state = run_opt("sgd", dict(n=n, gs=0.1, lr_now=0.0, variant=variant), d, state=state)
            d.update(param=outs["param"], velocity=outs.get("velocity", d["velocity"]))
        assert step == 5 and np.abs(outs["param"] - p["w"]).max() <= 2e-6, variant
    for variant, kw in (("plain", dict()), ("momentum", dict(momentum=0.9)), ("centered", dict(centered=True)),
                        ("centered_momentum", dict(centered=True, momentum=0.9))):
        p, rms, mg, mm = {"w": w0.astype(np.float64)}, {"w": np.zeros(n)}, {"w": np.zeros(n)}, {"w": np.zeros(n)}
        d = dict(param=w0, v=np.zeros(n, np.float32), m=np.zeros(n, np.float32), mom=np.zeros(n, np.float32))
        state, _ = _state(0, 0.0)
        for gr in grads:
            mo.rmsprop_step(p, {"w": 0.1 * gr.astype(np.float64)}, rms, mg, mm, lr=up.HP["rmsprop"]["lr"], **kw)
            d["grad"] = gr
            outs, step, _, state = run_opt("rmsprop", dict(n=n, gs=0.1, lr_now=0.0, variant=variant), d, state=state)
            d.update(param=outs["param"], v=outs["rms"], m=outs.get("mean_grad", d["m"]), mom=outs.get("mom", d["mom"]))
        assert step == 5 and np.abs(outs["param"] - p["w"]).max() <= 5e-6, variant


# ---------------------------------------------------------------------------------------------------- spatial and noise dropout
def _utterances(r, seed):
    """x [B, T, C] and its gapped host buffer (NaN in the gaps); an empty shape still gets a four-word NaN payload"""
    B, T, C = r["B"], r["T"], r["C"]
    x = np.random.default_rng([seed, B, T, C]).standard_normal((B, T, C)).astype(np.float32)
    bs = T * C + r["gap"]
    host = np.full(max(B * bs, 4), NAN32, np.float32)
    if B * T * C:
        host[:B * bs].reshape(B, bs)[:, :T * C] = x.reshape(B, T * C)
    return x, host, bs


def _split_utts(buf, host, r, bs):
    B, T, C = r["B"], r["T"], r["C"]
    y = buf.numpy()
    live = np.zeros(len(y), bool)
    if B * T * C:
        live[:B * bs].reshape(B, bs)[:, :T * C] = True
    assert _same(y[~live], host[~live]) and np.isnan(y[~live]).all(), "a gap was written"
    return y[:B * bs].reshape(B, bs)[:, :T * C].reshape(B, T, C) if B * T * C else np.zeros((B, T, C), np.float32)


def run_spatial(r, rate, step, want_mask=True, stddev=None):
    nv = _nv()
    B, T, C = r["B"], r["T"], r["C"]
    x, host, bs = _utterances(r, 21)
    X = _g(host)
    M = _nan((max(B * C, 4),)) if want_mask else None
    sd = _step_dev(step)
    if stddev is None:
        st = nv.lib.lidbox_spatial_dropout(X.ptr, B, T, C, bs, rate, SEED, _sp(sd), M.ptr if M else None, nv.current_stream())
    else:
        st = nv.lib.lidbox_input_noise_dropout(X.ptr, B, T, C, bs, stddev, rate, SEED, _sp(sd), nv.current_stream())
    nv.check(st)
    torch.cuda.synchronize()
    assert sd is None or int(sd.item()) == step, "the step counter was modified"
    return x, _split_utts(X, host, r, bs), (M.numpy() if M else None)


@pytest.mark.parametrize("r", up.SPATIAL, ids=lambda r: r["name"])
def test_spatial_dropout_row(r):
    B, T, C = r["B"], r["T"], r["C"]
    for rate in up.DROP_RATES:
        plan = up.spatial_plan(B, T, C, rate)
        for step in up.DROP_STEPS:
            x, y, mask = run_spatial(r, rate, step)
            if not plan["launch"]:                                   # B = 0, T = 0 or rate 0: nothing is written, mask_out included
                assert _same(y, x) and np.isnan(mask).all(), (r["name"], rate)
                continue
            ref, mref = up.spatial_ref(x, rate, SEED, step or 0)
            assert _same(mask[:B * C].reshape(B, C), mref), "%s rate %g step %s: mask_out differs from the host hash" % (r["name"], rate, step)
            assert np.isnan(mask[B * C:]).all()
            assert _same(y, ref), "%s rate %g step %s: %d elements differ" % (r["name"], rate, step, int((_bits(y) != _bits(ref)).sum()))
            _, y2, m2 = run_spatial(r, rate, step)
            assert _same(y, y2) and _same(mask, m2)
            _, y3, _ = run_spatial(r, rate, step, want_mask=False)   # mask_out NULL
            assert _same(y, y3)
            _, y4, _ = run_spatial(r, rate, step, stddev=0.0)        # the noise kernel with stddev 0: the same bits
            assert _same(y, y4), "%s: stddev 0 is not lidbox_spatial_dropout" % r["name"]


@pytest.mark.parametrize("r", up.NOISE, ids=lambda r: r["name"])
def test_input_noise_dropout_row(r):
    B, T, C = r["B"], r["T"], r["C"]
    for stddev in up.NOISE_STDDEVS[1:]:                              # stddev 0: test_spatial_dropout_row
        for rate in up.DROP_RATES:
            for step in up.DROP_STEPS:
                x, y, _ = run_spatial(r, rate, step, want_mask=False, stddev=stddev)
                if not B * T * C:
                    assert y.size == 0
                    continue
                ref, bound = up.noise_ref(x, stddev, rate, SEED, step or 0)
                assert np.isfinite(y).all()
                dropped = bound == 0
                assert (y[dropped] == 0).all(), "a dropped element is not zero"
                q = np.abs(y.astype(np.float64) - ref)[~dropped] / bound[~dropped]
                _note("noise stddev %g" % stddev, q)
                assert (q <= 1.0).all(), "%s stddev %g rate %g step %s: worst %.3g x" % (r["name"], stddev, rate, step, q.max())
                _, y2, _ = run_spatial(r, rate, step, want_mask=False, stddev=stddev)
                assert _same(y, y2)


def test_dropout_limits_are_refused_before_any_launch():
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    X, M = _nan((64,)), _nan((64,))
    cases = [("lidbox_spatial_dropout", lambda: lib.lidbox_spatial_dropout(X.ptr, 65536, 1, 1, 1, 0.25, SEED, None, M.ptr, st)),
             ("lidbox_spatial_dropout", lambda: lib.lidbox_spatial_dropout(X.ptr, 2, 3, 5, 14, 0.25, SEED, None, M.ptr, st)),
             ("lidbox_spatial_dropout", lambda: lib.lidbox_spatial_dropout(X.ptr, 2, 3, 5, 15, 1.0, SEED, None, M.ptr, st)),
             ("lidbox_spatial_dropout", lambda: lib.lidbox_spatial_dropout(X.ptr, 2, 3, 0, 15, 0.25, SEED, None, M.ptr, st)),
             ("lidbox_spatial_dropout", lambda: lib.lidbox_spatial_dropout(None, 2, 3, 5, 15, 0.25, SEED, None, M.ptr, st)),
             ("lidbox_input_noise_dropout", lambda: lib.lidbox_input_noise_dropout(X.ptr, 65536, 1, 1, 1, 0.01, 0.25, SEED, None, st)),
             ("lidbox_input_noise_dropout", lambda: lib.lidbox_input_noise_dropout(X.ptr, 1, 65536, 65536, 1 << 32, 0.01, 0.25, SEED, None, st)),
             ("lidbox_input_noise_dropout", lambda: lib.lidbox_input_noise_dropout(X.ptr, 2, 3, 5, 15, -0.5, 0.25, SEED, None, st)),
             ("lidbox_input_noise_dropout", lambda: lib.lidbox_input_noise_dropout(X.ptr, 2, 3, 5, 15, 0.01, 1.0, SEED, None, st)),
             ("lidbox_dropout_rows", lambda: lib.lidbox_dropout_rows(nv.Rows(X.view.data_ptr(), 0, 5, 1, 3), 5, 1.0, SEED, None, st)),
             ("lidbox_dropout_rows", lambda: lib.lidbox_dropout_rows(nv.Rows(X.view.data_ptr(), 0, 5, 1, 3), 0, 0.25, SEED, None, st)),
             ("lidbox_dropout_rows", lambda: lib.lidbox_dropout_rows(nv.Rows(None, 0, 5, 1, 3), 5, 0.25, SEED, None, st))]
    for fn, call in cases:
        _refused(call(), fn)
    torch.cuda.synchronize()
    assert np.isnan(X.numpy()).all() and np.isnan(M.numpy()).all()
    assert not up.spatial_accepts(65536, 1, 1, 1) and not up.spatial_accepts(1, 65536, 65536, 1 << 32, noise=True)


# ---------------------------------------------------------------------------------------------------- dropout_rows
def _rows_layout(r):
    batch, rpb, C, gap = r["batch"], r["rpb"], r["C"], r["gap"]
    rs = C + gap
    bs = rpb * rs + gap
    total = batch * bs + 3
    idx = (np.arange(batch)[:, None, None] * bs + np.arange(rpb)[None, :, None] * rs + np.arange(C)[None, None, :]).reshape(batch * rpb, C)
    return rs, bs, total, idx


def run_rows(r, x, rate, step):
    nv = _nv()
    rs, bs, total, idx = _rows_layout(r)
    host = np.full(total, NAN32, np.float32)
    host[idx] = x
    X = _g(host)
    sd = _step_dev(step)
    nv.check(nv.lib.lidbox_dropout_rows(nv.Rows(X.view.data_ptr(), bs, rs, r["batch"], r["rpb"]), r["C"], rate, SEED, _sp(sd), nv.current_stream()))
    torch.cuda.synchronize()
    y = X.numpy()
    live = np.zeros(total, bool)
    live[idx] = True
    assert _same(y[~live], host[~live]), "a gap was written"
    return y[idx]


@pytest.mark.parametrize("r", up.ROWS, ids=lambda r: r["name"])
def test_dropout_rows_row(r):
    R, C = r["batch"] * r["rpb"], r["C"]
    rng = np.random.default_rng([31, R, C])
    x, grad = rng.standard_normal((R, C)).astype(np.float32), rng.standard_normal((R, C)).astype(np.float32)
    big = R * C > 100000
    for rate in (up.DROP_RATES[1:] if big else up.DROP_RATES):
        for step in (((1 << 32) + 1,) if big else up.DROP_STEPS):
            y = run_rows(r, x, rate, step)
            want = x * up.rows_mask(R, C, rate, SEED, step or 0) if rate > 0 else x
            assert _same(y, want), "%s rate %g step %s: %d elements differ" % (r["name"], rate, step, int((_bits(y) != _bits(want)).sum()))
            assert _same(y, run_rows(r, x, rate, step))
    ones, gr = run_rows(r, np.ones((R, C), np.float32), 0.4, 7), run_rows(r, grad, 0.4, 7)
    assert _same(gr, grad * ones), "the gradient call does not regenerate the mask of the forward call"
    assert set(np.unique(ones)) <= {np.float32(0), up.keep_scale(0.4)}


# ---------------------------------------------------------------------------------------------------- bn -> relu -> dropout
def _bnrd_data(r):
    R, C = r["R"], r["C"]
    rng = np.random.default_rng([41, R, C])
    x = rng.standard_normal((R, C)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    shift = (0.3 * rng.standard_normal(C)).astype(np.float32)
    dy = rng.standard_normal((R, C)).astype(np.float32)
    # x scale + shift exactly +0 (0 * s + 0), exactly -0 (-0 * s + -0) and +0 by cancellation (2 * 0.5 - 1)
    shift[0], shift[1], scale[2], shift[2] = 0.0, -0.0, 0.5, -1.0
    x[:3, 0], x[:3, 1], x[:3, 2] = 0.0, -0.0, 2.0
    return x, scale, shift, dy


def run_bnrd(r, data, rate, step, fused=True, in_place=False, off="row"):
    """(y, dx) of the fused pass (or of the two-call compositions) with the row's pointer 4 bytes off"""
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    x, scale, shift, dy = data
    R, C = x.shape
    off = r["off"] if off == "row" else off
    sh = {k: int(off == k) for k in ("x", "scale", "shift", "out", "dy")}
    X, S, Sh = _g(x, sh["x"]), _g(scale, sh["scale"]), _g(shift, sh["shift"])
    Y, DY = _nan((R, C), sh["out"]), _g(dy, sh["dy"])
    DX = DY if in_place else _nan((R, C), sh["out"])
    sd = _step_dev(step)
    if fused:
        for g, k in ((X, "x"), (S, "scale"), (Sh, "shift"), (Y, "out"), (DY, "dy")):
            assert g.view.data_ptr() % 16 == 4 * sh[k]
        nv.check(lib.lidbox_bn_relu_dropout_fwd(X.ptr, R, C, S.ptr, Sh.ptr, rate, SEED, _sp(sd), Y.ptr, st))
        nv.check(lib.lidbox_bn_relu_dropout_bwd(X.ptr, R, C, S.ptr, Sh.ptr, rate, SEED, _sp(sd), DY.ptr, DX.ptr, st))
    else:
        nv.check(lib.lidbox_bn_relu_fwd(X.ptr, R, C, S.ptr, Sh.ptr, Y.ptr, st))
        nv.check(lib.lidbox_dropout_rows(nv.Rows(Y.view.data_ptr(), 0, C, 1, R), C, rate, SEED, _sp(sd), st))
        Gm = _g(dy)
        nv.check(lib.lidbox_dropout_rows(nv.Rows(Gm.view.data_ptr(), 0, C, 1, R), C, rate, SEED, _sp(sd), st))
        nv.check(lib.lidbox_bn_relu_bwd(X.ptr, R, C, S.ptr, Sh.ptr, Gm.ptr, DX.ptr, st))
    torch.cuda.synchronize()
    assert _same(X.numpy(), x) and _same(S.numpy(), scale) and _same(Sh.numpy(), shift), "an input was modified"
    if not in_place:
        assert _same(DY.numpy(), dy), "dy was modified"
    return Y.numpy(), DX.numpy()


@pytest.mark.parametrize("r", up.BNRD, ids=lambda r: r["name"])
def test_bn_relu_dropout_row(r):
    data = _bnrd_data(r)
    x, scale, shift, dy = data
    big = x.size > 1000000
    for rate, step in (((0.4, (1 << 32) + 1),) if big else ((0.4, (1 << 32) + 1), (0.25, None), (0.0, 3))):
        y, dx = run_bnrd(r, data, rate, step)
        y0, dx0 = run_bnrd(r, data, rate, step, fused=False)
        assert _same(y, y0), "%s rate %g: forward differs from bn_relu_fwd + dropout_rows in %d elements" % (r["name"], rate, int((_bits(y) != _bits(y0)).sum()))
        assert _same(dx, dx0), "%s rate %g: backward differs from dropout_rows + bn_relu_bwd" % (r["name"], rate)
        ref, dxref = up.bnrd_ref(x, scale, shift, rate, SEED, step or 0, dy)
        q = up.ulp_distance(y, ref)                                  # one ulp: 2^-23 |ref| (oracle/update_paths_np.py, section 3)
        _note("bn_relu_dropout fwd ulp", q)
        print("bn_relu_dropout %-10s rate %-4g |y - ref| <= %.3f ulp (%.3f spacings of ref)" % (r["name"], rate, q.max(), up.spacing_distance(y, ref).max()))
        assert (q <= 1.0).all(), (r["name"], rate, q.max())
        assert ((y == 0) == (ref == 0)).all(), "the mask or the ReLU differs from the reference"
        assert _same(y, up.bnrd_exact32(x, scale, shift, rate, SEED, step or 0)), "y is not fl(relu(fma(x, scale, shift)) m)"
        assert _same(dx, dxref), "%s rate %g: dx is not (v > 0) ? fl(dy m) : 0" % (r["name"], rate)
        assert not _bits(y[:3, :3]).any() and not _bits(dx[:3, :3]).any(), "x scale + shift = +-0 must give +0 in y and dx"
        if not big:
            y2, dx2 = run_bnrd(r, data, rate, step)
            assert _same(y, y2) and _same(dx, dx2)
            _, dx3 = run_bnrd(r, data, rate, step, in_place=True)
            assert _same(dx, dx3), "in place (dx == dy) differs"
            if r["off"] is not None:                                 # the other kernel on the same data: the same bits
                ya, dxa = run_bnrd(r, data, rate, step, off=None)
                assert _same(y, ya) and _same(dx, dxa), "vector and scalar kernels differ"


# ---------------------------------------------------------------------------------------------------- attention pool
_MLA_REF = {}


def _mla_case(r):
    """inputs and forward reference of a row, computed once"""
    key = r["name"]
    if key not in _MLA_REF:
        z, gd = up.mla_inputs(r["B"], r["T"], r["K"], 7)
        zoff = 4 * ("z" in r["off"])
        plan = up.mla_fwd_plan(r["T"], r["K"], up.mla_vec4(r["K"], zoff))
        _MLA_REF[key] = (z, gd, plan, up.mla_fwd_ref(z, plan))
    return _MLA_REF[key]


def run_mla(z, gd, off=(), ld=0):
    """forward and backward through the C ABI; returns att, colsum, dz"""
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    B, T, K = z.shape
    ldw, col = (ld, ld - K - 2) if ld else (K, 0)
    Z = _g(z, int("z" in off))
    DZ = _nan((B, T, K), int("z" in off or "dz" in off))
    A, S = _nan((B, ldw)), _nan((B, K))
    dh = np.full((B, ldw), NAN32, np.float32)
    dh[:, col:col + K] = gd
    D = _g(dh)
    assert Z.view.data_ptr() % 16 == 4 * int("z" in off)
    nv.check(lib.lidbox_mla_attention_fwd(Z.ptr, B, T, K, _off(A, col), ldw, S.ptr, st))
    torch.cuda.synchronize()
    a_full, s = A.numpy(), S.numpy()
    live = np.zeros((B, ldw), bool)
    live[:, col:col + K] = True
    assert np.isnan(a_full[~live]).all(), "att: another column was written"
    att = a_full[:, col:col + K].copy()
    assert np.isfinite(att).all() and np.isfinite(s).all(), "att or colsum not fully written"
    nv.check(lib.lidbox_mla_attention_bwd(Z.ptr, _off(A, col), ldw, S.ptr, _off(D, col), ldw, B, T, K, DZ.ptr, st))
    torch.cuda.synchronize()
    assert _same(Z.numpy(), z) and _same(A.numpy(), a_full) and _same(S.numpy(), s) and _same(D.numpy(), dh), "an input was modified"
    dz = DZ.numpy()
    assert np.isfinite(dz).all(), "dz not fully written"
    return att, s, dz


def _judge_mla(r, z, gd, plan, ref, att, s, dz, tag=""):
    zoff, dzoff = 4 * ("z" in r["off"]), 4 * ("dz" in r["off"])
    qa = np.abs(att - ref["att"]) / (ref["att_rel"] * ref["att"])
    qs = np.abs(s - ref["colsum"]) / (ref["colsum_rel"] * ref["colsum"])
    bplan = up.mla_bwd_plan(r["B"], r["T"], r["K"], up.mla_vec4(r["K"], zoff, dzoff))
    dref, dbound = up.mla_bwd_ref(z, att, s, gd, bplan)
    qd = np.abs(dz - dref) / dbound
    grp = "<%d,%d>" % (plan["vec"], plan["nj"])
    wa, ws, wd = _note("mla att %s" % grp, qa), _note("mla colsum %s" % grp, qs), _note("mla dz <%d,%d>" % (bplan["vec"], bplan["nj"]), qd)
    print("mla %-12s%s fwd %s G=%d bwd <%d,%d> gy=%d  err/bound att %.3f colsum %.3f dz %.3f  |att - ref| %.2e" % (
        r["name"], tag, grp, plan["G"], bplan["vec"], bplan["nj"], bplan["gy"], wa, ws, wd, np.abs(att - ref["att"]).max()))
    assert (qa <= 1.0).all() and (qs <= 1.0).all(), (r["name"], wa, ws)
    assert (qd <= 1.0).all(), (r["name"], wd, int(np.argmax(qd)))
    assert np.abs(att - ref["att"]).max() <= H_TOL                                  # the outer limit of tests/test_mla_ops_gpu.py
    assert np.linalg.norm(dz - dref) <= G_TOL * max(np.linalg.norm(dref), 1e-30)


@pytest.mark.parametrize("r", up.MLA, ids=lambda r: r["name"])
def test_attention_row(r):
    z, gd, plan, ref = _mla_case(r)
    att, s, dz = run_mla(z, gd, r["off"], r["ld"])
    _judge_mla(r, z, gd, plan, ref, att, s, dz)
    att2, s2, dz2 = run_mla(z, gd, r["off"], r["ld"])
    assert _same(att, att2) and _same(s, s2) and _same(dz, dz2), "a second run gives other bits"
    if r["ld"]:
        dense = run_mla(z, gd, r["off"])
        assert _same(att, dense[0]) and _same(dz, dense[2]), "ld_att / ld_datt change the values"


@pytest.mark.parametrize("K", [128, 512, 1024])
def test_vector_and_scalar_attention_agree_within_the_bounds(K):
    """the same data through <4,nj> and, 4 bytes off, through <1,4 nj>: both inside the bounds (another lane layout sums in
    another order, so bit-equality is recorded, not required)"""
    r = up.by_name("mla", "k%d_zoff" % K)
    z, gd, plan_s, _ = _mla_case(r)
    rv = dict(r, off=())
    plan_v = up.mla_fwd_plan(r["T"], K, True)
    assert (plan_v["vec"], plan_s["vec"]) == (4, 1)
    ref_v = up.mla_fwd_ref(z, plan_v)
    av, sv, dv = run_mla(z, gd, ())
    _judge_mla(rv, z, gd, plan_v, ref_v, av, sv, dv, tag=" (vector)")
    as_, ss, ds = run_mla(z, gd, ("z",))
    print("mla K=%d vector == scalar bits: att %s colsum %s dz %s" % (K, _same(av, as_), _same(sv, ss), _same(dv, ds)))
    assert np.abs(av - as_).max() <= 2 * (ref_v["att_rel"] * ref_v["att"]).max()


@pytest.mark.parametrize("T,K,off", [(37, 100, ()), (9, 511, ()), (9, 1024, ()), (9, 512, ("z",)), (70, 64, ()), (1025, 4, ())])
def test_an_utterance_is_bit_identical_alone_first_and_last_in_a_batch(T, K, off):
    z1, g1 = up.mla_inputs(1, T, K, 9)
    alone = run_mla(z1, g1, off)
    B = 256 if T * K <= 4480 else 5
    z, gd = up.mla_inputs(B, T, K, 10)
    for pos in (0, B - 1):
        z[pos], gd[pos] = z1[0], g1[0]
    att, s, dz = run_mla(z, gd, off)
    for pos in (0, B - 1):
        assert _same(att[pos], alone[0][0]) and _same(s[pos], alone[1][0]) and _same(dz[pos], alone[2][0]), (B, pos)


# ---------------------------------------------------------------------------------------------------- cavg_result
def _cavg_from_update(N, Th):
    """counters built by lidbox_cavg_update on a batch of 40 examples in which language 0 has none"""
    nv = _nv()
    rng = np.random.default_rng([51, N, Th])
    B = 40
    scores = (2 * rng.standard_normal((B, N))).astype(np.float32)
    scores = (scores - np.log(np.exp(scores.astype(np.float64)).sum(1, keepdims=True))).astype(np.float32)
    labels = rng.integers(1, N, B).astype(np.int32)
    thr = np.sort(rng.uniform(-5, 0, Th)).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (scores, labels, thr)]
    cnt = [torch.zeros(s, device="cuda") for s in ((N, Th), (N, Th), (N, N, Th), (N, N, Th))]
    nv.check(nv.lib.lidbox_cavg_update(*[_sp(t) for t in dev[:2]], B, N, _sp(dev[2]), Th, *[_sp(t) for t in cnt], nv.current_stream()))
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in cnt)
    assert not out[0][0].any() and not out[1][0].any() and out[0].sum() + out[1].sum() == B * Th
    return out


def run_cavg(cnt, with_c):
    nv = _nv()
    N, Th = cnt[0].shape
    bufs = [_g(a) for a in cnt]
    Cv, O = (_nan((Th,)) if with_c else None), _nan((4,))
    k = up.CAVG_COST
    nv.check(nv.lib.lidbox_cavg_result(*[b.ptr for b in bufs], N, Th, k["C_miss"], k["C_fa"], k["P_tar"], Cv.ptr if Cv else None, O.ptr,
                                       nv.current_stream()))
    torch.cuda.synchronize()
    assert all(_same(b.numpy(), a) for b, a in zip(bufs, cnt)), "a counter was modified"
    o = O.numpy()
    assert np.isnan(o[1:]).all()
    return (Cv.numpy() if Cv else None), o[0]


@pytest.mark.parametrize("source", ["hand_made", "cavg_update"])
@pytest.mark.parametrize("r", up.CAVG, ids=lambda r: r["name"])
def test_cavg_result_row(r, source):
    N, Th = r["N"], r["Th"]
    cnt = up.cavg_counters(N, Th, 5) if source == "hand_made" else _cavg_from_update(N, Th)
    c, bound, cmin, bmin = up.cavg_ref(*cnt, **up.CAVG_COST)
    got, out = run_cavg(cnt, True)
    assert np.isfinite(got).all() and np.isfinite(out)
    q = np.abs(got - c) / np.maximum(bound, 1e-300)
    q[(bound == 0) & (got == c)] = 0.0
    _note("cavg c_avg lds_pf=%d" % up.cavg_lds_pf(N, Th), q)
    assert (q <= 1.0).all(), (r["name"], q.max(), int(np.argmax(q)))
    assert abs(float(out) - cmin) <= bmin and _same(out, got.min()), "out[0] is not the smallest c_avg_out"
    none, out_null = run_cavg(cnt, False)
    assert none is None and _same(out, out_null), "c_avg_out NULL changes out[0]"
    got2, out2 = run_cavg(cnt, True)
    assert _same(got, got2) and _same(out, out2)


# ---------------------------------------------------------------------------------------------------- mean, scale, fill
@pytest.mark.parametrize("r", up.EW, ids=lambda r: r["name"])
def test_mean_scale_fill_row(r):
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    n = r["n"]
    x = (1.0 + np.random.default_rng([61, n]).standard_normal(n)).astype(np.float32)
    for _ in range(2):
        X, O = _g(x), _nan((4,))
        nv.check(lib.lidbox_mean(X.ptr, n, O.ptr, st))
        torch.cuda.synchronize()
        o = O.numpy()
        ref, bound = up.mean_ref(x)
        assert _same(X.numpy(), x) and np.isnan(o[1:]).all()
        assert _note("mean", abs(float(o[0]) - ref) / bound) <= 1.0
        alpha = np.float32(0.3)
        nv.check(lib.lidbox_scale(X.ptr, n, float(alpha), st))
        torch.cuda.synchronize()
        assert _same(X.numpy(), x * alpha), "scale is not fl(x alpha)"
        F = _nan((n,))
        nv.check(lib.lidbox_fill(F.ptr, n, -2.5, st))
        torch.cuda.synchronize()
        assert _same(F.numpy(), np.full(n, -2.5, np.float32))


# ---------------------------------------------------------------------------------------------------- empty calls, refusals
def test_empty_calls_write_nothing_but_the_step():
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    bufs = [_nan((64,)) for _ in range(5)]
    a, b, c, d, e = (g.ptr for g in bufs)
    for kind, call in (("adam", lambda s: lib.lidbox_adam_step(a, b, c, d, 0, 1e-3, 0.9, 0.999, 1e-7, 1.0, s.ptr, st)),
                       ("sgd", lambda s: lib.lidbox_sgd_step(a, b, c, 0, 0.03, 0.9, 0, 1.0, s.ptr, st)),
                       ("rmsprop", lambda s: lib.lidbox_rmsprop_step(a, b, c, d, e, 0, 1e-3, 0.9, 0.9, 1e-7, 1, 1.0, s.ptr, st))):
        state, _ = _state(41, 0.0)
        assert call(state) == 0
        torch.cuda.synchronize()
        step, lr_t, _ = _read_state(state)
        assert step == 42 and np.isfinite(lr_t), kind                # the header: the step advances even when n = 0
    state, h = _state(41, 0.0)
    assert lib.lidbox_adam_apply(a, b, c, d, 0, 0.9, 0.999, 1e-7, 1.0, state.ptr, st) == 0
    assert lib.lidbox_scale(a, 0, 0.5, st) == 0 and lib.lidbox_fill(a, 0, 1.0, st) == 0
    assert lib.lidbox_spatial_dropout(a, 0, 3, 5, 15, 0.25, SEED, None, b, st) == 0
    assert lib.lidbox_spatial_dropout(a, 2, 0, 5, 0, 0.25, SEED, None, b, st) == 0
    assert lib.lidbox_input_noise_dropout(a, 0, 3, 5, 15, 0.01, 0.25, SEED, None, st) == 0
    assert lib.lidbox_input_noise_dropout(a, 2, 3, 5, 15, 0.0, 0.0, SEED, None, st) == 0
    assert lib.lidbox_dropout_rows(nv.Rows(bufs[0].view.data_ptr(), 0, 5, 1, 0), 5, 0.25, SEED, None, st) == 0
    assert lib.lidbox_dropout_rows(nv.Rows(bufs[0].view.data_ptr(), 0, 5, 1, 3), 5, 0.0, SEED, None, st) == 0
    assert lib.lidbox_bn_relu_dropout_fwd(a, 0, 4, b, c, 0.25, SEED, None, d, st) == 0
    assert lib.lidbox_bn_relu_dropout_bwd(a, 0, 4, b, c, 0.25, SEED, None, d, e, st) == 0
    assert lib.lidbox_mla_attention_fwd(a, 0, 3, 4, b, 4, c, st) == 0
    assert lib.lidbox_mla_attention_bwd(a, b, 4, c, d, 4, 0, 3, 4, e, st) == 0
    torch.cuda.synchronize()
    assert _same(state.numpy(), h.view(np.float32)), "adam_apply with n = 0 touched the state"
    for g in bufs:
        assert np.isnan(g.numpy()).all()


def test_refusals_name_their_function_and_write_nothing():
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    bufs = [_nan((64,)) for _ in range(5)]
    a, b, c, d, e = (g.ptr for g in bufs)
    odd = _off(bufs[0], 1)                                           # 4 bytes off a 16-byte boundary
    state, h = _state(7, 0.0)
    s = state.ptr
    cases = [("lidbox_adam_step", lambda: lib.lidbox_adam_step(odd, b, c, d, 8, 1e-3, 0.9, 0.999, 1e-7, 1.0, s, st)),
             ("lidbox_adam_step", lambda: lib.lidbox_adam_step(a, b, c, d, -1, 1e-3, 0.9, 0.999, 1e-7, 1.0, s, st)),
             ("lidbox_adam_step", lambda: lib.lidbox_adam_step(a, b, None, d, 8, 1e-3, 0.9, 0.999, 1e-7, 1.0, s, st)),
             ("lidbox_adam_apply", lambda: lib.lidbox_adam_apply(a, b, c, _off(bufs[3], 1), 8, 0.9, 0.999, 1e-7, 1.0, s, st)),
             ("lidbox_adam_prepare_job", lambda: lib.lidbox_adam_prepare_job(_off(state, 1), 1e-3, 0.9, 0.999, (nv.ReduceJob * 1)())),
             ("lidbox_sgd_step", lambda: lib.lidbox_sgd_step(a, b, None, 8, 0.03, 0.9, 0, 1.0, s, st)),
             ("lidbox_sgd_step", lambda: lib.lidbox_sgd_step(a, b, c, 8, 0.03, -0.1, 0, 1.0, s, st)),
             ("lidbox_rmsprop_step", lambda: lib.lidbox_rmsprop_step(a, b, c, None, e, 8, 1e-3, 0.9, 0.0, 1e-7, 1, 1.0, s, st)),
             ("lidbox_rmsprop_step", lambda: lib.lidbox_rmsprop_step(a, b, c, d, None, 8, 1e-3, 0.9, 0.9, 1e-7, 0, 1.0, s, st)),
             ("lidbox_cavg_result", lambda: lib.lidbox_cavg_result(a, b, c, d, 1, 4, 1.0, 1.0, 0.5, None, e, st)),
             ("lidbox_cavg_result", lambda: lib.lidbox_cavg_result(a, b, c, d, 2, 0, 1.0, 1.0, 0.5, None, e, st)),
             ("lidbox_mean", lambda: lib.lidbox_mean(a, 0, b, st)),
             ("lidbox_scale", lambda: lib.lidbox_scale(None, 4, 0.5, st)),
             ("lidbox_fill", lambda: lib.lidbox_fill(a, -1, 0.5, st)),
             ("lidbox_mla_attention_fwd", lambda: lib.lidbox_mla_attention_fwd(a, 1, 1, 1025, b, 1025, c, st)),
             ("lidbox_mla_attention_fwd", lambda: lib.lidbox_mla_attention_fwd(a, 2, 3, 4, b, 3, c, st)),
             ("lidbox_mla_attention_bwd", lambda: lib.lidbox_mla_attention_bwd(a, b, 4, c, d, 3, 2, 3, 4, e, st)),
             ("lidbox_bn_relu_dropout_fwd", lambda: lib.lidbox_bn_relu_dropout_fwd(a, 2, 4, b, c, 1.0, SEED, None, d, st)),
             ("lidbox_bn_relu_dropout_fwd", lambda: lib.lidbox_bn_relu_dropout_fwd(a, 2, 0, b, c, 0.25, SEED, None, d, st)),
             ("lidbox_bn_relu_dropout_bwd", lambda: lib.lidbox_bn_relu_dropout_bwd(a, 2, 4, b, c, 0.25, SEED, None, None, e, st))]
    for fn, call in cases:
        _refused(call(), fn)
    torch.cuda.synchronize()
    assert _same(state.numpy(), h.view(np.float32)), "a refused call advanced the step"
    for g in bufs:
        assert np.isnan(g.numpy()).all()


def test_zz_report():
    """the largest err / bound of every group of this run (docs/LAB_NOTEBOOK.md section 28 records one such run)"""
    for g in sorted(WORST):
        print("WORST %-32s %.3e" % (g, WORST[g]))
    assert all(v <= 1.0 for v in WORST.values())
