"""
The ragged train step of multilevel_attention on the device: lidbox_mla_attention_ragged_bwd through the C ABI, the model's
forward_ragged_train / backward_ragged, Trainer.train_step_ragged / loss_and_grads_ragged and KerasWrapper.fit / evaluate on
ragged batches.  Cases and weights are tests/ragged_mla_cases.py's, the float64 restatements tests/ragged_mla_train_cases.py's.

Kernel level.  z and dz are tests/guarded.py payloads, att / datt column slices (offset K + 1) of guarded [B, 2 K + 3] buffers,
att and colsum the ragged forward's.  How results are judged:
    1. bit for bit against lidbox_mla_attention_bwd on every utterance alone (B = 1, T = T_b, the utterance's slices), for K
       values that reach all eight (VEC, NJ) pairs, two of them through bases 4 bytes off a 16-byte boundary, lengths that
       bracket one pass of the forward's row loop, shuffled; and on 256 utterances of 1 .. 298 frames at K = 100, where the cap
       on gridDim.y forces further trips of the row loop;
    2. every element against oracle/update_paths_np.mla_bwd_ref (float64) within its bound for mla_plan(K, vec4);
    3. the same bits in a permuted batch, beside a NaN utterance and in a second run; guard words, inputs and the other columns
       untouched;
    4. B = 0 and every refusal with nothing written.

Model level.  At equal lengths (B = 4, T = 33) the ragged pass is the dense pass bit for bit: loss, gradients, att, and one
whole step on a twin model.  At MODEL_LENGTHS (1 .. 298): H_TOL = 5e-5 on loss and logits, G_TOL = 1e-4 relative L2 on every
parameter gradient against float64 (the bounds of tests/test_multilevel_attention_gpu.py: the same kernels over no more rows),
masks rebuilt from oracle/update_paths_np.hash_uniform with r the row in the concatenation.  Measured maxima (MI355X): see
docs/LAB_NOTEBOOK.md section 33.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import ragged_mla_cases as rc
import ragged_mla_train_cases as tc
from guarded import Guarded
from oracle import update_paths_np as up

pytestmark = pytest.mark.gpu

H_TOL, G_TOL = tc.H_TOL, tc.G_TOL
NAN32 = np.float32(np.nan)


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


def _off(g, words):
    return ctypes.c_void_p(g.view.data_ptr() + 4 * words)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- kernel level
class KernelRun:
    """one batch on the device: z, the ragged forward's att / colsum, datt, and dz of the ragged backward (`dz`) and of the dense
    backward on every utterance alone (`dz_each`)"""

    def __init__(self, z, ro, shift, datt_seed=41, each=True):
        nv = _nv()
        lib, st = nv.lib, nv.current_stream()
        self.z, self.ro, self.shift = z, ro, shift
        B, K = len(ro) - 1, z.shape[1]
        R = int(ro[-1])
        self.B, self.K, self.ld, self.col = B, K, 2 * K + 3, K + 1
        ld, col = self.ld, self.col
        self.Z = Guarded(z.shape, init=_dev(np.array(z, np.float32)), shift=shift)
        assert self.Z.view.data_ptr() % 16 == 4 * shift
        self.ro_dev = _dev(np.array(ro, np.int64))
        self.A, self.S, self.D = Guarded((B, ld)), Guarded((B, K)), Guarded((B, ld))
        self.datt = np.random.default_rng([datt_seed, K]).standard_normal((B, K)).astype(np.float32)
        self.D.view[:, col:col + K] = _dev(self.datt)
        nv.check(lib.lidbox_mla_attention_ragged_fwd(self.Z.ptr, nv.ptr(self.ro_dev), B, K, _off(self.A, col), ld, self.S.ptr, st))
        torch.cuda.synchronize()
        before = [g.numpy().copy() for g in (self.Z, self.A, self.S, self.D)]
        self.att, self.colsum = before[1][:, col:col + K].copy(), before[2].copy()
        max_T = int(np.diff(ro).max())
        self.DZ = Guarded((R, K), shift=shift)
        nv.check(lib.lidbox_mla_attention_ragged_bwd(self.Z.ptr, nv.ptr(self.ro_dev), B, max_T, K, _off(self.A, col), ld, self.S.ptr,
                                                     _off(self.D, col), ld, self.DZ.ptr, st))
        torch.cuda.synchronize()
        self.dz = self.DZ.numpy()                                   # .numpy() checks the guard words
        for g, was in zip((self.Z, self.A, self.S, self.D), before):
            assert _same(g.numpy(), was), "an input of the backward pass was modified"
        self.dz_each = None
        if each:
            E = Guarded((R, K), shift=shift)
            for b in range(B):
                r0, T = int(ro[b]), int(ro[b + 1] - ro[b])
                nv.check(lib.lidbox_mla_attention_bwd(_off(self.Z, r0 * K), _off(self.A, b * ld + col), ld, _off(self.S, b * K),
                                                      _off(self.D, b * ld + col), ld, 1, T, K, _off(E, r0 * K), st))
            torch.cuda.synchronize()
            self.dz_each = E.numpy()


_KERNEL = {}


def _kernel_case(K, shift):
    if (K, shift) not in _KERNEL:
        z, ro = rc.kernel_inputs(K, shift)
        run = KernelRun(z, ro, shift)
        for a in (z, ro, run.dz, run.dz_each, run.att, run.colsum, run.datt):
            a.setflags(write=False)
        _KERNEL[(K, shift)] = run
    return _KERNEL[(K, shift)]


def _big_case():
    """256 utterances of 1 .. 298 frames at K = 100: gridDim.y is capped at cdiv(2048, 256) = 8 workgroups of 16 rows"""
    if "big" not in _KERNEL:
        rng = np.random.default_rng(33)
        lengths = rng.integers(1, 299, 256)
        lengths[[5, 77]] = (298, 1)
        ro = tc.offsets(lengths)
        z, _ = up.mla_inputs(1, int(ro[-1]), 100, 34)
        _KERNEL["big"] = KernelRun(z.reshape(-1, 100), ro, 0)
    return _KERNEL["big"]


def _assert_bits_and_bound(run, tag):
    K, ro, shift = run.K, run.ro, run.shift
    vec4 = K % 4 == 0 and not shift
    assert up.mla_vec4(K, run.Z.view.data_ptr(), run.DZ.view.data_ptr()) == vec4
    plan = up.mla_plan(K, vec4)
    assert np.isfinite(run.dz).all(), "dz not fully written"
    z64 = run.z.astype(np.float64)
    e = np.exp(z64 - z64.max(-1, keepdims=True))
    prob = e / e.sum(-1, keepdims=True)
    assert not up.near_clip_bound(prob).any() and (prob > up.HI).any() and ((prob < up.LO).any() or K == 1)
    worst = 0.0
    for b in range(run.B):
        r0, r1 = int(ro[b]), int(ro[b + 1])
        assert _same(run.dz[r0:r1], run.dz_each[r0:r1]), "dz of utterance %d (T = %d) differs from the dense call on it alone" % (b, r1 - r0)
        ref, bound = up.mla_bwd_ref(run.z[None, r0:r1], run.att[b:b + 1], run.colsum[b:b + 1], run.datt[b:b + 1], plan)
        q = np.abs(run.dz[r0:r1] - ref[0]) / bound[0]
        worst = max(worst, float(q.max()))
        assert (q <= 1.0).all(), (K, b, r1 - r0, float(q.max()))
    print("ragged mla bwd %s K=%d%s <%d,%d>: err/bound dz %.3f" % (tag, K, " off" if shift else "", plan["vec"], plan["nj"], worst))


@pytest.mark.parametrize("K,shift", rc.KERNEL_KS, ids=["k%d%s" % (K, "_off" if s else "") for K, s in rc.KERNEL_KS])
def test_every_utterance_gets_the_dense_backward_bits_within_the_float64_bound(K, shift):
    run = _kernel_case(K, shift)
    assert list(np.diff(run.ro)) == rc.kernel_lengths(K, shift) and list(np.diff(run.ro)) != sorted(np.diff(run.ro))
    _assert_bits_and_bound(run, "lengths around a pass")


def test_the_capped_grid_takes_further_trips_of_the_row_loop():
    run = _big_case()
    p = up.mla_bwd_plan(run.B, int(np.diff(run.ro).max()), 100, True)
    assert (p["gy"], p["trips"]) == (8, 3) and set(np.diff(run.ro)) >= {1, 298}
    _assert_bits_and_bound(run, "256 utterances")


@pytest.mark.parametrize("K,shift", [(100, 0), (127, 0), (5, 0), (128, 1)], ids=["k100", "k127", "k5", "k128_off"])
def test_an_utterance_does_not_depend_on_its_neighbours_place_or_run(K, shift):
    run = _kernel_case(K, shift)
    z, ro, B = run.z, run.ro, run.B
    rows = lambda r, b: r.dz[int(r.ro[b]):int(r.ro[b + 1])]
    # run to run
    again = KernelRun(z, ro, shift, each=False)
    assert _same(again.dz, run.dz)
    # another order: other neighbours, another place, another first row; datt follows the place, so give every utterance its own
    perm = np.random.default_rng(3).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    zp = np.concatenate([z[ro[b]:ro[b + 1]] for b in perm])
    rop = tc.offsets([ro[b + 1] - ro[b] for b in perm])
    permuted = KernelRun(zp, rop, shift, each=False)
    nv = _nv()
    permuted.D.view[:, permuted.col:permuted.col + K] = _dev(run.datt[perm])
    permuted.DZ.view.fill_(float("nan"))
    nv.check(nv.lib.lidbox_mla_attention_ragged_bwd(permuted.Z.ptr, nv.ptr(permuted.ro_dev), B, int(np.diff(rop).max()), K,
                                                    _off(permuted.A, permuted.col), permuted.ld, permuted.S.ptr,
                                                    _off(permuted.D, permuted.col), permuted.ld, permuted.DZ.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    permuted.dz = permuted.DZ.numpy()
    for i, b in enumerate(perm):
        assert _same(rows(permuted, i), rows(run, b)), (i, b)
    # a NaN neighbour
    victim = int(np.argsort(np.diff(ro))[B // 2])
    zn = z.copy()
    zn[ro[victim]:ro[victim + 1]] = NAN32
    nan = KernelRun(zn, ro, shift, each=False)
    assert np.isnan(rows(nan, victim)).all()
    for b in range(B):
        if b != victim:
            assert _same(rows(nan, b), rows(run, b)), b


def test_empty_batch_and_refusals_write_nothing():
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    buf = torch.full((64,), 3.0, device="cuda")
    ro = torch.tensor([0, 2, 5], dtype=torch.int64, device="cuda")
    p, o = nv.ptr(buf), nv.ptr(ro)
    f = lib.lidbox_mla_attention_ragged_bwd
    assert f(p, o, 0, 3, 4, p, 4, p, p, 4, p, st) == 0 and f(p, o, 0, 0, 4, p, 4, p, p, 4, p, st) == 0
    good = [p, o, 2, 3, 4, p, 4, p, p, 4, p]
    for i, v in ((0, None), (1, None), (5, None), (7, None), (8, None), (10, None), (2, -1), (2, 2 ** 31), (3, 0), (3, -1), (4, 0), (4, -2),
                 (4, 1025), (6, 3), (9, 3)):
        args = list(good)
        args[i] = v
        if (i, v) == (4, 1025):
            args[6] = args[9] = 1025
        assert f(*args, st) == -1, (i, v)
        assert "lidbox_mla_attention_ragged_bwd" in nv.last_error()
    with pytest.raises(ValueError):
        nv.check(f(p, o, 2, 3, 4, p, 3, p, p, 4, p, st))
    torch.cuda.synchronize()
    assert (buf == 3.0).all() and ro.tolist() == [0, 2, 5]


# ---------------------------------------------------------------------------------------------------- model level
def _model(case, rate, T=None, **kw):
    from lidbox_amd.models import multilevel_attention
    c = rc.MODEL_CASES[case]
    m = multilevel_attention.create((T or max(rc.MODEL_LENGTHS), c["D"]), c["K"], L=c["L"], H=c["H"], seed=1, dropout_rate=rate, **kw)
    m.set_weights(rc.model_weights(**c))
    return m


def _trainer(m, **kw):
    from lidbox_amd.train import Trainer
    return Trainer(m, use_graph=False, **kw)


def _ragged_batch(case):
    """(X on the device [823, D], offsets, labels on the device, the utterances, the labels)"""
    c = rc.MODEL_CASES[case]
    xs = rc.model_inputs(c["D"])
    y = tc.labels_for(len(xs), c["K"])
    return _dev(np.concatenate(xs)), tc.offsets([len(x) for x in xs]), _dev(y), xs, y


def _grads(m):
    return {n: m.param(n, grad=True).cpu().numpy().copy() for n in m.layout}


def _masks(m, R, step):
    if m.dropout_rate == 0:
        return None
    return [up.rows_mask(R, m.units, m.dropout_rate, m.level_dropout_seed(l), step) for l in range(m.levels)]


@pytest.mark.parametrize("rate", [0.4, 0.0])
@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_at_equal_lengths_the_ragged_pass_is_the_dense_pass_bit_for_bit(case, rate):
    c = rc.MODEL_CASES[case]
    B, T = tc.EQ_B, tc.EQ_T
    x, y = _dev(tc.equal_inputs(c["D"])), _dev(tc.labels_for(B, c["K"]))
    ro = tc.offsets([T] * B)
    m = _model(case, rate, T)
    tr = _trainer(m)
    state0 = m.state.clone()
    loss_d, g = tr.loss_and_grads(x, y)
    loss_d, g_d, att_d = loss_d.clone(), g.clone(), m.workspace(B, T).att.clone()
    loss_r, g = tr.loss_and_grads_ragged(x.reshape(B * T, c["D"]), ro, y)
    assert np.abs(g_d.cpu().numpy()).max() > 0 and math.isfinite(float(loss_r))
    assert _same(loss_r.cpu().numpy(), loss_d.cpu().numpy()) and _same(g.cpu().numpy(), g_d.cpu().numpy())
    assert _same(m._rtws.att[:B].cpu().numpy(), att_d.cpu().numpy())
    assert torch.equal(m.state, state0) and tr.step_count == 0
    # one whole step on twins
    twins = []
    for ragged in (False, True):
        m2 = _model(case, rate, T)
        tr2 = _trainer(m2)
        loss = tr2.train_step_ragged(x.reshape(B * T, c["D"]), ro, y) if ragged else tr2.train_step(x, y)
        twins.append((loss.cpu().numpy().copy(), m2.flat.cpu().numpy(), m2.state.cpu().numpy(), tr2.step_count))
    (l1, f1, s1, n1), (l2, f2, s2, n2) = twins
    assert _same(l1, l2) and _same(f1, f2) and _same(s1, s2) and n1 == n2 == 1
    assert not _same(f1, m.flat.cpu().numpy()) and not _same(s1, state0.cpu().numpy())


_REF64 = {}


def _float64(case, rate, m):
    """the float64 restatement on MODEL_LENGTHS with the masks of step 0: (leaves, logits, loss, stats, pre_bn, masks)"""
    if (case, rate) not in _REF64:
        c = rc.MODEL_CASES[case]
        _, ro, _, xs, y = _ragged_batch(case)
        masks = _masks(m, int(ro[-1]), 0)
        p = tc.params64(tc.trainable(rc.model_weights(**c)))
        logits, stats, pre_bn, probs = tc.ragged64(p, c["L"], np.concatenate(xs), ro, masks)
        assert tc.away_from_the_clip_bounds(probs)
        loss = tc.mean_nll(logits, y)
        loss.backward()
        _REF64[(case, rate)] = (p, logits.detach().numpy(), float(loss.detach()), stats, pre_bn, masks)
    return _REF64[(case, rate)]


@pytest.mark.parametrize("rate", [0.0, 0.4])
@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_unequal_lengths_match_float64(case, rate):
    c = rc.MODEL_CASES[case]
    X, ro, yd, xs, y = _ragged_batch(case)
    m = _model(case, rate)
    tr = _trainer(m)
    p, logits64, loss64, stats, pre_bn, masks = _float64(case, rate, m)
    w0 = m.get_weights()
    loss, _ = tr.loss_and_grads_ragged(X, ro, yd)
    ws, R, B = m._rtws, int(ro[-1]), len(xs)
    e_loss = abs(float(loss) - loss64)
    e_logits = float(np.abs(ws.h[-1][:B].cpu().numpy() - logits64).max())
    errs = tc.gradient_errors(_grads(m), p, pre_bn)
    worst = max(errs, key=errs.get)
    print("ragged train %s dropout %.1f: |loss - ref| = %.3e, |logits - ref| = %.3e, max rel L2 gradient error = %.3e (%s)"
          % (case, rate, e_loss, e_logits, errs[worst], worst))
    if masks is not None:
        for l, mask in enumerate(masks):                              # the model applied exactly these masks, row = concatenated row
            yl = ws.y[l][:R].cpu().numpy()
            assert (yl[mask == 0] == 0).all() and (yl[mask != 0] > 0).mean() > 0.2 and 0.4 < (mask != 0).mean() < 0.8
    assert e_loss <= H_TOL and e_logits <= H_TOL
    for n, e in errs.items():
        assert e <= G_TOL, (n, e)
    assert all(np.array_equal(w0[n], v) for n, v in m.get_weights().items())          # a probe moves nothing
    # one step: the moving statistics follow 0.99 old + 0.01 batch statistic over the real frames
    tr.train_step_ragged(X, ro, yd)
    w1 = m.get_weights()
    assert sorted(stats) == ["dense_block%d_bn" % l for l in range(1, c["L"] + 1)]
    for name, (mean, var) in stats.items():
        assert np.allclose(w1[name + ".moving_mean"], 0.99 * w0[name + ".moving_mean"] + 0.01 * mean, rtol=1e-5, atol=1e-6), name
        assert np.allclose(w1[name + ".moving_variance"], 0.99 * w0[name + ".moving_variance"] + 0.01 * var, rtol=1e-5, atol=1e-6), name


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_the_padded_dense_step_misses_the_gradient_bound(case):
    """the dense step on the batch zero-padded to 298 frames, against the float64 gradients of the real frames; the
    `dense_block{l}_fc.b`, whose exact gradient is zero on both routes, are left out (tests/test_ragged_mla_train_cpu.py)"""
    X, ro, yd, xs, y = _ragged_batch(case)
    m = _model(case, 0.0)
    tr = _trainer(m)
    p, _, loss64, _, pre_bn, _ = _float64(case, 0.0, m)
    tr.loss_and_grads_ragged(X, ro, yd)
    assert max(tc.gradient_errors(_grads(m), p, pre_bn).values()) <= G_TOL          # the ragged step on the same model meets it
    loss, _ = tr.loss_and_grads(_dev(tc.padded_batch(xs)), yd)
    errs = {n: e for n, e in tc.gradient_errors(_grads(m), p, pre_bn).items() if n not in pre_bn}
    print("padded dense step %s: |loss - ref| = %.3e, rel L2 gradient error %.3e .. %.3e" % (case, abs(float(loss) - loss64),
                                                                                             min(errs.values()), max(errs.values())))
    for n, e in errs.items():
        assert e > G_TOL, (n, e)


# ---------------------------------------------------------------------------------------------------- Trainer
def _keras_adam(p, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """one tf.keras Adam step from zero moments (t = 1) on float64 leaves with .grad"""
    lr_t = lr * math.sqrt(1 - b2) / (1 - b1)
    out = {}
    for n, t in p.items():
        g = t.grad.numpy()
        out[n] = t.detach().numpy() - lr_t * (1 - b1) * g / (np.sqrt((1 - b2) * g * g) + eps)
    return out


def test_one_adam_step_matches_float64():
    """the rule of tests/test_multilevel_attention_gpu.py::_check_step: an Adam step is ~lr sign(g), so compare where the gradient
    is not vanishingly small; the `_fc.b` divide rounding noise by its own size in either precision"""
    case, rate = "k5", 0.4
    X, ro, yd, xs, y = _ragged_batch(case)
    m = _model(case, rate)
    tr = _trainer(m)
    p, _, loss64, _, pre_bn, _ = _float64(case, rate, m)
    w0 = m.get_weights()
    loss = float(tr.train_step_ragged(X, ro, yd))
    w1 = m.get_weights()
    assert abs(loss - loss64) <= 1e-4 * max(1.0, abs(loss64)) and tr.step_count == 1
    want = _keras_adam(p)
    for n in m.layout:
        if n in pre_bn:
            continue
        g = p[n].grad.numpy()
        big = np.abs(g) > 1e-3 * max(1e-30, np.abs(g).max())
        assert np.abs((w1[n] - w0[n]) - (want[n] - w0[n]))[big].max() <= 2e-5, n


@pytest.mark.parametrize("opt", [dict(cls="SGD", lr=0.05, momentum=0.9), dict(cls="RMSprop", lr=1e-3)], ids=["sgd", "rmsprop"])
def test_one_step_of_the_other_optimizers(opt):
    X, ro, yd, xs, y = _ragged_batch("k5")
    m = _model("k5", 0.4)
    tr = _trainer(m, optimizer=opt)
    flat0 = m.flat.clone()
    loss = float(tr.train_step_ragged(X, ro, yd))
    assert math.isfinite(loss) and tr.step_count == 1
    assert torch.isfinite(m.flat).all() and (m.flat != flat0).float().mean() > 0.5


def test_counter_statistics_and_masks_advance_once_per_step():
    X, ro, yd, xs, y = _ragged_batch("k5")
    m = _model("k5", 0.4)
    tr = _trainer(m)
    R = int(ro[-1])
    state = [m.state.clone()]
    tr.loss_and_grads_ragged(X, ro, yd)
    assert tr.step_count == 0 and torch.equal(m.state, state[0])
    seen = []
    for step in range(2):
        tr.train_step_ragged(X, ro, yd)
        assert tr.step_count == step + 1
        state.append(m.state.clone())
        assert not torch.equal(state[-1], state[-2])
        masks = _masks(m, R, step)                               # the forward pass read the counter before its update
        for l in range(m.levels):
            yl = m._rtws.y[l][:R].cpu().numpy()
            assert (yl[masks[l] == 0] == 0).all() and (yl[masks[l] != 0] > 0).mean() > 0.2, (step, l)
        seen.append(masks)
        tr.loss_and_grads_ragged(X, ro, yd)
        assert tr.step_count == step + 1 and torch.equal(m.state, state[-1])
    for a, b in ((seen[0][0], seen[1][0]), (seen[0][1], seen[1][1]), (seen[0][0], seen[0][1])):
        differ = float(((a != 0) != (b != 0)).mean())
        assert 0.4 < differ < 0.56, differ                       # independent masks of rate 0.4 differ at 0.48 of the elements


def test_small_large_small_on_one_workspace():
    """the second small step runs on the front of grown buffers: the bits of a model whose buffers are poisoned before every
    step equal those of a fresh model fed the same sequence, and the workspace grows once"""
    X, ro, yd, xs, y = _ragged_batch("k5")
    small = (X[:ro[4]], ro[:5], yd[:4])
    seq = [small, (X, ro, yd), small]
    out = []
    for poison in (False, True):
        m = _model("k5", 0.4)
        tr = _trainer(m)
        caps, losses = [], []
        for Xi, roi, yi in seq:
            ws = getattr(m, "_rtws", None)
            if poison and ws is not None:
                for t in ws.a + ws.y + ws.z + ws.colsum + ws.h + ws.dh + [ws.att, ws.datt, ws.dz, ws.dy, ws.da, ws.logp]:
                    t.fill_(float("nan"))
            losses.append(tr.train_step_ragged(Xi, roi, yi).cpu().numpy().copy())
            caps.append((m._rtws.cap_rows, m._rtws.cap_B, id(m._rtws)))
        assert caps[0][:2] == (int(ro[4]), 4) and caps[1][:2] == (int(ro[-1]), len(xs)) and caps[2] == caps[1] and caps[0][2] == caps[1][2]
        assert m._rtws.grown == 2                                 # the first allocation and one growth
        out.append((losses, m.flat.cpu().numpy(), m.state.cpu().numpy()))
    (la, fa, sa), (lb, fb, sb) = out
    assert all(_same(a, b) for a, b in zip(la, lb)) and _same(fa, fb) and _same(sa, sb)
    assert np.isfinite(fa).all() and np.isfinite(la).all()


def test_ragged_training_leaves_the_dense_step_and_the_ragged_inference_untouched():
    c = rc.MODEL_CASES["k5"]
    X, ro, yd, xs, y = _ragged_batch("k5")
    m = _model("k5", 0.4, tc.EQ_T)
    tr = _trainer(m)
    x, ye = _dev(tc.equal_inputs(c["D"])), _dev(tc.labels_for(tc.EQ_B, c["K"]))

    def probe():
        loss, g = tr.loss_and_grads(x, ye)
        return loss.cpu().numpy().copy(), g.cpu().numpy().copy(), m.predict_ragged(X, ro).cpu().numpy()

    before = probe()
    saved = [t.clone() for t in (m.flat, m.state, tr.m, tr.v, tr.adam_state)]
    tr.loss_and_grads_ragged(X, ro, yd)
    tr.train_step_ragged(X, ro, yd)
    assert not torch.equal(m.flat, saved[0])
    for t, s in zip((m.flat, m.state, tr.m, tr.v, tr.adam_state), saved):
        t.copy_(s)
    after = probe()
    assert all(_same(a, b) for a, b in zip(before, after)) and np.abs(before[1]).max() > 0
    # and a dense step after ragged steps is the dense step of a model that never saw one
    m2 = _model("k5", 0.4, tc.EQ_T)
    l1, l2 = tr.train_step(x, ye), _trainer(m2).train_step(x, ye)
    assert _same(l1.cpu().numpy(), l2.cpu().numpy()) and _same(m.flat.cpu().numpy(), m2.flat.cpu().numpy())


def test_trainer_refusals():
    from lidbox_amd.models import xvector
    X, ro, yd, xs, y = _ragged_batch("k5")
    m = _model("k5", 0.4)
    tr = _trainer(m)
    for call in (tr.train_step_ragged, tr.loss_and_grads_ragged):
        with pytest.raises(ValueError, match="length 0"):
            call(X, [0, 3, 3, len(X)], yd[:3])
        with pytest.raises(ValueError, match="row_offsets"):
            call(X, ro[:-1], yd)
        with pytest.raises(ValueError, match=r"\[total_T, 8\]"):
            call(torch.zeros((5, 9), device="cuda"), [0, 5], yd[:1])
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros((5, 16), device="cuda")[:, :8], [0, 5], yd[:1])
        with pytest.raises(ValueError, match="labels"):
            call(X, ro, yd[:-1])
        with pytest.raises(ValueError, match="at least one utterance"):
            call(X[:0], [0], yd[:0])
        with pytest.raises(Exception):
            call(X.cpu(), ro, yd)
        with pytest.raises(Exception):
            call(X, ro, yd.long())
        tr.feature = dict(plan=None, kind=0)
        with pytest.raises(ValueError, match="feature= front-end"):
            call(X, ro, yd)
        tr.feature = None
        tr.sync.active = True
        with pytest.raises(ValueError, match="gradient exchange"):
            call(X, ro, yd)
        tr.sync.active = False
    assert getattr(m, "_rtws", None) is None and tr.step_count == 0
    xv = xvector.create((60, 8), 5, seed=0)
    with pytest.raises(ValueError, match="no ragged training pass"):
        _trainer(xv).train_step_ragged(X, ro, yd)


# ---------------------------------------------------------------------------------------------------- KerasWrapper
def _separable_batches(n_batches, B, D, K, seed=11):
    """ragged batches of a separable problem whose class does not depend on the length (the construction of
    tests/test_multilevel_attention_gpu.py::test_loss_falls_on_separable_problem, lengths 10 .. 30 drawn apart from the class)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, D)).astype(np.float32) * 2
    data = []
    for _ in range(n_batches):
        y = rng.integers(0, K, B).astype(np.int32)
        lengths = rng.integers(10, 31, B)
        X = np.concatenate([centres[c] + 0.5 * rng.standard_normal((T, D)) for c, T in zip(y, lengths)]).astype(np.float32)
        data.append(((torch.from_numpy(X), tc.offsets(lengths)), torch.from_numpy(y)))
    return data


def test_keras_wrapper_fits_and_evaluates_ragged_batches():
    from lidbox_amd.models import keras_utils as ku
    from lidbox_amd.models import multilevel_attention
    D, K = 8, 4
    data = _separable_batches(3, 32, D, K)
    m = multilevel_attention.create((30, D), K, H=512, seed=3)
    w = ku.KerasWrapper(m, "multilevel_attention", [], optimizer={"cls": "Adam", "lr": 3e-3})
    assert callable(w.trainer.train_step_ragged)
    hist = w.fit(data, data[:1], {"epochs": 10, "verbose": 0})
    loss, val = hist["history"]["loss"], hist["history"]["val_loss"]
    print("ragged fit: loss per epoch %s" % " ".join("%.4f" % v for v in loss))
    assert len(loss) == 10 and np.isfinite(loss).all() and np.isfinite(val).all() and w.trainer.step_count == 30
    assert loss[-1] < 0.5 * loss[0], loss
    # evaluate: the loss computed from predict_ragged
    logs = w.evaluate(data)
    total = 0.0
    for (X, ro), y in data:
        logp = m.predict_ragged(X.cuda(), ro).cpu().numpy().astype(np.float64)
        total += -logp[np.arange(len(y)), y.numpy()].sum()
    want = total / sum(len(y) for _, y in data)
    assert abs(logs["loss"] - want) <= 1e-5 * max(1.0, abs(want)), (logs, want)
    # dense elements still take the dense path, also in one dataset with ragged ones
    xd = torch.from_numpy(np.random.default_rng(1).standard_normal((4, 12, D)).astype(np.float32))
    mixed = [(xd, torch.zeros(4, dtype=torch.int32)), data[0]]
    before = w.trainer.step_count
    w.fit(mixed, None, {"epochs": 1, "verbose": 0})
    assert w.trainer.step_count == before + 2 and np.isfinite(w.evaluate(mixed)["loss"])
