"""
The ragged pass of crnn and clstm on the device: the three ragged kernels of csrc/conv2d.hip through the C ABI, then
forward_ragged / predict_ragged / embed_ragged of both models, steps.extract_embeddings(ragged: true) and
util.predict_ragged_with_model.

Kernel level.  Every output is a tests/guarded.py payload (NaN inside and around).  How results are judged:
    1. bit for bit against the dense call (lidbox_conv2d_fwd, lidbox_conv2d_strided_fwd, lidbox_bn_maxpool2d_fwd) on every
       utterance alone, B = 1, T = T_b;
    2. stride-1 case a and the first strided layer also element by element against oracle/conv2d_np.py's float64 convolution
       within its error_bound (n = the k-chain plus the bias add, as tests/test_conv2d_paths_gpu.py judges the dense kernels);
    3. the same bits for an utterance in a permuted batch (other neighbours, another place, other tiles);
    4. a smaller call into the buffers a larger call left full: the bits of a fresh call, the rest as the larger call left it;
    5. run-to-run identity, B = 0, and every refusal with nothing written.

Model level.  crnn at test_crnn_gpu's _small sizes with randomised BatchNormalization state and negative gammas, F = 33 and 70,
lengths 32 .. 100; clstm for all five FLAGS rows of test_clstm_gpu at F = 40 and 20 with reduced widths, lengths 1 .. 33.  Every
utterance of predict_ragged / embed_ragged against the float64 transcription of that utterance alone and against the model's own
dense call on it alone, at the dense model tests' own H_TOL (crnn 5e-6, clstm 3e-6).
"""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import conv2d_np as co

pytestmark = pytest.mark.gpu


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _off(lengths):
    return np.concatenate(([0], np.cumsum(np.asarray(lengths, np.int64)))).astype(np.int64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _split(y, off):
    return [y[off[b]:off[b + 1]] for b in range(len(off) - 1)]


# ---------------------------------------------------------------------------------------------------- stride-1 convolution
_rs = np.random.default_rng(77)
CONV_CASES = {
    "a": dict(F=5, ci=1, co=16, k=7, lengths=[1, 2, 3, 7, 40, 1, 26, 6]),
    "b": dict(F=8, ci=16, co=32, k=3, lengths=[16, 16, 1, 31, 16]),
    "c": dict(F=3, ci=16, co=64, k=5, lengths=_rs.permutation(np.tile(np.arange(1, 10), 8)[:70]).tolist() + [130]),
    "d": dict(F=33, ci=1, co=16, k=7, lengths=[32, 37, 100]),
}


def _conv_ragged(xs, W, b, relu, F, out=None):
    """the ragged call on the utterances xs ([T_b, F, ci] each) -> (y [total_T, F, co] as numpy, its Guarded buffer)"""
    nv = _nv()
    off = _off([len(x) for x in xs])
    total, ci, k, cout = int(off[-1]), xs[0].shape[2], W.shape[0], W.shape[3]
    y = out or Guarded((total, F, cout))
    xd, od, Wd, bd = _dev(np.concatenate(xs)), _dev(off), _dev(W), None if b is None else _dev(b)
    nv.check(nv.lib.lidbox_conv2d_ragged_fwd(nv.ptr(xd), nv.ptr(od), len(xs), total, F, ci, nv.ptr(Wd), k, cout, nv.ptr(bd), relu,
                                             y.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy().reshape(-1, F, cout)[:total], y


def _conv_dense(x, W, b, relu):
    nv = _nv()
    T, F, ci = x.shape
    y = Guarded((T, F, W.shape[3]))
    xd, Wd, bd = _dev(x), _dev(W), None if b is None else _dev(b)
    nv.check(nv.lib.lidbox_conv2d_fwd(nv.ptr(xd), 1, T, F, ci, nv.ptr(Wd), W.shape[0], W.shape[3], nv.ptr(bd), relu, y.ptr,
                                      nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy()


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    c = CONV_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    xs = [rng.standard_normal((T, c["F"], c["ci"])).astype(np.float32) for T in c["lengths"]]
    W = (rng.standard_normal((c["k"], c["k"], c["ci"], c["co"])) / c["k"]).astype(np.float32)
    b = rng.standard_normal(c["co"]).astype(np.float32)
    return xs, W, b


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_ragged_equals_dense_per_utterance(name, relu):
    xs, W, b = _conv_case(name)
    F = CONV_CASES[name]["F"]
    y, _ = _conv_ragged(xs, W, b, relu, F)
    assert np.isfinite(y).all()
    off = _off([len(x) for x in xs])
    for i, (x, got) in enumerate(zip(xs, _split(y, off))):
        assert _same_bits(got, _conv_dense(x, W, b, relu)), (name, i, len(x))
    if name == "a":
        worst = 0.0
        for x, got in zip(xs, _split(y, off)):
            ref, S = co.fwd(x[None], W, b, W.shape[0], relu=bool(relu))[0], co.abs_bound_fwd(x[None], W, b, W.shape[0])[0]
            err, bound = np.abs(got - ref), co.error_bound(S, W.shape[0] ** 2 * x.shape[2] + 1)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all()
        print("conv ragged case a relu=%d: worst error / bound %.3g" % (relu, worst))
    # run to run
    assert _same_bits(_conv_ragged(xs, W, b, relu, F)[0], y)


def test_conv_ragged_without_bias_and_single_utterance():
    xs, W, b = _conv_case("a")
    y, _ = _conv_ragged(xs, W, None, 0, 5)
    for x, got in zip(xs, _split(y, _off([len(x) for x in xs]))):
        assert _same_bits(got, _conv_dense(x, W, None, 0))
    # case e: B = 1 is the dense call
    for name in ("b", "d"):
        xs, W, b = _conv_case(name)
        x = np.concatenate(xs)
        assert _same_bits(_conv_ragged([x], W, b, 1, x.shape[1])[0], _conv_dense(x, W, b, 1))


@pytest.mark.parametrize("name", ["a", "c"])
def test_conv_ragged_permuted_batch_and_reused_buffer(name):
    xs, W, b = _conv_case(name)
    F = CONV_CASES[name]["F"]
    y, buf = _conv_ragged(xs, W, b, 1, F)
    off = _off([len(x) for x in xs])
    perm = np.random.default_rng(5).permutation(len(xs))
    yp, _ = _conv_ragged([xs[i] for i in perm], W, b, 1, F)
    offp = _off([len(xs[i]) for i in perm])
    for j, i in enumerate(perm):
        assert _same_bits(yp[offp[j]:offp[j + 1]], y[off[i]:off[i + 1]]), (name, i)
    # a smaller call into the buffer the larger one left full
    sub = xs[2:5]
    fresh, _ = _conv_ragged(sub, W, b, 1, F)
    again, _ = _conv_ragged(sub, W, b, 1, F, out=buf)
    n = len(fresh)
    full = buf.numpy()
    assert _same_bits(full[:n], fresh) and _same_bits(full[n:], y[n:]) and _same_bits(again, fresh)


# ---------------------------------------------------------------------------------------------------- BN + MaxPool2D
POOL_LENGTHS = [1, 2, 3, 7, 40, 1, 26, 6]
POOL_ROWS = [0, 1, 1, 3, 20, 0, 13, 3]


def _pool_case():
    rng = np.random.default_rng(11)
    F, C = 5, 16
    xs = [rng.standard_normal((T, F, C)).astype(np.float32) for T in POOL_LENGTHS]
    # planted exact ties inside 2 x 2 windows: all four equal, the two of one time row equal, a diagonal pair
    xs[4][0:2, 0:2, 0] = 1.5
    xs[4][2, 2:4, 4] = xs[4][2:4, 2:4, 4].max() + 1.0
    xs[4][4, 0, 5] = xs[4][5, 1, 5] = xs[4][4:6, 0:2, 5].max() + 1.0
    xs[4][7, 0, 7] = xs[4][6, 1, 7] = xs[4][6:8, 0:2, 7].max() + 1.0       # (freq 0, time 1) and (freq 1, time 0): codes 1 and 2
    xs[6][0:2, 2:4, 7] = -2.0
    scale = rng.uniform(0.5, 1.5, C).astype(np.float32)
    scale[::3] *= -1                                   # negative scales: the minimum of x wins
    scale[5] = 1.0
    shift = rng.standard_normal(C).astype(np.float32)
    return xs, scale, shift


def _pool_ragged(xs, scale, shift, slack, with_code=True, out=None):
    """-> (per-utterance pooled rows, per-utterance codes or None, (y, code) buffers); output segment b has slack[b] further
    rows, which must stay as they were (NaN / 0xA5 in a fresh buffer)"""
    nv = _nv()
    F, C = xs[0].shape[1:]
    ioff = _off([len(x) for x in xs])
    rows = [len(x) // 2 for x in xs]
    ooff = _off([r + s for r, s in zip(rows, slack)])
    total_out = int(ooff[-1])
    y, code = out or (Guarded((max(total_out, 1), F // 2, C)), Guarded((max(total_out, 1), F // 2, C), dtype=torch.uint8))
    xd, id_, od, sc, sh = _dev(np.concatenate(xs)), _dev(ioff), _dev(ooff), _dev(scale), _dev(shift)
    nv.check(nv.lib.lidbox_bn_maxpool2d_ragged_fwd(nv.ptr(xd), nv.ptr(id_), len(xs), F, C, nv.ptr(sc), nv.ptr(sh), y.ptr, nv.ptr(od),
                                                   total_out, code.ptr if with_code else None, nv.current_stream()))
    torch.cuda.synchronize()
    yn, cn = y.numpy(), code.numpy()
    ys, cs = [], []
    for b in range(len(xs)):
        ys.append(yn[ooff[b]:ooff[b] + rows[b]])
        cs.append(cn[ooff[b]:ooff[b] + rows[b]])
        if out is None:
            assert np.isnan(yn[ooff[b] + rows[b]:ooff[b + 1]]).all() and (cn[ooff[b] + rows[b]:ooff[b + 1]] == 0xA5).all(), b
    if not with_code:
        assert (cn == 0xA5).all()
    return ys, cs if with_code else None, (y, code)


def _pool_dense(x, scale, shift):
    nv = _nv()
    T, F, C = x.shape
    y, code = Guarded((T // 2, F // 2, C)), Guarded((T // 2, F // 2, C), dtype=torch.uint8)
    xd, sc, sh = _dev(x), _dev(scale), _dev(shift)
    nv.check(nv.lib.lidbox_bn_maxpool2d_fwd(nv.ptr(xd), 1, T, F, C, nv.ptr(sc), nv.ptr(sh), y.ptr, code.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy(), code.numpy()


def test_pool_ragged_equals_dense_per_utterance():
    xs, scale, shift = _pool_case()
    slack = [1, 0, 2, 0, 1, 3, 0, 1]
    ys, cs, bufs = _pool_ragged(xs, scale, shift, slack)
    assert [len(y) for y in ys] == POOL_ROWS
    for b, x in enumerate(xs):
        if len(x) < 2:
            continue                                        # T_b = 1: nothing written (the slack check saw the segment)
        yd, cd = _pool_dense(x, scale, shift)
        assert _same_bits(ys[b], yd) and np.array_equal(cs[b], cd), b
        ref, code = co.bn_maxpool2d(x[None], scale, shift)
        assert np.array_equal(cs[b], code[0]), b            # the tie rule: first maximum in the reference's scan order
        # fp32 x scale + shift with one rounding or two: at most 2 u (|x scale| + |shift|) from the float64 value
        assert np.abs(ys[b] - ref[0]).max() <= 2 * co.U * (np.abs(x).max() * np.abs(scale).max() + np.abs(shift).max())
    assert cs[4][0, 0, 0] == 0 and cs[6][0, 1, 7] == 0 and cs[4][1, 1, 4] == 0 and cs[4][2, 0, 5] == 0     # planted ties
    assert cs[4][3, 0, 7] == 1
    # argmax NULL: the same values, the code buffer untouched; run to run
    ys2, _, _ = _pool_ragged(xs, scale, shift, slack, with_code=False)
    ys3, cs3, _ = _pool_ragged(xs, scale, shift, slack)
    for b in range(len(xs)):
        assert _same_bits(ys2[b], ys[b]) and _same_bits(ys3[b], ys[b]) and np.array_equal(cs3[b], cs[b])
    # permuted batch, other slack
    perm = [4, 0, 7, 6, 1, 3, 5, 2]
    yp, cp, _ = _pool_ragged([xs[i] for i in perm], scale, shift, [0, 1, 0, 2, 0, 0, 1, 0])
    for j, i in enumerate(perm):
        assert _same_bits(yp[j], ys[i]) and np.array_equal(cp[j], cs[i]), i
    # a smaller call into the buffers the larger one left full
    before = bufs[0].numpy().copy()
    sub, sl = xs[3:5], [1, 0]
    fresh, fc, _ = _pool_ragged(sub, scale, shift, sl)
    again, ac, _ = _pool_ragged(sub, scale, shift, sl, out=bufs)
    after = bufs[0].numpy()
    for b in range(2):
        assert _same_bits(again[b], fresh[b]) and np.array_equal(ac[b], fc[b])
    assert _same_bits(after[3], before[3]) and _same_bits(after[24:], before[24:])     # row 3: the first segment's slack row


# ---------------------------------------------------------------------------------------------------- strided convolution
S_LENGTHS = [1, 2, 3, 50, 130, 1, 64, 64]


def _co_taps(t):
    return co.Taps(t.kt, t.kf, t.sf, t.pt0, t.pt1, t.pf0, t.pf1, t.time_first)


def _sconv_ragged(xs, W, b, taps, Fo, out=None):
    nv = _nv()
    off = _off([len(x) for x in xs])
    total, F, ci, cout = int(off[-1]), xs[0].shape[1], xs[0].shape[2], W.shape[3]
    y = out or Guarded((total, Fo, cout))
    xd, od, Wd, bd = _dev(np.concatenate(xs)), _dev(off), _dev(W), None if b is None else _dev(b)
    nv.check(nv.lib.lidbox_conv2d_strided_ragged_fwd(nv.ptr(xd), nv.ptr(od), len(xs), total, F, ci, nv.ptr(Wd), taps, cout,
                                                     nv.ptr(bd), y.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy().reshape(-1, Fo, cout)[:total], y


def _sconv_dense(x, W, b, taps, Fo):
    nv = _nv()
    T, F, ci = x.shape
    y = Guarded((T, Fo, W.shape[3]))
    xd, Wd, bd = _dev(x), _dev(W), None if b is None else _dev(b)
    nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(xd), 1, T, F, ci, nv.ptr(Wd), taps, W.shape[3], nv.ptr(bd), y.ptr,
                                              nv.current_stream()))
    torch.cuda.synchronize()
    return y.numpy()


@pytest.mark.parametrize("layer", [0, 1])
def test_sconv_ragged_equals_dense_per_utterance(layer):
    from lidbox_amd.models import clstm
    Fi, Fo, taps = clstm.conv2d_taps(40)[layer]
    assert (Fi, Fo) == ((40, 7), (7, 2))[layer]
    ci, cout = (1, 16) if layer == 0 else (16, 32)
    rng = np.random.default_rng(20 + layer)
    xs = [rng.standard_normal((T, Fi, ci)).astype(np.float32) for T in S_LENGTHS]
    W = (rng.standard_normal((taps.kt, taps.kf, ci, cout)) / 5).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    y, buf = _sconv_ragged(xs, W, b, taps, Fo)
    off = _off(S_LENGTHS)
    worst = 0.0
    for i, (x, got) in enumerate(zip(xs, _split(y, off))):
        assert _same_bits(got, _sconv_dense(x, W, b, taps, Fo)), (layer, i)
        if layer == 0:
            t = _co_taps(taps)
            ref, S = co.fwd(x[None], W, b, t)[0], co.abs_bound_fwd(x[None], W, b, t)[0]
            err, bound = np.abs(got - ref), co.error_bound(S, t.kt * t.kf * ci + 1)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all()
    if layer == 0:
        print("strided ragged layer 1: worst error / bound %.3g" % worst)
    assert _same_bits(_sconv_ragged(xs, W, b, taps, Fo)[0], y)                     # run to run
    assert _same_bits(_sconv_ragged(xs, W, None, taps, Fo)[0][off[3]:off[4]], _sconv_dense(xs[3], W, None, taps, Fo))
    perm = [4, 7, 0, 3, 5, 6, 2, 1]
    yp, _ = _sconv_ragged([xs[i] for i in perm], W, b, taps, Fo)
    offp = _off([S_LENGTHS[i] for i in perm])
    for j, i in enumerate(perm):
        assert _same_bits(yp[offp[j]:offp[j + 1]], y[off[i]:off[i + 1]]), i
    sub = xs[1:4]
    fresh, _ = _sconv_ragged(sub, W, b, taps, Fo)
    _sconv_ragged(sub, W, b, taps, Fo, out=buf)
    full = buf.numpy()
    assert _same_bits(full[:len(fresh)], fresh) and _same_bits(full[len(fresh):], y[len(fresh):])


# ---------------------------------------------------------------------------------------------------- B = 0 and refusals
def test_empty_batches_and_refusals_write_nothing():
    from lidbox_amd.models import clstm
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    d = _dev(np.ones(4096, np.float32))
    o = _dev(_off([3, 2]))
    y, code = Guarded((4096,)), Guarded((4096,), dtype=torch.uint8)
    p, op = nv.ptr(d), nv.ptr(o)
    taps = clstm.conv2d_taps(40)[0][2]
    OK, INVALID = 0, -1                                       # LIDBOX_OK, LIDBOX_E_INVALID

    def conv(x=p, off=op, B=2, T=5, F=4, ci=1, W=p, k=3, cout=16, yy=y.ptr):
        return lib.lidbox_conv2d_ragged_fwd(x, off, B, T, F, ci, W, k, cout, p, 1, yy, st)

    def sconv(x=p, off=op, B=2, T=5, F=40, ci=1, W=p, t=taps, cout=16, yy=y.ptr):
        return lib.lidbox_conv2d_strided_ragged_fwd(x, off, B, T, F, ci, W, t, cout, p, yy, st)

    def pool(x=p, ioff=op, B=2, F=4, C=16, sc=p, sh=p, yy=y.ptr, ooff=op, total=5, cc=code.ptr):
        return lib.lidbox_bn_maxpool2d_ragged_fwd(x, ioff, B, F, C, sc, sh, yy, ooff, total, cc, st)

    # B = 0 and no rows: LIDBOX_OK, no launch
    for rc in (conv(B=0), conv(T=0), sconv(B=0), sconv(T=0), pool(B=0), pool(total=0)):
        assert rc == OK
    bad_taps = nv.Conv2DTaps(taps.kt, taps.kf, taps.sf, 0, 1, taps.pf0, taps.pf1, 1)           # pt0 + pt1 != kt - 1
    refused = [conv(x=None), conv(off=None), conv(W=None), conv(yy=None), conv(B=-1), conv(T=-1), conv(cout=24), conv(cout=0),
               conv(k=4), conv(F=0), conv(ci=0),
               sconv(x=None), sconv(off=None), sconv(W=None), sconv(yy=None), sconv(B=-1), sconv(T=-1), sconv(cout=8),
               sconv(t=bad_taps),
               pool(x=None), pool(ioff=None), pool(sc=None), pool(sh=None), pool(yy=None), pool(ooff=None), pool(B=-1), pool(F=1),
               pool(C=0), pool(total=-1)]
    assert all(rc == INVALID for rc in refused), refused
    assert sconv(t=bad_taps) == INVALID and "pt0 + pt1 == kt - 1" in nv.last_error()
    torch.cuda.synchronize()
    assert np.isnan(y.numpy()).all() and (code.numpy() == 0xA5).all()


# ---------------------------------------------------------------------------------------------------- crnn
CRNN_LENGTHS = [32, 37, 64, 65, 100, 33, 95, 63]
CRNN_TOL = 5e-6


def _crnn_dense_embedding(m, x):
    ws = m.workspace(1, x.shape[0])
    m._load_input(ws, torch.from_numpy(x[None]).cuda(), False)
    return m.forward_ws(ws, stop_before_output=True).clone().cpu().numpy()[0]


@functools.lru_cache(maxsize=None)
def _crnn_case(F):
    """(model, utterances, X, offsets, float64 probabilities [B, N], float64 embeddings [B, 2H]) -- computed once, never changed"""
    from test_crnn_gpu import _randomise, _small, _torch_model
    rng = np.random.default_rng(F)
    m = _small(T=100, F=F)
    _randomise(m, rng)
    xs = [rng.standard_normal((T, F)).astype(np.float32) for T in CRNN_LENGTHS]
    w = m.get_weights()
    _, fwd = _torch_model(w, 0.001)
    H2 = w["output.W"].shape[0]
    _, fwd_h = _torch_model(dict(w, **{"output.W": np.eye(H2), "output.b": np.zeros(H2)}), 0.001)     # logits = the final states
    out = np.stack([torch.softmax(fwd(x[None], False)[0], 1).detach().numpy()[0] for x in xs])
    emb = np.stack([fwd_h(x[None], False)[0].detach().numpy()[0] for x in xs])
    return m, xs, torch.from_numpy(np.concatenate(xs)).cuda(), _off(CRNN_LENGTHS), out, emb


@pytest.mark.parametrize("F", [33, 70])
def test_crnn_ragged_matches_transcription_and_dense_per_utterance(F):
    m, xs, X, off, out_ref, emb_ref = _crnn_case(F)
    assert m.ragged_refusal() is None
    out, emb = m.predict_ragged(X, off).cpu().numpy(), m.embed_ragged(X, off).cpu().numpy()
    assert out.shape == out_ref.shape and emb.shape == emb_ref.shape
    dense = np.stack([m(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    dense_emb = np.stack([_crnn_dense_embedding(m, x) for x in xs])
    e = [np.abs(out - out_ref).max(), np.abs(out - dense).max(), np.abs(emb - emb_ref).max(), np.abs(emb - dense_emb).max()]
    print("crnn F=%d ragged: predict vs float64 %.3g, vs dense %.3g; embed vs float64 %.3g, vs dense %.3g" % (F, *e))
    assert max(e) <= CRNN_TOL, e
    # a second, smaller call reuses the workspace
    ws, caps = m._rws, (m._rws.cap_rows, m._rws.cap_rec, m._rws.cap_B)
    few = m.predict_ragged(X[off[1]:off[4]], off[1:5] - off[1]).cpu().numpy()
    assert m._rws is ws and (ws.cap_rows, ws.cap_rec, ws.cap_B) == caps
    assert np.abs(few - out_ref[1:4]).max() <= CRNN_TOL
    assert m.predict_ragged(X[:0], [0]).shape == (0, out_ref.shape[1])


@pytest.mark.parametrize("F", [33, 70])
def test_crnn_zero_padded_dense_batch_is_a_different_computation(F):
    """what the feature is for: the dense call on the batch zero-padded to 100 frames misses the tolerance on every shorter
    utterance (relu(bias) grows into the pad frames, the reverse LSTM starts inside them), the ragged pass meets it on all"""
    m, xs, X, off, out_ref, _ = _crnn_case(F)
    padded = np.zeros((len(xs), max(CRNN_LENGTHS), F), np.float32)
    for b, x in enumerate(xs):
        padded[b, :len(x)] = x
    err = np.abs(m(torch.from_numpy(padded).cuda()).cpu().numpy() - out_ref).max(1)
    rag = np.abs(m.predict_ragged(X, off).cpu().numpy() - out_ref).max(1)
    print("crnn F=%d per utterance: padded dense batch %s\n   ragged %s" % (F, err, rag))
    for b, T in enumerate(CRNN_LENGTHS):
        assert rag[b] <= CRNN_TOL
        assert (err[b] > CRNN_TOL) == (T < max(CRNN_LENGTHS)), (b, T, err[b])


def test_crnn_workspace_grows_to_the_same_bits():
    """a model whose first ragged call is small: the second, full call grows rows, BLSTM rows and utterances, and gives the
    bits of the model that saw the full call first"""
    from test_crnn_gpu import _small
    F = 33
    big, xs, X, off, out_ref, _ = _crnn_case(F)
    m = _small(T=100, F=F)
    m.set_weights(big.get_weights())
    few = m.predict_ragged(X[off[1]:off[4]], off[1:5] - off[1]).cpu().numpy()
    assert np.abs(few - out_ref[1:4]).max() <= CRNN_TOL
    ws = m._rws
    caps, old = (ws.cap_rows, ws.cap_rec, ws.cap_B), (ws.y, ws.x, ws.hlast)
    out = m.predict_ragged(X, off).cpu().numpy()
    assert np.abs(out - out_ref).max() <= CRNN_TOL
    assert _same_bits(out, big.predict_ragged(X, off).cpu().numpy())
    assert m._rws is ws and all(new > was for new, was in zip((ws.cap_rows, ws.cap_rec, ws.cap_B), caps)), caps
    assert all(new.data_ptr() != was.data_ptr() for new, was in zip((ws.y, ws.x, ws.hlast), old))


# ---------------------------------------------------------------------------------------------------- clstm
CLSTM_LENGTHS = [1, 4, 20, 7, 6, 33, 2, 11]
CLSTM_TOL = 3e-6
CLSTM_WIDTHS = dict(filters=(16, 32), frame_units=(32, 48, 32, 32, 60), segment_units=(24, 16))


@functools.lru_cache(maxsize=None)
def _clstm_case(flag, F):
    from test_clstm_gpu import FLAGS, _model, _transcription
    flags = FLAGS[flag]
    rng = np.random.default_rng(F + len(flag))
    m = _model(flags, 33, F, seed=F, **CLSTM_WIDTHS)
    for n in m.state_layout:                                  # BatchNormalization state off its initial (0, 1)
        shape = tuple(m.param(n).shape)
        v = rng.uniform(0.5, 1.5, shape) if n.endswith("variance") else rng.standard_normal(shape) * 0.3
        m.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    for n in m.layout:
        if n.endswith("_bn.gamma") or n.endswith("_bn.beta"):
            v = (1.0 if n.endswith("gamma") else 0.0) + rng.standard_normal(tuple(m.param(n).shape)) * 0.2
            if n.endswith("gamma"):
                v[::3] *= -1
            m.param(n).copy_(torch.from_numpy(v.astype(np.float32)))
    xs = [rng.standard_normal((T, F)).astype(np.float32) for T in CLSTM_LENGTHS]
    w = m.get_weights()
    _, fwd = _transcription(w, flags)
    out = np.stack([fwd(x[None], False)[0].detach().numpy()[0] for x in xs])
    # the embedding e = pooled W1 + b1 (in front of segment1's ReLU) through the same transcription: segment1 -> (e, -e), the
    # ReLUs keep (e+, e-), the output layer takes their difference, and log_softmax is switched off for the call
    W1, b1 = np.asarray(w["segment1.W"], np.float64), np.asarray(w["segment1.b"], np.float64)
    D = len(b1)
    eye = np.eye(D)
    w2 = dict(w, **{"segment1.W": np.concatenate([W1, -W1], 1), "segment1.b": np.concatenate([b1, -b1]),
                    "segment2.W": np.eye(2 * D), "segment2.b": np.zeros(2 * D),
                    "output.W": np.concatenate([eye, -eye], 0), "output.b": np.zeros(D)})
    _, fwd_e = _transcription(w2, flags)
    with mock.patch.object(torch, "log_softmax", lambda v, dim: v):
        emb = np.stack([fwd_e(x[None], False)[0].detach().numpy()[0] for x in xs])
    return m, xs, torch.from_numpy(np.concatenate(xs)).cuda(), _off(CLSTM_LENGTHS), out, emb


@pytest.mark.parametrize("F", [40, 20])
@pytest.mark.parametrize("flag", ["none", "conv2d", "lstm", "attention", "all"])
def test_clstm_ragged_matches_transcription_and_dense_per_utterance(flag, F):
    m, xs, X, off, out_ref, emb_ref = _clstm_case(flag, F)
    assert m.ragged_refusal() is None
    out, emb = m.predict_ragged(X, off).cpu().numpy(), m.embed_ragged(X, off).cpu().numpy()
    assert out.shape == out_ref.shape and emb.shape == emb_ref.shape
    dense = np.stack([m(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    dense_emb = np.stack([m.embed(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    e = [np.abs(out - out_ref).max(), np.abs(out - dense).max(), np.abs(emb - emb_ref).max(), np.abs(emb - dense_emb).max()]
    print("clstm %s F=%d ragged: predict vs float64 %.3g, vs dense %.3g; embed vs float64 %.3g, vs dense %.3g" % (flag, F, *e))
    assert max(e) <= CLSTM_TOL, e
    # a second, smaller call reuses the workspace
    ws, caps = m._rws, (m._rws.cap_rows, m._rws.cap_frames, m._rws.cap_B)
    few = m.predict_ragged(X[off[2]:off[5]], off[2:6] - off[2]).cpu().numpy()
    assert m._rws is ws and (ws.cap_rows, ws.cap_frames, ws.cap_B) == caps
    assert np.abs(few - out_ref[2:5]).max() <= CLSTM_TOL
    assert m.predict_ragged(X[:0], [0]).shape == (0, out_ref.shape[1])


@pytest.mark.parametrize("flag", ["lstm", "attention", "all"])
def test_clstm_workspace_grows_to_the_same_bits(flag):
    """a model whose first ragged call is utterances 2..4: the second call, all eight, grows rows, frames and utterances; the
    level buffers and the LSTM / attention buffers sized off them are replaced together; the result has the bits of the model
    that saw the large call first"""
    from test_clstm_gpu import FLAGS, _model
    F = 20
    big, xs, X, off, out_ref, _ = _clstm_case(flag, F)
    m = _model(FLAGS[flag], 33, F, seed=F, **CLSTM_WIDTHS)
    m.set_weights(big.get_weights())
    few = m.predict_ragged(X[off[2]:off[5]], off[2:6] - off[2]).cpu().numpy()
    assert np.abs(few - out_ref[2:5]).max() <= CLSTM_TOL
    ws = m._rws
    extras = [n for n, on in (("zg", m.use_lstm), ("cseq", m.use_lstm), ("lstm_hseq", m.use_lstm), ("fa_x1", m.use_attention),
                              ("fa_F", m.use_attention), ("hw", m.use_attention)) if on]
    caps, old = (ws.cap_rows, ws.cap_frames, ws.cap_B), [ws.act[3], ws.act[-1]] + [getattr(ws, n) for n in extras]
    cv_out = getattr(ws, "cv_out", None)
    out = m.predict_ragged(X, off).cpu().numpy()
    assert np.abs(out - out_ref).max() <= CLSTM_TOL
    assert _same_bits(out, big.predict_ragged(X, off).cpu().numpy())
    assert m._rws is ws and all(new > was for new, was in zip((ws.cap_rows, ws.cap_frames, ws.cap_B), caps)), caps
    # the old buffers are still referenced, so a new buffer cannot have an old one's address
    new = [ws.act[3], ws.act[-1]] + [getattr(ws, n) for n in extras]
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(new, old)), extras
    H = m.lstm_units
    if m.use_lstm:
        R3 = ws.act[3].shape[0]
        assert ws.zg.numel() == R3 * 4 * H and ws.cseq.numel() == R3 * H and tuple(ws.lstm_hseq.shape) == (R3 + 1, H)
    if m.use_attention:
        assert ws.hw.shape == ws.act[-1].shape and ws.fa_x1.shape[0] == ws.fa_F.shape[0] == ws.act[-1].shape[0]
    if flag == "all":
        assert ws.cv_out.data_ptr() != cv_out.data_ptr() and ws.cv_out.shape[0] == ws.cap_frames == int(off[-1]) > cv_out.shape[0]
        assert all(t.shape[0] == ws.cap_frames for t in ws.cv_y + [ws.cv_a1])


# ---------------------------------------------------------------------------------------------------- entry points, refusals
def test_pipeline_entry_points_run_crnn_and_clstm():
    from lidbox_amd import util
    from lidbox_amd.data import steps
    for name, (m, xs, X, off, out_ref, emb_ref), tol in (("crnn", _crnn_case(33), CRNN_TOL), ("clstm", _clstm_case("all", 40), CLSTM_TOL)):
        ds = [dict(id="u%d" % i, input=torch.from_numpy(x).cuda() if i % 2 else x) for i, x in enumerate(xs)]
        for bs in (3, 256):
            rag = list(steps.extract_embeddings(ds, {"extractors": [m], "batch_size": bs, "ragged": True}))
            assert [x["id"] for x in rag] == ["u%d" % i for i in range(len(xs))]
            got = np.stack([x["embedding"].cpu().numpy() for x in rag])
            assert got.shape == emb_ref.shape and np.abs(got - emb_ref).max() <= tol, (name, bs)
        elements = [dict(id="utt-%02d" % (len(xs) - i), input=torch.from_numpy(x).cuda()) for i, x in enumerate(xs)]
        dense = util.predict_with_model(m, [dict(id=[e["id"]], input=e["input"][None]) for e in elements])
        for lb in (256, 3):
            rag = util.predict_ragged_with_model(m, iter(elements), launch_batch=lb)
            assert list(rag.index) == list(dense.index) and list(rag.columns) == list(dense.columns)
            a, b = np.stack(rag.prediction.values), np.stack(dense.prediction.values)
            assert a.shape == b.shape and np.abs(a - b).max() <= tol, name
        assert np.abs(np.stack(rag.loc[[e["id"] for e in elements]].prediction.values) - out_ref).max() <= tol


@pytest.mark.parametrize("name", ["crnn", "clstm"])
def test_model_refusals(name):
    m, xs, X, off, _, _ = _crnn_case(33) if name == "crnn" else _clstm_case("all", 40)
    C = X.shape[1]
    with pytest.raises(ValueError, match="length 0"):
        m.predict_ragged(X, [0, 40, 40, len(X)])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, off[:-1])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, [1, len(X)])
    with pytest.raises(ValueError, match=r"\[total_T, %d\]" % C):
        m.predict_ragged(torch.zeros((64, C + 1), device="cuda"), [0, 64])
    with pytest.raises(ValueError, match="contiguous"):
        m.predict_ragged(torch.zeros((64, 2 * C), device="cuda")[:, :C], [0, 64])
    with pytest.raises(Exception):
        m.predict_ragged(X.cpu(), off)
    if name == "crnn":
        with pytest.raises(ValueError, match=r"utterance 1 has 31 frames.*too small for 5 pooling layers"):
            m.embed_ragged(X[:63], [0, 32, 63])
    # and the model still answers
    assert m.predict_ragged(X, off).shape[0] == len(xs)
