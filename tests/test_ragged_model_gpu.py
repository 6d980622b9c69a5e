"""
The ragged model pass on the device: the kernels of csrc/ragged.hip alone (pack, pad-row repair, the two pools), then
SequentialTDNN.forward_ragged / predict_ragged / embed_ragged, steps.extract_embeddings(ragged: true) and
util.predict_ragged_with_model.

Kernel outputs live in tests/guarded.Guarded buffers (NaN around the payload, NaN wherever a kernel must write, NaN between the
utterances a kernel reads).  How results are judged:
    pack, zero rows    bit for bit
    pool mean          error_bound(mean |x|, pool_chain(T, ("lds", V))): every utterance takes pool_fwd_kernel's arithmetic,
                       whatever its T -- ceil(T / 16) rows of a time group, the 16 groups, the division
    pool stddev        inside oracle stddev_interval for that chain
    whole model        every utterance against the float64 oracle on it ALONE, at the tolerances of test_model_gpu.py: 1e-3 on the
                       log-probs, cosine >= 0.9999 on the embeddings
"""
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from lidbox_amd.testutil import device_copy
from oracle import model_np as mo
from oracle import nnops_np as no

pytestmark = pytest.mark.gpu

POOL_LENGTHS = (1, 2, 15, 16, 17, 40, 41, 198)
MODEL_LENGTHS = (1, 2, 5, 6, 7, 23, 24, 25, 61, 198)


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


# ---------------------------------------------------------------------------------------------------- pack / zero rows
def _segments(lengths, pad, rng):
    """segment offsets with 0 .. 2 slack rows behind pad + frames"""
    rows = pad + np.asarray(lengths, np.int64) + rng.integers(0, 3, len(lengths))
    return np.concatenate(([0], np.cumsum(rows))).astype(np.int64)


def _run_pack(lengths, seg, C, pad, tail, mis, rng):
    """-> nothing; asserts the packed buffer bit for bit (compared on the device) and its guards"""
    nv = _nv()
    lengths = np.asarray(lengths, np.int64)
    src_off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    src = rng.standard_normal((int(src_off[-1]), C), dtype=np.float32)
    want = np.zeros((int(seg[-1]) + tail, C), np.float32)
    # frame r of the source is row seg[b] + pad + (r - src_off[b]) of the destination
    owner = np.repeat(np.arange(len(lengths)), lengths)
    want[seg[:-1][owner] + pad + np.arange(len(owner)) - src_off[:-1][owner]] = src
    dst = Guarded(want.shape, shift=1 if mis == "dst" else 0)                # NaN: every row must be written
    xs = device_copy(src, misalign=mis == "src")
    so, sg = _i64(src_off), _i64(seg)
    nv.check(nv.lib.lidbox_ragged_pack_rows(nv.ptr(xs), nv.ptr(so), dst.ptr, nv.ptr(sg), len(lengths), C, pad, tail, nv.current_stream()))
    torch.cuda.synchronize()
    dst.check()
    assert torch.equal(dst.view.view(torch.int32), torch.from_numpy(want).cuda().view(torch.int32)), (len(lengths), C, pad, mis)


def _run_zero_rows(seg, C, pad, mis, rng):
    nv = _nv()
    rows = int(seg[-1])
    init = rng.standard_normal((rows, C), dtype=np.float32)
    init[rng.random(rows) < 0.2] = np.nan                                    # what a GEMM over NaN slack leaves behind
    want = init.copy()
    for p in range(pad):
        r = seg[:-1] + p
        want[r[r < seg[1:]]] = 0.0
    x = Guarded((rows, C), init=torch.from_numpy(init), shift=1 if mis == "x" else 0)
    sg = _i64(seg)
    nv.check(nv.lib.lidbox_ragged_zero_rows(x.ptr, nv.ptr(sg), len(seg) - 1, C, pad, nv.current_stream()))
    torch.cuda.synchronize()
    x.check()
    assert torch.equal(x.view.view(torch.int32), torch.from_numpy(want).cuda().view(torch.int32)), (len(seg) - 1, C, pad, mis)


@pytest.mark.parametrize("mis", [None, "src", "dst"])
@pytest.mark.parametrize("C", [1, 3, 40, 512])
def test_pack_rows_is_bit_exact_and_writes_every_row(C, mis):
    rng = np.random.default_rng([C, 7])
    for lengths in ([3], [5, 1], [1, 2, 7, 3, 64]):                           # B = 1, 2 and a mix; 64 frames x 512: several trips of a block
        for pad in (0, 2, 4):
            _run_pack(lengths, _segments(lengths, pad, rng), C, pad, 4, mis, rng)
    _run_pack([2, 3], _segments([2, 3], 1, rng), C, 1, 0, mis, rng)            # no tail rows
    # a segment too short for its frames: the frames that do not fit are dropped, nothing is written past the segment
    nv = _nv()
    src = device_copy(np.ones((5, C), np.float32), misalign=mis == "src")
    dst = Guarded((4, C), shift=1 if mis == "dst" else 0)
    nv.check(nv.lib.lidbox_ragged_pack_rows(nv.ptr(src), nv.ptr(_i64([0, 5])), dst.ptr, nv.ptr(_i64([0, 3])), 1, C, 1, 1, nv.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(dst.numpy(), np.array([0, 1, 1, 0], np.float32)[:, None].repeat(C, 1))


@pytest.mark.parametrize("C,mis", [(1, None), (3, None), (40, None), (40, "src"), (40, "dst"), (512, None)])
def test_pack_rows_70000_segments_of_length_one(C, mis):
    """more utterances than a grid axis holds: the loop over segments strides"""
    rng = np.random.default_rng([C, 8])
    B = 70000
    seg = np.concatenate(([0], np.cumsum(2 + (np.arange(B) % 2)))).astype(np.int64)      # pad 1 + 1 frame + 0 / 1 slack
    _run_pack(np.ones(B, np.int64), seg, C, 1, 2, mis, rng)


@pytest.mark.parametrize("mis", [None, "x"])
@pytest.mark.parametrize("C", [1, 3, 40, 512])
def test_zero_rows_is_bit_exact_and_touches_nothing_else(C, mis):
    rng = np.random.default_rng([C, 9])
    for lengths in ([3], [5, 1], [1, 2, 7, 3, 64]):
        for pad in (1, 2, 4):
            _run_zero_rows(_segments(lengths, pad, rng), C, pad, mis, rng)
    _run_zero_rows(np.array([0, 1, 4], np.int64), C, 3, mis, rng)             # a pad longer than the first segment stays inside it
    B = 70000
    _run_zero_rows(np.concatenate(([0], np.cumsum(2 + (np.arange(B) % 2)))).astype(np.int64), C, 1, mis, rng)
    # pad 0: nothing to do, nothing touched
    nv = _nv()
    x = Guarded((4, C))
    nv.check(nv.lib.lidbox_ragged_zero_rows(x.ptr, nv.ptr(_i64([0, 4])), 1, C, 0, nv.current_stream()))
    torch.cuda.synchronize()
    assert np.isnan(x.numpy()).all()


# ---------------------------------------------------------------------------------------------------- pools
@functools.lru_cache(maxsize=None)
def _pool_utts(C, kind):
    rng = np.random.default_rng([C, kind == "offset"])
    xs = []
    for T in POOL_LENGTHS:
        x = rng.standard_normal((T, C))
        xs.append((1e4 + x if kind == "offset" else x).astype(np.float32))
        xs[-1].setflags(write=False)
    return tuple(xs)


def _pool_launch(fn, xs, order, rs, mis, width):
    """the utterances in `order` laid out with NaN rows between them and NaN in the row gaps -> out [B, width] in that order"""
    nv = _nv()
    C = xs[0].shape[1]
    starts, r = [], 1
    for b in order:
        starts.append(r)
        r += len(xs[b]) + 1 + (b % 2)                                        # one or two NaN rows behind every utterance
    flat = np.full(r * rs, np.nan, np.float32)
    for b, s in zip(order, starts):
        for t in range(len(xs[b])):
            flat[(s + t) * rs:(s + t) * rs + C] = xs[b][t]
    xd = device_copy(flat, misalign=mis == "x")
    out = Guarded((len(order), width), shift=1 if mis == "out" else 0)
    so, ln = _i64(starts), _i64([len(xs[b]) for b in order])
    nv.check(fn(nv.ptr(xd), rs, nv.ptr(so), nv.ptr(ln), len(order), C, out.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    return out.numpy()


@pytest.mark.parametrize("kind", ["normal", "offset"])
@pytest.mark.parametrize("C,pitch,mis", [(1, 0, None), (63, 0, None), (63, 4, None), (64, 0, None), (64, 4, None), (64, 1, None),
                                         (64, 0, "x"), (64, 0, "out"), (1500, 0, None), (1500, 4, None)])
def test_ragged_pools(C, pitch, mis, kind):
    nv = _nv()
    xs = _pool_utts(C, kind)
    B, rs = len(xs), C + pitch
    order = list(range(B))
    got = _pool_launch(nv.lib.lidbox_stats_pool_ragged_fwd, xs, order, rs, mis, 2 * C)
    avg = _pool_launch(nv.lib.lidbox_avg_pool_ragged_fwd, xs, order, rs, mis, C)
    assert np.isfinite(got).all() and _same(avg, got[:, :C])
    V = 4 if C % 4 == 0 and rs % 4 == 0 and mis != "x" else 1
    worst = 0.0
    for b, x in enumerate(xs):
        T = len(x)
        n = no.pool_chain(T, ("lds", V))
        assert n == -(-T // 16) + 17
        mean, _, _ = no.stats_pool_fwd(x[None])
        bound = no.error_bound(no.pool_mean_abs(x[None]), n)
        err = np.abs(got[b:b + 1, :C].astype(np.float64) - mean)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (T, float((err / bound).max()))
        lo, hi = no.stddev_interval(x[None], n)
        sd = got[b:b + 1, C:].astype(np.float64)
        assert (sd >= lo).all() and (sd <= hi).all(), (T, float((sd - hi).max()), float((lo - sd).max()))
    print("ragged pool C=%d rs=%d %s %s: mean err / bound <= %.3e" % (C, rs, mis, kind, worst))
    # run to run, and with the utterances in another order at other places
    assert _same(_pool_launch(nv.lib.lidbox_stats_pool_ragged_fwd, xs, order, rs, mis, 2 * C), got)
    perm = [5, 0, 7, 2, 1, 6, 3, 4]
    assert _same(_pool_launch(nv.lib.lidbox_stats_pool_ragged_fwd, xs, perm, rs, mis, 2 * C), got[perm])
    assert _same(_pool_launch(nv.lib.lidbox_avg_pool_ragged_fwd, xs, perm, rs, mis, C), avg[perm])


@pytest.mark.parametrize("C", [3, 64])
def test_ragged_pools_with_more_utterances_than_blocks(C):
    """20 000 utterances of 1 .. 3 frames: a block of the pooling kernels takes up to three utterances in turn and reuses its LDS
    sums between them.  Judged against launches of at most 8 192 utterances (one per block, the arithmetic test_ragged_pools
    holds to the oracle): the same bits; and the length-1 utterances against their own row."""
    nv = _nv()
    B = 20000
    rng = np.random.default_rng([C, 11])
    lengths = 1 + np.arange(B) % 3
    starts = np.concatenate(([0], np.cumsum(lengths)))[:-1]
    x = rng.standard_normal((int(lengths.sum()), C), dtype=np.float32)
    xd, so, ln = device_copy(x), _i64(starts), _i64(lengths)
    for fn, width in ((nv.lib.lidbox_stats_pool_ragged_fwd, 2 * C), (nv.lib.lidbox_avg_pool_ragged_fwd, C)):
        out = Guarded((B, width))
        nv.check(fn(nv.ptr(xd), C, nv.ptr(so), nv.ptr(ln), B, C, out.ptr, nv.current_stream()))
        torch.cuda.synchronize()
        got = out.numpy()
        parts = []
        for a in range(0, B, 8192):
            n = min(8192, B - a)
            part = Guarded((n, width))
            nv.check(fn(nv.ptr(xd), C, nv.ptr(so[a:a + n]), nv.ptr(ln[a:a + n]), n, C, part.ptr, nv.current_stream()))
            torch.cuda.synchronize()
            parts.append(part.numpy())
        assert np.isfinite(got).all() and _same(got, np.concatenate(parts))
        assert _same(got[lengths == 1][:, :C], x[starts[lengths == 1]])        # one frame: the mean is the frame


# ---------------------------------------------------------------------------------------------------- whole model
def _oracle(m, p, x, embedding=False):
    """float64 restatement of a SequentialTDNN without front-end or attention on ONE utterance x [T, C]"""
    h = np.asarray(x, np.float64)[None]
    for c in m.convs:
        W = p[c.name + ".W"]
        h = mo.conv1d_causal_fwd(h, W.reshape(c.k, -1, c.filters), p[c.name + ".b"], c.s, relu=c.relu)
    h = mo.stats_pool_fwd(h) if m.pool == "stats" else mo.global_avg_pool_fwd(h)
    for j, d in enumerate(m.denses):
        if embedding and j == 0:
            return mo.dense_fwd(h, p[d.name + ".W"], p[d.name + ".b"], relu=False)[0]
        h = mo.dense_fwd(h, p[d.name + ".W"], p[d.name + ".b"], relu=d.relu)
    return mo.log_softmax(h)[0]


def _make(kind):
    from lidbox_amd.models import cnn, xvector, xvector_extended
    if kind == "xvector":
        m = xvector.create((None, 40), 4, seed=0)
    elif kind == "xvector_extended":
        m = xvector_extended.create((None, 20), 6, seed=9)
    else:
        m = cnn.create((None, 24), 5, seed=3)                                 # average pooling
    rng = np.random.default_rng(22)
    m.set_weights({k: rng.standard_normal(v.shape) * 0.05 for k, v in m.get_weights().items() if k.endswith(".b")})
    return m


@functools.lru_cache(maxsize=None)
def _model_case(kind):
    """(model, float64 parameters, utterances, offsets, oracle log-probs [B, N], oracle embeddings [B, D]); computed once"""
    m = _make(kind)
    p = {k: v.astype(np.float64) for k, v in m.get_weights().items()}
    rng = np.random.default_rng(31)
    xs = [rng.standard_normal((T, m.input_dim)).astype(np.float32) for T in MODEL_LENGTHS]
    off = np.concatenate(([0], np.cumsum(MODEL_LENGTHS)))
    logp = np.stack([_oracle(m, p, x) for x in xs])
    emb = np.stack([_oracle(m, p, x, embedding=True) for x in xs])
    for a in xs + [logp, emb]:
        a.setflags(write=False)
    return m, p, xs, off, logp, emb


def _cat(xs):
    return torch.from_numpy(np.concatenate(xs)).cuda()


@pytest.mark.parametrize("kind", ["xvector", "xvector_extended", "cnn"])
def test_ragged_model_meets_the_oracle_on_every_utterance_alone(kind):
    m, p, xs, off, logp, emb = _model_case(kind)
    assert any(float(np.abs(p[c.name + ".b"]).max()) > 0 for c in m.convs)    # relu(bias) != 0 in the pad rows without the repair
    got = m.predict_ragged(_cat(xs), off).cpu().numpy()
    assert got.shape == logp.shape and np.isfinite(got).all()
    print("%s: max |ragged - oracle| on log-probs %.3e" % (kind, np.abs(got - logp).max()))
    assert np.abs(got - logp).max() < 1e-3
    from lidbox_amd.models.tdnn import EmbeddingExtractor
    e = EmbeddingExtractor(m).ragged(_cat(xs), off).cpu().numpy()
    assert e.shape == emb.shape and _cos(e, emb).min() >= 0.9999
    assert _same(m.embed_ragged(_cat(xs), off).cpu().numpy(), e)
    # against the dense pass on each utterance as its own batch (recorded; both sit within 1e-3 of the oracle)
    dense = np.stack([m(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    print("%s: max |ragged - dense own call| on log-probs %.3e" % (kind, np.abs(got - dense).max()))
    assert np.abs(dense - logp).max() < 1e-3
    # B == 0
    z = m.predict_ragged(torch.zeros((0, m.input_dim), device="cuda"), [0])
    assert tuple(z.shape) == (0, logp.shape[1])


@pytest.mark.parametrize("kind", ["xvector", "xvector_extended"])
def test_an_utterance_does_not_see_its_neighbours(kind):
    m, p, xs, off, logp, emb = _model_case(kind)
    base = m.predict_ragged(_cat(xs), off).cpu().numpy()
    base_e = m.embed_ragged(_cat(xs), off).cpu().numpy()
    rng = np.random.default_rng(41)
    for j in range(len(xs)):
        for fill in ("other", "nan"):
            ys = [x if b == j else (np.full_like(x, np.nan) if fill == "nan" else (3.0 * rng.standard_normal(x.shape)).astype(np.float32))
                  for b, x in enumerate(xs)]
            got = m.predict_ragged(_cat(ys), off).cpu().numpy()
            assert np.isfinite(got[j]).all() and _same(got[j], base[j]), (j, fill)
            if fill == "nan":
                got_e = m.embed_ragged(_cat(ys), off).cpu().numpy()
                assert np.isfinite(got_e[j]).all() and _same(got_e[j], base_e[j]), j
    # after the NaN passes the workspace is full of NaN slack: a clean pass still gives the same bits
    assert _same(m.predict_ragged(_cat(xs), off).cpu().numpy(), base)


@pytest.mark.parametrize("kind", ["xvector", "xvector_extended"])
def test_a_second_smaller_call_reuses_the_workspace(kind):
    m, p, xs, off, logp, emb = _model_case(kind)
    m.predict_ragged(_cat(xs), off)
    ws = m._rws
    ptrs = [a.data_ptr() for a in ws.act]
    pick = [6, 0, 4, 1]                                                       # lengths 24, 1, 7, 2
    sub = [xs[b] for b in pick]
    soff = np.concatenate(([0], np.cumsum([len(x) for x in sub])))
    got = m.predict_ragged(_cat(sub), soff).cpu().numpy()
    assert m._rws is ws and [a.data_ptr() for a in ws.act] == ptrs
    assert np.abs(got - logp[pick]).max() < 1e-3
    e = m.embed_ragged(_cat(sub), soff).cpu().numpy()
    assert _cos(e, emb[pick]).min() >= 0.9999
    # more utterances that fit into the rows: only the per-utterance buffers are replaced
    cap_rows, cap_B, pooled = ws.cap_rows, ws.cap_B, ws.pooled.data_ptr()
    from lidbox_amd.models.ragged import ragged_plan
    many = [xs[0]] * (2 * len(xs))                                           # length 1 each: 20 top-level rows
    assert cap_B < len(many) and ragged_plan([1] * len(many), m.convs).off[-1] <= cap_rows
    got = m.predict_ragged(_cat(many), np.arange(len(many) + 1)).cpu().numpy()
    assert m._rws is ws and ws.cap_rows == cap_rows and [a.data_ptr() for a in ws.act] == ptrs
    assert ws.cap_B >= max(len(many), cap_B + cap_B // 2) and ws.pooled.data_ptr() != pooled
    assert np.abs(got - logp[0]).max() < 1e-3 and _same(got, np.repeat(got[:1], len(many), 0))
    # more rows than fit: the level buffers grow, by at least a half, and the per-utterance buffers stay
    cap_B, pooled = ws.cap_B, ws.pooled.data_ptr()
    big = xs + xs
    got = m.predict_ragged(_cat(big), np.concatenate(([0], np.cumsum([len(x) for x in big])))).cpu().numpy()
    assert m._rws is ws and ws.cap_rows >= cap_rows + cap_rows // 2 and ws.cap_B == cap_B and ws.pooled.data_ptr() == pooled
    assert np.abs(got - np.concatenate([logp, logp])).max() < 1e-3 and _same(got[:len(xs)], got[len(xs):])


def test_refusals():
    from lidbox_amd.models import cnn, xvector, xvector_2d, xvector_freq_attention
    from lidbox_amd.models.tdnn import ConvSpec, DenseSpec, SequentialTDNN
    m, p, xs, off, logp, emb = _model_case("xvector")
    X = _cat(xs)
    with pytest.raises(ValueError, match="length 0"):
        m.predict_ragged(X, np.concatenate((off[:3], off[2:])))
    for bad in (off[1:], off[:-1], np.concatenate((off[:2], [off[3], off[2]], off[4:])), off + 1, []):
        with pytest.raises(ValueError, match="row_offsets must rise from 0"):
            m.predict_ragged(X, bad)
    with pytest.raises(ValueError, match="contiguous input"):
        m.embed_ragged(X[:, :39], off)
    with pytest.raises(ValueError, match="contiguous input"):
        m.embed_ragged(X[None], off)
    with pytest.raises(TypeError):
        m.embed_ragged(X.double(), off)
    with pytest.raises(_nv().LidboxHipError):
        m.embed_ragged(X.cpu(), off)
    x40, o2 = torch.zeros((7, 40), device="cuda"), [0, 3, 7]
    with pytest.raises(ValueError, match="2-D front-end"):
        xvector_2d.create((None, 40), 4, seed=0).predict_ragged(x40, o2)
    with pytest.raises(ValueError, match="frequency attention"):
        xvector_freq_attention.create((None, 40), 4, seed=0).predict_ragged(x40, o2)
    with pytest.raises(ValueError, match="float32 only"):
        xvector.create((None, 40), 4, seed=0, compute_dtype="bfloat16").embed_ragged(x40, o2)
    for padding in ("same", "valid"):
        with pytest.raises(ValueError, match="causal, undilated"):
            cnn.create((None, 40), 4, padding=padding, seed=0).predict_ragged(x40, o2)
    dil = SequentialTDNN((None, 40), [ConvSpec("c1", 8, 3, 1, dilation_rate=2)], "stats", [DenseSpec("d1", 8), DenseSpec("out", 3, relu=False)])
    with pytest.raises(ValueError, match="causal, undilated"):
        dil.predict_ragged(x40, o2)

    class Between(SequentialTDNN):
        def _before_conv(self, ws, i, training, update_moving):
            pass

    sub = Between((None, 40), [ConvSpec("c1", 8, 3, 1)], "stats", [DenseSpec("d1", 8), DenseSpec("out", 3, relu=False)])
    with pytest.raises(ValueError, match="_before_conv"):
        sub.predict_ragged(x40, o2)
    plain = SequentialTDNN((None, 40), [ConvSpec("c1", 8, 3, 1)], "stats", [DenseSpec("d1", 8), DenseSpec("out", 3, relu=False)])
    assert tuple(plain.predict_ragged(x40, o2).shape) == (2, 3)


# ---------------------------------------------------------------------------------------------------- pipeline surface
def test_extract_embeddings_ragged_gives_what_batch_size_one_gives():
    from lidbox_amd.data import steps
    from lidbox_amd.models import xvector
    m, p, xs, off, logp, emb = _model_case("xvector")
    ex = xvector.as_embedding_extractor(m)
    ds = [dict(id="u%d" % i, input=torch.from_numpy(x).cuda() if i % 2 else x) for i, x in enumerate(xs)]     # device and host inputs
    one = list(steps.extract_embeddings(ds, {"extractors": [ex], "batch_size": 1}))
    for bs in (4, 256):                                                       # three launches (4 + 4 + 2) / one
        rag = list(steps.extract_embeddings(ds, {"extractors": [ex, m], "batch_size": bs, "ragged": True}))
        assert [x["id"] for x in rag] == [x["id"] for x in one] == ["u%d" % i for i in range(len(xs))]
        for i, (a, b) in enumerate(zip(rag, one)):
            a, b = a["embedding"].cpu().numpy(), b["embedding"].cpu().numpy()
            assert a.shape == (1024,) and _same(a[:512], a[512:])             # two extractors, concatenated
            assert _cos(a[:512], b) >= 0.9999 and _cos(a[:512], emb[i]) >= 0.9999, i
    with pytest.raises(ValueError, match="no_unbatch"):
        list(steps.extract_embeddings(ds, {"extractors": [ex], "ragged": True, "no_unbatch": True}))
    with pytest.raises(ValueError, match="ragged form"):
        list(steps.extract_embeddings(ds, {"extractors": [lambda x: x], "ragged": True}))
    with pytest.raises(ValueError, match="one C"):
        list(steps.extract_embeddings([dict(input=torch.zeros(3, 40)), dict(input=torch.zeros(3, 39))], {"extractors": [ex], "ragged": True, "batch_size": 2}))
    assert set(steps.VALID_STEP_FUNCTIONS) == _VALID_STEPS


_VALID_STEPS = {"apply_filters", "apply_vad", "as_supervised", "augment_by_additive_noise", "augment_signals", "cache", "compute_rms_vad",
                "consume", "consume_to_tensorboard", "create_input_chunks", "create_signal_chunks", "drop_empty", "extract_embeddings",
                "extract_features", "filter_keys_in_set", "initialize", "lambda", "load_audio", "normalize", "random_signal_fir_filtering",
                "random_signal_speed_change", "remap_keys", "repeat_too_short_signals", "shuffle"}


def test_predict_ragged_with_model_equals_predict_with_model():
    from lidbox_amd import util
    m, p, xs, off, logp, emb = _model_case("xvector")
    elements = [dict(id="utt-%02d" % (len(xs) - i), input=torch.from_numpy(x).cuda()) for i, x in enumerate(xs)]
    dense = util.predict_with_model(m, [dict(id=[e["id"]], input=e["input"][None]) for e in elements])
    for lb in (256, 3):
        rag = util.predict_ragged_with_model(m, iter(elements), launch_batch=lb)
        assert list(rag.index) == list(dense.index) and list(rag.columns) == list(dense.columns)
        a, b = np.stack(rag.prediction.values), np.stack(dense.prediction.values)
        assert a.shape == b.shape == logp.shape and np.abs(a - b).max() < 1e-3
    assert np.abs(np.stack(rag.loc[[e["id"] for e in elements]].prediction.values) - logp).max() < 1e-3
