"""
The ragged pass of multilevel_attention on the device: lidbox_mla_attention_ragged_fwd through the C ABI, then forward_ragged /
predict_ragged / embed_ragged of the model, steps.extract_embeddings(ragged: true) and util.predict_ragged_with_model.  Cases,
weights and the float64 transcription are tests/ragged_mla_cases.py's.

Kernel level.  z is a tests/guarded.py payload, att a column slice (offset K + 1) of a guarded [B, 2 K + 3] buffer, colsum a
guarded [B, K].  How results are judged:
    1. bit for bit against lidbox_mla_attention_fwd on every utterance alone (z + row_offsets[b] K, B = 1, T = T_b), for K
       values that reach all eight (VEC, NJ) pairs, two of them through a base 4 bytes off a 16-byte boundary, with lengths
       that bracket one pass of the row loop, in shuffled order; and with colsum = NULL, where att keeps its bits;
    2. every utterance against oracle/update_paths_np.mla_fwd_ref (float64) within its bound for mla_fwd_plan(T_b, K, vec4);
    3. the same bits in a permuted batch, beside a NaN utterance and in a second run; guard words and the other columns of att
       untouched;
    4. B = 0 and every refusal with nothing written.

Model level.  (D, K, H, L) = (8, 5, 24, 2) and (8, 100, 64, 3), lengths 1 .. 298, random moving statistics, no zero bias.
H_TOL = 5e-5 absolute (tests/test_multilevel_attention_gpu.py's bound on the dense model) against float64 on every utterance
alone, for the ragged pass and for the dense call on every utterance as its own batch.  Measured maxima (MI355X):
see docs/LAB_NOTEBOOK.md section 29.
"""
import ctypes

import numpy as np
import pytest
import torch

import ragged_mla_cases as rc
from guarded import Guarded
from oracle import update_paths_np as up

pytestmark = pytest.mark.gpu

H_TOL = rc.H_TOL
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


# ---------------------------------------------------------------------------------------------------- kernel level
def _device_case(z, ro, shift):
    Z = Guarded(z.shape, init=torch.from_numpy(np.array(z, np.float32)), shift=shift)
    assert Z.view.data_ptr() % 16 == 4 * shift
    return Z, torch.from_numpy(np.array(ro, np.int64)).cuda()


def run_ragged(Z, ro_dev, B, K, with_colsum=True):
    """the ragged call into the level slice of a wider att buffer; returns (att [B, K], colsum [B, K] or None)"""
    nv = _nv()
    ld, col = 2 * K + 3, K + 1
    A, S = Guarded((B, ld)), Guarded((B, K))
    z_before = Z.numpy().copy()
    nv.check(nv.lib.lidbox_mla_attention_ragged_fwd(Z.ptr, nv.ptr(ro_dev), B, K, _off(A, col), ld, S.ptr if with_colsum else None,
                                                    nv.current_stream()))
    torch.cuda.synchronize()
    a_full, s = A.numpy(), S.numpy()                       # .numpy() checks the guard words
    live = np.zeros((B, ld), bool)
    live[:, col:col + K] = True
    assert (_bits(a_full[~live]) == _bits(NAN32)).all(), "att: a column outside the level's slice was written"
    assert _same(Z.numpy(), z_before), "z was modified"
    if not with_colsum:
        assert (_bits(s) == _bits(NAN32)).all(), "colsum = NULL, yet the buffer beside it was written"
        return a_full[:, col:col + K].copy(), None
    return a_full[:, col:col + K].copy(), s


def run_dense_each(Z, ro, K):
    """lidbox_mla_attention_fwd on every utterance alone: B = 1, T = T_b, z + row_offsets[b] K"""
    nv = _nv()
    B = len(ro) - 1
    att, cs = np.empty((B, K), np.float32), np.empty((B, K), np.float32)
    for b in range(B):
        A, S = Guarded((1, K)), Guarded((1, K))
        zb = ctypes.c_void_p(Z.view.data_ptr() + 4 * int(ro[b]) * K)
        nv.check(nv.lib.lidbox_mla_attention_fwd(zb, 1, int(ro[b + 1] - ro[b]), K, A.ptr, K, S.ptr, nv.current_stream()))
        torch.cuda.synchronize()
        att[b], cs[b] = A.numpy()[0], S.numpy()[0]
    return att, cs


_KERNEL = {}


def _kernel_case(K, shift):
    """inputs, the ragged result and the dense result on every utterance alone, computed once and left unchanged"""
    if (K, shift) not in _KERNEL:
        z, ro = rc.kernel_inputs(K, shift)
        Z, ro_dev = _device_case(z, ro, shift)
        B = len(ro) - 1
        att, cs = run_ragged(Z, ro_dev, B, K)
        d_att, d_cs = run_dense_each(Z, ro, K)
        for a in (z, ro, att, cs, d_att, d_cs):
            a.setflags(write=False)
        _KERNEL[(K, shift)] = (z, ro, Z, ro_dev, att, cs, d_att, d_cs)
    return _KERNEL[(K, shift)]


def test_the_cases_reach_every_instantiation():
    assert {(p["vec"], p["nj"]) for p in (rc.kernel_plan(K, s) for K, s in rc.KERNEL_KS)} == rc.ALL_PAIRS


@pytest.mark.parametrize("K,shift", rc.KERNEL_KS, ids=["k%d%s" % (K, "_zoff" if s else "") for K, s in rc.KERNEL_KS])
def test_every_utterance_gets_the_dense_kernels_bits(K, shift):
    z, ro, Z, ro_dev, att, cs, d_att, d_cs = _kernel_case(K, shift)
    B = len(ro) - 1
    assert np.isfinite(att).all() and np.isfinite(cs).all(), "att or colsum not fully written"
    for b in range(B):
        assert _same(att[b], d_att[b]), "att of utterance %d (T = %d) differs from the dense call on it alone" % (b, ro[b + 1] - ro[b])
        assert _same(cs[b], d_cs[b]), "colsum of utterance %d (T = %d) differs from the dense call on it alone" % (b, ro[b + 1] - ro[b])
    # colsum = NULL: the same att, nothing else written
    att0, none = run_ragged(Z, ro_dev, B, K, with_colsum=False)
    assert none is None and _same(att0, att)


@pytest.mark.parametrize("K,shift", rc.KERNEL_KS, ids=["k%d%s" % (K, "_zoff" if s else "") for K, s in rc.KERNEL_KS])
def test_every_utterance_lies_within_the_float64_bound(K, shift):
    z, ro, Z, ro_dev, att, cs, _, _ = _kernel_case(K, shift)
    worst_a = worst_s = 0.0
    clipped_lo = clipped_hi = False
    for b in range(len(ro) - 1):
        zb = z[ro[b]:ro[b + 1]]
        plan = up.mla_fwd_plan(len(zb), K, up.mla_vec4(K, 4 * shift))
        assert (plan["vec"], plan["nj"]) == (rc.kernel_plan(K, shift)["vec"], rc.kernel_plan(K, shift)["nj"])
        ref = up.mla_fwd_ref(zb[None], plan)
        qa = np.abs(att[b] - ref["att"][0]) / (ref["att_rel"][0] * ref["att"][0])
        qs = np.abs(cs[b] - ref["colsum"][0]) / (ref["colsum_rel"][0] * ref["colsum"][0])
        worst_a, worst_s = max(worst_a, float(qa.max())), max(worst_s, float(qs.max()))
        assert (qa <= 1.0).all() and (qs <= 1.0).all(), (K, b, len(zb), float(qa.max()), float(qs.max()))
        assert np.abs(att[b] - ref["att"][0]).max() <= H_TOL
        z64 = zb.astype(np.float64)
        e = np.exp(z64 - z64.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        clipped_lo |= bool((p < up.LO).any())
        clipped_hi |= bool((p > up.HI).any())
    print("ragged mla K=%d%s <%d,%d>: err/bound att %.3f colsum %.3f" % (K, " z off" if shift else "", plan["vec"], plan["nj"], worst_a, worst_s))
    assert clipped_hi and (clipped_lo or K == 1)                  # K = 1: p = 1 everywhere, clipped from above only


@pytest.mark.parametrize("K,shift", [(100, 0), (127, 0), (5, 0), (128, 1)], ids=["k100", "k127", "k5", "k128_zoff"])
def test_an_utterance_does_not_depend_on_its_neighbours_place_or_run(K, shift):
    z, ro, Z, ro_dev, att, cs, _, _ = _kernel_case(K, shift)
    B = len(ro) - 1
    # run to run
    att2, cs2 = run_ragged(Z, ro_dev, B, K)
    assert _same(att2, att) and _same(cs2, cs)
    # another order: other neighbours, another place, another first row
    perm = np.random.default_rng(3).permutation(B)
    assert not np.array_equal(perm, np.arange(B))
    zp = np.concatenate([z[ro[b]:ro[b + 1]] for b in perm])
    rop = np.concatenate(([0], np.cumsum([ro[b + 1] - ro[b] for b in perm]))).astype(np.int64)
    Zp, rop_dev = _device_case(zp, rop, shift)
    attp, csp = run_ragged(Zp, rop_dev, B, K)
    for i, b in enumerate(perm):
        assert _same(attp[i], att[b]) and _same(csp[i], cs[b]), (i, b)
    # a NaN neighbour
    victim = int(np.argsort(np.diff(ro))[B // 2])
    zn = z.copy()
    zn[ro[victim]:ro[victim + 1]] = NAN32
    Zn, ron_dev = _device_case(zn, ro, shift)
    attn, csn = run_ragged(Zn, ron_dev, B, K)
    assert np.isnan(attn[victim]).all()
    for b in range(B):
        if b != victim:
            assert _same(attn[b], att[b]) and _same(csn[b], cs[b]), b


def test_empty_batch_and_refusals_write_nothing():
    nv = _nv()
    lib, st = nv.lib, nv.current_stream()
    buf = torch.full((64,), 3.0, device="cuda")
    ro = torch.tensor([0, 2, 5], dtype=torch.int64, device="cuda")
    p, o = nv.ptr(buf), nv.ptr(ro)
    assert lib.lidbox_mla_attention_ragged_fwd(p, o, 0, 4, p, 4, p, st) == 0
    assert lib.lidbox_mla_attention_ragged_fwd(p, o, 0, 4, p, 4, None, st) == 0
    for args in ((None, o, 2, 4, p, 4, p), (p, None, 2, 4, p, 4, p), (p, o, 2, 4, None, 4, p), (p, o, -1, 4, p, 4, p),
                 (p, o, 2, 0, p, 4, p), (p, o, 2, -2, p, 4, p), (p, o, 2, 1025, p, 1025, p), (p, o, 2, 4, p, 3, p),
                 (p, o, 2, 4, p, 3, None)):
        assert lib.lidbox_mla_attention_ragged_fwd(*args, st) == -1, args
        assert "lidbox_mla_attention_ragged_fwd" in nv.last_error()
    with pytest.raises(ValueError):
        nv.check(lib.lidbox_mla_attention_ragged_fwd(p, o, 2, 4, p, 3, p, st))
    torch.cuda.synchronize()
    assert (buf == 3.0).all() and ro.tolist() == [0, 2, 5]


# ---------------------------------------------------------------------------------------------------- model level
_MODEL = {}


def model_case(case):
    """(model, utterances, X on the device, offsets, float64 outputs, float64 embeddings); the model is built once"""
    if case not in _MODEL:
        from lidbox_amd.models import multilevel_attention
        c = rc.MODEL_CASES[case]
        w, xs, out, emb = rc.model_reference(case)
        m = multilevel_attention.create((max(rc.MODEL_LENGTHS), c["D"]), c["K"], L=c["L"], H=c["H"], seed=1)
        m.set_weights(w)
        assert all(np.array_equal(v, w[k]) for k, v in m.get_weights().items())
        X = torch.from_numpy(np.concatenate(xs)).cuda()
        off = np.concatenate(([0], np.cumsum([len(x) for x in xs]))).astype(np.int64)
        _MODEL[case] = (m, xs, X, off, out, emb)
    return _MODEL[case]


def _err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max())


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_ragged_pass_matches_float64_on_every_utterance_alone(case):
    m, xs, X, off, out, emb = model_case(case)
    assert m.ragged_refusal() is None
    pred, e = m.predict_ragged(X, off), m.embed_ragged(X, off)
    c = rc.MODEL_CASES[case]
    assert pred.shape == (len(xs), c["K"]) and e.shape == (len(xs), c["L"] * c["K"])
    assert pred.data_ptr() != m.predict_ragged(X, off).data_ptr()                    # fresh tensors, not workspace views
    pred, e = pred.cpu().numpy(), e.cpu().numpy()
    dense = np.stack([m.predict(torch.from_numpy(x).cuda()[None])[0].cpu().numpy() for x in xs])
    dense_e = np.stack([m.embed(torch.from_numpy(x).cuda()[None])[0].cpu().numpy() for x in xs])
    print("multilevel_attention %s: ragged vs float64 %.3e (output) %.3e (embedding); dense alone vs float64 %.3e %.3e; "
          "ragged vs dense alone %.3e %.3e" % (case, _err(pred, out), _err(e, emb), _err(dense, out), _err(dense_e, emb),
                                               _err(pred, dense), _err(e, dense_e)))
    assert np.isfinite(pred).all() and np.isfinite(e).all()
    assert _err(pred, out) <= H_TOL and _err(e, emb) <= H_TOL
    assert _err(dense, out) <= H_TOL and _err(dense_e, emb) <= H_TOL


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_the_zero_padded_batch_is_wrong_for_the_short_utterance(case):
    m, xs, X, off, out, emb = model_case(case)
    T = max(rc.MODEL_LENGTHS)
    batch = torch.from_numpy(np.stack([rc.zero_padded(x, T) for x in xs])).cuda()
    padded = m.predict(batch).cpu().numpy()
    short, long_ = int(np.argmin(rc.MODEL_LENGTHS)), int(np.argmax(rc.MODEL_LENGTHS))
    print("multilevel_attention %s: padded batch vs float64: %.3e for T = 1, %.3e for T = %d"
          % (case, _err(padded[short], out[short]), _err(padded[long_], out[long_]), T))
    assert _err(padded[short], out[short]) > H_TOL
    assert _err(padded[long_], out[long_]) <= H_TOL


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_duplicates_nan_neighbours_and_workspace_reuse(case):
    m, xs, X, off, out, emb = model_case(case)
    B, c = len(xs), rc.MODEL_CASES[case]
    # the batch twice over: both copies of an utterance get the same bits
    X2 = torch.cat([X, X])
    off2 = np.concatenate((off, off[1:] + off[-1]))
    big = m.predict_ragged(X2, off2).cpu().numpy()
    big_e = m.embed_ragged(X2, off2).cpu().numpy()
    assert _same(big[:B], big[B:]) and _same(big_e[:B], big_e[B:])
    ws, caps = m._rws, (m._rws.cap_rows, m._rws.cap_B)
    # a smaller pass on the front of the buffers the larger one left full, then poisoned
    small = m.predict_ragged(X[:off[3]], off[:4]).cpu().numpy()
    assert _err(small, out[:3]) <= H_TOL
    for t in (ws.a, ws.y, ws.z, ws.att, ws.h, ws.logp):
        t.fill_(float("nan"))
    assert _same(m.predict_ragged(X[:off[3]], off[:4]).cpu().numpy(), small)
    assert _same(m.predict_ragged(X2, off2).cpu().numpy(), big) and _same(m.embed_ragged(X2, off2).cpu().numpy(), big_e)
    assert m._rws is ws and (ws.cap_rows, ws.cap_B) == caps
    # NaN frames in one utterance change no bit of any other (its own output need not be NaN: relu(NaN) is 0)
    victim = 4
    Xn = X2.clone()
    Xn[off[victim]:off[victim + 1]] = float("nan")
    nan_out = m.predict_ragged(Xn, off2).cpu().numpy()
    keep = [b for b in range(2 * B) if b != victim]
    assert _same(nan_out[keep], big[keep])
    # nothing to do
    assert m.predict_ragged(X[:0], [0]).shape == (0, c["K"]) and m.embed_ragged(X[:0], [0]).shape == (0, c["L"] * c["K"])


def test_pipeline_entry_points_accept_the_model():
    from lidbox_amd import util
    from lidbox_amd.data import steps
    from lidbox_amd.models.multilevel_attention import as_embedding_extractor
    assert set(steps.VALID_STEP_FUNCTIONS) >= {"extract_embeddings"}
    for case in sorted(rc.MODEL_CASES):
        m, xs, X, off, out, emb = model_case(case)
        D = emb.shape[1]
        ds = [dict(id="u%d" % i, input=torch.from_numpy(x).cuda() if i % 2 else x) for i, x in enumerate(xs)]
        one = list(steps.extract_embeddings(ds, {"extractors": [as_embedding_extractor(m), m], "batch_size": 1}))
        one = np.stack([x["embedding"].cpu().numpy() for x in one])
        assert _err(one[:, :D], emb) <= H_TOL
        for bs in (4, 256):
            rag = list(steps.extract_embeddings(ds, {"extractors": [as_embedding_extractor(m), m], "batch_size": bs, "ragged": True}))
            assert [x["id"] for x in rag] == ["u%d" % i for i in range(len(xs))]
            got = np.stack([x["embedding"].cpu().numpy() for x in rag])
            assert got.shape == (len(xs), 2 * D) and _same(got[:, :D], got[:, D:]), (case, bs)
            assert _err(got, one) <= H_TOL and _err(got[:, :D], emb) <= H_TOL, (case, bs)
        elements = [dict(id="utt-%02d" % (len(xs) - i), input=torch.from_numpy(x).cuda()) for i, x in enumerate(xs)]
        dense = util.predict_with_model(m, [dict(id=[e["id"]], input=e["input"][None]) for e in elements])
        for lb in (256, 3):
            rag = util.predict_ragged_with_model(m, iter(elements), launch_batch=lb)
            assert list(rag.index) == list(dense.index) and list(rag.columns) == list(dense.columns)
            a, b = np.stack(rag.prediction.values), np.stack(dense.prediction.values)
            assert a.shape == b.shape and _err(a, b) <= H_TOL, (case, lb)
        assert _err(np.stack(rag.loc[[e["id"] for e in elements]].prediction.values), out) <= H_TOL


def test_model_refusals():
    m, xs, X, off, _, _ = model_case("k5")
    with pytest.raises(ValueError, match="length 0"):
        m.predict_ragged(X, [0, 3, 3, len(X)])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, off[:-1])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, [1, len(X)])
    with pytest.raises(ValueError, match=r"\[total_T, 8\]"):
        m.predict_ragged(torch.zeros((5, 9), device="cuda"), [0, 5])
    with pytest.raises(ValueError, match="contiguous"):
        m.embed_ragged(torch.zeros((5, 16), device="cuda")[:, :8], [0, 5])
    with pytest.raises(Exception):
        m.predict_ragged(X.cpu(), off)


def test_a_ragged_call_leaves_training_untouched():
    """a training-mode forward and backward gives the bits it gave before the ragged calls; parameters and moving statistics
    are what they were"""
    m, xs, X, off, _, _ = model_case("k5")
    rng = np.random.default_rng(12)
    B, T = 3, 7
    x = torch.from_numpy(rng.standard_normal((B, T, m.input_dim)).astype(np.float32)).cuda()
    G = torch.from_numpy(rng.standard_normal((B, m.output_dim)).astype(np.float32)).cuda()

    def train_pass():
        ws = m.workspace(B, T)
        m._load_input(ws, x, False)
        out = m.forward_ws(ws, training=True, update_moving=False).clone()
        ws.dh[-1].copy_(G)
        m.backward_ws(ws)
        torch.cuda.synchronize()
        return out.cpu().numpy(), ws.att.cpu().numpy().copy(), m.flat_grad.cpu().numpy().copy()

    assert m.dropout_rate > 0
    flat, state = m.flat.cpu().numpy().copy(), m.state.cpu().numpy().copy()
    before = train_pass()
    m.predict_ragged(X, off)
    m.embed_ragged(X, off)
    after = train_pass()
    assert all(_same(a, b) for a, b in zip(before, after))
    assert np.abs(before[2]).max() > 0
    assert _same(m.flat.cpu().numpy(), flat) and _same(m.state.cpu().numpy(), state)
