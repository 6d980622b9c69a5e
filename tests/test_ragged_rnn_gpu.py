"""
The ragged recurrent pass on the device: the ragged walks of csrc/lstm_step.hip and gru.hip (the dense forward step kernels over
rnn_step.h's RaggedRows) and the ragged pool of rnn.hip through the C ABI, then forward_ragged / predict_ragged / embed_ragged of lstm, ap_lstm, bi_gru and spherespeaker, steps.extract_embeddings(ragged: true) and util.predict_ragged_with_model.

Kernel level.  Every buffer a call may write is a tests/guarded.py payload: NaN around it, NaN wherever the kernel must write (the
frame rows of hseq's slice, of cseq / qh, all of hlast), zero on the pad rows of hseq's slice, recognisable finite values on the
pad rows of zg, cseq and qh, NaN in the columns of a wide hseq outside the layer's slice.  How results are judged:
    1. bit for bit against lidbox_lstm_step_fwd / lidbox_gru_fwd, called once per distinct length on the utterances of that
       length with the same projections (their header promises rows independent of the batch): gates, c / qh, h, hlast;
    2. for one LSTM and one GRU case every utterance alone against oracle/rnn_paths_np.py's float64 one-step references within
       that module's own bounds, and h within its H_TOL of the whole-layer oracle, as tests/test_rnn_paths_gpu.py judges the
       dense kernels;
    3. pad rows and guards as they were;
    4. an utterance in two different batches (other neighbours, place and slot): the same bits;
    5. a second, smaller call into the buffers the first left full: the bits of a fresh call.
The length set (test_ragged_rnn_cpu.kernel_lengths) gives n_s = 70, 67, 65, 5, 5, 1, 1, 1, 1: the 64-slot tile boundary is crossed
with second tiles of 6, 3 and 1 slots, an utterance ends at every kind of step, T = 1 utterances are first and last step at once.

Model level.  Small widths, C = 8, lengths 1 .. 11, BatchNormalization state and gamma / beta random: every utterance of the ragged
pass against the model's own dense call on it alone and against the float64 torch restatements of test_rnn_gpu.py,
test_gru_gpu.py and test_spherespeaker_gpu.py, at those files' H_TOL (5e-5).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_gru_gpu as dense_gru
import test_rnn_gpu as dense_rnn
import test_spherespeaker_gpu as dense_sphere
from guarded import Guarded
from lidbox_amd.models.ragged import recurrent_plan
from lidbox_amd.testutil import device_copy
from oracle import rnn_paths_np as rp
from test_ragged_rnn_cpu import kernel_lengths

pytestmark = pytest.mark.gpu

H_TOL = dense_rnn.H_TOL
assert H_TOL == dense_gru.H_TOL == dense_sphere.H_TOL == rp.H_TOL == 5e-5
ZG_PAD, AUX_PAD = -3.25, 5.5                          # what the pad rows of zg and cseq / qh hold going in


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- data
MAIN = tuple(enumerate(kernel_lengths()))             # (utterance id, length) in the caller's order
# nine of them in MAIN's order: the 9, two 5s, two 1s, a 2 and three 3s
SUB9 = tuple(sorted([u for u in MAIN if u[1] == 9] + [u for u in MAIN if u[1] == 5][:2] + [u for u in MAIN if u[1] == 1][:2] +
                    [u for u in MAIN if u[1] == 2][:1] + [u for u in MAIN if u[1] == 3][:3]))
OTHER = tuple(reversed(MAIN))[4:40] + ((900, 4), (901, 1))       # MAIN's utterances in other company, places and slots


def _weights(fam, H, dirs):
    d = rp.draw(fam, H, dirs, 1, 1, "normal")
    return d["U"], d["brec"]


def _zg_in(fam, H, dirs, uid, T):
    """the projections of utterance uid: a function of (family, H, uid, T) only"""
    ng = 3 if fam == "gru" else 4
    return np.random.default_rng([ng, H, T, uid, 216]).standard_normal((2, T, ng * H)).astype(np.float32)[:dirs]


# ---------------------------------------------------------------------------------------------------- the dense yardstick
@functools.lru_cache(maxsize=None)
def dense_results(fam, H, dirs, utts, rs, col):
    """{uid: dict(gates [dirs, T, NG H], aux [dirs, T, H], h [T, dirs H], hlast [dirs H])} from the dense entry points, one
    call per distinct length"""
    nv = _nv()
    lib, st_ = nv.lib, nv.current_stream()
    gru = fam == "gru"
    D = dirs * H
    Uh, bh = _weights(fam, H, dirs)
    U = [device_copy(u) for u in Uh]
    brec = [device_copy(b) for b in bh]
    U1 = nv.ptr(U[1]) if dirs == 2 else None
    out = {}
    for T in sorted({t for _, t in utts}):
        ids = [u for u, t in utts if t == T]
        B = len(ids)
        zg = Guarded((dirs, B, T, (3 if gru else 4) * H), init=torch.from_numpy(np.stack([_zg_in(fam, H, dirs, u, T) for u in ids], 1)))
        hseq = Guarded((B, T + 2, rs))
        hseq.view[:, 0, col:col + D] = 0.0
        hseq.view[:, T + 1, col:col + D] = 0.0
        hp = ctypes.c_void_p(hseq.view.data_ptr() + 4 * col)
        aux = Guarded((dirs, B, T, H))
        if gru:
            hl = Guarded((B, D))
            nv.check(lib.lidbox_gru_fwd(nv.ptr(U[0]), U1, nv.ptr(brec[0]), nv.ptr(brec[1]) if dirs == 2 else None, dirs, B, T, H,
                                        zg.ptr, hp, aux.ptr, hl.ptr, st_))
        else:
            nv.check(lib.lidbox_lstm_step_fwd(nv.ptr(U[0]), U1, dirs, B, T, H, zg.ptr, hp, rs, aux.ptr, None, 0, st_))
        torch.cuda.synchronize()
        g, a, h = zg.numpy(), aux.numpy(), hseq.numpy()[:, 1:T + 1, col:col + D]
        for k, u in enumerate(ids):
            last = np.concatenate([h[k, T - 1 if d == 0 else 0, d * H:(d + 1) * H] for d in range(dirs)])
            if gru:
                assert _same(hl.numpy()[k], last)
            out[u] = dict(gates=g[:, k].copy(), aux=a[:, k].copy(), h=h[k].copy(), hlast=last)
    return out


# ---------------------------------------------------------------------------------------------------- the ragged call
class Buffers:
    """the guarded buffers of one layer at `rows` rows and B utterances"""

    def __init__(self, fam, H, dirs, rows, B, rs, shift=0):
        ng = 3 if fam == "gru" else 4
        self.zg, self.hseq = Guarded((dirs, rows, ng * H)), Guarded((rows, rs), shift=shift)
        self.aux, self.hlast = Guarded((dirs, rows, H)), Guarded((B, dirs * H))


def run_ragged(fam, H, dirs, utts, rs=None, col=0, hlast=True, reuse=None, shift=0):
    """one layer over the utterances `utts` ((uid, length), ..) through the C ABI.  reuse: the Buffers of an earlier, larger call,
    used as that call left them except for what the caller of the entry point owes: the projections and zero pad rows of hseq.
    shift: words hseq is moved past a 16-byte aligned address.
    Returns ({uid: results as dense_results}, the Buffers)."""
    nv = _nv()
    lib, st_ = nv.lib, nv.current_stream()
    gru = fam == "gru"
    ng = 3 if gru else 4
    D = dirs * H
    rs = D if rs is None else rs
    lengths = [t for _, t in utts]
    plan = recurrent_plan(lengths)
    B, Rp, seg = plan.B, plan.Rp, plan.seg
    pads = np.concatenate([seg[:-1], seg[1:] - 1])
    frames = np.ones(Rp, bool)
    frames[pads] = False
    Uh, bh = _weights(fam, H, dirs)
    U = [device_copy(u) for u in Uh]
    brec = [device_copy(b) for b in bh]
    bufs = reuse or Buffers(fam, H, dirs, Rp, B, rs, shift)
    rows = bufs.zg.view.shape[1]
    assert rows >= Rp and bufs.hlast.view.shape[0] >= B
    zin = np.full((dirs, Rp, ng * H), ZG_PAD, np.float32)
    for (u, T), s in zip(utts, seg):
        zin[:, s + 1:s + 1 + T] = _zg_in(fam, H, dirs, u, T)
    ft, pt = torch.from_numpy(np.flatnonzero(frames)).cuda(), torch.from_numpy(pads).cuda()
    if reuse is None:
        bufs.zg.view.copy_(torch.from_numpy(zin))
        bufs.aux.view[:, pt] = AUX_PAD
    else:
        bufs.zg.view[:, ft] = torch.from_numpy(zin[:, frames]).cuda()
    bufs.hseq.view[pt, col:col + D] = 0.0
    before = dict(zg=bufs.zg.numpy().copy(), aux=bufs.aux.numpy().copy(), hseq=bufs.hseq.numpy().copy(), hlast=bufs.hlast.numpy().copy())
    slots = device_copy(plan.slots())
    assert slots.dtype == torch.int64
    U1 = nv.ptr(U[1]) if dirs == 2 else None
    hp = ctypes.c_void_p(bufs.hseq.view.data_ptr() + 4 * col)
    hl = bufs.hlast.ptr if hlast else None
    sl = ctypes.c_void_p(plan.sorted_lengths.ctypes.data)
    if gru:
        assert rs == D and col == 0
        nv.check(lib.lidbox_gru_ragged_fwd(nv.ptr(U[0]), U1, nv.ptr(brec[0]), nv.ptr(brec[1]) if dirs == 2 else None, dirs, B, H,
                                           rows, nv.ptr(slots), sl, bufs.zg.ptr, hp, bufs.aux.ptr, hl, st_))
    else:
        nv.check(lib.lidbox_lstm_ragged_fwd(nv.ptr(U[0]), U1, dirs, B, H, rows, nv.ptr(slots), sl, bufs.zg.ptr, hp, rs, bufs.aux.ptr,
                                            hl, st_))
    torch.cuda.synchronize()
    g, a, h, l = bufs.zg.numpy(), bufs.aux.numpy(), bufs.hseq.numpy(), bufs.hlast.numpy()      # .numpy() checks the guards
    # 3. what the walk must not touch: pad rows, rows behind Rp, the columns outside the slice, hlast when it is not asked for
    keep = np.ones(rows, bool)
    keep[:Rp] = ~frames
    assert _same(g[:, keep], before["zg"][:, keep]), "zg: a pad row or a row behind the batch was written"
    assert _same(a[:, keep], before["aux"][:, keep]), "cseq / qh: a pad row or a row behind the batch was written"
    assert _same(h[keep], before["hseq"][keep]) and not h[pads, col:col + D].any(), "hseq: a pad row was written"
    other = np.ones(rs, bool)
    other[col:col + D] = False
    assert _same(h[:, other], before["hseq"][:, other]), "hseq: columns outside the layer's slice were written"
    assert _same(l[B:], before["hlast"][B:])
    if not hlast:
        assert _same(l, before["hlast"]), "hlast was written though NULL was passed"
    for name, v in (("gates", g[:, :Rp][:, frames]), ("c / qh", a[:, :Rp][:, frames]), ("h", h[:Rp][frames][:, col:col + D])):
        assert np.isfinite(v).all(), "%s: %d elements of frame rows not written" % (name, (~np.isfinite(v)).sum())
    if hlast:
        assert np.isfinite(l[:B]).all(), "hlast: rows not written"
    out = {}
    for b, ((u, T), s) in enumerate(zip(utts, seg)):
        f = slice(s + 1, s + 1 + T)
        out[u] = dict(gates=g[:, f].copy(), aux=a[:, f].copy(), h=h[f, col:col + D].copy(), hlast=l[b].copy() if hlast else None)
    return out, bufs


def _equal_utterance(got, want, what, hlast=True):
    for key in ("gates", "aux", "h") + (("hlast",) if hlast else ()):
        assert _same(got[key], want[key]), "%s: %s differs" % (what, key)


# family, H, dirs, utterances, h_row_stride (None: dirs H), column
CASES = [("step", 250, 2, MAIN, 1500, 500),        # the model's width: float2 path, last unit slice partial, a slice of a wide buffer
         ("step", 16, 1, MAIN, None, 0),           # float4 path
         ("step", 5, 2, MAIN, None, 0),            # scalar path, lanes past H
         ("step", 264, 2, SUB9, None, 0),          # a second K chunk of 8 -> kpad 32
         ("gru", 32, 2, MAIN, None, 0),            # float4 path
         ("gru", 7, 2, MAIN, None, 0),             # scalar path
         ("gru", 264, 2, SUB9, None, 0),           # second K chunk
         ("step", 16, 2, ((0, 1),), None, 0),      # B = 1, T = 1
         ("gru", 7, 1, ((0, 1),), None, 0),
         ("step", 5, 2, tuple((u, 3) for u in range(64)), None, 0),      # all lengths equal: the dense walk
         ("gru", 32, 2, tuple((u, 3) for u in range(64)), None, 0)]
IDS = ["%s-H%d-d%d-B%d" % (c[0], c[1], c[2], len(c[3])) for c in CASES]


@functools.lru_cache(maxsize=None)
def ragged_results(i):
    fam, H, dirs, utts, rs, col = CASES[i]
    return run_ragged(fam, H, dirs, utts, rs, col)[0]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_utterance_gets_the_bits_of_the_dense_kernels(i):
    fam, H, dirs, utts, rs, col = CASES[i]
    got = ragged_results(i)
    want = dense_results(fam, H, dirs, utts, dirs * H if rs is None else rs, col)
    assert sorted(got) == sorted(want) == sorted(u for u, _ in utts)
    for u, T in utts:
        _equal_utterance(got[u], want[u], "%s H=%d utterance %d (T=%d)" % (fam, H, u, T))


@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_every_utterance_alone_lies_within_the_float64_oracles_bounds(i):
    fam, H, dirs, utts, rs, col = CASES[i]
    got = ragged_results(i)
    Uh, bh = _weights(fam, H, dirs)
    worst = {}
    for u, T in utts:
        r = rp._row("u%d" % u, fam, H, dirs=dirs, B=1, T=T)
        zin = _zg_in(fam, H, dirs, u, T)[:, None]
        hs = np.zeros((1, T + 2, dirs * H), np.float32)
        hs[0, 1:T + 1] = got[u]["h"]
        st = dict(gates=got[u]["gates"][:, None], hs=hs)
        st["qh" if fam == "gru" else "c"] = got[u]["aux"][:, None]
        dat = dict(U=Uh, brec=bh, zg=zin)
        for name, val, ref in rp.fwd_checks(r, dat, st):
            q = rp.ratio(val, ref)
            worst[name] = max(worst.get(name, 0.0), float(q.max()))
            assert (q <= 1.0).all(), "%s utterance %d (T=%d) %s: worst %.3g x the bound" % (fam, u, T, name, q.max())
        whole = rp.gru_layer(Uh, bh, zin)[2] if fam == "gru" else rp.lstm_layer(Uh, zin)[2]
        assert np.abs(rp.h_of(hs, dirs, H) - whole).max() <= rp.H_TOL
    print("%s H=%d: largest err / bound %s" % (fam, H, {k: "%.3f" % v for k, v in worst.items()}))


@pytest.mark.parametrize("fam,H", [("step", 250), ("step", 16), ("gru", 32), ("gru", 7)])
def test_an_utterance_gets_the_same_bits_in_another_batch(fam, H):
    i = next(k for k, c in enumerate(CASES) if c[:2] == (fam, H) and c[3] is MAIN)
    _, _, dirs, _, rs, col = CASES[i]
    a = ragged_results(i)
    b, _ = run_ragged(fam, H, dirs, OTHER, rs, col)
    common = [u for u, _ in OTHER if u in a]
    assert len(common) == 36
    pa, pb = recurrent_plan([t for _, t in MAIN]), recurrent_plan([t for _, t in OTHER])
    place = lambda utts, plan, u: (k := [x for x, _ in utts].index(u), int(np.flatnonzero(plan.order == k)[0]))
    assert any(place(MAIN, pa, u)[1] // 64 != place(OTHER, pb, u)[1] // 64 for u in common)        # another row tile, too
    for u in common:
        assert place(MAIN, pa, u) != place(OTHER, pb, u)
        _equal_utterance(b[u], a[u], "%s H=%d utterance %d in another batch" % (fam, H, u))


@pytest.mark.parametrize("fam,H,dirs", [("step", 250, 2), ("gru", 32, 2)])
def test_a_smaller_call_into_used_buffers_gives_the_bits_of_a_fresh_call(fam, H, dirs):
    _, bufs = run_ragged(fam, H, dirs, MAIN)
    again, _ = run_ragged(fam, H, dirs, SUB9, reuse=bufs)
    fresh, _ = run_ragged(fam, H, dirs, SUB9)
    for u, T in SUB9:
        _equal_utterance(again[u], fresh[u], "%s H=%d utterance %d in used buffers" % (fam, H, u))


def test_gru_without_hlast_computes_the_same():
    i = next(k for k, c in enumerate(CASES) if c[:2] == ("gru", 32) and c[3] is MAIN)
    a = ragged_results(i)
    b, _ = run_ragged("gru", 32, 2, MAIN, hlast=False)
    for u, _ in MAIN:
        _equal_utterance(b[u], a[u], "utterance %d without hlast" % u, hlast=False)


def test_load_paths_agree_bit_for_bit():
    """LSTM, H = 16 at three alignments of hseq: a 16-byte aligned slice (float4), one 8 bytes off (float2), one 4 bytes off
    (scalar).  GRU, H = 32: every buffer aligned (float4) and hseq 4 bytes off (scalar)."""
    runs = [run_ragged("step", 16, 2, SUB9, rs=40, col=col)[0] for col in (0, 2, 1)]
    for u, _ in SUB9:
        _equal_utterance(runs[1][u], runs[0][u], "float2 against float4, utterance %d" % u)
        _equal_utterance(runs[2][u], runs[0][u], "scalar against float4, utterance %d" % u)
    vec, _ = run_ragged("gru", 32, 2, SUB9)
    scalar, bufs = run_ragged("gru", 32, 2, SUB9, shift=1)
    assert bufs.hseq.view.data_ptr() % 16 == 4
    for u, _ in SUB9:
        _equal_utterance(scalar[u], vec[u], "GRU scalar against float4, utterance %d" % u)


def test_an_empty_batch_touches_nothing_and_bad_arguments_are_refused():
    nv = _nv()
    lib, st_ = nv.lib, nv.current_stream()
    H = 16
    U = device_copy(np.ones((H, 4 * H), np.float32))
    b = device_copy(np.ones(3 * H, np.float32))
    bufs = [Guarded((64,)) for _ in range(5)]
    z, h, c, l, o = (g.ptr for g in bufs)
    for dirs in (1, 2):
        U1 = nv.ptr(U) if dirs == 2 else None
        assert lib.lidbox_lstm_ragged_fwd(nv.ptr(U), U1, dirs, 0, H, 0, None, None, z, h, dirs * H, c, l, st_) == 0
        assert lib.lidbox_gru_ragged_fwd(nv.ptr(U), U1, nv.ptr(b), nv.ptr(b) if dirs == 2 else None, dirs, 0, H, 0, None, None, z, h,
                                         c, l, st_) == 0
    assert lib.lidbox_seq_avg_pool_ragged_fwd(z, H, z, z, 0, H, 1.0, o, H, st_) == 0
    # refused before anything is launched: lengths that rise, an empty utterance, too few rows, a narrow row stride, no table
    slots = device_copy(recurrent_plan([2, 3]).slots())
    up, zero, ok = (np.array(v, np.int64) for v in ([2, 3], [3, 0], [3, 2]))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    call = lambda sl, rows, rs, tab: lib.lidbox_lstm_ragged_fwd(nv.ptr(U), None, 1, 2, H, rows, tab, sl, z, h, rs, c, l, st_)
    for args, word in (((p(up), 9, H, nv.ptr(slots)), "non-increasing"), ((p(zero), 9, H, nv.ptr(slots)), "non-increasing"),
                       ((p(ok), 8, H, nv.ptr(slots)), "rows >="), ((p(ok), 9, H - 1, nv.ptr(slots)), "h_row_stride"),
                       ((p(ok), 9, H, None), "slots"), ((None, 9, H, nv.ptr(slots)), "sorted_lengths")):
        assert call(*args) == -1 and "lidbox_lstm_ragged_fwd" in nv.last_error() and word in nv.last_error(), nv.last_error()
    assert lib.lidbox_gru_ragged_fwd(nv.ptr(U), None, None, None, 1, 2, H, 9, nv.ptr(slots), p(ok), z, h, c, l, st_) == -1
    assert lib.lidbox_lstm_ragged_fwd(nv.ptr(U), None, 2, 2, H, 9, nv.ptr(slots), p(ok), z, h, 2 * H, c, l, st_) == -1      # no U1
    torch.cuda.synchronize()
    for g in bufs:
        assert np.isnan(g.numpy()).all()


def test_seq_avg_pool_ragged_scales_and_lands_in_its_columns():
    """out[b, c] = alpha * mean over the utterance's own rows, in a pitched output; against float64 within the rounding of the
    fixed order: ceil(T / 16) additions per time group, 16 to combine, the division and the scale"""
    nv = _nv()
    utts = MAIN + ((500, 40),)
    lengths = np.array([t for _, t in utts], np.int64)
    plan = recurrent_plan(lengths)
    C, rs, ldo, alpha = 10, 13, 27, 0.7
    x = np.random.default_rng(5).standard_normal((plan.Rp, rs)).astype(np.float32)
    xg = Guarded(x.shape, init=torch.from_numpy(x))
    og = Guarded((len(utts), ldo))
    first = device_copy(plan.seg[:-1] + 1)
    nv.check(nv.lib.lidbox_seq_avg_pool_ragged_fwd(ctypes.c_void_p(xg.view.data_ptr() + 4 * 2), rs, nv.ptr(first),
                                                   nv.ptr(device_copy(lengths)), len(utts), C, alpha,
                                                   ctypes.c_void_p(og.view.data_ptr() + 4 * 5), ldo, nv.current_stream()))
    torch.cuda.synchronize()
    o = og.numpy()
    assert np.isnan(o[:, :5]).all() and np.isnan(o[:, 15:]).all(), "columns outside the layer's share were written"
    for b, (s, T) in enumerate(zip(plan.seg, lengths)):
        rows = x[s + 1:s + 1 + T, 2:2 + C].astype(np.float64)
        ref = alpha * rows.mean(0)
        n = -(-int(T) // 16) + 16 + 2
        bound = n * 2.0 ** -24 * alpha * np.abs(rows).sum(0) / T + 2.0 ** -149
        assert (np.abs(o[b, 5:15] - ref) <= bound).all(), (b, T)
    assert _same(xg.numpy(), x)


# ---------------------------------------------------------------------------------------------------- whole models
LENGTHS = [1, 4, 4, 7, 2, 11, 3, 1, 6]
C_IN, N_OUT = 8, 5


def _inputs(seed):
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((T, C_IN)).astype(np.float32) for T in LENGTHS]
    off = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)
    return xs, torch.from_numpy(np.concatenate(xs)).cuda(), off


def _logsm(z):
    return torch.log_softmax(z.detach(), 1).numpy()


@functools.lru_cache(maxsize=None)
def model_case(name):
    """(model, xs, X, offsets, per-utterance float64 reference of the output, of the embedding)"""
    from lidbox_amd.models import ap_lstm, bi_gru, lstm, spherespeaker
    rng = np.random.default_rng(len(name))
    xs, X, off = _inputs(11)
    if name == "lstm":
        m = lstm.create((None, C_IN), N_OUT, num_units=24, seed=3)
        _, fwd = dense_rnn._torch_model(m, m.get_weights())
        out = [_logsm(fwd(x[None]))[0] for x in xs]
        emb = None
    elif name == "ap_lstm":
        m = ap_lstm.create((None, C_IN), num_lstm_units=12, alpha1=0.7, alpha2=1.3, seed=4)
        _, fwd = dense_rnn._torch_model(m, m.get_weights())
        out = [torch.nn.functional.normalize(fwd(x[None]).detach(), dim=1).numpy()[0] for x in xs]
        emb = out
    elif name == "bi_gru":
        m = bi_gru.create((None, C_IN), N_OUT, seed=5, num_units=24, num_fc_units=32)
        dense_gru._randomise_state(m, rng)
        _, fwd = dense_gru._torch_model(m, m.get_weights())
        res = [fwd(x[None], False) for x in xs]
        out, emb = [_logsm(r[0])[0] for r in res], [r[1].detach().numpy()[0] for r in res]
    else:
        m = spherespeaker.create((None, C_IN), N_OUT, embedding_dim=32, seed=6, num_lstm_units=10)
        dense_sphere._randomise_state(m, rng)
        _, fwd = dense_sphere._torch_model(m.get_weights())
        res = [fwd(x[None], False) for x in xs]
        out, emb = [_logsm(r[0])[0] for r in res], [r[1].detach().numpy()[0] for r in res]
    return m, xs, X, off, np.stack(out), None if emb is None else np.stack(emb)


def _dense_embed(name, m, x):
    if name == "lstm":
        ws = m.workspace(1, x.shape[1])
        m._load_input(ws, x, False)
        m.forward_ws(ws)
        return ws.hseq[-1][:, x.shape[1]].clone()             # the final h: the output layer's input
    return m(x) if name == "ap_lstm" else m.embed(x)


@pytest.mark.parametrize("name", ["lstm", "ap_lstm", "bi_gru", "spherespeaker"])
def test_ragged_pass_gives_every_utterance_what_it_gets_alone(name):
    m, xs, X, off, out_ref, emb_ref = model_case(name)
    w0 = m.get_weights()
    got = m.predict_ragged(X, off).cpu().numpy()
    emb = m.embed_ragged(X, off).cpu().numpy()
    assert got.shape == out_ref.shape and np.isfinite(got).all() and np.isfinite(emb).all()
    e_ref = float(np.abs(got - out_ref).max())
    alone = np.stack([m(torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    alone_emb = np.stack([_dense_embed(name, m, torch.from_numpy(x[None]).cuda()).cpu().numpy()[0] for x in xs])
    e_alone, e_emb = float(np.abs(got - alone).max()), float(np.abs(emb - alone_emb).max())
    print("%s: |ragged - float64| = %.3e, |ragged - dense alone| = %.3e, embedding %.3e" % (name, e_ref, e_alone, e_emb))
    assert e_ref <= H_TOL and e_alone <= H_TOL and e_emb <= H_TOL
    assert emb.shape == alone_emb.shape == (len(xs), m._ragged_embedding_dim())
    if emb_ref is not None:
        assert np.abs(emb - emb_ref).max() <= H_TOL
    w1 = m.get_weights()
    assert all(np.array_equal(w0[n], w1[n]) for n in w0)                  # inference leaves weights and statistics alone
    # the workspace is sized by capacity: a later, smaller call uses its front and gives the same answers
    sub = m.predict_ragged(X[:int(off[4])], off[:5]).cpu().numpy()
    assert np.abs(sub - got[:4]).max() <= H_TOL and m._rws.cap_B == len(xs)
    one = m.predict_ragged(torch.from_numpy(xs[5]).cuda(), [0, 11]).cpu().numpy()
    assert np.abs(one[0] - got[5]).max() <= H_TOL
    view = m.forward_ragged(X, off)
    assert view.data_ptr() != m.predict_ragged(X, off).data_ptr()          # predict_ragged returns a fresh tensor
    assert tuple(m.predict_ragged(X[:0], [0]).shape) == (0, got.shape[1])


def test_a_zero_padded_dense_batch_is_a_different_computation():
    """what the feature is for: the dense call on the batch zero-padded to T = 11 misses the tolerance on the short utterances
    of bi_gru (its reverse direction starts inside the padding, its final forward state is the state after the padding), while
    the ragged pass meets it on all of them"""
    m, xs, X, off, out_ref, _ = model_case("bi_gru")
    padded = np.zeros((len(xs), max(LENGTHS), C_IN), np.float32)
    for b, x in enumerate(xs):
        padded[b, :len(x)] = x
    dense = m(torch.from_numpy(padded).cuda()).cpu().numpy()
    err = np.abs(dense - out_ref).max(1)
    rag = np.abs(m.predict_ragged(X, off).cpu().numpy() - out_ref).max(1)
    print("bi_gru, per utterance: padded dense batch %s\n                        ragged %s" % (err, rag))
    for b, T in enumerate(LENGTHS):
        assert rag[b] <= H_TOL
        assert (err[b] > H_TOL) == (T < max(LENGTHS)), (b, T, err[b])


def test_pipeline_entry_points_run_the_recurrent_models():
    from lidbox_amd import util
    from lidbox_amd.data import steps
    from lidbox_amd.models import bi_gru, spherespeaker
    for name, mod in (("bi_gru", bi_gru), ("spherespeaker", spherespeaker)):
        m, xs, X, off, out_ref, emb_ref = model_case(name)
        ex = mod.as_embedding_extractor(m)
        ds = [dict(id="u%d" % i, input=torch.from_numpy(x).cuda() if i % 2 else x) for i, x in enumerate(xs)]
        one = list(steps.extract_embeddings(ds, {"extractors": [ex], "batch_size": 1}))
        for bs in (4, 256):
            rag = list(steps.extract_embeddings(ds, {"extractors": [ex], "batch_size": bs, "ragged": True}))
            assert [x["id"] for x in rag] == [x["id"] for x in one] == ["u%d" % i for i in range(len(xs))]
            for i, (a, b) in enumerate(zip(rag, one)):
                a, b = a["embedding"].cpu().numpy(), b["embedding"].cpu().numpy()
                assert a.shape == b.shape == emb_ref[i].shape
                assert np.abs(a - b).max() <= H_TOL and np.abs(a - emb_ref[i]).max() <= H_TOL, (name, i)
        elements = [dict(id="utt-%02d" % (len(xs) - i), input=torch.from_numpy(x).cuda()) for i, x in enumerate(xs)]
        dense = util.predict_with_model(m, [dict(id=[e["id"]], input=e["input"][None]) for e in elements])
        for lb in (256, 3):
            rag = util.predict_ragged_with_model(m, iter(elements), launch_batch=lb)
            assert list(rag.index) == list(dense.index) and list(rag.columns) == list(dense.columns)
            a, b = np.stack(rag.prediction.values), np.stack(dense.prediction.values)
            assert a.shape == b.shape and np.abs(a - b).max() <= H_TOL, name
        assert np.abs(np.stack(rag.loc[[e["id"] for e in elements]].prediction.values) - out_ref).max() <= H_TOL


@pytest.mark.parametrize("name", ["lstm", "bi_gru", "spherespeaker"])
def test_refusals(name):
    m, xs, X, off, _, _ = model_case(name)
    assert m.ragged_refusal() is None
    with pytest.raises(ValueError, match="length 0"):
        m.predict_ragged(X, [0, 3, 3, len(X)])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, off[:-1])
    with pytest.raises(ValueError, match="row_offsets"):
        m.predict_ragged(X, [1, len(X)])
    with pytest.raises(ValueError, match=r"\[total_T, 8\]"):
        m.predict_ragged(torch.zeros((5, C_IN + 1), device="cuda"), [0, 5])
    with pytest.raises(ValueError, match="contiguous"):
        m.predict_ragged(torch.zeros((5, 2 * C_IN), device="cuda")[:, :C_IN], [0, 5])
    with pytest.raises(Exception):
        m.predict_ragged(X.cpu(), off)
    # a model that does not compute in float32 has no ragged pass, and says why
    m.compute_dtype = "bfloat16"
    try:
        assert "float32 only" in m.ragged_refusal() and "bfloat16" in m.ragged_refusal()
        with pytest.raises(ValueError, match="float32 only"):
            m.embed_ragged(X, off)
    finally:
        m.compute_dtype = "float32"
