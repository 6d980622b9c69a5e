"""
Every kernel and template instantiation of the recurrence files (csrc/rnn.hip, gru.hip, lstm_step.hip on csrc/rnn_step.h) on
each side of each dispatch condition, through the C ABI, against the float64 one-step references of oracle/rnn_paths_np.py.

The shapes that select a path sit in that module's PATHS tables (STEP: lidbox_lstm_step_*, GRU: lidbox_gru_*, LSTM: lidbox_lstm_*
resident and stepped, POOL: lidbox_seq_avg_pool_*), each row with the condition of the source it is there for;
tests/test_oracle_rnn_paths.py proves on the CPU that every row selects what it says, that the rows reach every instantiation,
and that the bounds used here catch a dropped k term, a shifted unit or row, a wrong neighbour row, swapped gate blocks and an
omitted dh_last or carry.

Buffers.  Every buffer a call may write -- zg, hseq, cseq, qh, hlast, the workspaces -- is a tests/guarded.py payload: the
words around it must still hold the fill afterwards.  Outputs start as NaN, except rows 0 and T + 1 of hseq's slice, which the
contract wants zero; the columns of a wide hseq / dh_seq outside the layer's slice are NaN going in and coming out.  Workspaces
have exactly the size the library asks for.  Misaligned pointers come from Guarded(shift=..) and the residues the row claims
are asserted.

How results are judged (oracle/rnn_paths_np.py, docstring section 3).  Forward: every stored step t of every direction -- gates,
c, h, the GRU's qh -- element by element against the float64 step recomputed from the DEVICE'S OWN state of step t -+ 1, within
the derived bound (n = 2 K roundings for a K-term MFMA or GEMM chain, K + 1 for the resident fmaf chain; 2 ulp for expf and 4
for tanhf, twice what the HIP math documentation states); h also within the project's 5e-5 of the whole-layer float64 oracle.
Backward: dZ (and the GRU's h block of dZrec) against a float64 chain seeded from the device's forward state, within the bound
propagated along it.  Exact: the float4 / float2 / scalar paths of one shape, a row alone and at the first and last place of
B = 65 and 129 (resident: across RT = 1, 2, 4), run to run, dirs = 1 against direction 0 of dirs = 2, hlast against hseq,
inputs after the call, zero rows, NaN gaps, B = 0.  Resident against fused at T = 2: step 0 is bit-identical, so step 1 of
both lies within its own bound of the same reference.  Each row runs on two data sets: N(0, 1) and 1 + 0.1 N(0, 1).

First measured (MI355X, one run, 291 cases in 5.7 s; largest err / bound, "normal" / "offset" data): fused step gates 0.64 /
0.54, c 0.30 / 0.32, h 0.22 / 0.20, dZ 0.56 / 0.40; GRU gates 0.52 / 0.58, qh 0.32 / 0.45, h 0.45 / 0.40, dZx 0.71 / 0.60, dZrec
0.67 / 0.50; resident gates 0.69 / 0.57, dZ 0.54 / 0.44; stepped gates 0.63 / 0.56, dZ 0.51 / 0.39; pool 0.29 / 0.32 forward, 0.92 /
0.79 backward.  The T = 1 rows (no product: the transcendental allowance alone) reach 0.59 on the gates.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded
from lidbox_amd.testutil import device_copy
from oracle import rnn_paths_np as rp

pytestmark = pytest.mark.gpu

WORST = {}                                           # group -> largest err / bound seen (printed by every case)
ROWS = [(k, r) for k in ("step", "gru", "lstm") for r in rp.PATHS[k]]
IDS = ["%s-%s" % (k, r["name"]) for k, r in ROWS]


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """bit for bit, NaN payloads included"""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _judge(group, what, got, ref):
    q = rp.ratio(got, ref)
    assert np.isfinite(np.asarray(got, np.float64)).all(), "%s: %d elements not written or not finite" % (
        what, (~np.isfinite(np.asarray(got, np.float64))).sum())
    worst = float(q.max()) if q.size else 0.0
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print("%-52s max err/bound=%.3e   [%s so far %.3e]" % (what, worst, group, WORST[group]))
    assert (q <= 1.0).all(), "%s: %d elements over the bound, worst %.3g x at %s" % (
        what, (q > 1.0).sum(), worst, np.unravel_index(np.argmax(q), q.shape))


def _ptr(g, words=0):
    return ctypes.c_void_p(g.view.data_ptr() + 4 * words)


def _ws(nbytes):
    """a workspace of exactly nbytes (None when the library asks for none)"""
    return Guarded((nbytes,), dtype=torch.uint8) if nbytes else None


def _wsargs(ws):
    return (ws.ptr, ws.n) if ws is not None else (None, 0)


def _strided(buf, B, bs, T, rs, D):
    """the [B, T, D] window of a flat buffer with batch stride bs and row stride rs"""
    return buf.view.as_strided((B, T, D), (bs, rs, 1))


def run_layer(r, dat):
    """one layer forward and backward through the C ABI, every buffer guarded.  Returns st (gates, c | qh, hs: the layer's
    slice of hseq), bw (dz, dq) and hlast, as numpy arrays."""
    nv = _nv()
    lib = nv.lib
    fam, H, dirs, B, T = r["fam"], r["H"], r["dirs"], r["B"], r["T"]
    gru = fam == "gru"
    ng = 3 if gru else 4
    D = dirs * H
    sh = r["shift"]
    st_ = nv.current_stream()
    rs = rp.h_rs(r) if fam == "step" else D
    col = r["col"]
    U = [Guarded(u.shape, init=torch.from_numpy(u), shift=sh.get("U%d" % d, 0)) for d, u in enumerate(dat["U"])]
    U0, U1 = U[0].ptr, (U[1].ptr if dirs == 2 else None)
    zg = Guarded(dat["zg"].shape, init=torch.from_numpy(dat["zg"]), shift=sh.get("zg", 0))
    hseq = Guarded((B, T + 2, rs), shift=sh.get("hseq", 0))
    hseq.view[:, 0, col:col + D] = 0.0
    hseq.view[:, T + 1, col:col + D] = 0.0
    hp = _ptr(hseq, col)
    want = rp.residues(r)
    got = dict(U0=U[0].view.data_ptr(), U1=U[dirs - 1].view.data_ptr(), zg=zg.view.data_ptr(), hseq=hp.value)
    aux = Guarded((dirs, B, T, H), shift=sh.get("qh", 0))             # cseq (LSTM) or qh (GRU)
    if gru:
        got["qh"] = aux.view.data_ptr()
    for k_, p in got.items():
        assert p % 16 == want[k_], (k_, p % 16, want[k_])
    dh_seq, dh_last = rp.given(r, dat)
    dseq = dlast = None
    dbs = drs = 0
    if dh_seq is not None:
        drs = D + (r["dh_wide"] if fam == "step" else 0)
        dbs = (T + 1) * drs if fam == "step" else T * D + r["dh_wide"]
        dseq = Guarded((B * dbs,))
        _strided(dseq, B, dbs, T, drs, D).copy_(torch.from_numpy(dh_seq))
        dseq0 = dseq.numpy().copy()
    if dh_last is not None:
        dlast = Guarded(dh_last.shape, init=torch.from_numpy(dh_last))
    pd = dseq.ptr if dseq is not None else None
    pl = dlast.ptr if dlast is not None else None
    hlast = Guarded((B, D)) if gru and r["hlast"] else None
    if gru:
        brec = [device_copy(b) for b in dat["brec"]]
        ws = _ws(lib.lidbox_gru_workspace(B, T, H, dirs))
        assert ws.n == rp.step_workspace(B, T, H, dirs)
        nv.check(lib.lidbox_gru_fwd(U0, U1, nv.ptr(brec[0]), nv.ptr(brec[1]) if dirs == 2 else None, dirs, B, T, H, zg.ptr, hp,
                                    aux.ptr, hlast.ptr if hlast is not None else None, st_))
    elif fam == "step":
        ws = _ws(lib.lidbox_lstm_step_workspace(B, T, H, dirs))
        assert ws.n == rp.step_workspace(B, T, H, dirs)
        nv.check(lib.lidbox_lstm_step_fwd(U0, U1, dirs, B, T, H, zg.ptr, hp, rs, aux.ptr, *_wsargs(ws), st_))
    else:
        ws = _ws(lib.lidbox_lstm_workspace(B, T, H, dirs))
        assert (ws is None) == (rp.lstm_form(H) == "res")
        nv.check(lib.lidbox_lstm_fwd(U0, U1, dirs, B, T, H, zg.ptr, hp, aux.ptr, *_wsargs(ws), st_))
    torch.cuda.synchronize()
    hfull = hseq.numpy().copy()
    st = dict(gates=zg.numpy().copy(), hs=np.ascontiguousarray(hfull[:, :, col:col + D]))
    st["qh" if gru else "c"] = aux.numpy().copy()
    out = dict(st=st, hlast=hlast.numpy().copy() if hlast is not None else None)
    other = np.ones(rs, bool)
    other[col:col + D] = False
    assert np.isnan(hfull[:, :, other]).all(), "hseq: columns outside the layer's slice were written"
    if ws is not None:
        ws.check()
    if gru:
        nv.check(lib.lidbox_gru_bwd(U0, U1, dirs, B, T, H, zg.ptr, hp, aux.ptr, pd, dbs, pl, *_wsargs(ws), st_))
    elif fam == "step":
        nv.check(lib.lidbox_lstm_step_bwd(U0, U1, dirs, B, T, H, zg.ptr, aux.ptr, pd, dbs, drs, pl, *_wsargs(ws), st_))
    else:
        nv.check(lib.lidbox_lstm_bwd(U0, U1, dirs, B, T, H, zg.ptr, aux.ptr, pd, dbs, pl, *_wsargs(ws), st_))
    torch.cuda.synchronize()
    out["bw"] = dict(dz=zg.numpy().copy())
    if gru:
        out["bw"]["dq"] = aux.numpy().copy()
    else:
        assert _same(aux.numpy(), st["c"]), "cseq was modified by backward"
    if ws is not None:
        ws.check()
    # inputs come back bit-identical
    assert _same(hseq.numpy(), hfull), "hseq was modified by backward"
    for d in range(dirs):
        assert _same(U[d].numpy(), dat["U"][d]), "U%d was modified" % d
    if dseq is not None:
        assert _same(dseq.numpy(), dseq0), "dh_seq (or a gap between its rows) was modified"
    if dlast is not None:
        assert _same(dlast.numpy(), dh_last), "dh_last was modified"
    return out


def _data(r, kind):
    return rp.draw("gru" if r["fam"] == "gru" else "step", r["H"], r["dirs"], r["B"], r["T"], kind)


@functools.lru_cache(maxsize=None)
def _result(k, name, kind):
    r = next(x for x in rp.PATHS[k] if x["name"] == name)
    dat = _data(r, kind)
    return r, dat, run_layer(r, dat)


def _equal_runs(a, b, bwd=True, what=""):
    for key in a["st"]:
        assert _same(a["st"][key], b["st"][key]), "%s: %s differs" % (what, key)
    if bwd:
        for key in a["bw"]:
            assert _same(a["bw"][key], b["bw"][key]), "%s: backward's %s differs" % (what, key)


# ---------------------------------------------------------------------------------------------------- every row
@pytest.mark.parametrize("kind", rp.KINDS)
@pytest.mark.parametrize("k,r", ROWS, ids=IDS)
def test_row(k, r, kind):
    r, dat, out = _result(k, r["name"], kind)
    st, bw = out["st"], out["bw"]
    fam, H, dirs, T = rp.fam_of(r), r["H"], r["dirs"], r["T"]
    group = "%s/%s" % (fam, kind)
    what = "%s-%s %s" % (k, r["name"], kind)
    assert not st["hs"][:, 0].any() and not st["hs"][:, T + 1].any(), "rows 0 and T + 1 of hseq are not zero"
    for name, got, ref in rp.fwd_checks(r, dat, st):
        _judge("%s fwd %s" % (group, name), "%s %s" % (what, name), got, ref)
    h = rp.h_of(st["hs"], dirs, H)
    whole = rp.gru_layer(dat["U"], dat["brec"], dat["zg"])[2] if fam == "gru" else rp.lstm_layer(dat["U"], dat["zg"])[2]
    eh = float(np.abs(h - whole).max())
    assert eh <= rp.H_TOL, eh
    for name, got, ref in rp.bwd_checks(r, dat, st, bw):
        _judge("%s bwd %s" % (group, name), "%s %s" % (what, name), got, ref)
    if out["hlast"] is not None:
        last = np.concatenate([h[d][:, T - 1 if d == 0 else 0] for d in range(dirs)], 1)
        assert _same(out["hlast"], last), "hlast is not the direction's final h"
    if r["twin"]:
        # the float4, float2 and scalar paths of one shape feed the MFMAs in the same k order: the same bits
        r2, _, out2 = _result(k, r["twin"], kind)
        _equal_runs(out, out2, bwd=(r2["dh"] == r["dh"]), what="%s against %s" % (r["name"], r["twin"]))


# ---------------------------------------------------------------------------------------------------- exact relations
def _take(dat, idx):
    return dict(dat, zg=np.ascontiguousarray(dat["zg"][:, idx]), dh_seq=np.ascontiguousarray(dat["dh_seq"][idx]),
                dh_last=np.ascontiguousarray(dat["dh_last"][idx]))


def _pick(out, b):
    """the results of batch row b"""
    return dict(st={k_: (v[:, b] if k_ != "hs" else v[b]) for k_, v in out["st"].items()},
                bw={k_: v[:, b] for k_, v in out["bw"].items()})


@pytest.mark.parametrize("fam,H,Bs", [("step", 17, (65, 129)), ("step", 16, (65, 129)), ("gru", 17, (65, 129)), ("gru", 16, (65, 129)),
                                      ("lstm", 17, (513, 1025)), ("lstm", 80, (513, 1025))])
def test_a_row_is_bit_identical_alone_and_in_a_batch(fam, H, Bs):
    """alone (B = 1) and at the first and last place of a batch; resident: B = 513 runs RT = 2, B = 1025 RT = 4"""
    T, dirs = 3, 2
    big = rp.draw("gru" if fam == "gru" else "step", H, dirs, max(Bs), T, "normal")
    alone = {}
    for B in Bs:
        r = rp._row("b%d" % B, fam, H, B=B, dh="both")
        out = run_layer(r, _take(big, slice(0, B)))
        for b in (0, B - 1):
            if b not in alone:
                alone[b] = run_layer(rp._row("b1", fam, H, B=1, dh="both"), _take(big, slice(b, b + 1)))
            _equal_runs(_pick(out, b), _pick(alone[b], 0), what="%s H=%d row %d of B=%d" % (fam, H, b, B))
    if fam == "lstm":
        assert [rp.pick_rt(B, dirs) for B in (1,) + Bs] == [1, 2, 4]


@pytest.mark.parametrize("k,name", [("step", "w2_H250"), ("step", "tile_B65_H17"), ("gru", "vec_H132"), ("gru", "tile_B65_H17"),
                                    ("lstm", "res_H65_B5"), ("lstm", "res_rt2_d2_H17"), ("lstm", "stp_H81_B17")])
def test_run_to_run_identity(k, name):
    r, dat, out = _result(k, name, "normal")
    _equal_runs(out, run_layer(r, dat), what="%s-%s run to run" % (k, name))


@pytest.mark.parametrize("fam,H", [("step", 16), ("step", 17), ("gru", 16), ("gru", 15), ("lstm", 17), ("lstm", 81)])
def test_one_direction_equals_direction_0_of_two(fam, H):
    B, T = 5, 3
    outs = []
    for dirs in (1, 2):
        r = rp._row("d%d" % dirs, fam, H, dirs=dirs, B=B, T=T, dh="both")
        outs.append(run_layer(r, _data(r, "offset")))
    one, two = outs
    for key, v in one["st"].items():
        w = two["st"][key]
        assert _same(v, w[:, :, :H] if key == "hs" else w[:1]), key
    for key, v in one["bw"].items():
        assert _same(v, two["bw"][key][:1]), key


@pytest.mark.parametrize("kind", rp.KINDS)
@pytest.mark.parametrize("H", [48, 80])
def test_resident_agrees_with_the_fused_step(H, kind):
    """T = 2: step 0 has no product and is bit-identical in both forms, so at step 1 both start from the same state and each
    lies within its own bound of one reference: they differ by at most the sum of the two bounds"""
    B, T, dirs = 5, 2, 2
    rr, rs_ = rp._row("res", "lstm", H, B=B, T=T), rp._row("fused", "step", H, B=B, T=T)
    dat = _data(rr, kind)
    a, b = run_layer(rr, dat), run_layer(rs_, dat)
    for d in range(dirs):
        t0 = 0 if d == 0 else T - 1
        for key in ("gates", "c"):
            assert _same(a["st"][key][d, :, t0], b["st"][key][d, :, t0]), (key, d)
        assert _same(a["st"]["hs"][:, t0 + 1, d * H:(d + 1) * H], b["st"]["hs"][:, t0 + 1, d * H:(d + 1) * H])
    ca, cb = rp.fwd_checks(rr, dat, a["st"]), rp.fwd_checks(rs_, dat, b["st"])
    for (name, ga, ea), (_, gb, eb) in zip(ca, cb):
        diff = np.abs(np.asarray(ga, np.float64) - np.asarray(gb, np.float64))
        assert (diff <= ea.e + eb.e).all(), name
        print("resident vs fused H=%d %s %s: max |diff| / (sum of bounds) = %.3e" % (H, kind, name, (diff / (ea.e + eb.e)).max()))
    da, db = rp.bwd_checks(rr, dat, a["st"], a["bw"])[0], rp.bwd_checks(rs_, dat, b["st"], b["bw"])[0]
    _judge("res/%s bwd dZ" % kind, "resident H=%d dZ" % H, da[1], da[2])
    _judge("step/%s bwd dZ" % kind, "fused H=%d dZ" % H, db[1], db[2])


# ---------------------------------------------------------------------------------------------------- sequence average pooling
@pytest.mark.parametrize("kind", rp.KINDS)
@pytest.mark.parametrize("p", rp.POOL, ids=lambda p: p["name"])
def test_seq_avg_pool(p, kind):
    nv = _nv()
    B, T, C, alpha = p["B"], p["T"], p["C"], p["alpha"]
    rs, ldo = (C + 3, C + 5) if p["pitched"] else (C, C)
    bs = (T + 1) * rs if p["pitched"] else T * rs
    rng = np.random.default_rng([B, T, C])
    draw = lambda shape: (rng.standard_normal(shape) if kind == "normal" else 1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    x, dout, dx0 = draw((B, T, C)), draw((B, C)), draw((B, T, C))
    st_ = nv.current_stream()
    xg = Guarded((B * bs,))
    _strided(xg, B, bs, T, rs, C).copy_(torch.from_numpy(x))
    og = Guarded((B, ldo))
    nv.check(nv.lib.lidbox_seq_avg_pool_fwd(xg.ptr, B, T, C, bs, rs, alpha, og.ptr, ldo, st_))
    torch.cuda.synchronize()
    o = og.numpy()
    assert np.isnan(o[:, C:]).all(), "the gap of out's rows was written"
    ref, bound = rp.seq_avg_pool_ref(x, alpha)
    _judge("pool/%s fwd" % kind, "pool fwd %s %s" % (p["name"], kind), o[:, :C], rp.E(ref, bound))
    # backward: dout pitched by ldo, dx pitched like x, pre-filled with known values where it accumulates
    dg = Guarded((B, ldo))
    dg.view[:, :C].copy_(torch.from_numpy(dout))
    if p["acc"]:
        _strided(xg, B, bs, T, rs, C).copy_(torch.from_numpy(dx0))
    else:
        xg.view.fill_(float("nan"))
    before = xg.numpy().copy()
    nv.check(nv.lib.lidbox_seq_avg_pool_bwd(dg.ptr, ldo, B, T, C, alpha, xg.ptr, bs, rs, p["acc"], st_))
    torch.cuda.synchronize()
    after = xg.numpy()
    win = np.lib.stride_tricks.as_strided(after, (B, T, C), (4 * bs, 4 * rs, 4))
    ref, bound = rp.seq_avg_pool_bwd_ref(dout, alpha, T, dx0 if p["acc"] else None)
    _judge("pool/%s bwd" % kind, "pool bwd %s %s" % (p["name"], kind), win, rp.E(ref, bound))
    mask = np.zeros(B * bs, bool)
    np.lib.stride_tricks.as_strided(mask, (B, T, C), (bs, rs, 1))[...] = True
    assert _same(after[~mask], before[~mask]) and np.isnan(after[~mask]).all(), "dx: a gap was written"
    assert _same(dg.numpy()[:, :C], dout)


# ---------------------------------------------------------------------------------------------------- B = 0
def test_an_empty_batch_touches_nothing():
    nv = _nv()
    lib = nv.lib
    st_ = nv.current_stream()
    H, T = 16, 3
    U = device_copy(np.ones((H, 4 * H), np.float32))
    b = device_copy(np.ones(3 * H, np.float32))
    bufs = [Guarded((64,)) for _ in range(6)]
    z, h, c, q, l, w = (g.ptr for g in bufs)
    for dirs in (1, 2):
        U1 = nv.ptr(U) if dirs == 2 else None
        b1 = nv.ptr(b) if dirs == 2 else None
        assert lib.lidbox_lstm_fwd(nv.ptr(U), U1, dirs, 0, T, H, z, h, c, None, 0, st_) == 0
        assert lib.lidbox_lstm_bwd(nv.ptr(U), U1, dirs, 0, T, H, z, c, q, T * dirs * H, l, None, 0, st_) == 0
        assert lib.lidbox_lstm_fwd(nv.ptr(U), U1, dirs, 0, T, 100, z, h, c, None, 0, st_) == 0
        assert lib.lidbox_lstm_bwd(nv.ptr(U), U1, dirs, 0, T, 100, z, c, q, T * dirs * 100, l, None, 0, st_) == 0
        assert lib.lidbox_lstm_step_fwd(nv.ptr(U), U1, dirs, 0, T, H, z, h, dirs * H, c, None, 0, st_) == 0
        assert lib.lidbox_lstm_step_bwd(nv.ptr(U), U1, dirs, 0, T, H, z, c, q, T * dirs * H, dirs * H, l, None, 0, st_) == 0
        assert lib.lidbox_gru_fwd(nv.ptr(U), U1, nv.ptr(b), b1, dirs, 0, T, H, z, h, q, l, st_) == 0
        assert lib.lidbox_gru_bwd(nv.ptr(U), U1, dirs, 0, T, H, z, h, q, c, T * dirs * H, l, None, 0, st_) == 0
    assert lib.lidbox_seq_avg_pool_fwd(z, 0, T, H, T * H, H, 1.0, h, H, st_) == 0
    assert lib.lidbox_seq_avg_pool_bwd(z, H, 0, T, H, 1.0, h, T * H, H, 1, st_) == 0
    torch.cuda.synchronize()
    for g in bufs:
        assert np.isnan(g.numpy()).all()
    for fn in (lib.lidbox_lstm_workspace, lib.lidbox_lstm_step_workspace, lib.lidbox_gru_workspace):
        assert fn(0, T, 100, 2) == 0


def test_zz_report():
    """the largest err / bound of every group of this run (docs/LAB_NOTEBOOK.md section 20 records one such run)"""
    for g in sorted(WORST):
        print("WORST %-28s %.3e" % (g, WORST[g]))
    assert all(v <= 1.0 for v in WORST.values())
