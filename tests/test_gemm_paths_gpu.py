"""
Every kernel instantiation of the fp32 GEMM family (csrc/gemm.hip on gemm_shared.h, gemm_dma.h, gemm_dma8.h, gemm_sk.h) on each
side of each dispatch condition, through the C ABI, against the float64 references of oracle/gemm_paths_np.py.

The shapes that select a path sit in that module's PATHS tables (ROWS: lidbox_gemm_nn / _nt, TN: lidbox_gemm_tn, COLSUM:
lidbox_colsum, PAIR: lidbox_gemm_nt_tn), each row with the source condition it is there for; tests/test_oracle_gemm_paths.py
proves on the CPU that the restated dispatch equals the library's planner exports, that every row selects what it says, that
the rows reach all 65 instantiations the launch sites name, and that the bounds used here catch each planted mutation.

Buffers.  Every buffer a call may write -- C / dX, dW, the bias gradient, the column sums, every workspace -- and every input
is a tests/guarded.py payload.  Outputs start as NaN (the old values where the epilogue accumulates); the rows between
utterances of a pitched C and the columns between N and ldc of dW are NaN going in and must be the same NaN coming out.  Pitched
inputs carry NaN in their gaps: A between K and row_stride, B between the row end and ldb, the mask between C's rows.
Workspaces start as NaN in every fp32 word and have exactly the size the library returns (or, where the row says so, one byte less / 4 bytes off 16-byte alignment).
Misaligned pointers come from Guarded(shift=..) and the residue the row claims is asserted.  Inputs are compared bit for bit
with their copies after the call.

Paths.  After each call lidbox_gemm_last_family and lidbox_gemm_last_launches must equal the oracle's prediction, and so must
lidbox_gemm_last_carried: the count of the row after a PAIR or CARRY call; after lidbox_gemm_nn / _nt / _tn, which carry nothing
and by their contract do not touch it (it reports the most recent carry call), the value it had before the call.  A mismatch
fails, no row skips.

Judging (oracle/gemm_paths_np.py section 3): element by element, err / bound <= 1 on `normal` and `offset` with
n = 2 K + p + e, bit equality with the int64 result on `exact`.  Exact identities: run to run on every row; a row of A at the
first and at the last place of M (families 0, 1, 3); the pair launch against the two calls; carried jobs against the same jobs
as a launch of their own (LIDBOX_GEMM_NO_CARRY).  DMA against LIDBOX_GEMM_DMA=0 is
NOT asserted bit-identical (the two operand paths were not read for the same summation order): the al-* and dma-* rows share
their shapes and are both judged within the bound of the same kind of reference.

Not run here: both sides of the 32-bit extent guards (PATHS["FAR"], run by tests/test_gemm_far_gpu.py in sparse allocations),
lidbox_gemm_nt_tn_carry with pending jobs (tests/test_gemm_sk_gpu.py), the bf16 family (tests/test_gemm16_paths_gpu.py).

Device-side sensitivity, tried once with a scratch build that is not part of the tree: gemm_rows_body made to skip the MFMAs of
K step 1 when a launch has three or more steps (the planted "dropped interior K step").  Of the 208 ROWS cases exactly the 33
that run a register-staged kernel over three or more K steps failed (every un-* and al-* row at the six tiles, K33 .. K35,
splitk-lone-tail, model-small, sk-refuse-K%4), each on all three data sets; the 175 others passed.  The other mutations rest
on the CPU emulation.

First measured (MI355X, one run on one card, 283 cases in 7.5 s; largest err / bound, `normal` / `offset`; `exact` is bit-equal
everywhere): gemm_rows_kernel 0.21 / 0.21, with rows_reduce_kernel 0.01 / 0.02; gemm_rows8_kernel 0.10 / 0.12, with rows_reduce_kernel 0.01 / 0.02;
gemm_rows_dma_kernel 0.12 / 0.12, with rows_reduce_kernel 0.01 / 0.03, with a streamed remainder 0.01 / 0.04;
gemm_rows_dma8_kernel 0.09 / 0.11, with rows_reduce_kernel 0.01 / 0.02; gemm_sk_rows_kernel 0.04 / 0.07; gemm_skp_rows_kernel 0.01 / 0.02; gemm_tn_kernel 0.02 / 0.06
(both reduces); gemm_tn_dma_kernel 0.15 / 0.16 with splitk_reduce4_kernel, 0.02 / 0.04 with splitk_reduce_kernel;
gemm_sk_tn_kernel 0.00 / 0.01; fused bias gradient 0.02 / 0.08; colsum 0.01 / 0.06; pair and its two calls 0.05 / 0.08; carried
dgrad and wgrad 0.03 / 0.06.  The slowest case takes 0.55 s (tail-split).  Every launch took the predicted path.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import gemm_paths_np as gp

pytestmark = pytest.mark.gpu

WORST = {}                                           # (group, data set) -> largest err / bound seen (printed by every case)


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _setenv(monkeypatch, env):
    for k in list(os.environ):
        if k.startswith("LIDBOX_GEMM_"):
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _buf(flat, shift=0):
    """a flat float32 array (NaN included) as a guarded device buffer, `shift` words off 16-byte alignment"""
    flat = np.ascontiguousarray(flat, np.float32).ravel()
    g = Guarded((flat.size,), init=torch.from_numpy(flat), shift=shift)
    assert g.view.data_ptr() % 16 == 4 * shift
    return g


def _ws(nbytes, aligned=True):
    """a workspace of exactly nbytes (None when there is none) whose fp32 words all start as NaN (a slab, slice or partial read
    before it was written shows in the result); not aligned: 4 bytes past a 16-byte boundary"""
    if nbytes <= 0:
        return None, None, 0
    g = Guarded((nbytes + (0 if aligned else 4),), dtype=torch.uint8)
    nan = torch.tensor([0x00, 0x00, 0xC0, 0x7F], dtype=torch.uint8, device="cuda")       # 0x7FC00000: every fp32 word starts as NaN
    g.view.copy_(nan.repeat(g.n // 4 + 1)[:g.n])
    p = g.view.data_ptr() + (0 if aligned else 4)
    assert p % 16 == (0 if aligned else 4)
    return g, ctypes.c_void_p(p), nbytes


def _note(group, ds, what, worst):
    key = (group, ds)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-60s %-6s max err/bound=%.3e   [%s so far %.3e]" % (what, ds, worst, group, WORST[key]))


def _desc(nv, g, d):
    return nv.Rows(g.view.data_ptr(), d["bs"], d["rs"], d["batch"], d["rpb"])


def _launches(nv):
    out = (ctypes.c_int * 3)()
    nv.check(nv.lib.lidbox_gemm_last_launches(out))
    return list(out)


def run_rows(r, dat):
    """one lidbox_gemm_nn / _nt call of a ROWS row in guarded buffers; returns (flat C, family, launches)"""
    nv = _nv()
    mis = r["mis"]
    a, b, c = _buf(dat["a_flat"], mis.get("A", 0)), _buf(dat["b_flat"], mis.get("B", 0)), _buf(dat["c_flat"], mis.get("C", 0))
    aux = None
    if r["epi"] in gp.EPI_HAS_BIAS:
        aux = _buf(dat["bias"], mis.get("aux", 0))
    elif r["epi"] in gp.EPI_HAS_MASK and dat["mask_flat"] is not None:
        aux = _buf(dat["mask_flat"], mis.get("aux", 0))
    elif r["epi"] in gp.EPI_HAS_MASK:
        aux = _buf(np.zeros(1, np.float32))
    wsb, ws_al = gp.row_ws_bytes(r)
    wsg, wsp, wsn = _ws(wsb, ws_al)
    fn = nv.lib.lidbox_gemm_nn if r["kind"] == "nn" else nv.lib.lidbox_gemm_nt
    carried = nv.lib.lidbox_gemm_last_carried()
    nv.check(fn(_desc(nv, a, r["a"]), b.ptr, gp.ldb_of(r), _desc(nv, c, r["c"]), r["K"], r["N"], r["epi"],
                aux.ptr if aux is not None else None, wsp, wsn, nv.current_stream()))
    torch.cuda.synchronize()
    fam, launches = nv.lib.lidbox_gemm_last_family(), _launches(nv)
    assert nv.lib.lidbox_gemm_last_carried() == carried, "a call that carries nothing leaves lidbox_gemm_last_carried as it was"
    got = c.numpy().copy()                                         # checks the guard words around C
    ins = [(a, dat["a_flat"]), (b, dat["b_flat"])]
    if r["epi"] in gp.EPI_HAS_BIAS:
        ins.append((aux, dat["bias"]))
    elif dat["mask_flat"] is not None:
        ins.append((aux, dat["mask_flat"]))
    for g_, src in ins:
        assert _same(g_.numpy(), np.ascontiguousarray(src, np.float32).ravel()), "an input changed"
    if wsg is not None:
        wsg.check()
    return got, fam, launches


ROWS = gp.PATHS["ROWS"]
BIG = [r for r in ROWS if r["M"] * r["K"] > 1 << 24]             # one data set per case: each case stays at a few seconds
CASES = [(r, gp.DATASETS) for r in ROWS if r not in BIG] + [(r, (ds,)) for r in BIG for ds in gp.DATASETS]


@pytest.mark.parametrize("r,sets", CASES, ids=[r["name"] + ("" if len(d) == 3 else "-" + d[0]) for r, d in CASES])
def test_rows_row(r, sets, monkeypatch):
    _setenv(monkeypatch, r["env"])
    pred = gp.row_predict(r)
    group = pred["kernels"][0].split("<")[0] + ("+reduce" if "rows_reduce_kernel" in pred["kernels"] else "") + ("+stream" if pred["g"] else "") if pred["kernels"] else "none"
    for ds in sets:
        dat = gp.make_rows_data(r, ds)
        got, fam, launches = run_rows(r, dat)
        assert fam == pred["family"] and launches == pred["launches"], (r["why"], fam, launches, pred)
        ok, worst, what = gp.judge_rows(r, ds, dat, got, pred["p"])
        _note(group, ds, r["name"], worst)
        assert ok, "%s [%s] %s: worst err/bound %.3g (%s)" % (r["name"], ds, what, worst, r["why"])
        again, _, _ = run_rows(r, dat)
        assert _same(got, again), "not bit-identical run to run"


def _place_rows():
    """the first dense row of every kernel (with and without its split-K reduce) of families 0, 1 and 3; a streamed remainder
    sums its tiles in pieces and a tail split's remainder is split along K while the whole tiles are not: left out"""
    seen, out = set(), []
    for r in ROWS:
        p = gp.row_predict(r)
        if not p["kernels"] or p["family"] == 2 or p["g"] or p["tail_split"] or r["a"]["batch"] != 1 or r["c"]["batch"] != 1 or r["M"] < 2:
            continue
        key = (p["kernels"][0].split("<")[0], p["kernels"][0].endswith("un>"), len(p["kernels"]))
        if key not in seen:
            seen.add(key)
            out.append(r)
    return out


PLACE = _place_rows()


@pytest.mark.parametrize("r", PLACE, ids=[r["name"] for r in PLACE])
def test_a_row_gives_the_same_bits_at_the_first_and_the_last_place_of_M(r, monkeypatch):
    """every output row is one k-ordered chain whatever tile and lane holds it (families 0, 1 and 3: the tile's split of K
    does not depend on the tile)"""
    _setenv(monkeypatch, r["env"])
    assert gp.row_predict(r)["family"] != 2 and r["a"]["batch"] == 1
    dat = gp.make_rows_data(r, "normal")
    M, N, K = r["M"], r["N"], r["K"]
    lo, hi = gp.row_offsets(r["a"])[[0, M - 1]]
    dat["a_flat"][hi:hi + K] = dat["a_flat"][lo:lo + K]
    clo, chi = gp.row_offsets(r["c"])[[0, M - 1]]
    if dat["mask_flat"] is not None:
        dat["mask_flat"][chi:chi + N] = dat["mask_flat"][clo:clo + N]
    if r["epi"] in gp.EPI_ACCUMS:
        dat["c_flat"][chi:chi + N] = dat["c_flat"][clo:clo + N]
    got, _, _ = run_rows(r, dat)
    assert _same(got[clo:clo + N], got[chi:chi + N])


TN = gp.PATHS["TN"]


def run_tn(r, dat):
    nv = _nv()
    mis = r["mis"]
    a, b = _buf(dat["a_flat"], mis.get("A", 0)), _buf(dat["b_flat"], mis.get("B", 0))
    c = _buf(dat["c_flat"], mis.get("C", 0))
    bg = _buf(dat["old_bg"], mis.get("bg", 0)) if r["bias_grad"] else None
    wsb = nv.lib.lidbox_gemm_tn_workspace(r["M"], r["K1"], r["N"])
    assert wsb == gp.tn_workspace(r["M"], r["K1"], r["N"], r["env"])
    wsg, wsp, wsn = _ws(wsb)
    carried = nv.lib.lidbox_gemm_last_carried()
    nv.check(nv.lib.lidbox_gemm_tn(_desc(nv, a, r["a"]), _desc(nv, b, r["b"]), c.ptr, r["N"] + r["ldc_pad"], r["K1"], r["N"], r["accumulate"],
                                   bg.ptr if bg is not None else None, wsp, wsn, nv.current_stream()))
    torch.cuda.synchronize()
    fam, launches = nv.lib.lidbox_gemm_last_family(), _launches(nv)
    assert nv.lib.lidbox_gemm_last_carried() == carried, "lidbox_gemm_tn carries nothing: lidbox_gemm_last_carried stays as it was"
    assert _same(a.numpy(), dat["a_flat"]) and _same(b.numpy(), dat["b_flat"]), "an input changed"
    wsg.check()
    return c.numpy().copy(), (bg.numpy().copy() if bg is not None else None), fam, launches


@pytest.mark.parametrize("r", TN, ids=[r["name"] for r in TN])
def test_tn_row(r, monkeypatch):
    _setenv(monkeypatch, r["env"])
    pred = gp.tn_row_predict(r)
    group = pred["kernels"][0].split("<")[0] + "+" + pred["kernels"][1]
    for ds in gp.DATASETS:
        dat = gp.make_tn_data(r, ds)
        c, bg, fam, launches = run_tn(r, dat)
        assert fam == pred["family"] and launches == pred["launches"], (r["why"], fam, launches, pred)
        ok, worst, worst_g = gp.judge_tn(r, ds, dat, c, bg, pred["splits"], pred["rps"])
        _note(group, ds, r["name"], worst)
        _note("bias_grad", ds, r["name"], worst_g)
        assert ok, "%s [%s]: worst err/bound dW %.3g, bias grad %.3g (%s)" % (r["name"], ds, worst, worst_g, r["why"])
        c2, bg2, _, _ = run_tn(r, dat)
        assert _same(c, c2) and (bg is None or _same(bg, bg2)), "not bit-identical run to run"


@pytest.mark.parametrize("r", gp.PATHS["COLSUM"], ids=[r["name"] for r in gp.PATHS["COLSUM"]])
def test_colsum_row(r):
    nv = _nv()
    M, N = r["M"], r["N"]
    for ds in gp.DATASETS:
        rng = np.random.default_rng([3, gp.DATASETS.index(ds), M])
        a_flat = gp.fill_flat(rng, ds, r["a"], N)
        old = gp.draw(rng, ds, N, "int" if ds == "exact" else "ab") if r["accumulate"] else np.full(N, np.nan, np.float32)
        a, out = _buf(a_flat, r["mis"]["A"]), _buf(old)
        wsb = nv.lib.lidbox_colsum_workspace(M, N)
        assert wsb == gp.colsum_workspace(M, N)
        wsg, wsp, wsn = _ws(wsb)
        nv.check(nv.lib.lidbox_colsum(_desc(nv, a, r["a"]), N, out.ptr, r["accumulate"], wsp, wsn, nv.current_stream()))
        torch.cuda.synchronize()
        A = gp.gather(a_flat, r["a"], N).astype(np.float64)
        ref, S = A.sum(0), np.abs(A).sum(0)
        if r["accumulate"]:
            ref, S = ref + old, S + np.abs(old)
        got = out.numpy()
        wsg.check()
        assert _same(a.numpy(), a_flat)
        if ds == "exact":
            assert _same(got, ref.astype(np.float32)), r["name"]
        else:
            q = gp.ratio(got, ref, S, gp.colsum_n(M))
            _note("colsum", ds, r["name"], float(q.max()))
            assert (q <= 1.0).all(), (r["name"], float(q.max()))


def run_pair(r, ds, env, monkeypatch):
    nv = _nv()
    _setenv(monkeypatch, env)
    M, Co, N, K1 = r["M"], r["Co"], r["N"], r["K1"]
    nt = gp._row(r["name"], r["why"], "nt", N, Co, gp._dense(M, Co), epi=gp.EPI_RELU_MASK, env=env)
    tn = gp._tn_row(r["name"], r["why"], K1, Co, gp._dense(M, K1), env=env, accumulate=1)
    dat = gp.make_rows_data(nt, ds)
    tdat = gp.make_tn_data(tn, ds)
    tdat["b_flat"], tdat["B"] = dat["a_flat"], dat["A"]              # dY is the dgrad's A and the wgrad's B
    dy, w, dx, mk = _buf(dat["a_flat"]), _buf(dat["b_flat"]), _buf(dat["c_flat"]), _buf(dat["mask_flat"])
    x, dw, bg = _buf(tdat["a_flat"]), _buf(tdat["c_flat"]), _buf(tdat["old_bg"])
    ws_nt_b = max(nv.lib.lidbox_gemm_rows_workspace(M, N, Co), 2 * M * N * 4)
    ws_tn_b = nv.lib.lidbox_gemm_tn_workspace(M, K1, Co)
    wn, wnp, wnn = _ws(ws_nt_b)
    wt, wtp, wtn = _ws(ws_tn_b)
    if r["shared"]:                                                    # one workspace for both, large enough for either
        wn, wnp, wnn = _ws(max(ws_nt_b, ws_tn_b))
        wt, wtp, wtn, ws_nt_b, ws_tn_b = wn, wnp, wnn, wnn, wnn
    nv.check(nv.lib.lidbox_gemm_nt_tn(_desc(nv, dy, nt["a"]), w.ptr, Co, _desc(nv, dx, nt["c"]), Co, N, nt["epi"], mk.ptr, wnp, wnn,
                                      _desc(nv, x, tn["a"]), dw.ptr, Co, K1, 1, bg.ptr, wtp, wtn, nv.current_stream()))
    torch.cuda.synchronize()
    fam, launches, carried = nv.lib.lidbox_gemm_last_family(), _launches(nv), nv.lib.lidbox_gemm_last_carried()
    wn.check()
    wt.check()
    assert _same(dy.numpy(), dat["a_flat"]) and _same(w.numpy(), dat["b_flat"]) and _same(x.numpy(), tdat["a_flat"]) and _same(mk.numpy(), dat["mask_flat"])
    pair = None if r["shared"] else gp.pair_plan(M, Co, N, K1, ws_nt_b, ws_tn_b, env)
    rows = gp.rows_dispatch(1, M, N, Co, Co % 4 == 0, ws_nt_b, env, nt["epi"])
    tnp = gp.tn_dispatch(M, K1, Co, True, True, ws_tn_b, env)
    if pair is not None:
        assert (fam, launches, carried) == (1, [1, 0, 1 + (1 if pair[0]["splits"] > 1 else 0)], 0), (fam, launches, carried)
    else:
        # the two calls: the wgrad first, its job-form reduce carried by an LDS-DMA dgrad launch
        # (a shared workspace: the reduce runs before the dgrad, a plain lidbox_gemm_nt that does not report a carry)
        job = tnp["kernels"][1] == "splitk_reduce4_kernel"
        assert (fam, launches) == (rows["family"], rows["launches"]), (fam, launches)
        assert r["shared"] or carried == (1 if (job and rows["family"] in (1, 3)) else 0), carried
    ok, worst, what = gp.judge_rows(nt, ds, dat, dx.numpy(), rows["p"])
    okt, worst_t, worst_g = gp.judge_tn(tn, ds, tdat, dw.numpy(), bg.numpy(), tnp["splits"], tnp["rps"])
    _note("pair" if pair is not None else "two calls", ds, r["name"], max(worst, worst_t, worst_g))
    assert ok and okt, (r["name"], ds, what, worst, worst_t, worst_g)
    return pair is not None, dx.numpy().copy(), dw.numpy().copy(), bg.numpy().copy()


@pytest.mark.parametrize("r", gp.PATHS["PAIR"], ids=[r["name"] for r in gp.PATHS["PAIR"]])
def test_pair_row(r, monkeypatch):
    for ds in gp.DATASETS:
        paired, dx, dw, bg = run_pair(r, ds, r["env"], monkeypatch)
        assert paired == r["pair"], r["why"]
        if paired:                                                     # the one launch against the two calls: bit-identical
            p2, dx2, dw2, bg2 = run_pair(r, ds, dict(r["env"], LIDBOX_GEMM_NO_PAIR="1"), monkeypatch)
            assert not p2 and _same(dx, dx2) and _same(dw, dw2) and _same(bg, bg2)


def _job_array(nv, jobs):
    arr = (nv.ReduceJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = j
    return arr


def run_carry(r, ds, env, carried, monkeypatch):
    """the wgrad's partial launch, the zero jobs and the carrying dgrad call of a CARRY row under `env`, judged against the oracle;
    returns (dX, dW, bias gradient, the zero job's buffer), or None where the call is refused"""
    nv = _nv()
    _setenv(monkeypatch, env)
    M, Co, N, K1, Mw = r["M"], r["Co"], r["N"], r["K1"], r["Mw"]
    st = nv.current_stream()
    nt = gp._row(r["name"], r["why"], "nt", N, Co, gp._dense(M, Co), c=gp._batched(4, M // 4, N, 4, 8), epi=gp.EPI_ACCUM_RELU_MASK, env=env)
    tn = gp._tn_row(r["name"], r["why"], K1, Co, gp._dense(Mw, K1), env=env, accumulate=1, ldc_pad=4)
    dat, tdat = gp.make_rows_data(nt, ds), gp.make_tn_data(tn, ds)
    dy, w, dx, mk = _buf(dat["a_flat"]), _buf(dat["b_flat"]), _buf(dat["c_flat"]), _buf(dat["mask_flat"])
    x, dyw, dw, bg = _buf(tdat["a_flat"]), _buf(tdat["b_flat"]), _buf(tdat["c_flat"]), _buf(tdat["old_bg"])
    zrows, zpitch, zbatch = 8, 20, 3                               # the zero job: 3 runs of 8 zeros, 20 floats apart
    zb = _buf(np.full(zbatch * zpitch, np.nan, np.float32))
    pending = []
    wt = None
    if "w" in r["jobs"]:
        ws_tn_b = nv.lib.lidbox_gemm_tn_workspace(Mw, K1, Co)
        wt, wtp, wtn = _ws(ws_tn_b)
        job = nv.ReduceJob()
        nv.check(nv.lib.lidbox_gemm_tn_partial(_desc(nv, x, tn["a"]), _desc(nv, dyw, tn["b"]), dw.ptr, Co + 4, K1, Co, 1, bg.ptr, wtp, wtn,
                                               ctypes.byref(job), st))
        assert job.nblocks > 0, "the job form of the reduce (reduce_job_vec_ok)"
        pending.append(job)
    for _ in range(r["jobs"].count("z")):
        job = nv.ReduceJob()
        nv.check(nv.lib.lidbox_zero_job(zb.ptr, zpitch, zrows, zbatch, ctypes.byref(job)))
        pending.append(job)
    ws_nt_b = nv.lib.lidbox_gemm_rows_workspace(M, N, Co)
    wn, wnp, wnn = _ws(ws_nt_b)
    rc = nv.lib.lidbox_gemm_nt_carry(_desc(nv, dy, nt["a"]), w.ptr, Co, _desc(nv, dx, nt["c"]), Co, N, nt["epi"], mk.ptr, wnp, wnn,
                                     _job_array(nv, pending), len(pending), st)
    torch.cuda.synchronize()
    if not r["rc_ok"]:
        assert rc != 0
        assert _same(dx.numpy(), dat["c_flat"]) and _same(zb.numpy(), np.full(zbatch * zpitch, np.nan, np.float32)), "a refused call wrote"
        return None
    nv.check(rc)
    pred = gp.rows_dispatch(1, M, N, Co, True, ws_nt_b, env, nt["epi"], True, 4, M // 4, N + 4, (M // 4) * (N + 4) + 8)
    assert nv.lib.lidbox_gemm_last_family() == pred["family"] and _launches(nv) == pred["launches"]
    assert nv.lib.lidbox_gemm_last_carried() == (carried if pred["family"] in (1, 3) else 0), r["why"]
    ok, worst, what = gp.judge_rows(nt, ds, dat, dx.numpy(), pred["p"])
    _note("carry dgrad", ds, r["name"], worst)
    assert ok, (r["name"], ds, what, worst)
    if "w" in r["jobs"]:
        tp = gp.tn_dispatch(Mw, K1, Co, True, True, ws_tn_b, env, ldc=Co + 4)
        okt, worst_t, worst_g = gp.judge_tn(tn, ds, tdat, dw.numpy(), bg.numpy(), tp["splits"], tp["rps"])
        _note("carry wgrad", ds, r["name"], max(worst_t, worst_g))
        assert okt, (r["name"], ds, worst_t, worst_g)
        wt.check()
    want = np.full((zbatch, zpitch), np.nan, np.float32)
    if "z" in r["jobs"]:
        want[:, :zrows] = 0.0
    assert _same(zb.numpy(), want.ravel()), "the zero job"
    if wn is not None:
        wn.check()
    assert _same(dy.numpy(), dat["a_flat"]) and _same(x.numpy(), tdat["a_flat"]) and _same(dyw.numpy(), tdat["b_flat"])
    return dx.numpy().copy(), dw.numpy().copy(), bg.numpy().copy(), zb.numpy().copy()


@pytest.mark.parametrize("r", gp.PATHS["CARRY"], ids=[r["name"] for r in gp.PATHS["CARRY"]])
def test_carry_row(r, monkeypatch):
    """a wgrad's pending slice sum and a zero job handed to a dgrad launch: the dgrad, the wgrad and the zeroed runs against the
    oracle in guarded buffers, lidbox_gemm_last_carried against the row; carried against separate launches
    (LIDBOX_GEMM_NO_CARRY: the jobs run as a launch of their own behind the GEMM) bit for bit"""
    for ds in gp.DATASETS:
        got = run_carry(r, ds, r["env"], r["carried"], monkeypatch)
        assert (got is not None) == r["rc_ok"]
        if got is not None and "LIDBOX_GEMM_NO_CARRY" not in r["env"]:
            sep = run_carry(r, ds, dict(r["env"], LIDBOX_GEMM_NO_CARRY="1"), 0, monkeypatch)
            for a, b, what in zip(got, sep, ("dX", "dW", "bias gradient", "zeroed runs")):
                assert _same(a, b), "%s: carried and separate launches differ in %s" % (r["name"], what)
