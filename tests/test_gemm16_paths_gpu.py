"""
The bf16 GEMM families on their dispatch paths (oracle/gemm16_paths_np.py, PATHS): every row through the C ABI on the three data
sets, all inputs, outputs, shadows, masks and workspaces in Guarded buffers (tests/guarded.py) with NaN in every gap of the pitched
A, B, mask, C and shadow, workspaces of exactly the size the planner asks for.

Every row asserts
  - the predicted kernel, splits and m_main against lidbox_gemm_bf16_last_plan (and the tile against lidbox_gemm_bf16s_last_variant);
  - err / bound <= 1 per element against the float64 reference (bound: conv2d_np.error_bound(S, 2 K + p + e));
  - the shadow: C16 == bf16_rne(C) bit for bit beside an fp32 C, inside [bf16_rne(ref - bound), bf16_rne(ref + bound)] alone;
  - bit equality with the int64 result on `exact`;
  - untouched guard words, gap words and inputs; the same bits run to run.
Identities: first against last row block of M; storage against compute family on the same values; the pair call against the two calls;
lidbox_gemm_bf16s_tn against _tn_partial + lidbox_reduce_jobs_run; carried against separate launches; policy-selected against forced launch.
A wgrad workspace one byte short, or any workspace 4 bytes off alignment, is refused and nothing is written; a rows workspace one byte
short is no refusal in these families: the planner steps the split down (plan_rows16, choose_dma16), and the test checks that plan.
The BIG16S / BIGTN16S / PAIR16S rows (policy branches that need about 192 tiles of 256 x 256, the tail split, the pair grid) are judged on
sampled rows / columns against float64 and bit for bit against a second launch of known path; one case per data set.

One run on one MI355X: 334 cases (178 rows, 2 + 3 workspace cases, 14 row-block identities, 8 storage-against-compute identities -- one
per epilogue --, 24 + 6 wgrads, 30 big-row and 24 pair cases, 9 carry rows, 36 converter rows), 94 s for the module, 3.4 s for
its slowest case (the small rows alone: 8 s).  Largest err / bound per kernel: 0.087
gemm16s_rows_dma_kernel<128,64,2>, 0.083 / 0.082 / 0.067 / 0.053 gemm16s_rows_pp_kernel<256,1> / <128,2> / <256,2> / <128,1>, 0.075
gemm16s_rows_kernel, 0.073 dma<64,128,2>, 0.072 / 0.068 / 0.062 dma<64,64,3> / <64,64,4> / <64,64,2>, 0.052 / 0.049 dma<128,128,2> / <128,128,3>,
0.051 dma<64,128,3>, 0.049 dma<128,64,3>, 0.048 gemm16s_rows_kres_kernel<0>, 0.004 <13>, 0.019 gemm16_rows_kernel (both), 0.019
gemm16_tn_kernel, 0.016 gemm16s_tn_kres_kernel, 0.005 gemm16s_tn_kernel and gemm16s_tn_pp_kernel, at most 0.009 through
rows_reduce_kernel, 0.008 on the policy-selected ping-pong tile and the pair grid, 0.002 on the policy-selected ping-pong wgrad; every `exact` case bit-equal in fp32 and in the shadow (docs/LAB_NOTEBOOK.md, section 24).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import gemm_paths_np as gp
from oracle import gemm16_paths_np as g
from tests.guarded import Guarded

pytestmark = pytest.mark.gpu

WORST = {}                                           # (kernel, data set) -> largest err / bound seen (printed by every case)


def _nv():
    from lidbox_amd import _native as nv
    return nv


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a device fault is sticky: nothing of this module runs after one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault, stopping the module: %s" % e, returncode=3)


def _setenv(monkeypatch, env):
    for k in list(os.environ):
        if k.startswith("LIDBOX_GEMM"):
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _buf(flat, shift=0):
    flat = np.ascontiguousarray(flat, np.float32).ravel()
    b = Guarded((flat.size,), init=torch.from_numpy(flat), shift=shift)
    assert b.view.data_ptr() % 16 == 4 * shift
    return b


class Buf16:
    """a flat array of bf16 VALUES (NaN included) as a guarded bfloat16 device buffer; `shift` elements of NaN in front of the payload
    move it off its alignment (they must stay NaN)"""

    def __init__(self, flat, shift=0):
        flat = np.ascontiguousarray(flat, np.float32).ravel()
        bits = g.bf16_bits(flat)
        assert np.array_equal(g.bf16_widen(bits), flat, equal_nan=True), "not bf16 values"
        self.g = Guarded((flat.size + shift,), dtype=torch.bfloat16)
        self.shift, self.n, self.src_bits = shift, flat.size, bits
        self.g.view.view(torch.int16)[shift:].copy_(torch.from_numpy(bits.view(np.int16)))                   # bits, so that NaN stays 0x7FC0
        self.addr = self.g.view.data_ptr() + 2 * shift
        self.ptr = ctypes.c_void_p(self.addr)

    def bits(self):
        """uint16 bits of the payload, after checking the guard words and the shift elements"""
        self.g.check()
        raw = self.g.view.view(torch.int16).cpu().numpy().view(np.uint16)
        assert (raw[:self.shift] == g.NAN16).all(), "the elements in front of a shifted payload were written"
        return raw[self.shift:].copy()

    def unchanged(self):
        return np.array_equal(self.bits(), self.src_bits)


def _ws(nbytes, aligned=True):
    """a workspace of exactly nbytes whose fp32 words all start as NaN; not aligned: 4 bytes past a 16-byte boundary"""
    if nbytes <= 0:
        return None, None, 0
    w = Guarded((nbytes + (0 if aligned else 4),), dtype=torch.uint8)
    nan = torch.tensor([0x00, 0x00, 0xC0, 0x7F], dtype=torch.uint8, device="cuda")
    w.view.copy_(nan.repeat(w.n // 4 + 1)[:w.n])
    p = w.view.data_ptr() + (0 if aligned else 4)
    assert p % 16 == (0 if aligned else 4)
    return w, ctypes.c_void_p(p), nbytes


def _note(group, ds, what, worst):
    key = (group, ds)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-44s %-6s max err/bound=%.3e   [%s so far %.3e]" % (what, ds, worst, group, WORST[key]))


def _desc(nv, addr, d):
    return nv.Rows(addr, d["bs"], d["rs"], d["batch"], d["rpb"])


def _last_plan(nv):
    out = (ctypes.c_long * 4)()
    nv.check(nv.lib.lidbox_gemm_bf16_last_plan(out))
    return list(out)


def _last_variant(nv):
    out = (ctypes.c_int * 3)()
    nv.check(nv.lib.lidbox_gemm_bf16s_last_variant(out))
    return list(out)


# ---------------------------------------------------------------------------------------------------------- rows
def run_rows(r, dat, wsb=None, ws_aligned=True):
    """one rows call of a ROWS16 / ROWS16S row in guarded buffers -> (rc, flat C or None, shadow bits or None)"""
    nv = _nv()
    sto = r["fam"] == "s"
    res = r["res"]
    if sto:
        a, b = Buf16(dat["a_flat"], res.get("A", 0) // 2), Buf16(dat["b_flat"], res.get("B", 0) // 2)
        a_addr, b_addr = a.addr, b.addr
    else:
        a, b = _buf(dat["a_flat"], res.get("A", 0) // 4), _buf(dat["b_flat"], res.get("B", 0) // 4)
        a_addr, b_addr = a.view.data_ptr(), b.view.data_ptr()
    c = _buf(dat["c_flat"], res.get("C", 0) // 4)
    c16 = Buf16(np.full(dat["c_flat"].size, np.nan, np.float32), res.get("C16", 0) // 2) if (sto and r["out"] != "f32") else None
    aux, aux_src = None, None
    if r["epi"] in gp.EPI_HAS_BIAS:
        aux, aux_src = _buf(dat["bias"]), dat["bias"]
    elif r["epi"] in gp.EPI_HAS_MASK:
        aux_src = dat["mask_flat"]
        aux = Buf16(aux_src) if r["mask16"] else _buf(aux_src)
    wsb = g.row_ws_bytes(r) if wsb is None else wsb
    wsg, wsp, wsn = _ws(wsb, ws_aligned)
    cd = _desc(nv, None if r["out"] == "shadow" else c.view.data_ptr(), r["c"])
    st = nv.current_stream()
    if sto:
        rc = nv.lib.lidbox_gemm_bf16s_nt(_desc(nv, a_addr, r["a"]), ctypes.c_void_p(b_addr), g.ldb_of(r), cd, c16.ptr if c16 is not None else None, r["K"], r["N"],
                                        r["epi"] | (g.EPI_MASK_BF16 if r["mask16"] else 0), aux.ptr if aux is not None else None, wsp, wsn, st)
    else:
        fn = nv.lib.lidbox_gemm_bf16_nn if r["kind"] == "nn" else nv.lib.lidbox_gemm_bf16_nt
        rc = fn(_desc(nv, a_addr, r["a"]), ctypes.c_void_p(b_addr), g.ldb_of(r), cd, r["K"], r["N"], r["epi"], aux.ptr if aux is not None else None, wsp, wsn, st)
    torch.cuda.synchronize()
    got_c = c.numpy().copy()                                       # checks the guard words around C
    got_s = c16.bits() if c16 is not None else None
    if sto:
        assert a.unchanged() and b.unchanged(), "an input changed"
    else:
        assert _same(a.numpy(), dat["a_flat"].ravel()) and _same(b.numpy(), dat["b_flat"].ravel()), "an input changed"
    if aux is not None:
        assert aux.unchanged() if isinstance(aux, Buf16) else _same(aux.numpy(), np.ravel(aux_src)), "bias / mask changed"
    if wsg is not None:
        wsg.check()
    if r["out"] == "shadow":
        assert _same(got_c, dat["c_flat"]), "C.base == NULL, yet the fp32 buffer of the test changed"
        got_c = None
    return rc, got_c, got_s


def _group(r, q):
    kind = g.Q16_NT if r["kind"] == "nt" else g.Q16_NN
    return (g.kernel_name(q, kind) or "none") + ("+reduce" if q[9] == g.R_ROWS else "")


ROWS = g.PATHS["ROWS16"] + g.PATHS["ROWS16S"]


@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_rows_row(r, monkeypatch):
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    q = g.row_query(r)
    for ds in g.DATASETS:
        dat = g.make_rows_data(r, ds)
        rc, got_c, got_s = run_rows(r, dat)
        if q[0] == g.K_REFUSED:
            assert rc != 0 and _same(got_c, dat["c_flat"]), "a refused call wrote"
            continue
        nv.check(rc)
        assert _last_plan(nv) == [q[0], q[4], q[5], q[6]], (r["why"], _last_plan(nv), q)
        if r["fam"] == "s":
            assert _last_variant(nv) == (q[1:4] if q[0] != g.KS_ROWS else [0, 0, 0]), (r["why"], _last_variant(nv), q)
        ok, worst, what = g.judge_rows(r, ds, dat, got_c, got_s, max(q[4], q[7]))
        _note(_group(r, q), ds, r["name"], worst)
        assert ok, "%s [%s] %s: worst err/bound %.3g (%s)" % (r["name"], ds, what, worst, r["why"])
        if ds == "normal":
            _, again_c, again_s = run_rows(r, dat)
            assert (got_c is None or _same(got_c, again_c)) and (got_s is None or np.array_equal(got_s, again_s)), "not bit-identical run to run"


WS_CASES = [r for r in ROWS if r["name"] in ("tile-64.64.2-split3-short", "c-nt-130x132x136-lib")]


@pytest.mark.parametrize("r", WS_CASES, ids=[r["name"] for r in WS_CASES])
def test_rows_workspace_short_and_misaligned(r, monkeypatch):
    """one byte short: the planner steps the split down and the result still holds (the rows families size their own split);
    4 bytes off a 16-byte boundary: refused, nothing written"""
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    dat = g.make_rows_data(r, "normal")
    wsb = g.row_ws_bytes(r)
    q_full, q_short = g.row_query(r, wsb), g.row_query(r, wsb - 1)
    assert q_short[4] < q_full[4]
    rc, got_c, got_s = run_rows(r, dat, wsb - 1)
    nv.check(rc)
    assert _last_plan(nv)[1] == q_short[4]
    ok, worst, what = g.judge_rows(r, "normal", dat, got_c, got_s, q_short[4])
    assert ok, (what, worst)
    rc, got_c, got_s = run_rows(r, dat, wsb, ws_aligned=False)
    assert rc != 0 and (got_c is None or _same(got_c, dat["c_flat"])) and (got_s is None or (got_s == g.NAN16).all()), "a refused call wrote"


PLACE = [(bm, bn, st) for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]]


@pytest.mark.parametrize("tile", PLACE, ids=["%d.%d.%d" % t for t in PLACE])
def test_first_and_last_row_block_give_the_same_bits(tile, monkeypatch):
    """the same rows of A as the first and as the last row block of M (a ragged block between them): the same bits in C and the shadow"""
    bm, bn, st = tile
    ebm = bm or 128
    env = {"LIDBOX_GEMM16S_DMA": "0" if bm == 0 else "%d,%d,%d" % tile}
    M = 2 * ebm + 40
    r = g._row("ROWS16S", "place-%d.%d.%d" % tile, "row block 0 against the last", "s", "nt", 72, 200, gp._dense(M, 200, 8), c=gp._dense(M, 72, 4), epi=gp.EPI_BIAS_RELU,
               out="both", env=env, ws="none")
    _setenv(monkeypatch, env)
    dat = g.make_rows_data(r, "normal")
    idx = gp.index(r["a"], 200)
    dat["a_flat"][idx[M - ebm:]] = dat["a_flat"][idx[:ebm]]
    dat["A"] = gp.gather(dat["a_flat"], r["a"], 200)
    rc, got_c, got_s = run_rows(r, dat)
    _nv().check(rc)
    ok, worst, what = g.judge_rows(r, "normal", dat, got_c, got_s, 1)
    assert ok, (what, worst)
    ci = gp.index(r["c"], 72)
    C, S = got_c[ci], got_s[ci]
    assert _same(C[:ebm], C[M - ebm:]) and np.array_equal(S[:ebm], S[M - ebm:])


# ---------------------------------------------------------------------------------------------------------- wgrads
def run_tn(r, dat, partial=False, wsb=None, ws_aligned=True):
    """one wgrad call in guarded buffers -> (rc, dW [K1, ldc], bias gradient, job.nblocks)"""
    nv = _nv()
    sto = r["fam"] == "s"
    res = r["res"]
    if sto:
        a, b = Buf16(dat["a_flat"]), Buf16(dat["b_flat"])
        a_addr, b_addr = a.addr, b.addr
    else:
        a, b = _buf(dat["a_flat"]), _buf(dat["b_flat"])
        a_addr, b_addr = a.view.data_ptr(), b.view.data_ptr()
    c = _buf(dat["c_flat"], res.get("C", 0) // 4)
    bg = _buf(dat["old_bg"]) if r["bias_grad"] else None
    wsb = g.tn_row_ws_bytes(r) if wsb is None else wsb
    wsg, wsp, wsn = _ws(wsb, ws_aligned)
    st = nv.current_stream()
    K1, N = r["K1"], r["N"]
    args = (_desc(nv, a_addr, r["a"]), _desc(nv, b_addr, r["b"]), c.ptr, N + r["ldc_pad"], K1, N, r["accumulate"], bg.ptr if bg is not None else None, wsp, wsn)
    nblocks = -1
    if not sto:
        rc = nv.lib.lidbox_gemm_bf16_tn(*args, st)
    elif not partial:
        rc = nv.lib.lidbox_gemm_bf16s_tn(*args, st)
    else:
        job = nv.ReduceJob()
        rc = nv.lib.lidbox_gemm_bf16s_tn_partial(*args, ctypes.byref(job), st)
        nblocks = job.nblocks
        if rc == 0 and job.nblocks:
            nv.check(nv.lib.lidbox_reduce_jobs_run(ctypes.byref(job), 1, st))
    torch.cuda.synchronize()
    got_c = c.numpy().copy()
    got_bg = bg.numpy().copy() if bg is not None else None
    if sto:
        assert np.array_equal(a.bits(), g.bf16_bits(dat["a_flat"])) and np.array_equal(b.bits(), g.bf16_bits(dat["b_flat"])), "an input changed"
    else:
        assert _same(a.numpy(), dat["a_flat"].ravel()) and _same(b.numpy(), dat["b_flat"].ravel()), "an input changed"
    if wsg is not None:
        wsg.check()
    return rc, got_c, got_bg, nblocks


TN = g.PATHS["TN16"] + g.PATHS["TN16S"]


@pytest.mark.parametrize("r", TN, ids=[r["name"] for r in TN])
def test_tn_row(r, monkeypatch):
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    q = g.tn_row_query(r)
    plan = g.tn_row_plan(r, q)
    want_plan = [q[0], q[4], q[11] if q[0] == g.KS_TN_KRES else q[5], 0]
    for ds in g.DATASETS:
        dat = g.make_tn_data(r, ds)
        rc, got_c, got_bg, _ = run_tn(r, dat)
        nv.check(rc)
        assert _last_plan(nv) == want_plan, (r["why"], _last_plan(nv), q)
        if r["fam"] == "s":
            assert nv.lib.lidbox_gemm_bf16s_tn_last_pp() == (q[4] if q[0] == g.KS_TN_PP else 0) and nv.lib.lidbox_gemm_bf16s_tn_last_kres() == (q[4] if q[0] == g.KS_TN_KRES else 0)
        ok, worst, worst_g = g.judge_tn(r, ds, dat, got_c, got_bg, plan["pieces"], plan["per"])
        _note(g.kernel_name(q), ds, r["name"], max(worst, worst_g))
        assert ok, "%s [%s]: worst err/bound %.3g, bias gradient %.3g (%s)" % (r["name"], ds, worst, worst_g, r["why"])
        if r["fam"] == "s" and ds == "normal":                      # tn == tn_partial + lidbox_reduce_jobs_run, bit for bit
            rc, c2, bg2, nblocks = run_tn(r, dat, partial=True)
            nv.check(rc)
            assert (nblocks == 0) == (q[9] == g.R_SCALAR), "job.nblocks == 0 exactly where the scalar reduce ran inside the call"
            assert _same(got_c, c2) and (got_bg is None or _same(got_bg, bg2))


TN_WS = [r for r in TN if r["name"] in ("c-tn-300x132x136", "s-tn-two", "s-tn-kres")]


@pytest.mark.parametrize("r", TN_WS, ids=[r["name"] for r in TN_WS])
def test_tn_workspace_short_and_misaligned(r, monkeypatch):
    """a workspace one byte short of the slices, or 4 bytes off a 16-byte boundary, is refused and nothing is written (the K1-resident
    kernel's own workspace one byte short falls back to the four-wave kernel, which needs less)"""
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    dat = g.make_tn_data(r, "normal")
    q = g.tn_row_query(r)
    need = (q[4] * r["K1"] * r["N"] + q[4] * r["N"]) * 4
    short = g.tn_row_query(r, need - 1)
    rc, got_c, got_bg, _ = run_tn(r, dat, wsb=need - 1)
    if short[10]:                                                   # the fallback fits
        assert q[0] == g.KS_TN_KRES and short[0] == g.KS_TN
        nv.check(rc)
        assert _last_plan(nv)[0] == g.KS_TN
    else:
        assert rc != 0 and _same(got_c, dat["c_flat"].ravel()) and (got_bg is None or _same(got_bg, dat["old_bg"])), "a refused call wrote"
    rc, got_c, got_bg, _ = run_tn(r, dat, wsb=need, ws_aligned=False)
    assert rc != 0 and _same(got_c, dat["c_flat"].ravel()) and (got_bg is None or _same(got_bg, dat["old_bg"])), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------- carry
def _job_array(nv, jobs):
    arr = (nv.ReduceJob * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = j
    return arr


def run_carry(r, ds, env, monkeypatch):
    """the storage wgrad's partial launch, the zero jobs and the carrying lidbox_gemm_bf16s_nt_carry call of a CARRY16S row under `env`,
    judged against the oracle -> (dX, dX shadow, dW, bias gradient, zeroed runs, carried)"""
    nv = _nv()
    _setenv(monkeypatch, env)
    M, Co, N, K1, Mw = r["M"], r["Co"], r["N"], r["K1"], r["Mw"]
    st = nv.current_stream()
    ws = "none" if r["nows"] else "plan"
    if r["kres"]:                                                   # windows the K-resident kernel takes when nothing is carried; a store-only epilogue, no mask
        nt = g._row("CARRY16S", r["name"], r["why"], "s", "nt", N, Co, dict(batch=4, rpb=M // 4, rs=8, bs=(M // 4 - 1) * 8 + Co + 8), c=gp._batched(4, M // 4, N, 4, 8),
                    epi=gp.EPI_BIAS, out="both", env=env, ws=ws)
    else:
        nt = g._row("CARRY16S", r["name"], r["why"], "s", "nt", N, Co, gp._dense(max(M, 4), Co), c=gp._batched(4, max(M, 4) // 4, N, 4, 8), epi=gp.EPI_ACCUM_RELU_MASK,
                    out="both", mask16=True, env=env, ws=ws)
    tn = g._tn_row("CARRY16S", r["name"], r["why"], "s", K1, Co, gp._dense(Mw, K1), env=env, accumulate=1, ldc_pad=4)
    dat, tdat = g.make_rows_data(nt, ds), g.make_tn_data(tn, ds)
    dy, w, dx = Buf16(dat["a_flat"]), Buf16(dat["b_flat"]), _buf(dat["c_flat"])
    mk = Buf16(dat["mask_flat"]) if nt["mask16"] else _buf(dat["bias"])
    flags = nt["epi"] | (g.EPI_MASK_BF16 if nt["mask16"] else 0)
    dx16 = Buf16(np.full(dat["c_flat"].size, np.nan, np.float32))
    x, dyw, dw, bg = Buf16(tdat["a_flat"]), Buf16(tdat["b_flat"]), _buf(tdat["c_flat"]), _buf(tdat["old_bg"])
    zrows, zpitch, zbatch = 8, 20, 3                               # the zero job: 3 runs of 8 zeros, 20 floats apart
    zb = _buf(np.full(zbatch * zpitch, np.nan, np.float32))
    pending, wt = [], None
    if "w" in r["jobs"]:
        wt, wtp, wtn = _ws(g.tn_row_ws_bytes(tn))
        job = nv.ReduceJob()
        nv.check(nv.lib.lidbox_gemm_bf16s_tn_partial(_desc(nv, x.addr, tn["a"]), _desc(nv, dyw.addr, tn["b"]), dw.ptr, Co + 4, K1, Co, 1, bg.ptr, wtp, wtn, ctypes.byref(job), st))
        assert job.nblocks > 0, "the job form of the reduce (reduce_job_vec_ok)"
        pending.append(job)
    for _ in range(r["jobs"].count("z")):
        job = nv.ReduceJob()
        nv.check(nv.lib.lidbox_zero_job(zb.ptr, zpitch, zrows, zbatch, ctypes.byref(job)))
        pending.append(job)
    q = g.plan_query(g.Q16S_NT, nt["a"], None, nt["c"], Co, N, nt["epi"], env, g.row_ws_bytes(nt), has_ws=not r["nows"], mask16=nt["mask16"], njobs=len(pending), ldb=Co)
    if r["kres"]:                                                   # the job alone keeps the call off the K-resident kernel
        alone = g.plan_query(g.Q16S_NT, nt["a"], None, nt["c"], Co, N, nt["epi"], env, 0, has_ws=False, njobs=0, ldb=Co)
        carries = "LIDBOX_GEMM_NO_CARRY" not in env
        assert alone[0] == g.KS_KRES0 and (q[0] == g.KS_DMA) == carries and (q[0] == g.KS_KRES0) == (not carries), (alone, q)
    wn, wnp, wnn = _ws(0 if r["nows"] else g.row_ws_bytes(nt))
    a_desc = _desc(nv, dy.addr, nt["a"]) if M else nv.Rows(dy.addr, 0, Co, 0, 5)
    c_desc = _desc(nv, dx.view.data_ptr(), nt["c"]) if M else nv.Rows(dx.view.data_ptr(), 0, N + 4, 0, 5)
    nv.check(nv.lib.lidbox_gemm_bf16s_nt_carry(a_desc, w.ptr, Co, c_desc, dx16.ptr, Co, N, flags, mk.ptr, wnp, wnn, _job_array(nv, pending), len(pending), st))
    torch.cuda.synchronize()
    carried = nv.lib.lidbox_gemm_bf16s_last_carried()
    if M:
        assert _last_plan(nv) == [q[0], q[4], q[5], q[6]], (r["why"], _last_plan(nv), q)
        ok, worst, what = g.judge_rows(nt, ds, dat, dx.numpy(), dx16.bits(), q[4])
        _note("carry dgrad", ds, r["name"], worst)
        assert ok, (r["name"], ds, what, worst)
    else:
        assert _last_plan(nv)[0] == g.K_NONE and _same(dx.numpy(), dat["c_flat"]) and (dx16.bits() == g.NAN16).all(), "M == 0 wrote C"
    if "w" in r["jobs"]:
        tq = g.tn_row_query(tn)
        okt, worst_t, worst_g = g.judge_tn(tn, ds, tdat, dw.numpy(), bg.numpy(), tq[4], tq[5])
        _note("carry wgrad", ds, r["name"], max(worst_t, worst_g))
        assert okt, (r["name"], ds, worst_t, worst_g)
        wt.check()
    want = np.full((zbatch, zpitch), np.nan, np.float32)
    if "z" in r["jobs"]:
        want[:, :zrows] = 0.0
    assert _same(zb.numpy(), want.ravel()), "the zero job"
    if wn is not None:
        wn.check()
    assert np.array_equal(dy.bits(), g.bf16_bits(dat["a_flat"])) and np.array_equal(x.bits(), g.bf16_bits(tdat["a_flat"]))
    return dx.numpy().copy(), dx16.bits(), dw.numpy().copy(), bg.numpy().copy(), zb.numpy().copy(), carried


@pytest.mark.parametrize("r", g.PATHS["CARRY16S"], ids=[r["name"] for r in g.PATHS["CARRY16S"]])
def test_carry_row(r, monkeypatch):
    """pending jobs handed to a storage dgrad launch: the dgrad, its shadow, the wgrad and the zeroed runs against the oracle in guarded
    buffers, lidbox_gemm_bf16s_last_carried against the row; carried against separate launches (LIDBOX_GEMM_NO_CARRY) bit for bit.
    carry-zero-nows is the call lidbox_gemm_bf16s_nt_carry used to refuse (a zero job's NULL slices compared equal to a NULL workspace)."""
    for ds in g.DATASETS:
        got = run_carry(r, ds, r["env"], monkeypatch)
        assert got[5] == r["carried"], (r["why"], got[5])
        if "LIDBOX_GEMM_NO_CARRY" not in r["env"]:
            sep = run_carry(r, ds, dict(r["env"], LIDBOX_GEMM_NO_CARRY="1"), monkeypatch)
            assert sep[5] == 0
            for a, b, what in zip(got[:5], sep[:5], ("dX", "dX shadow", "dW", "bias gradient", "zeroed runs")):
                if r["kres"] and what.startswith("dX"):             # without the job the K-resident kernel runs the dgrad: another summation order
                    continue
                assert np.array_equal(a, b, equal_nan=True) if a.dtype == np.uint16 else _same(a, b), "%s: carried and separate launches differ in %s" % (r["name"], what)


# ---------------------------------------------------------------------------------------------------------- big rows
BIG = g.PATHS["BIG16S"]
BIG_CASES = [(r, ds) for r in BIG for ds in ((r["ds"],) if r["ds"] else g.DATASETS)]


def _judge_sampled(r, ds, dat, got_c, got_s, q):
    rows = g.sample_rows(r["M"], edges=(q[6],) if q[6] else (), seed=r["M"] + r["K"])
    if q[6] and r["M"] - q[6] <= 256:
        rows = np.union1d(rows, np.arange(q[6], r["M"]))
    return g.judge_rows(r, ds, dat, got_c, got_s, max(q[4], q[7]), rows=rows)


@pytest.mark.parametrize("r,ds", BIG_CASES, ids=["%s-%s" % (r["name"], ds) for r, ds in BIG_CASES])
def test_big_row(r, ds, monkeypatch):
    """choose_dma16's policy branches and the tail split at the smallest shapes that take them: the predicted kernel, splits and m_main,
    sampled rows against float64 (g.sample_rows; every gap and guard word whole), and the whole output bit for bit against the same
    call under the forced variant -- for a tail split: the rows in front of m_main against the call without a workspace (one launch)"""
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    q = g.row_query(r)
    dat = g.make_rows_data(r, ds)
    rc, got_c, got_s = run_rows(r, dat)
    nv.check(rc)
    assert _last_plan(nv) == [q[0], q[4], q[5], q[6]], (r["why"], _last_plan(nv), q)
    if r["fam"] == "s":
        assert _last_variant(nv) == (q[1:4] if q[0] != g.KS_ROWS else [0, 0, 0]), (r["why"], _last_variant(nv), q)
    ok, worst, what = _judge_sampled(r, ds, dat, got_c, got_s, q)
    _note(_group(r, q) + (" tail" if q[6] else ""), ds, r["name"], worst)
    assert ok, "%s [%s] %s: worst err/bound %.3g (%s)" % (r["name"], ds, what, worst, r["why"])
    if r["twin_env"]:
        _setenv(monkeypatch, r["twin_env"])
        tq = g.row_query(r)
        assert tq[:6] == q[:6], "the forced variant is the same launch"
        rc, c2, s2 = run_rows(r, dat)
        nv.check(rc)
        assert (got_c is None or _same(got_c, c2)) and (got_s is None or np.array_equal(got_s, s2)), "policy-selected and forced launch differ"
    elif q[6]:
        rc, c2, s2 = run_rows(r, dat, wsb=0)
        nv.check(rc)
        assert _last_plan(nv)[3] == 0
        n = q[6] * r["N"]
        assert _same(got_c[:n], c2[:n]) and (got_s is None or np.array_equal(got_s[:n], s2[:n])), "rows in front of m_main differ from the single launch"
        okw, worst, what = _judge_sampled(r, ds, dat, c2, s2, [q[0], 0, 0, 0, 1, 0, 0, 0])
        assert okw, (what, worst)


BIGTN = g.PATHS["BIGTN16S"]


@pytest.mark.parametrize("r", BIGTN, ids=[r["name"] for r in BIGTN])
@pytest.mark.parametrize("ds", g.DATASETS)
def test_big_tn_row(r, ds, monkeypatch):
    """the ping-pong wgrad tile selected by policy (and one slice length short of it): 64 sampled output columns and the whole bias gradient"""
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    q = g.tn_row_query(r)
    plan = g.tn_row_plan(r, q)
    dat = g.make_tn_data(r, ds)
    rc, got_c, got_bg, _ = run_tn(r, dat)
    nv.check(rc)
    assert _last_plan(nv) == [q[0], q[4], q[5], 0] and nv.lib.lidbox_gemm_bf16s_tn_last_pp() == (q[4] if q[0] == g.KS_TN_PP else 0), (r["why"], _last_plan(nv), q)
    cols = np.unique(np.concatenate([[0, 255, 256, r["N"] - 1], np.random.default_rng(5).integers(0, r["N"], 60)]))
    ok, worst, worst_g = g.judge_tn(r, ds, dat, got_c, got_bg, plan["pieces"], plan["per"], cols=cols)
    _note(g.kernel_name(q) + " policy", ds, r["name"], max(worst, worst_g))
    assert ok, "%s [%s]: worst err/bound %.3g, bias gradient %.3g (%s)" % (r["name"], ds, worst, worst_g, r["why"])


# ---------------------------------------------------------------------------------------------------------- pair
def run_pair(r, ds, env, monkeypatch, paired=True, dats=None):
    """lidbox_gemm_bf16s_nt_pair_carry on a PAIR16S row (paired=False: the two lidbox_gemm_bf16s_nt calls one after the other, the zero job
    through lidbox_reduce_jobs_run) -> ([C0, shadow0, shadow1, zeroed runs], last_pair, last_carried); sampled rows against float64"""
    nv = _nv()
    _setenv(monkeypatch, env)
    st = nv.current_stream()
    probs = (r["p0"], r["p1"])
    dats = [g.make_rows_data(p_, ds) for p_ in probs] if dats is None else dats
    bufs = []
    for p_, d in zip(probs, dats):
        bufs.append(dict(a=Buf16(d["a_flat"]), b=Buf16(d["b_flat"]), c=_buf(d["c_flat"]), s=Buf16(np.full(d["c_flat"].size, np.nan, np.float32)), bias=_buf(d["bias"])))
    zb = _buf(np.full(60, np.nan, np.float32))
    jobs = []
    if r["zero"]:
        job = nv.ReduceJob()
        nv.check(nv.lib.lidbox_zero_job(zb.ptr, 20, 8, 3, ctypes.byref(job)))
        jobs.append(job)
    wsg, wsp, wsn = _ws(2 * max(p_["M"] * p_["N"] for p_ in probs) * 4 if r["ws"] else 0)
    args = []
    for p_, b in zip(probs, bufs):
        da, dc = (dict(p_["a"], batch=0), dict(p_["c"], batch=0, rpb=p_["a"]["rpb"])) if p_.get("empty") else (p_["a"], p_["c"])
        cd = _desc(nv, None if p_["out"] == "shadow" else b["c"].view.data_ptr(), dc)
        args.append([_desc(nv, b["a"].addr, da), b["b"].ptr, p_["K"], cd, b["s"].ptr, p_["K"], p_["N"], p_["epi"], b["bias"].ptr])
    if paired:
        nv.check(nv.lib.lidbox_gemm_bf16s_nt_pair_carry(*args[0], *args[1], wsp, wsn, _job_array(nv, jobs), len(jobs), st))
        pair, carried = nv.lib.lidbox_gemm_bf16s_last_pair(), nv.lib.lidbox_gemm_bf16s_last_carried()
    else:
        for p_, a_ in zip(probs, args):
            nv.check(nv.lib.lidbox_gemm_bf16s_nt(*a_, wsp, wsn, st))
            assert _last_plan(nv)[0] == (g.K_NONE if p_.get("empty") else g.row_query(p_, wsn)[0]), (p_["name"], _last_plan(nv))
        if jobs:
            nv.check(nv.lib.lidbox_reduce_jobs_run(_job_array(nv, jobs), len(jobs), st))
        pair, carried = 0, 0
    torch.cuda.synchronize()
    outs = []
    for p_, d, b in zip(probs, dats, bufs):
        got_c, got_s = b["c"].numpy().copy(), b["s"].bits()
        if p_["out"] == "shadow":
            assert _same(got_c, d["c_flat"])
            got_c = None
        if p_.get("empty"):
            assert (got_s == g.NAN16).all(), "a problem without rows wrote"
            outs.append(got_s)
            continue
        q = g.row_query(p_, wsn)
        ok, worst, what = _judge_sampled(p_, ds, d, got_c, got_s, q)
        _note("pair grid" if pair else "pair as two calls", ds, p_["name"], worst)
        assert ok, (p_["name"], ds, what, worst)
        assert b["a"].unchanged() and b["b"].unchanged(), "an input changed"
        outs += [got_c, got_s] if got_c is not None else [got_s]
    want = np.full((3, 20), np.nan, np.float32)
    if r["zero"]:
        want[:, :8] = 0.0
    assert _same(zb.numpy(), want.ravel()), "the zero job"
    if wsg is not None:
        wsg.check()
    return outs + [zb.numpy().copy()], pair, carried, dats


PAIR_CASES = [(r, ds) for r in g.PATHS["PAIR16S"] for ds in g.DATASETS]


@pytest.mark.parametrize("r,ds", PAIR_CASES, ids=["%s-%s" % (r["name"], ds) for r, ds in PAIR_CASES])
def test_pair_row(r, ds, monkeypatch):
    """two problems through lidbox_gemm_bf16s_nt_pair_carry: one grid exactly where both pass pp2_problem (swap both ways; with a zero job
    and workspace == NULL, the call the entry point used to demote because the job's NULL slices compared equal to the NULL workspace),
    two calls where one condition fails alone -- and the same bits as the two calls one after the other either way"""
    got, pair, carried, dats = run_pair(r, ds, r["env"], monkeypatch)
    assert pair == (1 if r["pair"] else 0), (r["why"], pair)
    want_carried = 1 if (r["zero"] and "LIDBOX_GEMM_NO_CARRY" not in r["env"]) else 0
    assert carried == want_carried, (r["why"], carried)
    if r["pair"]:
        assert _last_plan(_nv())[0] == g.KS_PP and _last_variant(_nv()) == [256, 256, 2]
    else:                                                           # the second of the two calls ran last
        assert _last_plan(_nv())[0] == (g.K_NONE if r["p1"].get("empty") else g.row_query(r["p1"], 2 * r["p1"]["M"] * r["p1"]["N"] * 4 if r["ws"] else 0)[0])
    sep, _, _, _ = run_pair(r, ds, r["env"], monkeypatch, paired=False, dats=dats)
    for a, b in zip(got, sep):
        assert np.array_equal(a, b) if a.dtype == np.uint16 else _same(a, b), "%s: the pair call and the two calls differ" % r["name"]


# ---------------------------------------------------------------------------------------------------------- storage against compute
IDENT = [r for r in g.PATHS["ROWS16S"] if r["name"].startswith("tile-0.0.0-e")]              # the eight epilogues


@pytest.mark.parametrize("r", IDENT, ids=[r["name"] for r in IDENT])
def test_storage_family_equals_compute_family_on_the_same_values(r, monkeypatch):
    """the register-staged storage kernel on bf16 values and lidbox_gemm_bf16_nt on the same values held as fp32 (rounding them is the
    identity): the same fp32 output bit for bit -- both add the K steps in order into one fp32 accumulator per element.  A shadow-only row
    runs with its fp32 C as well here, and a bf16 mask goes to the compute call as fp32 values"""
    nv = _nv()
    _setenv(monkeypatch, r["env"])
    for ds in g.DATASETS:
        dat = g.make_rows_data(r, ds)
        rc, c_s, _ = run_rows(dict(r, out="both" if r["out"] == "shadow" else r["out"]), dat)
        nv.check(rc)
        assert _last_plan(nv)[0] == g.KS_ROWS
        rc, c_c, _ = run_rows(dict(r, fam="c", out="f32", mask16=False), dat)
        nv.check(rc)
        assert _last_plan(nv)[0] == g.K_ROWS
        assert _same(c_s, c_c), "%s [%s]: storage and compute family differ on the same values" % (r["name"], ds)


# ---------------------------------------------------------------------------------------------------------- converters
def _special_values(n, rng):
    """n fp32 values that hold ties, +-0, subnormals, +-inf, the largest finite float (rounds to inf) and NaN among normal draws"""
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(np.float32)
    sp = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 257.0, 259.0, 0.0, -0.0, 1e-40, -1e-40, 2.0 ** -133, np.inf, -np.inf, 3.4028235e38, -3.4028235e38,
                   np.nan, 1.0 + 2.0 ** -8 + 2.0 ** -20], np.float32)
    k = min(n, sp.size)
    x[rng.permutation(n)[:k]] = sp[:k] if n >= sp.size else sp[rng.permutation(sp.size)[:k]]
    return x


CONVERT = g.PATHS["CONVERT"]


@pytest.mark.parametrize("r", CONVERT, ids=[r["name"] for r in CONVERT])
def test_convert_row(r):
    """expected values are exact: torch.Tensor.bfloat16() (round to nearest even) and its exact widening"""
    nv = _nv()
    st = nv.current_stream()
    rng = np.random.default_rng(sum(map(ord, r["name"])))
    if r["kind"] == "convert":
        n = r["n"]
        x = _special_values(max(n, 1), rng)[:n] if n else np.zeros(0, np.float32)
        src = _buf(x if n else np.zeros(1, np.float32))
        dst = Guarded((max(n, 1),), dtype=torch.bfloat16)
        nv.check(nv.lib.lidbox_f32_to_bf16(src.ptr, dst.ptr, n, st))
        torch.cuda.synchronize()
        dst.check()
        got = dst.view.view(torch.int16).cpu().numpy().view(np.uint16)
        want = torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
        nan = np.isnan(x)
        assert np.array_equal(got[:n][~nan], want[~nan]) and (np.isnan(g.bf16_widen(got[:n][nan]))).all() and (got[n:] == g.NAN16).all()
        assert np.array_equal(got[:n][~nan], g.bf16_bits(x)[~nan])
        back = Guarded((max(n, 1),))
        nv.check(nv.lib.lidbox_bf16_to_f32(dst.ptr, back.ptr, n, st))
        torch.cuda.synchronize()
        wide = back.numpy()
        assert np.array_equal(_bits(wide[:n]), _bits(g.bf16_widen(got[:n]))) and (_bits(wide[n:]) == g.NAN_BITS).all()
    elif r["kind"] == "refresh":
        n, mats = g.refresh_layout(r)
        x = _special_values(max(n, 16), rng)[:n]
        src = _buf(x)
        flat16 = Guarded((n,), dtype=torch.bfloat16)
        arr = (nv.WeightShadow * max(1, len(mats)))()
        dsts = []
        for i, m in enumerate(mats):
            rows_d, cols_d = (m["cols"], m["rows"]) if m["transpose"] else (m["rows"], m["cols"])
            d = Guarded((rows_d * m["ld_dst"] + m["dst_shift"],), dtype=torch.bfloat16)
            dsts.append(d)
            arr[i] = nv.WeightShadow(m["offset"], m["rows"], m["cols"], d.view.data_ptr() + 2 * m["dst_shift"], m["ld_dst"], m["transpose"])
            assert ((d.view.data_ptr() + 2 * m["dst_shift"]) % 8 == 0) == (m["dst_shift"] % 4 == 0)
        nv.check(nv.lib.lidbox_refresh_bf16_weights(src.ptr, flat16.ptr if r["flat16"] else None, n, arr, len(mats), st))
        torch.cuda.synchronize()
        assert _same(src.numpy(), x), "the flat vector changed"
        flat16.check()
        got = flat16.view.view(torch.int16).cpu().numpy().view(np.uint16)
        want, nan = g.bf16_bits(x), np.isnan(x)
        if r["flat16"]:
            assert np.array_equal(got[~nan], want[~nan]) and np.isnan(g.bf16_widen(got[nan])).all()
            assert np.array_equal(got[~nan], torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16)[~nan])
        else:
            assert (got == g.NAN16).all(), "flat16 == NULL, yet a conversion was written"
        for m, d in zip(mats, dsts):
            d.check()
            raw = d.view.view(torch.int16).cpu().numpy().view(np.uint16)
            assert (raw[:m["dst_shift"]] == g.NAN16).all()
            rows_d, cols_d = (m["cols"], m["rows"]) if m["transpose"] else (m["rows"], m["cols"])
            img = raw[m["dst_shift"]:].reshape(rows_d, m["ld_dst"])
            srcm = x[m["offset"]:m["offset"] + m["rows"] * m["cols"]].reshape(m["rows"], m["cols"])
            srcm = srcm.T if m["transpose"] else srcm
            w_, n_ = g.bf16_bits(np.ascontiguousarray(srcm)), np.isnan(srcm)
            assert np.array_equal(img[:, :cols_d][~n_], w_[~n_]) and np.isnan(g.bf16_widen(img[:, :cols_d][n_])).all(), (r["name"], m)
            assert (img[:, cols_d:] == g.NAN16).all(), "the pad behind a destination row was written"
    else:
        R, C, ld_src, ld_dst = r["R"], r["C"], r["ld_src"], r["ld_dst"]
        x = np.full((R, ld_src), np.nan, np.float32)
        x[:, :C] = _special_values(R * C, rng).reshape(R, C)
        src = _buf(x)
        dst = Guarded((C, ld_dst), dtype=torch.bfloat16)
        nv.check(nv.lib.lidbox_transpose_f32_to_bf16(src.ptr, R, C, ld_src, dst.ptr, ld_dst, st))
        torch.cuda.synchronize()
        dst.check()
        got = dst.view.view(torch.int16).cpu().numpy().view(np.uint16)
        want = g.bf16_bits(x[:, :C].T.copy())
        nan = np.isnan(x[:, :C].T)
        assert np.array_equal(got[:, :R][~nan], want[~nan]) and np.isnan(g.bf16_widen(got[:, :R][nan])).all() and (got[:, R:] == g.NAN16).all()
