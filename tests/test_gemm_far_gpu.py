"""
The fp32 and bf16 GEMM families on both sides of their 32-bit extent guards, through the C ABI, with operands whose last row lies
up to 5.2 GB behind their base.  fp32 first: sk_extent_ok, sk_b_extent_ok, reduce_job_vec_ok's byte limit, the inner test of
store_rows_tile.

The rows are PATHS["FAR"] of oracle/gemm_paths_np.py: a few-MFLOP problem put across a limit by stretching one stride (batch_stride,
row_stride or ldb) into a zone of the guard's own expression -- `high` (the largest byte offset dereferenced is at least 3.9e9, above
2^31, and the guard still holds), `edge-in` / `edge-out` (the two neighbouring aligned strides around the limit), `over` (1.05 L and
the call must fall to the register-staged kernels, family 0) -- and the C-far rows, where A and B are compact and C (with its mask and
old values) reaches 4.6e9 .. 5.2e9 bytes: no guard looks at C, the kernels stay on their fast path.  tests/test_oracle_gemm_paths.py
proves on the CPU that every row lies in its zone, selects what it names, and that every planted addressing mistake (sign extension,
truncation mod 2^32, a byte limit counted in elements, wrap32 beyond 2^30) turns into a wrong number inside the allocation.

Buffers (tests/far_buffers.py): every matrix operand lives in a module-scoped arena [2^31 + 256 bytes][extent][256 bytes] filled
with NaN, the payload written and read through an as_strided view; four arenas (A / X, B / dY, C, mask), 25.9 GiB together; the
module asserts the free device memory covers them and fails -- not skips -- if it does not.  After every call, on the device: each
input arena holds exactly its payload words, bit-identical; C's arena holds exactly M x N changed words (its payload, read back
through the descriptor); the workspace's guard words are untouched.

Judging: lidbox_gemm_last_family and lidbox_gemm_last_launches equal the oracle's prediction (a mismatch fails, no row skips); the
payload is inside the bounds of judge_rows / judge_tn (err / bound <= 1) on `normal` and bit-equal to int64 on `exact`; a `high`,
`edge-in` or C-far row, whose compact twin takes the same kernels and plan, is bit-identical to that twin (only addresses differ).
The twin runs first, the `over` and `edge-out` rows before the `high` rows.  The reduce job (`exact` data) is judged against an
int64 sum on the device for all elements and a numpy int64 sum on the host for 4096 sampled ones.

bf16 (PATHS["FAR16"] of oracle/gemm16_paths_np.py, arenas A and B refilled with 0x7FC0): the LDS-DMA, ping-pong and K-resident
rows kernels with A far by batch_stride and B by ldb, the ping-pong and K1-resident wgrads with either operand far, all four zones;
utterances are written as whole blocks (their windows may overlap).  lidbox_gemm_bf16_last_plan / _last_variant / _tn_last_pp /
_tn_last_kres equal the restated planner, which tests/test_oracle_gemm16_paths.py holds equal to the export on both sides.

Not here: the K-resident forward kernel's 2.0e9 per-utterance limit (one utterance of 1.25e8 windows: planner only) and
pp2_problem's own a_ext / b_ext (restated only); the row-stride edges of store_rows_tile on the stream-K kernels (M >= 128 rows
2^25 floats apart are 17 GB of C).

Found by this module: gemm16s_tn_kres_kernel returned NaN with its A far by batch_stride -- no addressing mistake, it reads every
element between two utterances against zero rows of dY, and the planner admitted batch strides that leave such elements to nobody.
plan_tn16s now refuses them (batch_stride < rows_per_batch row_stride + K1); the rows stay and expect the four-wave kernel.  Every
other guard holds as written up to 4.0e9 bytes.

First measured (MI355X, one run on one card): 144 cases in 11.9 s, the slowest 0.46 s (far-A-bs-sk_rows-nn-over, the first call),
peak 27.2 GiB.  Largest err / bound on `normal` (`exact` bit-equal everywhere, every same-plan row bit-identical to its twin):
gemm_sk_rows_kernel 0.005, gemm_skp_rows_kernel 0.002, gemm_rows_dma_kernel 0.051 (with a streamed remainder 0.011),
gemm_rows_dma8_kernel 0.034, gemm_sk_tn_kernel 0.017, gemm_tn_dma_kernel 0.018, the two calls behind a refused pair 0.043; on the
refused side gemm_rows_kernel 0.057, gemm_rows8_kernel 0.033, gemm_tn_kernel 0.023; gemm16s_rows_dma_kernel 0.009,
gemm16s_rows_pp_kernel 0.011, gemm16s_rows_kres_kernel 0.014, gemm16s_tn_pp_kernel 0.001, gemm16s_tn_kres_kernel 0.006,
gemm16s_rows_kernel 0.012, gemm16s_tn_kernel 0.005.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gemm16_paths_gpu as t16
import test_gemm_paths_gpu as tp
from far_buffers import Arena, MARGIN
from oracle import gemm16_paths_np as g
from oracle import gemm_paths_np as gp

pytestmark = pytest.mark.gpu

A_EXTENT = 4_300_000_000 // 16 * 16                  # the `over` rows: 1.05 x 4.0e9 bytes and the row behind them
C_EXTENT = 5_300_000_000 // 16 * 16                  # 40 rows 2^25 floats apart
NEED = 2 * (MARGIN + A_EXTENT + 256) + 2 * (MARGIN + C_EXTENT + 256)
assert NEED + (2 << 30) <= 32 << 30, "the module stays within 32 GiB"
WORST = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error ends the module: nothing more is launched on a device that has reported a fault"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error after a test of this module: %s" % e, returncode=3)


@pytest.fixture(scope="module")
def arenas():
    free = torch.cuda.mem_get_info()[0]
    assert free >= NEED + (2 << 30), "tests/test_gemm_far_gpu.py needs %.1f GiB of free device memory, %.1f GiB are free" % ((NEED + (2 << 30)) / 2 ** 30, free / 2 ** 30)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ar = dict(A=Arena(A_EXTENT), B=Arena(A_EXTENT), C=Arena(C_EXTENT), M=Arena(C_EXTENT))
    yield ar
    peak = torch.cuda.max_memory_allocated() - before
    print("peak device memory of the module: %.2f GiB" % (peak / 2 ** 30))
    assert peak <= 32 << 30
    ar.clear()
    torch.cuda.empty_cache()


def _rows(nv, arena, d):
    return nv.Rows(arena.base, d["bs"], d["rs"], d["batch"], d["rpb"])


def _note(group, ds, name, worst):
    key = (group, ds)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print("%-44s %-6s max err/bound=%.3e   [%s so far %.3e]" % (name, ds, worst, group, WORST[key]))


def _check_input(arena, d, cols, payload, what):
    assert arena.changed_words() == payload.numel() * payload.element_size() // 4, "%s: words outside the payload changed" % what
    assert arena.same_bits(d, cols, payload), "%s: the payload changed" % what
    arena.clear(d, cols)


def _b_desc(r):
    rows, cols = (r["K"], r["N"]) if r["kind"] == "nn" else (r["N"], r["K"])
    return dict(batch=1, rpb=rows, rs=gp.ldb_of(r), bs=0), cols


def run_far_rows(r, dat, ar):
    """one lidbox_gemm_nn / _nt call with A, B, C and the mask in the arenas, laid out by the row's descriptors; returns
    (C's payload [M, N] on the host, changed words of C's arena, family, launches)"""
    nv = tp._nv()
    M, N, K, epi = r["M"], r["N"], r["K"], r["epi"]
    bd, bcols = _b_desc(r)
    pa = ar["A"].put(r["a"], K, dat["A"])
    pb = ar["B"].put(bd, bcols, dat["B"])
    pm = aux = None
    if epi in gp.EPI_ACCUMS:
        ar["C"].put(r["c"], N, dat["old"])
    if epi in gp.EPI_HAS_BIAS:
        aux = tp._buf(dat["bias"])
    elif epi in gp.EPI_HAS_MASK:
        pm = ar["M"].put(r["c"], N, dat["mask"])
    wsb, ws_al = gp.row_ws_bytes(r)
    wsg, wsp, wsn = tp._ws(wsb, ws_al)
    fn = nv.lib.lidbox_gemm_nn if r["kind"] == "nn" else nv.lib.lidbox_gemm_nt
    auxp = aux.ptr if aux is not None else (ar["M"].ptr if pm is not None else None)
    nv.check(fn(_rows(nv, ar["A"], r["a"]), ar["B"].ptr, gp.ldb_of(r), _rows(nv, ar["C"], r["c"]), K, N, epi, auxp, wsp, wsn, nv.current_stream()))
    torch.cuda.synchronize()
    fam, launches = nv.lib.lidbox_gemm_last_family(), tp._launches(nv)
    _check_input(ar["A"], r["a"], K, pa, "A")
    _check_input(ar["B"], bd, bcols, pb, "B")
    if pm is not None:
        _check_input(ar["M"], r["c"], N, pm, "the mask")
    if aux is not None:
        assert tp._same(aux.numpy(), np.ascontiguousarray(dat["bias"], np.float32)), "the bias changed"
    if wsg is not None:
        wsg.check()
    changed = ar["C"].changed_words()
    got = ar["C"].get(r["c"], N).cpu().numpy()
    ar["C"].clear(r["c"], N)
    return got, changed, fam, launches


_ORDER = {"over": 0, "edge-out": 1, "c-far": 2, "edge-in": 3, "high": 4}
FAR = sorted(gp.PATHS["FAR"], key=lambda r: _ORDER[r["zone"]])
FAR_ROWS = [r for r in FAR if r["kind"] in ("nn", "nt")]
FAR_TN = [r for r in FAR if r["kind"] == "tn"]
FAR_PAIR = [r for r in FAR if r["kind"] == "pair"]
FAR_JOB = [r for r in FAR if r["kind"] == "job"]


@pytest.mark.parametrize("r", FAR_ROWS, ids=[r["name"] for r in FAR_ROWS])
def test_far_rows_row(r, arenas, monkeypatch):
    tp._setenv(monkeypatch, r["env"])
    pred = gp.far_row_predict(r)
    twin = gp.compact_twin(r)
    tpred = gp.far_row_predict(twin)
    same_plan = (pred["family"], pred["kernels"], pred["launches"], pred["g"], pred["p"]) == (tpred["family"], tpred["kernels"], tpred["launches"], tpred["g"], tpred["p"])
    assert same_plan == (r["zone"] in ("high", "edge-in", "c-far")), r["why"]
    group = pred["kernels"][0].split("<")[0] + ("+stream" if pred["g"] else "")
    for ds in ("normal", "exact"):
        dat = gp.make_rows_data(twin, ds)
        # the compact twin first, in guarded buffers
        tflat, tfam, tl = tp.run_rows(twin, dat)
        assert tfam == tpred["family"] and tl == tpred["launches"], ("twin", tfam, tl, tpred)
        ok, worst, what = gp.judge_rows(twin, ds, dat, tflat, tpred["p"])
        assert ok, "%s [%s] %s: worst err/bound %.3g" % (twin["name"], ds, what, worst)
        got, changed, fam, launches = run_far_rows(r, dat, arenas)
        assert fam == pred["family"] and launches == pred["launches"], (r["why"], fam, launches, pred)
        ok, worst, what = gp.judge_far_rows(r, ds, dat, got, changed, pred["p"])
        _note(group + " " + r["zone"], ds, r["name"], worst)
        assert ok, "%s [%s] %s: worst err/bound %.3g (%s)" % (r["name"], ds, what, worst, r["why"])
        if same_plan:
            assert tp._same(got, tflat[gp.index(twin["c"], r["N"])]), "%s [%s]: not bit-identical to its compact twin" % (r["name"], ds)


def run_far_tn(r, dat, ar):
    nv = tp._nv()
    K1, N = r["K1"], r["N"]
    pa = ar["A"].put(r["a"], K1, dat["A"])
    pb = ar["B"].put(r["b"], N, dat["B"])
    c = tp._buf(dat["c_flat"])
    bg = tp._buf(dat["old_bg"]) if r["bias_grad"] else None
    wsb = nv.lib.lidbox_gemm_tn_workspace(r["M"], K1, N)
    assert wsb == gp.tn_workspace(r["M"], K1, N, r["env"])
    wsg, wsp, wsn = tp._ws(wsb)
    nv.check(nv.lib.lidbox_gemm_tn(_rows(nv, ar["A"], r["a"]), _rows(nv, ar["B"], r["b"]), c.ptr, N + r["ldc_pad"], K1, N, r["accumulate"],
                                   bg.ptr if bg is not None else None, wsp, wsn, nv.current_stream()))
    torch.cuda.synchronize()
    fam, launches = nv.lib.lidbox_gemm_last_family(), tp._launches(nv)
    _check_input(ar["A"], r["a"], K1, pa, "X")
    _check_input(ar["B"], r["b"], N, pb, "dY")
    wsg.check()
    return c.numpy().copy(), (bg.numpy().copy() if bg is not None else None), fam, launches


@pytest.mark.parametrize("r", FAR_TN, ids=[r["name"] for r in FAR_TN])
def test_far_tn_row(r, arenas, monkeypatch):
    tp._setenv(monkeypatch, r["env"])
    pred, twin = gp.far_tn_predict(r), gp.compact_twin(r)
    tpred = gp.far_tn_predict(twin)
    same_plan = pred == tpred
    assert same_plan == (r["zone"] == "high"), r["why"]
    for ds in ("normal", "exact"):
        dat = gp.make_tn_data(twin, ds)
        tc, tbg, tfam, tl = tp.run_tn(twin, dat)
        assert tfam == tpred["family"] and tl == tpred["launches"], ("twin", tfam, tl, tpred)
        assert gp.judge_tn(twin, ds, dat, tc, tbg, tpred["splits"], tpred["rps"])[0], twin["name"]
        c, bg, fam, launches = run_far_tn(r, dat, arenas)
        assert fam == pred["family"] and launches == pred["launches"], (r["why"], fam, launches, pred)
        ok, worst, worst_g = gp.judge_tn(r, ds, dat, c, bg, pred["splits"], pred["rps"])
        _note(pred["kernels"][0].split("<")[0] + " " + r["zone"], ds, r["name"], max(worst, worst_g))
        assert ok, "%s [%s]: worst err/bound dW %.3g, bias grad %.3g (%s)" % (r["name"], ds, worst, worst_g, r["why"])
        if same_plan:
            assert tp._same(c, tc) and tp._same(bg, tbg), "%s [%s]: not bit-identical to its compact twin" % (r["name"], ds)


@pytest.mark.parametrize("r", FAR_PAIR, ids=[r["name"] for r in FAR_PAIR])
def test_far_pair_row(r, arenas, monkeypatch):
    """lidbox_gemm_nt_tn with one operand predicate refused: the two calls run (the wgrad, then the dgrad that carries its reduce where
    it is an LDS-DMA launch), each on the path its own guard leaves it"""
    nv = tp._nv()
    env = r["env"]
    tp._setenv(monkeypatch, env)
    M, Co, N, K1, ldb = r["M"], r["Co"], r["N"], r["K1"], r["ldb"]
    nt = gp._row(r["name"], r["why"], "nt", N, Co, gp._dense(M, Co), epi=gp.EPI_RELU_MASK, env=env, ldb_pad=ldb - Co)
    tn = gp._tn_row(r["name"], r["why"], K1, Co, r["x"], b=gp._dense(M, Co), env=env, accumulate=1)
    al_rows, al_tn = gp.pair_al(nt["a"], Co, N, ldb, r["x"], K1)
    ws_nt_b = max(nv.lib.lidbox_gemm_rows_workspace(M, N, Co), 2 * M * N * 4)
    ws_tn_b = nv.lib.lidbox_gemm_tn_workspace(M, K1, Co)
    assert gp.pair_plan(M, Co, N, K1, ws_nt_b, ws_tn_b, env) is not None and gp.pair_plan(M, Co, N, K1, ws_nt_b, ws_tn_b, env, al_rows, al_tn) is None
    rows = gp.rows_dispatch(1, M, N, Co, True, ws_nt_b, env, nt["epi"], b_ext=gp.sk_b_extent_ok(1, Co, N, ldb))
    tnp = gp.tn_dispatch(M, K1, Co, True, True, ws_tn_b, env, a_ext=gp.sk_extent_ok(r["x"], K1))
    assert (rows["family"], tnp["family"]) == ((0, 1) if r["refused"] == "al_rows" else (1, 0)), (rows, tnp)
    for ds in ("normal", "exact"):
        dat = gp.make_rows_data(gp.compact_twin(nt), ds)
        tdat = gp.make_tn_data(gp.compact_twin(tn), ds)
        tdat["b_flat"], tdat["B"] = dat["a_flat"], dat["A"]          # dY is the dgrad's A and the wgrad's B
        dy, dx, mk = tp._buf(dat["a_flat"]), tp._buf(dat["c_flat"]), tp._buf(dat["mask_flat"])
        dw, bg = tp._buf(tdat["c_flat"]), tp._buf(tdat["old_bg"])
        bd, bcols = _b_desc(nt)
        pw = arenas["B"].put(bd, bcols, dat["B"])
        px = arenas["A"].put(r["x"], K1, tdat["A"])
        wn, wnp, wnn = tp._ws(ws_nt_b)
        wt, wtp, wtn = tp._ws(ws_tn_b)
        nv.check(nv.lib.lidbox_gemm_nt_tn(tp._desc(nv, dy, nt["a"]), arenas["B"].ptr, ldb, tp._desc(nv, dx, nt["c"]), Co, N, nt["epi"], mk.ptr, wnp, wnn,
                                          _rows(nv, arenas["A"], r["x"]), dw.ptr, Co, K1, 1, bg.ptr, wtp, wtn, nv.current_stream()))
        torch.cuda.synchronize()
        fam, launches, carried = nv.lib.lidbox_gemm_last_family(), tp._launches(nv), nv.lib.lidbox_gemm_last_carried()
        wn.check()
        wt.check()
        _check_input(arenas["B"], bd, bcols, pw, "W")
        _check_input(arenas["A"], r["x"], K1, px, "X")
        assert tp._same(dy.numpy(), dat["a_flat"]) and tp._same(mk.numpy(), dat["mask_flat"])
        assert (fam, launches) == (rows["family"], rows["launches"]), (fam, launches, rows)
        assert carried == (1 if (tnp["kernels"][1] == "splitk_reduce4_kernel" and rows["family"] in (1, 3)) else 0), carried
        ok, worst, what = gp.judge_rows(nt, ds, dat, dx.numpy(), rows["p"])
        okt, worst_t, worst_g = gp.judge_tn(tn, ds, tdat, dw.numpy(), bg.numpy(), tnp["splits"], tnp["rps"])
        _note("two calls " + r["refused"], ds, r["name"], max(worst, worst_t, worst_g))
        assert ok and okt, (r["name"], ds, what, worst, worst_t, worst_g)


@pytest.fixture(scope="module")
def slices(arenas):
    """960 slices of 2^20 integers in [-7, 7] at the base of arena A, written 64 slices at a time; their int64 prefix sums over the
    first 940 and over all 960 slices, kept on the device"""
    n, top = 1 << 20, 960
    gen = torch.Generator(device="cuda").manual_seed(7)
    view = torch.as_strided(arenas["A"].words.view(torch.float32), (top, n), (n, 1), MARGIN // 4)
    total = torch.zeros(n, dtype=torch.int64, device="cuda")
    sums = {}
    for lo in range(0, top, 20):
        v = torch.randint(-7, 8, (20, n), generator=gen, device="cuda")
        view[lo:lo + 20].copy_(v.to(torch.float32))
        total += v.sum(0)
        if lo + 20 in (940, 960):
            sums[lo + 20] = total.clone()
    pc = torch.randint(-7, 8, (top, 1024), generator=gen, device="cuda")
    yield dict(view=view, sums=sums, pc=pc, n=n)
    arenas["A"].refill()


@pytest.mark.parametrize("r", FAR_JOB, ids=[r["name"] for r in FAR_JOB])
def test_far_reduce_job(r, arenas, slices):
    """lidbox_reduce_jobs_run on a hand-made job whose slices span 3.94e9 (940) and 4.03e9 (960) bytes: the entry point runs the
    16-byte kernel either way (reduce_job_vec_ok is the callers' test); its scalar offsets k n 4 stay below 2^32, so the sum must be
    the int64 one in both"""
    nv = tp._nv()
    n, N, splits, acc = r["n"], r["N"], r["splits"], r["accumulate"]
    rng = np.random.default_rng(splits + acc)
    old = rng.integers(-9, 10, n).astype(np.float32) if acc else np.full(n, np.nan, np.float32)
    oldb = rng.integers(-9, 10, N).astype(np.float32) if acc else np.full(N, np.nan, np.float32)
    c, bgr = tp._buf(old), tp._buf(oldb)
    pc = tp._buf(slices["pc"][:splits].to(torch.float32).cpu().numpy().ravel()) if r["bias_partials"] else None
    job = nv.ReduceJob()
    job.partials, job.C, job.n, job.ldc, job.splits, job.N, job.accumulate = arenas["A"].base, c.view.data_ptr(), n, N, splits, N, acc
    if pc is not None:
        job.bias_partials, job.bias_grad = pc.view.data_ptr(), bgr.view.data_ptr()
    job.nblocks = min(2048, gp.cdiv((n + N) // 4, 256))               # as make_reduce_job sets it
    nv.check(nv.lib.lidbox_reduce_jobs_run(ctypes.byref(job), 1, nv.current_stream()))
    torch.cuda.synchronize()
    assert arenas["A"].changed_words() == 960 * n, "words outside the slices changed"
    again = torch.zeros(n, dtype=torch.int64, device="cuda")
    for lo in range(0, splits, 20):
        again += slices["view"][lo:lo + 20].to(torch.int64).sum(0)
    assert torch.equal(again, slices["sums"][splits]), "the slices changed"
    want = slices["sums"][splits] + (torch.from_numpy(old).to("cuda").to(torch.int64) if acc else 0)
    c.check()
    assert torch.equal(c.view.to(torch.int64), want) and bool(torch.isfinite(c.view).all()), "%s: the device int64 sum differs" % r["name"]
    idx = np.sort(np.random.default_rng(3).choice(n, 4096, replace=False))
    host = slices["view"][:splits][:, torch.from_numpy(idx).to("cuda")].cpu().numpy().astype(np.int64).sum(0) + (old[idx].astype(np.int64) if acc else 0)
    assert np.array_equal(c.numpy()[idx].astype(np.int64), host), "%s: 4096 sampled elements against the host sum" % r["name"]
    if pc is not None:
        wantb = slices["pc"][:splits].sum(0).cpu().numpy() + (oldb.astype(np.int64) if acc else 0)
        assert tp._same(bgr.numpy(), wantb.astype(np.float32)), "%s: the bias gradient" % r["name"]
    else:
        assert tp._same(bgr.numpy(), oldb), "a job without bias slices leaves the bias gradient alone"


# ---------------------------------------------------------------------------------------------------------- bf16 storage kernels
FAR16 = sorted([r for r in g.PATHS["FAR16"] if not r.get("planner_only")], key=lambda r: _ORDER[r["zone"]])
FAR16_ROWS = [r for r in FAR16 if r["kind"] != "tn"]
FAR16_TN = [r for r in FAR16 if r["kind"] == "tn"]


@pytest.fixture(scope="module")
def arenas16(arenas):
    """arenas A and B hold bfloat16 rows (every element 0x7FC0) for the cases below"""
    arenas["A"].refill(bf16=True)
    arenas["B"].refill(bf16=True)
    yield arenas
    arenas["A"].refill()
    arenas["B"].refill()


def _blocks(d, w):
    """the utterances of a descriptor as non-overlapping blocks (windows inside an utterance may overlap): (descriptor, length)"""
    return dict(batch=d["batch"], rpb=1, rs=0, bs=d["bs"]), (d["rpb"] - 1) * d["rs"] + w


def _compact16(d, w):
    return dict(d, bs=gp.cdiv(_blocks(d, w)[1], 8) * 8 if d["batch"] > 1 else 0)


def _put_blocks(arena, far, twin, w, flat):
    bd, n = _blocks(far, w)
    pay = np.stack([flat[b * twin["bs"]:b * twin["bs"] + n] for b in range(far["batch"])])
    assert np.isfinite(pay).all(), "a payload block holds every element of its utterance"
    return bd, n, arena.put(bd, n, pay)


@pytest.mark.parametrize("r", FAR16_ROWS, ids=[r["name"] for r in FAR16_ROWS])
def test_far16_rows_row(r, arenas16, monkeypatch):
    nv = tp._nv()
    t16._setenv(monkeypatch, r["env"])
    K, N = r["K"], r["N"]
    twin = dict(r, name=r["name"] + "@compact", a=_compact16(r["a"], K), ldb_pad=0)
    q, tq = g.row_query(r), g.row_query(twin)
    e = r["expect"]
    assert (e["kernel"] is None or q[0] == e["kernel"]) and (e["not_kernel"] is None or q[0] != e["not_kernel"]), (r["why"], q)
    assert (q == tq) == (r["zone"] in ("high", "edge-in")), (q, tq)
    for ds in ("normal", "exact"):
        dat = g.make_rows_data(twin, ds)
        rc, tc, _ = t16.run_rows(twin, dat)
        nv.check(rc)
        assert t16._last_plan(nv) == [tq[0], tq[4], tq[5], tq[6]], ("twin", t16._last_plan(nv), tq)
        assert g.judge_rows(twin, ds, dat, tc, None, max(tq[4], tq[7]))[0], twin["name"]
        ad, an, pa = _put_blocks(arenas16["A"], r["a"], twin["a"], K, dat["a_flat"])
        bd = dict(batch=1, rpb=N, rs=g.ldb_of(r), bs=0)
        pb = arenas16["B"].put(bd, K, dat["B"])
        c = t16._buf(dat["c_flat"])
        wsg, wsp, wsn = t16._ws(g.row_ws_bytes(r))
        rc = nv.lib.lidbox_gemm_bf16s_nt(_rows(nv, arenas16["A"], r["a"]), arenas16["B"].ptr, g.ldb_of(r), t16._desc(nv, c.view.data_ptr(), r["c"]), None, K, N,
                                        r["epi"], None, wsp, wsn, nv.current_stream())
        torch.cuda.synchronize()
        nv.check(rc)
        plan, variant = t16._last_plan(nv), t16._last_variant(nv)
        _check_input(arenas16["A"], ad, an, pa, "A")
        _check_input(arenas16["B"], bd, K, pb, "B")
        if wsg is not None:
            wsg.check()
        got = c.numpy().copy()
        assert plan == [q[0], q[4], q[5], q[6]] and variant == (q[1:4] if q[0] != g.KS_ROWS else [0, 0, 0]), (r["why"], plan, variant, q)
        ok, worst, what = g.judge_rows(twin, ds, dat, got, None, max(q[4], q[7]))
        _note((g.kernel_name(q, g.Q16_NT) or "none") + " " + r["zone"], ds, r["name"], worst)
        assert ok, "%s [%s] %s: worst err/bound %.3g (%s)" % (r["name"], ds, what, worst, r["why"])
        if q == tq:
            assert tp._same(got, tc), "%s [%s]: not bit-identical to its compact twin" % (r["name"], ds)


@pytest.mark.parametrize("r", FAR16_TN, ids=[r["name"] for r in FAR16_TN])
def test_far16_tn_row(r, arenas16, monkeypatch):
    nv = tp._nv()
    t16._setenv(monkeypatch, r["env"])
    K1, N = r["K1"], r["N"]
    twin = dict(r, name=r["name"] + "@compact", a=_compact16(r["a"], K1), b=_compact16(r["b"], N))
    q, tq = g.tn_row_query(r), g.tn_row_query(twin)
    e = r["expect"]
    assert q[0] == e["kernel"] and (e["not_kernel"] is None or q[0] != e["not_kernel"]), (r["why"], q)
    assert (q == tq) == r["twin_same"], (q, tq)
    plan = g.tn_row_plan(r, q)
    for ds in ("normal", "exact"):
        dat = g.make_tn_data(twin, ds)
        rc, tc, tbg, _ = t16.run_tn(twin, dat)
        nv.check(rc)
        tplan = g.tn_row_plan(twin, tq)
        assert t16._last_plan(nv) == [tq[0], tq[4], tq[11] if tq[0] == g.KS_TN_KRES else tq[5], 0], ("twin", t16._last_plan(nv), tq)
        assert g.judge_tn(twin, ds, dat, tc, tbg, tplan["pieces"], tplan["per"])[0], twin["name"]
        ad, an, pa = _put_blocks(arenas16["A"], r["a"], twin["a"], K1, dat["a_flat"])
        bd, bn, pb = _put_blocks(arenas16["B"], r["b"], twin["b"], N, dat["b_flat"])
        c = t16._buf(dat["c_flat"])
        bg = t16._buf(dat["old_bg"]) if r["bias_grad"] else None
        wsg, wsp, wsn = t16._ws(g.tn_row_ws_bytes(r))
        rc = nv.lib.lidbox_gemm_bf16s_tn(_rows(nv, arenas16["A"], r["a"]), _rows(nv, arenas16["B"], r["b"]), c.ptr, N + r["ldc_pad"], K1, N, r["accumulate"],
                                        bg.ptr if bg is not None else None, wsp, wsn, nv.current_stream())
        torch.cuda.synchronize()
        nv.check(rc)
        last = t16._last_plan(nv)
        pp, kres = nv.lib.lidbox_gemm_bf16s_tn_last_pp(), nv.lib.lidbox_gemm_bf16s_tn_last_kres()
        _check_input(arenas16["A"], ad, an, pa, "X")
        _check_input(arenas16["B"], bd, bn, pb, "dY")
        wsg.check()
        got_c, got_bg = c.numpy().copy(), (bg.numpy().copy() if bg is not None else None)
        assert last == [q[0], q[4], q[11] if q[0] == g.KS_TN_KRES else q[5], 0], (r["why"], last, q)
        assert pp == (q[4] if q[0] == g.KS_TN_PP else 0) and kres == (q[4] if q[0] == g.KS_TN_KRES else 0)
        ok, worst, worst_g = g.judge_tn(twin, ds, dat, got_c, got_bg, plan["pieces"], plan["per"])
        _note(g.kernel_name(q) + " " + r["zone"], ds, r["name"], max(worst, worst_g))
        assert ok, "%s [%s]: worst err/bound %.3g, bias gradient %.3g (%s)" % (r["name"], ds, worst, worst_g, r["why"])
        if q == tq:
            assert tp._same(got_c, tc) and (got_bg is None or tp._same(got_bg, tbg)), "%s [%s]: not bit-identical to its compact twin" % (r["name"], ds)
