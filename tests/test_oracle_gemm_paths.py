"""
Pins oracle/gemm_paths_np.py on the CPU (no device, no launches):
  1. the restated host functions against the library's planner exports (lidbox_gemm_plan_query, _plan_is_stream_k,
     _plan_waves, _plan_stream_tail, _plan_is_pair, _rows_workspace, _tn_workspace, lidbox_colsum_workspace) over the tuned
     table, the PATHS rows and a grid of a few thousand shapes, under the default environment and every environment a row sets;
  2. every PATHS row selects what its `why` says under the restated dispatch, the rows together reach every kernel
     instantiation the launch sites of gemm.hip name (65, enumerated from the source text by gp.instantiations_from_source), and the tables hold
     every edge of the EDGES list;
  3. the float64 references against float64 torch (matmul; conv1d windows against unfold);
  4. the fp32 emulation of every row lies inside the bounds on `normal` and `offset` and equals int64 on `exact`, and every
     planted mutation is caught on every row it applies to (gp.applies: the explicit exclusion rules): zero uncaught pairs.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import gemm_paths_np as gp

ROWS, TN = gp.PATHS["ROWS"], gp.PATHS["TN"]


@pytest.fixture(scope="module")
def lib():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native.lib


def _setenv(monkeypatch, env):
    for k in list(os.environ):
        if k.startswith("LIDBOX_GEMM_"):
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _envs():
    seen, out = set(), []
    for r in [dict(env={})] + ROWS + TN + gp.PATHS["PAIR"] + [dict(env={"LIDBOX_GEMM_NO_TUNED": "1"}), dict(env={"LIDBOX_GEMM_NT8": "64"}),
                                                             dict(env={"LIDBOX_GEMM_NN8": "128"}), dict(env={"LIDBOX_GEMM_SK": "0"})]:
        key = tuple(sorted(r["env"].items()))
        if key not in seen:
            seen.add(key)
            out.append(dict(r["env"]))
    return out


def _query(lib, kind, M, N, K, wsb):
    out = (ctypes.c_int * 4)()
    assert lib.lidbox_gemm_plan_query(kind, M, N, K, wsb, out) == 0
    return list(out)


def _shapes():
    rng = np.random.default_rng(7)
    s = [(k[1], k[2], k[3]) for k in gp.tuned_table()]
    s += sorted({(r["M"], r["N"], r["K"]) for r in ROWS if r["M"] and r["N"]})
    s += [(r["M"], r["N"], r["K1"]) for r in TN]
    for _ in range(120):
        s.append((int(rng.choice([1, 7, 64, 130, 257, 512, 1000, 2112, 4224, 8448, 25344])), int(rng.integers(1, 1600)), int(rng.integers(1, 3100))))
    return s


# ------------------------------------------------------------------------------------------ 1. restated host functions
def test_restated_dispatch_matches_the_exports(lib, monkeypatch):
    shapes = _shapes()
    n = 0
    for env in _envs():
        _setenv(monkeypatch, env)
        for M, N, K in shapes:
            wss = (0, 1 << 20, gp.rows_workspace(M, N, K, env))
            assert lib.lidbox_gemm_rows_workspace(M, N, K) == wss[2], (env, M, N, K)
            assert lib.lidbox_gemm_tn_workspace(M, K, N) == gp.tn_workspace(M, K, N, env), (env, M, N, K)
            pl = gp.tn_plan(M, K, N, env)
            assert _query(lib, 2, M, N, K, 0) == [pl["bm"], pl["bn"], pl["splits"], pl["rps"]], (env, M, N, K)
            tws = gp.tn_workspace(M, K, N, env)
            assert lib.lidbox_gemm_plan_is_stream_k(2, M, N, K, tws) == gp.plan_is_stream_k(2, M, N, K, tws, env), (env, M, N, K)
            for kind in (0, 1):
                for wsb in wss:
                    ch = gp.choose_rows_env(kind, M, N, K, wsb, env)
                    assert _query(lib, kind, M, N, K, wsb) == [ch["bm"], ch["bn"], ch["splits"], ch["kps"]], (env, kind, M, N, K, wsb)
                    assert lib.lidbox_gemm_plan_waves(kind, M, N, K, wsb) == ch["waves"]
                    assert lib.lidbox_gemm_plan_is_stream_k(kind, M, N, K, wsb) == gp.plan_is_stream_k(kind, M, N, K, wsb, env), (env, kind, M, N, K, wsb)
                    assert lib.lidbox_gemm_plan_stream_tail(kind, M, N, K, wsb) == gp.plan_stream_tail(kind, M, N, K, wsb, env), (env, kind, M, N, K, wsb)
                    n += 1
            K1 = 64 if K > 64 else K
            ws_nt, ws_tn = wss[2], gp.tn_workspace(M, K1, K, env)
            assert lib.lidbox_gemm_plan_is_pair(M, K, N, K1, ws_nt, ws_tn) == int(gp.pair_plan(M, K, N, K1, ws_nt, ws_tn, env) is not None), (env, M, N, K)
    assert n >= 3000
    for M, N in ((1, 1), (255, 3), (257, 5), (40000, 7)):
        assert lib.lidbox_colsum_workspace(M, N) == gp.colsum_workspace(M, N)


def test_row_workspaces_match_the_exports(lib, monkeypatch):
    """the workspace size each GPU row hands over is the library's own figure (or, for a forced plan, that plan's need)"""
    for r in ROWS:
        if r["ws"] == "lib":
            _setenv(monkeypatch, r["env"])
            assert gp.row_ws_bytes(r)[0] == lib.lidbox_gemm_rows_workspace(r["M"], r["N"], r["K"]), r["name"]


# ------------------------------------------------------------------------------------------ 2. the rows select their paths
@pytest.mark.parametrize("r", ROWS, ids=[r["name"] for r in ROWS])
def test_rows_row_selects_its_path(r):
    p, e = gp.row_predict(r), r["expect"]
    if "family" in e:
        assert p["family"] == e["family"], p
    if "family_not" in e:
        assert p["family"] != e["family_not"] and gp.row_al(r) == (r["name"] != "sk-refuse-K%4"), p
    if "kernel" in e:
        assert p["kernels"][0] == e["kernel"], p
    if "launches" in e:
        assert p["launches"] == e["launches"], p
    if "splits" in e:
        assert p["ch"]["splits"] == e["splits"] and (p["ch"]["splits"] - 1) * p["ch"]["kps"] < r["K"], p
    if "g" in e:
        assert (p["g"] >= 2 if e["g"] == "model" else p["g"] == e["g"]), p
    if "branch" in e:
        assert p["sk"]["branch"] == e["branch"], p
    if "skp" in e:
        assert p["kernels"][0].startswith("gemm_skp_rows_kernel" if e["skp"] else "gemm_sk_rows_kernel"), p
    if r["name"].startswith("un-") or r["name"].startswith("alterm-"):
        assert not gp.row_al(r)
    # each row stays small (the largest is stream-g8: g = 8 needs K >= 1024 and more than 256 tiles of 64 x 64, 2.2 GFLOP)
    assert 2.0 * r["M"] * r["N"] * r["K"] <= 2.3e9 and r["M"] * r["K"] <= 42e6


def test_named_rows_hold_what_they_claim():
    by = {r["name"]: r for r in ROWS}
    p = gp.row_predict
    assert p(by["splitk-lone-tail"])["ch"]["kps"] == 48 and by["splitk-lone-tail"]["K"] - 2 * 48 == 4
    assert by["splitk-big-reduce"]["M"] * by["splitk-big-reduce"]["N"] > 2048 * 256
    assert p(by["splitk-ws-short"])["ch"]["splits"] == 1
    short, full = p(by["stream-ws-short"]), p(by["stream-g-model"])
    assert full["g"] >= 2 and short["g"] == 0
    assert p(by["stream-off"])["launches"] == [1, 0, 0]
    assert not p(by["no-tail-split"])["tail_split"]
    for name in ("sk-refuse-ws-short", "sk-refuse-ws-misaligned"):
        r = dict(by[name], ws="lib")
        assert p(r)["family"] == 2, name                      # one byte more, or 16-byte aligned: stream-K
    # a tuned shape leaves stream-K unless LIDBOX_GEMM_NO_TUNED (or SK_ALL) is set
    kind, M, N, K = 0, 8448, 512, 1536                         # frame3 fwd: 13 GFLOP, checked here only
    assert (kind, M, N, K) in gp.tuned_table()
    ws = gp.rows_workspace(M, N, K, {})
    assert gp.rows_dispatch(kind, M, N, K, True, ws, {})["family"] != 2
    assert gp.rows_dispatch(kind, M, N, K, True, gp.rows_workspace(M, N, K, {"LIDBOX_GEMM_NO_TUNED": "1"}), {"LIDBOX_GEMM_NO_TUNED": "1"})["family"] == 2


@pytest.mark.parametrize("r", TN, ids=[r["name"] for r in TN])
def test_tn_row_selects_its_path(r):
    p, e = gp.tn_row_predict(r), r["expect"]
    for k in ("family", "splits", "rps"):
        if k in e:
            assert p[k] == e[k], p
    if "kernel" in e:
        assert p["kernels"][0] == e["kernel"], p
    if "reduce" in e:
        assert p["kernels"][1] == e["reduce"], p
    if r["name"].startswith("tn-al") or r["name"].startswith("tn-dma"):
        assert r["M"] % p["rps"] != 0 and p["kernels"][1] == "splitk_reduce4_kernel"          # ragged last slice, job-form reduce


def test_carry_rows_hold_each_case():
    rows = gp.PATHS["CARRY"]
    assert {(r["jobs"], r["carried"], r["rc_ok"]) for r in rows} >= {("w", 1, True), ("wz", 2, True), ("z", 1, True), ("wzz", 0, False)}
    assert any(r["env"].get("LIDBOX_GEMM_DMA") == "0" and r["carried"] == 0 for r in rows)
    for r in rows:                                               # the dgrad is an LDS-DMA launch unless the row switches it off
        p = gp.rows_dispatch(1, r["M"], r["N"], r["Co"], True, gp.rows_workspace(r["M"], r["N"], r["Co"], r["env"]), r["env"], gp.EPI_ACCUM_RELU_MASK)
        assert (p["family"] == 1) == (r["env"].get("LIDBOX_GEMM_DMA") != "0"), r["name"]
        tp = gp.tn_dispatch(r["Mw"], r["K1"], r["Co"], True, True, gp.tn_workspace(r["Mw"], r["K1"], r["Co"], r["env"]), r["env"], ldc=r["Co"] + 4)
        assert tp["kernels"][1] == "splitk_reduce4_kernel", r["name"]


def test_pair_rows_select_their_path():
    for r in gp.PATHS["PAIR"]:
        M, Co, N, K1, env = r["M"], r["Co"], r["N"], r["K1"], r["env"]
        ws_nt = max(gp.rows_workspace(M, N, Co, env), 2 * M * N * 4)
        assert (gp.pair_plan(M, Co, N, K1, ws_nt, gp.tn_workspace(M, K1, Co, env), env) is not None) == (r["pair"] or r["shared"]), r["name"]


def _reached():
    got = set()
    for r in ROWS:
        got.update(gp.row_predict(r)["kernels"])
    for r in TN:
        got.update(gp.tn_row_predict(r)["kernels"])
    if gp.PATHS["COLSUM"]:
        got.update(["colsum_stage1", "colsum_stage2"])
    if any(r["pair"] for r in gp.PATHS["PAIR"]):
        got.add("gemm_nt_tn_pair_kernel")
    return got


def test_rows_reach_every_instantiation_the_launch_sites_name():
    inst = gp.instantiations_from_source()                  # enumerated from the hipLaunchKernelGGL sites and the macro invocations
    print("%d instantiations named by the launch sites" % len(inst))
    assert len(inst) == len(set(inst)) == 65
    assert set(inst) == set(gp.instantiations())            # the names the restated dispatch can predict are exactly these
    per = {}
    for k in inst:
        per[k.split("<")[0]] = per.get(k.split("<")[0], 0) + 1
    assert per == {"gemm_rows_kernel": 16, "gemm_rows8_kernel": 8, "gemm_tn_kernel": 8, "gemm_rows_dma_kernel": 8, "gemm_rows_dma8_kernel": 4,
                   "gemm_tn_dma_kernel": 4, "gemm_nt_tn_pair_kernel": 1, "gemm_sk_rows_kernel": 2, "gemm_skp_rows_kernel": 8, "gemm_sk_tn_kernel": 1,
                   "rows_reduce_kernel": 1, "splitk_reduce_kernel": 1, "splitk_reduce4_kernel": 1, "colsum_stage1": 1, "colsum_stage2": 1}, per
    missing = set(inst) - _reached()
    assert not missing, sorted(missing)
    # removing a row that is the only one for its instantiation leaves a hole
    for victim in ("gemm_rows8_kernel<128,64,nt,al>", "gemm_skp_rows_kernel<nn,mask,noacc>"):
        keep = [r for r in ROWS if gp.row_predict(r)["kernels"][:1] != [victim]]
        assert len(keep) < len(ROWS) and victim not in {k for r in keep for k in gp.row_predict(r)["kernels"]}


def _boundaries(r):
    """{(o, dr of h = 0, dr of h = 1)}: utterance boundaries of C that fall o rows into a 32-row block which store_rows_tile takes
    as INNER (all rows inside M, N a multiple of the wave's columns, rpb >= 28); dr = o - 4 h is wfrom of that lane half"""
    out = set()
    if r["c"]["rpb"] < 28 or r["N"] % 64:
        return out
    for b in range(1, r["c"]["batch"]):
        m = b * r["c"]["rpb"]
        if m // 32 * 32 + 32 <= r["M"]:
            out.add((m % 32, m % 32, m % 32 - 4))
    return out


def _bound_row(rpb):
    return next(r for r in ROWS if r["name"] == "epi-bound-rpb%d-e5" % rpb)


EDGES = {
    "each al term false on its own": lambda: {"Abase", "Ars", "K%4", "Bbase", "ldb", "N%4", "Abs"} <= {r["name"].split("-")[1] if r["name"].startswith("alterm") else r["name"].split("-")[-1] for r in ROWS if r["name"].startswith(("alterm", "un-"))},
    "unaligned and aligned register-staged and DMA kernels at every tile and both wave counts": lambda: all(
        any(r["name"].startswith("%s-%dx%dw%d-%s" % (f, bm, bn, wv, k)) for r in ROWS) for f in ("un", "al", "dma") for bm, bn, wv in gp._TILES for k in ("nn", "nt")),
    "K of 1, 15, 16, 17, aligned and per-element tails": lambda: {1, 15, 16, 17, 20, 24, 28, 33, 34, 35} <= {r["K"] for r in ROWS if r["name"].startswith("K")},
    "M and N of 1, around a tile edge, one live row / column, zero": lambda: {(1, 1), (63, 65), (64, 64), (65, 63), (129, 1), (1, 129), (0, 8), (5, 0)} <= {(r["M"], r["N"]) for r in ROWS},
    "rpb 27, 28, 29, 33 with wrap = 0 and > 0, store-only and accumulating masked forms, both families": lambda: all(
        any(r["name"] == "epi-rpb%d-gap%d-e%d-f%d" % (rpb, gap, e, f) for r in ROWS) for rpb in (27, 28, 29, 33) for gap in (0, 12) for e in (2, 5) for f in (0, 1)),
    "utterance boundary at dr = 0 in a select-form block, at dr = 27, and absent from every block": lambda: (
        any(o > 0 and d1 == 0 for o, d0, d1 in _boundaries(_bound_row(36))) and any(d0 == 27 for o, d0, d1 in _boundaries(_bound_row(59)))
        and all(o == 0 for r_ in (_bound_row(32), _bound_row(64)) for o, d0, d1 in _boundaries(r_)) and len(_boundaries(_bound_row(64))) >= 1),
    "a mask read through C's pitched layout": lambda: any(r["epi"] in gp.EPI_HAS_MASK and r["c"]["rs"] > r["N"] and r["c"]["batch"] > 1 for r in ROWS),
    "all eight epilogues on families 0, 1, 2 plain, 2 pipelined, 3, the DMA-streamed remainder": lambda: all(
        set(range(8)) <= {r["epi"] for r in ROWS if sel(gp.row_predict(r))} for sel in (
            lambda p: p["family"] == 0, lambda p: p["family"] == 1, lambda p: p["family"] == 3,
            lambda p: p["family"] == 2 and p["kernels"][0].startswith("gemm_sk_"), lambda p: "".join(p["kernels"][:1]).startswith("gemm_skp_"))),
    "all eight epilogues through rows_reduce_kernel": lambda: set(range(8)) <= {r["epi"] for r in ROWS if "rows_reduce_kernel" in gp.row_predict(r)["kernels"]},
    "stream-K schedule branches": lambda: {"whole", "parts", "spans_T<P", "dp_fallback"} <= {gp.row_predict(r)["sk"]["branch"] for r in ROWS if gp.row_predict(r)["sk"]},
    "stream-K refusals": lambda: {"M<128", "K%4", "span", "ws-short", "ws-misaligned"} <= {r["name"][10:] for r in ROWS if r["name"].startswith("sk-refuse-")},
    "tail split with the remainder planned split: {1, 1, 1}": lambda: any(gp.row_predict(r)["tail_split"] and gp.row_predict(r)["launches"] == [1, 1, 1] for r in ROWS),
    "DmaStream g of 0, 2, 3, 8": lambda: {0, 2, 3, 8} <= {gp.row_predict(r)["g"] for r in ROWS if r["name"].startswith(("stream", "no-tail"))},
    "wgrad: ragged slice, one slice, cap, accumulate 0 / 1, bias_grad NULL / given, ldc > N, both reduces, conv strides": lambda: (
        {0, 1} <= {r["accumulate"] for r in TN} and {True, False} <= {r["bias_grad"] for r in TN} and any(r["ldc_pad"] for r in TN)
        and {"splitk_reduce4_kernel", "splitk_reduce_kernel"} <= {gp.tn_row_predict(r)["kernels"][1] for r in TN}
        and {1, 2, 3} <= {r["a"]["rs"] // 16 for r in TN if r["name"].startswith("tn-conv")} and any(gp.tn_row_predict(r)["rps"] == 8192 for r in TN)
        and any(gp.tn_row_predict(r)["splits"] == 1 for r in TN)),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_tables_hold_the_edge(edge):
    assert EDGES[edge](), edge


def test_stream_epilogues_cover_the_dma_streamed_remainder():
    """the streamed remainder's last arriver (gemm_dma.h) runs its own copy of the epilogue: the stream rows carry
    all eight epilogues"""
    epis = {r["epi"] for r in ROWS if gp.row_predict(r)["g"] >= 2}
    assert set(range(8)) <= epis


# ------------------------------------------------------------------------------------------ 3. the float64 references
def test_references_match_float64_torch():
    rng = np.random.default_rng(3)
    A, B = rng.standard_normal((37, 19)), rng.standard_normal((19, 23))
    ta, tb = torch.from_numpy(A), torch.from_numpy(B)
    np.testing.assert_allclose(gp.product("nn", A, B), (ta @ tb).numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(gp.product("nt", A, B.T), (ta @ tb).numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(gp.product("tn", A.T, B), (ta @ tb).numpy(), rtol=0, atol=1e-13)
    for s in (1, 2, 3):                                              # overlapping causal windows against unfold
        Bn, T, C, k = 3, 40, 8, 3
        d = gp._conv(Bn, T, C, k, s)
        X = rng.standard_normal((Bn, T + k - 1, C))
        win = gp.gather(X.ravel(), d, k * C)
        ref = torch.from_numpy(X).unfold(1, k, s).permute(0, 1, 3, 2).reshape(-1, k * C).numpy()
        assert win.shape == ref.shape and np.array_equal(win, ref)
    v = rng.standard_normal((5, 7))
    bias, mask, old = rng.standard_normal(7), rng.standard_normal((5, 7)), rng.standard_normal((5, 7))
    tv, tm, to = torch.from_numpy(v), torch.from_numpy(mask), torch.from_numpy(old)
    want = [tv, tv + torch.from_numpy(bias), torch.relu(tv + torch.from_numpy(bias)), tv * (tm > 0), tv + to, to + tv * (tm > 0),
            torch.relu(to + tv), torch.relu(tv)]
    for epi in range(8):
        assert np.array_equal(gp.apply_epi(v, epi, bias, mask, old), want[epi].numpy()), epi


# ------------------------------------------------------------------------------------------ 4. emulation and mutations
def _pieces(r, p):
    return max(1, min(p["p"], gp.cdiv(r["K"], gp.BK)))


def test_emulation_inside_and_every_mutation_outside():
    uncaught, applied, worst = [], {}, 0.0
    for r in ROWS:
        p = gp.row_predict(r)
        pieces = _pieces(r, p)
        rr = dict(r, emu_pieces=pieces)
        data = {}
        for ds in gp.DATASETS:
            dat = data[ds] = gp.make_rows_data(r, ds)
            if r["M"] == 0 or r["N"] == 0:
                continue
            got = gp.emulate_rows(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask_flat"], dat["c_flat"], r["c"], pieces)
            ok, w, what = gp.judge_rows(r, ds, dat, got, p["p"])
            assert ok, (r["name"], ds, w, what)
            worst = max(worst, w)
        fam = p["kernels"][0].split("<")[0] if p["kernels"] else "none"
        for mut in gp.MUTATIONS:
            if mut == "bias_grad_slice_omitted" or not gp.applies(mut, rr):
                continue
            applied.setdefault(mut, set()).add(fam)
            for ds in ("exact", "normal", "offset"):
                dat = data[ds]
                got = gp.emulate_rows(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask_flat"], dat["c_flat"], r["c"], pieces, mut)
                if not gp.judge_rows(r, ds, dat, got, p["p"])[0]:
                    break
            else:
                uncaught.append((r["name"], mut))
    print("largest err/bound of the clean emulation: %.3f" % worst)
    assert not uncaught, uncaught
    assert worst < 1.0
    fams = {"gemm_rows_kernel", "gemm_rows8_kernel", "gemm_rows_dma_kernel", "gemm_rows_dma8_kernel", "gemm_sk_rows_kernel", "gemm_skp_rows_kernel"}
    for mut in gp.MUTATIONS[:-1]:                                    # every mutation on at least one row of every rows family
        assert fams <= applied[mut], (mut, fams - applied[mut])


def test_tn_emulation_inside_and_every_mutation_outside():
    uncaught, applied = [], set()
    for r in TN:
        p = gp.tn_row_predict(r)
        rr = dict(r, emu_pieces=p["splits"])
        data = {}
        for ds in gp.DATASETS:
            dat = data[ds] = gp.make_tn_data(r, ds)
            c, bg = gp.emulate_tn(dat["A"], dat["B"], dat["c_flat"], r["N"] + r["ldc_pad"], r["accumulate"], dat["old_bg"] if r["bias_grad"] else None, p["rps"])
            ok, w, wg = gp.judge_tn(r, ds, dat, c, bg, p["splits"], p["rps"])
            assert ok, (r["name"], ds, w, wg)
        for mut in gp.MUTATIONS:
            if mut in ("wrap_early", "wrap_late", "mask_dense", "bias_next", "no_relu") or not gp.applies(mut, rr):
                continue
            if mut == "drop_k_step" and gp.cdiv(min(p["rps"], r["M"]), gp.BK) < 3:
                continue
            applied.add(mut)
            for ds in ("exact", "normal", "offset"):
                dat = data[ds]
                c, bg = gp.emulate_tn(dat["A"], dat["B"], dat["c_flat"], r["N"] + r["ldc_pad"], r["accumulate"], dat["old_bg"] if r["bias_grad"] else None,
                                      p["rps"], mut)
                if not gp.judge_tn(r, ds, dat, c, bg, p["splits"], p["rps"])[0]:
                    break
            else:
                uncaught.append((r["name"], mut))
    assert not uncaught, uncaught
    assert {"drop_k_step", "drop_k_tail", "tail_not_zeroed", "col_shift_32", "row_from_0", "no_accum", "slab_twice", "slab_omitted",
            "bias_grad_slice_omitted"} <= applied


# ------------------------------------------------------------------------------------------ 5. the 32-bit extent guards (FAR)
FAR = gp.PATHS["FAR"]
FAR_ROWS = [r for r in FAR if r["kind"] in ("nn", "nt")]
FAR_TN = [r for r in FAR if r["kind"] == "tn"]


def _first_kernel(r):
    p = gp.far_tn_predict(r) if r["kind"] == "tn" else gp.far_row_predict(r)
    return p, p["kernels"][0]


def test_far_limits_are_the_ones_the_source_states():
    """the limits are read from the source text; the rows below were built for these values, and a change of the .hip moves both"""
    L = gp.limits()
    assert (L["a_bytes"], L["b_bytes"], L["job_bytes"]) == (4.0e9, 4.0e9, 4.0e9) and (L["a_pad"], L["b_pad"]) == (64, 16.0)
    assert (L["inner_rpb"], L["inner_rs"], L["inner_wrap"]) == (28, 1 << 25, 1 << 30)
    assert L["a_bytes"] > 2 ** 31, "the fast kernels are allowed byte offsets with bit 31 set: what the FAR rows are there for"


def test_every_far_row_lies_in_its_zone_of_the_guard():
    n = 0
    for r in FAR_ROWS + FAR_TN:
        flop = 2.0 * r["M"] * r["N"] * (r["K1"] if r["kind"] == "tn" else r["K"])
        assert flop <= 4.0e9, r["name"]
        deref = gp.far_deref_bytes(r)
        for op, which in r["far"].items():
            if op == "C":
                c, L = r["c"], gp.limits()
                assert deref["C"] >= 4.5e9, (r["name"], deref)
                wrap = c["bs"] - c["rpb"] * c["rs"] if c["batch"] > 1 else 0
                want = {"wrap-edge-in": (wrap, L["inner_wrap"] - 4), "wrap-edge-out": (wrap, L["inner_wrap"]), "off0": (wrap, L["inner_wrap"] - 4),
                        "rs-edge-in": (c["rs"], L["inner_rs"] - 4), "rs-edge-out": (c["rs"], L["inner_rs"])}[which]
                assert want[0] == want[1], r["name"]
                assert gp.store_inner_ok(c) == (not which.endswith("edge-out")), r["name"]
                if which == "off0":                                 # every block inner and free of a boundary, the second utterance 2^32 bytes on
                    assert c["rpb"] % 32 == 0 and c["bs"] * 4 >= 2 ** 32
                if which.startswith("wrap"):                        # a boundary inside a 32-row block: the select form
                    assert c["rpb"] % 32 != 0 and c["rpb"] >= L["inner_rpb"]
                for o in ("A", "B"):                                # compact: no guard is near
                    assert deref[o] < 2 ** 22
                n += 1
                continue
            g, L = gp.far_guard(r, op)
            step = lambda d: gp.far_guard(dict(r, **d), op)[0]
            if op == "B":
                nb = lambda k: step(dict(ldb_pad=r["ldb_pad"] + k))
            else:
                key = "a" if op in ("A", "X") else "b"
                d0 = r[key]
                nb = lambda k: step({key: dict(d0, bs=d0["bs"] + k) if which == "bs" else dict(d0, rs=d0["rs"] + k)})
            zone = r["zone"]
            if zone == "high":
                assert g < L and deref[op] >= gp.HIGH_BYTES, (r["name"], g, deref)
            elif zone == "edge-in":
                assert g < L <= nb(4), r["name"]
            elif zone == "edge-out":
                assert nb(-4) < L <= g, r["name"]
            else:
                assert zone == "over" and g >= gp.OVER * L, r["name"]
            n += 1
    assert n == len(FAR_ROWS) + len(FAR_TN)
    # SkOuterRows' int arithmetic: a_step = 16 rs >= 2^27 on a row-stride row, a_wrap >= 2^29 on a batch-stride row
    hi = [r for r in FAR_TN if r["zone"] == "high"]
    far_d = lambda r: r["a"] if "X" in r["far"] else r["b"]
    assert any(16 * far_d(r)["rs"] >= 2 ** 27 for r in hi if "rs" in r["far"].values())
    assert any(far_d(r)["bs"] - far_d(r)["rpb"] * far_d(r)["rs"] >= 2 ** 29 for r in hi if "bs" in r["far"].values())
    for r in hi:                                                    # and they stay ints: the last offset plus one step or wrap
        d = far_d(r)
        assert gp.far_layout(d, 1).max() + max(16 * d["rs"], d["bs"] - d["rpb"] * d["rs"] if d["batch"] > 1 else 0) + 128 < 2 ** 31, r["name"]


def test_every_far_row_selects_what_it_names_and_its_compact_twin_the_same():
    seen = set()
    for r in FAR_ROWS + FAR_TN:
        p, k = _first_kernel(r)
        e = r["expect"]
        assert p["family"] == e["family"], (r["name"], p)
        assert k.startswith("gemm_rows_dma_kernel" if e["kernel"] == "stream" else e["kernel"]), (r["name"], k)
        if e.get("stream"):
            assert p["g"] > 1, r["name"]
        t = gp.compact_twin(r)
        pt, kt = _first_kernel(t)
        if r["zone"] in ("high", "edge-in", "c-far"):
            assert (pt["family"], pt["kernels"], pt["launches"], pt.get("g"), pt["p"]) == (p["family"], p["kernels"], p["launches"], p.get("g"), p["p"]), r["name"]
            seen.add(k.split("<")[0] + ("+stream" if p.get("g", 0) > 1 else ""))
        else:
            assert p["family"] == 0 and pt["family"] != 0, (r["name"], "a refusal falls to the register-staged kernels; its twin does not")
    assert seen >= {"gemm_sk_rows_kernel", "gemm_skp_rows_kernel", "gemm_rows_dma_kernel", "gemm_rows_dma8_kernel", "gemm_rows_dma_kernel+stream",
                    "gemm_sk_tn_kernel", "gemm_tn_dma_kernel", "gemm_rows_kernel"}, seen


def test_far_pair_rows_refuse_one_predicate_each():
    rows = [r for r in FAR if r["kind"] == "pair"]
    assert sorted(r["refused"] for r in rows) == ["al_rows", "al_tn"]
    for r in rows:
        M, Co, N, K1 = r["M"], r["Co"], r["N"], r["K1"]
        al_rows, al_tn = gp.pair_al(gp._dense(M, Co), Co, N, r["ldb"], r["x"], K1)
        assert (al_rows, al_tn) == (r["refused"] != "al_rows", r["refused"] != "al_tn"), r["name"]
        ws_nt, ws_tn = max(gp.rows_workspace(M, N, Co, {}), 2 * M * N * 4), gp.tn_workspace(M, K1, Co, {})
        assert gp.pair_plan(M, Co, N, K1, ws_nt, ws_tn, {}) is not None, "the compact twin pairs"
        assert gp.pair_plan(M, Co, N, K1, ws_nt, ws_tn, {}, al_rows, al_tn) is None, r["name"]


def test_far_job_rows_stand_on_both_sides_of_the_limit_and_below_2_32():
    rows = [r for r in FAR if r["kind"] == "job"]
    assert {(r["splits"], r["bias_partials"], r["accumulate"]) for r in rows} == {(s, b, a) for s in (940, 960) for b in (False, True) for a in (0, 1)}
    for r in rows:
        g = gp.job_guard(r["splits"], r["n"])
        assert (g < gp.limits()["job_bytes"]) == (r["zone"] == "high") and g < 2 ** 32 and (r["zone"] == "over" or g >= gp.HIGH_BYTES)
        assert gp.reduce_job_vec_ok(0, r["splits"], r["n"] // r["N"], r["N"], 0, r["N"], r["bias_partials"]) == (r["zone"] == "high")


def test_sparse_reference_and_judge_equal_the_flat_ones_on_small_rows():
    rows = [r for r in ROWS if r["M"] and r["N"] and r["M"] * r["K"] < 1 << 16 and gp.row_predict(r)["kernels"]][::7][:14]
    tns = [r for r in TN if r["M"] * r["K1"] < 1 << 16][:6]
    assert len(rows) + len(tns) == 20
    for r in rows:
        for ds in ("normal", "exact"):
            dat = gp.make_rows_data(r, ds)
            assert np.array_equal(dat["a_flat"][gp.far_layout(r["a"], r["K"])[:, None] + np.arange(r["K"])], dat["A"], equal_nan=True)
            p = gp.row_predict(r)["p"]
            for mut in (None, "drop_k_step", "no_relu"):
                flat = gp.emulate_rows(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask_flat"], dat["c_flat"], r["c"], 1, mut)
                off = gp.far_layout(r["c"], r["N"])
                got = flat[off[:, None] + np.arange(r["N"])]
                changed = int((flat.view(np.int32) != gp.NAN_BITS).sum())
                a, b = gp.judge_rows(r, ds, dat, flat, p), gp.judge_far_rows(r, ds, dat, got, changed, p)
                assert a[0] == b[0] and (a[1] == b[1] or not a[0]), (r["name"], ds, mut, a, b)
            flat = np.array(gp.emulate_rows(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask_flat"], dat["c_flat"], r["c"]))
            gaps = np.ones(flat.size, bool)
            gaps[gp.index(r["c"], r["N"]).ravel()] = False
            if gaps.any():                                          # a gap word written: both judges refuse
                flat[np.flatnonzero(gaps)[0]] = 1.0
                got = flat[gp.far_layout(r["c"], r["N"])[:, None] + np.arange(r["N"])]
                changed = int((flat.view(np.int32) != gp.NAN_BITS).sum())
                assert not gp.judge_rows(r, ds, dat, flat, p)[0] and not gp.judge_far_rows(r, ds, dat, got, changed, p)[0], r["name"]
    for r in tns:
        dat = gp.make_tn_data(r, "normal")
        for d, w, flat, dense in ((r["a"], r["K1"], dat["a_flat"], dat["A"]), (r["b"], r["N"], dat["b_flat"], dat["B"])):
            assert np.array_equal(flat[gp.far_layout(d, w)[:, None] + np.arange(w)], dense, equal_nan=True), r["name"]


def _far_operands(r):
    """(operand, descriptor, columns) of the far operands of a row"""
    out = []
    for op in r["far"]:
        if op == "A":
            out.append((op, r["a"], r["K"]))
        elif op == "B":
            rows, cols = (r["K"], r["N"]) if r["kind"] == "nn" else (r["N"], r["K"])
            out.append((op, dict(batch=1, rpb=rows, rs=gp.ldb_of(r), bs=0), cols))
        elif op == "C":
            out.append((op, r["c"], r["N"]))
            if r["epi"] in gp.EPI_HAS_MASK:
                out.append(("mask", r["c"], r["N"]))
        elif op == "X":
            out.append((op, r["a"], r["K1"]))
        elif op == "dY":
            out.append((op, r["b"], r["N"]))
    return out


def _verdict_under_mistake(r, op, d, cols, mut, dat, pred):
    """(applies, caught, rows that left the allocation, message) for one planted addressing mistake on one far operand"""
    bad = gp.mistaken_offsets(mut, d, cols)
    if bad is None:
        return False, True, 0, ""
    f32 = lambda x: np.asarray(x, np.float32)
    if r["kind"] == "tn":
        dd = dict(dat)
        key = "A" if op == "X" else "B"
        dd[key], left = gp.emulate_far_gather(d, cols, dat[key], bad)
        v, S, g, Sg = gp.tn_reference(r, dict(dat, A=dd["A"], B=dd["B"]))
        got_c = np.array(dat["c_flat"], np.float32)
        got_c[:, :r["N"]] = f32(v)
        ok = gp.judge_tn(r, "normal", dat, got_c, f32(g), pred["splits"], pred["rps"])[0]
    else:
        A, B, mask, old = dat["A"], dat["B"], dat["mask"], dat["old"]
        left = 0
        if op == "A":
            A, left = gp.emulate_far_gather(d, cols, A, bad)
        elif op == "B":
            B, left = gp.emulate_far_gather(d, cols, B, bad)
        elif op == "mask":
            mask, left = gp.emulate_far_gather(d, cols, mask, bad)
        if op == "C" and old is not None:                          # the old values are read through the same mistaken address
            old_read, _ = gp.emulate_far_gather(d, cols, old, bad)
        else:
            old_read = old
        res = f32(gp.rows_reference(r["kind"], A, B, r["epi"], dat["bias"], mask, old_read)[0])
        changed = r["M"] * r["N"]
        if op == "C":
            res, changed, left = gp.emulate_far_scatter(d, cols, res, bad, old)
        ok = gp.judge_far_rows(r, "normal", dat, res, changed, pred["p"])[0]
    return True, not ok, left, "%s: %s of %s not caught" % (r["name"], mut, op)


def test_every_planted_addressing_mistake_becomes_a_wrong_number_inside_the_allocation():
    """the buffer layout of tests/far_buffers.py ([2^31 + 256 bytes][extent][256 bytes], NaN everywhere but the payload): each
    addressing mistake, planted in an emulated gather (inputs) or scatter (C), is rejected by the judge on every row it can change,
    and no mistaken row leaves the allocation"""
    pairs, uncaught, seen = 0, [], set()
    for r in FAR_ROWS + FAR_TN:
        if r["zone"] not in ("high", "edge-in", "c-far") or (r["kind"] != "tn" and r["M"] * r["K"] > 1 << 18 and "A" not in r["far"]):
            continue
        t = gp.compact_twin(r)
        dat = gp.make_tn_data(t, "normal") if r["kind"] == "tn" else gp.make_rows_data(t, "normal")
        pred = gp.far_tn_predict(r) if r["kind"] == "tn" else gp.far_row_predict(r)
        for op, d, cols in _far_operands(r):
            for mut in gp.ADDRESSING_MISTAKES:
                applies, caught, left, msg = _verdict_under_mistake(r, op, d, cols, mut, dat, pred)
                if not applies:
                    continue
                pairs += 1
                seen.add(mut)
                assert left == 0, "%s: %s of %s leaves the allocation (%d rows)" % (r["name"], mut, op, left)
                if not caught:
                    uncaught.append(msg)
    print("%d (row, operand, mistake) pairs, mistakes met: %s" % (pairs, sorted(seen)))
    assert not uncaught, uncaught
    # element_offset_mod_2^31 needs an element offset of 2^31 (8.6 GB behind the base): beyond the rows' 32 GiB budget, it changes none
    assert seen == set(gp.ADDRESSING_MISTAKES) - {"element_offset_mod_2^31"} and pairs >= 60
