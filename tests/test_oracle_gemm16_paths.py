"""
Pins oracle/gemm16_paths_np.py on the CPU (no device, no launches):
  1. the restated host functions against lidbox_gemm_bf16_plan_query and the workspace exports (lidbox_gemm_bf16_rows_workspace,
     _bf16_tn_workspace, _bf16s_tn_workspace) over the PATHS rows and a grid of a few thousand shapes and descriptors, under every
     environment a row sets;
  2. every PATHS row selects what its `why` says, the rows together reach the kernel instantiations the launch sites of
     gemm_bf16.hip name (enumerated from the source text by g.instantiations_from_source), none missing, and the tables hold every
     edge of the EDGES list;
  3. the float64 references and the bf16 rounding helpers against torch;
  4. the fp32 emulation of every row lies inside the bounds on `normal` and `offset` and equals int64 on `exact` (fp32 and shadow),
     the bounds are below half a bf16 ulp of typical outputs, and every planted mutation is caught on every row it applies to
     (g.applies: the explicit exclusion rules): zero uncaught pairs.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import conv2d_np
from oracle import gemm_paths_np as gp
from oracle import gemm16_paths_np as g

ROWS16, TN16, ROWS16S, TN16S = (g.PATHS[k] for k in ("ROWS16", "TN16", "ROWS16S", "TN16S"))
ROWS, TN = ROWS16 + ROWS16S, TN16 + TN16S

BIG, BIGTN, PAIR, CARRY = (g.PATHS[k] for k in ("BIG16S", "BIGTN16S", "PAIR16S", "CARRY16S"))


@pytest.fixture(scope="module")
def lib():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native.lib


def _setenv(monkeypatch, env):
    for k in list(os.environ):
        if k.startswith("LIDBOX_GEMM"):
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _envs():
    seen, out = set(), []
    extra = [{}, {"LIDBOX_GEMM16S_DMA": "64,64"}, {"LIDBOX_GEMM16S_DMA": "128,128,4"}, {"LIDBOX_GEMM16S_DMA": "256,64,2"}, {"LIDBOX_GEMM16S_DMA": "64,64,2,0"},
             {"LIDBOX_GEMM16S_DMA": "64, 128,3,2"}, {"LIDBOX_GEMM16S_KRES": "0"}, {"LIDBOX_GEMM16_TN_PP": "0"}, {"LIDBOX_GEMM16_TN_KRES": "0"}]
    for r in [dict(env=e) for e in extra] + ROWS + TN + g.PATHS["CARRY16S"]:
        key = tuple(sorted(r["env"].items()))
        if key not in seen:
            seen.add(key)
            out.append(dict(r["env"]))
    return out


def _rows_struct(d, res=0):
    from lidbox_amd import _native as nv
    if d is None:
        return nv.Rows(None, 0, 0, 0, 0)
    return nv.Rows(0x10000 + res, d["bs"], d["rs"], d["batch"], d["rpb"])


def _export(lib, kind, a, b, c, K, N, epi, wsb, has_ws=True, res=None, c_null=False, shadow=True, mask16=False, njobs=0, bias_grad=True, ldb=None):
    """lidbox_gemm_bf16_plan_query with fake (never dereferenced) pointers that carry the residues"""
    from lidbox_amd import _native as nv
    res = res or {}
    A = _rows_struct(a, res.get("A", 0))
    B = nv.Rows(0x20000 + res.get("B", 0), 0, ldb, 1, 0) if kind in (g.Q16_NN, g.Q16_NT, g.Q16S_NT) else _rows_struct(b, res.get("B", 0))
    C = _rows_struct(c, res.get("C", 0))
    c16 = None
    if kind == g.Q16S_NT:
        c16 = (0x30000 + res.get("C16", 0)) if shadow else None
        if c_null:
            C.base = None
    aux = (0x40000 + res.get("bg", 0)) if (kind in (g.Q16_TN, g.Q16S_TN) and bias_grad) else None
    out = (ctypes.c_long * 12)()
    flags = epi | (g.EPI_MASK_BF16 if mask16 else 0)
    ws = (0x50000 + res.get("ws", 0)) if has_ws else None
    assert lib.lidbox_gemm_bf16_plan_query(kind, A, B, C, c16, K, N, flags, aux, njobs, ws, wsb, out) == 0
    return list(out)


def _row_export(lib, r, wsb):
    kind = g.Q16S_NT if r["fam"] == "s" else (g.Q16_NT if r["kind"] == "nt" else g.Q16_NN)
    return _export(lib, kind, r["a"], None, r["c"], r["K"], r["N"], r["epi"], wsb, has_ws=wsb > 0, res=r["res"], c_null=r["out"] == "shadow",
                   shadow=r["out"] != "f32", mask16=r["mask16"], ldb=g.ldb_of(r))


def _tn_row_export(lib, r, wsb):
    c = dict(batch=1, rpb=r["K1"], rs=r["N"] + r["ldc_pad"], bs=0)
    return _export(lib, g.Q16S_TN if r["fam"] == "s" else g.Q16_TN, r["a"], r["b"], c, r["K1"], r["N"], 0, wsb, res=r["res"], bias_grad=r["bias_grad"])


def _grid():
    """shapes and descriptors: (a, c, K, N) for the rows kinds, (a, b, K1, N) for the wgrads"""
    rng = np.random.default_rng(16)
    rows, tns = [], []
    Ms = [1, 7, 64, 130, 257, 1000, 2112, 8448, 25344, 49153, 65537, 131072]
    for _ in range(260):
        M, N, K = int(rng.choice(Ms)), int(rng.choice([8, 36, 64, 72, 128, 256, 512, 1500, 1504, 3000])), int(rng.choice([8, 16, 40, 72, 200, 208, 216, 512, 520, 1024, 1500, 1536, 3072]))
        rows.append((gp._dense(M, K, int(rng.choice([0, 8]))), gp._dense(M, N, int(rng.choice([0, 4]))), K, N))
    for _ in range(120):                                           # windows of utterances: the K-resident kernels' ground
        batch, rpb, rs, K = int(rng.choice([1, 2, 7, 64, 600])), int(rng.choice([1, 31, 32, 33, 65, 199])), int(rng.choice([8, 16, 40, 48, 200])), int(rng.choice([16, 40, 200, 208, 216]))
        a = dict(batch=batch, rpb=rpb, rs=rs, bs=(rpb - 1) * rs + K + int(rng.choice([0, 8, 4])))
        N = int(rng.choice([64, 72, 512, 76]))
        c = gp._batched(batch, rpb, N, int(rng.choice([0, 4, 2])), 8) if rng.random() < 0.6 else gp._dense(batch * rpb, N)
        rows.append((a, c, K, N))
        b = gp._batched(batch, int(rng.choice([rpb, rpb, rpb + 1])) if batch > 1 else rpb, int(rng.choice([128, 512, 72])), 0, 0)
        if b["batch"] * b["rpb"] == batch * rpb:
            tns.append((a, b, K, b["rs"]))
    for _ in range(200):
        M, K1, N = int(rng.choice(Ms + [4096, 8192, 101000])), int(rng.choice([8, 20, 40, 136, 200, 224, 232, 256, 512, 1500, 1536])), int(rng.choice([8, 36, 128, 256, 512, 640, 1500, 1536, 4096]))
        tns.append((gp._dense(M, (K1 + 7) // 8 * 8), gp._dense(M, (N + 7) // 8 * 8), K1, N))
    return rows, tns


# ------------------------------------------------------------------------------------------ 1. restated host functions
def test_restated_dispatch_matches_the_export(lib, monkeypatch):
    rows, tns = _grid()
    n = 0
    for env in _envs():
        _setenv(monkeypatch, env)
        for a, c, K, N in rows:
            M = a["batch"] * a["rpb"]
            assert lib.lidbox_gemm_bf16_rows_workspace(M, N, K) == g.rows_workspace16(M, N, K), (M, N, K)
            for wsb in (0, 3 * M * N * 4, 1 << 34):
                for kind in (g.Q16_NN, g.Q16_NT):
                    want = g.plan_query(kind, a, None, c, K, N, 0, env, wsb, has_ws=wsb > 0, ldb=(N if kind == g.Q16_NN else K) + 4)
                    assert _export(lib, kind, a, None, c, K, N, 0, wsb, has_ws=wsb > 0, ldb=(N if kind == g.Q16_NN else K) + 4) == want, (env, kind, a, c, K, N, wsb)
                for epi, c_null, mask16, njobs in ((0, False, False, 0), (gp.EPI_BIAS_RELU, True, False, 0), (gp.EPI_RELU_MASK, False, True, 0), (gp.EPI_ACCUM, False, False, 1)):
                    kw = dict(has_ws=wsb > 0, c_null=c_null, mask16=mask16, njobs=njobs, ldb=K + 8)
                    want = g.plan_query(g.Q16S_NT, a, None, c, K, N, epi, env, wsb, **kw)
                    assert _export(lib, g.Q16S_NT, a, None, c, K, N, epi, wsb, **kw) == want, (env, a, c, K, N, wsb, kw)
                    n += 1
        for a, b, K1, N in tns:
            M = a["batch"] * a["rpb"]
            assert lib.lidbox_gemm_bf16_tn_workspace(M, K1, N) == g.tn_workspace16(M, K1, N), (M, K1, N)
            lw = g.tn_workspace16s(M, K1, N, env)
            assert lib.lidbox_gemm_bf16s_tn_workspace(M, K1, N) == lw, (env, M, K1, N)
            c = dict(batch=1, rpb=K1, rs=N, bs=0)
            for wsb in (lw, lw - 1, (K1 * N + N) * 4):
                for kind in (g.Q16_TN, g.Q16S_TN):
                    for res in ({}, {"C": 4}):
                        want = g.plan_query(kind, a, b, c, K1, N, 0, env, wsb, res=res)
                        assert _export(lib, kind, a, b, c, K1, N, 0, wsb, res=res) == want, (env, kind, a, b, K1, N, wsb, res)
                        n += 1
    print("%d planner queries compared" % n)
    assert n >= 3000


def test_every_row_matches_the_export(lib, monkeypatch):
    for r in ROWS + BIG + [p_ for r in PAIR for p_ in (r["p0"], r["p1"])]:
        _setenv(monkeypatch, r["env"])
        wsb = g.row_ws_bytes(r)
        assert _row_export(lib, r, wsb) == g.row_query(r, wsb), r["name"]
    for r in TN + BIGTN:
        _setenv(monkeypatch, r["env"])
        wsb = g.tn_row_ws_bytes(r)
        assert _tn_row_export(lib, r, wsb) == g.tn_row_query(r, wsb), r["name"]
        if r["ws"] == "lib":
            M, K1, N = r["M"], r["K1"], r["N"]
            assert wsb == (lib.lidbox_gemm_bf16s_tn_workspace(M, K1, N) if r["fam"] == "s" else lib.lidbox_gemm_bf16_tn_workspace(M, K1, N)), r["name"]


def test_alignment_refusals_term_by_term(lib):
    """each term of the three families' operand checks false on its own -> LIDBOX_K16_REFUSED, in the export and the restatement"""
    a, c = gp._dense(65, 72), gp._dense(65, 72)
    ok = dict(a=a, c=c, K=72, N=72, ldb=72, res={})
    cases16 = [dict(res={"A": 4}), dict(a=gp._dense(65, 72, 2)), dict(a=gp._batched(5, 13, 72, 0, 2)), dict(res={"C": 4}), dict(c=gp._dense(65, 72, 2)), dict(K=70),
               dict(res={"B": 4}), dict(ldb=74), dict(res={"ws": 4})]
    for kind in (g.Q16_NN, g.Q16_NT):
        assert _export(lib, kind, a, None, c, 72, 72, 0, 64, ldb=72)[0] == g.K_ROWS
        for ch in cases16 + ([dict(N=70, c=gp._dense(65, 70, 2))] if kind == g.Q16_NN else []):
            q = dict(ok, **ch)
            args = (kind, q["a"], None, q["c"], q["K"], q["N"], 0)
            got = _export(lib, *args, 64, res=q["res"], ldb=q["ldb"])
            assert got[0] == g.K_REFUSED and got == g.plan_query(*args, {}, 64, res=q["res"], ldb=q["ldb"]), (kind, ch)
    cases16s = [dict(res={"A": 8}), dict(a=gp._dense(65, 72, 4)), dict(a=gp._batched(5, 13, 72, 0, 4)), dict(res={"C": 4}), dict(c=gp._dense(65, 72, 2)), dict(K=76),
                dict(res={"B": 8}), dict(ldb=76), dict(res={"ws": 4}), dict(res={"C16": 1})]
    for ch in cases16s:
        q = dict(ok, **ch)
        args = (g.Q16S_NT, q["a"], None, q["c"], q["K"], q["N"], 0)
        got = _export(lib, *args, 64, res=q["res"], ldb=q["ldb"])
        assert got[0] == g.K_REFUSED and got == g.plan_query(*args, {}, 64, res=q["res"], ldb=q["ldb"]), ch
    b = gp._dense(65, 40)
    cd = dict(batch=1, rpb=72, rs=40, bs=0)
    for kind, cases in ((g.Q16_TN, [dict(res={"A": 4}), dict(a=gp._dense(65, 72, 2)), dict(res={"B": 4}), dict(b=gp._dense(65, 40, 2)), dict(res={"ws": 4})]),
                        (g.Q16S_TN, [dict(res={"A": 8}), dict(a=gp._dense(65, 72, 4)), dict(res={"B": 8}), dict(b=gp._dense(65, 40, 4)), dict(res={"ws": 4}),
                                     dict(a=gp._dense(65, 68), K1=68)])):
        assert _export(lib, kind, a, b, cd, 72, 40, 0, 1 << 20)[0] in (g.K_TN, g.KS_TN)
        for ch in cases:
            q = dict(a=a, b=b, K1=72, res={})
            q.update(ch)
            args = (kind, q["a"], q["b"], dict(cd, rpb=q["K1"]), q["K1"], 40, 0)
            got = _export(lib, *args, 1 << 20, res=q["res"])
            assert got[0] == g.K_REFUSED and got == g.plan_query(*args, {}, 1 << 20, res=q["res"]), (kind, ch)


def test_tail_split_restated_on_the_smallest_shape_that_takes_it(lib, monkeypatch):
    """the tail split of both families at the smallest shape that takes it (the BIG16S rows run it on the device): the plan against the export"""
    for fam, kind in (("c", g.Q16_NT), ("s", g.Q16S_NT)):
        M, N, K = g.smallest_tail_split(fam)
        a, c = gp._dense(M, K), gp._dense(M, N)
        env = {} if fam == "c" else {"LIDBOX_GEMM16S_DMA": "0"}
        _setenv(monkeypatch, env)
        for wsb in (1 << 30, 0):
            got = _export(lib, kind, a, None, c, K, N, 0, wsb, has_ws=wsb > 0, ldb=K)
            assert got == g.plan_query(kind, a, None, c, K, N, 0, env, wsb, has_ws=wsb > 0, ldb=K)
            assert (got[6] == M - 1 and got[7] > 1 and got[9] == g.R_ROWS) if wsb else got[6] == 0, got
        # one row fewer: no remainder tile; K below TAIL_MIN_K: off
        assert _export(lib, kind, gp._dense(M - 1, K), None, gp._dense(M - 1, N), K, N, 0, 1 << 30, ldb=K)[6] == 0
        assert _export(lib, kind, gp._dense(M, K - 8), None, c, K - 8, N, 0, 1 << 30, ldb=K)[6] == 0
        # rem_tiles == slots / 4 is taken, one tile more is not
        slots = 512
        for rem_tiles, taken in ((slots // 4, True), (slots // 4 + 1, False)):
            Mq = (slots + rem_tiles) * 128
            q = g.plan_query(kind, gp._dense(Mq, K), None, gp._dense(Mq, N), K, N, 0, env, 1 << 34, ldb=K)
            assert (q[6] > 0) == taken and q == _export(lib, kind, gp._dense(Mq, K), None, gp._dense(Mq, N), K, N, 0, 1 << 34, ldb=K), (fam, rem_tiles, q)


def test_choose_dma16_policy_branches_and_pp2(lib):
    """one shape per branch of choose_dma16 without an environment (the BIG16S rows run them on the device), the writes_fp32 exception on
    each side, and pp2_problem's conditions"""
    want = {"t128_small": (130, 72, 520), "default_64x128": (8129, 132, 72), "just_over_64x64": (49153, 8, 72), "k1536_128x128": (24577, 256, 1536),
            "pp_three_quarters": (256 * 192, 256, 512), "pp_half_round": (256 * 128, 256, 1504)}
    for br, (M, N, K) in want.items():
        assert g.dma_branch(M, N, K, False) == br, br
        a, c = gp._dense(M, K), gp._dense(M, N)
        for c_null in (False, True):
            got = _export(lib, g.Q16S_NT, a, None, c, K, N, 0, 0, has_ws=False, c_null=c_null, ldb=K)
            assert got == g.plan_query(g.Q16S_NT, a, None, c, K, N, 0, {}, 0, has_ws=False, c_null=c_null, ldb=K), (br, c_null)
    # writes_fp32 && K < 1024 && t256 > NUM_CU keeps the small tiles; K >= 1024 or a shadow-only output take the ping-pong tile
    M, N = 256 * 384, 256
    assert g.choose_dma16(M, N, 512, 0, True, {})["bm"] != 256 and g.choose_dma16(M, N, 512, 0, False, {})["bm"] == 256
    assert g.choose_dma16(M, N, 1024, 0, True, {})["bm"] == 256 and g.choose_dma16(256 * 256, N, 512, 0, True, {})["bm"] == 256
    call = dict(a=gp._dense(256 * 192, 512), c=gp._dense(256 * 192, 256), K=512, N=256, epi=gp.EPI_RELU_MASK, mask16=True)
    assert all(g.pp2_conditions(call, 0, {}).values())
    for ch, term in ((dict(a=gp._dense(256 * 64, 512), c=gp._dense(256 * 64, 256)), "pp256_unsplit"), (dict(epi=gp.EPI_RELU), "mask16_epi"),
                     (dict(c_null=True, epi=gp.EPI_ACCUM_RELU_MASK), "shadow_only_ok"), (dict(a_res=8), "aligned"),
                     (dict(a=dict(batch=256 * 192, rpb=1, rs=8, bs=8), K=16, mask16=False, epi=0), "not_kres")):
        cond = g.pp2_conditions(dict(call, **ch), 0, {})
        assert not cond[term] and sum(not v for v in cond.values()) <= 2, (term, cond)


# ------------------------------------------------------------------------------------------ 2. the rows select their paths
@pytest.mark.parametrize("r", ROWS + BIG, ids=[r["name"] for r in ROWS + BIG])
def test_rows_row_selects_its_path(r):
    q, e = g.row_query(r), r["expect"]
    assert q[0] == e["kernel"], q
    if "m_main" in e:
        assert q[6] == e["m_main"] and q[7] == e.get("rem_splits", 0), q
    if "tile" in e and e["tile"][0]:
        assert tuple(q[1:4]) == e["tile"], q
    if "splits" in e:
        assert q[4] == e["splits"] and (q[4] - 1) * q[5] < r["K"], q
    if "kps" in e:
        assert q[5] == e["kps"], q
    if "branch" in e:
        assert g.dma_branch(r["M"], r["N"], r["K"], r["out"] != "shadow") == e["branch"]
    if r["name"].startswith("kres-refuse-"):                     # exactly one condition of `can` fails
        cond = g.kres_conditions(r["a"], r["c"], r["K"], r["N"], r["epi"], r["mask16"], False, 0, r["res"].get("C16", 0) if r["out"] != "f32" else 0)
        failed = {k for k, v in cond.items() if not v}           # (a mask comes with a mask epilogue, which epi_ok refuses as well)
        assert failed == ({"no_mask16", "epi_ok"} if r["mask16"] else failed) and len(failed) == (2 if r["mask16"] else 1), cond
    # each row stays small; the BIG16S rows (judged on sampled rows) stay below 60 GFLOP and 340 MB per operand (the fp32 A of tail-c-quarter+1)
    if r["table"] == "BIG16S":
        assert 2.0 * r["M"] * r["N"] * r["K"] <= 6.0e10 and r["M"] * r["K"] * (2 if r["fam"] == "s" else 4) <= 3.4e8
    else:
        assert 2.0 * r["M"] * r["N"] * r["K"] <= 1.0e9 and r["M"] * max(r["K"], r["N"]) <= 8e6


def test_pair_rows_select_their_path():
    """both problems of a qualifying pair pass every pp2_problem condition; a non-qualifying row fails exactly one kind of condition"""
    for r in PAIR:
        conds = []
        for p_ in (r["p0"], r["p1"]):
            a_ = dict(p_["a"], batch=0) if p_.get("empty") else p_["a"]
            call = dict(a=a_, c=p_["c"], K=p_["K"], N=p_["N"], epi=p_["epi"], c_null=p_["out"] == "shadow")
            conds.append(g.pp2_conditions(call, 2 * p_["M"] * p_["N"] * 4 if r["ws"] else 0, r["env"]))
        ok = all(all(c.values()) for c in conds) and "LIDBOX_GEMM_NO_CARRY" not in r["env"]
        assert ok == r["pair"], (r["name"], conds)
        failed = {k for c in conds for k, v in c.items() if not v}
        assert len(failed) <= 1, (r["name"], failed)
    assert {True, False} <= {r["p1"]["K"] > r["p0"]["K"] for r in PAIR if r["pair"]}, "swap both ways"
    assert any(r["pair"] and r["zero"] and not r["ws"] for r in PAIR)
    # every term of pp2_problem that can fail alone and still run as two calls has a row (g.UNREACHED holds the others with the proof)
    alone = set()
    for r in PAIR:
        for p_ in (r["p0"], r["p1"]):
            a_ = dict(p_["a"], batch=0) if p_.get("empty") else p_["a"]
            c_ = g.pp2_conditions(dict(a=a_, c=p_["c"], K=p_["K"], N=p_["N"], epi=p_["epi"], c_null=p_["out"] == "shadow"), 2 * p_["M"] * p_["N"] * 4 if r["ws"] else 0, r["env"])
            alone |= {k for k, v in c_.items() if not v}
    assert alone == {"nonempty", "not_kres", "pp256_unsplit"}, alone
    kres = next(r for r in PAIR if r["name"] == "pair-kres")
    assert all(g.row_query(p_)[0] == g.KS_KRES13 for p_ in (kres["p0"], kres["p1"])), "both problems of pair-kres run on the K-resident kernel as single calls"


def test_shadow_vector_store_rule_names_the_rows_of_the_scratch_build():
    """g.shadow_through_vector_store: the rows whose shadow goes through the 16-byte store of pp_store_tile -- the 32 small rows (and the
    four ping-pong row-block cases of the GPU module) that the truncating scratch build of LAB_NOTEBOOK section 24 failed, no others"""
    hit = [r["name"] for r in ROWS16S if g.shadow_through_vector_store(r, g.row_query(r))]
    assert len(hit) == 32, hit
    for r in ROWS16S:
        q = g.row_query(r)
        if g.shadow_through_vector_store(r, q):
            assert r["out"] != "f32" and q[4] == 1 and (q[0] == g.KS_PP or (q[0] == g.KS_DMA and q[2] == 128 and r["epi"] in (3, 4, 5, 6))), r["name"]
        if q[0] == g.KS_PP and r["out"] != "f32" and q[4] == 1:
            assert g.shadow_through_vector_store(r, q), r["name"]


@pytest.mark.parametrize("r", TN + BIGTN, ids=[r["name"] for r in TN + BIGTN])
def test_tn_row_selects_its_path(r):
    q, e = g.tn_row_query(r), r["expect"]
    assert q[10] == 1, "the row's workspace holds its slices"
    for k, i in (("kernel", 0), ("splits", 4), ("rps", 5), ("reduce", 9), ("ups", 11)):
        if k in e:
            assert q[i] == e[k], (k, q)
    if r["name"].startswith("s-tn-kres-refuse-"):
        cond = g.tn_kres_conditions(r["a"], r["b"], r["K1"], r["N"], g.plan_tn16_kres(r["M"], r["K1"], r["N"], r["env"]))
        want = {"rpb": {"same_rpb", "same_batch"}, "bs-whole": {"bs_whole"}, "bs-covers": {"bs_covers"}, "img": {"img_elems", "img_bytes"}}[r["name"].split("refuse-")[1]]
        assert {k for k, v in cond.items() if not v} <= want and not all(cond.values()), cond
    if r["name"] == "s-tn-pp-policy-short":
        pp = g.plan_tn16_pp(r["M"], r["K1"], r["N"], r["env"])
        assert not pp["use"] and pp["rps"] < 2048 and g.plan_tn16_pp(r["M"] + 128, r["K1"], r["N"], r["env"])["use"], pp
    elif r["name"].startswith("s-tn-pp-") and e["kernel"] == g.KS_TN:
        cond = g.tn_pp_conditions(r["a"], r["b"], r["K1"], r["N"])
        assert sum(not v for v in cond.values()) == 1 and g.plan_tn16_pp(r["M"], r["K1"], r["N"], r["env"])["use"], cond
    assert 2.0 * r["M"] * r["N"] * r["K1"] <= (7.0e10 if r["table"] == "BIGTN16S" else 6.0e9)


def _reached():
    got = set()
    for r in ROWS + BIG:
        q = g.row_query(r)
        if q[0] > 0:
            got.add(g.kernel_name(q, g.Q16_NT if r["kind"] == "nt" else g.Q16_NN))
            if q[9] == g.R_ROWS:
                got.add("rows_reduce_kernel")
    if any(r["pair"] for r in PAIR):
        got.add("gemm16s_rows_pp2_kernel<256,2>")
    for r in TN + BIGTN:
        q = g.tn_row_query(r)
        got.add(g.kernel_name(q))
        if q[9] == g.R_JOB4:
            got.add("splitk_reduce4_kernel")
    kinds = {r["kind"] for r in g.PATHS["CONVERT"]}
    if "convert" in kinds:
        got.update(["f32_to_bf16_kernel", "bf16_to_f32_kernel"])
    if "transpose" in kinds:
        got.add("transpose_f32_to_bf16_kernel")
    if "refresh" in kinds:
        got.add("refresh_bf16_weights_kernel")
    return got


def test_rows_reach_the_instantiations_the_launch_sites_name():
    inst = g.instantiations_from_source()
    print("%d instantiations named by the launch sites of gemm_bf16.hip" % len(inst))
    assert len(inst) == len(set(inst)) == 29
    per = {}
    for k in inst:
        per[k.split("<")[0]] = per.get(k.split("<")[0], 0) + 1
    assert per["gemm16s_rows_dma_kernel"] == 9 and per["gemm16s_rows_pp_kernel"] == 4 and per["gemm16s_rows_kres_kernel"] == 2 and per["gemm16_rows_kernel"] == 2
    assert {k for k in inst if k.startswith("gemm16s_rows_dma_kernel")} == {"gemm16s_rows_dma_kernel<%d,%d,%d>" % t for t in g.DMA_TILES}
    missing = set(inst) - _reached()
    assert not missing, sorted(missing)


EDGES = {
    "every forced tile at M in {1, bm - 1, bm + 1, 2 bm + 3}": lambda: all(
        {1, (bm or 128) - 1, (bm or 128) + 1, 2 * (bm or 128) + 3} <= {r["M"] for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-e" % (bm, bn, st))}
        for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]),
    "every forced tile at N = 36 and N = 8 and every N % bn != 0": lambda: all(
        {36, 8} <= {r["N"] for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-e" % (bm, bn, st))} and
        all(r["N"] % (bn or 128) for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-e" % (bm, bn, st))) for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]),
    "every forced tile at K = 8 and every K tail 8 .. 56": lambda: all(
        8 in {r["K"] for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-e" % (bm, bn, st))} and
        {8, 16, 24, 32, 40, 48, 56} <= {r["K"] % 64 for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-e" % (bm, bn, st)) and r["K"] > 64}
        for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]),
    "every forced tile with every epilogue": lambda: all(
        set(range(8)) <= {r["epi"] for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-" % (bm, bn, st))} for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]),
    "every forced tile with fp32 only, fp32 + shadow, shadow only and a bf16 mask": lambda: all(
        {("f32", False), ("both", False), ("shadow", False)} <= {(r["out"], r["mask16"]) for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-" % (bm, bn, st))} and
        any(r["mask16"] for r in ROWS16S if r["name"].startswith("tile-%d.%d.%d-" % (bm, bn, st))) for bm, bn, st in g.DMA_TILES + g.PP_TILES + [(0, 0, 0)]),
    "a forced K split with a short last split, and one the rounding leaves with fewer splits, on every DMA and ping-pong tile": lambda: all(
        any(r["name"] == "tile-%d.%d.%d-split3-%s" % (bm, bn, st, s) for r in ROWS16S) for bm, bn, st in g.DMA_TILES + g.PP_TILES for s in ("short", "fewer")),
    "K-resident forward: rows_per_batch 1, 31, 32, 33, 65; both instantiations; both output forms; units above and below 12": lambda: (
        {1, 31, 32, 33, 65} <= {r["a"]["rpb"] for r in ROWS16S if r["name"].startswith("kres-K")} and
        {g.KS_KRES13, g.KS_KRES0} <= {r["expect"]["kernel"] for r in ROWS16S} and {16, 40, 200, 208} <= {r["K"] for r in ROWS16S if r["name"].startswith("kres-K")} and
        {True, False} <= {r["c"]["batch"] == 1 for r in ROWS16S if r["name"].startswith("kres-K")} and
        {True, False} <= {r["a"]["batch"] * gp.cdiv(r["a"]["rpb"], 32) > 12 for r in ROWS16S if r["name"].startswith("kres-K")}),
    "K-resident forward: each refusal": lambda: {"N%8", "C16%8", "Cbatch", "mask", "epi", "rs-long"} <= {r["name"][12:] for r in ROWS16S if r["name"].startswith("kres-refuse-")},
    "compute family: splits 1, 2, 64, cut by the workspace, none; nt with N % 4 != 0 and the nn refusal": lambda: (
        {1, 2, 3, 64} <= {r["expect"].get("splits") for r in ROWS16} and {"lib", "plan-1", "one-1", "none"} <= {r["ws"] for r in ROWS16} and
        any(r["N"] % 4 and r["expect"]["kernel"] == g.K_ROWS for r in ROWS16) and any(r["expect"]["kernel"] == g.K_REFUSED for r in ROWS16)),
    "storage wgrad: slices 1, 2; target NUM_CU against 2 NUM_CU; ragged last slice; padded rows; both reduces; accumulate and bias_grad both ways": lambda: (
        {1, 2, 16, 22} <= {r["expect"].get("splits") for r in TN16S} and any(r["M"] % 64 for r in TN16S) and any(r["K1"] % 8 and r["N"] % 8 for r in TN16S) and
        {g.R_JOB4, g.R_SCALAR} <= {g.tn_row_query(r)[9] for r in TN16S} and {0, 1} <= {r["accumulate"] for r in TN16S} and {True, False} <= {r["bias_grad"] for r in TN16S}),
    "storage wgrad: ping-pong and K1-resident kernels forced, ups > 1, batch < max_slices, the small workspace": lambda: (
        {g.KS_TN_PP, g.KS_TN_KRES} <= {r["expect"]["kernel"] for r in TN16S} and any(r["expect"].get("ups", 0) > 1 for r in TN16S) and any(r["ws"] == "fallback" for r in TN16S)),
    "K-resident forward by policy: <13> and <0> selected, one utterance short and a long row stride not": lambda: (
        {g.KS_KRES13, g.KS_KRES0, g.KS_DMA} <= {r["expect"]["kernel"] for r in ROWS16S if r["name"].startswith("kres-policy-")} and
        all(not r["env"] for r in ROWS16S if r["name"].startswith("kres-policy-"))),
    "a carried job keeps a call off the K-resident kernel": lambda: any(r["kres"] for r in CARRY),
    "choose_dma16 by policy on the device: both ping-pong conditions with a neighbour on the other side, the writes_fp32 exception on each side, K >= 1536": lambda: (
        {"pp_three_quarters", "pp_half_round", "default_64x128", "k1536_128x128"} <= {r["expect"].get("branch") for r in BIG} and
        {"policy-fp32-exception", "policy-fp32-exception-shadow", "policy-fp32-exception-K1024", "policy-pp-3q-less", "policy-pp-half-K"} <= {r["name"] for r in BIG}),
    "the tail split on and off at TAIL_MIN_K, at rem_tiles == slots / 4 and one more, both families": lambda: (
        {("s", True), ("s", False), ("c", True), ("c", False)} <= {(r["fam"], r["expect"]["m_main"] > 0) for r in BIG if "m_main" in r["expect"]} and
        {"tail-s-K", "tail-c-K", "tail-s-quarter", "tail-s-quarter+1", "tail-s-nows"} <= {r["name"] for r in BIG}),
    "the ping-pong wgrad by policy, and one slice length short of it": lambda: {g.KS_TN_PP, g.KS_TN} <= {r["expect"]["kernel"] for r in BIGTN},
    "refresh: flat16 NULL and set, vec on, each of its five conditions off alone, plain and transposed, padded ld_dst, 49 matrices, n % 4 != 0": lambda: (
        {True, False} <= {r["flat16"] for r in g.PATHS["CONVERT"] if r["kind"] == "refresh"} and
        {"refresh-novec-%s-t%d" % (n, t) for n in ("cols", "offset", "ld_dst", "dst") for t in (0, 1)} | {"refresh-novec-rows-t1", "refresh-vec-t0", "refresh-vec-t1"}
        <= {r["name"] for r in g.PATHS["CONVERT"]} and
        all(sum(1 for _ in [0]) and [m["vec"] for m in g.refresh_layout(r)[1]] == [False] for r in g.PATHS["CONVERT"] if r["name"].startswith("refresh-novec")) and
        any(len(r["mats"]) == 49 for r in g.PATHS["CONVERT"] if r["kind"] == "refresh") and any(g.refresh_layout(r)[0] % 4 for r in g.PATHS["CONVERT"] if r["kind"] == "refresh")),
    "carry: one and two jobs, NO_CARRY, CARRY_BLOCKS 7 and 8, M = 0, the zero job without a workspace": lambda: (
        {"w", "wz", "z"} <= {r["jobs"] for r in g.PATHS["CARRY16S"]} and {"7", "8"} <= {r["env"].get("LIDBOX_GEMM_CARRY_BLOCKS") for r in g.PATHS["CARRY16S"]} and
        any("LIDBOX_GEMM_NO_CARRY" in r["env"] for r in g.PATHS["CARRY16S"]) and any(r["M"] == 0 for r in g.PATHS["CARRY16S"]) and
        any(r["nows"] and r["jobs"] == "z" for r in g.PATHS["CARRY16S"])),
    "converters: n of 0, 1, 3, 4, 5, 1023 and one past the grid cap; transposes of 1, 31, 32, 33": lambda: (
        {0, 1, 3, 4, 5, 1023} <= {r["n"] for r in g.PATHS["CONVERT"] if r["kind"] == "convert"} and
        any(r["n"] > 4096 * 256 * 4 and r["n"] % 4 for r in g.PATHS["CONVERT"] if r["kind"] == "convert") and
        {(R, C) for R in (1, 31, 32, 33) for C in (1, 31, 32, 33)} <= {(r["R"], r["C"]) for r in g.PATHS["CONVERT"] if r["kind"] == "transpose"}),
}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_tables_hold_the_edge(edge):
    assert EDGES[edge](), edge


def test_carry_cap_restated():
    assert [g.carry_cap16({"LIDBOX_GEMM_CARRY_BLOCKS": v}) for v in ("7", "8", "200", "x")] == [96, 8, 200, 96] and g.carry_cap16({}) == 96


# ------------------------------------------------------------------------------------------ 3. references and rounding
def test_bf16_rounding_matches_torch():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-40, 39, 4000).astype(np.float32),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38, 1e-40, -1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, 258.0, 259.0],
                                 np.float32)])
    want = torch.from_numpy(x).bfloat16()
    got = g.bf16_rne(x)
    assert np.array_equal(np.isnan(got), torch.isnan(want).numpy())
    ok = ~np.isnan(got)
    assert np.array_equal(got[ok].view(np.int32), want.float().numpy()[ok].view(np.int32))
    assert g.bf16_rne(np.float32(257.0)) == 256.0 and g.bf16_rne(np.float32(259.0)) == 260.0 and np.isinf(g.bf16_rne(np.float32(3.4028235e38)))
    # the direct float64 rounding agrees on fp32 inputs and is monotonic
    fin = np.isfinite(x)
    assert np.array_equal(g.bf16_rne64(x[fin].astype(np.float64)), got[fin].astype(np.float64))
    y = np.sort(rng.standard_normal(5000))
    assert (np.diff(g.bf16_rne64(y)) >= 0).all()
    assert np.array_equal(g.bf16_trunc(np.array([1.0 + 2.0 ** -8 + 2.0 ** -9], np.float32)), np.array([1.0], np.float32))


def test_references_match_float64_torch():
    r = next(r for r in ROWS16 if r["name"].startswith("c-nt-130x132x136"))
    dat = g.make_rows_data(r, "normal")
    ref, S = g.rows_reference(dat=dat, r=r)
    ta, tb = torch.from_numpy(dat["A"]).bfloat16().double(), torch.from_numpy(dat["B"]).bfloat16().double()
    want = gp.apply_epi((ta @ tb.T).numpy(), r["epi"], dat["bias"], dat["mask"], dat["old"])
    np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
    t = next(r for r in TN16 if r["bias_grad"] and not r["accumulate"])
    dat = g.make_tn_data(t, "normal")
    v, S, gb, Sg = g.tn_reference(t, dat)
    ta, tb = torch.from_numpy(dat["A"]).bfloat16().double(), torch.from_numpy(dat["B"]).bfloat16().double()
    np.testing.assert_allclose(v, (ta.T @ tb).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(gb, torch.from_numpy(dat["B"]).double().sum(0).numpy(), rtol=0, atol=1e-12)      # the UNROUNDED operand
    s = next(r for r in TN16S if r["bias_grad"])
    dat = g.make_tn_data(s, "normal")
    assert np.array_equal(g.bf16_rne(dat["B"]), dat["B"])                                                          # storage operands are bf16 values
    np.testing.assert_allclose(g.tn_reference(s, dat)[2] - (dat["old_bg"].astype(np.float64) if s["accumulate"] else 0), dat["B"].astype(np.float64).sum(0), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------ 4. emulation, bounds, mutations
def test_bounds_are_below_half_a_bf16_ulp_of_typical_outputs():
    """a truncated shadow is off by up to one bf16 ulp; the fp32 bound must be far below half an ulp (2^-9 |ref| at the least) of outputs
    that are not cancellation-dominated -- every non-zero output of `offset`, whose products all have one sign -- or shadow_trunc
    could hide inside the shadow-only interval [bf16_rne(ref - b), bf16_rne(ref + b)]"""
    seen = 0
    for r in ROWS16S:
        if r["out"] != "shadow":
            continue
        dat = g.make_rows_data(r, "offset")
        ref, S = g.rows_reference(r, dat)
        b = conv2d_np.error_bound(S, gp.chain_n(r["K"], g.row_query(r)[4], r["epi"]))
        live = ref != 0
        assert live.any(), r["name"]
        worst = float((b[live] / (np.abs(ref[live]) * 2.0 ** -9)).max())
        assert worst < 0.25, (r["name"], worst)
        seen += 1
    assert seen >= 14                                            # a shadow-only row on every forced tile


def _caught_rows(r, q, data, mut):
    plan = g.row_plan(q)
    for ds in g.datasets_that_show(mut):
        c, s = g.emulate_rows(r, data[ds], plan, mut)
        if not g.judge_rows(r, ds, data[ds], c, s, q[4])[0]:
            return True
    return False


def test_emulation_inside_and_every_mutation_outside():
    uncaught, applied, worst, pairs = [], {}, 0.0, 0
    for r in ROWS:
        q = g.row_query(r)
        if q[0] <= 0:
            continue
        plan = g.row_plan(q)
        data = {ds: g.make_rows_data(r, ds) for ds in g.DATASETS}
        for ds in g.DATASETS:
            c, s = g.emulate_rows(r, data[ds], plan)
            ok, w, what = g.judge_rows(r, ds, data[ds], c, s, q[4])
            assert ok, (r["name"], ds, w, what)
            worst = max(worst, w)
        for mut in g.MUTATIONS:
            if not g.applies(mut, r, plan):
                continue
            pairs += 1
            applied.setdefault(mut, 0)
            applied[mut] += 1
            if not _caught_rows(r, q, data, mut):
                uncaught.append((r["name"], mut))
    for r in TN:
        q = g.tn_row_query(r)
        plan = g.tn_row_plan(r, q)
        data = {ds: g.make_tn_data(r, ds) for ds in g.DATASETS}
        for ds in g.DATASETS:
            c, bg = g.emulate_tn(r, data[ds], plan)
            ok, w, wg = g.judge_tn(r, ds, data[ds], c, bg, plan["pieces"], plan["per"])
            assert ok, (r["name"], ds, w, wg)
            worst = max(worst, w, wg)
        for mut in g.MUTATIONS:
            if not g.applies(mut, r, plan):
                continue
            pairs += 1
            applied.setdefault(mut, 0)
            applied[mut] += 1
            hit = False
            for ds in g.datasets_that_show(mut):
                c, bg = g.emulate_tn(r, data[ds], plan, mut)
                if not g.judge_tn(r, ds, data[ds], c, bg, plan["pieces"], plan["per"])[0]:
                    hit = True
                    break
            if not hit:
                uncaught.append((r["name"], mut))
    # CARRY16S: the wgrad whose pending slice sum is carried; PAIR16S: the second problem on 64 of its rows (the mutation is the epilogue's)
    twins = []
    for r in CARRY:
        if "w" in r["jobs"]:
            twins.append(("tn", g._tn_row("CARRY16S", r["name"], r["why"], "s", r["K1"], r["Co"], gp._dense(r["Mw"], r["K1"]), env=r["env"], accumulate=1, ldc_pad=4)))
    for r in PAIR:
        p1 = r["p1"]
        twins.append(("rows", dict(p1, M=64, a=gp._dense(64, p1["K"]), c=gp._dense(64, p1["N"]))))
    for kind, r in twins:
        if kind == "tn":
            q = g.tn_row_query(r)
            plan = g.tn_row_plan(r, q)
            run = lambda ds, mut=None: g.judge_tn(r, ds, data[ds], *g.emulate_tn(r, data[ds], plan, mut), plan["pieces"], plan["per"])[0]
            data = {ds: g.make_tn_data(r, ds) for ds in g.DATASETS}
        else:
            q = g.row_query(r)
            plan = g.row_plan(q)
            run = lambda ds, mut=None: g.judge_rows(r, ds, data[ds], *g.emulate_rows(r, data[ds], plan, mut), q[4])[0]
            data = {ds: g.make_rows_data(r, ds) for ds in g.DATASETS}
        assert all(run(ds) for ds in g.DATASETS), r["name"]
        for mut in ("carry_twice", "pair_epi_swapped"):
            if g.applies(mut, r, plan):
                pairs += 1
                applied[mut] = applied.get(mut, 0) + 1
                if not any(not run(ds, mut) for ds in g.datasets_that_show(mut)):
                    uncaught.append((r["name"], mut))
    print("emulation worst err / bound %.3f; %d (row, mutation) pairs, uncaught %d; rows per mutation %s" % (worst, pairs, len(uncaught), applied))
    assert not uncaught, uncaught[:20]
    assert set(applied) == set(g.MUTATIONS), set(g.MUTATIONS) ^ set(applied)            # every mutation was planted somewhere


# ------------------------------------------------------------------------------------------ 5. the 32-bit extent terms (FAR16)
FAR16 = g.PATHS["FAR16"]


def _far16_both(lib, r):
    if r["kind"] == "tn":
        wsb = g.tn_row_ws_bytes(r)
        return _tn_row_export(lib, r, wsb), g.tn_row_query(r, wsb)
    wsb = g.row_ws_bytes(r)
    return _row_export(lib, r, wsb), g.row_query(r, wsb)


def test_far16_limits_are_the_ones_the_source_states():
    L = g.limits16()
    assert L == dict(a_span=4.0e9, a_utt=2.0e9, a_ext=4.0e9, b_ext=4.0e9, pair_a_ext=4.0e9, pair_b_ext=4.0e9, span=4.0e9)


def test_every_far16_row_matches_the_export_and_selects_what_it_names(lib, monkeypatch):
    """the planner only tests pointers for alignment and NULL: both sides of every extent term are pinned through
    lidbox_gemm_bf16_plan_query with fake pointers, no memory behind them"""
    fast = set()
    for r in FAR16:
        _setenv(monkeypatch, r["env"])
        got, want = _far16_both(lib, r)
        assert got == want, (r["name"], got, want)
        e = r["expect"]
        assert (e["kernel"] is None or got[0] == e["kernel"]) and (e["not_kernel"] is None or got[0] != e["not_kernel"]), (r["name"], got)
        if r["term"] == "gap":                                       # the K1-resident wgrad's covered-gap term at its own edge
            cond = g.tn_kres_conditions(r["a"], r["b"], r["K1"], r["N"], g.plan_tn16_kres(r["M"], r["K1"], r["N"], r["env"]))
            assert [k for k, v in cond.items() if not v] == ([] if r["zone"] == "edge-in" else ["gap_covered"]), (r["name"], cond)
            continue
        op, which = next(iter(r["far"].items()))
        d = r["a"] if op == "A" else r.get("b")
        if r["term"] in ("a_ext", "a_span"):
            gq = g.a_ext16(r["a"], r["K"])
        elif r["term"] == "a_utt":
            gq = g.a_utt16(r["a"], r["K"])
        elif r["term"] == "b_ext":
            gq = g.b_ext16(r["N"], g.ldb_of(r), r["K"])
        else:
            gq = g.span16(d, r["K1"] if op == "A" else r["N"])
        L = g.limits16()[r["term"]]
        inside = r["zone"] in ("high", "edge-in")
        assert (gq < L) == inside, (r["name"], gq)
        if r["zone"] == "over":
            assert gq >= gp.OVER * L
        if r["zone"] == "high":
            assert gq >= 0.975 * L, "a bf16 operand needs about 2e9 elements of extent"
        if inside and r.get("twin_same", True):
            fast.add(got[0])
    assert fast >= {g.KS_DMA, g.KS_PP, g.KS_KRES0, g.KS_TN_PP, g.KS_TN_KRES}, fast


def test_far16_sweep_term_by_term(lib, monkeypatch):
    """each of batch_stride, rows_per_batch * row_stride and ldb stretched alone across each limit, in steps around it: the export
    equals the restated plan at every step, and the kernel changes exactly where the term crosses its limit"""
    n = 0
    L = g.limits16()
    for r in FAR16:
        if r["zone"] != "edge-in" or not r["far"] or not r.get("twin_same", True):
            continue
        _setenv(monkeypatch, r["env"])
        op, which = next(iter(r["far"].items()))
        kernels = []
        for k in (-(1 << 20), -64, -8, 0, 8, 64, 1 << 20, 1 << 27):
            rr = dict(r)
            if which == "ldb":
                rr["ldb_pad"] = r["ldb_pad"] + k
            elif which == "rpb":
                kk = k // 8
                rr["a"] = dict(r["a"], rpb=r["a"]["rpb"] + kk)
                rr["M"] = rr["a"]["rpb"]
                rr["c"] = gp._dense(rr["M"], r["N"])
            else:
                key = "a" if op == "A" else "b"
                step = r[key]["rs"] if r["expect"]["kernel"] == g.KS_TN_KRES and op == "A" else 1
                rr[key] = dict(r[key], bs=r[key]["bs"] + k * step)
            got, want = _far16_both(lib, rr)
            assert got == want, (r["name"], k, got, want)
            kernels.append(got[0])
            n += 1
        assert all(k == r["expect"]["kernel"] for k in kernels[:4]) and all(k != r["expect"]["kernel"] for k in kernels[4:]), (r["name"], kernels)
    # rows_per_batch * row_stride alone, through row_stride with batch = 1 (a_ext) and through rows_per_batch (a_span, a_utt above)
    _setenv(monkeypatch, {})
    for K, N, M in ((64, 64, 130),):
        for zone in ("edge-in", "edge-out"):
            rs = gp._solve(lambda s: g.a_ext16(dict(batch=1, rpb=M, rs=s, bs=0), K), L["a_ext"], zone, step=8, lo=K)
            a, c = dict(batch=1, rpb=M, rs=rs, bs=0), gp._dense(M, N)
            got = _export(lib, g.Q16S_NT, a, None, c, K, N, 0, 1 << 30, ldb=K)
            assert got == g.plan_query(g.Q16S_NT, a, None, c, K, N, 0, {}, 1 << 30, ldb=K) and (got[0] == g.KS_DMA) == (zone == "edge-in"), (zone, got)
            n += 1
    print("%d planner queries around the limits" % n)
    assert n >= 60


def test_far16_pair_site_restated():
    """pp2_problem's own a_ext / b_ext (no export reports it: the restated conditions, each limit failing alone)"""
    for name, call, ok in g.far16_pair_calls():
        cond = g.pp2_conditions(call, 2 * call["a"]["rpb"] * call["N"] * 4, {})
        assert all(cond.values()) == ok and (ok or [k for k, v in cond.items() if not v] == ["ext"]), (name, cond)
