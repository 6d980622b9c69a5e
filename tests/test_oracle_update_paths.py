"""
Pins oracle/update_paths_np.py on the CPU (no device, no launches):
  1. the restated constants and rules against the source text of csrc/nnops.hip and csrc/mla.hip;
  2. every PATHS row selects the path, trip count and instantiation it claims, and the rows together reach all 16 (VEC, NJ)
     launch sites of the attention pool, both kernels of bn_relu_dropout in both directions (each pointer alone knocking it
     off the vector path), both lds_pf values of cavg_result, every optimiser variant and every second trip;
  3. the counter hash against a plain-integer walk; the float32 emulations inside the stated bounds (optimiser steps, fused
     and unfused where a product feeds a sum; the Box-Muller draw on 4 M uniforms under HALF its bound; attention forward
     and backward; cavg_result), and the analytic attention backward against float64 autograd;
  4. each plantable mistake outside the bound on at least one of the rows oracle.update_paths_np.MISTAKES names for it.
"""
import os
import re

import numpy as np
import pytest

from oracle import update_paths_np as up
from oracle.conv2d_np import fma32


def _src(name):
    with open(os.path.join(up.CSRC, name)) as f:
        return f.read()


NNOPS, MLA = _src("nnops.hip"), _src("mla.hip")


def _body(fn):
    body = NNOPS[NNOPS.index('extern "C" int %s(' % fn):]
    return body[:body.index("\n}\n")]


# ---------------------------------------------------------------------------------------------------- 1. source text
def test_restated_constants_match_the_sources():
    assert "long g = lbx_cdiv(n, 256);" in NNOPS and "(g < 1 ? 1 : (g > %d ? %d : g))" % (up.EW_MAX_BLOCKS, up.EW_MAX_BLOCKS) in NNOPS
    assert NNOPS.count("dim3(ew_grid(n / 4 + 1)), dim3(256)") == 2 and "const long n4 = n >> 2;" in NNOPS
    assert "(n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride" in NNOPS
    for k in ("sgd_kernel", "rmsprop_kernel", "scale_kernel", "fill_kernel"):
        assert "%s, dim3(ew_grid(n)), dim3(256)" % k in NNOPS, k
    assert "hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256)" in NNOPS and "i < n; i += 256) s += x[i];" in NNOPS
    assert NNOPS.count("if (gx > %d) gx = %d;" % (up.DROP_MAX_GX, up.DROP_MAX_GX)) == 2
    assert NNOPS.count("long gx = lbx_cdiv((long)T * C, 256);") == 2
    for fn in ("lidbox_spatial_dropout", "lidbox_input_noise_dropout"):
        assert "LBX_ARG(B <= %d," % up.DROP_MAX_B in _body(fn), fn
    assert "if (B == 0 || T == 0 || rate == 0.f) return LIDBOX_OK;" in NNOPS
    assert "if (B == 0 || T == 0 || (rate == 0.f && stddev == 0.f)) return LIDBOX_OK;" in NNOPS
    assert "(long)T * C < (1L << 32)" in NNOPS and "if (mask_out && i < C) mask_out[(long)b * C + c] = m;" in NNOPS
    assert "if (R == 0 || rate == 0.f) return LIDBOX_OK;" in NNOPS
    assert "if (g > %d) g = %d;" % (up.ROWS_MAX_BLOCKS, up.ROWS_MAX_BLOCKS) in NNOPS
    assert "if (g > %d) g = %d;" % (up.BNRD_MAX_BLOCKS, up.BNRD_MAX_BLOCKS) in MLA
    assert ("const bool vec4 = C % 4 == 0 && aligned16(x) && aligned16(scale) && aligned16(shift) && aligned16(out) && "
            "(!BWD || aligned16(dy));") in MLA
    assert "const long n = R * C / (vec4 ? 4 : 1);" in MLA
    for src in (NNOPS, MLA):                                # the hash, stated twice
        assert "0x%Xull * (step + 1) + (((unsigned long long)b << 32) | c)" % up.GOLD in src
        assert "v ^= v >> 30; v *= 0x%Xull;" % up.MIX1 in src and "v ^= v >> 27; v *= 0x%Xull;" % up.MIX2 in src
        assert "v ^= v >> 31;" in src and "(float)(v >> 40) * (1.0f / 16777216.0f)" in src
        assert "const float keep_scale = 1.f / (1.f - rate);" in src
    assert "hash_uniform(seed + 0x%Xull, stp, (unsigned)b, (unsigned)i)" % up.NOISE_SEED1 in NNOPS
    assert "hash_uniform(seed + 0x%Xull, stp, (unsigned)b, (unsigned)i)" % up.NOISE_SEED2 in NNOPS
    assert "v += stddev * (sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2));" in NNOPS
    assert "hash_uniform(seed, stp, (unsigned)b, (unsigned)c) >= rate ? keep_scale : 0.f" in NNOPS
    assert "hash_uniform(seed, stp, (unsigned)r, (unsigned)c) >= rate ? keep_scale : 0.f" in NNOPS
    assert "mla_hash_uniform(seed, stp, (unsigned)r, (unsigned)(c0 + e)) >= rate ? keep_scale : 0.f" in MLA
    assert "constexpr int MLA_MAX_K = %d;" % up.MLA_MAX_K in MLA and "p.nw = K <= 512 ? 16 : 8;" in MLA
    assert "while (p.G < 64 && p.G < kv) p.G <<= 1;" in MLA and "while (p.nj < need) p.nj <<= 1;" in MLA
    assert "dim3(p.nw * 64), (size_t)p.nw * 2 * K * sizeof(float)" in MLA
    assert "const int nw = %d;" % up.MLA_BWD_NW in MLA and "const long want = lbx_cdiv(%d, B);" % up.MLA_BWD_WANT in MLA
    assert "const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z));" in MLA
    assert "const MlaPlan p = mla_plan(K, K % 4 == 0 && aligned16(z) && aligned16(dz));" in MLA
    assert "constexpr float MLA_CLIP_LO = 1e-7f;" in MLA and float(np.float32(0.99999988079071044921875)) == up.HI
    assert "const int lds_pf = Th <= %d && lds <= 48 * 1024;" % up.CAVG_LDS_TH in NNOPS
    assert "for (int th = threadIdx.x; th < Th; th += %d)" % up.CAVG_THREADS in NNOPS
    assert "return div_no_nan(inner, (float)(N - 1));" in NNOPS
    assert "const float base = __float_as_uint(st->lr_now) != 0u ? fabsf(st->lr_now) : lr;" in NNOPS
    assert "st->lr_t = __float_as_uint(st->lr_now) != 0u ? fabsf(st->lr_now) : lr;" in NNOPS
    # every refusal is made by the host-side argument check, before the first launch of its function
    for fn in ("lidbox_spatial_dropout", "lidbox_input_noise_dropout", "lidbox_dropout_rows", "lidbox_adam_step", "lidbox_sgd_step",
               "lidbox_rmsprop_step", "lidbox_cavg_result", "lidbox_mean"):
        body = _body(fn)
        assert body.rindex("LBX_ARG(") < body.index("hipLaunchKernelGGL"), fn


# ---------------------------------------------------------------------------------------------------- 2. what rows select
def test_ew_grid_and_the_adam_split():
    assert [up.ew_grid(n) for n in (0, 1, 256, 257, 524288, 524289)] == [1, 1, 1, 2, 2048, 2048]
    assert [up.ew_trips(n) for n in (1, 524288, 524289)] == [1, 1, 2]
    want = {0: (0, 0, 0, False), 1: (0, 1, 0, True), 3: (0, 3, 0, True), 4: (1, 0, 1, True), 5: (1, 1, 1, True), 7: (1, 3, 1, True),
            1023: (255, 3, 1, True), 1024: (256, 0, 1, True), 1027: (256, 3, 1, True), up._ADAM_BIG: (524544, 3, 2, True)}
    lens = sorted({r["n"] for r in up.ADAM})
    assert lens == sorted(want)
    for n in lens:
        p = up.adam_plan(n)
        assert (p["n4"], p["tail"], p["body_trips"], p["launch"]) == want[n], n
    assert {n & 3 for n in lens} == {0, 1, 2, 3} or {n & 3 for n in lens} >= {0, 1, 3}
    assert up.adam_plan(2097152)["body_trips"] == 1 and up.adam_plan(2097152 + 4)["body_trips"] == 2
    rows = {r["name"]: r for r in up.ADAM}
    assert {rows[k]["step"] for k in ("step0", "step1", "step10000", "step%d" % (1 << 33))} == {0, 1, 10000, 1 << 33}
    assert np.float32(rows["neg_zero"]["lr_now"]).view(np.uint32) == 0x80000000 and rows["gs05"]["gs"] == 0.5 and rows["zeroed"]["zero"]
    assert rows["lr_now"]["lr_now"] == 5e-4


def test_the_optimiser_rows_reach_every_variant_and_the_second_trip():
    for table, variants in ((up.SGD, up.SGD_VARIANTS), (up.RMSPROP, up.RMS_VARIANTS)):
        assert {(r["variant"], r["n"]) for r in table} == {(k, n) for k in variants for n in up.OPT_NS}
        assert {up.ew_trips(r["n"]) for r in table} == {0, 1, 2}
        assert {r["gs"] for r in table} == {1.0, 0.5}
        assert {int(np.float32(r["lr_now"]).view(np.uint32)) for r in table} == {0, 0x80000000, int(np.float32(5e-4).view(np.uint32))}
    assert up.ew_trips(524288) == 1 and up.ew_trips(524288 + 300) == 2
    assert {(v["mu"] > 0, v["nesterov"]) for v in up.SGD_VARIANTS.values()} == {(False, 0), (True, 0), (True, 1)}
    assert {(v["mu"] > 0, v["centered"]) for v in up.RMS_VARIANTS.values()} == {(a, b) for a in (False, True) for b in (0, 1)}
    assert [up.ew_trips(r["n"]) for r in up.EW] == [1, 1, 1, 1, 2]


def test_the_dropout_rows_select_what_they_say():
    got = {r["name"]: up.spatial_plan(r["B"], r["T"], r["C"], 0.25) for r in up.SPATIAL}
    assert (got["b1t1c1"]["gx"], got["b1t1c1"]["trips"]) == (1, 1)
    assert got["b2t1c257"]["mask_blocks"] == 2 and got["b2t3c300"]["mask_blocks"] == 2 and got["b2t3c300"]["gx"] == 4
    assert (got["b2t65c253"]["gx"], got["b2t65c253"]["trips"]) == (64, 2) and (64 * 256) % 253 != 0
    assert (got["b2t2c16400"]["gx"], got["b2t2c16400"]["trips"], got["b2t2c16400"]["mask_trips"]) == (64, 3, 2)
    assert got["b65535t1c1"]["launch"] and not got["b2t0c5"]["launch"] and not got["b0t3c5"]["launch"]
    assert not up.spatial_plan(3, 7, 5, 0.0)["launch"] and up.spatial_plan(3, 7, 5, 0.0, 0.01)["launch"]
    assert up.spatial_accepts(65535, 1, 1, 1) and not up.spatial_accepts(65536, 1, 1, 1)
    assert up.spatial_accepts(1, 65536, 65536, 1 << 32) and not up.spatial_accepts(1, 65536, 65536, 1 << 32, noise=True)
    assert not up.spatial_accepts(2, 3, 5, 14) and {r["gap"] for r in up.SPATIAL} == {0, 3}
    rows = {r["name"]: up.rows_plan(r["batch"] * r["rpb"], r["C"], 0.4) for r in up.ROWS}
    assert rows["trip2"]["grid"] == 4096 and rows["trip2"]["trips"] == 2 and rows["trip2_b3"]["trips"] == 2
    assert all(rows[k]["trips"] == 1 for k in rows if not k.startswith("trip2"))
    assert {(r["batch"], r["C"]) for r in up.ROWS} >= {(b, C) for b in (1, 3) for C in (1, 7, 64)}
    assert up.by_name("rows", "trip2")["rpb"] * 4 == 1048576 + 700


def _bnrd_addrs(off):
    a = dict(x=0x1000, scale=0x2000, shift=0x3000, out=0x4000, dy=0x5000)
    if off:
        a[off] += 4
    return a


def test_the_fused_pass_rows_select_both_kernels_in_both_directions():
    seen = set()
    for r in up.BNRD:
        for bwd in (False, True):
            if r["off"] == "dy" and not bwd:
                assert up.bnrd_plan(r["R"], r["C"], _bnrd_addrs("dy"), False)["vec"] == 4      # forward does not look at dy
                continue
            p = up.bnrd_plan(r["R"], r["C"], _bnrd_addrs(r["off"]), bwd)
            seen.add(p["kernel"])
            want_vec = 4 if (r["C"] % 4 == 0 and r["off"] is None) else 1
            assert p["vec"] == want_vec, r["name"]
            assert p["trips"] == (2 if r["name"].startswith("cap_") else 1), r["name"]
    assert seen == {k for k in up.launch_site_kernels() if k.startswith("bn_relu")}
    assert {r["off"] for r in up.BNRD} == {None, "x", "scale", "shift", "out", "dy"}
    cap = {r["name"]: r for r in up.BNRD}
    assert 0 < cap["cap_vec"]["R"] * 4 - 4 * 8192 * 256 <= 16 and 0 < cap["cap_scalar"]["R"] * 6 - 8192 * 256 <= 24


def _mla_sel(r):
    zoff, dzoff = 4 * ("z" in r["off"]), 4 * ("dz" in r["off"])
    f = up.mla_fwd_plan(r["T"], r["K"], up.mla_vec4(r["K"], zoff))
    b = up.mla_bwd_plan(r["B"], r["T"], r["K"], up.mla_vec4(r["K"], zoff, dzoff))
    return f, b


def test_the_attention_rows_reach_every_launch_site():
    fwd, bwd, Gs = set(), set(), {1: set(), 4: set()}
    rows = {r["name"]: r for r in up.MLA}
    for r in up.MLA:
        f, b = _mla_sel(r)
        fwd.add(f["kernel"])
        bwd.add(b["kernel"])
        Gs[f["vec"]].add(f["G"])
        assert f["lds"] <= 64 * 1024 and r["B"] * r["T"] * r["K"] < 5000000 and r["K"] <= up.MLA_MAX_K
        assert f["nw"] * 64 <= (512 if f["vec"] * f["nj"] >= 16 else 1024)          # the block fits __launch_bounds__
    sites = up.launch_site_kernels()
    assert fwd == {k for k in sites if "fwd" in k} and bwd == {k for k in sites if "bwd" in k} and len(fwd) == len(bwd) == 8
    assert Gs[1] == Gs[4] == {1, 2, 4, 8, 16, 32, 64}
    want = {4: (4, 1), 100: (4, 1), 256: (4, 1), 260: (4, 2), 512: (4, 2), 516: (4, 4), 1024: (4, 4), 1: (1, 1), 3: (1, 1), 63: (1, 1),
            127: (1, 2), 255: (1, 4), 511: (1, 8), 1023: (1, 16)}
    for K, vn in want.items():
        f, _ = _mla_sel(rows["k%d" % K])
        assert (f["vec"], f["nj"]) == vn, K
    for K, nj in ((128, 2), (512, 8), (1024, 16)):
        f, b = _mla_sel(rows["k%d_zoff" % K])
        assert (f["vec"], f["nj"], b["vec"], b["nj"]) == (1, nj, 1, nj)
    f, b = _mla_sel(rows["k128_dzoff"])
    assert (f["vec"], b["vec"], b["nj"]) == (4, 1, 2)
    assert [_mla_sel(rows[k])[0]["lds"] for k in ("k512", "k1024", "k512_zoff", "k1024_zoff")] == [65536] * 4
    assert _mla_sel(rows["k512"])[0]["nw"] == 16 and _mla_sel(rows["k1024"])[0]["nw"] == 8
    for K in (100, 3):
        ps = up._pass(K, K % 4 == 0)
        assert [rows["k%d_t%s" % (K, t)]["T"] for t in ("m1", "eq", "p1")] == [ps - 1, ps, ps + 1]
        assert [_mla_sel(rows["k%d_t%s" % (K, t)])[0]["passes"] for t in ("m1", "eq", "p1")] == [1, 1, 2]
    f, _ = _mla_sel(rows["k4_t1025"])
    assert (f["G"], f["pass_rows"], f["passes"]) == (1, 1024, 2)
    f, b = _mla_sel(rows["k64_trip2"])
    assert (b["rows_per_wg"], b["gy"], b["trips"]) == (32, 2, 2) and 70 - 64 == 6         # 6 rows take the second trip
    assert all(_mla_sel(r)[1]["trips"] == 1 for r in up.MLA if r["name"] != "k64_trip2")
    assert rows["k12_ld"]["ld"] > rows["k12_ld"]["K"] and _mla_sel(rows["k100_t1"])[0]["passes"] == 1


def test_the_cavg_rows_sit_on_both_sides_of_every_switch():
    got = {(r["N"], r["Th"]): (up.cavg_lds_pf(r["N"], r["Th"]), up.cavg_trips(r["Th"])) for r in up.CAVG}
    assert got == {(2, 1): (True, 1), (3, 5): (True, 1), (24, 512): (True, 1), (25, 512): (False, 1), (14, 513): (False, 1),
                   (3, 1024): (False, 1), (3, 1025): (False, 2), (2, 2049): (False, 3)}
    assert 24 * 512 * 4 == 48 * 1024 and 14 * 513 * 4 < 48 * 1024                        # (14, 513) is off by the Th rule alone
    tp, fn, fp, tn = up.cavg_counters(3, 5, 1)
    assert not tp[0].any() and not fn[0].any() and not fp[1, 0].any() and not tn[1, 0].any()


# ---------------------------------------------------------------------------------------------------- 3. hash, emulations
def _hash_int(seed, step, b, c):
    M = (1 << 64) - 1
    v = (seed + up.GOLD * (step + 1) + ((b << 32) | c)) & M
    v ^= v >> 30
    v = (v * up.MIX1) & M
    v ^= v >> 27
    v = (v * up.MIX2) & M
    v ^= v >> 31
    return (v >> 40) / 16777216.0


def test_the_hash_in_uint64_equals_a_plain_integer_walk():
    for seed in (0, 5, up.DROP_SEED, (1 << 64) - 1):
        for step in (0, 1, (1 << 32) + 1, (1 << 64) - 1):
            got = up.hash_uniform(seed, step, np.arange(3)[:, None], np.array([0, 1, 300, (1 << 32) - 1])[None, :])
            for b in range(3):
                for j, c in enumerate((0, 1, 300, (1 << 32) - 1)):
                    assert float(got[b, j]) == _hash_int(seed, step, b, c)
    u = up.hash_uniform(7, 3, np.arange(1000)[:, None], np.arange(1000)[None, :])
    assert u.dtype == np.float32 and 0.0 <= u.min() and u.max() < 1.0 and abs(float(u.mean()) - 0.5) < 2e-3
    assert up.keep_scale(0.25) == np.float32(4) / np.float32(3) and up.keep_scale(0.0) == 1.0
    m = up.spatial_mask(3, 7, 5, 0.4, 9, 2)
    assert (m == m[:, :1, :]).all() and set(np.unique(m)) <= {np.float32(0), up.keep_scale(0.4)}
    assert np.array_equal(m[:, 0, :], up.rows_mask(3, 5, 0.4, 9, 2))                  # (b, c) and (r, c) are one hash


def test_the_box_muller_draw_in_float32_stays_under_half_its_bound():
    rng = np.random.default_rng(1)
    h1, h2 = (rng.integers(0, 1 << 24, 1 << 22).astype(np.float32) * np.float32(2.0 ** -24) for _ in range(2))
    h1[:4] = [0.0, (2.0 ** 24 - 1) / 2.0 ** 24, 0.5, 0.25]
    u1 = np.float32(1) - h1
    R = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ref = R * np.cos(up.TWO_PI32 * h2.astype(np.float64))
    q = np.abs(up.box_muller32(u1, h2).astype(np.float64) - ref) / up.box_muller_bound(R, 1.0)
    assert q.max() <= 0.5, q.max()
    assert R.max() > 5.7 and R.min() == 0.0


OPT_CASES = [(k, r) for k in ("adam", "sgd", "rmsprop") for r in up.PATHS[k] if 0 < r["n"] <= 4096]


def _opt_data(kind, r):
    return up.opt_state(r["n"], 11, zero=r.get("zero", False))


@pytest.mark.parametrize("kind,r", OPT_CASES, ids=["%s-%s" % (k, r["name"]) for k, r in OPT_CASES])
def test_a_float32_optimiser_step_stays_inside_its_bounds(kind, r):
    d = _opt_data(kind, r)
    _, lr_t = up.opt_row_lr_t(kind, r)
    refs = up.opt_row_refs(kind, r, d, lr_t)
    emu = up.opt_row_emu32(kind, r, d, lr_t)
    assert set(refs) == set(emu)
    for name, (ref, bound) in refs.items():
        assert np.isfinite(ref).all() and (bound >= 0).all()
        assert (np.abs(emu[name].astype(np.float64) - ref) <= bound).all(), (name, np.abs(emu[name] - ref).max())
        assert (bound <= 2e-5 * np.maximum(1.0, np.abs(ref))).all(), name              # the bounds are roundings, not slack
    if np.float32(r["lr_now"]).view(np.uint32) == 0x80000000:
        assert lr_t == 0
    if lr_t == 0 and "velocity" not in refs and "mom" not in refs:        # with momentum the carried step still moves param
        assert np.array_equal(emu["param"].view(np.int32), d["param"].view(np.int32))
        assert np.array_equal(refs["param"][0], d["param"].astype(np.float64))


def test_fused_multiply_adds_stay_inside_the_same_bounds():
    d = up.opt_state(1027, 11)
    h = up.HP["adam"]
    b1, b2, one = np.float32(h["b1"]), np.float32(h["b2"]), np.float32(1)
    refs = up.adam_ref(d["param"], d["grad"], d["m"], d["v"], 1e-3, h["b1"], h["b2"], h["eps"], 0.5)
    gr = d["grad"] * np.float32(0.5)
    m1 = fma32(b1, d["m"], (one - b1) * gr).astype(np.float32)
    v1 = fma32(b2, d["v"], (one - b2) * gr * gr).astype(np.float32)
    for name, got in (("m", m1), ("v", v1)):
        assert (np.abs(got.astype(np.float64) - refs[name][0]) <= refs[name][1]).all(), name
    s = up.sgd_ref(d["param"], d["grad"], d["velocity"], 0.03, 0.9, 1, 0.5)
    lr, mu = np.float32(0.03), np.float32(0.9)
    v1 = fma32(mu, d["velocity"], -(lr * gr)).astype(np.float32)
    p1 = (d["param"] + fma32(mu, v1, -(lr * gr)).astype(np.float32)).astype(np.float32)
    assert (np.abs(v1 - s["velocity"][0]) <= s["velocity"][1]).all() and (np.abs(p1 - s["param"][0]) <= s["param"][1]).all()


def test_lr_t_follows_the_state():
    h = up.HP["adam"]
    t, v = up.lr_t_ref(h["lr"], 0.0, 0, h["b1"], h["b2"])
    assert t == 1 and abs(float(v) / (1e-3 * np.sqrt(1 - float(np.float32(0.999))) / (1 - float(np.float32(0.9)))) - 1) < 1e-6
    assert up.lr_t_ref(h["lr"], 0.0, 1 << 33, h["b1"], h["b2"]) == ((1 << 33) + 1, np.float32(1e-3))      # saturated
    assert up.lr_t_ref(h["lr"], -0.0, 5, h["b1"], h["b2"])[1] == 0 and up.lr_t_ref(0.03, -0.0, 5)[1] == 0
    assert up.lr_t_ref(0.03, 5e-4, 5) == (6, np.float32(5e-4)) and up.lr_t_ref(0.03, 0.0, 5) == (6, np.float32(0.03))
    assert up.lr_t_ref(h["lr"], -5e-4, 9999, h["b1"], h["b2"])[1] > 0                                    # |lr_now|


MLA_CPU = [r for r in up.MLA if r["B"] * r["T"] * r["K"] <= 200000]


@pytest.mark.parametrize("r", MLA_CPU, ids=lambda r: r["name"])
def test_float32_attention_stays_inside_the_derived_bounds(r):
    z, gd = up.mla_inputs(r["B"], r["T"], r["K"], 7)
    f, b = _mla_sel(r)
    ref = up.mla_fwd_ref(z, f)
    att, s, dz = up.mla_emu32(z, gd)
    assert (np.abs(att - ref["att"]) <= ref["att_rel"] * ref["att"]).all()
    assert (np.abs(s - ref["colsum"]) <= ref["colsum_rel"] * ref["colsum"]).all()
    assert ref["att_rel"].max() < 2e-5 and (r["T"] < 15 or ref["clipped"] > 0.1 or r["K"] <= 2)
    dref, dbound = up.mla_bwd_ref(z, att, s, gd, b)
    assert (np.abs(dz - dref) <= dbound).all(), (np.abs(dz - dref) / dbound).max()


def test_the_analytic_attention_backward_is_the_gradient():
    import torch
    z, gd = up.mla_inputs(3, 17, 5, 3)
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    c = torch.clamp(torch.softmax(zt, -1), up.LO, up.HI)
    att = ((c / c.sum(1, keepdim=True)) / (1 + torch.exp(-zt))).sum(1)
    (att * torch.from_numpy(gd.astype(np.float64))).sum().backward()
    plan = up.mla_bwd_plan(3, 17, 5, False)
    ref = up.mla_fwd_ref(z, up.mla_fwd_plan(17, 5, False))
    assert np.abs(ref["att"] - att.detach().numpy()).max() < 1e-14
    # the analytic form with exact (float64) att and colsum
    zz, p, _ = up._softmax_parts(z, plan)
    v, dv = up._sigmoid_parts(zz)
    cc = np.clip(p, up.LO, up.HI)
    gs = gd.astype(np.float64)[:, None, :] / ref["colsum"][:, None, :]
    dp = np.where((p >= up.LO) & (p <= up.HI), gs * (v - ref["att"][:, None, :]), 0.0)
    dz = p * (dp - (dp * p).sum(-1, keepdims=True)) + gs * cc * dv
    assert np.abs(dz - zt.grad.numpy()).max() < 1e-13
    # and mla_bwd_ref on float32 roundings of att and colsum agrees with it to those roundings
    d32, _ = up.mla_bwd_ref(z, ref["att"].astype(np.float32), ref["colsum"].astype(np.float32), gd, plan)
    assert np.abs(d32 - dz).max() < 1e-6


@pytest.mark.parametrize("r", up.CAVG, ids=lambda r: r["name"])
def test_float32_cavg_result_stays_inside_its_bound(r):
    cnt = up.cavg_counters(r["N"], r["Th"], 5)
    c, bound, cmin, bmin = up.cavg_ref(*cnt, **up.CAVG_COST)
    emu = up.cavg_emu32(*cnt, **up.CAVG_COST)
    assert (np.abs(emu - c) <= bound).all() and abs(float(emu.min()) - cmin) <= bmin and bound.max() < 1e-5


# ---------------------------------------------------------------------------------------------------- 4. planted mistakes
def _outside(value, ref, bound):
    return bool((np.abs(np.asarray(value, np.float64) - ref) > bound).any())


def _rejected(key, name):
    """whether the outputs of the reference WITH the mistake leave the bounds of the reference without it, on row `name`"""
    table, _ = up.MISTAKES[key]
    mistake = key.split(":")[1]
    r = up.by_name(table, name)
    if table in ("adam", "sgd", "rmsprop"):
        d = _opt_data(table, r)
        _, lr_t = up.opt_row_lr_t(table, r)
        good = up.opt_row_refs(table, r, d, lr_t)
        if mistake == "no_bias":
            _, bad_lr = up.opt_row_lr_t(table, r, mistake)
            assert abs(float(bad_lr) - float(lr_t)) > 2 * float(np.spacing(lr_t))         # outside the 1 ulp allowed on lr_t
            bad = up.opt_row_refs(table, r, d, bad_lr)
        else:
            bad = up.opt_row_refs(table, r, d, lr_t, mistake)
        return any(_outside(bad[k][0], *good[k]) for k in good)
    if table == "spatial":
        x = np.random.default_rng(2).standard_normal((r["B"], r["T"], r["C"])).astype(np.float32)
        good = up.spatial_ref(x, 0.25, up.DROP_SEED, 1)
        bad = up.spatial_ref(x, 0.25, up.DROP_SEED, 1, mistake)
        return not np.array_equal(good[0].view(np.int32), bad[0].view(np.int32))         # masks are judged bit for bit
    if table == "noise":
        x = np.random.default_rng(2).standard_normal((r["B"], r["T"], r["C"])).astype(np.float32)
        good = up.noise_ref(x, 0.01, 0.25, up.DROP_SEED, 1)
        return _outside(up.noise_ref(x, 0.01, 0.25, up.DROP_SEED, 1, mistake)[0], *good)
    if table == "mla":
        z, gd = up.mla_inputs(r["B"], r["T"], r["K"], 7)
        f, b = _mla_sel(r)
        good = up.mla_fwd_ref(z, f)
        if mistake == "pass_clipped":
            a32, s32 = good["att"].astype(np.float32), good["colsum"].astype(np.float32)
            return _outside(up.mla_bwd_ref(z, a32, s32, gd, b, mistake)[0], *up.mla_bwd_ref(z, a32, s32, gd, b))
        bad = up.mla_fwd_ref(z, f, mistake)
        return (_outside(bad["att"], good["att"], good["att_rel"] * good["att"])
                or _outside(bad["colsum"], good["colsum"], good["colsum_rel"] * good["colsum"]))
    cnt = up.cavg_counters(r["N"], r["Th"], 5)
    c, bound, cmin, bmin = up.cavg_ref(*cnt, **up.CAVG_COST)
    cb, _, cminb, _ = up.cavg_ref(*cnt, **up.CAVG_COST, mistake=mistake)
    return _outside(cb, c, bound) or abs(cminb - cmin) > bmin


@pytest.mark.parametrize("key", sorted(up.MISTAKES))
def test_every_planted_mistake_is_rejected_on_a_named_row(key):
    _, names = up.MISTAKES[key]
    hits = [n for n in names if _rejected(key, n)]
    print("%-24s rejected on %s of %s" % (key, hits, list(names)))
    assert hits, key
    assert key not in up.UNDETECTABLE and not up.UNDETECTABLE


def test_rows_not_named_for_a_mistake_can_miss_it():
    """why the rows are named: one trip cannot show a `c` kept from the first trip, and T <= one wave's share cannot show a
    missing wave"""
    assert not _rejected_on("spatial:c_first_trip", "b3t7c5") and not _rejected_on("att:drop_wave", "k100_t1")
    assert not _rejected_on("cavg:min_first_1024", "n3th1024")


def _rejected_on(key, name):
    return _rejected(key, name)


def test_every_row_says_why_it_exists():
    for table, rows in up.PATHS.items():
        names = [r["name"] for r in rows]
        assert len(set(names)) == len(names), table
        assert all(r["why"] for r in rows)
    for key, (table, names) in up.MISTAKES.items():
        assert all(any(r["name"] == n for r in up.PATHS[table]) for n in names), key
    assert re.search(r"rate == 0 .* returns before any launch", open(os.path.join(os.path.dirname(up.CSRC), "..", "include",
                                                                                  "lidbox_hip.h")).read())
