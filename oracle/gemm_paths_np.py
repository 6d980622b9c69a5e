"""
The fp32 GEMM family (csrc/gemm.hip on gemm_shared.h, gemm_dma.h, gemm_dma8.h, gemm_sk.h) on every dispatch path: the host
dispatch restated in Python, float64 references through the implicit-row descriptors, per-element bounds, three data sets, an
fp32 emulation of a tiled launch with plantable mutations, and the PATHS tables that tests/test_gemm_paths_gpu.py runs.
numpy only; tests/test_oracle_gemm_paths.py checks every restated function against the library's planner exports on the CPU.

1. Dispatch.  choose_rows / launch_cost / choose_rows_env (LIDBOX_GEMM_PLAN, _NN8, _NT8), sk_rows_plan (policy, grid and floor
   knobs), sk_tn_plan, dma_stream_plan, the tail split of launch_rows, tn_plan, pair_plan, the `al` predicate and
   reduce_job_vec_ok are restated line by line; the environment is an explicit dict.  The tuned table is READ from
   csrc/gemm_tuned.h (tuned_table), not copied.  rows_dispatch / tn_dispatch predict for a call: the family
   (lidbox_gemm_last_family), the kernel instantiations launched, the three lidbox_gemm_last_launches counters, the streamed
   remainder's g, and p, the number of partial sums the fixed-order reduce adds per element.

2. References (float64).  A . B, A . B^T, A^T B and column sums with rows addressed as base + b * batch_stride + t * row_stride
   (row_offsets; overlapping causal windows included), the eight epilogues exactly as apply_epi states them.

3. Bounds, per element: conv2d_np.error_bound(S, n), S the same product on absolute values (old C and bias by absolute value
   too).  n = 2 K + p + e for a K-term MFMA chain (2 K: the project's own count, rnn_paths_np.py), p partial sums (split-K
   splits, stream-K contributors of a tile, DmaStream pieces, wgrad slices), e = 1 (the store) + 1 when the epilogue adds
   bias or old C.  wgrad: K = contracted rows of one slice.  Column sums: colsum_stage1 adds ceil(rows_per_slice / 4) terms per
   lane group, 3 more across groups, colsum_stage2 adds `slices` partials and the old value: n = ceil(rps / 4) + 3 + slices + 1;
   the fused bias gradient is one chain over a slice's rows (zero-filled tail rows are exact) plus the slices plus the old
   value: n = rps + splits + 1.  Stream-K contributors in span mode: every workgroup takes floor(sk_tiles nk / P) K steps or
   one more, so a tile of nk steps has at most ceil(nk / span) + 1 contributors.

4. Data sets: `normal` N(0, 1); `offset` 1 + 0.1 N(0, 1); `exact` non-zero integers in [-7, 7] for A and B, integer bias and
   old C, mask values from {-2, -0.0, 0.0, 3}: every product and sum is exact in fp32 (|sum| <= 49 K < 2^24) and the device
   must equal the int64 result bit for bit, whatever the summation order.

5. emulate(): an fp32 emulation of one launch (16-deep K steps, splits / pieces summed in k order, the epilogue, the pitched
   store) with the MUTATIONS planted; the CPU test proves the unmutated emulation inside the bounds and every applicable
   (row, mutation) pair outside them.

6. PATHS: ROWS (lidbox_gemm_nn / _nt), TN (lidbox_gemm_tn), COLSUM (lidbox_colsum), PAIR (lidbox_gemm_nt_tn), CARRY
   (lidbox_gemm_tn_partial -> lidbox_gemm_nt_carry, lidbox_zero_job).  Each row names the source condition it is there for in
   `why`.  Shapes were found by searching the restated planner: the smallest that still select their path.

7. The 32-bit extent guards: limits() reads the limits of sk_extent_ok, sk_b_extent_ok, reduce_job_vec_ok and the inner test of
   store_rows_tile from the source; the guards restated and threaded through rows_dispatch / tn_dispatch / pair_plan; PATHS["FAR"]
   (rows in the zones high / edge-in / edge-out / over of a guard's own expression, C-far rows, the pair and reduce-job rows);
   far_layout, the sparse judge judge_far_rows, and the planted ADDRESSING_MISTAKES on an emulated far gather / scatter.

Largest err / bound seen on the device (one run on one MI355X; the figures per kernel stand in the docstring of
tests/test_gemm_paths_gpu.py): 0.21 (gemm_rows_kernel, K = 36 .. 52); every `exact` case bit-equal.

The 32-bit-extent guards (sk_extent_ok, sk_b_extent_ok, reduce_job_vec_ok's byte limit, the inner test of store_rows_tile) are
restated in section 7 with their limits READ from the source; PATHS["FAR"] holds the rows on both sides of each, which
tests/test_gemm_far_gpu.py runs in sparse allocations (tests/far_buffers.py).  The bf16 families
(gemm_bf16.hip, gemm16_*.h) have their own module, oracle/gemm16_paths_np.py, which imports this one's helpers.
lidbox_gemm_nt_tn_carry with pending jobs stays with tests/test_gemm_sk_gpu.py (bit identity).
"""
import os
import re

import numpy as np

from oracle import conv2d_np

NUM_CU = 256
BK = 16
CAND = [(128, 128), (128, 64), (64, 128), (64, 64)]
TILE_EFF = [1.0, 0.98, 0.97, 0.955]
RESIDENT = [3, 4, 4, 6]
FIXED_STEPS = [6.0, 5.0, 5.0, 3.0]
SK_BM = SK_BN = 128
SK_BK = 16
SK_WGCU, SKP_WGCU = 3, 2
SK_SLAB = SK_BM * SK_BN
SK_COUNTER_BYTES = 16384
SKP_DUMMY_BYTES = NUM_CU * SK_WGCU * 256 * 4
SK_MIN_SPAN = 8
SK_PART_STEPS = 16
DMA_STREAM_MIN_STEPS = 8
DMA_STREAM_MAX_G = 8
EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU_MASK, EPI_ACCUM, EPI_ACCUM_RELU_MASK, EPI_ACCUM_RELU, EPI_RELU = range(8)
EPI_HAS_BIAS = (EPI_BIAS, EPI_BIAS_RELU)
EPI_HAS_MASK = (EPI_RELU_MASK, EPI_ACCUM_RELU_MASK)
EPI_ACCUMS = (EPI_ACCUM, EPI_ACCUM_RELU_MASK, EPI_ACCUM_RELU)
EPI_RELUS = (EPI_BIAS_RELU, EPI_ACCUM_RELU, EPI_RELU)
KIND = {"nn": 0, "nt": 1, "tn": 2}


def cdiv(a, b):
    return (a + b - 1) // b


def _atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


# ------------------------------------------------------------------------------------------------ 1. the host dispatch
_TUNED = None


def tuned_table():
    """the rows of TUNED_GEMM, read from csrc/gemm_tuned.h: (kind, M, N, K) -> (bm, bn, splits, no_tail_split, waves)"""
    global _TUNED
    if _TUNED is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lidbox_amd", "csrc", "gemm_tuned.h")
        with open(path) as f:
            src = f.read()
        _TUNED = {}
        for m in re.finditer(r"^\s*\{\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\s*\},", src, re.M):
            v = [int(x) for x in m.groups()]
            _TUNED.setdefault(tuple(v[:4]), tuple(v[4:]))           # the first match wins, as in tuned_gemm
    return _TUNED


def tuned_gemm(kind, M, N, K, env):
    if "LIDBOX_GEMM_NO_TUNED" in env:
        return None
    return tuned_table().get((kind, M, N, K))


def conc_eff(w):
    if w <= 1.0:
        return 0.55
    if w <= 2.0:
        return 0.55 + 0.25 * (w - 1.0)
    if w <= 3.0:
        return 0.80 + 0.10 * (w - 2.0)
    return 0.92


def launch_cost(c, wgs, ksteps):
    bm, bn = CAND[c]
    tile_t = (bm * bn / 16384.0) * (ksteps + FIXED_STEPS[c]) / TILE_EFF[c]
    per_cu = float(cdiv(wgs, NUM_CU))
    if wgs > NUM_CU and wgs % NUM_CU != 0:
        fluid = wgs / NUM_CU + 0.12
        if fluid < per_cu:
            per_cu = fluid
    conc = wgs / NUM_CU if per_cu < RESIDENT[c] else float(RESIDENT[c])
    return per_cu * tile_t / conc_eff(1.0 if conc < 1.0 else conc)


def _choice(bm, bn, splits, kps, no_tail_split=False, waves=4):
    return dict(bm=bm, bn=bn, splits=splits, kps=kps, no_tail_split=no_tail_split, waves=waves)


def choose_rows(kind, M, N, K, ws_bytes, env):
    t = tuned_gemm(kind, M, N, K, env)
    if t is not None:
        bm, bn, sp, nts, wv = t
        kps = cdiv(cdiv(K, sp), BK) * BK
        splits = cdiv(K, kps)
        if splits == 1 or splits * M * N * 4 <= ws_bytes:
            return _choice(bm, bn, splits, kps, nts != 0, 8 if (wv == 8 and bm == 128) else 4)
    best, best_cost = _choice(128, 128, 1, K), 1e30
    for c in range(4):
        bm, bn = CAND[c]
        tiles = cdiv(M, bm) * cdiv(N, bn)
        s = 1
        while s <= 64:
            kps = cdiv(cdiv(K, s), BK) * BK
            splits = cdiv(K, kps)
            if s > 1 and (splits < 2 or kps < 4 * BK):
                break
            if splits > 1 and splits * M * N * 4 > ws_bytes:
                break
            cost = launch_cost(c, tiles * splits, kps / BK)
            if splits > 1:
                cost += 5.0 + M * N * 4.0 * (splits + 1) / 3.0e6
            if cost < best_cost:
                best_cost, best = cost, _choice(bm, bn, splits, kps)
            if splits < s:
                break
            s *= 2
    return best


def choose_rows_env(kind, M, N, K, wsb, env):
    ch = choose_rows(kind, M, N, K, wsb, env)
    if M >= 4096:
        f = env.get("LIDBOX_GEMM_NT8" if kind == 1 else "LIDBOX_GEMM_NN8")
        if f is not None and _atoi(f) in (64, 128):
            return _choice(128, _atoi(f), 1, K, False, 8)
    f = env.get("LIDBOX_GEMM_PLAN")
    if f is not None:
        m = re.match(r"\s*([+-]?\d+),\s*([+-]?\d+),\s*([+-]?\d+)(?:,\s*([+-]?\d+))?", f)
        if m:
            bm, bn, sp = int(m.group(1)), int(m.group(2)), int(m.group(3))
            wv = int(m.group(4)) if m.group(4) else 4
            if bm in (64, 128) and bn in (64, 128) and sp >= 1:
                kps = cdiv(cdiv(K, sp), BK) * BK
                splits = cdiv(K, kps)
                if splits == 1 or splits * M * N * 4 <= wsb:
                    ch = _choice(bm, bn, splits, kps, False, 8 if (wv == 8 and bm == 128) else 4)
    return ch


def sk_enabled(env):
    return not ("LIDBOX_GEMM_SK" in env and _atoi(env["LIDBOX_GEMM_SK"]) == 0)


def sk_grid(env):
    if "LIDBOX_GEMM_SK_GRID" in env:
        g = _atoi(env["LIDBOX_GEMM_SK_GRID"])
        if 1 <= g <= NUM_CU * SK_WGCU:
            return g
    return NUM_CU * SK_WGCU


def sk_min_flop(env):
    return float(env["LIDBOX_GEMM_SK_MIN_FLOP"]) if "LIDBOX_GEMM_SK_MIN_FLOP" in env else 3.0e9


def sk_all(env):
    return "LIDBOX_GEMM_SK_ALL" in env and _atoi(env["LIDBOX_GEMM_SK_ALL"]) != 0


def skp_mode(env):
    return _atoi(env["LIDBOX_GEMM_SKP"]) if "LIDBOX_GEMM_SKP" in env else 1


def sk_tuned_out(kind, M, N, K, env):
    return (not sk_all(env)) and tuned_gemm(kind, M, N, K, env) is not None


def sk_rows_plan(kind, M, N, K, env, pipelined=False):
    """SkRows as a dict (ok, P, ws_need and the SkPlan fields), or None where the C++ returns ok = false"""
    if not sk_enabled(env) or M < SK_BM or K % 4 != 0 or 2.0 * M * N * K < sk_min_flop(env):
        return None
    if not pipelined and not (sk_all(env) or (kind == 0 and K >= 1024)):
        return None
    P = sk_grid(env)
    if pipelined and P == NUM_CU * SK_WGCU:
        P = NUM_CU * SKP_WGCU
    if P % 8 != 0:
        return None
    tiles_n = cdiv(N, SK_BN)
    T = cdiv(M, SK_BM) * tiles_n
    if T > 0x3fffffff:
        return None
    nk = cdiv(K, SK_BK)
    dp_rounds = T // P
    sk_tiles = T - dp_rounds * P
    parts = 0
    if dp_rounds > 0 and sk_tiles > 0:
        g = nk // SK_PART_STEPS
        lim = (P // 8) // cdiv(sk_tiles, 8)
        if g > lim:
            g = lim
        g = min(max(g, 1), 200)
        wg_cu = P // NUM_CU if P // NUM_CU > 0 else 1
        cu_parts = float(dp_rounds) * nk * wg_cu + float(cdiv(sk_tiles * g, NUM_CU)) * (nk / g)
        cu_spans = 1.05 * T * nk / NUM_CU
        if cu_parts <= cu_spans:
            parts = g
        else:
            dp_rounds -= 1
            sk_tiles = T - dp_rounds * P
    if parts == 0 and sk_tiles > 0 and sk_tiles * nk < P * SK_MIN_SPAN:
        return None
    if parts == 0 and sk_tiles > 0 and (nk * P) // (sk_tiles * nk) + 2 > 250:
        return None
    if sk_tiles * 4 > SK_COUNTER_BYTES:
        return None
    ws_need = SK_COUNTER_BYTES + P * 2 * SK_SLAB * 4 + (SKP_DUMMY_BYTES if pipelined else 0)
    if parts:
        branch, p = "parts", parts
    elif sk_tiles == 0:
        branch, p = "whole", 1
    else:
        branch = "spans_T<P" if T < P else "dp_fallback"
        span = max(1, (sk_tiles * nk) // P)
        p = min(nk, cdiv(nk, span) + 1)
    return dict(P=P, ws_need=ws_need, ntiles=T, nk=nk, dp_rounds=dp_rounds, sk_tiles=sk_tiles, parts=parts, branch=branch, p=p)


def sk_tn_plan(M, K1, N, env):
    if not sk_enabled(env) or K1 % 4 != 0 or N % 4 != 0 or 2.0 * M * N * K1 < 2.0 * sk_min_flop(env):
        return None
    tiles_n = cdiv(N, SK_BN)
    ntiles = cdiv(K1, SK_BM) * tiles_n
    g = max(sk_grid(env) // ntiles, 1)
    rps = cdiv(cdiv(M, g), SK_BK) * SK_BK
    if rps < 8 * SK_BK:
        return None
    rps = min(rps, 8192)
    splits = cdiv(M, rps)
    return dict(splits=splits, rps=rps, ntiles=ntiles, ws_need=(splits * K1 * N + splits * N) * 4)


def dma_mode(env):
    return _atoi(env["LIDBOX_GEMM_DMA"]) if "LIDBOX_GEMM_DMA" in env else 1


def dma_stream_plan(bm, bn, M, N, K, env):
    """DmaStreamPlan: (g, rem, whole, ws_need); g = 0: no streamed remainder"""
    none = dict(g=0, rem=0, whole=0, ws_need=0)
    force = _atoi(env["LIDBOX_GEMM_STREAM_TAIL"]) if "LIDBOX_GEMM_STREAM_TAIL" in env else -1
    if force == 0:
        return none
    tiles = cdiv(M, bm) * cdiv(N, bn)
    rem = tiles % NUM_CU
    if tiles < NUM_CU or rem == 0:
        return none
    nk = cdiv(K, SK_BK)
    best, best_cost = 1, 1.0
    g = 2
    while g <= DMA_STREAM_MAX_G and nk // g >= DMA_STREAM_MIN_STEPS:
        cost = cdiv(rem * g, NUM_CU) / g + 0.03 + 0.01 * g
        if cost < best_cost - 1e-9:
            best_cost, best = cost, g
        g += 1
    if force > 1 and nk // force >= 2 and force <= 64:
        best = force
    elif best_cost > 0.9:
        return none
    if best < 2:
        return none
    return dict(g=best, rem=rem, whole=tiles - rem, ws_need=SK_COUNTER_BYTES + rem * best * bm * bn * 4)


def cand_index(bm, bn):
    return (0 if bn == 128 else 1) if bm == 128 else (2 if bn == 128 else 3)


def rows_al(a_res, a_rs, a_batch, a_bs, K, b_res, ldb, N, kind):
    """the `al` predicate of launch_rows; *_res: the pointer's residue modulo 16"""
    return (a_res == 0 and a_rs % 4 == 0 and (a_batch == 1 or a_bs % 4 == 0) and K % 4 == 0 and b_res == 0 and ldb % 4 == 0
            and (kind == 1 or N % 4 == 0))


def _kin(kind):
    return "nt" if kind == 1 else "nn"


def _range_launch(out, ch, kind, al, dma_ok, env, stream_g=0):
    """launch_rows_range: counters, family and kernel names of one launch (+ its reduce)"""
    if out["launches"][0] == 0:
        out["first_tile"] = (ch["bm"], ch["bn"])
    out["launches"][0 if (ch["bm"], ch["bn"]) == out["first_tile"] else 1] += 1
    if ch["splits"] > 1:
        out["launches"][2] += 1
    t = "%d,%d,%s" % (ch["bm"], ch["bn"], _kin(kind))
    eight = ch["waves"] == 8 and ch["bm"] == 128
    if dma_ok and al and dma_mode(env) != 0:
        out["family"] = 3 if eight else 1
        out["kernels"].append("gemm_rows_dma8_kernel<%d,%s>" % (ch["bn"], _kin(kind)) if eight else "gemm_rows_dma_kernel<%s>" % t)
        if stream_g > 1 and ch["splits"] == 1:
            out["g"] = stream_g
    elif eight:
        out["kernels"].append("gemm_rows8_kernel<%s,%s>" % (t, "al" if al else "un"))
    else:
        out["kernels"].append("gemm_rows_kernel<%s,%s>" % (t, "al" if al else "un"))
    if ch["splits"] > 1:
        out["kernels"].append("rows_reduce_kernel")
    out["p"] = max(out["p"], ch["splits"], out["g"])


def rows_dispatch(kind, M, N, K, al, ws_bytes, env, epi=EPI_NONE, ws_al=True, c_batch=1, c_rpb=0, c_rs=None, c_bs=0, c_res=0,
                  aux_res=0, a_ext=True, b_ext=True):
    """what launch_rows does: dict(family, kernels, launches, g, p, sk, tail_split, ch).  a_ext / b_ext: sk_extent_ok(A, K) and
    sk_b_extent_ok(B_KINNER, K, N, ldb) of the call (section 7; True for every operand far below the limits)"""
    out = dict(family=0, kernels=[], launches=[0, 0, 0], g=0, p=1, sk=None, tail_split=False, ch=None, first_tile=None)
    if M == 0 or N == 0:
        return out
    wsb = ws_bytes
    ch = choose_rows_env(kind, M, N, K, wsb, env)
    out["ch"] = ch
    c_rs = N if c_rs is None else c_rs
    if al and "LIDBOX_GEMM_PLAN" not in env and ws_al and not sk_tuned_out(kind, M, N, K, env) and b_ext:
        has_mask = epi in EPI_HAS_MASK
        skp_ok = (skp_mode(env) != 0 and (c_batch == 1 or c_rpb >= 32) and N % 4 == 0 and c_res == 0 and c_rs % 4 == 0
                  and (c_batch == 1 or c_bs % 4 == 0) and (not has_mask or aux_res == 0) and skp_mode(env) == 2)
        for pipelined in ((True, False) if skp_ok else (False,)):
            sk = sk_rows_plan(kind, M, N, K, env, pipelined)
            if sk is not None and wsb >= sk["ws_need"] and a_ext:
                out.update(family=2, launches=[1, 0, 0], sk=sk, p=sk["p"], first_tile=(SK_BM, SK_BN))
                if pipelined:
                    out["kernels"] = ["gemm_skp_rows_kernel<%s,%s,%s>" % (_kin(kind), "mask" if has_mask else "nomask",
                                                                         "acc" if epi in EPI_ACCUMS else "noacc")]
                else:
                    out["kernels"] = ["gemm_sk_rows_kernel<%s>" % _kin(kind)]
                return out
    dma_ok = al and a_ext and b_ext
    if dma_ok and dma_mode(env) != 0 and ch["splits"] == 1 and ws_al:
        spl = dma_stream_plan(ch["bm"], ch["bn"], M, N, K, env)
        if spl["g"] > 1 and wsb >= spl["ws_need"]:
            _range_launch(out, ch, kind, al, dma_ok, env, spl["g"])
            return out
    no_tail_split = ch["no_tail_split"] or "LIDBOX_GEMM_NO_TAIL_SPLIT" in env
    if not no_tail_split and ch["splits"] == 1:
        tiles_n, tiles_m = cdiv(N, ch["bn"]), cdiv(M, ch["bm"])
        wgs = tiles_m * tiles_n
        rounds = wgs // NUM_CU
        if rounds >= 1 and wgs % NUM_CU != 0:
            main_tiles_m = rounds * NUM_CU // tiles_n
            m_main = main_tiles_m * ch["bm"]
            m_rem = M - m_main
            if main_tiles_m >= 1 and m_rem > 0:
                rem = choose_rows(kind, m_rem, N, K, wsb, env)
                c, cr = cand_index(ch["bm"], ch["bn"]), cand_index(rem["bm"], rem["bn"])
                ksteps = float(cdiv(K, BK))
                whole = launch_cost(c, wgs, ksteps)
                split = (launch_cost(c, main_tiles_m * tiles_n, ksteps) + 4.0 +
                         launch_cost(cr, cdiv(m_rem, rem["bm"]) * cdiv(N, rem["bn"]) * rem["splits"], rem["kps"] / BK))
                if rem["splits"] > 1:
                    split += 5.0 + m_rem * N * 4.0 * (rem["splits"] + 1) / 3.0e6
                if split < 0.97 * whole:
                    out["tail_split"] = True
                    out["m_main"] = m_main
                    _range_launch(out, ch, kind, al, dma_ok, env)
                    _range_launch(out, rem, kind, al, dma_ok, env)
                    return out
    _range_launch(out, ch, kind, al, dma_ok, env)
    return out


def plan_is_stream_k(kind, M, N, K, wsb, env):
    """lidbox_gemm_plan_is_stream_k"""
    if kind == 2:
        t = sk_tn_plan(M, K, N, env)
        return int(t is not None and wsb >= t["ws_need"] and not sk_tuned_out(2, M, N, K, env))
    r = sk_rows_plan(kind, M, N, K, env)
    return int(r is not None and wsb >= r["ws_need"] and (kind == 1 or N % 4 == 0) and not sk_tuned_out(kind, M, N, K, env))


def plan_stream_tail(kind, M, N, K, wsb, env):
    """lidbox_gemm_plan_stream_tail"""
    if dma_mode(env) == 0:
        return 0
    if "LIDBOX_GEMM_PLAN" not in env and plan_is_stream_k(kind, M, N, K, wsb, env):
        return 0
    ch = choose_rows_env(kind, M, N, K, wsb, env)
    if ch["splits"] != 1:
        return 0
    spl = dma_stream_plan(ch["bm"], ch["bn"], M, N, K, env)
    return spl["g"] if (spl["g"] > 1 and wsb >= spl["ws_need"]) else 0


def rows_workspace(M, N, K, env):
    """lidbox_gemm_rows_workspace"""
    need = 0
    for kind in (0, 1):
        ch = choose_rows(kind, M, N, K, 64 << 20, env)
        if ch["splits"] > 1:
            need = max(need, ch["splits"] * M * N * 4)
    for bm in (64, 128):
        for bn in (64, 128):
            spl = dma_stream_plan(bm, bn, M, N, K, env)
            if spl["g"] > 1:
                need = max(need, spl["ws_need"])
    for kind in (0, 1):
        sk = sk_rows_plan(kind, M, N, K, env)
        if sk is not None:
            need = max(need, sk["ws_need"])
        if skp_mode(env) == 2:
            skp = sk_rows_plan(kind, M, N, K, env, True)
            if skp is not None:
                need = max(need, skp["ws_need"])
    return need


def tn_plan(M, K1, N, env):
    f = env.get("LIDBOX_GEMM_TN_PLAN")
    if f is not None:
        m = re.match(r"\s*([+-]?\d+),\s*([+-]?\d+),\s*([+-]?\d+)", f)
        if m:
            bm, bn, sp = (int(x) for x in m.groups())
            if bm in (64, 128) and bn in (64, 128) and sp >= 1:
                rps = cdiv(cdiv(M, sp), BK) * BK
                return dict(bm=bm, bn=bn, splits=cdiv(M, rps), rps=rps)
    t = tuned_gemm(2, M, N, K1, env)
    if t is not None:
        rps = cdiv(cdiv(M, t[2]), BK) * BK
        return dict(bm=t[0], bn=t[1], splits=cdiv(M, rps), rps=rps)
    best, best_cost = dict(bm=128, bn=128, splits=1, rps=M), 1e30
    for c in range(4):
        bm, bn = CAND[c]
        tiles = cdiv(K1, bm) * cdiv(N, bn)
        target = NUM_CU
        while target <= 8 * NUM_CU:
            s = max(target // tiles, 1)
            s = max(min(s, cdiv(M, 4 * BK)), 1)
            rps = cdiv(cdiv(M, s), BK) * BK
            s = cdiv(M, rps)
            cost = launch_cost(c, tiles * s, rps / BK) + 5.0 + K1 * N * 4.0 * (s + 1) / 3.0e6
            if cost < best_cost:
                best_cost, best = cost, dict(bm=bm, bn=bn, splits=s, rps=rps)
            target += NUM_CU // 2
    return best


def tn_workspace(M, K1, N, env):
    """lidbox_gemm_tn_workspace"""
    pl = tn_plan(M, K1, N, env)
    need = (pl["splits"] * K1 * N + pl["splits"] * N) * 4
    sk = sk_tn_plan(M, K1, N, env)
    return max(need, sk["ws_need"]) if sk is not None else need


def reduce_job_vec_ok(p_res, splits, K1, N, c_res, ldc, bias_grad, bg_res=0):
    """reduce_job_vec_ok with Pc = P + splits K1 N floats; *_res: residues modulo 16"""
    n = K1 * N
    pc_res = (p_res + 4 * splits * n) % 16
    return (N % 4 == 0 and ldc % 4 == 0 and n % 4 == 0 and p_res == 0 and c_res == 0 and
            (not bias_grad or (pc_res == 0 and bg_res == 0)) and job_guard(splits, n) < limits()["job_bytes"])


def tn_dispatch(M, K1, N, a_al, b_al, ws_bytes, env, ws_res=0, c_res=0, ldc=None, bias_grad=True, bg_res=0, a_ext=True, b_ext=True):
    """what tn_partial_launch + run_reduce_jobs do: dict(family, kernels, launches, splits, rps).  a_ext / b_ext:
    sk_extent_ok(A, K1) and sk_extent_ok(Bd, N), tested at the stream-K gate and again at the LDS-DMA gate"""
    ldc = N if ldc is None else ldc
    sk = sk_tn_plan(M, K1, N, env)
    if (sk is not None and "LIDBOX_GEMM_TN_PLAN" not in env and not sk_tuned_out(2, M, N, K1, env) and ws_res == 0 and
            ws_bytes >= sk["ws_need"] and a_al and b_al and a_ext and b_ext):
        fam, kern, splits, rps = 2, "gemm_sk_tn_kernel", sk["splits"], sk["rps"]
    else:
        pl = tn_plan(M, K1, N, env)
        splits, rps = pl["splits"], pl["rps"]
        al = a_al and b_al and K1 % 4 == 0 and N % 4 == 0
        if al and dma_mode(env) != 0 and a_ext and b_ext and rps % SK_BK == 0:
            fam, kern = 1, "gemm_tn_dma_kernel<%d,%d>" % (pl["bm"], pl["bn"])
        else:
            fam, kern = 0, "gemm_tn_kernel<%d,%d,%s>" % (pl["bm"], pl["bn"], "al" if al else "un")
    vec = reduce_job_vec_ok(ws_res, splits, K1, N, c_res, ldc, bias_grad, bg_res)
    return dict(family=fam, kernels=[kern, "splitk_reduce4_kernel" if vec else "splitk_reduce_kernel"], launches=[1, 0, 1],
                splits=splits, rps=rps, p=splits)


def pair_plan(M, Co, N, K1, ws_nt_bytes, ws_tn_bytes, env, al_rows=True, al_tn=True):
    """pair_plan / lidbox_gemm_plan_is_pair: (ch, pl) or None.  al_rows / al_tn: the two operand predicates of lidbox_gemm_nt_tn in
    front of pair_plan (pair_al_rows, pair_al_tn), each refusing the pair on its own"""
    if not (al_rows and al_tn):
        return None
    if dma_mode(env) == 0 or "LIDBOX_GEMM_NO_PAIR" in env or min(M, N, K1, Co) < 1 or Co % 4 != 0 or K1 % 4 != 0:
        return None
    ch = choose_rows_env(1, M, N, Co, ws_nt_bytes, env)
    pl = tn_plan(M, K1, Co, env)
    sk = sk_tn_plan(M, K1, Co, env)
    sk_rows = "LIDBOX_GEMM_PLAN" not in env and plan_is_stream_k(1, M, N, Co, ws_nt_bytes, env)
    sk_tn = sk is not None and "LIDBOX_GEMM_TN_PLAN" not in env and not sk_tuned_out(2, M, Co, K1, env) and ws_tn_bytes >= sk["ws_need"]
    tn_need = (pl["splits"] * K1 * Co + pl["splits"] * Co) * 4
    rows_blocks = cdiv(M, 64) * cdiv(N, 64) * ch["splits"]
    tn_blocks = cdiv(K1, 64) * cdiv(Co, 64) * pl["splits"]
    cap = int(env["LIDBOX_GEMM_PAIR_MAX_BLOCKS"]) if "LIDBOX_GEMM_PAIR_MAX_BLOCKS" in env else 12 * NUM_CU
    if not ((ch["bm"], ch["bn"], ch["waves"]) == (64, 64, 4) and (pl["bm"], pl["bn"]) == (64, 64) and not sk_rows and not sk_tn and
            ws_tn_bytes >= tn_need and (ch["splits"] == 1 or ch["splits"] * M * N * 4 <= ws_nt_bytes) and
            rows_blocks + tn_blocks <= cap):
        return None
    return ch, pl


def colsum_slices(M):
    return max(1, min(128, cdiv(M, 256)))


def colsum_workspace(M, N):
    return colsum_slices(M) * N * 4


def instantiations():
    """every kernel instantiation the oracle's predictions can name (launch_rows_t, launch_rows8_t, launch_tn_t, LBX_ROWS_DMA,
    the two gemm_rows_dma8_kernel sites, LBX_TN_DMA, LBX_SKP, the stream-K, pair, reduce and colsum sites); the CPU test holds it
    equal to instantiations_from_source(), the enumeration of the launch sites in the source text"""
    tiles = ["%d,%d" % t for t in CAND]
    out = ["gemm_rows_kernel<%s,%s,%s>" % (t, k, a) for t in tiles for k in ("nn", "nt") for a in ("al", "un")]
    out += ["gemm_rows8_kernel<128,%d,%s,%s>" % (bn, k, a) for bn in (128, 64) for k in ("nn", "nt") for a in ("al", "un")]
    out += ["gemm_tn_kernel<%s,%s>" % (t, a) for t in tiles for a in ("al", "un")]
    out += ["gemm_rows_dma_kernel<%s,%s>" % (t, k) for t in tiles for k in ("nn", "nt")]
    out += ["gemm_rows_dma8_kernel<%d,%s>" % (bn, k) for bn in (128, 64) for k in ("nn", "nt")]
    out += ["gemm_tn_dma_kernel<%s>" % t for t in tiles]
    out += ["gemm_nt_tn_pair_kernel", "gemm_sk_tn_kernel"]
    out += ["gemm_sk_rows_kernel<%s>" % k for k in ("nn", "nt")]
    out += ["gemm_skp_rows_kernel<%s,%s,%s>" % (k, m, a) for k in ("nn", "nt") for m in ("mask", "nomask") for a in ("acc", "noacc")]
    out += ["rows_reduce_kernel", "splitk_reduce_kernel", "splitk_reduce4_kernel", "colsum_stage1", "colsum_stage2"]
    return out


# ------------------------------------------------------------------------------------------------ 2. references
def row_offsets(d, M=None):
    """element offset of every row of a (batch, rpb, rs, bs) descriptor"""
    M = d["batch"] * d["rpb"] if M is None else M
    m = np.arange(M, dtype=np.int64)
    if d["batch"] == 1:
        return m * d["rs"]
    return (m // d["rpb"]) * d["bs"] + (m % d["rpb"]) * d["rs"]


def extent(d, cols):
    M = d["batch"] * d["rpb"]
    return int(row_offsets(d).max()) + cols if M else cols


def index(d, cols):
    """[M, cols] element offsets"""
    return row_offsets(d)[:, None] + np.arange(cols, dtype=np.int64)[None, :]


def gather(flat, d, cols):
    if d["batch"] == 1 and d["rs"] == cols:
        return np.asarray(flat)[:d["rpb"] * cols].reshape(d["rpb"], cols)
    return np.asarray(flat)[index(d, cols)]


def apply_epi(v, epi, bias=None, mask=None, old=None):
    """apply_epi of gemm_shared.h on arrays (any float type)"""
    if epi == EPI_BIAS:
        return v + bias
    if epi == EPI_BIAS_RELU:
        return np.maximum(v + bias, 0)
    if epi == EPI_RELU_MASK:
        return np.where(mask > 0, v, 0)
    if epi == EPI_ACCUM:
        return v + old
    if epi == EPI_ACCUM_RELU_MASK:
        return old + np.where(mask > 0, v, 0)
    if epi == EPI_ACCUM_RELU:
        return np.maximum(old + v, 0)
    if epi == EPI_RELU:
        return np.maximum(v, 0)
    return v


def product(kind, A, B):
    """float64 A . B (nn: B [K, N]), A . B^T (nt: B [N, K]) or A^T . B (tn)"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return A @ B if kind == "nn" else (A @ B.T if kind == "nt" else A.T @ B)


def rows_reference(kind, A, B, epi, bias=None, mask=None, old=None):
    """(reference, S): the float64 result and the same expression on absolute values (what the bound scales with)"""
    f = lambda x: None if x is None else np.asarray(x, np.float64)
    v = product(kind, A, B)
    S = product(kind, np.abs(A), np.abs(B))
    if epi in EPI_HAS_BIAS:
        S = S + np.abs(f(bias))
    if epi in EPI_ACCUMS:
        S = S + np.abs(f(old))
    return apply_epi(v, epi, f(bias), f(mask), f(old)), S


# ------------------------------------------------------------------------------------------------ 3. bounds
def chain_n(K, p, epi):
    return 2 * K + p + 1 + (1 if (epi in EPI_HAS_BIAS or epi in EPI_ACCUMS) else 0)


def ratio(got, ref, S, n):
    """err / bound per element; an element that is not finite counts as infinitely wrong"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    q = np.abs(got - ref) / conv2d_np.error_bound(S, n)
    return np.where(np.isfinite(got), q, np.inf)


def colsum_n(M):
    s = colsum_slices(M)
    return cdiv(cdiv(M, s), 4) + 3 + s + 1


def bias_grad_n(rps, splits):
    return rps + splits + 1


# ------------------------------------------------------------------------------------------------ 4. data
DATASETS = ("normal", "offset", "exact")


def draw(rng, ds, shape, what="ab"):
    """what: 'ab' operands, 'int' bias / old C, 'mask'"""
    if what == "mask":
        if ds == "exact":
            return rng.choice(np.array([-2.0, -0.0, 0.0, 3.0], np.float32), size=shape)
        return rng.standard_normal(shape).astype(np.float32)
    if ds == "normal":
        return rng.standard_normal(shape).astype(np.float32)
    if ds == "offset":
        return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
    if what == "ab":
        return (rng.integers(1, 8, size=shape) * rng.choice([-1, 1], size=shape)).astype(np.float32)
    return rng.integers(-9, 10, size=shape).astype(np.float32)


def fill_flat(rng, ds, d, cols, what="ab"):
    """a flat buffer of the descriptor's extent: drawn values where a row covers, NaN in the gaps"""
    n = extent(d, cols)
    if d["batch"] == 1 and d["rs"] == cols:                         # dense: every element is covered
        return np.ascontiguousarray(draw(rng, ds, n, what))
    flat = np.full(n, np.nan, np.float32)
    cover = np.zeros(n, bool)
    cover[index(d, cols).ravel()] = True
    flat[cover] = draw(rng, ds, int(cover.sum()), what)
    return flat


# ------------------------------------------------------------------------------------------------ 5. emulation + mutations
MUTATIONS = ("drop_k_step", "drop_k_tail", "tail_not_zeroed", "col_shift_32", "row_from_0", "wrap_early", "wrap_late",
             "mask_dense", "bias_next", "no_accum", "no_relu", "slab_twice", "slab_omitted", "bias_grad_slice_omitted")


def applies(mut, r):
    """whether planting `mut` can change the result of row r: the explicit exclusion rules of the mutation check"""
    kind = r.get("kind", "tn")
    if r["M"] == 0 or r.get("N", 1) == 0:
        return False
    Kc = r["M"] if kind == "tn" else r["K"]                      # contracted length
    epi = r.get("epi", EPI_NONE)
    pieces = r.get("emu_pieces", 1)
    if mut == "drop_k_step":
        return cdiv(Kc, BK) >= 3 * pieces                           # an interior step exists
    if mut in ("drop_k_tail", "tail_not_zeroed"):
        return Kc % BK != 0                                         # no tail step with K % 16 = 0
    if mut == "col_shift_32":
        return r["N"] > 32
    if mut == "row_from_0":
        return (r["K1"] if kind == "tn" else r["M"]) > 1
    if mut in ("wrap_early", "wrap_late"):                          # a dense C has no utterance boundary; wrap = 0: adding it is a no-op
        return kind != "tn" and r["c"]["batch"] > 1 and r["c"]["bs"] != r["c"]["rpb"] * r["c"]["rs"]
    if mut == "mask_dense":                                         # a dense C: the pitched offset IS the dense offset
        return epi in EPI_HAS_MASK and not (r["c"]["batch"] == 1 and r["c"]["rs"] == r["N"])
    if mut == "bias_next":
        return epi in EPI_HAS_BIAS and r["N"] > 1
    if mut == "no_accum":
        return epi in EPI_ACCUMS or (kind == "tn" and r.get("accumulate", 0) == 1)
    if mut == "no_relu":
        return epi in EPI_RELUS
    if mut in ("slab_twice", "slab_omitted"):
        return pieces > 1
    if mut == "bias_grad_slice_omitted":
        return kind == "tn" and r.get("bias_grad", False) and pieces > 1
    raise KeyError(mut)


def _steps(Kc, pieces):
    """[(piece, k0, k1)] of 16-deep steps; the contraction is cut into `pieces` runs of whole steps"""
    nk = cdiv(Kc, BK)
    per = cdiv(nk, pieces)
    return [(s // per, s * BK, min(Kc, s * BK + BK)) for s in range(nk)]


def emulate_rows(kind, A, B, epi, bias, mask_flat, c_flat, c_desc, pieces=1, mut=None):
    """fp32: 16-deep K steps accumulated per piece, pieces summed in k order, epilogue, pitched store into a copy of c_flat
    (NaN in the gaps; the old values where the epilogue accumulates).  mask_flat is laid out like C."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    Bk = B if kind == "nn" else B.T                                # [K, N]
    M, K = A.shape
    N = Bk.shape[1]
    steps = _steps(K, pieces)
    npieces = steps[-1][0] + 1
    part = np.zeros((npieces, M, N), np.float32)
    for i, (pc, k0, k1) in enumerate(steps):
        last = i == len(steps) - 1
        if mut == "drop_k_step" and i == len(steps) // 2 and 0 < i < len(steps) - 1:
            continue
        if mut == "drop_k_tail" and last and K % BK:
            continue
        a, b = A[:, k0:k1], Bk[k0:k1]
        if mut == "tail_not_zeroed" and last and K % BK:          # the stale LDS tile: what the step before left there
            pad = BK - (k1 - k0)
            a = np.concatenate([a, A[:, k0 - pad:k0] if k0 >= pad else np.ones((M, pad), np.float32)], 1)
            b = np.concatenate([b, Bk[k0 - pad:k0] if k0 >= pad else np.ones((pad, N), np.float32)], 0)
        if mut == "row_from_0" and i == 0:
            a = a.copy()
            a[M - 1] = a[0]
        part[pc] += a @ b
    if mut == "row_from_0" and len(steps) > 1:                       # the clamped row for every step
        part[:, M - 1] = part[:, 0]
    if mut == "slab_twice":
        part[npieces - 1] *= 2
    if mut == "slab_omitted":
        part[npieces - 1] = 0
    v = np.zeros((M, N), np.float32)
    for pc in range(npieces):
        v = v + part[pc]
    if mut == "col_shift_32":
        v = np.roll(v, -32, axis=1)
    idx = index(c_desc, N)
    if mut in ("wrap_early", "wrap_late"):
        m = np.arange(M)
        rpb, wrap = c_desc["rpb"], c_desc["bs"] - c_desc["rpb"] * c_desc["rs"]
        off = row_offsets(c_desc).copy()
        if mut == "wrap_early":                                     # the last row of an utterance already carries the wrap
            off[m % rpb == rpb - 1] += wrap
        else:                                                       # the first row of an utterance does not carry it yet
            off[(m % rpb == 0) & (m >= rpb)] -= wrap
        idx = off[:, None] + np.arange(N)[None, :]
    out = np.array(c_flat, np.float32)
    pad = max(0, int(idx.max()) + 1 - out.size)
    out = np.concatenate([out, np.full(pad, np.nan, np.float32)])
    old = out[np.minimum(index(c_desc, N), out.size - 1)]
    b_ = None
    if epi in EPI_HAS_BIAS:
        b_ = np.asarray(bias, np.float32)
        if mut == "bias_next":
            b_ = np.roll(b_, -1)
    mk = None
    if epi in EPI_HAS_MASK:
        mflat = np.asarray(mask_flat, np.float32)
        mk = mflat[(np.arange(M)[:, None] * N + np.arange(N)[None, :]) % mflat.size] if mut == "mask_dense" else mflat[index(c_desc, N)]
    e = epi
    if mut == "no_accum":
        e = {EPI_ACCUM: EPI_NONE, EPI_ACCUM_RELU_MASK: EPI_RELU_MASK, EPI_ACCUM_RELU: EPI_RELU}.get(epi, epi)
    if mut == "no_relu":
        e = {EPI_BIAS_RELU: EPI_BIAS, EPI_ACCUM_RELU: EPI_ACCUM, EPI_RELU: EPI_NONE}.get(epi, epi)
    res = np.asarray(apply_epi(v, e, b_, mk, old), np.float32)
    # rows are stored in order; where a mutated offset collides with a true one the later row wins
    out[idx] = res
    return out


def emulate_tn(A, B, old_c, ldc, accumulate, old_bg, rps, mut=None):
    """fp32 wgrad: slices of rps contracted rows, 16-deep steps, slices summed in order; returns (dW flat [K1, ldc], bias grad)"""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    M, K1 = A.shape
    N = B.shape[1]
    splits = cdiv(M, rps)
    P = np.zeros((splits, K1, N), np.float32)
    Pc = np.zeros((splits, N), np.float32)
    for s in range(splits):
        m0, m1 = s * rps, min(M, s * rps + rps)
        steps = _steps(m1 - m0, 1)
        for i, (_, k0, k1) in enumerate(steps):
            last = i == len(steps) - 1 and s == splits - 1
            if mut == "drop_k_step" and s == 0 and i == len(steps) // 2 and 0 < i < len(steps) - 1:
                continue
            if mut == "drop_k_tail" and last and M % BK:
                continue
            a, b = A[m0 + k0:m0 + k1], B[m0 + k0:m0 + k1]
            if mut == "tail_not_zeroed" and last and M % BK:
                pad = BK - (k1 - k0)
                a = np.concatenate([a, np.ones((pad, K1), np.float32)], 0)
                b = np.concatenate([b, np.ones((pad, N), np.float32)], 0)
            P[s] += a.T @ b
            Pc[s] += b.sum(0, dtype=np.float32)
    if mut == "row_from_0":
        P[:, K1 - 1] = P[:, 0]
    if mut == "slab_twice":
        P[splits - 1] *= 2
    if mut == "slab_omitted":
        P[splits - 1] = 0
    if mut == "bias_grad_slice_omitted":
        Pc[splits - 1] = 0
    v = np.zeros((K1, N), np.float32)
    g = np.zeros(N, np.float32)
    for s in range(splits):
        v, g = v + P[s], g + Pc[s]
    if mut == "col_shift_32":
        v = np.roll(v, -32, axis=1)
    out = np.array(old_c, np.float32).reshape(K1, ldc).copy()
    acc = accumulate and mut != "no_accum"
    out[:, :N] = out[:, :N] + v if acc else v
    bg = None
    if old_bg is not None:
        bg = np.asarray(old_bg, np.float32) + g if acc else g
    return out, bg


# ------------------------------------------------------------------------------------------------ 6. PATHS
def _dense(M, cols, pitch=0):
    return dict(batch=1, rpb=M, rs=cols + pitch, bs=0)


def _batched(batch, rpb, cols, pitch=0, gap=0):
    """`gap` floats between utterances (wrap = gap), rows `pitch` floats apart beyond cols"""
    rs = cols + pitch
    return dict(batch=batch, rpb=rpb, rs=rs, bs=rpb * rs + gap)


def _conv(batch, T, C, k, s):
    """overlapping causal windows of a padded [batch, T + k - 1, C] activation: K = k C, row stride s C"""
    return dict(batch=batch, rpb=(T - 1) // s + 1, rs=s * C, bs=(T + k - 1) * C)


SK_ENV = {"LIDBOX_GEMM_SK_ALL": "1", "LIDBOX_GEMM_SK_MIN_FLOP": "0"}
_TILES = [(128, 128, 4), (128, 64, 4), (64, 128, 4), (64, 64, 4), (128, 128, 8), (128, 64, 8)]


def _row(name, why, kind, N, K, a, c=None, epi=EPI_NONE, env=None, mis=None, ldb_pad=0, ws="lib", expect=None, **kw):
    M = a["batch"] * a["rpb"]
    c = _dense(M, N) if c is None else c
    assert c["batch"] * c["rpb"] == M, name
    r = dict(name=name, why=why, kind=kind, M=M, N=N, K=K, a=a, c=c, epi=epi, env=dict(env or {}), mis=dict(mis or {}),
             ldb_pad=ldb_pad, ws=ws, expect=dict(expect or {}))
    r.update(kw)
    return r


def _plan(bm, bn, sp=1, wv=4):
    return {"LIDBOX_GEMM_PLAN": "%d,%d,%d,%d" % (bm, bn, sp, wv)}


def _rows_table():
    T = []
    NODMA = {"LIDBOX_GEMM_DMA": "0"}
    # -- the `al` predicate: each term false on its own -> the unaligned register-staged kernel; at every tile and wave count
    terms = [("Abase", dict(mis={"A": 1})), ("Ars", dict(apitch=1)), ("K%4", dict(dK=1)), ("Bbase", dict(mis={"B": 1})),
             ("ldb", dict(ldb_pad=1)), ("N%4", dict(dN=1, only="nn"))]
    i = 0
    for bm, bn, wv in _TILES:
        for kind in ("nn", "nt"):
            tname, t = terms[i % len(terms)]
            if t.get("only", kind) != kind:
                tname, t = terms[(i + 1) % len(terms)]
            i += 1
            M, N, K = bm + 1, bn + 32 + (0 if t.get("dN") is None else 1), 36 + t.get("dK", 0)
            kern = ("gemm_rows8_kernel<%d,%d,%s,un>" if wv == 8 else "gemm_rows_kernel<%d,%d,%s,un>") % (bm, bn, kind)
            T.append(_row("un-%dx%dw%d-%s-%s" % (bm, bn, wv, kind, tname), "launch_rows: al false by %s -> %s" % (tname, kern), kind, N, K,
                          _dense(M, K, t.get("apitch", 0)), epi=i % 8, env=_plan(bm, bn, 1, wv), mis=t.get("mis"),
                          ldb_pad=t.get("ldb_pad", 0), ws="none", expect=dict(family=0, kernel=kern)))
            # aligned operands with LIDBOX_GEMM_DMA=0: the aligned register-staged kernel; pitched A with NaN behind K
            kern = kern.replace(",un>", ",al>")
            env = dict(_plan(bm, bn, 1, wv), **NODMA)
            T.append(_row("al-%dx%dw%d-%s" % (bm, bn, wv, kind), "launch_rows_range: LIDBOX_GEMM_DMA=0, al -> %s" % kern, kind, bn + 36,
                          40 + 4 * (i % 4), _dense(bm + 1, 40 + 4 * (i % 4), 4), epi=(i + 3) % 8, env=env, ldb_pad=4, ws="none",
                          expect=dict(family=0, kernel=kern)))
            # the same tile on the LDS-DMA path
            kern = ("gemm_rows_dma8_kernel<%d,%s>" % (bn, kind)) if wv == 8 else "gemm_rows_dma_kernel<%d,%d,%s>" % (bm, bn, kind)
            T.append(_row("dma-%dx%dw%d-%s" % (bm, bn, wv, kind), "launch_rows_range: dma_ok && al -> %s" % kern, kind, bn + 36,
                          40 + 4 * (i % 4), _dense(bm + 1, 40 + 4 * (i % 4), 4), epi=(i + 5) % 8, env=_plan(bm, bn, 1, wv), ldb_pad=4,
                          ws="none", expect=dict(family=3 if wv == 8 else 1, kernel=kern)))
    # remaining al terms that the rotation above met only once: every term on the 64 x 64 tile, both kinds
    for tname, t in terms:
        for kind in ("nn", "nt"):
            if t.get("only", kind) != kind:
                continue
            T.append(_row("alterm-%s-%s" % (tname, kind), "launch_rows: al term %s false on its own" % tname, kind, 68 + (1 if t.get("dN") else 0),
                          20 + t.get("dK", 0), _dense(70, 20 + t.get("dK", 0), t.get("apitch", 0)), epi=EPI_BIAS, env=_plan(64, 64),
                          mis=t.get("mis"), ldb_pad=t.get("ldb_pad", 0), ws="none",
                          expect=dict(family=0, kernel="gemm_rows_kernel<64,64,%s,un>" % kind)))
    T.append(_row("alterm-Abs-nt", "rows_aligned: batch_stride % 4 != 0 with batch > 1", "nt", 64, 16, _batched(2, 33, 16, 0, 1),
                  env=_plan(64, 64), ws="none", expect=dict(family=0, kernel="gemm_rows_kernel<64,64,nt,un>")))
    # -- K: 1; 15 / 16 / 17; aligned tails K % 16 in {4, 8, 12}; per-element tails K % 4 in {1, 2, 3}
    for K in (1, 15, 16, 17, 20, 24, 28, 33, 34, 35):
        for kind, env, fam in (("nn", NODMA, 0), ("nt", {}, 1 if K % 4 == 0 else 0)):
            T.append(_row("K%d-%s" % (K, kind), "KInnerLoader / KOuterLoader tail step at K = %d" % K, kind, 68, K, _dense(65, K),
                          epi=EPI_ACCUM if K % 2 else EPI_BIAS_RELU, env=dict(_plan(64, 64), **env), ws="none", expect=dict(family=fam)))
    # -- split-K through rows_reduce_kernel: every epilogue; last split shorter; last split a lone tail step
    for epi in range(8):
        kind = "nn" if epi % 2 else "nt"
        T.append(_row("splitk-epi%d" % epi, "rows_reduce_kernel: epilogue %d; last split shorter (K = 148: 80 + 68)" % epi, kind, 68, 148,
                      _dense(70, 148), c=_batched(2, 35, 68, 4, 8), epi=epi, env=_plan(64, 64, 2), ws="lib+plan",
                      expect=dict(family=1, launches=[1, 0, 1], splits=2)))
    T.append(_row("splitk-lone-tail", "split-K whose last split is a lone tail step (K = 100: 48 + 48 + 4)", "nn", 64, 100, _dense(64, 100),
                  epi=EPI_RELU, env=dict(_plan(64, 64, 3), **NODMA), ws="lib+plan", expect=dict(family=0, launches=[1, 0, 1], splits=3)))
    T.append(_row("splitk-big-reduce", "rows_reduce_kernel: M N > 2048 * 256, the grid-stride loop runs twice", "nt", 1024, 128,
                  _dense(520, 128), epi=EPI_ACCUM_RELU, env=_plan(128, 128, 2), ws="lib+plan",
                  expect=dict(family=1, launches=[1, 0, 1], splits=2)))
    T.append(_row("splitk-ws-short", "choose_rows_env: a workspace one byte short keeps the planner's choice, not the PLAN's split", "nn", 64,
                  100, _dense(64, 100), env=_plan(64, 64, 3), ws="plan-1", expect=dict(launches=[1, 0, 0])))
    # -- M, N edges: 1; one below / at / above a tile edge; a tile with one live row / column; M = 0, N = 0
    for M, N in ((1, 1), (63, 65), (64, 64), (65, 63), (129, 1), (1, 129)):
        for kind in ("nn", "nt"):
            un = kind == "nn" and N % 4 != 0
            T.append(_row("edge-%dx%d-%s" % (M, N, kind), "store_rows_tile: block cut by M / N at M = %d, N = %d" % (M, N), kind, N, 20,
                          _dense(M, 20), epi=EPI_BIAS if M % 2 else EPI_ACCUM_RELU_MASK, env=_plan(64, 64), ws="none",
                          expect=dict(family=0 if un else 1)))
    T.append(_row("M0", "launch_rows: M == 0 returns OK, nothing written", "nn", 8, 4, dict(batch=0, rpb=5, rs=4, bs=0), c=dict(batch=0, rpb=5, rs=8, bs=0),
                  ws="none", expect=dict(family=0, launches=[0, 0, 0])))
    T.append(_row("N0", "launch_rows: N == 0 returns OK, nothing written", "nt", 0, 4, _dense(5, 4), c=_dense(5, 4), ws="none",
                  expect=dict(family=0, launches=[0, 0, 0])))
    # -- epilogue forms of store_rows_tile: rpb 27 / 28 / 29 / 33, wrap = 0 and > 0, boundary at dr = 0 / 27 / absent, store-only and
    #    accumulating / masked forms at the same layouts, mask through C's pitched layout; register-staged and LDS-DMA kernels
    for rpb in (27, 28, 29, 33):
        for gap in (0, 12):
            for epi in (EPI_BIAS_RELU, EPI_ACCUM_RELU_MASK, EPI_RELU_MASK, EPI_ACCUM_RELU):
                for env, fam in ((NODMA, 0), ({}, 1)):
                    if fam == 1 and epi in (EPI_RELU_MASK, EPI_ACCUM_RELU) and gap == 0:
                        continue
                    T.append(_row("epi-rpb%d-gap%d-e%d-f%d" % (rpb, gap, epi, fam),
                                  "store_rows_tile: rpb %s 28 (%s), wrap %s 0" % (">=" if rpb >= 28 else "<", "INNER" if rpb >= 28 else "FAR / not inner",
                                                                                 ">" if gap else "="),
                                  "nt", 128, 32, _dense(5 * rpb, 32), c=_batched(5, rpb, 128, 4, gap), epi=epi,
                                  env=dict(_plan(128, 64), **env), ws="none", expect=dict(family=fam)))
    # store_rows_tile, INNER blocks: a lane owns rows rb0 + 4 h + dr, dr in {0..3, 8..11, 16..19, 24..27}; with the boundary o rows into
    # the block, wfrom = o - 4 h.  rpb = 36: o = 4, the half h = 1 starts on the first row of the next utterance (dr = 0) inside a block
    # that takes the select form; rpb = 59: o = 27, the last row a lane of h = 0 owns (dr = 27) is the first behind the boundary;
    # rpb = 32 / 64: every boundary on a block edge, none inside a block (NOWRAP)
    for rpb, what in ((36, "boundary at dr = 0 of the half h = 1, select form"), (32, "boundary on every block edge (NOWRAP)"),
                      (59, "boundary at dr = 27"), (64, "absent from every block")):
        for epi in (EPI_BIAS, EPI_ACCUM_RELU_MASK):
            T.append(_row("epi-bound-rpb%d-e%d" % (rpb, epi), "store_rows_tile: utterance %s" % what, "nt", 64, 16, _dense(4 * rpb, 16),
                          c=_batched(4, rpb, 64, 0, 8), epi=epi, env=_plan(64, 64), ws="none", expect=dict(family=1)))
    # -- conv-window A (overlapping causal windows), stride 1 / 2 / 3, nn forward with a batched C
    for s in (1, 2, 3):
        a = _conv(3, 40, 8, 3, s)
        T.append(_row("conv-s%d" % s, "row_offset: overlapping causal windows, k = 3, stride %d" % s, "nn", 72, 24, a,
                      c=_batched(3, a["rpb"], 72, 0, 0), epi=EPI_BIAS_RELU, env=_plan(64, 64), ws="none", expect=dict(family=1)))
    # -- the eight-wave LDS-DMA kernel (family 3): every epilogue, batched C with an utterance boundary inside a block
    for epi in range(8):
        T.append(_row("dma8-epi%d" % epi, "gemm_rows_dma8_kernel epilogue %d (store_rows_tile with waves 4 x 2)" % epi, "nt" if epi % 2 else "nn", 100,
                      48, _dense(3 * 45, 48), c=_batched(3, 45, 100, 0, 4), epi=epi, env=_plan(128, 64, 1, 8), ws="none",
                      expect=dict(family=3)))
    # -- the eight-wave register-staged kernel on a batched C (wrap, pitched mask), and split-K on both eight-wave kernels
    for epi in (EPI_BIAS_RELU, EPI_ACCUM_RELU_MASK):
        T.append(_row("rows8-batched-e%d" % epi, "gemm_rows8_kernel: store_rows_tile on a batched C, epilogue %d" % epi, "nt", 100, 48, _dense(3 * 45, 48),
                      c=_batched(3, 45, 100, 4, 4), epi=epi, env=dict(_plan(128, 64, 1, 8), **NODMA), ws="none",
                      expect=dict(family=0, kernel="gemm_rows8_kernel<128,64,nt,al>")))
    for env, fam, name in ((NODMA, 0, "reg"), ({}, 3, "dma")):
        T.append(_row("splitk-w8-" + name, "eight-wave tiles with K splits and rows_reduce_kernel (K = 148: 80 + 68)", "nn", 132, 148, _dense(130, 148),
                      epi=EPI_ACCUM_RELU, env=dict(_plan(128, 128, 2, 8), **env), ws="lib+plan", expect=dict(family=fam, launches=[1, 0, 1], splits=2)))
    # -- the planner's own choice (no PLAN): default path, small shapes
    T.append(_row("model-small", "choose_rows: the cost model's choice, no override", "nn", 257, 40, _dense(1000, 40), epi=EPI_BIAS, ws="lib",
                  expect={}))
    T.append(_row("model-dense-head", "choose_rows: small M, long K -> split-K by the model", "nt", 256, 1500, _dense(64, 1500), epi=EPI_RELU_MASK,
                  ws="lib", expect=dict(launches=[1, 0, 1])))
    # -- DmaStream: g = 0 (< 256 tiles; remainder 0), g by the model, forced 3, workspace one byte short, tail split, no_tail_split
    big = dict(a=_dense(64 * 33, 256), N=512)                       # 33 x 8 = 264 tiles of 64 x 64: remainder 8
    T.append(_row("stream-g-model", "dma_stream_plan: 264 tiles, remainder 8, g chosen by cost", "nt", big["N"], 256, big["a"], epi=EPI_ACCUM,
                  env=_plan(64, 64), ws="stream", expect=dict(family=1, launches=[1, 0, 0], g="model")))
    T.append(_row("stream-g3", "dma_stream_plan: LIDBOX_GEMM_STREAM_TAIL=3 forces g = 3", "nn", big["N"], 256, big["a"], epi=EPI_BIAS_RELU,
                  env=dict(_plan(64, 64), LIDBOX_GEMM_STREAM_TAIL="3"), ws="stream", expect=dict(family=1, g=3)))
    for epi in (EPI_BIAS, EPI_ACCUM_RELU_MASK, EPI_ACCUM_RELU, EPI_RELU):          # with the four above: all eight on the last arriver
        T.append(_row("stream-epi%d" % epi, "DmaStream last arriver: epilogue %d, batched C" % epi, "nt" if epi % 2 else "nn", big["N"], 256, big["a"],
                      c=_batched(33, 64, big["N"], 0, 8), epi=epi, env=dict(_plan(64, 64), LIDBOX_GEMM_STREAM_TAIL="3"), ws="stream",
                      expect=dict(family=1, g=3)))
    T.append(_row("stream-g8", "dma_stream_plan: K = 1024 -> g = 8", "nt", 512, 1024, _dense(64 * 33, 1024), epi=EPI_RELU_MASK,
                  env=_plan(64, 64), ws="stream", expect=dict(family=1, g=8)))
    T.append(_row("stream-g2", "dma_stream_plan: remainder 128 of 384 tiles -> g = 2", "nt", 512, 256, _dense(64 * 48, 256), epi=EPI_NONE,
                  env=_plan(64, 64), ws="stream", expect=dict(family=1, g=2)))
    T.append(_row("stream-ws-short", "launch_rows: wsb < spl.ws_need by one byte -> falls through to the plain launch", "nt", big["N"], 256, big["a"],
                  epi=EPI_ACCUM, env=_plan(64, 64), ws="stream-1", expect=dict(family=1, g=0)))
    T.append(_row("stream-off", "LIDBOX_GEMM_STREAM_TAIL=0 -> g = 0, the plain launch (the tail split declines)", "nt", big["N"], 256, big["a"], epi=EPI_BIAS,
                  env=dict(_plan(64, 64), LIDBOX_GEMM_STREAM_TAIL="0"), ws="lib", expect=dict(family=1, g=0)))
    T.append(_row("tail-split", "launch_rows: tail split, the remainder (one row) planned on its own and split along K: {1, 1, 1}; "
                  "the smallest such shape under the restated planner", "nt", 4, 1280, _dense(256 * 128 + 1, 1280), epi=EPI_BIAS,
                  env=dict(_plan(128, 128), LIDBOX_GEMM_STREAM_TAIL="0"), ws="64M", expect=dict(family=1, g=0, launches=[1, 1, 1])))
    T.append(_row("tail-split-unsplit", "launch_rows: tail split, the remainder (217 rows of N = 4) planned on its own and unsplit without a "
                  "workspace: {1, 1, 0}; the smallest M K for which the restated planner takes it", "nt", 4, 16, _dense(126081, 16), epi=EPI_ACCUM,
                  env=dict(_plan(128, 128), LIDBOX_GEMM_STREAM_TAIL="0"), ws="none", expect=dict(family=1, g=0, launches=[1, 1, 0])))
    T.append(_row("stream-rem0", "dma_stream_plan: 256 tiles, remainder 0 -> g = 0", "nt", 512, 64, _dense(64 * 32, 64), env=_plan(64, 64),
                  ws="lib", expect=dict(family=1, g=0, launches=[1, 0, 0])))
    T.append(_row("no-tail-split", "launch_rows: LIDBOX_GEMM_NO_TAIL_SPLIT keeps one launch", "nt", big["N"], 256, big["a"], epi=EPI_BIAS,
                  env=dict(_plan(64, 64), LIDBOX_GEMM_STREAM_TAIL="0", LIDBOX_GEMM_NO_TAIL_SPLIT="1"), ws="lib",
                  expect=dict(family=1, g=0, launches=[1, 0, 0])))
    # -- stream-K: every epilogue on the plain and the pipelined kernel; schedule branches; refusals
    for epi in range(8):
        kind = "nt" if epi in (3, 4, 5, 6) else "nn"
        T.append(_row("sk-epi%d" % epi, "gemm_sk_rows_kernel last arriver: epilogue %d, equal spans with T < P" % epi, kind, 200, 520,
                      _dense(250, 520), c=_batched(5, 50, 200, 0, 8), epi=epi, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16"), ws="lib",
                      expect=dict(family=2, launches=[1, 0, 0], branch="spans_T<P")))
        T.append(_row("skp-epi%d" % epi, "gemm_skp_rows_kernel in-loop drain: epilogue %d" % epi, kind, 200, 520, _dense(250, 520),
                      c=_batched(5, 50, 200, 0, 8), epi=epi, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib",
                      expect=dict(family=2, launches=[1, 0, 0], skp=True)))
    T.append(_row("skp-nt-nomask-noacc", "gemm_skp_rows_kernel<nt, nomask, noacc>", "nt", 200, 512, _dense(250, 512), epi=EPI_RELU,
                  env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib", expect=dict(family=2, skp=True)))
    T.append(_row("skp-nn-mask", "gemm_skp_rows_kernel<nn, mask, noacc>", "nn", 200, 512, _dense(250, 512), epi=EPI_RELU_MASK,
                  env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib", expect=dict(family=2, skp=True)))
    T.append(_row("skp-nn-mask-acc", "gemm_skp_rows_kernel<nn, mask, acc>", "nn", 200, 512, _dense(250, 512), epi=EPI_ACCUM_RELU_MASK,
                  env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib", expect=dict(family=2, skp=True)))
    T.append(_row("skp-nn-acc", "gemm_skp_rows_kernel<nn, nomask, acc>", "nn", 200, 512, _dense(250, 512), epi=EPI_ACCUM,
                  env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib", expect=dict(family=2, skp=True)))
    T.append(_row("skp-rpb31", "launch_rows: skp_ok false at rows_per_batch < 32 -> the plain stream-K kernel", "nn", 200, 512, _dense(248, 512),
                  c=_batched(8, 31, 200, 0, 8), epi=EPI_BIAS, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib",
                  expect=dict(family=2, skp=False)))
    for name, why, kw in (("Cbase", "aligned16(Cd.base) false", dict(mis={"C": 1})), ("auxbase", "aligned16(aux) false with a mask", dict(mis={"aux": 1})),
                          ("N%4", "N % 4 != 0 (nt)", dict(N=202))):
        T.append(_row("skp-refuse-" + name, "launch_rows: skp_ok false by %s -> the plain stream-K kernel" % why, "nt", kw.get("N", 200), 512,
                      _dense(250, 512), epi=EPI_ACCUM_RELU_MASK, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16", LIDBOX_GEMM_SKP="2"), ws="lib",
                      mis=kw.get("mis"), expect=dict(family=2, skp=False)))
    # -- LIDBOX_GEMM_NN8 / _NT8 (M >= 4096): the eight-wave tiles without a PLAN
    T.append(_row("nt8-64", "choose_rows_env: LIDBOX_GEMM_NT8=64 at M = 4096 -> gemm_rows_dma8_kernel<64,nt>", "nt", 68, 20, _dense(4096, 20), epi=EPI_ACCUM,
                  env={"LIDBOX_GEMM_NT8": "64"}, ws="none", expect=dict(family=3, kernel="gemm_rows_dma8_kernel<64,nt>")))
    T.append(_row("nn8-128-reg", "choose_rows_env: LIDBOX_GEMM_NN8=128 with LIDBOX_GEMM_DMA=0 -> gemm_rows8_kernel<128,128,nn,al>", "nn", 132, 20,
                  _dense(4096, 20), epi=EPI_BIAS_RELU, env={"LIDBOX_GEMM_NN8": "128", "LIDBOX_GEMM_DMA": "0"}, ws="none",
                  expect=dict(family=0, kernel="gemm_rows8_kernel<128,128,nn,al>")))
    T.append(_row("nt8-below", "choose_rows_env: LIDBOX_GEMM_NT8 ignored at M = 4095", "nt", 68, 20, _dense(4095, 20), env={"LIDBOX_GEMM_NT8": "64"},
                  ws="none", expect=dict(family=1)))
    T.append(_row("sk-whole", "sk_rows_plan: whole rounds only (16 tiles on 16 workgroups)", "nn", 512, 64, _dense(512, 64), epi=EPI_BIAS,
                  env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16"), ws="lib", expect=dict(family=2, branch="whole")))
    T.append(_row("sk-dp-fallback", "sk_rows_plan: cu_parts > cu_spans -> --dp_rounds, equal spans over T > P tiles", "nt", 512, 256,
                  _dense(640, 256), epi=EPI_ACCUM, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16"), ws="lib", expect=dict(family=2, branch="dp_fallback")))
    T.append(_row("sk-parts", "sk_rows_plan: a remainder cut into parts (496 tiles on 256 workgroups)", "nn", 2048, 64, _dense(3968, 64),
                  epi=EPI_BIAS_RELU, env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="256"), ws="lib", expect=dict(family=2, branch="parts")))
    # a tuned shape: sk_tuned_out keeps it on its measured classic decomposition unless LIDBOX_GEMM_NO_TUNED (or SK_ALL) is set; the
    # pipelined kernel is the stream-K kernel that needs no SK_ALL (LIDBOX_GEMM_SKP=2)
    TUNED_ENV = {"LIDBOX_GEMM_SK_MIN_FLOP": "0", "LIDBOX_GEMM_SK_GRID": "16", "LIDBOX_GEMM_SKP": "2"}
    for kind, M, N, K in (("nn", 512, 4, 512), ("nt", 1024, 512, 512)):
        T.append(_row("sk-refuse-tuned-%s" % kind, "launch_rows: sk_tuned_out true for a shape of gemm_tuned.h -> its tuned decomposition", kind, N, K,
                      _dense(M, K), epi=EPI_BIAS_RELU if kind == "nn" else EPI_ACCUM, env=TUNED_ENV, ws="lib", expect=dict(family=1, launches=[1, 0, 1])))
        T.append(_row("sk-no-tuned-%s" % kind, "launch_rows: LIDBOX_GEMM_NO_TUNED lifts sk_tuned_out -> stream-K", kind, N, K, _dense(M, K),
                      epi=EPI_BIAS_RELU if kind == "nn" else EPI_ACCUM, env=dict(TUNED_ENV, LIDBOX_GEMM_NO_TUNED="1"), ws="lib",
                      expect=dict(family=2, launches=[1, 0, 0], skp=True)))
    ref = dict(kind="nn", N=200, K=512, a=_dense(250, 512), epi=EPI_BIAS, ws="lib")
    for name, why, ch in (("M<128", "sk_rows_plan: M < SK_BM", dict(a=_dense(127, 512))),
                          ("K%4", "sk_rows_plan: K % 4 != 0", dict(K=510, a=_dense(250, 510))),
                          ("span", "sk_rows_plan: spans shorter than SK_MIN_SPAN", dict(K=64, a=_dense(250, 64))),
                          ("ws-short", "launch_rows: wsb < sk.ws_need by one byte", dict(ws="lib-1")),
                          ("ws-misaligned", "launch_rows: aligned16(ws) false", dict(ws="lib-mis"))):
        rr = dict(ref, **ch)
        T.append(_row("sk-refuse-" + name, why, rr["kind"], rr["N"], rr["K"], rr["a"], epi=rr["epi"], env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16"),
                      ws=rr["ws"], expect=dict(family_not=2)))
    return T


def _tn_row(name, why, K1, N, a, b=None, env=None, accumulate=0, bias_grad=True, ldc_pad=0, mis=None, ws="lib", expect=None):
    M = a["batch"] * a["rpb"]
    b = _dense(M, N) if b is None else b
    return dict(name=name, why=why, kind="tn", M=M, K1=K1, N=N, a=a, b=b, env=dict(env or {}), accumulate=accumulate, bias_grad=bias_grad,
                ldc_pad=ldc_pad, mis=dict(mis or {}), ws=ws, expect=dict(expect or {}))


def _tn_table():
    T = []
    NODMA = {"LIDBOX_GEMM_DMA": "0"}
    i = 0
    for bm, bn in CAND:
        pl = {"LIDBOX_GEMM_TN_PLAN": "%d,%d,3" % (bm, bn)}
        T.append(_tn_row("tn-al-%dx%d" % (bm, bn), "launch_tn_t: LIDBOX_GEMM_DMA=0, al -> gemm_tn_kernel<%d,%d,al>; ragged last slice" % (bm, bn),
                         bm + 4, bn + 4, _dense(100, bm + 4, 4), b=_dense(100, bn + 4, 4), env=dict(pl, **NODMA), accumulate=i % 2, bias_grad=True,
                         ldc_pad=4, expect=dict(family=0, kernel="gemm_tn_kernel<%d,%d,al>" % (bm, bn))))
        T.append(_tn_row("tn-dma-%dx%d" % (bm, bn), "tn_partial_launch: al && dma -> gemm_tn_dma_kernel<%d,%d>" % (bm, bn), bm + 4, bn + 4,
                         _dense(100, bm + 4, 4), b=_dense(100, bn + 4, 4), env=pl, accumulate=(i + 1) % 2, bias_grad=bool(i % 2), ldc_pad=4,
                         expect=dict(family=1, kernel="gemm_tn_dma_kernel<%d,%d>" % (bm, bn))))
        un = [dict(mis={"A": 1}), dict(mis={"B": 1}), dict(dK=1), dict(dN=1)][i]
        T.append(_tn_row("tn-un-%dx%d" % (bm, bn), "tn_partial_launch: al false -> gemm_tn_kernel<%d,%d,un>, scalar reduce" % (bm, bn),
                         bm + 4 + un.get("dK", 0), bn + 4 + un.get("dN", 0), _dense(100, bm + 4 + un.get("dK", 0)), env=pl, accumulate=i % 2,
                         mis=un.get("mis"), expect=dict(family=0, kernel="gemm_tn_kernel<%d,%d,un>" % (bm, bn))))
        i += 1
    one = {"LIDBOX_GEMM_TN_PLAN": "64,64,1"}
    T.append(_tn_row("tn-one-slice", "tn_plan: one slice", 64, 64, _dense(50, 64), env=one, bias_grad=False, expect=dict(splits=1)))
    T.append(_tn_row("tn-M1", "gemm_tn kernels: M = 1, a lone tail step", 8, 8, _dense(1, 8), env=one, expect=dict(splits=1)))
    T.append(_tn_row("tn-ldc-odd", "reduce_job_vec_ok: ldc % 4 != 0 -> splitk_reduce_kernel behind the DMA kernel", 64, 64, _dense(100, 64),
                     env={"LIDBOX_GEMM_TN_PLAN": "64,64,2"}, ldc_pad=3, expect=dict(family=1, reduce="splitk_reduce_kernel")))
    T.append(_tn_row("tn-c-misaligned", "reduce_job_vec_ok: aligned16(Cm) false", 64, 64, _dense(100, 64), env={"LIDBOX_GEMM_TN_PLAN": "64,64,2"},
                     mis={"C": 1}, accumulate=1, expect=dict(family=1, reduce="splitk_reduce_kernel")))
    T.append(_tn_row("tn-bg-misaligned", "reduce_job_vec_ok: aligned16(bias_grad) false", 64, 64, _dense(100, 64),
                     env={"LIDBOX_GEMM_TN_PLAN": "64,64,2"}, mis={"bg": 1}, expect=dict(family=1, reduce="splitk_reduce_kernel")))
    T.append(_tn_row("tn-model", "tn_plan: the cost model's choice", 40, 257, _dense(1000, 40), b=_dense(1000, 257), accumulate=1, expect={}))
    for s in (1, 2, 3):
        a = _conv(4, 50, 16, 3, s)
        T.append(_tn_row("tn-conv-s%d" % s, "gemm_tn kernels: conv-window A, stride %d (utterance wrap inside the contraction)" % s, 48, 64, a,
                         env={"LIDBOX_GEMM_TN_PLAN": "64,64,3"}, expect=dict(family=1)))
        T.append(_tn_row("tn-conv-s%d-reg" % s, "gemm_tn_kernel: conv-window A, stride %d" % s, 48, 64, a,
                         env={"LIDBOX_GEMM_TN_PLAN": "64,64,3", "LIDBOX_GEMM_DMA": "0"}, expect=dict(family=0)))
    T.append(_tn_row("tn-sk", "sk_tn_plan ok -> gemm_sk_tn_kernel, ragged last slice", 128, 128, _dense(1000, 128), env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="4"),
                     accumulate=1, expect=dict(family=2, kernel="gemm_sk_tn_kernel")))
    T.append(_tn_row("tn-sk-cap", "sk_tn_plan: the 8192-row slice cap reached through a grid of 1", 4, 4, _dense(8192 + 200, 4),
                     env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="1"), expect=dict(family=2, rps=8192, splits=2)))
    T.append(_tn_row("tn-sk-short", "sk_tn_plan: slices shorter than 128 rows -> classic", 128, 128, _dense(100, 128), env=dict(SK_ENV, LIDBOX_GEMM_SK_GRID="4"),
                     expect=dict(family=1)))
    return T


def _colsum_table():
    T = []
    for name, why, a, N, acc, mis in (
            ("cs-1", "colsum_stage1: one row, one column", _dense(1, 1), 1, 0, 0),
            ("cs-ragged", "colsum_stage1: N = 65 (two column blocks), 3 ragged slices", _dense(700, 65, 3), 65, 1, 0),
            ("cs-cap", "lidbox_colsum: slices capped at 128", _dense(128 * 256 + 300, 8), 8, 0, 1),
            ("cs-batched", "colsum_stage1: batched rows with a gap", _batched(7, 37, 20, 4, 8), 20, 1, 0),
            ("cs-257", "colsum_stage2: N = 257, two blocks", _dense(300, 257), 257, 0, 0)):
        T.append(dict(name=name, why=why, kind="colsum", a=a, M=a["batch"] * a["rpb"], N=N, accumulate=acc, mis={"A": mis}))
    return T


def _pair_table():
    T = []
    for name, why, M, Co, N, K1, env, pair in (
            ("pair", "pair_plan true -> gemm_nt_tn_pair_kernel (one launch)", 64, 64, 128, 64, {}, True),
            ("pair-splitk", "pair with a split-K dgrad (partial = 1) and rows_reduce_kernel", 64, 512, 64, 64, _plan(64, 64, 2), True),
            ("pair-off", "LIDBOX_GEMM_NO_PAIR -> the two calls", 64, 64, 128, 64, {"LIDBOX_GEMM_NO_PAIR": "1"}, False),
            ("pair-Co%4", "pair_plan: Co % 4 != 0 -> the two calls", 64, 66, 128, 64, {}, False),
            ("pair-shared-ws", "lidbox_gemm_nt_tn_carry: ws_nt == ws_tn -> wgrad, its reduce, then the dgrad", 64, 64, 128, 64, {}, False)):
        T.append(dict(name=name, why=why, kind="pair", M=M, Co=Co, N=N, K1=K1, env=dict(env), pair=pair, shared=name == "pair-shared-ws"))
    return T


def _carry_table():
    """lidbox_gemm_tn_partial -> lidbox_gemm_nt_carry: `jobs` pending jobs (w: a wgrad's slice sum, z: a zero job) handed to a
    dgrad launch; carried: what lidbox_gemm_last_carried must say; rc_ok False: the call is refused and nothing runs"""
    T = []
    for name, why, jobs, env, carried, rc_ok in (
            ("carry-1-dma", "launch_rows_range: one pending job in the leading workgroups of an LDS-DMA launch", "w", {}, 1, True),
            ("carry-2-dma", "pack_carry: two pending jobs (a wgrad reduce and a zero job) share the leading workgroups", "wz", {}, 2, True),
            ("carry-zero", "lidbox_zero_job carried alone", "z", {}, 1, True),
            ("carry-3-refused", "jobs_in: a third non-empty job is refused", "wzz", {}, 0, False),
            ("carry-non-dma", "lidbox_gemm_nt_carry: LIDBOX_GEMM_DMA=0, the jobs run as a launch behind the GEMM", "wz", {"LIDBOX_GEMM_DMA": "0"}, 0, True),
            ("carry-off", "LIDBOX_GEMM_NO_CARRY: the jobs run as a launch of their own", "w", {"LIDBOX_GEMM_NO_CARRY": "1"}, 0, True)):
        T.append(dict(name=name, why=why, kind="carry", jobs=jobs, env=dict(env), carried=carried, rc_ok=rc_ok, M=192, Co=64, N=96, K1=40, Mw=100))
    return T


PATHS = dict(ROWS=_rows_table(), TN=_tn_table(), COLSUM=_colsum_table(), PAIR=_pair_table(), CARRY=_carry_table())


# ------------------------------------------------------------------------------------------------ rows -> calls
def ldb_of(r):
    return (r["N"] if r["kind"] == "nn" else r["K"]) + r["ldb_pad"]


def row_al(r):
    a = r["a"]
    return rows_al(4 * r["mis"].get("A", 0), a["rs"], a["batch"], a["bs"], r["K"], 4 * r["mis"].get("B", 0), ldb_of(r), r["N"], KIND[r["kind"]])


def row_ws_bytes(r):
    """(bytes, aligned): the workspace the row's call gets.  'lib': lidbox_gemm_rows_workspace; 'lib+plan': room for the PLAN's
    split as well; 'stream': the streamed remainder's need for the PLAN's tile; '-1': one byte short; '-mis': 4 bytes off"""
    env, ws = r["env"], r["ws"]
    M, N, K = r["M"], r["N"], r["K"]
    if ws == "none" or M == 0 or N == 0:
        return 0, True
    if ws == "64M":
        return 64 << 20, True
    base = ws.split("-")[0]
    need = rows_workspace(M, N, K, env)
    if base in ("lib+plan", "plan"):
        sp = int(env["LIDBOX_GEMM_PLAN"].split(",")[2])
        kps = cdiv(cdiv(K, sp), BK) * BK
        need = max(need if base == "lib+plan" else 0, cdiv(K, kps) * M * N * 4)
    if base == "stream":
        bm, bn = (int(x) for x in env["LIDBOX_GEMM_PLAN"].split(",")[:2])
        need = dma_stream_plan(bm, bn, M, N, K, {k: v for k, v in env.items() if k != "LIDBOX_GEMM_STREAM_TAIL" or v != "0"})["ws_need"]
    if ws.endswith("-1"):
        need -= 1
    return need, not ws.endswith("-mis")


def row_predict(r):
    wsb, ws_al = row_ws_bytes(r)
    c = r["c"]
    return rows_dispatch(KIND[r["kind"]], r["M"], r["N"], r["K"], row_al(r), wsb, r["env"], r["epi"], ws_al, c["batch"], c["rpb"], c["rs"],
                         c["bs"], 4 * r["mis"].get("C", 0), 4 * r["mis"].get("aux", 0))


def tn_row_predict(r):
    a, b = r["a"], r["b"]
    a_al = r["mis"].get("A", 0) == 0 and a["rs"] % 4 == 0 and (a["batch"] == 1 or a["bs"] % 4 == 0)
    b_al = r["mis"].get("B", 0) == 0 and b["rs"] % 4 == 0 and (b["batch"] == 1 or b["bs"] % 4 == 0)
    wsb = tn_workspace(r["M"], r["K1"], r["N"], r["env"])
    return tn_dispatch(r["M"], r["K1"], r["N"], a_al, b_al, wsb, r["env"], 0, 4 * r["mis"].get("C", 0), r["N"] + r["ldc_pad"], r["bias_grad"],
                       4 * r["mis"].get("bg", 0))


def make_rows_data(r, ds, seed=0):
    """the inputs of one ROWS row as flat float32 buffers (NaN in every gap) and their dense views"""
    rng = np.random.default_rng([seed, DATASETS.index(ds), sum(map(ord, r["name"]))])
    M, N, K, kind, epi = r["M"], r["N"], r["K"], r["kind"], r["epi"]
    a_flat = fill_flat(rng, ds, r["a"], K)
    ldb = ldb_of(r)
    brows, bcols = (K, N) if kind == "nn" else (N, K)
    b_flat = np.full(max(1, brows * ldb), np.nan, np.float32)
    Bv = b_flat[:brows * ldb].reshape(brows, ldb)
    Bv[:, :bcols] = draw(rng, ds, (brows, bcols))
    next_ = extent(r["c"], N) if M and N else 1
    c_flat = np.full(next_, np.nan, np.float32)
    old = None
    if epi in EPI_ACCUMS and M and N:
        old = draw(rng, ds, (M, N), "int" if ds == "exact" else "ab")
        c_flat[index(r["c"], N)] = old
    bias = draw(rng, ds, N, "int" if ds == "exact" else "ab") if epi in EPI_HAS_BIAS else None
    mask_flat = fill_flat(rng, ds, r["c"], N, "mask") if (epi in EPI_HAS_MASK and M and N) else None
    A = gather(a_flat, r["a"], K) if M else np.zeros((0, K), np.float32)
    B = Bv[:, :bcols].copy()
    mask = mask_flat[index(r["c"], N)] if mask_flat is not None else None
    return dict(a_flat=a_flat, b_flat=b_flat, c_flat=c_flat, bias=bias, mask_flat=mask_flat, A=A, B=B, old=old, mask=mask)


def make_tn_data(r, ds, seed=0):
    rng = np.random.default_rng([seed, DATASETS.index(ds), sum(map(ord, r["name"]))])
    K1, N = r["K1"], r["N"]
    ldc = N + r["ldc_pad"]
    a_flat = fill_flat(rng, ds, r["a"], K1)
    b_flat = fill_flat(rng, ds, r["b"], N)
    c_flat = np.full((K1, ldc), np.nan, np.float32)
    old_bg = None
    if r["accumulate"]:
        c_flat[:, :N] = draw(rng, ds, (K1, N), "int" if ds == "exact" else "ab")
    if r["bias_grad"]:
        old_bg = draw(rng, ds, N, "int" if ds == "exact" else "ab") if r["accumulate"] else np.full(N, np.nan, np.float32)
    return dict(a_flat=a_flat, b_flat=b_flat, c_flat=c_flat, old_bg=old_bg, A=gather(a_flat, r["a"], K1), B=gather(b_flat, r["b"], N))


def tn_reference(r, dat):
    """(dW ref, S, bias grad ref, S) in float64"""
    N = r["N"]
    v, S = product("tn", dat["A"], dat["B"]), product("tn", np.abs(dat["A"]), np.abs(dat["B"]))
    g, Sg = np.asarray(dat["B"], np.float64).sum(0), np.abs(np.asarray(dat["B"], np.float64)).sum(0)
    if r["accumulate"]:
        old = np.asarray(dat["c_flat"][:, :N], np.float64)
        v, S = v + old, S + np.abs(old)
        if r["bias_grad"]:
            ob = np.asarray(dat["old_bg"], np.float64)
            g, Sg = g + ob, Sg + np.abs(ob)
    return v, S, g, Sg


# ------------------------------------------------------------------------------------------------ judging
NAN_BITS = 0x7FC00000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def judge_rows(r, ds, dat, got_flat, p):
    """(inside, worst err / bound, what) for the flat C buffer after a call: covered elements within the bound (`exact`: equal
    to the int64 result bit for bit), every gap word still the NaN it started as"""
    M, N = r["M"], r["N"]
    got_flat = np.asarray(got_flat, np.float32)
    if got_flat.size != dat["c_flat"].size:
        return False, np.inf, "wrote past C's extent"
    if M == 0 or N == 0:
        return bool(np.array_equal(_bits(got_flat), _bits(dat["c_flat"]))), 0.0, "fill"
    idx = index(r["c"], N)
    cover = np.zeros(got_flat.size, bool)
    cover[idx.ravel()] = True
    if not (_bits(got_flat)[~cover] == NAN_BITS).all():
        return False, np.inf, "a gap word of C was written"
    ref, S = rows_reference(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask"], dat["old"])
    got = got_flat[idx]
    if ds == "exact":
        same = np.array_equal(_bits(got), _bits(ref.astype(np.float32)))
        return same, 0.0 if same else np.inf, "bits"
    q = ratio(got, ref, S, chain_n(r["K"], p, r["epi"]))
    return bool((q <= 1.0).all()), float(q.max()), "bound"


def judge_tn(r, ds, dat, got_c, got_bg, splits, rps):
    """(inside, worst dW, worst bias grad): dW [K1, ldc] with NaN still behind column N"""
    N = r["N"]
    got_c = np.asarray(got_c, np.float32).reshape(r["K1"], N + r["ldc_pad"])
    if not (_bits(got_c[:, N:]) == NAN_BITS).all():
        return False, np.inf, 0.0
    v, S, g, Sg = tn_reference(r, dat)
    if ds == "exact":
        ok = np.array_equal(_bits(got_c[:, :N]), _bits(v.astype(np.float32)))
        okg = (not r["bias_grad"]) or np.array_equal(_bits(got_bg), _bits(g.astype(np.float32)))
        return ok and okg, 0.0 if ok else np.inf, 0.0 if okg else np.inf
    n = 2 * min(rps, r["M"]) + splits + 1 + r["accumulate"]
    q = ratio(got_c[:, :N], v, S, n)
    qg = ratio(got_bg, g, Sg, bias_grad_n(min(rps, r["M"]), splits)) if r["bias_grad"] else np.zeros(1)
    return bool((q <= 1.0).all() and (qg <= 1.0).all()), float(q.max()), float(qg.max())


# ------------------------------------------------------------------------------------------------ launch sites of the source
def instantiations_from_source():
    """the kernel instantiations that the launch sites of gemm.hip and gemm_shared.h name, enumerated from the source text: every
    hipLaunchKernelGGL site with its template arguments, the symbols among them replaced by the literal arguments of the macro
    invocations (LBX_ROWS(128, 64), LBX_SKP(true, false), ...) that reach the site -- directly for a site inside a macro, through
    the launch_*_t wrapper for a site inside one -- and B_KINNER by both values when launch_rows<true> and <false> are both
    instantiated.  Names come out in the spelling of instantiations()."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lidbox_amd", "csrc")
    src = ""
    for f in ("gemm.hip", "gemm_shared.h"):
        with open(os.path.join(here, f)) as fh:
            src += fh.read().replace("\\\n", " ") + "\n"
    lines = src.split("\n")
    macros = {}                                                     # name -> (params, body)
    for ln in lines:
        m = re.match(r"\s*#define\s+(LBX_\w+)\(([^)]*)\)\s+(.*)", ln)
        if m:
            macros[m.group(1)] = ([p.strip() for p in m.group(2).split(",")], m.group(3))
    plain = "\n".join(ln for ln in lines if not re.match(r"\s*#\s*(define|undef)", ln))

    def invocations(name):
        return sorted({tuple(a.strip() for a in m.group(1).split(",")) for m in re.finditer(r"\b%s\(([^()]*)\)" % name, plain)})

    kinner = ["false", "true"] if ("launch_rows<true>" in plain and "launch_rows<false>" in plain) else ["B_KINNER"]
    site = re.compile(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)\s*(?:<([^>]*)>)?")
    found = set()

    def emit(kernel, targs, binds):
        for b in binds:
            vals = [[b.get(t, t)] for t in targs]
            vals = [kinner if v == ["B_KINNER"] else v for v in vals]
            combos = [[]]
            for v in vals:
                combos = [c + [x] for c in combos for x in v]
            for c in combos:
                found.add((kernel, tuple(c)))

    # sites inside a macro body
    for name, (params, body) in macros.items():
        for m in site.finditer(body):
            targs = [t.strip() for t in m.group(2).split(",")] if m.group(2) else []
            emit(m.group(1), targs, [dict(zip(params, inv)) for inv in invocations(name)])
    # sites in plain code: inside a launch_*_t wrapper (bound through the macros that call it) or direct
    wrappers = [(m.start(), m.group(2), [p.split()[-1] for p in m.group(1).split(",")])
                for m in re.finditer(r"template <([^>]*)>\s*void (launch_\w+_t)\(", plain)]
    for m in site.finditer(plain):
        targs = [t.strip() for t in m.group(2).split(",")] if m.group(2) else []
        inside = None
        for pos, wname, tparams in wrappers:
            if pos < m.start() and "\n}" not in plain[pos:m.start()]:
                inside = (wname, tparams)
        if inside is None:
            emit(m.group(1), targs, [{}])
            continue
        wname, tparams = inside
        binds = []
        for name, (params, body) in macros.items():
            c = re.search(r"\b%s<([^>]*)>" % wname, body)
            if c:
                actual = [a.strip() for a in c.group(1).split(",")]
                for inv in invocations(name):
                    mp = dict(zip(params, inv))
                    binds.append({tp: mp.get(a, a) for tp, a in zip(tparams, actual)})
        emit(m.group(1), targs, binds)

    def spell(kernel, args):
        a = list(args)
        if kernel in ("gemm_rows_kernel", "gemm_rows8_kernel"):
            return "%s<%s,%s,%s,%s>" % (kernel, a[0], a[1], "nt" if a[2] == "true" else "nn", "al" if a[3] == "true" else "un")
        if kernel == "gemm_tn_kernel":
            return "%s<%s,%s,%s>" % (kernel, a[0], a[1], "al" if a[2] == "true" else "un")
        if kernel == "gemm_rows_dma_kernel":
            return "%s<%s,%s,%s>" % (kernel, a[0], a[1], "nt" if a[2] == "true" else "nn")
        if kernel == "gemm_rows_dma8_kernel":
            return "%s<%s,%s>" % (kernel, a[0], "nt" if a[1] == "true" else "nn")
        if kernel == "gemm_tn_dma_kernel":
            return "%s<%s,%s>" % (kernel, a[0], a[1])
        if kernel == "gemm_sk_rows_kernel":
            return "%s<%s>" % (kernel, "nt" if a[0] == "true" else "nn")
        if kernel == "gemm_skp_rows_kernel":
            return "%s<%s,%s,%s>" % (kernel, "nt" if a[0] == "true" else "nn", "mask" if a[1] == "true" else "nomask", "acc" if a[2] == "true" else "noacc")
        assert not a, (kernel, a)
        return kernel
    return sorted(spell(k, a) for k, a in found)


# ------------------------------------------------------------------------------------------------ 7. the 32-bit extent guards
# The LDS-DMA kernels address an operand with one 64-bit base and a 32-bit byte offset per lane; the host lets them run while
# the guard's expression g stays below its limit L (bytes, 4.0e9: above 2^31, so offsets with bit 31 set are legal).  The limits
# are READ from the source text, like the tuned table.  FAR rows put an operand across a limit by stretching one stride, so a
# case stays at a few MFLOP while its last row lies 4 GB behind the base.
_LIMITS = None
ZONES = ("high", "edge-in", "edge-out", "over")
HIGH_BYTES = 3.9e9                                                  # `high`: the largest byte offset dereferenced is at least this
OVER = 1.05


def limits():
    """the numeric limits of the guards, from csrc/gemm.hip and csrc/gemm_shared.h"""
    global _LIMITS
    if _LIMITS is None:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lidbox_amd", "csrc")
        with open(os.path.join(here, "gemm.hip")) as f:
            src = f.read()
        with open(os.path.join(here, "gemm_shared.h")) as f:
            sh = f.read()
        a = re.search(r"inline bool sk_extent_ok\(.*?\+ cols \+ (\d+);\s*return last \* 4\.0 < ([0-9.e]+);", src, re.S)
        b = re.search(r"inline bool sk_b_extent_ok\(.*?\+ ([0-9.]+)\) \* \(double\)ldb \* 4\.0 < ([0-9.e]+);", src, re.S)
        j = re.search(r"inline bool reduce_job_vec_ok\(.*?\(double\)splits \* \(double\)n \* 4\.0 < ([0-9.e]+);", sh, re.S)
        inner = re.findall(r"const bool inner = .*?\(unsigned\)Cd\.rpb >= (\d+)\) &&\s*out_rs > 0 && out_rs < \(1L << (\d+)\) && wrap_u >= 0 && "
                           r"wrap_u < \(1L << (\d+)\);", sh, re.S)
        assert a and b and j and inner, "a guard of gemm.hip / gemm_shared.h no longer reads as restated here"
        assert len(set(inner)) == 1, inner
        _LIMITS = dict(a_pad=int(a.group(1)), a_bytes=float(a.group(2)), b_pad=float(b.group(1)), b_bytes=float(b.group(2)),
                       job_bytes=float(j.group(1)), inner_rpb=int(inner[0][0]), inner_rs=1 << int(inner[0][1]), inner_wrap=1 << int(inner[0][2]))
    return _LIMITS


def a_guard(d, cols):
    """g of sk_extent_ok, in bytes"""
    last = float(max(d["batch"] - 1, 0)) * d["bs"] + float(max(d["rpb"] - 1, 0)) * d["rs"] + cols + limits()["a_pad"]
    return last * 4.0


def sk_extent_ok(d, cols):
    return a_guard(d, cols) < limits()["a_bytes"]


def b_guard(kind, K, N, ldb):
    """g of sk_b_extent_ok, in bytes; kind 1 (nt): B[N][ldb], kind 0 (nn): B[K][ldb]"""
    return (float(N if kind == 1 else K) + limits()["b_pad"]) * float(ldb) * 4.0


def sk_b_extent_ok(kind, K, N, ldb):
    return b_guard(kind, K, N, ldb) < limits()["b_bytes"]


def job_guard(splits, n):
    return float(splits) * float(n) * 4.0


def store_inner_ok(c, partial=False):
    """the descriptor terms of `inner` in store_rows_tile (the per-block terms -- all 32 rows inside M, all columns inside N -- aside)"""
    L = limits()
    batched = not partial and c["batch"] != 1
    wrap = c["bs"] - c["rpb"] * c["rs"] if batched else 0
    return (not batched or c["rpb"] >= L["inner_rpb"]) and 0 < c["rs"] < L["inner_rs"] and 0 <= wrap < L["inner_wrap"]


def pair_al(dy, Co, N, ldb, x, K1, res=None):
    """(al_rows, al_tn) of lidbox_gemm_nt_tn"""
    res = res or {}
    al = lambda d, r: r == 0 and d["rs"] % 4 == 0 and (d["batch"] == 1 or d["bs"] % 4 == 0)
    al_rows = (al(dy, res.get("dY", 0)) and res.get("W", 0) == 0 and ldb % 4 == 0 and sk_extent_ok(dy, Co) and sk_b_extent_ok(1, Co, N, ldb) and
               res.get("ws_nt", 0) == 0)
    return al_rows, al(x, res.get("X", 0)) and sk_extent_ok(x, K1) and res.get("ws_tn", 0) == 0


def far_layout(d, cols):
    """int64 element offsets of the rows of a descriptor whose extent is never materialised (the payload is [M, cols])"""
    assert cols >= 0
    return row_offsets(d)


def last_byte(d, cols):
    """the largest byte offset from the base that a row of the descriptor covers"""
    return (int(far_layout(d, cols).max()) + cols) * 4 - 1


def _solve(g, L, zone, step=4, lo=4):
    """a stride (multiple of `step`) in `zone` of the guard g(stride) < L, g increasing in the stride"""
    def last_in(lim):
        a, b = lo // step, 1 << 40
        assert g(a * step) < lim, "no stride is inside"
        while b - a > 1:
            m = (a + b) // 2
            a, b = (m, b) if g(m * step) < lim else (a, m)
        return a * step
    if zone == "edge-in":
        return last_in(L)
    if zone == "edge-out":
        return last_in(L) + step
    if zone == "over":
        return last_in(OVER * L) + step
    return last_in(0.9975 * L)                                      # high: g just below the limit, well inside


def stretch(d, cols, which, zone):
    """the descriptor with stride `which` ('bs' | 'rs') stretched into `zone` of sk_extent_ok"""
    assert which in ("bs", "rs") and (which == "rs" or d["batch"] > 1)
    mk = lambda s: dict(d, **({"bs": s} if which == "bs" else {"rs": s, "bs": d["rpb"] * s if d["batch"] > 1 else 0}))
    return mk(_solve(lambda s: a_guard(mk(s), cols), limits()["a_bytes"], zone, lo=max(4, d[which] if which == "rs" else d["rpb"] * d["rs"])))


def stretch_ldb(kind, K, N, zone):
    return _solve(lambda s: b_guard(KIND[kind], K, N, s), limits()["b_bytes"], zone, lo=(N if kind == "nn" else K))


def far_row_predict(r):
    """rows_dispatch for a FAR row of kind nn / nt: the extent predicates come from the row's own descriptors"""
    wsb, ws_al = row_ws_bytes(r)
    c = r["c"]
    return rows_dispatch(KIND[r["kind"]], r["M"], r["N"], r["K"], row_al(r), wsb, r["env"], r["epi"], ws_al, c["batch"], c["rpb"], c["rs"],
                         c["bs"], 0, 0, a_ext=sk_extent_ok(r["a"], r["K"]), b_ext=sk_b_extent_ok(KIND[r["kind"]], r["K"], r["N"], ldb_of(r)))


def far_tn_predict(r):
    a, b = r["a"], r["b"]
    al = lambda d: d["rs"] % 4 == 0 and (d["batch"] == 1 or d["bs"] % 4 == 0)
    wsb = tn_workspace(r["M"], r["K1"], r["N"], r["env"])
    return tn_dispatch(r["M"], r["K1"], r["N"], al(a), al(b), wsb, r["env"], 0, 0, r["N"] + r["ldc_pad"], r["bias_grad"], 0,
                       a_ext=sk_extent_ok(a, r["K1"]), b_ext=sk_extent_ok(b, r["N"]))


def compact(d, cols):
    """the same rows with compact strides"""
    return dict(batch=d["batch"], rpb=d["rpb"], rs=cols, bs=d["rpb"] * cols if d["batch"] > 1 else 0)


def compact_twin(r):
    """the row with every operand compact: same shape, same environment, same payload"""
    t = dict(r, name=r["name"] + "@compact", far={}, zone="compact")
    if r["kind"] == "tn":
        t.update(a=compact(r["a"], r["K1"]), b=compact(r["b"], r["N"]))
    else:
        t.update(a=compact(r["a"], r["K"]), c=compact(r["c"], r["N"]), ldb_pad=0)
    return t


def _far(r, zone, far, expect):
    r.update(zone=zone, far=far, expect=expect)
    return r


def _far_table():
    T = []
    SK16 = dict(SK_ENV, LIDBOX_GEMM_SK_GRID="16")
    SKP16 = dict(SK16, LIDBOX_GEMM_SKP="2")
    # kernel -> (env, M as 2 utterances, N, K, ws): the smallest shapes of the ROWS table that select it
    kernels = [("gemm_sk_rows_kernel", SK16, 250, 200, 520, "lib"), ("gemm_skp_rows_kernel", SKP16, 250, 200, 520, "lib"),
               ("gemm_rows_dma_kernel", _plan(64, 64), 130, 100, 40, "none"), ("gemm_rows_dma8_kernel", _plan(128, 64, 1, 8), 130, 100, 48, "none"),
               ("stream", _plan(64, 64), 64 * 33, 512, 256, "stream")]

    def expect(r, fast, kern, fam):
        """fast side: the named kernel; refused side: the register-staged kernels (family 0)"""
        if fast:
            return dict(family=fam, kernel=kern, stream=kern == "stream")
        return dict(family=0, kernel="gemm_rows")

    fam_of = {"gemm_sk_rows_kernel": 2, "gemm_skp_rows_kernel": 2, "gemm_rows_dma_kernel": 1, "gemm_rows_dma8_kernel": 3, "stream": 1}
    # 1. nn / nt, A stretched by batch_stride: high and over on every LDS-DMA rows kernel; both edges on one stream-K and one DMA row
    for kern, env, M, N, K, ws in kernels:
        for kind in ("nn", "nt"):
            zones = ["over", "high"]
            if (kern, kind) in (("gemm_sk_rows_kernel", "nn"), ("gemm_rows_dma_kernel", "nt")):
                zones = ["over", "edge-out", "edge-in", "high"]
            for zone in zones:
                a = stretch(_batched(2, M // 2, K), K, "bs", zone)
                fast = zone in ("high", "edge-in")
                T.append(_far(_row("far-A-bs-%s-%s-%s" % (kern.replace("gemm_", "").replace("_kernel", ""), kind, zone),
                                   "launch_rows: sk_extent_ok(A, K) %s by batch_stride (%s) -> %s" % ("true" if fast else "false", zone, kern if fast else "family 0"),
                                   kind, N, K, a, epi=EPI_BIAS_RELU if kind == "nn" else EPI_ACCUM, env=env, ws=ws), zone, {"A": "bs"},
                              expect(None, fast, kern, fam_of[kern])))
    # 2. the same two kernels, A stretched by row_stride (batch = 1)
    for kern, env, M, N, K, ws in (kernels[0], kernels[2]):
        kind = "nn" if kern == "gemm_sk_rows_kernel" else "nt"
        for zone in ("over", "high"):
            a = stretch(_dense(M, K), K, "rs", zone)
            fast = zone == "high"
            T.append(_far(_row("far-A-rs-%s-%s-%s" % (kern.replace("gemm_", "").replace("_kernel", ""), kind, zone),
                               "launch_rows: sk_extent_ok(A, K) %s by row_stride, batch = 1 (%s)" % ("true" if fast else "false", zone), kind, N, K, a,
                               epi=EPI_RELU, env=env, ws=ws), zone, {"A": "rs"}, expect(None, fast, kern, fam_of[kern])))
    # 3. B stretched by ldb: nt (N rows of ldb floats) and nn (K rows: SkOuter's vo and its 64-bit step); N resp. K = 1024 so that
    #    the last row of B lies above HIGH_BYTES while (rows + 16) ldb 4 stays below the limit
    for kern, env, M, _, _, ws in (kernels[0], kernels[2]):
        for kind in ("nt", "nn"):
            N, K = (1024, 64 if kern == "gemm_rows_dma_kernel" else 520) if kind == "nt" else (200, 1024)
            for zone in ("over", "high"):
                ldb = stretch_ldb(kind, K, N, zone)
                fast = zone == "high"
                T.append(_far(_row("far-B-ldb-%s-%s-%s" % (kern.replace("gemm_", "").replace("_kernel", ""), kind, zone),
                                   "launch_rows: sk_b_extent_ok %s by ldb (%s)" % ("true" if fast else "false", zone), kind, N, K, _dense(M, K),
                                   epi=EPI_BIAS, env=env, ws=ws, ldb_pad=ldb - (N if kind == "nn" else K)), zone, {"B": "ldb"},
                              expect(None, fast, kern, fam_of[kern])))
    # 6. C far, A and B compact: no guard looks at C, the kernels stay on the fast path.  store_rows_tile's inner test at both edges
    #    of wrap (2^30) and of row_stride (2^25); `off0`: every 32-row block inner and free of a boundary with off0 >= 2^32 bytes.
    #    rpb = 80 puts a boundary inside the block of rows 64 .. 95 (the wrap32 select); rpb = 96: none.
    Lm = limits()
    fams = [("f0", dict(_plan(64, 64), LIDBOX_GEMM_DMA="0"), 0, "gemm_rows_kernel", "none"), ("f1", _plan(64, 64), 1, "gemm_rows_dma_kernel", "none"),
            ("sk", SK16, 2, "gemm_sk_rows_kernel", "lib"), ("skp", SKP16, 2, "gemm_skp_rows_kernel", "lib")]
    for fname, env, fam, kern, ws in fams:
        for sub, c in (("wrap-edge-in", dict(batch=2, rpb=80, rs=1 << 19, bs=80 * (1 << 19) + Lm["inner_wrap"] - 4)),
                       ("wrap-edge-out", dict(batch=2, rpb=80, rs=1 << 19, bs=80 * (1 << 19) + Lm["inner_wrap"])),
                       ("off0", dict(batch=2, rpb=96, rs=1 << 19, bs=96 * (1 << 19) + Lm["inner_wrap"] - 4)),
                       ("rs-edge-in", dict(batch=1, rpb=40, rs=Lm["inner_rs"] - 4, bs=0)), ("rs-edge-out", dict(batch=1, rpb=40, rs=Lm["inner_rs"], bs=0))):
            if sub.startswith("rs-") and fam == 2:
                continue                                            # stream-K needs M >= 128: 17 GB of C at this row stride
            M = c["batch"] * c["rpb"]
            for epi in (EPI_BIAS_RELU, EPI_RELU_MASK, EPI_ACCUM):
                kind = "nt" if epi == EPI_ACCUM else "nn"
                T.append(_far(_row("far-C-%s-%s-e%d" % (sub, fname, epi), "store_rows_tile: C far (%s), no guard on C's extent -> %s stays" % (sub, kern),
                                   kind, 200, 520 if fam == 2 else 40, _dense(M, 520 if fam == 2 else 40), c=c, epi=epi, env=env, ws=ws), "c-far", {"C": sub},
                              dict(family=fam, kernel=kern, stream=False)))
    return T


def _far_tn_table():
    """4. tn: gemm_sk_tn_kernel and gemm_tn_dma_kernel with X far and with dY far, by batch_stride (a_wrap >= 2^29 in SkOuterRows'
    int arithmetic) and by row_stride (118 rows 2^23 floats apart: a_step = 16 rs >= 2^27)"""
    T = []
    for kern, env_bs, env_rs, fam in (("gemm_sk_tn_kernel", dict(SK_ENV, LIDBOX_GEMM_SK_GRID="4"), dict(SK_ENV, LIDBOX_GEMM_SK_GRID="1"), 2),
                                      ("gemm_tn_dma_kernel", {"LIDBOX_GEMM_TN_PLAN": "64,64,3"}, {"LIDBOX_GEMM_TN_PLAN": "64,64,2"}, 1)):
        for which in ("bs", "rs"):
            M, K1, N = (1000, 128, 128) if which == "bs" else (118, 128, 128)
            for op in ("X", "dY"):
                for zone in ("over", "high"):
                    base = _batched(2, M // 2, 128) if which == "bs" else _dense(M, 128)
                    far = stretch(base, 128, which, zone)
                    a, b = (far, compact(base, N)) if op == "X" else (compact(base, K1), far)
                    fast = zone == "high"
                    r = _tn_row("far-tn-%s-%s-%s-%s" % (kern.replace("gemm_", "").replace("_kernel", ""), op, which, zone),
                                "tn_partial_launch: sk_extent_ok(%s) %s by %s (%s)" % ("A, K1" if op == "X" else "Bd, N", "true" if fast else "false", which, zone),
                                K1, N, a, b=b, env=env_bs if which == "bs" else env_rs, accumulate=1 if op == "X" else 0, bias_grad=True)
                    T.append(_far(r, zone, {op: which}, dict(family=fam if fast else 0, kernel=kern if fast else "gemm_tn_kernel")))
    return T


def _far_pair_table():
    """5. lidbox_gemm_nt_tn: al_rows refused alone (W's ldb over the limit), al_tn refused alone (X over the limit by batch_stride)"""
    T = []
    M, Co, N, K1 = 64, 64, 128, 64
    T.append(dict(name="far-pair-al_rows", why="lidbox_gemm_nt_tn: only al_rows false (sk_b_extent_ok by ldb) -> the two calls", kind="pair", M=M, Co=Co,
                  N=N, K1=K1, env={}, ldb=stretch_ldb("nt", Co, N, "over"), x=_dense(M, K1), zone="over", far={"B": "ldb"}, refused="al_rows"))
    T.append(dict(name="far-pair-al_tn", why="lidbox_gemm_nt_tn: only al_tn false (sk_extent_ok(X, K1) by batch_stride) -> the two calls", kind="pair", M=M,
                  Co=Co, N=N, K1=K1, env={}, ldb=Co, x=stretch(_batched(2, M // 2, K1), K1, "bs", "over"), zone="over", far={"X": "bs"}, refused="al_tn"))
    return T


def _far_job_table():
    """7. lidbox_reduce_jobs_run on a hand-made job: N = 1024, n = 2^20; splits = 940: 3.94e9 bytes of slices (high); 960: 4.03e9,
    over reduce_job_vec_ok's limit yet below 2^32 -- the entry point does not test the limit (only the callers that build a job
    do), the 16-byte kernel runs and its unsigned scalar offsets k n 4 still fit: the sum must be right"""
    return [dict(name="far-job-s%d-bp%d-acc%d" % (s, bp, acc), why="reduce_slices: scalar offset k n 4 up to %.3g bytes" % job_guard(s - 1, 1 << 20), kind="job",
                 N=1024, n=1 << 20, splits=s, bias_partials=bool(bp), accumulate=acc, zone="high" if job_guard(s, 1 << 20) < limits()["job_bytes"] else "over")
            for s in (960, 940) for bp in (0, 1) for acc in (0, 1)]


def far_deref_bytes(r):
    """operand -> the largest byte offset from its base that the call dereferences"""
    out = {}
    if r["kind"] in ("nn", "nt"):
        out["A"] = last_byte(r["a"], r["K"])
        brows = r["K"] if r["kind"] == "nn" else r["N"]
        out["B"] = ((brows - 1) * ldb_of(r) + (r["N"] if r["kind"] == "nn" else r["K"])) * 4 - 1
        out["C"] = last_byte(r["c"], r["N"])
    elif r["kind"] == "tn":
        out["X"], out["dY"] = last_byte(r["a"], r["K1"]), last_byte(r["b"], r["N"])
    return out


def far_guard(r, op):
    """(g, L) of the guard that looks at operand `op` of the row"""
    L = limits()
    if op == "A":
        return a_guard(r["a"], r["K"]), L["a_bytes"]
    if op == "B":
        return b_guard(KIND[r["kind"]], r["K"], r["N"], ldb_of(r)), L["b_bytes"]
    if op == "X":
        return a_guard(r["a"], r["K1"]), L["a_bytes"]
    if op == "dY":
        return a_guard(r["b"], r["N"]), L["a_bytes"]
    raise KeyError(op)


PATHS["FAR"] = _far_table() + _far_tn_table() + _far_pair_table() + _far_job_table()


# -- the sparse judge: the payload [M, N] gathered on the device, and the count of words of C's whole allocation that no longer
#    hold the fill; never a flat host array
def judge_far_rows(r, ds, dat, got, changed_words, p):
    """judge_rows for a far C: `got` the [M, N] payload read through the descriptor, changed_words the number of words of the
    allocation (margins included) that differ from the NaN fill after the call"""
    M, N = r["M"], r["N"]
    got = np.asarray(got, np.float32).reshape(M, N)
    if changed_words != M * N:
        return False, np.inf, "words outside the payload were written, or payload words were not (%d changed, %d expected)" % (changed_words, M * N)
    ref, S = rows_reference(r["kind"], dat["A"], dat["B"], r["epi"], dat["bias"], dat["mask"], dat["old"])
    if ds == "exact":
        same = np.array_equal(_bits(got), _bits(ref.astype(np.float32)))
        return same, 0.0 if same else np.inf, "bits"
    q = ratio(got, ref, S, chain_n(r["K"], p, r["epi"]))
    return bool((q <= 1.0).all()), float(q.max()), "bound"


# -- planted addressing mistakes on the far layout.  An allocation is [margin][extent][256 bytes] with the base at the start of
#    the extent and every word NaN but the payload rows; a load is emulated on byte offsets.
FAR_MARGIN = (1 << 31) + 256
FAR_TAIL = 256
ADDRESSING_MISTAKES = ("sign_extended_32", "truncated_mod_2^32", "element_offset_mod_2^31", "limit_in_elements", "wrap32_beyond_2^30")


def mistaken_offsets(mut, d, cols):
    """byte offsets of the rows under the planted mistake (int64), or None where the mistake cannot change any row of d"""
    off = far_layout(d, cols) * 4
    last = off + (cols - 1) * 4
    if mut == "sign_extended_32":                                   # a 32-bit byte offset widened as signed
        bad = ((off & 0xffffffff) ^ 0x80000000) - 0x80000000
    elif mut in ("truncated_mod_2^32", "limit_in_elements"):        # 64 -> 32 bits; an element offset that fits, times 4 in 32 bits
        bad = off & 0xffffffff
    elif mut == "element_offset_mod_2^31":
        bad = ((off // 4) & 0x7fffffff) * 4
    elif mut == "wrap32_beyond_2^30":                               # the select adds (wrap * 4) mod 2^32 behind an utterance boundary
        if d["batch"] == 1:
            return None
        wrap = d["bs"] - d["rpb"] * d["rs"]
        b = np.arange(d["batch"] * d["rpb"], dtype=np.int64) // d["rpb"]
        bad = off - b * (wrap * 4) + b * ((wrap * 4) & 0xffffffff)
    else:
        raise KeyError(mut)
    del last
    return None if np.array_equal(bad, off) else bad


def _far_rows_in(d, cols, bad_off):
    off = far_layout(d, cols) * 4
    ext = int(off.max()) + cols * 4
    inside = (bad_off >= -FAR_MARGIN) & (bad_off + cols * 4 <= ext + FAR_TAIL)
    return off, inside


def emulate_far_gather(d, cols, payload, bad_off):
    """what a kernel reads that forms its row addresses as bad_off: (values [M, cols], left): payload words where a mistaken row
    lands on payload, NaN (the fill) elsewhere inside the allocation; left = number of rows that left the allocation"""
    off, inside = _far_rows_in(d, cols, bad_off)
    order = np.argsort(off)
    so = off[order]
    w = bad_off[:, None] + 4 * np.arange(cols, dtype=np.int64)[None, :]          # word by word: a row may straddle a payload row
    i = np.searchsorted(so, w.ravel(), side="right").reshape(w.shape) - 1
    rel = w - so[np.maximum(i, 0)]
    hit = (i >= 0) & (rel < cols * 4) & (rel % 4 == 0) & inside[:, None]
    out = np.full(w.shape, np.nan, np.float32)
    out[hit] = np.asarray(payload, np.float32)[order[np.maximum(i, 0)][hit], (rel // 4)[hit]]
    return out, int((~inside).sum())


def emulate_far_scatter(d, cols, result, bad_off, old=None):
    """what C's true rows hold after a kernel stored `result` through bad_off: (payload read back through the true offsets,
    changed words in the allocation, left); rows are stored in order, the later row wins"""
    off, inside = _far_rows_in(d, cols, bad_off)
    col = 4 * np.arange(cols, dtype=np.int64)[None, :]
    true_w = (off[:, None] + col).ravel()
    addr = (bad_off[inside][:, None] + col).ravel()
    vals = np.asarray(result, np.float32)[inside].ravel()
    if old is not None:
        addr, vals = np.concatenate([true_w, addr]), np.concatenate([np.asarray(old, np.float32).ravel(), vals])
    uniq, first_rev = np.unique(addr[::-1], return_index=True)
    uv = vals[::-1][first_rev]
    j = np.searchsorted(uniq, true_w)
    j = np.minimum(j, max(len(uniq) - 1, 0))
    got = np.full(true_w.shape, np.nan, np.float32)
    if len(uniq):
        hit = uniq[j] == true_w
        got[hit] = uv[j[hit]]
    return got.reshape(len(off), cols), int(len(uniq)), int((~inside).sum())
