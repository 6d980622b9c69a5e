"""
The bf16 GEMM families (csrc/gemm_bf16.hip on gemm16_dma.h, gemm16_pp.h, gemm16_kres.h, gemm16_pp_tn.h, gemm16_tn_kres.h) on their
dispatch paths: the host policy restated in Python, float64 references, per-element bounds, three data sets, an fp32 emulation of
one launch with plantable mutations, and the PATHS tables that tests/test_gemm16_paths_gpu.py runs.  numpy only;
tests/test_oracle_gemm16_paths.py checks every restated function against lidbox_gemm_bf16_plan_query and the three workspace
exports on the CPU (rows_workspace16s restates what the callers of lidbox_gemm_bf16s_nt size from the plan: it has no export).  The layout follows oracle/gemm_paths_np.py (the fp32 family), whose descriptor, epilogue, data and bound
helpers are imported, not copied.

1. Dispatch.  plan_rows16 (BK 32 / 64), the tail split (plan_tail16: TAIL_MIN_K, TAIL_MIN_ROUNDS, slots 2 NUM_CU / WAVES_S NUM_CU),
   choose_dma16 (LIDBOX_GEMM16S_DMA = "0" | "bm,bn,st" | "bm,bn,st,splits"), kres_applies and the c_ok / epi_ok / worth-it
   conditions of plan_rows16s, plan_tn16, plan_tn16_pp, plan_tn16_kres, span_ok and desc_ok of plan_tn16s, pp2_problem, the
   alignment refusals of the three entry families and the workspace functions, line by line; the environment is an explicit
   dict (LIDBOX_GEMM16S_DMA, LIDBOX_GEMM16S_KRES, LIDBOX_GEMM16_TN_PP, LIDBOX_GEMM16_TN_KRES, LIDBOX_GEMM_NO_CARRY,
   LIDBOX_GEMM_CARRY_BLOCKS).  reduce_job_vec_ok is the fp32 module's.  The constexpr constants are READ from the source text
   (constants()); NUM_CU is the compile-time 256.  plan_query() returns the twelve numbers of lidbox_gemm_bf16_plan_query.

2. References (float64).  Compute family (lidbox_gemm_bf16_nn / _nt / _tn): operands rounded to bf16 round-to-nearest-even, then
   float64; the fused bias gradient is summed from the UNROUNDED operand.  Storage family (lidbox_gemm_bf16s_*): the stored bf16
   values widened exactly; the bias gradient is summed from the shadow's values.

3. Bounds, per element: conv2d_np.error_bound(S, n), n = 2 K + p + e as in gemm_paths_np.py (a bf16 x bf16 product is exact in
   fp32, so only the accumulation rounds): p = K splits (the larger plan of a tail split), wgrad slices; e = 1 + 1 with a bias or
   old C.  wgrad: K = the contracted rows of one slice; bias gradient n = rows of a slice + slices + 1.
   Shadow: with an fp32 C as well, C16 == bf16_rne(C) bit for bit; shadow only, C16 lies in [bf16_rne(ref - bound),
   bf16_rne(ref + bound)] (rounding is monotonic: the exact image of the fp32 bound; bf16_rne64 rounds the float64 ends directly).

4. Data sets: gemm_paths_np's `normal`, `offset`, `exact`.  Storage operands are the draws rounded to bf16 (exact: integers in
   [-7, 7], already bf16): every sum is an integer below 2^24, so fp32 outputs equal int64 bit for bit, the shadow equals the RNE
   bf16 of that integer (ties occur beyond 256 and must go to even), masks come from {-2, -0.0, 0.0, 3} in fp32 and bf16 form.

5. emulate_rows / emulate_tn: fp32 emulation of one launch (64-deep steps for the storage kernels, 32-deep for the fp32-source
   ones; splits and slices summed in order; epilogue, pitched fp32 store, shadow store) with MUTATIONS planted; applies() holds
   the explicit exclusion rules.

6. PATHS: ROWS16 (lidbox_gemm_bf16_nn / _nt), TN16, ROWS16S (lidbox_gemm_bf16s_nt), TN16S (_tn / _tn_partial), PAIR16S, CARRY16S,
   CONVERT, and BIG16S / BIGTN16S: the policy branches and the tail split that need about 192 tiles of 256 x 256 or 513 row tiles,
   judged on sampled rows / columns (sample_rows) and bit for bit against a second launch of known path.  Every row names the source condition it is there for in `why`; shapes were found by searching the restated planner
   for the smallest that select the path.  UNREACHED lists policy conditions no shape can select, each with its proof.

Largest err / bound seen on the device (one run on one MI355X; per kernel in the docstring of tests/test_gemm16_paths_gpu.py): 0.087
(gemm16s_rows_dma_kernel<128,64,2>); every `exact` case bit-equal, fp32 and shadow.  The CPU emulation's largest figure is 0.087 too.

The 32-bit-extent terms (a_ext, b_ext, a_span with its per-utterance limit, span_ok, pp2_problem's a_ext / b_ext) are restated
with their limits READ from gemm_bf16.hip (limits16); PATHS["FAR16"] holds rows on both sides of each, found by stretching one
stride of a descriptor.  The planner only looks at the descriptors, so tests/test_oracle_gemm16_paths.py pins both sides of
every limit on the CPU through lidbox_gemm_bf16_plan_query.
"""
import os
import re

import numpy as np

from oracle import conv2d_np
from oracle import gemm_paths_np as gp
from oracle.gemm_paths_np import (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU_MASK, EPI_ACCUM, EPI_ACCUM_RELU_MASK, EPI_ACCUM_RELU, EPI_RELU,
                                  EPI_HAS_BIAS, EPI_HAS_MASK, EPI_ACCUMS, EPI_RELUS, cdiv, _atoi, _dense, _batched, _conv, reduce_job_vec_ok,
                                  DATASETS)

NUM_CU = 256
EPI_MASK_BF16 = 0x100
Q16_NN, Q16_NT, Q16_TN, Q16S_NT, Q16S_TN = range(5)
K_REFUSED, K_NONE, K_ROWS, K_TN, KS_ROWS, KS_DMA, KS_PP, KS_KRES13, KS_KRES0, KS_TN, KS_TN_PP, KS_TN_KRES = range(-1, 11)
R_NONE, R_ROWS, R_JOB4, R_SCALAR = range(4)
ENV_KEYS = ("LIDBOX_GEMM16S_DMA", "LIDBOX_GEMM16S_KRES", "LIDBOX_GEMM16_TN_PP", "LIDBOX_GEMM16_TN_KRES", "LIDBOX_GEMM_NO_CARRY",
            "LIDBOX_GEMM_CARRY_BLOCKS")
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lidbox_amd", "csrc")
_CONST = None


def constants():
    """the constexpr ints of the bf16 sources, read from the text: name -> value"""
    global _CONST
    if _CONST is None:
        _CONST = {}
        for f in ("gemm_bf16.hip", "gemm16_dma.h", "gemm16_kres.h", "gemm16_pp_tn.h", "gemm16_tn_kres.h", "gemm_shared.h"):
            with open(os.path.join(_CSRC, f)) as fh:
                for m in re.finditer(r"constexpr int (\w+) = (\d+);", fh.read()):
                    _CONST.setdefault(m.group(1), int(m.group(2)))
    return _CONST


def _c(name):
    return constants()[name]


# ------------------------------------------------------------------------------------------------ 1. the host dispatch
def plan_rows16(M, N, K, wsb, BK=32):
    """Rows16Plan: (splits, k_per_split)"""
    BT = _c("BT")
    tiles = cdiv(M, BT) * cdiv(N, BT)
    if tiles >= 2 * NUM_CU:
        return 1, K
    s = min((2 * NUM_CU) // tiles, K // (2 * BK), 64)
    while s > 1 and s * M * N * 4 > wsb:
        s -= 1
    if s <= 1:
        return 1, K
    kps = cdiv(cdiv(K, s), BK) * BK
    splits = cdiv(K, kps)
    return (1, K) if splits <= 1 else (splits, kps)


def plan_tail16(pl, M, N, K, wsb, BK, slots):
    """Rows16Tail: (m_main, rem plan); m_main == 0: one launch"""
    BT = _c("BT")
    tiles_n = cdiv(N, BT)
    tiles = cdiv(M, BT) * tiles_n
    if pl[0] == 1 and tiles > slots and K >= _c("TAIL_MIN_K"):
        rounds = tiles // slots
        rem_tiles = tiles - rounds * slots
        main_tiles_m = rounds * slots // tiles_n
        m_main = main_tiles_m * BT
        m_rem = M - m_main
        if rounds >= _c("TAIL_MIN_ROUNDS") and 0 < rem_tiles <= slots // 4 and main_tiles_m >= 1 and m_rem > 0:
            rp = plan_rows16(m_rem, N, K, wsb, BK)
            if rp[0] > 1:
                return m_main, rp
    return 0, (1, K)


def _sscanf_ints(s, n):
    """sscanf(s, "%d,%d,...") with n conversions: the values converted before the first mismatch"""
    out, pos = [], 0
    for i in range(n):
        m = re.match(r"\s*([+-]?\d+)", s[pos:])
        if not m:
            break
        out.append(int(m.group(1)))
        pos += m.end()
        if s[pos:pos + 1] != ",":
            break
        pos += 1
    return out


def choose_dma16(M, N, K, wsb, writes_fp32, env):
    """Dma16Choice as dict(bm, bn, stages, splits, kps); bm == 0: the register-staged kernel"""
    D = _c("D16_BK")
    none = dict(bm=0, bn=0, stages=0, splits=1, kps=0)
    sp = 0
    if "LIDBOX_GEMM16S_DMA" in env:
        v = _sscanf_ints(env["LIDBOX_GEMM16S_DMA"], 4)
        if len(v) < 3:
            return none
        bm, bn, stg = v[:3]
        sp = v[3] if len(v) > 3 else 0
        pp = bm == 256 and bn in (128, 256) and stg in (1, 2)
        if not pp and not (bm in (64, 128) and bn in (64, 128) and 2 <= stg <= 4):
            return none
    else:
        t256 = cdiv(M, 256) * cdiv(N, 256)
        r256 = cdiv(t256, NUM_CU)
        if (not (writes_fp32 and K < 1024 and t256 > NUM_CU) and
                ((K >= 512 and 4 * t256 >= 3 * r256 * NUM_CU) or (K >= 1500 and 2 * t256 >= r256 * NUM_CU))):
            return dict(bm=256, bn=256, stages=2, splits=1, kps=cdiv(K, D) * D)
        t128 = cdiv(M, 128) * cdiv(N, 128)
        t64x128 = cdiv(M, 64) * cdiv(N, 128)
        just_over = t64x128 > 3 * NUM_CU and 10 * t64x128 <= 12 * 3 * NUM_CU
        if t128 < NUM_CU // 2:
            bm, bn, stg = 64, 64, 2
        elif K >= 1536 and (t128 >= 3 * NUM_CU or just_over):
            bm, bn, stg = 128, 128, 2
        elif just_over:
            bm, bn, stg = 64, 64, 2
        else:
            bm, bn, stg = 64, 128, 2
    tiles = cdiv(M, bm) * cdiv(N, bn)
    s = sp if sp > 0 else 1
    if sp <= 0 and tiles < 2 * NUM_CU:
        s = min((2 * NUM_CU) // tiles, K // (2 * D), 64)
    while s > 1 and s * M * N * 4 > wsb:
        s -= 1
    s = max(s, 1)
    kps = cdiv(cdiv(K, s), D) * D
    return dict(bm=bm, bn=bn, stages=stg, splits=cdiv(K, kps), kps=kps)


def dma_branch(M, N, K, writes_fp32):
    """which branch of choose_dma16's policy (no environment) a shape takes"""
    t256 = cdiv(M, 256) * cdiv(N, 256)
    r256 = cdiv(t256, NUM_CU)
    if not (writes_fp32 and K < 1024 and t256 > NUM_CU):
        if K >= 512 and 4 * t256 >= 3 * r256 * NUM_CU:
            return "pp_three_quarters"
        if K >= 1500 and 2 * t256 >= r256 * NUM_CU:
            return "pp_half_round"
    t128 = cdiv(M, 128) * cdiv(N, 128)
    t64x128 = cdiv(M, 64) * cdiv(N, 128)
    just_over = t64x128 > 3 * NUM_CU and 10 * t64x128 <= 12 * 3 * NUM_CU
    if t128 < NUM_CU // 2:
        return "t128_small"
    if K >= 1536 and (t128 >= 3 * NUM_CU or just_over):
        return "k1536_128x128"
    if just_over:
        return "just_over_64x64"
    return "default_64x128"


_LIM16 = None


def limits16():
    """the byte limits of the 32-bit-extent terms, read from gemm_bf16.hip"""
    global _LIM16
    if _LIM16 is None:
        with open(os.path.join(_CSRC, "gemm_bf16.hip")) as fh:
            src = fh.read()
        span = re.search(r"a_span < ([0-9.e]+) && tiles_n <= NUM_CU &&\s*\(\(double\)\(A\.rows_per_batch - 1\) \* \(double\)A\.row_stride \+ K\) \* 2\.0 < ([0-9.e]+);", src)
        ext = re.findall(r"a_ext < ([0-9.e]+) && b_ext < ([0-9.e]+)", src)
        sp = re.search(r"return r\.batch_stride >= 0 && r\.row_stride >= 0 && span < ([0-9.e]+);", src)
        assert span and len(ext) == 2 and sp, "an extent term of gemm_bf16.hip no longer reads as restated here"
        _LIM16 = dict(a_span=float(span.group(1)), a_utt=float(span.group(2)), a_ext=float(ext[0][0]), b_ext=float(ext[0][1]),
                      pair_a_ext=float(ext[1][0]), pair_b_ext=float(ext[1][1]), span=float(sp.group(1)))
    return _LIM16


def a_ext16(a, K):
    """a_ext (and a_span: the same expression) of plan_rows16s / pp2_problem, bytes"""
    return (float(a["batch"] - 1) * float(a["bs"]) + float(a["rpb"]) * float(a["rs"]) + K) * 2.0


def a_utt16(a, K):
    """the per-utterance term of the K-resident `can`"""
    return (float(a["rpb"] - 1) * float(a["rs"]) + K) * 2.0


def b_ext16(N, ldb, K):
    return (float(N) * float(ldb) + K) * 2.0


def span16(d, w):
    return (float(d["batch"] - 1) * float(d["bs"]) + float(d["rpb"] - 1) * float(d["rs"]) + w) * 2.0


def kres_applies(a, K, N):
    if not (K % 8 == 0 and 16 <= K <= _c("KRES_KMAX") and a["batch"] >= 1 and a["rpb"] >= 1):
        return False
    if a["rs"] < 8 or a["rs"] % 8 != 0 or (a["batch"] > 1 and a["bs"] % 8 != 0):
        return False
    kp = (K + 15) // 16 * 16
    return (_c("KRES_ROWS") - 1) * a["rs"] * 2 + kp * 2 <= _c("KRES_A_BYTES")


def rows16_operands_ok(kinner, a, a_res, b_res, ldb, c, c_res, K, N, ws_res):
    """rows16_operands_ok; *_res: a pointer's residue modulo 16"""
    al = lambda d, res: res == 0 and d["rs"] % 4 == 0 and (d["batch"] == 1 or d["bs"] % 4 == 0)
    return al(a, a_res) and al(c, c_res) and K % 4 == 0 and b_res == 0 and ldb % 4 == 0 and (kinner or N % 4 == 0) and ws_res == 0


def rows16s_operands_ok(a, a_res, b_res, ldb, c, c_res, c16_res, K, ws_res):
    """rows16s_operands_ok; c_res: of C.base (NULL counts as 0); c16_res: None without a shadow"""
    a_ok = a_res == 0 and a["rs"] % 8 == 0 and (a["batch"] == 1 or a["bs"] % 8 == 0)
    c_al = c_res == 0 and c["rs"] % 4 == 0 and (c["batch"] == 1 or c["bs"] % 4 == 0)
    return a_ok and c_al and K % 8 == 0 and b_res == 0 and ldb % 8 == 0 and ws_res == 0 and (c16_res is None or c16_res % 2 == 0)


def kres_conditions(a, c, K, N, epi, has_mask16, carries, c_res=0, c16_res=0):
    """the named conditions of `can` in plan_rows16s (every one must hold)"""
    tiles_n = cdiv(N, _c("KRES_BN"))
    return dict(
        no_jobs=not carries,
        epi_ok=epi in (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU),
        c_ok=(((c["batch"] == a["batch"] and c["rpb"] == a["rpb"]) or c["batch"] == 1) and N % 8 == 0 and c["rs"] % 4 == 0 and
              (c["batch"] == 1 or c["bs"] % 4 == 0) and c_res == 0 and (c16_res or 0) % 8 == 0),
        no_mask16=not has_mask16,
        applies=kres_applies(a, K, N),
        bs_nonneg=a["bs"] >= 0,
        a_span=a_ext16(a, K) < limits16()["a_span"],
        tiles_n=tiles_n <= NUM_CU,
        a_utt=a_utt16(a, K) < limits16()["a_utt"])


def plan_rows16s(a, ldb, c, K, N, epi, has_mask16, carries, wsb, env, c_null=False, c_res=0, c16_res=0):
    """Rows16sPlan as dict(kernel, dc | pl, tail)"""
    M = a["batch"] * a["rpb"]
    mode = _atoi(env["LIDBOX_GEMM16S_KRES"]) if "LIDBOX_GEMM16S_KRES" in env else -1
    tiles_n = cdiv(N, _c("KRES_BN"))
    can = mode != 0 and all(kres_conditions(a, c, K, N, epi, has_mask16, carries, c_res, c16_res).values())
    if can and (mode == 1 or (a["rs"] * 2 <= K and a["batch"] * tiles_n >= 2 * NUM_CU)):
        return dict(kernel=KS_KRES13 if (K + 15) // 16 == 13 else KS_KRES0)
    dc = choose_dma16(M, N, K, wsb, not c_null, env)
    if dc["bm"] != 0 and a_ext16(a, K) < limits16()["a_ext"] and b_ext16(N, ldb, K) < limits16()["b_ext"]:
        return dict(kernel=KS_PP if dc["bm"] == 256 else KS_DMA, dc=dc)
    pl = plan_rows16(M, N, K, wsb, _c("BKS"))
    return dict(kernel=KS_ROWS, pl=pl, tail=plan_tail16(pl, M, N, K, wsb, _c("BKS"), _c("WAVES_S") * NUM_CU))


def plan_tn16(M, K1, N, BK=32):
    """Tn16Plan: (splits, rows_per_split)"""
    BT = _c("BT")
    tiles = cdiv(K1, BT) * cdiv(N, BT)
    target = NUM_CU if (BK == 64 and tiles <= 16) else 2 * NUM_CU
    s = max(min(target // tiles, cdiv(M, 4 * BK)), 1)
    rps = cdiv(cdiv(M, s), BK) * BK
    return cdiv(M, rps), rps


def plan_tn16_pp(M, K1, N, env):
    """TnPpPlan: dict(use, splits, rps)"""
    BT, BM = _c("PPT_BT"), _c("PPT_BM")
    tiles = cdiv(K1, BT) * cdiv(N, BT)
    mode = _atoi(env["LIDBOX_GEMM16_TN_PP"]) if "LIDBOX_GEMM16_TN_PP" in env else -1
    if mode == 0 or tiles > NUM_CU or M >= (1 << 31) - BM:
        return dict(use=False, splits=1, rps=M)
    s = max(min(NUM_CU // tiles, cdiv(M, 4 * BM)), 1)
    rps = cdiv(cdiv(M, s), BM) * BM
    splits = cdiv(M, rps)
    full = K1 % BT == 0 and N % BT == 0
    return dict(use=mode == 1 or (full and tiles >= 8 and tiles * splits >= (3 * NUM_CU) // 4 and rps >= 2048), splits=splits, rps=rps)


def plan_tn16_kres(M, K1, N, env):
    """TnKresPlan: dict(shape_ok, forced, max_slices)"""
    BN = _c("TKR_BN")
    mode = _atoi(env["LIDBOX_GEMM16_TN_KRES"]) if "LIDBOX_GEMM16_TN_KRES" in env else -1
    if mode == 0 or K1 > _c("TKR_MAX_K1") or K1 % 8 != 0 or N % BN != 0 or N // BN > NUM_CU:
        return dict(shape_ok=False, forced=False, max_slices=1)
    forced = mode == 1
    return dict(shape_ok=forced or (K1 > 128 and M >= 65536), forced=forced, max_slices=NUM_CU // (N // BN))


def tkr_img_stride(rs):
    s = 2 * rs
    while s % 256 != 64:
        s += 8
    return s


def span_ok(d, w):
    return d["bs"] >= 0 and d["rs"] >= 0 and span16(d, w) < limits16()["span"]


def tn_pp_conditions(a, b, K1, N):
    """the descriptor conditions the ping-pong wgrad tile needs beside plan_tn16_pp().use"""
    return dict(span_a=span_ok(a, K1), span_b=span_ok(b, N), K1_8=K1 % 8 == 0, N_8=N % 8 == 0,
                same_utts=(a["batch"] == 1 and b["batch"] == 1) or (a["batch"] == b["batch"] and a["rpb"] == b["rpb"]))


def tn_kres_conditions(a, b, K1, N, kp):
    """desc_ok of plan_tn16s, term by term"""
    rs = a["rs"]
    return dict(shape_ok=kp["shape_ok"], enough_utts=kp["forced"] or 2 * a["batch"] >= kp["max_slices"], same_batch=a["batch"] == b["batch"],
                same_rpb=a["rpb"] == b["rpb"], rs_pos=rs > 0, bs_whole=rs > 0 and (a["batch"] == 1 or a["bs"] % rs == 0),
                bs_covers=rs > 0 and (a["batch"] == 1 or a["bs"] // rs >= a["rpb"]),
                gap_covered=a["batch"] == 1 or a["bs"] < a["rpb"] * rs + K1, img_elems=63 * rs + K1 <= _c("TKR_IMG_ELEMS"),
                img_bytes=rs > 0 and (63 + cdiv(K1, rs)) * tkr_img_stride(rs) <= _c("TKR_IMG_BYTES"), span_a=span_ok(a, K1), span_b=span_ok(b, N))


def plan_tn16s(a, b, M, K1, N, wsb, env):
    """Tn16sPlan: dict(kernel, splits, rps, ups, ws_ok)"""
    pl = plan_tn16(M, K1, N, _c("BKT"))
    pp = plan_tn16_pp(M, K1, N, env)
    if pp["use"] and not all(tn_pp_conditions(a, b, K1, N).values()):
        pp["use"] = False
    kp = plan_tn16_kres(M, K1, N, env)
    if all(tn_kres_conditions(a, b, K1, N, kp).values()):
        batch = a["batch"]
        slices = min(kp["max_slices"], batch)
        ups = cdiv(batch, slices)
        slices = cdiv(batch, ups)
        if wsb >= (slices * K1 * N + slices * N) * 4:
            return dict(kernel=KS_TN_KRES, splits=slices, rps=0, ups=ups, ws_ok=True)
    if pp["use"]:
        pl = (pp["splits"], pp["rps"])
    need = (pl[0] * K1 * N + pl[0] * N) * 4
    return dict(kernel=KS_TN_PP if pp["use"] else KS_TN, splits=pl[0], rps=pl[1], ups=0, ws_ok=wsb >= need)


def tn16s_operands_ok(a, a_res, b, b_res, K1, N, ws_res):
    ok16 = lambda d, res: res == 0 and d["rs"] % 8 == 0 and (d["batch"] == 1 or d["bs"] % 8 == 0)
    width_ok = lambda d, w: w % 8 == 0 or d["rs"] >= (w + 7) // 8 * 8
    return ok16(a, a_res) and ok16(b, b_res) and width_ok(a, K1) and width_ok(b, N) and ws_res == 0


def rows_workspace16(M, N, K):
    """lidbox_gemm_bf16_rows_workspace"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    s, _ = plan_rows16(M, N, K, 64 << 20)
    return s * M * N * 4 if s > 1 else 0


def tn_workspace16(M, K1, N):
    """lidbox_gemm_bf16_tn_workspace"""
    if M <= 0 or K1 <= 0 or N <= 0:
        return 0
    s, _ = plan_tn16(M, K1, N)
    return (s * K1 * N + s * N) * 4


def tn_workspace16s(M, K1, N, env):
    """lidbox_gemm_bf16s_tn_workspace"""
    if M <= 0 or K1 <= 0 or N <= 0:
        return 0
    splits = plan_tn16(M, K1, N, _c("BKT"))[0]
    pp = plan_tn16_pp(M, K1, N, env)
    if pp["use"] and pp["splits"] > splits:
        splits = pp["splits"]
    kp = plan_tn16_kres(M, K1, N, env)
    if kp["shape_ok"] and kp["max_slices"] > splits:
        splits = kp["max_slices"]
    return (splits * K1 * N + splits * N) * 4


def rows_workspace16s(M, N, K, env, writes_fp32=True):
    """what lidbox_gemm_bf16s_nt needs for its K split (the family has no export of its own: the callers size it from the plan)"""
    best = 0
    dc = choose_dma16(M, N, K, 1 << 40, writes_fp32, env)
    if dc["bm"] != 0:
        return dc["splits"] * M * N * 4 if dc["splits"] > 1 else 0
    s, _ = plan_rows16(M, N, K, 1 << 40, _c("BKS"))
    if s > 1:
        best = s * M * N * 4
    m_main, rp = plan_tail16((s, K), M, N, K, 1 << 40, _c("BKS"), _c("WAVES_S") * NUM_CU)
    if m_main:
        best = max(best, rp[0] * (M - m_main) * N * 4)
    return best


def carry_cap16(env):
    if "LIDBOX_GEMM_CARRY_BLOCKS" in env:
        v = _atoi(env["LIDBOX_GEMM_CARRY_BLOCKS"])
        if v >= 8:
            return v
    return 96


def pp2_conditions(call, wsb, env):
    """pp2_problem, term by term, for call = dict(a, c, K, N, epi, mask16, c_null, shadow, ldb + residues)"""
    a, c, K, N, epi = call["a"], call["c"], call["K"], call["N"], call["epi"]
    M = a["batch"] * a["rpb"]
    dc = choose_dma16(M, N, K, wsb, not call.get("c_null", False), env) if M > 0 and N > 0 and K > 0 else dict(bm=0, bn=0, stages=0, splits=1)
    if not (M > 0 and N > 0 and K > 0):                            # the first test of pp2_problem: nothing behind it is evaluated
        return dict(nonempty=False, shadow_only_ok=True, mask16_epi=True, aligned=True, not_kres=True, pp256_unsplit=True, ext=True)
    return dict(nonempty=True,
                shadow_only_ok=not call.get("c_null", False) or (call.get("shadow", True) and epi not in EPI_ACCUMS),
                mask16_epi=not call.get("mask16", False) or epi in EPI_HAS_MASK,
                aligned=rows16s_operands_ok(a, call.get("a_res", 0), call.get("b_res", 0), call.get("ldb", K), c, call.get("c_res", 0),
                                            0 if call.get("shadow", True) else None, K, 0),
                not_kres=call.get("mask16", False) or not kres_applies(a, K, N),
                pp256_unsplit=(dc["bm"], dc["bn"], dc["stages"], dc["splits"]) == (256, 256, 2, 1),
                ext=a_ext16(a, K) < limits16()["pair_a_ext"] and b_ext16(N, call.get("ldb", K), K) < limits16()["pair_b_ext"])


def plan_query(kind, a, b, c, K, N, epi, env, wsb, has_ws=True, res=None, c_null=False, shadow=True, mask16=False, njobs=0, bias_grad=True,
               ldb=None):
    """the twelve numbers of lidbox_gemm_bf16_plan_query.  res: pointer residues modulo 16 by name (A, B, C, C16, ws, bg)"""
    res = res or {}
    out = [0] * 12
    M = a["batch"] * a["rpb"]
    wsb = wsb if has_ws else 0
    ws_res = res.get("ws", 0) if has_ws else 0
    if kind in (Q16_NN, Q16_NT):
        if M == 0 or N == 0:
            return out
        if not rows16_operands_ok(kind == Q16_NT, a, res.get("A", 0), res.get("B", 0), ldb, c, res.get("C", 0), K, N, ws_res):
            return [K_REFUSED] + out[1:]
        pl = plan_rows16(M, N, K, wsb)
        m_main, rem = plan_tail16(pl, M, N, K, wsb, 32, 2 * NUM_CU)
        out[0], out[4], out[5], out[6] = K_ROWS, pl[0], pl[1], m_main
        if m_main:
            out[7], out[8] = rem
        out[9] = R_ROWS if (pl[0] > 1 or m_main) else R_NONE
        return out
    if kind == Q16S_NT:
        if M == 0 or N == 0:
            return out
        c16_res = res.get("C16", 0) if shadow else None
        c_res = 0 if c_null else res.get("C", 0)                     # a NULL base is 16-byte aligned
        if not rows16s_operands_ok(a, res.get("A", 0), res.get("B", 0), ldb, c, c_res, c16_res, K, ws_res):
            return [K_REFUSED] + out[1:]
        carries = njobs > 0 and "LIDBOX_GEMM_NO_CARRY" not in env
        d = plan_rows16s(a, ldb, c, K, N, epi, mask16, carries, wsb, env, c_null, c_res, c16_res)
        out[0] = d["kernel"]
        if d["kernel"] in (KS_KRES13, KS_KRES0):
            out[1:6] = [1, _c("KRES_BN"), 1, 1, K]
        elif d["kernel"] == KS_ROWS:
            out[4], out[5], out[6] = d["pl"][0], d["pl"][1], d["tail"][0]
            if d["tail"][0]:
                out[7], out[8] = d["tail"][1]
            out[9] = R_ROWS if (d["pl"][0] > 1 or d["tail"][0]) else R_NONE
        else:
            dc = d["dc"]
            out[1:6] = [dc["bm"], dc["bn"], dc["stages"], dc["splits"], dc["kps"]]
            out[9] = R_ROWS if dc["splits"] > 1 else R_NONE
        return out
    ldc = c["rs"]
    if M < 1 or M != b["batch"] * b["rpb"] or K < 1 or N < 1 or ldc < N:
        return [K_REFUSED] + out[1:]
    if kind == Q16_TN:
        al = lambda d, r: r == 0 and d["rs"] % 4 == 0 and (d["batch"] == 1 or d["bs"] % 4 == 0)
        if not (al(a, res.get("A", 0)) and al(b, res.get("B", 0)) and K % 4 == 0 and N % 4 == 0 and ws_res == 0):
            return [K_REFUSED] + out[1:]
        splits, rps = plan_tn16(M, K, N)
        out[0], out[4], out[5], out[10] = K_TN, splits, rps, int(wsb >= (splits * K * N + splits * N) * 4)
    else:
        if not tn16s_operands_ok(a, res.get("A", 0), b, res.get("B", 0), K, N, ws_res):
            return [K_REFUSED] + out[1:]
        d = plan_tn16s(a, b, M, K, N, wsb, env)
        splits = d["splits"]
        out[0], out[4], out[5], out[10], out[11] = d["kernel"], d["splits"], d["rps"], int(d["ws_ok"]), d["ups"]
    vec = reduce_job_vec_ok(ws_res, splits, K, N, res.get("C", 0), ldc, bias_grad, res.get("bg", 0))
    out[9] = R_JOB4 if vec else R_SCALAR
    return out


def kernel_name(q, kind=None):
    """the instantiation a plan_query result names, in the spelling of instantiations_from_source()"""
    k = q[0]
    if k == K_ROWS:
        return "gemm16_rows_kernel<%s>" % ("nt" if kind == Q16_NT else "nn")
    if k == KS_DMA:
        return "gemm16s_rows_dma_kernel<%d,%d,%d>" % (q[1], q[2], q[3])
    if k == KS_PP:
        return "gemm16s_rows_pp_kernel<%d,%d>" % (q[2], q[3])
    return {K_TN: "gemm16_tn_kernel", KS_ROWS: "gemm16s_rows_kernel", KS_KRES13: "gemm16s_rows_kres_kernel<13>", KS_KRES0: "gemm16s_rows_kres_kernel<0>",
            KS_TN: "gemm16s_tn_kernel", KS_TN_PP: "gemm16s_tn_pp_kernel", KS_TN_KRES: "gemm16s_tn_kres_kernel"}.get(k)


def instantiations_from_source():
    """the kernel instantiations the launch sites of gemm_bf16.hip name, enumerated from the source text: every hipLaunchKernelGGL
    site with its template arguments; symbols inside a launch_*_t wrapper or the LBX_D16 macro are replaced by the literal arguments
    of the calls / invocations that reach the site, and B_KINNER by both values (launch_rows16<true> and <false> are both called)."""
    with open(os.path.join(_CSRC, "gemm_bf16.hip")) as fh:
        src = fh.read().replace("\\\n", " ")
    found = set()
    d16 = sorted(set(re.findall(r"^\s*LBX_D16\((\d+), (\d+), (\d+), \d+\);", src, re.M)))
    pp = sorted(set(re.findall(r"launch_rows16s_pp_t<(\d+), (\d+)>\(", src)))
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)\s*(?:<([^>]*)>)?", src):
        name, targs = m.group(1), [t.strip() for t in m.group(2).split(",")] if m.group(2) else []
        if name == "gemm16_rows_kernel":
            assert targs == ["B_KINNER"] and "launch_rows16<true>" in src and "launch_rows16<false>" in src
            found |= {"gemm16_rows_kernel<nn>", "gemm16_rows_kernel<nt>"}
        elif name == "gemm16s_rows_dma_kernel":
            assert targs == ["BM", "BN", "STAGES", "OCC"]
            found |= {"gemm16s_rows_dma_kernel<%s,%s,%s>" % t for t in d16}
        elif name == "gemm16s_rows_pp_kernel":
            assert targs == ["BN", "SUB"]
            found |= {"gemm16s_rows_pp_kernel<%s,%s>" % t for t in pp}
        else:
            assert all(t.isdigit() for t in targs), (name, targs)
            found.add(name + ("<%s>" % ",".join(targs) if targs else ""))
    return sorted(found)


# ------------------------------------------------------------------------------------------------ 2. values and references
BF16_MAX = float(np.float32(3.3895313892515355e38))


def bf16_bits(x):
    """uint16 bf16 bits of fp32 values, round-to-nearest-even (NaN stays a quiet NaN)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_trunc_bits(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_widen(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_rne(x):
    """fp32 values rounded to bf16 RNE, as fp32"""
    return bf16_widen(bf16_bits(x))


def bf16_trunc(x):
    return bf16_widen(bf16_trunc_bits(x))


def bf16_rne64(x):
    """float64 values rounded to bf16 RNE directly (no fp32 step), as float64: the monotonic map the shadow interval uses"""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(np.where(np.isfinite(x), x, 0.0))
    ulp = np.ldexp(1.0, np.maximum(e - 1, -126) - 7)
    q = np.rint(x / ulp) * ulp
    q = np.where(np.abs(q) > BF16_MAX, np.copysign(np.inf, q), q)
    return np.where(np.isfinite(x), q, x)


def operands(r, dat):
    """the float64 operand values the reference multiplies: bf16_rne of the fp32 originals (compute family) or the stored bf16
    values (storage family: dat already holds them)"""
    if r["fam"] == "c":
        return bf16_rne(dat["A"]).astype(np.float64), bf16_rne(dat["B"]).astype(np.float64)
    return np.asarray(dat["A"], np.float64), np.asarray(dat["B"], np.float64)


def rows_reference(r, dat):
    A, B = operands(r, dat)
    return gp.rows_reference(r["kind"], A, B, r["epi"], dat["bias"], dat["mask"], dat["old"])


def tn_reference(r, dat):
    """(dW, S, bias grad, S); the bias gradient sums the UNROUNDED operand (compute) / the shadow's values (storage: the same array)"""
    A, B = operands(r, dat)
    N = r["N"]
    v, S = A.T @ B, np.abs(A).T @ np.abs(B)
    Bg = np.asarray(dat["B"], np.float64)
    g, Sg = Bg.sum(0), np.abs(Bg).sum(0)
    if r["accumulate"]:
        old = np.asarray(dat["c_flat"][:, :N], np.float64)
        v, S = v + old, S + np.abs(old)
        if r["bias_grad"]:
            ob = np.asarray(dat["old_bg"], np.float64)
            g, Sg = g + ob, Sg + np.abs(ob)
    return v, S, g, Sg


def _bias_grad_reference(r, dat):
    Bg = np.asarray(dat["B"], np.float64)
    g, Sg = Bg.sum(0), np.abs(Bg).sum(0)
    if r["accumulate"] and r["bias_grad"]:
        ob = np.asarray(dat["old_bg"], np.float64)
        g, Sg = g + ob, Sg + np.abs(ob)
    return None, None, g, Sg


# ------------------------------------------------------------------------------------------------ 3. judging
NAN_BITS = 0x7FC00000
NAN16 = 0x7FC0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def judge_rows(r, ds, dat, got_c, got_c16, p, rows=None):
    """(inside, worst err / bound, what).  got_c: the flat fp32 C after the call (None: shadow only); got_c16: the flat shadow as
    uint16 bits (None: no shadow).  Covered elements inside the bound (`exact`: the int64 result bit for bit), every gap word still
    the NaN it started as, the shadow by the rules of section 3."""
    M, N = r["M"], r["N"]
    idx = gp.index(r["c"], N)
    cover = np.zeros(dat["c_flat"].size, bool)
    cover[idx.ravel()] = True
    if rows is not None:                                            # a sample of rows (the big rows): the reference of those rows only
        rows = np.asarray(rows)
        sub = dict(dat, A=dat["A"][rows], mask=None if dat["mask"] is None else dat["mask"][rows], old=None if dat["old"] is None else dat["old"][rows])
        ref, S = rows_reference(r, sub)
        idx = idx[rows]
    else:
        ref, S = rows_reference(r, dat)
    n = gp.chain_n(r["K"], p, r["epi"])
    worst = 0.0
    if got_c is not None:
        got_c = np.asarray(got_c, np.float32)
        if got_c.size != cover.size or not (_bits(got_c)[~cover] == NAN_BITS).all():
            return False, np.inf, "a gap word of C was written"
        got = got_c[idx]
        if ds == "exact":
            if not np.array_equal(_bits(got), _bits(ref.astype(np.float32))):
                return False, np.inf, "fp32 bits"
        else:
            q = gp.ratio(got, ref, S, n)
            worst = float(q.max())
            if worst > 1.0:
                return False, worst, "fp32 bound"
    if got_c16 is not None:
        got_c16 = np.asarray(got_c16, np.uint16)
        if got_c16.size != cover.size or not (got_c16[~cover] == NAN16).all():
            return False, np.inf, "a gap word of the shadow was written"
        s = got_c16[idx]
        if got_c is not None:
            if not np.array_equal(s, bf16_bits(got_c[idx])):
                return False, np.inf, "shadow != bf16_rne(C)"
        elif ds == "exact":
            if not np.array_equal(s, bf16_bits(ref.astype(np.float32))):
                return False, np.inf, "shadow bits"
        else:
            b = conv2d_np.error_bound(S, n)
            v = bf16_widen(s).astype(np.float64)
            lo, hi = bf16_rne64(ref - b), bf16_rne64(ref + b)
            if not (np.isfinite(v) & (v >= lo) & (v <= hi)).all():
                return False, np.inf, "shadow outside [rne(ref - b), rne(ref + b)]"
    return True, worst, "ok"


def sample_rows(M, edges=(), seed=0):
    """the rows a big case is judged on: the first and last row of the 256-row tiles at both ends of M, the rows around `edges`
    (a tail split's m_main) and 64 random rows"""
    rows = {0, min(255, M - 1), (M - 1) // 256 * 256, M - 1}
    for e in edges:
        rows |= {x for x in (e - 1, e, e + 1) if 0 <= x < M}
    rows |= set(int(x) for x in np.random.default_rng(seed).integers(0, M, 64))
    return np.array(sorted(rows))


def judge_tn(r, ds, dat, got_c, got_bg, splits, rows_in_slice, cols=None):
    """(inside, worst dW, worst bias grad): dW [K1, ldc] with NaN still behind column N.  cols: judge dW on these output columns only
    (the big rows; the bias gradient is always judged whole)"""
    N = r["N"]
    got_c = np.asarray(got_c, np.float32).reshape(r["K1"], N + r["ldc_pad"])
    if not (_bits(got_c[:, N:]) == NAN_BITS).all():
        return False, np.inf, 0.0
    if cols is not None:
        cols = np.asarray(cols)
        sub = dict(dat, B=dat["B"][:, cols], c_flat=dat["c_flat"][:, cols], old_bg=None if dat["old_bg"] is None else dat["old_bg"][cols])
        v, S, _, _ = tn_reference(dict(r, N=len(cols), bias_grad=False), sub)
        _, _, g, Sg = _bias_grad_reference(r, dat)
        got_c = np.concatenate([got_c[:, cols], got_c[:, N:]], 1)
        N = len(cols)
    else:
        v, S, g, Sg = tn_reference(r, dat)
    if ds == "exact":
        ok = np.array_equal(_bits(got_c[:, :N]), _bits(v.astype(np.float32)))
        okg = (not r["bias_grad"]) or np.array_equal(_bits(got_bg), _bits(g.astype(np.float32)))
        return ok and okg, 0.0 if ok else np.inf, 0.0 if okg else np.inf
    rows = min(rows_in_slice, r["M"])
    q = gp.ratio(got_c[:, :N], v, S, 2 * rows + splits + 1 + r["accumulate"])
    qg = gp.ratio(got_bg, g, Sg, gp.bias_grad_n(rows, splits)) if r["bias_grad"] else np.zeros(1)
    return bool((q <= 1.0).all() and (qg <= 1.0).all()), float(q.max()), float(qg.max())


# ------------------------------------------------------------------------------------------------ 4. data
def make_rows_data(r, ds, seed=0):
    """inputs of one rows call as flat fp32 buffers (NaN in every gap) and dense views.  Storage family: every operand value is
    already a bf16 value (the test converts the flat buffers to bf16 exactly); `mask` is bf16-valued where the row reads a bf16 mask"""
    rng = np.random.default_rng([seed, DATASETS.index(ds), sum(map(ord, r["name"]))])
    M, N, K, kind, epi = r["M"], r["N"], r["K"], r["kind"], r["epi"]
    sto = r["fam"] == "s"
    rnd = bf16_rne if sto else (lambda x: x)
    a_flat = rnd(gp.fill_flat(rng, ds, r["a"], K))
    ldb = ldb_of(r)
    brows, bcols = (K, N) if kind == "nn" else (N, K)
    b_flat = np.full(brows * ldb, np.nan, np.float32)
    Bv = b_flat.reshape(brows, ldb)
    Bv[:, :bcols] = rnd(gp.draw(rng, ds, (brows, bcols)))
    c_flat = np.full(gp.extent(r["c"], N), np.nan, np.float32)
    old = None
    if epi in EPI_ACCUMS:
        old = gp.draw(rng, ds, (M, N), "int" if ds == "exact" else "ab")
        if ds == "exact" and sto:
            old = old + np.float32(300.0)                          # 291 .. 309: the odd ones are not bf16 values
        c_flat[gp.index(r["c"], N)] = old
    bias = gp.draw(rng, ds, N, "int" if ds == "exact" else "ab") if epi in EPI_HAS_BIAS else None
    mask_flat = None
    if epi in EPI_HAS_MASK:
        mask_flat = gp.fill_flat(rng, ds, r["c"], N, "mask")
        if r.get("mask16"):
            mask_flat = bf16_rne(mask_flat)
    A = gp.gather(a_flat, r["a"], K)
    mask = mask_flat[gp.index(r["c"], N)] if mask_flat is not None else None
    return dict(a_flat=a_flat, b_flat=b_flat, c_flat=c_flat, bias=bias, mask_flat=mask_flat, A=A, B=Bv[:, :bcols].copy(), old=old, mask=mask)


def make_tn_data(r, ds, seed=0):
    """as gemm_paths_np.make_tn_data; storage family: bf16 values, the columns of a row padded to 8 behind K1 / N hold NaN"""
    rng = np.random.default_rng([seed, DATASETS.index(ds), sum(map(ord, r["name"]))])
    K1, N = r["K1"], r["N"]
    rnd = bf16_rne if r["fam"] == "s" else (lambda x: x)
    a_flat = rnd(gp.fill_flat(rng, ds, r["a"], K1))
    b_flat = rnd(gp.fill_flat(rng, ds, r["b"], N))
    c_flat = np.full((K1, N + r["ldc_pad"]), np.nan, np.float32)
    old_bg = None
    if r["accumulate"]:
        c_flat[:, :N] = gp.draw(rng, ds, (K1, N), "int" if ds == "exact" else "ab")
    if r["bias_grad"]:
        old_bg = gp.draw(rng, ds, N, "int" if ds == "exact" else "ab") if r["accumulate"] else np.full(N, np.nan, np.float32)
    return dict(a_flat=a_flat, b_flat=b_flat, c_flat=c_flat, old_bg=old_bg, A=gp.gather(a_flat, r["a"], K1), B=gp.gather(b_flat, r["b"], N))


# ------------------------------------------------------------------------------------------------ 5. emulation + mutations
MUTATIONS = ("drop_k_step", "drop_k_tail", "col_shift_32", "row_from_0", "mask_dense", "bias_next", "no_accum", "no_relu",
             "operand_trunc", "shadow_trunc", "shadow_pre_epi", "split_last_dropped", "split_first_twice", "epi_per_split",
             "accum_reads_shadow", "mask16_f32_offsets", "mask_ge0", "bias_grad_rounded", "bias_grad_from_f32", "bias_grad_slice_omitted",
             "pair_epi_swapped", "carry_twice")


def step_depth(r):
    return 64 if r["fam"] == "s" else 32


def applies(mut, r, plan):
    """whether planting `mut` can change what the row's checks see: the explicit exclusion rules.  plan: dict(pieces = K splits or
    wgrad slices, per = k_per_split or rows of a slice)"""
    kind = r["kind"]
    tn = kind == "tn"
    epi = r.get("epi", EPI_NONE)
    pieces, BKs = plan["pieces"], step_depth(r)
    Kc = r["M"] if tn else r["K"]
    shadow, c_null = (not tn) and r.get("out", "f32") in ("both", "shadow"), (not tn) and r.get("out", "f32") == "shadow"
    if mut == "drop_k_step":
        return cdiv(min(plan["per"], Kc), BKs) >= 3                # an interior step of the first piece exists
    if mut == "drop_k_tail":                                       # the tail past the last whole step of the contraction
        return Kc % BKs != 0 and Kc > BKs
    if mut == "col_shift_32":
        return r["N"] > 32
    if mut == "row_from_0":
        return (r["K1"] if tn else r["M"]) > 1
    if mut == "mask_dense":
        return epi in EPI_HAS_MASK and r["M"] > 1 and not (r["c"]["batch"] == 1 and r["c"]["rs"] == r["N"])    # one row has no pitch
    if mut == "bias_next":
        return epi in EPI_HAS_BIAS and r["N"] > 1
    if mut == "no_accum":
        return epi in EPI_ACCUMS or (tn and r["accumulate"] == 1)
    if mut == "no_relu":
        return epi in EPI_RELUS
    if mut == "operand_trunc":                                     # storage operands are bf16 already: truncation is the identity
        return r["fam"] == "c"
    if mut == "shadow_trunc":
        return shadow
    if mut == "shadow_pre_epi":                                    # visible where the epilogue changes the value
        return shadow and epi != EPI_NONE
    if mut in ("split_last_dropped", "split_first_twice"):
        return pieces > 1
    if mut == "epi_per_split":                                     # additive / clamping epilogues only: a mask select commutes with the sum
        return (not tn) and pieces > 1 and epi in (EPI_BIAS, EPI_BIAS_RELU, EPI_ACCUM, EPI_ACCUM_RELU, EPI_RELU)
    if mut == "accum_reads_shadow":                                # (`exact` draws the old C of a storage row beyond 256, where bf16 holds even integers only)
        return shadow and epi in EPI_ACCUMS
    if mut == "mask16_f32_offsets":
        return (not tn) and bool(r.get("mask16")) and r["M"] * r["N"] > 1
    if mut == "mask_ge0":
        return epi in EPI_HAS_MASK
    if mut == "bias_grad_rounded":
        return tn and r["fam"] == "c" and r["bias_grad"]
    if mut == "bias_grad_from_f32":
        return tn and r["fam"] == "s" and r["bias_grad"]
    if mut == "bias_grad_slice_omitted":
        return tn and r["bias_grad"] and pieces > 1
    if mut == "pair_epi_swapped":                                  # the second problem of a pair row, where the two epilogues differ
        return r.get("table") == "PAIR16S" and "first_epi" in r and r["first_epi"] != epi
    if mut == "carry_twice":                                       # the wgrad job of a carry row; an accumulating reduce (a zero fill run twice is the same fill)
        return r.get("table") == "CARRY16S" and tn and r["accumulate"] == 1
    raise KeyError(mut)


def datasets_that_show(mut):
    """data sets on which a planted mutation must be caught (a mutation of rounding shows only where values need rounding)"""
    if mut in ("operand_trunc", "bias_grad_rounded", "bias_grad_from_f32"):
        return ("normal", "offset")                                # `exact` operands are bf16 already
    return DATASETS


def emulate_rows(r, dat, plan, mut=None):
    """fp32 emulation of one rows launch -> (C flat or None, shadow bits flat or None).  plan: dict(pieces, per[, m_main, rem])"""
    kind, epi, N, K, M = r["kind"], r["epi"], r["N"], r["K"], r["M"]
    BKs = step_depth(r)
    if r["fam"] == "c":
        rnd = bf16_trunc if mut == "operand_trunc" else bf16_rne
        A, B = rnd(dat["A"]), rnd(dat["B"])
    else:
        A, B = np.asarray(dat["A"], np.float32), np.asarray(dat["B"], np.float32)
    Bk = B if kind == "nn" else B.T
    idx = gp.index(r["c"], N)
    out = np.array(dat["c_flat"], np.float32)
    old = out[idx]
    if mut == "accum_reads_shadow" and epi in EPI_ACCUMS:
        old = bf16_rne(old)
    bias = None
    if epi in EPI_HAS_BIAS:
        bias = np.roll(dat["bias"], -1) if mut == "bias_next" else np.asarray(dat["bias"], np.float32)
    mk = None
    if epi in EPI_HAS_MASK:
        mf = np.asarray(dat["mask_flat"], np.float32)
        mk = mf[idx]
        if mut == "mask_dense":
            mk = mf[(np.arange(M)[:, None] * N + np.arange(N)[None, :]) % mf.size]
        if mut == "mask16_f32_offsets":                              # bf16 data read at twice the element offset
            mk = mf[np.minimum(2 * idx, mf.size - 1)]
            mk = np.where(np.isnan(mk), np.float32(1.0), mk)
        if mut == "mask_ge0":
            mk = np.where(mk >= 0, np.float32(1.0), np.float32(-1.0))
    e = epi
    if mut == "no_accum":
        e = {EPI_ACCUM: EPI_NONE, EPI_ACCUM_RELU_MASK: EPI_RELU_MASK, EPI_ACCUM_RELU: EPI_RELU}.get(epi, epi)
    if mut == "no_relu":
        e = {EPI_BIAS_RELU: EPI_BIAS, EPI_ACCUM_RELU: EPI_ACCUM, EPI_RELU: EPI_NONE}.get(epi, epi)
    if mut == "pair_epi_swapped":                                   # the second problem of a pair written with the first one's epilogue
        e = r["first_epi"]

    def block(m0, m1, pieces, per):
        parts = []
        for s in range(pieces):
            k0s, k1s = s * per, min(K, s * per + per)
            acc = np.zeros((m1 - m0, N), np.float32)
            nst = cdiv(k1s - k0s, BKs)
            for i in range(nst):
                k0, k1 = k0s + i * BKs, min(k1s, k0s + i * BKs + BKs)
                if mut == "drop_k_step" and s == 0 and i == nst // 2 and 0 < i < nst - 1:
                    continue
                if mut == "drop_k_tail" and k1 == K and K % BKs and K > BKs:
                    continue
                acc += A[m0:m1, k0:k1] @ Bk[k0:k1]
            parts.append(acc)
        if mut == "split_last_dropped" and pieces > 1:
            parts[-1] = np.zeros_like(parts[-1])
        if mut == "split_first_twice" and pieces > 1:
            parts.insert(1, parts[0])
        if mut == "epi_per_split" and pieces > 1:
            parts = [np.asarray(gp.apply_epi(p_, e, bias, None if mk is None else mk[m0:m1], old[m0:m1]), np.float32) for p_ in parts]
        v = np.zeros((m1 - m0, N), np.float32)
        for p_ in parts:
            v = v + p_
        return v

    m_main = plan.get("m_main", 0)
    if m_main:
        v = np.concatenate([block(0, m_main, plan["pieces"], plan["per"]), block(m_main, M, plan["rem"][0], plan["rem"][1])], 0)
    else:
        v = block(0, M, plan["pieces"], plan["per"])
    if mut == "col_shift_32":
        v = np.roll(v, -32, axis=1)
    if mut == "row_from_0":
        v[M - 1] = v[0]
    per_split = mut == "epi_per_split" and (plan["pieces"] > 1 or plan.get("m_main", 0))
    res = v if per_split else np.asarray(gp.apply_epi(v, e, bias, mk, old), np.float32)      # (per split: the epilogue ran on every partial)
    mode = r.get("out", "f32")
    c_out = s_out = None
    if mode in ("f32", "both"):
        out[idx] = res
        c_out = out
    if mode in ("both", "shadow"):
        s_out = np.full(out.size, NAN16, np.uint16)
        src = v if mut == "shadow_pre_epi" else res
        s_out[idx] = bf16_trunc_bits(src) if mut == "shadow_trunc" else bf16_bits(src)
    return c_out, s_out


def emulate_tn(r, dat, plan, mut=None):
    """fp32 wgrad: `pieces` slices of `per` contracted rows, 64- / 32-deep steps, slices summed in order -> (dW [K1, ldc], bias grad)"""
    BKs = step_depth(r)
    if r["fam"] == "c":
        rnd = bf16_trunc if mut == "operand_trunc" else bf16_rne
        A, B = rnd(dat["A"]), rnd(dat["B"])
        Bg = B if mut == "bias_grad_rounded" else np.asarray(dat["B"], np.float32)
    else:
        A, B = np.asarray(dat["A"], np.float32), np.asarray(dat["B"], np.float32)
        Bg = B * np.float32(1.0 + 2.0 ** -10) if mut == "bias_grad_from_f32" else B     # an fp32 original the shadow is the rounding of
    M, K1 = A.shape
    N, per = B.shape[1], plan["per"]
    splits = cdiv(M, per)
    P, Pc = np.zeros((splits, K1, N), np.float32), np.zeros((splits, N), np.float32)
    for s in range(splits):
        m0, m1 = s * per, min(M, s * per + per)
        nst = cdiv(m1 - m0, BKs)
        for i in range(nst):
            k0, k1 = m0 + i * BKs, min(m1, m0 + i * BKs + BKs)
            Pc[s] += Bg[k0:k1].sum(0, dtype=np.float32)
            if mut == "drop_k_step" and s == 0 and i == nst // 2 and 0 < i < nst - 1:
                continue
            if mut == "drop_k_tail" and k1 == M and M % BKs and M > BKs:
                continue
            P[s] += A[k0:k1].T @ B[k0:k1]
    if mut == "row_from_0":
        P[:, K1 - 1] = P[:, 0]
    if mut == "split_last_dropped":
        P[splits - 1] = 0
    if mut == "split_first_twice":
        P[0] *= 2
    if mut == "bias_grad_slice_omitted":
        Pc[splits - 1] = 0
    v, g = np.zeros((K1, N), np.float32), np.zeros(N, np.float32)
    for s in range(splits):
        v, g = v + P[s], g + Pc[s]
    if mut == "col_shift_32":
        v = np.roll(v, -32, axis=1)
    if mut == "carry_twice" and r["accumulate"]:                    # the carried job run by two launches: the slices added twice
        v, g = v + v, g + g
    out = np.array(dat["c_flat"], np.float32)
    acc = r["accumulate"] and mut != "no_accum"
    out[:, :N] = out[:, :N] + v if acc else v
    bg = None
    if r["bias_grad"]:
        bg = np.asarray(dat["old_bg"], np.float32) + g if acc else g
    return out, bg


# ------------------------------------------------------------------------------------------------ 6. PATHS
ALL_EPIS = list(range(8))
DMA_TILES = [(64, 64, 2), (64, 64, 3), (64, 64, 4), (128, 64, 2), (128, 64, 3), (64, 128, 2), (64, 128, 3), (128, 128, 2), (128, 128, 3)]
PP_TILES = [(256, 256, 2), (256, 256, 1), (256, 128, 2), (256, 128, 1)]
OUT_FORMS = ("f32", "both", "shadow", "mask16")


def ldb_of(r):
    return (r["N"] if r["kind"] == "nn" else r["K"]) + r.get("ldb_pad", 0)


def _row(table, name, why, fam, kind, N, K, a, c=None, epi=EPI_NONE, out="f32", mask16=False, env=None, ws="plan", res=None, ldb_pad=0,
         expect=None, **kw):
    M = a["batch"] * a["rpb"]
    c = _dense(M, N) if c is None else c
    assert c["batch"] * c["rpb"] == M, name
    assert not (out == "shadow" and epi in EPI_ACCUMS) and not (mask16 and epi not in EPI_HAS_MASK), name
    r = dict(table=table, name=name, why=why, fam=fam, kind=kind, M=M, N=N, K=K, a=a, c=c, epi=epi, out=out, mask16=mask16, env=dict(env or {}),
             ws=ws, res=dict(res or {}), ldb_pad=ldb_pad, expect=dict(expect or {}))
    r.update(kw)
    return r


def _tn_row(table, name, why, fam, K1, N, a, b=None, env=None, accumulate=0, bias_grad=True, ldc_pad=0, res=None, ws="lib", expect=None, **kw):
    M = a["batch"] * a["rpb"]
    b = _dense(M, N) if b is None else b
    r = dict(table=table, name=name, why=why, fam=fam, kind="tn", M=M, K1=K1, N=N, a=a, b=b, env=dict(env or {}), accumulate=accumulate,
             bias_grad=bias_grad, ldc_pad=ldc_pad, res=dict(res or {}), ws=ws, expect=dict(expect or {}))
    r.update(kw)
    return r


def _form(ti, epi):
    """(out, mask16) of the ti-th tile's row for an epilogue: every tile gets fp32 only, fp32 + shadow and shadow only among its
    NONE / BIAS / BIAS_RELU rows and a bf16 mask on its RELU_MASK row; the accumulating epilogues need an fp32 C"""
    three = ("f32", "both", "shadow")
    forms = {EPI_NONE: (three[ti % 3], False),
             EPI_BIAS: (three[(ti + 1) % 3], False),
             EPI_BIAS_RELU: (three[(ti + 2) % 3], False),
             EPI_RELU_MASK: (("both", "shadow")[ti % 2], True),
             EPI_ACCUM: (("f32", "both")[ti % 2], False),
             EPI_ACCUM_RELU_MASK: ("both", True) if ti % 2 else ("f32", False),
             EPI_ACCUM_RELU: (("both", "f32")[ti % 2], False),
             EPI_RELU: (three[(ti + 1) % 3], False)}
    return forms[epi]


def _rows16s_table():
    T = []
    tails = [8, 16, 24, 32, 40, 48, 56]
    # 1. forced storage tiles at ragged shapes: M in {1, bm - 1, bm + 1, 2 bm + 3}, N % bn != 0 (36, 8 among them), K = 8 and 64 j + t
    #    for every tail t, every epilogue once per tile, every output form; pitched A / B / C with NaN in the gaps, batched C
    for ti, (bm, bn, st) in enumerate(DMA_TILES + PP_TILES + [(0, 0, 0)]):
        env = {"LIDBOX_GEMM16S_DMA": "0" if bm == 0 else "%d,%d,%d" % (bm, bn, st)}
        ebm, ebn = (bm, bn) if bm else (128, 128)
        kern = KS_ROWS if bm == 0 else (KS_PP if bm == 256 else KS_DMA)
        for ei, epi in enumerate(ALL_EPIS):
            M = [1, ebm - 1, ebm + 1, 2 * ebm + 3][(ei + ti) % 4]
            N = [36, 8, ebn + 36, ebn + 8, 2 * ebn - 4, ebn - 8, 36, ebn + 4][ei]
            j = (ei + ti) % 8
            K = 8 if j == 7 else 64 * (1 + j % 3) + tails[j]
            out, m16 = _form(ti, epi)
            c = _dense(M, N, 4) if M < 6 or ei % 2 else _batched(3 if M % 3 == 0 else 1, M // 3 if M % 3 == 0 else M, N, 4, 8)
            T.append(_row("ROWS16S", "tile-%d.%d.%d-e%d" % (bm, bn, st, epi),
                          "launch_rows16s_dma: forced %s, M = %d, N = %d (N %% bn != 0), K = %d (tail %d), epilogue %d, %s%s" %
                          ("register-staged kernel" if bm == 0 else "tile %d x %d, %d" % (bm, bn, st), M, N, K, K % 64, epi, out, " + bf16 mask" if m16 else ""),
                          "s", "nt", N, K, _dense(M, K, 8), c=c, epi=epi, out=out, mask16=m16, env=env, ldb_pad=8, ws="none",
                          expect=dict(kernel=kern, tile=(bm, bn, st), splits=1)))
        # a forced K split whose last split is short (K = 328: 3 x 128 -> 128 + 128 + 72), and one where the k_per_split rounding leaves
        # fewer splits than asked (K = 136 asked 3: kps = 64 -> 3 splits of 64, 64, 8; K = 72 asked 3: kps = 64 -> 2 splits)
        if bm:
            env3 = {"LIDBOX_GEMM16S_DMA": "%d,%d,%d,3" % (bm, bn, st)}
            T.append(_row("ROWS16S", "tile-%d.%d.%d-split3-short" % (bm, bn, st), "choose_dma16: forced splits = 3, last split short (K = 328: 128 + 128 + 72)",
                          "s", "nt", bn + 36, 328, _dense(bm + 1, 328), epi=ALL_EPIS[ti % 8], out=_form(ti, ALL_EPIS[ti % 8])[0], env=env3, ws="plan",
                          expect=dict(kernel=kern, tile=(bm, bn, st), splits=3, kps=128)))
            T.append(_row("ROWS16S", "tile-%d.%d.%d-split3-fewer" % (bm, bn, st), "choose_dma16: forced splits = 3 at K = 72: k_per_split rounds to 64 -> 2 splits",
                          "s", "nt", 36, 72, _dense(bm - 1, 72), epi=ALL_EPIS[(ti + 3) % 8], out=_form(ti + 1, ALL_EPIS[(ti + 3) % 8])[0], env=env3, ws="plan",
                          expect=dict(kernel=kern, tile=(bm, bn, st), splits=2, kps=64)))
    T.append(_row("ROWS16S", "split3-ws-short", "choose_dma16: a workspace one byte short of 3 M N floats steps the forced split down to 2", "s", "nt", 72, 328,
                  _dense(65, 328), epi=EPI_BIAS, out="both", env={"LIDBOX_GEMM16S_DMA": "64,64,2,3"}, ws="plan-1",
                  expect=dict(kernel=KS_DMA, tile=(64, 64, 2), splits=2, kps=192)))
    # 2. policy rows with no environment
    T.append(_row("ROWS16S", "policy-t128-small-split", "choose_dma16: t128 < NUM_CU / 2 -> 64 x 64 x 2, tiles < 2 NUM_CU -> automatic K split", "s", "nt", 72,
                  520, _dense(130, 520), epi=EPI_BIAS_RELU, out="both", ws="plan", expect=dict(kernel=KS_DMA, tile=(64, 64, 2), splits=3, kps=192, branch="t128_small")))
    T.append(_row("ROWS16S", "policy-t128-small-nosplit", "choose_dma16: t128 < NUM_CU / 2, K < 2 D16_BK -> max_s = 0, one split", "s", "nt", 72, 72,
                  _dense(130, 72), epi=EPI_RELU, out="shadow", ws="none", expect=dict(kernel=KS_DMA, tile=(64, 64, 2), splits=1, branch="t128_small")))
    T.append(_row("ROWS16S", "policy-t128-small-nows", "choose_dma16: the automatic K split without a workspace falls to one split", "s", "nt", 72, 520,
                  _dense(130, 520), epi=EPI_ACCUM, out="both", ws="none", expect=dict(kernel=KS_DMA, tile=(64, 64, 2), splits=1, branch="t128_small")))
    T.append(_row("ROWS16S", "policy-default", "choose_dma16: the default 64 x 128 x 2 (t128 = 128 = NUM_CU / 2, K < 512)", "s", "nt", 132, 72,
                  _dense(64 * 128 + 1 - 64, 72), epi=EPI_RELU_MASK, out="both", mask16=True, ws="none",
                  expect=dict(kernel=KS_DMA, tile=(64, 128, 2), branch="default_64x128")))
    T.append(_row("ROWS16S", "policy-just-over", "choose_dma16: just_over_a_round (769 tiles of 64 x 128) with K < 1536 -> 64 x 64 x 2", "s", "nt", 8, 72,
                  _dense(64 * 768 + 1, 72), epi=EPI_NONE, out="shadow", ws="none", expect=dict(kernel=KS_DMA, tile=(64, 64, 2), splits=1, branch="just_over_64x64")))
    # 3. the K-resident forward kernel: <13> (K = 200) and <0> (K = 16, 40, 208), forced; rows_per_batch in {1, 31, 32, 33, 65};
    #    more units than 12 streams and fewer; Cd.batch == 1 against the batched output form
    KR = {"LIDBOX_GEMM16S_KRES": "1"}
    for i, (K, rpb, batch) in enumerate(((200, 33, 3), (200, 1, 2), (16, 31, 3), (40, 32, 2), (208, 65, 14), (200, 65, 2), (40, 33, 1))):
        a = dict(batch=batch, rpb=rpb, rs=40 if K > 40 else 8, bs=(rpb + 7) * (40 if K > 40 else 8) + 0)
        a["bs"] = cdiv((rpb - 1) * a["rs"] + K, 8) * 8 + 8
        epi = (EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_RELU)[i % 4]
        cform = _batched(batch, rpb, 72, 4, 8) if i % 2 == 0 else _dense(batch * rpb, 72, 4)
        T.append(_row("ROWS16S", "kres-K%d-rpb%d-b%d" % (K, rpb, batch), "plan_rows16s: LIDBOX_GEMM16S_KRES=1, K = %d -> gemm16s_rows_kres_kernel<%s>; %s; %s C" %
                      (K, "13" if (K + 15) // 16 == 13 else "0", "units > 12 x streams" if batch * cdiv(rpb, 32) > 12 else "units < 12", "batched" if i % 2 == 0 else "flat"),
                      "s", "nt", 72, K, a, c=cform, epi=epi, out=("both", "shadow", "f32")[i % 3], env=KR, ws="none",
                      expect=dict(kernel=KS_KRES13 if (K + 15) // 16 == 13 else KS_KRES0)))
    # policy-selected (no environment): row_stride * 2 <= K and batch * tiles_n >= 2 NUM_CU
    for K, rs, rpb in ((200, 40, 3), (16, 8, 33)):
        a = dict(batch=2 * NUM_CU, rpb=rpb, rs=rs, bs=(rpb - 1) * rs + K + 8)
        T.append(_row("ROWS16S", "kres-policy-K%d" % K, "plan_rows16s: no environment, row_stride * 2 <= K and 512 utterances x 1 column tile -> gemm16s_rows_kres_kernel<%s>" %
                      ("13" if K == 200 else "0"), "s", "nt", 64, K, a, c=_batched(2 * NUM_CU, rpb, 64, 0, 8), epi=EPI_BIAS_RELU, out="both", ws="none",
                      expect=dict(kernel=KS_KRES13 if K == 200 else KS_KRES0)))
    a = dict(batch=2 * NUM_CU - 1, rpb=3, rs=40, bs=2 * 40 + 208)
    T.append(_row("ROWS16S", "kres-policy-511", "plan_rows16s: 511 utterances x 1 column tile < 2 NUM_CU -> not worth it, choose_dma16", "s", "nt", 64, 200, a,
                  c=_batched(2 * NUM_CU - 1, 3, 64, 0, 8), epi=EPI_BIAS_RELU, out="both", ws="plan", expect=dict(kernel=KS_DMA)))
    a = dict(batch=2 * NUM_CU, rpb=3, rs=104, bs=2 * 104 + 208)
    T.append(_row("ROWS16S", "kres-policy-rs", "plan_rows16s: row_stride * 2 > K (104 against 200) -> not worth it, choose_dma16", "s", "nt", 64, 200, a,
                  c=_batched(2 * NUM_CU, 3, 64, 0, 8), epi=EPI_BIAS_RELU, out="both", ws="plan", expect=dict(kernel=KS_DMA)))
    base = dict(a=dict(batch=3, rpb=33, rs=40, bs=33 * 40 + 200), K=200, N=72)
    for name, why, kw in (
            ("N%8", "c_ok: N % 8 != 0", dict(N=76)),
            # (of c_ok's terms, row_stride % 4, batch_stride % 4 and aligned16(Cd.base) are refused by rows_aligned before plan_rows16s
            #  is reached -- test_alignment_refusals_term_by_term; N % 8, the shadow's 8-byte alignment and the utterance structure remain)
            ("C16%8", "c_ok: the shadow 4 bytes off an 8-byte boundary (C's row_stride / batch_stride % 4 and base are rows_aligned's, refused before)",
             dict(res={"C16": 4})),
            ("Cbatch", "c_ok: C cut into utterances differently from A (9 x 11 against 3 x 33) and not flat", dict(c=_batched(9, 11, 72, 4, 8))),
            ("mask", "can: a bf16 mask", dict(epi=EPI_RELU_MASK, mask16=True)),
            ("epi", "epi_ok: an epilogue outside NONE / BIAS / BIAS_RELU / RELU", dict(epi=EPI_ACCUM)),
            ("rs-long", "kres_applies: 31 row strides + K beyond the 3 KB image", dict(a=dict(batch=3, rpb=33, rs=48, bs=33 * 48 + 200)))):
        kw = dict(kw)
        T.append(_row("ROWS16S", "kres-refuse-" + name, "plan_rows16s: %s -> falls back to choose_dma16" % why, "s", "nt", kw.pop("N", base["N"]), base["K"],
                      kw.pop("a", base["a"]), c=kw.pop("c", None), epi=kw.pop("epi", EPI_BIAS), out="both", env=KR, ws="plan", expect=dict(kernel=KS_DMA), **kw))
    return T


def _rows16_table():
    T = []
    # 4. the compute family: splits 1, 2 and the cap of 64; splits cut by the workspace down to 1; nt with N % 4 != 0 against nn
    for i, (M, N, K, ws, splits, why) in enumerate((
            (130, 132, 36, "lib", 1, "plan_rows16: K < 2 BK x 2 -> one split (K tail 4 behind a 32-deep step)"),
            (130, 132, 136, "lib", 2, "plan_rows16: max_s = K / 64 = 2 -> 2 splits, the last one short (96 + 40)"),
            (5, 8, 8192, "lib", 64, "plan_rows16: max_s = 128, s capped at 64 -> 64 splits of 128"),
            (130, 132, 264, "lib", 3, "plan_rows16: s = 4 asked, k_per_split rounds to 96 -> 3 splits (96 + 96 + 72)"),
            (130, 132, 264, "plan-1", 2, "plan_rows16: the workspace one byte short of 3 M N floats -> s = 2, 2 splits of 160 + 104"),
            (130, 132, 264, "one-1", 1, "plan_rows16: the workspace one byte short of 2 M N floats -> 1 split"),
            (130, 132, 264, "none", 1, "plan_rows16: no workspace -> 1 split"))):
        for kind in ("nn", "nt"):
            epi = (i * 2 + (kind == "nt")) % 8
            T.append(_row("ROWS16", "c-%s-%dx%dx%d-%s" % (kind, M, N, K, ws), why, "c", kind, N, K, _dense(M, K, 4),
                          c=_batched(2, M // 2, N, 4, 8) if M % 2 == 0 else _dense(M, N, 4), epi=epi, ws=ws, ldb_pad=4, expect=dict(kernel=K_ROWS, splits=splits)))
    T.append(_row("ROWS16", "c-nt-N%4", "rows16_operands_ok: nt allows N % 4 != 0", "c", "nt", 70, 72, _dense(65, 72), c=_dense(65, 70, 2), epi=EPI_BIAS, ws="none", expect=dict(kernel=K_ROWS)))
    T.append(_row("ROWS16", "c-nn-N%4", "rows16_operands_ok: nn refuses N % 4 != 0", "c", "nn", 70, 72, _dense(65, 72), c=_dense(65, 70, 2), epi=EPI_BIAS, ws="none",
                  expect=dict(kernel=K_REFUSED)))
    T.append(_row("ROWS16", "c-conv", "gemm16_rows_kernel: overlapping causal windows (k = 3, stride 2), batched C", "c", "nn", 72, 24, _conv(3, 40, 8, 3, 2),
                  c=_batched(3, 20, 72, 0, 0), epi=EPI_BIAS_RELU, ws="lib", expect=dict(kernel=K_ROWS)))
    return T


def _tn16_table():
    T = []
    for i, (M, K1, N, why) in enumerate(((100, 36, 40, "plan_tn16: max_s = cdiv(M, 128) = 1 -> one slice"),
                                         (300, 132, 136, "plan_tn16: 3 slices of 128, 128, 44 rows (the last not a multiple of 32)"),
                                         (1, 4, 4, "gemm16_tn_kernel: M = 1"))):
        T.append(_tn_row("TN16", "c-tn-%dx%dx%d" % (M, K1, N), why, "c", K1, N, _dense(M, K1, 4), b=_dense(M, N, 4), accumulate=i % 2, bias_grad=i != 2, ldc_pad=4 * (i % 2),
                         expect=dict(kernel=K_TN)))
    T.append(_tn_row("TN16", "c-tn-conv", "gemm16_tn_kernel: conv-window A, stride 2", "c", 48, 64, _conv(4, 50, 16, 3, 2), accumulate=1, expect=dict(kernel=K_TN)))
    return T


def _tn16s_table():
    T = []
    PP1, KR1 = {"LIDBOX_GEMM16_TN_PP": "1"}, {"LIDBOX_GEMM16_TN_KRES": "1"}
    # 5. the four-wave kernel: splits 1 and 2; target NUM_CU at tiles <= 16; a last slice that is no multiple of 64
    T.append(_tn_row("TN16S", "s-tn-one", "plan_tn16: M < 256 -> one slice", "s", 40, 72, _dense(100, 40), b=_dense(100, 72), bias_grad=False, expect=dict(kernel=KS_TN, splits=1)))
    T.append(_tn_row("TN16S", "s-tn-two", "plan_tn16 (BK 64): 2 slices of 192 + 108 rows; the last slice is no multiple of 64", "s", 136, 72, _dense(300, 136), b=_dense(300, 72),
                     accumulate=1, expect=dict(kernel=KS_TN, splits=2, rps=192)))
    T.append(_tn_row("TN16S", "s-tn-target-cu", "plan_tn16 (BK 64): tiles = 16 -> target NUM_CU: 16 slices of 512 rows", "s", 512, 512, _dense(8192, 512), b=_dense(8192, 512),
                     accumulate=0, expect=dict(kernel=KS_TN, splits=16, rps=512)))
    T.append(_tn_row("TN16S", "s-tn-target-2cu", "plan_tn16 (BK 64): tiles = 20 -> target 2 NUM_CU: s = 25, 22 slices of 384 rows", "s", 512, 640, _dense(8192, 512),
                     b=_dense(8192, 640), accumulate=1, bias_grad=False, expect=dict(kernel=KS_TN, splits=22, rps=384)))
    T.append(_tn_row("TN16S", "s-tn-pad8", "width_ok: K1 = 20 and N = 36 inside rows padded to 8 (24 / 40 wide, NaN in the pad columns)", "s", 20, 36,
                     _dense(100, 20, 4), b=_dense(100, 36, 4), accumulate=0, expect=dict(kernel=KS_TN, reduce=R_JOB4)))
    T.append(_tn_row("TN16S", "s-tn-ldc-odd", "reduce_job_vec_ok: ldc % 4 != 0 -> splitk_reduce_kernel, job.nblocks == 0", "s", 40, 72, _dense(300, 40), b=_dense(300, 72),
                     ldc_pad=3, accumulate=1, expect=dict(kernel=KS_TN, reduce=R_SCALAR)))
    T.append(_tn_row("TN16S", "s-tn-c-mis", "reduce_job_vec_ok: Cm 4 bytes off a 16-byte boundary -> scalar reduce", "s", 40, 72, _dense(300, 40), b=_dense(300, 72),
                     res={"C": 4}, expect=dict(kernel=KS_TN, reduce=R_SCALAR)))
    T.append(_tn_row("TN16S", "s-tn-conv", "gemm16s_tn_kernel: conv-window A (k = 5, stride 1), batched dY", "s", 40, 128, _conv(4, 50, 8, 5, 1), b=_batched(4, 50, 128, 0, 8),
                     accumulate=0, expect=dict(kernel=KS_TN)))
    # the ping-pong tile forced, and each of its descriptor conditions failing alone
    T.append(_tn_row("TN16S", "s-tn-pp", "plan_tn16_pp: LIDBOX_GEMM16_TN_PP=1 -> gemm16s_tn_pp_kernel, 2 slices of 128 + 72 rows, ragged tile (K1 = 40, N = 72)", "s", 40, 72,
                     _dense(200, 40), b=_dense(200, 72), env=PP1, accumulate=1, expect=dict(kernel=KS_TN_PP, splits=2, rps=128)))
    T.append(_tn_row("TN16S", "s-tn-pp-batched", "plan_tn16s: same utterances on both sides -> the ping-pong tile on batched operands", "s", 40, 72,
                     _conv(4, 50, 8, 5, 1), b=_batched(4, 50, 72, 0, 8), env=PP1, expect=dict(kernel=KS_TN_PP)))
    T.append(_tn_row("TN16S", "s-tn-pp-K1%8", "plan_tn16s: K1 % 8 != 0 (rows padded to 8) -> the four-wave kernel", "s", 20, 72, _dense(200, 20, 4), b=_dense(200, 72), env=PP1,
                     expect=dict(kernel=KS_TN)))
    T.append(_tn_row("TN16S", "s-tn-pp-N%8", "plan_tn16s: N % 8 != 0 -> the four-wave kernel", "s", 40, 36, _dense(200, 40), b=_dense(200, 36, 4), env=PP1, expect=dict(kernel=KS_TN)))
    T.append(_tn_row("TN16S", "s-tn-pp-utts", "plan_tn16s: utterance lengths differ between the operands -> the four-wave kernel", "s", 40, 72, _batched(4, 50, 40, 0, 8),
                     b=_batched(2, 100, 72, 0, 8), env=PP1, expect=dict(kernel=KS_TN)))
    # the K1-resident kernel forced: batch < max_slices, ups > 1, each desc_ok condition failing alone, a workspace too small for it
    T.append(_tn_row("TN16S", "s-tn-kres", "plan_tn16_kres: LIDBOX_GEMM16_TN_KRES=1, batch 5 < max_slices 256 -> 5 slices of one utterance", "s", 200, 128,
                     _conv(5, 70, 40, 5, 1), b=_batched(5, 70, 128, 0, 0), env=KR1, accumulate=1, expect=dict(kernel=KS_TN_KRES, splits=5, ups=1)))
    T.append(_tn_row("TN16S", "s-tn-kres-ups", "plan_tn16s: N = 4096 -> max_slices 8 < batch 19 -> ups = 3, 7 slices", "s", 16, 4096,
                     _conv(19, 9, 8, 2, 1), b=_batched(19, 9, 4096, 0, 0), env=KR1, expect=dict(kernel=KS_TN_KRES, splits=7, ups=3)))
    for name, why, a, b in (
            ("rpb", "rows_per_batch differ", _conv(4, 70, 40, 5, 1), _batched(5, 56, 128, 0, 0)),
            ("bs-whole", "batch_stride no whole number of row strides", dict(batch=4, rpb=70, rs=40, bs=74 * 40 - 8), _batched(4, 70, 128, 0, 0)),
            ("bs-covers", "batch_stride / row_stride < rows_per_batch", dict(batch=4, rpb=70, rs=40, bs=40 * 40), _batched(4, 70, 128, 0, 0)),
            ("img", "63 row strides + K1 beyond the stage image", dict(batch=4, rpb=70, rs=64, bs=72 * 64), _batched(4, 70, 128, 0, 0))):
        T.append(_tn_row("TN16S", "s-tn-kres-refuse-" + name, "plan_tn16s: desc_ok false by %s -> the four-wave kernel" % why, "s", 200, 128, a, b=b, env=KR1,
                         expect=dict(kernel=KS_TN)))
    T.append(_tn_row("TN16S", "s-tn-kres-ws", "plan_tn16s: a workspace too small for 5 utterance slices but enough for plan_tn16's 2 -> the four-wave kernel", "s", 200, 128,
                     _conv(5, 70, 40, 5, 1), b=_batched(5, 70, 128, 0, 0), env=KR1, ws="fallback", expect=dict(kernel=KS_TN, splits=2)))
    return T


def _carry16s_table():
    """lidbox_gemm_bf16s_tn_partial -> lidbox_gemm_bf16s_nt_carry: `jobs` pending jobs (w: a wgrad's slice sum, z: a zero job)"""
    T = []
    for name, why, jobs, env, carried, kw in (
            ("carry-1", "launch_rows16s: one pending job in the leading workgroups", "w", {}, 1, {}),
            ("carry-2", "pack_carry: a wgrad reduce and a zero job share the leading workgroups", "wz", {}, 2, {}),
            ("carry-off", "LIDBOX_GEMM_NO_CARRY: the jobs run as a launch of their own", "wz", {"LIDBOX_GEMM_NO_CARRY": "1"}, 0, {}),
            ("carry-blocks-7", "carry_cap16: LIDBOX_GEMM_CARRY_BLOCKS=7 is ignored", "w", {"LIDBOX_GEMM_CARRY_BLOCKS": "7"}, 1, {}),
            ("carry-blocks-8", "carry_cap16: LIDBOX_GEMM_CARRY_BLOCKS=8", "wz", {"LIDBOX_GEMM_CARRY_BLOCKS": "8"}, 2, {}),
            ("carry-M0", "launch_rows16s: M == 0 with jobs pending -> the jobs alone", "w", {}, 1, dict(M=0)),
            ("carry-zero-nows", "lidbox_gemm_bf16s_nt_carry: a zero job (P == NULL) with workspace == NULL is not `slices in this workspace`", "z", {}, 1,
             dict(nows=True)),
            ("carry-reg", "gemm16s_rows_kernel: the register-staged kernel carries", "wz", {"LIDBOX_GEMM16S_DMA": "0"}, 2, {}),
            ("carry-kres", "plan_rows16s: a carried job alone keeps a call off the K-resident kernel (LIDBOX_GEMM16S_KRES=1, K = 64; without the job it runs there)", "w",
             {"LIDBOX_GEMM16S_KRES": "1"}, 1, dict(kres=True))):
        T.append(dict(table="CARRY16S", name=name, why=why, kind="carry", jobs=jobs, env=dict(env), carried=carried, M=kw.get("M", 192), Co=64, N=96, K1=40, Mw=300,
                      nows=kw.get("nows", False), kres=kw.get("kres", False)))
    return T


def _convert_table():
    T = []
    for n in (0, 1, 3, 4, 5, 1023, 4096 * 256 * 4 + 3):
        T.append(dict(table="CONVERT", name="cvt-%d" % n, why="f32_to_bf16_kernel / bf16_to_f32_kernel: n = %d%s" % (n, " (past the 4096-block grid cap, n % 4 != 0)" if n > 1 << 20 else ""),
                      kind="convert", n=n))
    for R in (1, 31, 32, 33):
        for C in (1, 31, 32, 33):
            T.append(dict(table="CONVERT", name="tr-%dx%d" % (R, C), why="transpose_f32_to_bf16_kernel: R = %d, C = %d, pitched ld_src / ld_dst" % (R, C), kind="transpose",
                          R=R, C=C, ld_src=C + 3, ld_dst=R + 5))
    # lidbox_refresh_bf16_weights: mats = [(rows, cols, offset, ld_dst pad, transpose, dst shift in elements)]; vec needs cols % 4, offset % 4,
    # ld_dst % 4, dst 8-byte aligned and, transposed, rows % 4: all hold, then each fails alone, plain and transposed
    vec_ok = (8, 12, 0, 0, 0, 0)
    fails = [("cols", (8, 10, 0, 2, 0, 0)), ("offset", (8, 12, 2, 0, 0, 0)), ("ld_dst", (8, 12, 0, 2, 0, 0)), ("dst", (8, 12, 0, 0, 0, 2)), ("rows", (6, 12, 0, 2, 1, 0))]
    for tr in (0, 1):
        T.append(dict(table="CONVERT", name="refresh-vec-t%d" % tr, why="refresh_bf16_weights_kernel: vec on, %s; flat16 set, n %% 4 != 0" % ("transposed" if tr else "plain"),
                      kind="refresh", flat16=True, n_extra=3, mats=[vec_ok[:4] + (tr, 0), (65, 132, 0, 4, tr, 0)]))
        for name, m in fails:
            if name == "rows" and not tr:
                continue
            mm = m[:4] + (tr, m[5]) if name != "rows" else m
            T.append(dict(table="CONVERT", name="refresh-novec-%s-t%d" % (name, tr), why="refresh_bf16_weights_kernel: vec off by %s alone, %s" % (name, "transposed" if tr else "plain"),
                          kind="refresh", flat16=bool(tr), n_extra=0 if name != "offset" else 2, mats=[mm]))
    T.append(dict(table="CONVERT", name="refresh-flat-only", why="lidbox_refresh_bf16_weights: no matrices, only the flat conversion; n = 1021", kind="refresh", flat16=True, n_extra=1021, mats=[]))
    T.append(dict(table="CONVERT", name="refresh-49", why="lidbox_refresh_bf16_weights: 49 matrices take a second launch (MAX_WT = 48); flat16 NULL; padded ld_dst", kind="refresh",
                  flat16=False, n_extra=1, mats=[(5 + i % 3, 4 + 4 * (i % 2), 0, 4, i % 2, 0) for i in range(49)]))
    return T


def refresh_layout(r):
    """(n, [dict(offset, rows, cols, ld_dst, transpose, dst_shift, vec)]) of a refresh row: the matrices one behind the other in the flat
    vector, each at an offset that is a multiple of 4 plus its own shift"""
    mats, off = [], 0
    for rows, cols, oshift, ldpad, tr, dshift in r["mats"]:
        off = cdiv(off, 4) * 4 + oshift
        ld = (rows if tr else cols) + ldpad
        vec = cols % 4 == 0 and off % 4 == 0 and ld % 4 == 0 and dshift % 4 == 0 and (not tr or rows % 4 == 0)
        mats.append(dict(offset=off, rows=rows, cols=cols, ld_dst=ld, transpose=tr, dst_shift=dshift, vec=vec))
        off += rows * cols
    return off + r["n_extra"], mats


def _big16s_table():
    """rows too large for a whole-matrix float64 reference on every case: judged on sample_rows (first / last row of the 256-row tiles
    at both ends of M, the rows around a tail split's m_main, 64 random rows) against float64, and bit for bit against the same call
    under the forced variant (`twin_env`) or, for the tail split, against a call cut at m_main by hand.  The CPU mutation check
    runs on the small forced rows of the same kernels."""
    T = []
    PPF = {"LIDBOX_GEMM16S_DMA": "256,256,2"}
    def big(name, why, M, N, K, epi, out, expect, fam="s", mask16=False, env=None, twin=None, ws="none", ds=None):
        r = _row("BIG16S", name, why, fam, "nt", N, K, _dense(M, K), epi=epi, out=out, mask16=mask16, env=env, ws=ws, expect=expect)
        r["twin_env"], r["ds"] = twin, ds
        return r
    # choose_dma16 by policy: both ping-pong conditions, the writes_fp32 exception on each side, just_over_a_round with K >= 1536
    T.append(big("policy-pp-3q", "choose_dma16: K >= 512 and 192 tiles of 256 x 256 (3/4 of a round) -> the ping-pong tile; fp32 + shadow (t256 <= NUM_CU: no exception)",
                 24576, 512, 512, EPI_RELU_MASK, "both", dict(kernel=KS_PP, tile=(256, 256, 2), splits=1, branch="pp_three_quarters"), mask16=True, twin=PPF))
    T.append(big("policy-pp-3q-less", "choose_dma16: 191 tiles of 256 x 256, K = 512 -> not the ping-pong tile (default 64 x 128)", 24576 - 256, 512, 512, EPI_BIAS,
                 "shadow", dict(kernel=KS_DMA, tile=(64, 128, 2), splits=1, branch="default_64x128"), twin={"LIDBOX_GEMM16S_DMA": "64,128,2"}))
    T.append(big("policy-pp-half", "choose_dma16: K >= 1500 and 128 tiles (half a round) -> the ping-pong tile", 16384, 512, 1504, EPI_ACCUM_RELU, "both",
                 dict(kernel=KS_PP, tile=(256, 256, 2), splits=1, branch="pp_half_round"), twin=PPF))
    T.append(big("policy-pp-half-K", "choose_dma16: the same 128 tiles at K = 1496 < 1500 -> default 64 x 128", 16384, 512, 1496, EPI_ACCUM_RELU, "both",
                 dict(kernel=KS_DMA, tile=(64, 128, 2), splits=1, branch="default_64x128"), twin={"LIDBOX_GEMM16S_DMA": "64,128,2"}))
    T.append(big("policy-fp32-exception", "choose_dma16: writes_fp32 && K < 1024 && t256 = 384 > NUM_CU -> stays on the small tiles", 49152, 512, 512, EPI_BIAS_RELU, "both",
                 dict(kernel=KS_DMA, tile=(64, 128, 2), splits=1, branch="default_64x128"), twin={"LIDBOX_GEMM16S_DMA": "64,128,2"}))
    T.append(big("policy-fp32-exception-shadow", "choose_dma16: the same call shadow only (writes_fp32 false) -> the ping-pong tile", 49152, 512, 512, EPI_BIAS_RELU,
                 "shadow", dict(kernel=KS_PP, tile=(256, 256, 2), splits=1, branch="pp_three_quarters"), twin=PPF))
    T.append(big("policy-fp32-exception-K1024", "choose_dma16: the same call with fp32 C at K = 1024 -> the ping-pong tile", 49152, 512, 1024, EPI_BIAS_RELU, "both",
                 dict(kernel=KS_PP, tile=(256, 256, 2), splits=1, branch="pp_three_quarters"), twin=PPF, ds="normal"))
    T.append(big("policy-k1536", "choose_dma16: just_over_a_round (770 tiles of 64 x 128) with K >= 1536 -> 128 x 128 x 2", 24577, 256, 1536, EPI_NONE, "shadow",
                 dict(kernel=KS_DMA, tile=(128, 128, 2), splits=1, branch="k1536_128x128"), twin={"LIDBOX_GEMM16S_DMA": "128,128,2"}, ds="offset"))
    # the tail split (plan_tail16) on and off at TAIL_MIN_K, at rem_tiles == slots / 4 and one more; both families
    K0 = _c("TAIL_MIN_K")
    REG = {"LIDBOX_GEMM16S_DMA": "0"}
    for fam, env in (("s", REG), ("c", {})):
        M = 512 * 128 + 1
        T.append(big("tail-%s-on" % fam, "plan_tail16: 513 row tiles, K = TAIL_MIN_K -> m_main = 65536, the one remaining row split 16 (32-deep steps) or 8 (64-deep) ways", M, 8, K0, EPI_BIAS, "f32",
                     dict(kernel=KS_ROWS if fam == "s" else K_ROWS, splits=1, m_main=65536, rem_splits=8 if fam == "s" else 16), fam=fam, env=env, ws="tail", ds="normal"))
        T.append(big("tail-%s-K" % fam, "plan_tail16: K = TAIL_MIN_K - 8 -> one launch", M, 8, K0 - 8, EPI_BIAS, "f32",
                     dict(kernel=KS_ROWS if fam == "s" else K_ROWS, splits=1, m_main=0), fam=fam, env=env, ws="tail", ds="offset"))
        T.append(big("tail-%s-nows" % fam, "plan_tail16: no workspace -> the remainder cannot split -> one launch", M, 8, K0, EPI_BIAS, "f32",
                     dict(kernel=KS_ROWS if fam == "s" else K_ROWS, splits=1, m_main=0), fam=fam, env=env, ws="none", ds="exact"))
    T.append(big("tail-s-quarter", "plan_tail16: rem_tiles == slots / 4 = 128 -> taken, 16 384 remaining rows split 4 ways", 640 * 128, 8, K0, EPI_ACCUM, "both",
                 dict(kernel=KS_ROWS, splits=1, m_main=65536, rem_splits=4), env=REG, ws="tail", ds="exact"))
    T.append(big("tail-s-quarter+1", "plan_tail16: rem_tiles == slots / 4 + 1 -> one launch", 641 * 128, 8, K0, EPI_ACCUM, "both",
                 dict(kernel=KS_ROWS, splits=1, m_main=0), env=REG, ws="tail", ds="normal"))
    T.append(big("tail-c-quarter", "plan_tail16 (compute family): rem_tiles == slots / 4 = 128 -> taken, 16 384 remaining rows split 4 ways", 640 * 128, 8, K0, EPI_ACCUM,
                 "f32", dict(kernel=K_ROWS, splits=1, m_main=65536, rem_splits=4), fam="c", ws="tail", ds="offset"))
    T.append(big("tail-c-quarter+1", "plan_tail16 (compute family): rem_tiles == slots / 4 + 1 -> one launch", 641 * 128, 8, K0, EPI_ACCUM, "f32",
                 dict(kernel=K_ROWS, splits=1, m_main=0), fam="c", ws="tail", ds="exact"))
    return T


def _pair16s_table():
    """lidbox_gemm_bf16s_nt_pair_carry: two problems (BIG16S-style rows p0, p1: judged on sample_rows, and bit for bit against the two
    calls one after the other).  pair: lidbox_gemm_bf16s_last_pair; zero: a zero job rides along; nows: workspace == NULL"""
    T = []
    def prob(name, M, K, epi, out, env, a=None):
        return _row("PAIR16S", name, "a problem of a pair", "s", "nt", 512, K, _dense(M, K) if a is None else a, epi=epi, out=out, env=env, ws="none")
    for name, why, K0, K1, M1, env, pair, zero, ws in (
            ("pair", "pp2_problem true twice, the deeper contraction first in the call: swap = false", 576, 512, 24576, {}, True, False, False),
            ("pair-swap", "pp2_problem true twice, the deeper contraction second: swap = true", 512, 576, 24576, {}, True, False, False),
            ("pair-zero-nows", "a zero job (P == NULL) with workspace == NULL is in order: one grid that carries it", 576, 512, 24576, {}, True, True, False),
            ("pair-small", "pp2_problem: the second problem has 191 tiles (not the ping-pong tile) -> two calls", 576, 512, 24576 - 256, {}, False, False, False),
            ("pair-split", "pp2_problem: a forced K split of 2 with a workspace (dc.splits != 1) -> two calls", 576, 512, 24576,
             {"LIDBOX_GEMM16S_DMA": "256,256,2,2"}, False, False, True),
            ("pair-nocarry", "LIDBOX_GEMM_NO_CARRY -> two calls", 576, 512, 24576, {"LIDBOX_GEMM_NO_CARRY": "1"}, False, True, False)):
        p0 = prob(name + "-p0", 24576, K0, EPI_BIAS, "both", env)
        p1 = prob(name + "-p1", M1, K1, EPI_BIAS_RELU, "shadow", env)
        p1["first_epi"] = EPI_BIAS
        T.append(dict(table="PAIR16S", name=name, why=why, kind="pair", p0=p0, p1=p1, env=dict(env), pair=pair, zero=zero, ws=ws))
    # `!mask16 && kres_applies`: windows the K-resident forward kernel may take (K = 200, row stride 8, 64 utterances x 8 column tiles: it
    # does take them, by policy) under a forced ping-pong tile -- every other term of pp2_problem holds
    env = {"LIDBOX_GEMM16S_DMA": "256,256,2"}
    win = dict(batch=64, rpb=33, rs=8, bs=32 * 8 + 200 + 8)
    p0, p1 = prob("pair-kres-p0", 64 * 33, 200, EPI_BIAS, "both", env, a=win), prob("pair-kres-p1", 64 * 33, 200, EPI_BIAS_RELU, "shadow", env, a=win)
    p1["first_epi"] = EPI_BIAS
    T.append(dict(table="PAIR16S", name="pair-kres", why="pp2_problem: kres_applies without a bf16 mask (the K-resident forward kernel may take it) -> two calls, both on that kernel",
                  kind="pair", p0=p0, p1=p1, env=env, pair=False, zero=True, ws=False))
    # M == 0: the second problem has no rows -> two calls, the second of which does nothing
    p0, p1 = prob("pair-empty-p0", 24576, 576, EPI_BIAS, "both", {}), prob("pair-empty-p1", 4, 512, EPI_BIAS_RELU, "shadow", {})
    p1["first_epi"], p1["empty"] = EPI_BIAS, True
    T.append(dict(table="PAIR16S", name="pair-empty", why="pp2_problem: M == 0 in the second problem -> two calls, the second writes nothing", kind="pair", p0=p0, p1=p1,
                  env={}, pair=False, zero=True, ws=False))
    return T


def _bigtn16s_table():
    """wgrads judged on 64 sampled output columns (and the whole bias gradient)"""
    T = []
    T.append(_tn_row("BIGTN16S", "s-tn-pp-policy", "plan_tn16_pp by policy: 64 full tiles of 256 x 256, 4 slices of 2 048 rows (tiles x slices = 256)", "s", 2048, 2048,
                     _dense(8192, 2048), b=_dense(8192, 2048), accumulate=0, expect=dict(kernel=KS_TN_PP, splits=4, rps=2048)))
    T.append(_tn_row("BIGTN16S", "s-tn-pp-policy-short", "plan_tn16_pp by policy: the same tiles with 128 rows fewer -> slices of 2 016 < 2 048 rows -> the four-wave kernel", "s",
                     2048, 2048, _dense(8192 - 128, 2048), b=_dense(8192 - 128, 2048), accumulate=1, bias_grad=False, expect=dict(kernel=KS_TN)))
    return T


PATHS = dict(ROWS16=_rows16_table(), TN16=_tn16_table(), ROWS16S=_rows16s_table(), TN16S=_tn16s_table(), PAIR16S=_pair16s_table(),
             CARRY16S=_carry16s_table(), CONVERT=_convert_table(), BIG16S=_big16s_table(), BIGTN16S=_bigtn16s_table())

def _far16_table():
    """rows on both sides of every 32-bit-extent term of the storage planners, found by stretching one stride ('bs', 'rs' or 'ldb') of
    a small problem into a zone (gp.ZONES) of the term's own expression.  far: operand -> stride; term: the limit of limits16();
    expect: the kernel the restated planner and the export must name."""
    T = []
    L = limits16()
    # two utterances one after the other: the second starts behind the last window of the first
    pair = lambda rpb, w, rs=None: dict(batch=2, rpb=rpb, rs=w if rs is None else rs, bs=cdiv((rpb - 1) * (w if rs is None else rs) + w, 8) * 8)

    def solve(mk, g, term, zone, step=8, lo=8):
        return mk(gp._solve(lambda s: g(mk(s)), L[term], zone, step=step, lo=lo))

    # rows: the LDS-DMA tile (the policy's own 64 x 64 x 2), the ping-pong tile (forced 256 x 128 x 2), the K-resident kernel
    # (LIDBOX_GEMM16S_KRES=1)
    for kname, kern, env, a0, N, K in (("dma", KS_DMA, {}, pair(65, 64), 64, 64),
                                       ("pp", KS_PP, {"LIDBOX_GEMM16S_DMA": "256,128,2"}, pair(129, 64), 64, 64),
                                       ("kres0", KS_KRES0, {"LIDBOX_GEMM16S_KRES": "1"}, pair(65, 40, 8), 64, 40)):
        term = "a_span" if kern == KS_KRES0 else "a_ext"
        for zone in ("over", "edge-out", "edge-in", "high"):
            a = solve(lambda s: dict(a0, bs=s), lambda d: a_ext16(d, K), term, zone, lo=a0["bs"])
            fast = zone in ("high", "edge-in")
            T.append(_row("FAR16", "far16-%s-A-bs-%s" % (kname, zone), "plan_rows16s: %s %s %.1e by batch_stride (%s)" % (term, "<" if fast else ">=", L[term], zone),
                          "s", "nt", N, K, a, c=_batched(2, a0["rpb"], N), env=env, ws="plan", zone=zone, far={"A": "bs"}, term=term,
                          expect=dict(kernel=kern if fast else None, not_kernel=None if fast else kern)))
    # the K-resident kernel's per-utterance limit: one utterance of 1.25e8 windows 8 elements apart (planner only: no device could
    # hold its C); the total a_span stays below its own limit
    for zone in ("over", "edge-out", "edge-in", "high"):
        mk = lambda s: dict(batch=1, rpb=s, rs=8, bs=0)
        a = solve(mk, lambda d: a_utt16(d, 40), "a_utt", zone, step=1, lo=1)
        fast = zone in ("high", "edge-in")
        T.append(_row("FAR16", "far16-kres0-A-utt-%s" % zone, "plan_rows16s: the per-utterance term of `can` %s %.1e (%s)" % ("<" if fast else ">=", L["a_utt"], zone),
                      "s", "nt", 64, 40, a, env={"LIDBOX_GEMM16S_KRES": "1"}, ws="none", zone=zone, far={"A": "rpb"}, term="a_utt", planner_only=True,
                      expect=dict(kernel=KS_KRES0 if fast else None, not_kernel=None if fast else KS_KRES0)))
    # b_ext by ldb on the LDS-DMA tile
    for zone in ("over", "edge-out", "edge-in", "high"):
        ldb = gp._solve(lambda s: b_ext16(64, s, 64), L["b_ext"], zone, step=8, lo=64)
        fast = zone in ("high", "edge-in")
        T.append(_row("FAR16", "far16-dma-B-ldb-%s" % zone, "plan_rows16s: b_ext %s %.1e by ldb (%s)" % ("<" if fast else ">=", L["b_ext"], zone), "s", "nt", 64, 64,
                      _dense(130, 64), env={}, ws="plan", ldb_pad=ldb - 64, zone=zone, far={"B": "ldb"}, term="b_ext",
                      expect=dict(kernel=KS_DMA if fast else KS_ROWS, not_kernel=None if fast else KS_DMA)))
    # wgrads: the ping-pong tile (LIDBOX_GEMM16_TN_PP=1) and the K1-resident kernel (LIDBOX_GEMM16_TN_KRES=1), span_ok on either operand
    for kname, kern, env, rpb, K1, N, rs in (("tn_pp", KS_TN_PP, {"LIDBOX_GEMM16_TN_PP": "1", "LIDBOX_GEMM16_TN_KRES": "0"}, 512, 64, 64, 64),
                                             ("tn_kres", KS_TN_KRES, {"LIDBOX_GEMM16_TN_KRES": "1", "LIDBOX_GEMM16_TN_PP": "0"}, 64, 40, 128, 8)):
        for op in ("A", "B"):
            for zone in ("over", "edge-out", "edge-in", "high"):
                a0, b0 = pair(rpb, K1, rs), pair(rpb, N)
                w = K1 if op == "A" else N
                step = rs if (kern == KS_TN_KRES and op == "A") else 8          # the K1-resident kernel: utterances whole row strides apart
                far = solve(lambda s: dict(a0 if op == "A" else b0, bs=s), lambda d: span16(d, w), "span", zone, step=step, lo=(a0 if op == "A" else b0)["bs"])
                a, b = (far, b0) if op == "A" else (a0, far)
                fast = zone in ("high", "edge-in")
                why = "plan_tn16s: span_ok(%s) %s by batch_stride (%s)" % (op, "true" if fast else "false", zone)
                if kern == KS_TN_KRES and op == "A":
                    # the K1-resident kernel reads every element between two utterances' first windows: a stretched batch stride of
                    # its A leaves elements no window covers and is refused (gap_covered) on both sides of span_ok's limit
                    fast, why = False, why + "; gap_covered false first -> the four-wave kernel"
                T.append(_tn_row("FAR16", "far16-%s-%s-bs-%s" % (kname, op, zone), why, "s", K1, N, a, b=b, env=env, zone=zone, far={op: "bs"}, term="span",
                                 twin_same=fast, expect=dict(kernel=kern if fast else KS_TN, not_kernel=None if fast else kern)))
    # the K1-resident kernel's own gap term at its edge: the next utterance begins where the windows of this one end / one row stride on
    for name, extra, fast in (("in", 0, True), ("out", 8, False)):
        a = dict(batch=2, rpb=64, rs=8, bs=63 * 8 + 40 + extra)
        T.append(_tn_row("FAR16", "far16-tn_kres-gap-" + name, "plan_tn16s: batch_stride %s rpb rs + K1 -> %s" % ("<" if fast else "==", "K1-resident" if fast else "four-wave"),
                         "s", 40, 128, a, b=pair(64, 128), env={"LIDBOX_GEMM16_TN_KRES": "1", "LIDBOX_GEMM16_TN_PP": "0"}, zone="edge-in" if fast else "edge-out",
                         far={}, term="gap", twin_same=fast, expect=dict(kernel=KS_TN_KRES if fast else KS_TN, not_kernel=None if fast else KS_TN_KRES)))
    return T


PATHS["FAR16"] = _far16_table()


def far16_pair_calls():
    """pp2_problem's a_ext / b_ext (the second site): a call that joins a two-problem grid, then stretched over either limit alone"""
    M, N, K = 256 * 192, 256, 512
    base = dict(a=_dense(M, K), c=_dense(M, N), K=K, N=N, epi=EPI_NONE, ldb=K)
    L = limits16()
    out = [("far16-pair-in", base, True)]
    for zone in ("edge-in", "edge-out", "over"):
        rs = gp._solve(lambda s: a_ext16(dict(batch=1, rpb=M, rs=s, bs=0), K), L["pair_a_ext"], zone, step=8, lo=K)
        out.append(("far16-pair-A-rs-%s" % zone, dict(base, a=dict(batch=1, rpb=M, rs=rs, bs=0)), zone == "edge-in"))
        ldb = gp._solve(lambda s: b_ext16(N, s, K), L["pair_b_ext"], zone, step=8, lo=K)
        out.append(("far16-pair-B-ldb-%s" % zone, dict(base, ldb=ldb), zone == "edge-in"))
    return out


# policy branches no row selects, with the reason
UNREACHED = [
    dict(what="choose_dma16: `t128 >= 3 * NUM_CU` in the K >= 1536 branch",
         why="contradicts the ping-pong test above it: t128 <= 4 t256, so t128 >= 768 gives t256 >= 192, and with K >= 1536 >= 1500 the "
             "second ping-pong condition 2 t256 >= r256 NUM_CU holds for every such t256 (r256 = 1: 384 >= 256; r256 >= 2: t256 > "
             "(r256 - 1) 256 gives 2 t256 > r256 256).  The branch is only entered through just_over_a_round (row policy-k1536)."),
    dict(what="pp2_problem: the shadow-only, mask-flag, validate_rows_call and alignment terms failing alone with `the same bits as two calls`",
         why="each of them is a test lidbox_gemm_bf16s_nt_carry makes too (C.base == NULL needs the shadow and a non-accumulating epilogue; "
             "LIDBOX_EPI_MASK_BF16 goes with a ReLU-mask epilogue; validate_rows_call; rows16s_operands_ok), so the two-call path the pair "
             "entry falls back to refuses the same call: there are no two results to compare.  The terms that can fail alone and still run "
             "have rows: M == 0 (pair-empty), kres_applies (pair-kres), the tile / split (pair-small, pair-split); a_ext / b_ext: FAR16 "
             "(far16-pair-*, pinned on the CPU through pp2_conditions)."),
    dict(what="plan_rows16s: a bf16 mask as the ONLY failing condition of the K-resident `can`",
         why="LIDBOX_EPI_MASK_BF16 is accepted with a ReLU-mask epilogue only, and epi_ok refuses those epilogues: the two fail together "
             "(row kres-refuse-mask)"),
]


def shadow_through_vector_store(r, q):
    """whether a rows launch writes shadow values through the 16-byte path of pp_store_tile (gemm16_pp.h): what a device build that
    truncates in that store changes.  The path serves the ping-pong tiles, and the LDS-DMA tiles with 128 columns under the
    epilogues that read per element; unsplit launches only (a split's shadow is rows_reduce_kernel's); every whole 8-column chunk
    of a row, in the strips wholly inside the matrix and in the edge strips alike; C, shadow and mask laid out for vector accesses"""
    c = r["c"]
    if r["out"] == "f32" or q[4] != 1 or r["N"] < 8:
        return False
    if c["rs"] % 4 or (c["batch"] != 1 and c["bs"] % 4) or r["res"].get("C16", 0) % 8 or r["res"].get("C", 0):
        return False
    if q[0] == KS_PP:
        return True
    return q[0] == KS_DMA and q[2] == 128 and r["epi"] in (EPI_RELU_MASK, EPI_ACCUM_RELU_MASK, EPI_ACCUM, EPI_ACCUM_RELU)


def smallest_tail_split(fam):
    """the smallest (M, N, K) for which plan_tail16 cuts a launch, by the restated planner: N = 8 (one column of tiles)"""
    BK, slots = (32, 2 * NUM_CU) if fam == "c" else (_c("BKS"), _c("WAVES_S") * NUM_CU)
    K = _c("TAIL_MIN_K")
    for M in range(slots * 128 + 1, slots * 128 + 130):
        pl = plan_rows16(M, 8, K, 1 << 40, BK)
        if plan_tail16(pl, M, 8, K, 1 << 40, BK, slots)[0]:
            return M, 8, K
    return None


# ------------------------------------------------------------------------------------------------ rows -> calls
def row_ws_bytes(r):
    """the workspace a rows call gets: 'none'; 'lib' lidbox_gemm_bf16_rows_workspace; 'plan' what the row's plan needs with room to
    spare asked (the splits it would take with an unbounded workspace); 'plan-1' one byte short of that; 'one-1' one byte short of 2 M N floats"""
    M, N, K, ws = r["M"], r["N"], r["K"], r["ws"]
    if ws == "none":
        return 0
    if ws == "lib":
        return rows_workspace16(M, N, K)
    if ws.startswith("one"):
        return 2 * M * N * 4 - 1
    if ws == "tail":                                                # what the remainder of a tail split needs: a split of the rows behind the last whole round
        BK, slots = (32, 2 * NUM_CU) if r["fam"] == "c" else (_c("BKS"), _c("WAVES_S") * NUM_CU)
        m_main, rp = plan_tail16((1, K), M, N, K, 1 << 40, BK, slots)
        return rp[0] * (M - m_main) * N * 4 if m_main else 64
    if r["fam"] == "c":
        need = plan_rows16(M, N, K, 1 << 40)[0] * M * N * 4
    else:
        need = rows_workspace16s(M, N, K, r["env"], r["out"] != "shadow")
    return need - 1 if ws.endswith("-1") else need


def row_query(r, wsb=None):
    wsb = row_ws_bytes(r) if wsb is None else wsb
    kind = Q16S_NT if r["fam"] == "s" else (Q16_NT if r["kind"] == "nt" else Q16_NN)
    return plan_query(kind, r["a"], None, r["c"], r["K"], r["N"], r["epi"], r["env"], wsb, has_ws=wsb > 0, res=r["res"], c_null=r["out"] == "shadow",
                      shadow=r["out"] != "f32", mask16=r["mask16"], ldb=ldb_of(r))


def row_plan(q):
    """the emulation's plan from a plan_query result"""
    p = dict(pieces=max(q[4], 1), per=q[5] if q[4] > 1 else 1 << 40, m_main=q[6])
    if q[6]:
        p["rem"] = (q[7], q[8])
    return p


def tn_row_ws_bytes(r):
    if r["fam"] == "c":
        return tn_workspace16(r["M"], r["K1"], r["N"])
    if r["ws"] == "fallback":
        s = plan_tn16(r["M"], r["K1"], r["N"], _c("BKT"))[0]
        return (s * r["K1"] * r["N"] + s * r["N"]) * 4
    return tn_workspace16s(r["M"], r["K1"], r["N"], r["env"])


def tn_row_query(r, wsb=None):
    wsb = tn_row_ws_bytes(r) if wsb is None else wsb
    c = dict(batch=1, rpb=r["K1"], rs=r["N"] + r["ldc_pad"], bs=0)
    return plan_query(Q16S_TN if r["fam"] == "s" else Q16_TN, r["a"], r["b"], c, r["K1"], r["N"], 0, r["env"], wsb, res=r["res"], bias_grad=r["bias_grad"])


def tn_row_plan(r, q):
    """(slices, rows of the longest slice) for the bound and the emulation; the K1-resident kernel slices by utterances"""
    if q[0] == KS_TN_KRES:
        return dict(pieces=q[4], per=q[11] * r["a"]["rpb"])
    return dict(pieces=q[4], per=q[5])
