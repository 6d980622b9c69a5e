"""
Pins oracle/augment_paths_np.py on the CPU (no device, no launches):
  1. the restated workspace sizes against lidbox_resample_workspace and lidbox_mix_noise_workspace (host-only exports) for
     every row and on a grid around the form thresholds;
  2. every PATHS row selects what it says under the restated dispatch: transform sizes per stage, groups and slot offsets of
     the batch rows, FIR trips / main loop / tail / store forms, the mix form, tile trips; the per-size launch shapes of the
     resampler (log1, log2, tiles, grid, radix-2 placement, block threads) are pinned as a table;
  3. the rows reach every (stage, logP) pair, every length / parity class in both forms, every FIR trip count, every mix form
     and both periodic_load4 branches, and every kernel and instantiation the hipLaunchKernelGGL sites of the two files name
     (read from the source text);
  4. digit_perm against a literal walk of the forward radix-4 / radix-2 stages; the float64 pipeline model against the
     rfft / irfft reference to 1e-12 on every row up to logP = 16; the float32 run of the model inside the 4e-6 tolerance on
     the same rows (no bound is replaced); and each planted mistake outside the tolerance on a row marked for it -- or, for the
     two of ap.UNDETECTABLE, inside it on every marked row, so a stale entry fails;
  5. the FIR bound: an fp32 chain of one product and K - 1 fused multiply-adds lies inside error_bound(S, K), a dropped tap
     and an output shifted by one sample do not, and y[0] is the exact product.
"""

import numpy as np
import pytest

from oracle import augment_paths_np as ap
from oracle.conv2d_np import fma32

RS_IDS = [r["name"] for r in ap.RESAMPLE]


@pytest.fixture(scope="module")
def lib():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native.lib


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64))


def _max_logp(r):
    return max([max(ap.rs_logp(N, M)) for N, M in r["utts"] if N and M], default=-1)


# ---------------------------------------------------------------------------------------------------- 1. exports
def test_restated_workspaces_match_the_exports(lib):
    batches = [r["utts"] for r in ap.RESAMPLE]
    batches += [[(n, m)] for n in (1, 2, 3, 5, 8, 9, 100, 16384, 16385) for m in (0, 1, 2, 7, 9, 12000)]
    batches += [[(9, 16), (16, 9), (0, 0), (5, 0)], [], [(48000, 43637), (131071, 120000), (1 << 21, (1 << 21) - 7)]]
    for utts in batches:
        n_h, m_h = _i64([u[0] for u in utts]), _i64([u[1] for u in utts])
        got = lib.lidbox_resample_workspace(n_h.ctypes.data, m_h.ctypes.data, len(utts))
        assert got == ap.rs_workspace(utts), utts[:4]
    lens = sorted({r["n"] for r in ap.MIX} | {0, 65535, 65536, 65537, 1 << 21})
    for n in lens:
        for J in sorted({len(r["ms"]) for r in ap.MIX} | {0, 1, 3}):
            assert lib.lidbox_mix_noise_workspace(n, J) == ap.mix_workspace(n, J), (n, J)
            assert (ap.mix_workspace(n, J) > 0) == (J > 0 and ap.mix_form(n) == "tiled")


# ---------------------------------------------------------------------------------------------------- 2. what rows select
@pytest.mark.parametrize("r", ap.RESAMPLE, ids=RS_IDS)
def test_every_resample_row_selects_what_it_says(r):
    sel = ap.rs_select(r["utts"])
    assert sel["stages"] == [r["expect"][0], r["expect"][1]], (sel["stages"], r["expect"])
    for N, M in r["utts"]:
        assert 0 <= N <= 1 << ap.RS_MAX_LOG_LEN and 0 <= M <= 1 << ap.RS_MAX_LOG_LEN and (N > 0 or M == 0)
    assert r["one_set"] == (_max_logp(r) >= 19)
    assert set(r["muts"]) <= set(ap.MUTATIONS)


def test_the_batch_rows_split_into_the_groups_they_claim():
    rows = {r["name"]: r for r in ap.RESAMPLE}
    sel = ap.rs_select(rows["b600"]["utts"])
    for stage in (0, 1):                                     # 16-point slots: filter and data, 32 points each
        assert sel["groups"][stage] == [(4, 256, 0), (4, 256, 256 * 32), (4, 88, 512 * 32)]
    utts = rows["boundary"]["utts"]
    gs = ap.rs_groups(utts, 0)
    assert [(lp, len(u), s) for lp, u, s in gs] == [(4, 256, 0), (7, 3, 256 * 32)]
    assert gs[0][1] == list(range(2, 258)) and gs[1][1] == [0, 1, 258]            # stable: batch order inside a size
    assert ap.rs_groups(utts, 1)[1][1] == [0, 1, 258]
    utts = rows["long_among_short"]["utts"]
    sel = ap.rs_select(utts)
    assert sel["groups"] == [[(5, 20, 0), (15, 1, 20 * 64)], [(4, 20, 0), (15, 1, 20 * 32)]]
    kmax, pts, active = ap.rs_plan(utts)
    assert kmax == 10001 and active == 21 and pts == [20 * 64 + (2 << 15), 20 * 32 + (2 << 15)]
    assert ap.rs_workspace(utts) == 16384 * 8 + 21 * 10001 * 8 + pts[0] * 8
    assert ap.rs_k(12, 10) == 6 < kmax                                            # the short ones sit in a wider pitch
    # the group cap itself
    assert [len(u) for _, u, _ in ap.rs_groups([(9, 7)] * 257, 0)] == [256, 1]
    assert [len(u) for _, u, _ in ap.rs_groups([(9, 7)] * 256, 0)] == [256]


def test_the_launch_shape_of_every_transform_size():
    for logP in range(0, 15):
        st = ap.rs_stage(logP)
        assert st["form"] == "lds" and st["log1"] == 0 and st["log2"] == logP and st["grid"] == 1
        assert st["threads"] == {10: 128, 11: 256, 12: 512}.get(logP, 64 if logP < 10 else 1024)
        assert st["r2_rows"] == bool(logP % 2) and not st["r2_cols"] and st["lds"] == 8 << logP <= 128 * 1024
    # logP: log1, log2, columns per tile, rows per tile, workgroups, radix 2 in the columns, in the rows
    want = {15: (7, 8, 32, 16, 8, True, False), 16: (8, 8, 16, 16, 16, False, False), 17: (8, 9, 16, 8, 32, False, True),
            18: (9, 9, 8, 8, 64, True, True), 19: (9, 10, 8, 4, 128, True, False), 20: (10, 10, 4, 4, 256, False, False),
            21: (10, 11, 4, 2, 512, False, True), 22: (11, 11, 2, 2, 1024, True, True)}
    for logP, w in want.items():
        st = ap.rs_stage(logP)
        got = (st["log1"], st["log2"], st["col_tile"], st["row_tile"], st["grid"], st["r2_cols"], st["r2_rows"])
        assert st["form"] == "four" and got == w and st["threads"] == 256 and st["lds"] == 32768, (logP, got)
        assert st["col_tile"] << st["log1"] == 4096 == st["row_tile"] << st["log2"]
        assert st["grid"] * st["col_tile"] == 1 << st["log2"] and st["grid"] * st["row_tile"] == 1 << st["log1"]
    assert len(set(want.values())) == 8
    assert ap.ceil_log2(1) == 0 and ap.ceil_log2(2) == 1 and ap.ceil_log2(3) == 2 and ap.ceil_log2((1 << 22) + 1) == 23
    assert _max_logp(dict(utts=[(1 << 21, 1 << 21)])) == 22                        # the longest utterance still fits


@pytest.mark.parametrize("r", ap.FIR, ids=lambda r: r["name"])
def test_every_fir_row_selects_what_it_says(r):
    K, ns = r["K"], r["ns"]
    p = ap.fir_plan(max(ns), K)
    assert 1 <= K <= ap.FIR_MAX_COEFS and p["main"] == K // 4 and p["tail"] == K % 4 and 4 * p["main"] + p["tail"] == K
    assert p["halo"] % 4 == 0 and K + 3 <= p["halo"] + 3 and p["halo"] >= K and p["lds"] <= 64 * 1024
    assert p["halo"] - 4 * (p["main"] + 1) >= 0                                   # the window's last refill stays inside xs
    assert p["tiles"] == min(-(-max(ns) // 2048), 64)
    trips = [ap.fir_trips(n, p["tiles"]) for n in ns]
    if r["name"].startswith("long_k") and len(ns) == 3:
        assert trips == [1, 2, 3]
    elif r["name"] == "long_k4096":
        assert trips == [2, 2] and p["halo"] == 4100
    else:
        assert set(trips) == {1}
    starts, total = ap.fir_starts(ns)
    assert [s % 4 for s in starts] == [i % 4 for i in range(len(ns))]
    assert all(b - (a + n) >= 4 for a, n, b in zip(starts, ns, starts[1:])) and total >= starts[-1] + ns[-1]


@pytest.mark.parametrize("r", ap.MIX, ids=lambda r: r["name"])
def test_every_mix_row_selects_what_it_says(r):
    n = r["n"]
    want = ("reg<4,0>" if n <= 16384 else "reg<8,0>" if n <= 32768 else "reg<8,8>" if n <= 65536 else "tiled")
    assert ap.mix_form(n) == want and (r["why"].startswith(want) or n == 1 << 21)
    assert ap.mix_tiles(n) == (0 if n <= 65536 else -(-n // 8192)) <= ap.MIX_MAX_TILES
    assert all(m >= 1 for m in r["ms"]) and len(r["ms"]) >= 2
    if n < 1 << 21:
        assert set(r["ms"]) == {m for m in (1, 2, 3, 4, 5, 7, 8, n - 1, n, n + 1, 60001) if m >= 1}


@pytest.mark.parametrize("r", ap.TILE, ids=lambda r: r["name"])
def test_every_tile_row_selects_what_it_says(r):
    totals = [n * k for n, k in r["items"]]
    p = ap.tile_plan(max(totals), max(totals))
    want = dict(small=(4, 4), above_cap=(1024, 5), on_cap=(1024, 4))[r["name"]]
    assert (p["strips"], p["trips"]) == want
    assert ap.tile_one_set(r) == (r["name"] != "small")


# ---------------------------------------------------------------------------------------------------- 3. coverage
def _classes(rows):
    out = set()
    for r in rows:
        for N, M in r["utts"]:
            if N and M:
                form = {ap.rs_stage(lp)["form"] for lp in ap.rs_logp(N, M)}
                for f in form:
                    out.add((f, "M<N" if M < N else ("M=N" if M == N else "M>N")))
                    out.add((f, "min even" if min(N, M) % 2 == 0 else "min odd"))
                    out.add((f, "M even" if M % 2 == 0 else "M odd"))
    return out


def test_resample_rows_reach_every_size_class_and_group_shape():
    assert len(set(RS_IDS)) == len(RS_IDS)
    seen = set()
    for r in ap.RESAMPLE:
        for N, M in r["utts"]:
            if N and M:
                lp = ap.rs_logp(N, M)
                seen |= {(0, lp[0]), (1, lp[1])}
    assert seen == {(s, lp) for s in (0, 1) for lp in range(23)}, sorted({(s, lp) for s in (0, 1) for lp in range(23)} - seen)
    # the smallest N = M of every size really is the smallest
    for n, lp in zip(ap._SMALLEST, (0,) + tuple(range(2, 23))):
        assert ap.rs_logp(n, n) == (lp, lp) and (n == 1 or ap.rs_logp(n - 1, n - 1)[0] < lp)
    assert all(ap.rs_logp(n, n)[0] != 1 for n in range(1, 10))                    # logP = 1 needs unequal lengths
    want = {(f, c) for f in ("lds", "four") for c in ("M<N", "M=N", "M>N", "min even", "min odd", "M even", "M odd")}
    assert _classes(ap.RESAMPLE) == want
    # every class also among the rows that run a single utterance (a batch row cannot stand in for them)
    assert _classes([r for r in ap.RESAMPLE if len(r["utts"]) == 1]) == want
    utts = {u for r in ap.RESAMPLE for u in r["utts"]}
    assert (0, 0) in utts and any(N > 0 and M == 0 for N, M in utts)
    groups = {tuple(len(u) for _, u, _ in ap.rs_groups(r["utts"], 0)) for r in ap.RESAMPLE}
    assert (256, 256, 88) in groups and (256, 3) in groups and (20, 1) in groups
    # the tone data set reaches both forms and both Nyquist factors that it can see (0.5 and 1)
    tone = {(ap.rs_stage(ap.rs_logp(N, M)[0])["form"], M > N) for r in ap.RESAMPLE if "nyquist" in ap.rs_kinds(r)
            for N, M in r["utts"] if ap.rs_kind_of("nyquist", N, M) == "nyquist"}
    assert tone == {("lds", False), ("lds", True), ("four", False), ("four", True)}
    assert all(ap.rs_kinds(r) == ("normal",) for r in ap.RESAMPLE if r["one_set"])
    assert {19, 20, 21, 22} <= {_max_logp(r) for r in ap.RESAMPLE if r["one_set"]}


def test_fir_rows_reach_every_tap_count_length_trip_and_store_form():
    assert {r["K"] for r in ap.FIR} == {1, 2, 3, 4, 5, 7, 8, 9, 4095, 4096}
    assert {n for r in ap.FIR for n in r["ns"]} >= {1, 7, 8, 9, 2047, 2048, 2049, 131072, 131073, 270000}
    assert {r["K"] % 4 for r in ap.FIR} == {0, 1, 2, 3} and {r["K"] // 4 for r in ap.FIR} >= {0, 1, 2, 1023, 1024}
    trips = {(r["K"], ap.fir_trips(n, ap.fir_plan(max(r["ns"]), r["K"])["tiles"])) for r in ap.FIR for n in r["ns"]}
    assert {t for _, t in trips} == {1, 2, 3} and (4096, 2) in trips and (5, 3) in trips and (1, 3) in trips
    res, stores = set(), set()
    for r in ap.FIR:
        starts, _ = ap.fir_starts(r["ns"])
        for s, n in zip(starts, r["ns"]):
            res.add(s % 4)
            stores |= {(s % 4 == 0, f) for f in ap.fir_stores(s, n)}
    assert res == {0, 1, 2, 3}
    assert stores == {(True, "vec"), (True, "scalar"), (False, "scalar")}        # an aligned utterance ends on a scalar lane
    assert ap.fir_store_vec(4, 8, 16) and not ap.fir_store_vec(4, 8, 15) and not ap.fir_store_vec(5, 8, 16)


def test_mix_and_tile_rows_reach_every_form_branch_and_trip():
    assert {r["n"] for r in ap.MIX} == set(ap.MIX_NS) | {1 << 21}
    assert set(ap.MIX_NS) == {1, 3, 4, 5, 16384, 16385, 32768, 32769, 65536, 65537, 73728, 73729}
    assert {ap.mix_form(r["n"]) for r in ap.MIX} == {"reg<4,0>", "reg<8,0>", "reg<8,8>", "tiled"}
    for a, b in ((16384, 16385), (32768, 32769), (65536, 65537)):                  # each switch, from both sides
        assert ap.mix_form(a) != ap.mix_form(b)
    assert ap.mix_tiles(73728) == 9 and ap.mix_tiles(73729) == 10 and ap.mix_tiles(1 << 21) == 256
    assert {r["res"][0] for r in ap.MIX} == {0, 1, 2, 3} == {r["res"][1] for r in ap.MIX}
    by_form = {}
    for r in ap.MIX:
        for j, m in enumerate(r["ms"]):
            br = ap.mix_branches(r["n"], m, (r["res"][1] + j) % 4)
            s = by_form.setdefault(ap.mix_form(r["n"]), set())
            s |= {k for k, v in br.items() if v}
    assert all(v == {"vec", "loop"} for v in by_form.values()) and len(by_form) == 4, by_form
    # the restated branch, at its edges
    assert ap.periodic_branch(8, 0, 0) == "vec" and ap.periodic_branch(8, 4, 0) == "vec" and ap.periodic_branch(7, 4, 0) == "loop"
    assert ap.periodic_branch(8, 0, 1) == "loop" and ap.periodic_branch(9, 3, 1) == "vec" and ap.periodic_branch(8, 12, 0) == "vec"
    assert ap.mix_branches(16, 8, 0) == dict(vec=4, loop=0) and ap.mix_branches(16, 7, 0) == dict(vec=1, loop=3)
    assert {n for r in ap.TILE for n, _ in r["items"]} >= {1, 3, 4, 5, 4099}
    totals = {n * k for r in ap.TILE for n, k in r["items"]}
    assert 1024 * 4096 in totals and 4099 * 1100 in totals and 4099 * 1100 > 1024 * 4096
    assert {ap.tile_plan(t, t)["trips"] for t in totals if t} >= {1, 4, 5}


def test_rows_reach_every_kernel_the_launch_sites_name():
    sites = ap.launch_site_kernels()
    assert sites["augment.hip"] == {"rs_twiddle_kernel", "rs_col_fwd_kernel<true>", "rs_col_fwd_kernel<false>",
                                    "rs_row_kernel<true>", "rs_row_kernel<false>", "rs_col_inv_kernel", "fir_kernel"}
    assert sites["mix_noise.hip"] == {"mix_reg_kernel<4,0>", "mix_reg_kernel<8,0>", "mix_reg_kernel<8,8>", "mix_tile_kernel<0>",
                                      "mix_tile_kernel<1>", "mix_tile_kernel<2>", "signal_tile_kernel"}
    seen = set()
    for r in ap.RESAMPLE:
        seen |= ap.rs_select(r["utts"])["kernels"]
    assert ap.FIR and ap.TILE                                 # one kernel each, whatever the row
    seen |= {"fir_kernel", "signal_tile_kernel"}
    seen |= ap.mix_kernels([r["n"] for r in ap.MIX])
    want = sites["augment.hip"] | sites["mix_noise.hip"]
    assert seen == want, (sorted(want - seen), sorted(seen - want))
    # both forms launch rs_row_kernel; each is reached on its own
    lds = set().union(*(ap.rs_select(r["utts"])["kernels"] for r in ap.RESAMPLE if 0 <= _max_logp(r) <= 14))
    assert lds == {"rs_twiddle_kernel", "rs_row_kernel<true>", "rs_row_kernel<false>"}


# ---------------------------------------------------------------------------------------------------- 4. model, mutations
@pytest.mark.parametrize("logn", range(1, 9))
def test_digit_perm_is_the_order_the_forward_stages_leave(logn):
    n = 1 << logn
    x = np.random.default_rng(logn).standard_normal(2 * n).view(np.complex128)
    perm = [ap.digit_perm(j, logn) for j in range(n)]
    assert sorted(perm) == list(range(n))
    assert np.abs(ap.lds_fft_forward(x) - np.fft.fft(x)[perm]).max() <= 1e-12 * np.abs(x).sum()


def _model_rows():
    return [r for r in ap.RESAMPLE if _max_logp(r) <= 16]


@pytest.mark.parametrize("r", _model_rows(), ids=lambda r: r["name"])
def test_the_model_equals_the_reference_and_its_float32_run_keeps_the_tolerance(r):
    ms = [M for _, M in r["utts"]]
    for kind in ap.rs_kinds(r):
        xs = ap.rs_draw(r, kind)
        refs = [ap.resample_ref(x, m) for x, m in zip(xs, ms)]
        for y, ref in zip(ap.rs_model(xs, ms), refs):
            assert y.shape == ref.shape
            if len(ref):
                assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max(), (r["name"], kind)
        worst = (0.0, 0.0)
        for x, y, ref in zip(xs, ap.rs_model(xs, ms, dt=np.float32), refs):
            e = ap.rs_errors(y, ref, x)
            worst = (max(worst[0], e[0]), max(worst[1], e[1]))
        print("%-18s %-8s float32 model: rel L2 %.2e  max / max|x| %.2e" % (r["name"], kind, *worst))
        assert max(worst) <= ap.RS_TOL and (r["name"], kind) not in ap.RS_TOL_OVERRIDE


def test_the_reference_is_the_fourier_method():
    import scipy.signal as scipy_signal
    rng = np.random.default_rng(0)
    for N, M in ((12, 10), (13, 9), (10, 13), (9, 12), (11, 11), (16, 16), (1, 5), (5, 1), (2, 1), (1, 2), (700, 701)):
        x = rng.standard_normal(N).astype(np.float32)
        assert np.abs(ap.resample_ref(x, M) - scipy_signal.resample(x.astype(np.float64), M)).max() <= 5e-15


def _caught(r, mut):
    """does the mistake leave the tolerance for some utterance of the row on some data set"""
    ms = [M for _, M in r["utts"]]
    for kind in ap.rs_kinds(r):
        xs = ap.rs_draw(r, kind)
        for x, m, y in zip(xs, ms, ap.rs_model(xs, ms, mut)):
            if m and max(ap.rs_errors(y, ap.resample_ref(x, m), x)) > ap.RS_TOL:
                return True
    return False


@pytest.mark.parametrize("mut", ap.MUTATIONS)
def test_every_planted_mistake_is_caught_or_listed(mut):
    rows = [r for r in ap.RESAMPLE if mut in r["muts"]]
    assert rows and all(_max_logp(r) <= 16 for r in rows)
    hits = [r["name"] for r in rows if _caught(r, mut)]
    print(mut, "caught on", hits, "of", [r["name"] for r in rows])
    if mut in ap.UNDETECTABLE:
        assert not hits, "%s is listed as undetectable but leaves the tolerance on %s" % (mut, hits)
        assert mut in ap.__doc__.split("UNDETECTABLE.")[1]
    else:
        assert hits, "%s stays inside the tolerance on every row marked for it" % mut


def test_a_slot_offset_that_is_too_large_leaves_the_workspace():
    """the other direction of slot_255: what the exactly sized, guarded workspace of the GPU module is there for"""
    utts = next(r for r in ap.RESAMPLE if r["name"] == "b600")["utts"]
    _, pts, _ = ap.rs_plan(utts)
    last = ap.rs_groups(utts, 0, slot_count=257)[-1]
    assert last[2] + len(last[1]) * (2 << last[0]) > max(pts)
    last = ap.rs_groups(utts, 0)[-1]
    assert last[2] + len(last[1]) * (2 << last[0]) == max(pts)


# ---------------------------------------------------------------------------------------------------- 5. FIR
def test_sparse_taps_make_the_bound_see_one_lost_sample_under_the_largest_halo():
    K, n, at = 4096, 4096 + 400, 4096 + 100
    x = ap.draw("normal", n, 9)
    for kind in ap.fir_kinds(dict(K=K)):
        f = ap.fir_coefs(kind, K, 10)
        ref, S = ap.fir_ref(x, f)
        lost = x.copy()
        lost[at] = 0.0                                        # one sample of a full window never arrives
        got = ap.fir_ref(lost, f)[0]
        seen = np.abs(got - ref) > ap.error_bound(S, K)
        live = np.flatnonzero(f) + at
        live = live[live < n]
        if kind == "sparse":
            assert np.count_nonzero(f) <= 16 and f[0] and f[K - 1] and seen[live].all() and not seen[:at].any()
        else:
            assert not seen[live].all()                       # a dense set sees it in some outputs only: the term is about the bound
    assert ap.fir_kinds(dict(K=9)) == ap.KINDS and [r["K"] for r in ap.FIR if "sparse" in ap.fir_kinds(r)] == [4095, 4096, 4096]
    assert next(r for r in ap.FIR if r["name"] == "long_k4096")["ns"] == [131073, 135000]          # one and 3 928 outputs in trip 2


@pytest.mark.parametrize("K", [1, 3, 4, 9, 64])
def test_the_fir_bound_holds_an_fp32_chain_and_sees_a_dropped_tap(K):
    for kind in ap.KINDS:
        x, f = ap.draw(kind, 200, 7), ap.draw(kind, K, 8)
        xp = np.concatenate([np.zeros(K - 1, np.float32), x])
        taps = lambda k: xp[K - 1 - k:K - 1 - k + len(x)]                          # x[n - k], zero before the start
        acc = (f[0] * taps(0)).astype(np.float32)
        for k in range(1, K):
            acc = fma32(np.full_like(x, f[k]), taps(k), acc)
        ref, S = ap.fir_ref(x, f)
        bound = ap.error_bound(S, K)
        assert (np.abs(acc - ref) <= bound).all() and acc[0] == np.float32(f[0] * x[0])
        assert K > 1 or np.array_equal(acc, f[0] * x)
        dropped = acc - (f[K - 1] * taps(K - 1)).astype(np.float32)
        assert (np.abs(dropped - ref) > bound)[K - 1:].mean() > 0.9
        shifted = np.concatenate([[np.float32(0)], acc[:-1]])
        assert (np.abs(shifted - ref) > bound).mean() > 0.9
        # a wrong first output alone, which a whole-signal bound cannot see
        wrong = acc.copy()
        wrong[0] = np.float32(f[0]) * x[0] * np.float32(1 + 3 * ap.gamma(K))
        assert np.abs(wrong[0] - ref[0]) > bound[0] and np.abs(wrong - ref).max() <= 1e-6 * np.abs(f).sum() * np.abs(x).max()
