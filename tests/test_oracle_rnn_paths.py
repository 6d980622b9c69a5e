"""
Pins oracle/rnn_paths_np.py on the CPU (no device, no launches):
  1. the whole-layer float64 LSTM / GRU against float64 torch.nn.LSTM / torch.nn.GRU autograd to 1e-12 (both directions,
     sequence and final-state gradients), and the one-step references chained over T against the whole-layer oracle;
  2. the restated host functions against the library's own exports on a grid that holds every PATHS row;
  3. every PATHS row selects what its comment says under the restated dispatch, and the rows together reach every kernel and
     instantiation of the recurrence files (an enumerated set: 17 of the recurrences and the two pool kernels);
  4. the fp32 emulation of every row lies inside the bounds on both data sets, and the bounds are not vacuous: each mutation of
     rp.MUT_FWD / rp.MUT_BWD planted into one step leaves the bound in every (direction, batch row) it touches while the
     untouched rows stay inside.

Mutations are planted where they touch one step only: forward at step s = 1 (the first with a product), recomputed from the
clean stored state; backward at step s = T - 2 (the first with a product and a carry), from the clean state after step
T - 1, and judged at that step alone (the steps after it inherit the fault in ways that depend on the data); omit_dh_last at
s = T - 1, judged there.  A mutation applies to a row when the row has what it removes (rp.mut_applies): a product needs T >= 2, drop_first_k2 a
second chunk, row_shift a second batch row, omit_dh_last a dh_last.  Rows with B > 130 are emulated on 13 of their batch rows
(the first four, 62 .. 66 and the last four): rows are independent of each other in every form.  EXCLUDED lists the pairs
that are left out, with the reason; its cap is 1 % of the pairs.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import rnn_paths_np as rp

ROWS = [(k, r) for k in ("step", "gru", "lstm") for r in rp.PATHS[k]]
IDS = ["%s-%s" % (k, r["name"]) for k, r in ROWS]
# (table, row name, kind, pass, mutation) -> reason.  Both are single terms of a backward chain of K >= 784 terms on the N(0, 1)
# data set: the dropped |dZ[b, k]| max_u |U[u, k]| is smaller than gamma(2 K) sum_k |dZ[b, k]| |U[u, k]| when |dZ[b, k]| is
# under about an eighth of the row's mean |dZ|, which a product of normal factors is every so often (the 1 + 0.1 N(0, 1) data
# set has no such element).  Four seeds of the draw were tried; each leaves two or three such pairs.  The test asserts that
# an excluded pair really stays inside, so a stale entry fails.
_SMALL = "the dropped term of batch row 0 is below the rounding bound of its %d-term chain"
EXCLUDED = {("step", "w4_H196", "normal", "bwd", "drop_last_k"): _SMALL % 784,
            ("gru", "vec_H768", "normal", "bwd", "drop_last_k"): _SMALL % 2304}


@pytest.fixture(scope="module")
def lib():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native.lib


# ---------------------------------------------------------------------------------------------------- 1. the oracle itself
def _torch_lstm(U, zg, dh_seq, dh_last):
    """float64 torch.nn.LSTM fed the projection through an identity input weight: dX is dZ"""
    dirs, B, T, H4 = zg.shape
    H = H4 // 4
    hs, dzs = [], []
    for d in range(dirs):
        m = torch.nn.LSTM(H4, H, batch_first=True).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(torch.eye(H4))
            m.weight_hh_l0.copy_(torch.from_numpy(U[d].astype(np.float64).T))
            m.bias_ih_l0.zero_()
            m.bias_hh_l0.zero_()
        x = torch.from_numpy(zg[d].astype(np.float64))
        x = (x.flip(1) if d else x).requires_grad_(True)
        y, _ = m(x)
        g = torch.from_numpy(dh_seq[:, :, d * H:(d + 1) * H].astype(np.float64))
        loss = (y * (g.flip(1) if d else g)).sum() + (y[:, -1] * torch.from_numpy(dh_last[:, d * H:(d + 1) * H].astype(np.float64))).sum()
        loss.backward()
        hs.append((y.flip(1) if d else y).detach().numpy())
        dzs.append((x.grad.flip(1) if d else x.grad).numpy())
    return np.stack(hs), np.stack(dzs)


def _torch_gru(U, brec, zg, dh_seq, dh_last):
    """torch orders the gates r, z, n; ours are z, r, h (as test_gru_gpu.py maps them)"""
    dirs, B, T, H3 = zg.shape
    H = H3 // 3
    perm = np.concatenate([np.arange(H, 2 * H), np.arange(0, H), np.arange(2 * H, 3 * H)])      # torch block -> ours
    hs, dzs, dbn = [], [], []
    for d in range(dirs):
        m = torch.nn.GRU(H3, H, batch_first=True).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(torch.eye(H3))
            m.weight_hh_l0.copy_(torch.from_numpy(U[d].astype(np.float64)[:, perm].T))
            m.bias_ih_l0.zero_()
            m.bias_hh_l0.copy_(torch.from_numpy(brec[d].astype(np.float64)[perm]))
        x0 = torch.from_numpy(zg[d].astype(np.float64)).requires_grad_(True)
        x = x0[:, :, perm]
        y, _ = m(x.flip(1) if d else x)
        g = torch.from_numpy(dh_seq[:, :, d * H:(d + 1) * H].astype(np.float64))
        loss = (y * (g.flip(1) if d else g)).sum() + (y[:, -1] * torch.from_numpy(dh_last[:, d * H:(d + 1) * H].astype(np.float64))).sum()
        loss.backward()
        hs.append((y.flip(1) if d else y).detach().numpy())
        dzs.append(x0.grad.numpy())
        dbn.append(m.bias_hh_l0.grad.numpy()[2 * H:])
    return np.stack(hs), np.stack(dzs), np.stack(dbn)


@pytest.mark.parametrize("H,B,T", [(1, 1, 1), (5, 3, 4), (17, 2, 3)])
def test_whole_layer_oracle_matches_torch_autograd(H, B, T):
    for fam in ("step", "gru"):
        dat = rp.draw(fam, H, 2, B, T, "normal")
        if fam == "gru":
            G, Q, Hs, DZ, DQ = rp.gru_layer(dat["U"], dat["brec"], dat["zg"], dat["dh_seq"], dat["dh_last"])
            h, dz, dbn = _torch_gru(dat["U"], dat["brec"], dat["zg"], dat["dh_seq"], dat["dh_last"])
            assert np.abs(DQ.sum((1, 2)) - dbn).max() <= 1e-12 * max(1.0, np.abs(dbn).max())
        else:
            G, C, Hs, DZ = rp.lstm_layer(dat["U"], dat["zg"], dat["dh_seq"], dat["dh_last"])
            h, dz = _torch_lstm(dat["U"], dat["zg"], dat["dh_seq"], dat["dh_last"])
        assert np.abs(Hs - h).max() <= 1e-12
        assert np.abs(DZ - dz).max() <= 1e-12 * max(1.0, np.abs(dz).max())


@pytest.mark.parametrize("dh", ["seq", "last", "both"])
@pytest.mark.parametrize("dirs", [1, 2])
def test_one_step_references_chained_equal_the_whole_layer(dirs, dh):
    H, B, T = 17, 3, 4
    r = dict(dh=dh)
    for fam in ("step", "gru"):
        dat = rp.draw(fam, H, dirs, B, T, "offset")
        dh_seq, dh_last = rp.given(r, dat)
        hs = np.zeros((B, T + 2, dirs * H))
        if fam == "gru":
            G, Q, Hs, DZ, DQ = rp.gru_layer(dat["U"], dat["brec"], dat["zg"], dh_seq, dh_last)
            for _ in range(T):
                ref = rp.gru_fwd_ref(dat["U"], dat["brec"], dat["zg"], hs, 2 * H)
                for d in range(dirs):
                    hs[:, 1:T + 1, d * H:(d + 1) * H] = ref["h"].v[d]
            assert max(np.abs(ref["gates"].v - G).max(), np.abs(ref["qh"].v - Q).max(), np.abs(ref["h"].v - Hs).max()) <= 1e-12
            dz, dq = rp.gru_bwd_ref(dat["U"], G, Q, hs, dh_seq, dh_last, 6 * H)
            assert max(np.abs(dz.v - DZ).max(), np.abs(dq.v - DQ).max()) <= 1e-12
        else:
            G, C, Hs, DZ = rp.lstm_layer(dat["U"], dat["zg"], dh_seq, dh_last)
            cs = np.zeros((dirs, B, T, H))
            for _ in range(T):
                ref = rp.lstm_fwd_ref(dat["U"], dat["zg"], hs, cs, 2 * H)
                cs = ref["c"].v
                for d in range(dirs):
                    hs[:, 1:T + 1, d * H:(d + 1) * H] = ref["h"].v[d]
            assert max(np.abs(ref["gates"].v - G).max(), np.abs(ref["c"].v - C).max(), np.abs(ref["h"].v - Hs).max()) <= 1e-12
            dz = rp.lstm_bwd_ref(dat["U"], G, C, dh_seq, dh_last, 8 * H)
            assert np.abs(dz.v - DZ).max() <= 1e-12
        # the bounds of exact inputs are positive and small
        assert (dz.e > 0).all() and dz.e.max() < 1e-3


# ---------------------------------------------------------------------------------------------------- 2. exports
def test_restated_host_functions_match_the_exports(lib):
    grw = lambda M, N, K: lib.lidbox_gemm_rows_workspace(M, N, K)
    Hs = sorted({r["H"] for _, r in ROWS} | set(range(0, 100)) | {250, 1024, 16384})
    for H in Hs:
        assert lib.lidbox_lstm_resident_ok(H) == rp.lstm_resident_ok(H), H
    shapes = {(r["B"], r["T"], r["H"], r["dirs"]) for _, r in ROWS}
    shapes |= {(B, T, H, dirs) for B in (0, 1, 7, 256) for T in (0, 1, 5) for H in (0, 1, 80, 81, 250) for dirs in (0, 1, 2, 3)}
    for B, T, H, dirs in sorted(shapes):
        assert lib.lidbox_lstm_workspace(B, T, H, dirs) == rp.lstm_workspace(B, T, H, dirs, grw), (B, T, H, dirs)
        assert lib.lidbox_lstm_step_workspace(B, T, H, dirs) == rp.step_workspace(B, T, H, dirs), (B, T, H, dirs)
        assert lib.lidbox_gru_workspace(B, T, H, dirs) == rp.step_workspace(B, T, H, dirs), (B, T, H, dirs)
    assert rp.resident_lds(80, 4, True) <= rp.LSTM_LDS_BUDGET < rp.resident_lds(96, 4, True)
    assert rp.lstm_workspace(17, 3, 81, 2, grw) >= 2 * 2 * 17 * 81 * 4


# ---------------------------------------------------------------------------------------------------- 3. PATHS
@pytest.mark.parametrize("k,r", ROWS, ids=IDS)
def test_every_row_selects_what_it_is_there_for(k, r):
    sel = rp.select(r)
    for key, want in r["expect"].items():
        assert sel[key] == want, (key, sel[key], want)
    assert 1 <= r["T"] <= 4 and r["B"] >= 1
    if k == "step":
        assert r["col"] + r["dirs"] * r["H"] <= rp.h_rs(r)
    else:
        assert r["rs_extra"] == 0 and r["col"] == 0
    if r["twin"]:
        t = next(x for x in rp.PATHS[k] if x["name"] == r["twin"])
        assert (t["H"], t["dirs"], t["B"], t["T"]) == (r["H"], r["dirs"], r["B"], r["T"]) and not t["shift"] and t["rs_extra"] == 0


def test_rows_reach_every_instantiation():
    names = IDS
    assert len(set(names)) == len(names)
    seen = set()
    for _, r in ROWS:
        seen |= rp.select(r)["kernels"]
    assert rp.POOL                                           # the two pool kernels have one form each
    seen |= {("seq_avg_pool_fwd_kernel",), ("seq_avg_pool_bwd_kernel",)}
    want = rp.reachable()
    assert len(want) == 3 + 2 + 4 + 6 + 2 + 2           # 17 recurrence kernels / instantiations and the two pool kernels
    assert seen == want, (sorted(map(str, want - seen)), sorted(map(str, seen - want)))


def test_tables_cover_the_edges_the_issue_names():
    step = {r["name"]: rp.select(r) for r in rp.STEP}
    by_w = {w: {tuple(s["kpads"]) for s in step.values() if s["w"] == w} for w in (4, 2, 1)}
    for w in (4, 2, 1):                                       # kpad 32 .. 256 in steps of 32 under every forward width
        assert {(k,) for k in range(32, 257, 32)} <= by_w[w], (w, by_w[w])
    assert {1, 2, 3, 4} <= {s["last_group"][0] for s in step.values()}                      # partial prefetch groups of 1 - 3 blocks
    assert step["w1_H257"]["kpads"] == [256, 32] and step["w1_H255"]["bkpads"] == [1024] and step["w4_H256"]["bkpads"] == [1024]
    assert step["w1_H257"]["bkpads"] == [1024, 32]
    assert rp.chunk_plan(rp.LstmStep, 257, True)[1]["klen"] == 1 and rp.chunk_plan(rp.LstmStep, 1028, False)[1]["klen"] == 4
    gru = {r["name"]: rp.select(r) for r in rp.GRU}
    assert gru["sc_H767"]["bkpads"] == [768] and gru["vec_H768"]["bkpads"] == [768] and gru["sc_H769"]["bkpads"] == [768, 32]
    assert gru["vec_H772"]["bkpads"] == [768, 32] and rp.chunk_plan(rp.GruStep, 769, False)[1]["klen"] == 1
    for tab in (rp.STEP, rp.GRU):
        assert {1, 15, 16, 17, 63, 64, 65, 129} <= {r["B"] for r in tab}
        assert {(65, 17), (17, 33), (1, 1)} <= {(r["B"], r["H"]) for r in tab}
        assert {"seq", "last", "both"} <= {r["dh"] for r in tab} and {1, 2} <= {r["dirs"] for r in tab}
        assert {1, 2, 3, 4} <= {r["T"] for r in tab}
    # each pointer misaligned alone
    assert {tuple(r["shift"]) for r in rp.GRU if r["shift"]} == {("U0",), ("U1",), ("zg",), ("hseq",), ("qh",)}
    assert {(tuple(r["shift"].items())) for r in rp.STEP if r["H"] == 16 and r["shift"]} >= {
        (("U0", 1),), (("U1", 1),), (("hseq", 1),), (("U0", 2),), (("U1", 2),), (("hseq", 2),), (("zg", 1),)}
    lstm = {r["name"]: (r, rp.select(r)) for r in rp.LSTM}
    assert {rp.pad16(r["H"]) for r, s in lstm.values() if s["form"] == "res"} == {16, 32, 48, 64, 80}
    assert {s["big_lds"] for r, s in lstm.values() if s["form"] == "res" and s["rt"] == 1} == {True, False}
    assert {(r["B"], r["dirs"], s["rt"]) for r, s in lstm.values() if s.get("rt", 1) > 1} == {(513, 2, 2), (1025, 1, 2), (1025, 2, 4), (2049, 1, 4)}
    for B, dirs in ((512, 2), (1024, 1)):
        assert rp.pick_rt(B, dirs) == 1 and rp.pick_rt(2 * B, dirs) == 2 and rp.pick_rt(2 * B + 1, dirs) == 4
    assert {(r["H"], r["B"]) for r, s in lstm.values() if s["form"] == "stp"} >= {(H, B) for H in (81, 100) for B in (1, 17, 65)}
    bc = lambda p: p["B"] * p["C"]
    assert {bc(p) for p in rp.POOL} >= {255, 256, 257} and {bc(p) * p["T"] for p in rp.POOL} >= {255, 256, 257}
    assert {p["acc"] for p in rp.POOL} == {0, 1} and {p["pitched"] for p in rp.POOL} == {True, False} and any(p["T"] == 1 for p in rp.POOL)


def test_k_order_is_a_permutation_in_blocks_of_32():
    for P, H, fwd in ((rp.LstmStep, 257, True), (rp.LstmStep, 33, False), (rp.GruStep, 769, False), (rp.GruStep, 17, True)):
        plans = rp.pass_plan(P, H, fwd)
        o = rp.k_order(plans, H)
        K = sum(c["klen"] for p in plans for c in p)
        assert sorted(o) == list(range(K)) and rp.n_fused(P, H, fwd) == 2 * K
    assert rp.k_order(rp.pass_plan(rp.LstmStep, 40, True), 40)[:6] == [0, 8, 16, 24, 1, 9]


# ---------------------------------------------------------------------------------------------------- 4. emulation, mutations
def _sub(r, dat):
    """rows with a large B are emulated on 13 of their batch rows"""
    B = r["B"]
    if B <= 130:
        return r, dat
    idx = np.r_[0:4, 62:67, B - 4:B]
    d2 = dict(dat, zg=dat["zg"][:, idx], dh_seq=dat["dh_seq"][idx], dh_last=dat["dh_last"][idx])
    return dict(r, B=len(idx)), d2


def _inside(checks, what):
    for name, got, ref in checks:
        q = rp.ratio(got, ref)
        assert (q <= 1.0).all(), "%s %s: emulation %.3g x the bound" % (what, name, q.max())


def _touched(checks, sel, rows, cols=None):
    """per batch row of `rows`: does any judged output at the selected (direction, time) leave the bound; and do all other
    batch rows (and, with cols, all other units of the touched rows) stay inside"""
    B = checks[0][1].shape[1]
    out = np.zeros(B, bool)
    clean = True
    for name, got, ref in checks:
        q = rp.ratio(got, ref) > 1.0
        for d, t in sel:
            m = q[d, :, t]                                    # [B, W]
            if cols is not None:
                W, H = m.shape[1], len(cols)
                unit = np.tile(cols, W // H)
                clean &= not m[:, ~unit].any()
                m = m[:, unit]
            out |= m.any(1)
            others = np.setdiff1d(np.arange(B), rows)
            clean &= not q[d, others, t].any()
    return out[rows], clean


@pytest.mark.parametrize("kind", rp.KINDS)
@pytest.mark.parametrize("k,r", ROWS, ids=IDS)
def test_emulation_is_inside_the_bounds_and_every_mutation_outside(k, r, kind):
    fam = rp.fam_of(r)
    H, dirs, T = r["H"], r["dirs"], r["T"]
    r2, dat = _sub(r, rp.draw("gru" if fam == "gru" else "step", H, dirs, r["B"], T, kind))
    B = r2["B"]
    U = dat["U"]
    dh_seq, dh_last = rp.given(r2, dat)
    what = "%s/%s/%s" % (k, r["name"], kind)
    # ---- forward
    st = rp.emu_gru_fwd(U, dat["brec"], dat["zg"]) if fam == "gru" else rp.emu_lstm_fwd(fam, U, dat["zg"])
    _inside(rp.fwd_checks(r2, dat, st), what)
    h = rp.h_of(st["hs"], dirs, H)
    whole = rp.gru_layer(U, dat["brec"], dat["zg"])[2] if fam == "gru" else rp.lstm_layer(U, dat["zg"])[2]
    assert np.abs(h - whole).max() <= rp.H_TOL
    assert not st["hs"][:, 0].any() and not st["hs"][:, T + 1].any()
    sel = [(d, 1 if d == 0 else T - 2) for d in range(dirs)]                    # t of step s = 1
    allb = np.arange(B)
    last_slice = np.arange(H) >= 16 * ((H - 1) // 16)
    for mut in rp.MUT_FWD:
        if not rp.mut_applies(fam, mut, True, H, B, T):
            continue
        st2 = copy.deepcopy(st)
        if fam == "gru":
            rp.emu_gru_fwd_step(U, dat["brec"], dat["zg"], st2, 1, mut)
        else:
            rp.emu_lstm_fwd_step(fam, U, dat["zg"], st2, 1, mut)
        rows = np.array([rp.mut_row(B)]) if mut == "row_shift" else allb
        hit, clean = _touched(rp.fwd_checks(r2, dat, st2), sel, rows, last_slice if mut == "unit_shift" else None)
        assert hit.all(), "%s fwd %s: batch rows %s stay inside the bound" % (what, mut, rows[~hit])
        assert clean, "%s fwd %s: an untouched row left the bound" % (what, mut)
    # ---- backward
    if fam == "gru":
        run = lambda upto, mut=None: rp.emu_gru_bwd(U, st, dh_seq, dh_last, upto, mut)
        step = lambda bw, s, mut: rp.emu_gru_bwd_step(U, st, dh_seq, dh_last, bw, s, mut)
    else:
        run = lambda upto, mut=None: rp.emu_lstm_bwd(fam, U, st, dh_seq, dh_last, upto, mut)
        step = lambda bw, s, mut: rp.emu_lstm_bwd_step(fam, U, st, dh_seq, dh_last, bw, s, mut)
    _inside(rp.bwd_checks(r2, dat, st, run(0)), what + " bwd")
    before = run(T - 1)                                                         # the state after the first step walked
    sel0 = [(d, T - 2 if d == 0 else 1) for d in range(dirs)]                   # t of step s = T - 2
    selL = [(d, T - 1 if d == 0 else 0) for d in range(dirs)]                   # t of step s = T - 1
    for mut in rp.MUT_BWD:
        if not rp.mut_applies(fam, mut, False, H, B, T, dh_last is not None):
            continue
        if mut == "omit_dh_last":
            bw2, s_ = run(0, mut), selL
        else:
            bw2, s_ = copy.deepcopy(before), sel0
            step(bw2, T - 2, mut)
        rows = np.array([rp.mut_row(B)]) if mut == "row_shift" else allb
        hit, clean = _touched(rp.bwd_checks(r2, dat, st, bw2), s_, rows)
        if (k, r["name"], kind, "bwd", mut) in EXCLUDED:
            assert not hit.all() and hit.any(), "%s bwd %s: listed in EXCLUDED, but caught in %s" % (what, mut, rows[hit])
        else:
            assert hit.all(), "%s bwd %s: batch rows %s stay inside the bound" % (what, mut, rows[~hit])
        if mut != "omit_dh_last":
            assert clean, "%s bwd %s: an untouched row left the bound" % (what, mut)


def test_exclusions_stay_under_the_cap():
    """the (row, data set, pass, mutation) pairs the cases above plant, counted with the rule they use"""
    pairs = 0
    for k, r in ROWS:
        fam, B = rp.fam_of(r), min(r["B"], 13 if r["B"] > 130 else r["B"])
        for fwd, muts in ((True, rp.MUT_FWD), (False, rp.MUT_BWD)):
            pairs += 2 * sum(rp.mut_applies(fam, m, fwd, r["H"], B, r["T"], r["dh"] != "seq") for m in muts)
    names = {(k, r["name"]) for k, r in ROWS}
    assert all(key[:2] in names and key[2] in rp.KINDS for key in EXCLUDED)
    print("mutation pairs planted: %d, excluded: %d" % (pairs, len(EXCLUDED)))
    assert pairs > 2000 and len(EXCLUDED) <= 0.01 * pairs


def test_pool_reference_and_bounds():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 5, 7)).astype(np.float32)
    out, bound = rp.seq_avg_pool_ref(x, 0.5)
    s = np.zeros((3, 7), np.float32)
    for t in range(5):
        s = s + x[:, t]
    got = np.float32(0.5) * (s / np.float32(5))
    assert (np.abs(got - out) <= bound).all() and (np.abs(got * np.float32(1.001) - out) > bound).any()
    dx0 = rng.standard_normal((3, 5, 7)).astype(np.float32)
    dout = rng.standard_normal((3, 7)).astype(np.float32)
    ref, b = rp.seq_avg_pool_bwd_ref(dout, 0.5, 5, dx0)
    got = dx0 + (np.float32(0.5) * dout / np.float32(5))[:, None, :]
    assert (np.abs(got - ref) <= b).all()
    assert (np.abs(dx0 - ref) > b).any()
