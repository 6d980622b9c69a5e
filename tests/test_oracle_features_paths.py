"""
Pins oracle/features_paths_np.py on the CPU (no device, no launches):
  1. for every row of its PATHS table, the property the row is there for, computed from the restated plan and dispatch of
     features.hip at several CU counts: a shape that stops selecting its path fails here;
  2. the census of `seg_ok` over a grid of plans: the only plans whose bands do not split into 64 runs have `fmax` above
     Nyquist, and the SEGMEL = false rows use one of them;
  3. the float32 transcription of the tile (16 x 16 transform with the plan's tables, untangling, segmented mel, DCT runs)
     against the float64 reference on both data sets: inside the bounds, and the bounds not vacuous;
  4. the small pieces: xcd_chunk_id is a bijection, ulp32 / ln_pos_bound, the tail arithmetic of the non-finite contract.
"""
import numpy as np
import pytest

from oracle import features_np as fo
from oracle import features_paths_np as fp


@pytest.fixture(scope="module")
def lib():
    from lidbox_amd import build
    build.build(verbose=False)              # hipcc cross-compiles for gfx950 without a GPU
    from lidbox_amd import _native
    return _native.lib


# ---------------------------------------------------------------------------------------------------- 1. PATHS
@pytest.mark.parametrize("r", fp.PATHS, ids=lambda r: r["name"])
def test_every_row_selects_what_it_is_there_for(lib, r):
    for ncu in (256, 304, 120, 64):
        p, d, B = fp.resolve(r, lib, ncu)
        assert d is not None and d["refused"] is None
        assert fp.check_expect(r, p, d) == [], (ncu, d["kernel"], d.get("targs"))
        if d["kernel"] == "feat512_stream_kernel":
            # the split covers every tile once, in workgroups of tiles_per_wg but the last
            assert (d["nwg"] - 1) * d["tiles_per_wg"] + d["last_wg_tiles"] == d["ntiles"] and 1 <= d["last_wg_tiles"] <= d["tiles_per_wg"]
            assert d["nwg"] <= ncu and 1 <= d["waves"] <= 16
            assert fp.stream_table_bytes(p, r["kind"]) + d["waves"] * fp.WAVE_SCRATCH <= fp.LDS_BYTES


def test_row_names_are_unique_and_every_instantiation_family_has_a_row(lib):
    names = [r["name"] for r in fp.PATHS]
    assert len(set(names)) == len(names)
    seen = set()
    for r in fp.PATHS:
        p, d, _ = fp.resolve(r, lib, 256)
        seen.add((d["kernel"],) + tuple(d["targs"]))
    want = fp.reachable()
    assert len(want) == 24 + 14 + 6 + 1
    assert seen == want, (sorted(want - seen), sorted(seen - want))


def test_the_work_split_properties_at_256_cus(lib):
    """what the split rows reach on the 256 CUs of an MI355X (the GPU module asserts the same from the device's own count)"""
    d = {r["name"]: fp.resolve(r, lib, 256)[1] for r in fp.PATHS if r["name"].startswith("split_")}
    assert (d["split_1"]["nwg"], d["split_1"]["waves"]) == (1, 1)
    assert d["split_ncu-1"]["nwg"] == 255 and d["split_ncu-1"]["nwg"] % 8 == 7            # the remainder branch of xcd_chunk_id
    assert d["split_ncu"]["nwg"] == 256
    assert (d["split_ncu+1"]["tiles_per_wg"], d["split_ncu+1"]["nwg"], d["split_ncu+1"]["last_wg_tiles"]) == (2, 129, 1)      # a short last workgroup
    assert (d["split_2ncu+3"]["tiles_per_wg"], d["split_2ncu+3"]["nwg"], d["split_2ncu+3"]["last_wg_tiles"]) == (3, 172, 2)
    big = d["split_16ncu+5"]
    assert (big["tiles_per_wg"], big["waves"], big["nwg"], big["last_wg_tiles"]) == (17, 16, 242, 4)      # one tile past the first hand-out of s_next
    assert big["nwg"] % 8 == 2
    r1 = fp.resolve(next(r for r in fp.PATHS if r["name"] == "r1_iters2"), lib, 256)[1]
    assert (r1["iters"], r1["tiles_per_wg"], r1["nwg"]) == (2, 8, 1537)
    assert fp.dispatch(fp.resolve(fp.PATHS[0], lib, 256)[0], fp.LOGMEL, 12288, fp.N8, 256, sig_align=4)["iters"] == 1


def test_store_branches_and_dct_plans(lib):
    rows = {r["name"]: r for r in fp.PATHS}
    p, d, _ = fp.resolve(rows["store_realigned_shadow"], lib, 256)
    assert d["store"] == ["scalar", "scalar", "vec", "vec"] and d["shadow"] == "kernel"
    plans = {}
    for name, r in rows.items():
        if r["kind"] == fp.MFCC:
            p, d, _ = fp.resolve(r, lib, 256)
            plans[(p.ncoef, p.M)] = (p.dct_runs, p.dct_len)
    assert plans[(12, 40)] == (5, 8) and plans[(1, 40)] == (40, 1) and plans[(20, 40)] == (3, 14) and plans[(13, 13)] == (4, 4)
    assert plans[(25, 25)] == (2, 13)             # (40, 25): coef_end is cut to M; an ODD dct_len under CH = 2
    assert plans[(16, 16)] == (4, 4)              # (64, 16): likewise
    assert plans[(12, 45)] == (5, 9)              # DCT_REGS false on the round-1 kernel
    assert plans[(16, 64)] == (4, 16) and plans[(13, 45)] == (4, 12)
    assert any(v[1] % 2 == 1 and v[1] > 1 for v in plans.values())


def test_dispatch_edges(lib):
    p = fp.resolve(fp.PATHS[0], lib, 256)[0]
    assert fp.dispatch(p, fp.LOGMEL, 0, 2000, 256) is None and fp.dispatch(p, fp.LOGMEL, 3, 399, 256) is None
    assert fp.dispatch(p, fp.LOGMEL, 2, 2000, 256, src16=True, sig_align=2)["refused"] == "streaming"
    W = fp.host_mel_matrix(lib, 40, 257, 16000, 0.0, 8000.0)
    p1 = fp.make_plan(W, 16000, 400, 160, power=1.0)
    assert fp.dispatch(p1, fp.LOGMEL, 2, 2000, 256, src16=True)["refused"] == "streaming"
    W1k = fp.host_mel_matrix(lib, 40, 513, 16000, 0.0, 8000.0)
    g = fp.dispatch(fp.make_plan(W1k, 16000, 400, 160, nfft=1024), fp.SPEC, 1, 16000, 256)
    assert (g["Leff"], g["nwg"], g["ntiles"]) == (400, 98, 98)                             # one workgroup per frame
    assert g["kernel"] == "pow2_fft_spectrogram_kernel" and g["flag_trips"] == 4          # T = 98, F = 513: 50 274 values, 64 x 256 per trip
    assert fp.dispatch(fp.make_plan(W1k, 16000, 400, 160, nfft=1024), fp.SPEC, 1, 16000, 256, src16=True)["refused"] == "fused"
    # M ncoef: 1 024 is fused, 1 088 is not; nnz never limits a 257-bin plan (<= 2 bands per bin)
    W64 = fp.host_mel_matrix(lib, 64, 257, 16000, 0.0, 8000.0)
    assert fp.make_plan(W64, 16000, 400, 160, coef_begin=0, coef_end=16).fused_ok
    assert not fp.make_plan(W64, 16000, 400, 160, coef_begin=0, coef_end=17).fused_ok
    assert fp.make_plan(W64, 16000, 512, 160).fused_ok and not fp.make_plan(W64, 16000, 513, 160).fused_ok


# ---------------------------------------------------------------------------------------------------- 2. census
def test_census_of_seg_ok(lib):
    """1 296 plans.  Not seg_ok: only plans with fmax above Nyquist; every seg_len 1 .. 32 but 28 occurs; bands without weights occur."""
    notok, lens, zero = [], set(), 0
    for sr in (8000, 16000, 22050, 44100):
        for M in (1, 2, 3, 4, 5, 8, 10, 13, 16, 20, 23, 25, 32, 40, 45, 48, 56, 64):
            for fmin in (0.0, 20.0, 300.0):
                for fmax in (sr / 8, sr / 4, sr / 2 - 200, sr / 2, sr, 4 * sr):
                    st, cnt, nnz, ok, sl, steps, lanes, sw = fp.mel_segments(fp.host_mel_matrix(lib, M, 257, sr, fmin, fmax))
                    assert nnz <= 1024 and cnt.max() <= 257
                    zero += bool((cnt == 0).any())
                    if ok:
                        lens.add(sl)
                        assert len(lanes) <= 64 and steps <= 6 and (1 << steps) >= max(l[3] for l in lanes)
                        assert sl == 1 or sum(max(1, -(-c // (sl - 1))) for c in cnt) > 64            # the smallest that fits
                    else:
                        notok.append((sr, M, fmin, fmax))
    assert len(notok) == 8 and all(fmax > sr / 2 and M == 64 for sr, M, fmin, fmax in notok), notok
    assert (16000, 64, 0.0, 64000) in notok
    assert lens >= set(range(1, 28)) | {29, 30, 31, 32} and zero > 0
    kw = fp._plan_kw(**fp.CENSUS_PLAN)
    assert not fp.make_plan(fp.host_mel_matrix(lib, kw["M"], 257, kw["sample_rate"], kw["fmin"], kw["fmax"]), 16000, 400, 160).seg_ok


def test_segments_reassemble_the_matrix(lib):
    """the lane table and the padded weights are the matrix: scattering every lane's run back gives W, and each band's lanes are
    consecutive with indices 0 .. ns - 1"""
    for sr, M, fmin, fmax in ((16000, 40, 0.0, 8000.0), (8000, 23, 0.0, 2000.0), (8000, 1, 0.0, 1000.0), (8000, 64, 0.0, 32000.0)):
        W = fp.host_mel_matrix(lib, M, 257, sr, fmin, fmax)
        st, cnt, nnz, ok, sl, steps, lanes, sw = fp.mel_segments(W)
        back = np.zeros_like(W)
        for lane, (band, b0, idx, ns) in enumerate(lanes):
            for j in range(sl):
                if sw[j, lane] != 0:
                    back[b0 + j, band] = sw[j, lane]
            assert lanes[lane - idx][0] == band and lanes[lane - idx][2] == 0 and idx < ns
        assert ok and np.array_equal(back, W) and nnz == sum(cnt)
        assert not sw[:, len(lanes):].any()


# ---------------------------------------------------------------------------------------------------- 3. transcription and bounds
TRANSCRIPTION_PLANS = [dict(), dict(M=23, sample_rate=8000, fmax=2000.0), dict(M=64, coef_begin=0, coef_end=16), dict(L=512), dict(L=4, S=4)]


@pytest.mark.parametrize("ds", fp.DATASETS)
@pytest.mark.parametrize("plan", TRANSCRIPTION_PLANS, ids=str)
def test_float32_transcription_stays_inside_non_vacuous_bounds(lib, plan, ds):
    kw = fp._plan_kw(**plan)
    W = fp.host_mel_matrix(lib, kw.pop("M"), 257, kw["sample_rate"], kw.pop("fmin"), kw.pop("fmax"))
    p = fp.make_plan(W, **kw)
    win = fp.host_window(lib, p.L)
    tw256, tw512 = fp.twiddles()
    x = fp.dataset(ds, 3, p.L + 40 * p.S, [p.L, p.M], p.sample_rate)
    ref = fp.reference(p, x.astype(np.float64), win)
    fr = fo.frame(x, p.L, p.S).reshape(-1, p.L)
    Xr, Xi, P = fp.tile_f32(fr, win, tw256, tw512)
    mel = fp.segmel_f32(p, P)
    logmel = np.log((mel + np.float32(1e-6)).astype(np.float32)).astype(np.float32)      # numpy's float32 log: correctly rounded to an ulp
    mfcc = fp.segdct_f32(p, logmel)
    flat = lambda a: a.reshape(-1, a.shape[-1])
    ratios = {
        "X": np.abs((Xr.astype(np.float64) + 1j * Xi) - flat(ref.X)) / flat(ref.eX),
        "P": np.abs(P - flat(ref.P)) / flat(ref.eP),
        "mel": np.abs(mel - flat(ref.mel)) / flat(ref.eMel),
        "logmel": np.abs(logmel - flat(ref.logmel)) / flat(ref.eLog),
        "mfcc": np.abs(mfcc - flat(ref.mfcc)) / flat(ref.eMfcc),
    }
    worst = {k: float(v.max()) for k, v in ratios.items()}
    print("\nRATIO cpu", plan, ds, " ".join("%s=%.4f" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (k, v)
    # not vacuous: a bound 1 000 times the error it covers would pass a kernel that drops a bin 60 dB below the peak
    assert worst["X"] >= 1e-2 and worst["P"] >= 1e-2 and worst["mel"] >= 5e-3 and worst["logmel"] >= 5e-3 and worst["mfcc"] >= 5e-4
    # and what the old whole-tensor tolerance hid: on the tone the bound of the smallest bin is below a hundredth of 2e-5 of the largest value
    if ds == "tone":
        assert (flat(ref.eP).min(axis=1) < 1e-2 * 2e-5 * flat(ref.P).max(axis=1)).all()


def test_transcription_is_a_transform(lib):
    """one impulse per position: the transcription's bins are the window weight times the twiddle, to float32 rounding (the 1 / 2 in
    the window table is the 1 / 2 the untangling leaves out)"""
    win = fp.host_window(lib, 512)
    tw256, tw512 = fp.twiddles()
    fr = np.eye(512, dtype=np.float32)[[0, 1, 2, 17, 255, 256, 399, 511]]
    Xr, Xi, P = fp.tile_f32(fr, win, tw256, tw512)
    n = np.array([0, 1, 2, 17, 255, 256, 399, 511])[:, None]
    want = win[n[:, 0]].astype(np.float64)[:, None] * np.exp(-2j * np.pi * n * np.arange(257)[None] / 512)
    assert np.abs((Xr + 1j * Xi) - want).max() <= 40 * fp.U


# ---------------------------------------------------------------------------------------------------- 4. small pieces
def test_xcd_chunk_id_is_a_bijection():
    for nwg in list(range(1, 40)) + [129, 172, 242, 255, 256, 304]:
        assert sorted(fp.xcd_chunk_id(b, nwg) for b in range(nwg)) == list(range(nwg))
    # the remainder branch: with nwg % 8 = r, XCDs below r own one chunk more
    assert [fp.xcd_chunk_id(b, 10) for b in range(10)] == [0, 2, 4, 5, 6, 7, 8, 9, 1, 3]


def test_ulp_and_ln_bound():
    assert fp.ulp32(1.0) == 2.0 ** -23 and fp.ulp32(1.5) == 2.0 ** -23 and fp.ulp32(-19.9) == 2.0 ** -19 and fp.ulp32(0.75) == 2.0 ** -24
    v = np.array([1e-6, 1e-3, 0.9, 1.0 + 1e-6, 7.0, 3e4])
    b = fp.ln_pos_bound(v)
    assert (b >= 1.05 * fp.U).all() and (b <= 5e-6).all()
    assert fp.ln_pos_bound(1e-6) > fp.ln_pos_bound(1e-6, claim=1.0) > 0


def test_tail_arithmetic_of_the_non_finite_contract(lib):
    """L = 400, S = 160, N = 16 000: 98 frames, the last one owns 15 520 .. 15 919 and its lanes load up to 15 935; with the loads
    bounded at (T - 1) S + L = 15 920 a poisoned 15 920 is lost by no frame, a poisoned 15 919 by the frames that own it, and one
    owned by a later frame also by the earlier frame whose 416 loaded samples reach it."""
    rows = {r["name"]: r for r in fp.PATHS}
    p, d, _ = fp.resolve(rows["stream_LOGMEL_p2"], lib, 256)
    assert fp.num_frames(16000, 400, 160) == 98 and d["reach"] == 416
    assert fp.lost_frames(p, d, 16000, 15920) == set() and fp.lost_frames(p, d, 16000, 15999) == set()
    assert fp.lost_frames(p, d, 16000, 15919) == {97} and fp.lost_frames(p, d, 16000, 15520) == {95, 96, 97}
    assert fp.lost_frames(p, d, 16000, 15610) == {95, 96, 97} and fp.lost_frames(p, d, 16000, 15600) == {95, 96, 97}
    assert fp.lost_frames(p, d, 16000, 400) == {0, 1, 2}         # frame 0 owns 0 .. 399 and loads 0 .. 415
    assert fp.lost_frames(p, d, 16000, 416) == {1, 2}
    # round-1 kernel, aligned rows of the census plan: T = 8 at N = 1 650 has no interior tile once the test is (T - 1) S + L
    pc, dc, _ = fp.resolve(rows["csr_vec4_MEL"], lib, 256)
    assert dc["vec4"] and fp.num_frames(1650, 400, 160) == 8
    assert fp.lost_frames(pc, dc, 1650, 1600) == set() and fp.lost_frames(pc, dc, 1650, 1519) == {7}
    # T = 17: tiles 0 and 1 are interior (512 samples per frame), tile 2 is not
    N = 400 + 16 * 160 + 50
    assert fp.lost_frames(pc, dc, N, 990) == {3, 4, 5, 6} and fp.lost_frames(pc, dc, N, 2959) == {16} and fp.lost_frames(pc, dc, N, 2960) == set()
