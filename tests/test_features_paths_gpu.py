"""
Every dispatch path, instantiation and tile split of csrc/features.hip against the float64 oracle, element by element.

The rows are oracle/features_paths_np.PATHS (tests/test_oracle_features_paths.py proves on the CPU what each selects; here the
restated dispatch is evaluated again with the device's own CU count and must still select it).  Every output lies in a
NaN-filled guarded buffer (tests/guarded.py), batch gaps hold NaN before and after, signals lie in rows with NaN between N and
sig_stride and behind the last row, so that an over-read that reaches arithmetic shows up as NaN.  Two data sets per case: 0.1 N(0, 1),
and a 440 Hz tone at 0.5 over noise at 1e-4, whose small bins the whole-tensor tolerances of test_features_gpu.py cannot see.

Bounds: oracle/features_paths_np.py, section 3 of its docstring (complex bin 34 u sum |w x| plus the window tables' computed
difference, power, mel, log-mel, MFCC propagated from it; generic kernels sqrt(2) (Leff + 2) u sum |w x|).  power != 2 runs
__powf, a fast-math intrinsic whose error no document of the toolchain states: those cases keep the project's tolerances, 2e-5 of the utterance's
largest value for spectrogram and mel, 1e-3 for log-mel and MFCC.  Log-mel is judged twice: against the oracle with the
propagated bound, and against float64 ln(mel_device + 1e-6) of the MEL kind's output on the same input with `ln_pos_bound`
(twice the 1 ulp features.hip claims for v_log_f32).

Exact relations (section 4 there): shadow == bf16(out), PCM == convert-then-float, an utterance's output alone == in any batch
== at any batch position == from run to run, gaps untouched, B = 0 and T = 0 leave the buffers alone.

Non-finite contract (section 5): the flag is set iff the oracle's output has a non-finite value; the frames that turn non-finite
are exactly `lost_frames` -- the owners of the poisoned sample and the earlier frames whose 416 / 512 loaded samples reach a
sample a LATER frame owns (pinned as it is: the utterance fails either way); every other frame keeps the bits of the clean run.
A sample behind the last frame, zero-weighted samples 15 920 (streaming, N = 16 000) and 1 600 (round-1, N = 1 650) included, is
read by nothing.

Each case prints its largest err / bound as a RATIO line (pytest -s).
"""
import numpy as np
import pytest
import torch

from guarded import NAN_BITS, Guarded
from oracle import features_paths_np as fp

pytestmark = pytest.mark.gpu

CHUNK = 8               # utterances per launch of the bit-identity runs of the large batches


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio
    e = Env()
    e.nv, e.audio, e.lib = nv, audio, nv.lib
    e.ncu = torch.cuda.get_device_properties(0).multi_processor_count
    e.win = {}
    return e


def _win(env, L):
    if L not in env.win:
        env.win[L] = fp.host_window(env.lib, L)
    return env.win[L]


def _plan(env, kw):
    return env.audio.get_plan(kw["sample_rate"], kw["L"], kw["S"], kw["nfft"], kw["power"], kw["M"], kw["fmin"], kw["fmax"],
                              kw["coef_begin"], kw["coef_end"])


def _rows(host, stride, misalign=False):
    """host [B, N] -> a device view [B, N] whose rows lie `stride` apart; NaN (float) / -32768 (int16) between N and stride and in
    the 1 024 samples behind the last row; misalign: the whole buffer one float past a multiple of 16 bytes"""
    from lidbox_amd.testutil import device_copy
    B, N = host.shape
    if host.dtype == np.int16:
        buf = np.full(B * stride + 1024, -32768, np.int16)
        buf[:B * stride].reshape(B, stride)[:, :N] = host
        t = torch.from_numpy(buf).cuda()
        assert not misalign and t.data_ptr() % 16 == 0
    else:
        buf = np.full(B * stride + 1024, np.nan, np.float32)
        buf[:B * stride].reshape(B, stride)[:, :N] = host
        t = device_copy(buf, misalign=misalign)
    return t[:B * stride].view(B, stride)[:, :N]


class Run:
    pass


def _run(env, plan, kind, sig, gap=0, out_shift=0, out16=False, flag=True):
    """one call into guarded buffers: .out [B, T, C] numpy, .dev the device payload [B, T * C], .flag, shadow and gaps checked"""
    B, N = sig.shape
    T, C = plan.num_frames(N), plan.channels(kind)
    bs = T * C + gap
    r = Run()
    g = Guarded((B * bs,), shift=out_shift)
    out = g.view.as_strided((B, T, C), (bs, C, 1))
    g16 = Guarded((B * bs,), dtype=torch.bfloat16) if out16 else None
    fl = torch.zeros(1, dtype=torch.int32, device="cuda") if flag else None
    plan.run(kind, sig, out=out, out_batch_stride=bs if gap else 0, out16=g16.view if out16 else None, nonfinite=fl)
    torch.cuda.synchronize()
    g.check()
    full = g.view.view(B, bs)
    r.dev = full[:, :T * C]
    r.out = r.dev.cpu().numpy().reshape(B, T, C)
    r.flag = int(fl.item()) if flag else None
    if gap:
        assert bool((full[:, T * C:].view(torch.int32) == NAN_BITS).all()), "batch gap overwritten"
    if out16:
        g16.check()
        f16 = g16.view.view(B, bs)
        assert torch.equal(f16[:, :T * C].view(torch.int16), r.dev.to(torch.bfloat16).view(torch.int16)), "shadow != bf16(out)"
        if gap:
            assert bool((f16[:, T * C:].view(torch.int16) == NAN_BITS >> 16).all()), "shadow gap overwritten"
    return r


def _judge(tag, p, kind, got, ref, generic=False):
    """got [b, T, C] against the stage's reference, element by element"""
    want, bound = fp.stage(ref, kind)
    assert got.shape == want.shape and np.isfinite(got).all(), tag
    err = np.abs(got.astype(np.float64) - want)
    if p.power == 2.0:
        # a band without weights (cnt = 0) is an exact zero with a zero bound: there the error must be zero
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        print("\nRATIO gpu %s %s%s err/bound=%.4f" % (tag, fp.KIND_NAMES[kind], " generic" if generic else "", ratio.max()))
        assert ratio.max() <= 1.0, (tag, ratio.max(), np.unravel_index(ratio.argmax(), err.shape))
    elif kind in (fp.SPEC, fp.MEL):
        rel = float((err / np.abs(want).max(axis=(1, 2), keepdims=True)).max())
        print("\nRATIO gpu %s %s powf rel=%.3g of %.0e" % (tag, fp.KIND_NAMES[kind], rel, fp.TOL_POWF_REL))
        assert rel <= fp.TOL_POWF_REL, (tag, rel)
    else:
        print("\nRATIO gpu %s %s powf abs=%.3g of %.0e" % (tag, fp.KIND_NAMES[kind], err.max(), fp.TOL_POWF_LOG))
        assert err.max() <= fp.TOL_POWF_LOG, (tag, err.max())


def _host_signal(r, B, ds):
    src16 = bool(r["call"].get("src16"))
    x = fp.dataset(ds, B, r["N"], [len(r["name"]), r["N"], B], r["plan"]["sample_rate"])
    if src16:
        pcm = np.round(x * 32767.0).astype(np.int16)
        return pcm, pcm.astype(np.float64) / 32768.0
    return x, x.astype(np.float64)


BIG = ("split_16ncu+5", "split_16ncu+5_spec", "r1_iters2")


# ---------------------------------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("ds", fp.DATASETS)
@pytest.mark.parametrize("r", fp.PATHS, ids=lambda r: r["name"])
def test_row_against_the_oracle(env, r, ds):
    p, d, B = fp.resolve(r, env.lib, env.ncu)
    assert fp.check_expect(r, p, d) == [], (env.ncu, d)
    c, kind = r["call"], r["kind"]
    plan = _plan(env, r["plan"])
    assert plan.fused == p.fused_ok
    host, x64 = _host_signal(r, B, ds)
    sig = _rows(host, c["sig_stride"], misalign=bool(c.get("sig_misalign")))
    assert (sig.data_ptr() % 16 == 4) == bool(c.get("sig_misalign"))
    generic = not p.fused_ok
    run = _run(env, plan, kind, sig, gap=c.get("gap", 0), out_shift=c.get("out_shift", 0), out16=bool(c.get("out16")))
    assert run.flag == 0
    if r["name"] in BIG:
        # the oracle on at most 64 utterances: the first and last of the first, a middle and the last workgroup's chunk, and others
        tpw, nwg = d["tiles_per_wg"], d["nwg"]
        pick = set()
        for chunk in (0, nwg // 2, nwg - 1):
            pick |= {chunk * tpw, min((chunk + 1) * tpw, B) - 1}
        pick |= set(np.random.default_rng(B).integers(0, B, 64 - len(pick)).tolist())
        pick = sorted(pick)
        # every utterance bit-identical to itself in a batch of CHUNK through the same kernel (same alignment, same instantiation)
        small = torch.cat([plan.run(kind, sig[b0:b0 + CHUNK]).reshape(-1, run.dev.shape[1]) for b0 in range(0, B, CHUNK)])
        assert fp.dispatch(p, kind, CHUNK, r["N"], env.ncu, sig_align=4 if c.get("sig_misalign") else 0, sig_stride=c["sig_stride"])["targs"] == d["targs"]
        assert torch.equal(small.view(torch.int32), run.dev.view(torch.int32)), "an utterance depends on its batch"
    else:
        pick = list(range(B))
    ref = fp.reference(p, x64[pick], _win(env, p.L), generic=generic, csr=not p.seg_ok)
    _judge("%s %s" % (r["name"], ds), p, kind, run.out[pick], ref, generic)
    if c.get("src16"):
        # PCM == convert-then-float, through the float instantiation of the same kernel (rows of the same stride)
        conv = env.audio.pcm16_to_float(sig.contiguous().reshape(-1), 1).reshape(B, r["N"])
        assert np.array_equal(conv.cpu().numpy().astype(np.float64), x64)
        fsig = _rows(conv.cpu().numpy(), c["sig_stride"])
        frun = _run(env, plan, kind, fsig)
        assert torch.equal(frun.dev.view(torch.int32), run.dev.view(torch.int32)), "PCM != convert-then-float"


def test_the_work_split_reaches_every_branch_on_this_device(env):
    """from the device's own CU count: one wave per workgroup, 2 <= tiles_per_wg <= waves, tiles_per_wg past the first hand-out of
    s_next, a short last workgroup, nwg both a multiple of 8 and not (the remainder branch of xcd_chunk_id)"""
    d = {r["name"]: fp.resolve(r, env.lib, env.ncu)[1] for r in fp.PATHS if r["name"].startswith("split_")}
    assert any(v["waves"] == 1 and v["nwg"] > 1 for v in d.values())
    assert any(2 <= v["tiles_per_wg"] <= v["waves"] for v in d.values())
    assert any(v["tiles_per_wg"] > v["waves"] == 16 for v in d.values())
    assert any(v["last_wg_tiles"] < v["tiles_per_wg"] for v in d.values())
    assert any(v["nwg"] % 8 for v in d.values()) and any(v["nwg"] % 8 == 0 and v["nwg"] >= 8 for v in d.values())


# ---------------------------------------------------------------------------------------------------- ln_pos against the device's mel
LN_ROWS = ("stream_LOGMEL_p2", "stream_L512", "r1_LOGMEL_p2", "csr_vec4_LOGMEL", "csr_scalar_LOGMEL", "fused_M64")


@pytest.mark.parametrize("ds", fp.DATASETS)
@pytest.mark.parametrize("name", LN_ROWS)
def test_logmel_is_ln_of_the_device_mel(env, name, ds):
    """LOGMEL and MEL run the same sums (segmel_tile, or the CSR loop), so log-mel must be ln_pos of the MEL kind's output: judged
    against float64 ln(mel_device + 1e-6) with twice the claimed error of v_log_f32 (the CSR loop calls __logf: the same instruction
    plus a denormal rescue that never triggers at >= 1e-6)."""
    r = next(r for r in fp.PATHS if r["name"] == name)
    p, d, B = fp.resolve(r, env.lib, env.ncu)
    plan = _plan(env, r["plan"])
    host, x64 = _host_signal(r, B, ds)
    sig = _rows(host, r["call"]["sig_stride"], misalign=bool(r["call"].get("sig_misalign")))
    mel32 = _run(env, plan, fp.MEL, sig).out
    mel = mel32.astype(np.float64)
    logmel = _run(env, plan, fp.LOGMEL, sig).out.astype(np.float64)
    v = mel + np.float64(np.float32(1e-6))
    err = np.abs(logmel - np.log(v))
    ratio = float((err / fp.ln_pos_bound(v)).max())
    # measured, not asserted: v_log_f32 alone, against ln of the float32 sum the device forms (numpy's float32 addition is the
    # same correctly rounded operation), in units of the claimed ulp of log2 x plus the two roundings of the product with ln 2
    v32 = (mel32 + np.float32(1e-6)).astype(np.float64)
    own = np.abs(logmel - np.log(v32)) / (fp.ulp32(np.log2(v32)) * np.log(2.0) + 2.0 * fp.U * np.abs(np.log(v32)))
    print("\nRATIO gpu ln_pos %s %s err/bound=%.4f, v_log_f32 alone %.3f of its claim" % (name, ds, ratio, float(own.max())))
    assert ratio <= 1.0, (name, ratio)


# ---------------------------------------------------------------------------------------------------- exact relations
@pytest.mark.parametrize("kind", (fp.SPEC, fp.MEL, fp.LOGMEL, fp.MFCC), ids=lambda k: fp.KIND_NAMES[k])
@pytest.mark.parametrize("misalign", (False, True), ids=("stream", "round1"))
def test_an_utterance_alone_in_any_batch_at_any_position_and_again(env, kind, misalign):
    plan = _plan(env, fp._plan_kw())
    B, N = 5, 400 + 18 * 160            # N % 4 = 0: a lone utterance carries sig_stride = N and must stay on the same kernel
    stride = N + 4
    x = fp.dataset("normal", B, N, [kind, 77])
    a = _run(env, plan, kind, _rows(x, stride, misalign)).dev
    again = _run(env, plan, kind, _rows(x, stride, misalign)).dev
    assert torch.equal(a.view(torch.int32), again.view(torch.int32)), "run to run"
    rev = _run(env, plan, kind, _rows(x[::-1].copy(), stride, misalign)).dev
    assert torch.equal(a.view(torch.int32), rev.flip(0).view(torch.int32)), "batch position"
    pair = _run(env, plan, kind, _rows(x[[3, 1]], stride, misalign)).dev
    assert torch.equal(a[[3, 1]].view(torch.int32), pair.view(torch.int32)), "another batch"
    for b in range(B):
        one = _run(env, plan, kind, _rows(x[b:b + 1], stride, misalign)).dev
        assert torch.equal(one.view(torch.int32), a[b:b + 1].view(torch.int32)), ("alone", b)


def test_empty_calls_leave_the_buffers_alone(env):
    """B = 0 and T = 0 (N < frame_length) through the C ABI itself: status 0, nothing written, no flag"""
    nv = env.nv
    plan = _plan(env, fp._plan_kw())
    sig = _rows(fp.dataset("normal", 2, 399, 5), 400)
    for kind in (fp.SPEC, fp.LOGMEL):
        for B, N in ((0, 399), (2, 399), (0, 16000)):
            g, g16 = Guarded((64,)), Guarded((64,), dtype=torch.bfloat16)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            nv.check(nv.lib.lidbox_extract_features_fwd_ex(plan.handle, kind, nv.ptr(sig), nv.SRC_F32, B, N, max(N, 400), g.ptr, 0, g16.ptr,
                                                           nv.ptr(flag), None, 0, nv.current_stream()))
            torch.cuda.synchronize()
            assert np.isnan(g.numpy()).all() and np.isnan(g16.numpy()).all() and int(flag.item()) == 0


def test_pcm_with_another_power_is_converted_by_the_python_layer_and_refused_by_the_c_abi(env):
    nv = env.nv
    kw = fp._plan_kw(power=1.0)
    plan = _plan(env, kw)
    x = fp.dataset("tone", 2, 2000, 3)
    pcm = np.round(x * 32767.0).astype(np.int16)
    sig = _rows(pcm, 2000)
    got = plan.run(fp.LOGMEL, sig)
    want = plan.run(fp.LOGMEL, torch.from_numpy(pcm.astype(np.float32) / np.float32(32768.0)).cuda())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    g = Guarded((2 * 11 * 40,))
    rc = nv.lib.lidbox_extract_features_fwd_ex(plan.handle, fp.LOGMEL, nv.ptr(sig), nv.SRC_PCM16, 2, 2000, 2000, g.ptr, 0, None, None, None, 0,
                                               nv.current_stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"16-bit PCM" in nv.lib.lidbox_hip_last_error() and np.isnan(g.numpy()).all()


# ---------------------------------------------------------------------------------------------------- non-finite contract
def _contract(env, row_name, N, stride, positions, misalign=False):
    r = next(r for r in fp.PATHS if r["name"] == row_name)
    kind = r["kind"]
    p, _, _ = fp.resolve(r, env.lib, env.ncu)
    plan = _plan(env, r["plan"])
    B, b = 3, 1
    d = fp.dispatch(p, kind, B, N, env.ncu, sig_align=4 if misalign else 0, sig_stride=stride)
    assert (d["kernel"], d["targs"]) == (r["expect"]["kernel"], r["expect"]["targs"])
    T = fp.num_frames(N, p.L, p.S)
    x = fp.dataset("normal", B, N, [N, kind])
    clean = _run(env, plan, kind, _rows(x, stride, misalign))
    assert clean.flag == 0
    _judge("contract %s clean" % row_name, p, kind, clean.out, fp.reference(p, x.astype(np.float64), _win(env, p.L), csr=not p.seg_ok))
    for pos in positions:
        for v in (np.nan, np.inf):
            y = x.copy()
            y[b, pos] = v
            run = _run(env, plan, kind, _rows(y, stride, misalign))
            want, _ = fp.stage(fp.reference(p, y.astype(np.float64), _win(env, p.L), csr=not p.seg_ok), kind)
            oracle_bad = not np.isfinite(want).all()
            assert oracle_bad == any(t * p.S <= pos < t * p.S + p.L for t in range(T))
            assert (run.flag != 0) == oracle_bad, (row_name, pos, v, run.flag)
            lost = fp.lost_frames(p, d, N, pos)
            got_bad = {t for t in range(T) if not np.isfinite(run.out[b, t]).all()}
            assert got_bad == lost, (row_name, pos, v, sorted(got_bad), sorted(lost))
            keep = np.ones((B, T), bool)
            keep[b, sorted(lost)] = False
            assert np.array_equal(run.out[keep].view(np.int32), clean.out[keep].view(np.int32)), (row_name, pos, v)


@pytest.mark.parametrize("name", ("stream_SPECTROGRAM_p2", "stream_MEL_p2", "stream_LOGMEL_p2", "stream_MFCC_p2"))
def test_non_finite_contract_streaming_kernel(env, name):
    """N = 16 000: 98 frames, the last owns 15 520 .. 15 919 and loads up to 15 935.  15 920 .. 15 999 belong to no frame."""
    _contract(env, name, 16000, 16000, (0, 399, 400, 416, 8000, 15519, 15600, 15919, 15920, 15923, 15935, 15936, 15999))


@pytest.mark.parametrize("name", ("stream_L512", "stream_L420"))
def test_non_finite_contract_streaming_kernel_nl16(env, name):
    L = 512 if name.endswith("512") else 420
    N = L + 20 * 160 + 100
    _contract(env, name, N, N, (0, L - 1, L, L + 160 * 20 - 1, L + 160 * 20, L + 160 * 20 + 3, N - 1))


@pytest.mark.parametrize("name", ("csr_vec4_MEL", "csr_vec4_LOGMEL", "csr_vec4_MFCC"))
def test_non_finite_contract_round1_kernel_aligned(env, name):
    """VEC4 = true (the census plan).  N = 1 650: 8 frames, (T - 1) S + L = 1 520, 7 S + 512 = 1 632 <= N: sample 1 600 is behind the
    last frame and inside what an interior tile would load.  N = 3 010: 17 frames, tiles 0 and 1 interior, tile 2 guarded."""
    _contract(env, name, 1650, 1652, (0, 1119, 1519, 1520, 1600, 1631, 1632, 1649))
    _contract(env, name, 3010, 3012, (0, 990, 1000, 2559, 2560, 2959, 2960, 2990, 3009))


@pytest.mark.parametrize("name", ("r1_SPECTROGRAM_p2", "r1_LOGMEL_p2", "r1_MFCC_p2"))
def test_non_finite_contract_round1_kernel_misaligned(env, name):
    _contract(env, name, 1650, 1652, (0, 399, 400, 1519, 1520, 1600, 1649), misalign=True)


# ---------------------------------------------------------------------------------------------------- generic side: the flag pass
def test_nonfinite_rows_kernel_second_grid_stride_trip(env):
    """fft_length 1 024: (T = 98, F = 513) = 50 274 values per utterance, 64 workgroups x 256 threads per trip: the last element
    is read in the fourth trip.  A NaN planted there (the last sample of the last frame reaches every bin) and a clean run."""
    kw = fp._plan_kw(nfft=1024)
    plan = _plan(env, kw)
    W = fp.host_mel_matrix(env.lib, 40, 513, 16000, 0.0, 8000.0)
    p = fp.make_plan(W, 16000, 400, 160, nfft=1024)
    assert fp.dispatch(p, fp.SPEC, 1, 16000, env.ncu)["flag_trips"] == 4 and not plan.fused
    x = fp.dataset("normal", 1, 16000, 11)
    run = _run(env, plan, fp.SPEC, _rows(x, 16000))
    assert run.flag == 0
    _judge("generic_1024 normal", p, fp.SPEC, run.out, fp.reference(p, x.astype(np.float64), _win(env, 400), generic=True), True)
    # a poisoned last frame turns values 49 761 .. 50 273 NaN, the last element among them: all of them lie in the fourth trip
    # (49 152 ..), so a flag pass that stops after its first trips reports a clean tensor
    y = x.copy()
    y[0, 15919] = np.nan
    bad = _run(env, plan, fp.SPEC, _rows(y, 16000))
    assert bad.flag != 0 and np.isnan(bad.out[0, 97]).all() and np.isfinite(bad.out[0, :97]).all()
    z = x.copy()
    z[0, 15920] = np.nan                    # behind the last frame
    assert _run(env, plan, fp.SPEC, _rows(z, 16000)).flag == 0
