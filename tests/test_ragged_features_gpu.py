"""
The ragged feature path on the device: lidbox_extract_features_ragged (the RAGGED form of feat512_stream_kernel), the ragged
CMVN / window normalisation kernels, and the layers above them up to the dataset steps.

The contract at every layer: utterance b of a ragged batch gets what the dense path gives it ALONE, bit for bit.  The dense
reference of the kernel tests is `plan.run` on copies of the utterance in a [G, N] view whose row stride is a multiple of 4, which
makes the dense call select the streaming kernel too (asserted through oracle/features_paths_np.dispatch); the step tests compare
with the same config at `batch_size: 1`.

Oracle: at most 64 utterances per case are judged element by element against the float64 reference with the bounds of
oracle/features_paths_np.py (`fp.reference` / `fp.stage`; power != 2 keeps the project's __powf tolerances, as in
test_features_paths_gpu.py).  The remaining utterances of the large work-split batches are covered by the bit identity with the
dense path, which test_features_paths_gpu.py judges against the same oracle.

Every output lies in a NaN-filled guarded buffer of exact size (tests/guarded.py); the sample buffer holds NaN in every alignment
gap and in the 1 024 samples behind the last utterance, so that a read that reaches arithmetic shows up as NaN.
"""
import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import features_paths_np as fp

pytestmark = pytest.mark.gpu

S = 160
KINDS = (fp.SPEC, fp.MEL, fp.LOGMEL, fp.MFCC)
RAGGED_WAVES = 12               # RAGGED_MAX_WAVES of csrc/features.hip


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    from lidbox_amd import _native as nv
    from lidbox_amd.features import audio, signal_ops
    e = Env()
    e.nv, e.audio, e.sg, e.lib = nv, audio, signal_ops, nv.lib
    e.ncu = torch.cuda.get_device_properties(0).multi_processor_count
    e.cache = {}
    return e


def _plans(env, **kw):
    """(device plan, oracle plan, float32 window) of the census configuration with `kw` changed"""
    kw = fp._plan_kw(**kw)
    key = tuple(sorted(kw.items()))
    if key not in env.cache:
        plan = env.audio.get_plan(kw["sample_rate"], kw["L"], kw["S"], kw["nfft"], kw["power"], kw["M"], kw["fmin"], kw["fmax"],
                                  kw["coef_begin"], kw["coef_end"])
        o = dict(kw)
        W = fp.host_mel_matrix(env.lib, o.pop("M"), o["nfft"] // 2 + 1, o["sample_rate"], o.pop("fmin"), o.pop("fmax"))
        env.cache[key] = (plan, fp.make_plan(W, **o), fp.host_window(env.lib, kw["L"]))
    return env.cache[key]


def _lengths(L):
    """the issue's lengths at frame length L (L = 400: 0, 399, 400, 1520, 1523, 1680, 16000) with the zero-frame utterances first,
    twice in a row in the middle, and last; T = 0, 1, 8, 0, 0, 8, 9, 98, 0"""
    return [0, L, L + 7 * S, L - 1, 0, L + 7 * S + 3, L + 8 * S, L + 97 * S, L - 1]


def _signals(lengths, seed, ds="normal"):
    return [fp.dataset(ds, 1, n, [seed, i, n])[0] if n else np.zeros(0, np.float32) for i, n in enumerate(lengths)]


def _ragged(env, sigs, misalign=False):
    """RaggedSignals over a buffer with NaN in every alignment gap and in the 1 024 samples behind the last utterance"""
    from lidbox_amd.testutil import device_copy
    lengths = np.array([len(s) for s in sigs], np.int64)
    starts, total = env.sg._aligned_starts(lengths)
    buf = np.full(total + 1024, np.nan, np.float32)
    for s, st in zip(sigs, starts):
        buf[int(st):int(st) + len(s)] = s
    flat = device_copy(buf, misalign=misalign)
    assert flat.data_ptr() % 16 == (4 if misalign else 0)
    return env.sg.RaggedSignals(flat, starts, lengths)


def _run_ragged(env, plan, kind, r, python=False):
    """one ragged call into a guarded buffer of exact size -> (out [total_frames, C] device, frame offsets, flag).  The kernel tests
    call the C ABI, which gives every utterance to the kernel; python: FeaturePlan.run_ragged, which falls back to the dense call for
    plans and buffers the kernel does not take and for utterances whose length is no multiple of 4"""
    to, fo = env.sg.ragged_frame_plan(r.lengths_host, plan.frame_length, plan.frame_step)
    g = Guarded((int(fo[-1]), plan.channels(kind)))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    if python:
        out, fo2 = plan.run_ragged(kind, r, out=g.view, nonfinite=flag)
        assert out.data_ptr() == g.view.data_ptr() and np.array_equal(fo, fo2)
    else:
        assert _c_call(env, plan, kind, r, g, flag) == 0, env.nv.last_error()
    torch.cuda.synchronize()
    g.check()
    return g.view, fo, int(flag.item())


def _dense(env, plan, p, kind, rows):
    """the dense call on equal-length utterances `rows` [G, N] plus a copy of the first, rows a multiple of 4 samples apart with NaN
    between them: the streaming kernel -> [G, T, C] device"""
    G, N = rows.shape
    stride = (N + 3) // 4 * 4 + 4
    buf = np.full((G + 1) * stride + 1024, np.nan, np.float32)
    v = buf[:(G + 1) * stride].reshape(G + 1, stride)
    v[:G, :N] = rows
    v[G, :N] = rows[0]
    sig = torch.from_numpy(buf).cuda()[:(G + 1) * stride].view(G + 1, stride)[:, :N]
    assert sig.data_ptr() % 16 == 0
    d = fp.dispatch(p, kind, G + 1, N, env.ncu, sig_stride=stride)
    assert d["kernel"] == "feat512_stream_kernel" and d["targs"][2:4] == (False, False), d
    out = plan.run(kind, sig)
    assert torch.equal(out[G].view(torch.int32), out[0].view(torch.int32))
    return out[:G], d


def _dense_by_length(env, plan, p, kind, sigs):
    """per-utterance dense results: utterances of one length share a launch (the dense path does not depend on the batch:
    test_features_paths_gpu.py) -> list of [T_b, C] device tensors"""
    groups = {}
    for b, s in enumerate(sigs):
        groups.setdefault(len(s), []).append(b)
    C = plan.channels(kind)
    want = [None] * len(sigs)
    for n, idx in groups.items():
        if plan.num_frames(n) == 0:
            for b in idx:
                want[b] = torch.zeros((0, C), device="cuda")
            continue
        out, _ = _dense(env, plan, p, kind, np.stack([sigs[b] for b in idx]))
        for b, o in zip(idx, out):
            want[b] = o
    return want


def _assert_rows_equal(out, fo, want, tag):
    for b, w in enumerate(want):
        got = out[int(fo[b]):int(fo[b + 1])]
        assert got.shape == w.shape, (tag, b, got.shape, w.shape)
        assert torch.equal(got.view(torch.int32), w.view(torch.int32)), (tag, "utterance", b)


def _judge(tag, p, kind, got, ref):
    """got [1, T, C] against the stage's reference, element by element (test_features_paths_gpu._judge)"""
    want, bound = fp.stage(ref, kind)
    assert got.shape == want.shape and np.isfinite(got).all(), tag
    err = np.abs(got.astype(np.float64) - want)
    if p.power == 2.0:
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
        assert ratio.max() <= 1.0, (tag, ratio.max(), np.unravel_index(ratio.argmax(), err.shape))
        return float(ratio.max())
    if kind in (fp.SPEC, fp.MEL):
        rel = float((err / np.abs(want).max(axis=(1, 2), keepdims=True)).max())
        assert rel <= fp.TOL_POWF_REL, (tag, rel)
        return rel / fp.TOL_POWF_REL
    assert err.max() <= fp.TOL_POWF_LOG, (tag, err.max())
    return float(err.max()) / fp.TOL_POWF_LOG


def _judge_utterances(tag, p, win, kind, out, fo, sigs, pick):
    assert len(pick) <= 64
    worst = 0.0
    host = out.cpu().numpy()
    for b in pick:
        if fo[b + 1] == fo[b]:
            continue
        ref = fp.reference(p, sigs[b].astype(np.float64)[None], win)
        worst = max(worst, _judge("%s utt %d" % (tag, b), p, kind, host[int(fo[b]):int(fo[b + 1])][None], ref))
    print("\nRATIO gpu ragged %s %s worst err/bound=%.4f over %d utterances" % (tag, fp.KIND_NAMES[kind], worst, len(pick)))


# ---------------------------------------------------------------------------------------------------- kernel: bit identity + oracle
PLANS = {"L400_p2": dict(), "L512_p2": dict(L=512), "L400_p1.5": dict(power=1.5)}


@pytest.mark.parametrize("ds", fp.DATASETS)
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: fp.KIND_NAMES[k])
@pytest.mark.parametrize("name", sorted(PLANS))
def test_every_utterance_gets_its_dense_bits_and_meets_the_oracle(env, name, kind, ds):
    """the 12 ragged instantiations: four kinds x (NL = 13, NL = 16 at L = 512, power 1.5); every utterance has its dense bits and
    is judged by the oracle.  power 1.5 is judged on the 'normal' set only: for power != 2 the oracle has no propagated bound, only
    the flat __powf tolerances (1e-3 on log-mel), and those cannot hold on the 'tone' set at 98 frames.  Its floor lies 80 dB under
    the peak, so the float32 FFT's own rounding error, which the oracle bounds by eX = 34 u sum |w x| ~ 2e-4 against floor bins of
    |X| ~ 1e-3, is a relative error of the floor bins that no kernel can avoid, and log-mel moves by `power` times that relative
    error (measured here: 1.6e-3, on bits identical to the dense kernel's).  On the 'tone' set power 1.5 keeps the bit identity."""
    plan, p, win = _plans(env, **PLANS[name])
    assert plan.ragged_ok(kind)
    sigs = _signals(_lengths(p.L), len(name), ds)
    r = _ragged(env, sigs)
    assert [plan.num_frames(len(s)) for s in sigs] == [0, 1, 8, 0, 0, 8, 9, 98, 0] and len(sigs[5]) % 4 == 3
    out, fo, flag = _run_ragged(env, plan, kind, r)
    assert flag == 0 and int(fo[-1]) == 124
    _assert_rows_equal(out, fo, _dense_by_length(env, plan, p, kind, sigs), name)
    if p.power == 2.0 or ds == "normal":
        _judge_utterances("%s %s" % (name, ds), p, win, kind, out, fo, sigs, range(len(sigs)))


# ---------------------------------------------------------------------------------------------------- kernel: work split
def _split(env, plan_p, kind, ntiles):
    """the ragged launch's work split (lidbox_extract_features_ragged), restated"""
    waves = min(RAGGED_WAVES, fp.stream_waves(plan_p, kind))
    tpw = -(-ntiles // env.ncu)
    nwg = -(-ntiles // tpw)
    return dict(tiles_per_wg=tpw, nwg=nwg, waves=min(waves, tpw), last_wg_tiles=ntiles - (nwg - 1) * tpw)


def _short_batch(target_tiles, seed, long_at=None):
    """frame counts in 0 .. 10 (0, 1 or 2 tiles) that sum to exactly target_tiles tiles; long_at: one utterance of 98 frames (13
    tiles) at that tile position"""
    rng = np.random.default_rng(seed)
    T, tiles = [], 0
    while tiles < target_tiles:
        if long_at is not None and tiles >= long_at and 98 not in T and target_tiles - tiles >= 13:
            T.append(98)
        else:
            t = int(rng.integers(0, 11))
            if tiles + (t + 7) // 8 > target_tiles:
                t = 8
            T.append(t)
        tiles += (T[-1] + 7) // 8
    assert tiles == target_tiles
    return T


SPLITS = {"one_wave": lambda ncu: (max(ncu - 3, 2), None), "one_wave_nwg8": lambda ncu: (max(8 * (ncu // 8), 8), None),
          "few_tiles_long": lambda ncu: (3 * ncu - 5, ncu), "many_tiles": lambda ncu: (17 * ncu + 5, None)}


def _split_case(env, name):
    if ("split", name) not in env.cache:
        plan, p, win = _plans(env)
        target, long_at = SPLITS[name](env.ncu)
        T = _short_batch(target, len(name), long_at)
        rng = np.random.default_rng(target)
        # lengths: the frames' samples plus 0 .. 3 that no frame owns (T = 0: 0 .. 399 samples)
        lengths = [int(rng.integers(0, 400)) if t == 0 else 400 + (t - 1) * S + int(rng.integers(0, 4)) for t in T]
        sigs = _signals(lengths, target)
        env.cache[("split", name)] = (T, sigs, _split(env, p, fp.LOGMEL, target))
    return env.cache[("split", name)]


def test_the_ragged_work_split_reaches_every_branch_on_this_device(env):
    d = {name: _split_case(env, name)[2] for name in SPLITS}
    assert any(v["waves"] == 1 and v["nwg"] > 1 for v in d.values())
    assert any(2 <= v["tiles_per_wg"] <= v["waves"] for v in d.values())
    assert any(v["tiles_per_wg"] > 16 for v in d.values())
    assert any(v["last_wg_tiles"] < v["tiles_per_wg"] for v in d.values())
    assert any(v["nwg"] % 8 for v in d.values()) and any(v["nwg"] % 8 == 0 and v["nwg"] >= 8 for v in d.values())
    # the long utterance's 13 tiles begin at a workgroup's last tiles and end workgroups later
    T, _, v = _split_case(env, "few_tiles_long")
    first = sum((t + 7) // 8 for t in T[:T.index(98)])
    assert first // v["tiles_per_wg"] < (first + 12) // v["tiles_per_wg"]


@pytest.mark.parametrize("name", sorted(SPLITS))
def test_work_split_bits_permutation_and_repeat(env, name):
    """many short utterances (T in 0 .. 10) at tile counts taken from the device's CU count: every utterance has its dense bits
    (utterances of one length share the dense launch), permuting the utterances permutes the rows, a second run repeats the first;
    64 utterances against the oracle, the others are covered by the bit identity"""
    plan, p, win = _plans(env)
    T, sigs, _ = _split_case(env, name)
    kinds = KINDS if name == "few_tiles_long" else (fp.LOGMEL,)
    for kind in kinds:
        r = _ragged(env, sigs)
        out, fo, flag = _run_ragged(env, plan, kind, r)
        assert flag == 0 and np.array_equal(np.diff(fo), T)
        _assert_rows_equal(out, fo, _dense_by_length(env, plan, p, kind, sigs), name)
        again, _, _ = _run_ragged(env, plan, kind, r)
        assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "run to run"
        perm = np.random.default_rng(5).permutation(len(sigs))
        pout, pfo, _ = _run_ragged(env, plan, kind, _ragged(env, [sigs[i] for i in perm]))
        rows = torch.cat([torch.arange(int(fo[i]), int(fo[i + 1])) for i in perm]).cuda()
        assert torch.equal(pout.view(torch.int32), out[rows].view(torch.int32)), "permutation"
        pick = sorted(set(np.random.default_rng(7).integers(0, len(sigs), 60).tolist()) | {0, len(sigs) - 1, T.index(max(T))})
        _judge_utterances(name, p, win, kind, out, fo, sigs, pick)


# ---------------------------------------------------------------------------------------------------- kernel: non-finite contract
@pytest.mark.parametrize("kind", (fp.SPEC, fp.LOGMEL, fp.MFCC), ids=lambda k: fp.KIND_NAMES[k])
def test_non_finite_contract(env, kind):
    """a NaN / Inf in a sample that a frame of utterance k owns: flag set, exactly fp.lost_frames of k turn non-finite, every other
    row keeps the clean run's bits; in an alignment gap, behind an utterance's last frame or in a zero-frame utterance: flag 0, all
    bits unchanged"""
    plan, p, win = _plans(env)
    sigs = _signals(_lengths(400), 3)
    clean, fo, flag = _run_ragged(env, plan, kind, _ragged(env, sigs))
    assert flag == 0
    host = clean.cpu().numpy()
    for k, positions in ((7, (0, 399, 400, 8000, 15519, 15919)), (5, (0, 1519)), (1, (0, 399))):
        N = len(sigs[k])
        _, d = _dense(env, plan, p, kind, sigs[k][None])
        T = fp.num_frames(N, 400, S)
        for pos in positions:
            for v in (np.nan, np.inf):
                y = [s.copy() for s in sigs]
                y[k][pos] = v
                out, _, flag = _run_ragged(env, plan, kind, _ragged(env, y))
                lost = fp.lost_frames(p, d, N, pos)
                assert flag != 0 and lost, (k, pos, v)
                got = out.cpu().numpy()
                bad = {t for t in range(T) if not np.isfinite(got[int(fo[k]) + t]).all()}
                assert bad == lost, (k, pos, v, sorted(bad), sorted(lost))
                keep = np.ones(len(got), bool)
                keep[[int(fo[k]) + t for t in lost]] = False
                assert np.array_equal(got[keep].view(np.int32), host[keep].view(np.int32)), (k, pos, v)
    # samples no frame owns: behind the last frame (15 920 .., 1 520 .. 1 522), zero-frame utterances, and the alignment gap behind
    # the 1 523 samples of utterance 5 (NaN in the clean run already; an Inf here)
    for k, pos in ((7, 15920), (7, 15935), (7, 15999), (5, 1520), (5, 1522), (3, 0), (3, 398), (8, 200), (5, 1523)):
        for v in (np.nan, np.inf):
            r = _ragged(env, sigs)
            r.flat[int(r.starts_host[k]) + pos] = v
            out, _, flag = _run_ragged(env, plan, kind, r)
            assert flag == 0 and torch.equal(out.view(torch.int32), clean.view(torch.int32)), (k, pos, v)


# ---------------------------------------------------------------------------------------------------- refusals and the fallback
def _c_call(env, plan, kind, r, g, flag):
    to, fo = env.sg.ragged_frame_plan(r.lengths_host, plan.frame_length, plan.frame_step)
    to_d, fo_d = torch.from_numpy(to).cuda(), torch.from_numpy(fo).cuda()
    nv = env.nv
    rc = nv.lib.lidbox_extract_features_ragged(plan.handle, kind, nv.ptr(r.flat), nv.ptr(r.starts), nv.ptr(to_d), nv.ptr(fo_d), r.B,
                                               int(to[-1]), int(fo[-1]), g.ptr, nv.ptr(flag), None, 0, nv.current_stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", ("fft256", "misaligned"))
def test_refusals_leave_the_output_untouched_and_run_ragged_falls_back(env, case):
    plan, p, win = _plans(env, **(dict(nfft=256, L=200, S=80) if case == "fft256" else {}))
    kind = fp.LOGMEL
    L, step = plan.frame_length, plan.frame_step
    lengths = [0, L, L + 7 * step, L - 1, L + 7 * step + 3, L + 20 * step]
    sigs = _signals(lengths, 11)
    r = _ragged(env, sigs, misalign=(case == "misaligned"))
    assert plan.ragged_ok(kind) == (case == "misaligned")
    _, fo = env.sg.ragged_frame_plan(r.lengths_host, L, step)
    g = Guarded((int(fo[-1]), plan.channels(kind)))
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _c_call(env, plan, kind, r, g, flag)
    assert rc == -1 and ("16-byte" if case == "misaligned" else "does not take the ragged kernel") in env.nv.last_error()
    assert np.isnan(g.numpy()).all() and int(flag.item()) == 0
    # NULL pointers and negative counts are refused the same way
    nv = env.nv
    z = torch.zeros(len(lengths) + 1, dtype=torch.int64, device="cuda")
    ok_plan = _plans(env)[0]
    for args in ((None, nv.ptr(r.starts), nv.ptr(z), nv.ptr(z), 1, 0, 0, g.ptr), (nv.ptr(z), None, nv.ptr(z), nv.ptr(z), 1, 0, 0, g.ptr),
                 (nv.ptr(z), nv.ptr(z), None, nv.ptr(z), 1, 0, 0, g.ptr), (nv.ptr(z), nv.ptr(z), nv.ptr(z), None, 1, 0, 0, g.ptr),
                 (nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), 1, 0, 0, None), (nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), -1, 0, 0, g.ptr),
                 (nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), 1, -1, 0, g.ptr), (nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), 1, 1, -1, g.ptr)):
        assert nv.lib.lidbox_extract_features_ragged(ok_plan.handle, kind, *args[:7], args[7], None, None, 0, nv.current_stream()) == -1
    # B = 0 and total_frames = 0: OK without a launch
    assert nv.lib.lidbox_extract_features_ragged(ok_plan.handle, kind, nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), 0, 0, 0, g.ptr, None, None, 0,
                                                 nv.current_stream()) == 0
    assert nv.lib.lidbox_extract_features_ragged(ok_plan.handle, kind, nv.ptr(z), nv.ptr(z), nv.ptr(z), nv.ptr(z), 3, 0, 0, g.ptr, None, None, 0,
                                                 nv.current_stream()) == 0
    torch.cuda.synchronize()
    assert np.isnan(g.numpy()).all()
    # the Python layer falls back to the dense path, utterance by utterance
    out, fo2, flag = _run_ragged(env, plan, kind, r, python=True)
    assert flag == 0
    want = [plan.run(kind, torch.from_numpy(s).cuda()[None])[0] for s in sigs]
    _assert_rows_equal(out, fo2, want, case)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: fp.KIND_NAMES[k])
def test_run_ragged_gives_every_utterance_what_run_gives_it_alone(env, kind):
    """through the Python layer, whatever the length: a lone utterance of 1 523 samples (no multiple of 4) is read by the dense
    call's scalar-load kernel, whose last bits differ from the streaming kernel's; run_ragged hands it to that call"""
    plan, p, win = _plans(env)
    sigs = _signals(_lengths(400) + [1523, 803], 31)
    out, fo, flag = _run_ragged(env, plan, kind, _ragged(env, sigs), python=True)
    assert flag == 0
    _assert_rows_equal(out, fo, [plan.run(kind, torch.from_numpy(s).cuda()[None])[0] for s in sigs], "alone")
    # and a NaN in such an utterance still raises the flag
    sigs[5][700] = np.nan
    out, fo, flag = _run_ragged(env, plan, kind, _ragged(env, sigs), python=True)
    assert flag != 0 and not bool(torch.isfinite(out[int(fo[5]):int(fo[6])]).all()) and bool(torch.isfinite(out[int(fo[6]):]).all())


# ---------------------------------------------------------------------------------------------------- normalisation
NORM_T = (0, 1, 2, 3, 8, 197, 1000, 0, 0, 5, 0)           # the issue's T_b, and empty utterances in a row and last


def _rows_of(T, C, seed):
    rng = np.random.default_rng([seed, C])
    x = torch.from_numpy((rng.standard_normal((sum(T), C)) * 3 + rng.standard_normal((1, C))).astype(np.float32)).cuda()
    return x, np.concatenate(([0], np.cumsum(T)))


@pytest.mark.parametrize("C", (1, 13, 33, 64, 65, 257))
def test_ragged_cmvn_and_cmn_equal_the_dense_call_per_utterance(env, C):
    from lidbox_amd import features
    x, ro = _rows_of(NORM_T, C, 1)
    for ragged, dense in ((features.cmvn_ragged, features.cmvn), (features.cmn_ragged, features.cmn)):
        g = Guarded(tuple(x.shape))
        out = ragged(x, ro, out=g.view)
        torch.cuda.synchronize()
        g.check()
        for b in range(len(NORM_T)):
            lo, hi = int(ro[b]), int(ro[b + 1])
            assert torch.equal(out[lo:hi], dense(x[lo:hi][None])[0]), (C, b)
        inplace = x.clone()
        assert ragged(inplace, ro, out=inplace) is inplace and torch.equal(inplace, out), "in place"


def test_ragged_cmvn_past_one_grid_dimension(env):
    """65 537 utterances at C = 1: utterances 65 535 and 65 536 are a workgroup's second trip.  All have one row but the last,
    whose three rows give a result that is not zero."""
    from lidbox_amd import features
    T = [1] * 65536 + [3]
    x, ro = _rows_of(T, 1, 2)
    out = features.cmvn_ragged(x, ro)
    assert torch.equal(out[:65536], features.cmvn(x[:65536].reshape(65536, 1, 1)).reshape(65536, 1))
    assert torch.equal(out[65536:], features.cmvn(x[65536:][None])[0]) and float(out[65536:].abs().min()) > 0


@pytest.mark.parametrize("normalize_variance", (True, False))
@pytest.mark.parametrize("w", (2, 3, 300))
def test_ragged_window_normalization_equals_the_dense_call_per_utterance(env, w, normalize_variance):
    from lidbox_amd import features
    T = (w - 1, 0, w, w + 1, 1001, 0)
    for C in (13, 65):
        x, ro = _rows_of(T, C, w)
        g = Guarded(tuple(x.shape))
        env.nv.check(env.lib.lidbox_window_norm_ragged_fwd(env.nv.ptr(x), env.nv.ptr(torch.from_numpy(ro).cuda()), len(T), C, w,
                                                           int(normalize_variance), g.ptr, env.nv.current_stream()))
        torch.cuda.synchronize()
        g.check()
        out = features.window_normalization_ragged(x, ro, window_len=w, normalize_variance=normalize_variance)
        assert torch.equal(out, g.view)
        for b in range(len(T)):
            lo, hi = int(ro[b]), int(ro[b + 1])
            want = features.window_normalization(x[lo:hi][None], window_len=w, normalize_variance=normalize_variance)[0]
            assert torch.equal(out[lo:hi], want), (w, C, b)
    whole = features.window_normalization_ragged(x, ro, window_len=-1, normalize_variance=normalize_variance)
    assert torch.equal(whole, (features.cmvn_ragged if normalize_variance else features.cmn_ragged)(x, ro))


# ---------------------------------------------------------------------------------------------------- steps
STEP_LENGTHS = (0, 399, 400, 1520, 1523, 1680, 16000)


def _elements():
    return [dict(id="utt%d" % i, signal=s, sample_rate=16000, label="l%d" % (i % 2)) for i, s in enumerate(_signals(STEP_LENGTHS, 21))]


def _assert_same_elements(got, want):
    assert [x["id"] for x in got] == [x["id"] for x in want]
    for g, w in zip(got, want):
        assert set(g) == set(w) and g["feature_type"] == w["feature_type"] and g["label"] == w["label"]
        assert g["input"].shape == w["input"].shape and torch.equal(g["input"].view(torch.int32), w["input"].view(torch.int32)), g["id"]


@pytest.mark.parametrize("extra", ({}, {"window_normalization": {"window_len": 5, "normalize_variance": True}},
                                   {"sample_minmax_scaling": {"min": -1.0, "max": 1.0}}), ids=("plain", "window_norm", "minmax"))
@pytest.mark.parametrize("ftype", ("spectrogram", "db_spectrogram", "melspectrogram", "logmelspectrogram", "mfcc"))
def test_extract_features_step_ragged_equals_batch_size_one(env, ftype, extra):
    from lidbox_amd.data import steps
    config = dict({"type": ftype}, **extra)
    got = list(steps.extract_features(_elements(), dict(config, ragged_batch_size=4)))
    want = list(steps.extract_features(_elements(), dict(config, batch_size=1)))
    assert [x["input"].shape[0] for x in got] == [0, 0, 1, 8, 8, 9, 98]
    _assert_same_elements(got, want)


def test_extract_features_step_ragged_refusals(env):
    from lidbox_amd.data import steps
    with pytest.raises(ValueError, match="group_by_input_length"):
        list(steps.extract_features(_elements(), {"type": "mfcc", "ragged_batch_size": 4, "group_by_input_length": {"max_batch_size": 4}}))
    mixed = _elements()
    mixed[2]["sample_rate"] = 8000
    with pytest.raises(ValueError, match="Different sample rates in a single batch not supported"):
        list(steps.extract_features(mixed, {"type": "mfcc", "ragged_batch_size": 4}))


def test_normalize_step_ragged_equals_batch_size_one(env):
    from lidbox_amd.data import steps
    feats = list(steps.extract_features(_elements(), {"type": "logmelspectrogram", "ragged_batch_size": 7}))
    got = list(steps.normalize(iter(feats), {"key": "input", "ragged": True, "batch_size": 4}))
    want = list(steps.normalize(iter(feats), {"key": "input", "batch_size": 1}))
    _assert_same_elements(got, want)
    with pytest.raises(ValueError, match="different shapes"):
        list(steps.normalize(iter(feats), {"key": "input", "batch_size": 4}))


def test_pipeline_end_to_end_ragged_equals_batch_size_one(env, wav_paths):
    """no signal chunking: rms_vad leaves every utterance its own length, ragged features, input chunks, ragged normalize"""
    from lidbox_amd.data import pipelines, steps
    labels = ["l0", "l1"]
    init_data = {"id": ["utt%d" % i for i in range(5)], "path": list(wav_paths), "label": ["l%d" % (i % 2) for i in range(5)]}

    def run(features, normalize):
        config = {"pre_process": {"rms_vad": {"strength": 0.1, "vad_frame_length_ms": 10, "min_non_speech_length_ms": 100}},
                  "features": dict({"type": "logmelspectrogram"}, **features),
                  "post_process": {"chunks": {"length": 50, "step": 24}, "normalize": dict({"key": "input"}, **normalize)}}
        plan = pipelines.create_dataset("test", labels, init_data, config)
        assert [s.key for s in plan][-3:] == ["extract_features", "create_input_chunks", "normalize"]
        return list(steps.from_steps(plan))

    got = run({"ragged_batch_size": 4}, {"ragged": True, "batch_size": 4})
    want = run({"batch_size": 1}, {"batch_size": 1})
    assert len(got) == len(want) > 0
    assert [x["id"] for x in got] == [x["id"] for x in want]
    for g, w in zip(got, want):
        assert g["input"].shape == (50, 40) and torch.equal(g["input"].view(torch.int32), w["input"].view(torch.int32)), g["id"]
