"""
Additive-noise mixing from a device-resident bank, tiling and input chunks (csrc/mix_noise.hip, signal_ops) and the dataset
steps and pipeline driver on top of them, against float64 restatements built from the oracle.
"""
import os

import numpy as np
import pytest
import scipy.io.wavfile
import torch

from oracle import features_np as fo
from oracle import signal_np as so

pytestmark = pytest.mark.gpu

SNRS = [-5.0, 0.0, 3.0, 12.5, 30.0]
LENGTHS = [0, 1, 3, 4, 17, 4001, 16000, 32768, 32772, 48000, 2 ** 21]
CLIP_LENGTHS = [1, 2, 7, 4000, 48000, 60001]


def _sg():
    from lidbox_amd.features import signal_ops
    return signal_ops


def _ragged(xs, rng=None):
    """RaggedSignals of float32 copies of xs; with an rng, starts are shifted by 0..3 samples (some unaligned)"""
    sg = _sg()
    xs = [np.asarray(x, np.float32) for x in xs]
    if rng is None:
        return sg.RaggedSignals.from_list([torch.from_numpy(x) for x in xs])
    starts = np.cumsum([1] + [len(x) + int(rng.integers(0, 4)) for x in xs[:-1]]) if xs else np.zeros(0, np.int64)
    total = int(max([s + len(x) for s, x in zip(starts, xs)] + [0])) + 4
    flat = torch.zeros(total, dtype=torch.float32)
    for s, x in zip(starts, xs):
        flat[int(s):int(s) + len(x)] = torch.from_numpy(x)
    return sg.RaggedSignals(flat.cuda(), starts, [len(x) for x in xs])


def _mix_ref(clean, clip, snr):
    clean = np.asarray(clean, np.float32).astype(np.float64)
    clip = np.asarray(clip, np.float32).astype(np.float64)
    return so.snr_mixer(clean, np.resize(clip, len(clean)), snr)[2]


def _assert_mix_close(got, ref, what):
    assert got.shape == ref.shape, what
    if len(ref) == 0:
        return
    err, bound = np.abs(got - ref).max(), 2e-5 * np.abs(ref).max()
    print("mix", what, "max|d| = %.3e bound %.3e" % (err, bound))
    assert err <= bound, (what, err, bound)


def _signals(rng, lengths, lo, hi):
    """gaussian signals.  Every signal starts with a positive sample: a one-sample utterance and the noise sample it meets have
    the same magnitude after the -25 dBFS normalisation, so at 0 dB with opposite signs the exact mix is 0.0 and a bound
    relative to max|ref| would ask fp32 for an exact cancellation"""
    xs = [(rng.standard_normal(n) * rng.uniform(lo, hi)).astype(np.float32) for n in lengths]
    for x in xs:
        x[:1] = np.abs(x[:1])
    return xs


# ------------------------------------------------------------------ 1. mixer parity
@pytest.mark.parametrize("unaligned", [False, True])
def test_mix_noise_matches_float64_oracle(unaligned):
    sg = _sg()
    rng = np.random.default_rng(1 + unaligned)
    clean = _signals(rng, LENGTHS, 0.01, 1.0)
    clips = _signals(rng, CLIP_LENGTHS, 0.001, 0.3)
    r = _ragged(clean, rng if unaligned else None)
    bank = _ragged(clips, rng if unaligned else None)
    if unaligned:
        assert (r.starts_host % 4 != 0).any() and (bank.starts_host % 4 != 0).any()
    # every (utterance, clip) pair, the snr cycling; and every snr on pairs of both work splits
    jobs = [(b, k, SNRS[(b + k) % 5]) for b in range(len(LENGTHS)) for k in range(len(CLIP_LENGTHS))]
    jobs += [(b, k, s) for b, k in ((4, 2), (5, 3), (9, 3), (9, 5), (7, 4)) for s in SNRS]
    out = sg.mix_noise(r, bank, [j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    assert out.B == len(jobs) and (out.starts_host % 4 == 0).all()
    for (b, k, snr), y in zip(jobs, out.split()):
        assert y.shape == (LENGTHS[b],)
        if LENGTHS[b]:
            _assert_mix_close(y.cpu().numpy(), _mix_ref(clean[b], clips[k], snr), (LENGTHS[b], CLIP_LENGTHS[k], snr))


# ------------------------------------------------------------------ 2. agreement with the dense kernel
@pytest.mark.parametrize("N", [32000, 4001, 40000, 4])
def test_mix_noise_agrees_with_dense_snr_mixer(N):
    sg = _sg()
    rng = np.random.default_rng(N)
    B = 5
    clean = (rng.standard_normal((B, N)) * rng.uniform(0.01, 1.0, size=(B, 1))).astype(np.float32)
    noise = (rng.standard_normal((B, N)) * rng.uniform(0.001, 0.3, size=(B, 1))).astype(np.float32)
    dense = sg.snr_mixer(torch.from_numpy(clean).cuda(), torch.from_numpy(noise).cuda(), torch.tensor(SNRS).cuda())[2].cpu().numpy()
    out = sg.mix_noise(_ragged(list(clean)), _ragged(list(noise)), np.arange(B), np.arange(B), SNRS)
    for b, y in enumerate(out.split()):
        err, bound = np.abs(y.cpu().numpy() - dense[b]).max(), 2e-5 * np.abs(dense[b]).max()
        print("dense", N, b, "max|d| = %.3e bound %.3e" % (err, bound))
        assert err <= bound


@pytest.mark.parametrize("N", [4000, 40000])
def test_mix_noise_zero_signals_give_the_dense_kernels_non_finite_values(N):
    sg = _sg()
    rng = np.random.default_rng(3)
    x = rng.standard_normal(N).astype(np.float32)
    zero = np.zeros(N, np.float32)
    clean, noise = np.stack([zero, x, zero]), np.stack([x, zero, zero])
    dense = sg.snr_mixer(torch.from_numpy(clean).cuda(), torch.from_numpy(noise).cuda(), torch.tensor([3.0] * 3).cuda())[2].cpu().numpy()
    out = sg.mix_noise(_ragged(list(clean)), _ragged(list(noise)), [0, 1, 2], [0, 1, 2], [3.0] * 3)
    assert not np.isfinite(dense).any()
    for b, y in enumerate(out.split()):
        y = y.cpu().numpy()
        assert np.array_equal(np.isnan(y), np.isnan(dense[b])) and np.array_equal(np.isposinf(y), np.isposinf(dense[b]))
        assert np.array_equal(np.isneginf(y), np.isneginf(dense[b]))


# ------------------------------------------------------------------ 3. bit identity
def test_mix_noise_output_does_not_depend_on_the_batch():
    sg = _sg()
    rng = np.random.default_rng(4)
    lengths = [int(v) for v in rng.integers(1, 70000, 12)]
    lengths[:7] = [1, 17, 32768, 32769, 65536, 65537, 100003]
    clean = _signals(rng, lengths, 0.01, 1.0)
    clips = _signals(rng, [5, 4000, 16001, 60001], 0.001, 0.3)
    r, bank = _ragged(clean, rng), _ragged(clips, rng)
    jobs = [(int(rng.integers(0, len(lengths))), int(rng.integers(0, 4)), float(rng.uniform(-5, 30))) for _ in range(40)]
    jobs[:7] = [(6, 3, 0.0), (6, 1, 0.0), (6, 3, 10.0), (2, 3, 0.0), (3, 2, 1.0), (4, 0, 2.0), (5, 1, 3.0)]     # outputs share an utterance
    args = ([j[0] for j in jobs], [j[1] for j in jobs], [j[2] for j in jobs])
    together = sg.mix_noise(r, bank, *args)
    got = [y.cpu().numpy() for y in together.split()]
    again = [y.cpu().numpy() for y in sg.mix_noise(r, bank, *args).split()]
    for j, (b, k, snr) in enumerate(jobs):
        alone = sg.mix_noise(_ragged([clean[b]]), _ragged([clips[k]]), [0], [0], [snr]).split()[0].cpu().numpy()
        assert np.array_equal(got[j], alone), (j, lengths[b])
        assert np.array_equal(got[j], again[j])
    assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[0], got[2])
    # nothing is written outside the outputs: the alignment gaps of the zero-initialised buffer are still zero
    flat = together.flat.cpu().numpy()
    inside = np.zeros(len(flat), bool)
    for s, n in zip(together.starts_host, together.lengths_host):
        inside[int(s):int(s) + int(n)] = True
    assert (flat[~inside] == 0).all() and np.isfinite(flat).all()


# ------------------------------------------------------------------ 4. refusals and edges
def test_mix_noise_edges_and_refusals():
    from lidbox_amd._native import LidboxHipError
    sg = _sg()
    rng = np.random.default_rng(5)
    clean = _signals(rng, [0, 100], 0.1, 1.0)
    clips = _signals(rng, [50, 0], 0.1, 1.0)
    r, bank = _ragged(clean), _ragged(clips)
    out = sg.mix_noise(r, bank, [0, 1, 0], [0, 0, 0], [0.0, 0.0, 5.0])
    assert [int(n) for n in out.lengths_host] == [0, 100, 0]
    _assert_mix_close(out.split()[1].cpu().numpy(), _mix_ref(clean[1], clips[0], 0.0), "with empty neighbours")
    assert sg.mix_noise(r, bank, [], [], []).B == 0                                      # J = 0
    assert sg.mix_noise(_ragged([]), bank, [], [], []).B == 0                            # B = 0
    assert sg.mix_noise(r, bank, [0], [0], [1.0]).split()[0].numel() == 0                # n = 0 only
    with pytest.raises(ValueError, match="empty"):
        sg.mix_noise(r, bank, [1], [1], [0.0])                                           # a referenced clip is empty
    with pytest.raises(ValueError):
        sg.mix_noise(r, bank, [0], [1], [0.0])                                           # ... even for an empty utterance
    for src, clip in (([2], [0]), ([-1], [0]), ([1], [2]), ([1], [-1])):
        with pytest.raises(ValueError, match="range|outside"):
            sg.mix_noise(r, bank, src, clip, [0.0])
    with pytest.raises(ValueError):
        sg.mix_noise(r, bank, [0, 1], [0], [0.0, 0.0])
    with pytest.raises(ValueError, match="2\\^21"):
        sg.mix_noise(_ragged([np.ones(2 ** 21 + 1)]), bank, [0], [0], [0.0])
    with pytest.raises(LidboxHipError):
        sg.RaggedSignals(torch.zeros(8), [0], [8])
    with pytest.raises(LidboxHipError):
        sg.input_chunks([torch.zeros(10, 3)], 2, 1)


def test_abi_reports_bad_indexes_and_empty_clips():
    """lidbox_mix_noise itself (not only the wrapper) returns the invalid-argument code"""
    from lidbox_amd import _native as nv
    n_h, m_h = np.array([10], np.int64), np.array([0, 5], np.int64)
    buf = torch.zeros(64, device="cuda")
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(4, dtype=torch.int32, device="cuda")

    def call(src, clip):
        s, c = np.array([src], np.int32), np.array([clip], np.int32)
        return nv.lib.lidbox_mix_noise(nv.ptr(buf), nv.ptr(idx), nv.ptr(idx), nv.ptr(buf), nv.ptr(idx), nv.ptr(idx), nv.ptr(i32),
                                       nv.ptr(i32), nv.ptr(buf), nv.ptr(buf), nv.ptr(idx), n_h.ctypes.data, m_h.ctypes.data,
                                       s.ctypes.data, c.ctypes.data, 1, 2, 1, None, 0, nv.current_stream())

    for src, clip, word in ((0, 0, "empty"), (1, 1, "utterance index"), (0, 2, "clip index"), (-1, 1, "utterance index")):
        assert call(src, clip) == -1
        assert word in nv.last_error()


# ------------------------------------------------------------------ 5. tile and input chunks
def test_tile_matches_numpy_tile_bit_exact():
    sg = _sg()
    rng = np.random.default_rng(6)
    cases = [(n, k) for n in (0, 1, 3, 4, 5, 4099) for k in (0, 1, 2, 7)]
    xs = [rng.standard_normal(n).astype(np.float32) for n, _ in cases]
    for r in (_ragged(xs), _ragged(xs, rng)):
        out = sg.tile(r, [k for _, k in cases])
        assert (out.starts_host % 4 == 0).all()
        for x, (n, k), y in zip(xs, cases, out.split()):
            assert np.array_equal(y.cpu().numpy(), np.tile(x, k)), (n, k)
    with pytest.raises(ValueError):
        sg.tile(_ragged(xs[:2]), [1, -1])
    assert sg.tile(_ragged([]), []).B == 0


def _windows(x, length, step):
    n = max(0, 1 + (x.shape[0] - length) // step)
    return np.stack([x[i * step:i * step + length] for i in range(n)]) if n else np.zeros((0, length, x.shape[1]), x.dtype)


@pytest.mark.parametrize("C", [1, 3, 40, 64])
def test_input_chunks_match_numpy_windows_bit_exact(C):
    from lidbox_amd.data import steps
    sg = _sg()
    rng = np.random.default_rng(C)
    length, step = 50, 20
    Ts = [0, length - 1, length, length + step - 1, 198, 1000]
    xs = [rng.standard_normal((T, C)).astype(np.float32) for T in Ts]
    chunks, nch = sg.input_chunks([torch.from_numpy(x).cuda() for x in xs], length, step)
    assert chunks.shape == (int(nch.sum()), length, C)
    assert [int(n) for n in nch] == [0, 0, 1, 1, 8, 48] == [int(n) for n in sg.input_chunk_counts(Ts, length, step)]
    ref = np.concatenate([_windows(x, length, step) for x in xs])
    assert np.array_equal(chunks.cpu().numpy(), ref)
    ds = [dict(id="utt", input=torch.from_numpy(x).cuda(), target=i) for i, x in enumerate(xs)]
    out = list(steps.create_input_chunks(ds, length, step, launch_batch=4))
    assert len(out) == len(ref)
    want_ids = ["utt-%06d" % (k + 1) for n in nch for k in range(int(n))]
    assert [o["id"] for o in out] == want_ids and want_ids[0] == "utt-000001"
    assert [o["target"] for o in out] == [i for i, n in enumerate(nch) for _ in range(int(n))]
    assert np.array_equal(np.stack([o["input"].cpu().numpy() for o in out]), ref)
    with pytest.raises(ValueError):
        sg.input_chunks([torch.zeros(4, 2, device="cuda"), torch.zeros(4, 3, device="cuda")], 2, 1)


# ------------------------------------------------------------------ 6. steps
SNR_LIST = [("sine", 0, 10), ("hum", 5, 15), ("sine", -5, 5)]


@pytest.fixture()
def noise_dir(tmp_path, wav_paths):
    """two noise types: `sine` (three of the golden sines, the second cut to 10007 samples) and `hum` (noise.wav)"""
    d = tmp_path / "noise"
    d.mkdir()
    rate, x = scipy.io.wavfile.read(wav_paths[1])
    short = str(d / "short_sine.wav")
    scipy.io.wavfile.write(short, rate, x[:10007])
    paths = {"s1": wav_paths[0], "s2": short, "h1": wav_paths[4], "s3": wav_paths[2]}
    (d / "id2label").write_text("# noise id, type\ns1 sine\ns2 sine\nh1 hum\ns3 sine\n")
    (d / "id2path").write_text("".join("%s %s\n" % kv for kv in paths.items()))
    return str(d)


def _elements(wav_paths):
    ds = []
    for i, p in enumerate(wav_paths):
        sig, rate = fo.read_wav_pcm16(p)
        ds.append(dict(id="utt%d" % i, signal=sig, sample_rate=rate, label="l%d" % (i % 2), target=i % 2))
    return ds


def _sigs(out):
    return [x["signal"].cpu().numpy() for x in out]


def test_augment_by_additive_noise_step(noise_dir, wav_paths, tmp_path, monkeypatch):
    from lidbox_amd.data import steps
    ds = _elements(wav_paths)
    type2paths = steps.noise_paths_by_type(noise_dir)
    assert list(type2paths) == ["sine", "hum"] and [len(v) for v in type2paths.values()] == [3, 1]
    counts = {t: len(p) for t, p in type2paths.items()}
    out = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST, seed=11, launch_batch=2))
    assert len(out) == len(ds) * len(SNR_LIST)
    rng = np.random.default_rng(11)
    k = 0
    used = set()
    for x in ds:
        for noise_type, index, snr in steps.additive_noise_draws(rng, SNR_LIST, counts):
            y = out[k]
            assert y["id"] == "augmented-%s-%s-snr%.2f" % (x["id"], noise_type, snr)
            assert y["sample_rate"] == 16000 and y["label"] == x["label"] and y["target"] == x["target"]
            assert set(y) == set(x)
            clip, _ = fo.read_wav_pcm16(type2paths[noise_type][index])
            used.add(len(clip))
            _assert_mix_close(y["signal"].cpu().numpy(), _mix_ref(x["signal"], clip, snr), y["id"])
            k += 1
    assert used == {48000, 10007}                                   # whole clips and the short one that wraps
    same = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST, seed=11, launch_batch=256))
    assert [x["id"] for x in same] == [x["id"] for x in out]
    assert all(np.array_equal(a, b) for a, b in zip(_sigs(same), _sigs(out)))            # launch_batch 2 vs 256, second run
    other = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST, seed=12))
    assert [x["id"] for x in other] != [x["id"] for x in out]
    monkeypatch.setenv("TMPDIR", str(tmp_path / "tmp"))
    copied = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST, copy_noise_files_to_tmpdir=True, seed=11))
    assert all(np.array_equal(a, b) for a, b in zip(_sigs(copied), _sigs(out)))
    for noise_type, paths in type2paths.items():
        for p in paths:
            assert os.path.isfile(str(tmp_path / "tmp" / "lidbox_noise_signals" / noise_type / os.path.basename(p)))
    assert steps.augment_by_additive_noise(ds, str(tmp_path / "missing"), SNR_LIST) is None
    with pytest.raises((KeyError, ValueError), match="music"):
        steps.augment_by_additive_noise(ds, noise_dir, [("music", 0, 1)])


def test_augment_by_additive_noise_refuses_another_sample_rate(noise_dir, wav_paths, tmp_path):
    from lidbox_amd.data import steps
    d = tmp_path / "noise8k"
    d.mkdir()
    _, x = scipy.io.wavfile.read(wav_paths[0])
    scipy.io.wavfile.write(str(d / "n.wav"), 8000, x[::2])
    (d / "id2label").write_text("n hum\n")
    (d / "id2path").write_text("n %s\n" % (d / "n.wav"))
    with pytest.raises(ValueError, match="same sample rate"):
        list(steps.augment_by_additive_noise(_elements(wav_paths), str(d), [("hum", 0, 10)], seed=0))


def test_repeat_too_short_signals_step():
    from lidbox_amd.data import steps
    rng = np.random.default_rng(7)
    grid = [(ms, rate, n) for ms, rate in ((1000, 16000), (250, 8000), (30, 44100), (1, 16000), (2500, 16000))
            for n in (0, 1, 7, int(np.float32(1e-3 * ms) * np.float32(rate)) - 1, int(np.float32(1e-3 * ms) * np.float32(rate)),
                      int(np.float32(1e-3 * ms) * np.float32(rate)) + 1, 100000) if n >= 0]
    assert steps.repeat_count(1000, 16000, 16000) == 1 and steps.repeat_count(1000, 16000, 15999) == 2
    assert steps.repeat_count(1000, 16000, 16001) == 1 and steps.repeat_count(1000, 16000, 0) == 0
    for ms in sorted({g[0] for g in grid}):
        ds = [dict(id="u%d" % i, signal=rng.standard_normal(n).astype(np.float32), sample_rate=rate, target=i)
              for i, (m, rate, n) in enumerate(grid) if m == ms]
        out = list(steps.repeat_too_short_signals(ds, ms, launch_batch=3))
        assert [o["id"] for o in out] == [x["id"] for x in ds]
        for x, o in zip(ds, out):
            n = len(x["signal"])
            ratio = np.float32(0) if n == 0 else np.float32(np.float32(1e-3 * ms) * np.float32(x["sample_rate"])) / np.float32(n)
            reps = int(np.ceil(ratio))
            got = o["signal"].cpu().numpy() if isinstance(o["signal"], torch.Tensor) else o["signal"]
            assert np.array_equal(got, np.tile(x["signal"], reps)), (ms, x["sample_rate"], n)
            assert len(got) == 0 or len(got) >= int(np.float32(1e-3 * ms) * np.float32(x["sample_rate"]))
            assert o["target"] == x["target"]


def test_normalize_step():
    import lidbox_amd.features as F
    from lidbox_amd.data import steps
    rng = np.random.default_rng(8)
    xs = [(rng.standard_normal((50, 40)) * 3 + 1).astype(np.float32) for _ in range(7)]
    ds = [dict(id="u%d" % i, input=torch.from_numpy(x).cuda(), target=i) for i, x in enumerate(xs)]
    out = list(steps.normalize(ds, {"key": "input", "batch_size": 3}))
    assert [o["id"] for o in out] == [x["id"] for x in ds]
    for lo in (0, 3, 6):
        ref = F.cmvn(torch.stack([x["input"] for x in ds[lo:lo + 3]]))
        assert torch.equal(torch.stack([o["input"] for o in out[lo:lo + 3]]), ref)
    for x, o in zip(xs, out):
        err = np.abs(o["input"].cpu().numpy() - fo.cmvn(x[None])[0]).max()
        print("normalize max|d| = %.3e" % err)
        assert err <= 1e-4
    one = list(steps.normalize(ds, {"key": "input", "kwargs": {"axis": 1}}))                    # batch_size defaults to 1
    assert all(np.abs(a["input"].cpu().numpy() - b["input"].cpu().numpy()).max() <= 1e-5 for a, b in zip(one, out))
    ds[1] = dict(ds[1], input=ds[1]["input"][:40])
    with pytest.raises(ValueError, match="different shapes"):
        list(steps.normalize(ds, {"key": "input", "batch_size": 3}))


def test_augment_signals_samples_the_union(noise_dir, wav_paths):
    from lidbox_amd.data import steps
    ds = _elements(wav_paths)
    confs = [{"type": "additive_noise", "split": "train", "noise_datadir": noise_dir, "snr_list": SNR_LIST[:2], "seed": 3},
             {"type": "no_such_augmentation", "split": "train"},
             {"type": "additive_noise", "split": "train", "noise_datadir": noise_dir, "snr_list": SNR_LIST[2:], "seed": 4}]
    out = list(steps.augment_signals(iter(ds), confs, seed=21))               # a one-shot iterator: ds is read once
    a = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST[:2], seed=3))
    b = list(steps.augment_by_additive_noise(ds, noise_dir, SNR_LIST[2:], seed=4))
    assert len(out) == len(ds) + len(a) + len(b) == 5 + 10 + 5
    ids = [x["id"] for x in out]
    assert sorted(ids) == sorted(x["id"] for x in ds + a + b) and len(set(ids)) == len(ids)
    for source in (ds, a, b):                                                   # every source keeps its own order
        want = [x["id"] for x in source]
        assert [i for i in ids if i in set(want)] == want
    by_id = {x["id"]: x for x in a + b}
    for x in out:
        if x["id"] in by_id:
            assert np.array_equal(x["signal"].cpu().numpy(), by_id[x["id"]]["signal"].cpu().numpy())
    assert ids != [x["id"] for x in ds + a + b]                                 # interleaved, not concatenated
    assert [x["id"] for x in steps.augment_signals(iter(ds), confs, seed=21)] == ids
    assert [x["id"] for x in steps.augment_signals(iter(ds), confs, seed=22)] != ids
    with pytest.raises(ValueError, match="random_signal_speed_change"):
        steps.augment_signals(ds, [{"type": "random_resampling", "split": "train", "range": [0.9, 1.1]}])


# ------------------------------------------------------------------ 7. end to end
def test_pipeline_end_to_end(noise_dir, wav_paths):
    from lidbox_amd.data import pipelines, steps
    labels = ["l0", "l1"]
    init_data = {"id": ["utt%d" % i for i in range(5)], "path": list(wav_paths), "label": ["l%d" % (i % 2) for i in range(5)]}
    augment = [{"type": "additive_noise", "split": "train", "noise_datadir": noise_dir, "snr_list": SNR_LIST, "seed": 5}]
    config = {
        "pre_process": {"rms_vad": {"strength": 0.1, "vad_frame_length_ms": 10, "min_non_speech_length_ms": 100},
                        "repeat_too_short_signals": {"min_length_ms": 4000},
                        "augment": augment,
                        "chunks": {"length_ms": 1000, "step_ms": 500}},
        "features": {"type": "logmelspectrogram"},
        "post_process": {"chunks": {"length": 50, "step": 24}, "normalize": {"key": "input"},
                         "remap_keys": {"signal": None, "path": None}},
    }
    results = {}
    for split in ("train", "test"):
        plan = pipelines.create_dataset(split, labels, init_data, config)
        assert ("augment_signals" in [s.key for s in plan]) == (split == "train")
        out = list(steps.from_steps(plan))
        ds = steps.drop_empty(steps.load_audio(steps.initialize(labels, init_data)))
        ds = steps.drop_empty(steps.apply_vad(steps.compute_rms_vad(ds, **config["pre_process"]["rms_vad"])))
        ds = steps.repeat_too_short_signals(ds, min_length_ms=4000)
        if split == "train":
            ds = steps.augment_signals(ds, augment_configs=augment)
        ds = steps.create_signal_chunks(ds, length_ms=1000, step_ms=500)
        ds = steps.extract_features(ds, config=config["features"])
        ds = steps.create_input_chunks(ds, length=50, step=24)
        ds = steps.remap_keys(steps.normalize(ds, config={"key": "input"}), new_keys={"signal": None, "path": None})
        want = {x["id"]: x for x in ds}
        assert len(out) == len(want) > 0 and {x["id"] for x in out} == set(want)
        for x in out:
            assert set(x) == {"id", "label", "target", "sample_rate", "input", "feature_type"}
            assert x["input"].shape == (50, 40) and bool(torch.isfinite(x["input"]).all())
            assert torch.equal(x["input"], want[x["id"]]["input"]), x["id"]
            assert x["target"] == labels.index(x["label"])
            parent, chunk, window = x["id"].rsplit("-", 2)
            assert len(chunk) == 6 and len(window) == 6 and int(chunk) >= 1 and 1 <= int(window) <= 3
        results[split] = {x["id"] for x in out}
    augmented = {i for i in results["train"] if i.startswith("augmented-")}
    assert augmented and not any(i.startswith("augmented-") for i in results["test"])
    assert results["test"] == results["train"] - augmented                  # the originals are all there, unchanged ids
    assert {i.split("-")[1] for i in augmented} == set(init_data["id"])       # every utterance was augmented
