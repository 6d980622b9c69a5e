"""
Speed-change resampling and FIR filtering on the device (csrc/augment.hip) against float64 scipy.signal.
"""
import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from lidbox_amd.features import signal_ops
    return signal_ops


def _resample_all(xs, ms, starts=None):
    so = _ops()
    if starts is None:
        r = so.RaggedSignals.from_list([torch.from_numpy(x.astype(np.float32)) for x in xs])
    else:
        total = int(max(s + len(x) for s, x in zip(starts, xs))) + 4
        flat = torch.zeros(total, dtype=torch.float32)
        for s, x in zip(starts, xs):
            flat[s:s + len(x)] = torch.from_numpy(x.astype(np.float32))
        r = so.RaggedSignals(flat.cuda(), starts, [len(x) for x in xs])
    out = so.resample(r, ms)
    assert all(int(s) % 4 == 0 for s in out.starts_host)
    return [y.cpu().numpy() for y in out.split()]


def _check_resample(x, y, m):
    ref = scipy.signal.resample(x.astype(np.float32).astype(np.float64), m)
    assert y.shape == (m,)
    if m == 0:
        return
    rel = np.linalg.norm(y - ref) / max(np.linalg.norm(ref), 1e-30)
    mx = np.abs(y - ref).max()
    assert rel <= 4e-6 and mx <= 4e-6 * np.abs(x).max(), (len(x), m, rel, mx)


GRID = ([(n, m) for n in list(range(1, 10)) + [16] for m in list(range(1, 10)) + [16]]
        + [(10923, 12000), (10924, 12000), (12000, 8768), (12001, 8768), (8000, 12384), (8000, 12385),
           (7, 8), (8, 7), (9, 11), (12, 10), (11, 13), (14, 14), (15, 15), (4096, 4096), (4097, 4095)])


def test_resample_parity_grid():
    rng = np.random.default_rng(0)
    xs = [rng.standard_normal(n) for n, _ in GRID]
    ys = _resample_all(xs, [m for _, m in GRID])
    for x, y, (_, m) in zip(xs, ys, GRID):
        _check_resample(x, y, m)


@pytest.mark.parametrize("n,m", [(48000, 43637), (131071, 120000), (1 << 20, 1000003), (2 ** 21, 2 ** 21 - 3)])
def test_resample_parity_long(n, m):
    x = np.random.default_rng(n).standard_normal(n)
    _check_resample(x, _resample_all([x], [m])[0], m)


def test_resample_empty_and_zero_outputs():
    x = np.random.default_rng(1).standard_normal(20)
    ys = _resample_all([np.zeros(0), x, x], [0, 0, 7])
    assert [len(y) for y in ys] == [0, 0, 7]
    _check_resample(x, ys[2], 7)
    with pytest.raises(ValueError, match="2\\^21"):
        _resample_all([np.zeros(8)], [2 ** 21 + 1])


@pytest.mark.parametrize("n,m,cycles", [(64, 100, 3), (1000, 733, 7), (30000, 27271, 40), (9, 16, 2)])
def test_resample_whole_period_sinusoid(n, m, cycles):
    x = np.cos(2 * np.pi * cycles * np.arange(n) / n + 0.3)
    y = _resample_all([x], [m])[0]
    want = np.cos(2 * np.pi * cycles * np.arange(m) / m + 0.3)
    assert np.abs(y - want).max() <= 1e-5


def _mixed_batch(rng, count=40):
    lengths = [int(v) for v in rng.integers(0, 20000, count)]
    lengths[:6] = [0, 1, 3, 17, 16385, 40000]
    xs = [rng.standard_normal(n) for n in lengths]
    starts = np.cumsum([0] + [n + int(rng.integers(0, 4)) for n in lengths[:-1]])          # some starts unaligned
    return xs, [int(s) for s in starts]


def test_resample_batch_independence():
    rng = np.random.default_rng(2)
    xs, starts = _mixed_batch(rng)
    ms = [int(len(x) * rng.uniform(0.85, 1.15)) if len(x) else 0 for x in xs]
    together = _resample_all(xs, ms, starts)
    for x, m, y in zip(xs, ms, together):
        alone = _resample_all([x], [m])[0]
        assert np.array_equal(alone, y)


def _fir_all(xs, coefs, starts=None):
    so = _ops()
    if starts is None:
        r = so.RaggedSignals.from_list([torch.from_numpy(x.astype(np.float32)) for x in xs])
    else:
        total = int(max(s + len(x) for s, x in zip(starts, xs))) + 4
        flat = torch.zeros(total, dtype=torch.float32)
        for s, x in zip(starts, xs):
            flat[s:s + len(x)] = torch.from_numpy(x.astype(np.float32))
        r = so.RaggedSignals(flat.cuda(), starts, [len(x) for x in xs])
    return [y.cpu().numpy() for y in so.fir_filter(r, torch.from_numpy(np.asarray(coefs, np.float32))).split()]


@pytest.mark.parametrize("K", [1, 2, 10, 33, 257, 4096])
def test_fir_parity(K):
    rng = np.random.default_rng(K)
    lengths = [0, 1, max(K - 1, 1), K, K + 1, 4099, 2047, 5003]
    xs = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    f = rng.standard_normal((len(xs), K)).astype(np.float32)
    ys = _fir_all(xs, f)
    for x, fb, y in zip(xs, f, ys):
        assert y.shape == x.shape
        if not len(x):
            continue
        ref = scipy.signal.lfilter(fb.astype(np.float64), 1.0, x.astype(np.float64))
        assert np.abs(y - ref).max() <= 1e-6 * np.abs(fb).sum() * np.abs(x).max()
        if K == 1:
            assert np.array_equal(y, fb[0] * x)


def test_fir_batch_independence():
    rng = np.random.default_rng(3)
    xs, starts = _mixed_batch(rng)
    xs = [x.astype(np.float32) for x in xs]
    f = rng.standard_normal((len(xs), 10)).astype(np.float32)
    together = _fir_all(xs, f, starts)
    for x, fb, y in zip(xs, f, together):
        assert np.array_equal(_fir_all([x], fb[None])[0], y)


# ------------------------------------------------------------------ steps and audio functions
def _elements(rng, count=20):
    rates = [8000, 16000, 22050]
    els = []
    for i in range(count):
        n = int(rng.integers(0, 30000)) if i else 0
        els.append(dict(id="utt%02d" % i, signal=rng.standard_normal(n).astype(np.float32), sample_rate=rates[i % 3],
                        keep=bool(i % 4), label=i))
    return els


def test_speed_change_step():
    from lidbox_amd.data import steps
    from lidbox_amd.features import audio
    rng = np.random.default_rng(4)
    els = _elements(rng)
    outs = [list(steps.random_signal_speed_change(iter(els), 0.9, 1.1, flag="keep", seed=11, launch_batch=lb))
            for lb in (1, 7, 256)]
    again = list(steps.random_signal_speed_change(iter(els), 0.9, 1.1, flag="keep", seed=11))
    draws = np.random.default_rng(11)
    for k, x in enumerate(els):
        ys = [o[k] for o in outs] + [again[k]]
        for y in ys:
            assert y["id"] == x["id"] and y["label"] == x["label"] and y["sample_rate"] == x["sample_rate"]
        if not x["keep"]:
            assert all(y["signal"] is x["signal"] for y in ys)
            continue
        got = [torch.as_tensor(y["signal"]).cpu().numpy() for y in ys]
        for g in got[1:]:
            assert np.array_equal(got[0], g)
        in_rate = steps.speed_change_rate(draws, x["sample_rate"], 0.9, 1.1)
        assert len(got[0]) == len(x["signal"]) * x["sample_rate"] // in_rate
        want, rate = audio.pyfunc_resample(torch.from_numpy(x["signal"]).cuda(), in_rate, x["sample_rate"])
        assert rate == x["sample_rate"]
        assert np.array_equal(want.cpu().numpy(), got[0])
        if len(x["signal"]):
            _check_resample(x["signal"], got[0], len(got[0]))


def test_fir_step():
    from lidbox_amd.data import steps
    from lidbox_amd.features import audio
    rng = np.random.default_rng(5)
    els = _elements(rng)
    outs = [list(steps.random_signal_fir_filtering(iter(els), 10, flag="keep", seed=3, launch_batch=lb))
            for lb in (1, 7, 256)]
    draws = np.random.default_rng(3)
    for k, x in enumerate(els):
        ys = [o[k] for o in outs]
        for y in ys:
            assert y["id"] == x["id"] and y["label"] == x["label"]
        if not x["keep"]:
            assert all(y["signal"] is x["signal"] for y in ys)
            continue
        got = [y["signal"].cpu().numpy() for y in ys]
        for g in got[1:]:
            assert np.array_equal(got[0], g)
        f = draws.standard_normal(10, dtype=np.float32)
        want = audio.scipy_lfilter(torch.from_numpy(x["signal"]).cuda(), f).cpu().numpy()
        assert np.array_equal(want, got[0])
        if len(x["signal"]):
            ref = scipy.signal.lfilter(f.astype(np.float64), 1.0, x["signal"].astype(np.float64))
            assert np.abs(got[0] - ref).max() <= 1e-6 * np.abs(f).sum() * np.abs(x["signal"]).max()


def test_random_gaussian_fir_filter_is_seeded():
    from lidbox_amd.features import audio
    x = torch.from_numpy(np.random.default_rng(6).standard_normal(1000).astype(np.float32)).cuda()
    a = audio.random_gaussian_fir_filter(x, 10, seed=9).cpu().numpy()
    f = np.random.default_rng(9).standard_normal(10, dtype=np.float32)
    assert np.array_equal(a, audio.scipy_lfilter(x, f).cpu().numpy())
    y = audio.scipy_resample(x, 16000, 8000)
    assert y.shape == (500,)
