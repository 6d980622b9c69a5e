"""
Host-only planning of the augmentation steps (no GPU): output lengths of the speed change, the seeded draws,
the resampling workspace (which follows the transform sizes the kernels are grouped by) and the limit errors.
"""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, np.int64))


def test_resample_length_is_exact_floor():
    from lidbox_amd.features.signal_ops import resample_length
    assert resample_length(16000, 17600, 16000) == 14545
    assert resample_length(48000, 14400, 16000) == 53333
    assert resample_length(0, 15000, 16000) == 0
    # past 2^31 / 16000 samples the reference's int32 product wraps; the length here stays exact
    n = 2 ** 31 // 16000 + 10
    assert resample_length(n, 15000, 16000) == n * 16000 // 15000 > 0
    assert (n * 16000) % 2 ** 32 >= 2 ** 31            # = negative as an int32
    with pytest.raises(ValueError):
        resample_length(100, 0, 16000)


def test_speed_change_draws_follow_float32_formula():
    from lidbox_amd.data.steps import speed_change_rate
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    for sr in (8000, 16000, 44100):
        u = b.random(dtype=np.float32)
        ratio = np.float32(0.9) + (np.float32(1.1) - np.float32(0.9)) * u
        assert speed_change_rate(a, sr, 0.9, 1.1) == int(ratio * np.float32(sr))
    r = [speed_change_rate(np.random.default_rng(1), 16000, 0.9, 1.1) for _ in range(2)]
    assert r[0] == r[1] and 14400 <= r[0] <= 17600


def _plan_bytes(n, m):
    tw = 16384 * 8
    active = [(a, b) for a, b in zip(n, m) if a and b]
    if not active:
        return 0
    ks = [min(a, b) // 2 + 1 for a, b in active]
    p1 = [1 << int(np.ceil(np.log2(a + k - 1))) if a + k > 2 else 1 for (a, _), k in zip(active, ks)]
    p2 = [1 << int(np.ceil(np.log2(k + b - 1))) if k + b > 2 else 1 for (_, b), k in zip(active, ks)]
    return tw + len(n) * max(ks) * 8 + max(2 * sum(p1), 2 * sum(p2)) * 8


@pytest.mark.parametrize("n,m", [([1], [1]), ([9, 16, 0, 5], [4, 9, 0, 0]), ([10923, 12001], [12000, 8768]),
                                 ([48000, 131071, 2 ** 21], [43637, 120000, 2 ** 21 - 7])])
def test_resample_workspace_follows_transform_sizes(nv, n, m):
    n_h, m_h = _i64(n), _i64(m)
    got = nv.lib.lidbox_resample_workspace(n_h.ctypes.data, m_h.ctypes.data, len(n))
    assert got == _plan_bytes(n, m)


def _plan_only(nv, n, m):
    n_h, m_h = _i64(n), _i64(m)
    return nv.lib.lidbox_resample(None, None, None, None, None, None, n_h.ctypes.data, m_h.ctypes.data, len(n), None, 0,
                                  None)


def test_resample_refuses_lengths_past_the_limit(nv):
    for n, m in (([2 ** 21 + 1], [100]), ([100], [2 ** 21 + 1])):
        assert _plan_only(nv, n, m) == -1
        assert "2^21" in nv.last_error()
    assert _plan_only(nv, [0], [5]) == -1 and "empty" in nv.last_error()
    assert _plan_only(nv, [0, 7], [0, 0]) == 0          # nothing to do: no workspace, no launch


def test_fir_refuses_bad_tap_counts(nv):
    for k in (0, 4097):
        assert nv.lib.lidbox_fir_filter(None, None, None, 1, 10, None, k, None, None) == -1
        assert "4096" in nv.last_error()
