"""
The kernels of csrc/norm.hip at the sizes where their tiling, grid caps and stride loops change behaviour, against the
float64 oracles of oracle/features_np.py.  `PATHS` is the one table of those sizes, each with the condition in norm.hip
it sits on; the bounds are the ones tests/test_features_gpu.py already states for these operations.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import features_np as fo

pytestmark = pytest.mark.gpu

PATHS = dict(
    # lidbox_cmvn_strided_fwd: `cw = 64` columns per workgroup, grid.x = cdiv(inner, cw); `active = c < inner` masks the
    # last tile when inner % 64 != 0 (257 = 4 * 64 + 1); `cw / 2 >= inner` narrows the tile for inner < 64
    cmvn_tile=64,
    # cmvn_kernel: `o += gridDim.y` with grid.y = min(outer, 65535): a second trip from outer = 65 536
    grid_y=65535,
    # window_norm_kernel: one thread per (b, c), 256 per workgroup: grid = cdiv(B * C, 256); 8 time steps per iteration
    window_block=256,
    window_unroll=8,
    # lidbox_minmax: nwg = min(cdiv(n, 256 * 8), MM_MAX_WG = 1024): minmax_stage1's `i += gridDim.x * 256` takes more than
    # 8 trips, and the cap is reached, above n = 1024 * 256 * 8
    minmax_cap=1024 * 256 * 8,
    # ew_grid: `g > 2048 ? 2048 : g` workgroups of 256: feature_scaling_kernel / log10_kernel / power_to_db_kernel loop
    # a second time above n = 2048 * 256
    ew_cap=2048 * 256,
)
assert PATHS["minmax_cap"] == 2097152

SPEC = (64, 198, 257)                                   # a spectrogram batch: n = 3 256 704 > minmax_cap > ew_cap
assert int(np.prod(SPEC)) > PATHS["minmax_cap"] > PATHS["ew_cap"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).cuda()


# ------------------------------------------------------------------ window_normalization
WINDOW_SHAPES = [(5, 198, 40), (3, 198, 257), (2, 1000, 64), (300, 9, 3)]      # B * C = 200, 771, 128, 900; T % 8 = 6, 6, 0, 1
WINDOW_LENS = (2, 3, 8, "T-1", 150, 299, 300)
WINDOW_DATA = dict(standard=(0.0, 1.0), offset_1e4=(1e4, 0.1), offset_m3e3=(-3e3, 5.0))


def _window_ref(x, w, normalize_variance):
    """fo.window_normalization (float64, two-pass over materialised windows) a few channels at a time: the windows of
    (2, 1000, 64) at w = 999 would otherwise be a gigabyte; every (b, c) is independent"""
    B, T, C = x.shape
    out = np.empty(x.shape, np.float64)
    cstep = max(1, int(4e6 // (T * w)))
    for b in range(B):
        for c0 in range(0, C, cstep):
            out[b:b + 1, :, c0:c0 + cstep] = fo.window_normalization(x[b:b + 1, :, c0:c0 + cstep], window_len=w,
                                                                     normalize_variance=normalize_variance)
    return out


@pytest.mark.parametrize("data", list(WINDOW_DATA))
@pytest.mark.parametrize("shape", WINDOW_SHAPES)
def test_window_normalization_shapes_windows_and_offsets(shape, data):
    """B * C over several workgroups and not a multiple of 256, T not a multiple of the 8-step unroll, windows from 2 to
    T - 1, data far from zero (the kernel's running sums are taken relative to the channel's first sample)"""
    import lidbox_amd.features as F
    B, T, C = shape
    assert (B * C) % PATHS["window_block"] != 0
    rng = np.random.default_rng(B * T + C)
    mean, std = WINDOW_DATA[data]
    x = (mean + std * rng.standard_normal(shape)).astype(np.float32)
    xd = _dev(x)
    lens = sorted({T - 1 if w == "T-1" else w for w in WINDOW_LENS})
    lens = [w for w in lens if w < T]
    assert lens
    for w in lens:
        for nv_ in (True, False):
            got = F.window_normalization(xd, window_len=w, normalize_variance=nv_).cpu().numpy()
            ref = _window_ref(x, w, nv_)
            assert got.shape == x.shape and not np.isnan(got).any()
            err = np.abs(got - ref).max()
            assert err <= 1e-4 * max(1.0, np.abs(ref).max()), (w, nv_, err)


# ------------------------------------------------------------------ cmn / cmvn
CMVN_CASES = [
    ((6, 198, 257), 1),        # the spectrogram shape: inner = 257 is not a multiple of the 64-column tile
    ((6, 198, 257), 2),        # inner = 1 (cw = 1, 256 row groups), outer = 1188
    ((6, 198, 257), 0),        # outer = 1, inner = 50 886: 796 column tiles
    ((70000, 7, 5), 1),        # outer past grid.y = 65 535: the `o += gridDim.y` walk, R = 7 < row groups
    ((4, 1, 33), 1),           # R = 1: mean = x, std = 0
    ((2, 20000, 3), 1),        # R = 20 000 rows per column, inner = 3 (cw = 4, 64 row groups)
]


@pytest.mark.parametrize("shape,axis", CMVN_CASES)
def test_cmn_cmvn_tiles_grid_walk_and_long_columns(shape, axis):
    import lidbox_amd.features as F
    rng = np.random.default_rng(sum(shape) + axis)
    x = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    xd = _dev(x)
    for fn, ref_fn in ((F.cmn, fo.cmn), (F.cmvn, fo.cmvn)):
        got = fn(xd, axis=axis).cpu().numpy()
        ref = ref_fn(x, axis=axis)
        assert got.shape == x.shape and not np.isnan(got).any()
        assert np.abs(got - ref).max() <= 1e-4, (fn.__name__, np.abs(got - ref).max())
    if shape[axis] == 1:
        assert (F.cmvn(xd, axis=axis) == 0).all() and (F.cmn(xd, axis=axis) == 0).all()


@pytest.mark.parametrize("shape", [(6, 198, 257), (70000, 7, 5)])
def test_cmvn_in_place_and_strided_at_the_path_shapes(shape):
    """lidbox_cmvn_strided_fwd over the rows of a padded buffer, output written over the input: equal to the oracle and bit
    for bit to the dense call; the padding rows stay untouched"""
    from lidbox_amd import _native as nv
    rng = np.random.default_rng(shape[0])
    st = nv.current_stream()
    B, T, C = shape
    pad = 3
    x = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
    dense_in, dense_out = _dev(x), torch.zeros(shape, device="cuda")
    for flag, ref_fn in ((0, fo.cmn), (1, fo.cmvn)):
        nv.check(nv.lib.lidbox_cmvn_fwd(nv.ptr(dense_in), B, T, C, flag, nv.ptr(dense_out), st))
        padded = torch.full((B, pad + T, C), 9.0, device="cuda")
        padded[:, pad:] = dense_in
        p = ctypes.c_void_p(padded.data_ptr() + 4 * pad * C)
        nv.check(nv.lib.lidbox_cmvn_strided_fwd(p, B, T, C, (pad + T) * C, flag, p, (pad + T) * C, st))
        assert torch.equal(padded[:, pad:], dense_out) and bool((padded[:, :pad] == 9.0).all())
        assert np.abs(dense_out.cpu().numpy() - ref_fn(x, axis=1)).max() <= 1e-4


# ------------------------------------------------------------------ feature_scaling (min-max), log10, power_to_db
def test_feature_scaling_minmax_past_the_workgroup_cap():
    """n > 2 097 152: minmax_stage1 runs MM_MAX_WG workgroups that each stride over the input; the global minimum and
    maximum sit in the last 1 000 elements, so an element the stride loop skipped changes every output"""
    import lidbox_amd.features as F
    rng = np.random.default_rng(31)
    x = rng.normal(0, 50, size=SPEC).astype(np.float32)
    flat = x.reshape(-1)
    flat[-500], flat[-3] = 1000.0, -1200.0
    assert flat.argmax() == flat.size - 500 and flat.argmin() == flat.size - 3
    y = F.feature_scaling(_dev(x), -1.0, 1.0).cpu().numpy()
    assert abs(y.min() + 1) < 1e-6 and abs(y.max() - 1) < 1e-6
    assert y.reshape(-1).argmax() == flat.size - 500 and y.reshape(-1).argmin() == flat.size - 3
    assert np.abs(y - fo.feature_scaling(x, -1.0, 1.0)).max() < 1e-5


@pytest.mark.parametrize("where", [-1, -777, -1000])
def test_feature_scaling_nan_in_the_last_elements_gives_all_nan(where):
    """tf.reduce_min / reduce_max propagate NaN: as at small n, one NaN makes the whole result NaN -- also when only the
    last trip of the stride loop sees it"""
    import lidbox_amd.features as F
    rng = np.random.default_rng(32)
    x = rng.normal(0, 50, size=SPEC).astype(np.float32)
    x.reshape(-1)[where] = np.nan
    assert np.isnan(F.feature_scaling(_dev(x), 0.0, 1.0).cpu().numpy()).all()


def test_log10_at_spectrogram_batch_size():
    from lidbox_amd.features import audio
    rng = np.random.default_rng(33)
    p = np.abs(rng.standard_normal(SPEC).astype(np.float32)) + np.float32(1e-3)
    got = audio.log10(_dev(p)).cpu().numpy()
    assert got.shape == SPEC
    assert np.abs(got - fo.log10(p)).max() < 1e-6 and np.abs(got - np.log10(p.astype(np.float64))).max() < 1e-6


@pytest.mark.parametrize("top_db", [10.0, 80.0])
def test_power_to_db_at_spectrogram_batch_size(top_db):
    """the batch-global maximum (the dB reference) is planted in the last 1 000 elements"""
    from lidbox_amd.features import audio
    rng = np.random.default_rng(34)
    S = np.abs(rng.standard_normal(SPEC).astype(np.float32)) ** 2
    S.reshape(-1)[-250] = 50.0
    assert S.reshape(-1).argmax() == S.size - 250
    db = audio.power_to_db(_dev(S), top_db=top_db).cpu().numpy()
    assert db.shape == SPEC and db.max() <= 0 and db.min() >= -top_db - 1e-4
    assert db.reshape(-1)[-250] == 0.0
    assert np.abs(db - fo.power_to_db(S, top_db=top_db)).max() < 1e-3
