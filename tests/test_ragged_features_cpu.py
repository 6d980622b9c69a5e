"""
Host side of the ragged feature path (no GPU): the CSR arrays of signal_ops.ragged_frame_plan against a brute-force loop, the new
C-ABI symbols and their argument refusals in the no-compute form, the register budget of the ragged kernels, and the steps'
refusal to run without a device.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

RAGGED_SYMBOLS = ("lidbox_feat_plan_ragged_ok", "lidbox_extract_features_ragged", "lidbox_cmvn_ragged_fwd",
                  "lidbox_window_norm_ragged_fwd")


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


def test_ragged_frame_plan_against_a_brute_force_loop(nv):
    from lidbox_amd.features import signal_ops as sg
    rng = np.random.default_rng(0)
    cases = [([0, 399, 400, 1520, 1523, 1680, 16000], 400, 160), ([], 400, 160), ([0], 400, 160), ([559, 560, 561, 719, 720], 400, 160),
             ([511, 512, 513, 1632, 1633], 512, 160), ([3, 4, 5, 7, 8, 35, 36], 4, 4), ([1, 2, 3], 1, 1)]
    for _ in range(20):
        L, S = int(rng.integers(1, 600)), int(rng.integers(1, 300))
        cases.append((rng.integers(0, 40000, int(rng.integers(1, 300))).tolist(), L, S))
    for lengths, L, S in cases:
        tiles, frames = [0], [0]
        for n in lengths:
            T = 0
            while T * S + L <= n:                       # frame T owns samples T S .. T S + L - 1
                T += 1
            assert T == nv.lib.lidbox_num_frames(int(n), L, S)
            frames.append(frames[-1] + T)
            tiles.append(tiles[-1] + (T + 7) // 8)
        to, fo = sg.ragged_frame_plan(lengths, L, S)
        assert to.dtype == fo.dtype == np.int64 and to.tolist() == tiles and fo.tolist() == frames, (lengths, L, S)
    for bad in (([10], 0, 1), ([10], 1, 0), ([-1], 4, 4)):
        with pytest.raises(ValueError):
            sg.ragged_frame_plan(*bad)


def test_the_ragged_symbols_are_exported_and_declared(nv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lidbox_hip.h")).read()
    for name in RAGGED_SYMBOLS:
        assert hasattr(nv.lib, name) and name in nv._SIGS and re.search(r"\b%s\s*\(" % name, header), name


def test_ragged_argument_errors_are_reported_not_thrown(nv):
    """no-compute form: every call is refused on its arguments before anything touches a device"""
    lib = nv.lib
    buf = np.zeros(64, np.float32)
    off = np.zeros(2, np.int64)
    p, o = buf.ctypes.data, off.ctypes.data
    assert lib.lidbox_feat_plan_ragged_ok(None, nv.FEAT_LOGMEL) == 0
    assert lib.lidbox_extract_features_ragged(None, nv.FEAT_LOGMEL, p, o, o, o, 1, 0, 0, p, None, None, 0, None) == -1
    assert "lidbox_extract_features_ragged" in nv.last_error()
    for args, word in (((None, o, 1, 4, 1, p), "NULL"), ((p, None, 1, 4, 1, p), "NULL"), ((p, o, 1, 4, 1, None), "NULL"),
                       ((p, o, -1, 4, 1, p), ">= 0"), ((p, o, 1, -4, 1, p), ">= 0")):
        assert lib.lidbox_cmvn_ragged_fwd(*args, None) == -1
        assert "lidbox_cmvn_ragged_fwd" in nv.last_error() and word in nv.last_error()
    for args, word in (((None, o, 1, 4, 3, 1, p + 16), "NULL"), ((p, None, 1, 4, 3, 1, p + 16), "NULL"), ((p, o, 1, 4, 3, 1, None), "NULL"),
                       ((p, o, -1, 4, 3, 1, p + 16), ">= 0"), ((p, o, 1, 4, 1, 1, p + 16), "window_len"), ((p, o, 1, 4, 0, 1, p + 16), "window_len"),
                       ((p, o, 1, 4, 3, 1, p), "differ")):
        assert lib.lidbox_window_norm_ragged_fwd(*args, None) == -1
        assert "lidbox_window_norm_ragged_fwd" in nv.last_error() and word in nv.last_error()
    with pytest.raises(ValueError):
        nv.check(lib.lidbox_cmvn_ragged_fwd(None, o, 1, 4, 1, p, None))
    # nothing to do: OK without a launch
    assert lib.lidbox_cmvn_ragged_fwd(p, o, 0, 4, 1, p, None) == 0 and lib.lidbox_window_norm_ragged_fwd(p, o, 1, 0, 3, 1, p + 16, None) == 0


def _resource_usage(build, tmp_path, name):
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, name + ".hip"),
                                         "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--offload-arch=gfx950" in cmd
    usage, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and fn:
            usage[fn] = int(m.group(1))
    return usage


def test_ragged_kernels_build_for_gfx950_without_scratch(nv, tmp_path):
    """the 12 ragged instantiations of feat512_stream_kernel (four kinds x {power 2 with 13 and 16 loads, another power with 16}) and
    the two ragged normalisation kernels keep their state in registers"""
    from lidbox_amd import build
    usage = _resource_usage(build, tmp_path, "features")
    # <KIND, POW2, SHADOW, SRC16, NL, RAGGED>: the ragged form is the one whose last template argument is true
    ragged = {k: v for k, v in usage.items() if re.search(r"feat512_stream_kernelILi[0-3]ELb[01]ELb0ELb0ELi1[36]ELb1EEE", k)}
    dense = [k for k in usage if "feat512_stream_kernel" in k and k not in ragged]
    assert len(ragged) == 12 and len(dense) == 24, sorted(usage)
    assert len({re.search(r"ILi([0-3])ELb([01])ELb0ELb0ELi(1[36])E", k).groups() for k in ragged}) == 12
    assert all(v == 0 for v in ragged.values()), ragged
    usage = _resource_usage(build, tmp_path, "norm")
    norm = [k for k in usage if "cmvn_ragged_kernel" in k or "window_norm_ragged_kernel" in k]
    assert len(norm) == 2 and all(usage[k] == 0 for k in norm), usage


def test_ragged_steps_raise_without_a_device(nv):
    from lidbox_amd import features
    from lidbox_amd.data import steps, tf_utils
    from lidbox_amd.features import signal_ops as sg
    with pytest.raises(nv.LidboxHipError):
        features.cmvn_ragged(torch.zeros(5, 3), [0, 2, 5])
    with pytest.raises(nv.LidboxHipError):
        features.window_normalization_ragged(torch.zeros(5, 3), [0, 2, 5], window_len=2)
    ds = [dict(id="u%d" % i, signal=np.ones(n, np.float32), sample_rate=16000) for i, n in enumerate((500, 900))]
    with pytest.raises(ValueError, match="group_by_input_length"):
        list(steps.extract_features(ds, {"type": "mfcc", "ragged_batch_size": 2, "group_by_input_length": {"max_batch_size": 2}}))
    with pytest.raises(ValueError, match="axis"):
        list(steps.normalize([dict(input=torch.zeros(3, 2))], {"key": "input", "ragged": True, "kwargs": {"axis": 0}}))
    if not torch.cuda.is_available():
        with pytest.raises(nv.LidboxHipError):
            list(steps.extract_features(ds, {"type": "logmelspectrogram", "ragged_batch_size": 2}))
        with pytest.raises(nv.LidboxHipError):
            tf_utils.extract_features_ragged([np.ones(500, np.float32)], 16000, "mfcc")
        with pytest.raises(nv.LidboxHipError):
            list(steps.normalize([dict(input=torch.zeros(3, 2)), dict(input=torch.zeros(4, 2))], {"key": "input", "ragged": True, "batch_size": 2}))
        with pytest.raises(nv.LidboxHipError):
            sg.RaggedSignals.from_list([np.ones(8, np.float32)])
