"""
Host side of the ragged model pass (no GPU): the invariants of models/ragged.ragged_plan, a float64 simulation of the layout it
describes -- one GEMM over all rows per layer, the pad-row repair, slack rows left as NaN -- against the oracle's causal convolution
of every utterance alone, and the argument refusals of the new C-ABI entry points in the no-compute form.
"""
import os
import re

import numpy as np
import pytest

from oracle import model_np as mo

STACKS = {
    "xvector": [(5, 1), (3, 2), (3, 3), (1, 1), (1, 1)],
    "xvector_extended": [(5, 1), (1, 1), (3, 2), (1, 1), (3, 3), (1, 1), (3, 4), (1, 1), (1, 1), (1, 1)],
    "odd": [(4, 3), (2, 2), (5, 1), (3, 5)],
}
PLAN_LENGTHS = list(range(1, 65)) + [198, 300, 1000]
SIM_LENGTHS = [1, 2, 3, 5, 6, 7, 23, 24, 25, 61, 198, 300]
RAGGED_SYMBOLS = ("lidbox_ragged_pack_rows", "lidbox_ragged_zero_rows", "lidbox_stats_pool_ragged_fwd", "lidbox_avg_pool_ragged_fwd")


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


@pytest.mark.parametrize("stack", sorted(STACKS))
def test_plan_invariants(nv, stack):
    from lidbox_amd.models.ragged import ragged_plan
    convs = STACKS[stack]
    n = len(convs)
    plan = ragged_plan(PLAN_LENGTHS, convs)
    assert plan.pads == [k - 1 for k, _ in convs] + [0] and plan.cum[n] == 1 and len(plan.T) == n + 1
    assert plan.off.dtype == np.int64 and plan.off[0] == 0 and np.array_equal(np.diff(plan.off), plan.L)
    assert np.array_equal(plan.T[0], PLAN_LENGTHS)
    for i, (k, s) in enumerate(convs):
        assert plan.cum[i] == s * plan.cum[i + 1]
        assert np.array_equal(plan.T[i + 1], [mo.conv1d_out_len(int(t), s) for t in plan.T[i]])
        # level i segments are exactly s_i times the level i + 1 segments, at s_i times their start
        assert np.array_equal(plan.seg_offsets(i), s * plan.seg_offsets(i + 1))
    for i in range(n + 1):
        seg = np.diff(plan.seg_offsets(i))
        assert (seg >= plan.pads[i] + plan.T[i]).all(), i                      # pad + frames fit
        assert plan.rows[i] == plan.seg_offsets(i)[-1] == plan.off[-1] * plan.cum[i]
    # no smaller top-level segment would do for any utterance
    tight = np.zeros(len(PLAN_LENGTHS), bool)
    for i in range(n + 1):
        tight |= (plan.L - 1) * plan.cum[i] < plan.pads[i] + plan.T[i]
    assert tight.all()
    # the plan of an utterance does not depend on its neighbours
    alone = ragged_plan([300], convs)
    j = PLAN_LENGTHS.index(300)
    assert alone.L[0] == plan.L[j] and all(alone.T[i][0] == plan.T[i][j] for i in range(n + 1))
    for bad in ([0], [5, 0, 3], [-1]):
        with pytest.raises(ValueError, match="at least one frame"):
            ragged_plan(bad, convs)
    with pytest.raises(ValueError):
        ragged_plan([5], [(0, 1)])
    empty = ragged_plan([], convs)
    assert empty.B == 0 and empty.off.tolist() == [0] and empty.rows == [0] * (n + 1)


@pytest.mark.parametrize("stack", sorted(STACKS))
def test_layout_simulation_equals_the_convolution_of_every_utterance_alone(nv, stack):
    """float64: what the device pass does, row for row.  Slack rows and the rows behind a level start as NaN and the GEMM of a layer
    computes EVERY row, so a valid output that read slack, a neighbour's frames or an unrepaired pad row would not match."""
    from lidbox_amd.models.ragged import ragged_plan
    convs = STACKS[stack]
    n = len(convs)
    rng = np.random.default_rng(5)
    chans = [3] + [int(rng.integers(2, 6)) for _ in convs]
    Ws = [rng.standard_normal((k, chans[i], chans[i + 1])) for i, (k, _) in enumerate(convs)]
    bs = [rng.standard_normal(chans[i + 1]) + 0.5 for i in range(n)]          # relu(bias) != 0: the pad rows need their repair
    xs = [rng.standard_normal((t, chans[0])) for t in SIM_LENGTHS]
    plan = ragged_plan(SIM_LENGTHS, convs)
    B = len(xs)
    # pack: every row of every segment, zero rows behind the last one
    level = np.full((plan.rows[0] + convs[0][0] - 1, chans[0]), np.nan)
    level[plan.rows[0]:] = 0.0
    seg = plan.seg_offsets(0)
    for b, x in enumerate(xs):
        level[seg[b]:seg[b + 1]] = 0.0
        level[seg[b] + plan.pads[0]:seg[b] + plan.pads[0] + len(x)] = x
    refs = xs
    for i, (k, s) in enumerate(convs):
        p = plan.pads[i + 1]
        M = plan.rows[i + 1] - p
        tail = convs[i + 1][0] - 1 if i + 1 < n else 0
        nxt = np.full((plan.rows[i + 1] + tail, chans[i + 1]), np.nan)        # also behind the level: finite or not, never read
        nxt[:p] = 0.0
        idx = np.arange(M)[:, None] * s + np.arange(k)[None, :]
        assert idx.max() < len(level)
        A = level[idx].reshape(M, k * chans[i])                               # the batch = 1 rows descriptor, row stride s C
        with np.errstate(invalid="ignore"):
            nxt[p:p + M] = np.maximum(A @ Ws[i].reshape(k * chans[i], chans[i + 1]) + bs[i], 0)
        seg = plan.seg_offsets(i + 1)
        if p > 0:
            assert B < 2 or (nxt[seg[1]:seg[1] + p] != 0).any()               # the GEMM did write the pad rows of utterance 1 ...
            for b in range(B):
                nxt[seg[b]:seg[b] + p] = 0.0                                  # ... lidbox_ragged_zero_rows
        refs = [mo.conv1d_causal_fwd(r[None], Ws[i], bs[i], s, relu=True)[0] for r in refs]
        for b, r in enumerate(refs):
            got = nxt[seg[b] + p:seg[b] + p + plan.T[i + 1][b]]
            assert got.shape == r.shape and np.isfinite(got).all(), (i, b)
            assert np.abs(got - r).max() <= 1e-12, (i, b, np.abs(got - r).max())
        level = nxt


def test_the_ragged_symbols_are_exported_and_declared(nv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lidbox_hip.h")).read()
    for name in RAGGED_SYMBOLS:
        assert hasattr(nv.lib, name) and name in nv._SIGS and re.search(r"\b%s\s*\(" % name, header), name


def test_ragged_argument_errors_are_reported_not_thrown(nv):
    """no-compute form: every call is refused on its arguments (or has nothing to do) before anything touches a device"""
    lib = nv.lib
    buf = np.zeros(64, np.float32)
    off = np.zeros(2, np.int64)
    p, o = buf.ctypes.data, off.ctypes.data
    for args, word in (((None, o, p, o, 1, 4, 1, 0), "NULL"), ((p, None, p, o, 1, 4, 1, 0), "NULL"), ((p, o, None, o, 1, 4, 1, 0), "NULL"),
                       ((p, o, p, None, 1, 4, 1, 0), "NULL"), ((p, o, p, o, -1, 4, 1, 0), ">= 0"), ((p, o, p, o, 1, 0, 1, 0), "C >= 1"),
                       ((p, o, p, o, 1, 4, -1, 0), ">= 0"), ((p, o, p, o, 1, 4, 1, -1), ">= 0")):
        assert lib.lidbox_ragged_pack_rows(*args, None) == -1
        assert "lidbox_ragged_pack_rows" in nv.last_error() and word in nv.last_error()
    for args, word in (((None, o, 1, 4, 1), "NULL"), ((p, None, 1, 4, 1), "NULL"), ((p, o, -1, 4, 1), ">= 0"), ((p, o, 1, 0, 1), "C >= 1"),
                       ((p, o, 1, 4, -1), ">= 0")):
        assert lib.lidbox_ragged_zero_rows(*args, None) == -1
        assert "lidbox_ragged_zero_rows" in nv.last_error() and word in nv.last_error()
    for name in ("lidbox_stats_pool_ragged_fwd", "lidbox_avg_pool_ragged_fwd"):
        fn = getattr(lib, name)
        for args, word in (((None, 4, o, o, 1, 4, p), "NULL"), ((p, 4, None, o, 1, 4, p), "NULL"), ((p, 4, o, None, 1, 4, p), "NULL"),
                           ((p, 4, o, o, 1, 4, None), "NULL"), ((p, 4, o, o, -1, 4, p), "B >= 0"), ((p, 4, o, o, 1, 0, p), "C >= 1"),
                           ((p, 3, o, o, 1, 4, p), "row_stride")):
            assert fn(*args, None) == -1
            assert name in nv.last_error() and word in nv.last_error()
        assert fn(p, 4, o, o, 0, 4, p, None) == 0                              # B == 0: OK, nothing touched
    with pytest.raises(ValueError):
        nv.check(lib.lidbox_ragged_zero_rows(None, o, 1, 4, 1, None))
    assert lib.lidbox_ragged_pack_rows(p, o, p, o, 0, 4, 1, 3, None) == 0
    assert lib.lidbox_ragged_zero_rows(p, o, 0, 4, 1, None) == 0 and lib.lidbox_ragged_zero_rows(p, o, 1, 4, 0, None) == 0
    assert not buf.any()


def test_ragged_kernels_build_for_gfx950_without_scratch(nv, tmp_path):
    """two instantiations (16-byte / scalar accesses) of the pack and the repair kernel, four of the pooling kernel"""
    import subprocess
    from lidbox_amd import build
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "ragged.hip"),
                                         "-o", str(tmp_path / "ragged.o")]
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
    for kernel, count in (("pack_rows_kernel", 2), ("zero_rows_kernel", 2), ("pool_ragged_kernel", 4)):
        assert sum(kernel in k for k in usage) == count, sorted(usage)
    assert len(usage) == 8 and all(v == 0 for v in usage.values()), usage


def test_ragged_entry_points_raise_without_a_device(nv):
    import torch
    from lidbox_amd import util
    from lidbox_amd.data import steps
    assert set(steps.VALID_STEP_FUNCTIONS) == {          # exactly the keys it had before the ragged options
        "apply_filters", "apply_vad", "as_supervised", "augment_by_additive_noise", "augment_signals", "cache", "compute_rms_vad",
        "consume", "consume_to_tensorboard", "create_input_chunks", "create_signal_chunks", "drop_empty", "extract_embeddings",
        "extract_features", "filter_keys_in_set", "initialize", "lambda", "load_audio", "normalize", "random_signal_fir_filtering",
        "random_signal_speed_change", "remap_keys", "repeat_too_short_signals", "shuffle"}
    with pytest.raises(ValueError, match="no_unbatch"):
        list(steps.extract_embeddings([], {"extractors": [], "ragged": True, "no_unbatch": True}))
    with pytest.raises(ValueError, match="ragged form"):
        list(steps.extract_embeddings([], {"extractors": [lambda x: x], "ragged": True}))
    with pytest.raises(ValueError, match="launch_batch"):
        util.predict_ragged_with_model(None, [], launch_batch=0)
    assert len(util.predict_ragged_with_model(None, [])) == 0
    if not torch.cuda.is_available():
        from lidbox_amd.models import xvector
        with pytest.raises(nv.LidboxHipError):
            xvector.create((None, 40), 4)
