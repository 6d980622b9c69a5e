"""
Host side of the ragged pass of multilevel_attention (no GPU): the new symbol in the header and the ctypes table, its argument
refusals in the no-compute form, the model's new methods and their argument messages, the register budget of the ragged
kernels, and the float64 evidence that a zero-padded batch is no alternative to the ragged pass.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ragged_mla_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "lidbox_mla_attention_ragged_fwd"


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


def test_symbol_declared_and_bound(nv):
    header = open(os.path.join(ROOT, "include", "lidbox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % SYMBOL, header)
    assert m and len(m.group(1).split(",")) == 8, SYMBOL
    assert SYMBOL in nv._SIGS and len(nv._SIGS[SYMBOL][1]) == 8
    assert getattr(nv.lib, SYMBOL).argtypes == nv._SIGS[SYMBOL][1]
    assert nv.lib.lidbox_hip_abi_version() == 1


def test_refusals_before_any_launch(nv):
    """no-compute form: host memory stands in for device buffers; every call below is refused, or returns for an empty batch,
    before anything touches a device"""
    buf = np.full(64, 3.0, np.float32)
    off = np.array([0, 2, 5], np.int64)
    p, o = buf.ctypes.data, off.ctypes.data

    def call(z=p, ro=o, B=2, K=4, att=p, ld=4, cs=p):
        return nv.lib.lidbox_mla_attention_ragged_fwd(z, ro, B, K, att, ld, cs, None)

    for kw in (dict(z=None), dict(ro=None), dict(att=None), dict(B=-1), dict(K=0), dict(K=-3), dict(K=1025, ld=1025), dict(ld=3),
               dict(ld=3, cs=None), dict(z=None, cs=None)):
        assert call(**kw) == -1, kw
        assert SYMBOL in nv.last_error(), (kw, nv.last_error())
    with pytest.raises(ValueError):
        nv.check(call(ld=3))
    assert call(B=0) == 0 and call(B=0, cs=None) == 0
    assert (buf == 3.0).all() and off.tolist() == [0, 2, 5]


def test_model_has_the_methods_the_pipeline_looks_up():
    from lidbox_amd.models import multilevel_attention as mla
    for attr in ("ragged_refusal", "forward_ragged", "predict_ragged", "embed_ragged", "embed"):
        assert callable(getattr(mla.MultilevelAttentionModel, attr)), attr
    assert {"as_embedding_extractor", "MultilevelAttentionModel", "create", "loader"} <= set(mla.__all__)
    m = mla.create((50, 8), 5, H=24, device="cpu", seed=0)
    assert m.ragged_refusal() is None
    e = mla.as_embedding_extractor(m)
    assert callable(e) and callable(e.ragged) and e.model is m


def test_forward_ragged_argument_messages(nv, monkeypatch):
    """the messages of the other models (tests/test_ragged_rnn_gpu.py::test_refusals).  The project's convention puts the
    device check first, so a host tensor is refused as such; with that one check stood in for, every other refusal is
    raised on the host, before a workspace exists or anything is launched (the model lives on the CPU device here)"""
    from lidbox_amd.models import multilevel_attention as mla
    m = mla.create((50, 8), 5, H=24, device="cpu", seed=0)
    X = torch.zeros((9, 8))
    with pytest.raises(nv.LidboxHipError):
        m.predict_ragged(X, [0, 4, 9])
    monkeypatch.setattr(nv, "require_gpu_tensor", lambda t, name, dtype=None: t)
    for call in (m.forward_ragged, m.predict_ragged, m.embed_ragged, mla.as_embedding_extractor(m).ragged):
        with pytest.raises(ValueError, match="length 0"):
            call(X, [0, 3, 3, 9])
        with pytest.raises(ValueError, match="row_offsets"):
            call(X, [0, 4])
        with pytest.raises(ValueError, match="row_offsets"):
            call(X, [1, 9])
        with pytest.raises(ValueError, match="row_offsets"):
            call(X, [0, 5, 4, 9])
        with pytest.raises(ValueError, match=r"\[total_T, 8\]"):
            call(torch.zeros((5, 9)), [0, 5])
        with pytest.raises(ValueError, match="contiguous"):
            call(torch.zeros((5, 16))[:, :8], [0, 5])
    assert getattr(m, "_rws", None) is None


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
    """eight ragged beside the eight dense forward instantiations, one per (VEC, NJ) pair, none with scratch"""
    from lidbox_amd import build
    usage = _resource_usage(build, tmp_path, "mla")
    pairs = lambda kernel: {tuple(int(v) for v in re.search(r"ILi(\d+)ELi(\d+)EEE", k).groups()): s
                            for k, s in usage.items() if re.search(r"\d%sI" % kernel, k)}
    ragged, dense = pairs("mla_attention_ragged_fwd_kernel"), pairs("mla_attention_fwd_kernel")
    assert set(ragged) == set(dense) == rc.ALL_PAIRS, sorted(usage)
    assert all(s == 0 for s in ragged.values()), ragged
    assert all(s == 0 for s in dense.values()), dense
    # the K values of the device tests reach every pair
    assert {(p["vec"], p["nj"]) for p in (rc.kernel_plan(K, s) for K, s in rc.KERNEL_KS)} == rc.ALL_PAIRS


def test_kernel_length_lists_bracket_one_pass():
    assert sorted(rc.kernel_lengths(100)) == [1, 2, 31, 32, 33, 65, 298]
    assert {1, 127, 128, 129} <= set(rc.kernel_lengths(5)) and {1, 1023, 1024, 1025} <= set(rc.kernel_lengths(1))
    for K, s in rc.KERNEL_KS:
        L, P = rc.kernel_lengths(K, s), rc.kernel_plan(K, s)["pass_rows"]
        assert {1, P, P + 1, 2 * P + 1} <= set(L) and L != sorted(L) and min(L) >= 1, (K, L)
    assert (rc.kernel_plan(128, 1)["vec"], rc.kernel_plan(128, 1)["nj"]) == (1, 2)
    assert (rc.kernel_plan(512, 1)["vec"], rc.kernel_plan(512, 1)["nj"]) == (1, 8)


@pytest.mark.parametrize("case", sorted(rc.MODEL_CASES))
def test_a_zero_padded_batch_computes_another_function(case):
    """float64 alone: the shortest utterance, zero-padded to the longest one's 298 frames as a padded dense batch holds it,
    comes out more than H_TOL away from its own output; the longest utterance needs no padding and is unchanged.  The padded
    frames leave every block as relu(BN(bias)) != 0 and enter both sums of every attention level."""
    c = rc.MODEL_CASES[case]
    w, xs, out, emb = rc.model_reference(case)
    assert all(np.abs(v).min() > 0 for k, v in w.items() if k.endswith(".b") or k.endswith(".beta"))
    assert all(np.abs(w[k] - (1.0 if k.endswith("variance") else 0.0)).min() > 0 for k in w if ".moving_" in k)
    T = max(rc.MODEL_LENGTHS)
    short, long_ = int(np.argmin(rc.MODEL_LENGTHS)), int(np.argmax(rc.MODEL_LENGTHS))
    assert len(xs[short]) == 1 and len(xs[long_]) == T == 298
    pad_out, pad_emb = rc.forward64(w, rc.zero_padded(xs[short], T), c["L"])
    d_out, d_emb = float(np.abs(pad_out - out[short]).max()), float(np.abs(pad_emb - emb[short]).max())
    print("%s: padded vs own output of the 1-frame utterance: %.3e (log-probabilities), %.3e (embedding)" % (case, d_out, d_emb))
    assert d_out > rc.H_TOL and d_emb > rc.H_TOL
    same_out, same_emb = rc.forward64(w, rc.zero_padded(xs[long_], T), c["L"])
    assert np.array_equal(same_out, out[long_]) and np.array_equal(same_emb, emb[long_])
    # a padded frame is not a zero row behind the first block
    y1 = np.maximum((w["dense_block1_fc.b"].astype(np.float64) - w["dense_block1_bn.moving_mean"])
                    / np.sqrt(w["dense_block1_bn.moving_variance"] + rc.BN_EPS) * w["dense_block1_bn.gamma"] + w["dense_block1_bn.beta"], 0.0)
    assert (y1 > 0).any()
