"""
Host-only tests of the multilevel_attention model (lidbox_amd.models.multilevel_attention): parameter names, layouts and
counts as Keras reports them, the Keras initialisation rules, the module interface, the Keras HDF5 fixture (subclassed
DenseBlock / Attention layers: variables under the outer layer's group with the inner layer's scope) and the new native entry
points' declarations and argument checks.  Models are built on the CPU device: nothing here launches a kernel.
"""
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "keras_multilevel_attention_weights.h5")
NEW_SYMBOLS = ("lidbox_mla_attention_fwd", "lidbox_mla_attention_bwd", "lidbox_bn_relu_dropout_fwd", "lidbox_bn_relu_dropout_bwd")


def _expected_count(D, H, L, K):
    return sum((D if l == 0 else H) * H + H + 4 * H + H * K + K for l in range(L)) + L * K * K + K


@pytest.mark.parametrize("D,H,L,K", [(40, 512, 2, 100), (40, 8, 20, 1), (13, 77, 3, 7), (5, 1, 1, 3)])
def test_parameter_counts_and_layouts(D, H, L, K):
    from lidbox_amd.models import multilevel_attention
    m = multilevel_attention.create((198, D), K, L=L, H=H, device="cpu", seed=0)
    assert m.count_params() == _expected_count(D, H, L, K)
    names = []
    for l in range(1, L + 1):
        names += ["dense_block%d_fc.W" % l, "dense_block%d_fc.b" % l, "dense_block%d_bn.gamma" % l, "dense_block%d_bn.beta" % l,
                  "attention%d_input.W" % l, "attention%d_input.b" % l]
    assert list(m.layout) == names + ["outputs.W", "outputs.b"]
    assert list(m.state_layout) == ["dense_block%d_bn.%s" % (l, s) for l in range(1, L + 1) for s in ("moving_mean", "moving_variance")]
    assert m.layout["dense_block1_fc.W"][1] == (D, H) and m.layout["dense_block%d_fc.W" % L][1] == ((D if L == 1 else H), H)
    assert m.layout["dense_block1_fc.b"][1] == (H,) and m.layout["dense_block1_bn.gamma"][1] == (H,)
    assert m.layout["attention%d_input.W" % L][1] == (H, K) and m.layout["attention1_input.b"][1] == (K,)
    assert m.layout["outputs.W"][1] == (L * K, K) and m.layout["outputs.b"][1] == (K,)
    assert m.state_layout["dense_block1_bn.moving_variance"][1] == (H,)
    assert all(off % 4 == 0 for off, _ in list(m.layout.values()) + list(m.state_layout.values()))
    assert m.output_dim == K and m.output_activation == "log_softmax" and m.dropout_rate == 0.4
    assert not m.convs and not m.fused_output_ok()
    w = m.get_weights()
    assert sorted(w) == sorted(list(m.layout) + list(m.state_layout))
    assert sum(v.size for v in w.values()) == m.count_params()


def test_reference_default_size():
    from lidbox_amd.models import multilevel_attention
    m = multilevel_attention.create((198, 40), 100, device="cpu", seed=0)
    assert m.levels == 2 and m.units == 512
    assert m.count_params() == (40 * 512 + 512 + 2048 + 51200 + 100) + (512 * 512 + 512 + 2048 + 51200 + 100) + 20000 + 100


def test_keras_initialisation_rules():
    from lidbox_amd.models import multilevel_attention
    kw = dict(device="cpu", seed=7, L=3, H=48)
    m = multilevel_attention.create((50, 20), 6, **kw)
    w = m.get_weights()
    for n in m.layout:
        if n.endswith(".W"):
            lim = np.sqrt(6.0 / sum(w[n].shape))
            assert np.abs(w[n]).max() <= lim and np.abs(w[n]).max() > 0.8 * lim, n      # glorot_uniform
            assert abs(float(w[n].mean())) < 0.2 * lim, n
        elif n.endswith(".b") or n.endswith(".beta"):
            assert not w[n].any(), n
        else:
            assert n.endswith(".gamma") and (w[n] == 1).all(), n
    for n in m.state_layout:
        assert (w[n] == (1 if n.endswith("variance") else 0)).all(), n
    w2 = multilevel_attention.create((50, 20), 6, **kw).get_weights()
    assert all(np.array_equal(w[k], w2[k]) for k in w)
    w3 = multilevel_attention.create((50, 20), 6, **dict(kw, seed=8)).get_weights()
    assert not np.array_equal(w["dense_block1_fc.W"], w3["dense_block1_fc.W"])


def test_module_interface():
    from lidbox_amd.models import multilevel_attention
    assert multilevel_attention.loader is multilevel_attention.create
    assert {"create", "loader"} <= set(multilevel_attention.__all__)
    params = list(inspect.signature(multilevel_attention.create).parameters)
    assert params[:5] == ["input_shape", "num_outputs", "output_activation", "L", "H"]      # the reference's positional order
    sig = inspect.signature(multilevel_attention.create).parameters
    assert sig["output_activation"].default == "log_softmax" and sig["L"].default == 2 and sig["H"].default == 512
    assert sig["dropout_rate"].default == 0.4 and sig["compute_dtype"].default == "float32"
    m = multilevel_attention.loader((50, 20), 3, "softmax", 4, 16, device="cpu", seed=0)
    assert m.output_activation == "softmax" and m.levels == 4 and m.units == 16
    assert multilevel_attention.create((50, 20), 3, None, device="cpu", H=8).output_activation is None
    assert multilevel_attention.create((50, 20), 3, "", device="cpu", H=8).output_activation is None
    for dt in ("bfloat16", "float16"):
        with pytest.raises(ValueError):
            multilevel_attention.create((50, 20), 3, device="cpu", H=8, compute_dtype=dt)
    with pytest.raises(ValueError):
        multilevel_attention.create((50, 20), 3, "sigmoid", device="cpu", H=8)
    for bad in (dict(L=0), dict(H=0), dict(dropout_rate=1.0)):
        with pytest.raises(ValueError):
            multilevel_attention.create((50, 20), 3, device="cpu", **dict(dict(H=8), **bad))
    with pytest.raises(ValueError):
        multilevel_attention.create((50, 20), 0, device="cpu", H=8)


def test_level_dropout_seeds_differ_per_level_and_rank():
    from lidbox_amd.models import multilevel_attention
    m = multilevel_attention.create((50, 20), 3, device="cpu", seed=0, L=20, H=8)
    seeds = [m.level_dropout_seed(l) for l in range(20)]
    assert len(set(seeds)) == 20 and all(0 <= s < 2 ** 64 for s in seeds)
    m.dropout_seed_mix = 0x9E3779B97F4A7C15
    assert not set(seeds) & {m.level_dropout_seed(l) for l in range(20)}


def _fixture_tables():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_keras_multilevel_attention_h5 as fx
    from make_keras_h5 import values
    return fx, values


def test_hdf5_fixture_reads():
    from lidbox_amd.models.hdf5_reader import keras_param_name, load_keras_weights
    from lidbox_amd.models.keras_utils import read_weights_file
    fx, values = _fixture_tables()
    assert [n for n, _ in fx.MULTILEVEL_ATTENTION_LAYERS] == ["input", "dense_block1", "attention1", "dense_block2", "attention2",
                                                              "attention_concat", "outputs", "log_softmax"]
    assert keras_param_name("dense_block1/dense_block1_fc/kernel:0", "dense_block1") == "dense_block1_fc.W"
    assert keras_param_name("dense_block1/dense_block1_bn/moving_mean:0", "dense_block1") == "dense_block1_bn.moving_mean"
    assert keras_param_name("attention2/attention2_input/bias:0", "attention2") == "attention2_input.b"
    variables = [(wname, shape) for _, vars_ in fx.MULTILEVEL_ATTENTION_LAYERS for wname, shape in vars_]
    want = {fx.expected_name(wname): values(wname, shape) for wname, shape in variables}
    assert len(want) == len(variables) == 2 * 8 + 2                  # nothing lands on another variable's name
    for w in (load_keras_weights(FIXTURE), read_weights_file(FIXTURE)):
        assert sorted(w) == sorted(want)
        for k in want:
            assert np.array_equal(w[k], want[k]), k


def test_fixture_names_match_model_layout():
    from lidbox_amd.models import multilevel_attention
    from lidbox_amd.models.keras_utils import read_model_weights
    fx, _ = _fixture_tables()
    m = multilevel_attention.create((20, fx.D), fx.K, L=fx.L, H=fx.H, device="cpu", seed=0)
    w = read_model_weights(m, FIXTURE)
    want = dict(list(m.layout.items()) + list(m.state_layout.items()))
    assert sorted(want) == sorted(w)
    for n, (_, shape) in want.items():
        assert w[n].shape == tuple(shape), n


def test_new_symbols_declared_and_bound():
    from lidbox_amd import _native as nv
    with open(os.path.join(os.path.dirname(HERE), "include", "lidbox_hip.h")) as fh:
        header = fh.read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in nv._SIGS and getattr(nv.lib, sym).argtypes == nv._SIGS[sym][1], sym
    assert nv.lib.lidbox_hip_abi_version() == 1


def test_native_refusals_before_any_launch():
    """host memory stands in for device buffers: every call below is refused, or returns for an empty batch, before anything
    is launched"""
    from lidbox_amd import _native as nv
    lib = nv.lib
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def fwd(z=p, B=2, T=3, K=4, att=p, ld=4, cs=p):
        return lib.lidbox_mla_attention_fwd(z, B, T, K, att, ld, cs, None)

    def bwd(z=p, att=p, ld=4, cs=p, datt=p, ldd=4, B=2, T=3, K=4, dz=p):
        return lib.lidbox_mla_attention_bwd(z, att, ld, cs, datt, ldd, B, T, K, dz, None)

    for kw in (dict(z=None), dict(att=None), dict(cs=None), dict(T=0), dict(T=-1), dict(K=0), dict(K=-3), dict(B=-1), dict(ld=3),
               dict(K=1025, ld=1025)):
        assert fwd(**kw) == -1, kw
        assert "lidbox_mla_attention_fwd" in nv.last_error(), (kw, nv.last_error())
    for kw in (dict(z=None), dict(att=None), dict(cs=None), dict(datt=None), dict(dz=None), dict(T=0), dict(K=0), dict(B=-1),
               dict(ld=3), dict(ldd=3)):
        assert bwd(**kw) == -1, kw
        assert "lidbox_mla_attention_bwd" in nv.last_error(), (kw, nv.last_error())
    assert fwd(B=0) == 0 and bwd(B=0) == 0

    def ffwd(x=p, R=4, C=4, sc=p, sh=p, rate=0.4, y=p):
        return lib.lidbox_bn_relu_dropout_fwd(x, R, C, sc, sh, rate, 1, None, y, None)

    def fbwd(x=p, R=4, C=4, sc=p, sh=p, rate=0.4, dy=p, dx=p):
        return lib.lidbox_bn_relu_dropout_bwd(x, R, C, sc, sh, rate, 1, None, dy, dx, None)

    for kw in (dict(x=None), dict(sc=None), dict(sh=None), dict(y=None), dict(R=-1), dict(C=0), dict(rate=1.0), dict(rate=-0.1)):
        assert ffwd(**kw) == -1, kw
        assert "lidbox_bn_relu_dropout_fwd" in nv.last_error(), (kw, nv.last_error())
    for kw in (dict(x=None), dict(sc=None), dict(sh=None), dict(dy=None), dict(dx=None), dict(R=-1), dict(C=0), dict(rate=1.0)):
        assert fbwd(**kw) == -1, kw
        assert "lidbox_bn_relu_dropout_bwd" in nv.last_error(), (kw, nv.last_error())
    assert ffwd(R=0) == 0 and fbwd(R=0) == 0
