"""
Host-only tests of the spherespeaker model (lidbox_amd.models.spherespeaker), of the HDF5 reader's wrapper-and-direction
rule for Bidirectional LSTM halves and of the fused LSTM step entry points' argument checks: parameter names, layouts and
counts as Keras reports them and the Keras initialisation rules.  Models are built on the CPU device: nothing here launches
a kernel.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "keras_spherespeaker_weights.h5")


def test_spherespeaker_parameter_counts_and_layouts():
    from lidbox_amd.models import spherespeaker
    C, N, H, E = 40, 10, 250, 1000
    m = spherespeaker.create((198, C), N, device="cpu", seed=0)
    lstm1 = 2 * 4 * H * (C + H + 1)
    lstm23 = 2 * 2 * 4 * H * (2 * H + H + 1)
    dense = (6 * H * E + E) + (E * N + N)
    bn = 4 * 6 * H + 4 * E
    assert m.count_params() == lstm1 + lstm23 + dense + bn == 5107010
    assert m.output_dim == N and m.output_activation == "log_softmax"
    halves = ["blstm_%d_%s.%s" % (i, d, v) for i in (1, 2, 3) for d in ("forward", "backward") for v in "WUb"]
    assert list(m.layout) == halves + ["blstm_bn.gamma", "blstm_bn.beta", "fc_relu.W", "fc_relu.b", "pool_bn.gamma",
                                       "pool_bn.beta", "outputs.W", "outputs.b"]
    assert m.layout["blstm_1_forward.W"][1] == (C, 4 * H) and m.layout["blstm_2_backward.W"][1] == (2 * H, 4 * H)
    assert m.layout["blstm_3_forward.U"][1] == (H, 4 * H) and m.layout["blstm_1_backward.b"][1] == (4 * H,)
    assert m.layout["blstm_bn.gamma"][1] == (6 * H,) and m.layout["fc_relu.W"][1] == (6 * H, E)
    assert m.layout["pool_bn.beta"][1] == (E,) and m.layout["outputs.W"][1] == (E, N) and m.layout["outputs.b"][1] == (N,)
    assert list(m.state_layout) == ["%s.%s" % (b, s) for b in ("blstm_bn", "pool_bn") for s in ("moving_mean", "moving_variance")]
    assert m.state_layout["blstm_bn.moving_variance"][1] == (6 * H,) and m.state_layout["pool_bn.moving_mean"][1] == (E,)
    assert all(off % 4 == 0 for off, _ in list(m.layout.values()) + list(m.state_layout.values()))
    assert not m.convs and not m.fused_output_ok()
    assert m.keras_blstm_by_wrapper
    with pytest.raises(ValueError):
        spherespeaker.create((198, C), N, device="cpu", compute_dtype="bfloat16")
    small = spherespeaker.create((50, 12), 3, embedding_dim=24, num_lstm_units=20, device="cpu", seed=0, output_activation=None)
    assert small.layout["blstm_2_forward.W"][1] == (40, 80) and small.layout["fc_relu.W"][1] == (120, 24)
    assert small.output_activation is None


def test_spherespeaker_keras_initialisation_rules():
    from lidbox_amd.models import spherespeaker
    H = 30
    kw = dict(device="cpu", seed=7, num_lstm_units=H, embedding_dim=16)
    m = spherespeaker.create((50, 20), 4, **kw)
    w = m.get_weights()
    for half in ("blstm_1_forward", "blstm_2_backward", "blstm_3_forward"):
        U = w[half + ".U"].astype(np.float64)
        assert np.allclose(U @ U.T, np.eye(H), atol=1e-5)                   # orthogonal: orthonormal rows
        b = w[half + ".b"]
        assert (b[H:2 * H] == 1).all() and not b[:H].any() and not b[2 * H:].any()      # unit_forget_bias
        W = w[half + ".W"]
        lim = np.sqrt(6.0 / (W.shape[0] + W.shape[1]))
        assert np.abs(W).max() <= lim and np.abs(W).max() > 0.9 * lim       # glorot_uniform
    for d in ("fc_relu", "outputs"):
        W = w[d + ".W"]
        lim = np.sqrt(6.0 / (W.shape[0] + W.shape[1]))
        assert np.abs(W).max() <= lim and np.abs(W).max() > 0.8 * lim and not w[d + ".b"].any()
    for bn in ("blstm_bn", "pool_bn"):
        assert (w[bn + ".gamma"] == 1).all() and not w[bn + ".beta"].any()
        assert not w[bn + ".moving_mean"].any() and (w[bn + ".moving_variance"] == 1).all()
    w2 = spherespeaker.create((50, 20), 4, **kw).get_weights()
    assert all(np.array_equal(w[k], w2[k]) for k in w)


def test_spherespeaker_module_interface():
    from lidbox_amd.models import spherespeaker
    assert spherespeaker.loader is spherespeaker.create
    m = spherespeaker.loader((50, 20), 3, device="cpu", seed=0, num_lstm_units=8, embedding_dim=8)
    assert callable(spherespeaker.as_embedding_extractor(m))


def test_hdf5_blstm_names_by_wrapper():
    from lidbox_amd.models.hdf5_reader import keras_param_name
    name = "blstm_2/forward_lstm_7/lstm_cell_22/kernel:0"
    assert keras_param_name(name, "blstm_2", blstm_by_wrapper=True) == "blstm_2_forward.W"
    assert keras_param_name("blstm_3/backward_lstm_8/lstm_cell_26/recurrent_kernel:0", "blstm_3", True) == "blstm_3_backward.U"
    assert keras_param_name("blstm_1/backward_lstm/bias:0", "blstm_1", blstm_by_wrapper=True) == "blstm_1_backward.b"
    assert keras_param_name("blstm_bn/moving_mean:0", "blstm_bn", blstm_by_wrapper=True) == "blstm_bn.moving_mean"
    assert keras_param_name("outputs/kernel:0", "outputs", blstm_by_wrapper=True) == "outputs.W"
    # without the argument: ap_lstm's rule, unchanged
    assert keras_param_name(name, "blstm_2") == "forward_lstm_7.W"
    assert keras_param_name("blstm_1/forward_lstm_1/lstm_cell_1/kernel:0", "blstm_1") == "forward_lstm_1.W"
    assert keras_param_name("blstm_1/forward_lstm_1/lstm_cell_1/kernel:0", "blstm_1", False) == "forward_lstm_1.W"
    assert keras_param_name("blstm/forward_lstm_3/lstm_cell_10/kernel:0", "blstm") == "blstm_forward.W"


def _fixture_tables():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_keras_spherespeaker_h5 as fx
    from make_keras_h5 import values
    return fx, values


def test_hdf5_spherespeaker_fixture_reads():
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    from lidbox_amd.models.keras_utils import read_weights_file
    fx, values = _fixture_tables()
    variables = [(wname, shape) for _, vars_ in fx.SPHERESPEAKER_LAYERS for wname, shape in vars_]
    want = {fx.expected_name(wname): values(wname, shape) for wname, shape in variables}
    assert len(want) == len(variables) == 30                      # nothing lands on another variable's name
    for w in (load_keras_weights(FIXTURE, blstm_by_wrapper=True), read_weights_file(FIXTURE, blstm_by_wrapper=True)):
        assert sorted(w) == sorted(want)
        for k in want:
            assert np.array_equal(w[k], want[k]), k
        assert w["blstm_1_forward.W"].shape == (fx.C, 4 * fx.H) and w["blstm_3_backward.W"].shape == (2 * fx.H, 4 * fx.H)
    # without the argument the halves keep their (session-numbered) inner names
    old = load_keras_weights(FIXTURE)
    assert "forward_lstm_7.W" in old and "blstm_2_forward.W" not in old


def test_spherespeaker_fixture_names_match_model_layout():
    from lidbox_amd.models import spherespeaker
    from lidbox_amd.models.keras_utils import read_model_weights
    fx, _ = _fixture_tables()
    m = spherespeaker.create((20, fx.C), fx.N, embedding_dim=fx.E, num_lstm_units=fx.H, device="cpu", seed=0)
    w = read_model_weights(m, FIXTURE)                             # the model asks for the wrapper-and-direction rule
    want = dict(list(m.layout.items()) + list(m.state_layout.items()))
    assert sorted(want) == sorted(w)
    for n, (_, shape) in want.items():
        assert w[n].shape == tuple(shape), n


def test_native_lstm_step_queries():
    from lidbox_amd import _native as nv
    lib = nv.lib
    B, T, H = 256, 198, 250
    assert lib.lidbox_lstm_step_workspace(B, T, H, 2) >= 2 * B * H * 4            # backward's carried dc
    assert lib.lidbox_lstm_step_workspace(B, T, H, 1) >= B * H * 4
    assert lib.lidbox_lstm_step_workspace(0, T, H, 2) == 0
    # host memory stands in for device buffers: every call below is refused before anything is launched
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data

    def fwd(U0=p, U1=p, dirs=2, zg=p, hseq=p, rs=16, cseq=p):
        return lib.lidbox_lstm_step_fwd(U0, U1, dirs, 4, 10, 8, zg, hseq, rs, cseq, None, 0, None)

    def bwd(U0=p, U1=p, dirs=2, zg=p, cseq=p, dh=p, bs=160, rs=16, dl=None, ws=p, wsn=1 << 20):
        return lib.lidbox_lstm_step_bwd(U0, U1, dirs, 4, 10, 8, zg, cseq, dh, bs, rs, dl, ws, wsn, None)

    for call, fn in ((fwd, "lidbox_lstm_step_fwd"), (bwd, "lidbox_lstm_step_bwd")):
        for kw in (dict(U0=None), dict(U1=None), dict(dirs=3), dict(dirs=0), dict(zg=None), dict(cseq=None), dict(rs=15)):
            assert call(**kw) == -1, (fn, kw)
            assert fn in nv.last_error(), (fn, kw, nv.last_error())
    assert fwd(hseq=None) == -1 and "lidbox_lstm_step_fwd" in nv.last_error()
    assert bwd(dh=None) == -1 and "lidbox_lstm_step_bwd" in nv.last_error()          # neither dh_seq nor dh_last
    assert bwd(bs=100) == -1 and "lidbox_lstm_step_bwd" in nv.last_error()           # utterances would overlap
    assert bwd(ws=None) == -1 and bwd(wsn=8) == -1 and "lidbox_lstm_step_bwd" in nv.last_error()
    assert fwd(dirs=1, U1=None, rs=7) == -1                                          # h_row_stride < dirs * H
