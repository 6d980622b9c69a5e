"""
Host-only tests of the recurrent models (lidbox_amd.models.lstm / ap_lstm / rnn) and of the HDF5 reader's LSTM names:
parameter names, layouts and counts as Keras reports them, the Keras initialisation rules and the ap_lstm loader's
width rule.  Models are built on the CPU device: nothing here launches a kernel.
"""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hdf5_lstm_names():
    from lidbox_amd.models.hdf5_reader import keras_param_name
    assert keras_param_name("blstm_1/forward_lstm_1/lstm_cell_1/kernel:0", "blstm_1") == "forward_lstm_1.W"
    assert keras_param_name("blstm_2/backward_lstm_2/lstm_cell_5/recurrent_kernel:0", "blstm_2") == "backward_lstm_2.U"
    assert keras_param_name("lstm/lstm_cell/kernel:0", "lstm") == "lstm.W"
    assert keras_param_name("lstm/lstm_cell/bias:0", "lstm") == "lstm.b"
    assert keras_param_name("lstm/recurrent_kernel:0", "lstm") == "lstm.U"                  # plain form
    assert keras_param_name("blstm_1/forward_lstm_1/kernel:0", "blstm_1") == "forward_lstm_1.W"
    assert keras_param_name("frame1/kernel:0", "frame1") == "frame1.W"                      # unchanged for other layers
    assert keras_param_name("frame2d_1/frame2d_1_bn/gamma:0", "frame2d_1") == "frame2d_1_bn.gamma"


def test_hdf5_lstm_fixture_reads():
    import sys
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_lstm_h5 import AP_LSTM_LAYERS, C, H
    from make_keras_h5 import values
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_ap_lstm_weights.h5"))
    want = {}
    for _, vars_ in AP_LSTM_LAYERS:
        for wname, shape in vars_:
            parts = wname.split("/")
            want[parts[1] + {"kernel:0": ".W", "recurrent_kernel:0": ".U", "bias:0": ".b"}[parts[-1]]] = values(wname, shape)
    assert sorted(w) == sorted(want)
    for k in want:
        assert np.array_equal(w[k], want[k]), k
    assert w["forward_lstm_1.W"].shape == (C, 4 * H) and w["backward_lstm_2.W"].shape == (2 * H, 4 * H)


def test_parameter_counts_and_layouts():
    from lidbox_amd.models import ap_lstm, lstm
    m = ap_lstm.create((198, 40), device="cpu", seed=0)
    assert m.count_params() == 143840
    assert m.output_dim == 248 and m.output_activation is None
    names = ["%s_lstm_%d.%s" % (d, i, v) for i in (1, 2) for d in ("forward", "backward") for v in "WUb"]
    assert list(m.layout) == names
    assert m.layout["forward_lstm_1.W"][1] == (40, 248) and m.layout["backward_lstm_2.W"][1] == (124, 248)
    assert m.layout["forward_lstm_2.U"][1] == (62, 248) and m.layout["backward_lstm_1.b"][1] == (248,)
    assert all(off % 4 == 0 for off, _ in m.layout.values())
    m = lstm.create((None, 40), 10, device="cpu", seed=0)
    H = 1024
    assert m.count_params() == 4 * H * (40 + H + 1) + H * 10 + 10
    assert list(m.layout) == ["lstm.W", "lstm.U", "lstm.b", "output.W", "output.b"]
    assert m.output_activation == "log_softmax" and not m.convs and not m.fused_output_ok()
    with pytest.raises(ValueError):
        lstm.create((None, 40), 10, num_units=8, device="cpu", compute_dtype="bfloat16")


def test_keras_initialisation_rules():
    from lidbox_amd.models import ap_lstm
    m = ap_lstm.create((50, 20), num_lstm_units=30, device="cpu", seed=7)
    w = m.get_weights()
    for half in ("forward_lstm_1", "backward_lstm_2"):
        U = w[half + ".U"].astype(np.float64)
        assert np.allclose(U @ U.T, np.eye(30), atol=1e-5)                  # orthogonal: orthonormal rows
        b = w[half + ".b"]
        assert np.array_equal(b[30:60], np.ones(30, np.float32)) and not b[:30].any() and not b[60:].any()
        W = w[half + ".W"]
        lim = np.sqrt(6.0 / (W.shape[0] + W.shape[1]))
        assert np.abs(W).max() <= lim and np.abs(W).max() > 0.9 * lim      # glorot_uniform
    w2 = ap_lstm.create((50, 20), num_lstm_units=30, device="cpu", seed=7).get_weights()
    assert all(np.array_equal(w[k], w2[k]) for k in w)


def test_ap_lstm_loader_width_rule():
    from lidbox_amd.models import ap_lstm
    m = ap_lstm.loader((50, 20), 8, num_lstm_units=2, device="cpu", seed=0)
    assert m.output_dim == 8
    with pytest.raises(ValueError):
        ap_lstm.loader((50, 20), 9, num_lstm_units=2, device="cpu")
    with pytest.raises(ValueError):
        ap_lstm.loader((50, 20), 300, device="cpu")


def test_native_lstm_queries():
    from lidbox_amd import _native as nv
    assert [nv.lib.lidbox_lstm_resident_ok(h) for h in (0, 1, 62, 80, 81, 1024)] == [0, 1, 1, 1, 0, 0]
    assert nv.lib.lidbox_lstm_workspace(256, 198, 62, 2) == 0
    assert nv.lib.lidbox_lstm_workspace(256, 198, 1024, 1) >= 2 * 256 * 1024 * 4
    assert nv.lib.lidbox_lstm_fwd(None, None, 1, 4, 10, 8, None, None, None, None, 0, None) == -1
    assert nv.lib.lidbox_lstm_bwd(None, None, 3, 4, 10, 8, None, None, None, 0, None, None, 0, None) == -1
