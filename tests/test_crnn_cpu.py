"""
Host-only tests of the crnn model (lidbox_amd.models.crnn / conv_rnn) and of the HDF5 reader's Bidirectional LSTM names:
shape bookkeeping, parameter names, layouts and counts as Keras reports them, the input-size and dtype checks and the native
conv entry points' argument checks.  Models are built on the CPU device: nothing here launches a kernel.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pooled_sizes_odd():
    from lidbox_amd.models.conv_rnn import pooled_sizes
    assert pooled_sizes(198, 40, 5) == [(198, 40), (99, 20), (49, 10), (24, 5), (12, 2), (6, 1)]
    assert pooled_sizes(37, 33, 5) == [(37, 33), (18, 16), (9, 8), (4, 4), (2, 2), (1, 1)]


def test_crnn_lstm_input_width():
    from lidbox_amd.models import crnn
    assert crnn.create((198, 40), 10, device="cpu", seed=0).lstm_input_dim == 1 * 256
    assert crnn.create((50, 64), 10, device="cpu", seed=0).lstm_input_dim == 2 * 256
    m = crnn.create((45, 97), 4, device="cpu", seed=0, filters=(16, 16, 16, 32, 48), num_units=8)
    assert m.lstm_input_dim == 3 * 48 and m.layout["blstm_forward.W"][1] == (144, 32)


def test_crnn_rejects_small_inputs_and_bf16():
    from lidbox_amd.models import crnn
    with pytest.raises(ValueError):
        crnn.create((31, 40), 10, device="cpu")
    with pytest.raises(ValueError):
        crnn.create((40, 31), 10, device="cpu")
    with pytest.raises(ValueError):
        crnn.create((40, 40), 10, device="cpu", compute_dtype="bfloat16")
    crnn.create((32, 32), 10, device="cpu")


def test_crnn_parameter_counts_and_layouts():
    from lidbox_amd.models import crnn
    m = crnn.create((198, 40), 10, device="cpu", seed=0)
    assert m.count_params() == 1458890                         # Keras' count_params() of the reference model
    assert m.output_activation == "softmax" and m.output_dim == 10
    cin = 1
    for i, (f, k) in enumerate(zip((16, 32, 64, 128, 256), (7, 5, 3, 3, 3)), start=1):
        assert m.layout["conv_%d.W" % i][1] == (k, k, cin, f) and m.layout["conv_%d.b" % i][1] == (f,)
        assert m.layout["conv_%d_bn.gamma" % i][1] == (f,)
        assert m.state_layout["conv_%d_bn.moving_variance" % i][1] == (f,)
        cin = f
    for half in ("blstm_forward", "blstm_backward"):
        assert m.layout[half + ".W"][1] == (256, 1024) and m.layout[half + ".U"][1] == (256, 1024)
        assert m.layout[half + ".b"][1] == (1024,)
    assert m.layout["output.W"][1] == (512, 10)
    assert all(off % 4 == 0 for off, _ in list(m.layout.values()) + list(m.state_layout.values()))
    assert m.regularizers == [("conv_%d.W" % i, 0.001) for i in range(1, 6)]
    assert not m.convs and not m.fused_output_ok()
    assert crnn.create((198, 40), 10, device="cpu", weight_decay=0).regularizers == []


def test_crnn_keras_initialisation_rules():
    from lidbox_amd.models import crnn
    m = crnn.create((40, 40), 4, device="cpu", seed=3, filters=(16, 16, 32, 32, 16), num_units=8)
    w = m.get_weights()
    for i, k in enumerate((7, 5, 3, 3, 3), start=1):
        W = w["conv_%d.W" % i]
        lim = np.sqrt(6.0 / (k * k * W.shape[2] + k * k * W.shape[3]))
        assert np.abs(W).max() <= lim and np.abs(W).max() > 0.9 * lim
        assert not w["conv_%d.b" % i].any()
        assert (w["conv_%d_bn.gamma" % i] == 1).all() and (w["conv_%d_bn.moving_variance" % i] == 1).all()
    for half in ("blstm_forward", "blstm_backward"):
        U = w[half + ".U"].astype(np.float64)
        assert np.allclose(U @ U.T, np.eye(8), atol=1e-5)           # orthogonal: orthonormal rows
        b = w[half + ".b"]
        assert (b[8:16] == 1).all() and not b[:8].any() and not b[16:].any()
    assert crnn.loader is crnn.create


def test_hdf5_blstm_names():
    from lidbox_amd.models.hdf5_reader import keras_param_name
    assert keras_param_name("blstm/forward_lstm_3/lstm_cell_10/kernel:0", "blstm") == "blstm_forward.W"
    assert keras_param_name("blstm/backward_lstm/lstm_cell_1/recurrent_kernel:0", "blstm") == "blstm_backward.U"
    assert keras_param_name("blstm/backward_lstm_2/bias:0", "blstm") == "blstm_backward.b"
    assert keras_param_name("conv_3/kernel:0", "conv_3") == "conv_3.W"
    # the names ap_lstm and lstm use are unchanged
    assert keras_param_name("blstm_1/forward_lstm_1/lstm_cell_1/kernel:0", "blstm_1") == "forward_lstm_1.W"
    assert keras_param_name("blstm_2/backward_lstm_2/lstm_cell_5/recurrent_kernel:0", "blstm_2") == "backward_lstm_2.U"
    assert keras_param_name("lstm/lstm_cell/kernel:0", "lstm") == "lstm.W"


def test_hdf5_crnn_fixture_reads_into_model_layout():
    from lidbox_amd.models import crnn
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_crnn_h5 import CRNN_LAYERS, FILTERS, F, H, N, T, expected_name
    from make_keras_h5 import values
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_crnn_weights.h5"))
    want = {expected_name(wname): values(wname, shape) for _, vars_ in CRNN_LAYERS for wname, shape in vars_}
    assert sorted(w) == sorted(want)
    for k in want:
        assert np.array_equal(w[k], want[k]), k
    assert w["conv_1.W"].shape == (7, 7, 1, FILTERS) and w["conv_2.W"].shape == (5, 5, FILTERS, FILTERS)
    m = crnn.create((T, F), N, device="cpu", seed=0, filters=(FILTERS,) * 5, num_units=H)
    layout = dict(list(m.layout.items()) + list(m.state_layout.items()))
    assert sorted(layout) == sorted(w)
    for n, (_, shape) in layout.items():
        assert w[n].shape == tuple(shape), n


def test_native_conv2d_argument_checks():
    from lidbox_amd import _native as nv
    assert nv.lib.lidbox_conv2d_dgrad_workspace(3, 32, 64) == 9 * 32 * 64 * 4
    assert nv.lib.lidbox_conv2d_wgrad_workspace(4, 40, 40, 16, 15, 3) == 0              # C_out not a multiple of 16
    assert nv.lib.lidbox_conv2d_wgrad_workspace(4, 40, 40, 16, 32, 3) > 0
    assert nv.lib.lidbox_conv2d_fwd(None, 1, 8, 8, 1, None, 3, 16, None, 1, None, None) == -1
    assert nv.lib.lidbox_conv2d_fwd(None, 1, 8, 8, 1, None, 4, 16, None, 1, None, None) == -1   # even k
    assert nv.lib.lidbox_conv2d_dgrad(None, 1, 8, 8, 8, 16, None, 3, None, None, 0, None) == -1  # C_in % 16
    assert nv.lib.lidbox_bn_maxpool2d_fwd(None, 1, 1, 8, 16, None, None, None, None, None) == -1
    assert nv.lib.lidbox_maxpool2d_bwd(None, None, 1, 8, 8, 16, None, None) == -1
    assert nv.lib.lidbox_l2_penalty(None, None, 0, None, None, None, 1.0, None, None, 0, None) == -1
    assert nv.lib.lidbox_l2_penalty_workspace() > 0
