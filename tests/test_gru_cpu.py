"""
Host-only tests of the bi_gru model (lidbox_amd.models.bi_gru / gru_rnn) and of the HDF5 reader's GRU names: parameter
names, layouts and counts as Keras reports them, the Keras initialisation rules and the native GRU entry points' argument
checks.  Models are built on the CPU device: nothing here launches a kernel.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_hdf5_gru_names():
    from lidbox_amd.models.hdf5_reader import keras_param_name
    assert keras_param_name("BGRU_1/forward_gru_7/gru_cell_22/kernel:0", "BGRU_1") == "BGRU_1_forward.W"
    assert keras_param_name("BGRU_2/backward_gru/gru_cell_5/recurrent_kernel:0", "BGRU_2") == "BGRU_2_backward.U"
    assert keras_param_name("BGRU_2/backward_gru_3/bias:0", "BGRU_2") == "BGRU_2_backward.b"          # no cell scope
    assert keras_param_name("gru/gru_cell/kernel:0", "gru") == "gru.W"
    assert keras_param_name("BGRU_2_bn/moving_variance:0", "BGRU_2_bn") == "BGRU_2_bn.moving_variance"
    assert keras_param_name("fc_relu_1/kernel:0", "fc_relu_1") == "fc_relu_1.W"
    # LSTM names are unchanged
    assert keras_param_name("blstm_1/forward_lstm_1/lstm_cell_1/kernel:0", "blstm_1") == "forward_lstm_1.W"


def test_hdf5_bi_gru_fixture_reads():
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_bi_gru_h5 import BI_GRU_LAYERS, C, H, expected_name
    from make_keras_h5 import values
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_bi_gru_weights.h5"))
    want = {expected_name(wname): values(wname, shape) for _, vars_ in BI_GRU_LAYERS for wname, shape in vars_}
    assert sorted(w) == sorted(want)
    for k in want:
        assert np.array_equal(w[k], want[k]), k
    assert w["BGRU_1_forward.W"].shape == (C, 3 * H) and w["BGRU_2_backward.W"].shape == (2 * H, 3 * H)
    assert w["BGRU_1_backward.b"].shape == (2, 3 * H)


def test_bi_gru_fixture_names_match_model_layout():
    from lidbox_amd.models import bi_gru
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_bi_gru_h5 import C, F, H, N
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_bi_gru_weights.h5"))
    m = bi_gru.create((20, C), N, device="cpu", seed=0, num_units=H, num_fc_units=F)
    want = dict(list(m.layout.items()) + list(m.state_layout.items()))
    assert sorted(want) == sorted(w)
    for n, (_, shape) in want.items():
        assert w[n].shape == tuple(shape), n


def test_bi_gru_parameter_counts_and_layouts():
    from lidbox_amd.models import bi_gru
    C, N, H, F = 40, 10, 512, 1024
    m = bi_gru.create((198, C), N, device="cpu", seed=0)
    gru1 = 2 * 3 * H * (C + H + 2)
    gru2 = 2 * 3 * H * (2 * H + H + 2)
    dense = (2 * H * F + F) + (F * F + F) + (F * N + N)
    bn = 4 * (2 * H) + 4 * F + 4 * F
    assert m.count_params() == gru1 + gru2 + dense + bn == 8548362
    assert m.output_dim == N and m.output_activation == "log_softmax"
    halves = ["BGRU_%d_%s.%s" % (i, d, v) for i in (1, 2) for d in ("forward", "backward") for v in "WUb"]
    assert list(m.layout)[:12] == halves
    assert m.layout["BGRU_1_forward.W"][1] == (C, 3 * H) and m.layout["BGRU_2_backward.W"][1] == (2 * H, 3 * H)
    assert m.layout["BGRU_2_forward.U"][1] == (H, 3 * H) and m.layout["BGRU_1_backward.b"][1] == (2, 3 * H)
    assert m.layout["fc_relu_1.W"][1] == (2 * H, F) and m.layout["output.W"][1] == (F, N)
    assert list(m.state_layout) == ["%s.%s" % (b, s) for b in ("BGRU_2_bn", "fc_relu_1_bn", "fc_relu_2_bn")
                                    for s in ("moving_mean", "moving_variance")]
    assert all(off % 4 == 0 for off, _ in list(m.layout.values()) + list(m.state_layout.values()))
    assert not m.convs and not m.fused_output_ok()
    with pytest.raises(ValueError):
        bi_gru.create((198, C), N, device="cpu", compute_dtype="bfloat16")


def test_bi_gru_keras_initialisation_rules():
    from lidbox_amd.models import bi_gru
    H = 30
    m = bi_gru.create((50, 20), 4, device="cpu", seed=7, num_units=H, num_fc_units=16)
    w = m.get_weights()
    for half in ("BGRU_1_forward", "BGRU_2_backward"):
        U = w[half + ".U"].astype(np.float64)
        assert np.allclose(U @ U.T, np.eye(H), atol=1e-5)                   # orthogonal: orthonormal rows
        assert not w[half + ".b"].any()
        W = w[half + ".W"]
        lim = np.sqrt(6.0 / (W.shape[0] + W.shape[1]))
        assert np.abs(W).max() <= lim and np.abs(W).max() > 0.9 * lim       # glorot_uniform
    for bn in ("BGRU_2_bn", "fc_relu_1_bn", "fc_relu_2_bn"):
        assert (w[bn + ".gamma"] == 1).all() and not w[bn + ".beta"].any()
        assert not w[bn + ".moving_mean"].any() and (w[bn + ".moving_variance"] == 1).all()
    w2 = bi_gru.create((50, 20), 4, device="cpu", seed=7, num_units=H, num_fc_units=16).get_weights()
    assert all(np.array_equal(w[k], w2[k]) for k in w)


def test_bi_gru_module_interface():
    from lidbox_amd.models import bi_gru
    assert bi_gru.loader is bi_gru.create
    m = bi_gru.loader((50, 20), 3, device="cpu", seed=0, num_units=8, num_fc_units=8)
    assert callable(bi_gru.as_embedding_extractor(m))


def test_native_gru_queries():
    from lidbox_amd import _native as nv
    assert nv.lib.lidbox_gru_workspace(256, 198, 512, 2) == 2 * 256 * 512 * 4
    assert nv.lib.lidbox_gru_workspace(0, 198, 512, 2) == 0
    assert nv.lib.lidbox_gru_fwd(None, None, None, None, 1, 4, 10, 8, None, None, None, None, None) == -1
    assert nv.lib.lidbox_gru_fwd(None, None, None, None, 3, 4, 10, 8, None, None, None, None, None) == -1
    assert nv.lib.lidbox_gru_bwd(None, None, 1, 4, 10, 8, None, None, None, None, 0, None, None, 0, None) == -1
