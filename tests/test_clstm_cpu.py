"""
Host-only tests of the clstm model (lidbox_amd.models.clstm): TF "same" padding sizes and pads of the Conv2D front-end, the
frame layers' time steps, parameter names, shapes and counts as Keras reports them, the argument checks of create() and of the
new native entry points (which return before any launch), and the HDF5 fixture read into the model's layout.  Nothing here
needs a GPU.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_same_padding_sizes_and_pads():
    from lidbox_amd.models import clstm
    assert clstm.same_padding(198, 3, 1) == (198, 1, 1)
    assert clstm.conv2d_frequency_sizes(40) == [(40, 7, 2, 3), (7, 2, 4, 4)]
    assert [s[:2] for s in clstm.conv2d_frequency_sizes(64)] == [(64, 11), (11, 2)]
    assert [s[:2] for s in clstm.conv2d_frequency_sizes(20)] == [(20, 4), (4, 1)]
    for F in range(1, 7):
        assert [s[:2] for s in clstm.conv2d_frequency_sizes(F)] == [(F, 1), (1, 1)]


def test_frame_time_steps():
    from lidbox_amd.models.tdnn import ConvSpec
    from lidbox_amd.models import clstm
    for T, want in ((198, [198, 99, 33]), (6, [6, 3, 1]), (20, [20, 10, 4])):
        Ts = [T]
        for i, (k, s) in enumerate(clstm.FRAME_KERNELS[:3]):
            Ts.append(ConvSpec("f", 8, k, s).geometry(Ts[-1])[2])
        assert Ts[1:] == want


@pytest.mark.parametrize("flags,count", [({}, 4513254), (dict(use_conv2d=True), 5956326), (dict(use_lstm=True), 6612454),
                                         (dict(use_attention=True), 4613094),
                                         (dict(use_conv2d=True, use_lstm=True, use_attention=True), 8155366)])
def test_parameter_counts(flags, count):
    from lidbox_amd.models import clstm
    assert clstm.count_params((198, 40), 10, **flags) == count


def test_parameter_names_shapes_and_order():
    from lidbox_amd.models import clstm
    lay = clstm.keras_layout((None, 40), 10, use_attention=True, use_conv2d=True, use_lstm=True)
    shapes = {n: s for n, s, _ in lay}
    assert shapes["conv2d_1.W"] == (3, 9, 1, 128) and shapes["conv2d_2.W"] == (3, 9, 128, 256)
    assert shapes["conv2d_2_bn.moving_variance"] == (256,)
    assert shapes["frame1.W"] == (5, 256, 512) and shapes["frame5.W"] == (1, 512, 1500)
    assert shapes["lstm.W"] == (512, 2048) and shapes["lstm.U"] == (512, 2048) and shapes["lstm.b"] == (2048,)
    assert shapes["Wf_1.W"] == (1500, 64) and shapes["Wf_2.W"] == (64, 60)
    assert shapes["segment1.W"] == (3000, 512) and shapes["output.W"] == (512, 10)
    names = [n for n, _, t in lay if t]
    # the bucket-safe order: front-end lowest, the LSTM between frame3 and frame4
    assert names.index("conv2d_2_bn.beta") < names.index("frame1.W")
    assert names.index("frame3.b") < names.index("lstm.W") < names.index("lstm.b") < names.index("frame4.W")
    assert not [n for n, _, t in lay if not t and not n.endswith(("moving_mean", "moving_variance"))]
    assert shapes == {n: s for n, s, _ in clstm.keras_layout((198, 40), 10, True, True, True)}


def test_create_rejects_bf16_and_bad_attention_bins():
    from lidbox_amd.models import clstm
    with pytest.raises(ValueError):
        clstm.create((198, 40), 10, compute_dtype="bfloat16", device="cpu")
    with pytest.raises(ValueError, match="d_f=60"):
        clstm.create((198, 40), 10, use_attention=True, frame_units=(512, 512, 512, 512, 1000), device="cpu")
    with pytest.raises(ValueError):
        clstm.create((198, None), 10, device="cpu")


def test_native_argument_checks():
    from lidbox_amd import _native as nv
    lib = nv.lib
    good = nv.Conv2DTaps(3, 9, 6, 1, 1, 2, 3, 1)
    assert lib.lidbox_conv2d_strided_dgrad_workspace(good, 128, 256) == 3 * 9 * 128 * 256 * 4
    assert lib.lidbox_conv2d_strided_wgrad_workspace(4, 10, 40, 1, 128, good) > 0
    assert lib.lidbox_conv2d_strided_wgrad_workspace(4, 10, 40, 1, 100, good) == 0
    x = 16                                                     # never dereferenced: the checks return first
    for taps, cout in ((good, 100), (nv.Conv2DTaps(3, 9, 0, 1, 1, 2, 3, 1), 128), (nv.Conv2DTaps(3, 9, 6, 3, 1, 2, 3, 1), 128),
                       (nv.Conv2DTaps(3, 9, 6, 1, 1, -1, 3, 1), 128)):
        assert lib.lidbox_conv2d_strided_fwd(x, 2, 10, 40, 1, x, taps, cout, None, x, None) == -1
    assert lib.lidbox_conv2d_strided_fwd(None, 2, 10, 40, 1, x, good, 128, None, x, None) == -1
    assert lib.lidbox_conv2d_strided_dgrad(x, 2, 10, 40, 8, 128, x, good, x, x, 1 << 30, None) == -1     # C_in % 16
    assert lib.lidbox_conv2d_strided_dgrad(x, 2, 10, 40, 128, 256, x, good, x, None, 0, None) == -1
    assert lib.lidbox_conv2d_strided_wgrad(x, x, 2, 10, 40, 1, 128, good, x, x, None, 0, None) == -1
    assert lib.lidbox_bn_relu_maxf_fwd(x, 2, 10, 2, 16, x, x, x, 10, None) == -1                      # batch stride < T C
    assert lib.lidbox_bn_relu_maxf_bwd(x, 2, 10, 2, 16, x, x, None, 160, x, None) == -1
    assert lib.lidbox_bn_relu_fwd(x, -1, 16, x, x, x, None) == -1
    assert lib.lidbox_bn_relu_bwd(x, 4, 0, x, x, x, x, None) == -1
    assert lib.lidbox_input_noise_dropout(x, 2, 10, 40, 400, 0.01, 1.0, 0, None, None) == -1           # rate < 1
    assert lib.lidbox_input_noise_dropout(x, 2, 10, 40, 399, 0.01, 0.4, 0, None, None) == -1
    assert lib.lidbox_input_noise_dropout(x, 2, 10, 40, 400, -0.01, 0.4, 0, None, None) == -1


def test_hdf5_fixture_in_model_layout():
    from lidbox_amd.models import clstm
    from lidbox_amd.models.hdf5_reader import load_keras_weights
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_keras_clstm_h5 import CLSTM_LAYERS, F, FILTERS, FRAME_UNITS, N, SEGMENT_UNITS, expected_name, values
    w = load_keras_weights(os.path.join(HERE, "golden", "keras_clstm_weights.h5"))
    lay = clstm.keras_layout((None, F), N, True, True, True, FILTERS, FRAME_UNITS, SEGMENT_UNITS)
    assert sorted(w) == sorted(n for n, _, _ in lay)
    for n, shape, _ in lay:
        assert w[n].shape == shape, n
    for _, variables in CLSTM_LAYERS:
        for wname, shape in variables:
            assert np.array_equal(w[expected_name(wname)], values(wname, shape)), wname
    assert os.path.getsize(os.path.join(HERE, "golden", "keras_clstm_weights.h5")) < 200 * 1024
