"""
Writes the Keras-layout HDF5 fixture of the clstm model (tests/test_clstm_gpu.py, tests/test_clstm_cpu.py) with h5py, in the
layout make_keras_h5.py documents.  Run with an interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_keras_clstm_h5.py

clstm with every switch on (use_conv2d, use_lstm, use_attention), F = 20 frequency bins, Conv2D filters (16, 16), frame widths
(16, 16, 16, 16, 60) (frame5 = d_f, so the attention's 60 bins hold one channel each), segment widths (16, 16) and N = 3 outputs.
Conv2D kernels are [3 (time), 9 (frequency), C_in, C_out]; the LSTM's variables sit under its cell scope, as TF2 writes them
("lstm/lstm_cell/kernel:0").  The values are make_keras_h5.values (an exact integer hash of the name), so the tests regenerate
them without h5py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_keras_h5 import save_weights_to_group, values  # noqa: E402,F401

F, N = 20, 3
FILTERS = (16, 16)
FRAME_UNITS = (16, 16, 16, 16, 60)
SEGMENT_UNITS = (16, 16)
H = FRAME_UNITS[2]


def _vars(name, shapes):
    return [("%s/%s:0" % (name, v), s) for v, s in shapes]


def _bn(name, c):
    return _vars(name, [(v, (c,)) for v in ("gamma", "beta", "moving_mean", "moving_variance")])


CLSTM_LAYERS = [("input", []), ("input_noise", []), ("channel_dropout", []), ("reshape_to_image", [])]
_cin = 1
for _l, _f in enumerate(FILTERS, start=1):
    _n = "conv2d_%d" % _l
    CLSTM_LAYERS += [(_n, _vars(_n, [("kernel", (3, 9, _cin, _f)), ("bias", (_f,))])), (_n + "_bn", _bn(_n + "_bn", _f)),
                     (_n + "_relu", [])]
    _cin = _f
CLSTM_LAYERS += [("tf_op_layer_maxpool_image_channels", [])]
for _i, (_u, _k) in enumerate(zip(FRAME_UNITS, (5, 3, 3, 1, 1)), start=1):
    _n = "frame%d" % _i
    CLSTM_LAYERS += [(_n, _vars(_n, [("kernel", (_k, _cin, _u)), ("bias", (_u,))]))]
    _cin = _u
    if _i == 3:
        CLSTM_LAYERS += [("lstm", _vars("lstm/lstm_cell", [("kernel", (_cin, 4 * H)), ("recurrent_kernel", (H, 4 * H)),
                                                         ("bias", (4 * H,))]))]
CLSTM_LAYERS += [("Wf_1", _vars("Wf_1", [("kernel", (_cin, 64))])), ("Wf_2", _vars("Wf_2", [("kernel", (64, 60))])),
                 ("expand_bin_weight_dim", []), ("partition_freq_bins", []), ("freq_attention", []), ("merge_weighted_bins", []),
                 ("stats_pooling", [])]
_din = 2 * _cin
for _j, _u in enumerate(SEGMENT_UNITS, start=1):
    _n = "segment%d" % _j
    CLSTM_LAYERS += [(_n, _vars(_n, [("kernel", (_din, _u)), ("bias", (_u,))]))]
    _din = _u
CLSTM_LAYERS += [("output", _vars("output", [("kernel", (_din, N)), ("bias", (N,))])), ("log_softmax", [])]


def expected_name(wname):
    prefix, var = wname.rsplit("/", 1)
    var = var.split(":")[0]
    suffix = {"kernel": ".W", "recurrent_kernel": ".U", "bias": ".b"}.get(var, "." + var)
    return prefix.split("/")[0] + suffix


def main():
    import h5py
    path = os.path.join(HERE, "keras_clstm_weights.h5")
    with h5py.File(path, "w") as f:
        save_weights_to_group(f, CLSTM_LAYERS)
    print("h5py", h5py.__version__, "->", path)


if __name__ == "__main__":
    sys.exit(main())
