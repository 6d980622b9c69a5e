"""
Writes the Keras-layout HDF5 fixture of the crnn model (tests/test_crnn_gpu.py, tests/test_crnn_cpu.py) with h5py, in the
layout make_keras_h5.py documents.  Run with an interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_keras_crnn_h5.py

crnn with input (T, F) = (32, 32), FILTERS = 16 in every block (kernels 7, 5, 3, 3, 3), BLSTM units H = 4 and N = 3 outputs.
Conv2D kernels are [k, k, C_in, C_out].  The Bidirectional LSTM halves are stored under the wrapper's group "blstm" with the
LSTM cell scope and deliberately non-default, session-numbered inner names ("blstm/forward_lstm_3/lstm_cell_10/kernel:0"):
the reader must map them by wrapper and direction.  The values are make_keras_h5.values (an exact integer hash of the name),
so the tests regenerate them without h5py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_keras_h5 import save_weights_to_group, values  # noqa: E402,F401

T, F, FILTERS, H, N = 32, 32, 16, 4, 3
KERNELS = (7, 5, 3, 3, 3)
D = 1 * FILTERS                        # F5 * C: 32 frequency bins pool down to 1


def _conv_vars(name, k, cin, cout):
    return [(name + "/kernel:0", (k, k, cin, cout)), (name + "/bias:0", (cout,))]


def _bn_vars(name, c):
    return [("%s/%s:0" % (name, v), (c,)) for v in ("gamma", "beta", "moving_mean", "moving_variance")]


def _lstm_vars(wrapper, half, cell, cin):
    p = "%s/%s/%s/" % (wrapper, half, cell)
    return [(p + "kernel:0", (cin, 4 * H)), (p + "recurrent_kernel:0", (H, 4 * H)), (p + "bias:0", (4 * H,))]


CRNN_LAYERS = [("input", []), ("expand_channel_dim", []), ("freq_bins_first", [])]
for _i, _k in enumerate(KERNELS, start=1):
    CRNN_LAYERS += [("conv_%d" % _i, _conv_vars("conv_%d" % _i, _k, 1 if _i == 1 else FILTERS, FILTERS)),
                    ("conv_%d_bn" % _i, _bn_vars("conv_%d_bn" % _i, FILTERS)), ("conv_%d_pool" % _i, [])]
CRNN_LAYERS += [
    ("timesteps_first", []), ("flatten_channels", []),
    ("blstm", _lstm_vars("blstm", "forward_lstm_3", "lstm_cell_10", D) + _lstm_vars("blstm", "backward_lstm_3", "lstm_cell_11", D)),
    ("output", [("output/kernel:0", (2 * H, N)), ("output/bias:0", (N,))]),
    ("softmax", []),
]

# this build's parameter name of every variable above
EXPECTED_NAMES = {"blstm/forward_lstm_3/lstm_cell_10/": "blstm_forward", "blstm/backward_lstm_3/lstm_cell_11/": "blstm_backward"}


def expected_name(wname):
    prefix, var = wname.rsplit("/", 1)
    var = var.split(":")[0]
    suffix = {"kernel": ".W", "recurrent_kernel": ".U", "bias": ".b"}.get(var, "." + var)
    return EXPECTED_NAMES.get(prefix + "/", prefix) + suffix


def main():
    import h5py
    path = os.path.join(HERE, "keras_crnn_weights.h5")
    with h5py.File(path, "w") as f:
        save_weights_to_group(f, CRNN_LAYERS)
    print("h5py", h5py.__version__, "->", path)


if __name__ == "__main__":
    sys.exit(main())
