"""
Writes the Keras-layout HDF5 fixture of the bi_gru model (tests/test_gru_gpu.py, tests/test_gru_cpu.py) with h5py, in the
layout make_keras_h5.py documents.  Run with an interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_keras_bi_gru_h5.py

bi_gru with C = 5 input channels, GRU units H = 3, Dense units F = 4 and N = 2 outputs.  Bidirectional halves are stored
under the wrapper's group with the GRU cell scope and deliberately non-default, session-numbered inner names
("BGRU_1/forward_gru_7/gru_cell_22/kernel:0"): the reader must map them by wrapper and direction.  The values are
make_keras_h5.values (an exact integer hash of the name), so the tests regenerate them without h5py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_keras_h5 import save_weights_to_group, values  # noqa: E402,F401

C, H, F, N = 5, 3, 4, 2


def _gru_vars(wrapper, half, cell, cin):
    p = "%s/%s/%s/" % (wrapper, half, cell)
    return [(p + "kernel:0", (cin, 3 * H)), (p + "recurrent_kernel:0", (H, 3 * H)), (p + "bias:0", (2, 3 * H))]


def _bn_vars(name, c):
    return [("%s/%s:0" % (name, v), (c,)) for v in ("gamma", "beta", "moving_mean", "moving_variance")]


def _dense_vars(name, cin, cout):
    return [(name + "/kernel:0", (cin, cout)), (name + "/bias:0", (cout,))]


BI_GRU_LAYERS = [
    ("input", []),
    ("BGRU_1", _gru_vars("BGRU_1", "forward_gru_7", "gru_cell_22", C) + _gru_vars("BGRU_1", "backward_gru_7", "gru_cell_23", C)),
    ("BGRU_2", _gru_vars("BGRU_2", "forward_gru_8", "gru_cell_25", 2 * H)
     + _gru_vars("BGRU_2", "backward_gru_8", "gru_cell_26", 2 * H)),
    ("BGRU_2_bn", _bn_vars("BGRU_2_bn", 2 * H)),
    ("fc_relu_1", _dense_vars("fc_relu_1", 2 * H, F)),
    ("fc_relu_1_bn", _bn_vars("fc_relu_1_bn", F)),
    ("fc_relu_2", _dense_vars("fc_relu_2", F, F)),
    ("fc_relu_2_bn", _bn_vars("fc_relu_2_bn", F)),
    ("output", _dense_vars("output", F, N)),
    ("log_softmax", []),
]

# this build's parameter name of every variable above
EXPECTED_NAMES = {
    "BGRU_1/forward_gru_7/gru_cell_22/": "BGRU_1_forward", "BGRU_1/backward_gru_7/gru_cell_23/": "BGRU_1_backward",
    "BGRU_2/forward_gru_8/gru_cell_25/": "BGRU_2_forward", "BGRU_2/backward_gru_8/gru_cell_26/": "BGRU_2_backward",
}


def expected_name(wname):
    prefix, var = wname.rsplit("/", 1)
    var = var.split(":")[0]
    suffix = {"kernel": ".W", "recurrent_kernel": ".U", "bias": ".b"}.get(var, "." + var)
    return EXPECTED_NAMES.get(prefix + "/", prefix) + suffix


def main():
    import h5py
    path = os.path.join(HERE, "keras_bi_gru_weights.h5")
    with h5py.File(path, "w") as f:
        save_weights_to_group(f, BI_GRU_LAYERS)
    print("h5py", h5py.__version__, "->", path)


if __name__ == "__main__":
    sys.exit(main())
