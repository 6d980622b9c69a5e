"""
Writes the Keras-layout HDF5 fixture of the spherespeaker model (tests/test_spherespeaker_cpu.py,
tests/test_spherespeaker_gpu.py) with h5py, in the layout make_keras_h5.py documents.  Run with an interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_keras_spherespeaker_h5.py

spherespeaker with C = 5 input channels, LSTM units H = 3, embedding_dim E = 4 and N = 2 outputs.  Bidirectional halves are
stored under the wrapper's group with the LSTM cell scope and deliberately non-default, session-numbered inner names
("blstm_2/forward_lstm_7/lstm_cell_22/kernel:0"): the reader must map them by wrapper and direction, also in groups called
"blstm_N" (which, without the reader's `blstm_by_wrapper` argument, keep ap_lstm's inner names).  The values are
make_keras_h5.values (an exact integer hash of the name), so the tests regenerate them without h5py.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_keras_h5 import save_weights_to_group, values  # noqa: E402,F401

C, H, E, N = 5, 3, 4, 2


def _lstm_vars(wrapper, half, cell, cin):
    p = "%s/%s/%s/" % (wrapper, half, cell)
    return [(p + "kernel:0", (cin, 4 * H)), (p + "recurrent_kernel:0", (H, 4 * H)), (p + "bias:0", (4 * H,))]


def _bn_vars(name, c):
    return [("%s/%s:0" % (name, v), (c,)) for v in ("gamma", "beta", "moving_mean", "moving_variance")]


def _dense_vars(name, cin, cout):
    return [(name + "/kernel:0", (cin, cout)), (name + "/bias:0", (cout,))]


# (wrapper, forward half, its cell, backward half, its cell): inner names as a long session numbers them
_HALVES = [("blstm_1", "forward_lstm_6", "lstm_cell_19", "backward_lstm_6", "lstm_cell_20"),
           ("blstm_2", "forward_lstm_7", "lstm_cell_22", "backward_lstm_7", "lstm_cell_23"),
           ("blstm_3", "forward_lstm_8", "lstm_cell_25", "backward_lstm_8", "lstm_cell_26")]

SPHERESPEAKER_LAYERS = [("input", [])] + [
    (w, _lstm_vars(w, f, fc, C if i == 0 else 2 * H) + _lstm_vars(w, b, bc, C if i == 0 else 2 * H))
    for i, (w, f, fc, b, bc) in enumerate(_HALVES)] + [
    ("blstm_concat", []),
    ("blstm_bn", _bn_vars("blstm_bn", 6 * H)),
    ("fc_relu", _dense_vars("fc_relu", 6 * H, E)),
    ("avg_pooling", []),
    ("pool_bn", _bn_vars("pool_bn", E)),
    ("l2_normalize", []),
    ("outputs", _dense_vars("outputs", E, N)),
    ("log_softmax", []),
]

# this build's parameter name of every LSTM variable above
EXPECTED_NAMES = {}
for _w, _f, _fc, _b, _bc in _HALVES:
    EXPECTED_NAMES["%s/%s/%s/" % (_w, _f, _fc)] = _w + "_forward"
    EXPECTED_NAMES["%s/%s/%s/" % (_w, _b, _bc)] = _w + "_backward"


def expected_name(wname):
    prefix, var = wname.rsplit("/", 1)
    var = var.split(":")[0]
    suffix = {"kernel": ".W", "recurrent_kernel": ".U", "bias": ".b"}.get(var, "." + var)
    return EXPECTED_NAMES.get(prefix + "/", prefix) + suffix


def main():
    import h5py
    path = os.path.join(HERE, "keras_spherespeaker_weights.h5")
    with h5py.File(path, "w") as f:
        save_weights_to_group(f, SPHERESPEAKER_LAYERS)
    print("h5py", h5py.__version__, "->", path)


if __name__ == "__main__":
    sys.exit(main())
