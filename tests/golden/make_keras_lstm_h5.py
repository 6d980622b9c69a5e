"""
Writes the Keras-layout HDF5 fixture of the recurrent models (tests/test_rnn_gpu.py, tests/test_rnn_cpu.py) with h5py, in
the layout make_keras_h5.py documents.  Run with an interpreter that has h5py:

    /opt/conda/bin/python3.9 tests/golden/make_keras_lstm_h5.py

ap_lstm with C = 6 input channels and num_lstm_units = 3.  Bidirectional halves are stored under the wrapper's group with
the LSTM cell scope, "blstm_1/forward_lstm_1/lstm_cell_1/kernel:0"; the values are make_keras_h5.values (an exact integer
hash of the name), so the test regenerates them without h5py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_keras_h5 import save_weights_to_group, values  # noqa: E402

C, H = 6, 3


def _lstm_vars(wrapper, half, cell, cin):
    p = "%s/%s/%s/" % (wrapper, half, cell)
    return [(p + "kernel:0", (cin, 4 * H)), (p + "recurrent_kernel:0", (H, 4 * H)), (p + "bias:0", (4 * H,))]


AP_LSTM_LAYERS = [
    ("input", []),
    ("blstm_1", _lstm_vars("blstm_1", "forward_lstm_1", "lstm_cell_1", C) + _lstm_vars("blstm_1", "backward_lstm_1", "lstm_cell_2", C)),
    ("blstm_2", _lstm_vars("blstm_2", "forward_lstm_2", "lstm_cell_4", 2 * H) + _lstm_vars("blstm_2", "backward_lstm_2", "lstm_cell_5", 2 * H)),
    ("alpha1", []),
    ("alpha2", []),
    ("blstm_concat", []),
    ("avg_over_time", []),
]


def main():
    import h5py
    with h5py.File(os.path.join(HERE, "keras_ap_lstm_weights.h5"), "w") as f:
        save_weights_to_group(f, AP_LSTM_LAYERS)
    print("h5py", h5py.__version__, "->", os.path.join(HERE, "keras_ap_lstm_weights.h5"))


if __name__ == "__main__":
    sys.exit(main())
