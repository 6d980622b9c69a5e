"""
Single-layer LSTM classifier (reference lidbox/models/lstm.py:14-20): LSTM(num_units) -> its final h -> Dense(num_outputs)
-> output activation.  Built on the recurrent engine of `lidbox_amd.models.rnn`.
"""
from .rnn import DenseSpec, LSTMSpec, RecurrentModel


def create(input_shape, num_outputs, output_activation="log_softmax", num_units=1024, seed=None, device=None,
           compute_dtype="float32"):
    """output_activation: "log_softmax" (what the reference's configurations train with), "softmax" or None (logits)"""
    return RecurrentModel(input_shape, [LSTMSpec("lstm", num_units, return_sequences=False)], "last",
                          denses=[DenseSpec("output", num_outputs, relu=False)], name="lstm",
                          output_activation=output_activation or None, seed=seed, device=device, compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`
