"""
BLSTM language-vector extractor of Gelly & Gauvain (2017) for the angular-proximity loss (reference
lidbox/models/ap_lstm.py:23-44): [SpatialDropout1D] -> Bidirectional(LSTM) `blstm_1` -> Bidirectional(LSTM) `blstm_2`, both
returning sequences -> alpha-weighted concatenation -> GlobalAveragePooling1D -> tf.math.l2_normalize.  The output has
4 * num_lstm_units dimensions and no output activation; calling the model returns the L2-normalised vector.
"""
from .rnn import LSTMSpec, RecurrentModel


def create(input_shape, num_lstm_units=62, alpha1=1.0, alpha2=1.0, channel_dropout_rate=0, seed=None, device=None,
           compute_dtype="float32"):
    lstms = [LSTMSpec("lstm_1", num_lstm_units, bidirectional=True, wrapper="blstm_1"),
             LSTMSpec("lstm_2", num_lstm_units, bidirectional=True, wrapper="blstm_2")]
    return RecurrentModel(input_shape, lstms, "avg_concat", name="angular_proximity_lstm", output_activation=None,
                          channel_dropout_rate=channel_dropout_rate, alphas=[alpha1, alpha2], seed=seed, device=device,
                          compute_dtype=compute_dtype)


def loader(input_shape, num_outputs, **kwargs):
    """what lidbox/models/keras_utils.py:134 calls: the output width is 4 * num_lstm_units, not num_outputs; the
    angular-proximity loss needs it to be at least the number of classes"""
    units = int(kwargs.get("num_lstm_units", 62))
    if 4 * units < int(num_outputs):
        raise ValueError("ap_lstm: the language vector has 4 * num_lstm_units = %d dimensions, fewer than the %d classes "
                         "the angular-proximity loss needs" % (4 * units, int(num_outputs)))
    return create(input_shape, **kwargs)
