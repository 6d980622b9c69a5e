"""
CRNN of Bartz et al. (2017), reference lidbox/models/crnn.py:24-52: the input [B, T, F] as an image (height = frequency, width =
time) -> five blocks Conv2D(f, k, relu, padding="same", l2(weight_decay)) `conv_i` -> BatchNormalization `conv_i_bn` ->
MaxPool2D(2), filters (16, 32, 64, 128, 256), kernels (7, 5, 3, 3, 3) -> time-major [B, T5, F5 * 256] ->
Bidirectional(LSTM(256)) `blstm` (final states, forward t = T5-1 and backward t = 0 concatenated) -> Dense(num_outputs)
`output` -> output activation (softmax by default).  Built on the engine of `lidbox_amd.models.conv_rnn`.
"""
from .conv_rnn import Conv2DSpec, ConvRecurrentModel

FILTERS = (16, 32, 64, 128, 256)
KERNELS = (7, 5, 3, 3, 3)
MIN_SIZE = 32           # five poolings must leave at least one cell (the reference's tests/test_models.py draws T, F >= 32)


def create(input_shape, num_outputs, output_activation="softmax", weight_decay=0.001, seed=None, device=None,
           compute_dtype="float32", filters=FILTERS, num_units=256):
    """input_shape (T, F).  output_activation: "softmax" (the reference's default), "log_softmax" or None (logits).
    filters / num_units: the reference's fixed widths by default (multiples of 16); smaller values serve tests."""
    if compute_dtype not in ("float32", "fp32", "f32"):
        raise ValueError("crnn computes in float32 only, got compute_dtype=%r" % (compute_dtype,))
    T, F = (None if s is None else int(s) for s in input_shape)
    if (T is not None and T < MIN_SIZE) or F is None or F < MIN_SIZE:
        raise ValueError("crnn needs at least %d frames and %d frequency bins (five 2 x 2 poolings), got %r"
                         % (MIN_SIZE, MIN_SIZE, tuple(input_shape)))
    if len(filters) != len(KERNELS):
        raise ValueError("filters: one width per block (%d)" % len(KERNELS))
    convs = [Conv2DSpec("conv_%d" % i, f, k, weight_decay=weight_decay) for i, (f, k) in enumerate(zip(filters, KERNELS), start=1)]
    return ConvRecurrentModel((T, F), convs, num_units, num_outputs, name="CRNN", output_activation=output_activation or None,
                              seed=seed, device=device, compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`
