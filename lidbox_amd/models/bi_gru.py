"""
Bidirectional GRU classifier of Mateju et al. (2018), reference lidbox/models/bi_gru.py:26-48:
[SpatialDropout1D] -> Bidirectional(GRU(512), return_sequences) `BGRU_1` -> Bidirectional(GRU(512)) `BGRU_2` (final states,
forward t = T-1 and backward t = 0 concatenated) -> BatchNormalization `BGRU_2_bn` -> Dense(1024, relu) `fc_relu_1` ->
BatchNormalization -> Dense(1024, relu) `fc_relu_2` -> BatchNormalization -> Dense(num_outputs) `output` -> output activation.
Built on the GRU engine of `lidbox_amd.models.gru_rnn`.
"""
from .gru_rnn import BatchNormSpec, DenseSpec, GRUModel, GRUSpec
from .ragged_pass import EmbeddingExtractor


def create(input_shape, num_outputs, output_activation="log_softmax", channel_dropout_rate=0, seed=None, device=None,
           compute_dtype="float32", num_units=512, num_fc_units=1024):
    """output_activation: "log_softmax" (what the reference's configurations train with), "softmax" or None (logits).
    num_units / num_fc_units: the reference's fixed widths (512, 1024) by default; smaller values serve tests."""
    grus = [GRUSpec("BGRU_1", num_units, bidirectional=True, return_sequences=True),
            GRUSpec("BGRU_2", num_units, bidirectional=True, return_sequences=False)]
    denses = [DenseSpec("fc_relu_1", num_fc_units, relu=True), DenseSpec("fc_relu_2", num_fc_units, relu=True),
              DenseSpec("output", num_outputs, relu=False)]
    bns = [BatchNormSpec("fc_relu_1_bn"), BatchNormSpec("fc_relu_2_bn"), None]
    return GRUModel(input_shape, grus, denses, rnn_bn=BatchNormSpec("BGRU_2_bn"), dense_bns=bns, name="BGRU",
                    output_activation=output_activation or None, channel_dropout_rate=channel_dropout_rate, seed=seed,
                    device=device, compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`


def as_embedding_extractor(model):
    """reference bi_gru.py:20-23: the output of `fc_relu_1` with its activation removed, in inference mode, [B, num_fc_units]"""
    return EmbeddingExtractor(model)
