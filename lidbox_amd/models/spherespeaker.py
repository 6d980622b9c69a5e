"""
SphereSpeaker of Kaseva, Rouhe and Kurimo (2019) with mean pooling, reference lidbox/models/spherespeaker.py:36-54:
Bidirectional(LSTM(250), return_sequences) `blstm_1` -> `blstm_2` -> `blstm_3` -> Concatenate of the three output sequences ->
BatchNormalization `blstm_bn` -> Dense(embedding_dim, relu) `fc_relu` on every frame -> GlobalAveragePooling1D `avg_pooling` ->
BatchNormalization `pool_bn` -> L2 normalisation `l2_normalize` -> Dense(num_outputs) `outputs` -> output activation.

The scaffolding is `lidbox_amd.models.flat`'s; every BLSTM is its lstm_layer_fwd / lstm_layer_bwd on the stepped walk
lidbox_lstm_step_fwd / _bwd (csrc/lstm_step.hip, one launch per step for both directions).

The Concatenate is free: the three layers write their output sequences into column slices 0, 2H and 4H of one
[B, T+2, 6H] buffer (rows 0 and T+1 of every utterance stay zero, as the LSTM calls want), layer i+1 reads layer i's slice
through a rows descriptor with row stride 6H, and backward keeps one [B, T, 6H] gradient buffer: `blstm_bn`'s backward
fills all of it, then layer i+1's dX accumulates into layer i's slice.

`blstm_bn` sees a 3-D input, which tf.keras normalises on its non-fused path like the 2-D `pool_bn`: batch mean and
population variance over the B*T (or B) rows, the moving variance moved towards the population variance
(lidbox_bn_train_stats_ex, bessel = 0).  The statistics kernel reads dense rows, so one pitched copy drops the two pad rows
per utterance first.  Moving statistics live in `state` / `state_layout` and move only when `update_moving`.

The LSTM halves are named by wrapper and direction (`blstm_1_forward.W`, `blstm_3_backward.b`), because Keras numbers the
unnamed inner LSTMs per session; the other layers keep their Keras names.
"""
import ctypes

import torch

from .. import _native as nv
from .flat import FlatModel, LSTMLayer, Workspace, _rows, lstm_layer_bwd, lstm_layer_fwd
from .gru_rnn import BatchNormSpec
from .ragged_pass import EmbeddingExtractor
from .rnn_ragged import RaggedRecurrent
from .tdnn import DenseSpec

NUM_BLSTM = 3


class _Workspace(Workspace):
    """All per-(B, T) device buffers of one spherespeaker model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
        lib = nv.lib
        self.B, self.T = B, T
        H, E, N, C6 = model.units, model.embedding_dim, model.output_dim, model.concat_dim
        R = B * T
        self.x = torch.zeros((B, T, model.input_dim), **f32)
        self.hcat = torch.zeros((B, T + 2, C6), **f32)          # the three output sequences side by side; pad rows stay zero
        self.dcat = torch.zeros((B, T, C6), **f32)              # their gradient
        self.zg = [torch.zeros((2, B, T, 4 * H), **f32) for _ in range(NUM_BLSTM)]
        self.cseq = [torch.zeros((2, B, T, H), **f32) for _ in range(NUM_BLSTM)]
        self.xcat = torch.zeros((R, C6), **f32)                 # hcat without its pad rows: blstm_bn's input
        self.ycat = torch.zeros((R, C6), **f32)                 # blstm_bn's output, then the gradient of it
        self.c_cat = torch.zeros((4, C6), **f32)                # mean, invstd, scale, shift
        self.a = torch.zeros((R, E), **f32)                     # fc_relu's output, then the gradient of its pre-activation
        self.da = torch.zeros((R, E), **f32)
        self.pooled = torch.zeros((B, E), **f32)
        self.dpooled = torch.zeros((B, E), **f32)
        self.ypool = torch.zeros((B, E), **f32)
        self.dypool = torch.zeros((B, E), **f32)
        self.c_pool = torch.zeros((4, E), **f32)
        self.emb = torch.zeros((B, E), **f32)                   # the l2_normalize layer's output
        self.demb = torch.zeros((B, E), **f32)
        self.h = [torch.zeros((B, N), **f32)]                   # logits
        self.dh = [torch.zeros((B, N), **f32)]
        self.logp = torch.zeros((B, N), **f32)
        self.loss = torch.zeros(4, **f32)
        gws, tws = 0, 16
        cin = model.input_dim
        for _ in range(NUM_BLSTM):
            gws = max(gws, lib.lidbox_gemm_rows_workspace(R, 4 * H, cin), lib.lidbox_gemm_rows_workspace(R, cin, 4 * H))
            tws = max(tws, lib.lidbox_gemm_tn_workspace(R, cin, 4 * H), lib.lidbox_gemm_tn_workspace(R, H, 4 * H))
            cin = 2 * H
        gws = max(gws, lib.lidbox_gemm_rows_workspace(R, E, C6), lib.lidbox_gemm_rows_workspace(R, C6, E),
                  lib.lidbox_gemm_rows_workspace(B, N, E), lib.lidbox_gemm_rows_workspace(B, E, N))
        tws = max(tws, lib.lidbox_gemm_tn_workspace(R, C6, E), lib.lidbox_gemm_tn_workspace(B, E, N))
        self.lstm_ws = torch.empty(max(16, lib.lidbox_lstm_step_workspace(B, T, H, 2)), dtype=torch.uint8, device=dev)
        self.gemm_ws = torch.empty(max(16, gws), dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.bn_ws = torch.empty(max(16, lib.lidbox_bn_workspace(max(R, 1), C6), lib.lidbox_bn_workspace(max(B, 1), E)),
                                 dtype=torch.uint8, device=dev)
        self.pending = []


class SphereSpeakerModel(FlatModel, RaggedRecurrent):
    """Three stacked BLSTMs -> concat -> BatchNormalization -> Dense(relu) -> time average -> BatchNormalization -> L2
    normalisation -> Dense (see the module docstring)."""

    workspace_class = _Workspace

    # Keras HDF5 files of this model name their LSTM halves by wrapper and direction in every group
    # (lidbox_amd.models.hdf5_reader.keras_param_name)
    keras_blstm_by_wrapper = True

    def __init__(self, input_shape, num_outputs, embedding_dim=1000, num_lstm_units=250, name="spherespeaker",
                 output_activation="log_softmax", seed=None, device=None, compute_dtype="float32"):
        super().__init__(input_shape, name, output_activation, seed, device, compute_dtype)
        self.units, self.embedding_dim = int(num_lstm_units), int(embedding_dim)
        self.concat_dim = 2 * NUM_BLSTM * self.units
        self.output_dim = int(num_outputs)
        self.blstms = ["blstm_%d" % (i + 1) for i in range(NUM_BLSTM)]
        self.cat_bn, self.pool_bn = BatchNormSpec("blstm_bn"), BatchNormSpec("pool_bn")
        self.fc, self.out = DenseSpec("fc_relu", self.embedding_dim, relu=True), DenseSpec("outputs", self.output_dim, relu=False)
        self.denses = [self.fc, self.out]
        H = self.units
        cin = self.input_dim
        for wrapper in self.blstms:
            for p in self.prefixes(wrapper):
                self.add_param(p + ".W", (cin, 4 * H))
                self.add_param(p + ".U", (H, 4 * H))
                self.add_param(p + ".b", (4 * H,))
            cin = 2 * H
        self.add_bn(self.cat_bn.name, self.concat_dim)
        self.add_param("fc_relu.W", (self.concat_dim, self.embedding_dim))
        self.add_param("fc_relu.b", (self.embedding_dim,))
        self.add_bn(self.pool_bn.name, self.embedding_dim)
        self.add_param("outputs.W", (self.embedding_dim, self.output_dim))
        self.add_param("outputs.b", (self.output_dim,))
        self.unit_forget_biases = {p + ".b" for wrapper in self.blstms for p in self.prefixes(wrapper)}
        self._finish(seed)

    @staticmethod
    def prefixes(wrapper):
        return [wrapper + "_forward", wrapper + "_backward"]

    def _slice(self, ws, i, row=1, col=0):
        """address of column `col` of layer i's slice in row `row` of the first utterance of hcat"""
        return ws.hcat.data_ptr() + 4 * (row * self.concat_dim + 2 * self.units * i + col)

    def _in_rows(self, ws, i):
        """(rows descriptor, K) of layer i's input: the model input, or rows 1..T of layer i-1's slice of hcat"""
        B, T = ws.B, ws.T
        if i == 0:
            return _rows(ws.x.data_ptr(), 0, self.input_dim, 1, B * T), self.input_dim
        C6 = self.concat_dim
        return _rows(self._slice(ws, i - 1), (T + 2) * C6, C6, B, T), 2 * self.units

    def _layer(self, ws, i):
        X, K = self._in_rows(ws, i)
        return LSTMLayer(self.prefixes(self.blstms[i]), X, K, ws.B, ws.T, self.units, ws.zg[i], ws.cseq[i], self._slice(ws, i, row=0),
                         self.concat_dim, ws.lstm_ws, ws.gemm_ws, ws.tn_ws, step=True)

    # ------------------------------------------------------------------ forward
    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False, embedding=False):
        """The model input buffer (ws.input_view()) must already hold the input.  training selects batch statistics in the
        BatchNormalization layers (update_moving=False leaves the running statistics untouched).  Returns the log-probs /
        probabilities / logits (output_activation None); stop_before_output or embedding: the l2_normalize layer's output."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        E, C6 = self.embedding_dim, self.concat_dim
        R = B * T
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.emb if (embedding or stop_before_output) else ws.logp
        for i in range(NUM_BLSTM):
            lstm_layer_fwd(self, self._layer(ws, i))
        # blstm_bn on the B*T rows: drop the two pad rows per utterance, then statistics + apply
        nv.check(lib.lidbox_copy_2d(nv.ptr(ws.xcat), 4 * T * C6, ctypes.c_void_p(self._slice(ws, 0)), 4 * (T + 2) * C6,
                                    4 * T * C6, B, st))
        self._bn_fwd(self.cat_bn, ws.xcat, R, C6, ws.c_cat, ws.ycat, ws, training, update_moving)
        nv.check(lib.lidbox_gemm_nn(_rows(ws.ycat.data_ptr(), 0, C6, 1, R), self._p("fc_relu.W"), E,
                                    _rows(ws.a.data_ptr(), 0, E, 1, R), C6, E, nv.EPI_BIAS_RELU, self._p("fc_relu.b"),
                                    gws, gws_n, st))
        nv.check(lib.lidbox_avg_pool_fwd(nv.ptr(ws.a), B, T, E, T * E, E, nv.ptr(ws.pooled), st))
        return self._forward_pooled(ws, training, update_moving, embedding or stop_before_output)

    def _forward_pooled(self, ws, training=False, update_moving=True, embedding=False):
        """`pool_bn` -> L2 normalisation -> `outputs` -> output activation on the ws.B rows of ws.pooled (the dense and the
        ragged pass share it); embedding: the l2_normalize layer's output"""
        st, lib, B = nv.current_stream(), nv.lib, ws.B
        E, N = self.embedding_dim, self.output_dim
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        self._bn_fwd(self.pool_bn, ws.pooled, B, E, ws.c_pool, ws.ypool, ws, training, update_moving)
        nv.check(lib.lidbox_l2_normalize_fwd(nv.ptr(ws.ypool), B, E, nv.ptr(ws.emb), st))
        if embedding:
            return ws.emb
        nv.check(lib.lidbox_gemm_nn(_rows(ws.emb.data_ptr(), 0, E, 1, B), self._p("outputs.W"), N,
                                    _rows(ws.h[-1].data_ptr(), 0, N, 1, B), E, N, nv.EPI_BIAS, self._p("outputs.b"),
                                    gws, gws_n, st))
        return self._output_activation(ws, ws.h[-1], N)

    # ------------------------------------------------------------------ ragged pass (inference, float32; models/rnn_ragged.py)
    def _ragged_embedding_dim(self):
        return self.embedding_dim

    def _ragged_buffers_rows(self, cap):
        """the per-row buffers for `cap` rows (one zg / cseq serves the three layers in turn) and the BatchNormalization constants"""
        f32 = dict(dtype=torch.float32, device=self.device)
        H, E, C6 = self.units, self.embedding_dim, self.concat_dim
        return dict(x=torch.zeros((cap, self.input_dim), **f32), zg=torch.zeros(2 * cap * 4 * H, **f32),
                    cseq=torch.zeros(2 * cap * H, **f32), hcat=torch.zeros((cap, C6), **f32), ycat=torch.zeros((cap, C6), **f32),
                    a=torch.zeros((cap, E), **f32), c_cat=torch.zeros((4, C6), **f32), c_pool=torch.zeros((4, E), **f32))

    def _ragged_buffers_B(self, cap):
        """what _forward_pooled reads of a workspace, for `cap` utterances"""
        f32 = dict(dtype=torch.float32, device=self.device)
        E, N = self.embedding_dim, self.output_dim
        return dict(pooled=torch.zeros((cap, E), **f32), ypool=torch.zeros((cap, E), **f32), emb=torch.zeros((cap, E), **f32),
                    h=[torch.zeros((cap, N), **f32)], logp=torch.zeros((cap, N), **f32))

    def _forward_ragged(self, ws, plan, dev, upto_embedding):
        """the three BLSTMs on the ragged walk into their column slices of hcat [Rp, 6H]; `blstm_bn` and `fc_relu` on all Rp
        rows, in buffers of their own, so that hcat's pad rows stay zero (what they make of a pad row is never read); the
        average over each utterance's own frames; then the shared tail"""
        st, lib, B, Rp = nv.current_stream(), nv.lib, plan.B, plan.Rp
        H, E, N, C6 = self.units, self.embedding_dim, self.output_dim, self.concat_dim
        ws.hcat[:Rp].zero_()                                  # the pad rows: projections, blstm_bn and fc_relu read every row
        X, K = _rows(ws.x.data_ptr(), 0, self.input_dim, 1, Rp), self.input_dim
        for i, wrapper in enumerate(self.blstms):
            h = ws.hcat.data_ptr() + 4 * 2 * H * i
            self._ragged_lstm_layer(ws, plan, dev, X, K, self.prefixes(wrapper), H, h, C6)
            X, K = _rows(h, 0, C6, 1, Rp), 2 * H
        ws.reserve_gemm_ws(self, max(16, lib.lidbox_gemm_rows_workspace(Rp, E, C6), lib.lidbox_gemm_rows_workspace(B, N, E)))
        self._bn_fwd(self.cat_bn, ws.hcat, Rp, C6, ws.c_cat, ws.ycat, ws, False, False)
        nv.check(lib.lidbox_gemm_nn(_rows(ws.ycat.data_ptr(), 0, C6, 1, Rp), self._p("fc_relu.W"), E,
                                    _rows(ws.a.data_ptr(), 0, E, 1, Rp), C6, E, nv.EPI_BIAS_RELU, self._p("fc_relu.b"),
                                    nv.ptr(ws.gemm_ws), ws.gemm_ws.numel(), st))
        nv.check(lib.lidbox_avg_pool_ragged_fwd(nv.ptr(ws.a), E, dev.first, dev.lengths, B, E, nv.ptr(ws.pooled), st))
        return self._forward_pooled(ws, embedding=upto_embedding)

    # ------------------------------------------------------------------ backward

    def backward_head_ws(self, ws):
        """the whole backward pass of a training-mode forward (dh[-1] holds d loss / d logits): the head, then the three
        BLSTM layers from the top down.  Fills flat_grad (overwrites)."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        H, E, N, C6 = self.units, self.embedding_dim, self.output_dim, self.concat_dim
        R = B * T
        ws.pending = []
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        tws, tws_n = nv.ptr(ws.tn_ws), ws.tn_ws.numel()
        if B == 0:
            return
        # outputs
        dy = _rows(ws.dh[-1].data_ptr(), 0, N, 1, B)
        nv.check(lib.lidbox_gemm_tn(_rows(ws.emb.data_ptr(), 0, E, 1, B), dy, self._p("outputs.W", True), N, E, N, 0,
                                    self._p("outputs.b", True), tws, tws_n, st))
        nv.check(lib.lidbox_gemm_nt(dy, self._p("outputs.W"), N, _rows(ws.demb.data_ptr(), 0, E, 1, B), N, E, nv.EPI_NONE, None,
                                    gws, gws_n, st))
        # l2_normalize, pool_bn, avg_pooling (with fc_relu's ReLU mask)
        nv.check(lib.lidbox_l2_normalize_bwd(nv.ptr(ws.ypool), nv.ptr(ws.demb), B, E, nv.ptr(ws.dypool), st))
        self._bn_bwd(self.pool_bn, ws.pooled, B, E, ws.c_pool, ws.dypool, 0, ws.dpooled, ws)
        nv.check(lib.lidbox_avg_pool_bwd(nv.ptr(ws.a), nv.ptr(ws.dpooled), B, T, E, T * E, E, 1, nv.ptr(ws.da), st))
        # fc_relu: da is the gradient of its pre-activation; the gradient of blstm_bn's output overwrites that output
        da = _rows(ws.da.data_ptr(), 0, E, 1, R)
        nv.check(lib.lidbox_gemm_tn(_rows(ws.ycat.data_ptr(), 0, C6, 1, R), da, self._p("fc_relu.W", True), E, C6, E, 0,
                                    self._p("fc_relu.b", True), tws, tws_n, st))
        nv.check(lib.lidbox_gemm_nt(da, self._p("fc_relu.W"), E, _rows(ws.ycat.data_ptr(), 0, C6, 1, R), E, C6, nv.EPI_NONE, None,
                                    gws, gws_n, st))
        # blstm_bn: its input gradient is the gradient of all three output sequences
        self._bn_bwd(self.cat_bn, ws.xcat, R, C6, ws.c_cat, ws.ycat, 0, ws.dcat, ws)
        for i in range(NUM_BLSTM - 1, -1, -1):
            # dX of layer i lands on top of blstm_bn's gradient in layer i-1's slice
            dX = _rows(ws.dcat.data_ptr() + 4 * 2 * H * (i - 1), T * C6, C6, B, T) if i > 0 else None
            lstm_layer_bwd(self, self._layer(ws, i), ctypes.c_void_p(ws.dcat.data_ptr() + 4 * 2 * H * i), T * C6, C6, dX=dX,
                           dX_epi=(nv.EPI_ACCUM, nv.EPI_ACCUM))

    # ------------------------------------------------------------------ public call
    def embed(self, x):
        """inference-mode output of the l2_normalize layer, [B, embedding_dim] (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, False)
            return self.forward_ws(ws, training=False, embedding=True).clone()


def create(input_shape, num_outputs, embedding_dim=1000, output_activation="log_softmax", seed=None, device=None,
           compute_dtype="float32", num_lstm_units=250):
    """output_activation: "log_softmax" (the reference's default), "softmax" or None (logits).  num_lstm_units: the
    reference's fixed width (250) by default; smaller values serve tests."""
    return SphereSpeakerModel(input_shape, num_outputs, embedding_dim=embedding_dim, num_lstm_units=num_lstm_units,
                              output_activation=output_activation or None, seed=seed, device=device,
                              compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`


def as_embedding_extractor(model):
    """reference spherespeaker.py:23-25: the output of the `l2_normalize` layer, in inference mode, [B, embedding_dim]"""
    return EmbeddingExtractor(model)


__all__ = ["SphereSpeakerModel", "EmbeddingExtractor", "create", "loader", "as_embedding_extractor"]
