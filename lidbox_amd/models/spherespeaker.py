"""
SphereSpeaker of Kaseva, Rouhe and Kurimo (2019) with mean pooling, reference lidbox/models/spherespeaker.py:36-54:
Bidirectional(LSTM(250), return_sequences) `blstm_1` -> `blstm_2` -> `blstm_3` -> Concatenate of the three output sequences ->
BatchNormalization `blstm_bn` -> Dense(embedding_dim, relu) `fc_relu` on every frame -> GlobalAveragePooling1D `avg_pooling` ->
BatchNormalization `pool_bn` -> L2 normalisation `l2_normalize` -> Dense(num_outputs) `outputs` -> output activation.

Everything numeric is a liblidbox_hip.so call on preallocated device buffers, so `lidbox_amd.train.Trainer` captures the whole
train step into a hipGraph (one gradient bucket, backward is `backward_head_ws`).  Per BLSTM layer and direction the input
projection X W + b of all B*T rows is one lidbox_gemm_nn; the walk through time is lidbox_lstm_step_fwd / _bwd
(csrc/lstm_step.hip, one launch per step for both directions); dW = X^T dZ (with db), dU = H_prev^T dZ and dX = dZ W^T are
one GEMM each.

The Concatenate is free: the three layers write their output sequences into column slices 0, 2H and 4H of one
[B, T+2, 6H] buffer (rows 0 and T+1 of every utterance stay zero, as the LSTM calls want), layer i+1 reads layer i's slice
through a rows descriptor with row stride 6H, and backward keeps one [B, T, 6H] gradient buffer: `blstm_bn`'s backward
fills all of it, then layer i+1's dX accumulates into layer i's slice.

`blstm_bn` sees a 3-D input, which tf.keras normalises on its non-fused path like the 2-D `pool_bn`: batch mean and
population variance over the B*T (or B) rows, the moving variance moved towards the population variance
(lidbox_bn_train_stats_ex, bessel = 0).  The statistics kernel reads dense rows, so one pitched copy drops the two pad rows
per utterance first.  Moving statistics live in `state` / `state_layout` and move only when `update_moving`.

Parameters live in one flat fp32 buffer in Keras layouts (kernel W [C, 4H], recurrent_kernel U [H, 4H], bias b [4H], gate
order i, f, c, o).  The LSTM halves are named by wrapper and direction (`blstm_1_forward.W`, `blstm_3_backward.b`), because
Keras numbers the unnamed inner LSTMs per session; the other layers keep their Keras names.  Initialisation as Keras:
glorot_uniform kernels, orthogonal recurrent kernels, unit_forget_bias, BatchNormalization 1 / 0 / 0 / 1.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv
from .gru_rnn import BatchNormSpec
from .rnn import RecurrentModel, orthogonal
from .tdnn import DenseSpec, _rows

NUM_BLSTM = 3


def _align4(n):
    return (n + 3) & ~3


class _Workspace:
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

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        return ctypes.c_void_p(self.x.data_ptr()), self.x.stride(0), self.x.shape[1], self.x.shape[2]


class SphereSpeakerModel(RecurrentModel):
    """Three stacked BLSTMs -> concat -> BatchNormalization -> Dense(relu) -> time average -> BatchNormalization -> L2
    normalisation -> Dense.  Shares the public calls of `RecurrentModel` (workspace cache, input loading, __call__); see the
    module docstring."""

    # Keras HDF5 files of this model name their LSTM halves by wrapper and direction in every group
    # (lidbox_amd.models.hdf5_reader.keras_param_name)
    keras_blstm_by_wrapper = True

    def __init__(self, input_shape, num_outputs, embedding_dim=1000, num_lstm_units=250, name="spherespeaker",
                 output_activation="log_softmax", seed=None, device=None, compute_dtype="float32"):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("recurrent models compute in float32 only, got compute_dtype=%r" % (compute_dtype,))
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        self.units, self.embedding_dim = int(num_lstm_units), int(embedding_dim)
        self.concat_dim = 2 * NUM_BLSTM * self.units
        self.output_dim = int(num_outputs)
        self.blstms = ["blstm_%d" % (i + 1) for i in range(NUM_BLSTM)]
        self.cat_bn, self.pool_bn = BatchNormSpec("blstm_bn"), BatchNormSpec("pool_bn")
        self.fc, self.out = DenseSpec("fc_relu", self.embedding_dim, relu=True), DenseSpec("outputs", self.output_dim, relu=False)
        self.denses = [self.fc, self.out]
        self.head = "last"
        self.lstms = []
        self.output_activation = output_activation
        self.channel_dropout_rate = 0.0
        self.dropout_seed = int(np.random.default_rng(seed).integers(1, 2 ** 62))
        self._dropout_calls = 0
        self.compute_dtype = "float32"
        # what lidbox_amd.train.Trainer reads from every model
        self.convs, self.frontend, self.bf16_storage, self.attention = [], None, False, None
        self.wgrad_stream = None
        self.head_wgrad_stream = None
        self.layout, self.state_layout = {}, {}
        off, soff = 0, 0

        def entry(pname, shape):
            nonlocal off
            self.layout[pname] = (off, shape)
            off = _align4(off + int(np.prod(shape)))

        def bn_entries(bn, C):
            nonlocal soff
            for suffix in (".gamma", ".beta"):
                entry(bn.name + suffix, (C,))
            for suffix in (".moving_mean", ".moving_variance"):
                self.state_layout[bn.name + suffix] = (soff, (C,))
                soff = _align4(soff + C)

        H = self.units
        cin = self.input_dim
        for wrapper in self.blstms:
            for p in self.prefixes(wrapper):
                entry(p + ".W", (cin, 4 * H))
                entry(p + ".U", (H, 4 * H))
                entry(p + ".b", (4 * H,))
            cin = 2 * H
        bn_entries(self.cat_bn, self.concat_dim)
        entry("fc_relu.W", (self.concat_dim, self.embedding_dim))
        entry("fc_relu.b", (self.embedding_dim,))
        bn_entries(self.pool_bn, self.embedding_dim)
        entry("outputs.W", (self.embedding_dim, self.output_dim))
        entry("outputs.b", (self.output_dim,))
        self.num_flat = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(max(soff, 4), dtype=torch.float32, device=self.device)
        self._init_weights(seed)
        self._ws = {}

    @staticmethod
    def prefixes(wrapper):
        return [wrapper + "_forward", wrapper + "_backward"]

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        """Keras defaults: glorot_uniform kernels, orthogonal recurrent kernels, zero biases with the LSTM forget gate's
        quarter set to 1 (unit_forget_bias), gamma 1, beta 0, moving mean 0, moving variance 1"""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.num_flat, np.float32)
        for name, (off, shape) in self.layout.items():
            n = int(np.prod(shape))
            if name.endswith(".W"):
                limit = math.sqrt(6.0 / (shape[0] + shape[1]))
                host[off:off + n] = rng.uniform(-limit, limit, size=n).astype(np.float32)
            elif name.endswith(".U"):
                host[off:off + n] = orthogonal(shape, rng).astype(np.float32).ravel()
            elif name.endswith(".gamma"):
                host[off:off + n] = 1.0
            elif name.endswith(".b") and name.startswith("blstm_"):
                host[off + self.units:off + 2 * self.units] = 1.0
        self.flat.copy_(torch.from_numpy(host))
        self.state.zero_()
        for name, (off, shape) in self.state_layout.items():
            if name.endswith(".moving_variance"):
                self.state[off:off + shape[0]] = 1.0

    def param(self, name, grad=False):
        if name in self.state_layout:
            off, shape = self.state_layout[name]
            return self.state[off:off + int(np.prod(shape))].view(shape)
        return super().param(name, grad)

    def count_params(self):
        """Keras `Model.count_params()`: 4H(C + H + 1) per LSTM direction, the Dense layers and 4C per BatchNormalization
        (gamma, beta and the two moving statistics)"""
        return sum(int(np.prod(s)) for _, s in list(self.layout.values()) + list(self.state_layout.values()))

    def get_weights(self):
        """dict name -> numpy array in Keras layouts (trainable parameters and the BatchNormalization moving statistics)"""
        return {n: self.param(n).detach().cpu().numpy().copy() for n in list(self.layout) + list(self.state_layout)}

    def _sp(self, name):
        off, _ = self.state_layout[name]
        return ctypes.c_void_p(self.state.data_ptr() + 4 * off)

    # ------------------------------------------------------------------ workspace
    def workspace(self, B, T):
        key = (int(B), int(T))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.pop(next(iter(self._ws)))
            ws = _Workspace(self, *key)
            self._ws[key] = ws
        return ws

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

    # ------------------------------------------------------------------ forward
    def _bn_fwd(self, bn, x, R, C, consts, y, ws, training, update_moving):
        lib, st = nv.lib, nv.current_stream()
        cp = [ctypes.c_void_p(consts.data_ptr() + 4 * j * C) for j in range(4)]
        if training:
            mm = self._sp(bn.name + ".moving_mean") if update_moving else None
            mv = self._sp(bn.name + ".moving_variance") if update_moving else None
            nv.check(lib.lidbox_bn_train_stats_ex(nv.ptr(x), R, C, self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                  bn.epsilon, bn.momentum, 0, mm, mv, cp[0], cp[1], cp[2], cp[3],
                                                  nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
        else:
            nv.check(lib.lidbox_bn_infer_consts(self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                self._sp(bn.name + ".moving_mean"), self._sp(bn.name + ".moving_variance"),
                                                bn.epsilon, C, cp[2], cp[3], st))
        nv.check(lib.lidbox_bn_apply(nv.ptr(x), R, C, cp[2], cp[3], _rows(y.data_ptr(), 0, C, 1, R), st))

    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False, embedding=False):
        """The model input buffer (ws.input_view()) must already hold the input.  training selects batch statistics in the
        BatchNormalization layers (update_moving=False leaves the running statistics untouched).  Returns the log-probs /
        probabilities / logits (output_activation None); stop_before_output or embedding: the l2_normalize layer's output."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        H, H4, E, N, C6 = self.units, 4 * self.units, self.embedding_dim, self.output_dim, self.concat_dim
        R = B * T
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.emb if (embedding or stop_before_output) else ws.logp
        for i, wrapper in enumerate(self.blstms):
            X, K = self._in_rows(ws, i)
            pf, pb = self.prefixes(wrapper)
            for d, p in enumerate((pf, pb)):
                nv.check(lib.lidbox_gemm_nn(X, self._p(p + ".W"), H4, _rows(ws.zg[i][d].data_ptr(), 0, H4, 1, R), K, H4,
                                            nv.EPI_BIAS, self._p(p + ".b"), gws, gws_n, st))
            nv.check(lib.lidbox_lstm_step_fwd(self._p(pf + ".U"), self._p(pb + ".U"), 2, B, T, H, nv.ptr(ws.zg[i]),
                                              ctypes.c_void_p(self._slice(ws, i, row=0)), C6, nv.ptr(ws.cseq[i]),
                                              nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
        # blstm_bn on the B*T rows: drop the two pad rows per utterance, then statistics + apply
        nv.check(lib.lidbox_copy_2d(nv.ptr(ws.xcat), 4 * T * C6, ctypes.c_void_p(self._slice(ws, 0)), 4 * (T + 2) * C6,
                                    4 * T * C6, B, st))
        self._bn_fwd(self.cat_bn, ws.xcat, R, C6, ws.c_cat, ws.ycat, ws, training, update_moving)
        nv.check(lib.lidbox_gemm_nn(_rows(ws.ycat.data_ptr(), 0, C6, 1, R), self._p("fc_relu.W"), E,
                                    _rows(ws.a.data_ptr(), 0, E, 1, R), C6, E, nv.EPI_BIAS_RELU, self._p("fc_relu.b"),
                                    gws, gws_n, st))
        nv.check(lib.lidbox_avg_pool_fwd(nv.ptr(ws.a), B, T, E, T * E, E, nv.ptr(ws.pooled), st))
        self._bn_fwd(self.pool_bn, ws.pooled, B, E, ws.c_pool, ws.ypool, ws, training, update_moving)
        nv.check(lib.lidbox_l2_normalize_fwd(nv.ptr(ws.ypool), B, E, nv.ptr(ws.emb), st))
        if embedding or stop_before_output:
            return ws.emb
        nv.check(lib.lidbox_gemm_nn(_rows(ws.emb.data_ptr(), 0, E, 1, B), self._p("outputs.W"), N,
                                    _rows(ws.h[-1].data_ptr(), 0, N, 1, B), E, N, nv.EPI_BIAS, self._p("outputs.b"),
                                    gws, gws_n, st))
        if self.output_activation is None:
            return ws.h[-1]
        fn = lib.lidbox_softmax_fwd if self.output_activation == "softmax" else lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(ws.h[-1]), B, N, nv.ptr(ws.logp), st))
        return ws.logp

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, bn, x, R, C, consts, dy, dx, ws):
        nv.check(nv.lib.lidbox_bn_bwd(nv.ptr(x), _rows(dy.data_ptr(), 0, C, 1, R), R, C, ctypes.c_void_p(consts.data_ptr()),
                                      ctypes.c_void_p(consts.data_ptr() + 4 * C), self._p(bn.name + ".gamma"), 0,
                                      self._p(bn.name + ".gamma", True), self._p(bn.name + ".beta", True), nv.ptr(dx),
                                      nv.ptr(ws.bn_ws), ws.bn_ws.numel(), nv.current_stream()))

    def backward_head_ws(self, ws):
        """the whole backward pass of a training-mode forward (dh[-1] holds d loss / d logits): the head, then the three
        BLSTM layers from the top down.  Fills flat_grad (overwrites)."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        H, H4, E, N, C6 = self.units, 4 * self.units, self.embedding_dim, self.output_dim, self.concat_dim
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
        self._bn_bwd(self.pool_bn, ws.pooled, B, E, ws.c_pool, ws.dypool, ws.dpooled, ws)
        nv.check(lib.lidbox_avg_pool_bwd(nv.ptr(ws.a), nv.ptr(ws.dpooled), B, T, E, T * E, E, 1, nv.ptr(ws.da), st))
        # fc_relu: da is the gradient of its pre-activation; the gradient of blstm_bn's output overwrites that output
        da = _rows(ws.da.data_ptr(), 0, E, 1, R)
        nv.check(lib.lidbox_gemm_tn(_rows(ws.ycat.data_ptr(), 0, C6, 1, R), da, self._p("fc_relu.W", True), E, C6, E, 0,
                                    self._p("fc_relu.b", True), tws, tws_n, st))
        nv.check(lib.lidbox_gemm_nt(da, self._p("fc_relu.W"), E, _rows(ws.ycat.data_ptr(), 0, C6, 1, R), E, C6, nv.EPI_NONE, None,
                                    gws, gws_n, st))
        # blstm_bn: its input gradient is the gradient of all three output sequences
        self._bn_bwd(self.cat_bn, ws.xcat, R, C6, ws.c_cat, ws.ycat, ws.dcat, ws)
        for i in range(NUM_BLSTM - 1, -1, -1):
            pf, pb = self.prefixes(self.blstms[i])
            dseq = ctypes.c_void_p(ws.dcat.data_ptr() + 4 * 2 * H * i)
            nv.check(lib.lidbox_lstm_step_bwd(self._p(pf + ".U"), self._p(pb + ".U"), 2, B, T, H, nv.ptr(ws.zg[i]),
                                              nv.ptr(ws.cseq[i]), dseq, T * C6, C6, None,
                                              nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
            X, K = self._in_rows(ws, i)
            for d, p in enumerate((pf, pb)):
                dz = _rows(ws.zg[i][d].data_ptr(), 0, H4, 1, R)
                nv.check(lib.lidbox_gemm_tn(X, dz, self._p(p + ".W", True), H4, K, H4, 0, self._p(p + ".b", True), tws, tws_n, st))
                prow = 0 if d == 0 else 2                 # h_{t-1} (forward) / h_{t+1} (reverse): zero rows at both ends
                hprev = _rows(self._slice(ws, i, row=prow, col=d * H), (T + 2) * C6, C6, B, T)
                nv.check(lib.lidbox_gemm_tn(hprev, dz, self._p(p + ".U", True), H4, H, H4, 0, None, tws, tws_n, st))
                if i > 0:
                    # dX of layer i lands on top of blstm_bn's gradient in layer i-1's slice
                    dprev = _rows(ws.dcat.data_ptr() + 4 * 2 * H * (i - 1), T * C6, C6, B, T)
                    nv.check(lib.lidbox_gemm_nt(dz, self._p(p + ".W"), H4, dprev, H4, K, nv.EPI_ACCUM, None, gws, gws_n, st))

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


class EmbeddingExtractor:
    """reference spherespeaker.py:23-25: the output of the `l2_normalize` layer, in inference mode"""

    def __init__(self, model):
        self.model = model

    def __call__(self, x, training=False):
        return self.model.embed(x)

    predict = __call__


def as_embedding_extractor(model):
    return EmbeddingExtractor(model)


__all__ = ["SphereSpeakerModel", "create", "loader", "as_embedding_extractor"]
