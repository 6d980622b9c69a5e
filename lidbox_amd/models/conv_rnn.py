"""
Convolutional-recurrent engine: the host-side orchestration of `lidbox_amd.models.crnn` (reference lidbox/models/crnn.py:24-52).

A model is  Conv2D blocks  ->  Bidirectional(LSTM) final states  ->  Dense  ->  output activation.  Each block is
Conv2D(f, k, relu, padding="same", l2 kernel regulariser) -> BatchNormalization -> MaxPool2D(2).  The reference turns the input
[B, T, F] into an image [B, F, T, 1] (height = frequency); here images are stored time-major, [B, T, F, C] with channels
innermost, so the model input is already the first block's image, both Permutes cost nothing and the last pool output is the
BLSTM's input [B, T5, F5 * C] in Keras' feature order (f * C + c).  Conv kernels keep the Keras layout [k, k, C_in, C_out]
(first index over frequency); csrc/conv2d.hip maps it onto the time-major storage.

Everything numeric is a liblidbox_hip.so call on preallocated device buffers, so `lidbox_amd.train.Trainer` captures the whole
train step into a hipGraph (one gradient bucket, backward is `backward_head_ws`).  Per block: lidbox_conv2d_fwd (ReLU in the
epilogue) -> lidbox_bn_train_stats (4-D input: tf.keras' fused path, Bessel-corrected moving variance) ->
lidbox_bn_maxpool2d_fwd (normalise, 2 x 2 maximum, winner codes); backward lidbox_maxpool2d_bwd -> lidbox_bn_bwd(relu_mask) ->
lidbox_conv2d_wgrad (dW, db) -> lidbox_conv2d_dgrad (not for the first block, whose input is the model input).  The BLSTM is
`models/rnn.py`'s LSTM walk (lidbox_lstm_fwd / _bwd with dh_last) with the input projection, dW / dU and dX as GEMMs; its final
states (forward t = T5-1, backward t = 0) are copied side by side into the Dense head's input.

The conv kernels' l2(weight_decay) terms are the model's `regularizers` [(parameter name, lambda)]: the Trainer adds
lambda * sum W^2 to the loss and 2 lambda W to the gradient (lidbox_l2_penalty).

Parameters live in one flat fp32 buffer with Keras names: `conv_1.W`, `conv_1.b`, `conv_1_bn.gamma`, `blstm_forward.W`,
`blstm_backward.U`, `output.W`; the BatchNormalization moving statistics (`conv_1_bn.moving_mean`, ...) in `state`.  The
BLSTM halves are named by the Bidirectional wrapper and the direction, because Keras numbers the inner `forward_lstm_N` per
session.  Initialisation as Keras: glorot_uniform kernels (Conv2D fan_in = k^2 C_in, fan_out = k^2 C_out), orthogonal
recurrent kernels, zero biases with unit forget bias, gamma 1 / beta 0 / moving mean 0 / moving variance 1.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv
from .rnn import LSTMSpec, RecurrentModel, orthogonal
from .tdnn import DenseSpec, _rows


class Conv2DSpec:
    """Conv2D(filters, kernel_size, activation="relu", padding="same", kernel_regularizer=l2(weight_decay)) ->
    BatchNormalization(epsilon=1e-3, momentum=0.99) -> MaxPool2D(2), the reference's block `name` (crnn.py:36-43)"""

    def __init__(self, name, filters, kernel_size, weight_decay=0.0, momentum=0.99, epsilon=1e-3):
        self.name, self.filters, self.k = name, int(filters), int(kernel_size)
        self.weight_decay, self.momentum, self.epsilon = float(weight_decay), float(momentum), float(epsilon)
        self.bn = name + "_bn"


def _align4(n):
    return (n + 3) & ~3


def pooled_sizes(T, F, blocks):
    """[(T_l, F_l)] of every block's input and, last, of the last pool's output (MaxPool2D(2) "valid": floor halving)"""
    out = [(int(T), int(F))]
    for _ in range(blocks):
        T, F = T // 2, F // 2
        out.append((T, F))
    return out


class _Workspace:
    """All per-(B, T) device buffers of one CRNN model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.T = B, T
        F = model.input_dim
        self.sizes = pooled_sizes(T, F, len(model.convs2d))
        if self.sizes[-1][0] < 1 or self.sizes[-1][1] < 1:
            raise ValueError("%s: input (%d, %d) is too small for %d pooling layers" % (model.name, T, F, len(model.convs2d)))
        self.x = torch.zeros((B, T, F), **f32)
        # block l: y conv output (after the ReLU), c BatchNormalization constants (mean, invstd, scale, shift), p pool output
        # (the next block's input), code the pool's winner codes, dp the gradient of p
        self.y, self.c, self.p, self.code, self.dp = [], [], [], [], []
        bws, dws, wws = 16, 16, 16
        cin = 1
        big = 0
        for l, (Tl, Fl), (To, Fo) in zip(model.convs2d, self.sizes[:-1], self.sizes[1:]):
            C = l.filters
            self.y.append(torch.zeros((B, Tl, Fl, C), **f32))
            self.c.append(torch.zeros((4, C), **f32))
            self.p.append(torch.zeros((B, To, Fo, C), **f32))
            self.code.append(torch.zeros((B, To, Fo, C), dtype=torch.uint8, device=dev))
            self.dp.append(torch.zeros((B, To, Fo, C), **f32))
            bws = max(bws, nv.lib.lidbox_bn_workspace(B * Tl * Fl, C))
            dws = max(dws, nv.lib.lidbox_conv2d_dgrad_workspace(l.k, cin, C))
            wws = max(wws, nv.lib.lidbox_conv2d_wgrad_workspace(B, Tl, Fl, cin, C, l.k))
            big = max(big, B * Tl * Fl * C)
            cin = C
        self.dbn = torch.zeros(max(big, 1), **f32)          # pool backward's output (the gradient of the BatchNormalization output)
        self.dz = torch.zeros(max(big, 1), **f32)           # BatchNormalization backward's output (the gradient in front of the ReLU)
        # BLSTM over the last pool output [B, T5, D]
        T5 = self.sizes[-1][0]
        H, D = model.lstm.units, model.lstm_input_dim
        self.T5 = T5
        self.zg = torch.zeros((2, B, T5, 4 * H), **f32)
        self.hseq = torch.zeros((B, T5 + 2, 2 * H), **f32)  # rows 0 and T5+1 stay zero
        self.cseq = torch.zeros((2, B, T5, H), **f32)
        self.hlast = torch.zeros((B, 2 * H), **f32)
        self.dlast = torch.zeros((B, 2 * H), **f32)
        N = model.output_dim
        self.h = [torch.zeros((B, N), **f32)]                # logits
        self.dh = [torch.zeros((B, N), **f32)]
        self.logp = torch.zeros((B, N), **f32)
        self.loss = torch.zeros(4, **f32)
        lws = nv.lib.lidbox_lstm_workspace(B, T5, H, 2)
        gws = max(nv.lib.lidbox_gemm_rows_workspace(B * T5, 4 * H, D), nv.lib.lidbox_gemm_rows_workspace(B * T5, D, 4 * H),
                  nv.lib.lidbox_gemm_rows_workspace(B, N, 2 * H), nv.lib.lidbox_gemm_rows_workspace(B, 2 * H, N))
        tws = max(16, nv.lib.lidbox_gemm_tn_workspace(B * T5, D, 4 * H), nv.lib.lidbox_gemm_tn_workspace(B * T5, H, 4 * H),
                  nv.lib.lidbox_gemm_tn_workspace(B, 2 * H, N))
        self.lstm_ws = torch.empty(max(16, lws), dtype=torch.uint8, device=dev)
        self.gemm_ws = torch.empty(max(16, gws), dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.bn_ws = torch.empty(bws, dtype=torch.uint8, device=dev)
        self.dgrad_ws = torch.empty(dws, dtype=torch.uint8, device=dev)
        self.wgrad_ws = torch.empty(wws, dtype=torch.uint8, device=dev)
        self.pending = []

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        return ctypes.c_void_p(self.x.data_ptr()), self.x.stride(0), self.x.shape[1], self.x.shape[2]


class ConvRecurrentModel(RecurrentModel):
    """Conv2D blocks -> Bidirectional(LSTM) final states -> Dense -> output activation (see the module docstring).  Shares the
    public calls of `RecurrentModel` (input loading, __call__, set_weights, backward_ws)."""

    def __init__(self, input_shape, convs2d, lstm_units, num_outputs, name="crnn", output_activation="softmax", seed=None,
                 device=None, compute_dtype="float32"):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("%s computes in float32 only, got compute_dtype=%r" % (name, compute_dtype))
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        if len(input_shape) != 2:
            raise ValueError("input_shape must be (T, F), got %r" % (input_shape,))
        self.convs2d = list(convs2d)
        for l in self.convs2d:
            if l.filters % 16 or l.k % 2 == 0:
                raise ValueError("%s: filters must be a multiple of 16 and the kernel size odd" % l.name)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        F5 = pooled_sizes(1, self.input_dim, len(self.convs2d))[-1][1]
        if F5 < 1:
            raise ValueError("%s: %d frequency bins are too few for %d pooling layers" % (name, self.input_dim, len(self.convs2d)))
        self.lstm_input_dim = F5 * self.convs2d[-1].filters
        self.lstm = LSTMSpec("lstm", lstm_units, bidirectional=True, return_sequences=False, wrapper="blstm")
        self.lstm.prefixes = ["blstm_forward", "blstm_backward"]       # named by wrapper and direction (module docstring)
        self.denses = [DenseSpec("output", num_outputs, relu=False)]
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
        cin = 1
        for l in self.convs2d:
            for suffix, shape in ((".W", (l.k, l.k, cin, l.filters)), (".b", (l.filters,))):
                self.layout[l.name + suffix] = (off, shape)
                off = _align4(off + int(np.prod(shape)))
            for suffix in (".gamma", ".beta"):
                self.layout[l.bn + suffix] = (off, (l.filters,))
                off = _align4(off + l.filters)
            for suffix in (".moving_mean", ".moving_variance"):
                self.state_layout[l.bn + suffix] = (soff, (l.filters,))
                soff = _align4(soff + l.filters)
            cin = l.filters
        H, D = self.lstm.units, self.lstm_input_dim
        for p in self.lstm.prefixes:
            for suffix, shape in ((".W", (D, 4 * H)), (".U", (H, 4 * H)), (".b", (4 * H,))):
                self.layout[p + suffix] = (off, shape)
                off = _align4(off + int(np.prod(shape)))
        for suffix, shape in ((".W", (2 * H, num_outputs)), (".b", (num_outputs,))):
            self.layout["output" + suffix] = (off, shape)
            off = _align4(off + int(np.prod(shape)))
        self.output_dim = int(num_outputs)
        self.regularizers = [(l.name + ".W", l.weight_decay) for l in self.convs2d if l.weight_decay > 0]
        self.num_flat = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(max(soff, 4), dtype=torch.float32, device=self.device)
        self.l2_ws = torch.empty(nv.lib.lidbox_l2_penalty_workspace(), dtype=torch.uint8, device=self.device)
        self._init_weights(seed)
        self._ws = {}

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        """Keras defaults: glorot_uniform kernels, orthogonal recurrent kernels, zero biases with the LSTM forget gate's
        quarter set to 1, gamma 1, beta 0, moving mean 0, moving variance 1"""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.num_flat, np.float32)
        for name, (off, shape) in self.layout.items():
            n = int(np.prod(shape))
            if name.endswith(".W"):
                rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1          # receptive field of a Conv2D kernel
                limit = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
                host[off:off + n] = rng.uniform(-limit, limit, size=n).astype(np.float32)
            elif name.endswith(".U"):
                host[off:off + n] = orthogonal(shape, rng).astype(np.float32).ravel()
            elif name.endswith(".gamma"):
                host[off:off + n] = 1.0
            elif name.endswith(".b") and name.startswith("blstm_"):
                H = shape[0] // 4
                host[off + H:off + 2 * H] = 1.0
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
        """Keras `Model.count_params()`: every Conv2D / LSTM / Dense variable and 4C per BatchNormalization (gamma, beta and
        the two moving statistics)"""
        return sum(int(np.prod(s)) for _, s in list(self.layout.values()) + list(self.state_layout.values()))

    def get_weights(self):
        """dict name -> numpy array in Keras layouts (trainable parameters and the BatchNormalization moving statistics)"""
        return {n: self.param(n).detach().cpu().numpy().copy() for n in list(self.layout) + list(self.state_layout)}

    def _sp(self, name):
        off, _ = self.state_layout[name]
        return ctypes.c_void_p(self.state.data_ptr() + 4 * off)

    def regularization_loss(self):
        """sum of lambda * sum W^2 over the regularised kernels (what Keras adds to the loss in `evaluate` too), a float"""
        if not self.regularizers:
            return 0.0
        with torch.cuda.device(self.device):
            out = torch.zeros(1, dtype=torch.float32, device=self.device)
            self.apply_regularizers(None, out, 1.0)
            return float(out)

    def apply_regularizers(self, grad, loss, grad_scale):
        """grad (flat_grad or None) += 2 lambda grad_scale W, loss[0] (or None) += lambda sum W^2 (lidbox_l2_penalty)"""
        if not self.regularizers:
            return
        n = len(self.regularizers)
        offs = (ctypes.c_long * n)(*[self.layout[p][0] for p, _ in self.regularizers])
        sizes = (ctypes.c_long * n)(*[int(np.prod(self.layout[p][1])) for p, _ in self.regularizers])
        lams = (ctypes.c_float * n)(*[lam for _, lam in self.regularizers])
        nv.check(nv.lib.lidbox_l2_penalty(nv.ptr(self.flat), nv.ptr(grad), n, offs, sizes, lams, float(grad_scale), nv.ptr(loss),
                                          nv.ptr(self.l2_ws), self.l2_ws.numel(), nv.current_stream()))

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

    def _block_input(self, ws, i):
        return ws.x if i == 0 else ws.p[i - 1]

    def _lstm_in_rows(self, ws):
        return _rows(ws.p[-1].data_ptr(), 0, self.lstm_input_dim, 1, ws.B * ws.T5)

    # ------------------------------------------------------------------ forward
    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False):
        """The model input buffer (ws.input_view()) must already hold the input.  training selects batch statistics in the
        BatchNormalization layers (update_moving=False leaves the moving statistics untouched).  Returns the probabilities /
        log-probs / logits (output_activation None); stop_before_output: the BLSTM output [B, 2H]."""
        st = nv.current_stream()
        lib = nv.lib
        B = ws.B
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.hlast if stop_before_output else ws.logp
        cin = 1
        for i, l in enumerate(self.convs2d):
            (T, F), C = ws.sizes[i], l.filters
            x = self._block_input(ws, i)
            nv.check(lib.lidbox_conv2d_fwd(nv.ptr(x), B, T, F, cin, self._p(l.name + ".W"), l.k, C, self._p(l.name + ".b"), 1,
                                           nv.ptr(ws.y[i]), st))
            cp = [ctypes.c_void_p(ws.c[i].data_ptr() + 4 * j * C) for j in range(4)]
            R = B * T * F
            if training:
                mm = self._sp(l.bn + ".moving_mean") if update_moving else None
                mv = self._sp(l.bn + ".moving_variance") if update_moving else None
                nv.check(lib.lidbox_bn_train_stats(nv.ptr(ws.y[i]), R, C, self._p(l.bn + ".gamma"), self._p(l.bn + ".beta"),
                                                   l.epsilon, l.momentum, mm, mv, cp[0], cp[1], cp[2], cp[3],
                                                   nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
            else:
                nv.check(lib.lidbox_bn_infer_consts(self._p(l.bn + ".gamma"), self._p(l.bn + ".beta"), self._sp(l.bn + ".moving_mean"),
                                                    self._sp(l.bn + ".moving_variance"), l.epsilon, C, cp[2], cp[3], st))
            nv.check(lib.lidbox_bn_maxpool2d_fwd(nv.ptr(ws.y[i]), B, T, F, C, cp[2], cp[3], nv.ptr(ws.p[i]), nv.ptr(ws.code[i]), st))
            cin = C
        # BLSTM: input projections, the walk, then the final states side by side (forward t = T5-1, backward t = 0)
        H, D, T5 = self.lstm.units, self.lstm_input_dim, ws.T5
        X = self._lstm_in_rows(ws)
        for d, p in enumerate(self.lstm.prefixes):
            nv.check(lib.lidbox_gemm_nn(X, self._p(p + ".W"), 4 * H, _rows(ws.zg[d].data_ptr(), 0, 4 * H, 1, B * T5), D, 4 * H,
                                        nv.EPI_BIAS, self._p(p + ".b"), gws, gws_n, st))
        nv.check(lib.lidbox_lstm_fwd(self._p("blstm_forward.U"), self._p("blstm_backward.U"), 2, B, T5, H, nv.ptr(ws.zg),
                                     nv.ptr(ws.hseq), nv.ptr(ws.cseq), nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
        hs, row = ws.hseq.data_ptr(), 4 * 2 * H
        for d, r in ((0, T5), (1, 1)):
            nv.check(lib.lidbox_copy_2d(ctypes.c_void_p(ws.hlast.data_ptr() + 4 * d * H), 4 * 2 * H,
                                        ctypes.c_void_p(hs + r * row + 4 * d * H), (T5 + 2) * row, 4 * H, B, st))
        if stop_before_output:
            return ws.hlast
        nv.check(lib.lidbox_gemm_nn(_rows(ws.hlast.data_ptr(), 0, 2 * H, 1, B), self._p("output.W"), self.output_dim,
                                    _rows(ws.h[0].data_ptr(), 0, self.output_dim, 1, B), 2 * H, self.output_dim, nv.EPI_BIAS,
                                    self._p("output.b"), gws, gws_n, st))
        if self.output_activation is None:
            return ws.h[0]
        fn = lib.lidbox_softmax_fwd if self.output_activation == "softmax" else lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(ws.h[0]), B, self.output_dim, nv.ptr(ws.logp), st))
        return ws.logp

    # ------------------------------------------------------------------ backward
    def backward_head_ws(self, ws):
        """the whole backward pass (dh[-1] holds d loss / d logits): Dense, BLSTM, then every block from the top down.
        Fills flat_grad (overwrites; the regularisers are the Trainer's)."""
        st = nv.current_stream()
        lib = nv.lib
        B = ws.B
        ws.pending = []
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        tws, tws_n = nv.ptr(ws.tn_ws), ws.tn_ws.numel()
        if B == 0:
            return
        H, D, T5, N = self.lstm.units, self.lstm_input_dim, ws.T5, self.output_dim
        dy = _rows(ws.dh[0].data_ptr(), 0, N, 1, B)
        nv.check(lib.lidbox_gemm_tn(_rows(ws.hlast.data_ptr(), 0, 2 * H, 1, B), dy, self._p("output.W", True), N, 2 * H, N, 0,
                                    self._p("output.b", True), tws, tws_n, st))
        nv.check(lib.lidbox_gemm_nt(dy, self._p("output.W"), N, _rows(ws.dlast.data_ptr(), 0, 2 * H, 1, B), N, 2 * H,
                                    nv.EPI_NONE, None, gws, gws_n, st))
        nv.check(lib.lidbox_lstm_bwd(self._p("blstm_forward.U"), self._p("blstm_backward.U"), 2, B, T5, H, nv.ptr(ws.zg),
                                     nv.ptr(ws.cseq), None, T5 * 2 * H, nv.ptr(ws.dlast), nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
        X = self._lstm_in_rows(ws)
        hs, ldo = ws.hseq.data_ptr(), 2 * H
        for d, p in enumerate(self.lstm.prefixes):
            dz = _rows(ws.zg[d].data_ptr(), 0, 4 * H, 1, B * T5)
            nv.check(lib.lidbox_gemm_tn(X, dz, self._p(p + ".W", True), 4 * H, D, 4 * H, 0, self._p(p + ".b", True), tws, tws_n, st))
            prow = 0 if d == 0 else 2                 # h_{t-1} (forward) / h_{t+1} (reverse): zero rows at both ends
            hprev = _rows(hs + 4 * (prow * ldo + d * H), (T5 + 2) * ldo, ldo, B, T5)
            nv.check(lib.lidbox_gemm_tn(hprev, dz, self._p(p + ".U", True), 4 * H, H, 4 * H, 0, None, tws, tws_n, st))
            nv.check(lib.lidbox_gemm_nt(dz, self._p(p + ".W"), 4 * H, _rows(ws.dp[-1].data_ptr(), 0, D, 1, B * T5), 4 * H, D,
                                        nv.EPI_ACCUM if d > 0 else nv.EPI_NONE, None, gws, gws_n, st))
        for i in range(len(self.convs2d) - 1, -1, -1):
            l = self.convs2d[i]
            (T, F), C = ws.sizes[i], l.filters
            cin = 1 if i == 0 else self.convs2d[i - 1].filters
            R = B * T * F
            nv.check(lib.lidbox_maxpool2d_bwd(nv.ptr(ws.dp[i]), nv.ptr(ws.code[i]), B, T, F, C, nv.ptr(ws.dbn), st))
            nv.check(lib.lidbox_bn_bwd(nv.ptr(ws.y[i]), _rows(ws.dbn.data_ptr(), 0, C, 1, R), R, C, nv.ptr(ws.c[i][0]),
                                       nv.ptr(ws.c[i][1]), self._p(l.bn + ".gamma"), 1, self._p(l.bn + ".gamma", True),
                                       self._p(l.bn + ".beta", True), nv.ptr(ws.dz), nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
            x = self._block_input(ws, i)
            nv.check(lib.lidbox_conv2d_wgrad(nv.ptr(x), nv.ptr(ws.dz), B, T, F, cin, C, l.k, self._p(l.name + ".W", True),
                                             self._p(l.name + ".b", True), nv.ptr(ws.wgrad_ws), ws.wgrad_ws.numel(), st))
            if i > 0:
                nv.check(lib.lidbox_conv2d_dgrad(nv.ptr(ws.dz), B, T, F, cin, C, self._p(l.name + ".W"), l.k, nv.ptr(ws.dp[i - 1]),
                                                 nv.ptr(ws.dgrad_ws), ws.dgrad_ws.numel(), st))

    # ------------------------------------------------------------------ public call
    def __call__(self, x, training=False):
        """x [B, T, F] on the HIP device -> the model output [B, num_outputs] (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, training)
            return self.forward_ws(ws, training=training).clone()

    predict = __call__


__all__ = ["Conv2DSpec", "ConvRecurrentModel", "pooled_sizes"]
