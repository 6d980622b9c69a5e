"""
Convolutional-recurrent engine: the host-side orchestration of `lidbox_amd.models.crnn` (reference lidbox/models/crnn.py:24-52).

A model is  Conv2D blocks  ->  Bidirectional(LSTM) final states  ->  Dense  ->  output activation.  Each block is
Conv2D(f, k, relu, padding="same", l2 kernel regulariser) -> BatchNormalization -> MaxPool2D(2).  The reference turns the input
[B, T, F] into an image [B, F, T, 1] (height = frequency); here images are stored time-major, [B, T, F, C] with channels
innermost, so the model input is already the first block's image, both Permutes cost nothing and the last pool output is the
BLSTM's input [B, T5, F5 * C] in Keras' feature order (f * C + c).  Conv kernels keep the Keras layout [k, k, C_in, C_out]
(first index over frequency); csrc/conv2d.hip maps it onto the time-major storage.

The scaffolding is `lidbox_amd.models.flat`'s.  Per block: lidbox_conv2d_fwd (ReLU in the
epilogue) -> lidbox_bn_train_stats (4-D input: tf.keras' fused path, Bessel-corrected moving variance) ->
lidbox_bn_maxpool2d_fwd (normalise, 2 x 2 maximum, winner codes); backward lidbox_maxpool2d_bwd -> lidbox_bn_bwd(relu_mask) ->
lidbox_conv2d_wgrad (dW, db) -> lidbox_conv2d_dgrad (not for the first block, whose input is the model input).  The BLSTM is
flat's lstm_layer_fwd / lstm_layer_bwd on the lidbox_lstm_fwd / _bwd walk (with dh_last); its final
states (forward t = T5-1, backward t = 0) are copied side by side into the Dense head's input.

The conv kernels' l2(weight_decay) terms are the model's `regularizers` [(parameter name, lambda)]: the Trainer adds
lambda * sum W^2 to the loss and 2 lambda W to the gradient (lidbox_l2_penalty).

Parameter names: `conv_1.W`, `conv_1.b`, `conv_1_bn.gamma`, `blstm_forward.W`, `blstm_backward.U`, `output.W`; moving
statistics `conv_1_bn.moving_mean`, ...  The BLSTM halves are named by the Bidirectional wrapper and the direction, because
Keras numbers the inner `forward_lstm_N` per session.

Ragged pass (inference, float32): `rnn_ragged.RaggedRecurrent` on `ragged_pass.RaggedPass`; the model adds its length check,
its plan (per-level offsets and the BLSTM's `recurrent_plan`, with the capacity `rec` for the BLSTM's rows) and `_ragged_pass`.
"""
import ctypes

import numpy as np
import torch

from .. import _native as nv
from .flat import BatchNormSpec, FlatModel, LSTMLayer, Workspace, _rows, lstm_layer_bwd, lstm_layer_fwd
from .ragged import recurrent_plan
from .rnn import LSTMSpec
from .rnn_ragged import RaggedPlanOnDevice, RaggedRecurrent
from .tdnn import DenseSpec


class Conv2DSpec:
    """Conv2D(filters, kernel_size, activation="relu", padding="same", kernel_regularizer=l2(weight_decay)) ->
    BatchNormalization(epsilon=1e-3, momentum=0.99) -> MaxPool2D(2), the reference's block `name` (crnn.py:36-43)"""

    def __init__(self, name, filters, kernel_size, weight_decay=0.0, momentum=0.99, epsilon=1e-3):
        self.name, self.filters, self.k = name, int(filters), int(kernel_size)
        self.weight_decay, self.momentum, self.epsilon = float(weight_decay), float(momentum), float(epsilon)
        self.bn = name + "_bn"
        self.bn_spec = BatchNormSpec(self.bn, momentum, epsilon)


def pooled_sizes(T, F, blocks):
    """[(T_l, F_l)] of every block's input and, last, of the last pool's output (MaxPool2D(2) "valid": floor halving)"""
    out = [(int(T), int(F))]
    for _ in range(blocks):
        T, F = T // 2, F // 2
        out.append((T, F))
    return out


def pooled_lengths(lengths, blocks):
    """[blocks + 1][B]: every utterance's frames at the input of each block and, last, behind the last pool (T_b -> T_b // 2)"""
    T = np.asarray(lengths, np.int64).reshape(-1)
    out = [T]
    for _ in range(blocks):
        out.append(out[-1] // 2)
    return out


def pooled_offsets(lengths, blocks):
    """[blocks + 1][B + 1] int64: the first image row of every utterance at each level of `pooled_lengths` (entry B: the level's
    rows), utterances stored end to end"""
    return [np.concatenate(([0], np.cumsum(T))).astype(np.int64) for T in pooled_lengths(lengths, blocks)]


def check_pooled_lengths(name, lengths, blocks):
    """the dense workspace's refusal ("too small for ... pooling layers") for the first utterance no frame of which survives"""
    short = np.flatnonzero(np.asarray(lengths) < 2 ** blocks)
    if len(short):
        b = int(short[0])
        raise ValueError("%s: utterance %d has %d frames, which is too small for %d pooling layers (at least %d frames)"
                         % (name, b, int(lengths[b]), blocks, 2 ** blocks))


class _Workspace(Workspace):
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


class ConvRecurrentModel(FlatModel, RaggedRecurrent):
    """Conv2D blocks -> Bidirectional(LSTM) final states -> Dense -> output activation (see the module docstring)."""

    workspace_class = _Workspace

    def __init__(self, input_shape, convs2d, lstm_units, num_outputs, name="crnn", output_activation="softmax", seed=None,
                 device=None, compute_dtype="float32"):
        super().__init__(input_shape, name, output_activation, seed, device, compute_dtype)
        if len(input_shape) != 2:
            raise ValueError("input_shape must be (T, F), got %r" % (input_shape,))
        self.convs2d = list(convs2d)
        for l in self.convs2d:
            if l.filters % 16 or l.k % 2 == 0:
                raise ValueError("%s: filters must be a multiple of 16 and the kernel size odd" % l.name)
        F5 = pooled_sizes(1, self.input_dim, len(self.convs2d))[-1][1]
        if F5 < 1:
            raise ValueError("%s: %d frequency bins are too few for %d pooling layers" % (name, self.input_dim, len(self.convs2d)))
        self.lstm_input_dim = F5 * self.convs2d[-1].filters
        self.lstm = LSTMSpec("lstm", lstm_units, bidirectional=True, return_sequences=False, wrapper="blstm")
        self.lstm.prefixes = ["blstm_forward", "blstm_backward"]       # named by wrapper and direction (module docstring)
        self.denses = [DenseSpec("output", num_outputs, relu=False)]
        cin = 1
        for l in self.convs2d:
            self.add_param(l.name + ".W", (l.k, l.k, cin, l.filters))
            self.add_param(l.name + ".b", (l.filters,))
            self.add_bn(l.bn, l.filters)
            cin = l.filters
        H, D = self.lstm.units, self.lstm_input_dim
        for p in self.lstm.prefixes:
            self.add_param(p + ".W", (D, 4 * H))
            self.add_param(p + ".U", (H, 4 * H))
            self.add_param(p + ".b", (4 * H,))
        self.add_param("output.W", (2 * H, num_outputs))
        self.add_param("output.b", (num_outputs,))
        self.unit_forget_biases = {p + ".b" for p in self.lstm.prefixes}
        self.output_dim = int(num_outputs)
        self.regularizers = [(l.name + ".W", l.weight_decay) for l in self.convs2d if l.weight_decay > 0]
        self.l2_ws = torch.empty(nv.lib.lidbox_l2_penalty_workspace(), dtype=torch.uint8, device=self.device)
        self._finish(seed)

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

    def _block_input(self, ws, i):
        return ws.x if i == 0 else ws.p[i - 1]

    def _blstm(self, ws):
        H, D = self.lstm.units, self.lstm_input_dim
        return LSTMLayer(self.lstm.prefixes, _rows(ws.p[-1].data_ptr(), 0, D, 1, ws.B * ws.T5), D, ws.B, ws.T5, H, ws.zg, ws.cseq,
                         ws.hseq.data_ptr(), 2 * H, ws.lstm_ws, ws.gemm_ws, ws.tn_ws)

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
            cp = self._bn_fwd(l.bn_spec, ws.y[i], B * T * F, C, ws.c[i], None, ws, training, update_moving, bessel=None)
            nv.check(lib.lidbox_bn_maxpool2d_fwd(nv.ptr(ws.y[i]), B, T, F, C, cp[2], cp[3], nv.ptr(ws.p[i]), nv.ptr(ws.code[i]), st))
            cin = C
        # BLSTM: input projections, the walk, then the final states side by side (forward t = T5-1, backward t = 0)
        H, T5 = self.lstm.units, ws.T5
        lstm_layer_fwd(self, self._blstm(ws))
        hs, row = ws.hseq.data_ptr(), 4 * 2 * H
        for d, r in ((0, T5), (1, 1)):
            nv.check(lib.lidbox_copy_2d(ctypes.c_void_p(ws.hlast.data_ptr() + 4 * d * H), 4 * 2 * H,
                                        ctypes.c_void_p(hs + r * row + 4 * d * H), (T5 + 2) * row, 4 * H, B, st))
        if stop_before_output:
            return ws.hlast
        nv.check(lib.lidbox_gemm_nn(_rows(ws.hlast.data_ptr(), 0, 2 * H, 1, B), self._p("output.W"), self.output_dim,
                                    _rows(ws.h[0].data_ptr(), 0, self.output_dim, 1, B), 2 * H, self.output_dim, nv.EPI_BIAS,
                                    self._p("output.b"), gws, gws_n, st))
        return self._output_activation(ws, ws.h[0], self.output_dim)

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
        lstm_layer_bwd(self, self._blstm(ws), None, T5 * 2 * H, 2 * H, dh_last=nv.ptr(ws.dlast),
                       dX=_rows(ws.dp[-1].data_ptr(), 0, D, 1, B * T5))
        for i in range(len(self.convs2d) - 1, -1, -1):
            l = self.convs2d[i]
            (T, F), C = ws.sizes[i], l.filters
            cin = 1 if i == 0 else self.convs2d[i - 1].filters
            R = B * T * F
            nv.check(lib.lidbox_maxpool2d_bwd(nv.ptr(ws.dp[i]), nv.ptr(ws.code[i]), B, T, F, C, nv.ptr(ws.dbn), st))
            self._bn_bwd(l.bn_spec, ws.y[i], R, C, ws.c[i], ws.dbn, 1, ws.dz, ws)
            x = self._block_input(ws, i)
            nv.check(lib.lidbox_conv2d_wgrad(nv.ptr(x), nv.ptr(ws.dz), B, T, F, cin, C, l.k, self._p(l.name + ".W", True),
                                             self._p(l.name + ".b", True), nv.ptr(ws.wgrad_ws), ws.wgrad_ws.numel(), st))
            if i > 0:
                nv.check(lib.lidbox_conv2d_dgrad(nv.ptr(ws.dz), B, T, F, cin, C, self._p(l.name + ".W"), l.k, nv.ptr(ws.dp[i - 1]),
                                                 nv.ptr(ws.dgrad_ws), ws.dgrad_ws.numel(), st))

    # ------------------------------------------------------------ ragged pass (inference, float32; models/ragged_pass.py)
    def _ragged_embedding_dim(self):
        return 2 * self.lstm.units

    def _ragged_buffers_rows(self, cap):
        """per input row: y, one block's conv output (the largest level decides), and p[i], the pool output of block i < n - 1
        (level i + 1 has at most cap // 2^(i+1) rows); c: the BatchNormalization constants of every block"""
        f32 = dict(dtype=torch.float32, device=self.device)
        Fs = [F for _, F in pooled_sizes(1, self.input_dim, len(self.convs2d))]
        ny = max((cap >> i) * Fs[i] * l.filters for i, l in enumerate(self.convs2d))
        p = [torch.zeros(max(1, (cap >> (i + 1)) * Fs[i + 1] * l.filters), **f32) for i, l in enumerate(self.convs2d[:-1])]
        return dict(y=torch.zeros(max(1, ny), **f32), p=p, c=[torch.zeros((4, l.filters), **f32) for l in self.convs2d])

    def _ragged_buffers_rec(self, cap):
        """per row of the BLSTM's [pad, frames, pad] layout: its input (the last pool's output), the gates, c and h"""
        f32 = dict(dtype=torch.float32, device=self.device)
        H, D = self.lstm.units, self.lstm_input_dim
        return dict(x=torch.zeros((cap, D), **f32), zg=torch.zeros(2 * cap * 4 * H, **f32), cseq=torch.zeros(2 * cap * H, **f32),
                    hseq=torch.zeros((cap, 2 * H), **f32))

    def _ragged_buffers_B(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        return dict(hlast=torch.zeros((cap, 2 * self.lstm.units), **f32), h=[torch.zeros((cap, self.output_dim), **f32)],
                    logp=torch.zeros((cap, self.output_dim), **f32))

    def _ragged_check_lengths(self, lengths):
        check_pooled_lengths(self.name, lengths, len(self.convs2d))

    def _ragged_plan(self, ro, lengths):
        """(the offsets of every pooled level, the BLSTM's plan over the lengths behind the last pool)"""
        offs = pooled_offsets(lengths, len(self.convs2d))
        plan = recurrent_plan(np.diff(offs[-1]))
        return (offs, plan), dict(rows=int(ro[-1]), B=plan.B, rec=plan.Rp)

    def _ragged_pass(self, ws, plan, X, ro, upto_embedding):
        """X [total_T, F], every utterance with at least 2^blocks frames; returns the model output [B, N] or, upto_embedding,
        the BLSTM's final states [B, 2H] (the dense pass's stop_before_output).  The blocks run over all frames at once
        (lidbox_conv2d_ragged_fwd -> lidbox_bn_maxpool2d_ragged_fwd on per-level offsets T_b -> T_b // 2, utterances end to
        end); the last pool writes into `recurrent_plan`'s layout over the T_b // 2^blocks, where the BLSTM is one projection
        GEMM per direction and lidbox_lstm_ragged_fwd."""
        (offs, plan), B, n = plan, ws.B, len(self.convs2d)
        st, lib = nv.current_stream(), nv.lib
        dev = RaggedPlanOnDevice(plan, ro, self.device, extra=offs[1:n])
        dev_offs = [dev.ro] + dev.extra
        Fs = [F for _, F in pooled_sizes(1, self.input_dim, n)]
        x, cin = nv.ptr(X), 1
        for i, l in enumerate(self.convs2d):
            C, rows = l.filters, int(offs[i][-1])
            nv.check(lib.lidbox_conv2d_ragged_fwd(x, dev_offs[i], B, rows, Fs[i], cin, self._p(l.name + ".W"), l.k, C,
                                                  self._p(l.name + ".b"), 1, nv.ptr(ws.y), st))
            cp = self._bn_fwd(l.bn_spec, None, 0, C, ws.c[i], None, ws, False, False)
            if i + 1 < n:
                out, out_offs, out_rows = nv.ptr(ws.p[i]), dev_offs[i + 1], int(offs[i + 1][-1])
            else:
                # the frames of utterance b go behind the pad row that opens its segment: y one row on, segments as they are
                out = ctypes.c_void_p(ws.x.data_ptr() + 4 * self.lstm_input_dim)
                out_offs, out_rows = dev.seg, plan.Rp - 1
            nv.check(lib.lidbox_bn_maxpool2d_ragged_fwd(nv.ptr(ws.y), dev_offs[i], B, Fs[i], C, cp[2], cp[3], out, out_offs,
                                                        out_rows, None, st))
            x, cin = out, C
        H, D = self.lstm.units, self.lstm_input_dim
        self._ragged_lstm_layer(ws, plan, dev, _rows(ws.x.data_ptr(), 0, D, 1, plan.Rp), D, self.lstm.prefixes, H,
                                ws.hseq.data_ptr(), 2 * H, ws.hlast)
        if upto_embedding:
            return ws.hlast
        N = self.output_dim
        ws.reserve_gemm_ws(self, max(16, lib.lidbox_gemm_rows_workspace(B, N, 2 * H)))
        nv.check(lib.lidbox_gemm_nn(_rows(ws.hlast.data_ptr(), 0, 2 * H, 1, B), self._p("output.W"), N,
                                    _rows(ws.h[0].data_ptr(), 0, N, 1, B), 2 * H, N, nv.EPI_BIAS, self._p("output.b"),
                                    nv.ptr(ws.gemm_ws), ws.gemm_ws.numel(), st))
        return self._output_activation(ws, ws.h[0], N)


__all__ = ["Conv2DSpec", "ConvRecurrentModel", "pooled_sizes", "pooled_lengths", "pooled_offsets"]
