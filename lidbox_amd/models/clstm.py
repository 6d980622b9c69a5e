"""
Counterpart of lidbox/models/clstm.py:45-81 (Miao et al. 2019): the x-vector with three switches.

    input [B, T, F] -> GaussianNoise(0.01) -> Dropout(0.4, noise_shape=(None, 1, F))           (training only)
    [use_conv2d]    image [B, T, F, 1] -> Conv2D(128, (3, 9), strides=(1, 6), "same") `conv2d_1` -> BatchNormalization -> ReLU
                    -> Conv2D(256, (3, 9), (1, 6), "same") `conv2d_2` -> BatchNormalization -> ReLU -> max over frequency
    frame1 (512, k 5) -> frame2 (512, k 3, s 2) -> frame3 (512, k 3, s 3)        causal Conv1D + ReLU, as in the x-vector
    [use_lstm]      LSTM(512, return_sequences=True) `lstm` (TF2 defaults)
    frame4 (512, k 1) -> frame5 (1500, k 1)
    [use_attention] frequency_attention(d_a=64, d_f=60) (`Wf_1`, `Wf_2`)
    stats pooling -> segment1 -> segment2 (512, ReLU) -> Dense(N) `output` -> output activation

The frame layers, the pooling, the attention, the head and their backward are `SequentialTDNN`'s.  This module adds the 2-D
front-end, which writes frame1's input rows (behind its causal zero rows), and the LSTM between frame3 and frame4, whose h
sequence frame4 reads in place.  The images are stored time-major, [B][T][F][C], which is already the reference's
Reshape((T, F, 1)) with height = time.  Front-end per layer: lidbox_conv2d_strided_fwd (fp32 MFMA, taps that lie wholly in the
padding skipped) -> lidbox_bn_train_stats (4-D input: tf.keras' fused path, Bessel-corrected moving variance) ->
lidbox_bn_relu_fwd / lidbox_bn_relu_maxf_fwd; backward lidbox_bn_relu_maxf_bwd (TF's even split over ties) / lidbox_bn_relu_bwd
-> lidbox_bn_bwd -> lidbox_conv2d_strided_wgrad, and lidbox_conv2d_strided_dgrad for conv2d_2.  The LSTM is models/flat.py's
lstm_layer_fwd / lstm_layer_bwd on the lidbox_lstm_fwd / _bwd walk, with its GEMMs on the model's GEMM family.

Input noise and channel dropout run as ONE launch (lidbox_input_noise_dropout) keyed by the Trainer's device step counter,
so every replay of the captured step draws fresh noise; outside training neither is applied.

Parameters: one flat fp32 buffer in Keras layouts, in the order conv2d_1, conv2d_2 (lowest: complete last), frame1..frame3,
lstm, frame4, frame5, Wf_1, Wf_2, segment1, segment2, output, so that the Trainer's default bucketed gradient exchange stays
correct: every bucket boundary is a frame layer's kernel, and each parameter's gradient is final before the stage that
completes its bucket ends.  BatchNormalization moving statistics live in `state`.  fp32 only.

Ragged pass (inference): `_ragged_pass` composes SequentialTDNN's helpers (upload, pack, conv, pool and head) with the 2-D
front-end in front of the pack, the LSTM on level 3 in front of frame4 and the attention in front of the pool; the buffers of
the LSTM and the attention are sized off the level buffers and live and die with them (`_ragged_buffers_rows`), the
front-end's are sized by the capacity `frames`.
"""
import ctypes

import numpy as np
import torch

from .. import _native as nv
from .flat import BatchNormSpec, FlatParams, LSTMLayer, _rows, lstm_layer_bwd, lstm_layer_fwd
from .ragged import ragged_plan, recurrent_plan
from .tdnn import DenseSpec, FreqAttentionSpec, SequentialTDNN, _Workspace as _TDNNWorkspace
from .xvector import frame_layer, segment_layer

NOISE_STDDEV = 0.01                 # clstm.py:48
DROPOUT_RATE = 0.4                  # clstm.py:49
FILTERS = (128, 256)                # clstm.py:53,56
KERNEL = (3, 9)                     # (time, frequency)
STRIDES = (1, 6)
FRAME_UNITS = (512, 512, 512, 512, 1500)
FRAME_KERNELS = ((5, 1), (3, 2), (3, 3), (1, 1), (1, 1))   # (kernel, stride) of frame1..frame5
SEGMENT_UNITS = (512, 512)
ATTENTION_D_A, ATTENTION_D_F = 64, 60                       # clstm.py:71 calls frequency_attention(x, d_f=60)
BN_MOMENTUM, BN_EPSILON = 0.99, 1e-3


def same_padding(n, k, s):
    """TF padding="same" along one axis of n cells: (outputs, zeros before, zeros after) = (ceil(n / s), pad // 2, the rest)
    with pad = max((outputs - 1) s + k - n, 0)"""
    out = -(-int(n) // int(s))
    pad = max((out - 1) * int(s) + int(k) - int(n), 0)
    return out, pad // 2, pad - pad // 2


def conv2d_frequency_sizes(F):
    """[(F_in, F_out, pad before, pad after)] of conv2d_1 and conv2d_2 along frequency (40 -> 7 -> 2)"""
    out = []
    for _ in FILTERS:
        Fo, p0, p1 = same_padding(F, KERNEL[1], STRIDES[1])
        out.append((F, Fo, p0, p1))
        F = Fo
    return out


def conv2d_taps(F):
    """[(F_in, F_out, nv.Conv2DTaps)] of the two layers; time: stride 1, pads 1 / 1 (same_padding(T, 3, 1) for any T)"""
    _, t0, t1 = same_padding(1, KERNEL[0], STRIDES[0])
    return [(Fi, Fo, nv.Conv2DTaps(KERNEL[0], KERNEL[1], STRIDES[1], t0, t1, p0, p1, 1))
            for Fi, Fo, p0, p1 in conv2d_frequency_sizes(F)]


def keras_layout(input_shape, num_outputs, use_attention=False, use_conv2d=False, use_lstm=False, filters=FILTERS,
                 frame_units=FRAME_UNITS, segment_units=SEGMENT_UNITS):
    """[(name, shape, trainable)] of every Keras variable, in flat-buffer order (the moving statistics are not trainable).
    The LSTM has frame3's width (512 in the reference)."""
    F = int(input_shape[-1])
    out = []
    cin = F
    if use_conv2d:
        c = 1
        for l, f in enumerate(filters, start=1):
            n = "conv2d_%d" % l
            out += [(n + ".W", (KERNEL[0], KERNEL[1], c, int(f)), True), (n + ".b", (int(f),), True)]
            out += [(n + "_bn." + v, (int(f),), v in ("gamma", "beta")) for v in ("gamma", "beta", "moving_mean", "moving_variance")]
            c = int(f)
        cin = c
    for i, (u, (k, _)) in enumerate(zip(frame_units, FRAME_KERNELS)):
        n = "frame%d" % (i + 1)
        out += [(n + ".W", (k, cin, int(u)), True), (n + ".b", (int(u),), True)]
        cin = int(u)
        if i == 2 and use_lstm:
            out += [("lstm.W", (cin, 4 * cin), True), ("lstm.U", (cin, 4 * cin), True), ("lstm.b", (4 * cin,), True)]
    if use_attention:
        out += [("Wf_1.W", (cin, ATTENTION_D_A), True), ("Wf_2.W", (ATTENTION_D_A, ATTENTION_D_F), True)]
    din = 2 * cin
    for j, u in enumerate(segment_units, start=1):
        out += [("segment%d.W" % j, (din, int(u)), True), ("segment%d.b" % j, (int(u),), True)]
        din = int(u)
    out += [("output.W", (din, int(num_outputs)), True), ("output.b", (int(num_outputs),), True)]
    return out


def count_params(*args, **kwargs):
    """Keras `Model.count_params()` of the model keras_layout describes (moving statistics included)"""
    return sum(int(np.prod(s)) for _, s, _ in keras_layout(*args, **kwargs))


def _check_args(input_shape, compute_dtype, use_attention, use_conv2d, filters, frame_units, segment_units):
    if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
        raise ValueError("clstm computes in float32 only, got compute_dtype=%r" % (compute_dtype,))
    if len(input_shape) != 2 or input_shape[1] is None:
        raise ValueError("input_shape must be (T, F) with F known (clstm.py:49), got %r" % (tuple(input_shape),))
    if len(frame_units) != 5 or len(segment_units) != 2 or len(filters) != 2:
        raise ValueError("frame_units: five widths, segment_units: two, filters: two")
    if use_attention and frame_units[4] % ATTENTION_D_F:
        # clstm.py:32
        raise ValueError("amount of frequency channels (%d) must be evenly divisible by the amount of frequency attention "
                         "bins (d_f=%d)" % (frame_units[4], ATTENTION_D_F))
    if use_conv2d and any(int(f) % 16 for f in filters):
        raise ValueError("conv2d filters must be multiples of 16, got %r" % (tuple(filters),))


class _Workspace(_TDNNWorkspace):
    """SequentialTDNN's buffers plus those of the 2-D front-end and the LSTM"""

    def __init__(self, model, B, T):
        super().__init__(model, B, T)
        model._extend_workspace(self)


class CLSTM(SequentialTDNN):
    """The reference's CLSTM on SequentialTDNN (see the module docstring)."""

    workspace_class = _Workspace
    unit_forget_biases = frozenset(["lstm.b"])
    _init_weights = FlatParams._init_weights          # the Keras defaults of every layer kind, not just SequentialTDNN's

    def __init__(self, input_shape, num_outputs, output_activation="log_softmax", use_attention=False, use_conv2d=False,
                 use_lstm=False, seed=None, device=None, compute_dtype="float32", filters=FILTERS, frame_units=FRAME_UNITS,
                 segment_units=SEGMENT_UNITS):
        _check_args(input_shape, compute_dtype, use_attention, use_conv2d, filters, frame_units, segment_units)
        T, F = input_shape[0], int(input_shape[1])
        self.use_attention, self.use_conv2d, self.use_lstm = bool(use_attention), bool(use_conv2d), bool(use_lstm)
        self.filters = tuple(int(f) for f in filters)
        self.fe_geom = conv2d_taps(F) if self.use_conv2d else []
        self.lstm_units = int(frame_units[2])
        convs = [frame_layer(int(u), k, s, name="frame%d" % (i + 1)) for i, (u, (k, s)) in enumerate(zip(frame_units, FRAME_KERNELS))]
        denses = [segment_layer(int(u), name="segment%d" % j) for j, u in enumerate(segment_units, start=1)]
        denses.append(DenseSpec("output", num_outputs, relu=False))
        att = FreqAttentionSpec(d_a=ATTENTION_D_A, d_f=ATTENTION_D_F) if self.use_attention else None
        c0 = self.filters[-1] if self.use_conv2d else F
        super().__init__((T, c0), convs, "stats", denses, name="CLSTM", output_activation=output_activation or None,
                         channel_dropout_rate=DROPOUT_RATE, seed=seed, device=device, compute_dtype="float32", attention=att)
        self.model_input_dim = F
        self.input_noise_stddev = NOISE_STDDEV          # the Trainer's cue for lidbox_input_noise_dropout
        # the Keras layout in the bucket-safe order (module docstring) replaces the plain x-vector one
        self.new_layout()
        for name, shape, trainable in keras_layout(input_shape, num_outputs, use_attention, use_conv2d, use_lstm, filters,
                                                   frame_units, segment_units):
            (self.add_param if trainable else self.add_state)(name, shape)
        self.allocate()
        self._init_weights(seed)
        self.fe_bns = [BatchNormSpec("conv2d_%d_bn" % l, BN_MOMENTUM, BN_EPSILON) for l in (1, 2)]

    # ------------------------------------------------------------------ workspace
    def _extend_workspace(self, ws):
        dev, B, T = self.device, ws.B, ws.T
        f32 = dict(dtype=torch.float32, device=dev)
        g = self.gemm
        gws = 16
        if self.use_conv2d:
            (F0, F1, tp1), (_, F2, tp2) = self.fe_geom
            C1, C2 = self.filters
            ws.fe_in = torch.zeros((B, T, F0), **f32)          # the model input (ws.input_view())
            ws.dact[0] = torch.zeros_like(ws.act[0])           # frame1's dgrad: the gradient of the front-end output
            ws.cv_y = [torch.zeros((B, T, F1, C1), **f32), torch.zeros((B, T, F2, C2), **f32)]    # conv outputs
            ws.cv_a1 = torch.zeros((B, T, F1, C1), **f32)      # relu(bn(conv2d_1)): conv2d_2's input
            ws.cv_c = [torch.zeros((4, C1), **f32), torch.zeros((4, C2), **f32)]                   # mean, invstd, scale, shift
            ws.cv_dbn = [torch.zeros_like(y) for y in ws.cv_y]  # gradient of each BatchNormalization output
            ws.cv_dz = [torch.zeros_like(y) for y in ws.cv_y]   # gradient of each conv output
            R1, R2 = B * T * F1, B * T * F2
            ws.bn_ws = torch.empty(max(16, nv.lib.lidbox_bn_workspace(max(R1, 1), C1), nv.lib.lidbox_bn_workspace(max(R2, 1), C2)),
                                   dtype=torch.uint8, device=dev)
            ws.cv_dgrad_ws = torch.empty(max(16, nv.lib.lidbox_conv2d_strided_dgrad_workspace(tp2, C1, C2)), dtype=torch.uint8, device=dev)
            wws = 16
            if B > 0:
                wws = max(wws, nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, F0, 1, C1, tp1),
                          nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, F1, C1, C2, tp2))
            ws.cv_wgrad_ws = torch.empty(wws, dtype=torch.uint8, device=dev)
            c1 = self.convs[0]
            if B * T > 0:
                gws = max(gws, g.rows_workspace(B * T, C2, c1.filters))
        if self.use_lstm:
            T3, H, C3 = ws.Ts[3], self.lstm_units, self.convs[2].filters
            R = B * T3
            ws.lstm_zg = torch.zeros((1, B, T3, 4 * H), **f32)
            ws.lstm_hseq = torch.zeros((B, T3 + 2, H), **f32)   # rows 0 and T3+1 stay zero
            ws.lstm_cseq = torch.zeros((1, B, T3, H), **f32)
            ws.lstm_dh = torch.zeros((B, T3, H), **f32)         # frame4's dgrad: the gradient of the h sequence
            ws.lstm_ws = torch.empty(max(16, nv.lib.lidbox_lstm_workspace(B, T3, H, 1)), dtype=torch.uint8, device=dev)
            if R > 0:
                gws = max(gws, g.rows_workspace(R, 4 * H, C3), g.rows_workspace(R, C3, 4 * H), g.tn_workspace(R, C3, 4 * H),
                          g.tn_workspace(R, H, 4 * H))
        ws.cl_gemm_ws = torch.empty(gws, dtype=torch.uint8, device=dev)

    def _cws(self, ws):
        return nv.ptr(ws.cl_gemm_ws), ws.cl_gemm_ws.numel()

    def _lstm(self, ws):
        T3, H, C3 = ws.Ts[3], self.lstm_units, self.convs[2].filters
        return LSTMLayer(["lstm"], _rows(ws.act[3].data_ptr(), 0, C3, 1, ws.B * T3), C3, ws.B, T3, H, ws.lstm_zg, ws.lstm_cseq,
                         ws.lstm_hseq.data_ptr(), H, ws.lstm_ws, ws.cl_gemm_ws, ws.cl_gemm_ws, gemm=self.gemm)

    def _conv_rows_in(self, ws, i):
        if i == 3 and self.use_lstm:        # frame4 (k 1, s 1) reads the LSTM's h sequence in place
            H, T3 = self.lstm_units, ws.Ts[3]
            return _rows(ws.lstm_hseq.data_ptr() + 4 * H, (T3 + 2) * H, H, ws.B, ws.Ts[4])
        return super()._conv_rows_in(ws, i)

    def _const_ptrs(self, c, C):
        return [ctypes.c_void_p(c.data_ptr() + 4 * j * C) for j in range(4)]

    # ------------------------------------------------------------------ forward
    def _before_conv(self, ws, i, training, update_moving):
        if i == 0 and self.use_conv2d:
            self._forward_conv2d(ws, training, update_moving)
        elif i == 3 and self.use_lstm:
            self._forward_lstm(ws)

    def _forward_conv2d(self, ws, training, update_moving):
        st, lib = nv.current_stream(), nv.lib
        B, T = ws.B, ws.T
        if B * T == 0:
            return
        x, cin = ws.fe_in, 1
        for l, (Fi, Fo, taps) in enumerate(self.fe_geom):
            name, C = "conv2d_%d" % (l + 1), self.filters[l]
            y, R = ws.cv_y[l], B * T * Fo
            nv.check(lib.lidbox_conv2d_strided_fwd(nv.ptr(x), B, T, Fi, cin, self._p(name + ".W"), taps, C, self._p(name + ".b"),
                                                   nv.ptr(y), st))
            cp = self._bn_fwd(self.fe_bns[l], y, R, C, ws.cv_c[l], None, ws, training, update_moving, bessel=None)
            if l == 0:
                nv.check(lib.lidbox_bn_relu_fwd(nv.ptr(y), R, C, cp[2], cp[3], nv.ptr(ws.cv_a1), st))
                x, cin = ws.cv_a1, C
            else:
                # reduce_max over frequency straight into frame1's input rows, behind its causal zero rows
                a0 = ws.act[0]
                nv.check(lib.lidbox_bn_relu_maxf_fwd(nv.ptr(y), B, T, Fo, C, cp[2], cp[3],
                                                     ctypes.c_void_p(a0.data_ptr() + 4 * ws.pads[0] * C), a0.shape[1] * C, st))

    def _forward_lstm(self, ws):
        if ws.B * ws.Ts[3] > 0:
            lstm_layer_fwd(self, self._lstm(ws))

    # ------------------------------------------------------------------ backward
    def backward_conv_ws(self, ws, i):
        if i == 3 and self.use_lstm:
            self._backward_frame4_lstm(ws)
            return
        super().backward_conv_ws(ws, i)
        if i == 0 and self.use_conv2d:
            self._backward_conv2d(ws)

    def _zero_grads(self, *names):
        for n in names:
            self.param(n, True).zero_()

    def _backward_frame4_lstm(self, ws):
        """frame4's wgrad and its dgrad into the h sequence's gradient (no ReLU in between), then the LSTM: the walk back,
        dW with db, dU, and dX into dact[3] masked by frame3's ReLU"""
        T3, H = ws.Ts[3], self.lstm_units
        c, C3, R = self.convs[3], self.convs[2].filters, ws.B * ws.Ts[3]
        if R == 0:
            self._zero_grads("frame4.W", "frame4.b", "lstm.W", "lstm.U", "lstm.b")
            return
        dy = self._rows_out(ws.dact[4], ws, 4)
        self._dgrad_wgrad(ws, dy, self._p(c.name + ".W"), c.filters, _rows(ws.lstm_dh.data_ptr(), 0, H, 1, R), c.filters, H,
                          nv.EPI_NONE, None, self._conv_rows_in(ws, 3), self._p(c.name + ".W", True), c.filters, H,
                          self._p(c.name + ".b", True))
        lstm_layer_bwd(self, self._lstm(ws), nv.ptr(ws.lstm_dh), T3 * H, H, dX=_rows(ws.dact[3].data_ptr(), 0, C3, 1, R),
                       dX_epi=(nv.EPI_RELU_MASK if self.convs[2].relu else nv.EPI_NONE,), dX_aux=nv.ptr(ws.act[3]))

    def _backward_conv2d(self, ws):
        """frame1's dgrad into the front-end output's gradient, then both Conv2D layers from the top down"""
        st, lib = nv.current_stream(), nv.lib
        B, T = ws.B, ws.T
        names = [("conv2d_%d" % l, "conv2d_%d_bn" % l) for l in (1, 2)]
        if B * T == 0:
            self._zero_grads(*[n + s for n, bn in names for s in (".W", ".b")], *[bn + s for n, bn in names for s in (".gamma", ".beta")])
            return
        gws, gws_n = self._cws(ws)
        c, d0 = self.convs[0], ws.dact[0]
        C2, Tp = self.filters[1], d0.shape[1]
        # frame1 (causal, k taps, stride 1): tap j adds dY[t] W[j]^T to padded row t + j; tap 0 overwrites rows [0, T)
        nv.check(lib.lidbox_zero_2d(ctypes.c_void_p(d0.data_ptr() + 4 * T * C2), 4 * Tp * C2, 4 * (Tp - T) * C2, B, st))
        dy = self._rows_out(ws.dact[1], ws, 1)
        for j in range(c.k):
            Wj = ctypes.c_void_p(self._p(c.name + ".W").value + 4 * j * C2 * c.filters)
            nv.check(self.gemm.nt(dy, Wj, c.filters, _rows(d0.data_ptr() + 4 * j * C2, Tp * C2, C2, B, T), c.filters, C2,
                                  nv.EPI_NONE if j == 0 else nv.EPI_ACCUM, None, gws, gws_n, st))
        (F0, F1, tp1), (_, F2, tp2) = self.fe_geom
        C1 = self.filters[0]
        (n1, _), (n2, _) = names
        c1, c2 = self._const_ptrs(ws.cv_c[0], C1), self._const_ptrs(ws.cv_c[1], C2)
        R1, R2 = B * T * F1, B * T * F2
        nv.check(lib.lidbox_bn_relu_maxf_bwd(nv.ptr(ws.cv_y[1]), B, T, F2, C2, c2[2], c2[3],
                                             ctypes.c_void_p(d0.data_ptr() + 4 * ws.pads[0] * C2), Tp * C2, nv.ptr(ws.cv_dbn[1]), st))
        self._bn_bwd(self.fe_bns[1], ws.cv_y[1], R2, C2, ws.cv_c[1], ws.cv_dbn[1], 0, ws.cv_dz[1], ws)
        wws, wws_n = nv.ptr(ws.cv_wgrad_ws), ws.cv_wgrad_ws.numel()
        nv.check(lib.lidbox_conv2d_strided_wgrad(nv.ptr(ws.cv_a1), nv.ptr(ws.cv_dz[1]), B, T, F1, C1, C2, tp2, self._p(n2 + ".W", True),
                                                 self._p(n2 + ".b", True), wws, wws_n, st))
        nv.check(lib.lidbox_conv2d_strided_dgrad(nv.ptr(ws.cv_dz[1]), B, T, F1, C1, C2, self._p(n2 + ".W"), tp2, nv.ptr(ws.cv_dbn[0]),
                                                 nv.ptr(ws.cv_dgrad_ws), ws.cv_dgrad_ws.numel(), st))
        nv.check(lib.lidbox_bn_relu_bwd(nv.ptr(ws.cv_y[0]), R1, C1, c1[2], c1[3], nv.ptr(ws.cv_dbn[0]), nv.ptr(ws.cv_dbn[0]), st))
        self._bn_bwd(self.fe_bns[0], ws.cv_y[0], R1, C1, ws.cv_c[0], ws.cv_dbn[0], 0, ws.cv_dz[0], ws)
        nv.check(lib.lidbox_conv2d_strided_wgrad(nv.ptr(ws.fe_in), nv.ptr(ws.cv_dz[0]), B, T, F0, 1, C1, tp1, self._p(n1 + ".W", True),
                                                 self._p(n1 + ".b", True), wws, wws_n, st))

    # ------------------------------------------------------------ ragged pass (inference, float32; models/ragged_pass.py)
    def ragged_refusal(self):
        """None for every flag combination: this module runs what SequentialTDNN's ragged pass leaves out (the 2-D front-end,
        the LSTM between frame3 and frame4, the frequency attention)"""
        return None

    def _ragged_plan(self, ro, lengths):
        """use_lstm: level 3 carries a pad row before and after each utterance's frames, for the LSTM that runs there in place"""
        plan = ragged_plan(lengths, self.convs, {3: (1, 1)} if self.use_lstm else None)
        return plan, dict(rows=int(plan.off[-1]), B=plan.B, frames=int(ro[-1]))

    def _ragged_buffers_rows(self, cap):
        """SequentialTDNN's levels plus, per row of level 3, the LSTM's buffers and, per row of the pooling level, the
        attention's"""
        f32 = dict(dtype=torch.float32, device=self.device)
        bufs = super()._ragged_buffers_rows(cap)
        if self.use_lstm:
            H, R3 = self.lstm_units, bufs["act"][3].shape[0]
            # lstm_hseq: frame4's windows start one row on, hence one row behind the last
            bufs.update(zg=torch.zeros(R3 * 4 * H, **f32), cseq=torch.zeros(R3 * H, **f32), lstm_hseq=torch.zeros((R3 + 1, H), **f32))
        if self.attention is not None:
            att, last = self.attention, bufs["act"][-1]
            bufs.update(fa_x1=torch.zeros((last.shape[0], att.d_a), **f32), fa_F=torch.zeros((last.shape[0], att.d_f), **f32),
                        hw=torch.zeros_like(last))
        return bufs

    def _ragged_buffers_frames(self, cap):
        """per input frame: the 2-D front-end's buffers (none without use_conv2d)"""
        if not self.use_conv2d:
            return {}
        f32 = dict(dtype=torch.float32, device=self.device)
        (_, F1, _), (_, F2, _) = self.fe_geom
        C1, C2 = self.filters
        return dict(cv_y=[torch.zeros((cap, F1, C1), **f32), torch.zeros((cap, F2, C2), **f32)], cv_a1=torch.zeros((cap, F1, C1), **f32),
                    cv_out=torch.zeros((cap, C2), **f32), cv_c=[torch.zeros((4, C1), **f32), torch.zeros((4, C2), **f32)])

    def _ragged_conv2d(self, ws, X, dev_ro, B, total_T):
        """the 2-D front-end over all frames: both strided convolutions on each utterance's own rows
        (lidbox_conv2d_strided_ragged_fwd), BatchNormalization + ReLU and + max over frequency row-wise; returns [total_T, C2]"""
        st, lib = nv.current_stream(), nv.lib
        x, cin = X, 1
        for l, (Fi, Fo, taps) in enumerate(self.fe_geom):
            name, C = "conv2d_%d" % (l + 1), self.filters[l]
            y = ws.cv_y[l]
            nv.check(lib.lidbox_conv2d_strided_ragged_fwd(nv.ptr(x), dev_ro, B, total_T, Fi, cin, self._p(name + ".W"), taps, C,
                                                          self._p(name + ".b"), nv.ptr(y), st))
            cp = self._bn_fwd(self.fe_bns[l], None, 0, C, ws.cv_c[l], None, ws, False, False)
            if l == 0:
                nv.check(lib.lidbox_bn_relu_fwd(nv.ptr(y), total_T * Fo, C, cp[2], cp[3], nv.ptr(ws.cv_a1), st))
                x, cin = ws.cv_a1, C
            else:
                nv.check(lib.lidbox_bn_relu_maxf_fwd(nv.ptr(y), 1, total_T, Fo, C, cp[2], cp[3], nv.ptr(ws.cv_out), total_T * C, st))
        return ws.cv_out

    def _ragged_pass(self, ws, plan, X, ro, upto_embedding):
        """SequentialTDNN's ragged pass for every flag combination, built from its helpers.  X [total_T, F] (F: the model's
        input features).  use_conv2d: the front-end runs on [total_T, ...] and its output is packed into level 0; use_lstm: the
        LSTM runs on level 3 (its pad rows: `_ragged_plan`) on lidbox_lstm_ragged_fwd and frame4 reads its h sequence;
        use_attention: lidbox_freq_attention_fwd over the rows of the pooling level."""
        st, lib, g = nv.current_stream(), nv.lib, self.gemm
        B, n, H, att = plan.B, len(self.convs), self.lstm_units, self.attention
        R3, C3, Rn, Cn = plan.rows[3], ws.act[3].shape[1], plan.rows[n], ws.act[n].shape[1]
        need = self._ragged_gemm_need(ws, plan)
        if self.use_lstm:
            need = max(need, g.rows_workspace(R3, 4 * H, C3))
        if att is not None:
            need = max(need, g.rows_workspace(Rn, att.d_a, Cn), g.rows_workspace(Rn, att.d_f, att.d_a))
        ws.reserve_gemm_ws(self, need)
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        # the LSTM's walk over the segments of level 3; its slot table goes behind SequentialTDNN's in the one upload
        rp = recurrent_plan(plan.T[3], plan.seg_offsets(3)) if self.use_lstm else None
        table, seg = self._ragged_upload(plan, ro, [rp.slots()] if rp else [])
        self._ragged_pack(ws, plan, seg, self._ragged_conv2d(ws, X, seg[n + 1], B, int(ro[-1])) if self.use_conv2d else X)
        for i in range(n):
            A = None
            if i == 3 and rp:
                # the LSTM on level 3 in place: one projection over all its rows, the walk over each utterance's own frames
                # (segment b: a pad row, its frames, a pad row at least), then frame4 on the h sequence, one row on
                nv.check(g.nn(_rows(ws.act[3].data_ptr(), 0, C3, 1, R3), self._p("lstm.W"), 4 * H,
                              _rows(ws.zg.data_ptr(), 0, 4 * H, 1, R3), C3, 4 * H, nv.EPI_BIAS, self._p("lstm.b"), gws, gws_n, st))
                nv.check(lib.lidbox_lstm_ragged_fwd(self._p("lstm.U"), None, 1, B, H, R3, seg[n + 3],
                                                    ctypes.c_void_p(rp.sorted_lengths.ctypes.data), nv.ptr(ws.zg),
                                                    nv.ptr(ws.lstm_hseq), H, nv.ptr(ws.cseq), None, st))
                A = _rows(ws.lstm_hseq.data_ptr() + 4 * plan.lead[3] * H, 0, self.convs[3].s * H, 1, plan.rows[4] - plan.pads[4])
            self._ragged_conv(ws, plan, seg, i, A)
        last = ws.act[n]
        if att is not None:
            nv.check(g.nn(_rows(last.data_ptr(), 0, Cn, 1, Rn), self._p("Wf_1.W"), att.d_a,
                          _rows(ws.fa_x1.data_ptr(), 0, att.d_a, 1, Rn), Cn, att.d_a, nv.EPI_RELU, None, gws, gws_n, st))
            nv.check(g.nn(_rows(ws.fa_x1.data_ptr(), 0, att.d_a, 1, Rn), self._p("Wf_2.W"), att.d_f,
                          _rows(ws.fa_F.data_ptr(), 0, att.d_f, 1, Rn), att.d_a, att.d_f, nv.EPI_NONE, None, gws, gws_n, st))
            nv.check(lib.lidbox_freq_attention_fwd(nv.ptr(last), nv.ptr(ws.fa_F), Rn, Cn, att.d_f, nv.ptr(ws.fa_F), nv.ptr(ws.hw), st))
            last = ws.hw
        return self._ragged_pool_head(ws, plan, seg, upto_embedding, last)

    # ------------------------------------------------------------------ public call
    def _load_input(self, ws, x, training):
        """copy x into the model input; in training, GaussianNoise + channel Dropout in place (eager calls key the draws on a
        host-side call counter; the captured train step keys them on the device-side optimizer step)"""
        super()._load_input(ws, x, False)
        if training:
            self._dropout_calls += 1
            in_ptr, in_bs, T, C = ws.input_target()
            nv.check(nv.lib.lidbox_input_noise_dropout(in_ptr, ws.B, T, C, in_bs, self.input_noise_stddev, self.channel_dropout_rate,
                                                       (self.dropout_seed + 0x51ED27 * self._dropout_calls) & (2 ** 64 - 1), None,
                                                       nv.current_stream()))


def create(input_shape, num_outputs, output_activation="log_softmax", use_attention=False, use_conv2d=False, use_lstm=False,
           seed=None, device=None, compute_dtype="float32", filters=FILTERS, frame_units=FRAME_UNITS, segment_units=SEGMENT_UNITS):
    """reference clstm.py:45-81.  input_shape (T, F) with F known.  output_activation: "log_softmax" (the reference's
    default), "softmax" or None.  filters / frame_units / segment_units: the reference's widths by default; smaller values
    serve tests (the LSTM takes frame3's width, 512 in the reference)."""
    _check_args(input_shape, compute_dtype, use_attention, use_conv2d, filters, frame_units, segment_units)
    return CLSTM(input_shape, num_outputs, output_activation=output_activation, use_attention=use_attention,
                 use_conv2d=use_conv2d, use_lstm=use_lstm, seed=seed, device=device, compute_dtype=compute_dtype, filters=filters,
                 frame_units=frame_units, segment_units=segment_units)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`
