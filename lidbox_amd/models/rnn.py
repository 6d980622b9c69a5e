"""
Recurrent engine: the host-side orchestration shared by `lidbox_amd.models.lstm` and `lidbox_amd.models.ap_lstm`.

A model is  [SpatialDropout1D]  ->  LSTM / Bidirectional(LSTM) layers  ->  a head:
  * "last": the last layer's final h -> Dense -> output activation (reference lidbox/models/lstm.py:14-20);
  * "avg_concat": each BLSTM's output sequence, scaled by its alpha, averaged over time into its half of the pooled
    vector (ap_lstm.py:37-41; the Concatenate is folded into where each half lands).  The model output is that vector
    L2-normalised (ap_lstm.py:42); the train step hands the un-normalised vector to the angular-proximity head, which
    normalises it itself (normalising twice is the identity).

The scaffolding is `lidbox_amd.models.flat`'s; every LSTM layer is its lstm_layer_fwd / lstm_layer_bwd on the
lidbox_lstm_fwd / _bwd walk (csrc/rnn.hip).  Parameter names follow the Keras layer names (`lstm.W`, `forward_lstm_1.U`,
`backward_lstm_1.b`, `output.W`).
"""
import ctypes

import torch

from .. import _native as nv
from .flat import FlatModel, LSTMLayer, Workspace, _rows, lstm_layer_bwd, lstm_layer_fwd, orthogonal
from .rnn_ragged import RaggedRecurrent
from .tdnn import DenseSpec


class LSTMSpec:
    """tf.keras.layers.LSTM(units, return_sequences), optionally wrapped in Bidirectional(merge_mode="concat").
    name: the Keras name of the LSTM layer itself (`lstm`, `lstm_1`); a Bidirectional wrapper names its halves
    `forward_<name>` / `backward_<name>`."""

    def __init__(self, name, units, bidirectional=False, return_sequences=True, wrapper=None):
        self.name, self.units = name, int(units)
        self.bidirectional, self.return_sequences = bool(bidirectional), bool(return_sequences)
        self.wrapper = wrapper or name
        self.dirs = 2 if self.bidirectional else 1
        self.prefixes = ["forward_" + name, "backward_" + name] if self.bidirectional else [name]

    @property
    def out_dim(self):
        return self.dirs * self.units


class _Workspace(Workspace):
    """All per-(B, T) device buffers of one recurrent model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.T = B, T
        self.x = torch.zeros((B, T, model.input_dim), **f32)
        self.zg, self.hseq, self.cseq, self.dseq = [], [], [], []
        lws = 0
        gws = 0
        tws = 16
        cin = model.input_dim
        for l in model.lstms:
            H, dirs = l.units, l.dirs
            self.zg.append(torch.zeros((dirs, B, T, 4 * H), **f32))
            self.hseq.append(torch.zeros((B, T + 2, dirs * H), **f32))          # rows 0 and T+1 stay zero
            self.cseq.append(torch.zeros((dirs, B, T, H), **f32))
            self.dseq.append(torch.zeros((B, T, dirs * H), **f32) if l.return_sequences else None)
            lws = max(lws, nv.lib.lidbox_lstm_workspace(B, T, H, dirs))
            gws = max(gws, nv.lib.lidbox_gemm_rows_workspace(B * T, 4 * H, cin), nv.lib.lidbox_gemm_rows_workspace(B * T, cin, 4 * H))
            tws = max(tws, nv.lib.lidbox_gemm_tn_workspace(B * T, cin, 4 * H), nv.lib.lidbox_gemm_tn_workspace(B * T, H, 4 * H))
            cin = dirs * H
        last = model.lstms[-1]
        self.dlast = torch.zeros((B, last.out_dim), **f32)
        if model.head == "avg_concat":
            D = model.output_dim
            self.h = [torch.zeros((B, D), **f32)]
            self.dh = [torch.zeros((B, D), **f32)]
        else:
            x_dim = last.out_dim
            for d in model.denses:
                gws = max(gws, nv.lib.lidbox_gemm_rows_workspace(B, d.units, x_dim), nv.lib.lidbox_gemm_rows_workspace(B, x_dim, d.units))
                tws = max(tws, nv.lib.lidbox_gemm_tn_workspace(B, x_dim, d.units))
                x_dim = d.units
            self.h = [torch.zeros((B, d.units), **f32) for d in model.denses]
            self.dh = [torch.zeros((B, d.units), **f32) for d in model.denses]
        self.logp = torch.zeros_like(self.h[-1])
        self.out = torch.zeros_like(self.h[-1])                   # the L2-normalised model output (avg_concat)
        self.loss = torch.zeros(4, **f32)
        self.lstm_ws = torch.empty(max(16, lws), dtype=torch.uint8, device=dev)
        self.gemm_ws = torch.empty(max(16, gws), dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.pending = []


class RecurrentModel(FlatModel, RaggedRecurrent):
    """[SpatialDropout1D] -> LSTM layers -> head, parameters in one flat buffer (see the module docstring)."""

    workspace_class = _Workspace

    def __init__(self, input_shape, lstms, head, denses=(), name="rnn", output_activation="log_softmax",
                 channel_dropout_rate=0.0, alphas=None, seed=None, device=None, compute_dtype="float32"):
        super().__init__(input_shape, name, output_activation, seed, device, compute_dtype, channel_dropout_rate)
        if head not in ("last", "avg_concat"):
            raise ValueError("head must be 'last' or 'avg_concat'")
        self.lstms, self.head, self.denses = list(lstms), head, list(denses)
        if head == "last" and (self.lstms[-1].return_sequences or not self.denses):
            raise ValueError("a 'last' head reads the final h of an LSTM with return_sequences=False into Dense layers")
        if head == "last" and self.lstms[-1].bidirectional:
            raise ValueError("a 'last' head reads a forward-only LSTM")
        if head == "avg_concat" and (self.denses or not all(l.return_sequences for l in self.lstms)):
            raise ValueError("an 'avg_concat' head pools the output sequences of every LSTM layer and has no Dense layer")
        self.alphas = [float(a) for a in (alphas or [1.0] * len(self.lstms))]
        cin = self.input_dim
        for l in self.lstms:
            for p in l.prefixes:
                self.add_param(p + ".W", (cin, 4 * l.units))
                self.add_param(p + ".U", (l.units, 4 * l.units))
                self.add_param(p + ".b", (4 * l.units,))
            cin = l.out_dim
        for d in self.denses:
            self.add_param(d.name + ".W", (cin, d.units))
            self.add_param(d.name + ".b", (d.units,))
            cin = d.units
        self.output_dim = cin if head == "last" else sum(l.out_dim for l in self.lstms)
        self.unit_forget_biases = {p + ".b" for l in self.lstms for p in l.prefixes}
        self._finish(seed)

    def _in_rows(self, ws, i):
        """(rows descriptor, K) of layer i's input: the model input, or rows 1..T of the previous layer's h sequence"""
        B, T = ws.B, ws.T
        if i == 0:
            return _rows(ws.x.data_ptr(), 0, self.input_dim, 1, B * T), self.input_dim
        prev = self.lstms[i - 1]
        hs = ws.hseq[i - 1]
        return _rows(hs.data_ptr() + 4 * prev.out_dim, (T + 2) * prev.out_dim, prev.out_dim, B, T), prev.out_dim

    def _out_seq_rows(self, ws, i):
        l = self.lstms[i]
        return ws.hseq[i].data_ptr() + 4 * l.out_dim, (ws.T + 2) * l.out_dim, l.out_dim

    def _last_rows(self, ws):
        """final h of the last (return_sequences=False, forward-only) layer: row T of its h sequence"""
        l = self.lstms[-1]
        return _rows(ws.hseq[-1].data_ptr() + 4 * ws.T * l.out_dim, (ws.T + 2) * l.out_dim, 0, ws.B, 1)

    def _layer(self, ws, i):
        l = self.lstms[i]
        X, K = self._in_rows(ws, i)
        return LSTMLayer(l.prefixes, X, K, ws.B, ws.T, l.units, ws.zg[i], ws.cseq[i], ws.hseq[i].data_ptr(), l.out_dim,
                         ws.lstm_ws, ws.gemm_ws, ws.tn_ws)

    # ------------------------------------------------------------------ forward
    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False):
        """The model input buffer (ws.input_view()) must already hold the input.  Returns the model output before its
        output activation's normalisation for 'avg_concat' (normalize=True: the L2-normalised output), the log-probs /
        probabilities / logits of a 'last' head otherwise."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        for i in range(len(self.lstms)):
            lstm_layer_fwd(self, self._layer(ws, i))
        if self.head == "avg_concat":
            out = ws.h[-1]
            col = 0
            for i, l in enumerate(self.lstms):
                base, bs, rs = self._out_seq_rows(ws, i)
                nv.check(lib.lidbox_seq_avg_pool_fwd(ctypes.c_void_p(base), B, T, l.out_dim, bs, rs, self.alphas[i],
                                                     ctypes.c_void_p(out.data_ptr() + 4 * col), self.output_dim, st))
                col += l.out_dim
            if normalize:
                nv.check(lib.lidbox_l2_normalize_fwd(nv.ptr(out), B, self.output_dim, nv.ptr(ws.out), st))
                return ws.out
            return out
        return self._forward_dense_head(ws, self._last_rows(ws), stop_before_output)

    def _forward_dense_head(self, ws, x, stop_before_output=False):
        """the Dense layers and the output activation of a 'last' head on x, the rows descriptor of the ws.B final states (the
        dense and the ragged pass share it)"""
        st, lib, B = nv.current_stream(), nv.lib, ws.B
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        din = self.lstms[-1].out_dim
        for j, d in enumerate(self.denses):
            if stop_before_output and j == len(self.denses) - 1:
                return x
            nv.check(lib.lidbox_gemm_nn(x, self._p(d.name + ".W"), d.units, _rows(ws.h[j].data_ptr(), 0, d.units, 1, B), din,
                                        d.units, nv.EPI_BIAS_RELU if d.relu else nv.EPI_BIAS, self._p(d.name + ".b"),
                                        gws, gws_n, st))
            x, din = _rows(ws.h[j].data_ptr(), 0, d.units, 1, B), d.units
        return self._output_activation(ws, ws.h[-1], din)

    # ------------------------------------------------------------------ ragged pass (inference, float32; models/rnn_ragged.py)
    def _ragged_embedding_dim(self):
        """'last': the final h, the output layer's input; 'avg_concat': the language vector, which is the model output"""
        return self.lstms[-1].out_dim if self.head == "last" else self.output_dim

    def _ragged_buffers_rows(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        H, dirs = max(l.units for l in self.lstms), max(l.dirs for l in self.lstms)
        return dict(x=torch.zeros((cap, self.input_dim), **f32), zg=torch.zeros(dirs * cap * 4 * H, **f32),
                    cseq=torch.zeros(dirs * cap * H, **f32), hseq=[torch.zeros((cap, l.out_dim), **f32) for l in self.lstms])

    def _ragged_buffers_B(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        if self.head == "avg_concat":
            h = [torch.zeros((cap, self.output_dim), **f32)]
        else:
            h = [torch.zeros((cap, d.units), **f32) for d in self.denses]
        return dict(hlast=torch.zeros((cap, self.lstms[-1].out_dim), **f32), h=h, logp=torch.zeros_like(h[-1]),
                    out=torch.zeros_like(h[-1]))

    def _forward_ragged(self, ws, plan, dev, upto_embedding):
        """every LSTM layer on the ragged walk (lidbox_lstm_ragged_fwd, whatever H), then the head: the final h of every
        utterance into the Dense layers, or the alpha-scaled time averages over each utterance's own frames, L2-normalised"""
        st, lib, B, Rp = nv.current_stream(), nv.lib, plan.B, plan.Rp
        X, K = _rows(ws.x.data_ptr(), 0, self.input_dim, 1, Rp), self.input_dim
        for i, l in enumerate(self.lstms):
            hs = ws.hseq[i]
            hs[:Rp].zero_()                                   # the pad rows: the next layer's projection reads every row
            last = self.head == "last" and i == len(self.lstms) - 1
            self._ragged_lstm_layer(ws, plan, dev, X, K, l.prefixes, l.units, hs.data_ptr(), l.out_dim, ws.hlast if last else None)
            X, K = _rows(hs.data_ptr(), 0, l.out_dim, 1, Rp), l.out_dim
        if self.head == "avg_concat":
            out, col = ws.h[-1], 0
            for i, l in enumerate(self.lstms):
                nv.check(lib.lidbox_seq_avg_pool_ragged_fwd(nv.ptr(ws.hseq[i]), l.out_dim, dev.first, dev.lengths, B, l.out_dim,
                                                            self.alphas[i], ctypes.c_void_p(out.data_ptr() + 4 * col),
                                                            self.output_dim, st))
                col += l.out_dim
            nv.check(lib.lidbox_l2_normalize_fwd(nv.ptr(out), B, self.output_dim, nv.ptr(ws.out), st))
            return ws.out
        if upto_embedding:
            return ws.hlast
        need = 16
        din = self.lstms[-1].out_dim
        for d in self.denses:
            need, din = max(need, lib.lidbox_gemm_rows_workspace(B, d.units, din)), d.units
        ws.reserve_gemm_ws(self, need)
        return self._forward_dense_head(ws, _rows(ws.hlast.data_ptr(), 0, self.lstms[-1].out_dim, 1, B))

    # ------------------------------------------------------------------ backward
    def backward_head_ws(self, ws):
        """the whole backward pass: head, then every LSTM layer from the top down"""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        ws.pending = []
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        tws, tws_n = nv.ptr(ws.tn_ws), ws.tn_ws.numel()
        if B == 0:
            return
        if self.head == "avg_concat":
            col = 0
            for i, l in enumerate(self.lstms):
                nv.check(lib.lidbox_seq_avg_pool_bwd(ctypes.c_void_p(ws.dh[-1].data_ptr() + 4 * col), self.output_dim, B, T,
                                                     l.out_dim, self.alphas[i], nv.ptr(ws.dseq[i]), T * l.out_dim, l.out_dim, 0, st))
                col += l.out_dim
        else:
            for j in range(len(self.denses) - 1, -1, -1):
                d = self.denses[j]
                x = self._last_rows(ws) if j == 0 else _rows(ws.h[j - 1].data_ptr(), 0, self.denses[j - 1].units, 1, B)
                din = self.lstms[-1].out_dim if j == 0 else self.denses[j - 1].units
                dy = _rows(ws.dh[j].data_ptr(), 0, d.units, 1, B)
                nv.check(lib.lidbox_gemm_tn(x, dy, self._p(d.name + ".W", True), d.units, din, d.units, 0,
                                            self._p(d.name + ".b", True), tws, tws_n, st))
                dst = ws.dlast if j == 0 else ws.dh[j - 1]
                relu_prev = j > 0 and self.denses[j - 1].relu
                epi, aux = (nv.EPI_RELU_MASK, nv.ptr(ws.h[j - 1])) if relu_prev else (nv.EPI_NONE, None)
                nv.check(lib.lidbox_gemm_nt(dy, self._p(d.name + ".W"), d.units, _rows(dst.data_ptr(), 0, din, 1, B), d.units, din,
                                            epi, aux, gws, gws_n, st))
        for i in range(len(self.lstms) - 1, -1, -1):
            l, layer = self.lstms[i], self._layer(ws, i)
            # dX of layer i = the gradient of layer i-1's output sequence (on top of its pooled share, if any)
            dX = _rows(ws.dseq[i - 1].data_ptr(), 0, layer.K, 1, B * T) if i > 0 else None
            lstm_layer_bwd(self, layer, nv.ptr(ws.dseq[i]), T * l.out_dim, l.out_dim,
                           dh_last=None if l.return_sequences else nv.ptr(ws.dlast), dX=dX,
                           dX_epi=(nv.EPI_ACCUM if self.head == "avg_concat" else nv.EPI_NONE, nv.EPI_ACCUM))


__all__ = ["LSTMSpec", "DenseSpec", "RecurrentModel", "orthogonal"]
