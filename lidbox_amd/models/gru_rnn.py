"""
GRU engine: the host-side orchestration of `lidbox_amd.models.bi_gru`, the GRU twin of `lidbox_amd.models.rnn`.

A model is  [SpatialDropout1D]  ->  GRU / Bidirectional(GRU) layers  ->  the last layer's final state (both directions
concatenated, forward t = T-1 and backward t = 0)  ->  [BatchNormalization]  ->  Dense layers, each optionally followed by
BatchNormalization  ->  output activation (reference lidbox/models/bi_gru.py:26-48).

The scaffolding is `lidbox_amd.models.flat`'s.  Per GRU layer and direction: the input
projection X W + b_in of all B*T rows is one lidbox_gemm_nn; the walk through time is lidbox_gru_fwd / _bwd (csrc/gru.hip, one
launch per step for both directions); dW = X^T dZx (with db_in), dU = H_prev^T dZrec (with db_rec, in two column blocks:
dZrec's h block lives in qh) and dX = dZx W^T are GEMMs.

BatchNormalization here sees 2-D inputs [B, C], so it follows tf.keras' non-fused path: normalise with the batch mean and
population variance, move the running variance towards the population variance (lidbox_bn_train_stats_ex, bessel = 0).  The
moving statistics live in `state` / `state_layout` and move only when `update_moving` (not in the Trainer's warm-up pass), as
in `lidbox_amd.models.xvector_2d`.

Keras layouts of a GRU: kernel W [C, 3H], recurrent_kernel U [H, 3H], bias b [2, 3H] (input bias, recurrent bias), gate
order z, r, h.  A Bidirectional wrapper's halves are named by wrapper and direction (`BGRU_1_forward.W`, `BGRU_1_backward.U`),
not by Keras' session-dependent inner names; Dense and BatchNormalization layers keep their Keras names (`fc_relu_1.W`,
`BGRU_2_bn.gamma`, `BGRU_2_bn.moving_variance`).
"""
import ctypes

import torch

from .. import _native as nv
from .flat import BatchNormSpec, FlatModel, Workspace, _rows, h_neighbour_rows
from .rnn_ragged import RaggedRecurrent
from .tdnn import DenseSpec


class GRUSpec:
    """tf.keras.layers.GRU(units, return_sequences) with the TF2 defaults, optionally wrapped in
    Bidirectional(merge_mode="concat").  name: the wrapper's Keras name (`BGRU_1`), which also names the halves."""

    def __init__(self, name, units, bidirectional=False, return_sequences=True):
        self.name, self.units = name, int(units)
        self.bidirectional, self.return_sequences = bool(bidirectional), bool(return_sequences)
        self.dirs = 2 if self.bidirectional else 1
        self.prefixes = [name + "_forward", name + "_backward"] if self.bidirectional else [name]

    @property
    def out_dim(self):
        return self.dirs * self.units


class _Workspace(Workspace):
    """All per-(B, T) device buffers of one GRU model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
        self.B, self.T = B, T
        self.x = torch.zeros((B, T, model.input_dim), **f32)
        self.zg, self.hseq, self.qh, self.dseq = [], [], [], []
        rws, gws, tws = 16, 0, 16
        cin = model.input_dim
        for l in model.grus:
            H, dirs = l.units, l.dirs
            self.zg.append(torch.zeros((dirs, B, T, 3 * H), **f32))
            self.hseq.append(torch.zeros((B, T + 2, dirs * H), **f32))          # rows 0 and T+1 stay zero
            self.qh.append(torch.zeros((dirs, B, T, H), **f32))
            self.dseq.append(torch.zeros((B, T, dirs * H), **f32) if l.return_sequences else None)
            rws = max(rws, nv.lib.lidbox_gru_workspace(B, T, H, dirs))
            gws = max(gws, nv.lib.lidbox_gemm_rows_workspace(B * T, 3 * H, cin), nv.lib.lidbox_gemm_rows_workspace(B * T, cin, 3 * H))
            tws = max(tws, nv.lib.lidbox_gemm_tn_workspace(B * T, cin, 3 * H), nv.lib.lidbox_gemm_tn_workspace(B * T, H, 2 * H),
                      nv.lib.lidbox_gemm_tn_workspace(B * T, H, H))
            cin = dirs * H
        D = model.grus[-1].out_dim
        self.hlast = torch.zeros((B, D), **f32)
        self.dlast = torch.zeros((B, D), **f32)
        bws = 16
        # BatchNormalization after the recurrent part: its output / output gradient, per-channel constants
        # (mean, invstd, scale, shift)
        if model.rnn_bn is not None:
            self.y0 = torch.zeros((B, D), **f32)
            self.dy0 = torch.zeros((B, D), **f32)
            self.c0 = torch.zeros((4, D), **f32)
            bws = max(bws, nv.lib.lidbox_bn_workspace(B, D))
        # Dense j: h[j] its output (post-activation, pre-BatchNormalization), dh[j] the gradient of its pre-activation;
        # y[j] / dy[j] / c[j] of the BatchNormalization behind it (None without one)
        self.h, self.dh, self.y, self.dy, self.c = [], [], [], [], []
        x_dim = D
        for d, bn in zip(model.denses, model.dense_bns):
            gws = max(gws, nv.lib.lidbox_gemm_rows_workspace(B, d.units, x_dim), nv.lib.lidbox_gemm_rows_workspace(B, x_dim, d.units))
            tws = max(tws, nv.lib.lidbox_gemm_tn_workspace(B, x_dim, d.units))
            self.h.append(torch.zeros((B, d.units), **f32))
            self.dh.append(torch.zeros((B, d.units), **f32))
            has = bn is not None
            self.y.append(torch.zeros((B, d.units), **f32) if has else None)
            self.dy.append(torch.zeros((B, d.units), **f32) if has else None)
            self.c.append(torch.zeros((4, d.units), **f32) if has else None)
            if has:
                bws = max(bws, nv.lib.lidbox_bn_workspace(B, d.units))
            x_dim = d.units
        self.emb = torch.zeros((B, model.denses[0].units), **f32)
        self.logp = torch.zeros_like(self.h[-1])
        self.loss = torch.zeros(4, **f32)
        self.gru_ws = torch.empty(rws, dtype=torch.uint8, device=dev)
        self.gemm_ws = torch.empty(max(16, gws), dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.bn_ws = torch.empty(bws, dtype=torch.uint8, device=dev)
        self.pending = []


class GRUModel(FlatModel, RaggedRecurrent):
    """[SpatialDropout1D] -> GRU layers -> final state -> [BatchNormalization] -> Dense [+ BatchNormalization] layers (see the
    module docstring)."""

    workspace_class = _Workspace

    def __init__(self, input_shape, grus, denses, rnn_bn=None, dense_bns=None, name="gru", output_activation="log_softmax",
                 channel_dropout_rate=0.0, seed=None, device=None, compute_dtype="float32"):
        super().__init__(input_shape, name, output_activation, seed, device, compute_dtype, channel_dropout_rate)
        self.grus, self.denses = list(grus), list(denses)
        if not self.denses or self.grus[-1].return_sequences or not all(l.return_sequences for l in self.grus[:-1]):
            raise ValueError("the last GRU returns its final state only, into Dense layers; the others return sequences")
        self.dense_bns = list(dense_bns) if dense_bns is not None else [None] * len(self.denses)
        if len(self.dense_bns) != len(self.denses) or self.dense_bns[-1] is not None:
            raise ValueError("dense_bns: one entry (BatchNormSpec or None) per Dense layer, None for the output layer")
        self.rnn_bn = rnn_bn
        cin = self.input_dim
        for l in self.grus:
            H = l.units
            for p in l.prefixes:
                self.add_param(p + ".W", (cin, 3 * H))
                self.add_param(p + ".U", (H, 3 * H))
                self.add_param(p + ".b", (2, 3 * H))
            cin = l.out_dim
        if rnn_bn is not None:
            self.add_bn(rnn_bn.name, cin)
        for d, bn in zip(self.denses, self.dense_bns):
            self.add_param(d.name + ".W", (cin, d.units))
            self.add_param(d.name + ".b", (d.units,))
            cin = d.units
            if bn is not None:
                self.add_bn(bn.name, cin)
        self.output_dim = cin
        self._finish(seed)

    def _b_rec(self, prefix, grad=False):
        """row 1 of the Keras bias [2, 3H]: the recurrent bias"""
        off, shape = self.layout[prefix + ".b"]
        return ctypes.c_void_p((self.flat_grad if grad else self.flat).data_ptr() + 4 * (off + shape[1]))

    def _in_rows(self, ws, i):
        """(rows descriptor, K) of layer i's input: the model input, or rows 1..T of the previous layer's h sequence"""
        B, T = ws.B, ws.T
        if i == 0:
            return _rows(ws.x.data_ptr(), 0, self.input_dim, 1, B * T), self.input_dim
        prev = self.grus[i - 1]
        return _rows(ws.hseq[i - 1].data_ptr() + 4 * prev.out_dim, (T + 2) * prev.out_dim, prev.out_dim, B, T), prev.out_dim

    def _U(self, l):
        return self._p(l.prefixes[0] + ".U"), (self._p(l.prefixes[1] + ".U") if l.dirs == 2 else None)

    # ------------------------------------------------------------------ forward
    def _head_input(self, ws, j):
        """the input tensor of Dense j"""
        if j == 0:
            return ws.hlast if self.rnn_bn is None else ws.y0
        return ws.h[j - 1] if self.dense_bns[j - 1] is None else ws.y[j - 1]

    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False, embedding=False):
        """The model input buffer (ws.input_view()) must already hold the input.  training selects batch statistics in the
        BatchNormalization layers (update_moving=False leaves the running statistics untouched).  Returns the log-probs /
        probabilities / logits (output_activation None); stop_before_output: the output layer's input; embedding: the first
        Dense layer's output without its activation (as_embedding_extractor)."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.emb if embedding else ws.logp
        for i, l in enumerate(self.grus):
            X, K = self._in_rows(ws, i)
            H3 = 3 * l.units
            for d, p in enumerate(l.prefixes):
                zg = ws.zg[i][d]
                nv.check(lib.lidbox_gemm_nn(X, self._p(p + ".W"), H3, _rows(zg.data_ptr(), 0, H3, 1, B * T), K, H3,
                                            nv.EPI_BIAS, self._p(p + ".b"), gws, gws_n, st))
            U0, U1 = self._U(l)
            last = i == len(self.grus) - 1
            nv.check(lib.lidbox_gru_fwd(U0, U1, self._b_rec(l.prefixes[0]), self._b_rec(l.prefixes[-1]), l.dirs, B, T, l.units,
                                        nv.ptr(ws.zg[i]), nv.ptr(ws.hseq[i]), nv.ptr(ws.qh[i]),
                                        nv.ptr(ws.hlast) if last else None, st))
        return self._forward_head(ws, training, update_moving, stop_before_output, embedding)

    def _forward_head(self, ws, training=False, update_moving=True, stop_before_output=False, embedding=False):
        """[BatchNormalization] -> Dense [+ BatchNormalization] layers -> output activation on the ws.B final states in
        ws.hlast (the dense and the ragged pass share it); the return value is forward_ws's"""
        st, lib, B = nv.current_stream(), nv.lib, ws.B
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if self.rnn_bn is not None:
            self._bn_fwd(self.rnn_bn, ws.hlast, B, ws.hlast.shape[1], ws.c0, ws.y0, ws, training, update_moving)
        for j, (d, bn) in enumerate(zip(self.denses, self.dense_bns)):
            x = self._head_input(ws, j)
            din = x.shape[1]
            if stop_before_output and j == len(self.denses) - 1:
                return x
            xr = _rows(x.data_ptr(), 0, din, 1, B)
            if embedding:
                nv.check(lib.lidbox_gemm_nn(xr, self._p(d.name + ".W"), d.units, _rows(ws.emb.data_ptr(), 0, d.units, 1, B), din,
                                            d.units, nv.EPI_BIAS, self._p(d.name + ".b"), gws, gws_n, st))
                return ws.emb
            nv.check(lib.lidbox_gemm_nn(xr, self._p(d.name + ".W"), d.units, _rows(ws.h[j].data_ptr(), 0, d.units, 1, B), din,
                                        d.units, nv.EPI_BIAS_RELU if d.relu else nv.EPI_BIAS, self._p(d.name + ".b"),
                                        gws, gws_n, st))
            if bn is not None:
                self._bn_fwd(bn, ws.h[j], B, d.units, ws.c[j], ws.y[j], ws, training, update_moving)
        return self._output_activation(ws, ws.h[-1], self.output_dim)

    # ------------------------------------------------------------------ backward
    def backward_head_ws(self, ws):
        """the whole backward pass (dh[-1] holds d loss / d logits): the Dense / BatchNormalization head, then every GRU
        layer from the top down.  Fills flat_grad (overwrites)."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        ws.pending = []
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        tws, tws_n = nv.ptr(ws.tn_ws), ws.tn_ws.numel()
        if B == 0:
            return
        for j in range(len(self.denses) - 1, -1, -1):
            d = self.denses[j]
            x = self._head_input(ws, j)
            din = x.shape[1]
            dy = _rows(ws.dh[j].data_ptr(), 0, d.units, 1, B)
            nv.check(lib.lidbox_gemm_tn(_rows(x.data_ptr(), 0, din, 1, B), dy, self._p(d.name + ".W", True), d.units, din, d.units,
                                        0, self._p(d.name + ".b", True), tws, tws_n, st))
            if j == 0:
                dst = ws.dlast if self.rnn_bn is None else ws.dy0
                epi, aux = nv.EPI_NONE, None
            elif self.dense_bns[j - 1] is not None:
                dst = ws.dy[j - 1]
                epi, aux = nv.EPI_NONE, None
            else:
                dst = ws.dh[j - 1]
                epi, aux = (nv.EPI_RELU_MASK, nv.ptr(ws.h[j - 1])) if self.denses[j - 1].relu else (nv.EPI_NONE, None)
            nv.check(lib.lidbox_gemm_nt(dy, self._p(d.name + ".W"), d.units, _rows(dst.data_ptr(), 0, din, 1, B), d.units, din,
                                        epi, aux, gws, gws_n, st))
            if j > 0 and self.dense_bns[j - 1] is not None:
                # through the BatchNormalization and (relu_mask) the ReLU of Dense j-1: dh[j-1] = d loss / d pre-activation
                p = self.denses[j - 1]
                self._bn_bwd(self.dense_bns[j - 1], ws.h[j - 1], B, p.units, ws.c[j - 1], ws.dy[j - 1], 1 if p.relu else 0,
                             ws.dh[j - 1], ws)
        if self.rnn_bn is not None:
            self._bn_bwd(self.rnn_bn, ws.hlast, B, ws.hlast.shape[1], ws.c0, ws.dy0, 0, ws.dlast, ws)
        for i in range(len(self.grus) - 1, -1, -1):
            l = self.grus[i]
            H, H3, ldo = l.units, 3 * l.units, l.out_dim
            U0, U1 = self._U(l)
            last = i == len(self.grus) - 1
            nv.check(lib.lidbox_gru_bwd(U0, U1, l.dirs, B, T, H, nv.ptr(ws.zg[i]), nv.ptr(ws.hseq[i]), nv.ptr(ws.qh[i]),
                                        None if last else nv.ptr(ws.dseq[i]), T * ldo, nv.ptr(ws.dlast) if last else None,
                                        nv.ptr(ws.gru_ws), ws.gru_ws.numel(), st))
            X, K = self._in_rows(ws, i)
            hs = ws.hseq[i].data_ptr()
            for d, p in enumerate(l.prefixes):
                zg, qh = ws.zg[i][d].data_ptr(), ws.qh[i][d].data_ptr()
                dzx = _rows(zg, 0, H3, 1, B * T)
                nv.check(lib.lidbox_gemm_tn(X, dzx, self._p(p + ".W", True), H3, K, H3, 0, self._p(p + ".b", True), tws, tws_n, st))
                hprev = h_neighbour_rows(hs, ldo, d, H, B, T)
                dU, dbr = self._p(p + ".U", True), self._b_rec(p, True)
                # dZrec = (dz, dr | dhh * r): its z, r block is dZx's, its h block is qh
                nv.check(lib.lidbox_gemm_tn(hprev, dzx, dU, H3, H, 2 * H, 0, dbr, tws, tws_n, st))
                nv.check(lib.lidbox_gemm_tn(hprev, _rows(qh, 0, H, 1, B * T), ctypes.c_void_p(dU.value + 8 * H), H3, H, H, 0,
                                            ctypes.c_void_p(dbr.value + 8 * H), tws, tws_n, st))
                if i > 0:
                    dprev = ws.dseq[i - 1]
                    nv.check(lib.lidbox_gemm_nt(dzx, self._p(p + ".W"), H3, _rows(dprev.data_ptr(), 0, K, 1, B * T), H3, K,
                                                nv.EPI_ACCUM if d > 0 else nv.EPI_NONE, None, gws, gws_n, st))

    # ------------------------------------------------------------------ ragged pass (inference, float32; models/rnn_ragged.py)
    def _ragged_embedding_dim(self):
        return self.denses[0].units

    def _ragged_buffers_rows(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        H, dirs = max(l.units for l in self.grus), max(l.dirs for l in self.grus)
        return dict(x=torch.zeros((cap, self.input_dim), **f32), zg=torch.zeros(dirs * cap * 3 * H, **f32),
                    qh=torch.zeros(dirs * cap * H, **f32), hseq=[torch.zeros((cap, l.out_dim), **f32) for l in self.grus])

    def _ragged_buffers_B(self, cap):
        """what _forward_head reads of a workspace, for `cap` utterances"""
        f32 = dict(dtype=torch.float32, device=self.device)
        D = self.grus[-1].out_dim
        bufs = dict(hlast=torch.zeros((cap, D), **f32), h=[torch.zeros((cap, d.units), **f32) for d in self.denses],
                    y=[torch.zeros((cap, d.units), **f32) if bn is not None else None for d, bn in zip(self.denses, self.dense_bns)],
                    c=[torch.zeros((4, d.units), **f32) if bn is not None else None for d, bn in zip(self.denses, self.dense_bns)],
                    emb=torch.zeros((cap, self.denses[0].units), **f32), logp=torch.zeros((cap, self.output_dim), **f32))
        if self.rnn_bn is not None:
            bufs.update(y0=torch.zeros((cap, D), **f32), c0=torch.zeros((4, D), **f32))
        return bufs

    def _forward_ragged(self, ws, plan, dev, upto_embedding):
        """every GRU layer on the ragged walk (lidbox_gru_ragged_fwd), then the last layer's final states -- forward at every
        utterance's own last frame, backward at its first -- through the head with the moving statistics"""
        st, lib, B, Rp = nv.current_stream(), nv.lib, plan.B, plan.Rp
        X, K = _rows(ws.x.data_ptr(), 0, self.input_dim, 1, Rp), self.input_dim
        for i, l in enumerate(self.grus):
            hs = ws.hseq[i]
            hs[:Rp].zero_()                                   # the pad rows: the next layer's projection reads every row
            self._ragged_projection(ws, plan, X, K, l.prefixes, 3 * l.units, ws.zg)
            U0, U1 = self._U(l)
            last = i == len(self.grus) - 1
            nv.check(lib.lidbox_gru_ragged_fwd(U0, U1, self._b_rec(l.prefixes[0]), self._b_rec(l.prefixes[-1]), l.dirs, B, l.units,
                                               Rp, dev.slots, dev.sorted_lengths, nv.ptr(ws.zg), nv.ptr(hs), nv.ptr(ws.qh),
                                               nv.ptr(ws.hlast) if last else None, st))
            X, K = _rows(hs.data_ptr(), 0, l.out_dim, 1, Rp), l.out_dim
        need, din = 16, self.grus[-1].out_dim
        for d in self.denses:
            need, din = max(need, lib.lidbox_gemm_rows_workspace(B, d.units, din)), d.units
        ws.reserve_gemm_ws(self, need)
        return self._forward_head(ws, embedding=upto_embedding)

    # ------------------------------------------------------------------ public call
    def embed(self, x):
        """inference-mode output of the first Dense layer without its activation, [B, units] (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, False)
            return self.forward_ws(ws, training=False, embedding=True).clone()


__all__ = ["GRUSpec", "BatchNormSpec", "DenseSpec", "GRUModel"]
