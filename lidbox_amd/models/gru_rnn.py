"""
GRU engine: the host-side orchestration of `lidbox_amd.models.bi_gru`, the GRU twin of `lidbox_amd.models.rnn`.

A model is  [SpatialDropout1D]  ->  GRU / Bidirectional(GRU) layers  ->  the last layer's final state (both directions
concatenated, forward t = T-1 and backward t = 0)  ->  [BatchNormalization]  ->  Dense layers, each optionally followed by
BatchNormalization  ->  output activation (reference lidbox/models/bi_gru.py:26-48).

Everything numeric is a liblidbox_hip.so call on preallocated device buffers, so `lidbox_amd.train.Trainer` captures the whole
train step into a hipGraph (one gradient bucket, backward is `backward_head_ws`).  Per GRU layer and direction: the input
projection X W + b_in of all B*T rows is one lidbox_gemm_nn; the walk through time is lidbox_gru_fwd / _bwd (csrc/gru.hip, one
launch per step for both directions); dW = X^T dZx (with db_in), dU = H_prev^T dZrec (with db_rec, in two column blocks:
dZrec's h block lives in qh) and dX = dZx W^T are GEMMs.

BatchNormalization here sees 2-D inputs [B, C], so it follows tf.keras' non-fused path: normalise with the batch mean and
population variance, move the running variance towards the population variance (lidbox_bn_train_stats_ex, bessel = 0).  The
moving statistics live in `state` / `state_layout` and move only when `update_moving` (not in the Trainer's warm-up pass), as
in `lidbox_amd.models.xvector_2d`.

Parameters live in one flat fp32 buffer in Keras layouts: kernel W [C, 3H], recurrent_kernel U [H, 3H], bias b [2, 3H]
(input bias, recurrent bias), gate order z, r, h.  A Bidirectional wrapper's halves are named by wrapper and direction
(`BGRU_1_forward.W`, `BGRU_1_backward.U`), not by Keras' session-dependent inner names; Dense and BatchNormalization layers
keep their Keras names (`fc_relu_1.W`, `BGRU_2_bn.gamma`, `BGRU_2_bn.moving_variance`).  Initialisation as Keras:
glorot_uniform kernels, orthogonal recurrent kernels, zero biases, BatchNormalization gamma 1 / beta 0 / moving mean 0 /
moving variance 1.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv
from .rnn import RecurrentModel, orthogonal
from .tdnn import DenseSpec, _rows


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


class BatchNormSpec:
    """tf.keras.layers.BatchNormalization defaults on a [B, C] input"""

    def __init__(self, name, momentum=0.99, epsilon=1e-3):
        self.name, self.momentum, self.epsilon = name, float(momentum), float(epsilon)


def _align4(n):
    return (n + 3) & ~3


class _Workspace:
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

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        return ctypes.c_void_p(self.x.data_ptr()), self.x.stride(0), self.x.shape[1], self.x.shape[2]


class GRUModel(RecurrentModel):
    """[SpatialDropout1D] -> GRU layers -> final state -> [BatchNormalization] -> Dense [+ BatchNormalization] layers.
    Shares the public calls of `RecurrentModel` (workspace cache, input loading, __call__); see the module docstring."""

    def __init__(self, input_shape, grus, denses, rnn_bn=None, dense_bns=None, name="gru", output_activation="log_softmax",
                 channel_dropout_rate=0.0, seed=None, device=None, compute_dtype="float32"):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("recurrent models compute in float32 only, got compute_dtype=%r" % (compute_dtype,))
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        self.grus, self.denses = list(grus), list(denses)
        if not self.denses or self.grus[-1].return_sequences or not all(l.return_sequences for l in self.grus[:-1]):
            raise ValueError("the last GRU returns its final state only, into Dense layers; the others return sequences")
        self.dense_bns = list(dense_bns) if dense_bns is not None else [None] * len(self.denses)
        if len(self.dense_bns) != len(self.denses) or self.dense_bns[-1] is not None:
            raise ValueError("dense_bns: one entry (BatchNormSpec or None) per Dense layer, None for the output layer")
        self.rnn_bn = rnn_bn
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        self.head = "last"
        self.lstms = []
        self.output_activation = output_activation
        self.channel_dropout_rate = float(channel_dropout_rate)
        self.dropout_seed = int(np.random.default_rng(seed).integers(1, 2 ** 62))
        self._dropout_calls = 0
        self.compute_dtype = "float32"
        # what lidbox_amd.train.Trainer reads from every model
        self.convs, self.frontend, self.bf16_storage, self.attention = [], None, False, None
        self.wgrad_stream = None
        self.head_wgrad_stream = None
        self.layout, self.state_layout = {}, {}
        off, soff = 0, 0

        def bn_entries(bn, C):
            nonlocal off, soff
            for suffix in (".gamma", ".beta"):
                self.layout[bn.name + suffix] = (off, (C,))
                off = _align4(off + C)
            for suffix in (".moving_mean", ".moving_variance"):
                self.state_layout[bn.name + suffix] = (soff, (C,))
                soff = _align4(soff + C)

        cin = self.input_dim
        for l in self.grus:
            H = l.units
            for p in l.prefixes:
                for suffix, shape in ((".W", (cin, 3 * H)), (".U", (H, 3 * H)), (".b", (2, 3 * H))):
                    self.layout[p + suffix] = (off, shape)
                    off = _align4(off + int(np.prod(shape)))
            cin = l.out_dim
        if rnn_bn is not None:
            bn_entries(rnn_bn, cin)
        for d, bn in zip(self.denses, self.dense_bns):
            for suffix, shape in ((".W", (cin, d.units)), (".b", (d.units,))):
                self.layout[d.name + suffix] = (off, shape)
                off = _align4(off + int(np.prod(shape)))
            cin = d.units
            if bn is not None:
                bn_entries(bn, cin)
        self.output_dim = cin
        self.num_flat = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(max(soff, 4), dtype=torch.float32, device=self.device)
        self._init_weights(seed)
        self._ws = {}

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        """Keras GRU / Dense / BatchNormalization defaults: glorot_uniform kernels, orthogonal recurrent kernels, zero biases,
        gamma 1, beta 0, moving mean 0, moving variance 1"""
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
        """Keras `Model.count_params()`: 3H(C + H + 2) per GRU direction, the Dense layers and 4C per BatchNormalization
        (gamma, beta and the two moving statistics)"""
        return sum(int(np.prod(s)) for _, s in list(self.layout.values()) + list(self.state_layout.values()))

    def get_weights(self):
        """dict name -> numpy array in Keras layouts (trainable parameters and the BatchNormalization moving statistics)"""
        return {n: self.param(n).detach().cpu().numpy().copy() for n in list(self.layout) + list(self.state_layout)}

    def _sp(self, name):
        off, _ = self.state_layout[name]
        return ctypes.c_void_p(self.state.data_ptr() + 4 * off)

    def _b_rec(self, prefix, grad=False):
        """row 1 of the Keras bias [2, 3H]: the recurrent bias"""
        off, shape = self.layout[prefix + ".b"]
        return ctypes.c_void_p((self.flat_grad if grad else self.flat).data_ptr() + 4 * (off + shape[1]))

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
    def _bn_fwd(self, bn, x, C, consts, y, ws, training, update_moving):
        lib, st = nv.lib, nv.current_stream()
        B = ws.B
        cp = [ctypes.c_void_p(consts.data_ptr() + 4 * j * C) for j in range(4)]
        if training:
            mm = self._sp(bn.name + ".moving_mean") if update_moving else None
            mv = self._sp(bn.name + ".moving_variance") if update_moving else None
            nv.check(lib.lidbox_bn_train_stats_ex(nv.ptr(x), B, C, self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                  bn.epsilon, bn.momentum, 0, mm, mv, cp[0], cp[1], cp[2], cp[3],
                                                  nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
        else:
            nv.check(lib.lidbox_bn_infer_consts(self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                self._sp(bn.name + ".moving_mean"), self._sp(bn.name + ".moving_variance"),
                                                bn.epsilon, C, cp[2], cp[3], st))
        nv.check(lib.lidbox_bn_apply(nv.ptr(x), B, C, cp[2], cp[3], _rows(y.data_ptr(), 0, C, 1, B), st))

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
        if self.rnn_bn is not None:
            self._bn_fwd(self.rnn_bn, ws.hlast, ws.hlast.shape[1], ws.c0, ws.y0, ws, training, update_moving)
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
                self._bn_fwd(bn, ws.h[j], d.units, ws.c[j], ws.y[j], ws, training, update_moving)
        if self.output_activation is None:
            return ws.h[-1]
        fn = lib.lidbox_softmax_fwd if self.output_activation == "softmax" else lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(ws.h[-1]), B, self.output_dim, nv.ptr(ws.logp), st))
        return ws.logp

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, bn, x, C, consts, dy, relu_mask, dx, ws):
        nv.check(nv.lib.lidbox_bn_bwd(nv.ptr(x), _rows(dy.data_ptr(), 0, C, 1, ws.B), ws.B, C, ctypes.c_void_p(consts.data_ptr()),
                                      ctypes.c_void_p(consts.data_ptr() + 4 * C), self._p(bn.name + ".gamma"), relu_mask,
                                      self._p(bn.name + ".gamma", True), self._p(bn.name + ".beta", True), nv.ptr(dx),
                                      nv.ptr(ws.bn_ws), ws.bn_ws.numel(), nv.current_stream()))

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
                self._bn_bwd(self.dense_bns[j - 1], ws.h[j - 1], p.units, ws.c[j - 1], ws.dy[j - 1], 1 if p.relu else 0,
                             ws.dh[j - 1], ws)
        if self.rnn_bn is not None:
            self._bn_bwd(self.rnn_bn, ws.hlast, ws.hlast.shape[1], ws.c0, ws.dy0, 0, ws.dlast, ws)
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
                prow = 0 if d == 0 else 2                 # h_{t-1} (forward) / h_{t+1} (reverse): zero rows at both ends
                hprev = _rows(hs + 4 * (prow * ldo + d * H), (T + 2) * ldo, ldo, B, T)
                dU, dbr = self._p(p + ".U", True), self._b_rec(p, True)
                # dZrec = (dz, dr | dhh * r): its z, r block is dZx's, its h block is qh
                nv.check(lib.lidbox_gemm_tn(hprev, dzx, dU, H3, H, 2 * H, 0, dbr, tws, tws_n, st))
                nv.check(lib.lidbox_gemm_tn(hprev, _rows(qh, 0, H, 1, B * T), ctypes.c_void_p(dU.value + 8 * H), H3, H, H, 0,
                                            ctypes.c_void_p(dbr.value + 8 * H), tws, tws_n, st))
                if i > 0:
                    dprev = ws.dseq[i - 1]
                    nv.check(lib.lidbox_gemm_nt(dzx, self._p(p + ".W"), H3, _rows(dprev.data_ptr(), 0, K, 1, B * T), H3, K,
                                                nv.EPI_ACCUM if d > 0 else nv.EPI_NONE, None, gws, gws_n, st))

    # ------------------------------------------------------------------ public call
    def embed(self, x):
        """inference-mode output of the first Dense layer without its activation, [B, units] (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, False)
            return self.forward_ws(ws, training=False, embedding=True).clone()


__all__ = ["GRUSpec", "BatchNormSpec", "DenseSpec", "GRUModel"]
