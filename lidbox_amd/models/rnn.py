"""
Recurrent engine: the host-side orchestration shared by `lidbox_amd.models.lstm` and `lidbox_amd.models.ap_lstm`.

A model is  [SpatialDropout1D]  ->  LSTM / Bidirectional(LSTM) layers  ->  a head:
  * "last": the last layer's final h -> Dense -> output activation (reference lidbox/models/lstm.py:14-20);
  * "avg_concat": each BLSTM's output sequence, scaled by its alpha, averaged over time into its half of the pooled
    vector (ap_lstm.py:37-41; the Concatenate is folded into where each half lands).  The model output is that vector
    L2-normalised (ap_lstm.py:42); the train step hands the un-normalised vector to the angular-proximity head, which
    normalises it itself (normalising twice is the identity).

Everything numeric is a liblidbox_hip.so call on preallocated device buffers, so the whole train step can be captured
into a hipGraph by `lidbox_amd.train.Trainer` (the model has no Conv1D layers: one gradient bucket, and backward is
`backward_head_ws`).  Per LSTM layer and direction: the input projection X W + b of all B*T rows is one lidbox_gemm_nn, the
walk through time is lidbox_lstm_fwd / _bwd (csrc/rnn.hip), and dW = X^T dZ (with db), dU = H_prev^T dZ and dX = dZ W^T are
one GEMM each.

Parameters live in one flat fp32 buffer in Keras layouts: kernel W [C, 4H], recurrent_kernel U [H, 4H], bias b [4H], gate
order i, f, c, o; names follow the Keras layer names (`lstm.W`, `forward_lstm_1.U`, `backward_lstm_1.b`, `output.W`), so a
checkpoint maps 1:1.  Initialisation as Keras: glorot_uniform kernels, orthogonal recurrent kernels, zero biases with the
forget gate's quarter set to 1 (unit_forget_bias).
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv
from .tdnn import DenseSpec, _rows


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


def _align4(n):
    return (n + 3) & ~3


class _Workspace:
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

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        return ctypes.c_void_p(self.x.data_ptr()), self.x.stride(0), self.x.shape[1], self.x.shape[2]


class RecurrentModel:
    """[SpatialDropout1D] -> LSTM layers -> head, parameters in one flat buffer (see the module docstring)."""

    def __init__(self, input_shape, lstms, head, denses=(), name="rnn", output_activation="log_softmax",
                 channel_dropout_rate=0.0, alphas=None, seed=None, device=None, compute_dtype="float32"):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("recurrent models compute in float32 only, got compute_dtype=%r" % (compute_dtype,))
        if head not in ("last", "avg_concat"):
            raise ValueError("head must be 'last' or 'avg_concat'")
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        self.lstms, self.head, self.denses = list(lstms), head, list(denses)
        if head == "last" and (self.lstms[-1].return_sequences or not self.denses):
            raise ValueError("a 'last' head reads the final h of an LSTM with return_sequences=False into Dense layers")
        if head == "last" and self.lstms[-1].bidirectional:
            raise ValueError("a 'last' head reads a forward-only LSTM")
        if head == "avg_concat" and (self.denses or not all(l.return_sequences for l in self.lstms)):
            raise ValueError("an 'avg_concat' head pools the output sequences of every LSTM layer and has no Dense layer")
        self.alphas = [float(a) for a in (alphas or [1.0] * len(self.lstms))]
        self.output_activation = output_activation
        self.channel_dropout_rate = float(channel_dropout_rate)
        self.dropout_seed = int(np.random.default_rng(seed).integers(1, 2 ** 62))
        self._dropout_calls = 0
        self.compute_dtype = "float32"
        # what lidbox_amd.train.Trainer reads from every model
        self.convs, self.frontend, self.bf16_storage, self.attention = [], None, False, None
        self.state_layout = {}
        self.wgrad_stream = None
        self.head_wgrad_stream = None
        self.layout = {}
        off = 0
        cin = self.input_dim
        for l in self.lstms:
            for p in l.prefixes:
                for suffix, shape in ((".W", (cin, 4 * l.units)), (".U", (l.units, 4 * l.units)), (".b", (4 * l.units,))):
                    self.layout[p + suffix] = (off, shape)
                    off = _align4(off + int(np.prod(shape)))
            cin = l.out_dim
        for d in self.denses:
            for suffix, shape in ((".W", (cin, d.units)), (".b", (d.units,))):
                self.layout[d.name + suffix] = (off, shape)
                off = _align4(off + int(np.prod(shape)))
            cin = d.units
        self.output_dim = cin if head == "last" else sum(l.out_dim for l in self.lstms)
        self.num_flat = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._init_weights(seed)
        self._ws = {}

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        """Keras LSTM / Dense defaults: glorot_uniform kernels, orthogonal recurrent kernels, zero biases, unit_forget_bias."""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.num_flat, np.float32)
        for name, (off, shape) in self.layout.items():
            n = int(np.prod(shape))
            if name.endswith(".W"):
                limit = math.sqrt(6.0 / (shape[0] + shape[1]))
                host[off:off + n] = rng.uniform(-limit, limit, size=n).astype(np.float32)
            elif name.endswith(".U"):
                host[off:off + n] = orthogonal(shape, rng).astype(np.float32).ravel()
            elif name.endswith(".b") and name.rsplit(".", 1)[0] not in {d.name for d in self.denses}:
                H = shape[0] // 4
                host[off + H:off + 2 * H] = 1.0
        self.flat.copy_(torch.from_numpy(host))

    def param(self, name, grad=False):
        off, shape = self.layout[name]
        buf = self.flat_grad if grad else self.flat
        return buf[off:off + int(np.prod(shape))].view(shape)

    def named_parameters(self):
        return [(n, self.param(n)) for n in self.layout]

    def count_params(self):
        """Keras `Model.count_params()`: 4H(C + H + 1) per LSTM direction plus the Dense layers"""
        return sum(int(np.prod(s)) for _, s in self.layout.values())

    def get_weights(self):
        return {n: self.param(n).detach().cpu().numpy().copy() for n in self.layout}

    def set_weights(self, weights):
        for n, w in weights.items():
            self.param(n).copy_(torch.as_tensor(np.asarray(w, np.float32)).to(self.device).reshape(self.param(n).shape))

    def _p(self, name, grad=False):
        off, _ = self.layout[name]
        return ctypes.c_void_p((self.flat_grad if grad else self.flat).data_ptr() + 4 * off)

    def fused_output_ok(self):
        return False

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

    def _U(self, l):
        return self._p(l.prefixes[0] + ".U"), (self._p(l.prefixes[1] + ".U") if l.dirs == 2 else None)

    # ------------------------------------------------------------------ forward
    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False):
        """The model input buffer (ws.input_view()) must already hold the input.  Returns the model output before its
        output activation's normalisation for 'avg_concat' (normalize=True: the L2-normalised output), the log-probs /
        probabilities / logits of a 'last' head otherwise."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        for i, l in enumerate(self.lstms):
            X, K = self._in_rows(ws, i)
            H4 = 4 * l.units
            for d, p in enumerate(l.prefixes):
                zg = ws.zg[i][d]
                nv.check(lib.lidbox_gemm_nn(X, self._p(p + ".W"), H4, _rows(zg.data_ptr(), 0, H4, 1, B * T), K, H4,
                                            nv.EPI_BIAS, self._p(p + ".b"), gws, gws_n, st))
            U0, U1 = self._U(l)
            nv.check(lib.lidbox_lstm_fwd(U0, U1, l.dirs, B, T, l.units, nv.ptr(ws.zg[i]), nv.ptr(ws.hseq[i]), nv.ptr(ws.cseq[i]),
                                         nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
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
        x, din = self._last_rows(ws), self.lstms[-1].out_dim
        for j, d in enumerate(self.denses):
            if stop_before_output and j == len(self.denses) - 1:
                return x
            nv.check(lib.lidbox_gemm_nn(x, self._p(d.name + ".W"), d.units, _rows(ws.h[j].data_ptr(), 0, d.units, 1, B), din,
                                        d.units, nv.EPI_BIAS_RELU if d.relu else nv.EPI_BIAS, self._p(d.name + ".b"),
                                        gws, gws_n, st))
            x, din = _rows(ws.h[j].data_ptr(), 0, d.units, 1, B), d.units
        if self.output_activation is None:
            return ws.h[-1]
        fn = lib.lidbox_softmax_fwd if self.output_activation == "softmax" else lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(ws.h[-1]), B, din, nv.ptr(ws.logp), st))
        return ws.logp

    # ------------------------------------------------------------------ backward
    def flush_reduce_jobs(self, ws):
        """run what is still pending (the optimizer's prepare job the train step appends) as a launch of its own"""
        while ws.pending:
            chunk, ws.pending = ws.pending[:2], ws.pending[2:]
            arr = (nv.ReduceJob * len(chunk))(*[j for j, _ in chunk])
            nv.check(nv.lib.lidbox_reduce_jobs_run(arr, len(chunk), nv.current_stream()))

    def join_wgrad(self):
        pass

    def backward_ws(self, ws):
        """dh[-1] must hold d loss / d (model output before its activation).  Fills flat_grad (overwrites)."""
        self.backward_head_ws(ws)
        self.flush_reduce_jobs(ws)

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
            l = self.lstms[i]
            H, H4, ldo = l.units, 4 * l.units, l.out_dim
            U0, U1 = self._U(l)
            dseq = ws.dseq[i]
            nv.check(lib.lidbox_lstm_bwd(U0, U1, l.dirs, B, T, H, nv.ptr(ws.zg[i]), nv.ptr(ws.cseq[i]), nv.ptr(dseq),
                                         T * ldo, None if l.return_sequences else nv.ptr(ws.dlast),
                                         nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
            X, K = self._in_rows(ws, i)
            hs = ws.hseq[i].data_ptr()
            for d, p in enumerate(l.prefixes):
                dz = _rows(ws.zg[i][d].data_ptr(), 0, H4, 1, B * T)
                nv.check(lib.lidbox_gemm_tn(X, dz, self._p(p + ".W", True), H4, K, H4, 0, self._p(p + ".b", True), tws, tws_n, st))
                prow = 0 if d == 0 else 2                 # h_{t-1} (forward) / h_{t+1} (reverse): zero rows at both ends
                hprev = _rows(hs + 4 * (prow * ldo + d * H), (T + 2) * ldo, ldo, B, T)
                nv.check(lib.lidbox_gemm_tn(hprev, dz, self._p(p + ".U", True), H4, H, H4, 0, None, tws, tws_n, st))
                if i > 0:
                    # dX of layer i = the gradient of layer i-1's output sequence (on top of its pooled share, if any)
                    acc = d > 0 or self.head == "avg_concat"
                    dprev = ws.dseq[i - 1]
                    nv.check(lib.lidbox_gemm_nt(dz, self._p(p + ".W"), H4, _rows(dprev.data_ptr(), 0, K, 1, B * T), H4, K,
                                                nv.EPI_ACCUM if acc else nv.EPI_NONE, None, gws, gws_n, st))

    # ------------------------------------------------------------------ public call
    def _load_input(self, ws, x, training):
        x = nv.require_gpu_tensor(x, "x", torch.float32)
        if x.dim() != 3 or x.shape[2] != self.input_dim:
            raise ValueError("expected input [B, T, %d], got %s" % (self.input_dim, tuple(x.shape)))
        st = nv.current_stream()
        ws.x.copy_(x)
        if training and self.channel_dropout_rate > 0:
            # SpatialDropout1D (ap_lstm.py:27-28); eager calls draw from a host-side call counter
            self._dropout_calls += 1
            in_ptr, in_bs, _, C = ws.input_target()
            nv.check(nv.lib.lidbox_spatial_dropout(in_ptr, ws.B, ws.T, C, in_bs, self.channel_dropout_rate,
                                                   (self.dropout_seed + 0x51ED27 * self._dropout_calls) & (2 ** 64 - 1),
                                                   None, None, st))

    def __call__(self, x, training=False):
        """x [B, T, C] on the HIP device -> the model output [B, D] (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, training)
            return self.forward_ws(ws, training=training, normalize=True).clone()

    predict = __call__


def orthogonal(shape, rng, gain=1.0):
    """tf.keras.initializers.Orthogonal: QR of a normal [max, min] matrix, signs fixed by diag(R), transposed to `shape`
    when it has fewer rows than columns (then its rows are orthonormal)"""
    rows, cols = shape
    a = rng.standard_normal((max(rows, cols), min(rows, cols)))
    q, r = np.linalg.qr(a)
    q = q * np.sign(np.diag(r))
    if rows < cols:
        q = q.T
    return np.ascontiguousarray(gain * q.reshape(shape))


__all__ = ["LSTMSpec", "DenseSpec", "RecurrentModel", "orthogonal"]
