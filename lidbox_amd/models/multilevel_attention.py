"""
Multi-level attention classifier of Yu et al. (2018), reference lidbox/models/multilevel_attention.py:21-85.  With
K = num_outputs and y_0 = the input [B, T, D], level l = 1..L is
  DenseBlock `dense_block{l}`: Dense(H) `dense_block{l}_fc` on every frame -> BatchNormalization `dense_block{l}_bn` -> ReLU ->
  Dropout(dropout_rate), giving y_l [B, T, H], which feeds the next level and
  Attention `attention{l}`: z = Dense(K) `attention{l}_input` of y_l, p = softmax(z) over the classes, c = clip(p, 1e-7, 1 - 1e-7),
  q = c / sum_t c, att_l = sum_t q * sigmoid(z)  [B, K];
then Concatenate `attention_concat` of the L attention outputs -> Dense(K) `outputs` -> output activation.

Everything numeric is a liblidbox_hip.so call on preallocated device buffers, so `lidbox_amd.train.Trainer` captures the whole
train step into a hipGraph (one gradient bucket, backward is `backward_head_ws`).  Every Dense product and weight gradient is
one call of the GEMM family over the B*T (or B) rows.  The BatchNormalization apply, the ReLU and the Dropout of a level are
one pass (lidbox_bn_relu_dropout_fwd / _bwd, csrc/mla.hip), and so is a level's attention pooling
(lidbox_mla_attention_fwd / _bwd).  The Concatenate is free: the levels write their attention outputs into column slices of one
[B, L*K] buffer, and backward reads the gradient slices of one [B, L*K] buffer.  In backward the gradient of y_l is the
attention branch dz W_att^T plus, below the top level, the next level's da W_fc^T (EPI_ACCUM).

The BatchNormalization layers see a 3-D input, which tf.keras normalises on its non-fused path: batch mean and population
variance over the B*T rows, eps 1e-3, momentum 0.99, the moving variance moved towards the population variance
(lidbox_bn_train_stats_ex, bessel = 0).  Moving statistics live in `state` / `state_layout` and move only when `update_moving`.

Dropout masks are never stored: level l's mask is a counter-based hash of (seed_l, *step, row, channel), regenerated in
backward.  seed_l is mixed per level and per data-parallel rank as SequentialTDNN._fe_dropout_seed mixes FrameLayer2D's; the
step is `dropout_step`, which the Trainer points at its optimizer step counter (a standalone training-mode call reads 0).

Parameters live in one flat fp32 buffer in Keras layouts (Dense kernel [in, out]) under the Keras names of the inner layers
(`dense_block1_fc.W`, `dense_block2_bn.gamma`, `attention1_input.b`, `outputs.W`), so a checkpoint maps 1:1.  Initialisation as
Keras: glorot_uniform kernels, zero biases, BatchNormalization 1 / 0 / 0 / 1.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv
from .gru_rnn import BatchNormSpec
from .rnn import RecurrentModel
from .tdnn import DenseSpec, _rows

MAX_OUTPUTS = 1024          # lidbox_mla_attention_*: a row of class logits lives in the registers of one wave


def _align4(n):
    return (n + 3) & ~3


class _Workspace:
    """All per-(B, T) device buffers of one multilevel_attention model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
        lib = nv.lib
        self.B, self.T = B, T
        H, K, L, D = model.units, model.output_dim, model.levels, model.input_dim
        R = B * T
        self.x = torch.zeros((B, T, D), **f32)
        self.a = [torch.zeros((R, H), **f32) for _ in range(L)]          # dense_block{l}_fc's output: the BatchNormalization input
        self.y = [torch.zeros((R, H), **f32) for _ in range(L)]          # the block's output y_l
        self.consts = [torch.zeros((4, H), **f32) for _ in range(L)]     # mean, invstd, scale, shift
        self.z = [torch.zeros((R, K), **f32) for _ in range(L)]          # attention logits
        self.colsum = [torch.zeros((B, K), **f32) for _ in range(L)]     # sum_t clip(p)
        self.att = torch.zeros((B, L * K), **f32)                        # the concatenated attention outputs
        self.datt = torch.zeros((B, L * K), **f32)
        self.dz = torch.zeros((R, K), **f32)
        self.dy = torch.zeros((R, H), **f32)                             # gradient of y_l, then of the BatchNormalization output
        self.da = torch.zeros((R, H), **f32)                             # gradient of a_l
        self.h = [torch.zeros((B, K), **f32)]                            # logits
        self.dh = [torch.zeros((B, K), **f32)]
        self.logp = torch.zeros((B, K), **f32)
        self.loss = torch.zeros(4, **f32)
        gws, tws = 0, 16
        cin = D
        for _ in range(L):
            gws = max(gws, lib.lidbox_gemm_rows_workspace(R, H, cin), lib.lidbox_gemm_rows_workspace(R, cin, H),
                      lib.lidbox_gemm_rows_workspace(R, K, H), lib.lidbox_gemm_rows_workspace(R, H, K))
            tws = max(tws, lib.lidbox_gemm_tn_workspace(R, cin, H), lib.lidbox_gemm_tn_workspace(R, H, K))
            cin = H
        gws = max(gws, lib.lidbox_gemm_rows_workspace(B, K, L * K), lib.lidbox_gemm_rows_workspace(B, L * K, K))
        tws = max(tws, lib.lidbox_gemm_tn_workspace(B, L * K, K))
        self.gemm_ws = torch.empty(max(16, gws), dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.bn_ws = torch.empty(max(16, lib.lidbox_bn_workspace(max(R, 1), H)), dtype=torch.uint8, device=dev)
        self.pending = []

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        return ctypes.c_void_p(self.x.data_ptr()), self.x.stride(0), self.x.shape[1], self.x.shape[2]


class MultilevelAttentionModel(RecurrentModel):
    """L x (Dense -> BatchNormalization -> ReLU -> Dropout, with an attention pooling of its output) -> Concatenate -> Dense.
    Shares the public calls of `RecurrentModel` (parameter access, input loading, __call__); see the module docstring."""

    def __init__(self, input_shape, num_outputs, L=2, H=512, dropout_rate=0.4, name="DNN_multilevel_attention",
                 output_activation="log_softmax", seed=None, device=None, compute_dtype="float32"):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("multilevel_attention computes in float32 only, got compute_dtype=%r" % (compute_dtype,))
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        if int(L) < 1 or int(H) < 1 or not 1 <= int(num_outputs) <= MAX_OUTPUTS:
            raise ValueError("multilevel_attention needs L >= 1, H >= 1 and 1 <= num_outputs <= %d, got L=%r, H=%r, num_outputs=%r"
                             % (MAX_OUTPUTS, L, H, num_outputs))
        if not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        self.levels, self.units, self.output_dim = int(L), int(H), int(num_outputs)
        self.dropout_rate = float(dropout_rate)
        self.blocks = ["dense_block%d" % (l + 1) for l in range(self.levels)]
        self.bns = [BatchNormSpec(b + "_bn") for b in self.blocks]
        self.attentions = ["attention%d_input" % (l + 1) for l in range(self.levels)]
        self.out = DenseSpec("outputs", self.output_dim, relu=False)
        self.denses = [self.out]
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

        Hn, K = self.units, self.output_dim
        cin = self.input_dim
        for l in range(self.levels):
            fc, bn, at = self.blocks[l] + "_fc", self.bns[l].name, self.attentions[l]
            entry(fc + ".W", (cin, Hn))
            entry(fc + ".b", (Hn,))
            entry(bn + ".gamma", (Hn,))
            entry(bn + ".beta", (Hn,))
            for suffix in (".moving_mean", ".moving_variance"):
                self.state_layout[bn + suffix] = (soff, (Hn,))
                soff = _align4(soff + Hn)
            entry(at + ".W", (Hn, K))
            entry(at + ".b", (K,))
            cin = Hn
        entry("outputs.W", (self.levels * K, K))
        entry("outputs.b", (K,))
        self.num_flat = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(max(soff, 4), dtype=torch.float32, device=self.device)
        self._init_weights(seed)
        self._ws = {}

    # ------------------------------------------------------------------ parameters
    def _init_weights(self, seed):
        """Keras defaults: glorot_uniform kernels, zero biases, gamma 1, beta 0, moving mean 0, moving variance 1"""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.num_flat, np.float32)
        for name, (off, shape) in self.layout.items():
            n = int(np.prod(shape))
            if name.endswith(".W"):
                limit = math.sqrt(6.0 / (shape[0] + shape[1]))
                host[off:off + n] = rng.uniform(-limit, limit, size=n).astype(np.float32)
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
        """Keras `Model.count_params()`: the Dense layers and 4H per BatchNormalization (gamma, beta and the two moving
        statistics)"""
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

    def _in_rows(self, ws, l):
        """(rows descriptor, width) of level l's input: the model input, or the previous level's output"""
        R = ws.B * ws.T
        if l == 0:
            return _rows(ws.x.data_ptr(), 0, self.input_dim, 1, R), self.input_dim
        return _rows(ws.y[l - 1].data_ptr(), 0, self.units, 1, R), self.units

    # ------------------------------------------------------------------ dropout keys
    def level_dropout_seed(self, l):
        """the seed of level l's mask (l from 0): mixed per level and, through `dropout_seed_mix` (the Trainer's per-rank offset
        under data parallelism, 0 otherwise), per rank -- the mixing of SequentialTDNN._fe_dropout_seed"""
        return (self.dropout_seed + getattr(self, "dropout_seed_mix", 0) + 0xD1B54A32D192ED03 * (l + 1)) & (2 ** 64 - 1)

    def _dropout_step_ptr(self):
        """device int64 that keys the masks: the Trainer points `dropout_step` at its optimizer step (a fresh mask per step,
        also under graph replay); standalone training-mode calls use a constant zero"""
        t = getattr(self, "dropout_step", None)
        return None if t is None else nv.ptr(t)

    # ------------------------------------------------------------------ forward
    def forward_ws(self, ws, training=False, update_moving=True, stop_before_output=False, normalize=False):
        """The model input buffer (ws.input_view()) must already hold the input.  training selects batch statistics in the
        BatchNormalization layers (update_moving=False leaves the running statistics untouched) and switches the Dropout
        on.  Returns the log-probs / probabilities / logits (output_activation None); stop_before_output: the concatenated
        attention outputs [B, L*K]."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        H, K, L = self.units, self.output_dim, self.levels
        R = B * T
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.att if stop_before_output else ws.logp
        rate = self.dropout_rate if training else 0.0
        for l in range(L):
            fc, bn, at = self.blocks[l] + "_fc", self.bns[l], self.attentions[l]
            X, cin = self._in_rows(ws, l)
            nv.check(lib.lidbox_gemm_nn(X, self._p(fc + ".W"), H, _rows(ws.a[l].data_ptr(), 0, H, 1, R), cin, H, nv.EPI_BIAS,
                                        self._p(fc + ".b"), gws, gws_n, st))
            cp = [ctypes.c_void_p(ws.consts[l].data_ptr() + 4 * j * H) for j in range(4)]
            if training:
                mm = self._sp(bn.name + ".moving_mean") if update_moving else None
                mv = self._sp(bn.name + ".moving_variance") if update_moving else None
                nv.check(lib.lidbox_bn_train_stats_ex(nv.ptr(ws.a[l]), R, H, self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                      bn.epsilon, bn.momentum, 0, mm, mv, cp[0], cp[1], cp[2], cp[3],
                                                      nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
            else:
                nv.check(lib.lidbox_bn_infer_consts(self._p(bn.name + ".gamma"), self._p(bn.name + ".beta"),
                                                    self._sp(bn.name + ".moving_mean"), self._sp(bn.name + ".moving_variance"),
                                                    bn.epsilon, H, cp[2], cp[3], st))
            nv.check(lib.lidbox_bn_relu_dropout_fwd(nv.ptr(ws.a[l]), R, H, cp[2], cp[3], rate, self.level_dropout_seed(l),
                                                    self._dropout_step_ptr(), nv.ptr(ws.y[l]), st))
            nv.check(lib.lidbox_gemm_nn(_rows(ws.y[l].data_ptr(), 0, H, 1, R), self._p(at + ".W"), K,
                                        _rows(ws.z[l].data_ptr(), 0, K, 1, R), H, K, nv.EPI_BIAS, self._p(at + ".b"), gws, gws_n, st))
            nv.check(lib.lidbox_mla_attention_fwd(nv.ptr(ws.z[l]), B, T, K, ctypes.c_void_p(ws.att.data_ptr() + 4 * l * K), L * K,
                                                  nv.ptr(ws.colsum[l]), st))
        if stop_before_output:
            return ws.att
        nv.check(lib.lidbox_gemm_nn(_rows(ws.att.data_ptr(), 0, L * K, 1, B), self._p("outputs.W"), K,
                                    _rows(ws.h[-1].data_ptr(), 0, K, 1, B), L * K, K, nv.EPI_BIAS, self._p("outputs.b"),
                                    gws, gws_n, st))
        if self.output_activation is None:
            return ws.h[-1]
        fn = lib.lidbox_softmax_fwd if self.output_activation == "softmax" else lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(ws.h[-1]), B, K, nv.ptr(ws.logp), st))
        return ws.logp

    # ------------------------------------------------------------------ backward
    def backward_head_ws(self, ws):
        """the whole backward pass of a training-mode forward (dh[-1] holds d loss / d logits): the output layer, then the
        levels from the top down.  Fills flat_grad (overwrites)."""
        st = nv.current_stream()
        lib = nv.lib
        B, T = ws.B, ws.T
        H, K, L = self.units, self.output_dim, self.levels
        R = B * T
        ws.pending = []
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        tws, tws_n = nv.ptr(ws.tn_ws), ws.tn_ws.numel()
        if B == 0:
            return
        # outputs: the gradient of the concatenated attention outputs
        dlogits = _rows(ws.dh[-1].data_ptr(), 0, K, 1, B)
        nv.check(lib.lidbox_gemm_tn(_rows(ws.att.data_ptr(), 0, L * K, 1, B), dlogits, self._p("outputs.W", True), K, L * K, K, 0,
                                    self._p("outputs.b", True), tws, tws_n, st))
        nv.check(lib.lidbox_gemm_nt(dlogits, self._p("outputs.W"), K, _rows(ws.datt.data_ptr(), 0, L * K, 1, B), K, L * K,
                                    nv.EPI_NONE, None, gws, gws_n, st))
        dz = _rows(ws.dz.data_ptr(), 0, K, 1, R)
        dy = _rows(ws.dy.data_ptr(), 0, H, 1, R)
        da = _rows(ws.da.data_ptr(), 0, H, 1, R)
        for l in range(L - 1, -1, -1):
            fc, bn, at = self.blocks[l] + "_fc", self.bns[l], self.attentions[l]
            yl = _rows(ws.y[l].data_ptr(), 0, H, 1, R)
            # attention{l}: dz from the level's slices of att / datt, then its Dense
            nv.check(lib.lidbox_mla_attention_bwd(nv.ptr(ws.z[l]), ctypes.c_void_p(ws.att.data_ptr() + 4 * l * K), L * K,
                                                  nv.ptr(ws.colsum[l]), ctypes.c_void_p(ws.datt.data_ptr() + 4 * l * K), L * K,
                                                  B, T, K, nv.ptr(ws.dz), st))
            nv.check(lib.lidbox_gemm_tn(yl, dz, self._p(at + ".W", True), K, H, K, 0, self._p(at + ".b", True), tws, tws_n, st))
            # gradient of y_l: the attention branch, on top of the next level's da W_fc^T below the top level
            nv.check(lib.lidbox_gemm_nt(dz, self._p(at + ".W"), K, dy, K, H, nv.EPI_NONE if l == L - 1 else nv.EPI_ACCUM, None,
                                        gws, gws_n, st))
            # Dropout and ReLU (mask regenerated from the forward key), then the BatchNormalization
            c = ws.consts[l]
            nv.check(lib.lidbox_bn_relu_dropout_bwd(nv.ptr(ws.a[l]), R, H, ctypes.c_void_p(c.data_ptr() + 4 * 2 * H),
                                                    ctypes.c_void_p(c.data_ptr() + 4 * 3 * H), self.dropout_rate,
                                                    self.level_dropout_seed(l), self._dropout_step_ptr(), nv.ptr(ws.dy),
                                                    nv.ptr(ws.dy), st))
            nv.check(lib.lidbox_bn_bwd(nv.ptr(ws.a[l]), dy, R, H, ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(c.data_ptr() + 4 * H),
                                       self._p(bn.name + ".gamma"), 0, self._p(bn.name + ".gamma", True),
                                       self._p(bn.name + ".beta", True), nv.ptr(ws.da), nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
            # dense_block{l}_fc
            X, cin = self._in_rows(ws, l)
            nv.check(lib.lidbox_gemm_tn(X, da, self._p(fc + ".W", True), H, cin, H, 0, self._p(fc + ".b", True), tws, tws_n, st))
            if l > 0:
                nv.check(lib.lidbox_gemm_nt(da, self._p(fc + ".W"), H, dy, H, cin, nv.EPI_NONE, None, gws, gws_n, st))


def create(input_shape, num_outputs, output_activation="log_softmax", L=2, H=512, seed=None, device=None,
           compute_dtype="float32", dropout_rate=0.4):
    """output_activation: "log_softmax" (the reference's default), "softmax" or None (logits).  L levels of width H.
    dropout_rate: the reference's fixed rate (0.4) by default; 0 serves tests."""
    return MultilevelAttentionModel(input_shape, num_outputs, L=L, H=H, dropout_rate=dropout_rate,
                                    output_activation=output_activation or None, seed=seed, device=device,
                                    compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`

__all__ = ["MultilevelAttentionModel", "create", "loader"]
