"""
The scaffolding every model engine shares: parameters in one flat fp32 buffer, a cache of per-(B, T) workspaces, and what
`lidbox_amd.train.Trainer` expects of a model.

`FlatParams` is the part that even `SequentialTDNN` (models/tdnn.py) uses:
  * the layout builder.  `add_param` / `add_state` / `add_bn` append entries name -> (offset in floats, shape) to `layout`
    (trainable, in `flat`; `flat_grad` mirrors it and is what RCCL all-reduces) and `state_layout` (BatchNormalization moving
    statistics, in `state`, which Adam never touches); every entry starts on a 16-byte boundary.  `allocate` creates the three
    buffers.  Names are the Keras layer names with the suffixes .W (kernel), .U (recurrent kernel), .b, .gamma, .beta,
    .moving_mean, .moving_variance, in Keras layouts, so a checkpoint maps 1:1;
  * `_init_weights`, the Keras defaults drawn in layout order from one `np.random.default_rng(seed)`;
  * the accessors (`param`, `get_weights`, `_p`, ...) and the `workspace(B, T)` cache;
  * BatchNormalization forward / backward on dense rows (`_bn_fwd` / `_bn_bwd`), on the workspace's `bn_ws` bytes.

`FlatModel` adds what the engines behind rnn / gru_rnn / conv_rnn / spherespeaker / multilevel_attention have in common: the
constructor preamble with the attributes the Trainer reads, the public call and the output activation.  Such a model
computes in float32, has no Conv1D stages (`convs` is empty: one gradient bucket, the whole backward pass is the subclass's
`backward_head_ws`), and everything numeric it does is a liblidbox_hip.so call on the preallocated buffers of a `Workspace`,
so the Trainer can capture a whole train step into a hipGraph.

`lstm_layer_fwd` / `lstm_layer_bwd` are the one LSTM layer of all engines: per direction the input projection X W + b of all
B*T rows as one GEMM, the walk through time (lidbox_lstm_* of csrc/rnn.hip, or the stepped lidbox_lstm_step_* of
csrc/lstm_step.hip), and in backward dW = X^T dZ (with db), dU = H_prev^T dZ and dX = dZ W^T as one GEMM each.  Keras layouts:
kernel W [C, 4H], recurrent_kernel U [H, 4H], bias b [4H], gate order i, f, c, o.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _native as nv


def _align4(n):
    return (n + 3) & ~3


def _rows(t_ptr, batch_stride, row_stride, batch, rpb):
    return nv.Rows(t_ptr, int(batch_stride), int(row_stride), int(batch), int(rpb))


def h_neighbour_rows(h, ld_h, d, H, B, T):
    """rows descriptor of the states a recurrent layer's direction d (width H) came from, for its dU = H_prev^T dZ.  h:
    address of the layer's first column in row 0 of the first utterance's h sequence, rows ld_h floats apart, T + 2 per
    utterance, of which rows 0 and T + 1 stay zero"""
    prow = 0 if d == 0 else 2                 # h_{t-1} (forward) / h_{t+1} (reverse): zero rows at both ends
    return _rows(h + 4 * (prow * ld_h + d * H), (T + 2) * ld_h, ld_h, B, T)


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


class BatchNormSpec:
    """tf.keras.layers.BatchNormalization with its default momentum and epsilon"""

    def __init__(self, name, momentum=0.99, epsilon=1e-3):
        self.name, self.momentum, self.epsilon = name, float(momentum), float(epsilon)


class Workspace:
    """Base of the per-(B, T) device buffers of one model: `x` [B, T, C] is the model input unless a subclass says otherwise"""

    def input_view(self):
        return self.x

    def input_target(self):
        """(pointer, floats between utterances, T, C) of the model input buffer (what Trainer / _load_input fill)"""
        v = self.input_view()
        return ctypes.c_void_p(v.data_ptr()), v.stride(0), v.shape[1], v.shape[2]


class FlatParams:
    """Layout builder, initialiser, accessors and workspace cache (see the module docstring)"""

    workspace_class = None                 # the model's Workspace subclass, built as workspace_class(model, B, T)
    unit_forget_biases = frozenset()       # names of the LSTM biases [4H]: Keras' unit_forget_bias sets their f quarter to 1

    # ------------------------------------------------------------------ layout
    def new_layout(self):
        self.layout, self.state_layout = {}, {}
        self.num_flat = self._num_state = 0

    def add_param(self, name, shape):
        self.layout[name] = (self.num_flat, shape)
        self.num_flat = _align4(self.num_flat + int(np.prod(shape)))

    def add_state(self, name, shape):
        self.state_layout[name] = (self._num_state, shape)
        self._num_state = _align4(self._num_state + int(np.prod(shape)))

    def add_bn(self, name, C):
        """a BatchNormalization over C channels: gamma and beta are parameters, the moving statistics are state"""
        self.add_param(name + ".gamma", (C,))
        self.add_param(name + ".beta", (C,))
        self.add_state(name + ".moving_mean", (C,))
        self.add_state(name + ".moving_variance", (C,))

    def allocate(self):
        self.flat = torch.zeros(self.num_flat, dtype=torch.float32, device=self.device)
        self.flat_grad = torch.zeros_like(self.flat)
        self.state = torch.zeros(max(self._num_state, 4), dtype=torch.float32, device=self.device)

    def _init_weights(self, seed):
        """Keras defaults: glorot_uniform kernels (a Conv kernel's fans count its receptive field), orthogonal recurrent
        kernels, zero biases with the LSTM forget gate's quarter set to 1, gamma 1, beta 0, moving mean 0, moving variance 1"""
        rng = np.random.default_rng(seed)
        host = np.zeros(self.num_flat, np.float32)
        for name, (off, shape) in self.layout.items():
            n = int(np.prod(shape))
            if name.endswith(".W"):
                rf = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
                limit = math.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
                host[off:off + n] = rng.uniform(-limit, limit, size=n).astype(np.float32)
            elif name.endswith(".U"):
                host[off:off + n] = orthogonal(shape, rng).astype(np.float32).ravel()
            elif name.endswith(".gamma"):
                host[off:off + n] = 1.0
            elif name in self.unit_forget_biases:
                H = shape[0] // 4
                host[off + H:off + 2 * H] = 1.0
        self.flat.copy_(torch.from_numpy(host))
        self.state.zero_()
        for name, (off, shape) in self.state_layout.items():
            if name.endswith(".moving_variance"):
                self.state[off:off + shape[0]] = 1.0

    # ------------------------------------------------------------------ accessors
    def param(self, name, grad=False):
        if name in self.state_layout:
            off, shape = self.state_layout[name]
            return self.state[off:off + int(np.prod(shape))].view(shape)
        off, shape = self.layout[name]
        buf = self.flat_grad if grad else self.flat
        return buf[off:off + int(np.prod(shape))].view(shape)

    def named_parameters(self):
        return [(n, self.param(n)) for n in self.layout]

    def count_params(self):
        """Keras `Model.count_params()`: trainable + non-trainable (BatchNormalization moving statistics)"""
        return sum(int(np.prod(s)) for _, s in list(self.layout.values()) + list(self.state_layout.values()))

    def get_weights(self):
        """dict name -> numpy array in Keras layouts (trainable parameters and the BatchNormalization moving statistics)"""
        return {n: self.param(n).detach().cpu().numpy().copy() for n in list(self.layout) + list(self.state_layout)}

    def set_weights(self, weights):
        for n, w in weights.items():
            self.param(n).copy_(torch.as_tensor(np.asarray(w, np.float32)).to(self.device).reshape(self.param(n).shape))

    def _p(self, name, grad=False):
        off, _ = self.layout[name]
        return ctypes.c_void_p((self.flat_grad if grad else self.flat).data_ptr() + 4 * off)

    def _sp(self, name):
        off, _ = self.state_layout[name]
        return ctypes.c_void_p(self.state.data_ptr() + 4 * off)

    # ------------------------------------------------------------------ BatchNormalization
    def _bn_fwd(self, bn, x, R, C, consts, y, ws, training, update_moving, bessel=0):
        """BatchNormalization `bn` (a BatchNormSpec) of the dense rows x [R, C]: fills consts [4, C] (mean, invstd, scale,
        shift: from batch statistics when training, which also move the moving statistics if update_moving; else from the
        moving statistics) and writes y = scale x + shift; y None leaves the apply to the caller's fused kernel.  Returns the
        four pointers into consts.  bessel 0: tf.keras' non-fused path (2-D / 3-D inputs), the moving variance moves towards
        the population variance; bessel None: its fused path (4-D inputs, lidbox_bn_train_stats), towards the
        Bessel-corrected one."""
        lib, st = nv.lib, nv.current_stream()
        cp = [ctypes.c_void_p(consts.data_ptr() + 4 * j * C) for j in range(4)]
        gamma, beta = self._p(bn.name + ".gamma"), self._p(bn.name + ".beta")
        if training:
            mm = self._sp(bn.name + ".moving_mean") if update_moving else None
            mv = self._sp(bn.name + ".moving_variance") if update_moving else None
            if bessel is None:
                nv.check(lib.lidbox_bn_train_stats(nv.ptr(x), R, C, gamma, beta, bn.epsilon, bn.momentum, mm, mv,
                                                   cp[0], cp[1], cp[2], cp[3], nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
            else:
                nv.check(lib.lidbox_bn_train_stats_ex(nv.ptr(x), R, C, gamma, beta, bn.epsilon, bn.momentum, bessel, mm, mv,
                                                      cp[0], cp[1], cp[2], cp[3], nv.ptr(ws.bn_ws), ws.bn_ws.numel(), st))
        else:
            nv.check(lib.lidbox_bn_infer_consts(gamma, beta, self._sp(bn.name + ".moving_mean"),
                                                self._sp(bn.name + ".moving_variance"), bn.epsilon, C, cp[2], cp[3], st))
        if y is not None:
            nv.check(lib.lidbox_bn_apply(nv.ptr(x), R, C, cp[2], cp[3], _rows(y.data_ptr(), 0, C, 1, R), st))
        return cp

    def _bn_bwd(self, bn, x, R, C, consts, dy, relu_mask, dx, ws):
        """dx = gradient of the BatchNormalization input x [R, C] from dy, the gradient of its output; relu_mask 1: x is a
        ReLU's output and dx the gradient in front of that ReLU.  Fills the gradients of gamma and beta."""
        nv.check(nv.lib.lidbox_bn_bwd(nv.ptr(x), _rows(dy.data_ptr(), 0, C, 1, R), R, C, ctypes.c_void_p(consts.data_ptr()),
                                      ctypes.c_void_p(consts.data_ptr() + 4 * C), self._p(bn.name + ".gamma"), relu_mask,
                                      self._p(bn.name + ".gamma", True), self._p(bn.name + ".beta", True), nv.ptr(dx),
                                      nv.ptr(ws.bn_ws), ws.bn_ws.numel(), nv.current_stream()))

    # ------------------------------------------------------------------ workspace
    def workspace(self, B, T):
        key = (int(B), int(T))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) >= 4:                     # keep the cache small
                self._ws.pop(next(iter(self._ws)))
            ws = self.workspace_class(self, *key)
            self._ws[key] = ws
        return ws


class FlatModel(FlatParams):
    """Base of the float32 engines without Conv1D stages (see the module docstring).  A subclass's __init__ calls
    `super().__init__`, lays its parameters out with add_param / add_state / add_bn and ends with `self._finish(seed)`; it
    provides `workspace_class`, `forward_ws(ws, training, update_moving, stop_before_output, normalize)` and
    `backward_head_ws(ws)`, and its workspace has `x`, `h` / `dh` (last entry: the logits and their gradient), `logp`, `loss`
    and `pending`."""

    def __init__(self, input_shape, name, output_activation, seed, device, compute_dtype, channel_dropout_rate=0.0):
        if compute_dtype not in ("float32", "fp32", "f32", torch.float32):
            raise ValueError("%s computes in float32 only, got compute_dtype=%r" % (name, compute_dtype))
        if output_activation not in (None, "log_softmax", "softmax"):
            raise ValueError("output_activation must be None, 'log_softmax' or 'softmax', got %r" % (output_activation,))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.name = name
        self.input_shape = tuple(input_shape)
        self.input_dim = self.model_input_dim = int(input_shape[-1])
        self.output_activation = output_activation
        self.compute_dtype = "float32"
        # SpatialDropout1D on the input; the seed is drawn from `seed` by a generator of its own, so it does not depend on
        # the layout.  Eager calls key their masks on the host-side call counter, the captured train step on its step counter
        self.channel_dropout_rate = float(channel_dropout_rate)
        self.dropout_seed = int(np.random.default_rng(seed).integers(1, 2 ** 62))
        self._dropout_calls = 0
        # what lidbox_amd.train.Trainer reads from every model: no Conv1D stages (so one gradient bucket and no
        # backward_conv_ws), no 2-D front-end, no bf16 shadows, no frequency attention, no wgrad side streams
        self.convs, self.frontend, self.bf16_storage, self.attention = [], None, False, None
        self.wgrad_stream = None
        self.head_wgrad_stream = None
        self.new_layout()

    def _finish(self, seed):
        self.allocate()
        self._init_weights(seed)
        self._ws = {}

    def fused_output_ok(self):
        return False

    def _output_activation(self, ws, logits, N):
        """the model output from the logits [B, N]: the logits themselves, or their (log-)softmax in ws.logp"""
        if self.output_activation is None:
            return logits
        fn = nv.lib.lidbox_softmax_fwd if self.output_activation == "softmax" else nv.lib.lidbox_log_softmax_fwd
        nv.check(fn(nv.ptr(logits), ws.B, N, nv.ptr(ws.logp), nv.current_stream()))
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


class LSTMLayer:
    """One LSTM layer's place in a workspace, as lstm_layer_fwd / lstm_layer_bwd take it.
    prefixes: the parameter name prefixes of its one or two directions (forward first).  X, K: rows descriptor and width of
    its input.  zg [dirs, B, T, 4H]: the gate pre-activations, in backward overwritten by their gradient dZ; cseq
    [dirs, B, T, H]: the cell states.  h, ld_h: the h sequence as h_neighbour_rows takes it.  step: the stepped walk
    (lidbox_lstm_step_*, which takes ld_h) instead of lidbox_lstm_* (whose h sequence is dense, ld_h = dirs * H).  gemm: a
    GEMM family (`SequentialTDNN.gemm`), default the fp32 entry points; gemm_ws / tn_ws / lstm_ws: workspace bytes of the
    nn / nt GEMMs, the tn GEMMs and the walk."""

    def __init__(self, prefixes, X, K, B, T, H, zg, cseq, h, ld_h, lstm_ws, gemm_ws, tn_ws, step=False, gemm=None):
        self.prefixes, self.X, self.K, self.B, self.T, self.H = list(prefixes), X, K, B, T, H
        self.zg, self.cseq, self.h, self.ld_h, self.step = zg, cseq, h, ld_h, step
        self.lstm_ws, self.gemm_ws, self.tn_ws = lstm_ws, gemm_ws, tn_ws
        self.nn, self.nt, self.tn = ((nv.lib.lidbox_gemm_nn, nv.lib.lidbox_gemm_nt, nv.lib.lidbox_gemm_tn) if gemm is None
                                     else (gemm.nn, gemm.nt, gemm.tn))
        assert step or ld_h == len(self.prefixes) * H

    def dz(self, d):
        return _rows(self.zg[d].data_ptr(), 0, 4 * self.H, 1, self.B * self.T)


def lstm_layer_fwd(m, l):
    """layer l (an LSTMLayer) of model m: the input projections into zg, then the walk, which fills the h sequence and cseq"""
    st = nv.current_stream()
    B, T, H, H4 = l.B, l.T, l.H, 4 * l.H
    for d, p in enumerate(l.prefixes):
        nv.check(l.nn(l.X, m._p(p + ".W"), H4, l.dz(d), l.K, H4, nv.EPI_BIAS, m._p(p + ".b"), nv.ptr(l.gemm_ws), l.gemm_ws.numel(), st))
    U = [m._p(p + ".U") for p in l.prefixes] + [None]
    if l.step:
        nv.check(nv.lib.lidbox_lstm_step_fwd(U[0], U[1], len(l.prefixes), B, T, H, nv.ptr(l.zg), ctypes.c_void_p(l.h), l.ld_h,
                                             nv.ptr(l.cseq), nv.ptr(l.lstm_ws), l.lstm_ws.numel(), st))
    else:
        nv.check(nv.lib.lidbox_lstm_fwd(U[0], U[1], len(l.prefixes), B, T, H, nv.ptr(l.zg), ctypes.c_void_p(l.h), nv.ptr(l.cseq),
                                        nv.ptr(l.lstm_ws), l.lstm_ws.numel(), st))


def lstm_layer_bwd(m, l, dseq, dseq_bs, dseq_rs, dh_last=None, dX=None, dX_epi=(nv.EPI_NONE, nv.EPI_ACCUM), dX_aux=None):
    """backward of layer l of model m.  dseq: pointer to the gradient of its output sequence (None: none), utterances
    dseq_bs and rows dseq_rs floats apart (lidbox_lstm_bwd takes dense rows, dseq_rs = dirs * H); dh_last: pointer to the
    gradient of its final states [B, dirs * H] (None: none).  The walk turns zg into dZ; then per direction dW with db, dU and,
    with dX (the rows descriptor of the input gradient), dX = dZ W^T under epilogue dX_epi[0] for the first direction and
    dX_epi[1] for the second (dX_aux: the ReLU-mask source of EPI_RELU_MASK)."""
    st = nv.current_stream()
    B, T, H, H4, dirs = l.B, l.T, l.H, 4 * l.H, len(l.prefixes)
    tws, tws_n = nv.ptr(l.tn_ws), l.tn_ws.numel()
    U = [m._p(p + ".U") for p in l.prefixes] + [None]
    if l.step:
        nv.check(nv.lib.lidbox_lstm_step_bwd(U[0], U[1], dirs, B, T, H, nv.ptr(l.zg), nv.ptr(l.cseq), dseq, dseq_bs, dseq_rs, dh_last,
                                             nv.ptr(l.lstm_ws), l.lstm_ws.numel(), st))
    else:
        assert dseq_rs == dirs * H
        nv.check(nv.lib.lidbox_lstm_bwd(U[0], U[1], dirs, B, T, H, nv.ptr(l.zg), nv.ptr(l.cseq), dseq, dseq_bs, dh_last,
                                        nv.ptr(l.lstm_ws), l.lstm_ws.numel(), st))
    for d, p in enumerate(l.prefixes):
        dz = l.dz(d)
        nv.check(l.tn(l.X, dz, m._p(p + ".W", True), H4, l.K, H4, 0, m._p(p + ".b", True), tws, tws_n, st))
        hprev = h_neighbour_rows(l.h, l.ld_h, d, H, B, T)
        nv.check(l.tn(hprev, dz, m._p(p + ".U", True), H4, H, H4, 0, None, tws, tws_n, st))
        if dX is not None:
            nv.check(l.nt(dz, m._p(p + ".W"), H4, dX, H4, l.K, dX_epi[min(d, 1)], dX_aux, nv.ptr(l.gemm_ws), l.gemm_ws.numel(), st))


__all__ = ["FlatParams", "FlatModel", "Workspace", "BatchNormSpec", "LSTMLayer", "orthogonal", "lstm_layer_fwd", "lstm_layer_bwd"]
