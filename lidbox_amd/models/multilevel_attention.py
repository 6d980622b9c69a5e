"""
Multi-level attention classifier of Yu et al. (2018), reference lidbox/models/multilevel_attention.py:21-85.  With
K = num_outputs and y_0 = the input [B, T, D], level l = 1..L is
  DenseBlock `dense_block{l}`: Dense(H) `dense_block{l}_fc` on every frame -> BatchNormalization `dense_block{l}_bn` -> ReLU ->
  Dropout(dropout_rate), giving y_l [B, T, H], which feeds the next level and
  Attention `attention{l}`: z = Dense(K) `attention{l}_input` of y_l, p = softmax(z) over the classes, c = clip(p, 1e-7, 1 - 1e-7),
  q = c / sum_t c, att_l = sum_t q * sigmoid(z)  [B, K];
then Concatenate `attention_concat` of the L attention outputs -> Dense(K) `outputs` -> output activation.

The scaffolding is `lidbox_amd.models.flat`'s.  Every Dense product and weight gradient is
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

Parameters carry the Keras names of the inner layers (`dense_block1_fc.W`, `dense_block2_bn.gamma`, `attention1_input.b`,
`outputs.W`).

Ragged pass (inference): `ragged_pass.RaggedPass` with `_ragged_pass`, which needs no layout of its own.

Ragged training pass: `forward_ragged_train` / `backward_ragged` on a `RaggedTrainWorkspace`.  They are the launches of
`forward_ws(training=True)` / `backward_head_ws` (one body each, `_forward_levels` / `_backward_levels`) over the R = total_T
concatenated frames, with the two pooling calls swapped for lidbox_mla_attention_ragged_fwd (with colsum) / _ragged_bwd.  The
batch statistics are those of the real frames and a mask's row is the row in the concatenation.
"""
import ctypes

import torch

from .. import _native as nv
from .flat import FlatModel, Workspace, _rows
from .gru_rnn import BatchNormSpec
from .ragged_pass import EmbeddingExtractor, RaggedPass, RaggedWorkspace, upload_int64
from .tdnn import DenseSpec

MAX_OUTPUTS = 1024          # lidbox_mla_attention_*: a row of class logits lives in the registers of one wave


class _Workspace(Workspace):
    """All per-(B, T) device buffers of one multilevel_attention model."""

    def __init__(self, model, B, T):
        dev = model.device
        f32 = dict(dtype=torch.float32, device=dev)
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
        gws, tws, bws = model.train_byte_needs(R, B)
        self.gemm_ws = torch.empty(gws, dtype=torch.uint8, device=dev)
        self.tn_ws = torch.empty(tws, dtype=torch.uint8, device=dev)
        self.bn_ws = torch.empty(bws, dtype=torch.uint8, device=dev)
        self.pending = []

    def pool_fwd(self, model, l, st):
        K, L = model.output_dim, model.levels
        nv.check(nv.lib.lidbox_mla_attention_fwd(nv.ptr(self.z[l]), self.B, self.T, K, ctypes.c_void_p(self.att.data_ptr() + 4 * l * K),
                                                 L * K, nv.ptr(self.colsum[l]), st))

    def pool_bwd(self, model, l, st):
        K, L = model.output_dim, model.levels
        nv.check(nv.lib.lidbox_mla_attention_bwd(nv.ptr(self.z[l]), ctypes.c_void_p(self.att.data_ptr() + 4 * l * K), L * K,
                                                 nv.ptr(self.colsum[l]), ctypes.c_void_p(self.datt.data_ptr() + 4 * l * K), L * K,
                                                 self.B, self.T, K, nv.ptr(self.dz), st))


class RaggedTrainWorkspace(RaggedWorkspace):
    """Device buffers of the ragged training pass, sized by the capacities `cap_rows` and `cap_B` (growth:
    `RaggedWorkspace.reserve`); a pass uses the front of them.  Unlike the inference workspace it keeps every level's `a`, `y` and
    `z` for backward.  `x` is the caller's X [R, D] itself, `ro_table` the pass's one upload.  The byte workspaces are reserved per
    call for the call's own R and B (`reserve_bytes`)."""

    buffers_prefix = "_ragged_train_buffers_"

    def __init__(self, model):
        super().__init__(model)
        self.tn_ws = torch.empty(16, dtype=torch.uint8, device=model.device)
        self.bn_ws = torch.empty(16, dtype=torch.uint8, device=model.device)
        self.x = self.ro_table = self.ro_dev = None
        self.R = self.max_T = 0
        self.grown = 0                     # how often a capacity was exceeded
        self.pending = []

    def reserve(self, model, **needs):
        caps = (self.cap_rows, self.cap_B)
        super().reserve(model, **needs)
        if (self.cap_rows, self.cap_B) != caps:
            self.grown += 1
            for name in ("ap_zn", "ap_dzn", "ap_per", "ap_scores"):          # the Trainer's angular-proximity buffers, sized by cap_B
                self.__dict__.pop(name, None)

    def reserve_bytes(self, model, R, B):
        for name, n in zip(("gemm_ws", "tn_ws", "bn_ws"), model.train_byte_needs(R, B)):
            if n > getattr(self, name).numel():
                setattr(self, name, torch.empty(int(n), dtype=torch.uint8, device=model.device))

    def pool_fwd(self, model, l, st):
        K, L = model.output_dim, model.levels
        nv.check(nv.lib.lidbox_mla_attention_ragged_fwd(nv.ptr(self.z[l]), self.ro_dev, self.B, K,
                                                        ctypes.c_void_p(self.att.data_ptr() + 4 * l * K), L * K, nv.ptr(self.colsum[l]), st))

    def pool_bwd(self, model, l, st):
        K, L = model.output_dim, model.levels
        nv.check(nv.lib.lidbox_mla_attention_ragged_bwd(nv.ptr(self.z[l]), self.ro_dev, self.B, self.max_T, K,
                                                        ctypes.c_void_p(self.att.data_ptr() + 4 * l * K), L * K, nv.ptr(self.colsum[l]),
                                                        ctypes.c_void_p(self.datt.data_ptr() + 4 * l * K), L * K, nv.ptr(self.dz), st))


class MultilevelAttentionModel(FlatModel, RaggedPass):
    """L x (Dense -> BatchNormalization -> ReLU -> Dropout, with an attention pooling of its output) -> Concatenate -> Dense
    (see the module docstring)."""

    workspace_class = _Workspace

    def __init__(self, input_shape, num_outputs, L=2, H=512, dropout_rate=0.4, name="DNN_multilevel_attention",
                 output_activation="log_softmax", seed=None, device=None, compute_dtype="float32"):
        super().__init__(input_shape, name, output_activation, seed, device, compute_dtype)
        if int(L) < 1 or int(H) < 1 or not 1 <= int(num_outputs) <= MAX_OUTPUTS:
            raise ValueError("multilevel_attention needs L >= 1, H >= 1 and 1 <= num_outputs <= %d, got L=%r, H=%r, num_outputs=%r"
                             % (MAX_OUTPUTS, L, H, num_outputs))
        if not 0.0 <= float(dropout_rate) < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        self.levels, self.units, self.output_dim = int(L), int(H), int(num_outputs)
        self.dropout_rate = float(dropout_rate)
        self.blocks = ["dense_block%d" % (l + 1) for l in range(self.levels)]
        self.bns = [BatchNormSpec(b + "_bn") for b in self.blocks]
        self.attentions = ["attention%d_input" % (l + 1) for l in range(self.levels)]
        self.out = DenseSpec("outputs", self.output_dim, relu=False)
        self.denses = [self.out]
        Hn, K = self.units, self.output_dim
        cin = self.input_dim
        for l in range(self.levels):
            fc, at = self.blocks[l] + "_fc", self.attentions[l]
            self.add_param(fc + ".W", (cin, Hn))
            self.add_param(fc + ".b", (Hn,))
            self.add_bn(self.bns[l].name, Hn)
            self.add_param(at + ".W", (Hn, K))
            self.add_param(at + ".b", (K,))
            cin = Hn
        self.add_param("outputs.W", (self.levels * K, K))
        self.add_param("outputs.b", (K,))
        self._finish(seed)

    def train_byte_needs(self, R, B):
        """bytes of (gemm_ws, tn_ws, bn_ws) a training pass over R frames of B utterances needs"""
        lib = nv.lib
        H, K, L = self.units, self.output_dim, self.levels
        gws, tws = 0, 16
        cin = self.input_dim
        for _ in range(L):
            gws = max(gws, lib.lidbox_gemm_rows_workspace(R, H, cin), lib.lidbox_gemm_rows_workspace(R, cin, H),
                      lib.lidbox_gemm_rows_workspace(R, K, H), lib.lidbox_gemm_rows_workspace(R, H, K))
            tws = max(tws, lib.lidbox_gemm_tn_workspace(R, cin, H), lib.lidbox_gemm_tn_workspace(R, H, K))
            cin = H
        gws = max(gws, lib.lidbox_gemm_rows_workspace(B, K, L * K), lib.lidbox_gemm_rows_workspace(B, L * K, K))
        tws = max(tws, lib.lidbox_gemm_tn_workspace(B, L * K, K))
        return max(16, gws), tws, max(16, lib.lidbox_bn_workspace(max(R, 1), H))

    def _in_rows(self, ws, l, R):
        """(rows descriptor, width) of level l's input over R rows: the model input, or the previous level's output"""
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
        return self._forward_levels(ws, ws.B * ws.T, training, update_moving, stop_before_output)

    def _forward_levels(self, ws, R, training, update_moving, stop_before_output=False):
        """the forward launches over the R rows of ws.B utterances, dense ([B, T, D] in ws.x, R = B T) or ragged (ws.x the
        concatenated frames): they differ in where the rows come from and in `ws.pool_fwd`"""
        st = nv.current_stream()
        lib = nv.lib
        B = ws.B
        H, K, L = self.units, self.output_dim, self.levels
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        if B == 0:
            return ws.att if stop_before_output else ws.logp
        rate = self.dropout_rate if training else 0.0
        for l in range(L):
            fc, bn, at = self.blocks[l] + "_fc", self.bns[l], self.attentions[l]
            X, cin = self._in_rows(ws, l, R)
            nv.check(lib.lidbox_gemm_nn(X, self._p(fc + ".W"), H, _rows(ws.a[l].data_ptr(), 0, H, 1, R), cin, H, nv.EPI_BIAS,
                                        self._p(fc + ".b"), gws, gws_n, st))
            cp = self._bn_fwd(bn, ws.a[l], R, H, ws.consts[l], None, ws, training, update_moving)
            nv.check(lib.lidbox_bn_relu_dropout_fwd(nv.ptr(ws.a[l]), R, H, cp[2], cp[3], rate, self.level_dropout_seed(l),
                                                    self._dropout_step_ptr(), nv.ptr(ws.y[l]), st))
            nv.check(lib.lidbox_gemm_nn(_rows(ws.y[l].data_ptr(), 0, H, 1, R), self._p(at + ".W"), K,
                                        _rows(ws.z[l].data_ptr(), 0, K, 1, R), H, K, nv.EPI_BIAS, self._p(at + ".b"), gws, gws_n, st))
            ws.pool_fwd(self, l, st)
        if stop_before_output:
            return ws.att
        nv.check(lib.lidbox_gemm_nn(_rows(ws.att.data_ptr(), 0, L * K, 1, B), self._p("outputs.W"), K,
                                    _rows(ws.h[-1].data_ptr(), 0, K, 1, B), L * K, K, nv.EPI_BIAS, self._p("outputs.b"),
                                    gws, gws_n, st))
        return self._output_activation(ws, ws.h[-1], K)

    def embed(self, x):
        """the concatenated attention outputs [B, L*K] of a batch x [B, T, D] in inference mode (a fresh tensor)"""
        with torch.cuda.device(self.device):
            ws = self.workspace(x.shape[0], x.shape[1])
            self._load_input(ws, x, False)
            return self.forward_ws(ws, training=False, stop_before_output=True).clone()

    # ------------------------------------------------------------------ ragged pass (inference; models/ragged_pass.py)
    def _ragged_embedding_dim(self):
        return self.levels * self.output_dim

    def _ragged_plan(self, ro, lengths):
        """no layout of its own: the frames stay where the caller has them"""
        return None, dict(rows=int(ro[-1]), B=len(lengths))

    def _ragged_buffers_rows(self, cap):
        """per frame.  Inference keeps nothing for a backward pass, so one `a`, one `y` and one `z` serve every level: level
        l's y overwrites level l - 1's once a_l = y_{l-1} W has been formed.  consts: every pass writes the scale and shift
        it reads (`_bn_fwd`), so they may be replaced with the rest"""
        f32 = dict(dtype=torch.float32, device=self.device)
        H, K = self.units, self.output_dim
        return dict(a=torch.zeros((cap, H), **f32),          # dense_block{l}_fc's output: the BatchNormalization input
                    y=torch.zeros((cap, H), **f32),          # the block's output y_l
                    z=torch.zeros((cap, K), **f32),          # attention logits
                    consts=[torch.zeros((4, H), **f32) for _ in range(self.levels)])     # mean, invstd, scale, shift

    def _ragged_buffers_B(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        K = self.output_dim
        return dict(att=torch.zeros((cap, self.levels * K), **f32),       # the concatenated attention outputs
                    h=torch.zeros((cap, K), **f32), logp=torch.zeros((cap, K), **f32))

    def _ragged_pass(self, ws, plan, X, ro, upto_embedding):
        """X [total_T, D].  Every layer in front of the pooling works on single frames, so X is the GEMM operand as it stands;
        only the attention pooling knows the utterances (lidbox_mla_attention_ragged_fwd).  BatchNormalization uses the
        moving statistics and the Dropout is off.  Returns the model output [B, K] or, upto_embedding, the concatenated
        attention outputs [B, L*K].  The one upload is row_offsets."""
        B, R = ws.B, int(X.shape[0])
        H, K, L = self.units, self.output_dim, self.levels
        st, lib = nv.current_stream(), nv.lib
        need, cin = max(lib.lidbox_gemm_rows_workspace(B, K, L * K), 16), self.input_dim
        for _ in range(L):
            need = max(need, lib.lidbox_gemm_rows_workspace(R, H, cin), lib.lidbox_gemm_rows_workspace(R, K, H))
            cin = H
        ws.reserve_gemm_ws(self, need)
        gws, gws_n = nv.ptr(ws.gemm_ws), ws.gemm_ws.numel()
        table, (ro_dev,) = upload_int64([ro], self.device)
        a, y, z = (_rows(t.data_ptr(), 0, t.shape[1], 1, R) for t in (ws.a, ws.y, ws.z))
        rows_in, cin = _rows(X.data_ptr(), 0, self.input_dim, 1, R), self.input_dim
        for l in range(L):
            fc, bn, at = self.blocks[l] + "_fc", self.bns[l], self.attentions[l]
            nv.check(lib.lidbox_gemm_nn(rows_in, self._p(fc + ".W"), H, a, cin, H, nv.EPI_BIAS, self._p(fc + ".b"), gws, gws_n, st))
            cp = self._bn_fwd(bn, ws.a, R, H, ws.consts[l], None, ws, False, False)
            nv.check(lib.lidbox_bn_relu_dropout_fwd(nv.ptr(ws.a), R, H, cp[2], cp[3], 0.0, self.level_dropout_seed(l), None,
                                                    nv.ptr(ws.y), st))
            nv.check(lib.lidbox_gemm_nn(y, self._p(at + ".W"), K, z, H, K, nv.EPI_BIAS, self._p(at + ".b"), gws, gws_n, st))
            nv.check(lib.lidbox_mla_attention_ragged_fwd(nv.ptr(ws.z), ro_dev, B, K,
                                                         ctypes.c_void_p(ws.att.data_ptr() + 4 * l * K), L * K, None, st))
            rows_in, cin = y, H
        if upto_embedding:
            return ws.att
        nv.check(lib.lidbox_gemm_nn(_rows(ws.att.data_ptr(), 0, L * K, 1, B), self._p("outputs.W"), K,
                                    _rows(ws.h.data_ptr(), 0, K, 1, B), L * K, K, nv.EPI_BIAS, self._p("outputs.b"), gws, gws_n, st))
        return self._output_activation(ws, ws.h, K)

    # ------------------------------------------------------------------ backward
    def backward_head_ws(self, ws):
        """the whole backward pass of a training-mode forward (dh[-1] holds d loss / d logits): the output layer, then the
        levels from the top down.  Fills flat_grad (overwrites)."""
        self._backward_levels(ws, ws.B * ws.T)

    def _backward_levels(self, ws, R):
        """the backward launches over the R rows of ws.B utterances, dense or ragged (`_forward_levels`): `ws.pool_bwd`"""
        st = nv.current_stream()
        lib = nv.lib
        B = ws.B
        H, K, L = self.units, self.output_dim, self.levels
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
            ws.pool_bwd(self, l, st)
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
            self._bn_bwd(bn, ws.a[l], R, H, c, ws.dy, 0, ws.da, ws)
            # dense_block{l}_fc
            X, cin = self._in_rows(ws, l, R)
            nv.check(lib.lidbox_gemm_tn(X, da, self._p(fc + ".W", True), H, cin, H, 0, self._p(fc + ".b", True), tws, tws_n, st))
            if l > 0:
                nv.check(lib.lidbox_gemm_nt(da, self._p(fc + ".W"), H, dy, H, cin, nv.EPI_NONE, None, gws, gws_n, st))

    # ------------------------------------------------------------------ ragged training pass
    def _ragged_train_buffers_rows(self, cap):
        """per frame; every level's a, y and z are kept for backward"""
        f32 = dict(dtype=torch.float32, device=self.device)
        H, K, L = self.units, self.output_dim, self.levels
        return dict(a=[torch.zeros((cap, H), **f32) for _ in range(L)], y=[torch.zeros((cap, H), **f32) for _ in range(L)],
                    z=[torch.zeros((cap, K), **f32) for _ in range(L)], consts=[torch.zeros((4, H), **f32) for _ in range(L)],
                    dz=torch.zeros((cap, K), **f32), dy=torch.zeros((cap, H), **f32), da=torch.zeros((cap, H), **f32))

    def _ragged_train_buffers_B(self, cap):
        f32 = dict(dtype=torch.float32, device=self.device)
        K, L = self.output_dim, self.levels
        return dict(colsum=[torch.zeros((cap, K), **f32) for _ in range(L)], att=torch.zeros((cap, L * K), **f32),
                    datt=torch.zeros((cap, L * K), **f32), h=[torch.zeros((cap, K), **f32)], dh=[torch.zeros((cap, K), **f32)],
                    logp=torch.zeros((cap, K), **f32), loss=torch.zeros(4, **f32))

    def ragged_train_workspace(self, rows, B):
        """the model's one RaggedTrainWorkspace, with room for `rows` frames of `B` utterances"""
        ws = getattr(self, "_rtws", None)
        if ws is None:
            ws = self._rtws = RaggedTrainWorkspace(self)
        ws.reserve(self, rows=rows, B=B)
        ws.reserve_bytes(self, rows, B)
        return ws

    def forward_ragged_train(self, ws, X, ro, update_moving=True):
        """training-mode forward on X [total_T, D] (float32, contiguous, on the device: the GEMM operand as it stands, which
        must stay alive until backward_ragged has run) with the offsets ro (host int64 [B + 1], already checked by
        ragged_pass.ragged_input; no empty utterance).  ws: ragged_train_workspace(total_T, B).  Returns the model output, B
        rows at the front of a workspace buffer."""
        ws.B, ws.R, ws.x = len(ro) - 1, int(X.shape[0]), X
        ws.max_T = int((ro[1:] - ro[:-1]).max()) if ws.B else 0
        ws.ro_table, (ws.ro_dev,) = upload_int64([ro], self.device)
        return self._forward_levels(ws, ws.R, True, update_moving)[:ws.B]

    def backward_ragged(self, ws):
        """the backward pass of forward_ragged_train (dh[-1][:B] holds d loss / d logits).  Fills flat_grad (overwrites)."""
        self._backward_levels(ws, ws.R)


def create(input_shape, num_outputs, output_activation="log_softmax", L=2, H=512, seed=None, device=None,
           compute_dtype="float32", dropout_rate=0.4):
    """output_activation: "log_softmax" (the reference's default), "softmax" or None (logits).  L levels of width H.
    dropout_rate: the reference's fixed rate (0.4) by default; 0 serves tests."""
    return MultilevelAttentionModel(input_shape, num_outputs, L=L, H=H, dropout_rate=dropout_rate,
                                    output_activation=output_activation or None, seed=seed, device=device,
                                    compute_dtype=compute_dtype)


loader = create      # lidbox/models/keras_utils.py:134 calls `model_module.loader(...)`


def as_embedding_extractor(model):
    """The concatenated attention outputs [B, L*K] (the input of the `outputs` layer) in inference mode.  The reference has
    no as_embedding_extractor for this model (lidbox/models/multilevel_attention.py defines `create` alone); this one follows
    the other models' convention of cutting in front of the classification layer."""
    return EmbeddingExtractor(model)


__all__ = ["MultilevelAttentionModel", "RaggedTrainWorkspace", "EmbeddingExtractor", "as_embedding_extractor", "create", "loader"]
