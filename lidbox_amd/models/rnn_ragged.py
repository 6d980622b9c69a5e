"""
The ragged pass of the recurrent engines (`rnn.RecurrentModel`, `gru_rnn.GRUModel`, `spherespeaker.SphereSpeakerModel`): what
`SequentialTDNN.forward_ragged` is to the x-vector family.  Float32 inference on B utterances of DIFFERENT lengths in one pass:

    lidbox_ragged_pack_rows (pad = 1)  ->  per layer and direction ONE input projection GEMM over all Rp rows  ->
    lidbox_lstm_ragged_fwd / lidbox_gru_ragged_fwd (csrc/rnn_ragged.hip: T_max launches, each over the utterances still
    running)  ->  the model's head on each utterance's own frames or final states

in the layout of `ragged.recurrent_plan`.  Every utterance gets what the dense pass gives it alone: the reverse directions start
at its own last frame, time averages run over its own frames, "the final h" is the state after its own last frame -- none of
which a zero-padded dense batch gives, because the Keras layers run without masking.

`RaggedRecurrent` is the mixin the three engines share: validation, the plan and its one upload, the workspace cache and the
public calls.  An engine provides `_ragged_buffers_rows / _ragged_buffers_utts` (what its workspace holds per row / per
utterance, `x` [cap_rows, C] among the former), `_ragged_embedding_dim()` and `_forward_ragged(ws, plan, dev, upto_embedding)`,
which finds the packed input in ws.x.
"""
import ctypes

import numpy as np
import torch

from .. import _native as nv
from .flat import _rows
from .ragged import recurrent_plan


def ragged_input(X, row_offsets, C):
    """the checks a ragged pass makes of its arguments (X [total_T, C] float32, contiguous, on the HIP device; row_offsets rising
    from 0 to total_T, no empty utterance); returns (X, the offsets as int64 [B + 1], the lengths [B])"""
    X = nv.require_gpu_tensor(X, "X", torch.float32)
    if X.dim() != 2 or X.shape[1] != C or not X.is_contiguous():
        raise ValueError("expected a contiguous input [total_T, %d], got %s" % (C, tuple(X.shape)))
    ro = np.ascontiguousarray(np.asarray(row_offsets, np.int64).reshape(-1))
    if len(ro) < 1 or ro[0] != 0 or (np.diff(ro) < 0).any() or int(ro[-1]) != X.shape[0]:
        raise ValueError("row_offsets must rise from 0 to the %d rows of X" % X.shape[0])
    lengths = np.diff(ro)
    if (lengths < 1).any():
        raise ValueError("utterance %d has length 0: every utterance needs at least one frame" % int(np.flatnonzero(lengths < 1)[0]))
    return X, ro, lengths


class RaggedRecurrentWorkspace:
    """Device buffers of the ragged recurrent pass, sized by capacity: `cap_rows` rows (frames + 2 per utterance) and `cap_B`
    utterances; a pass with fewer of either uses the front of every buffer.  The engine's `_ragged_buffers_rows(cap_rows)` /
    `_ragged_buffers_utts(cap_B)` return the buffers as dicts name -> tensor, which become attributes."""

    def __init__(self, model):
        self.cap_rows = self.cap_B = self.B = 0
        self.gemm_ws = torch.empty(16, dtype=torch.uint8, device=model.device)

    def reserve(self, model, rows, B):
        """a capacity that is exceeded becomes at least half as large again; only its own buffers are replaced"""
        if rows > self.cap_rows:
            self.cap_rows = max(int(rows), self.cap_rows + self.cap_rows // 2)
            self.__dict__.update(model._ragged_buffers_rows(self.cap_rows))
        if B > self.cap_B:
            self.cap_B = max(int(B), self.cap_B + self.cap_B // 2)
            self.__dict__.update(model._ragged_buffers_utts(self.cap_B))

    def reserve_gemm_ws(self, model, nbytes):
        if nbytes > self.gemm_ws.numel():
            self.gemm_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=model.device)


class RaggedPlanOnDevice:
    """the plan's arrays in one int64 device tensor: ro [B + 1] (the caller's row offsets), seg [B + 1], slots [3, B], first [B]
    (row of every utterance's first frame) and lengths [B], as pointers; `extra`: see below"""

    def __init__(self, plan, ro, device, extra=()):
        B = plan.B
        host = np.concatenate([ro, plan.seg, plan.slots().reshape(-1), plan.seg[:-1] + 1, plan.lengths] + list(extra)).astype(np.int64)
        self.tensor = torch.from_numpy(host).to(device)
        at = lambda words: ctypes.c_void_p(self.tensor.data_ptr() + 8 * words)
        self.ro, self.seg, self.slots, self.first, self.lengths = at(0), at(B + 1), at(2 * B + 2), at(5 * B + 2), at(6 * B + 2)
        # further int64 arrays of the caller's (the conv-recurrent pass: the offsets of its pooled levels), same upload
        self.extra, words = [], 7 * B + 2
        for e in extra:
            self.extra.append(at(words))
            words += len(e)
        self.sorted_lengths = ctypes.c_void_p(plan.sorted_lengths.ctypes.data)       # host array, read by the launcher


class RaggedRecurrent:
    """Mixin of the recurrent engines (see the module docstring)."""

    def ragged_refusal(self):
        """why this model has no ragged pass (None: it has one)"""
        if self.compute_dtype != "float32":
            return "the ragged pass computes in float32 only, this model has compute_dtype=%r" % (self.compute_dtype,)
        return None

    ragged_workspace_class = RaggedRecurrentWorkspace

    def ragged_workspace(self, rows, B):
        """the model's one RaggedRecurrentWorkspace, with room for `rows` rows and B utterances"""
        ws = getattr(self, "_rws", None)
        if ws is None:
            ws = self._rws = self.ragged_workspace_class(self)
        ws.reserve(self, rows, B)
        return ws

    def _ragged_input(self, X, row_offsets):
        """the model's refusal, then `ragged_input`"""
        reason = self.ragged_refusal()
        if reason:
            raise ValueError(reason)
        return ragged_input(X, row_offsets, self.input_dim)

    def forward_ragged(self, X, row_offsets, upto_embedding=False):
        """Inference on utterances of different lengths in one pass.  X [total_T, C] float32, contiguous, on the HIP device;
        utterance b = rows row_offsets[b] .. row_offsets[b + 1] (host array of B + 1 entries: the conventions of
        SequentialTDNN.forward_ragged).  Returns a view of the workspace, [B, D]: the model output or, upto_embedding, the
        model's embedding (`_ragged_embedding_dim` has its width) -- what the dense pass gives each utterance alone, up to the
        rounding of another GEMM / pooling path."""
        X, ro, lengths = self._ragged_input(X, row_offsets)
        B = len(lengths)
        with torch.cuda.device(self.device):
            if B == 0:
                D = self._ragged_embedding_dim() if upto_embedding else self.output_dim
                return torch.zeros((0, D), dtype=torch.float32, device=self.device)
            plan = recurrent_plan(lengths)
            ws = self.ragged_workspace(plan.Rp, B)
            ws.B = B
            dev = RaggedPlanOnDevice(plan, ro, self.device)
            nv.check(nv.lib.lidbox_ragged_pack_rows(nv.ptr(X), dev.ro, nv.ptr(ws.x), dev.seg, B, self.input_dim, 1, 0,
                                                    nv.current_stream()))
            return self._forward_ragged(ws, plan, dev, upto_embedding)[:B]

    def predict_ragged(self, X, row_offsets):
        """the model output [B, D] of B utterances of different lengths (a fresh tensor)"""
        return self.forward_ragged(X, row_offsets).clone()

    def embed_ragged(self, X, row_offsets):
        """the model's embedding [B, D] of B utterances of different lengths (a fresh tensor)"""
        return self.forward_ragged(X, row_offsets, upto_embedding=True).clone()

    # ------------------------------------------------------------------ what the engines build their passes from
    def _ragged_projection(self, ws, plan, X, K, prefixes, NG_H, zg):
        """zg [dirs][Rp][NG_H] = X W_d + b_d over all Rp rows (X: rows descriptor, K wide), one GEMM per direction"""
        st, Rp = nv.current_stream(), plan.Rp
        ws.reserve_gemm_ws(self, max(16, nv.lib.lidbox_gemm_rows_workspace(Rp, NG_H, K)))
        for d, p in enumerate(prefixes):
            nv.check(nv.lib.lidbox_gemm_nn(X, self._p(p + ".W"), NG_H, _rows(zg.data_ptr() + 4 * d * Rp * NG_H, 0, NG_H, 1, Rp), K,
                                           NG_H, nv.EPI_BIAS, self._p(p + ".b"), nv.ptr(ws.gemm_ws), ws.gemm_ws.numel(), st))

    def _ragged_lstm_layer(self, ws, plan, dev, X, K, prefixes, H, h, ld_h, hlast=None):
        """one LSTM layer: the projections into ws.zg, then the walk, which fills the layer's columns of the h sequence (h:
        address of its first column in row 0, rows ld_h floats apart), ws.cseq and, when given, hlast [B, dirs * H]"""
        self._ragged_projection(ws, plan, X, K, prefixes, 4 * H, ws.zg)
        U = [self._p(p + ".U") for p in prefixes] + [None]
        nv.check(nv.lib.lidbox_lstm_ragged_fwd(U[0], U[1], len(prefixes), plan.B, H, plan.Rp, dev.slots, dev.sorted_lengths,
                                               nv.ptr(ws.zg), ctypes.c_void_p(h), ld_h, nv.ptr(ws.cseq),
                                               None if hlast is None else nv.ptr(hlast), nv.current_stream()))


__all__ = ["RaggedRecurrent", "RaggedRecurrentWorkspace", "RaggedPlanOnDevice", "ragged_input"]
