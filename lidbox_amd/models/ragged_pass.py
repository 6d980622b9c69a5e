"""
What every model with a ragged pass shares.  A ragged pass is float32 inference on B utterances of DIFFERENT lengths in one pass:
X [total_T, C] float32, contiguous, on the HIP device, holds the utterances end to end; utterance b = rows row_offsets[b] ..
row_offsets[b + 1] (host array of B + 1 entries: the conventions of features.cmvn_ragged).  Every utterance gets what the dense
pass gives it alone, up to the rounding of another GEMM / pooling / recurrence path.

`RaggedPass` is the base of such a model: the refusal, the argument checks, `forward_ragged` (the template: checks, the empty
batch, the workspace, the model's own pass), `predict_ragged` / `embed_ragged` and the cache of the model's one
`RaggedWorkspace`.  A model provides

    _ragged_plan(ro, lengths)                        its host plan (models/ragged.py) and what the plan needs of the workspace,
                                                     {capacity name: count}
    _ragged_buffers_<capacity>(cap)                  the buffers sized by that capacity, {attribute name: tensor}
    _ragged_pass(ws, plan, X, ro, upto_embedding)    the launches; returns a buffer of the workspace, utterances in its rows
    _ragged_embedding_dim()                          the width of what upto_embedding returns (`output_dim`: of the output)

and, where it needs them, `ragged_refusal()` and `_ragged_check_lengths(lengths)`.  `upload_int64` is the one upload of a
pass's host tables; `EmbeddingExtractor` is what every model module's `as_embedding_extractor` returns.
"""
import ctypes

import numpy as np
import torch

from .. import _native as nv


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


def upload_int64(arrays, device):
    """the host arrays end to end in ONE int64 device tensor; returns (the tensor, which the caller keeps while the pointers
    are in use, [pointer to the first word of every array])"""
    arrays = [np.asarray(a).reshape(-1) for a in arrays]
    tensor = torch.from_numpy(np.concatenate(arrays).astype(np.int64, copy=False)).to(device)
    ptrs, at = [], tensor.data_ptr()
    for a in arrays:
        ptrs.append(ctypes.c_void_p(at))
        at += 8 * a.size
    return tensor, ptrs


class RaggedWorkspace:
    """Device buffers of a model's ragged pass, sized by named capacities (`cap_rows` rows and `cap_B` utterances in every
    model; crnn's `cap_rec`, clstm's `cap_frames`); a pass that needs less of a capacity uses the front of its buffers.  The
    buffers of capacity <name> come from the model's `_ragged_buffers_<name>(cap)` as a dict, whose entries become
    attributes (`buffers_prefix`: a subclass with buffers of its own names another family of such methods)."""

    buffers_prefix = "_ragged_buffers_"

    def __init__(self, model):
        self.cap_rows = self.cap_B = self.B = 0
        self.gemm_ws = torch.empty(16, dtype=torch.uint8, device=model.device)

    def reserve(self, model, **needs):
        """a capacity that is exceeded becomes at least half as large again; only its own buffers are replaced"""
        for name, n in needs.items():
            cap = getattr(self, "cap_" + name, 0)
            if n > cap:
                cap = max(int(n), cap + cap // 2)
                setattr(self, "cap_" + name, cap)
                self.__dict__.update(getattr(model, self.buffers_prefix + name)(cap))

    def reserve_gemm_ws(self, model, nbytes):
        if nbytes > self.gemm_ws.numel():
            self.gemm_ws = torch.empty(int(nbytes), dtype=torch.uint8, device=model.device)


class RaggedPass:
    """Base of a model with a ragged pass (see the module docstring)."""

    def ragged_refusal(self):
        """why this model has no ragged pass (None: it has one)"""
        return None

    def _ragged_check_lengths(self, lengths):
        """a model's own demand on the utterance lengths (ValueError), checked on the host in front of everything else"""

    def ragged_workspace(self, **needs):
        """the model's one RaggedWorkspace, with room for what `needs` {capacity name: count} asks"""
        ws = getattr(self, "_rws", None)
        if ws is None:
            ws = self._rws = RaggedWorkspace(self)
        ws.reserve(self, **needs)
        return ws

    def forward_ragged(self, X, row_offsets, upto_embedding=False):
        """Inference on utterances of different lengths in one pass (X, row_offsets: the module docstring).  Returns a view of
        the workspace, [B, D]: the model output or, upto_embedding, the model's embedding (`_ragged_embedding_dim` has its
        width).  What the pass runs: the model's `_ragged_pass`."""
        reason = self.ragged_refusal()
        if reason:
            raise ValueError(reason)
        X, ro, lengths = ragged_input(X, row_offsets, self.model_input_dim)
        self._ragged_check_lengths(lengths)
        B = len(lengths)
        with torch.cuda.device(self.device):
            if B == 0:
                D = self._ragged_embedding_dim() if upto_embedding else self.output_dim
                return torch.zeros((0, D), dtype=torch.float32, device=self.device)
            plan, needs = self._ragged_plan(ro, lengths)
            ws = self.ragged_workspace(**needs)
            ws.B = B
            return self._ragged_pass(ws, plan, X, ro, upto_embedding)[:B]

    def predict_ragged(self, X, row_offsets):
        """the model output [B, D] of B utterances of different lengths (a fresh tensor)"""
        return self.forward_ragged(X, row_offsets).clone()

    def embed_ragged(self, X, row_offsets):
        """the model's embedding [B, D] of B utterances of different lengths (a fresh tensor)"""
        return self.forward_ragged(X, row_offsets, upto_embedding=True).clone()


class EmbeddingExtractor:
    """Result of a model module's `as_embedding_extractor(model)`: the model's embedding in inference mode (`model.embed`),
    named "<model>:<layer>" where the model names its `embedding_layer`."""

    def __init__(self, model):
        self.model = model
        if hasattr(model, "embedding_layer"):
            self.name = model.name + ":" + model.embedding_layer

    def __call__(self, x, training=False):
        return self.model.embed(x)

    predict = __call__

    def ragged(self, X, row_offsets):
        """the embeddings [B, D] of B utterances of different lengths (`embed_ragged`)"""
        return self.model.embed_ragged(X, row_offsets)


__all__ = ["RaggedPass", "RaggedWorkspace", "EmbeddingExtractor", "ragged_input", "upload_int64"]
