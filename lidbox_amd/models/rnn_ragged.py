"""
The ragged pass of the recurrent engines (`rnn.RecurrentModel`, `gru_rnn.GRUModel`, `spherespeaker.SphereSpeakerModel`, and
under its Conv2D blocks `conv_rnn.ConvRecurrentModel`): the recurrent specialisation of `ragged_pass.RaggedPass`.  Float32
inference on B utterances of DIFFERENT lengths in one pass:

    lidbox_ragged_pack_rows (pad = 1)  ->  per layer and direction ONE input projection GEMM over all Rp rows  ->
    lidbox_lstm_ragged_fwd / lidbox_gru_ragged_fwd (csrc/lstm_step.hip, gru.hip: the dense forward step kernels over a
    ragged row map, T_max launches, each over the utterances still running)  ->  the model's head on each utterance's own frames or final states

in the layout of `ragged.recurrent_plan`.  Every utterance gets what the dense pass gives it alone: the reverse directions start
at its own last frame, time averages run over its own frames, "the final h" is the state after its own last frame -- none of
which a zero-padded dense batch gives, because the Keras layers run without masking.

`RaggedRecurrent` adds to the base the plan and its one upload (`RaggedPlanOnDevice`), the pack and the layer helpers.  An
engine provides `_ragged_buffers_rows / _ragged_buffers_B` (what its workspace holds per row / per utterance, `x`
[cap_rows, C] among the former), `_ragged_embedding_dim()` and `_forward_ragged(ws, plan, dev, upto_embedding)`, which finds
the packed input in ws.x.
"""
import ctypes

from .. import _native as nv
from .flat import _rows
from .ragged import recurrent_plan
from .ragged_pass import RaggedPass, upload_int64


class RaggedPlanOnDevice:
    """the plan's arrays in one int64 device tensor: ro [B + 1] (the caller's row offsets), seg [B + 1], slots [3, B], first [B]
    (row of every utterance's first frame) and lengths [B], as pointers; `extra`: further int64 arrays of the caller's (the
    conv-recurrent pass: the offsets of its pooled levels) behind them in the same upload"""

    def __init__(self, plan, ro, device, extra=()):
        self.tensor, ptrs = upload_int64([ro, plan.seg, plan.slots(), plan.seg[:-1] + 1, plan.lengths] + list(extra), device)
        self.ro, self.seg, self.slots, self.first, self.lengths = ptrs[:5]
        self.extra = ptrs[5:]
        self.sorted_lengths = ctypes.c_void_p(plan.sorted_lengths.ctypes.data)       # host array, read by the launcher


class RaggedRecurrent(RaggedPass):
    """Mixin of the recurrent engines (see the module docstring)."""

    def ragged_refusal(self):
        if self.compute_dtype != "float32":
            return "the ragged pass computes in float32 only, this model has compute_dtype=%r" % (self.compute_dtype,)
        return None

    def _ragged_plan(self, ro, lengths):
        plan = recurrent_plan(lengths)
        return plan, dict(rows=plan.Rp, B=plan.B)

    def _ragged_pass(self, ws, plan, X, ro, upto_embedding):
        """the plan's one upload, every utterance between its two pad rows in ws.x, then the engine's `_forward_ragged`"""
        dev = RaggedPlanOnDevice(plan, ro, self.device)
        nv.check(nv.lib.lidbox_ragged_pack_rows(nv.ptr(X), dev.ro, nv.ptr(ws.x), dev.seg, plan.B, self.input_dim, 1, 0,
                                                nv.current_stream()))
        return self._forward_ragged(ws, plan, dev, upto_embedding)

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


__all__ = ["RaggedRecurrent", "RaggedPlanOnDevice"]
