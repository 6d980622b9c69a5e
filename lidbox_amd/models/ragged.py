"""
Host plan of the ragged model pass: where utterances of DIFFERENT lengths live when a causal Conv1D stack runs over all of them in one
GEMM per layer (no reference counterpart: tf.data batches need one shape).  Pure Python on host integers; what the models do with a
plan -- the checks, the workspace, the one upload, the public calls -- is models/ragged_pass.py's.

Conv i (i = 0 .. n-1) has kernel k_i and stride s_i, padding "causal", no dilation.  Level i is the input of conv i, level n the
pooling input.  With

    p_i   = k_i - 1  (i < n),   p_n = 0            causal zero rows ahead of an utterance's frames
    cum_i = s_i s_{i+1} ... s_{n-1},   cum_n = 1
    T_{0,b} = frames of utterance b,   T_{i+1,b} = (T_{i,b} - 1) // s_i + 1

utterance b gets  L_b = max_i ceil((p_i + T_{i,b}) / cum_i)  rows at the top level and L_b cum_i rows at level i: its segment starts at
row off[b] cum_i (off = exclusive prefix sum of L) and holds p_i zero rows, its T_{i,b} frames, then slack.  Level i has
M_i = off[B] cum_i rows.  Because a level-i segment is exactly s_i times the level-(i+1) segment, ONE rows descriptor with batch = 1
and row stride s_i C_i over level i lines every utterance's causal windows up with its output rows:

    output row r (counted from p_{i+1} rows into level i+1) reads the level-i rows r s_i .. r s_i + k_i - 1
    frame t of utterance b at level i+1 is r = off[b] cum_{i+1} + t, whose window starts at level-i row off[b] cum_i + t s_i: the
    window of padded position t s_i of utterance b

so conv i is one GEMM over M_{i+1} - p_{i+1} rows.  It also writes the p_{i+1} pad rows of utterances 1 .. B-1 (zeroed again right
behind the GEMM) and the slack rows, which no valid output row ever reads: the last frame's window ends at padded position
(T_{i+1,b} - 1) s_i + k_i - 1 <= p_i + T_{i,b} - 1.  The last GEMM rows read up to k_i - 1 rows behind M_i, which the buffers have.

`recurrent_plan` is the plan of the ragged RECURRENT pass (csrc/rnn_step.h: RaggedRows): the dense [B][T + 2] convention of the recurrence
kernels with a per-utterance T.  Utterance b owns the rows seg[b] .. seg[b + 1] of every per-frame buffer of a layer, seg[b] =
row_offsets[b] + 2 b: a pad row, its T_b frames, a pad row; Rp = total_T + 2 B rows in all.  The walk through time runs step s over
the n_s = #{b : T_b > s} utterances that are still running; slot j of a step is the j-th longest utterance under a stable sort by
length, descending, so the running ones are always the leading slots.
"""
import numpy as np


class RaggedPlan:
    """pads [n+1], cum [n+1], T [n+1][B] (frames per level and utterance), L [B], off [B+1] (top-level rows, int64) and rows [n+1] = M_i;
    lead [n+1]: the part of pads[i] that is not the reading conv's causal padding (ragged_plan's extra_pads; zeros without)"""

    def __init__(self, pads, cum, T, L, off):
        self.pads, self.cum, self.T, self.L, self.off = pads, cum, T, L, off
        self.B = len(L)
        self.rows = [int(off[-1]) * c for c in cum]

    def seg_offsets(self, i):
        """start rows of the segments of level i, with the level's end as entry B (int64 [B + 1])"""
        return self.off * self.cum[i]

    def valid_rows(self, i):
        return int(self.T[i].sum())


def ragged_plan(lengths, convs, extra_pads=None):
    """lengths: frames per utterance (each >= 1); convs: (kernel, stride) pairs or objects with .k and .s.  Returns a RaggedPlan.
    extra_pads {level: (before, after)} asks for further pad rows around an utterance's frames at a level, for a layer that runs
    on that level in place (clstm's LSTM on level 3: one row each side, the [pad, frames, pad] segments of `recurrent_plan`):
    pads[level] grows by `before`, so the frames start that much deeper in the segment and the conv that reads the level must
    start its windows `before` rows on (plan.lead[level]), and the segment has room for `after` rows behind the frames."""
    ks = [(int(c.k), int(c.s)) if hasattr(c, "k") else (int(c[0]), int(c[1])) for c in convs]
    if any(k < 1 or s < 1 for k, s in ks):
        raise ValueError("kernel sizes and strides must be >= 1")
    T0 = np.asarray(lengths, np.int64).reshape(-1)
    if (T0 < 1).any():
        raise ValueError("every utterance needs at least one frame, got lengths %s" % T0[T0 < 1][:8].tolist())
    n = len(ks)
    pads = [k - 1 for k, _ in ks] + [0]
    cum = [1] * (n + 1)
    for i in range(n - 1, -1, -1):
        cum[i] = cum[i + 1] * ks[i][1]
    T = [T0]
    for _, s in ks:
        T.append((T[-1] - 1) // s + 1)
    lead, after = [0] * (n + 1), [0] * (n + 1)
    for i, (p0, p1) in (extra_pads or {}).items():
        if not 0 <= int(i) <= n or p0 < 0 or p1 < 0:
            raise ValueError("extra_pads: levels 0 .. %d, pads >= 0" % n)
        lead[i], after[i] = int(p0), int(p1)
        pads[i] += int(p0)
    L = np.zeros(len(T0), np.int64)
    for i in range(n + 1):
        L = np.maximum(L, -(-(pads[i] + T[i] + after[i]) // cum[i]))
    off = np.concatenate(([0], np.cumsum(L))).astype(np.int64)
    plan = RaggedPlan(pads, cum, T, L, off)
    plan.lead = lead
    return plan


class RecurrentPlan:
    """seg [B + 1] (first row of every segment, Rp as entry B), order [B] (the utterance of slot j), sorted_lengths [B] (its
    length: non-increasing), n_s [T_max] (utterances running at step s) -- int64 arrays -- and Rp"""

    def __init__(self, lengths, seg, order, sorted_lengths, n_s):
        self.lengths, self.seg, self.order, self.sorted_lengths, self.n_s = lengths, seg, order, sorted_lengths, n_s
        self.B = len(lengths)
        self.Rp = int(seg[-1])

    def slots(self):
        """the device table of the walk, [3, B]: per slot the utterance's first row, its length and its index"""
        return np.ascontiguousarray(np.stack([self.seg[:-1][self.order], self.sorted_lengths, self.order]))


def recurrent_plan(lengths, seg=None):
    """lengths: frames per utterance (each >= 1, ValueError otherwise).  Returns a RecurrentPlan.  seg [B + 1]: the segments of
    a caller whose [pad, frames, pad at least] segments lie elsewhere (clstm: level 3 of its `ragged_plan`); default: end to end."""
    T = np.asarray(lengths, np.int64).reshape(-1)
    if (T < 1).any():
        raise ValueError("every utterance needs at least one frame, got lengths %s" % T[T < 1][:8].tolist())
    B = len(T)
    if seg is None:
        seg = np.concatenate(([0], np.cumsum(T))).astype(np.int64) + 2 * np.arange(B + 1, dtype=np.int64)
    order = np.argsort(-T, kind="stable").astype(np.int64)
    sorted_lengths = np.ascontiguousarray(T[order])
    T_max = int(sorted_lengths[0]) if B else 0
    # n_s = #{b : T_b > s}: the sorted lengths are non-increasing, so count from the short end
    n_s = B - np.searchsorted(sorted_lengths[::-1], np.arange(T_max, dtype=np.int64), side="right").astype(np.int64)
    return RecurrentPlan(T, seg, order, sorted_lengths, n_s)
