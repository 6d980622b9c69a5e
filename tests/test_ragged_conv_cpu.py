"""
Host side of the ragged pass of crnn and clstm (no device): the per-level lengths and offsets of the pooled image levels, the
extended `ragged_plan` (extra pad rows for a layer that runs on a level in place) with its default unchanged, the refusal of
utterances that five poolings leave nothing of, and the new symbols in the header and the ctypes table.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRNN_LENGTHS = [32, 37, 64, 65, 100, 33, 95, 63]
CLSTM_LENGTHS = [1, 4, 20, 7, 6, 33, 2, 11]
CLSTM_CONVS = [(5, 1), (3, 2), (3, 3), (1, 1), (1, 1)]


def test_pooled_lengths_and_offsets():
    from lidbox_amd.models.conv_rnn import pooled_lengths, pooled_offsets, pooled_sizes
    lv = pooled_lengths(CRNN_LENGTHS, 5)
    assert len(lv) == 6
    for b, T in enumerate(CRNN_LENGTHS):
        # an utterance's level lengths are those of the dense workspace for it alone
        assert [int(l[b]) for l in lv] == [t for t, _ in pooled_sizes(T, 33, 5)]
    assert lv[5].tolist() == [1, 1, 2, 2, 3, 1, 2, 1]
    offs = pooled_offsets(CRNN_LENGTHS, 5)
    for l, o in zip(lv, offs):
        assert o.dtype == np.int64 and o[0] == 0 and np.array_equal(np.diff(o), l)
    # floor halving per utterance, not of the total: level 1 has 242 rows where 489 // 2 = 244
    assert int(offs[0][-1]) == 489 and int(offs[1][-1]) == 242
    # the kernel-level pool case: lengths of case a give 0, 1, 1, 3, 20, 0, 13, 3 rows
    assert pooled_lengths([1, 2, 3, 7, 40, 1, 26, 6], 1)[1].tolist() == [0, 1, 1, 3, 20, 0, 13, 3]
    assert pooled_offsets([], 2)[2].tolist() == [0]


def test_too_short_utterances_are_refused_by_name():
    from lidbox_amd.models.conv_rnn import check_pooled_lengths
    check_pooled_lengths("CRNN", CRNN_LENGTHS, 5)
    with pytest.raises(ValueError, match=r"utterance 2 has 31 frames.*too small for 5 pooling layers"):
        check_pooled_lengths("CRNN", [32, 40, 31, 5], 5)


def _plan_fields(p):
    return (list(p.pads), list(p.cum), [t.tolist() for t in p.T], p.L.tolist(), p.off.tolist(), list(p.rows))


def test_ragged_plan_default_is_unchanged_and_extra_pads_make_room():
    from lidbox_amd.models.ragged import ragged_plan
    base = ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS)
    # today's plan of these lengths, written out: pads k - 1, cum 6 6 3 1 1 1, L = max_i ceil((p_i + T_i) / cum_i)
    assert base.pads == [4, 2, 2, 0, 0, 0] and base.cum == [6, 6, 3, 1, 1, 1]
    assert base.T[3].tolist() == [1, 1, 4, 2, 1, 6, 1, 2]
    assert base.L.tolist() == [1, 2, 4, 2, 2, 7, 1, 3] and base.lead == [0] * 6
    for same in (ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS, None), ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS, {})):
        assert _plan_fields(same) == _plan_fields(base)
    ext = ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS, {3: (1, 1)})
    assert ext.pads == [4, 2, 2, 1, 0, 0] and ext.lead == [0, 0, 0, 1, 0, 0]
    assert [t.tolist() for t in ext.T] == [t.tolist() for t in base.T]
    # level 3 (cum 1) now needs T3 + 2 rows: a pad row, the frames, a pad row
    assert (ext.L >= ext.T[3] + 2).all() and (ext.L >= base.L).all()
    assert ext.L.tolist() == [3, 3, 6, 4, 3, 8, 3, 4]
    with pytest.raises(ValueError):
        ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS, {6: (1, 1)})
    with pytest.raises(ValueError):
        ragged_plan(CLSTM_LENGTHS, CLSTM_CONVS, {3: (-1, 0)})


@pytest.mark.parametrize("lengths", [CLSTM_LENGTHS, [1], [298, 98, 3, 1, 1, 17]])
def test_every_window_of_the_lstm_layout_stays_inside_its_utterance(lengths):
    """label every row of every level with its owner (utterance, frame), -1 for a zero row, None for slack; then every valid
    output frame's window, started plan.lead[i] rows on, must read its own utterance's frames t s - (k - 1) .. t s in order, with
    zero rows for the negative ones -- and at level 3 the [pad, frames, pad] segments of the recurrent walk must hold"""
    from lidbox_amd.models.ragged import ragged_plan
    plan = ragged_plan(lengths, CLSTM_CONVS, {3: (1, 1)})
    n, B = len(CLSTM_CONVS), len(lengths)
    owner = []
    for i in range(n + 1):
        rows = [None] * (plan.rows[i] + 8)
        seg = plan.seg_offsets(i)
        for b in range(B):
            assert seg[b] + plan.pads[i] + plan.T[i][b] <= seg[b + 1]
            for r in range(plan.pads[i]):
                rows[seg[b] + r] = -1
            for t in range(int(plan.T[i][b])):
                rows[seg[b] + plan.pads[i] + t] = (b, t)
        owner.append(rows)
    for i, (k, s) in enumerate(CLSTM_CONVS):
        seg_in, seg_out = plan.seg_offsets(i), plan.seg_offsets(i + 1)
        for b in range(B):
            for t in range(int(plan.T[i + 1][b])):
                r = int(seg_out[b]) + t                       # output row counted from pads[i + 1] rows into level i + 1
                assert owner[i + 1][r + plan.pads[i + 1]] == (b, t)
                win = [owner[i][r * s + plan.lead[i] + j] for j in range(k)]
                want = [(b, t * s - (k - 1) + j) if t * s - (k - 1) + j >= 0 else -1 for j in range(k)]
                assert win == want, (i, b, t, win, want)
    seg3 = plan.seg_offsets(3)
    for b in range(B):
        T3 = int(plan.T[3][b])
        assert owner[3][seg3[b]] == -1 and owner[3][seg3[b] + 1] == (b, 0) and owner[3][seg3[b] + T3] == (b, T3 - 1)
        assert seg3[b] + T3 + 2 <= seg3[b + 1] and owner[3][seg3[b] + T3 + 1] is None     # the pad row behind: nobody's frame


def test_symbols_in_header_and_ctypes_table():
    from lidbox_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "lidbox_hip.h")).read()
    assert re.search(r"#define\s+LIDBOX_HIP_ABI_VERSION\s+1\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("lidbox_conv2d_ragged_fwd", "lidbox_conv2d_strided_ragged_fwd", "lidbox_bn_maxpool2d_ragged_fwd"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in nv._SIGS and hasattr(nv.lib, name), name
    from lidbox_amd.models.clstm import CLSTM
    from lidbox_amd.models.conv_rnn import ConvRecurrentModel
    from lidbox_amd.models.tdnn import SequentialTDNN
    for cls in (ConvRecurrentModel, CLSTM):
        for attr in ("ragged_refusal", "forward_ragged", "predict_ragged", "embed_ragged"):
            assert callable(getattr(cls, attr)), (cls, attr)
    # forward_ragged is the shared template (models/ragged_pass.py); `_ragged_pass` holds a model's own pass
    assert CLSTM._ragged_pass is not SequentialTDNN._ragged_pass and CLSTM.ragged_refusal is not SequentialTDNN.ragged_refusal
