"""
Host side of the ragged recurrent pass (no GPU): `models.ragged.recurrent_plan` against a brute-force restatement of its
definition, its refusal of empty utterances, the presence of the new entry points in the header and the ctypes table, and the
instantiations of the forward step kernels that the dense and the ragged walk share.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from lidbox_amd.models.ragged import recurrent_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_lengths():
    """the length set of the kernel tests: 70 utterances, 216 frames, shuffled with a fixed seed"""
    L = [1] * 3 + [2] * 2 + [3] * 60 + [5] * 4 + [9]
    np.random.default_rng(20).shuffle(L)
    return L


def brute_force(lengths):
    """the definition, spelled out: seg[b] = (frames ahead of b) + 2 b; slot j = the j-th longest utterance, earlier utterances
    first among equals; n_s = #{b : T_b > s}"""
    B = len(lengths)
    seg = [sum(lengths[:b]) + 2 * b for b in range(B + 1)]
    order = sorted(range(B), key=lambda b: (-lengths[b], b))
    n_s = [sum(1 for t in lengths if t > s) for s in range(max(lengths) if B else 0)]
    return seg, order, [lengths[b] for b in order], n_s


@pytest.mark.parametrize("lengths", [kernel_lengths(), [4] * 64, [7], [1], [3, 5, 3, 5, 1, 5, 3], [2, 2, 2, 9, 9, 1, 1]],
                         ids=["kernel-set", "all-equal", "B1", "B1-T1", "ties", "ties-2"])
def test_recurrent_plan_matches_its_definition(lengths):
    p = recurrent_plan(lengths)
    seg, order, sorted_lengths, n_s = brute_force(list(lengths))
    assert p.B == len(lengths) and p.Rp == sum(lengths) + 2 * len(lengths) == seg[-1]
    assert p.seg.tolist() == seg and p.order.tolist() == order
    assert p.sorted_lengths.tolist() == sorted_lengths and p.n_s.tolist() == n_s
    for a in (p.seg, p.order, p.sorted_lengths, p.n_s):
        assert a.dtype == np.int64
    slots = p.slots()
    assert slots.shape == (3, p.B) and slots.dtype == np.int64 and slots.flags.c_contiguous
    assert slots[0].tolist() == [seg[b] for b in order] and slots[1].tolist() == sorted_lengths and slots[2].tolist() == order
    # every utterance's segment holds its frames and two pad rows, and the segments tile the buffer
    assert (np.diff(p.seg) == np.asarray(lengths) + 2).all()


def test_the_kernel_length_set_is_what_the_kernel_tests_rely_on():
    L = kernel_lengths()
    p = recurrent_plan(L)
    assert len(L) == 70 and sum(L) == 216
    assert p.n_s.tolist() == [70, 67, 65, 5, 5, 1, 1, 1, 1]         # second row tiles of 6, 3 and 1 slots
    assert L != sorted(L) and L != sorted(L, reverse=True)


def test_ties_keep_the_callers_order():
    p = recurrent_plan([3, 5, 3, 5, 1, 5, 3])
    assert p.order.tolist() == [1, 3, 5, 0, 2, 6, 4]


def test_empty_batch_and_empty_utterances():
    p = recurrent_plan([])
    assert p.B == 0 and p.Rp == 0 and p.n_s.tolist() == [] and p.seg.tolist() == [0]
    for bad in ([0], [3, 0, 2], [2, -1]):
        with pytest.raises(ValueError, match="at least one frame"):
            recurrent_plan(bad)


def test_new_symbols_are_declared_and_bound():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native as nv
    header = open(os.path.join(ROOT, "include", "lidbox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("lidbox_lstm_ragged_fwd", "lidbox_gru_ragged_fwd", "lidbox_seq_avg_pool_ragged_fwd"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in nv._SIGS and hasattr(nv.lib, name), name
    assert len(nv._SIGS["lidbox_lstm_ragged_fwd"][1]) == 14 and len(nv._SIGS["lidbox_gru_ragged_fwd"][1]) == 15


def _resource_usage(build, tmp_path, name):
    """{function name: {remark field: number}} of one source compiled for gfx950 with the flags of the build"""
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, name + ".hip"),
                                         "-o", str(tmp_path / (name + ".o"))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--offload-arch=gfx950" in cmd
    usage, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
        m = re.search(r"remark: .*?(ScratchSize|LDS Size) \[bytes/\w+\]: (\d+)", line)
        if m and fn:
            usage.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    return usage


def test_one_forward_kernel_per_recurrence_serves_both_layouts(tmp_path):
    """lstm_step_fwd_kernel<VW, Rows> and gru_fwd_step_kernel<VEC, Rows> exist for every load path x {DenseRows, RaggedRows},
    nothing in either file uses scratch, a dense and a ragged instantiation of one load path have the same LDS size, and
    no copy named *_ragged_fwd_kernel is left.  Itanium names: <length><name>I <args> E, Li<n>E an int, Lb<0|1>E a bool."""
    from lidbox_amd import build
    for src, kernel, arg, paths in (("lstm_step", "lstm_step_fwd_kernel", "Li", {4, 2, 1}),
                                    ("gru", "gru_fwd_step_kernel", "Lb", {1, 0})):
        usage = _resource_usage(build, tmp_path, src)
        assert usage and all(set(u) == {"ScratchSize", "LDS Size"} for u in usage.values()), usage
        assert all(u["ScratchSize"] == 0 for u in usage.values()), usage
        assert not [k for k in usage if "_ragged_fwd_kernel" in k], sorted(usage)
        lds = {}
        for k, u in usage.items():
            m = re.search(r"\d+%sI%s(\d+)E.*?\d+(DenseRows|RaggedRows)E" % (kernel, arg), k)
            if m:
                assert (int(m.group(1)), m.group(2)) not in lds, k
                lds[int(m.group(1)), m.group(2)] = u["LDS Size"]
        assert set(lds) == {(p, rows) for p in paths for rows in ("DenseRows", "RaggedRows")}, sorted(usage)
        assert all(lds[p, "DenseRows"] == lds[p, "RaggedRows"] > 0 for p in paths), lds
        # the forward kernel exists under no other template signature
        assert sum(1 for k in usage if kernel in k) == len(lds), sorted(usage)


def test_models_have_the_methods_the_pipeline_looks_up():
    from lidbox_amd.models import bi_gru, spherespeaker
    from lidbox_amd.models.gru_rnn import GRUModel
    from lidbox_amd.models.rnn import RecurrentModel
    from lidbox_amd.models.spherespeaker import SphereSpeakerModel
    for cls in (RecurrentModel, GRUModel, SphereSpeakerModel):
        for m in ("forward_ragged", "predict_ragged", "embed_ragged", "ragged_refusal"):
            assert callable(getattr(cls, m)), (cls, m)
    assert callable(bi_gru.EmbeddingExtractor.ragged) and callable(spherespeaker.EmbeddingExtractor.ragged)
