"""
Host side of what the ragged passes share (models/ragged_pass.py, no GPU): the growth rule of `RaggedWorkspace` on a stub model
whose buffers are CPU tensors, the one int64 table of `upload_int64`, and the one `EmbeddingExtractor` of all model modules.
"""
import ctypes
import types

import numpy as np
import torch


class _Stub:
    """a model as RaggedWorkspace sees it: a device and one `_ragged_buffers_<capacity>` per capacity; counts the calls"""

    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _ragged_buffers_rows(self, cap):
        self.calls.append(("rows", cap))
        return dict(act=[torch.zeros((cap, 3)), torch.zeros((2 * cap + 1, 2))], x=torch.zeros((cap, 5)))

    def _ragged_buffers_B(self, cap):
        self.calls.append(("B", cap))
        return dict(pooled=torch.zeros((cap, 4)), h=[torch.zeros((cap, 2))])

    def _ragged_buffers_rec(self, cap):
        self.calls.append(("rec", cap))
        return dict(hseq=torch.zeros((cap, 6)))


def _grow(cap, n):
    """the rule, written out: a capacity that is exceeded becomes the request, or half as large again if that is more"""
    return cap if n <= cap else max(n, cap + cap // 2)


def test_workspace_growth_sequence_and_what_is_replaced():
    from lidbox_amd.models.ragged_pass import RaggedWorkspace
    m = _Stub()
    ws = RaggedWorkspace(m)
    assert (ws.cap_rows, ws.cap_B, ws.B) == (0, 0, 0) and not hasattr(ws, "cap_rec")
    # equal, smaller, + 1, x 3 of each capacity, one capacity at a time and together
    requests = [dict(rows=10, B=4), dict(rows=10, B=4), dict(rows=7, B=1), dict(rows=11, B=4), dict(rows=11, B=5),
                dict(rows=45, B=6), dict(rows=45, B=18, rec=3), dict(rows=1, B=1, rec=3), dict(rows=46, B=19, rec=4),
                dict(rows=46, B=19, rec=12)]
    want = dict(rows=0, B=0, rec=0)
    expected_caps = []
    for req in requests:
        before = {n: getattr(ws, a) for n, a in (("rows", "x"), ("B", "pooled"), ("rec", "hseq")) if hasattr(ws, a)}
        lists = (getattr(ws, "act", None), getattr(ws, "h", None))
        calls = len(m.calls)
        ws.reserve(m, **req)
        grown = [n for n in req if req[n] > want[n]]
        want = {n: _grow(want[n], req.get(n, 0)) for n in want}
        expected_caps.append((want["rows"], want["B"], want["rec"]))
        assert (ws.cap_rows, ws.cap_B, getattr(ws, "cap_rec", 0)) == expected_caps[-1], req
        # one call of the model per outgrown capacity, with the new capacity; the other capacities keep their very buffers
        assert m.calls[calls:] == [(n, want[n]) for n in grown], (req, m.calls[calls:])
        for n, a in (("rows", "x"), ("B", "pooled"), ("rec", "hseq")):
            if n in before:
                assert (getattr(ws, a) is before[n]) == (n not in grown), (req, n)
        assert (ws.act is lists[0]) == ("rows" not in grown) and (ws.h is lists[1]) == ("B" not in grown)
        assert ws.x.shape[0] == ws.act[0].shape[0] == ws.cap_rows and ws.act[1].shape[0] == 2 * ws.cap_rows + 1
        assert ws.pooled.shape[0] == ws.h[0].shape[0] == ws.cap_B
    # the sequence in figures: 11 > 10 gives 15 (half as large again), 45 > 15 gives 45 (the request); 5 > 4 gives 6, 18 > 6
    # gives 18, 19 > 18 gives 27; 4 > 3 gives 4, 12 > 4 gives 12
    assert expected_caps == [(10, 4, 0), (10, 4, 0), (10, 4, 0), (15, 4, 0), (15, 6, 0), (45, 6, 0), (45, 18, 3), (45, 18, 3),
                             (67, 27, 4), (67, 27, 12)]
    assert ws.hseq.shape[0] == ws.cap_rec == 12


def test_gemm_workspace_never_shrinks():
    from lidbox_amd.models.ragged_pass import RaggedWorkspace
    m = _Stub()
    ws = RaggedWorkspace(m)
    assert ws.gemm_ws.dtype == torch.uint8 and ws.gemm_ws.numel() == 16
    sizes = []
    for nbytes in (16, 8, 17, 17, 4096, 100, 4097, 0):
        held = ws.gemm_ws
        ws.reserve_gemm_ws(m, nbytes)
        sizes.append(ws.gemm_ws.numel())
        assert (ws.gemm_ws is held) == (nbytes <= held.numel())
    assert sizes == [16, 16, 17, 17, 4096, 4096, 4097, 4097]
    assert not m.calls


def test_upload_is_one_tensor_with_pointers_at_word_offsets():
    from lidbox_amd.models.ragged_pass import upload_int64
    arrays = [np.arange(4, dtype=np.int64), np.arange(6, dtype=np.int64).reshape(3, 2) + 10, np.array([7], np.int32)]
    t, ptrs = upload_int64(arrays, "cpu")
    assert t.dtype == torch.int64 and t.tolist() == [0, 1, 2, 3, 10, 11, 12, 13, 14, 15, 7]
    assert [p.value for p in ptrs] == [t.data_ptr() + 8 * w for w in (0, 4, 10)]
    assert ctypes.cast(ptrs[1], ctypes.POINTER(ctypes.c_int64))[5] == 15


def test_one_embedding_extractor_for_every_module():
    from lidbox_amd.models import bi_gru, cnn, multilevel_attention, ragged_pass, spherespeaker, tdnn, xvector
    for mod in (tdnn, bi_gru, spherespeaker, multilevel_attention):
        assert mod.EmbeddingExtractor is ragged_pass.EmbeddingExtractor, mod.__name__
        assert callable(getattr(mod.EmbeddingExtractor, "predict")) and callable(getattr(mod.EmbeddingExtractor, "ragged"))
    # an x-vector model names its embedding layer, and so does its extractor
    model = types.SimpleNamespace(name="x-vector", embedding_layer="segment1", embed=lambda x: ("embed", x),
                                  embed_ragged=lambda X, ro: ("embed_ragged", X, ro))
    for mod in (xvector, cnn):
        e = mod.as_embedding_extractor(model)
        assert type(e) is ragged_pass.EmbeddingExtractor and e.model is model
        assert e.name == model.name + ":" + model.embedding_layer == "x-vector:segment1"
        assert e(1) == e.predict(1) == ("embed", 1) and e.ragged(2, 3) == ("embed_ragged", 2, 3)
    # a model without a named embedding layer gives an extractor without a name
    m = multilevel_attention.create((50, 8), 5, H=24, device="cpu", seed=0)
    for mod in (bi_gru, spherespeaker, multilevel_attention):
        assert not hasattr(mod.as_embedding_extractor(m), "name")
