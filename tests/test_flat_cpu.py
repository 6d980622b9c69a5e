"""
Host-only tests of the shared model scaffolding (lidbox_amd.models.flat): the layout builder, the one initialiser, the
workspace cache and the class structure of the engines.  Models are built on the CPU device: nothing here launches a kernel.
"""
import numpy as np
import torch


def _bare():
    from lidbox_amd.models.flat import FlatParams
    m = FlatParams()
    m.device = torch.device("cpu")
    m.new_layout()
    return m


def test_layout_builder_aligns_and_keeps_order():
    m = _bare()
    m.add_param("a.W", (3, 5))              # 15 floats -> the next entry starts at 16
    m.add_param("a.b", (5,))
    m.add_bn("a_bn", 6)
    m.add_param("lstm.U", (2, 8))
    m.add_state("extra", (3,))
    assert list(m.layout) == ["a.W", "a.b", "a_bn.gamma", "a_bn.beta", "lstm.U"]
    assert [m.layout[n][0] for n in m.layout] == [0, 16, 24, 32, 40]
    assert m.num_flat == 56
    assert list(m.state_layout) == ["a_bn.moving_mean", "a_bn.moving_variance", "extra"]
    assert [m.state_layout[n][0] for n in m.state_layout] == [0, 8, 16]
    m.allocate()
    assert m.flat.numel() == m.flat_grad.numel() == 56 and m.state.numel() == 20
    assert m.count_params() == 15 + 5 + 4 * 6 + 16 + 3
    assert sorted(m.get_weights()) == sorted(list(m.layout) + list(m.state_layout))
    assert m._p("a.b").value == m.flat.data_ptr() + 4 * 16 and m._p("a.b", True).value == m.flat_grad.data_ptr() + 4 * 16
    assert m._sp("extra").value == m.state.data_ptr() + 4 * 16
    empty = _bare()
    empty.add_param("w.W", (2, 2))
    empty.allocate()
    assert empty.state.numel() == 4         # never an empty state buffer


def test_initialiser_rules_and_random_stream_order():
    from lidbox_amd.models.flat import orthogonal
    m = _bare()
    m.add_param("conv.W", (3, 3, 2, 4))
    m.add_param("lstm.W", (5, 8))
    m.add_param("lstm.U", (2, 8))
    m.add_param("lstm.b", (8,))
    m.add_param("dense.b", (8,))
    m.add_bn("bn", 4)
    m.unit_forget_biases = {"lstm.b"}
    m.allocate()
    m._init_weights(7)
    rng = np.random.default_rng(7)          # one generator, consumed in layout order
    lim = np.sqrt(6.0 / (9 * 2 + 9 * 4))
    assert np.array_equal(m.param("conv.W").numpy().ravel(), rng.uniform(-lim, lim, size=72).astype(np.float32))
    lim = np.sqrt(6.0 / (5 + 8))
    assert np.array_equal(m.param("lstm.W").numpy().ravel(), rng.uniform(-lim, lim, size=40).astype(np.float32))
    assert np.array_equal(m.param("lstm.U").numpy(), orthogonal((2, 8), rng).astype(np.float32))
    assert m.param("lstm.b").tolist() == [0, 0, 1, 1, 0, 0, 0, 0]          # the forget gate's quarter, by name only
    assert not m.param("dense.b").any()
    assert m.param("bn.gamma").tolist() == [1] * 4 and not m.param("bn.beta").any()
    assert not m.param("bn.moving_mean").any() and m.param("bn.moving_variance").tolist() == [1] * 4


def test_engines_derive_from_the_base_and_old_imports_work():
    from lidbox_amd.models import flat, gru_rnn, rnn
    from lidbox_amd.models import ap_lstm, bi_gru, crnn, multilevel_attention, spherespeaker
    from lidbox_amd.models.tdnn import SequentialTDNN, _align4, _rows
    assert rnn.orthogonal is flat.orthogonal and gru_rnn.BatchNormSpec is flat.BatchNormSpec
    assert _align4 is flat._align4 and _rows is flat._rows
    assert issubclass(SequentialTDNN, flat.FlatParams) and not issubclass(SequentialTDNN, flat.FlatModel)
    models = [ap_lstm.create((None, 40), num_lstm_units=4, device="cpu", seed=0),
              bi_gru.create((None, 40), 3, num_units=4, num_fc_units=8, device="cpu", seed=0),
              crnn.create((64, 40), 3, filters=(16,) * 5, num_units=4, device="cpu", seed=0),
              spherespeaker.create((None, 40), 3, embedding_dim=8, num_lstm_units=4, device="cpu", seed=0),
              multilevel_attention.create((None, 40), 3, L=1, H=8, device="cpu", seed=0)]
    for m in models:
        assert type(m).__mro__[1] is flat.FlatModel, type(m)
        assert m.convs == [] and m.frontend is None and m.attention is None and not m.bf16_storage
        assert m.wgrad_stream is None and m.head_wgrad_stream is None and not m.fused_output_ok()
    for m in models[1:]:                    # placeholders of the former LSTM parent are gone
        assert not hasattr(m, "lstms") and not hasattr(m, "head")


def test_workspace_cache_keeps_four():
    from lidbox_amd.models import multilevel_attention
    m = multilevel_attention.create((None, 40), 3, L=1, H=8, device="cpu", seed=0)
    ws = [m.workspace(2, T) for T in (5, 6, 7, 8)]
    assert m.workspace(2, 5) is ws[0] and isinstance(ws[0], multilevel_attention._Workspace)
    m.workspace(2, 9)                       # evicts the oldest
    assert len(m._ws) == 4 and (2, 5) not in m._ws and m.workspace(2, 9) is m._ws[(2, 9)]
    ptr, bs, T, C = ws[1].input_target()
    assert (ptr.value, bs, T, C) == (ws[1].x.data_ptr(), 6 * 40, 6, 40) and ws[1].input_view() is ws[1].x
