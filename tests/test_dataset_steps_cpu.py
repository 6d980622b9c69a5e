"""
Host side of the dataset steps and of lidbox_amd.data.pipelines (no GPU): the step lists create_dataset makes of a config,
from_steps, the host-only steps on plain dicts, the metadata readers, the draw / id / count functions of the device steps,
and the register budget of the new kernels.
"""
import logging
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def steps():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd.data import steps
    return steps


@pytest.fixture(scope="module")
def pipelines(steps):
    from lidbox_amd.data import pipelines
    return pipelines


LABELS = ["a", "b"]
INIT = {"id": ["u1", "u2"], "path": ["/x/u1.wav", "/x/u2.wav"], "label": ["b", "a"]}
FIRST = ("initialize", {"labels": LABELS, "init_data": INIT})
LOAD = [("load_audio", {"num_prefetch": None}), ("drop_empty", {})]
RMS = {"strength": 0.1, "vad_frame_length_ms": 10, "min_non_speech_length_ms": 100}
WEBRTC = {"aggressiveness": 0, "vad_frame_length_ms": 10, "min_non_speech_length_ms": 100}
AUG_TRAIN = {"type": "additive_noise", "split": "train", "noise_datadir": "/noise", "snr_list": [["noise", 0, 10]]}
AUG_DEV = {"type": "additive_noise", "split": "dev", "noise_datadir": "/noise", "snr_list": [["noise", 5, 10]]}
FEATS = {"type": "logmelspectrogram", "batch_size": 4}
EXPERIMENT = {"cache_directory": "/cache", "name": "exp1", "model": {"key": "xvector"},
              "data": {"train": {"split": "train", "shuffle_buffer_size": 1000}, "validation": {"split": "dev"},
                       "more": {"split": "train", "shuffle_buffer_size": 7}}}
POST_FULL = {"filters": {"min_shape": {"key": "input", "shape": [50, 40]}}, "chunks": {"length": 50, "step": 25},
             "normalize": {"key": "input", "batch_size": 8}, "shuffle_buffer_size": 300,
             "tensorboard": {"batch_size": 4, "num_batches": 2}, "remap_keys": {"signal": None},
             "cache": {"directory": "/cache/post", "batch_size": 16, "key": "k1", "log_interval": 50}}

# (config, split) -> the steps after `initialize`, written out from the decision logic of reference pipelines.py:32-142
PIPELINE_TABLE = [
    ({}, "train", LOAD),
    ({"post_initialize": {"shuffle_buffer_size": 10, "binary_classification": "a", "check_wav_headers": True,
                          "num_prefetched_signals": 5}}, "train",
     [("shuffle", {"buffer_size": 10}), ("convert_to_binary_classification", {"positive_class": "a"}),
      ("drop_invalid_wavs", {}), ("load_audio", {"num_prefetch": 5}), ("drop_empty", {})]),
    ({"post_initialize": {"check_wav_headers": False, "num_prefetched_signals": None}}, "train", LOAD),
    ({"pre_process": {"filters": {"min_signal_length_ms": 500}, "rms_vad": RMS, "repeat_too_short_signals": {"min_length_ms": 2000},
                      "chunks": {"length_ms": 1000, "step_ms": 500}}}, "train",
     LOAD + [("apply_filters", {"config": {"min_signal_length_ms": 500}}), ("compute_rms_vad", RMS), ("apply_vad", {}),
             ("drop_empty", {}), ("repeat_too_short_signals", {"min_length_ms": 2000}),
             ("create_signal_chunks", {"length_ms": 1000, "step_ms": 500})]),
    ({"pre_process": {"webrtcvad": WEBRTC, "rms_vad": RMS}}, "train",                # WebRTC wins when both are given
     LOAD + [("compute_webrtc_vad", WEBRTC), ("apply_vad", {}), ("drop_empty", {})]),
    ({"pre_process": {"augment": [AUG_TRAIN, AUG_DEV, dict(AUG_TRAIN, snr_list=[["music", 0, 1]])]}}, "train",
     LOAD + [("augment_signals", {"augment_configs": [AUG_TRAIN, dict(AUG_TRAIN, snr_list=[["music", 0, 1]])]})]),
    ({"pre_process": {"augment": [AUG_TRAIN, AUG_DEV]}}, "test", LOAD),              # augmentation for other splits only
    ({"pre_process": {"cache": {"directory": "/c", "batch_size": 2, "consume": False}}}, "dev",
     LOAD + [("cache", {"directory": "/c/dataset/dev", "cache_key": None, "batch_size": 2})]),
    ({"features": {"type": "kaldi", "kaldi": {"shape": [None, 23]}}, "pre_process": {"filters": {"equal": {"key": "label", "value": "a"}}}},
     "train", [("apply_filters", {"config": {"equal": {"key": "label", "value": "a"}}}), ("load_kaldi_data", {"shape": [None, 23]})]),
    ({"features": FEATS, "post_process": POST_FULL, "experiment": EXPERIMENT}, "train",
     LOAD + [("extract_features", {"config": FEATS}), ("apply_filters", {"config": POST_FULL["filters"]}),
             ("create_input_chunks", {"length": 50, "step": 25}), ("normalize", {"config": POST_FULL["normalize"]}),
             ("shuffle", {"buffer_size": 300}),
             ("consume_to_tensorboard", {"summary_dir": "/cache/xvector/exp1/tensorboard/dataset/train", "config": POST_FULL["tensorboard"]}),
             ("remap_keys", {"new_keys": {"signal": None}}),
             ("cache", {"directory": "/cache/post/dataset/train", "cache_key": "k1", "batch_size": 16}),
             ("consume", {"log_interval": 50}),
             ("shuffle", {"buffer_size": 1000})]),                                   # the first experiment dataset of the split only
    ({"features": FEATS, "experiment": EXPERIMENT}, "dev", LOAD + [("extract_features", {"config": FEATS})]),
    ({"features": FEATS, "embeddings": {"extractors": [], "batch_size": 2, "remap_keys": {"embedding": "input", "input": None},
                                        "cache": {"directory": "/e", "batch_size": 1}}}, "test",
     LOAD + [("extract_features", {"config": FEATS}),
             ("extract_embeddings", {"config": {"extractors": [], "batch_size": 2, "remap_keys": {"embedding": "input", "input": None},
                                                "cache": {"directory": "/e", "batch_size": 1}}}),
             ("remap_keys", {"new_keys": {"embedding": "input", "input": None}}),
             ("cache", {"directory": "/e/dataset/test", "cache_key": None, "batch_size": 1}), ("consume", {"log_interval": -1})]),
]


@pytest.mark.parametrize("case", range(len(PIPELINE_TABLE)))
def test_create_dataset_step_lists(pipelines, steps, case):
    config, split, expect = PIPELINE_TABLE[case]
    plan = pipelines.create_dataset(split, LABELS, INIT, config)
    assert all(isinstance(s, steps.Step) for s in plan)
    assert [(s.key, s.kwargs) for s in plan] == [FIRST] + expect


def test_create_dataset_file_limit_is_a_lambda_step(pipelines, steps):
    plan = pipelines.create_dataset("train", LABELS, INIT, {"post_initialize": {"file_limit": 1, "shuffle_buffer_size": 3}})
    assert [s.key for s in plan] == ["initialize", "lambda", "shuffle", "load_audio", "drop_empty"]
    ds = steps.from_steps(plan[:2])
    assert [x["id"] for x in ds] == ["u1"]


# ------------------------------------------------------------------ from_steps and the host steps
def _ds():
    return [dict(id="u%d" % i, label="ab"[i % 2], signal=np.arange(i * 1000, dtype=np.float32), sample_rate=16000,
                 input=np.zeros((i, 4), np.float32)) for i in range(6)]


def test_from_steps(steps, caplog):
    Step = steps.Step
    with caplog.at_level(logging.WARNING, logger="lidbox_amd"):
        assert steps.from_steps([Step("drop_empty", {}), Step("initialize", {"labels": LABELS, "init_data": INIT})]) is None
    assert any(r.levelno == logging.CRITICAL and "'initialize'" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="lidbox_amd"):
        ds = steps.from_steps([Step("initialize", {"labels": LABELS, "init_data": INIT}), None,
                               Step("cache", {"directory": "/nowhere", "batch_size": 1, "cache_key": None}),
                               Step("consume", {"log_interval": -1}),
                               Step("remap_keys", {"new_keys": {"path": None, "id": "utt"}})])
        out = list(ds)
    assert out == [{"utt": "u1", "label": "b", "target": 1}, {"utt": "u2", "label": "a", "target": 0}]
    messages = [r.getMessage() for r in caplog.records]
    assert any("None" in m for m in messages) and any("'cache'" in m for m in messages) and any("'consume'" in m for m in messages)
    for key in ("compute_webrtc_vad", "load_kaldi_data", "drop_invalid_wavs", "convert_to_binary_classification", "no_such_step"):
        with pytest.raises(ValueError, match=key):
            steps.from_steps([Step("initialize", {"labels": LABELS, "init_data": INIT}), Step(key, {})])
    assert steps.from_steps([Step("initialize", {"labels": LABELS, "init_data": {"id": ["u1"], "label": []}})]) is None
    expected = {"apply_filters", "apply_vad", "as_supervised", "augment_by_additive_noise", "augment_signals", "cache",
                "compute_rms_vad", "consume", "consume_to_tensorboard", "create_input_chunks", "create_signal_chunks", "drop_empty",
                "extract_embeddings", "extract_features", "filter_keys_in_set", "initialize", "lambda", "load_audio", "normalize",
                "random_signal_fir_filtering", "random_signal_speed_change", "remap_keys", "repeat_too_short_signals", "shuffle"}
    assert set(steps.VALID_STEP_FUNCTIONS) == expected


def test_host_steps_on_plain_dicts(steps):
    init = list(steps.initialize(["a", "b"], {"id": ["x", "y", "z"], "label": ["b", "a", "c"]}))
    assert [x["target"] for x in init] == [1, 0, 2] and init[0] == {"id": "x", "label": "b", "target": 1}   # unknown label: one past the last
    ds = _ds()
    assert [x["id"] for x in steps.drop_empty(ds)] == ["u1", "u2", "u3", "u4", "u5"]
    assert [x["id"] for x in steps.drop_empty([{"id": "s", "signal": torch.zeros(0)}, {"id": "t", "signal": torch.zeros(1)}])] == ["t"]
    assert [x["id"] for x in steps.apply_filters(ds, {"equal": {"key": "label", "value": "b"}})] == ["u1", "u3", "u5"]
    # 187.5 ms at 16 kHz: int(float32(16000) * float32(0.1875)) = 3000 samples
    assert [x["id"] for x in steps.apply_filters(ds, {"min_signal_length_ms": 187.5})] == ["u3", "u4", "u5"]
    assert [x["id"] for x in steps.apply_filters(ds, {"min_shape": {"key": "input", "shape": [4, 4]}})] == ["u4", "u5"]
    assert [x["id"] for x in steps.apply_filters(ds, {"min_shape": {"key": "input", "shape": [1, 5]}})] == []
    both = {"equal": {"key": "label", "value": "a"}, "min_signal_length_ms": 100, "min_shape": {"key": "missing", "shape": [1]}}
    assert [x["id"] for x in steps.apply_filters(ds, both)] == ["u2", "u4"]
    assert steps.apply_filters(ds, {}) is ds                                       # no filters: the dataset itself
    out = list(steps.remap_keys(ds[:1], {"signal": None, "input": "features", "absent": "x"}))
    assert list(out[0]) == ["id", "label", "sample_rate", "features"]
    assert [sorted(x) for x in steps.filter_keys_in_set(ds[:1], {"id", "input", "nothing"})] == [["id", "input"]]
    pairs = list(steps.as_supervised([{"input": 1, "target": 2, "id": "x"}]))
    assert pairs == [(1, 2)]
    assert list(steps.lambda_fn(ds, lambda d: (x["id"] for x in d))) == ["u%d" % i for i in range(6)]


def test_shuffle_is_a_seeded_buffered_permutation(steps):
    ds = list(range(100))
    a, b, c = (list(steps.shuffle(iter(ds), 10, seed=s)) for s in (1, 1, 2))
    assert a == b and a != c and a != ds and sorted(a) == ds and sorted(c) == ds
    assert all(v <= pos + 9 for pos, v in enumerate(a))                            # element v cannot leave before it entered the buffer
    assert list(steps.shuffle(ds, 1, seed=0)) == ds
    assert sorted(steps.shuffle(ds[:5], 1000, seed=0)) == ds[:5]
    with pytest.raises(ValueError):
        steps.shuffle(ds, 0)


# ------------------------------------------------------------------ metadata, draws, ids, counts
def test_iter_metadata_file_and_noise_grouping(steps, tmp_path):
    import lidbox_amd
    p = tmp_path / "utt2path"
    p.write_text("# comment\n\nu1 /a/b.wav\n  u2 /c d/e.wav extra  \nu3\n", encoding="utf-8")
    assert list(lidbox_amd.iter_metadata_file(str(p), 2)) == [["u1", "/a/b.wav"], ["u2", "/c"], ["u3"]]
    assert list(lidbox_amd.iter_metadata_file(str(p), 1)) == [["u1"], ["u2"], ["u3"]]
    assert list(lidbox_amd.iter_metadata_file(str(p), 3))[1] == ["u2", "/c", "d/e.wav"]
    d = tmp_path / "noise"
    d.mkdir()
    (d / "id2label").write_text("n1 noise\nm1 music\nn2 noise\ns1 speech\n")
    (d / "id2path").write_text("n2 /n/2.wav\nm1 /m/1.wav\nn1 /n/1.wav\n")          # s1 has no path: the type does not appear
    grouped = steps.noise_paths_by_type(str(d))
    assert dict(grouped) == {"noise": ["/n/2.wav", "/n/1.wav"], "music": ["/m/1.wav"]} and list(grouped) == ["noise", "music"]
    assert steps.augment_by_additive_noise([], str(tmp_path / "missing"), [("noise", 0, 1)]) is None


def test_additive_noise_draws_and_ids(steps):
    snr_list = [("noise", 5, 15), ("music", -3, -3), ("noise", 0, 1)]
    counts = {"noise": 7, "music": 1}
    got = [steps.additive_noise_draws(rng, snr_list, counts) for rng in [np.random.default_rng(5)] for _ in range(50)]
    rng = np.random.default_rng(5)
    for draws in got:                                                              # replay: index first, then the snr, in float32
        assert [d[0] for d in draws] == ["noise", "music", "noise"]
        for (_, index, snr), (noise_type, lo, hi) in zip(draws, snr_list):
            assert index == int(rng.integers(0, counts[noise_type]))
            u = rng.random(dtype=np.float32)
            assert isinstance(snr, np.float32) and snr == np.float32(lo) + (np.float32(hi) - np.float32(lo)) * u
            assert 0 <= index < counts[noise_type] and lo <= snr <= hi
    assert {d[0][1] for d in got} == set(range(7)) and all(d[1][1] == 0 and d[1][2] == -3 for d in got)
    with pytest.raises(KeyError, match="babble"):
        steps.additive_noise_draws(np.random.default_rng(0), [("babble", 0, 1)], counts)
    with pytest.raises(ValueError):
        steps.additive_noise_draws(np.random.default_rng(0), [("noise", 0, 1)], {"noise": 0})
    assert steps.additive_noise_id("utt1", "noise", np.float32(12.345)) == "augmented-utt1-noise-snr12.35"
    assert steps.additive_noise_id(b"utt1", "music", -3) == "augmented-utt1-music-snr-3.00"
    assert steps.additive_noise_id("u", "n", np.float32(0.004)) == "augmented-u-n-snr0.00"


def test_repeat_and_chunk_counts(steps):
    from lidbox_amd.features import signal_ops as sg
    assert [steps.repeat_count(1000, 16000, n) for n in (0, 1, 7999, 8000, 8001, 15999, 16000, 16001, 10 ** 6)] == \
        [0, 16000, 3, 2, 2, 2, 1, 1, 1]
    assert steps.repeat_count(0, 16000, 100) == 0 and steps.repeat_count(2500, 8000, 1) == 20000
    for ms, rate, n in [(30, 44100, 1000), (30, 44100, 1323), (1, 16000, 16), (1, 16000, 17), (999, 22050, 5)]:
        want = int(np.ceil(np.float32(np.float32(1e-3 * ms) * np.float32(rate)) / np.float32(n)))
        assert steps.repeat_count(ms, rate, n) == want
    assert [int(v) for v in sg.input_chunk_counts([0, 49, 50, 74, 75, 198, 1000], 50, 25)] == [0, 0, 1, 1, 2, 6, 39]
    assert [int(v) for v in sg.input_chunk_counts([10, 11], 10, 3)] == [1, 1]
    with pytest.raises(ValueError):
        sg.input_chunk_counts([10], 0, 1)


def test_new_ops_refuse_cpu_tensors(steps):
    from lidbox_amd._native import LidboxHipError
    from lidbox_amd.features import signal_ops as sg
    with pytest.raises(LidboxHipError):
        sg.RaggedSignals(torch.zeros(8), [0], [8])
    with pytest.raises(LidboxHipError):
        sg.input_chunks([torch.zeros(10, 3)], 2, 1)
    if not torch.cuda.is_available():
        with pytest.raises(LidboxHipError):
            list(steps.repeat_too_short_signals([dict(id="u", signal=np.ones(10, np.float32), sample_rate=16000)], 1000))


# ------------------------------------------------------------------ the new kernels' register budget
def test_new_kernels_build_for_gfx950_without_scratch(steps, tmp_path):
    from lidbox_amd import _native, build
    for name in ("lidbox_mix_noise", "lidbox_mix_noise_workspace", "lidbox_signal_tile"):
        assert hasattr(_native.lib, name)
    assert _native.lib.lidbox_mix_noise_workspace(65536, 10) == 0
    assert _native.lib.lidbox_mix_noise_workspace(65537, 10) == 2 * 10 * 256 * 8
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "mix_noise.hip"),
                                         "-o", str(tmp_path / "mix_noise.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--offload-arch=gfx950" in cmd
    usage = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    kernels = [k for k in usage if "mix_reg_kernel" in k or "mix_tile_kernel" in k or "signal_tile_kernel" in k]
    assert len(kernels) == 7, sorted(usage)                                        # 3 resident forms, 3 tiled phases, tile
    assert all(usage[k] == 0 for k in kernels), usage
