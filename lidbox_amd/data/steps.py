"""
Counterpart of lidbox.data.steps.  `ds` is any iterable of element dicts (the reference maps the same functions over a
tf.data.Dataset); results are generators of dicts.  `from_steps` turns a list of `Step`s -- what
`lidbox_amd.data.pipelines.create_dataset` makes of a lidbox config -- into such a generator.

  device steps
  extract_features      reference steps.py:708-736   (the hot path's boundary)
  compute_rms_vad       reference steps.py:417-432   energy VAD decisions             
  apply_vad             reference steps.py:183-200   drop the non-speech frames        
  create_signal_chunks  reference steps.py:579-632   fixed-length chunks, new ids      
  random_signal_speed_change   reference steps.py:331-352   Fourier resampling at a random speed ratio
  random_signal_fir_filtering  reference steps.py:355-368   random N(0, 1) FIR filter per signal
  augment_by_additive_noise    reference steps.py:235-328   noise clips from a device-resident bank mixed in at random SNRs
  augment_signals       reference steps.py:215-229   originals and augmented copies, sampled at random
  repeat_too_short_signals     reference steps.py:950-969   tile signals up to a minimum length
  create_input_chunks   reference steps.py:558-576   windows of `input` frames, new ids
  normalize             reference steps.py:821-834   batched CMVN of one key
  extract_embeddings    reference steps.py:674-705   batched embedding extraction      
  load_audio            reference steps.py:803-818   WAV files -> `signal`, `sample_rate`

  host steps
  initialize, drop_empty, apply_filters, remap_keys, filter_keys_in_set, as_supervised, shuffle, lambda

The signal steps gather `launch_batch` elements into one ragged device batch per kernel launch
(lidbox_amd/features/signal_ops.py); the order of elements is preserved.

`extract_features(ds, config)` takes the reference's config
schema (`_feature_extraction_kwargs_to_args`, steps.py:94-104):

    {"type": "logmelspectrogram" | "mfcc" | "melspectrogram" | "spectrogram" | "db_spectrogram",
     "spectrogram": {...}, "melspectrogram": {...}, "mfcc": {...}, "db_spectrogram": {...},
     "sample_minmax_scaling": {...}, "window_normalization": {...},
     "batch_size": 1 | "group_by_input_length": {"max_batch_size": n} | "ragged_batch_size": n, "device": ...}

`ragged_batch_size: n` (lidbox_amd only, like `launch_batch` of the signal steps) puts n consecutive elements of ANY lengths into
one launch of the ragged feature kernel; every element gets what `batch_size: 1` gives it, bit for bit, and the element order is
kept.  That is the pipeline without signal chunking: VAD leaves every utterance its own length, so `group_by_input_length` finds
groups of one.  `normalize` has the matching opt-in `ragged: true`, and so has `extract_embeddings`: with it, up to `batch_size`
consecutive `input` tensors of any T go through one ragged model pass per extractor (models/ragged.py), so features, normalisation
and embeddings of un-chunked utterances all run without one launch per length.

The reference maps this over a tf.data.Dataset (batch -> map -> unbatch); here `ds` is any
iterable of element dicts holding at least `signal` (1-D float32 tensor or array) and
`sample_rate`, and the result is a generator of the same dicts with `input` ([T, C] tensor on the
HIP device) and `feature_type` added.  Not built: WebRTC VAD, Kaldi I/O, WAV header checks, on-disk caching,
TensorBoard dumps and the debug / statistics steps; `from_steps` names them instead of skipping them.
"""
import collections
import itertools
import logging
import os
import shutil

import numpy as np
import torch

from .. import features
from .. import iter_metadata_file
from ..features import audio as audio_features
from ..features import signal_ops
from . import tf_utils

logger = logging.getLogger("lidbox_amd")

VALID_FEATURE_ARGS = ["type", "spectrogram", "melspectrogram", "mfcc", "db_spectrogram", "sample_minmax_scaling",
                      "window_normalization"]


def _feature_extraction_kwargs_to_args(config):
    """reference steps.py:94-104"""
    return [config.get(arg, {}) for arg in VALID_FEATURE_ARGS]


def _get_device_or_default(config):
    """reference steps.py:115-122 -- there is no CPU path here: the default IS the HIP device."""
    dev = config.get("device", "cuda")
    if isinstance(dev, str):
        name = dev.upper().lstrip("/")
        if name.startswith("GPU"):
            dev = "cuda" + (":" + name[4:] if name[3:4] == ":" and name[4:] else "")
        elif name.startswith("CPU"):
            raise ValueError("lidbox_amd extracts features on the HIP device only (got device=%r)" % (config.get("device"),))
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise ValueError("lidbox_amd extracts features on the HIP device only (got device=%r)" % (config.get("device"),))
    return dev


def _batches(ds, config):
    if "group_by_input_length" in config:
        # reference steps.py:725-728 + group_by_axis_length (:751-773): same-length batches of bounded size
        max_bs = int(config["group_by_input_length"]["max_batch_size"])
        groups = {}
        for x in ds:
            n = int(torch.as_tensor(x["signal"]).shape[0])
            g = groups.setdefault(n, [])
            g.append(x)
            if len(g) == max_bs:
                yield groups.pop(n)
        for g in groups.values():
            if g:
                yield g
    else:
        bs = int(config.get("batch_size", 1))                                        # reference steps.py:730
        batch = []
        for x in ds:
            if batch and int(torch.as_tensor(x["signal"]).shape[0]) != int(torch.as_tensor(batch[0]["signal"]).shape[0]):
                raise ValueError("cannot batch signals of different lengths; use group_by_input_length")
            batch.append(x)
            if len(batch) == bs:
                yield batch
                batch = []
        if batch:
            yield batch


def extract_features(ds, config):
    """reference lidbox/data/steps.py:708-736"""
    feature_type = config["type"]
    args = _feature_extraction_kwargs_to_args(config)
    device = _get_device_or_default(config)
    logger.info("Extracting '%s' features on device '%s' with arguments:\n  %s", feature_type, device,
                "\n  ".join(repr(a) for a in args[1:]))
    if "ragged_batch_size" in config:
        yield from _extract_features_ragged(ds, config, feature_type, args, device)
        return
    for batch in _batches(ds, config):
        sigs = [torch.as_tensor(x["signal"]) for x in batch]
        if not all(t.dtype == torch.int16 for t in sigs):                            # 16-bit PCM stays int16: the kernel reads it in place
            sigs = [t.to(torch.float32) for t in sigs]
        signals = torch.stack(sigs).to(device)
        rates = [int(x["sample_rate"]) for x in batch]
        feats = tf_utils.extract_features(signals, rates, *args)
        for x, f in zip(batch, feats.unbind(0)):                                     # unbatch (:736): one call for all the views
            yield dict(x, input=f, feature_type=feature_type)


def _extract_features_ragged(ds, config, feature_type, args, device):
    """`ragged_batch_size: n`: n elements of any lengths per feature launch (tf_utils.extract_features_ragged), in input order"""
    if "group_by_input_length" in config:
        raise ValueError("ragged_batch_size and group_by_input_length exclude each other: a ragged batch needs no equal lengths")
    n = int(config["ragged_batch_size"])
    if n < 1:
        raise ValueError("ragged_batch_size must be at least 1")
    for batch in _launch_batches(ds, n):
        sigs = [torch.as_tensor(x["signal"]) for x in batch]
        # 16-bit PCM: scaled as the dense call reads it in place (value / 32768)
        sigs = [audio_features.pcm16_to_float(t, 1, device=device) if t.dtype == torch.int16 else t for t in sigs]
        rates = [int(x["sample_rate"]) for x in batch]
        feats = tf_utils.extract_features_ragged(signal_ops.RaggedSignals.from_list(sigs, device=device), rates, *args)
        for x, f in zip(batch, feats):
            yield dict(x, input=f, feature_type=feature_type)


# ------------------------------------------------------------------ signal steps
def _launch_batches(ds, launch_batch):
    batch = []
    for x in ds:
        batch.append(x)
        if len(batch) == launch_batch:
            yield batch
            batch = []
    if batch:
        yield batch


def _vad_frame_length(sample_rate, vad_frame_length_ms):
    """reference steps.py:192-193: int32(float32(sr) * (1e-3 * float32(ms)))"""
    sec = np.float32(1e-3) * np.float32(vad_frame_length_ms)
    return int(np.float32(sample_rate) * sec)


def compute_rms_vad(ds, strength, vad_frame_length_ms, min_non_speech_length_ms=0, launch_batch=256):
    """reference steps.py:417-432: adds `vad_is_speech` (bool [num_frames], on the HIP device) and
    `vad_frame_length_ms` to every element."""
    logger.info("Computing voice activity detection decisions by mean RMS values on %d ms long windows.\n"
                "Minimum length of continuous non-speech segment before it is marked as non-speech is %d ms.",
                vad_frame_length_ms, min_non_speech_length_ms)
    for batch in _launch_batches(ds, launch_batch):
        by_rate = {}
        for i, x in enumerate(batch):
            by_rate.setdefault(int(x["sample_rate"]), []).append(i)
        decisions = [None] * len(batch)
        for rate, idx in by_rate.items():
            frame_step = audio_features.ms_to_frames(rate, vad_frame_length_ms)
            min_frames = int(audio_features.ms_to_frames(rate, min_non_speech_length_ms) / frame_step)
            r = signal_ops.RaggedSignals.from_list([batch[i]["signal"] for i in idx])
            vad = signal_ops.vad_decisions(r, frame_step, min_frames, strength)
            for i, d in zip(idx, signal_ops.split_frames(vad, vad["decisions"])):
                decisions[i] = d.to(torch.bool)
        for x, d in zip(batch, decisions):
            yield dict(x, vad_is_speech=d, vad_frame_length_ms=vad_frame_length_ms)


def apply_vad(ds, launch_batch=256):
    """reference steps.py:183-200: `signal` keeps only the frames whose `vad_is_speech` is set; the two VAD keys
    are dropped."""
    logger.info("Using previously computed voice activity decisions to drop signal frames marked as non-speech.")
    drop_keys_after_done = {"vad_frame_length_ms", "vad_is_speech"}
    for batch in _launch_batches(ds, launch_batch):
        by_len = {}
        for i, x in enumerate(batch):
            by_len.setdefault(_vad_frame_length(x["sample_rate"], x["vad_frame_length_ms"]), []).append(i)
        voiced = [None] * len(batch)
        for L, idx in by_len.items():
            r = signal_ops.RaggedSignals.from_list([batch[i]["signal"] for i in idx])
            dev = r.flat.device
            decs = [torch.as_tensor(batch[i]["vad_is_speech"]).to(device=dev, dtype=torch.uint8).reshape(-1) for i in idx]
            nf = r.lengths_host // L
            for i, d, n in zip(idx, decs, nf):
                if d.numel() != n:
                    raise ValueError("element %r: %d VAD decisions for %d frames" % (batch[i].get("id"), d.numel(), n))
            fo_h, fo_d = signal_ops._csr(nf, dev)
            dec = torch.cat(decs) if decs else torch.zeros(0, dtype=torch.uint8, device=dev)
            slots = torch.empty(int(fo_h[-1]), dtype=torch.int32, device=dev)
            counts = torch.zeros(r.B, dtype=torch.int32, device=dev)
            from .. import _native as nv
            with torch.cuda.device(dev):
                nv.check(nv.lib.lidbox_vad_scan(nv.ptr(dec), nv.ptr(fo_d), r.B, nv.ptr(slots), nv.ptr(counts),
                                                nv.current_stream()))
            out = signal_ops.apply_vad(r, dict(decisions=dec, slots=slots, counts=counts, frame_offsets_host=fo_h,
                                               frame_offsets=fo_d, frame_len=L))
            for i, v in zip(idx, out.split()):
                voiced[i] = v
        for x, v in zip(batch, voiced):
            yield {k: val for k, val in dict(x, signal=v).items() if k not in drop_keys_after_done}


def create_signal_chunks(ds, length_ms, step_ms, max_pad_ms=0, deterministic_output_order=True,
                         max_num_chunks_per_signal=int(1e6), avg_num_chunks_from_signals=100, launch_batch=256):
    """reference steps.py:579-632: every signal becomes its fixed-length chunks; `id` gets the 1-based chunk
    number appended (zero padded to round(log10(max_num_chunks_per_signal)) digits), `duration` is recomputed.
    Output order is the deterministic one (`deterministic_output_order` and the interleave block length only
    affect tf.data scheduling in the reference)."""
    logger.info("Dividing every signal in the dataset into new signals by creating signal chunks of length %d ms and "
                "offset %d ms. Maximum amount of padding allowed in the last chunk is %d ms.", length_ms, step_ms, max_pad_ms)
    id_str_padding = int(round(float(np.log10(np.float32(max_num_chunks_per_signal)))))              # steps.py:589
    for batch in _launch_batches(ds, launch_batch):
        by_rate = {}
        for i, x in enumerate(batch):
            by_rate.setdefault(int(x["sample_rate"]), []).append(i)
        chunks_of = [None] * len(batch)
        for rate, idx in by_rate.items():
            r = signal_ops.RaggedSignals.from_list([batch[i]["signal"] for i in idx])
            for n in r.lengths_host:
                L, S, _, _ = signal_ops.chunk_plan(n, rate, length_ms, step_ms, max_pad_ms)
                if max(0, 1 + (int(n) - L) // S) >= max_num_chunks_per_signal:                       # steps.py:608
                    raise ValueError("Too many chunks created from signal, cannot create unique utterance ids, raise "
                                     "the max_num_chunks_per_signal parameter")
            chunks, nch = signal_ops.signal_chunks(r, rate, length_ms, step_ms, max_pad_ms)
            c0 = 0
            for i, n in zip(idx, nch):
                chunks_of[i] = chunks[c0:c0 + int(n)]
                c0 += int(n)
        for x, ch in zip(batch, chunks_of):
            for k in range(ch.shape[0]):
                out = dict(x, signal=ch[k], id="%s-%s" % (x["id"], str(k + 1).zfill(id_str_padding)))
                if "duration" in x:
                    out["duration"] = float(np.float32(ch.shape[1] / int(x["sample_rate"])))          # steps.py:597
                yield out


# ------------------------------------------------------------------ augmentation (csrc/augment.hip)
def _selected(batch, flag):
    """indexes of the elements a step processes: all, or those whose x[flag] is truthy (reference `if flag and not x[flag]`)"""
    return [i for i, x in enumerate(batch) if not (flag and not x[flag])]


def speed_change_rate(rng, sample_rate, min, max):
    """one draw of steps.py:343-345 in float32: ratio = min + (max - min) * u, u = rng.random(float32);
    in_rate = int32(ratio * float32(sample_rate)) truncated as tf.cast does"""
    u = rng.random(dtype=np.float32)
    ratio = np.float32(min) + (np.float32(max) - np.float32(min)) * u
    return int(np.float32(ratio) * np.float32(sample_rate))


def _augmented(batch, idx, signals):
    out = list(batch)
    for i, s in zip(idx, signals):
        out[i] = dict(batch[i], signal=s)
    return out


def random_signal_speed_change(ds, min, max, flag=None, seed=None, launch_batch=256):
    """reference steps.py:331-352: every selected signal is resampled (scipy.signal.resample semantics) from
    (N * sample_rate) // in_rate samples, in_rate = sample_rate times a ratio drawn uniformly from [min, max]
    (`speed_change_rate`; one np.random.default_rng(seed) per call, one draw per selected element in element order,
    so the output does not depend on launch_batch).  The output length is exact where the reference's int32 product
    wraps (signal_ops.resample_length)."""
    logger.info("Applying random resampling to signals with a random speed ratio chosen uniformly at random from [%.3f, %.3f]",
                min, max)
    rng = np.random.default_rng(seed)
    for batch in _launch_batches(ds, launch_batch):
        idx = _selected(batch, flag)
        if not idx:
            yield from batch
            continue
        r = signal_ops.RaggedSignals.from_list([batch[i]["signal"] for i in idx])
        m = []
        for i, n in zip(idx, r.lengths_host):
            sr = int(batch[i]["sample_rate"])
            in_rate = speed_change_rate(rng, sr, min, max)
            if in_rate <= 0:
                raise ValueError("element %r: speed ratio gives an input rate of %d" % (batch[i].get("id"), in_rate))
            m.append(signal_ops.resample_length(n, in_rate, sr))
        yield from _augmented(batch, idx, signal_ops.resample(r, m).split())


def random_signal_fir_filtering(ds, num_coefs=10, flag=None, seed=None, launch_batch=256):
    """reference steps.py:355-368: every selected signal goes through lfilter(f, 1.0, signal) with num_coefs coefficients
    drawn as np.random.default_rng(seed).standard_normal(num_coefs, dtype=np.float32), one draw per selected element in
    element order (independent of launch_batch)."""
    logger.info("Applying random FIR filters of size %d on signals", num_coefs)
    rng = np.random.default_rng(seed)
    num_coefs = int(num_coefs)
    for batch in _launch_batches(ds, launch_batch):
        idx = _selected(batch, flag)
        if not idx:
            yield from batch
            continue
        coefs = np.stack([rng.standard_normal(num_coefs, dtype=np.float32) for _ in idx])
        r = signal_ops.RaggedSignals.from_list([batch[i]["signal"] for i in idx])
        yield from _augmented(batch, idx, signal_ops.fir_filter(r, torch.from_numpy(coefs)).split())


# ------------------------------------------------------------------ additive noise (csrc/mix_noise.hip)
def noise_paths_by_type(noise_datadir):
    """steps.py:252-256: `noise_datadir/id2label` (noise id, noise type) and `id2path` (noise id, path) ->
    {noise type: [paths]} in file order.  Host only."""
    id2type = dict(iter_metadata_file(os.path.join(noise_datadir, "id2label"), 2))
    type2paths = collections.OrderedDict()
    for noise_id, path in iter_metadata_file(os.path.join(noise_datadir, "id2path"), 2):
        type2paths.setdefault(id2type[noise_id], []).append(path)
    return type2paths


def additive_noise_draws(rng, snr_list, type_counts):
    """the draws of steps.py:281-285 for ONE element: for every (noise_type, snr_low, snr_high) of snr_list, in order, first
    the clip index rng.integers(0, type_counts[noise_type]), then snr = low + (high - low) * rng.random(float32) in float32
    -> [(noise_type, index, snr)]"""
    draws = []
    for noise_type, snr_low, snr_high in snr_list:
        if noise_type not in type_counts:
            raise KeyError("noise type %r of snr_list is not in the noise directory (types: %s)"
                           % (noise_type, ", ".join(sorted(type_counts))))
        count = int(type_counts[noise_type])
        if count < 1:
            raise ValueError("noise type %r has no clips" % (noise_type,))
        index = int(rng.integers(0, count))
        u = rng.random(dtype=np.float32)
        snr = np.float32(np.float32(snr_low) + (np.float32(snr_high) - np.float32(snr_low)) * u)
        draws.append((noise_type, index, snr))
    return draws


def additive_noise_id(utt_id, noise_type, snr):
    """steps.py:309-316: "augmented-<id>-<noise type>-snr<snr with two decimals>" """
    if isinstance(utt_id, bytes):
        utt_id = utt_id.decode("utf-8")
    return "augmented-%s-%s-snr%.2f" % (utt_id, noise_type, float(np.float32(snr)))


def _copy_noise_files_to_tmpdir(type2paths):
    """steps.py:258-269"""
    tmpdir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "lidbox_noise_signals")
    logger.info("Copying all noise files to TMPDIR '%s'", tmpdir)
    copied = collections.OrderedDict()
    for noise_type, paths in type2paths.items():
        copied[noise_type] = []
        for src in paths:
            dst = os.path.join(tmpdir, noise_type, os.path.basename(src))
            logger.debug("%s -> %s", src, dst)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(src, dst)
            copied[noise_type].append(dst)
    return copied


def augment_by_additive_noise(ds, noise_datadir, snr_list, copy_noise_files_to_tmpdir=False, seed=None, launch_batch=256):
    """reference steps.py:235-328.  Every element yields len(snr_list) NEW elements, in snr_list order, and not itself: its
    signal mixed (audio.snr_mixer, third value) with a clip of the given noise type drawn from `noise_datadir`, repeated to the
    signal's length, at an SNR drawn from [snr_low, snr_high]; `id` becomes `additive_noise_id(...)`, other keys are carried.
    All clips are read once into one bank on the device.  Draws: one np.random.default_rng(seed) per call,
    `additive_noise_draws` per element in element order, so the output does not depend on launch_batch.
    Returns None (after logging the reference's error) when `noise_datadir` does not exist."""
    logger.info("Augmenting dataset with additive noise from '%s'.", noise_datadir)
    if not os.path.isdir(noise_datadir):
        logger.error("Noise source dir '%s' does not exist.", noise_datadir)
        return None
    type2paths = noise_paths_by_type(noise_datadir)
    snr_list = [tuple(s) for s in snr_list]
    for noise_type, _, _ in snr_list:
        if noise_type not in type2paths:
            raise KeyError("noise type %r of snr_list is not in '%s' (types: %s)"
                           % (noise_type, noise_datadir, ", ".join(sorted(type2paths))))
    if copy_noise_files_to_tmpdir:
        type2paths = _copy_noise_files_to_tmpdir(type2paths)
    clips, rates, first = [], [], {}
    for noise_type, paths in type2paths.items():
        first[noise_type] = len(clips)
        for path in paths:
            signal, rate = audio_features.read_wav(path)
            clips.append(signal)
            rates.append(int(rate))
    bank = signal_ops.RaggedSignals.from_list(clips)
    type_counts = {t: len(p) for t, p in type2paths.items()}
    rng = np.random.default_rng(seed)

    def mixed():
        for batch in _launch_batches(ds, launch_batch):
            src, clip, snrs, ids = [], [], [], []
            for i, x in enumerate(batch):
                for noise_type, index, snr in additive_noise_draws(rng, snr_list, type_counts):
                    k = first[noise_type] + index
                    if rates[k] != int(x["sample_rate"]):                                            # steps.py:294
                        raise ValueError("Invalid noise signals are being used, all noise signals must have same sample rate "
                                         "as speech signals that are being augmented (clip '%s' has %d Hz, element %r %d Hz)"
                                         % (type2paths[noise_type][index], rates[k], x.get("id"), int(x["sample_rate"])))
                    src.append(i)
                    clip.append(k)
                    snrs.append(snr)
                    ids.append(additive_noise_id(x["id"], noise_type, snr))
            r = signal_ops.RaggedSignals.from_list([x["signal"] for x in batch])
            out = signal_ops.mix_noise(r, bank, src, clip, snrs).split()
            for i, new_id, signal in zip(src, ids, out):
                yield dict(batch[i], id=new_id, signal=signal)

    return mixed()


def augment_signals(ds, augment_configs, seed=None):
    """reference steps.py:215-229: one augmented dataset per config (`type` "additive_noise" -> augment_by_additive_noise
    with the config's other keys, `split` aside, as keyword arguments), then elements are drawn from [ds] + augmented like
    tf.data.experimental.sample_from_datasets: at each draw one of the sources that are not exhausted is chosen uniformly
    (np.random.default_rng(seed)), so every source keeps its own order and the output is exactly the union.
    `ds` is iterated once: every source reads its own itertools.tee branch, which buffers only what the others have not
    consumed yet (at most one launch batch)."""
    branches = list(itertools.tee(ds, 1 + len(augment_configs)))
    sources = [branches[0]]
    for conf, branch in zip(augment_configs, branches[1:]):
        aug_kwargs = {k: v for k, v in conf.items() if k not in {"type", "split"}}
        if conf["type"] == "random_resampling":
            # the reference calls augment_by_random_resampling here, a function it never defines (steps.py:223)
            raise ValueError("augmentation type 'random_resampling' is not defined by lidbox; use the step "
                             "'random_signal_speed_change' instead")
        elif conf["type"] == "additive_noise":
            augmented = augment_by_additive_noise(branch, **aug_kwargs)
            if augmented is not None:
                sources.append(augmented)
        else:
            logger.warning("Unknown signal augmentation type '%s', skipping", conf["type"])
    rng = np.random.default_rng(seed)

    def sampled():
        live = [iter(s) for s in sources]
        while live:
            i = int(rng.integers(0, len(live)))
            try:
                yield next(live[i])
            except StopIteration:
                del live[i]

    return sampled()


def repeat_count(min_length_ms, sample_rate, num_samples):
    """steps.py:961-966 in the reference's float32: int(ceil(divide_no_nan(float32(1e-3 * ms) * float32(rate), float32(n))))"""
    target = np.float32(1e-3 * min_length_ms) * np.float32(sample_rate)
    n = np.float32(num_samples)
    ratio = np.float32(0.0) if n == 0 else np.float32(target / n)
    return int(np.ceil(ratio))


def repeat_too_short_signals(ds, min_length_ms, launch_batch=256):
    """reference steps.py:950-969: every signal is repeated `repeat_count` times (signal_ops.tile), which makes it at least
    min_length_ms long; a signal that is long enough already (one repeat) and an empty one are passed on as they are."""
    logger.info("Repeating all signals until they are at least %d ms", min_length_ms)
    for batch in _launch_batches(ds, launch_batch):
        sigs = [torch.as_tensor(x["signal"]) for x in batch]
        reps = [repeat_count(min_length_ms, x["sample_rate"], s.numel()) for x, s in zip(batch, sigs)]
        if min(reps) < 0:
            raise ValueError("min_length_ms = %r gives a negative repeat count" % (min_length_ms,))
        idx = [i for i, (s, k) in enumerate(zip(sigs, reps)) if s.numel() and k != 1]
        if not idx:
            yield from batch
            continue
        r = signal_ops.RaggedSignals.from_list([sigs[i] for i in idx])
        yield from _augmented(batch, idx, signal_ops.tile(r, [reps[i] for i in idx]).split())


# ------------------------------------------------------------------ steps on `input`
def create_input_chunks(ds, length, step, launch_batch=256):
    """reference steps.py:558-576: `input` [T, C] becomes its max(0, 1 + (T - length) // step) windows of `length` frames
    (signal_ops.input_chunks); `id` gets "-%06d" with the 1-based window number, other keys are carried; elements
    with T < length vanish."""
    for batch in _launch_batches(ds, launch_batch):
        by_width = {}
        for i, x in enumerate(batch):
            by_width.setdefault(int(x["input"].shape[1]), []).append(i)
        chunks_of = [None] * len(batch)
        for idx in by_width.values():
            chunks, nch = signal_ops.input_chunks([batch[i]["input"] for i in idx], length, step)
            c0 = 0
            for i, n in zip(idx, nch):
                chunks_of[i] = chunks[c0:c0 + int(n)]
                c0 += int(n)
        for x, ch in zip(batch, chunks_of):
            for k in range(ch.shape[0]):
                yield dict(x, id="%s-%06d" % (x["id"], k + 1), input=ch[k])


def normalize(ds, config):
    """reference steps.py:821-834: batches of config.get("batch_size", 1) elements, features.cmvn(x[key], **kwargs) on the
    stacked batch, unbatched.  Elements of one batch must share the shape (tf.data's `batch` has the same requirement).
    `ragged: true` (lidbox_amd only): the [T, C] values of a batch may differ in T; one launch of features.cmvn_ragged gives every
    element what `batch_size: 1` gives it, bit for bit.  Axis 1 (time) only."""
    logger.info("Applying normalization with config:\n  %s", _dict_to_logstring(config))
    key = config["key"]
    kwargs = config.get("kwargs", {})
    ragged = bool(config.get("ragged", False))
    if ragged and set(kwargs) - {"axis"} or ragged and kwargs.get("axis", 1) != 1:
        raise ValueError("ragged normalization takes axis=1 (time) only, got kwargs %r" % (kwargs,))
    for batch in _launch_batches(ds, int(config.get("batch_size", 1))):
        values = [torch.as_tensor(x[key]) for x in batch]
        if ragged:
            if any(v.dim() != 2 or v.shape[1] != values[0].shape[1] for v in values):
                raise ValueError("ragged normalization needs [T, C] '%s' tensors with one C" % key)
            offsets = np.concatenate(([0], np.cumsum([int(v.shape[0]) for v in values])))
            normalized = features.cmvn_ragged(torch.cat(values), offsets)
            for x, lo, hi in zip(batch, offsets[:-1], offsets[1:]):
                yield dict(x, **{key: normalized[int(lo):int(hi)]})
            continue
        if any(v.shape != values[0].shape for v in values):
            raise ValueError("cannot batch '%s' tensors of different shapes for normalization" % key)
        normalized = features.cmvn(torch.stack(values), **kwargs)
        for x, v in zip(batch, normalized.unbind(0)):
            yield dict(x, **{key: v})


# ------------------------------------------------------------------ embeddings
def extract_embeddings(ds, config):
    """reference steps.py:674-705.  config = {"extractors": [...], "batch_size": 1, "no_unbatch": False}.
    An extractor is, as in the reference, a model config + checkpoint description handed to
    `KerasWrapper.from_config_as_embedding_extractor_fn` (keys cache_directory, model, experiment_name, input_shape,
    output_shape, best_checkpoint; steps.py:680-681) -- or, additionally, an already built callable: the result of
    `module.as_embedding_extractor(model)`, or a model that has `.embed`, mapping inputs [B, T, C] to embeddings
    [B, D].  The embeddings of several extractors are concatenated on axis 1 (steps.py:693).  Elements of one batch
    must share the input shape (tf.data's `batch` has the same requirement).
    `ragged: true` (lidbox_amd only): up to `batch_size` consecutive elements whose [T, C] inputs may differ in T go through ONE
    ragged pass per extractor (`embed_ragged` of models/ragged_pass.py's RaggedPass, the base of every model with such a pass:
    the x-vector family, lstm, ap_lstm, bi_gru, spherespeaker, crnn -- whose utterances need 32 frames at least -- clstm and
    multilevel_attention); order is kept and every element gets what `batch_size: 1` gives it up to rounding.  Every
    extractor must have a ragged form (`.ragged` of an as_embedding_extractor result, `.embed_ragged` of a model);
    `no_unbatch` has no meaning without one input shape and is refused."""
    ragged = bool(config.get("ragged", False))
    no_unbatch = bool(config.get("no_unbatch", False))
    if ragged and no_unbatch:
        raise ValueError("ragged embedding extraction yields elements: no_unbatch needs batches of one input shape")
    extractors = []
    for e in config["extractors"]:
        if isinstance(e, dict):
            from ..models.keras_utils import KerasWrapper
            e = KerasWrapper.from_config_as_embedding_extractor_fn(e)
        fn = e.embed if hasattr(e, "embed") else e
        if ragged:
            fn = getattr(e, "embed_ragged", None) or getattr(e, "ragged", None)
            if fn is None:
                raise ValueError("extractor %r has no ragged form (.embed_ragged of a model, .ragged of an embedding extractor)" % (e,))
        if not callable(fn):
            raise ValueError("extractors must be checkpoint configs or callables mapping inputs [B,T,C] to embeddings [B,D]")
        extractors.append(fn)
    logger.info("Using %d extractors", len(extractors))
    batch_size = int(config.get("batch_size", 1))
    logger.info("Batching inputs with batch size %s, extracting embeddings in batches.", batch_size)
    if ragged:
        for batch in _launch_batches(ds, batch_size):
            values = [torch.as_tensor(x["input"], dtype=torch.float32) for x in batch]
            if any(v.dim() != 2 or v.shape[1] != values[0].shape[1] for v in values):
                raise ValueError("ragged embedding extraction needs [T, C] 'input' tensors with one C")
            offsets = np.concatenate(([0], np.cumsum([int(v.shape[0]) for v in values])))
            inputs = torch.cat([v if v.is_cuda else v.cuda() for v in values])
            embeddings = torch.cat([fn(inputs, offsets) for fn in extractors], dim=1)
            for i, x in enumerate(batch):
                yield dict(x, embedding=embeddings[i])
        return
    for batch in _launch_batches(ds, batch_size):
        inputs = torch.stack([torch.as_tensor(x["input"], dtype=torch.float32) for x in batch])
        if not inputs.is_cuda:
            inputs = inputs.cuda()
        embeddings = torch.cat([fn(inputs) for fn in extractors], dim=1)                              # steps.py:693
        if no_unbatch:
            keys = batch[0].keys()
            out = {k: [x[k] for x in batch] for k in keys}
            out["input"], out["embedding"] = inputs, embeddings
            yield out
        else:
            for i, x in enumerate(batch):
                yield dict(x, embedding=embeddings[i])


# ------------------------------------------------------------------ host steps and the step list driver
Step = collections.namedtuple("Step", ("key", "kwargs"))


def _dict_to_logstring(d):
    return "\n  ".join("{}: {}".format(k, p) for k, p in d.items())


def _size(v):
    return int(v.numel()) if isinstance(v, torch.Tensor) else int(np.size(v))


def _all_true(v):
    return bool(v.all()) if isinstance(v, (torch.Tensor, np.ndarray)) else bool(v)


def initialize(labels, init_data):
    """reference steps.py:776-800: one element per utterance from the metadata columns of `init_data`, plus `target` = the
    index of its `label` in `labels` (len(labels) for a label that is not listed, as the reference's lookup table)."""
    init_data = {k: list(v) for k, v in init_data.items()}
    logger.info("Initializing dataset from metadata:\n  %s",
                "\n  ".join("{}: {}".format(k, len(init_data[k])) for k in sorted(init_data)))
    sizes = {len(v) for v in init_data.values()}
    if len(sizes) != 1:
        logger.error("Cannot initialize dataset from metadata dictionary that has values of different lengths")
        return None
    label2int = {label: i for i, label in enumerate(labels)}
    count = sizes.pop()

    def elements():
        for i in range(count):
            x = {k: v[i] for k, v in init_data.items()}
            yield dict(x, target=label2int.get(x["label"], len(label2int)))

    return elements()


def load_audio(ds, num_prefetch=None):
    """reference steps.py:803-818: `signal` (float32 on the HIP device) and `sample_rate` from the WAV file at `path`.
    `num_prefetch` is accepted for the config's sake; elements are produced on demand."""
    logger.info("Reading audio files from the path of each element and appending the read signals and their sample rates "
                "to each element.")
    for x in ds:
        signal, sample_rate = audio_features.read_wav(x["path"])
        yield dict(x, signal=signal, sample_rate=sample_rate)


def drop_empty(ds):
    """reference steps.py:635-650: drop elements whose `signal` or `input` has no entries"""
    non_scalar_keys = ("signal", "input")
    logger.info("Dropping every element which have an empty tensor at any of the non-scalar element keys:\n  %s",
                "\n  ".join(non_scalar_keys))
    return (x for x in ds if not any(k in x and _size(x[k]) == 0 for k in non_scalar_keys))


def apply_filters(ds, config):
    """reference steps.py:137-180: keep the elements that pass every filter of `config`: `equal` {key, value},
    `min_signal_length_ms` (threshold int(float32(sample_rate) * float32(1e-3 * ms)) samples, steps.py:154-157) and
    `min_shape` {key, shape}.  A filter passes elements that do not have its key."""
    logger.info("Applying filters on every element in the dataset, keeping only elements which match the given config:\n  %s",
                _dict_to_logstring(config))
    filters = []
    if "equal" in config:
        key, value = config["equal"]["key"], config["equal"]["value"]
        filters.append((lambda x, k=key, v=value: k not in x or _all_true(x[k] == v), key))
    if "min_signal_length_ms" in config:
        min_sec = np.float32(1e-3 * config["min_signal_length_ms"])
        filters.append((lambda x, v=min_sec: "signal" not in x or _size(x["signal"]) >= int(np.float32(x["sample_rate"]) * v),
                        "min_signal_length_sec"))
    if "min_shape" in config:
        key, shape = config["min_shape"]["key"], tuple(config["min_shape"]["shape"])
        filters.append((lambda x, k=key, v=shape: k not in x or (len(x[k].shape) == len(v) and
                                                                 all(a >= b for a, b in zip(x[k].shape, v))), key))
    if not filters:
        logger.warning("No filters defined, skipping filtering")
        return ds
    logger.info("Using %d different filters:\n  %s", len(filters), "\n  ".join(name for _, name in filters))
    return (x for x in ds if all(fn(x) for fn, _ in filters))


def remap_keys(ds, new_keys):
    """reference steps.py:938-947: rename keys; a key mapped to None is dropped"""
    logger.info("Remapping keys of every element using config:\n  %s", _dict_to_logstring(new_keys))
    return ({new_keys.get(k, k): v for k, v in x.items() if new_keys.get(k, k) is not None} for x in ds)


def filter_keys_in_set(ds, keys):
    """reference steps.py:739-748"""
    logger.info("For each element in the dataset, keeping only values with keys: %s.", ", ".join(keys))
    return ({k: v for k, v in x.items() if k in keys} for x in ds)


def as_supervised(ds):
    """reference steps.py:203-212: (input, target) pairs"""
    logger.info("Converting all elements to tuple pairs (inputs, targets) and dropping all other values.")
    return ((x["input"], x["target"]) for x in ds)


def shuffle(ds, buffer_size, seed=None):
    """reference steps.py:997-999 (tf.data's buffered shuffle): a buffer of `buffer_size` elements is kept full; every output
    is drawn uniformly from it (np.random.default_rng(seed))"""
    logger.info("Shuffling dataset with buffer size %d", buffer_size)
    buffer_size = int(buffer_size)
    if buffer_size < 1:
        raise ValueError("buffer_size must be at least 1")
    rng = np.random.default_rng(seed)

    def shuffled():
        buf = []
        for x in ds:
            if len(buf) < buffer_size:
                buf.append(x)
                continue
            i = int(rng.integers(0, buffer_size))
            yield buf[i]
            buf[i] = x
        while buf:
            i = int(rng.integers(0, len(buf)))
            buf[i], buf[-1] = buf[-1], buf[i]
            yield buf.pop()

    return shuffled()


def lambda_fn(ds, fn):
    """reference steps.py:837-842"""
    logger.info("Applying function '%s' on dataset.", str(fn))
    return fn(ds)


def _pass_through(key):
    def step(ds, **kwargs):
        logger.warning("Step '%s' is not built in lidbox_amd; it does not alter elements, the dataset is passed on as it is.", key)
        return ds
    return step


VALID_STEP_FUNCTIONS = {
    "apply_filters": apply_filters,
    "apply_vad": apply_vad,
    "as_supervised": as_supervised,
    "augment_by_additive_noise": augment_by_additive_noise,
    "augment_signals": augment_signals,
    "cache": _pass_through("cache"),
    "compute_rms_vad": compute_rms_vad,
    "consume": _pass_through("consume"),
    "consume_to_tensorboard": _pass_through("consume_to_tensorboard"),
    "create_input_chunks": create_input_chunks,
    "create_signal_chunks": create_signal_chunks,
    "drop_empty": drop_empty,
    "extract_embeddings": extract_embeddings,
    "extract_features": extract_features,
    "filter_keys_in_set": filter_keys_in_set,
    "initialize": initialize,
    "lambda": lambda_fn,
    "load_audio": load_audio,
    "normalize": normalize,
    "random_signal_fir_filtering": random_signal_fir_filtering,
    "random_signal_speed_change": random_signal_speed_change,
    "remap_keys": remap_keys,
    "repeat_too_short_signals": repeat_too_short_signals,
    "shuffle": shuffle,
}


def from_steps(steps):
    """reference steps.py:34-58: initialize(**steps[0].kwargs), then every further step applied in order.  A step that
    is None is skipped.  Unlike the reference, which logs an unknown key and goes on, a key without a function here raises
    ValueError: dropping e.g. a VAD step silently would change the data."""
    logger.info("Initializing and preparing dataset from %d steps:\n  %s", len(steps),
                "\n  ".join(s.key for s in steps if s is not None))
    if steps[0] is None or steps[0].key != "initialize":
        logger.critical("When constructing a dataset, the first step must be 'initialize' but it was '%s'. The 'initialize' step "
                        "is needed for first loading all metadata such as the utterance_id to wavpath mappings.",
                        None if steps[0] is None else steps[0].key)
        return None
    for step in steps[1:]:
        if step is not None and step.key not in VALID_STEP_FUNCTIONS:
            raise ValueError("step '%s' is not implemented in lidbox_amd.data.steps" % step.key)
    ds = initialize(**steps[0].kwargs)
    if ds is None:
        logger.critical("Failed to apply step 'initialize', it did not return a dataset.")
        return None
    for step_num, step in enumerate(steps[1:], start=2):
        if step is None:
            logger.warning("Skipping no-op step with value None")
            continue
        logger.info("Applying step number %d: '%s'.", step_num, step.key)
        ds = VALID_STEP_FUNCTIONS[step.key](ds, **step.kwargs)
        if ds is None:
            logger.critical("Failed to apply step '%s', it did not return a dataset.", step.key)
            return None
    logger.info("All %d steps completed, returning prepared dataset.", len(steps))
    return ds
