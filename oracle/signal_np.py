"""
oracle.signal_np -- numpy restatement of the lidbox signal steps that sit immediately before the feature
kernel: RMS, peak normalisation, run-length encoding, energy VAD, silence removal, VAD
application, fixed-length chunking and the SNR mixer.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Pinned by the reference's own tests for these functions
(tests/test_features_audio.py:49-67, 157-191: dBFS_to_linear, peak_normalize bound, root_mean_square 1e-5,
run_length_encoding known answer, VAD all-speech on the WAV fixtures / all-silence on zeros, remove_silence
shape laws) -- restated in tests/test_oracle_signal.py -- and by `numpy_snr_mixer` (audio.py:100-121), the
reference's own numpy twin of snr_mixer.  VALUES of the TF versions: parity unpinned (no TensorFlow here).

All file:line citations are relative to /root/reference/lidbox/.
"""
import numpy as np

from .features_np import ms_to_frames


def dBFS_to_linear(level):
    """features/audio.py:49-51"""
    return np.float32(10.0) ** (np.float32(level) / np.float32(20.0))


def peak_normalize(signal, dBFS=0.0):
    """features/audio.py:57-59"""
    signal = np.asarray(signal)
    return dBFS_to_linear(dBFS) * (signal / np.max(np.abs(signal)))


def root_mean_square(x, axis=-1):
    """features/audio.py:266-270"""
    x = np.asarray(x)
    return np.sqrt(np.mean(np.square(np.abs(x)), axis=axis))


def run_length_encoding(v):
    """features/audio.py:275-283 -> (start positions, lengths) of the runs of equal values"""
    v = np.asarray(v)
    if v.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    i = np.concatenate(([-1], np.nonzero(v[1:] != v[:-1])[0], [v.size - 1]))
    pos = np.concatenate(([0], np.cumsum(i[1:] - i[:-1])))
    return pos[:-1], pos[1:] - pos[:-1]


def invert_too_short_consecutive_false(mask, min_length):
    """features/audio.py:289-297: runs of False shorter than min_length become True"""
    mask = np.asarray(mask, bool)
    if min_length == 0 or mask.size == 0:
        return mask
    pos, lengths = run_length_encoding(mask.astype(np.int32))
    true_or_too_short = np.logical_or(mask[pos], lengths < min_length)
    return np.repeat(true_or_too_short, lengths)


def frame_nonoverlapping(signal, frame_length):
    """tf.signal.frame(signal, L, L) with pad_end=False: [N // L, L]; the tail is dropped"""
    signal = np.asarray(signal)
    n = signal.shape[0] // frame_length if frame_length > 0 else 0
    return signal[:n * frame_length].reshape(n, frame_length)


def framewise_rms_energy_vad_decisions(signal, sample_rate, frame_step_ms, min_non_speech_ms=0, strength=0.05,
                                       min_rms_threshold=1e-3, dtype=np.float64):
    """features/audio.py:308-329 (time_axis=0).  dtype=np.float32 follows the reference's arithmetic type."""
    signal = np.asarray(signal, dtype)
    frame_step = ms_to_frames(sample_rate, frame_step_ms)
    frames = frame_nonoverlapping(signal, frame_step)                                  # :314
    rms = root_mean_square(frames, axis=1).astype(dtype)                               # :317
    if rms.size == 0:
        return np.zeros(0, bool)
    mean_rms = np.mean(rms, dtype=dtype)                                               # :318
    threshold = dtype(strength) * np.maximum(dtype(min_rms_threshold), mean_rms)       # :321
    vad = rms > threshold                                                              # :322
    min_non_speech_frames = int(ms_to_frames(sample_rate, min_non_speech_ms) / frame_step)   # :325 (int64 cast truncates)
    return invert_too_short_consecutive_false(vad, min_non_speech_frames)              # :326


def remove_silence(signal, rate, window_ms=10, min_non_speech_ms=300, dtype=np.float64):
    """features/audio.py:337-353"""
    window_frames = (window_ms * rate) // 1000
    vad_1 = framewise_rms_energy_vad_decisions(signal, rate, window_ms, min_non_speech_ms, strength=0.1, dtype=dtype)
    windows = frame_nonoverlapping(np.asarray(signal), window_frames)
    return windows[vad_1].reshape(-1)


def apply_vad(signal, sample_rate, vad_frame_length_ms, vad_is_speech):
    """data/steps.py:191-198: keep the VAD frames marked as speech, flattened"""
    sec = np.float32(1e-3) * np.float32(vad_frame_length_ms)
    vad_frame_length = int(np.float32(sample_rate) * sec)
    frames = frame_nonoverlapping(np.asarray(signal), vad_frame_length)
    return frames[np.asarray(vad_is_speech, bool)].reshape(-1)


def signal_chunk_plan(num_samples, sample_rate, length_ms, step_ms, max_pad_ms=0):
    """data/steps.py:586-588, 604-614: (chunk_length, chunk_step, padded signal length, number of chunks)"""
    sr = np.float32(sample_rate)
    chunk_length = int(sr * np.float32(1e-3 * length_ms))
    chunk_step = int(sr * np.float32(1e-3 * step_ms))
    max_pad = int(sr * np.float32(1e-3 * max_pad_ms))
    n = int(num_samples)
    num_full_chunks = max(0, 1 + (n - chunk_length) // chunk_step)                     # :607
    last_chunk_length = n - num_full_chunks * chunk_step                               # :610
    if last_chunk_length < chunk_length and chunk_length <= last_chunk_length + max_pad:   # :611
        n = n + chunk_length - last_chunk_length                                       # :612
    num_chunks = max(0, 1 + (n - chunk_length) // chunk_step) if n >= chunk_length else 0   # tf.signal.frame, :614
    return chunk_length, chunk_step, n, num_chunks


def create_signal_chunks(signal, sample_rate, length_ms, step_ms, max_pad_ms=0):
    """data/steps.py:600-614 -> [num_chunks, chunk_length]"""
    signal = np.asarray(signal)
    L, S, n, nc = signal_chunk_plan(signal.shape[0], sample_rate, length_ms, step_ms, max_pad_ms)
    padded = np.concatenate([signal, np.zeros(n - signal.shape[0], signal.dtype)])
    idx = np.arange(nc)[:, None] * S + np.arange(L)[None, :]
    return padded[idx] if nc > 0 else np.zeros((0, L), signal.dtype)


def snr_mixer(clean, noise, snr, dtype=np.float64):
    """features/audio.py:128-148 (TF version; numpy twin at :100-121)"""
    clean, noise = np.asarray(clean, dtype), np.asarray(noise, dtype)
    assert clean.size == noise.size                                                    # :132
    lvl25 = dtype(10.0) ** dtype(-25.0 / 20.0)
    clean_norm = (lvl25 / root_mean_square(clean)) * clean                             # :134-135
    rmsclean = root_mean_square(clean_norm)
    noise_norm = (lvl25 / root_mean_square(noise)) * noise                             # :138-139
    rmsnoise = root_mean_square(noise_norm)
    level = dtype(10.0) ** (dtype(snr) / dtype(20.0))                                  # :143
    noisescalar = np.sqrt(rmsclean / level / rmsnoise)                                 # :144
    noisenewlevel = noisescalar * noise_norm
    return clean_norm, noisenewlevel, clean_norm + noisenewlevel


def numpy_snr_mixer_reference_twin(clean, noise, snr):
    """features/audio.py:100-121 restated verbatim in meaning (the reference's own numpy version)"""
    rmsclean = (clean ** 2).mean() ** 0.5
    clean = clean * (10 ** (-25 / 20) / rmsclean)
    rmsclean = (clean ** 2).mean() ** 0.5
    rmsnoise = (noise ** 2).mean() ** 0.5
    noise = noise * (10 ** (-25 / 20) / rmsnoise)
    rmsnoise = (noise ** 2).mean() ** 0.5
    noisescalar = np.sqrt(rmsclean / (10 ** (snr / 20)) / rmsnoise)
    noisenewlevel = noise * noisescalar
    return clean, noisenewlevel, clean + noisenewlevel


# --------------------------------------------------------------------------- planted VAD inputs
# Inputs whose VAD answer is known by construction (tests/test_oracle_signal.py proves it on the CPU,
# tests/test_signal_paths_gpu.py holds the kernels to it bit for bit).

VAD_PLAN_MIN_LENS = (1, 2, 3, 30, 100)
VAD_PLAN_FRAME_LENS = (160, 400, 7, 6, 1)
VAD_PLAN_SIZES = (0, 1, 255, 256, 257, 1000, 60000)          # frames; the last is ten minutes of 10 ms frames


def vad_run_lengths(min_len):
    """the non-speech run lengths on either side of the inversion rule: min_len - 1, min_len, min_len + 1, 2 min_len + 5"""
    return [n for n in (min_len - 1, min_len, min_len + 1, 2 * min_len + 5) if n > 0]


def invert_too_short_brute_force(mask, min_length):
    """the definition of invert_too_short_consecutive_false, frame by frame: a frame is inverted iff it is False and its
    maximal run of False is shorter than min_length"""
    mask = [bool(v) for v in mask]
    out = list(mask)
    for i, v in enumerate(mask):
        if v:
            continue
        a = i
        while a > 0 and not mask[a - 1]:
            a -= 1
        b = i
        while b + 1 < len(mask) and not mask[b + 1]:
            b += 1
        if b - a + 1 < min_length:
            out[i] = True
    return np.array(out, bool)


def vad_frame_plans(min_len, seed=0):
    """per-utterance boolean plans (True = loud frame) for one min_len, in batch order:
      * runs of vad_run_lengths(min_len) quiet frames at the start, in the middle and at the end of an utterance;
      * two neighbours that end / start with min_len - 1 quiet frames (both runs inverted, never merged);
      * quiet runs that straddle a multiple of 256 of the batch's global frame index;
      * utterances of VAD_PLAN_SIZES frames with random runs of 1 .. 2 min_len + 5 frames."""
    rng = np.random.default_rng(1000 + 7 * min_len + seed)
    T, F = np.ones, np.zeros
    plans = []
    for n in vad_run_lengths(min_len):
        plans.append(np.concatenate([F(n, bool), T(min_len + 3, bool)]))                           # start
        plans.append(np.concatenate([T(5, bool), F(n, bool), T(2 * min_len + 1, bool)]))           # middle
        plans.append(np.concatenate([T(min_len + 2, bool), F(n, bool)]))                           # end
    if min_len >= 2:
        plans.append(np.concatenate([T(4, bool), F(min_len - 1, bool)]))
        plans.append(np.concatenate([F(min_len - 1, bool), T(4, bool)]))
    for n in sorted({max(2, min_len - 1), max(2, min_len), 2 * min_len + 5}):
        done = sum(len(p) for p in plans)
        lead = (-(done + 3)) % 256 + 3 - n // 2                 # the run covers global frames k * 256 - n // 2 .. + n
        if lead < 1:
            lead += 256
        plans.append(np.concatenate([T(lead, bool), F(n, bool), T(3, bool)]))
        first = done + lead
        assert first // 256 != (first + n - 1) // 256
    for size in VAD_PLAN_SIZES:
        p = np.zeros(size, bool)
        i, loud = 0, bool(rng.integers(0, 2))
        while i < size:
            n = int(rng.integers(1, 2 * min_len + 6)) if rng.random() < 0.7 else int(rng.choice(vad_run_lengths(min_len)))
            p[i:i + n] = loud
            i, loud = i + n, not loud
        plans.append(p)
    plans.append(np.zeros(2 * min_len + 7, bool))               # all quiet: stays non-speech
    return plans


def planted_vad_signal(plan, frame_len, tail, rng):
    """float32 signal of len(plan) frames + `tail` (< frame_len) more samples: noise of amplitude 0.2 (every |sample| in
    [0.1, 0.2], so even a one-sample frame is loud), quiet frames are the same noise scaled by 1e-4"""
    n = len(plan) * frame_len
    u = rng.random(n + tail, dtype=np.float32) - np.float32(0.5)
    x = np.copysign(np.float32(0.1) + np.float32(0.2) * np.abs(u), u).astype(np.float32)
    if n:
        scale = np.where(plan, np.float32(1.0), np.float32(1e-4)).astype(np.float32)
        x[:n] = (x[:n].reshape(len(plan), frame_len) * scale[:, None]).reshape(-1)
    return x


def planted_vad_batch(min_len, frame_len, seed=0):
    """-> (plans, signals) of one test case"""
    plans = vad_frame_plans(min_len, seed)
    rng = np.random.default_rng(77 * frame_len + min_len + seed)
    sigs = [planted_vad_signal(p, frame_len, (3 * b) % frame_len, rng) for b, p in enumerate(plans)]
    return plans, sigs
