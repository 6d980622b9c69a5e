"""
Every kernel and template instantiation of csrc/signal.hip on each side of each dispatch condition, against the float64
oracle (oracle/signal_np.py) or exact numpy where the operation is a copy.

The kernels pick a path by length, alignment and grid limits; `PATHS` below is the one table of the sizes that select a
path, each with the condition in signal.hip it sits on.  The planted VAD inputs come from oracle/signal_np.py and are
proven decidable with margin on the CPU (tests/test_oracle_signal.py), so decisions here are compared bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import signal_np as so

pytestmark = pytest.mark.gpu

PATHS = dict(
    # lidbox_peak_normalize_max: `max_length <= 1024L * 4 * 4` -> peak_normalize_reg_kernel<4>;
    # lidbox_snr_mixer:          `N <= 1024L * 4 * 4`          -> snr_mixer_reg_kernel<4>
    reg4=1024 * 4 * 4,
    # lidbox_peak_normalize_max: `max_length <= 1024L * 4 * 8` -> <8>, above it <16>;
    # lidbox_snr_mixer:          `vec && N <= 1024L * 4 * 8`   -> snr_mixer_reg_kernel<8>, above it snr_mixer_kernel
    reg8=1024 * 4 * 8,
    # lidbox_peak_normalize_max: `max_length <= 1024L * 4 * 16` -> peak_normalize_reg_kernel<16>, above it (or with
    # `aligned16 == 0`, or an unaligned `signals` / `out` base) lidbox_peak_normalize -> peak_normalize_kernel
    reg16=1024 * 4 * 16,
    # signal_rms_kernel, vad_threshold_kernel, vad_scan_kernel, peak_normalize_kernel: `i += 256` -- one trip up to 256 items
    block=256,
    # lidbox_signal_chunks: `c0 += 65535` (grid.y); util.segment_mean: `range(0, nseg, 65535)` + pointer offsets
    grid_y=65535,
    # segment_mean_kernel: `d = blockIdx.x * 256 + threadIdx.x` -- blockIdx.x > 0 from D = 257
    seg_block=256,
    # lidbox_pcm16_to_f32: `if (g > 8192) g = 8192` with g = cdiv(channels == 1 ? cdiv(frames, 8) : frames, 256):
    # the grid-stride loops take a second trip above 8192 * 256 * 8 mono frames / 8192 * 256 multi-channel frames
    pcm_mono=8192 * 256 * 8,
    pcm_multi=8192 * 256,
)
assert (PATHS["reg4"], PATHS["reg8"], PATHS["reg16"]) == (16384, 32768, 65536)
assert (PATHS["pcm_mono"], PATHS["pcm_multi"]) == (16777216, 2097152)

LEVELS = (0, -3, -9)
PEAK_LENGTHS = [1, 2, 3, 5] + [b + d for b in (PATHS["reg4"], PATHS["reg8"], PATHS["reg16"]) for d in (-3, -1, 0, 1, 4)] + [200001]


def _dev(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).cuda()


def _sg():
    from lidbox_amd.features import signal_ops as sg
    return sg


# ------------------------------------------------------------------ ragged layouts
def _aligned(sigs):
    return _sg().RaggedSignals.from_list(sigs)


def _unaligned_starts(sigs):
    """a RaggedSignals built by hand: gaps of 1 .. 3 floats, so starts are not multiples of 4 (aligned16 == 0)"""
    starts, pos = [], 1
    for b, s in enumerate(sigs):
        if pos % 4 == 0:
            pos += 1
        starts.append(pos)
        pos += len(s) + 1 + b % 3
    flat = np.full(pos + 4, 7.0, np.float32)
    for st, s in zip(starts, sigs):
        flat[st:st + len(s)] = s
    assert any(st % 4 for st in starts)
    return _sg().RaggedSignals(_dev(flat), starts, [len(s) for s in sigs])


def _offset_base(sigs):
    """16-byte aligned starts inside a flat buffer whose base is one float off a 16-byte boundary"""
    sg = _sg()
    starts, total = sg._aligned_starts([len(s) for s in sigs])
    flat = np.zeros(max(total, 4) + 1, np.float32)
    for st, s in zip(starts, sigs):
        flat[1 + st:1 + st + len(s)] = s
    buf = _dev(flat)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4
    return sg.RaggedSignals(view, starts, [len(s) for s in sigs])


LAYOUTS = dict(aligned=_aligned, unaligned_starts=_unaligned_starts, offset_base=_offset_base)


def _peak_kernel(max_len, layout):
    """the dispatch of lidbox_peak_normalize_max restated (a reviewer checks it against signal.hip)"""
    if layout != "aligned" or max_len > PATHS["reg16"]:
        return "peak_normalize_kernel"
    return "peak_normalize_reg_kernel<%d>" % (4 if max_len <= PATHS["reg4"] else 8 if max_len <= PATHS["reg8"] else 16)


# ------------------------------------------------------------------ VAD, apply_vad: exact
def _check_planted_vad(r, plans, sigs, frame_len, min_len, strength):
    sg = _sg()
    vad = sg.vad_decisions(r, frame_len, min_len, strength)
    fo = vad["frame_offsets_host"]
    assert (fo == np.concatenate(([0], np.cumsum([len(p) for p in plans])))).all()
    dec = vad["decisions"].cpu().numpy()
    slots = vad["slots"].cpu().numpy()
    counts = vad["counts"].cpu().numpy()
    voiced = sg.apply_vad(r, vad)
    out = [v.cpu().numpy() for v in voiced.split()]
    assert dec.shape == (int(fo[-1]),) and set(np.unique(dec)) <= {0, 1}
    for b, (p, s) in enumerate(zip(plans, sigs)):
        want = so.invert_too_short_consecutive_false(p, min_len)
        got = dec[fo[b]:fo[b + 1]].astype(bool)
        assert got.shape == want.shape, b
        assert (got == want).all(), (b, len(p), np.nonzero(got != want)[0][:8])
        assert (slots[fo[b]:fo[b + 1]] == np.cumsum(want) - want).all(), b          # exclusive prefix sum
        assert counts[b] == want.sum(), b
        ref_out = so.frame_nonoverlapping(s, frame_len)[want].reshape(-1)
        assert out[b].dtype == np.float32 and out[b].shape == ref_out.shape and np.array_equal(out[b], ref_out), b


@pytest.mark.parametrize("frame_len", so.VAD_PLAN_FRAME_LENS)
@pytest.mark.parametrize("min_len", so.VAD_PLAN_MIN_LENS)
def test_planted_vad_decisions_slots_and_gather_are_exact(min_len, frame_len):
    """the plan is the pre-inversion mask, the expected decisions are invert(plan, min_len): runs of min_len - 1, min_len,
    min_len + 1 and 2 min_len + 5 quiet frames at the start / middle / end of an utterance, a pair of runs that meet at an
    utterance boundary, runs across a multiple of 256 of the global frame index, utterances of 0 .. 60 000 frames.  Bit-equal
    decisions for every utterance, slots = exclusive cumulative sum, counts = sum, gathered samples = frames[decisions]."""
    plans, sigs = so.planted_vad_batch(min_len, frame_len)
    r = _aligned(sigs)
    for strength in (0.05, 0.5):
        _check_planted_vad(r, plans, sigs, frame_len, min_len, strength)


@pytest.mark.parametrize("min_len,frame_len", [(3, 160), (30, 400), (2, 6)])
@pytest.mark.parametrize("layout", ["unaligned_starts", "offset_base"])
def test_planted_vad_on_unaligned_layouts(layout, min_len, frame_len):
    """frame_rms_kernel / apply_vad_kernel: `(L & 3) == 0 && aligned` fails on the pointer, not on L -- the scalar loops
    with a frame length that is a multiple of 4"""
    plans, sigs = so.planted_vad_batch(min_len, frame_len)
    keep = [b for b, p in enumerate(plans) if len(p) <= 1000]
    plans, sigs = [plans[b] for b in keep], [sigs[b] for b in keep]
    _check_planted_vad(LAYOUTS[layout](sigs), plans, sigs, frame_len, min_len, 0.05)


# ------------------------------------------------------------------ peak_normalize
def _level32(dbfs):
    """10^(dBFS / 20) with the exponent in float32, correctly rounded to float32 (what powf(10.0f, dBFS / 20.0f) returns)"""
    return np.float32(10.0 ** float(np.float32(dbfs) / np.float32(20.0)))


def _peak_utterance(n, seed):
    """-> (x, index of the unique peak); exact zeros planted; the last three samples are non-zero (the scalar tail of the
    register kernels), and for odd seeds the peak itself is the last sample"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.3).astype(np.float32)
    x[np.abs(x) < 1e-3] = np.float32(0.01)
    if n >= 8:
        x[rng.integers(0, n - 3, size=max(1, n // 64))] = 0.0
    x[-3:] = np.float32(0.2) * np.where(rng.random(min(3, n)) < 0.5, -1, 1).astype(np.float32)
    p = n - 1 if seed % 2 else int(rng.integers(0, n))
    x[p] = np.float32(-2.5 if seed % 3 == 0 else 2.5)
    return x, p


def _check_peak(got, x, p, dbfs):
    ref = so.peak_normalize(x.astype(np.float64), dbfs)
    assert got.shape == x.shape and not np.isnan(got).any()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    assert got[p] == np.sign(x[p]) * _level32(dbfs)                  # fl(level * fl(x / m)) with x = +-m
    assert (got[x == 0] == 0).all()


def _peak_run(layout, sigs, dbfs):
    sg = _sg()
    return [o.cpu().numpy() for o in sg.peak_normalize(LAYOUTS[layout](sigs), dbfs).split()]


@pytest.mark.parametrize("n", PEAK_LENGTHS)
def test_peak_normalize_each_length_alone_and_identical_on_every_kernel(n):
    """each utterance alone (the register kernel its own length selects, or peak_normalize_kernel above 65 536), then the
    same utterance where the batch maximum, unaligned starts or an unaligned base select another kernel: every path computes
    fl(level * fl(x / m)) with the same exact maximum m, so the outputs are bit-identical"""
    from lidbox_amd.features import audio
    x, p = _peak_utterance(n, n)
    fillers = [f for f in (20000, 50000, 70001) if f > n]
    for dbfs in LEVELS:
        alone = _peak_run("aligned", [x], dbfs)[0]
        _check_peak(alone, x, p, dbfs)
        seen = {_peak_kernel(n, "aligned")}
        assert np.array_equal(audio.peak_normalize(_dev(x), dBFS=dbfs).cpu().numpy(), alone)
        for f in fillers:                                            # NV follows the batch maximum
            y, _ = _peak_utterance(f, f)
            got = _peak_run("aligned", [y, x], dbfs)[1]
            seen.add(_peak_kernel(f, "aligned"))
            assert np.array_equal(got, alone), (f, dbfs)
        for layout in ("unaligned_starts", "offset_base"):
            got = _peak_run(layout, [x[:3], x], dbfs)[1]
            seen.add(_peak_kernel(n, layout))
            assert np.array_equal(got, alone), (layout, dbfs)
        want = {"peak_normalize_kernel"} | {"peak_normalize_reg_kernel<%d>" % v for v, cap in ((4, "reg4"), (8, "reg8"), (16, "reg16")) if n <= PATHS[cap]}
        assert seen == want


PEAK_BATCHES = [                                                     # lengths; the maximum picks the kernel
    [1, 2, 3, 5, 0, 16381, 16384],                                   # <4>
    [5, 16385, 0, 32767, 3, 16383],                                  # <8>: 16383 alone would take <4>
    [16383, 32769, 65536, 0, 2, 65533],                              # <16>
    [65537, 5, 16384, 0, 200001, 32772],                             # peak_normalize_kernel: longer than 65 536
]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", range(len(PEAK_BATCHES)))
def test_peak_normalize_ragged_batches_with_empty_and_all_zero_utterances(case, layout):
    """short and long utterances in one launch, an empty one and an all-zero one among them: every utterance equals the
    oracle and its own result alone; the all-zero utterance is NaN (the reference's 0 / 0) and leaves its neighbours alone"""
    lens = PEAK_BATCHES[case]
    made = [_peak_utterance(n, 10 * case + i) if n else (np.zeros(0, np.float32), None) for i, n in enumerate(lens)]
    sigs = [m[0] for m in made]
    sigs.insert(3, np.zeros(257, np.float32))
    made.insert(3, (sigs[3], None))
    for dbfs in LEVELS:
        got = _peak_run(layout, sigs, dbfs)
        for b, (x, p) in enumerate(made):
            assert got[b].shape == x.shape
            if b == 3:
                assert np.isnan(got[b]).all()
            elif len(x):
                _check_peak(got[b], x, p, dbfs)
                assert np.array_equal(got[b], _peak_run("aligned", [x], dbfs)[0]), b


@pytest.mark.parametrize("n", [100, 20000, 40000, 70000])          # <4>, <8>, <16>, peak_normalize_kernel
def test_peak_normalize_of_silence_is_nan_on_every_kernel(n):
    for layout in LAYOUTS:
        got = _peak_run(layout, [np.zeros(n, np.float32)], -3)[0]
        assert got.shape == (n,) and np.isnan(got).all()


# ------------------------------------------------------------------ signal_rms / root_mean_square
RMS_LENGTHS = [1, 255, 256, 257, 4001, 65537, 1 << 21]             # signal_rms_kernel `i += 256`: 1 trip, 1, 1, 2, 16, 257, 8192


def _rms_data(kind, shape, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    return (x if kind == "gauss" else 0.3 + 0.05 * x).astype(np.float32)


@pytest.mark.parametrize("kind", ["gauss", "dc"])
def test_signal_rms_over_the_stride_loop(kind):
    """relative 1e-5 against float64 (the bound tests/test_signal_gpu.py states for RMS values) from 1 sample to 2^21, ragged
    in one launch, then as dense rows: a row length that is a multiple of 4 is read in place, any other goes through from_list"""
    from lidbox_amd.features import audio
    sg = _sg()
    sigs = [_rms_data(kind, n, n) for n in RMS_LENGTHS]
    for layout in LAYOUTS:
        got = sg.signal_rms(LAYOUTS[layout](sigs)).cpu().numpy()
        for n, s, g in zip(RMS_LENGTHS, sigs, got):
            ref = so.root_mean_square(s.astype(np.float64))
            assert abs(g - ref) <= 1e-5 * ref, (layout, n, g, ref)
    for n in RMS_LENGTHS:
        x = _rms_data(kind, (3, n), n + 1)
        got = audio.root_mean_square(_dev(x), axis=-1).cpu().numpy()
        ref = so.root_mean_square(x.astype(np.float64), axis=-1)
        assert got.shape == (3,) and (np.abs(got - ref) <= 1e-5 * ref).all(), (n, got, ref)


# ------------------------------------------------------------------ snr_mixer
SNR_N = [PATHS["reg4"] - 4, PATHS["reg4"], PATHS["reg4"] + 4, PATHS["reg8"] - 4, PATHS["reg8"], PATHS["reg8"] + 4, 1 << 21, 1, 3]
SNR_DB = np.array([-5.0, 0.0, 3.0, 12.5, 30.0])


def _snr_inputs(N, B, seed):
    rng = np.random.default_rng(seed)
    clean = rng.standard_normal((B, N)) * rng.uniform(0.01, 1.0, size=(B, 1))
    noise = rng.standard_normal((B, N)) * rng.uniform(0.001, 0.3, size=(B, 1))
    if N == 1:
        # one sample: |clean_norm| = |noise_norm|, so at 0 dB opposite signs would cancel to a mixture of exactly zero in
        # the oracle, where a relative bound has no meaning; equal signs keep max|ref| at the signal's scale
        clean, noise = np.abs(clean), np.abs(noise)
    return clean.astype(np.float32), noise.astype(np.float32)


def _check_snr(got, clean, noise, snr):
    for b in range(clean.shape[0]):
        ref = so.snr_mixer(clean[b].astype(np.float64), noise[b].astype(np.float64), snr[b])
        for g, rf in zip(got, ref):
            assert g[b].shape == rf.shape and np.abs(g[b] - rf).max() <= 2e-5 * np.abs(rf).max(), b


@pytest.mark.parametrize("N", SNR_N)
def test_snr_mixer_at_the_register_kernel_switches(N):
    """N on either side of 16 384 (<4> / <8>) and 32 768 (<8> / three-pass vector), 2^21, and N % 4 != 0 (three-pass scalar)"""
    from lidbox_amd.features import audio
    sg = _sg()
    B = 5 if N < (1 << 20) else 2
    clean, noise = _snr_inputs(N, B, N)
    snr = SNR_DB[:B]
    cd, zd = _dev(clean), _dev(noise)
    assert cd.data_ptr() % 16 == 0 and zd.data_ptr() % 16 == 0
    got = sg.snr_mixer(cd, zd, _dev(snr))
    _check_snr([g.cpu().numpy() for g in got], clean, noise, snr)
    one = audio.snr_mixer(_dev(clean[1]), _dev(noise[1]), float(snr[1]))
    for k in range(3):
        assert one[k].shape == (N,) and torch.equal(one[k], got[k][1]), k


@pytest.mark.parametrize("N", [4000, PATHS["reg4"], PATHS["reg8"] + 4])
def test_snr_mixer_unaligned_view_takes_the_scalar_path(N):
    """a contiguous [B, N] view with N % 4 == 0 that starts one float off a 16-byte boundary: `vec` is false on the pointers,
    so snr_mixer_kernel runs its scalar loops over a length the vector paths would otherwise take"""
    from lidbox_amd.features import audio
    sg = _sg()
    B = 5
    clean, noise = _snr_inputs(N, B, N + 1)
    cbuf, zbuf = torch.zeros(B * N + 1, device="cuda"), torch.zeros(B * N + 1, device="cuda")
    cv, zv = cbuf[1:].view(B, N), zbuf[1:].view(B, N)
    cv.copy_(_dev(clean)); zv.copy_(_dev(noise))
    assert cv.is_contiguous() and cv.data_ptr() % 16 == 4 and zv.data_ptr() % 16 == 4
    got = sg.snr_mixer(cv, zv, _dev(SNR_DB))
    _check_snr([g.cpu().numpy() for g in got], clean, noise, SNR_DB)
    assert cv[1].data_ptr() % 16 == 4
    one = audio.snr_mixer(cv[1], zv[1], float(SNR_DB[1]))
    for k in range(3):
        assert torch.equal(one[k], got[k][1]), k


# ------------------------------------------------------------------ signal_chunks
def _chunk_signals(lens):
    return [(np.arange(n) % 977 + 1).astype(np.float32) * (1 + i) for i, n in enumerate(lens)]


def _check_chunks(sigs, sr, length_ms, step_ms, pad_ms):
    sg = _sg()
    chunks, nch = sg.signal_chunks(_aligned(sigs), sr, length_ms, step_ms, pad_ms)
    chunks = chunks.cpu().numpy()
    ref = [so.create_signal_chunks(s, sr, length_ms, step_ms, pad_ms) for s in sigs]
    assert [int(v) for v in nch] == [rf.shape[0] for rf in ref]
    ref = np.concatenate(ref, axis=0)
    assert chunks.shape == ref.shape
    return chunks, ref


@pytest.mark.parametrize("sr,length_ms,step_ms,pad_ms,step", [(22050, 25, 5, 0, 110), (22050, 10, 5, 10, 110), (22050, 5, 3, 2, 66),
                                                               (11025, 4, 1, 0, 11), (8000, 25, 3, 0, 24), (8000, 3, 3, 3, 24)])
def test_signal_chunks_with_steps_that_are_not_multiples_of_four(sr, length_ms, step_ms, pad_ms, step):
    """signal_chunks_kernel: the float4 copy needs `src + i` 16-byte aligned, i.e. chunk_row * S % 4 == 0.  With S = 110, 66
    or 11 samples most rows take the scalar branch over their whole length, not only at the tail (S = 24 is the aligned
    control at another rate)."""
    assert so.signal_chunk_plan(0, sr, length_ms, step_ms, pad_ms)[1] == step
    rng = np.random.default_rng(sr + step_ms)
    lens = [0, 1, 109, 110, 111, 551, 552, 1102, 22050, 22051, 40007] + [int(v) for v in rng.integers(0, 50000, size=8)]
    chunks, ref = _check_chunks(_chunk_signals(lens), sr, length_ms, step_ms, pad_ms)
    assert len(ref) > 100 and np.array_equal(chunks, ref)


@pytest.mark.parametrize("sr,length_ms,step_ms,lens", [(22050, 5, 1, [800001, 5, 799990]), (8000, 3, 1, [300000, 300004])])
def test_signal_chunks_second_launch_past_65535_chunks(sr, length_ms, step_ms, lens):
    """lidbox_signal_chunks launches grid.y = 65 535 chunk rows at a time; short chunks over long utterances plan more than
    that, so rows from 65 535 on come from the launch with c0 > 0.  Rows on both sides of the boundary, the last row and
    then the whole array, bit for bit."""
    chunks, ref = _check_chunks(_chunk_signals(lens), sr, length_ms, step_ms, 0)
    G = PATHS["grid_y"]
    assert len(ref) > G + 1000
    for row in (0, G - 1, G, G + 1, len(ref) - 1):
        assert np.array_equal(chunks[row], ref[row]), row
    assert np.array_equal(chunks, ref)


# ------------------------------------------------------------------ segment_mean
def _check_segment_mean(x, sizes):
    """|got - ref| <= 1.1 * 2^-24 * (sum_i |x_i| / rows + |ref|) per element, the sum over the segment's rows of that column.

    Derivation: adding `rows` fp32 values one after the other makes rows - 1 roundings, each at most 2^-24 of a partial sum
    that is itself at most sum_i |x_i|, so to first order the error of the sum is at most (rows - 1) * 2^-24 * sum_i |x_i|;
    dividing by `rows` scales that and adds one more rounding of 2^-24 * |ref|; 10 % covers the second-order terms.
    The asserted form carries sum_i |x_i| / rows, not (rows - 1) / rows * sum_i |x_i|: it is `rows - 1` times tighter than
    what a sequential fp32 sum can promise (measured in numpy: such a sum misses it by 26x at 5 000 rows of 1 + 0.1 N(0, 1)),
    and what holds for a kernel that keeps its running sum in float64 and rounds once: |got - ref| <= 2^-24 * |ref|.
    segment_mean_kernel accumulates in float64 for that reason."""
    from lidbox_amd import util
    sizes = np.asarray(sizes, np.int64)
    off = np.concatenate(([0], np.cumsum(sizes)))
    assert off[-1] == x.shape[0]
    got = util.segment_mean(_dev(x), off).cpu().numpy()
    x64 = x.astype(np.float64)
    ref = np.add.reduceat(x64, off[:-1], axis=0) / sizes[:, None]
    mean_abs = np.add.reduceat(np.abs(x64), off[:-1], axis=0) / sizes[:, None]
    assert got.shape == ref.shape and not np.isnan(got).any()
    bound = 1.1 * 2.0 ** -24 * (mean_abs + np.abs(ref))
    excess = np.abs(got - ref) - bound
    assert (excess <= 0).all(), (np.unravel_index(excess.argmax(), excess.shape), excess.max())


SEGMENT_SIZES = [1, 2, 3, 5000, 17, 256, 257, 1, 1000, 4999, 64]


@pytest.mark.parametrize("kind", ["gauss", "dc"])
@pytest.mark.parametrize("D", [1, 4, 100, 257, 1000])
def test_segment_mean_widths_and_segment_sizes(D, kind):
    rng = np.random.default_rng(D)
    x = rng.standard_normal((sum(SEGMENT_SIZES), D))
    x = (x if kind == "gauss" else 1.0 + 0.1 * x).astype(np.float32)
    _check_segment_mean(x, SEGMENT_SIZES)


def test_segment_mean_more_segments_than_one_grid_dimension():
    """util.segment_mean calls lidbox_segment_mean 65 535 segments at a time with offset pointers"""
    rng = np.random.default_rng(12)
    sizes = rng.integers(1, 4, size=PATHS["grid_y"] + 4465)
    x = (0.5 + rng.standard_normal((int(sizes.sum()), 4))).astype(np.float32)
    _check_segment_mean(x, sizes)


# ------------------------------------------------------------------ pcm16_to_f32
@pytest.mark.parametrize("frames,channels", [(PATHS["pcm_mono"] + 100003, 1), (PATHS["pcm_multi"] + 70001, 3)])
def test_pcm16_ingest_past_the_grid_cap_is_bit_exact(frames, channels):
    """more frames than 8192 workgroups cover in one trip of the grid-stride loop (vector mono loop / multi-channel loop)"""
    from lidbox_amd.features import audio
    rng = np.random.default_rng(channels)
    pcm = rng.integers(-32768, 32768, size=(frames, channels), dtype=np.int16)
    pcm[0, :], pcm[-1, :] = -32768, 32767
    ref = (pcm.astype(np.float32) / np.float32(32768.0)).mean(axis=1, dtype=np.float32)
    got = audio.pcm16_to_float(pcm, channels)
    assert got.dtype == torch.float32 and got.shape == (frames,)
    assert np.array_equal(got.cpu().numpy(), ref)
