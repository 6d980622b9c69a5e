"""
Every kernel and template instantiation of the augmentation files (csrc/augment.hip: lidbox_resample, lidbox_fir_filter;
csrc/mix_noise.hip: lidbox_mix_noise, lidbox_signal_tile) on each side of each dispatch condition, through the C ABI, against
the float64 references of oracle/augment_paths_np.py.

The shapes that select a path sit in that module's PATHS tables (RESAMPLE, FIR, MIX, TILE), each row with the condition it is
there for; tests/test_oracle_augment_paths.py proves on the CPU that every row selects what it says, that the rows reach
every (stage, logP) pair, class, form, trip count and launch-site kernel, and which planted mistakes the resample tolerance
catches.

Buffers.  Signals, the noise bank, coefficients, outputs and workspaces are tests/guarded.py payloads.  Utterances lie at
start residues 0 .. 3 modulo 4 with gaps of 4 .. 7 words; the gaps hold NaN going in and the same NaN coming out, in inputs
and in outputs; outputs start as NaN; inputs are compared bit for bit with their host copies after every call.  Workspaces
have exactly the size the library returns (asserted equal to the restated size).  One resample row and one mix row repeat
with a workspace one byte short and with one 4 bytes off its alignment: both are refused with nothing written.

Judging.  Resample: relative L2 error <= 4e-6 and max error <= 4e-6 max|x| per utterance (the project's tolerance; no row
needed another).  FIR: element by element within conv2d_np.error_bound(S, K); y[0] is the exact fp32 product on every row and
K = 1 is bit-exact throughout; rows with K >= 4095 also run on sparse taps, where the same bound is tight enough for one lost
sample of the halo (oracle/augment_paths_np.py, section 5).  Mix: 2e-5 max|ref|.  Tile: bit-exact.  Exact identities: run to run (every row runs twice);
an utterance alone, first and last in a batch; an utterance of each of the three groups of the 600-utterance batch; one
(utterance, clip, snr) at every utterance, clip and output residue; one signal at FIR residues 0 .. 3; empty calls.
Each row runs on "normal" N(0, 1) and "offset" 1 + 0.1 N(0, 1); resample rows whose utterance has N even and M >= N also on
the Nyquist tone; rows with logP >= 19, n = 2^21 or a tile output above 4 M samples on one set.

First measured (MI355X, one run, 186 cases in 4.5 s, the slowest 0.5 s).  Resample, largest of (relative L2, max error /
max|x|) over the rows of a transform size, as a fraction of the 4e-6 tolerance, the same for both stages unless two figures
are given (stage 0 / stage 1): logP 0: 0 / 0.008, 1: 0.008 / 0, 2: 0.021, 3: 0.057, 4: 0.140, 5: 0.104 / 0.125, 6: 0.119, 7: 0.149,
8: 0.178, 9: 0.178, 10: 0.208, 11: 0.223, 12: 0.208, 13: 0.252, 14: 0.267, 15: 0.327, 16: 0.335, 17: 0.356, 18: 0.356, 19: 0.136,
20: 0.117, 21: 0.130, 22: 0.127 (19 .. 22 on N(0, 1) only; below that the largest figure is the max error of the offset or the tone
set).  Largest absolute figure: 1.42e-6.  FIR err / bound: 0.450 normal, 0.367 offset, 8.4e-4 sparse.  Mix err / (2e-5 max|ref|),
normal / offset: <4,0> 0.020 / 0.008, <8,0> 0.005 / 0.011, <8,8> 0.007 / 0.012, tiled 0.007 / 0.011.  Tile and every identity: bit-equal.
"""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Guarded
from oracle import augment_paths_np as ap

pytestmark = pytest.mark.gpu

WORST = {}                                           # group -> largest err / bound seen
# no 0 dB: a one-sample utterance and a one-sample-period clip of opposite sign are both normalised to exactly -25 dBFS and
# cancel to an exact zero there, against which a relative bound has no meaning
SNRS = (-5.0, 1.0, 3.0, 10.0, 20.0)
NAN32 = np.float32(np.nan)


def _nv():
    from lidbox_amd import _native as nv
    return nv


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(a, b):
    """bit for bit, NaN payloads included"""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _note(group, q):
    WORST[group] = max(WORST.get(group, 0.0), float(q))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _starts(lengths, residues):
    """start offsets with the given residues modulo 4 and 4 .. 7 words before every utterance; the words of the buffer"""
    starts, pos = [], 0
    for n, r in zip(lengths, residues):
        pos += 4
        pos += (r - pos) % 4
        starts.append(pos)
        pos += n
    return starts, pos + 5


def _packed(arrays, starts, total):
    """a guarded NaN-filled buffer with the arrays at their starts, and its host copy"""
    host = np.full(total, NAN32, np.float32)
    for a, s in zip(arrays, starts):
        host[s:s + len(a)] = a
    return Guarded((total,), init=torch.from_numpy(host)), host


def _split(g, host_before, starts, lengths, what):
    """the pieces of a guarded buffer; everything outside them still holds what it held (NaN)"""
    y = g.numpy().copy()
    mask = np.zeros(len(y), bool)
    for s, n in zip(starts, lengths):
        mask[s:s + n] = True
    assert _same(y[~mask], host_before[~mask]) and np.isnan(y[~mask]).all(), "%s: a gap was written" % what
    return [y[s:s + n] for s, n in zip(starts, lengths)]


def _ws(nbytes, shift=0):
    return Guarded((nbytes + shift,), dtype=torch.uint8) if nbytes + shift else None


def _ws_untouched(ws):
    ws.check()
    assert bool((ws.view == 0xA5).all()), "the workspace of a refused call was written"


# ---------------------------------------------------------------------------------------------------- resample
def run_resample(utts, xs, ws_short=0, ws_shift=0, expect=0, rin=1, rout=2):
    nv = _nv()
    lib = nv.lib
    B = len(utts)
    ns, ms = [u[0] for u in utts], [u[1] for u in utts]
    in_starts, in_total = _starts(ns, [(rin + i) % 4 for i in range(B)])
    out_starts, out_total = _starts(ms, [(rout + 3 * i) % 4 for i in range(B)])
    xin, host_in = _packed(xs, in_starts, in_total)
    yout = Guarded((out_total,))
    host_out = np.full(out_total, NAN32, np.float32)
    n_h, m_h = np.asarray(ns, np.int64), np.asarray(ms, np.int64)
    nbytes = lib.lidbox_resample_workspace(n_h.ctypes.data, m_h.ctypes.data, B)
    assert nbytes == ap.rs_workspace(utts)
    ws = _ws(nbytes, ws_shift)
    wptr = ctypes.c_void_p(ws.view.data_ptr() + ws_shift) if ws is not None else None
    assert ws is None or ws.view.data_ptr() % 16 == 0
    dev = [_dev(a, np.int64) for a in (in_starts, ns, out_starts, ms)]
    st = lib.lidbox_resample(xin.ptr, _p(dev[0]), _p(dev[1]), yout.ptr, _p(dev[2]), _p(dev[3]), n_h.ctypes.data,
                             m_h.ctypes.data, B, wptr, nbytes - ws_short, nv.current_stream())
    torch.cuda.synchronize()
    assert st == expect, (st, nv.last_error())
    assert _same(xin.numpy(), host_in), "the input (or a gap of it) was modified"
    if ws is not None:
        ws.check()
    if expect != 0:
        assert np.isnan(yout.numpy()).all(), "a refused call wrote output"
        _ws_untouched(ws)
        return None
    return _split(yout, host_out, out_starts, ms, "resample out")


def _judge_resample(r, kind, utts, xs, ys):
    worst = (0.0, 0.0)
    for (N, M), x, y in zip(utts, xs, ys):
        assert y.shape == (M,)
        if not M:
            continue
        assert np.isfinite(y).all(), "%s: output of (%d, %d) not fully written" % (r["name"], N, M)
        rel, mx = ap.rs_errors(y, ap.resample_ref(x, M), x)
        worst = (max(worst[0], rel), max(worst[1], mx))
        for stage, lp in enumerate(ap.rs_logp(N, M)):
            _note("resample s%d logP=%02d" % (stage, lp), max(rel, mx) / ap.RS_TOL)
    tol = ap.RS_TOL_OVERRIDE.get((r["name"], kind), ap.RS_TOL)
    print("resample %-18s %-8s rel L2 %.3e  max / max|x| %.3e  (tolerance %.1e)" % (r["name"], kind, *worst, tol))
    assert worst[0] <= tol and worst[1] <= tol, (r["name"], kind, worst)


RS_CASES = [(r, kind) for r in ap.RESAMPLE for kind in ap.rs_kinds(r)]


@pytest.mark.parametrize("r,kind", RS_CASES, ids=["%s-%s" % (r["name"], k) for r, k in RS_CASES])
def test_resample_row(r, kind):
    utts = r["utts"]
    xs = ap.rs_draw(r, kind)
    ys = run_resample(utts, xs)
    _judge_resample(r, kind, utts, xs, ys)
    again = run_resample(utts, xs)
    assert all(_same(a, b) for a, b in zip(ys, again)), "%s: a second run gives other bits" % r["name"]
    if r["name"] == "b600" and kind == "normal":
        groups = ap.rs_groups(utts, 0)
        assert [len(u) for _, u, _ in groups] == [256, 256, 88]
        for _, members, _ in groups:                         # an utterance of each group, alone
            for b in (members[0], members[-1]):
                assert _same(run_resample([utts[b]], [xs[b]])[0], ys[b]), "utterance %d alone differs" % b


@pytest.mark.parametrize("utt", [(700, 650), (13, 9), (20001, 18181), (1, 2)])
def test_a_resampled_utterance_is_bit_identical_alone_first_and_last_in_a_batch(utt):
    others = [(12, 10), (2732, 2732), (0, 0), (21846, 21846), (9, 12), (5, 0)]
    x = ap.draw("normal", utt[0], 77)
    ox = [ap.draw("offset", N, 78 + i) for i, (N, _) in enumerate(others)]
    alone = run_resample([utt], [x], rin=0, rout=0)[0]
    first = run_resample([utt] + others, [x] + ox)[0]
    last = run_resample(others + [utt], ox + [x], rin=3, rout=1)[-1]
    assert _same(alone, first) and _same(alone, last)


@pytest.mark.parametrize("how", ["one_byte_short", "misaligned"])
def test_resample_refuses_a_bad_workspace_and_writes_nothing(how):
    r = next(x for x in ap.RESAMPLE if x["name"] == "long_among_short")
    xs = ap.rs_draw(r, "normal")
    if how == "one_byte_short":
        run_resample(r["utts"], xs, ws_short=1, expect=-1)
    else:
        run_resample(r["utts"], xs, ws_shift=4, expect=-1)
    assert "workspace" in _nv().last_error()


# ---------------------------------------------------------------------------------------------------- FIR
def run_fir(K, ns, xs, fs, r0=0):
    nv = _nv()
    B = len(ns)
    starts, total = _starts(ns, [(r0 + i) % 4 for i in range(B)])
    x, host = _packed(xs, starts, total)
    y = Guarded((total,))
    coefs = Guarded((B, K), init=torch.from_numpy(np.asarray(fs, np.float32)))
    dev = [_dev(starts, np.int64), _dev(ns, np.int64)]
    nv.check(nv.lib.lidbox_fir_filter(x.ptr, _p(dev[0]), _p(dev[1]), B, max(ns), coefs.ptr, K, y.ptr, nv.current_stream()))
    torch.cuda.synchronize()
    assert _same(x.numpy(), host) and _same(coefs.numpy(), np.asarray(fs, np.float32)), "an input was modified"
    return _split(y, np.full(total, NAN32, np.float32), starts, ns, "fir out")


FIR_CASES = [(r, kind) for r in ap.FIR for kind in ap.fir_kinds(r)]


@pytest.mark.parametrize("r,kind", FIR_CASES, ids=["%s-%s" % (r["name"], k) for r, k in FIR_CASES])
def test_fir_row(r, kind):
    K, ns = r["K"], r["ns"]
    xs = [ap.draw("normal" if kind == "sparse" else kind, n, 200 + i) for i, n in enumerate(ns)]
    fs = np.stack([ap.fir_coefs(kind, K, 300 + i) for i in range(len(ns))])
    ys = run_fir(K, ns, xs, fs)
    worst = 0.0
    for x, f, y in zip(xs, fs, ys):
        ref, S = ap.fir_ref(x, f)
        q = np.abs(y.astype(np.float64) - ref) / ap.error_bound(S, K)
        assert np.isfinite(y).all()
        worst = max(worst, float(q.max()))
        assert (q <= 1.0).all(), "%s n=%d: %d outputs over the bound, worst %.3g x at %d" % (
            r["name"], len(x), (q > 1).sum(), q.max(), int(np.argmax(q)))
        assert _bits(y[:1])[0] == _bits(np.float32(f[0]) * x[:1])[0], "y[0] is not the exact product f[0] x[0]"
        if K == 1:
            assert _same(y, np.float32(f[0]) * x)
    _note("fir/%s" % kind, worst)
    print("fir %-12s %-7s max err/bound=%.3e" % (r["name"], kind, worst))
    again = run_fir(K, ns, xs, fs)
    assert all(_same(a, b) for a, b in zip(ys, again))


@pytest.mark.parametrize("K,n", [(9, 4099), (4096, 4099), (3, 7)])
def test_fir_gives_the_same_bits_at_every_start_residue(K, n):
    x, f = ap.draw("normal", n, 5), ap.draw("normal", K, 6)[None]
    outs = [run_fir(K, [n], [x], f, r0=r)[0] for r in range(4)]
    assert all(_same(outs[0], o) for o in outs[1:])
    # and inside a batch, behind a longer neighbour
    both = run_fir(K, [131073, n], [ap.draw("offset", 131073, 7), x], np.concatenate([f, f]), r0=1)
    assert _same(both[1], outs[0])


# ---------------------------------------------------------------------------------------------------- mix
def run_mix(utts, ures, clips, cres, jobs, ores, ws_short=0, ws_shift=0, expect=0):
    """jobs: (utterance, clip, snr) per output; *res: the start residue of every utterance, clip, output"""
    nv = _nv()
    lib = nv.lib
    B, M, J = len(utts), len(clips), len(jobs)
    ns, cl = [len(u) for u in utts], [len(c) for c in clips]
    outn = [ns[b] for b, _, _ in jobs]
    us, ut = _starts(ns, ures)
    cs, ct = _starts(cl, cres)
    os_, ot = _starts(outn, ores)
    sig, sig_h = _packed(utts, us, ut)
    bank, bank_h = _packed(clips, cs, ct)
    out = Guarded((ot,))
    src_h, clip_h = np.asarray([j[0] for j in jobs], np.int32), np.asarray([j[1] for j in jobs], np.int32)
    n_h, c_h = np.asarray(ns, np.int64), np.asarray(cl, np.int64)
    nbytes = lib.lidbox_mix_noise_workspace(max(outn, default=0), J)
    assert nbytes == ap.mix_workspace(max(outn, default=0), J)
    ws = _ws(nbytes, ws_shift)
    wptr = ctypes.c_void_p(ws.view.data_ptr() + ws_shift) if ws is not None else None
    dev = [_dev(us, np.int64), _dev(ns, np.int64), _dev(cs, np.int64), _dev(cl, np.int64), _dev(src_h, np.int32),
           _dev(clip_h, np.int32), _dev([j[2] for j in jobs], np.float32), _dev(os_, np.int64)]
    st = lib.lidbox_mix_noise(sig.ptr, _p(dev[0]), _p(dev[1]), bank.ptr, _p(dev[2]), _p(dev[3]), _p(dev[4]), _p(dev[5]),
                              _p(dev[6]), out.ptr, _p(dev[7]), n_h.ctypes.data, c_h.ctypes.data, src_h.ctypes.data,
                              clip_h.ctypes.data, B, M, J, wptr, nbytes - ws_short, nv.current_stream())
    torch.cuda.synchronize()
    assert st == expect, (st, nv.last_error())
    assert _same(sig.numpy(), sig_h) and _same(bank.numpy(), bank_h), "an input (or a gap of it) was modified"
    if ws is not None:
        ws.check()
    if expect != 0:
        assert np.isnan(out.numpy()).all(), "a refused call wrote output"
        _ws_untouched(ws)
        return None
    assert [s % 4 for s in os_] == [r % 4 for r in ores]
    return _split(out, np.full(ot, NAN32, np.float32), os_, outn, "mix out")


def _mix_row_call(r, kind, **kw):
    n, ms = r["n"], r["ms"]
    utt = ap.draw(kind, n, 400)
    clips = [np.float32(0.3) * ap.draw(kind, m, 500 + j) for j, m in enumerate(ms)]
    jobs = [(0, j, SNRS[j % 5]) for j in range(len(ms))]
    ys = run_mix([utt], [r["res"][0]], clips, [(r["res"][1] + j) % 4 for j in range(len(ms))], jobs,
                 [(1 + j) % 4 for j in range(len(ms))], **kw)
    return utt, clips, jobs, ys


MIX_CASES = [(r, kind) for r in ap.MIX for kind in (ap.KINDS[:1] if ap.mix_one_set(r) else ap.KINDS)]


@pytest.mark.parametrize("r,kind", MIX_CASES, ids=["%s-%s" % (r["name"], k) for r, k in MIX_CASES])
def test_mix_row(r, kind):
    utt, clips, jobs, ys = _mix_row_call(r, kind)
    worst = 0.0
    for (b, k, snr), y in zip(jobs, ys):
        ref = ap.mix_ref(utt, clips[k], snr)
        assert np.isfinite(y).all()
        q = np.abs(y - ref).max() / (ap.MIX_TOL * np.abs(ref).max())
        worst = max(worst, float(q))
        assert q <= 1.0, (r["name"], kind, len(clips[k]), snr, q)
    _note("mix %s/%s" % (ap.mix_form(r["n"]), kind), worst)
    print("mix %-8s %-7s max err/bound=%.3e" % (r["name"], kind, worst))
    again = _mix_row_call(r, kind)[3]
    assert all(_same(a, b) for a, b in zip(ys, again))


RES3 = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 2, 3),
        (3, 1, 2), (2, 3, 1)]


@pytest.mark.parametrize("m", [7, 60001])
@pytest.mark.parametrize("n", [5, 4099, 16385, 32769, 65537, 73729])
def test_mix_gives_the_same_bits_at_every_residue(n, m):
    """the vector and the scalar access paths load the same values and add them in the same order"""
    utt, clip = ap.draw("normal", n, 1), np.float32(0.3) * ap.draw("normal", m, 2)
    ys = run_mix([utt] * 4, [0, 1, 2, 3], [clip] * 4, [0, 1, 2, 3], [(u, c, 3.0) for u, c, _ in RES3], [o for _, _, o in RES3])
    assert all(_same(ys[0], y) for y in ys[1:])
    ref = ap.mix_ref(utt, clip, 3.0)
    assert np.abs(ys[0] - ref).max() <= ap.MIX_TOL * np.abs(ref).max()


@pytest.mark.parametrize("n", [5, 16384, 32769, 65536, 73729])
def test_a_mixed_output_is_bit_identical_alone_first_and_last_in_a_batch(n):
    lens = [n, 16385, 3, 65537, 0, 32768]
    utts = [ap.draw("normal", k, 10 + i) for i, k in enumerate(lens)]
    clips = [np.float32(0.3) * ap.draw("normal", m, 20 + i) for i, m in enumerate((60001, 5, 8))]
    alone = run_mix([utts[0]], [0], [clips[0]], [0], [(0, 0, 10.0)], [0])[0]
    others = [(1, 1, 0.0), (2, 2, 3.0), (3, 0, -5.0), (4, 1, 0.0), (5, 2, 20.0), (0, 1, 10.0)]
    res = [0, 1, 2, 3, 0, 1]
    first = run_mix(utts, res, clips, [1, 2, 3], [(0, 0, 10.0)] + others, [0, 1, 2, 3, 0, 1, 2])
    last = run_mix(utts, res, clips, [1, 2, 3], others + [(0, 0, 10.0)], [3, 2, 1, 0, 3, 2, 1])
    assert _same(alone, first[0]) and _same(alone, last[-1])
    assert not _same(alone, first[-1])                       # another clip gives another result


@pytest.mark.parametrize("how", ["one_byte_short", "misaligned"])
def test_mix_refuses_a_bad_workspace(how):
    """the resident launches of a batch come before the workspace is looked at, so the row is one with tiled outputs only:
    nothing is written"""
    r = next(x for x in ap.MIX if x["name"] == "n65537")
    kw = dict(ws_short=1) if how == "one_byte_short" else dict(ws_shift=4)
    _mix_row_call(r, "normal", expect=-1, **kw)
    assert "workspace" in _nv().last_error()


# ---------------------------------------------------------------------------------------------------- tile
@pytest.mark.parametrize("r", ap.TILE, ids=lambda r: r["name"])
def test_tile_row(r):
    nv = _nv()
    items = r["items"]
    B = len(items)
    for kind in (ap.KINDS[:1] if ap.tile_one_set(r) else ap.KINDS):
        xs = [ap.draw(kind, n, 600 + i) for i, (n, _) in enumerate(items)]
        ns, reps = [n for n, _ in items], [k for _, k in items]
        totals = [n * k for n, k in items]
        starts, total = _starts(ns, [i % 4 for i in range(B)])
        os_, ot = _starts(totals, [(i + 1) % 4 if i else 0 for i in range(B)])
        x, host = _packed(xs, starts, total)
        y = Guarded((ot,))
        dev = [_dev(starts, np.int64), _dev(ns, np.int64), _dev(reps, np.int64), _dev(os_, np.int64)]
        nv.check(nv.lib.lidbox_signal_tile(x.ptr, _p(dev[0]), _p(dev[1]), _p(dev[2]), y.ptr, _p(dev[3]), B, max(totals),
                                           nv.current_stream()))
        torch.cuda.synchronize()
        assert _same(x.numpy(), host)
        ys = _split(y, np.full(ot, NAN32, np.float32), os_, totals, "tile out")
        for xi, k, yi in zip(xs, reps, ys):
            assert _same(yi, np.tile(xi, k)), "%s: n=%d x %d is not the tiled signal" % (r["name"], len(xi), k)


# ---------------------------------------------------------------------------------------------------- empty calls
def test_empty_calls_touch_nothing():
    nv = _nv()
    lib = nv.lib
    st = nv.current_stream()
    # through the helpers: every buffer guarded, gaps and guards checked
    assert run_resample([], []) == []
    assert [len(y) for y in run_resample([(0, 0), (5, 0)], [np.zeros(0, np.float32), ap.draw("normal", 5, 1)])] == [0, 0]
    x5 = ap.draw("normal", 5, 1)
    assert run_mix([x5], [1], [x5], [2], [], []) == []                                                  # J = 0
    assert [len(y) for y in run_mix([np.zeros(0, np.float32)], [0], [x5], [0], [(0, 0, 3.0)], [1])] == [0]   # n = 0 only
    # raw calls on NaN buffers
    bufs = [Guarded((64,)) for _ in range(4)]
    a, b, c, d = (g.ptr for g in bufs)
    idx = _dev([0, 0], np.int64)
    zero_h = np.zeros(2, np.int64)
    i32_h = np.zeros(2, np.int32)
    i32 = _dev(i32_h, np.int32)
    assert lib.lidbox_resample(a, _p(idx), _p(idx), b, _p(idx), _p(idx), zero_h.ctypes.data, zero_h.ctypes.data, 0, None, 0, st) == 0
    assert lib.lidbox_fir_filter(a, _p(idx), _p(idx), 0, 10, c, 3, b, st) == 0                           # B = 0
    assert lib.lidbox_fir_filter(a, _p(idx), _p(idx), 2, 0, c, 3, b, st) == 0                            # max_length = 0
    assert lib.lidbox_mix_noise(a, _p(idx), _p(idx), c, _p(idx), _p(idx), _p(i32), _p(i32), d, b, _p(idx), zero_h.ctypes.data,
                                zero_h.ctypes.data, i32_h.ctypes.data, i32_h.ctypes.data, 0, 0, 0, None, 0, st) == 0      # B = M = J = 0
    assert lib.lidbox_signal_tile(a, _p(idx), _p(idx), _p(idx), b, _p(idx), 0, 10, st) == 0             # B = 0
    assert lib.lidbox_signal_tile(a, _p(idx), _p(idx), _p(idx), b, _p(idx), 2, 0, st) == 0              # max_out_length = 0
    torch.cuda.synchronize()
    for g in bufs:
        assert np.isnan(g.numpy()).all()
    # empty utterances between real ones in a FIR batch
    xs = [np.zeros(0, np.float32), ap.draw("normal", 9, 2), np.zeros(0, np.float32)]
    ys = run_fir(3, [0, 9, 0], xs, np.stack([ap.draw("normal", 3, 3)] * 3))
    assert [len(y) for y in ys] == [0, 9, 0] and np.isfinite(ys[1]).all()
    assert lib.lidbox_resample_workspace(zero_h.ctypes.data, zero_h.ctypes.data, 2) == 0 and lib.lidbox_mix_noise_workspace(0, 5) == 0


def test_zz_report():
    """the largest err / bound of every group of this run (docs/LAB_NOTEBOOK.md section 26 records one such run)"""
    for g in sorted(WORST):
        print("WORST %-28s %.3e" % (g, WORST[g]))
    assert all(v <= 1.0 for v in WORST.values())
