"""
Timing of the ragged pass of multilevel_attention (docs/LAB_NOTEBOOK.md section 29) on one GPU:

    python tools/bench_ragged_mla.py [--rounds 6] [--reps 3] [--out result.json]

Workload: the 256 utterances of sections 23 / 25 / 27 (98 .. 298 frames, 48 772 frames, 144 distinct lengths, seed 2024), 40
features, the reference's widths (L = 2, H = 512), K = 100.  HIP events around whole calls, every variant warmed up first, the
variants alternating round by round so that a drift of the machine lands on all of them:
    (a)  one predict_ragged over all utterances;
    (b)  the correct dense form: one dense call per distinct length, all 144 workspaces kept by the caller (the form that costs
         the dense path least: no workspace is ever rebuilt);
    (c)  one dense call on the batch zero-padded to 298 frames: wrong answers for all but the longest utterances, a cost
         yardstick only.
Then the kernel pair on logits [rows, K]: lidbox_mla_attention_fwd at B = 256, T = 190 against lidbox_mla_attention_ragged_fwd
on the same 48 640 rows cut into 256 utterances of 190 frames (equal rows and equal work per workgroup: what remains is the
offset load), and the ragged kernel on the workload's own lengths (48 772 rows, workgroups of unequal length); a launch takes
a few microseconds, so a kernel measurement is 20 launches between one pair of events, divided by 20.
Reported: median (min .. max) in ms per variant and the largest |(a) - (b)| over all outputs.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, K, LEVELS, UNITS, B, SEED = 40, 100, 2, 512, 256, 2024


def workload():
    """lengths in frames of section 21's signals (1 .. 3 s at 16 kHz in 10-ms multiples, 25-ms windows every 10 ms) and features"""
    samples = np.random.default_rng(SEED).integers(100, 301, B) * 160
    lengths = (samples - 400) // 160 + 1
    rng = np.random.default_rng(SEED + 1)
    xs = [rng.standard_normal((int(T), C)).astype(np.float32) for T in lengths]
    return lengths, xs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v)) if v else None


def bench_model(rounds, reps):
    from lidbox_amd.models import multilevel_attention
    m = multilevel_attention.create((None, C), K, L=LEVELS, H=UNITS, seed=1)
    # a BatchNormalization that is not the identity and biases that are not zero, as after training
    rng = np.random.default_rng(SEED + 2)
    w = m.get_weights()
    for n in w:
        if n.endswith(".b") or n.endswith(".beta") or n.endswith(".moving_mean"):
            w[n] = (0.2 * rng.standard_normal(w[n].shape)).astype(np.float32)
        elif n.endswith(".moving_variance"):
            w[n] = rng.uniform(0.5, 1.5, w[n].shape).astype(np.float32)
    m.set_weights(w)
    lengths, xs = workload()
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    X = torch.from_numpy(np.concatenate(xs)).cuda()
    groups = {int(T): np.flatnonzero(lengths == T) for T in sorted(set(lengths.tolist()))}
    dense_in = {T: torch.from_numpy(np.stack([xs[i] for i in idx])).cuda() for T, idx in groups.items()}
    padded = torch.zeros((B, int(lengths.max()), C), device="cuda")
    for b, x in enumerate(xs):
        padded[b, :len(x)] = torch.from_numpy(x).cuda()
    kept = {T: m.workspace_class(m, len(idx), T) for T, idx in groups.items()}

    def ragged():
        return m.predict_ragged(X, off)

    def per_length_kept():
        out = {}
        for T, x in dense_in.items():
            m._load_input(kept[T], x, False)
            out[T] = m.forward_ws(kept[T], normalize=True).clone()
        return out

    def padded_call():
        return m(padded)

    variants = dict(a_ragged=ragged, b_per_length_kept=per_length_kept, c_padded=padded_call)
    for fn in variants.values():                              # warm-up: code objects, workspaces, GEMM plans
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            for _ in range(1 if k.startswith("b_") else reps):
                times[k].append(timed(fn)[0])
    a = ragged().cpu().numpy()
    dev = 0.0
    for T, o in per_length_kept().items():
        dev = max(dev, float(np.abs(o.cpu().numpy() - a[groups[T]]).max()))
    pad_err = float(np.abs(padded_call().cpu().numpy() - a).max())
    res = dict(model="multilevel_attention", utterances=B, frames=int(lengths.sum()), distinct_lengths=len(groups),
               padded_frames=B * int(lengths.max()), ms={k: stats(v) for k, v in times.items()},
               max_abs_ragged_minus_per_length=dev, max_abs_padded_minus_ragged=pad_err)
    del kept, dense_in, padded
    torch.cuda.empty_cache()
    return res


def bench_kernel_pair(rounds, reps):
    """the attention pooling alone: the dense kernel, the ragged kernel on the same rows in equal utterances, and the ragged
    kernel on the workload's lengths"""
    from lidbox_amd import _native as nv
    lengths, _ = workload()
    T = int(lengths.sum()) // B
    rows_eq, rows_wl = B * T, int(lengths.sum())
    st, lib = nv.current_stream(), nv.lib
    g = torch.Generator(device="cuda").manual_seed(SEED)
    z = torch.randn((max(rows_eq, rows_wl), K), device="cuda", generator=g)
    att, colsum = torch.empty((B, LEVELS * K), device="cuda"), torch.empty((B, K), device="cuda")
    off_eq = torch.arange(B + 1, dtype=torch.int64, device="cuda") * T
    off_wl = torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)).cuda()

    def dense():
        nv.check(lib.lidbox_mla_attention_fwd(nv.ptr(z), B, T, K, nv.ptr(att), LEVELS * K, nv.ptr(colsum), st))

    def ragged_equal():
        nv.check(lib.lidbox_mla_attention_ragged_fwd(nv.ptr(z), nv.ptr(off_eq), B, K, nv.ptr(att), LEVELS * K, nv.ptr(colsum), st))

    def ragged_equal_no_colsum():
        nv.check(lib.lidbox_mla_attention_ragged_fwd(nv.ptr(z), nv.ptr(off_eq), B, K, nv.ptr(att), LEVELS * K, None, st))

    def ragged_workload():
        nv.check(lib.lidbox_mla_attention_ragged_fwd(nv.ptr(z), nv.ptr(off_wl), B, K, nv.ptr(att), LEVELS * K, None, st))

    pair = dict(dense=dense, ragged_equal=ragged_equal, ragged_equal_no_colsum=ragged_equal_no_colsum, ragged_workload=ragged_workload)
    for fn in pair.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dense()
    want = att.clone()
    ragged_equal()
    same = bool(torch.equal(want.view(torch.int32)[:, :K], att.view(torch.int32)[:, :K]))
    times = {n: [] for n in pair}
    inner = 20                                                # launches per event pair: one launch is a few microseconds

    def burst(fn):
        for _ in range(inner):
            fn()

    for _ in range(rounds):
        for n, fn in pair.items():
            for _ in range(reps):
                times[n].append(timed(lambda: burst(fn))[0] / inner)
    return dict(K=K, B=B, T_equal=T, rows_equal=rows_eq, rows_workload=rows_wl, ragged_equal_bits_match_dense=same,
                launches_per_measurement=inner, ms={n: stats(v) for n, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel pair")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_mla.py measures on a GPU; none is visible")
    results = [bench_model(args.rounds, args.reps)]
    print(json.dumps(results[-1]), flush=True)
    if not args.no_kernels:
        results.append(dict(kernel_pair=bench_kernel_pair(args.rounds, args.reps)))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
