"""
Timing of the ragged pass of crnn and clstm (docs/LAB_NOTEBOOK.md section 27) on one GPU:

    python tools/bench_ragged_conv.py [--models crnn,clstm] [--rounds 6] [--reps 3] [--out result.json]

Workload: the 256 utterances of sections 23 / 25 (98 .. 298 frames, 48 772 frames, 144 distinct lengths, seed 2024), 40 features,
crnn and clstm (all three flags) at the reference's widths.  Per model, HIP events around whole calls, every variant warmed up
first, the variants alternating round by round so that a drift of the machine lands on all of them:
    (a)  one predict_ragged over all utterances;
    (b)  the correct dense form: one dense call per distinct length, all 144 workspaces kept by the caller (the form that costs
         the dense path least: no workspace is ever rebuilt);
    (c)  one dense call on the batch zero-padded to 298 frames: wrong answers for all but the longest utterances, a cost
         yardstick only.
Then, for crnn's five layers on the same pixels, lidbox_conv2d_ragged_fwd against lidbox_conv2d_fwd at B = 1, T = total_T,
alternating: both run the same MFMA work (the dense call convolves across utterance borders, so its values differ there), the
difference is the row lookup and the registers it costs.
Reported: median (min .. max) in ms per variant and the largest |(a) - (b)| over all outputs.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, N_OUT, B, SEED = 40, 4, 256, 2024


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


def create(name):
    from lidbox_amd.models import clstm, crnn
    if name == "crnn":
        return crnn.create((None, C), N_OUT, seed=1)
    return clstm.create((None, C), N_OUT, seed=1, use_attention=True, use_conv2d=True, use_lstm=True)


def bench_model(name, rounds, reps):
    m = create(name)
    lengths, xs = workload()
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    X = torch.from_numpy(np.concatenate(xs)).cuda()
    groups = {int(T): np.flatnonzero(lengths == T) for T in sorted(set(lengths.tolist()))}
    dense_in = {T: torch.from_numpy(np.stack([xs[i] for i in idx])).cuda() for T, idx in groups.items()}
    padded = torch.zeros((B, int(lengths.max()), C), device="cuda")
    for b, x in enumerate(xs):
        padded[b, :len(x)] = torch.from_numpy(x).cuda()
    kept = {T: m.workspace_class(m, len(idx), T) for T, idx in groups.items()}
    kw = dict(normalize=True) if name == "crnn" else {}

    def ragged():
        return m.predict_ragged(X, off)

    def per_length_kept():
        out = {}
        for T, x in dense_in.items():
            m._load_input(kept[T], x, False)
            out[T] = m.forward_ws(kept[T], **kw).clone()
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
    res = dict(model=name, utterances=B, frames=int(lengths.sum()), distinct_lengths=len(groups),
               padded_frames=B * int(lengths.max()), ms={k: stats(v) for k, v in times.items()},
               max_abs_ragged_minus_per_length=dev, max_abs_padded_minus_ragged=pad_err)
    del kept, dense_in, padded
    torch.cuda.empty_cache()
    return res


def bench_kernel_pairs(rounds, reps):
    """crnn's five Conv2D layers on the workload's pixels: the ragged kernel against its dense twin at B = 1, T = total_T"""
    from lidbox_amd import _native as nv
    from lidbox_amd.models import crnn
    from lidbox_amd.models.conv_rnn import pooled_offsets, pooled_sizes
    lengths, _ = workload()
    offs = pooled_offsets(lengths, len(crnn.FILTERS))
    Fs = [F for _, F in pooled_sizes(1, C, len(crnn.FILTERS))]
    st, lib = nv.current_stream(), nv.lib
    out, cin = [], 1
    g = torch.Generator(device="cuda").manual_seed(SEED)
    for i, (co, k) in enumerate(zip(crnn.FILTERS, crnn.KERNELS)):
        rows, F = int(offs[i][-1]), Fs[i]
        x = torch.randn((rows, F, cin), device="cuda", generator=g)
        W = torch.randn((k, k, cin, co), device="cuda", generator=g) / k
        bias = torch.randn(co, device="cuda", generator=g)
        y = torch.empty((rows, F, co), device="cuda")
        od = torch.from_numpy(offs[i]).cuda()

        def ragged():
            nv.check(lib.lidbox_conv2d_ragged_fwd(nv.ptr(x), nv.ptr(od), B, rows, F, cin, nv.ptr(W), k, co, nv.ptr(bias), 1, nv.ptr(y), st))

        def dense():
            nv.check(lib.lidbox_conv2d_fwd(nv.ptr(x), 1, rows, F, cin, nv.ptr(W), k, co, nv.ptr(bias), 1, nv.ptr(y), st))

        pair = dict(ragged=ragged, dense=dense)
        for fn in pair.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {n: [] for n in pair}
        for _ in range(rounds):
            for n, fn in pair.items():
                for _ in range(reps):
                    times[n].append(timed(fn)[0])
        out.append(dict(layer=i + 1, rows=rows, F=F, C_in=cin, C_out=co, k=k, pixels=rows * F, ms={n: stats(v) for n, v in times.items()}))
        cin = co
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="crnn,clstm")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel pairs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_conv.py measures on a GPU; none is visible")
    results = []
    for name in [n for n in args.models.split(",") if n]:
        res = bench_model(name, args.rounds, args.reps)
        results.append(res)
        print(json.dumps(res), flush=True)
    if not args.no_kernels:
        res = dict(kernel_pairs=bench_kernel_pairs(args.rounds, args.reps))
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
