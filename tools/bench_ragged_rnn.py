"""
Timing of the ragged recurrent pass (docs/LAB_NOTEBOOK.md section 25) on one GPU:

    python tools/bench_ragged_rnn.py [--models spherespeaker,bi_gru] [--rounds 6] [--reps 3] [--out result.json]

Workload: the 256 utterances of section 23 (98 .. 298 frames, 48 772 frames, 144 distinct lengths, seed 2024), 40 features, the
models at the reference's widths.  Per model, HIP events around whole calls, every variant warmed up first, the variants
alternating round by round so that a drift of the machine lands on all of them:
    (a)  one predict_ragged over all utterances;
    (b)  the correct dense form: one dense call per distinct length -- with the model's own cache of four (B, T) workspaces (every
         call builds one; timed in the first two rounds only, it takes seconds) and with all 144 workspaces kept by the caller;
    (c)  one dense call on the batch zero-padded to 298 frames: wrong answers for all but the longest utterances, a cost
         yardstick only.
Reported: median (min .. max) in ms per variant, launches of the walk per pass, and the largest |(a) - (b)| over all outputs.
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


def bench_model(name, rounds, reps):
    from lidbox_amd.models import bi_gru, spherespeaker
    m = (spherespeaker if name == "spherespeaker" else bi_gru).create((None, C), N_OUT, seed=1)
    lengths, xs = workload()
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    X = torch.from_numpy(np.concatenate(xs)).cuda()
    groups = {int(T): np.flatnonzero(lengths == T) for T in sorted(set(lengths.tolist()))}
    dense_in = {T: torch.from_numpy(np.stack([xs[i] for i in idx])).cuda() for T, idx in groups.items()}
    padded = torch.zeros((B, int(lengths.max()), C), device="cuda")
    for b, x in enumerate(xs):
        padded[b, :len(x)] = torch.from_numpy(x).cuda()
    kept = {T: m.workspace_class(m, len(idx), T) for T, idx in groups.items()}      # (b) with every workspace kept by the caller

    def ragged():
        return m.predict_ragged(X, off)

    def per_length():
        return {T: m(x) for T, x in dense_in.items()}

    def per_length_kept():
        out = {}
        for T, x in dense_in.items():
            m._load_input(kept[T], x, False)
            out[T] = m.forward_ws(kept[T], normalize=True).clone()
        return out

    def padded_call():
        return m(padded)

    variants = dict(a_ragged=ragged, b_per_length_kept=per_length_kept, c_padded=padded_call, b_per_length=per_length)
    for k, fn in variants.items():                            # warm-up: code objects, workspaces, GEMM plans
        for _ in range(1 if k == "b_per_length" else 2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for r in range(rounds):
        for k, fn in variants.items():
            if k == "b_per_length" and r >= 2:
                continue
            for _ in range(1 if k.startswith("b_") else reps):
                times[k].append(timed(fn)[0])
    a = ragged().cpu().numpy()
    dev = 0.0
    for outs in (per_length_kept(), per_length()):
        for T, o in outs.items():
            dev = max(dev, float(np.abs(o.cpu().numpy() - a[groups[T]]).max()))
    pad_err = float(np.abs(padded_call().cpu().numpy() - a).max())
    layers = 3 if name == "spherespeaker" else 2
    res = dict(model=name, utterances=B, frames=int(lengths.sum()), distinct_lengths=len(groups), rows=int(lengths.sum()) + 2 * B,
               walk_launches=dict(a_ragged=layers * int(lengths.max()), b_per_length=layers * int(sum(groups)),
                                  c_padded=layers * int(lengths.max())),
               ms={k: stats(v) for k, v in times.items()}, max_abs_ragged_minus_per_length=dev,
               max_abs_padded_minus_ragged=pad_err)
    del kept, dense_in
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="spherespeaker,bi_gru")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_rnn.py measures on a GPU; none is visible")
    results = []
    for name in args.models.split(","):
        res = bench_model(name, args.rounds, args.reps)
        results.append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
