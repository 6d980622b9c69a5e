"""
Timing of the ragged train step of multilevel_attention (docs/LAB_NOTEBOOK.md section 33) on one GPU:

    python tools/bench_ragged_mla_train.py [--rounds 6] [--reps 3] [--out result.json]

Workload: tools/bench_ragged_mla.py's (256 utterances of 98 .. 298 frames, 48 772 frames, 144 distinct lengths, seed 2024; 40
features, L = 2, H = 512, K = 100) with the reference's dropout 0.4 and random labels.  HIP events around whole steps, every
variant warmed up first (for the captured ones: built and replayed), the variants alternating round by round:
    (a)  one Trainer.train_step_ragged over all utterances (eager);
    (b)  the only correct route without it: one captured dense step per distinct length, all 144 workspaces and graphs kept by
         the caller.  A different optimisation (144 small steps, 144 sets of batch statistics), compared on time per utterance;
    (c)  one captured dense step on the batch zero-padded to 298 frames: wrong gradients, a cost yardstick only.
Each variant trains a model of its own from the same initial weights.
Then the kernel pair on logits [rows, K]: lidbox_mla_attention_bwd at B = 256, T = 190 against lidbox_mla_attention_ragged_bwd
on the same 48 640 rows cut into 256 utterances of 190 frames, and the ragged kernel on the workload's own lengths; a kernel
measurement is 20 launches between one pair of events, divided by 20.
Reported: median (min .. max) in ms per variant.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_ragged_mla import B, C, K, LEVELS, SEED, UNITS, stats, timed, workload      # noqa: E402

DROPOUT = 0.4


def bench_steps(rounds, reps):
    from lidbox_amd.models import multilevel_attention
    from lidbox_amd.train import Trainer
    lengths, xs = workload()
    labels = np.random.default_rng(SEED + 3).integers(0, K, B).astype(np.int32)
    off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    X = torch.from_numpy(np.concatenate(xs)).cuda()
    y = torch.from_numpy(labels).cuda()
    groups = {int(T): np.flatnonzero(lengths == T) for T in sorted(set(lengths.tolist()))}

    def model():
        return multilevel_attention.create((None, C), K, L=LEVELS, H=UNITS, seed=1, dropout_rate=DROPOUT)

    # (a)
    tr_a = Trainer(model(), use_graph=False)

    def ragged():
        return tr_a.train_step_ragged(X, off, y)

    # (b): the entries of Trainer.train_step's own cache, built the same way but all kept
    tr_b = Trainer(model(), use_graph=True)
    entries = {}
    for T, idx in groups.items():
        x_T = torch.from_numpy(np.stack([xs[i] for i in idx])).cuda()
        y_T = torch.from_numpy(labels[idx]).cuda()
        tr_b._step_global_batch = tr_b._step_feat = None
        entries[T] = tr_b._build(x_T, y_T)
        assert len(entries[T]["graphs"]) == 1

    def per_length_kept():
        for e in entries.values():
            e["graphs"][0]()

    # (c)
    tr_c = Trainer(model(), use_graph=True)
    padded = torch.zeros((B, int(lengths.max()), C), device="cuda")
    for b, x in enumerate(xs):
        padded[b, :len(x)] = torch.from_numpy(x).cuda()

    def padded_step():
        return tr_c.train_step(padded, y)

    variants = dict(a_ragged_step=ragged, b_per_length_captured=per_length_kept, c_padded_captured=padded_step)
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            for _ in range(1 if k.startswith("b_") else reps):
                times[k].append(timed(fn)[0])
    finite = bool(all(torch.isfinite(t.model.flat).all() for t in (tr_a, tr_b, tr_c)))
    res = dict(model="multilevel_attention", utterances=B, frames=int(lengths.sum()), distinct_lengths=len(groups),
               padded_frames=B * int(lengths.max()), dropout=DROPOUT, ms={k: stats(v) for k, v in times.items()},
               steps_taken=dict(a=tr_a.step_count, b=tr_b.step_count, c=tr_c.step_count), weights_finite=finite)
    res["us_per_utterance"] = {k: 1e3 * v["median"] / B for k, v in res["ms"].items()}
    del entries, padded
    torch.cuda.empty_cache()
    return res


def bench_kernel_pair(rounds, reps):
    """the backward pooling alone: the dense kernel, the ragged kernel on the same rows in equal utterances, and the ragged
    kernel on the workload's lengths; att and colsum are the forward's"""
    from lidbox_amd import _native as nv
    lengths, _ = workload()
    T = int(lengths.sum()) // B
    rows_eq, rows_wl = B * T, int(lengths.sum())
    st, lib = nv.current_stream(), nv.lib
    g = torch.Generator(device="cuda").manual_seed(SEED)
    z = torch.randn((max(rows_eq, rows_wl), K), device="cuda", generator=g)
    datt = torch.randn((B, LEVELS * K), device="cuda", generator=g)
    dz = torch.empty_like(z)
    off_eq = torch.arange(B + 1, dtype=torch.int64, device="cuda") * T
    off_wl = torch.from_numpy(np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)).cuda()
    fwd = {}
    for name, off in (("eq", off_eq), ("wl", off_wl)):
        att, colsum = torch.empty((B, LEVELS * K), device="cuda"), torch.empty((B, K), device="cuda")
        nv.check(lib.lidbox_mla_attention_ragged_fwd(nv.ptr(z), nv.ptr(off), B, K, nv.ptr(att), LEVELS * K, nv.ptr(colsum), st))
        fwd[name] = (att, colsum)
    max_wl = int(lengths.max())

    def dense():
        att, colsum = fwd["eq"]
        nv.check(lib.lidbox_mla_attention_bwd(nv.ptr(z), nv.ptr(att), LEVELS * K, nv.ptr(colsum), nv.ptr(datt), LEVELS * K, B, T, K,
                                              nv.ptr(dz), st))

    def ragged_equal():
        att, colsum = fwd["eq"]
        nv.check(lib.lidbox_mla_attention_ragged_bwd(nv.ptr(z), nv.ptr(off_eq), B, T, K, nv.ptr(att), LEVELS * K, nv.ptr(colsum),
                                                     nv.ptr(datt), LEVELS * K, nv.ptr(dz), st))

    def ragged_workload():
        att, colsum = fwd["wl"]
        nv.check(lib.lidbox_mla_attention_ragged_bwd(nv.ptr(z), nv.ptr(off_wl), B, max_wl, K, nv.ptr(att), LEVELS * K, nv.ptr(colsum),
                                                     nv.ptr(datt), LEVELS * K, nv.ptr(dz), st))

    pair = dict(dense=dense, ragged_equal=ragged_equal, ragged_workload=ragged_workload)
    for fn in pair.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    dense()
    want = dz[:rows_eq].clone()
    ragged_equal()
    same = bool(torch.equal(want.view(torch.int32), dz[:rows_eq].view(torch.int32)))
    times = {n: [] for n in pair}
    inner = 20

    def burst(fn):
        for _ in range(inner):
            fn()

    for _ in range(rounds):
        for n, fn in pair.items():
            for _ in range(reps):
                times[n].append(timed(lambda: burst(fn))[0] / inner)
    return dict(K=K, B=B, T_equal=T, rows_equal=rows_eq, rows_workload=rows_wl, max_T_workload=max_wl,
                ragged_equal_bits_match_dense=same, launches_per_measurement=inner, ms={n: stats(v) for n, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="skip the kernel pair")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged_mla_train.py measures on a GPU; none is visible")
    results = [bench_steps(args.rounds, args.reps)]
    print(json.dumps(results[-1]), flush=True)
    if not args.no_kernels:
        results.append(dict(kernel_pair=bench_kernel_pair(args.rounds, args.reps)))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
