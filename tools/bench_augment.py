"""Throughput of the augmentation kernels (csrc/augment.hip) against scipy on the host, in one run.
A ragged batch of B utterances of 2-4 s at 16 kHz; speed change at ratios drawn from [0.9, 1.1] (as
data.steps.random_signal_speed_change draws them) and FIR filtering with K = 10 taps.  Device times come from
events around REPS calls of the signal_ops wrappers after one warm-up call; the host reference runs the same
work through scipy.signal.resample / lfilter on at most 16 threads.
usage: python tools/bench_augment.py [B] [--json]"""
import concurrent.futures
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.signal
import torch
from lidbox_amd.data import steps
from lidbox_amd.features import signal_ops as sg

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(ARGS[0]) if ARGS else 256
REPS = 10
SR = 16000
HOST_THREADS = min(16, os.cpu_count() or 1)


def device_us(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


def host_us(fn, items):
    with concurrent.futures.ThreadPoolExecutor(HOST_THREADS) as ex:
        list(ex.map(fn, items[:HOST_THREADS]))                     # warm-up
        t0 = time.perf_counter()
        list(ex.map(fn, items))
        return (time.perf_counter() - t0) * 1e6


def main():
    rng = np.random.default_rng(0)
    lengths = rng.integers(2 * SR, 4 * SR + 1, B)
    xs = [rng.standard_normal(int(n)).astype(np.float32) * 0.1 for n in lengths]
    r = sg.RaggedSignals.from_list([torch.from_numpy(x) for x in xs])
    draw = np.random.default_rng(1)
    m = [sg.resample_length(n, steps.speed_change_rate(draw, SR, 0.9, 1.1), SR) for n in lengths]
    coefs = draw.standard_normal((B, 10), dtype=np.float32)
    coefs_d = torch.from_numpy(coefs).cuda()
    n_in, n_out = int(lengths.sum()), int(sum(m))

    res = {}
    us = device_us(lambda: sg.resample(r, m))
    host = host_us(lambda i: scipy.signal.resample(xs[i], m[i]).astype(np.float32), list(range(B)))
    res["speed_change"] = dict(device_us=us, utt_per_s=B / us * 1e6, algorithmic_GBps=(n_in + n_out) * 4 / us / 1e3,
                               host_us=host, host_utt_per_s=B / host * 1e6, speedup_vs_host=host / us)
    us = device_us(lambda: sg.fir_filter(r, coefs_d))
    host = host_us(lambda i: scipy.signal.lfilter(coefs[i], 1.0, xs[i]).astype(np.float32), list(range(B)))
    gbps = 2 * n_in * 4 / us / 1e3
    res["fir_k10"] = dict(device_us=us, utt_per_s=B / us * 1e6, algorithmic_GBps=gbps, share_of_8TBps=gbps / 8000,
                          host_us=host, host_utt_per_s=B / host * 1e6, speedup_vs_host=host / us)
    res["batch"] = dict(utterances=B, seconds=n_in / SR, host_threads=HOST_THREADS,
                        gate_speed_change_20x_host=res["speed_change"]["speedup_vs_host"] >= 20)
    if "--json" in sys.argv:
        print(json.dumps(res))
    else:
        for k, v in res.items():
            print(k, " ".join("%s=%.4g" % (a, b) if isinstance(b, float) else "%s=%s" % (a, b) for a, b in v.items()))


if __name__ == "__main__":
    main()
