"""Train-step and convolution timings of the clstm model (lidbox_amd.models.clstm, csrc/conv2d.hip's strided Conv2D), in one run.

  * clstm at B = 256, T = 198, F = 40, N = 10 with sparse categorical cross-entropy: the captured Trainer step for the five flag
    rows none / use_conv2d / use_lstm / use_attention / all three;
  * conv2d_1 and conv2d_2 forward, dgrad (conv2d_2 only: conv2d_1's input is the model input) and wgrad alone, with the FLOP
    count of the taps that fall inside the image (2 * B * T * C_in * C_out * kt * sum over output columns of the in-image
    frequency taps) and its share of the 157.3 TFLOP/s fp32 MFMA peak.
Device times are HIP events around REPS replays of the captured Trainer step (or REPS calls) after a warm-up.
usage: python tools/bench_clstm.py [--json]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.models import clstm
from lidbox_amd.train import Trainer

REPS = 10
B, T, F, N = 256, 198, 40, 10
PEAK_TFLOPS = 157.3
ROWS = {"none": {}, "conv2d": dict(use_conv2d=True), "lstm": dict(use_lstm=True), "attention": dict(use_attention=True),
        "all": dict(use_conv2d=True, use_lstm=True, use_attention=True)}


def events_ms(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def step_ms(flags):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    tr = Trainer(clstm.create((T, F), N, seed=0, **flags))
    return events_ms(lambda: tr.train_step(x, y))


def inside_taps(Fi, Fo, taps):
    """frequency taps inside the image, summed over the output columns"""
    return sum(len([j for j in range(taps.kf) if 0 <= fo * taps.sf + j - taps.pf0 < Fi]) for fo in range(Fo))


def conv_layers():
    out = {}
    st = nv.current_stream()
    rng = np.random.default_rng(1)
    cin = 1
    for i, ((Fi, Fo, taps), f) in enumerate(zip(clstm.conv2d_taps(F), clstm.FILTERS), start=1):
        x = torch.from_numpy(rng.standard_normal((B, T, Fi, cin)).astype(np.float32)).cuda()
        W = torch.from_numpy((rng.standard_normal((taps.kt, taps.kf, cin, f)) * 0.05).astype(np.float32)).cuda()
        b = torch.zeros(f, device="cuda")
        y = torch.empty((B, T, Fo, f), device="cuda")
        dx = torch.empty_like(x)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        dws = torch.empty(max(16, nv.lib.lidbox_conv2d_strided_dgrad_workspace(taps, cin, f)), dtype=torch.uint8, device="cuda")
        wws = torch.empty(nv.lib.lidbox_conv2d_strided_wgrad_workspace(B, T, Fi, cin, f, taps), dtype=torch.uint8, device="cuda")
        flop = 2.0 * B * T * cin * f * taps.kt * inside_taps(Fi, Fo, taps)
        res = {"F": "%d->%d" % (Fi, Fo), "C_in": cin, "C_out": f, "GFLOP_per_pass": round(flop / 1e9, 2),
               "GFLOP_with_padding": round(2.0 * B * T * Fo * taps.kt * taps.kf * cin * f / 1e9, 2)}

        def fwd():
            nv.check(nv.lib.lidbox_conv2d_strided_fwd(nv.ptr(x), B, T, Fi, cin, nv.ptr(W), taps, f, nv.ptr(b), nv.ptr(y), st))

        def dgrad():
            nv.check(nv.lib.lidbox_conv2d_strided_dgrad(nv.ptr(y), B, T, Fi, cin, f, nv.ptr(W), taps, nv.ptr(dx), nv.ptr(dws),
                                                        dws.numel(), st))

        def wgrad():
            nv.check(nv.lib.lidbox_conv2d_strided_wgrad(nv.ptr(x), nv.ptr(y), B, T, Fi, cin, f, taps, nv.ptr(dW), nv.ptr(db),
                                                        nv.ptr(wws), wws.numel(), st))
        for name, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
            if name == "dgrad" and i == 1:
                continue
            ms = events_ms(fn)
            res[name + "_ms"] = round(ms, 4)
            res[name + "_pct_peak"] = round(100.0 * flop / (ms * 1e-3) / (PEAK_TFLOPS * 1e12), 1)
        out["conv2d_%d" % i] = res
        cin = f
    return out


def main():
    torch.cuda.set_device(0)
    res = {"B": B, "T": T, "F": F, "N": N}
    for row, flags in ROWS.items():
        ms = step_ms(flags)
        res["clstm_%s_step_B%d" % (row, B)] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    res.update(conv_layers())
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-26s %s" % (k, v))


if __name__ == "__main__":
    main()
