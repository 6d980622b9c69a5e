"""Train-step and convolution timings of the crnn model (csrc/conv2d.hip, lidbox_amd.models.conv_rnn), in one run.

  * crnn (five Conv2D / BatchNormalization / MaxPool2D blocks, BLSTM(256), Dense) with SparseCategoricalCrossentropy
    (from_logits=False) at B = 256, T = 198, F = 40, N = 10: the captured Trainer step;
  * each block's Conv2D forward, dgrad (not block 1: its input is the model input) and wgrad (with the bias gradient) alone,
    with the FLOP count from shapes (2 * pixels * k^2 * C_in * C_out per pass) and the share of the 157.3 TFLOP/s fp32 MFMA
    peak.
Device times are HIP events around REPS replays of the captured Trainer step (or REPS calls) after a warm-up.
usage: python tools/bench_crnn.py [--json]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.models import crnn
from lidbox_amd.models.conv_rnn import pooled_sizes
from lidbox_amd.train import Trainer

REPS = 10
B, T, F, N = 256, 198, 40, 10
PEAK_TFLOPS = 157.3


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


def step_ms():
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, F)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    tr = Trainer(crnn.create((T, F), N, seed=0), loss="sparse_categorical_crossentropy_probs")
    return events_ms(lambda: tr.train_step(x, y))


def conv_layers():
    out = {}
    st = nv.current_stream()
    rng = np.random.default_rng(1)
    cin = 1
    for i, ((Tl, Fl), f, k) in enumerate(zip(pooled_sizes(T, F, 5), crnn.FILTERS, crnn.KERNELS), start=1):
        x = torch.from_numpy(rng.standard_normal((B, Tl, Fl, cin)).astype(np.float32)).cuda()
        W = torch.from_numpy((rng.standard_normal((k, k, cin, f)) * 0.05).astype(np.float32)).cuda()
        b = torch.zeros(f, device="cuda")
        y = torch.empty((B, Tl, Fl, f), device="cuda")
        dx = torch.empty_like(x)
        dW, db = torch.empty_like(W), torch.empty_like(b)
        dws = torch.empty(nv.lib.lidbox_conv2d_dgrad_workspace(k, cin, f), dtype=torch.uint8, device="cuda")
        wws = torch.empty(nv.lib.lidbox_conv2d_wgrad_workspace(B, Tl, Fl, cin, f, k), dtype=torch.uint8, device="cuda")
        flop = 2.0 * B * Tl * Fl * k * k * cin * f
        res = {"k": k, "C_in": cin, "C_out": f, "pixels": B * Tl * Fl, "GFLOP_per_pass": round(flop / 1e9, 2)}

        def fwd():
            nv.check(nv.lib.lidbox_conv2d_fwd(nv.ptr(x), B, Tl, Fl, cin, nv.ptr(W), k, f, nv.ptr(b), 1, nv.ptr(y), st))

        def dgrad():
            nv.check(nv.lib.lidbox_conv2d_dgrad(nv.ptr(y), B, Tl, Fl, cin, f, nv.ptr(W), k, nv.ptr(dx), nv.ptr(dws), dws.numel(), st))

        def wgrad():
            nv.check(nv.lib.lidbox_conv2d_wgrad(nv.ptr(x), nv.ptr(y), B, Tl, Fl, cin, f, k, nv.ptr(dW), nv.ptr(db), nv.ptr(wws),
                                                wws.numel(), st))
        for name, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
            if name == "dgrad" and i == 1:
                continue
            ms = events_ms(fn)
            res[name + "_ms"] = round(ms, 4)
            res[name + "_pct_peak"] = round(100.0 * flop / (ms * 1e-3) / (PEAK_TFLOPS * 1e12), 1)
        out["conv_%d" % i] = res
        cin = f
    return out


def main():
    torch.cuda.set_device(0)
    res = {"B": B, "T": T, "F": F, "N": N}
    ms = step_ms()
    res["crnn_step_B%d" % B] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    res.update(conv_layers())
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-16s %s" % (k, v))


if __name__ == "__main__":
    main()
