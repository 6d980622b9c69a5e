"""Recurrence and train-step timings of the spherespeaker model (csrc/lstm_step.hip, lidbox_amd.models.spherespeaker), in one run.

  * one Bidirectional(LSTM(250)) layer's walk through time alone at T = 198, B in {64, 256}, forward and backward: the fused
    step (lidbox_lstm_step_fwd / _bwd) against the stepped form (lidbox_lstm_fwd / _bwd: one GEMM per step and direction plus
    a cell kernel), alternating stepped, fused, stepped in every round; the two stepped series against each other give the
    run-to-run spread;
  * spherespeaker (three such layers, BatchNormalization, Dense(1000), pooling head) with sparse cross-entropy at C = 40: the
    captured Trainer step;
  * torch-CPU nn.LSTM (3 layers, bidirectional, 250 units) forward + backward of the same stack on 16 threads, as context.
Device times are HIP events around REPS calls (or replays of the captured step) after a warm-up.
usage: python tools/bench_spherespeaker.py [--json] [--step-only B]   (--step-only: just REPS captured steps, for a profiler)"""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.models import spherespeaker
from lidbox_amd.train import Trainer

REPS = 10
ROUNDS = 3
T, C, N, H = 198, 40, 10, 250
BATCHES = (64, 256)


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


def step_ms(B, reps=REPS):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    tr = Trainer(spherespeaker.create((T, C), N, seed=0))
    return events_ms(lambda: tr.train_step(x, y), reps)


def walk_ms(B):
    """{form: (fwd ms, bwd ms)} of one BLSTM(250) layer's walk; stepped_a / stepped_b are the same code measured before
    and after the fused form in every round"""
    dev = torch.device("cuda")
    f32 = dict(dtype=torch.float32, device=dev)
    rng = np.random.default_rng(1)
    m = spherespeaker.create((T, C), N, seed=0)
    U0, U1 = m._p("blstm_2_forward.U"), m._p("blstm_2_backward.U")
    zg_in = torch.from_numpy((rng.standard_normal((2, B, T, 4 * H)) * 0.5).astype(np.float32)).to(dev)
    zg = torch.zeros_like(zg_in)
    acts = torch.zeros_like(zg_in)
    hseq = torch.zeros((B, T + 2, 2 * H), **f32)
    cseq = torch.zeros((2, B, T, H), **f32)
    dseq = torch.from_numpy(rng.standard_normal((B, T, 2 * H)).astype(np.float32)).to(dev)
    ws_n = max(16, nv.lib.lidbox_lstm_workspace(B, T, H, 2), nv.lib.lidbox_lstm_step_workspace(B, T, H, 2))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
    st = nv.current_stream()

    def fwd(fused):
        if fused:
            nv.check(nv.lib.lidbox_lstm_step_fwd(U0, U1, 2, B, T, H, nv.ptr(zg), nv.ptr(hseq), 2 * H, nv.ptr(cseq), nv.ptr(ws), ws_n, st))
        else:
            nv.check(nv.lib.lidbox_lstm_fwd(U0, U1, 2, B, T, H, nv.ptr(zg), nv.ptr(hseq), nv.ptr(cseq), nv.ptr(ws), ws_n, st))

    def bwd(fused):
        if fused:
            nv.check(nv.lib.lidbox_lstm_step_bwd(U0, U1, 2, B, T, H, nv.ptr(zg), nv.ptr(cseq), nv.ptr(dseq), T * 2 * H, 2 * H, None,
                                                 nv.ptr(ws), ws_n, st))
        else:
            nv.check(nv.lib.lidbox_lstm_bwd(U0, U1, 2, B, T, H, nv.ptr(zg), nv.ptr(cseq), nv.ptr(dseq), T * 2 * H, None,
                                            nv.ptr(ws), ws_n, st))

    # both passes overwrite zg: every timed call restores it first, and the copy's own time is taken off
    copy = min(events_ms(lambda: zg.copy_(zg_in)) for _ in range(ROUNDS))
    zg.copy_(zg_in)
    fwd(True)
    acts.copy_(zg)
    out = {k: ([], []) for k in ("stepped_a", "fused", "stepped_b")}
    for _ in range(ROUNDS):
        for key, fused in (("stepped_a", False), ("fused", True), ("stepped_b", False)):
            out[key][0].append(events_ms(lambda: (zg.copy_(zg_in), fwd(fused))) - copy)
            out[key][1].append(events_ms(lambda: (zg.copy_(acts), bwd(fused))) - copy)
    return {k: (float(np.median(f)), float(np.median(b))) for k, (f, b) in out.items()}


def cpu_lstm_ms(B, reps=2):
    torch.set_num_threads(16)
    m = torch.nn.LSTM(C, H, num_layers=3, batch_first=True, bidirectional=True)
    x = torch.randn(B, T, C)
    best = float("inf")
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        y, _ = m(x)
        y.sum().backward()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    torch.cuda.set_device(0)
    if "--step-only" in sys.argv:
        B = int(sys.argv[sys.argv.index("--step-only") + 1])
        print(json.dumps({"B": B, "ms": round(step_ms(B), 3)}))
        return
    res = {"T": T, "C": C, "H": H}
    for B in BATCHES:
        w = walk_ms(B)
        sf = [w["stepped_a"][i] for i in (0, 1)]
        spread = [abs(w["stepped_a"][i] - w["stepped_b"][i]) for i in (0, 1)]
        res["walk_B%d" % B] = {
            "fused_fwd_ms": round(w["fused"][0], 3), "fused_bwd_ms": round(w["fused"][1], 3),
            "stepped_fwd_ms": round(sf[0], 3), "stepped_bwd_ms": round(sf[1], 3),
            "stepped_again_fwd_ms": round(w["stepped_b"][0], 3), "stepped_again_bwd_ms": round(w["stepped_b"][1], 3),
            "spread_fwd_ms": round(spread[0], 3), "spread_bwd_ms": round(spread[1], 3),
            "fused_fwd_us_per_step": round(w["fused"][0] / T * 1e3, 2), "fused_bwd_us_per_step": round(w["fused"][1] / T * 1e3, 2),
            "stepped_fwd_us_per_step": round(sf[0] / T * 1e3, 2), "stepped_bwd_us_per_step": round(sf[1] / T * 1e3, 2)}
    for B in BATCHES:
        ms = step_ms(B)
        res["spherespeaker_step_B%d" % B] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    for B in BATCHES:
        res["torch_cpu_lstm_stack_fwd_bwd_B%d" % B] = {"ms": round(cpu_lstm_ms(B), 1), "threads": 16}
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-38s %s" % (k, v))


if __name__ == "__main__":
    main()
