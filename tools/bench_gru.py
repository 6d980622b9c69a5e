"""Train-step and recurrence timings of the bi_gru model (csrc/gru.hip, lidbox_amd.models.gru_rnn), in one run.

  * bi_gru (two Bidirectional(GRU(512)) layers, BatchNormalization + Dense head) with sparse cross-entropy at B = 256,
    T = 198, C = 40: the captured Trainer step;
  * one BGRU(512) layer's walk through time alone (lidbox_gru_fwd / _bwd of bi_gru's first layer, both directions) at
    B = 256, and its per-step time (the pass divided by T).
Device times are HIP events around REPS replays of the captured Trainer step (or REPS calls) after a warm-up.
usage: python tools/bench_gru.py [--json]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.models import bi_gru
from lidbox_amd.train import Trainer

REPS = 10
T, C, N = 198, 40, 10


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


def step_ms(B):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    tr = Trainer(bi_gru.create((T, C), N, seed=0))
    return events_ms(lambda: tr.train_step(x, y))


def recurrence_ms(B):
    m = bi_gru.create((T, C), N, seed=0)
    ws = m.workspace(B, T)
    rng = np.random.default_rng(1)
    ws.zg[0].copy_(torch.from_numpy(rng.standard_normal(tuple(ws.zg[0].shape)).astype(np.float32)))
    ws.dseq[0].copy_(torch.from_numpy(rng.standard_normal(tuple(ws.dseq[0].shape)).astype(np.float32)))
    zg0 = ws.zg[0].clone()
    l = m.grus[0]
    H = l.units
    U0, U1 = m._U(l)
    b0, b1 = m._b_rec(l.prefixes[0]), m._b_rec(l.prefixes[1])
    st = nv.current_stream()

    def fwd():
        nv.check(nv.lib.lidbox_gru_fwd(U0, U1, b0, b1, 2, B, T, H, nv.ptr(ws.zg[0]), nv.ptr(ws.hseq[0]), nv.ptr(ws.qh[0]),
                                       None, st))

    def bwd():
        nv.check(nv.lib.lidbox_gru_bwd(U0, U1, 2, B, T, H, nv.ptr(ws.zg[0]), nv.ptr(ws.hseq[0]), nv.ptr(ws.qh[0]),
                                       nv.ptr(ws.dseq[0]), T * 2 * H, None, nv.ptr(ws.gru_ws), ws.gru_ws.numel(), st))
    f = events_ms(lambda: (ws.zg[0].copy_(zg0), fwd())) - events_ms(lambda: ws.zg[0].copy_(zg0))
    fwd()
    b = events_ms(bwd)                      # dZx overwrites the gate activations: timing only, the values are not used
    return f, b


def main():
    torch.cuda.set_device(0)
    res = {"T": T, "C": C}
    B = 256
    ms = step_ms(B)
    res["bi_gru_step_B%d" % B] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    f, b = recurrence_ms(B)
    res["recurrence_H512_bidir_B%d" % B] = {"fwd_ms": round(f, 3), "bwd_ms": round(b, 3),
                                            "fwd_us_per_step": round(f / T * 1e3, 2), "bwd_us_per_step": round(b / T * 1e3, 2)}
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-34s %s" % (k, v))


if __name__ == "__main__":
    main()
