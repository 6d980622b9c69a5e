"""Train-step and recurrence timings of the recurrent models (csrc/rnn.hip, lidbox_amd.models.rnn), in one run.

  * ap_lstm (H = 62, resident form) with the angular-proximity loss at B = 256 and 2048, T = 198, C = 40;
  * lstm (num_units = 1024, stepped form) with sparse cross-entropy at B = 256;
  * the forward and backward recurrence launches alone (lidbox_lstm_fwd / _bwd of ap_lstm's first BLSTM);
  * torch-CPU nn.LSTM on 16 threads (forward + backward of the same BLSTM stack at B = 256), as context.
Device times are HIP events around REPS replays of the captured Trainer step (or REPS calls) after a warm-up.
usage: python tools/bench_rnn.py [--json]"""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.losses import SparseAngularProximity
from lidbox_amd.models import ap_lstm, lstm
from lidbox_amd.train import Trainer

REPS = 10
T, C = 198, 40


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


def step_ms(model, loss, B, N):
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, N, B).astype(np.int32)).cuda()
    tr = Trainer(model, loss=loss)
    return events_ms(lambda: tr.train_step(x, y))


def recurrence_ms(B, H=62):
    m = ap_lstm.create((T, C), num_lstm_units=H, seed=0)
    ws = m.workspace(B, T)
    rng = np.random.default_rng(1)
    ws.zg[0].copy_(torch.from_numpy(rng.standard_normal(tuple(ws.zg[0].shape)).astype(np.float32)))
    ws.dseq[0].copy_(torch.from_numpy(rng.standard_normal(tuple(ws.dseq[0].shape)).astype(np.float32)))
    zg0 = ws.zg[0].clone()
    l = m.lstms[0]
    U0, U1 = (m._p(p + ".U") for p in l.prefixes)
    st = nv.current_stream()

    def fwd():
        nv.check(nv.lib.lidbox_lstm_fwd(U0, U1, 2, B, T, H, nv.ptr(ws.zg[0]), nv.ptr(ws.hseq[0]), nv.ptr(ws.cseq[0]),
                                        nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))

    def bwd():
        nv.check(nv.lib.lidbox_lstm_bwd(U0, U1, 2, B, T, H, nv.ptr(ws.zg[0]), nv.ptr(ws.cseq[0]), nv.ptr(ws.dseq[0]),
                                        T * 2 * H, None, nv.ptr(ws.lstm_ws), ws.lstm_ws.numel(), st))
    f = events_ms(lambda: (ws.zg[0].copy_(zg0), fwd())) - events_ms(lambda: ws.zg[0].copy_(zg0))
    fwd()
    b = events_ms(bwd)                      # dZ overwrites the gate activations: timing only, the values are not used
    return f, b


def torch_cpu_ms(B, H=62, threads=16):
    torch.set_num_threads(min(threads, os.cpu_count() or 1))
    m1 = torch.nn.LSTM(C, H, batch_first=True, bidirectional=True)
    m2 = torch.nn.LSTM(2 * H, H, batch_first=True, bidirectional=True)
    x = torch.randn(B, T, C)
    def run():
        y1, _ = m1(x)
        y2, _ = m2(y1)
        (y1.mean() + y2.mean()).backward()
    run()
    t0 = time.perf_counter()
    for _ in range(3):
        run()
    return (time.perf_counter() - t0) / 3 * 1e3


def main():
    torch.cuda.set_device(0)
    res = {"T": T, "C": C}
    for B in (256, 2048):
        ms = step_ms(ap_lstm.create((T, C), seed=0), SparseAngularProximity(N=4, D=248), B, 4)
        res["ap_lstm_step_B%d" % B] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    ms = step_ms(lstm.create((T, C), 10, num_units=1024, seed=0), "sparse_categorical_crossentropy", 256, 10)
    res["lstm1024_step_B256"] = {"ms": round(ms, 3), "utt_per_s": round(256 / ms * 1e3, 1),
                                 "resident": bool(nv.lib.lidbox_lstm_resident_ok(1024))}
    for B in (256, 2048):
        f, b = recurrence_ms(B)
        res["recurrence_H62_bidir_B%d" % B] = {"fwd_ms": round(f, 3), "bwd_ms": round(b, 3)}
    ms = torch_cpu_ms(256)
    res["torch_cpu_ap_lstm_fwd_bwd_B256"] = {"ms": round(ms, 1), "threads": min(16, os.cpu_count() or 1)}
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-34s %s" % (k, v))


if __name__ == "__main__":
    main()
