"""Kernel and train-step timings of the multilevel_attention model (csrc/mla.hip, lidbox_amd.models.multilevel_attention), in one run.

  * the fused BatchNormalization-apply + ReLU + Dropout pass (lidbox_bn_relu_dropout_fwd / _bwd) against the two-call
    compositions it replaces (lidbox_bn_relu_fwd + lidbox_dropout_rows, lidbox_dropout_rows + lidbox_bn_relu_bwd) at
    (R, C) = (50688, 512) and (12672, 512), alternating composed, fused, composed in every round; the two composed series against
    each other give the run-to-run spread;
  * the attention pooling kernels (lidbox_mla_attention_fwd / _bwd) alone at (B, T, K) = (256, 198, 100) and (64, 198, 100):
    time, achieved bytes/s over the algorithmic minimum (forward 4 B T K read + 8 B K written; backward 4 B T K read +
    4 B T K written + 16 B K of small vectors) as a share of 8 TB/s, and the ratio to the same math as torch eager ops on the
    same device, alternating in the same process.  These are back-to-back launches timed with device events, so the launch
    overhead of each call is part of the figure (at the full shape z is 20 MB);
  * the captured Trainer step with sparse cross-entropy at D = 40, L = 2, H = 512.
Device times are HIP events around REPS calls (or replays of the captured step) after a warm-up.  Needs a device.
usage: python tools/bench_multilevel_attention.py [--json] [--step-only B]   (--step-only: just REPS captured steps, for a profiler)"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from lidbox_amd import _native as nv
from lidbox_amd.models import multilevel_attention
from lidbox_amd.models.tdnn import _rows
from lidbox_amd.train import Trainer

REPS = 20
ROUNDS = 5
T, D, K, L, H = 198, 40, 100, 2, 512
BATCHES = (256, 64)
PEAK_BYTES_PER_S = 8e12
LO, HI = float(np.float32(1e-7)), float(np.float32(1 - 1e-7))


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
    x = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, K, B).astype(np.int32)).cuda()
    tr = Trainer(multilevel_attention.create((T, D), K, L=L, H=H, seed=0))
    return events_ms(lambda: tr.train_step(x, y), reps)


def fused_pass_ms(R, C, rate=0.4):
    """{form: (fwd ms, bwd ms)} medians; composed_a / composed_b are the same code measured before and after the fused form"""
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((R, C)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.standard_normal((R, C)).astype(np.float32)).cuda()
    scale = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32)).cuda()
    shift = torch.from_numpy((0.3 * rng.standard_normal(C)).astype(np.float32)).cuda()
    y, g = torch.empty_like(x), torch.empty_like(x)
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    st, lib = nv.current_stream(), nv.lib
    px, ps, ph, py, pg, pdy, pstep = (nv.ptr(t) for t in (x, scale, shift, y, g, dy, step))
    yrows, grows = _rows(y.data_ptr(), 0, C, 1, R), _rows(g.data_ptr(), 0, C, 1, R)

    def fwd(fused):
        if fused:
            nv.check(lib.lidbox_bn_relu_dropout_fwd(px, R, C, ps, ph, rate, 7, pstep, py, st))
        else:
            nv.check(lib.lidbox_bn_relu_fwd(px, R, C, ps, ph, py, st))
            nv.check(lib.lidbox_dropout_rows(yrows, C, rate, 7, pstep, st))

    def bwd(fused):
        # in place on g, as the model runs it; the gradient is not restored between calls (its values do not change the time)
        if fused:
            nv.check(lib.lidbox_bn_relu_dropout_bwd(px, R, C, ps, ph, rate, 7, pstep, pg, pg, st))
        else:
            nv.check(lib.lidbox_dropout_rows(grows, C, rate, 7, pstep, st))
            nv.check(lib.lidbox_bn_relu_bwd(px, R, C, ps, ph, pg, pg, st))

    g.copy_(dy)
    out = {k: ([], []) for k in ("composed_a", "fused", "composed_b")}
    for _ in range(ROUNDS):
        for key, fused in (("composed_a", False), ("fused", True), ("composed_b", False)):
            out[key][0].append(events_ms(lambda: fwd(fused)))
            out[key][1].append(events_ms(lambda: bwd(fused)))
    return {k: (float(np.median(f)), float(np.median(b))) for k, (f, b) in out.items()}


def attention_ms(B):
    """medians of the HIP kernels and of the same math in torch eager ops on the device, alternating"""
    rng = np.random.default_rng(2)
    z = torch.from_numpy(rng.standard_normal((B, T, K)).astype(np.float32)).cuda()
    datt = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).cuda()
    att, colsum, dz = torch.zeros((B, K), device="cuda"), torch.zeros((B, K), device="cuda"), torch.zeros_like(z)
    st, lib = nv.current_stream(), nv.lib

    def hip_fwd():
        nv.check(lib.lidbox_mla_attention_fwd(nv.ptr(z), B, T, K, nv.ptr(att), K, nv.ptr(colsum), st))

    def hip_bwd():
        nv.check(lib.lidbox_mla_attention_bwd(nv.ptr(z), nv.ptr(att), K, nv.ptr(colsum), nv.ptr(datt), K, B, T, K, nv.ptr(dz), st))

    def eager_fwd():
        c = torch.softmax(z, -1).clamp_(LO, HI)
        s = c.sum(1)
        return (c * torch.sigmoid(z)).sum(1) / s, s

    def eager_bwd():
        p = torch.softmax(z, -1)
        v = torch.sigmoid(z)
        c = p.clamp(LO, HI)
        s = c.sum(1, keepdim=True)
        a = (c * v).sum(1, keepdim=True) / s
        gs = (datt.unsqueeze(1) / s)
        dp = torch.where((p >= LO) & (p <= HI), gs * (v - a), torch.zeros_like(p))
        return p * (dp - (dp * p).sum(-1, keepdim=True)) + gs * c * v * (1 - v)

    hip_fwd()
    out = {k: [] for k in ("hip_fwd", "hip_bwd", "eager_fwd", "eager_bwd")}
    for _ in range(ROUNDS):
        for k, fn in (("eager_fwd", eager_fwd), ("hip_fwd", hip_fwd), ("eager_bwd", eager_bwd), ("hip_bwd", hip_bwd)):
            out[k].append(events_ms(fn))
    torch.cuda.synchronize()
    a_ref, _ = eager_fwd()
    assert float((att - a_ref).abs().max()) < 1e-5 and float((dz - eager_bwd()).abs().max()) < 1e-5
    med = {k: float(np.median(v)) for k, v in out.items()}
    spread = {k: float(max(v) - min(v)) for k, v in out.items()}
    fwd_bytes = 4 * B * T * K + 8 * B * K
    bwd_bytes = 8 * B * T * K + 16 * B * K
    res = {}
    for d, nbytes in (("fwd", fwd_bytes), ("bwd", bwd_bytes)):
        ms = med["hip_" + d]
        res[d] = {"ms": round(ms, 4), "spread_ms": round(spread["hip_" + d], 4), "min_bytes": nbytes,
                  "TB_per_s": round(nbytes / ms / 1e9, 3), "share_of_8TBps": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3),
                  "torch_eager_ms": round(med["eager_" + d], 4), "eager_over_hip": round(med["eager_" + d] / ms, 2)}
    return res


def main():
    if not torch.cuda.is_available():
        sys.exit("bench_multilevel_attention: no HIP device")
    torch.cuda.set_device(0)
    if "--step-only" in sys.argv:
        B = int(sys.argv[sys.argv.index("--step-only") + 1])
        print(json.dumps({"B": B, "ms": round(step_ms(B), 3)}))
        return
    res = {"T": T, "D": D, "K": K, "L": L, "H": H}
    for B in BATCHES:
        R = B * T
        w = fused_pass_ms(R, H)
        entry = {}
        for i, d in enumerate(("fwd", "bwd")):
            entry.update({"fused_%s_ms" % d: round(w["fused"][i], 4), "composed_%s_ms" % d: round(w["composed_a"][i], 4),
                          "composed_again_%s_ms" % d: round(w["composed_b"][i], 4),
                          "spread_%s_ms" % d: round(abs(w["composed_a"][i] - w["composed_b"][i]), 4),
                          "fused_%s_TB_per_s" % d: round((8 if d == "fwd" else 12) * R * H / w["fused"][i] / 1e9, 3)})
        res["bn_relu_dropout_R%d_C%d" % (R, H)] = entry
    for B in BATCHES:
        res["attention_B%d" % B] = attention_ms(B)
    for B in BATCHES:
        ms = step_ms(B)
        res["multilevel_attention_step_B%d" % B] = {"ms": round(ms, 3), "utt_per_s": round(B / ms * 1e3, 1)}
    if "--json" in sys.argv:
        print(json.dumps(res))
        return
    for k, v in res.items():
        print("%-38s %s" % (k, v))


if __name__ == "__main__":
    main()
