"""
What tests/test_ragged_mla_train_cpu.py and tests/test_ragged_mla_train_gpu.py share (no test in here): float64 torch-autograd
restatements of the TRAINING computation of multilevel_attention (reference lidbox/models/multilevel_attention.py:21-85), and
the inputs of the model cases of tests/ragged_mla_cases.py.

  ragged64   the concatenated frames [total_T, D]: per level Dense on every frame, BatchNormalization with batch mean and
             population variance over ALL real frames (eps 1e-3), ReLU, Dropout with the applied factors as data, Dense(K),
             and the attention pooling softmax -> clip -> renormalise over time -> sigmoid-weighted sum PER UTTERANCE;
             Concatenate, Dense.
  dense64    the same on a dense batch [B, T, D], written on the 3-D tensor (statistics over the B T rows, sums over axis 1):
             what a zero-padded batch computes, and at equal lengths what ragged64 computes.

Both return (logits [B, K], {bn name: (batch mean, population variance)}, {`dense_block{l}_fc.b`: the Dense output the bias is
added to}, [softmax probabilities of every level]).
"""
import numpy as np
import torch

import ragged_mla_cases as rc

G_TOL = 1e-4                     # tests/test_multilevel_attention_gpu.py: relative L2 on every parameter gradient
H_TOL = rc.H_TOL
LO, HI = rc.LO, rc.HI
EQ_B, EQ_T = 4, 33               # the equal-length case


def params64(weights):
    return {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in weights.items()}


def _levels(p, L, y, stat_rows, pool, masks):
    stats, pre_bn, probs, atts = {}, {}, [], []
    for l in range(1, L + 1):
        a = y @ p["dense_block%d_fc.W" % l] + p["dense_block%d_fc.b" % l]
        a.retain_grad()
        pre_bn["dense_block%d_fc.b" % l] = a
        name = "dense_block%d_bn" % l
        flat = stat_rows(a)
        mean, var = flat.mean(0), flat.var(0, unbiased=False)
        stats[name] = (mean.detach().numpy(), var.detach().numpy())
        y = torch.relu((a - mean) / torch.sqrt(var + rc.BN_EPS) * p[name + ".gamma"] + p[name + ".beta"])
        if masks is not None:
            y = y * torch.from_numpy(np.asarray(masks[l - 1], np.float64)).reshape(y.shape)
        z = y @ p["attention%d_input.W" % l] + p["attention%d_input.b" % l]
        prob = torch.softmax(z, -1)
        probs.append(prob.detach().numpy())
        atts.append(pool(torch.clamp(prob, LO, HI), torch.sigmoid(z)))
    return torch.cat(atts, 1) @ p["outputs.W"] + p["outputs.b"], stats, pre_bn, probs


def ragged64(p, L, xcat, ro, masks=None):
    """masks: per level the applied dropout factors [total_T, H] (row = the row in the concatenation), or None"""
    def pool(c, v):
        return torch.stack([(c[a:b] * v[a:b]).sum(0) / c[a:b].sum(0) for a, b in zip(ro[:-1], ro[1:])])
    return _levels(p, L, torch.from_numpy(np.asarray(xcat, np.float64)), lambda a: a, pool, masks)


def dense64(p, L, x, masks=None):
    """masks: per level [B T, H] (row b T + t), or None"""
    def pool(c, v):
        return ((c / c.sum(1, keepdim=True)) * v).sum(1)
    return _levels(p, L, torch.from_numpy(np.asarray(x, np.float64)), lambda a: a.reshape(-1, a.shape[-1]), pool, masks)


def mean_nll(logits, labels):
    return torch.nn.functional.cross_entropy(logits, torch.from_numpy(np.asarray(labels, np.int64)))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def gradient_errors(got, p, pre_bn):
    """relative L2 error of every parameter gradient in `got` (name -> array) against the leaves' .grad.  A `dense_block{l}_fc`
    bias is added in front of a training-mode BatchNormalization, which subtracts the batch mean again: its exact gradient is
    zero, a column sum of a gradient whose columns cancel, and float64 returns its own rounding noise for it.  For these
    biases the scale is the norm of the same column sums without the cancellation (the rule of
    tests/test_multilevel_attention_gpu.py)."""
    errs = {}
    for n, g in got.items():
        ref = p[n].grad.numpy()
        if n in pre_bn:
            da = pre_bn[n].grad.numpy()
            scale = np.linalg.norm(np.abs(da).reshape(-1, da.shape[-1]).sum(0))
            errs[n] = float(np.linalg.norm(np.asarray(g, np.float64) - ref) / max(scale, 1e-30))
        else:
            errs[n] = rel(g, ref)
    return errs


def away_from_the_clip_bounds(probs):
    """float64: no softmax probability is clipped or lies in the band around a bound (oracle/update_paths_np.near_clip_bound)"""
    from oracle import update_paths_np as up
    return all((q > LO).all() and (q < HI).all() and not up.near_clip_bound(q).any() for q in probs)


def trainable(w):
    return {k: v for k, v in w.items() if ".moving_" not in k}


def labels_for(B, K, seed=7):
    return np.random.default_rng([seed, B, K]).integers(0, K, B).astype(np.int32)


def equal_inputs(D, seed=8):
    """[EQ_B, EQ_T, D] float32"""
    return np.random.default_rng([seed, D]).standard_normal((EQ_B, EQ_T, D)).astype(np.float32)


def offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def padded_batch(xs):
    T = max(len(x) for x in xs)
    return np.stack([rc.zero_padded(x, T) for x in xs])
