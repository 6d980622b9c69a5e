"""
What tests/test_ragged_mla_cpu.py and tests/test_ragged_mla_gpu.py share (no test in here): the kernel cases with their length
lists, the two model cases with random weights, and a float64 numpy transcription of the model's inference pass on ONE
utterance (reference lidbox/models/multilevel_attention.py:21-85).

Model cases: random kernels, all biases non-zero, gamma / beta off 1 / 0 and RANDOM moving statistics, so the
BatchNormalization is not the identity and a zero frame does not come out of a block as a zero row.
"""
import numpy as np

from oracle import update_paths_np as up

H_TOL = 5e-5                     # tests/test_multilevel_attention_gpu.py: the bound the dense model is held to
LO, HI = up.LO, up.HI
BN_EPS = 1e-3

# ---------------------------------------------------------------------------------------------------- kernel cases
# K -> whether z starts 4 bytes off a 16-byte boundary.  260 and 255 are there for <4,2> and <1,4>, which the other values miss.
KERNEL_KS = [(1, 0), (3, 0), (5, 0), (8, 0), (100, 0), (127, 0), (516, 0), (1023, 0), (260, 0), (255, 0), (128, 1), (512, 1)]
ALL_PAIRS = {(4, 1), (4, 2), (4, 4), (1, 1), (1, 2), (1, 4), (1, 8), (1, 16)}


def kernel_plan(K, shift):
    """mla_plan of the call (the ragged and the dense one choose alike): vec4 = K % 4 == 0 and an aligned base"""
    return up.mla_fwd_plan(1, K, K % 4 == 0 and not shift)


def kernel_lengths(K, shift=0):
    """lengths that bracket one pass P = nw * 64 / G of the row loop: 1, 2, P - 1, P, P + 1, 2 P + 1 and, at K = 100, the
    longest utterance of the model cases; shuffled with a fixed seed"""
    P = kernel_plan(K, shift)["pass_rows"]
    L = sorted({1, 2, max(P - 1, 1), P, P + 1, 2 * P + 1} | ({298} if K == 100 else set()))
    np.random.default_rng(K).shuffle(L)
    return [int(t) for t in L]


def kernel_inputs(K, shift=0, seed=29):
    """(z [total_T, K] float32, row_offsets int64 [B + 1]): tests/test_mla_ops_gpu.py's logits (N(0, 1), two entries at -30 in
    every third row and one at +30 in every fifth: probabilities clipped on both sides, none near a bound)"""
    lengths = kernel_lengths(K, shift)
    ro = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    z, _ = up.mla_inputs(1, int(ro[-1]), K, seed)
    return z.reshape(int(ro[-1]), K), ro


# ---------------------------------------------------------------------------------------------------- model cases
MODEL_CASES = {"k5": dict(D=8, K=5, H=24, L=2), "k100": dict(D=8, K=100, H=64, L=3)}
MODEL_LENGTHS = (1, 2, 31, 32, 33, 64, 127, 128, 129, 298)


def model_weights(D, K, H, L, seed=5):
    """name -> float32 array in the model's layout names"""
    rng = np.random.default_rng([seed, D, K, H, L])
    w = {}

    def glorot(i, o):
        lim = np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o))

    def bias(n):
        b = 0.2 * rng.standard_normal(n)
        return b + np.where(b >= 0, 0.05, -0.05)          # no bias within 0.05 of zero

    cin = D
    for l in range(1, L + 1):
        w["dense_block%d_fc.W" % l], w["dense_block%d_fc.b" % l] = glorot(cin, H), bias(H)
        w["dense_block%d_bn.gamma" % l], w["dense_block%d_bn.beta" % l] = 1.0 + 0.1 * rng.standard_normal(H), bias(H)
        w["dense_block%d_bn.moving_mean" % l] = 0.3 * rng.standard_normal(H)
        w["dense_block%d_bn.moving_variance" % l] = rng.uniform(0.5, 1.5, H)
        w["attention%d_input.W" % l], w["attention%d_input.b" % l] = glorot(H, K), bias(K)
        cin = H
    w["outputs.W"], w["outputs.b"] = glorot(L * K, K), bias(K)
    return {k: v.astype(np.float32) for k, v in w.items()}


def model_inputs(D, seed=6):
    """the utterances [T_b, D] of MODEL_LENGTHS, float32"""
    rng = np.random.default_rng([seed, D])
    return [rng.standard_normal((T, D)).astype(np.float32) for T in MODEL_LENGTHS]


def forward64(w, x, L):
    """float64 inference pass on ONE utterance x [T, D]: (log-probabilities [K], concatenated attention outputs [L K])"""
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    y = np.asarray(x, np.float64)
    atts = []
    for l in range(1, L + 1):
        a = y @ w["dense_block%d_fc.W" % l] + w["dense_block%d_fc.b" % l]
        bn = "dense_block%d_bn" % l
        y = (a - w[bn + ".moving_mean"]) / np.sqrt(w[bn + ".moving_variance"] + BN_EPS) * w[bn + ".gamma"] + w[bn + ".beta"]
        y = np.maximum(y, 0.0)
        z = y @ w["attention%d_input.W" % l] + w["attention%d_input.b" % l]
        e = np.exp(z - z.max(-1, keepdims=True))
        c = np.clip(e / e.sum(-1, keepdims=True), LO, HI)
        atts.append((c * (1.0 / (1.0 + np.exp(-z)))).sum(0) / c.sum(0))
    emb = np.concatenate(atts)
    logits = emb @ w["outputs.W"] + w["outputs.b"]
    m = logits.max()
    return logits - m - np.log(np.exp(logits - m).sum()), emb


def zero_padded(x, T):
    """x [T_b, D] with zero frames behind it, [T, D]: what a padded dense batch holds for this utterance"""
    out = np.zeros((T, x.shape[1]), x.dtype)
    out[:len(x)] = x
    return out


_REF = {}


def model_reference(case):
    """(weights, utterances, float64 log-probabilities [B, K], float64 embeddings [B, L K]) of a model case, computed once"""
    if case not in _REF:
        c = MODEL_CASES[case]
        w, xs = model_weights(**c), model_inputs(c["D"])
        outs = [forward64(w, x, c["L"]) for x in xs]
        out, emb = np.stack([o for o, _ in outs]), np.stack([e for _, e in outs])
        out.setflags(write=False)
        emb.setflags(write=False)
        _REF[case] = (w, xs, out, emb)
    return _REF[case]
