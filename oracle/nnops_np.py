"""
float64 numpy restatement of the reduction kernels every model ends in: the first half of csrc/nnops.hip (stats / average
pooling, softmax, log-softmax, the two cross-entropies, the fused softmax head, l2_normalize), csrc/batchnorm.hip and
csrc/attention.hip, written from the definitions in those files' header comments.  tests/test_oracle_nnops.py pins every
function against float64 torch autograd.

Layouts are the library's: activations [B, T, C] with channels innermost, matrices row-major.

abs sums: every function that sums returns (or has a twin `*_abs` that returns) the same operation on absolute values, the S of
    |got - ref| <= gamma(n) S + n 2^-126            (conv2d_np.error_bound; derivation in tests/test_conv2d_paths_gpu.py)
that holds for an fp32 chain of n additions / fused multiply-adds in any order.

The second half restates the host-side dispatch of the three files (which kernel, which template instantiation, how many
slices, trips and idle groups) as plain functions, so that a CPU test can prove which path a test shape selects, and holds
fp32 emulations of the kernels' summation orders, so that a CPU test can show the derived bounds hold for those orders.
"""
import numpy as np

from oracle import model_np as mo
from oracle.conv2d_np import U, cdiv, error_bound, fma32, gamma       # noqa: F401  (re-exported for the test modules)

STDDEV_CLIP = float(np.float32(1e-10))            # nnops.hip STDDEV_SQRT_MIN_CLIP (the fp32 constant)
STDDEV_CLIPPED_MAX = float(np.float32(1.0000001e-5))   # `sd > 1.0000001e-5f`: a larger stddev was not clipped
KERAS_EPSILON = float(np.float32(1e-7))
L2_EPS = float(np.float32(1e-12))
AP_ACOS_CLAMP = float(np.float32(1e-6))
BN_COLS = 64


def f64(a):
    return np.asarray(a, np.float64)


def bf16_round(a):
    """float32 -> the float32 value of its bfloat16, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ------------------------------------------------------------------------------------------ pooling
def stats_pool_fwd(x):
    """x [B, T, C] -> (mean, var, out): out = [mean | sqrt(clip(var, 1e-10, fmax))] with the two-pass population variance"""
    x = f64(x)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None, :]) ** 2).mean(axis=1)
    sd = np.sqrt(np.clip(var, STDDEV_CLIP, np.finfo(np.float32).max))
    return mean, var, np.concatenate([mean, sd], axis=1)


def avg_pool_fwd(x):
    return f64(x).mean(axis=1)


def pool_mean_abs(x):
    """S of the mean: mean |x|"""
    return np.abs(f64(x)).mean(axis=1)


def stats_pool_bwd(x, pooled, dout, relu_mask=False):
    """dx of stats_pool_fwd from the FORWARD'S OUTPUT `pooled` = [mean | sd] (what the kernels read): dmean / T + dsd (x - mean) /
    (sd T), the second term only where the stddev was not the clipped value; times (x > 0) under the mask"""
    x, pooled, dout = f64(x), f64(pooled), f64(dout)
    B, T, C = x.shape
    mean, sd = pooled[:, :C], pooled[:, C:]
    dvar = np.where(sd > STDDEV_CLIPPED_MAX, dout[:, C:] / (2.0 * sd), 0.0)
    dx = dout[:, None, :C] / T + (2.0 * dvar / T)[:, None, :] * (x - mean[:, None, :])
    return np.where(x > 0, dx, 0.0) if relu_mask else dx


def stats_pool_bwd_abs(x, pooled, dout):
    x, pooled, dout = f64(x), f64(pooled), f64(dout)
    B, T, C = x.shape
    mean, sd = pooled[:, :C], pooled[:, C:]
    dvar = np.where(sd > STDDEV_CLIPPED_MAX, np.abs(dout[:, C:]) / (2.0 * sd), 0.0)
    return np.abs(dout[:, None, :C]) / T + (2.0 * dvar / T)[:, None, :] * (np.abs(x) + np.abs(mean[:, None, :]))


def avg_pool_bwd(x, dout, relu_mask=False):
    x, dout = f64(x), f64(dout)
    dx = np.broadcast_to(dout[:, None, :] / x.shape[1], x.shape)
    return np.where(x > 0, dx, 0.0) if relu_mask else dx.copy()


def pool_chain(T, path):
    """longest chain of roundings behind a pooled mean: the register kernel adds T rows in order; pool_fwd_kernel adds
    ceil(T / 16) rows per time group, then the 16 groups; + 1 for the division by T"""
    return (T if path[0] == "reg" else cdiv(T, 16) + 16) + 1


def stddev_interval(x, T_chain):
    """[lo, hi] that contains the fp32 stddev of any kernel that computes mean (chain T_chain), d = x - mean, sum d d (the same
    chain, one fma each), / T, clip, sqrtf.  With e_m the mean's bound and delta = e_m + u (|d| + e_m) the error of one computed d:
        |sum dhat^2 - sum d^2| <= sum (2 |d| delta + delta^2),     |fl(sum dhat^2) - sum dhat^2| <= gamma(n) sum (|d| + delta)^2
    the interval is sqrt(clip(var -+ e_var)) widened by 2 u for the square root's own rounding."""
    x = f64(x)
    mean, var, _ = stats_pool_fwd(x)
    e_m = error_bound(pool_mean_abs(x), T_chain)
    d = np.abs(x - mean[:, None, :])
    delta = e_m[:, None, :] + U * (d + e_m[:, None, :])
    T = x.shape[1]
    e_var = ((2 * d * delta + delta ** 2).sum(axis=1) + error_bound(((d + delta) ** 2).sum(axis=1), T_chain + 2)) / T
    fmax = np.finfo(np.float32).max
    lo = np.sqrt(np.clip(var - e_var, STDDEV_CLIP, fmax)) * (1 - 2 * U)
    hi = np.sqrt(np.clip(var + e_var, STDDEV_CLIP, fmax)) * (1 + 2 * U)
    return lo, hi


# ------------------------------------------------------------------------------------------ softmax, cross-entropies
def softmax(z):
    return mo.softmax(f64(z))


def log_softmax(z):
    return mo.log_softmax(f64(z))


def nll(logp, y, scale):
    """Keras SparseCategoricalCrossentropy(from_logits=True) on rows that already are log-probabilities:
    loss = mean_b(logsumexp(logp_b) - logp[b, y_b]), dz = (softmax(logp) - onehot) scale.  A label outside [0, N): NaN loss,
    zero gradient row.  -> (loss, dz, per-row losses)"""
    logp = f64(logp)
    y = np.asarray(y)
    B, N = logp.shape
    ok = (y >= 0) & (y < N)
    yc = np.where(ok, y, 0)
    lp2 = mo.log_softmax(logp)
    rows = np.where(ok, -lp2[np.arange(B), yc], np.nan)
    dz = np.exp(lp2)
    dz[np.arange(B), yc] -= 1.0
    dz = np.where(ok[:, None], dz * scale, 0.0)
    return float(rows.mean()), dz, rows


def softmax_nll(z, y, scale, eps=KERAS_EPSILON):
    """Keras SparseCategoricalCrossentropy(from_logits=False) on softmax outputs: q = clip(p, eps, 1 - eps), loss = mean_b(log
    sum_j q_j - log q_y), the gradient through clip (open interval only) and softmax.  -> (probs, loss, dz)"""
    z = f64(z)
    y = np.asarray(y)
    B, N = z.shape
    ok = (y >= 0) & (y < N)
    yc = np.where(ok, y, 0)
    p = mo.softmax(z)
    q = np.clip(p, eps, 1.0 - eps)
    sq = q.sum(axis=1, keepdims=True)
    idx = np.arange(B)
    rows = np.where(ok, np.log(sq[:, 0]) - np.log(q[idx, yc]), np.nan)
    opened = (p > eps) & (p < 1.0 - eps)
    g = np.where(opened, 1.0 / sq, 0.0)
    gy = np.zeros_like(g)
    gy[idx, yc] = 1.0 / q[idx, yc]
    g = g - np.where(opened, gy, 0.0)
    dz = p * (g - (p * g).sum(axis=1, keepdims=True)) * scale
    return p, float(rows.mean()), np.where(ok[:, None], dz, 0.0)


def softmax_head(h, W, bias, y, scale, relu_mask=False):
    """Dense(N) + log_softmax + nll() and all five gradients -> dict(z, S_z, logp, loss, rows, dz, dW, db, dh)"""
    h, W, bias = f64(h), f64(W), f64(bias)
    z = h @ W + bias
    logp = mo.log_softmax(z)
    loss, dz, rows = nll(logp, y, scale)
    dh = dz @ W.T
    return dict(z=z, S_z=np.abs(h) @ np.abs(W) + np.abs(bias), logp=logp, loss=loss, rows=rows, dz=dz, dW=h.T @ dz,
                db=dz.sum(axis=0), dh=np.where(h > 0, dh, 0.0) if relu_mask else dh)


def head_grads_from_dz(h, W, dz, relu_mask=False):
    """the three sums the head takes over dz, for a GIVEN dz (the device's, so that expf's error stays out of the comparison)
    -> (dW, S_dW, db, S_db, dh, S_dh)"""
    h, W, dz = f64(h), f64(W), f64(dz)
    dh, S_dh = dz @ W.T, np.abs(dz) @ np.abs(W).T
    if relu_mask:
        dh = np.where(h > 0, dh, 0.0)
    return h.T @ dz, np.abs(h).T @ np.abs(dz), dz.sum(axis=0), np.abs(dz).sum(axis=0), dh, S_dh


# ------------------------------------------------------------------------------------------ l2_normalize
def l2_normalize(x):
    x = f64(x)
    return x / np.sqrt(np.maximum((x * x).sum(axis=1, keepdims=True), L2_EPS))


def l2_normalize_bwd(x, g):
    """gradient of l2_normalize: g / |x| - x (x . g) / |x|^3; a clipped row (sum x^2 < eps) is x / sqrt(eps): g / sqrt(eps)"""
    x, g = f64(x), f64(g)
    s = (x * x).sum(axis=1, keepdims=True)
    inv = 1.0 / np.sqrt(np.maximum(s, L2_EPS))
    k = np.where(s < L2_EPS, 0.0, (x * g).sum(axis=1, keepdims=True) * inv ** 3)
    return g * inv - x * k


def l2_chain(D):
    """a lane's ceil(D / 64) fused multiply-adds, then wave_sum's six steps"""
    return cdiv(D, 64) + 6


def l2_bounds(x, g=None):
    """error bounds of l2_normalize (g None) or its gradient, propagated through rsqrtf (2 ulp allowed) from the bound of the
    sums: with r = e_s / (2 s) + 2 u the relative error of inv = rsqrt(s),
        |y - yref| <= |y| (r + 2 u)
        |dx - ref| <= |g| inv (r + 2 u) + |x| (e_k + 2 u |k|),   e_k = e_dot inv^3 + |dot| inv^3 (3 r + 4 u)"""
    x = f64(x)
    D = x.shape[1]
    s = (x * x).sum(axis=1, keepdims=True)
    sc = np.maximum(s, L2_EPS)
    inv = 1.0 / np.sqrt(sc)
    r = np.where(s < L2_EPS, 0.0, error_bound(s, l2_chain(D)) / (2 * sc)) + 2 * U
    if g is None:
        return np.abs(x) * inv * (r + 2 * U) + 2.0 ** -126
    g = f64(g)
    dot = (x * g).sum(axis=1, keepdims=True)
    e_dot = error_bound((np.abs(x) * np.abs(g)).sum(axis=1, keepdims=True), l2_chain(D))
    k = np.where(s < L2_EPS, 0.0, np.abs(dot) * inv ** 3)
    e_k = np.where(s < L2_EPS, 0.0, e_dot * inv ** 3 + k * (3 * r + 4 * U))
    return np.abs(g) * inv * (r + 2 * U) + np.abs(x) * (e_k + 2 * U * k) + 2 * U * (np.abs(g) * inv + np.abs(x) * k) + 2.0 ** -126


# ------------------------------------------------------------------------------------------ batch normalisation
def bn_train_stats(x, gamma_, beta, eps, momentum, bessel, moving_mean=None, moving_var=None):
    """x [R, C] -> dict(mean, var, invstd, scale, shift, moving_mean, moving_var): batch mean and POPULATION variance; the moving
    variance moves towards var R / (R - 1) with `bessel` (and R > 1), towards var without"""
    x = f64(x)
    R = x.shape[0]
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = f64(gamma_) * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=f64(beta) - mean * scale, moving_mean=None, moving_var=None)
    if moving_mean is not None:
        target = var * (R / (R - 1.0)) if bessel and R > 1 else var
        out["moving_mean"] = f64(moving_mean) * momentum + mean * (1.0 - momentum)
        out["moving_var"] = f64(moving_var) * momentum + target * (1.0 - momentum)
    return out


def bn_apply(x, scale, shift):
    """fp32, one fused multiply-add per element: what bn_apply_kernel computes, bit for bit"""
    return fma32(x, scale, shift)


def bn_bwd(x, dy, mean, invstd, gamma_, relu_mask=False):
    """backward of y = gamma (x - mean) invstd + beta through the batch statistics, for GIVEN mean / invstd (the forward's):
    dbeta = sum dy, dgamma = sum dy xhat, dx = gamma invstd (dy - dbeta / R - xhat dgamma / R), times (x > 0) under the mask
    -> dict(dgamma, S_dgamma, dbeta, S_dbeta, dx, S_dx)"""
    x, dy, mean, invstd, gamma_ = (f64(a) for a in (x, dy, mean, invstd, gamma_))
    R = x.shape[0]
    xh = (x - mean) * invstd
    dbeta, dgamma = dy.sum(axis=0), (dy * xh).sum(axis=0)
    kd = gamma_ * invstd
    dx = kd * (dy - dbeta / R - xh * dgamma / R)
    S_dx = np.abs(kd) * (np.abs(dy) + np.abs(dbeta) / R + (np.abs(x) + np.abs(mean)) * invstd * np.abs(dgamma) / R)
    if relu_mask:
        dx = np.where(x > 0, dx, 0.0)
    return dict(dgamma=dgamma, S_dgamma=(np.abs(dy) * (np.abs(x) + np.abs(mean)) * invstd).sum(axis=0), dbeta=dbeta,
                S_dbeta=np.abs(dy).sum(axis=0), dx=dx, S_dx=S_dx, kd_abs=np.abs(kd), xhat_abs=(np.abs(x) + np.abs(mean)) * invstd)


def bn_dx_bound(ref, R, e_dbeta, e_dgamma):
    """bound of dx = k_dy (dy - mean_dy - xhat mean_dyx) for the dict `ref` of bn_bwd: ten roundings of the expression itself
    (three constants, two for xhat, two products, two differences, the final product) on S_dx, plus what the two means inherit
    from their sums -- mean_dy = dbeta / R and mean_dyx = dgamma / R carry e_dbeta / R and e_dgamma / R, the bounds of those sums,
    which a channel with |dgamma| << sum |dy xhat| does not hide behind u |mean_dyx|"""
    return error_bound(ref["S_dx"], 10) + ref["kd_abs"] * (np.asarray(e_dbeta) / R + ref["xhat_abs"] * np.asarray(e_dgamma) / R)


# ------------------------------------------------------------------------------------------ frequency attention
def freq_attention_fwd(H, logits):
    """H [rows, C], logits [rows, d_f]: F = softmax(logits); channel c belongs to bin c / (C / d_f) and is scaled by its weight"""
    H, F = f64(H), mo.softmax(f64(logits))
    rows, C = H.shape
    d_f = F.shape[1]
    return F, (H.reshape(rows, d_f, C // d_f) * F[:, :, None]).reshape(rows, C)


def freq_attention_bwd(H, F, dHw, relu_mask=False):
    """for a GIVEN F: dF[bin] = sum over the bin's channels of dHw H, dlogits = F (dF - sum F dF), dH = dHw F[bin] (times (H > 0))
    -> dict(dF, S_dF, dlogits, dH)"""
    H, F, dHw = f64(H), f64(F), f64(dHw)
    rows, C = H.shape
    d_f = F.shape[1]
    hb, db = H.reshape(rows, d_f, -1), dHw.reshape(rows, d_f, -1)
    dF = (db * hb).sum(axis=2)
    dH = (db * F[:, :, None]).reshape(rows, C)
    if relu_mask:
        dH = np.where(H > 0, dH, 0.0)
    return dict(dF=dF, S_dF=np.abs(db * hb).sum(axis=2), dlogits=F * (dF - (F * dF).sum(axis=1, keepdims=True)), dH=dH)


def freq_attention_dlogits_bound(F, dF, S_dF, cb):
    """dlogits = f (dF - s), s = wave_sum(f dF): with e = error_bound(S_dF, cb) per bin,
        e_s <= sum_j f_j e_j + gamma(7) sum_j |f_j dF_j|        (one product, six butterfly steps)
        |got - ref| <= f (e + e_s) + 2 u f (|dF| + |s|) + 2^-126"""
    F, dF = f64(F), f64(dF)
    e = error_bound(S_dF, cb)
    a = np.abs(F * dF).sum(axis=1, keepdims=True)
    e_s = (F * e).sum(axis=1, keepdims=True) + gamma(7) * a
    return F * (e + e_s) + 2 * U * F * (np.abs(dF) + a) + 2.0 ** -126


# ------------------------------------------------------------------------------------------ the dispatch, restated
def _al16(addr):
    return addr % 16 == 0


def pool_fwd_path(T, C, bs, rs, x_addr, out_addr):
    """launch_pool_fwd(): ("reg", TMAX) | ("lds", V)"""
    vec = C % 4 == 0 and bs % 4 == 0 and rs % 4 == 0 and _al16(x_addr)
    if vec and 1 <= T <= 40 and _al16(out_addr):
        return ("reg", next(m for m in (8, 16, 24, 32, 36, 40) if T <= m))
    return ("lds", 4 if vec else 1)


def pool_fwd_grid(T, C, path):
    """-> (x blocks, live lanes / channel groups of the last x block, rows of the busiest and of the idlest time group)"""
    if path[0] == "reg":
        return cdiv(C, 256), cdiv(C - (cdiv(C, 256) - 1) * 256, 4), T, T
    per = 16 * path[1]
    return cdiv(C, per), cdiv(C - (cdiv(C, per) - 1) * per, path[1]), cdiv(T, 16), T // 16


def pool_bf16_accepts(T, C, bs, rs, x_addr, out_addr):
    """lidbox_stats_pool_fwd_bf16's argument check"""
    return T <= 40 and C % 4 == 0 and bs % 4 == 0 and rs % 4 == 0 and rs >= C and x_addr % 8 == 0 and _al16(out_addr)


def pool_bwd_path(T, C, bs, rs, x_addr, dx_addr, pooled_addr, dout_addr, shadow=None):
    """launch_pool_bwd(): ("rows", z blocks) | ("loop", V, time splits).  shadow = (bs16, rs16, dx16_addr) or None"""
    vec = C % 4 == 0 and bs % 4 == 0 and rs % 4 == 0 and _al16(x_addr) and _al16(dx_addr)
    if shadow is not None:
        vec = vec and shadow[0] % 4 == 0 and shadow[1] % 4 == 0 and shadow[2] % 8 == 0
    if vec and 1 <= T <= 48 and _al16(pooled_addr) and _al16(dout_addr):
        return ("rows", cdiv(T, 12))
    return ("loop", 4 if vec else 1, min(T, 8))


def head_np_u(N):
    """lidbox_softmax_head_fwd_bwd: the instantiation NP and its unroll U"""
    NP = 4 if N <= 4 else 8 if N <= 8 else 16 if N <= 16 else 32
    return NP, {4: 8, 8: 4, 16: 2, 32: 1}[NP]


def head_trips(K, N):
    """-> (trips of lane 0, trips of lane 63, reloaded trips of lane 0): `for (k0 = lane; k0 < K; k0 += 64 U)`"""
    _, Uu = head_np_u(N)
    t0 = cdiv(K, 64 * Uu)
    t63 = cdiv(K - 63, 64 * Uu) if K > 63 else 0
    return t0, t63, t0 - 1


def head_wvec(N, W_addr):
    return N == head_np_u(N)[0] and _al16(W_addr)


def head_logit_chain(K):
    """a lane's ceil(K / 64) fused multiply-adds, six butterfly steps, the bias"""
    return cdiv(K, 64) + 6 + 1


def head_dw_chain(B):
    """softmax_head_wgrad_kernel: 16 row classes of ceil(B / 16) fused multiply-adds, then the 16 partial sums"""
    return cdiv(B, 16) + 16


def head_db_chain(B):
    return cdiv(B, 64) + 6 + 1


def head_workspace_bytes(B, K, N):
    return (B * N + B) * 4 if B > 0 and K > 0 and N > 0 else 0


def loss_trips(B):
    """nll_kernel / softmax_nll_kernel: rows per thread of the single workgroup of 256 -> (thread 0, thread 255)"""
    return cdiv(B, 256), cdiv(B - 255, 256) if B > 255 else 0


def row_lane_trips(N):
    """log_softmax_kernel / softmax_kernel / l2norm: `for (n = lane; n < N; n += 64)` -> (lane 0, lane 63)"""
    return cdiv(N, 64), cdiv(N - 63, 64) if N > 63 else 0


def bn_slices(R):
    return max(1, min(1024, R // 256))


def bn_rows_per_slice(R):
    return cdiv(R, bn_slices(R))


def bn_slice_rows(R):
    """rows of every slice; 0: the slice is empty and must store zeros"""
    rps = bn_rows_per_slice(R)
    return [max(0, min(R, (s + 1) * rps) - s * rps) for s in range(bn_slices(R))]


def bn_workspace_bytes(R, C):
    return bn_slices(R) * 2 * C * 8 + 3 * C * 4 if R >= 0 and C >= 1 else 0


def bn_channel_sum_trips(R):
    """bn_channel_sums: `for (k = t; k < slices; k += 256)` -> trips of thread 0"""
    return cdiv(bn_slices(R), 256)


def bn_apply_path(R, C, addrs, row_stride, batch, batch_stride):
    """lidbox_bn_apply / the apply of lidbox_bn_bwd -> (vec, grid-stride trips of thread 0)"""
    vec = C % 4 == 0 and all(_al16(a) for a in addrs) and row_stride % 4 == 0 and (batch == 1 or batch_stride % 4 == 0)
    n = R * (C // 4 if vec else C)
    return vec, cdiv(n, 8192 * 256)


def attention_grid(rows):
    """rows_grid(): workgroups of 4 waves -> (grid, trips of wave 0 of block 0)"""
    g = min(cdiv(rows, 4), 256 * 8)
    return g, cdiv(rows, g * 4)


def attention_vec(C, addrs):
    return C % 4 == 0 and all(_al16(a) for a in addrs)


def attention_bwd_accepts(C, d_f):
    return 1 <= d_f <= 64 and C % d_f == 0 and C <= 4096


# ------------------------------------------------------------------------------------------ fp32 emulations of the kernels' orders
def _f32(a):
    return np.asarray(a, np.float32)


def emu_sum_in_order(terms, axis=0):
    """fp32 running sum along `axis`, one rounding per addition"""
    t = np.moveaxis(_f32(terms), axis, 0)
    s = np.zeros(t.shape[1:], np.float32)
    for v in t:
        s = (s + v).astype(np.float32)
    return s


def emu_butterfly(v, offsets=(1, 2, 4, 8, 16, 32)):
    """the __shfl_xor butterfly over the LAST axis of 64 lanes (softmax_head_rows_kernel: offsets 1 .. 32; wave_sum: 32 .. 1):
    every lane ends with the same fp32 value"""
    v = _f32(v).copy()
    lanes = np.arange(64)
    for o in offsets:
        v = (v + v[..., lanes ^ o]).astype(np.float32)
    return v[..., 0]


def emu_pool_mean(x, path):
    """fp32 mean of x [B, T, C] in the order of the selected forward kernel"""
    x = _f32(x)
    T = x.shape[1]
    if path[0] == "reg":
        s = emu_sum_in_order(x, axis=1)
    else:
        groups = [emu_sum_in_order(x[:, g::16], axis=1) if g < T else np.zeros((x.shape[0], x.shape[2]), np.float32) for g in range(16)]
        s = emu_sum_in_order(np.stack(groups), axis=0)
    return (s / np.float32(T)).astype(np.float32)


def emu_pool_std(x, path):
    x = _f32(x)
    T = x.shape[1]
    mean = emu_pool_mean(x, path)
    d = (x - mean[:, None, :]).astype(np.float32)

    def chain(dd):
        s = np.zeros((x.shape[0], x.shape[2]), np.float32)
        for t in range(dd.shape[1]):
            s = fma32(dd[:, t], dd[:, t], s)
        return s
    if path[0] == "reg":
        q = chain(d)
    else:
        q = emu_sum_in_order(np.stack([chain(d[:, g::16]) for g in range(16)]), axis=0)
    var = (q / np.float32(T)).astype(np.float32)
    return np.sqrt(np.clip(var, np.float32(1e-10), np.finfo(np.float32).max)).astype(np.float32)


def emu_lane_dot(a, b, offsets=(1, 2, 4, 8, 16, 32)):
    """sum_k a[..., k] b[..., k] as one wave computes it: lane l chains k = l, l + 64, ... with fma, then the butterfly"""
    a, b = _f32(a), _f32(b)
    K = a.shape[-1]
    pad = cdiv(K, 64) * 64 - K
    a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(a.shape[:-1] + (-1, 64))
    b = np.concatenate([b, np.zeros(b.shape[:-1] + (pad,), np.float32)], axis=-1).reshape(b.shape[:-1] + (-1, 64))
    acc = np.zeros(a.shape[:-2] + (64,), np.float32)
    for t in range(a.shape[-2]):
        acc = fma32(a[..., t, :], b[..., t, :], acc)
    return emu_butterfly(acc, offsets)


def emu_head_logits(h, W, bias):
    """z[r, n] of softmax_head_rows_kernel (the U-way unrolled loop adds in the same order as the plain one)"""
    h, W = _f32(h), _f32(W)
    z = np.stack([emu_lane_dot(h, np.broadcast_to(W[:, n], h.shape)) for n in range(W.shape[1])], axis=1)
    return (z + _f32(bias)).astype(np.float32)


def emu_head_dw(h, dz):
    """dW[k, n] of softmax_head_wgrad_kernel: row class s adds rows s, s + 16, ... with fma; one lane adds the 16 classes in order"""
    h, dz = _f32(h), _f32(dz)
    B, K = h.shape
    N = dz.shape[1]
    parts = []
    for s in range(16):
        acc = np.zeros((K, N), np.float32)
        for r in range(s, B, 16):
            acc = fma32(np.broadcast_to(h[r][:, None], (K, N)), np.broadcast_to(dz[r][None, :], (K, N)), acc)
        parts.append(acc)
    return emu_sum_in_order(np.stack(parts), axis=0)


def emu_attention_dF(H, dHw, d_f):
    """dF[row, bin]: one lane chains the bin's C / d_f channels with fma"""
    H, dHw = _f32(H), _f32(dHw)
    rows = H.shape[0]
    hb, db = H.reshape(rows, d_f, -1), dHw.reshape(rows, d_f, -1)
    acc = np.zeros((rows, d_f), np.float32)
    for i in range(hb.shape[2]):
        acc = fma32(db[:, :, i], hb[:, :, i], acc)
    return acc


def emu_l2_sum(x):
    return emu_lane_dot(x, x, (32, 16, 8, 4, 2, 1))
