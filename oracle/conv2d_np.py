"""
float64 numpy restatement of csrc/conv2d.hip, written from the definitions in that file's header comments and not through
any library convolution: a loop over the kernel's taps with one einsum (or one [C_in, M] @ [M, C_out] product) per tap on a
zero-padded copy.  tests/test_oracle_conv2d.py pins it against torch.nn.functional.conv2d + autograd.

Layouts are the library's: images time-major [B, T, F, C], channels innermost.
  stride 1 "same":  W[kh][kw][ci][co], kh over frequency, kw over time, p = (k - 1) / 2
      y[b, t, f, co] = bias[co] + sum_{kh, kw, ci} x[b, t + kw - p, f + kh - p, ci] W[kh, kw, ci, co]
  strided:          taps = (kt, kf, sf, pt0, pt1, pf0, pf1, time_first), W[kt][kf][ci][co] (time_first) or W[kf][kt][ci][co]
      y[b, to, fo, co] = bias[co] + sum_{i, j, ci} x[b, to + i - pt0, fo sf + j - pf0, ci] W[tap(i, j), ci, co]
A stride-1 call is the strided form with taps (k, k, 1, p, p, p, p, 0); every function takes either `k` (int) or `taps`.

abs_bound_*: the same operation on the absolute values of its operands: sum |terms| of every output element, the S of
    |got - ref| <= gamma(n) S + n 2^-126
that holds for an fp32 chain of n fused multiply-adds in any order (tests/test_conv2d_paths_gpu.py states the derivation).

The second half restates the host-side dispatch of conv2d.hip (tile width, wgrad partition plan, the live taps of a strided
forward / dgrad column, the (tile, partition) pairs the strided wgrad skips), so that a CPU test can prove which path a test
shape selects.
"""
import collections

import numpy as np

Taps = collections.namedtuple("Taps", "kt kf sf pt0 pt1 pf0 pf1 time_first")

U = 2.0 ** -24                   # fp32 unit roundoff
CV_BM, CV_KC = 128, 16           # conv2d.hip: tile rows, contraction elements per LDS chunk
EW_CAP = 8192 * 256              # conv2d.hip ew_blocks(): elements one grid-stride trip covers


def as_taps(k):
    if isinstance(k, Taps):
        return k
    if isinstance(k, (tuple, list)):
        return Taps(*k)
    p = (int(k) - 1) // 2
    return Taps(int(k), int(k), 1, p, p, p, p, 0)


def out_size(T, F, k):
    t = as_taps(k)
    return T + t.pt0 + t.pt1 - t.kt + 1, (F + t.pf0 + t.pf1 - t.kf) // t.sf + 1


def _w_tap(W, t, i, j):
    """W[tap(i, j)] as [C_in, C_out]: i the time tap, j the frequency tap"""
    return W[i, j] if t.time_first else W[j, i]


def _w_shape(t, Ci, Co):
    return (t.kt, t.kf, Ci, Co) if t.time_first else (t.kf, t.kt, Ci, Co)


def _padded(x, t):
    return np.pad(np.asarray(x, np.float64), ((0, 0), (t.pt0, t.pt1), (t.pf0, t.pf1), (0, 0)))


def _window(xp, t, i, j, To, Fo):
    """xp[b, to + i, fo sf + j, :] for every (to, fo)"""
    return xp[:, i:i + To, j:j + (Fo - 1) * t.sf + 1:t.sf, :]


def fwd(x, W, bias, k, relu=False):
    t = as_taps(k)
    B, T, F, Ci = x.shape
    W = np.asarray(W, np.float64)
    To, Fo = out_size(T, F, t)
    xp = _padded(x, t)
    y = np.zeros((B, To, Fo, W.shape[3]))
    for i in range(t.kt):
        for j in range(t.kf):
            y += np.einsum("btfc,cd->btfd", _window(xp, t, i, j, To, Fo), _w_tap(W, t, i, j))
    if bias is not None:
        y += np.asarray(bias, np.float64)
    return np.maximum(y, 0.0) if relu else y


def dgrad(dy, W, k, T, F):
    """dx[b, t, f, ci] = sum over the (to, fo, i, j) with to + i - pt0 = t, fo sf + j - pf0 = f of dy[b, to, fo, :] . W[tap(i, j), ci, :]"""
    t = as_taps(k)
    dy = np.asarray(dy, np.float64)
    W = np.asarray(W, np.float64)
    B, To, Fo, _ = dy.shape
    dxp = np.zeros((B, T + t.pt0 + t.pt1, F + t.pf0 + t.pf1, W.shape[2]))
    for i in range(t.kt):
        for j in range(t.kf):
            _window(dxp, t, i, j, To, Fo)[...] += np.einsum("btfd,cd->btfc", dy, _w_tap(W, t, i, j))
    return np.ascontiguousarray(dxp[:, t.pt0:t.pt0 + T, t.pf0:t.pf0 + F, :])


def wgrad(x, dy, k):
    """dW in W's layout: per tap one [C_in, M] @ [M, C_out] product"""
    t = as_taps(k)
    B, T, F, Ci = x.shape
    dy = np.asarray(dy, np.float64)
    _, To, Fo, Co = dy.shape
    xp = _padded(x, t)
    dW = np.zeros(_w_shape(t, Ci, Co))
    d2 = dy.reshape(-1, Co)
    for i in range(t.kt):
        for j in range(t.kf):
            _w_tap(dW, t, i, j)[...] = np.ascontiguousarray(_window(xp, t, i, j, To, Fo)).reshape(-1, Ci).T @ d2
    return dW


def bias_grad(dy):
    dy = np.asarray(dy, np.float64)
    return dy.reshape(-1, dy.shape[-1]).sum(axis=0)


def abs_bound_fwd(x, W, bias, k):
    return fwd(np.abs(x), np.abs(W), None if bias is None else np.abs(bias), k)


def abs_bound_dgrad(dy, W, k, T, F):
    return dgrad(np.abs(dy), np.abs(W), k, T, F)


def abs_bound_wgrad(x, dy, k):
    return wgrad(np.abs(x), np.abs(dy), k)


def abs_bound_bias_grad(dy):
    return bias_grad(np.abs(dy))


def gamma(n):
    """(n + 2) u / (1 - (n + 2) u): n roundings of a chain plus two of slack (the bias add, the final store)"""
    return (n + 2) * U / (1.0 - (n + 2) * U)


def error_bound(S, n):
    return gamma(n) * np.asarray(S, np.float64) + n * 2.0 ** -126


# ------------------------------------------------------------------------------------------ element-wise passes, pooling, L2
def fma32(x, a, b):
    """the fp32 fused multiply-add round(x a + b) with ONE rounding, for fp32 inputs: the product is exact in float64, the sum's
    float64 rounding error is recovered with TwoSum, and it decides the rare case in which the float64 sum sits exactly on the
    midpoint of two fp32 neighbours"""
    x, a, b = (np.asarray(v, np.float32).astype(np.float64) for v in (x, a, b))
    p = x * a
    s = p + b
    bb = s - p
    e = (p - (s - bb)) + (b - bb)
    r = s.astype(np.float32)
    up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    r64 = r.astype(np.float64)
    fix_up = (s == (r64 + up.astype(np.float64)) / 2) & (e > 0)
    fix_dn = (s == (r64 + dn.astype(np.float64)) / 2) & (e < 0)
    return np.where(fix_up, up, np.where(fix_dn, dn, r)).astype(np.float32)


def bn_relu(x, scale, shift):
    """relu(x scale[c] + shift[c]), channels innermost; fp32 result of the one fma the kernels use"""
    return np.maximum(fma32(x, scale, shift), np.float32(0))


def bn_relu_grad(x, scale, shift, dy):
    """dy where the BatchNormalization output is positive, else 0.  The sign of the exact x scale + shift: float64 rounds
    the exact sum of an exact product and keeps its sign"""
    v = np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return np.where(v > 0, np.asarray(dy), np.zeros_like(np.asarray(dy)))


def bn_relu_maxf(x, scale, shift):
    """max over F of relu(x scale + shift): x [B, T, F, C] -> [B, T, C]"""
    return bn_relu(x, scale, shift).max(axis=2)


def bn_relu_maxf_grad(x, scale, shift, dy):
    """TF's _MinOrMaxGrad followed by ReLU's gradient: dy split evenly over every f whose relu output equals the maximum, then
    zero where the output is not positive.  -> (dx float64 [B, T, F, C], count [B, T, C] of the tied cells)"""
    r = bn_relu(x, scale, shift).astype(np.float64)
    m = r.max(axis=2, keepdims=True)
    tied = r == m
    cnt = tied.sum(axis=2)
    dx = np.where(tied & (r > 0), np.asarray(dy, np.float64)[:, :, None, :] / cnt[:, :, None, :], 0.0)
    return dx, cnt


def bn_maxpool2d(x, scale, shift):
    """BN-apply, then the 2 x 2 "valid" maximum with the FIRST maximum in the reference image's scan order: (freq 0, time 0),
    (freq 0, time 1), (freq 1, time 0), (freq 1, time 1); code = 2 dfreq + dtime.  -> (y float64, code uint8)"""
    v = np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    B, T, F, C = v.shape
    T2, F2 = T // 2, F // 2
    v = v[:, :2 * T2, :2 * F2].reshape(B, T2, 2, F2, 2, C)            # [b, t2, dt, f2, df, c]
    cand = np.stack([v[:, :, dt, :, df] for df in (0, 1) for dt in (0, 1)], axis=0)
    code = cand.argmax(axis=0)                                       # numpy: the first occurrence
    return cand.max(axis=0), code.astype(np.uint8)


def maxpool2d_grad(dy, code, T, F):
    """each input cell takes its window's gradient when it is the recorded winner; dropped odd cells get zero"""
    dy = np.asarray(dy)
    B, T2, F2, C = dy.shape
    dx = np.zeros((B, T, F, C), dy.dtype)
    for df in (0, 1):
        for dt in (0, 1):
            dx[:, dt:2 * T2:2, df:2 * F2:2] = np.where(code == 2 * df + dt, dy, 0)
    return dx


def l2_penalty(params, grads, offsets, sizes, lambdas, grad_scale, loss0=0.0):
    """grads[o : o + n] += 2 lam grad_scale params[o : o + n] per tensor; loss = loss0 + sum lam sum w^2  (float64)"""
    g = None if grads is None else np.array(grads, np.float64)
    loss = float(loss0)
    for o, n, lam in zip(offsets, sizes, lambdas):
        w = np.asarray(params[o:o + n], np.float64)
        if g is not None:
            g[o:o + n] += 2.0 * lam * grad_scale * w
        loss += lam * float((w * w).sum())
    return g, loss


# ------------------------------------------------------------------------------------------ the dispatch of conv2d.hip, restated
def cdiv(a, b):
    return -(-a // b)


def conv_tile_n(C):
    """conv_tile_n(): `Cout % 64 == 0 ? 64 : Cout % 32 == 0 ? 32 : 16`"""
    return 64 if C % 64 == 0 else 32 if C % 32 == 0 else 16


def wgrad_plan(K, M, C_out):
    """wgrad_plan_kmn() -> (P, per)"""
    tiles = cdiv(K, CV_BM) * (C_out // conv_tile_n(C_out))
    p = min(cdiv(1024, tiles), cdiv(M, 512), 1024)
    p = max(p, 1)
    return p, cdiv(cdiv(M, CV_KC), p) * CV_KC


def wgrad_workspace_bytes(K, M, C_out):
    P, _ = wgrad_plan(K, M, C_out)
    return P * (K * C_out + C_out) * 4


def partitions(M, P, per):
    """[(lo, hi)] of every partition; hi <= lo: the partition is empty (`p * per >= M`)"""
    return [(p * per, min(M, (p + 1) * per)) for p in range(P)]


def sconv_fwd_taps(F, k, fo):
    """sconv_kernel<BN, false>: (j0, nj), the frequency taps of output column fo that land inside the image"""
    t = as_taps(k)
    f0 = fo * t.sf - t.pf0
    j0 = max(0, -f0)
    return j0, max(0, min(t.kf, F - f0) - j0)


def sconv_dgrad_taps(F, k, f):
    """sconv_kernel<BN, true>: (j0, nj, fo0), the taps j = j0 + sf m that reach input column f, tap m from column fo0 - m"""
    t = as_taps(k)
    Fo = (F + t.pf0 + t.pf1 - t.kf) // t.sf + 1
    jf, q0 = (f + t.pf0) % t.sf, (f + t.pf0) // t.sf
    mlo, mhi = max(0, q0 - Fo + 1), min((t.kf - jf + t.sf - 1) // t.sf, q0 + 1)
    return jf + mlo * t.sf, max(0, mhi - mlo), q0 - mlo


def _tap_ij(t, tap):
    return (tap // t.kf, tap % t.kf) if t.time_first else (tap % t.kt, tap // t.kt)


def sconv_wgrad_tile_taps(Cin, k, tile):
    """the (i, j) of every tap with a row in K tile `tile` (rows kidx = tap C_in + ci, 128 per tile)"""
    t = as_taps(k)
    K = t.kt * t.kf * Cin
    klast = min(K, (tile + 1) * CV_BM) - 1
    return [_tap_ij(t, tap) for tap in range(tile * CV_BM // Cin, klast // Cin + 1)]


def sconv_wgrad_pairs(B, T, F, Cin, Cout, k):
    """-> (P, per, skipped, dead): `skipped` the (tile, partition) pairs sconv_wgrad_kernel's `live` test turns off (its
    jmin / jmax condition restated), `dead` the pairs whose every (frequency tap, column) product reads padding -- the only
    pairs that MAY be skipped.  Empty partitions are in neither."""
    t = as_taps(k)
    To, Fo = out_size(T, F, t)
    K, BTo = t.kt * t.kf * Cin, B * To
    P, per = wgrad_plan(K, BTo * Fo, Cout)
    skipped, dead = set(), set()
    for p, (lo, hi) in enumerate(partitions(BTo * Fo, P, per)):
        if hi <= lo:
            continue
        cols = range(lo // BTo, (hi - 1) // BTo + 1)
        for tile in range(cdiv(K, CV_BM)):
            js = [j for _, j in sconv_wgrad_tile_taps(Cin, t, tile)]
            if all(not 0 <= fo * t.sf + j - t.pf0 < F for fo in cols for j in js):
                dead.add((tile, p))
            live = tile == 0 or any(fo * t.sf + max(js) - t.pf0 >= 0 and fo * t.sf + min(js) - t.pf0 < F for fo in cols)
            if not live:
                skipped.add((tile, p))
    return P, per, skipped, dead
