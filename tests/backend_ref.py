"""
Float64 restatement of the embedding back-end (lidbox/embed/sklearn_utils.py), shared by test_backend_cpu.py and
test_backend_gpu.py: the planted-data generator, the PLDA maths (Ioffe 2006 as the `plda` package's Model implements
it), naive Bayes, LDA, the composed pipeline, and the scoring kernel's oracle with its per-element rounding bound.
Nothing here imports lidbox_amd.
"""
import functools

import numpy as np
import scipy.linalg

U = 2.0 ** -24                  # unit roundoff of fp32
EPS32 = 2.0 ** -23

# (N, D, K, sep, off); the float64 pipeline alone gives the U_model dimensions R below
CASES = [(2000, 64, 10, 0.15, 0), (600, 7, 3, 0.6, 0), (4000, 200, 100, 0.12, 0), (3000, 512, 10, 0.06, 0), (2000, 64, 10, 0.15, 50)]
EXPECTED_R = [9, 2, 83, 9, 9]


def gamma(n):
    return n * U / (1.0 - n * U)


@functools.lru_cache(maxsize=None)
def planted(N, D, K, sep, off, seed=1):
    """train X [N, D], y, held-out X [N/2, D], y; fp32 values (what the device sees), returned as float32"""
    rng = np.random.default_rng(seed)
    M = N + N // 2
    mu = sep * rng.standard_normal((K, D))
    A = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    y = np.arange(M) % K
    rng.shuffle(y)
    X = (mu[y] + rng.standard_normal((M, D)) @ A + off).astype(np.float32)
    for a in (X, y):
        a.setflags(write=False)
    return X[:N], y[:N], X[N:], y[N:]


# ------------------------------------------------------------------ statistics

def class_stats(X, y, f32=False):
    """class means, S_w = sum_k n_k/N cov_k (biased), counts.  f32: the sums run in float32 as on the device (means by a
    float32 mean, the Gram of the float32 centred rows in float32), the result is returned in float64."""
    K = int(y.max()) + 1
    counts = np.bincount(y, minlength=K).astype(np.float64)
    N = X.shape[0]
    if f32:
        X = X.astype(np.float32)
        means = np.stack([X[y == k].mean(axis=0, dtype=np.float32) for k in range(K)])
        Xc = X - means[y]
        Sw = (Xc.T @ Xc).astype(np.float64) / N
        means = means.astype(np.float64)
    else:
        X = X.astype(np.float64)
        means = np.stack([X[y == k].mean(axis=0) for k in range(K)])
        Xc = X - means[y]
        Sw = Xc.T @ Xc / N
    return means, 0.5 * (Sw + Sw.T), counts


def between(means, counts):
    p = counts / counts.sum()
    m = p @ means
    d = means - m
    return m, (d * p[:, None]).T @ d


def plda_fit(m, Sb, Sw, n, n_components=None):
    """dict with C (PCA components [D, c] or None), W, A, inv_A, Psi (before and after clipping), relevant, P [D, R]"""
    D = Sw.shape[0]
    lam = np.linalg.eigvalsh(Sw)
    rank = int((lam > D * EPS32 * lam.max()).sum())
    C = None
    Sb0, Sw0 = Sb, Sw
    if n_components is not None or rank < D:
        nc = rank if n_components is None else n_components
        _, vec = np.linalg.eigh(Sw + Sb)
        C = vec[:, ::-1][:, :nc]
        Sb, Sw = C.T @ Sb @ C, C.T @ Sw @ C
        Sb, Sw = 0.5 * (Sb + Sb.T), 0.5 * (Sw + Sw.T)
    _, W = scipy.linalg.eigh(Sb, Sw)
    Lb, Lw = np.diag(W.T @ Sb @ W), np.diag(W.T @ Sw @ W)
    scale = np.sqrt(n / (n - 1.0) * Lw)
    A = np.linalg.inv(W.T) * scale[None, :]
    inv_A = np.linalg.inv(A)
    psi_raw = (n - 1.0) / n * Lb / Lw - 1.0 / n
    Psi = np.maximum(0.0, psi_raw)
    rel = np.flatnonzero(Psi != 0)
    T = inv_A.T[:, rel]
    return dict(m=m, C=C, W=W, A=A, inv_A=inv_A, psi_raw=psi_raw, Psi=Psi, relevant=rel, P=T if C is None else C @ T, Sb=Sb, Sw=Sw,
                Sb_D=Sb0, Sw_D=Sw0, rank=rank, n=n)


def plda_fit_data(X, y, n_components=None, f32=False):
    means, Sw, counts = class_stats(X, y, f32)
    m, Sb = between(means, counts)
    f = plda_fit(m, Sb, Sw, X.shape[0] / counts.shape[0], n_components)
    f.update(means=means, counts=counts)
    return f


def plda_transform(f, X):
    return (X.astype(np.float64) - f["m"]) @ f["P"]


def plda_predictive(f):
    """(theta, var) of the posterior predictive per class in U_model"""
    psi = f["Psi"][f["relevant"]]
    ubar = (f["means"] - f["m"]) @ f["P"]
    nk = f["counts"][:, None]
    return nk * psi / (1.0 + nk * psi) * ubar, 1.0 + psi / (1.0 + nk * psi)


def gauss_logpdf(X, theta, var):
    """[N, K] sum_r log N(x_r; theta_kr, var_kr)"""
    d = X[:, None, :] - theta[None]
    return -0.5 * (np.log(2 * np.pi * var).sum(axis=1))[None] - 0.5 * (d * d / var[None]).sum(axis=2)


def log_softmax(s):
    m = s.max(axis=1, keepdims=True)
    return s - m - np.log(np.exp(s - m).sum(axis=1, keepdims=True))


def l2n(X):
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return X / np.where(n == 0, 1.0, n)


def nb_fit(X, y, f32=False):
    K = int(y.max()) + 1
    dt = np.float32 if f32 else np.float64
    X = X.astype(dt)
    theta = np.stack([X[y == k].mean(axis=0, dtype=dt) for k in range(K)])
    var = np.stack([((X[y == k] - theta[k]) ** 2).mean(axis=0, dtype=dt) for k in range(K)]).astype(np.float64)
    var = var + 1e-9 * X.astype(np.float64).var(axis=0).max()
    prior = np.bincount(y, minlength=K) / y.shape[0]
    return theta.astype(np.float64), var, prior


def nb_log_proba(X, theta, var, prior):
    return log_softmax(gauss_logpdf(X.astype(np.float64), theta, var) + np.log(prior)[None])


def lda_fit(X, y, unbiased):
    """(coef [K, D], intercept [K], xbar [D]) of the discriminant in its centred form coef (x - xbar) + intercept, which adds
    the same number to every class's score as the uncentred one and keeps rows far from the origin from cancelling; pooled
    covariance divided by N - K (sklearn's svd solver) or by N (lsqr / eigen)"""
    means, Sw, counts = class_stats(X, y)
    N, K = X.shape[0], counts.shape[0]
    cov = Sw * (N / (N - K)) if unbiased else Sw
    xbar = (counts / N) @ means
    coef = np.linalg.solve(cov, (means - xbar).T).T
    return coef, -0.5 * ((means - xbar) * coef).sum(axis=1) + np.log(counts / N), xbar


def lda_log_proba(X, coef, intercept, xbar=0.0):
    return log_softmax((X.astype(np.float64) - xbar) @ coef.T + intercept)


def pipeline_fit(X, y, n_components=None, f32=False):
    """StandardScaler -> PLDA -> L2 -> GaussianNB fitted step by step in float64; f32: every statistic over the rows is
    accumulated in float32 and every intermediate [N, .] array is rounded to float32, as the device holds them"""
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if f32 else (lambda a: a)
    X = X.astype(np.float64)
    mean, var = X.mean(axis=0), X.var(axis=0)
    scale = np.where(var > 0, np.sqrt(var), 1.0)
    if f32:
        mean, scale = rnd(mean), 1.0 / rnd(1.0 / scale)
    Xs = rnd((X - mean) / scale)
    f = plda_fit_data(Xs, y, n_components, f32)
    if f32:
        f["m"], f["P"] = rnd(f["m"]), rnd(f["P"])
    V = rnd(l2n(rnd(plda_transform(f, Xs))))
    theta, nvar, prior = nb_fit(V, y, f32)
    return dict(mean=mean, scale=scale, plda=f, theta=theta, var=nvar, prior=prior)


def pipeline_steps(p, X):
    """(scaled, U_model, normalised, clipped log-probabilities) of the fitted pipeline on X, float64"""
    Xs = (X.astype(np.float64) - p["mean"]) / p["scale"]
    Um = plda_transform(p["plda"], Xs)
    V = l2n(Um)
    return Xs, Um, V, np.maximum(nb_log_proba(V, p["theta"], p["var"], p["prior"]), -100.0)


def min_principal_cosine(A, B):
    """smallest cosine of the principal angles between the column spans of A and B"""
    qa, qb = scipy.linalg.orth(A), scipy.linalg.orth(B)
    return float(np.linalg.svd(qa.T @ qb, compute_uv=False).min())


def max_principal_sine(A, B):
    """largest sine of the principal angles between two spans of the same dimension (accurate for small angles)"""
    qa, qb = scipy.linalg.orth(A), scipy.linalg.orth(B)
    return float(np.linalg.svd(qb - qa @ (qa.T @ qb), compute_uv=False).max())


# ------------------------------------------------------------------ the scoring kernel's oracle

L2, NORMALISED, LINEAR = 1, 2, 4


def score_oracle(x, mu, P, q, theta, w, c0, flags):
    """float64 evaluation of lidbox_backend_score on the fp32 values given, with a rounding bound per element.

    Bounds (u = 2^-24, gamma_n = n u / (1 - n u); Higham, Accuracy and Stability, section 3.1).  The norm, class and softmax
    stages use gamma_n sum|terms|, which holds for ANY order of the fp32 additions.  The u stage does not: its bound follows
    the order in which csrc/backend.hip adds (k ascending, four products per MFMA into one accumulator per output) and
    would have to change with it.
      u stage   a running bound instead of gamma_{D+3} S, S = sum_k |x_k - mu_k| |P_kr|: the discriminative directions are
                small projections of large sums (S / |u| reaches 10^3 at D = 512) and D u S would swamp every later stage.
                The kernel adds the products in the order of k, four per v_mfma_f32_16x16x4_f32 into one accumulator; the
                accumulator after group g is rounded once, u |S_g| with S_g the partial sum, whatever happens inside the
                instruction costs at most 3 u of the group's |terms| (three additions among four products, in whatever
                order; the products themselves are not rounded: the instruction is a chain of fused multiply-adds), each
                term carries the one rounding of x - mu (u of the term), and q is added once (u |u|, and |q_r| for a
                rounding before the sum): |du| <= 1.01 u (sum_g |S_g| + (3 + 1) S + |u| + |q_r|), the 1.01 for the
                second-order terms
      norm      ss = sum u^2 over R terms, then sqrt and the division:
                d(ss) <= 2 sum |u| du + sum du^2 + gamma_{R+2} ss;  rel(norm) <= 0.505 d(ss) / ss + 2 u;
                dv <= du / norm + |v| (rel(norm) + u)
      class     d = v - theta: dd <= dv + u |d|;  t = d^2 w;  ds <= 1/2 sum_r (2 |d| dd + dd^2) w + (1/2 gamma_{R+3} + u) sum t
                + 2 u |c0|
      softmax   lse(s + e) - lse(s) = log sum_c p_c exp(e_c), p = softmax(s), so ds moves lse by at most log sum_c p_c exp(ds_c)
                (Jensen gives the same bound for the other sign).  Its own arithmetic (s - m, expf and
                logf within 2 ulp, K additions) costs at most u (|m| + |lse| + 2 K + 16): a term with s - m = -a weighs
                e^-a, and a e^-a <= 0.37.  The final subtraction rounds once more.
    Returns dict(u, v, s, out, ev, eo): values (v after the optional L2 step; out after the optional log-softmax and clip)
    and bounds for v and out."""
    x, P = x.astype(np.float64), P.astype(np.float64)
    N, D = x.shape
    R = P.shape[1]
    xm = x - (0.0 if mu is None else mu.astype(np.float64))
    qq = np.zeros(R) if q is None else q.astype(np.float64)
    u = xm @ P + qq
    eu = np.empty_like(u)
    Dp = (D + 3) // 4 * 4
    for a in range(0, N, 128):                                      # row blocks: the [rows, D, R] products stay small
        T = np.zeros((min(128, N - a), Dp, R))
        T[:, :D] = xm[a:a + 128, :, None] * P[None]
        partial = np.cumsum(T.reshape(T.shape[0], Dp // 4, 4, R).sum(axis=2), axis=1)
        eu[a:a + 128] = 1.01 * U * (np.abs(partial).sum(axis=1) + 4 * np.abs(T).sum(axis=1) + np.abs(u[a:a + 128]) + np.abs(qq))
    eu += D * 2.0 ** -126
    if flags & L2:
        ss = (u * u).sum(axis=1, keepdims=True)
        nrm = np.sqrt(ss)
        safe = np.where(ss == 0, 1.0, ss)
        dss = 2 * (np.abs(u) * eu).sum(axis=1, keepdims=True) + (eu * eu).sum(axis=1, keepdims=True) + gamma(R + 2) * ss
        reln = 0.505 * dss / safe + 2 * U
        nn = np.where(nrm == 0, 1.0, nrm)
        v = u / nn
        ev = eu / nn + np.abs(v) * (reln + U)
    else:
        v, ev = u, eu
    res = dict(u=u, v=v, ev=ev, s=None, out=None, eo=None)
    if theta is None and not flags & LINEAR:
        return res
    if flags & LINEAR:
        s, es = v, ev
    else:
        th, ww, cc = theta.astype(np.float64), w.astype(np.float64), c0.astype(np.float64)
        d = v[:, None, :] - th[None]
        dd = ev[:, None, :] + U * np.abs(d)
        t = d * d * ww[None]
        st = t.sum(axis=2)
        s = cc[None] - 0.5 * st
        es = 0.5 * ((2 * np.abs(d) * dd + dd * dd) * np.abs(ww)[None]).sum(axis=2) + (0.5 * gamma(R + 3) + U) * np.abs(t).sum(axis=2) \
            + 2 * U * np.abs(cc)[None]
    K = s.shape[1]
    if flags & NORMALISED:
        m = s.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(s - m).sum(axis=1, keepdims=True))
        raw = s - lse
        # lse(s + e) - lse(s) = log sum_c p_c exp(e_c) with p = softmax(s): a class far below the maximum cannot move it
        dl = np.log((np.exp(raw) * np.exp(np.minimum(es, 700.0))).sum(axis=1, keepdims=True))
        eo = es + dl + U * (np.abs(m) + np.abs(lse) + 2 * K + 16) + 2 * U * np.abs(raw)
        res.update(s=s, raw=raw, out=np.maximum(raw, -100.0), eo=eo)
    else:
        res.update(s=s, raw=s, out=s, eo=es)
    return res


def assert_score_close(got, ref, bound, what, clip_raw=None):
    """elementwise |got - ref| <= bound; where clip_raw (the unclipped reference) is clearly below -100 the value must be
    exactly -100"""
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    if clip_raw is not None:
        sure = clip_raw < -100.0 - bound
        assert (got[sure] == -100.0).all(), what + ": a value below -100 did not come out as exactly -100"
        assert (got >= -100.0).all(), what + ": a value below -100 survived the clip"
        near = np.abs(clip_raw + 100.0) <= bound                    # either side of the clip is acceptable there
        err = np.where(near, np.minimum(err, np.abs(got + 100.0)), err)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    print("%s: max err %.3e, max err/bound %.3f" % (what, float(err.max()) if err.size else 0.0, worst))
    assert np.isfinite(got).all(), what + ": non-finite output"
    assert worst <= 1.0, "%s: error %.3e exceeds the derived bound (ratio %.2f)" % (what, float(err.max()), worst)
