"""
Counterpart of lidbox/embed/sklearn_utils.py: the back-end between `extract_embeddings` and the report,

    StandardScaler -> PLDA -> L2-normalise -> GaussianNB -> log-probabilities clipped at -100

with the embeddings staying on the HIP device.  Every pass over the [N, D] data is a kernel of liblidbox_hip.so
(lidbox_backend_score, lidbox_backend_center_rows, lidbox_bn_train_stats, lidbox_segment_mean, lidbox_gemm_tn); every D x D
or K x R solve is float64 on the host (scipy.linalg.eigh, numpy.linalg).  There is no CPU fallback: inputs are CUDA fp32
tensors, or numpy arrays that are copied to the device; without a device the library's usual error is raised.

The estimators keep their fitted state as numpy float64 arrays (so joblib.dump / load works) and rebuild fp32 device
copies lazily.

PLDA follows Ioffe 2006 as the `plda` package's Model implements it (the reference subclasses its Classifier); that
package is not a dependency here and parity with it is unpinned: see docs/TRACEABILITY.md 8(f).  With n = N / K:
    m = mean of rows, S_b = sum_k n_k/N (m_k - m)(m_k - m)^T, S_w = sum_k n_k/N cov_k (biased)
    PCA first when n_components is given or rank(S_w) < D: the top eigenvectors C of S_t = S_w + S_b, S -> C^T S C
    W = eigenvectors of eigh(S_b, S_w), L_b = diag(W^T S_b W), L_w = diag(W^T S_w W)
    A = W^-T diag(sqrt(n/(n-1) L_w)), Psi = max(0, (n-1)/n L_b/L_w - 1/n), relevant = {Psi != 0}
    transform(x) = ((pca(x) - m) A^-T)[relevant]                                          (D -> U_model)
    predict: per class the posterior predictive N(n_k Psi/(1 + n_k Psi) u_k, 1 + Psi/(1 + n_k Psi)) with u_k the class's
             training mean in U_model; unnormalised log-densities
The reference's fit_plda passes `n_principal_components=` to PLDA.fit, whose parameter is `n_components` (TypeError);
the evident intent is built (SURVEY, reference defects).  The plotting functions are not built.
"""
import collections
import logging
import os

import numpy as np
import torch

from .. import _native as nv
from .. import util as _util

logger = logging.getLogger(__name__)

_EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ device plumbing

def _as_device(X, name="X"):
    """CUDA fp32 [N, D] tensor with unit column stride from a CUDA tensor or a numpy array"""
    if isinstance(X, np.ndarray):
        if not torch.cuda.is_available():
            raise nv.LidboxHipError("%s: lidbox_amd runs on the HIP device only (no CPU fallback) and no device is present" % name)
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    X = nv.require_gpu_tensor(X, name, torch.float32)
    if X.dim() != 2:
        raise ValueError("%s must be [rows, features], got shape %s" % (name, tuple(X.shape)))
    if X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < X.shape[1]):
        X = X.contiguous()
    return X


def _like(result, X):
    """results come back as the kind of array the caller passed"""
    return result.cpu().numpy() if isinstance(X, np.ndarray) else result


def _labels(y, N=None):
    """host int64 labels, checked to be exactly 0 .. K-1 with at least two rows per class; returns (y, counts)"""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.asarray(y)
    if y.ndim != 1 or (N is not None and y.shape[0] != N):
        raise ValueError("y must be a vector with one label per row")
    if y.size == 0:
        raise ValueError("no rows")
    if not np.issubdtype(y.dtype, np.integer):
        if not np.all(y == np.floor(y)):
            raise ValueError("labels must be integers 0 .. K-1")
    y = y.astype(np.int64)
    if y.min() < 0:
        raise ValueError("labels must be integers 0 .. K-1, got %d" % y.min())
    counts = np.bincount(y)
    if (counts == 0).any():
        raise ValueError("labels must cover 0 .. K-1 without gaps; missing: %s" % np.flatnonzero(counts == 0)[:8].tolist())
    if (counts < 2).any():
        raise ValueError("every class needs at least two rows; class %d has one" % int(np.flatnonzero(counts < 2)[0]))
    return y, counts


def _ptr(t, offset_floats=0):
    return None if t is None else nv.C.c_void_p(t.data_ptr() + 4 * offset_floats)


def _f32(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def backend_score(X, P, mu=None, q=None, theta=None, w=None, c0=None, flags=0, want_v=False, want_out=True):
    """lidbox_backend_score on X [N, D] (CUDA fp32, any row stride) with fp32 device parameters; rows beyond the per-call
    limit are split here.  Returns (v or None, out or None)."""
    N, D = X.shape
    R = P.shape[1]
    linear = bool(flags & nv.BACKEND_LINEAR)
    K = theta.shape[0] if theta is not None else (R if linear else 0)
    want_out = want_out and (theta is not None or linear)
    v = torch.empty((N, R), dtype=torch.float32, device=X.device) if want_v else None
    out = torch.empty((N, K), dtype=torch.float32, device=X.device) if want_out else None
    ldx = X.stride(0) if N > 1 else D
    with torch.cuda.device(X.device):
        for s in range(0, max(N, 1), nv.BACKEND_MAX_ROWS):
            n = min(nv.BACKEND_MAX_ROWS, N - s)
            nv.check(nv.lib.lidbox_backend_score(
                _ptr(X, s * ldx), n, D, ldx, _ptr(mu), _ptr(P), _ptr(q), R, _ptr(theta), _ptr(w), _ptr(c0), K, flags,
                _ptr(v, s * R), R, _ptr(out, s * K), K, nv.current_stream()))
    return v, out


def center_rows(X, mu=None, inv_scale=None, cm=None, offsets=None, square=False):
    """lidbox_backend_center_rows: (X - mu) * inv_scale - cm[segment of the row], squared on request -> new [N, D] tensor"""
    N, D = X.shape
    out = torch.empty((N, D), dtype=torch.float32, device=X.device)
    nseg = 0 if offsets is None else offsets.numel() - 1
    with torch.cuda.device(X.device):
        nv.check(nv.lib.lidbox_backend_center_rows(
            _ptr(X), N, D, X.stride(0) if N > 1 else D, _ptr(mu), _ptr(inv_scale), _ptr(cm),
            None if offsets is None else nv.C.c_void_p(offsets.data_ptr()), nseg, int(square), _ptr(out), D, nv.current_stream()))
    return out


_STATS_EPS = 1e-30


def column_stats(X):
    """column mean and biased variance of X [N, D] as float64 host arrays: lidbox_bn_train_stats sums in float64 on the
    device (one pass, no cancellation on data far from zero).  Its invstd is 1 / sqrt(var + eps) and it wants eps > 0:
    eps = 1e-30 vanishes beside any fp32 variance above 1e-22, and a column whose variance comes back at or below 2 eps is
    constant (variance 0)."""
    X = X.contiguous()
    N, D = X.shape
    dev = X.device
    ones, zeros = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    res = torch.empty((4, D), dtype=torch.float32, device=dev)
    nbytes = int(nv.lib.lidbox_bn_workspace(N, D))
    ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib.lidbox_bn_train_stats(_ptr(X), N, D, _ptr(ones), _ptr(zeros), _STATS_EPS, 0.0, None, None, _ptr(res[0]),
                                              _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), nv.C.c_void_p(ws.data_ptr()), nbytes,
                                              nv.current_stream()))
    r = res.cpu().numpy().astype(np.float64)
    var = 1.0 / (r[1] * r[1]) - _STATS_EPS
    return r[0], np.where(var <= 2 * _STATS_EPS, 0.0, var)


def _sort_by_class(X, y):
    """rows permuted so that each class is contiguous (stable), with the segment offsets on host and device"""
    order = np.argsort(y, kind="stable")
    counts = np.bincount(y)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    Xs = X.index_select(0, torch.from_numpy(order).to(X.device))
    return Xs, offsets, torch.from_numpy(offsets).to(X.device)


def class_statistics(X, y, scatter=True):
    """class means [K, D] (float64, from lidbox_segment_mean) and, when `scatter`, the within-class scatter
    S_w = sum_k n_k/N cov_k (biased) from the centred rows through lidbox_gemm_tn (fixed-order reduce: run-to-run
    identical).  Also returns the centred-and-sorted intermediates needed by GaussianNB."""
    Xs, offsets, offsets_dev = _sort_by_class(X, y)
    N, D = Xs.shape
    means_dev = _util.segment_mean(Xs, offsets)
    means = means_dev.cpu().numpy().astype(np.float64)
    Sw = None
    if scatter:
        Xc = center_rows(Xs, cm=means_dev, offsets=offsets_dev)
        G = torch.empty((D, D), dtype=torch.float32, device=X.device)
        nbytes = int(nv.lib.lidbox_gemm_tn_workspace(N, D, D))
        ws = torch.empty(max(16, nbytes), dtype=torch.uint8, device=X.device)
        rows = nv.Rows(Xc.data_ptr(), 0, D, 1, N)
        with torch.cuda.device(X.device):
            nv.check(nv.lib.lidbox_gemm_tn(rows, rows, _ptr(G), D, D, D, 0, None, nv.C.c_void_p(ws.data_ptr()), nbytes,
                                           nv.current_stream()))
        Sw = G.cpu().numpy().astype(np.float64) / N
        Sw = 0.5 * (Sw + Sw.T)
    return means, Sw, (Xs, offsets, offsets_dev, means_dev)


def between_scatter(means, counts):
    """m and S_b = sum_k n_k/N (m_k - m)(m_k - m)^T in float64"""
    p = counts / counts.sum()
    m = p @ means
    d = means - m
    return m, (d * p[:, None]).T @ d


def normalize(X):
    """sklearn.preprocessing.normalize (L2, rows; a zero row stays zero) on the device: the scoring kernel's own norm stage
    behind an identity map, so a step-by-step pipeline and the fused call share their arithmetic.  The kernel's limit
    applies: rows wider than 255 columns are refused (ValueError), so a foreign dim_reducer that returns more than 255
    columns cannot be followed by this function."""
    Xd = _as_device(X)
    eye = torch.eye(Xd.shape[1], dtype=torch.float32, device=Xd.device)
    v, _ = backend_score(Xd, eye, flags=nv.BACKEND_L2, want_v=True, want_out=False)
    return _like(v, X)


class _Estimator:
    """fitted state = numpy float64 attributes; fp32 device copies are rebuilt on demand and never pickled"""

    def _dev(self, name, device, make=None):
        cache = self.__dict__.setdefault("_cache", {})
        key = (name, str(device))
        if key not in cache:
            cache[key] = _f32(getattr(self, name) if make is None else make(), device)
        return cache[key]

    def _fitted(self, attr):
        if not hasattr(self, attr):
            raise ValueError("%s is not fitted" % type(self).__name__)

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k != "_cache"}

    def __repr__(self):
        return type(self).__name__ + "()"


# ------------------------------------------------------------------ estimators

class StandardScaler(_Estimator):
    """sklearn.preprocessing.StandardScaler with its defaults: mean_, var_ (biased), scale_ (zero variance -> 1)"""

    def fit(self, X, y=None):
        Xd = _as_device(X)
        if Xd.shape[0] < 1:
            raise ValueError("no rows")
        self.__dict__.pop("_cache", None)
        self.mean_, self.var_ = column_stats(Xd)
        self.scale_ = np.where(self.var_ > 0, np.sqrt(self.var_), 1.0)
        self.n_samples_seen_ = int(Xd.shape[0])
        return self

    def transform(self, X):
        self._fitted("scale_")
        Xd = _as_device(X)
        if Xd.shape[1] != self.mean_.shape[0]:
            raise ValueError("X has %d features, the scaler was fitted on %d" % (Xd.shape[1], self.mean_.shape[0]))
        out = center_rows(Xd, mu=self._dev("mean_", Xd.device), inv_scale=self._dev("inv_scale_", Xd.device, lambda: 1.0 / self.scale_))
        return _like(out, X)

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)


def plda_from_scatter(m, Sb, Sw, n, n_components=None):
    """The float64 part of PLDA.fit: from the mean, the scatter matrices and n = N / K to
    (components C or None, W, A, inv_A, Psi, relevant indices)."""
    import scipy.linalg
    D = Sw.shape[0]
    lam = np.linalg.eigvalsh(Sw)
    # the scatter was summed in fp32: eigenvalues below D eps_fp32 lambda_max are rounding noise, not rank
    rank = int((lam > D * _EPS32 * lam.max()).sum())
    C = None
    if n_components is not None or rank < D:
        ncomp = rank if n_components is None else int(n_components)
        if not 1 <= ncomp <= D:
            raise ValueError("n_components must be 1 .. %d, got %d" % (D, ncomp))
        if ncomp > rank:
            raise ValueError("n_components %d exceeds the rank %d of the within-class scatter" % (ncomp, rank))
        _, vec = np.linalg.eigh(Sw + Sb)
        C = vec[:, ::-1][:, :ncomp]                                 # top eigenvectors of S_t, as PCA's components_.T
        Sb, Sw = C.T @ Sb @ C, C.T @ Sw @ C
        Sb, Sw = 0.5 * (Sb + Sb.T), 0.5 * (Sw + Sw.T)
    try:
        _, W = scipy.linalg.eigh(Sb, Sw)
    except np.linalg.LinAlgError as e:
        raise ValueError("the within-class scatter is singular in the %d dimensions kept; pass a smaller n_components (%s)"
                         % (Sw.shape[0], e)) from e
    Lb = np.diag(W.T @ Sb @ W)
    Lw = np.diag(W.T @ Sw @ W)
    scale = np.sqrt(n / (n - 1.0) * Lw)
    A = np.linalg.inv(W.T) * scale[None, :]
    inv_A = (W / scale[None, :]).T
    Psi = np.maximum(0.0, (n - 1.0) / n * Lb / Lw - 1.0 / n)
    relevant = np.flatnonzero(Psi != 0)
    return C, W, A, inv_A, Psi, relevant


class PLDA(_Estimator):
    """reference sklearn_utils.py:25-36: fit(X, y, n_components=None), transform (D -> U_model), predict -> (pred, logpp)"""

    def fit(self, X, y, n_components=None):
        y, counts = _labels(y, None if not hasattr(X, "shape") else X.shape[0])
        Xd = _as_device(X)
        N, D = Xd.shape
        K = counts.shape[0]
        if K < 2:
            raise ValueError("PLDA needs at least two classes")
        self.__dict__.pop("_cache", None)
        means, Sw, _ = class_statistics(Xd, y)
        m, Sb = between_scatter(means, counts)
        n = N / K
        C, W, A, inv_A, Psi, relevant = plda_from_scatter(m, Sb, Sw, n, n_components)
        if relevant.size == 0:
            raise ValueError("PLDA found no discriminative dimension (every Psi is 0)")
        if relevant.size > 255:
            raise ValueError("U_model has %d dimensions, the scoring kernel takes 255" % relevant.size)
        self.m_, self.pca_components_, self.W_, self.A_, self.inv_A_, self.Psi_ = m, C, W, A, inv_A, Psi
        self.relevant_U_dims_ = relevant
        self.class_counts_ = counts.astype(np.float64)
        self.n_avg_ = n
        # transform(x) = (x - m) P_:  P_ = C inv_A^T restricted to the relevant columns
        T = inv_A.T[:, relevant]
        self.P_ = T if C is None else C @ T
        self.class_means_U_ = (means - m) @ self.P_
        psi = Psi[relevant]
        nk = self.class_counts_[:, None]
        self.pp_mean_ = nk * psi / (1.0 + nk * psi) * self.class_means_U_
        self.pp_var_ = 1.0 + psi / (1.0 + nk * psi)
        return self

    def get_dimensionality(self, space):
        self._fitted("P_")
        d_x = self.A_.shape[0]
        return {"D": self.P_.shape[0], "X": d_x, "U": d_x, "U_model": self.P_.shape[1]}[space]

    def transform(self, X):
        self._fitted("P_")
        Xd = _as_device(X)
        v, _ = backend_score(Xd, self._dev("P_", Xd.device), mu=self._dev("m_", Xd.device), want_v=True, want_out=False)
        return _like(v, X)

    def score_parameters(self):
        """(theta, w, c0) of the posterior predictive as the scoring kernel's class stage, float64"""
        return self.pp_mean_, 1.0 / self.pp_var_, -0.5 * np.log(2.0 * np.pi * self.pp_var_).sum(axis=1)

    def predict(self, X):
        self._fitted("P_")
        Xd = _as_device(X)
        dev = Xd.device
        _, logpp = backend_score(Xd, self._dev("P_", dev), mu=self._dev("m_", dev),
                                 theta=self._dev("_theta", dev, lambda: self.score_parameters()[0]),
                                 w=self._dev("_w", dev, lambda: self.score_parameters()[1]),
                                 c0=self._dev("_c0", dev, lambda: self.score_parameters()[2]))
        return _like(logpp.argmax(dim=1), X), _like(logpp, X)

    def __str__(self):
        """one line in the layout the reference prints: the dimensions of the four spaces and the PCA size"""
        d_in, d_x, d_u, d_model = (self.get_dimensionality(space) for space in ("D", "X", "U", "U_model"))
        n_pca = None if self.pca_components_ is None else self.pca_components_.shape[1]
        return "PLDA: %d -> %d -> %d -> %d (PCA preprocessing with %s coefs)" % (d_in, d_x, d_u, d_model, n_pca)


class GaussianNB(_Estimator):
    """sklearn.naive_bayes.GaussianNB with its defaults: priors n_k/N, var_ += 1e-9 max_r var(X[:, r]).
    Two differences from sklearn: predict_log_proba is the scoring kernel's normalised output, which is clipped at -100
    (sklearn does not clip), and the features pass through the kernel's product stage behind an identity map, so at most
    255 features are taken."""

    var_smoothing = 1e-9

    def fit(self, X, y):
        y, counts = _labels(y, None if not hasattr(X, "shape") else X.shape[0])
        Xd = _as_device(X)
        if Xd.shape[1] > 255:
            raise ValueError("GaussianNB scores at most 255 features on the device, got %d" % Xd.shape[1])
        self.__dict__.pop("_cache", None)
        means, _, (Xs, offsets, offsets_dev, means_dev) = class_statistics(Xd, y, scatter=False)
        sq = center_rows(Xs, cm=means_dev, offsets=offsets_dev, square=True)
        var = _util.segment_mean(sq, offsets).cpu().numpy().astype(np.float64)
        _, colvar = column_stats(Xd)
        self.epsilon_ = self.var_smoothing * colvar.max()
        self.theta_ = means
        self.var_ = var + self.epsilon_
        self.class_count_ = counts.astype(np.float64)
        self.class_prior_ = self.class_count_ / self.class_count_.sum()
        self.classes_ = np.arange(counts.shape[0])
        return self

    def score_parameters(self):
        """(theta, w, c0) of the joint log-likelihood as the scoring kernel's class stage, float64"""
        return self.theta_, 1.0 / self.var_, np.log(self.class_prior_) - 0.5 * np.log(2.0 * np.pi * self.var_).sum(axis=1)

    def predict_log_proba(self, X):
        self._fitted("theta_")
        Xd = _as_device(X)
        dev = Xd.device
        if Xd.shape[1] != self.theta_.shape[1]:
            raise ValueError("X has %d features, the classifier was fitted on %d" % (Xd.shape[1], self.theta_.shape[1]))
        eye = torch.eye(Xd.shape[1], dtype=torch.float32, device=dev)
        _, out = backend_score(Xd, eye, theta=self._dev("theta_", dev), w=self._dev("_w", dev, lambda: self.score_parameters()[1]),
                               c0=self._dev("_c0", dev, lambda: self.score_parameters()[2]), flags=nv.BACKEND_NORMALISED)
        return _like(out, X)

    def predict(self, X):
        Xd = _as_device(X)
        return _like(self.predict_log_proba(Xd).argmax(dim=1), X)


class LinearDiscriminantAnalysis(_Estimator):
    """sklearn.discriminant_analysis.LinearDiscriminantAnalysis, priors n_k/N, no shrinkage:
        coef_ = Sigma^-1 m_k,   intercept_ = -1/2 m_k^T Sigma^-1 m_k + log prior
    Sigma is the pooled within-class covariance.  solver="svd" (sklearn's default, what the reference's fit_lda builds)
    divides the pooled scatter by N - K, "lsqr" / "eigen" by N (prior-weighted biased class covariances); the solvers'
    log-probabilities differ by exactly that factor on the scores.  coef_ / intercept_ are kept in the uncentred form for
    every solver.  The device never sees them: every class's uncentred score carries the same term x^T Sigma^-1 xbar, which
    on rows far from the origin is 10^4 times the class-specific part and would eat fp32's digits.  Scoring
    (lidbox_backend_score in its LINEAR mode) uses the centred discriminant
        u_k = (x - xbar_) . Sigma^-1 (m_k - xbar_) - 1/2 (m_k - xbar_)^T Sigma^-1 (m_k - xbar_) + log prior_k
    (coef_centred_, intercept_centred_), which differs from the uncentred one by a number that is the same for all
    classes and so gives the same log-softmax.  predict_log_proba is the kernel's normalised output and is clipped at -100,
    which sklearn's is not."""

    def __init__(self, solver="svd"):
        if solver not in ("svd", "lsqr", "eigen"):
            raise ValueError("unknown solver %r" % (solver,))
        self.solver = solver

    def fit(self, X, y):
        y, counts = _labels(y, None if not hasattr(X, "shape") else X.shape[0])
        Xd = _as_device(X)
        N, D = Xd.shape
        K = counts.shape[0]
        if K < 2:
            raise ValueError("LinearDiscriminantAnalysis needs at least two classes")
        if K > 255:
            raise ValueError("the scoring kernel takes at most 255 classes in its linear mode, got %d" % K)
        self.__dict__.pop("_cache", None)
        means, Sw, _ = class_statistics(Xd, y)
        self.means_ = means
        self.priors_ = counts / counts.sum()
        self.xbar_ = self.priors_ @ means
        self.covariance_ = Sw * (N / (N - K)) if self.solver == "svd" else Sw
        self.coef_, self.intercept_ = lda_from_moments(means, self.covariance_, self.priors_)
        self.coef_centred_, self.intercept_centred_ = lda_from_moments(means - self.xbar_, self.covariance_, self.priors_)
        self.classes_ = np.arange(K)
        return self

    def predict_log_proba(self, X):
        self._fitted("coef_centred_")
        Xd = _as_device(X)
        dev = Xd.device
        _, out = backend_score(Xd, self._dev("_P", dev, lambda: self.coef_centred_.T), mu=self._dev("xbar_", dev),
                               q=self._dev("intercept_centred_", dev), flags=nv.BACKEND_NORMALISED | nv.BACKEND_LINEAR)
        return _like(out, X)

    def predict(self, X):
        Xd = _as_device(X)
        return _like(self.predict_log_proba(Xd).argmax(dim=1), X)

    def __repr__(self):
        return "LinearDiscriminantAnalysis(solver=%r)" % self.solver


def lda_from_moments(means, cov, priors):
    """coef [K, D] = Sigma^-1 m_k and intercept [K] = -1/2 m_k . coef_k + log prior_k in float64, for class means given
    relative to any origin"""
    lam = np.linalg.eigvalsh(cov)
    if lam.min() <= cov.shape[0] * _EPS32 * lam.max():
        raise ValueError("the within-class covariance is singular at fp32 precision; reduce the dimensions first")
    coef = np.linalg.solve(cov, means.T).T
    return coef, -0.5 * (means * coef).sum(axis=1) + np.log(priors)


# ------------------------------------------------------------------ the reference's functions (names and signatures)

def _shape(a):
    return "x".join(str(n) for n in np.shape(a)) or "scalar"


def _sparse_cross_entropy(logits, y):
    """mean over rows of -log_softmax(logits)[y]: lidbox_log_softmax_fwd + lidbox_nll_fwd_bwd"""
    rows, classes = logits.shape
    logp = torch.empty_like(logits)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        nv.check(nv.lib.lidbox_log_softmax_fwd(_ptr(logits), rows, classes, _ptr(logp), nv.current_stream()))
        nv.check(nv.lib.lidbox_nll_fwd_bwd(_ptr(logp), nv.C.c_void_p(y.data_ptr()), rows, classes, 1.0 / rows, _ptr(loss), None,
                                           nv.current_stream()))
    return float(loss)


def get_lda_scores(lda, test):
    """(accuracy, cross-entropy) of a fitted PLDA or LDA on test = {"X", "y"}.  The scores are treated as logits of a sparse
    categorical cross-entropy, averaged over the rows, as the reference's Keras loss does; a PLDA's scores are the
    unnormalised log-densities of its predict, anything else gives predict / predict_log_proba."""
    Xd = _as_device(test["X"])
    if isinstance(lda, PLDA):
        decided, scores = lda.predict(Xd)
    else:
        scores = lda.predict_log_proba(Xd)
        decided = lda.predict(Xd)
    truth = torch.as_tensor(np.asarray(test["y"]) if not isinstance(test["y"], torch.Tensor) else test["y"])
    truth = truth.to(device=Xd.device, dtype=torch.int32).contiguous()
    scores = _as_device(scores, "scores").contiguous()
    decided = torch.as_tensor(decided).to(device=Xd.device, dtype=torch.int32)
    accuracy = float((decided == truth).float().mean())
    return accuracy, _sparse_cross_entropy(scores, truth)


def _log_fit_result(model, test):
    accuracy, cce = get_lda_scores(model, test)
    logger.info("%s fitted: held-out accuracy %.3f, cross-entropy %.3f", model, accuracy, cce)


def fit_lda(train, test):
    """LinearDiscriminantAnalysis (sklearn's default solver) fitted on train, scored on test for the log"""
    logger.info("LDA: fitting on %s rows, labels %s", _shape(train["X"]), _shape(train["y"]))
    lda = LinearDiscriminantAnalysis().fit(train["X"], train["y"])
    _log_fit_result(lda, test)
    return lda


def fit_plda(train, test, n_components=None):
    """PLDA fitted on train (PCA to n_components first; None keeps every dimension the within-class scatter has rank
    for), scored on test for the log.  The reference passes a keyword PLDA.fit does not have; this is its evident intent."""
    logger.info("PLDA: fitting on %s rows, labels %s, PCA components: %s", _shape(train["X"]), _shape(train["y"]),
                "rank of the within-class scatter" if n_components is None else n_components)
    plda = PLDA().fit(train["X"], train["y"], n_components=n_components)
    _log_fit_result(plda, test)
    return plda


def fit_plda_gridsearch(train, test, grid):
    """one PLDA per PCA size in grid; the one with the lowest held-out cross-entropy is returned (the first on a tie)"""
    logger.info("PLDA grid search over %d PCA sizes: %s", len(grid), list(grid))
    candidates = []
    for n_components in grid:
        plda = fit_plda(train, test, n_components=n_components)
        candidates.append((get_lda_scores(plda, test)[1], plda))
    losses = [loss for loss, _ in candidates]
    winner = int(np.argmin(losses)) if len(losses) else None
    if winner is None:
        return None
    logger.info("PLDA grid search: %s wins with cross-entropy %.3f", candidates[winner][1], losses[winner])
    return candidates[winner][1]


def reduce_dimensions(train, test, dim_reducer):
    """replaces X of both splits, in place, by dim_reducer.transform(X)"""
    for split in (train, test):
        before = _shape(split["X"])
        split["X"] = dim_reducer.transform(split["X"])
        logger.info("%s: %s -> %s", dim_reducer, before, _shape(split["X"]))


def draw_random_sample(train, test, labels, target2label, sample_size=100):
    """{"train": {label: rows}, "test": {label: rows}} with `sample_size` rows per label drawn without replacement (numpy's
    global generator); labels in sorted order, the rows gathered where X lives"""
    logger.info("sampling %d rows per label (%d labels) from train %s and test %s", sample_size, len(labels),
                _shape(train["X"]), _shape(test["X"]))
    wanted = sorted(labels)

    def sample(data):
        X = data["X"]
        y = data["y"].detach().cpu().numpy() if isinstance(data["y"], torch.Tensor) else np.asarray(data["y"])
        drawn = {}
        for target in np.unique(y):
            members = np.flatnonzero(y == target)
            picked = members[np.random.choice(members.shape[0], size=sample_size, replace=False)]
            drawn[target2label[target]] = X[torch.from_numpy(picked).to(X.device)] if isinstance(X, torch.Tensor) else X[picked]
        return collections.OrderedDict((label, drawn[label]) for label in wanted if label in drawn)
    return {"train": sample(train), "test": sample(test)}


def fit_classifier(train, test, labels, config, target2label, Classifier, n_plda_coefs=None, plot_demo=True):
    """scaler -> PLDA (n_plda_coefs PCA components) -> L2 normalisation -> Classifier(), each fitted on the device on what
    the stage before it produced.  train["X"] / test["X"] end up as the normalised U_model vectors, as the reference leaves
    them.  Returns {"scaler", "dim_reducer", "classifier"}."""
    scaler = StandardScaler().fit(train["X"])
    logger.info("scaler fitted on %s", _shape(train["X"]))
    for split in (train, test):
        split["X"] = scaler.transform(split["X"])
    plda = fit_plda(train, test, n_plda_coefs)
    reduce_dimensions(train, test, plda)
    for split in (train, test):
        split["X"] = normalize(split["X"])
    if plot_demo:
        logger.warning("The embedding demo figures (plot_embedding_demo) are not built in lidbox_amd; nothing is drawn, "
                       "the pipeline is fitted as it is.")
    classifier = Classifier()
    classifier.fit(X=train["X"], y=train["y"])
    logger.info("%s fitted on unit-length vectors %s", classifier, _shape(train["X"]))
    return dict(scaler=scaler, dim_reducer=plda, classifier=classifier)


def fused_parameters(pipeline):
    """mu, P, q, theta, w, c0 (float64) of the one lidbox_backend_score call that equals
    scaler.transform -> dim_reducer.transform -> normalize -> classifier.predict_log_proba for this module's
    StandardScaler (optional), PLDA and GaussianNB; None for any other pipeline.
        ((x - mean) / scale - m) P  =  (x - (mean + scale m)) (P / scale)
    so the scaler's 1 / scale goes into P in float64 and the two means stay one subtraction at load time."""
    scaler, plda, nb = pipeline.get("scaler"), pipeline.get("dim_reducer"), pipeline.get("classifier")
    if not (isinstance(plda, PLDA) and isinstance(nb, GaussianNB) and (scaler is None or isinstance(scaler, StandardScaler))):
        return None
    mu, P = plda.m_, plda.P_
    if scaler is not None:
        mu = scaler.mean_ + scaler.scale_ * plda.m_
        P = plda.P_ / scaler.scale_[:, None]
    theta, w, c0 = nb.score_parameters()
    return dict(mu=mu, P=P, q=np.zeros(P.shape[1]), theta=theta, w=w, c0=c0)


def predict_with_trained_classifier(unlabeled, config, target2label, pipeline):
    """log-probabilities, floored at -100, of unlabeled["X"] under a pipeline from fit_classifier / pipeline_from_disk.
    A pipeline of this module's scaler, PLDA and GaussianNB is ONE lidbox_backend_score call per row block.  Anything else
    runs stage by stage through the objects' own methods: the optional "scaler" and "dim_reducer" entries, this module's
    normalize (at most 255 columns), then the classifier's predict_log_proba."""
    X = unlabeled["X"]
    fused = fused_parameters(pipeline)
    if fused is not None:
        Xd = _as_device(X)
        p = {k: _f32(a, Xd.device) for k, a in fused.items()}      # a few D x R arrays: composed once per call
        logger.info("scoring %s in one fused scaler -> PLDA -> normalise -> %s pass", _shape(Xd), pipeline["classifier"])
        _, out = backend_score(Xd, p["P"], mu=p["mu"], q=p["q"], theta=p["theta"], w=p["w"], c0=p["c0"],
                               flags=nv.BACKEND_L2 | nv.BACKEND_NORMALISED)
        return _like(out, X)
    for stage in ("scaler", "dim_reducer"):
        if stage in pipeline:
            X = pipeline[stage].transform(X)
            logger.info("stage %s (%s) gave %s", stage, pipeline[stage], _shape(X))
    log_proba = pipeline["classifier"].predict_log_proba(normalize(X))
    logger.info("%s scored %s rows", pipeline["classifier"], len(log_proba))
    floor = -100.0
    return torch.clamp_min(log_proba, floor) if isinstance(log_proba, torch.Tensor) else np.maximum(log_proba, floor)


_JOBLIB_SUFFIX = ".joblib"


def joblib_dir_from_config(config):
    """<cache_directory>/<model key>/<experiment name>/sklearn_objects of the config's sklearn_experiment section"""
    experiment = config["sklearn_experiment"]
    return os.path.join(experiment["cache_directory"], experiment["model"]["key"], experiment["name"], "sklearn_objects")


def pipeline_to_disk(config, sklearn_objects):
    """one <key>.joblib per pipeline entry under joblib_dir_from_config(config); returns that directory"""
    import joblib
    target = joblib_dir_from_config(config)
    os.makedirs(target, exist_ok=True)
    for key in sklearn_objects:
        path = os.path.join(target, key + _JOBLIB_SUFFIX)
        joblib.dump(sklearn_objects[key], path)
        logger.info("pipeline entry %s (%s) saved as %s", key, sklearn_objects[key], path)
    return target


def pipeline_from_disk(config):
    """{key: object} of every <key>.joblib under joblib_dir_from_config(config); an empty dict, with an error in the log,
    when the directory is missing"""
    import joblib
    source = joblib_dir_from_config(config)
    if not os.path.isdir(source):
        logger.error("no pipeline to load: %s is not a directory", source)
        return {}
    names = sorted(n for n in os.listdir(source) if n.endswith(_JOBLIB_SUFFIX))
    logger.info("loading %d pipeline entries from %s", len(names), source)
    return {n[:-len(_JOBLIB_SUFFIX)]: joblib.load(os.path.join(source, n)) for n in names}
