"""
The embedding back-end (lidbox_amd/embed/sklearn_utils.py) without a device: the float64 restatement that the GPU tests use
as their oracle (tests/backend_ref.py) is pinned by algebraic properties and by scikit-learn, the planted-data generator is
pinned by the U_model dimensions it yields, and the host layer's float64 parts (the PLDA solve, the composition of the fused
call's parameters, pickling, the refusals) are checked directly.  The `plda` package the reference builds on is not
available: parity with it is unpinned (docs/TRACEABILITY.md 8(f)).
"""
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import backend_ref as br


@pytest.fixture(scope="module")
def nv():
    from lidbox_amd import build
    build.build(verbose=False)
    from lidbox_amd import _native
    return _native


@pytest.fixture(scope="module")
def su(nv):
    from lidbox_amd.embed import sklearn_utils
    return sklearn_utils


@functools.lru_cache(maxsize=None)
def _raw_fit(i):
    Xtr, ytr, _, _ = br.planted(*br.CASES[i])
    return br.plda_fit_data(Xtr, ytr)


@functools.lru_cache(maxsize=None)
def _pipeline(i):
    Xtr, ytr, _, _ = br.planted(*br.CASES[i])
    return br.pipeline_fit(Xtr, ytr)


def _offdiag(M):
    return np.abs(M - np.diag(np.diag(M))).max()


@pytest.mark.parametrize("i", range(len(br.CASES)))
def test_plda_restatement_algebra(i):
    f = _raw_fit(i)
    W, A, Sb, Sw, n = f["W"], f["A"], f["Sb"], f["Sw"], f["n"]
    # only the D = 512 case has eigenvalues of S_w below D eps_fp32 lambda_max (two: 0.008 and 0.50 of the threshold, the next
    # is 1.8) and takes the PCA branch with 510 components; the identities then hold for the projected scatter matrices
    assert (f["C"] is None) == (i != 3) and f["rank"] == (510 if i == 3 else Sw.shape[0])
    sw, sb = np.abs(Sw).max(), np.abs(Sb).max()
    assert _offdiag(W.T @ Sw @ W) <= 1e-9 and _offdiag(W.T @ Sb @ W) <= 1e-9 * max(1.0, sb / sw)
    assert np.abs(A @ A.T - n / (n - 1.0) * Sw).max() <= 1e-9 * sw
    assert np.abs((A * f["psi_raw"][None, :]) @ A.T - (Sb - Sw / (n - 1.0))).max() <= 1e-9 * max(sw, sb)
    assert np.abs(f["inv_A"] @ A - np.eye(A.shape[0])).max() <= 1e-8
    assert (f["Psi"] >= 0).all() and f["relevant"].size <= f["counts"].shape[0] - 1


@pytest.mark.parametrize("i", range(len(br.CASES)))
def test_plda_span_is_sklearn_eigen_lda_span(i):
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    Xtr, ytr, _, _ = br.planted(*br.CASES[i])
    f = _raw_fit(i)
    R = f["relevant"].size
    X = Xtr.astype(np.float64)
    if f["C"] is not None:                                          # the model lives in the PCA space
        X = (X - f["m"]) @ f["C"]
    sk = LinearDiscriminantAnalysis(solver="eigen").fit(X, ytr)
    cos = br.min_principal_cosine(f["W"][:, f["relevant"]], sk.scalings_[:, :R])
    print("case %d: R = %d, smallest principal-angle cosine = 1 - %.1e" % (i, R, 1 - cos))
    assert cos >= 1 - 1e-9


def test_planted_generator_is_pinned_by_its_model_dimensions():
    """R of the float64 pipeline (scaler -> PLDA) on the five cases, and that the held-out rows are classifiable at all"""
    for i, case in enumerate(br.CASES):
        p = _pipeline(i)
        assert p["plda"]["relevant"].size == br.EXPECTED_R[i], (case, p["plda"]["relevant"].size)
        _, _, Xte, yte = br.planted(*case)
        logp = br.pipeline_steps(p, Xte)[3]
        acc = (logp.argmax(axis=1) == yte).mean()
        print("case %d: R = %d, held-out accuracy %.3f" % (i, br.EXPECTED_R[i], acc))
        assert acc >= 0.7 and logp.max() <= 0 and logp.min() >= -100


@pytest.mark.parametrize("nc", [5, 32])
def test_pca_branch_is_sklearn_pca_up_to_sign(nc):
    from sklearn.decomposition import PCA
    Xtr, ytr, _, _ = br.planted(*br.CASES[0])
    X = Xtr.astype(np.float64)
    f = br.plda_fit_data(X, ytr, n_components=nc)
    sk = PCA(n_components=nc, svd_solver="full").fit(X)
    assert f["C"].shape == (64, nc)
    assert np.abs(np.abs(f["C"].T @ sk.components_.T) - np.eye(nc)).max() <= 1e-8
    assert np.abs(f["m"] - sk.mean_).max() <= 1e-12                          # m = sum_k n_k/N m_k is the mean of the rows
    assert f["relevant"].size <= min(nc, 9)
    # after the PCA the model is the full-rank model of the projected rows
    g = br.plda_fit_data((X - f["m"]) @ f["C"], ytr)
    assert br.min_principal_cosine(f["P"], f["C"] @ g["P"]) >= 1 - 1e-9


def test_rank_deficient_scatter_takes_the_pca_branch():
    """8 of 40 columns are exact copies: rank 32 is found at the fp32 tolerance and R is that of the 32 free columns"""
    Xtr, ytr, _, _ = br.planted(2000, 32, 10, 0.15, 0)
    X = np.concatenate([Xtr, Xtr[:, :8]], axis=1).astype(np.float64)
    f = br.plda_fit_data(X, ytr)
    g = br.plda_fit_data(Xtr.astype(np.float64), ytr)
    assert f["rank"] == 32 and f["C"].shape == (40, 32)
    assert f["relevant"].size == g["relevant"].size == 9
    for f32 in (False, True):
        assert br.plda_fit_data(X, ytr, f32=f32)["rank"] == 32


@pytest.mark.parametrize("i", [0, 1, 4])
def test_restated_naive_bayes_and_lda_equal_sklearn(i):
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    from sklearn.naive_bayes import GaussianNB
    Xtr, ytr, Xte, _ = br.planted(*br.CASES[i])
    p = _pipeline(i)
    Vtr, Vte = br.pipeline_steps(p, Xtr)[2], br.pipeline_steps(p, Xte)[2]
    sk = GaussianNB().fit(Vtr, ytr)
    theta, var, prior = br.nb_fit(Vtr, ytr)
    assert np.abs(var - sk.var_).max() <= 1e-12 and np.abs(theta - sk.theta_).max() <= 1e-12
    assert np.abs(br.nb_log_proba(Vte, theta, var, prior) - sk.predict_log_proba(Vte)).max() <= 1e-10
    X, Xt = Xtr.astype(np.float64), Xte.astype(np.float64)
    # sklearn's lsqr / eigen solvers evaluate coef x + intercept uncentred: on the rows offset by 50 their own output
    # cancels to about 1e-9, so there only the svd solver (which centres, and is the reference's default) is a 1e-10 pin
    for solver, unbiased in (("svd", True), ("lsqr", False), ("eigen", False))[:1 if i == 4 else 3]:
        sk = LinearDiscriminantAnalysis(solver=solver).fit(X, ytr)
        err = np.abs(br.lda_log_proba(Xt, *br.lda_fit(X, ytr, unbiased)) - sk.predict_log_proba(Xt)).max()
        print("case %d LDA %s: %.1e" % (i, solver, err))
        assert err <= 1e-10, solver


def _fitted_objects(su, i):
    """this module's estimators carrying the float64 restatement's state (no device involved)"""
    p = _pipeline(i)
    f = p["plda"]
    scaler, plda, nb = su.StandardScaler(), su.PLDA(), su.GaussianNB()
    scaler.mean_, scaler.scale_, scaler.var_ = p["mean"], p["scale"], p["scale"] ** 2
    plda.m_, plda.P_, plda.A_, plda.pca_components_ = f["m"], f["P"], f["A"], f["C"]
    theta_pp, var_pp = br.plda_predictive(f)
    plda.pp_mean_, plda.pp_var_ = theta_pp, var_pp
    nb.theta_, nb.var_, nb.class_prior_ = p["theta"], p["var"], p["prior"]
    return dict(scaler=scaler, dim_reducer=plda, classifier=nb)


@pytest.mark.parametrize("i", [0, 1, 2, 4])
def test_fused_parameters_reproduce_the_step_by_step_pipeline(su, i):
    _, _, Xte, _ = br.planted(*br.CASES[i])
    pipe = _fitted_objects(su, i)
    fp = su.fused_parameters(pipe)
    assert sorted(fp) == ["P", "c0", "mu", "q", "theta", "w"] and all(a.dtype == np.float64 for a in fp.values())
    o = br.score_oracle(Xte, fp["mu"], fp["P"], fp["q"], fp["theta"], fp["w"], fp["c0"], br.L2 | br.NORMALISED)
    _, Um, V, logp = br.pipeline_steps(_pipeline(i), Xte)
    scale = np.abs(Um).max()
    assert np.abs(o["u"] - Um).max() <= 1e-9 * max(1.0, scale)               # off = 50: (x - 50) terms of size 1, not 50
    assert np.abs(o["v"] - V).max() <= 1e-9
    assert np.abs(o["out"] - logp).max() <= 1e-8
    # without the scaler the PLDA's own mean and map are passed through
    fp2 = su.fused_parameters(dict(dim_reducer=pipe["dim_reducer"], classifier=pipe["classifier"]))
    assert fp2["mu"] is pipe["dim_reducer"].m_ and fp2["P"] is pipe["dim_reducer"].P_
    # any foreign object: no fused call
    assert su.fused_parameters(dict(scaler=object(), dim_reducer=pipe["dim_reducer"], classifier=pipe["classifier"])) is None
    assert su.fused_parameters(dict(dim_reducer=pipe["dim_reducer"], classifier=object())) is None


@pytest.mark.parametrize("i,nc", [(0, None), (1, None), (2, None), (0, 5), (0, 32)])
def test_host_plda_solve_is_the_restatement(su, i, nc):
    Xtr, ytr, _, _ = br.planted(*br.CASES[i])
    f = br.plda_fit_data(Xtr, ytr, n_components=nc)
    C, W, A, inv_A, Psi, rel = su.plda_from_scatter(f["m"], f["Sb_D"], f["Sw_D"], f["n"], nc)
    assert (C is None) == (f["C"] is None) and np.array_equal(rel, f["relevant"])
    T = inv_A.T[:, rel]
    P = T if C is None else C @ T
    assert br.min_principal_cosine(P, f["P"]) >= 1 - 1e-12
    assert np.abs(np.abs(P) - np.abs(f["P"])).max() <= 1e-9 * np.abs(f["P"]).max()
    assert np.abs(Psi - f["Psi"]).max() <= 1e-9 * f["Psi"].max()
    m, Sb = su.between_scatter(f["means"], f["counts"])
    assert np.abs(m - f["m"]).max() <= 1e-13 * max(1.0, np.abs(f["m"]).max()) and np.abs(Sb - f["Sb_D"]).max() <= 1e-12
    with pytest.raises(ValueError):
        su.plda_from_scatter(f["m"], f["Sb_D"], f["Sw_D"], f["n"], f["Sw_D"].shape[0] + 1)


def test_host_lda_solve_is_the_restatement(su):
    Xtr, ytr, _, _ = br.planted(*br.CASES[1])
    means, Sw, counts = br.class_stats(Xtr, ytr)
    coef, icpt = su.lda_from_moments(means, Sw, counts / counts.sum())
    assert coef.shape == (3, 7) and icpt.shape == (3,)
    _, _, Xte, _ = br.planted(*br.CASES[1])
    ref = br.lda_log_proba(Xte, *br.lda_fit(Xtr, ytr, unbiased=False))
    assert np.abs(br.lda_log_proba(Xte, coef, icpt) - ref).max() <= 1e-10         # uncentred form, same log-probabilities
    with pytest.raises(ValueError):
        su.lda_from_moments(means, np.ones_like(Sw), counts / counts.sum())


def test_reference_names_and_signatures(su):
    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    E = inspect.Parameter.empty
    assert params(su.PLDA.fit) == [("self", E), ("X", E), ("y", E), ("n_components", None)]
    assert params(su.PLDA.transform) == [("self", E), ("X", E)]
    assert params(su.get_lda_scores) == [("lda", E), ("test", E)]
    assert params(su.fit_lda) == [("train", E), ("test", E)]
    assert params(su.fit_plda) == [("train", E), ("test", E), ("n_components", None)]
    assert params(su.fit_plda_gridsearch) == [("train", E), ("test", E), ("grid", E)]
    assert params(su.reduce_dimensions) == [("train", E), ("test", E), ("dim_reducer", E)]
    assert params(su.draw_random_sample) == [("train", E), ("test", E), ("labels", E), ("target2label", E), ("sample_size", 100)]
    assert params(su.fit_classifier) == [("train", E), ("test", E), ("labels", E), ("config", E), ("target2label", E),
                                         ("Classifier", E), ("n_plda_coefs", None), ("plot_demo", True)]
    assert params(su.predict_with_trained_classifier) == [("unlabeled", E), ("config", E), ("target2label", E), ("pipeline", E)]
    for name in ("joblib_dir_from_config", "pipeline_to_disk", "pipeline_from_disk"):
        assert callable(getattr(su, name))
    for cls, methods in ((su.StandardScaler, ("fit", "transform")), (su.PLDA, ("fit", "transform", "predict", "__str__")),
                         (su.GaussianNB, ("fit", "predict", "predict_log_proba")),
                         (su.LinearDiscriminantAnalysis, ("fit", "predict", "predict_log_proba"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    import lidbox_amd.embed
    assert lidbox_amd.embed.sklearn_utils is su
    plda = _fitted_objects(su, 0)["dim_reducer"]
    assert str(plda) == "PLDA: 64 -> 64 -> 64 -> 9 (PCA preprocessing with None coefs)"


CONFIG = lambda d: {"sklearn_experiment": {"cache_directory": str(d), "model": {"key": "xvector"}, "name": "nb"}}   # noqa: E731


def test_joblib_round_trip(su, tmp_path):
    import joblib
    pipe = _fitted_objects(su, 1)
    lda = su.LinearDiscriminantAnalysis()
    lda.coef_, lda.intercept_ = np.arange(6.0).reshape(2, 3), np.arange(2.0)
    for name, obj in list(pipe.items()) + [("lda", lda)]:
        obj._cache = {("poison", "cuda:0"): lambda: None}           # device copies are never pickled (a lambda cannot be)
        path = tmp_path / (name + ".joblib")
        joblib.dump(obj, path)
        back = joblib.load(path)
        assert type(back) is type(obj) and "_cache" not in back.__dict__
        state = {k: v for k, v in obj.__dict__.items() if k != "_cache"}
        assert sorted(back.__dict__) == sorted(state)
        for k, v in state.items():
            if isinstance(v, np.ndarray):
                assert back.__dict__[k].dtype == np.float64 and np.array_equal(back.__dict__[k], v), k
            else:
                assert back.__dict__[k] == v or (v is None and back.__dict__[k] is None), k
    cfg = CONFIG(tmp_path)
    d = su.pipeline_to_disk(cfg, pipe)
    assert d == su.joblib_dir_from_config(cfg) == os.path.join(str(tmp_path), "xvector", "nb", "sklearn_objects")
    assert sorted(os.listdir(d)) == ["classifier.joblib", "dim_reducer.joblib", "scaler.joblib"]
    back = su.pipeline_from_disk(cfg)
    assert sorted(back) == sorted(pipe)
    a, b = su.fused_parameters(pipe), su.fused_parameters(back)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert su.pipeline_from_disk(CONFIG(tmp_path / "missing")) == {}


def test_kernel_refuses_sizes_outside_its_limits(nv):
    score = nv.lib.lidbox_backend_score

    def call(N=1, D=4, R=2, K=3, flags=0, ldx=None, ldv=None, ldo=None, cls=True, v=True, out=True):
        one = 16                                                    # never dereferenced: every refusal precedes the launch
        th = one if cls else None
        return score(one, N, D, D if ldx is None else ldx, None, one, None, R, th, th, th, K, flags, one if v else None,
                     R if ldv is None else ldv, one if out else None, K if ldo is None else ldo, None)
    for bad in (dict(D=0), dict(D=4097), dict(R=0), dict(R=256), dict(K=0), dict(K=257), dict(N=-1), dict(N=nv.BACKEND_MAX_ROWS + 1),
                dict(ldx=3), dict(ldv=1), dict(ldo=2), dict(flags=8), dict(cls=False, v=False), dict(out=False),
                dict(flags=nv.BACKEND_LINEAR), dict(flags=nv.BACKEND_LINEAR, cls=False, K=3, R=2)):
        assert call(**bad) == -1, bad
        assert "lidbox_backend_score" in nv.last_error()
    with pytest.raises(ValueError):
        nv.check(call(R=256))
    assert call(N=0) == 0 and call(N=0, D=4096, R=255, K=256) == 0                     # N = 0: validated, then a no-op
    center = nv.lib.lidbox_backend_center_rows
    assert center(16, 1, 0, 4, None, None, None, None, 0, 0, 16, 4, None) == -1
    assert center(16, 1, 4, 3, None, None, None, None, 0, 0, 16, 4, None) == -1
    assert center(16, 1, 4, 4, None, None, 16, None, 0, 0, 16, 4, None) == -1          # class means without offsets
    assert center(16, 0, 4, 4, None, None, None, None, 0, 0, 16, 4, None) == 0


def test_host_layer_refusals(su, nv):
    X = torch.zeros(6, 3)
    for Est in (su.PLDA, su.GaussianNB, su.LinearDiscriminantAnalysis):
        for y in ([0, 2, 2, 0, 2, 0], [1, 1, 2, 2, 1, 2], [0, 0, -1, -1, 0, 0], [0.5, 0, 0, 1, 1, 1]):     # not 0 .. K-1
            with pytest.raises(ValueError, match="labels"):
                Est().fit(X, y)
        with pytest.raises(ValueError, match="two rows"):
            Est().fit(X, [0, 0, 0, 1, 1, 2])
        with pytest.raises(ValueError):
            Est().fit(X, [0, 1, 0, 1])                                                  # one label per row
        with pytest.raises(nv.LidboxHipError, match="HIP device only"):
            Est().fit(X, [0, 0, 0, 1, 1, 1])                                            # a CPU tensor
    with pytest.raises(nv.LidboxHipError):
        su.StandardScaler().fit(X)
    with pytest.raises(nv.LidboxHipError):
        su.normalize(X)
    with pytest.raises(ValueError, match="not fitted"):
        su.PLDA().transform(X)
    pipe = _fitted_objects(su, 1)
    with pytest.raises(nv.LidboxHipError):
        su.predict_with_trained_classifier({"X": torch.zeros(4, 7)}, {}, {}, pipe)
    with pytest.raises(nv.LidboxHipError):
        su.get_lda_scores(pipe["dim_reducer"], {"X": torch.zeros(4, 7), "y": np.zeros(4, np.int64)})
    if not torch.cuda.is_available():
        with pytest.raises(nv.LidboxHipError, match="no device"):
            su.StandardScaler().fit(np.zeros((6, 3), np.float32))
    with pytest.raises(ValueError):
        su.LinearDiscriminantAnalysis(solver="qr")


def test_library_binds_the_backend_symbols(nv):
    assert {"lidbox_backend_score", "lidbox_backend_center_rows"} <= set(nv._SIGS)
    assert (nv.BACKEND_L2, nv.BACKEND_NORMALISED, nv.BACKEND_LINEAR) == (br.L2, br.NORMALISED, br.LINEAR)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lidbox_hip.h")).read()
    assert "#define LIDBOX_BACKEND_MAX_ROWS    (1L << 22)" in text and nv.BACKEND_MAX_ROWS == 1 << 22


def test_backend_kernels_build_for_gfx950_without_scratch(nv, tmp_path):
    """all 16 instantiations of the scoring kernel (one per accumulator-tile count) and both centring kernels keep their
    state in registers, and the widest scoring tile fits the 64 KiB of LDS a workgroup may declare"""
    import re
    import subprocess
    from lidbox_amd import build
    cmd = [build.HIPCC] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "backend.hip"),
                                         "-o", str(tmp_path / "backend.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--offload-arch=gfx950" in cmd
    scratch, lds, name = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    score = [k for k in scratch if "backend_score_kernel" in k]
    center = [k for k in scratch if "backend_center_rows_kernel" in k]
    assert len(score) == 16 and len(center) == 2, sorted(scratch)
    assert all(scratch[k] == 0 for k in score + center), scratch
    assert max(lds[k] for k in score) == 65536 and all(lds[k] == 0 for k in center)
