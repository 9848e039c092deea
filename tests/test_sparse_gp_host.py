"""Sparse GP regression, the parts that need no GPU: sr_gp_fit_sparse / sr_gp_is_sparse are declared, exported and bound;
the fp64 NumPy restatement of the DTC formulas (tests/_sparse_ref.py, on the oracle's kernels) agrees with their long-double
evaluation and collapses to the exact GP for Z_u = X; train / update_model handle do_sparse_gp as documented (library calls
monkeypatched)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _sparse_ref as R
from oracle import oracle_np as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_sparse_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in ("sr_gp_fit_sparse", "sr_gp_is_sparse"):
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export " + name
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_fit_sparse\(sr_gp_t h, const double\* X, const double\* Y, long N, double jitter, "
                     r"void\* stream, int\* info\);", hdr)
    assert "int sr_gp_is_sparse(sr_gp_t h);" in hdr
    from safe_exploration_amd import _lib
    restype, args = _lib.SIGNATURES["sr_gp_fit_sparse"]
    assert restype is ctypes.c_int and args == [_lib._H, _lib._P, _lib._P, _lib._L, _lib._D, _lib._P, _lib._PI]
    assert _lib.SIGNATURES["sr_gp_is_sparse"] == (ctypes.c_int, [_lib._H])
    # argument checks that need no device
    info = (ctypes.c_int * 2)()
    assert _lib.lib.sr_gp_fit_sparse(None, None, None, 10, 1e-6, None, info) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_is_sparse(None) == _lib.SR_EINVAL


@pytest.mark.parametrize("kern", ["rbf", "mat52", "lin_rbf", "lin_mat52"])
def test_long_double_kernels_restate_the_oracle(kern):
    case = R.make_case(3, kern, 2, 3, 24, 200)
    for d in range(2):
        k64 = orc.kernel_matrix(kern, case["hyp"][d], case["xq"], case["Zu"])
        kld = R.kernel_matrix_ld(kern, case["hyp"][d], case["xq"], case["Zu"])
        # the oracle's distances come from |x|^2 + |y|^2 - 2 x.y: r^2 carries an absolute rounding error of a few eps |x / l|^2
        # (|x / l|^2 up to 1e4 for the lin_* cases' lengthscale of 0.02), the kernel value that much relative to its maximum
        np.testing.assert_allclose(k64, kld.astype(np.float64), rtol=0, atol=1e-11 * float(np.abs(k64).max()))
        np.testing.assert_allclose(orc.kernel_diag(kern, case["hyp"][d], case["xq"]),
                                   R.kernel_diag_ld(kern, case["hyp"][d], case["xq"]).astype(np.float64), rtol=1e-14)


def test_numpy_restatement_against_long_double():
    """N = 3000, m = 96, D = 3: the figures the tolerances of the device test are built on (cond K_uu ~ 1e5, variance
    error ~ 1e-12 sigma_f^2, mean error ~ 1e-11 at |beta|_1 ~ 1e3)."""
    assert np.finfo(np.longdouble).eps < 1e-18
    case = R.make_case(5, "rbf", 2, 3, 96, 3000)
    a = (case["kern_types"], case["hyp"], case["Zu"], case["X"], case["Y"], case["s2"], 1e-6)
    b_np, M_np, cond = R.sparse_fit_np(*a)
    b_ld, M_ld = R.sparse_fit_ld(*a)
    mu_np, var_np = R.predict_any(a[0], a[1], a[2], b_np, M_np, case["xq"])
    mu_ld, var_ld = R.predict_any(a[0], a[1], a[2], b_ld, M_ld, case["xq"], ld=True)
    sf2 = R.sigma_f2(a[0], a[1], case["xq"])
    assert max(cond) <= 1e6
    assert (np.abs(var_np - var_ld) / sf2).max() <= 1e-10
    # rounding of the fp64 route, amplified by cond K_uu at most: eps cond |beta|_1
    assert np.abs(mu_np - mu_ld).max() <= 2.3e-16 * max(cond) * np.abs(b_np).sum(0).max()
    for d in range(2):
        assert np.linalg.eigvalsh(M_np[d]).min() > 0          # N >= m, distinct data: M is positive definite
    # P upper triangular with P P^T = M, taken from the last row upwards (what the device writes into Wt)
    J = np.arange(96)[::-1]
    L = np.linalg.cholesky(M_np[0][np.ix_(J, J)])
    P = L[np.ix_(J, J)]
    assert np.array_equal(np.tril(P, -1), np.zeros_like(P))
    np.testing.assert_allclose(P.dot(P.T), M_np[0], rtol=0, atol=1e-12 * np.abs(M_np[0]).max())


def test_inducing_inputs_equal_to_the_data_give_the_exact_gp():
    """Z_u = X: M = (K + s2 I)^-1 and beta = M y, the exact model with diagonal term s2 (rounding only: the sparse route
    goes through K_uu^-1, so its rounding is amplified by cond K_uu where the exact fit's is by cond K_y).
    The collapse is exact for jit = 0 only: the jitter sits on K_uu but not on K_uf, and per eigenvalue l of K
    M = l^2 / ((l + jit) (s2 (l + jit) + l^2)), which differs from 1 / (l + jit + s2) by (2 s2 jit l + s2 jit^2) over the
    same denominator -- 0.7 % of an entry at jit = 1e-6 here.  Hence jit = 0 in this check."""
    rng = np.random.default_rng(1)
    n, D = 40, 3
    X = rng.uniform(-1, 1, (n, D))
    Y = rng.standard_normal((n, 2))
    ls = rng.uniform(0.4, 0.6, (2, D))
    sf2 = np.array([1.1, 0.9])
    s2, jit = np.array([1e-2, 2e-2]), 0.0
    hyp = [{"lengthscale": ls[d], "variance": sf2[d]} for d in range(2)]
    beta, Ms, cond = R.sparse_fit_np(["rbf"] * 2, hyp, X, X, Y, s2, jit)
    # the oracle's exact posterior adds its own GPy jitter (1e-8) to the diagonal it is given
    rb, rinv, _ = orc.gp_fit(X, Y, ls, sf2, s2 + jit - 1e-8)
    for d in range(2):
        # M is the difference of two inverses computed through Cholesky factors; each carries the standard bound
        # c n eps cond |X|_2 with c ~ 2, and both are of the size of K_uu^-1: atol = 4 n eps cond(K_uu) |K_uu^-1|_2
        Kinv = np.linalg.inv(orc.kernel_matrix("rbf", hyp[d], X, X) + jit * np.eye(n))
        atol = 4 * n * 2.3e-16 * cond[d] * np.linalg.norm(Kinv, 2)
        assert atol <= 1e-6 * np.abs(rinv[d]).max()               # (the check is informative: rounding, not per cent)
        np.testing.assert_allclose(Ms[d], rinv[d], rtol=0, atol=atol)
        np.testing.assert_allclose(beta[:, d], rb[:, d], rtol=0, atol=atol * np.abs(Y[:, d]).sum())


# ------------------------------------------------------------------ argument handling, library calls monkeypatched
@pytest.fixture
def sparse_model(lib_built, monkeypatch):
    from safe_exploration_amd import SimpleGPModel
    calls = []

    def fake_fit(self, Zu, X, Y, noise_diag, jitter):
        calls.append(dict(Zu=Zu.copy(), N=X.shape[0], noise_diag=noise_diag, jitter=jitter))
    monkeypatch.setattr(SimpleGPModel, "_fit_sparse", fake_fit)
    monkeypatch.setattr(SimpleGPModel, "choose_datapoints_maxvar",
                        lambda self, x, y, m, **kw: (x[:m], y[:m]))

    def make(**kw):
        gp = SimpleGPModel(2, 2, 1, **kw)
        gp.do_sparse_gp = True
        return gp
    return make, calls


def test_train_arguments_with_do_sparse_gp(sparse_model):
    from safe_exploration_amd.ssm_hip import gaussian_process as G
    make, calls = sparse_model
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(-1, 1, (50, 3)), rng.standard_normal((50, 2))
    gp = make()
    with pytest.raises(ValueError, match="inducing points m"):
        gp.train(X, Y, None, opt_hyp=False)
    with pytest.raises(NotImplementedError):
        gp.train(X, Y, 10, opt_hyp=True)
    assert not calls and not gp.gp_trained
    # the caller's Z wins over a selection; all of the data goes to the fit
    Z = rng.uniform(-1, 1, (7, 3))
    gp.train(X, Y, 10, opt_hyp=False, Z=Z)
    assert calls[-1]["N"] == 50 and np.array_equal(calls[-1]["Zu"], Z) and calls[-1]["jitter"] == G.SPARSE_JITTER == 1e-6
    assert gp.gp_trained and np.array_equal(gp.z, Z) and gp.x_train.shape == (50, 3) and gp.y_z.shape == (7, 2)
    # no Z: the m rows _select_subset picks
    gp.train(X, Y, 10, opt_hyp=False)
    assert np.array_equal(calls[-1]["Zu"], X[:10]) and calls[-1]["N"] == 50
    with pytest.raises(ValueError):
        gp.train(X[:5], Y[:5], 10, opt_hyp=False, Z=Z)          # fewer data rows than inducing inputs
    with pytest.raises(ValueError):
        gp.train(X, Y, 10, opt_hyp=False, Z=Z[:, :2])


def test_update_model_refits_a_sparse_model_over_all_data(sparse_model):
    make, calls = sparse_model
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(-1, 1, (50, 3)), rng.standard_normal((50, 2))
    Z = rng.uniform(-1, 1, (7, 3))
    gp = make(m=7, Z=Z)                                          # z_fixed: the inducing inputs stay
    assert gp.z_fixed
    gp.train(X[:30], Y[:30], 7, opt_hyp=False, Z=Z)
    gp.update_model(X[30:], Y[30:], replace_old=False)
    assert calls[-1]["N"] == 50 and np.array_equal(calls[-1]["Zu"], Z) and gp.x_train.shape == (50, 3)
    gp.update_model(X[30:], Y[30:], replace_old=True)
    assert calls[-1]["N"] == 20 and np.array_equal(calls[-1]["Zu"], Z) and gp.x_train.shape == (20, 3)
    with pytest.raises(NotImplementedError):
        gp.update_model(X[:1], Y[:1], opt_hyp=True, replace_old=False)
    # not z_fixed: the inducing rows are selected again from the grown data; one new point never takes the append route
    g2 = make()
    g2.train(X[:30], Y[:30], 7, opt_hyp=False)
    n = len(calls)
    g2.update_model(X[30:31], Y[30:31], replace_old=False)
    assert len(calls) == n + 1 and calls[-1]["N"] == 31 and np.array_equal(calls[-1]["Zu"], X[:7])


def test_information_gain_of_a_sparse_model_is_refused(sparse_model):
    make, calls = sparse_model
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(-1, 1, (20, 3)), rng.standard_normal((20, 2))
    gp = make()
    gp.train(X, Y, 5, opt_hyp=False)
    gp._handle = object()                                         # (no device here: the refusal comes first)
    with pytest.raises(NotImplementedError, match="sparse"):
        gp.information_gain()
