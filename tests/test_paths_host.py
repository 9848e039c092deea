"""Posterior function samples by pathwise conditioning (sr_gp_paths_draw / _count / _eval / _step) are part of the C-ABI:
declared in the header, exported by the cross-compiled library, bound in _lib.py; sample_n_step's new keywords default to the
old behaviour; draw_paths on an untrained model raises before any device is touched; and the NumPy reference the GPU tests
compare with (tests/_paths_ref.py) has the properties the algebra promises.  Runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_np as orc
import _paths_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sr_gp_paths_draw": r"int sr_gp_paths_draw\(sr_gp_t h, int S, int M, const double\* omega, const double\* tau, const double\* w, "
                        r"const double\* eps,\s+void\* stream\);",
    "sr_gp_paths_count": r"int sr_gp_paths_count\(sr_gp_t h, int\* S, int\* M\);",
    "sr_gp_paths_eval": r"int sr_gp_paths_eval\(sr_gp_t h, const double\* Xq, long T, double\* F, void\* stream\);",
    "sr_gp_paths_step": r"int sr_gp_paths_step\(sr_gp_t h, const double\* Xs, double\* F, const double\* k_fb, const double\* k_ff, "
                        r"double\* z_next,\s+void\* stream\);",
}


def test_paths_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    from safe_exploration_amd import _lib
    for name, decl in DECLS.items():
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export %s" % name
        assert re.search(decl, hdr), "include/safereach.h does not declare %s" % name
        assert hasattr(_lib.lib, name)
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    doc = hdr[hdr.index("posterior FUNCTION samples"):hdr.index("int sr_gp_paths_draw(")]
    assert "ssm_gpy/gaussian_process.py:598-619" in doc and "sampling_models.py:66-80" in doc
    assert "Out of scope" in doc
    P, I, L, H, PI = _lib._P, _lib._I, _lib._L, _lib._H, _lib._PI
    assert _lib.SIGNATURES["sr_gp_paths_draw"][1] == [H, I, I, P, P, P, P, P]
    assert _lib.SIGNATURES["sr_gp_paths_count"][1] == [H, PI, PI]
    assert _lib.SIGNATURES["sr_gp_paths_eval"][1] == [H, P, L, P, P]
    assert _lib.SIGNATURES["sr_gp_paths_step"][1] == [H, P, P, P, P, P, P]


def test_python_surface_and_defaults(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    params = list(inspect.signature(MonteCarloSafetyVerification.sample_n_step).parameters.values())
    assert [p.name for p in params[-2:]] == ["consistent", "n_features"]
    assert params[-2].default is False and params[-1].default == 1024
    # (everything in front of them is what it was: the old positional calls mean the same)
    assert [p.name for p in params[:-2]] == ["self", "x0", "K", "k", "n", "n_samples", "eps", "generator", "as_tensor"]
    sig = inspect.signature(SimpleGPModel.draw_paths)
    assert list(sig.parameters) == ["self", "size", "n_features", "generator", "omega", "tau", "w", "eps"]
    assert sig.parameters["n_features"].default == 1024
    for name in ("paths_count", "sample_paths_device", "sample_paths", "paths_step_device"):
        assert callable(getattr(SimpleGPModel, name))
    gp = SimpleGPModel(2, 2, 1)                    # untrained: nothing below may reach a device
    with pytest.raises(RuntimeError):
        gp.draw_paths(8, 16)
    with pytest.raises(RuntimeError):
        gp.paths_count()
    with pytest.raises(RuntimeError):
        gp.sample_paths(np.zeros((1, 3)))
    assert gp._handle is None


def _tiny(seed, N, M, D, n_out, S):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    noise_var = np.full(n_out, 1e-2 - orc.GPY_JITTER)
    omega, tau = rng.standard_normal((M, D)), rng.uniform(0, 2 * np.pi, M)
    w, eps = rng.standard_normal((n_out, S, M)), rng.standard_normal((n_out, S, N))
    return dict(Z=Z, Y=Y, ls=ls, sf2=sf2, noise_var=noise_var, omega=omega, tau=tau, w=w, eps=eps, rng=rng)


def test_zero_draws_give_the_posterior_mean():
    p = _tiny(1, 40, 24, 3, 2, 3)
    x = p["rng"].uniform(-1.2, 1.2, (17, 3))
    beta, inv_K, _ = orc.gp_fit(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"])
    mu = orc.gp_predict(x, p["Z"], beta, inv_K, p["ls"], p["sf2"], False)[0]
    for route in ("chol", "lu"):
        c = pr.coeffs(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"], p["omega"], p["tau"], 0 * p["w"], 0 * p["eps"], route)
        F = pr.evaluate(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], 0 * p["w"], c)
        for s in range(3):
            np.testing.assert_allclose(F[:, s, :], mu, rtol=1e-10, atol=1e-10 * np.abs(mu).max())
        Fs = pr.step(x[:3], p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], 0 * p["w"], c)
        np.testing.assert_allclose(Fs, mu[:3], rtol=1e-10, atol=1e-10 * np.abs(mu).max())


def test_reference_is_linear_with_the_closed_form_covariance():
    """N = 12, M = 16, D = 2, 5 queries: the unit vectors of (w, eps) through the reference give J; J J^T is the
    covariance of f under standard-normal draws and must equal the closed form."""
    N, M, D, T = 12, 16, 2, 5
    p = _tiny(2, N, M, D, 1, M + N)
    x = p["rng"].uniform(-1, 1, (T, D))
    S = M + N
    w = np.zeros((1, S, M))
    eps = np.zeros((1, S, N))
    w[0, :M, :] = np.eye(M)
    eps[0, M:, :] = np.eye(N)
    zero = np.zeros((1, 1, M)), np.zeros((1, 1, N))
    args = (p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"], p["omega"], p["tau"])
    mu = pr.evaluate(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], zero[0], pr.coeffs(*args, zero[0], zero[1]))[:, 0, 0]
    F = pr.evaluate(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], w, pr.coeffs(*args, w, eps))[:, :, 0]
    J = F - mu[:, None]                                                # (T, M + N)
    # linearity: twice the draws, twice the deviation from the mean
    F2 = pr.evaluate(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], 2 * w, pr.coeffs(*args, 2 * w, 2 * eps))[:, :, 0]
    np.testing.assert_allclose(F2 - mu[:, None], 2 * J, rtol=1e-9, atol=1e-12)
    cov = pr.path_covariance(x, p["Z"], p["ls"][0], p["sf2"][0], pr.diag_term(p["noise_var"])[0], p["omega"], p["tau"])
    np.testing.assert_allclose(J.dot(J.T), cov, rtol=1e-9, atol=1e-9 * np.abs(cov).max())


def test_feature_scaling():
    """Phi(x) . Phi(x') is a Monte-Carlo estimate of k(x, x') from M draws of a term bounded by 2 sf2 with standard
    deviation <= sf2: five standard errors.  Distinct lengthscales per dimension, so that a missing 1 / l shows."""
    M, D = 8192, 3
    rng = np.random.default_rng(3)
    ls, sf2 = np.array([0.4, 0.9, 1.7]), 1.3
    omega, tau = rng.standard_normal((M, D)), rng.uniform(0, 2 * np.pi, M)
    x, y = rng.uniform(-1, 1, (50, D)), rng.uniform(-1, 1, (50, D))
    est = np.einsum("tm,tm->t", pr.features(x, omega, tau, ls, sf2), pr.features(y, omega, tau, ls, sf2))
    k = np.diag(orc.rbf_kernel(x, y, sf2, ls))
    assert np.abs(est - k).max() <= 5 * sf2 / np.sqrt(M)
    wrong = np.einsum("tm,tm->t", pr.features(x, omega, tau, np.ones(D), sf2), pr.features(y, omega, tau, np.ones(D), sf2))
    assert np.abs(wrong - k).max() > 5 * sf2 / np.sqrt(M)              # (the check can tell)
