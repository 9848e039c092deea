"""Retiring training points without a refit (sr_gp_remove) and the leave-one-out posterior (sr_gp_loo) are part of the
C-ABI: declared in the header, exported by the cross-compiled library, bound in _lib.py; update_model takes n_max= / retire=
and remove_data checks its arguments before any device is touched; and the closed form the kernels implement
(tests/_remove_ref.py) equals a dense refit on the remaining rows.  Runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _remove_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_remove_and_loo_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    for name in ("sr_gp_remove", "sr_gp_loo"):
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export %s" % name
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_remove\(sr_gp_t h, const int\* idx_host, int m, void\* stream\);", hdr)
    assert re.search(r"int sr_gp_loo\(sr_gp_t h, double\* mu_loo, double\* var_loo, void\* stream\);", hdr)
    assert "ssm_gpy/gaussian_process.py:347-419" in hdr[hdr.index("Retire m training points"):hdr.index("int sr_gp_remove(")]
    from safe_exploration_amd import _lib
    restype, args = _lib.SIGNATURES["sr_gp_remove"]
    assert restype is ctypes.c_int and args == [_lib._H, _lib._PI, _lib._I, _lib._P]
    restype, args = _lib.SIGNATURES["sr_gp_loo"]
    assert restype is ctypes.c_int and args == [_lib._H, _lib._P, _lib._P, _lib._P]
    assert hasattr(_lib.lib, "sr_gp_remove") and hasattr(_lib.lib, "sr_gp_loo")


def test_update_model_and_remove_data_arguments(lib_built):
    from safe_exploration_amd import SimpleGPModel
    params = list(inspect.signature(SimpleGPModel.update_model).parameters.values())
    assert [p.name for p in params[-2:]] == ["n_max", "retire"]
    assert params[-2].default is None and params[-1].default == "oldest"
    for name in ("remove_data", "loo", "loo_device"):
        assert callable(getattr(SimpleGPModel, name))
    gp = SimpleGPModel(2, 2, 1)                    # untrained: nothing below may reach a device
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-1, 1, (4, 3)), rng.standard_normal((4, 2))
    with pytest.raises(ValueError):
        gp.update_model(x, y, replace_old=False, n_max=10, retire="bogus")
    with pytest.raises(ValueError):
        gp.update_model(x, y, replace_old=False, n_max=0)
    with pytest.raises(ValueError):
        gp.remove_data(0)                          # no training data
    gp.x_train, gp.y_train, gp.gp_trained = x, y, True       # the host side of a trained model; still no handle
    for bad in ([0, 0], 4, -1, [0, 1, 2, 3], [], 1.5, [[0, 1]]):
        with pytest.raises(ValueError):
            gp.remove_data(bad)
    np.testing.assert_array_equal(gp.x_train, x)


def _rbf_gram(rng, N, noise=1e-4, dtype=np.float64):
    Z = rng.uniform(-1, 1, (N, 3)).astype(dtype)
    ls = np.array([0.7, 0.9, 1.1], dtype=dtype)
    d2 = (((Z[:, None, :] - Z[None, :, :]) / ls) ** 2).sum(-1)
    return np.exp(-d2 / 2) + dtype(noise) * np.eye(N, dtype=dtype)


def _fit(K, y):
    Wt = rr.factor(K)
    return Wt, Wt.dot(Wt.T.dot(y)), -2 * np.log(np.diag(Wt)).sum()


@pytest.mark.parametrize("N", [40, 150])
@pytest.mark.parametrize("dtype", [np.longdouble, np.float64])
def test_closed_form_equals_dense_refit(N, dtype):
    """_remove_ref.remove on the unpadded factor and on the front-padded one (off = 1 and a full 128-row padding block) against
    the factor, alpha and log det of a dense fit on the remaining rows; first, a middle and the last row.
    Entry by entry at rtol 1e-6 in extended precision (x86 long double, eps 1.1e-19): both sides carry cond(K) eps of the
    factor's SCALE as absolute error -- cond(K) ~ 1e6 at noise 1e-4 -- which in float64 is 1e-10 of the largest entry and
    hides entries 1e-4 of it (measured at N = 150: one entry of 22201, |W| = 1.2e-4, off by 1.6e-10); in long double it is
    1e-13.  float64, what the kernels compute in, is held to the same bounds with the absolute term of the project's
    "incremental equals refit" tolerance for the factor (1e-9 of its largest entry)."""
    if dtype is np.longdouble:
        assert np.finfo(np.longdouble).eps < 1e-18, "long double is not extended precision here"
    rng = np.random.default_rng(N)
    K = _rbf_gram(rng, N, dtype=dtype)
    y = rng.standard_normal(N).astype(dtype)
    Wt, alpha, ld = _fit(K, y)
    for j in (0, N // 2, N - 1):
        keep = np.arange(N) != j
        W_ref, a_ref, ld_ref = _fit(K[np.ix_(keep, keep)], y[keep])
        atol = 0.0 if dtype is np.longdouble else 1e-9 * float(np.abs(W_ref).max())
        for Np in (N, N + 1, N + 128):
            Wp, ap = rr.pad_front(Wt, alpha, Np)
            off = Np - N
            W1, a1, lr = rr.remove(Wp, ap, j + off)
            assert W1.dtype == dtype
            assert np.all(np.tril(W1, -1) == 0.0)
            assert np.all(W1[:off + 1, :off + 1] == np.eye(off + 1)) and np.all(W1[:off + 1, off + 1:] == 0.0)
            assert np.all(a1[:off + 1] == 0.0)
            np.testing.assert_allclose(np.triu(W1[off + 1:, off + 1:]), W_ref, rtol=1e-6, atol=atol)
            np.testing.assert_allclose(a1[off + 1:], a_ref, rtol=1e-7)
            assert abs(ld + lr - ld_ref) <= 1e-8


def test_loo_formulas_equal_explicit_leave_one_out_fits():
    """R&W 5.12 from the rows of the factor against N explicit fits with one row left out.  Bounds: cond(K) ~ N / noise =
    3e3, so both sides are good to ~1e-12 relative; 1e-9 / 1e-8 leave three orders."""
    N = 30
    rng = np.random.default_rng(5)
    K = _rbf_gram(rng, N, noise=1e-2)
    y = rng.standard_normal(N)
    Wt, alpha = rr.factor(K), np.linalg.solve(K, y)
    mu, var = rr.loo(Wt, alpha, y)
    mu_i, var_i = rr.loo_from_inv(np.linalg.inv(K), alpha, y)
    np.testing.assert_allclose(mu, mu_i, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(var, var_i, rtol=1e-9)
    for j in range(N):
        keep = np.arange(N) != j
        kj = K[keep, j]
        sol = np.linalg.solve(K[np.ix_(keep, keep)], np.column_stack((y[keep], kj)))
        assert abs(mu[j] - kj.dot(sol[:, 0])) <= 1e-9 * max(1.0, np.abs(y).max())
        np.testing.assert_allclose(var[j], K[j, j] - kj.dot(sol[:, 1]), rtol=1e-8)
    sc = rr.redundancy_scores(np.column_stack((alpha, alpha)), np.column_stack((var, var)))
    np.testing.assert_allclose(sc, 2 * alpha ** 2 * var, rtol=1e-14)
