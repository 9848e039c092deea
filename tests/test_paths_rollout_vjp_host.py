"""The reverse pass of the consistent roll-out (sr_gp_paths_rollout_vjp) without a GPU: the NumPy reference the GPU tests
compare with (tests/_paths_rollout_vjp_ref.py) is right -- its gradients against central differences of _paths_ref.rollout in
every entry of K, k and x0 --, the symbol is declared, exported by the cross-compiled library and bound, and the Python surface
(SimpleGPModel.paths_rollout_vjp_device / paths_rollout_diff_device, MonteCarloSafetyVerification.rollout_paths_diff) has the
agreed parameter lists and raises on an untrained model before any device is touched.

Bar of the finite differences: the rule of tests/test_paths_grad_host.py for this function, h = 1e-5 and 1e-6 max|gradient|
(per gradient array: the stricter reading).  Measured with exactly these inputs: the worst case is 1.2e-7 of the scale
(N200-S40-M32-D4-o3-H5), the others are <= 1.5e-8.

Every test here fails on the parent commit: the reference's subject, the symbol and the methods do not exist there."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _paths_ref as pr
import _paths_rollout_vjp_ref as rv
import test_gpu_paths as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_FD = 1e-5

# (N, S, M, D, n_out, H): the first five cases of tests/test_gpu_paths_rollout_vjp.py
CASES = [(1, 1, 1, 2, 1, 2), (60, 70, 64, 3, 2, 3), (257, 129, 100, 5, 4, 4), (300, 65, 300, 8, 2, 2), (200, 40, 32, 4, 3, 5)]
IDS = ["N%d-S%d-M%d-D%d-o%d-H%d" % c for c in CASES]


def _args(p, route="chol"):
    return p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][route]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_against_central_differences(case):
    N, S, M, D, n_s, H = case
    n_u = D - n_s
    p = tg._problem(N, S, M, 1, D, n_s)
    rng = np.random.default_rng(9 + H)                   # the recipe of test_gpu_paths_rollout._setup
    K = 0.3 * rng.standard_normal((H, n_u, n_s))
    k = 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, n_s)
    X_bar = np.random.default_rng(31).standard_normal((H, S, n_s))
    cost = lambda x0_, K_, k_: float(np.sum(X_bar * pr.rollout(x0_, K_, k_, *_args(p))))
    x0_bar, K_bar, k_bar, _ = rv.vjp(x0, K, k, pr.rollout(x0, K, k, *_args(p)), X_bar, *_args(p))
    x0_bar = x0_bar.sum(axis=0)                          # one start for all paths

    def fd(arr, which):
        out = np.empty_like(arr)
        for idx in np.ndindex(*arr.shape):
            v = []
            for sgn in (1.0, -1.0):
                t = arr.copy()
                t[idx] += sgn * H_FD
                v.append(cost(*(t if which == n else a for n, a in (("x0", x0), ("K", K), ("k", k)))))
            out[idx] = (v[0] - v[1]) / (2 * H_FD)
        return out

    for which, arr, grad in (("K", K, K_bar), ("k", k, k_bar), ("x0", x0, x0_bar)):
        num = fd(arr, which)
        scale, err = float(np.abs(grad).max()), float(np.abs(num - grad).max())
        print("paths rollout vjp fd %s %-2s  err=%.3e  bar=%.3e  err/scale=%.2e"
              % (IDS[CASES.index(case)], which, err, 1e-6 * scale, err / scale))
        assert num.shape == grad.shape and err <= 1e-6 * scale


def test_sweep_dtypes_agree():
    """the long-double sweep the GPU tests run on the device's Jacobians is the fp64 sweep to fp64 rounding"""
    rng = np.random.default_rng(3)
    H, S, n_s, n_u = 4, 37, 3, 2
    J, Xp, Xb = rng.standard_normal((H, S, n_s, n_s + n_u)), rng.standard_normal((H, S, n_s)), rng.standard_normal((H, S, n_s))
    K = rng.standard_normal((H, n_u, n_s))
    a, b, A = rv.sweep(J, Xp, Xb, K), rv.sweep(J, Xp, Xb, K, np.longdouble), rv.sweep_abs(J, Xp, Xb, K)
    n = H * (n_s + n_u + 2) + S + 8
    for u, v, w in zip(a, b, A):
        assert u.dtype == np.float64 and v.dtype == np.longdouble and u.shape == v.shape
        assert np.all(np.abs(u - v) <= n * 2.0 ** -53 * w)


DECL = (r"int sr_gp_paths_rollout_vjp\(sr_gp_t h, const double\* x0, int x0_per_path, int H, const double\* k_fb, "
        r"const double\* k_ff,\s+const double\* X_all, const double\* X_bar, double\* x0_bar, double\* k_fb_bar, "
        r"double\* k_ff_bar,\s+double\* J_all, void\* stream\);")


def test_symbol_declared_exported_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_paths_rollout_vjp$", out, re.M), "libsafereach.so does not export sr_gp_paths_rollout_vjp"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    m = re.search(DECL, hdr)
    assert m, "include/safereach.h does not declare sr_gp_paths_rollout_vjp"
    assert m.start() > hdr.index("int sr_gp_paths_rollout(")           # behind the forward's declaration
    head = hdr[:m.start()].rstrip()                                    # its own contract comment right in front
    assert head.endswith("*/") and head[head.rindex("/*"):].startswith("/* sr_gp_paths_rollout_vjp:")
    from safe_exploration_amd import _lib
    P, I, H = _lib._P, _lib._I, _lib._H
    assert hasattr(_lib.lib, "sr_gp_paths_rollout_vjp")
    assert _lib.SIGNATURES["sr_gp_paths_rollout_vjp"] == (ctypes.c_int, [H, P, I, I, P, P, P, P, P, P, P, P, P])


def test_python_surface(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    sig = inspect.signature(SimpleGPModel.paths_rollout_vjp_device)
    assert list(sig.parameters) == ["self", "x0", "K", "k", "X_all", "X_bar", "jacobians"]
    assert sig.parameters["jacobians"].default is False
    assert list(inspect.signature(SimpleGPModel.paths_rollout_diff_device).parameters) == ["self", "x0", "K", "k"]
    sig = inspect.signature(MonteCarloSafetyVerification.rollout_paths_diff)
    assert list(sig.parameters) == ["self", "x0", "K", "k", "n", "n_samples", "generator", "n_features"]
    assert [sig.parameters[n].default for n in ("n", "n_samples", "generator", "n_features")] == [1, 1000, None, 1024]


def test_untrained_model_raises_before_any_device(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    gp = SimpleGPModel(2, 2, 1)
    K, k, X = np.zeros((3, 1, 2)), np.zeros((3, 1)), np.zeros((3, 8, 2))
    with pytest.raises(RuntimeError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, k, X, X)
    with pytest.raises(RuntimeError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, k, X, X, jacobians=True)
    with pytest.raises(RuntimeError):
        gp.paths_rollout_diff_device(np.zeros(2), K, k)
    with pytest.raises(RuntimeError):
        MonteCarloSafetyVerification(gp).rollout_paths_diff(np.zeros((2, 1)), K, k, n=3, n_samples=8)
    assert gp._handle is None
