"""The NumPy reference of the path Jacobians (tests/_paths_grad_ref.py) is right, shown without a GPU on the problems of
test_gpu_paths._problem: against torch-fp64 autograd through an independently written forward (cos features plus
exp(-r^2 / 2)), against central differences of _paths_ref.evaluate, and the ordered product of rollout_grad's A_i against
central differences of _paths_ref.rollout in x0.  Also: the two new symbols are declared, exported and bound.

Bars: autograd -- the GPU tests' own rule, max(20 e0, 1e-12 max|J| sqrt(N + M)) with e0 the difference of the reference
between its Cholesky and LU coefficients; finite differences -- 1e-6 max|J|, the truncation error of h = 1e-5 with two
orders of headroom."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _paths_ref as pr
import _paths_grad_ref as pg
import test_gpu_paths as tg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_FD = 1e-5

# (N, S, M, T, D, n_out): test_gpu_paths.CASES and the three widths below / at the compiled ones the GPU tests add
CASES = [c[:6] for c in tg.CASES] + [(64, 16, 16, 16, 2, 1), (64, 16, 16, 16, 4, 2), (64, 16, 16, 16, 7, 1)]
IDS = ["N%d-S%d-M%d-T%d-D%d-o%d" % c for c in CASES]


def _args(p, route):
    return p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][route]


def _jref(p, x):
    a, b = (pg.evaluate_grad(x, *_args(p, r)) for r in ("chol", "lu"))
    e0, scale = float(np.abs(a - b).max()), float(np.abs(a).max())
    return a, e0, scale, max(20.0 * e0, 1e-12 * scale * np.sqrt(p["N"] + p["M"]))


def _torch_forward(x, p):
    """F (T, S, n_out) written from the header's formula alone: nothing of _paths_ref or the oracle"""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64)
    Z, om, tau = t(p["Z"]), t(p["omega"]), t(p["tau"])
    M = om.shape[0]
    cols = []
    for d in range(p["n_out"]):
        l, sf2 = t(p["ls"][d]), float(p["sf2"][d])
        phi = (2.0 * sf2 / M) ** 0.5 * torch.cos((x / l) @ om.T + tau)
        r2 = (((x[:, None, :] - Z[None, :, :]) / l) ** 2).sum(-1)
        cols.append(phi @ t(p["w"][d]).T + (sf2 * torch.exp(-0.5 * r2)) @ t(p["c"]["chol"][d]))
    return torch.stack(cols, dim=-1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_against_autograd(case):
    p = tg._problem(*case)
    D = p["D"]
    ref, e0, scale, bar = _jref(p, p["x"])
    x = torch.as_tensor(p["x"], dtype=torch.float64)
    J = np.empty_like(ref)
    for j in range(D):                                   # forward mode: one tangent per input dimension, all queries at once
        v = torch.zeros_like(x)
        v[:, j] = 1.0
        J[..., j] = torch.autograd.functional.jvp(lambda q: _torch_forward(q, p), x, v)[1].numpy()
    err = float(np.abs(J - ref).max())
    print("paths grad autograd %s  e0=%.3e  err=%.3e  bar=%.3e  scale=%.3g  margin=%.1f"
          % (IDS[CASES.index(case)], e0, err, bar, scale, bar / max(err, 1e-300)))
    assert err <= bar


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_against_central_differences(case):
    p = tg._problem(*case)
    ref = pg.evaluate_grad(p["x"], *_args(p, "chol"))
    sref = pg.step_grad(p["xs"], *_args(p, "chol"))
    fd, sfd = np.empty_like(ref), np.empty_like(sref)
    for j in range(p["D"]):
        e = np.zeros(p["D"])
        e[j] = H_FD
        fd[..., j] = (pr.evaluate(p["x"] + e, *_args(p, "chol")) - pr.evaluate(p["x"] - e, *_args(p, "chol"))) / (2 * H_FD)
        sfd[..., j] = (pr.step(p["xs"] + e, *_args(p, "chol")) - pr.step(p["xs"] - e, *_args(p, "chol"))) / (2 * H_FD)
    for what, a, b in (("eval", fd, ref), ("step", sfd, sref)):
        scale = float(np.abs(b).max())
        err = float(np.abs(a - b).max())
        print("paths grad fd %s %s  err=%.3e  bar=%.3e" % (what, IDS[CASES.index(case)], err, 1e-6 * scale))
        assert err <= 1e-6 * scale


def test_step_grad_is_the_diagonal_of_evaluate_grad():
    p = tg._problem(129, 65, 17, 129, 5, 4)
    J = pg.evaluate_grad(p["xs"], *_args(p, "chol"))
    Js = pg.step_grad(p["xs"], *_args(p, "chol"))
    s = np.arange(p["S"])
    np.testing.assert_allclose(Js, J[s, s], rtol=0, atol=1e-13 * np.abs(J).max())


def test_rollout_grad_product_against_central_differences():
    """n_s = 2, n_u = 1, N = 60, 3 steps, 70 particles, M = 64 (the problem of test_gpu_paths.test_consistent_rollout):
    A_{i} ... A_0 is d x_{i+1} / d x_0 of every particle"""
    n_s, n_u, N, n, S, M = 2, 1, 60, 3, 70, 64
    p = tg._problem(N, S, M, 1, n_s + n_u, n_s)
    rng = np.random.default_rng(9)
    K = 0.3 * rng.standard_normal((n, n_u, n_s))
    k = 0.1 * rng.standard_normal((n, n_u))
    x0 = rng.uniform(-0.5, 0.5, n_s)
    X, A = pg.rollout_grad(x0, K, k, *_args(p, "chol"))
    np.testing.assert_array_equal(X, pr.rollout(x0, K, k, *_args(p, "chol")))
    assert A.shape == (n, S, n_s, n_s)
    fd = np.empty((n, S, n_s, n_s))
    for j in range(n_s):
        e = np.zeros(n_s)
        e[j] = H_FD
        fd[..., j] = (pr.rollout(x0 + e, K, k, *_args(p, "chol")) - pr.rollout(x0 - e, K, k, *_args(p, "chol"))) / (2 * H_FD)
    P = np.tile(np.eye(n_s), (S, 1, 1))
    for i in range(n):
        P = A[i] @ P
        scale, err = float(np.abs(P).max()), float(np.abs(P - fd[i]).max())
        print("paths grad rollout step %d  err=%.3e  bar=%.3e" % (i, err, 1e-6 * scale))
        assert err <= 1e-6 * scale


DECLS = {
    "sr_gp_paths_eval_grad": r"int sr_gp_paths_eval_grad\(sr_gp_t h, const double\* Xq, long T, double\* F, double\* J, "
                             r"void\* stream\);",
    "sr_gp_paths_step_grad": r"int sr_gp_paths_step_grad\(sr_gp_t h, const double\* Xs, double\* F, double\* J, "
                             r"const double\* k_fb, const double\* k_ff,\s+double\* z_next, void\* stream\);",
}


def test_grad_symbols_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    from safe_exploration_amd import _lib
    for name, decl in DECLS.items():
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export %s" % name
        assert re.search(decl, hdr), "include/safereach.h does not declare %s" % name
        assert hasattr(_lib.lib, name) and _lib.SIGNATURES[name][0] is ctypes.c_int
    P, L, H = _lib._P, _lib._L, _lib._H
    assert _lib.SIGNATURES["sr_gp_paths_eval_grad"][1] == [H, P, L, P, P, P]
    assert _lib.SIGNATURES["sr_gp_paths_step_grad"][1] == [H, P, P, P, P, P, P, P]
    doc = hdr[hdr.index("posterior FUNCTION samples"):hdr.index("int sr_gp_paths_draw(")]
    assert "the Jacobian of the paths" not in doc[doc.index("Out of scope"):]


def test_python_keywords_default_to_the_old_returns(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    for fn in (SimpleGPModel.sample_paths_device, SimpleGPModel.sample_paths, SimpleGPModel.paths_step_device):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "jacobians" and last.default is False
    # sample_n_step keeps its parameter list (tests/test_paths_host.py pins it); the Jacobians have a method of their own
    assert "jacobians" not in inspect.signature(MonteCarloSafetyVerification.sample_n_step).parameters
    assert list(inspect.signature(MonteCarloSafetyVerification.sample_n_step_jacobians).parameters) == [
        "self", "x0", "K", "k", "n", "n_samples", "generator", "as_tensor", "consistent", "n_features"]
    assert list(inspect.signature(SimpleGPModel.paths_step_device).parameters) == ["self", "x_s", "k_fb", "k_ff", "jacobians"]
