"""The reverse pass of the moment-matching roll-out (sr_gp_moment_match_rollout_vjp), the part that needs no GPU.

The NumPy sweep of tests/_mm_rollout_grad_ref.py -- the reference of tests/test_gpu_moment_match_rollout_vjp.py -- against
``_mm_grad_ref.propagate_grad`` on both of its routes (autograd through the torch port of the forward, and autograd with the
analytic VJP as the GP's backward), against autograd with a seed on the GP's covariance (which ``propagate_grad`` does not
take), and against central differences of ``_mm_ref.propagate``; on the cases of tests/_mm_rollout_cases.py that the GPU test
uses, with the exact GP fitted in NumPy on the case's rows.

The figure the GPU bar is built on: the largest disagreement of the two autograd routes, relative to each gradient's largest
element, over all those cases (the first two trajectories of each, the four gradients): MEASURED = 5.6e-11, seen 5.58e-11
(size-256, noise 1e-2; then nout-1 1.9e-11, size-255 8.8e-12, model-from-global 9.0e-12; cartpole 2.7e-13).
``test_routes_agree`` holds the routes to it, so that it cannot drift unnoticed.  The GPU bar is BAR = 30 x MEASURED = 1.68e-9
of a gradient's largest element, the convention of tests/test_gpu_moment_match_grad.py; the sweep is held to the same bar
against both routes here (seen: 5.9e-11 at most, size-256).

Central differences along random unit directions of (mu_0, sigma_0 symmetric, k_ff, k_fb), h = 1e-5, on ``start-full-own``
(N = 80, H = 4): bar 1e-5 (1 + |dL|) as in tests/test_moment_match_grad_host.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import _mm_ref as R
import _mm_grad_ref as G
import _mm_rollout_cases as C
import _mm_rollout_grad_ref as S

MEASURED = 5.6e-11
BAR = 30.0 * MEASURED

# the cases of the GPU test (its own N = 1100 case aside: a forward of that size by autograd takes minutes on the CPU)
GPU_CASES = (["width-%d" % d for d in (2, 3, 4, 5, 8, 9, 12)] + ["size-%d" % n for n in (1, 2, 63, 64, 65, 255, 256, 257)] +
             ["model-from-global"] + ["start-%s-%s" % (k, g) for k in ("point", "rank1", "full") for g in ("shared", "own")] +
             ["tz-hidden", "tz-hidden-point", "h1-point", "h1-full", "nout-1", "nout-4", "cartpole", "sparse"])
NAMES = ("mu0_bar", "sigma0_bar", "kff_bar", "kfb_bar")


def seeds(c, tag="seeds"):
    """random seeds on all three outputs, (T, H, ..); the matrix seeds are NOT symmetric"""
    from test_gpu_moment_match import _seed
    rng = np.random.default_rng(_seed("mmrv-" + tag, c["name"]))
    T, H, n = c["T"], c["H"], c["n_s"]
    return rng.standard_normal((T, H, n)), rng.standard_normal((T, H, n, n)), rng.standard_normal((T, H, n, n))


def rel(got, ref):
    """largest difference as a share of the reference's largest element"""
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def sym(x):
    """sigma0_bar is the gradient of the function extended to unsymmetric sigma_0 by sigma -> (sigma + sigma^T) / 2 (the
    convention of ``_mm_grad_ref`` for S_bar): autograd through a forward that does not symmetrise gives Hm^T w Hm with the
    unsymmetric seed w, whose symmetric part is meant"""
    return 0.5 * (x + np.swapaxes(x, -2, -1))


def _traj(c, t):
    kff, kfb = C.gains(c, t)
    return c["mu0"][t], None if c["sigma0"] is None else c["sigma0"][t], kff, kfb


@pytest.mark.parametrize("name", GPU_CASES)
def test_routes_agree(name):
    c = C.build(name)
    arrs = C.host_arrays(c)
    tz = C.tz_of(c)
    w_mu, w_sig, _ = seeds(c)
    worst_routes, worst_sweep = 0.0, 0.0
    for t in range(min(c["T"], 2)):
        mu0, s0, kff, kfb = _traj(c, t)
        mu_all, sigma_all, _ = R.propagate(*arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz)
        sw = S.sweep(arrs, mu0, s0, kff, kfb, c["a"], c["b"], tz, mu_all, sigma_all, w_mu[t], w_sig[t], None)
        auto = G.propagate_grad(arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz, w_mu[t], w_sig[t])
        anal = G.propagate_grad(arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz, w_mu[t], w_sig[t], analytic=True)
        for what, x, y, z in zip(NAMES, sw, auto, anal):
            if y is None:
                assert x is None and z is None
                continue
            if what == "sigma0_bar":
                y, z = sym(y), sym(z)
            rr, rs = rel(z, y), max(rel(x, y), rel(x, z))
            print("mmrv-host %s t=%d %s: routes %.2e, sweep %.2e (|g| %.1e)" % (name, t, what, rr, rs, np.abs(y).max()))
            worst_routes, worst_sweep = max(worst_routes, rr), max(worst_sweep, rs)
        if s0 is not None:
            assert np.array_equal(sw[1], sw[1].T)
    print("mmrv-host %s worst: routes %.3e, sweep %.3e" % (name, worst_routes, worst_sweep))
    assert worst_routes <= MEASURED, (name, worst_routes)
    assert worst_sweep <= BAR, (name, worst_sweep)


@pytest.mark.parametrize("name", ["start-full-own", "start-point-shared", "tz-hidden"])
def test_cov_seed_against_autograd(name):
    """a seed on all three outputs: autograd through ``propagate_torch`` with the covariance in the loss"""
    import torch
    c = C.build(name)
    arrs = C.host_arrays(c)
    tz = C.tz_of(c)
    w_mu, w_sig, w_cov = seeds(c)
    tt = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    for t in range(c["T"]):
        mu0, s0, kff, kfb = _traj(c, t)
        mu_all, sigma_all, _ = R.propagate(*arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz)
        sw = S.sweep(arrs, mu0, s0, kff, kfb, c["a"], c["b"], tz, mu_all, sigma_all, w_mu[t], w_sig[t], w_cov[t])
        leaves = [None if x is None else tt(x).clone().requires_grad_(True) for x in (mu0, s0, kff, kfb)]
        outs = G.propagate_torch(tuple(tt(x) for x in arrs), leaves[0], leaves[2], leaves[3], tt(c["a"]), tt(c["b"]), leaves[1],
                                 tt(tz))
        L = sum((tt(w) * o).sum() for w, o in zip((w_mu[t], w_sig[t], w_cov[t]), outs))
        grads = iter(torch.autograd.grad(L, [x for x in leaves if x is not None]))
        auto = [None if x is None else next(grads).numpy() for x in leaves]
        for what, x, y in zip(NAMES, sw, auto):
            if y is None:
                assert x is None
                continue
            y = sym(y) if what == "sigma0_bar" else y
            print("mmrv-host cov %s t=%d %s: %.2e of the largest element" % (name, t, what, rel(x, y)))
            assert rel(x, y) <= BAR, (name, t, what)


def test_against_central_differences():
    c = C.build("start-full-own")
    arrs = C.host_arrays(c)
    tz = C.tz_of(c)
    w_mu, w_sig, w_cov = seeds(c)
    t, h = 0, 1e-5
    mu0, s0, kff, kfb = _traj(c, t)

    def L(m, s, f, k):
        outs = R.propagate(*arrs, m, f, k, c["a"], c["b"], s, tz)
        return sum(np.sum(w * o) for w, o in zip((w_mu[t], w_sig[t], w_cov[t]), outs))

    mu_all, sigma_all, _ = R.propagate(*arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz)
    g = S.sweep(arrs, mu0, s0, kff, kfb, c["a"], c["b"], tz, mu_all, sigma_all, w_mu[t], w_sig[t], w_cov[t])
    rng = np.random.default_rng(5)
    for _ in range(4):
        d = [rng.standard_normal(x.shape) for x in (mu0, s0, kff, kfb)]
        d[1] = 0.5 * (d[1] + d[1].T)
        nrm = np.sqrt(sum(np.sum(x * x) for x in d))
        d = [x / nrm for x in d]
        cd = (L(mu0 + h * d[0], s0 + h * d[1], kff + h * d[2], kfb + h * d[3]) -
              L(mu0 - h * d[0], s0 - h * d[1], kff - h * d[2], kfb - h * d[3])) / (2 * h)
        an = sum(np.sum(x * y) for x, y in zip(g, d))
        print("mmrv-host central difference: directional derivative %.6e, off by %.2e" % (an, abs(cd - an)))
        assert abs(cd - an) <= 1e-5 * (1.0 + abs(an))


def test_seed_conventions():
    """only the symmetric parts of the matrix seeds count; None is zero; the sweep is linear in the seeds"""
    c = C.build("start-rank1-own")
    arrs = C.host_arrays(c)
    tz = C.tz_of(c)
    w_mu, w_sig, w_cov = seeds(c)
    mu0, s0, kff, kfb = _traj(c, 1)
    mu_all, sigma_all, _ = R.propagate(*arrs, mu0, kff, kfb, c["a"], c["b"], s0, tz)
    run = lambda *s: S.sweep(arrs, mu0, s0, kff, kfb, c["a"], c["b"], tz, mu_all, sigma_all, *s)
    full = run(w_mu[1], w_sig[1], w_cov[1])
    sym = run(w_mu[1], 0.5 * (w_sig[1] + np.swapaxes(w_sig[1], 1, 2)), 0.5 * (w_cov[1] + np.swapaxes(w_cov[1], 1, 2)))
    parts = [run(w_mu[1], None, None), run(None, w_sig[1], None), run(None, None, w_cov[1])]
    zero = run(w_mu[1], np.zeros_like(w_sig[1]), None)
    for k in range(4):
        assert rel(sym[k], full[k]) <= 1e-13
        assert rel(parts[0][k] + parts[1][k] + parts[2][k], full[k]) <= 1e-12
        assert np.array_equal(zero[k], parts[0][k])


DECL = (r"int sr_gp_moment_match_rollout_vjp\(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj,\s+"
        r"const double\* mu0, const double\* sigma0, const double\* k_ff, const double\* k_fb,\s+"
        r"const double\* a, const double\* b, const double\* tz, const double\* inv_k,\s+"
        r"const double\* mu_all, const double\* sigma_all,\s+"
        r"const double\* mu_all_bar, const double\* sigma_all_bar, const double\* cov_all_bar,\s+"
        r"double\* mu0_bar, double\* sigma0_bar, double\* kff_bar, double\* kfb_bar, void\* stream\);")


def test_declared_interface(lib_built):
    """the header declares the entry as agreed, the library exports it, the ctypes table carries its signature, and the Python
    layers have their three names"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "safereach.h")) as f:
        assert re.search(DECL, f.read()), "include/safereach.h does not declare sr_gp_moment_match_rollout_vjp as agreed"
    from safe_exploration_amd import _lib, SimpleGPModel, uncertainty_propagation_casadi as up
    assert hasattr(_lib.lib, "sr_gp_moment_match_rollout_vjp")
    H, L, I, P = _lib.SIGNATURES["sr_gp_moment_match"][1][0], ctypes.c_long, ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["sr_gp_moment_match_rollout_vjp"] == (ctypes.c_int, [H, L, I, I, I] + [P] * 18)
    assert callable(SimpleGPModel.moment_match_rollout_vjp_device)
    assert callable(up.moment_matching_rollout_vjp_batch) and callable(up.moment_matching_rollout_diff_batch)
