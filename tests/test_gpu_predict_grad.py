"""Batched gradient of the predictive variance (sr_gp_predict_grad, SimpleGPModel.predict_device_grad,
predict(states, actions, jacobians=True) for batches, predictive_gradients(grad_sigma=True)) against the oracle, the
single-query route, central differences of the variance, and itself across chunk boundaries and model updates."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _helpers import hip_model, mu_atol, hyp_from, cached_oracle_model
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_S, N_U = 2, 1


def _queries(seed, T, D=N_S + N_U):
    rng = np.random.default_rng(seed)
    return np.hstack((0.3 * rng.standard_normal((T, N_S)), 0.1 * rng.standard_normal((T, D - N_S))))


def _jv_atol(om):
    return 1e-11 * float(np.max(om["signal_var"])) / float(np.min(om["lengthscale"]) ** 2)


def _model(N, seed=5):
    om = cached_oracle_model(seed, N, N_S, N_U)
    syn = orc.make_synthetic(seed, N, N_S, N_U, 4)
    gp = hip_model(syn["Z"], syn["Y"], syn["lengthscale"], syn["signal_var"], syn["noise_var"], N_S, N_U)
    return om, gp


def _check_rows(x, jv, om, rows):
    for t in rows:
        rjv, _ = orc.gp_linearize_extras(x[t], om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
        np.testing.assert_allclose(jv[t], rjv, rtol=1e-9, atol=_jv_atol(om), err_msg="row %d" % t)


@pytest.mark.parametrize("N", [50, 200, 1000, 2000])
def test_predict_grad_oracle_rbf(N):
    om, gp = _model(N)
    rng = np.random.default_rng(N)
    for T in (2, 17, 129, 1000):
        x = _queries(100 + T, T)
        mu, var, jm, jv = gp.predict_device_grad(x)
        mu, var, jm, jv = (o.cpu().numpy() for o in (mu, var, jm, jv))
        assert jv.shape == (T, N_S, N_S + N_U)
        rows = np.arange(T) if T <= 64 else np.sort(rng.choice(T, 64, replace=False))
        _check_rows(x, jv, om, rows)
        pmu, pvar, pjm = gp.predict(x, None, True)
        np.testing.assert_allclose(mu, pmu, rtol=1e-10, atol=mu_atol(om))
        np.testing.assert_allclose(var, pvar, rtol=0, atol=1e-9 * float(np.max(om["signal_var"])))
        np.testing.assert_allclose(jm, pjm, rtol=1e-9, atol=mu_atol(om))


def _refined_jac_var(x, om):
    """d var/dx = -2 sum_i g_i k*_i (z_i - x) / l^2 (the formula of orc.gp_linearize_extras) with g = K^-1 k* from the
    Cholesky factor and two steps of iterative refinement instead of the explicit inverse.  At N = 5000 the explicit
    inverse carries errors of ~cond(K) eps that change with the host's BLAS thread count (6e-12 in a row of d var/dx,
    the size of the bar 1e-11 sf2 / l_min^2; refining the inverse itself does not remove them); the refined solve gives
    the same row to 1e-16 whatever the thread count."""
    import scipy.linalg as sla
    Z = om["Z"]
    jv = np.empty((x.shape[0], len(om["signal_var"]), Z.shape[1]))
    for d in range(jv.shape[1]):
        ls, sf2 = om["lengthscale"][d], om["signal_var"][d]
        L = om["chol"][d]
        Ky = orc.rbf_kernel(Z, Z, sf2, ls) + (om["noise_var"][d] + orc.GPY_JITTER) * np.eye(Z.shape[0])
        ks = orc.rbf_kernel(x, Z, sf2, ls)                                   # (R, N)
        g = sla.cho_solve((L, True), ks.T)
        for _ in range(2):
            g += sla.cho_solve((L, True), ks.T - Ky.dot(g))
        w = g.T * ks
        jv[:, d, :] = -2.0 * (w.dot(Z) - w.sum(1)[:, None] * x) / ls[None, :] ** 2
    return jv


@pytest.mark.parametrize("N", [2000, 5000])
def test_predict_grad_oracle_rbf_refined_solve(N):
    """test_predict_grad_oracle_rbf for the big models, at the same bars, with d var/dx of the oracle from a refined
    Cholesky solve (_refined_jac_var) -- at N = 5000 the explicit inverse of the oracle is not accurate to the bar.
    (N = 2000: both references on one model, the explicit inverse above and the refined solve here.)"""
    om, gp = _model(N)
    rng = np.random.default_rng(N)
    for T in (2, 17, 129, 1000):
        x = _queries(100 + T, T)
        mu, var, jm, jv = (o.cpu().numpy() for o in gp.predict_device_grad(x))
        assert jv.shape == (T, N_S, N_S + N_U)
        rows = np.arange(T) if T <= 64 else np.sort(rng.choice(T, 64, replace=False))
        rjv = _refined_jac_var(x[rows], om)
        for i, t in enumerate(rows):
            np.testing.assert_allclose(jv[t], rjv[i], rtol=1e-9, atol=_jv_atol(om), err_msg="row %d" % t)
        pmu, pvar, pjm = gp.predict(x, None, True)
        np.testing.assert_allclose(mu, pmu, rtol=1e-10, atol=mu_atol(om))
        np.testing.assert_allclose(var, pvar, rtol=0, atol=1e-9 * float(np.max(om["signal_var"])))
        np.testing.assert_allclose(jm, pjm, rtol=1e-9, atol=mu_atol(om))


@pytest.mark.parametrize("kt", ["mat52", "lin_rbf", "lin_mat52"])
def test_predict_grad_general_kernels(kt):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(77)
    D, N, T = 3, 700, 300
    Z = rng.uniform(-1, 1, (N, D))
    Y = rng.standard_normal((N, 2))
    hyp = [orc.make_hyp(kt, rng, D) for _ in range(2)]
    noise = np.array([0.02, 0.03])
    beta, inv_K = orc.gp_fit_k(Z, Y, [kt] * 2, hyp, noise + 1e-5)
    gp = SimpleGPModel(2, 2, 1, kern_types=[kt] * 2, hyp=[dict(h, noise_variance=nv) for h, nv in zip(hyp, noise)])
    gp.train(Z, Y, opt_hyp=False)
    x = rng.uniform(-0.8, 0.8, (T, D))
    mu, var, jm, jv = (o.cpu().numpy() for o in gp.predict_device_grad(x))
    scale = max(np.abs(beta).sum(0).max(), 1.0)
    for t in list(range(8)) + list(rng.choice(T, 24, replace=False)):
        rjv, _ = orc.gp_linearize_extras_k(x[t], Z, beta, inv_K, [kt] * 2, hyp)
        np.testing.assert_allclose(jv[t], rjv, rtol=1e-7, atol=1e-9, err_msg="%s row %d" % (kt, t))
    rmu, rvar = orc.gp_predict_k(x, Z, beta, inv_K, [kt] * 2, hyp)
    np.testing.assert_allclose(mu, rmu, rtol=1e-9, atol=1e-11 * scale)
    np.testing.assert_allclose(var, rvar, rtol=0, atol=1e-8 * max(1.0, float(rvar.max())))
    np.testing.assert_allclose(jm, orc.gp_mean_jacobian_k(x, Z, beta, [kt] * 2, hyp), rtol=1e-9, atol=1e-11 * scale)


def test_predict_grad_matches_single_query_route():
    om, gp = _model(1500)
    x = _queries(3, 200)
    jv = gp.predict_device_grad(x)[3].cpu().numpy()
    # d var/dx is a sum of terms of size sf2 |G_i| |z_i - x| / l^2 that cancel down to ~1e-5 here: the two routes sum them
    # in different orders, so an entry near zero can differ by a few ulps of the terms (2.5e-15 seen), not of the result
    atol = 1e-12 * float(np.max(om["signal_var"])) / float(np.min(om["lengthscale"]) ** 2)
    for t in range(16):
        out = gp.linearize_device(x[t])
        ref = out[3].cpu().numpy()
        np.testing.assert_allclose(jv[t], ref, rtol=1e-10, atol=atol, err_msg="row %d" % t)


def test_predict_grad_central_differences():
    om, gp = _model(1000)
    T, D = 64, N_S + N_U
    x = _queries(4, T)
    jv = gp.predict_device_grad(x)[3].cpu().numpy()
    l = np.min(om["lengthscale"], axis=0)
    fd = np.empty_like(jv)
    for j in range(D):
        h = 1e-5 * l[j]
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        fd[:, :, j] = (gp.predict(xp)[1] - gp.predict(xm)[1]) / (2 * h)
    np.testing.assert_allclose(jv, fd, rtol=1e-6, atol=1e-6 * np.abs(jv).max())


def test_predict_grad_chunk_boundaries():
    om, gp = _model(2000)
    x = _queries(5, 10000)
    whole = [o.cpu().numpy() for o in gp.predict_device_grad(x)]
    gp.set_chunk(4096)
    parts = [o.cpu().numpy() for o in gp.predict_device_grad(x)]
    gp.set_chunk(65536)
    # the gradient comes from per-tile arithmetic and a fixed-order reduction that do not depend on the chunk: the same bits
    np.testing.assert_array_equal(parts[3], whole[3])
    # var: sr_finalize adds the row blocks' partials in another order up to 4096 queries (one wavefront per query)
    np.testing.assert_allclose(parts[1], whole[1], rtol=1e-11, atol=1e-15)
    # mu / d mu/dx: the K* pass splits the training rows by batch width, so the order of the sum may differ
    np.testing.assert_allclose(parts[0], whole[0], rtol=1e-13, atol=mu_atol(om))
    np.testing.assert_allclose(parts[2], whole[2], rtol=1e-12, atol=mu_atol(om))


def test_batched_jacobians_take_no_per_row_loop(monkeypatch):
    from safe_exploration_amd import SimpleGPModel
    om, gp = _model(800)

    def boom(self, x):
        raise AssertionError("per-row linearisation called")

    monkeypatch.setattr(SimpleGPModel, "_linearize_host", boom)
    x = _queries(6, 64)
    m, v, jm, jv = gp.predict(x[:, :N_S], x[:, N_S:], True)
    assert isinstance(jv, np.ndarray) and jv.shape == (64, N_S, N_S + N_U)
    _check_rows(x, jv, om, range(64))
    rmu, rvar, rjm = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
    np.testing.assert_allclose(m, rmu, rtol=1e-9, atol=mu_atol(om))
    np.testing.assert_allclose(jm, rjm, rtol=1e-9, atol=mu_atol(om))


def test_predict_grad_device_tensors():
    import torch
    om, gp = _model(600)
    x = _queries(7, 100)
    tx = torch.from_numpy(x).to(gp.device)
    outs = gp.predict_device_grad(tx)
    assert all(isinstance(o, torch.Tensor) and o.device == tx.device for o in outs)
    outs2 = gp.predict(tx[:, :N_S], tx[:, N_S:], True)
    assert len(outs2) == 4 and all(isinstance(o, torch.Tensor) and o.device == tx.device for o in outs2)
    for a, b in zip(outs, outs2):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    gm, gv = gp.predictive_gradients(tx, grad_sigma=True)
    assert isinstance(gv, torch.Tensor) and gv.shape == (100, N_S, N_S + N_U)
    torch.testing.assert_close(gv, outs[3], rtol=0, atol=0)
    torch.testing.assert_close(gm, outs[2], rtol=0, atol=0)
    gm_np, gv_np = gp.predictive_gradients(x, grad_sigma=True)
    assert isinstance(gv_np, np.ndarray)
    np.testing.assert_array_equal(gv_np, outs[3].cpu().numpy())
    # grad_sigma=False is the plain predict, which may take a small-batch route: same numbers, not the same bits
    np.testing.assert_allclose(gp.predictive_gradients(x), gm_np, rtol=1e-11, atol=1e-14)


@pytest.mark.parametrize("n_out", [1, 4])
def test_predict_grad_follows_model_updates(n_out):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(40 + n_out)
    D, N = 3, 900
    Z = rng.uniform(-1, 1, (N, D))
    Y = rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.5, (n_out, D))
    sf2 = rng.uniform(0.5, 1.5, n_out)
    noise = np.full(n_out, 1e-2 + 1e-5)
    gps = []
    for _ in range(2):                                     # two handles alive, both with grown workspaces
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp_from(ls, sf2, noise))
        gp.train(Z, Y, opt_hyp=False)
        gps.append(gp)
    x = rng.uniform(-0.8, 0.8, (300, D))
    before = [gp.predict_device_grad(x)[3].cpu().numpy() for gp in gps]
    np.testing.assert_array_equal(before[0], before[1])
    Zn, Yn = rng.uniform(-1, 1, (40, D)), rng.standard_normal((40, n_out))
    gps[0].update_model(Zn, Yn, replace_old=False)
    jv = gps[0].predict_device_grad(x)[3].cpu().numpy()
    beta, inv_K, _ = orc.gp_fit(gps[0].z_fit, gps[0].y_z, ls, sf2, noise)
    assert not np.allclose(jv, before[0])
    for t in range(0, 300, 15):
        rjv, _ = orc.gp_linearize_extras(x[t], gps[0].z_fit, beta, inv_K, ls, sf2)
        np.testing.assert_allclose(jv[t], rjv, rtol=1e-9, atol=1e-11 * sf2.max() / ls.min() ** 2)
    np.testing.assert_array_equal(gps[1].predict_device_grad(x)[3].cpu().numpy(), before[1])


_NT_CHECK = r"""
import ctypes, sys
import numpy as np
import torch
lib = ctypes.CDLL(sys.argv[1])
f = lib.sr_test_gemm_nt
f.restype = ctypes.c_int
f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p,
              ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
dev = torch.device("cuda", 0)
rng = np.random.default_rng(1)
def run(A, Bm, M, N, K):
    a = torch.from_numpy(np.ascontiguousarray(A)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(Bm)).to(dev)
    c = torch.full((M, N), float("nan"), dtype=torch.float64, device=dev)
    rc = f(0, a.data_ptr(), A.shape[1], b.data_ptr(), Bm.shape[1], c.data_ptr(), N, M, N, K, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return c.cpu().numpy()
# identity A against an asymmetric B: C == B exactly (catches a row/column swap and a wrong swizzle)
M = N = K = 256
Bm = np.arange(K * N, dtype=np.float64).reshape(K, N) * 1.0 + 0.25 * np.arange(K)[:, None] ** 2
C = run(np.eye(M), Bm, M, N, K)
np.testing.assert_array_equal(C, Bm)
# a rectangular product with a row stride beyond K
M, N, K, lda = 384, 256, 208, 240
A = rng.standard_normal((M, lda))
Bm = rng.standard_normal((K, N))
C = run(A, Bm, M, N, K)
np.testing.assert_allclose(C, A[:, :K] @ Bm, rtol=1e-12, atol=1e-12 * K)
print("NT OK")
"""


def test_nt_main_loop_identity_lab():
    """srt::mainloop_nt_glds (A read along its rows, swizzled LDS-DMA) through the lab build's test entry."""
    lab = os.path.join(ROOT, "scripts", "_bin", "libsafereach_lab.so")
    if not os.path.exists(lab):
        pytest.skip("lab build missing (make -C safe_exploration_amd/csrc lab)")
    r = subprocess.run([sys.executable, "-c", _NT_CHECK, lab], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NT OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
