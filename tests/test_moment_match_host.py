"""The CPU references of exact moment matching (tests/_mm_ref.py) against each other and against the oracle.

The textbook closed form (``moment_match``) against 80-node Gauss-Hermite quadrature over the oracle-style posterior:
mean, full output covariance and cov(x, g) = Sigma G^T V, also for a singular input covariance; its S = 0 limit against
the oracle's mean, variance and mean Jacobian; the state-propagation formula
Sigma+ = (A + V G) Sigma (A + V G)^T + Cov - (V G) Sigma (V G)^T against quadrature.

Bars: 1e-10 for the quadrature comparisons, 1e-12 for the S = 0 identities.  Inputs stay where 80 nodes are far past
convergence: lengthscales >= 0.5, input standard deviation <= 0.3."""
import numpy as np
import pytest

import _mm_ref as R
from oracle import oracle_np as orc


def _model(seed, N, D, n_out, noise=1e-2):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.2, (n_out, D))
    sf2 = rng.uniform(0.5, 1.5, n_out)
    beta, inv_K, _ = orc.gp_fit(Z, Y, ls, sf2, np.full(n_out, noise))
    return dict(Z=Z, alpha=beta.T.copy(), M=np.stack(inv_K), ls=ls, sf2=sf2, beta=beta, inv_K=inv_K)


def _args(md):
    return md["Z"], md["alpha"], md["M"], md["ls"], md["sf2"]


def _check_quadrature(md, mx, Sx, G, g0, tag):
    G = np.asarray(G, float)
    mu, cov, V = R.moment_match(*_args(md), G.dot(mx) + g0, G.dot(Sx).dot(G.T))
    qmu, qcov, qcxg, _ = R.quadrature(*_args(md), mx, Sx, G, g0)
    cxg = np.atleast_2d(Sx).dot(G.T).dot(V.T)
    print("%s: mu %.2e, cov %.2e, cov(x,g) %.2e" % (tag, np.abs(mu - qmu).max(), np.abs(cov - qcov).max(),
                                                   np.abs(cxg - qcxg).max()))
    np.testing.assert_allclose(mu, qmu, rtol=0, atol=1e-10)
    np.testing.assert_allclose(cov, qcov, rtol=0, atol=1e-10)
    np.testing.assert_allclose(cxg, qcxg, rtol=0, atol=1e-10)
    assert np.abs(cov - cov.T).max() == 0.0


def test_one_input_dimension():
    md = _model(1, 25, 1, 1)
    _check_quadrature(md, np.array([0.2]), np.array([[0.3 ** 2]]), np.eye(1), np.zeros(1), "D=1")


def test_two_dimensions_full_rank():
    md = _model(2, 30, 2, 1)
    L = np.array([[0.25, 0.0], [0.1, 0.15]])
    _check_quadrature(md, np.array([0.1, -0.3]), L.dot(L.T), np.eye(2), np.zeros(2), "D=2 full rank")


def test_three_dimensions_rank_one():
    """S = G s^2 G^T of rank 1 in D = 3: nothing in the closed form may invert S"""
    md = _model(3, 30, 3, 1)
    G = np.array([[1.0], [0.6], [-0.8]])
    _check_quadrature(md, np.array([0.15]), np.array([[0.2 ** 2]]), G, np.array([0.0, 0.2, -0.1]), "D=3 rank 1")
    assert np.linalg.matrix_rank(G.dot(G.T)) == 1


def test_two_outputs_with_different_lengthscales():
    md = _model(4, 30, 3, 2)
    assert np.abs(md["ls"][0] - md["ls"][1]).min() > 1e-3
    G = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, -0.7]])
    L = np.array([[0.2, 0.0], [-0.05, 0.25]])
    _check_quadrature(md, np.array([0.1, 0.2]), L.dot(L.T), G, np.array([0.0, 0.0, 0.1]), "two outputs")
    mu, cov, V = R.moment_match(*_args(md), G.dot([0.1, 0.2]), G.dot(L.dot(L.T)).dot(G.T))
    assert abs(cov[0, 1]) > 1e-6                     # the cross-covariance is not a structural zero


def test_point_input_is_the_ordinary_posterior():
    md = _model(5, 40, 3, 2)
    rng = np.random.default_rng(55)
    for x in rng.uniform(-1, 1, (4, 3)):
        rmu, rvar, rjac = orc.gp_predict(x[None], md["Z"], md["beta"], md["inv_K"], md["ls"], md["sf2"])
        for S in (None, np.zeros((3, 3))):
            mu, cov, V = R.moment_match(*_args(md), x, S)
            np.testing.assert_allclose(mu, rmu[0], rtol=0, atol=1e-12)
            np.testing.assert_allclose(np.diag(cov), rvar[0], rtol=0, atol=1e-12)
            np.testing.assert_allclose(V, rjac[0], rtol=0, atol=1e-12)
            assert abs(cov[0, 1]) <= 1e-12 and cov[0, 1] == cov[1, 0]


def test_state_propagation_formula():
    """n_s = 1, n_u = 1, x+ = a x + b (K x + k_ff) + g([x; u]): mean and variance of x+ by quadrature over x"""
    md = _model(6, 30, 2, 1)
    a, b, K = np.array([[0.9]]), np.array([[0.4]]), np.array([[-0.7]])
    mu_x, sigma, k_ff = np.array([0.2]), np.array([[0.25 ** 2]]), np.array([0.1])
    mu_new, sigma_new, cov = R.step(*_args(md), mu_x, sigma, k_ff, K, a, b, np.eye(1))
    G, g0 = np.vstack((np.eye(1), K)), np.array([0.0, k_ff[0]])
    _, _, _, (x, wt, mu, var) = R.quadrature(*_args(md), mu_x, sigma, G, g0)
    nxt = (a + b.dot(K))[0, 0] * x[:, 0] + b[0, 0] * k_ff[0] + mu[:, 0]
    q_mean = wt.dot(nxt)
    q_var = wt.dot((nxt - q_mean) ** 2) + wt.dot(var[:, 0])
    print("propagation: mean %.2e, variance %.2e" % (abs(mu_new[0] - q_mean), abs(sigma_new[0, 0] - q_var)))
    assert abs(mu_new[0] - q_mean) <= 1e-10
    assert abs(sigma_new[0, 0] - q_var) <= 1e-10
    # without feedback and from a point the step is the GP's own moments
    m0, s0, c0 = R.step(*_args(md), mu_x, None, k_ff, None, a, b, np.eye(1))
    rmu, rvar = orc.gp_predict(np.array([[mu_x[0], k_ff[0]]]), md["Z"], md["beta"], md["inv_K"], md["ls"], md["sf2"], False)
    assert abs(m0[0] - (0.9 * mu_x[0] + 0.4 * k_ff[0] + rmu[0, 0])) <= 1e-12 and abs(s0[0, 0] - rvar[0, 0]) <= 1e-12


def test_interface_is_declared():
    """FAILS without the feature: the header, the ctypes table and the Python surface name the new entry point"""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "sr_gp_moment_match" in open(os.path.join(root, "include", "safereach.h")).read()
    src = open(os.path.join(root, "safe_exploration_amd", "_lib.py")).read()
    assert '"sr_gp_moment_match"' in src
    up = open(os.path.join(root, "safe_exploration_amd", "uncertainty_propagation_casadi.py")).read()
    for name in ("MOMENT_MATCHING", "def one_step_moment_matching", "def multi_step_moment_matching",
                 "def moment_matching_batch"):
        assert name in up, name
