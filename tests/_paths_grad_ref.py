"""fp64 NumPy reference of the Jacobian of the posterior function samples (include/safereach.h), on the coefficients of
tests/_paths_ref.py (coeffs by either solve route):

    d f_{d,s}(x) / d x_j = - sqrt(2 sf2_d / M) / l_dj * sum_i sin(omega_i . x / l_d + tau_i) omega_ij w_{d,s,i}
                           + sf2_d / l_dj^2        * sum_i exp(-r_i^2 / 2) (z_ij - x_j) c_{d,s,i}

The kernel part is formed on the explicit differences Z - x (never expanded around a centre), so that it stays exact when
inputs and data are translated together."""
import numpy as np

import _paths_ref as pr


def features_grad(x, omega, tau, ls_d, sf2_d):
    """d Phi_d(x) / d x: (T, M, D)"""
    ls_d = np.asarray(ls_d, dtype=np.float64).reshape(-1)
    M = omega.shape[0]
    s = np.sin((x / ls_d[None, :]).dot(omega.T) + tau[None, :])
    return -np.sqrt(2.0 * sf2_d / M) * s[:, :, None] * (omega / ls_d[None, :])[None, :, :]


def kernel_grad(x, Z, ls_d, sf2_d):
    """d k_d(x, Z) / d x: (T, N, D), from the differences Z - x themselves"""
    ls_d = np.asarray(ls_d, dtype=np.float64).reshape(-1)
    diff = Z[None, :, :] - x[:, None, :]                               # (T, N, D)
    k = sf2_d * np.exp(-0.5 * np.sum((diff / ls_d) ** 2, axis=2))
    return k[:, :, None] * diff / ls_d ** 2


def evaluate_grad(x, Z, ls, sf2, omega, tau, w, c):
    """every path at every input: J (T, S, n_out, D)"""
    n_out, D = c.shape[0], x.shape[1]
    J = np.empty((x.shape[0], c.shape[2], n_out, D))
    for d in range(n_out):
        J[:, :, d, :] = (np.einsum("tmj,sm->tsj", features_grad(x, omega, tau, ls[d], sf2[d]), w[d])
                         + np.einsum("tnj,ns->tsj", kernel_grad(x, Z, ls[d], sf2[d]), c[d]))
    return J


def step_grad(xs, Z, ls, sf2, omega, tau, w, c):
    """path s at its own input xs[s]: J (S, n_out, D)"""
    n_out, D = c.shape[0], xs.shape[1]
    J = np.empty((xs.shape[0], n_out, D))
    for d in range(n_out):
        J[:, d, :] = (np.einsum("smj,sm->sj", features_grad(xs, omega, tau, ls[d], sf2[d]), w[d])
                      + np.einsum("snj,ns->sj", kernel_grad(xs, Z, ls[d], sf2[d]), c[d]))
    return J


def rollout_grad(x0, K, k, Z, ls, sf2, omega, tau, w, c):
    """the closed loop of _paths_ref.rollout with the transition Jacobian of every step and particle:
    states (n, S, n_s) and A (n, S, n_s, n_s), A[i] = J_i[..., :n_s] + J_i[..., n_s:] K[i] = d x_{i+1} / d x_i"""
    n, S = K.shape[0], c.shape[2]
    n_s = c.shape[0]
    x = np.tile(np.asarray(x0, dtype=np.float64).reshape(1, -1), (S, 1))
    out, A = [], []
    for i in range(n):
        inp = np.hstack((x, x.dot(K[i].T) + k[i][None, :]))
        J = step_grad(inp, Z, ls, sf2, omega, tau, w, c)
        A.append(J[:, :, :n_s] + J[:, :, n_s:].dot(K[i]))
        x = pr.step(inp, Z, ls, sf2, omega, tau, w, c)
        out.append(x)
    return np.stack(out), np.stack(A)
