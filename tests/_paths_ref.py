"""fp64 NumPy reference of the posterior function samples (pathwise conditioning, include/safereach.h):

    phi_d(x)_i  = sqrt(2 sf2_d / M) cos(sum_j Omega[i][j] x_j / l_d[j] + tau[i])
    r_{d,s}     = y_d - Phi_d(Z) w_{d,s} - sqrt(n_d) eps_{d,s}
    c_{d,s}     = K_y,d^-1 r_{d,s}
    f_{d,s}(x)  = phi_d(x) . w_{d,s} + k_d(x, Z) c_{d,s}

K_y,d = K_d + n_d I is dense, built with the oracle's kernel; n_d = noise_var_d + GPY_JITTER, the diagonal term of a model
made by _helpers.hip_model / hyp_from from the same noise_var (which already includes noise_diag), as oracle.gp_fit forms it.
Two solve routes for c -- Cholesky and LU -- whose difference is the reference's own error (the tests' tolerance)."""
import numpy as np
import scipy.linalg as sla

from oracle import oracle_np as orc


def diag_term(noise_var):
    return np.asarray(noise_var, dtype=np.float64) + orc.GPY_JITTER


def features(x, omega, tau, ls_d, sf2_d):
    """Phi_d(x): (T, M)"""
    M = omega.shape[0]
    return np.sqrt(2.0 * sf2_d / M) * np.cos((x / np.asarray(ls_d).reshape(1, -1)).dot(omega.T) + tau[None, :])


def k_y(Z, ls_d, sf2_d, n_d):
    return orc.rbf_kernel(Z, Z, sf2_d, ls_d) + n_d * np.eye(Z.shape[0])


def solve(Ky, R, route):
    if route == "chol":
        return sla.cho_solve((sla.cholesky(Ky, lower=True), True), R)
    if route == "lu":
        return np.linalg.solve(Ky, R)
    raise ValueError(route)


def coeffs(Z, Y, ls, sf2, noise_var, omega, tau, w, eps, route="chol"):
    """c: (n_out, N, S) from w (n_out, S, M) and eps (n_out, S, N)"""
    n_out = Y.shape[1]
    nd = diag_term(noise_var)
    out = []
    for d in range(n_out):
        R = Y[:, d][:, None] - features(Z, omega, tau, ls[d], sf2[d]).dot(w[d].T) - np.sqrt(nd[d]) * eps[d].T
        out.append(solve(k_y(Z, ls[d], sf2[d], nd[d]), R, route))
    return np.stack(out)


def evaluate(x, Z, ls, sf2, omega, tau, w, c):
    """every path at every input: (T, S, n_out)"""
    n_out = c.shape[0]
    F = np.empty((x.shape[0], c.shape[2], n_out))
    for d in range(n_out):
        F[:, :, d] = features(x, omega, tau, ls[d], sf2[d]).dot(w[d].T) + orc.rbf_kernel(x, Z, sf2[d], ls[d]).dot(c[d])
    return F


def step(xs, Z, ls, sf2, omega, tau, w, c):
    """path s at its own input xs[s]: (S, n_out)"""
    n_out = c.shape[0]
    F = np.empty((xs.shape[0], n_out))
    for d in range(n_out):
        F[:, d] = (np.einsum("sm,sm->s", features(xs, omega, tau, ls[d], sf2[d]), w[d])
                   + np.einsum("sn,ns->s", orc.rbf_kernel(xs, Z, sf2[d], ls[d]), c[d]))
    return F


def rollout(x0, K, k, Z, ls, sf2, omega, tau, w, c):
    """closed loop u_i = K[i] x_i + k[i] from the single start x0 (n_s,), every path through its own function:
    (n, S, n_s)"""
    n, S = K.shape[0], c.shape[2]
    x = np.tile(np.asarray(x0, dtype=np.float64).reshape(1, -1), (S, 1))
    out = []
    for i in range(n):
        inp = np.hstack((x, x.dot(K[i].T) + k[i][None, :]))
        x = step(inp, Z, ls, sf2, omega, tau, w, c)
        out.append(x)
    return np.stack(out)


def path_covariance(x, Z, ls_d, sf2_d, n_d, omega, tau):
    """closed-form covariance of f_d at the rows of x for standard-normal (w, eps), with Q = Phi Phi^T:
    Q(x,x') - Q(x,Z) K_y^-1 k(Z,x') - k(x,Z) K_y^-1 Q(Z,x') + k(x,Z) K_y^-1 (Q(Z,Z) + n I) K_y^-1 k(Z,x')"""
    px, pz = features(x, omega, tau, ls_d, sf2_d), features(Z, omega, tau, ls_d, sf2_d)
    A = np.linalg.solve(k_y(Z, ls_d, sf2_d, n_d), orc.rbf_kernel(Z, x, sf2_d, ls_d))       # K_y^-1 k(Z, x)
    Qxz = px.dot(pz.T)
    return px.dot(px.T) - Qxz.dot(A) - A.T.dot(Qxz.T) + A.T.dot(pz.dot(pz.T) + n_d * np.eye(Z.shape[0])).dot(A)
