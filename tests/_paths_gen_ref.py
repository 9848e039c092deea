"""fp64 NumPy reference of the posterior function samples of the general kernel family with the RBF radial part
(include/safereach.h), on the packed parameters kp (n_out, 3 + 3 D) = [kappa id, v, c0, s[D], a[D], b[D]] per output:

    k(x, y)    = (c0 + sum_j a_j x_j y_j) v exp(-r^2 / 2) + sum_j b_j x_j y_j,   r^2 = sum_j (s_j (x_j - y_j))^2
    base_i(x)  = sqrt(2 v / M) cos(sum_j omega[i][j] s_j x_j + tau[i])                        i < M
    A_0(x) = sqrt(c0),  A_l(x) = sqrt(a_l) x_l  (l = 1 .. D);  the groups: the l, ascending, active on at least one output
    phi(x)     = [A_g(x) base_i(x) at g M + i | sqrt(b_j) x_j at G M + j]                     n_w = G M + D
    c_{d,s}    = K_y,d^-1 (y_d - Phi_d(Z) w_{d,s} - sqrt(n_d) eps_{d,s})
    f_{d,s}(x) = phi_d(x) . w_{d,s} + k_d(x, Z) c_{d,s}

n_d is the diagonal term the handle holds.  Two solve routes for c -- Cholesky and LU -- whose difference is the reference's
own error (the tests' tolerance), as tests/_paths_ref.py has them."""
import numpy as np

import _paths_ref as pr


def unpack(kp_d):
    kp_d = np.asarray(kp_d, dtype=np.float64)
    D = (kp_d.size - 3) // 3
    return kp_d[1], kp_d[2], kp_d[3:3 + D], kp_d[3 + D:3 + 2 * D], kp_d[3 + 2 * D:3 + 3 * D]


def groups(kp):
    """the active l: 0 where c0, l = j + 1 where a_j, is non-zero on at least one output"""
    kp = np.atleast_2d(kp)
    D = (kp.shape[1] - 3) // 3
    act = [0] if np.any(kp[:, 2] != 0.0) else []
    return act + [j + 1 for j in range(D) if np.any(kp[:, 3 + D + j] != 0.0)]


def weight_count(kp, M):
    kp = np.atleast_2d(kp)
    return len(groups(kp)) * M + (kp.shape[1] - 3) // 3


def kernel(x, y, kp_d):
    v, c0, s, a, b = unpack(kp_d)
    df = (x[:, None, :] - y[None, :, :]) * s[None, None, :]
    return (c0 + (x * a[None, :]).dot(y.T)) * v * np.exp(-0.5 * np.sum(df * df, axis=2)) + (x * b[None, :]).dot(y.T)


def dkernel(x, Z, kp_d):
    """d k(x_t, z_i) / d x_tj: (T, N, D)"""
    v, c0, s, a, b = unpack(kp_d)
    diff = x[:, None, :] - Z[None, :, :]
    kap = np.exp(-0.5 * np.sum((diff * s) ** 2, axis=2))
    cl = c0 + (x * a[None, :]).dot(Z.T)
    return ((a * v)[None, None, :] * Z[None, :, :] * kap[:, :, None] - (cl * v * kap)[:, :, None] * (s * s) * diff
            + b[None, None, :] * Z[None, :, :])


def _arg(x, omega, tau, s):
    return (x * s[None, :]).dot(omega.T) + tau[None, :]


def _amps(x, kp_d, grp):
    """A_g(x): (T, G)"""
    _, c0, _, a, _ = unpack(kp_d)
    return np.stack([np.full(x.shape[0], np.sqrt(c0)) if l == 0 else np.sqrt(a[l - 1]) * x[:, l - 1] for l in grp], axis=1) \
        if grp else np.zeros((x.shape[0], 0))


def features(x, omega, tau, kp_d, grp):
    """phi(x): (T, n_w)"""
    v, _, s, _, b = unpack(kp_d)
    M = omega.shape[0]
    base = np.sqrt(2.0 * v / M) * np.cos(_arg(x, omega, tau, s))
    A = _amps(x, kp_d, grp)
    return np.hstack([A[:, g:g + 1] * base for g in range(len(grp))] + [np.sqrt(b)[None, :] * x])


def dfeatures(x, omega, tau, kp_d, grp):
    """d phi(x_t) / d x_tj: (T, n_w, D)"""
    v, _, s, a, b = unpack(kp_d)
    T, D = x.shape
    M = omega.shape[0]
    amp = np.sqrt(2.0 * v / M)
    arg = _arg(x, omega, tau, s)
    base, dbase = amp * np.cos(arg), -amp * np.sin(arg)[:, :, None] * (omega * s[None, :])[None, :, :]      # (T, M), (T, M, D)
    A = _amps(x, kp_d, grp)
    out = np.zeros((T, len(grp) * M + D, D))
    for g, l in enumerate(grp):
        out[:, g * M:(g + 1) * M, :] = A[:, g][:, None, None] * dbase
        if l > 0:
            out[:, g * M:(g + 1) * M, l - 1] += np.sqrt(a[l - 1]) * base
    out[:, len(grp) * M + np.arange(D), np.arange(D)] = np.sqrt(b)[None, :]
    return out


def k_y(Z, kp_d, n_d):
    return kernel(Z, Z, kp_d) + n_d * np.eye(Z.shape[0])


def coeffs(Z, Y, kp, n_diag, omega, tau, w, eps, route="chol"):
    """c: (n_out, N, S) from w (n_out, S, n_w) and eps (n_out, S, N)"""
    grp = groups(kp)
    out = []
    for d in range(Y.shape[1]):
        R = Y[:, d][:, None] - features(Z, omega, tau, kp[d], grp).dot(w[d].T) - np.sqrt(n_diag[d]) * eps[d].T
        out.append(pr.solve(k_y(Z, kp[d], n_diag[d]), R, route))
    return np.stack(out)


def evaluate(x, Z, kp, omega, tau, w, c):
    """every path at every input: (T, S, n_out)"""
    grp = groups(kp)
    F = np.empty((x.shape[0], c.shape[2], c.shape[0]))
    for d in range(c.shape[0]):
        F[:, :, d] = features(x, omega, tau, kp[d], grp).dot(w[d].T) + kernel(x, Z, kp[d]).dot(c[d])
    return F


def evaluate_grad(x, Z, kp, omega, tau, w, c):
    """(T, S, n_out, D)"""
    grp = groups(kp)
    J = np.empty((x.shape[0], c.shape[2], c.shape[0], x.shape[1]))
    for d in range(c.shape[0]):
        J[:, :, d, :] = (np.einsum("tmj,sm->tsj", dfeatures(x, omega, tau, kp[d], grp), w[d])
                         + np.einsum("tnj,ns->tsj", dkernel(x, Z, kp[d]), c[d]))
    return J


def step(xs, Z, kp, omega, tau, w, c):
    """path s at its own input xs[s]: (S, n_out)"""
    grp = groups(kp)
    F = np.empty((xs.shape[0], c.shape[0]))
    for d in range(c.shape[0]):
        F[:, d] = (np.einsum("sm,sm->s", features(xs, omega, tau, kp[d], grp), w[d])
                   + np.einsum("sn,ns->s", kernel(xs, Z, kp[d]), c[d]))
    return F


def step_grad(xs, Z, kp, omega, tau, w, c):
    """(S, n_out, D)"""
    grp = groups(kp)
    J = np.empty((xs.shape[0], c.shape[0], xs.shape[1]))
    for d in range(c.shape[0]):
        J[:, d, :] = (np.einsum("smj,sm->sj", dfeatures(xs, omega, tau, kp[d], grp), w[d])
                      + np.einsum("snj,ns->sj", dkernel(xs, Z, kp[d]), c[d]))
    return J


def rollout(x0, K, k, Z, kp, omega, tau, w, c):
    """closed loop u_i = K[i] x_i + k[i] from the single start x0 (n_s,), every path through its own function:
    (n, S, n_s)"""
    S = c.shape[2]
    x = np.tile(np.asarray(x0, dtype=np.float64).reshape(1, -1), (S, 1))
    out = []
    for i in range(K.shape[0]):
        x = step(np.hstack((x, x.dot(K[i].T) + k[i][None, :])), Z, kp, omega, tau, w, c)
        out.append(x)
    return np.stack(out)
