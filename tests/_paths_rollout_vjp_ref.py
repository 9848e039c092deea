"""NumPy reference of the reverse pass of the consistent roll-out (sr_gp_paths_rollout_vjp, include/safereach.h).  With
x_0[s] the start, z_i[s] = [x_i[s], K[i] x_i[s] + k[i]], x_{i+1}[s] = f_s(z_i[s]), J_i[s] = d f_s / d z at z_i[s] (n_s x D,
columns [J_x | J_u]) and L = sum_{i,s} X_bar[i][s] . x_{i+1}[s], per path

    lambda = X_bar[H-1][s]
    for i = H-1 .. 0:
        g = J_i[s]^T lambda                        g_x = g[:n_s], g_u = g[n_s:]
        k_bar[i] += g_u                            (summed over s)
        K_bar[i] += g_u x_i[s]^T                   (summed over s)
        lambda = (i >= 1 ? X_bar[i-1][s] : 0) + g_x + K[i]^T g_u
    x0_bar[s] = lambda

sweep() is that recursion on given Jacobians in the dtype asked for (np.float64 or np.longdouble); vjp() forms the inputs from
the stored states, takes J from _paths_grad_ref.step_grad and sweeps."""
import numpy as np

import _paths_grad_ref as pg


def sweep(J, X_prev, X_bar, K, dtype=np.float64):
    """J (H, S, n_s, D), X_prev (H, S, n_s) = x_0 .. x_{H-1}, X_bar (H, S, n_s), K (H, n_u, n_s) ->
    x0_bar (S, n_s) per path, K_bar (H, n_u, n_s), k_bar (H, n_u), all of `dtype`"""
    J, X_prev, X_bar, K = (np.asarray(a, dtype=dtype) for a in (J, X_prev, X_bar, K))
    H, S, n_s, _ = J.shape
    K_bar, k_bar = np.zeros(K.shape, dtype=dtype), np.zeros(K.shape[:2], dtype=dtype)
    lam = X_bar[H - 1].copy()
    for i in range(H - 1, -1, -1):
        g = np.einsum("sdj,sd->sj", J[i], lam)
        g_x, g_u = g[:, :n_s], g[:, n_s:]
        k_bar[i] = g_u.sum(axis=0)
        K_bar[i] = np.einsum("sq,sc->qc", g_u, X_prev[i])
        lam = g_x + g_u.dot(K[i])
        if i >= 1:
            lam = lam + X_bar[i - 1]
    return lam, K_bar, k_bar


def sweep_abs(J, X_prev, X_bar, K, dtype=np.longdouble):
    """the same polynomials in the absolute values of their arguments: the scale of their forward-error bounds"""
    return sweep(*(np.abs(np.asarray(a, dtype=dtype)) for a in (J, X_prev, X_bar, K)), dtype=dtype)


def states_before(x0, X_all):
    """X_prev (H, S, n_s): the start (one for all paths, or one per path), then X_all[:-1] (X_all[H-1] is not read)"""
    H, S, n_s = X_all.shape
    x0 = np.asarray(x0, dtype=np.float64)
    first = np.tile(x0.reshape(1, n_s), (S, 1)) if x0.size == n_s and x0.shape != (S, n_s) else x0.reshape(S, n_s)
    return np.concatenate((first[None], X_all[:H - 1]), axis=0)


def inputs(X_prev, K, k, i):
    return np.hstack((X_prev[i], X_prev[i].dot(K[i].T) + k[i][None, :]))


def jacobians(X_prev, K, k, Z, ls, sf2, omega, tau, w, c):
    """J (H, S, n_s, D) at the inputs the stored states give"""
    return np.stack([pg.step_grad(inputs(X_prev, K, k, i), Z, ls, sf2, omega, tau, w, c) for i in range(K.shape[0])])


def vjp(x0, K, k, X_all, X_bar, Z, ls, sf2, omega, tau, w, c):
    """(x0_bar (S, n_s) per path, K_bar, k_bar, J); a shared start's gradient is x0_bar.sum(0)"""
    X_prev = states_before(x0, X_all)
    J = jacobians(X_prev, K, k, Z, ls, sf2, omega, tau, w, c)
    return sweep(J, X_prev, X_bar, K) + (J,)
