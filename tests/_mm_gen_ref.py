"""NumPy references of exact moment matching for the general kernel family with the RBF radial part -- TEST infrastructure.

    k_a(x, z) = v_a (c0_a + sum_j a_aj x_j z_j) exp(-1/2 sum_j s_aj^2 (x_j - z_j)^2) + sum_j b_aj x_j z_j

The model is a dict ``par`` of arrays v (n,), c0 (n,), s (n, D), a (n, D), b (n, D) (``params_from_packed``: the rows
[kappa id, v, c0, s, a, b] of sr_gp_set_data_general) beside Z (N, D), alpha (n, N) and M (n, N, N) (K_y^-1 per output).

``moment_match``: the closed form, unexpanded and in the conditioning ("Kalman") form, which shares no algebra with the device
kernels: the RBF factor of output a is a Gaussian observation of the rows I_a = {j : s_aj != 0} of x with covariance
Lam_a = diag(1 / s_aj^2), so with H the stacked selectors, y the stacked nu and Sig = H S H^T + blockdiag(Lam) (an explicit
inverse, of S + Lam on the dimensions where s != 0 only)
    E[prod e] = sqrt(prod |Lam| / |Sig|) exp(-1/2 y^T Sig^-1 y),   x | tilt ~ N(m + S H^T Sig^-1 y, S - S H^T Sig^-1 H S)
for one factor (single tilt) and for two (double tilt).  All four terms of E[k_ai k_bj] are formed inside one N x N array; no
separation of the sums.  ``dtype=np.longdouble`` runs the same code in extended precision (own Gauss-Jordan inverse, NumPy's
linalg is fp64 only): the rounding floor the GPU bars rest on.

``quadrature``: tensor Gauss-Hermite over z ~ N(m, S), D <= 3, of the posterior mean / variance computed from the plain kernel
formula.

``propagate``: uncertainty_propagation_casadi.moment_matching_batch composed from ``moment_match``, one trajectory."""
import numpy as np


def params_from_packed(kp):
    kp = np.asarray(kp, float)
    D = (kp.shape[1] - 3) // 3
    assert np.all(kp[:, 0] == 0.0), "RBF radial part only"
    return {"v": kp[:, 1].copy(), "c0": kp[:, 2].copy(), "s": kp[:, 3:3 + D].copy(), "a": kp[:, 3 + D:3 + 2 * D].copy(),
            "b": kp[:, 3 + 2 * D:3 + 3 * D].copy()}


def kernel(par, o, X, Y):
    """k_o(X, Y): (P, D), (Q, D) -> (P, Q), the plain formula"""
    d = (X[:, None, :] - Y[None, :, :]) * par["s"][o][None, None, :]
    lin = lambda w: (X * w[None, :]).dot(Y.T)
    return par["v"][o] * (par["c0"][o] + lin(par["a"][o])) * np.exp(-0.5 * np.sum(d * d, axis=2)) + lin(par["b"][o])


def kernel_diag(par, o, X):
    return par["c0"][o] * par["v"][o] + np.sum((par["a"][o] * par["v"][o] + par["b"][o])[None, :] * X * X, axis=1)


def fit(par, Z, Y, noise):
    """alpha (n, N) and M = K_y^-1 (n, N, N) in NumPy fp64 (the host tests' model)"""
    n = par["v"].shape[0]
    M = np.stack([np.linalg.inv(kernel(par, o, Z, Z) + noise[o] * np.eye(Z.shape[0])) for o in range(n)])
    M = 0.5 * (M + np.transpose(M, (0, 2, 1)))
    return np.stack([M[o].dot(Y[:, o]) for o in range(n)]), M


def _inv(A):
    """inverse and determinant; np.linalg in fp64, Gauss-Jordan with partial pivoting in any other dtype"""
    k = A.shape[0]
    if k == 0:
        return A.copy(), A.dtype.type(1)
    if A.dtype == np.float64:
        return np.linalg.inv(A), np.linalg.det(A)
    W = np.concatenate((A.copy(), np.eye(k, dtype=A.dtype)), axis=1)
    det = A.dtype.type(1)
    for c in range(k):
        p = c + int(np.argmax(np.abs(W[c:, c])))
        if p != c:
            W[[c, p]] = W[[p, c]]
            det = -det
        det = det * W[c, c]
        W[c] = W[c] / W[c, c]
        for r in range(k):
            if r != c:
                W[r] = W[r] - W[r, c] * W[c]
    return W[:, k:], det


def _tilt(S, sels, lams):
    """H (k, D), Sig^-1, sqrt(prod |Lam| / |Sig|) of the stacked observation"""
    D = S.shape[0]
    H = np.concatenate([np.eye(D, dtype=S.dtype)[I] for I in sels], axis=0).reshape(-1, D)
    lam = np.concatenate(lams)
    Sig = H.dot(S).dot(H.T) + np.diag(lam)
    Si, det = _inv(Sig)
    return H, Si, np.sqrt(np.prod(lam) / det)


def moment_match(par, Z, alpha, M, m, S, dtype=np.float64):
    """m (D,); S (D, D) PSD, may be singular, or None -> mu (n,), cov (n, n) (diagonal NOT clipped), V (n, D), and the scales
    (sum_i |alpha_ai| max_i |E k_ai| (n,), E[k_a(x, x)] (n,)) of the bars"""
    f = lambda x: np.asarray(x, dtype=dtype)
    Z, alpha, M, m = f(Z), f(alpha), f(M), f(m)
    n, D = par["s"].shape
    S = np.zeros((D, D), dtype=dtype) if S is None else f(S)
    v, c0, s, av, bv = (f(par[k]) for k in ("v", "c0", "s", "a", "b"))
    nu = Z - m[None, :]
    eye = np.eye(D, dtype=dtype)
    sel = [np.nonzero(par["s"][o] != 0.0)[0] for o in range(n)]
    lam = [1.0 / s[o][sel[o]] ** 2 for o in range(n)]
    SM = S + np.outer(m, m)
    q, mt, St, c, Ek = [], [], [], [], []
    mu, V = np.empty(n, dtype=dtype), np.empty((n, D), dtype=dtype)
    for o in range(n):
        H, Si, nrm = _tilt(S, [sel[o]], [lam[o]])
        y = nu[:, sel[o]]                                            # (N, k)
        G = S.dot(H.T).dot(Si)                                       # (D, k)
        q.append(nrm * np.exp(-0.5 * np.einsum("ik,kl,il->i", y, Si, y)))
        mt.append(m[None, :] + y.dot(G.T))                           # tilted means (N, D)
        St.append(S - G.dot(H).dot(S))                               # tilted covariance
        az, bz = Z * av[o][None, :], Z * bv[o][None, :]
        c.append(c0[o] + np.sum(mt[o] * az, axis=1))
        Ek.append(v[o] * q[o] * c[o] + bz.dot(m))
        mu[o] = alpha[o].dot(Ek[o])
        # (I + Li S)^-1 Li nu = H^T Sig^-1 y ;  (I + Li S)^-1 = I - H^T Sig^-1 H S
        inner = c[o][:, None] * y.dot(Si).dot(H) + az.dot((eye - H.T.dot(Si).dot(H).dot(S)).T)
        V[o] = alpha[o].dot(v[o] * q[o][:, None] * inner + bz)
    cov = np.empty((n, n), dtype=dtype)
    N = Z.shape[0]
    for a in range(n):
        for b in range(a, n):
            H, Si, nrm = _tilt(S, [sel[a], sel[b]], [lam[a], lam[b]])
            ka = len(sel[a])
            y = np.concatenate((np.broadcast_to(nu[:, None, sel[a]], (N, N, ka)),
                                np.broadcast_to(nu[None, :, sel[b]], (N, N, len(sel[b])))), axis=2)      # (N, N, k)
            G = S.dot(H.T).dot(Si)
            Q = nrm * np.exp(-0.5 * np.einsum("ijk,kl,ijl->ij", y, Si, y))
            mh = m[None, None, :] + y.dot(G.T)                       # (N, N, D)
            Mt = S - G.dot(H).dot(S)
            aza, azb = Z * av[a][None, :], Z * av[b][None, :]
            bza, bzb = Z * bv[a][None, :], Z * bv[b][None, :]
            E = v[a] * v[b] * Q * ((c0[a] + np.einsum("ijd,id->ij", mh, aza)) * (c0[b] + np.einsum("ijd,jd->ij", mh, azb))
                                   + aza.dot(Mt).dot(azb.T))
            E = E + (v[a] * q[a] * c[a])[:, None] * mt[a].dot(bzb.T) + (v[a] * q[a])[:, None] * aza.dot(St[a]).dot(bzb.T)
            E = E + ((v[b] * q[b] * c[b])[:, None] * mt[b].dot(bza.T) + (v[b] * q[b])[:, None] * azb.dot(St[b]).dot(bza.T)).T
            E = E + bza.dot(SM).dot(bzb.T)
            w = np.outer(alpha[a], alpha[b])
            if a == b:
                w = w - M[a]
            cab = np.sum(w * E) - mu[a] * mu[b]
            if a == b:
                cab = cab + c0[a] * v[a] + np.sum((av[a] * v[a] + bv[a]) * np.diag(SM))
            cov[a, b] = cov[b, a] = cab
    mu_scale = np.array([np.abs(alpha[o]).sum() * np.abs(Ek[o]).max() for o in range(n)], dtype=np.float64)
    kxx = np.array([c0[o] * v[o] + np.sum((av[o] * v[o] + bv[o]) * np.diag(SM)) for o in range(n)], dtype=np.float64)
    return mu, cov, V, (mu_scale, kxx)


def moment_match_batch(par, Z, alpha, M, m, S, dtype=np.float64):
    """rows of m (T, D) / S (T, D, D) or None -> mu (T, n), cov (T, n, n), V (T, n, D) and the scales (T, n) each; the diagonal
    of cov is clipped at 1e-15"""
    outs = [moment_match(par, Z, alpha, M, m[t], None if S is None else S[t], dtype) for t in range(len(m))]
    mu, cov, V = (np.stack([o[k] for o in outs]) for k in range(3))
    idx = np.arange(cov.shape[1])
    cov[:, idx, idx] = np.maximum(cov[:, idx, idx], 1e-15)
    return mu, cov, V, (np.stack([o[3][0] for o in outs]), np.stack([o[3][1] for o in outs]))


def posterior(par, Z, alpha, M, X):
    """mean (P, n) and variance (P, n) of the posterior at points X (P, D), from the plain kernel formula"""
    n = par["v"].shape[0]
    mu, var = np.empty((X.shape[0], n)), np.empty((X.shape[0], n))
    for o in range(n):
        k = kernel(par, o, X, Z)
        mu[:, o] = k.dot(alpha[o])
        var[:, o] = kernel_diag(par, o, X) - np.sum(k.dot(M[o]) * k, axis=1)
    return mu, var


def quadrature(par, Z, alpha, M, m, S, nodes):
    """tensor Gauss-Hermite, D <= 3, any PSD S (its symmetric square root from the eigen-decomposition)
    -> E[mu] (n,), E[mu mu^T] + diag E[var] - E[mu] E[mu]^T (n, n), E[(x - m) mu^T] (D, n)"""
    m = np.asarray(m, float)
    D = m.shape[0]
    assert D <= 3
    S = np.zeros((D, D)) if S is None else np.asarray(S, float)
    xi, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / np.sqrt(2.0 * np.pi)
    ev, U = np.linalg.eigh(S)
    live = np.nonzero(ev > 1e-14 * max(ev.max(), 1e-300))[0]           # directions without spread need one node
    grids = np.meshgrid(*([xi] * len(live)), indexing="ij") if len(live) else []
    wts = np.meshgrid(*([w] * len(live)), indexing="ij") if len(live) else []
    pts = np.stack([g.ravel() for g in grids], axis=1) if len(live) else np.zeros((1, 0))
    wt = np.prod(np.stack([g.ravel() for g in wts], axis=1), axis=1) if len(live) else np.ones(1)
    X = m[None, :] + (pts * np.sqrt(ev[live])[None, :]).dot(U[:, live].T)
    mu, var = posterior(par, Z, alpha, M, X)
    e_mu = wt.dot(mu)
    cov = (mu * wt[:, None]).T.dot(mu) - np.outer(e_mu, e_mu) + np.diag(wt.dot(var))
    cxg = ((X - m[None, :]) * wt[:, None]).T.dot(mu)
    return e_mu, cov, cxg


def step(par, Z, alpha, M, mu_x, sigma, k_ff, K, a, b, tz):
    """One exact step for x+ = a x + b u + g(z), u = K x + k_ff, z = [tz; K] x + [0; k_ff]; sigma / K None = point input
    without feedback.  -> mu_new (n_s,), sigma_new (n_s, n_s), Cov of the GP outputs (n_s, n_s)."""
    n_s, n_u = mu_x.shape[0], k_ff.shape[0]
    Kz = np.zeros((n_u, n_s)) if K is None else K
    G = np.vstack((tz, Kz))
    A = a + b.dot(Kz)
    zbar = G.dot(mu_x) + np.concatenate((np.zeros(tz.shape[0]), k_ff))
    S = None if sigma is None else G.dot(sigma).dot(G.T)
    mu_g, cov, V, _ = moment_match(par, Z, alpha, M, zbar, S)
    idx = np.arange(n_s)
    cov[idx, idx] = np.maximum(cov[idx, idx], 1e-15)
    mu_new = A.dot(mu_x) + b.dot(k_ff) + mu_g
    if sigma is None:
        return mu_new, cov, cov
    VG = V.dot(G)
    Hm = A + VG
    return mu_new, Hm.dot(sigma).dot(Hm.T) + cov - VG.dot(sigma).dot(VG.T), cov


def propagate(par, Z, alpha, M, mu_0, k_ff, k_fb, a, b, sigma_0=None, tz=None):
    """One trajectory: k_ff (H, n_u), k_fb (H - 1, n_u, n_s) -> mu_all (H, n_s), sigma_all (H, n_s, n_s), cov_all (H, n_s, n_s)"""
    n_s = mu_0.shape[0]
    tz = np.eye(n_s) if tz is None else tz
    mu, sigma = mu_0, sigma_0
    mus, sigmas, covs = [], [], []
    for i in range(k_ff.shape[0]):
        mu, sigma, cov = step(par, Z, alpha, M, mu, sigma, k_ff[i], None if i == 0 else k_fb[i - 1], a, b, tz)
        mus.append(mu), sigmas.append(sigma), covs.append(cov)
    return np.stack(mus), np.stack(sigmas), np.stack(covs)
