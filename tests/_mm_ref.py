"""fp64 NumPy references of exact moment matching (the GP at a Gaussian input z ~ N(m, S)) -- TEST infrastructure.

``moment_match``: the textbook form, unexpanded: zeta_ij = L_a^-1 nu_i + L_b^-1 nu_j, the exponent
-1/2 nu_i^T L_a^-1 nu_i - 1/2 nu_j^T L_b^-1 nu_j + 1/2 zeta^T R^-1 S zeta, explicit ``np.linalg`` inverses and determinants.
It takes the model as arrays (Z, alpha, M, ls, sf2) and shares no algebra with the device kernel's expanded exponent.

``quadrature``: Gauss-Hermite evaluation of the same three quantities over the posterior mean / variance of the oracle's
``gp_predict`` form, for x of dimension 1 or 2 mapped through z = G x + g0.

``propagate``: the state propagation of uncertainty_propagation_casadi.moment_matching_batch composed from
``moment_match``, one trajectory."""
import numpy as np


def moment_match(Z, alpha, M, ls, sf2, m, S):
    """Z (N,D); alpha (n,N); M (n,N,N) (K_y^-1 per output); ls (n,D); sf2 (n,); m (D,); S (D,D) PSD, may be singular.
    -> mu (n,), cov (n,n), V (n,D) with cov(z, g_a) = S V_a."""
    Z, alpha, M = np.asarray(Z, float), np.asarray(alpha, float), np.asarray(M, float)
    ls, sf2 = np.asarray(ls, float), np.asarray(sf2, float)
    n, D = ls.shape
    nu = Z - np.asarray(m, float)[None, :]
    S = np.zeros((D, D)) if S is None else np.asarray(S, float)
    eye = np.eye(D)
    mu, V, q = np.empty(n), np.empty((n, D)), []
    for a in range(n):
        Lam = np.diag(ls[a] ** 2)
        Ainv = np.linalg.inv(S + Lam)
        det = np.linalg.det(S.dot(np.linalg.inv(Lam)) + eye)
        qa = sf2[a] / np.sqrt(det) * np.exp(-0.5 * np.einsum("id,de,ie->i", nu, Ainv, nu))
        mu[a] = alpha[a].dot(qa)
        V[a] = Ainv.dot(nu.T.dot(alpha[a] * qa))
        q.append(qa)
    cov = np.empty((n, n))
    for a in range(n):
        for b in range(a, n):
            Lai, Lbi = np.diag(1.0 / ls[a] ** 2), np.diag(1.0 / ls[b] ** 2)
            R = S.dot(Lai + Lbi) + eye
            RiS = np.linalg.solve(R, S)
            sign, logdet = np.linalg.slogdet(R)
            assert sign > 0
            za, zb = nu.dot(Lai), nu.dot(Lbi)                                  # rows L_a^-1 nu_i, L_b^-1 nu_j
            zeta = za[:, None, :] + zb[None, :, :]                             # (N, N, D)
            quad = np.einsum("ijd,de,ije->ij", zeta, RiS, zeta)
            ea = np.sum(nu * za, axis=1)
            eb = np.sum(nu * zb, axis=1)
            logq = np.log(sf2[a] * sf2[b]) - 0.5 * logdet - 0.5 * ea[:, None] - 0.5 * eb[None, :] + 0.5 * quad
            Q = np.exp(logq)
            c = alpha[a].dot(Q).dot(alpha[b]) - mu[a] * mu[b]
            if a == b:
                c += sf2[a] - np.sum(M[a] * Q)
            cov[a, b] = cov[b, a] = c
    return mu, cov, V


def moment_match_batch(Z, alpha, M, ls, sf2, m, S):
    """rows of m (T,D) / S (T,D,D) or None -> mu (T,n), cov (T,n,n), V (T,n,D); diagonal of cov clipped at 1e-15"""
    outs = [moment_match(Z, alpha, M, ls, sf2, m[t], None if S is None else S[t]) for t in range(len(m))]
    mu, cov, V = (np.stack([o[k] for o in outs]) for k in range(3))
    idx = np.arange(cov.shape[1])
    cov[:, idx, idx] = np.maximum(cov[:, idx, idx], 1e-15)
    return mu, cov, V


def posterior(Z, alpha, M, ls, sf2, z):
    """mean (P,n) and variance (P,n) of the GP posterior at points z (P,D): mu = k* alpha, var = sf2 - k* M k*^T"""
    n = ls.shape[0]
    mu, var = np.empty((z.shape[0], n)), np.empty((z.shape[0], n))
    for a in range(n):
        d = (z[:, None, :] - Z[None, :, :]) / ls[a][None, None, :]
        k = sf2[a] * np.exp(-0.5 * np.sum(d * d, axis=2))
        mu[:, a] = k.dot(alpha[a])
        var[:, a] = sf2[a] - np.sum(k.dot(M[a]) * k, axis=1)
    return mu, var


def quadrature(Z, alpha, M, ls, sf2, mx, Sx, G, g0, nodes=80):
    """x ~ N(mx, Sx) of dimension 1 or 2 (Sx positive definite), z = G x + g0.
    -> E[mu(z)] (n,), E[mu mu^T] - E[mu] E[mu]^T + diag E[var] (n,n), cov(x, mu(z)) (dim,n), and the nodes' (x, weights)."""
    mx, Sx = np.atleast_1d(np.asarray(mx, float)), np.atleast_2d(np.asarray(Sx, float))
    dim = mx.shape[0]
    assert dim in (1, 2)
    xi, w = np.polynomial.hermite_e.hermegauss(nodes)
    w = w / np.sqrt(2.0 * np.pi)
    if dim == 1:
        pts, wt = xi[:, None], w
    else:
        a, b = np.meshgrid(xi, xi, indexing="ij")
        pts, wt = np.stack((a.ravel(), b.ravel()), axis=1), np.outer(w, w).ravel()
    x = mx[None, :] + pts.dot(np.linalg.cholesky(Sx).T)
    z = x.dot(np.asarray(G, float).T) + np.asarray(g0, float)[None, :]
    mu, var = posterior(Z, alpha, M, ls, sf2, z)
    e_mu = wt.dot(mu)
    cov = (mu * wt[:, None]).T.dot(mu) - np.outer(e_mu, e_mu) + np.diag(wt.dot(var))
    cxg = ((x - mx[None, :]) * wt[:, None]).T.dot(mu - e_mu[None, :])
    return e_mu, cov, cxg, (x, wt, mu, var)


def step(Z, alpha, M, ls, sf2, mu_x, sigma, k_ff, K, a, b, tz):
    """One exact step for x+ = a x + b u + g(z), u = K x + k_ff, z = [tz; K] x + [0; k_ff]; sigma / K None = point input
    without feedback.  -> mu_new (n_s,), sigma_new (n_s,n_s), Cov of the GP outputs (n_s,n_s)."""
    n_s, n_u = mu_x.shape[0], k_ff.shape[0]
    Kz = np.zeros((n_u, n_s)) if K is None else K
    G = np.vstack((tz, Kz))
    A = a + b.dot(Kz)
    zbar = G.dot(mu_x) + np.concatenate((np.zeros(tz.shape[0]), k_ff))
    S = None if sigma is None else G.dot(sigma).dot(G.T)
    mu_g, cov, V = moment_match(Z, alpha, M, ls, sf2, zbar, S)
    idx = np.arange(n_s)
    cov[idx, idx] = np.maximum(cov[idx, idx], 1e-15)
    mu_new = A.dot(mu_x) + b.dot(k_ff) + mu_g
    if sigma is None:
        return mu_new, cov, cov
    VG = V.dot(G)
    Hm = A + VG
    return mu_new, Hm.dot(sigma).dot(Hm.T) + cov - VG.dot(sigma).dot(VG.T), cov


def propagate(Z, alpha, M, ls, sf2, mu_0, k_ff, k_fb, a, b, sigma_0=None, tz=None):
    """One trajectory: k_ff (H,n_u), k_fb (H-1,n_u,n_s) -> mu_all (H,n_s), sigma_all (H,n_s,n_s), cov_all (H,n_s,n_s)"""
    n_s = mu_0.shape[0]
    tz = np.eye(n_s) if tz is None else tz
    mu, sigma = mu_0, sigma_0
    mus, sigmas, covs = [], [], []
    for i in range(k_ff.shape[0]):
        mu, sigma, cov = step(Z, alpha, M, ls, sf2, mu, sigma, k_ff[i], None if i == 0 else k_fb[i - 1], a, b, tz)
        mus.append(mu), sigmas.append(sigma), covs.append(cov)
    return np.stack(mus), np.stack(sigmas), np.stack(covs)
