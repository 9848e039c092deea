"""References of the reverse pass (vector-Jacobian product) of exact moment matching -- TEST infrastructure.

The scalar differentiated is  L = mu_bar . mu + sum_ab cov_bar_ab Cov_ab + sum_a V_bar_a . V_a  of the three outputs of
``_mm_ref.moment_match`` at one Gaussian input N(m, S), with Cov the unclipped closed form; the results are dL/dm (D,) and
dL/dS (D, D), the latter exactly symmetric: the gradient of the function extended to unsymmetric arguments by
S -> (S + S^T) / 2.

``vjp``: the analytic form in NumPy, in any floating dtype (np.float64, np.longdouble) and in two summation orders:
``order="direct"`` keeps y_ij = R^-T zeta_ij per (i, j) and contracts t_ij y_ij y_ij^T as it stands; ``order="rowsum"`` keeps
row sums r_i = sum_j t_ij, g_i = sum_j t_ij nu_j and the column sums, and assembles the second moment from
Ya [sum_i r_i nu_i nu_i^T] Ya^T + Ya [sum_i nu_i g_i^T] Yb^T + transpose + Yb [sum_j c_j nu_j nu_j^T] Yb^T.
Every D x D inverse is a Cholesky inverse of S + (a positive diagonal), written out here so that it runs in long double.

``moment_match_torch`` / ``step_torch`` / ``propagate_torch``: torch fp64 ports of the textbook forward of
``_mm_ref.moment_match`` and of ``_mm_ref.step`` / ``propagate`` (explicit ``torch.linalg`` inverses and determinants; they
share no algebra with ``vjp``), so that autograd gives an independent second reference.  The clip of the covariance
diagonal at 1e-15 is left out: the derivative ignores it by convention."""
import numpy as np

# The fp64 rounding floor of ``vjp`` itself: both summation orders in np.float64 against the direct order in np.longdouble
# with the same alpha and K_y^-1, at the size edges N = 1, 2, 63, 64, 65, 255, 256, 257, 300 (D = 3, two outputs, noise 1e-2,
# S full rank and zero), as a multiple of the scale the result carries:
#   seeds on mu or V:  sigma_f |alpha|_1 |seed|_1 / min ls        worst 1.402e-16 (N = 1; 2e-17 from N = 63 on)
#   seeds on Cov:      max sf2 |Cs|_1 / min ls^2                  worst 5.22e-13 (N = 257; 1.2e-16 at N <= 2, 4e-14 at N = 65)
# (tests/test_moment_match_grad_host.py measures them again and holds them against these constants).  The two references,
# ``vjp`` and autograd through ``moment_match_torch``, disagree by at most 8.7e-17 and 6.7e-13 of the same scales there.
# A device result is held to MARGIN floors: its summation order and its exp differ from both.
FLOOR_MEAN, FLOOR_COV, MARGIN = 1.41e-16, 5.3e-13, 30.0     # (the two worst cases, rounded up)


def bars(alpha, ls, sf2, mu_bar=None, cov_bar=None, V_bar=None):
    """absolute bar of m_bar and S_bar per query, (T,), from seeds (T, ..) or None: MARGIN floors at the seeds' scales"""
    alpha, ls, sf2 = np.asarray(alpha, float), np.asarray(ls, float), np.asarray(sf2, float)
    s1 = np.sqrt(sf2.max()) * np.abs(alpha).sum(1).max() / ls.min()
    s2 = sf2.max() / ls.min() ** 2
    bar = 0.0
    if mu_bar is not None:
        bar = bar + FLOOR_MEAN * s1 * np.abs(mu_bar).sum(axis=-1)
    if V_bar is not None:
        bar = bar + FLOOR_MEAN * s1 * np.abs(V_bar).sum(axis=(-2, -1))
    if cov_bar is not None:
        Cs = 0.5 * (np.asarray(cov_bar) + np.swapaxes(cov_bar, -2, -1))
        bar = bar + FLOOR_COV * s2 * np.abs(Cs).sum(axis=(-2, -1))
    return MARGIN * np.atleast_1d(bar)


def _chol_inv(X):
    """inverse and log-determinant of a symmetric positive definite matrix, in the dtype of X"""
    n = X.shape[0]
    L = np.zeros_like(X)
    for k in range(n):
        L[k, k] = np.sqrt(X[k, k] - L[k, :k].dot(L[k, :k]))
        for i in range(k + 1, n):
            L[i, k] = (X[i, k] - L[i, :k].dot(L[k, :k])) / L[k, k]
    Li = np.zeros_like(X)
    for j in range(n):
        for i in range(j, n):
            Li[i, j] = ((1.0 if i == j else 0.0) - L[i, j:i].dot(Li[j:i, j])) / L[i, i]
    return Li.T.dot(Li), 2.0 * np.sum(np.log(np.diag(L)))


def vjp(Z, alpha, M, ls, sf2, m, S, mu_bar=None, cov_bar=None, V_bar=None, dtype=np.float64, order="direct"):
    """Z (N,D); alpha (n,N); M (n,N,N); ls (n,D); sf2 (n,); m (D,); S (D,D) PSD or None; seeds mu_bar (n,), cov_bar (n,n),
    V_bar (n,D), None = zero.  -> m_bar (D,), S_bar (D,D) in ``dtype``."""
    Z, alpha, M, ls, sf2, m = (np.asarray(x, dtype=dtype) for x in (Z, alpha, M, ls, sf2, m))
    n, D = ls.shape
    N = Z.shape[0]
    S = np.zeros((D, D), dtype=dtype) if S is None else np.asarray(S, dtype=dtype)
    S = (S + S.T) / 2
    mu_bar = np.zeros(n, dtype=dtype) if mu_bar is None else np.asarray(mu_bar, dtype=dtype)
    cov_bar = np.zeros((n, n), dtype=dtype) if cov_bar is None else np.asarray(cov_bar, dtype=dtype)
    V_bar = np.zeros((n, D), dtype=dtype) if V_bar is None else np.asarray(V_bar, dtype=dtype)
    Cs = (cov_bar + cov_bar.T) / 2
    nu = Z - m[None, :]
    half = dtype(0.5)
    # the forward's mean quantities
    A, An, aq = [], [], []
    mu, V = np.zeros(n, dtype=dtype), np.zeros((n, D), dtype=dtype)
    for a in range(n):
        Aa, logdet = _chol_inv(S + np.diag(ls[a] ** 2))
        logdet = logdet - np.sum(np.log(ls[a] ** 2))                      # log |S L_a^-1 + I|
        Ana = nu.dot(Aa)
        q = sf2[a] * np.exp(-half * logdet - half * np.sum(Ana * nu, axis=1))
        A.append(Aa), An.append(Ana), aq.append(alpha[a] * q)
        mu[a] = np.sum(aq[a])
        V[a] = Aa.dot(nu.T.dot(aq[a]))
    m_bar, S_bar = np.zeros(D, dtype=dtype), np.zeros((D, D), dtype=dtype)
    for a in range(n):
        h = A[a].dot(V_bar[a])
        me = mu_bar[a] - 2 * Cs[a].dot(mu)
        c = aq[a] * (me + nu.dot(h))
        m_bar += An[a].T.dot(c) - mu[a] * h
        S_bar += half * (An[a] * c[:, None]).T.dot(An[a]) - half * np.sum(c) * A[a] \
            - half * (np.outer(h, V[a]) + np.outer(V[a], h))
    for a in range(n):
        for b in range(n):
            la, lb = 1 / ls[a] ** 2, 1 / ls[b] ** 2
            Ld = la + lb
            Bm, logdet = _chol_inv(S + np.diag(1 / Ld))                    # Ld R^-1 = (Ld^-1 + S)^-1
            logdet = logdet + np.sum(np.log(Ld))                           # log |R|
            RiS = np.diag(1 / Ld) - Bm / Ld[:, None] / Ld[None, :]         # R^-1 S
            RT = Bm / Ld[None, :]                                          # R^-T
            za, zb = nu * la[None, :], nu * lb[None, :]
            w = np.outer(alpha[a], alpha[b]) - (M[a] if a == b else 0)
            lead = np.log(sf2[a] * sf2[b]) - half * logdet
            ea, eb = np.sum(nu * za, axis=1), np.sum(nu * zb, axis=1)
            if order == "direct":
                zeta = za[:, None, :] + zb[None, :, :]
                quad = np.einsum("ijd,de,ije->ij", zeta, RiS, zeta)
                t = w * np.exp(lead - half * ea[:, None] - half * eb[None, :] + half * quad)
                y = zeta.dot(RT.T)
                ty = t[:, :, None] * y
                m_bar += Cs[a, b] * np.sum(ty, axis=(0, 1))
                S_bar += Cs[a, b] * (half * np.einsum("ijd,ije->de", ty, y) - half * np.sum(t) * Bm)
            else:
                zaR, zbR = za.dot(RiS), zb.dot(RiS)
                si = lead - half * ea + half * np.sum(zaR * za, axis=1)
                sj = -half * eb + half * np.sum(zbR * zb, axis=1)
                t = w * np.exp(si[:, None] + sj[None, :] + zaR.dot(zb.T))
                Ya, Yb = RT * la[None, :], RT * lb[None, :]
                r, cc, g = np.sum(t, axis=1), np.sum(t, axis=0), t.dot(nu)
                R1, R1c = nu.T.dot(r), nu.T.dot(cc)
                R2, R2c, X = (nu * r[:, None]).T.dot(nu), (nu * cc[:, None]).T.dot(nu), nu.T.dot(g)
                cross = Ya.dot(X).dot(Yb.T)
                m_bar += Cs[a, b] * (Ya.dot(R1) + Yb.dot(R1c))
                S_bar += Cs[a, b] * (half * (Ya.dot(R2).dot(Ya.T) + cross + cross.T + Yb.dot(R2c).dot(Yb.T))
                                     - half * np.sum(r) * Bm)
    return m_bar, (S_bar + S_bar.T) / 2


def vjp_batch(Z, alpha, M, ls, sf2, m, S, mu_bar=None, cov_bar=None, V_bar=None, **kw):
    """rows of m (T,D) / S (T,D,D) or None and of the seeds -> m_bar (T,D), S_bar (T,D,D)"""
    outs = [vjp(Z, alpha, M, ls, sf2, m[t], None if S is None else S[t], None if mu_bar is None else mu_bar[t],
                None if cov_bar is None else cov_bar[t], None if V_bar is None else V_bar[t], **kw)
            for t in range(len(m))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


# ------------------------------------------------------------------------------------------------- torch fp64 ports
def moment_match_torch(Z, alpha, M, ls, sf2, m, S):
    """``_mm_ref.moment_match`` on torch fp64 tensors (m (D,), S (D,D) or None): mu (n,), cov (n,n) unclipped, V (n,D)"""
    import torch
    n, D = ls.shape
    nu = Z - m[None, :]
    S = torch.zeros((D, D), dtype=torch.float64) if S is None else 0.5 * (S + S.t())
    eye = torch.eye(D, dtype=torch.float64)
    mu, V = [], []
    for a in range(n):
        Lam = torch.diag(ls[a] ** 2)
        Ainv = torch.linalg.inv(S + Lam)
        det = torch.linalg.det(S.matmul(torch.linalg.inv(Lam)) + eye)
        qa = sf2[a] / torch.sqrt(det) * torch.exp(-0.5 * torch.einsum("id,de,ie->i", nu, Ainv, nu))
        mu.append(alpha[a].dot(qa))
        V.append(Ainv.matmul(nu.t().matmul(alpha[a] * qa)))
    rows = [[None] * n for _ in range(n)]
    for a in range(n):
        for b in range(a, n):
            Lai, Lbi = torch.diag(1.0 / ls[a] ** 2), torch.diag(1.0 / ls[b] ** 2)
            R = S.matmul(Lai + Lbi) + eye
            RiS = torch.linalg.solve(R, S)
            logdet = torch.linalg.slogdet(R)[1]
            za, zb = nu.matmul(Lai), nu.matmul(Lbi)
            zeta = za[:, None, :] + zb[None, :, :]
            quad = torch.einsum("ijd,de,ije->ij", zeta, RiS, zeta)
            ea, eb = (nu * za).sum(1), (nu * zb).sum(1)
            Q = torch.exp(torch.log(sf2[a] * sf2[b]) - 0.5 * logdet - 0.5 * ea[:, None] - 0.5 * eb[None, :] + 0.5 * quad)
            c = alpha[a].matmul(Q).dot(alpha[b]) - mu[a] * mu[b]
            if a == b:
                c = c + sf2[a] - (M[a] * Q).sum()
            rows[a][b] = rows[b][a] = c
    return torch.stack(mu), torch.stack([torch.stack(r) for r in rows]), torch.stack(V)


def autograd_vjp(Z, alpha, M, ls, sf2, m, S, mu_bar=None, cov_bar=None, V_bar=None):
    """the same VJP by torch autograd through ``moment_match_torch`` (NumPy in, NumPy out)"""
    import torch
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64))
    n, D = np.shape(ls)
    tm = t(m).clone().requires_grad_(True)
    tS = t(np.zeros((D, D)) if S is None else S).clone().requires_grad_(True)
    mu, cov, V = moment_match_torch(t(Z), t(alpha), t(M), t(ls), t(sf2), tm, tS)
    L = torch.zeros((), dtype=torch.float64)
    if mu_bar is not None:
        L = L + (t(mu_bar) * mu).sum()
    if cov_bar is not None:
        L = L + (t(cov_bar) * cov).sum()
    if V_bar is not None:
        L = L + (t(V_bar) * V).sum()
    gm, gS = torch.autograd.grad(L, (tm, tS), allow_unused=True)
    gm = torch.zeros(D, dtype=torch.float64) if gm is None else gm
    gS = torch.zeros((D, D), dtype=torch.float64) if gS is None else gS
    return gm.numpy(), gS.numpy()


def moment_match_analytic(Z, alpha, M, ls, sf2, m, S):
    """the same three outputs as a torch.autograd.Function on the CPU: forward ``_mm_ref.moment_match`` in NumPy, backward
    ``vjp`` -- the second way to a propagated gradient (the model arguments are constants)"""
    import torch
    import _mm_ref as R
    arrs = tuple(x.detach().numpy() for x in (Z, alpha, M, ls, sf2))

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, m, S):
            ctx.save_for_backward(m, S)
            return tuple(torch.from_numpy(o) for o in R.moment_match(*arrs, m.numpy(), S.numpy()))

        @staticmethod
        def backward(ctx, mu_bar, cov_bar, V_bar):
            m, S = ctx.saved_tensors
            gm, gS = vjp(*arrs, m.numpy(), S.numpy(), mu_bar.numpy(), cov_bar.numpy(), V_bar.numpy())
            return torch.from_numpy(gm), torch.from_numpy(gS)

    D = ls.shape[1]
    return Fn.apply(m, torch.zeros((D, D), dtype=torch.float64) if S is None else 0.5 * (S + S.t()))


def step_torch(model, mu_x, sigma, k_ff, K, a, b, tz, mm=moment_match_torch):
    """``_mm_ref.step`` on torch tensors (model = (Z, alpha, M, ls, sf2) as tensors)"""
    import torch
    n_s, n_u = mu_x.shape[0], k_ff.shape[0]
    Kz = torch.zeros((n_u, n_s), dtype=torch.float64) if K is None else K
    G = torch.cat((tz, Kz), dim=0)
    A = a + b.matmul(Kz)
    zbar = G.matmul(mu_x) + torch.cat((torch.zeros(tz.shape[0], dtype=torch.float64), k_ff))
    S = None if sigma is None else G.matmul(sigma).matmul(G.t())
    mu_g, cov, V = mm(*model, zbar, S)
    mu_new = A.matmul(mu_x) + b.matmul(k_ff) + mu_g
    if sigma is None:
        return mu_new, cov, cov
    VG = V.matmul(G)
    Hm = A + VG
    return mu_new, Hm.matmul(sigma).matmul(Hm.t()) + cov - VG.matmul(sigma).matmul(VG.t()), cov


def propagate_torch(model, mu_0, k_ff, k_fb, a, b, sigma_0=None, tz=None, mm=moment_match_torch):
    """``_mm_ref.propagate`` on torch tensors, one trajectory -> mu_all (H,n_s), sigma_all (H,n_s,n_s), cov_all (H,n_s,n_s)"""
    import torch
    n_s = mu_0.shape[0]
    tz = torch.eye(n_s, dtype=torch.float64) if tz is None else tz
    mu, sigma = mu_0, sigma_0
    mus, sigmas, covs = [], [], []
    for i in range(k_ff.shape[0]):
        mu, sigma, cov = step_torch(model, mu, sigma, k_ff[i], None if i == 0 else k_fb[i - 1], a, b, tz, mm)
        mus.append(mu), sigmas.append(sigma), covs.append(cov)
    return torch.stack(mus), torch.stack(sigmas), torch.stack(covs)


def propagate_grad(arrs, mu_0, k_ff, k_fb, a, b, sigma_0, tz, w_mu, w_sigma, analytic=False):
    """gradient of sum(w_mu * mu_all) + sum(w_sigma * sigma_all) of one trajectory in (mu_0, sigma_0 | None, k_ff, k_fb) by
    autograd through ``propagate_torch`` -- through the torch port of the forward, or (analytic) through ``vjp``"""
    import torch
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64))
    leaves = [None if x is None else t(x).clone().requires_grad_(True) for x in (mu_0, sigma_0, k_ff, k_fb)]
    mm = moment_match_analytic if analytic else moment_match_torch
    mu_all, sigma_all, _ = propagate_torch(tuple(t(x) for x in arrs), leaves[0], leaves[2], leaves[3], t(a), t(b), leaves[1],
                                           t(tz), mm)
    L = (t(w_mu) * mu_all).sum() + (t(w_sigma) * sigma_all).sum()
    used = [x for x in leaves if x is not None]
    grads = iter(torch.autograd.grad(L, used))
    return [None if x is None else next(grads).numpy() for x in leaves]
