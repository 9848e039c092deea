"""Reference side of the sparse-GP tests: the DTC / VarDTC posterior

    Sigma = K_uu + K_uf K_fu / s2,  beta = Sigma^-1 K_uf y / s2,  M = K_uu^-1 - Sigma^-1   (K_uu includes jit I)
    mu(x) = k_u(x)^T beta,  var(x) = k(x, x) - k_u(x)^T M k_u(x)

restated twice: in fp64 NumPy on the oracle's kernels (``sparse_fit_np``) and in ``np.longdouble`` (80-bit on x86) with
kernels, products, Cholesky factorisation and triangular inversion written out here (``sparse_fit_ld``) -- the truth the
device is compared with, and the yardstick ``e_ref`` = |fp64 restatement - truth|."""
import numpy as np
import scipy.linalg as sla

from oracle import oracle_np as orc

LD = np.longdouble
SQRT5_LD = np.sqrt(LD(5))


def _f(v):
    return np.asarray(v, dtype=np.float64).reshape(-1)


def kernel_matrix_ld(kern_type, hyp, x, y):
    """orc.kernel_matrix in long double with direct (x - y)^2 distances."""
    x, y = np.asarray(x, LD), np.asarray(y, LD)

    def stat(kind, xa, ya, var, ls):
        ls = np.asarray(_f(ls), LD) * np.ones(xa.shape[1], LD)
        d = xa[:, None, :] / ls - ya[None, :, :] / ls
        r2 = (d * d).sum(-1)
        if kind == "rbf":
            return LD(var) * np.exp(-r2 / 2)
        r = np.sqrt(r2)
        return LD(var) * (1 + SQRT5_LD * r + LD(5) / 3 * r2) * np.exp(-SQRT5_LD * r)

    def lin(xa, ya, v):
        v = np.asarray(_f(v), LD) * np.ones(xa.shape[1], LD)
        return (xa * v).dot(ya.T)

    if kern_type in ("rbf", "mat52"):
        return stat(kern_type, x, y, hyp["variance"], hyp["lengthscale"])
    st = "rbf" if kern_type == "lin_rbf" else "mat52"
    x1, y1 = x[:, 1:2], y[:, 1:2]
    return (lin(x1, y1, hyp["prod.linear.variances"]) * stat(st, x1, y1, hyp["prod.%s.variance" % st],
                                                            hyp["prod.%s.lengthscale" % st])
            + lin(x, y, hyp["linear.variances"]))


def kernel_diag_ld(kern_type, hyp, x):
    return np.array([kernel_matrix_ld(kern_type, hyp, x[t:t + 1], x[t:t + 1])[0, 0] for t in range(x.shape[0])], LD)


def chol_ld(A):
    """lower Cholesky factor, column by column, in the dtype of A; LinAlgError on a non-positive pivot"""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        s = A[j, j] - (L[j, :j] ** 2).sum()
        if not s > 0:
            raise np.linalg.LinAlgError("pivot %d not positive" % (j + 1))
        L[j, j] = np.sqrt(s)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j].dot(L[j, :j])) / L[j, j]
    return L


def trinv_ld(L):
    """inverse of a lower triangular matrix by forward substitution over all columns at once"""
    n = L.shape[0]
    X = np.zeros_like(L)
    eye = np.eye(n, dtype=L.dtype)
    for i in range(n):
        X[i] = (eye[i] - L[i, :i].dot(X[:i])) / L[i, i]
    return X


def sparse_fit_ld(kern_types, hyp, Zu, X, Y, s2, jit):
    """truth: beta (m, n_out), M list of (m, m), both long double"""
    m = Zu.shape[0]
    beta, Ms = np.empty((m, Y.shape[1]), LD), []
    for d, (kt, hp) in enumerate(zip(kern_types, hyp)):
        Kuu = kernel_matrix_ld(kt, hp, Zu, Zu) + LD(jit) * np.eye(m, dtype=LD)
        Kuf = kernel_matrix_ld(kt, hp, Zu, X)
        Sig = Kuu + Kuf.dot(Kuf.T) / LD(s2[d])
        Li, Si = trinv_ld(chol_ld(Kuu)), trinv_ld(chol_ld(Sig))
        Ms.append(Li.T.dot(Li) - Si.T.dot(Si))
        beta[:, d] = Si.T.dot(Si.dot(Kuf.dot(np.asarray(Y[:, d], LD)))) / LD(s2[d])
    return beta, Ms


def sparse_fit_np(kern_types, hyp, Zu, X, Y, s2, jit):
    """the same formulas in fp64 on the oracle's kernels (two Cholesky inversions); also returns cond(K_uu) per output"""
    m = Zu.shape[0]
    beta, Ms, conds = np.empty((m, Y.shape[1])), [], []
    for d, (kt, hp) in enumerate(zip(kern_types, hyp)):
        Kuu = orc.kernel_matrix(kt, hp, Zu, Zu) + jit * np.eye(m)
        Kuf = orc.kernel_matrix(kt, hp, Zu, X)
        Sig = Kuu + Kuf.dot(Kuf.T) / s2[d]
        Li = sla.solve_triangular(np.linalg.cholesky(Kuu), np.eye(m), lower=True)
        Si = sla.solve_triangular(np.linalg.cholesky(Sig), np.eye(m), lower=True)
        Ms.append(Li.T.dot(Li) - Si.T.dot(Si))
        beta[:, d] = Si.T.dot(Si.dot(Kuf.dot(Y[:, d]))) / s2[d]
        conds.append(np.linalg.cond(Kuu))
    return beta, Ms, conds


def predict_any(kern_types, hyp, Zu, beta, Ms, xq, ld=False):
    """mu, var (T, n_out), unclipped, in fp64 or long double arithmetic"""
    T = xq.shape[0]
    dt = LD if ld else np.float64
    mu, var = np.empty((T, beta.shape[1]), dt), np.empty((T, beta.shape[1]), dt)
    for d, (kt, hp) in enumerate(zip(kern_types, hyp)):
        if ld:
            ks, kxx = kernel_matrix_ld(kt, hp, xq, Zu), kernel_diag_ld(kt, hp, xq)
        else:
            ks, kxx = orc.kernel_matrix(kt, hp, xq, Zu), orc.kernel_diag(kt, hp, xq)
        mu[:, d] = ks.dot(np.asarray(beta[:, d], dt))
        var[:, d] = kxx - (ks.dot(np.asarray(Ms[d], dt)) * ks).sum(1)
    return mu, var


def sigma_f2(kern_types, hyp, x):
    """the prior variance scale of each output over the points x (sigma_f^2 of the tolerances)"""
    return np.array([float(np.max(orc.kernel_diag(kt, hp, x))) for kt, hp in zip(kern_types, hyp)])


def make_case(seed, kern_type, n_out, D, m, N, s2=1e-2):
    """uniform data in [-1, 1]^D (lin_*: dimension 1 in [1, 2], where the product kernel's variance does not vanish),
    inducing rows drawn from the data, lengthscales per output around 0.45 of the unit range for D >= 3 and shorter
    below (the condition of K_uu is what the dimension leaves of m points per lengthscale)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (N, D))
    lin = kern_type.startswith("lin_")
    if lin:
        X[:, 1] = rng.uniform(1, 2, N)
    Zu = X[rng.choice(N, m, replace=False)].copy()
    w = rng.uniform(0.5, 1.5, (D, n_out))
    Y = np.sin(X.dot(w)) + np.sqrt(s2) * rng.standard_normal((N, n_out))
    hyp = []
    for d in range(n_out):
        base = {2: 0.12, 3: 0.45}.get(D, 0.5)
        if lin:
            st = "rbf" if kern_type == "lin_rbf" else "mat52"
            hyp.append({"prod.%s.lengthscale" % st: np.array([rng.uniform(0.02, 0.03)]),
                        "prod.%s.variance" % st: float(rng.uniform(0.8, 1.2)),
                        "prod.linear.variances": np.array([rng.uniform(0.8, 1.2)]),
                        "linear.variances": rng.uniform(1e-3, 2e-3, D), "noise_variance": s2 - 1e-5})
        else:
            hyp.append({"lengthscale": rng.uniform(0.9, 1.1, D) * base, "variance": float(rng.uniform(0.8, 1.2)),
                        "noise_variance": s2 - 1e-5})
    xq = rng.uniform(-1, 1, (64, D))
    if lin:
        xq[:, 1] = rng.uniform(1, 2, 64)
    return dict(X=X, Y=Y, Zu=Zu, hyp=hyp, kern_types=[kern_type] * n_out, xq=xq, s2=np.full(n_out, s2))
