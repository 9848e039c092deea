"""NumPy statement of the closed form behind ``sr_gp_remove`` and ``sr_gp_loo`` (TEST infrastructure).

The library keeps, per output, Wt = U^-1 (upper triangular, K_y = U^T U, K_y^-1 = Wt Wt^T) with identity padding in FRONT.
Removing index q deletes column q of the factor of K_y^-1 and turns row q, w = Wt[q, q:], into rho e_q -- the product of the
Givens rotations of the column pairs (q, k), k > q, written without the chain:

    p_k^2 = sum_{q <= l < k} w_l^2          rho^2 = p_n^2 = (K_y^-1)_qq
    d_k   = sum_{q <= l < k} w_l x_l        for every other row x = Wt[i, :]
    x'_k  = (p_k x_k - w_k d_k / p_k) / p_{k+1}   (k > q),   x'_k = x_k   (k < q)
    alpha'_i = alpha_i - (d_n(i) / rho^2) alpha_q,   log det K'_y = log det K_y + log rho^2
"""
import numpy as np


def factor(K):
    """Wt = U^-1 with K = U^T U, U upper triangular (the unique upper triangular Wt, positive diagonal, Wt Wt^T = K^-1).
    In the precision of K: LAPACK for float64, plain loops for np.longdouble (the tests compare the algebra entry by entry
    where the rounding of float64, cond(K) eps of the factor's scale, would hide small entries)."""
    n = K.shape[0]
    if K.dtype == np.float64:
        U = np.linalg.cholesky(K).T
        return np.triu(np.linalg.solve(U, np.eye(n)))
    U = np.zeros_like(K)
    for i in range(n):                                    # row i of U from rows 0 .. i-1
        r = K[i, i:] - U[:i, i].dot(U[:i, i:])
        U[i, i:] = r / np.sqrt(r[0])
    W = np.zeros_like(K)
    for i in range(n - 1, -1, -1):                        # U W = I, row i of W from rows i+1 ..
        e = np.zeros(n, dtype=K.dtype)
        e[i] = 1
        W[i] = (e - U[i, i + 1:].dot(W[i + 1:])) / U[i, i]
    return np.triu(W)


def pad_front(Wt, alpha, Np):
    """the library's layout: Np - n identity rows and columns in front, alpha zero there"""
    n = Wt.shape[0]
    out = np.eye(Np, dtype=Wt.dtype)
    out[Np - n:, Np - n:] = Wt
    a = np.zeros(Np, dtype=Wt.dtype)
    a[Np - n:] = alpha
    return out, a


def remove(Wt, alpha, q):
    """(Wt, alpha) n x n, n and index q -> (Wt', alpha', log rho^2) in the layout the library leaves while the padded size
    stays: rows and columns behind q keep their index, those in front of it move one place down, index 0 becomes a row and
    column of the identity (alpha' = 0 there).  Wt'[1:, 1:] is the factor of the remaining rows."""
    n = Wt.shape[0]
    w = Wt[q, q:]
    p2 = np.concatenate((np.zeros(1, dtype=Wt.dtype), np.cumsum(w * w)))           # p2[t] = p_{q+t}^2, t = 0 .. n - q
    p = np.sqrt(p2)
    rho2 = p2[-1]
    X = Wt[:, q:]
    prod = X * w
    d = np.concatenate((np.zeros((n, 1), dtype=Wt.dtype), np.cumsum(prod, axis=1)), axis=1)     # d[:, t] = d_{q+t}
    Xn = np.array(Wt)
    t = np.arange(1, n - q)                                   # columns k = q + t > q
    Xn[:, q + t] = (p[t] * X[:, t] - w[t] * d[:, t] / p[t]) / p[t + 1]
    a_new = alpha - d[:, -1] / rho2 * alpha[q]
    src = np.array([i for i in range(n) if i != q])
    dst = src + (src < q)
    out = np.eye(n, dtype=Wt.dtype)
    out[np.ix_(dst, dst)] = Xn[np.ix_(src, src)]
    a_out = np.zeros(n, dtype=Wt.dtype)
    a_out[dst] = a_new[src]
    return out, a_out, float(np.log(rho2))


def loo(Wt, alpha, y):
    """Leave-one-out posterior of every row (Rasmussen & Williams 5.12) from the rows of Wt: (mu_loo, var_loo);
    var_loo includes the noise term."""
    rho2 = np.sum(Wt * Wt, axis=1)
    return y - alpha / rho2, 1.0 / rho2


def loo_from_inv(inv_K, alpha, y):
    """the same from the explicit inverse"""
    rho2 = np.diag(inv_K)
    return y - alpha / rho2, 1.0 / rho2


def redundancy_scores(alpha, var_loo):
    """alpha, var_loo (N, n_out) -> score (N,): sum_d alpha_dj^2 var_loo[d, j] (Csato & Opper), summed over the outputs; the
    row to retire is the first argmin."""
    return np.sum(np.asarray(alpha) ** 2 * np.asarray(var_loo), axis=1)
