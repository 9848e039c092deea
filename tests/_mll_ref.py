"""fp64 CPU reference of the negative log marginal likelihood for the packed kernel family (TEST infrastructure).

    k(x, y) = (c0 + sum_j a_j x_j y_j) v kappa(r) + sum_j b_j x_j y_j ,   r^2 = sum_j (s_j (x_j - y_j))^2
    kappa = exp(-r^2 / 2)  (kind 0)   or   (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)  (kind 1)
    K_y = K + noise I ,   nll = 1/2 y^T K_y^-1 y + 1/2 log det K_y + N/2 log 2 pi

Written from the formula in the header of csrc/sr_train.hip and the layout of SimpleGPModel._pack_kernel_params.  The
gradient in the order of sr_gp_mll, [v, c0, s[D], a[D], b[D], noise], is torch autograd through the Cholesky factor: it
shares no derivation with the device kernel (which sums 1/2 (K_y^-1 - alpha alpha^T) dK/dtheta by hand) nor with
oracle.gp_nll_grad (closed forms per kernel name).  ``noise`` is the value handed to sr_gp_set_data_general: nothing is
added to it here."""
import math

import numpy as np
import torch

KINDS = {"rbf": 0, "mat52": 1}
_SQRT5 = math.sqrt(5.0)
_R2_FLOOR = 1e-300      # under the square root of Matern-5/2: d sqrt / d r2 stays finite on the diagonal (r2 = 0, d r2 = 0)


def _kernel(Z, kind, v, c0, s, a, b):
    """K (N, N) of the packed family; every argument a torch fp64 tensor (kind: 0 / 1)."""
    diff = (Z[:, None, :] - Z[None, :, :]) * s
    r2 = (diff * diff).sum(-1)
    if int(kind) == 0:
        kap = torch.exp(-0.5 * r2)
    else:
        r = torch.sqrt(r2 + _R2_FLOOR)
        kap = (1.0 + _SQRT5 * r + (5.0 / 3.0) * r2) * torch.exp(-_SQRT5 * r)
    return (c0 + (Z * a) @ Z.T) * v * kap + (Z * b) @ Z.T


def _tensors(Z, v, c0, s, a, b, noise, grad):
    D = np.shape(Z)[1]
    t = lambda x, n: torch.tensor(np.broadcast_to(np.asarray(x, dtype=np.float64).reshape(-1), (n,)).copy(),
                                  dtype=torch.float64, requires_grad=grad)
    return (torch.tensor(np.ascontiguousarray(Z, dtype=np.float64)),
            [t(v, 1), t(c0, 1), t(s, D), t(a, D), t(b, D), t(noise, 1)])


def ky_general(Z, kind, v, c0, s, a, b, noise):
    """K_y = K + noise I as a NumPy array."""
    kind = KINDS.get(kind, kind)
    Zt, (tv, tc, ts, ta, tb, tn) = _tensors(Z, v, c0, s, a, b, noise, False)
    return (_kernel(Zt, kind, tv, tc, ts, ta, tb) + tn * torch.eye(Zt.shape[0], dtype=torch.float64)).numpy()


def nll_general(Z, y, kind, v, c0, s, a, b, noise, with_grad=True):
    """nll (float) and its gradient (3 + 3 D,) in the order [v, c0, s[D], a[D], b[D], noise] (None without with_grad).
    ``kind``: "rbf" / "mat52" or 0 / 1.  Raises numpy.linalg.LinAlgError if K_y is not positive definite."""
    kind = KINDS.get(kind, kind)
    Zt, leaves = _tensors(Z, v, c0, s, a, b, noise, with_grad)
    tv, tc, ts, ta, tb, tn = leaves
    N = Zt.shape[0]
    yt = torch.tensor(np.asarray(y, dtype=np.float64).reshape(N, 1))
    Ky = _kernel(Zt, kind, tv, tc, ts, ta, tb) + tn * torch.eye(N, dtype=torch.float64)
    L, info = torch.linalg.cholesky_ex(Ky)
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        raise np.linalg.LinAlgError("K_y is not positive definite (pivot %d)" % int(info))
    alpha = torch.cholesky_solve(yt, L)
    nll = 0.5 * (yt * alpha).sum() + torch.log(torch.diagonal(L)).sum() + 0.5 * N * math.log(2.0 * math.pi)
    if not with_grad:
        return float(nll.detach()), None
    g = torch.autograd.grad(nll, leaves)
    return float(nll.detach()), np.concatenate([x.numpy().reshape(-1) for x in g])


def unpack(kp):
    """One row [kind, v, c0, s[D], a[D], b[D]] of the packed parameters -> the keyword arguments of nll_general."""
    kp = np.asarray(kp, dtype=np.float64).reshape(-1)
    D = (kp.size - 3) // 3
    assert kp.size == 3 + 3 * D
    return dict(kind=int(kp[0]), v=kp[1], c0=kp[2], s=kp[3:3 + D], a=kp[3 + D:3 + 2 * D], b=kp[3 + 2 * D:])


def nll_packed(Z, y, kp, noise, with_grad=True):
    return nll_general(Z, y, noise=noise, with_grad=with_grad, **unpack(kp))


def ky_packed(Z, kp, noise):
    return ky_general(Z, noise=noise, **unpack(kp))


def pack_named(kern_type, hyp, D):
    """The four named kernels as a member of the family (tests/test_mll_host.py holds this against
    SimpleGPModel._pack_kernel_params): rbf / mat52 are c0 = 1, s = 1 / lengthscale; lin_rbf / lin_mat52 act with their
    product part on input dimension 1 alone (s_1, a_1) and carry the ARD linear kernel in b."""
    kp = np.zeros(3 + 3 * D)
    if kern_type in ("rbf", "mat52"):
        kp[0] = KINDS[kern_type]
        kp[1], kp[2] = float(hyp["variance"]), 1.0
        kp[3:3 + D] = 1.0 / (np.asarray(hyp["lengthscale"], dtype=np.float64).reshape(-1) * np.ones(D))
        return kp
    st = {"lin_rbf": "rbf", "lin_mat52": "mat52"}[kern_type]
    kp[0] = KINDS[st]
    kp[1] = float(hyp["prod.%s.variance" % st])
    kp[3 + 1] = 1.0 / float(np.reshape(hyp["prod.%s.lengthscale" % st], (-1,))[0])
    kp[3 + D + 1] = float(np.reshape(hyp["prod.linear.variances"], (-1,))[0])
    kp[3 + 2 * D:] = np.asarray(hyp["linear.variances"], dtype=np.float64).reshape(-1) * np.ones(D)
    return kp


def named_gradient(kern_type, hyp, g, D):
    """The API vector g (3 + 3 D) as the gradient with respect to the named hyper-parameters, keys of
    oracle.gp_nll_grad (chain rule s = 1 / lengthscale)."""
    g = np.asarray(g)
    out = {"noise_variance": g[-1:]}
    if kern_type in ("rbf", "mat52"):
        ell = np.asarray(hyp["lengthscale"], dtype=np.float64).reshape(-1) * np.ones(D)
        out["variance"] = g[0:1]
        out["lengthscale"] = -g[2:2 + D] / ell ** 2
        return out
    st = {"lin_rbf": "rbf", "lin_mat52": "mat52"}[kern_type]
    ell = float(np.reshape(hyp["prod.%s.lengthscale" % st], (-1,))[0])
    out["prod.%s.variance" % st] = g[0:1]
    out["prod.%s.lengthscale" % st] = np.array([-g[2 + 1] / ell ** 2])
    out["prod.linear.variances"] = g[2 + D + 1:2 + D + 2]
    out["linear.variances"] = g[2 + 2 * D:2 + 3 * D]
    return out


def general_case(seed, N, D, kind, noise=0.05):
    """A genuinely general member: c0, every s_j, a_j, b_j positive, targets with structure.  Parameters of order one and
    b small keep cond(K_y) <= (N max|K| + noise) / noise near 1e5 (asserted by the callers, not assumed)."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (N, D))
    w = rng.standard_normal(D) / np.sqrt(D)
    y = np.sin(2.0 * Z.dot(w)) + 0.3 * Z[:, 0] + 0.05 * rng.standard_normal(N)
    return dict(Z=Z, y=y, kind=kind, v=float(rng.uniform(0.5, 1.5)), c0=float(rng.uniform(0.3, 1.2)),
                s=rng.uniform(0.4, 1.6, D) / np.sqrt(max(D, 3) / 3.0), a=rng.uniform(0.2, 1.0, D),
                b=rng.uniform(0.02, 0.2, D), noise=float(noise))


def case_kp(case):
    """packed row [kind, v, c0, s, a, b] of a general_case"""
    return np.concatenate([[KINDS.get(case["kind"], case["kind"]), case["v"], case["c0"]], case["s"], case["a"], case["b"]])
