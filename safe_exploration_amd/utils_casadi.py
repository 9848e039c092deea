"""The MPC objective of the reference's journal experiments, numeric and batched.

Numeric counterparts of the reference's safe_exploration/utils_casadi.py (trig_prop :178-234, trig_aug :237-278, generic_cost
:281-307, cost_dev_safe_perf :310-324, loss_sat :327-363, loss_quadratic :366-395) with the same names and argument orders, NumPy
in and out: ``generic_cost`` over a moment trajectory with ``trig_aug`` as the state transformation and ``loss_sat`` as stage and
terminal cost is what every journal experiment minimises (defaultconfig_episode.py:118-164).

On the device: ``rollout_cost_batch`` (``sr_rollout_cost``: T trajectories x H stored states in one launch) and its reverse pass
``rollout_cost_vjp_batch`` (``sr_rollout_cost_vjp``, one launch), whose outputs are shaped like, and are, the seeds mu_all_bar /
sigma_all_bar (p_all_bar / q_all_bar) that ``multistep_moments_vjp_batch``, ``moment_matching_rollout_vjp_batch`` and
``multistep_reachability_vjp_batch`` take: the gradient of the objective in k_ff, k_fb is three library calls with no autograd
graph, or ``rollout_cost_batch(differentiable=True)`` on top of one of the ``*_diff_batch`` roll-outs.

The saturating loss 1 - exp(-d^T W (I + S W)^-1 d / 2) / sqrt|I + S W| is computed, here and on the device, from a factor
W = F F^T (symmetric PSD, may be singular: ``diag(20, 0, 0, 0, 5) / 100`` is the reference's) and the Cholesky factor of
I + F^T S F, which is SPD for every PSD S: nothing inverts S, W or the unsymmetric I + S W (the reference warns about its own
inverse), and ``expm1`` / ``log1p`` keep the digits of a cost of 1e-9 at the target.  The variance of the trigonometric features is
written without the cancellation of E[.^2] - E[.]^2: exactly zero for a point.
"""
import numpy as np
import torch

from . import _buffers as B
from ._lib import lib, check

LOSSES = {"sat": 0, "quadratic": 1}


# ---- host functions under the reference's names ---------------------------------------------------------------------------------
def trig_prop(m, v, idx, a=1.0):
    """Exact moments of [a sin x, a cos x] for x ~ N(m[idx], v[idx, idx]) (utils_casadi.py:178-234).
    Returns m_out (2,1), v_out (2,2) and c_out (d,2) = inv(v) times the input-output covariance (cov(x, out) = v c_out)."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    v = np.asarray(v, dtype=np.float64)
    th, s2 = m[idx], v[idx, idx]
    e, x, h = np.exp(-s2), -np.expm1(-s2), np.exp(-0.5 * s2)
    m_out = a * h * np.array([[np.sin(th)], [np.cos(th)]])
    c2, s2t = np.cos(2 * th), np.sin(2 * th)
    v_out = 0.5 * a * a * x * np.array([[1 + e * c2, -e * s2t], [-e * s2t, 1 - e * c2]])
    c_out = np.zeros((m.size, 2))
    c_out[idx, 0] = m_out[1, 0]
    c_out[idx, 1] = -m_out[0, 0]
    return m_out, v_out, c_out


def trig_aug(m, v, idx, a=1.0, keep_radian=False):
    """The Gaussian state augmented with a sin / a cos of coordinate idx (utils_casadi.py:237-278): m_aug (d+1 | d+2, 1) and
    v_aug, the angle's own row and column deleted unless keep_radian."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 1)
    v = np.asarray(v, dtype=np.float64)
    v = 0.5 * (v + v.T)
    m_trig, v_trig, c_trig = trig_prop(m, v, idx, a)
    c = v.dot(c_trig)
    m_aug = np.vstack((m, m_trig))
    v_aug = np.vstack((np.hstack((v, c)), np.hstack((c.T, v_trig))))
    if not keep_radian:
        m_aug = np.delete(m_aug, idx, axis=0)
        v_aug = np.delete(np.delete(v_aug, idx, axis=0), idx, axis=1)
    return m_aug, v_aug


def factor_weight(W, n):
    """F (n,n) with W = F F^T for a symmetric PSD W (None: the identity), by eigendecomposition with the tiny negative eigenvalues
    clipped to zero.  ValueError for a wrong shape, an unsymmetric or an indefinite W."""
    if W is None:
        return np.eye(n)
    W = np.asarray(B.to_numpy(W) if B.is_tensor(W) else W, dtype=np.float64)
    if W.shape != (n, n):
        raise ValueError("W must be ({0}, {0}), got {1}".format(n, W.shape))
    scale = np.abs(W).max()
    if not np.isfinite(scale) or np.abs(W - W.T).max() > 1e-12 * scale:
        raise ValueError("W must be finite and symmetric")
    lam, vec = np.linalg.eigh(0.5 * (W + W.T))
    if lam.min() < -1e-12 * max(scale, np.finfo(np.float64).tiny):
        raise ValueError("W must be positive semi-definite (smallest eigenvalue {:.3e})".format(lam.min()))
    return vec * np.sqrt(np.clip(lam, 0.0, None))


def _sat(F, d, v):
    Bm = np.eye(F.shape[1]) + F.T.dot(0.5 * (v + v.T)).dot(F)
    Lb = np.linalg.cholesky(0.5 * (Bm + Bm.T))
    y = np.linalg.solve(Lb, F.T.dot(d))
    return float(-np.expm1(-0.5 * y.dot(y) - np.log(np.diag(Lb)).sum()))


def loss_sat(m, v, z, W=None):
    """Saturating cost 1 - exp(-(m-z)^T W (I + v W)^-1 (m-z) / 2) / sqrt|I + v W| (utils_casadi.py:327-363).  As the reference
    returns a casadi Function of (m, v), this returns a callable ``(m, v) -> float``; the arguments m, v given here fix nothing but
    may be None.  W symmetric PSD, may be singular (ValueError when indefinite)."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    F = factor_weight(W, z.size)

    def l_sat(m, v):
        m = np.asarray(m, dtype=np.float64).reshape(-1)
        v = np.zeros((z.size, z.size)) if v is None else np.asarray(v, dtype=np.float64)
        if m.size != z.size or v.shape != (z.size, z.size):
            raise ValueError("m must have {0} entries and v be ({0}, {0})".format(z.size))
        return _sat(F, m - z, v)
    return l_sat


def loss_quadratic(m, z, v=None, W=None):
    """(m-z)^T W (m-z) + tr(W v) (utils_casadi.py:366-395)."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    F = factor_weight(W, m.size)
    y = F.T.dot(m - z)
    l_var = 0.0 if v is None else np.trace(F.T.dot(np.asarray(v, dtype=np.float64)).dot(F))
    return float(y.dot(y) + l_var)


def generic_cost(mu, sigma, u, step_cost, terminal_cost, state_trafo=None, lambd=1.0):
    """sum_{i < T-1} step_cost(trafo(mu_i, sigma_i), u_i) + terminal_cost(trafo(mu_{T-1}, sigma_{T-1})) (utils_casadi.py:281-307).
    mu (T,n_s); sigma (T,n_s*n_s) or (T,n_s,n_s); u (T',n_u), T' >= T - 1.  state_trafo None: the identity (the reference's default
    is a tuple by mistake).  lambd is unused, as in the reference."""
    mu = np.asarray(mu, dtype=np.float64)
    T, n_s = mu.shape
    sigma = np.asarray(sigma, dtype=np.float64).reshape(T, n_s, n_s)
    u = np.asarray(u, dtype=np.float64)
    if state_trafo is None:
        state_trafo = lambda m, v: (m, v)
    c = 0.0
    for i in range(T - 1):
        m_i, v_i = state_trafo(mu[i].reshape(n_s, 1), sigma[i])
        c += step_cost(m_i, v_i, u[i].reshape(-1, 1))
    m_T, v_T = state_trafo(mu[-1].reshape(n_s, 1), sigma[-1])
    c += terminal_cost(m_T, v_T)
    return c


def cost_dev_safe_perf(m_safe, m_perf, W=None):
    """Quadratic cost on the deviation between the safety and the performance trajectory, steps 1 .. (utils_casadi.py:310-324)."""
    m_safe, m_perf = np.asarray(m_safe, dtype=np.float64), np.asarray(m_perf, dtype=np.float64)
    n_s = m_safe.shape[1]
    if W is None:
        W = 2 * np.eye(n_s)
    cost = 0.0
    for i in range(1, min(m_safe.shape[0], m_perf.shape[0])):
        d = m_perf[i] - m_safe[i]
        cost += float(d.dot(np.asarray(W, dtype=np.float64)).dot(d))
    return cost


# ---- the device surface ---------------------------------------------------------------------------------------------------------
def _prepare(mu_all, sigma_all, z, W, u, R, idx_angle, a, keep_radian, loss, device):
    """Shapes checked, the factor of W computed (host, once per call), everything on the device: the arguments both entry points
    share, in the order of the C ABI after `device`."""
    as_t = B.is_tensor(mu_all)
    shp = tuple(np.shape(mu_all))
    if len(shp) != 3 or shp[1] < 1 or shp[2] < 1:
        raise ValueError("mu_all must be (T, H, n_s) with H >= 1")
    T, H, n_s = shp
    if sigma_all is not None and tuple(np.shape(sigma_all)) != (T, H, n_s, n_s):
        raise ValueError("sigma_all must be {}".format((T, H, n_s, n_s)))
    if loss not in LOSSES:
        raise ValueError("loss must be one of {}, got {!r}".format(sorted(LOSSES), loss))
    idx = -1 if idx_angle is None else int(idx_angle)
    if idx_angle is not None and not 0 <= idx < n_s:
        raise ValueError("idx_angle must be in 0 .. {}".format(n_s - 1))
    if keep_radian and idx < 0:
        raise ValueError("keep_radian needs idx_angle")
    n_c = n_s if idx < 0 else (n_s + 2 if keep_radian else n_s + 1)
    zv = np.asarray(B.to_numpy(z) if B.is_tensor(z) else z, dtype=np.float64).reshape(-1)
    if zv.size != n_c:
        raise ValueError("z must have {} entries (the augmented state)".format(n_c))
    F = factor_weight(W, n_c)
    if (u is None) != (R is None):
        raise ValueError("u and R go together")
    n_u = 0
    if u is not None:
        ushp = tuple(np.shape(u))
        if len(ushp) != 3 or ushp[:2] != (T, H) or ushp[2] < 1:
            raise ValueError("u must be (T, H, n_u)")
        n_u = ushp[2]
        if tuple(np.shape(R)) != (n_u, n_u):
            raise ValueError("R must be ({0}, {0})".format(n_u))
    dev = B.resolve_device(mu_all.device if as_t else device)
    ma, sa, ua = B.as_dev(mu_all, dev), B.as_dev(sigma_all, dev), B.as_dev(u, dev)
    zd, Fd = B.const_dev(zv, dev, (n_c,)), B.const_dev(F, dev, (n_c, n_c))
    Rd = None if R is None else B.const_dev(R, dev, (n_u, n_u))
    head = (dev.index, T, H, n_s, n_u, idx, float(a), int(bool(keep_radian)), LOSSES[loss], B.ptr(zd), B.ptr(Fd))
    tail = (B.ptr(Rd), B.ptr(ma), B.ptr(sa), B.ptr(ua))
    return as_t, dev, (T, H, n_s, n_u), head, tail, (ma, sa, ua, zd, Fd, Rd)


def rollout_cost_batch(mu_all, sigma_all, z, W=None, u=None, R=None, idx_angle=None, a=1.0, keep_radian=False, loss="sat",
                       w_stage=1.0, w_term=1.0, return_steps=False, differentiable=False, device=None):
    """The MPC objective of T moment trajectories in one launch (``sr_rollout_cost``).

    mu_all (T,H,n_s), sigma_all (T,H,n_s,n_s) or None (zero): what the roll-outs return.  Per state the augmentation
    ``trig_aug(m, v, idx_angle, a, keep_radian)`` (idx_angle None: none) and ``loss`` "sat" / "quadratic" against the target z (the
    augmented width) under W (symmetric PSD, may be singular; None: the identity; ValueError when indefinite):
    cost[t] = sum_{i < H-1} (w_stage loss_i + u_i^T R u_i) + w_term loss_{H-1}, the terms added in the order i = 0 .. H - 1.
    u (T,H,n_u) and R (n_u,n_u) go together (row H - 1 of u is not read).  Returns cost (T), with return_steps (cost, cost_steps
    (T,H)).  differentiable (tensors only): the same bits, with an autograd graph to mu_all, sigma_all and u whose backward is one
    ``rollout_cost_vjp_batch`` call (once differentiable; cost_steps carries no gradient).  numpy in -> numpy out, tensors in ->
    tensors out."""
    if differentiable:
        if not B.is_tensor(mu_all):
            raise TypeError("differentiable=True needs tensors")
        cfg = (z, W, R, idx_angle, a, keep_radian, loss, w_stage, w_term, return_steps)
        out = _RolloutCostFn.apply(cfg, mu_all, sigma_all, u)
        return out if return_steps else out[0]
    as_t, dev, (T, H, n_s, n_u), head, tail, keep = _prepare(mu_all, sigma_all, z, W, u, R, idx_angle, a, keep_radian, loss, device)
    cost = B.empty((T,), dev)
    steps = B.empty((T, H), dev) if return_steps else None
    check(lib.sr_rollout_cost(*head, float(w_stage), float(w_term), *tail, B.ptr(cost), B.ptr(steps), B.stream_ptr(dev)))
    outs = (cost, steps) if return_steps else (cost,)
    if not as_t:
        outs = tuple(B.to_numpy(o) for o in outs)
    return outs if return_steps else outs[0]


def rollout_cost_vjp_batch(mu_all, sigma_all, z, W=None, u=None, R=None, idx_angle=None, a=1.0, keep_radian=False, loss="sat",
                           w_stage=1.0, w_term=1.0, cost_bar=None, device=None):
    """Reverse pass of ``rollout_cost_batch`` in one launch (``sr_rollout_cost_vjp``): for the seed cost_bar (T; None = ones) the
    gradients (mu_bar (T,H,n_s), sigma_bar (T,H,n_s,n_s), u_bar (T,H,n_u) or None without u) of sum(cost_bar * cost).  sigma_bar is
    exactly symmetric, also for sigma_all None; u_bar[:, H-1] is zero.  They are the seeds mu_all_bar / sigma_all_bar (p_all_bar /
    q_all_bar) of the roll-outs' reverse passes."""
    as_t, dev, (T, H, n_s, n_u), head, tail, keep = _prepare(mu_all, sigma_all, z, W, u, R, idx_angle, a, keep_radian, loss, device)
    if cost_bar is not None and tuple(np.shape(cost_bar)) != (T,):
        raise ValueError("cost_bar must be ({},)".format(T))
    cb = B.as_dev(cost_bar, dev)
    outs = [B.empty((T, H, n_s), dev), B.empty((T, H, n_s, n_s), dev), B.empty((T, H, n_u), dev) if u is not None else None]
    check(lib.sr_rollout_cost_vjp(*head, float(w_stage), float(w_term), *tail, B.ptr(cb), *[B.ptr(o) for o in outs],
                                  B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _RolloutCostFn(torch.autograd.Function):
    """``rollout_cost_batch(differentiable=True)``: the forward is the plain call, the backward one ``rollout_cost_vjp_batch``."""

    @staticmethod
    def forward(ctx, cfg, mu_all, sigma_all, u):
        z, W, R, idx_angle, a, keep_radian, loss, w_stage, w_term, return_steps = cfg
        cost, steps = rollout_cost_batch(mu_all, sigma_all, z, W, u, R, idx_angle, a, keep_radian, loss, w_stage, w_term, True)
        ctx.cfg = cfg
        ctx.save_for_backward(mu_all, sigma_all, u)
        ctx.mark_non_differentiable(steps)
        ctx.set_materialize_grads(False)
        return cost, steps

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cost_bar, _steps_bar):
        mu_all, sigma_all, u = ctx.saved_tensors
        z, W, R, idx_angle, a, keep_radian, loss, w_stage, w_term, _ = ctx.cfg
        if cost_bar is None:
            return (None,) * 4
        g = rollout_cost_vjp_batch(mu_all, sigma_all, z, W, u, R, idx_angle, a, keep_radian, loss, w_stage, w_term, cost_bar)
        return None, g[0], (g[1] if sigma_all is not None else None), g[2]
