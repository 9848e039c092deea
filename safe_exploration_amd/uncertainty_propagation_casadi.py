"""Gaussian moment propagation through the GP dynamics (the CautiousMPC baseline), numeric and batched.

Numeric counterparts of the symbolic graph builders in
/root/reference/safe_exploration/uncertainty_propagation_casadi.py (one_step_taylor :11-87,
multi_step_taylor_symbolic :88-146, mean_equivalent_multistep :149-207, one_step_mean_equivalent
:210-283) with the same argument orders.  The covariance algebra of both schemes collapses to
``Sigma_new = H Sigma H^T + diag(var)`` with ``H = a + J_x + (b + J_u) K`` (Taylor) or ``H = a + b K``
(mean-equivalent); it runs in the same per-query kernel as the robust ellipsoid step.
The input transform ``a_gp_inp_x`` of the reference (the GP sees ``a_gp_inp_x @ state``, :40-47,60) is supported:
the state Jacobian is chain-ruled through the constant matrix.

Beyond the reference: EXACT moment matching (``MOMENT_MATCHING``; ``one_step_moment_matching``,
``multi_step_moment_matching``, ``moment_matching_batch``; ``moment_matching_rollout_batch``: the whole horizon in one launch;
``moment_matching_rollout_vjp_batch`` / ``moment_matching_rollout_diff_batch``: its reverse pass in one call, one autograd node),
the scheme the two above approximate.  The GP is evaluated at
the Gaussian input z = G x + g0, G = [a_gp_inp_x; K], g0 = [0; k_ff] (``SimpleGPModel.moment_match_device``: mean, full
covariance across outputs and expected Jacobian V in closed form), and with A = a + b K
``mu_new = A mu + b k_ff + mu_g``, ``Sigma_new = (A + V G) Sigma (A + V G)^T + Cov - (V G) Sigma (V G)^T``.
An initial covariance ``sigma_0`` is supported there.  Models whose kernels are all "rbf" or "lin_rbf" (a Matern kernel has no
closed form: NotImplementedError); ``differentiable=True`` needs an ARD-RBF model.

Beyond the reference as well: the reverse pass of ONE Taylor / mean-equivalent step on the device (``moment_step_vjp_batch`` /
``sr_moment_step_vjp``, ``onestep_moments_vjp_batch`` / ``sr_onestep_moments_vjp``), the one-step call from a Gaussian state with
the GP inside (``onestep_moments_batch`` / ``sr_onestep_moments``) and, on top of them, ``differentiable=True`` on
``moment_step_batch``, ``onestep_moments_batch`` and ``multistep_moments_batch``: the forward stays the plain call (the same
bits), the backward is the device reverse pass, steps are chained by torch autograd.  Gradients reach the means, covariances and
controls (and mu_g, var_g, jac_g of ``moment_step_batch``), not the model.  D <= 8.
The reverse pass of a WHOLE Taylor / mean-equivalent roll-out in one call: ``multistep_moments_vjp_batch`` /
``sr_multistep_moments_vjp`` (one pass of GP derivatives over all T*H steps, then a sweep, one thread per trajectory);
``multistep_moments_diff_batch`` is the autograd surface over it, one node for the roll-out, its forward the plain one-launch
``multistep_moments_batch`` (from sigma_0: H plain one-step calls).
"""
import numpy as np
import torch

from . import _buffers as B
from ._lib import lib, check
from .gp_reachability import _lin_model
from .ssm_hip.gaussian_process import SimpleGPModel

TAYLOR, MEAN_EQUIVALENT, MOMENT_MATCHING = 1, 2, 3


def multistep_moments_batch(mu_0, ssm, k_ff, k_fb, a=None, b=None, mode=TAYLOR, a_gp_inp_x=None, differentiable=False,
                            sigma_0=None):
    """T trajectories x H steps.  mu_0 (T,n_s); k_ff (T,H,n_u); k_fb (T,H-1,n_u,n_s); a_gp_inp_x (n_x_in,n_s) or None.
    Returns mu_all (T,H,n_s), sigma_all (T,H,n_s,n_s), gp_var_all (T,H,n_s).
    differentiable (tensors only): H differentiable ``onestep_moments_batch`` calls chained in torch and stacked, with an autograd
    graph from mu_0, sigma_0, k_ff and k_fb to the three results.  Every step is one ``sr_onestep_moments`` call: the
    launches of the plain call's per-step route (``ssm.set_chain(False)``), so the values are that route's to the bit.
    sigma_0 (T,n_s,n_s), with differentiable=True only: the roll-out starts from N(mu_0, sigma_0); step 0 has no feedback (a zero
    gain), as in ``moment_matching_batch``."""
    from .gp_reachability import _input_transform, _reach_dims
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("multistep_moments_batch needs the HIP SimpleGPModel")
    ssm._need_trained()
    if differentiable:
        if not B.is_tensor(mu_0):
            raise TypeError("differentiable=True needs tensors")
        if k_ff.dim() != 3:
            raise ValueError("k_ff must be (T, H, n_u)")
        H = k_ff.shape[1]
        mu, sigma, steps = mu_0, sigma_0, []
        for i in range(H):
            if i == 0:
                kfb_i = None if sigma_0 is None else sigma_0.new_zeros((mu_0.shape[0], k_ff.shape[2], mu_0.shape[1]))
            else:
                kfb_i = k_fb[:, i - 1]
            mu, sigma, var = onestep_moments_batch(mu, ssm, k_ff[:, i], sigma, kfb_i, a, b, mode, a_gp_inp_x, differentiable=True)
            steps.append((mu, sigma, var))
        return tuple(torch.stack([st[k] for st in steps], dim=1) for k in range(3))
    if sigma_0 is not None:
        raise NotImplementedError("sigma_0 needs differentiable=True (the per-step route; sr_multistep_moments starts from a point)")
    as_t = B.is_tensor(mu_0)
    hd = ssm._handle
    dev = hd.device
    n_s, n_u = _reach_dims(hd, a_gp_inp_x)
    m0 = B.as_dev(mu_0, dev)
    T = m0.shape[0]
    kff = B.as_dev(k_ff, dev)
    if kff.dim() != 3 or kff.shape[0] != T or kff.shape[2] != n_u:
        raise ValueError("k_ff must be (T, H, {})".format(n_u))
    H = kff.shape[1]
    kfb = B.as_dev(k_fb, dev, (T, H - 1, n_u, n_s)) if H > 1 else None
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    mu_all, sigma_all = B.empty((T, H, n_s), dev), B.empty((T, H, n_s, n_s), dev)
    var_all = B.empty((T, H, n_s), dev)
    with _input_transform(ssm, a_gp_inp_x):
        check(lib.sr_multistep_moments(hd.h, T, H, int(mode), B.ptr(m0), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb),
                                       B.ptr(mu_all), B.ptr(sigma_all), B.ptr(var_all), B.stream_ptr(dev)))
    outs = (mu_all, sigma_all, var_all)
    if as_t:
        return outs
    from .gp_reachability import _raise_if_chain_failed
    _raise_if_chain_failed(hd, dev, False)
    return tuple(B.to_numpy(o) for o in outs)


def moment_step_batch(mu_x, k_ff, mu_g, var_g, jac_g, sigma_x=None, k_fb=None, a=None, b=None, mode=TAYLOR,
                      device=None, differentiable=False):
    """One propagation step for T inputs with caller-supplied GP outputs (any StateSpaceModel).
    differentiable (tensors only): the outputs, the same bits, carry an autograd graph to mu_x, sigma_x, k_ff, k_fb, mu_g, var_g
    and jac_g whose backward is ``moment_step_vjp_batch`` (once differentiable)."""
    if differentiable:
        if not B.is_tensor(mu_x):
            raise TypeError("differentiable=True needs tensors")
        if sigma_x is not None and k_fb is None:
            raise ValueError("k_fb is required when sigma_x is given")
        gauss = sigma_x is not None
        return _MomentStepFn.apply((a, b, mode), mu_x, sigma_x, k_ff, k_fb if gauss else None, mu_g, var_g,
                                   jac_g if gauss else None)
    as_t = B.is_tensor(mu_x)
    dev = B.resolve_device(mu_x.device if as_t else device)
    mx = B.as_dev(mu_x, dev)
    T, n_s = mx.shape
    kff = B.as_dev(k_ff, dev).reshape(T, -1)
    n_u = kff.shape[1]
    sx = B.as_dev(sigma_x, dev, (T, n_s, n_s)) if sigma_x is not None else None
    if sx is not None and k_fb is None:
        raise ValueError("k_fb is required when sigma_x is given")
    kfb = B.as_dev(k_fb, dev, (T, n_u, n_s)) if sx is not None else None
    tmu, tvar = B.as_dev(mu_g, dev, (T, n_s)), B.as_dev(var_g, dev, (T, n_s))
    tjac = B.as_dev(jac_g, dev, (T, n_s, n_s + n_u)) if (jac_g is not None and sx is not None) else None
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    mo, so = B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev)
    check(lib.sr_moment_step(dev.index, T, n_s, n_u, int(mode), B.ptr(mx), B.ptr(sx), B.ptr(kff), B.ptr(kfb),
                             B.ptr(tmu), B.ptr(tvar), B.ptr(tjac), B.ptr(ta), B.ptr(tb), B.ptr(mo), B.ptr(so),
                             B.stream_ptr(dev)))
    return (mo, so) if as_t else (B.to_numpy(mo), B.to_numpy(so))


def _check_step(mu_x, k_ff, sigma_x, k_fb, mode, n_u=None):
    """argument checks of the one-step calls, before any device is touched: (T, n_s, n_u)"""
    if int(mode) not in (TAYLOR, MEAN_EQUIVALENT):
        raise ValueError("mode must be TAYLOR (1) or MEAN_EQUIVALENT (2), got {}".format(mode))
    shp = tuple(np.shape(mu_x))
    if len(shp) != 2:
        raise ValueError("mu_x must be (T, n_s)")
    T, n_s = shp
    kshp = tuple(np.shape(k_ff))
    if len(kshp) not in (1, 2) or kshp[0] != T or (n_u is not None and int(np.prod(kshp[1:])) != n_u):
        raise ValueError("k_ff must be (T, {})".format("n_u" if n_u is None else n_u))
    n_u = int(np.prod(kshp[1:]))
    if sigma_x is not None:
        if k_fb is None:
            raise ValueError("k_fb is required when sigma_x is given")
        if tuple(np.shape(sigma_x)) != (T, n_s, n_s) or tuple(np.shape(k_fb)) != (T, n_u, n_s):
            raise ValueError("sigma_x must be (T, {0}, {0}) and k_fb (T, {1}, {0})".format(n_s, n_u))
    return T, n_s, n_u


def _check_seeds(seeds, shapes):
    if all(s is None for s in seeds):
        raise ValueError("at least one seed is needed")
    for s, shape in zip(seeds, shapes):
        if s is not None and tuple(np.shape(s)) != shape:
            raise ValueError("a seed must be shaped like its output, {}".format(shape))


def moment_step_vjp_batch(mu_x, k_ff, mu_g, var_g, jac_g, mu1_bar=None, sigma1_bar=None, sigma_x=None, k_fb=None, a=None,
                          b=None, mode=TAYLOR, device=None):
    """Reverse pass of ``moment_step_batch`` (``sr_moment_step_vjp``): for seeds mu1_bar (T,n_s), sigma1_bar (T,n_s,n_s) on its two
    outputs (None = zero) the gradients (mux_bar, sigma_bar, kff_bar, kfb_bar, mug_bar, var_bar, jac_bar), shaped like the inputs;
    sigma_bar, kfb_bar and jac_bar are None at a point start (sigma_x None); jac_bar is zero in the mean-equivalent mode.  Only
    the symmetric part of sigma1_bar counts, sigma_bar is exactly symmetric.  numpy in -> numpy out, tensors in -> tensors out."""
    T, n_s, n_u = _check_step(mu_x, k_ff, sigma_x, k_fb, mode)
    gauss = sigma_x is not None
    if gauss and int(mode) == TAYLOR and jac_g is None:
        raise ValueError("jac_g is required when sigma_x is given (Taylor mode)")
    if tuple(np.shape(mu_g)) != (T, n_s) or tuple(np.shape(var_g)) != (T, n_s):
        raise ValueError("mu_g and var_g must be (T, {})".format(n_s))
    if gauss and jac_g is not None and tuple(np.shape(jac_g)) != (T, n_s, n_s + n_u):
        raise ValueError("jac_g must be (T, {}, {})".format(n_s, n_s + n_u))
    _check_seeds((mu1_bar, sigma1_bar), ((T, n_s), (T, n_s, n_s)))
    as_t = B.is_tensor(mu_x)
    dev = B.resolve_device(mu_x.device if as_t else device)
    mx, kff = B.as_dev(mu_x, dev), B.as_dev(k_ff, dev, (T, n_u))
    sx = B.as_dev(sigma_x, dev) if gauss else None
    kfb = B.as_dev(k_fb, dev) if gauss else None
    tmu, tvar = B.as_dev(mu_g, dev), B.as_dev(var_g, dev)
    tjac = B.as_dev(jac_g, dev) if (gauss and jac_g is not None) else None
    mb, sb = B.as_dev(mu1_bar, dev), B.as_dev(sigma1_bar, dev)
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if gauss else None, B.empty((T, n_u), dev),
            B.empty((T, n_u, n_s), dev) if gauss else None, B.empty((T, n_s), dev), B.empty((T, n_s), dev),
            B.empty((T, n_s, n_s + n_u), dev) if gauss else None]
    check(lib.sr_moment_step_vjp(dev.index, T, n_s, n_u, int(mode), B.ptr(mx), B.ptr(sx), B.ptr(kff), B.ptr(kfb), B.ptr(tmu),
                                 B.ptr(tvar), B.ptr(tjac), B.ptr(ta), B.ptr(tb), B.ptr(mb), B.ptr(sb), *[B.ptr(o) for o in outs],
                                 B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


def _onestep_setup(name, mu_x, ssm, k_ff, sigma_x, k_fb, a, b, mode, a_gp_inp_x):
    from .gp_reachability import _reach_dims
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError(name + " needs the HIP SimpleGPModel")
    ssm._need_trained()
    hd = ssm._handle
    n_s, n_u = _reach_dims(hd, a_gp_inp_x)
    T, ns_in, _ = _check_step(mu_x, k_ff, sigma_x, k_fb, mode, n_u)
    if ns_in != n_s:
        raise ValueError("mu_x must be (T, {})".format(n_s))
    dev = hd.device
    gauss = sigma_x is not None
    a, b = _lin_model(a, b, n_s, n_u)
    return (hd, dev, T, n_s, n_u, B.as_dev(mu_x, dev), B.as_dev(sigma_x, dev) if gauss else None, B.as_dev(k_ff, dev, (T, n_u)),
            B.as_dev(k_fb, dev) if gauss else None, B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u)))


def onestep_moments_batch(mu_x, ssm, k_ff, sigma_x=None, k_fb=None, a=None, b=None, mode=TAYLOR, a_gp_inp_x=None,
                          differentiable=False):
    """One Taylor / mean-equivalent step for T states with the GP inside (``sr_onestep_moments``), from points (sigma_x None) or
    from N(mu_x, sigma_x).  mu_x (T,n_s); k_ff (T,n_u); sigma_x (T,n_s,n_s); k_fb (T,n_u,n_s), required with sigma_x.
    Returns mu_new (T,n_s), sigma_new (T,n_s,n_s), gp variances (T,n_s).  numpy in -> numpy out, tensors in -> tensors out.
    differentiable (tensors only): the three outputs, the same bits, carry an autograd graph to mu_x, sigma_x, k_ff and k_fb whose
    backward is ``onestep_moments_vjp_batch`` (once differentiable; no gradient to the model)."""
    from .gp_reachability import _input_transform
    if differentiable:
        if not isinstance(ssm, SimpleGPModel):
            raise TypeError("onestep_moments_batch needs the HIP SimpleGPModel")
        if not B.is_tensor(mu_x):
            raise TypeError("differentiable=True needs tensors")
        if sigma_x is not None and k_fb is None:
            raise ValueError("k_fb is required when sigma_x is given")
        return _OnestepMomentsFn.apply(ssm, (a, b, mode, a_gp_inp_x), mu_x, sigma_x, k_ff, k_fb if sigma_x is not None else None)
    as_t = B.is_tensor(mu_x)
    hd, dev, T, n_s, n_u, mx, sx, kff, kfb, ta, tb = _onestep_setup("onestep_moments_batch", mu_x, ssm, k_ff, sigma_x, k_fb, a, b,
                                                                    mode, a_gp_inp_x)
    outs = (B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev), B.empty((T, n_s), dev))
    with _input_transform(ssm, a_gp_inp_x):
        check(lib.sr_onestep_moments(hd.h, T, int(mode), B.ptr(mx), B.ptr(sx), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb),
                                     *[B.ptr(o) for o in outs], B.stream_ptr(dev)))
    return outs if as_t else tuple(B.to_numpy(o) for o in outs)


def onestep_moments_vjp_batch(mu_x, ssm, k_ff, mu1_bar=None, sigma1_bar=None, gpvar_bar=None, sigma_x=None, k_fb=None, a=None,
                              b=None, mode=TAYLOR, a_gp_inp_x=None):
    """Reverse pass of ``onestep_moments_batch``, GP included (``sr_onestep_moments_vjp``: the GP derivatives at
    z = [a_gp_inp_x mu_x; k_ff], then one launch with the reverse of the moment algebra and the GP link): for seeds mu1_bar (T,n_s),
    sigma1_bar (T,n_s,n_s), gpvar_bar (T,n_s) on the three outputs (None = zero) the gradients (mux_bar, sigma_bar, kff_bar,
    kfb_bar); sigma_bar and kfb_bar are None at a point start.  Models as ``linearize_device_batch`` takes them (every kernel, exact
    and sparse, D <= 8: NotImplementedError beyond).  numpy in -> numpy out, tensors in -> tensors out."""
    from .gp_reachability import _input_transform
    as_t = B.is_tensor(mu_x)
    hd, dev, T, n_s, n_u, mx, sx, kff, kfb, ta, tb = _onestep_setup("onestep_moments_vjp_batch", mu_x, ssm, k_ff, sigma_x, k_fb, a,
                                                                    b, mode, a_gp_inp_x)
    _check_seeds((mu1_bar, sigma1_bar, gpvar_bar), ((T, n_s), (T, n_s, n_s), (T, n_s)))
    seeds = [B.as_dev(x, dev) for x in (mu1_bar, sigma1_bar, gpvar_bar)]
    gauss = sx is not None
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if gauss else None, B.empty((T, n_u), dev),
            B.empty((T, n_u, n_s), dev) if gauss else None]
    with _input_transform(ssm, a_gp_inp_x):
        check(lib.sr_onestep_moments_vjp(hd.h, T, int(mode), B.ptr(mx), B.ptr(sx), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb),
                                         *[B.ptr(x) for x in seeds], *[B.ptr(o) for o in outs], B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _MomentStepFn(torch.autograd.Function):
    """``moment_step_batch(..., differentiable=True)``: the forward is the plain call, the backward ``moment_step_vjp_batch`` at
    the saved inputs.  Seeds of outputs nobody used arrive as None (= zero, the same bits)."""

    @staticmethod
    def forward(ctx, cfg, mu_x, sigma_x, k_ff, k_fb, mu_g, var_g, jac_g):
        a, b, mode = cfg
        mu1, sigma1 = moment_step_batch(mu_x, k_ff, mu_g, var_g, jac_g, sigma_x, k_fb, a, b, mode)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mu_x, sigma_x, k_ff, k_fb, mu_g, var_g, jac_g)
        return mu1, sigma1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mu1_bar, sigma1_bar):
        mu_x, sigma_x, k_ff, k_fb, mu_g, var_g, jac_g = ctx.saved_tensors
        a, b, mode = ctx.cfg
        if mu1_bar is None and sigma1_bar is None:
            return (None,) * 8
        g = moment_step_vjp_batch(mu_x, k_ff, mu_g, var_g, jac_g, mu1_bar, sigma1_bar, sigma_x, k_fb, a, b, mode)
        return (None, g[0], g[1], g[2].reshape(k_ff.shape), g[3], g[4], g[5], g[6] if jac_g is not None else None)


class _OnestepMomentsFn(torch.autograd.Function):
    """``onestep_moments_batch(..., differentiable=True)``, likewise over ``onestep_moments_vjp_batch``; the GP variances carry a
    gradient too (the seed gpvar_bar)."""

    @staticmethod
    def forward(ctx, ssm, cfg, mu_x, sigma_x, k_ff, k_fb):
        a, b, mode, a_gp_inp_x = cfg
        outs = onestep_moments_batch(mu_x, ssm, k_ff, sigma_x, k_fb, a, b, mode, a_gp_inp_x)
        ctx.ssm, ctx.cfg = ssm, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mu_x, sigma_x, k_ff, k_fb)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mu1_bar, sigma1_bar, gpvar_bar):
        mu_x, sigma_x, k_ff, k_fb = ctx.saved_tensors
        a, b, mode, a_gp_inp_x = ctx.cfg
        if mu1_bar is None and sigma1_bar is None and gpvar_bar is None:
            return (None,) * 6
        g = onestep_moments_vjp_batch(mu_x, ctx.ssm, k_ff, mu1_bar, sigma1_bar, gpvar_bar, sigma_x, k_fb, a, b, mode, a_gp_inp_x)
        return None, None, g[0], g[1], g[2].reshape(k_ff.shape), g[3]


def multistep_moments_vjp_batch(mu_0, ssm, k_ff, k_fb, mu_all, sigma_all, mu_all_bar=None, sigma_all_bar=None, gpvar_all_bar=None,
                                a=None, b=None, mode=TAYLOR, a_gp_inp_x=None, sigma_0=None):
    """Reverse pass of a whole Taylor / mean-equivalent roll-out in one call (``sr_multistep_moments_vjp``): one pass of GP
    derivatives at the inputs of all T*H steps -- the means mu_all are known --, then a sweep over the steps, one thread per
    trajectory.

    The forward arguments as ``multistep_moments_batch`` takes them (k_fb may be None when H == 1); sigma_0 (T,n_s,n_s): the
    roll-out started from N(mu_0, sigma_0), step 0 with a zero gain, as ``multistep_moments_batch(sigma_0=..., differentiable=True)``
    runs it.  mu_all (T,H,n_s), sigma_all (T,H,n_s,n_s) are what the forward returned; seeds mu_all_bar, sigma_all_bar,
    gpvar_all_bar (T,H,n_s) shaped like its three results (None = zero, not all three).  Returns the gradients of
    sum(mu_all_bar * mu_all) + sum(sigma_all_bar * sigma_all) + sum(gpvar_all_bar * gp_var_all): (mu0_bar, sigma0_bar, kff_bar,
    kfb_bar), shaped like mu_0, sigma_0, k_ff and k_fb ((T,H-1,n_u,n_s)); sigma0_bar is None without sigma_0.  Only the symmetric
    part of sigma_all_bar counts, sigma0_bar is exactly symmetric.  The same bits on every call and for any ``set_chunk``.
    Models as ``linearize_device_batch`` takes them (D <= 8: NotImplementedError beyond).  numpy in -> numpy out, tensors in ->
    tensors out."""
    from .gp_reachability import _input_transform, _reach_dims
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("multistep_moments_vjp_batch needs the HIP SimpleGPModel")
    ssm._need_trained()
    if int(mode) not in (TAYLOR, MEAN_EQUIVALENT):
        raise ValueError("mode must be TAYLOR (1) or MEAN_EQUIVALENT (2), got {}".format(mode))
    as_t = B.is_tensor(mu_0)
    hd = ssm._handle
    dev = hd.device
    n_s, n_u = _reach_dims(hd, a_gp_inp_x)
    shp, kshp = tuple(np.shape(mu_0)), tuple(np.shape(k_ff))
    if len(shp) != 2 or shp[1] != n_s:
        raise ValueError("mu_0 must be (T, {})".format(n_s))
    T = shp[0]
    if len(kshp) != 3 or kshp[0] != T or kshp[2] != n_u or kshp[1] < 1:
        raise ValueError("k_ff must be (T, H, {}) with H >= 1".format(n_u))
    H = kshp[1]
    if H > 1 and (k_fb is None or tuple(np.shape(k_fb)) != (T, H - 1, n_u, n_s)):
        raise ValueError("k_fb must be {}".format((T, H - 1, n_u, n_s)))
    for x, shape, name in ((sigma_0, (T, n_s, n_s), "sigma_0"), (mu_all, (T, H, n_s), "mu_all"),
                           (sigma_all, (T, H, n_s, n_s), "sigma_all")):
        if (x is None and name != "sigma_0") or (x is not None and tuple(np.shape(x)) != shape):
            raise ValueError("{} must be {}".format(name, shape))
    _check_seeds((mu_all_bar, sigma_all_bar, gpvar_all_bar), ((T, H, n_s), (T, H, n_s, n_s), (T, H, n_s)))
    m0, kff = B.as_dev(mu_0, dev), B.as_dev(k_ff, dev)
    kfb = B.as_dev(k_fb, dev) if H > 1 else None
    s0, ma, sa = B.as_dev(sigma_0, dev), B.as_dev(mu_all, dev), B.as_dev(sigma_all, dev)
    seeds = [B.as_dev(x, dev) for x in (mu_all_bar, sigma_all_bar, gpvar_all_bar)]
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if s0 is not None else None, B.empty((T, H, n_u), dev),
            B.empty((T, H - 1, n_u, n_s), dev)]
    with _input_transform(ssm, a_gp_inp_x):
        check(lib.sr_multistep_moments_vjp(hd.h, T, H, int(mode), B.ptr(m0), B.ptr(s0), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb),
                                           B.ptr(ma), B.ptr(sa), *[B.ptr(x) for x in seeds],
                                           *[B.ptr(o) if o is not None and o.numel() else None for o in outs], B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _MultistepMomentsFn(torch.autograd.Function):
    """``multistep_moments_diff_batch``: the forward is the plain one-launch ``multistep_moments_batch`` from a point, H plain
    ``onestep_moments_batch`` calls from N(mu_0, sigma_0); the backward ONE ``multistep_moments_vjp_batch`` call at the saved
    mu_all, sigma_all.  Seeds of results nobody used arrive as None (= zero, the same bits)."""

    @staticmethod
    def forward(ctx, ssm, cfg, mu_0, sigma_0, k_ff, k_fb):
        a, b, mode, a_gp_inp_x = cfg
        if sigma_0 is None:
            outs = multistep_moments_batch(mu_0, ssm, k_ff, k_fb, a, b, mode, a_gp_inp_x)
        else:
            mu, sigma, steps = mu_0, sigma_0, []
            for i in range(k_ff.shape[1]):
                kfb_i = sigma_0.new_zeros((mu_0.shape[0], k_ff.shape[2], mu_0.shape[1])) if i == 0 else k_fb[:, i - 1]
                mu, sigma, var = onestep_moments_batch(mu, ssm, k_ff[:, i], sigma, kfb_i, a, b, mode, a_gp_inp_x)
                steps.append((mu, sigma, var))
            outs = tuple(torch.stack([st[k] for st in steps], dim=1) for k in range(3))
        ctx.ssm, ctx.cfg = ssm, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mu_0, sigma_0, k_ff, k_fb, outs[0], outs[1])
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mu_all_bar, sigma_all_bar, gpvar_all_bar):
        mu_0, sigma_0, k_ff, k_fb, mu_all, sigma_all = ctx.saved_tensors
        a, b, mode, a_gp_inp_x = ctx.cfg
        if mu_all_bar is None and sigma_all_bar is None and gpvar_all_bar is None:
            return (None,) * 6
        g = multistep_moments_vjp_batch(mu_0, ctx.ssm, k_ff, k_fb, mu_all, sigma_all, mu_all_bar, sigma_all_bar, gpvar_all_bar,
                                        a, b, mode, a_gp_inp_x, sigma_0)
        return None, None, g[0], g[1], g[2], (g[3].reshape(k_fb.shape) if k_fb is not None else None)


def multistep_moments_diff_batch(mu_0, ssm, k_ff, k_fb, a=None, b=None, mode=TAYLOR, a_gp_inp_x=None, sigma_0=None):
    """``multistep_moments_batch`` (tensors only) as ONE autograd node for the whole roll-out, with gradients to mu_0, sigma_0, k_ff
    and k_fb.  From a point the forward IS the plain one-launch call (the same bits); from sigma_0 (T,n_s,n_s) it is H plain
    ``sr_onestep_moments`` calls, step 0 with a zero gain: the bits of ``multistep_moments_batch(sigma_0=..., differentiable=True)``.
    The backward is ONE ``multistep_moments_vjp_batch`` call at the saved mu_all, sigma_all (once differentiable; no gradient to
    a, b or the model).  ``multistep_moments_batch(differentiable=True)`` chains H one-step nodes instead and stays as it is."""
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("multistep_moments_diff_batch needs the HIP SimpleGPModel")
    ssm._need_trained()
    if not B.is_tensor(mu_0):
        raise TypeError("multistep_moments_diff_batch needs tensors")
    if k_ff.dim() != 3:
        raise ValueError("k_ff must be (T, H, n_u)")
    if k_ff.shape[1] > 1 and k_fb is None:
        raise ValueError("k_fb is required for H > 1")
    return _MultistepMomentsFn.apply(ssm, (a, b, mode, a_gp_inp_x), mu_0, sigma_0, k_ff, k_fb if k_ff.shape[1] > 1 else None)


def _one_step(mu_x, ssm, k_ff, sigma_x, k_fb, a, b, a_gp_inp_x, mode):
    mu_x = np.asarray(mu_x, dtype=np.float64)
    k_ff = np.asarray(k_ff, dtype=np.float64)
    n_s = mu_x.shape[0]
    t = None if a_gp_inp_x is None else np.asarray(a_gp_inp_x, dtype=np.float64)
    x_bar = mu_x if t is None else t.dot(mu_x)
    out = ssm(x_bar.T, k_ff.T)                         # (mu n x 1, var n x 1, jac n x D)
    mu_g, var_g = np.asarray(out[0], dtype=np.float64), np.asarray(out[1], dtype=np.float64)
    jac = np.asarray(out[2], dtype=np.float64) if sigma_x is not None else None
    if jac is not None and t is not None:              # chain rule through the constant input map (:60)
        jac = np.hstack((jac[:, :t.shape[0]].dot(t), jac[:, t.shape[0]:]))
    jac = jac[None] if jac is not None else None
    sx = None if sigma_x is None else np.asarray(sigma_x, dtype=np.float64)[None]
    kfb = None if sigma_x is None else np.asarray(k_fb, dtype=np.float64)[None]
    mu_new, sigma_new = moment_step_batch(mu_x.T, k_ff.T, mu_g.reshape(1, n_s), var_g.reshape(1, n_s), jac, sx,
                                          kfb, a, b, mode)
    return mu_new.reshape(n_s, 1), sigma_new[0], var_g.reshape(1, n_s)


def one_step_taylor(mu_x, ssm, k_ff, sigma_x=None, k_fb=None, a=None, b=None, a_gp_inp_x=None):
    """First-order Taylor propagation of N(mu_x, sigma_x) (uncertainty_propagation_casadi.py:11-87).
    Returns mu_new (n_s,1), sigma_new (n_s,n_s), gp variances (1,n_s)."""
    return _one_step(mu_x, ssm, k_ff, sigma_x, k_fb, a, b, a_gp_inp_x, TAYLOR)


def one_step_mean_equivalent(mu_x, ssm, k_ff, sigma_x=None, k_fb=None, a=None, b=None, a_gp_inp_x=None):
    """'Mean-equivalent' propagation: no Jacobian cross terms (uncertainty_propagation_casadi.py:210-283)."""
    return _one_step(mu_x, ssm, k_ff, sigma_x, k_fb, a, b, a_gp_inp_x, MEAN_EQUIVALENT)


def _multi(mu_0, ssm, k_ff, k_fb, sigma_0, a, b, a_gp_inp_x, mode):
    if sigma_0 is not None:
        raise NotImplementedError("Still need  to do this")        # like the reference (:124, :170)
    k_ff = np.asarray(k_ff, dtype=np.float64)
    T, n_u = k_ff.shape
    n_s = np.shape(mu_0)[0]
    kfb = np.asarray(k_fb, dtype=np.float64).reshape(T - 1, n_u, n_s)[None] if T > 1 else None
    if isinstance(ssm, SimpleGPModel):
        mu_all, sigma_all, var_all = multistep_moments_batch(np.asarray(mu_0, dtype=np.float64).reshape(1, n_s),
                                                             ssm, k_ff[None], kfb, a, b, mode, a_gp_inp_x)
        return mu_all[0], sigma_all[0].reshape(T, n_s * n_s), var_all[0]
    one = one_step_taylor if mode == TAYLOR else one_step_mean_equivalent
    mu_new, sigma_new, gv = one(mu_0, ssm, k_ff[0].reshape(n_u, 1), None, None, a, b, a_gp_inp_x)
    mus, sigmas, gvs = [mu_new.T], [sigma_new.reshape(1, -1)], [gv]
    for i in range(T - 1):
        mu_new, sigma_new, gv = one(mu_new, ssm, k_ff[i + 1].reshape(n_u, 1), sigma_new, kfb[0, i], a, b, a_gp_inp_x)
        mus.append(mu_new.T), sigmas.append(sigma_new.reshape(1, -1)), gvs.append(gv)
    return np.vstack(mus), np.vstack(sigmas), np.vstack(gvs)


def multi_step_taylor(mu_0, ssm, k_ff, k_fb, sigma_0=None, a=None, b=None, a_gp_inp_x=None):
    """Numeric ``multi_step_taylor_symbolic`` (uncertainty_propagation_casadi.py:88-146): k_ff (T,n_u),
    k_fb list/array of T-1 (n_u,n_s) gains.  Returns mu_all (T,n_s), sigma_all (T,n_s*n_s), gp variances (T,n_s)."""
    return _multi(mu_0, ssm, k_ff, k_fb, sigma_0, a, b, a_gp_inp_x, TAYLOR)


def mean_equivalent_multistep(mu_0, ssm, k_ff, k_fb, sigma_0=None, a=None, b=None, a_gp_inp_x=None):
    """uncertainty_propagation_casadi.py:149-207."""
    return _multi(mu_0, ssm, k_ff, k_fb, sigma_0, a, b, a_gp_inp_x, MEAN_EQUIVALENT)


multi_step_taylor_symbolic = multi_step_taylor      # the reference's name (uncertainty_propagation_casadi.py:11)


# ---------------------------------------------------------------------------------------------- exact moment matching
def _mm_step(ssm, mu, sigma, kff, K, ta, tb, tz, differentiable=False):
    """One exact step on device tensors: mu (T,n_s), sigma (T,n_s,n_s) or None, kff (T,n_u), K (T,n_u,n_s) or None (= 0),
    tz (n_x_in,n_s).  The control is u = K x + k_ff.  Returns mu_new, sigma_new, Cov of the GP outputs.
    differentiable: the GP call keeps the autograd graph (``moment_match_device(differentiable=True)``)."""
    T, n_s = mu.shape
    zx = mu.matmul(tz.t())
    if K is None:
        A = ta.expand(T, n_s, n_s)
        zu = kff
        G = torch.cat((tz.expand(T, -1, -1), kff.new_zeros((T, kff.shape[1], n_s))), dim=1)
    else:
        A = ta + tb.matmul(K)
        zu = kff + K.matmul(mu.unsqueeze(2)).squeeze(2)
        G = torch.cat((tz.expand(T, -1, -1), K), dim=1)
    S = None if sigma is None else G.matmul(sigma).matmul(G.transpose(1, 2))
    mu_g, cov, V = ssm.moment_match_device(torch.cat((zx, zu), dim=1), S, differentiable=differentiable)
    mu_new = A.matmul(mu.unsqueeze(2)).squeeze(2) + kff.matmul(tb.t()) + mu_g
    if sigma is None:
        return mu_new, cov, cov
    VG = V.matmul(G)
    Hm = A + VG
    sigma_new = Hm.matmul(sigma).matmul(Hm.transpose(1, 2)) + cov - VG.matmul(sigma).matmul(VG.transpose(1, 2))
    return mu_new, sigma_new, cov


def _mm_setup(ssm, a, b, a_gp_inp_x):
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("moment matching needs the HIP SimpleGPModel")
    ssm._need_trained()
    hd = ssm._handle
    n_s = hd.n_out
    tzn = np.eye(n_s) if a_gp_inp_x is None else np.asarray(a_gp_inp_x, dtype=np.float64)
    if tzn.ndim != 2 or tzn.shape[1] != n_s or tzn.shape[0] > hd.D:
        raise ValueError("a_gp_inp_x must be (n_x_in, {}) with n_x_in <= {}".format(n_s, hd.D))
    n_u = hd.D - tzn.shape[0]
    a, b = _lin_model(a, b, n_s, n_u)
    dev = hd.device
    return dev, n_s, n_u, B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u)), B.const_dev(tzn, dev, tzn.shape)


def moment_matching_batch(mu_0, ssm, k_ff, k_fb, a=None, b=None, sigma_0=None, a_gp_inp_x=None, differentiable=False):
    """Exact moment matching for T trajectories x H steps.  mu_0 (T,n_s); k_ff (T,H,n_u); k_fb (T,H-1,n_u,n_s) (step 0 has
    no feedback, step i >= 1 uses k_fb[:, i-1]); sigma_0 (T,n_s,n_s) or None (a point).
    Returns mu_all (T,H,n_s), sigma_all (T,H,n_s,n_s), gp_cov_all (T,H,n_s,n_s) (the GP's full output covariance).
    H calls of ``sr_gp_moment_match`` with the small algebra in batched torch ops; nothing synchronises between steps.
    Device tensors in -> device tensors out.
    differentiable=True: the autograd graph is kept from mu_0, sigma_0, k_ff and k_fb (device tensors that require grad) to the
    three results: every GP call hangs on ``sr_gp_moment_match_vjp`` and the steps are stacked, not written into a buffer.
    The values are those of the plain call."""
    dev, n_s, n_u, ta, tb, tz = _mm_setup(ssm, a, b, a_gp_inp_x)
    as_t = B.is_tensor(mu_0)
    mu = B.as_dev(mu_0, dev)
    T = mu.shape[0]
    kff = B.as_dev(k_ff, dev)
    if mu.dim() != 2 or mu.shape[1] != n_s or kff.dim() != 3 or kff.shape[0] != T or kff.shape[2] != n_u:
        raise ValueError("mu_0 must be (T, {}) and k_ff (T, H, {})".format(n_s, n_u))
    H = kff.shape[1]
    kfb = B.as_dev(k_fb, dev, (T, H - 1, n_u, n_s)) if H > 1 else None
    sigma = B.as_dev(sigma_0, dev, (T, n_s, n_s)) if sigma_0 is not None else None
    if differentiable:
        steps = []
        for i in range(H):
            mu, sigma, cov = _mm_step(ssm, mu, sigma, kff[:, i], None if i == 0 else kfb[:, i - 1], ta, tb, tz, True)
            steps.append((mu, sigma, cov))
        outs = tuple(torch.stack([st[k] for st in steps], dim=1) for k in range(3))
        return outs if as_t else tuple(B.to_numpy(o.detach()) for o in outs)
    mu_all, sigma_all = B.empty((T, H, n_s), dev), B.empty((T, H, n_s, n_s), dev)
    cov_all = B.empty((T, H, n_s, n_s), dev)
    for i in range(H):
        mu, sigma, cov = _mm_step(ssm, mu, sigma, kff[:, i], None if i == 0 else kfb[:, i - 1], ta, tb, tz)
        mu_all[:, i], sigma_all[:, i], cov_all[:, i] = mu, sigma, cov
    outs = (mu_all, sigma_all, cov_all)
    return outs if as_t else tuple(B.to_numpy(o) for o in outs)


def moment_matching_rollout_batch(mu_0, ssm, k_ff, k_fb, a=None, b=None, sigma_0=None, a_gp_inp_x=None):
    """``moment_matching_batch`` with all H steps of every trajectory in ONE launch (``sr_gp_moment_match_rollout``,
    ``SimpleGPModel.moment_match_rollout_device``): the same arguments (mu_0 (T,n_s); k_ff (T,H,n_u); k_fb (T,H-1,n_u,n_s);
    sigma_0 (T,n_s,n_s) or None) and the same three results, mu_all (T,H,n_s), sigma_all (T,H,n_s,n_s), gp_cov_all
    (T,H,n_s,n_s), equal to those of ``moment_matching_batch`` to rounding (the double sum is added in another order).
    NumPy in -> NumPy out; device tensors in -> device tensors out.
    Inside the fused kernel's domain -- ARD-RBF models, exact or sparse, with N <= 1024 and D <= 12 -- it calls the fused
    kernel; outside of it (a ``lin_rbf`` model, a larger model) it calls ``moment_matching_batch`` and returns what that
    returns."""
    dev, n_s, n_u, ta, tb, tz = _mm_setup(ssm, a, b, a_gp_inp_x)
    if not ssm.moment_match_rollout_supported():
        return moment_matching_batch(mu_0, ssm, k_ff, k_fb, a, b, sigma_0, a_gp_inp_x)
    as_t = B.is_tensor(mu_0)
    mu = B.as_dev(mu_0, dev)
    T = mu.shape[0]
    kff = B.as_dev(k_ff, dev)
    if mu.dim() != 2 or mu.shape[1] != n_s or kff.dim() != 3 or kff.shape[0] != T or kff.shape[2] != n_u:
        raise ValueError("mu_0 must be (T, {}) and k_ff (T, H, {})".format(n_s, n_u))
    H = kff.shape[1]
    kfb = B.as_dev(k_fb, dev, (T, H - 1, n_u, n_s)) if H > 1 else None
    outs = ssm.moment_match_rollout_device(mu, kff, kfb, ta, tb, sigma_0, None if a_gp_inp_x is None else tz)
    return outs if as_t else tuple(B.to_numpy(o) for o in outs)


def moment_matching_rollout_vjp_batch(mu_0, ssm, k_ff, k_fb, mu_all, sigma_all, mu_all_bar=None, sigma_all_bar=None,
                                      cov_all_bar=None, a=None, b=None, sigma_0=None, a_gp_inp_x=None):
    """The reverse pass of ``moment_matching_batch`` / ``moment_matching_rollout_batch`` in ONE call
    (``sr_gp_moment_match_rollout_vjp``, ``SimpleGPModel.moment_match_rollout_vjp_device``): the gradient of
    sum(mu_all_bar * mu_all) + sum(sigma_all_bar * sigma_all) + sum(cov_all_bar * gp_cov_all) in mu_0, sigma_0, k_ff and k_fb at
    the mu_all, sigma_all either forward returned.  Seeds shaped like the forward's results, None = zero (not all three).
    Returns (mu_0_bar, sigma_0_bar | None without sigma_0, k_ff_bar, k_fb_bar | None when H == 1), the gain gradients shaped
    like k_ff / k_fb (summed over T for a shared, 2-D policy).  NumPy in -> NumPy out; device tensors in -> device tensors
    out.  ARD-RBF models of any size (NotImplementedError otherwise)."""
    dev, n_s, n_u, ta, tb, tz = _mm_setup(ssm, a, b, a_gp_inp_x)
    as_t = B.is_tensor(mu_0)
    outs = ssm.moment_match_rollout_vjp_device(mu_0, k_ff, k_fb, ta, tb, mu_all, sigma_all, mu_all_bar, sigma_all_bar,
                                               cov_all_bar, sigma_0, None if a_gp_inp_x is None else tz)
    return outs if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _MomentMatchRolloutFn(torch.autograd.Function):
    """``moment_matching_rollout_diff_batch``: the forward is ``moment_matching_rollout_batch``, the backward ONE call of
    ``moment_match_rollout_vjp_device`` at the saved results.  Seeds of results nobody used arrive as None (= zero)."""

    @staticmethod
    def forward(ctx, ssm, a, b, a_gp_inp_x, mu_0, sigma_0, k_ff, k_fb):
        outs = moment_matching_rollout_batch(mu_0.detach(), ssm, k_ff.detach(), None if k_fb is None else k_fb.detach(), a, b,
                                             None if sigma_0 is None else sigma_0.detach(), a_gp_inp_x)
        ctx.ssm, ctx.lin = ssm, (a, b, a_gp_inp_x)
        ctx.opt = (sigma_0 is not None, k_fb is not None)
        ctx.save_for_backward(mu_0, k_ff, outs[0], outs[1], *[x for x in (sigma_0, k_fb) if x is not None])
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mu_all_bar, sigma_all_bar, cov_all_bar):
        mu_0, k_ff, mu_all, sigma_all, *rest = ctx.saved_tensors
        rest = list(rest)
        sigma_0 = rest.pop(0) if ctx.opt[0] else None
        k_fb = rest.pop(0) if ctx.opt[1] else None
        a, b, a_gp_inp_x = ctx.lin
        if mu_all_bar is None and sigma_all_bar is None and cov_all_bar is None:
            return (None,) * 8
        dev, n_s, n_u, ta, tb, tz = _mm_setup(ctx.ssm, a, b, a_gp_inp_x)
        g = ctx.ssm.moment_match_rollout_vjp_device(mu_0, k_ff, k_fb, ta, tb, mu_all, sigma_all, mu_all_bar, sigma_all_bar,
                                                    cov_all_bar, sigma_0, None if a_gp_inp_x is None else tz)
        return None, None, None, None, g[0], g[1], g[2], g[3]


def moment_matching_rollout_diff_batch(mu_0, ssm, k_ff, k_fb, a=None, b=None, sigma_0=None, a_gp_inp_x=None):
    """``moment_matching_rollout_batch`` as ONE ``torch.autograd.Function`` for the whole roll-out: the same arguments
    (mu_0 (T,n_s); k_ff (T,H,n_u); k_fb (T,H-1,n_u,n_s) or None when H == 1; sigma_0 (T,n_s,n_s) or None), the same three
    results with the same bits -- the fused kernel inside its domain, the per-step route outside --, and a backward that is
    one call of ``sr_gp_moment_match_rollout_vjp`` (once differentiable; gradients to mu_0, sigma_0, k_ff and k_fb, not to a, b
    or the model).  ARD-RBF models only (NotImplementedError otherwise, before any launch).  Device tensors come back as
    device tensors that carry the graph; NumPy inputs give NumPy results (the plain forward: nothing to differentiate)."""
    dev, n_s, n_u, ta, tb, tz = _mm_setup(ssm, a, b, a_gp_inp_x)
    if any(kt != "rbf" for kt in ssm.kern_types):
        raise NotImplementedError("moment matching: the reverse pass is for ARD-RBF models only")
    as_t = B.is_tensor(mu_0)
    leaves = [None if x is None else B.as_dev(x, dev) for x in (mu_0, sigma_0, k_ff, k_fb)]
    outs = _MomentMatchRolloutFn.apply(ssm, a, b, a_gp_inp_x, *leaves)
    return outs if as_t else tuple(B.to_numpy(o.detach()) for o in outs)


def one_step_moment_matching(mu_x, ssm, k_ff, sigma_x=None, k_fb=None, a=None, b=None, a_gp_inp_x=None):
    """Exact moment matching of N(mu_x, sigma_x) through the GP dynamics with u = k_fb x + k_ff; shapes as
    ``one_step_taylor``: mu_x (n_s,1), k_ff (n_u,1) -> mu_new (n_s,1), sigma_new (n_s,n_s), diag of the GP's output
    covariance (1,n_s)."""
    dev, n_s, n_u, ta, tb, tz = _mm_setup(ssm, a, b, a_gp_inp_x)
    if sigma_x is not None and k_fb is None:
        raise ValueError("k_fb is required when sigma_x is given")
    mu = B.as_dev(np.asarray(mu_x, dtype=np.float64).reshape(1, n_s), dev)
    kff = B.as_dev(np.asarray(k_ff, dtype=np.float64).reshape(1, n_u), dev)
    sigma = B.as_dev(sigma_x, dev, (1, n_s, n_s)) if sigma_x is not None else None
    K = B.as_dev(k_fb, dev, (1, n_u, n_s)) if sigma_x is not None else None
    mu_new, sigma_new, cov = _mm_step(ssm, mu, sigma, kff, K, ta, tb, tz)
    return (B.to_numpy(mu_new).reshape(n_s, 1), B.to_numpy(sigma_new)[0],
            B.to_numpy(torch.diagonal(cov, dim1=1, dim2=2)).reshape(1, n_s))


def multi_step_moment_matching(mu_0, ssm, k_ff, k_fb, sigma_0=None, a=None, b=None, a_gp_inp_x=None):
    """Exact moment matching over H steps; shapes as ``multi_step_taylor``: k_ff (H,n_u), k_fb H-1 gains (n_u,n_s);
    ``sigma_0`` (n_s,n_s) is supported.  Returns mu_all (H,n_s), sigma_all (H,n_s*n_s), diag of the GP's output covariance
    (H,n_s)."""
    k_ff = np.asarray(k_ff, dtype=np.float64)
    H, n_u = k_ff.shape
    n_s = np.shape(mu_0)[0]
    kfb = np.asarray(k_fb, dtype=np.float64).reshape(H - 1, n_u, n_s)[None] if H > 1 else None
    s0 = None if sigma_0 is None else np.asarray(sigma_0, dtype=np.float64).reshape(1, n_s, n_s)
    mu_all, sigma_all, cov_all = moment_matching_batch(np.asarray(mu_0, dtype=np.float64).reshape(1, n_s), ssm, k_ff[None],
                                                       kfb, a, b, s0, a_gp_inp_x)
    return mu_all[0], sigma_all[0].reshape(H, n_s * n_s), np.diagonal(cov_all[0], axis1=1, axis2=2).copy()
