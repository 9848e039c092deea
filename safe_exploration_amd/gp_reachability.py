"""Ellipsoidal one-step / multi-step reachability on MI355X.

Same function names, positional orders and return conventions as
/root/reference/safe_exploration/gp_reachability.py:19-250; the ``*_batch`` variants carry a
leading T axis (T query states / T candidate trajectories) and are what the benchmark measures.
All arithmetic happens in the HIP kernels behind include/safereach.h:

  * ssm is a HIP ``SimpleGPModel``  -> sr_onestep_reach / sr_multistep_reach (GP + ellipsoid fused
    on the device, nothing returns to the host between the kernels),
  * any other StateSpaceModel     -> its ``ssm(x, u)`` is called on the host exactly like the
    reference does (gp_reachability.py:74,101) and the ellipsoid algebra runs in sr_ellipsoid_step.

Beyond the reference: the reverse pass of ONE step on the device (``ellipsoid_step_vjp_batch`` / ``sr_ellipsoid_step_vjp``,
``onestep_reachability_vjp_batch`` / ``sr_onestep_reach_vjp``) and, on top of it, ``differentiable=True`` on the three batched
entry points: the forward stays the plain call (the same bits), the backward is the device reverse pass, steps are chained by
torch autograd.  Gradients reach the centres, shape matrices and controls (and mu, var, jac of ``ellipsoid_step_batch``), not
the model.  Mode 0 here (the moment modes: uncertainty_propagation_casadi); D <= 8.  A whole roll-out is differentiated in one
call by ``multistep_reachability_vjp_batch`` / ``sr_multistep_reach_vjp`` (one linearisation pass over all T*H steps, then a
sweep); ``multistep_reachability_diff_batch`` is the autograd surface over it, its forward the plain one-launch roll-out.
The exploration objective (the reference's default MPC cost, a function of the GP variances of a roll-out): the variances come
back with ``return_gp_var=True``, take a seed of their own in the reverse pass (``gpvar_all_bar``), and the objective with its
closed-form gradient is ``exploration_cost_batch`` / ``exploration_cost_vjp_batch`` (``sr_rollout_explore``, one launch each);
``safempc_default_cost`` is the reference's expression on the host.
"""
import ctypes

import numpy as np
import torch

from . import _buffers as B
from ._lib import lib, check
from .ssm_hip.gaussian_process import SimpleGPModel
from .utils import print_ellipsoid


def _lin_model(a, b, n_s, n_u):
    if a is None:                      # gp_reachability.py:61-63
        a = np.eye(n_s)
        b = np.zeros((n_s, n_u))
    return np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)


class _input_transform(object):
    """``with _input_transform(ssm, t_z_gp):`` -- the GP is evaluated at t_z_gp @ state for the reachability calls
    inside the block (gp_reachability_casadi.py:60-61,85,94-97); restored to the identity afterwards."""

    def __init__(self, ssm, t_z_gp):
        self.hd, self.t = ssm._handle, t_z_gp

    def __enter__(self):
        if self.t is not None:
            hd = self.hd
            t = np.asarray(self.t, dtype=np.float64)
            if t.ndim != 2 or t.shape[1] != hd.n_out or not (1 <= t.shape[0] < hd.D):
                raise ValueError("t_z_gp must be (n_x_in, {}) with n_x_in < D = {}".format(hd.n_out, hd.D))
            self.dev_t = B.as_dev(t, hd.device)
            check(lib.sr_gp_set_input_transform(hd.h, B.ptr(self.dev_t), int(t.shape[0]), B.stream_ptr(hd.device)))
        return self

    def __exit__(self, *exc):
        if self.t is not None:
            check(lib.sr_gp_set_input_transform(self.hd.h, None, 0, B.stream_ptr(self.hd.device)))
        return False


def _reach_dims(hd, t_z_gp):
    """(n_s, n_u) of the reachability problem on this model: D = n_x_in + n_u with n_x_in = rows of t_z_gp"""
    n_xin = hd.n_out if t_z_gp is None else int(np.shape(t_z_gp)[0])
    if hd.D - n_xin < 1:
        raise ValueError("the model has {} inputs for {} states: a GP input transform (t_z_gp / a_gp_inp_x, "
                         "(n_x_in, n_s) with n_x_in < {}) is needed".format(hd.D, hd.n_out, hd.D))
    return hd.n_out, hd.D - n_xin


def _raise_if_bad(n_bad):
    if n_bad is not None and int(n_bad.item()) > 0:
        # the reference asserts inside ellipsoid_from_rectangle (utils_ellipsoid.py:226-228)
        raise AssertionError("all elements of u_b need to be greater than zero! "
                             "({} query state(s) affected)".format(int(n_bad.item())))


def chain_timed_out(hd, sync_device=None):
    """True if a persistent multi-step launch of this handle failed since the last query: its workgroups did not become
    co-resident within 100 ms and it filled its outputs with NaN (``sr_gp_chain_status``).  Synchronises the current
    stream first when a device is given -- the status word is only final once the launch has ended."""
    if sync_device is not None:
        torch.cuda.current_stream(sync_device).synchronize()
    flag = ctypes.c_int(0)
    check(lib.sr_gp_chain_status(hd.h, ctypes.byref(flag)))
    return bool(flag.value)


def _raise_if_chain_failed(hd, dev, synced):
    """After a call whose results the caller is about to read on the host: never hand NaN ellipsoids back silently."""
    if lib.sr_gp_last_chain(hd.h) and chain_timed_out(hd, None if synced else dev):
        raise RuntimeError("libsafereach: the persistent multi-step kernel timed out (its workgroups were not co-resident "
                           "within 100 ms: the device was busy with other work); the model now uses per-step launches -- "
                           "repeat the call")


def onestep_reachability_batch(p_center, ssm, k_ff, l_mu, l_sigma, q_shape=None, k_fb=None,
                               c_safety=1., a=None, b=None, check_bounds=False, return_var=False, t_z_gp=None,
                               differentiable=False):
    """Batched ``onestep_reachability``.

    p_center (T,n_s); k_ff (T,n_u); q_shape (T,n_s,n_s) or None; k_fb (T,n_u,n_s) or None.
    numpy in -> numpy out, torch (device) in -> torch out.  Requires a HIP ``SimpleGPModel``.
    t_z_gp (n_x_in, n_s): the GP's state inputs are t_z_gp @ state (the argument of the same name of
    gp_reachability_casadi.onestep_reachability, :17-19,60-61); the model then has D = n_x_in + n_u inputs.
    Returns p_new (T,n_s), q_new (T,n_s,n_s) [, var (T,n_s)].
    differentiable (tensors only): p_new and q_new, the same bits, carry an autograd graph to p_center, q_shape, k_ff and k_fb
    whose backward is ``onestep_reachability_vjp_batch`` (once differentiable; no gradient to the model or to var).
    """
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("onestep_reachability_batch needs the HIP SimpleGPModel")
    if differentiable:
        if not B.is_tensor(p_center):
            raise TypeError("differentiable=True needs tensors")
        p1, q1, var = _OnestepReachFn.apply(ssm, (l_mu, l_sigma, c_safety, a, b, check_bounds, t_z_gp), p_center, q_shape,
                                            k_ff, k_fb if q_shape is not None else None)
        return (p1, q1, var) if return_var else (p1, q1)
    as_t = B.is_tensor(p_center)
    hd = ssm._handle
    ssm._need_trained()
    dev = hd.device
    n_s, n_u = _reach_dims(hd, t_z_gp)
    if q_shape is not None and k_fb is None:
        raise ValueError("k_fb is required when q_shape is given")
    staged = (not as_t) and not any(B.is_tensor(x) for x in (k_ff, q_shape, k_fb))
    if staged:
        np_p = np.ascontiguousarray(np.asarray(p_center, dtype=np.float64))
        staged = np_p.ndim == 2 and np_p.shape[0] * (n_s * n_s + n_s + n_u * n_s + n_u) <= B.STAGING_MAX_DOUBLES
    if staged:
        # NumPy in / out: every argument through one pinned block, every result back through one (B.Staging)
        f64 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        T = np_p.shape[0]
        if np_p.shape[1] != n_s:
            raise ValueError("p_center must be (T, {})".format(n_s))
        np_q = f64(q_shape).reshape(T, n_s, n_s) if q_shape is not None else None
        np_kfb = f64(k_fb).reshape(T, n_u, n_s) if (k_fb is not None and q_shape is not None) else None
        st = getattr(hd, "_staging", None)
        if st is None:
            st = hd._staging = B.Staging(dev)
        shapes = [(T, n_s), (T, n_s, n_s), (1,)] + ([(T, n_s)] if return_var else [])
        (p, kff, q, kfb), outs_d = st.stage([np_p, f64(k_ff).reshape(T, n_u), np_q, np_kfb], shapes, zero_copy=True)
        p_out, q_out, bad_slot = outs_d[:3]
        var = outs_d[3] if return_var else None
        n_bad = None
        if check_bounds:
            bad_slot.zero_()
            n_bad = bad_slot.view(torch.int32)
    else:
        p = B.as_dev(p_center, dev)
        T = p.shape[0]
        if p.dim() != 2 or p.shape[1] != n_s:
            raise ValueError("p_center must be (T, {})".format(n_s))
        kff = B.as_dev(k_ff, dev, (T, n_u))
        q = B.as_dev(q_shape, dev, (T, n_s, n_s)) if q_shape is not None else None
        kfb = B.as_dev(k_fb, dev, (T, n_u, n_s)) if (k_fb is not None and q is not None) else None
        p_out = B.empty((T, n_s), dev)
        q_out = B.empty((T, n_s, n_s), dev)
        var = B.empty((T, n_s), dev) if return_var else None
        n_bad = B.zeros_i32(1, dev) if check_bounds else None
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(l_mu, dev, (n_s,)), B.const_dev(l_sigma, dev, (n_s,))
    with _input_transform(ssm, t_z_gp):
        check(lib.sr_onestep_reach(hd.h, T, B.ptr(p), B.ptr(q), B.ptr(kff), B.ptr(kfb), B.ptr(ta),
                                   B.ptr(tb), B.ptr(tlm), B.ptr(tls), float(c_safety), B.ptr(p_out),
                                   B.ptr(q_out), B.ptr(var), B.ptr(n_bad), B.stream_ptr(dev)))
    if staged:
        res = st.fetch()                              # (synchronises the stream)
        if check_bounds:
            n_viol = int(res[2].view(np.int32)[0])
            if n_viol > 0:
                raise AssertionError("all elements of u_b need to be greater than zero! "
                                     "({} query state(s) affected)".format(n_viol))
        _raise_if_chain_failed(hd, dev, True)
        return (res[0], res[1], res[3]) if return_var else (res[0], res[1])
    _raise_if_bad(n_bad)
    outs = (p_out, q_out, var) if return_var else (p_out, q_out)
    if as_t:
        return outs          # device tensors, nothing synchronised: a failed chain is reported by the next entry point
    _raise_if_chain_failed(hd, dev, n_bad is not None)
    return tuple(B.to_numpy(o) for o in outs)


def ellipsoid_step_batch(p_center, k_ff, mu, var, jac, l_mu, l_sigma, q_shape=None, k_fb=None,
                         c_safety=1., a=None, b=None, check_bounds=False, device=None, differentiable=False):
    """The ellipsoid algebra of gp_reachability.py:65-156 for T queries whose GP outputs
    (mu (T,n_s), var (T,n_s), jac (T,n_s,n_s+n_u)) are supplied by the caller.
    differentiable (tensors only): the outputs, the same bits, carry an autograd graph to p_center, q_shape, k_ff, k_fb, mu, var
    and jac whose backward is ``ellipsoid_step_vjp_batch`` (once differentiable)."""
    if differentiable:
        if not B.is_tensor(p_center):
            raise TypeError("differentiable=True needs tensors")
        return _EllipsoidStepFn.apply((l_mu, l_sigma, c_safety, a, b, check_bounds), p_center, q_shape, k_ff,
                                      k_fb if q_shape is not None else None, mu, var, jac if q_shape is not None else None)
    as_t = B.is_tensor(p_center)
    dev = B.resolve_device(p_center.device if as_t else device)
    p = B.as_dev(p_center, dev)
    T, n_s = p.shape
    kff = B.as_dev(k_ff, dev).reshape(T, -1)
    n_u = kff.shape[1]
    tmu, tvar = B.as_dev(mu, dev, (T, n_s)), B.as_dev(var, dev, (T, n_s))
    q = B.as_dev(q_shape, dev, (T, n_s, n_s)) if q_shape is not None else None
    if q is not None and (k_fb is None or jac is None):
        raise ValueError("k_fb and jac are required when q_shape is given")
    kfb = B.as_dev(k_fb, dev, (T, n_u, n_s)) if q is not None else None
    tjac = B.as_dev(jac, dev, (T, n_s, n_s + n_u)) if (jac is not None and q is not None) else None
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(l_mu, dev, (n_s,)), B.const_dev(l_sigma, dev, (n_s,))
    p_out = B.empty((T, n_s), dev)
    q_out = B.empty((T, n_s, n_s), dev)
    n_bad = B.zeros_i32(1, dev) if check_bounds else None
    check(lib.sr_ellipsoid_step(dev.index, T, n_s, n_u, B.ptr(p), B.ptr(q), B.ptr(kff), B.ptr(kfb),
                                B.ptr(tmu), B.ptr(tvar), B.ptr(tjac), B.ptr(ta), B.ptr(tb),
                                B.ptr(tlm), B.ptr(tls), float(c_safety), B.ptr(p_out), B.ptr(q_out),
                                B.ptr(n_bad), B.stream_ptr(dev)))
    _raise_if_bad(n_bad)
    return (p_out, q_out) if as_t else (B.to_numpy(p_out), B.to_numpy(q_out))


def _seed_pair(p1_bar, q1_bar, dev, T, n_s):
    if p1_bar is None and q1_bar is None:
        raise ValueError("at least one of p1_bar, q1_bar is needed")
    return B.as_dev(p1_bar, dev, (T, n_s)), B.as_dev(q1_bar, dev, (T, n_s, n_s))


def ellipsoid_step_vjp_batch(p_center, k_ff, mu, var, jac, l_mu, l_sigma, p1_bar=None, q1_bar=None, q_shape=None, k_fb=None,
                             c_safety=1., a=None, b=None, device=None):
    """Reverse pass of ``ellipsoid_step_batch`` (``sr_ellipsoid_step_vjp``): for seeds p1_bar (T,n_s), q1_bar (T,n_s,n_s) on its two
    outputs (None = zero) the gradients (p_bar, q_bar, kff_bar, kfb_bar, mu_bar, var_bar, jac_bar), shaped like the inputs;
    q_bar, kfb_bar and jac_bar are None in the point branch (q_shape None).  Only the symmetric part of q1_bar counts, q_bar is
    exactly symmetric, a query the forward would count as a bound violation is NaN.  numpy in -> numpy out, tensors in ->
    tensors out."""
    as_t = B.is_tensor(p_center)
    dev = B.resolve_device(p_center.device if as_t else device)
    p = B.as_dev(p_center, dev)
    T, n_s = p.shape
    kff = B.as_dev(k_ff, dev).reshape(T, -1)
    n_u = kff.shape[1]
    tmu, tvar = B.as_dev(mu, dev, (T, n_s)), B.as_dev(var, dev, (T, n_s))
    q = B.as_dev(q_shape, dev, (T, n_s, n_s)) if q_shape is not None else None
    if q is not None and (k_fb is None or jac is None):
        raise ValueError("k_fb and jac are required when q_shape is given")
    kfb = B.as_dev(k_fb, dev, (T, n_u, n_s)) if q is not None else None
    tjac = B.as_dev(jac, dev, (T, n_s, n_s + n_u)) if q is not None else None
    pb, qb = _seed_pair(p1_bar, q1_bar, dev, T, n_s)
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(l_mu, dev, (n_s,)), B.const_dev(l_sigma, dev, (n_s,))
    ell = q is not None
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if ell else None, B.empty((T, n_u), dev),
            B.empty((T, n_u, n_s), dev) if ell else None, B.empty((T, n_s), dev), B.empty((T, n_s), dev),
            B.empty((T, n_s, n_s + n_u), dev) if ell else None]
    check(lib.sr_ellipsoid_step_vjp(dev.index, T, n_s, n_u, B.ptr(p), B.ptr(q), B.ptr(kff), B.ptr(kfb), B.ptr(tmu), B.ptr(tvar),
                                    B.ptr(tjac), B.ptr(ta), B.ptr(tb), B.ptr(tlm), B.ptr(tls), float(c_safety), B.ptr(pb),
                                    B.ptr(qb), *[B.ptr(o) for o in outs], B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


def onestep_reachability_vjp_batch(p_center, ssm, k_ff, l_mu, l_sigma, p1_bar=None, q1_bar=None, q_shape=None, k_fb=None,
                                   c_safety=1., a=None, b=None, t_z_gp=None):
    """Reverse pass of ``onestep_reachability_batch``, GP included (``sr_onestep_reach_vjp``: a batched linearisation at
    z = [t_z_gp p; k_ff], then one launch with the reverse of the ellipsoid algebra and the GP link): for seeds p1_bar (T,n_s),
    q1_bar (T,n_s,n_s) (None = zero) the gradients (p_bar, q_bar, kff_bar, kfb_bar); q_bar and kfb_bar are None in the point
    branch.  Models as ``linearize_device_batch`` takes them (every kernel, exact and sparse, D <= 8: NotImplementedError
    beyond).  numpy in -> numpy out, tensors in -> tensors out."""
    if not isinstance(ssm, SimpleGPModel):
        raise TypeError("onestep_reachability_vjp_batch needs the HIP SimpleGPModel")
    as_t = B.is_tensor(p_center)
    hd = ssm._handle
    ssm._need_trained()
    dev = hd.device
    n_s, n_u = _reach_dims(hd, t_z_gp)
    if q_shape is not None and k_fb is None:
        raise ValueError("k_fb is required when q_shape is given")
    p = B.as_dev(p_center, dev)
    T = p.shape[0]
    if p.dim() != 2 or p.shape[1] != n_s:
        raise ValueError("p_center must be (T, {})".format(n_s))
    kff = B.as_dev(k_ff, dev, (T, n_u))
    q = B.as_dev(q_shape, dev, (T, n_s, n_s)) if q_shape is not None else None
    kfb = B.as_dev(k_fb, dev, (T, n_u, n_s)) if q is not None else None
    pb, qb = _seed_pair(p1_bar, q1_bar, dev, T, n_s)
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(l_mu, dev, (n_s,)), B.const_dev(l_sigma, dev, (n_s,))
    ell = q is not None
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if ell else None, B.empty((T, n_u), dev),
            B.empty((T, n_u, n_s), dev) if ell else None]
    with _input_transform(ssm, t_z_gp):
        check(lib.sr_onestep_reach_vjp(hd.h, T, B.ptr(p), B.ptr(q), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb), B.ptr(tlm),
                                       B.ptr(tls), float(c_safety), B.ptr(pb), B.ptr(qb), *[B.ptr(o) for o in outs],
                                       B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _OnestepReachFn(torch.autograd.Function):
    """``onestep_reachability_batch(..., differentiable=True)``: the forward is the plain call, the backward
    ``onestep_reachability_vjp_batch`` at the saved inputs.  Seeds of outputs nobody used arrive as None (= zero, the same
    bits); the variance output carries no gradient."""

    @staticmethod
    def forward(ctx, ssm, cfg, p, q, k_ff, k_fb):
        l_mu, l_sigma, c_safety, a, b, check_bounds, t_z_gp = cfg
        p1, q1, var = onestep_reachability_batch(p, ssm, k_ff, l_mu, l_sigma, q, k_fb, c_safety, a, b, check_bounds, True, t_z_gp)
        ctx.ssm, ctx.cfg = ssm, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p, q, k_ff, k_fb)
        ctx.mark_non_differentiable(var)
        return p1, q1, var

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, p1_bar, q1_bar, _var_bar):
        p, q, k_ff, k_fb = ctx.saved_tensors
        l_mu, l_sigma, c_safety, a, b, _, t_z_gp = ctx.cfg
        if p1_bar is None and q1_bar is None:
            return (None,) * 6
        p_bar, q_bar, kff_bar, kfb_bar = onestep_reachability_vjp_batch(p, ctx.ssm, k_ff, l_mu, l_sigma, p1_bar, q1_bar, q, k_fb,
                                                                        c_safety, a, b, t_z_gp)
        return None, None, p_bar, q_bar, kff_bar.reshape(k_ff.shape), kfb_bar


class _EllipsoidStepFn(torch.autograd.Function):
    """``ellipsoid_step_batch(..., differentiable=True)``, likewise over ``ellipsoid_step_vjp_batch``."""

    @staticmethod
    def forward(ctx, cfg, p, q, k_ff, k_fb, mu, var, jac):
        l_mu, l_sigma, c_safety, a, b, check_bounds = cfg
        p1, q1 = ellipsoid_step_batch(p, k_ff, mu, var, jac, l_mu, l_sigma, q, k_fb, c_safety, a, b, check_bounds)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p, q, k_ff, k_fb, mu, var, jac)
        return p1, q1

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, p1_bar, q1_bar):
        p, q, k_ff, k_fb, mu, var, jac = ctx.saved_tensors
        l_mu, l_sigma, c_safety, a, b, _ = ctx.cfg
        if p1_bar is None and q1_bar is None:
            return (None,) * 8
        g = ellipsoid_step_vjp_batch(p, k_ff, mu, var, jac, l_mu, l_sigma, p1_bar, q1_bar, q, k_fb, c_safety, a, b)
        return (None, g[0], g[1], g[2].reshape(k_ff.shape), g[3], g[4].reshape(mu.shape), g[5].reshape(var.shape), g[6])


def onestep_reachability(p_center, ssm, k_ff, l_mu, l_sigma, q_shape=None, k_fb=None,
                         c_safety=1., verbose=1, a=None, b=None, t_z_gp=None):
    """Overapproximate the reachable set of states under the affine control law u = K(x-p) + k.

    Single-query semantics and argument order of gp_reachability.py:19-156.
    p_center (n_s,1); k_ff (n_u,1); q_shape (n_s,n_s) or None; k_fb (n_u,n_s) or None.
    Returns p_new (n_s,1), q_new (n_s,n_s).
    """
    p_center = np.asarray(p_center, dtype=np.float64)
    k_ff = np.asarray(k_ff, dtype=np.float64)
    n_s = np.shape(p_center)[0]
    n_u = np.shape(k_ff)[0]
    if verbose > 0:
        if q_shape is not None:
            print_ellipsoid(p_center, q_shape, text="initial uncertainty ellipsoid")
        print("\nApplying action:")
        print(k_ff)
    q_b = None if q_shape is None else np.asarray(q_shape, dtype=np.float64)[None]
    kfb_b = None if (k_fb is None or q_shape is None) else np.asarray(k_fb, dtype=np.float64)[None]
    if isinstance(ssm, SimpleGPModel):
        p1, q1 = onestep_reachability_batch(p_center.T, ssm, k_ff.T, l_mu, l_sigma, q_b, kfb_b,
                                            c_safety, a, b, check_bounds=True, t_z_gp=t_z_gp)
    else:
        x_bar = p_center if t_z_gp is None else np.asarray(t_z_gp, dtype=np.float64).dot(p_center)
        out = ssm(x_bar.T, k_ff.T)                     # (mu n x 1, sigma n x 1, jac n x D)
        mu_0, sigm_0 = np.array(out[0], dtype=np.float64), np.array(out[1], dtype=np.float64)
        jac_mu = np.array(out[2], dtype=np.float64) if q_shape is not None else None
        if jac_mu is not None and t_z_gp is not None:   # chain rule through the constant input map
            t = np.asarray(t_z_gp, dtype=np.float64)
            jac_mu = np.hstack((jac_mu[:, :t.shape[0]].dot(t), jac_mu[:, t.shape[0]:]))
        jac_mu = jac_mu[None] if jac_mu is not None else None
        p1, q1 = ellipsoid_step_batch(p_center.T, k_ff.T, mu_0.reshape(1, n_s), sigm_0.reshape(1, n_s),
                                      jac_mu, l_mu, l_sigma, q_b, kfb_b, c_safety, a, b,
                                      check_bounds=True)
    p_1, q_1 = p1.reshape(n_s, 1), q1[0]
    if verbose > 0:
        print_ellipsoid(p_1, q_1, text="accumulated uncertainty current step")
    return p_1, q_1


def multistep_reachability_batch(p_0, gp, k_fb, k_ff, L_mu, L_sigm, q_0=None, c_safety=1., a=None,
                                 b=None, k_fb_init=None, check_bounds=False, t_z_gp=None, differentiable=False,
                                 return_gp_var=False):
    """Batched ``multistep_reachability``: T independent trajectories, H sequential steps each.

    p_0 (T,n_s); k_fb (T,H-1,n_u,n_s); k_ff (T,H,n_u); q_0 (T,n_s,n_s) or None;
    k_fb_init (T,n_u,n_s) (needed iff q_0 is given).  Returns p_all (T,H,n_s), q_all (T,H,n_s,n_s).
    return_gp_var: also gp_var_all (T,H,n_s), the GP's predictive variances at the linearisation point of every step (the
    reference's third output, gp_pred_sigma_all), through ``sr_multistep_reach_var``: p_all and q_all keep their bits.  With
    differentiable=True: NotImplementedError (``multistep_reachability_diff_batch(return_gp_var=True)`` is the surface for it).
    differentiable (tensors only): H differentiable one-step calls chained in torch (step 0 from the point, or from
    (q_0, k_fb_init), exactly as the forward), stacked into p_all, q_all with an autograd graph to p_0, q_0, k_fb_init, k_ff and
    k_fb.  Every step is one ``sr_onestep_reach`` call, so the values are those of the forward's per-step-launch route
    (``gp.set_chain(False)``: a K* pass, the variance contraction and the ellipsoid kernel per step), to the bit, wherever one
    step takes that route itself: for n_s >= 3 always, for n_s <= 2 with ``gp.set_chain(False)`` around this call as well (a
    one-step call of a small model with n_s <= 2 otherwise runs posterior and step in one launch of its own and agrees with the
    per-step route to rounding).  The reverse pass of the whole roll-out in one call, behind the one-launch forward:
    ``multistep_reachability_diff_batch`` (``multistep_reachability_vjp_batch``).
    """
    if not isinstance(gp, SimpleGPModel):
        raise TypeError("multistep_reachability_batch needs the HIP SimpleGPModel")
    gp._need_trained()
    if differentiable and return_gp_var:
        raise NotImplementedError("return_gp_var with differentiable=True: use multistep_reachability_diff_batch(return_gp_var=True)")
    if differentiable:
        if not B.is_tensor(p_0):
            raise TypeError("differentiable=True needs tensors")
        if q_0 is not None and k_fb_init is None:
            raise ValueError("k_fb_init is required when q_0 is given")
        H = k_ff.shape[1]
        p, q, ps, qs = p_0, q_0, [], []
        for i in range(H):
            kfb_i = (k_fb_init if q_0 is not None else None) if i == 0 else k_fb[:, i - 1]
            p, q = onestep_reachability_batch(p, gp, k_ff[:, i], L_mu, L_sigm, q, kfb_i, c_safety, a, b,
                                              check_bounds=check_bounds, t_z_gp=t_z_gp, differentiable=True)
            ps.append(p)
            qs.append(q)
        return torch.stack(ps, dim=1), torch.stack(qs, dim=1)
    as_t = B.is_tensor(p_0)
    hd = gp._handle
    dev = hd.device
    n_s, n_u = _reach_dims(hd, t_z_gp)
    if q_0 is not None and k_fb_init is None:
        raise ValueError("k_fb_init is required when q_0 is given")
    staged = (not as_t) and not any(B.is_tensor(x) for x in (k_fb, k_ff, q_0, k_fb_init))
    if staged:
        staged = np.size(k_ff) * (n_s * n_s + n_s + 1) <= B.STAGING_MAX_DOUBLES * max(n_u, 1)
    if staged:
        # NumPy in / out: every argument through one pinned block, every result back through one (B.Staging)
        f64 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        np_p0, np_kff = f64(p_0), f64(k_ff)
        T = np_p0.shape[0]
        if np_kff.ndim != 3 or np_kff.shape[0] != T or np_kff.shape[2] != n_u:
            raise ValueError("k_ff must be (T, H, {})".format(n_u))
        H = np_kff.shape[1]
        np_kfb = f64(k_fb).reshape(T, H - 1, n_u, n_s) if H > 1 else None
        np_q0 = f64(q_0).reshape(T, n_s, n_s) if q_0 is not None else None
        np_kfb0 = f64(k_fb_init).reshape(T, n_u, n_s) if q_0 is not None else None
        st = getattr(hd, "_staging", None)
        if st is None:
            st = hd._staging = B.Staging(dev)
        (p0, kff, kfb, q0, kfb0), outs_d = st.stage(
            [np_p0.reshape(T, n_s), np_kff, np_kfb, np_q0, np_kfb0],
            [(T, H, n_s), (T, H, n_s, n_s), (1,)] + ([(T, H, n_s)] if return_gp_var else []), zero_copy=True)
        p_all, q_all, bad_slot = outs_d[:3]
        gp_var = outs_d[3] if return_gp_var else None
    else:
        p0 = B.as_dev(p_0, dev)
        T = p0.shape[0]
        kff = B.as_dev(k_ff, dev)
        if kff.dim() != 3 or kff.shape[0] != T or kff.shape[2] != n_u:
            raise ValueError("k_ff must be (T, H, {})".format(n_u))
        H = kff.shape[1]
        kfb = B.as_dev(k_fb, dev, (T, H - 1, n_u, n_s)) if H > 1 else None
        q0 = B.as_dev(q_0, dev, (T, n_s, n_s)) if q_0 is not None else None
        kfb0 = B.as_dev(k_fb_init, dev, (T, n_u, n_s)) if q0 is not None else None
        p_all = B.empty((T, H, n_s), dev)
        q_all = B.empty((T, H, n_s, n_s), dev)
        gp_var = B.empty((T, H, n_s), dev) if return_gp_var else None
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(L_mu, dev, (n_s,)), B.const_dev(L_sigm, dev, (n_s,))
    if staged and check_bounds:
        # the violation counter travels back inside the packed result block (its own D2H copy + synchronisation otherwise)
        bad_slot.zero_()
        n_bad = bad_slot.view(torch.int32)
    else:
        n_bad = B.zeros_i32(1, dev) if check_bounds else None
    with _input_transform(gp, t_z_gp):
        head = (hd.h, T, H, B.ptr(p0), B.ptr(q0), B.ptr(kfb0), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb), B.ptr(tlm), B.ptr(tls),
                float(c_safety), B.ptr(p_all), B.ptr(q_all))
        if return_gp_var:
            check(lib.sr_multistep_reach_var(*head, B.ptr(gp_var), B.ptr(n_bad), B.stream_ptr(dev)))
        else:
            check(lib.sr_multistep_reach(*head, B.ptr(n_bad), B.stream_ptr(dev)))
    if as_t:
        _raise_if_bad(n_bad)
        return (p_all, q_all, gp_var) if return_gp_var else (p_all, q_all)
    if staged:
        fetched = st.fetch()                          # (synchronises the stream)
        p_np, q_np, bad_np = fetched[:3]
        if check_bounds:
            n_viol = int(bad_np.view(np.int32)[0])
            if n_viol > 0:
                raise AssertionError("all elements of u_b need to be greater than zero! "
                                     "({} query state(s) affected)".format(n_viol))
        _raise_if_chain_failed(hd, dev, True)
        return (p_np, q_np, fetched[3]) if return_gp_var else (p_np, q_np)
    _raise_if_bad(n_bad)
    _raise_if_chain_failed(hd, dev, n_bad is not None)
    if return_gp_var:
        return B.to_numpy(p_all), B.to_numpy(q_all), B.to_numpy(gp_var)
    return B.to_numpy(p_all), B.to_numpy(q_all)


def multistep_reachability_vjp_batch(p_0, gp, k_fb, k_ff, L_mu, L_sigm, p_all, q_all, p_all_bar=None, q_all_bar=None, q_0=None,
                                     c_safety=1., a=None, b=None, k_fb_init=None, t_z_gp=None, gpvar_all_bar=None):
    """Reverse pass of ``multistep_reachability_batch`` in one call (``sr_multistep_reach_vjp``): one batched linearisation at the
    inputs of all T*H steps -- the centres p_all are known --, then a sweep over the steps, one thread per trajectory.

    The forward arguments as ``multistep_reachability_batch`` takes them; p_all (T,H,n_s), q_all (T,H,n_s,n_s) are what it
    returned; seeds p_all_bar, q_all_bar of those shapes (None = zero, not both).  Returns the gradients of
    sum(p_all_bar * p_all) + sum(q_all_bar * q_all): (p0_bar, q0_bar, kfb_init_bar, kff_bar, kfb_bar), shaped like p_0, q_0,
    k_fb_init, k_ff and k_fb; q0_bar and kfb_init_bar are None in a point start (q_0 None).  Only the symmetric part of q_all_bar
    counts, q0_bar is exactly symmetric, a step the forward would count as a bound violation turns the gradients that flow
    through it into NaN.  The same bits on every call and for any ``set_chunk``.  Models as ``linearize_device_batch`` takes
    them (D <= 8: NotImplementedError beyond).  numpy in -> numpy out, tensors in -> tensors out.
    gpvar_all_bar (T,H,n_s): a third seed, on the gp_var_all of ``multistep_reachability_batch(return_gp_var=True)``
    (``sr_multistep_reach_var_vjp``; the clip of the variances is ignored); None: the call and the bits of before."""
    if not isinstance(gp, SimpleGPModel):
        raise TypeError("multistep_reachability_vjp_batch needs the HIP SimpleGPModel")
    as_t = B.is_tensor(p_0)
    hd = gp._handle
    gp._need_trained()
    dev = hd.device
    n_s, n_u = _reach_dims(hd, t_z_gp)
    if q_0 is not None and k_fb_init is None:
        raise ValueError("k_fb_init is required when q_0 is given")
    if p_all_bar is None and q_all_bar is None and gpvar_all_bar is None:
        raise ValueError("at least one of p_all_bar, q_all_bar, gpvar_all_bar is needed")
    p0 = B.as_dev(p_0, dev)
    T = p0.shape[0]
    if p0.dim() != 2 or p0.shape[1] != n_s:
        raise ValueError("p_0 must be (T, {})".format(n_s))
    kff = B.as_dev(k_ff, dev)
    if kff.dim() != 3 or kff.shape[0] != T or kff.shape[2] != n_u:
        raise ValueError("k_ff must be (T, H, {})".format(n_u))
    H = kff.shape[1]
    if H < 1:
        raise ValueError("k_ff must hold at least one step")
    def shaped(x, shape, name):
        try:
            return B.as_dev(x, dev, shape)
        except RuntimeError:
            raise ValueError("{} must be {}".format(name, shape))
    kfb = shaped(k_fb, (T, H - 1, n_u, n_s), "k_fb") if H > 1 else None
    q0 = shaped(q_0, (T, n_s, n_s), "q_0")
    kfb0 = shaped(k_fb_init, (T, n_u, n_s), "k_fb_init") if q0 is not None else None
    pa, qa = shaped(p_all, (T, H, n_s), "p_all"), shaped(q_all, (T, H, n_s, n_s), "q_all")
    pab, qab = shaped(p_all_bar, (T, H, n_s), "p_all_bar"), shaped(q_all_bar, (T, H, n_s, n_s), "q_all_bar")
    gvb = shaped(gpvar_all_bar, (T, H, n_s), "gpvar_all_bar")
    a, b = _lin_model(a, b, n_s, n_u)
    ta, tb = B.const_dev(a, dev, (n_s, n_s)), B.const_dev(b, dev, (n_s, n_u))
    tlm, tls = B.const_dev(L_mu, dev, (n_s,)), B.const_dev(L_sigm, dev, (n_s,))
    ell = q0 is not None
    outs = [B.empty((T, n_s), dev), B.empty((T, n_s, n_s), dev) if ell else None, B.empty((T, n_u, n_s), dev) if ell else None,
            B.empty((T, H, n_u), dev), B.empty((T, H - 1, n_u, n_s), dev)]
    with _input_transform(gp, t_z_gp):
        head = (hd.h, T, H, B.ptr(p0), B.ptr(q0), B.ptr(kfb0), B.ptr(kff), B.ptr(kfb), B.ptr(ta), B.ptr(tb), B.ptr(tlm), B.ptr(tls),
                float(c_safety), B.ptr(pa), B.ptr(qa), B.ptr(pab), B.ptr(qab))
        tail = [B.ptr(o) if o is not None and o.numel() else None for o in outs] + [B.stream_ptr(dev)]
        if gvb is None:
            check(lib.sr_multistep_reach_vjp(*head, *tail))
        else:
            check(lib.sr_multistep_reach_var_vjp(*head, B.ptr(gvb), *tail))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _MultistepReachFn(torch.autograd.Function):
    """``multistep_reachability_diff_batch``: the forward is the plain one-launch ``multistep_reachability_batch``, the backward
    ``multistep_reachability_vjp_batch`` at the saved p_all, q_all.  Seeds of outputs nobody used arrive as None."""

    @staticmethod
    def forward(ctx, gp, cfg, p_0, q_0, k_fb_init, k_ff, k_fb):
        L_mu, L_sigm, c_safety, a, b, check_bounds, t_z_gp = cfg
        p_all, q_all = multistep_reachability_batch(p_0, gp, k_fb, k_ff, L_mu, L_sigm, q_0, c_safety, a, b, k_fb_init,
                                                    check_bounds, t_z_gp)
        ctx.gp, ctx.cfg = gp, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p_0, q_0, k_fb_init, k_ff, k_fb, p_all, q_all)
        return p_all, q_all

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, p_all_bar, q_all_bar, gpvar_all_bar=None):
        p_0, q_0, k_fb_init, k_ff, k_fb, p_all, q_all = ctx.saved_tensors
        L_mu, L_sigm, c_safety, a, b, _, t_z_gp = ctx.cfg
        if p_all_bar is None and q_all_bar is None and gpvar_all_bar is None:
            return (None,) * 7
        g = multistep_reachability_vjp_batch(p_0, ctx.gp, k_fb, k_ff, L_mu, L_sigm, p_all, q_all, p_all_bar, q_all_bar, q_0,
                                             c_safety, a, b, k_fb_init, t_z_gp, gpvar_all_bar)
        return None, None, g[0], g[1], g[2], g[3], (g[4].reshape(k_fb.shape) if k_fb is not None else None)


class _MultistepReachVarFn(_MultistepReachFn):
    """``multistep_reachability_diff_batch(return_gp_var=True)``: three outputs (p_all, q_all, gp_var_all); the backward, inherited,
    is one ``sr_multistep_reach_var_vjp`` call."""

    @staticmethod
    def forward(ctx, gp, cfg, p_0, q_0, k_fb_init, k_ff, k_fb):
        L_mu, L_sigm, c_safety, a, b, check_bounds, t_z_gp = cfg
        p_all, q_all, gp_var = multistep_reachability_batch(p_0, gp, k_fb, k_ff, L_mu, L_sigm, q_0, c_safety, a, b, k_fb_init,
                                                            check_bounds, t_z_gp, return_gp_var=True)
        ctx.gp, ctx.cfg = gp, cfg
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(p_0, q_0, k_fb_init, k_ff, k_fb, p_all, q_all)
        return p_all, q_all, gp_var


def multistep_reachability_diff_batch(p_0, gp, k_fb, k_ff, L_mu, L_sigm, q_0=None, c_safety=1., a=None, b=None, k_fb_init=None,
                                      check_bounds=False, t_z_gp=None, return_gp_var=False):
    """``multistep_reachability_batch`` (tensors only) with an autograd graph to p_0, q_0, k_fb_init, k_ff and k_fb: the forward IS
    the plain call (the persistent one-launch chain where it applies; the same bits, ``check_bounds`` honoured), the backward is
    ONE ``multistep_reachability_vjp_batch`` call at the saved p_all, q_all (once differentiable; no gradient to the model).
    ``multistep_reachability_batch(differentiable=True)`` chains H one-step nodes instead and stays as it is.
    return_gp_var: a third output gp_var_all (T,H,n_s) with a gradient of its own (the exploration objectives are functions of it,
    ``exploration_cost_batch``); the backward is still one call, ``sr_multistep_reach_var_vjp``."""
    if not isinstance(gp, SimpleGPModel):
        raise TypeError("multistep_reachability_diff_batch needs the HIP SimpleGPModel")
    if not B.is_tensor(p_0):
        raise TypeError("multistep_reachability_diff_batch needs tensors")
    if q_0 is not None and k_fb_init is None:
        raise ValueError("k_fb_init is required when q_0 is given")
    fn = _MultistepReachVarFn if return_gp_var else _MultistepReachFn
    return fn.apply(gp, (L_mu, L_sigm, c_safety, a, b, check_bounds, t_z_gp), p_0, q_0,
                    k_fb_init if q_0 is not None else None, k_ff, k_fb if k_ff.shape[1] > 1 else None)


def multistep_reachability(p_0, gp, k_fb, k_ff, L_mu, L_sigm, q_0=None, c_safety=1., verbose=1,
                           a=None, b=None, k_fb_init=None, t_z_gp=None):
    """Ellipsoidal overapproximation after n actions (gp_reachability.py:159-212).

    p_0 (n_s,1); k_fb (n-1,n_u,n_s); k_ff (n,n_u).  Returns p_new (n_s,1), q_new (n_s,n_s),
    p_all (n,n_s), q_all (n,n_s,n_s).
    """
    k_fb = np.asarray(k_fb, dtype=np.float64)
    k_ff = np.asarray(k_ff, dtype=np.float64)
    n_, n_u, n_s = np.shape(k_fb)
    n = n_ + 1
    if isinstance(gp, SimpleGPModel):
        q0 = None if q_0 is None else np.asarray(q_0, dtype=np.float64)[None]
        kfb0 = None if (k_fb_init is None or q_0 is None) else np.asarray(k_fb_init, dtype=np.float64)[None]
        p_all, q_all = multistep_reachability_batch(np.asarray(p_0, dtype=np.float64).reshape(1, n_s), gp,
                                                    k_fb[None], k_ff[None], L_mu, L_sigm, q0, c_safety,
                                                    a, b, kfb0, check_bounds=True, t_z_gp=t_z_gp)
        p_all, q_all = p_all[0], q_all[0]
    else:
        p_all = np.empty((n, n_s))
        q_all = np.empty((n, n_s, n_s))
        p_new, q_new = onestep_reachability(p_0, gp, k_ff[0, :, None], L_mu, L_sigm, q_0, k_fb_init,
                                            c_safety, verbose, a, b, t_z_gp)
        p_all[0], q_all[0] = p_new.T, q_new
        for i in range(1, n):
            p_new, q_new = onestep_reachability(p_new, gp, k_ff[i, :, None], L_mu, L_sigm, q_new,
                                                k_fb[i - 1], c_safety, verbose, a, b, t_z_gp)
            p_all[i], q_all[i] = p_new.T, q_new
    return p_all[-1][:, None].copy(), q_all[-1].copy(), p_all, q_all


def lin_ellipsoid_safety_distance_batch(p_center, q_shape, h_mat, h_vec, c_safety=1.0, device=None):
    """d (T,m) = h_mat p + c sqrt(diag(h_mat Q h_mat^T)) - h_vec for T ellipsoids."""
    as_t = B.is_tensor(p_center)
    dev = B.resolve_device(p_center.device if as_t else device)
    p = B.as_dev(p_center, dev)
    T, n_s = p.shape
    q = B.as_dev(q_shape, dev, (T, n_s, n_s))
    hm = B.as_dev(h_mat, dev)
    m = hm.shape[0]
    if hm.dim() != 2 or hm.shape[1] != n_s:
        raise ValueError("h_mat must be (m, {})".format(n_s))
    hv = B.as_dev(np.reshape(B.to_numpy(h_vec) if B.is_tensor(h_vec) else h_vec, (-1,)), dev, (m,))
    d = B.empty((T, m), dev)
    check(lib.sr_safety_distance(dev.index, T, n_s, m, B.ptr(p), B.ptr(q), B.ptr(hm), B.ptr(hv),
                                 float(c_safety), B.ptr(d), B.stream_ptr(dev)))
    return d if as_t else B.to_numpy(d)


def lin_ellipsoid_safety_distance(p_center, q_shape, h_mat, h_vec, c_safety=1.0):
    """Distance between ellipsoid E(p,Q) and polytope h_mat x <= h_vec (gp_reachability.py:215-250).
    d < 0 (element-wise) <=> the ellipsoid is inside the polytope.  Returns (m,1)."""
    m, n_s = np.shape(h_mat)
    assert np.shape(p_center) == (n_s, 1), "p_center has to have shape n_s x 1"
    assert np.shape(q_shape) == (n_s, n_s), "q_shape has to have shape n_s x n_s"
    assert np.shape(h_vec) == (m, 1), "q_shape has to have shape m x 1"
    d = lin_ellipsoid_safety_distance_batch(np.asarray(p_center, dtype=np.float64).reshape(1, n_s),
                                            np.asarray(q_shape, dtype=np.float64)[None], h_mat, h_vec,
                                            c_safety)
    return d.reshape(m, 1)


# ------------------------------------------------------------------------------------------------
# the constraint vector of SimpleSafeMPC.generate_safety_constraints over stored roll-outs (safempc_simple.py:317-392, 488-532)
# ------------------------------------------------------------------------------------------------
def rollout_constraint_layout(H, n_u, m_obs, m_safe, has_bounds):
    """Host only: where the rows of ``rollout_constraints_batch`` sit.  Returns (blocks, names): blocks = dict(control=slice,
    obstacle=slice, terminal=slice) into the n_g = (2 n_u H if has_bounds) + m_obs (H - 1) + m_safe rows of a trajectory, names
    one string per row -- the reference's g_name strings: "u_0_ctrl_constraint" for the 2 n_u rows of step 0,
    "ellipsoid_ctrl_constraint_{i}" for those of step i + 1 (the reference counts from its k_fb[i]),
    "obstacle_avoidance_constraint{i}" for state i, "terminal constraint"."""
    H, n_u, m_obs, m_safe = int(H), int(n_u), int(m_obs), int(m_safe)
    if H < 1 or n_u < 0 or m_obs < 0 or m_safe < 0 or (has_bounds and n_u < 1):
        raise ValueError("need H >= 1, m_obs >= 0, m_safe >= 0 and n_u >= 1 with bounds")
    n_ctrl = 2 * n_u * H if has_bounds else 0
    n_obs = m_obs * (H - 1)
    blocks = dict(control=slice(0, n_ctrl), obstacle=slice(n_ctrl, n_ctrl + n_obs), terminal=slice(n_ctrl + n_obs, n_ctrl + n_obs + m_safe))
    names = []
    if has_bounds:
        names += ["u_0_ctrl_constraint"] * (2 * n_u)
        for i in range(H - 1):
            names += ["ellipsoid_ctrl_constraint_{}".format(i)] * (2 * n_u)
    for i in range(H - 1):
        names += ["obstacle_avoidance_constraint{}".format(i)] * m_obs
    names += ["terminal constraint"] * m_safe
    return blocks, names


def _constraints_prepare(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, q_0, k_fb_0, c_safety, device):
    """Shapes checked (ValueError, before anything touches the device), then everything on the device: the arguments both entry
    points share, in the order of the C ABI after `device`."""
    as_t = B.is_tensor(p_all)
    shp = tuple(np.shape(p_all))
    if len(shp) != 3 or shp[1] < 1 or shp[2] < 1:
        raise ValueError("p_all must be (T, H, n_s) with H >= 1")
    T, H, n_s = shp
    if tuple(np.shape(q_all)) != (T, H, n_s, n_s):
        raise ValueError("q_all must be {}".format((T, H, n_s, n_s)))
    has_bounds = ctrl_bounds is not None
    n_u = 0
    if k_ff is not None:
        ushp = tuple(np.shape(k_ff))
        if len(ushp) != 3 or ushp[:2] != (T, H):
            raise ValueError("k_ff must be (T, H, n_u)")
        n_u = ushp[2]
    if has_bounds:
        if k_ff is None or n_u < 1:
            raise ValueError("ctrl_bounds needs k_ff (T, H, n_u) with n_u >= 1")
        cb = np.asarray(B.to_numpy(ctrl_bounds) if B.is_tensor(ctrl_bounds) else ctrl_bounds, dtype=np.float64)
        if cb.shape != (n_u, 2):
            raise ValueError("ctrl_bounds must be ({}, 2)".format(n_u))
        if H > 1 and k_fb is None:
            raise ValueError("ctrl_bounds needs k_fb for H > 1")
    if k_fb is not None and H > 1 and int(np.prod(np.shape(k_fb))) != T * (H - 1) * n_u * n_s:
        raise ValueError("k_fb must be {}".format((T, H - 1, n_u, n_s)))
    if (q_0 is None) != (k_fb_0 is None):
        raise ValueError("q_0 and k_fb_0 go together")
    if q_0 is not None:
        if tuple(np.shape(q_0)) != (T, n_s, n_s):
            raise ValueError("q_0 must be {}".format((T, n_s, n_s)))
        if k_ff is None or tuple(np.shape(k_fb_0)) != (T, n_u, n_s):
            raise ValueError("k_fb_0 must be (T, n_u, n_s), with k_ff given")
    hs = []
    for hm, hv, what in ((h_mat_obs, h_obs, "obs"), (h_mat_safe, h_safe, "safe")):
        if (hm is None) != (hv is None):
            raise ValueError("h_mat_{0} and h_{0} go together".format(what))
        if hm is None:
            hs.append((0, None, None))
            continue
        hm = np.asarray(B.to_numpy(hm) if B.is_tensor(hm) else hm, dtype=np.float64)
        hv = np.asarray(B.to_numpy(hv) if B.is_tensor(hv) else hv, dtype=np.float64).reshape(-1)
        if hm.ndim != 2 or hm.shape[0] < 1 or hm.shape[1] != n_s or hv.size != hm.shape[0]:
            raise ValueError("h_mat_{0} must be (m, {1}) and h_{0} hold m entries".format(what, n_s))
        hs.append((hm.shape[0], hm, hv))
    (m_obs, hmo, hvo), (m_safe, hms, hvs) = hs
    n_g = (2 * n_u * H if has_bounds else 0) + m_obs * (H - 1) + m_safe
    if n_g == 0:
        raise ValueError("no constraint rows: give ctrl_bounds, obstacles (H > 1) or a terminal set")
    if n_s > 12 or n_u > 12:
        raise NotImplementedError("rollout constraints: n_s and n_u up to 12")
    dev = B.resolve_device(p_all.device if as_t else device)
    pa, qa, kff = B.as_dev(p_all, dev), B.as_dev(q_all, dev), B.as_dev(k_ff, dev)
    kfb = B.as_dev(k_fb, dev, (T, H - 1, n_u, n_s)) if (k_fb is not None and H > 1) else None
    q0, kfb0 = B.as_dev(q_0, dev), B.as_dev(k_fb_0, dev)
    umin = B.const_dev(cb[:, 0], dev, (n_u,)) if has_bounds else None
    umax = B.const_dev(cb[:, 1], dev, (n_u,)) if has_bounds else None
    dho = [None if x is None else B.const_dev(x, dev, x.shape) for x in (hmo, hvo, hms, hvs)]
    head = (dev.index, T, H, n_s, n_u, B.ptr(pa), B.ptr(qa), B.ptr(kff), B.ptr(kfb), B.ptr(q0), B.ptr(kfb0), B.ptr(umin), B.ptr(umax),
            m_obs, B.ptr(dho[0]), B.ptr(dho[1]), m_safe, B.ptr(dho[2]), B.ptr(dho[3]), float(c_safety))
    return as_t, dev, (T, H, n_s, n_u, n_g), head, (pa, qa, kff, kfb, q0, kfb0, umin, umax, dho)


def rollout_constraints_batch(p_all, q_all, k_ff, k_fb, ctrl_bounds=None, h_mat_obs=None, h_obs=None, h_mat_safe=None, h_safe=None,
                              q_0=None, k_fb_0=None, c_safety=1.0, return_max=False, differentiable=False, device=None):
    """The SafeMPC constraint rows of T roll-outs in one launch (``sr_rollout_constraints``; the reference's
    ``SimpleSafeMPC.generate_safety_constraints``).

    p_all (T,H,n_s), q_all (T,H,n_s,n_s): what ``multistep_reachability_batch`` returned; k_ff (T,H,n_u), k_fb (T,H-1,n_u,n_s):
    what it was given (both may be None without ctrl_bounds; k_fb None for H == 1); q_0 (T,n_s,n_s) with k_fb_0 (T,n_u,n_s) its
    ellipsoid start.  ctrl_bounds (n_u,2) = [u_min, u_max] as in the reference; (h_mat_obs (m_obs,n_s), h_obs) the obstacle
    half-spaces on the states 0 .. H-2, (h_mat_safe, h_safe) the terminal set on the last one.  Returns g (T,n_g), every row
    satisfied iff g <= 0, in the order of ``rollout_constraint_layout``; with return_max (g, g_max (T)): the largest row per
    trajectory (NaN if any row is NaN), g_max <= 0 iff the candidate is feasible.  c_safety scales every square root.  The rows work
    on mu_all / sigma_all of the moment roll-outs as they are (the chance constraints of CautiousMPC).  differentiable (tensors
    only): the same bits, with an autograd graph to p_all, q_all, k_ff, k_fb, q_0 and k_fb_0 whose backward is one
    ``rollout_constraints_vjp_batch`` call (once differentiable; g_max carries no gradient).  numpy in -> numpy out, tensors in ->
    tensors out."""
    if differentiable:
        if not B.is_tensor(p_all):
            raise TypeError("differentiable=True needs tensors")
        cfg = (ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, c_safety)
        out = _RolloutConstraintsFn.apply(cfg, p_all, q_all, k_ff, k_fb, q_0, k_fb_0)
        return out if return_max else out[0]
    as_t, dev, (T, H, n_s, n_u, n_g), head, keep = _constraints_prepare(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_mat_obs, h_obs,
                                                                       h_mat_safe, h_safe, q_0, k_fb_0, c_safety, device)
    g = B.empty((T, n_g), dev)
    g_max = B.empty((T,), dev) if return_max else None
    check(lib.sr_rollout_constraints(*head, B.ptr(g), B.ptr(g_max), B.stream_ptr(dev)))
    outs = (g, g_max) if return_max else (g,)
    if not as_t:
        outs = tuple(B.to_numpy(o) for o in outs)
    return outs if return_max else outs[0]


def rollout_constraints_vjp_batch(p_all, q_all, k_ff, k_fb, ctrl_bounds=None, h_mat_obs=None, h_obs=None, h_mat_safe=None,
                                  h_safe=None, q_0=None, k_fb_0=None, c_safety=1.0, g_bar=None, device=None):
    """Reverse pass of ``rollout_constraints_batch`` in one launch (``sr_rollout_constraints_vjp``): for the seed g_bar (T,n_g) the
    gradients of sum(g_bar * g): (p_all_bar, q_all_bar, kff_bar, kfb_bar, q0_bar, kfb0_bar), shaped like p_all, q_all, k_ff, k_fb,
    q_0, k_fb_0 (None where the input is None or empty).  q_all_bar and q0_bar are exactly symmetric.  p_all_bar / q_all_bar are the
    seeds of ``multistep_reachability_vjp_batch``; kff_bar / kfb_bar are added to what that call returns for k_ff / k_fb.  A radicand
    that is exactly zero (a zero k_fb row, q = 0) contributes zero through its square root; a negative one NaN in q_all_bar, kfb_bar
    of its own state only."""
    as_t, dev, (T, H, n_s, n_u, n_g), head, keep = _constraints_prepare(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_mat_obs, h_obs,
                                                                       h_mat_safe, h_safe, q_0, k_fb_0, c_safety, device)
    if g_bar is None or tuple(np.shape(g_bar)) != (T, n_g):
        raise ValueError("g_bar must be {}".format((T, n_g)))
    gb = B.as_dev(g_bar, dev)
    kfb, q0 = keep[3], keep[4]
    outs = [B.empty((T, H, n_s), dev), B.empty((T, H, n_s, n_s), dev),
            B.empty((T, H, n_u), dev) if (k_ff is not None and n_u) else None,
            B.empty((T, H - 1, n_u, n_s), dev) if kfb is not None else None,
            B.empty((T, n_s, n_s), dev) if q0 is not None else None, B.empty((T, n_u, n_s), dev) if q0 is not None else None]
    check(lib.sr_rollout_constraints_vjp(*head, B.ptr(gb), *[B.ptr(o) for o in outs], B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _RolloutConstraintsFn(torch.autograd.Function):
    """``rollout_constraints_batch(differentiable=True)``: the forward is the plain call, the backward one
    ``rollout_constraints_vjp_batch``."""

    @staticmethod
    def forward(ctx, cfg, p_all, q_all, k_ff, k_fb, q_0, k_fb_0):
        ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, c_safety = cfg
        g, g_max = rollout_constraints_batch(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, q_0, k_fb_0,
                                             c_safety, True)
        ctx.cfg = cfg
        ctx.save_for_backward(p_all, q_all, k_ff, k_fb, q_0, k_fb_0)
        ctx.mark_non_differentiable(g_max)
        ctx.set_materialize_grads(False)
        return g, g_max

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_bar, _g_max_bar):
        p_all, q_all, k_ff, k_fb, q_0, k_fb_0 = ctx.saved_tensors
        ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, c_safety = ctx.cfg
        if g_bar is None:
            return (None,) * 7
        out = rollout_constraints_vjp_batch(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_mat_obs, h_obs, h_mat_safe, h_safe, q_0, k_fb_0,
                                            c_safety, g_bar)
        ins = (p_all, q_all, k_ff, k_fb, q_0, k_fb_0)
        return (None,) + tuple(None if (x is None or o is None) else o.reshape(x.shape) for x, o in zip(ins, out))


def safety_constraints(p_all, q_all, u_0, k_fb, k_ff_all, ctrl_bounds=None, h_mat_obs=None, h_obs=None, h_mat_safe=None, h_safe=None,
                       q_0=None, k_fb_0=None, c_safety=1.0):
    """Host twin (NumPy, no device) of ``SimpleSafeMPC.generate_safety_constraints`` for ONE trajectory (safempc_simple.py:317-392),
    with the reference's argument split: p_all (H,n_s), q_all (H,n_s,n_s) or (H,n_s*n_s), u_0 (n_u) the first control, k_fb
    (H-1,n_u,n_s) or (H-1,n_u*n_s), k_ff_all (H-1,n_u) the feed-forward terms of the steps 1 .. H-1.  Returns (g, lbg, ubg, g_name)
    in the reference's own order, lbg <= g <= ubg: the u_0 rows as the reference emits them -- for a point start plain u_0 with the
    bounds u_min / u_max, with (q_0, k_fb_0) the 2 n_u ellipsoid rows with (-inf, 0) --, then the control rows of the steps
    1 .. H-1, the obstacle rows and the terminal rows, each with (-inf, 0).  g_name holds one string per row.  Behind the u_0 rows
    this is a trajectory's row of ``rollout_constraints_batch`` (k_ff = [u_0; k_ff_all]), to rounding."""
    p = np.asarray(p_all, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] < 1:
        raise ValueError("p_all must be (H, n_s)")
    H, n_s = p.shape
    q = np.asarray(q_all, dtype=np.float64).reshape(H, n_s, n_s)
    q = 0.5 * (q + q.transpose(0, 2, 1))
    if (q_0 is None) != (k_fb_0 is None):
        raise ValueError("q_0 and k_fb_0 go together")

    def dist(pc, qs, h_mat, h_vec):
        h_mat = np.asarray(h_mat, dtype=np.float64)
        return h_mat.dot(pc) + c_safety * np.sqrt(np.sum(qs.dot(h_mat.T) * h_mat.T, axis=0)) - np.asarray(h_vec, dtype=np.float64).reshape(-1)

    g, lbg, ubg, names = [], [], [], []
    if ctrl_bounds is not None:
        cb = np.asarray(ctrl_bounds, dtype=np.float64)
        n_u = cb.shape[0]
        if cb.shape != (n_u, 2) or u_0 is None:
            raise ValueError("ctrl_bounds must be (n_u, 2), with u_0 given")
        u0 = np.asarray(u_0, dtype=np.float64).reshape(n_u)
        kff = np.asarray(k_ff_all, dtype=np.float64).reshape(H - 1, n_u) if H > 1 else np.zeros((0, n_u))
        kfb = np.asarray(k_fb, dtype=np.float64).reshape(H - 1, n_u, n_s) if H > 1 else np.zeros((0, n_u, n_s))
        h_u, v_u = np.vstack((np.eye(n_u), -np.eye(n_u))), np.concatenate((cb[:, 1], -cb[:, 0]))
        if q_0 is None:
            g.append(u0)
            lbg += cb[:, 0].tolist()
            ubg += cb[:, 1].tolist()
            names += ["u_0_ctrl_constraint"] * n_u
        else:
            q0, k0 = np.asarray(q_0, dtype=np.float64).reshape(n_s, n_s), np.asarray(k_fb_0, dtype=np.float64).reshape(n_u, n_s)
            g.append(dist(u0, k0.dot(0.5 * (q0 + q0.T)).dot(k0.T), h_u, v_u))
            names += ["u_0_ctrl_constraint"] * (2 * n_u)
        for i in range(H - 1):
            g.append(dist(kff[i], kfb[i].dot(q[i]).dot(kfb[i].T), h_u, v_u))
            names += ["ellipsoid_ctrl_constraint_{}".format(i)] * (2 * n_u)
    if h_mat_obs is not None:
        for i in range(H - 1):
            g.append(dist(p[i], q[i], h_mat_obs, h_obs))
            names += ["obstacle_avoidance_constraint{}".format(i)] * np.shape(h_mat_obs)[0]
    if h_mat_safe is not None:
        g.append(dist(p[-1], q[-1], h_mat_safe, h_safe))
        names += ["terminal constraint"] * np.shape(h_mat_safe)[0]
    if not g:
        raise ValueError("no constraint rows: give ctrl_bounds, obstacles (H > 1) or a terminal set")
    g = np.concatenate(g)
    lbg += [-np.inf] * (g.size - len(lbg))
    ubg += [0.0] * (g.size - len(ubg))
    return g, lbg, ubg, names


# ------------------------------------------------------------------------------------------------
# the exploration objective: the default cost of SimpleSafeMPC.generate_cost_function (safempc_simple.py:286-315) and of
# StaticSafeMPCExploration.init_solver (safempc_exploration.py:104) over the stored GP variances of roll-outs
# ------------------------------------------------------------------------------------------------
def _explore_prepare(gp_var_all, kind, eps, p_all, mu_perf, wx_cost, n_dev, device):
    """Shapes checked (ValueError, before anything touches the device), then everything on the device: the arguments both entry
    points share, in the order of the C ABI after `device`."""
    as_t = B.is_tensor(gp_var_all)
    if kind not in ("sqrt", "sum"):
        raise ValueError("kind must be 'sqrt' or 'sum'")
    shp = tuple(np.shape(gp_var_all))
    if len(shp) != 3 or shp[1] < 1 or shp[2] < 1:
        raise ValueError("gp_var_all must be (T, H_v, n_s) with H_v >= 1")
    T, H_v, n_s = shp
    if not float(eps) >= 0.0:
        raise ValueError("eps must be >= 0")
    if (p_all is None) != (mu_perf is None):
        raise ValueError("p_all and mu_perf go together")
    H_p = H_m = 0
    if p_all is not None:
        ps, ms = tuple(np.shape(p_all)), tuple(np.shape(mu_perf))
        if len(ps) != 3 or ps[0] != T or ps[1] < 1 or ps[2] != n_s or len(ms) != 3 or ms[0] != T or ms[1] < 1 or ms[2] != n_s:
            raise ValueError("p_all must be (T, H_p, {0}) and mu_perf (T, H_m, {0})".format(n_s))
        H_p, H_m = ps[1], ms[1]
        n_dev = min(H_p, H_m) if n_dev is None else int(n_dev)
        if n_dev == 1:
            n_dev = 0                   # the deviation sum runs over 1 <= i < n_dev: empty
        if n_dev < 0 or n_dev > min(H_p, H_m):
            raise ValueError("n_dev must be within 0 .. min(H_p, H_m) = {}".format(min(H_p, H_m)))
        if n_dev >= 2 and wx_cost is None:
            raise ValueError("the deviation term needs wx_cost")
    elif n_dev:
        raise ValueError("n_dev without p_all, mu_perf")
    else:
        n_dev = 0
    if n_s > 12:
        raise NotImplementedError("exploration cost: n_s up to 12")
    w = None
    if wx_cost is not None and p_all is not None:
        w = np.asarray(B.to_numpy(wx_cost) if B.is_tensor(wx_cost) else wx_cost, dtype=np.float64)
        if w.shape != (n_s, n_s):
            raise ValueError("wx_cost must be ({0}, {0})".format(n_s))
    dev = B.resolve_device(gp_var_all.device if as_t else device)
    W = None if w is None else B.const_dev(0.1 * w, dev, (n_s, n_s))      # the reference applies 0.1 wx_cost (safempc_simple.py:300)
    v, p, m = B.as_dev(gp_var_all, dev), B.as_dev(p_all, dev), B.as_dev(mu_perf, dev)
    head = (dev.index, T, 1 if kind == "sqrt" else 0, n_s, H_v, B.ptr(v), float(eps), n_dev, H_p, B.ptr(p), H_m, B.ptr(m), B.ptr(W))
    return as_t, dev, (T, H_v, H_p, H_m, n_s), head, (v, p, m, W)


def exploration_cost_batch(gp_var_all, kind="sqrt", eps=0., p_all=None, mu_perf=None, wx_cost=None, n_dev=None, return_steps=False,
                           differentiable=False, device=None):
    """The exploration objective of T roll-outs in one launch (``sr_rollout_explore``).

    gp_var_all (T,H_v,n_s): the GP variances of a roll-out (``multistep_reachability_batch(return_gp_var=True)``, or the gp_var_all
    of the moment roll-outs).  kind "sqrt": cost[t] = -sum_i sqrt(sum_j gp_var_all[t,i,j] + eps), the default objective of the
    reference's ``SimpleSafeMPC.generate_cost_function``; "sum": -sum_i sum_j gp_var_all[t,i,j], that of
    ``StaticSafeMPCExploration``.  With p_all (T,H_p,n_s) -- the safe trajectory --, mu_perf (T,H_m,n_s) -- the performance
    trajectory -- and wx_cost (n_s,n_s): plus sum_{i=1}^{n_dev-1} d_i^T (0.1 wx_cost) d_i, d_i = mu_perf[t,i] - p_all[t,i] (n_dev
    default min(H_p, H_m); the reference's n_perf > 1 branch with n_dev = min(n_perf, n_safe); n_dev = 0 or 1: an empty sum, no
    deviation term -- the C ABI takes 0 for that and refuses 1).  Returns cost (T); with return_steps
    (cost, steps (T,H_v)): the information terms.  differentiable (tensors only): the same bits, with an autograd graph to
    gp_var_all, p_all and mu_perf whose backward is one ``exploration_cost_vjp_batch`` call (once differentiable; steps carries no
    gradient).  numpy in -> numpy out, tensors in -> tensors out."""
    if differentiable:
        if not B.is_tensor(gp_var_all):
            raise TypeError("differentiable=True needs tensors")
        out = _ExploreCostFn.apply((kind, eps, wx_cost, n_dev), gp_var_all, p_all, mu_perf)
        return out if return_steps else out[0]
    as_t, dev, (T, H_v, H_p, H_m, n_s), head, keep = _explore_prepare(gp_var_all, kind, eps, p_all, mu_perf, wx_cost, n_dev, device)
    cost = B.empty((T,), dev)
    steps = B.empty((T, H_v), dev) if return_steps else None
    check(lib.sr_rollout_explore(*head, B.ptr(cost), B.ptr(steps), B.stream_ptr(dev)))
    outs = (cost, steps) if return_steps else (cost,)
    if not as_t:
        outs = tuple(B.to_numpy(o) for o in outs)
    return outs if return_steps else outs[0]


def exploration_cost_vjp_batch(gp_var_all, kind="sqrt", eps=0., p_all=None, mu_perf=None, wx_cost=None, n_dev=None, cost_bar=None,
                               device=None):
    """Reverse pass of ``exploration_cost_batch`` in one launch (``sr_rollout_explore_vjp``): for the seed cost_bar (T; None = ones)
    the gradients of sum(cost_bar * cost): (gpvar_bar, p_bar, mu_bar), shaped like gp_var_all, p_all, mu_perf (None where the input
    is None).  gpvar_bar is the seed gpvar_all_bar of ``multistep_reachability_vjp_batch`` (or of the moment roll-outs' reverse
    pass), p_bar is added to the seed on p_all, mu_bar is the seed on the performance trajectory's means.  A radicand that is
    exactly zero contributes zero; a negative one NaN in its own row of gpvar_bar only.  n_dev = 0 or 1: no deviation term, p_bar and
    mu_bar all zero (as in ``exploration_cost_batch``)."""
    if cost_bar is not None and tuple(np.shape(cost_bar)) != tuple(np.shape(gp_var_all))[:1]:
        raise ValueError("cost_bar must be (T,)")
    as_t, dev, (T, H_v, H_p, H_m, n_s), head, keep = _explore_prepare(gp_var_all, kind, eps, p_all, mu_perf, wx_cost, n_dev, device)
    cb = B.as_dev(cost_bar, dev)
    outs = [B.empty((T, H_v, n_s), dev), B.empty((T, H_p, n_s), dev) if p_all is not None else None,
            B.empty((T, H_m, n_s), dev) if mu_perf is not None else None]
    check(lib.sr_rollout_explore_vjp(*head, B.ptr(cb), *[B.ptr(o) for o in outs], B.stream_ptr(dev)))
    return tuple(outs) if as_t else tuple(None if o is None else B.to_numpy(o) for o in outs)


class _ExploreCostFn(torch.autograd.Function):
    """``exploration_cost_batch(differentiable=True)``: the forward is the plain call, the backward one
    ``exploration_cost_vjp_batch``."""

    @staticmethod
    def forward(ctx, cfg, gp_var_all, p_all, mu_perf):
        kind, eps, wx_cost, n_dev = cfg
        cost, steps = exploration_cost_batch(gp_var_all, kind, eps, p_all, mu_perf, wx_cost, n_dev, True)
        ctx.cfg = cfg
        ctx.save_for_backward(gp_var_all, p_all, mu_perf)
        ctx.mark_non_differentiable(steps)
        ctx.set_materialize_grads(False)
        return cost, steps

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, cost_bar, _steps_bar):
        gp_var_all, p_all, mu_perf = ctx.saved_tensors
        kind, eps, wx_cost, n_dev = ctx.cfg
        if cost_bar is None:
            return (None,) * 4
        out = exploration_cost_vjp_batch(gp_var_all, kind, eps, p_all, mu_perf, wx_cost, n_dev, cost_bar)
        return (None,) + tuple(out)


def safempc_default_cost(p_all, sigma_safe, mu_perf=None, gp_pred_sigma_perf=None, wx_cost=None, n_safe=None, n_perf=None,
                         eps_noise=0.):
    """Host twin (NumPy, no device) of the default branch of ``SimpleSafeMPC.generate_cost_function`` for ONE problem
    (safempc_simple.py:286-315, no custom cost), under the reference's names: p_all (n_safe,n_s) the safe trajectory's centres,
    sigma_safe (n_safe,n_s) its GP variances (gp_sigma_pred_safe_all), mu_perf (n_perf,n_s) and gp_pred_sigma_perf (n_perf,n_s) the
    performance trajectory and its GP variances, wx_cost (n_s,n_s).  n_perf <= 1 (default: 0 without mu_perf, else its rows):
    cost = -sum_{i < n_safe} sqrt(sum_j (sigma_safe[i,j] + eps_noise)).  n_perf > 1: cost = sum_{i=1}^{min(n_perf,n_safe)-1}
    (mu_perf[i] - p_all[i]) (0.1 wx_cost) (mu_perf[i] - p_all[i])^T - sum_{i < n_perf} sqrt(sum_j (gp_pred_sigma_perf[i,j] +
    eps_noise)).  The reference adds eps_noise to every element before it sums: on the device this is
    ``exploration_cost_batch(..., eps=n_s * eps_noise)``.  Returns a float."""
    p_all = np.asarray(p_all, dtype=np.float64)
    sigma_safe = np.asarray(sigma_safe, dtype=np.float64)
    n_safe = sigma_safe.shape[0] if n_safe is None else int(n_safe)
    if n_perf is None:
        n_perf = 0 if mu_perf is None else np.shape(mu_perf)[0]
    cost = 0.0
    if n_perf > 1:
        if mu_perf is None or gp_pred_sigma_perf is None or wx_cost is None:
            raise ValueError("n_perf > 1 needs mu_perf, gp_pred_sigma_perf and wx_cost")
        mu_perf = np.asarray(mu_perf, dtype=np.float64)
        sig = np.asarray(gp_pred_sigma_perf, dtype=np.float64)
        w = 0.1 * np.asarray(wx_cost, dtype=np.float64)
        for i in range(1, min(n_perf, n_safe)):
            d = (mu_perf[i] - p_all[i]).reshape(1, -1)
            cost += float(d.dot(w).dot(d.T)[0, 0])
        for i in range(n_perf):
            cost -= float(np.sqrt(np.sum(sig[i] + eps_noise)))
    else:
        for i in range(n_safe):
            cost -= float(np.sqrt(np.sum(sigma_safe[i] + eps_noise)))
    return cost


# ------------------------------------------------------------------------------------------------
# closed-loop roll-outs of the TRUE system against the predicted ellipsoids (gp_reachability.py:253-356).
# `env` is the caller's environment object (duck-typed: ``simulate_onestep(state, action) -> (state, ...)``,
# attributes n_s / n_u); these are host-side bookkeeping around the batched containment kernels.
# ------------------------------------------------------------------------------------------------
def simulate_trajectory(env, p_0, k_fb, k_ff, p_ctrl):
    """Roll the environment forward under u_0 = k_ff[0], u_i = k_fb[i-1] (x_i - p_ctrl[i-1]) + k_ff[i]
    (gp_reachability.py:253-283).  k_ff (n, n_u); k_fb (n-1, n_u*n_s); p_ctrl (n-1, n_s) -> x_all (n+1, n_s)."""
    from .utils import feedback_ctrl
    k_ff = np.asarray(k_ff, dtype=np.float64)
    n, n_u = k_ff.shape
    x = np.asarray(p_0, dtype=np.float64).reshape(-1)
    n_s = x.size
    x_all = np.empty((n + 1, n_s))
    x_all[0] = x
    for i in range(n):
        if i == 0:
            action = k_ff[0]
        else:
            action = feedback_ctrl(x[:, None], k_ff[i, :, None], np.reshape(k_fb[i - 1], (n_u, n_s)),
                                   np.asarray(p_ctrl[i - 1], dtype=np.float64)[:, None])
        x = np.asarray(env.simulate_onestep(x, action)[0], dtype=np.float64).reshape(-1)
        x_all[i + 1] = x
    return x_all


def verify_trajectory_safety(env, p_0, k_fb, k_ff, p_ctrl, h_mat_safe, h_safe, h_mat_obs=None, h_obs=None):
    """True trajectory inside the obstacle-free polytope at steps 1..n-1 and inside the terminal safe polytope at
    the last step (gp_reachability.py:286-320).  Returns (bool, x_all)."""
    from .utils import sample_inside_polytope
    n = np.shape(k_ff)[0]
    x_all = simulate_trajectory(env, p_0, k_fb, k_ff, p_ctrl)
    inside = True
    if h_mat_obs is not None and n > 1:
        inside = bool(np.all(sample_inside_polytope(x_all[1:n], h_mat_obs, h_obs)))
    inside = inside and bool(np.all(sample_inside_polytope(x_all[None, -1, :], h_mat_safe, h_safe)))
    return inside, x_all


def trajectory_inside_ellipsoid(env, p_0, p_all, q_all, k_fb, k_ff):
    """Is the true state at step i inside the predicted ellipsoid (p_all[i], q_all[i])?  (gp_reachability.py:323-356)
    p_all (n, n_s); q_all (n, n_s*n_s) -> bool (n,)."""
    n = np.shape(k_ff)[0]
    n_s = env.n_s
    x_all = simulate_trajectory(env, p_0, k_fb, k_ff, p_all)[1:]
    centred = x_all - np.asarray(p_all, dtype=np.float64).reshape(n, n_s)
    q_all = np.asarray(q_all, dtype=np.float64).reshape(n, n_s, n_s)
    return np.einsum('ij,ij->i', centred, np.linalg.solve(q_all, centred[:, :, None])[:, :, 0]) < 1.0
