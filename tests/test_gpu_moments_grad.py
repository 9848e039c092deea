"""The reverse pass of one Taylor / mean-equivalent moment step on the device (sr_moment_step_vjp, sr_onestep_moments_vjp), the
one-step forward from a Gaussian state (sr_onestep_moments) and the autograd surface over them, against the long-double reference
tests/_moments_grad_ref.py.

1. sr_moment_step_vjp at all 32 (n_s, n_u) instances x modes 1, 2 x both starts x every family of _ellipsoid_ref.cases (all ten
   are value families: nothing passes through an eigenvalue), T = 257, into sentinel-filled outputs.  Bars (stated once in
   _moments_grad_ref): per output array 30 x SHARE x EPS x abs-scale, SHARE the measured floor of a plain fp64 restatement
   (mux_bar 1.4, sigma_bar 2.2, kff_bar 1.0, kfb_bar 1.6, jac_bar 2.3; mug_bar and var_bar 0: equal bits).  sigma_bar is bitwise
   symmetric; a NULL seed gives the bits of a zero seed, an unsymmetric sigma1_bar the bits of its symmetric part; in mode 2
   jac_bar is exactly zero and jac_g = NULL is accepted; at a point start the optional outputs are zero-filled where given;
   SR_EINVAL and SR_EUNSUPPORTED as include/safereach.h states them.
2. sr_onestep_moments / sr_onestep_moments_vjp on fitted models -- (n_out, D) = (2, 3) rbf at N = 150 and 600, (4, 5) rbf, (2, 3)
   lin_mat52, the cart-pole shape with an input transform (3 x 4, D = 4), one sparse handle; modes 1 and 2, both starts, with and
   without gpvar_bar.  The forward against _ellipsoid_ref.step on the device's own predict outputs at z with the forward bars of
   _ellipsoid_ref (p1_atol, q1_atol, RTOL); the reverse against the long-double reference composed with the device's OWN
   linearize_device_batch outputs at z, so that only the new kernels' rounding is under test (the composed mux_bar and kff_bar
   are held to 30 x the largest link share, jac_bar's 2.3).  Same bits with set_chunk(64), and with chunks of 64 / 1000 / the
   default at N = 2000, T = 1500; NotImplementedError at D = 9.
3. The autograd surface: differentiable=True returns the bits of the plain call (moment_step_batch, onestep_moments_batch),
   torch.autograd.grad equals the wrapper's VJP to the bit.  The values of multistep_moments_batch(differentiable=True), H = 3, 33
   trajectories from a point, equal sr_multistep_moments with set_chain(False) TO THE BIT: sr_onestep_moments issues the launches
   of one step of that per-step route (transformed states, posterior with its Jacobian, the moment step).  The gradient of a
   random linear functional of (mu_all, sigma_all, gp_var_all) in mu_0, k_ff, k_fb (and sigma_0) equals the step-by-step
   reverse sweep of the reference on the device's own per-step linearisations; its bar is relative to the largest element of each
   gradient: PROP_RTOL = 30 x the disagreement of two CPU routes to that gradient (the sweep in long double and in fp64).
4. examples/cautious_shooting_gradient.py runs and its loss goes down.

Observed on MI355X, as shares of the bars: sr_moment_step_vjp mux_bar 0.052, sigma_bar 0.047 (7x4), kff_bar 0.063 (8x4), kfb_bar 0.051
(1x3), jac_bar 0.038, mug_bar and var_bar exact; sr_onestep_moments at most 0.032 (mu, the (4, 5) model) and 0.008 (sigma);
sr_onestep_moments_vjp at most 0.032 (kff_bar with the input transform, kfb_bar on the sparse handle); propagated gradients: device
1.5e-16 .. 6.0e-16 of the largest element, the two CPU routes 8.4e-17 .. 4.96e-16 (d/dsigma_0, mode 1), bar 1.5e-14.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ellipsoid_ref as R
import _moments_grad_ref as M
from _helpers import width_problem, width_gp

pytestmark = pytest.mark.gpu
LD = np.longdouble
T = R.T_CASE
SENTINEL = -7.25e+300
INSTANCES = [(n_s, n_u) for n_s in range(1, 9) for n_u in range(1, 5)]
LINK_SHARE = max(M.SHARE[k] for k in ("mux_bar", "kff_bar", "mug_bar", "var_bar", "jac_bar"))
PROP_RTOL = 30 * 5.0e-16          # two CPU routes (long double / fp64 sweep) disagree by at most 4.96e-16 of the largest element
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = dict(mux_bar=lambda T_, s, u: (T_, s), sigma_bar=lambda T_, s, u: (T_, s, s), kff_bar=lambda T_, s, u: (T_, u),
              kfb_bar=lambda T_, s, u: (T_, u, s), mug_bar=lambda T_, s, u: (T_, s), var_bar=lambda T_, s, u: (T_, s),
              jac_bar=lambda T_, s, u: (T_, s, s + u))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(x):
    import torch
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device=_dev())


def _step_vjp_raw(case, start, mode, mb, sb, lin=True, jac=True, give=M.OUTPUTS, n_s=None, n_u=None, T_=None):
    """sr_moment_step_vjp through the C ABI into sentinel-filled outputs: (status, dict name -> array); outputs not in `give` are
    passed as NULL and keep their sentinels"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    Tn, ns = case["p"].shape
    nu = case["k_ff"].shape[1]
    gauss = start == "gauss"
    a = case["a"] if lin else np.eye(ns)
    b = case["b"] if lin else np.zeros((ns, nu))
    ins = [_t(case["p"]), _t(case["q"]) if gauss else None, _t(case["k_ff"]), _t(case["k_fb"]) if gauss else None, _t(case["mu"]),
           _t(case["var"]), _t(case["jac"]) if (gauss and jac) else None, _t(a), _t(b)]
    outs = {k: torch.full(SHAPES[k](Tn, ns, nu), SENTINEL, dtype=torch.float64, device=_dev()) for k in M.OUTPUTS}
    tmb, tsb = _t(mb), _t(sb)                             # (held until the copies below have synchronised)
    rc = lib.sr_moment_step_vjp(0, Tn if T_ is None else T_, ns if n_s is None else n_s, nu if n_u is None else n_u, mode,
                                *[B.ptr(x) for x in ins], B.ptr(tmb), B.ptr(tsb),
                                *[B.ptr(outs[k]) if k in give else None for k in M.OUTPUTS], B.stream_ptr(_dev()))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in outs.items()}


def _step_vjp_device(case, start, mode, mb, sb, **kw):
    rc, outs = _step_vjp_raw(case, start, mode, mb, sb, **kw)
    assert rc == 0, rc
    return outs


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: "%dx%d" % i)
def test_moment_step_vjp_against_the_long_double_reference(inst):
    cases = R.cases(*inst)
    failures, top = [], {k: 0.0 for k in M.OUTPUTS}
    for fam in R.families(inst[0]):
        case = cases[fam]
        mb, sb, _ = M.seeds(case)
        for mode in M.MODES:
            for start in M.STARTS:
                got = _step_vjp_device(case, start, mode, mb, sb)
                ref = M.vjp_batch(case, start, mode, mb, sb)
                for name in M.OUTPUTS:
                    assert np.isfinite(got[name]).all() and not (got[name] == SENTINEL).any(), (fam, mode, start, name)
                assert np.array_equal(got["sigma_bar"], got["sigma_bar"].transpose(0, 2, 1)), (fam, mode, start)
                if start == "point":
                    assert not got["sigma_bar"].any() and not got["kfb_bar"].any() and not got["jac_bar"].any()
                if mode == 2:
                    assert not got["jac_bar"].any(), (fam, start)
                for name in M.OUTPUTS:
                    v = M.within_bar(got[name], ref[name], ref[name + "_abs"], name)
                    top[name] = max(top[name], v)
                    if not v <= 1.0:
                        failures.append((fam, mode, start, name, v))
    print("%dx%d: share of the bar used %s" % (inst + ({k: "%.3f" % v for k, v in top.items()},)))
    assert not failures, failures


def test_conventions_on_the_device():
    """NULL seed = zero seed to the bit; an unsymmetric sigma1_bar gives the bits of its symmetric part; a = b = None; mode 2 takes
    jac_g = NULL and gives the bits it gives with one; the optional outputs of a point start; the wrapper gives the C ABI's bits"""
    inst = (3, 2)
    case = R.cases(*inst)["rounded"]
    mb, sb, _ = M.seeds(case)
    for mode in M.MODES:
        for start in M.STARTS:
            full = _step_vjp_device(case, start, mode, mb, sb)
            for null, zero in (((None, sb), (np.zeros_like(mb), sb)), ((mb, None), (mb, np.zeros_like(sb)))):
                x, y = _step_vjp_device(case, start, mode, *null), _step_vjp_device(case, start, mode, *zero)
                assert all(np.array_equal(x[k], y[k]) for k in M.OUTPUTS), (mode, start)
            sym = _step_vjp_device(case, start, mode, mb, (sb + sb.transpose(0, 2, 1)) / 2)
            assert all(np.array_equal(sym[k], full[k]) for k in M.OUTPUTS), (mode, start)
            nolin = _step_vjp_device(case, start, mode, mb, sb, lin=False)
            ref0 = M.vjp_batch(case, start, mode, mb, sb, lin=False)
            worst = {k: M.within_bar(nolin[k], ref0[k], ref0[k + "_abs"], k) for k in M.OUTPUTS}
            assert all(v <= 1.0 for v in worst.values()), (mode, start, worst)
        nojac = _step_vjp_device(case, "gauss", mode, mb, sb, jac=False) if mode == 2 else None
        if nojac is not None:
            with_jac = _step_vjp_device(case, "gauss", mode, mb, sb)
            assert all(np.array_equal(nojac[k], with_jac[k]) for k in M.OUTPUTS)
        # a point start: the three optional outputs may be NULL; those given are zero-filled, the rest of the call is the same
        full = _step_vjp_device(case, "point", mode, mb, sb)
        part = _step_vjp_device(case, "point", mode, mb, sb, give=("mux_bar", "kff_bar", "mug_bar", "var_bar", "jac_bar"))
        assert not part["jac_bar"].any() and (part["sigma_bar"] == SENTINEL).all() and (part["kfb_bar"] == SENTINEL).all()
        none = _step_vjp_device(case, "point", mode, mb, sb, give=("mux_bar", "kff_bar", "mug_bar", "var_bar"))
        assert all((none[k] == SENTINEL).all() for k in ("sigma_bar", "kfb_bar", "jac_bar"))
        for k in ("mux_bar", "kff_bar", "mug_bar", "var_bar"):
            assert np.array_equal(part[k], full[k]) and np.array_equal(none[k], full[k])
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    outs = U.moment_step_vjp_batch(case["p"], case["k_ff"], case["mu"], case["var"], case["jac"], mb, sb, case["q"], case["k_fb"],
                                   case["a"], case["b"], mode=1)
    full = _step_vjp_device(case, "gauss", 1, mb, sb)
    assert all(isinstance(o, np.ndarray) and np.array_equal(o, full[k]) for o, k in zip(outs, M.OUTPUTS))
    outs = U.moment_step_vjp_batch(case["p"], case["k_ff"], case["mu"], case["var"], None, mb, sb, a=case["a"], b=case["b"], mode=2)
    assert outs[1] is None and outs[3] is None and outs[6] is None


def test_moment_step_vjp_refusals():
    from safe_exploration_amd._lib import SR_EINVAL, SR_EUNSUPPORTED
    case = R.cases(3, 2)["random"]
    mb, sb, _ = M.seeds(case)
    small = {k: (v[:4] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == T else v) for k, v in case.items()}
    mb, sb = mb[:4], sb[:4]
    rc = lambda *a, **kw: _step_vjp_raw(small, *a, **kw)[0]
    assert rc("gauss", 1, mb, sb) == 0
    assert rc("gauss", 0, mb, sb) == SR_EINVAL and rc("gauss", 3, mb, sb) == SR_EINVAL              # mode outside {1, 2}
    assert rc("gauss", 1, None, None) == SR_EINVAL and rc("point", 2, None, None) == SR_EINVAL     # both seeds NULL
    assert rc("gauss", 1, mb, sb, jac=False) == SR_EINVAL                                          # Taylor mode without jac_g
    for missing in ("sigma_bar", "kfb_bar", "jac_bar"):                                            # required with sigma_x
        assert rc("gauss", 2, mb, sb, give=tuple(k for k in M.OUTPUTS if k != missing)) == SR_EINVAL
    for missing in ("mux_bar", "kff_bar", "mug_bar", "var_bar"):                                   # required always
        assert rc("point", 1, mb, sb, give=tuple(k for k in M.OUTPUTS if k != missing)) == SR_EINVAL
    assert rc("gauss", 1, mb, sb, T_=-1) == SR_EINVAL
    assert rc("gauss", 1, None, None, T_=0) == 0                                                   # T = 0: a no-op
    # (the sizes are checked before anything is launched: the arrays of the 3 x 2 case are never read)
    assert rc("point", 1, mb, sb, n_s=9) == SR_EUNSUPPORTED and rc("point", 1, mb, sb, n_u=5) == SR_EUNSUPPORTED


# ---- 2. sr_onestep_moments / sr_onestep_moments_vjp on fitted models -----------------------------------------------------------
def _gp_model(spec):
    kind, kt, n_out, D, N = spec
    if kind == "sparse":
        import _sparse_ref as S
        from test_gpu_sparse_gp import _sparse_model
        return _sparse_model(S.make_case(5, kt, n_out, D, 96, N))
    return width_gp(width_problem(4000 + N + D, kt, D, N, n_out))


MODELS = [("exact", "rbf", 2, 3, 150), ("exact", "rbf", 2, 3, 600), ("exact", "rbf", 4, 5, 150), ("exact", "lin_mat52", 2, 3, 150),
          ("cartpole", "rbf", 4, 4, 150), ("sparse", "rbf", 2, 3, 3000)]


def _inputs(n_s, n_u, Tn, seed):
    rng = np.random.default_rng([seed, n_s, n_u, Tn])
    A = rng.standard_normal((Tn, n_s, n_s))
    return dict(p=0.3 * rng.standard_normal((Tn, n_s)), k_ff=0.2 * rng.standard_normal((Tn, n_u)),
                q=0.02 * np.einsum('tij,tkj->tik', A, A) / n_s, k_fb=0.3 * rng.standard_normal((Tn, n_u, n_s)),
                a=0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
                mb=rng.standard_normal((Tn, n_s)), sb=rng.standard_normal((Tn, n_s, n_s)), vb=rng.standard_normal((Tn, n_s)))


def _composed_reference(x, lin, tz, start, mode, mb, sb, vb, fp64=False):
    """_moments_grad_ref.step_vjp composed with linearisations (mu, var, jac_mu, jac_var, hess_mu at z = [tz mu_x; k_ff]) that the
    caller supplies: mux_bar, sigma_bar, kff_bar, kfb_bar with their abs-scales, per query, in long double (fp64: the restatement)"""
    dt = np.float64 if fp64 else LD
    mu, var, jm, jv, hm = lin
    Tn, n_s = x["p"].shape
    tzm = np.eye(n_s, dtype=dt) if tz is None else np.asarray(tz, dtype=dt)
    nx = tzm.shape[0]
    names = ("mux_bar", "sigma_bar", "kff_bar", "kfb_bar")
    res = {k: [] for k in names + tuple(n + "_abs" for n in names)}
    pick = lambda s, t: None if s is None else s[t]
    for t in range(Tn):
        jmt, jvt, hmt = jm[t].astype(dt), jv[t].astype(dt), hm[t].astype(dt)
        jac_s = np.hstack((jmt[:, :nx].dot(tzm), jmt[:, nx:]))
        o = M.step_vjp(x["p"][t], x["q"][t] if start == "gauss" else None, x["k_ff"][t], x["k_fb"][t], mu[t], var[t], jac_s,
                       x["a"], x["b"], mode, pick(mb, t), pick(sb, t), pick(vb, t), fp64=fp64)
        jz = np.hstack((o["jac_bar"][:, :n_s].dot(tzm.T), o["jac_bar"][:, n_s:]))
        jz_abs = np.hstack((o["jac_bar_abs"][:, :n_s].dot(np.abs(tzm).T), o["jac_bar_abs"][:, n_s:]))
        zb = jmt.T.dot(o["mug_bar"]) + jvt.T.dot(o["var_bar"]) + np.einsum('ad,ade->e', jz, hmt)
        zb_abs = np.abs(jmt).T.dot(o["mug_bar_abs"]) + np.abs(jvt).T.dot(o["var_bar_abs"]) + np.einsum('ad,ade->e', jz_abs, np.abs(hmt))
        res["mux_bar"].append(o["mux_bar"] + tzm.T.dot(zb[:nx]))
        res["mux_bar_abs"].append(o["mux_bar_abs"] + np.abs(tzm).T.dot(zb_abs[:nx]))
        res["kff_bar"].append(o["kff_bar"] + zb[nx:])
        res["kff_bar_abs"].append(o["kff_bar_abs"] + zb_abs[nx:])
        for k in ("sigma_bar", "kfb_bar", "sigma_bar_abs", "kfb_bar_abs"):
            res[k].append(o[k])
    return {k: np.array(v).astype(np.float64) for k, v in res.items()}


def _z(p, k_ff, tz):
    return np.hstack((p if tz is None else p.dot(np.asarray(tz).T), k_ff))


def _spec_dims(spec):
    tz = np.eye(4)[1:] if spec[0] == "cartpole" else None          # the cart position is not a GP input (exact in fp64)
    return spec[2], spec[3] - (3 if tz is not None else spec[2]), tz


@pytest.mark.parametrize("spec", MODELS, ids=lambda s: "%s-%s-%dx%d-N%d" % s)
def test_onestep_moments_and_their_vjp_on_fitted_models(spec):
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    gp = _gp_model(spec)
    n_s, n_u, tz = _spec_dims(spec)
    x = _inputs(n_s, n_u, T, 11)
    z = _z(x["p"], x["k_ff"], tz)
    lin = tuple(o.cpu().numpy() for o in gp.linearize_device_batch(z))
    pmu, pvar, pjac = (o.cpu().numpy() for o in gp.predict_device(_t(z), compute_gradients=True))
    nx = n_s if tz is None else tz.shape[0]
    pjac_s = pjac if tz is None else np.concatenate((pjac[:, :, :nx].dot(tz), pjac[:, :, nx:]), axis=2)
    fcase = dict(x, mu=pmu, var=pvar, jac=pjac_s, l_mu=None, l_sigma=None, c=1.0)
    worst_f, worst_r = {}, {}
    for mode in M.MODES:
        for start in M.STARTS:
            gauss = start == "gauss"
            kw = dict(sigma_x=x["q"] if gauss else None, k_fb=x["k_fb"] if gauss else None, a=x["a"], b=x["b"], mode=mode,
                      a_gp_inp_x=tz)
            # forward
            mu1, sig1, gvar = U.onestep_moments_batch(x["p"], gp, x["k_ff"], **kw)
            want = R.step_batch(fcase, "ell" if gauss else "point", mode)
            assert R.used(gvar, pvar, R.RTOL) <= 1.0
            worst_f[(mode, start)] = (R.used(mu1, want["p1"], R.RTOL, R.p1_atol(want["p1_abs"])),
                                      R.used(sig1, want["q1"], R.RTOL, R.q1_atol(n_s, want["q1_abs"])))
            # reverse, with and without the seed on the GP variances
            for vb in (x["vb"], None):
                call = lambda: U.onestep_moments_vjp_batch(x["p"], gp, x["k_ff"], x["mb"], x["sb"], vb, **kw)
                got = call()
                ref = _composed_reference(x, lin, tz, start, mode, x["mb"], x["sb"], vb)
                if not gauss:
                    assert got[1] is None and got[3] is None
                for name, arr in zip(("mux_bar", "sigma_bar", "kff_bar", "kfb_bar"), got):
                    if arr is None:
                        continue
                    assert np.isfinite(arr).all(), name
                    share = LINK_SHARE if name in ("mux_bar", "kff_bar") else M.SHARE[name]
                    v = M.share_used(arr, ref[name], ref[name + "_abs"]) / (M.FACTOR * share)
                    worst_r[name] = max(worst_r.get(name, 0.0), v)
                if gauss:
                    assert np.array_equal(got[1], got[1].transpose(0, 2, 1))
                gp.set_chunk(64)
                try:
                    chunked = call()
                finally:
                    gp.set_chunk(65536)
                assert all(u is v or np.array_equal(u, v) for u, v in zip(got, chunked)), "chunking changed the bits"
    print("%s forward: share of the bars used (mu, sigma) %s" % (spec, {k: "%.3f/%.3f" % v for k, v in worst_f.items()}))
    print("%s reverse: share of the bar used %s" % (spec, {k: "%.3f" % v for k, v in worst_r.items()}))
    assert all(max(v) <= 1.0 for v in worst_f.values()), worst_f
    assert all(v <= 1.0 for v in worst_r.values()), worst_r


def test_onestep_moments_vjp_chunks_at_a_size_where_the_passes_matter():
    """N = 2000, n_out = 2, T = 1500: the GP derivative calls split their sums by the width of the batch they are given -- other
    bits on 1500 queries at once than on 64.  sr_onestep_moments_vjp bounds its passes as sr_onestep_reach_vjp does, so every
    chunk size gives the same bits, in the case that runs sr_gp_linearize_batch and in those that run sr_gp_predict_grad."""
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    gp = width_gp(width_problem(4242, "rbf", 3, 2000, 2))
    Tn = 1500
    x = _inputs(2, 1, Tn, 17)
    for mode, gauss in ((1, True), (2, True), (1, False)):
        call = lambda: U.onestep_moments_vjp_batch(x["p"], gp, x["k_ff"], x["mb"], x["sb"], x["vb"], x["q"] if gauss else None,
                                                   x["k_fb"] if gauss else None, x["a"], x["b"], mode)
        whole = call()
        assert all(o is None or np.isfinite(o).all() for o in whole)
        try:
            for chunk in (64, 1000):
                gp.set_chunk(chunk)
                parts = call()
                assert all(u is v or np.array_equal(u, v) for u, v in zip(whole, parts)), "chunk %d changed the bits" % chunk
        finally:
            gp.set_chunk(65536)


def test_onestep_moments_refusals():
    from safe_exploration_amd import uncertainty_propagation_casadi as U, _buffers as B
    from safe_exploration_amd._lib import lib, SR_EINVAL
    gp9 = width_gp(width_problem(77, "rbf", 9, 60, 8))           # n_s = 8, n_u = 1, D = 9
    x = _inputs(8, 1, 4, 3)
    with pytest.raises(NotImplementedError):
        U.onestep_moments_vjp_batch(x["p"], gp9, x["k_ff"], x["mb"], None, None, mode=2)
    gp = _gp_model(MODELS[0])
    hd, s = gp._handle, B.stream_ptr(gp._handle.device)
    x = _inputs(2, 1, 4, 3)
    d = {k: _t(v) for k, v in x.items()}
    o = [B.empty((4, 2), hd.device), B.empty((4, 2, 2), hd.device), B.empty((4, 1), hd.device), B.empty((4, 1, 2), hd.device)]
    P = B.ptr
    args = lambda mode, q, kfb, mb, sb, vb, T_=4: (hd.h, T_, mode, P(d["p"]), q, P(d["k_ff"]), kfb, P(d["a"]), P(d["b"]), mb, sb, vb,
                                                   P(o[0]), P(o[1]), P(o[2]), P(o[3]), s)
    assert lib.sr_onestep_moments_vjp(*args(1, P(d["q"]), P(d["k_fb"]), P(d["mb"]), P(d["sb"]), None)) == 0
    assert lib.sr_onestep_moments_vjp(*args(1, P(d["q"]), None, P(d["mb"]), P(d["sb"]), None)) == SR_EINVAL     # sigma_x without k_fb
    assert lib.sr_onestep_moments_vjp(*args(1, P(d["q"]), P(d["k_fb"]), None, None, None)) == SR_EINVAL         # every seed NULL
    assert lib.sr_onestep_moments_vjp(*args(3, P(d["q"]), P(d["k_fb"]), P(d["mb"]), None, None)) == SR_EINVAL   # mode
    assert lib.sr_onestep_moments_vjp(*args(2, None, None, None, None, P(d["vb"]))) == 0                        # gpvar_bar alone
    assert lib.sr_onestep_moments_vjp(*args(1, None, None, None, None, None, T_=0)) == 0                        # T = 0: a no-op
    fwd = lambda mode, q, kfb, T_=4: lib.sr_onestep_moments(hd.h, T_, mode, P(d["p"]), q, P(d["k_ff"]), kfb, P(d["a"]), P(d["b"]),
                                                            P(o[0]), P(o[1]), None, s)
    assert fwd(1, P(d["q"]), P(d["k_fb"])) == 0 and fwd(0, None, None) == SR_EINVAL and fwd(2, P(d["q"]), None) == SR_EINVAL
    assert fwd(1, None, None, T_=0) == 0
    with pytest.raises(ValueError):
        U.onestep_moments_batch(x["p"], gp, x["k_ff"], sigma_x=x["q"])
    import torch
    torch.cuda.synchronize()


# ---- 3. the autograd surface --------------------------------------------------------------------------------------------------
def test_differentiable_steps_are_the_plain_calls_and_their_vjps():
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    for spec in (MODELS[0], MODELS[4]):
        gp = _gp_model(spec)
        n_s, n_u, tz = _spec_dims(spec)
        x = _inputs(n_s, n_u, 33, 5)
        for mode in M.MODES:
            for gauss in (True, False):
                ins = [_t(x["p"]).requires_grad_(True), _t(x["q"]).requires_grad_(True) if gauss else None,
                       _t(x["k_ff"]).requires_grad_(True), _t(x["k_fb"]).requires_grad_(True) if gauss else None]
                det = [None if v is None else v.detach() for v in ins]
                kw = dict(a=x["a"], b=x["b"], mode=mode, a_gp_inp_x=tz)
                plain = U.onestep_moments_batch(det[0], gp, det[2], det[1], det[3], **kw)
                diff = U.onestep_moments_batch(ins[0], gp, ins[2], ins[1], ins[3], differentiable=True, **kw)
                assert all(torch.equal(u, v) for u, v in zip(plain, diff))
                assert all(o.requires_grad for o in diff)
                mb, sb, vb = _t(x["mb"]), _t(x["sb"]), _t(x["vb"])
                grads = torch.autograd.grad((diff[0] * mb).sum() + (diff[1] * sb).sum() + (diff[2] * vb).sum(),
                                            [v for v in ins if v is not None])
                vjp = U.onestep_moments_vjp_batch(det[0], gp, det[2], mb, sb, vb, det[1], det[3], **kw)
                assert all(torch.equal(u, v) for u, v in zip(grads, [v for v in vjp if v is not None]))
    # moment_step_batch(differentiable=True): gradients also reach mu_g, var_g, jac_g
    case = R.cases(3, 2)["random"]
    mb, sb, _ = M.seeds(case)
    for mode in M.MODES:
        ts = {k: _t(case[k]).requires_grad_(True) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
        kw = dict(a=case["a"], b=case["b"], mode=mode)
        plain = U.moment_step_batch(*[ts[k].detach() for k in ("p", "k_ff", "mu", "var", "jac")], ts["q"].detach(),
                                    ts["k_fb"].detach(), **kw)
        diff = U.moment_step_batch(*[ts[k] for k in ("p", "k_ff", "mu", "var", "jac")], ts["q"], ts["k_fb"], differentiable=True, **kw)
        assert all(torch.equal(u, v) for u, v in zip(plain, diff))
        order = ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")
        grads = torch.autograd.grad((diff[0] * _t(mb)).sum() + (diff[1] * _t(sb)).sum(), [ts[k] for k in order])
        full = _step_vjp_device(case, "gauss", mode, mb, sb)
        assert all(np.array_equal(g.cpu().numpy(), full[k]) for g, k in zip(grads, M.OUTPUTS))


def _sweep_reference(x, H, lins, states, mode, w_mu, w_sig, w_var, k_ff, k_fb, k_fb_0, fp64):
    """reverse sweep over H steps: the gradient of sum w_mu . mu_all + w_sig . sigma_all + w_var . gp_var_all in mu_0, sigma_0,
    k_ff and k_fb (step 0 from sigma_0 runs with the gain k_fb_0, zero), from the reference VJP of every step at the device's own states and linearisations"""
    Tn, n_s = x["p"].shape
    n_u = k_ff.shape[2]
    dt = np.float64 if fp64 else LD
    mu_bar, sig_bar = np.zeros((Tn, n_s), dtype=dt), np.zeros((Tn, n_s, n_s), dtype=dt)
    g_kff, g_kfb = np.zeros((Tn, H, n_u), dtype=dt), np.zeros((Tn, max(H - 1, 0), n_u, n_s), dtype=dt)
    for i in range(H - 1, -1, -1):
        mu_in, sig_in = states[i]
        gauss = sig_in is not None
        kfb_i = k_fb_0 if i == 0 else k_fb[:, i - 1]
        xi = dict(x, p=mu_in, q=sig_in, k_ff=k_ff[:, i], k_fb=kfb_i if gauss else np.zeros((Tn, n_u, n_s)))
        out = _composed_reference(xi, lins[i], None, "gauss" if gauss else "point", mode, mu_bar + w_mu[:, i], sig_bar + w_sig[:, i],
                                  w_var[:, i], fp64=fp64)
        # (the composed reference rounds its results to fp64; at 30 x the floor that is invisible)
        mu_bar, g_kff[:, i] = out["mux_bar"], out["kff_bar"]
        if gauss:
            sig_bar = out["sigma_bar"]
            if i > 0:
                g_kfb[:, i - 1] = out["kfb_bar"]
    return dict(mu_0=mu_bar.astype(np.float64), sigma_0=sig_bar.astype(np.float64), k_ff=g_kff.astype(np.float64),
                k_fb=g_kfb.astype(np.float64))


@pytest.mark.parametrize("mode", M.MODES, ids=("taylor", "mean_equivalent"))
@pytest.mark.parametrize("with_sigma_0", (False, True), ids=("from_a_point", "from_sigma_0"))
def test_differentiable_multistep(with_sigma_0, mode):
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    gp = _gp_model(MODELS[2])
    n_s, n_u, Tn, H = 4, 1, 33, 3
    x = _inputs(n_s, n_u, Tn, 21)
    rng = np.random.default_rng(8)
    k_ff, k_fb = 0.2 * rng.standard_normal((Tn, H, n_u)), 0.3 * rng.standard_normal((Tn, H - 1, n_u, n_s))
    w_mu, w_sig, w_var = rng.standard_normal((Tn, H, n_s)), rng.standard_normal((Tn, H, n_s, n_s)), rng.standard_normal((Tn, H, n_s))
    leaves = dict(mu_0=_t(x["p"]).requires_grad_(True), k_ff=_t(k_ff).requires_grad_(True), k_fb=_t(k_fb).requires_grad_(True))
    if with_sigma_0:
        leaves.update(sigma_0=_t(x["q"]).requires_grad_(True))
    mu_all, sig_all, var_all = U.multistep_moments_batch(leaves["mu_0"], gp, leaves["k_ff"], leaves["k_fb"], x["a"], x["b"], mode,
                                                         differentiable=True, sigma_0=leaves.get("sigma_0"))
    if not with_sigma_0:
        gp.set_chain(False)
        try:
            fwd = U.multistep_moments_batch(leaves["mu_0"].detach(), gp, leaves["k_ff"].detach(), leaves["k_fb"].detach(), x["a"],
                                            x["b"], mode)
        finally:
            gp.set_chain(True)
        assert all(torch.equal(u, v) for u, v in zip((mu_all, sig_all, var_all), fwd)), "values differ from the per-step route"
    names = list(leaves)
    grads = dict(zip(names, torch.autograd.grad((mu_all * _t(w_mu)).sum() + (sig_all * _t(w_sig)).sum() + (var_all * _t(w_var)).sum(),
                                                [leaves[k] for k in names])))
    ma, sa = mu_all.detach().cpu().numpy(), sig_all.detach().cpu().numpy()
    states = [(x["p"], x["q"] if with_sigma_0 else None)] + [(ma[:, i], sa[:, i]) for i in range(H - 1)]
    lins = [tuple(o.cpu().numpy() for o in gp.linearize_device_batch(np.hstack((states[i][0], k_ff[:, i])))) for i in range(H)]
    sweep = lambda fp64: _sweep_reference(x, H, lins, states, mode, w_mu, w_sig, w_var, k_ff, k_fb, np.zeros_like(x["k_fb"]), fp64)
    ref, alt = sweep(False), sweep(True)
    for name in names:
        got = grads[name].cpu().numpy()
        scale = np.abs(ref[name]).max()
        err, floor = np.abs(got - ref[name]).max() / scale, np.abs(alt[name] - ref[name]).max() / scale
        print("multistep mode %d sigma_0=%s d/d%s: device %.2e, two CPU routes %.2e of the largest element (bar %.1e)"
              % (mode, with_sigma_0, name, err, floor, PROP_RTOL))
        assert np.isfinite(got).all() and err <= PROP_RTOL, (name, err)


# ---- 4. the example ------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_its_loss_goes_down():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cautious_shooting_gradient.py")], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    losses = [float(line.split()[-1]) for line in res.stdout.splitlines() if line.startswith("step")]
    assert len(losses) >= 3 and losses[-1] < losses[0], res.stdout
