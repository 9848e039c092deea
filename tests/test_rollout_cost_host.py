"""Host side of the roll-out cost (sr_rollout_cost, sr_rollout_cost_vjp; safe_exploration_amd.utils_casadi).  No GPU.

1. The two entries are declared by the header, exported by the library, bound in _lib.py with the agreed signatures, built from
   sr_rollout_cost.hip; the module has the reference's names and the agreed device surface, and is exported by the package (fails
   without the feature).  Wrong shapes and an indefinite W raise ValueError before a device is touched.
2. trig_prop (mean, variance, input-output covariance), loss_sat and loss_quadratic against tensor Gauss-Hermite quadrature
   (48 nodes a dimension, n_s <= 3): 1e-12 absolute on quantities of size 1 (the integrands are entire; 48 nodes integrate them to
   rounding at these variances).
3. The reference's closed-form reverse pass (tests/_rollout_cost_ref.vjp) against torch autograd (CPU) through a torch port of the
   cost -- 1e-11 of the largest element: two fp64 evaluations with an explicit inverse --, and in long double against central
   differences -- 1e-8 (step 1e-6: truncation 1e-12, rounding 1e-13).
4. The host generic_cost with trig_aug / loss_sat / loss_quadratic callables against the batched reference: 1e-12 at the cost's scale.
5. The floors behind the GPU bars, on exactly _rollout_cost_ref.CASES (the GPU test's inputs): fp64 against long double of the
   reference, per quantity; at the target; and the chain floor: the gradient in k_ff, k_fb through the NumPy roll-out's reverse sweep
   (tests/_moments_rollout_grad_ref) with the closed-form seeds against the seeds of torch autograd through the torch port.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _rollout_cost_ref as RC

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="np.longdouble is no wider than float64 here")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_and_bound(lib_built):
    """fails without the feature"""
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    hdr = _read("include", "safereach.h")
    for name in ("sr_rollout_cost", "sr_rollout_cost_vjp"):
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export " + name
        assert re.search(r"^int %s\(int device, long T, int H, int n_s, int n_u, int idx_angle" % name, hdr, re.M), name
    for word in ("NULL = zero", "W = F F^T", "expm1", "in the order i = 0 .. H - 1", "SR_EINVAL", "SR_EUNSUPPORTED n_s > 12", "T == 0 is a no-op",
                 "NULL = ones", "exactly symmetric", "row H - 1 exactly zero", "not all three", "`stream`"):
        assert word in hdr, word
    from safe_exploration_amd import _lib
    P, I, L, D = _lib._P, _lib._I, _lib._L, _lib._D
    head = [I, L, I, I, I, I, D, I, I, P, P, D, D]
    assert _lib.SIGNATURES["sr_rollout_cost"] == (ctypes.c_int, head + [P] * 7)
    assert _lib.SIGNATURES["sr_rollout_cost_vjp"] == (ctypes.c_int, head + [P] * 9)
    assert "sr_rollout_cost.hip" in _read("safe_exploration_amd", "csrc", "Makefile")


def test_python_surface(lib_built):
    import safe_exploration_amd
    from safe_exploration_amd import utils_casadi as uc
    assert safe_exploration_amd.utils_casadi is uc and "utils_casadi" in safe_exploration_amd.__all__
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(uc.trig_prop) == ["m", "v", "idx", "a"]
    assert names(uc.trig_aug) == ["m", "v", "idx", "a", "keep_radian"]
    assert names(uc.loss_sat) == ["m", "v", "z", "W"]
    assert names(uc.loss_quadratic) == ["m", "z", "v", "W"]
    assert names(uc.generic_cost) == ["mu", "sigma", "u", "step_cost", "terminal_cost", "state_trafo", "lambd"]
    assert names(uc.cost_dev_safe_perf) == ["m_safe", "m_perf", "W"]
    common = ["mu_all", "sigma_all", "z", "W", "u", "R", "idx_angle", "a", "keep_radian", "loss", "w_stage", "w_term"]
    assert names(uc.rollout_cost_batch) == common + ["return_steps", "differentiable", "device"]
    assert names(uc.rollout_cost_vjp_batch) == common + ["cost_bar", "device"]
    sig = inspect.signature(uc.rollout_cost_batch)
    assert [sig.parameters[n].default for n in names(uc.rollout_cost_batch)[3:]] == [None, None, None, None, 1.0, False, "sat", 1.0, 1.0,
                                                                                      False, False, None]


def test_refusals_before_any_device(lib_built):
    from safe_exploration_amd import utils_casadi as uc
    mu, sg, z = np.zeros((2, 3, 4)), np.zeros((2, 3, 4, 4)), np.zeros(5)
    ok = dict(mu_all=mu, sigma_all=sg, z=z, idx_angle=2)
    bad = (dict(W=np.diag([1.0, 1, 1, 1, -1e-3])), dict(W=np.eye(4)), dict(W=np.triu(np.ones((5, 5)))), dict(z=np.zeros(4)), dict(mu_all=mu[0]),
           dict(sigma_all=sg[:, :2]), dict(idx_angle=4), dict(idx_angle=None, keep_radian=True, z=np.zeros(4)), dict(loss="huber"),
           dict(u=np.zeros((2, 3, 1))), dict(R=np.eye(1)), dict(u=np.zeros((2, 2, 1)), R=np.eye(1)), dict(u=np.zeros((2, 3, 1)), R=np.eye(2)))
    for kw in bad:
        for fn in (uc.rollout_cost_batch, uc.rollout_cost_vjp_batch):
            with pytest.raises(ValueError):
                fn(**dict(ok, **kw))
    with pytest.raises(ValueError):
        uc.loss_sat(None, None, z, np.diag([1.0, 1, 1, 1, -1.0]))
    with pytest.raises(TypeError):
        uc.rollout_cost_batch(mu, sg, z, idx_angle=2, differentiable=True)
    # tiny negative eigenvalues are rounding, not indefiniteness
    F = uc.factor_weight(np.diag([20.0, 0, 0, 0, 5]) / 100 - 1e-18 * np.eye(5), 5)
    assert np.allclose(F @ F.T, np.diag([20.0, 0, 0, 0, 5]) / 100, atol=1e-16)


# ---- 2. against quadrature ----------------------------------------------------------------------------------------------------------
def _quadrature(m, v, order=48):
    """nodes (K, d) and weights (K) of the tensor Gauss-Hermite rule for N(m, v)"""
    d = m.size
    xi, wi = np.polynomial.hermite_e.hermegauss(order)
    wi = wi / wi.sum()
    grids = np.meshgrid(*([xi] * d), indexing="ij")
    pts = np.stack([g.reshape(-1) for g in grids], axis=1)
    w = np.ones(pts.shape[0])
    for k in range(d):
        w = w * np.meshgrid(*([wi] * d), indexing="ij")[k].reshape(-1)
    lam, vec = np.linalg.eigh(v)
    return m + pts @ (vec * np.sqrt(np.clip(lam, 0, None))).T, w


def _gauss(n_s, seed):
    rng = np.random.RandomState(seed)
    A = rng.randn(n_s, n_s) * 0.4
    return rng.randn(n_s), A @ A.T + 0.02 * np.eye(n_s)


@pytest.mark.parametrize("n_s", (1, 2, 3))
def test_trig_prop_against_quadrature(lib_built, n_s):
    from safe_exploration_amd import utils_casadi as uc
    for idx in range(n_s):
        m, v = _gauss(n_s, 10 * n_s + idx)
        x, w = _quadrature(m, v)
        f = 0.7 * np.stack((np.sin(x[:, idx]), np.cos(x[:, idx])), axis=1)
        mean = w @ f
        var = (f - mean).T @ ((f - mean) * w[:, None])
        cov_io = (x - m).T @ ((f - mean) * w[:, None])
        m_out, v_out, c_out = uc.trig_prop(m[:, None], v, idx, 0.7)
        assert m_out.shape == (2, 1) and v_out.shape == (2, 2) and c_out.shape == (n_s, 2)
        assert np.max(np.abs(m_out[:, 0] - mean)) <= 1e-12
        assert np.max(np.abs(v_out - var)) <= 1e-12
        assert np.max(np.abs(v @ c_out - cov_io)) <= 1e-12
        for keep in (False, True):                                             # the augmented state is the joint Gaussian's moments
            m_aug, v_aug = uc.trig_aug(m[:, None], v, idx, 0.7, keep)
            joint = np.concatenate((x, f), axis=1)
            if not keep:
                joint = np.delete(joint, idx, axis=1)
            jm = w @ joint
            assert np.max(np.abs(m_aug[:, 0] - jm)) <= 1e-12
            assert np.max(np.abs(v_aug - (joint - jm).T @ ((joint - jm) * w[:, None]))) <= 1e-12
            assert np.linalg.eigvalsh(v_aug).min() >= -1e-15
    m_out, v_out, _ = uc.trig_prop(np.array([0.3]), np.zeros((1, 1)), 0)
    assert np.array_equal(v_out, np.zeros((2, 2)))                             # a point: exactly zero


@pytest.mark.parametrize("n_s", (1, 2, 3))
def test_the_losses_against_quadrature(lib_built, n_s):
    from safe_exploration_amd import utils_casadi as uc
    rng = np.random.RandomState(n_s)
    m, v = _gauss(n_s, 50 + n_s)
    z = rng.randn(n_s)
    Bm = rng.randn(n_s, max(1, n_s - 1))
    for W in (None, Bm @ Bm.T):                                                # (the second is singular for n_s >= 2)
        Wm = np.eye(n_s) if W is None else W
        x, w = _quadrature(m, v)
        q = np.einsum("ki,ij,kj->k", x - z, Wm, x - z)
        assert abs(uc.loss_sat(None, None, z, W)(m, v) - w @ (1 - np.exp(-q / 2))) <= 1e-12
        assert abs(uc.loss_quadratic(m, z, v, W) - w @ q) <= 1e-12 * max(1.0, w @ q)
        x64 = dict(mu=m[None, None], sigma=v[None, None], u=None, R=None, z=z, W=W, idx=None, keep=False, a=1.0, w_stage=1.0, w_term=1.0)
        assert abs(RC.cost(dict(x64, loss="sat"))[1][0] - w @ (1 - np.exp(-q / 2))) <= 1e-12
        assert abs(RC.cost(dict(x64, loss="quadratic"))[1][0] - w @ q) <= 1e-12 * max(1.0, w @ q)


# ---- 3. the closed-form reverse pass ----------------------------------------------------------------------------------------------
VJP_CASES = [dict(n_s=3, aug=aug, T=2, H=3, sigma=sigma, wkind=wkind, loss=loss, pos=pos, seed=8)
             for aug, pos in (("none", "mid"), ("drop", "first"), ("keep", "last"), ("drop", "mid"))
             for sigma, wkind in (("full", "dense2"), ("rank1", "diag"), ("none", "none"))
             for loss in ("sat", "quadratic")]


def _autograd(x):
    import torch
    mu = torch.tensor(x["mu"], requires_grad=True)
    sigma = torch.tensor(x["sigma"] if x["sigma"] is not None else np.zeros(x["mu"].shape + x["mu"].shape[-1:]), requires_grad=True)
    u = None if x["u"] is None else torch.tensor(x["u"], requires_grad=True)
    c = RC.torch_cost(mu, sigma, x, u)
    leaves = [mu, sigma] + ([u] if u is not None else [])
    g = torch.autograd.grad((c * torch.tensor(x["cost_bar"])).sum(), leaves)
    return c.detach().numpy(), dict(mu_bar=g[0].numpy(), sigma_bar=g[1].numpy(), u_bar=g[2].numpy() if u is not None else None)


@pytest.mark.parametrize("case", VJP_CASES, ids=RC.case_id)
def test_the_reference_reverse_pass_against_autograd_and_central_differences(case):
    x = RC.make_inputs(**case)
    ref = RC.vjp(x, x["cost_bar"])
    c, auto = _autograd(x)
    assert RC.rel_err(c, RC.cost(x)[1]) <= 1e-12
    for k in RC.OUTS:
        if ref[k] is not None:
            assert RC.rel_err(auto[k], ref[k]) <= 1e-11, (k, RC.rel_err(auto[k], ref[k]))
    assert np.array_equal(ref["sigma_bar"], ref["sigma_bar"].transpose(0, 1, 3, 2))
    assert np.array_equal(ref["u_bar"][:, -1], np.zeros_like(ref["u_bar"][:, -1]))
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        return
    step = LD(1e-6)
    f = lambda y: (RC.cost(y, LD)[1] * x["cost_bar"].astype(LD)).sum()
    sym = x["sigma"] is not None
    for key, out in (("mu", "mu_bar"), ("sigma", "sigma_bar"), ("u", "u_bar")):
        if x[key] is None:
            continue
        fd = np.zeros(x[key].shape)
        for i in np.ndindex(x[key].shape):
            vals = []
            for sgn in (1, -1):
                arr = x[key].astype(LD)
                arr[i] += sgn * step
                vals.append(f(dict(x, **{key: arr})))
            fd[i] = float((vals[0] - vals[1]) / (2 * step))
        if key == "sigma":
            fd = (fd + fd.transpose(0, 1, 3, 2)) / 2
        assert RC.rel_err(fd, ref[out]) <= 1e-8, (key, RC.rel_err(fd, ref[out]))
    assert sym or ref["sigma_bar"].shape == x["mu"].shape + (x["n_s"],)


# ---- 4. the host generic_cost -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in VJP_CASES if c["sigma"] != "none"], ids=RC.case_id)
def test_generic_cost_with_callables_against_the_batched_reference(lib_built, case):
    from safe_exploration_amd import utils_casadi as uc
    x = RC.make_inputs(**case)
    steps, total = RC.cost(x)
    trafo = None if x["idx"] is None else (lambda m, v: uc.trig_aug(m, v, x["idx"], x["a"], x["keep"]))
    if x["loss"] == "sat":
        l_sat = uc.loss_sat(None, None, x["z"], x["W"])
        loss = lambda m, v: l_sat(m, v)
    else:
        loss = lambda m, v: uc.loss_quadratic(m, x["z"], v, x["W"])
    stage = lambda m, v, u: x["w_stage"] * loss(m, v) + float((u.T @ x["R"] @ u)[0, 0])
    term = lambda m, v: x["w_term"] * loss(m, v)
    for t in range(x["T"]):
        got = uc.generic_cost(x["mu"][t], x["sigma"][t].reshape(x["H"], -1), x["u"][t], stage, term, trafo)
        assert abs(got - total[t]) <= 1e-12 * x["H"] * RC.cost_scale(x), (t, got, total[t])
    assert uc.cost_dev_safe_perf(x["mu"][0], x["mu"][1]) == pytest.approx(2 * ((x["mu"][0, 1:] - x["mu"][1, 1:]) ** 2).sum(), rel=1e-14)


# ---- 5. the floors behind the GPU bars ----------------------------------------------------------------------------------------------
@needs_ld
def test_the_floors_behind_the_gpu_bars():
    worst = {}
    for c in RC.CASES:
        x = RC.make_inputs(**c)
        (s64, c64), (sld, cld) = RC.cost(x), RC.cost(x, LD)
        g64, gld = RC.vjp(x, x["cost_bar"]), RC.vjp(x, x["cost_bar"], LD)
        scale = RC.cost_scale(x)
        e = dict(cost=max(float(np.max(np.abs(s64 - sld))) / scale, float(np.max(np.abs(c64 - cld))) / (scale * x["H"])))
        for k in RC.OUTS:
            if gld[k] is not None:
                e[k] = RC.rel_err(g64[k], gld[k])
        for k, v in e.items():
            if v > worst.get(k, (0.0, None))[0]:
                worst[k] = (v, RC.case_id(c))
    for k, (v, where) in worst.items():
        print("fp64 against long double, %s: worst %.3e at %s; the GPU bar is %.2e" % (k, v, where, RC.FACTOR * RC.FLOOR[k]))
        assert v <= RC.FLOOR[k], (k, v, where)
        assert v >= RC.FLOOR[k] / 4, "FLOOR[%s] is not what is measured here any more: %.3e" % (k, v)


@needs_ld
def test_the_reference_at_the_target():
    """the long-double reference's own uncertainty at a cost of 1e-9 is far below TARGET_RTOL, the fp64 reference's far above"""
    x = RC.target_inputs()
    steps = RC.cost(x, LD)[0]
    assert 1e-10 < float(steps.min()) and float(steps.max()) < 1e-8
    # the unexpanded expressions in fp64 lose the cost's digits: this is why the GPU test compares with the long-double evaluation
    err64 = float(np.max(np.abs(RC.cost(x)[0] / steps - 1)))
    print("at the target: cost %.2e .. %.2e, fp64 reference off by %.1e of it" % (steps.min(), steps.max(), err64))
    assert err64 > RC.TARGET_RTOL
    # the long-double evaluation against a second long-double route without the cancellation (the host module's algebra)
    from safe_exploration_amd.utils_casadi import factor_weight
    F = factor_weight(x["W"], 5).astype(LD)
    m, v, W, z, a = RC._states(x, LD)
    th, s2 = m[:, 2], v[:, 2, 2]
    e, xx, h = np.exp(-s2), -np.expm1(-s2), np.exp(-s2 / 2)
    vt = np.empty((m.shape[0], 2, 2), dtype=LD)
    vt[:, 0, 0], vt[:, 1, 1] = a * a * xx / 2 * (1 + e * np.cos(2 * th)), a * a * xx / 2 * (1 - e * np.cos(2 * th))
    vt[:, 0, 1] = vt[:, 1, 0] = -a * a * xx / 2 * e * np.sin(2 * th)
    C = v[:, :, 2:3] * np.stack((a * h * np.cos(th), -a * h * np.sin(th)), axis=1)[:, None, :]
    ma = np.delete(np.concatenate((m, (a * h * np.sin(th))[:, None], (a * h * np.cos(th))[:, None]), axis=1), 2, axis=1)
    va = np.concatenate((np.concatenate((v, C), axis=2), np.concatenate((C.transpose(0, 2, 1), vt), axis=2)), axis=1)
    va = np.delete(np.delete(va, 2, axis=1), 2, axis=2)
    E = F.T @ va @ F
    # to first order in E (E is 1e-9: the second order is 1e-18 of 1): loss = tr(E) / 2 + |F^T d|^2 / 2 - (tr E)^2 / 8 - tr(E^2) / 4 ..
    y = (ma - z) @ F
    first = np.trace(E, axis1=1, axis2=2) / 2 + (y * y).sum(axis=1) / 2
    w = RC._weights(x, LD).reshape(-1)
    assert float(np.max(np.abs(first * w / steps.reshape(-1) - 1))) <= RC.TARGET_RTOL / 2


@needs_ld
def test_the_floor_behind_the_chain_bar():
    """seeds of the closed form against seeds of autograd through the torch port, both pushed through the same NumPy reverse sweep"""
    import torch
    import _moments_rollout_grad_ref as MR
    worst = 0.0
    for n_s, idx in ((2, 1), (4, 2)):
        for mode in (1, 2):
            T, H, n_u = 3, 4, 1
            gp = MR.NumpyGP(n_s, n_s + n_u, 30, seed=7)
            r = MR.rollout_inputs(n_s, n_u, T, H, seed=2)
            ma, sa, _ = MR.forward(gp, r, H, mode, "point", None, np.float64)
            x = RC.make_inputs(n_s, "drop", T=T, H=H, wkind="diag", ctrl=False, seed=6)
            x["idx"] = idx
            x["mu"], x["sigma"] = np.asarray(ma, dtype=np.float64), np.asarray(sa, dtype=np.float64)
            closed = RC.vjp(x)
            mu, sg = torch.tensor(x["mu"], requires_grad=True), torch.tensor(x["sigma"], requires_grad=True)
            auto = torch.autograd.grad(RC.torch_cost(mu, sg, x).sum(), [mu, sg])
            lins = MR.linearisations(gp, r, ma, H, None)
            zero = np.zeros((T, H, n_s))
            g1 = MR.sweep(r, H, mode, lins, ma, sa, closed["mu_bar"], closed["sigma_bar"], zero, "point", None, fp64=True)
            g2 = MR.sweep(r, H, mode, lins, ma, sa, auto[0].numpy(), auto[1].numpy(), zero, "point", None, fp64=True)
            for k in ("k_ff", "k_fb"):
                worst = max(worst, MR.rel_err(g1[k], g2[k]))
    print("closed-form seeds against autograd seeds through the same sweep: worst %.3e of the largest element; CHAIN_RTOL = %.2e"
          % (worst, RC.CHAIN_RTOL))
    assert worst <= RC.CHAIN_FLOOR
    assert worst >= RC.CHAIN_FLOOR / 4, "CHAIN_FLOOR is not what is measured here any more: %.3e" % worst
