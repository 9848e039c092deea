"""Host side of the exploration objective and of the variance seed of the roll-out's reverse pass (sr_multistep_reach_var,
sr_multistep_reach_var_vjp, sr_rollout_explore, sr_rollout_explore_vjp; gp_reachability.exploration_cost_batch and friends).  No GPU.

0. The new names are declared by the header, the ctypes table, the Makefile and gp_reachability.py, with as many ctypes arguments
   as the declarations have (fails without the feature); safempc_default_cost against the expressions of the reference written
   out here, both n_perf branches; wrong shapes raise ValueError before anything touches a device.
1. The floor of the objective's GPU bar: fp64 against long double of cost, steps, gpvar_bar, p_bar, mu_bar on _explore_ref.OBJ_CASES.
   The closed-form gradient against central differences of the objective in long double.
2. The floor of the roll-out's GPU bar: the fp64 against the long-double sweep with the seeds (w_p, w_q, w_v), w_v alone and w_v = None
   on _explore_ref.ROLL_CASES x both starts with _reach_rollout_grad_ref.NumpyGP standing in (N = 30).  With w_v = None the sweep is
   _reach_rollout_grad_ref.sweep to the bit.  Trajectories with an eigen-gap factor g < G_MIN at any step are left out, at most
   2 % of a case (asserted).
3. The sweep against central differences in long double of the roll-out extended by its variance output (n_s = 2, n_u = 1, N = 20,
   H = 3, both starts; n_s = 3 behind an input transform): bar 1e-8 of the largest element (step 1e-7: truncation 1e-14, rounding
   1e-12), as tests/test_reach_rollout_vjp_host.py sets it.
Each bar of the GPU test is 30 x the floor recorded in _explore_ref.py; the measured floor must stay below the recorded one (and
above a quarter of it: the record is what is measured).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import _explore_ref as E
import _reach_rollout_grad_ref as RR

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the records in _explore_ref.py were measured with the 80-bit long double of x86-64 and this NumPy's summation order: only there is a
# floor far BELOW its record a sign that the record is stale; the upper bound, which the GPU bars rest on, holds everywhere
X87 = np.finfo(LD).nmant == 63
needs_ld = pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="np.longdouble is no wider than float64 here")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_new_names_are_declared():
    """fails without the feature"""
    header = _read("include", "safereach.h")
    lib_py = _read("safe_exploration_amd", "_lib.py")
    for name in ("sr_multistep_reach_var", "sr_multistep_reach_var_vjp", "sr_rollout_explore", "sr_rollout_explore_vjp"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert '"%s"' % name in lib_py, name
    src = _read("safe_exploration_amd", "gp_reachability.py")
    for name in ("exploration_cost_batch", "exploration_cost_vjp_batch", "safempc_default_cost"):
        assert re.search(r"^def %s\(" % name, src, re.M), name
    assert "sr_rollout_explore.hip" in _read("safe_exploration_amd", "csrc", "Makefile")
    # the ctypes signatures have as many arguments as the declarations, and the new ones extend the old ones by one pointer
    from safe_exploration_amd import _lib
    P = ctypes.c_void_p
    for name in ("sr_multistep_reach_var", "sr_multistep_reach_var_vjp", "sr_rollout_explore", "sr_rollout_explore_vjp"):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(_lib.SIGNATURES[name][1]) == len(decl.split(",")), name
    assert _lib.SIGNATURES["sr_multistep_reach_var"][1] == _lib.SIGNATURES["sr_multistep_reach"][1] + [P]
    assert _lib.SIGNATURES["sr_multistep_reach_var_vjp"][1] == _lib.SIGNATURES["sr_multistep_reach_vjp"][1] + [P]
    assert _lib.SIGNATURES["sr_rollout_explore_vjp"][1] == _lib.SIGNATURES["sr_rollout_explore"][1] + [P, P]


def test_safempc_default_cost_is_the_reference_expression():
    from safe_exploration_amd.gp_reachability import safempc_default_cost
    rng = np.random.default_rng(5)
    n_s, n_safe, n_perf = 3, 4, 6
    p_all, sig = rng.standard_normal((n_safe, n_s)), rng.uniform(1e-3, 1e-2, (n_safe, n_s))
    mu, sigp, wx = rng.standard_normal((n_perf, n_s)), rng.uniform(1e-3, 1e-2, (n_perf, n_s)), rng.standard_normal((n_s, n_s))
    for eps in (0.0, 1e-6):
        want = -sum(np.sqrt(np.sum(sig[i, :] + eps)) for i in range(n_safe))
        assert abs(safempc_default_cost(p_all, sig, eps_noise=eps) - want) <= 4e-16 * abs(want)
        assert safempc_default_cost(p_all, sig, mu, sigp, wx, n_perf=1, eps_noise=eps) == safempc_default_cost(p_all, sig, eps_noise=eps)
        want = 0.0
        for i in range(1, min(n_perf, n_safe)):
            d = (mu[i, :] - p_all[i, :]).reshape(1, -1)
            want += d.dot((.1 * wx).dot(d.T))[0, 0]
        for i in range(n_perf):
            want -= np.sqrt(np.sum(sigp[i, :] + eps))
        got = safempc_default_cost(p_all, sig, mu, sigp, wx, n_safe=n_safe, n_perf=n_perf, eps_noise=eps)
        assert abs(got - want) <= 1e-15 * max(1.0, abs(want))
    with pytest.raises(ValueError):
        safempc_default_cost(p_all, sig, mu, None, wx, n_perf=n_perf)


def test_wrong_arguments_raise_before_the_device():
    from safe_exploration_amd import gp_reachability as reach
    v, p, mu, wx = np.ones((3, 4, 2)), np.zeros((3, 4, 2)), np.zeros((3, 5, 2)), np.eye(2)
    bad = (dict(gp_var_all=np.ones((3, 4))), dict(kind="max"), dict(eps=-1.0), dict(p_all=p), dict(p_all=p, mu_perf=mu),
           dict(p_all=p, mu_perf=mu, wx_cost=np.eye(3)), dict(p_all=p, mu_perf=mu, wx_cost=wx, n_dev=5), dict(n_dev=2),
           dict(p_all=p[:2], mu_perf=mu, wx_cost=wx), dict(gp_var_all=np.ones((3, 0, 2))))
    for kw in bad:
        kw = dict(dict(gp_var_all=v), **kw)
        with pytest.raises(ValueError):
            reach.exploration_cost_batch(**kw)
        with pytest.raises(ValueError):
            reach.exploration_cost_vjp_batch(**kw)
    with pytest.raises(ValueError):
        reach.exploration_cost_vjp_batch(v, cost_bar=np.ones(4))
    with pytest.raises(NotImplementedError):
        reach.exploration_cost_batch(np.ones((3, 4, 13)))
    with pytest.raises(TypeError):
        reach.exploration_cost_batch(v, differentiable=True)


# ---- 1. the objective -------------------------------------------------------------------------------------------------------------
@needs_ld
def test_the_floor_behind_the_objective_bar():
    worst, where = 0.0, None
    for case in E.OBJ_CASES:
        x = E.objective_inputs(case)
        for cb in (x["cost_bar"], None):
            ld = E.objective(x) + E.objective_grad(x, cb)
            f64 = E.objective(x, np.float64) + E.objective_grad(x, cb, np.float64)
            for name, a, b in zip(("cost", "steps", "gpvar_bar", "p_bar", "mu_bar"), f64, ld):
                if b is None:
                    assert a is None
                    continue
                e = RR.rel_err(a, b)
                if e > worst:
                    worst, where = e, (E.case_id(case), name)
        # rows outside 1 .. n_dev - 1 are exact zeros in the reference itself
        if x["p"] is not None:
            for g in ld[3:]:
                assert not g[:, 0].any() and not g[:, x["n_dev"]:].any()
    print("objective, long double against fp64: worst %.3e of the largest element at %s; OBJ_RTOL = %.2e" % (worst, where, E.OBJ_RTOL))
    assert worst <= E.OBJ_FLOOR, (worst, where)
    if X87:
        assert worst >= E.OBJ_FLOOR / 4, "OBJ_FLOOR is not what is measured here any more: %.3e" % worst


@needs_ld
@pytest.mark.parametrize("case", (E.OBJ_CASES[4], E.OBJ_CASES[7], (4, 2, 3, "sqrt", 1e-6, (3, 4, None))), ids=E.case_id)
def test_the_objective_gradient_against_central_differences(case):
    x = E.objective_inputs(case)
    for k in ("v", "p", "mu"):
        x[k] = x[k][:3]                                         # three trajectories are enough here
    x["cost_bar"] = x["cost_bar"][:3]
    grads = dict(zip(("v", "p", "mu"), E.objective_grad(x, x["cost_bar"])))
    step = LD(1e-7)
    for key, g in grads.items():
        fd = np.zeros(x[key].shape)
        for idx in np.ndindex(x[key].shape):
            vals = []
            for sgn in (1, -1):
                arr = x[key].astype(LD)
                arr[idx] += sgn * step
                vals.append((E.objective(dict(x, **{key: arr}))[0] * x["cost_bar"].astype(LD)).sum())
            fd[idx] = float((vals[0] - vals[1]) / (2 * step))
        err = RR.rel_err(g, fd)
        print("d/d%s: closed form against central differences %.2e of the largest element" % (key, err))
        # sqrt(r) at r ~ 1e-3 .. 1e-1 with a step of 1e-7: truncation (step / r)^2 / 8 ~ 1e-9 of the derivative at the smallest r
        assert err <= (1e-7 if key == "v" and x["kind"] == "sqrt" else 1e-8), (key, err)


# ---- 2. the sweep with the variance seed: the floor -----------------------------------------------------------------------------------
@needs_ld
def test_the_floor_behind_the_rollout_bar():
    worst, where = 0.0, None
    for key, T, H in E.ROLL_CASES:
        assert (key, T, H) in RR.CASES
        n_s, n_u, tz = RR.model_dims(key)
        gp = RR.NumpyGP(n_s, (n_s if tz is None else tz.shape[0]) + n_u, 30, seed=7)
        x = RR.rollout_inputs(n_s, n_u, T, H)
        for start_q in (False, True):
            pa, qa = RR.forward(gp, x, H, start_q, tz, np.float64)
            lins = RR.linearisations(gp, x, pa, H, tz)
            for which in E.SEEDS:
                w_p, w_q, w_v = E.seeds(x, which)
                ld = E.sweep_var(x, H, lins, pa, qa, w_p, w_q, w_v, start_q, tz)
                f64 = E.sweep_var(x, H, lins, pa, qa, w_p, w_q, w_v, start_q, tz, fp64=True)
                assert not ld["bad"].any()
                keep = ld["g"] >= RR.G_MIN
                assert (~keep).sum() <= 0.02 * T, (key, T, H, start_q, int((~keep).sum()))
                for name in RR.NAMES:
                    if ld[name] is None:
                        continue
                    e = RR.rel_err(f64[name], ld[name], keep)
                    if e > worst:
                        worst, where = e, (key, T, H, start_q, which, name)
                if which == "no_w_v":
                    base = RR.sweep(x, H, lins, pa, qa, w_p, w_q, start_q, tz)
                    assert all(ld[k] is None or np.array_equal(ld[k], base[k]) for k in RR.NAMES), "w_v = None is not the old sweep"
    print("roll-out with the variance seed, long double against fp64 sweep: worst %.3e of the largest element at %s; VAR_RTOL = %.2e"
          % (worst, where, E.VAR_RTOL))
    assert worst <= E.VAR_FLOOR, (worst, where)
    if X87:
        assert worst >= E.VAR_FLOOR / 4, "VAR_FLOOR is not what is measured here any more: %.3e" % worst


# ---- 3. the sweep against central differences of the roll-out with its variances ---------------------------------------------------
def _functional(gp, x, H, start_q, tz, t, w_v):
    pa, qa, va = E.forward_var(gp, x, H, start_q, tz, LD, t)
    return (pa[0] * x["w_p"][t].astype(LD)).sum() + (qa[0] * x["w_q"][t].astype(LD)).sum() + (va[0] * w_v[t].astype(LD)).sum()


@needs_ld
@pytest.mark.parametrize("shape", ((2, 1, None), (3, 1, np.eye(3)[1:])), ids=("2x1", "3x1_tz"))
@pytest.mark.parametrize("start_q", (False, True), ids=("from_a_point", "from_q0"))
def test_the_sweep_with_the_variance_seed_against_central_differences(shape, start_q):
    n_s, n_u, tz = shape
    T, H, N = 2, 3, 20
    gp = RR.NumpyGP(n_s, (n_s if tz is None else tz.shape[0]) + n_u, N, seed=3)
    x = RR.rollout_inputs(n_s, n_u, T, H, seed=1)
    w_v = E.variance_seed(x)
    pa, qa, va = E.forward_var(gp, x, H, start_q, tz, LD)
    pa2, qa2 = RR.forward(gp, x, H, start_q, tz, LD)
    assert np.array_equal(pa, pa2) and np.array_equal(qa, qa2) and va.shape == (T, H, n_s) and (va > 0).all()
    lins = RR.linearisations(gp, x, pa, H, tz, LD)
    assert np.array_equal(lins[1], va), "the variances of the forward are those of the linearisations"
    ref = E.sweep_var(x, H, lins, pa, qa, x["w_p"], x["w_q"], w_v, start_q, tz)
    assert not ref["bad"].any()
    step = LD(1e-7)
    leaves = dict(p_0="p", k_ff="k_ff", k_fb="k_fb")
    if start_q:
        leaves.update(q_0="q", k_fb_init="k_fb0")
    for name, key in leaves.items():
        fd = np.zeros(x[key].shape)
        for t in range(T):
            for idx in np.ndindex(x[key].shape[1:]):
                vals = []
                for sgn in (1, -1):
                    arr = x[key].astype(LD)
                    arr[(t,) + idx] += sgn * step
                    vals.append(_functional(gp, dict(x, **{key: arr}), H, start_q, tz, t, w_v))
                fd[(t,) + idx] = float((vals[0] - vals[1]) / (2 * step))
        err = RR.rel_err(ref[name], fd)
        print("d/d%s: sweep with w_v against central differences %.2e of the largest element" % (name, err))
        assert err <= 1e-8, (name, err)
    # the variance seed matters: without it the gradient is another one
    without = E.sweep_var(x, H, lins, pa, qa, x["w_p"], x["w_q"], None, start_q, tz)
    assert RR.rel_err(without["k_ff"], ref["k_ff"]) > 1e-6


# ---- the floor of the end-to-end bar --------------------------------------------------------------------------------------------------
def test_the_floor_behind_the_end_to_end_bar():
    """the gradient of the n_perf > 1 default cost in p_0 and the controls of both roll-outs: the closed-form seeds against the
    seeds of torch autograd through the cost written in torch, both pushed through the same NumPy reverse sweeps (fp64) at one
    stored forward"""
    import torch
    import _moments_rollout_grad_ref as MR
    worst = 0.0
    for n_s in (2, 4):
        safe, perf, wx = E.e2e_inputs(n_s)
        gp = RR.NumpyGP(n_s, n_s + 1, 30, seed=7)
        Hs, Hp, eps = E.E2E_H_SAFE, E.E2E_H_PERF, E.E2E_EPS_NOISE
        pa, qa = RR.forward(gp, safe, Hs, False, None, np.float64)
        ma, sa, va = MR.forward(gp, perf, Hp, 1, "point", None, np.float64)
        lins_s, lins_p = RR.linearisations(gp, safe, pa, Hs, None), RR.linearisations(gp, perf, ma, Hp, None)
        x = dict(v=va, kind="sqrt", eps=n_s * eps, p=pa, mu=ma, wx=wx, n_dev=min(Hs, Hp))
        closed = E.objective_grad(x, None, np.float64)
        leaves = [torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in (va, pa, ma)]
        auto = [g.numpy() for g in torch.autograd.grad(E.torch_default_cost(leaves[1], leaves[2], leaves[0], torch.tensor(wx), eps), leaves)]
        grads = []
        for gv, pb, mb in (closed, auto):
            gs = RR.sweep(safe, Hs, lins_s, pa, qa, pb, None, False, None, fp64=True)
            gp_ = MR.sweep(perf, Hp, 1, lins_p, ma, sa, mb, None, gv, "point", None, fp64=True)
            grads.append(dict(p_0=gs["p_0"] + gp_["mu_0"], k_ff_safe=gs["k_ff"], k_fb_safe=gs["k_fb"], k_ff_perf=gp_["k_ff"], k_fb_perf=gp_["k_fb"]))
        for k in grads[0]:
            worst = max(worst, RR.rel_err(grads[0][k], grads[1][k]))
    print("closed-form seeds against autograd seeds through the same sweeps: worst %.3e of the largest element; E2E_RTOL = %.2e"
          % (worst, E.E2E_RTOL))
    assert worst <= E.E2E_FLOOR
    if X87:
        assert worst >= E.E2E_FLOOR / 4, "E2E_FLOOR is not what is measured here any more: %.3e" % worst
