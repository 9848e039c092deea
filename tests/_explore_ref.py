"""Reference of the exploration objective (sr_rollout_explore, sr_rollout_explore_vjp) and of the reverse pass of a reachability
roll-out with a seed on its GP variances (sr_multistep_reach_var_vjp).  NumPy only.  np.longdouble by default; fp64=True /
dt=np.float64 runs the same lines in float64 (the rounding floor of a correct fp64 implementation).

The objective, from the reference's own expressions (safempc_simple.py:286-315, safempc_exploration.py:104), per trajectory:
    kind "sqrt":  cost = - sum_i sqrt(sum_j v[i, j] + eps)          kind "sum":  cost = - sum_i sum_j v[i, j]
    with a deviation term:  + sum_{i=1}^{n_dev-1} (mu[i] - p[i]) W (mu[i] - p[i])^T        (W = 0.1 wx_cost, not symmetric here)
and its closed-form gradient:  gpvar_bar[i, :] = -cost_bar / (2 sqrt(r_i)) (sqrt; exactly 0 at r_i == 0) or -cost_bar (sum);
mu_bar[i] = cost_bar (W + W^T) d_i = -p_bar[i] for 1 <= i < n_dev, zero rows elsewhere.

The roll-out: sweep_var is the sweep of tests/_reach_rollout_grad_ref.py with w_v[t, i] added to the var_bar that
_ellipsoid_grad_ref.step_vjp returns, before the GP link reads it; the step algebra is imported, not copied.  forward_var is
_reach_rollout_grad_ref.forward with the variances the steps used beside its outputs.

BARS.  Every array is compared relative to its own largest element (_reach_rollout_grad_ref.rel_err).  A bar is 30 x the worst
disagreement of the long-double and the fp64 evaluation on exactly the cases the GPU test runs (tests/test_explore_host.py
measures and asserts the floors; roll-outs with a NumPy GP standing in, trajectories with an eigen-gap factor g < G_MIN at any
step left out of the value bars, at most 2 % of a case).  Measured on x86-64 (80-bit long double):
    objective   worst 4.14e-16 (cost; n_s = 5, H_v = 65, T = 64, sqrt, deviation term over 66 rows):  OBJ_FLOOR = 4.2e-16,  OBJ_RTOL = 1.26e-14
    roll-out    worst 6.02e-16 (d/dk_fb_init; rbf45, T = 1, H = 5, from q_0, seeds (w_p, w_q, w_v)):  VAR_FLOOR = 6.1e-16,  VAR_RTOL = 1.83e-14
    end to end  E2E_RTOL = 30 x E2E_FLOOR: the gradient of the n_perf > 1 default cost in p_0 and the controls of a safe (H = 3) and a
                performance (H = 4, Taylor moments) roll-out with the seeds of this reference's closed form against the seeds of torch
                autograd through the cost written in torch (torch_default_cost), both pushed through the same NumPy reverse sweeps on
                the CPU at one stored forward (n_s = 2 and 4, N = 30, T = 3): worst 2.88e-16, E2E_FLOOR = 2.9e-16, E2E_RTOL = 8.7e-15
"""
import numpy as np

import _ellipsoid_ref as R
import _ellipsoid_grad_ref as G
import _reach_rollout_grad_ref as RR

LD = np.longdouble
FACTOR = 30.0
OBJ_FLOOR = 4.2e-16               # measured (see the docstring), rounded up
OBJ_RTOL = FACTOR * OBJ_FLOOR
VAR_FLOOR = 6.1e-16               # measured (see the docstring), rounded up
VAR_RTOL = FACTOR * VAR_FLOOR

# (n_s, H_v, T, kind, eps, dev): dev None or (H_p, H_m, n_dev), n_dev None = min(H_p, H_m).  n_s = 1, 4, 5, 12; H_v = 1, 2, 15, 65
# (past one wavefront); T = 1, 64, 65, 257; both kinds; eps = 0, 1e-6; the deviation term at H_p < H_m and H_p > H_m, n_dev = 2
# and the minimum, n_dev below and above H_v
OBJ_CASES = ((1, 1, 1, "sqrt", 0.0, None), (4, 15, 64, "sqrt", 1e-6, None), (5, 65, 65, "sum", 0.0, None),
             (12, 2, 257, "sqrt", 0.0, None), (4, 2, 65, "sum", 0.0, (3, 5, 2)), (4, 15, 257, "sqrt", 1e-6, (15, 16, None)),
             (5, 65, 64, "sqrt", 0.0, (70, 66, None)), (12, 15, 65, "sqrt", 1e-6, (6, 4, 2)), (1, 65, 1, "sum", 1e-6, (2, 3, None)),
             (12, 1, 64, "sqrt", 0.0, (5, 4, None)))

# the roll-outs of the reverse pass with the variance seed, out of _reach_rollout_grad_ref.CASES, each from a point and from q_0
ROLL_CASES = (("rbf23_150", 65, 5), ("rbf45", 1, 5), ("rbf56", 65, 3), ("cartpole", 65, 3), ("sparse23", 65, 2),
              ("linmat52_23", 65, 3), ("rbf23_150", 1, 1))
SEEDS = ("all", "w_v", "no_w_v")


def case_id(c):
    return "ns%d-Hv%d-T%d-%s-eps%g-%s" % (c[0], c[1], c[2], c[3], c[4], "nodev" if c[5] is None else "dev%d_%d_%s" % c[5])


def objective_inputs(case):
    """inputs of one objective case: v (T,H_v,n_s) > 0, cost_bar (T), and with a deviation term p (T,H_p,n_s), mu (T,H_m,n_s),
    wx (n_s,n_s) not symmetric, n_dev"""
    n_s, H_v, T, kind, eps, dev = case
    rng = np.random.default_rng([n_s, H_v, T, 2828])
    x = dict(v=rng.uniform(1e-4, 1e-2, (T, H_v, n_s)), cost_bar=rng.standard_normal(T), kind=kind, eps=eps, p=None, mu=None, wx=None,
             n_dev=0)
    if dev is not None:
        H_p, H_m, n_dev = dev
        x.update(p=rng.standard_normal((T, H_p, n_s)), mu=rng.standard_normal((T, H_m, n_s)), wx=rng.standard_normal((n_s, n_s)),
                 n_dev=min(H_p, H_m) if n_dev is None else n_dev)
    return x


def objective(x, dt=LD):
    """cost (T), steps (T,H_v) of dtype dt"""
    v = np.asarray(x["v"], dtype=dt)
    T, H_v, _ = v.shape
    steps = np.zeros((T, H_v), dtype=dt)
    cost = np.zeros(T, dtype=dt)
    W = None if x["wx"] is None else np.asarray(0.1 * np.asarray(x["wx"], dtype=np.float64), dtype=dt)
    for t in range(T):
        for i in range(H_v):
            r = v[t, i].sum()
            steps[t, i] = -np.sqrt(r + dt(x["eps"])) if x["kind"] == "sqrt" else -r
        c = steps[t].sum()
        for i in range(1, x["n_dev"]):
            d = (np.asarray(x["mu"][t, i], dtype=dt) - np.asarray(x["p"][t, i], dtype=dt)).reshape(1, -1)
            c = c + d.dot(W.dot(d.T))[0, 0]
        cost[t] = c
    return cost, steps


def objective_grad(x, cost_bar=None, dt=LD):
    """(gpvar_bar, p_bar, mu_bar) of dtype dt; p_bar, mu_bar None without p, mu.  cost_bar None = ones"""
    v = np.asarray(x["v"], dtype=dt)
    T, H_v, n_s = v.shape
    cb = np.ones(T, dtype=dt) if cost_bar is None else np.asarray(cost_bar, dtype=dt)
    gv = np.zeros_like(v)
    for t in range(T):
        for i in range(H_v):
            if x["kind"] == "sqrt":
                r = v[t, i].sum() + dt(x["eps"])
                gv[t, i] = 0 if r == 0 else -cb[t] / (2 * np.sqrt(r))
            else:
                gv[t, i] = -cb[t]
    if x["p"] is None:
        return gv, None, None
    pb, mb = np.zeros(x["p"].shape, dtype=dt), np.zeros(x["mu"].shape, dtype=dt)
    W = np.asarray(0.1 * np.asarray(x["wx"], dtype=np.float64), dtype=dt)
    for t in range(T):
        for i in range(1, x["n_dev"]):
            d = np.asarray(x["mu"][t, i], dtype=dt) - np.asarray(x["p"][t, i], dtype=dt)
            mb[t, i] = cb[t] * (W + W.T).dot(d)
            pb[t, i] = -mb[t, i]
    return gv, pb, mb


# ---- the roll-out with its variances, and the sweep with a seed on them -----------------------------------------------------------
def variance_seed(x):
    """w_v (T,H,n_s) for the inputs of _reach_rollout_grad_ref.rollout_inputs"""
    T, H = x["k_ff"].shape[:2]
    n_s = x["p"].shape[1]
    return np.random.default_rng([T, H, n_s, 2829]).standard_normal((T, H, n_s))


def seeds(x, which):
    """(w_p, w_q, w_v) of a seed variant of SEEDS"""
    w_v = variance_seed(x)
    return dict(all=(x["w_p"], x["w_q"], w_v), w_v=(None, None, w_v), no_w_v=(x["w_p"], x["w_q"], None))[which]


def forward_var(gp, x, H, start_q, tz=None, dt=LD, t=None):
    """_reach_rollout_grad_ref.forward with the third output: p_all, q_all, gp_var_all (T,H,n_s), the variances the steps used"""
    rows = range(x["p"].shape[0]) if t is None else [t]
    n_s = x["p"].shape[1]
    pa, qa, va = [], [], []
    for r in rows:
        p, q = np.asarray(x["p"][r], dtype=dt), (np.asarray(x["q"][r], dtype=dt) if start_q else None)
        if q is not None:
            q = (q + q.T) / 2
        ps, qs, vs = [], [], []
        for i in range(H):
            kfb = (x["k_fb0"][r] if start_q else None) if i == 0 else x["k_fb"][r, i - 1]
            mu, var, jm, _, _ = gp.linearize(RR._z(p, x["k_ff"][r, i], tz, dt), dt)
            o = R.step(p, q, x["k_ff"][r, i], kfb if q is not None else np.zeros((x["k_ff"].shape[2], n_s)), mu, var,
                       RR._jac_state(jm, tz, n_s, dt), x["l_mu"], x["l_sigma"], x["c"], x["a"], x["b"])
            p, q = o["p1"], (o["q1"] + o["q1"].T) / 2
            ps.append(p)
            qs.append(q)
            vs.append(var)
        pa.append(ps)
        qa.append(qs)
        va.append(vs)
    return np.array(pa, dtype=dt), np.array(qa, dtype=dt), np.array(va, dtype=dt)


def sweep_var(x, H, lins, p_all, q_all, w_p, w_q, w_v, start_q, tz=None, fp64=False, rows=None):
    """_reach_rollout_grad_ref.sweep for sum w_p . p_all + w_q . q_all + w_v . gp_var_all (None = zero): the same outputs.  w_v[t, i]
    is added to the var_bar of step i before the GP link; w_v None adds nothing (the lines of that sweep)."""
    dt = np.float64 if fp64 else LD
    T, n_s = x["p"].shape
    n_u = x["k_ff"].shape[2]
    tzm = np.eye(n_s, dtype=dt) if tz is None else np.asarray(tz, dtype=dt)
    nx = tzm.shape[0]
    rows = list(range(T)) if rows is None else list(rows)
    res = dict(p_0=[], q_0=[], k_fb_init=[], k_ff=[], k_fb=[], g=[], bad=[])
    mu, var, jm, jv, hm = lins
    for t in rows:
        p_bar, q_bar = np.zeros(n_s, dtype=dt), np.zeros((n_s, n_s), dtype=dt)
        g_kff, g_kfb = np.zeros((H, n_u), dtype=dt), np.zeros((max(H - 1, 0), n_u, n_s), dtype=dt)
        g_kfb0, g_min, bad = None, 1.0, np.zeros(H, dtype=bool)
        for i in range(H - 1, -1, -1):
            p_in = x["p"][t] if i == 0 else p_all[t, i - 1]
            q_in = (x["q"][t] if start_q else None) if i == 0 else q_all[t, i - 1]
            ell = q_in is not None
            kfb = (x["k_fb0"][t] if i == 0 else x["k_fb"][t, i - 1]) if ell else np.zeros((n_u, n_s))
            sp = p_bar + (0 if w_p is None else np.asarray(w_p[t, i], dtype=dt))
            sq = q_bar + (0 if w_q is None else np.asarray(w_q[t, i], dtype=dt))
            jmt, jvt, hmt = jm[t, i].astype(dt), jv[t, i].astype(dt), hm[t, i].astype(dt)
            o = G.step_vjp(p_in, q_in, x["k_ff"][t, i], kfb, mu[t, i], var[t, i], RR._jac_state(jmt, None if tz is None else tzm, n_s, dt),
                           x["l_mu"], x["l_sigma"], x["c"], x["a"], x["b"], sp, sq, fp64=fp64)
            var_bar = o["var_bar"] if w_v is None else o["var_bar"] + np.asarray(w_v[t, i], dtype=dt)
            jz = np.hstack((o["jac_bar"][:, :n_s].dot(tzm.T), o["jac_bar"][:, n_s:]))
            zb = jmt.T.dot(o["mu_bar"]) + jvt.T.dot(var_bar) + np.einsum('ad,ade->e', jz, hmt)
            p_bar = o["p_bar"] + tzm.T.dot(zb[:nx])
            g_kff[i] = o["kff_bar"] + zb[nx:]
            q_bar = o["q_bar"]
            bad[i] = o["bad"]
            if ell:
                g_min = min(g_min, o["g"])
                if i == 0:
                    g_kfb0 = o["kfb_bar"]
                else:
                    g_kfb[i - 1] = o["kfb_bar"]
        res["p_0"].append(p_bar)
        res["q_0"].append(q_bar)
        res["k_fb_init"].append(g_kfb0)
        res["k_ff"].append(g_kff)
        res["k_fb"].append(g_kfb)
        res["g"].append(g_min)
        res["bad"].append(bad)
    out = {k: np.array(res[k]).astype(np.float64) for k in ("p_0", "k_ff", "k_fb")}
    out["q_0"] = np.array(res["q_0"]).astype(np.float64) if start_q else None
    out["k_fb_init"] = np.array(res["k_fb_init"]).astype(np.float64) if start_q else None
    out["g"], out["bad"] = np.array(res["g"], dtype=np.float64), np.array(res["bad"])
    return out


# ---- the end-to-end test's problem: the n_perf > 1 default cost over a safe and a performance roll-out ---------------------------------
E2E_T, E2E_H_SAFE, E2E_H_PERF, E2E_EPS_NOISE = 3, 3, 4, 1e-6
E2E_FLOOR = 2.9e-16               # measured (see the docstring), rounded up
E2E_RTOL = FACTOR * E2E_FLOOR


def e2e_inputs(n_s, n_u=1):
    """(safe, perf, wx): the inputs of the safe roll-out (H = 3, mode 0 from a point) and of the performance roll-out (H = 4, Taylor
    moments from the same point) as _reach_rollout_grad_ref.rollout_inputs draws them, and wx_cost (n_s,n_s), not symmetric"""
    safe = RR.rollout_inputs(n_s, n_u, E2E_T, E2E_H_SAFE, seed=2)
    perf = RR.rollout_inputs(n_s, n_u, E2E_T, E2E_H_PERF, seed=3)
    perf.update(p=safe["p"], a=safe["a"], b=safe["b"])
    wx = np.random.default_rng([n_s, 2830]).standard_normal((n_s, n_s))
    return safe, perf, wx


def torch_default_cost(p_all, mu_perf, gp_pred_sigma_perf, wx, eps_noise):
    """the n_perf > 1 branch of generate_cost_function in batched torch (T trajectories), summed over the batch"""
    import torch
    n_dev = min(p_all.shape[1], mu_perf.shape[1])
    d = mu_perf[:, 1:n_dev] - p_all[:, 1:n_dev]
    dev = torch.einsum("tia,ab,tib->t", d, 0.1 * wx, d)
    info = torch.sqrt((gp_pred_sigma_perf + eps_noise).sum(dim=2)).sum(dim=1)
    return (dev - info).sum()
