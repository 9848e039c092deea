"""Reference of the reverse pass of a whole Taylor / mean-equivalent roll-out (sr_multistep_moments_vjp): the reverse sweep over the
H steps, composed from tests/_moments_grad_ref.step_vjp (the reverse of one step's algebra) and the GP link written out in
tests/_reach_rollout_grad_ref.py's docstring, for per-step linearisations the caller supplies.  NumPy only.  np.longdouble by
default; fp64=True runs the same lines in float64 (the rounding floor of a correct fp64 implementation).  Both starts: "point"
(step 0 is the point branch, what sr_multistep_moments computes) and "gauss" (from N(mu_0, sigma_0), step 0 with a zero gain,
what multistep_moments_batch(sigma_0=..., differentiable=True) computes), and the input transform.

    step i reads (mu_{i-1}, Sigma_{i-1}, k_ff_i, k_fb_{i-1}), step 0 (mu_0, sigma_0, K = 0) or the point branch;
    its seed is (w_m[i], w_s[i]) plus the (mux_bar, sigma_bar) step i + 1 produced, and w_v[i] on the GP variances;
    GP link at z_i = [tz mu_{i-1}; k_ff_i]: as in _reach_rollout_grad_ref (jac_bar is zero in mode 2 and at a point: no Hessian term).

The NumPy GP, rollout_inputs (p = mu_0, q = sigma_0, k_ff, k_fb, a, b, w_p = w_m, w_q = w_s; k_fb0, l_mu, l_sigma and c are not
read here) and model_dims are those of _reach_rollout_grad_ref; seed_v() adds the weights on the GP variances.

BARS.  Each gradient is compared relative to its own largest element.  There is no square root and no eigen-gap in these modes:
no trajectory is left out of any bar.
  PROP_RTOL = 30 x WORST_FLOOR, the worst disagreement of the long-double and the fp64 sweep over exactly CASES with the NumPy GP
    standing in (tests/test_moments_rollout_vjp_host.py measures and asserts it).  Measured on x86-64 (80-bit long double): worst
    8.37e-16 (d/dk_ff, the (4, 5) shape, T = 1, H = 5, mode 1 from a Gaussian), so PROP_RTOL = 2.52e-14.
  CHAIN_RTOL = 30 x CHAIN_FLOOR, for the comparison with the chained route (H one-step reverse calls at the states of ITS forward):
    the worst distance over CASES between the fp64 sweep at an fp64 forward and the fp64 sweep at a forward that agrees with it to
    rounding (the long-double forward rounded to fp64), each with the linearisations at its own states -- what two correct fp64
    routes that store two correctly rounded roll-outs can differ by.  Measured: worst 5.75e-12 (d/dk_fb, the (2, 3) shape, T = 65,
    H = 2, mode 2 from a point), so CHAIN_RTOL = 1.74e-10.  It is that far above the other floor because d/dk_fb[0] from a point
    is proportional to Sigma_0 = diag(var), and a GP variance is what is left of sf2 - k^T K^-1 k: two correct fp64 evaluations of
    it differ by 1e-13 and more of its value.
"""
import numpy as np

import _ellipsoid_ref as R
import _moments_grad_ref as MG
import _reach_rollout_grad_ref as RR
from _reach_rollout_grad_ref import NumpyGP, rollout_inputs, model_dims, rel_err, linearisations   # noqa: F401 (re-exported)

LD = np.longdouble
FACTOR = 30.0
WORST_FLOOR = 8.4e-16              # measured (see the docstring), rounded up
PROP_RTOL = FACTOR * WORST_FLOOR
CHAIN_FLOOR = 5.8e-12              # measured (see the docstring), rounded up
CHAIN_RTOL = FACTOR * CHAIN_FLOOR
NAMES = ("mu_0", "sigma_0", "k_ff", "k_fb")
MODES = (1, 2)
STARTS = ("point", "gauss")
# (model key, T, H, mode, start): the (model key, T, H) of _reach_rollout_grad_ref.CASES -- H = 1, 2, 3, 5; T = 1, 65, 257; n_s = 2,
# 4, 5; cart-pole behind Tz; a sparse handle; lin_mat52 -- in both modes from both starts
CASES = tuple((key, T, H, mode, start) for key, T, H in RR.CASES for mode in MODES for start in STARTS)


def seed_v(T, H, n_s, seed=0):
    """the weights w_v (T,H,n_s) on the GP variances the roll-out returns beside its moments"""
    return np.random.default_rng([seed, T, H, n_s, 2424]).standard_normal((T, H, n_s))


def forward(gp, x, H, mode, start, tz=None, dt=LD, t=None):
    """the roll-out of trajectory t (all: t None) over the NumPy GP, everything in dtype dt: mu_all (T,H,n_s), sigma_all
    (T,H,n_s,n_s), var_all (T,H,n_s) of dtype dt.  x as rollout_inputs gives it (entries may already be of dtype dt)."""
    rows = range(x["p"].shape[0]) if t is None else [t]
    n_s, n_u = x["p"].shape[1], x["k_ff"].shape[2]
    ma, sa, va = [], [], []
    for r in rows:
        m = np.asarray(x["p"][r], dtype=dt)
        s = np.asarray(x["q"][r], dtype=dt) if start == "gauss" else None
        if s is not None:
            s = (s + s.T) / 2
        ms, ss, vs = [], [], []
        for i in range(H):
            kfb = np.zeros((n_u, n_s)) if i == 0 else x["k_fb"][r, i - 1]
            mu, var, jm, _, _ = gp.linearize(RR._z(m, x["k_ff"][r, i], tz, dt), dt)
            o = R.step(m, s, x["k_ff"][r, i], kfb, mu, var, RR._jac_state(jm, tz, n_s, dt), None, None, None, x["a"], x["b"],
                       mode=mode, dtype=dt)
            m, s = o["p1"], (o["q1"] + o["q1"].T) / 2
            ms.append(m)
            ss.append(s)
            vs.append(var)
        ma.append(ms)
        sa.append(ss)
        va.append(vs)
    return np.array(ma, dtype=dt), np.array(sa, dtype=dt), np.array(va, dtype=dt)


def sweep(x, H, mode, lins, mu_all, sigma_all, w_m, w_s, w_v, start, tz=None, fp64=False, rows=None):
    """The gradient of sum w_m . mu_all + w_s . sigma_all + w_v . var_all (None = zero) in mu_0, sigma_0, k_ff and k_fb for the
    trajectories `rows` (default: all): dict of float64 arrays under NAMES (sigma_0 None from a point).  lins: (mu, var, jac_mu,
    jac_var, hess_mu), each (T,H,...), at z_i = [tz mu_{i-1}; k_ff_i]; mu_all, sigma_all: what the forward returned."""
    dt = np.float64 if fp64 else LD
    T, n_s = x["p"].shape
    n_u = x["k_ff"].shape[2]
    tzm = np.eye(n_s, dtype=dt) if tz is None else np.asarray(tz, dtype=dt)
    nx = tzm.shape[0]
    rows = list(range(T)) if rows is None else list(rows)
    gauss = start == "gauss"
    res = dict(mu_0=[], sigma_0=[], k_ff=[], k_fb=[])
    mu, var, jm, jv, hm = lins
    pick = lambda w, t, i: None if w is None else w[t, i]
    for t in rows:
        m_bar, s_bar = np.zeros(n_s, dtype=dt), np.zeros((n_s, n_s), dtype=dt)
        g_kff, g_kfb = np.zeros((H, n_u), dtype=dt), np.zeros((max(H - 1, 0), n_u, n_s), dtype=dt)
        for i in range(H - 1, -1, -1):
            m_in = x["p"][t] if i == 0 else mu_all[t, i - 1]
            s_in = (x["q"][t] if gauss else None) if i == 0 else sigma_all[t, i - 1]
            kfb = np.zeros((n_u, n_s)) if i == 0 else x["k_fb"][t, i - 1]
            ws = pick(w_s, t, i)
            sm = m_bar + (0 if w_m is None else np.asarray(w_m[t, i], dtype=dt))
            # (the seed is symmetrised before the carried, exactly symmetric sigma_bar is added)
            ss = s_bar + (0 if ws is None else (np.asarray(ws, dtype=dt) + np.asarray(ws, dtype=dt).T) / 2)
            jmt, jvt, hmt = jm[t, i].astype(dt), jv[t, i].astype(dt), hm[t, i].astype(dt)
            o = MG.step_vjp(m_in, s_in, x["k_ff"][t, i], kfb, mu[t, i], var[t, i], RR._jac_state(jmt, None if tz is None else tzm, n_s, dt),
                            x["a"], x["b"], mode, sm, ss, pick(w_v, t, i), fp64=fp64)
            jz = np.hstack((o["jac_bar"][:, :n_s].dot(tzm.T), o["jac_bar"][:, n_s:]))
            zb = jmt.T.dot(o["mug_bar"]) + jvt.T.dot(o["var_bar"]) + np.einsum('ad,ade->e', jz, hmt)
            m_bar = o["mux_bar"] + tzm.T.dot(zb[:nx])
            g_kff[i] = o["kff_bar"] + zb[nx:]
            s_bar = o["sigma_bar"]
            if i > 0:
                g_kfb[i - 1] = o["kfb_bar"]
        res["mu_0"].append(m_bar)
        res["sigma_0"].append(s_bar)
        res["k_ff"].append(g_kff)
        res["k_fb"].append(g_kfb)
    out = {k: np.array(res[k]).astype(np.float64) for k in ("mu_0", "k_ff", "k_fb")}
    out["sigma_0"] = np.array(res["sigma_0"]).astype(np.float64) if gauss else None
    return out
