"""Reference of the reverse pass of a whole reachability roll-out (sr_multistep_reach_vjp): the reverse sweep over the H steps,
composed from tests/_ellipsoid_grad_ref.step_vjp (the reverse of one step's algebra) and the GP link, for per-step
linearisations the caller supplies.  NumPy only.  np.longdouble by default; fp64=True runs the same lines in float64 (the
rounding floor of a correct fp64 implementation).  Both starts (q_0 None: step 0 is the point branch) and the input transform.

    step i reads (p_{i-1}, q_{i-1}, k_ff_i, k_fb_{i-1}), step 0 (p_0, q_0, k_fb_init) or the point branch;
    its seed is (w_p[i], w_q[i]) plus the (p_bar, q_bar) step i + 1 produced;
    GP link at z_i = [tz p_{i-1}; k_ff_i] with (jac_mu, jac_var, hess_mu) there:
        z_bar = jac_mu^T mu_bar + jac_var^T var_bar + sum_{a,d} jz[a][d] hess_mu[a][d],  jz = [jac_bar[:, :n_s] tz^T, jac_bar[:, n_s:]],
        p_bar += tz^T z_bar[:n_x_in],  kff_bar[i] = b^T p1_bar + z_bar[n_x_in:]
    (the state-space Jacobian the step itself reads is [jac_mu[:, :n_x_in] tz, jac_mu[:, n_x_in:]]).

Also here, for the host test: a small NumPy ARD-RBF GP with its linearisation (mean, variance, both Jacobians, the Hessian of
the mean) in either precision, the forward roll-out over it, and the roll-out cases the GPU test runs (CASES, rollout_inputs), so
that the host test measures the floor on exactly those shapes.

BARS.  Each gradient is compared relative to its own largest element.  PROP_RTOL = 30 x the worst disagreement of the long-double
and the fp64 sweep over CASES x both starts with the NumPy GP standing in (tests/test_reach_rollout_vjp_host.py measures and
asserts it; trajectories with an eigen-gap factor g < G_MIN at any step are left out of the value bars, at most 2 % of a case).
Measured on x86-64 (80-bit long double): worst 6.34e-16 (d/dk_fb_init, the (5, 6) case at T = 1, H = 1), so PROP_RTOL = 1.92e-14.
tests/test_gpu_reach_grad.py measured 1.54e-15 for its own H = 3 roll-out with rounding to fp64 between the steps of its long-double
sweep; this sweep carries its adjoints in long double, and the number is measured here, not carried over.
"""
import numpy as np

import _ellipsoid_ref as R
import _ellipsoid_grad_ref as G

LD = np.longdouble
G_MIN = G.G_MIN
FACTOR = 30.0
WORST_FLOOR = 6.4e-16              # measured (see the docstring), rounded up
PROP_RTOL = FACTOR * WORST_FLOOR
NAMES = ("p_0", "q_0", "k_fb_init", "k_ff", "k_fb")

# (model key, T, H): the roll-outs of the GPU test, each from a point and from (q_0, k_fb_init).  H = 1, 2, 3, 5; T = 1, 65 (past
# one 64-thread workgroup), 257 (past 256); the model keys are resolved by the GPU test (MODELS there) and by model_dims below.
CASES = (("rbf23_150", 257, 3), ("rbf23_150", 1, 1), ("rbf23_150", 65, 2), ("rbf23_150", 65, 5), ("rbf23_600", 65, 2),
         ("rbf45", 257, 3), ("rbf45", 1, 5), ("linmat52_23", 65, 3), ("cartpole", 65, 3), ("sparse23", 65, 2),
         ("rbf56", 65, 3), ("rbf56", 1, 1))
CARTPOLE_TZ = np.eye(4)[1:]        # the cart position is not a GP input


def model_dims(key):
    """(n_s, n_u, tz) of a model key of CASES"""
    return dict(rbf23_150=(2, 1, None), rbf23_600=(2, 1, None), rbf45=(4, 1, None), linmat52_23=(2, 1, None),
                cartpole=(4, 1, CARTPOLE_TZ), sparse23=(2, 1, None), rbf56=(5, 1, None))[key]


def rollout_inputs(n_s, n_u, T, H, seed=0):
    """the inputs of one roll-out case and the weights w_p, w_q (not symmetric) of the functional that is differentiated"""
    rng = np.random.default_rng([seed, n_s, n_u, T, H, 2222])
    A = rng.standard_normal((T, n_s, n_s))
    return dict(p=0.3 * rng.standard_normal((T, n_s)), q=0.02 * np.einsum('tij,tkj->tik', A, A) / n_s,
                k_fb0=0.3 * rng.standard_normal((T, n_u, n_s)), k_ff=0.2 * rng.standard_normal((T, H, n_u)),
                k_fb=0.3 * rng.standard_normal((T, H - 1, n_u, n_s)),
                a=0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
                l_mu=rng.uniform(0.01, 0.05, n_s), l_sigma=rng.uniform(0.01, 0.05, n_s), c=R.C_SAFETY,
                w_p=rng.standard_normal((T, H, n_s)), w_q=rng.standard_normal((T, H, n_s, n_s)))


# ---- a NumPy ARD-RBF GP standing in for the device model ------------------------------------------------------------------------
class NumpyGP(object):
    """n_out independent ARD-RBF GPs on D inputs, fitted in fp64; linearize(z, dt) evaluates in dtype dt"""

    def __init__(self, n_out, D, N, seed=0, noise=1e-2):
        rng = np.random.default_rng([seed, n_out, D, N])
        self.Z = rng.uniform(-1, 1, (N, D))
        W = rng.standard_normal((n_out, D)) / np.sqrt(D)
        Y = np.sin(2.0 * self.Z.dot(W.T)) + 0.05 * rng.standard_normal((N, n_out))
        self.ls = rng.uniform(0.8, 1.6, (n_out, D)) * np.sqrt(D / 3.0)
        self.sf2 = rng.uniform(0.5, 1.5, n_out)
        self.n_out, self.D = n_out, D
        self.kinv, self.alpha = [], []
        for o in range(n_out):
            d = (self.Z[:, None, :] - self.Z[None, :, :]) / self.ls[o]
            K = self.sf2[o] * np.exp(-0.5 * (d * d).sum(-1)) + noise * np.eye(N)
            Ki = np.linalg.inv(K)
            self.kinv.append((Ki + Ki.T) / 2)
            self.alpha.append(Ki.dot(Y[:, o]))

    def linearize(self, z, dt=np.float64):
        """one input z (D,): mu (n,), var (n,), jac_mu (n,D), jac_var (n,D), hess_mu (n,D,D)"""
        z, Z = np.asarray(z, dtype=dt), self.Z.astype(dt)
        n, D = self.n_out, self.D
        mu, var = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
        jm, jv, hm = np.zeros((n, D), dtype=dt), np.zeros((n, D), dtype=dt), np.zeros((n, D, D), dtype=dt)
        for o in range(n):
            il2 = 1 / (self.ls[o].astype(dt) ** 2)
            diff = Z - z                                        # (N, D)
            k = dt(self.sf2[o]) * np.exp(-(diff * diff * il2).sum(-1) / 2)
            dk = k[:, None] * diff * il2                        # d k_n / d z_e
            al, Ki = self.alpha[o].astype(dt), self.kinv[o].astype(dt)
            mu[o] = k.dot(al)
            jm[o] = dk.T.dot(al)
            u = diff * il2
            hm[o] = np.einsum('n,nd,ne->de', al * k, u, u) - np.diag(il2) * (al * k).sum()
            kk = Ki.dot(k)
            var[o] = dt(self.sf2[o]) - k.dot(kk)
            jv[o] = -2 * dk.T.dot(kk)
        return mu, var, jm, jv, hm


def _z(p, k_ff, tz, dt):
    p = np.asarray(p, dtype=dt)
    return np.concatenate((p if tz is None else np.asarray(tz, dtype=dt).dot(p), np.asarray(k_ff, dtype=dt)))


def _jac_state(jm, tz, n_s, dt):
    if tz is None:
        return jm
    tzm = np.asarray(tz, dtype=dt)
    nx = tzm.shape[0]
    return np.hstack((jm[:, :nx].dot(tzm), jm[:, nx:]))


def forward(gp, x, H, start_q, tz=None, dt=LD, t=None):
    """the roll-out of trajectory t (all: t None) over the NumPy GP, everything in dtype dt.  x as rollout_inputs gives it
    (entries may already be of dtype dt: the finite-difference check perturbs them).  Returns p_all (T,H,n_s), q_all
    (T,H,n_s,n_s) of dtype dt."""
    rows = range(x["p"].shape[0]) if t is None else [t]
    n_s = x["p"].shape[1]
    pa, qa = [], []
    for r in rows:
        p, q = np.asarray(x["p"][r], dtype=dt), (np.asarray(x["q"][r], dtype=dt) if start_q else None)
        if q is not None:
            q = (q + q.T) / 2
        ps, qs = [], []
        for i in range(H):
            kfb = (x["k_fb0"][r] if start_q else None) if i == 0 else x["k_fb"][r, i - 1]
            mu, var, jm, _, _ = gp.linearize(_z(p, x["k_ff"][r, i], tz, dt), dt)
            o = R.step(p, q, x["k_ff"][r, i], kfb if q is not None else np.zeros((x["k_ff"].shape[2], n_s)), mu, var,
                       _jac_state(jm, tz, n_s, dt), x["l_mu"], x["l_sigma"], x["c"], x["a"], x["b"])
            p, q = o["p1"], (o["q1"] + o["q1"].T) / 2
            ps.append(p)
            qs.append(q)
        pa.append(ps)
        qa.append(qs)
    return np.array(pa, dtype=dt), np.array(qa, dtype=dt)


def linearisations(gp, x, p_all, H, tz=None, dt=np.float64):
    """(mu, var, jac_mu, jac_var, hess_mu), each (T,H,...), of the NumPy GP at z_i = [tz p_{i-1}; k_ff_i]"""
    T = x["p"].shape[0]
    outs = [[gp.linearize(_z(x["p"][t] if i == 0 else p_all[t, i - 1], x["k_ff"][t, i], tz, dt), dt) for i in range(H)]
            for t in range(T)]
    return tuple(np.array([[outs[t][i][k] for i in range(H)] for t in range(T)]) for k in range(5))


# ---- the sweep ------------------------------------------------------------------------------------------------------------------
def sweep(x, H, lins, p_all, q_all, w_p, w_q, start_q, tz=None, fp64=False, rows=None):
    """The gradient of sum w_p . p_all + w_q . q_all (None = zero) in p_0, (q_0, k_fb_init), k_ff and k_fb for the trajectories
    `rows` (default: all): dict of float64 arrays under NAMES (q_0, k_fb_init None from a point), `g` (rows,) the smallest
    eigen-gap factor over the steps of a trajectory, `bad` (rows, H).  lins: (mu, var, jac_mu, jac_var, hess_mu), each (T,H,...);
    p_all, q_all: what the forward returned."""
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
            o = G.step_vjp(p_in, q_in, x["k_ff"][t, i], kfb, mu[t, i], var[t, i], _jac_state(jmt, None if tz is None else tzm, n_s, dt),
                           x["l_mu"], x["l_sigma"], x["c"], x["a"], x["b"], sp, sq, fp64=fp64)
            jz = np.hstack((o["jac_bar"][:, :n_s].dot(tzm.T), o["jac_bar"][:, n_s:]))
            zb = jmt.T.dot(o["mu_bar"]) + jvt.T.dot(o["var_bar"]) + np.einsum('ad,ade->e', jz, hmt)
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


def rel_err(got, want, keep=None):
    """largest |got - want| over the kept trajectories, relative to the largest kept element of want (0 for an empty array)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if keep is not None:
        got, want = got[keep], want[keep]
    if want.size == 0:
        return 0.0
    scale = np.abs(want).max()
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - want).max() / scale) if scale > 0 else (0.0 if not np.abs(got).max() else np.inf)
