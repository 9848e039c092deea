"""Long-double reference of a whole multi-step chain (sr_multistep_reach, sr_multistep_moments): the GP posterior and the
ellipsoid / moment step composed over H steps, from what the suite already trusts -- the long-double algebra of
tests/_posterior_ref.py (cholesky_ld, solve_lower_ld, solve_upper_ld, kernel_ld) for a DENSE ARD-RBF fit at N <= 512 and
tests/_ellipsoid_ref.step for modes 0 (ellipsoids, from a point or from (q0, k_fb0)), 1 (Taylor moments) and 2 (mean-equivalent
moments).  NumPy only: no GPU, no torch, no SciPy.  The shape matrix is symmetrised between steps, as
tests/_reach_rollout_grad_ref.forward does.  The diagonal term of the fit is noise + 1e-5 + 1e-8, as in _posterior_ref.

The centres do not depend on the shape matrices (p_{i+1} = a p_i + b u_i + mu(p_i, u_i)), so a chain is evaluated in two
passes: rollout() moves the centres and records (mu, sigma^2 = sf2 - |L^-1 k*|^2, d mu / dx) of every step, all checked roll-outs
(and all perturbed copies of them) as ONE right-hand side per step and output; chain() then runs the step algebra of one
variant ("point", "q0": mode 0 from a point / from (q0, k_fb0); "m1", "m2": the moment modes) over the recorded outputs.

THREE RUNS of the same lines:
    long double          the reference;
    float64 (the twin)   FLOOR = |twin - long double|: what a correct fp64 implementation may differ by;
    perturbed            long double with EVERY GP output of EVERY step displaced by its accepted accuracy, in four sign
                         patterns (all plus, all minus, two seeded random ones): RESP = |perturbed - unperturbed|, the response
                         of the chain to errors the posterior tests accept.  Displacements: mu and d mu / dx by the smaller of
                         (3 N + 40) u kappa magnitude (the a-priori bar of _posterior_ref with b = N, kappa = cond_2(K)) and the
                         project's 1e-12 sigma_f |alpha|_1; sigma^2 by the smaller of (3 N + 40) u kappa sf2 and 1e-9 sf2.
BAR, per case, variant, quantity (p, q, gp_var) and step, absolute on every element:
    bar = 30 x floor + 2 x resp
floor and resp the largest over the checked roll-outs and elements of that step.  30 is the factor of the project's other
floor-based bars (_reach_rollout_grad_ref.FACTOR); 2 because the displacements are worst-case bounds already while the signs
of real per-step errors need not match a tested pattern.  Nothing of it comes from a device.

DATA.  The recipe of the existing chain test (oracle_np.make_synthetic: Z ~ U[-1, 1]^D, y = sin(2 z . w) + 0.05 randn,
l ~ U[0.5, 1.5], sf2 = 1; inputs and the contracting a = 0.6 I + 0.03 randn of test_persistent_chain_matches_per_step_launches),
changed where a condition of tests/test_chain_ref_host.py asked for it, each time on the reference's numbers alone:
  * noise 0.1.  With 0.01 (and 0.05) |alpha|_1 reaches 1.9e4 at N = 511, the accepted error of the mean 1e-12 sigma_f |alpha|_1
    moves the centres by 2.5e-7 (1.6e-7) of their largest element within 5 steps, and the bar leaves what the existing test grants;
  * w ~ N(0, 1 / D) and y scaled by Y_GAIN = 0.15: the spectral radius of a + d mu / dx stays below 1.  With |d mu / dx| ~ 1 the
    ellipsoids of mode 0 at n_s = 4 pass 1e24 within 20 steps; beyond 16 steps a = 0.3 I + 0.03 randn for the same reason;
  * models of fewer than 32 points (N = Np - 127 = 1) draw Z from 0.3 U[-1, 1]^D, where the roll-outs start: with one training
    point anywhere in the cube the median sigma^2 stays at 0.73 k(x,x).

MEASURED on x86-64 (80-bit long double) by tests/test_chain_ref_host.py (pytest -s prints every case), worst over all_cases(),
relative to the largest element of the quantity at that step (gp_var: relative to sf2):
    mode 0 (point, q0)   p: floor 3.2e-14, resp 2.0e-9      q: floor 1.1e-13, resp 1.2e-7
    mode 1               p: floor 4.0e-14, resp 2.0e-9      q: floor 1.1e-13, resp 1.2e-7     gp_var: floor 1.0e-15, resp 4.5e-10
    mode 2               p: floor 3.2e-14, resp 2.0e-9      q: floor 1.1e-13, resp 1.1e-7     gp_var: floor 7.6e-16, resp 4.5e-10
so the worst bars are 4.0e-9 (p), 2.4e-7 (q) and 9.1e-10 (gp_var): the response to the accepted errors of the posterior
dominates every one.  The MI355X used at most 3 % of a bar (the models of one training point, whose bars are a few 1e-14 of the
largest element) and less than 0.05 % of any other.
"""
import numpy as np

import _ellipsoid_ref as R
import _posterior_ref as P

LD = np.longdouble
U53 = P.U53
FACTOR_FLOOR, FACTOR_RESP = 30.0, 2.0
P_LIMIT, Q_LIMIT = 1e-7, 1e-6          # what test_persistent_chain_matches_per_step_launches grants against the fp64 oracle
VARIANTS = ("point", "q0", "m1", "m2")
MODE = dict(point=0, q0=0, m1=1, m2=2)
C_SAFETY = 2.0
NOISE = 0.1
Y_GAIN = 0.15                          # spectral radius of d mu / dx ~ 0.3: with a = 0.6 I the tubes of mode 0 stay bounded over H_max = 38 steps
GROUP = 16                             # roll-outs per group of the persistent kernel
CHAIN_GROUPS, CHAIN_XELS, FUSED_T = 240, 240 * 112 * 96, 1024
NOMINAL_CUS = 256                      # MI355X; the GPU test asks the device


# ---- the launch arithmetic of try_chain (csrc/sr_capi_chain.hip), restated from its documentation ---------------------------------
def padded(N):
    return -(-N // 128) * 128


def wgs_per_group(Np, n_s):
    return n_s * (Np // 128) + (1 if (n_s > 1 or Np > 128) else 0)


def gmax(Np, n_s, n_u, H, cus=NOMINAL_CUS):
    """groups of 16 roll-outs one launch holds: min(240, CUs - 16) // workgroups per group, and the exchange-element bound"""
    xpg = H * n_s * (GROUP * (n_s + n_u + 1) + GROUP * (Np // 128))
    return max(1, min(min(CHAIN_GROUPS, cus - 16) // wgs_per_group(Np, n_s), CHAIN_XELS // xpg))


def launches(T, Np, n_s, n_u, H, cus=NOMINAL_CUS):
    g = gmax(Np, n_s, n_u, H, cus)
    return (-(-T // GROUP) + g - 1) // g


def max_launches(T, H):
    return 1 if H <= 2 else (6 if T > FUSED_T else 2)


def h_max(n_s, n_u):
    """the longest chain whose control sequence fits the LDS control block"""
    return 24576 // (128 * (n_u + n_u * n_s))


# ---- models ---------------------------------------------------------------------------------------------------------------------
class Model(object):
    """training data and hyper-parameters of one (n_s, n_u, N, seed); tz (n_x_in, n_s) or None is the input transform"""

    def __init__(self, n_s, n_u, N, seed=0, tz=None):
        rng = np.random.default_rng([seed, n_s, n_u, N, 4711])
        nx = n_s if tz is None else tz.shape[0]
        D = nx + n_u
        self.n_s, self.n_u, self.N, self.D, self.nx, self.seed, self.tz = n_s, n_u, N, D, nx, seed, tz
        self.Z = rng.uniform(-1, 1, (N, D)) * (0.3 if N < 32 else 1.0)
        W = rng.standard_normal((n_s, D)) / np.sqrt(D)
        self.Y = Y_GAIN * (np.sin(2.0 * self.Z.dot(W.T)) + 0.05 * rng.standard_normal((N, n_s)))
        self.ls = rng.uniform(0.5, 1.5, (n_s, D))
        self.sf2 = np.ones(n_s)
        self.noise = np.full(n_s, NOISE)                                 # noise_variance of the hyp list
        self.nugget = self.noise + P.NOISE_DIAG + P.GPY_JITTER
        self.Np = padded(N)
        self._fit = {}

    @classmethod
    def from_arrays(cls, Z, Y, ls, sf2, nugget, n_u, tz=None):
        """a model of given data; nugget: the whole diagonal term per output"""
        m = cls.__new__(cls)
        m.Z, m.Y, m.ls, m.sf2, m.nugget = (np.asarray(v, dtype=np.float64) for v in (Z, Y, ls, sf2, nugget))
        m.N, m.D = m.Z.shape
        m.n_s, m.n_u, m.tz, m.seed = m.Y.shape[1], n_u, tz, 0
        m.nx = m.D - n_u
        m.noise = m.nugget - P.NOISE_DIAG - P.GPY_JITTER
        m.Np, m._fit = padded(m.N), {}
        return m

    @property
    def hyp(self):
        return [{"lengthscale": self.ls[d].copy(), "variance": float(self.sf2[d]), "noise_variance": float(self.noise[d])}
                for d in range(self.n_s)]

    def fit(self, dt=LD):
        """(L, alpha) per output in dtype dt, and (float64) kappa = cond_2(K), a1 = |alpha|_1; cached"""
        if dt not in self._fit:
            Ls, als, kap, a1 = [], [], [], []
            for d in range(self.n_s):
                k, _ = P.kernel_ld("rbf", self.Z, self.Z, self.ls[d], self.sf2[d], dt)
                k = (k + k.T) / 2 + dt(self.nugget[d]) * np.eye(self.N, dtype=dt)
                l = P.cholesky_ld(k, dt)
                y = np.asarray(self.Y[:, d], dtype=dt)[:, None]
                al = P.solve_upper_ld(l, P.solve_lower_ld(l, y, dt), dt)[:, 0]
                ev = np.linalg.eigvalsh(k.astype(np.float64))
                Ls.append(l)
                als.append(al)
                kap.append(float(ev[-1] / ev[0]))
                a1.append(float(np.abs(al).sum()))
            self._fit[dt] = (Ls, als, np.array(kap), np.array(a1))
        return self._fit[dt]

    def posterior(self, X, dt=LD, want_v=False):
        """X (R, D) GP inputs -> mu, var (R, n_s), jac (R, n_s, D) in dtype dt, and the displacements d_mu, d_var, d_jac
        (float64) of the perturbed run; want_v: also v = L^-1 k* (n_s, N, R) for the coverage condition"""
        Ls, als, kap, a1 = self.fit(dt)
        R_, n, D = X.shape[0], self.n_s, self.D
        mu, var, jac = np.empty((R_, n), dtype=dt), np.empty((R_, n), dtype=dt), np.empty((R_, n, D), dtype=dt)
        d_mu, d_var, d_jac = np.empty((R_, n)), np.empty((R_, n)), np.empty((R_, n, D))
        vs = []
        xq, z = np.asarray(X, dtype=dt), np.asarray(self.Z, dtype=dt)
        for d in range(n):
            k, g = P.kernel_ld("rbf", xq, z, self.ls[d], self.sf2[d], dt)            # (R, N)
            v = P.solve_lower_ld(Ls[d], k.T, dt)                                      # (N, R): one right-hand side
            l2 = np.asarray(self.ls[d], dtype=dt) ** 2
            dx = (xq[:, None, :] - z[None, :, :]) / l2[None, None, :]                 # (R, N, D)
            ga = g * als[d][None, :]
            mu[:, d] = k.dot(als[d])
            var[:, d] = dt(self.sf2[d]) - np.sum(v * v, axis=0)
            jac[:, d] = np.einsum("rn,rnj->rj", ga, dx)
            c = (3 * self.N + 40) * U53 * kap[d]
            old = 1e-12 * np.sqrt(self.sf2[d]) * a1[d]
            d_mu[:, d] = np.minimum(c * np.abs(k).dot(np.abs(als[d])).astype(np.float64), old)
            d_jac[:, d] = np.minimum(c * np.einsum("rn,rnj->rj", np.abs(ga), np.abs(dx)).astype(np.float64), old)
            d_var[:, d] = min(c * self.sf2[d], 1e-9 * self.sf2[d])
            if want_v:
                vs.append(v.astype(np.float64))
        return (mu, var, jac, d_mu, d_var, d_jac) + ((np.array(vs),) if want_v else ())


_MODELS = {}


def model(n_s, n_u, N, seed=0, tz=None):
    key = (n_s, n_u, N, seed, None if tz is None else tz.tobytes())
    if key not in _MODELS:
        _MODELS[key] = Model(n_s, n_u, N, seed, tz)
    return _MODELS[key]


def inputs(n_s, n_u, T, H, seed=0):
    """the inputs of T roll-outs of H steps (the recipe of test_persistent_chain_matches_per_step_launches); row t is drawn
    from (seed, t) alone, so that roll-out t is the same whatever T"""
    out = dict(p=np.empty((T, n_s)), q=np.empty((T, n_s, n_s)), k_fb0=np.empty((T, n_u, n_s)), k_ff=np.empty((T, H, n_u)),
               k_fb=np.empty((T, max(H - 1, 0), n_u, n_s)))
    for t in range(T):
        rng = np.random.default_rng([seed, n_s, n_u, H, t, 99])
        A = rng.standard_normal((n_s, n_s))
        out["p"][t], out["q"][t] = 0.3 * rng.standard_normal(n_s), 0.01 * A.dot(A.T) + 0.01 * np.eye(n_s)
        out["k_fb0"][t], out["k_ff"][t] = 0.1 * rng.standard_normal((n_u, n_s)), 0.3 * rng.standard_normal((H, n_u))
        out["k_fb"][t] = 0.1 * rng.standard_normal((max(H - 1, 0), n_u, n_s))
    rng = np.random.default_rng([seed, n_s, n_u, 98])
    # |a| = 0.6 up to 16 steps; 0.3 beyond: the tubes of mode 0 at n_s = 4 grow past 1e24 within 20 steps otherwise
    out.update(a=(0.6 if H <= 16 else 0.3) * np.eye(n_s) + 0.03 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
               l_mu=np.linspace(0.005, 0.008, n_s), l_sigma=np.linspace(0.002, 0.003, n_s), c=C_SAFETY)
    return out


# ---- the two passes ---------------------------------------------------------------------------------------------------------------
def sign_patterns(R_, H, n_s, D, seed=0):
    """[None (unperturbed), all plus, all minus, two seeded random ones]: each (s_mu (R,H,n_s), s_var (R,H,n_s), s_jac (R,H,n_s,D))"""
    one = (np.ones((R_, H, n_s)), np.ones((R_, H, n_s)), np.ones((R_, H, n_s, D)))
    out = [None, one, tuple(-s for s in one)]
    for k in (1, 2):
        rng = np.random.default_rng([seed, k, R_, H, 555])
        out.append(tuple(rng.choice((-1.0, 1.0), s.shape) for s in one))
    return out


def rollout(m, x, H, rows, dt=LD, patterns=(None,), want_v=False):
    """The centres of the roll-outs `rows` and the GP outputs of every step, for every sign pattern of `patterns` at once.
    Returns dict(p (S,R,H,n_s), mu, var (S,R,H,n_s), jac (S,R,H,n_s,n_s+n_u) in state space), dtype dt; with want_v also
    v (H, n_s, N, S R) float64."""
    rows = np.asarray(rows)
    S, R_, n_s, n_u = len(patterns), len(rows), m.n_s, m.n_u
    a, b = np.asarray(x["a"], dtype=dt), np.asarray(x["b"], dtype=dt)
    tz = None if m.tz is None else np.asarray(m.tz, dtype=dt)
    p = np.broadcast_to(np.asarray(x["p"][rows], dtype=dt), (S, R_, n_s)).reshape(S * R_, n_s)
    out = dict(p=np.empty((S, R_, H, n_s), dtype=dt), mu=np.empty((S, R_, H, n_s), dtype=dt), var=np.empty((S, R_, H, n_s), dtype=dt),
               jac=np.empty((S, R_, H, n_s, n_s + n_u), dtype=dt), v=[])
    for i in range(H):
        u = np.broadcast_to(np.asarray(x["k_ff"][rows, i], dtype=dt), (S, R_, n_u)).reshape(S * R_, n_u)
        X = np.hstack((p if tz is None else p.dot(tz.T), u))
        res = m.posterior(X, dt, want_v)
        mu, var, jac = (r.reshape((S, R_) + r.shape[1:]).copy() for r in res[:3])
        d_mu, d_var, d_jac = (r.reshape((S, R_) + r.shape[1:]) for r in res[3:6])
        for s, pat in enumerate(patterns):
            if pat is not None:
                mu[s] += np.asarray(pat[0][:, i] * d_mu[s], dtype=dt)
                var[s] += np.asarray(pat[1][:, i] * d_var[s], dtype=dt)
                jac[s] += np.asarray(pat[2][:, i] * d_jac[s], dtype=dt)
        if tz is not None:                                               # the Jacobian the step reads is in state space
            jac = np.concatenate((np.einsum("srdx,xj->srdj", jac[..., :m.nx], tz), jac[..., m.nx:]), axis=-1)
        p = p.dot(a.T) + u.dot(b.T) + mu.reshape(S * R_, n_s)
        out["p"][:, :, i], out["mu"][:, :, i], out["var"][:, :, i], out["jac"][:, :, i] = p.reshape(S, R_, n_s), mu, var, jac
        if want_v:
            out["v"].append(res[6])
    return out


def chain(m, x, H, rows, variant, ro, s=0, dt=LD):
    """the step algebra of one variant over the recorded GP outputs of pattern s: p_all (R,H,n_s), q_all (R,H,n_s,n_s),
    var_all (R,H,n_s), dtype dt"""
    mode, n_s, n_u = MODE[variant], m.n_s, m.n_u
    pa, qa = np.empty((len(rows), H, n_s), dtype=dt), np.empty((len(rows), H, n_s, n_s), dtype=dt)
    for r, t in enumerate(rows):
        p, q = np.asarray(x["p"][t], dtype=dt), None
        if variant == "q0":
            q = np.asarray(x["q"][t], dtype=dt)
            q = (q + q.T) / 2
        for i in range(H):
            kfb = (x["k_fb0"][t] if variant == "q0" else np.zeros((n_u, n_s))) if i == 0 else x["k_fb"][t, i - 1]
            o = R.step(p, q, x["k_ff"][t, i], kfb, ro["mu"][s, r, i], ro["var"][s, r, i], ro["jac"][s, r, i], x["l_mu"],
                       x["l_sigma"], x["c"], x["a"], x["b"], mode, dt)
            assert not o["bad"], "the remainder boxes of the reference must be positive"
            p, q = o["p1"], (o["q1"] + o["q1"].T) / 2
            pa[r, i], qa[r, i] = p, q
    return pa, qa, ro["var"][s]


_ROLL = {}


def _rollouts(m, x, H, rows, key):
    """(long-double roll-out of all five patterns, fp64 twin) of one (model, inputs, rows); cached under key"""
    if key not in _ROLL:
        pats = sign_patterns(len(rows), H, m.n_s, m.D, m.seed)
        _ROLL[key] = (rollout(m, x, H, rows, LD, pats), rollout(m, x, H, rows, np.float64))
        if len(_ROLL) > 8:
            _ROLL.pop(next(iter(_ROLL)))
    return _ROLL[key]


def reference(m, x, H, rows, variant, key=None):
    """What a device chain is held to on the roll-outs `rows`: dict(p, q, var (float64, rounded from long double),
    floor_p, floor_q, floor_var, resp_p, resp_q, resp_var, bar_p, bar_q, bar_var (each (H,)), scale_p, scale_q (H,): the
    largest element of the quantity at that step)."""
    rows = list(rows)
    key = (id(m), id(x), H, tuple(rows)) if key is None else key
    ld, tw = _rollouts(m, x, H, rows, key)
    want = chain(m, x, H, rows, variant, ld, 0, LD)
    twin = chain(m, x, H, rows, variant, tw, 0, np.float64)
    pert = [chain(m, x, H, rows, variant, ld, s, LD) for s in range(1, 5)]
    out = {}
    for k, name in enumerate(("p", "q", "var")):
        w = np.asarray(want[k])
        red = tuple(a for a in range(w.ndim) if a != 1)
        assert np.all(np.isfinite(w.astype(np.float64))), "the reference trajectory left the finite range"
        floor = np.abs(np.asarray(twin[k], dtype=LD) - w).max(axis=red).astype(np.float64)
        resp = np.max([np.abs(pt[k] - w).max(axis=red) for pt in pert], axis=0).astype(np.float64)
        out[name] = w.astype(np.float64)
        out["floor_" + name], out["resp_" + name] = floor, resp
        out["bar_" + name] = FACTOR_FLOOR * floor + FACTOR_RESP * resp
        out["scale_" + name] = np.abs(w).max(axis=red).astype(np.float64)
    return out


def part_rows(Np, part):
    """the 128 rows of U^-T k* (padded indices) that workgroup `part` of an output contracts: strips 4 part + j and
    Np / 16 - 1 - (4 part + j), j < 4, of 16 rows each (sr_flat_geo of csrc/sr_chain.hip)"""
    strips = [4 * part + j for j in range(4)] + [Np // 16 - 1 - (4 * part + j) for j in range(4)]
    return np.concatenate([np.arange(16 * s, 16 * s + 16) for s in strips])


def data_conditions(m, x, H, rows):
    """the conditions of a case that mean something only on its data, decided on the fp64 twin of the reference alone: returns
    dict(ratio: median sigma^2 / k(x,x), coverage: for every (output, part) the largest relative change of sigma^2 over the
    checked queries when the part's share of |U^-T k*|^2 is dropped (n_s, parts))"""
    ro = rollout(m, x, H, rows, np.float64, want_v=True)
    var = ro["var"][0].astype(np.float64)                               # (R, H, n_s)
    off, parts = m.Np - m.N, m.Np // 128
    cov = np.zeros((m.n_s, parts))
    for i in range(H):
        v2 = np.zeros((m.n_s, m.Np, len(rows)))
        v2[:, off:] = ro["v"][i] ** 2
        for part in range(parts):
            share = v2[:, part_rows(m.Np, part)].sum(axis=1)            # (n_s, R)
            cov[:, part] = np.maximum(cov[:, part], (share / var[:, i].T).max(axis=1))
    return dict(ratio=float(np.median(var / m.sf2[None, None, :])), coverage=cov)


# ---- the case table: shared by tests/test_chain_ref_host.py and tests/test_gpu_chain_family.py ------------------------------------
PAIRS = ((1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (3, 2))
NPS = (128, 256, 384, 512)
T_FAMILY, H_FAMILY = 17, 5


def family():
    """the 24 instantiations: (id, n_s, n_u, N) with N = Np - 1 (least front padding) for half of them and Np - 127 (most) for
    the other half, alternating so that every Np and every pair sees both"""
    out = []
    for i, Np in enumerate(NPS):
        for j, (n_s, n_u) in enumerate(PAIRS):
            N = Np - 1 if (i + j) % 2 == 0 else Np - 127
            out.append(("Np%d-ns%d-nu%d-N%d" % (Np, n_s, n_u, N), n_s, n_u, N))
    return out


EDGE_MODELS = ((2, 1, 200), (4, 1, 511))           # (n_s, n_u, N): Np = 256 and Np = 512


def edge_rows(T, per_launch):
    """the roll-outs of a batch that are checked against the reference: the first group, the last group, and the first
    roll-out of the second launch"""
    rows = set(range(min(T, GROUP))) | set(range((T - 1) // GROUP * GROUP, T))
    if T > per_launch:
        rows.add(per_launch)
    return sorted(rows)


def edge_cases(n_s, n_u, N, cus=NOMINAL_CUS):
    """(T, H, variant, chain expected) of the group and launch edges of one model on a device of `cus` CUs"""
    Np = padded(N)
    g3, g2 = gmax(Np, n_s, n_u, 3, cus), gmax(Np, n_s, n_u, 2, cus)
    out = [(1, 3, "point", True), (15, 3, "m1", True), (16, 3, "q0", True), (17, 1, "m2", True), (17, 2, "q0", True),
           (17, 1, "point", True), (16 * g3, 3, "point", True), (16 * g3 + 1, 3, "m1", True), (16 * g2 + 1, 2, "point", False)]
    if 32 * g3 + 1 <= FUSED_T:
        out.append((32 * g3 + 1, 3, "q0", False))
    return out


HMAX_MODELS = ((3, 2, 255), (4, 1, 129))          # H_max = 24 and 38; both Np = 256
HMAX_VARIANTS = (("q0", 0), ("m1", 0), ("point", 1), ("m2", 1))        # (variant, H - H_max): persistent at H_max, per-step beyond


def per_step_cases():
    """(id, n_s, n_u, N, tz, T, H, chunk, variants): the per-step route where the persistent kernel never applies"""
    from _reach_rollout_grad_ref import CARTPOLE_TZ
    return (("N600", 2, 1, 600, None, 17, 5, None, ("point", "m1", "m2")),
            ("N600-chunk16", 2, 1, 600, None, 40, 4, 16, ("q0", "m1", "m2")),
            ("cartpole-tz", 4, 1, 200, CARTPOLE_TZ, 33, 5, None, ("q0", "m1", "m2")))


REFIT = ((2, 1, 200), 100, "m1", 5, 17)    # fit, release_scratch, 100 more rows on the same handle (Np 256 -> 384), then (variant, H, T)


def refit_model():
    """the model of REFIT after its growth: the rows of model(2, 1, 200) and behind them the first 100 of model(2, 1, 300)"""
    (n_s, n_u, N0), more, _, _, _ = REFIT
    if "refit" not in _MODELS:
        m0, m1 = model(n_s, n_u, N0), model(n_s, n_u, N0 + more)
        _MODELS["refit"] = Model.from_arrays(np.vstack((m0.Z, m1.Z[:more])), np.vstack((m0.Y, m1.Y[:more])), m0.ls, m0.sf2, m0.nugget, n_u)
    return _MODELS["refit"]


def all_cases(cus=NOMINAL_CUS):
    """every (id, model, T, H, variant, rows) that a GPU test compares with the reference, for a device of `cus` CUs"""
    out = []
    for cid, n_s, n_u, N in family():
        out += [(cid + "-" + v, model(n_s, n_u, N), T_FAMILY, H_FAMILY, v, list(range(T_FAMILY))) for v in VARIANTS]
    for n_s, n_u, N in EDGE_MODELS:
        for T, H, v, _ in edge_cases(n_s, n_u, N, cus):
            per = GROUP * gmax(padded(N), n_s, n_u, H, cus)
            out.append(("edge-ns%d-N%d-T%d-H%d-%s" % (n_s, N, T, H, v), model(n_s, n_u, N), T, H, v, edge_rows(T, per)))
    for n_s, n_u, N in HMAX_MODELS:
        for v, dh in HMAX_VARIANTS:
            H = h_max(n_s, n_u) + dh
            out.append(("hmax-ns%d-nu%d-H%d-%s" % (n_s, n_u, H, v), model(n_s, n_u, N), T_FAMILY, H, v, list(range(T_FAMILY))))
    for v, H, T in STATE_SEQUENCE[:3]:
        out.append(("state-%s-H%d-T%d" % (v, H, T), model(2, 1, 200), T, H, v, list(range(T))))
    for v, H, T in STALE_SEQUENCE[:1] + STALE_SEQUENCE[2:]:
        out.append(("tags-%s-H%d-T%d" % (v, H, T), model(2, 1, 200), T, H, v, list(range(T))))
    _, _, v, H, T = REFIT
    out.append(("refit-N%d-%s" % (refit_model().N, v), refit_model(), T, H, v, list(range(T))))
    for cid, n_s, n_u, N, tz, T, H, _, variants in per_step_cases():
        out += [(cid + "-" + v, model(n_s, n_u, N, tz=tz), T, H, v, list(range(min(T, 48)))) for v in variants]
    return out


STATE_SEQUENCE = (("point", 7, 40), ("m1", 3, 17), ("m2", 12, 5), ("point", 7, 40))     # (variant, H, T) on one handle
# a sequence after which, with tags that count per group only, the second group's slots of the last call still hold the first
# call's elements under exactly the tags the last call waits for (slot (g H + i), tag epoch[g] + i + 1: the first call leaves tag
# s + 1 in slot s < 12, the two H = 2 calls move epoch[1] to 4, and group 1 of the H = 4 call reads slots 4 .. 7 for tags 5 .. 8)
STALE_SEQUENCE = (("m1", 12, 5), ("m1", 2, 32), ("m1", 2, 32), ("m1", 4, 32))
