"""Reference of the reverse pass of the Gaussian moment step (csrc/sr_moments_vjp_dev.h): the analytic vector-Jacobian product of
tests/_ellipsoid_ref.step in modes 1 (first-order Taylor) and 2 (mean-equivalent), both starts, one query at a time, in
np.longdouble.  NumPy only: no GPU, no torch, no SciPy.

Written from the formulas of the forward reference (_ellipsoid_ref.step, which cites the reference project by line), in matrix
form, on the inputs of _ellipsoid_ref.cases; the device code works entry by entry, one row of each product at a time, and shares
nothing with this file.

For seeds mu1_bar, sigma1_bar on (p1, q1) of the step and gpvar_bar on the GP variances a roll-out returns beside them (None =
zero), with S = (sigma1_bar + sigma1_bar^T) / 2:

    p1 = a mu_x + b k_ff + mu_g              mug_bar = mu1_bar, mux_bar = a^T mu1_bar, kff_bar = b^T mu1_bar
    q1 = [H Sigma H^T +] diag(var_g)         var_bar = diag(S) + gpvar_bar
    Gaussian start:  H = a + J_x + (J_u + b) K (mode 1),  H = a + b K (mode 2)
                     sigma_bar = H^T S H,   H_bar = 2 S H sym(Sigma)
                     mode 1: jac_bar = [H_bar, H_bar K^T], kfb_bar = (J_u + b)^T H_bar;  mode 2: jac_bar = 0, kfb_bar = b^T H_bar
    point start:     sigma_bar, kfb_bar, jac_bar = 0

Sigma is read as (Sigma + Sigma^T) / 2, so sigma_bar is symmetric.  Nothing passes through an eigenvalue or a square root: all ten
families of _ellipsoid_ref.cases are value families here, `tiny` and `huge` included, no query is bad, there is no gap factor.
The fp64 restatement (step_vjp(..., fp64=True)) runs the same formulas in float64; it exists only to measure the rounding floor
of a correct fp64 implementation.

ERROR SCALES.  Per output array step_vjp returns `<name>_abs`, the same reverse pass with every term replaced by its absolute value
(|H| = |a| + |J_x| + (|J_u| + |b|) |K| and so on): the sum of the absolute values of the terms of that entry, what its rounding
errors grow with.

TOLERANCES, stated once for the host and the GPU tests:  |got - want| <= FACTOR SHARE[name] EPS <name>_abs, FACTOR = 30 (the
project's margin over a CPU floor), SHARE[name] the worst ratio |fp64 restatement - long double| / (EPS <name>_abs) over the host
cases (instances (1,1), (2,1), (3,2), (4,1), (8,4); every family; modes 1 and 2; both starts; 16 queries of each case, every
17th of the 257, so that the three gain scales 0, 0.3 and 1e3 are all met; measure_shares() below, obtained as
_ellipsoid_grad_ref.measure_shares obtains its table and asserted by tests/test_moments_grad_host.py wherever np.longdouble is
wider than fp64).  A share of 0 (mug_bar: a copy) means bit equality.  Measured on x86-64 (80-bit long double), then rounded up:

    mux_bar 1.38   sigma_bar 2.14   kff_bar 0.99   kfb_bar 1.54   mug_bar 0 (a copy)   var_bar 0 (one rounding)   jac_bar 2.30

var_bar = S_ii + gpvar_bar_i is ONE fp64 addition of two fp64 numbers (S_ii = (G_ii + G_ii) / 2 is exact): the restatement and the
long-double sum rounded to fp64 gave the same bits in every case, so the device is held to the bits as well.
"""
import numpy as np

import _ellipsoid_ref as R

LD = np.longdouble
EPS = R.EPS
FACTOR = 30.0
MODES = (1, 2)
STARTS = ("gauss", "point")
OUTPUTS = ("mux_bar", "sigma_bar", "kff_bar", "kfb_bar", "mug_bar", "var_bar", "jac_bar")
FAMILIES = R.Q_FAMILIES
HOST_INSTANCES = ((1, 1), (2, 1), (3, 2), (4, 1), (8, 4))
# worst measured share of EPS x abs-scale used by the fp64 restatement (see the docstring), rounded up
SHARE = dict(mux_bar=1.4, sigma_bar=2.2, kff_bar=1.0, kfb_bar=1.6, mug_bar=0.0, var_bar=0.0, jac_bar=2.3)
SHARE_ROWS = tuple(range(0, R.T_CASE, 17))[:16]


def step_vjp(mu_x, sigma_x, k_ff, k_fb, mu_g, var_g, jac, a, b, mode, mu1_bar=None, sigma1_bar=None, gpvar_bar=None, fp64=False):
    """One query; forward arguments as _ellipsoid_ref.step (sigma_x None = point start; mu_x, k_ff, mu_g, var_g are not read by the
    derivative but give the sizes), seeds mu1_bar (n_s,), sigma1_bar (n_s,n_s), gpvar_bar (n_s,) or None.
    Returns a dict: the seven arrays of OUTPUTS and `<name>_abs` for each.  At a point start, and jac_bar in mode 2, zeros."""
    assert mode in MODES
    dt = np.float64 if fp64 else LD
    cv = lambda x: None if x is None else np.asarray(x, dtype=dt)
    n_s, n_u = np.asarray(mu_x).shape[0], np.asarray(k_ff).shape[0]
    D = n_s + n_u
    if a is None:
        a, b = np.eye(n_s, dtype=dt), np.zeros((n_s, n_u), dtype=dt)
    a, b = cv(a), cv(b)
    zeros = lambda *s: np.zeros(s, dtype=dt)
    mb = zeros(n_s) if mu1_bar is None else cv(mu1_bar)
    S = zeros(n_s, n_s) if sigma1_bar is None else cv(sigma1_bar)
    S = (S + S.T) / 2
    gv = zeros(n_s) if gpvar_bar is None else cv(gpvar_bar)
    out = dict(mug_bar=mb.copy(), mug_bar_abs=np.abs(mb), mux_bar=a.T.dot(mb), mux_bar_abs=np.abs(a).T.dot(np.abs(mb)),
               kff_bar=b.T.dot(mb), kff_bar_abs=np.abs(b).T.dot(np.abs(mb)),
               var_bar=np.diag(S) + gv, var_bar_abs=np.abs(np.diag(S)) + np.abs(gv))
    if sigma_x is None:
        for name, shape in (("sigma_bar", (n_s, n_s)), ("kfb_bar", (n_u, n_s)), ("jac_bar", (n_s, D))):
            out[name], out[name + "_abs"] = zeros(*shape), zeros(*shape)
        return out
    q, k = cv(sigma_x), cv(k_fb)
    qs = (q + q.T) / 2
    if mode == 1:
        jac = cv(jac)
        bm, bm_abs = jac[:, n_s:] + b, np.abs(jac[:, n_s:]) + np.abs(b)
        h = a + jac[:, :n_s] + bm.dot(k)
        h_abs = np.abs(a) + np.abs(jac[:, :n_s]) + bm_abs.dot(np.abs(k))
    else:
        bm, bm_abs = b, np.abs(b)
        h, h_abs = a + b.dot(k), np.abs(a) + np.abs(b).dot(np.abs(k))
    hb = 2 * S.dot(h).dot(qs)
    hb_abs = 2 * np.abs(S).dot(h_abs).dot(np.abs(qs))
    sb = h.T.dot(S).dot(h)
    out.update(sigma_bar=(sb + sb.T) / 2, sigma_bar_abs=h_abs.T.dot(np.abs(S)).dot(h_abs),
               kfb_bar=bm.T.dot(hb), kfb_bar_abs=bm_abs.T.dot(hb_abs))
    if mode == 1:
        out.update(jac_bar=np.hstack((hb, hb.dot(k.T))), jac_bar_abs=np.hstack((hb_abs, hb_abs.dot(np.abs(k).T))))
    else:
        out.update(jac_bar=zeros(n_s, D), jac_bar_abs=zeros(n_s, D))
    return out


def seeds(case, seed=0):
    """mu1_bar (T,n_s), sigma1_bar (T,n_s,n_s) (not symmetric: only its symmetric part may count), gpvar_bar (T,n_s) for a case of
    _ellipsoid_ref.cases"""
    T, n_s = case["p"].shape
    rng = np.random.default_rng([seed, T, n_s, 1612])
    return rng.standard_normal((T, n_s)), rng.standard_normal((T, n_s, n_s)), rng.standard_normal((T, n_s))


def vjp_batch(case, start, mode, mu1_bar, sigma1_bar, gpvar_bar=None, lin=True, fp64=False, rows=None):
    """step_vjp over the queries `rows` (default: all) of a case; start "point" passes sigma_x = None.  float64 arrays per name and
    the `_abs` arrays."""
    rows = range(case["p"].shape[0]) if rows is None else rows
    a, b = (case["a"], case["b"]) if lin else (None, None)
    pick = lambda x, t: None if x is None else x[t]
    outs = [step_vjp(case["p"][t], case["q"][t] if start == "gauss" else None, case["k_ff"][t], case["k_fb"][t], case["mu"][t],
                     case["var"][t], case["jac"][t], a, b, mode, pick(mu1_bar, t), pick(sigma1_bar, t), pick(gpvar_bar, t),
                     fp64=fp64) for t in rows]
    res = {}
    for name in OUTPUTS:
        res[name] = np.array([o[name] for o in outs]).astype(np.float64)
        res[name + "_abs"] = np.array([o[name + "_abs"] for o in outs]).astype(np.float64)
    return res


def share_used(got, want, want_abs):
    """largest |got - want| / (EPS abs) over the entries (0 where both agree exactly, inf where got is not finite or differs at a
    zero scale)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    err, tol = np.abs(got - want), EPS * np.asarray(want_abs, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    share = np.where(np.isfinite(got), share, np.inf)
    return float(np.max(share))


def bar(name):
    """the GPU bar of output `name` as a share of EPS x abs-scale"""
    return FACTOR * SHARE[name]


def within_bar(got, want, want_abs, name):
    """share of the bar of `name` that is used (<= 1 passes); a bar of zero asks for equal bits"""
    used = share_used(got, want, want_abs)
    return used / bar(name) if bar(name) > 0 else (0.0 if used == 0 else np.inf)


def measure_shares(instances=HOST_INSTANCES, families=FAMILIES, rows=SHARE_ROWS):
    """the fp64 restatement against the long-double VJP: worst share per output over the host cases"""
    worst = {name: 0.0 for name in OUTPUTS}
    for n_s, n_u in instances:
        cs = R.cases(n_s, n_u)
        for fam in families:
            if fam not in cs:
                continue
            sd = seeds(cs[fam])
            for mode in MODES:
                for start in STARTS:
                    ld = vjp_batch(cs[fam], start, mode, *sd, rows=rows)
                    f64 = vjp_batch(cs[fam], start, mode, *sd, rows=rows, fp64=True)
                    for name in OUTPUTS:
                        worst[name] = max(worst[name], share_used(f64[name], ld[name], ld[name + "_abs"]))
    return worst
