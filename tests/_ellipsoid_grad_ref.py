"""Reference of the reverse pass of the ellipsoid step (csrc/sr_ellipsoid_vjp_dev.h): the analytic vector-Jacobian product of
tests/_ellipsoid_ref.step in mode 0, one query at a time, in np.longdouble.  NumPy only: no GPU, no torch, no SciPy.

Written from the formulas of the forward reference (_ellipsoid_ref.step, which cites the reference project by line), in
matrix form; the device code works entry by entry, one row of each product at a time, and shares nothing with this file.

For seeds p1_bar, q1_bar (None = zero) on (p1, q1), with G = (q1_bar + q1_bar^T) / 2:

    p1 = a p + b u + mu                      mu_bar = p1_bar, p_bar = a^T p1_bar, kff_bar = b^T p1_bar
    point:  q1 = diag(n c^2 var)             var_bar = n c^2 diag(G)
    ellipsoid:  q1 = (1 + c2) Q0 + (1 + 1/c2) diag(dL),  c2 = sqrt(tr dL / tr Q0),  dL = (1 + 1/c1) dS + (1 + c1) dM,
        c1 = sqrt(tr dS / tr dM),  dS = n (c (sqrt(var) + l_sigma r))^2,  dM = n (l_mu r^2)^2,  Q0 = H q H^T,
        H = a + J_x + (J_u + b) K,  r^2 = lambda_max(q (I + K^T K)),
    each reversed in turn; d r^2 / dq = w w^T, d r^2 / dK = 2 r^2 (K v) v^T with y the unit top eigenvector of M = L^T q L
    (I + K^T K = L L^T), w = L y, v = L^-T y.  q is read as (q + q^T) / 2, so q_bar is symmetric.

THE EIGENVECTOR in long double: np.linalg.eigh has no long-double form.  Its fp64 eigenvectors v_i are corrected by first-order
perturbation theory against the long-double M, three times:  y <- y + sum_{i != top} v_i (v_i . (M y - lambda y)) / (lambda -
lambda_i); the error after a pass is the square of the one before (times 1 / g), so from 1e-16 / g it is below the long-double
rounding for every g >= 1e-3.  The fp64 restatement (step_vjp(..., fp64=True)) runs the same formulas in float64 with the eigh
vector as it comes; it exists only to measure the rounding floor of a correct fp64 implementation.

ERROR SCALES.  Per output array step_vjp returns `<name>_abs`, the same reverse pass with every term replaced by its absolute
value (|H| = |a| + |J_x| + (|J_u| + |b|) |K| and so on): what the rounding errors of the array grow with.  The two eigenvector
terms enter by their norms, |r2_bar| |w|^2 for every entry of q_bar and 2 |r2_bar| r^2 |K_u| |v|^2 for row u of kfb_bar: an
eigenvector is accurate to eps / g of its NORM, not entry by entry, so a small entry of w w^T carries the error of the large.
It also returns g = (lambda_1 - lambda_2) / lambda_1 of M (1 for n_s = 1): the eigenvector's error, and that of everything that passes
through r^2, grows as 1 / g.

TOLERANCES, stated once for the host and the GPU tests:  |got - want| <= 30 SHARE[name] EPS <name>_abs max(1, 1 / g), where
SHARE[name] is the worst ratio |fp64 restatement - long double| / (EPS <name>_abs max(1, 1 / g)) over the host cases
(instances (1,1), (2,1), (3,2), (4,1), (8,4); families random, diag, rank1, graded, rounded, tiny, huge; both branches; 16
queries of each case, every 17th of the 257, so that the three gain scales 0, 0.3 and 1e3 of the cases are all met;
measure_shares() below, asserted by tests/test_ellipsoid_grad_host.py wherever np.longdouble is wider than fp64).  30 is the factor the moment-matching tests use over their CPU floor.  Queries with g < G_MIN = 1e-3 are
left out of the value bars (at most 2 % of a case).  Measured on x86-64 (80-bit long double):

    p_bar 1.00   kff_bar 1.23   mu_bar 0 (a copy)   var_bar 9.50   q_bar 4.44   kfb_bar 201.5   jac_bar 1.11

kfb_bar stands apart: at a gain of 1e3, I + K^T K has a condition number of 1e6 n_s n_u, v = L^-T y carries 1e3 eps of its norm
and K v cancels on top, which the entrywise scale 2 |r2_bar| r^2 |K_u| |v|^2 does not see.  (The first 16 queries of a case all
have K = 0 and give 1.25: a floor measured there says nothing about the queries with a gain.)

`tiny` and `huge` are in: the fp64 restatement stays finite there and inside the same shares (the step is homogeneous in the
scale of q; nothing under- or overflows at 1e-100 / 1e+100).  `identity`, `twin_top`, `all_equal` tie by construction and are
tested for finite outputs, a symmetric q_bar and exact agreement of what does not pass through r^2 only.
"""
import numpy as np

import _ellipsoid_ref as R

LD = np.longdouble
EPS = R.EPS
G_MIN = 1e-3
FACTOR = 30.0
OUTPUTS = ("p_bar", "q_bar", "kff_bar", "kfb_bar", "mu_bar", "var_bar", "jac_bar")
VALUE_FAMILIES = ("random", "diag", "rank1", "graded", "rounded", "tiny", "huge")
TIE_FAMILIES = ("identity", "twin_top", "all_equal")
HOST_INSTANCES = ((1, 1), (2, 1), (3, 2), (4, 1), (8, 4))
# worst measured share of EPS x abs-scale x max(1, 1/g) used by the fp64 restatement (see the docstring), rounded up
SHARE = dict(p_bar=1.0, kff_bar=1.3, mu_bar=0.0, var_bar=9.6, q_bar=4.5, kfb_bar=202.0, jac_bar=1.2)
SHARE_ROWS = tuple(range(0, R.T_CASE, 17))[:16]


def _cholesky(b, dt):
    n = b.shape[0]
    l = np.zeros((n, n), dtype=dt)
    for j in range(n):
        l[j, j] = np.sqrt(b[j, j] - np.dot(l[j, :j], l[j, :j]))
        for i in range(j + 1, n):
            l[i, j] = (b[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return l


def _solve_upper(u, y, dt):
    """u x = y, u upper triangular"""
    n = u.shape[0]
    x = np.zeros(n, dtype=dt)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - np.dot(u[i, i + 1:], x[i + 1:])) / u[i, i]
    return x


def top_eigenpair(qs, k, dt, refine):
    """r^2, w, v, g for the symmetric qs and the gain k (see the module docstring)"""
    n = qs.shape[0]
    l = _cholesky(np.eye(n, dtype=dt) + k.T.dot(k), dt)
    m = l.T.dot(qs).dot(l)
    m = (m + m.T) / 2
    lam64, vec64 = np.linalg.eigh(m.astype(np.float64))
    g = 1.0 if n == 1 else float((lam64[-1] - lam64[-2]) / lam64[-1]) if lam64[-1] > 0 else 0.0
    vec = vec64.astype(dt)
    y = vec[:, -1]
    if refine and n > 1:
        lam_i = [vec[:, i].dot(m).dot(vec[:, i]) / vec[:, i].dot(vec[:, i]) for i in range(n - 1)]
        for _ in range(3):
            y = y / np.sqrt(y.dot(y))
            lam = y.dot(m).dot(y)
            r = m.dot(y) - lam * y
            for i in range(n - 1):
                den = (lam - lam_i[i]) * vec[:, i].dot(vec[:, i])
                if den != 0:
                    y = y + vec[:, i] * (vec[:, i].dot(r) / den)
    y = y / np.sqrt(y.dot(y))
    lam = y.dot(m).dot(y)
    return lam, l.dot(y), _solve_upper(l.T, y, dt), g


def step_vjp(p, q, k_ff, k_fb, mu, var, jac, l_mu, l_sigma, c, a, b, p1_bar=None, q1_bar=None, fp64=False):
    """One query; arguments as _ellipsoid_ref.step (mode 0), seeds p1_bar (n_s,), q1_bar (n_s,n_s) or None.
    Returns a dict: the seven arrays of OUTPUTS, `<name>_abs` for each, g, bad.  In the point branch q_bar, kfb_bar and
    jac_bar are zero.  A bad query (a box half-width not > 0) is all NaN."""
    dt = np.float64 if fp64 else LD
    cv = lambda x: None if x is None else np.asarray(x, dtype=dt)
    var = cv(var)
    n_s, n_u = var.shape[0], np.asarray(k_ff).shape[0]
    D = n_s + n_u
    if a is None:
        a, b = np.eye(n_s, dtype=dt), np.zeros((n_s, n_u), dtype=dt)
    a, b = cv(a), cv(b)
    pb = np.zeros(n_s, dtype=dt) if p1_bar is None else cv(p1_bar)
    G = np.zeros((n_s, n_s), dtype=dt) if q1_bar is None else cv(q1_bar)
    G = (G + G.T) / 2
    c = dt(c)
    out = dict(mu_bar=pb.copy(), mu_bar_abs=np.abs(pb), p_bar=a.T.dot(pb), p_bar_abs=np.abs(a).T.dot(np.abs(pb)),
               kff_bar=b.T.dot(pb), kff_bar_abs=np.abs(b).T.dot(np.abs(pb)), g=1.0)
    zeros = lambda *s: np.zeros(s, dtype=dt)
    if q is None:
        bad = not bool(np.all(c * np.sqrt(var) > 0))
        out.update(var_bar=n_s * c * c * np.diag(G), q_bar=zeros(n_s, n_s), kfb_bar=zeros(n_u, n_s), jac_bar=zeros(n_s, D))
        out.update(var_bar_abs=np.abs(out["var_bar"]), q_bar_abs=zeros(n_s, n_s), kfb_bar_abs=zeros(n_u, n_s),
                   jac_bar_abs=zeros(n_s, D))
    else:
        q, k, jac, lm, ls = cv(q), cv(k_fb), cv(jac), cv(l_mu), cv(l_sigma)
        qs = (q + q.T) / 2
        r2, w, v, g = top_eigenpair(qs, k, dt, refine=not fp64)
        r1 = np.sqrt(r2)
        jx, ju = jac[:, :n_s], jac[:, n_s:]
        bm = ju + b
        h = a + jx + bm.dot(k)
        h_abs = np.abs(a) + np.abs(jx) + (np.abs(ju) + np.abs(b)).dot(np.abs(k))
        q0 = h.dot(qs).dot(h.T)
        q0_abs = h_abs.dot(np.abs(qs)).dot(h_abs.T)
        tq0 = np.trace(q0)
        s = np.sqrt(var)
        ub_mu, ub_sg = lm * r2, c * (s + ls * r1)
        bad = not bool(np.all(ub_mu > 0) and np.all(ub_sg > 0))
        d_s, d_m = n_s * ub_sg * ub_sg, n_s * ub_mu * ub_mu
        ts, tm = d_s.sum(), d_m.sum()
        c1 = np.sqrt(ts / tm)
        d_l = (1 + 1 / c1) * d_s + (1 + c1) * d_m
        c2 = np.sqrt(d_l.sum() / tq0)
        gd, gd_abs = np.diag(G), np.abs(np.diag(G))
        # q1 = (1 + c2) q0 + (1 + 1/c2) diag(d_l); every line has its twin in absolute values
        c2b = (G * q0).sum() - (gd * d_l).sum() / (c2 * c2)
        c2b_abs = (np.abs(G) * q0_abs).sum() + (gd_abs * d_l).sum() / (c2 * c2)
        tlb, tq0b = c2b / (2 * c2 * tq0), -c2b * c2 / (2 * tq0)
        tlb_abs, tq0b_abs = c2b_abs / (2 * c2 * tq0), c2b_abs * c2 / (2 * tq0)
        dlb, dlb_abs = (1 + 1 / c2) * gd + tlb, (1 + 1 / c2) * gd_abs + tlb_abs
        c1b = (dlb * (d_m - d_s / (c1 * c1))).sum()
        c1b_abs = (dlb_abs * (d_m + d_s / (c1 * c1))).sum()
        dsb = (1 + 1 / c1) * dlb + c1b / (2 * c1 * tm)
        dsb_abs = (1 + 1 / c1) * dlb_abs + c1b_abs / (2 * c1 * tm)
        dmb = (1 + c1) * dlb - c1b * c1 / (2 * tm)
        dmb_abs = (1 + c1) * dlb_abs + c1b_abs * c1 / (2 * tm)
        ubb, ubb_abs = 2 * n_s * ub_sg * dsb, 2 * n_s * ub_sg * dsb_abs
        var_bar, var_bar_abs = c * ubb / (2 * s), c * ubb_abs / (2 * s)
        r2b = (2 * n_s * lm * lm * r2 * dmb).sum() + (c * ls * ubb).sum() / (2 * r1)
        r2b_abs = (2 * n_s * lm * lm * r2 * dmb_abs).sum() + (c * ls * ubb_abs).sum() / (2 * r1)
        q0b = (1 + c2) * G + tq0b * np.eye(n_s, dtype=dt)
        q0b_abs = (1 + c2) * np.abs(G) + tq0b_abs * np.eye(n_s, dtype=dt)
        hb = 2 * q0b.dot(h).dot(qs)
        hb_abs = 2 * q0b_abs.dot(h_abs).dot(np.abs(qs))
        kv, k_norm = k.dot(v), np.sqrt((k * k).sum(axis=1))
        out.update(g=g, var_bar=var_bar, var_bar_abs=var_bar_abs,
                   q_bar=h.T.dot(q0b).dot(h) + r2b * np.outer(w, w),
                   q_bar_abs=h_abs.T.dot(q0b_abs).dot(h_abs) + r2b_abs * w.dot(w),
                   kfb_bar=bm.T.dot(hb) + 2 * r2b * r2 * np.outer(kv, v),
                   kfb_bar_abs=(np.abs(ju) + np.abs(b)).T.dot(hb_abs) + 2 * r2b_abs * r2 * v.dot(v) * k_norm[:, None],
                   jac_bar=np.hstack((hb, hb.dot(k.T))), jac_bar_abs=np.hstack((hb_abs, hb_abs.dot(np.abs(k).T))))
        out["q_bar"] = (out["q_bar"] + out["q_bar"].T) / 2
    out["bad"] = bad
    if bad:
        for name in OUTPUTS:
            out[name] = np.full(out[name].shape, np.nan, dtype=dt)
    return out


def seeds(case, seed=0):
    """p1_bar (T,n_s), q1_bar (T,n_s,n_s) (not symmetric: only its symmetric part may count) for a case of _ellipsoid_ref.cases"""
    T, n_s = case["p"].shape
    rng = np.random.default_rng([seed, T, n_s, 4711])
    return rng.standard_normal((T, n_s)), rng.standard_normal((T, n_s, n_s))


def vjp_batch(case, branch, p1_bar, q1_bar, lin=True, fp64=False, rows=None):
    """step_vjp over the queries `rows` (default: all) of a case; branch "point" passes q = None.  float64 arrays per name,
    the `_abs` arrays, g (T,) and bad (T,)."""
    rows = range(case["p"].shape[0]) if rows is None else rows
    a, b = (case["a"], case["b"]) if lin else (None, None)
    outs = [step_vjp(case["p"][t], case["q"][t] if branch == "ell" else None, case["k_ff"][t], case["k_fb"][t], case["mu"][t],
                     case["var"][t], case["jac"][t], case["l_mu"], case["l_sigma"], case["c"], a, b,
                     None if p1_bar is None else p1_bar[t], None if q1_bar is None else q1_bar[t], fp64=fp64) for t in rows]
    res = {}
    for name in OUTPUTS:
        res[name] = np.array([o[name] for o in outs]).astype(np.float64)
        res[name + "_abs"] = np.array([o[name + "_abs"] for o in outs]).astype(np.float64)
    res["g"] = np.array([o["g"] for o in outs])
    res["bad"] = np.array([o["bad"] for o in outs])
    return res


def gap_factor(g):
    """max(1, 1/g) per query, shaped to broadcast against an output array of any rank"""
    return np.maximum(1.0, 1.0 / np.maximum(np.asarray(g, dtype=np.float64), 1e-300))


def share_used(got, want, want_abs, g):
    """largest |got - want| / (EPS abs max(1, 1/g)) over the entries (0 where both agree exactly, inf where got is not finite or
    differs at a zero scale)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    gf = gap_factor(g).reshape((-1,) + (1,) * (got.ndim - 1))
    err, tol = np.abs(got - want), EPS * np.asarray(want_abs, dtype=np.float64) * gf
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    share = np.where(np.isfinite(got), share, np.inf)
    return float(np.max(share))


def bar(name):
    """the GPU bar of output `name` as a share of EPS x abs-scale x max(1, 1/g)"""
    return FACTOR * SHARE[name]


def measure_shares(instances=HOST_INSTANCES, families=VALUE_FAMILIES, rows=SHARE_ROWS):
    """the fp64 restatement against the long-double VJP: worst share per output over the host cases (queries with g >= G_MIN)"""
    worst = {name: 0.0 for name in OUTPUTS}
    for n_s, n_u in instances:
        cs = R.cases(n_s, n_u)
        for fam in families:
            if fam not in cs:
                continue
            pb, qb = seeds(cs[fam])
            for branch in ("ell", "point"):
                ld = vjp_batch(cs[fam], branch, pb, qb, rows=rows)
                f64 = vjp_batch(cs[fam], branch, pb, qb, rows=rows, fp64=True)
                keep = (ld["g"] >= G_MIN) & ~ld["bad"]
                for name in OUTPUTS:
                    worst[name] = max(worst[name], share_used(f64[name][keep], ld[name][keep], ld[name + "_abs"][keep],
                                                              ld["g"][keep]))
    return worst
