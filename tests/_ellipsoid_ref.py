"""Long-double reference of the per-query ellipsoid family of csrc/sr_ellipsoid_dev.h / csrc/sr_ellipsoid.hip (the ellipsoid
and moment step, the remainder boxes, distance to centre, safety distance, the sampling step) and the inputs its tests run
on.  NumPy only: no GPU, no torch, no SciPy.

The formulas are those of the reference project that oracle/oracle_np.py: onestep_reachability_from_gp cites by line
(gp_reachability.py:65-156, utils.py:108-144, utils_ellipsoid.py:36-94, 197-233, uncertainty_propagation_casadi.py:57-87,
260-283), written as plain loops over one query at a time in np.longdouble.  Where np.longdouble is the 80-bit x87 format
(eps 1.1e-19) the results carry three more digits than any fp64 implementation; where it is fp64 the module is simply an
independent fp64 implementation -- every tolerance of the tests was chosen so that a correct fp64 implementation meets it.

The one quantity that is not a finite formula is r^2 = lambda_max(Q (I + K^T K)).  lambda_max_qb takes the symmetric form
M = L^T Q L (B = I + K^T K = L L^T) in long double, the top eigenvector of M rounded to fp64 from np.linalg.eigh, and
returns its Rayleigh quotient with the long-double M: the error of a Rayleigh quotient is QUADRATIC in the eigenvector's
error (sum_i (lambda_max - lambda_i) delta_i^2 with delta_i ~ eps |M| / (lambda_max - lambda_i)), so it stays at a few
1e-16 relative even where the top eigenvalues agree to 14 digits.

ERROR BOUNDS.  step() also returns, entrywise, the magnitude that the rounding errors of a step scale with:
    p1_abs = |a| |p| + |b| |u| + |mu|
    q1_abs = (1 + c2) |H|b |Q| |H|b^T + the diagonal term,      |H|b = |a| + |jac_x| + (|jac_u| + |b|) |k_fb|
An off-diagonal entry of H Q H^T may cancel to far below q1_abs; the tests forgive 16 n_s eps q1_abs there (the standard
bound of the two dot products of length n_s) and nothing more.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
T_CASE = 257                       # a full 256-thread block and a one-thread tail
C_SAFETY = 1.7
KFB_SCALES = (0.0, 0.3, 1e3)       # thirds of every family; 1e3 makes I + K^T K ill-conditioned (cond ~ 1e6 n_s n_u)
Q_FAMILIES = ("random", "diag", "identity", "rank1", "twin_top", "all_equal", "graded", "tiny", "huge", "rounded")


def _ld(x, dtype=LD):
    return None if x is None else np.asarray(x, dtype=dtype)


def _cholesky(b):
    """lower Cholesky factor in the dtype of b (long double unless the caller chose another), plain column loop"""
    n = b.shape[0]
    l = np.zeros((n, n), dtype=b.dtype)
    for j in range(n):
        s = b[j, j] - np.dot(l[j, :j], l[j, :j])
        l[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            l[i, j] = (b[i, j] - np.dot(l[i, :j], l[j, :j])) / l[j, j]
    return l


def similarity(q, k_fb, dtype=LD):
    """M = L^T Q L with B = I + K^T K = L L^T, all in `dtype` (long double): eig(M) == eig(Q B)."""
    q = _ld(q, dtype)
    q = (q + q.T) / 2
    k = _ld(k_fb, dtype)
    l = _cholesky(np.eye(q.shape[0], dtype=dtype) + k.T.dot(k))
    return l.T.dot(q).dot(l)


def lambda_max_qb(q, k_fb, dtype=LD):
    """largest eigenvalue of Q (I + K^T K), Q symmetric positive semi-definite; a scalar of `dtype` (long double)"""
    m = similarity(q, k_fb, dtype)
    m = (m + m.T) / 2
    _, vec = np.linalg.eigh(m.astype(np.float64))
    v = _ld(vec[:, -1], dtype)
    return v.dot(m).dot(v) / v.dot(v)


def _lin(a, b, n_s, n_u, dtype=LD):
    if a is None:                                  # gp_reachability.py:61-63
        return np.eye(n_s, dtype=dtype), np.zeros((n_s, n_u), dtype=dtype)
    return _ld(a, dtype), _ld(b, dtype)


def step(p, q, k_ff, k_fb, mu, var, jac, l_mu, l_sigma, c, a, b, mode=0, dtype=LD):
    """One query.  p (n_s,), q (n_s,n_s) or None, k_ff (n_u,), k_fb (n_u,n_s), mu, var (n_s,), jac (n_s,n_s+n_u),
    mode 0: reachability step; 1: Taylor moments; 2: mean-equivalent moments (jac is not read).
    Returns dict(p1, q1, bad, p1_abs, q1_abs), long double; dtype=np.float64 runs the same lines in fp64 (the rounding floor of
    a correct fp64 implementation; tests/_chain_ref.py)."""
    ld = lambda x: _ld(x, dtype)
    p, u, mu, var = ld(p), ld(k_ff), ld(mu), ld(var)
    n_s, n_u = p.shape[0], u.shape[0]
    a, b = _lin(a, b, n_s, n_u, dtype)
    p1 = a.dot(p) + b.dot(u) + mu                                     # :82-83 / :115
    p1_abs = np.abs(a).dot(np.abs(p)) + np.abs(b).dot(np.abs(u)) + np.abs(mu)
    if q is None:
        if mode == 0:                                                 # :78-80: diag(n_s (c sqrt(var))^2)
            ub = c * np.sqrt(var)
            q1 = np.diag(n_s * ub * ub)
            bad = not bool(np.all(ub > 0))
        else:                                                         # uncertainty_propagation_casadi.py:50-55
            q1, bad = np.diag(var), False
        return dict(p1=p1, q1=q1, bad=bad, p1_abs=p1_abs, q1_abs=np.abs(q1))
    q, k = ld(q), ld(k_fb)
    if mode == 2:
        h = a + b.dot(k)
        h_abs = np.abs(a) + np.abs(b).dot(np.abs(k))
    else:
        jac = ld(jac)
        a_mu, b_mu = jac[:, :n_s], jac[:, n_s:]                       # :110-111
        h = a + a_mu + (b_mu + b).dot(k)                              # :114
        h_abs = np.abs(a) + np.abs(a_mu) + (np.abs(b_mu) + np.abs(b)).dot(np.abs(k))
    q0 = h.dot(q).dot(h.T)                                            # :117
    q0_abs = h_abs.dot(np.abs(q)).dot(h_abs.T)
    if mode != 0:                                                     # [a b I] Sigma_all [a b I]^T = H Sigma H^T + diag(var)
        return dict(p1=p1, q1=q0 + np.diag(var), bad=False, p1_abs=p1_abs, q1_abs=q0_abs + np.diag(var))
    r2 = lambda_max_qb(q, k, dtype)                                        # utils.py:129-142
    ub_mu = ld(l_mu) * r2
    ub_sg = c * (np.sqrt(var) + ld(l_sigma) * np.sqrt(r2))           # :127
    bad = not bool(np.all(ub_mu > 0) and np.all(ub_sg > 0))
    d_s, d_m = n_s * ub_sg * ub_sg, n_s * ub_mu * ub_mu               # utils_ellipsoid.py:197-233
    c1 = np.sqrt(d_s.sum() / d_m.sum())                               # utils_ellipsoid.py:88-92
    d_l = (1 + 1 / c1) * d_s + (1 + c1) * d_m                         # :143
    c2 = np.sqrt(d_l.sum() / np.trace(q0))
    q1 = (1 + c2) * q0 + np.diag((1 + 1 / c2) * d_l)                  # :148
    q1_abs = (1 + c2) * q0_abs + np.diag((1 + 1 / c2) * d_l)
    return dict(p1=p1, q1=q1, bad=bad, p1_abs=p1_abs, q1_abs=q1_abs)


def step_batch(case, branch="ell", mode=0, lin=True, jac=True):
    """step() over the T queries of a case of cases(); branch "point" passes q = None.  Returns float64 arrays p1 (T,n_s),
    q1 (T,n_s,n_s), p1_abs, q1_abs (rounded from long double) and bad (T,) bool."""
    T = case["p"].shape[0]
    a, b = (case["a"], case["b"]) if lin else (None, None)
    out = [step(case["p"][t], case["q"][t] if branch == "ell" else None, case["k_ff"][t], case["k_fb"][t], case["mu"][t],
                case["var"][t], case["jac"][t] if jac else None, case["l_mu"], case["l_sigma"], case["c"], a, b, mode)
           for t in range(T)]
    res = {k: np.array([o[k] for o in out]).astype(np.float64) for k in ("p1", "q1", "p1_abs", "q1_abs")}
    res["bad"] = np.array([o["bad"] for o in out])
    return res


def remainder(q, k_fb, l_mu, l_sigma):
    """utils.py:108-144 for one query: u_mu = l_mu r^2, u_sigma = l_sigma r."""
    r2 = lambda_max_qb(q, k_fb)
    return _ld(l_mu) * r2, _ld(l_sigma) * np.sqrt(r2)


def remainder_batch(case):
    out = [remainder(case["q"][t], case["k_fb"][t], case["l_mu"], case["l_sigma"]) for t in range(case["q"].shape[0])]
    return (np.array([o[0] for o in out]).astype(np.float64), np.array([o[1] for o in out]).astype(np.float64))


def distance(samples, p, q):
    """d_k = (s_k - p)^T Q^-1 (s_k - p) for one ellipsoid, samples (K,n_s): Cholesky solve in long double.
    Returns d (K,) and cond_2(Q) from fp64 np.linalg.cond."""
    l = _cholesky(_ld(q))
    n = l.shape[0]
    d = []
    for s in _ld(samples):
        v, y = s - _ld(p), np.zeros(n, dtype=LD)
        for i in range(n):
            y[i] = (v[i] - np.dot(l[i, :i], y[:i])) / l[i, i]
        d.append(y.dot(y))
    return np.array(d, dtype=LD), float(np.linalg.cond(np.asarray(q, dtype=np.float64)))


def safety(p, q, h_mat, h_vec, c):
    """gp_reachability.py:245-248 for one ellipsoid: d_m = h_m p + c sqrt(h_m Q h_m^T) - h_vec_m, and the magnitude
    |h_m| |p| + c sqrt(h_m Q h_m^T) + |h_vec_m| its rounding errors scale with."""
    p, q, h, hv = _ld(p), _ld(q), _ld(h_mat), _ld(h_vec).reshape(-1)
    quad = np.array([h[m].dot(q).dot(h[m]) for m in range(h.shape[0])], dtype=LD)
    root = c * np.sqrt(quad)
    return h.dot(p) + root - hv, np.abs(h).dot(np.abs(p)) + root + np.abs(hv)


def sample(mu, var, eps, k_fb=None, k_ff=None):
    """sampling_models.py:66-80 for one test input: S (size,n_out) = mu + sqrt(var) eps, z = [S, k_fb S + k_ff]."""
    mu, var, eps = _ld(mu), _ld(var), _ld(eps)
    s = mu[None, :] + np.sqrt(var)[None, :] * eps
    if k_fb is None:
        return s, None
    return s, np.hstack((s, s.dot(_ld(k_fb).T) + _ld(k_ff)[None, :]))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _orthogonal(rng, T, n):
    o, r = np.linalg.qr(rng.standard_normal((T, n, n)))
    return o * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def _from_spectrum(o, lam):
    q = np.einsum('tij,tj,tkj->tik', o, lam, o)
    return (q + q.transpose(0, 2, 1)) / 2


def _random_q(rng, T, n):
    A = rng.standard_normal((T, n, n))
    return np.einsum('tij,tkj->tik', A, A) / n


def shape_matrices(name, rng, T, n_s, grade=(-12, 4)):
    """T shape matrices of one family (see Q_FAMILIES; the module docstring of tests/test_gpu_ellipsoid_family.py has the table)"""
    if name in ("random", "tiny", "huge", "rounded"):
        q = _random_q(rng, T, n_s)
        if name == "tiny":
            q = q * 1e-100
        elif name == "huge":
            q = q * 1e+100
        elif name == "rounded":                       # one ulp on the strict lower triangle: not bitwise symmetric,
            low = np.tril(np.ones((n_s, n_s), dtype=bool), -1)       # as the output of a previous step is not
            q[:, low] = np.nextafter(q[:, low], np.inf)
        return q
    if name == "diag":
        return np.einsum('ti,ij->tij', rng.uniform(0.1, 2.0, (T, n_s)), np.eye(n_s))
    if name == "identity":
        return np.broadcast_to(0.37 * np.eye(n_s), (T, n_s, n_s)).copy()
    if name == "rank1":
        v = rng.standard_normal((T, n_s))
        return np.einsum('ti,tj->tij', v, v)
    o = _orthogonal(rng, T, n_s)
    if name == "twin_top":
        assert n_s >= 2
        lam = rng.uniform(0.01, 0.5, (T, n_s))
        lam[:, 0], lam[:, 1] = 1.0, 1.0 + 1e-14
    elif name == "all_equal":
        lam = 1.0 + 1e-13 * rng.standard_normal((T, n_s))
    elif name == "graded":
        lam = np.broadcast_to(np.logspace(grade[0], grade[1], n_s), (T, n_s))
    else:
        raise KeyError(name)
    return _from_spectrum(o, lam)


def families(n_s):
    return tuple(f for f in Q_FAMILIES if not (f == "twin_top" and n_s < 2))


MIN_COS = 0.1


def _gain_that_sees_the_top_direction(rng, q, k_fb, scale):
    """Where one eigenvalue of q dominates (`rank1`, `graded`: q ~ lam w w^T), r^2 ~ lam (1 + sum_u (k_u . w)^2): with rows
    k_u of length ~1e3 almost orthogonal to w, each k_u . w is what is left of terms 1e3 times larger, and r^2 is
    ill-conditioned in its INPUTS by about 1 / max_u |cos(k_u, w)| -- no fp64 implementation can hold 1e-12 there (the
    fp64 oracle misses it by two orders of magnitude).  Such draws are drawn again until every query has a row with
    |cos| >= MIN_COS; about one query in five is redrawn at n_s = 8, n_u = 1."""
    w = np.linalg.eigh((q + q.transpose(0, 2, 1)) / 2)[1][:, :, -1]
    k_fb = k_fb.copy()
    while True:
        norm = np.linalg.norm(k_fb, axis=2)
        cos = np.abs(np.einsum('tui,ti->tu', k_fb, w)) / np.where(norm > 0, norm, 1.0)
        again = (scale > 0) & (cos.max(axis=1) < MIN_COS)
        if not again.any():
            return k_fb
        k_fb[again] = scale[again, None, None] * rng.standard_normal((int(again.sum()),) + k_fb.shape[1:])


_CASES = {}


def cases(n_s, n_u, seed=0):
    """family name -> dict of fp64 inputs for T_CASE queries: p, q, k_ff, k_fb, mu, var, jac, l_mu, l_sigma, c, a, b.
    Everything but q and k_fb is benign; k_fb is N(0,1) times 0, 0.3, 1e3 in thirds of the queries (KFB_SCALES), so with
    `diag` and `identity` the first third enters the eigen-solver with an exactly diagonal matrix.  `tiny` / `huge` scale
    l_mu by 1e+100 / 1e-100 and var by 1e-100 / 1e+100 beside q, which keeps every term of the step finite.  Cached: every
    caller gets the same arrays and must leave them unchanged."""
    key = (n_s, n_u, seed)
    if key in _CASES:
        return _CASES[key]
    T, D = T_CASE, n_s + n_u
    out = {}
    for i, name in enumerate(families(n_s)):
        rng = np.random.default_rng([seed, n_s, n_u, i])
        scale = np.repeat(KFB_SCALES, (T + 2) // 3)[:T]
        c = dict(p=rng.standard_normal((T, n_s)), k_ff=rng.standard_normal((T, n_u)), mu=rng.standard_normal((T, n_s)),
                 var=rng.uniform(1e-4, 1e-1, (T, n_s)), jac=0.1 * rng.standard_normal((T, n_s, D)),
                 l_mu=rng.uniform(0.01, 0.05, n_s), l_sigma=rng.uniform(0.01, 0.05, n_s), c=C_SAFETY,
                 a=0.7 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
                 k_fb=scale[:, None, None] * rng.standard_normal((T, n_u, n_s)), q=shape_matrices(name, rng, T, n_s))
        if name in ("rank1", "graded"):
            c["k_fb"] = _gain_that_sees_the_top_direction(rng, c["q"], c["k_fb"], scale)
        if name == "tiny":
            c["l_mu"], c["var"] = c["l_mu"] * 1e+100, c["var"] * 1e-100
        elif name == "huge":
            c["l_mu"], c["var"] = c["l_mu"] * 1e-100, c["var"] * 1e+100
        out[name] = c
    _CASES[key] = out
    return out


def distance_cases(n_s, seed=0, T=T_CASE, K=5):
    """family name -> dict(p (T,n_s), q (T,n_s,n_s), shared (K,n_s), per_t (T,K,n_s)) for `random` and for `graded` with the
    spectrum logspace(-6, 2): the tolerance of a solve scales with cond(q), and cond = 1e8 keeps it below 1e-6."""
    out = {}
    for i, name in enumerate(("random", "graded")):
        rng = np.random.default_rng([seed, n_s, 77, i])
        q = shape_matrices(name, rng, T, n_s, grade=(-6, 2))
        out[name] = dict(p=rng.standard_normal((T, n_s)), q=q, shared=rng.standard_normal((K, n_s)),
                         per_t=rng.standard_normal((T, K, n_s)))
    return out


# ---- tolerances (one statement of them for the host and the GPU tests) -------------------------------------------------------
RTOL = 1e-12                       # SURVEY 8(d), "ellipsoid algebra alone"
RTOL_SAMPLE = 1e-14


def p1_atol(p1_abs):
    return 8 * EPS * p1_abs


def q1_atol(n_s, q1_abs):
    """the two dot products of length n_s behind an entry of H Q H^T"""
    return 16 * n_s * EPS * q1_abs


def safety_atol(d_abs):
    return 8 * EPS * d_abs


def distance_rtol(cond):
    """64 u cond(q) with the unit roundoff u = EPS / 2, floored at RTOL (1.4e-6 / 2 at cond = 1e8)"""
    return np.maximum(RTOL, 64 * (EPS / 2) * np.asarray(cond))


def used(got, want, rtol, atol=0.0):
    """largest |got - want| / (rtol |want| + atol) over the entries: the share of the tolerance that is used, <= 1 passes.
    Anything non-finite in got, or an entry that differs where the tolerance is zero, gives inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err, tol = np.abs(got - want), rtol * np.abs(want) + atol
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(err == 0, 0.0, err / tol)
    share = np.where(np.isfinite(got), share, np.inf)
    return float(np.max(share)) if share.size else 0.0


# ---- the smaller kernels: batches of the per-query functions above, and their inputs -----------------------------------------
def distance_batch(dc, per_t):
    """distance() over the ellipsoids of one entry of distance_cases(): d (T,K) float64 and cond (T,)."""
    out = [distance(dc["per_t"][t] if per_t else dc["shared"], dc["p"][t], dc["q"][t]) for t in range(dc["p"].shape[0])]
    return np.array([o[0] for o in out]).astype(np.float64), np.array([o[1] for o in out])


def safety_cases(n_s, m, seed=0, T=T_CASE):
    """family name -> dict(p, q, h_mat (m,n_s), h_vec (m,), c) for `random` and `rank1`; the rows of h_mat are N(0,1).
    rank1: h Q h^T = (h . v)^2 is what is left of n_s^2 terms of size |h_i v_i h_j v_j|, so sqrt(h Q h^T) has a condition
    number of about 1 / cos(h, v)^2 in its inputs; a v with |cos(h_m, v)| < 0.05 for some row is drawn again (otherwise
    the smallest of the T m cosines is ~1e-3 and no fp64 evaluation meets the tolerance: the fp64 oracle did not)."""
    out = {}
    for i, name in enumerate(("random", "rank1")):
        rng = np.random.default_rng([seed, n_s, m, 55, i])
        h_mat = rng.standard_normal((m, n_s))
        if name == "rank1":
            v = rng.standard_normal((T, n_s))
            while True:
                cos = np.abs(v.dot(h_mat.T)) / (np.linalg.norm(v, axis=1)[:, None] * np.linalg.norm(h_mat, axis=1)[None, :])
                again = cos.min(axis=1) < 0.05
                if not again.any():
                    break
                v[again] = rng.standard_normal((int(again.sum()), n_s))
            q = np.einsum('ti,tj->tij', v, v)
        else:
            q = shape_matrices(name, rng, T, n_s)
        out[name] = dict(p=rng.standard_normal((T, n_s)), q=q, h_mat=h_mat, h_vec=rng.standard_normal(m), c=C_SAFETY)
    return out


def safety_batch(sc):
    out = [safety(sc["p"][t], sc["q"][t], sc["h_mat"], sc["h_vec"], sc["c"]) for t in range(sc["p"].shape[0])]
    return np.array([o[0] for o in out]).astype(np.float64), np.array([o[1] for o in out]).astype(np.float64)


def sample_case(n_out, n_u, T, size, seed=0):
    """mu (T,n_out), var, eps (T,size,n_out), k_fb (n_u,n_out), k_ff (n_u,).  Signs are mixed but no sum cancels: output d has
    the sign s_d in mu and eps, so |S| = |mu| + sqrt(var) |eps|, and row u of k_fb has the signs sigma_u s_d, k_ff the sign
    sigma_u, so every term of k_fb S + k_ff has the sign sigma_u.  (With free signs S and z come arbitrarily close to zero,
    and no fp64 evaluation holds a RELATIVE 1e-14 there.)"""
    rng = np.random.default_rng([seed, n_out, n_u, T, size, 33])
    s_d, s_u = rng.choice((-1.0, 1.0), n_out), rng.choice((-1.0, 1.0), n_u)
    pos = lambda *shape: np.abs(rng.standard_normal(shape)) + 0.01
    return dict(mu=s_d * pos(T, n_out), var=rng.uniform(1e-4, 1e-1, (T, n_out)), eps=s_d * pos(T, size, n_out),
                k_fb=s_u[:, None] * s_d[None, :] * pos(n_u, n_out), k_ff=s_u * pos(n_u))


def sample_batch(sc):
    """sample() over the T test inputs: S (T,size,n_out), z (T,size,n_out+n_u), float64"""
    out = [sample(sc["mu"][t], sc["var"][t], sc["eps"][t], sc["k_fb"], sc["k_ff"]) for t in range(sc["mu"].shape[0])]
    return np.array([o[0] for o in out]).astype(np.float64), np.array([o[1] for o in out]).astype(np.float64)
