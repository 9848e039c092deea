"""Long-double reference of the GP posterior (mean, variance, mean Jacobian) that is cheap at ANY number of training points,
the training data that makes it exact, and the a-priori error bars of the tests that use it (tests/test_gpu_posterior_routes.py,
tests/test_posterior_ref_host.py).  NumPy only: no GPU, no torch, no SciPy.

DATA.  N training points in c = ceil(N / 90) clusters of b = ceil(N / c) <= 90 points (c <= 128).  The cluster centres sit on a
D-dimensional lattice whose spacing is 40 lengthscales of the LONGEST output per axis; a point is its centre + U[-1.5, 1.5] l,
a query a centre + U[-2, 2] l (l: the per-axis base lengthscale; the outputs' ARD lengthscales are l times a factor in
[0.85, 1.2], all inside [0.5, 2]).  Point i belongs to cluster i mod c, so every 128-row chunk of the padded model holds
members of every cluster and every tile of U^-1 holds non-zeros: the device sees a dense-looking problem.  Beyond D = 3 both
half-widths shrink by 3 / D: 90 points in a box of 3 lengthscales
in six dimensions are so far apart that sigma^2 stays near k(x,x) and a broken variance would pass (median sigma^2 / k(x,x)
0.6 at D = 6 without it, 0.55 with sqrt(3 / D)).

Two points of different clusters are at least 40 - 1.5 / 0.85 - 2 / 0.85 > 35.8 lengthscales apart along one axis: their kernel
value is below exp(-640) ~ 1e-278 of the signal variance for "rbf" (no fp64 product with it survives) and below
(1 + 80 + 2137) exp(-80) ~ 4e-32 for "mat52".  The Gram matrix is therefore a permuted block-diagonal matrix to far below
the rounding of any fp64 -- or long-double -- evaluation, and the exact posterior at a query is that of the query's own
cluster.  (tests/test_posterior_ref_host.py compares with a dense long-double evaluation at N = 300.)

REFERENCE.  Ref factors every b x b block on its own in np.longdouble with a hand-written Cholesky and hand-written
triangular solves (columns / rows as single vector operations), all queries of a cluster as one right-hand side:
    mu = k*^T alpha,  sigma^2 = k(x,x) - |L^-1 k*|^2,  d mu / dx_j = sum_i alpha_i g_i (x_j - z_ij) / l_j^2
with g = kappa'(r) / r (rbf: -k; mat52: -(5/3)(1 + sqrt5 r) exp(-sqrt5 r) sf2).  The diagonal term is the one the library
adds: noise_variance + 1e-5 (noise_diag) + 1e-8 (GPy's jitter).  Where np.longdouble is the 80-bit x87 format the results
carry three more digits than any fp64 route; where it is fp64 the module is simply an independent fp64 implementation, and
the bars below were chosen so that a correct fp64 implementation meets them.

BARS (a priori; nothing here was measured on a device).  With u = 2^-53, kappa = cond_2 of the query's block K_c, b its size:
    bar_var = (3 b + 40) u kappa k(x,x)
    bar_mu  = (3 b + 40) u kappa sum_i |k*_i| |alpha_i|
    bar_jac = (3 b + 40) u kappa sum_i |k*_i'| |alpha_i| |z_ij - x_j| / l_j^2          (k*': |g_i|)
3 b u kappa is the textbook forward bound of a Cholesky solve with a b x b matrix (Higham, Accuracy and Stability, Th. 10.4:
backward error gamma_{3b+1} |L||L^T|, times the condition number); the cross-cluster entries a dense route adds are exact
zeros or below 1e-30 and lengthen no sum that matters.  The + 40 covers what the solve is fed and what follows it:
  * a kernel value: D <= 6 differences, divisions, squares and their sum give the exponent a = r^2 / 2 a relative error of at
    most (D + 2) u, so k* = sf2 exp(-a) is off by at most [(D + 2) a + 2] u k*; a exp(-a) <= 1 / e, hence |dk*_i| <=
    [(D + 2) / e + 2] u sf2 < 5 u k(x,x) per entry.  sigma^2 moves by 2 |k*^T K^-1 dk*| <= 2 |K^-1 k*| |dk*|, and with
    k*^T K^-1 k* <= k(x,x), |k*|^2 <= lambda_max k(x,x): at most 2 * 5 u kappa k(x,x) sqrt(b_eff) where only the ~ 6 points
    within a lengthscale or two of the query carry weight: <= 25 u kappa k(x,x);
  * the sum of squares, the subtraction from k(x,x) and the padding of the partial sums: < 15 u k(x,x) in any order of
    summation that adds b_eff significant terms.
The same count holds for mu and its Jacobian with their own magnitude sums (the weights alpha come out of the same solve).
For b = 90, kappa = 680 the bar is 2.3e-11 relative -- forty times below the project's 1e-9 bar for sigma^2;
bars() asserts that for sigma^2 and returns the smaller of the two for mu and J.  tests/test_posterior_ref_host.py shows that two independent fp64
NumPy routes (explicit inverse and Cholesky solve of the DENSE matrix) stay under a quarter of it on every case's data.
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
CLUSTER = 90                      # points per cluster (at most)
SPACING = 40.0                    # lattice spacing in lengthscales of the longest output
HALF_TRAIN, HALF_QUERY = 1.5, 2.0
NOISE_VARIANCE = 0.05
NOISE_DIAG, GPY_JITTER = 1e-5, 1e-8
CHUNK, COLBLOCK = 128, 256        # k-rows per chunk and columns per column block of the streamed kernels


def _lattice(c, D):
    """c distinct integer lattice points in D dimensions, the smallest cube that holds them"""
    side = 1
    while side ** D < c:
        side += 1
    idx = np.arange(c)
    out = np.empty((c, D))
    for j in range(D):
        out[:, j] = idx % side
        idx = idx // side
    return out


class Problem(object):
    """clustered training data of one (seed, N, D, n_out, kernel).  Fields: Z (N, D), Y (N, n_out), member (N,) cluster of
    every point, centres (c, D), base (D,) base lengthscales, ls (n_out, D), sf2 (n_out,), kern, nugget (n_out,), hyp
    (the list SimpleGPModel takes)."""

    def __init__(self, seed, N, D, n_out, kern="rbf", max_clusters=128, cap=CLUSTER):
        """cap: points per cluster at most (CLUSTER); cap >= N is ONE cluster, the recipe without the cap: a dense problem in
        which every row depends on every other (tests/_factor_ref.dense_problem)"""
        assert kern in ("rbf", "mat52")
        rng = np.random.default_rng(seed)
        c = -(-N // cap)
        assert 1 <= c <= max_clusters, "N = %d needs %d clusters (> %d)" % (N, c, max_clusters)
        self.seed, self.N, self.D, self.n_out, self.kern, self.c = seed, N, D, n_out, kern, c
        self.base = rng.uniform(0.6, 1.6, D)
        self.ls = self.base[None, :] * rng.uniform(0.85, 1.2, (n_out, D))
        assert self.ls.min() >= 0.5 and self.ls.max() <= 2.0
        self.sf2 = rng.uniform(0.9, 1.1, n_out)
        self.centres = _lattice(c, D) * (SPACING * self.ls.max(axis=0))[None, :]
        self.member = np.arange(N) % c
        self.shrink = min(1.0, 3.0 / D)
        self.Z = self.centres[self.member] + rng.uniform(-HALF_TRAIN, HALF_TRAIN, (N, D)) * self.base[None, :] * self.shrink
        self.w = rng.standard_normal((n_out, D))
        self.Y = self.targets(self.Z, self.member) + 0.05 * rng.standard_normal((N, n_out))
        self.nugget = np.full(n_out, NOISE_VARIANCE + NOISE_DIAG + GPY_JITTER)
        self._rng = rng

    def targets(self, x, member):
        """the smooth function the targets are noisy values of"""
        rel = (x - self.centres[member]) / self.base[None, :]
        return np.sin(rel.dot(self.w.T)) + 0.5 * np.cos(1.0 + member[:, None] + np.arange(self.n_out)[None, :])

    @property
    def hyp(self):
        return [{"lengthscale": self.ls[d].copy(), "variance": float(self.sf2[d]), "noise_variance": NOISE_VARIANCE}
                for d in range(self.n_out)]

    def queries(self, T, seed):
        """T queries: a cluster centre + U[-2, 2] l; the clusters are visited in turn from cluster 0 on (the cluster of the
        first training row: with N = Np - 127 the first chunk holds that one row, and only a query of its cluster can tell
        whether the chunk was read).  Returns X (T, D), qc (T,)"""
        rng = np.random.default_rng([self.seed, seed, T])
        qc = (np.arange(T) * max(1, self.c // 7 | 1)) % self.c
        X = self.centres[qc] + rng.uniform(-HALF_QUERY, HALF_QUERY, (T, self.D)) * self.base[None, :] * self.shrink
        return X, qc

    def new_points(self, m, seed):
        """m further training points (each joins a cluster): x (m, D), y (m, n_out), cluster (m,)"""
        rng = np.random.default_rng([self.seed, 7919, seed, m])
        q = rng.integers(0, self.c, m)
        x = self.centres[q] + rng.uniform(-HALF_TRAIN, HALF_TRAIN, (m, self.D)) * self.base[None, :] * self.shrink
        return x, self.targets(x, q) + 0.05 * rng.standard_normal((m, self.n_out)), q

    def grown(self, x, y, q):
        """a copy with the points (x, y) of clusters q appended behind the others"""
        import copy
        p = copy.copy(self)
        p.Z, p.Y, p.member = np.vstack((self.Z, x)), np.vstack((self.Y, y)), np.concatenate((self.member, q))
        p.N = p.Z.shape[0]
        return p

    def without(self, rows):
        """a copy without the rows `rows` (indices into the current rows, any order, each once); the others keep their order.
        Removal keeps the order inside every cluster, as appending behind the others does, so after any mixture of `grown` and
        `without` the dense factor of the remaining rows restricted to a cluster's indices is still the factor of that
        cluster's remaining rows in their order: the argument of tests/_factor_ref.py's docstring (a permutation that keeps
        the order inside every block of a block-diagonal matrix) carries over unchanged, and Ref / FactorRef of the copy are
        exact.  No cluster may lose its last point (the classes factor every cluster)."""
        import copy
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        assert rows.size == np.unique(rows).size and rows.min() >= 0 and rows.max() < self.N
        keep = np.ones(self.N, dtype=bool)
        keep[rows] = False
        p = copy.copy(self)
        p.Z, p.Y, p.member = self.Z[keep], self.Y[keep], self.member[keep]
        p.N = p.Z.shape[0]
        assert np.all(np.bincount(p.member, minlength=p.c) > 0), "a cluster lost its last point"
        return p


# ------------------------------------------------------------------------------------------------ long-double algebra
def cholesky_ld(a, dtype=LD):
    """lower Cholesky factor of a (long double), one vector operation per column.  dtype (here and below): np.float64 runs
    the same lines in fp64, the rounding floor of a correct fp64 implementation (tests/_chain_ref.py)"""
    n = a.shape[0]
    a = np.asarray(a, dtype=dtype)
    l = np.zeros((n, n), dtype=dtype)
    for j in range(n):
        s = a[j, j] - np.dot(l[j, :j], l[j, :j])
        assert s > 0
        l[j, j] = np.sqrt(s)
        if j + 1 < n:
            l[j + 1:, j] = (a[j + 1:, j] - l[j + 1:, :j].dot(l[j, :j])) / l[j, j]
    return l


def solve_lower_ld(l, rhs, dtype=LD):
    """l^-1 rhs by forward substitution, rhs (n, m)"""
    x = np.array(rhs, dtype=dtype)
    for i in range(l.shape[0]):
        if i:
            x[i] -= l[i, :i].dot(x[:i])
        x[i] /= l[i, i]
    return x


def solve_upper_ld(l, rhs, dtype=LD):
    """l^-T rhs by back substitution (l lower), rhs (n, m)"""
    x = np.array(rhs, dtype=dtype)
    for i in range(l.shape[0] - 1, -1, -1):
        if i + 1 < l.shape[0]:
            x[i] -= l[i + 1:, i].dot(x[i + 1:])
        x[i] /= l[i, i]
    return x


def kernel_ld(kern, x, z, ls, sf2, dtype=LD):
    """k (T, n) and g = kappa'(r) / r (T, n) of x (T, D) against z (n, D), long double"""
    LD = dtype
    x, z, ls = np.asarray(x, dtype=LD), np.asarray(z, dtype=LD), np.asarray(ls, dtype=LD)
    diff = (x[:, None, :] - z[None, :, :]) / ls[None, None, :]
    r2 = np.sum(diff * diff, axis=2)
    sf2 = LD(sf2)
    if kern == "rbf":
        k = sf2 * np.exp(-r2 / 2)
        return k, -k
    r = np.sqrt(r2)
    s5 = np.sqrt(LD(5))
    e = sf2 * np.exp(-s5 * r)
    return (1 + s5 * r + LD(5) / 3 * r2) * e, -(LD(5) / 3) * (1 + s5 * r) * e


class Ref(object):
    """the factored blocks of a Problem; predict() evaluates queries against them"""

    def __init__(self, prob):
        self.p = prob
        self.idx = [np.flatnonzero(prob.member == q) for q in range(prob.c)]      # ascending: the order of the dense factor
        self.b = max(len(i) for i in self.idx)
        self.L, self.alpha, self.kappa = {}, {}, {}

    def block(self, q, d):
        """(L, alpha, kappa_2) of cluster q, output d"""
        if (q, d) not in self.L:
            p, i = self.p, self.idx[q]
            k, _ = kernel_ld(p.kern, p.Z[i], p.Z[i], p.ls[d], p.sf2[d])
            k = (k + k.T) / 2 + LD(p.nugget[d]) * np.eye(len(i), dtype=LD)
            l = cholesky_ld(k)
            self.L[q, d] = l
            self.alpha[q, d] = solve_upper_ld(l, solve_lower_ld(l, np.asarray(p.Y[i, d], dtype=LD)[:, None]))[:, 0]
            ev = np.linalg.eigvalsh(k.astype(np.float64))
            self.kappa[q, d] = float(ev[-1] / ev[0])
        return self.L[q, d], self.alpha[q, d], self.kappa[q, d]

    def predict(self, X, qc):
        """dict of float64 arrays: mu, var (T, n_out), jac (T, n_out, D), s_mu (T, n_out) = sum |k*||alpha|, s_jac
        (T, n_out, D) = sum |g||alpha||z - x| / l^2, kappa (T, n_out), kxx (n_out,), red (T, n_out) = k*^T K^-1 k*"""
        p = self.p
        T, n, D = X.shape[0], p.n_out, p.D
        out = dict(mu=np.empty((T, n)), var=np.empty((T, n)), jac=np.empty((T, n, D)), s_mu=np.empty((T, n)),
                   s_jac=np.empty((T, n, D)), kappa=np.empty((T, n)), red=np.empty((T, n)), kxx=p.sf2.copy())
        for q in np.unique(qc):
            t = np.flatnonzero(qc == q)
            zi = np.asarray(p.Z[self.idx[q]], dtype=LD)
            xq = np.asarray(X[t], dtype=LD)
            for d in range(n):
                l, alpha, kappa = self.block(q, d)
                k, g = kernel_ld(p.kern, xq, zi, p.ls[d], p.sf2[d])               # (t, b)
                v = solve_lower_ld(l, k.T)                                        # (b, t)
                red = np.sum(v * v, axis=0)
                l2 = np.asarray(p.ls[d], dtype=LD) ** 2
                dx = (xq[:, None, :] - zi[None, :, :]) / l2[None, None, :]        # (t, b, D)
                ga = g * alpha[None, :]
                out["mu"][t, d] = k.dot(alpha)
                out["var"][t, d] = LD(p.sf2[d]) - red
                out["red"][t, d] = red
                out["jac"][t, d] = np.einsum("tb,tbj->tj", ga, dx)
                out["s_mu"][t, d] = np.abs(k).dot(np.abs(alpha))
                out["s_jac"][t, d] = np.einsum("tb,tbj->tj", np.abs(ga), np.abs(dx))
                out["kappa"][t, d] = kappa
        return out

    def coverage(self, X, qc, Np, limit=64):
        """Does every (256-column block, 128-row chunk) pair of the padded U^-1 matter to at least one query?  For the
        first `limit` queries and every output: v = U^-T k* from the long-double block factor scattered to the padded indices
        of its points (the dense upper factor of a permuted block-diagonal matrix is, on a cluster's indices, the factor of
        that cluster's block), and for every pair the change of |v|^2 = k*^T K^-1 k* when the pair's share of v is dropped,
        relative to |v|^2.  Returns the (n_out, column blocks, chunks) array of the largest such change over the queries;
        pairs above the diagonal (chunk past the column block) hold no entry of U^-1 and are NaN."""
        p = self.p
        off = Np - p.N
        ncb, nch = -(-Np // COLBLOCK), Np // CHUNK
        first = (off // 16 * 16) // CHUNK                                         # chunks of nothing but padding
        best = np.zeros((p.n_out, ncb, nch))
        inv = {}
        for t in range(min(limit, X.shape[0])):
            q = int(qc[t])
            pad = self.idx[q] + off
            chunk, cb = pad // CHUNK, pad // COLBLOCK
            for d in range(p.n_out):
                if (q, d) not in inv:
                    l = self.block(q, d)[0]
                    inv[q, d] = solve_lower_ld(l, np.eye(l.shape[0], dtype=LD)).astype(np.float64)   # L^-1 = U^-T
                k, _ = kernel_ld(p.kern, X[t:t + 1], p.Z[self.idx[q]], p.ls[d], p.sf2[d])
                m = inv[q, d] * k[0].astype(np.float64)[None, :]                  # m[i, k] = U^-1[k, i] k*_k
                v = m.sum(axis=1)
                tot = float(v.dot(v))
                for j in np.unique(chunk):
                    share = m[:, chunk == j].sum(axis=1)                          # the chunk's share of every v_i
                    change = 2 * v * share - share * share
                    for b in np.unique(cb):
                        best[d, b, j] = max(best[d, b, j], abs(change[cb == b].sum()) / tot)
        for b in range(ncb):
            best[:, b, min(nch, 2 * b + 2):] = np.nan
        best[:, :, :first] = np.nan
        return best


_CACHE = {}


def cached(seed, N, D, n_out, kern):
    """(Problem, Ref) shared between the tests of one process"""
    key = (seed, N, D, n_out, kern)
    if key not in _CACHE:
        prob = Problem(*key)
        _CACHE[key] = (prob, Ref(prob))
    return _CACHE[key]


def queries_for(ref, T, seed=0):
    """queries of the first seed from `seed` on whose reference results meet the two cheap data conditions (two or three
    queries at up to two lengthscales from a centre can all lie outside their clusters): X, qc, predict(X, qc).  Decided on the
    reference side alone."""
    for s in range(seed, seed + 50):
        X, qc = ref.p.queries(T, s)
        res = ref.predict(X, qc)
        if np.median(res["var"] / res["kxx"][None, :]) < 0.5 and \
                np.abs(res["jac"]).max() >= 1e-3 * np.abs(res["mu"]).max() / ref.p.ls.max():
            return X, qc, res
    raise AssertionError("no seed gives queries near the data")


def bars(ref, res):
    """(bar_mu (T, n), bar_var (T, n), bar_jac (T, n, D)) of a predict() result: the bars of the module docstring, and never
    above the project's bars of DESIGN 6 (mu, J: 1e-12 sigma_f |alpha|_1 of the whole model; sigma^2: 1e-9 sigma_f^2).  The
    variance bar must lie below the project's by itself (asserted); a model of one or two clusters has so short an |alpha|_1
    that 1e-12 sigma_f |alpha|_1 is the smaller of the two for mu and J, and the smaller one is what is returned."""
    p = ref.p
    c = (3 * ref.b + 40) * U53 * res["kappa"]
    a1 = np.array([sum(float(np.abs(ref.block(q, d)[1]).sum()) for q in range(p.c)) for d in range(p.n_out)])
    old_mu = 1e-12 * np.sqrt(p.sf2) * a1
    bar_var = c * res["kxx"][None, :]
    assert np.all(bar_var <= 1e-9 * p.sf2[None, :]), "variance bar above the project's 1e-9 sigma_f^2"
    bar_mu = np.minimum(c * res["s_mu"], old_mu[None, :])
    bar_jac = np.minimum(c[:, :, None] * res["s_jac"], old_mu[None, :, None])
    assert np.all(bar_mu > 0) and np.all(bar_jac > 0)
    return bar_mu, bar_var, bar_jac


def data_conditions(ref, res, X, qc, Np, need_coverage):
    """the conditions the data must meet for a test on it to mean something; asserts, returns the smallest coverage"""
    p = ref.p
    assert np.median(res["var"] / res["kxx"][None, :]) < 0.5, "queries too far from the data"
    assert np.abs(res["jac"]).max() >= 1e-3 * np.abs(res["mu"]).max() / p.ls.max(), "flat mean: the Jacobian checks nothing"
    if not need_coverage:
        return None
    cov = ref.coverage(X, qc, Np)
    worst = np.nanmin(cov)
    assert worst >= 1e-6, "a (column block, chunk) pair of U^-1 matters to no query: %s" % (np.argwhere(cov < 1e-6)[:4],)
    return float(worst)
