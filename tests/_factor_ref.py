"""Long-double reference of the STORED MODEL -- U^-1 (`Wt`), alpha, log det, K^-1 -- that sr_gp_factorize and sr_gp_append leave
behind, exact at any number of training points, and the a-priori bars of the tests that use it (tests/test_gpu_model_state.py,
tests/test_factor_ref_host.py).  NumPy only.  The data, the kernel and the long-double algebra are those of
tests/_posterior_ref.py (imported, not restated).

WHY IT IS EXACT.  _posterior_ref.Problem puts point i into cluster i mod c, the clusters 40 lengthscales apart: the Gram matrix
is a permuted block-diagonal matrix to 1e-278 (rbf) / 4e-32 (mat52) of the signal variance.  The permutation keeps the order
inside every cluster (and Problem.grown appends behind the existing rows, so that stays true after any sequence of appends), hence
  * the dense upper factor U (K = U^T U) restricted to a cluster's indices is the factor L_c^T of that cluster's block K_c,
  * so are U^-1 = L_c^-T =: W_c, alpha = K_c^-1 y_c and K^-1 = W_c W_c^T; log det K is the sum over the clusters,
  * every other entry of U^-1 is zero, and the front padding of the padded model is the identity.
A hand-written long-double Cholesky of blocks of at most 90 rows (more after appends: a cluster grows by what joins it) is the
stored model.  tests/test_factor_ref_host.py compares it with a dense long-double factorisation at N = 300.

BARS (a priori; nothing here was measured on a device).  u = 2^-53, b the cluster's size, kappa = cond_2(K_c), lambda_min its
smallest eigenvalue, c_b = 3 b + 40 as in _posterior_ref:
    U^-1, cluster entries   c_b u kappa |W_c|_2,         |W_c|_2 = lambda_min^-1/2
    alpha                   c_b u kappa |alpha_c|_2
    log det                 2 N c_b u kappa                (absolute; b, kappa: the largest over the clusters)
    K^-1, cluster entries   2 c_b u kappa |K_c^-1|_2,    |K_c^-1|_2 = 1 / lambda_min
The computed factor is the exact factor of K + dK with |dK| <= gamma_{3b+1} |U^T||U| (Higham, Accuracy and Stability, Th. 10.3),
and to first order dW = -W up(W^T dK W) (up: the upper triangle, the diagonal halved), so |dW| <= |W| kappa |dK| / |K|.  The
explicit inversion's own error and the five-ulp kernel entries sit under the + 40, as in _posterior_ref.  After `a` append calls
since the last fit every bar is multiplied by 1 + a: each append is one more backward-stable step of the same kind on the
factor it is handed.  A REMOVED point counts like an append call (FactorRef(prob, appends=a): a = append calls + removed points
since the last fit): sr_gp_remove applies the product of the Givens rotations of the column pairs (q, k) to the factor it is
handed, written as x'_k = a_k x_k - b_k d_k with a_k = p_k / p_{k+1} <= 1 and |b_k d_k| = |w_k| |d_k| / (p_k p_{k+1}) <= |x|_2 (Cauchy-
Schwarz on d_k = sum w_l x_l, |w_{q..k-1}|_2 = p_k) -- an orthogonal transformation of every row, backward stable like the
rotations themselves (Higham, Th. 19.10: a perturbation of gamma_{c n} |x|_2 per row, below one Cholesky's c_b u kappa |W|_2).
After removals the reference is FactorRef(prob.without(rows)): _posterior_ref.Problem.without says why it stays exact.
LEAVE-ONE-OUT (sr_gp_loo; FactorRef.loo): var_j = 1 / k_jj with k = K_c^-1, mu_j = y_j - alpha_j var_j.  An error dk of k_jj moves
var_j by -dk / k_jj^2 to first order, so |dvar_j| <= bar_kinv var_j^2; mu_j moves by -dalpha_j var_j - alpha_j dvar_j, so
|dmu_j| <= bar_alpha var_j + |alpha_j| bar_kinv var_j^2.  (k_jj = |row j of W_c|^2 is summed from entries under bar_w: 2 |W_c|_2
bar_w = bar_kinv, the K^-1 bar itself; y_j is data.)
DENSE PROBLEM (dense_problem): the recipe of one cluster without the cap of 90 points -- all N points in one box of 3
lengthscales, one block of size b = N, the same formulas.  Every row of U^-1 then depends on every other, so a removal transforms
every row (on the clustered data only the ~90 rows of the retired point's cluster change; the others are shifted).
EXACT VALUES (no bar): the strict lower triangle is 0.0, the front padding is the identity, the bands between padding and real
rows are 0.0.  OFF-CLUSTER entries inside the real rows: |w| <= OFF_REL |W| with |W| the largest |W_c|_2 and OFF_REL = 1e-200
(rbf) / 1e-24 (mat52): the cross-cluster kernel bounds of _posterior_ref's docstring (1e-278, 4e-32) times kappa^2 < 1e6 and the
number of terms, with room.  The same relative bound holds for K^-1.

The comparisons are made in float64 against the reference rounded to float64 (2^-53 relative: a fortieth of the smallest bar).
"""
import numpy as np

import _posterior_ref as R

LD = R.LD
U53 = R.U53
NB = 128                          # rows of a factor block (SR_NB)
MAX_CLUSTERS = 192                # N <= 17280: the largest model of the tests has 16500 rows
OFF_REL = {"rbf": 1e-200, "mat52": 1e-24}


def problem(seed, N, D, n_out, kern="rbf"):
    return R.Problem(seed, N, D, n_out, kern, max_clusters=MAX_CLUSTERS)


def dense_problem(seed, N, D, n_out, kern="rbf"):
    """all N points in ONE cluster (module docstring, DENSE PROBLEM); its FactorRef is a dense long-double Cholesky"""
    return R.Problem(seed, N, D, n_out, kern, cap=N)


def noise_per_output(prob, step=0.01):
    """a copy of prob with the noise variance 0.05 + d * step on output d (Problem gives every output the same, so a fit that
    read another output's noise would go unnoticed): the field noise_variance, and nugget as the library sums it"""
    import copy
    p = copy.copy(prob)
    p.noise_variance = R.NOISE_VARIANCE + step * np.arange(prob.n_out)
    p.nugget = p.noise_variance + R.NOISE_DIAG + R.GPY_JITTER
    return p


def hyp_of(prob):
    """the list SimpleGPModel takes: prob.hyp, with the noise variances of noise_per_output where prob carries them"""
    nv = getattr(prob, "noise_variance", None)
    return prob.hyp if nv is None else [dict(h, noise_variance=float(v)) for h, v in zip(prob.hyp, nv)]


class FactorRef(object):
    """the stored model of a Problem, block by block.  appends: append calls since the last fit (the bars' factor 1 + a)."""

    def __init__(self, prob, appends=0):
        self.p = prob
        self.mult = 1.0 + appends
        self.idx = [np.flatnonzero(prob.member == q) for q in range(prob.c)]      # ascending: the order of the dense factor
        self.pos = np.empty(prob.N, dtype=np.int64)                              # position of a point inside its cluster
        for i in self.idx:
            self.pos[i] = np.arange(len(i))
        self._blk = {}

    def block(self, q, d):
        """dict of cluster q, output d.  Long double: W = L^-T (upper), L, alpha, Kinv, piv (diag L); float: kappa, lmin,
        logdet, and the float64 roundings W64, alpha64, Kinv64"""
        if (q, d) not in self._blk:
            p, i = self.p, self.idx[q]
            k, _ = R.kernel_ld(p.kern, p.Z[i], p.Z[i], p.ls[d], p.sf2[d])
            k = (k + k.T) / 2 + LD(p.nugget[d]) * np.eye(len(i), dtype=LD)
            l = R.cholesky_ld(k)
            w = R.solve_lower_ld(l, np.eye(len(i), dtype=LD)).T                   # L^-T
            alpha = R.solve_upper_ld(l, R.solve_lower_ld(l, np.asarray(p.Y[i, d], dtype=LD)[:, None]))[:, 0]
            kinv = w.dot(w.T)
            ev = np.linalg.eigvalsh(k.astype(np.float64))
            self._blk[q, d] = dict(W=w, L=l, alpha=alpha, Kinv=kinv, piv=np.diag(l).copy(), kappa=float(ev[-1] / ev[0]),
                                   lmin=float(ev[0]), logdet=float(2 * np.sum(np.log(np.diag(l)))), b=len(i),
                                   W64=w.astype(np.float64), alpha64=alpha.astype(np.float64), Kinv64=kinv.astype(np.float64))
        return self._blk[q, d]

    # ---- the bars ------------------------------------------------------------------------------------------------------
    def _c(self, blk):
        return self.mult * (3 * blk["b"] + 40) * U53 * blk["kappa"]

    def bar_w(self, q, d):
        blk = self.block(q, d)
        return self._c(blk) / np.sqrt(blk["lmin"])

    def bar_alpha(self, q, d):
        blk = self.block(q, d)
        return self._c(blk) * float(np.sqrt(np.sum(blk["alpha"] ** 2)))

    def bar_kinv(self, q, d):
        blk = self.block(q, d)
        return 2 * self._c(blk) / blk["lmin"]

    def bar_logdet(self, d):
        blks = [self.block(q, d) for q in range(self.p.c)]
        return self.mult * 2 * self.p.N * (3 * max(b["b"] for b in blks) + 40) * U53 * max(b["kappa"] for b in blks)

    def w_norm(self, d):
        return max(self.block(q, d)["lmin"] ** -0.5 for q in range(self.p.c))

    def kappa_max(self, d):
        return max(self.block(q, d)["kappa"] for q in range(self.p.c))

    # ---- the values ----------------------------------------------------------------------------------------------------
    def logdet(self, d):
        return float(sum(self.block(q, d)["logdet"] for q in range(self.p.c)))

    def alpha(self, d):
        out = np.empty(self.p.N)
        for q, i in enumerate(self.idx):
            out[i] = self.block(q, d)["alpha64"]
        return out

    def loo(self, d):
        """leave-one-out posterior of output d from the cluster blocks, float64: (mu, var, bar_mu, bar_var), each (N,) (module
        docstring, LEAVE-ONE-OUT)"""
        N = self.p.N
        mu, var, bmu, bvar = np.empty(N), np.empty(N), np.empty(N), np.empty(N)
        for q, i in enumerate(self.idx):
            blk = self.block(q, d)
            v = 1 / np.diag(blk["Kinv"])
            mu[i] = np.asarray(self.p.Y[i, d], dtype=LD) - blk["alpha"] * v
            var[i] = v
            v64 = v.astype(np.float64)
            bvar[i] = self.bar_kinv(q, d) * v64 ** 2
            bmu[i] = self.bar_alpha(q, d) * v64 + np.abs(blk["alpha64"]) * self.bar_kinv(q, d) * v64 ** 2
        return mu, var, bmu, bvar

    def alpha_ratio(self, alpha):
        """largest |alpha - reference| / bar over outputs and clusters; alpha (n_out, N)"""
        worst = 0.0
        for d in range(self.p.n_out):
            for q, i in enumerate(self.idx):
                worst = max(worst, float(np.abs(alpha[d, i] - self.block(q, d)["alpha64"]).max()) / self.bar_alpha(q, d))
        return worst

    def dense(self, d, Np, what="W"):
        """the padded (Np, Np) matrix U^-1 ("W") or U ("U") of output d in float64 (small models only)"""
        off = Np - self.p.N
        out = np.zeros((Np, Np))
        out[np.arange(off), np.arange(off)] = 1.0
        for q, i in enumerate(self.idx):
            blk = self.block(q, d)
            out[np.ix_(i + off, i + off)] = blk["W64"] if what == "W" else blk["L"].T.astype(np.float64)
        return out

    def check_wt(self, d, rows, Np, band=256):
        """a padded U^-1 of output d against the reference, in bands of rows.  rows(r0, r1) returns rows [r0, r1) as a float64
        array (r1 - r0, Np).  Returns the largest error / bar of each class: "cluster", "off" (off-cluster entries inside the
        real rows, against OFF_REL |W|), and for the classes with exact values the largest absolute deviation: "lower" (the
        strict lower triangle, 0.0), "padding" (the front padding rows: the identity)."""
        p = self.p
        off = Np - p.N
        assert off >= 0
        mp = np.full(Np, -1, dtype=np.int64)
        mp[off:] = p.member
        off_bar = OFF_REL[p.kern] * self.w_norm(d)
        bars = np.array([self.bar_w(q, d) for q in range(p.c)])
        res = dict(cluster=0.0, off=0.0, lower=0.0, padding=0.0)
        for r0 in range(0, Np, band):
            r1 = min(Np, r0 + band)
            got = np.asarray(rows(r0, r1), dtype=np.float64)
            assert got.shape == (r1 - r0, Np)
            assert not np.any(np.isnan(got)), "NaN in U^-1, rows %d .. %d" % (r0, r1)
            rr = np.arange(r0, r1)
            if r0 > 0:
                res["lower"] = max(res["lower"], float(np.abs(got[:, :r0]).max()))
            sub = got[:, r0:]                                                     # columns from the band's first row on
            low = np.arange(r0, Np)[None, :] < rr[:, None]
            if low.any():
                res["lower"] = max(res["lower"], float(np.abs(sub[low]).max()))
            npad = max(0, min(off, r1) - r0)                                      # padding rows of the band (the first ones)
            if npad:
                eye = (np.arange(r0, Np)[None, :] == rr[:npad, None]).astype(np.float64)
                res["padding"] = max(res["padding"], float(np.abs(sub[:npad] - eye).max()))
            if npad == r1 - r0:
                continue
            real = sub[npad:]
            rreal = rr[npad:]
            ref = np.zeros_like(real)
            barm = np.full(real.shape, off_bar)
            iscl = np.zeros(real.shape, dtype=bool)
            for q in np.unique(mp[rreal]):
                blk = self.block(q, d)
                mine = np.flatnonzero(mp[rreal] == q)                             # the band's rows of cluster q
                cols = self.idx[q] + off
                keep = cols >= r0
                pr = self.pos[rreal[mine] - off]
                at = np.ix_(mine, cols[keep] - r0)
                ref[at] = blk["W64"][np.ix_(pr, np.flatnonzero(keep))]
                barm[at] = bars[q]
                iscl[at] = True
            ratio = np.abs(real - ref) / barm
            up = np.arange(r0, Np)[None, :] >= rreal[:, None]
            res["cluster"] = max(res["cluster"], float(ratio[iscl & up].max()))
            rest = up & ~iscl
            if rest.any():
                res["off"] = max(res["off"], float(ratio[rest].max()))
        return res

    def check_inv_k(self, d, kinv):
        """an (N, N) K^-1 of output d (sr_gp_inv_k) against the reference: largest error / bar on the cluster entries and, on
        the others, largest |entry| / (OFF_REL |K^-1|)"""
        p = self.p
        assert kinv.shape == (p.N, p.N) and not np.any(np.isnan(kinv))
        seen = np.zeros((p.N, p.N), dtype=bool)
        res = dict(cluster=0.0, off=0.0)
        for q, i in enumerate(self.idx):
            at = np.ix_(i, i)
            res["cluster"] = max(res["cluster"], float(np.abs(kinv[at] - self.block(q, d)["Kinv64"]).max()) / self.bar_kinv(q, d))
            seen[at] = True
        if not seen.all():
            res["off"] = float(np.abs(kinv[~seen]).max()) / (OFF_REL[p.kern] * self.w_norm(d) ** 2)
        return res

    # ---- conditions on the data ----------------------------------------------------------------------------------------
    def tile_conditions(self, d, Np):
        """smallest over the 128 x 128 tiles of the upper block triangle of the largest |entry| of the tile, relative to the
        matrix' largest entry: (for U, for U^-1).  Asserts both >= 1e-3: every tile of the factor and of its inverse holds
        an entry a wrong tile would show in."""
        off = Np - self.p.N
        nb = Np // NB
        out = []
        for key in ("U", "W"):
            tm = np.zeros(nb * nb)
            pad = np.arange(off) // NB
            tm[pad * nb + pad] = 1.0
            for q, i in enumerate(self.idx):
                blk = self.block(q, d)
                a = np.abs(blk["W64"] if key == "W" else blk["L"].T.astype(np.float64))
                t = (i + off) // NB
                np.maximum.at(tm, (t[:, None] * nb + t[None, :]).ravel(), a.ravel())
            tm = tm.reshape(nb, nb)
            out.append(float(tm[np.triu_indices(nb)].min() / tm.max()))
        assert min(out) >= 1e-3, "a tile of U / U^-1 holds no entry above 1e-3 of the largest: %s" % (out,)
        return tuple(out)

    def update_terms(self, d, Np):
        """smallest over (k, I, J), k < I <= J, of the largest |entry| of the term U[k, I]^T U[k, J] of the trailing updates
        (up to 17 blocks: the dense factor).  Asserts >= 1e-6."""
        nb = Np // NB
        assert nb <= 17
        u = self.dense(d, Np, "U")
        worst = np.inf
        for k in range(nb - 1):
            row = u[k * NB:(k + 1) * NB, (k + 1) * NB:]
            g = np.abs(row.T.dot(row))
            n = nb - k - 1
            tm = g.reshape(n, NB, n, NB).max(axis=(1, 3))
            worst = min(worst, float(tm[np.triu_indices(n)].min()))
        assert worst >= 1e-6, "a term of a trailing update moves its tile by %.3g only" % worst
        return worst


_CACHE = {}


def cached(seed, N, D, n_out, kern, vary_noise=False):
    """(Problem, FactorRef) shared between the tests of one process (the last few); vary_noise: noise_per_output"""
    key = (seed, N, D, n_out, kern, vary_noise)
    if key not in _CACHE:
        while len(_CACHE) >= 6:
            _CACHE.pop(next(iter(_CACHE)))
        prob = problem(*key[:5])
        if vary_noise:
            prob = noise_per_output(prob)
        _CACHE[key] = (prob, FactorRef(prob))
    return _CACHE[key]
