"""The per-query kernels of csrc/sr_ellipsoid_dev.h / csrc/sr_ellipsoid.hip in isolation, every compiled instance, against the
long-double reference of tests/_ellipsoid_ref.py (which tests/test_ellipsoid_ref_host.py checks on the CPU first):

    sr_ellipsoid_kernel<n_s, n_u>   8 x 4 instances   ellipsoid_step_batch (mode 0), moment_step_batch (modes 1, 2)
    sr_remainder_kernel<n_s, n_u>   8 x 4 instances   compute_remainder_overapproximations_batch
    sr_distance_kernel<n_s>         8 instances       distance_to_center_batch, shared and per-ellipsoid samples
    sr_safety_kernel                n_s = 1 .. 8      lin_ellipsoid_safety_distance_batch
    sr_sample_kernel                                  sr_gp_sample, the entry SimpleGPModel.sample_device launches it through
                                                      (called with mu and var of the test's own: no GP in front of it)

Every batch is T = 257 queries: a full 256-thread block and a one-thread tail.  The shape matrices come in families
(_ellipsoid_ref.shape_matrices), each crossed with feedback gains of scale 0, 0.3 and 1e3 in thirds of the batch:

    random      A A^T / n_s, A normal                       all_equal   O diag(1 + 1e-13 N(0,1)) O^T
    diag        diag(U(0.1, 2))    (gain 0: off == 0        graded      O diag(logspace(-12, 4, n_s)) O^T
    identity    0.37 I              on entry to the solver) tiny, huge  random times 1e-100, 1e+100
    rank1       v v^T                                       rounded     random, one ulp added below the diagonal
    twin_top    O diag(1, 1 + 1e-14, U(0.01, 0.5) ...) O^T  (n_s >= 2)

The scale sweep stops at 1e+-100: `off` and `dia` of the Jacobi stopping rule are sums of squares, which underflow for
|M_ij| below about 1e-154 -- where the remainder box n_s (l_mu r^2)^2 has underflowed as well and the step is non-finite
anyway (the range of validity is stated beside the stopping rule in sr_ellipsoid_dev.h).  Q = 0 is not a case either: the
reference project divides by a zero trace there.  (`tiny` / `huge` scale l_mu by 1e+100 / 1e-100 and var by 1e-100 / 1e+100 beside q:
every term stays finite; the box of the mean remainder then dominates (tiny) or vanishes (huge) beside the other two terms.)

TOLERANCES (stated once, in _ellipsoid_ref):   p1: rtol 1e-12 + 8 eps p1_abs;   q1: rtol 1e-12 + 16 n_s eps q1_abs, where
q1_abs bounds the terms an entry is summed from -- it forgives the cancellation of off-diagonal entries and nothing else
(below 1e-3 of max |q1| for every query, asserted on the host);   remainders: rtol 1e-12;   distance: rtol 64 u cond(q), at
least 1e-12;   safety distance: rtol 1e-12 + 8 eps (|h| |p| + c sqrt(h Q h^T) + |h_vec|);   samples: rtol 1e-14.
Every entry is called twice and must return the same bits.

ATTAINABLE: tests/test_ellipsoid_ref_host.py holds the fp64 oracle to the same tolerances on the same inputs.  Three kinds of
input had to be drawn so that ANY fp64 evaluation can meet them (the reasons are with the generators in _ellipsoid_ref):
gains of `rank1` and `graded` keep a row with |cos| >= 0.1 to the dominant direction of q; v of the `rank1` safety cases keeps
|cos(h_m, v)| >= 0.05; the sampling inputs have mixed signs but sums that do not cancel.  u in the distance tolerance is the
unit roundoff 2^-53, which keeps it below 1e-6 at cond(q) = 1e8.

WHAT THE KERNELS USE OF THEM, measured on an MI355X (test_error_table prints this with -s): per entry and family, the worst
error of a query relative to its largest entry, and the largest share of the tolerance any entry used (1 = at the bound):

    entry                        family     worst rel    share of tolerance
    distance per_t               graded     8.06e-09     0.011
    distance per_t               random     8.30e-08     0.016
    distance shared              graded     8.06e-09     0.011
    distance shared              random     8.30e-08     0.016
    moments meaneq p1            (all)      2.85e-14     0.046
    moments meaneq point p1      (all)      2.85e-14     0.046
    moments meaneq point q1      graded     0.00e+00     0.000
    moments meaneq point q1      random     0.00e+00     0.000
    moments meaneq point q1      rank1      0.00e+00     0.000
    moments meaneq q1            graded     1.59e-14     0.008
    moments meaneq q1            random     2.29e-14     0.009
    moments meaneq q1            rank1      1.70e-14     0.006
    moments taylor p1            (all)      2.85e-14     0.046
    moments taylor point p1      (all)      2.85e-14     0.046
    moments taylor point q1      graded     0.00e+00     0.000
    moments taylor point q1      random     0.00e+00     0.000
    moments taylor point q1      rank1      0.00e+00     0.000
    moments taylor q1            graded     7.14e-15     0.008
    moments taylor q1            random     7.99e-15     0.012
    moments taylor q1            rank1      1.09e-14     0.015
    remainder                    all_equal  2.88e-13     0.288
    remainder                    diag       9.47e-16     0.001
    remainder                    graded     1.08e-14     0.011
    remainder                    huge       2.46e-15     0.003
    remainder                    identity   8.01e-16     0.001
    remainder                    random     3.28e-15     0.003
    remainder                    rank1      5.38e-15     0.005
    remainder                    rounded    2.70e-15     0.003
    remainder                    tiny       2.42e-15     0.002
    remainder                    twin_top   5.16e-15     0.005
    safety m=1                   random     1.55e-13     0.036
    safety m=1                   rank1      7.84e-14     0.028
    safety m=2n_s                random     3.61e-16     0.034
    safety m=2n_s                rank1      5.76e-16     0.118
    sample S                     T=1        2.01e-16     0.022
    sample S                     T=257      2.21e-16     0.022
    sample z                     T=1        3.08e-16     0.035
    sample z                     T=257      4.45e-16     0.044
    step ell a=b=None p1         (all)      0.00e+00     0.000
    step ell a=b=None q1         random     5.10e-15     0.008
    step ell p1                  (all)      3.50e-14     0.056
    step ell q1                  all_equal  5.27e-14     0.070
    step ell q1                  diag       1.52e-15     0.008
    step ell q1                  graded     2.14e-14     0.021
    step ell q1                  huge       1.29e-15     0.010
    step ell q1                  identity   1.30e-15     0.008
    step ell q1                  random     4.97e-15     0.012
    step ell q1                  rank1      1.07e-14     0.015
    step ell q1                  rounded    4.79e-15     0.008
    step ell q1                  tiny       4.79e-15     0.006
    step ell q1                  twin_top   1.54e-15     0.008
    step point a=b=None p1       (all)      0.00e+00     0.000
    step point a=b=None q1       random     5.16e-16     0.001
    step point p1                (all)      2.85e-14     0.030
    step point q1                random     5.16e-16     0.001
"""
import functools

import numpy as np
import pytest

import _ellipsoid_ref as er

pytestmark = pytest.mark.gpu

INSTANCES = [(n_s, n_u) for n_s in range(1, 9) for n_u in range(1, 5)]
MOMENT_FAMILIES = ("random", "graded", "rank1")
TABLE = {}                         # (entry, family) -> [worst normwise relative error, largest share of the tolerance used]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _twice(call):
    """call() twice: the same bits both times.  Returns the first result (a tuple of arrays, or one array)."""
    one, two = call(), call()
    for x, y in zip(one if isinstance(one, tuple) else (one,), two if isinstance(two, tuple) else (two,)):
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), "two calls of one entry differ"
    return one


def _hold(entry, family, got, want, rtol, atol=0.0):
    """got within rtol |want| + atol, entry by entry; the figures go to TABLE first"""
    got = np.asarray(got)
    assert got.shape == want.shape, (entry, family, got.shape, want.shape)
    share = er.used(got, want, rtol, atol)
    T = want.shape[0]
    with np.errstate(invalid="ignore"):
        rel = np.abs(got - want).reshape(T, -1).max(axis=1) / np.abs(want).reshape(T, -1).max(axis=1)
    rel = float(np.nanmax(rel)) if np.isfinite(got).all() else np.inf
    row = TABLE.setdefault((entry, family), [0.0, 0.0])
    row[0], row[1] = max(row[0], rel), max(row[1], share)
    assert share <= 1.0, "%s / %s: %.3g of the tolerance used (worst relative error of a query %.3g)" % (entry, family, share, rel)


@functools.lru_cache(maxsize=None)
def _ref_step(n_s, n_u, family, branch, mode, lin):
    return er.step_batch(er.cases(n_s, n_u)[family], branch, mode, lin)


def _hold_step(entry, family, n_s, got, ref, T=None):
    sl = slice(0, T)
    _hold(entry + " p1", "(all)", got[0], ref["p1"][sl], er.RTOL, er.p1_atol(ref["p1_abs"][sl]))
    _hold(entry + " q1", family, got[1], ref["q1"][sl], er.RTOL, er.q1_atol(n_s, ref["q1_abs"][sl]))


# ---- sr_ellipsoid_kernel, mode 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u", INSTANCES)
def test_ellipsoid_step(n_s, n_u):
    """the ellipsoid branch on every family; the point branch on `random`, with and without a linear model, also at T = 1 and
    T = 256, and its q1 exactly diagonal"""
    from safe_exploration_amd import gp_reachability as reach
    cs = er.cases(n_s, n_u)

    def run(c, ell, lin, T=None):
        sl = slice(0, T)
        a, b = (c["a"], c["b"]) if lin else (None, None)
        q, k_fb = (c["q"][sl], c["k_fb"][sl]) if ell else (None, None)
        return _twice(lambda: reach.ellipsoid_step_batch(c["p"][sl], c["k_ff"][sl], c["mu"][sl], c["var"][sl], c["jac"][sl],
                                                         c["l_mu"], c["l_sigma"], q, k_fb, c["c"], a, b, check_bounds=True))

    for family, c in cs.items():
        _hold_step("step ell", family, n_s, run(c, True, True), _ref_step(n_s, n_u, family, "ell", 0, True))
    c = cs["random"]
    _hold_step("step ell a=b=None", "random", n_s, run(c, True, False), _ref_step(n_s, n_u, "random", "ell", 0, False))
    off = ~np.eye(n_s, dtype=bool)
    for lin in (True, False):
        for T in (None, 1, 256):
            got = run(c, False, lin, T)
            _hold_step("step point" + ("" if lin else " a=b=None"), "random", n_s, got,
                       _ref_step(n_s, n_u, "random", "point", 0, lin), T)
            assert (got[1][:, off] == 0.0).all(), "q1 of the point branch is not exactly diagonal"


# ---- sr_ellipsoid_kernel, modes 1 and 2 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u", INSTANCES)
def test_moment_step(n_s, n_u):
    """TAYLOR and MEAN_EQUIVALENT, with and without sigma_x; the mean-equivalent result must not depend on jac: None, NaN and
    the case's own Jacobians give the same bits"""
    from safe_exploration_amd import uncertainty_propagation_casadi as prop
    cs = er.cases(n_s, n_u)

    def run(c, mode, with_sigma, jac):
        sx, k_fb = (c["q"], c["k_fb"]) if with_sigma else (None, None)
        return _twice(lambda: prop.moment_step_batch(c["p"], c["k_ff"], c["mu"], c["var"], jac, sx, k_fb, c["a"], c["b"], mode))

    for family in MOMENT_FAMILIES:
        c = cs[family]
        for mode, tag in ((prop.TAYLOR, "taylor"), (prop.MEAN_EQUIVALENT, "meaneq")):
            for with_sigma in (True, False):
                got = run(c, mode, with_sigma, c["jac"])
                ref = _ref_step(n_s, n_u, family, "ell" if with_sigma else "point", int(mode), True)
                _hold_step("moments %s%s" % (tag, "" if with_sigma else " point"), family, n_s, got, ref)
                if mode == prop.MEAN_EQUIVALENT or not with_sigma:
                    for jac in (None, np.full_like(c["jac"], np.nan)):
                        other = run(c, mode, with_sigma, jac)
                        assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(got, other)), \
                            "the result depends on jac where the mode does not read it"


# ---- sr_remainder_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u", INSTANCES)
def test_remainder_overapproximations(n_s, n_u):
    from safe_exploration_amd import utils
    for family, c in er.cases(n_s, n_u).items():
        um, us = _twice(lambda: utils.compute_remainder_overapproximations_batch(c["q"], c["k_fb"], c["l_mu"], c["l_sigma"]))
        r_um, r_us = er.remainder_batch(c)
        _hold("remainder", family, um, r_um, er.RTOL)
        _hold("remainder", family, us, r_us, er.RTOL)


# ---- sr_distance_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", range(1, 9))
def test_distance_to_center(n_s):
    from safe_exploration_amd import utils_ellipsoid as ue
    for family, dc in er.distance_cases(n_s).items():
        for per_t in (False, True):
            want, cond = er.distance_batch(dc, per_t)
            rtol = er.distance_rtol(cond)
            if family == "graded":
                assert rtol.max() < 1e-6
            got = _twice(lambda: ue.distance_to_center_batch(dc["per_t"] if per_t else dc["shared"], dc["p"], dc["q"]))
            _hold("distance " + ("per_t" if per_t else "shared"), family, got, want, rtol[:, None])


# ---- sr_safety_kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", range(1, 9))
def test_safety_distance(n_s):
    from safe_exploration_amd import gp_reachability as reach
    for m in (1, 2 * n_s):
        for family, sc in er.safety_cases(n_s, m).items():
            want, d_abs = er.safety_batch(sc)
            got = _twice(lambda: reach.lin_ellipsoid_safety_distance_batch(sc["p"], sc["q"], sc["h_mat"], sc["h_vec"], sc["c"]))
            _hold("safety m=%s" % ("1" if m == 1 else "2n_s"), family, got, want, er.RTOL, er.safety_atol(d_abs))


# ---- sr_sample_kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [1, 4, 8])
@pytest.mark.parametrize("n_u", [1, 4])
def test_sampling_step(n_out, n_u):
    """T * size = 257 both ways round; with and without the next inputs z"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    dev = torch.device("cuda", 0)
    for T, size in ((257, 1), (1, 257)):
        sc = er.sample_case(n_out, n_u, T, size)
        want_S, want_z = er.sample_batch(sc)
        mu, var, eps = B.as_dev(sc["mu"], dev), B.as_dev(sc["var"], dev), B.as_dev(sc["eps"], dev)
        k_fb, k_ff = B.as_dev(sc["k_fb"], dev), B.as_dev(sc["k_ff"], dev)

        def run(with_z):
            S = torch.full((T, size, n_out), float("nan"), dtype=torch.float64, device=dev)
            z = torch.full((T, size, n_out + n_u), float("nan"), dtype=torch.float64, device=dev) if with_z else None
            check(lib.sr_gp_sample(dev.index, T, size, n_out, n_u if with_z else 0, B.ptr(mu), B.ptr(var), B.ptr(eps), B.ptr(S),
                                   B.ptr(k_fb if with_z else None), B.ptr(k_ff if with_z else None), B.ptr(z),
                                   B.stream_ptr(dev)))
            return (B.to_numpy(S), B.to_numpy(z)) if with_z else B.to_numpy(S)

        S, z = _twice(lambda: run(True))
        _hold("sample S", "T=%d" % T, S, want_S, er.RTOL_SAMPLE)
        _hold("sample z", "T=%d" % T, z, want_z, er.RTOL_SAMPLE)
        S_only = _twice(lambda: run(False))
        assert np.array_equal(S_only.view(np.int64), S.view(np.int64))


# ---- the violation counter ---------------------------------------------------------------------------------------------------
BAD = (0, 7, 255, 256, 257, 298, 299)           # both thread blocks of T = 300, their first and last threads


@pytest.mark.parametrize("n_s,n_u", [(1, 1), (2, 3), (3, 2), (8, 4)])
def test_bad_boxes_are_counted_once_per_query(n_s, n_u):
    """7 chosen queries of 300 have a zero-width box: var = 0 in the point branch (in one dimension for some, in all for the
    others), a zero shape matrix (v = 0 in v v^T, so l_mu r^2 == 0 in every dimension) in the ellipsoid branch.  The message
    must name 7 -- queries, not dimensions -- and the repaired batch must pass."""
    from safe_exploration_amd import gp_reachability as reach
    c = {k: (np.concatenate((v, v[:43])) if isinstance(v, np.ndarray) and v.shape[:1] == (er.T_CASE,) else v)
         for k, v in er.cases(n_s, n_u)["rank1"].items()}
    bad = np.array(BAD)

    def run(var, q):
        k_fb = None if q is None else c["k_fb"]
        return reach.ellipsoid_step_batch(c["p"], c["k_ff"], c["mu"], var, c["jac"], c["l_mu"], c["l_sigma"], q, k_fb, c["c"],
                                          c["a"], c["b"], check_bounds=True)

    var0 = c["var"].copy()
    var0[bad[::2]] = 0.0
    var0[bad[1::2], n_s - 1] = 0.0
    q0 = c["q"].copy()
    q0[bad] = 0.0
    for var, q in ((var0, None), (c["var"], q0)):
        with pytest.raises(AssertionError, match=r"\(7 query"):
            run(var, q)
        run(c["var"], None if q is None else c["q"])


# ---- the figures -------------------------------------------------------------------------------------------------------------
def test_error_table():
    """prints what the tests above measured (run the whole file with -s); asserts nothing of its own"""
    entries = sorted({e for e, _ in TABLE})
    print("\n%-28s %-10s %-12s %s" % ("entry", "family", "worst rel", "share of tolerance"))
    for e in entries:
        for (ee, f), (rel, share) in sorted(TABLE.items()):
            if ee == e:
                print("%-28s %-10s %-12.2e %.3f" % (e, f, rel, share))
