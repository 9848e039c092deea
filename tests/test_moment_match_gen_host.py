"""The NumPy references of the general-family moment matching (tests/_mm_gen_ref.py) held against each other -- CPU only.

* the closed form (a) against tensor Gauss-Hermite quadrature (b) of the posterior computed from the plain kernel formula, at
  every parameter corner and input covariance kind.  NODES = 32 per dimension, found here: doubling the nodes changes (b) by
  1.3e-7 at 16, 5.4e-11 at 24 and 2.7e-14 at 32 over these cases (asserted < 1e-10), so (a) is held to 1e-9 of (b), ten times
  the quadrature's own bar (measured 1.3e-13).  The inputs' standard deviations are halved against the GPU test's (~0.1): at
  0.5 against a lengthscale of 0.35 the quadrature of k M k needs more than 48 nodes;
* (a) at a = b = 0, c0 = 1, v = sf2 against the ARD-RBF reference ``_mm_ref.moment_match`` to 1e-12 relative to the scales of the
  GPU bars (measured: mu and V 3e-17, Cov 1.7e-13);
* (a) in fp64 against (a) in long double on exactly the inputs of tests/test_gpu_moment_match_gen.py (``_mm_gen_cases``): the
  rounding floor its bars rest on.  Every bar must sit at least 10 x above the floor.  Measured here (model fitted in NumPy),
  floor over bar: mu <= 3.4e-4, V <= 1.7e-4, Cov <= 3.2e-2 (corner s1; the covariance kinds 9e-3, N = 300 9e-4, the +5
  translation 1.7e-3).  At noise 1e-3 the Cov floor of N = 300 is 1.6e-10, within 12 x of its bar, which is why the size cases run
  at noise 1e-2 like the rest."""
import numpy as np
import pytest

import _mm_gen_cases as C
import _mm_gen_ref as G
import _mm_ref as R

NODES = 32


def _small(corner, D, kind, n_out=2):
    Z, Y, kp, noise = C.problem(("host", corner, D), 14, D, n_out, corner=corner)
    m, S = C.inputs(("host-q", corner, D, kind), Z, 2, kind)
    par = G.params_from_packed(kp)
    # (standard deviations ~0.1 and never above 0.25: the quadrature of k M k, half the lengthscale, converges at NODES)
    return (par, Z) + G.fit(par, Z, Y, noise) + (m, None if S is None else 0.25 * S)


@pytest.mark.parametrize("kind", C.S_KINDS)
@pytest.mark.parametrize("corner,D", [("dense", 1), ("dense", 2), ("dense", 3), ("s1", 2), ("s1", 3), ("c00", 2), ("b0", 2),
                                      ("a0", 3), ("lin_rbf", 3)])
def test_closed_form_against_quadrature(corner, D, kind):
    """s with zeros (the RBF on one dimension only), c0 = 0, b = 0, outputs with different parameters; S zero, rank 1
    (singular) and full"""
    par, Z, alpha, M, m, S = _small(corner, D, kind)
    for t in range(len(m)):
        St = None if S is None else S[t]
        mu, cov, V, _ = G.moment_match(par, Z, alpha, M, m[t], St)
        q1 = G.quadrature(par, Z, alpha, M, m[t], St, NODES)
        q2 = G.quadrature(par, Z, alpha, M, m[t], St, 2 * NODES)
        conv = max(np.abs(x - y).max() for x, y in zip(q1, q2))
        SV = np.zeros_like(V.T) if St is None else St.dot(V.T)
        err = max(np.abs(mu - q1[0]).max(), np.abs(cov - q1[1]).max(), np.abs(SV - q1[2]).max())
        print("quadrature %s D=%d %s: doubling the nodes %.1e, closed form against it %.1e" % (corner, D, kind, conv, err))
        assert conv < 1e-10
        assert err < 1e-9
    if kind != "zero":
        assert np.abs(cov[0, 1]) > 1e-9                    # the cross-covariance is informative


def test_singular_input_covariance_with_zero_rows():
    """an S whose rows and columns of the RBF dimension are zero, and one that is zero everywhere else: the conditioning form
    and the quadrature must agree where S + Lam is formed on one dimension only"""
    par, Z, alpha, M, m, _ = _small("lin_rbf", 3, "zero")
    for keep in ([0, 2], [1]):
        S = np.zeros((3, 3))
        g = np.array([0.3, -0.2, 0.25])
        S[np.ix_(keep, keep)] = np.outer(g[keep], g[keep]) + 0.01 * np.eye(len(keep))
        mu, cov, V, _ = G.moment_match(par, Z, alpha, M, m[0], S)
        q = G.quadrature(par, Z, alpha, M, m[0], S, NODES)
        err = max(np.abs(mu - q[0]).max(), np.abs(cov - q[1]).max(), np.abs(S.dot(V.T) - q[2]).max())
        print("singular S on %s: %.1e" % (keep, err))
        assert err < 1e-9


@pytest.mark.parametrize("kind", C.S_KINDS)
def test_rbf_corner_is_the_ard_rbf_reference(kind):
    Z, Y, kp, noise = C.problem(("host-rbf",), 30, 3, 2, corner="rbf")
    m, S = C.inputs(("host-rbf-q", kind), Z, 3, kind)
    par = G.params_from_packed(kp)
    alpha, M = G.fit(par, Z, Y, noise)
    ls, sf2 = 1.0 / par["s"], par["v"]
    for t in range(len(m)):
        St = None if S is None else S[t]
        mu, cov, V, (mu_scale, kxx) = G.moment_match(par, Z, alpha, M, m[t], St)
        ref = R.moment_match(Z, alpha, M, ls, sf2, m[t], St)
        # relative to the scales of the bars: sum_i |alpha_ai| max_i |E k_ai| for mu and V, the prior variance for Cov (Cov
        # itself is what a cancellation against the prior leaves: its own size is no measure of the rounding)
        for name, x, y, scale in (("mu", mu, ref[0], mu_scale), ("cov", cov, ref[1], kxx.max()), ("V", V, ref[2], mu_scale[:, None])):
            rel = (np.abs(x - y) / scale).max()
            print("rbf corner %s %s: %.1e" % (kind, name, rel))
            assert rel < 1e-12, name


def floors(case):
    """(floor, bar) of mu, V and Cov: fp64 against long double of reference (a), and the GPU test's absolute bars"""
    Z, Y, kp, noise, m, S = case
    par = G.params_from_packed(kp)
    alpha, M = G.fit(par, Z, Y, noise)
    mu, cov, V, (mu_scale, kxx) = G.moment_match_batch(par, Z, alpha, M, m, S)
    lmu, lcov, lV, _ = G.moment_match_batch(par, Z, alpha, M, m, S, dtype=np.longdouble)
    at = 1e-12 * mu_scale                                  # per query and output
    ct = 1e-9 * kxx.max(axis=1)                            # per query
    return (float((np.abs(mu - lmu) / at).max()), float((np.abs(V - lV) / at[:, :, None]).max()),
            float((np.abs(cov - lcov) / ct[:, None, None]).max()))


def test_rounding_floor_under_the_gpu_bars():
    """every comparison of the GPU test: the reference alone, fp64 against long double, stays 10 x under each absolute bar"""
    worst = [0.0, 0.0, 0.0]
    for tag, case in C.all_cases():
        r = floors(case)
        print("floor / bar  %-22s mu %.1e V %.1e cov %.1e" % ((tag,) + r))
        worst = [max(w, x) for w, x in zip(worst, r)]
        assert max(r) <= 0.1, tag
    print("worst floor / bar: mu %.1e V %.1e cov %.1e" % tuple(worst))
