"""The long-double reference of tests/_ellipsoid_ref.py, checked without a GPU before anything on the device is held to it:

  * it reproduces the reference project's recorded outputs (tests/golden) at the tolerances test_gpu_parity.py holds the
    kernels to on the same files, and the fp64 oracle on all 32 (n_s, n_u) instances of the `random` family;
  * its lambda_max agrees with a 50-digit mpmath eigenvalue to 1e-15 on every input family;
  * ATTAINABILITY: the fp64 oracle (oracle/oracle_np.py, SciPy's non-symmetric eigvals -- a less favourable algorithm than the
    kernel's symmetric one) stays inside every tolerance of tests/test_gpu_ellipsoid_family.py on every query of every
    family.  A correct fp64 implementation can therefore pass, and a failure on the GPU is the kernel's.  Two families
    needed their inputs changed for this (see _ellipsoid_ref._gain_that_sees_the_top_direction and safety_cases);
  * the absolute term of the q1 tolerance stays below 1e-3 of max |q1| for every query, so it forgives the cancellation in
    off-diagonal entries and nothing else.
"""
import numpy as np
import pytest

import _ellipsoid_ref as er
from conftest import load_golden
from oracle import oracle_np as orc

INSTANCES = [(n_s, n_u) for n_s in range(1, 9) for n_u in range(1, 5)]


# ---- recorded outputs of the reference project -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reach_pend.npz", "reach_cart.npz", "reach_n3u2.npz"])
def test_reference_reproduces_the_recorded_steps(name):
    g = load_golden(name)
    case = dict(p=g["p"], q=g["Q"], k_ff=g["k_ff"], k_fb=g["k_fb"], mu=g["mu"], var=g["var"], jac=g["jac"], l_mu=g["l_mu"],
                l_sigma=g["l_sigma"], c=float(g["c_safety"]), a=g["a_lin"], b=g["b_lin"])
    for tag, lin in (("id", False), ("lin", True)):
        r = er.step_batch(case, "point", lin=lin)
        np.testing.assert_allclose(r["p1"], g["p1_point_" + tag], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(r["q1"], g["q1_point_" + tag], rtol=1e-12, atol=1e-16)
        r = er.step_batch(case, "ell", lin=lin)
        np.testing.assert_allclose(r["p1"], g["p1_ell_" + tag], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(r["q1"], g["q1_ell_" + tag], rtol=1e-12, atol=1e-15)
        assert not r["bad"].any()
    d = np.array([er.safety(g["p1_ell_id"][t], g["q1_ell_id"][t], g["h_mat"], g["h_vec"], case["c"])[0]
                  for t in range(len(g["p"]))]).astype(np.float64)
    np.testing.assert_allclose(d, g["d_safety"], rtol=1e-12, atol=1e-14)


def test_reference_reproduces_the_anchor():
    g = load_golden("anchor.npz")
    l, flat = g["l"], lambda x: np.reshape(x, -1)
    args = (flat(g["mu"]), flat(g["var"]), g["jac"], l, l, 2.0)
    r = er.step(flat(g["p"]), None, flat(g["k_ff"]), None, *args, None, None)
    np.testing.assert_allclose(r["p1"].astype(float), flat(g["p_point"]), rtol=1e-13)
    np.testing.assert_allclose(r["q1"].astype(float), np.diag([0.08, 0.32]), rtol=1e-13)
    r = er.step(flat(g["p"]), g["Q"], flat(g["k_ff"]), g["k_fb"], *args, None, None)
    np.testing.assert_allclose(r["p1"].astype(float), flat(g["p_ell"]), rtol=1e-13)
    np.testing.assert_allclose(r["q1"].astype(float), g["q_ell"], rtol=1e-12)
    d, _ = er.safety(r["p1"], r["q1"], np.vstack((np.eye(2), -np.eye(2))), np.ones(4), 1.0)
    np.testing.assert_allclose(d.astype(float), flat(g["d_safety"]), rtol=1e-12)
    r = er.step(flat(g["p"]), g["Q"], flat(g["k_ff"]), g["k_fb"], *args, g["a2"], g["b2"])
    np.testing.assert_allclose(r["p1"].astype(float), flat(g["p_lin"]), rtol=1e-13)
    np.testing.assert_allclose(r["q1"].astype(float), g["q_lin"], rtol=1e-12)


def test_reference_reproduces_the_recorded_remainders():
    g = load_golden("remainder.npz")
    for tag in "1234":
        q, k, lm, ls = (g[n + tag] for n in ("q_", "k_fb_", "l_mu_", "l_sigma_"))
        um, us = er.remainder(q, k, lm, ls)
        np.testing.assert_allclose(um.astype(float), g["u_mu_" + tag], rtol=1e-12)
        np.testing.assert_allclose(us.astype(float), g["u_sigma_" + tag], rtol=1e-12)
        um, us = er.remainder(q, 0 * k, lm, ls)
        np.testing.assert_allclose(um.astype(float), g["u_mu_k0_" + tag], rtol=1e-12)
        np.testing.assert_allclose(us.astype(float), g["u_sigma_k0_" + tag], rtol=1e-12)


# ---- the fp64 oracle --------------------------------------------------------------------------------------------------------
def _oracle_step(c, branch="ell", lin=True):
    n_s, n_u = c["p"].shape[1], c["k_ff"].shape[1]
    a, b = (c["a"], c["b"]) if lin else (np.eye(n_s), np.zeros((n_s, n_u)))
    out = [orc.onestep_reachability_from_gp(c["p"][t], c["q"][t] if branch == "ell" else None, c["k_ff"][t], c["k_fb"][t],
                                            c["mu"][t], c["var"][t], c["jac"][t], c["l_mu"], c["l_sigma"], c["c"], a, b)
           for t in range(c["p"].shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _oracle_remainder(c):
    out = [orc.compute_remainder_overapproximations(c["q"][t], c["k_fb"][t], c["l_mu"], c["l_sigma"])
           for t in range(c["q"].shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _oracle_moments(c, mode, with_sigma):
    n_s, T = c["p"].shape[1], c["p"].shape[0]
    out = [orc.one_step_moments(c["p"][t], c["q"][t] if with_sigma else None, c["k_ff"][t], c["k_fb"][t], c["mu"][t],
                                c["var"][t], c["jac"][t], c["a"], c["b"], taylor=(mode == 1)) for t in range(T)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]).reshape(T, n_s, n_s)


@pytest.mark.parametrize("n_s,n_u", INSTANCES)
def test_reference_matches_the_fp64_oracle_on_random(n_s, n_u):
    """rtol 1e-12: alone on the diagonal of q1 and on the remainders, beside the absolute terms of the GPU tests where a sum may
    cancel (p1, the off-diagonal of H Q H^T: two fp64 evaluations in different orders do not agree to a relative 1e-12 there)"""
    c = er.cases(n_s, n_u)["random"]
    for branch in ("ell", "point"):
        for lin in (True, False):
            r = er.step_batch(c, branch, lin=lin)
            p1, q1 = _oracle_step(c, branch, lin)
            diag = np.eye(n_s, dtype=bool)
            assert er.used(p1, r["p1"], 1e-12, er.p1_atol(r["p1_abs"])) <= 1, (branch, lin)
            assert er.used(q1[:, diag], r["q1"][:, diag], 1e-12) <= 1, (branch, lin)
            assert er.used(q1, r["q1"], 1e-12, er.q1_atol(n_s, r["q1_abs"])) <= 1, (branch, lin)
    um, us = er.remainder_batch(c)
    oum, ous = _oracle_remainder(c)
    np.testing.assert_allclose(oum, um, rtol=1e-12)
    np.testing.assert_allclose(ous, us, rtol=1e-12)


# ---- lambda_max against 50 digits -------------------------------------------------------------------------------------------
def _lambda_max_mp(mp, q, k_fb):
    n = q.shape[0]
    qm = mp.matrix([[mp.mpf(float(q[i, j]) + float(q[j, i])) / 2 for j in range(n)] for i in range(n)])
    km = mp.matrix([[mp.mpf(float(x)) for x in row] for row in k_fb])
    L = mp.cholesky(mp.eye(n) + km.T * km)
    return max(mp.eigsy(L.T * qm * L, eigvals_only=True))


@pytest.mark.parametrize("n_s", range(3, 9))
def test_lambda_max_against_50_digits(n_s):
    """two queries of every third of the gains, every family, n_u = 1 and 4: relative error <= 1e-15"""
    mp = pytest.importorskip("mpmath")
    worst = 0.0
    with mp.workdps(50):
        for n_u in (1, 4):
            for name, c in er.cases(n_s, n_u).items():
                for t in (0, 85, 86, 171, 172, 256):
                    want = _lambda_max_mp(mp, c["q"][t], c["k_fb"][t])
                    got = er.lambda_max_qb(c["q"][t], c["k_fb"][t])
                    err = abs(float((mp.mpf(float(got)) + mp.mpf(float(got - er.LD(float(got)))) - want) / want))
                    worst = max(worst, err)
                    assert err <= 1e-15, (n_s, n_u, name, t, err)
    print("n_s=%d worst relative error of lambda_max_qb vs mpmath: %.2e" % (n_s, worst))


# ---- attainability, and the condition on the absolute term -----------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u", INSTANCES)
def test_fp64_oracle_is_inside_the_gpu_tolerances(n_s, n_u):
    for name, c in er.cases(n_s, n_u).items():
        r = er.step_batch(c)
        atol = er.q1_atol(n_s, r["q1_abs"])
        T = atol.shape[0]
        share = atol.reshape(T, -1).max(axis=1) / np.abs(r["q1"]).reshape(T, -1).max(axis=1)
        assert share.max() < 1e-3, (name, share.max())           # the absolute term forgives cancellation, nothing else
        assert not r["bad"].any(), name
        p1, q1 = _oracle_step(c)
        assert er.used(p1, r["p1"], er.RTOL, er.p1_atol(r["p1_abs"])) <= 1, name
        assert er.used(q1, r["q1"], er.RTOL, atol) <= 1, name
        um, us = er.remainder_batch(c)
        oum, ous = _oracle_remainder(c)
        assert er.used(oum, um, er.RTOL) <= 1 and er.used(ous, us, er.RTOL) <= 1, name
        if name in ("random", "graded", "rank1"):
            for mode in (1, 2):
                for with_sigma in (True, False):
                    r = er.step_batch(c, "ell" if with_sigma else "point", mode)
                    atol = er.q1_atol(n_s, r["q1_abs"])
                    assert (atol.reshape(T, -1).max(axis=1) < 1e-3 * np.abs(r["q1"]).reshape(T, -1).max(axis=1)).all()
                    m1, s1 = _oracle_moments(c, mode, with_sigma)
                    assert er.used(m1, r["p1"], er.RTOL, er.p1_atol(r["p1_abs"])) <= 1, (name, mode)
                    assert er.used(s1, r["q1"], er.RTOL, atol) <= 1, (name, mode)


@pytest.mark.parametrize("n_s", range(1, 9))
def test_fp64_oracle_is_inside_the_tolerances_of_the_small_kernels(n_s):
    for name, dc in er.distance_cases(n_s).items():
        for per_t in (False, True):
            d, cond = er.distance_batch(dc, per_t)
            rtol = er.distance_rtol(cond)
            if name == "graded":
                assert rtol.max() < 1e-6
            od = np.array([orc.distance_to_center(dc["per_t"][t] if per_t else dc["shared"], dc["p"][t][:, None], dc["q"][t])
                           for t in range(d.shape[0])])
            assert er.used(od, d, rtol[:, None]) <= 1, (name, per_t)
    for m in (1, 2 * n_s):
        for name, sc in er.safety_cases(n_s, m).items():
            d, d_abs = er.safety_batch(sc)
            od = np.array([orc.lin_ellipsoid_safety_distance(sc["p"][t][:, None], sc["q"][t], sc["h_mat"], sc["h_vec"][:, None],
                                                             sc["c"])[:, 0] for t in range(d.shape[0])])
            assert er.used(od, d, er.RTOL, er.safety_atol(d_abs)) <= 1, (name, m)
    for n_u in (1, 4):
        sc = er.sample_case(n_s, n_u, 257, 1)
        S, z = er.sample_batch(sc)
        oS = sc["mu"][:, None, :] + np.sqrt(sc["var"])[:, None, :] * sc["eps"]
        oz = np.concatenate((oS, oS.dot(sc["k_fb"].T) + sc["k_ff"]), axis=2)
        assert er.used(oS, S, er.RTOL_SAMPLE) <= 1 and er.used(oz, z, er.RTOL_SAMPLE) <= 1
