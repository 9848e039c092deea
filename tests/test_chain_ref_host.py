"""CPU tests of tests/_chain_ref.py, the long-double reference of whole multi-step chains that tests/test_gpu_chain_family.py
holds the device to: it reproduces the fp64 oracle's chain and the reference project's own recorded chains, its bars stay below
what the existing chain test grants against the oracle on every case of the table, and the data of every case can tell a
broken chain from a correct one.  The floor and the response of every case are printed (pytest -s)."""
import numpy as np
import pytest

import _chain_ref as C
from conftest import load_golden
from oracle import oracle_np as orc

LD = np.longdouble


def _golden_model(g, n_u):
    return C.Model.from_arrays(g["Z"], g["Y"], g["lengthscale"], g["signal_var"], g["noise_var"] + 1e-8, n_u)


@pytest.mark.parametrize("n_s,n_u,N,with_q0", [(2, 1, 200, False), (2, 1, 200, True), (3, 2, 129, True)])
def test_reference_reproduces_the_oracle_chain(n_s, n_u, N, with_q0):
    """oracle_np.multistep_reachability_batch (fp64, explicit inverse, scipy's eigenvalues) on the same model and inputs"""
    m, T, H = C.model(n_s, n_u, N), 6, 7
    x = C.inputs(n_s, n_u, T, H)
    beta, inv_K, _ = orc.gp_fit(m.Z, m.Y, m.ls, m.sf2, m.noise + 1e-5)
    om = dict(Z=m.Z, beta=beta, inv_K=inv_K, lengthscale=m.ls, signal_var=m.sf2)
    rp, rq = orc.multistep_reachability_batch(om, x["p"], x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], x["q"] if with_q0 else None,
                                              x["c"], x["a"], x["b"], x["k_fb0"] if with_q0 else None)
    ro = C.rollout(m, x, H, range(T))
    p, q, _ = C.chain(m, x, H, range(T), "q0" if with_q0 else "point", ro)
    np.testing.assert_allclose(p.astype(np.float64), rp, rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(q.astype(np.float64), rq, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("name,n_u", [("reach_pend.npz", 1)])
def test_reference_reproduces_the_recorded_reachability_chains(name, n_u):
    """the reference project's multi_step_reachability on numbers (tests/golden), at the tolerances of
    test_onestep_and_multistep_vs_reference_golden"""
    g = load_golden(name)
    m = _golden_model(g, n_u)
    Tm, H = g["ms_p0"].shape[0], g["ms_k_ff"].shape[1]
    x = dict(p=g["ms_p0"], k_ff=g["ms_k_ff"], k_fb=g["ms_k_fb"], q=g["Q"][:Tm], k_fb0=g["k_fb"][:Tm], a=g["a_lin"], b=g["b_lin"],
             l_mu=g["l_mu"], l_sigma=g["l_sigma"], c=float(g["c_safety"]))
    ro = C.rollout(m, x, H, range(Tm))
    for variant, tag in (("point", ""), ("q0", "_q0")):
        p, q, _ = C.chain(m, x, H, range(Tm), variant, ro)
        np.testing.assert_allclose(p.astype(np.float64), g["ms_p_all" + tag], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(q.astype(np.float64), g["ms_q_all" + tag], rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("name,n_u", [("moments_pend.npz", 1), ("moments_cart.npz", 1)])
def test_reference_reproduces_the_recorded_moment_chains(name, n_u):
    """the reference project's multi_step_taylor_symbolic / mean_equivalent_multistep on numbers, at the tolerances of
    test_moment_propagation_vs_reference_golden"""
    g = load_golden(name)
    m = _golden_model(g, n_u)
    T, H = g["mu0"].shape[0], g["k_ff"].shape[1]
    x = dict(p=g["mu0"], k_ff=g["k_ff"], k_fb=g["k_fb"], a=g["a_lin"], b=g["b_lin"], l_mu=None, l_sigma=None, c=1.0)
    ro = C.rollout(m, x, H, range(T))
    for variant, tag in (("m1", "taylor"), ("m2", "meaneq")):
        mu, sig, gv = C.chain(m, x, H, range(T), variant, ro)
        np.testing.assert_allclose(mu.astype(np.float64), g["mu_" + tag], rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(sig.astype(np.float64), g["sigma_" + tag], rtol=1e-7, atol=1e-13)
        if tag == "meaneq":
            np.testing.assert_allclose(gv.astype(np.float64), g["gpvar_meaneq"], rtol=0, atol=1e-9)


def test_fp64_twin_of_the_reference_modules_is_fp64_and_the_default_is_unchanged():
    """the dtype argument added to _posterior_ref / _ellipsoid_ref: float64 in, float64 out; the default still long double"""
    import _ellipsoid_ref as R
    import _posterior_ref as P
    rng = np.random.default_rng(3)
    A = rng.standard_normal((5, 5))
    K = A.dot(A.T) + 5 * np.eye(5)
    for dt in (LD, np.float64):
        l = P.cholesky_ld(K, dt) if dt is not LD else P.cholesky_ld(np.asarray(K, dtype=LD))
        assert l.dtype == dt and P.solve_lower_ld(l, K, dt).dtype == dt and P.solve_upper_ld(l, K, dt).dtype == dt
        assert P.kernel_ld("rbf", A, A, np.ones(5), 1.0, dt)[0].dtype == dt
        np.testing.assert_allclose((l.dot(l.T)).astype(np.float64), K, rtol=1e-14)
    c = R.cases(3, 2)["random"]
    args = (c["p"][0], c["q"][0], c["k_ff"][0], c["k_fb"][0], c["mu"][0], c["var"][0], c["jac"][0], c["l_mu"], c["l_sigma"], c["c"],
            c["a"], c["b"])
    for mode in (0, 1, 2):
        o, o64 = R.step(*args, mode=mode), R.step(*args, mode=mode, dtype=np.float64)
        assert o["q1"].dtype == LD and o64["q1"].dtype == np.float64 and o64["p1"].dtype == np.float64
        np.testing.assert_allclose(o64["q1"], o["q1"].astype(np.float64), rtol=1e-12)


def test_launch_arithmetic_matches_the_documented_examples():
    """csrc/sr_capi_chain.hip: 768 roll-outs of a pendulum model with N <= 256 and 416 of a cart-pole model (N <= 256) in one
    launch on a device that leaves 240 workgroups; H_max of the LDS control block"""
    assert 16 * C.gmax(256, 2, 1, 15) == 768 and 16 * C.gmax(256, 4, 1, 6) == 416
    assert C.h_max(3, 2) == 24 and C.h_max(4, 1) == 38
    assert C.max_launches(1000, 2) == 1 and C.max_launches(1000, 3) == 2 and C.max_launches(1025, 3) == 6
    assert len(C.family()) == 24 and len({c[0] for c in C.family()}) == 24
    for Np in C.NPS:
        for part in range(Np // 128):
            assert len(np.unique(C.part_rows(Np, part))) == 128
        assert len(np.unique(np.concatenate([C.part_rows(Np, part) for part in range(Np // 128)]))) == Np


_SEEN = {}


@pytest.mark.parametrize("case", C.all_cases(), ids=[c[0] for c in C.all_cases()])
def test_bar_and_data_conditions(case):
    """bar = 30 floor + 2 resp, relative to the largest element of the quantity at that step, stays below 1e-7 (centres) and
    1e-6 (shape matrices; the GP variance relative to sf2): otherwise the data is too ill-conditioned -- change the data.  And
    on the reference alone: every checked trajectory finite, the median sigma^2 / k(x,x) below 0.5, every (output, 128-row part)
    of the padded model carrying more than 1e-3 of some checked sigma^2, q far from under- and overflow."""
    cid, m, T, H, variant, rows = case
    x = _SEEN.setdefault((m.n_s, m.n_u, T, H), C.inputs(m.n_s, m.n_u, T, H))
    r = C.reference(m, x, H, rows, variant, key=(id(m), T, H, tuple(rows)))
    rel_p, rel_q = r["bar_p"] / r["scale_p"], r["bar_q"] / r["scale_q"]
    rel_v = r["bar_var"] / m.sf2.max()
    print("%s: floor p %.1e q %.1e var %.1e | resp p %.1e q %.1e var %.1e | bar p %.1e q %.1e var %.1e (relative)" % (
        cid, (r["floor_p"] / r["scale_p"]).max(), (r["floor_q"] / r["scale_q"]).max(), r["floor_var"].max() / m.sf2.max(),
        (r["resp_p"] / r["scale_p"]).max(), (r["resp_q"] / r["scale_q"]).max(), r["resp_var"].max() / m.sf2.max(),
        rel_p.max(), rel_q.max(), rel_v.max()))
    assert np.all(r["bar_p"] > 0) and np.all(r["bar_q"] > 0) and np.all(r["bar_var"] > 0)
    assert rel_p.max() < C.P_LIMIT, "centres: bar %.2e of the step's largest element" % rel_p.max()
    assert rel_q.max() < C.Q_LIMIT, "shape matrices: bar %.2e of the step's largest element" % rel_q.max()
    assert rel_v.max() < C.Q_LIMIT, "GP variance: bar %.2e of sf2" % rel_v.max()
    assert np.isfinite(r["p"]).all() and np.isfinite(r["q"]).all() and np.isfinite(r["var"]).all()
    diag = np.diagonal(r["q"], axis1=2, axis2=3)
    assert diag.min() > 1e-30 and np.abs(r["q"]).max() < 1e30, "q under- or overflows over H = %d steps" % H
    dc = C.data_conditions(m, x, H, rows)
    assert dc["ratio"] < 0.5, "median sigma^2 / k(x,x) = %.3f: the variance contraction does not matter" % dc["ratio"]
    assert dc["coverage"].min() > 1e-3, "a 128-row part matters to no checked query: %s" % (dc["coverage"],)
