"""The Jacobian of the posterior function samples on the device (sr_gp_paths_eval_grad / _step_grad, sample_paths /
paths_step_device with jacobians=True, sample_n_step_jacobians) against the NumPy reference tests/_paths_grad_ref.py -- every
element of J, on the problems of test_gpu_paths at the edges where padding, tiles, chunks and the compiled widths can go wrong.

Tolerance (the rule of test_gpu_paths applied to J, nothing invented): e0 = the largest difference of J_ref between the
reference's two solve routes (Cholesky, LU), scale = max |J_ref|, bar = max(20 e0, 1e-12 scale sqrt(N + M)).  Every case
prints e0, the device's error, the bar and the margin (profiles/r13_paths_grad.txt).

Every test here fails on the parent commit: the symbols and the keywords do not exist there."""
import numpy as np
import pytest

from _helpers import oracle_model, mu_atol
import _paths_ref as pr
import _paths_grad_ref as pg
import test_gpu_paths as tg
from test_gpu_paths import _problem, _gp, _draw, _np, SR_EINVAL, SR_ESTATE, SR_EUNSUPPORTED

pytestmark = pytest.mark.gpu

# (N, S, M, T, D, n_out, chunk): the cases of test_gpu_paths and D below / at every compiled width (3, 5, 8)
CASES = list(tg.CASES) + [(64, 16, 16, 16, 2, 1, None), (64, 16, 16, 16, 4, 2, None), (64, 16, 16, 16, 7, 1, None)]
BIG = (300, 129, 100, 300, 3, 2)


def _jref(p, fn, x):
    a, b = (fn(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][r]) for r in ("chol", "lu"))
    e0, scale = float(np.abs(a - b).max()), float(np.abs(a).max())
    return a, e0, scale, max(20.0 * e0, 1e-12 * scale * np.sqrt(p["N"] + p["M"]))


def _report(what, case, e0, err, bar):
    print("paths grad %-5s N=%d S=%d M=%d T=%d D=%d n_out=%d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
          % ((what,) + tuple(case[:6]) + (e0, err, bar, bar / max(err, 1e-300))))


def _check(gp, p, case, tag=""):
    """J of both calls against the reference (every element), F bit for bit that of the calls without Jacobians"""
    S, D, n_out = p["S"], p["D"], p["n_out"]
    T = p["x"].shape[0]
    F, J = gp.sample_paths(p["x"], jacobians=True)
    assert F.shape == (T, S, n_out) and J.shape == (T, S, n_out, D)
    ref, e0, scale, bar = _jref(p, pg.evaluate_grad, p["x"])
    err = float(np.abs(J - ref).max())
    _report("eval" + tag, case, e0, err, bar)
    Fs, Js = (_np(t) for t in gp.paths_step_device(p["xs"], jacobians=True))
    assert Fs.shape == (S, n_out) and Js.shape == (S, n_out, D)
    sref, se0, sscale, sbar = _jref(p, pg.step_grad, p["xs"])
    serr = float(np.abs(Js - sref).max())
    _report("step" + tag, case, se0, serr, sbar)
    Jd = gp.sample_paths(p["xs"], jacobians=True)[1][np.arange(S), np.arange(S)]
    derr = float(np.abs(Js - Jd).max())
    print("paths grad diag  |step - eval[s, s]| = %.3e  bar = %.3e" % (derr, 1e-12 * sscale))
    assert np.all(np.isfinite(J)) and np.all(np.isfinite(Js))
    np.testing.assert_array_equal(F, gp.sample_paths(p["x"]))
    np.testing.assert_array_equal(Fs, _np(gp.paths_step_device(p["xs"])))
    assert err <= bar
    assert serr <= sbar
    assert derr <= 1e-12 * sscale


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-S%d-M%d-T%d-D%d-o%d" % c[:6])
def test_eval_grad_and_step_grad_against_the_reference(case):
    N, S, M, T, D, n_out, chunk = case
    p = _problem(N, S, M, T, D, n_out)
    gp = _gp(p)
    if chunk:
        gp.set_chunk(chunk)
    _draw(gp, p)
    _check(gp, p, case)


def test_closed_loop_step_grad_keeps_f_and_z_next():
    p = _problem(*BIG)
    gp = _gp(p)
    _draw(gp, p)
    rng = np.random.default_rng(3)
    kfb, kff = 0.3 * rng.standard_normal((1, 2)), 0.1 * rng.standard_normal(1)
    F0, z0 = gp.paths_step_device(p["xs"], kfb, kff)
    F1, z1, J1 = gp.paths_step_device(p["xs"], kfb, kff, jacobians=True)
    np.testing.assert_array_equal(_np(F0), _np(F1))
    np.testing.assert_array_equal(_np(z0), _np(z1))
    np.testing.assert_array_equal(_np(J1), _np(gp.paths_step_device(p["xs"], jacobians=True)[1]))


def test_translated_inputs():
    """Z, x and xs shifted by +30 in every dimension, against the reference at the shifted inputs: an algebra that expands
    z - x around a far centre loses its digits here, the explicit differences do not"""
    base = _problem(*BIG)
    key = BIG + ("shift30",)
    if key not in tg._CACHE:
        p = dict(base, Z=base["Z"] + 30.0, x=base["x"] + 30.0, xs=base["xs"] + 30.0)
        p["c"] = {r: pr.coeffs(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"], p["omega"], p["tau"], p["w"], p["eps"], r)
                  for r in ("chol", "lu")}
        tg._CACHE[key] = p
    p = tg._CACHE[key]
    gp = _gp(p)
    gp.set_chunk(128)
    _draw(gp, p)
    _check(gp, p, BIG, tag="+30")


def test_zero_draws_give_the_mean_jacobian():
    p = _problem(*BIG)
    gp = _gp(p)
    _draw(gp, p, w=0 * p["w"], eps=0 * p["eps"])
    _, J = gp.sample_paths(p["x"], jacobians=True)
    _, Js = gp.paths_step_device(p["xs"], jacobians=True)
    jac = gp.predict(p["x"][:, :2], p["x"][:, 2:], jacobians=True)[2]
    jac_s = gp.predict(p["xs"][:, :2], p["xs"][:, 2:], jacobians=True)[2]
    assert jac.shape == J.shape[:1] + J.shape[2:]
    om = oracle_model(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"])
    atol = mu_atol(om) / p["ls"].min()
    for s in range(p["S"]):
        np.testing.assert_allclose(J[:, s], jac, rtol=1e-9, atol=atol)
    np.testing.assert_allclose(_np(Js), jac_s, rtol=1e-9, atol=atol)


def _raw_eval_grad(gp, x, n_alloc, sentinel=None, with_f=True):
    """sr_gp_paths_eval_grad through the raw symbol into a J buffer of n_alloc doubles: (rc, J as NumPy)"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    xt = B.as_dev(x, hd.device)
    S = max(1, gp.paths_count()[0])
    F = B.empty((x.shape[0], S, hd.n_out), hd.device)
    J = torch.full((n_alloc,), float(sentinel if sentinel is not None else 0.0), dtype=torch.float64, device=hd.device)
    rc = lib.sr_gp_paths_eval_grad(hd.h, B.ptr(xt), x.shape[0], B.ptr(F) if with_f else None, B.ptr(J), B.stream_ptr(hd.device))
    return rc, _np(J)


def test_bitwise_repeatable_chunks_sentinel_and_shared_workspace():
    p = _problem(*BIG)
    gp = _gp(p)
    T, S, D, n_out = p["x"].shape[0], p["S"], p["D"], p["n_out"]
    x1000 = np.random.default_rng(5).uniform(-1, 1, (1000, 3))
    mu0, var0 = gp.predict(x1000)
    outs = []
    for _ in range(2):
        _draw(gp, p)
        outs.append((gp.sample_paths(p["x"], jacobians=True)[1], _np(gp.paths_step_device(p["xs"], jacobians=True)[1])))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    J0 = outs[0][0]
    ref, e0, scale, bar = _jref(p, pg.evaluate_grad, p["x"])
    # the shared workspace: a predict of 1000 queries in between changes neither predict nor J
    mu1, var1 = gp.predict(x1000)
    np.testing.assert_array_equal(mu0, mu1)
    np.testing.assert_array_equal(var0, var1)
    np.testing.assert_array_equal(gp.sample_paths(p["x"], jacobians=True)[1], J0)
    # nothing behind T S n_out D doubles is written; F == NULL gives the same J
    n = T * S * n_out * D
    for with_f in (True, False):
        rc, buf = _raw_eval_grad(gp, p["x"], n + 64, sentinel=-7.25, with_f=with_f)
        assert rc == 0
        np.testing.assert_array_equal(buf[:n].reshape(J0.shape), J0)
        np.testing.assert_array_equal(buf[n:], np.full(64, -7.25))
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    ns = S * n_out * D
    Jb = torch.full((ns + 64,), -7.25, dtype=torch.float64, device=hd.device)
    Fb = B.empty((S, n_out), hd.device)
    assert lib.sr_gp_paths_step_grad(hd.h, B.ptr(B.as_dev(p["xs"], hd.device)), B.ptr(Fb), B.ptr(Jb), None, None, None,
                                     B.stream_ptr(hd.device)) == 0
    np.testing.assert_array_equal(_np(Jb)[:ns].reshape(S, n_out, D), outs[0][1])
    np.testing.assert_array_equal(_np(Jb)[ns:], np.full(64, -7.25))
    # another chunk size: equal to 1e-13 relative
    gp.set_chunk(77)
    J77 = gp.sample_paths(p["x"], jacobians=True)[1]
    assert np.abs(J77 - J0).max() <= 1e-13 * scale
    assert np.abs(J77 - ref).max() <= bar
    gp.release_scratch()                                # frees the workspaces, not the paths
    assert gp.paths_count() == (p["S"], p["M"])
    np.testing.assert_array_equal(gp.sample_paths(p["x"], jacobians=True)[1], J77)
    np.testing.assert_array_equal(_np(gp.paths_step_device(p["xs"], jacobians=True)[1]), outs[0][1])


def _rc(gp, x):
    return _raw_eval_grad(gp, x, x.shape[0] * max(1, gp.paths_count()[0]) * gp._handle.n_out * gp._handle.D)[0]


def _check_against(gp, p):
    ref, e0, scale, bar = _jref(p, pg.evaluate_grad, p["x"])
    assert np.abs(gp.sample_paths(p["x"], jacobians=True)[1] - ref).max() <= bar
    sref, _, _, sbar = _jref(p, pg.step_grad, p["xs"])
    assert np.abs(_np(gp.paths_step_device(p["xs"], jacobians=True)[1]) - sref).max() <= sbar


def _coeffs(q):
    return {r: pr.coeffs(q["Z"], q["Y"], q["ls"], q["sf2"], q["noise_var"], q["omega"], q["tau"], q["w"], q["eps"], r)
            for r in ("chol", "lu")}


def test_states_and_errors():
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    p = _problem(200, 40, 32, 9, 3, 2)
    gp = _gp(p)
    hd = gp._handle
    st = B.stream_ptr(hd.device)
    xs = B.as_dev(p["xs"], hd.device)
    Ft, Jt = B.empty((p["S"], 2), hd.device), B.empty((p["S"], 2, 3), hd.device)

    def step_rc():
        return lib.sr_gp_paths_step_grad(hd.h, B.ptr(xs), B.ptr(Ft), B.ptr(Jt), None, None, None, st)

    assert _rc(gp, p["x"]) == SR_ESTATE and step_rc() == SR_ESTATE          # before any draw
    with pytest.raises(RuntimeError):
        gp.sample_paths(p["x"], jacobians=True)
    _draw(gp, p)
    _check_against(gp, p)
    xq = B.as_dev(p["x"], hd.device)
    Fq = B.empty((9, p["S"], 2), hd.device)
    assert lib.sr_gp_paths_eval_grad(hd.h, B.ptr(xq), 9, B.ptr(Fq), None, st) == SR_EINVAL         # NULL J
    assert lib.sr_gp_paths_eval_grad(hd.h, B.ptr(xq), -1, B.ptr(Fq), B.ptr(Jt), st) == SR_EINVAL   # T = -1
    assert lib.sr_gp_paths_eval_grad(hd.h, None, 0, None, B.ptr(Jt), st) == 0                      # T == 0: a no-op
    assert lib.sr_gp_paths_step_grad(hd.h, B.ptr(xs), B.ptr(Ft), None, None, None, None, st) == SR_EINVAL
    # a broken closed-loop triple
    assert lib.sr_gp_paths_step_grad(hd.h, B.ptr(xs), B.ptr(Ft), B.ptr(Jt), B.ptr(Ft), None, None, st) == SR_EINVAL
    # ... and all three set on a model with D == n_out (no n_u)
    p2 = _problem(40, 8, 8, 3, 2, 2)
    g2 = _gp(p2)
    _draw(g2, p2)
    h2 = g2._handle
    x2, F2, z2 = B.as_dev(p2["xs"], h2.device), B.empty((8, 2), h2.device), B.empty((8, 2), h2.device)
    J2 = B.empty((8, 2, 2), h2.device)
    kf = B.as_dev(np.zeros(4), h2.device)
    assert lib.sr_gp_paths_step_grad(h2.h, B.ptr(x2), B.ptr(F2), B.ptr(J2), B.ptr(kf), B.ptr(kf), B.ptr(z2),
                                     B.stream_ptr(h2.device)) == SR_EINVAL
    with pytest.raises(ValueError):
        g2.paths_step_device(p2["xs"], np.zeros((1, 2)), np.zeros(1), jacobians=True)
    _check_against(g2, p2)

    # a refit invalidates; a new draw works against a refit reference
    q = _problem(200, 40, 32, 9, 3, 2, seed=77)
    gp.update_model(q["Z"], q["Y"], opt_hyp=False, replace_old=True)
    assert gp.paths_count() == (0, 0) and _rc(gp, p["x"]) == SR_ESTATE and step_rc() == SR_ESTATE
    q = dict(q, ls=p["ls"], sf2=p["sf2"])                             # (the model keeps its hyper-parameters)
    q["c"] = _coeffs(q)
    _draw(gp, q)
    _check_against(gp, q)
    # removal
    gp.remove_data([3, 150])
    assert gp.paths_count() == (0, 0) and _rc(gp, p["x"]) == SR_ESTATE and step_rc() == SR_ESTATE
    keep = np.delete(np.arange(200), [3, 150])
    r = dict(q, Z=q["Z"][keep], Y=q["Y"][keep], eps=q["eps"][:, :, keep], N=198)
    r["c"] = _coeffs(r)
    _draw(gp, r)
    _check_against(gp, r)


def test_in_place_append_invalidates():
    N = 600
    full = _problem(N + 1, 16, 32, 5, 3, 2)
    p = dict(full, Z=full["Z"][:N], Y=full["Y"][:N], eps=full["eps"][:, :, :N], N=N)
    p["c"] = _coeffs(p)
    gp = _gp(p)
    gp.append_limit = 10 ** 9
    _draw(gp, p)
    _check_against(gp, p)
    gp.update_model(full["Z"][N:], full["Y"][N:], opt_hyp=False, replace_old=False)
    assert gp._handle.N == N + 1
    assert gp.paths_count() == (0, 0) and _rc(gp, p["x"]) == SR_ESTATE
    _draw(gp, full)
    _check_against(gp, full)


def test_unsupported_models():
    from safe_exploration_amd import SimpleGPModel, _buffers as B
    from safe_exploration_amd._lib import lib, check
    from _helpers import width_problem, width_gp
    rng = np.random.default_rng(0)

    def rcs(g, D, n_out):
        hd = g._handle
        x = B.as_dev(rng.uniform(-1, 1, (4, D)), hd.device)
        F, J = B.empty((4, 4, n_out), hd.device), B.empty((4, 4, n_out, D), hd.device)
        st = B.stream_ptr(hd.device)
        return (lib.sr_gp_paths_eval_grad(hd.h, B.ptr(x), 4, B.ptr(F), B.ptr(J), st),
                lib.sr_gp_paths_step_grad(hd.h, B.ptr(x), B.ptr(F), B.ptr(J), None, None, None, st))

    # sparse: Wt is not the factor of K_y
    p = _problem(200, 40, 32, 9, 3, 2)
    hyp = [{"lengthscale": p["ls"][d], "variance": p["sf2"][d], "noise_variance": 1e-2} for d in range(2)]
    Zu = p["Z"][:32].copy()
    sp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, Z=Zu)
    sp.do_sparse_gp = True
    sp.train(p["Z"], p["Y"], 32, opt_hyp=False, Z=Zu)
    assert rcs(sp, 3, 2) == (SR_ESTATE, SR_ESTATE)
    # general family, and D = 9
    for kt, D in (("mat52", 3), ("rbf", 9)):
        g = width_gp(width_problem(11, kt, D, 60, 2))
        rc = rcs(g, D, 2)
        assert rc == (SR_EUNSUPPORTED, SR_EUNSUPPORTED)
        for r in rc:                                     # what the Python surface makes of the status
            with pytest.raises(NotImplementedError):
                check(r)


def test_consistent_rollout_jacobians():
    """n_s = 2, n_u = 1, N = 60, 3 steps, 70 particles, M = 64: S_all bit for bit that of sample_n_step(consistent=True), A_all
    against rollout_grad by the bar rule per step.  (The Jacobians come from a method of their own, sample_n_step_jacobians:
    tests/test_paths_host.py pins the parameter list of sample_n_step, so it takes no further keyword.)"""
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    n_s, n_u, N, n, S, M = 2, 1, 60, 3, 70, 64
    p = _problem(N, S, M, 1, n_s + n_u, n_s)
    gp = _gp(p, n_u=n_u)
    rng = np.random.default_rng(9)
    K = 0.3 * rng.standard_normal((n, n_u, n_s))
    k = 0.1 * rng.standard_normal((n, n_u))
    x0 = rng.uniform(-0.5, 0.5, (n_s, 1))
    mc = MonteCarloSafetyVerification(gp)
    _draw(gp, p)
    S0, S_all0 = mc.sample_n_step(x0, K, k, n=n, n_samples=S, consistent=True, n_features=M)
    S1, S_all, A_all = mc.sample_n_step_jacobians(x0, K, k, n=n, n_samples=S, consistent=True, n_features=M)
    assert gp.paths_count() == (S, M) and A_all.shape == (n, S, n_s, n_s)
    np.testing.assert_array_equal(S_all, S_all0)
    np.testing.assert_array_equal(S1, S0)
    (_, Aa), (_, Ab) = (pg.rollout_grad(x0[:, 0], K, k, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][r])
                        for r in ("chol", "lu"))
    for i in range(n):
        e0, scale = float(np.abs(Aa[i] - Ab[i]).max()), float(np.abs(Aa[i]).max())
        bar = max(20.0 * e0, 1e-12 * scale * np.sqrt(N + M))
        err = float(np.abs(A_all[i] - Aa[i]).max())
        print("paths grad rollout step %d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f" % (i, e0, err, bar, bar / max(err, 1e-300)))
        assert err <= bar
    with pytest.raises(ValueError):
        mc.sample_n_step_jacobians(x0, K, k, n=n, n_samples=S, consistent=False)
