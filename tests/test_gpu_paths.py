"""Posterior function samples by pathwise conditioning on the device (sr_gp_paths_draw / _eval / _step, SimpleGPModel.draw_paths /
sample_paths / paths_step_device, sample_n_step(consistent=True)) against the NumPy reference tests/_paths_ref.py -- every
element of F, at the edges where padding, tiles and chunks can go wrong.

Tolerance (per case, nothing invented): e0 = the largest difference between the reference's two solve routes (Cholesky, LU),
scale = max |F_ref|, bar = max(20 e0, 1e-12 scale sqrt(N + M)); the factor 20 covers the other summation order over up to
N + M terms and the device's exp / cos.  Every case prints e0, the device's error and the bar (profiles/r12_paths.txt).

Every test here fails on the parent commit: the symbols and the methods do not exist there."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as orc
from _helpers import hip_model, oracle_model, mu_atol
import _paths_ref as pr

pytestmark = pytest.mark.gpu

SR_EINVAL, SR_ESTATE, SR_EUNSUPPORTED = -1, -4, -5

# (N, S, M, T, D, n_out, chunk)
CASES = [
    (1, 1, 1, 1, 1, 1, None),
    (127, 63, 15, 127, 3, 2, None),
    (128, 64, 16, 128, 3, 2, None),
    (129, 65, 17, 129, 5, 4, None),
    (300, 129, 100, 300, 3, 2, 128),          # three chunks
    (300, 200, 256, 1, 8, 1, None),
    (700, 128, 64, 130, 3, 2, None),          # six block rows: multi-block triangular products, a k-range behind real padding
]

_CACHE = {}


def _problem(N, S, M, T, D, n_out, seed=None):
    """Z ~ U[-1,1]^D, sf2 near 1, total diagonal term 1e-2, lengthscales distinct per output and dimension scaled by
    sqrt(D / 3) (as _helpers.width_problem), all draws from default_rng(seed); the reference by both solve routes (cached)."""
    key = (N, S, M, T, D, n_out, seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(1000 * N + S if seed is None else seed)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    noise_var = np.full(n_out, 1e-2 - orc.GPY_JITTER)          # + GPy's jitter = 1e-2 on the diagonal
    p = dict(Z=Z, Y=Y, ls=ls, sf2=sf2, noise_var=noise_var, D=D, n_out=n_out, N=N, S=S, M=M,
             omega=rng.standard_normal((M, D)), tau=rng.uniform(0, 2 * np.pi, M),
             w=rng.standard_normal((n_out, S, M)), eps=rng.standard_normal((n_out, S, N)),
             x=rng.uniform(-1.2, 1.2, (T, D)), xs=rng.uniform(-1.2, 1.2, (S, D)))
    p["c"] = {r: pr.coeffs(Z, Y, ls, sf2, noise_var, p["omega"], p["tau"], p["w"], p["eps"], r) for r in ("chol", "lu")}
    _CACHE[key] = p
    return p


def _ref(p, fn, x):
    a, b = (fn(x, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][r]) for r in ("chol", "lu"))
    e0 = float(np.abs(a - b).max())
    scale = float(np.abs(a).max())
    return a, e0, scale, max(20.0 * e0, 1e-12 * scale * np.sqrt(p["N"] + p["M"]))


def _gp(p, n_u=None):
    from safe_exploration_amd import SimpleGPModel
    from _helpers import hyp_from
    D, n_out = p["D"], p["n_out"]
    if n_u is None:
        n_u = 1                                # (as _helpers.width_gp: D = 1 is one action and no state input)
    gp = SimpleGPModel(n_out, D - n_u, n_u, kern_types=["rbf"] * n_out, hyp=hyp_from(p["ls"], p["sf2"], p["noise_var"]))
    gp.train(p["Z"], p["Y"], opt_hyp=False)
    return gp


def _draw(gp, p, **over):
    d = dict(omega=p["omega"], tau=p["tau"], w=p["w"], eps=p["eps"])
    d.update(over)
    gp.draw_paths(p["S"], p["M"], **d)


def _np(t):
    return t.cpu().numpy()


def _report(what, case, e0, err, bar):
    print("paths %-5s N=%d S=%d M=%d T=%d D=%d n_out=%d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
          % ((what,) + tuple(case[:6]) + (e0, err, bar, bar / max(err, 1e-300))))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-S%d-M%d-T%d-D%d-o%d" % c[:6])
def test_eval_and_step_against_the_reference(case):
    N, S, M, T, D, n_out, chunk = case
    p = _problem(N, S, M, T, D, n_out)
    gp = _gp(p)
    if chunk:
        gp.set_chunk(chunk)
    assert gp.paths_count() == (0, 0)
    _draw(gp, p)
    assert gp.paths_count() == (S, M)
    F = gp.sample_paths(p["x"])
    assert F.shape == (T, S, n_out)
    ref, e0, scale, bar = _ref(p, pr.evaluate, p["x"])
    err = float(np.abs(F - ref).max())
    _report("eval", case, e0, err, bar)
    # _step on the same model, T = S queries: against the reference, and against the diagonal of _eval
    Fs = _np(gp.paths_step_device(p["xs"]))
    assert Fs.shape == (S, n_out)
    sref, se0, sscale, sbar = _ref(p, pr.step, p["xs"])
    serr = float(np.abs(Fs - sref).max())
    _report("step", case, se0, serr, sbar)
    Fd = gp.sample_paths(p["xs"])[np.arange(S), np.arange(S), :]
    derr = float(np.abs(Fs - Fd).max())
    print("paths diag  |step - eval[s, s]| = %.3e  bar = %.3e" % (derr, 1e-12 * sscale))
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(Fs))
    assert err <= bar
    assert serr <= sbar
    assert derr <= 1e-12 * sscale


def test_zero_draws_are_the_posterior_mean():
    p = _problem(300, 129, 100, 300, 3, 2)
    gp = _gp(p)
    _draw(gp, p, w=0 * p["w"], eps=0 * p["eps"])
    F = gp.sample_paths(p["x"])
    mu = gp.predict(p["x"])[0]
    om = oracle_model(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"])
    for s in range(p["S"]):
        np.testing.assert_allclose(F[:, s, :], mu, rtol=1e-9, atol=mu_atol(om))


def test_bitwise_repeatable_chunks_and_shared_workspace():
    p = _problem(300, 129, 100, 300, 3, 2)
    gp = _gp(p)
    x1000 = np.random.default_rng(5).uniform(-1, 1, (1000, 3))
    mu0, var0 = gp.predict(x1000)
    outs = []
    for _ in range(2):
        _draw(gp, p)
        outs.append((gp.sample_paths(p["x"]), _np(gp.paths_step_device(p["xs"]))))
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    # the shared workspace: predict is what it was, and the paths are still right after a predict of 1000 queries
    mu1, var1 = gp.predict(x1000)
    np.testing.assert_array_equal(mu0, mu1)
    np.testing.assert_array_equal(var0, var1)
    ref, e0, scale, bar = _ref(p, pr.evaluate, p["x"])
    F = gp.sample_paths(p["x"])
    assert np.abs(F - ref).max() <= bar
    np.testing.assert_array_equal(F, outs[0][0])
    # another chunk size: equal to 1e-13 relative
    gp.set_chunk(77)
    F77 = gp.sample_paths(p["x"])
    assert np.abs(F77 - F).max() <= 1e-13 * scale
    gp.release_scratch()                                # frees the workspaces, not the paths
    assert gp.paths_count() == (p["S"], p["M"])
    np.testing.assert_array_equal(gp.sample_paths(p["x"]), F77)


def _eval_rc(gp, x):
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    xt = B.as_dev(x, hd.device)
    F = B.empty((x.shape[0], max(1, gp.paths_count()[0]), hd.n_out), hd.device)
    return lib.sr_gp_paths_eval(hd.h, B.ptr(xt), x.shape[0], B.ptr(F), B.stream_ptr(hd.device))


def _draw_rc(gp, p, S, M, null_w=False):
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    t = [B.as_dev(p[k], hd.device) for k in ("omega", "tau", "w", "eps")]
    return lib.sr_gp_paths_draw(hd.h, S, M, B.ptr(t[0]), B.ptr(t[1]), None if null_w else B.ptr(t[2]), B.ptr(t[3]),
                                B.stream_ptr(hd.device))


def _check_against(gp, p):
    ref, e0, scale, bar = _ref(p, pr.evaluate, p["x"])
    assert np.abs(gp.sample_paths(p["x"]) - ref).max() <= bar


def test_states_and_errors():
    p = _problem(200, 40, 32, 9, 3, 2)
    gp = _gp(p)
    assert _eval_rc(gp, p["x"]) == SR_ESTATE                          # before any draw
    with pytest.raises(RuntimeError):
        gp.sample_paths(p["x"])
    _draw(gp, p)
    F = gp.sample_paths(p["x"])
    # invalid arguments leave the paths drawn earlier intact
    assert _draw_rc(gp, p, p["S"], 0) == SR_EINVAL
    assert _draw_rc(gp, p, p["S"], p["M"], null_w=True) == SR_EINVAL
    assert _draw_rc(gp, p, -1, p["M"]) == SR_EINVAL
    assert gp.paths_count() == (p["S"], p["M"])
    np.testing.assert_array_equal(gp.sample_paths(p["x"]), F)
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    assert lib.sr_gp_paths_eval(hd.h, None, -1, None, B.stream_ptr(hd.device)) == SR_EINVAL
    assert lib.sr_gp_paths_eval(hd.h, None, 0, None, B.stream_ptr(hd.device)) == 0     # T == 0: a no-op
    # the closed loop needs D = n_out + n_u
    xs = B.as_dev(p["xs"], hd.device)
    Ft = B.empty((p["S"], 2), hd.device)
    assert lib.sr_gp_paths_step(hd.h, B.ptr(xs), B.ptr(Ft), B.ptr(Ft), None, None, B.stream_ptr(hd.device)) == SR_EINVAL
    # ... also with all three pointers set: a model with D == n_out (two outputs, one state input, one action) has no n_u
    p2 = _problem(40, 8, 8, 3, 2, 2)
    g2 = _gp(p2)
    _draw(g2, p2)
    h2 = g2._handle
    x2, F2, z2 = B.as_dev(p2["xs"], h2.device), B.empty((8, 2), h2.device), B.empty((8, 2), h2.device)
    kf = B.as_dev(np.zeros(4), h2.device)
    assert lib.sr_gp_paths_step(h2.h, B.ptr(x2), B.ptr(F2), B.ptr(kf), B.ptr(kf), B.ptr(z2), B.stream_ptr(h2.device)) == SR_EINVAL
    assert lib.sr_gp_paths_step(h2.h, B.ptr(x2), B.ptr(F2), None, None, None, B.stream_ptr(h2.device)) == 0
    ref2, _, _, bar2 = _ref(p2, pr.step, p2["xs"])
    assert np.abs(_np(F2) - ref2).max() <= bar2
    with pytest.raises(ValueError):
        g2.paths_step_device(p2["xs"], np.zeros((1, 2)), np.zeros(1))
    # S = 0 drops the paths
    gp.drop_paths()
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE

    # a refit invalidates; a new draw works against a refit reference
    _draw(gp, p)
    q = _problem(200, 40, 32, 9, 3, 2, seed=77)
    gp.update_model(q["Z"], q["Y"], opt_hyp=False, replace_old=True)
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE
    q = dict(q, ls=p["ls"], sf2=p["sf2"])                             # (the model keeps its hyper-parameters)
    q["c"] = {r: pr.coeffs(q["Z"], q["Y"], q["ls"], q["sf2"], q["noise_var"], q["omega"], q["tau"], q["w"], q["eps"], r)
              for r in ("chol", "lu")}
    _draw(gp, q)
    _check_against(gp, q)

    # removal
    gp.remove_data([3, 150])
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE
    keep = np.delete(np.arange(200), [3, 150])
    r = dict(q, Z=q["Z"][keep], Y=q["Y"][keep], eps=q["eps"][:, :, keep], N=198)
    r["c"] = {k: pr.coeffs(r["Z"], r["Y"], r["ls"], r["sf2"], r["noise_var"], r["omega"], r["tau"], r["w"], r["eps"], k)
              for k in ("chol", "lu")}
    _draw(gp, r)
    _check_against(gp, r)


def test_in_place_append_invalidates():
    """a one-point append at N = 600 (the in-place route: the model's buffers become views; an odd slide makes _draw put the
    factor back in plain buffers first)"""
    N = 600
    full = _problem(N + 1, 16, 32, 5, 3, 2)
    p = dict(full, Z=full["Z"][:N], Y=full["Y"][:N], eps=full["eps"][:, :, :N], N=N)
    p["c"] = {k: pr.coeffs(p["Z"], p["Y"], p["ls"], p["sf2"], p["noise_var"], p["omega"], p["tau"], p["w"], p["eps"], k)
              for k in ("chol", "lu")}
    gp = _gp(p)
    gp.append_limit = 10 ** 9
    _draw(gp, p)
    _check_against(gp, p)
    gp.update_model(full["Z"][N:], full["Y"][N:], opt_hyp=False, replace_old=False)
    assert gp._handle.N == N + 1
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE
    _draw(gp, full)
    _check_against(gp, full)


def test_unsupported_models():
    from safe_exploration_amd import SimpleGPModel
    from _helpers import width_problem, width_gp
    rng = np.random.default_rng(0)
    # sparse: Wt is not the factor of K_y
    p = _problem(200, 40, 32, 9, 3, 2)
    hyp = [{"lengthscale": p["ls"][d], "variance": p["sf2"][d], "noise_variance": 1e-2} for d in range(2)]
    Zu = p["Z"][:32].copy()
    sp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, Z=Zu)
    sp.do_sparse_gp = True
    sp.train(p["Z"], p["Y"], 32, opt_hyp=False, Z=Zu)
    q = dict(p, eps=p["eps"][:, :, :32])
    assert _draw_rc(sp, q, p["S"], p["M"]) == SR_ESTATE
    assert sp.paths_count() == (0, 0)
    # general family, and D = 9
    for kt, D in (("mat52", 3), ("rbf", 9)):
        prob = width_problem(11, kt, D, 60, 2)
        g = width_gp(prob)
        d = dict(omega=rng.standard_normal((8, D)), tau=rng.uniform(0, 6, 8), w=rng.standard_normal((2, 4, 8)),
                 eps=rng.standard_normal((2, 4, 60)))
        assert _draw_rc(g, d, 4, 8) == SR_EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            g.draw_paths(4, 8, **d)
        assert g.paths_count() == (0, 0)


def test_with_a_resident_server():
    p = _problem(100, 20, 16, 7, 3, 2)
    gp = _gp(p)
    assert gp.start_server(idle_timeout_s=0.002)
    x1 = p["x"][:1]
    o0 = gp(x1[:, :2], x1[:, 2:])
    _draw(gp, p)
    _check_against(gp, p)
    o1 = gp(x1[:, :2], x1[:, 2:])
    armed, _, _, calls = gp.server_state()
    assert armed and calls == 2
    for u, v in zip(o0, o1):
        np.testing.assert_array_equal(u, v)
    gp.stop_server()


def test_consistent_rollout():
    """n_s = 2, n_u = 1, N = 60, 3 steps, 70 particles, M = 64: sample_n_step(consistent=True) equals a NumPy rollout of the
    reference step by step; consistent=False with supplied eps is bit-identical to the marginal route through sample_device."""
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
    S_last, S_all = mc.sample_n_step(x0, K, k, n=n, n_samples=S, consistent=True, n_features=M)
    assert gp.paths_count() == (S, M) and S_all.shape == (n, S, n_s)
    ra, rb = (pr.rollout(x0[:, 0], K, k, p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][r]) for r in ("chol", "lu"))
    for i in range(n):
        e0, scale = float(np.abs(ra[i] - rb[i]).max()), float(np.abs(ra[i]).max())
        bar = max(20.0 * e0, 1e-12 * scale * np.sqrt(N + M))
        err = float(np.abs(S_all[i] - ra[i]).max())
        print("paths rollout step %d  e0=%.3e  err=%.3e  bar=%.3e" % (i, e0, err, bar))
        assert err <= bar
    np.testing.assert_array_equal(S_last, S_all[n - 1])
    # another particle count: the paths are drawn afresh from the generator
    mc.sample_n_step(x0, K, k, n=n, n_samples=33, consistent=True, n_features=M)
    assert gp.paths_count() == (33, M)
    # the default route is untouched: the same calls of sample_device, the same bits
    eps = rng.standard_normal((n, S, n_s))
    _, A = mc.sample_n_step(x0, K, k, n=n, n_samples=S, eps=eps)
    inp = np.vstack((x0, K[0].dot(x0) + k[0, :, None])).T
    for i in range(n):
        e = eps[i][None] if i == 0 else eps[i][:, None]
        size = S if i == 0 else 1
        if i + 1 < n:
            Sd, z = gp.sample_device(inp, size, e, None, K[i + 1], k[i + 1])
            inp = z.reshape(S, n_s + n_u)
        else:
            Sd = gp.sample_device(inp, size, e, None)
        np.testing.assert_array_equal(A[i], _np(Sd).reshape(S, n_s))
