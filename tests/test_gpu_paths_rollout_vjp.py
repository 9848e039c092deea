"""The reverse pass of the consistent roll-out on the device (sr_gp_paths_rollout_vjp, SimpleGPModel.paths_rollout_vjp_device /
paths_rollout_diff_device, MonteCarloSafetyVerification.rollout_paths_diff) against the NumPy references
tests/_paths_rollout_vjp_ref.py and tests/_paths_grad_ref.py.  X_all is the device forward's own output, the seeds are
X_bar = default_rng(31).standard_normal((H, S, n_s)), every case runs with a shared and with a per-path start.

Tolerances (none measured on the code under test):
 1. every Jacobian J_all[i] against _paths_grad_ref.step_grad at the kernel's own input [x_i, K[i] x_i + k[i]]: the project's
    rule for a step, bar_i = max(20 e0_i, 1e-12 max|J_ref| sqrt(N + M)), e0_i the difference of the reference's Cholesky and
    LU routes;
 2. the device's three gradients against the long-double sweep over the device's OWN J_all, elementwise: the forward-error bound
    of a sum of products n u A, u = 2^-53, n = H (D + 2) + S + 8 (the operations along the longest chain of the recursion and
    of the reduction over the paths), A the same sweep over |J|, |x|, |X_bar|, |K|.  It holds for any summation order;
 3. end to end against the reference (Cholesky route, at the device's X_all), elementwise: the gradients are polynomials in
    the entries of J, so |dJ_i| <= bar_i changes them by at most sweep_abs(|J_ref| + bar_i) - sweep_abs(|J_ref|); added to it
    n u A with A taken on |J_ref| + bar_i (which bounds the device's |J| by test 1).
Every assertion prints error, bar and margin first.

Every test here fails on the parent commit: the symbol and the methods do not exist there."""
import numpy as np
import pytest

import _paths_grad_ref as pg
import _paths_rollout_vjp_ref as rv
import test_gpu_paths_rollout as tr
from test_gpu_paths import _problem, _gp, _draw, _np, SR_EINVAL, SR_ESTATE, SR_EUNSUPPORTED

pytestmark = pytest.mark.gpu

# (N, S, M, D, n_out, H): the forward's seven and one for the reduction over the paths
CASES = tr.CASES + [(60, 257, 16, 3, 2, 2)]              # one path past a 256-path block of the sweep
IDS = ["N%d-S%d-M%d-D%d-o%d-H%d" % c for c in CASES]
U = 2.0 ** -53
_RUNS = {}


def _n_ops(p, H):
    return H * (p["D"] + 2) + p["S"] + 8


def _margin(bar, err):
    return float(np.min(np.where(err > 0.0, bar / np.where(err > 0.0, err, 1.0), np.inf)))


def _device(gp, start, K, k, X_all, X_bar):
    out = gp.paths_rollout_vjp_device(start, K, k, X_all, X_bar, jacobians=True)
    return tuple(_np(t) for t in out)


def _reference(p, start, K, k, X_all):
    """per step: the reference Jacobian (Cholesky route), e0 and the bar of a step; computed once per run"""
    X_prev = rv.states_before(start, X_all)
    Jref, e0s, bars = [], [], []
    for i in range(K.shape[0]):
        inp = rv.inputs(X_prev, K, k, i)
        Ja, Jb = (pg.step_grad(inp, *tr._args(p, r)) for r in ("chol", "lu"))
        e0 = float(np.abs(Ja - Jb).max())
        Jref.append(Ja)
        e0s.append(e0)
        bars.append(max(20.0 * e0, 1e-12 * float(np.abs(Ja).max()) * np.sqrt(p["N"] + p["M"])))
    return X_prev, np.stack(Jref), e0s, bars


def _run(case, per_path):
    """model, gains, the device's forward and reverse results and the reference of one (case, start): shared by the tests"""
    key = (case, per_path)
    if key not in _RUNS:
        p, gp, K, k, x0, x0s = tr._setup(case)
        start = x0s if per_path else x0
        H, S, n_s = case[5], case[1], case[4]
        X_all_t = gp.paths_rollout_device(start, K, k)
        X_bar = np.random.default_rng(31).standard_normal((H, S, n_s))
        r = dict(p=p, gp=gp, K=K, k=k, start=start, X_all_t=X_all_t, X_all=_np(X_all_t), X_bar=X_bar)
        r["x0_bar"], r["K_bar"], r["k_bar"], r["J_all"] = _device(gp, start, K, k, X_all_t, X_bar)
        r["X_prev"], r["J_ref"], r["e0"], r["bar"] = _reference(p, start, K, k, r["X_all"])
        _RUNS[key] = r
    return _RUNS[key]


def _check_jacobians(p, J_all, J_ref, e0s, bars, tag=""):
    H, S, n_s, D = J_ref.shape
    assert J_all.shape == (H, S, n_s, D) and np.all(np.isfinite(J_all))
    for i in range(H):
        err = float(np.abs(J_all[i] - J_ref[i]).max())
        print("paths rollout vjp%s J N=%d S=%d M=%d D=%d n_out=%d step %d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
              % (tag, p["N"], S, p["M"], D, n_s, i, e0s[i], err, bars[i], tr._margin(bars[i], err)))
        assert err <= bars[i]


def _compare(what, r, per_path, ref, bar):
    """ref, bar: (x0_bar per path, K_bar, k_bar) triples; a shared start's x0_bar is their sum over the paths"""
    for name, dev, a, b in zip(("x0_bar", "K_bar", "k_bar"), (r["x0_bar"], r["K_bar"], r["k_bar"]), ref, bar):
        if name == "x0_bar" and not per_path:
            a, b = a.sum(axis=0), b.sum(axis=0)
        assert dev.shape == a.shape and np.all(np.isfinite(dev))
        err = np.abs(dev.astype(np.longdouble) - a)
        print("paths rollout vjp %s %-6s max err=%.3e  max bar=%.3e  min margin=%.1f"
              % (what, name, float(err.max()), float(b.max()), _margin(b, err)))
        assert np.all(err <= b)


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_jacobian_at_the_kernels_own_inputs(case, per_path):
    r = _run(case, per_path)
    _check_jacobians(r["p"], r["J_all"], r["J_ref"], r["e0"], r["bar"])


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sweep_on_the_kernels_own_jacobians(case, per_path):
    r = _run(case, per_path)
    n = _n_ops(r["p"], case[5])
    ref = rv.sweep(r["J_all"], r["X_prev"], r["X_bar"], r["K"], np.longdouble)
    A = rv.sweep_abs(r["J_all"], r["X_prev"], r["X_bar"], r["K"])
    _compare("sweep %s n=%d" % (IDS[CASES.index(case)], n), r, per_path, ref, tuple(n * U * a for a in A))


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_end_to_end_against_the_reference(case, per_path):
    r = _run(case, per_path)
    n = _n_ops(r["p"], case[5])
    ref = rv.sweep(r["J_ref"], r["X_prev"], r["X_bar"], r["K"])                  # = _paths_rollout_vjp_ref.vjp at X_all
    chk = rv.vjp(r["start"], r["K"], r["k"], r["X_all"], r["X_bar"], *tr._args(r["p"], "chol"))
    for a, b in zip(ref, chk[:3]):
        np.testing.assert_array_equal(a, b)
    dJ = np.stack([np.full(r["J_ref"][i].shape, r["bar"][i]) for i in range(case[5])])
    A0 = rv.sweep_abs(r["J_ref"], r["X_prev"], r["X_bar"], r["K"])
    A1 = rv.sweep_abs(np.abs(r["J_ref"]).astype(np.longdouble) + dJ, r["X_prev"], r["X_bar"], r["K"])
    bar = tuple((a1 - a0) + n * U * a1 for a0, a1 in zip(A0, A1))
    _compare("e2e   %s n=%d" % (IDS[CASES.index(case)], n), r, per_path, ref, bar)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_properties(case):
    rs, rp = _run(case, False), _run(case, True)
    S, n_s, H = case[1], case[4], case[5]
    for r in (rs, rp):
        gp, a = r["gp"], (r["start"], r["K"], r["k"], r["X_all_t"], r["X_bar"])
        again = _device(gp, *a)                                                   # the same bits on two calls
        for u, v in zip(again, (r["x0_bar"], r["K_bar"], r["k_bar"], r["J_all"])):
            np.testing.assert_array_equal(u, v)
        plain = gp.paths_rollout_vjp_device(*a)                                   # ... and without J_all
        assert len(plain) == 3
        for u, v in zip(plain, again[:3]):
            np.testing.assert_array_equal(_np(u), v)
        zero = gp.paths_rollout_vjp_device(*a[:4], np.zeros((H, S, n_s)))         # X_bar = 0: exact zeros
        for u, v in zip(zero, again[:3]):
            assert tuple(u.shape) == v.shape and not np.any(_np(u))
    # a shared start's x0_bar is the ordered sum over the paths of what a per-path call at the tiled start gives
    gp, x0 = rs["gp"], rs["start"]
    tiled = np.tile(x0[None, :], (S, 1))
    per = _device(gp, tiled, rs["K"], rs["k"], rs["X_all_t"], rs["X_bar"])
    assert rs["x0_bar"].shape == (n_s,) and per[0].shape == (S, n_s)
    for u, v in zip(per[1:], (rs["K_bar"], rs["k_bar"], rs["J_all"])):
        np.testing.assert_array_equal(u, v)
    A = rv.sweep_abs(rs["J_all"], rs["X_prev"], rs["X_bar"], rs["K"])[0].sum(axis=0)
    bar = _n_ops(rs["p"], H) * U * A
    err = np.abs(rs["x0_bar"].astype(np.longdouble) - per[0].astype(np.longdouble).sum(axis=0))
    print("paths rollout vjp shared x0_bar against the per-path sum %s  max err=%.3e  max bar=%.3e  min margin=%.1f"
          % (IDS[CASES.index(case)], float(err.max()), float(bar.max()), _margin(bar, err)))
    assert np.all(err <= bar)
    # (n_s, 1), the start as sample_n_step takes it: the same call, the gradient in that shape
    col = gp.paths_rollout_vjp_device(x0[:, None], rs["K"], rs["k"], rs["X_all_t"], rs["X_bar"])
    assert tuple(col[0].shape) == (n_s, 1)
    np.testing.assert_array_equal(_np(col[0])[:, 0], rs["x0_bar"])


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
def test_autograd(per_path):
    import torch
    case = CASES[2]
    r = _run(case, per_path)
    gp, dev = r["gp"], r["gp"].device
    t = lambda a, g: torch.as_tensor(a, device=dev).requires_grad_(g)
    x0, K, k = t(r["start"], True), t(r["K"], True), t(r["k"], True)
    X_bar = torch.as_tensor(r["X_bar"], device=dev)
    X_all = gp.paths_rollout_diff_device(x0, K, k)
    assert X_all.requires_grad
    np.testing.assert_array_equal(_np(X_all.detach()), r["X_all"])               # the bits of paths_rollout_device
    (X_bar * X_all).sum().backward()
    for g, ref in ((x0.grad, r["x0_bar"]), (K.grad, r["K_bar"]), (k.grad, r["k_bar"])):
        np.testing.assert_array_equal(_np(g), ref)                              # the bits of paths_rollout_vjp_device
    # a tensor that does not require a gradient gets none
    x0, K, k = t(r["start"], False), t(r["K"], True), t(r["k"], False)
    (X_bar * gp.paths_rollout_diff_device(x0, K, k)).sum().backward()
    assert x0.grad is None and k.grad is None
    np.testing.assert_array_equal(_np(K.grad), r["K_bar"])
    assert not gp.paths_rollout_diff_device(r["start"], r["K"], r["k"]).requires_grad
    # once differentiable
    x0 = t(r["start"], True)
    g, = torch.autograd.grad((X_bar * gp.paths_rollout_diff_device(x0, r["K"], r["k"])).sum(), x0, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_rollout_paths_diff():
    import torch
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    case = CASES[1]
    N, S, M, D, n_s, H = case
    r = _run(case, False)
    gp, dev = r["gp"], r["gp"].device
    mc = MonteCarloSafetyVerification(gp)
    K = torch.as_tensor(r["K"], device=dev).requires_grad_(True)
    k = torch.as_tensor(r["k"], device=dev).requires_grad_(True)
    S_last, S_all = mc.rollout_paths_diff(r["start"][:, None], K, k, n=H, n_samples=S, n_features=M)
    assert gp.paths_count() == (S, M)                                            # the model's valid paths were used
    assert tuple(S_all.shape) == (H, S, n_s) and tuple(S_last.shape) == (S, n_s)
    assert S_last._base is not None and S_last.data_ptr() == S_all[H - 1].data_ptr() and S_last.requires_grad
    np.testing.assert_array_equal(_np(S_all.detach()), mc.rollout_paths(r["start"][:, None], r["K"], r["k"], n=H, n_samples=S,
                                                                         n_features=M)[1])
    # a cost of the last state alone: the seeds of the earlier steps are zero
    w = torch.as_tensor(r["X_bar"][H - 1], device=dev)
    (w * S_last).sum().backward()
    X_bar = np.zeros((H, S, n_s))
    X_bar[H - 1] = r["X_bar"][H - 1]
    ref = gp.paths_rollout_vjp_device(r["start"], r["K"], r["k"], r["X_all_t"], X_bar)
    np.testing.assert_array_equal(_np(K.grad), _np(ref[1]))
    np.testing.assert_array_equal(_np(k.grad), _np(ref[2]))
    # another particle count: the paths are drawn afresh from the generator
    g = torch.Generator(device=dev).manual_seed(4)
    out = mc.rollout_paths_diff(r["start"], K, k, n=H, n_samples=33, generator=g, n_features=48)
    assert gp.paths_count() == (33, 48) and tuple(out[1].shape) == (H, 33, n_s) and bool(torch.isfinite(out[1]).all())
    _RUNS.pop((case, False))                                                     # (its model holds other paths now)


NAMES = ("x0", "k_fb", "k_ff", "X_all", "X_bar", "x0_bar", "k_fb_bar", "k_ff_bar")


def _rc(gp, H=2, null=None, handle=True, per_path=0):
    """the raw status of a call without J_all on zero inputs; `null` names the pointer passed as NULL"""
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    n_s, n_u, Hb = hd.n_out, max(1, hd.D - hd.n_out), max(1, H)
    S = max(1, gp.paths_count()[0])
    z = lambda *shape: B.as_dev(np.zeros(shape), hd.device)
    bufs = dict(x0=z(S, n_s), k_fb=z(Hb, n_u, n_s), k_ff=z(Hb, n_u), X_all=z(Hb, S, n_s), X_bar=z(Hb, S, n_s), x0_bar=z(S, n_s),
                k_fb_bar=z(Hb, n_u, n_s), k_ff_bar=z(Hb, n_u))
    a = {n: (None if n == null else B.ptr(t)) for n, t in bufs.items()}
    return lib.sr_gp_paths_rollout_vjp(hd.h if handle else None, a["x0"], per_path, H, a["k_fb"], a["k_ff"], a["X_all"],
                                       a["X_bar"], a["x0_bar"], a["k_fb_bar"], a["k_ff_bar"], None, B.stream_ptr(hd.device))


def _check_valid(gp, p, H=2):
    """a valid call passes test 1 (per-path start, the device forward's own states)"""
    rng = np.random.default_rng(21)
    n_s, n_u = p["n_out"], p["D"] - p["n_out"]
    K, k = 0.3 * rng.standard_normal((H, n_u, n_s)), 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, (p["S"], n_s))
    X_all = gp.paths_rollout_device(x0, K, k)
    out = _device(gp, x0, K, k, X_all, rng.standard_normal((H, p["S"], n_s)))
    _, J_ref, e0s, bars = _reference(p, x0, K, k, _np(X_all))
    _check_jacobians(p, out[3], J_ref, e0s, bars, tag=" state")


def test_states_and_errors():
    p = _problem(200, 40, 32, 9, 3, 2)
    gp = _gp(p)
    K, k, X = np.zeros((2, 1, 2)), np.zeros((2, 1)), np.zeros((2, 40, 2))
    assert _rc(gp) == SR_ESTATE                                        # before any draw
    with pytest.raises(RuntimeError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, k, X, X)
    with pytest.raises(RuntimeError):
        gp.paths_rollout_diff_device(np.zeros(2), K, k)
    _draw(gp, p)
    _check_valid(gp, p)
    # invalid arguments: refused, the paths are what they were and a valid call works
    refused = [dict(H=0), dict(H=-3), dict(handle=False), dict(per_path=2), dict(per_path=-1)] + [dict(null=n) for n in NAMES]
    for kw in refused:
        assert _rc(gp, **kw) == SR_EINVAL, kw
        assert gp.paths_count() == (p["S"], p["M"])
        _check_valid(gp, p)
    assert _rc(gp) == 0 and _rc(gp, per_path=1) == 0
    for bad in (np.zeros(3), np.zeros((p["S"] + 1, 2))):               # the shapes the Python surface refuses
        with pytest.raises(ValueError):
            gp.paths_rollout_vjp_device(bad, K, k, X, X)
    with pytest.raises(ValueError):
        gp.paths_rollout_vjp_device(np.zeros(2), np.zeros((2, 2, 2)), k, X, X)
    with pytest.raises(ValueError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, np.zeros((3, 1)), X, X)
    with pytest.raises(ValueError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, k, X[:1], X)
    with pytest.raises(ValueError):
        gp.paths_rollout_vjp_device(np.zeros(2), K, k, X, np.zeros((2, 41, 2)))
    # D == n_out (two outputs, one state input, one action): no closed loop
    p2 = _problem(40, 8, 8, 3, 2, 2)
    g2 = _gp(p2)
    _draw(g2, p2)
    assert _rc(g2) == SR_EINVAL and g2.paths_count() == (8, 8)
    with pytest.raises(ValueError):
        g2.paths_rollout_vjp_device(np.zeros(2), np.zeros((2, 1, 2)), np.zeros((2, 1)), np.zeros((2, 8, 2)), np.zeros((2, 8, 2)))
    _check_valid(gp, p)
    # S = 0 drops the paths
    gp.drop_paths()
    assert _rc(gp) == SR_ESTATE
    _draw(gp, p)
    _check_valid(gp, p)
    # a refit invalidates; a new draw works against a refit reference
    q = _problem(200, 40, 32, 9, 3, 2, seed=77)
    gp.update_model(q["Z"], q["Y"], opt_hyp=False, replace_old=True)
    assert gp.paths_count() == (0, 0) and _rc(gp) == SR_ESTATE
    q = dict(q, ls=p["ls"], sf2=p["sf2"])                              # (the model keeps its hyper-parameters)
    q["c"] = tr._coeffs(q)
    _draw(gp, q)
    _check_valid(gp, q)
    # an append of one row
    rng = np.random.default_rng(5)
    zn, yn = rng.uniform(-1, 1, (1, 3)), rng.standard_normal((1, 2))
    gp.update_model(zn, yn, opt_hyp=False, replace_old=False)
    assert gp._handle.N == 201
    assert gp.paths_count() == (0, 0) and _rc(gp) == SR_ESTATE
    a = dict(q, Z=np.vstack((q["Z"], zn)), Y=np.vstack((q["Y"], yn)), eps=rng.standard_normal((2, 40, 201)), N=201)
    a["c"] = tr._coeffs(a)
    _draw(gp, a)
    _check_valid(gp, a)
    # a removal
    gp.remove_data([3, 150])
    assert gp.paths_count() == (0, 0) and _rc(gp) == SR_ESTATE
    keep = np.delete(np.arange(201), [3, 150])
    r = dict(a, Z=a["Z"][keep], Y=a["Y"][keep], eps=a["eps"][:, :, keep], N=199)
    r["c"] = tr._coeffs(r)
    _draw(gp, r)
    _check_valid(gp, r)


def test_unsupported_models():
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd._lib import check
    from _helpers import width_problem, width_gp
    # sparse: Wt is not the factor of K_y
    p = _problem(200, 40, 32, 9, 3, 2)
    hyp = [{"lengthscale": p["ls"][d], "variance": p["sf2"][d], "noise_variance": 1e-2} for d in range(2)]
    Zu = p["Z"][:32].copy()
    sp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, Z=Zu)
    sp.do_sparse_gp = True
    sp.train(p["Z"], p["Y"], 32, opt_hyp=False, Z=Zu)
    assert _rc(sp) == SR_ESTATE
    # general family, and D = 9
    for kt, D in (("mat52", 3), ("rbf", 9)):
        g = width_gp(width_problem(11, kt, D, 60, 2))
        rc = _rc(g)
        assert rc == SR_EUNSUPPORTED
        with pytest.raises(NotImplementedError):
            check(rc)
    # a valid call on a supported model afterwards
    gp = _gp(p)
    _draw(gp, p)
    _check_valid(gp, p)


def test_the_neighbours_are_undisturbed():
    """sample_n_step(consistent=True), sample_n_step_jacobians and paths_rollout_device(jacobians=True) share the workspace of
    the path calls with the reverse pass: the same bits before and after it"""
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    case = CASES[1]
    N, S, M, D, n_s, H = case
    p, gp, K, k, x0, x0s = tr._setup(case)
    mc = MonteCarloSafetyVerification(gp)
    x0c = x0[:, None]

    def neighbours():
        a = mc.sample_n_step(x0c, K, k, n=H, n_samples=S, consistent=True, n_features=M)
        b = mc.sample_n_step_jacobians(x0c, K, k, n=H, n_samples=S, n_features=M)
        c = tuple(_np(t) for t in gp.paths_rollout_device(x0s, K, k, jacobians=True))
        return a + b + c

    before = neighbours()
    X_bar = np.random.default_rng(31).standard_normal((H, S, n_s))
    X_all = gp.paths_rollout_device(x0s, K, k)
    with_j = _device(gp, x0s, K, k, X_all, X_bar)
    without = gp.paths_rollout_vjp_device(x0, K, k, gp.paths_rollout_device(x0, K, k), X_bar)
    assert gp.paths_count() == (S, M) and np.all(np.isfinite(with_j[1])) and bool(without[1].isfinite().all())
    for u, v in zip(before, neighbours()):
        np.testing.assert_array_equal(u, v)
    for u, v in zip(with_j, _device(gp, x0s, K, k, X_all, X_bar)):               # ... and the reverse pass after them
        np.testing.assert_array_equal(u, v)
