"""The closed-loop roll-out of the posterior function samples in one launch (sr_gp_paths_rollout, SimpleGPModel.
paths_rollout_device, MonteCarloSafetyVerification.rollout_paths) against the NumPy references tests/_paths_ref.py and
tests/_paths_grad_ref.py, STEP BY STEP AT THE KERNEL'S OWN INPUTS: for step i the reference is evaluated at
[x_i, K[i] x_i + k[i]] with x_i the state the kernel itself produced (x0, or X_all[i - 1]), so the closed loop's amplification
of earlier rounding stays out of the comparison and the bar of one step applies to every step.

Tolerance (the rule of test_gpu_paths for a step, nothing invented): e0 = the largest difference between the reference's two
solve routes (Cholesky, LU) at that input, scale = max |ref|, bar = max(20 e0, 1e-12 scale sqrt(N + M)); for A_all the same
rule on A = J_x + J_u K[i] formed from the reference Jacobian (as test_gpu_paths_grad.test_consistent_rollout_jacobians).
Every step prints e0, the device's error, the bar and the margin.

Every test here fails on the parent commit: the symbol and the methods do not exist there."""
import numpy as np
import pytest

import _paths_ref as pr
import _paths_grad_ref as pg
import test_gpu_paths as tg
from test_gpu_paths import _problem, _gp, _draw, _np, SR_EINVAL, SR_ESTATE, SR_EUNSUPPORTED

pytestmark = pytest.mark.gpu

# (N, S, M, D, n_out, H)
CASES = [
    (1, 1, 1, 2, 1, 2),                      # minimal everything
    (60, 70, 64, 3, 2, 3),                   # the shape of test_consistent_rollout; S not a multiple of 64
    (257, 129, 100, 5, 4, 4),                # one row past four Z tiles; S past one 128 tile; cart-pole widths
    (300, 65, 300, 8, 2, 2),                 # widest bucket, n_u = 6, M past one omega tile
    (200, 40, 32, 4, 3, 5),                  # D below its bucket
    (60, 70, 64, 3, 2, 1),                   # H = 1
    (65, 5, 513, 3, 2, 2),                   # one row past a Z tile, one feature past the 512-row omega tile of D <= 5; a
]                                            # second workgroup with one live path
IDS = ["N%d-S%d-M%d-D%d-o%d-H%d" % c for c in CASES]


def _setup(case, draw=True):
    N, S, M, D, n_out, H = case
    p = _problem(N, S, M, 1, D, n_out)
    gp = _gp(p, n_u=D - n_out)
    if draw:
        _draw(gp, p)
    rng = np.random.default_rng(9 + H)
    n_u = D - n_out
    K = 0.3 * rng.standard_normal((H, n_u, n_out))
    k = 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, n_out)
    x0s = rng.uniform(-0.5, 0.5, (S, n_out))
    return p, gp, K, k, x0, x0s


def _args(p, r):
    return p["Z"], p["ls"], p["sf2"], p["omega"], p["tau"], p["w"], p["c"][r]


def _margin(bar, err):
    return bar / err if err > 0.0 else float("inf")


def _stepwise(p, x0, K, k, X_all, A_all=None, tag=""):
    """every step against the reference at the kernel's own input; asserts after printing the step's figures"""
    S, n_s, NM = p["S"], p["n_out"], p["N"] + p["M"]
    H = K.shape[0]
    assert X_all.shape == (H, S, n_s) and np.all(np.isfinite(X_all))
    x = np.tile(np.asarray(x0).reshape(1, n_s), (S, 1)) if np.ndim(x0) == 1 else np.asarray(x0)
    for i in range(H):
        inp = np.hstack((x, x.dot(K[i].T) + k[i][None, :]))
        ref, e0, scale, bar = tg._ref(p, pr.step, inp)
        err = float(np.abs(X_all[i] - ref).max())
        print("paths rollout%s N=%d S=%d M=%d D=%d n_out=%d step %d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
              % (tag, p["N"], S, p["M"], p["D"], n_s, i, e0, err, bar, _margin(bar, err)))
        assert err <= bar
        if A_all is not None:
            Aa, Ab = (J[:, :, :n_s] + J[:, :, n_s:].dot(K[i]) for J in (pg.step_grad(inp, *_args(p, r)) for r in ("chol", "lu")))
            ae0, ascale = float(np.abs(Aa - Ab).max()), float(np.abs(Aa).max())
            abar = max(20.0 * ae0, 1e-12 * ascale * np.sqrt(NM))
            aerr = float(np.abs(A_all[i] - Aa).max())
            print("paths rollout%s A step %d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
                  % (tag, i, ae0, aerr, abar, _margin(abar, aerr)))
            assert A_all[i].shape == (S, n_s, n_s) and aerr <= abar
        x = X_all[i]


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_step_against_the_reference_at_the_kernels_own_inputs(case, per_path):
    p, gp, K, k, x0, x0s = _setup(case)
    start = x0s if per_path else x0
    X_all = _np(gp.paths_rollout_device(start, K, k))
    _stepwise(p, start, K, k, X_all)
    if not per_path:                                     # (n_s, 1), the start as sample_n_step takes it: the same call
        np.testing.assert_array_equal(_np(gp.paths_rollout_device(x0[:, None], K, k)), X_all)


@pytest.mark.parametrize("per_path", [False, True], ids=["shared-x0", "per-path-x0"])
@pytest.mark.parametrize("case", CASES[1:4] + CASES[6:], ids=IDS[1:4] + IDS[6:])
def test_jacobians(case, per_path):
    p, gp, K, k, x0, x0s = _setup(case)
    start = x0s if per_path else x0
    X_all, A_all = (_np(t) for t in gp.paths_rollout_device(start, K, k, jacobians=True))
    _stepwise(p, start, K, k, X_all, A_all, tag=" grad")
    np.testing.assert_array_equal(X_all, _np(gp.paths_rollout_device(start, K, k)))


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_same_bits_on_every_call_and_for_every_horizon(case):
    p, gp, K, k, x0, x0s = _setup(case)
    H = case[5]
    for start in (x0, x0s):
        X, A = (_np(t) for t in gp.paths_rollout_device(start, K, k, jacobians=True))
        X2, A2 = (_np(t) for t in gp.paths_rollout_device(start, K, k, jacobians=True))
        np.testing.assert_array_equal(X, X2)
        np.testing.assert_array_equal(A, A2)
        for h in (1, H - 1):
            Xh, Ah = (_np(t) for t in gp.paths_rollout_device(start, K[:h], k[:h], jacobians=True))
            np.testing.assert_array_equal(Xh, X[:h])
            np.testing.assert_array_equal(Ah, A[:h])
            np.testing.assert_array_equal(_np(gp.paths_rollout_device(start, K[:h], k[:h])), X[:h])


def test_rollout_paths():
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    import torch
    case = CASES[1]
    N, S, M, D, n_s, H = case
    p, gp, K, k, x0, x0s = _setup(case)
    mc = MonteCarloSafetyVerification(gp)
    x0c = x0[:, None]
    before = mc.sample_n_step(x0c, K, k, n=H, n_samples=S, consistent=True, n_features=M)
    before_j = mc.sample_n_step_jacobians(x0c, K, k, n=H, n_samples=S, n_features=M)
    # NumPy out by default, on the supplied draws: the step-wise test, shared and per-particle starts
    S_last, S_all = mc.rollout_paths(x0c, K, k, n=H, n_samples=S, n_features=M)
    assert gp.paths_count() == (S, M)
    assert isinstance(S_all, np.ndarray) and S_all.shape == (H, S, n_s) and S_last.shape == (S, n_s)
    np.testing.assert_array_equal(S_last, S_all[H - 1])
    _stepwise(p, x0, K, k, S_all, tag=" mc")
    out = mc.rollout_paths(x0s, K, k, n=H, n_samples=S, n_features=M, jacobians=True)
    assert len(out) == 3 and out[2].shape == (H, S, n_s, n_s)
    np.testing.assert_array_equal(out[0], out[1][H - 1])
    _stepwise(p, x0s, K, k, out[1], out[2], tag=" mc")
    # tensors on request
    t = mc.rollout_paths(x0c, K, k, n=H, n_samples=S, n_features=M, as_tensor=True, jacobians=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t)
    assert tuple(t[0].shape) == (S, n_s) and tuple(t[1].shape) == (H, S, n_s) and tuple(t[2].shape) == (H, S, n_s, n_s)
    np.testing.assert_array_equal(_np(t[1]), S_all)
    # close to the chained route (not bit for bit: the terms are summed in another order; 1e-9 leaves three steps of the
    # closed loop room to amplify rounding of 1e-16 sqrt(N + M) scale)
    assert np.abs(S_all - before[1]).max() <= 1e-9 * np.abs(before[1]).max()
    # the fused call disturbs neither the paths nor the shared workspace: the chained route returns what it did
    after = mc.sample_n_step(x0c, K, k, n=H, n_samples=S, consistent=True, n_features=M)
    after_j = mc.sample_n_step_jacobians(x0c, K, k, n=H, n_samples=S, n_features=M)
    for u, v in zip(before + before_j, after + after_j):
        np.testing.assert_array_equal(u, v)
    # another particle count: the paths are drawn afresh from the generator
    g = torch.Generator(device=gp.device).manual_seed(4)
    r = mc.rollout_paths(x0c, K, k, n=H, n_samples=33, generator=g, n_features=48)
    assert gp.paths_count() == (33, 48) and r[1].shape == (H, 33, n_s) and np.all(np.isfinite(r[1]))


def _rc(gp, H=2, null=None, handle=True):
    """the raw status of a shared-start call without Jacobians; `null` names the pointer passed as NULL"""
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    n_s, n_u, Hb = hd.n_out, max(1, hd.D - hd.n_out), max(1, H)
    S = max(1, gp.paths_count()[0])
    bufs = dict(x0=B.as_dev(np.zeros(n_s), hd.device), k_fb=B.as_dev(np.zeros((Hb, n_u, n_s)), hd.device),
                k_ff=B.as_dev(np.zeros((Hb, n_u)), hd.device), X_all=B.empty((Hb, S, n_s), hd.device))
    a = {n: (None if n == null else B.ptr(t)) for n, t in bufs.items()}
    return lib.sr_gp_paths_rollout(hd.h if handle else None, a["x0"], 0, H, a["k_fb"], a["k_ff"], a["X_all"], None,
                                   B.stream_ptr(hd.device))


def _check_valid(gp, p, H=2):
    rng = np.random.default_rng(21)
    n_s, n_u = p["n_out"], p["D"] - p["n_out"]
    K, k = 0.3 * rng.standard_normal((H, n_u, n_s)), 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, (p["S"], n_s))
    X_all, A_all = (_np(t) for t in gp.paths_rollout_device(x0, K, k, jacobians=True))
    _stepwise(p, x0, K, k, X_all, A_all, tag=" state")


def _coeffs(q):
    return {r: pr.coeffs(q["Z"], q["Y"], q["ls"], q["sf2"], q["noise_var"], q["omega"], q["tau"], q["w"], q["eps"], r)
            for r in ("chol", "lu")}


def test_states_and_errors():
    p = _problem(200, 40, 32, 9, 3, 2)
    gp = _gp(p)
    K, k = np.zeros((2, 1, 2)), np.zeros((2, 1))
    assert _rc(gp) == SR_ESTATE                                        # before any draw
    with pytest.raises(RuntimeError):
        gp.paths_rollout_device(np.zeros(2), K, k)
    _draw(gp, p)
    _check_valid(gp, p)
    # invalid arguments: refused, and the paths are what they were
    assert _rc(gp, H=0) == SR_EINVAL
    assert _rc(gp, H=-3) == SR_EINVAL
    assert _rc(gp, handle=False) == SR_EINVAL
    for name in ("x0", "k_fb", "k_ff", "X_all"):
        assert _rc(gp, null=name) == SR_EINVAL, name
    assert gp.paths_count() == (p["S"], p["M"]) and _rc(gp) == 0
    _check_valid(gp, p)
    for bad in (np.zeros(3), np.zeros((p["S"] + 1, 2))):               # the shapes the Python surface refuses
        with pytest.raises(ValueError):
            gp.paths_rollout_device(bad, K, k)
    with pytest.raises(ValueError):
        gp.paths_rollout_device(np.zeros(2), np.zeros((2, 2, 2)), k)
    with pytest.raises(ValueError):
        gp.paths_rollout_device(np.zeros(2), K, np.zeros((3, 1)))
    # D == n_out (two outputs, one state input, one action): no closed loop
    p2 = _problem(40, 8, 8, 3, 2, 2)
    g2 = _gp(p2)
    _draw(g2, p2)
    assert _rc(g2) == SR_EINVAL
    with pytest.raises(ValueError):
        g2.paths_rollout_device(np.zeros(2), np.zeros((2, 1, 2)), np.zeros((2, 1)))
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
    q["c"] = _coeffs(q)
    _draw(gp, q)
    _check_valid(gp, q)
    # an append of one row
    rng = np.random.default_rng(5)
    zn, yn = rng.uniform(-1, 1, (1, 3)), rng.standard_normal((1, 2))
    gp.update_model(zn, yn, opt_hyp=False, replace_old=False)
    assert gp._handle.N == 201
    assert gp.paths_count() == (0, 0) and _rc(gp) == SR_ESTATE
    a = dict(q, Z=np.vstack((q["Z"], zn)), Y=np.vstack((q["Y"], yn)), eps=rng.standard_normal((2, 40, 201)), N=201)
    a["c"] = _coeffs(a)
    _draw(gp, a)
    _check_valid(gp, a)
    # a removal
    gp.remove_data([3, 150])
    assert gp.paths_count() == (0, 0) and _rc(gp) == SR_ESTATE
    keep = np.delete(np.arange(201), [3, 150])
    r = dict(a, Z=a["Z"][keep], Y=a["Y"][keep], eps=a["eps"][:, :, keep], N=199)
    r["c"] = _coeffs(r)
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
