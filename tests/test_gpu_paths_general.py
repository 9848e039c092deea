"""Posterior function samples of general-family models with the RBF radial part on the device (sr_gp_paths_draw / _eval /
_step and their Jacobians on a handle of sr_gp_set_data_general, csrc/sr_paths_gen.hip; SimpleGPModel.draw_paths /
sample_paths / paths_step_device, sample_n_step(consistent=True), sample_n_step_jacobians on "lin_rbf" models) against the
NumPy reference tests/_paths_gen_ref.py -- every element of F and J.

Models hold arbitrary packed parameters kp (the model class with its parameter packing replaced, as
test_gpu_moment_match_gen._gp builds them): variant "g1" has the structure of the in-tree "lin_rbf" (one group), variant "g0"
no group at all (c0 = 0, a = 0: a purely linear kernel, n_w = D), variant "gn" a full packing -- c0 > 0 on some outputs, several a_j and b_j, an s_j = 0, active sets that differ between the outputs, so
that a group has zero amplitude on one of them (G >= 2).

Tolerance: the rule of test_gpu_paths.py / test_gpu_paths_grad.py with the family's weight count, nothing new: e0 = the
largest difference between the reference's two solve routes (Cholesky, LU), scale = max |ref|,
bar = max(20 e0, 1e-12 scale sqrt(N + n_w)); the step against the diagonal of the evaluation: 1e-12 scale.  Every case
prints e0, the error, the bar and the margin (profiles/r21_paths_general_tests.txt).

Every test here fails on the parent commit: the draw raises NotImplementedError there."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as orc
import _paths_ref as pr
import _paths_gen_ref as gr

pytestmark = pytest.mark.gpu

SR_EINVAL, SR_ESTATE, SR_EUNSUPPORTED = -1, -4, -5
NDIAG = 1e-2                                   # the diagonal term of every model here

# (N, S, M, T, D, n_out, chunk): the cases of test_gpu_paths, every width below and at 3 / 5 / 8, and n_w = G M + D at a
# multiple of 16 and one past it (variant g1: G = 1, M = 13 and 14 at D = 3)
CASES = [
    (1, 1, 1, 1, 1, 1, None),
    (127, 63, 15, 127, 3, 2, None),
    (128, 64, 16, 128, 3, 2, None),
    (129, 65, 17, 129, 5, 4, None),
    (300, 129, 100, 300, 3, 2, 128),
    (300, 200, 256, 1, 8, 1, None),
    (700, 128, 64, 130, 3, 2, None),
    (64, 16, 16, 16, 2, 1, None), (64, 16, 16, 16, 4, 2, None), (64, 16, 16, 16, 6, 2, None), (64, 16, 16, 16, 7, 1, None),
    (64, 16, 13, 16, 3, 2, None), (64, 16, 14, 16, 3, 2, None),
]
VARIANTS = ("g1", "gn")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def make_kp(D, n_out, variant, rng):
    """packed parameters [0, v, c0, s, a, b] per output (see the module docstring); lengthscales scaled by sqrt(D / 3)"""
    kp = np.zeros((n_out, 3 + 3 * D))
    wide = np.sqrt(D / 3.0)
    for o in range(n_out):
        kp[o, 1] = rng.uniform(0.8, 1.2)
        s, a, b = np.zeros(D), np.zeros(D), rng.uniform(0.05, 0.3, D)
        if variant == "g0":                    # c0 = 0 and every a_j = 0: a purely linear kernel, no group at all
            s[:], b = 1.0 / rng.uniform(0.5, 1.0, D), rng.uniform(0.3, 1.0, D)
        elif variant == "g1":
            l0 = min(1, D - 1)                 # the stationary and the product-linear factor on input dimension 1
            s[l0], a[l0] = 1.0 / rng.uniform(0.5, 1.0), rng.uniform(0.5, 1.0)
        else:
            kp[o, 2] = rng.uniform(0.3, 1.0) if o % 2 == 0 else 0.0
            s[:] = 1.0 / (rng.uniform(0.5, 1.0, D) * wide)
            if D >= 3 and o % 2 == 0:
                s[D - 1] = 0.0
            for j in range(D):
                if (j + o) % 2 == 0 or D == 1:
                    a[j] = rng.uniform(0.3, 1.0)
            b[rng.integers(D)] = 0.0
        kp[o, 3:3 + D], kp[o, 3 + D:3 + 2 * D], kp[o, 3 + 2 * D:] = s, a, b
    return kp


_CACHE = {}


def _both(p, **over):
    q = dict(p, **over)
    return {r: gr.coeffs(q["Z"], q["Y"], q["kp"], q["nd"], q["omega"], q["tau"], q["w"], q["eps"], r) for r in ("chol", "lu")}


def _problem(N, S, M, T, D, n_out, variant="g1", seed=None, kp=None):
    """Z ~ U[-1,1]^D, all draws from default_rng(seed); the reference's coefficients by both solve routes (cached; kp: these
    parameters instead of make_kp's)"""
    key = (N, S, M, T, D, n_out, variant, seed, None if kp is None else kp.tobytes())
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng((1000 * N + S if seed is None else seed) + {"g1": 0, "gn": 7, "g0": 13}[variant])
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    kp = make_kp(D, n_out, variant, rng) if kp is None else kp
    n_w = gr.weight_count(kp, M)
    p = dict(Z=Z, Y=Y, kp=kp, nd=np.full(n_out, NDIAG), D=D, n_out=n_out, N=N, S=S, M=M, n_w=n_w, G=len(gr.groups(kp)),
             omega=rng.standard_normal((M, D)), tau=rng.uniform(0, 2 * np.pi, M),
             w=rng.standard_normal((n_out, S, n_w)), eps=rng.standard_normal((n_out, S, N)),
             x=rng.uniform(-1.2, 1.2, (T, D)), xs=rng.uniform(-1.2, 1.2, (S, D)))
    p["c"] = _both(p)
    _CACHE[key] = p
    return p


def _ref(p, fn, x):
    a, b = (fn(x, p["Z"], p["kp"], p["omega"], p["tau"], p["w"], p["c"][r]) for r in ("chol", "lu"))
    e0, scale = float(np.abs(a - b).max()), float(np.abs(a).max())
    return a, e0, scale, max(20.0 * e0, 1e-12 * scale * np.sqrt(p["N"] + p["n_w"]))


def _gp(p, kp=None):
    """a fitted model whose handle holds the packed parameters (through sr_gp_set_data_general), diagonal term NDIAG"""
    from safe_exploration_amd import SimpleGPModel
    kp = p["kp"] if kp is None else kp
    n_out, D = kp.shape[0], p["Z"].shape[1]
    n_in = max(1, D - 1)
    gp = SimpleGPModel(n_out, n_in, D - n_in, kern_types=["lin_rbf"] * n_out,
                       hyp=[{"noise_variance": NDIAG - 1e-5 - orc.GPY_JITTER} for _ in range(n_out)])
    gp._pack_kernel_params = lambda only=None: kp.copy() if only is None else kp[only:only + 1].copy()
    gp.train(p["Z"], p["Y"], opt_hyp=False)
    return gp


def _draw(gp, p, **over):
    d = dict(omega=p["omega"], tau=p["tau"], w=p["w"], eps=p["eps"])
    d.update(over)
    gp.draw_paths(p["S"], p["M"], **d)


def _np(t):
    return t.cpu().numpy()


MARGINS = []


def _report(what, tag, p, e0, err, bar):
    MARGINS.append(bar / max(err, 1e-300))
    print("paths gen %-7s %-2s N=%d S=%d M=%d D=%d n_out=%d G=%d n_w=%d  e0=%.3e  err=%.3e  bar=%.3e  margin=%.1f"
          % (what, tag, p["N"], p["S"], p["M"], p["D"], p["n_out"], p["G"], p["n_w"], e0, err, bar, bar / max(err, 1e-300)))


def _check(gp, p, tag):
    """F and J of _eval / _eval_grad and _step / _step_grad against the reference, every element; F of the _grad forms bit for
    bit F of the plain forms; the step against the diagonal of the evaluation"""
    S, D, n_out, T = p["S"], p["D"], p["n_out"], p["x"].shape[0]
    F = gp.sample_paths(p["x"])
    Fg, J = gp.sample_paths(p["x"], jacobians=True)
    Fs = _np(gp.paths_step_device(p["xs"]))
    Fsg, Js = (_np(t) for t in gp.paths_step_device(p["xs"], jacobians=True))
    assert F.shape == (T, S, n_out) and J.shape == (T, S, n_out, D) and Fs.shape == (S, n_out) and Js.shape == (S, n_out, D)
    assert all(np.all(np.isfinite(a)) for a in (F, J, Fs, Js))
    checks = []
    for what, got, fn, x in (("eval F", F, gr.evaluate, p["x"]), ("eval J", J, gr.evaluate_grad, p["x"]),
                             ("step F", Fs, gr.step, p["xs"]), ("step J", Js, gr.step_grad, p["xs"])):
        ref, e0, scale, bar = _ref(p, fn, x)
        err = float(np.abs(got - ref).max())
        _report(what, tag, p, e0, err, bar)
        checks.append((what, err, bar, scale))
    Fd, Jd = gp.sample_paths(p["xs"], jacobians=True)
    ar = np.arange(S)
    dF, dJ = float(np.abs(Fs - Fd[ar, ar]).max()), float(np.abs(Js - Jd[ar, ar]).max())
    print("paths gen diag    %-2s |step - eval[s, s]|: F %.3e (bar %.3e)  J %.3e (bar %.3e)"
          % (tag, dF, 1e-12 * checks[2][3], dJ, 1e-12 * checks[3][3]))
    np.testing.assert_array_equal(F, Fg)
    np.testing.assert_array_equal(Fs, Fsg)
    for what, err, bar, _ in checks:
        assert err <= bar, what
    assert dF <= 1e-12 * checks[2][3] and dJ <= 1e-12 * checks[3][3]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-S%d-M%d-T%d-D%d-o%d" % c[:6])
def test_eval_and_step_against_the_reference(case, variant):
    N, S, M, T, D, n_out, chunk = case
    p = _problem(N, S, M, T, D, n_out, variant)
    assert p["G"] == 1 if variant == "g1" else p["G"] >= 2
    gp = _gp(p)
    if chunk:
        gp.set_chunk(chunk)
    assert gp.paths_count() == (0, 0) and gp.paths_weight_count(M) == p["n_w"]
    _draw(gp, p)
    assert gp.paths_count() == (S, M)                    # (the base count, not n_w)
    _check(gp, p, variant)


@pytest.mark.parametrize("case", [(64, 16, 16, 16, 3, 2, None), (130, 65, 17, 129, 5, 1, None)],
                         ids=lambda c: "N%d-S%d-M%d-T%d-D%d-o%d" % c[:6])
def test_no_active_group(case):
    """G = 0: n_w = D, the base strips of the feature slab write nothing, the last strip fills it (the D linear rows and the
    padding up to 16); the step's feature loop adds nothing"""
    N, S, M, T, D, n_out, _ = case
    p = _problem(N, S, M, T, D, n_out, "g0")
    assert p["G"] == 0 and p["n_w"] == D
    gp = _gp(p)
    assert gp.paths_weight_count(M) == D
    _draw(gp, p)
    assert gp.paths_count() == (S, M)
    _check(gp, p, "g0")


def test_the_cases_cover_the_padding_edges_of_the_weights():
    """n_w at a multiple of 16 and one past it; a group with zero amplitude on one output"""
    nws = [_problem(*c[:6], "g1")["n_w"] for c in CASES[-2:]]
    assert nws[0] % 16 == 0 and nws[1] % 16 == 1
    p = _problem(*CASES[2][:6], "gn")
    D = p["D"]
    amp = np.array([[p["kp"][o, 2] if l == 0 else p["kp"][o, 3 + D + l - 1] for l in gr.groups(p["kp"])] for o in range(2)])
    assert np.any(amp == 0.0) and np.all(amp.max(axis=0) > 0.0)


def test_rbf_model_and_the_same_model_packed_into_the_family():
    """an "rbf" model through sr_gp_set_data and the same model as c0 = 1, a = b = 0, s = 1 / l: F and J agree within the bar
    (the family's weights behind the first M are zero-amplitude linear features)"""
    import test_gpu_paths as tg
    N, S, M, T, D, n_out = 300, 129, 100, 300, 3, 2
    q = tg._problem(N, S, M, T, D, n_out)
    kp = np.zeros((n_out, 3 + 3 * D))
    kp[:, 1], kp[:, 2], kp[:, 3:3 + D] = q["sf2"], 1.0, 1.0 / q["ls"]
    rng = np.random.default_rng(2)
    w = np.concatenate((q["w"], rng.standard_normal((n_out, S, D))), axis=2)
    p = dict(Z=q["Z"], Y=q["Y"], kp=kp, nd=np.full(n_out, NDIAG), D=D, n_out=n_out, N=N, S=S, M=M, n_w=M + D, G=1,
             omega=q["omega"], tau=q["tau"], w=w, eps=q["eps"], x=q["x"], xs=q["xs"])
    p["c"] = _both(p)
    ga, gg = tg._gp(q), _gp(p)
    tg._draw(ga, q)
    _draw(gg, p)
    assert gg.paths_weight_count(M) == M + D and ga.paths_weight_count(M) == M
    Fa, Ja = ga.sample_paths(q["x"], jacobians=True)
    Fg, Jg = gg.sample_paths(p["x"], jacobians=True)
    Fsa, Jsa = (_np(t) for t in ga.paths_step_device(q["xs"], jacobians=True))
    Fsg, Jsg = (_np(t) for t in gg.paths_step_device(p["xs"], jacobians=True))
    for what, a, g, fn, x in (("eval F", Fa, Fg, gr.evaluate, p["x"]), ("eval J", Ja, Jg, gr.evaluate_grad, p["x"]),
                              ("step F", Fsa, Fsg, gr.step, p["xs"]), ("step J", Jsa, Jsg, gr.step_grad, p["xs"])):
        ref, e0, scale, bar = _ref(p, fn, x)
        err = float(np.abs(a - g).max())
        _report(what, "ab", p, e0, err, bar)
        assert err <= bar and np.abs(g - ref).max() <= bar, what


def test_zero_draws_are_the_posterior_mean():
    p = _problem(300, 129, 100, 300, 3, 2, "gn")
    gp = _gp(p)
    _draw(gp, p, w=0 * p["w"], eps=0 * p["eps"])
    F = gp.sample_paths(p["x"])
    mu = gp.predict(p["x"])[0]
    atol = 1e-12 * float(np.abs(gp.beta).sum(0).max() * max(gr.kernel(p["x"], p["Z"], k).max() for k in p["kp"]))
    for s in range(p["S"]):
        np.testing.assert_allclose(F[:, s, :], mu, rtol=1e-9, atol=atol)


def test_bitwise_repeatable():
    p = _problem(300, 129, 100, 300, 3, 2, "gn")
    gp = _gp(p)
    gp.set_chunk(128)
    outs = []
    for _ in range(2):
        _draw(gp, p)
        outs.append(gp.sample_paths(p["x"], jacobians=True) + tuple(_np(t) for t in gp.paths_step_device(p["xs"], jacobians=True)))
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)
    again = gp.sample_paths(p["x"], jacobians=True)         # a second call on the same paths
    np.testing.assert_array_equal(again[0], outs[0][0])
    np.testing.assert_array_equal(again[1], outs[0][1])


def test_closed_loop_z_next():
    p = _problem(129, 65, 17, 129, 5, 4, "gn")
    gp = _gp(p)
    _draw(gp, p)
    rng = np.random.default_rng(3)
    kfb, kff = 0.3 * rng.standard_normal((1, 4)), 0.1 * rng.standard_normal(1)
    F0 = _np(gp.paths_step_device(p["xs"]))
    F1, z1 = (_np(t) for t in gp.paths_step_device(p["xs"], kfb, kff))
    F2, z2, J2 = (_np(t) for t in gp.paths_step_device(p["xs"], kfb, kff, jacobians=True))
    np.testing.assert_array_equal(F0, F1)
    np.testing.assert_array_equal(F0, F2)
    np.testing.assert_array_equal(z1, z2)
    np.testing.assert_array_equal(z1[:, :4], F1)
    np.testing.assert_allclose(z1[:, 4:], F1.dot(kfb.T) + kff[None, :], rtol=1e-14, atol=1e-15)
    np.testing.assert_array_equal(J2, _np(gp.paths_step_device(p["xs"], jacobians=True)[1]))


def _eval_rc(gp, x):
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    xt = B.as_dev(x, hd.device)
    F = B.empty((x.shape[0], max(1, gp.paths_count()[0]), hd.n_out), hd.device)
    return lib.sr_gp_paths_eval(hd.h, B.ptr(xt), x.shape[0], B.ptr(F), B.stream_ptr(hd.device))


def _draw_rc(gp, p):
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    hd = gp._handle
    t = [B.as_dev(p[k], hd.device) for k in ("omega", "tau", "w", "eps")]
    return lib.sr_gp_paths_draw(hd.h, p["S"], p["M"], B.ptr(t[0]), B.ptr(t[1]), B.ptr(t[2]), B.ptr(t[3]), B.stream_ptr(hd.device))


def _check_against(gp, p):
    ref, _, _, bar = _ref(p, gr.evaluate, p["x"])
    assert np.abs(gp.sample_paths(p["x"]) - ref).max() <= bar


def test_model_updates_invalidate_the_paths():
    p = _problem(200, 40, 32, 9, 3, 2, "gn")
    gp = _gp(p)
    assert _eval_rc(gp, p["x"]) == SR_ESTATE                          # before any draw
    _draw(gp, p)
    _check_against(gp, p)
    # a refit with other data (the parameters stay): no paths until the next draw, which is right for the new model
    q = _problem(200, 40, 32, 9, 3, 2, "gn", seed=77, kp=p["kp"])
    gp.update_model(q["Z"], q["Y"], opt_hyp=False, replace_old=True)
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE
    with pytest.raises(RuntimeError):
        gp.sample_paths(p["x"])
    _draw(gp, q)
    _check_against(gp, q)
    # removal
    gp.remove_data([3, 150])
    assert gp.paths_count() == (0, 0) and _eval_rc(gp, p["x"]) == SR_ESTATE
    keep = np.delete(np.arange(200), [3, 150])
    r = dict(q, Z=q["Z"][keep], Y=q["Y"][keep], eps=q["eps"][:, :, keep], N=198)
    r["c"] = _both(r)
    _draw(gp, r)
    _check_against(gp, r)
    gp.drop_paths()
    assert gp.paths_count() == (0, 0)


@pytest.mark.parametrize("which", ["v", "c0", "a", "b"])
def test_negative_parameter_is_refused(which):
    """SR_EINVAL at the draw and at the weight count, the parameter named in the error text; the paths of the handle (none: every
    change of the parameters has invalidated them) and those of another model stay as they are"""
    from safe_exploration_amd._lib import lib, last_error
    p = _problem(64, 16, 16, 16, 4, 2, "gn")
    good = _gp(p)
    _draw(good, p)
    F = good.sample_paths(p["x"])
    kp = p["kp"].copy()
    D = p["D"]
    col, name = {"v": (1, "v"), "c0": (2, "c0"), "a": (3 + D + 2, "a[2]"), "b": (3 + 2 * D + 1, "b[1]")}[which]
    kp[1, col] = -5e-5                                   # (small: K_y stays positive definite, the model fits)
    bad = _gp(p, kp)
    assert _draw_rc(bad, p) == SR_EINVAL
    assert "output 1: %s = %g" % (name, -5e-5) in last_error()
    n_w = ctypes.c_int(-1)
    assert lib.sr_gp_paths_weight_count(bad._handle.h, p["M"], ctypes.byref(n_w)) == SR_EINVAL and n_w.value == -1
    with pytest.raises(ValueError):
        _draw(bad, p)
    assert bad.paths_count() == (0, 0) and _eval_rc(bad, p["x"]) == SR_ESTATE
    np.testing.assert_array_equal(good.sample_paths(p["x"]), F)
    # the model itself is served as before
    assert np.all(np.isfinite(bad.predict(p["x"])[0]))


def test_rollout_in_one_launch_is_refused_paths_intact():
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    p = _problem(64, 16, 16, 16, 4, 2, "g1")             # D = 4: n_s = 2 states ... the model class holds n_in = 3, n_u = 1
    gp = _gp(p)
    _draw(gp, p)
    F = gp.sample_paths(p["x"])
    hd = gp._handle
    H, S, n_s, n_u = 3, p["S"], 2, 2
    dev = hd.device
    x0, K, k = B.as_dev(np.zeros(n_s), dev), B.as_dev(np.zeros((H, n_u, n_s)), dev), B.as_dev(np.zeros((H, n_u)), dev)
    X = B.empty((H, S, n_s), dev)
    assert lib.sr_gp_paths_rollout(hd.h, B.ptr(x0), 0, H, B.ptr(K), B.ptr(k), B.ptr(X), None, B.stream_ptr(dev)) == SR_EUNSUPPORTED
    assert lib.sr_gp_paths_rollout_vjp(hd.h, B.ptr(x0), 0, H, B.ptr(K), B.ptr(k), B.ptr(X), B.ptr(X), B.ptr(x0), B.ptr(K),
                                       B.ptr(k), None, B.stream_ptr(dev)) == SR_EUNSUPPORTED
    assert gp.paths_count() == (p["S"], p["M"])
    np.testing.assert_array_equal(gp.sample_paths(p["x"]), F)
    with pytest.raises(NotImplementedError):
        gp.paths_rollout_device(np.zeros(n_s), np.zeros((H, n_u, n_s)), np.zeros((H, n_u)))
    with pytest.raises(NotImplementedError):
        gp.paths_rollout_diff_device(np.zeros(n_s), np.zeros((H, n_u, n_s)), np.zeros((H, n_u)))
    with pytest.raises(NotImplementedError):
        MonteCarloSafetyVerification(gp).rollout_paths_diff(np.zeros((3, 1)), np.zeros((H, 1, 3)), np.zeros((H, 1)), n=H,
                                                            n_samples=S)
    np.testing.assert_array_equal(gp.sample_paths(p["x"]), F)


@pytest.mark.parametrize("kts", [("lin_rbf", "lin_rbf"), ("rbf", "lin_rbf")], ids=["lin_rbf", "mixed"])
def test_consistent_rollout_on_in_tree_models(kts):
    """sample_n_step(consistent=True) and sample_n_step_jacobians, H = 4, 33 particles, through the model class as it is: every
    step against the reference at the kernel's own inputs (the device's previous states) within the step's bar; rollout_paths
    falls back to the same chained route (the same bits)"""
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    n_s, n_u, N, H, S, M = 2, 1, 60, 4, 33, 64
    D = n_s + n_u
    rng = np.random.default_rng(11)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_s)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_s))
    hyp = [dict(orc.make_hyp(kt, rng, D), noise_variance=NDIAG - 1e-5 - orc.GPY_JITTER) for kt in kts]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=list(kts), hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    kp = gp._pack_kernel_params()
    G = len(gr.groups(kp))
    assert G == (1 if kts[0] == "lin_rbf" else 2) and gp.paths_weight_count(M) == G * M + D
    p = dict(Z=Z, Y=Y, kp=kp, nd=np.full(n_s, NDIAG), D=D, n_out=n_s, N=N, S=S, M=M, n_w=G * M + D, G=G,
             omega=rng.standard_normal((M, D)), tau=rng.uniform(0, 2 * np.pi, M),
             w=rng.standard_normal((n_s, S, G * M + D)), eps=rng.standard_normal((n_s, S, N)))
    p["c"] = _both(p)
    K, k = 0.3 * rng.standard_normal((H, n_u, n_s)), 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, (n_s, 1))
    mc = MonteCarloSafetyVerification(gp)
    _draw(gp, p)
    S_last, S_all = mc.sample_n_step(x0, K, k, n=H, n_samples=S, consistent=True, n_features=M)
    S2, S_all2, A_all = mc.sample_n_step_jacobians(x0, K, k, n=H, n_samples=S, n_features=M)
    assert gp.paths_count() == (S, M) and S_all.shape == (H, S, n_s) and A_all.shape == (H, S, n_s, n_s)
    np.testing.assert_array_equal(S_all, S_all2)
    np.testing.assert_array_equal(S_last, S_all[H - 1])
    x = np.tile(x0.T, (S, 1))
    for i in range(H):
        inp = np.hstack((x, x.dot(K[i].T) + k[i][None, :]))
        ref, e0, scale, bar = _ref(p, gr.step, inp)
        err = float(np.abs(S_all[i] - ref).max())
        _report("roll F%d" % i, kts[0][:2], p, e0, err, bar)
        Jr, je0, jscale, jbar = _ref(p, gr.step_grad, inp)
        Ar = Jr[..., :n_s] + Jr[..., n_s:].dot(K[i])
        # (A = J_x + J_u K[i]: the bar of J with the gain's row sums)
        abar = jbar * (1.0 + np.abs(K[i]).sum())
        aerr = float(np.abs(A_all[i] - Ar).max())
        _report("roll A%d" % i, kts[0][:2], p, je0, aerr, abar)
        assert err <= bar and aerr <= abar
        x = S_all[i]
    # the reference's own closed loop, for information: the steps' errors pass through H - 1 Jacobians
    full = gr.rollout(x0[:, 0], K, k, Z, kp, p["omega"], p["tau"], p["w"], p["c"]["chol"])
    print("paths gen rollout against the reference's closed loop: %.3e (scale %.3e)" % (np.abs(S_all - full).max(), np.abs(full).max()))
    out = mc.rollout_paths(x0, K, k, n=H, n_samples=S, n_features=M, jacobians=True)
    np.testing.assert_array_equal(out[1], S_all)
    np.testing.assert_array_equal(out[2], A_all)
    with pytest.raises(NotImplementedError):
        mc.rollout_paths_diff(x0, K, k, n=H, n_samples=S, n_features=M)
    with pytest.raises(NotImplementedError):             # one start per particle: the one-launch roll-out only
        mc.rollout_paths(np.tile(x0.T, (S, 1)), K, k, n=H, n_samples=S, n_features=M)
    assert gp.paths_count() == (S, M)
    # another particle count: the paths are drawn afresh from the generator, with the family's weight count
    mc.sample_n_step(x0, K, k, n=H, n_samples=17, consistent=True, n_features=M)
    assert gp.paths_count() == (17, M)


def test_thinnest_margin_is_reported():
    """(runs last: prints the thinnest margin of the module's comparisons against the reference)"""
    if MARGINS:
        print("paths gen thinnest margin: %.2f over %d comparisons" % (min(MARGINS), len(MARGINS)))
        assert min(MARGINS) >= 1.0
