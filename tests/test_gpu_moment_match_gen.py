"""sr_gp_moment_match on the general-family route (kappa = RBF on every output; csrc/sr_moment_match_gen.hip) and the
propagation built on it, against the unexpanded closed form in NumPy fp64 (tests/_mm_gen_ref.py, itself held against quadrature
and against the ARD-RBF reference by tests/test_moment_match_gen_host.py).

The reference is fed the device's OWN alpha (export_alpha) and K_y^-1 (a fresh sr_gp_inv_k), so only the new kernels'
rounding is under test, not the conditioning of the factorisation.  The inputs are those of tests/_mm_gen_cases.py; models with
arbitrary packed parameters [0, v, c0, s, a, b] go through the model class with its parameter packing replaced (``_gp``), the
in-tree "lin_rbf" / "rbf" kernels through the class as it is.

Bars: mu and V rtol 1e-10, atol 1e-12 sum_i |alpha_ai| max_i |E k_ai|; Cov atol 1e-9 max_a E[k_a(x, x)] (the ARD-RBF test's bar
with the family's prior scale); propagated moments rtol 1e-8.  The rounding floor of the reference alone (fp64 against long
double on these inputs, model fitted in NumPy; test_moment_match_gen_host.py) is at most 3.4e-4 of the mu bar, 1.7e-4 of the V
bar and 3.2e-2 of the Cov bar (corner s1; the covariance kinds 9e-3, N = 300 9e-4, the +5 translation 1.7e-3).  All models here have noise 1e-2:
at noise 1e-3 the Cov floor at N = 300 comes within 12 x of its bar.

Observed on MI355X, for information (each check prints its figures, absolute and as a fraction of its bar): widths mu <= 1.6e-14,
V <= 1.7e-14, Cov <= 8.4e-13 (6e-4 of the bar); sizes Cov <= 2.2e-12 (2e-3); covariance kinds (the in-tree structure, prior
variance ~0.02 near the origin) Cov 1.1e-11 (1.4e-2); corners Cov <= 4.2e-11 (3.5e-2, s1); the +5 translation mu 7.4e-14, Cov
3.9e-11 (2e-3); against the ARD-RBF route Cov 1.9e-13; sparse Cov 8.0e-12; S = 0 against predict_device mu 6.4e-15, V 6.1e-15,
var 1.7e-13; propagated moments within 8.6e-14.  mu and V never above 6e-4 of their bars.

Tile sizes of the double-sum kernel the size edges are derived from: SR_MMX_IT = 64 rows i per workgroup, SR_MMX_JT = 256 rows j
per staged tile; the model is padded to blocks of 128 rows."""
import numpy as np
import pytest

import _mm_gen_cases as C
import _mm_gen_ref as G

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _gp(Z, Y, kp, noise):
    """a fitted model whose handle holds the packed parameters kp (through sr_gp_set_data_general)"""
    from safe_exploration_amd import SimpleGPModel
    n_out, D = kp.shape[0], Z.shape[1]
    n_in = max(1, D - 1)
    gp = SimpleGPModel(n_out, n_in, D - n_in, kern_types=["lin_rbf"] * n_out,
                       hyp=[{"noise_variance": float(noise[o])} for o in range(n_out)])
    gp._pack_kernel_params = lambda only=None: kp.copy() if only is None else kp[only:only + 1].copy()
    gp.train(Z, Y, opt_hyp=False)
    return gp


def _model_arrays(gp, Z):
    """what the handle holds NOW: alpha by export_alpha, K_y^-1 by a fresh sr_gp_inv_k (not the model's cached copy)"""
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    assert hd.N == Z.shape[0]
    alpha = B.to_numpy(gp.export_alpha())
    M = np.empty((hd.n_out, hd.N, hd.N))
    for d in range(hd.n_out):
        t = B.empty((hd.N, hd.N), hd.device)
        check(lib.sr_gp_inv_k(hd.h, d, B.ptr(t), B.stream_ptr(hd.device)))
        M[d] = B.to_numpy(t)
    return G.params_from_packed(gp._pack_kernel_params()), Z, alpha, M


def _compare(tag, got, ref):
    """prints the figures, then asserts the bars of the module docstring"""
    (mu, cov, V), (rmu, rcov, rV, (mu_scale, kxx)) = got, ref
    at, ct = 1e-12 * mu_scale, 1e-9 * kxx.max(axis=1)
    print("mmx %s: mu %.2e (%.1e of its atol), V %.2e (%.1e), cov %.2e (%.1e)" % (
        tag, np.abs(mu - rmu).max(), (np.abs(mu - rmu) / at).max(), np.abs(V - rV).max(),
        (np.abs(V - rV) / at[:, :, None]).max(), np.abs(cov - rcov).max(), (np.abs(cov - rcov) / ct[:, None, None]).max()))
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(cov)) and np.all(np.isfinite(V))
    assert np.all(np.abs(mu - rmu) <= 1e-10 * np.abs(rmu) + at), tag
    assert np.all(np.abs(V - rV) <= 1e-10 * np.abs(rV) + at[:, :, None]), tag
    assert np.all(np.abs(cov - rcov) <= ct[:, None, None]), tag
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1))), tag


def _run(gp, m, S):
    from safe_exploration_amd import _buffers as B
    return tuple(B.to_numpy(o) for o in gp.moment_match_device(m, S))


def _check(tag, case, gp=None):
    Z, Y, kp, noise, m, S = case
    gp = _gp(Z, Y, kp, noise) if gp is None else gp
    got = _run(gp, m, S)
    _compare(tag, got, G.moment_match_batch(*_model_arrays(gp, Z), m, S))
    return gp, got


# ------------------------------------------------------------------ widths
@pytest.mark.parametrize("kind", C.S_KINDS)
@pytest.mark.parametrize("D", C.WIDTHS)
def test_every_width(D, kind):
    """every instantiation of the kernels with D < DT and D == DT at N = 130, T = 5; two outputs whose parameters differ"""
    _, (mu, cov, V) = _check("width D=%d %s" % (D, kind), C.width_case(D, kind))
    if kind == "zero":
        assert np.all(cov[:, 0, 1] == 0.0)
    else:
        assert np.abs(cov[:, 0, 1]).max() > 1e-9          # the cross-covariance is informative


# ------------------------------------------------------------------ size edges
@pytest.mark.parametrize("N", C.SIZES)
def test_every_size_edge(N):
    """one and two rows; either side of the i tile (64) and of the j tile (256); 300: past one padded block and a second j
    tile (the symmetric half of the double sum)"""
    gp = None
    for kind in ("full", "zero"):
        gp, _ = _check("size N=%d %s" % (N, kind), C.size_case(N, kind), gp)


# ------------------------------------------------------------------ outputs
@pytest.mark.parametrize("n_out", [1, 3])
def test_outputs_on_one_handle(n_out):
    """per-output parameters that differ; the diagonal blocks of Cov, mu and V of each output are bit-identical to the model of
    that output alone"""
    case = C.outputs_case(n_out)
    Z, Y, kp, noise, m, S = case
    _, (mu, cov, V) = _check("outputs n_out=%d" % n_out, case)
    for o in range(n_out):
        mu1, cov1, V1 = _run(_gp(Z, Y[:, o:o + 1], kp[o:o + 1], noise[o:o + 1]), m, S)
        assert np.array_equal(mu1[:, 0], mu[:, o]) and np.array_equal(V1[:, 0], V[:, o]), o
        assert np.array_equal(cov1[:, 0, 0], cov[:, o, o]), o


# ------------------------------------------------------------------ covariance kinds
def test_covariance_kinds():
    """zero (None and a zero array give the same bits), rank 1, full; identical rows give identical results"""
    gp = None
    for kind in C.S_KINDS + ("same",):
        case = C.kinds_case(kind)
        gp, got = _check("kinds %s" % kind, case, gp)
        if kind == "zero":
            m = case[4]
            zero = _run(gp, m, np.zeros((len(m), 3, 3)))
            assert all(np.array_equal(x, y) for x, y in zip(got, zero)), "S = None and S = 0 differ"
        if kind == "same":
            assert all(np.array_equal(x, np.repeat(x[:1], len(x), axis=0)) for x in got), "identical rows differ"


# ------------------------------------------------------------------ parameter corners
@pytest.mark.parametrize("corner", ["s1", "a0", "b0", "c00", "lin_rbf"])
def test_parameter_corner(corner):
    _check("corner %s" % corner, C.corner_case(corner))


def test_rbf_corner_is_the_ard_rbf_route():
    """a = 0, b = 0, c0 = 1: the new route against the ARD-RBF route on the same data and hyper-parameters"""
    from safe_exploration_amd import SimpleGPModel
    case = C.corner_case("rbf")
    Z, Y, kp, noise, m, S = case
    gp, got = _check("corner rbf", case)
    hyp = [{"lengthscale": 1.0 / kp[o, 3:6], "variance": kp[o, 1], "noise_variance": noise[o]} for o in range(2)]
    rbf = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp)
    rbf.train(Z, Y, opt_hyp=False)
    ref = _run(rbf, m, S)
    scales = G.moment_match_batch(*_model_arrays(gp, Z), m, S)[3]
    _compare("general route against the ARD-RBF route", got, ref + (scales,))


def test_translated_inputs():
    """inputs and data translated by +5: the linear parts dominate and - mu_a mu_b cancels against them"""
    _check("shift +%g" % C.SHIFT, C.corner_case("dense", C.SHIFT))


# ------------------------------------------------------------------ the limit S = 0
def test_point_limit_is_predict():
    """S = 0 against predict_device(compute_gradients=True) of the same model: mu, the mean Jacobian, the variance"""
    from safe_exploration_amd import _buffers as B
    Z, Y, kp, noise = C.problem(("limit",), 150, 3, 2)
    gp = _gp(Z, Y, kp, noise)
    m, _ = C.inputs(("limit-q",), Z, 6, "zero")
    ref = G.moment_match_batch(*_model_arrays(gp, Z), m, None)
    at, ct = 1e-12 * ref[3][0], 1e-9 * ref[3][1].max(axis=1)
    pmu, pvar, pjac = (B.to_numpy(o) for o in gp.predict_device(m, compute_gradients=True))
    mu, cov, V = _run(gp, m, None)
    var = np.diagonal(cov, axis1=1, axis2=2)
    print("limit: mu %.2e, V %.2e, var %.2e" % (np.abs(mu - pmu).max(), np.abs(V - pjac).max(), np.abs(var - pvar).max()))
    assert np.all(np.abs(mu - pmu) <= 1e-10 * np.abs(pmu) + at)
    assert np.all(np.abs(V - pjac) <= 1e-10 * np.abs(pjac) + at[:, :, None])
    assert np.all(np.abs(var - pvar) <= ct[:, None])
    assert np.all(cov[:, 0, 1] == 0.0) and np.all(cov[:, 1, 0] == 0.0)


# ------------------------------------------------------------------ layout, chunks, determinism
def test_layout_chunks_and_determinism():
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    case = C.width_case(3, "full")
    Z, Y, kp, noise, m, S = case
    gp, first = _check("layout", case)
    hd = gp._handle
    kinv = gp.inv_K_device()
    tm, tS = B.as_dev(m, hd.device), B.as_dev(S, hd.device)

    def call(T, with_V=True):
        """through the C-ABI into sentinel-filled buffers with room for 3 more queries"""
        mu = torch.full((T + 3, 2), SENTINEL, dtype=torch.float64, device=hd.device)
        cov = torch.full((T + 3, 2, 2), SENTINEL, dtype=torch.float64, device=hd.device)
        V = torch.full((T + 3, 2, 3), SENTINEL, dtype=torch.float64, device=hd.device)
        check(lib.sr_gp_moment_match(hd.h, B.ptr(tm), B.ptr(tS), T, B.ptr(kinv), B.ptr(mu), B.ptr(cov),
                                     B.ptr(V) if with_V else None, B.stream_ptr(hd.device)))
        outs = [B.to_numpy(o) for o in (mu, cov, V)]
        assert all(np.all(o[T:] == SENTINEL) for o in outs), "written past T=%d" % T
        assert with_V or np.all(outs[2] == SENTINEL)
        return [o[:T] for o in outs]

    whole = call(5)
    assert all(np.array_equal(x, y) for x, y in zip(whole, first)), "the C-ABI and the model class differ"
    assert all(np.array_equal(x, y) for x, y in zip(whole, call(5))), "two calls differ"
    part = call(2)
    assert all(np.array_equal(x, y[:2]) for x, y in zip(part, whole)), "T = 2 differs from the first rows of T = 5"
    gp.set_chunk(2)
    assert all(np.array_equal(x, y) for x, y in zip(whole, call(5))), "chunking changed the bits"       # chunks 2, 2, 1
    no_v = call(5, with_V=False)
    assert np.array_equal(no_v[0], whole[0]) and np.array_equal(no_v[1], whole[1])
    assert lib.sr_gp_moment_match(hd.h, None, None, 0, None, None, None, None, B.stream_ptr(hd.device)) == 0


# ------------------------------------------------------------------ the model class
def _lin_rbf_model(kern_types, N, D, n_u, key):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(C.seed(*key))
    Z = rng.uniform(-1, 1, (N, D))
    n = len(kern_types)
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n)) / np.sqrt(D))) + 0.3 * Z.dot(rng.standard_normal((D, n)))
    hyp = []
    for kt in kern_types:
        if kt == "rbf":
            hyp.append({"lengthscale": rng.uniform(0.6, 1.4, D), "variance": float(rng.uniform(0.5, 1.5)), "noise_variance": 1e-2})
        else:
            hyp.append({"prod.rbf.lengthscale": rng.uniform(0.6, 1.4, 1), "prod.rbf.variance": float(rng.uniform(0.5, 1.5)),
                        "prod.linear.variances": rng.uniform(0.3, 0.9, 1), "linear.variances": rng.uniform(0.1, 0.5, D),
                        "noise_variance": 1e-2})
    gp = SimpleGPModel(n, D - n_u, n_u, kern_types=list(kern_types), hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp, Z


@pytest.mark.parametrize("kern_types", [("lin_rbf", "lin_rbf"), ("lin_rbf", "rbf")])
def test_model_class(kern_types):
    """the in-tree kernels through predict_uncertain; a mixed model goes through the general packing"""
    gp, Z = _lin_rbf_model(kern_types, 80, 3, 1, ("class",) + kern_types)
    m, S = C.inputs(("class-q",), Z, 3, "full")
    got = gp.predict_uncertain(m, S)
    _compare("model class %s" % "/".join(kern_types), got, G.moment_match_batch(*_model_arrays(gp, Z), m, S))
    one = gp.predict_uncertain(m[0], S[0])
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(one, got))


def test_sparse_model():
    """a do_sparse_gp model (32 inducing rows over N = 400): sr_gp_inv_k gives P P^T, the matrix of its variance"""
    from safe_exploration_amd import SimpleGPModel
    X, Y, kp, noise = C.problem(("sparse",), 400, 3, 2)
    gp = SimpleGPModel(2, 2, 1, kern_types=["lin_rbf"] * 2, hyp=[{"noise_variance": 1e-2}] * 2)
    gp._pack_kernel_params = lambda only=None: kp.copy() if only is None else kp[only:only + 1].copy()
    gp.do_sparse_gp = True
    gp.train(X, Y, 32, opt_hyp=False, Z=X[:32])
    assert gp.is_sparse
    m, S = C.inputs(("sparse-q",), X, 3, "full")
    got = _run(gp, m, S)
    _compare("sparse", got, G.moment_match_batch(*_model_arrays(gp, X[:32]), m, S))


# ------------------------------------------------------------------ propagation
def test_multi_step_propagation():
    """H = 3 roll-out of a lin_rbf model from N(mu_0, sigma_0), against the closed form composed step by step"""
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    n_s, n_u, H = 2, 1, 3
    gp, Z = _lin_rbf_model(("lin_rbf",) * n_s, 80, n_s + n_u, n_u, ("prop",))
    arrs = _model_arrays(gp, Z)
    rng = np.random.default_rng(C.seed("prop-c"))
    a, b = 0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), 0.3 * rng.standard_normal((n_s, n_u))
    mu_0 = 0.3 * rng.standard_normal(n_s)
    k_ff, k_fb = 0.2 * rng.standard_normal((H, n_u)), 0.4 * rng.standard_normal((H - 1, n_u, n_s))
    L = 0.15 * rng.standard_normal((n_s, n_s))
    s0 = L.dot(L.T)
    mu_all, sigma_all, var_all = up.multi_step_moment_matching(mu_0.reshape(n_s, 1), gp, k_ff, list(k_fb), s0, a, b)
    rm, rs, rc = G.propagate(*arrs, mu_0, k_ff, k_fb, a, b, s0)
    print("multi-step lin_rbf: mu %.2e sigma %.2e" % (np.abs(mu_all - rm).max(), np.abs(sigma_all.reshape(H, n_s, n_s) - rs).max()))
    np.testing.assert_allclose(mu_all, rm, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(sigma_all.reshape(H, n_s, n_s), rs, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(var_all, np.diagonal(rc, axis1=1, axis2=2), rtol=1e-8, atol=1e-12)


# ------------------------------------------------------------------ refusals
def test_refusals():
    """host-side refusals only: none of these launches a moment-matching kernel"""
    import torch
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    s = B.stream_ptr(dev)
    Z, Y, _, _ = C.problem(("refuse",), 50, 3, 1)
    buf = B.empty((64,), dev).fill_(SENTINEL)
    p = B.ptr(buf)
    # Matern radial parts: through the model class and through the C-ABI
    for kt, hyp in (("mat52", {"lengthscale": np.ones(3), "variance": 1.0, "noise_variance": 0.01}),
                    ("lin_mat52", {"noise_variance": 0.01})):
        gen = SimpleGPModel(1, 2, 1, kern_types=[kt], hyp=[hyp])
        gen.train(Z, Y, opt_hyp=False)
        with pytest.raises(NotImplementedError):
            gen.moment_match_device(Z[:2], None)
        assert gen._inv_K_dev is None
        assert lib.sr_gp_moment_match(gen._handle.h, p, None, 1, p, p, p, p, s) == _lib.SR_EUNSUPPORTED
        assert "ARD-RBF" in _lib.last_error()
    # the reverse pass of the family is not provided: refused before the forward runs
    lin = SimpleGPModel(1, 2, 1, kern_types=["lin_rbf"], hyp=[{"noise_variance": 0.01}])
    lin.train(Z, Y, opt_hyp=False)
    tm = torch.as_tensor(Z[:2], device=dev).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        lin.moment_match_device(tm, None, differentiable=True)
    with pytest.raises(NotImplementedError):
        lin.moment_match_vjp_device(Z[:2], None, mu_bar=np.ones((2, 1)))
    with pytest.raises(NotImplementedError):
        lin.predict_uncertain_vjp(Z[:2], None, mu_bar=np.ones((2, 1)))
    assert lin._inv_K_dev is None                        # nothing was prepared, nothing launched
    assert lib.sr_gp_moment_match_vjp(lin._handle.h, p, None, 1, p, p, None, None, p, p, s) == _lib.SR_EUNSUPPORTED
    assert "ARD-RBF" in _lib.last_error()
    # a handle that was never fitted
    raw = _Handle(dev, 50, 3, 1)
    assert lib.sr_gp_moment_match(raw.h, p, None, 1, p, p, p, p, s) == _lib.SR_ESTATE
    assert "not factorized" in _lib.last_error()
    # NULL arguments and a negative count on a good lin_rbf model
    h = lin._handle.h
    for args in ((None, None, 1, p, p, p, p), (p, None, 1, None, p, p, p), (p, None, 1, p, None, p, p),
                 (p, None, 1, p, p, None, p), (p, None, -1, p, p, p, p)):
        assert lib.sr_gp_moment_match(h, *(args + (s,))) == _lib.SR_EINVAL, args
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
