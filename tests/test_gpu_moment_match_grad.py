"""sr_gp_moment_match_vjp (the reverse pass of exact moment matching) and the autograd surface built on it, against the
analytic NumPy fp64 VJP of tests/_mm_grad_ref.py (itself held against torch autograd through the textbook forward and against
central differences by tests/test_moment_match_grad_host.py).

The reference is fed the device's OWN alpha (export_alpha) and K_y^-1 (a fresh sr_gp_inv_k), as the forward's test does, so
only the new kernels' rounding is under test.

Bars (``_mm_grad_ref.bars``), absolute, per query: 30 x the fp64 rounding floor of the reference itself (both of its summation
orders against long double at the size edges, same alpha and K_y^-1) at the scale of the seeds,
  m_bar, S_bar from mu / V seeds:  30 x 1.41e-16 x sigma_f |alpha|_1 |seed|_1 / min ls
  m_bar, S_bar from Cov seeds:     30 x 5.3e-13  x max sf2 |Cs|_1 / min ls^2
The two CPU references disagree by at most 8.7e-17 and 6.7e-13 of those scales.  The propagated gradients
(moment_matching_batch(differentiable=True)) are held to a relative bar on the largest element of each gradient: 30 x the
disagreement of two CPU routes to the same gradient (autograd through the torch port of the forward, and autograd through the
steps with the analytic VJP as the GP's backward), which is at most 4.47e-12 over the four cases of the test (fitted on the CPU) -> 1.35e-10.

Observed on MI355X, for information (each check prints its figures; "share" = worst error / bar):
  widths D = 1 .. 12 (N = 70):                  m_bar <= 2.0e-12, S_bar <= 2.5e-12, share <= 0.015
  sizes N = 1 .. 65 / 255 .. 300:               S_bar <= 1.2e-12 / 6.0e-12, share <= 0.010 / 0.036
  outputs 1, 2, 3, 8, every seed:               <= 1.1e-12, share <= 0.005
  model states (N = 600 .. 643):                <= 5.3e-12, share <= 0.020;  sparse handle 2.7e-11, share 0.11
  S = None against predict_device_grad:         d mu/dx 9.2e-15, d var/dx 4.5e-13 (bars 1.0e-12, 6.5e-12)
  propagated gradients:                         <= 5.0e-12 of the largest element

Tile sizes the size edges are derived from: the reverse pair pass keeps the forward's SR_MM_IT = 64 rows i per workgroup and
SR_MM_JT = 256 rows j per staged tile."""
import numpy as np
import pytest

import _mm_grad_ref as G
from test_gpu_moment_match import _problem, _gp, _inputs, _model_arrays, _seed, _slide, _prop_case, WIDTHS, S_KINDS, MM_IT, MM_JT

pytestmark = pytest.mark.gpu

SIZES = (1, 2, MM_IT - 1, MM_IT, MM_IT + 1, MM_JT - 1, MM_JT, MM_JT + 1, 300)
SENTINEL = -7.25
PROP_RTOL = 30 * 4.5e-12


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _seeds(seed, T, n, D):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, n)), rng.standard_normal((T, n, n)), rng.standard_normal((T, n, D))


def _run(gp, m, S, seeds):
    from safe_exploration_amd import _buffers as B
    return tuple(B.to_numpy(o) for o in gp.moment_match_vjp_device(m, S, *seeds))


def _compare(tag, got, ref, arrs, seeds):
    """prints the figures, then asserts the bars of the module docstring, query by query"""
    bar = G.bars(arrs[1], arrs[3], arrs[4], *seeds)
    em = np.abs(got[0] - ref[0]).max(axis=1)
    es = np.abs(got[1] - ref[1]).max(axis=(1, 2))
    print("mmg %s: m_bar %.2e, S_bar %.2e (bar %.1e; worst share of the bar %.3f)" % (
        tag, em.max(), es.max(), bar.min(), max((em / bar).max(), (es / bar).max())))
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])), tag
    assert np.all(em <= bar) and np.all(es <= bar), tag
    assert np.array_equal(got[1], np.transpose(got[1], (0, 2, 1))), tag


def _check(tag, gp, Z, m, S, seeds):
    arrs = _model_arrays(gp, Z)
    got = _run(gp, m, S, seeds)
    _compare(tag, got, G.vjp_batch(*arrs, m, S, *seeds), arrs, seeds)
    return got


# ------------------------------------------------------------------ widths
@pytest.mark.parametrize("kind", S_KINDS)
@pytest.mark.parametrize("D", WIDTHS)
def test_every_width(D, kind):
    """every instantiation of the kernels with D < DT and D == DT; two outputs with different lengthscales"""
    Z, Y, hyp = _problem(_seed("gwidth", D), 70, D, 2)
    gp = _gp(Z, Y, hyp)
    m, S = _inputs(_seed("gwidth-q", D, kind), Z, 3, kind)
    _check("width D=%d %s" % (D, kind), gp, Z, m, S, _seeds(_seed("gwidth-s", D), 3, 2, D))


# ------------------------------------------------------------------ size edges
@pytest.mark.parametrize("N", SIZES)
def test_every_size_edge(N):
    """one and two rows; either side of the i tile (64) and of the j tile (256); 300: a second j tile, five i tiles"""
    Z, Y, hyp = _problem(_seed("gsize", N), N, 3, 2)
    gp = _gp(Z, Y, hyp)
    for kind in ("full", "zero"):
        m, S = _inputs(_seed("gsize-q", N, kind), Z, 2, kind)
        _check("size N=%d %s" % (N, kind), gp, Z, m, S, _seeds(_seed("gsize-s", N, kind), 2, 2, 3))


# ------------------------------------------------------------------ outputs and seeds
@pytest.mark.parametrize("n_out", [1, 2, 3, 8])
def test_outputs_and_seeds(n_out):
    """each seed alone and all together; an unsymmetric cov_bar gives the bits of its symmetric part"""
    Z, Y, hyp = _problem(_seed("goutputs"), 40, 3, 8)
    gp = _gp(Z, Y, hyp, range(n_out))
    m, S = _inputs(_seed("goutputs-q"), Z, 3, "full")
    mb, cb, Vb = _seeds(_seed("goutputs-s", n_out), 3, n_out, 3)
    for tag, seeds in (("mu", (mb, None, None)), ("cov", (None, cb, None)), ("V", (None, None, Vb)), ("all", (mb, cb, Vb))):
        _check("outputs n_out=%d %s" % (n_out, tag), gp, Z, m, S, seeds)
    sym = 0.5 * (cb + np.transpose(cb, (0, 2, 1)))
    a, b = _run(gp, m, S, (None, cb, None)), _run(gp, m, S, (None, sym, None))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if n_out > 1:
        assert np.abs(cb - sym).max() > 0.1


# ------------------------------------------------------------------ the point limit against existing entry points
@pytest.mark.parametrize("N,D", [(150, 3), (90, 8)])
def test_point_limit_against_predict(N, D):
    """S = None.  Seeds on mu: m_bar = sum_a mu_bar_a d mu_a/dx; seeds on the diagonal of Cov: m_bar = sum_a c_aa d var_a/dx,
    both from predict_device_grad; S_bar there (not zero) against the reference"""
    from safe_exploration_amd import _buffers as B
    Z, Y, hyp = _problem(_seed("glimit", N), N, D, 2)
    gp = _gp(Z, Y, hyp)
    arrs = _model_arrays(gp, Z)
    T = 4
    m, _ = _inputs(_seed("glimit-q", N), Z, T, "zero")
    mb, cb, _ = _seeds(_seed("glimit-s", N), T, 2, D)
    cd = cb * np.eye(2)[None]
    _, _, jm, jv = (B.to_numpy(o) for o in gp.predict_device_grad(m))
    got = _check("limit N=%d mu seeds" % N, gp, Z, m, None, (mb, None, None))
    want = np.einsum("ta,tad->td", mb, jm)
    bar = G.bars(arrs[1], arrs[3], arrs[4], mb, None, None)
    print("limit N=%d: m_bar against d mu/dx %.2e (bar %.1e)" % (N, np.abs(got[0] - want).max(), bar.min()))
    assert np.all(np.abs(got[0] - want).max(axis=1) <= bar)
    got = _check("limit N=%d var seeds" % N, gp, Z, m, None, (None, cd, None))
    want = np.einsum("ta,tad->td", np.diagonal(cd, axis1=1, axis2=2), jv)
    bar = G.bars(arrs[1], arrs[3], arrs[4], None, cd, None)
    print("limit N=%d: m_bar against d var/dx %.2e (bar %.1e)" % (N, np.abs(got[0] - want).max(), bar.min()))
    assert np.all(np.abs(got[0] - want).max(axis=1) <= bar)
    assert np.abs(got[1]).max() > 1e-3                   # dCov/dS is not zero at a point
    off = np.zeros((T, 2, 2))
    off[:, 0, 1] = 1.0
    got = _check("limit N=%d cross seeds" % N, gp, Z, m, None, (None, off, None))
    assert np.abs(got[1]).max() > 1e-6                   # the forward writes an exact zero there, its derivative is not one


# ------------------------------------------------------------------ chunks, determinism, bounds
def test_chunks_determinism_and_bounds():
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    Z, Y, hyp = _problem(_seed("gcounts"), 90, 3, 2)
    gp = _gp(Z, Y, hyp)
    arrs = _model_arrays(gp, Z)
    hd = gp._handle
    kinv = gp.inv_K_device()
    T = 5
    m, S = _inputs(_seed("gcounts-q"), Z, T, "full")
    seeds = _seeds(_seed("gcounts-s"), T, 2, 3)
    tm, tS = B.as_dev(m, hd.device), B.as_dev(S, hd.device)
    ts = [B.as_dev(x, hd.device) for x in seeds]
    s = B.stream_ptr(hd.device)

    def call(T, sd, want_m=True, want_S=True):
        """through the C-ABI into sentinel-filled buffers with 2 queries of room in front and 3 behind"""
        mbar = torch.full((T + 5, 3), SENTINEL, dtype=torch.float64, device=hd.device)
        sbar = torch.full((T + 5, 3, 3), SENTINEL, dtype=torch.float64, device=hd.device)
        check(lib.sr_gp_moment_match_vjp(hd.h, B.ptr(tm), B.ptr(tS), T, B.ptr(kinv), B.ptr(sd[0]), B.ptr(sd[1]), B.ptr(sd[2]),
                                         B.ptr(mbar[2:]) if want_m else None, B.ptr(sbar[2:]) if want_S else None, s))
        outs = [B.to_numpy(mbar), B.to_numpy(sbar)]
        for o, want in zip(outs, (want_m, want_S)):
            assert np.all(o[:2] == SENTINEL) and np.all(o[2 + T:] == SENTINEL), "written outside T=%d" % T
            assert want or np.all(o == SENTINEL)
        return [o[2:2 + T] for o in outs]

    first = call(T, ts)
    _compare("T=5", first, G.vjp_batch(*arrs, m, S, *seeds), arrs, seeds)
    again = call(T, ts)
    assert all(np.array_equal(x, y) for x, y in zip(first, again)), "two calls differ"
    only_m, only_S = call(T, ts, want_S=False), call(T, ts, want_m=False)
    assert np.array_equal(only_m[0], first[0]) and np.array_equal(only_S[1], first[1])
    gp.set_chunk(2)
    chunked = call(T, ts)                                # three chunks: 2, 2, 1
    assert all(np.array_equal(x, y) for x, y in zip(first, chunked)), "chunking changed the bits"
    short = call(3, ts)
    assert all(np.array_equal(x, y[:3]) for x, y in zip(short, first))
    gp.set_chunk(65536)
    # NULL seeds are zero seeds, one at a time
    zeros = [torch.zeros_like(x) for x in ts]
    for k in range(3):
        with_null = call(T, [None if j == k else ts[j] for j in range(3)])
        with_zero = call(T, [zeros[j] if j == k else ts[j] for j in range(3)])
        assert all(np.array_equal(x, y) for x, y in zip(with_null, with_zero)), "NULL seed %d differs from zeros" % k
    none = call(T, [None, None, None])
    assert not none[0].any() and not none[1].any()
    # T == 0 is a no-op
    assert lib.sr_gp_moment_match_vjp(hd.h, None, None, 0, None, None, None, None, None, None, s) == 0


# ------------------------------------------------------------------ model states
def test_every_model_state():
    """the states of the forward's test: fitted, three in-place appends (alpha a slid view), a block append,
    release_scratch + refit, and after a removal"""
    N0, D = 600, 3
    Z, Y, hyp = _problem(_seed("gstates"), N0 + 43, D, 2)
    gp = _gp(Z[:N0], Y[:N0], hyp)
    gp.append_limit = 10 ** 9
    m, S = _inputs(_seed("gstates-q"), Z, 2, "full")
    seeds = _seeds(_seed("gstates-s"), 2, 2, D)
    n = N0
    _check("fitted", gp, Z[:n], m, S, seeds)
    for k in (1, 2, 3):
        gp.update_model(Z[n:n + 1], Y[n:n + 1], opt_hyp=False, replace_old=False)
        n += 1
        assert _slide(gp) == k
    _check("three in-place appends", gp, Z[:n], m, S, seeds)
    assert _slide(gp) == 3
    gp.update_model(Z[n:n + 40], Y[n:n + 40], opt_hyp=False, replace_old=False)
    n += 40
    _check("40-row append", gp, Z[:n], m, S, seeds)
    gp.release_scratch()
    gp.train(Z[:n], Y[:n], opt_hyp=False)
    _check("release_scratch + refit", gp, Z[:n], m, S, seeds)
    gp.remove_data([5])
    keep = np.delete(np.arange(n), 5)
    _check("after a removal", gp, Z[keep], m, S, seeds)


def test_sparse_model():
    """a do_sparse_gp model (32 inducing rows over N = 400): inv_k = P P^T, as the forward"""
    from safe_exploration_amd import SimpleGPModel
    X, Y, hyp = _problem(_seed("gsparse"), 400, 3, 2)
    gp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp)
    gp.do_sparse_gp = True
    gp.train(X, Y, 32, opt_hyp=False, Z=X[:32])
    assert gp.is_sparse
    m, S = _inputs(_seed("gsparse-q"), X, 3, "full")
    _check("sparse", gp, X[:32], m, S, _seeds(_seed("gsparse-s"), 3, 2, 3))


# ------------------------------------------------------------------ the autograd surface
def test_autograd_function():
    """differentiable=True: the same forward bits; backward = the direct call, bit for bit; no gradient for S = None"""
    import torch
    from safe_exploration_amd import _buffers as B
    Z, Y, hyp = _problem(_seed("gauto"), 70, 3, 2)
    gp = _gp(Z, Y, hyp)
    dev = gp._handle.device
    m, S = _inputs(_seed("gauto-q"), Z, 3, "full")
    seeds = [B.as_dev(x, dev) for x in _seeds(_seed("gauto-s"), 3, 2, 3)]
    plain = gp.moment_match_device(m, S)
    tm, tS = B.as_dev(m, dev).requires_grad_(True), B.as_dev(S, dev).requires_grad_(True)
    outs = gp.moment_match_device(tm, tS, differentiable=True)
    assert all(torch.equal(x, y) for x, y in zip(plain, outs)) and all(o.requires_grad for o in outs)
    L = sum((w * o).sum() for w, o in zip(seeds, outs))
    gm, gS = torch.autograd.grad(L, (tm, tS))
    dm, dS = gp.moment_match_vjp_device(m, S, *seeds)
    assert torch.equal(gm, dm) and torch.equal(gS, dS)
    # one output used only: the other seeds arrive as None
    outs = gp.moment_match_device(tm, tS, differentiable=True)
    gm, gS = torch.autograd.grad((seeds[1] * outs[1]).sum(), (tm, tS))
    dm, dS = gp.moment_match_vjp_device(m, S, None, seeds[1], None)
    assert torch.equal(gm, dm) and torch.equal(gS, dS)
    # S = None: a gradient for m alone
    tm2 = B.as_dev(m, dev).requires_grad_(True)
    outs = gp.moment_match_device(tm2, None, differentiable=True)
    assert all(torch.equal(x, y) for x, y in zip(gp.moment_match_device(m, None), outs))
    (gm,) = torch.autograd.grad(sum((w * o).sum() for w, o in zip(seeds, outs)), (tm2,))
    assert torch.equal(gm, gp.moment_match_vjp_device(m, None, *seeds)[0])
    # the NumPy form
    nm, nS = gp.predict_uncertain_vjp(m, S, *(B.to_numpy(x) for x in seeds))
    assert nm.shape == (3, 3) and nS.shape == (3, 3, 3)
    fm, fS = gp.moment_match_vjp_device(m, S, *seeds)
    assert np.array_equal(nm, B.to_numpy(fm)) and np.array_equal(nS, B.to_numpy(fS))


@pytest.mark.parametrize("with_sigma0", [False, True])
@pytest.mark.parametrize("tz_rows", [None, 1])
def test_propagated_gradient(with_sigma0, tz_rows):
    """moment_matching_batch(differentiable=True), T = 2, H = 3, n_s = 2, n_u = 1: the gradient of a fixed random linear
    functional of (mu_all, sigma_all) in mu_0, sigma_0, k_ff, k_fb against autograd through the CPU port of the propagation;
    the values are the bits of the plain call"""
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as up, _buffers as B
    n_s, n_u, H, T = 2, 1, 3, 2
    gp, arrs, a, b, rng = _prop_case(n_s, n_u, tz_rows)
    dev = gp._handle.device
    tz = None if tz_rows is None else np.eye(n_s)[1:]
    mu_0 = 0.3 * rng.standard_normal((T, n_s))
    k_ff, k_fb = 0.2 * rng.standard_normal((T, H, n_u)), 0.4 * rng.standard_normal((T, H - 1, n_u, n_s))
    Lc = 0.15 * rng.standard_normal((T, n_s, n_s))
    s0 = np.matmul(Lc, np.transpose(Lc, (0, 2, 1))) if with_sigma0 else None
    w_mu, w_sigma = rng.standard_normal((T, H, n_s)), rng.standard_normal((T, H, n_s, n_s))
    leaves = [None if x is None else B.as_dev(x, dev).requires_grad_(True) for x in (mu_0, s0, k_ff, k_fb)]
    outs = up.moment_matching_batch(leaves[0], gp, leaves[2], leaves[3], a, b, leaves[1], tz, differentiable=True)
    plain = up.moment_matching_batch(B.as_dev(mu_0, dev), gp, B.as_dev(k_ff, dev), B.as_dev(k_fb, dev), a, b,
                                     None if s0 is None else B.as_dev(s0, dev), tz)
    assert all(torch.equal(x, y) for x, y in zip(outs, plain))
    L = (B.as_dev(w_mu, dev) * outs[0]).sum() + (B.as_dev(w_sigma, dev) * outs[1]).sum()
    used = [x for x in leaves if x is not None]
    grads = iter(torch.autograd.grad(L, used))
    got = [None if x is None else B.to_numpy(next(grads)) for x in leaves]
    for t in range(T):
        ref = G.propagate_grad(arrs, mu_0[t], k_ff[t], k_fb[t], a, b, None if s0 is None else s0[t], tz, w_mu[t], w_sigma[t])
        for name, g, r in zip(("mu_0", "sigma_0", "k_ff", "k_fb"), got, ref):
            if r is None:
                continue
            err, scale = np.abs(g[t] - r).max(), np.abs(r).max()
            print("propagated sigma0=%s tz=%s t=%d d/d%s: %.2e of %.2e (rtol %.1e)" % (with_sigma0, tz_rows, t, name, err, scale,
                                                                                    PROP_RTOL))
            assert err <= PROP_RTOL * scale, name


# ------------------------------------------------------------------ refusals
def test_refusals():
    """host-side refusals only: none of these launches anything, and the outputs stay as they were"""
    import torch
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    s = B.stream_ptr(dev)
    Z, Y, hyp = _problem(_seed("grefuse"), 50, 3, 1)
    buf = B.empty((64,), dev).fill_(SENTINEL)
    p = B.ptr(buf)
    gen = SimpleGPModel(1, 2, 1, kern_types=["mat52"], hyp=[{"lengthscale": np.ones(3), "variance": 1.0,
                                                             "noise_variance": 0.01}])
    gen.train(Z, Y, opt_hyp=False)
    with pytest.raises(NotImplementedError):
        gen.moment_match_vjp_device(Z[:2], None, np.ones((2, 1)))
    with pytest.raises(NotImplementedError):
        gen.moment_match_device(Z[:2], None, differentiable=True)
    assert gen._inv_K_dev is None
    assert lib.sr_gp_moment_match_vjp(gen._handle.h, p, None, 1, p, p, p, p, p, p, s) == _lib.SR_EUNSUPPORTED
    assert "ARD-RBF" in _lib.last_error()
    raw = _Handle(dev, 50, 3, 1)
    assert lib.sr_gp_moment_match_vjp(raw.h, p, None, 1, p, p, p, p, p, p, s) == _lib.SR_ESTATE
    assert "not factorized" in _lib.last_error()
    with pytest.raises(RuntimeError):
        SimpleGPModel(1, 2, 1).moment_match_vjp_device(Z[:2], None)
    gp = _gp(Z, Y, hyp)
    h = gp._handle.h
    for args in ((None, None, 1, p, p, p, p, p, p), (p, None, 1, None, p, p, p, p, p), (p, None, 1, p, p, p, p, None, None),
                 (p, None, -1, p, p, p, p, p, p)):
        assert lib.sr_gp_moment_match_vjp(h, *(args + (s,))) == _lib.SR_EINVAL, args
    assert lib.sr_gp_moment_match_vjp(None, p, None, 1, p, p, p, p, p, p, s) == _lib.SR_EINVAL
    with pytest.raises(ValueError):
        gp.moment_match_vjp_device(Z[:2, :2], None)
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
