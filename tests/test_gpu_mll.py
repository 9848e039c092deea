"""sr_gp_mll (objective and gradient of train(opt_hyp=True)) at every compiled width, every size edge, several outputs
on a handle, the whole packed kernel family, and every state a model can be in -- each against an fp64 CPU reference.

References: oracle.gp_nll_grad (closed forms per kernel name) for the four named kernels, tests/_mll_ref.py (autograd
through the Cholesky factor) for the packed family k = (c0 + sum a x y) v kappa(r) + sum b x y; the two agree to 1.3e-13
of max|gradient| on the CPU (tests/test_mll_host.py).

Tolerances, those of test_gpu_parity.py::test_marginal_likelihood_and_gradient: nll 1e-9 |ref|; gradient rtol 1e-7,
atol 1e-8 max|ref| (element-wise relative error is not usable: the smallest entry of a lin_* gradient is 1e-5 .. 1e-7 of
the largest).  inv_k: atol 1e-9 max|ref| (the variance tolerance of SURVEY 8d: the same product).

What the kernels leave unrun at the one shape of that test (N = 150, D = 3, one output): three of the four instantiations
of sr_mll_grad_kernel<DT> and every D < DT (the compaction from DT-strided accumulators to the D-strided result), the
second trip of the strided block reduction (more than 256 blocks: N >= 257), the strides of the loop over outputs, most
of the gradient vector (c0, a_j, s_j for j != 1), and the views a model's buffers become after in-place appends."""
import ctypes
import zlib

import numpy as np
import pytest

import _mll_ref as R
from _helpers import hip_model, width_problem
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

KERNELS = ("rbf", "mat52", "lin_rbf", "lin_mat52")
WIDTHS = tuple(range(2, 13))                     # D = n_s_in + n_u of the constructor; D = 1: the C-ABI cases below
SIZES = (1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300, 1000, 2100)
GENERAL_WIDTHS = (1, 2, 5, 8, 12)
SENTINEL = -7.25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


def _check_mll(tag, nll, g, rnll, rg):
    """prints the figures, then asserts the tolerances of the module docstring"""
    g, rg = np.asarray(g), np.asarray(rg)
    scale = np.abs(rg).max()
    print("mll %s: nll rel %.2e, grad max-abs / max|ref| %.2e" % (tag, abs(nll - rnll) / abs(rnll),
                                                                  np.abs(g - rg).max() / scale))
    assert g.shape == rg.shape and np.all(np.isfinite(g))
    assert abs(nll - rnll) <= 1e-9 * abs(rnll), (tag, nll, rnll)
    np.testing.assert_allclose(g, rg, rtol=1e-7, atol=1e-8 * scale, err_msg=tag)


# ------------------------------------------------------------------ through SimpleGPModel: widths and sizes
def _python_model(kt, D, N, tag):
    from safe_exploration_amd import SimpleGPModel
    prob = width_problem(_seed(tag, kt, D, N), kt, D, N, 1)
    n_in = min(8, D - 1)
    gp = SimpleGPModel(1, n_in, D - n_in, kern_types=[kt])              # nothing fixed: every hyper-parameter is free
    gp.hyp[0] = {k: (np.array(v, dtype=float) if np.ndim(v) else float(v)) for k, v in prob["hyp"][0].items()}
    gp._noise[0] = 0.03
    return gp, prob


def _oracle_free(gp, prob, kt):
    rnll, rg = orc.gp_nll_grad(prob["Z"], prob["Y"][:, 0], kt, prob["hyp"][0], gp._noise[0])
    return rnll, np.concatenate([np.reshape(rg[k], (-1,)) for k, _ in gp._free_hyp(0)])


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("kt", KERNELS)
def test_every_width(kt, D):
    """N = 150, every D from 2 to 12: sr_mll_grad_kernel<3> at D = 2, 3; <5> at 4, 5; <8> at 6, 7, 8; <12> at 9 .. 12 --
    every instantiation with D < DT and with D == DT.
    Observed on MI355X, for information (gradient max-abs / max|ref|, worst of the four kernels per width; the bar is 1e-8):
      D     2        3        4        5        6        7        8        9        10       11       12
            1.3e-13  2.2e-15  2.4e-14  1.3e-13  9.7e-14  1.3e-13  2.8e-14  7.8e-15  2.9e-13  5.0e-14  3.0e-14
    (nll: at most 1.0e-13 relative.)  The lin_* kernels set the worst cases, as they do between the two CPU references."""
    gp, prob = _python_model(kt, D, 150, "width")
    nll, g = gp.neg_log_marginal_likelihood(prob["Z"], prob["Y"], 0)
    rnll, rg = _oracle_free(gp, prob, kt)
    assert np.abs(rg).min() > 0                                          # no entry of the reference is a structural zero
    _check_mll("width %s D=%d" % (kt, D), nll, g, rnll, rg)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kt,D", [("rbf", 3), ("rbf", 7), ("lin_mat52", 3), ("lin_mat52", 7)])
def test_every_size_edge(kt, D, N):
    """One point; either side of the 16 x 16 pair tile; N a multiple of the 128-row padding (no front padding) and either
    side; 257: the first size with more than 256 partial blocks (17 x 17: the second trip of the strided reduction);
    2100: the factor comes from the panelled update.  At N = 2100 also with panels of 2 blocks and with the three-stream
    pipeline asked for on the handle the objective uses (the library's queue check decides whether that one runs pipelined;
    which it was is printed, the numbers must not care; on MI355X with four hardware queues it did run pipelined).
    Observed worst over all sizes: nll 7.7e-13 relative, gradient 2.4e-12 of max|ref|."""
    import torch
    from safe_exploration_amd._lib import lib, check
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    gp, prob = _python_model(kt, D, N, "size")
    rnll, rg = _oracle_free(gp, prob, kt)
    nll, g = gp.neg_log_marginal_likelihood(prob["Z"], prob["Y"], 0)
    _check_mll("size %s D=%d N=%d" % (kt, D, N), nll, g, rnll, rg)
    if N == 2100:
        for what, setter, arg in (("panel=2", lib.sr_gp_set_fact_panel, 2), ("pipeline=1", lib.sr_gp_set_fact_pipeline, 1)):
            hd = gp._mll_handle = _Handle(torch.device("cuda", 0), N, D, 1)      # the objective reuses a handle of this shape
            check(setter(hd.h, arg))
            nll, g = gp.neg_log_marginal_likelihood(prob["Z"], prob["Y"], 0)
            assert gp._mll_handle is hd
            print("size %s D=%d N=%d %s: ran pipelined = %d" % (kt, D, N, what, lib.sr_gp_fact_pipelined(hd.h)))
            _check_mll("size %s D=%d N=%d %s" % (kt, D, N, what), nll, g, rnll, rg)


# ------------------------------------------------------------------ through the C-ABI
class _Abi(object):
    """sr_gp_create / sr_gp_set_data_general / sr_gp_factorize / sr_gp_mll on one handle of n_out outputs"""

    def __init__(self, Z, Y, kp, noise):
        import torch
        from safe_exploration_amd import _buffers as B
        from safe_exploration_amd._lib import lib, check
        from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
        self.B, self.lib, self.check = B, lib, check
        self.dev = torch.device("cuda", 0)
        Z, Y, kp = np.atleast_2d(Z), np.asarray(Y, dtype=np.float64), np.atleast_2d(kp)
        self.N, self.D = Z.shape
        self.n_out = Y.shape[1]
        assert kp.shape == (self.n_out, 3 + 3 * self.D)
        self.hd = _Handle(self.dev, self.N, self.D, self.n_out)
        self.s = B.stream_ptr(self.dev)
        self.set_data(Z, Y, kp, noise)

    def set_data(self, Z, Y, kp, noise):
        B = self.B
        self.keep = [B.as_dev(np.ascontiguousarray(a, dtype=np.float64), self.dev)
                     for a in (Z, Y, kp, np.reshape(noise, (-1,)))]
        tz, ty, tk, tn = self.keep
        self.check(self.lib.sr_gp_set_data_general(self.hd.h, B.ptr(tz), B.ptr(ty), B.ptr(tk), B.ptr(tn), self.s))

    def factorize(self):
        info = (ctypes.c_int * self.n_out)()
        return self.lib.sr_gp_factorize(self.hd.h, self.s, info)

    def mll(self, extra=(4, 8)):
        """-> nll (n_out,), grad (n_out, 3 + 3 D); the buffers are longer than that and hold a sentinel: nothing beyond
        n_out and n_out (3 + 3 D) doubles may be written"""
        import torch
        B, ng = self.B, 3 + 3 * self.D
        nll = torch.full((self.n_out + extra[0],), SENTINEL, dtype=torch.float64, device=self.dev)
        g = torch.full((self.n_out * ng + extra[1],), SENTINEL, dtype=torch.float64, device=self.dev)
        self.check(self.lib.sr_gp_mll(self.hd.h, B.ptr(nll), B.ptr(g), self.s))
        nll, g = B.to_numpy(nll), B.to_numpy(g)
        assert np.all(nll[self.n_out:] == SENTINEL) and np.all(g[self.n_out * ng:] == SENTINEL)
        assert not np.any(nll[:self.n_out] == SENTINEL) and not np.any(g[:self.n_out * ng] == SENTINEL)
        return nll[:self.n_out].copy(), g[:self.n_out * ng].reshape(self.n_out, ng).copy()


def _assert_well_conditioned(case):
    """cond(K_y) < 1e8, computed here: a failing comparison cannot be blamed on the inputs"""
    Ky = R.ky_general(**{k: case[k] for k in ("Z", "kind", "v", "c0", "s", "a", "b", "noise")})
    cond = np.linalg.cond(Ky)
    assert cond < 1e8, cond
    return cond


@pytest.mark.parametrize("N", [150, 300])
@pytest.mark.parametrize("D", GENERAL_WIDTHS)
@pytest.mark.parametrize("kind", ["rbf", "mat52"])
def test_general_family_whole_gradient_vector(kind, D, N):
    """c0, every s_j, a_j, b_j positive (what GPy's all-input linear kernels pack to: DESIGN.md 7): all 3 + 3 D entries
    against autograd, d/dc0, d/da_j and d/ds_j (j != 1) among them -- none of these is reachable through SimpleGPModel."""
    case = R.general_case(_seed("general", kind, D, N), N, D, kind)
    cond = _assert_well_conditioned(case)
    rnll, rg = R.nll_general(**case)
    assert np.abs(rg).min() > 0
    m = _Abi(case["Z"], case["y"][:, None], R.case_kp(case), case["noise"])
    assert m.factorize() == 0
    nll, g = m.mll()
    print("general %s D=%d N=%d: cond(K_y) = %.1e" % (kind, D, N, cond))
    _check_mll("general %s D=%d N=%d" % (kind, D, N), nll[0], g[0], rnll, rg)


def _multi_output_cases(n_out, N, D):
    Z = np.random.default_rng(_seed("multi", n_out, N, D)).uniform(-1, 1, (N, D))
    cases = []
    for d in range(n_out):
        c = R.general_case(_seed("multi", n_out, d), N, D, ("rbf", "mat52")[d % 2], noise=0.03 + 0.01 * d)
        rng = np.random.default_rng(_seed("multi-y", n_out, d))
        c["Z"] = Z                                                        # one set of inputs, targets of its own per output
        c["y"] = np.sin(2.0 * Z.dot(rng.standard_normal(D) / np.sqrt(D))) + 0.05 * rng.standard_normal(N)
        cases.append(c)
    return Z, cases


@pytest.mark.parametrize("n_out,N,D", [(2, 150, 4), (3, 300, 3), (9, 200, 7)])
def test_several_outputs_on_one_handle(n_out, N, D):
    """One sr_gp_mll call on a handle of 2, 3 and 9 outputs (9: more than the 8 factorisation slots), a different kappa and
    different parameters per output: the strides alpha + d Np, kp + d (3 + 3 D), grad + d (3 + 3 D), logdet + d.  Every
    output against the reference, and bit for bit what a one-output handle returns for that output alone."""
    Z, cases = _multi_output_cases(n_out, N, D)
    for c in cases:
        _assert_well_conditioned(c)
    m = _Abi(Z, np.stack([c["y"] for c in cases], axis=1), np.stack([R.case_kp(c) for c in cases]),
             np.array([c["noise"] for c in cases]))
    assert m.factorize() == 0
    nll, g = m.mll()
    for d, c in enumerate(cases):
        rnll, rg = R.nll_general(**c)
        _check_mll("n_out=%d output %d" % (n_out, d), nll[d], g[d], rnll, rg)
    for d, c in enumerate(cases):
        one = _Abi(Z, c["y"][:, None], R.case_kp(c), c["noise"])
        assert one.factorize() == 0
        n1, g1 = one.mll()
        assert n1[0] == nll[d], (d, n1[0], nll[d])
        np.testing.assert_array_equal(g1[0], g[d])


# ------------------------------------------------------------------ model states
def _slide(gp):
    from safe_exploration_amd._lib import lib
    k = ctypes.c_int(-1)
    assert lib.sr_gp_slide_steps(gp._handle.h, ctypes.byref(k)) == 0
    return k.value


def _check_state(gp, Z, Y, tag):
    """sr_gp_mll, sr_gp_logdet and sr_gp_inv_k of the model's own handle against the reference on the rows it holds now"""
    import scipy.linalg as sla
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    n_out, D, N = hd.n_out, hd.D, Z.shape[0]
    assert hd.N == N
    s = B.stream_ptr(hd.device)
    nll, g, ld = B.empty((n_out,), hd.device), B.empty((n_out, 3 + 3 * D), hd.device), B.empty((n_out,), hd.device)
    check(lib.sr_gp_mll(hd.h, B.ptr(nll), B.ptr(g), s))
    check(lib.sr_gp_logdet(hd.h, B.ptr(ld), s))
    nll, g, ld = B.to_numpy(nll), B.to_numpy(g), B.to_numpy(ld)
    gp._inv_K = None
    inv = gp.inv_K
    kp = gp._pack_kernel_params()
    for d in range(n_out):
        noise = gp._noise[d] + 1e-5 + 1e-8               # sigma_n^2 + noise_diag + GPy's jitter: what _fit hands over
        rnll, rg = R.nll_packed(Z, Y[:, d], kp[d], noise)
        _check_mll("%s output %d" % (tag, d), nll[d], g[d], rnll, rg)
        c = sla.cho_factor(R.ky_packed(Z, kp[d], noise), lower=True)
        rld = 2.0 * np.sum(np.log(np.diag(c[0])))
        rinv = sla.cho_solve(c, np.eye(N))
        print("state %s output %d: logdet rel %.2e, inv_k max-abs / max|ref| %.2e" % (
            tag, d, abs(ld[d] - rld) / max(abs(rld), 1.0), np.abs(inv[d] - rinv).max() / np.abs(rinv).max()))
        assert abs(ld[d] - rld) <= 1e-9 * max(abs(rld), 1.0)
        assert inv[d].shape == (N, N)
        np.testing.assert_allclose(inv[d], rinv, rtol=0, atol=1e-9 * np.abs(rinv).max())


@pytest.mark.parametrize("N0", [120, 250, 600])
def test_read_outs_in_every_model_state(N0):
    """sr_gp_mll and sr_gp_inv_k read U^-1, alpha and the targets where the handle says they are, without going back to
    plain buffers first; after in-place one-point appends those are views `slide` steps into their allocations.  One handle
    with packed parameters (an rbf and a lin_mat52 output) through: the fit; one, two and three one-point appends; three
    rows at once; 40 rows at once; release_scratch and a refit.  After each, the three read-outs against the reference on
    the rows the model holds, and a prediction at the end.
    The in-place route exists beyond 512 padded rows only (sr_capi_append.hip, append1_route): N0 = 600 takes it, and
    sr_gp_slide_steps must say 1, 2, 3 (odd and even); N0 = 120 and 250 grow through the one-launch append of small models
    into the handle's second set of buffers (slide stays 0) and cross a padded size on the way."""
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(N0)
    ntot, D = N0 + 50, 3
    Z = rng.uniform(-1, 1, (ntot, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, 2)))) + 0.05 * rng.standard_normal((ntot, 2))
    kts = ["rbf", "lin_mat52"]
    hyp = [dict(orc.make_hyp(kt, rng, D), noise_variance=nv) for kt, nv in zip(kts, (0.03, 0.05))]
    gp = SimpleGPModel(2, 2, 1, kern_types=kts, hyp=hyp)
    gp.train(Z[:N0], Y[:N0], opt_hyp=False)
    gp.append_limit = 10 ** 9
    in_place = N0 > 512
    n = N0
    assert _slide(gp) == 0
    _check_state(gp, Z[:n], Y[:n], "N0=%d fitted" % N0)
    for k in (1, 2, 3):
        gp.update_model(Z[n:n + 1], Y[n:n + 1], opt_hyp=False, replace_old=False)
        n += 1
        assert _slide(gp) == (k if in_place else 0)
        _check_state(gp, Z[:n], Y[:n], "N0=%d +1 (slide %d)" % (N0, _slide(gp)))
    for m in (3, 40):
        gp.update_model(Z[n:n + m], Y[n:n + m], opt_hyp=False, replace_old=False)
        n += m
        assert _slide(gp) == 0 and gp._handle.N == n
        _check_state(gp, Z[:n], Y[:n], "N0=%d +%d rows" % (N0, m))
    gp.release_scratch()
    gp.train(Z[:n], Y[:n], opt_hyp=False)
    _check_state(gp, Z[:n], Y[:n], "N0=%d refit" % N0)
    # the read-outs left the model as it was
    xq = rng.uniform(-1, 1, (64, D))
    beta, inv_K = orc.gp_fit_k(Z[:n], Y[:n], kts, hyp, np.array([0.03, 0.05]) + 1e-5)
    rmu, rvar = orc.gp_predict_k(xq, Z[:n], beta, inv_K, kts, hyp)
    mu, var = gp.predict(xq)
    np.testing.assert_allclose(mu, rmu, rtol=0, atol=1e-11 * np.abs(beta).sum(0).max())
    np.testing.assert_allclose(var, rvar, rtol=0, atol=1e-8)


def test_read_outs_on_a_slid_model_leave_the_views_intact():
    """Between in-place appends: mll and inv_k on the views, then the next in-place append and a prediction on the grown
    model must match a model fitted on the same rows from scratch."""
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(99)
    N0, D = 600, 3
    Z = rng.uniform(-1, 1, (N0 + 4, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, 2)))) + 0.05 * rng.standard_normal((N0 + 4, 2))
    kts = ["mat52", "lin_rbf"]
    hyp = [dict(orc.make_hyp(kt, rng, D), noise_variance=0.04) for kt in kts]
    gp = SimpleGPModel(2, 2, 1, kern_types=kts, hyp=hyp)
    gp.train(Z[:N0], Y[:N0], opt_hyp=False)
    gp.append_limit = 10 ** 9
    for i in range(N0, N0 + 4):
        gp.update_model(Z[i:i + 1], Y[i:i + 1], opt_hyp=False, replace_old=False)
        assert _slide(gp) == i + 1 - N0
        _check_state(gp, Z[:i + 1], Y[:i + 1], "between appends, slide %d" % _slide(gp))
    xq = rng.uniform(-1, 1, (16, D))
    beta, inv_K = orc.gp_fit_k(Z, Y, kts, hyp, np.full(2, 0.04 + 1e-5))
    rmu, rvar = orc.gp_predict_k(xq, Z, beta, inv_K, kts, hyp)
    mu, var = gp.predict(xq)
    np.testing.assert_allclose(mu, rmu, rtol=0, atol=1e-11 * np.abs(beta).sum(0).max())
    np.testing.assert_allclose(var, rvar, rtol=0, atol=1e-8)


# ------------------------------------------------------------------ refusals
def test_refusals_name_their_reason():
    """Host-side refusals only: nothing here reaches a kernel with bad arguments."""
    import torch
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    s = B.stream_ptr(dev)
    rng = np.random.default_rng(3)
    nll, g = B.empty((2,), dev).fill_(SENTINEL), B.empty((2, 12), dev).fill_(SENTINEL)
    # a sparse model
    X = rng.uniform(-1, 1, (400, 3))
    Yx = np.sin(X.dot(rng.standard_normal((3, 2))))
    sp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=[{"lengthscale": np.ones(3), "variance": 1.0,
                                                              "noise_variance": 0.01}] * 2)
    sp.do_sparse_gp = True
    sp.train(X, Yx, 40, opt_hyp=False, Z=X[:40])
    assert sp.is_sparse
    assert lib.sr_gp_mll(sp._handle.h, B.ptr(nll), B.ptr(g), s) == _lib.SR_ESTATE
    assert "sr_gp_mll" in _lib.last_error() and "sparse" in _lib.last_error()
    # a handle with data and no factor
    case = R.general_case(1, 100, 3, "rbf")
    m = _Abi(case["Z"], case["y"][:, None], R.case_kp(case), case["noise"])
    assert lib.sr_gp_mll(m.hd.h, B.ptr(nll), B.ptr(g), s) == _lib.SR_ESTATE
    assert "sr_gp_mll" in _lib.last_error() and "not factorized" in _lib.last_error()
    # a factorised model set through sr_gp_set_data (lengthscales / variances, not the packed parameters)
    plain = hip_model(X[:100], Yx[:100], np.ones((2, 3)), np.ones(2), np.full(2, 0.01), 2, 1)
    assert lib.sr_gp_mll(plain._handle.h, B.ptr(nll), B.ptr(g), s) == _lib.SR_ESTATE
    assert "sr_gp_set_data_general" in _lib.last_error()
    # NULL results on a good model
    assert m.factorize() == 0
    for a, b in ((None, B.ptr(g)), (B.ptr(nll), None), (None, None)):
        assert lib.sr_gp_mll(m.hd.h, a, b, s) == _lib.SR_EINVAL
        assert "NULL" in _lib.last_error()
    assert lib.sr_gp_mll(None, B.ptr(nll), B.ptr(g), s) == _lib.SR_EINVAL
    torch.cuda.synchronize()
    assert np.all(B.to_numpy(nll) == SENTINEL) and np.all(B.to_numpy(g) == SENTINEL)       # no refusal wrote anything
    # and the good model answers
    n1, g1 = m.mll()
    rnll, rg = R.nll_general(**case)
    _check_mll("after refusals", n1[0], g1[0], rnll, rg)


@pytest.mark.parametrize("kt", ["rbf", "lin_mat52"])
def test_matrix_that_is_not_positive_definite(kt):
    """A NaN among the training inputs: the fp64 Cholesky of that K_y has no positive pivot in row 71 on the CPU either
    (numpy.linalg.cholesky raises or, with LAPACK builds that do not test their pivots for NaN, hands back a factor that is
    not finite; the reference raises), the library reports it through its own status word (no fault),
    neg_log_marginal_likelihood answers (inf, None) -- and the same handle gives the right numbers next."""
    gp, prob = _python_model(kt, 3, 200, "notpd")
    bad = prob["Z"].copy()
    bad[70, 1] = np.nan
    kp = R.pack_named(kt, prob["hyp"][0], 3)
    try:
        rejected = not np.all(np.isfinite(np.linalg.cholesky(R.ky_packed(bad, kp, gp._noise[0] + 1e-8))))
    except np.linalg.LinAlgError:
        rejected = True
    assert rejected
    with pytest.raises(np.linalg.LinAlgError):
        R.nll_packed(bad, prob["Y"][:, 0], kp, gp._noise[0] + 1e-8)
    assert gp.neg_log_marginal_likelihood(bad, prob["Y"], 0) == (np.inf, None)
    hd = gp._mll_handle
    nll, g = gp.neg_log_marginal_likelihood(prob["Z"], prob["Y"], 0)
    assert gp._mll_handle is hd
    rnll, rg = _oracle_free(gp, prob, kt)
    _check_mll("after a matrix that is not positive definite, %s" % kt, nll, g, rnll, rg)


# ------------------------------------------------------------------ the optimiser
def _opt_problem(kt, D, N=200):
    """targets drawn from a GP of the kernel itself: the likelihood has a well-defined interior optimum"""
    rng = np.random.default_rng(_seed("opt", kt, D))
    Z = rng.uniform(-2, 2, (N, D))
    true = orc.make_hyp(kt, rng, D)
    K = orc.kernel_matrix(kt, true, Z, Z) + 0.01 * np.eye(N)
    y = np.linalg.cholesky(K).dot(rng.standard_normal(N))
    return Z, y


def _cpu_optimum(kt, D, Z, y, objective):
    """scipy's L-BFGS-B over the logarithms of the free parameters, as optimize_hyperparameters runs it, on a CPU objective
    ("oracle": orc.gp_nll_grad, "autograd": _mll_ref).  A SimpleGPModel carries the parameters (no device call is made)."""
    from scipy import optimize
    from safe_exploration_amd import SimpleGPModel
    n_in = min(8, D - 1)
    gp = SimpleGPModel(1, n_in, D - n_in, kern_types=[kt])
    free = gp._free_hyp(0)

    def fun(phi):
        th = np.exp(np.clip(phi, -25.0, 25.0))
        gp._set_free(0, th)
        try:
            if objective == "oracle":
                nll, grad = orc.gp_nll_grad(Z, y, kt, gp.hyp[0], gp._noise[0])
            else:
                nll, g = R.nll_packed(Z, y, gp._pack_kernel_params(only=0)[0], gp._noise[0] + 1e-8)
                grad = R.named_gradient(kt, gp.hyp[0], g, D)
        except np.linalg.LinAlgError:
            return 1e25, np.zeros_like(phi)
        return nll, np.concatenate([np.reshape(grad[k], (-1,)) for k, _ in free]) * th

    res = optimize.minimize(fun, np.log(gp._get_free(0)), jac=True, method="L-BFGS-B", options={"maxiter": 1000})
    gp._set_free(0, np.exp(np.clip(res.x, -25.0, 25.0)))
    return orc.gp_nll_grad(Z, y, kt, gp.hyp[0], gp._noise[0])[0], gp, res


# |nll(optimum of the oracle objective) - nll(optimum of the autograd objective)| / |nll|: both on the CPU, the same start,
# both optima evaluated by the oracle (the two objectives agree to 1.3e-13: tests/test_mll_host.py).  Measured:
#   rbf     D = 5 : 1.6e-16  (176.63991725604757 against ...754; 16 iterations, 18 evaluations each)
#   lin_rbf D = 4 : 1.9e-13  (-124.96629298473462 against ...71120; 39 iterations, 46 evaluations each)
# The spread of the method is the larger of the two; the bound is ten times that.
# Observed on MI355X (device optimum against oracle optimum): rbf D = 5 3.2e-16, lin_rbf D = 4 2.3e-13.
OPT_SPREAD = 1.9e-13
OPT_BOUND = 10.0 * OPT_SPREAD


@pytest.mark.parametrize("kt,D", [("rbf", 5), ("lin_rbf", 4)])
def test_optimiser_reaches_the_optimum_of_the_cpu_objective(kt, D):
    """D = 5 runs sr_mll_grad_kernel<5> with D == DT, lin_rbf at D = 4 with D < DT.  The same L-BFGS-B from the same start
    over the same logarithms, once on the device objective (optimize_hyperparameters), once on the oracle's: two runs on
    objectives that differ in the last bits may stop an iteration apart, so the bound on the difference of the two optima's
    nll is ten times the spread measured between the two CPU references used as objectives (OPT_BOUND above)."""
    from safe_exploration_amd import SimpleGPModel
    Z, y = _opt_problem(kt, D)
    ref_nll, ref_gp, ref_res = _cpu_optimum(kt, D, Z, y, "oracle")
    n_in = min(8, D - 1)
    gp = SimpleGPModel(1, n_in, D - n_in, kern_types=[kt])
    start = gp.neg_log_marginal_likelihood(Z, y[:, None], 0, with_grad=False)[0]
    gp.optimize_hyperparameters(Z, y[:, None])
    dev_nll = orc.gp_nll_grad(Z, y, kt, gp.hyp[0], gp._noise[0])[0]
    own, g = gp.neg_log_marginal_likelihood(Z, y[:, None], 0)
    print("optimiser %s D=%d: start %.6f, device optimum %.12f, oracle optimum %.12f, relative difference %.2e" % (
        kt, D, start, dev_nll, ref_nll, abs(dev_nll - ref_nll) / abs(ref_nll)))
    assert abs(own - dev_nll) <= 1e-9 * abs(dev_nll)                      # the device's value at its own optimum
    assert dev_nll < start - 10
    assert np.abs(g * gp._get_free(0)).max() < 1e-2                       # stationary in log-parameters (as the rbf test)
    assert abs(dev_nll - ref_nll) <= OPT_BOUND * abs(ref_nll)
