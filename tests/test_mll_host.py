"""CPU checks behind tests/test_gpu_mll.py: the autograd reference of the packed kernel family (tests/_mll_ref.py)
against the oracle's hand-written closed forms and against central differences, and the Python mapping from the vector
sr_gp_mll returns to the named hyper-parameters (library calls monkeypatched).  No GPU."""
import numpy as np
import pytest

import _mll_ref as R
from oracle import oracle_np as orc

KERNELS = ("rbf", "mat52", "lin_rbf", "lin_mat52")
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 12)


def _named_problem(kt, D, N, seed):
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (N, D))
    y = np.sin(2.0 * Z.dot(rng.standard_normal(D) / np.sqrt(D))) + 0.05 * rng.standard_normal(N)
    hyp = orc.make_hyp(kt, rng, D)
    if kt in ("rbf", "mat52"):
        hyp["lengthscale"] = hyp["lengthscale"] * np.sqrt(max(D, 3) / 3.0)
    return Z, y, hyp


# lin_* act with their product part on input dimension 1: they need D >= 2
NAMED_CASES = [(kt, D) for D in WIDTHS for kt in KERNELS if D >= 2 or not kt.startswith("lin_")]


@pytest.mark.parametrize("kt,D", NAMED_CASES)
def test_autograd_reference_equals_the_oracle_closed_forms(kt, D):
    """Two references with nothing in common but the formula of nll: agreement to 1e-11 of max|ref| (nll: relative).
    Measured worst case over this grid and the two larger shapes below: nll 8.4e-14, gradient 1.3e-13; the bar of the device
    comparison (rtol 1e-7, atol 1e-8 max|ref|) is five orders of magnitude above that."""
    _compare_with_oracle(kt, D, 150, 1000 + D)


@pytest.mark.parametrize("kt", KERNELS)
@pytest.mark.parametrize("N,D", [(129, 12), (700, 7)])
def test_autograd_reference_equals_the_oracle_at_larger_shapes(kt, N, D):
    _compare_with_oracle(kt, D, N, 2000 + N)


def _compare_with_oracle(kt, D, N, seed):
    Z, y, hyp = _named_problem(kt, D, N, seed)
    noise = 0.03
    rnll, rg = orc.gp_nll_grad(Z, y, kt, hyp, noise)
    nll, g = R.nll_packed(Z, y, R.pack_named(kt, hyp, D), noise + orc.GPY_JITTER)
    named = R.named_gradient(kt, hyp, g, D)
    assert set(named) == set(rg)
    ref = np.concatenate([np.reshape(rg[k], (-1,)) for k in sorted(rg)])
    got = np.concatenate([np.reshape(named[k], (-1,)) for k in sorted(rg)])
    err_nll, err_g = abs(nll - rnll) / abs(rnll), np.abs(got - ref).max() / np.abs(ref).max()
    print("ref-vs-oracle %s D=%d N=%d: nll %.2e grad %.2e" % (kt, D, N, err_nll, err_g))
    assert err_nll < 1e-11 and err_g < 1e-11
    # the entries of the API vector no named kernel uses are exact zeros of the named gradient's complement only where the
    # parameter itself multiplies nothing: d/db of rbf / mat52 is NOT zero (b = 0 is a point of the family, not a wall)
    if kt in ("rbf", "mat52"):
        assert np.abs(g[2 + 2 * D:2 + 3 * D]).max() > 0


@pytest.mark.parametrize("kind", ["rbf", "mat52"])
def test_autograd_reference_equals_central_differences_on_a_general_member(kind):
    """c0 != 0, every a_j, b_j, s_j != 0: the part of the family the oracle cannot express.  Central differences with a
    relative step h = 1e-5: truncation ~ h^2 |f'''| / 6 and rounding ~ eps |nll| / h give ~1e-9 relative to the largest
    entry here; asserted at 1e-6 of max|g| (and every entry must be resolved: max|g| / min|g| is printed)."""
    c = R.general_case(5 + R.KINDS[kind], 60, 4, kind)
    names = ("v", "c0", "s", "a", "b", "noise")
    nll, g = R.nll_general(**c)
    assert g.shape == (3 + 3 * 4,)
    fd, pos = np.empty_like(g), 0
    for name in names:
        base = np.array(c[name], dtype=np.float64).reshape(-1)
        for j in range(base.size):
            vals = []
            for sign in (1.0, -1.0):
                p = base.copy()
                p[j] *= 1.0 + sign * 1e-5
                cc = dict(c)
                cc[name] = p if base.size > 1 else float(p[0])
                vals.append(R.nll_general(with_grad=False, **cc)[0])
            fd[pos] = (vals[0] - vals[1]) / (2e-5 * base[j])
            pos += 1
    assert pos == g.size
    print("fd-vs-autograd %s: %.2e of max|g|, max|g| / min|g| = %.1e" % (kind, np.abs(fd - g).max() / np.abs(g).max(),
                                                                           np.abs(g).max() / np.abs(g).min()))
    np.testing.assert_allclose(g, fd, rtol=0, atol=1e-6 * np.abs(g).max())
    assert np.abs(g).min() > 1e-5 * np.abs(g).max()          # no entry passes by being ~0 (measured: 1 / 180, 1 / 9400)
    assert np.linalg.cond(R.ky_general(**{k: c[k] for k in ("Z", "kind", "v", "c0", "s", "a", "b", "noise")})) < 1e8


@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("kt", KERNELS)
def test_named_packing_is_the_model_s_packing(lib_built, kt, D):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(D)
    hyp = orc.make_hyp(kt, rng, D)
    gp = SimpleGPModel(1, D - 1, 1, kern_types=[kt], hyp=[hyp])
    np.testing.assert_array_equal(gp._pack_kernel_params()[0], R.pack_named(kt, hyp, D))
    np.testing.assert_array_equal(gp._pack_kernel_params(only=0)[0], R.pack_named(kt, hyp, D))


# ------------------------------------------------------------------ API vector -> named hyper-parameters
class _FakeBuffers(object):
    """what neg_log_marginal_likelihood needs of safe_exploration_amd._buffers, on NumPy arrays"""

    def __init__(self):
        self.sent = []

    def resolve_device(self, device=None):
        return "fake:0"

    def stream_ptr(self, dev):
        return None

    def as_dev(self, x, dev, shape=None):
        a = np.array(x, dtype=np.float64)
        self.sent.append(a)
        return a

    def empty(self, shape, dev):
        return np.full(shape, np.nan)

    def ptr(self, t):
        return t

    def to_numpy(self, t):
        return np.array(t)


class _FakeLib(object):
    def __init__(self, api_vector, nll=12.5, factorize_rc=0):
        self.api_vector, self.nll, self.factorize_rc, self.calls = api_vector, nll, factorize_rc, []

    def sr_gp_set_data_general(self, h, z, y, kp, noise, s):
        self.calls.append(("set", z.shape, y.shape, kp.copy(), noise.copy()))
        return 0

    def sr_gp_factorize(self, h, s, info):
        self.calls.append(("factorize",))
        return self.factorize_rc

    def sr_gp_mll(self, h, nll, g, s):
        assert nll.shape == (1,) and g.shape == self.api_vector.shape
        nll[0] = self.nll
        g[:] = self.api_vector
        self.calls.append(("mll",))
        return 0


class _FakeHandle(object):
    def __init__(self, device, N, D, n_out):
        self.device, self.N, self.D, self.n_out, self.h = device, N, D, n_out, object()


def _patched_model(monkeypatch, kt, D, fixed, api_vector, **kw):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.ssm_hip import gaussian_process as G
    rng = np.random.default_rng(17 + D)
    full = dict(orc.make_hyp(kt, rng, D), noise_variance=0.04)
    gp = SimpleGPModel(2, D - 1, 1, kern_types=[kt] * 2, hyp=[{k: full[k] for k in fixed}] * 2)
    for i in range(2):                      # the free ones away from their defaults too
        for k, v in full.items():
            if k == "noise_variance":
                gp._noise[i] = v
            else:
                gp.hyp[i][k] = np.array(v, dtype=float) if np.ndim(v) else float(v)
    fake = _FakeLib(api_vector, **kw)
    bufs = _FakeBuffers()
    monkeypatch.setattr(G, "lib", fake)
    monkeypatch.setattr(G, "B", bufs)
    monkeypatch.setattr(G, "_Handle", _FakeHandle)
    monkeypatch.setattr(G, "check", lambda rc: None if rc == 0 else (_ for _ in ()).throw(RuntimeError(rc)))
    return gp, full, fake, bufs


def _key_order(kt):
    if kt in ("rbf", "mat52"):
        return ["lengthscale", "variance", "noise_variance"]
    st = kt[4:]
    return ["prod.%s.lengthscale" % st, "prod.%s.variance" % st, "prod.linear.variances", "linear.variances",
            "noise_variance"]


@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("kt", KERNELS)
def test_api_vector_lands_in_the_named_hyper_parameters(lib_built, monkeypatch, kt, D):
    """A synthetic API vector [v, c0, s[D], a[D], b[D], noise] with a different value in every slot: each named gradient
    must come from its own slot (-g_s / l^2 for a lengthscale), in the order of _free_hyp, for several sets of fixed keys;
    the packed parameters and the noise (+ GPy's jitter, no noise_diag) that reach the library are the model's."""
    api = 100.0 + np.arange(3 + 3 * D, dtype=np.float64)            # slot q holds 100 + q
    keys = _key_order(kt)
    for fixed in ([], [keys[0]], [keys[1], "noise_variance"], keys[:-1], keys):
        gp, full, fake, bufs = _patched_model(monkeypatch, kt, D, fixed, api)
        Z, Y = np.zeros((7, D)), np.arange(14.0).reshape(7, 2)
        for i in range(2):
            free = gp._free_hyp(i)
            assert [k for k, _ in free] == [k for k in keys if k not in fixed]
            assert [n for _, n in free] == [int(np.size(full[k])) for k, _ in free]
            nll, g = gp.neg_log_marginal_likelihood(Z, Y, i)
            assert nll == 12.5 and g.shape == (sum(n for _, n in free),)
            if kt in ("rbf", "mat52"):
                want = {"variance": api[0:1], "lengthscale": -api[2:2 + D] / np.asarray(full["lengthscale"]) ** 2}
            else:
                st = kt[4:]
                ell = float(np.reshape(full["prod.%s.lengthscale" % st], (-1,))[0])
                want = {"prod.%s.variance" % st: api[0:1], "prod.%s.lengthscale" % st: np.array([-api[2 + 1] / ell ** 2]),
                        "prod.linear.variances": api[2 + D + 1:2 + D + 2], "linear.variances": api[2 + 2 * D:2 + 3 * D]}
            want["noise_variance"] = api[-1:]
            expect = np.concatenate([want[k] for k, _ in free]) if free else np.zeros(0)
            np.testing.assert_allclose(g, expect, rtol=1e-15, atol=0)
            # what reached the library: column i of Y, the packed row of output i, noise + 1e-8
            call = [c for c in fake.calls if c[0] == "set"][-1]
            assert call[1] == (7, D) and call[2] == (7, 1)
            np.testing.assert_array_equal(call[3], R.pack_named(kt, full, D)[None, :])
            np.testing.assert_array_equal(call[4], np.array([0.04 + 1e-8]))
            np.testing.assert_array_equal(bufs.sent[-3], Y[:, i:i + 1])
            assert gp.neg_log_marginal_likelihood(Z, Y, i, with_grad=False) == (12.5, None)
        assert gp._mll_handle.N == 7 and gp._mll_handle.n_out == 1       # one handle, reused


@pytest.mark.parametrize("kt", KERNELS)
def test_set_free_of_get_free_is_the_identity(lib_built, monkeypatch, kt):
    D = 5
    keys = _key_order(kt)
    for fixed in ([], [keys[0]], keys[1:]):
        gp, full, _, _ = _patched_model(monkeypatch, kt, D, fixed, np.zeros(3 + 3 * D))
        before = ({k: np.array(v, copy=True) for k, v in gp.hyp[0].items()}, gp._noise.copy())
        theta = gp._get_free(0)
        assert theta.shape == (sum(n for _, n in gp._free_hyp(0)),)
        gp._set_free(0, theta)
        for k, v in before[0].items():
            np.testing.assert_array_equal(gp.hyp[0][k], v)
            assert np.ndim(gp.hyp[0][k]) == np.ndim(v)                   # scalars stay scalars, vectors vectors
        np.testing.assert_array_equal(gp._noise, before[1])
        np.testing.assert_array_equal(gp._get_free(0), theta)
        # and a changed vector comes back as it was set, the fixed keys untouched
        gp._set_free(0, theta * 1.5)
        np.testing.assert_array_equal(gp._get_free(0), theta * 1.5)
        for k in fixed:
            if k != "noise_variance":
                np.testing.assert_array_equal(gp.hyp[0][k], before[0][k])
        np.testing.assert_array_equal(gp._pack_kernel_params(only=1), R.pack_named(kt, full, D)[None, :])   # output 1 alone


def test_matrix_that_is_not_positive_definite_gives_inf_and_no_gradient(lib_built, monkeypatch):
    gp, _, fake, _ = _patched_model(monkeypatch, "rbf", 3, [], np.zeros(12), factorize_rc=-4)
    assert gp.neg_log_marginal_likelihood(np.zeros((4, 3)), np.zeros((4, 2)), 0) == (np.inf, None)
    assert ("mll",) not in fake.calls
