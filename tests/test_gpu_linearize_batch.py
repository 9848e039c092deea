"""Batched second-order linearisation (sr_gp_linearize_batch, SimpleGPModel.linearize_device_batch and
linearize_predict_batch): the Hessian of the mean for every query of a batch, against the fp64 oracle, the single-query
route, central differences of the batched d mu/dx, and itself across widths, chunk boundaries, repeated calls and model
updates; mu, var, jac_mu and jac_var against sr_gp_predict_grad to the bit.

Bars: ARD-RBF hess_mu rtol 1e-8 atol 100 mu_atol, the general family rtol 1e-8 atol 1e-10 |beta|_1 (the hm bars of
test_gpu_widths._tol, which the single-query routes meet)."""
import ctypes

import numpy as np
import pytest

from _helpers import hip_model, mu_atol, hyp_from, cached_oracle_model, width_problem, width_oracle, width_gp, \
    width_queries
from oracle import oracle_np as orc
from test_gpu_widths import _tol, _close, _oracle_rows, _assert_informative, _seed

pytestmark = pytest.mark.gpu
N_S, N_U = 2, 1
KERNELS = ("rbf", "mat52", "lin_rbf", "lin_mat52")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _queries(seed, T, D=N_S + N_U):
    rng = np.random.default_rng(seed)
    return np.hstack((0.3 * rng.standard_normal((T, N_S)), 0.1 * rng.standard_normal((T, D - N_S))))


def _model(N, seed=5):
    om = cached_oracle_model(seed, N, N_S, N_U)
    syn = orc.make_synthetic(seed, N, N_S, N_U, 4)
    gp = hip_model(syn["Z"], syn["Y"], syn["lengthscale"], syn["signal_var"], syn["noise_var"], N_S, N_U)
    return om, gp


def _np(outs):
    return tuple(o.cpu().numpy() for o in outs)


def _hm_atol(om):
    return 100 * mu_atol(om)


def _check_hess_rbf(x, hm, om, rows):
    for t in rows:
        _, rhm = orc.gp_linearize_extras(x[t], om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
        np.testing.assert_allclose(hm[t], rhm, rtol=1e-8, atol=_hm_atol(om), err_msg="row %d" % t)


# ------------------------------------------------------------------ 1. RBF against the oracle
@pytest.mark.parametrize("N", [50, 200, 1000, 2000])
def test_linearize_batch_oracle_rbf(N):
    om, gp = _model(N)
    rng = np.random.default_rng(N)
    for T in (2, 17, 129, 1000):
        x = _queries(200 + T, T)
        mu, var, jm, jv, hm = _np(gp.linearize_device_batch(x))
        assert hm.shape == (T, N_S, N_S + N_U, N_S + N_U)
        rows = np.arange(T) if T <= 64 else np.sort(rng.choice(T, 64, replace=False))
        _check_hess_rbf(x, hm, om, rows)
        assert np.abs(hm).max() > 1e3 * _hm_atol(om)


# ------------------------------------------------------------------ 2. the general family against the oracle
@pytest.mark.parametrize("kt", ["mat52", "lin_rbf", "lin_mat52"])
def test_linearize_batch_general_kernels(kt):
    prob = width_problem(_seed("hess-general", kt), kt, 3, 700, 2)
    om, gp = width_oracle(prob), width_gp(prob)
    T = 300
    x = width_queries(prob, T, _seed("hess-general-q", kt))
    rng = np.random.default_rng(3)
    rows = np.sort(np.concatenate((np.arange(8), rng.choice(np.arange(8, T), 24, replace=False))))
    mu, var, jm, jv, hm = _np(gp.linearize_device_batch(x))
    rmu, rvar, rjm, rjv, rhm = _oracle_rows(om, x, rows)
    _assert_informative(om, x, rvar, rjv, rhm)
    tol = _tol(om)
    assert tol["hm"] == (1e-8, 1e-10 * max(float(np.abs(om["beta"]).sum(0).max()), 1.0))
    _close("hm", hm[rows], rhm, tol, kt)
    _close("jv", jv[rows], rjv, tol, kt)
    _close("mu", mu, rmu, tol, kt)
    _close("var", var, rvar, tol, kt)


# ------------------------------------------------------------------ 3. identity with the gradient pass
@pytest.mark.parametrize("kt,n_out,T", [("rbf", 2, 300), ("rbf", 1, 5), ("mat52", 2, 1000), ("lin_rbf", 3, 129)])
def test_linearize_batch_first_order_is_predict_grad(kt, n_out, T):
    prob = width_problem(_seed("hess-ident", kt, n_out), kt, 3, 900, n_out)
    gp = width_gp(prob)
    x = width_queries(prob, T, _seed("hess-ident-q", kt, n_out, T))
    lin = _np(gp.linearize_device_batch(x))
    grad = _np(gp.predict_device_grad(x))
    for name, a, b in zip(("mu", "var", "jac_mu", "jac_var"), lin[:4], grad):
        np.testing.assert_array_equal(a, b, err_msg=name)


# ------------------------------------------------------------------ 4. against the single-query route
def test_linearize_batch_matches_single_query_route():
    om, gp = _model(1500)
    x = _queries(3, 200)
    hm = gp.linearize_device_batch(x)[4].cpu().numpy()
    # the bars of the single-query routes against each other (test_gpu_widths.test_single_query_second_order_widths)
    scale = max(float(np.abs(om["beta"]).sum(0).max()), 1.0)
    for t in range(12):
        ref = gp.linearize_device(x[t])[4].cpu().numpy()
        np.testing.assert_allclose(hm[t], ref, rtol=1e-8, atol=1e-10 * scale, err_msg="row %d" % t)


# ------------------------------------------------------------------ 5. independent of the oracle
def test_linearize_batch_central_differences():
    """H_jc = d (d mu/dx_j) / dx_c against central differences of the batched d mu/dx (predict_device_grad).
    Step h_c = 1e-4 l_c (l_c the smallest lengthscale of coordinate c over the outputs).  On this model (|alpha|_1 ~ 4e3,
    max |H| ~ 10) the same differences of the fp64 oracle's d mu/dx miss its closed-form Hessian by 7e-9 max |H| at this
    step (truncation, h^2 / 6 d^4 mu; 7e-7 at 1e-3 l) and by 1.5e-9 max |H| at 1e-5 l (rounding of d mu/dx over 2 h).
    The bar, 1e-6 max |H| (plus rtol 1e-6), sits two orders above that and far below a wrong entry (~ max |H|)."""
    import torch
    om, gp = _model(1000)
    T, D = 64, N_S + N_U
    x = _queries(4, T)
    hm = gp.linearize_device_batch(x)[4].cpu().numpy()
    l = np.min(om["lengthscale"], axis=0)
    fd = np.empty_like(hm)
    for c in range(D):
        h = 1e-4 * l[c]
        xp, xm = x.copy(), x.copy()
        xp[:, c] += h
        xm[:, c] -= h
        jp = gp.predict_device_grad(torch.from_numpy(xp))[2].cpu().numpy()
        jn = gp.predict_device_grad(torch.from_numpy(xm))[2].cpu().numpy()
        fd[:, :, :, c] = (jp - jn) / (2 * h)
    np.testing.assert_allclose(hm, fd, rtol=1e-6, atol=1e-6 * np.abs(hm).max())


# ------------------------------------------------------------------ 6. widths and symmetry
WIDTHS = (2, 3, 4, 5, 6, 8)                          # either side of the DT edges 3 and 5, and DT = 8 (SR_GRAD_MAX_D)
WIDTH_CASES = ([(KERNELS[(2 * i + k) % 4], D, n_out) for i, D in enumerate(WIDTHS) for k, n_out in enumerate((1, 2))] +
               [("rbf", 6, 9), ("mat52", 6, 9)])


@pytest.mark.parametrize("kt,D,n_out", WIDTH_CASES)
def test_linearize_batch_widths(kt, D, n_out):
    """every padded width DT = 3, 5, 8 on both forms (ARD-RBF from the K* slab, the general family from Z); the D-wide
    triangle of the partials mapped to D x D where D != DT; exact symmetry"""
    prob = width_problem(_seed("hess-width", kt, D, n_out), kt, D, 300, n_out)
    om, gp = width_oracle(prob), width_gp(prob)
    T = 129
    x = width_queries(prob, T, _seed("hess-width-q", kt, D, n_out))
    mu, var, jm, jv, hm = _np(gp.linearize_device_batch(x))
    assert hm.shape == (T, n_out, D, D)
    np.testing.assert_array_equal(hm, np.swapaxes(hm, -1, -2))
    rows = np.arange(0, T, 4)
    rmu, rvar, rjm, rjv, rhm = _oracle_rows(om, x, rows)
    _assert_informative(om, x, rvar, rjv, rhm)
    tol = _tol(om)
    _close("hm", hm[rows], rhm, tol, "%s D=%d n_out=%d" % (kt, D, n_out))
    _close("mu", mu, rmu, tol)
    _close("var", var, rvar, tol)


# ------------------------------------------------------------------ 7. chunk boundaries
def test_linearize_batch_chunk_boundaries():
    om, gp = _model(2000)
    T = 1000
    x = _queries(5, T)
    whole = _np(gp.linearize_device_batch(x))
    gp.set_chunk(128)
    try:
        parts = _np(gp.linearize_device_batch(x))
    finally:
        gp.set_chunk(65536)
    # the K* pass and the Hessian pass split the training rows by the chunk's width: the same numbers, other sums
    at = mu_atol(om)
    for name, a, b, atol in zip(("mu", "var", "jac_mu", "jac_var", "hess_mu"), parts, whole,
                                (at, 1e-15, at, 1e-15, at)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=atol, err_msg=name)
    rows = np.sort(np.random.default_rng(7).choice(T, 64, replace=False))
    _check_hess_rbf(x, parts[4], om, rows)


# ------------------------------------------------------------------ 8. every output written, determinism, T = 0
@pytest.mark.parametrize("kt", ["rbf", "lin_mat52"])
def test_linearize_batch_writes_everything_and_repeats(kt):
    import torch
    from safe_exploration_amd import _lib
    prob = width_problem(_seed("hess-nan", kt), kt, 5, 600, 2)
    gp = width_gp(prob)
    hd = gp._handle
    T, n, D = 777, 2, 5
    x = torch.from_numpy(width_queries(prob, T, 11)).to(gp.device)
    runs = []
    for _ in range(2):
        outs = [torch.full(s, float("nan"), dtype=torch.float64, device=gp.device)
                for s in ((T, n), (T, n), (T, n, D), (T, n, D), (T, n, D, D))]
        rc = _lib.lib.sr_gp_linearize_batch(hd.h, ctypes.c_void_p(x.data_ptr()), T,
                                            *[ctypes.c_void_p(o.data_ptr()) for o in outs], None)
        assert rc == _lib.SR_OK, _lib.last_error()
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
        for o in outs:
            assert np.isfinite(o).all()
        runs.append(outs)
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    empty = gp.linearize_predict_batch(np.zeros((0, D - 1)), np.zeros((0, 1)))
    assert [o.shape for o in empty] == [(0, n), (0, n), (0, n, D), (0, n, D), (0, n, D, D)]
    assert all(isinstance(o, np.ndarray) for o in empty)
    assert [tuple(o.shape) for o in gp.linearize_device_batch(x[:0])] == [(0, n), (0, n), (0, n, D), (0, n, D),
                                                                          (0, n, D, D)]


# ------------------------------------------------------------------ 9. routing
def test_linearize_batch_takes_no_per_row_loop(monkeypatch):
    import torch
    from safe_exploration_amd import SimpleGPModel
    om, gp = _model(800)

    def boom(self, x):
        raise AssertionError("per-row linearisation called")

    monkeypatch.setattr(SimpleGPModel, "_linearize_host", boom)
    for T in (2, 64):
        x = _queries(6 + T, T)
        outs = gp.linearize_predict_batch(x[:, :N_S], x[:, N_S:])
        assert len(outs) == 5 and all(isinstance(o, np.ndarray) for o in outs)
        assert outs[4].shape == (T, N_S, N_S + N_U, N_S + N_U)
        _check_hess_rbf(x, outs[4], om, range(T))
        tx = torch.from_numpy(x).to(gp.device)
        touts = gp.linearize_predict_batch(tx[:, :N_S], tx[:, N_S:])
        assert all(isinstance(o, torch.Tensor) and o.device == tx.device for o in touts)
        for a, b in zip(touts, outs):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
    # one row: the single-query latency route, same shapes as a batch
    monkeypatch.undo()
    x = _queries(9, 1)
    one = gp.linearize_predict_batch(x[:, :N_S], x[:, N_S:])
    assert [o.shape for o in one] == [(1, N_S), (1, N_S), (1, N_S, 3), (1, N_S, 3), (1, N_S, 3, 3)]
    _check_hess_rbf(x, one[4], om, [0])
    with pytest.raises(NotImplementedError):
        gp.linearize_predict(np.zeros((2, N_S)), np.zeros((2, N_U)), True)


def test_linearize_batch_beyond_max_d_loops():
    from safe_exploration_amd import SimpleGPModel, _lib
    D = 9
    assert D == SimpleGPModel.GRAD_MAX_D + 1
    prob = width_problem(_seed("hess-d9"), "rbf", D, 300, 2)
    om, gp = width_oracle(prob), width_gp(prob)
    x = width_queries(prob, 5, 12)
    import torch
    tx = torch.from_numpy(x).to(gp.device)
    outs = [torch.empty(s, dtype=torch.float64, device=gp.device) for s in ((5, 2), (5, 2), (5, 2, D), (5, 2, D),
                                                                            (5, 2, D, D))]
    rc = _lib.lib.sr_gp_linearize_batch(gp._handle.h, ctypes.c_void_p(tx.data_ptr()), 5,
                                        *[ctypes.c_void_p(o.data_ptr()) for o in outs], None)
    assert rc == _lib.SR_EUNSUPPORTED
    assert "sr_gp_linearize" in _lib.last_error()
    mu, var, jm, jv, hm = gp.linearize_predict_batch(x[:, :D - 1], x[:, D - 1:])
    rmu, rvar, rjm, rjv, rhm = _oracle_rows(om, x, np.arange(5))
    tol = _tol(om)
    _close("hm", hm, rhm, tol)
    _close("jv", jv, rjv, tol)
    _close("mu", mu, rmu, tol)


# ------------------------------------------------------------------ 10. model updates, two handles
@pytest.mark.parametrize("n_out", [1, 3])
def test_linearize_batch_follows_model_updates(n_out):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(60 + n_out)
    D, N = 3, 900
    Z = rng.uniform(-1, 1, (N, D))
    Y = rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.5, (n_out, D))
    sf2 = rng.uniform(0.5, 1.5, n_out)
    noise = np.full(n_out, 1e-2 + 1e-5)

    def fit(Zf, Yf):
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp_from(ls, sf2, noise))
        gp.train(Zf, Yf, opt_hyp=False)
        return gp

    gps = [fit(Z, Y), fit(Z, Y)]                           # two handles alive
    x = rng.uniform(-0.8, 0.8, (300, D))
    before = [gp.linearize_device_batch(x)[4].cpu().numpy() for gp in gps]
    np.testing.assert_array_equal(before[0], before[1])
    for m in (1, 40):                                      # a one-row append, then a block of rows
        gps[0].update_model(rng.uniform(-1, 1, (m, D)), rng.standard_normal((m, n_out)), replace_old=False)
    big = rng.uniform(-0.8, 0.8, (3000, D))
    gps[0].linearize_device_batch(big)                     # grows handle 0's workspace only
    hm = gps[0].linearize_device_batch(x)[4].cpu().numpy()
    assert not np.allclose(hm, before[0])
    fresh = fit(gps[0].z_fit, gps[0].y_z).linearize_device_batch(x)[4].cpu().numpy()
    beta, inv_K, _ = orc.gp_fit(gps[0].z_fit, gps[0].y_z, ls, sf2, noise)
    atol = 100 * 1e-12 * float(np.sqrt(sf2.max()) * np.abs(beta).sum(0).max())     # 100 mu_atol
    np.testing.assert_allclose(hm, fresh, rtol=1e-8, atol=atol)
    for t in range(0, 300, 30):
        _, rhm = orc.gp_linearize_extras(x[t], gps[0].z_fit, beta, inv_K, ls, sf2)
        np.testing.assert_allclose(hm[t], rhm, rtol=1e-8, atol=atol, err_msg="row %d" % t)
    np.testing.assert_array_equal(gps[1].linearize_device_batch(x)[4].cpu().numpy(), before[1])
