"""Retiring training points without a refit (sr_gp_remove / SimpleGPModel.remove_data), the leave-one-out posterior
(sr_gp_loo) and the bounded update (update_model(n_max=...)) on the device -- always against a FRESH fit on the remaining
rows, at the project's "incremental equals refit" tolerances (test_row_append_update_equals_refit).

Every test here fails on the parent commit: the two symbols and the methods do not exist there."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_np as orc
from _helpers import hip_model, oracle_model
import _remove_ref as rr

pytestmark = pytest.mark.gpu

SR_EINVAL, SR_ESTATE = -1, -4


def _fresh(syn, rows, n_s, n_u):
    return hip_model(syn["Z"][rows], syn["Y"][rows], syn["lengthscale"], syn["signal_var"], syn["noise_var"], n_s, n_u)


def _logdet(gp):
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    t = B.empty((hd.n_out,), hd.device)
    check(lib.sr_gp_logdet(hd.h, B.ptr(t), B.stream_ptr(hd.device)))
    return B.to_numpy(t)


def _state(gp):
    alpha, wt = gp.export_state()
    return alpha.cpu().numpy().copy(), wt.cpu().numpy().copy()


def _assert_equals_refit(gp, syn, rows, n_s, n_u, x=None, inverse=True):
    """gp, after its removals, against a fresh fit on syn's rows `rows` (in that order)."""
    rows = np.asarray(rows)
    n = rows.size
    assert gp._handle.N == n and gp.x_train.shape[0] == n and gp._handle.Np == (n + 127) // 128 * 128
    np.testing.assert_array_equal(gp.x_train, syn["Z"][rows])
    np.testing.assert_array_equal(gp.y_train, syn["Y"][rows])
    np.testing.assert_array_equal(gp.z, syn["Z"][rows])
    full = _fresh(syn, rows, n_s, n_u)
    if x is None:
        x = np.hstack((syn["p"], syn["k_ff"]))
    mu_a, var_a, jac_a = gp.predict(x, None, True)
    mu_f, var_f, jac_f = full.predict(x, None, True)
    scale = np.abs(full.beta).sum(0).max()
    np.testing.assert_allclose(gp.beta, full.beta, rtol=1e-7, atol=1e-9 * np.abs(full.beta).max())
    np.testing.assert_allclose(mu_a, mu_f, rtol=1e-9, atol=1e-11 * scale)
    np.testing.assert_allclose(jac_a, jac_f, rtol=1e-9, atol=1e-10 * scale)
    np.testing.assert_allclose(var_a, var_f, rtol=0, atol=1e-9)
    # the factor itself: equal to the refit's entry by entry, zeros below the diagonal and identity padding exact
    wa, wf = _state(gp)[1], _state(full)[1]
    off = gp._handle.Np - n
    assert wa.shape == wf.shape
    for d in range(n_s):
        assert np.all(np.tril(wa[d], -1) == 0.0)
        assert np.all(wa[d][:off, :off] == np.eye(off)) and np.all(wa[d][:off, off:] == 0.0)
        np.testing.assert_allclose(wa[d], wf[d], rtol=1e-6, atol=1e-9 * np.abs(wf[d]).max())
    np.testing.assert_allclose(_logdet(gp), _logdet(full), rtol=1e-10, atol=1e-8)
    if inverse:
        om = oracle_model(syn["Z"][rows], syn["Y"][rows], syn["lengthscale"], syn["signal_var"], syn["noise_var"])
        _, rvar = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"], False)
        np.testing.assert_allclose(var_a, rvar, rtol=0, atol=1e-9)
        np.testing.assert_allclose(gp.inv_K[0], om["inv_K"][0], rtol=1e-6, atol=1e-8 * np.abs(om["inv_K"][0]).max())
    return full


@pytest.mark.parametrize("N0,idx,n_s", [(129, 0, 2), (129, 128, 2), (200, 77, 2), (256, 255, 2), (257, 0, 2), (385, 200, 2),
                                        (640, 0, 2), (640, 639, 2), (257, 130, 4), (200, 0, 1)])
def test_single_removal_equals_refit(N0, idx, n_s):
    """first, a middle and the last row; front padding 0 (256, 640) and 127 (129, 257, 385); 129 -> 128, 257 -> 256 and
    385 -> 384 cross a padded size downward; one, two and four outputs"""
    syn = orc.make_synthetic(1000 + N0 + idx, N0, n_s, 1, 64)
    gp = _fresh(syn, np.arange(N0), n_s, 1)
    gp.remove_data(idx)
    x = np.hstack((syn["p"], syn["k_ff"]))
    full = _assert_equals_refit(gp, syn, np.delete(np.arange(N0), idx), n_s, 1, x=x)
    np.testing.assert_allclose(gp.predict(x[:1])[1], full.predict(x[:1])[1], rtol=0, atol=1e-9)      # the single-query path


@pytest.mark.parametrize("N0,idx", [(300, [299, 0, 150, 151, 17]), (260, [3, 259, 100, 101, 102, 7, 200, 64, 128, 255])])
def test_several_removals_in_one_call(N0, idx):
    """unsorted indices; 260 -> 250 crosses the padded size 384 -> 256 in the middle of the call"""
    syn = orc.make_synthetic(2000 + N0, N0, 2, 1, 64)
    gp = _fresh(syn, np.arange(N0), 2, 1)
    gp.remove_data(idx)
    _assert_equals_refit(gp, syn, np.delete(np.arange(N0), idx), 2, 1)


def _slide_steps(gp):
    from safe_exploration_amd._lib import lib, check
    steps, aborts = ctypes.c_int(-1), ctypes.c_long(-1)
    check(lib.sr_gp_slide_steps(gp._handle.h, ctypes.byref(steps)))
    check(lib.sr_gp_grid_append_aborts(gp._handle.h, ctypes.byref(aborts)))
    return steps.value, aborts.value


def test_removal_after_in_place_appends():
    """N0 = 600: one-point appends go IN PLACE (the model's buffers become views into their allocations); a removal from the
    slid state, an append and a removal again; the single-query path and a T = 256 batch (the tile route's alignment
    path) afterwards."""
    N0 = 600
    syn = orc.make_synthetic(77, N0 + 4, 2, 1, 256)
    gp = _fresh(syn, np.arange(N0), 2, 1)
    gp.append_limit = 10 ** 9
    rows = list(range(N0))
    for i in range(N0, N0 + 3):
        gp.update_model(syn["Z"][i:i + 1], syn["Y"][i:i + 1], opt_hyp=False, replace_old=False)
        rows.append(i)
    steps, aborts = _slide_steps(gp)
    if aborts == 0:                      # (a grid that could not become resident falls back to separate launches)
        assert steps > 0
    gp.remove_data(0)
    del rows[0]
    assert _slide_steps(gp)[0] == 0
    gp.update_model(syn["Z"][N0 + 3:N0 + 4], syn["Y"][N0 + 3:N0 + 4], opt_hyp=False, replace_old=False)
    rows.append(N0 + 3)
    gp.remove_data(301)
    del rows[301]
    x = np.hstack((syn["p"], syn["k_ff"]))
    assert x.shape[0] == 256
    full = _assert_equals_refit(gp, syn, rows, 2, 1, x=x)
    mu1, var1 = gp.predict(x[:1])
    mu_f, var_f = full.predict(x[:1])
    scale = np.abs(full.beta).sum(0).max()
    np.testing.assert_allclose(mu1, mu_f, rtol=1e-9, atol=1e-11 * scale)
    np.testing.assert_allclose(var1, var_f, rtol=0, atol=1e-9)


def test_append_remove_rounds():
    """append one, retire one, six rounds (first, middle and last rows in turn) against a fit on the final rows"""
    N0 = 520
    syn = orc.make_synthetic(78, N0 + 6, 2, 1, 256)
    gp = _fresh(syn, np.arange(N0), 2, 1)
    gp.append_limit = 10 ** 9
    rows = list(range(N0))
    for r in range(6):
        i = N0 + r
        gp.update_model(syn["Z"][i:i + 1], syn["Y"][i:i + 1], opt_hyp=False, replace_old=False)
        rows.append(i)
        j = (0, len(rows) // 2, len(rows) - 1)[r % 3]
        gp.remove_data(j)
        del rows[j]
    x = np.hstack((syn["p"], syn["k_ff"]))
    full = _assert_equals_refit(gp, syn, rows, 2, 1, x=x)
    np.testing.assert_allclose(gp.predict(x[:1])[1], full.predict(x[:1])[1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("kt", ["mat52", "lin_rbf"])
def test_removal_with_the_journal_kernels(kt):
    """the general kernel family (built as in test_row_append_with_the_journal_kernels, its tolerances)"""
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(277)
    D, N0 = 3, 200
    Z = rng.uniform(-1, 1, (N0, D))
    Y = rng.standard_normal((N0, 2))
    hyp = [orc.make_hyp(kt, rng, D) for _ in range(2)]
    noise = np.array([0.02, 0.03])
    hh = [dict(h, noise_variance=nv) for h, nv in zip(hyp, noise)]
    gp = SimpleGPModel(2, 2, 1, kern_types=[kt] * 2, hyp=hh)
    gp.train(Z, Y, opt_hyp=False)
    gp.remove_data([0, 100])
    keep = np.delete(np.arange(N0), [0, 100])
    assert gp._handle.N == N0 - 2
    full = SimpleGPModel(2, 2, 1, kern_types=[kt] * 2, hyp=hh)
    full.train(Z[keep], Y[keep], opt_hyp=False)
    np.testing.assert_allclose(gp.beta, full.beta, rtol=1e-6, atol=1e-8 * np.abs(full.beta).max())
    x = rng.uniform(-0.8, 0.8, (40, D))
    mu_a, var_a, jac_a = gp.predict(x, None, True)
    mu_f, var_f, jac_f = full.predict(x, None, True)
    scale = max(np.abs(full.beta).sum(0).max(), 1.0)
    np.testing.assert_allclose(mu_a, mu_f, rtol=1e-8, atol=1e-10 * scale)
    np.testing.assert_allclose(jac_a, jac_f, rtol=1e-8, atol=1e-9 * scale)
    np.testing.assert_allclose(var_a, var_f, rtol=0, atol=1e-9 * scale)
    wa, wf = _state(gp)[1], _state(full)[1]
    for d in range(2):
        assert np.all(np.tril(wa[d], -1) == 0.0)
        np.testing.assert_allclose(wa[d], wf[d], rtol=1e-6, atol=1e-9 * np.abs(wf[d]).max())
    beta_ref, inv_K = orc.gp_fit_k(Z[keep], Y[keep], [kt] * 2, hyp, noise + 1e-5)
    rmu, rvar = orc.gp_predict_k(x, Z[keep], beta_ref, inv_K, [kt] * 2, hyp)
    np.testing.assert_allclose(mu_a, rmu, rtol=1e-7, atol=1e-8 * scale)
    np.testing.assert_allclose(var_a, rvar, rtol=0, atol=1e-7 * scale)


def test_errors_leave_the_model_bit_identical():
    from safe_exploration_amd import SimpleGPModel, _buffers as B
    from safe_exploration_amd._lib import lib
    N0 = 140
    syn = orc.make_synthetic(5, N0, 2, 1, 8)
    gp = _fresh(syn, np.arange(N0), 2, 1)
    before = _state(gp)
    s = B.stream_ptr(gp._handle.device)

    def c_remove(idx):
        arr = (ctypes.c_int * max(len(idx), 1))(*idx)
        return lib.sr_gp_remove(gp._handle.h, arr, len(idx), s)

    assert c_remove([3, 7, 3]) == SR_EINVAL              # a duplicate
    assert c_remove([N0]) == SR_EINVAL                   # index = N
    assert c_remove([-1]) == SR_EINVAL
    assert c_remove(list(range(N0))) == SR_EINVAL        # m = N: at least one point stays
    assert c_remove([]) == SR_EINVAL                     # m = 0
    assert lib.sr_gp_remove(gp._handle.h, None, 1, s) == SR_EINVAL
    for bad in ([3, 7, 3], N0, list(range(N0))):
        with pytest.raises(ValueError):
            gp.remove_data(bad)
    after = _state(gp)
    assert gp._handle.N == N0 and gp.x_train.shape[0] == N0
    for u, v in zip(before, after):
        np.testing.assert_array_equal(u, v)
    # a sparse handle: SR_ESTATE from the C call, nothing touched; remove_data refits the remaining rows instead
    hyp = [{"lengthscale": syn["lengthscale"][d], "variance": syn["signal_var"][d], "noise_variance": syn["noise_var"][d]}
           for d in range(2)]
    Zu = syn["Z"][:32].copy()
    sp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, Z=Zu)
    sp.do_sparse_gp = True
    sp.train(syn["Z"], syn["Y"], 32, opt_hyp=False, Z=Zu)
    sb = _state(sp)
    arr = (ctypes.c_int * 1)(0)
    assert lib.sr_gp_remove(sp._handle.h, arr, 1, s) == SR_ESTATE
    mu_t = B.empty((2, 32), sp._handle.device)
    assert lib.sr_gp_loo(sp._handle.h, B.ptr(mu_t), None, s) == SR_ESTATE
    for u, v in zip(sb, _state(sp)):
        np.testing.assert_array_equal(u, v)
    sp.remove_data([1, 5])
    assert sp.x_train.shape[0] == N0 - 2 and sp.is_sparse and sp._handle.N == 32
    ref = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, Z=Zu)
    ref.do_sparse_gp = True
    keep = np.delete(np.arange(N0), [1, 5])
    ref.train(syn["Z"][keep], syn["Y"][keep], 32, opt_hyp=False, Z=Zu)
    for u, v in zip(_state(sp), _state(ref)):
        np.testing.assert_array_equal(u, v)


def test_cached_logdet_is_never_stale_and_removal_is_deterministic():
    from safe_exploration_amd._lib import lib
    N0 = 300
    syn = orc.make_synthetic(6, N0 + 1, 2, 1, 8)
    states = []
    for _ in range(2):
        gp = _fresh(syn, np.arange(N0), 2, 1)
        gp.append_limit = 10 ** 9
        gp.update_model(syn["Z"][N0:], syn["Y"][N0:], opt_hyp=False, replace_old=False)     # leaves a host copy of log det
        host = (ctypes.c_double * 2)()
        assert lib.sr_gp_logdet_cached(gp._handle.h, host) == 0
        gp.remove_data([40, 250])
        rc = lib.sr_gp_logdet_cached(gp._handle.h, host)
        assert rc in (0, SR_ESTATE)
        if rc == 0:
            np.testing.assert_allclose(np.array(host[:]), _logdet(gp), rtol=0, atol=1e-9)
        states.append(_state(gp))
    for u, v in zip(*states):
        np.testing.assert_array_equal(u, v)           # the same call on the same state: the same bits


def test_removal_under_the_resident_server():
    syn = orc.make_synthetic(79, 100, 2, 1, 6)
    gp = _fresh(syn, np.arange(100), 2, 1)
    assert gp.start_server(idle_timeout_s=0.002)
    gp(syn["p"][:1], syn["k_ff"][:1])
    gp.remove_data(0)
    o = gp(syn["p"][:1], syn["k_ff"][:1])
    armed, _, _, calls = gp.server_state()
    assert armed and calls == 2                        # still armed, and the second query was SERVED
    ref = _fresh(syn, np.arange(1, 100), 2, 1)
    r = ref(syn["p"][:1], syn["k_ff"][:1])
    for u, v in zip(o, r):
        np.testing.assert_allclose(u, v, rtol=1e-9, atol=1e-11)
    mu, var = ref.predict(np.hstack((syn["p"][:1], syn["k_ff"][:1])))
    np.testing.assert_allclose(o[0][:, 0], mu[0], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(o[1][:, 0], var[0], rtol=0, atol=1e-9)
    gp.stop_server()


def test_loo_against_the_oracle_inverse_and_explicit_refits():
    N = 200
    syn = orc.make_synthetic(80, N, 2, 1, 8)
    Z, Y = syn["Z"], syn["Y"]
    gp = _fresh(syn, np.arange(N), 2, 1)
    mu, var = gp.loo()
    assert mu.shape == (N, 2) and var.shape == (N, 2)
    mu_d, var_d = gp.loo_device()
    np.testing.assert_array_equal(mu_d.cpu().numpy(), mu)
    np.testing.assert_array_equal(var_d.cpu().numpy(), var)
    om = oracle_model(Z, Y, syn["lengthscale"], syn["signal_var"], syn["noise_var"])
    scale = np.abs(Y).max()
    for d in range(2):
        rmu, rvar = rr.loo_from_inv(om["inv_K"][d], om["beta"][:, d], Y[:, d])
        np.testing.assert_allclose(var[:, d], rvar, rtol=1e-7)
        np.testing.assert_allclose(mu[:, d], rmu, rtol=0, atol=1e-8 * scale)
    # five rows against actual fits with that row left out (the predictive variance of the OBSERVATION: + noise)
    for j in (0, 1, 99, 150, N - 1):
        keep = np.delete(np.arange(N), j)
        o1 = oracle_model(Z[keep], Y[keep], syn["lengthscale"], syn["signal_var"], syn["noise_var"])
        pm, pv = orc.gp_predict(Z[j:j + 1], o1["Z"], o1["beta"], o1["inv_K"], o1["lengthscale"], o1["signal_var"], False)
        np.testing.assert_allclose(mu[j], pm[0], rtol=0, atol=1e-8 * scale)
        np.testing.assert_allclose(var[j], pv[0] + syn["noise_var"] + 1e-8, rtol=1e-7)
    # the slid state of the in-place appends is read as it is (no copy back)
    big = orc.make_synthetic(81, 601, 2, 1, 8)
    g2 = _fresh(big, np.arange(600), 2, 1)
    g2.append_limit = 10 ** 9
    g2.update_model(big["Z"][600:], big["Y"][600:], opt_hyp=False, replace_old=False)
    steps = _slide_steps(g2)[0]
    mu2, var2 = g2.loo()
    assert _slide_steps(g2)[0] == steps
    f2 = _fresh(big, np.arange(601), 2, 1)
    mu3, var3 = f2.loo()
    np.testing.assert_allclose(var2, var3, rtol=1e-7)
    np.testing.assert_allclose(mu2, mu3, rtol=0, atol=1e-8 * np.abs(big["Y"]).max())


def test_update_model_n_max_sliding_window():
    """N0 = 150, n_max = 150, 20 one-point updates retiring the oldest row: N stays 150 and the model is the fit on the
    last 150 rows; n_max = None leaves update_model as it was."""
    N0, steps = 150, 20
    syn = orc.make_synthetic(82, N0 + steps, 2, 1, 64)
    gp = _fresh(syn, np.arange(N0), 2, 1)
    gp.append_limit = 10 ** 9
    h0 = gp._handle
    for i in range(N0, N0 + steps):
        gp.update_model(syn["Z"][i:i + 1], syn["Y"][i:i + 1], opt_hyp=False, replace_old=False, n_max=N0, retire="oldest")
        assert gp._handle.N == N0 and gp.x_train.shape[0] == N0
    assert gp._handle is h0                            # no refit on the way
    _assert_equals_refit(gp, syn, np.arange(steps, N0 + steps), 2, 1)
    gp.update_model(syn["Z"][:1], syn["Y"][:1], opt_hyp=False, replace_old=False)
    assert gp._handle.N == N0 + 1
    with pytest.raises(ValueError):
        gp.update_model(syn["Z"][:1], syn["Y"][:1], opt_hyp=False, replace_old=False, n_max=N0, retire="bogus")
    assert gp._handle.N == N0 + 1
    # the refit route drops the same rows on the host
    g2 = _fresh(syn, np.arange(N0), 2, 1)
    g2.append_limit = 0
    g2.update_model(syn["Z"][N0:N0 + 5], syn["Y"][N0:N0 + 5], opt_hyp=False, replace_old=False, n_max=N0)
    np.testing.assert_array_equal(g2.x_train, syn["Z"][5:N0 + 5])
    assert g2._handle.N == N0


def test_update_model_retires_the_most_redundant_row():
    """one near-duplicate pair (rows 12 and 37); the row that goes is the one _remove_ref's score names on the oracle's fit
    of all rows, and the reference's margin to the runner-up is far above rounding"""
    N0 = 60
    syn = orc.make_synthetic(91, N0 + 1, 2, 1, 8)
    syn["Z"][37] = syn["Z"][12] + 1e-3
    Z, Y = syn["Z"], syn["Y"]
    om = oracle_model(Z, Y, syn["lengthscale"], syn["signal_var"], syn["noise_var"])
    var = np.column_stack([rr.loo_from_inv(om["inv_K"][d], om["beta"][:, d], Y[:, d])[1] for d in range(2)])
    score = rr.redundancy_scores(om["beta"], var)
    order = np.argsort(score)
    jref = int(order[0])
    assert score[order[1]] > 1.01 * score[jref]
    gp = _fresh(syn, np.arange(N0), 2, 1)
    gp.append_limit = 10 ** 9
    gp.update_model(Z[N0:], Y[N0:], opt_hyp=False, replace_old=False, n_max=N0, retire="redundant")
    keep = np.delete(np.arange(N0 + 1), jref)
    _assert_equals_refit(gp, syn, keep, 2, 1)
    # the refit route scores the same model and drops the same row
    g2 = _fresh(syn, np.arange(N0), 2, 1)
    g2.append_limit = 0
    g2.update_model(Z[N0:], Y[N0:], opt_hyp=False, replace_old=False, n_max=N0, retire="redundant")
    np.testing.assert_array_equal(g2.x_train, Z[keep])
