"""Every compiled input width and the output counts beyond the factorisation slots against the fp64 oracle.

The hot kernels are templates over a padded width DT (D <= 3 ? 3 : D <= 5 ? 5 : D <= 8 ? 8 : 12) and the dispatch
switches routes on D (sr_common.h: SR_STREAM_FUSED_MAX_D, SR_LIN_FUSED_MAX_D, the one-launch pass K0 up to D = 8;
sr_predict_grad.hip: SR_GRAD_MAX_D).  A width bug does not crash: it returns plausible numbers -- a mis-mapped Hessian
entry, a padded column that is not masked, a wrong offset.  So every route below is compared with the oracle at the
widths either side of each edge, with data on which the gradients are not ~0 (asserted on the oracle side in every test),
and the profiler pins down which route ran.  The width lists are module constants: tests/test_widths_host.py checks on
the CPU that they still hold every edge and edge + 1 of the sources.

Tolerances (oracle side): ARD-RBF mu rtol 1e-9 atol mu_atol, var atol 1e-9 sf2, jac_mu 10 mu_atol, jac_var rtol 1e-9
atol 1e-11 sf2 / l_min^2, hess_mu rtol 1e-8 atol 100 mu_atol; the general family (mat52, lin_rbf, lin_mat52) at the bars
of the existing general-kernel tests: mu / jac_mu atol 1e-11 |beta|_1, var 1e-8, jac_var rtol 1e-7 atol 1e-9, hess_mu
atol 1e-10 |beta|_1."""
import zlib

import numpy as np
import pytest

from _helpers import mu_atol, width_problem, width_oracle, width_gp, width_queries
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

# mirrors of the sources' thresholds (checked against them on the CPU by tests/test_widths_host.py)
DT_LADDER = (3, 5, 8, 12)
SR_STREAM_FUSED_MAX_D = 5
SR_LIN_FUSED_MAX_D = 3
SR_GRAD_MAX_D = 8
K0_MAX_D, K0_GENERAL_LIN_MAX_D = 8, 5

# the width lists of each group of tests
LIN_WIDTHS = (3, 4, 5, 6, 7, 8, 9, 11, 12)          # single query, second order (3 and 5: the reference's anchors)
LIN_NS = (200, 500, 1300, 3000)                      # K0 (Np = 256), Np = 512 streamed, two streamed sizes
LIN_KERNELS = ("rbf", "mat52", "lin_rbf")
BATCH_WIDTHS = (3, 4, 5, 6, 8, 9, 12)                # batched posterior
BATCH_NS = (700, 2500)                               # either side of SR_MFMA_SMALL_MAX_NP (2048 padded rows)
BATCH_TS = (1, 3, 16, 33, 128, 300, 1100)
BATCH_GENERAL_WIDTHS = (6, 12)                       # lin_mat52: the general K* pass at DT = 8 and 12
KSTAR2_WIDTHS = (4, 5, 6)                            # T = 8193: sr_kstar_kernel<5, 2, 2> (D <= 5) and its contrast
STREAM_EDGE_WIDTHS = (5, 6)                          # one query at N = 2500: K* inside the streamed kernel or not
GRAD_WIDTHS = (2, 3, 4, 5, 6, 7, 8)                  # batched variance gradient: DT = 3, 5, 8
GRAD_FALLBACK_WIDTHS = (9, 12)                       # beyond SR_GRAD_MAX_D: the per-row loop
GRAD_NS = (1, 130, 1000)
GRAD_TS = (2, 129, 1000)
GRAD_KERNELS = ("rbf", "mat52", "lin_rbf", "lin_mat52")

# covering designs: every width meets every kernel and every N of its group at least once (and every T, looped inside)
LIN_CASES = [(LIN_KERNELS[(i + j) % 3], D, N) for i, D in enumerate(LIN_WIDTHS) for j, N in enumerate(LIN_NS)]
BATCH_CASES = ([("rbf", D, N) for D in BATCH_WIDTHS for N in BATCH_NS] +
               [("lin_mat52", D, N) for D in BATCH_GENERAL_WIDTHS for N in BATCH_NS])


def _grad_ns(i):
    """N per kernel of the i-th gradient width: N = 1 (one training point) on a stationary kernel -- a linear part of D
    variances is not explained by one point --, the two others on the linear-product pair."""
    big = (130, 1000) if i % 2 == 0 else (1000, 130)
    stationary = (1, big[i // 2 % 2]) if i % 2 == 0 else (big[i // 2 % 2], 1)
    return dict(zip(GRAD_KERNELS, stationary + big))


GRAD_CASES = [(kt, D, _grad_ns(i)[kt], (1, 3)[(i + k) % 2]) for i, D in enumerate(GRAD_WIDTHS)
              for k, kt in enumerate(GRAD_KERNELS)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _seed(*key):
    """a fixed seed per case (crc32: the same in every process, unlike hash())"""
    return zlib.crc32("/".join(str(k) for k in key).encode())


def _setup(kt, D, N, n_out, tag):
    prob = width_problem(_seed(tag, kt, D, N, n_out), kt, D, N, n_out)
    return prob, width_oracle(prob), width_gp(prob)


def _kxx(om, x):
    return np.stack([orc.kernel_diag(kt, h, x) for kt, h in zip(om["kts"], om["hyp"])], axis=1)


def _scale(om, x):
    """the natural scale of d var / dx and d2 mu / dx2: sf2 / l_min^2.  sf2 is the signal variance of a stationary kernel;
    of lin_rbf / lin_mat52 the prior variance of the product part, v_prod v_stat x_1^2 (the linear part's share of the
    variance is explained by a few points and contributes little to either gradient)"""
    if om["kts"][0] in ("rbf", "mat52"):
        return float(np.max(om["signal_var"])) / om["l_min"] ** 2
    st = "rbf" if om["kts"][0] == "lin_rbf" else "mat52"
    vprod = max(float(np.asarray(h["prod.linear.variances"]).max()) * float(h["prod.%s.variance" % st]) for h in om["hyp"])
    return vprod * float(np.max(x[:, 1] ** 2)) / om["l_min"] ** 2


def _tol(om):
    general = om["kts"][0] != "rbf"
    if not general:
        at = mu_atol(om)
        return dict(mu=(1e-9, at), var=(0.0, 1e-9 * float(np.max(om["signal_var"]))), jm=(1e-9, 10 * at),
                    jv=(1e-9, 1e-11 * float(np.max(om["signal_var"])) / om["l_min"] ** 2), hm=(1e-8, 100 * at))
    scale = max(float(np.abs(om["beta"]).sum(0).max()), 1.0)
    return dict(mu=(1e-9, 1e-11 * scale), var=(0.0, 1e-8), jm=(1e-9, 1e-11 * scale), jv=(1e-7, 1e-9),
                hm=(1e-8, 1e-10 * scale))


def _close(name, got, ref, tol, msg=""):
    np.testing.assert_allclose(got, ref, rtol=tol[name][0], atol=tol[name][1], err_msg="%s %s" % (name, msg))


def _oracle_rows(om, x, rows, jac=True, extras=True):
    """mu, var (all rows); jac_mu, jac_var, hess_mu (the given rows)"""
    args = (om["Z"], om["beta"], om["inv_K"], om["kts"], om["hyp"])
    mu, var = orc.gp_predict_k(x, *args)
    jm = orc.gp_mean_jacobian_k(x[rows], om["Z"], om["beta"], om["kts"], om["hyp"]) if jac else None
    jv = hm = None
    if extras:
        ex = [orc.gp_linearize_extras_k(x[t], *args) for t in rows]
        jv, hm = np.array([e[0] for e in ex]), np.array([e[1] for e in ex])
    return mu, var, jm, jv, hm


def _assert_informative(om, x, var, jv=None, hm=None):
    """the data must make a wrong kernel visible: k* not ~0 (posterior variance well below the prior), gradients not ~0"""
    ratio = var / _kxx(om, x)
    assert np.median(ratio) < 0.5, "uninformative data: median var / k(x,x) = %.3f" % np.median(ratio)
    s = _scale(om, x)
    if jv is not None:
        assert np.abs(jv).max() >= 1e-3 * s, "uninformative data: max |jac_var| = %.3e, scale %.3e" % (np.abs(jv).max(), s)
    if hm is not None:
        assert np.abs(hm).max() >= 1e-3 * s, "uninformative data: max |hess_mu| = %.3e, scale %.3e" % (np.abs(hm).max(), s)


def _profiled(gp, fn):
    from safe_exploration_amd import _lib
    gp.prof_reset()
    gp.prof_enable(True)
    try:
        out = fn()
    finally:
        gp.prof_enable(False)
    names = ("K_SMALL", "K_KSTAR", "K_VAR", "K_FINAL")
    return out, {n: gp.prof_get(getattr(_lib, n))[1] for n in names}


def _np(outs):
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o) for o in outs)


# ------------------------------------------------------------------ single query, second order
def _lin_route(kt, D, Np):
    """launch counts of sr_gp_linearize with the default small path: K0 (one launch) where sr_gp_small_lin_wanted holds
    (Np <= 384 -- 512 only for T > 128 --, ARD-RBF up to D = 8, the general family up to D = 5), else the streamed
    route: one launch up to SR_LIN_FUSED_MAX_D (ARD-RBF), the columns pass in front of it beyond.  D = 9 .. 12 and general
    D = 6 .. 8 at Np = 256 fall off K0 onto the streamed route."""
    general = kt != "rbf"
    if Np <= 384 and D <= (K0_GENERAL_LIN_MAX_D if general else K0_MAX_D):
        return dict(K_SMALL=1, K_KSTAR=0, K_VAR=0, K_FINAL=0)
    fused = not general and D <= SR_LIN_FUSED_MAX_D
    return dict(K_SMALL=0, K_KSTAR=0 if fused else 1, K_VAR=1, K_FINAL=0)


@pytest.mark.parametrize("kt,D,N", LIN_CASES)
def test_single_query_second_order_widths(kt, D, N):
    """linearize_predict(jacobians=True) (the one-command route) and linearize_device (sr_gp_linearize) against the oracle
    on the default route and on the two-pass route (set_small_path(0): K1 -> K2 -> K3, U^-1 (U^-T k*), reduction); the
    DT-wide packed Hessian triangle mapped to D x D is checked where the mapping is not the identity (D != DT)."""
    n_out = 2
    prob, om, gp = _setup(kt, D, N, n_out, "lin")
    tol = _tol(om)
    expect = _lin_route(kt, D, gp._handle.Np)
    xs = width_queries(prob, 4, _seed("linq", kt, D, N))
    ref = _oracle_rows(om, xs, np.arange(len(xs)))
    _assert_informative(om, xs, ref[1], ref[3], ref[4])
    for q, x in enumerate(xs):
        rmu, rvar, rjm, rjv, rhm = (r[q:q + 1] for r in ref)
        routes = {}
        routes["host"], cnt = _profiled(gp, lambda: gp.linearize_predict(x[None, :D - 1], x[None, D - 1:], True))
        assert cnt == expect, "host route %s, expected %s" % (cnt, expect)
        out, cnt = _profiled(gp, lambda: gp.linearize_device(x))
        assert cnt == expect, "device route %s, expected %s" % (cnt, expect)
        routes["device"] = _np(out)
        gp.set_small_path(0)
        try:
            routes["two-pass"], cnt = _profiled(gp, lambda: gp.linearize_predict(x[None, :D - 1], x[None, D - 1:], True))
        finally:
            gp.set_small_path(1)
        assert cnt["K_SMALL"] == 0 and cnt["K_KSTAR"] == 1 and cnt["K_FINAL"] == 1, cnt
        for name, (mu, var, jm, jv, hm) in routes.items():
            msg = "%s query %d" % (name, q)
            _close("mu", np.reshape(mu, -1), rmu[0], tol, msg)
            _close("var", np.reshape(var, -1), rvar[0], tol, msg)
            _close("jm", jm, rjm[0], tol, msg)
            _close("jv", jv, rjv[0], tol, msg)
            _close("hm", hm, rhm[0], tol, msg)
            np.testing.assert_array_equal(hm, np.swapaxes(hm, 1, 2), err_msg=msg)
        # the two routes against each other at the bars of test_streamed_linearize_all_kernels
        scale = max(float(np.abs(om["beta"]).sum(0).max()), 1.0)
        for a_, b_, at in zip(routes["host"], routes["two-pass"], (1e-12 * scale, 1e-11, 1e-11 * scale, 1e-9, 1e-10 * scale)):
            np.testing.assert_allclose(a_, b_, rtol=1e-8, atol=at)


# ------------------------------------------------------------------ batched posterior
@pytest.mark.parametrize("kt,D,N", BATCH_CASES)
def test_batched_posterior_widths(kt, D, N):
    """predict(x, None, True) at every batch size of the list (streamed, balanced-share, 64- and 128-tile routes as the
    dispatch picks them), then once more with set_small_path(False) (plain tiles whatever the size)."""
    prob, om, gp = _setup(kt, D, N, 2, "batch")
    tol = _tol(om)
    x_all = width_queries(prob, sum(BATCH_TS), _seed("batchq", kt, D, N))
    rng = np.random.default_rng(D * N)
    rows_of = {}
    for T in BATCH_TS:
        rows_of[T] = np.arange(T) if T <= 64 or kt == "rbf" else np.sort(rng.choice(T, 64, replace=False))
    ref = {}
    t0 = 0
    for T in BATCH_TS:
        x = x_all[t0:t0 + T]
        t0 += T
        if kt == "rbf":
            rmu, rvar, rjm = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
        else:
            rmu, rvar, rjm, _, _ = _oracle_rows(om, x, rows_of[T], extras=False)
        ref[T] = (x, rmu, rvar, rjm)
    _assert_informative(om, x_all, np.concatenate([ref[T][2] for T in BATCH_TS]))
    for small in (True, False):
        gp.set_small_path(small)
        try:
            for T in BATCH_TS:
                x, rmu, rvar, rjm = ref[T]
                mu, var, jm = gp.predict(x, None, True)
                msg = "T=%d small_path=%s" % (T, small)
                _close("mu", mu, rmu, tol, msg)
                _close("var", var, rvar, tol, msg)
                _close("jm", jm[rows_of[T]], rjm, tol, msg)
        finally:
            gp.set_small_path(True)


@pytest.mark.parametrize("D", KSTAR2_WIDTHS)
def test_two_queries_per_thread_kstar_widths(D):
    """T = 8193 (8320 padded columns >= 8192): D <= 5 takes sr_kstar_kernel<5, 2, 2> -- two neighbouring queries per
    thread, the last pair half padding --, D = 6 the one-query kernel at DT = 8.  Every row against the oracle."""
    prob, om, gp = _setup("rbf", D, 700, 2, "kstar2")
    tol = _tol(om)
    x = width_queries(prob, 8193, _seed("kstar2q", D))
    rmu, rvar, rjm = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
    _assert_informative(om, x, rvar)
    (mu, var, jm), cnt = _profiled(gp, lambda: gp.predict(x, None, True))
    assert cnt["K_KSTAR"] == 1 and cnt["K_SMALL"] == 0, cnt
    _close("mu", mu, rmu, tol)
    _close("var", var, rvar, tol)
    _close("jm", jm, rjm, tol)
    _close("mu", mu[-1], rmu[-1], tol, "last (odd) query")
    _close("jm", jm[-1], rjm[-1], tol, "last (odd) query")


@pytest.mark.parametrize("D", STREAM_EDGE_WIDTHS)
def test_one_query_streamed_predict_width_edge(D):
    """ONE query at N = 2500: up to SR_STREAM_FUSED_MAX_D the streamed kernel evaluates its own K* column (no K* launch),
    beyond it a K* pass runs in front.  Through the one-command route (host query) and sr_gp_predict (device query)."""
    import torch
    prob, om, gp = _setup("rbf", D, 2500, 2, "edge")
    tol = _tol(om)
    x = width_queries(prob, 1, _seed("edgeq", D))
    rmu, rvar, rjm = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"])
    _assert_informative(om, x, rvar)
    expect = 0 if D <= SR_STREAM_FUSED_MAX_D else 1
    for name, fn in (("host", lambda: gp.predict(x, None, True)),
                     ("device", lambda: _np(gp.predict(torch.from_numpy(x).to(gp.device), None, True)))):
        (mu, var, jm), cnt = _profiled(gp, fn)
        assert cnt["K_KSTAR"] == expect and cnt["K_VAR"] == 1 and cnt["K_SMALL"] == 0, (name, cnt)
        _close("mu", mu, rmu, tol, name)
        _close("var", var, rvar, tol, name)
        _close("jm", jm, rjm, tol, name)


# ------------------------------------------------------------------ batched variance gradient
def _check_grad_model(prob, om, gp, Ts, seed):
    """predict_device_grad against the oracle (all rows up to T = 64, 64 sampled rows beyond), against predict, against
    the two other entry points of the same pass, and against linearize_device on 8 rows."""
    tol = _tol(om)
    general = om["kts"][0] != "rbf"
    rng = np.random.default_rng(seed)
    for T in Ts:
        x = width_queries(prob, T, seed + T)
        D = x.shape[1]
        mu, var, jm, jv = _np(gp.predict_device_grad(x))
        rows = np.arange(T) if T <= 64 else np.sort(rng.choice(T, 64, replace=False))
        rmu, rvar, rjm, rjv, _ = _oracle_rows(om, x, rows)
        _assert_informative(om, x, rvar, rjv)
        msg = "T=%d" % T
        _close("jv", jv[rows], rjv, tol, msg)
        _close("mu", mu, rmu, tol, msg)
        _close("var", var, rvar, tol, msg)
        _close("jm", jm[rows], rjm, tol, msg)
        # the plain posterior: the bars of test_predict_grad_oracle_rbf
        pmu, pvar, pjm = gp.predict(x, None, True)
        at = tol["mu"][1]
        np.testing.assert_allclose(mu, pmu, rtol=1e-10, atol=at, err_msg=msg)
        np.testing.assert_allclose(var, pvar, rtol=0, atol=tol["var"][1], err_msg=msg)
        np.testing.assert_allclose(jm, pjm, rtol=1e-9, atol=at, err_msg=msg)
        # predict(states, actions, True) and predictive_gradients(grad_sigma=True): the same pass, the same bits
        for a_, b_ in zip(gp.predict(x[:, :D - 1], x[:, D - 1:], True), (mu, var, jm, jv)):
            np.testing.assert_array_equal(a_, b_, err_msg=msg)
        gm, gv = gp.predictive_gradients(x, grad_sigma=True)
        np.testing.assert_array_equal(gm, jm, err_msg=msg)
        np.testing.assert_array_equal(gv, jv, err_msg=msg)
        # the single-query route on 8 rows.  ARD-RBF: the bar of test_predict_grad_matches_single_query_route (d var / dx
        # is a sum of terms of size sf2 |z_i - x| / l^2 that cancel: the routes sum them in different orders, so an entry
        # near zero may differ by ulps of the terms); the general family: its oracle bar
        jt = (1e-10, 1e-12 * float(np.max(om["signal_var"])) / om["l_min"] ** 2) if not general else tol["jv"]
        for t in rows[:8]:
            ljv = gp.linearize_device(x[t])[3].cpu().numpy()
            np.testing.assert_allclose(jv[t], ljv, rtol=jt[0], atol=jt[1], err_msg="%s row %d vs linearize" % (msg, t))


@pytest.mark.parametrize("kt,D,N,n_out", GRAD_CASES)
def test_predict_grad_widths(kt, D, N, n_out):
    """sr_gp_predict_grad at DT = 3, 5 and 8 (the D = 6 .. 8 instantiation: launch_bounds(256, 1), the j < D masking of
    the padded columns) for all four kernel types, one training point to 1000, one output or three."""
    prob, om, gp = _setup(kt, D, N, n_out, "grad")
    _check_grad_model(prob, om, gp, GRAD_TS, _seed("gradq", kt, D, N))


@pytest.mark.parametrize("kt", ["rbf", "lin_mat52"])
def test_predict_grad_central_differences_widest(kt):
    """d var / dx at D = 8 (DT = 8) against central differences of the batched variance."""
    D, T = 8, 64
    prob, om, gp = _setup(kt, D, 1000, 2, "gradfd")
    x = width_queries(prob, T, 11)
    jv = gp.predict_device_grad(x)[3].cpu().numpy()
    _assert_informative(om, x, orc.gp_predict_k(x, om["Z"], om["beta"], om["inv_K"], om["kts"], om["hyp"])[1], jv)
    fd = np.empty_like(jv)
    h = 1e-5 * om["l_min"]
    for j in range(D):
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        fd[:, :, j] = (gp.predict(xp)[1] - gp.predict(xm)[1]) / (2 * h)
    np.testing.assert_allclose(jv, fd, rtol=1e-6, atol=1e-6 * np.abs(jv).max())


@pytest.mark.parametrize("kt,D", [("rbf", 9), ("mat52", 12)])
def test_predict_grad_beyond_compiled_widths(kt, D, monkeypatch):
    """D > SR_GRAD_MAX_D: sr_gp_predict_grad refuses with its error; predict(states, actions, True) linearises row by row
    (exactly one _linearize_host per row) and still matches the oracle."""
    from safe_exploration_amd import SimpleGPModel
    T = 5
    prob, om, gp = _setup(kt, D, 500, 2, "gradwide")
    assert D in GRAD_FALLBACK_WIDTHS and D > SR_GRAD_MAX_D
    x = width_queries(prob, T, 12)
    with pytest.raises(NotImplementedError, match=r"D=%d > %d" % (D, SR_GRAD_MAX_D)):
        gp.predict_device_grad(x)
    calls = []
    orig = SimpleGPModel._linearize_host

    def counted(self, xq):
        calls.append(1)
        return orig(self, xq)

    monkeypatch.setattr(SimpleGPModel, "_linearize_host", counted)
    mu, var, jm, jv = gp.predict(x[:, :D - 1], x[:, D - 1:], True)
    assert len(calls) == T
    rmu, rvar, rjm, rjv, _ = _oracle_rows(om, x, np.arange(T))
    _assert_informative(om, x, rvar, rjv)
    tol = _tol(om)
    for name, got, ref in (("mu", mu, rmu), ("var", var, rvar), ("jm", jm, rjm), ("jv", jv, rjv)):
        _close(name, got, ref, tol)


# ------------------------------------------------------------------ more outputs than factorisation slots
@pytest.mark.parametrize("kt,n_out,N", [("rbf", 9, 700), ("mat52", 17, 400)])
def test_many_outputs_at_width_six(kt, n_out, N):
    """n_out > SR_FACT_SLOTS (8) at D = 6 (DT = 8): batched posterior, single-query second order and the batched
    variance gradient against the oracle."""
    D = 6
    prob, om, gp = _setup(kt, D, N, n_out, "many")
    tol = _tol(om)
    x = width_queries(prob, 40, 13)
    rmu, rvar, rjm, _, _ = _oracle_rows(om, x, np.arange(40), extras=False)
    mu, var, jm = gp.predict(x, None, True)
    _close("mu", mu, rmu, tol)
    _close("var", var, rvar, tol)
    _close("jm", jm, rjm, tol)
    for t in (0, 1):
        _, _, _, rjv, rhm = _oracle_rows(om, x[t:t + 1], [0])
        _assert_informative(om, x[t:t + 1], rvar[t:t + 1], rjv, rhm)
        lmu, lvar, ljm, ljv, lhm = gp.linearize_predict(x[t:t + 1, :D - 1], x[t:t + 1, D - 1:], True)
        _close("mu", lmu[:, 0], rmu[t], tol)
        _close("var", lvar[:, 0], rvar[t], tol)
        _close("jm", ljm, rjm[t], tol)
        _close("jv", ljv, rjv[0], tol)
        _close("hm", lhm, rhm[0], tol)
        np.testing.assert_array_equal(lhm, np.swapaxes(lhm, 1, 2))
    _check_grad_model(prob, om, gp, (2, 129), 14)
