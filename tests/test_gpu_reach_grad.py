"""The reverse pass of one reachability step on the device (sr_ellipsoid_step_vjp, sr_onestep_reach_vjp) and the autograd
surface over it, against the long-double reference tests/_ellipsoid_grad_ref.py.

1. sr_ellipsoid_step_vjp at all 32 (n_s, n_u) instances x every family of _ellipsoid_ref.cases, both branches, T = 257, into
   sentinel-filled outputs.  Bars (stated once in _ellipsoid_grad_ref): per output array 30 x SHARE x EPS x abs-scale x
   max(1, 1/g), SHARE the measured floor of a plain fp64 restatement (p_bar 1.0, kff_bar 1.3, mu_bar 0 -- a copy --, var_bar 9.6,
   q_bar 4.5, kfb_bar 202, jac_bar 1.2).  Queries with g < 1e-3 are left out of the value bars (at most 2 % of a case, asserted);
   the families that tie by construction (identity, twin_top, all_equal) are held to finite outputs, a symmetric q_bar and the
   bars of what does not pass through r^2 (p_bar, kff_bar, mu_bar; var_bar in the point branch).  tiny and huge are in.
   In the point branch var_bar = n_s c^2 G_ii is three roundings away from the long-double value rounded to fp64: held to
   POINT_VAR_ULPS = 4 eps of its own magnitude in every family (bitwise equality with a long-double reference is not defined).
2. sr_onestep_reach_vjp on fitted models -- (n_out, D) = (2, 3) rbf at N = 150 and 600, (4, 5) rbf, (2, 3) lin_mat52, the
   cart-pole shape with an input transform (3 x 4, D = 4), one sparse handle -- against the reference composed in long double
   with the device's OWN linearize_device_batch outputs at z, so that only the new kernels' rounding is under test.  The link
   adds dot products of the seeds on (mu, var, jac), whose own bars are the shares above: the composed p_bar and kff_bar are
   held to 30 x the largest of those shares (var_bar: 9.6) of their composed abs-scale.  Same bits with set_chunk(64), and with
   chunks of 64 / 1000 / the default at N = 2000, T = 1500, where the linearisation's split counts DO depend on the width of a
   pass (64 splits of the K* pass at 1500 queries, 128 at 64) unless the entry point bounds its passes; NaN in every output of
   a query with q = 0 (ellipsoid branch, through the GP link), nothing else touched; NotImplementedError at D = 9.
3. The autograd surface: differentiable=True returns the bits of the plain call, torch.autograd.grad equals the wrapper's VJP
   to the bit, and the gradient of a random linear functional of a differentiable H = 3 roll-out of 33 trajectories (both
   starts) equals the reverse sweep of the reference, step by step, on the device's own per-step linearisations.  Its bar is
   relative to the largest element of each gradient: PROP_RTOL = 30 x the disagreement of two CPU routes to that gradient (the
   sweep in long double and in fp64).  The values of the roll-out equal the forward's per-step route (set_chain(False)) to the bit;
   at n_s = 2, where a one-step call of a small model is one launch of its own, to the bit with set_chain(False) around the
   differentiable roll-out as well, and without it to the bars test_gpu_parity holds the one-launch kernel to against the per-step
   route (p: rtol 1e-8, atol 1e-11; q: rtol 1e-7, atol 1e-14).
4. examples/safe_shooting_gradient.py runs and its loss goes down.

Observed on MI355X, as shares of the bars: sr_ellipsoid_step_vjp p_bar 0.072, kff_bar 0.045, mu_bar exact, var_bar 0.133 (4x3
graded), q_bar 0.055, kfb_bar 0.105 (8x1 graded), jac_bar 0.058, var_bar of the point branch within its 4 eps; sr_onestep_reach_vjp at most 0.013 (q_bar, lin_mat52), p_bar and
kff_bar at most 0.007; propagated gradients: device 1.7e-16 .. 7.8e-16 of the largest element, the two CPU
routes 1.3e-16 .. 1.54e-15 (d/dk_fb_init), bar 4.8e-14.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ellipsoid_ref as R
import _ellipsoid_grad_ref as G
from _helpers import width_problem, width_gp

pytestmark = pytest.mark.gpu
LD = np.longdouble
T = R.T_CASE
SENTINEL = -7.25e+300
INSTANCES = [(n_s, n_u) for n_s in range(1, 9) for n_u in range(1, 5)]
LINK_SHARE = max(G.SHARE[k] for k in ("p_bar", "kff_bar", "mu_bar", "var_bar", "jac_bar"))
POINT_VAR_ULPS = 4.0
PROP_RTOL = 30 * 1.6e-15          # two CPU routes (long double / fp64 sweep) disagree by at most 1.54e-15 of the largest element
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _dev():
    import torch
    return torch.device("cuda:0")


def _t(x):
    import torch
    return None if x is None else torch.tensor(np.ascontiguousarray(x, dtype=np.float64), device=_dev())


def _step_vjp_device(case, branch, pb, qb, lin=True):
    """sr_ellipsoid_step_vjp through the C ABI into sentinel-filled outputs: dict name -> array"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    Tn, n_s = case["p"].shape
    n_u = case["k_ff"].shape[1]
    ell = branch == "ell"
    a = case["a"] if lin else np.eye(n_s)
    b = case["b"] if lin else np.zeros((n_s, n_u))
    ins = [_t(case["p"]), _t(case["q"]) if ell else None, _t(case["k_ff"]), _t(case["k_fb"]) if ell else None, _t(case["mu"]),
           _t(case["var"]), _t(case["jac"]) if ell else None, _t(a), _t(b), _t(case["l_mu"]), _t(case["l_sigma"])]
    shapes = dict(p_bar=(Tn, n_s), q_bar=(Tn, n_s, n_s), kff_bar=(Tn, n_u), kfb_bar=(Tn, n_u, n_s), mu_bar=(Tn, n_s),
                  var_bar=(Tn, n_s), jac_bar=(Tn, n_s, n_s + n_u))
    outs = {k: torch.full(s, SENTINEL, dtype=torch.float64, device=_dev()) for k, s in shapes.items()}
    tpb, tqb = _t(pb), _t(qb)                             # (held until the copies below have synchronised)
    check(lib.sr_ellipsoid_step_vjp(0, Tn, n_s, n_u, *[B.ptr(x) for x in ins], float(case["c"]), B.ptr(tpb), B.ptr(tqb),
                                    *[B.ptr(outs[k]) for k in G.OUTPUTS], B.stream_ptr(_dev())))
    return {k: v.cpu().numpy() for k, v in outs.items()}


_REF = {}


def _reference(inst, fam, branch):
    """computed once per case, shared, left unchanged"""
    key = (inst, fam, branch)
    if key not in _REF:
        case = R.cases(*inst)[fam]
        pb, qb = G.seeds(case)
        _REF[key] = G.vjp_batch(case, branch, pb, qb)
    return _REF[key]


def _compare(tag, got, ref, names, keep):
    worst = {}
    for name in names:
        used = G.share_used(got[name][keep], ref[name][keep], ref[name + "_abs"][keep], ref["g"][keep])
        worst[name] = used / G.bar(name) if G.bar(name) > 0 else (0.0 if used == 0 else np.inf)
    print("%s: share of the bar used %s" % (tag, {k: "%.3f" % v for k, v in worst.items()}))
    return worst


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda i: "%dx%d" % i)
def test_ellipsoid_step_vjp_against_the_long_double_reference(inst):
    cases = R.cases(*inst)
    failures = []
    for fam in R.families(inst[0]):
        case = cases[fam]
        pb, qb = G.seeds(case)
        for branch in ("ell", "point"):
            got = _step_vjp_device(case, branch, pb, qb)
            ref = _reference(inst, fam, branch)
            assert not ref["bad"].any()
            written = G.OUTPUTS
            for name in written:
                assert np.isfinite(got[name]).all() and not (got[name] == SENTINEL).any(), (fam, branch, name)
            assert np.array_equal(got["q_bar"], got["q_bar"].transpose(0, 2, 1)), (fam, branch)
            if branch == "point":
                assert not got["q_bar"].any() and not got["kfb_bar"].any() and not got["jac_bar"].any()
            if fam in G.TIE_FAMILIES:
                names = ("p_bar", "kff_bar", "mu_bar") + (("var_bar",) if branch == "point" else ())
                keep = np.ones(T, dtype=bool)
            else:
                names = G.OUTPUTS
                keep = ref["g"] >= G.G_MIN
                assert (~keep).sum() <= 0.02 * T, (fam, branch, int((~keep).sum()))
            worst = _compare("%dx%d %s %s" % (inst + (fam, branch)), got, ref, names, keep)
            failures += [(fam, branch, k, v) for k, v in worst.items() if not v <= 1.0]
            if branch == "point":
                ulps = G.share_used(got["var_bar"], ref["var_bar"], np.abs(ref["var_bar"]), np.ones(T))
                failures += [(fam, branch, "var_bar ulps", ulps)] if not ulps <= POINT_VAR_ULPS else []
    assert not failures, failures


def test_conventions_on_the_device():
    """NULL seed = zero seed to the bit; only the symmetric part of q1_bar counts; a = b = None; NaN for a query with var = 0 in
    the point branch and for a query with q = 0 in the ellipsoid branch; every other query keeps its bits"""
    inst = (3, 2)
    case = R.cases(*inst)["rounded"]
    pb, qb = G.seeds(case)
    for branch in ("ell", "point"):
        full = _step_vjp_device(case, branch, pb, qb)
        for null, zero in (((None, qb), (np.zeros_like(pb), qb)), ((pb, None), (pb, np.zeros_like(qb)))):
            x, y = _step_vjp_device(case, branch, *null), _step_vjp_device(case, branch, *zero)
            assert all(np.array_equal(x[k], y[k]) for k in G.OUTPUTS), branch
        sym = _step_vjp_device(case, branch, pb, (qb + qb.transpose(0, 2, 1)) / 2)
        ref = _reference(inst, "rounded", branch)
        for k in G.OUTPUTS:
            assert np.all(np.abs(sym[k] - full[k]) <= 4 * G.EPS * ref[k + "_abs"] * G.gap_factor(ref["g"]).reshape(
                (-1,) + (1,) * (full[k].ndim - 1))), (branch, k)
        nolin = _step_vjp_device(case, branch, pb, qb, lin=False)
        rows = range(0, T, 16)
        ref0 = G.vjp_batch(case, branch, pb, qb, lin=False, rows=rows)
        sel = {k: v[::16] for k, v in nolin.items()}
        worst = _compare("a=b=None %s" % branch, sel, ref0, G.OUTPUTS, ref0["g"] >= G.G_MIN)
        assert all(v <= 1.0 for v in worst.values()), worst
        bad_case = dict(case, var=case["var"].copy(), q=case["q"].copy())
        bad_case["var"][5, 0] = 0.0
        bad_case["q"][7] = 0.0
        got = _step_vjp_device(bad_case, branch, pb, qb)
        others = (np.arange(T) != 5) & (np.arange(T) != 7 if branch == "ell" else True)
        for k in G.OUTPUTS:
            if branch == "point":                       # c sqrt(0) is not > 0
                assert np.isnan(got[k][5]).all(), k
            else:                                       # q = 0: r^2 = 0, l_mu r^2 is not > 0 -> the query is NaN throughout
                assert np.isnan(got[k][7]).all(), k
                # var = 0 is no violation there (c l_sigma r > 0), but d sqrt(var) / d var is infinite: var_bar_0 is not
                # finite, every other output of the query is
                if k == "var_bar":
                    assert not np.isfinite(got[k][5, 0]) and np.isfinite(got[k][5, 1:]).all()
                else:
                    assert np.isfinite(got[k][5]).all(), k
            assert np.array_equal(got[k][others], full[k][others]), (branch, k)
    import torch
    from safe_exploration_amd import gp_reachability as reach
    with pytest.raises(ValueError):
        reach.ellipsoid_step_vjp_batch(_t(case["p"]), _t(case["k_ff"]), _t(case["mu"]), _t(case["var"]), None, case["l_mu"],
                                       case["l_sigma"])
    # the wrapper: NumPy in, NumPy out, the same bits as the C ABI
    outs = reach.ellipsoid_step_vjp_batch(case["p"], case["k_ff"], case["mu"], case["var"], case["jac"], case["l_mu"],
                                          case["l_sigma"], pb, qb, case["q"], case["k_fb"], case["c"], case["a"], case["b"])
    full = _step_vjp_device(case, "ell", pb, qb)
    assert all(isinstance(o, np.ndarray) and np.array_equal(o, full[k]) for o, k in zip(outs, G.OUTPUTS))
    assert torch.cuda.is_available()


# ---- 2. sr_onestep_reach_vjp on fitted models ---------------------------------------------------------------------------------
def _gp_model(spec):
    kind, kt, n_out, D, N = spec
    if kind == "sparse":
        import _sparse_ref as S
        from test_gpu_sparse_gp import _sparse_model
        return _sparse_model(S.make_case(5, kt, n_out, D, 96, N))
    return width_gp(width_problem(4000 + N + D, kt, D, N, n_out))


MODELS = [("exact", "rbf", 2, 3, 150), ("exact", "rbf", 2, 3, 600), ("exact", "rbf", 4, 5, 150), ("exact", "lin_mat52", 2, 3, 150),
          ("cartpole", "rbf", 4, 4, 150), ("sparse", "rbf", 2, 3, 3000)]


def _reach_inputs(n_s, n_u, Tn, seed):
    rng = np.random.default_rng([seed, n_s, n_u, Tn])
    A = rng.standard_normal((Tn, n_s, n_s))
    return dict(p=0.3 * rng.standard_normal((Tn, n_s)), k_ff=0.2 * rng.standard_normal((Tn, n_u)),
                q=0.02 * np.einsum('tij,tkj->tik', A, A) / n_s, k_fb=0.3 * rng.standard_normal((Tn, n_u, n_s)),
                a=0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
                l_mu=rng.uniform(0.01, 0.05, n_s), l_sigma=rng.uniform(0.01, 0.05, n_s), c=R.C_SAFETY,
                pb=rng.standard_normal((Tn, n_s)), qb=rng.standard_normal((Tn, n_s, n_s)))


def _composed_reference(x, lin, tz, branch, pb, qb, fp64=False, rows=None):
    """_ellipsoid_grad_ref.step_vjp composed with linearisations (mu, var, jac_mu, jac_var, hess_mu at z = [tz p; k_ff]) that the
    caller supplies: p_bar, q_bar, kff_bar, kfb_bar with their abs-scales, per query, in long double (fp64: the restatement)"""
    dt = np.float64 if fp64 else LD
    mu, var, jm, jv, hm = lin
    Tn, n_s = x["p"].shape
    n_u = x["k_ff"].shape[1]
    tzm = np.eye(n_s, dtype=dt) if tz is None else np.asarray(tz, dtype=dt)
    nx = tzm.shape[0]
    res = {k: [] for k in ("p_bar", "q_bar", "kff_bar", "kfb_bar", "p_bar_abs", "q_bar_abs", "kff_bar_abs", "kfb_bar_abs", "g")}
    for t in (range(Tn) if rows is None else rows):
        jmt, jvt, hmt = jm[t].astype(dt), jv[t].astype(dt), hm[t].astype(dt)
        jac_s = np.hstack((jmt[:, :nx].dot(tzm), jmt[:, nx:]))
        o = G.step_vjp(x["p"][t], x["q"][t] if branch == "ell" else None, x["k_ff"][t], x["k_fb"][t], mu[t], var[t], jac_s,
                       x["l_mu"], x["l_sigma"], x["c"], x["a"], x["b"], None if pb is None else pb[t],
                       None if qb is None else qb[t], fp64=fp64)
        jz = np.hstack((o["jac_bar"][:, :n_s].dot(tzm.T), o["jac_bar"][:, n_s:]))
        jz_abs = np.hstack((o["jac_bar_abs"][:, :n_s].dot(np.abs(tzm).T), o["jac_bar_abs"][:, n_s:]))
        zb = jmt.T.dot(o["mu_bar"]) + jvt.T.dot(o["var_bar"]) + np.einsum('ad,ade->e', jz, hmt)
        zb_abs = np.abs(jmt).T.dot(o["mu_bar_abs"]) + np.abs(jvt).T.dot(o["var_bar_abs"]) + np.einsum('ad,ade->e', jz_abs, np.abs(hmt))
        res["p_bar"].append(o["p_bar"] + tzm.T.dot(zb[:nx]))
        res["p_bar_abs"].append(o["p_bar_abs"] + np.abs(tzm).T.dot(zb_abs[:nx]))
        res["kff_bar"].append(o["kff_bar"] + zb[nx:])
        res["kff_bar_abs"].append(o["kff_bar_abs"] + zb_abs[nx:])
        for k in ("q_bar", "kfb_bar", "q_bar_abs", "kfb_bar_abs", "g"):
            res[k].append(o[k])
    return {k: np.array(v).astype(np.float64) for k, v in res.items()}


def _z(x, tz):
    px = x["p"] if tz is None else x["p"].dot(np.asarray(tz).T)
    return np.hstack((px, x["k_ff"]))


@pytest.mark.parametrize("spec", MODELS, ids=lambda s: "%s-%s-%dx%d-N%d" % s)
def test_onestep_reach_vjp_on_fitted_models(spec):
    from safe_exploration_amd import gp_reachability as reach
    gp = _gp_model(spec)
    n_s = spec[2]
    tz = np.eye(4)[1:] if spec[0] == "cartpole" else None          # the cart position is not a GP input (exact in fp64)
    n_u = spec[3] - (3 if tz is not None else n_s)
    x = _reach_inputs(n_s, n_u, T, 11)
    lin = tuple(o.cpu().numpy() for o in gp.linearize_device_batch(_z(x, tz)))
    for branch in ("ell", "point"):
        ell = branch == "ell"
        call = lambda: reach.onestep_reachability_vjp_batch(x["p"], gp, x["k_ff"], x["l_mu"], x["l_sigma"], x["pb"], x["qb"],
                                                            x["q"] if ell else None, x["k_fb"] if ell else None, x["c"], x["a"],
                                                            x["b"], t_z_gp=tz)
        got = call()
        ref = _composed_reference(x, lin, tz, branch, x["pb"], x["qb"])
        names = ("p_bar", "q_bar", "kff_bar", "kfb_bar") if ell else ("p_bar", "kff_bar")
        if not ell:
            assert got[1] is None and got[3] is None
        keep = ref["g"] >= G.G_MIN
        assert (~keep).sum() <= 0.02 * T
        worst = {}
        for name, arr in zip(("p_bar", "q_bar", "kff_bar", "kfb_bar"), got):
            if name not in names:
                continue
            assert np.isfinite(arr).all(), name
            share = LINK_SHARE if name in ("p_bar", "kff_bar") else G.SHARE[name]
            worst[name] = G.share_used(arr[keep], ref[name][keep], ref[name + "_abs"][keep], ref["g"][keep]) / (G.FACTOR * share)
        print("%s %s: share of the bar used %s" % (spec, branch, {k: "%.3f" % v for k, v in worst.items()}))
        assert all(v <= 1.0 for v in worst.values()), worst
        if ell:
            assert np.array_equal(got[1], got[1].transpose(0, 2, 1))
        gp.set_chunk(64)
        try:
            chunked = call()
        finally:
            gp.set_chunk(65536)
        assert all(a is b or np.array_equal(a, b) for a, b in zip(got, chunked)), "chunking changed the bits"


def test_onestep_reach_vjp_chunks_and_bad_queries_at_a_size_where_the_passes_matter():
    """N = 2000, n_out = 2, T = 1500: sr_gp_linearize_batch on all 1500 queries at once splits the K* pass 64 ways, on 64 queries
    128 ways (pick_nsplit) -- other bits.  sr_onestep_reach_vjp bounds its passes at 768 queries here, where the split counts
    are those of the model size (128, and 63 of the Hessian pass), so every chunk size gives the same bits.  And a query with
    q = 0 is NaN in all four outputs, through the GP link too, and nothing else moves."""
    from safe_exploration_amd import gp_reachability as reach
    gp = width_gp(width_problem(4242, "rbf", 3, 2000, 2))
    Tn = 1500
    x = _reach_inputs(2, 1, Tn, 17)
    for ell in (True, False):
        call = lambda q=x["q"]: reach.onestep_reachability_vjp_batch(x["p"], gp, x["k_ff"], x["l_mu"], x["l_sigma"], x["pb"],
                                                                    x["qb"], q if ell else None, x["k_fb"] if ell else None,
                                                                    x["c"], x["a"], x["b"])
        whole = call()
        assert all(o is None or np.isfinite(o).all() for o in whole)
        try:
            for chunk in (64, 1000):
                gp.set_chunk(chunk)
                parts = call()
                assert all(a is b or np.array_equal(a, b) for a, b in zip(whole, parts)), "chunk %d changed the bits" % chunk
        finally:
            gp.set_chunk(65536)
        if ell:
            q_bad = x["q"].copy()
            q_bad[9] = 0.0
            got = call(q_bad)
            others = np.arange(Tn) != 9
            for a, b in zip(got, whole):
                assert np.isnan(a[9]).all() and np.array_equal(a[others], b[others])


def test_differentiable_multistep_values_at_two_states():
    """n_s = 2: a one-step call of a small model is one launch of its own (posterior and step), the forward roll-out with
    set_chain(False) is per-step launches.  With set_chain(False) around the differentiable roll-out too its steps take the
    per-step launches and the values are equal to the bit; without, the two routes of the posterior agree to rounding."""
    import torch
    from safe_exploration_amd import gp_reachability as reach
    gp = _gp_model(MODELS[0])
    n_s, n_u, Tn, H = 2, 1, 33, 3
    x = _reach_inputs(n_s, n_u, Tn, 23)
    rng = np.random.default_rng(9)
    k_ff, k_fb = _t(0.2 * rng.standard_normal((Tn, H, n_u))), _t(0.3 * rng.standard_normal((Tn, H - 1, n_u, n_s)))
    p_0 = _t(x["p"]).requires_grad_(True)
    roll = lambda diff: reach.multistep_reachability_batch(p_0 if diff else p_0.detach(), gp, k_fb, k_ff, x["l_mu"], x["l_sigma"],
                                                           None, x["c"], x["a"], x["b"], differentiable=diff)
    fused = roll(True)
    gp.set_chain(False)
    try:
        fwd, per_step = roll(False), roll(True)
    finally:
        gp.set_chain(True)
    assert torch.equal(per_step[0], fwd[0]) and torch.equal(per_step[1], fwd[1])
    assert per_step[0].requires_grad and fused[0].requires_grad
    # the bars test_gpu_parity holds the one-launch chain kernel to against the per-step route
    np.testing.assert_allclose(fused[0].detach().cpu().numpy(), fwd[0].cpu().numpy(), rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fused[1].detach().cpu().numpy(), fwd[1].cpu().numpy(), rtol=1e-7, atol=1e-14)


def test_onestep_reach_vjp_refusals():
    from safe_exploration_amd import gp_reachability as reach, _buffers as B
    from safe_exploration_amd._lib import lib, SR_EINVAL
    gp9 = width_gp(width_problem(77, "rbf", 9, 60, 8))           # n_s = 8, n_u = 1, D = 9
    x = _reach_inputs(8, 1, 4, 3)
    with pytest.raises(NotImplementedError):
        reach.onestep_reachability_vjp_batch(x["p"], gp9, x["k_ff"], x["l_mu"], x["l_sigma"], x["pb"], None, None, None, x["c"])
    gp = _gp_model(MODELS[0])
    hd, s = gp._handle, B.stream_ptr(gp._handle.device)
    x = _reach_inputs(2, 1, 4, 3)
    d = {k: _t(v) for k, v in x.items() if isinstance(v, np.ndarray)}
    o = [B.empty((4, 2), hd.device), B.empty((4, 2, 2), hd.device), B.empty((4, 1), hd.device), B.empty((4, 1, 2), hd.device)]
    P = B.ptr
    args = lambda q, kfb, pb, qb, T_=4: (hd.h, T_, P(d["p"]), q, P(d["k_ff"]), kfb, P(d["a"]), P(d["b"]), P(d["l_mu"]),
                                        P(d["l_sigma"]), 1.7, pb, qb, P(o[0]), P(o[1]), P(o[2]), P(o[3]), s)
    assert lib.sr_onestep_reach_vjp(*args(P(d["q"]), None, P(d["pb"]), P(d["qb"]))) == SR_EINVAL       # q without k_fb
    assert lib.sr_onestep_reach_vjp(*args(P(d["q"]), P(d["k_fb"]), None, None)) == SR_EINVAL          # both seeds NULL
    assert lib.sr_onestep_reach_vjp(*args(None, None, None, None, T_=0)) == 0                          # T = 0: a no-op


# ---- 3. the autograd surface --------------------------------------------------------------------------------------------------
def test_differentiable_onestep_is_the_plain_call_and_its_vjp():
    import torch
    from safe_exploration_amd import gp_reachability as reach
    for spec in (MODELS[0], MODELS[4]):
        gp = _gp_model(spec)
        n_s = spec[2]
        tz = np.eye(4)[1:] if spec[0] == "cartpole" else None
        n_u = spec[3] - (3 if tz is not None else n_s)
        x = _reach_inputs(n_s, n_u, 33, 5)
        for ell in (True, False):
            ins = [_t(x["p"]).requires_grad_(True), _t(x["q"]).requires_grad_(True) if ell else None,
                   _t(x["k_ff"]).requires_grad_(True), _t(x["k_fb"]).requires_grad_(True) if ell else None]
            kw = dict(c_safety=x["c"], a=x["a"], b=x["b"], t_z_gp=tz)
            plain = reach.onestep_reachability_batch(ins[0].detach(), gp, ins[2].detach(), x["l_mu"], x["l_sigma"],
                                                     None if not ell else ins[1].detach(), None if not ell else ins[3].detach(), **kw)
            diff = reach.onestep_reachability_batch(ins[0], gp, ins[2], x["l_mu"], x["l_sigma"], ins[1], ins[3],
                                                    differentiable=True, **kw)
            assert all(torch.equal(u, v) for u, v in zip(plain, diff))
            assert diff[0].requires_grad and diff[1].requires_grad
            pb, qb = _t(x["pb"]), _t(x["qb"])
            wanted = [t for t in ins if t is not None]
            grads = torch.autograd.grad((diff[0] * pb).sum() + (diff[1] * qb).sum(), wanted)
            vjp = reach.onestep_reachability_vjp_batch(ins[0].detach(), gp, ins[2].detach(), x["l_mu"], x["l_sigma"], pb, qb,
                                                       None if not ell else ins[1].detach(), None if not ell else ins[3].detach(),
                                                       x["c"], x["a"], x["b"], tz)
            assert all(torch.equal(u, v) for u, v in zip(grads, [v for v in vjp if v is not None]))
    # ellipsoid_step_batch(differentiable=True): gradients also reach mu, var, jac
    case = R.cases(3, 2)["random"]
    pb, qb = G.seeds(case)
    ts = {k: _t(case[k]).requires_grad_(True) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
    kw = dict(c_safety=case["c"], a=case["a"], b=case["b"])
    plain = reach.ellipsoid_step_batch(*[ts[k].detach() for k in ("p", "k_ff", "mu", "var", "jac")], case["l_mu"], case["l_sigma"],
                                       ts["q"].detach(), ts["k_fb"].detach(), **kw)
    diff = reach.ellipsoid_step_batch(*[ts[k] for k in ("p", "k_ff", "mu", "var", "jac")], case["l_mu"], case["l_sigma"], ts["q"],
                                      ts["k_fb"], differentiable=True, **kw)
    assert all(torch.equal(u, v) for u, v in zip(plain, diff))
    order = ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")
    grads = torch.autograd.grad((diff[0] * _t(pb)).sum() + (diff[1] * _t(qb)).sum(), [ts[k] for k in order])
    full = _step_vjp_device(case, "ell", pb, qb)
    assert all(np.array_equal(g.cpu().numpy(), full[k]) for g, k in zip(grads, G.OUTPUTS))


def _sweep_reference(x, H, lins, states, tz, w_p, w_q, k_ff, k_fb, start_q, fp64):
    """reverse sweep over H steps, one trajectory set: the gradient of sum w_p . p_all + w_q . q_all in p_0, (q_0, k_fb_init),
    k_ff and k_fb, from the reference VJP of every step at the device's own states and linearisations"""
    Tn, n_s = x["p"].shape
    n_u = k_ff.shape[2]
    dt = np.float64 if fp64 else LD
    p_bar, q_bar = np.zeros((Tn, n_s), dtype=dt), np.zeros((Tn, n_s, n_s), dtype=dt)
    g_kff, g_kfb = np.zeros((Tn, H, n_u), dtype=dt), np.zeros((Tn, max(H - 1, 0), n_u, n_s), dtype=dt)
    g_kfb0 = None
    for i in range(H - 1, -1, -1):
        p_in, q_in = states[i]
        ell = q_in is not None
        kfb_i = (x["k_fb"] if start_q else None) if i == 0 else k_fb[:, i - 1]
        xi = dict(x, p=p_in, q=q_in, k_ff=k_ff[:, i], k_fb=kfb_i if ell else np.zeros((Tn, n_u, n_s)))
        seeds_p, seeds_q = p_bar + w_p[:, i], q_bar + w_q[:, i]
        out = _composed_reference(xi, lins[i], tz, "ell" if ell else "point", seeds_p, seeds_q, fp64=fp64)
        # (the composed reference rounds its results to fp64; at 30 x 1e-13 that is invisible)
        p_bar, g_kff[:, i] = out["p_bar"], out["kff_bar"]
        if ell:
            q_bar = out["q_bar"]
            if i == 0:
                g_kfb0 = out["kfb_bar"]
            else:
                g_kfb[:, i - 1] = out["kfb_bar"]
    return dict(p_0=p_bar.astype(np.float64), q_0=q_bar.astype(np.float64) if start_q else None, k_fb_init=g_kfb0,
                k_ff=g_kff.astype(np.float64), k_fb=g_kfb.astype(np.float64))


@pytest.mark.parametrize("start_q", (False, True), ids=("from_a_point", "from_q0"))
def test_differentiable_multistep(start_q):
    import torch
    from safe_exploration_amd import gp_reachability as reach
    gp = _gp_model(MODELS[2])                                         # (4, 5) rbf: one step takes the per-step route itself
    n_s, n_u, Tn, H = 4, 1, 33, 3
    x = _reach_inputs(n_s, n_u, Tn, 21)
    rng = np.random.default_rng(8)
    k_ff, k_fb = 0.2 * rng.standard_normal((Tn, H, n_u)), 0.3 * rng.standard_normal((Tn, H - 1, n_u, n_s))
    w_p, w_q = rng.standard_normal((Tn, H, n_s)), rng.standard_normal((Tn, H, n_s, n_s))
    leaves = dict(p_0=_t(x["p"]).requires_grad_(True), k_ff=_t(k_ff).requires_grad_(True), k_fb=_t(k_fb).requires_grad_(True))
    if start_q:
        leaves.update(q_0=_t(x["q"]).requires_grad_(True), k_fb_init=_t(x["k_fb"]).requires_grad_(True))
    kw = dict(q_0=leaves.get("q_0"), c_safety=x["c"], a=x["a"], b=x["b"], k_fb_init=leaves.get("k_fb_init"))
    p_all, q_all = reach.multistep_reachability_batch(leaves["p_0"], gp, leaves["k_fb"], leaves["k_ff"], x["l_mu"], x["l_sigma"],
                                                      differentiable=True, **kw)
    gp.set_chain(False)
    try:
        kw0 = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in kw.items()}
        fwd = reach.multistep_reachability_batch(leaves["p_0"].detach(), gp, leaves["k_fb"].detach(), leaves["k_ff"].detach(),
                                                 x["l_mu"], x["l_sigma"], **kw0)
    finally:
        gp.set_chain(True)
    assert torch.equal(p_all, fwd[0]) and torch.equal(q_all, fwd[1]), "values differ from the forward's per-step route"
    names = list(leaves)
    grads = dict(zip(names, torch.autograd.grad((p_all * _t(w_p)).sum() + (q_all * _t(w_q)).sum(), [leaves[k] for k in names])))
    pa, qa = p_all.detach().cpu().numpy(), q_all.detach().cpu().numpy()
    states = [(x["p"], x["q"] if start_q else None)] + [(pa[:, i], qa[:, i]) for i in range(H - 1)]
    lins = [tuple(o.cpu().numpy() for o in gp.linearize_device_batch(np.hstack((states[i][0], k_ff[:, i])))) for i in range(H)]
    ref = _sweep_reference(x, H, lins, states, None, w_p, w_q, k_ff, k_fb, start_q, fp64=False)
    alt = _sweep_reference(x, H, lins, states, None, w_p, w_q, k_ff, k_fb, start_q, fp64=True)
    for name in names:
        got = grads[name].cpu().numpy()
        scale = np.abs(ref[name]).max()
        err, floor = np.abs(got - ref[name]).max() / scale, np.abs(alt[name] - ref[name]).max() / scale
        print("multistep start_q=%s d/d%s: device %.2e, two CPU routes %.2e of the largest element (bar %.1e)"
              % (start_q, name, err, floor, PROP_RTOL))
        assert np.isfinite(got).all() and err <= PROP_RTOL, (name, err)


# ---- 4. the example ------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_its_loss_goes_down():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "safe_shooting_gradient.py")], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    losses = [float(line.split()[-1]) for line in res.stdout.splitlines() if line.startswith("step")]
    assert len(losses) >= 3 and losses[-1] < losses[0], res.stdout
