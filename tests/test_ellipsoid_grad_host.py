"""The long-double reverse pass of the ellipsoid step (tests/_ellipsoid_grad_ref.py) against two independent routes to the same
gradient, on the CPU:

  1. central differences of _ellipsoid_ref.step in long double, every entry of every input, contracted with random seeds
     (the differences of p1 and q1 are formed entry by entry BEFORE the contraction, so an input that does not move q1 sees none
     of its rounding); agreement to 1e-6 of the largest entry of each gradient.  A formula error is O(1); the bar is loose on
     purpose and also holds where long double is fp64 (five-point differences with a step of 1e-3 of the entry or of a tenth of
     the array's largest, 3e-2 for var, whose effect on q1 sits 1e-10 below the entries it is added to at a gain of 1e3:
     truncation below 1e-8, rounding 1e-16 / 1e-3 times the cancellation in the entry).
  2. torch autograd (CPU, fp64) through a torch restatement of the step with torch.linalg.eigvalsh; agreement to 1e-8 of the
     largest entry (fp64 rounding of two different routes, amplified by the gain of 1e3 in a third of the queries).

Instances (1,1), (2,1), (3,2), (4,1), (8,4); families random, diag, rank1, graded, rounded; both branches; 16 queries per case
(every 17th query of the 257, so that all three gain scales of the cases are met); a = b = None once.  Then: symmetry of q_bar,
NULL seed = zero seed to the bit, NaN for a query with var = 0, and the measured shares of the fp64 restatement against
_ellipsoid_grad_ref.SHARE.
"""
import numpy as np
import pytest

import _ellipsoid_ref as R
import _ellipsoid_grad_ref as G

LD = np.longdouble
FAMILIES = ("random", "diag", "rank1", "graded", "rounded")
ROWS = tuple(range(0, 257, 17))[:16]
INPUT_OF = dict(p_bar="p", q_bar="q", kff_bar="k_ff", kfb_bar="k_fb", mu_bar="mu", var_bar="var", jac_bar="jac")


def _outputs(branch):
    return tuple(n for n in G.OUTPUTS if branch == "ell" or n not in ("q_bar", "kfb_bar", "jac_bar"))


def _fd_gradient(case, t, branch, lin, pb, qb, key):
    a, b = (case["a"], case["b"]) if lin else (None, None)
    base = {k: np.array(case[k][t], dtype=LD) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
    if key == "q":
        base["q"] = (base["q"] + base["q"].T) / 2

    def f(d):
        return R.step(d["p"], d["q"] if branch == "ell" else None, d["k_ff"], d["k_fb"], d["mu"], d["var"], d["jac"],
                      case["l_mu"], case["l_sigma"], case["c"], a, b)

    x = base[key]
    grad = np.zeros(x.shape, dtype=LD)
    # a tenth of the array's largest entry at least; the gain enters through I + K^T K, so its own floor is 1
    floor = max(LD(0.1) * np.abs(x).max(), LD(1.0) if key == "k_fb" else LD(0))
    for idx in np.ndindex(x.shape):
        if key == "q" and idx[0] > idx[1]:
            continue
        h = LD(3e-2) * abs(x[idx]) if key == "var" else LD(1e-3) * max(abs(x[idx]), floor)     # (sqrt(var): no floor)
        e = np.zeros(x.shape, dtype=LD)
        e[idx] = h
        if key == "q" and idx[0] != idx[1]:
            e[idx[::-1]] = h                       # a symmetric move: both halves of the gradient at once
        up, dn = f(dict(base, **{key: x + e})), f(dict(base, **{key: x - e}))
        up2, dn2 = f(dict(base, **{key: x + 2 * e})), f(dict(base, **{key: x - 2 * e}))
        d1 = lambda k: 8 * (up[k] - dn[k]) - (up2[k] - dn2[k])          # the five-point central difference, times 12 h
        d = ((d1("p1") * pb).sum() + (d1("q1") * qb).sum()) / (12 * h)
        if key == "q" and idx[0] != idx[1]:
            grad[idx] = grad[idx[::-1]] = d / 2
        else:
            grad[idx] = d
    return grad


def _against_central_differences(inst, family, branch, lin):
    case = R.cases(*inst)[family]
    pb_all, qb_all = G.seeds(case)
    worst = {}
    for t in ROWS:
        pb, qb = LD(1) * pb_all[t], LD(1) * qb_all[t]
        o = G.step_vjp(case["p"][t], case["q"][t] if branch == "ell" else None, case["k_ff"][t], case["k_fb"][t],
                       case["mu"][t], case["var"][t], case["jac"][t], case["l_mu"], case["l_sigma"], case["c"],
                       case["a"] if lin else None, case["b"] if lin else None, pb, qb)
        assert not o["bad"]
        for name in _outputs(branch):
            fd = _fd_gradient(case, t, branch, lin, pb, qb, INPUT_OF[name])
            top = float(np.abs(o[name]).max())
            err = float(np.abs(fd - o[name]).max())
            worst[name] = max(worst.get(name, 0.0), err / top if top > 0 else err)
    print(inst, family, branch, {k: "%.1e" % v for k, v in worst.items()})
    assert all(v <= 1e-6 for v in worst.values()), worst


@pytest.mark.parametrize("branch", ("ell", "point"))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inst", G.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_vjp_against_central_differences(inst, family, branch):
    _against_central_differences(inst, family, branch, True)


@pytest.mark.parametrize("branch", ("ell", "point"))
def test_vjp_against_central_differences_without_a_and_b(branch):
    _against_central_differences((3, 2), "random", branch, False)


def _torch_step(torch, p, q, u, k, mu, var, jac, l_mu, l_sigma, c, a, b):
    n_s = p.shape[0]
    p1 = a @ p + b @ u + mu
    if q is None:
        return p1, torch.diag(n_s * (c * torch.sqrt(var)) ** 2)
    qs = (q + q.T) / 2
    h = a + jac[:, :n_s] + (jac[:, n_s:] + b) @ k
    q0 = h @ qs @ h.T
    l = torch.linalg.cholesky(torch.eye(n_s, dtype=q.dtype) + k.T @ k)
    r2 = torch.linalg.eigvalsh(l.T @ qs @ l)[-1]
    ub_mu, ub_sg = l_mu * r2, c * (torch.sqrt(var) + l_sigma * torch.sqrt(r2))
    d_s, d_m = n_s * ub_sg ** 2, n_s * ub_mu ** 2
    c1 = torch.sqrt(d_s.sum() / d_m.sum())
    d_l = (1 + 1 / c1) * d_s + (1 + c1) * d_m
    c2 = torch.sqrt(d_l.sum() / torch.trace(q0))
    return p1, (1 + c2) * q0 + torch.diag((1 + 1 / c2) * d_l)


@pytest.mark.parametrize("branch", ("ell", "point"))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inst", G.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_vjp_against_torch_autograd(inst, family, branch):
    torch = pytest.importorskip("torch")
    case = R.cases(*inst)[family]
    pb_all, qb_all = G.seeds(case)
    tt = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    const = [tt(case[k]) for k in ("l_mu", "l_sigma")] + [case["c"], tt(case["a"]), tt(case["b"])]
    worst = {}
    for t in ROWS:
        ins = {k: tt(case[k][t]).requires_grad_(True) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
        p1, q1 = _torch_step(torch, ins["p"], ins["q"] if branch == "ell" else None, ins["k_ff"], ins["k_fb"], ins["mu"],
                             ins["var"], ins["jac"], *const)
        ((p1 * tt(pb_all[t])).sum() + (q1 * tt(qb_all[t])).sum()).backward()
        o = G.step_vjp(case["p"][t], case["q"][t] if branch == "ell" else None, case["k_ff"][t], case["k_fb"][t],
                       case["mu"][t], case["var"][t], case["jac"][t], case["l_mu"], case["l_sigma"], case["c"], case["a"],
                       case["b"], pb_all[t], qb_all[t])
        if o["g"] < G.G_MIN:
            continue
        for name in _outputs(branch):
            got = ins[INPUT_OF[name]].grad.numpy()
            want = o[name].astype(np.float64)
            top = float(np.abs(want).max())
            err = float(np.abs(got - want).max())
            worst[name] = max(worst.get(name, 0.0), err / top if top > 0 else err)
    print(inst, family, branch, {k: "%.1e" % v for k, v in worst.items()})
    assert all(v <= 1e-8 for v in worst.values()), worst


@pytest.mark.parametrize("inst", G.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_conventions(inst):
    case = R.cases(*inst)["rounded"]
    pb, qb = G.seeds(case)
    for branch in ("ell", "point"):
        both = G.vjp_batch(case, branch, pb, qb, rows=ROWS[:4])
        assert np.array_equal(both["q_bar"], both["q_bar"].transpose(0, 2, 1))
        # only the symmetric part of q1_bar counts
        sym = G.vjp_batch(case, branch, pb, (qb + qb.transpose(0, 2, 1)) / 2, rows=ROWS[:4])
        # a NULL seed is a zero seed, to the bit
        for null, zero in (((None, qb), (np.zeros_like(pb), qb)), ((pb, None), (pb, np.zeros_like(qb)))):
            x, y = G.vjp_batch(case, branch, *null, rows=ROWS[:4]), G.vjp_batch(case, branch, *zero, rows=ROWS[:4])
            for name in G.OUTPUTS:
                assert np.array_equal(x[name], y[name]), (branch, name)
        for name in G.OUTPUTS:            # (the seed is symmetrised in fp64 here and in long double there)
            assert np.all(np.abs(sym[name] - both[name]) <= 4 * G.EPS * both[name + "_abs"]), (branch, name)
    # a query with var = 0: its box half-widths are not all > 0 in the point branch -> NaN there, and only there
    t = ROWS[1]
    var0 = np.array(case["var"][t])
    var0[0] = 0.0
    o = G.step_vjp(case["p"][t], None, case["k_ff"][t], case["k_fb"][t], case["mu"][t], var0, case["jac"][t], case["l_mu"],
                   case["l_sigma"], case["c"], case["a"], case["b"], pb[t], qb[t])
    assert o["bad"] and all(np.isnan(o[name]).all() for name in G.OUTPUTS)


def test_measured_shares_of_the_fp64_restatement():
    """the floor the GPU bars are 30 times of: fp64 against long double over the host cases, per output array"""
    worst = G.measure_shares()
    print({k: "%.2f" % v for k, v in worst.items()})
    for name in G.OUTPUTS:
        assert np.isfinite(worst[name])
    if np.finfo(LD).eps < np.finfo(np.float64).eps:
        for name in G.OUTPUTS:
            assert worst[name] <= G.SHARE[name], (name, worst[name])
