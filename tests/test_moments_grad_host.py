"""The long-double reverse pass of the moment step (tests/_moments_grad_ref.py) against two independent routes to the same gradient,
on the CPU, and the argument checks of the Python wrappers, which run before any device is touched:

  1. central differences of _ellipsoid_ref.step (modes 1 and 2) in long double, every entry of every input, contracted with
     random seeds.  The step is a polynomial of degree two in every single input entry, so a central difference has no truncation
     error; agreement to 1e-6 of the largest entry of each gradient (a formula error is O(1); the bar also holds where long
     double is fp64: steps of 1e-3 of the entry or of a tenth of the array's largest, 3e-2 for var, whose effect on q1 sits 1e-10
     below the entries it is added to at a gain of 1e3; differences in any other input are taken at var = 0, the same additive
     term on both sides).
  2. torch autograd (CPU, fp64) through a torch restatement of the step: agreement to HOST_RTOL of the largest entry of each
     gradient, 30 x the largest disagreement, in the same measure, of the two CPU routes of _moments_grad_ref (long double and its
     fp64 restatement) over the same cases.

Instances (1,1), (2,1), (3,2), (4,1), (8,4); both modes and starts; families random, diag, rank1, graded, rounded (central
differences: 4 queries per case, one or two at each of the three gain scales; autograd: 16, every 17th of the 257); a = b = None
once.  Then the conventions (symmetry of sigma_bar, an unsymmetric seed = its symmetric part, NULL seed = zero seed to the bit)
and the measured shares of the fp64 restatement against _moments_grad_ref.SHARE.
"""
import numpy as np
import pytest

import _ellipsoid_ref as R
import _moments_grad_ref as M

LD = np.longdouble
FAMILIES = ("random", "diag", "rank1", "graded", "rounded")
ROWS = M.SHARE_ROWS
FD_ROWS = (0, 102, 187, 238)
INPUT_OF = dict(mux_bar="p", sigma_bar="q", kff_bar="k_ff", kfb_bar="k_fb", mug_bar="mu", var_bar="var", jac_bar="jac")
HOST_RTOL = 30 * 1.35e-14          # the two CPU routes disagree by at most 1.31e-14 of the largest element (test_host_rtol_floor)


def _outputs(start):
    return tuple(n for n in M.OUTPUTS if start == "gauss" or n not in ("sigma_bar", "kfb_bar", "jac_bar"))


def _fd_gradient(case, t, start, mode, lin, mb, sb, key):
    a, b = (case["a"], case["b"]) if lin else (None, None)
    base = {k: np.array(case[k][t], dtype=LD) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
    if key == "q":
        base["q"] = (base["q"] + base["q"].T) / 2

    def f(d):
        return R.step(d["p"], d["q"] if start == "gauss" else None, d["k_ff"], d["k_fb"], d["mu"], d["var"], d["jac"],
                      None, None, 1.0, a, b, mode)

    if key != "var":
        # diag(var) is the same term in both evaluations of a difference in any other input; where the shape matrix is 1e-12
        # (`graded` at n_s = 1) it would only leave its rounding, ten orders above the difference itself
        base["var"] = np.zeros_like(base["var"])
    x = base[key]
    grad = np.zeros(x.shape, dtype=LD)
    floor = max(LD(0.1) * np.abs(x).max(), LD(1.0) if key == "k_fb" else LD(0))
    for idx in np.ndindex(x.shape):
        if key == "q" and idx[0] > idx[1]:
            continue
        h = LD(3e-2) * abs(x[idx]) if key == "var" else LD(1e-3) * max(abs(x[idx]), floor)
        e = np.zeros(x.shape, dtype=LD)
        e[idx] = h
        if key == "q" and idx[0] != idx[1]:
            e[idx[::-1]] = h                       # a symmetric move: both halves of the gradient at once
        up, dn = f(dict(base, **{key: x + e})), f(dict(base, **{key: x - e}))
        d = (((up["p1"] - dn["p1"]) * mb).sum() + ((up["q1"] - dn["q1"]) * sb).sum()) / (2 * h)
        if key == "q" and idx[0] != idx[1]:
            grad[idx] = grad[idx[::-1]] = d / 2
        else:
            grad[idx] = d
    return grad


def _against_central_differences(inst, family, start, mode, lin):
    case = R.cases(*inst)[family]
    mb_all, sb_all, _ = M.seeds(case)
    worst = {}
    for t in FD_ROWS:
        mb, sb = LD(1) * mb_all[t], LD(1) * sb_all[t]
        o = M.step_vjp(case["p"][t], case["q"][t] if start == "gauss" else None, case["k_ff"][t], case["k_fb"][t], case["mu"][t],
                       case["var"][t], case["jac"][t], case["a"] if lin else None, case["b"] if lin else None, mode, mb, sb)
        for name in _outputs(start):
            fd = _fd_gradient(case, t, start, mode, lin, mb, sb, INPUT_OF[name])
            top = float(np.abs(o[name]).max())
            err = float(np.abs(fd - o[name]).max())
            worst[name] = max(worst.get(name, 0.0), err / top if top > 0 else err)
    print(inst, family, start, mode, {k: "%.1e" % v for k, v in worst.items()})
    assert all(v <= 1e-6 for v in worst.values()), worst


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("start", M.STARTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inst", M.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_vjp_against_central_differences(inst, family, start, mode):
    _against_central_differences(inst, family, start, mode, True)


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("start", M.STARTS)
def test_vjp_against_central_differences_without_a_and_b(start, mode):
    _against_central_differences((3, 2), "random", start, mode, False)


def _torch_step(p, q, u, k, mu, var, jac, a, b, mode):
    import torch
    n_s = p.shape[0]
    p1 = a @ p + b @ u + mu
    if q is None:
        return p1, torch.diag(var)
    qs = (q + q.T) / 2
    h = a + b @ k if mode == 2 else a + jac[:, :n_s] + (jac[:, n_s:] + b) @ k
    return p1, h @ qs @ h.T + torch.diag(var)


def _relative_to_the_largest(inst, family, start, mode, route):
    """worst |route - long double| / max |long double| per output over ROWS; route "fp64": the restatement, "torch": autograd"""
    case = R.cases(*inst)[family]
    mb_all, sb_all, _ = M.seeds(case)
    worst = {}
    if route == "torch":
        import torch
        tt = lambda x: torch.tensor(np.asarray(x, dtype=np.float64))
    for t in ROWS:
        args = (case["p"][t], case["q"][t] if start == "gauss" else None, case["k_ff"][t], case["k_fb"][t], case["mu"][t],
                case["var"][t], case["jac"][t], case["a"], case["b"], mode, mb_all[t], sb_all[t])
        o = M.step_vjp(*args)
        if route == "torch":
            ins = {k: tt(case[k][t]).requires_grad_(True) for k in ("p", "q", "k_ff", "k_fb", "mu", "var", "jac")}
            p1, q1 = _torch_step(ins["p"], ins["q"] if start == "gauss" else None, ins["k_ff"], ins["k_fb"], ins["mu"], ins["var"],
                                 ins["jac"], tt(case["a"]), tt(case["b"]), mode)
            ((p1 * tt(mb_all[t])).sum() + (q1 * tt(sb_all[t])).sum()).backward()
            other = {n: (ins[INPUT_OF[n]].grad.numpy() if ins[INPUT_OF[n]].grad is not None else np.zeros(o[n].shape))
                     for n in _outputs(start)}
        else:
            other = M.step_vjp(*args, fp64=True)
        for name in _outputs(start):
            want = o[name].astype(np.float64)
            top = float(np.abs(want).max())
            err = float(np.abs(np.asarray(other[name], dtype=np.float64) - want).max())
            worst[name] = max(worst.get(name, 0.0), err / top if top > 0 else err)
    return worst


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("start", M.STARTS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("inst", M.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_vjp_against_torch_autograd(inst, family, start, mode):
    pytest.importorskip("torch")
    worst = _relative_to_the_largest(inst, family, start, mode, "torch")
    print(inst, family, start, mode, {k: "%.1e" % v for k, v in worst.items()})
    assert all(v <= HOST_RTOL for v in worst.values()), worst


def test_host_rtol_floor():
    """the disagreement of the two CPU routes that HOST_RTOL is 30 times of"""
    floor = 0.0
    for inst in M.HOST_INSTANCES:
        for family in FAMILIES:
            for start in M.STARTS:
                for mode in M.MODES:
                    floor = max(floor, max(_relative_to_the_largest(inst, family, start, mode, "fp64").values()))
    print("two CPU routes: %.2e of the largest element" % floor)
    if np.finfo(LD).eps < np.finfo(np.float64).eps:
        assert HOST_RTOL / 60 <= floor <= HOST_RTOL / 30, floor


@pytest.mark.parametrize("inst", M.HOST_INSTANCES, ids=lambda i: "%dx%d" % i)
def test_conventions(inst):
    case = R.cases(*inst)["rounded"]
    mb, sb, vb = M.seeds(case)
    for mode in M.MODES:
        for start in M.STARTS:
            both = M.vjp_batch(case, start, mode, mb, sb, vb, rows=ROWS[:4])
            assert np.array_equal(both["sigma_bar"], both["sigma_bar"].transpose(0, 2, 1))
            # only the symmetric part of sigma1_bar counts
            sym = M.vjp_batch(case, start, mode, mb, (sb + sb.transpose(0, 2, 1)) / 2, vb, rows=ROWS[:4])
            for name in M.OUTPUTS:        # (the seed is symmetrised in fp64 here and in long double there)
                assert np.all(np.abs(sym[name] - both[name]) <= 4 * M.EPS * both[name + "_abs"]), (mode, start, name)
            # a NULL seed is a zero seed, to the bit
            for null, zero in (((None, sb, vb), (np.zeros_like(mb), sb, vb)), ((mb, None, vb), (mb, np.zeros_like(sb), vb)),
                               ((mb, sb, None), (mb, sb, np.zeros_like(vb)))):
                x, y = M.vjp_batch(case, start, mode, *null, rows=ROWS[:4]), M.vjp_batch(case, start, mode, *zero, rows=ROWS[:4])
                for name in M.OUTPUTS:
                    assert np.array_equal(x[name], y[name]), (mode, start, name)
            if mode == 2 or start == "point":
                assert not both["jac_bar"].any()
            if start == "point":
                assert not both["sigma_bar"].any() and not both["kfb_bar"].any()


def test_measured_shares_of_the_fp64_restatement():
    """the floor the GPU bars are 30 times of: fp64 against long double over the host cases, per output array; the committed
    table is reproduced within a factor 2"""
    worst = M.measure_shares()
    print({k: "%.2f" % v for k, v in worst.items()})
    for name in M.OUTPUTS:
        assert np.isfinite(worst[name])
    if np.finfo(LD).eps < np.finfo(np.float64).eps:
        for name in M.OUTPUTS:
            assert M.SHARE[name] / 2 <= worst[name] <= M.SHARE[name], (name, worst[name])


def test_wrapper_argument_checks_need_no_device():
    from safe_exploration_amd import uncertainty_propagation_casadi as U
    T_, n_s, n_u = 3, 2, 1
    z = lambda *s: np.zeros(s)
    ok = dict(mu_x=z(T_, n_s), k_ff=z(T_, n_u), mu_g=z(T_, n_s), var_g=z(T_, n_s), jac_g=z(T_, n_s, n_s + n_u), mu1_bar=z(T_, n_s))
    bad = [dict(mode=0), dict(mode=3),                                                  # mode outside {1, 2}
           dict(sigma_x=z(T_, n_s, n_s)),                                               # k_fb required with sigma_x
           dict(sigma_x=z(T_, n_s, n_s), k_fb=z(T_, n_u, n_s), jac_g=None),             # jac_g required with sigma_x (Taylor)
           dict(mu_x=z(n_s)), dict(k_ff=z(T_ + 1, n_u)), dict(mu_g=z(T_, n_s + 1)), dict(var_g=z(T_)),
           dict(sigma_x=z(T_, n_s, n_s + 1), k_fb=z(T_, n_u, n_s)), dict(sigma_x=z(T_, n_s, n_s), k_fb=z(T_, n_s, n_u)),
           dict(sigma_x=z(T_, n_s, n_s), k_fb=z(T_, n_u, n_s), jac_g=z(T_, n_s, n_s)),
           dict(mu1_bar=None), dict(mu1_bar=z(T_, n_s + 1)), dict(sigma1_bar=z(T_, n_s))]
    for change in bad:
        with pytest.raises(ValueError):
            U.moment_step_vjp_batch(**dict(ok, **change))
    with pytest.raises(TypeError):            # differentiable=True needs tensors
        U.moment_step_batch(ok["mu_x"], ok["k_ff"], ok["mu_g"], ok["var_g"], None, differentiable=True)
    for fn in (U.onestep_moments_batch, U.onestep_moments_vjp_batch):
        with pytest.raises(TypeError):        # any other state space model: the GP has to be the device model
            fn(ok["mu_x"], object(), ok["k_ff"])
    with pytest.raises(TypeError):
        U.onestep_moments_batch(ok["mu_x"], object(), ok["k_ff"], differentiable=True)
    with pytest.raises(TypeError):
        U.multistep_moments_batch(ok["mu_x"], object(), z(T_, 2, n_u), None, differentiable=True)
