"""Host side of the SafeMPC constraint rows (sr_rollout_constraints, sr_rollout_constraints_vjp;
safe_exploration_amd.gp_reachability).  No GPU.

1. The two entries are declared by the header, exported by the library, bound in _lib.py with the agreed signatures, built from
   sr_rollout_constraints.hip; the module has the agreed surface (fails without the feature).  Wrong shapes raise ValueError before
   a device is touched.
2. rollout_constraint_layout and the host twin safety_constraints against a hand-written H = 3 instance (n_s = 2, n_u = 1; every
   number below is written out from lin_ellipsoid_safety_distance by hand), in the reference's order, for both starts; and the
   batched reference (tests/_rollout_constraints_ref) against the host twin.
3. The reference's closed-form reverse pass against torch autograd (CPU) through the einsum form -- 1e-11 of the largest element:
   two fp64 evaluations whose slopes 1 / (2 s) carry the cancellation in a rank-1 radicand, 1e4 roundings at the worst --, and in long double against central differences on the full-rank shapes -- 1e-8 (step 1e-7:
   rounding 1e-19 / 1e-7 = 1e-12; truncation step^2 / (8 x^2) of a row's slope at a radicand x, below 1e-8 for x > 4e-4; a rank-1
   shape has rows with radicands of 1e-5, where a difference quotient says nothing: those are left to autograd).  The zero-radicand convention: no NaN, no contribution.
4. The floors behind the GPU bars, on exactly _rollout_constraints_ref.CASES (the GPU test's inputs): fp64 against long double of
   the reference, per output; and the chain floor: the gradient in k_ff, k_fb of the augmented Lagrangian through the NumPy
   roll-out's reverse sweep (tests/_reach_rollout_grad_ref) with the closed-form seeds and direct terms against those of torch
   autograd through the einsum form.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _rollout_constraints_ref as RN

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="np.longdouble is no wider than float64 here")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- 1. the surface -----------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_and_bound(lib_built):
    """fails without the feature"""
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    hdr = _read("include", "safereach.h")
    for name in ("sr_rollout_constraints", "sr_rollout_constraints_vjp"):
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export " + name
        assert re.search(r"^int %s\(int device, long T, int H, int n_s, int n_u,$" % name, hdr, re.M), name
    for word in ("satisfied iff g <= 0", "(bounds ? 2 n_u H : 0) + m_obs (H - 1) + m_safe", "symmetric parts", "NaN if any of its rows is NaN",
                 "the bits of sr_safety_distance", "exactly symmetric", "Overwritten, not accumulated", "not all four", "contributes ZERO",
                 "subdifferential", "infinite one-sided slope", "sr_ellipsoid_step_vjp", "SR_EUNSUPPORTED n_s > 12 or n_u > 12",
                 "T == 0 is a no-op", "required iff q0 is given", "`stream`"):
        assert word in hdr, word
    from safe_exploration_amd import _lib
    P, I, L, D = _lib._P, _lib._I, _lib._L, _lib._D
    head = [I, L, I, I, I] + [P] * 8 + [I, P, P, I, P, P, D]
    assert _lib.SIGNATURES["sr_rollout_constraints"] == (ctypes.c_int, head + [P] * 3)
    assert _lib.SIGNATURES["sr_rollout_constraints_vjp"] == (ctypes.c_int, head + [P] * 8)
    assert "sr_rollout_constraints.hip" in _read("safe_exploration_amd", "csrc", "Makefile")
    kernel = _read("safe_exploration_amd", "csrc", "sr_rollout_constraints.hip")
    assert "sr_safety_row(" in kernel and "sr_safety_row(" in _read("safe_exploration_amd", "csrc", "sr_ellipsoid.hip")


def test_python_surface(lib_built):
    from safe_exploration_amd import gp_reachability as reach
    names = lambda f: list(inspect.signature(f).parameters)
    common = ["p_all", "q_all", "k_ff", "k_fb", "ctrl_bounds", "h_mat_obs", "h_obs", "h_mat_safe", "h_safe", "q_0", "k_fb_0", "c_safety"]
    assert names(reach.rollout_constraints_batch) == common + ["return_max", "differentiable", "device"]
    assert names(reach.rollout_constraints_vjp_batch) == common + ["g_bar", "device"]
    sig = inspect.signature(reach.rollout_constraints_batch)
    assert [sig.parameters[n].default for n in names(reach.rollout_constraints_batch)[4:]] == [None] * 7 + [1.0, False, False, None]
    assert names(reach.rollout_constraint_layout) == ["H", "n_u", "m_obs", "m_safe", "has_bounds"]
    assert names(reach.safety_constraints)[:5] == ["p_all", "q_all", "u_0", "k_fb", "k_ff_all"]


def test_refusals_before_any_device(lib_built):
    from safe_exploration_amd import gp_reachability as reach
    T, H, n_s, n_u = 2, 3, 4, 1
    ok = dict(p_all=np.zeros((T, H, n_s)), q_all=np.zeros((T, H, n_s, n_s)), k_ff=np.zeros((T, H, n_u)), k_fb=np.zeros((T, H - 1, n_u, n_s)),
              ctrl_bounds=np.array([[-1.0, 1.0]]), h_mat_safe=np.ones((2, n_s)), h_safe=np.ones(2))
    bad = (dict(p_all=np.zeros((T, n_s))), dict(q_all=np.zeros((T, H, n_s, 3))), dict(k_ff=np.zeros((T, H + 1, n_u))), dict(k_ff=None),
           dict(k_fb=None), dict(k_fb=np.zeros((T, H, n_u, n_s))), dict(ctrl_bounds=np.zeros((2, 2))), dict(ctrl_bounds=np.zeros((1, 3))),
           dict(q_0=np.zeros((T, n_s, n_s))), dict(k_fb_0=np.zeros((T, n_u, n_s))), dict(q_0=np.zeros((T, n_s, 3)), k_fb_0=np.zeros((T, n_u, n_s))),
           dict(q_0=np.zeros((T, n_s, n_s)), k_fb_0=np.zeros((T, 2, n_s))), dict(h_mat_obs=np.ones((1, n_s))), dict(h_obs=np.ones(1)),
           dict(h_mat_safe=np.ones((2, 3))), dict(h_safe=np.ones(3)), dict(ctrl_bounds=None, h_mat_safe=None, h_safe=None))
    for kw in bad:
        for fn, more in ((reach.rollout_constraints_batch, {}), (reach.rollout_constraints_vjp_batch, dict(g_bar=np.zeros((T, 2 * H + 2))))):
            with pytest.raises(ValueError):
                fn(**dict(ok, **dict(kw, **more)))
    with pytest.raises(TypeError):
        reach.rollout_constraints_batch(differentiable=True, **ok)
    with pytest.raises(NotImplementedError):
        reach.rollout_constraints_batch(np.zeros((1, 2, 13)), np.zeros((1, 2, 13, 13)), None, None, h_mat_safe=np.ones((1, 13)), h_safe=np.ones(1))
    with pytest.raises(ValueError):
        reach.rollout_constraint_layout(0, 1, 0, 1, True)
    with pytest.raises(ValueError):
        reach.rollout_constraint_layout(3, 0, 0, 1, True)


# ---- 2. the layout and the host twin against a hand-written instance ------------------------------------------------------------------
def _hand_instance():
    """H = 3, n_s = 2, n_u = 1, diagonal shapes and axis-aligned or (3, 4) half-spaces: every square root is of a perfect square"""
    x = dict(p_all=np.array([[1.0, 2.0], [0.5, -1.0], [-2.0, 0.25]]), q_all=np.array([np.diag([4.0, 9.0]), np.diag([0.25, 1.0]), np.diag([16.0, 1.0])]),
             u_0=np.array([0.5]), k_ff_all=np.array([[-0.25], [1.5]]), k_fb=np.array([[[1.0, 0.0]], [[0.0, 2.0]]]),
             ctrl_bounds=np.array([[-1.0, 2.0]]), h_mat_obs=np.array([[1.0, 0.0], [0.0, -1.0]]), h_obs=np.array([3.0, 1.0]),
             h_mat_safe=np.array([[3.0, 4.0]]), h_safe=np.array([10.0]), q_0=np.array([[1.0, 0.0], [0.0, 4.0]]), k_fb_0=np.array([[0.0, 1.5]]))
    # control: step 1 reads (q_all[0], k_fb[0] = [1, 0]): r = sqrt(4) = 2;  step 2 reads (q_all[1], k_fb[1] = [0, 2]): r = sqrt(4 * 1) = 2
    ctrl = [-0.25 + 2 - 2, -1 + 0.25 + 2, 1.5 + 2 - 2, -1 - 1.5 + 2]
    # obstacle rows on the states 0 and 1: h = (1, 0): p_x + sqrt(q_xx) - 3;  h = (0, -1): -p_y + sqrt(q_yy) - 1
    obs = [1 + 2 - 3, -2 + 3 - 1, 0.5 + 0.5 - 3, 1 + 1 - 1]
    # terminal row on state 2: 3 (-2) + 4 (0.25) + sqrt(9 * 16 + 16 * 1) - 10
    term = [-6 + 1 + np.sqrt(160.0) - 10]
    # u_0 from the ellipsoid (q_0, k_fb_0 = [0, 1.5]): r = sqrt(2.25 * 4) = 3
    u0_ell = [0.5 + 3 - 2, -1 - 0.5 + 3]
    return x, ctrl, obs, term, u0_ell


def test_layout_and_host_twin_against_a_hand_written_instance(lib_built):
    from safe_exploration_amd import gp_reachability as reach
    x, ctrl, obs, term, u0_ell = _hand_instance()
    blocks, names = reach.rollout_constraint_layout(3, 1, 2, 1, True)
    assert blocks == dict(control=slice(0, 6), obstacle=slice(6, 10), terminal=slice(10, 11))
    assert names == (["u_0_ctrl_constraint"] * 2 + ["ellipsoid_ctrl_constraint_0"] * 2 + ["ellipsoid_ctrl_constraint_1"] * 2
                     + ["obstacle_avoidance_constraint0"] * 2 + ["obstacle_avoidance_constraint1"] * 2 + ["terminal constraint"])
    blocks, names = reach.rollout_constraint_layout(1, 3, 4, 2, False)
    assert blocks == dict(control=slice(0, 0), obstacle=slice(0, 0), terminal=slice(0, 2)) and names == ["terminal constraint"] * 2
    point = {k: v for k, v in x.items() if k not in ("q_0", "k_fb_0")}
    g, lbg, ubg, g_name = reach.safety_constraints(**point)
    assert np.allclose(g, [0.5] + ctrl + obs + term, rtol=0, atol=1e-15)
    assert lbg == [-1.0] + [-np.inf] * 9 and ubg == [2.0] + [0.0] * 9
    assert g_name == ["u_0_ctrl_constraint"] + names_of(3, 1, 2, 1)[2:]
    g, lbg, ubg, g_name = reach.safety_constraints(c_safety=1.0, **x)
    assert np.allclose(g, u0_ell + ctrl + obs + term, rtol=0, atol=1e-15)
    assert lbg == [-np.inf] * 11 and ubg == [0.0] * 11 and g_name == names_of(3, 1, 2, 1)
    # the batched reference on the same instance: the library's layout, the point u_0 as the two one-sided rows
    for start in ("point", "q0"):
        r = _as_ref_inputs(x, start)
        got = RN.constraints(r)[0][0]
        want = ([0.5 - 2.0, -1.0 - 0.5] if start == "point" else u0_ell) + ctrl + obs + term
        assert np.allclose(got, want, rtol=0, atol=1e-15), start
    # without bounds or obstacles only the terminal row is left; c_safety scales the square root alone
    g, lbg, ubg, g_name = reach.safety_constraints(x["p_all"], x["q_all"], None, None, None, h_mat_safe=x["h_mat_safe"], h_safe=x["h_safe"], c_safety=2.0)
    assert np.allclose(g, [-6 + 1 + 2 * np.sqrt(160.0) - 10]) and g_name == ["terminal constraint"] and ubg == [0.0]


def names_of(H, n_u, m_obs, m_safe):
    from safe_exploration_amd import gp_reachability as reach
    return reach.rollout_constraint_layout(H, n_u, m_obs, m_safe, True)[1]


def _as_ref_inputs(x, start):
    """the hand-written instance in the layout of _rollout_constraints_ref (T = 1)"""
    return dict(T=1, H=3, n_s=2, n_u=1, c=1.0, bounds=True, m_obs=2, m_safe=1, p_all=x["p_all"][None], q_all=x["q_all"][None],
                k_ff=np.concatenate((x["u_0"][None], x["k_ff_all"]))[None], k_fb=x["k_fb"][None], ctrl_bounds=x["ctrl_bounds"],
                h_obs_mat=x["h_mat_obs"], h_obs=x["h_obs"], h_safe_mat=x["h_mat_safe"], h_safe=x["h_safe"],
                q0=x["q_0"][None] if start == "q0" else None, kfb0=x["k_fb_0"][None] if start == "q0" else None)


@pytest.mark.parametrize("case", [c for c in RN.CASES if c["T"] <= 5 and c["H"] <= 3], ids=RN.case_id)
def test_the_batched_reference_against_the_host_twin(lib_built, case):
    from safe_exploration_amd import gp_reachability as reach
    x = RN.make_inputs(**case)
    g = RN.constraints(x)[0]
    scale = RN.row_scale(x)
    n_u, H = x["n_u"], x["H"]
    for t in range(x["T"]):
        kw = dict(ctrl_bounds=x["ctrl_bounds"], h_mat_obs=x["h_obs_mat"], h_obs=x["h_obs"], h_mat_safe=x["h_safe_mat"], h_safe=x["h_safe"],
                  c_safety=x["c"])
        if x["q0"] is not None:
            kw.update(q_0=x["q0"][t], k_fb_0=x["kfb0"][t])
        got = reach.safety_constraints(x["p_all"][t], x["q_all"][t], x["k_ff"][t, 0], None if H == 1 else x["k_fb"][t], x["k_ff"][t, 1:], **kw)[0]
        skip = n_u if (x["bounds"] and x["q0"] is None) else 0             # the point u_0: n_u two-sided rows against 2 n_u one-sided
        assert got.size == x["n_g"] - skip
        assert np.max(np.abs(got[skip:] - g[t, 2 * skip:]) / scale[t, 2 * skip:]) <= 1e-14, t
        if skip:
            assert np.array_equal(got[:skip], x["k_ff"][t, 0])


# ---- 3. the closed-form reverse pass ------------------------------------------------------------------------------------------------
VJP_CASES = [dict(n_s=3, n_u=2, T=2, H=3, bounds=bounds, m_obs=m_obs, m_safe=m_safe, start=start, qkind=qkind, seed=8)
             for bounds, m_obs, m_safe in ((True, 2, 3), (True, 0, 1), (False, 2, 0), (True, 1, 0))
             for start in ("point", "q0") for qkind in ("full", "rank1")] + [dict(n_s=2, n_u=1, T=2, H=1, m_obs=0, m_safe=2, start="q0", seed=8)]


def _autograd(x):
    import torch
    leaves, order = {}, ("p_all", "q_all", "k_ff", "k_fb", "q0", "kfb0")
    for k in order:
        if x[k] is not None:
            leaves[k] = torch.tensor(x[k], requires_grad=True)
    g = RN.torch_constraints(leaves["p_all"], leaves["q_all"], leaves["k_ff"], leaves.get("k_fb"), x, leaves.get("q0"), leaves.get("kfb0"))
    keys = [k for k in order if k in leaves]
    grads = torch.autograd.grad((g * torch.tensor(x["g_bar"])).sum(), [leaves[k] for k in keys], allow_unused=True)
    out = dict(zip(keys, [None if v is None else v.numpy() for v in grads]))
    return g.detach().numpy(), dict(p_all_bar=out["p_all"], q_all_bar=out["q_all"], kff_bar=out["k_ff"], kfb_bar=out.get("k_fb"),
                                    q0_bar=out.get("q0"), kfb0_bar=out.get("kfb0"))


@pytest.mark.parametrize("case", VJP_CASES, ids=RN.case_id)
def test_the_reference_reverse_pass_against_autograd_and_central_differences(case):
    x = RN.make_inputs(**case)
    ref = RN.vjp(x)
    g, auto = _autograd(x)
    assert RN.g_err(g, RN.constraints(x)[0], RN.row_scale(x)) <= 1e-14
    for k in RN.OUTS:
        if ref[k] is None:
            continue
        if auto[k] is None:                                                    # autograd: the input is not read by any row
            assert not ref[k].any(), k
            continue
        sym = (auto[k] + np.swapaxes(auto[k], -1, -2)) / 2 if k in ("q_all_bar", "q0_bar") else auto[k]
        assert RN.rel_err(sym, ref[k]) <= 1e-11, (k, RN.rel_err(sym, ref[k]))
    assert np.array_equal(ref["q_all_bar"], ref["q_all_bar"].transpose(0, 1, 3, 2))
    if np.finfo(LD).eps >= np.finfo(np.float64).eps or case.get("qkind") == "rank1":
        return
    step = LD(1e-7)
    f = lambda y: (RN.constraints(y, LD)[0] * x["g_bar"].astype(LD)).sum()
    for key, out in (("p_all", "p_all_bar"), ("q_all", "q_all_bar"), ("k_ff", "kff_bar"), ("k_fb", "kfb_bar"), ("q0", "q0_bar"), ("kfb0", "kfb0_bar")):
        if x[key] is None:
            continue
        fd = np.zeros(x[key].shape)
        for i in np.ndindex(x[key].shape):
            vals = []
            for sgn in (1, -1):
                arr = x[key].astype(LD)
                arr[i] += sgn * step
                vals.append(f(dict(x, **{key: arr})))
            fd[i] = float((vals[0] - vals[1]) / (2 * step))
        if key in ("q_all", "q0"):
            fd = (fd + np.swapaxes(fd, -1, -2)) / 2
        assert RN.rel_err(fd, ref[out]) <= 1e-8, (key, RN.rel_err(fd, ref[out]))


def test_the_zero_radicand_convention_of_the_reference():
    """a zero k_fb row and q = 0: finite everywhere, no contribution through the square root"""
    x = RN.make_inputs(4, n_u=2, T=2, H=3, m_obs=1, m_safe=1, start="q0", kkind="zero_row", seed=3)
    r = RN.vjp(x)
    assert all(np.isfinite(v).all() for v in r.values())
    assert not r["kfb_bar"][:, 0, 1].any() and not r["kfb0_bar"][:, 1].any() and r["kfb_bar"][:, 0, 0].any()
    other = x["g_bar"].copy()
    other[:, 2 * 2 * 1 + 1] += 3.0                                             # the upper seed of output 1 of step 1: the zero row's
    r2 = RN.vjp(x, other)
    assert np.array_equal(r2["q_all_bar"], r["q_all_bar"]) and not np.array_equal(r2["kff_bar"], r["kff_bar"])
    z = RN.make_inputs(4, n_u=2, T=2, H=3, m_obs=1, m_safe=1, start="q0", qkind="zero", seed=3)
    rz = RN.vjp(z)
    assert all(np.isfinite(v).all() for v in rz.values())
    assert not rz["q_all_bar"].any() and not rz["kfb_bar"].any() and not rz["q0_bar"].any() and rz["p_all_bar"].any()


# ---- 4. the floors behind the GPU bars ----------------------------------------------------------------------------------------------
@needs_ld
def test_the_floors_behind_the_gpu_bars():
    worst = {}
    for c in RN.CASES:
        x = RN.make_inputs(**c)
        (g64, m64), (gld, mld) = RN.constraints(x), RN.constraints(x, LD)
        v64, vld = RN.vjp(x), RN.vjp(x, dtype=LD)
        scale = RN.row_scale(x)
        e = dict(g=max(RN.g_err(g64, gld, scale), RN.g_err(m64, mld, scale.max(axis=1))))
        for k in RN.OUTS:
            if vld[k] is not None and vld[k].size:
                e[k] = RN.rel_err(v64[k], vld[k])
        for k, v in e.items():
            if v >= worst.get(k, (0.0, None))[0]:
                worst[k] = (v, RN.case_id(c))
    assert set(worst) == set(RN.FLOOR)
    for k, (v, where) in sorted(worst.items()):
        print("fp64 against long double, %s: worst %.3e at %s; the GPU bar is %.2e" % (k, v, where, RN.FACTOR * RN.FLOOR[k]))
        assert v <= RN.FLOOR[k], (k, v, where)
        assert v >= RN.FLOOR[k] / 4, "FLOOR[%s] is not what is measured here any more: %.3e" % (k, v)


@needs_ld
def test_the_floor_behind_the_chain_bar():
    """closed-form seeds and direct terms against those of autograd through the einsum form, the seeds pushed through the same NumPy
    reverse sweep of the roll-out"""
    import torch
    import _reach_rollout_grad_ref as RR
    worst = 0.0
    rho = RN.CHAIN_LAM_RHO[1]
    for n_s in (2, 4):
        T, H, n_u = 3, 4, 1
        gp = RR.NumpyGP(n_s, n_s + n_u, 30, seed=7)
        r = RR.rollout_inputs(n_s, n_u, T, H, seed=2)
        pa, qa = RR.forward(gp, r, H, False, None, np.float64)
        x = RN.chain_constants(n_s, n_u, T, H)
        x.update(p_all=np.asarray(pa, dtype=np.float64), q_all=np.asarray(qa, dtype=np.float64), k_ff=r["k_ff"], k_fb=r["k_fb"], q0=None, kfb0=None,
                 c=r["c"])
        g = RN.constraints(x)[0]
        z = x["lam"] + rho * g
        assert (z > 1e-6).any() and (z < -1e-6).any() and (np.abs(z) > 1e-6).all(), "the set-up needs active and inactive rows off the kink"
        closed = RN.vjp(x, RN.lagrangian_seed(g, x["lam"], rho))
        leaves = [torch.tensor(x[k], requires_grad=True) for k in ("p_all", "q_all", "k_ff", "k_fb")]
        auto = torch.autograd.grad(RN.torch_lagrangian(RN.torch_constraints(*leaves, x), torch.tensor(x["lam"]), rho), leaves)
        lins = RR.linearisations(gp, r, pa, H, None)
        g1 = RR.sweep(r, H, lins, pa, qa, closed["p_all_bar"], closed["q_all_bar"], False, None, fp64=True)
        g2 = RR.sweep(r, H, lins, pa, qa, auto[0].numpy(), auto[1].numpy(), False, None, fp64=True)
        worst = max(worst, RR.rel_err(g1["k_ff"] + closed["kff_bar"], g2["k_ff"] + auto[2].numpy()),
                    RR.rel_err(g1["k_fb"] + closed["kfb_bar"], g2["k_fb"] + auto[3].numpy()))
    print("closed-form seeds against autograd seeds through the same sweep: worst %.3e of the largest element; CHAIN_RTOL = %.2e"
          % (worst, RN.CHAIN_RTOL))
    assert worst <= RN.CHAIN_FLOOR
    assert worst >= RN.CHAIN_FLOOR / 4, "CHAIN_FLOOR is not what is measured here any more: %.3e" % worst
