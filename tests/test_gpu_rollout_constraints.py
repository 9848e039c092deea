"""The SafeMPC constraint rows on the device (sr_rollout_constraints, sr_rollout_constraints_vjp;
gp_reachability.rollout_constraints_batch / rollout_constraints_vjp_batch) against the long-double evaluation of
tests/_rollout_constraints_ref.py (the reference's unexpanded lin_ellipsoid_safety_distance, the control rows through the explicit
product K q K^T) at the same inputs.

CASES (_rollout_constraints_ref.CASES): n_s = 1, 2, 4, 5, 8, 9, 12 -- every width bucket of the reverse kernel (n_s <= 4, 8, 12;
workgroups of 64, 64, 32 threads) at and past its edge -- from a point and from (q0, k_fb0); n_u = 1, 2, 4, 12; H = 1 (the terminal
rows and the control rows of step 0 only, k_fb None), 2, 3, 15, 65 (past one wavefront: the owner thread takes the maximum over two
rounds); T = 1, 2, 63, 64, 65, 257, and T = 257 x H = 65; with and without bounds; m_obs = 0, 1, 5; m_safe = 0 (with obstacles), 1,
2 n_s; q full PSD with an antisymmetric part added (which must not count), rank 1, exactly zero; k_fb full, with a row of zeros, all
zero.  c_safety = 1.3.

BARS (30 x the floor of the fp64 reference against its long-double self on exactly these inputs, measured and asserted by
tests/test_rollout_constraints_host.py):
  g, g_max      30 x 2e-15 = 6e-14 of the row's scale |h| . |p| + c sqrt|h q h^T| + |h_vec|
  p_all_bar     30 x 4e-16 = 1.2e-14 of the largest element      q_all_bar   30 x 3e-15 = 9e-14      kff_bar    30 x 2e-16 = 6e-15
  kfb_bar       30 x 6e-16 = 1.8e-14      q0_bar   30 x 8e-15 = 2.4e-13      kfb0_bar   30 x 3e-15 = 9e-14
  (floors measured: g 1.50e-15, p_all_bar 3.03e-16, q_all_bar 2.47e-15, kff_bar 1.06e-16, kfb_bar 5.71e-16, q0_bar 7.93e-15,
  kfb0_bar 2.98e-15; the three largest at n_s = 2 with n_u = 4 gain rows, one of them close to the short axis of q0)
  chain         the gradient in k_ff, k_fb of the augmented Lagrangian sum (max(0, lam + rho g)^2 - lam^2) / (2 rho) on
                multistep_reachability_diff_batch (N = 60, n_s = 2 and 4, H = 4, T = 3) by the three raw calls against autograd
                through the einsum form on the same roll-out: 30 x 4e-16 = 1.2e-14 of the largest element (floor measured: 3.63e-16,
                the two routes in CPU torch at one stored forward).
Conditions, not tolerances: a zero radicand contributes exactly zero and leaves everything finite; a negative radicand gives NaN in
exactly the rows and gradient blocks of its own state; two calls equal; a trajectory alone and inside a batch of 257; with and
without g_max; g_max the exact maximum; the obstacle and terminal rows the bits of lin_ellipsoid_safety_distance_batch on the
symmetrised ellipsoids; q_all_bar, q0_bar symmetric; a zero g_bar gives zeros; outputs passed as NULL leave sentinel-filled
neighbours untouched; the autograd surface equals the raw calls.

Observed on MI355X (every share is printed): g at most 0.025 of the bar, g_max 0.003, p_all_bar 0.025, q_all_bar 0.021 (rank-1 q),
kff_bar 0.018, kfb_bar 0.020 (n_u = 12), q0_bar 0.039 and kfb0_bar 0.040 (n_s = 2 with n_u = 4, the case that sets their floors); the
chain 1.3e-16 and 4.3e-16 of the largest element at n_s = 2 and 4 (0.011 and 0.036 of the bar), with 50 of 63 and 70 of 75 rows
active and the closest 4.0e-3 from the kink.
"""
import ctypes

import numpy as np
import pytest

import _rollout_constraints_ref as RN
import _reach_rollout_grad_ref as RR
from _helpers import width_problem, width_gp

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e+300
GUARD = 64
LD = np.longdouble
REF_DTYPE = LD if np.finfo(LD).eps < np.finfo(np.float64).eps else np.float64


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


def _args(x, conv=lambda v: v):
    return (conv(x["p_all"]), conv(x["q_all"]), conv(x["k_ff"]), conv(x["k_fb"]), x["ctrl_bounds"], x["h_obs_mat"], x["h_obs"], x["h_safe_mat"],
            x["h_safe"], conv(x["q0"]), conv(x["kfb0"]), x["c"])


def _rows(x, **more):
    from safe_exploration_amd import gp_reachability as reach
    return reach.rollout_constraints_batch(*_args(x), **more)


def _vjp(x, g_bar=None):
    from safe_exploration_amd import gp_reachability as reach
    return dict(zip(RN.OUTS, reach.rollout_constraints_vjp_batch(*_args(x), g_bar=x["g_bar"] if g_bar is None else g_bar)))


def _same(u, v):
    return all((u[k] is None and v[k] is None) or np.array_equal(u[k], v[k], equal_nan=True) for k in u)


_REF = {}


def _ref(case):
    """inputs and the reference of a case: computed once, shared, left unchanged"""
    key = RN.case_id(case)
    if key not in _REF:
        x = RN.make_inputs(**case)
        _REF[key] = (x, RN.constraints(x, REF_DTYPE), RN.vjp(x, dtype=REF_DTYPE), RN.row_scale(x))
    return _REF[key]


@pytest.mark.parametrize("case", RN.CASES, ids=RN.case_id)
def test_rows_and_reverse_pass_against_the_reference(case):
    x, (g_ref, max_ref), v_ref, scale = _ref(case)
    g, g_max = _rows(x, return_max=True)
    v = _vjp(x)
    assert g.shape == (x["T"], x["n_g"]) and g_max.shape == (x["T"],) and np.isfinite(g).all()
    share = dict(g=RN.g_err(g, g_ref, scale) / (RN.FACTOR * RN.FLOOR["g"]),
                 g_max=RN.g_err(g_max, max_ref, scale.max(axis=1)) / (RN.FACTOR * RN.FLOOR["g"]))
    for k in RN.OUTS:
        if v_ref[k] is None or not v_ref[k].size:
            assert v[k] is None or not v[k].size, k
            continue
        assert v[k].shape == v_ref[k].shape and np.isfinite(v[k]).all(), k
        share[k] = RN.rel_err(v[k], v_ref[k]) / (RN.FACTOR * RN.FLOOR[k])
    print("%s: share of the bar used %s" % (RN.case_id(case), {k: "%.3f" % s for k, s in share.items()}))
    assert np.array_equal(g_max, g.max(axis=1)), "g_max is not the largest returned row"
    assert np.array_equal(v["q_all_bar"], v["q_all_bar"].transpose(0, 1, 3, 2)), "q_all_bar is not symmetric"
    if v["q0_bar"] is not None:
        assert np.array_equal(v["q0_bar"], v["q0_bar"].transpose(0, 2, 1)), "q0_bar is not symmetric"
    assert all(s <= 1.0 for s in share.values()), share


# ---- zero and negative radicands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ("point", "q0"))
def test_a_zero_radicand_contributes_exactly_zero(start):
    n_u, H = 2, 3
    x = RN.make_inputs(4, n_u=n_u, T=2, H=H, m_obs=1, m_safe=1, start=start, kkind="zero_row", seed=3)
    v = _vjp(x)
    assert all(np.isfinite(a).all() for a in v.values() if a is not None)
    assert not v["kfb_bar"][:, 0, n_u - 1].any() and v["kfb_bar"][:, 0, 0].all() and v["kfb_bar"][:, 1].all()
    other = x["g_bar"].copy()
    other[:, 2 * n_u * 1 + (n_u - 1)] += 3.0                                   # the upper seed of the zero row's output, step 1
    other[:, 2 * n_u * 1 + n_u + (n_u - 1)] -= 1.0                             # and the lower
    v2 = _vjp(x, other)
    assert np.array_equal(v2["q_all_bar"], v["q_all_bar"]) and np.array_equal(v2["kfb_bar"], v["kfb_bar"]), "a zero row's seed reached q or k_fb"
    assert not np.array_equal(v2["kff_bar"], v["kff_bar"])
    if start == "q0":
        assert not v["kfb0_bar"][:, n_u - 1].any() and v["kfb0_bar"][:, 0].all()
    for kind in (dict(kkind="zero"), dict(qkind="zero"), dict(kkind="zero", qkind="zero")):
        z = RN.make_inputs(4, n_u=n_u, T=2, H=H, m_obs=1, m_safe=1, start=start, seed=3, **kind)
        g, g_max = _rows(z, return_max=True)
        vz = _vjp(z)
        assert np.isfinite(g).all() and np.isfinite(g_max).all() and all(np.isfinite(a).all() for a in vz.values() if a is not None), kind
        assert not vz["kfb_bar"].any(), kind                                   # k = 0: the subgradient 0;  q = 0: Q k = 0
        assert vz["p_all_bar"].any() and vz["kff_bar"].any()
        if "qkind" in kind:
            assert not vz["q_all_bar"].any() and (start == "point" or not vz["q0_bar"].any()), kind
            up = z["k_ff"] - z["ctrl_bounds"][:, 1]                            # every square root is exactly zero: the point's rows
            assert np.array_equal(g[:, :2 * n_u * H].reshape(2, H, 2, n_u)[:, :, 0], up)
        else:
            assert vz["q_all_bar"].any()                                       # (the state rows still read q)


def test_a_negative_radicand_gives_nan_in_its_own_state_only():
    n_u, H, T, tb, ib, m_obs = 2, 3, 5, 2, 1, 5
    x = RN.make_inputs(4, n_u=n_u, T=T, H=H, m_obs=m_obs, m_safe=1, start="q0", seed=4)
    bad = dict(x, q_all=x["q_all"].copy())
    bad["q_all"][tb, ib] = -np.eye(4) - 0.1
    g0, m0 = _rows(x, return_max=True)
    g, g_max = _rows(bad, return_max=True)
    rows = np.zeros(x["n_g"], dtype=bool)
    rows[2 * n_u * (ib + 1):2 * n_u * (ib + 2)] = True                         # the control rows of step ib + 1
    rows[2 * n_u * H + m_obs * ib:2 * n_u * H + m_obs * (ib + 1)] = True       # the obstacle rows of state ib
    assert np.isnan(g[tb, rows]).all() and np.isfinite(g[tb, ~rows]).all() and np.isnan(g_max[tb])
    keep = np.arange(T) != tb
    assert np.array_equal(g[keep], g0[keep]) and np.array_equal(g_max[keep], m0[keep]) and np.array_equal(g[tb, ~rows], g0[tb, ~rows])
    v0, v = _vjp(x), _vjp(bad)
    assert np.isnan(v["q_all_bar"][tb, ib]).all() and np.isnan(v["kfb_bar"][tb, ib]).all()
    for k in RN.OUTS:
        a = v[k].copy()
        if k in ("q_all_bar", "kfb_bar"):
            a[tb, ib] = v0[k][tb, ib]
        assert np.array_equal(a, v0[k]), "%s: NaN or other bits outside the bad state" % k


# ---- bit-level conditions -----------------------------------------------------------------------------------------------------------
BIT_CASES = [dict(n_s=4, n_u=1, T=257, H=15, m_obs=5, m_safe="2n", start="q0", seed=11), dict(n_s=4, n_u=2, T=257, H=65, m_obs=1, m_safe=1, seed=11),
             dict(n_s=7, n_u=4, T=257, H=3, m_obs=5, m_safe=0, start="q0", seed=11), dict(n_s=12, n_u=12, T=257, H=2, m_obs=1, m_safe="2n", seed=11),
             dict(n_s=3, n_u=2, T=257, H=5, bounds=False, m_obs=5, m_safe=1, start="q0", seed=11)]


@pytest.mark.parametrize("case", BIT_CASES, ids=RN.case_id)
def test_bit_level_conditions(case):
    import torch
    from safe_exploration_amd import gp_reachability as reach
    x = RN.make_inputs(**case)
    T, H, n_s, n_u = x["T"], x["H"], x["n_s"], x["n_u"]
    g, g_max = _rows(x, return_max=True)
    v = _vjp(x)
    g2, g_max2 = _rows(x, return_max=True)
    assert np.array_equal(g, g2) and np.array_equal(g_max, g_max2) and _same(v, _vjp(x)), "two calls differ"
    assert np.array_equal(g, _rows(x)), "without g_max the rows have other bits"
    assert np.array_equal(g_max, g.max(axis=1))
    per = ("p_all", "q_all", "k_ff", "k_fb", "q0", "kfb0", "g_bar")
    for t in (0, 63, 64, 256):                                                 # alone and inside the batch of 257
        xs = dict(x, T=1, **{k: (None if x[k] is None else x[k][t:t + 1]) for k in per})
        g1, m1 = _rows(xs, return_max=True)
        assert np.array_equal(g1, g[t:t + 1]) and np.array_equal(m1, g_max[t:t + 1]), t
        v1 = _vjp(xs)
        assert all(v[k] is None or np.array_equal(v1[k], v[k][t:t + 1]) for k in RN.OUTS), t
    # the obstacle and terminal rows are sr_safety_distance on the symmetrised ellipsoids, bit for bit
    qs = 0.5 * (x["q_all"] + x["q_all"].transpose(0, 1, 3, 2))
    at = 2 * n_u * H if x["bounds"] else 0
    if x["m_obs"]:
        d = reach.lin_ellipsoid_safety_distance_batch(x["p_all"][:, :-1].reshape(-1, n_s), qs[:, :-1].reshape(-1, n_s, n_s), x["h_obs_mat"], x["h_obs"], x["c"])
        assert np.array_equal(d.reshape(T, -1), g[:, at:at + x["m_obs"] * (H - 1)]), "obstacle rows are not sr_safety_distance's bits"
        at += x["m_obs"] * (H - 1)
    if x["m_safe"]:
        d = reach.lin_ellipsoid_safety_distance_batch(x["p_all"][:, -1], qs[:, -1], x["h_safe_mat"], x["h_safe"], x["c"])
        assert np.array_equal(d, g[:, at:]), "terminal rows are not sr_safety_distance's bits"
    assert np.array_equal(v["q_all_bar"], v["q_all_bar"].transpose(0, 1, 3, 2))
    assert v["q0_bar"] is None or np.array_equal(v["q0_bar"], v["q0_bar"].transpose(0, 2, 1))
    vz = _vjp(x, np.zeros_like(x["g_bar"]))
    assert all(a is None or not a.any() for a in vz.values()), "a zero g_bar does not give zero outputs"
    if not x["bounds"]:
        assert not v["kff_bar"].any() and not v["kfb_bar"].any() and not v["kfb0_bar"].any() and not v["q0_bar"].any()
    # tensors in, tensors out, the same bits; the autograd surface is the plain call and its backward the raw reverse pass
    gt = reach.rollout_constraints_batch(*_args(x, _t))
    assert torch.is_tensor(gt) and np.array_equal(gt.cpu().numpy(), g)
    leaves = {k: _t(x[k]).requires_grad_(True) for k in ("p_all", "q_all", "k_ff", "k_fb", "q0", "kfb0") if x[k] is not None}
    xa = dict(x, **leaves)
    gd, md = reach.rollout_constraints_batch(*_args(xa), return_max=True, differentiable=True)
    assert torch.equal(gd.detach(), gt) and np.array_equal(md.cpu().numpy(), g_max) and gd.requires_grad and not md.requires_grad
    names = list(leaves)
    grads = dict(zip(names, torch.autograd.grad((gd * _t(x["g_bar"])).sum(), [leaves[k] for k in names])))
    for name, out in (("p_all", "p_all_bar"), ("q_all", "q_all_bar"), ("k_ff", "kff_bar"), ("k_fb", "kfb_bar"), ("q0", "q0_bar"), ("kfb0", "kfb0_bar")):
        if name in grads:
            assert np.array_equal(grads[name].cpu().numpy(), v[out]), "autograd and the raw reverse pass differ in " + out


# ---- through the C ABI into sentinel-filled buffers ---------------------------------------------------------------------------------
class _Abi(object):
    """sr_rollout_constraints / sr_rollout_constraints_vjp with every output inside a sentinel-filled buffer, GUARD doubles in front
    and behind"""
    INS = ("p_all", "q_all", "k_ff", "k_fb", "q0", "kfb0", "u_min", "u_max", "h_obs_mat", "h_obs", "h_safe_mat", "h_safe", "g_bar")

    def __init__(self, x):
        self.x = x
        T, H, n_s, n_u = x["T"], x["H"], x["n_s"], x["n_u"]
        cb = x["ctrl_bounds"]
        host = dict(x, u_min=None if cb is None else cb[:, 0], u_max=None if cb is None else cb[:, 1])
        self.d = {k: _t(host[k]) for k in self.INS}
        ell = x["q0"] is not None
        self.shapes = dict(g=(T, x["n_g"]), g_max=(T,), p_all_bar=(T, H, n_s), q_all_bar=(T, H, n_s, n_s), kff_bar=(T, H, n_u),
                           kfb_bar=(T, H - 1, n_u, n_s), q0_bar=(T, n_s, n_s) if ell else (0,), kfb0_bar=(T, n_u, n_s) if ell else (0,))

    def call(self, reverse, drop=(), **over):
        """(status, outputs); `drop`: outputs, and inputs as "in:<name>", passed as NULL; over: scalar arguments replaced"""
        import torch
        from safe_exploration_amd import _buffers as B
        from safe_exploration_amd._lib import lib
        x, d = self.x, self.d
        names = RN.OUTS if reverse else ("g", "g_max")
        bufs = {k: torch.full((int(np.prod(self.shapes[k])) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=_dev()) for k in names}
        optr = lambda k: None if (k in drop or not int(np.prod(self.shapes[k]))) else ctypes.c_void_p(bufs[k].data_ptr() + 8 * GUARD)
        iptr = lambda k: None if ("in:" + k in drop or d[k] is None or not d[k].numel()) else B.ptr(d[k])
        s = dict(device=0, T=x["T"], H=x["H"], n_s=x["n_s"], n_u=x["n_u"], m_obs=x["m_obs"], m_safe=x["m_safe"], c=x["c"])
        s.update(over)
        head = (s["device"], s["T"], s["H"], s["n_s"], s["n_u"], iptr("p_all"), iptr("q_all"), iptr("k_ff"), iptr("k_fb"), iptr("q0"), iptr("kfb0"),
                iptr("u_min"), iptr("u_max"), s["m_obs"], iptr("h_obs_mat"), iptr("h_obs"), s["m_safe"], iptr("h_safe_mat"), iptr("h_safe"), s["c"])
        if reverse:
            rc = lib.sr_rollout_constraints_vjp(*head, iptr("g_bar"), *[optr(k) for k in names], B.stream_ptr(_dev()))
        else:
            rc = lib.sr_rollout_constraints(*head, *[optr(k) for k in names], B.stream_ptr(_dev()))
        torch.cuda.synchronize()
        out = {}
        for k in names:
            flat, n = bufs[k].cpu().numpy(), int(np.prod(self.shapes[k]))
            assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all(), "%s: written outside" % k
            out[k] = flat[GUARD:GUARD + n].reshape(self.shapes[k])
        return rc, out


MAIN = RN.OUTS[:4]


@pytest.mark.parametrize("case", (dict(n_s=4, n_u=1, T=65, H=15, m_obs=5, m_safe="2n", start="q0"), dict(n_s=12, n_u=4, T=5, H=3, m_obs=1, m_safe=1),
                                  dict(n_s=2, n_u=2, T=3, H=65, m_obs=1, m_safe=0, start="q0"), dict(n_s=5, n_u=1, T=3, H=1, m_obs=0, m_safe=1, start="q0")),
                         ids=RN.case_id)
def test_c_abi_bounds_null_outputs_and_t_zero(case):
    x = RN.make_inputs(**case)
    abi = _Abi(x)
    rc, fwd = abi.call(False)
    assert rc == 0 and not any((a == SENTINEL).any() for a in fwd.values())
    g, g_max = _rows(x, return_max=True)
    assert np.array_equal(fwd["g"], g) and np.array_equal(fwd["g_max"], g_max), "the wrapper and the C ABI differ"
    rc, only = abi.call(False, drop=("g_max",))
    assert rc == 0 and np.array_equal(only["g"], g) and (only["g_max"] == SENTINEL).all()
    rc, rev = abi.call(True)
    assert rc == 0 and not any((a == SENTINEL).any() for a in rev.values())
    v = _vjp(x)
    assert all(np.array_equal(rev[k].reshape(-1), (np.zeros(0) if v[k] is None else v[k]).reshape(-1)) for k in RN.OUTS), "the wrapper and the C ABI differ"
    live = [k for k in MAIN if int(np.prod(abi.shapes[k]))]
    for keep in live:                                                          # one main output at a time, the others NULL and untouched
        rc, part = abi.call(True, drop=tuple(k for k in MAIN if k != keep))
        assert rc == 0 and np.array_equal(part[keep], rev[keep]), keep
        assert all((part[k] == SENTINEL).all() for k in MAIN if k != keep), keep
        assert np.array_equal(part["q0_bar"], rev["q0_bar"]) and np.array_equal(part["kfb0_bar"], rev["kfb0_bar"]), keep
    for reverse in (False, True):
        rc, none = abi.call(reverse, T=0)
        assert rc == 0 and all((a == SENTINEL).all() for a in none.values()), "T == 0 wrote something"


def test_refusals_through_the_raw_abi():
    from safe_exploration_amd._lib import SR_EINVAL, SR_EUNSUPPORTED, last_error
    ell = _Abi(RN.make_inputs(4, n_u=2, T=3, H=3, m_obs=1, m_safe=1, start="q0"))
    h1 = _Abi(RN.make_inputs(4, n_u=2, T=3, H=1, m_obs=0, m_safe=1, start="q0"))
    untouched = lambda out: all((a == SENTINEL).all() for a in out.values())
    only_bounds = ("in:h_obs_mat", "in:h_obs", "in:h_safe_mat", "in:h_safe")
    for reverse, name in ((False, "sr_rollout_constraints"), (True, "sr_rollout_constraints_vjp")):
        for who, kw, want in ((ell, dict(drop=("in:p_all",)), SR_EINVAL), (ell, dict(drop=("in:q_all",)), SR_EINVAL), (ell, dict(drop=("in:k_ff",)), SR_EINVAL),
                              (ell, dict(drop=("in:k_fb",)), SR_EINVAL), (ell, dict(drop=("in:q0",)), SR_EINVAL), (ell, dict(drop=("in:kfb0",)), SR_EINVAL),
                              (ell, dict(drop=("in:u_min",)), SR_EINVAL), (ell, dict(drop=("in:u_max",)), SR_EINVAL), (ell, dict(m_obs=-1), SR_EINVAL),
                              (ell, dict(m_safe=-1), SR_EINVAL), (ell, dict(drop=("in:h_obs_mat",)), SR_EINVAL), (ell, dict(drop=("in:h_obs",)), SR_EINVAL),
                              (ell, dict(drop=("in:h_safe_mat",)), SR_EINVAL), (ell, dict(drop=("in:h_safe",)), SR_EINVAL),
                              (ell, dict(drop=("in:u_min", "in:u_max") + only_bounds, m_obs=0, m_safe=0), SR_EINVAL),
                              (h1, dict(drop=("in:u_min", "in:u_max", "in:h_safe_mat", "in:h_safe"), m_obs=1, m_safe=0), SR_EINVAL),
                              (ell, dict(T=-1), SR_EINVAL), (ell, dict(H=0), SR_EINVAL), (ell, dict(n_s=0), SR_EINVAL), (ell, dict(n_u=0), SR_EINVAL),
                              (ell, dict(n_s=13), SR_EUNSUPPORTED), (ell, dict(n_u=13), SR_EUNSUPPORTED)):
            rc, out = who.call(reverse, **kw)
            assert rc == want and untouched(out), (name, kw, rc)
            assert last_error().startswith(name + ":"), (name, kw, last_error())
    rc, out = ell.call(False, drop=("g",))
    assert rc == SR_EINVAL and untouched(out) and last_error().startswith("sr_rollout_constraints:")
    for drop in (("in:g_bar",), MAIN, ("q0_bar",), ("kfb0_bar",)):
        rc, out = ell.call(True, drop=drop)
        assert rc == SR_EINVAL and untouched(out) and last_error().startswith("sr_rollout_constraints_vjp:"), drop
    rc, out = h1.call(True, drop=("in:k_fb", "kfb_bar"))                        # H == 1: k_fb and kfb_bar NULL are fine
    assert rc == 0 and not (out["q0_bar"] == SENTINEL).any()
    from safe_exploration_amd import gp_reachability as reach
    x = ell.x
    with pytest.raises(ValueError):
        reach.rollout_constraints_batch(x["p_all"], x["q_all"][:, :2], x["k_ff"], x["k_fb"], x["ctrl_bounds"])
    with pytest.raises(ValueError):
        reach.rollout_constraints_vjp_batch(*_args(x), g_bar=np.ones((3, x["n_g"] + 1)))
    with pytest.raises(ValueError):
        reach.rollout_constraints_vjp_batch(*_args(x))
    with pytest.raises(NotImplementedError):
        reach.rollout_constraints_batch(np.zeros((2, 2, 13)), np.zeros((2, 2, 13, 13)), None, None, h_mat_safe=np.ones((1, 13)), h_safe=np.ones(1))


# ---- the chain: the augmented Lagrangian's gradient in k_ff, k_fb ---------------------------------------------------------------------
@pytest.mark.parametrize("n_s", (2, 4))
def test_the_chain_against_autograd_through_the_einsum_form_and_the_three_raw_calls(n_s):
    import torch
    from safe_exploration_amd import gp_reachability as reach
    T, H, n_u = 3, 4, 1
    gp = width_gp(width_problem(900 + n_s, "rbf", n_s + 1, 60, n_s))
    r = RR.rollout_inputs(n_s, n_u, T, H, seed=2)
    x = RN.chain_constants(n_s, n_u, T, H)
    x["c"] = r["c"]
    lam, rho = _t(x["lam"]), RN.CHAIN_LAM_RHO[1]
    sets = (x["ctrl_bounds"], x["h_obs_mat"], x["h_obs"], x["h_safe_mat"], x["h_safe"], None, None, x["c"])
    grads = {}
    for which in ("device", "einsum"):
        leaves = dict(k_ff=_t(r["k_ff"]).requires_grad_(True), k_fb=_t(r["k_fb"]).requires_grad_(True))
        p_all, q_all = reach.multistep_reachability_diff_batch(_t(r["p"]), gp, leaves["k_fb"], leaves["k_ff"], r["l_mu"], r["l_sigma"], None, r["c"],
                                                               r["a"], r["b"])
        if which == "device":
            g = reach.rollout_constraints_batch(p_all, q_all, leaves["k_ff"], leaves["k_fb"], *sets, differentiable=True)
            stored = (p_all.detach(), q_all.detach(), g.detach())
            assert torch.equal(stored[2], reach.rollout_constraints_batch(stored[0], stored[1], leaves["k_ff"].detach(), leaves["k_fb"].detach(), *sets))
            z = (lam + rho * stored[2]).cpu().numpy()
            print("n_s=%d: %d of %d rows active, closest to the kink %.2e" % (n_s, int((z > 0).sum()), z.size, np.abs(z).min()))
            assert (z > 1e-6).any() and (z < -1e-6).any() and (np.abs(z) > 1e-6).all(), "the set-up needs active and inactive rows off the kink"
        else:
            g = RN.torch_constraints(p_all, q_all, leaves["k_ff"], leaves["k_fb"], x)
        grads[which] = torch.autograd.grad(RN.torch_lagrangian(g, lam, rho), [leaves["k_ff"], leaves["k_fb"]])
    err = max(RR.rel_err(d.cpu().numpy(), e.cpu().numpy()) for d, e in zip(grads["device"], grads["einsum"]))
    print("n_s=%d: the device rows against the einsum form, gradient in k_ff, k_fb: %.3e of the largest element, share of the bar %.3f"
          % (n_s, err, err / RN.CHAIN_RTOL))
    # the three raw calls: roll-out (stored above), the constraints' reverse pass, the roll-out's reverse pass, plus the direct terms
    kff, kfb = _t(r["k_ff"]), _t(r["k_fb"])
    seed = torch.relu(lam + rho * stored[2])
    cv = reach.rollout_constraints_vjp_batch(stored[0], stored[1], kff, kfb, *sets, g_bar=seed)
    raw = reach.multistep_reachability_vjp_batch(_t(r["p"]), gp, kfb, kff, r["l_mu"], r["l_sigma"], stored[0], stored[1], cv[0], cv[1], None, r["c"],
                                                 r["a"], r["b"])
    assert torch.equal(raw[3] + cv[2], grads["device"][0]) and torch.equal(raw[4].reshape(kfb.shape) + cv[3], grads["device"][1]), \
        "the three raw calls and the autograd surface differ"
    assert err <= RN.CHAIN_RTOL, err
