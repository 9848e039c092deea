"""The roll-out cost on the device (sr_rollout_cost, sr_rollout_cost_vjp; utils_casadi.rollout_cost_batch / rollout_cost_vjp_batch)
against the long-double evaluation of tests/_rollout_cost_ref.py (the reference's unexpanded expressions: explicit inverse and
determinant, E[.^2] - E[.]^2) at the same inputs.

CASES (_rollout_cost_ref.CASES): n_s = 1 .. 12, each with no angle / the angle dropped / kept, both losses -- augmented widths
n_c = 1 .. 14, i.e. every width bucket of the kernel below and AT its edge: the buckets are n_c <= 4, <= 6, <= 10, <= 14 (workgroups
of 64, 64, 32, 16 threads) --; the angle first, in the middle, last; a = 0.7; the cart-pole regime (n_s = 4, angle 2 dropped, the
reference's singular W = diag(20, 0, 0, 0, 5) / 100) at H = 1 (the terminal term only), 2, 3, 15, 65 (past one wavefront: the
owner thread adds over two rounds) and T = 1, 2, 63, 64, 65, 257, and T = 257 x H = 65; sigma None / zero / rank 1 / full (with an
antisymmetric part, which must not count); W None / singular diagonal / dense PSD of rank 2; R, u absent and present.

BARS (30 x the floor of the fp64 reference against its long-double self on exactly these inputs, measured and asserted by
tests/test_rollout_cost_host.py):
  cost_steps, cost    30 x 5e-16 = 1.5e-14 at the scale of the quantity (w for the saturating loss, w |W| (|d|^2 + |v|) for the
                      quadratic, plus |R| |u|^2; H times that for the total)
  mu_bar              30 x 5e-15 = 1.5e-13 of the largest element      sigma_bar   30 x 1e-14 = 3e-13
  u_bar               30 x 3e-16 = 9e-15
  at the target       (m = z after the augmentation, v of 3e-8: a cost of 1e-9) RELATIVE 1e-8 (_rollout_cost_ref: what the long-double
                      reference itself is good for there, a tenth of what fp64 without expm1 / log1p reaches)
  chain               the gradient in k_ff, k_fb of the cost on multistep_moments_diff_batch (modes 1, 2) and on
                      moment_matching_rollout_diff_batch (N = 60, n_s = 2 and 4, H = 4, T = 3) against autograd through the torch
                      port of the cost on the same roll-out: 30 x 6e-16 = 1.8e-14 of the largest element, the disagreement of
                      the two routes in CPU torch at one stored forward (the host test).
Bit-level conditions (conditions, not tolerances): cost == the in-order sum of cost_steps; two calls equal; with and without
cost_steps; a trajectory alone and inside a batch of 257; sigma_bar == sigma_bar^T; u_bar[:, H-1] == 0; cost_bar None == ones;
sigma None == zeros; outputs passed as NULL leave sentinel-filled neighbours untouched; the three raw calls (roll-out, cost VJP,
roll-out VJP) equal the autograd surface.

Observed on MI355X (every share is printed): cost_steps at most 0.033 of the bar, cost 0.012, mu_bar 0.035 (n_s = 8, the angle kept),
sigma_bar 0.032 (n_s = 10, the angle kept), u_bar 0.030; at the target a cost of 3.3e-9 within 2.4e-10 of itself (the fp64 reference:
3.4e-7); the chain 2.8e-16 .. 1.5e-15 of the largest element on the Taylor and mean-equivalent roll-outs, 3.6e-15 and 8.0e-15 on the
moment-matching roll-out at n_s = 2 and 4 (0.20 and 0.45 of the bar).
"""
import ctypes

import numpy as np
import pytest

import _rollout_cost_ref as RC
import _moments_rollout_grad_ref as MR
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


def _kw(x):
    return dict(z=x["z"], W=x["W"], R=x["R"], idx_angle=x["idx"], a=x["a"], keep_radian=x["keep"], loss=x["loss"], w_stage=x["w_stage"],
                w_term=x["w_term"])


def _cost(x, **more):
    from safe_exploration_amd import utils_casadi as uc
    return uc.rollout_cost_batch(x["mu"], x["sigma"], u=x["u"], **dict(_kw(x), **more))


def _vjp(x, cost_bar="own"):
    from safe_exploration_amd import utils_casadi as uc
    g = uc.rollout_cost_vjp_batch(x["mu"], x["sigma"], u=x["u"], cost_bar=x["cost_bar"] if isinstance(cost_bar, str) else cost_bar, **_kw(x))
    return dict(zip(RC.OUTS, g))


def _in_order_sum(steps):
    total = np.zeros(steps.shape[0])
    for i in range(steps.shape[1]):
        total = total + steps[:, i]
    return total


_REF = {}


def _ref(case):
    """inputs and the reference of a case: computed once, shared, left unchanged"""
    key = RC.case_id(case)
    if key not in _REF:
        x = RC.make_inputs(**case)
        _REF[key] = (x, RC.cost(x, REF_DTYPE), RC.vjp(x, x["cost_bar"], REF_DTYPE))
    return _REF[key]


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_cost_and_reverse_pass_against_the_reference(case):
    x, (steps_ref, cost_ref), g_ref = _ref(case)
    cost, steps = _cost(x, return_steps=True)
    g = _vjp(x)
    scale = RC.cost_scale(x)
    share = dict(steps=float(np.max(np.abs(steps - steps_ref))) / scale / (RC.FACTOR * RC.FLOOR["cost"]),
                 cost=float(np.max(np.abs(cost - cost_ref))) / (scale * x["H"]) / (RC.FACTOR * RC.FLOOR["cost"]))
    for k in RC.OUTS:
        if g_ref[k] is None:
            assert g[k] is None
            continue
        assert g[k].shape == g_ref[k].shape and np.isfinite(g[k]).all(), k
        share[k] = RC.rel_err(g[k], g_ref[k]) / (RC.FACTOR * RC.FLOOR[k])
    print("%s: share of the bar used %s" % (RC.case_id(case), {k: "%.3f" % v for k, v in share.items()}))
    assert np.array_equal(cost, _in_order_sum(steps)), "cost is not the in-order sum of cost_steps"
    assert np.array_equal(g["sigma_bar"], g["sigma_bar"].transpose(0, 1, 3, 2)), "sigma_bar is not symmetric"
    if g["u_bar"] is not None:
        assert not g["u_bar"][:, -1].any(), "u_bar[:, H-1] is not zero"
    assert all(v <= 1.0 for v in share.values()), share


def test_at_the_target_the_cost_keeps_its_digits():
    if REF_DTYPE is np.float64:
        pytest.skip("np.longdouble is no wider than float64 here")
    x = RC.target_inputs()
    steps_ref, cost_ref = RC.cost(x, LD)
    cost, steps = _cost(x, return_steps=True)
    rel = max(float(np.max(np.abs(steps / steps_ref - 1))), float(np.max(np.abs(cost / cost_ref - 1))))
    print("at the target: cost %.3e .. %.3e, relative error %.2e (bar %.0e)" % (cost.min(), cost.max(), rel, RC.TARGET_RTOL))
    assert 1e-10 < cost.min() and cost.max() < 1e-8
    assert rel <= RC.TARGET_RTOL
    # (no bar on mu_bar here: at d = 0 it is W d with d the rounding of z, 1e-16, beside terms of 1e-11 -- noise in any arithmetic)
    g, g_ref = _vjp(x), RC.vjp(x, x["cost_bar"], LD)
    assert RC.rel_err(g["sigma_bar"], g_ref["sigma_bar"]) <= RC.FACTOR * RC.FLOOR["sigma_bar"]


# ---- bit-level conditions -----------------------------------------------------------------------------------------------------------
BIT_CASES = [dict(n_s=4, aug="drop", T=257, H=15, wkind="diag", seed=11), dict(n_s=4, aug="drop", T=257, H=65, wkind="diag", loss="quadratic", seed=11),
             dict(n_s=7, aug="keep", T=257, H=3, wkind="dense2", seed=11), dict(n_s=12, aug="keep", T=257, H=2, wkind="dense2", seed=11),
             dict(n_s=3, aug="none", T=257, H=5, wkind="none", seed=11)]


def _same(u, v):
    return all((u[k] is None and v[k] is None) or np.array_equal(u[k], v[k]) for k in u)


@pytest.mark.parametrize("case", BIT_CASES, ids=RC.case_id)
def test_bit_level_conditions(case):
    x = RC.make_inputs(**case)
    cost, steps = _cost(x, return_steps=True)
    g = _vjp(x)
    assert np.array_equal(cost, _in_order_sum(steps))
    cost2, steps2 = _cost(x, return_steps=True)
    assert np.array_equal(cost, cost2) and np.array_equal(steps, steps2) and _same(g, _vjp(x)), "two calls differ"
    assert np.array_equal(cost, _cost(x)), "without cost_steps the cost has other bits"
    for t in (0, 63, 64, 256):                                                 # alone and inside the batch of 257
        xs = dict(x, mu=x["mu"][t:t + 1], sigma=x["sigma"][t:t + 1], u=x["u"][t:t + 1], cost_bar=x["cost_bar"][t:t + 1])
        c1, s1 = _cost(xs, return_steps=True)
        assert np.array_equal(c1, cost[t:t + 1]) and np.array_equal(s1, steps[t:t + 1]), t
        g1 = _vjp(xs)
        assert all(np.array_equal(g1[k], g[k][t:t + 1]) for k in RC.OUTS), t
    assert _same(_vjp(x, None), _vjp(x, np.ones(x["T"]))), "cost_bar None is not an array of ones"
    x0, xz = dict(x, sigma=None), dict(x, sigma=np.zeros_like(x["sigma"]))
    assert np.array_equal(_cost(x0), _cost(xz)) and _same(_vjp(x0), _vjp(xz)), "sigma None is not a zero array"
    s0 = _vjp(x0)["sigma_bar"]
    assert np.array_equal(s0, s0.transpose(0, 1, 3, 2)) and s0.any()
    assert np.array_equal(g["sigma_bar"], g["sigma_bar"].transpose(0, 1, 3, 2)) and not g["u_bar"][:, -1].any()
    # tensors in, tensors out, the same bits
    import torch
    from safe_exploration_amd import utils_casadi as uc
    ct = uc.rollout_cost_batch(_t(x["mu"]), _t(x["sigma"]), u=_t(x["u"]), **_kw(x))
    assert torch.is_tensor(ct) and np.array_equal(ct.cpu().numpy(), cost)


# ---- through the C ABI into sentinel-filled buffers ---------------------------------------------------------------------------------
class _Abi(object):
    """sr_rollout_cost / sr_rollout_cost_vjp with every output inside a sentinel-filled buffer, GUARD doubles in front and behind"""

    def __init__(self, x):
        from safe_exploration_amd.utils_casadi import factor_weight
        self.x = x
        self.T, self.H, self.n_s = x["mu"].shape
        self.n_u = 0 if x["u"] is None else x["u"].shape[2]
        n_c = RC.n_aug(self.n_s, x["idx"], x["keep"])
        self.d = {k: _t(x[k]) for k in ("mu", "sigma", "u", "R", "z", "cost_bar")}
        self.d["F"] = _t(factor_weight(x["W"], n_c))
        T, H, n_s, n_u = self.T, self.H, self.n_s, self.n_u
        self.shapes = dict(cost=(T,), cost_steps=(T, H), mu_bar=(T, H, n_s), sigma_bar=(T, H, n_s, n_s), u_bar=(T, H, n_u))

    def call(self, reverse, drop=(), **over):
        """(status, outputs); `drop`: outputs, and inputs as "in:<name>", passed as NULL; over: scalar arguments replaced"""
        import torch
        from safe_exploration_amd import _buffers as B
        from safe_exploration_amd._lib import lib
        x, d = self.x, self.d
        names = ("mu_bar", "sigma_bar", "u_bar") if reverse else ("cost", "cost_steps")
        bufs = {k: torch.full((int(np.prod(self.shapes[k])) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=_dev()) for k in names}
        optr = lambda k: None if (k in drop or not int(np.prod(self.shapes[k]))) else ctypes.c_void_p(bufs[k].data_ptr() + 8 * GUARD)
        iptr = lambda k: None if "in:" + k in drop else B.ptr(d[k])
        s = dict(device=0, T=self.T, H=self.H, n_s=self.n_s, n_u=self.n_u, idx=-1 if x["idx"] is None else x["idx"], a=x["a"],
                 keep=int(x["keep"]), loss=RC_LOSS[x["loss"]], w_stage=x["w_stage"], w_term=x["w_term"])
        s.update(over)
        head = (s["device"], s["T"], s["H"], s["n_s"], s["n_u"], s["idx"], s["a"], s["keep"], s["loss"], iptr("z"), iptr("F"), s["w_stage"],
                s["w_term"], iptr("R"), iptr("mu"), iptr("sigma"), iptr("u"))
        if reverse:
            rc = lib.sr_rollout_cost_vjp(*head, iptr("cost_bar"), *[optr(k) for k in names], B.stream_ptr(_dev()))
        else:
            rc = lib.sr_rollout_cost(*head, *[optr(k) for k in names], B.stream_ptr(_dev()))
        torch.cuda.synchronize()
        out = {}
        for k in names:
            flat, n = bufs[k].cpu().numpy(), int(np.prod(self.shapes[k]))
            assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all(), "%s: written outside" % k
            out[k] = flat[GUARD:GUARD + n].reshape(self.shapes[k])
        return rc, out


RC_LOSS = dict(sat=0, quadratic=1)


@pytest.mark.parametrize("case", (dict(n_s=4, aug="drop", T=65, H=15, wkind="diag"), dict(n_s=12, aug="keep", T=5, H=3), dict(n_s=2, aug="none", T=3, H=65)),
                         ids=RC.case_id)
def test_c_abi_bounds_null_outputs_and_t_zero(case):
    x = RC.make_inputs(**case)
    abi = _Abi(x)
    rc, fwd = abi.call(False)
    assert rc == 0 and not any((v == SENTINEL).any() for v in fwd.values())
    cost, steps = _cost(x, return_steps=True)
    assert np.array_equal(fwd["cost"], cost) and np.array_equal(fwd["cost_steps"], steps), "the wrapper and the C ABI differ"
    rc, only = abi.call(False, drop=("cost_steps",))
    assert rc == 0 and np.array_equal(only["cost"], cost) and (only["cost_steps"] == SENTINEL).all()
    rc, rev = abi.call(True)
    assert rc == 0 and not any((v == SENTINEL).any() for v in rev.values())
    assert _same(rev, _vjp(x)), "the wrapper and the C ABI differ"
    for keep in RC.OUTS:                                                       # one output at a time, the other two NULL and untouched
        rc, part = abi.call(True, drop=tuple(k for k in RC.OUTS if k != keep))
        assert rc == 0 and np.array_equal(part[keep], rev[keep]), keep
        assert all((part[k] == SENTINEL).all() for k in RC.OUTS if k != keep), keep
    for reverse in (False, True):
        rc, none = abi.call(reverse, T=0)
        assert rc == 0 and all((v == SENTINEL).all() for v in none.values()), "T == 0 wrote something"


def test_refusals_through_the_raw_abi():
    from safe_exploration_amd._lib import SR_EINVAL, SR_EUNSUPPORTED, last_error
    x = RC.make_inputs(4, "drop", T=3, H=3, wkind="diag")
    abi = _Abi(x)
    plain = _Abi(RC.make_inputs(4, "none", T=3, H=3, wkind="diag"))
    untouched = lambda out: all((v == SENTINEL).all() for v in out.values())
    for reverse, name in ((False, "sr_rollout_cost"), (True, "sr_rollout_cost_vjp")):
        for who, kw, want in ((abi, dict(drop=("in:z",)), SR_EINVAL), (abi, dict(drop=("in:F",)), SR_EINVAL), (abi, dict(drop=("in:mu",)), SR_EINVAL),
                              (abi, dict(T=-1), SR_EINVAL), (abi, dict(H=0), SR_EINVAL), (abi, dict(idx=-2), SR_EINVAL), (abi, dict(idx=4), SR_EINVAL),
                              (abi, dict(loss=2), SR_EINVAL), (abi, dict(loss=-1), SR_EINVAL), (abi, dict(drop=("in:u",)), SR_EINVAL),
                              (plain, dict(keep=1), SR_EINVAL), (abi, dict(n_s=13), SR_EUNSUPPORTED), (abi, dict(n_u=13), SR_EUNSUPPORTED)):
            rc, out = who.call(reverse, **kw)
            assert rc == want and untouched(out), (name, kw, rc)
            assert last_error().startswith(name + ":"), (name, kw, last_error())
    rc, out = abi.call(False, drop=("cost",))
    assert rc == SR_EINVAL and untouched(out) and last_error().startswith("sr_rollout_cost:")
    rc, out = abi.call(True, drop=RC.OUTS)
    assert rc == SR_EINVAL and untouched(out) and last_error().startswith("sr_rollout_cost_vjp:")
    from safe_exploration_amd import utils_casadi as uc
    with pytest.raises(ValueError):
        uc.rollout_cost_batch(x["mu"], x["sigma"], x["z"], np.diag([1.0, 1, 1, 1, -0.5]), idx_angle=2)
    with pytest.raises(ValueError):
        uc.rollout_cost_vjp_batch(x["mu"], x["sigma"], x["z"], x["W"], idx_angle=2, cost_bar=np.ones(4))
    with pytest.raises(NotImplementedError):
        uc.rollout_cost_batch(np.zeros((2, 2, 13)), None, np.zeros(13))


# ---- the chain: the objective's gradient in k_ff, k_fb ------------------------------------------------------------------------------
_GPS = {}


def _gp(n_s):
    if n_s not in _GPS:
        _GPS[n_s] = width_gp(width_problem(900 + n_s, "rbf", n_s + 1, 60, n_s))
    return _GPS[n_s]


def _rollout(route, gp, leaves, r):
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    if route == "moment_matching":
        return up.moment_matching_rollout_diff_batch(leaves["mu_0"], gp, leaves["k_ff"], leaves["k_fb"], r["a"], r["b"])[:2]
    return up.multistep_moments_diff_batch(leaves["mu_0"], gp, leaves["k_ff"], leaves["k_fb"], r["a"], r["b"], dict(taylor=1, mean_equivalent=2)[route])[:2]


@pytest.mark.parametrize("n_s", (2, 4))
@pytest.mark.parametrize("route", ("taylor", "mean_equivalent", "moment_matching"))
def test_the_chain_against_autograd_through_the_torch_port_and_the_three_raw_calls(route, n_s):
    import torch
    from safe_exploration_amd import utils_casadi as uc, uncertainty_propagation_casadi as up
    T, H, n_u = 3, 4, 1
    gp = _gp(n_s)
    r = MR.rollout_inputs(n_s, n_u, T, H, seed=2)
    x = RC.make_inputs(n_s, "drop", T=T, H=H, wkind="diag", ctrl=False, seed=6)
    kw = _kw(x)
    grads = {}
    for which in ("device", "port"):
        leaves = dict(mu_0=_t(r["p"]), k_ff=_t(r["k_ff"]).requires_grad_(True), k_fb=_t(r["k_fb"]).requires_grad_(True))
        mu_all, sigma_all = _rollout(route, gp, leaves, r)
        if which == "device":
            c = uc.rollout_cost_batch(mu_all, sigma_all, differentiable=True, **kw)
            assert torch.equal(c, uc.rollout_cost_batch(mu_all.detach(), sigma_all.detach(), **kw)), "not the bits of the plain call"
            stored = (mu_all.detach(), sigma_all.detach())
        else:
            c = RC.torch_cost(mu_all, sigma_all, x)
        grads[which] = torch.autograd.grad(c.sum(), [leaves["k_ff"], leaves["k_fb"]])
    err = max(MR.rel_err(d.cpu().numpy(), p.cpu().numpy()) for d, p in zip(grads["device"], grads["port"]))
    print("%s n_s=%d: the device cost against the torch port, gradient in k_ff, k_fb: %.3e of the largest element, share of the bar %.3f"
          % (route, n_s, err, err / RC.CHAIN_RTOL))
    # the three raw calls: roll-out (stored above), the cost's reverse pass, the roll-out's reverse pass
    mu_bar, sigma_bar, _ = uc.rollout_cost_vjp_batch(stored[0], stored[1], **kw)
    p, kff, kfb = _t(r["p"]), _t(r["k_ff"]), _t(r["k_fb"])
    if route == "moment_matching":
        raw = up.moment_matching_rollout_vjp_batch(p, gp, kff, kfb, stored[0], stored[1], mu_bar, sigma_bar, None, r["a"], r["b"])
    else:
        raw = up.multistep_moments_vjp_batch(p, gp, kff, kfb, stored[0], stored[1], mu_bar, sigma_bar, None, r["a"], r["b"],
                                             dict(taylor=1, mean_equivalent=2)[route])
    assert torch.equal(raw[2].reshape(kff.shape), grads["device"][0]) and torch.equal(raw[3].reshape(kfb.shape), grads["device"][1]), \
        "the three raw calls and the autograd surface differ"
    assert err <= RC.CHAIN_RTOL, err
