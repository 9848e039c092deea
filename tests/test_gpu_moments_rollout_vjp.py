"""The reverse pass of a whole Taylor / mean-equivalent roll-out on the device (sr_multistep_moments_vjp,
uncertainty_propagation_casadi.multistep_moments_vjp_batch / multistep_moments_diff_batch) against the long-double sweep of
tests/_moments_rollout_grad_ref.py.

The reference is fed the device's OWN linearize_device_batch outputs at the z_i of the device's mu_all, so only the sweep is under
test.  Cases (_moments_rollout_grad_ref.CASES: the roll-outs of tests/test_gpu_reach_rollout_vjp.py in modes 1 and 2, each from a
point and from N(mu_0, sigma_0)): H = 1, 2, 3, 5; T = 1, 65, 257; models (2, 3) rbf at N = 150 and 600, (4, 5) rbf, (2, 3) lin_mat52,
the cart-pole shape behind an input transform (3 x 4, D = 4), a sparse handle, (5, 6) rbf at N = 60 (n_s >= 5: the thread's matrix
lives in LDS, the hand-off arrays in the scratch).  Seeds on all three outputs (mu_all, sigma_all, gp_var_all).

BARS.  Each gradient within PROP_RTOL = 30 x 8.4e-16 = 2.52e-14 of its largest element, every trajectory (no square root and no
eigen-gap here: nothing is left out); 8.4e-16 is the worst disagreement of the long-double and the fp64 sweep on exactly these
cases with a NumPy GP standing in, measured and asserted by tests/test_moments_rollout_vjp_host.py.  sigma0_bar is exactly
symmetric.  End to end, against torch.autograd.grad through multistep_moments_batch(differentiable=True) on the same inputs:
within CHAIN_RTOL = 30 x 5.8e-12 = 1.74e-10, the floor measured on the CPU by the same host test (two fp64 sweeps at two forwards
that agree to rounding -- the chained route differentiates at the states of its own per-step forward).  Every share is printed.

Also: two calls equal; set_chunk(2 H) and set_chunk(H - 1) at T = 5 the bits of the default; chunks of 64 / 1000 / the default at
N = 2000, T = 100, H = 15; a trajectory alone equals its rows in a batch; a NULL seed equals a zero seed; an unsymmetric
sigma_all_bar equals its symmetric part; seeds on one output only and on the last step only; through the C ABI into
sentinel-filled buffers with room in front and behind (nothing outside written, T == 0 a no-op); the autograd surface (forward
bits, backward bits); the refusals; the example.

Observed on MI355X: at most 0.045 of the bar against the long-double sweep (d/dmu_0), typically 0.005 - 0.03; at most 0.005 of the bar
against the chained route (9e-13 of the largest element).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _moments_rollout_grad_ref as MR
from _helpers import width_problem, width_gp

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e+300
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = dict(rbf23_150=("exact", "rbf", 2, 3, 150), rbf23_600=("exact", "rbf", 2, 3, 600), rbf45=("exact", "rbf", 4, 5, 150),
              linmat52_23=("exact", "lin_mat52", 2, 3, 150), cartpole=("exact", "rbf", 4, 4, 150),
              sparse23=("sparse", "rbf", 2, 3, 3000), rbf56=("exact", "rbf", 5, 6, 60))


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


_GPS = {}


def _gp(key):
    if key not in _GPS:
        kind, kt, n_out, D, N = MODELS[key]
        if kind == "sparse":
            import _sparse_ref as S
            from test_gpu_sparse_gp import _sparse_model
            _GPS[key] = _sparse_model(S.make_case(5, kt, n_out, D, 96, N))
        else:
            _GPS[key] = width_gp(width_problem(4000 + N + D, kt, D, N, n_out))
    return _GPS[key]


def _kfb(x):
    return x["k_fb"] if x["k_ff"].shape[1] > 1 else None


def _forward(gp, x, mode, start, tz):
    """mu_all, sigma_all, gp_var_all (NumPy): the one-launch roll-out from a point, the per-step route from N(mu_0, sigma_0)"""
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    if start == "point":
        return up.multistep_moments_batch(x["p"], gp, x["k_ff"], _kfb(x), x["a"], x["b"], mode, tz)
    outs = up.multistep_moments_batch(_t(x["p"]), gp, _t(x["k_ff"]), _t(_kfb(x)), x["a"], x["b"], mode, tz, differentiable=True,
                                      sigma_0=_t(x["q"]))
    return tuple(o.cpu().numpy() for o in outs)


def _vjp(gp, x, ma, sa, w_m, w_s, w_v, mode, start, tz):
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    g = up.multistep_moments_vjp_batch(x["p"], gp, x["k_ff"], _kfb(x), ma, sa, w_m, w_s, w_v, x["a"], x["b"], mode, tz,
                                       x["q"] if start == "gauss" else None)
    return dict(zip(MR.NAMES, g))


def _device_lins(gp, x, ma, tz):
    T, H = x["k_ff"].shape[:2]
    prev = np.concatenate((x["p"][:, None], ma[:, :-1]), axis=1)                   # the mean every step starts from
    z = np.concatenate((prev if tz is None else prev.dot(np.asarray(tz).T), x["k_ff"]), axis=2)
    outs = gp.linearize_device_batch(z.reshape(T * H, -1))
    return tuple(o.cpu().numpy().reshape((T, H) + tuple(o.shape[1:])) for o in outs)


_CASE = {}


def _case(key, T, H, mode, start):
    """inputs, the device's forward and linearisations, the long-double sweep: computed once, shared, left unchanged"""
    k = (key, T, H, mode, start)
    if k not in _CASE:
        n_s, n_u, tz = MR.model_dims(key)
        gp = _gp(key)
        x = MR.rollout_inputs(n_s, n_u, T, H)
        x["w_v"] = MR.seed_v(T, H, n_s)
        ma, sa, va = _forward(gp, x, mode, start, tz)
        lins = _device_lins(gp, x, ma, tz)
        ref = MR.sweep(x, H, mode, lins, ma, sa, x["w_p"], x["w_q"], x["w_v"], start, tz)
        _CASE[k] = (gp, x, tz, ma, sa, lins, ref)
    return _CASE[k]


def _shares(tag, got, ref, rtol=MR.PROP_RTOL):
    worst = {}
    for name in MR.NAMES:
        if name not in ref:                                  # (the chained route has no leaf for it: k_fb at H = 1, sigma_0 from a point)
            continue
        if ref[name] is None:
            assert got[name] is None, name
            continue
        assert got[name].shape == ref[name].shape and np.isfinite(got[name]).all(), name
        worst[name] = MR.rel_err(got[name], ref[name]) / rtol
    print("%s: share of the bar used %s" % (tag, {k: "%.3f" % v for k, v in worst.items()}))
    return worst


def _chained(gp, x, w_m, w_s, w_v, mode, start, tz):
    """torch.autograd.grad through multistep_moments_batch(differentiable=True): H one-step nodes"""
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    leaves = dict(mu_0=_t(x["p"]).requires_grad_(True), k_ff=_t(x["k_ff"]).requires_grad_(True))
    if x["k_ff"].shape[1] > 1:
        leaves["k_fb"] = _t(x["k_fb"]).requires_grad_(True)
    if start == "gauss":
        leaves["sigma_0"] = _t(x["q"]).requires_grad_(True)
    ma, sa, va = up.multistep_moments_batch(leaves["mu_0"], gp, leaves["k_ff"], leaves.get("k_fb"), x["a"], x["b"], mode, tz,
                                            differentiable=True, sigma_0=leaves.get("sigma_0"))
    names = list(leaves)
    grads = torch.autograd.grad((ma * _t(w_m)).sum() + (sa * _t(w_s)).sum() + (va * _t(w_v)).sum(), [leaves[k] for k in names])
    return {k: g.cpu().numpy() for k, g in zip(names, grads)}


@pytest.mark.parametrize("case", MR.CASES, ids=lambda c: "%s-T%d-H%d-mode%d-%s" % c)
def test_rollout_vjp_against_the_long_double_sweep_and_the_chained_route(case):
    key, T, H, mode, start = case
    gp, x, tz, ma, sa, lins, ref = _case(*case)
    got = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], x["w_v"], mode, start, tz)
    worst = _shares("%s T=%d H=%d mode=%d %s" % case, got, ref)
    if start == "gauss":
        assert np.array_equal(got["sigma_0"], got["sigma_0"].transpose(0, 2, 1))
    else:
        assert got["sigma_0"] is None
    chained = _chained(gp, x, x["w_p"], x["w_q"], x["w_v"], mode, start, tz)
    far = _shares("   against the chained autograd route", got, chained, MR.CHAIN_RTOL)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(v <= 1.0 for v in far.values()), far


@pytest.mark.parametrize("start", MR.STARTS)
@pytest.mark.parametrize("mode", MR.MODES)
def test_seed_variants(mode, start):
    """seeds on one output only, on the last step only (the terminal constraint); an unsymmetric sigma_all_bar and its symmetric
    part give the same bits"""
    key, T, H = "cartpole", 65, 3
    gp, x, tz, ma, sa, lins, _ = _case(key, T, H, mode, start)
    last = [np.zeros_like(x[k]) for k in ("w_p", "w_q", "w_v")]
    for l, k in zip(last, ("w_p", "w_q", "w_v")):
        l[:, -1] = x[k][:, -1]
    for tag, w in (("mu only", (x["w_p"], None, None)), ("sigma only", (None, x["w_q"], None)), ("gp_var only", (None, None, x["w_v"])),
                   ("last step", tuple(last))):
        got = _vjp(gp, x, ma, sa, w[0], w[1], w[2], mode, start, tz)
        ref = MR.sweep(x, H, mode, lins, ma, sa, w[0], w[1], w[2], start, tz)
        worst = _shares("seeds %s mode=%d %s" % (tag, mode, start), got, ref)
        assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    full = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], x["w_v"], mode, start, tz)
    sym = _vjp(gp, x, ma, sa, x["w_p"], 0.5 * (x["w_q"] + x["w_q"].transpose(0, 1, 3, 2)), x["w_v"], mode, start, tz)
    for name in MR.NAMES:
        assert (full[name] is None and sym[name] is None) or np.array_equal(full[name], sym[name]), name


@pytest.mark.parametrize("key", ("cartpole", "rbf56"))
def test_a_trajectory_alone_equals_its_rows_in_a_batch(key):
    T, H = 65, 3
    for mode in MR.MODES:
        for start in MR.STARTS:
            gp, x, tz, ma, sa, lins, _ = _case(key, T, H, mode, start)
            whole = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], x["w_v"], mode, start, tz)
            for t in (0, 64):
                xs = {k: (v[t:t + 1] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == T and k not in ("a", "b") else v)
                      for k, v in x.items()}
                alone = _vjp(gp, xs, ma[t:t + 1], sa[t:t + 1], xs["w_p"], xs["w_q"], xs["w_v"], mode, start, tz)
                for name in MR.NAMES:
                    assert (whole[name] is None and alone[name] is None) or np.array_equal(whole[name][t:t + 1], alone[name]), (name, t)


# ---- through the C ABI into sentinel-filled buffers -------------------------------------------------------------------------
GUARD = 64


class _Abi(object):
    """one call of sr_multistep_moments_vjp with every output inside a sentinel-filled buffer, GUARD doubles in front and behind"""

    def __init__(self, gp, x, ma, sa, mode, start, tz=None):
        self.gp, self.x, self.mode, self.start, self.tz = gp, x, mode, start, tz
        self.T, self.H, self.n_u = x["k_ff"].shape
        self.n_s = x["p"].shape[1]
        self.d = {k: _t(v) for k, v in x.items() if isinstance(v, np.ndarray)}
        self.d["ma"], self.d["sa"] = _t(ma), _t(sa)
        T, H, n_s, n_u = self.T, self.H, self.n_s, self.n_u
        self.shapes = dict(mu_0=(T, n_s), sigma_0=(T, n_s, n_s), k_ff=(T, H, n_u), k_fb=(T, H - 1, n_u, n_s))

    def call(self, w_m, w_s, w_v, T=None, H=None, mode=None, drop=(), handle=False):
        """returns (status, dict name -> array); `drop`: outputs, and inputs as "in:<name>", passed as NULL"""
        import torch
        from safe_exploration_amd import _buffers as B
        from safe_exploration_amd._lib import lib
        from safe_exploration_amd.gp_reachability import _input_transform
        d, P = self.d, B.ptr
        bufs = {k: torch.full((int(np.prod(s)) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=_dev())
                for k, s in self.shapes.items()}
        gauss = self.start == "gauss"
        given = lambda k: k not in drop and (gauss or k != "sigma_0") and int(np.prod(self.shapes[k])) > 0
        optr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 8 * GUARD) if given(k) else None
        iptr = lambda k: None if "in:" + k in drop else P(d[k])
        hd = self.gp._handle
        with _input_transform(self.gp, self.tz):
            rc = lib.sr_multistep_moments_vjp(hd.h if handle is False else handle, self.T if T is None else T,
                                              self.H if H is None else H, self.mode if mode is None else mode, iptr("p"),
                                              iptr("q") if gauss else None, iptr("k_ff"), iptr("k_fb") if self.H > 1 else None,
                                              iptr("a"), iptr("b"), iptr("ma"), iptr("sa"), P(w_m), P(w_s), P(w_v), optr("mu_0"),
                                              optr("sigma_0"), optr("k_ff"), optr("k_fb"), B.stream_ptr(hd.device))
        torch.cuda.synchronize()
        out = {}
        for k, s in self.shapes.items():
            flat = bufs[k].cpu().numpy()
            n = int(np.prod(s))
            assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all(), "%s: written outside" % k
            out[k] = flat[GUARD:GUARD + n].reshape(s)
        return rc, out


def _same(u, v):
    return all(np.array_equal(u[k], v[k]) for k in u)


@pytest.mark.parametrize("start", MR.STARTS)
@pytest.mark.parametrize("mode", MR.MODES)
def test_c_abi_bounds_repeats_chunks_and_null_seeds(mode, start):
    import torch
    gp = _gp("rbf23_150")
    T, H = 5, 3
    x = MR.rollout_inputs(2, 1, T, H, seed=3)
    ma, sa, _ = _forward(gp, x, mode, start, None)
    abi = _Abi(gp, x, ma, sa, mode, start)
    w = [_t(x["w_p"]), _t(x["w_q"]), _t(MR.seed_v(T, H, 2, seed=3))]
    rc, first = abi.call(*w)
    assert rc == 0
    for k, v in first.items():
        untouched = start == "point" and k == "sigma_0"
        assert (v == SENTINEL).all() if untouched else (np.isfinite(v).all() and not (v == SENTINEL).any()), k
    py = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], MR.seed_v(T, H, 2, seed=3), mode, start, None)
    assert all(py[k] is None or np.array_equal(py[k], first[k]) for k in MR.NAMES), "the wrapper and the C ABI differ"
    assert _same(first, abi.call(*w)[1]), "two calls differ"
    try:
        for chunk in (2 * H, H - 1):
            gp.set_chunk(chunk)
            assert _same(first, abi.call(*w)[1]), "set_chunk(%d) changed the bits" % chunk
    finally:
        gp.set_chunk(65536)
    for k in range(3):
        null, zero = list(w), list(w)
        null[k], zero[k] = None, torch.zeros_like(w[k])
        assert _same(abi.call(*null)[1], abi.call(*zero)[1]), "a NULL seed is not a zero seed"
    rc, none = abi.call(*w, T=0)
    assert rc == 0 and all((v == SENTINEL).all() for v in none.values()), "T == 0 wrote something"


def test_chunks_at_a_size_where_the_passes_matter():
    """N = 2000, n_out = 2: the GP pass's split counts depend on the width of a pass unless the entry point bounds it.  T = 100,
    H = 15 = 1500 queries: chunks of 64 (4 trajectories a group), 1000 (66) and the default, the same bits."""
    gp = width_gp(width_problem(4242, "rbf", 3, 2000, 2))
    T, H = 100, 15
    x = MR.rollout_inputs(2, 1, T, H, seed=5)
    x["k_ff"] *= 0.25
    w_v = MR.seed_v(T, H, 2, seed=5)
    for mode, start in ((1, "gauss"), (1, "point"), (2, "point")):
        ma, sa, _ = _forward(gp, x, mode, start, None)
        whole = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], w_v, mode, start, None)
        assert all(v is None or np.isfinite(v).all() for v in whole.values())
        try:
            for chunk in (64, 1000):
                gp.set_chunk(chunk)
                parts = _vjp(gp, x, ma, sa, x["w_p"], x["w_q"], w_v, mode, start, None)
                assert all(whole[k] is None or np.array_equal(whole[k], parts[k]) for k in MR.NAMES), "chunk %d" % chunk
        finally:
            gp.set_chunk(65536)


# ---- the autograd surface ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ("rbf23_150", "cartpole"))
def test_the_autograd_surface(key):
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    gp = _gp(key)
    n_s, n_u, tz = MR.model_dims(key)
    T, H = 33, 3
    x = MR.rollout_inputs(n_s, n_u, T, H, seed=9)
    w = [_t(x["w_p"]), _t(x["w_q"]), _t(MR.seed_v(T, H, n_s, seed=9))]
    for mode in MR.MODES:
        for start in MR.STARTS:
            leaves = dict(mu_0=_t(x["p"]).requires_grad_(True), k_ff=_t(x["k_ff"]).requires_grad_(True),
                          k_fb=_t(x["k_fb"]).requires_grad_(True))
            if start == "gauss":
                leaves["sigma_0"] = _t(x["q"]).requires_grad_(True)
            s0 = leaves.get("sigma_0")
            det = {k: v.detach() for k, v in leaves.items()}
            if start == "point":
                plain = up.multistep_moments_batch(det["mu_0"], gp, det["k_ff"], det["k_fb"], x["a"], x["b"], mode, tz)
            else:
                plain = up.multistep_moments_batch(det["mu_0"], gp, det["k_ff"], det["k_fb"], x["a"], x["b"], mode, tz,
                                                   differentiable=True, sigma_0=det["sigma_0"])
            diff = up.multistep_moments_diff_batch(leaves["mu_0"], gp, leaves["k_ff"], leaves["k_fb"], x["a"], x["b"], mode, tz, s0)
            assert all(torch.equal(p, d) for p, d in zip(plain, diff)), "not the bits of the plain call"
            assert all(d.requires_grad for d in diff)
            names = list(leaves)
            loss = sum((d * wk).sum() for d, wk in zip(diff, w))
            grads = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)))
            vjp = up.multistep_moments_vjp_batch(det["mu_0"], gp, det["k_ff"], det["k_fb"], plain[0], plain[1], w[0], w[1], w[2],
                                                 x["a"], x["b"], mode, tz, det.get("sigma_0"))
            assert all(torch.is_tensor(v) or v is None for v in vjp)
            for name, v in zip(MR.NAMES, vjp):
                assert (v is None and name not in grads) or torch.equal(grads[name], v), name
            # a result nobody used arrives as a None seed: sigma_all alone
            only = torch.autograd.grad((diff[1] * w[1]).sum(), leaves["k_ff"], retain_graph=True)[0]
            direct = up.multistep_moments_vjp_batch(det["mu_0"], gp, det["k_ff"], det["k_fb"], plain[0], plain[1], None, w[1], None,
                                                    x["a"], x["b"], mode, tz, det.get("sigma_0"))
            assert torch.equal(only, direct[2])
    with pytest.raises(TypeError):
        up.multistep_moments_diff_batch(x["p"], gp, x["k_ff"], x["k_fb"])


def test_numpy_in_numpy_out_and_h_equal_one():
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    gp = _gp("rbf23_150")
    x = MR.rollout_inputs(2, 1, 3, 1, seed=2)
    ma, sa, _ = _forward(gp, x, 1, "point", None)
    g = up.multistep_moments_vjp_batch(x["p"], gp, x["k_ff"], None, ma, sa, x["w_p"], x["w_q"], None, x["a"], x["b"])
    assert isinstance(g[0], np.ndarray) and g[1] is None and g[2].shape == (3, 1, 1) and g[3].shape == (3, 0, 1, 2)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from safe_exploration_amd import SimpleGPModel, uncertainty_propagation_casadi as up
    from safe_exploration_amd._lib import lib, SR_EINVAL, SR_ESTATE
    gp9 = width_gp(width_problem(77, "rbf", 9, 60, 8))           # n_s = 8, n_u = 1, D = 9
    x9 = MR.rollout_inputs(8, 1, 4, 2, seed=1)
    with pytest.raises(NotImplementedError):
        up.multistep_moments_vjp_batch(x9["p"], gp9, x9["k_ff"], x9["k_fb"], np.zeros((4, 2, 8)), np.zeros((4, 2, 8, 8)), x9["w_p"])
    x = MR.rollout_inputs(2, 1, 4, 3, seed=1)
    with pytest.raises(RuntimeError):                            # untrained: before a device is touched
        up.multistep_moments_vjp_batch(x["p"], SimpleGPModel(2, 2, 1), x["k_ff"], x["k_fb"], np.zeros((4, 3, 2)),
                                       np.zeros((4, 3, 2, 2)), x["w_p"])
    gp = _gp("rbf23_150")
    ma, sa, _ = _forward(gp, x, 1, "gauss", None)
    call = lambda **kw: up.multistep_moments_vjp_batch(
        x["p"], gp, x["k_ff"], kw.get("k_fb", x["k_fb"]), kw.get("ma", ma), sa, kw.get("w_m", x["w_p"]), kw.get("w_s", x["w_q"]),
        None, x["a"], x["b"], kw.get("mode", 1), None, kw.get("s0", x["q"]))
    with pytest.raises(TypeError):
        up.multistep_moments_vjp_batch(x["p"], object(), x["k_ff"], x["k_fb"], ma, sa, x["w_p"])
    for kw in (dict(w_m=None, w_s=None), dict(ma=ma[:, :2]), dict(w_s=x["w_q"][:3]), dict(k_fb=x["k_fb"][:, :1]), dict(k_fb=None),
               dict(mode=3), dict(s0=x["q"][:3])):
        with pytest.raises(ValueError):
            call(**kw)
    # the C ABI: host-side refusals, nothing launched, the outputs untouched
    abi = _Abi(gp, x, ma, sa, 1, "gauss")
    w = [_t(x["w_p"]), _t(x["w_q"]), _t(MR.seed_v(4, 3, 2))]
    untouched = lambda out: all((v == SENTINEL).all() for v in out.values())
    for kw, want in ((dict(drop=("sigma_0",)), SR_EINVAL),       # sigma0 without sigma0_bar
                     (dict(drop=("mu_0",)), SR_EINVAL), (dict(drop=("k_ff",)), SR_EINVAL), (dict(drop=("k_fb",)), SR_EINVAL),
                     (dict(drop=("in:p",)), SR_EINVAL), (dict(drop=("in:k_ff",)), SR_EINVAL), (dict(drop=("in:k_fb",)), SR_EINVAL),
                     (dict(drop=("in:a",)), SR_EINVAL), (dict(drop=("in:b",)), SR_EINVAL), (dict(drop=("in:ma",)), SR_EINVAL),
                     (dict(drop=("in:sa",)), SR_EINVAL),
                     (dict(T=-1), SR_EINVAL), (dict(H=0), SR_EINVAL), (dict(mode=0), SR_EINVAL), (dict(mode=3), SR_EINVAL),
                     (dict(handle=None), SR_EINVAL)):
        rc, out = abi.call(*w, **kw)
        assert rc == want and untouched(out), kw
    rc, out = abi.call(None, None, None)
    assert rc == SR_EINVAL and untouched(out)                    # every seed NULL
    raw = ctypes.c_void_p()
    assert lib.sr_gp_create(ctypes.byref(raw), 0, 16, 3, 2) == 0
    try:
        rc, out = abi.call(*w, handle=raw)
        assert rc == SR_ESTATE and untouched(out)                # not factorized
    finally:
        lib.sr_gp_destroy(raw)
    torch.cuda.synchronize()


# ---- the example ------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_its_two_gradients_agree():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "cautious_shooting_fused.py")], capture_output=True,
                         text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert sum(" route: " in line for line in lines) == 2, res.stdout
    dist = [float(line.split()[-1]) for line in lines if line.startswith("distance")]
    assert len(dist) == 1 and dist[0] <= MR.CHAIN_RTOL, res.stdout
