"""The exploration objective on the device: the GP variances of a reachability roll-out (sr_multistep_reach_var), their seed in
the roll-out's reverse pass (sr_multistep_reach_var_vjp), and the objective with its closed-form gradient (sr_rollout_explore,
sr_rollout_explore_vjp; gp_reachability.exploration_cost_batch / exploration_cost_vjp_batch / safempc_default_cost).

FORWARD VARIANCES.  gp_var_all of the mode-0 variants of tests/_chain_ref.py (from a point, from (q0, k_fb0)) against
_chain_ref.reference at its own bar for `var` (30 x the fp64 floor + 2 x the response to the accepted errors of the posterior), on
the persistent launch and on the per-step launches (gp.last_chain asserted): (2, 1) at Np = 128, (4, 1) at Np = 256, T = 1, 17,
H = 1, 5; N = 600 with a chunk boundary inside the batch and the cart-pole shape behind an input transform (per-step only).  p_all,
q_all are the bits of the call without the flag on the same route.

REVERSE WITH THE VARIANCE SEED.  _explore_ref.ROLL_CASES, each from a point and from q_0, seeds (w_p, w_q, w_v), w_v alone, w_v = None,
against the long-double sweep of _explore_ref.sweep_var fed the device's own linearisations (the method of
tests/test_gpu_reach_rollout_vjp.py), within VAR_RTOL = 30 x 6.1e-16 = 1.83e-14 of each gradient's largest element;
trajectories with an eigen-gap factor g < G_MIN left out of the value bars (at most 2 % of a case, asserted).  Every share of the
bar is printed.  Conditions: NULL gpvar_all_bar = the bits of sr_multistep_reach_vjp, a zero array = equal numbers, two calls
equal, any set_chunk the same bits (also where the passes matter), a trajectory alone = inside a batch of 257, a bound violation
makes NaN exactly what flows through it also under a w_v-only seed, guard bands, refusals.

OBJECTIVE.  _explore_ref.OBJ_CASES against the long-double reference within OBJ_RTOL = 30 x 4.2e-16 = 1.26e-14 of each array's
largest element; rows of p_bar / mu_bar outside 1 .. n_dev - 1 exactly zero; cost_bar None = ones; with and without cost_steps; a
zero and a negative radicand; the autograd surface; safempc_default_cost; every refusal.

END TO END.  The gradient in p_0, k_ff, k_fb (of both roll-outs) of the n_perf > 1 default cost, N = 60, n_s = 2 and 4, H_safe = 3,
H_perf = 4, T = 3: the objective's raw reverse call feeding the two roll-out nodes against torch autograd through the cost written
in torch on the same nodes, within E2E_RTOL = 30 x 2.9e-16 = 8.7e-15 of the largest element; 2.88e-16 is the disagreement of the two
routes measured in CPU torch at one stored forward by tests/test_explore_host.py.

Observed on MI355X: the reverse pass with the variance seed at most 0.13 of its bar (d/dk_ff, (4, 5) rbf, T = 1, H = 5, from a point,
all three seeds), typically 0.01 - 0.03; the objective at most 0.05 (the cost over 65 steps); end to end 0.035 (n_s = 4); the forward
variances at most 1e-5 of theirs.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _chain_ref as C
import _explore_ref as E
import _reach_rollout_grad_ref as RR
from _helpers import width_problem, width_gp

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e+300
GUARD = 64
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


def _eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- forward variances ------------------------------------------------------------------------------------------------------------
def _fit(m):
    from safe_exploration_amd import SimpleGPModel
    gp = SimpleGPModel(m.n_s, m.nx, m.n_u, kern_types=["rbf"] * m.n_s, hyp=m.hyp)
    gp.train(m.Z, m.Y, opt_hyp=False)
    return gp


def _reach(gp, m, x, variant, flag):
    from safe_exploration_amd import gp_reachability as reach
    q0, kfb0 = (x["q"], x["k_fb0"]) if variant == "q0" else (None, None)
    return reach.multistep_reachability_batch(x["p"], gp, x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], q0, x["c"], x["a"], x["b"],
                                              kfb0, t_z_gp=m.tz, return_gp_var=flag)


def _check_var(tag, gp, m, x, T, H, variant, chain, rows):
    gp.set_chain(chain)
    try:
        p, q, v = _reach(gp, m, x, variant, True)
        assert bool(gp.last_chain) == chain, "%s: %s route expected" % (tag, "persistent" if chain else "per-step")
        p0, q0 = _reach(gp, m, x, variant, False)
        assert bool(gp.last_chain) == chain
    finally:
        gp.set_chain(True)
    assert np.array_equal(p, p0) and np.array_equal(q, q0), "%s: the flag changed p_all / q_all" % tag
    ref = C.reference(m, x, H, rows, variant, key=(id(m), T, H, tuple(rows)))
    assert v.shape == (T, H, m.n_s) and np.isfinite(v).all() and (v >= 1e-15).all()
    err = np.abs(v[rows] - ref["var"]).max(axis=(0, 2))
    print("%s gp_var: worst share of the bar %.1e (bar %.1e .. %.1e)" % (tag, float((err / ref["bar_var"]).max()), ref["bar_var"].min(),
                                                                        ref["bar_var"].max()))
    assert np.all(err <= ref["bar_var"]), (tag, err, ref["bar_var"])


@pytest.mark.parametrize("n_s,n_u,N", ((2, 1, 100), (4, 1, 200)), ids=("Np128", "Np256"))
def test_forward_variances_on_both_routes(n_s, n_u, N):
    import torch
    m = C.model(n_s, n_u, N)
    gp = _fit(m)
    assert gp._handle.Np_now() == m.Np
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for T in (1, 17):
        for H in (1, 5):
            x = C.inputs(n_s, n_u, T, H)
            persistent = C.launches(T, m.Np, n_s, n_u, H, cus) <= C.max_launches(T, H)
            for variant in ("point", "q0"):
                for chain in ((True, False) if persistent else (False,)):
                    _check_var("ns%d N%d T%d H%d %s %s" % (n_s, N, T, H, variant, "persistent" if chain else "per-step"), gp, m, x, T, H,
                               variant, chain, list(range(T)))
            assert persistent, "the persistent launch was expected to apply at T=%d H=%d" % (T, H)


@pytest.mark.parametrize("cid,n_s,n_u,N,tz,T,H,chunk", [c[:8] for c in C.per_step_cases()[1:]], ids=[c[0] for c in C.per_step_cases()[1:]])
def test_forward_variances_where_only_the_per_step_route_applies(cid, n_s, n_u, N, tz, T, H, chunk):
    m = C.model(n_s, n_u, N, tz=tz)
    gp = _fit(m)
    x = C.inputs(n_s, n_u, T, H)
    rows = list(range(min(T, 24))) + list(range(max(T - 4, 24), T))
    try:
        if chunk:
            gp.set_chunk(chunk)
        for variant in ("point", "q0"):
            _check_var("%s %s" % (cid, variant), gp, m, x, T, H, variant, False, rows)
    finally:
        gp.set_chunk(65536)


# ---- reverse with the variance seed -----------------------------------------------------------------------------------------------
def _tv():
    import test_gpu_reach_rollout_vjp as TV
    return TV


def _vjp(gp, x, pa, qa, w_p, w_q, w_v, start_q, tz):
    from safe_exploration_amd import gp_reachability as reach
    g = reach.multistep_reachability_vjp_batch(x["p"], gp, x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], pa, qa, w_p, w_q,
                                               x["q"] if start_q else None, x["c"], x["a"], x["b"], x["k_fb0"] if start_q else None, tz,
                                               gpvar_all_bar=w_v)
    return dict(zip(RR.NAMES, g))


def _shares(tag, got, ref, keep):
    worst = {}
    for name in RR.NAMES:
        if ref[name] is None:
            assert got[name] is None, name
            continue
        assert got[name].shape == ref[name].shape and np.isfinite(got[name]).all(), name
        worst[name] = RR.rel_err(got[name], ref[name], keep) / E.VAR_RTOL
    print("%s: share of the bar used %s" % (tag, {k: "%.3f" % v for k, v in worst.items()}))
    return worst


@pytest.mark.parametrize("start_q", (False, True), ids=("from_a_point", "from_q0"))
@pytest.mark.parametrize("case", E.ROLL_CASES, ids=lambda c: "%s-T%d-H%d" % c)
def test_rollout_vjp_with_the_variance_seed_against_the_long_double_sweep(case, start_q):
    key, T, H = case
    gp, x, tz, pa, qa, lins, _ = _tv()._case(key, T, H, start_q)
    for which in E.SEEDS:
        w_p, w_q, w_v = E.seeds(x, which)
        ref = E.sweep_var(x, H, lins, pa, qa, w_p, w_q, w_v, start_q, tz)
        assert not ref["bad"].any()
        keep = ref["g"] >= RR.G_MIN
        assert (~keep).sum() <= 0.02 * T, int((~keep).sum())
        got = _vjp(gp, x, pa, qa, w_p, w_q, w_v, start_q, tz)
        worst = _shares("%s T=%d H=%d start_q=%s seeds=%s" % (key, T, H, start_q, which), got, ref, keep)
        if start_q:
            assert np.array_equal(got["q_0"], got["q_0"].transpose(0, 2, 1))
        assert all(v <= 1.0 for v in worst.values()), (which, worst)


class _Abi(object):
    """one call of sr_multistep_reach_var_vjp (var=False: sr_multistep_reach_vjp) with every output inside a sentinel-filled buffer,
    GUARD doubles in front and behind"""

    def __init__(self, gp, x, pa, qa, start_q, tz=None):
        self.gp, self.x, self.start_q, self.tz = gp, x, start_q, tz
        self.T, self.H, self.n_u = x["k_ff"].shape
        self.n_s = x["p"].shape[1]
        self.d = {k: _t(v) for k, v in x.items() if isinstance(v, np.ndarray)}
        self.d["pa"], self.d["qa"] = _t(pa), _t(qa)
        T, H, n_s, n_u = self.T, self.H, self.n_s, self.n_u
        self.shapes = dict(p_0=(T, n_s), q_0=(T, n_s, n_s), k_fb_init=(T, n_u, n_s), k_ff=(T, H, n_u), k_fb=(T, H - 1, n_u, n_s))

    def call(self, w_p, w_q, w_v, var=True, T=None, drop=(), kfb0=True):
        import torch
        from safe_exploration_amd import _buffers as B
        from safe_exploration_amd._lib import lib
        from safe_exploration_amd.gp_reachability import _input_transform
        d, P = self.d, B.ptr
        bufs = {k: torch.full((int(np.prod(s)) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=_dev()) for k, s in self.shapes.items()}
        given = lambda k: k not in drop and (self.start_q or k not in ("q_0", "k_fb_init")) and int(np.prod(self.shapes[k])) > 0
        optr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 8 * GUARD) if given(k) else None
        sq = self.start_q
        hd = self.gp._handle
        head = (hd.h, self.T if T is None else T, self.H, P(d["p"]), P(d["q"]) if sq else None, P(d["k_fb0"]) if (sq and kfb0) else None,
                P(d["k_ff"]), P(d["k_fb"]) if self.H > 1 else None, P(d["a"]), P(d["b"]), P(d["l_mu"]), P(d["l_sigma"]), float(self.x["c"]),
                P(d["pa"]), P(d["qa"]), P(w_p), P(w_q))
        tail = (optr("p_0"), optr("q_0"), optr("k_fb_init"), optr("k_ff"), optr("k_fb"), B.stream_ptr(hd.device))
        with _input_transform(self.gp, self.tz):
            rc = lib.sr_multistep_reach_var_vjp(*head, P(w_v), *tail) if var else lib.sr_multistep_reach_vjp(*head, *tail)
        out = {}
        for k, s in self.shapes.items():
            flat = bufs[k].cpu().numpy()
            n = int(np.prod(s))
            assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all(), "%s: written outside" % k
            out[k] = flat[GUARD:GUARD + n].reshape(s)
        return rc, out


def _same(u, v):
    return all(_eq(u[k], v[k]) for k in u)


@pytest.mark.parametrize("start_q", (False, True), ids=("from_a_point", "from_q0"))
def test_c_abi_null_and_zero_seeds_repeats_chunks_and_guard_bands(start_q):
    import torch
    TV = _tv()
    gp = TV._gp("rbf23_150")
    T, H = 5, 3
    x = RR.rollout_inputs(2, 1, T, H, seed=3)
    pa, qa = TV._forward(gp, x, start_q, None)
    abi = _Abi(gp, x, pa, qa, start_q)
    w_p, w_q, w_v = _t(x["w_p"]), _t(x["w_q"]), _t(E.variance_seed(x))
    rc, first = abi.call(w_p, w_q, w_v)
    assert rc == 0
    for k, v in first.items():
        untouched = not start_q and k in ("q_0", "k_fb_init")
        assert (v == SENTINEL).all() if untouched else (np.isfinite(v).all() and not (v == SENTINEL).any()), k
    py = _vjp(gp, x, pa, qa, x["w_p"], x["w_q"], E.variance_seed(x), start_q, None)
    assert all(py[k] is None or np.array_equal(py[k], first[k]) for k in RR.NAMES), "the wrapper and the C ABI differ"
    assert _same(first, abi.call(w_p, w_q, w_v)[1]), "two calls differ"
    try:
        for chunk in (2 * H, H - 1):
            gp.set_chunk(chunk)
            assert _same(first, abi.call(w_p, w_q, w_v)[1]), "set_chunk(%d) changed the bits" % chunk
    finally:
        gp.set_chunk(65536)
    # NULL gpvar_all_bar: the bits of sr_multistep_reach_vjp; a zero array: equal numbers; the seed matters
    rc, null = abi.call(w_p, w_q, None)
    rc0, old = abi.call(w_p, w_q, None, var=False)
    assert rc == 0 and rc0 == 0 and _same(null, old), "NULL gpvar_all_bar is not sr_multistep_reach_vjp"
    zero = abi.call(w_p, w_q, torch.zeros_like(w_v))[1]
    assert all(np.array_equal(zero[k], old[k]) for k in zero), "a zero seed on the variances changed the numbers"
    assert not np.array_equal(first["k_ff"], old["k_ff"])
    # the other seeds NULL: zero seeds
    for null_s, zero_s in (((None, w_q, w_v), (torch.zeros_like(w_p), w_q, w_v)), ((w_p, None, w_v), (w_p, torch.zeros_like(w_q), w_v)),
                           ((None, None, w_v), (torch.zeros_like(w_p), torch.zeros_like(w_q), w_v))):
        a, b = abi.call(*null_s)[1], abi.call(*zero_s)[1]
        assert all(np.array_equal(a[k], b[k]) for k in a), "a NULL seed is not a zero seed"
    rc, none = abi.call(w_p, w_q, w_v, T=0)
    assert rc == 0 and all((v == SENTINEL).all() for v in none.values()), "T == 0 wrote something"


def test_chunks_at_a_size_where_the_passes_matter():
    """N = 2000, n_out = 2, T = 100, H = 15 (the size tests/test_gpu_reach_rollout_vjp.py picks): chunks of 64, 1000 and the default"""
    TV = _tv()
    gp = width_gp(width_problem(4242, "rbf", 3, 2000, 2))
    T, H = 100, 15
    x = RR.rollout_inputs(2, 1, T, H, seed=5)
    x["k_ff"] *= 0.25
    w_v = E.variance_seed(x)
    pa, qa = TV._forward(gp, x, True, None)
    whole = _vjp(gp, x, pa, qa, x["w_p"], x["w_q"], w_v, True, None)
    assert all(np.isfinite(v).all() for v in whole.values())
    try:
        for chunk in (64, 1000):
            gp.set_chunk(chunk)
            parts = _vjp(gp, x, pa, qa, x["w_p"], x["w_q"], w_v, True, None)
            assert all(np.array_equal(whole[k], parts[k]) for k in RR.NAMES), "chunk %d" % chunk
    finally:
        gp.set_chunk(65536)


def test_a_trajectory_alone_equals_itself_inside_a_batch_of_257():
    gp, x, tz, pa, qa, lins, _ = _tv()._case("rbf23_150", 257, 3, True)
    w_v = E.variance_seed(x)
    whole = _vjp(gp, x, pa, qa, x["w_p"], x["w_q"], w_v, True, tz)
    for t in (0, 100, 256):
        one = {k: (v[t:t + 1] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == 257 else v) for k, v in x.items()}
        alone = _vjp(gp, one, pa[t:t + 1], qa[t:t + 1], one["w_p"], one["w_q"], w_v[t:t + 1], True, tz)
        for k in RR.NAMES:
            assert np.array_equal(alone[k][0], whole[k][t]), (k, t)


@pytest.mark.parametrize("seeds", ("all", "w_v"))
def test_a_bound_violation_reaches_what_flows_through_it_and_nothing_else(seeds):
    TV = _tv()
    gp = TV._gp("rbf23_150")
    T, H, bad_t = 9, 3, 4
    x = RR.rollout_inputs(2, 1, T, H, seed=7)
    pa, qa = TV._forward(gp, x, True, None)
    w_p, w_q, w_v = E.seeds(x, seeds)
    clean = _vjp(gp, x, pa, qa, w_p, w_q, w_v, True, None)
    assert all(np.isfinite(v).all() for v in clean.values())
    others = np.arange(T) != bad_t
    # step 1 of 3 reads q_all[t][0] = 0: r^2 = 0, l_mu r^2 is not > 0
    qa_bad = qa.copy()
    qa_bad[bad_t, 0] = 0.0
    got = _vjp(gp, x, pa, qa_bad, w_p, w_q, w_v, True, None)
    for k in ("p_0", "q_0", "k_fb_init"):
        assert np.isnan(got[k][bad_t]).all(), k
    assert np.isnan(got["k_ff"][bad_t, :2]).all() and np.isnan(got["k_fb"][bad_t, :1]).all()
    assert np.array_equal(got["k_ff"][bad_t, 2:], clean["k_ff"][bad_t, 2:]) and np.array_equal(got["k_fb"][bad_t, 1:], clean["k_fb"][bad_t, 1:])
    # step 0 with q_0[t] = 0 (the later steps read the q_all they are given)
    x_bad = dict(x, q=x["q"].copy())
    x_bad["q"][bad_t] = 0.0
    got0 = _vjp(gp, x_bad, pa, qa, w_p, w_q, w_v, True, None)
    for k in ("p_0", "q_0", "k_fb_init"):
        assert np.isnan(got0[k][bad_t]).all(), k
    assert np.isnan(got0["k_ff"][bad_t, :1]).all()
    assert np.array_equal(got0["k_ff"][bad_t, 1:], clean["k_ff"][bad_t, 1:]) and np.array_equal(got0["k_fb"][bad_t], clean["k_fb"][bad_t])
    for res in (got, got0):
        for k in RR.NAMES:
            assert np.array_equal(res[k][others], clean[k][others]), k


def test_the_autograd_surface_with_three_outputs():
    import torch
    from safe_exploration_amd import gp_reachability as reach
    TV = _tv()
    for key in ("rbf23_150", "cartpole"):
        gp = TV._gp(key)
        n_s, n_u, tz = RR.model_dims(key)
        T, H = 33, 3
        x = RR.rollout_inputs(n_s, n_u, T, H, seed=9)
        w_p, w_q, w_v = _t(x["w_p"]), _t(x["w_q"]), _t(E.variance_seed(x))
        for start_q in (True, False):
            leaves = dict(p_0=_t(x["p"]).requires_grad_(True), k_ff=_t(x["k_ff"]).requires_grad_(True), k_fb=_t(x["k_fb"]).requires_grad_(True))
            if start_q:
                leaves.update(q_0=_t(x["q"]).requires_grad_(True), k_fb_init=_t(x["k_fb0"]).requires_grad_(True))
            kw = dict(q_0=leaves.get("q_0"), c_safety=x["c"], a=x["a"], b=x["b"], k_fb_init=leaves.get("k_fb_init"), t_z_gp=tz)
            kw0 = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in kw.items()}
            det = lambda k: leaves[k].detach()
            plain = reach.multistep_reachability_batch(det("p_0"), gp, det("k_fb"), det("k_ff"), x["l_mu"], x["l_sigma"], return_gp_var=True, **kw0)
            two = reach.multistep_reachability_batch(det("p_0"), gp, det("k_fb"), det("k_ff"), x["l_mu"], x["l_sigma"], **kw0)
            assert len(plain) == 3 and torch.equal(plain[0], two[0]) and torch.equal(plain[1], two[1])
            diff = reach.multistep_reachability_diff_batch(leaves["p_0"], gp, leaves["k_fb"], leaves["k_ff"], x["l_mu"], x["l_sigma"],
                                                           return_gp_var=True, **kw)
            assert len(diff) == 3 and all(torch.equal(a, b) for a, b in zip(plain, diff)) and diff[2].requires_grad
            names = list(leaves)
            for seeds in ((w_p, w_q, w_v), (None, None, w_v), (w_p, None, None)):
                loss = sum((o * w).sum() for o, w in zip(diff, seeds) if w is not None)
                grads = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names], retain_graph=True)))
                vjp = reach.multistep_reachability_vjp_batch(det("p_0"), gp, det("k_fb"), det("k_ff"), x["l_mu"], x["l_sigma"], plain[0],
                                                             plain[1], seeds[0], seeds[1], kw0["q_0"], x["c"], x["a"], x["b"],
                                                             kw0["k_fb_init"], tz, gpvar_all_bar=seeds[2])
                for name, v in zip(RR.NAMES, vjp):
                    assert (v is None and name not in grads) or torch.equal(grads[name], v), name
    with pytest.raises(NotImplementedError):
        reach.multistep_reachability_batch(_t(x["p"]), gp, _t(x["k_fb"]), _t(x["k_ff"]), x["l_mu"], x["l_sigma"], differentiable=True,
                                           return_gp_var=True, t_z_gp=tz)
    # numpy in, numpy out
    out = reach.multistep_reachability_batch(x["p"], gp, x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], None, x["c"], x["a"], x["b"],
                                             t_z_gp=tz, return_gp_var=True)
    assert len(out) == 3 and all(isinstance(o, np.ndarray) for o in out) and np.array_equal(out[2], plain[2].cpu().numpy())


def test_refusals_of_the_roll_out_calls():
    from safe_exploration_amd import gp_reachability as reach
    from safe_exploration_amd._lib import SR_EINVAL
    TV = _tv()
    gp9 = width_gp(width_problem(77, "rbf", 9, 60, 8))           # n_s = 8, n_u = 1, D = 9
    x9 = RR.rollout_inputs(8, 1, 4, 2, seed=1)
    with pytest.raises(NotImplementedError):
        reach.multistep_reachability_vjp_batch(x9["p"], gp9, x9["k_fb"], x9["k_ff"], x9["l_mu"], x9["l_sigma"], np.zeros((4, 2, 8)),
                                               np.zeros((4, 2, 8, 8)), None, None, None, x9["c"], gpvar_all_bar=np.ones((4, 2, 8)))
    gp = TV._gp("rbf23_150")
    x = RR.rollout_inputs(2, 1, 4, 3, seed=1)
    pa, qa = TV._forward(gp, x, True, None)
    w_v = E.variance_seed(x)
    with pytest.raises(ValueError):
        _vjp(gp, x, pa, qa, None, None, None, True, None)
    with pytest.raises(ValueError):
        _vjp(gp, x, pa, qa, None, None, w_v[:, :2], True, None)
    with pytest.raises(ValueError):
        _vjp(gp, dict(x, k_fb0=None), pa, qa, None, None, w_v, True, None)
    abi = _Abi(gp, x, pa, qa, True)
    untouched = lambda out: all((v == SENTINEL).all() for v in out.values())
    rc, out = abi.call(None, None, None)
    assert rc == SR_EINVAL and untouched(out)                                                       # every seed NULL
    rc, out = abi.call(None, None, _t(w_v), kfb0=False)
    assert rc == SR_EINVAL and untouched(out)                                                       # q0 without k_fb0
    rc, out = abi.call(None, None, _t(w_v), drop=("p_0",))
    assert rc == SR_EINVAL and untouched(out)
    rc, out = abi.call(None, None, _t(w_v), T=-1)
    assert rc == SR_EINVAL and untouched(out)


# ---- the objective ------------------------------------------------------------------------------------------------------------------
def _cost_args(x):
    return dict(kind=x["kind"], eps=x["eps"], p_all=x["p"], mu_perf=x["mu"], wx_cost=x["wx"], n_dev=(x["n_dev"] if x["p"] is not None else None))


@pytest.mark.parametrize("case", E.OBJ_CASES, ids=E.case_id)
def test_the_objective_against_the_long_double_reference(case):
    from safe_exploration_amd import gp_reachability as reach
    x = E.objective_inputs(case)
    kw = _cost_args(x)
    cost, steps = reach.exploration_cost_batch(x["v"], return_steps=True, **kw)
    assert np.array_equal(cost, reach.exploration_cost_batch(x["v"], **kw)), "cost_steps changed the bits of cost"
    assert np.array_equal(cost, reach.exploration_cost_batch(x["v"], **kw)), "two calls differ"
    grads = reach.exploration_cost_vjp_batch(x["v"], cost_bar=x["cost_bar"], **kw)
    ref = E.objective(x) + E.objective_grad(x, x["cost_bar"])
    shares = {}
    for name, got, want in zip(("cost", "steps", "gpvar_bar", "p_bar", "mu_bar"), (cost, steps) + tuple(grads), ref):
        if want is None:
            assert got is None, name
            continue
        assert got.shape == want.shape and np.isfinite(got).all(), name
        shares[name] = RR.rel_err(got, want.astype(np.float64)) / E.OBJ_RTOL
    print("%s: share of the bar used %s" % (E.case_id(case), {k: "%.3f" % v for k, v in shares.items()}))
    assert all(v <= 1.0 for v in shares.values()), shares
    if x["p"] is not None:
        n_dev = x["n_dev"]
        for g in grads[1:]:
            assert not g[:, 0].any() and not g[:, n_dev:].any() and g[:, 1:n_dev].any(), "rows outside 1 .. n_dev - 1 must be exactly zero"
        assert np.array_equal(grads[1][:, 1:n_dev], -grads[2][:, 1:n_dev])
    # the order of the sum over the steps is the stated one: the information terms added one after the other
    assert np.array_equal(reach.exploration_cost_batch(x["v"], x["kind"], x["eps"]), steps.cumsum(axis=1)[:, -1])
    # cost_bar None = ones, to the bit; two calls equal
    ones = reach.exploration_cost_vjp_batch(x["v"], cost_bar=np.ones(x["v"].shape[0]), **kw)
    none = reach.exploration_cost_vjp_batch(x["v"], **kw)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(ones, none))
    again = reach.exploration_cost_vjp_batch(x["v"], cost_bar=x["cost_bar"], **kw)
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(grads, again))
    # a trajectory alone: the bits it has inside the batch
    t = x["v"].shape[0] // 2
    one = reach.exploration_cost_batch(x["v"][t:t + 1], **dict(kw, p_all=None if x["p"] is None else x["p"][t:t + 1],
                                                             mu_perf=None if x["mu"] is None else x["mu"][t:t + 1]))
    assert one[0] == cost[t]


def test_zero_and_negative_radicands():
    from safe_exploration_amd import gp_reachability as reach
    x = E.objective_inputs((4, 15, 65, "sqrt", 0.0, (15, 16, None)))
    kw = _cost_args(x)
    clean = reach.exploration_cost_batch(x["v"], return_steps=True, **kw), reach.exploration_cost_vjp_batch(x["v"], cost_bar=x["cost_bar"], **kw)
    v = x["v"].copy()
    v[3, 7] = 0.0                          # a zero radicand: an exact zero, everything finite
    v[40, 2] = [-1.0, 0.5, 0.25, 0.125]    # a negative one (-0.125)
    cost, steps = reach.exploration_cost_batch(v, return_steps=True, **kw)
    gv, pb, mb = reach.exploration_cost_vjp_batch(v, cost_bar=x["cost_bar"], **kw)
    assert steps[3, 7] == 0.0 and np.isfinite(cost[3]) and not gv[3, 7].any() and np.isfinite(gv[3]).all()
    assert np.isnan(cost[40]) and np.isnan(steps[40, 2]) and np.isnan(gv[40, 2]).all()
    nan_s, nan_g = np.zeros_like(steps, dtype=bool), np.zeros_like(gv, dtype=bool)
    nan_s[40, 2], nan_g[40, 2] = True, True
    assert np.array_equal(np.isnan(steps), nan_s) and np.array_equal(np.isnan(gv), nan_g) and np.isnan(cost).sum() == 1
    assert np.array_equal(pb, clean[1][1]) and np.array_equal(mb, clean[1][2])
    keep = np.ones(65, dtype=bool)
    keep[[3, 40]] = False
    assert np.array_equal(cost[keep], clean[0][0][keep]) and np.array_equal(gv[keep], clean[1][0][keep])
    # with eps > 0 the zero row is an ordinary one
    gv_eps = reach.exploration_cost_vjp_batch(v, **dict(kw, eps=1e-6))[0]
    assert np.allclose(gv_eps[3, 7], -1.0 / (2 * np.sqrt(1e-6)), rtol=1e-14, atol=0)


def test_the_autograd_surface_of_the_objective_equals_the_raw_calls():
    import torch
    from safe_exploration_amd import gp_reachability as reach
    for case in (E.OBJ_CASES[1], E.OBJ_CASES[5], E.OBJ_CASES[4]):
        x = E.objective_inputs(case)
        kw = {k: (_t(v) if isinstance(v, np.ndarray) and k != "wx_cost" else v) for k, v in _cost_args(x).items()}
        v = _t(x["v"]).requires_grad_(True)
        leaves = [v] + [kw[k].requires_grad_(True) for k in ("p_all", "mu_perf") if kw[k] is not None]
        cost, steps = reach.exploration_cost_batch(v, return_steps=True, differentiable=True, **kw)
        kw0 = {k: (t.detach() if torch.is_tensor(t) else t) for k, t in kw.items()}
        raw = reach.exploration_cost_batch(v.detach(), return_steps=True, **kw0)
        assert torch.equal(cost, raw[0]) and torch.equal(steps, raw[1]) and cost.requires_grad and not steps.requires_grad
        cb = _t(x["cost_bar"])
        grads = torch.autograd.grad((cost * cb).sum(), leaves)
        want = [g for g in reach.exploration_cost_vjp_batch(v.detach(), cost_bar=cb, **kw0) if g is not None]
        assert len(grads) == len(want) and all(torch.equal(a, b) for a, b in zip(grads, want))
        assert torch.is_tensor(reach.exploration_cost_batch(v.detach(), **kw0))
    with pytest.raises(TypeError):
        reach.exploration_cost_batch(x["v"], differentiable=True)


def test_safempc_default_cost_agrees_with_the_device():
    from safe_exploration_amd import gp_reachability as reach
    rng = np.random.default_rng(11)
    T, n_s, n_safe, n_perf, eps = 5, 4, 3, 5, 1e-6
    p_all, sig = rng.standard_normal((T, n_safe, n_s)), rng.uniform(1e-4, 1e-2, (T, n_safe, n_s))
    mu, sigp, wx = rng.standard_normal((T, n_perf, n_s)), rng.uniform(1e-4, 1e-2, (T, n_perf, n_s)), rng.standard_normal((n_s, n_s))
    # n_perf <= 1: the information of the safe trajectory; the reference adds eps_noise per element
    dev = reach.exploration_cost_batch(sig, "sqrt", n_s * eps)
    host = np.array([reach.safempc_default_cost(p_all[t], sig[t], eps_noise=eps) for t in range(T)])
    assert RR.rel_err(dev, host) <= E.OBJ_RTOL
    # n_perf > 1: deviation over 1 .. min(n_perf, n_safe) - 1, information of the performance trajectory
    dev = reach.exploration_cost_batch(sigp, "sqrt", n_s * eps, p_all, mu, wx)
    host = np.array([reach.safempc_default_cost(p_all[t], sig[t], mu[t], sigp[t], wx, n_safe, n_perf, eps) for t in range(T)])
    assert RR.rel_err(dev, host) <= E.OBJ_RTOL
    # StaticSafeMPCExploration: -sum1(sum2(sigma))
    assert RR.rel_err(reach.exploration_cost_batch(sig, "sum"), -sig.sum(axis=(1, 2))) <= E.OBJ_RTOL


def test_refusals_of_the_objective():
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, last_error, SR_EINVAL, SR_EUNSUPPORTED
    T, n_s, H_v, H_p, H_m = 3, 2, 4, 5, 6
    P = B.ptr
    d = dict(v=_t(np.ones((T, H_v, n_s))), p=_t(np.zeros((T, H_p, n_s))), mu=_t(np.ones((T, H_m, n_s))), W=_t(np.eye(n_s)), cb=_t(np.ones(T)))
    outs = dict(cost=(T,), steps=(T, H_v), gv=(T, H_v, n_s), pb=(T, H_p, n_s), mb=(T, H_m, n_s))
    o = {k: torch.full(s, SENTINEL, dtype=torch.float64, device=_dev()) for k, s in outs.items()}
    s = B.stream_ptr(_dev())

    def fwd(**kw):
        a = dict(T=T, kind=1, n_s=n_s, H_v=H_v, v=P(d["v"]), eps=0.0, n_dev=2, H_p=H_p, p=P(d["p"]), H_m=H_m, mu=P(d["mu"]), W=P(d["W"]),
                 cost=P(o["cost"]), steps=P(o["steps"]))
        a.update(kw)
        return lib.sr_rollout_explore(0, a["T"], a["kind"], a["n_s"], a["H_v"], a["v"], a["eps"], a["n_dev"], a["H_p"], a["p"], a["H_m"],
                                      a["mu"], a["W"], a["cost"], a["steps"], s)

    def rev(**kw):
        a = dict(T=T, kind=1, n_s=n_s, H_v=H_v, v=P(d["v"]), eps=0.0, n_dev=2, H_p=H_p, p=P(d["p"]), H_m=H_m, mu=P(d["mu"]), W=P(d["W"]),
                 cb=P(d["cb"]), gv=P(o["gv"]), pb=P(o["pb"]), mb=P(o["mb"]))
        a.update(kw)
        return lib.sr_rollout_explore_vjp(0, a["T"], a["kind"], a["n_s"], a["H_v"], a["v"], a["eps"], a["n_dev"], a["H_p"], a["p"], a["H_m"],
                                          a["mu"], a["W"], a["cb"], a["gv"], a["pb"], a["mb"], s)

    bad = (dict(v=None), dict(kind=2), dict(kind=-1), dict(T=-1), dict(H_v=0), dict(n_s=0), dict(n_dev=-1), dict(n_dev=1), dict(n_dev=6),
           dict(n_dev=2, H_p=1), dict(p=None), dict(mu=None), dict(W=None), dict(eps=-1e-9), dict(eps=float("nan")))
    for call, name in ((fwd, "sr_rollout_explore:"), (rev, "sr_rollout_explore_vjp:")):
        for kw in bad:
            assert call(**kw) == SR_EINVAL and last_error().startswith(name), (name, kw)
        assert call(n_s=13) == SR_EUNSUPPORTED
        assert call(T=0) == 0
    assert fwd(cost=None) == SR_EINVAL
    assert rev(gv=None, pb=None, mb=None) == SR_EINVAL
    assert rev(n_dev=0, p=None) == SR_EINVAL and rev(n_dev=0, mu=None) == SR_EINVAL       # p_bar without p, mu_bar without mu
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == SENTINEL).all() for t in o.values()), "a refused call wrote something"
    # what is allowed: no deviation term without p, mu, W; any single output
    assert fwd(n_dev=0, p=None, mu=None, W=None, steps=None) == 0
    assert rev(n_dev=0, p=None, mu=None, W=None, pb=None, mb=None, cb=None) == 0
    assert rev(gv=None, mb=None) == 0 and rev(gv=None, pb=None) == 0
    torch.cuda.synchronize()
    assert (o["steps"].cpu().numpy() == SENTINEL).all() and np.allclose(o["cost"].cpu().numpy(), -H_v * np.sqrt(2.0))
    assert np.allclose(o["gv"].cpu().numpy(), -1 / (2 * np.sqrt(2.0))) and o["pb"][:, 2:].abs().sum().item() == 0


def test_guard_bands_of_the_objective():
    """every output inside a sentinel-filled buffer, GUARD doubles in front and behind, at sizes that end inside a workgroup"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    x = E.objective_inputs((5, 65, 65, "sqrt", 0.0, (70, 66, None)))
    T, H_v, n_s = x["v"].shape
    H_p, H_m = x["p"].shape[1], x["mu"].shape[1]
    shapes = dict(cost=(T,), steps=(T, H_v), gv=(T, H_v, n_s), pb=(T, H_p, n_s), mb=(T, H_m, n_s))
    bufs = {k: torch.full((int(np.prod(s)) + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=_dev()) for k, s in shapes.items()}
    ptr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 8 * GUARD)
    d = [_t(x[k]) for k in ("v", "p", "mu")] + [_t(0.1 * x["wx"]), _t(x["cost_bar"])]
    head = (0, T, 1, n_s, H_v, B.ptr(d[0]), 0.0, x["n_dev"], H_p, B.ptr(d[1]), H_m, B.ptr(d[2]), B.ptr(d[3]))
    s = B.stream_ptr(_dev())
    assert lib.sr_rollout_explore(*head, ptr("cost"), ptr("steps"), s) == 0
    assert lib.sr_rollout_explore_vjp(*head, B.ptr(d[4]), ptr("gv"), ptr("pb"), ptr("mb"), s) == 0
    for k, shp in shapes.items():
        flat = bufs[k].cpu().numpy()
        n = int(np.prod(shp))
        assert (flat[:GUARD] == SENTINEL).all() and (flat[GUARD + n:] == SENTINEL).all(), "%s: written outside" % k
        assert not (flat[GUARD:GUARD + n] == SENTINEL).any(), "%s: not every element written" % k


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s", (2, 4))
def test_the_default_cost_gradient_by_the_raw_reverse_call_and_by_autograd(n_s):
    """measured floor of the two routes in CPU torch at one stored forward: 2.88e-16 of the largest element (tests/test_explore_host.py),
    bar 30 x 2.9e-16 = 8.7e-15"""
    import torch
    from safe_exploration_amd import gp_reachability as reach, uncertainty_propagation_casadi as prop
    gp = width_gp(width_problem(900 + n_s, "rbf", n_s + 1, 60, n_s))
    safe, perf, wx = E.e2e_inputs(n_s)
    eps = E.E2E_EPS_NOISE
    grads = {}
    for which in ("raw", "autograd"):
        p_0 = _t(safe["p"]).requires_grad_(True)
        ls = dict(k_ff=_t(safe["k_ff"]).requires_grad_(True), k_fb=_t(safe["k_fb"]).requires_grad_(True))
        lp = dict(k_ff=_t(perf["k_ff"]).requires_grad_(True), k_fb=_t(perf["k_fb"]).requires_grad_(True))
        p_all, q_all, var_safe = reach.multistep_reachability_diff_batch(p_0, gp, ls["k_fb"], ls["k_ff"], safe["l_mu"], safe["l_sigma"], None,
                                                                         safe["c"], safe["a"], safe["b"], return_gp_var=True)
        mu_all, sigma_all, var_perf = prop.multistep_moments_diff_batch(p_0, gp, lp["k_ff"], lp["k_fb"], safe["a"], safe["b"], 1)
        leaves = [p_0, ls["k_ff"], ls["k_fb"], lp["k_ff"], lp["k_fb"]]
        if which == "raw":
            gv, pb, mb = reach.exploration_cost_vjp_batch(var_perf.detach(), "sqrt", n_s * eps, p_all.detach(), mu_all.detach(), wx)
            grads[which] = torch.autograd.grad([var_perf, p_all, mu_all], leaves, [gv, pb, mb])
            cost = reach.exploration_cost_batch(var_perf.detach(), "sqrt", n_s * eps, p_all.detach(), mu_all.detach(), wx)
            host = [reach.safempc_default_cost(p_all[t].detach().cpu().numpy(), var_safe[t].detach().cpu().numpy(), mu_all[t].detach().cpu().numpy(),
                                               var_perf[t].detach().cpu().numpy(), wx, eps_noise=eps) for t in range(E.E2E_T)]
            assert RR.rel_err(cost.cpu().numpy(), np.array(host)) <= E.OBJ_RTOL
        else:
            grads[which] = torch.autograd.grad(E.torch_default_cost(p_all, mu_all, var_perf, _t(wx), eps), leaves)
    names = ("p_0", "k_ff_safe", "k_fb_safe", "k_ff_perf", "k_fb_perf")
    errs = {k: RR.rel_err(a.cpu().numpy(), b.cpu().numpy()) for k, a, b in zip(names, grads["raw"], grads["autograd"])}
    print("n_s=%d: raw reverse call against autograd through the torch cost: %s of the largest element; share of the bar %.3f"
          % (n_s, {k: "%.2e" % v for k, v in errs.items()}, max(errs.values()) / E.E2E_RTOL))
    # the centres and the Taylor means do not depend on the feedback gains (they act on deviations), and this cost reads nothing else
    for k, g in zip(names, grads["raw"]):
        assert (np.abs(g.cpu().numpy()).max() > 0) == (not k.startswith("k_fb")), k
    assert max(errs.values()) <= E.E2E_RTOL, errs


# ---- the example --------------------------------------------------------------------------------------------------------------------
def test_the_example_runs_and_its_objective_goes_down():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "safe_exploration_objective.py")], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stdout + res.stderr
    vals = [float(line.split()[-1]) for line in res.stdout.splitlines() if line.startswith("step")]
    assert len(vals) >= 3 and vals[-1] < vals[0], res.stdout
    dist = [float(line.split()[-1]) for line in res.stdout.splitlines() if line.startswith("gradient distance")]
    assert len(dist) == 1 and dist[0] <= 1e-10, res.stdout
