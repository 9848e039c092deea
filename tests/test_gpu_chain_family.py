"""Multi-step chains (sr_multistep_reach, sr_multistep_moments) on every compiled instantiation of the persistent kernel
sr_chain_kernel<Np, DT, n_s, n_u> (Np in {128, 256, 384, 512} x six (n_s, n_u) pairs), in the three algebras its `mode` word
carries, on both routes (the persistent launch and the per-step launches), against the long-double reference of the WHOLE chain
of tests/_chain_ref.py at its bar (30 x the fp64 floor + 2 x the response to the accepted errors of the posterior, per case,
quantity and step; computed from the reference alone).  Every case asserts the route it ran on (gp.last_chain): a silent change
of route fails the test.

 a. every instantiation x {mode 0 from a point, mode 0 from (q0, k_fb0), mode 1, mode 2}, N = Np - 1 or Np - 127, T = 17, H = 5,
    both routes, each called twice for the same bits (neither route has a sum whose order depends on arrival: the tail workgroup
    adds the Np / 128 shares of |U^-T k*|^2 in the order of the parts);
 b. group and launch edges: T = 1, 15, 16, 16 gmax, 16 gmax + 1 (second launch with H = 3, per-step with H = 2), just beyond two
    launches, H = 1 and 2; gmax from the documented formula with the device's CU count;
 c. the H bound of the LDS control block: H_max on the persistent kernel, H_max + 1 per-step;
 d. state on one handle: calls with other H, T and mode one after another equal fresh handles to the bit; a roll-out does not
    depend on its batch-mates; release_scratch and a refit at another N;
 e. the per-step route where the persistent kernel never applies: N = 600, a chunk boundary inside the batch, an input transform;
 f. the C ABI conventions of sr_multistep_moments.
"""
import numpy as np
import pytest

import _chain_ref as C

pytestmark = pytest.mark.gpu
P_RR, Q_RR = dict(rtol=1e-8, atol=1e-11), dict(rtol=1e-7, atol=1e-14)      # route against route, as the existing chain test


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _fit(m):
    """a fresh handle with the model m"""
    from safe_exploration_amd import SimpleGPModel
    gp = SimpleGPModel(m.n_s, m.nx, m.n_u, kern_types=["rbf"] * m.n_s, hyp=m.hyp)
    gp.train(m.Z, m.Y, opt_hyp=False)
    return gp


_GPS = {}


def _gp(m):
    """one handle per model, shared between the cases of this module (the last few are kept)"""
    if id(m) not in _GPS:
        if len(_GPS) >= 4:
            _GPS.pop(next(iter(_GPS)))
        _GPS[id(m)] = _fit(m)
    return _GPS[id(m)]


def _run(gp, m, x, H, variant, rows=None):
    """one chain of `variant` over the roll-outs `rows` (all): p_all, q_all, gp_var_all (None in mode 0)"""
    from safe_exploration_amd import gp_reachability as reach, uncertainty_propagation_casadi as prop
    s = slice(None) if rows is None else rows
    if C.MODE[variant] == 0:
        q0, kfb0 = (x["q"][s], x["k_fb0"][s]) if variant == "q0" else (None, None)
        p, q = reach.multistep_reachability_batch(x["p"][s], gp, x["k_fb"][s], x["k_ff"][s], x["l_mu"], x["l_sigma"], q0, x["c"],
                                                  x["a"], x["b"], kfb0, t_z_gp=m.tz)
        return p, q, None
    return prop.multistep_moments_batch(x["p"][s], gp, x["k_ff"][s], x["k_fb"][s], x["a"], x["b"], C.MODE[variant], a_gp_inp_x=m.tz)


def _route(gp, m, x, H, variant, chain, rows=None, calls=1):
    """_run on the asked route, `calls` times with the same bits; asserts the route that ran"""
    gp.set_chain(chain)
    try:
        out = _run(gp, m, x, H, variant, rows)
        assert gp.last_chain == chain, "%s route expected" % ("persistent" if chain else "per-step")
        for _ in range(calls - 1):
            again = _run(gp, m, x, H, variant, rows)
            assert gp.last_chain == chain
            assert all(a is None or np.array_equal(a, b) for a, b in zip(out, again)), "two calls differ in their bits"
    finally:
        gp.set_chain(True)
    return out


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(u, v) for u, v in zip(a, b))


def _check(tag, got, ref, rows):
    """every element of p, q (and gp_var in the moment modes) of the roll-outs `rows`, step by step, within the step's bar"""
    rows = list(rows)
    for k, name in enumerate(("p", "q", "var")):
        if got[k] is None:
            continue
        g, want, bar = np.asarray(got[k])[rows], ref[name], ref["bar_" + name]
        assert g.shape == want.shape, (tag, name, g.shape, want.shape)
        assert np.isfinite(g).all(), "%s: %s not finite" % (tag, name)
        err = np.abs(g - want).max(axis=tuple(a for a in range(g.ndim) if a != 1))
        print("%s %s: worst share of the bar %.1e (bar %.1e .. %.1e)" % (tag, name, float((err / bar).max()), bar.min(), bar.max()))
        assert np.all(err <= bar), "%s: %s misses its bar at steps %s: err %s bar %s" % (
            tag, name, np.flatnonzero(err > bar), err[err > bar], bar[err > bar])


def _reference(m, x, H, rows, variant, T):
    return C.reference(m, x, H, rows, variant, key=(id(m), T, H, tuple(rows)))


_INPUTS = {}


def _inputs(n_s, n_u, T, H):
    key = (n_s, n_u, T, H)
    if key not in _INPUTS:
        _INPUTS[key] = C.inputs(n_s, n_u, T, H)
    return _INPUTS[key]


# ---- a. every instantiation x every mode ------------------------------------------------------------------------------------------
FAMILY = [c + (v,) for c in C.family() for v in C.VARIANTS]      # the variants of a model side by side: they share its fits


@pytest.mark.parametrize("cid,n_s,n_u,N,variant", FAMILY, ids=["%s-%s" % (c[0], c[4]) for c in FAMILY])
def test_every_instantiation_and_mode_on_both_routes(cid, n_s, n_u, N, variant):
    m, T, H = C.model(n_s, n_u, N), C.T_FAMILY, C.H_FAMILY
    x = _inputs(n_s, n_u, T, H)
    gp = _gp(m)
    assert gp._handle.Np_now() == m.Np
    ref = _reference(m, x, H, range(T), variant, T)
    for chain in (True, False):
        got = _route(gp, m, x, H, variant, chain, calls=2)
        _check("%s %s %s" % (cid, variant, "persistent" if chain else "per-step"), got, ref, range(T))


# ---- b. group and launch edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u,N", C.EDGE_MODELS)
def test_group_and_launch_edges(n_s, n_u, N):
    m, cus = C.model(n_s, n_u, N), _cus()
    gp = _gp(m)
    for T, H, variant, want_chain in C.edge_cases(n_s, n_u, N, cus):
        per = C.GROUP * C.gmax(m.Np, n_s, n_u, H, cus)
        assert want_chain == (C.launches(T, m.Np, n_s, n_u, H, cus) <= C.max_launches(T, H))
        x = _inputs(n_s, n_u, T, H)
        rows = C.edge_rows(T, per)
        tag = "edge ns%d N%d T%d H%d %s (%d per launch)" % (n_s, N, T, H, variant, per)
        got = _route(gp, m, x, H, variant, want_chain)
        _check(tag, got, _reference(m, x, H, rows, variant, T), rows)
        other = _route(gp, m, x, H, variant, False)
        for k, tol in ((0, P_RR), (1, Q_RR), (2, dict(rtol=0, atol=1e-9))):
            if got[k] is not None:
                np.testing.assert_allclose(got[k], other[k], err_msg=tag, **tol)


# ---- c. the H bound of the LDS control block ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_s,n_u,N", C.HMAX_MODELS)
def test_longest_chain_of_the_control_block(n_s, n_u, N):
    m, T = C.model(n_s, n_u, N), C.T_FAMILY
    gp = _gp(m)
    for variant, dh in C.HMAX_VARIANTS:
        H = C.h_max(n_s, n_u) + dh
        x = _inputs(n_s, n_u, T, H)
        got = _route(gp, m, x, H, variant, dh == 0)
        _check("hmax ns%d nu%d H%d %s" % (n_s, n_u, H, variant), got, _reference(m, x, H, range(T), variant, T), range(T))


# ---- d. state on one handle --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sequence", [C.STATE_SEQUENCE, C.STALE_SEQUENCE], ids=["modes", "tags"])
def test_calls_on_one_handle_equal_fresh_handles(sequence):
    """the tags of the exchange elements carry on from launch to launch, whatever H, T and mode the launches have: every
    result equals, to the bit, that of a fresh handle given only that call; and the reference"""
    m = C.model(2, 1, 200)
    one = _fit(m)
    for k, (variant, H, T) in enumerate(sequence):
        x = _inputs(2, 1, T, H)
        got = _route(one, m, x, H, variant, True)
        fresh = _route(_fit(m), m, x, H, variant, True)
        assert _same(got, fresh), "call %d (%s, H = %d, T = %d) differs from a fresh handle's" % (k, variant, H, T)
        rows = range(min(T, 48))
        _check("state %d %s H%d T%d" % (k, variant, H, T), got, _reference(m, x, H, rows, variant, T), rows)


def test_a_rollout_does_not_depend_on_its_batch_mates_and_a_refit_starts_clean():
    """Roll-out 16 of a batch of 17 equals the same roll-out run alone, to the bit, in every variant.  Then release_scratch and
    100 more rows ON THE SAME HANDLE (the exchange buffer and the groups' epochs stay; the padded size, and with it the layout of
    the exchange elements, changes from 256 to 384), and a refit of that handle: against the reference each time."""
    (n_s, n_u, N0), more, variant, H, T = C.REFIT
    m0, m1 = C.model(n_s, n_u, N0), C.refit_model()
    gp = _fit(m0)
    x = _inputs(n_s, n_u, T, H)
    for v in C.VARIANTS:
        full = _route(gp, m0, x, H, v, True)
        alone = _route(gp, m0, x, H, v, True, rows=slice(T - 1, T))
        assert _same([None if a is None else a[T - 1:] for a in full], alone), "%s: roll-out %d alone differs" % (v, T - 1)
    handle = gp._handle
    gp.release_scratch()
    gp.append_limit = more                                   # (by default a block of more than N / 5 rows refits into a new handle)
    gp.update_model(m1.Z[N0:], m1.Y[N0:], opt_hyp=False, replace_old=False)
    assert gp._handle is handle and handle.Np_now() == m1.Np != m0.Np
    ref = _reference(m1, x, H, range(T), variant, T)
    _check("grown to N%d %s" % (m1.N, variant), _route(gp, m1, x, H, variant, True, calls=2), ref, range(T))
    gp.release_scratch()
    gp.train(m1.Z, m1.Y, opt_hyp=False)
    assert gp._handle is handle
    _check("refit N%d %s" % (m1.N, variant), _route(gp, m1, x, H, variant, True, calls=2), ref, range(T))


# ---- e. the per-step route where the persistent kernel never applies ----------------------------------------------------------------
@pytest.mark.parametrize("cid,n_s,n_u,N,tz,T,H,chunk,variants", C.per_step_cases(), ids=[c[0] for c in C.per_step_cases()])
def test_per_step_route_where_the_persistent_kernel_never_applies(cid, n_s, n_u, N, tz, T, H, chunk, variants):
    m = C.model(n_s, n_u, N, tz=tz)
    gp = _gp(m)
    x = _inputs(n_s, n_u, T, H)
    rows = range(min(T, 48))
    if chunk is not None:
        gp.set_chunk(chunk)
    try:
        for variant in variants:
            gp.set_chain(True)
            got = _run(gp, m, x, H, variant)
            assert not gp.last_chain, "the persistent kernel does not apply here"
            _check("%s %s" % (cid, variant), got, _reference(m, x, H, rows, variant, T), rows)
    finally:
        gp.set_chunk(65536)


# ---- f. the C ABI conventions of sr_multistep_moments -------------------------------------------------------------------------------
def test_multistep_moments_c_abi():
    import torch
    from safe_exploration_amd import _buffers as B, _lib
    from safe_exploration_amd._lib import lib
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    n_s, n_u, T, H = 2, 1, 17, 4
    m = C.model(n_s, n_u, 200)
    gp = _gp(m)
    hd, dev = gp._handle, gp._handle.device
    s = B.stream_ptr(dev)
    x = _inputs(n_s, n_u, T, H)
    t = lambda v: torch.tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev)
    d = {k: t(x[k]) for k in ("p", "k_ff", "k_fb", "a", "b")}
    P = B.ptr

    def call(mode, T_=T, H_=H, mu0=True, k_fb=True, var=True, h=None):
        o = [torch.full(shape, float("nan"), dtype=torch.float64, device=dev) for shape in ((T, H_, n_s), (T, H_, n_s, n_s), (T, H_, n_s))]
        kff = d["k_ff"][:, :H_].contiguous()
        rc = lib.sr_multistep_moments(hd.h if h is None else h, T_, H_, mode, P(d["p"]) if mu0 else None, P(kff),
                                      P(d["k_fb"][:, :max(H_ - 1, 1)].contiguous()) if k_fb else None, P(d["a"]), P(d["b"]), P(o[0]), P(o[1]),
                                      P(o[2]) if var else None, s)
        torch.cuda.synchronize()
        return rc, [v.cpu().numpy() for v in o]

    for mode in (1, 2):
        rc, full = call(mode)
        assert rc == 0 and gp.last_chain
        assert all(np.isfinite(v).all() for v in full), "T = 17: an element of the NaN-prefilled outputs was not written"
        ref = _reference(m, x, H, range(T), "m%d" % mode, T)
        _check("C ABI mode %d" % mode, full, ref, range(T))
        rc, novar = call(mode, var=False)                                 # gp_var_all NULL: the same bits, nothing written there
        assert rc == 0 and np.array_equal(novar[0], full[0]) and np.array_equal(novar[1], full[1]) and np.isnan(novar[2]).all()
        rc, one = call(mode, H_=1, k_fb=False)                            # H = 1 needs no k_fb
        assert rc == 0 and np.array_equal(one[0][:, 0], full[0][:, 0]) and np.array_equal(one[1][:, 0], full[1][:, 0])
        rc, none = call(mode, T_=0)                                       # T = 0: nothing is touched
        assert rc == 0 and all(np.isnan(v).all() for v in none)
    for mode in (0, 3):
        assert call(mode)[0] == _lib.SR_EINVAL
    assert call(1, mu0=False)[0] == _lib.SR_EINVAL
    assert call(1, k_fb=False)[0] == _lib.SR_EINVAL                        # H > 1 without k_fb
    raw = _Handle(dev, 50, n_s + n_u, n_s)
    assert call(1, h=raw.h)[0] == _lib.SR_ESTATE and "not factorized" in _lib.last_error()
