"""The stored model -- U^-1 (`Wt`), alpha, log det, the breakdown index -- as sr_gp_factorize and sr_gp_append leave it, entry
by entry against the long-double reference of tests/_factor_ref.py, with the launch structure asserted (sr_gp_last_update).

Every prediction, gradient, moment, path and selection kernel reads this object; until now it was compared with a refit of the
same library at 1e-6 or looked at through the variance of a few queries.  Each case fits or appends through the public entry
points, exports alpha and Wt with sr_gp_export and wants
  * the cluster entries of U^-1, alpha, log det (and K^-1 where asked) under the a-priori bars of _factor_ref
    (c_b u kappa |W_c|_2 and its kin, times 1 + a after `a` appends: ~1e-11 relative),
  * the strict lower triangle 0.0, the front padding the identity, the off-cluster entries below 1e-200 |W| (mat52: 1e-24),
  * the report of sr_gp_last_update equal to a mirror of the drivers' predicates (expected_fit, AppendMirror); the host side,
    tests/test_factor_ref_host.py, holds the mirror and the case table against csrc/sr_common.h and the bars against two
    independent fp64 routes.
Fits: one block count either side of every rule of factorize_impl (FIT_NB), exact and nearly empty padding, mat52, a second round
of outputs, the smallest model of stream regime 2, forced panels; several models one after the other in one process; the
breakdown index.  Appends: the one-workgroup launch, the co-resident grid in place and not, the matrix-vector route, the
MFMA-tile route, each with the padded size staying and growing.  Default settings only: set_fact_pipeline(1 / 2 / 3) keep their
comparisons with the chain of launches this file pins (tests/test_gpu_parity.py).
The largest error / bar per case goes to stdout (-s); profiles/r16_model_state.txt keeps a run."""
import ctypes
import time

import numpy as np
import pytest

import _factor_ref as F

SEED = 11
NB = 128
# ---- restated from csrc/sr_common.h (tests/test_factor_ref_host.py parses the header and compares) -------------------------
SR_FACT_ONE_STREAM_MAX_NB, SR_FACT_CHAIN_MAX_NB, SR_FACT_SLOTS = 15, 128, 8
SR_APPEND1_MAX_NP0, SR_APPEND1G_MAX_NP0, SR_SMALL_T, SR_SLIDE_STEPS, SR_APPEND1_MAX_OUT = 512, 8192, 16, 128, 16
EARLY_INV_MIN_NB, STAGED_INV_MAX_NB, STAGED_INV_MIN_REST = 8, 24, 3       # (sr_capi_update.hip: early_inv, inv_min_rest)


def fact_panel(nb):
    return 2 if nb <= 28 else (3 if nb <= 44 else (4 if nb <= 64 else (8 if nb <= 200 else 24)))


def fact_reserved_cus(regime, nb):
    return 8 if regime == 2 else (64 if 36 < nb <= 52 else 32)


def inv_stages(nb, P, own_streams, regime):
    """stages of the inversion the plain chain launches beside itself: at the first panel end at or past nb / 2, then -- up to
    24 blocks -- halfway to the end again while three blocks remain (factorize_impl, restated)"""
    if not (regime == 1 and own_streams and nb >= EARLY_INV_MIN_NB):
        return 0
    min_rest = STAGED_INV_MIN_REST if nb <= STAGED_INV_MAX_NB else 1000
    trigger, n = nb // 2, 0
    for p1 in list(range(P, nb, P)):
        if p1 >= trigger:
            n += 1
            while trigger <= p1:
                nxt = (trigger + nb) // 2
                trigger = nxt if (nb - nxt >= min_rest and nxt > trigger) else nb + 1
    return n


def expected_fit(nb, n_out, panel=0):
    """what sr_gp_last_update must say after a fit on default settings (set_fact_pipeline(0))"""
    P = panel if panel > 0 else fact_panel(nb)
    regime = 1 if nb <= SR_FACT_CHAIN_MAX_NB else 2
    own = not (nb <= 2 and P >= nb) and not nb <= SR_FACT_ONE_STREAM_MAX_NB
    n_par = min(n_out, SR_FACT_SLOTS)
    return dict(kind="fit", nb=nb, panel=P, regime=regime, own_streams=int(own), n_par=n_par, rounds=-(-n_out // n_par),
                inv_stages=inv_stages(nb, P, own, regime), form="plain")


class AppendMirror(object):
    """the handle's state the append drivers decide by (sr_capi_append.hip), restated: N, Np, the slide of the views, the rows Z
    has room for, the spare U^-1 buffer"""

    def __init__(self, N, n_out, small_path=1):
        self.N, self.Np, self.n_out, self.small_path = N, -(-N // NB) * NB, n_out, small_path
        self.slide, self.z_cap, self.alt = 0, self.Np, False
        self.hold, self.aborts_row = 0, 0                  # the grid route rests after a launch that gave up (grid_hold)

    def append(self, m, grid_gave_up=False):
        """-> the report expected of sr_gp_last_update, and whether sr_gp_logdet_cached has a value.  grid_gave_up: the grid
        launch of this call did not become resident (sr_gp_grid_append_aborts advanced: another process held the CUs) and the
        library took the separate launches, as it does for the next `hold` one-point appends"""
        N1 = self.N + m
        Np0, Np1 = self.Np, -(-N1 // NB) * NB
        if m > SR_SMALL_T:
            route = "tile"
        elif m == 1 and self.small_path and Np0 <= SR_APPEND1_MAX_NP0 and Np1 <= SR_APPEND1_MAX_NP0 + NB:
            route = "one_wg"
        elif m == 1 and self.small_path and Np0 <= SR_APPEND1G_MAX_NP0 and self.n_out <= SR_APPEND1_MAX_OUT:
            route = "grid"
        else:
            route = "small"
        if route == "grid" and (grid_gave_up or self.hold > 0):
            if grid_gave_up:
                self.hold = 16 << min(self.aborts_row, 10)
                self.aborts_row += 1
            self.hold -= 1
            route = "small"
        elif route == "grid":
            self.aborts_row = 0
        if route == "grid" and Np1 == Np0 and self.slide < SR_SLIDE_STEPS - 1 and N1 <= self.z_cap:
            self.slide += 1
            self.N = N1
            return dict(kind="append", route="grid", in_place=1, Np0=Np0, Np1=Np0, spare=0), True
        spare = int(Np1 == Np0 and self.alt)
        self.slide = 0
        if route == "tile":
            self.z_cap = N1
        elif N1 > self.z_cap:
            self.z_cap = Np1
        self.alt = Np1 == Np0
        self.N, self.Np = N1, Np1
        return dict(kind="append", route=route, in_place=0, Np0=Np0, Np1=Np1, spare=spare), route != "tile"


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _fit(cid, nb, n_out=2, r=37, kern="rbf", D=3, panel=0, edge=None, vary_noise=False):
    return dict(id="%s-%s-D%d-n%d-nb%d-r%d%s" % (cid, kern, D, n_out, nb, r, "-P%d" % panel if panel else ""), nb=nb, N=NB * nb - r,
                n_out=n_out, kern=kern, D=D, panel=panel, edge=edge, vary_noise=vary_noise)


# (nb, the rule of factorize_impl whose last / first size it is)
FIT_NB = [(1, "one-block"), (2, "two-blocks"), (3, "two-blocks"), (4, "inv-tree"), (8, "early-inv"), (15, "one-stream"),
          (16, "one-stream"), (17, "inv-tree"), (24, "staged-inv"), (25, "staged-inv"), (28, "panel"), (29, "panel"),
          (36, "reserved"), (37, "reserved"), (44, "panel"), (45, "panel"), (52, "reserved"), (53, "reserved"), (64, "panel"),
          (65, "panel")]


def _fit_cases():
    cases = [_fit("edge", nb, 2 if nb < 44 else 1, edge=edge) for nb, edge in FIT_NB]
    for nb in (1, 3, 16):                                  # no padding at all; one real row in the first block
        cases += [_fit("pad", nb, r=0), _fit("pad", nb, r=127)]
    cases.append(_fit("mat52", 5, kern="mat52", D=6))
    # the second round of n_par outputs (d0 = 8); every output with a noise variance of its own (h->noise + d0)
    cases.append(_fit("rounds", 3, n_out=9, vary_noise=True))
    for P in (1, 3, 5, 64):                                # a short last panel, a boundary at nb / 2, no panel at all
        cases.append(_fit("panel", 7, panel=P))
    cases.append(_fit("panel", 17, panel=4))
    return cases


FIT_CASES = _fit_cases()
BIG = _fit("regime2", 129, n_out=1, r=12, edge="regime")    # N = 16500: the smallest model of stream regime 2


def _app(cid, N0, steps, n_out=2, kern="rbf", D=3, small_path=1, host=False, inv_k=False, give_up=0):
    return dict(give_up=give_up, id="%s-%s-n%d-N%d+%s" % (cid, kern, n_out, N0, "+".join(str(m) for m in steps)), N0=N0, steps=steps, n_out=n_out,
                kern=kern, D=D, small_path=small_path, host=host, inv_k=inv_k, route=cid.split("/")[0])


def _append_cases():
    c = [_app("one_wg", 127, [1]), _app("one_wg", 128, [1]), _app("one_wg", 511, [1, 1]), _app("one_wg/host", 511, [1, 1], host=True),
         _app("grid", 600, [1, 1, 1]), _app("grid", 640, [1]), _app("grid", 1151, [1, 1]), _app("grid", 8100, [1], n_out=1),
         _app("small/np0", 8200, [1], n_out=1), _app("small/path0", 600, [1], small_path=0)]
    for N0 in (600, 1100):
        c += [_app("small", N0, [2]), _app("small", N0, [16])]
    c.append(_app("small", 1145, [16]))                    # across a padding boundary
    # a grid that cannot assemble (the library's own diagnostic makes the first launch give up): separate launches, then rest
    c.append(_app("small/gave_up", 600, [1, 1], give_up=1))
    for N0 in (100, 600, 1000):                            # Np0 = 640: one full 512-row K slice and a cut one; 1024: two full
        for m in (17, 50, 128):
            c.append(_app("tile", N0, [m]))
    c += [_app("tile", 600, [20, 19]),                     # the padded size stays: the second one writes the spare buffer
          _app("tile", 630, [17]),                         # the padded size grows
          _app("tile", 640, [128]), _app("tile", 600, [33], kern="mat52"),
          _app("mixed", 1100, [1, 16, 50, 1], inv_k=True)]
    return c


APPEND_CASES = _append_cases()
BREAKDOWN = [(3, 2), (17, 2), (3, 9)]                      # (nb, n_out)


def breakdown_rows(nb):
    N = NB * nb - 37
    return [0, 5, NB - 37, 2 * NB - 37 + 41, N - 1]        # row 0, 5, the first row of block 1, a row inside block 2, the last


# ---- the device side -----------------------------------------------------------------------------------------------------
RATIOS = {}                      # case id -> dict of the largest error / bar seen


def _new_model(prob, n_out=None, panel=0):
    from safe_exploration_amd import SimpleGPModel
    n = prob.n_out if n_out is None else n_out
    gp = SimpleGPModel(n, prob.D - 1, 1, kern_types=[prob.kern] * n, hyp=F.hyp_of(prob)[:n])
    if panel:
        gp.set_fact_panel(panel)
    return gp


def _train(prob, n_out=None, panel=0):
    gp = _new_model(prob, n_out, panel)
    gp.train(prob.Z, prob.Y[:, :gp.n_s_out], opt_hyp=False)
    return gp


def _dims(gp):
    from safe_exploration_amd._lib import lib, check
    N, D, n, Np = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_long()
    check(lib.sr_gp_dims(gp._handle.h, ctypes.byref(N), ctypes.byref(D), ctypes.byref(n), ctypes.byref(Np)))
    return N.value, Np.value


def _logdet(gp):
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    out = torch.full((hd.n_out,), float("nan"), dtype=torch.float64, device=hd.device)
    check(lib.sr_gp_logdet(hd.h, B.ptr(out), B.stream_ptr(hd.device)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_state(what, gp, ref, cached_logdet=False):
    """alpha, U^-1 and log det of gp against ref under the bars; returns the exported (alpha, Wt) device tensors"""
    import torch
    from safe_exploration_amd._lib import lib
    p = ref.p
    N, Np = _dims(gp)
    assert (N, Np) == (p.N, -(-p.N // NB) * NB) and (gp._handle.N, gp._handle.Np) == (N, Np), (what, N, Np)
    alpha, wt = gp.export_state()
    torch.cuda.synchronize()
    assert tuple(wt.shape) == (p.n_out, Np, Np)
    got = dict(alpha=ref.alpha_ratio(alpha.cpu().numpy()), cluster=0.0, off=0.0, lower=0.0, padding=0.0, logdet=0.0)
    for d in range(p.n_out):
        r = ref.check_wt(d, lambda r0, r1: wt[d, r0:r1].cpu().numpy(), Np)
        for k in r:
            got[k] = max(got[k], r[k])
    ld = _logdet(gp)
    lds = [ld]
    if cached_logdet:
        host = (ctypes.c_double * p.n_out)()
        assert lib.sr_gp_logdet_cached(gp._handle.h, host) == 0, (what, "no host copy of log det")
        lds.append(np.array(host[:]))
    for d in range(p.n_out):
        for v in lds:
            got["logdet"] = max(got["logdet"], abs(v[d] - ref.logdet(d)) / ref.bar_logdet(d))
    print("%-44s err/bar U^-1 %.3g alpha %.3g logdet %.3g  off-cluster %.3g  lower %.3g padding %.3g"
          % (what, got["cluster"], got["alpha"], got["logdet"], got["off"], got["lower"], got["padding"]))
    RATIOS[what] = got
    assert got["lower"] == 0.0, (what, "strict lower triangle", got)
    assert got["padding"] == 0.0, (what, "front padding", got)
    assert got["off"] <= 1.0, (what, "off-cluster entries", got)
    assert got["cluster"] <= 1.0, (what, "U^-1", got)
    assert got["alpha"] <= 1.0, (what, "alpha", got)
    assert got["logdet"] <= 1.0, (what, "log det", got)
    return alpha, wt


def _data_conditions(ref, Np):
    for d in range(ref.p.n_out):
        ref.tile_conditions(d, Np)


@pytest.mark.gpu
@pytest.mark.parametrize("c", FIT_CASES, ids=[c["id"] for c in FIT_CASES])
def test_fit_against_reference(c):
    prob, ref = F.cached(SEED, c["N"], c["D"], c["n_out"], c["kern"], c["vary_noise"])
    _data_conditions(ref, NB * c["nb"])
    gp = _train(prob, panel=c["panel"])
    assert gp.last_update() == expected_fit(c["nb"], c["n_out"], c["panel"]), (c["id"], gp.last_update())
    _check_state(c["id"], gp, ref)


@pytest.mark.gpu
def test_second_round_of_outputs_equals_the_first_eight():
    """9 outputs are two rounds of the batch (8 + 1): outputs 0 .. 7 bit-equal to a fit of those eight alone"""
    import torch
    c = next(c for c in FIT_CASES if c["n_out"] == 9)
    prob, _ = F.cached(SEED, c["N"], c["D"], c["n_out"], c["kern"], c["vary_noise"])
    a9, w9 = _train(prob).export_state()
    a8, w8 = _train(prob, n_out=8).export_state()
    torch.cuda.synchronize()
    assert torch.equal(a9[:8], a8) and torch.equal(w9[:8], w8)


@pytest.mark.gpu
def test_smallest_model_of_stream_regime_2():
    """N = 16500 (129 blocks): two bulk streams and the free-ratio choice.  Three N x N buffers of 2.2 GB each plus the export;
    the one case that may take tens of seconds (its time goes to stdout)"""
    import torch
    free, _ = torch.cuda.mem_get_info()
    if free < 14 * 2 ** 30:
        pytest.skip("N = 16500 needs 14 GB of device memory, %.1f free (no smaller model reaches regime 2)" % (free / 2.0 ** 30))
    c = BIG
    t0 = time.perf_counter()
    prob = F.problem(SEED, c["N"], c["D"], c["n_out"], c["kern"])
    ref = F.FactorRef(prob)
    _data_conditions(ref, NB * c["nb"])
    t1 = time.perf_counter()
    gp = _train(prob)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert gp.last_update() == expected_fit(c["nb"], c["n_out"]), gp.last_update()
    _check_state(c["id"], gp, ref)
    print("%s: reference %.1f s, first fit %.1f s, comparison %.1f s" % (c["id"], t1 - t0, t2 - t1, time.perf_counter() - t2))
    gp.release_scratch()


@pytest.mark.gpu
def test_many_models_one_after_the_other():
    """17 blocks, then 7, then 17 again on one SimpleGPModel, then 9 outputs at 3 blocks.  A handle's N is fixed when it is made,
    so SimpleGPModel makes a NEW handle at every change of size: what the sequence shares is the process' state -- the stream
    sets, the device-memory block cache the handles' buffers come from and go back to -- and every export must be bit-equal to
    that of a model made for the size alone.  On ONE handle: the same fit twice (the U^-1 buffer, its never-written lower
    triangle and the scratch are met as the first fit left them) and a refit after release_scratch give the same bits.  A fit
    on a handle whose padded size changed is test_refit_on_a_handle_whose_padded_size_grew"""
    import torch
    probs = {nb: F.cached(SEED, NB * nb - 37, 3, 2, "rbf")[0] for nb in (17, 7)}
    gp = _new_model(probs[17])
    for nb in (17, 7, 17):
        p = probs[nb]
        gp.train(p.Z, p.Y, opt_hyp=False)
        assert gp.last_update() == expected_fit(nb, 2)
        a, w = gp.export_state()
        a1, w1 = _train(p).export_state()
        torch.cuda.synchronize()
        assert torch.equal(a, a1) and torch.equal(w, w1), "nb = %d after other sizes differs from a fresh model" % nb
    p9 = F.cached(SEED, NB * 3 - 37, 3, 9, "rbf")[0]
    g9 = _train(p9)
    a9, w9 = g9.export_state()
    p = probs[17]
    gp.train(p.Z, p.Y, opt_hyp=False)                      # the same handle, the same data: the same bits
    a2, w2 = gp.export_state()
    torch.cuda.synchronize()
    assert torch.equal(a2, a) and torch.equal(w2, w)
    gp.release_scratch()
    gp.train(p.Z, p.Y, opt_hyp=False)
    a3, w3 = gp.export_state()
    g9.train(p9.Z, p9.Y, opt_hyp=False)
    a9b, w9b = g9.export_state()
    torch.cuda.synchronize()
    assert torch.equal(a3, a) and torch.equal(w3, w), "refit after release_scratch differs"
    assert torch.equal(a9b, a9) and torch.equal(w9b, w9)


def _raw_fit(gp, handle, Z, Y, nugget):
    """sr_gp_set_data + sr_gp_factorize on a handle of our own: (status, info)"""
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    s = B.stream_ptr(handle.device)
    gp._set_data(handle, Z, Y, np.asarray(nugget, dtype=np.float64), handle.device, s)
    info = (ctypes.c_int * handle.n_out)()
    rc = lib.sr_gp_factorize(handle.h, s, info)
    return rc, list(info)


def _raw_export(handle):
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib
    alpha = B.empty((handle.n_out, handle.N), handle.device)
    wt = B.empty((handle.n_out, handle.Np, handle.Np), handle.device)
    rc = lib.sr_gp_export(handle.h, B.ptr(alpha), B.ptr(wt), B.stream_ptr(handle.device))
    torch.cuda.synchronize()
    return rc, alpha, wt


@pytest.mark.gpu
@pytest.mark.parametrize("nb,n_out", BREAKDOWN)
def test_breakdown_index(nb, n_out):
    """a NaN in Z[r] makes pivot r the first that is not positive (r = 0: pivot 1, see below), for every output: SR_ENOTPD,
    info[d] == r + 1, the handle not factorized; a clean refit on it is bit-equal to a fresh handle.  With 9 outputs, output 8 (the second round) also gets
    a nugget of -(sf2 + 1): its first pivot fails, the others still say r + 1"""
    import torch
    from safe_exploration_amd import _buffers as B, _lib
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    prob, _ = F.cached(SEED, NB * nb - 37, 3, n_out, "rbf")
    gp = _new_model(prob)
    dev = B.resolve_device(gp._device_arg)
    fresh = _Handle(dev, prob.N, prob.D, n_out)
    rc, info = _raw_fit(gp, fresh, prob.Z, prob.Y, prob.nugget)
    assert rc == 0 and info == [0] * n_out
    _, a0, w0 = _raw_export(fresh)
    hd = _Handle(dev, prob.N, prob.D, n_out)
    for r in breakdown_rows(nb):
        Z = prob.Z.copy()
        Z[r, 1] = np.nan
        nugget = prob.nugget.copy()
        # (the Gram kernels write the diagonal as sf2 + noise without looking at the inputs and row 0 has no row above it:
        #  its own pivot stays finite, U[0][1] is the first NaN and pivot 1 the first to fail)
        want = [r + 1 if r > 0 else 2] * n_out
        if n_out > SR_FACT_SLOTS:
            nugget[8] = -(prob.sf2[8] + 1.0)
            want[8] = 1
        rc, info = _raw_fit(gp, hd, Z, prob.Y, nugget)
        assert rc == _lib.SR_ENOTPD and info == want, (r, rc, info)
        assert _raw_export(hd)[0] == _lib.SR_ESTATE, "a handle whose fit broke down says it is factorized"
        rc, info = _raw_fit(gp, hd, prob.Z, prob.Y, prob.nugget)
        assert rc == 0 and info == [0] * n_out
        rc, a1, w1 = _raw_export(hd)
        assert rc == 0 and torch.equal(a1, a0) and torch.equal(w1, w0), "refit after a breakdown at row %d differs" % r


@pytest.mark.gpu
def test_last_update_refusals():
    """a NULL buffer and cap < 1 are refused; a short buffer gets its words; before any update the kind is 0"""
    from safe_exploration_amd import _buffers as B, _lib
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    prob, _ = F.cached(SEED, NB - 37, 3, 2, "rbf")
    gp = _new_model(prob)
    hd = _Handle(B.resolve_device(gp._device_arg), prob.N, prob.D, 2)
    out = (ctypes.c_int * 9)(*([7] * 9))
    assert _lib.lib.sr_gp_last_update(hd.h, None, 9) == _lib.SR_EINVAL and _lib.lib.sr_gp_last_update(hd.h, out, 0) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_update(hd.h, out, 9) == 9 and list(out) == [0] * 9
    assert _raw_fit(gp, hd, prob.Z, prob.Y, prob.nugget)[0] == 0
    out = (ctypes.c_int * 9)(*([7] * 9))
    assert _lib.lib.sr_gp_last_update(hd.h, out, 3) == 3 and list(out) == [1, 1, 2] + [7] * 6
    assert _lib.lib.sr_gp_last_update(hd.h, out, 20) == 9


def _grid_aborts(gp):
    from safe_exploration_amd._lib import lib, check
    n = ctypes.c_long(-1)
    check(lib.sr_gp_grid_append_aborts(gp._handle.h, ctypes.byref(n)))
    return n.value


def _slide_steps(gp):
    from safe_exploration_amd._lib import lib, check
    k = ctypes.c_int(-1)
    check(lib.sr_gp_slide_steps(gp._handle.h, ctypes.byref(k)))
    return k.value


def _append(gp, x, y, host):
    """sr_gp_append (or, one point in host memory, sr_gp_append1_host) on the model's handle; the Python side's sizes follow"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    s = B.stream_ptr(hd.device)
    info = (ctypes.c_int * hd.n_out)()
    if host:
        xr, yr = np.ascontiguousarray(x[0]), np.ascontiguousarray(y[0])
        check(lib.sr_gp_append1_host(hd.h, ctypes.c_void_p(xr.ctypes.data), ctypes.c_void_p(yr.ctypes.data), s, info))
    else:
        tx, ty = B.as_dev(np.ascontiguousarray(x), hd.device), B.as_dev(np.ascontiguousarray(y), hd.device)
        check(lib.sr_gp_append(hd.h, B.ptr(tx), B.ptr(ty), x.shape[0], s, info))
        torch.cuda.synchronize()
    assert list(info) == [0] * hd.n_out
    hd.N, hd.Np = _dims(gp)
    gp._beta = gp._inv_K = gp._inv_K_dev = None


@pytest.mark.gpu
@pytest.mark.parametrize("c", APPEND_CASES, ids=[c["id"] for c in APPEND_CASES])
def test_append_against_reference(c):
    """after every call: U^-1, alpha, N / Np, log det (the host copy too after <= 16 points), the report and the slide.
    The grid route assumes a device it can fill: where a grid launch gives up because another process holds the CUs
    (sr_gp_grid_append_aborts advances) the library appends by separate launches by design, and the mirror follows it"""
    from safe_exploration_amd._lib import lib, check
    prob = F.problem(SEED, c["N0"], c["D"], c["n_out"], c["kern"])
    gp = _train(prob)
    mirror = AppendMirror(c["N0"], c["n_out"], c["small_path"])
    try:
        if c["small_path"] != 1:
            gp.set_small_path(c["small_path"])
        if c["give_up"]:
            check(lib.sr_test_grid_append_abort(c["give_up"]))
        for a, m in enumerate(c["steps"], 1):
            x, y, q = prob.new_points(m, a)
            before = _grid_aborts(gp)
            _append(gp, x, y, c["host"] and m == 1)
            gave_up = _grid_aborts(gp) > before
            assert gave_up == (a <= c["give_up"]) or not c["give_up"], (c["id"], a, gave_up)
            expect, cached = mirror.append(m, gave_up)
            prob = prob.grown(x, y, q)
            assert gp.last_update() == expect, (c["id"], a, gp.last_update(), expect)
            assert _slide_steps(gp) == mirror.slide, (c["id"], a)
            ref = F.FactorRef(prob, appends=a)
            _data_conditions(ref, mirror.Np)
            _check_state("%s step %d" % (c["id"], a), gp, ref, cached_logdet=cached)
        if c["inv_k"]:
            worst = dict(cluster=0.0, off=0.0)
            for d, k in enumerate(gp.inv_K):
                r = ref.check_inv_k(d, k)
                worst = {key: max(worst[key], r[key]) for key in worst}
            print("%-44s err/bar K^-1 %.3g  off-cluster %.3g" % (c["id"], worst["cluster"], worst["off"]))
            RATIOS[c["id"] + " K^-1"] = worst
            assert worst["cluster"] <= 1.0 and worst["off"] <= 1.0, worst
    finally:
        gp.set_small_path(1)
        if c["give_up"]:
            check(lib.sr_test_grid_append_abort(0))


@pytest.mark.gpu
@pytest.mark.parametrize("N0,m", [(630, 17), (2139, 50), (640, 1)])
def test_refit_on_a_handle_whose_padded_size_grew(N0, m):
    """the one public route on which a handle's Np changes under a fit: an append that grows Np (640 -> 768 on the tile route
    and on the grid, 17 -> 18 blocks), then sr_gp_set_data + sr_gp_factorize of the grown data on THAT handle.  The fit meets the
    handle's scratch (fact_ws) and inversion job lists (inv_jobs, cached by Np) of the old size and the U^-1 buffer the append
    left: it must say it ran as a fit of the new size, agree with the reference and be bit-equal to a fresh handle"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle
    prob = F.problem(SEED, N0, 3, 2, "rbf")
    gp = _train(prob)
    nb0 = gp._handle.Np // NB
    x, y, q = prob.new_points(m, 1)
    _append(gp, x, y, False)
    prob = prob.grown(x, y, q)
    hd = gp._handle
    assert hd.Np == NB * (nb0 + 1) and gp.last_update()["Np1"] == hd.Np
    rc, info = _raw_fit(gp, hd, prob.Z, prob.Y, prob.nugget)
    assert rc == 0 and info == [0, 0]
    assert gp.last_update() == expected_fit(nb0 + 1, 2), gp.last_update()
    assert _slide_steps(gp) == 0
    alpha, wt = _check_state("refit on the grown handle N%d+%d" % (N0, m), gp, F.FactorRef(prob))
    fresh = _Handle(B.resolve_device(gp._device_arg), prob.N, prob.D, 2)
    assert _raw_fit(gp, fresh, prob.Z, prob.Y, prob.nugget)[0] == 0
    rc, a1, w1 = _raw_export(fresh)
    assert rc == 0 and torch.equal(alpha, a1) and torch.equal(wt, w1), "the refit on the grown handle differs from a fresh handle"


@pytest.mark.gpu
def test_margins():
    """runs last in this file: the thinnest margin of the run"""
    if not RATIOS:
        return
    what, key = max(((w, k) for w in RATIOS for k in ("cluster", "alpha", "logdet") if k in RATIOS[w]), key=lambda t: RATIOS[t[0]][t[1]])
    print("thinnest margin: %s, %s at %.3g of its bar (%d states compared)" % (what, key, RATIOS[what][key], len(RATIOS)))
