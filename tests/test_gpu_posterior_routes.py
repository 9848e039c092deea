"""Every kernel form of one posterior pass (csrc/sr_capi_posterior.hip: gp_pass) against the long-double reference of
tests/_posterior_ref.py, with the route asserted.

gp_pass picks one of about twenty kernel forms from (Np, T, D, n_out, kernel family, slide state, CU count).  Every case
below names the form it aims at (CASES: built on the CPU, checked by tests/test_posterior_ref_host.py against
sr_test_stream_plan and the thresholds of sr_common.h), and then
  * calls sr_gp_predict with Jacobians on caller buffers that carry NaN sentinels behind the outputs,
  * compares mu, sigma^2 and d mu / dx with the reference under the a-priori bars of _posterior_ref.bars (the textbook bound
    of a Cholesky solve on the query's own 90-point block: ~2e-11 relative; forty times below the project's bars),
  * asserts sr_gp_last_route == the form (expected_route: a mirror of gp_pass's predicates on top of the library's own
    planner sr_test_stream_plan, plus the case's declared target),
  * repeats the call and wants the same bits,
  * asserts, on the reference side, that the data can tell: median sigma^2 / k(x,x) < 0.5, a Jacobian that is not flat and --
    from 5 queries on -- every (256-column block, 128-row chunk) pair of the padded U^-1 changing k*^T K^-1 k* of some query
    by at least 1e-6 (bars: 2e-11) when dropped.
The largest observed error / bar per route goes to stdout (-s); profiles/r15_posterior_routes.txt keeps a run.

Sizes are N = Np - r: every form at r = 0, the first shape of every streamed form and one shape of every other route also at
r in RS (the k range starts at (Np - N) rounded down to 16).  "general" is mat52, "wide" is ARD-RBF with D = 6; lin_rbf / lin_mat52 are not local and stay
with tests/test_gpu_parity.py and tests/test_gpu_widths.py."""
import ctypes

import numpy as np
import pytest

import _posterior_ref as R

N_CU = 256                      # compute units of the MI355X: the streamed plan depends on it (sr_stream_items)
RS = (1, 15, 16, 17, 127)
PAD = 64                        # NaN sentinels behind every output buffer

# ---- thresholds restated from csrc/sr_common.h (tests/test_posterior_ref_host.py parses the header and compares) ----------
SR_FUSED_NP, SR_FUSED_T, SR_STREAM_MIN_NP, SR_STREAM_MAX_T, SR_SMALL_T = 512, 1024, 384, 64, 16
SR_ONE_STREAMED_NP, SR_MFMA_SMALL_MAX_NP, SR_STREAM_FUSED_MAX_D, SR_STREAM_FUSED32_MAX_NCB = 384, 2048, 5, 8
SR_FINAL_WAVE_T, SR_ST1_SLOTS_MAX, K0_MAX_D, FUSED16_MAX_NCB, REDUCE_REGS = 4096, 1536, 8, 28, 12
BAL_THR, VAR_SMALL_BYTES, VAR_SMALL_GROUPS, VAR64_MAX_NP, VAR64_WGS, SPLITK_WGS, NSPLIT_WGS = 8192, 300e6, 64, 1024, 256, 1024, 768


def stream_width(ncols):
    return 1 if ncols <= 1 else next(w for w in (4, 16, 32, 64, 128) if ncols <= w)


def stream_plan(Np, n_out, ncols, n_cu, can_fuse):
    """(g, kc, kr, nitems, nwg, items of the last column block) from the library's own planner (host only)"""
    from safe_exploration_amd import _lib
    out = (ctypes.c_int * 6)()
    assert _lib.lib.sr_test_stream_plan(Np, n_out, ncols, n_cu, int(can_fuse), out) == 0
    return tuple(out)


def pick_nsplit(Np, n_out, Tp):
    blocks = -(-Tp // 256) * n_out
    ns = -(-NSPLIT_WGS // blocks)
    maxs = Np // 16 if Tp <= SR_FINAL_WAVE_T else min(Np // 16, max(16, Np // 128))
    return max(1, min(ns, maxs))


def var_small_groups_max(Np, n_out):
    return max(1, min(VAR_SMALL_GROUPS, int(VAR_SMALL_BYTES / (float(n_out) * Np * Np * 4.0))))


def expected_route(Np, T, D, n_out, general, n_cu=N_CU, small_path=1, slide=0):
    """what sr_gp_last_route must say for one pass: the predicates of gp_pass / stream_predict / sr_launch_stream, restated"""
    e = dict(route=None, src=0, width=0, nc=0, kc=0, kr=0, nitems=0, nwg=0, multi=0, reduce_items=0, polled=0, nsplit=0, bal_wgs=0,
             final=0, unslid=0, T=T)
    rbf_narrow = not general and D <= SR_STREAM_FUSED_MAX_D
    one_streamed = Np == SR_ONE_STREAMED_NP and T == 1 and rbf_narrow
    k0 = Np <= SR_FUSED_NP and T <= SR_FUSED_T and D <= K0_MAX_D and not (Np == 512 and T <= 128)
    if small_path == 1 and not one_streamed and k0:
        e["route"] = "K0"
        return e
    if small_path != 0 and (Np > SR_STREAM_MIN_NP or (one_streamed and small_path == 1)) and T <= SR_STREAM_MAX_T:
        ncb = (Np + 255) // 256
        mfma_small = 2 <= T <= 4 and Np <= SR_MFMA_SMALL_MAX_NP
        wmin = 16 if mfma_small else 0
        nc = max(stream_width(T), wmin)
        fused_mfma = False
        if rbf_narrow and (T > 4 or mfma_small):
            g, kc = stream_plan(Np, n_out, nc, n_cu, True)[:2]
            fused_mfma = kc == 1 and (g == 1 or (g == 2 and ncb <= SR_STREAM_FUSED32_MAX_NCB))
        fused = (rbf_narrow and T <= 4 and not mfma_small) or fused_mfma
        e.update(src=int(fused), nc=nc, nsplit=2 * ncb if fused else pick_nsplit(Np, n_out, 128))
        if nc <= 4:
            nslot = n_out * ncb * (1 + 2 * (1 + D))
            e.update(route="stream1", width=nc, polled=int(fused and T == 1 and nslot <= SR_ST1_SLOTS_MAX and 2 * ncb <= 64))
            return e
        g, kc, kr, nitems, nwg, last = stream_plan(Np, n_out, nc, n_cu, fused)
        e.update(route="mfma1" if kc == 1 else "runs", width=g, kc=kc)
        if kc > 1:
            e.update(kr=kr, nitems=nitems, nwg=nwg, multi=int(g == 4 and nwg < nitems), reduce_items=last)
        return e
    Tp = -(-T // 128) * 128
    nrb = Np // 128
    e.update(nsplit=pick_nsplit(Np, n_out, Tp), final=1 if T <= SR_FINAL_WAVE_T else 2)
    wgs = nrb * (Tp // 128) * n_out
    if small_path and Np > SR_STREAM_MIN_NP and (T <= SR_SMALL_T or
                                                 (small_path == 1 and T <= SR_SMALL_T * var_small_groups_max(Np, n_out))):
        e["route"] = "K2s"
        return e
    if small_path and nrb > 2 and wgs <= SPLITK_WGS:
        U = n_out * (Tp // 128) * nrb * (nrb + 1) // 2
        e.update(route="K2b", bal_wgs=512 if U >= BAL_THR else (256 if U >= 256 else U))
    elif small_path and Np <= VAR64_MAX_NP and wgs < VAR64_WGS:
        e["route"] = "K2m"
    else:
        e["route"] = "K2"
    e["unslid"] = slide & 1
    return e


# ---- the cases --------------------------------------------------------------------------------------------------------
def _case(cid, Np, n_out, T, kern="rbf", D=3, r=0, **target):
    return dict(id="%s-%s-D%d-n%d-Np%d-r%d-T%d" % (cid, kern, D, n_out, Np, r, T), Np=Np, n_out=n_out, T=T, kern=kern, D=D, r=r,
                form=cid, target=target)


def _streamed_forms():
    """(form, [shapes (Np, n_out, T, kern, D)], target): the streamed kernel forms of the issue's table, confirmed at 256 CUs"""
    m1, runs = "mfma1", "runs"
    return [
        ("mfma1-G1-src1", [(512, 1, 2, "rbf", 3)], dict(route=m1, width=1, src=1, nc=16)),
        ("mfma1-G1-src0", [(512, 1, 2, "mat52", 3)], dict(route=m1, width=1, src=0, nc=16)),
        ("mfma1-G2-src1", [(1408, 4, 33, "rbf", 3)], dict(route=m1, width=2, src=1, nc=64)),
        ("mfma1-G2-src0", [(1408, 4, 33, "mat52", 3)], dict(route=m1, width=2, src=0, nc=64)),
        ("mfma1-G4-src0", [(1920, 4, 33, "rbf", 3)], dict(route=m1, width=4, src=0, nc=64)),
        ("runs-G1", [(1152, 4, 33, "rbf", 3)], dict(route=runs, width=1, multi=0, reduce_gt=0)),
        ("runs-G1-reduce13", [(3456, 1, 17, "rbf", 3)], dict(route=runs, width=1, multi=0, reduce_gt=1)),
        ("runs-G2", [(1664, 4, 33, "rbf", 3)], dict(route=runs, width=2, multi=0, reduce_gt=0)),
        ("runs-G2-reduce13", [(3456, 1, 33, "rbf", 3)], dict(route=runs, width=2, multi=0, reduce_gt=1)),
        ("runs-G4", [(2432, 4, 33, "rbf", 3)], dict(route=runs, width=4, multi=0, reduce_gt=0)),
        ("runs-G4-reduce13", [(3456, 2, 33, "rbf", 3)], dict(route=runs, width=4, multi=0, reduce_gt=1)),
        ("runs-G4-MULTI", [(2944, 4, 33, "rbf", 3), (2944, 4, 64, "rbf", 3)], dict(route=runs, width=4, multi=1, reduce_gt=0)),
        ("runs-G4-MULTI-reduce13", [(4224, 2, 33, "rbf", 3)], dict(route=runs, width=4, multi=1, reduce_gt=1)),
        ("stream1-TQ1-src1", [(640, 2, 1, "rbf", 3), (640, 2, 1, "rbf", 5)], dict(route="stream1", width=1, src=1, polled=1)),
        ("stream1-TQ4-src1", [(2176, 2, 3, "rbf", 3), (2176, 2, 3, "rbf", 5)], dict(route="stream1", width=4, src=1)),
        ("stream1-TQ1-src0", [(640, 2, 1, "rbf", 6), (640, 2, 1, "mat52", 3)], dict(route="stream1", width=1, src=0, polled=0)),
        ("stream1-TQ4-src0", [(2176, 2, 3, "rbf", 6), (2176, 2, 3, "mat52", 3)], dict(route="stream1", width=4, src=0)),
    ]


def _build_cases():
    cases = []
    for form, shapes, target in _streamed_forms():
        for i, (Np, n_out, T, kern, D) in enumerate(shapes):
            for r in ((0,) + RS if i == 0 else (0,)):
                cases.append(_case(form, Np, n_out, T, kern, D, r, **target))
    # -- further edges of the streamed route
    for T in (2, 4):              # SR_MFMA_SMALL_MAX_NP: 2 .. 4 queries on the MFMA kernel up to 2048 padded rows, the VALU kernel beyond
        cases.append(_case("mfma-small-max-np", 2048, 2, T, route="mfma1", width=1, src=1, nc=16))
        cases.append(_case("mfma-small-max-np", 2176, 2, T, route="stream1", width=4, src=1))
    # SR_STREAM_FUSED32_MAX_NCB: 32 columns per workgroup evaluate their K* rows up to 8 column blocks
    cases.append(_case("fused32-max-ncb", 2048, 4, 32, route="mfma1", width=2, src=1, nc=32))
    cases.append(_case("fused32-max-ncb", 2176, 4, 32, route="mfma1", width=2, src=0, nc=32))
    # 16 columns: one-chunk items that evaluate K* up to 28 column blocks, the run kernel beyond (the only large cases)
    cases.append(_case("fused16-max-ncb", 7168, 1, 16, route="mfma1", width=1, src=1, nc=16))
    cases.append(_case("fused16-max-ncb", 7296, 1, 16, route="runs", width=1, src=0, nc=16, reduce_gt=1))
    # the polling finaliser's slot limit: 8 outputs x ncb x 13 doubles <= 1536
    cases.append(_case("st1-slots", 3584, 8, 1, D=5, route="stream1", width=1, src=1, polled=1))
    cases.append(_case("st1-slots", 3840, 8, 1, D=5, route="stream1", width=1, src=1, polled=0))
    # T either side of every width, on the two models the state tests use too
    for Np, n_out in ((1408, 4), (2944, 4)):
        for T in (1, 2, 4, 5, 16, 17, 32, 33, 64, 65):
            cases.append(_case("width-edge", Np, n_out, T))
    # -- K0 and its two exclusions
    for Np in (128, 256, 384, 512):
        for T in (1, 2, 16, 17, 128, 129, 1024, 1025):
            cases.append(_case("K0-edge", Np, 2, T))
    # -- K2s: T = 16 sr_var_small_groups_max and one more
    for Np, T in ((2048, 128), (2560, 80), (640, 1024)):
        cases.append(_case("K2s-max", Np, 2, T, route="K2s"))
        cases.append(_case("K2s-max", Np, 2, T + 1, route="K2b"))
    # -- K2b: below 256 cells, 256 and 512 workgroups, nrb > 2, wgs <= 1024
    cases.append(_case("K2b-cells", 384, 2, 1100, route="K2b", bal_wgs=108))
    cases.append(_case("K2b-256", 2048, 2, 3840, route="K2b", bal_wgs=256))
    cases.append(_case("K2b-512", 2048, 2, 4096, route="K2b", bal_wgs=512))
    cases.append(_case("K2b-wgs", 2048, 4, 2048, route="K2b"))
    cases.append(_case("K2b-wgs", 2048, 4, 2049, route="K2"))
    # -- K2m
    cases.append(_case("K2m", 128, 2, 1100, route="K2m"))
    cases.append(_case("K2m", 256, 2, 1100, route="K2m"))          # (nrb = 2: not K2b)
    cases.append(_case("K2m-wgs", 256, 4, 3968, route="K2m"))
    cases.append(_case("K2m-wgs", 256, 4, 3969, route="K2"))
    # -- final stage: SR_FINAL_WAVE_T and the second clamp of pick_nsplit
    cases.append(_case("final", 256, 2, 4096, route="K2m", final=1))
    cases.append(_case("final", 256, 2, 4097, route="K2m", final=2))
    # -- the k range of the other routes starts at (Np - N) rounded down to 16 too: one shape of each at r in RS
    for form, Np, n_out, T, route in (("K0-r", 256, 2, 17, "K0"), ("K2s-r", 2048, 2, 128, "K2s"), ("K2b-r", 384, 2, 1100, "K2b"),
                                      ("K2m-r", 256, 2, 1100, "K2m"), ("K2-r", 2048, 4, 2049, "K2")):
        for r in RS:
            cases.append(_case(form, Np, n_out, T, r=r, route=route))
    return cases


CASES = _build_cases()
# (form, Np, n_out, T, small_path): set_small_path(0 / 2) on three shapes against the same reference
SMALL_PATH_CASES = [(1408, 4, 33), (256, 2, 17), (2944, 4, 64)]


def case_expected(c, n_cu=N_CU):
    return expected_route(c["Np"], c["T"], c["D"], c["n_out"], c["kern"] != "rbf", n_cu)


def check_target(c, got):
    """the case's declared form against a route record (expected or observed)"""
    for k, v in c["target"].items():
        if k == "reduce_gt":
            assert (got["reduce_items"] > REDUCE_REGS) == bool(v), (c["id"], "reduce", got)
        else:
            assert got[k] == v, (c["id"], k, got)


# ---- the device side ----------------------------------------------------------------------------------------------------
_MODELS = {}
SHARES = {}                     # route -> largest err / bar seen (mu, var, jac)


def _model(seed, N, D, n_out, kern):
    """(gp, prob, ref) of one model; the last two stay (the cases are ordered by model)"""
    from safe_exploration_amd import SimpleGPModel
    key = (seed, N, D, n_out, kern)
    if key not in _MODELS:
        while len(_MODELS) >= 2:
            _MODELS.pop(next(iter(_MODELS)))
        prob, ref = R.cached(*key)
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=[kern] * n_out, hyp=prob.hyp)
        gp.train(prob.Z, prob.Y, opt_hyp=False)
        assert gp._handle.N == N and gp._handle.Np == -(-N // 128) * 128
        _MODELS[key] = (gp, prob, ref)
    return _MODELS[key]


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _predict_raw(gp, X):
    """sr_gp_predict on caller buffers with NaN sentinels behind them; returns mu, var, jac (NumPy)"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    T, n, D = X.shape[0], hd.n_out, hd.D
    x = B.as_dev(X, hd.device)
    bufs = [torch.full((T * n * w + PAD,), float("nan"), dtype=torch.float64, device=hd.device) for w in (1, 1, D)]
    check(lib.sr_gp_predict(hd.h, B.ptr(x), T, B.ptr(bufs[0]), B.ptr(bufs[1]), B.ptr(bufs[2]), B.stream_ptr(hd.device)))
    torch.cuda.synchronize()
    out = [b.cpu().numpy() for b in bufs]
    for o, w in zip(out, (1, 1, D)):
        assert np.all(np.isnan(o[T * n * w:])), "write behind an output buffer"
        assert not np.any(np.isnan(o[:T * n * w])), "output element not written"
    return out[0][:T * n].reshape(T, n), out[1][:T * n].reshape(T, n), out[2][:T * n * D].reshape(T, n, D)


def _check_against_reference(what, gp, prob, ref, T, expect, qseed=0, target=None, chunked=False):
    """one call of T queries: data conditions, route, mu / var / jac under the bars, the same bits twice"""
    X, qc, res = R.queries_for(ref, T, qseed)
    bar_mu, bar_var, bar_jac = R.bars(ref, res)
    Np = gp._handle.Np
    cov = R.data_conditions(ref, res, X, qc, Np, T >= 5)
    mu, var, jac = _predict_raw(gp, X)
    got = gp.last_route()
    if not chunked:
        assert got == expect, (what, "route", got, expect)
    if target is not None:
        check_target(target, got)
    mu2, var2, jac2 = _predict_raw(gp, X)
    share = [float((np.abs(a - res[k]) / b).max()) for a, k, b in ((mu, "mu", bar_mu), (var, "var", bar_var), (jac, "jac", bar_jac))]
    print("%-58s %-8s err/bar mu %.3g var %.3g jac %.3g  (bars %.2g %.2g %.2g; coverage %s)"
          % (what, got["route"], share[0], share[1], share[2], bar_mu.max(), bar_var.max(), bar_jac.max(),
             "-" if cov is None else "%.2g" % cov))
    key = "%s src%d w%d%s%s" % (got["route"], got["src"], got["width"], " MULTI" if got["multi"] else "",
                                " reduce>12" if got["reduce_items"] > REDUCE_REGS else "")
    SHARES[key] = np.maximum(SHARES.get(key, np.zeros(3)), share)
    assert share[1] <= 1.0, (what, "var", share)
    assert share[0] <= 1.0, (what, "mu", share)
    assert share[2] <= 1.0, (what, "jac", share)
    for a, b in ((mu, mu2), (var, var2), (jac, jac2)):
        assert np.array_equal(a, b), (what, "second call differs")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_route_against_reference(c):
    gp, prob, ref = _model(15, c["Np"] - c["r"], c["D"], c["n_out"], c["kern"])
    expect = case_expected(c, _n_cu())
    _check_against_reference(c["id"], gp, prob, ref, c["T"], expect, target=c)


@pytest.mark.gpu
@pytest.mark.parametrize("Np,n_out,T", SMALL_PATH_CASES)
def test_small_path_switch(Np, n_out, T):
    """set_small_path(0): the plain tiles whatever the size; 2: everything but the one-launch pass -- the same reference"""
    gp, prob, ref = _model(15, Np, 3, n_out, "rbf")
    try:
        for sp in (0, 2):
            gp.set_small_path(sp)
            _check_against_reference("small_path=%d Np%d T%d" % (sp, Np, T), gp, prob, ref, T,
                                     expected_route(Np, T, 3, n_out, False, _n_cu(), small_path=sp))
    finally:
        gp.set_small_path(1)


@pytest.mark.gpu
def test_chunked_batch():
    """set_chunk(1000) at T = 2100: three passes (1000, 1000, 100) into one set of outputs; the route is that of the last"""
    gp, prob, ref = _model(15, 1408, 3, 4, "rbf")
    try:
        gp.set_chunk(1000)
        got = _check_against_reference("chunk 1000, T 2100", gp, prob, ref, 2100, None, chunked=True)
        assert got == expected_route(1408, 100, 3, 4, False, _n_cu()), got
    finally:
        gp.set_chunk(65536)                                # (the handle's default)


def _slide_steps(gp):
    from safe_exploration_amd._lib import lib, check
    k = ctypes.c_int(-1)
    check(lib.sr_gp_slide_steps(gp._handle.h, ctypes.byref(k)))
    return k.value


@pytest.mark.gpu
@pytest.mark.parametrize("Np,n_out", [(1408, 4), (2944, 4)])
def test_after_in_place_appends(Np, n_out):
    """one and two in-place one-point appends (the model's buffers become views one / two steps in; U^-1 is then 8 bytes off
    a 16-byte boundary / back on it): the streamed kernels read it as it is, a tile route that meets the odd slide must
    report the unslide; afterwards release_scratch + a refit gives the plain model again"""
    from safe_exploration_amd import SimpleGPModel
    N0 = Np - 17
    prob0, _ = R.cached(15, N0, 3, n_out, "rbf")
    gp = SimpleGPModel(n_out, 2, 1, kern_types=["rbf"] * n_out, hyp=prob0.hyp)
    gp.train(prob0.Z, prob0.Y, opt_hyp=False)
    prob = prob0
    ncu = _n_cu()
    for step in (1, 2):
        x, y, q = prob.new_points(1, step)
        gp.update_model(x, y, opt_hyp=False, replace_old=False)
        prob = prob.grown(x, y, q)
        ref = R.Ref(prob)
        assert gp._handle.N == N0 + step and gp._handle.Np == Np
        assert _slide_steps(gp) == step, "the one-point append did not run in place"
        for T in (1, 16, 64):
            _check_against_reference("slide %d Np%d T%d" % (step, Np, T), gp, prob, ref, T,
                                     expected_route(Np, T, 3, n_out, False, ncu))
            assert _slide_steps(gp) == step
        if step == 2:                                      # an even slide keeps U^-1 on 16 bytes: the tiles read the view
            got = _check_against_reference("slide 2 Np%d T300" % Np, gp, prob, ref, 300,
                                           expected_route(Np, 300, 3, n_out, False, ncu, slide=2))
            assert got["unslid"] == 0 and _slide_steps(gp) == 2
            break
        # 300 queries: a tile route; the odd slide must be reported, and the model is plain afterwards
        got = _check_against_reference("slide 1 Np%d T300" % Np, gp, prob, ref, 300,
                                       expected_route(Np, 300, 3, n_out, False, ncu, slide=1))
        assert got["unslid"] == 1 and _slide_steps(gp) == 0
        # (the forced unslide holds the next one-point appends off the in-place route: a fresh model for the second step)
        gp = SimpleGPModel(n_out, 2, 1, kern_types=["rbf"] * n_out, hyp=prob0.hyp)
        gp.train(prob0.Z, prob0.Y, opt_hyp=False)
        x, y, q = prob0.new_points(1, 1)
        gp.update_model(x, y, opt_hyp=False, replace_old=False)
        assert _slide_steps(gp) == 1
    gp.release_scratch()
    gp.train(prob.Z, prob.Y, opt_hyp=False)
    assert _slide_steps(gp) == 0
    _check_against_reference("refit after release_scratch Np%d T33" % Np, gp, prob, R.Ref(prob), 33,
                             expected_route(Np, 33, 3, n_out, False, ncu))


@pytest.mark.gpu
def test_every_listed_form_was_met():
    """runs last in this file: the shares of the bar per route, and every streamed form of the table seen on the device"""
    for k in sorted(SHARES):
        print("share of the bar  %-34s mu %.3g  var %.3g  jac %.3g" % ((k,) + tuple(SHARES[k])))
    want = {"mfma1 src1 w1", "mfma1 src0 w1", "mfma1 src1 w2", "mfma1 src0 w2", "mfma1 src0 w4", "runs src0 w1",
            "runs src0 w1 reduce>12", "runs src0 w2", "runs src0 w2 reduce>12", "runs src0 w4", "runs src0 w4 reduce>12",
            "runs src0 w4 MULTI", "runs src0 w4 MULTI reduce>12", "stream1 src1 w1", "stream1 src1 w4", "stream1 src0 w1",
            "stream1 src0 w4", "K0 src0 w0", "K2s src0 w0", "K2b src0 w0", "K2m src0 w0", "K2 src0 w0"}
    if len(SHARES) >= 5:                                   # (a run of single cases with -k has nothing to say here)
        assert want <= set(SHARES), sorted(want - set(SHARES))
