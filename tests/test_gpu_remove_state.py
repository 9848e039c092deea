"""The stored model -- U^-1 (`Wt`), alpha, log det, K^-1 -- as sr_gp_remove leaves it, entry by entry against the long-double
reference of tests/_factor_ref.py on the remaining rows (Problem.without), with the branch each removal took asserted
(sr_gp_last_remove), and sr_gp_loo against the reference's cluster blocks.

tests/test_gpu_remove.py compares removals with a refit of the same library at 1e-6 on models of up to 640 rows; tests/
test_gpu_model_state.py stops where the padded size shrinks.  Here every case runs its sequence of in-place appends and removals
through the public entry points and asserts, in this order,
  * the report of sr_gp_last_remove equal to a mirror of remove_one's predicates (RemoveMirror) and to what the case is there for
    (`want`); the host side, tests/test_remove_state_host.py, holds the mirror's constants and every case's claimed loop geometry
    (`claims`: row-norm steps, steps of the longest wavefront of the rows kernel, q mod 4, q mod 256, q first or second of its
    wavefront's pair) against csrc/sr_remove.hip and csrc/sr_common.h, and shows on the reference side that a carry dropped at
    the claimed loop edge misses the reference by 100 bars;
  * the state: the checking of test_gpu_model_state._check_state (cluster entries of U^-1, alpha, log det under the a-priori bars,
    times 1 + a with a = append calls + removed points since the fit; the strict lower triangle, the front padding and the
    identity row the removal leaves exactly 0.0 / 1.0; off-cluster entries under OFF_REL);
  * the host copies of Z and y compacted bit for bit (the handle exports neither: the device's copies are read through the
    posterior passes of the consumer cases and through sr_gp_loo, whose mean is y_j - alpha_j var_j);
  * the same bits from a second model taken through the same sequence.
Cases: the smallest shapes at which each edge exists -- one, two and three steps of the row-norm loop (4 SR_RM_NORM_T = 4096
columns each), the rows kernel at Np = 1152 and 1280 (a half and a full last step of 256 columns) with q at every position mod 4,
at both sides of a 256-column boundary, first and second of a pair, at off0 and at Np - 1, N0 odd and even; the shrinking form;
sources slid by 1 .. 5 in-place appends (both kernel instances, the clean kernel, the cleaned allocation reused); the spare
buffer reused as it lies and after clearing; 1, 2, 4, 9 outputs with a noise variance each; mat52 at D = 6; two DENSE problems
in which every row is transformed.  A case whose in-place append met a grid that did not assemble (another process held the CUs)
skips, as in test_gpu_model_state.
NOT covered: buffers too large to keep as spares (keep_old false needs 16 GiB of factor).
The largest error / bar per case goes to stdout (-s); profiles/r17_remove_state.txt keeps a run."""
import ctypes

import numpy as np
import pytest

import _factor_ref as F
import _posterior_ref as R
import test_gpu_model_state as G

pytestmark = pytest.mark.gpu

SEED = 13
NB = G.NB
# ---- restated from csrc/sr_remove.hip (tests/test_remove_state_host.py parses the source and compares) ------------------------
SR_RM_CHUNK, SR_RM_ROWS, SR_RM_WAVES, SR_RM_NORM_T = 256, 2, 4, 1024
NORM_STEP = 4 * SR_RM_NORM_T                                # columns per step of the row-norm loop


def geometry(N0, Np0, j):
    """(row-norm steps, steps of the rows kernel's longest wavefront, q mod 4, q mod 256, q first / second of its pair) of the
    removal of training row j from a model of N0 rows: the loop bounds of csrc/sr_remove.hip, restated"""
    off0 = Np0 - N0
    q = j + off0
    i0 = off0                                               # the first wavefront's first row: the longest walk
    return (-(-(Np0 - q) // NORM_STEP), -(-(Np0 - i0 // SR_RM_CHUNK * SR_RM_CHUNK) // SR_RM_CHUNK), q % 4, q % SR_RM_CHUNK,
            "first" if (q - off0) % SR_RM_ROWS == 0 else "second")


class RemoveMirror(object):
    """the handle's state remove_one decides by (sr_capi_remove.hip), restated on top of test_gpu_model_state.AppendMirror: the
    front padding of the factor the spare buffer last held (None: no spare buffer), the padded size of the spare vectors, the
    points retired since the fit"""

    def __init__(self, N, n_out):
        self.am = G.AppendMirror(N, n_out)
        self.alt_off, self.vec_np, self.count = None, 0, 0

    def append1(self, gave_up=False):
        am = self.am
        Np0, off0 = am.Np, am.Np - am.N
        rep, _ = am.append(1, gave_up)
        if not rep["in_place"]:
            self.alt_off, self.vec_np = (off0, Np0) if rep["Np1"] == Np0 else (None, 0)
        return rep

    def remove(self, j):
        """-> the report expected of sr_gp_last_remove after training row j has gone"""
        am = self.am
        N0, Np0, slide0 = am.N, am.Np, am.slide
        assert 0 <= j < N0
        off0, Np1 = Np0 - N0, -(-(N0 - 1) // NB) * NB
        same = Np1 == Np0
        reuse = same and self.alt_off is not None
        self.count += 1
        rep = dict(count=self.count, Np0=Np0, Np1=Np1, off0=off0, q=j + off0, slide=slide0,
                   aligned=int(slide0 * (Np0 + 1) % 4 == 0),                       # (the view starts slide (Np + 1) doubles in)
                   spare="none" if not reuse else ("cleared" if self.alt_off < off0 else "as_is"),
                   vec_spare=int(same and self.vec_np == Np1), clean=int(slide0 > 0 and same), kept_old=int(same))
        self.alt_off, self.vec_np = (off0 + slide0, Np0) if same else (None, 0)
        am.alt = same
        am.N, am.Np, am.slide = N0 - 1, Np1, 0
        return rep


# ---- the cases ---------------------------------------------------------------------------------------------------------
APP, WIN = ("app",), ("win",)


def rm(*rows):
    return ("rm", list(rows))


def _c(cid, N0, ops, claims, want=None, n_out=2, kern="rbf", D=3, vary_noise=False, dense=False, consumers=False):
    """ops: APP one in-place append, rm(rows) one sr_gp_remove call (negative: from the end), WIN one round of
    update_model(n_max=N0): append one, retire the oldest.  claims: geometry() of the case's FIRST removed point, by hand.
    want: per removing op the words of the report the case is there for"""
    return dict(id="%s-%s-D%d-n%d-N%d" % (cid, kern, D, n_out, N0), N0=N0, ops=ops, claims=claims, want=want or [], n_out=n_out,
                kern=kern, D=D, vary_noise=vary_noise, dense=dense, consumers=consumers)


def _cases():
    c = [
        # row-norm steps: 4097 columns (a second step of one column), exactly 4096, 4224, three steps, two steps from a slid view
        _c("norm/4097", 4224, [rm(127)], (2, 17, 3, 127, "second")),
        _c("norm/4096", 4224, [rm(128)], (1, 17, 0, 128, "first")),
        _c("norm/4224", 4224, [rm(0)], (2, 17, 0, 0, "first"), consumers=True),
        _c("norm/8320", 8320, [rm(0)], (3, 33, 0, 0, "first"), n_out=1),
        _c("norm/slid", 4200, [APP, rm(0)], (2, 17, 3, 23, "first"), [dict(aligned=0, slide=1, clean=1)]),
    ]
    # the rows kernel at Np = 1152 (off 52: the last step is half a chunk) and 1280 (off 0: a full one; the identity row is row 0)
    for j, g in ((0, (1, 5, 0, 52, "first")), (1, (1, 5, 1, 53, "second")), (2, (1, 5, 2, 54, "first")), (3, (1, 5, 3, 55, "second")),
                 (203, (1, 5, 3, 255, "second")), (204, (1, 5, 0, 0, "first")), (1099, (1, 5, 3, 127, "second"))):
        c.append(_c("rows/j%d" % j, 1100, [rm(j)], g, [dict(Np0=1152, off0=52, spare="none", aligned=1)]))
    for j, g in ((1100, (1, 5, 3, 127, "first")), (550, (1, 5, 1, 89, "first"))):          # N0 odd: a dead second row in the last pair
        c.append(_c("rows/j%d" % j, 1101, [rm(j)], g, [dict(off0=51)]))
    for j, g in ((0, (1, 5, 0, 0, "first")), (255, (1, 5, 3, 255, "second")), (256, (1, 5, 0, 0, "first")),
                 (1279, (1, 5, 3, 255, "second")), (641, (1, 5, 1, 129, "second")), (770, (1, 5, 2, 2, "first"))):
        c.append(_c("rows/j%d" % j, 1280, [rm(j)], g, [dict(Np0=1280, off0=0)]))
    # the shrinking form (sh = 128): the destination drops the 128 front rows
    for j, g in ((0, (1, 5, 3, 127, "first")), (576, (1, 5, 3, 191, "first")), (1152, (1, 5, 3, 255, "first"))):
        c.append(_c("shrink/j%d" % j, 1153, [rm(j)], g, [dict(Np0=1280, Np1=1152, spare="none", kept_old=0)]))
    c.append(_c("shrink/ten", 1158, [rm(3, 1157, 100, 101, 102, 7, 600, 64, 128, 255)], (1, 5, 3, 255, "second"),
                [dict(Np0=1152, Np1=1152, count=10, q=6)]))
    c.append(_c("shrink/4225", 4225, [rm(2000)], (1, 17, 3, 79, "first"), [dict(Np0=4352, Np1=4224)], n_out=1))
    # sources slid by s in-place appends: the 8-byte instance unless s is a multiple of 4, the clean kernel, and the next removal
    # into the cleaned allocation as it lies
    for s in (1, 2, 3, 4, 5):
        c.append(_c("slid/%d" % s, 1100, [APP] * s + [rm(0), rm(550)], (1, 5, (52 - s) % 4, 52 - s, "first"),
                    [dict(slide=s, aligned=int(s == 4), clean=1, kept_old=1), dict(slide=0, aligned=1, spare="as_is", clean=0)]))
    c.append(_c("slid/mid", 1100, [APP] * 3 + [rm(555), rm(0)], (1, 5, 0, 92, "second"),
                [dict(slide=3, aligned=0, clean=1), dict(spare="as_is")], consumers=True))
    # the spare factor buffer: three removals in a row (the padding grows past the spare's: cleared), six rounds of the sliding
    # window (the cleaned allocation has a padding row more than the view: as it lies)
    c.append(_c("spare/three", 1100, [rm(10), rm(500), rm(-1)], (1, 5, 2, 62, "first"),
                [dict(spare="none", vec_spare=0), dict(spare="cleared", vec_spare=1), dict(spare="cleared", vec_spare=1)]))
    c.append(_c("spare/window", 1100, [WIN] * 6, (1, 5, 3, 51, "first"),
                [dict(spare="none", slide=1, aligned=0, clean=1)] + [dict(spare="as_is", slide=1, aligned=0, clean=1)] * 5))
    # outputs (each with a noise variance of its own: a table read at another output's stride fails) and the general kernel family
    for n in (1, 2, 4, 9):
        c.append(_c("outputs", 1100, [rm(301)], (1, 5, 1, 97, "second"), n_out=n, vary_noise=True))
    c.append(_c("mat52", 1100, [rm(301)], (1, 5, 1, 97, "second"), kern="mat52", D=6))
    # dense data: every row is transformed; 513 -> 512 crosses 640 -> 512
    c.append(_c("dense/shrink", 513, [rm(256)], (1, 3, 3, 127, "first"), [dict(Np0=640, Np1=512)], dense=True))
    # (540, not 600, rows: the long-double reference of 600 takes more than 5 s on one core)
    c.append(_c("dense/stay", 540, [rm(0)], (1, 3, 0, 100, "first"), [dict(Np0=640, Np1=640)], dense=True))
    return c


CASES = _cases()
LOO_CASES = [(1100, 2, 0), (1100, 2, 3), (4224, 2, 0), (1100, 9, 0)]       # (N0, outputs, in-place appends before)


def problem_of(c):
    if c["dense"]:
        return F.dense_problem(SEED, c["N0"], c["D"], c["n_out"], c["kern"])
    prob = F.problem(SEED, c["N0"], c["D"], c["n_out"], c["kern"])
    return F.noise_per_output(prob) if c["vary_noise"] else prob


def resolve(rows, N):
    return [r if r >= 0 else N + r for r in rows]


def walk(c, prob, on_append=None, on_remove=None):
    """the case's sequence on the reference side: the mirror's report for every point removed and the problem after every
    removing op.  on_append(x, y, window) / on_remove(rows) drive a model beside it.  Yields (op index, problem, a, reports of the
    op's removals) after every removing op; a = append calls + removed points so far"""
    mirror = RemoveMirror(c["N0"], c["n_out"])
    a = n_app = 0
    for k, op in enumerate(c["ops"]):
        rows = None
        if op[0] in ("app", "win"):
            n_app += 1
            x, y, qn = prob.new_points(1, n_app)
            rep = mirror.append1()
            assert rep["in_place"] == 1 and rep["route"] == "grid", (c["id"], k, rep)
            if on_append:
                on_append(x, y, op[0] == "win", rep)
            prob = prob.grown(x, y, qn)
            a += 1
            rows = [0] if op[0] == "win" else None
        if op[0] == "rm":
            rows = resolve(op[1], prob.N)
            if on_remove:
                on_remove(rows)
        if rows is not None:
            reps = [mirror.remove(j) for j in sorted(rows, reverse=True)]      # (the library retires in descending order)
            prob = prob.without(rows)
            a += len(rows)
            yield k, prob, a, reps


def first_removal(c):
    """(N0, Np0, j) of the case's first removed point"""
    n = c["N0"]
    for op in c["ops"]:
        if op[0] == "app":
            n += 1
        elif op[0] == "win":
            return n + 1, -(-(n + 1) // NB) * NB, 0
        else:
            return n, -(-n // NB) * NB, max(resolve(op[1], n))


# ---- the device side -----------------------------------------------------------------------------------------------------
RATIOS = {}


def _adopt(ref, old):
    """blocks of `old` whose cluster holds the same rows: a removal or an append touches one cluster"""
    if old is None or old.p.n_out != ref.p.n_out:
        return ref
    for q, i in enumerate(ref.idx):
        j = old.idx[q]
        if len(i) == len(j) and np.array_equal(ref.p.Z[i], old.p.Z[j]) and np.array_equal(ref.p.Y[i], old.p.Y[j]):
            for d in range(ref.p.n_out):
                if (q, d) in old._blk:
                    ref._blk[q, d] = old._blk[q, d]
    return ref


class _GridGaveUp(Exception):
    pass


def _drive(c, prob0, checked):
    """one model through the case's sequence; checked: assert the report and the state after every removing op.  Returns
    (gp, final problem, final reference or None, a)"""
    gp = G._train(prob0)
    gp.append_limit = 10 ** 9
    N0 = c["N0"]

    def on_append(x, y, window, rep):
        before = G._grid_aborts(gp)
        if window:
            gp.update_model(x, y, opt_hyp=False, replace_old=False, n_max=N0, retire="oldest")
        else:
            gp.update_model(x, y, opt_hyp=False, replace_old=False)
        if G._grid_aborts(gp) > before:
            raise _GridGaveUp()
        if checked:
            assert gp.last_update() == rep, (c["id"], gp.last_update(), rep)
            if not window:
                assert G._slide_steps(gp) == rep["in_place"] + on_append.slide
        on_append.slide = 0 if window else on_append.slide + 1

    on_append.slide = 0

    def on_remove(rows):
        if c["consumers"] and checked:
            gp.inv_K                                        # (fills the cache a removal must drop)
        gp.remove_data(rows)
        on_append.slide = 0

    ref, prob, a, n_rm = None, prob0, 0, 0
    for k, prob, a, reps in walk(c, prob0, on_append, on_remove):
        if not checked:
            continue
        what = "%s op %d" % (c["id"], k)
        got = gp.last_remove()
        assert got == reps[-1], (what, "route", got, reps[-1])
        if n_rm < len(c["want"]):
            assert {key: got[key] for key in c["want"][n_rm]} == c["want"][n_rm], (what, "route", got, c["want"][n_rm])
        n_rm += 1
        assert G._slide_steps(gp) == 0, what
        ref = _adopt(F.FactorRef(prob, appends=a), ref)
        G._data_conditions(ref, reps[-1]["Np1"])
        G._check_state(what, gp, ref)
        RATIOS[what] = dict(G.RATIOS.pop(what))
        mu, var = gp.loo()                                  # (mu_loo = y_j - alpha_j var_j reads the device's compacted targets)
        for d in range(prob.n_out):
            rmu, rvar, bmu, bvar = ref.loo(d)
            RATIOS[what]["loo_mu"] = max(RATIOS[what].get("loo_mu", 0.0), float((np.abs(mu[:, d] - rmu) / bmu).max()))
            RATIOS[what]["loo_var"] = max(RATIOS[what].get("loo_var", 0.0), float((np.abs(var[:, d] - rvar) / bvar).max()))
        print("%-44s err/bar mu_loo %.3g var_loo %.3g" % ("", RATIOS[what]["loo_mu"], RATIOS[what]["loo_var"]))
        assert RATIOS[what]["loo_var"] <= 1.0 and RATIOS[what]["loo_mu"] <= 1.0, (what, "leave-one-out", RATIOS[what])
        for host in (gp.x_train, gp.z):
            assert np.array_equal(host, prob.Z), (what, "Z not compacted")
        assert np.array_equal(gp.y_train, prob.Y), (what, "y not compacted")
    return gp, prob, ref, a


def _consumers(c, gp, prob, ref):
    """K^-1 (a stale cached inverse fails) and two posterior passes on the model the case left"""
    from test_gpu_posterior_routes import _predict_raw
    worst = dict(cluster=0.0, off=0.0)
    for d, k in enumerate(gp.inv_K):
        r = ref.check_inv_k(d, k)
        worst = {key: max(worst[key], r[key]) for key in worst}
    print("%-44s err/bar K^-1 %.3g  off-cluster %.3g" % (c["id"], worst["cluster"], worst["off"]))
    RATIOS[c["id"] + " K^-1"] = dict(kinv=worst["cluster"])
    assert worst["cluster"] <= 1.0 and worst["off"] <= 1.0, worst
    pref = R.Ref(prob)
    for T in (1, 40):
        X, qc, res = R.queries_for(pref, T, 0)
        bar_mu, bar_var, bar_jac = R.bars(pref, res)
        R.data_conditions(pref, res, X, qc, gp._handle.Np, False)
        mu, var, jac = _predict_raw(gp, X)
        share = dict(mu=float((np.abs(mu - res["mu"]) / bar_mu).max()), var=float((np.abs(var - res["var"]) / bar_var).max()),
                     jac=float((np.abs(jac - res["jac"]) / bar_jac).max()))
        print("%-44s T = %-3d err/bar mu %.3g var %.3g jac %.3g" % (c["id"], T, share["mu"], share["var"], share["jac"]))
        RATIOS["%s T%d" % (c["id"], T)] = share
        assert max(share.values()) <= 1.0, (c["id"], T, share)


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_removal_against_reference(c):
    import torch
    prob0 = problem_of(c)
    try:
        gp, prob, ref, a = _drive(c, prob0, True)
        alpha, wt = gp.export_state()
        if c["consumers"]:
            _consumers(c, gp, prob, ref)
        gp2 = _drive(c, prob0, False)[0]
    except _GridGaveUp:
        pytest.skip("the grid of an in-place append did not assemble (sr_gp_grid_append_aborts advanced)")
    a2, w2 = gp2.export_state()
    torch.cuda.synchronize()
    assert torch.equal(a2, alpha) and torch.equal(w2, wt), (c["id"], "a second model through the same sequence differs")


def _loo_raw(gp, want_mu=True, want_var=True, pad=64):
    """sr_gp_loo on caller buffers with NaN sentinels behind them: (mu, var) as (n_out, N) arrays, None where not asked for"""
    import torch
    from safe_exploration_amd import _buffers as B
    from safe_exploration_amd._lib import lib, check
    hd = gp._handle
    n = hd.n_out * hd.N
    bufs = [torch.full((n + pad,), float("nan"), dtype=torch.float64, device=hd.device) if w else None for w in (want_mu, want_var)]
    check(lib.sr_gp_loo(hd.h, B.ptr(bufs[0]) if want_mu else None, B.ptr(bufs[1]) if want_var else None, B.stream_ptr(hd.device)))
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        if b is None:
            out.append(None)
            continue
        o = b.cpu().numpy()
        assert np.all(np.isnan(o[n:])), "write behind an output buffer"
        assert not np.any(np.isnan(o[:n])), "output element not written"
        out.append(o[:n].reshape(hd.n_out, hd.N))
    return out


@pytest.mark.parametrize("N0,n_out,apps", LOO_CASES)
def test_loo_against_reference(N0, n_out, apps):
    """both outputs of sr_gp_loo under the propagated bars of _factor_ref (LEAVE-ONE-OUT), on a plain model and on the slid view
    of in-place appends, which is read where it lies; sentinels behind both buffers; either pointer NULL gives the other's bits"""
    c = _c("loo", N0, [APP] * apps, None, n_out=n_out, vary_noise=n_out == 9)
    prob = problem_of(c)
    gp = G._train(prob)
    gp.append_limit = 10 ** 9
    for k in range(apps):
        x, y, qn = prob.new_points(1, k + 1)
        before = G._grid_aborts(gp)
        gp.update_model(x, y, opt_hyp=False, replace_old=False)
        if G._grid_aborts(gp) > before:
            pytest.skip("the grid of an in-place append did not assemble (sr_gp_grid_append_aborts advanced)")
        prob = prob.grown(x, y, qn)
    assert G._slide_steps(gp) == apps
    ref = F.FactorRef(prob, appends=apps)
    mu, var = _loo_raw(gp)
    assert G._slide_steps(gp) == apps, "sr_gp_loo moved the view"
    worst = dict(loo_mu=0.0, loo_var=0.0)
    for d in range(n_out):
        rmu, rvar, bmu, bvar = ref.loo(d)
        worst["loo_mu"] = max(worst["loo_mu"], float((np.abs(mu[d] - rmu) / bmu).max()))
        worst["loo_var"] = max(worst["loo_var"], float((np.abs(var[d] - rvar) / bvar).max()))
    what = "loo N%d n%d +%d" % (N0, n_out, apps)
    print("%-44s err/bar mu_loo %.3g var_loo %.3g" % (what, worst["loo_mu"], worst["loo_var"]))
    RATIOS[what] = worst
    assert worst["loo_var"] <= 1.0 and worst["loo_mu"] <= 1.0, worst
    assert np.array_equal(_loo_raw(gp, want_var=False)[0], mu) and np.array_equal(_loo_raw(gp, want_mu=False)[1], var)
    m2, v2 = gp.loo()
    assert np.array_equal(m2, mu.T) and np.array_equal(v2, var.T)


def test_last_remove_refusals_and_count():
    """a NULL buffer and cap < 1 are refused on a live handle; a short buffer gets its words; the count is 0 before the first
    removal and after a refit, which leaves the other words as they were"""
    from safe_exploration_amd import _lib
    prob = F.problem(SEED, 200, 3, 2)
    gp = G._train(prob)
    h = gp._handle.h
    out = (ctypes.c_int * 11)(*([7] * 11))
    assert _lib.lib.sr_gp_last_remove(h, None, 11) == _lib.SR_EINVAL and _lib.lib.sr_gp_last_remove(h, out, 0) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_remove(h, out, 11) == 11 and list(out) == [0] * 11
    gp.remove_data([5, 17])
    want = RemoveMirror(200, 2)
    want.remove(17)
    rep = want.remove(5)
    assert gp.last_remove() == rep and rep["count"] == 2
    out = (ctypes.c_int * 11)(*([7] * 11))
    assert _lib.lib.sr_gp_last_remove(h, out, 3) == 3 and list(out) == [2, 256, 256] + [7] * 8
    assert _lib.lib.sr_gp_last_remove(h, out, 20) == 11
    rc, info = G._raw_fit(gp, gp._handle, prob.Z[:198], prob.Y[:198], prob.nugget)
    assert rc == 0
    assert gp.last_remove() == dict(rep, count=0)


def test_margins():
    """runs last in this file: the thinnest margin of the run"""
    if not RATIOS:
        return
    keys = ("cluster", "alpha", "logdet", "kinv", "mu", "var", "jac", "loo_mu", "loo_var")
    what, key = max(((w, k) for w in RATIOS for k in keys if k in RATIOS[w]), key=lambda t: RATIOS[t[0]][t[1]])
    print("thinnest margin: %s, %s at %.3g of its bar (%d states compared)" % (what, key, RATIOS[what][key], len(RATIOS)))
