"""CPU side of tests/test_gpu_model_state.py: the block reference of tests/_factor_ref.py against a dense long-double
factorisation, two independent fp64 NumPy routes under a quarter of every bar on every GPU case's data (appends: a refit of the
grown data), the data conditions, the case table against the rules of csrc/sr_common.h and the drivers, and the refusals of
sr_gp_last_update.  Runs without a GPU."""
import ctypes
import os
import re
import time

import numpy as np
import pytest
import scipy.linalg as sla

import _factor_ref as F
import _posterior_ref as R
import test_gpu_model_state as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe_exploration_amd", "csrc")
N_DENSE_MAX = 4000               # dense fp64 routes up to here; cluster by cluster beyond, and one dense case at N = 4000
QUARTER = 0.25


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(src, name):
    m = re.search(r"^#define\s+%s\s+(\w+)\b" % name, src, re.M)
    assert m, "#define %s not found" % name
    return m.group(1)


# ---- the block reference against a dense long-double factorisation -------------------------------------------------------
def test_block_reference_against_dense_long_double():
    """N = 300 (four clusters): U^-1, alpha and log det of the blocks against a long-double Cholesky of the WHOLE matrix, which
    keeps every cross-cluster term: equal to 1e-17 relative (80-bit long double; in proportion where it is wider or narrower)"""
    tol = 1e-17 * float(np.finfo(R.LD).eps) / 2.0 ** -63
    for kern in ("rbf", "mat52"):
        prob, ref = F.cached(G.SEED, 300, 3, 2, kern)
        for d in range(2):
            k, _ = R.kernel_ld(kern, prob.Z, prob.Z, prob.ls[d], prob.sf2[d])
            l = R.cholesky_ld((k + k.T) / 2 + R.LD(prob.nugget[d]) * np.eye(300, dtype=R.LD))
            w = R.solve_lower_ld(l, np.eye(300, dtype=R.LD)).T
            alpha = R.solve_upper_ld(l, R.solve_lower_ld(l, np.asarray(prob.Y[:, d], dtype=R.LD)[:, None]))[:, 0]
            logdet = 2 * np.sum(np.log(np.diag(l)))
            wr = np.zeros((300, 300), dtype=R.LD)
            ar = np.zeros(300, dtype=R.LD)
            for q, i in enumerate(ref.idx):
                wr[np.ix_(i, i)] = ref.block(q, d)["W"]
                ar[i] = ref.block(q, d)["alpha"]
            if kern == "rbf":                              # (mat52: the cross-cluster terms themselves are 4e-32 of the signal)
                assert float(np.abs(w - wr).max() / np.abs(wr).max()) <= tol
                assert float(np.abs(alpha - ar).max() / np.abs(ar).max()) <= tol
            else:
                assert float(np.abs(w - wr).max() / np.abs(wr).max()) <= 1e-24 + tol
                assert float(np.abs(alpha - ar).max() / np.abs(ar).max()) <= 1e-24 + tol
            blocks = sum(R.LD(2) * np.sum(np.log(ref.block(q, d)["piv"])) for q in range(prob.c))     # (long double)
            assert abs(logdet - blocks) <= tol * abs(logdet)
            assert abs(float(logdet) - ref.logdet(d)) <= 2.0 ** -52 * abs(ref.logdet(d))      # (and what logdet() hands out: its float)


# ---- two fp64 routes ---------------------------------------------------------------------------------------------------
def _kernel64(kern, x, z, ls, sf2):
    """fp64 kernel matrix from coordinate differences, as the device kernels form it"""
    r2 = np.zeros((x.shape[0], z.shape[0]))
    for j in range(x.shape[1]):
        diff = (x[:, j, None] - z[None, :, j]) / ls[j]
        r2 += diff * diff
    if kern == "rbf":
        return sf2 * np.exp(-0.5 * r2)
    r = np.sqrt(r2)
    return sf2 * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * np.exp(-np.sqrt(5.0) * r)


def _route_chol(k, y):
    """dense Cholesky plus triangular inverse: (U^-1, alpha, log det, K^-1)"""
    l = np.linalg.cholesky(k)
    w = sla.solve_triangular(l, np.eye(k.shape[0]), lower=True).T
    return w, sla.cho_solve((l, True), y), 2.0 * np.sum(np.log(np.diag(l))), w.dot(w.T)


def _route_inv(k, y):
    """inv(K) followed by its own Cholesky: K^-1 = W W^T with W upper triangular is the reversed Cholesky factor"""
    ki = np.linalg.inv(k)
    ki = (ki + ki.T) / 2
    w = np.linalg.cholesky(ki[::-1, ::-1])[::-1, ::-1]
    return w, ki.dot(y), -2.0 * np.sum(np.log(np.diag(w))), ki


def _routes_share(prob, ref, dense, outputs=None):
    """largest share of a bar (a = 0) either fp64 route takes on prob's data; dense: the N x N matrix, else cluster by cluster"""
    worst = 0.0
    for d in (range(prob.n_out) if outputs is None else outputs):
        for route in (_route_chol, _route_inv):
            if dense:
                k = _kernel64(prob.kern, prob.Z, prob.Z, prob.ls[d], prob.sf2[d]) + prob.nugget[d] * np.eye(prob.N)
                w, alpha, logdet, kinv = route(k, prob.Y[:, d])
                r = ref.check_wt(d, lambda r0, r1: w[r0:r1], prob.N)
                assert r["lower"] == 0.0
                ri = ref.check_inv_k(d, kinv)
                a = max(float(np.abs(alpha[i] - ref.block(q, d)["alpha64"]).max()) / ref.bar_alpha(q, d) for q, i in enumerate(ref.idx))
                worst = max(worst, r["cluster"], r["off"], ri["cluster"], ri["off"], a)
            else:
                logdet = 0.0
                for q, i in enumerate(ref.idx):
                    blk = ref.block(q, d)
                    k = _kernel64(prob.kern, prob.Z[i], prob.Z[i], prob.ls[d], prob.sf2[d]) + prob.nugget[d] * np.eye(len(i))
                    w, alpha, ld, kinv = route(k, prob.Y[i, d])
                    logdet += ld
                    worst = max(worst, float(np.abs(w - blk["W64"]).max()) / ref.bar_w(q, d),
                                float(np.abs(alpha - blk["alpha64"]).max()) / ref.bar_alpha(q, d),
                                float(np.abs(kinv - blk["Kinv64"]).max()) / ref.bar_kinv(q, d))
            worst = max(worst, abs(logdet - ref.logdet(d)) / ref.bar_logdet(d))
    return worst


def _fit_models():
    """(N, D, n_out, kern) of every fit case, the regime-2 case and the breakdown cases (their clean fits), once each"""
    keys = {(c["N"], c["D"], c["n_out"], c["kern"], c["vary_noise"]): c["nb"] for c in G.FIT_CASES + [G.BIG]}
    return sorted(keys.items())


@pytest.mark.parametrize("key,nb", _fit_models(), ids=["N%d-D%d-n%d-%s" % k[:4] for k, _ in _fit_models()])
def test_fit_data_and_fp64_routes(key, nb):
    """on every fit case's data: every tile of U and U^-1 holds an entry above 1e-3 of the largest, up to 17 blocks every term
    of the trailing updates moves its tile by 1e-6 at least, and both fp64 routes stay under a quarter of every bar"""
    prob, ref = F.cached(G.SEED, *key)
    if key[4]:                                             # every output its own noise, and hyp and nugget agree about it
        assert len(set(prob.nugget)) == prob.n_out
        assert [h["noise_variance"] + R.NOISE_DIAG + R.GPY_JITTER for h in F.hyp_of(prob)] == list(prob.nugget)
    assert np.all(np.bincount(prob.member, minlength=prob.c) <= R.CLUSTER)
    for d in range(prob.n_out):
        ref.tile_conditions(d, G.NB * nb)
        if nb <= 17:
            ref.update_terms(d, G.NB * nb)
    share = _routes_share(prob, ref, prob.N <= N_DENSE_MAX)
    assert share <= QUARTER, share


def test_fp64_routes_dense_at_4000():
    prob, ref = F.cached(G.SEED, 4000, 3, 1, "rbf")
    share = _routes_share(prob, ref, True)
    assert share <= QUARTER, share


@pytest.mark.parametrize("c", G.APPEND_CASES, ids=[c["id"] for c in G.APPEND_CASES])
def test_append_data_and_fp64_routes(c):
    """after every step of every append sequence: the data conditions on the grown problem, and a refit of the grown data by
    both fp64 routes under a quarter of the bars of a fit (the device gets 1 + a of them)"""
    prob = F.problem(G.SEED, c["N0"], c["D"], c["n_out"], c["kern"])
    mirror = G.AppendMirror(c["N0"], c["n_out"], c["small_path"])
    for a, m in enumerate(c["steps"], 1):
        x, y, q = prob.new_points(m, a)
        mirror.append(m, a <= c["give_up"])
        prob = prob.grown(x, y, q)
        assert prob.N == mirror.N
        ref = F.FactorRef(prob)
        for d in range(prob.n_out):
            ref.tile_conditions(d, mirror.Np)
            if mirror.Np <= 17 * G.NB:
                ref.update_terms(d, mirror.Np)
        assert F.FactorRef(prob, appends=a).bar_w(0, 0) == pytest.approx((1 + a) * ref.bar_w(0, 0), rel=1e-14)
    share = _routes_share(prob, ref, prob.N <= N_DENSE_MAX)     # (the last step: the earlier ones are its leading rows)
    assert share <= QUARTER, share


def test_reference_build_time_of_the_largest_case():
    c = G.BIG
    t0 = time.perf_counter()
    prob = F.problem(G.SEED, c["N"], c["D"], c["n_out"], c["kern"])
    ref = F.FactorRef(prob)
    for q in range(prob.c):
        ref.block(q, 0)
    dt = time.perf_counter() - t0
    assert prob.c == 184 and dt < 5.0, dt


# ---- the case table against the sources -------------------------------------------------------------------------------
def test_thresholds_mirrored():
    common, update, append = _read("sr_common.h"), _read("sr_capi_update.hip"), _read("sr_capi_append.hip")
    for name in ("SR_FACT_ONE_STREAM_MAX_NB", "SR_FACT_CHAIN_MAX_NB", "SR_FACT_SLOTS", "SR_APPEND1_MAX_NP0", "SR_APPEND1G_MAX_NP0",
                 "SR_SMALL_T"):
        assert getattr(G, name) == int(_define(common, name)), name
    assert _define(common, "SR_SLIDE_STEPS") == "SR_NB" and int(_define(common, "SR_NB")) == G.NB == G.SR_SLIDE_STEPS
    assert int(_define(common, "SR_APPEND1_MAX_OUT")) == G.SR_APPEND1_MAX_OUT
    def body(name):
        m = re.search(r"static\s+inline\s+int\s+%s\s*\([^)]*\)\s*\{(.*?)\}" % name, common, re.S)
        assert m, name
        return [int(v) for v in re.findall(r"\b\d+\b", m.group(1))]
    # the numbers of the two tables in the order they stand in; the mirrors' values at both sides of every step
    assert body("sr_fact_panel") == [28, 2, 44, 3, 64, 4, 200, 8, 24]
    assert [G.fact_panel(nb) for nb in (1, 28, 29, 44, 45, 64, 65, 200, 201)] == [2, 2, 3, 3, 4, 4, 8, 8, 24]
    assert body("sr_fact_reserved_cus") == [2, 8, 36, 52, 64, 32]
    assert [G.fact_reserved_cus(1, nb) for nb in (36, 37, 52, 53)] == [32, 64, 64, 32] and G.fact_reserved_cus(2, 129) == 8
    assert int(_define(common, "SR_FLOW_MIN_NB")) > int(_define(common, "SR_FLOW_MAX_NB")), "the tile flow has become a default"
    # the predicates expected_fit and inv_stages restate
    # (patterns, not lines: the names and numbers a predicate rests on, whatever stands around them)
    def has(src, pattern):
        return re.search(re.sub(r" ", r"\\s*", pattern), src) is not None
    assert has(update, r"regime = nb <= SR_FACT_CHAIN_MAX_NB \? 1 : 2")
    assert has(update, r"own_streams =[^;]*nb <= 2 && P >= nb[^;]*nb <= one_stream_nb")
    assert has(update, r"one_stream_nb =[^;]*SR_FACT_ONE_STREAM_MAX_NB")
    assert has(update, r"early_inv =[^;]*nb >= %d\b" % G.EARLY_INV_MIN_NB)
    assert has(update, r"inv_min_rest =[^;]*nb <= %d \? %d : 1000" % (G.STAGED_INV_MAX_NB, G.STAGED_INV_MIN_REST))
    assert has(update, r"min\(h->n_out, SR_FACT_SLOTS\)")
    # ... and those of AppendMirror
    assert has(append, r"h->Np <= SR_APPEND1_MAX_NP0 && Np1 <= SR_APPEND1_MAX_NP0 \+ SR_NB\) return 1")
    assert has(append, r"h->Np <= SR_APPEND1G_MAX_NP0 && h->n_out <= SR_APPEND1_MAX_OUT")
    assert has(append, r"if \(m <= SR_SMALL_T\) return append_small")
    assert has(append, r"np1 == h->Np && h->slack_ok && h->slide < SR_SLIDE_STEPS - 1") and has(append, r"h->N \+ 1 <= h->z_cap")
    assert has(append, r"grid_hold = 16 << std::min\(h->grid_aborts_row, 10\)")
    assert has(append, r"APP_KS = 512\b")


def test_every_fit_case_sits_on_its_edge():
    """each block count of FIT_NB is the last or the first size of the rule it names: the neighbour on the other side differs"""
    rule = {
        "one-block": lambda nb: (nb <= 1,),                                 # no block row to solve, no trailing update
        "two-blocks": lambda nb: (nb <= 2,),                                # (nb <= 2 && P >= nb: no look-ahead, no bulk update)
        "inv-tree": lambda nb: ((nb & (nb - 1)) == 0,),                     # a power of two: a balanced halving tree, one more is not
        "early-inv": lambda nb: (nb >= G.EARLY_INV_MIN_NB,),
        "one-stream": lambda nb: (G.expected_fit(nb, 2)["own_streams"],),
        "staged-inv": lambda nb: (G.inv_stages(nb, G.fact_panel(nb), True, 1) > 1,),
        "panel": lambda nb: (G.fact_panel(nb),),
        "reserved": lambda nb: (G.fact_reserved_cus(1, nb),),
        "regime": lambda nb: (G.expected_fit(nb, 1)["regime"],),
    }
    for nb, edge in G.FIT_NB + [(G.BIG["nb"], G.BIG["edge"])]:
        f = rule[edge]
        assert f(nb) != f(nb - 1) or f(nb) != f(nb + 1), (nb, edge)
    nbs = [nb for nb, _ in G.FIT_NB]
    for lo in (2, 15, 16, 24, 28, 36, 44, 52, 64):                          # both sides of every rule are cases
        assert lo in nbs and lo + 1 in nbs, lo
    assert G.expected_fit(15, 2)["own_streams"] == 0 and G.expected_fit(16, 2)["own_streams"] == 1
    assert G.expected_fit(16, 2)["inv_stages"] == 2 and G.expected_fit(24, 2)["inv_stages"] >= 2 and G.expected_fit(25, 2)["inv_stages"] == 1
    assert G.expected_fit(128, 1)["regime"] == 1 and G.expected_fit(129, 1)["regime"] == 2 and G.expected_fit(129, 1)["inv_stages"] == 0
    assert G.expected_fit(3, 9)["rounds"] == 2 and G.expected_fit(3, 8)["rounds"] == 1
    assert all(c["N"] == G.NB * c["nb"] - 37 for c in G.FIT_CASES if c["id"].startswith("edge"))
    assert {(c["nb"], c["N"]) for c in G.FIT_CASES if c["id"].startswith("pad")} == \
        {(nb, G.NB * nb - r) for nb in (1, 3, 16) for r in (0, 127)}
    assert [c["panel"] for c in G.FIT_CASES if c["panel"]] == [1, 3, 5, 64, 4]
    assert G.BIG["N"] == 16500 and all(c["n_out"] == (2 if c["nb"] < 44 else 1) for c in G.FIT_CASES if c["id"].startswith("edge"))
    for nb, n_out in G.BREAKDOWN:
        rows = G.breakdown_rows(nb)
        off = 37
        assert [(r + off) // G.NB for r in rows[:4]] == [0, 0, 1, 2] and (rows[2] + off) % G.NB == 0 and rows[4] == G.NB * nb - 38


def test_every_append_case_takes_its_route():
    """AppendMirror on every sequence: the route each case names, in place where the issue says so, the spare buffer on the
    second append of an unchanged padded size, the edges of the two one-launch routes"""
    seen = {}
    for c in G.APPEND_CASES:
        m = G.AppendMirror(c["N0"], c["n_out"], c["small_path"])
        reps = [m.append(k, a <= c["give_up"])[0] for a, k in enumerate(c["steps"], 1)]
        seen[c["id"]] = reps
        if c["route"] != "mixed":
            assert all(r["route"] == c["route"] for r in reps), (c["id"], reps)
    def rep(cid):
        return seen[next(k for k in seen if k.startswith(cid))]
    assert [r["Np1"] for r in rep("one_wg-rbf-n2-N127")] == [128] and [r["Np1"] for r in rep("one_wg-rbf-n2-N128")] == [256]
    assert [(r["Np0"], r["Np1"]) for r in rep("one_wg-rbf-n2-N511")] == [(512, 512), (512, 640)]
    assert [r["in_place"] for r in rep("grid-rbf-n2-N600")] == [1, 1, 1]
    assert [(r["in_place"], r["Np1"]) for r in rep("grid-rbf-n2-N640")] == [(0, 768)]
    assert [(r["in_place"], r["Np1"]) for r in rep("grid-rbf-n2-N1151")] == [(1, 1152), (0, 1280)]
    assert [(r["route"], r["Np0"]) for r in rep("grid-rbf-n1-N8100")] == [("grid", 8192)]
    assert [(r["route"], r["Np0"]) for r in rep("small/np0")] == [("small", 8320)]
    assert [r["spare"] for r in rep("tile-rbf-n2-N600+20+19")] == [0, 1]
    assert [(r["Np0"], r["Np1"]) for r in rep("tile-rbf-n2-N630")] == [(640, 768)]
    assert [(r["route"], r["in_place"], r["Np1"]) for r in rep("mixed")] == \
        [("grid", 1, 1152), ("small", 0, 1152), ("tile", 0, 1280), ("grid", 0, 1280)]
    assert G.AppendMirror(8192, 1).append(1)[0]["route"] == "grid" and G.AppendMirror(8193, 1).append(1)[0]["route"] == "small"
    assert [(r["route"], r["in_place"], r["spare"]) for r in rep("small/gave_up")] == [("small", 0, 0), ("small", 0, 1)]
    held = G.AppendMirror(600, 2)
    assert [held.append(1, a == 0)[0]["route"] for a in range(17)] == ["small"] * 16 + ["grid"]      # (it rests for 16 appends)
    assert G.AppendMirror(513, 2).append(1)[0]["route"] == "grid" and G.AppendMirror(600, 2).append(16)[0]["route"] == "small"
    assert G.AppendMirror(600, 2).append(17)[0]["route"] == "tile"
    # a K slice of the tile route is 512 rows: Np0 = 640 is one full slice and a cut one, 1024 two full ones, 128 a cut one alone
    assert sorted({-(-c["N0"] // G.NB) * G.NB for c in G.APPEND_CASES if c["id"].startswith("tile-rbf-n2") and len(c["steps"]) == 1
                   and c["steps"][0] in (17, 50, 128)}) == [128, 640, 1024]


def test_last_update_symbol_and_refusals(lib_built):
    """the symbol, its words against the Python names, and the refusal of NULL arguments.  A handle cannot be made without a
    device (sr_gp_create selects it), so the refusal of cap < 1 and of a NULL buffer on a LIVE handle, and the short buffer, are
    in tests/test_gpu_model_state.py::test_last_update_refusals"""
    from safe_exploration_amd import _lib
    from safe_exploration_amd.ssm_hip.gaussian_process import SimpleGPModel
    assert hasattr(_lib.lib, "sr_gp_last_update") and "sr_gp_last_update" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        header = f.read()
    assert int(re.search(r"#define SR_UPDATE_WORDS (\d+)", header).group(1)) == len(SimpleGPModel.UPDATE_FIT_WORDS)
    words = re.search(r"enum \{ SR_UPD_KIND = 0,([^}]*)\}", header).group(1)
    assert ["kind"] + [s.strip()[len("SR_UPD_"):].lower() for s in words.split(",")] == \
        [w.lower() for w in SimpleGPModel.UPDATE_FIT_WORDS[:5]] + ["npar", "rounds", "inv_stages", "form"]
    words = re.search(r"enum \{ SR_UPD_ROUTE = 1,([^}]*)\}", header).group(1)
    assert ["kind", "route"] + [s.strip()[len("SR_UPD_"):].lower() for s in words.split(",")] == \
        [w.lower() for w in SimpleGPModel.UPDATE_APPEND_WORDS]
    names = re.search(r"enum \{ SR_UPD_SMALL = 0,([^}]*)\}", header).group(1)
    assert ["small"] + [s.strip()[len("SR_UPD_"):].lower() for s in names.split(",")] == list(SimpleGPModel.UPDATE_ROUTES)
    out = (ctypes.c_int * 9)()
    assert _lib.lib.sr_gp_last_update(None, out, 9) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_update(None, None, 9) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_update(None, out, 0) == _lib.SR_EINVAL
