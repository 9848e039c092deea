"""CPU side of tests/test_gpu_posterior_routes.py: the long-double reference of tests/_posterior_ref.py against two independent
fp64 routes and against a dense long-double evaluation, the data conditions on every case's data, the case table against the
library's own streamed planner at 256 compute units, the restated thresholds against csrc/sr_common.h, and the two new
diagnostics of the C ABI.  Runs without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import _posterior_ref as R
import test_gpu_posterior_routes as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe_exploration_amd", "csrc")
N_HOST_MAX = 3000                # dense fp64 fits beyond this take too long for a CPU test


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(src, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
    assert m, "#define %s not found" % name
    return int(m.group(1))


# ---- two fp64 routes on the DENSE matrix ---------------------------------------------------------------------------------
def _kernel64(kern, x, z, ls, sf2):
    """fp64 k and g = kappa'(r) / r from coordinate DIFFERENCES, as the device kernels form them.  (oracle_np's
    unscaled_dist_sq expands |x - z|^2 = |x|^2 - 2 x.z + |z|^2: with cluster centres a few hundred lengthscales from the origin
    that cancellation alone costs 1e-11 relative in k, five hundred times the error of either algebraic route below.)"""
    r2 = np.zeros((x.shape[0], z.shape[0]))
    for j in range(x.shape[1]):                       # (one dimension at a time: no N x N x D temporary)
        diff = (x[:, j, None] - z[None, :, j]) / ls[j]
        r2 += diff * diff
    if kern == "rbf":
        k = sf2 * np.exp(-0.5 * r2)
        return k, -k
    r = np.sqrt(r2)
    e = sf2 * np.exp(-np.sqrt(5.0) * r)
    return (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * e, -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * e


_DENSE = {}


def _dense_fit(prob):
    """the algebra of oracle_np.gp_fit (Cholesky, explicit inverse L^-T L^-1 as GPy's pdinv, alpha by cho_solve) on the
    dense N x N matrix of every output; the last fit is kept"""
    key = (prob.seed, prob.N, prob.D, prob.n_out, prob.kern)
    if key not in _DENSE:
        _DENSE.clear()
        fit = []
        for d in range(prob.n_out):
            k, _ = _kernel64(prob.kern, prob.Z, prob.Z, prob.ls[d], prob.sf2[d])
            l = sla.cholesky(k + prob.nugget[d] * np.eye(prob.N), lower=True)
            ki, info = sla.lapack.dpotri(l, lower=1)                  # (what GPy's pdinv calls; the lower triangle)
            assert info == 0
            ki = np.tril(ki) + np.tril(ki, -1).T
            fit.append((l, ki, sla.cho_solve((l, True), prob.Y[:, d])))
        _DENSE[key] = fit
    return _DENSE[key]


def _dense_predict(prob, X):
    """(mu, jac, var by the explicit inverse, var by the triangular solve)"""
    T, n, D = X.shape[0], prob.n_out, prob.D
    mu, vi, vc, jac = np.empty((T, n)), np.empty((T, n)), np.empty((T, n)), np.empty((T, n, D))
    for d, (l, ki, alpha) in enumerate(_dense_fit(prob)):
        k, g = _kernel64(prob.kern, X, prob.Z, prob.ls[d], prob.sf2[d])
        mu[:, d] = k.dot(alpha)
        vi[:, d] = prob.sf2[d] - np.sum(k.dot(ki) * k, axis=1)
        v = sla.solve_triangular(l, k.T, lower=True)
        vc[:, d] = prob.sf2[d] - np.sum(v * v, axis=0)
        w = g * alpha[None, :]
        jac[:, d] = (w.sum(axis=1)[:, None] * X - w.dot(prob.Z)) / prob.ls[d][None, :] ** 2
    return mu, jac, vi, vc


def _host_models():
    """the models of the case table up to N_HOST_MAX rows, with the largest batch each is asked (up to 65 queries)"""
    models = {}
    for c in G.CASES:
        key = (c["Np"] - c["r"], c["D"], c["n_out"], c["kern"])
        if key[0] <= N_HOST_MAX:
            models[key] = max(models.get(key, 0), min(c["T"], 65))
    return sorted(models.items())


@pytest.mark.parametrize("key,T", _host_models(), ids=["N%d-D%d-n%d-%s" % k for k, _ in _host_models()])
def test_reference_against_two_fp64_routes(key, T):
    """the explicit-inverse route and the Cholesky-solve route of the DENSE fp64 matrix stay under a quarter of the bars"""
    N, D, n_out, kern = key
    prob, ref = R.cached(15, N, D, n_out, kern)
    X, qc, res = R.queries_for(ref, T)
    bar_mu, bar_var, bar_jac = R.bars(ref, res)
    mu, jac, var_inv, var_chol = _dense_predict(prob, X)
    shares = [np.abs(mu - res["mu"]) / bar_mu, np.abs(jac - res["jac"]) / bar_jac, np.abs(var_inv - res["var"]) / bar_var,
              np.abs(var_chol - res["var"]) / bar_var]
    assert max(s.max() for s in shares) <= 0.25, [float(s.max()) for s in shares]


def test_dropped_cross_cluster_terms():
    """N = 300 (four clusters): the reference's mu against a dense np.longdouble evaluation that keeps every cross-cluster
    term -- they are below 1e-25 of the signal, so the two agree to the rounding of long double"""
    for kern in ("rbf", "mat52"):
        prob, ref = R.cached(15, 300, 3, 2, kern)
        X, qc = prob.queries(12, 1)
        res = ref.predict(X, qc)
        cross_max = 0.0
        for d in range(prob.n_out):
            k, _ = R.kernel_ld(kern, prob.Z, prob.Z, prob.ls[d], prob.sf2[d])
            other = prob.member[:, None] != prob.member[None, :]
            cross_max = max(cross_max, float(np.abs(k[other]).max()))
            l = R.cholesky_ld((k + k.T) / 2 + R.LD(prob.nugget[d]) * np.eye(prob.N, dtype=R.LD))
            alpha = R.solve_upper_ld(l, R.solve_lower_ld(l, np.asarray(prob.Y[:, d], dtype=R.LD)[:, None]))[:, 0]
            ks, _ = R.kernel_ld(kern, X, prob.Z, prob.ls[d], prob.sf2[d])
            mu = ks.dot(alpha)
            v = R.solve_lower_ld(l, ks.T)
            var = R.LD(prob.sf2[d]) - np.sum(v * v, axis=0)
            eps = float(np.finfo(R.LD).eps)
            # (the outputs of predict() are rounded to fp64: 2^-53 relative on top of the long-double rounding of 300-term sums)
            tol = (300 * eps + 2.0 ** -52) * res["s_mu"][:, d]
            assert np.all(np.abs(mu.astype(np.float64) - res["mu"][:, d]) <= tol)
            assert np.all(np.abs(var.astype(np.float64) - res["var"][:, d]) <= (300 * eps * res["kappa"][:, d] + 2.0 ** -52) * prob.sf2[d])
        assert cross_max < 1e-25, cross_max


@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_data_conditions(c):
    """every GPU case's data can tell a wrong kernel: the assertions the GPU test repeats, here without a device"""
    prob, ref = R.cached(15, c["Np"] - c["r"], c["D"], c["n_out"], c["kern"])
    assert prob.c <= 128 and np.all(np.bincount(prob.member, minlength=prob.c) <= R.CLUSTER)
    X, qc, res = R.queries_for(ref, c["T"])
    R.bars(ref, res)
    R.data_conditions(ref, res, X, qc, c["Np"], c["T"] >= 5)


def test_case_table_meets_every_streamed_form(lib_built):
    """sr_test_stream_plan at 256 CUs: every case's declared form is the one the library's predicates give, every streamed
    form of the table is met, and no batch of <= 64 queries reaches 8 groups of 16 columns per workgroup"""
    met = set()
    for c in G.CASES:
        e = G.case_expected(c, 256)
        G.check_target(c, e)
        met.add((e["route"], e["src"], e["width"], e["multi"], e["reduce_items"] > G.REDUCE_REGS))
    for route, src, width in (("stream1", 1, 1), ("stream1", 1, 4), ("stream1", 0, 1), ("stream1", 0, 4), ("mfma1", 1, 1),
                              ("mfma1", 0, 1), ("mfma1", 1, 2), ("mfma1", 0, 2), ("mfma1", 0, 4)):
        assert (route, src, width, 0, False) in met, (route, src, width)
    for width in (1, 2, 4):
        for gt in (False, True):
            assert ("runs", 0, width, 0, gt) in met, ("runs", width, gt)
    assert ("runs", 0, 4, 1, False) in met and ("runs", 0, 4, 1, True) in met, "MULTI"
    for route in ("K0", "K2s", "K2b", "K2m", "K2"):
        assert any(m[0] == route for m in met), route
    # the first sizes at which the planner turns to MULTI and to the reduce kernel's long form (as the issue found)
    assert G.stream_plan(2944, 4, 64, 256, False)[3:5] == (67, 64)
    assert G.stream_plan(4992, 2, 33, 256, False)[3:5] == (129, 128) and G.stream_plan(4992, 2, 33, 304, False)[3:5] == (147, 147)
    assert G.stream_plan(3456, 1, 17, 256, False)[5] > G.REDUCE_REGS >= G.stream_plan(3328, 1, 17, 256, False)[5]
    # G = 8 (128 columns per workgroup) needs 128 columns: no batch gp_pass streams (T <= SR_STREAM_MAX_T = 64) gets there
    for Np in range(512, 16384 + 1, 128):
        for n_out in (1, 2, 3, 4, 8):
            for ncols in (16, 32, 64):
                assert G.stream_plan(Np, n_out, ncols, 256, False)[0] <= 4, (Np, n_out, ncols)
    assert any(G.stream_plan(Np, 4, 128, 256, False)[0] == 8 for Np in range(512, 4096, 128))
    # r in RS on the first shape of every streamed form; every edge pair on both sides
    for form, shapes, _ in G._streamed_forms():
        Np, n_out, T, kern, D = shapes[0]
        assert {c["r"] for c in G.CASES if c["form"] == form and (c["Np"], c["T"], c["kern"], c["D"]) == (Np, T, kern, D)} == \
            set((0,) + G.RS), form


def test_thresholds_mirrored():
    """the thresholds expected_route restates are those of the sources"""
    common, stream, post = _read("sr_common.h"), _read("sr_stream.hip"), _read("sr_capi_posterior.hip")
    for name in ("SR_FUSED_NP", "SR_FUSED_T", "SR_STREAM_MIN_NP", "SR_STREAM_MAX_T", "SR_SMALL_T", "SR_ONE_STREAMED_NP",
                 "SR_MFMA_SMALL_MAX_NP", "SR_STREAM_FUSED_MAX_D", "SR_STREAM_FUSED32_MAX_NCB", "SR_FINAL_WAVE_T", "SR_ST1_SLOTS_MAX"):
        assert getattr(G, name) == _define(common, name), name
    m = re.search(r"sr_gp_small_wanted\(.*?\{(.*?)\n\}", common, re.S)
    assert m and re.search(r"Np == 512 && T <= 128\) return false", m.group(1))
    assert re.search(r"D\s*<=\s*%d\s*;" % G.K0_MAX_D, m.group(1))
    assert re.search(r"can_fuse && nc == 16 && ncb <= %d\b" % G.FUSED16_MAX_NCB, stream)
    assert re.search(r"sr_st_items_rows\(a\.ncb - 1, KR\) <= %d\)" % G.REDUCE_REGS, stream)
    assert re.search(r'sr_lab_env\("SR_BAL_THR", %d\)' % G.BAL_THR, common)
    assert re.search(r"return U >= thr \? 512 : \(U >= 256 \? 256 : U\);", common)
    m = re.search(r"sr_var_small_groups_max\(.*?\{(.*?)\n\}", common, re.S)
    assert m and "300e6 / bytes" in m.group(1) and "Np * (double)Np * 4.0" in m.group(1) and "g > %d" % G.VAR_SMALL_GROUPS in m.group(1)
    m = re.search(r"sr_var64_wanted\(.*?\{(.*?)\n\}", common, re.S)
    assert m and "Np <= %d && wgs128 < %d" % (G.VAR64_MAX_NP, G.VAR64_WGS) in m.group(1)
    m = re.search(r"sr_var_splitk_wanted\(.*?\{(.*?)\n\}", common, re.S)
    assert m and "nrb > 2 && wgs <= %d" % G.SPLITK_WGS in m.group(1)
    assert _define(common, "SR_KSTAR_WGS") == G.NSPLIT_WGS
    m = re.search(r"sr_kstar_nsplit\(.*?\{(.*?)\n\}", common, re.S)
    assert m and "long ns = (SR_KSTAR_WGS + blocks - 1) / blocks;" in m.group(1)
    assert "Tc >= 2 && Tc <= 4 && h->Np <= SR_MFMA_SMALL_MAX_NP" in post
    assert "nslot <= SR_ST1_SLOTS_MAX && 2 * ncb <= 64" in post
    widths = [int(w) for w in re.findall(r"if \(ncols <= (\d+)\) return \1;", stream)]
    assert widths == [1, 4, 16, 32, 64] and [G.stream_width(w) for w in widths] == widths
    assert [G.stream_width(w + 1) for w in widths] == [4, 16, 32, 64, 128]


def test_pick_nsplit_and_groups():
    """spot values of the two small helpers the mirror restates (the second clamp of pick_nsplit; the 300 MB rule)"""
    assert G.pick_nsplit(256, 2, 4096) == 16 and G.pick_nsplit(256, 2, 4224) == 16
    assert G.pick_nsplit(5120, 2, 4096) == 24 and G.pick_nsplit(5120, 1, 8192) == 24 and G.pick_nsplit(2048, 1, 8192) == 16
    assert [G.var_small_groups_max(Np, 2) for Np in (2048, 2560, 640)] == [8, 5, 64]


def test_new_symbols_bound(lib_built):
    from safe_exploration_amd import _lib
    from safe_exploration_amd.ssm_hip.gaussian_process import SimpleGPModel
    for name in ("sr_gp_last_route", "sr_test_stream_plan"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        header = f.read()
    assert int(re.search(r"#define SR_ROUTE_WORDS (\d+)", header).group(1)) == len(SimpleGPModel.ROUTE_WORDS)
    ids = re.search(r"enum \{ SR_ROUTE_K0 = 1,([^}]*)\}", header).group(1)
    assert ["K0"] + [s.strip()[len("SR_ROUTE_"):] for s in ids.split(",")] == [n.upper() for n in SimpleGPModel.ROUTE_NAMES[1:]]
    out = (ctypes.c_int * 6)()
    assert _lib.lib.sr_test_stream_plan(1000, 2, 16, 256, 0, out) == _lib.SR_EINVAL       # (not a multiple of 128)
    assert _lib.lib.sr_test_stream_plan(1024, 2, 4, 256, 0, out) == _lib.SR_EINVAL        # (the MFMA route starts at 5 columns)
    assert _lib.lib.sr_test_stream_plan(1024, 2, 16, 256, 0, None) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_route(None, out, 6) == _lib.SR_EINVAL
