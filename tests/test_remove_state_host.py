"""CPU side of tests/test_gpu_remove_state.py: Problem.without + FactorRef against a dense long-double factorisation of the
remaining rows, the closed form of tests/_remove_ref.py chained in fp64 through every GPU case's removals under a quarter of
every bar (U^-1, alpha, log det, K^-1, both leave-one-out outputs), the proof on the reference side that every case's data can
tell a carry dropped at the loop edge the case claims, the case table against the constants and loops of csrc/sr_remove.hip and
the predicates of csrc/sr_capi_remove.hip, and the refusals of sr_gp_last_remove that need no device.  Runs without a GPU."""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import _factor_ref as F
import _posterior_ref as R
import _remove_ref as rr
import test_factor_ref_host as H
import test_gpu_remove_state as G

QUARTER = 0.25
MISS = 100.0                     # bars a broken loop edge must miss the reference by


# ---- without + FactorRef against a dense long-double factorisation -------------------------------------------------------
def _dense_ld(prob, d):
    """(U^-1, alpha, log det) of output d from a long-double Cholesky of the WHOLE matrix, which keeps every cross-cluster term"""
    n = prob.N
    k, _ = R.kernel_ld(prob.kern, prob.Z, prob.Z, prob.ls[d], prob.sf2[d])
    l = R.cholesky_ld((k + k.T) / 2 + R.LD(prob.nugget[d]) * np.eye(n, dtype=R.LD))
    w = R.solve_lower_ld(l, np.eye(n, dtype=R.LD)).T
    alpha = R.solve_upper_ld(l, R.solve_lower_ld(l, np.asarray(prob.Y[:, d], dtype=R.LD)[:, None]))[:, 0]
    return w, alpha, 2 * np.sum(np.log(np.diag(l)))


def test_without_against_dense_long_double():
    """N = 300 (four clusters; rows 5 and 9 share cluster 1): three removals, an append of three points, three more removals
    (one of them an appended point).  The blocks of the remaining rows against a dense long-double factorisation of them: equal
    to 1e-17 relative, the leave-one-out outputs too; the rows that stay keep their order"""
    tol = 1e-17 * float(np.finfo(R.LD).eps) / 2.0 ** -63
    prob = F.problem(G.SEED, 300, 3, 2)
    assert prob.member[5] == prob.member[9]
    keep = np.delete(np.arange(300), [5, 9, 200])
    p1 = prob.without([200, 5, 9])
    assert np.array_equal(p1.Z, prob.Z[keep]) and np.array_equal(p1.Y, prob.Y[keep]) and np.array_equal(p1.member, prob.member[keep])
    x, y, q = p1.new_points(3, 1)
    p2 = p1.grown(x, y, q).without([0, 150, 298])
    assert p2.N == 297 and np.array_equal(p2.Z[-2:], x[[0, 2]]) and prob.N == 300 and p1.N == 297
    ref = F.FactorRef(p2, appends=7)
    assert ref.bar_w(0, 0) == pytest.approx(8 * F.FactorRef(p2).bar_w(0, 0), rel=1e-14)
    for d in range(2):
        w, alpha, logdet = _dense_ld(p2, d)
        wr, ar = np.zeros((297, 297), dtype=R.LD), np.zeros(297, dtype=R.LD)
        for c, i in enumerate(ref.idx):
            wr[np.ix_(i, i)] = ref.block(c, d)["W"]
            ar[i] = ref.block(c, d)["alpha"]
        assert float(np.abs(w - wr).max() / np.abs(wr).max()) <= tol
        assert float(np.abs(alpha - ar).max() / np.abs(ar).max()) <= tol
        assert abs(float(logdet) - ref.logdet(d)) <= 2.0 ** -52 * abs(ref.logdet(d))
        var = 1 / np.sum(w * w, axis=1)
        mu = np.asarray(p2.Y[:, d], dtype=R.LD) - alpha * var
        rmu, rvar, bmu, bvar = ref.loo(d)
        assert np.abs(var.astype(np.float64) - rvar).max() <= 2.0 ** -52 * rvar.max()
        assert np.abs(mu.astype(np.float64) - rmu).max() <= 2.0 ** -51 * max(np.abs(rmu).max(), np.abs(p2.Y).max())
        assert np.all(bmu > 0) and np.all(bvar > 0)
    with pytest.raises(AssertionError):
        prob.without([3, 3])


def test_dense_problem_and_reference_time():
    """the dense problems are one cluster of the same recipe (b = N in the bars), and their reference -- a dense long-double
    Cholesky through cholesky_ld / solve_*_ld -- stays under ~5 s per case on an idle core"""
    for c in G.CASES:
        if not c["dense"]:
            continue
        t0 = time.perf_counter()
        prob = G.problem_of(c)
        assert prob.c == 1 and np.all(prob.member == 0) and -(-c["N0"] // G.NB) * G.NB == 640
        ref = F.FactorRef(prob.without(G.resolve(c["ops"][0][1], prob.N)), appends=1)
        for d in range(prob.n_out):
            assert ref.block(0, d)["b"] == c["N0"] - 1
        dt = time.perf_counter() - t0
        print("%s: reference %.1f s, kappa %.0f, bar U^-1 %.2g |W|" % (c["id"], dt, ref.kappa_max(0),
                                                                     ref.bar_w(0, 0) * np.sqrt(ref.block(0, 0)["lmin"])))
        assert dt < 10.0, dt                                 # (3 s on an idle core; the bound leaves room for a busy machine)
    assert sorted(c["N0"] for c in G.CASES if c["dense"]) == [513, 540]
    same = F.problem(G.SEED, 90, 3, 2)
    assert np.array_equal(F.dense_problem(G.SEED, 90, 3, 2).Z, same.Z)     # (the cap changes nothing below it)


# ---- the closed form in fp64 through every case's removals -----------------------------------------------------------------
def _fit64(prob, rows_z, rows_y, d):
    k = H._kernel64(prob.kern, rows_z, rows_z, prob.ls[d], prob.sf2[d]) + prob.nugget[d] * np.eye(rows_z.shape[0])
    w, alpha, logdet, _ = H._route_chol(k, rows_y[:, d])
    return w, alpha, logdet


class Chain64(object):
    """the stored model cluster by cluster in fp64: a fit of every cluster's block, then _remove_ref.remove for every point a
    cluster loses (a cluster that gains a point is refitted with it first).  On block-diagonal data a removal transforms the
    retired point's cluster alone: w is zero in every other column, so a_k = 1, b_k = 0 and d does not move there"""

    def __init__(self, prob):
        self.st = {}
        self.follow(prob)

    def follow(self, prob):
        for q in range(prob.c):
            i = np.flatnonzero(prob.member == q)
            z, y = prob.Z[i], prob.Y[i]
            key = [r.tobytes() for r in z]
            if q not in self.st:
                self.st[q] = dict(key=key, z=z, y=y, f=[_fit64(prob, z, y, d) for d in range(prob.n_out)])
                continue
            s = self.st[q]
            if s["key"] == key:
                continue
            new = [k for k in key if k not in set(s["key"])]
            if new:                                            # points that joined since: behind the others
                at = [key.index(k) for k in new]
                s["z"], s["y"] = np.vstack((s["z"], z[at])), np.vstack((s["y"], y[at]))
                s["key"] = s["key"] + new
                s["f"] = [_fit64(prob, s["z"], s["y"], d) for d in range(prob.n_out)]
            gone = [t for t, k in enumerate(s["key"]) if k not in set(key)]
            for t in sorted(gone, reverse=True):
                f = []
                for w, alpha, logdet in s["f"]:
                    w1, a1, lr = rr.remove(w, alpha, t)
                    f.append((w1[1:, 1:], a1[1:], logdet + lr))
                s["f"] = f
                s["z"], s["y"] = np.delete(s["z"], t, axis=0), np.delete(s["y"], t, axis=0)
                del s["key"][t]
            assert s["key"] == key

    def share(self, ref):
        """largest share of a bar of ref the chained fp64 state takes"""
        p = ref.p
        worst = dict(w=0.0, alpha=0.0, logdet=0.0, kinv=0.0, loo_mu=0.0, loo_var=0.0)
        for d in range(p.n_out):
            rmu, rvar, bmu, bvar = ref.loo(d)
            logdet = 0.0
            for q, i in enumerate(ref.idx):
                w, alpha, ld = self.st[q]["f"][d]
                blk = ref.block(q, d)
                mu, var = rr.loo(w, alpha, p.Y[i, d])
                logdet += ld
                for key, v in (("w", np.abs(w - blk["W64"]).max() / ref.bar_w(q, d)),
                               ("alpha", np.abs(alpha - blk["alpha64"]).max() / ref.bar_alpha(q, d)),
                               ("kinv", np.abs(w.dot(w.T) - blk["Kinv64"]).max() / ref.bar_kinv(q, d)),
                               ("loo_mu", (np.abs(mu - rmu[i]) / bmu[i]).max()), ("loo_var", (np.abs(var - rvar[i]) / bvar[i]).max())):
                    worst[key] = max(worst[key], float(v))
            worst["logdet"] = max(worst["logdet"], abs(logdet - ref.logdet(d)) / ref.bar_logdet(d))
        return worst


@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_fp64_closed_form_under_a_quarter_of_every_bar(c):
    """if this fails for a case the DERIVATION of a bar is wrong, not the factor"""
    prob0 = G.problem_of(c)
    chain = Chain64(prob0)
    ref, t_ref = None, 0.0
    for k, prob, a, reps in G.walk(c, prob0):
        t0 = time.perf_counter()
        ref = G._adopt(F.FactorRef(prob, appends=a), ref)
        for d in range(prob.n_out):
            for q in range(prob.c):
                ref.block(q, d)
        t_ref += time.perf_counter() - t0
        chain.follow(prob)
        share = chain.share(ref)
        print("%s op %d (a = %d): fp64 closed form at %s of the bars" % (c["id"], k, a, {key: "%.2g" % v for key, v in share.items()}))
        assert max(share.values()) <= QUARTER, (c["id"], k, share)
    print("%s: reference side %.1f s" % (c["id"], t_ref))
    assert ref is not None and ref.p.N == c["N0"] + sum(op[0] == "app" for op in c["ops"]) - sum(len(op[1]) for op in c["ops"] if op[0] == "rm")


# ---- the data can tell -----------------------------------------------------------------------------------------------------
def remove_variant(Wt, alpha, q, cols, d_reset=None, p_reset=None):
    """_remove_ref.remove with a loop edge broken.  cols: the padded column index of every column of Wt (a cluster's block sits
    at its members' padded indices).  d_reset: the running dot product d starts again from zero at that padded column (the rows
    kernel's carry lost between two steps of SR_RM_CHUNK columns); p_reset: the running p^2 does (the row-norm kernel's carry
    lost between two steps of 4 SR_RM_NORM_T columns; rho^2 with it).  Neither: _remove_ref.remove, bit for bit"""
    n = Wt.shape[0]
    w = Wt[q, q:]
    ck = np.concatenate((cols[q:], [np.iinfo(np.int64).max]))                        # column of p2[t], d[:, t]: q + t (the last: the end)
    p2 = np.concatenate((np.zeros(1, dtype=Wt.dtype), np.cumsum(w * w)))
    if p_reset is not None:
        lost = np.sum((w * w)[cols[q:] < p_reset])
        p2 = np.where(ck >= p_reset, p2 - lost, p2)
    p = np.sqrt(p2)
    rho2 = p2[-1]
    X = Wt[:, q:]
    prod = X * w
    d = np.concatenate((np.zeros((n, 1), dtype=Wt.dtype), np.cumsum(prod, axis=1)), axis=1)
    if d_reset is not None:
        lost = np.sum(prod[:, cols[q:] < d_reset], axis=1)
        d = np.where((ck >= d_reset)[None, :], d - lost[:, None], d)
    Xn = np.array(Wt)
    t = np.arange(1, n - q)
    with np.errstate(all="ignore"):
        Xn[:, q + t] = (p[t] * X[:, t] - w[t] * d[:, t] / p[t]) / p[t + 1]
        a_new = alpha - d[:, -1] / rho2 * alpha[q]
        logrho = float(np.log(rho2))
    src = np.array([i for i in range(n) if i != q])
    dst = src + (src < q)
    out = np.eye(n, dtype=Wt.dtype)
    out[np.ix_(dst, dst)] = Xn[np.ix_(src, src)]
    a_out = np.zeros(n, dtype=Wt.dtype)
    a_out[dst] = a_new[src]
    return out, a_out, logrho


def _before_first_removal(c):
    """(problem, a, j) as the case's first removed point meets them"""
    prob, a, n_app = G.problem_of(c), 0, 0
    for op in c["ops"]:
        if op[0] == "rm":
            return prob, a, max(G.resolve(op[1], prob.N))
        n_app += 1
        x, y, qn = prob.new_points(1, n_app)
        prob, a = prob.grown(x, y, qn), a + 1
        if op[0] == "win":
            return prob, a, 0
    raise AssertionError("a case without a removal")


def edges_of(c):
    """the loop edges the case's first removal claims: padded columns at which the rows kernel hands d to its next step (the
    first multiple of SR_RM_CHUNK behind q and the last one inside the matrix) and at which the row-norm kernel hands p^2 on"""
    N0, Np0, j = G.first_removal(c)
    q = j + Np0 - N0
    first, last = (q // G.SR_RM_CHUNK + 1) * G.SR_RM_CHUNK, (Np0 - 1) // G.SR_RM_CHUNK * G.SR_RM_CHUNK
    d_edges = sorted({b for b in (first, last) if q < b < Np0})
    p_edges = [q + s * G.NORM_STEP for s in range(1, c["claims"][0])]
    return d_edges, p_edges


@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_the_data_can_tell_a_broken_loop_edge(c):
    """for every loop edge a case claims, the closed form with the carry dropped THERE misses the reference of the remaining
    rows by at least 100 bars on some entry of U^-1 or alpha (a value that is not finite counts): a case whose data could not
    notice fails here, on the reference side"""
    prob, a, j = _before_first_removal(c)
    assert (prob.N, -(-prob.N // G.NB) * G.NB, j) == G.first_removal(c)
    d_edges, p_edges = edges_of(c)
    assert len(p_edges) == c["claims"][0] - 1
    off0 = -(-prob.N // G.NB) * G.NB - prob.N
    qc = int(prob.member[j])
    i = np.flatnonzero(prob.member == qc)
    t = int(np.flatnonzero(i == j)[0])
    cols = i + off0
    after = F.FactorRef(prob.without([j]), appends=a + 1)
    for d in range(prob.n_out if c["vary_noise"] else 1):
        w, alpha, _ = _fit64(prob, prob.Z[i], prob.Y[i], d)
        blk = after.block(qc, d)
        plain = remove_variant(w, alpha, t, cols)
        for u, v in zip(plain, rr.remove(w, alpha, t)):
            assert np.array_equal(u, v), "the variant without a break is not _remove_ref.remove"

        def miss(out):
            wv, av = out[0][1:, 1:], out[1][1:]
            if not (np.all(np.isfinite(wv)) and np.all(np.isfinite(av))):
                return np.inf
            return max(float(np.abs(wv - blk["W64"]).max()) / after.bar_w(qc, d), float(np.abs(av - blk["alpha64"]).max()) / after.bar_alpha(qc, d))

        assert miss(plain) <= QUARTER
        for b in d_edges:
            m = miss(remove_variant(w, alpha, t, cols, d_reset=b))
            assert m >= MISS, (c["id"], "d dropped at column %d goes unnoticed" % b, m)
        for b in p_edges:
            m = miss(remove_variant(w, alpha, t, cols, p_reset=b))
            assert m >= MISS, (c["id"], "p^2 dropped at column %d goes unnoticed" % b, m)


# ---- the case table against the sources ---------------------------------------------------------------------------------
def test_constants_and_loops_mirrored():
    src, common, capi = H._read("sr_remove.hip"), H._read("sr_common.h"), H._read("sr_capi_remove.hip")
    for name in ("SR_RM_CHUNK", "SR_RM_ROWS", "SR_RM_WAVES", "SR_RM_NORM_T"):
        assert getattr(G, name) == int(H._define(src, name)), name
    assert (G.SR_RM_CHUNK, G.SR_RM_ROWS, G.SR_RM_WAVES, G.SR_RM_NORM_T) == (256, 2, 4, 1024)
    assert int(H._define(common, "SR_NB")) == G.NB == 128 and H._define(common, "SR_SLIDE_STEPS") == "SR_NB"

    def has(text, pattern):
        return re.search(re.sub(r" ", r"\\s*", pattern), text) is not None
    # the loops geometry() restates
    assert has(src, r"for \(int base = q; base < Np; base \+= 4 \* SR_RM_NORM_T\)")
    assert has(src, r"i0 = off0 \+ \(\(int\)blockIdx\.x \* SR_RM_WAVES \+ wave\) \* SR_RM_ROWS")
    assert has(src, r"for \(int cbase = i0 & ~\(SR_RM_CHUNK - 1\); cbase < Np0; cbase \+= SR_RM_CHUNK\)")
    assert has(src, r"c = cbase \+ 4 \* lane")
    assert has(src, r"reinterpret_cast<uintptr_t>\(Wt0\) % 32 == 0")
    # the predicates RemoveMirror restates
    assert has(capi, r"reuse_alt = same && h->Wt_alt && h->wt_alt_cap >=")
    assert has(capi, r"vec_alt = same && h->yT_alt && h->alpha_alt && h->vec_alt_np == Np1")
    assert has(capi, r"if \(h->wt_alt_off < off0\)")
    assert has(capi, r"keep_old = same &&[^;]*SR_FACT_PAR_BYTES \* 2")
    assert has(capi, r"clean_run = slide0 > 0 && keep_old && h->slack_ok")
    assert has(capi, r"h->wt_alt_off = off0 \+ slide0") and has(capi, r"h->vec_alt_np = Np0")
    assert has(H._read("sr_handle.h"), r"h->Wt - \(size_t\)h->slide \* \(h->Np \+ 1\)")
    # the largest factor of the table stays a spare (keep_old false needs 16 GiB: not covered)
    assert max(c["n_out"] * (-(-(c["N0"] + 6) // G.NB) * G.NB) ** 2 * 8 for c in G.CASES) <= 2 * (8 << 30)


def test_every_case_sits_on_its_edge():
    """each case's claims, written by hand, are what the restated loops give for its first removed point; and the table holds
    every edge of the issue"""
    by = {}
    for c in G.CASES:
        assert G.geometry(*G.first_removal(c)) == c["claims"], (c["id"], G.geometry(*G.first_removal(c)))
        by.setdefault(re.split("[/-]", c["id"])[0], []).append(c)
    assert sorted(c["claims"][0] for c in by["norm"]) == [1, 2, 2, 2, 3]
    N0, Np0, j = G.first_removal(by["norm"][0])
    assert Np0 - (j + Np0 - N0) == G.NORM_STEP + 1                              # a second step of ONE column
    N0, Np0, j = G.first_removal(by["norm"][1])
    assert Np0 - (j + Np0 - N0) == G.NORM_STEP
    for N0, last in ((1100, G.SR_RM_CHUNK // 2), (1280, 0)):                    # a half and a full last step
        rows = [c for c in by["rows"] if c["N0"] == N0]
        assert (-(-N0 // G.NB) * G.NB) % G.SR_RM_CHUNK == last
        assert {c["claims"][2] for c in rows} == {0, 1, 2, 3} and {c["claims"][4] for c in rows} == {"first", "second"}
        assert {255, 0} <= {c["claims"][3] for c in rows}
        qs = [G.first_removal(c)[2] + G.first_removal(c)[1] - N0 for c in rows]
        assert G.first_removal(rows[0])[1] - N0 in qs and G.first_removal(rows[0])[1] - 1 in qs      # q = off0 and q = Np - 1
    assert any(c["N0"] % 2 for c in by["rows"]) and any(G.first_removal(c)[2] == c["N0"] - 1 for c in by["rows"] if c["N0"] % 2)
    assert sorted(c["N0"] for c in by["shrink"]) == [1153, 1153, 1153, 1158, 4225]
    ten = next(c for c in by["shrink"] if c["N0"] == 1158)
    reps = [r for _, _, _, rs in G.walk(ten, G.problem_of(ten)) for r in rs]
    assert len(reps) == 10 and [r["Np1"] < r["Np0"] for r in reps].index(True) == 5 and reps[5]["Np0"] - reps[5]["Np1"] == G.NB
    # what the mirror says of every case is what its `want` pins; and every branch is pinned by some case
    seen = dict(aligned=set(), spare=set(), clean=set(), shrink=set(), kept_old=set())
    for c in G.CASES:
        n = 0
        for _, _, _, reps in G.walk(c, G.problem_of(c)):
            rep = reps[-1]
            if n < len(c["want"]):
                assert {k: rep[k] for k in c["want"][n]} == c["want"][n], (c["id"], n, rep)
                for k in ("aligned", "spare", "clean", "kept_old"):
                    if k in c["want"][n]:
                        seen[k].add(c["want"][n][k])
                if "Np1" in c["want"][n] and "Np0" in c["want"][n]:
                    seen["shrink"].add(c["want"][n]["Np1"] < c["want"][n]["Np0"])
            n += 1
        assert n >= max(1, len(c["want"]))
    assert seen == dict(aligned={0, 1}, spare={"none", "as_is", "cleared"}, clean={0, 1}, shrink={False, True}, kept_old={0, 1}), seen
    assert {c["claims"][0] for c in G.CASES} == {1, 2, 3}
    slid = {c["want"][0]["slide"]: c["want"][0]["aligned"] for c in by["slid"]}
    assert slid == {1: 0, 2: 0, 3: 0, 4: 1, 5: 0}
    assert sorted(c["n_out"] for c in by["outputs"]) == [1, 2, 4, 9] and all(c["vary_noise"] for c in by["outputs"])
    assert [(c["kern"], c["D"]) for c in by["mat52"]] == [("mat52", 6)]
    assert sorted(re.split("[/-]", c["id"])[0] for c in G.CASES if c["consumers"]) == ["norm", "slid"]
    assert all(c["n_out"] == 1 for c in G.CASES if c["N0"] in (8320, 4225))


def test_last_remove_symbol_and_refusals(lib_built):
    """the symbol, its words against the Python names, and the refusals that need no handle (those on a live handle:
    tests/test_gpu_remove_state.py::test_last_remove_refusals_and_count)"""
    from safe_exploration_amd import _lib
    from safe_exploration_amd.ssm_hip.gaussian_process import SimpleGPModel
    assert hasattr(_lib.lib, "sr_gp_last_remove") and "sr_gp_last_remove" in _lib.SIGNATURES
    with open(os.path.join(H.ROOT, "include", "safereach.h")) as f:
        header = f.read()
    assert int(re.search(r"#define SR_REMOVE_WORDS (\d+)", header).group(1)) == len(SimpleGPModel.REMOVE_WORDS)
    words = re.search(r"enum \{ SR_RM_COUNT = 0,([^}]*)\}", header).group(1)
    assert ["count"] + [s.strip()[len("SR_RM_"):].lower() for s in words.split(",")] == [w.lower() for w in SimpleGPModel.REMOVE_WORDS]
    names = re.search(r"enum \{ SR_RM_SPARE_NONE = 0,([^}]*)\}", header).group(1)
    assert ["none"] + [s.strip()[len("SR_RM_SPARE_"):].lower() for s in names.split(",")] == list(SimpleGPModel.REMOVE_SPARES)
    out = (ctypes.c_int * 11)()
    assert _lib.lib.sr_gp_last_remove(None, out, 11) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_remove(None, None, 11) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_last_remove(None, out, 0) == _lib.SR_EINVAL
