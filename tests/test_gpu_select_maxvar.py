"""Greedy max-variance selection by pivoted Cholesky downdates on the device (choose_datapoints_maxvar(route="downdate"),
sr_gp_select_maxvar) against fp64 oracles and against the predict route it stands beside.

Oracles: orc.choose_datapoints_maxvar (ARD-RBF, a refit per round) and, for every kernel identifier, the greedy refit below
(an explicit solve of K_SS + sigma^2 I per round and output, fp64).  Every case asserts that its data are informative: at
every greedy round the oracle's best and second-best scores differ by more than 1e-9 relative, so a pick can only differ
through a wrong kernel, factor or tie rule, not through rounding.  Scores: atol 1e-10 sum_d max_x k_d(x, x)."""
import ctypes

import numpy as np
import pytest

from _helpers import hyp_from, mu_atol, oracle_model, width_problem
from oracle import oracle_np as orc
from test_gpu_widths import _seed

pytestmark = pytest.mark.gpu

GAP = 1e-9
NOISE_DIAG = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


def _greedy_oracle(Z, kts, hyp, noise, init, m):
    """picks, scores (sum_d max(var_d, 1e-15) at each pick, before it is taken) and the relative gap between the best and
    the second-best score of every greedy round; noise = sigma_n^2 + noise_diag (the jitter is added here)"""
    n, n_out = Z.shape[0], len(kts)
    kdiag = np.stack([orc.kernel_diag(kt, h, Z) for kt, h in zip(kts, hyp)], 1)
    K = [orc.kernel_matrix(kt, h, Z, Z) for kt, h in zip(kts, hyp)]
    picks, scores, gaps = [], [], []
    for r in range(m):
        var = kdiag.copy()
        if picks:
            for d in range(n_out):
                Kss = K[d][np.ix_(picks, picks)] + (noise[d] + orc.GPY_JITTER) * np.eye(len(picks))
                Kxs = K[d][:, picks]
                var[:, d] -= np.sum(Kxs * np.linalg.solve(Kss, Kxs.T).T, axis=1)
        s = np.clip(var, orc.GPY_VAR_CLIP, np.inf).sum(1)
        if r < len(init):
            j = int(init[r])
        else:
            masked = s.copy()
            masked[picks] = -np.inf
            j = int(np.argmax(masked))
            if n - len(picks) > 1:
                gaps.append((masked[j] - np.max(np.delete(masked, j))) / masked[j])
        picks.append(j)
        scores.append(s[j])
    return np.array(picks), np.array(scores), np.array(gaps)


def _scale(prob):
    return float(sum(np.max(orc.kernel_diag(kt, h, prob["Z"])) for kt, h in zip(prob["kts"], prob["hyp"])))


def _model(prob):
    from safe_exploration_amd import SimpleGPModel
    n_out, D = len(prob["kts"]), prob["Z"].shape[1]
    return SimpleGPModel(n_out, D - 1, 1, kern_types=prob["kts"],
                         hyp=[dict(h, noise_variance=nv) for h, nv in zip(prob["hyp"], prob["noise"])])


def _informative(kt, D, n, n_out, k, m, tag):
    """the first of a few seeded problems whose greedy rounds are all informative (the seed search of test_gpu_widths)"""
    for attempt in range(8):
        prob = width_problem(_seed(tag, kt, D, n, n_out, attempt), kt, D, n, n_out)
        init = [int(i) for i in np.random.default_rng(_seed("init", tag, attempt)).choice(n, k, replace=False)]
        ref = _greedy_oracle(prob["Z"], prob["kts"], prob["hyp"], prob["noise"] + NOISE_DIAG, init, m)
        if len(ref[2]) == 0 or ref[2].min() > GAP:
            return prob, init, ref
    pytest.fail("no informative problem among 8 seeds for %s" % ((kt, D, n, n_out, k, m),))


def _check(prob, init, ref, m, predict_route=True):
    picks, scores, gaps = ref
    assert len(gaps) == 0 or gaps.min() > GAP, "uninformative data: smallest gap %.2e" % gaps.min()
    gp = _model(prob)
    Z, Y = prob["Z"], prob["Y"]
    xs, ys, idx, sc = gp.choose_datapoints_maxvar(Z, Y, m, init_idx=init, return_index=True, route="downdate",
                                                  return_scores=True)
    np.testing.assert_array_equal(idx, picks)
    np.testing.assert_array_equal(xs, Z[picks])
    np.testing.assert_array_equal(ys, Y[picks])
    np.testing.assert_allclose(sc, scores, rtol=0, atol=1e-10 * _scale(prob))
    assert np.all(np.diff(sc[len(init):]) <= 0), "scores increase after the seeds"
    assert np.isfinite(sc).all()
    if predict_route:
        idx2 = _model(prob).choose_datapoints_maxvar(Z, Y, m, init_idx=init, return_index=True, route="predict")[2]
        np.testing.assert_array_equal(idx2, idx)
    return gp, idx, sc


# ------------------------------------------------------------------ against the oracles
def test_rbf_matches_reference_oracle_and_predict_route():
    """the data and seeds of test_max_variance_data_selection: picks of orc.choose_datapoints_maxvar, scores of the greedy
    refit, the same picks as route="predict", and the model after selection equals a fresh fit on the chosen rows"""
    from safe_exploration_amd import SimpleGPModel
    syn = orc.make_synthetic(123, 300, 2, 1, 4)
    ls, sf2, nv = syn["lengthscale"], syn["signal_var"], syn["noise_var"]
    init = [3, 57, 111, 160, 201, 250, 299, 8, 77, 140]
    hyp = [{"lengthscale": ls[d], "variance": sf2[d]} for d in range(2)]
    ref = _greedy_oracle(syn["Z"], ["rbf"] * 2, hyp, nv, init, 40)
    np.testing.assert_array_equal(ref[0], orc.choose_datapoints_maxvar(syn["Z"], syn["Y"], 40, init, ls, sf2, nv))
    prob = dict(Z=syn["Z"], Y=syn["Y"], kts=["rbf"] * 2, hyp=hyp, noise=nv - NOISE_DIAG)
    gp, idx, _ = _check(prob, init, ref, 40)
    xs, ys = syn["Z"][idx], syn["Y"][idx]
    assert gp.gp_trained and gp._beta is None and gp._inv_K is None
    np.testing.assert_array_equal(gp.z, xs)
    np.testing.assert_array_equal(gp.z_fit, xs)
    np.testing.assert_array_equal(gp.y_z, ys)
    np.testing.assert_array_equal(gp.x_train, syn["Z"])
    np.testing.assert_array_equal(gp.y_train, syn["Y"])
    x = np.hstack((syn["p"], syn["k_ff"]))
    mu, var = gp.predict(x)
    om = oracle_model(xs, ys, ls, sf2, nv)
    rmu, rvar = orc.gp_predict(x, om["Z"], om["beta"], om["inv_K"], om["lengthscale"], om["signal_var"], False)
    np.testing.assert_allclose(mu, rmu, rtol=1e-9, atol=max(mu_atol(om), 1e-12))
    np.testing.assert_allclose(var, rvar, rtol=0, atol=1e-9)
    # a model built with the reference's hyp list gives the same
    gp2 = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp_from(ls, sf2, nv), m=40)
    np.testing.assert_array_equal(gp2.choose_datapoints_maxvar(syn["Z"], syn["Y"], 40, init_idx=init, return_index=True,
                                                               route="downdate")[2], idx)


@pytest.mark.parametrize("kt", ["mat52", "lin_rbf", "lin_mat52"])
def test_general_kernels_match_greedy_oracle(kt):
    prob, init, ref = _informative(kt, 3, 300, 2, 5, 40, "general")
    _check(prob, init, ref, 40)


def test_train_with_downdate_route_chooses_the_same_rows():
    """np.random.seed(0); train(X, Y, m=40, opt_hyp=False): the k-means seeds come from the same RNG state, the downdate
    route (set_select_route) picks the rows of the default route; update_model follows the model's route too"""
    from safe_exploration_amd import SimpleGPModel
    syn = orc.make_synthetic(123, 300, 2, 1, 4)
    hyp = hyp_from(syn["lengthscale"], syn["signal_var"], syn["noise_var"])
    a = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, m=40)
    b = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=hyp, m=40)
    b.set_select_route("downdate")
    np.random.seed(0)
    a.train(syn["Z"], syn["Y"], m=40, opt_hyp=False)
    np.random.seed(0)
    b.train(syn["Z"], syn["Y"], m=40, opt_hyp=False)
    np.testing.assert_array_equal(a.z, b.z)
    # informative: the picks in order, their seeds, and the oracle's gaps
    rows = {tuple(r): i for i, r in enumerate(syn["Z"])}
    idx = np.array([rows[tuple(r)] for r in b.z])
    k = min(int(300 * 0.25), 10)
    hy = [{"lengthscale": syn["lengthscale"][d], "variance": syn["signal_var"][d]} for d in range(2)]
    picks, _, gaps = _greedy_oracle(syn["Z"], ["rbf"] * 2, hy, syn["noise_var"], list(idx[:k]), 40)
    assert gaps.min() > GAP
    np.testing.assert_array_equal(picks, idx)
    np.random.seed(1)
    a.update_model(syn["Z"][:120], syn["Y"][:120], opt_hyp=False, replace_old=True)
    np.random.seed(1)
    b.update_model(syn["Z"][:120], syn["Y"][:120], opt_hyp=False, replace_old=True)
    np.testing.assert_array_equal(a.z, b.z)


# ------------------------------------------------------------------ edges
# (kernel, D, n, n_out, k, m): pool sizes around the 64-row workgroup tile (one below, a multiple, one past), no greedy
# round (m = k, m = k = 1) and m = n - 1, n_out 1 / 2 / 4 / 9, every compiled width edge D 2 3 4 5 8 12
EDGE_CASES = [
    ("rbf", 2, 191, 1, 3, 190),
    ("mat52", 3, 192, 2, 4, 40),
    ("lin_rbf", 4, 193, 4, 5, 5),
    ("lin_mat52", 5, 127, 9, 2, 30),
    ("rbf", 8, 128, 2, 1, 127),
    ("mat52", 12, 129, 4, 3, 50),
    ("rbf", 12, 65, 9, 1, 1),
]


@pytest.mark.parametrize("kt,D,n,n_out,k,m", EDGE_CASES)
def test_edges(kt, D, n, n_out, k, m):
    prob, init, ref = _informative(kt, D, n, n_out, k, m, "edge")
    _check(prob, init, ref, m)


def test_duplicate_rows_tie_to_the_lower_index():
    """two identical rows far outside the pool (the linear part makes them the largest variance): equal scores to the
    bit, the lower index wins, no NaN after the duplicate's variance collapses"""
    prob = width_problem(_seed("dup"), "lin_rbf", 3, 200, 2)
    Z, Y = prob["Z"].copy(), prob["Y"]
    a, b = 37, 150
    Z[a] = Z[b] = np.array([0.5, 6.0, -0.5])
    prob = dict(prob, Z=Z)
    init = [0, 1, 2, 3]
    gp = _model(prob)
    idx, sc = gp.choose_datapoints_maxvar(Z, Y, 30, init_idx=init, return_index=True, route="downdate",
                                          return_scores=True)[2:]
    assert idx[4] == a and b not in idx[4:6]
    assert np.isfinite(sc).all()
    sa = gp.choose_datapoints_maxvar(Z, Y, 5, init_idx=init + [a], route="downdate", return_scores=True)[2][-1]
    sb = gp.choose_datapoints_maxvar(Z, Y, 5, init_idx=init + [b], route="downdate", return_scores=True)[2][-1]
    assert sa == sb == sc[4]


# ------------------------------------------------------------------ the C entry point
def _capi(n=193, m=41, k=3):
    import torch
    prob, init, ref = _informative("mat52", 3, n, 2, k, m, "capi")
    gp = _model(prob)
    gp.choose_datapoints_maxvar(prob["Z"], prob["Y"], k, init_idx=init, route="downdate")   # kernel + noise on the handle
    dev = gp._handle.device
    tx = torch.from_numpy(prob["Z"]).to(dev)
    seeds = torch.tensor(init, dtype=torch.int32, device=dev)
    return gp, tx, seeds, ref


def _call(gp, tx, n, m, seeds, k, score=True):
    import torch
    from safe_exploration_amd import _lib
    from safe_exploration_amd import _buffers as B
    dev = gp._handle.device
    idx = torch.full((max(m, 1),), -7, dtype=torch.int32, device=dev)
    sc = torch.full((max(m, 1),), float("nan"), dtype=torch.float64, device=dev)
    rc = _lib.lib.sr_gp_select_maxvar(gp._handle.h, B.ptr(tx), n, m, B.ptr(seeds), k, B.ptr(idx),
                                      B.ptr(sc) if score else None, B.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, idx.cpu().numpy(), sc.cpu().numpy()


def test_capi_repeatable_after_release_and_nan_prefilled():
    from safe_exploration_amd import _lib
    gp, tx, seeds, ref = _capi()
    n, m, k = tx.shape[0], 41, 3
    rc, i1, s1 = _call(gp, tx, n, m, seeds, k)
    assert rc == _lib.SR_OK
    np.testing.assert_array_equal(i1, ref[0])
    assert np.isfinite(s1).all()
    rc, i2, s2 = _call(gp, tx, n, m, seeds, k)
    assert rc == _lib.SR_OK and np.array_equal(i1, i2) and s1.tobytes() == s2.tobytes()
    gp.release_scratch()
    rc, i3, s3 = _call(gp, tx, n, m, seeds, k)
    assert rc == _lib.SR_OK and np.array_equal(i1, i3) and s1.tobytes() == s3.tobytes()
    rc, i4, s4 = _call(gp, tx, n, m, seeds, k, score=False)        # score may be NULL
    assert rc == _lib.SR_OK and np.array_equal(i1, i4) and np.isnan(s4).all()


def test_capi_rejects_bad_arguments():
    import torch
    from safe_exploration_amd import _lib
    gp, tx, seeds, _ = _capi()
    n = tx.shape[0]
    dev = tx.device
    bad_seed = torch.tensor([0, n], dtype=torch.int32, device=dev)
    neg_seed = torch.tensor([-1, 4], dtype=torch.int32, device=dev)
    dup_seed = torch.tensor([5, 5], dtype=torch.int32, device=dev)
    for args in ((n, 10, seeds, 0), (n, 2, seeds, 3), (n, n + 1, seeds, 3), (n, 10, bad_seed, 2), (n, 10, neg_seed, 2),
                 (n, 10, dup_seed, 2)):
        rc, idx, sc = _call(gp, tx, *args)
        assert rc == _lib.SR_EINVAL, args
        assert (idx == -7).all() and np.isnan(sc).all(), args
