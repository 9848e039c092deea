"""Shared helpers for the parity tests (oracle side is TEST infrastructure)."""
import numpy as np

from oracle import oracle_np as orc


def hyp_from(ls, sf2, noise_var, noise_diag=1e-5):
    """hyp list for SimpleGPModel such that its diagonal term equals oracle's noise_var + 1e-8:
    oracle.gp_fit receives noise_var (already incl. noise_diag) and adds the GPy jitter itself."""
    return [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": noise_var[d] - noise_diag}
            for d in range(len(sf2))]


def oracle_model(Z, Y, ls, sf2, noise_var):
    beta, inv_K, chol = orc.gp_fit(Z, Y, ls, sf2, noise_var)
    return dict(Z=Z, beta=beta, inv_K=inv_K, chol=chol, lengthscale=ls, signal_var=sf2)


def hip_model(Z, Y, ls, sf2, noise_var, n_s, n_u):
    from safe_exploration_amd import SimpleGPModel
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp_from(ls, sf2, noise_var))
    gp.train(Z, Y, opt_hyp=False)
    return gp


def mu_atol(model):
    """atol for mu / jac: 1e-12 * sigma_f * |alpha|_1  (SURVEY 8d)."""
    return 1e-12 * float(np.sqrt(np.max(model["signal_var"])) * np.abs(model["beta"]).sum(0).max())


_ORACLE_CACHE = {}


def cached_oracle_model(seed, N, n_s, n_u, sf2=1.0):
    """oracle fit of orc.make_synthetic(seed, N, ...) -- O(N^3) on the CPU, shared between the full-size tests."""
    key = (seed, N, n_s, n_u, sf2)
    if key not in _ORACLE_CACHE:
        syn = orc.make_synthetic(seed, N, n_s, n_u, 4, sf2=sf2)
        _ORACLE_CACHE[key] = oracle_model(syn["Z"], syn["Y"], syn["lengthscale"], syn["signal_var"], syn["noise_var"])
        _ORACLE_CACHE[key]["noise_var"] = syn["noise_var"]
    return _ORACLE_CACHE[key]


# ------------------------------------------------------------------ models of any input width and output count
_WIDTH_CACHE = {}
_WIDTH_CACHE_MAX = 4          # oracle inverses of N = 3000 are 72 MB per output: keep only the last few fits


def width_problem(seed, kt, D, N, n_out, noise=1e-2):
    """Z ~ U[-1,1]^D, Y = sin(2 Z w) + noise, kernel hyper-parameters of orc.make_hyp with the stationary lengthscales
    scaled by sqrt(D / 3): without that the points of a wide input space are so far apart (in lengthscales) that k* ~ 0,
    var ~ k(x,x) and every gradient ~ 0 -- a broken kernel would still pass."""
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (N, D))
    W = rng.standard_normal((n_out, D)) / np.sqrt(D)
    Y = np.sin(2.0 * Z.dot(W.T)) + 0.05 * rng.standard_normal((N, n_out))
    hyp = []
    for _ in range(n_out):
        h = orc.make_hyp(kt, rng, D)
        if kt in ("rbf", "mat52"):
            h["lengthscale"] = h["lengthscale"] * np.sqrt(D / 3.0)
        hyp.append(h)
    return dict(Z=Z, Y=Y, kts=[kt] * n_out, hyp=hyp, noise=np.full(n_out, noise), seed=seed)


def width_oracle(prob):
    """fp64 fit of a width_problem (cached by its seed and shape); the stationary models also carry lengthscale /
    signal_var / natural scales for the tolerances."""
    Z, kts, hyp = prob["Z"], prob["kts"], prob["hyp"]
    key = (prob["seed"], kts[0], Z.shape, len(kts))
    if key not in _WIDTH_CACHE:
        beta, inv_K = orc.gp_fit_k(Z, prob["Y"], kts, hyp, prob["noise"] + 1e-5)
        if len(_WIDTH_CACHE) >= _WIDTH_CACHE_MAX:
            _WIDTH_CACHE.pop(next(iter(_WIDTH_CACHE)))
        _WIDTH_CACHE[key] = dict(Z=Z, beta=beta, inv_K=inv_K)
    om = dict(_WIDTH_CACHE[key], kts=kts, hyp=hyp)
    if kts[0] in ("rbf", "mat52"):
        om["lengthscale"] = np.array([h["lengthscale"] for h in hyp])
        om["signal_var"] = np.array([h["variance"] for h in hyp])
        l_min = float(np.min(om["lengthscale"]))
    else:
        st = "rbf" if kts[0] == "lin_rbf" else "mat52"
        l_min = min(float(np.asarray(h["prod.%s.lengthscale" % st]).min()) for h in hyp)
    om["l_min"] = l_min
    return om


def width_gp(prob):
    """SimpleGPModel(n_out, D - 1, 1) of a width_problem, trained without hyper-parameter optimisation."""
    from safe_exploration_amd import SimpleGPModel
    n_out, D = len(prob["kts"]), prob["Z"].shape[1]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=prob["kts"],
                       hyp=[dict(h, noise_variance=nv) for h, nv in zip(prob["hyp"], prob["noise"])])
    gp.train(prob["Z"], prob["Y"], opt_hyp=False)
    return gp


def width_queries(prob, T, seed):
    """T queries, alternately near a training point (a step of r ~ U[0.05, 0.5] typical lengthscales sqrt(D / 3) in a
    random direction: the posterior variance well below the prior even with one training point) and just outside the
    data (x ~ U[-1,1]^D with x_1 = +-U[1.1, 2]; not for one or a few training points: inside a dense cloud of points d var / dx is ~0, and the product part of
    lin_rbf / lin_mat52 acts on x_1 alone)."""
    rng = np.random.default_rng(seed)
    Z = prob["Z"]
    D = Z.shape[1]
    step = rng.uniform(0.05, 0.5, (T, 1)) * np.sqrt(D / 3.0) / np.sqrt(D)
    x = Z[rng.integers(0, Z.shape[0], T)] + step * rng.standard_normal((T, D))
    out = rng.uniform(-1, 1, (T, D))
    out[:, 1] = rng.choice((-1.0, 1.0), T) * rng.uniform(1.1, 2.0, T)
    if Z.shape[0] >= 8:
        x[1::2] = out[1::2]
    return x
