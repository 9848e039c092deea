"""The inputs of the fused moment-matching roll-out's tests (sr_gp_moment_match_rollout) -- TEST infrastructure, shared by
tests/test_gpu_moment_match_rollout.py (the kernel against the references) and tests/test_moment_match_rollout_host.py (the two
references against each other, on the CPU, on the same inputs).

A case is a dict: the data Z (N, D), Y (N, n_s) and the hyper-parameters of an ARD-RBF model (the generator of
tests/test_gpu_moment_match.py), the linear part a (n_s, n_s), b (n_s, n_u), a_gp_inp_x ``tz`` (n_x_in, n_s) or None, the
starts mu0 (T, n_s), sigma0 (T, n_s, n_s) or None, and the gains k_ff ([T,] H, n_u), k_fb ([T,] H-1, n_u, n_s) -- per
trajectory or one policy for all (``per_traj``).

The bars are the project's (tests/test_gpu_moment_match.py): end to end rtol 1e-8, atol 1e-12; a step at the kernel's own
previous state mu+ rtol 1e-10 + 1e-12 sigma_f |alpha|_1, Sigma+ and Cov rtol 1e-8 + 1e-9 max sf2."""
import numpy as np

from test_gpu_moment_match import _problem, _seed

IT, JT, N_MAX = 64, 256, 1024                     # the kernel's tiles (rows i per tile, rows j per staged tile), its largest model

# name -> (N, n_s, n_u, tz_rows | None, H, T, sigma0 kind, per_traj, noise, end_to_end)
SPECS = {}
# every width bucket, D < DT and D == DT: D = 2, 3, 4 | 5, 8 | 9, 12
WIDTHS = {2: (1, 1, None), 3: (2, 1, None), 4: (3, 2, 2), 5: (4, 1, None), 8: (4, 4, None), 9: (4, 5, None), 12: (5, 8, 4)}
for _D, (_ns, _nu, _tz) in WIDTHS.items():
    SPECS["width-%d" % _D] = (70, _ns, _nu, _tz, 3, 2, "full", True, 1e-2, True)
# size edges: one and two rows, either side of the i tile and of the j tile (one past the largest tile: 257), the largest model
SIZES = (1, 2, IT - 1, IT, IT + 1, JT - 1, JT, JT + 1, N_MAX)
for _N in SIZES:
    SPECS["size-%d" % _N] = (_N, 2, 1, None, 2, 1 if _N == N_MAX else 2, "full", True, 1e-2, False)
# a model too large for the kernel to keep Z and alpha in LDS beside its tiles (N (D + n_s) doubles: 38 KB here): it reads them
# through the caches (at D = 12 with five outputs, width-12, the step's records do not fit either and go to the scratch)
SPECS["model-from-global"] = (700, 2, 3, None, 2, 1, "full", True, 1e-2, False)
# starts and gains.  At noise 1e-2 the two CPU references disagree end to end by up to 0.39 of the bar on these models and on the
# cart-pole shape (|alpha|_1 grows as 1 / noise and the mean's atol is 1e-12): they have noise 5e-2, where it is at most 0.02
NOISE = 5e-2
for _kind in ("point", "rank1", "full"):
    for _per in (False, True):
        SPECS["start-%s-%s" % (_kind, "own" if _per else "shared")] = (80, 3, 1, None, 4, 3, _kind, _per, NOISE, True)
SPECS["tz-hidden"] = (80, 3, 1, 2, 4, 3, "full", True, NOISE, True)
SPECS["tz-hidden-point"] = (80, 3, 1, 2, 4, 3, "point", False, NOISE, True)
SPECS["h1-point"] = (80, 3, 1, None, 1, 3, "point", True, NOISE, True)
SPECS["h1-full"] = (80, 3, 1, None, 1, 3, "full", False, NOISE, True)
SPECS["nout-1"] = (80, 1, 2, None, 4, 3, "full", True, NOISE, True)
SPECS["nout-4"] = (80, 4, 1, None, 4, 3, "rank1", True, NOISE, True)
# the cart-pole shape
SPECS["cartpole"] = (150, 4, 1, None, 15, 4, "full", True, NOISE, True)
# the bitwise properties: the same shape, 8 trajectories
SPECS["cartpole-8"] = (150, 4, 1, None, 15, 8, "full", True, NOISE, False)
# the inducing rows of the sparse model (m = 32 of N = 200; the GPU test fits the sparse model on `X`, `Yx`)
SPECS["sparse"] = (32, 2, 1, None, 4, 3, "full", True, NOISE, True)
SPARSE_N = 200


def build(name):
    N, n_s, n_u, tz_rows, H, T, kind, per_traj, noise, e2e = SPECS[name]
    D = (n_s if tz_rows is None else tz_rows) + n_u
    n_data = SPARSE_N if name == "sparse" else N
    X, Yx, hyp = _problem(_seed("mmr", name), n_data, D, n_s, noise=noise)
    rng = np.random.default_rng(_seed("mmr-c", name))
    c = dict(name=name, N=N, n_s=n_s, n_u=n_u, D=D, H=H, T=T, kind=kind, per_traj=per_traj, noise=noise, e2e=e2e,
             X=X, Yx=Yx, Z=X[:N], Y=Yx[:N], hyp=hyp)
    c["a"] = 0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s))
    c["b"] = 0.3 * rng.standard_normal((n_s, n_u))
    c["tz"] = None if tz_rows is None else np.eye(n_s)[n_s - tz_rows:]             # the GP does not see the first state(s)
    c["mu0"] = 0.3 * rng.standard_normal((T, n_s))
    lead = (T,) if per_traj else ()
    c["k_ff"] = 0.2 * rng.standard_normal(lead + (H, n_u))
    c["k_fb"] = 0.4 * rng.standard_normal(lead + (H - 1, n_u, n_s)) if H > 1 else None
    if kind == "point":
        c["sigma0"] = None
    else:
        L = 0.15 * rng.standard_normal((T, n_s, 1 if kind == "rank1" else n_s))
        c["sigma0"] = np.matmul(L, np.transpose(L, (0, 2, 1)))
    return c


def gains(c, t):
    """k_ff (H, n_u) and k_fb (H-1, n_u, n_s) | None of trajectory t"""
    if c["per_traj"]:
        return c["k_ff"][t], None if c["k_fb"] is None else c["k_fb"][t]
    return c["k_ff"], c["k_fb"]


def tz_of(c):
    return np.eye(c["n_s"]) if c["tz"] is None else c["tz"]


def host_arrays(c):
    """(Z, alpha, M, ls, sf2) of the exact GP on the case's rows, fitted in NumPy (the GPU test takes the device's own)"""
    Z, Y = c["Z"], c["Y"]
    ls = np.stack([np.asarray(h["lengthscale"], float) for h in c["hyp"]])
    sf2 = np.array([float(h["variance"]) for h in c["hyp"]])
    alpha, M = np.empty((c["n_s"], c["N"])), np.empty((c["n_s"], c["N"], c["N"]))
    for o in range(c["n_s"]):
        d = (Z[:, None, :] - Z[None, :, :]) / ls[o][None, None, :]
        K = sf2[o] * np.exp(-0.5 * np.sum(d * d, axis=2)) + c["noise"] * np.eye(c["N"])
        M[o] = np.linalg.inv(K)
        M[o] = 0.5 * (M[o] + M[o].T)
        alpha[o] = np.linalg.solve(K, Y[:, o])
    return Z, alpha, M, ls, sf2


def e2e_bar(ref):
    return 1e-8 * np.abs(ref) + 1e-12


def step_bars(arrs, ref_mu, ref_mat):
    """the absolute bars of mu+ and of Sigma+ / Cov at the references' values"""
    _, alpha, _, _, sf2 = arrs
    return (1e-10 * np.abs(ref_mu) + 1e-12 * float(np.sqrt(sf2.max()) * np.abs(alpha).sum(1).max()),
            1e-8 * np.abs(ref_mat) + 1e-9 * float(sf2.max()))
