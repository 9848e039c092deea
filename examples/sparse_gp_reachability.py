"""Sparse GP regression on the device: m = 256 inducing inputs summarise N = 200000 observed transitions
(``do_sparse_gp = True`` -> sr_gp_fit_sparse), then a batch of one-step reachability queries runs on the sparse model
exactly as on an exact one.

    python examples/sparse_gp_reachability.py
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_exploration_amd import SimpleGPModel, gp_reachability as reach  # noqa: E402


def main():
    n_s, n_u, N, m, T = 2, 1, 200000, 256, 4096
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.1 * np.sin(X @ rng.uniform(0.5, 1.5, (n_s + n_u, n_s))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.full(n_s + n_u, 0.5), "variance": 0.01, "noise_variance": 1e-4} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.do_sparse_gp = True
    t0 = time.perf_counter()
    gp.train(X, Y, m, opt_hyp=False, Z=X[rng.choice(N, m, replace=False)])
    print("sparse fit: N = %d rows, m = %d inducing inputs, %.1f ms (beta %s, inv_K %d x %s)"
          % (N, m, 1e3 * (time.perf_counter() - t0), gp.beta.shape, len(gp.inv_K), gp.inv_K[0].shape))
    p = rng.uniform(-0.5, 0.5, (T, n_s))
    q = np.tile(0.01 * np.eye(n_s), (T, 1, 1))
    k_ff = rng.uniform(-0.5, 0.5, (T, n_u))
    k_fb = 0.1 * rng.standard_normal((T, n_u, n_s))
    l = np.array([0.05, 0.02])
    p1, q1 = reach.onestep_reachability_batch(p, gp, k_ff, l, l, q, k_fb, 2.0)
    print("one-step reachability of %d ellipsoids: centres %s, shape matrices %s, largest semi-axis %.3e"
          % (T, p1.shape, q1.shape, float(np.sqrt(np.linalg.eigvalsh(q1).max()))))


if __name__ == "__main__":
    main()
