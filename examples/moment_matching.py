"""Exact moment matching through a GP dynamics model: a Gaussian state pushed through H steps of
x+ = a x + b (K x + k_ff) + g([x; u]), against the two approximations (first-order Taylor, mean-equivalent).

    python examples/moment_matching.py

Needs a GPU: the GP is evaluated by sr_gp_moment_match (mean, FULL output covariance and expected Jacobian in closed form), for
an ARD-RBF model and for a "lin_rbf" model."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as up             # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n_s, n_u, N, H, T = 2, 1, 150, 6, 4
    Z = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((n_s + n_u, n_s)))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.full(n_s + n_u, 0.8), "variance": 0.05, "noise_variance": 1e-4} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)

    # one Gaussian input: mean, full covariance across the outputs, expected Jacobian
    mu, cov, V = gp.predict_uncertain([0.1, -0.2, 0.05], np.diag([0.02, 0.01, 0.0]))
    print("E[g] =", mu[0], "\nCov[g] =\n", cov[0], "\nV (cov(z, g) = S V^T) =\n", V[0])

    a, b = 0.9 * np.eye(n_s), np.array([[0.0], [0.3]])
    k_ff = 0.1 * rng.standard_normal((H, n_u))
    k_fb = [-0.3 * np.ones((n_u, n_s)) for _ in range(H - 1)]
    mu_0, sigma_0 = np.array([[0.2], [-0.1]]), np.diag([0.01, 0.02])
    mm_mu, mm_sigma, _ = up.multi_step_moment_matching(mu_0, gp, k_ff, k_fb, sigma_0, a, b)
    ty_mu, ty_sigma, _ = up.multi_step_taylor(mu_0, gp, k_ff, k_fb, None, a, b)
    print("\nstep  trace Sigma (moment matching from sigma_0)   trace Sigma (Taylor from a point)")
    for i in range(H):
        print("%4d  %.6f  %36.6f" % (i, np.trace(mm_sigma[i].reshape(n_s, n_s)), np.trace(ty_sigma[i].reshape(n_s, n_s))))

    # T roll-outs at once, device tensors in and out, no host synchronisation between the steps
    import torch
    dev = gp.device
    mu_all, sigma_all, cov_all = up.moment_matching_batch(
        torch.as_tensor(0.2 * rng.standard_normal((T, n_s)), device=dev), gp,
        torch.as_tensor(0.1 * rng.standard_normal((T, H, n_u)), device=dev),
        torch.as_tensor(-0.3 * np.ones((T, H - 1, n_u, n_s)), device=dev), a, b,
        sigma_0=torch.as_tensor(np.tile(sigma_0, (T, 1, 1)), device=dev))
    print("\nbatch:", tuple(mu_all.shape), tuple(sigma_all.shape), tuple(cov_all.shape))

    # the roll-out in ONE launch (sr_gp_moment_match_rollout): a workgroup owns a trajectory for the whole horizon.  The same
    # arguments and results as moment_matching_batch, equal to rounding; outside the kernel's domain (a lin_rbf model, N > 1024)
    # the call goes through moment_matching_batch
    mu0 = 0.2 * rng.standard_normal((T, n_s))
    kff_T, kfb_T = 0.1 * rng.standard_normal((T, H, n_u)), -0.3 * np.ones((T, H - 1, n_u, n_s))
    s0_T = np.tile(sigma_0, (T, 1, 1))
    fused = up.moment_matching_rollout_batch(mu0, gp, kff_T, kfb_T, a, b, sigma_0=s0_T)
    chained = up.moment_matching_batch(mu0, gp, kff_T, kfb_T, a, b, sigma_0=s0_T)
    print("roll-out in one launch against the per-step route: max |difference| of (mu_all, sigma_all, gp_cov_all) =",
          ["%.1e" % np.abs(x - y).max() for x, y in zip(fused, chained)])
    # on device tensors, one policy for all trajectories, without the GP's output covariances
    mu_d, sigma_d, _ = gp.moment_match_rollout_device(torch.as_tensor(mu0, device=dev), k_ff, np.stack(k_fb), a, b,
                                                      sigma0=s0_T, with_cov=False)
    print("shared policy:", tuple(mu_d.shape), tuple(sigma_d.shape), " trace Sigma_H of trajectory 0 = %.6f"
          % float(torch.trace(sigma_d[0, -1])))

    # the same roll-out with the reference's "lin_rbf" kernel (linear x RBF on input dimension 1 + ARD linear): a near-linear
    # plant, whose linear part the kernel carries; the closed form exists for it too (a Matern kernel has none)
    Yl = Y + Z.dot(np.array([[0.1, 0.0], [0.0, 0.1], [0.05, -0.05]]))
    hyp_l = [{"prod.rbf.lengthscale": 0.8, "prod.rbf.variance": 0.05, "prod.linear.variances": 1.0,
              "linear.variances": np.full(n_s + n_u, 0.02), "noise_variance": 1e-4} for _ in range(n_s)]
    gp_l = SimpleGPModel(n_s, n_s, n_u, kern_types=["lin_rbf"] * n_s, hyp=hyp_l)
    gp_l.train(Z, Yl, opt_hyp=False)
    ml_mu, ml_sigma, _ = up.multi_step_moment_matching(mu_0, gp_l, k_ff, k_fb, sigma_0, a, b)
    print("\nlin_rbf model:  step  mean                      trace Sigma")
    for i in range(H):
        print("%20d  %-24s  %.6f" % (i, np.array2string(ml_mu[i], precision=4), np.trace(ml_sigma[i].reshape(n_s, n_s))))


if __name__ == "__main__":
    main()
