"""Monte-Carlo rollouts through ONE plausible system per particle: posterior function samples by pathwise conditioning
(SimpleGPModel.draw_paths, sample_n_step(consistent=True)) against the marginal draws of sample_from_gp, where a
particle meets an unrelated dynamics function at every step.

    python examples/consistent_rollouts.py

Needs a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification     # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n_s, n_u, N, n, S = 2, 1, 150, 8, 2000
    Z = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.8 * Z[:, :n_s] + 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((n_s + n_u, n_s)))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.array([0.7, 0.9, 1.1]), "variance": 0.5, "noise_variance": 1e-3} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)

    # S whole functions; the values of one path at several inputs belong to one function
    gp.draw_paths(S, n_features=1024)
    x = np.array([[1.5, 1.5, 0.0], [1.5, 1.5, 0.01], [-1.5, 0.5, 0.0]])      # two neighbours away from the data, one far off
    F = gp.sample_paths(x)                                                  # (3, S, n_s)
    M = gp.sample_from_gp(x, size=S)                                        # marginal draws: independent per input
    print("paths %s: corr(f(x0), f(x1)) = %.3f   corr(f(x0), f(x2)) = %.3f"
          % (F.shape, np.corrcoef(F[0, :, 0], F[1, :, 0])[0, 1], np.corrcoef(F[0, :, 0], F[2, :, 0])[0, 1]))
    print("marginal draws: corr(f(x0), f(x1)) = %.3f" % np.corrcoef(M[0, :, 0], M[1, :, 0])[0, 1])
    mu, var = gp.predict(x)
    print("mean of the paths", F.mean(1)[0], "posterior mean", mu[0], "| variance", F.var(1)[0], "posterior variance", var[0])

    K = np.tile(-0.2 * np.ones((1, n_u, n_s)), (n, 1, 1))
    k = np.zeros((n, n_u))
    x0 = np.array([[0.4], [-0.3]])
    mc = MonteCarloSafetyVerification(gp)
    _, consistent = mc.sample_n_step(x0, K, k, n=n, n_samples=S, consistent=True)     # uses the S paths drawn above
    _, marginal = mc.sample_n_step(x0, K, k, n=n, n_samples=S)
    _, fused = mc.rollout_paths(x0, K, k, n=n, n_samples=S)                           # the same roll-out in one launch
    print("one launch against the chained steps: max difference %.2e" % np.abs(fused - consistent).max())
    print("\nstep  spread of the particles (trace of their covariance): consistent | marginal")
    for i in range(n):
        print("%4d  %.5f | %.5f" % (i, np.trace(np.cov(consistent[i].T)), np.trace(np.cov(marginal[i].T))))

    # the same with the reference's "lin_rbf" kernel on the second state (linear x RBF on input dimension 1 + ARD linear): a
    # model of the general kernel family, whose prior sample is a sum over products of features (G M + D weights per path)
    hyp[1] = {"prod.rbf.lengthscale": 0.9, "prod.rbf.variance": 0.5, "prod.linear.variances": 1.0,
              "linear.variances": np.array([0.3, 0.6, 0.1]), "noise_variance": 1e-3}
    gl = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf", "lin_rbf"], hyp=hyp)
    gl.train(Z, Y, opt_hyp=False)
    print("\nrbf / lin_rbf model: %d weights per path for 1024 features" % gl.paths_weight_count(1024))
    ml = MonteCarloSafetyVerification(gl)
    _, consistent, A = ml.sample_n_step_jacobians(x0, K, k, n=n, n_samples=S)           # draws the paths itself
    _, marginal = ml.sample_n_step(x0, K, k, n=n, n_samples=S)
    _, chained = ml.rollout_paths(x0, K, k, n=n, n_samples=S)                           # no one-launch form: the chained steps
    print("rollout_paths on the family: max difference to the chained steps %.1e" % np.abs(chained - consistent).max())
    print("step  spread: consistent | marginal      mean |d x_(i+1) / d x_i| over the particles")
    for i in range(n):
        print("%4d  %.5f | %.5f      %.3f" % (i, np.trace(np.cov(consistent[i].T)), np.trace(np.cov(marginal[i].T)),
                                             np.abs(A[i]).mean()))


if __name__ == "__main__":
    main()
