"""How a consistent Monte-Carlo rollout reacts to its start state: every particle is rolled through ITS OWN posterior function
(SimpleGPModel.draw_paths), sample_n_step_jacobians returns the closed-loop transition Jacobian of
every step and particle, and their ordered product is d x_n / d x_0 -- checked here against central differences of the
rollout itself (2 n_s further rollouts, which the Jacobians replace).

    python examples/path_sensitivities.py

Needs a GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification     # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n_s, n_u, N, n, S = 2, 1, 150, 6, 1000
    Z = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.8 * Z[:, :n_s] + 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((n_s + n_u, n_s)))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.array([0.7, 0.9, 1.1]), "variance": 0.5, "noise_variance": 1e-3} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    gp.draw_paths(S, n_features=1024)

    # one sampled function and its Jacobian at a few inputs
    x = rng.uniform(-1, 1, (4, n_s + n_u))
    F, J = gp.sample_paths(x, jacobians=True)                              # (4, S, n_s), (4, S, n_s, n_s + n_u)
    print("values", F.shape, "Jacobians", J.shape, "| spread of d f_0 / d x_0 over the paths at x[0]: %.3f +- %.3f"
          % (J[0, :, 0, 0].mean(), J[0, :, 0, 0].std()))

    K = np.tile(-0.2 * np.ones((1, n_u, n_s)), (n, 1, 1))
    k = np.zeros((n, n_u))
    x0 = np.array([[0.4], [-0.3]])
    mc = MonteCarloSafetyVerification(gp)
    _, X, A = mc.sample_n_step_jacobians(x0, K, k, n=n, n_samples=S)      # uses the S paths drawn above
    P = np.tile(np.eye(n_s), (S, 1, 1))
    for i in range(n):
        P = A[i] @ P                                                       # d x_{i+1} / d x_0 of every particle
    h = 1e-5
    fd = np.empty_like(P)
    for j in range(n_s):
        e = np.zeros((n_s, 1))
        e[j] = h
        fd[:, :, j] = (mc.sample_n_step(x0 + e, K, k, n=n, n_samples=S, consistent=True)[1][n - 1]
                       - mc.sample_n_step(x0 - e, K, k, n=n, n_samples=S, consistent=True)[1][n - 1]) / (2 * h)
    print("d x_%d / d x_0, mean over the particles:\n%s\nspread over the particles (std):\n%s" % (n, P.mean(0), P.std(0)))
    print("largest difference to central differences of the rollout: %.2e" % np.abs(P - fd).max())


if __name__ == "__main__":
    main()
