"""Exploration with a bounded model: every step appends one observed transition and, once the budget is reached,
retires one row -- no refit on the way (exploration_runner.py:186-189 appends without a bound).

    python examples/bounded_exploration.py

Needs a GPU: the append is sr_gp_append1_host, the retire sr_gp_remove, the redundancy score comes from sr_gp_loo."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402


def main():
    rng = np.random.default_rng(0)
    n_s, n_u, budget, steps = 2, 1, 200, 300
    w = rng.standard_normal((n_s + n_u, n_s))

    def system(z):
        return 0.2 * np.sin(2.0 * z.dot(w)) + 0.01 * rng.standard_normal((z.shape[0], n_s))

    hyp = [{"lengthscale": np.full(n_s + n_u, 0.8), "variance": 0.05, "noise_variance": 1e-4} for _ in range(n_s)]
    for rule in ("oldest", "redundant"):
        Z = rng.uniform(-1, 1, (20, n_s + n_u))
        gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
        gp.train(Z, system(Z), opt_hyp=False)
        test = rng.uniform(-1, 1, (256, n_s + n_u))
        for t in range(steps):
            # the most uncertain of a few candidates is visited, observed and appended; n_max keeps the model at its budget
            cand = rng.uniform(-1, 1, (32, n_s + n_u))
            z = cand[np.argmax(gp.predict(cand)[1].sum(axis=1))][None, :]
            gp.update_model(z, system(z), opt_hyp=False, replace_old=False, n_max=budget, retire=rule)
        mu_loo, var_loo = gp.loo()
        print("retire=%-9s  N = %d  mean predictive variance %.3e  mean |y - mu_loo| %.3e"
              % (rule, gp.x_train.shape[0], gp.predict(test)[1].mean(), np.abs(gp.y_train - mu_loo).mean()))


if __name__ == "__main__":
    main()
