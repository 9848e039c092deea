"""Bit check of the ARD-RBF route of the posterior function samples between two builds: every paths call -- draw, _eval,
_eval_grad, _step, _step_grad with and without the closed loop, sr_gp_paths_rollout with A_all, sr_gp_paths_rollout_vjp with
J_all, sample_n_step(consistent=True), sample_n_step_jacobians, rollout_paths -- on "rbf" models at three sizes, seeded inputs.

    python scripts/paths_ard_bitcheck.py <root of a built checkout> out.npz        (once per checkout, one process each)
    python scripts/paths_ard_bitcheck.py --compare a.npz b.npz                     (array_equal on every array; exit 1 if not)

Needs a GPU for the first form."""
import os
import sys

import numpy as np
if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if not np.array_equal(a[k], b[k])]
    print("ARD handles, parent library against this one: %d arrays, array_equal on %s" % (len(a.files), "ALL" if not bad else "all but " + str(bad)))
    sys.exit(1 if bad else 0)
root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import torch
from safe_exploration_amd import SimpleGPModel, _build
assert os.path.dirname(_build.LIB_PATH) == os.path.join(root, "safe_exploration_amd"), _build.LIB_PATH
from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
res = {}
for (N, n_out, D, S, M, T, chunk) in ((150, 4, 5, 300, 257, 200, None), (700, 2, 3, 129, 100, 300, 128), (64, 1, 8, 16, 16, 16, None)):
    rng = np.random.default_rng(N)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    hyp = [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": 1e-2} for d in range(n_out)]
    n_u = D - n_out if D > n_out else 1
    gp = SimpleGPModel(n_out, D - n_u, n_u, kern_types=["rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    if chunk:
        gp.set_chunk(chunk)
    gp.draw_paths(S, M, omega=rng.standard_normal((M, D)), tau=rng.uniform(0, 2 * np.pi, M), w=rng.standard_normal((n_out, S, M)),
                  eps=rng.standard_normal((n_out, S, N)))
    x, xs = rng.uniform(-1.2, 1.2, (T, D)), rng.uniform(-1.2, 1.2, (S, D))
    t = "N%d_" % N
    res[t + "F"] = gp.sample_paths(x)
    res[t + "Fg"], res[t + "J"] = gp.sample_paths(x, jacobians=True)
    res[t + "Fs"] = gp.paths_step_device(xs).cpu().numpy()
    fs, js = gp.paths_step_device(xs, jacobians=True)
    res[t + "Fsg"], res[t + "Js"] = fs.cpu().numpy(), js.cpu().numpy()
    if D > n_out:
        H = 4
        K, k = 0.3 * rng.standard_normal((H, n_u, n_out)), 0.1 * rng.standard_normal((H, n_u))
        fz, z = gp.paths_step_device(xs, K[0], k[0])
        res[t + "z"] = z.cpu().numpy()
        x0 = rng.uniform(-0.5, 0.5, n_out)
        X, A = gp.paths_rollout_device(x0, K, k, jacobians=True)
        res[t + "X"], res[t + "A"] = X.cpu().numpy(), A.cpu().numpy()
        Xb = torch.as_tensor(rng.standard_normal((H, S, n_out)), device=X.device)
        for name, v in zip(("x0b", "Kb", "kb", "Jall"), gp.paths_rollout_vjp_device(x0, K, k, X, Xb, jacobians=True)):
            res[t + name] = v.cpu().numpy()
        mc = MonteCarloSafetyVerification(gp)
        res[t + "mc"] = mc.sample_n_step(x0.reshape(-1, 1), K, k, n=H, n_samples=S, consistent=True, n_features=M)[1]
        res[t + "mcA"] = mc.sample_n_step_jacobians(x0.reshape(-1, 1), K, k, n=H, n_samples=S, n_features=M)[2]
        res[t + "mcr"] = mc.rollout_paths(x0.reshape(-1, 1), K, k, n=H, n_samples=S, n_features=M)[1]
np.savez(out, **res)
print("wrote", out, len(res), "arrays")
