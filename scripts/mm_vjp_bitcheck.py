"""Bit check of sr_gp_moment_match_vjp between two builds: m_bar and S_bar on fixed inputs, hashed.  The split of its launch
sequence into a seed-independent and a seed-dependent half (for sr_gp_moment_match_rollout_vjp) must not change a bit.

    python scripts/mm_vjp_bitcheck.py <root of a built checkout>        (once per checkout, one process each)

Three shapes (D, N, n_out) = (3, 70, 1), (5, 300, 4), (12, 70, 4); T = 37 queries with S of full rank, of rank 1 and None, seeds
on all three outputs, and a second run at chunk 16.  Prints one sha256 per array; equal lines = equal bits.  Needs a GPU."""
import hashlib
import os
import sys

import numpy as np

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
from safe_exploration_amd import SimpleGPModel, _build                              # noqa: E402
assert os.path.dirname(_build.LIB_PATH) == os.path.join(root, "safe_exploration_amd"), _build.LIB_PATH

for D, N, n_out in ((3, 70, 1), (5, 300, 4), (12, 70, 4)):
    rng = np.random.default_rng(1000 * D + N)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    hyp = [{"lengthscale": rng.uniform(0.5, 1.0, D) * np.sqrt(D / 3.0), "variance": float(rng.uniform(0.8, 1.2)),
            "noise_variance": 1e-2} for _ in range(n_out)]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    T = 37
    m = 0.3 * rng.standard_normal((T, D))
    g = 0.25 * rng.standard_normal((T, D, D)) / np.sqrt(D)
    seeds = rng.standard_normal((T, n_out)), rng.standard_normal((T, n_out, n_out)), rng.standard_normal((T, n_out, D))
    for kind, S in (("full", np.matmul(g, np.transpose(g, (0, 2, 1)))), ("rank1", np.matmul(g[:, :, :1], np.transpose(g[:, :, :1], (0, 2, 1)))),
                    ("point", None)):
        for chunk in (65536, 16):
            gp.set_chunk(chunk)
            m_bar, S_bar = gp.predict_uncertain_vjp(m, S, *seeds)
            for what, x in (("m_bar", m_bar), ("S_bar", S_bar)):
                print("D=%d N=%d n_out=%d S=%s chunk=%d %s %s" % (D, N, n_out, kind, chunk, what,
                                                                 hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()[:32]))
