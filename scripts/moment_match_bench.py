"""Time per call of sr_gp_moment_match against the same formulas in batched torch fp64 (the expanded form, chunked to fit
memory) at the shapes of profiles/r10_moment_match.txt.  Device events, warmed up.

    python scripts/moment_match_bench.py [OUTPUT_FILE]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_exploration_amd import SimpleGPModel

def torch_mm(Z, alpha, Kinv, ls, sf2, m, S, budget=2 ** 27):
    n, D = ls.shape; N = Z.shape[0]; T = m.shape[0]
    Tc = max(1, min(T, budget // (N * N)))
    eye = torch.eye(D, dtype=torch.float64, device=Z.device)
    mu = torch.empty((T, n), dtype=torch.float64, device=Z.device); cov = torch.empty((T, n, n), dtype=torch.float64, device=Z.device)
    V = torch.empty((T, n, D), dtype=torch.float64, device=Z.device)
    for t0 in range(0, T, Tc):
        mm, SS = m[t0:t0 + Tc], S[t0:t0 + Tc]
        nu = Z[None] - mm[:, None, :]                                   # (Tc, N, D)
        for a in range(n):
            r = 1.0 / ls[a]
            C = eye + r[None, :, None] * SS * r[None, None, :]
            Lc = torch.linalg.cholesky(C)
            W = torch.linalg.solve_triangular(Lc, torch.diag(r).expand(len(mm), D, D), upper=False)
            y = nu.matmul(W.transpose(1, 2))
            q = alpha[a][None] * torch.exp(torch.log(sf2[a]) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1)[:, None] - 0.5 * (y * y).sum(2))
            mu[t0:t0 + Tc, a] = q.sum(1)
            g = (q[:, :, None] * nu).sum(1)
            V[t0:t0 + Tc, a] = W.transpose(1, 2).matmul(W.matmul(g[:, :, None])).squeeze(2)
        for a in range(n):
            for b in range(a, n):
                la, lb = 1 / ls[a] ** 2, 1 / ls[b] ** 2
                r = torch.sqrt(la + lb)
                Bm = r[None, :, None] * SS * r[None, None, :]
                C = eye + Bm
                X = torch.linalg.solve(C, Bm)
                Mm = 0.5 * (X + X.transpose(1, 2)) / (r[:, None] * r[None, :])
                P = lb[None, :, None] * Mm * la[None, None, :]
                Ga = torch.diag(la) - la[None, :, None] * Mm * la[None, None, :]
                Gb = torch.diag(lb) - lb[None, :, None] * Mm * lb[None, None, :]
                c = torch.log(sf2[a] * sf2[b]) - 0.5 * torch.linalg.slogdet(C)[1]
                u = nu.matmul(P.transpose(1, 2))
                si = c[:, None] - 0.5 * (nu.matmul(Ga) * nu).sum(2)
                sj = -0.5 * (nu.matmul(Gb) * nu).sum(2)
                Q = torch.exp(u.matmul(nu.transpose(1, 2)) + si[:, :, None] + sj[:, None, :])
                s = torch.einsum("ti,tij,tj->t", alpha[a][None].expand(len(mm), N), Q, alpha[b][None].expand(len(mm), N))
                if a == b:
                    s = s - (Q * Kinv[a][None]).sum((1, 2)) + sf2[a]
                v = s - mu[t0:t0 + Tc, a] * mu[t0:t0 + Tc, b]
                cov[t0:t0 + Tc, a, b] = v; cov[t0:t0 + Tc, b, a] = v
    return mu, cov, V

def timed(fn, warm, reps):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps

out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


dev = torch.device("cuda", 0)
for N, n_out, D, T, reps, treps in ((150, 4, 5, 256, 20, 3), (150, 4, 5, 3840, 5, 2), (1000, 2, 3, 1024, 3, 1), (5000, 2, 3, 64, 3, 1)):
    rng = np.random.default_rng(N + T)
    Zh = rng.uniform(-1, 1, (N, D)); Yh = np.sin(2 * Zh.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    hyp = [{"lengthscale": rng.uniform(0.6, 1.4, D) * np.sqrt(D / 3.0), "variance": 1.0, "noise_variance": 1e-2} for _ in range(n_out)]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp, device=dev)
    gp.train(Zh, Yh, opt_hyp=False)
    m = torch.as_tensor(Zh[rng.integers(0, N, T)] + 0.2 * rng.standard_normal((T, D)), device=dev)
    g = torch.as_tensor(0.25 * rng.standard_normal((T, D, 2)) / np.sqrt(D), device=dev)
    S = g.matmul(g.transpose(1, 2))
    gp.inv_K_device(); torch.cuda.synchronize()
    ms = timed(lambda: gp.moment_match_device(m, S), 2, reps)
    Z, alpha, Kinv = torch.as_tensor(Zh, device=dev), gp.export_alpha(), gp.inv_K_device()
    ls = torch.as_tensor(np.stack([h["lengthscale"] for h in hyp]), device=dev); sf2 = torch.ones(n_out, dtype=torch.float64, device=dev)
    ref = torch_mm(Z, alpha, Kinv, ls, sf2, m, S)
    got = gp.moment_match_device(m, S)
    diffs = [float((x - y).abs().max()) for x, y in zip(got, ref)]
    tms = timed(lambda: torch_mm(Z, alpha, Kinv, ls, sf2, m, S), 1, treps)
    pairs = n_out * (n_out + 1) // 2
    evals = T * pairs * N * N
    say("N=%d n_out=%d D=%d T=%d: kernel %.3f ms, torch %.3f ms (x%.1f); %.3g pair evaluations/s (all T pairs N^2); max|kernel - torch| mu %.1e cov %.1e V %.1e"
        % (N, n_out, D, T, ms, tms, tms / ms, evals / (ms * 1e-3), diffs[0], diffs[1], diffs[2]))
