"""Time per call of sr_gp_moment_match_vjp (the reverse pass) against sr_gp_moment_match (the forward) and against torch
autograd through the same closed form in batched torch fp64 (forward + backward, query chunks sized to keep one (Tc, N, N)
tensor below 1 GB, one backward per chunk), at the shapes of profiles/r14_moment_match_grad.txt.  Device events, warmed up;
forward and reverse alternate, three rounds each, all three times printed.

    python scripts/moment_match_grad_bench.py [OUTPUT_FILE]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_exploration_amd import SimpleGPModel


def torch_mm(Z, alpha, Kinv, ls, sf2, m, S):
    """the expanded closed form of one chunk of queries, differentiable in m and S -> mu (T,n), cov (T,n,n), V (T,n,D)"""
    n, D = ls.shape
    N, T = Z.shape[0], m.shape[0]
    eye = torch.eye(D, dtype=torch.float64, device=Z.device)
    nu = Z[None] - m[:, None, :]
    mu, V = [], []
    for a in range(n):
        r = 1.0 / ls[a]
        C = eye + r[None, :, None] * S * r[None, None, :]
        Lc = torch.linalg.cholesky(C)
        W = torch.linalg.solve_triangular(Lc, torch.diag(r).expand(T, D, D), upper=False)
        y = nu.matmul(W.transpose(1, 2))
        q = alpha[a][None] * torch.exp(torch.log(sf2[a]) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1)[:, None]
                                       - 0.5 * (y * y).sum(2))
        mu.append(q.sum(1))
        g = (q[:, :, None] * nu).sum(1)
        V.append(W.transpose(1, 2).matmul(W.matmul(g[:, :, None])).squeeze(2))
    rows = [[None] * n for _ in range(n)]
    for a in range(n):
        for b in range(a, n):
            la, lb = 1 / ls[a] ** 2, 1 / ls[b] ** 2
            r = torch.sqrt(la + lb)
            Bm = r[None, :, None] * S * r[None, None, :]
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
            s = torch.einsum("i,tij,j->t", alpha[a], Q, alpha[b])
            if a == b:
                s = s - (Q * Kinv[a][None]).sum((1, 2)) + sf2[a]
            rows[a][b] = rows[b][a] = s - mu[a] * mu[b]
    return torch.stack(mu, 1), torch.stack([torch.stack(r, 1) for r in rows], 1), torch.stack(V, 1)


def torch_vjp(Z, alpha, Kinv, ls, sf2, m, S, seeds, budget=2 ** 27):
    N, T = Z.shape[0], m.shape[0]
    Tc = max(1, min(T, budget // (N * N)))
    gm, gS = torch.empty_like(m), torch.empty_like(S)
    for t0 in range(0, T, Tc):
        mm, SS = m[t0:t0 + Tc].clone().requires_grad_(True), S[t0:t0 + Tc].clone().requires_grad_(True)
        outs = torch_mm(Z, alpha, Kinv, ls, sf2, mm, 0.5 * (SS + SS.transpose(1, 2)))
        L = sum((w[t0:t0 + Tc] * o).sum() for w, o in zip(seeds, outs))
        gm[t0:t0 + Tc], gS[t0:t0 + Tc] = torch.autograd.grad(L, (mm, SS))
    return gm, gS


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


dev = torch.device("cuda", 0)
for N, n_out, D, T, reps, treps in ((150, 4, 5, 256, 200, 3), (150, 4, 5, 3840, 40, 2), (5000, 2, 3, 64, 10, 1)):
    rng = np.random.default_rng(N + T)
    Zh = rng.uniform(-1, 1, (N, D))
    Yh = np.sin(2 * Zh.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    hyp = [{"lengthscale": rng.uniform(0.6, 1.4, D) * np.sqrt(D / 3.0), "variance": 1.0, "noise_variance": 1e-2}
           for _ in range(n_out)]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp, device=dev)
    gp.train(Zh, Yh, opt_hyp=False)
    m = torch.as_tensor(Zh[rng.integers(0, N, T)] + 0.2 * rng.standard_normal((T, D)), device=dev)
    g = torch.as_tensor(0.25 * rng.standard_normal((T, D, 2)) / np.sqrt(D), device=dev)
    S = g.matmul(g.transpose(1, 2))
    seeds = [torch.as_tensor(rng.standard_normal(shp), device=dev) for shp in ((T, n_out), (T, n_out, n_out), (T, n_out, D))]
    gp.inv_K_device()
    torch.cuda.synchronize()
    fwd, rev = [], []
    for _ in range(3):
        fwd.append(timed(lambda: gp.moment_match_device(m, S), 2, reps))
        rev.append(timed(lambda: gp.moment_match_vjp_device(m, S, *seeds), 2, reps))
    Z, alpha, Kinv = torch.as_tensor(Zh, device=dev), gp.export_alpha(), gp.inv_K_device()
    ls = torch.as_tensor(np.stack([h["lengthscale"] for h in hyp]), device=dev)
    sf2 = torch.ones(n_out, dtype=torch.float64, device=dev)
    ref = torch_vjp(Z, alpha, Kinv, ls, sf2, m, S, seeds)
    got = gp.moment_match_vjp_device(m, S, *seeds)
    diffs = [float((x - y).abs().max()) for x, y in zip(got, ref)]
    tms = timed(lambda: torch_vjp(Z, alpha, Kinv, ls, sf2, m, S, seeds), 1, treps)
    say("N=%d n_out=%d D=%d T=%d: forward %s ms, reverse %s ms (x%.2f of the forward, medians), torch forward + backward %.3f ms "
        "(x%.1f of the reverse); max|kernel - torch| m_bar %.1e S_bar %.1e"
        % (N, n_out, D, T, " / ".join("%.3f" % x for x in fwd), " / ".join("%.3f" % x for x in rev),
           sorted(rev)[1] / sorted(fwd)[1], tms, tms / sorted(rev)[1], diffs[0], diffs[1]))
