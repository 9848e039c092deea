"""Times of the reverse pass of one Taylor / mean-equivalent moment step (sr_onestep_moments_vjp), per mode and start, each beside
(a) the forward call (sr_onestep_moments), (b) the two GP derivative calls it runs one of (sr_gp_predict_grad,
sr_gp_linearize_batch) on the whole batch, (c) torch autograd through a batched torch-fp64 port of the step fed by
linearize_device_batch (the GP enters the port by its second-order expansion at z, so autograd returns the same gradient).

    python scripts/moments_grad_bench.py [OUT]        (default OUT: profiles/r16_moments_grad.txt)

One run measures every side; times are medians of five batches (scripts/_timing.timeit)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from _timing import timeit                                                         # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop           # noqa: E402
from reach_grad_bench import model                                                 # noqa: E402


def torch_step(p, q, u, k, lin, z0, a, b, mode):
    """the moment step of T queries in batched torch; the GP by its expansion (mu, var, jac_mu, jac_var, hess_mu) at z0"""
    mu0, var0, jm, jv, hm = lin
    n_s = p.shape[1]
    dz = torch.cat((p, u), dim=1) - z0
    mu = mu0 + torch.einsum('tad,td->ta', jm, dz)
    var = var0 + torch.einsum('tad,td->ta', jv, dz)
    p1 = p @ a.T + u @ b.T + mu
    if q is None:
        return p1, torch.diag_embed(var), var
    q = (q + q.transpose(1, 2)) / 2
    if mode == 1:
        jac = jm + torch.einsum('tade,te->tad', hm, dz)
        h = a + jac[:, :, :n_s] + (jac[:, :, n_s:] + b) @ k
    else:
        h = a + b @ k
    return p1, h @ q @ h.transpose(1, 2) + torch.diag_embed(var), var


def regime(out, name, N, n_s, n_u, T, n=100):
    gp = model(N, n_s, n_u)
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    A = rng.standard_normal((T, n_s, n_s))
    p, u = t(0.3 * rng.standard_normal((T, n_s))), t(0.2 * rng.standard_normal((T, n_u)))
    q, k = t(0.02 * np.einsum('tij,tkj->tik', A, A) / n_s), t(0.3 * rng.standard_normal((T, n_u, n_s)))
    mb, sb, vb = t(rng.standard_normal((T, n_s))), t(rng.standard_normal((T, n_s, n_s))), t(rng.standard_normal((T, n_s)))
    a_np, b_np = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    a, b = t(a_np), t(b_np)
    z0 = torch.cat((p, u), dim=1)
    grad_t = timeit(lambda: gp.predict_device_grad(z0), n=n)
    lin_t = timeit(lambda: gp.linearize_device_batch(z0), n=n)
    out.append("  %-34s sr_gp_predict_grad %8.1f us   sr_gp_linearize_batch %8.1f us   (whole batch, one call)" % (name, grad_t, lin_t))
    for mode, mname in ((1, "taylor"), (2, "mean-eq")):
        for gauss in (True, False):
            sx, kk = (q, k) if gauss else (None, None)
            fwd = timeit(lambda: prop.onestep_moments_batch(p, gp, u, sx, kk, a_np, b_np, mode), n=n)
            vjp = lambda: prop.onestep_moments_vjp_batch(p, gp, u, mb, sb, vb, sx, kk, a_np, b_np, mode)
            rev = timeit(vjp, n=n)
            gp_t, gp_name = (lin_t, "linearize_batch") if (gauss and mode == 1) else (grad_t, "predict_grad")

            def torch_route():
                lin = gp.linearize_device_batch(z0)
                leaves = [x.detach().requires_grad_(True) for x in ((p, q, u, k) if gauss else (p, u))]
                if gauss:
                    outs = torch_step(leaves[0], leaves[1], leaves[2], leaves[3], lin, z0, a, b, mode)
                else:
                    outs = torch_step(leaves[0], None, leaves[1], None, lin, z0, a, b, mode)
                return torch.autograd.grad((outs[0] * mb).sum() + (outs[1] * sb).sum() + (outs[2] * vb).sum(), leaves)

            tor = timeit(torch_route, n=max(5, n // 10))
            got = [g for g in vjp() if g is not None]
            agree = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, torch_route()))
            out.append("    %-8s %-6s fwd %8.1f us   vjp %8.1f us (%.2f fwd, %.2f %s)   torch port %9.1f us (%.1f vjp)   vjp vs torch %.1e"
                       % (mname, "gauss" if gauss else "point", fwd, rev, rev / fwd, rev / gp_t, gp_name, tor, tor / rev, agree))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r16_moments_grad.txt")
    out = ["sr_onestep_moments_vjp -- time per call beside the forward sr_onestep_moments, 1 x MI355X",
           "(scripts/moments_grad_bench.py; medians of five batches, host clock around synchronised batches of calls on device tensors)",
           ""]
    regime(out, "cart-pole N=150 n_s=4 n_u=1 T=256", 150, 4, 1, 256)
    regime(out, "cart-pole N=150 n_s=4 n_u=1 T=3840", 150, 4, 1, 3840)
    regime(out, "N=5000 n_s=2 n_u=1 T=4096", 5000, 2, 1, 4096, n=20)
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
