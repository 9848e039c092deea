"""Reference of the reverse pass of the exact moment-matching roll-out (sr_gp_moment_match_rollout_vjp) -- TEST
infrastructure, CPU only.

``sweep``: one trajectory, in NumPy.  Like the device it takes the stored ``mu_all`` / ``sigma_all`` of a forward as given:
step i is differentiated at (mu_{i-1}, Sigma_{i-1}) as stored, step 0 at (mu_0, sigma_0) or in the point branch.  The GP link
is ``_mm_grad_ref.vjp`` at the step's Gaussian input; the algebra around it is the step of ``_mm_ref.step`` written backwards:

  forward   G = [tz; K], A = a + b K, W = V G, Hm = A + W
            mu+ = A mu + b k + mu_g,   Sigma+ = Hm Sigma Hm^T + C - W Sigma W^T,   cov = C
  reverse   Ss = sym(Sigma+_bar), Sigma its symmetric part
            mu_g_bar = mu+_bar,  C_bar = Ss + sym(c_bar),  W_bar = 2 Ss A Sigma,  V_bar = W_bar G^T
            A_bar = 2 Ss Hm Sigma + mu+_bar mu^T,  G_bar = V^T W_bar,  mu_bar = A^T mu+_bar
            Sigma_bar = Hm^T Ss Hm - W^T Ss W,  k_bar = b^T mu+_bar,  K_bar = b^T A_bar
            (m_z_bar, S_z_bar) = MM-vjp(mu_g_bar, C_bar, V_bar)
            mu_bar += G^T m_z_bar,  k_bar += m_z_bar[n_x_in:],  G_bar += m_z_bar mu^T + 2 S_z_bar G Sigma
            Sigma_bar += G^T S_z_bar G,  K_bar += G_bar[n_x_in:]
Step 0 has K = 0 and no K_bar; from a point Sigma+ = C, so V_bar = 0 and S_z_bar is dropped.  The seed of step i is the
caller's seed at i plus the (mu_bar, Sigma_bar) of step i + 1.  The scalar differentiated is
  L = sum(mu_all_bar * mu_all) + sum(sigma_all_bar * sigma_all) + sum(cov_all_bar * cov_all)        (cov unclipped)."""
import numpy as np

import _mm_ref as R
import _mm_grad_ref as G


def _sym(x):
    return 0.5 * (x + x.T)


def sweep(arrs, mu0, sigma0, k_ff, k_fb, a, b, tz, mu_all, sigma_all, mu_all_bar=None, sigma_all_bar=None,
          cov_all_bar=None, dtype=np.float64):
    """arrs = (Z, alpha, M, ls, sf2); mu0 (n_s,), sigma0 (n_s,n_s) | None; k_ff (H,n_u); k_fb (H-1,n_u,n_s) | None; tz
    (n_x_in,n_s); mu_all (H,n_s), sigma_all (H,n_s,n_s) as a forward stored them; seeds shaped like the forward's outputs,
    None = zero.  -> mu0_bar (n_s,), sigma0_bar (n_s,n_s) | None, kff_bar (H,n_u), kfb_bar (H-1,n_u,n_s) | None"""
    H, n_u = k_ff.shape
    n_s, n_x = mu0.shape[0], tz.shape[0]
    zero = lambda x, shp: np.zeros(shp) if x is None else np.asarray(x, float)
    mb_all, sb_all, cb_all = zero(mu_all_bar, (H, n_s)), zero(sigma_all_bar, (H, n_s, n_s)), zero(cov_all_bar, (H, n_s, n_s))
    kff_bar = np.zeros((H, n_u))
    kfb_bar = np.zeros((H - 1, n_u, n_s)) if H > 1 else None
    carry_mu, carry_sig = np.zeros(n_s), np.zeros((n_s, n_s))
    for i in range(H - 1, -1, -1):
        mu = mu0 if i == 0 else mu_all[i - 1]
        point = i == 0 and sigma0 is None
        Sg = np.zeros((n_s, n_s)) if point else _sym(sigma0 if i == 0 else sigma_all[i - 1])
        K = np.zeros((n_u, n_s)) if i == 0 else k_fb[i - 1]
        Gm = np.vstack((tz, K))
        A = a + b.dot(K)
        m_z = Gm.dot(mu) + np.concatenate((np.zeros(n_x), k_ff[i]))
        S_z = None if point else Gm.dot(Sg).dot(Gm.T)
        _, _, V = R.moment_match(*arrs, m_z, S_z)
        W = V.dot(Gm)
        Hm = A + W
        mub = mb_all[i] + carry_mu
        Ss = _sym(sb_all[i] + carry_sig)
        C_bar = Ss + _sym(cb_all[i])
        W_bar = 2.0 * Ss.dot(A).dot(Sg)
        V_bar = W_bar.dot(Gm.T)
        A_bar = 2.0 * Ss.dot(Hm).dot(Sg) + np.outer(mub, mu)
        G_bar = V.T.dot(W_bar)
        carry_mu = A.T.dot(mub)
        carry_sig = Hm.T.dot(Ss).dot(Hm) - W.T.dot(Ss).dot(W)
        k_bar = b.T.dot(mub)
        K_bar = b.T.dot(A_bar)
        mz_bar, Sz_bar = G.vjp(*arrs, m_z, S_z, mub, C_bar, None if point else V_bar, dtype=dtype)
        mz_bar, Sz_bar = np.asarray(mz_bar, float), np.asarray(Sz_bar, float)
        carry_mu = carry_mu + Gm.T.dot(mz_bar)
        k_bar = k_bar + mz_bar[n_x:]
        G_bar = G_bar + np.outer(mz_bar, mu) + 2.0 * Sz_bar.dot(Gm).dot(Sg)
        carry_sig = carry_sig + Gm.T.dot(Sz_bar).dot(Gm)
        kff_bar[i] = k_bar
        if i > 0:
            kfb_bar[i - 1] = K_bar + G_bar[n_x:]
    return carry_mu, None if sigma0 is None else _sym(carry_sig), kff_bar, kfb_bar


def sweep_batch(arrs, c, mu_all, sigma_all, mu_all_bar=None, sigma_all_bar=None, cov_all_bar=None, trajs=None):
    """every trajectory of a case of ``_mm_rollout_cases`` (or those in ``trajs``); the gradients per trajectory, also for a
    shared policy: mu0_bar (T,n_s), sigma0_bar (T,n_s,n_s) | None, kff_bar (T,H,n_u), kfb_bar (T,H-1,n_u,n_s) | None"""
    import _mm_rollout_cases as C
    trajs = range(c["T"]) if trajs is None else trajs
    outs = []
    for k, t in enumerate(trajs):
        kff, kfb = C.gains(c, t)
        outs.append(sweep(arrs, c["mu0"][t], None if c["sigma0"] is None else c["sigma0"][t], kff, kfb, c["a"], c["b"],
                          C.tz_of(c), mu_all[k], sigma_all[k], None if mu_all_bar is None else mu_all_bar[k],
                          None if sigma_all_bar is None else sigma_all_bar[k],
                          None if cov_all_bar is None else cov_all_bar[k]))
    return tuple(None if outs[0][j] is None else np.stack([o[j] for o in outs]) for j in range(4))
