// sr_reach_ws.h -- the layout of the handle's reach_ws, the scratch of the reverse passes with the GP inside (sr_capi_reach.hip:
// onestep_vjp_impl, rollout_vjp_impl).  Host only, nothing from HIP: tests/test_reach_ws_host.py compiles it alone.
// The scratch is one array per block, `rows` entries each (the queries of a one-step pass, or the (trajectory, step) pairs of a
// roll-out group), the blocks one behind the other in the order of sr_reach_ws_carve.  A use that has no need of a block leaves it
// out; the order of the others does not change.  The walk gives the base of every block and the doubles per row at once.
#pragma once

// at most 2^28 doubles (2 GB) of reach_ws: both drivers cut their passes / groups by it
constexpr long SR_REACH_WS_MAX_DOUBLES = (long)1 << 28;

// what is carved: one step (every mode has all of z .. jz), or a roll-out in mode 0 (robust ellipsoids), 1 (Taylor) or
// 2 (mean-equivalent); second: a Taylor roll-out that reads the Hessian of the mean (H > 1, or a Gaussian start)
struct sr_reach_ws_use { int n_s, n_u, D; bool rollout; int mode; bool second; };

struct sr_reach_ws {
    long per;                                        // doubles per row, all present blocks
    double *z, *mu, *var, *jac_mu, *jac_var, *hess_mu, *mu_bar, *var_bar, *jac_bar, *jac_s, *jz;
    double *q_in, *kfb_in, *p_seed, *q_seed, *p_bar, *q_bar, *kff_bar, *kfb_bar, *eig;          // roll-outs only
};

// base == NULL: every pointer NULL, per is the size
static inline sr_reach_ws sr_reach_ws_carve(const sr_reach_ws_use& u, long rows, double* base) {
    const long n_s = u.n_s, n_u = u.n_u, D = u.D, nss = n_s * n_s, nus = n_u * n_s, nd = n_s * D, nds = n_s * (n_s + n_u);
    const bool ro = u.rollout;
    const bool hess = !ro || u.mode == 0 || (u.mode == 1 && u.second);
    const bool link = !ro || u.mode != 2;            // mode 2 has no seed on the Jacobian
    long per = 0;
    auto take = [&](bool present, long each) -> double* {
        if (!present) return nullptr;
        double* x = base ? base + rows * per : nullptr;
        per += each;
        return x;
    };
    sr_reach_ws w;
    w.z = take(true, D);                                                          // z = [Tz p; k_ff]
    w.mu = take(true, n_s); w.var = take(true, n_s);                              // the GP at z ...
    w.jac_mu = take(true, nd); w.jac_var = take(true, nd);                        // ... its first derivatives ...
    w.hess_mu = take(hess, nd * D);                                               // ... and the Hessian of the mean
    w.mu_bar = take(true, n_s); w.var_bar = take(true, n_s);                      // the step's seeds on the GP's outputs
    w.jac_bar = take(link, nds); w.jac_s = take(link, nds);                       // seed on the Jacobian, the state-space Jacobian
    w.jz = take(link, nd);                                                        // seed on the GP's Jacobian
    w.q_in = take(ro, nss); w.kfb_in = take(ro, nus); w.p_seed = take(ro, n_s); w.q_seed = take(ro, nss);      // a step's inputs, seeds
    w.p_bar = take(ro, n_s); w.q_bar = take(ro, nss); w.kff_bar = take(ro, n_u); w.kfb_bar = take(ro, nus);    // a step's results
    w.eig = take(ro && u.mode == 0, 1 + 2 * n_s + n_u);                           // r^2, w, v, K v of the ellipsoid step
    w.per = per;
    return w;
}
