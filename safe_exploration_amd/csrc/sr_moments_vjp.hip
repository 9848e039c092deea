// sr_moments_vjp.hip -- reverse pass of ONE Gaussian moment step, modes 1 (Taylor) and 2 (mean-equivalent)
// (sr_moment_step_vjp, sr_onestep_moments_vjp).
//
//   sr_moments_vjp_kernel   one thread per query: (mode 1 under an input transform) the state-space Jacobian from the GP's, the
//                           reverse of the moment algebra (sr_moments_vjp_one), and the GP link of sr_reach_vjp.hip that adds
//                           [Tz^T z_bar[:n_xin]; z_bar[n_xin:]] to mux_bar and kff_bar (sr_reach_gp_vjp_one) -- each thread reads
//                           back only what it wrote itself, so the three stages need no barrier and no second launch
// z = [Tz mu_x; k_ff] comes from sr_reach_z_kernel (sr_reach_vjp.hip).  The link is told by the two fields sr_reach_vjp.hip names:
// jac_mu == NULL, no link (sr_moment_step_vjp); hess_mu == NULL, no second-order term.  The host sets hess_mu only where jac_bar is
// not zero: mode 1 from a Gaussian start.  The formulas and the conventions: sr_moments_vjp_dev.h.  Chains of steps are
// differentiated by torch autograd over this one step (uncertainty_propagation_casadi.multistep_moments_batch(differentiable=
// True)), or in one call by the sweep of sr_moments_rollout_vjp.hip over the same device functions.
#include "sr_common.h"
#include "sr_moments_vjp_dev.h"

template <int NS, int NU, int MODE>
__global__ __launch_bounds__(sr_vjp_threads<NS>()) void sr_moments_vjp_kernel(sr_momvjp_args m) {
    constexpr int BT = sr_vjp_threads<NS>();
    __shared__ double lds[sr_vjp_in_lds<NS>() ? NS * NS * BT : 1];
    const long t = (long)blockIdx.x * BT + threadIdx.x;
    if (t >= m.e.T) return;
    if (m.e.jac_mu && m.e.Tz && m.e.hess_mu) {
        sr_reach_gp_jac_one(m.e, t, NS, NU);
        m.e.jac = m.e.jac_s;
    }
    sr_moments_vjp_one<NS, NU, MODE>(m, t, lds + threadIdx.x, BT);
    if (m.e.jac_mu) sr_reach_gp_vjp_one(m.e, t, NS, NU);
}

int sr_launch_moments_vjp(const sr_momvjp_args& m, int n_s, int n_u, hipStream_t s) {
    if (m.e.T <= 0) return SR_OK;
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("moments vjp: n_s=%d outside 1..8", n_s, [&](auto ns) {
        constexpr int BT = sr_vjp_threads<decltype(ns)::value>();
        const dim3 grid((unsigned)((m.e.T + BT - 1) / BT));
        return sr_pick_eq<1, 2, 3, 4>("moments vjp: n_u=%d outside 1..4", n_u, [&](auto nu) {
            return sr_pick_eq<1, 2>("moments vjp: mode=%d outside 1..2", m.mode, [&](auto mode) {
                return sr_launch(sr_moments_vjp_kernel<decltype(ns)::value, decltype(nu)::value, decltype(mode)::value>, grid,
                                 dim3(BT), 0, s, m); }); }); });
}
