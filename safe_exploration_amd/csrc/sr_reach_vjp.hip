// sr_reach_vjp.hip -- reverse pass of ONE reachability step (sr_ellipsoid_step_vjp, sr_onestep_reach_vjp).
//
//   sr_reach_z_kernel       z[t] = [Tz p[t]; k_ff[t]], the GP input the step linearises at (one thread per entry)
//   sr_reach_vjp_kernel     one thread per query: (under an input transform) the state-space Jacobian from the GP's, the
//                           reverse of the ellipsoid algebra (sr_ellipsoid_vjp_one), and the GP link that adds
//                           [Tz^T z_bar[:n_xin]; z_bar[n_xin:]] to p_bar and kff_bar (sr_reach_gp_vjp_one) -- each thread reads
//                           back only what it wrote itself, so the three stages need no barrier and no second launch
// The link is told by two fields of sr_ellvjp_args: jac_mu == NULL, no link (sr_ellipsoid_step_vjp); hess_mu == NULL, no second-order
// term (the point branch, where jac_bar is zero: the host has run sr_gp_predict_grad, not sr_gp_linearize_batch).
// The formulas, the eigenvector route and the conventions: sr_ellipsoid_vjp_dev.h.  Chains of steps are differentiated by
// torch autograd over this one step (gp_reachability.multistep_reachability_batch(differentiable=True)), or in one call by
// sr_multistep_reach_vjp (sr_reach_rollout_vjp.hip: one linearisation pass over every step, then a sweep over the same device
// functions).
#include "sr_common.h"
#include "sr_ellipsoid_vjp_dev.h"

__global__ __launch_bounds__(256) void sr_reach_z_kernel(const double* __restrict__ p, const double* __restrict__ k_ff,
                                                         const double* __restrict__ Tz, double* __restrict__ z, long T,
                                                         int n_s, int n_u, int n_xin) {
    const int D = n_xin + n_u;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= T * D) return;
    const long t = e / D;
    const int i = (int)(e % D);
    double v;
    if (i >= n_xin) {
        v = k_ff[t * n_u + (i - n_xin)];
    } else if (Tz) {
        v = 0.0;
        for (int j = 0; j < n_s; ++j) v = fma(Tz[i * n_s + j], p[t * n_s + j], v);
    } else {
        v = p[t * n_s + i];
    }
    z[e] = v;
}

template <int NS, int NU>
__global__ __launch_bounds__(sr_vjp_threads<NS>()) void sr_reach_vjp_kernel(sr_ellvjp_args a) {
    constexpr int BT = sr_vjp_threads<NS>();
    __shared__ double lds[sr_vjp_in_lds<NS>() ? NS * NS * BT : 1];
    const long t = (long)blockIdx.x * BT + threadIdx.x;
    if (t >= a.T) return;
    if (a.jac_mu && a.Tz && a.hess_mu) {
        sr_reach_gp_jac_one(a, t, NS, NU);
        a.jac = a.jac_s;
    }
    sr_ellipsoid_vjp_one<NS, NU>(a, t, lds + threadIdx.x, BT);
    if (a.jac_mu) sr_reach_gp_vjp_one(a, t, NS, NU);
}

int sr_launch_reach_z(long T, int n_s, int n_u, int n_xin, const double* p, const double* k_ff, const double* Tz, double* z,
                      hipStream_t s) {
    if (T <= 0) return SR_OK;
    const long n = T * (n_xin + n_u);
    return sr_launch(sr_reach_z_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, k_ff, Tz, z, T, n_s, n_u, n_xin);
}

int sr_launch_reach_vjp(const sr_ellvjp_args& a, int n_s, int n_u, hipStream_t s) {
    if (a.T <= 0) return SR_OK;
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("ellipsoid vjp: n_s=%d outside 1..8", n_s, [&](auto ns) {
        constexpr int BT = sr_vjp_threads<decltype(ns)::value>();
        const dim3 grid((unsigned)((a.T + BT - 1) / BT));
        return sr_pick_eq<1, 2, 3, 4>("ellipsoid vjp: n_u=%d outside 1..4", n_u, [&](auto nu) {
            return sr_launch(sr_reach_vjp_kernel<decltype(ns)::value, decltype(nu)::value>, grid, dim3(BT), 0, s, a); }); });
}
