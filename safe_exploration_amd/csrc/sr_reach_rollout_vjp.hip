// sr_reach_rollout_vjp.hip -- reverse pass of a whole roll-out of reachability steps (sr_multistep_reach_vjp), behind ONE batched
// linearisation over every (trajectory, step) pair.
//
//   sr_reach_rollout_prep_kernel   parallel over the Tg H (trajectory, step) pairs of a group, query n = t H + i: the GP input
//                                  z[n] = [Tz p_in; k_ff[t][i]] and the step's (q_in, k_fb_in), copied to a layout dense in n;
//                                  (p_in, q_in, k_fb_in) = (p0, q0, k_fb0)[t] at i = 0, (p_all[t][i-1], q_all[t][i-1], k_fb[t][i-1])
//                                  behind it.  The centres do not depend on the sweep, so all of this runs before it.
//   sr_reach_rollout_eig_kernel    one thread per query: r^2 and its eigenvectors by the Jacobi iteration of the one-step kernel
//                                  (sr_top_eigenpair_qb), stored: they depend on no seed
//   sr_reach_rollout_vjp_kernel    one thread per trajectory, i = H - 1 .. 0: seed of step i = the caller's seed on (p_all, q_all)[t][i]
//                                  plus the (p_bar, q_bar) step i + 1 left; then the three stages of sr_reach_vjp_kernel at query n
//                                  (sr_reach_gp_jac_one, sr_ellipsoid_vjp_one, sr_reach_gp_vjp_one: sr_ellipsoid_vjp_dev.h, nothing
//                                  is derived here a second time; between the last two the caller's seed on the step's GP variances,
//                                  where there is one, is added to var_bar); then k_fb_bar of the step to where the caller wants it.
// Everything a thread reads back it wrote itself: no barrier, no atomics, no waiting between workgroups, sums in a fixed order --
// the same bits on every call and for any grouping of the trajectories.
// The caller's q seed is symmetrised BEFORE the carried q_bar (exactly symmetric) is added, and the sum is stored in both halves:
// a seed and its symmetric part give the same bits.  A step that is a bound violation writes NaN into its own outputs
// (sr_ellipsoid_vjp_one); the NaN (p_bar, q_bar) are the seeds of every earlier step of that trajectory and of nothing else.
// FORM.  Between the two that were on the table.  Out of the sequential loop, in launches parallel over all (trajectory, step)
// pairs: the inputs, the GP with all its derivatives, and the eigenpair of r^2 (the Jacobi iteration and two of the three Cholesky
// factorisations of a step).  Still inside it, by the one-step device functions as they stand: H, tr Q0, c1, c2 (a few square roots
// and n_s^3 multiply-adds, interleaved there with the sums over the seed), the linear map of the seed and the GP link.  Workgroups
// of one wavefront for every n_s, so that 256 trajectories spread over four CUs instead of one.
// MEASURED (profiles/r22_reach_rollout_vjp.txt, H = 15), the sweep of a cart-pole roll-out (n_s = 4) at T = 1 / 256: everything in
// the loop 443 / 663 us; the eigenpair out of it 323 / 561 us; the hand-off arrays in LDS (sr_rrv_slots) 239 / 400 us, which is
// 66 % / 57 % of the call's kernel time there, 34 - 39 % at n_s = 2, and 12 % / 4 % at T = 3840, where the linearisation pass
// dominates.  A step is not arithmetic but latency: what the stages handed to each other through global memory cost a round trip
// per store and dependent load; what is left (16 us per step at n_s = 4) is the step's own inputs -- q, K, the GP derivatives, the
// caller's seed --, loaded from global memory stage after stage with one wavefront per SIMD to hide it.
#include "sr_common.h"
#include "sr_ellipsoid_vjp_dev.h"

#define SR_RRV_THREADS 64

__global__ __launch_bounds__(256) void sr_reach_rollout_prep_kernel(sr_rrv_args r) {
    const int NS = r.n_s, NU = r.n_u, H = r.H;
    const int nx = r.e.Tz ? r.e.n_xin : NS, D = nx + NU;
    const int nss = NS * NS, nus = NU * NS, per = D + nss + nus;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= r.e.T * H * per) return;
    const long n = idx / per, t = n / H;
    const int e = (int)(idx % per), i = (int)(n % H);
    if (e < D) {
        const double* p = i == 0 ? r.p0 + t * NS : r.p_all + (n - 1) * NS;
        double v;
        if (e >= nx) {
            v = r.k_ff[n * NU + (e - nx)];
        } else if (r.e.Tz) {
            v = 0.0;
            for (int j = 0; j < NS; ++j) v = fma(r.e.Tz[e * NS + j], p[j], v);
        } else {
            v = p[e];
        }
        r.z[n * D + e] = v;
    } else if (e < D + nss) {
        const int k = e - D;
        const double* q = i == 0 ? (r.q0 ? r.q0 + t * nss : nullptr) : r.q_all + (n - 1) * nss;
        r.q_in[n * nss + k] = q ? q[k] : 0.0;
    } else {
        const int k = e - D - nss;
        const double* kf = i == 0 ? (r.k_fb0 ? r.k_fb0 + t * nus : nullptr) : r.k_fb + (t * (H - 1) + (i - 1)) * nus;
        r.kfb_in[n * nus + k] = kf ? kf[k] : 0.0;
    }
}

// r^2 = lambda_max(q_in (I + kfb_in^T kfb_in)) of query n with its eigenvectors (sr_top_eigenpair_qb, as the one-step kernel calls
// it), stored for the sweep: no seed enters, so every (trajectory, step) pair has a thread of its own here
template <int NS, int NU>
__global__ __launch_bounds__(sr_vjp_threads<NS>()) void sr_reach_rollout_eig_kernel(sr_rrv_args r) {
    constexpr int BT = sr_vjp_threads<NS>();
    __shared__ double lds[sr_vjp_in_lds<NS>() ? NS * NS * BT : 1];
    const long n = (long)blockIdx.x * BT + threadIdx.x;
    if (n >= r.e.T * r.H) return;
    if (r.q0 == nullptr && n % r.H == 0) return;                 // step 0 of a point start has no ellipsoid
    double r2, w[NS], v[NS], kv[NU];
    sr_tmat<NS, sr_vjp_in_lds<NS>()> V(lds + threadIdx.x, BT);
    sr_top_eigenpair_qb<NS, NU>(r.q_in, r.kfb_in, n, r2, w, v, kv, V);
    double* e = r.eig + n * sr_vjp_eig_doubles(NS, NU);
    e[0] = r2;
#pragma unroll
    for (int i = 0; i < NS; ++i) { e[1 + i] = w[i]; e[1 + NS + i] = v[i]; }
#pragma unroll
    for (int u = 0; u < NU; ++u) e[1 + 2 * NS + u] = kv[u];
}

// The arrays the stages of a step hand to each other and to the next step (sr_ellipsoid_vjp_dev.h: the index ts).  n_s <= 4: one
// slot per thread in LDS (at most 84 KB per workgroup at n_s = 4, n_u = 4) -- a store and a dependent load through global memory
// cost a round trip each, a dozen of them per step, and with one thread walking H steps nothing hides them.  n_s >= 5, where the
// thread's n_s x n_s block already takes the LDS: the per-query slots of the scratch, as in the one-step kernel.
template <int NS, int NU>
struct sr_rrv_slots {
    static constexpr bool IN_LDS = !sr_vjp_in_lds<NS>();
    static constexpr int DS = NS + NU, DMAX = 8;                       // D <= 8: the widths of sr_gp_linearize_batch
    static constexpr int WORDS = IN_LDS ? 4 * NS + NU + 2 * NS * NS + NU * NS + 2 * NS * DS + NS * DMAX : 1;
};

template <int NS, int NU>
__global__ __launch_bounds__(SR_RRV_THREADS) void sr_reach_rollout_vjp_kernel(sr_rrv_args r) {
    using S = sr_rrv_slots<NS, NU>;
    constexpr int BT = SR_RRV_THREADS;
    __shared__ double lds[sr_vjp_in_lds<NS>() ? NS * NS * BT : 1];
    __shared__ double slots[S::WORDS * BT];
    const long t = (long)blockIdx.x * BT + threadIdx.x;
    if (t >= r.e.T) return;
    const int H = r.H;
    const bool point = r.q0 == nullptr;
    sr_ellvjp_args a = r.e;
    double* p_seed = r.p_seed;
    double* q_seed = r.q_seed;
    if (S::IN_LDS) {
        double* w = slots;
        auto take = [&](int each) { double* x = w; w += each * BT; return x; };
        a.mu_bar = take(NS); a.var_bar = take(NS); p_seed = take(NS); a.p_bar = take(NS); a.kff_bar = take(NU);
        q_seed = take(NS * NS); a.q_bar = take(NS * NS); a.kfb_bar = take(NU * NS);
        a.jac_bar = take(NS * S::DS); a.jac_s = take(NS * S::DS); a.jz = take(NS * S::DMAX);
    }
    a.p1_bar = p_seed; a.q1_bar = q_seed;
    for (int i = H - 1; i >= 0; --i) {
        const long n = t * H + i;
        // where this step's hand-off arrays are, and where step i + 1 left its (p_bar, q_bar): the thread's slot, or the queries'
        const long ts = S::IN_LDS ? (long)threadIdx.x : n, tc = S::IN_LDS ? (long)threadIdx.x : n + 1;
        // the seed of step i
        const bool carry = i + 1 < H;
        const double* pe = r.p_all_bar ? r.p_all_bar + n * NS : nullptr;
        const double* qe = r.q_all_bar ? r.q_all_bar + n * NS * NS : nullptr;
        double pc[NS], qc[NS][NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            pc[k] = carry ? a.p_bar[tc * NS + k] : 0.0;
#pragma unroll
            for (int l = 0; l < NS; ++l)
                if (l >= k) qc[k][l] = carry ? a.q_bar[(tc * NS + k) * NS + l] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const double x = pe ? pe[k] : 0.0;
            p_seed[ts * NS + k] = carry ? x + pc[k] : x;
#pragma unroll
            for (int l = 0; l < NS; ++l)
                if (l >= k) {
                    const double y = qe ? 0.5 * (qe[k * NS + l] + qe[l * NS + k]) : 0.0;
                    const double z = carry ? y + qc[k][l] : y;
                    q_seed[(ts * NS + k) * NS + l] = z;
                    q_seed[(ts * NS + l) * NS + k] = z;
                }
        }
        // the step (the stages of sr_reach_vjp_kernel); a point start has neither q nor a second-order term at step 0
        const bool pt = point && i == 0;
        a.q = pt ? nullptr : r.e.q;
        a.hess_mu = pt ? nullptr : r.e.hess_mu;
        a.jac = r.e.jac;
        if (a.Tz && a.hess_mu) {
            sr_reach_gp_jac_one(a, n, NS, NU, ts);
            a.jac = a.jac_s;
        }
        sr_ellipsoid_vjp_one<NS, NU, true>(a, n, lds + threadIdx.x, BT, r.eig, ts);
        // the caller's seed on this step's GP variances (sr_multistep_reach_var_vjp), between the stage that writes var_bar and the
        // one that reads it.  Behind a branch: x + 0.0 is not x for x = -0.0; a NaN var_bar of a bound violation stays NaN
        if (r.gpvar_all_bar)
#pragma unroll
            for (int k = 0; k < NS; ++k) a.var_bar[ts * NS + k] += r.gpvar_all_bar[n * NS + k];
        sr_reach_gp_vjp_one(a, n, NS, NU, ts);
        // the gradients of the controls: to the caller's kff_bar[t][i] and k_fb_bar[t][i - 1], or kfb0_bar[t]
#pragma unroll
        for (int k = 0; k < NU; ++k) r.kff_bar[n * NU + k] = a.kff_bar[ts * NU + k];
        double* kd = i > 0 ? r.kfb_bar + (t * (H - 1) + (i - 1)) * NU * NS : (r.kfb0_bar ? r.kfb0_bar + t * NU * NS : nullptr);
        if (kd)
#pragma unroll
            for (int k = 0; k < NU * NS; ++k) kd[k] = a.kfb_bar[ts * NU * NS + k];
    }
    const long t0 = S::IN_LDS ? (long)threadIdx.x : t * H;
#pragma unroll
    for (int k = 0; k < NS; ++k) r.p0_bar[t * NS + k] = a.p_bar[t0 * NS + k];
    if (r.q0_bar)
#pragma unroll
        for (int k = 0; k < NS * NS; ++k) r.q0_bar[t * NS * NS + k] = a.q_bar[t0 * NS * NS + k];
}

int sr_launch_reach_rollout_prep(const sr_rrv_args& r, hipStream_t s) {
    if (r.e.T <= 0) return SR_OK;
    const int nx = r.e.Tz ? r.e.n_xin : r.n_s;
    const long n = r.e.T * r.H * (nx + r.n_u + (long)r.n_s * r.n_s + (long)r.n_u * r.n_s);
    return sr_launch(sr_reach_rollout_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, r);
}

int sr_launch_reach_rollout_eig(const sr_rrv_args& r, hipStream_t s) {
    if (r.e.T <= 0) return SR_OK;
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    const long Q = r.e.T * r.H;
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("roll-out vjp: n_s=%d outside 1..8", r.n_s, [&](auto ns) {
        constexpr int BT = sr_vjp_threads<decltype(ns)::value>();
        const dim3 grid((unsigned)((Q + BT - 1) / BT));
        return sr_pick_eq<1, 2, 3, 4>("roll-out vjp: n_u=%d outside 1..4", r.n_u, [&](auto nu) {
            return sr_launch(sr_reach_rollout_eig_kernel<decltype(ns)::value, decltype(nu)::value>, grid, dim3(BT), 0, s, r); }); });
}

int sr_launch_reach_rollout_vjp(const sr_rrv_args& r, hipStream_t s) {
    if (r.e.T <= 0) return SR_OK;
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    const dim3 grid((unsigned)((r.e.T + SR_RRV_THREADS - 1) / SR_RRV_THREADS));
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("roll-out vjp: n_s=%d outside 1..8", r.n_s, [&](auto ns) {
        return sr_pick_eq<1, 2, 3, 4>("roll-out vjp: n_u=%d outside 1..4", r.n_u, [&](auto nu) {
            return sr_launch(sr_reach_rollout_vjp_kernel<decltype(ns)::value, decltype(nu)::value>, grid, dim3(SR_RRV_THREADS), 0,
                             s, r); }); });
}
