// sr_moments_rollout_vjp.hip -- reverse pass of a whole roll-out of Gaussian moment steps, modes 1 (Taylor) and 2 (mean-equivalent)
// (sr_multistep_moments_vjp), behind ONE pass of GP derivatives over every (trajectory, step) pair.
//
//   sr_reach_rollout_prep_kernel     (sr_reach_rollout_vjp.hip, as it stands, under the names p = mu, q = sigma) the GP input
//                                    z[n] = [Tz mu_in; k_ff[t][i]] of query n = t H + i and the step's (sigma_in, k_fb_in) dense in n:
//                                    zeros at i = 0 of a point start, a zero gain at i = 0 of a Gaussian start (k_fb0 == NULL)
//   sr_moments_rollout_vjp_kernel    one thread per trajectory, i = H - 1 .. 0: seed of step i = the caller's seed on (mu_all,
//                                    sigma_all)[t][i] plus the (mu_bar, sigma_bar) step i + 1 left; then the three stages of
//                                    sr_moments_vjp_kernel at query n (sr_reach_gp_jac_one, sr_moments_vjp_one, sr_reach_gp_vjp_one:
//                                    nothing is derived here a second time; the seed on the GP variances is read where the caller
//                                    has it, it is carried nowhere); then k_fb_bar of the step to where the caller wants it.
// Everything a thread reads back it wrote itself: no barrier, no atomics, no waiting between workgroups, sums in a fixed order --
// the same bits on every call and for any grouping of the trajectories.  The caller's sigma seed is symmetrised BEFORE the carried
// sigma_bar (exactly symmetric) is added, and the sum is stored in both halves: a seed and its symmetric part give the same bits.
// There is no square root and no eigenvalue in these modes: no step is "bad", nothing is NaN that was not NaN in the inputs.
// FORM, that of sr_reach_rollout_vjp.hip, for the reasons measured there: the hand-off arrays of a step live in LDS for n_s <= 4
// (sr_mrv_slots; the mean-equivalent mode has no jac_bar, jac_s or jz and leaves them out), in the per-query slots of the scratch
// for n_s >= 5, where the thread's n_s x n_s block takes the LDS; workgroups of one wavefront for every n_s, so that a few hundred
// trajectories spread over several CUs.  No instance uses scratch memory: profiles/r24_moments_rollout_vjp_resources.txt.
#include "sr_common.h"
#include "sr_moments_vjp_dev.h"

#define SR_MRV_THREADS 64

template <int NS, int NU, int MODE>
struct sr_mrv_slots {
    static constexpr bool IN_LDS = !sr_vjp_in_lds<NS>();
    static constexpr int DS = NS + NU, DMAX = 8;                       // D <= 8: the widths of sr_gp_linearize_batch
    static constexpr int WORDS = IN_LDS ? 4 * NS + NU + 2 * NS * NS + NU * NS + (MODE == 1 ? 2 * NS * DS + NS * DMAX : 0) : 1;
};

template <int NS, int NU, int MODE>
__global__ __launch_bounds__(SR_MRV_THREADS) void sr_moments_rollout_vjp_kernel(sr_mrv_args mr) {
    using S = sr_mrv_slots<NS, NU, MODE>;
    constexpr int BT = SR_MRV_THREADS;
    __shared__ double lds[sr_vjp_in_lds<NS>() ? NS * NS * BT : 1];
    __shared__ double slots[S::WORDS * BT];
    const sr_rrv_args& r = mr.r;
    const long t = (long)blockIdx.x * BT + threadIdx.x;
    if (t >= r.e.T) return;
    const int H = r.H;
    const bool point = r.q0 == nullptr;
    sr_momvjp_args m;
    m.e = r.e; m.gpvar_bar = r.gpvar_all_bar; m.mode = MODE;
    sr_ellvjp_args& a = m.e;
    double* p_seed = r.p_seed;
    double* q_seed = r.q_seed;
    if (S::IN_LDS) {
        double* w = slots;
        auto take = [&](int each) { double* x = w; w += each * BT; return x; };
        a.mu_bar = take(NS); a.var_bar = take(NS); p_seed = take(NS); a.p_bar = take(NS); a.kff_bar = take(NU);
        q_seed = take(NS * NS); a.q_bar = take(NS * NS); a.kfb_bar = take(NU * NS);
        if (MODE == 1) { a.jac_bar = take(NS * S::DS); a.jac_s = take(NS * S::DS); a.jz = take(NS * S::DMAX); }
    }
    a.p1_bar = p_seed; a.q1_bar = q_seed;
    for (int i = H - 1; i >= 0; --i) {
        const long n = t * H + i;
        // where this step's hand-off arrays are, and where step i + 1 left its (mu_bar, sigma_bar): the thread's slot, or the queries'
        const long ts = S::IN_LDS ? (long)threadIdx.x : n, tc = S::IN_LDS ? (long)threadIdx.x : n + 1;
        // the seed of step i (the lines of sr_reach_rollout_vjp_kernel: shared through a device function they changed that kernel's
        // register allocation, so they stand here a second time)
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
        // the step (the stages of sr_moments_vjp_kernel); a point start has neither sigma nor a second-order term at step 0
        const bool pt = point && i == 0;
        a.q = pt ? nullptr : r.e.q;
        a.hess_mu = pt ? nullptr : r.e.hess_mu;
        a.jac = r.e.jac;
        if (MODE == 1 && a.Tz && a.hess_mu) {
            sr_reach_gp_jac_one(a, n, NS, NU, ts);
            a.jac = a.jac_s;
        }
        sr_moments_vjp_one<NS, NU, MODE>(m, n, lds + threadIdx.x, BT, ts);
        sr_reach_gp_vjp_one(a, n, NS, NU, ts);
        // the gradients of the controls: to the caller's kff_bar[t][i] and kfb_bar[t][i - 1] (step 0 has no gain of the caller's)
#pragma unroll
        for (int k = 0; k < NU; ++k) r.kff_bar[n * NU + k] = a.kff_bar[ts * NU + k];
        if (i > 0) {
            double* kd = r.kfb_bar + (t * (H - 1) + (i - 1)) * NU * NS;
#pragma unroll
            for (int k = 0; k < NU * NS; ++k) kd[k] = a.kfb_bar[ts * NU * NS + k];
        }
    }
    const long t0 = S::IN_LDS ? (long)threadIdx.x : t * H;
#pragma unroll
    for (int k = 0; k < NS; ++k) r.p0_bar[t * NS + k] = a.p_bar[t0 * NS + k];
    if (r.q0_bar)
#pragma unroll
        for (int k = 0; k < NS * NS; ++k) r.q0_bar[t * NS * NS + k] = a.q_bar[t0 * NS * NS + k];
}

int sr_launch_moments_rollout_vjp(const sr_mrv_args& m, hipStream_t s) {
    if (m.r.e.T <= 0) return SR_OK;
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    const dim3 grid((unsigned)((m.r.e.T + SR_MRV_THREADS - 1) / SR_MRV_THREADS));
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("moments roll-out vjp: n_s=%d outside 1..8", m.r.n_s, [&](auto ns) {
        return sr_pick_eq<1, 2, 3, 4>("moments roll-out vjp: n_u=%d outside 1..4", m.r.n_u, [&](auto nu) {
            return sr_pick_eq<1, 2>("moments roll-out vjp: mode=%d outside 1..2", m.mode, [&](auto mode) {
                return sr_launch(sr_moments_rollout_vjp_kernel<decltype(ns)::value, decltype(nu)::value, decltype(mode)::value>, grid,
                                 dim3(SR_MRV_THREADS), 0, s, m); }); }); });
}
