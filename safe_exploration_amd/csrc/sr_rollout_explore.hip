// sr_rollout_explore.hip -- the exploration objective over the stored GP variances of a roll-out (sr_rollout_explore) and its
// reverse pass (sr_rollout_explore_vjp): the default cost of SimpleSafeMPC.generate_cost_function (safempc_simple.py:286-315 of
// the reference: minus the summed square roots of the per-step variance sums, plus the deviation of the performance trajectory
// from the safe one) and of StaticSafeMPCExploration.init_solver (safempc_exploration.py:104: minus the summed variances), one
// launch each.
//
//   sr_rollout_explore_kernel       one thread per (trajectory, step) pair computes the step's information term (i < H_v) and its
//                                   deviation term (1 <= i < n_dev); a workgroup owns max(1, BT / HH) whole trajectories,
//                                   HH = max(H_v, n_dev); the terms of a round of BT pairs go through LDS and the trajectory's owner
//                                   thread adds them in the order i = 0 .. HH - 1, information and deviation apart.
//   sr_rollout_explore_vjp_kernel   one thread per (trajectory, row) pair, rows 0 .. max(H_v, H_p, H_m) - 1: the closed-form
//                                   gradient of row i of each of the three outputs -- every output element has one writer.
// The sums a thread forms (in the order include/safereach.h states):
//   r_i    = ((v_0 + v_1) + ... + v_{n_s-1}) + eps                      (kind 0: without eps)
//   info_i = -r_i (kind 0), -sqrt(r_i) (kind 1)
//   s_a    = fma(W[a][n_s-1], d_{n_s-1}, ... fma(W[a][0], d_0, 0)),  d = mu[t][i] - p[t][i];  dev_i = fma(d_{n_s-1}, s_{n_s-1}, ... fma(d_0, s_0, 0))
//   cost   = ((info_0 + info_1) + ...) + ((dev_1 + dev_2) + ...)        (the second bracket only with n_dev >= 2)
// The ordered sum over the steps is one thread's: a wavefront reduction would fix another order per H and split a trajectory that
// is longer than a wavefront over several of them; here H may be anything, a round is 64 pairs, and the owner reads at most 64
// words of LDS per round at consecutive addresses.  No private arrays (d is recomputed from global memory where it is used, W is
// read at wave-uniform addresses): no scratch memory, profiles/r28_explore_resources.txt.  No atomics, no waiting between
// workgroups: the same bits on every call and whatever else is in the batch, with and without cost_steps.
// Reverse:  gpvar_bar[t][i][:] = -cost_bar (kind 0), -cost_bar / (2 sqrt(r_i)) (kind 1; exactly 0 at r_i == 0: the truncated slope
// of sr_rollout_constraints_vjp; NaN at r_i < 0);  mu_bar[t][i][a] = cost_bar fma-sum_b (W[a][b] + W[b][a]) d_b and p_bar = -mu_bar
// for 1 <= i < n_dev, exact zeros in every other row.
#include "sr_common.h"
#include "sr_dispatch.h"

#define XPL_BT 64

// r_i of pair (t, i): the variances of the step in the order j = 0 .. n_s - 1, then eps (kind 1)
__device__ static inline double xpl_radicand(const sr_xpl_args& a, long t, int i) {
    const double* v = a.gp_var + (t * a.H_v + i) * a.n_s;
    double r = v[0];
    for (int j = 1; j < a.n_s; ++j) r += v[j];
    return a.kind ? r + a.eps : r;
}

// d^T W d of pair (t, i), d = mu[t][i] - p[t][i]
__device__ static inline double xpl_dev(const sr_xpl_args& a, long t, int i) {
    const int n_s = a.n_s;
    const double* m = a.mu + (t * a.H_m + i) * n_s;
    const double* p = a.p + (t * a.H_p + i) * n_s;
    double c = 0.0;
    for (int r = 0; r < n_s; ++r) {
        double s = 0.0;
        for (int q = 0; q < n_s; ++q) s = fma(a.W[r * n_s + q], m[q] - p[q], s);
        c = fma(m[r] - p[r], s, c);
    }
    return c;
}

__global__ __launch_bounds__(XPL_BT) void sr_rollout_explore_kernel(sr_xpl_args a) {
    __shared__ double info[XPL_BT], dev[XPL_BT];
    const int HH = a.H_v > a.n_dev ? a.H_v : a.n_dev, tid = threadIdx.x;
    const long t0 = (long)blockIdx.x * a.G;
    const int ng = (int)(a.T - t0 < a.G ? a.T - t0 : a.G);     // trajectories of this workgroup; ng HH <= max(XPL_BT, HH)
    const int nitem = ng * HH;
    double acc_i = 0.0, acc_d = 0.0;
    for (int base = 0; base < nitem; base += XPL_BT) {
        const int e = base + tid;
        if (e < nitem) {
            const long t = t0 + e / HH;                         // pair (t, i)
            const int i = e % HH;
            double c = 0.0, d = 0.0;
            if (i < a.H_v) {
                const double r = xpl_radicand(a, t, i);
                c = a.kind ? -sqrt(r) : -r;
                if (a.cost_steps) a.cost_steps[t * a.H_v + i] = c;
            }
            if (i >= 1 && i < a.n_dev) d = xpl_dev(a, t, i);
            info[tid] = c;
            dev[tid] = d;
        }
        __syncthreads();
        if (tid < ng) {                                         // the owner of trajectory t0 + tid: its terms of this round, in order
            const int lo = tid * HH > base ? tid * HH : base;
            int hi = (tid + 1) * HH;
            if (hi > base + XPL_BT) hi = base + XPL_BT;
            for (int k = lo; k < hi; ++k) {
                const int i = k - tid * HH;
                if (i < a.H_v) acc_i += info[k - base];
                if (i >= 1 && i < a.n_dev) acc_d += dev[k - base];
            }
        }
        __syncthreads();
    }
    if (tid < ng) a.cost[t0 + tid] = a.n_dev >= 2 ? acc_i + acc_d : acc_i;
}

__global__ __launch_bounds__(XPL_BT) void sr_rollout_explore_vjp_kernel(sr_xpl_args a) {
    const int HP = a.p_bar ? a.H_p : 0, HM = a.mu_bar ? a.H_m : 0, HV = a.gpvar_bar ? a.H_v : 0;
    const int HH = HV > HP ? (HV > HM ? HV : HM) : (HP > HM ? HP : HM);
    const long n = (long)blockIdx.x * XPL_BT + threadIdx.x;
    if (n >= a.T * HH) return;
    const long t = n / HH;
    const int i = (int)(n % HH), n_s = a.n_s;
    const double cb = a.cost_bar ? a.cost_bar[t] : 1.0;
    if (i < HV) {
        double g = -cb;
        if (a.kind) {
            const double r = xpl_radicand(a, t, i);
            g = r == 0.0 ? 0.0 : -cb / (2.0 * sqrt(r));
        }
        double* gb = a.gpvar_bar + (t * a.H_v + i) * n_s;
        for (int j = 0; j < n_s; ++j) gb[j] = g;
    }
    if (i >= HP && i >= HM) return;
    double* pb = i < HP ? a.p_bar + (t * a.H_p + i) * n_s : nullptr;
    double* mb = i < HM ? a.mu_bar + (t * a.H_m + i) * n_s : nullptr;
    const bool in = i >= 1 && i < a.n_dev;
    const double* m = in ? a.mu + (t * a.H_m + i) * n_s : nullptr;
    const double* p = in ? a.p + (t * a.H_p + i) * n_s : nullptr;
    for (int r = 0; r < n_s; ++r) {
        double s = 0.0;
        if (in) {
            for (int q = 0; q < n_s; ++q) s = fma(a.W[r * n_s + q] + a.W[q * n_s + r], m[q] - p[q], s);
            s *= cb;
        }
        if (mb) mb[r] = in ? s : 0.0;
        if (pb) pb[r] = in ? -s : 0.0;
    }
}

int sr_launch_rollout_explore(sr_xpl_args a, bool reverse, hipStream_t s) {
    const char* who = reverse ? "sr_rollout_explore_vjp" : "sr_rollout_explore";
    long grid;
    if (reverse) {
        const int HP = a.p_bar ? a.H_p : 0, HM = a.mu_bar ? a.H_m : 0, HV = a.gpvar_bar ? a.H_v : 0;
        grid = (a.T * std::max({HV, HP, HM}) + XPL_BT - 1) / XPL_BT;
    } else {
        const int HH = std::max(a.H_v, a.n_dev);
        a.G = HH >= XPL_BT ? 1 : XPL_BT / HH;
        grid = (a.T + a.G - 1) / a.G;
    }
    if (grid > 2147483647L) {
        sr_set_error("%s: T=%ld beyond the launch grid", who, a.T);
        return (int)SR_EUNSUPPORTED;
    }
    return reverse ? sr_launch(sr_rollout_explore_vjp_kernel, dim3((unsigned)grid), dim3(XPL_BT), 0, s, a)
                   : sr_launch(sr_rollout_explore_kernel, dim3((unsigned)grid), dim3(XPL_BT), 0, s, a);
}
