// sr_rollout_constraints.hip -- the constraint vector of SimpleSafeMPC.generate_safety_constraints over a stored roll-out
// (sr_rollout_constraints) and its reverse pass (sr_rollout_constraints_vjp): control bounds on the ellipsoid of controls, obstacle
// half-spaces on every intermediate ellipsoid, the terminal safe set on the last one (safempc_simple.py:317-392, 488-532 of the
// reference; every row is a lin_ellipsoid_safety_distance), one launch each.
//
//   sr_rollout_constraints_kernel       one thread per (trajectory, step) pair writes the rows of step i: its 2 n_u control rows
//                                       (from (q_all[i-1], k_fb[i-1]); step 0 from (q0, k_fb0) or the point) and the obstacle rows
//                                       of state i, for i = H - 1 the terminal rows.  A workgroup owns max(1, BT / H) whole
//                                       trajectories; the largest row of a round of BT pairs goes through LDS and the trajectory's
//                                       owner thread takes the maximum in the order i = 0 .. H - 1 (NaN once any row is NaN).
//   sr_rollout_constraints_vjp_kernel   one thread per (trajectory, STATE) pair, so that every output element has one writer:
//                                       thread (t, i) takes the obstacle / terminal rows on (p_i, q_i) and the square-root parts of
//                                       the control rows of step i + 1 (K = k_fb[i], Q = q_all[i]) and writes p_all_bar[t, i],
//                                       q_all_bar[t, i], kfb_bar[t, i]; kff_bar[t, i] is the difference of two seeds; with q0 one
//                                       pseudo-state per trajectory writes q0_bar, kfb0_bar.
// The state rows go through sr_safety_row (sr_ellipsoid_dev.h), the function sr_safety_kernel calls: at a symmetric q they are the
// bits of sr_safety_distance.  The reverse pass keeps the lower triangle of a state's q_bar and the vector Q k in LDS, element-major
// with the threads of the block innermost (a thread's own column: no bank conflicts, no dynamically indexed private array, no
// scratch memory: profiles/r27_rollout_constraints_resources.txt).  h_*_mat, u_min, u_max are read at wave-uniform addresses.  No
// atomics, no waiting between workgroups; a thread's sums run in a fixed order (state rows r = 0 .., then control outputs
// j = 0 ..): the same bits on every call and whatever else is in the batch.
//
// Reverse, per row with s = sqrt(h Q_s h^T), Q_s the symmetric part:  d / d p = g_bar h,  d / d Q = c g_bar h^T h / (2 s);  per
// control output j with g+ = g_bar_upper + g_bar_lower, k = K[j, :]:  d / d k_ff[j] = g_bar_upper - g_bar_lower,
// d / d k = c g+ Q_s k^T / s_j,  d / d Q = c g+ k^T k / (2 s_j).  A radicand that is exactly zero contributes zero through its
// square root (include/safereach.h says why); a negative one NaN, in the outputs of its own (trajectory, state) only.
#include "sr_common.h"
#include "sr_dispatch.h"
#include "sr_ellipsoid_dev.h"

#define RCN_BT 64                                            // the forward's workgroup
#define RCN_AT(M, i, j) M[((i) * NT + (j)) * BT + threadIdx.x]
#define RCN_V(v, k) v[(k) * BT + threadIdx.x]
// the reverse pass's block size per width bucket: NT^2 + NT doubles of LDS per thread (10, 36, 39 KB per workgroup)
template <int NT> struct rcn_bt { static constexpr int value = NT <= 8 ? 64 : 32; };

// max that keeps a NaN: fmax would swallow it
__device__ static inline double rcn_max(double m, double v) { return (v > m || v != v) ? v : m; }
// 1 / sqrt of a radicand, 0 for a radicand that is exactly zero (the truncated slope), NaN for a negative one
__device__ static inline double rcn_rsqrt(double quad) { return quad == 0.0 ? 0.0 : 1.0 / sqrt(quad); }

__global__ __launch_bounds__(RCN_BT) void sr_rollout_constraints_kernel(sr_rcn_args a) {
    __shared__ double term[RCN_BT];
    const int H = a.H, n_s = a.n_s, n_u = a.n_u, tid = threadIdx.x;
    const int nc = a.bounds ? 2 * n_u : 0;                      // control rows per step
    const long nss = (long)n_s * n_s, t0 = (long)blockIdx.x * a.G;
    const int ng = (int)(a.T - t0 < a.G ? a.T - t0 : a.G);     // trajectories of this workgroup; ng H <= max(RCN_BT, H)
    const int nitem = ng * H;
    double acc = -INFINITY;
    for (int base = 0; base < nitem; base += RCN_BT) {
        const int e = base + tid;
        if (e < nitem) {
            const long n = t0 * H + e, t = t0 + e / H;          // pair (t, i)
            const int i = e % H;
            double* g = a.g + t * a.n_g;
            double mx = -INFINITY;
            if (a.bounds) {
                const double* Q = i ? a.q_all + (n - 1) * nss : (a.q0 ? a.q0 + t * nss : nullptr);
                const double* K = i ? a.k_fb + (t * (H - 1) + i - 1) * n_u * n_s : (a.q0 ? a.kfb0 + t * n_u * n_s : nullptr);
                const double* u = a.k_ff + n * n_u;
                double* gc = g + (long)i * nc;
                for (int j = 0; j < n_u; ++j) {
                    double r = 0.0;
                    if (Q) {
                        const double* k = K + j * n_s;
                        double quad = 0.0;
                        for (int p = 0; p < n_s; ++p) {
                            double s = 0.0;
                            for (int q = 0; q < n_s; ++q) s = fma(0.5 * (Q[p * n_s + q] + Q[q * n_s + p]), k[q], s);
                            quad = fma(s, k[p], quad);
                        }
                        r = a.c * sqrt(quad);
                    }
                    const double up = u[j] + r - a.u_max[j], lo = a.u_min[j] - u[j] + r;
                    gc[j] = up;
                    gc[n_u + j] = lo;
                    mx = rcn_max(rcn_max(mx, up), lo);
                }
            }
            const bool last = i == H - 1;
            const int m = last ? a.m_safe : a.m_obs;
            const double* hm = last ? a.h_safe_mat : a.h_obs_mat;
            const double* hv = last ? a.h_safe : a.h_obs;
            const double* pt = a.p_all + n * n_s;
            const double* qt = a.q_all + n * nss;
            double* gs = g + (long)nc * H + (long)a.m_obs * i;  // (i = H - 1: behind the m_obs (H - 1) obstacle rows)
            for (int r = 0; r < m; ++r) {
                double quad;
                const double v = sr_safety_row(hm + r * n_s, pt, [&](int p, int q) { return 0.5 * (qt[p * n_s + q] + qt[q * n_s + p]); },
                                               n_s, a.c, hv[r], quad);
                gs[r] = v;
                mx = rcn_max(mx, v);
            }
            term[tid] = mx;
        }
        __syncthreads();
        if (tid < ng) {                                         // the owner of trajectory t0 + tid: its steps of this round, in order
            const int lo = tid * H > base ? tid * H : base;
            int hi = (tid + 1) * H;
            if (hi > base + RCN_BT) hi = base + RCN_BT;
            for (int k = lo; k < hi; ++k) acc = rcn_max(acc, term[k - base]);
        }
        __syncthreads();
    }
    if (a.g_max && tid < ng) a.g_max[t0 + tid] = acc;
}

template <int NT>
__global__ __launch_bounds__(rcn_bt<NT>::value) void sr_rollout_constraints_vjp_kernel(sr_rcn_args a) {
    constexpr int BT = rcn_bt<NT>::value;
    __shared__ double qb[NT * NT * BT], wv[NT * BT];
    const int H = a.H, n_s = a.n_s, n_u = a.n_u;
    const int HH = H + (a.q0 ? 1 : 0);                          // states per trajectory, the pseudo-state of (q0, k_fb0) last
    const long n = (long)blockIdx.x * BT + threadIdx.x;
    if (n >= a.T * HH) return;
    const long t = n / HH, nss = (long)n_s * n_s;
    const int i = (int)(n % HH);
    const bool pseudo = i == H;
    const int nc = a.bounds ? 2 * n_u : 0;
    const double* gb = a.g_bar + t * a.n_g;
    const double c = a.c;
    // the state rows on (p_i, q_i): obstacle rows, for i = H - 1 the terminal rows; none on the pseudo-state
    const bool last = i == H - 1;
    const int m = pseudo ? 0 : (last ? a.m_safe : a.m_obs);
    const double* hm = last ? a.h_safe_mat : a.h_obs_mat;
    const double* gs = gb + (long)nc * H + (long)a.m_obs * i;
    if (!pseudo) {
        if (a.kff_bar)
            for (int j = 0; j < n_u; ++j)
                a.kff_bar[(t * H + i) * n_u + j] = a.bounds ? gb[(long)i * nc + j] - gb[(long)i * nc + n_u + j] : 0.0;
        if (a.p_all_bar)
            for (int p = 0; p < n_s; ++p) {
                double v = 0.0;
                for (int r = 0; r < m; ++r) v = fma(gs[r], hm[r * n_s + p], v);
                a.p_all_bar[(t * H + i) * n_s + p] = v;
            }
    }
    // the control rows whose square root reads this state: those of step i + 1, for the pseudo-state those of step 0
    const int step = pseudo ? 0 : i + 1;
    const bool ctrl = a.bounds && step < H;
    const double* Q = pseudo ? a.q0 + t * nss : a.q_all + (t * H + i) * nss;
    const double* K = !ctrl ? nullptr : (pseudo ? a.kfb0 + t * n_u * n_s : a.k_fb + (t * (H - 1) + i) * n_u * n_s);
    double* Qb = pseudo ? a.q0_bar + t * nss : (a.q_all_bar ? a.q_all_bar + (t * H + i) * nss : nullptr);
    double* Kb = pseudo ? a.kfb0_bar + t * n_u * n_s : ((a.kfb_bar && i < H - 1) ? a.kfb_bar + (t * (H - 1) + i) * n_u * n_s : nullptr);
    if (!Qb && !Kb) return;
    auto qs = [&](int p, int q) { return 0.5 * (Q[p * n_s + q] + Q[q * n_s + p]); };
    if (Qb) {
        for (int p = 0; p < n_s; ++p)
            for (int q = 0; q <= p; ++q) RCN_AT(qb, p, q) = 0.0;
        for (int r = 0; r < m; ++r) {
            const double* h = hm + r * n_s;
            double quad = 0.0;
            for (int p = 0; p < n_s; ++p) {
                double s = 0.0;
                for (int q = 0; q < n_s; ++q) s = fma(qs(p, q), h[q], s);
                quad = fma(s, h[p], quad);
            }
            const double cf = 0.5 * c * gs[r] * rcn_rsqrt(quad);
            for (int p = 0; p < n_s; ++p) {
                const double cp = cf * h[p];
                for (int q = 0; q <= p; ++q) RCN_AT(qb, p, q) = fma(cp, h[q], RCN_AT(qb, p, q));
            }
        }
    }
    for (int j = 0; j < n_u; ++j) {
        if (!ctrl) {                                            // no bounds: k_fb is not read by any row
            if (Kb)
                for (int p = 0; p < n_s; ++p) Kb[j * n_s + p] = 0.0;
            continue;
        }
        const double* k = K + j * n_s;
        double quad = 0.0;
        for (int p = 0; p < n_s; ++p) {
            double s = 0.0;
            for (int q = 0; q < n_s; ++q) s = fma(qs(p, q), k[q], s);
            RCN_V(wv, p) = s;
            quad = fma(s, k[p], quad);
        }
        const double cf = c * (gb[(long)step * nc + j] + gb[(long)step * nc + n_u + j]) * rcn_rsqrt(quad);
        if (Kb)
            for (int p = 0; p < n_s; ++p) Kb[j * n_s + p] = cf * RCN_V(wv, p);
        if (Qb)
            for (int p = 0; p < n_s; ++p) {
                const double cp = 0.5 * cf * k[p];
                for (int q = 0; q <= p; ++q) RCN_AT(qb, p, q) = fma(cp, k[q], RCN_AT(qb, p, q));
            }
    }
    if (Qb)
        for (int p = 0; p < n_s; ++p)
            for (int q = 0; q <= p; ++q) {
                const double v = RCN_AT(qb, p, q);
                Qb[p * n_s + q] = v;
                Qb[q * n_s + p] = v;
            }
}
#undef RCN_AT
#undef RCN_V

int sr_launch_rollout_constraints(sr_rcn_args a, bool reverse, hipStream_t s) {
    const char* who = reverse ? "sr_rollout_constraints_vjp" : "sr_rollout_constraints";
    if (!reverse) {
        a.G = a.H >= RCN_BT ? 1 : RCN_BT / a.H;
        const long grid = (a.T + a.G - 1) / a.G;
        if (grid > 2147483647L) {
            sr_set_error("%s: T=%ld H=%d beyond the launch grid", who, a.T, a.H);
            return (int)SR_EUNSUPPORTED;
        }
        return sr_launch(sr_rollout_constraints_kernel, dim3((unsigned)grid), dim3(RCN_BT), 0, s, a);
    }
    return sr_pick_le<4, 8, 12>(who, a.n_s, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, BT = rcn_bt<NT>::value;
        const long grid = (a.T * (a.H + (a.q0 ? 1 : 0)) + BT - 1) / BT;
        if (grid > 2147483647L) {
            sr_set_error("%s: T=%ld H=%d beyond the launch grid", who, a.T, a.H);
            return (int)SR_EUNSUPPORTED;
        }
        return sr_launch(sr_rollout_constraints_vjp_kernel<NT>, dim3((unsigned)grid), dim3(BT), 0, s, a);
    });
}
