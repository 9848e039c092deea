// sr_rollout_cost.hip -- the MPC objective over a stored moment trajectory (sr_rollout_cost) and its reverse pass
// (sr_rollout_cost_vjp): generic_cost with trig_aug as the state transformation and loss_sat / loss_quadratic as stage and
// terminal cost (utils_casadi.py:178-395 of the reference), one launch each.
//
//   sr_rollout_cost_kernel       one thread per (trajectory, step) pair computes the step's term; a workgroup owns max(1, BT / H)
//                                whole trajectories, the terms of a round of BT pairs go through LDS and the trajectory's owner
//                                thread adds them in the order i = 0 .. H - 1.
//   sr_rollout_cost_vjp_kernel   one thread per pair: the same factorisation, then the closed-form gradient in (mu, sigma, u).
// A pair's n_c x n_c algebra lives in LDS, element-major with the threads of the block innermost (a thread's own column: no bank
// conflicts, no dynamically indexed private array, no scratch memory: profiles/r25_rollout_cost_resources.txt).  F is read at
// wave-uniform addresses.  No atomics, no waiting between workgroups; a thread's sums run in a fixed order and a trajectory's
// total is added by one thread: the same bits on every call and whatever else is in the batch.
//
// Per pair, with (m, v) the state, v read as (v + v^T) / 2 (NULL: zero):
//   augmentation   theta = m[idx], s2 = v[idx][idx], e = exp(-s2), x = -expm1(-s2), h = exp(-s2 / 2):
//                  m_trig = a h [sin, cos];  v_trig = a^2 x / 2 [[1 + e cos 2theta, -e sin 2theta], [., 1 - e cos 2theta]] (the
//                  reference's E[.^2] - E[.]^2 with the cancellation removed: exactly zero at s2 = 0);  C = v[:, idx] (x) [a h cos,
//                  -a h sin];  state [m; m_trig], [[v, C], [C^T, v_trig]], row and column idx deleted unless keep_radian.
//   saturating     W = F F^T, E = F^T S F, I + E = L L^T (SPD for any PSD S; nothing inverts S, W or I + S W), y = L^-1 F^T d:
//                  loss = -expm1(-|y|^2 / 2 - sum_k log L_kk).  The pivots are formed as 1 + delta_k and their logarithms as
//                  log1p(delta_k) / 2, so that a loss of 1e-9 keeps its digits.
//   quadratic      |F^T d|^2 + tr E.
//   reverse        G = L^-1 F^T (quadratic: F^T), g = G^T y, q = 1 - loss:  d loss / d m_aug = q g (2 g),  d loss / d S_aug =
//                  q (G^T G - g g^T) / 2 (G^T G), formed for i >= j and stored in both halves; then back through the augmentation.
#include "sr_common.h"
#include "sr_dispatch.h"

#define RC_AT(M, i, j) M[((i) * CT + (j)) * BT + threadIdx.x]
#define RC_V(v, k) v[(k) * BT + threadIdx.x]
// block size per width bucket: 2 CT^2 + 3 CT doubles of LDS per thread, under 64 KB per workgroup (22, 45, 58, 54 KB)
template <int CT> struct rc_bt { static constexpr int value = CT <= 6 ? 64 : (CT <= 10 ? 32 : 16); };

struct rc_trig { double ms, mc, e, x, s2t, c2t, aa; };      // a h sin, a h cos, exp(-s2), -expm1(-s2), sin 2 theta, cos 2 theta, a^2

// augmented index p < n_k -> index of the original state
__device__ static inline int rc_orig(const sr_cost_args& a, int p) { return (a.idx < 0 || a.keep || p < a.idx) ? p : p + 1; }
// number of original coordinates the augmented state keeps
__device__ static inline int rc_nk(const sr_cost_args& a) { return (a.idx < 0 || a.keep) ? a.n_s : a.n_s - 1; }
// symmetric part of the stored covariance
__device__ static inline double rc_vs(const double* sg, int n_s, int i, int j) {
    return sg ? 0.5 * (sg[i * n_s + j] + sg[j * n_s + i]) : 0.0;
}

// The loss of pair (t, i).  On return dv = d, yv = y (saturating: L^-1 F^T d, quadratic: F^T d), S holds L in its lower triangle
// (saturating) or E (quadratic); P is overwritten.
template <int CT, int BT>
__device__ static inline double rc_loss(const sr_cost_args& a, const double* m, const double* sg, double* S, double* P, double* dv,
                                        double* yv, rc_trig& tr) {
    const int n_s = a.n_s, n_c = a.n_c, n_k = rc_nk(a), idx = a.idx;
    const double* F = a.F;
    for (int p = 0; p < n_k; ++p) {
        const int op = rc_orig(a, p);
        RC_V(dv, p) = m[op] - a.z[p];
        for (int q = 0; q <= p; ++q) {
            const double v = rc_vs(sg, n_s, op, rc_orig(a, q));
            RC_AT(S, p, q) = v;
            RC_AT(S, q, p) = v;
        }
    }
    if (idx >= 0) {
        const double s2 = sg ? sg[idx * n_s + idx] : 0.0, h = exp(-0.5 * s2);
        double sn, cs;
        sincos(m[idx], &sn, &cs);
        tr.ms = a.a_trig * h * sn;
        tr.mc = a.a_trig * h * cs;
        tr.e = exp(-s2);
        tr.x = -expm1(-s2);
        tr.s2t = 2.0 * sn * cs;
        tr.c2t = (cs - sn) * (cs + sn);
        tr.aa = a.a_trig * a.a_trig;
        RC_V(dv, n_k) = tr.ms - a.z[n_k];
        RC_V(dv, n_k + 1) = tr.mc - a.z[n_k + 1];
        for (int p = 0; p < n_k; ++p) {
            const double vk = rc_vs(sg, n_s, rc_orig(a, p), idx);
            RC_AT(S, p, n_k) = vk * tr.mc;
            RC_AT(S, n_k, p) = vk * tr.mc;
            RC_AT(S, p, n_k + 1) = -vk * tr.ms;
            RC_AT(S, n_k + 1, p) = -vk * tr.ms;
        }
        const double hx = 0.5 * tr.aa * tr.x;
        RC_AT(S, n_k, n_k) = hx * (1.0 + tr.e * tr.c2t);
        RC_AT(S, n_k + 1, n_k + 1) = hx * (1.0 - tr.e * tr.c2t);
        RC_AT(S, n_k, n_k + 1) = -hx * tr.e * tr.s2t;
        RC_AT(S, n_k + 1, n_k) = -hx * tr.e * tr.s2t;
    }
    // P = S F;  E = F^T P (lower triangle, over S);  y = F^T d
    for (int i = 0; i < n_c; ++i)
        for (int j = 0; j < n_c; ++j) {
            double v = 0.0;
            for (int k = 0; k < n_c; ++k) v = fma(RC_AT(S, i, k), F[k * n_c + j], v);
            RC_AT(P, i, j) = v;
        }
    double tr_e = 0.0, yy = 0.0;
    for (int i = 0; i < n_c; ++i) {
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = 0; k < n_c; ++k) v = fma(F[k * n_c + i], RC_AT(P, k, j), v);
            RC_AT(S, i, j) = v;
        }
        tr_e += RC_AT(S, i, i);
        double v = 0.0;
        for (int k = 0; k < n_c; ++k) v = fma(F[k * n_c + i], RC_V(dv, k), v);
        RC_V(yv, i) = v;
        yy = fma(v, v, yy);
    }
    if (a.loss == 1) return yy + tr_e;
    // I + E = L L^T in place; the pivot as 1 + delta, half its logarithm as log1p(delta) / 2
    double lsum = 0.0;
    for (int k = 0; k < n_c; ++k) {
        double dl = RC_AT(S, k, k);
        for (int p = 0; p < k; ++p) dl -= RC_AT(S, k, p) * RC_AT(S, k, p);
        lsum += 0.5 * log1p(dl);
        const double l = sqrt(1.0 + dl), inv = 1.0 / l;
        RC_AT(S, k, k) = l;
        for (int i = k + 1; i < n_c; ++i) {
            double v = RC_AT(S, i, k);
            for (int p = 0; p < k; ++p) v -= RC_AT(S, i, p) * RC_AT(S, k, p);
            RC_AT(S, i, k) = v * inv;
        }
    }
    yy = 0.0;
    for (int i = 0; i < n_c; ++i) {
        double v = RC_V(yv, i);
        for (int p = 0; p < i; ++p) v -= RC_AT(S, i, p) * RC_V(yv, p);
        v /= RC_AT(S, i, i);
        RC_V(yv, i) = v;
        yy = fma(v, v, yy);
    }
    return -expm1(-0.5 * yy - lsum);
}

// u^T R u of pair (t, i)
__device__ static inline double rc_control(const sr_cost_args& a, const double* u) {
    double c = 0.0;
    for (int i = 0; i < a.n_u; ++i) {
        double v = 0.0;
        for (int j = 0; j < a.n_u; ++j) v = fma(a.R[i * a.n_u + j], u[j], v);
        c = fma(u[i], v, c);
    }
    return c;
}

template <int CT>
__global__ __launch_bounds__(rc_bt<CT>::value) void sr_rollout_cost_kernel(sr_cost_args a) {
    constexpr int BT = rc_bt<CT>::value;
    __shared__ double S[CT * CT * BT], P[CT * CT * BT], dv[CT * BT], yv[CT * BT], term[BT];
    const int H = a.H, tid = threadIdx.x;
    const long t0 = (long)blockIdx.x * a.G;
    const int ng = (int)(a.T - t0 < a.G ? a.T - t0 : a.G);     // trajectories of this workgroup; ng H <= max(BT, H)
    const int nitem = ng * H;
    double acc = 0.0;
    for (int base = 0; base < nitem; base += BT) {
        const int e = base + tid;
        if (e < nitem) {
            const long n = t0 * H + e;                          // pair (t, i) = (n / H, n % H)
            const int i = e % H;
            const bool last = i == H - 1;
            rc_trig tr = {};
            const double l = rc_loss<CT, BT>(a, a.mu + n * a.n_s, a.sigma ? a.sigma + n * a.n_s * a.n_s : nullptr, S, P, dv, yv, tr);
            double c = (last ? a.w_term : a.w_stage) * l;
            if (a.R && !last) c += rc_control(a, a.u + n * a.n_u);
            term[tid] = c;
            if (a.cost_steps) a.cost_steps[n] = c;
        }
        __syncthreads();
        if (tid < ng) {                                         // the owner of trajectory t0 + tid: its terms of this round, in order
            const int lo = tid * H > base ? tid * H : base;
            int hi = (tid + 1) * H;
            if (hi > base + BT) hi = base + BT;
            for (int k = lo; k < hi; ++k) acc += term[k - base];
        }
        __syncthreads();
    }
    if (tid < ng) a.cost[t0 + tid] = acc;
}

template <int CT>
__global__ __launch_bounds__(rc_bt<CT>::value) void sr_rollout_cost_vjp_kernel(sr_cost_args a) {
    constexpr int BT = rc_bt<CT>::value;
    __shared__ double S[CT * CT * BT], P[CT * CT * BT], dv[CT * BT], yv[CT * BT], gv[CT * BT];
    const long n = (long)blockIdx.x * BT + threadIdx.x;
    if (n >= a.T * a.H) return;
    const long t = n / a.H;
    const int i = (int)(n % a.H), n_s = a.n_s, n_c = a.n_c, n_u = a.n_u, n_k = rc_nk(a), idx = a.idx;
    const bool last = i == a.H - 1;
    const double cb = a.cost_bar ? a.cost_bar[t] : 1.0;
    if (a.u_bar) {
        double* ub = a.u_bar + n * n_u;
        const double* u = a.u ? a.u + n * n_u : nullptr;
        for (int k = 0; k < n_u; ++k) {
            double v = 0.0;
            if (a.R && !last)
                for (int j = 0; j < n_u; ++j) v = fma(a.R[k * n_u + j] + a.R[j * n_u + k], u[j], v);
            ub[k] = (a.R && !last) ? cb * v : 0.0;
        }
    }
    if (!a.mu_bar && !a.sigma_bar) return;
    const double* m = a.mu + n * n_s;
    const double* sg = a.sigma ? a.sigma + n * n_s * n_s : nullptr;
    const double* F = a.F;
    rc_trig tr = {};
    const double l = rc_loss<CT, BT>(a, m, sg, S, P, dv, yv, tr);
    const double w = (last ? a.w_term : a.w_stage) * cb;
    const bool sat = a.loss == 0;
    // G = L^-1 F^T (saturating) or F^T, over P
    for (int j = 0; j < n_c; ++j)
        for (int r = 0; r < n_c; ++r) {
            double v = F[j * n_c + r];
            if (sat) {
                for (int p = 0; p < r; ++p) v -= RC_AT(S, r, p) * RC_AT(P, p, j);
                v /= RC_AT(S, r, r);
            }
            RC_AT(P, r, j) = v;
        }
    // g = G^T y;  the seeds of the augmented state: gm = cm g over gv, GS = cs (G^T G - sub g g^T) over S, both halves
    const double cm = sat ? w * (1.0 - l) : 2.0 * w, cs = sat ? 0.5 * w * (1.0 - l) : w;
    for (int j = 0; j < n_c; ++j) {
        double v = 0.0;
        for (int k = 0; k < n_c; ++k) v = fma(RC_AT(P, k, j), RC_V(yv, k), v);
        RC_V(dv, j) = v;
        RC_V(gv, j) = cm * v;
    }
    for (int r = 0; r < n_c; ++r)
        for (int c = 0; c <= r; ++c) {
            double v = sat ? -RC_V(dv, r) * RC_V(dv, c) : 0.0;
            for (int k = 0; k < n_c; ++k) v = fma(RC_AT(P, k, r), RC_AT(P, k, c), v);
            RC_AT(S, r, c) = cs * v;
            RC_AT(S, c, r) = cs * v;
        }
    // back through the augmentation: seeds Ms, Mc on the two trigonometric means (their own and the cross block's), then theta, s2
    double g_th = 0.0, g_s2 = 0.0;
    if (idx >= 0) {
        double Ms = RC_V(gv, n_k), Mc = RC_V(gv, n_k + 1);
        for (int p = 0; p < n_k; ++p) {
            const double vk = rc_vs(sg, n_s, rc_orig(a, p), idx);
            Ms -= 2.0 * RC_AT(S, p, n_k + 1) * vk;
            Mc += 2.0 * RC_AT(S, p, n_k) * vk;
        }
        const double gss = RC_AT(S, n_k, n_k), gcc = RC_AT(S, n_k + 1, n_k + 1), gsc = 2.0 * RC_AT(S, n_k + 1, n_k);
        const double axe = tr.aa * tr.x * tr.e, hae = 0.5 * tr.aa * tr.e, k2 = 2.0 * tr.e - 1.0;
        g_th = Ms * tr.mc - Mc * tr.ms + axe * (tr.s2t * (gcc - gss) - tr.c2t * gsc);
        g_s2 = -0.5 * (Ms * tr.ms + Mc * tr.mc)
             + hae * (gss * (1.0 + tr.c2t * k2) + gcc * (1.0 - tr.c2t * k2) - gsc * tr.s2t * k2);
    }
    // (augmented index of an original coordinate: the inverse of rc_orig; the angle itself only with keep_radian)
    auto aug = [&](int r) { return (idx < 0 || a.keep || r < idx) ? r : r - 1; };
    const bool has_idx_row = idx >= 0 && a.keep;
    if (a.mu_bar) {
        double* mb = a.mu_bar + n * n_s;
        for (int r = 0; r < n_s; ++r) {
            double v = (r != idx || has_idx_row) ? RC_V(gv, aug(r)) : 0.0;
            if (r == idx) v += g_th;
            mb[r] = v;
        }
    }
    if (a.sigma_bar) {
        double* sb = a.sigma_bar + n * n_s * n_s;
        for (int r = 0; r < n_s; ++r)
            for (int c = 0; c < n_s; ++c) {
                const bool rin = r != idx || has_idx_row, cin = c != idx || has_idx_row;
                double v = (rin && cin) ? RC_AT(S, aug(r), aug(c)) : 0.0;
                if (idx >= 0 && (r == idx || c == idx)) {
                    // cross block: C[k] = v[k][idx] [mc, -ms] sits in both halves of the augmented matrix, and v[k][idx] is the
                    // mean of two stored entries: each of them takes h_k = GS[k][sin] mc - GS[k][cos] ms, the diagonal 2 h_idx
                    const int k = r == idx ? c : r;
                    const bool kin = k != idx || has_idx_row;
                    const double hk = kin ? RC_AT(S, aug(k), n_k) * tr.mc - RC_AT(S, aug(k), n_k + 1) * tr.ms : 0.0;
                    v += (r == idx && c == idx) ? 2.0 * hk + g_s2 : hk;
                }
                sb[r * n_s + c] = v;
            }
    }
}
#undef RC_AT
#undef RC_V

int sr_launch_rollout_cost(sr_cost_args a, bool reverse, hipStream_t s) {
    const char* who = reverse ? "sr_rollout_cost_vjp" : "sr_rollout_cost";
    return sr_pick_le<4, 6, 10, 14>(who, a.n_c, [&](auto ct) {
        constexpr int CT = decltype(ct)::value, BT = rc_bt<CT>::value;
        a.G = a.H >= BT ? 1 : BT / a.H;
        const long grid = reverse ? (a.T * a.H + BT - 1) / BT : (a.T + a.G - 1) / a.G;
        if (grid > 2147483647L) {
            sr_set_error("%s: T=%ld H=%d beyond the launch grid", who, a.T, a.H);
            return (int)SR_EUNSUPPORTED;
        }
        return reverse ? sr_launch(sr_rollout_cost_vjp_kernel<CT>, dim3((unsigned)grid), dim3(BT), 0, s, a)
                       : sr_launch(sr_rollout_cost_kernel<CT>, dim3((unsigned)grid), dim3(BT), 0, s, a);
    });
}
