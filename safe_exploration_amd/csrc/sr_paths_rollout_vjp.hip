// sr_paths_rollout_vjp.hip -- the reverse pass of the closed-loop roll-out of the posterior function samples
// (sr_gp_paths_rollout_vjp; the C-ABI and the algebra: include/safereach.h, the checks: sr_capi_paths.hip, the forward:
// sr_paths_rollout.hip KPO).  The forward is sequential in the step index; once its states X_all are stored the input of every
// (step, path) pair is known, so nothing transcendental is sequential here:
//
//   KRJ  sr_paths_rollout_jac_kernel     : J_i[s] = d f_s / d z at z_i[s] = [x_i[s], k_fb[i] x_i[s] + k_ff[i]] for ALL H S pairs in
//                                          one launch: one lane per path (c and w read coalesced along s, as KPT reads them),
//                                          the step a grid dimension, the N + M terms split over workgroups [exp / sin bound]
//   KRJS sr_paths_rollout_jac_sum_kernel : the splits in ascending order, one thread per element of J (as KPR<GRAD>)
//   KRS  sr_paths_rollout_sweep_kernel   : one lane per path runs lambda <- X_bar[i-1] + J_x^T lambda + k_fb[i]^T J_u^T lambda
//                                          from i = H - 1 down to 0 in registers; per step the workgroup's sum of g_u and
//                                          g_u x_i^T in a fixed tree (64 lanes by shuffles, then the four waves in order): one
//                                          record per workgroup
//   KRF  sr_paths_rollout_fin_kernel     : the workgroups' records in ascending order into k_ff_bar, k_fb_bar (and x0_bar of a
//                                          shared start)
// No atomics: the same inputs give the same bits.  KRS reads J through three strides -- the caller's J_all (H x S x n_s x D) or the
// workspace copy with the path index fastest -- so that the gradients are the same bits with and without J_all.
// The formulas per term, their scalings and the prefactors at the end of KRJ are those of KPT<GRAD> (sr_paths.hip) without the
// value: exp for the training rows, sin for the features, no cos.  Padded paths (s >= S) contribute exact zeros.
#include "sr_common.h"
#include "sr_kernel_dev.h"

#define SR_RVJP_ZT 256               /* rows of Z resp. omega per LDS tile: one per thread */

template <int DT>
__global__ __launch_bounds__(256) void sr_paths_rollout_jac_kernel(sr_paths_rollout_vjp_args a) {
    __shared__ double rows[SR_RVJP_ZT * DT];
    __shared__ double ta[SR_RVJP_ZT];
    const int n_out = a.m.n_out, D = a.m.D, n_u = D - n_out;
    const int i = blockIdx.y, d = blockIdx.z % n_out, sp = blockIdx.z / n_out;
    const int sq = blockIdx.x * 256 + threadIdx.x;
    const bool live = sq < a.S;
    const int off = a.Np - a.N;
    // the input of step i as the forward forms it: the state from x0 resp. X_all[i - 1], u_q = k_ff[i][q] + sum_c k_fb[i][q][c] x_c
    double x[DT], inv_l[DT];
    {
        const double* xp = (i == 0) ? a.x0 + (a.x0_per_path ? (long)sq * n_out : 0) : a.X_all + ((long)(i - 1) * a.S + sq) * n_out;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            inv_l[j] = (j < D) ? 1.0 / a.m.ls[d * D + j] : 0.0;
            x[j] = (live && j < n_out) ? xp[j] : 0.0;
        }
#pragma unroll
        for (int j = 1; j < DT; ++j)
            if (j >= n_out && j < D) {
                const int q = j - n_out;
                const double* kb = a.k_fb + ((long)i * n_u + q) * n_out;
                double u = a.k_ff[(long)i * n_u + q];
#pragma unroll
                for (int c = 0; c < j; ++c)
                    if (c < n_out) u = fma(kb[c], x[c], u);
                x[j] = u;
            }
    }
    const int total = a.N + a.m.M;
    const int per = (total + a.nsplit - 1) / a.nsplit;
    const int e_beg = sp * per, e_end = min(total, e_beg + per);
    double gk[DT], gf[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) gk[j] = gf[j] = 0.0;
    // training rows [e_beg, min(e_end, N)): sum_r exp(-r2 / 2) c_r (z_rj - x_j) / l_j, times sf2 / l_j at the end
    {
        double xs[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) xs[j] = x[j] * inv_l[j];
        const int i_end = min(e_end, a.N);
        const double* cc = a.C + ((long)d * a.Np + off) * a.Sp + (live ? sq : 0);
        for (int i0 = e_beg; i0 < i_end; i0 += SR_RVJP_ZT) {
            const int nrow = min(SR_RVJP_ZT, i_end - i0);
            __syncthreads();
            if ((int)threadIdx.x < nrow) {
#pragma unroll
                for (int j = 0; j < DT; ++j)
                    rows[threadIdx.x * DT + j] = (j < D) ? a.Z[(long)(i0 + threadIdx.x) * D + j] * inv_l[j] : 0.0;
            }
            __syncthreads();
            if (!live) continue;
#pragma unroll 4
            for (int r = 0; r < nrow; ++r) {
                double r2 = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    const double df = xs[j] - rows[r * DT + j];
                    r2 = fma(df, df, r2);
                }
                const double kc = sr_kappa(0, r2) * cc[(long)(i0 + r) * a.Sp];
#pragma unroll
                for (int j = 0; j < DT; ++j) gk[j] = fma(kc, rows[r * DT + j] - xs[j], gk[j]);
            }
        }
    }
    // features [max(e_beg, N) - N, e_end - N): sum_r sin(omega_r . (x / l) + tau_r) w_r omega_rj, times -sqrt(2 sf2 / M) / l_j
    {
        double xs[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) xs[j] = (j < D) ? x[j] / a.m.ls[d * D + j] : 0.0;
        const int f_beg = max(e_beg, a.N) - a.N, f_end = e_end - a.N;
        const double* ww = a.Wk + (long)d * a.m.Mp * a.Sp + (live ? sq : 0);
        for (int i0 = f_beg; i0 < f_end; i0 += SR_RVJP_ZT) {
            const int nrow = min(SR_RVJP_ZT, f_end - i0);
            __syncthreads();
            if ((int)threadIdx.x < nrow) {
#pragma unroll
                for (int j = 0; j < DT; ++j)
                    rows[threadIdx.x * DT + j] = (j < D) ? a.m.omega[(long)(i0 + threadIdx.x) * D + j] : 0.0;
                ta[threadIdx.x] = a.m.tau[i0 + threadIdx.x];
            }
            __syncthreads();
            if (!live) continue;
#pragma unroll 4
            for (int r = 0; r < nrow; ++r) {
                double arg = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) arg = fma(rows[r * DT + j], xs[j], arg);
                const double sw = sin(arg + ta[r]) * ww[(long)(i0 + r) * a.Sp];
#pragma unroll
                for (int j = 0; j < DT; ++j) gf[j] = fma(sw, rows[r * DT + j], gf[j]);
            }
        }
    }
    if (live) {
        const double sf2 = a.m.sf2[d], amp = sqrt(2.0 * sf2 / (double)a.m.M);
        double* p = a.part + (((long)(sp * n_out + d) * D) * a.H + i) * a.Sp + sq;
#pragma unroll
        for (int j = 0; j < DT; ++j)
            if (j < D) p[(long)j * a.H * a.Sp] = fma(sf2 * inv_l[j], gk[j], -(amp * inv_l[j]) * gf[j]);
    }
}

// KRJS: blockIdx.y = d D + j, blockIdx.z = step: one element of J per thread, its splits in ascending order
__global__ __launch_bounds__(256) void sr_paths_rollout_jac_sum_kernel(sr_paths_rollout_vjp_args a) {
    const int sq = blockIdx.x * 256 + threadIdx.x;
    if (sq >= a.S) return;
    const int e = blockIdx.y, i = blockIdx.z;
    const long split = (long)a.m.n_out * a.m.D * a.H * a.Sp;
    const double* p = a.part + ((long)e * a.H + i) * a.Sp + sq;
    double g = 0.0;
#pragma unroll 8
    for (int sp = 0; sp < a.nsplit; ++sp) g += p[(long)sp * split];
    a.J[(long)i * a.j_si + (long)sq * a.j_ss + (long)e * a.j_se] = g;
}

// the sum of v over the 64 lanes of a wave in lane 0, in a fixed tree
__device__ __forceinline__ double rvjp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}

// KRS, one instance per (n_s, n_u) with n_s + n_u <= SR_PATHS_MAX_D: lambda, g_x, g_u and x_i live in registers and every loop
// over them has compile-time bounds (no dynamically indexed private array, and no branch around a load: the n_s (D + 2) loads of a
// step are issued together -- behind uniform branches each of them waited for the one before, 7.7 us per step at D = 5).  Dead lanes
// (s >= S) read path 0 and carry lambda = 0: exact zeros.  A step's sums go through one of two LDS buffers (step parity), so one
// barrier per step is enough.
template <int NS, int NU>
__global__ __launch_bounds__(SR_RVJP_BLOCK) void sr_paths_rollout_sweep_kernel(sr_paths_rollout_vjp_args a) {
    constexpr int D = NS + NU, NK = NU * (1 + NS), NW = SR_RVJP_BLOCK / 64;
    __shared__ double red[2][NW][NK];
    const int H = a.H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sq = blockIdx.x * SR_RVJP_BLOCK + tid;
    const bool live = sq < a.S;
    const long sr = live ? sq : 0;                       // the path whose data this lane reads
    double* rec = a.rec + (long)blockIdx.x * H * NK;
    double lam[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const double v = a.X_bar[((long)(H - 1) * a.S + sr) * NS + c];
        lam[c] = live ? v : 0.0;
    }
    for (int i = H - 1; i >= 0; --i) {
        const double* Jp = a.J + (long)i * a.j_si + sr * a.j_ss;
        const double* xp = (i == 0) ? a.x0 + (a.x0_per_path ? sr * NS : 0) : a.X_all + ((long)(i - 1) * a.S + sr) * NS;
        const double* bp = a.X_bar + ((long)(i >= 1 ? i - 1 : 0) * a.S + sr) * NS;
        const double* kb = a.k_fb + (long)i * NU * NS;
        double Jv[NS][D], xi[NS], xb[NS];
#pragma unroll
        for (int d = 0; d < NS; ++d) {
#pragma unroll
            for (int j = 0; j < D; ++j) Jv[d][j] = Jp[(long)(d * D + j) * a.j_se];
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            xi[c] = xp[c];
            xb[c] = bp[c];
        }
        // g = J_i[s]^T lambda, the outputs in ascending order
        double gx[NS], gu[NU];
#pragma unroll
        for (int c = 0; c < NS; ++c) gx[c] = 0.0;
#pragma unroll
        for (int q = 0; q < NU; ++q) gu[q] = 0.0;
#pragma unroll
        for (int d = 0; d < NS; ++d) {
#pragma unroll
            for (int c = 0; c < NS; ++c) gx[c] = fma(Jv[d][c], lam[d], gx[c]);
#pragma unroll
            for (int q = 0; q < NU; ++q) gu[q] = fma(Jv[d][NS + q], lam[d], gu[q]);
        }
        // this workgroup's share of k_ff_bar[i] (g_u) and k_fb_bar[i] (g_u x_i^T)
        double* rb = red[i & 1][wave];
#pragma unroll
        for (int q = 0; q < NU; ++q) {
            const double v = rvjp_wave_sum(gu[q]);
            if (lane == 0) rb[q] = v;
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                const double vx = rvjp_wave_sum(gu[q] * xi[c]);
                if (lane == 0) rb[NU + q * NS + c] = vx;
            }
        }
        __syncthreads();
        if (tid < NK) {
            double v = red[i & 1][0][tid];
#pragma unroll
            for (int w = 1; w < NW; ++w) v += red[i & 1][w][tid];
            rec[(long)i * NK + tid] = v;
        }
        // lambda = X_bar[i - 1][s] + g_x + k_fb[i]^T g_u
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            double t = gx[c];
#pragma unroll
            for (int q = 0; q < NU; ++q) t = fma(kb[q * NS + c], gu[q], t);
            lam[c] = (i >= 1 && live) ? xb[c] + t : t;
        }
    }
    if (a.x0_per_path) {
        if (live) {
#pragma unroll
            for (int c = 0; c < NS; ++c) a.x0_bar[(long)sq * NS + c] = lam[c];
        }
        return;
    }
    // a shared start: the sum over the paths through the same tree (buffer 1: step 0 used buffer 0, and every thread has passed
    // the barrier of step 0 since step 1 read buffer 1)
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        const double v = rvjp_wave_sum(lam[c]);
        if (lane == 0) red[1][wave][c] = v;
    }
    __syncthreads();
    if (tid < NS) {
        double v = red[1][0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) v += red[1][w][tid];
        a.rec[(long)gridDim.x * H * NK + (long)blockIdx.x * NS + tid] = v;
    }
}

// KRF: one thread per element of k_ff_bar, k_fb_bar (and of a shared start's x0_bar): the records in ascending order
__global__ __launch_bounds__(256) void sr_paths_rollout_fin_kernel(sr_paths_rollout_vjp_args a, int nblk) {
    const int n_s = a.m.n_out, n_u = a.m.D - n_s, nk = n_u * (1 + n_s);
    const long e = (long)blockIdx.x * 256 + threadIdx.x, ngain = (long)a.H * nk;
    if (e < ngain) {
        const long i = e / nk;
        const int k = (int)(e - i * nk);
        double v = 0.0;
        for (int b = 0; b < nblk; ++b) v += a.rec[(long)b * ngain + e];
        if (k < n_u) a.k_ff_bar[i * n_u + k] = v;
        else a.k_fb_bar[i * n_u * n_s + (k - n_u)] = v;
    } else if (e < ngain + n_s && !a.x0_per_path) {
        double v = 0.0;
        for (int b = 0; b < nblk; ++b) v += a.rec[(long)nblk * ngain + (long)b * n_s + (e - ngain)];
        a.x0_bar[e - ngain] = v;
    }
}

int sr_launch_paths_rollout_vjp(const sr_paths_rollout_vjp_args& a, hipStream_t s) {
    const int n_s = a.m.n_out, D = a.m.D, n_u = D - n_s;
    SR_CHECK(a.S >= 1 && a.S <= a.Sp && a.H >= 1 && n_s >= 1 && n_u >= 1 && D <= SR_PATHS_MAX_D && a.N >= 1 && a.m.M >= 1 &&
                 a.nsplit >= 1,
             SR_EINVAL, "paths_rollout_vjp: S=%d Sp=%d H=%d D=%d n_out=%d nsplit=%d", a.S, a.Sp, a.H, D, n_s, a.nsplit);
    SR_CHECK(a.H <= 65535 && (long)a.nsplit * n_s <= 65535, SR_EINVAL, "paths_rollout_vjp: H=%d, %d splits of %d outputs: a grid dimension past 65535",
             a.H, a.nsplit, n_s);
    const int sb = (a.S + 255) / 256, nblk = sr_paths_rollout_vjp_blocks(a.S);
    SR_TRY((sr_pick_le<3, 5, 8>("paths_rollout_vjp", D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return sr_launch(sr_paths_rollout_jac_kernel<DT>, dim3(sb, a.H, a.nsplit * n_s), dim3(256), 0, s, a); })));
    SR_TRY(sr_launch(sr_paths_rollout_jac_sum_kernel, dim3(sb, n_s * D, a.H), dim3(256), 0, s, a));
    // the sweep: the exact (n_s, n_u), every pair with n_s + n_u <= SR_PATHS_MAX_D
    SR_TRY((sr_pick_eq<1, 2, 3, 4, 5, 6, 7>("paths_rollout_vjp: n_out=%d", n_s, [&](auto ns) {
        return sr_pick_eq<1, 2, 3, 4, 5, 6, 7>("paths_rollout_vjp: n_u=%d", n_u, [&](auto nu) {
            constexpr int NS = decltype(ns)::value, NU = decltype(nu)::value;
            if constexpr (NS + NU <= SR_PATHS_MAX_D)
                return sr_launch(sr_paths_rollout_sweep_kernel<NS, NU>, dim3(nblk), dim3(SR_RVJP_BLOCK), 0, s, a);
            else
                return (int)SR_EUNSUPPORTED;             // (D <= SR_PATHS_MAX_D is checked above)
        }); })));
    const long nfin = (long)a.H * n_u * (1 + n_s) + (a.x0_per_path ? 0 : n_s);
    return sr_launch(sr_paths_rollout_fin_kernel, dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, s, a, nblk);
}
