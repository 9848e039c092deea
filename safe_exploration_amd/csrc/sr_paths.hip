// sr_paths.hip -- posterior FUNCTION samples of an ARD-RBF model by pathwise conditioning (Matheron's rule on a
// random-Fourier-feature prior; the algebra and the C-ABI: include/safereach.h, the launch plan: sr_capi_paths.hip).
//
//   KPF sr_paths_feature_kernel : the feature slab Phi_d of a set of rows (Z, or a chunk of queries) as a k-major operand,
//                                 one fp64 cos per element, padding written as zero                      [cos bound]
//   KPP sr_paths_pack_kernel    : path-major draws -> k-major operand (w), or the residual R = y - P - sqrt(n_d) eps^T
//                                 in place of the prior P (32 x 32 tiles through LDS: both sides coalesced)  [HBM bound]
//   KPS sr_paths_solve_kernel   : C = U^-1 V on srt::mainloop_nt_glds, the loop of the gradient pass' G = U^-1 V   [MFMA bound]
//   KPE sr_paths_eval_kernel    : a 128 x 128 tile of F for output d: ONE accumulator takes the k-range [0, Mp) of
//                                 Phi_d(X)^T w_d and then the k-range [front padding, Np) of K*_d^T c_d; the epilogue writes
//                                 straight into the T x S x n_out layout                                  [MFMA bound]
//   KPT sr_paths_step_kernel    : path s at its own input: one lane per path, c and w read coalesced along s, Z and omega
//                                 rows through LDS (broadcast reads), the N + M terms split over workgroups   [exp / cos bound]
//   KPR sr_paths_step_sum_kernel: the splits in ascending order (no atomics: the same inputs give the same bits), F and the
//                                 closed-loop next inputs
// The Jacobian of the paths (sr_gp_paths_eval_grad / _step_grad) runs through the same kernels: KPF<GRAD> writes the
// derivative of the feature slab in one input dimension, KPD sr_paths_dkstar_kernel that of K* (K* times the explicit
// difference z_ij - x_tj: nothing is expanded around a centre) [HBM bound], KPE contracts them with its output base and
// stride as arguments; KPT<GRAD> / KPR<GRAD> carry D more accumulators per range next to the value's, whose operations
// and order they leave as they are (F of the GRAD forms is F of the plain forms, bit for bit).
// The first product of the draw (V = U^-T R) and the prior at the training rows are plain TN products: sr_launch_gemm_tn.
#include "sr_mfma_tile.h"
#include "sr_kernel_dev.h"

// ------------------------------------------------------------------------------------------------
// KPF: SR_PATHS_FROWS features x 256 columns per workgroup; the lane's row of X (divided by the lengthscales, as the
// formula is written) sits in registers, the omega rows of the strip in LDS.
// ------------------------------------------------------------------------------------------------
// GRAD: d Phi / d x_jg = -amp sin(arg) omega[i][jg] / l_d[jg] in its place.
template <int DT, bool GRAD = false>
__global__ __launch_bounds__(256) void sr_paths_feature_kernel(sr_paths_feat m, const double* __restrict__ X, long ldx, long T,
                                                               long col0, long ncols, double* __restrict__ Phi, int jg) {
    __shared__ double om[SR_PATHS_FROWS * DT];
    __shared__ double ta[SR_PATHS_FROWS];
    const int d = blockIdx.z, i0 = blockIdx.y * SR_PATHS_FROWS;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const long t = c - col0;
    const bool live = c < ncols && t >= 0 && t < T;
    double xs[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) xs[j] = (live && j < m.D) ? X[t * ldx + j] / m.ls[d * m.D + j] : 0.0;
    if (threadIdx.x < SR_PATHS_FROWS) {
        const int i = i0 + threadIdx.x;
#pragma unroll
        for (int j = 0; j < DT; ++j) om[threadIdx.x * DT + j] = (i < m.M && j < m.D) ? m.omega[(long)i * m.D + j] : 0.0;
        ta[threadIdx.x] = i < m.M ? m.tau[i] : 0.0;
    }
    __syncthreads();
    if (c >= ncols) return;
    double amp = sqrt(2.0 * m.sf2[d] / (double)m.M);
    if (GRAD) amp = -amp / m.ls[d * m.D + jg];
    double* out = Phi + ((long)d * m.Mp + i0) * ncols + c;
#pragma unroll 4
    for (int r = 0; r < SR_PATHS_FROWS; ++r) {
        double arg = 0.0;
#pragma unroll
        for (int j = 0; j < DT; ++j) arg = fma(om[r * DT + j], xs[j], arg);
        if (GRAD)
            out[(long)r * ncols] = (live && i0 + r < m.M) ? amp * sin(arg + ta[r]) * m.omega[(long)(i0 + r) * m.D + jg] : 0.0;
        else
            out[(long)r * ncols] = (live && i0 + r < m.M) ? amp * cos(arg + ta[r]) : 0.0;
    }
}

int sr_launch_paths_features(const sr_paths_feat& m, const double* X, long ldx, long T, long col0, long ncols, double* Phi,
                             hipStream_t s, int jg) {
    SR_CHECK(m.Mp % SR_PATHS_FROWS == 0 && m.Mp >= m.M && ncols > 0 && jg < m.D, SR_EINVAL,
             "paths_features: M=%d Mp=%d ncols=%ld jg=%d", m.M, m.Mp, ncols, jg);
    const dim3 grid((unsigned)((ncols + 255) / 256), m.Mp / SR_PATHS_FROWS, m.n_out);
    return sr_pick_le<3, 5, 8>("paths_features", m.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (jg >= 0)
            return sr_launch(sr_paths_feature_kernel<DT, true>, grid, dim3(256), 0, s, m, X, ldx, T, col0, ncols, Phi, jg);
        return sr_launch(sr_paths_feature_kernel<DT, false>, grid, dim3(256), 0, s, m, X, ldx, T, col0, ncols, Phi, 0); });
}

// ------------------------------------------------------------------------------------------------
// KPD: dKs[d][k][c] = Ks[d][k][c] (z_{k - off, jg} - x_{c, jg}) / l_d[jg]^2 for the real rows and the queries c < T, exactly
// zero elsewhere (k < Np, c < Tp): one element per lane, 256 columns x 16 rows per workgroup, the rows' z through LDS.
// ------------------------------------------------------------------------------------------------
#define SR_PATHS_DROWS 16
__global__ __launch_bounds__(256) void sr_paths_dkstar_kernel(const double* __restrict__ Ks, double* __restrict__ dKs,
                                                              const double* __restrict__ Z, const double* __restrict__ X,
                                                              const double* __restrict__ ls, int N, int Np, int D, long T,
                                                              long Tp, int jg) {
    __shared__ double zj[SR_PATHS_DROWS];
    const int d = blockIdx.z, k0 = blockIdx.y * SR_PATHS_DROWS, off = Np - N;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < SR_PATHS_DROWS) {
        const int i = k0 + threadIdx.x - off;
        zj[threadIdx.x] = (i >= 0 && i < N) ? Z[(long)i * D + jg] : 0.0;
    }
    __syncthreads();
    if (c >= Tp) return;
    const bool live = c < T;
    const double l = ls[d * D + jg], il2 = 1.0 / (l * l);
    const double xj = live ? X[c * D + jg] : 0.0;
    const long e = ((long)d * Np + k0) * Tp + c;
#pragma unroll 4
    for (int r = 0; r < SR_PATHS_DROWS; ++r)
        dKs[e + (long)r * Tp] = (live && k0 + r >= off) ? Ks[e + (long)r * Tp] * ((zj[r] - xj) * il2) : 0.0;
}

int sr_launch_paths_dkstar(const double* Ks, double* dKs, const double* Z, const double* X, const double* ls, int N, int Np,
                           int D, int n_out, long T, long Tp, int jg, hipStream_t s) {
    SR_CHECK(Np % SR_PATHS_DROWS == 0 && N >= 1 && N <= Np && T <= Tp && jg >= 0 && jg < D, SR_EINVAL,
             "paths_dkstar: N=%d Np=%d T=%ld Tp=%ld jg=%d", N, Np, T, Tp, jg);
    return sr_launch(sr_paths_dkstar_kernel, dim3((unsigned)((Tp + 255) / 256), Np / SR_PATHS_DROWS, n_out), dim3(256), 0, s, Ks,
                     dKs, Z, X, ls, N, Np, D, T, Tp, jg);
}

// ------------------------------------------------------------------------------------------------
// KPP: dst[d][r][s] from src[d][s][r - off]; a 32 x 32 tile is read along the rows of src and written along the rows of dst.
// ------------------------------------------------------------------------------------------------
template <bool RESID>
__global__ __launch_bounds__(256) void sr_paths_pack_kernel(const double* __restrict__ src, double* dst,
                                                            const double* __restrict__ yT, const double* __restrict__ noise,
                                                            int n, int off, int Rp, int S, int Sp) {
    __shared__ double tile[32][33];
    const int d = blockIdx.z, r0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sq = s0 + ty + 8 * k, i = r0 + tx - off;
        tile[ty + 8 * k][tx] = (sq < S && i >= 0 && i < n) ? src[((long)d * S + sq) * n + i] : 0.0;
    }
    __syncthreads();
    const double sn = RESID ? sqrt(noise[d]) : 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, sq = s0 + tx, i = r - off;
        if (r >= Rp || sq >= Sp) continue;
        const bool live = sq < S && i >= 0 && i < n;
        double* o = dst + ((long)d * Rp + r) * Sp + sq;
        double v = tile[tx][ty + 8 * k];
        if (RESID) v = yT[(long)d * Rp + r] - *o - sn * v;
        *o = live ? v : 0.0;
    }
}

int sr_launch_paths_pack(const double* src, double* dst, const double* yT, const double* noise, int n, int off, int Rp, int S,
                         int Sp, int n_out, hipStream_t s) {
    const dim3 grid((Sp + 31) / 32, (Rp + 31) / 32, n_out);
    return yT ? sr_launch(sr_paths_pack_kernel<true>, grid, dim3(256), 0, s, src, dst, yT, noise, n, off, Rp, S, Sp)
              : sr_launch(sr_paths_pack_kernel<false>, grid, dim3(256), 0, s, src, dst, yT, noise, n, off, Rp, S, Sp);
}

// ------------------------------------------------------------------------------------------------
// KPS: row block kb of C = U^-1 V contracts over k in [kb 128, Np) (U^-1 upper triangular, read along its rows); the
// blocks with the longest range come first in the grid.  Rows of the front padding: exactly zero.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sr_paths_solve_kernel(const double* __restrict__ Wt, const double* __restrict__ V,
                                                                double* __restrict__ C, int N, int Np, int Sp) {
    __shared__ double smem[srt::SMEM_DOUBLES];
    const int d = blockIdx.z, m0 = blockIdx.y * srt::BM, n0 = blockIdx.x * srt::BN;
    const int off = Np - N, k_lo = (off / srt::BK) * srt::BK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    double* Ct = C + ((long)d * Np + m0) * Sp + n0;
    srt::Acc acc;
    acc.zero();
    if (m0 + srt::BM > off)                              // (a block of padding rows only: nothing to contract)
        srt::mainloop_nt_glds(Wt + (long)d * Np * Np + (long)m0 * Np, Np, V + (long)d * Np * Sp + n0, Sp, max(m0, k_lo), Np, smem,
                              acc);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = srt::acc_row(wm, mi, lane, r);
            const bool real = m0 + row >= off;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) Ct[(long)row * Sp + srt::acc_col(wn, ni, lane)] = real ? acc.v[mi][ni][r] : 0.0;
        }
}

int sr_launch_paths_solve(const double* Wt, const double* V, double* C, int N, int Np, int Sp, int n_out, hipStream_t s) {
    SR_CHECK(Np % srt::BM == 0 && Sp % srt::BN == 0 && N >= 1 && N <= Np, SR_EINVAL, "paths_solve: N=%d Np=%d Sp=%d", N, Np, Sp);
    return sr_launch(sr_paths_solve_kernel, dim3(Sp / srt::BN, Np / srt::BM, n_out), dim3(256), 0, s, Wt, V, C, N, Np, Sp);
}

// ------------------------------------------------------------------------------------------------
// KPE: tile (queries t0 .., paths s0 ..) of output d.  Both ranges run through the LDS-DMA TN loop into the same
// accumulator; path tiles are the fast grid index, so that the workgroups resident together share a tile of Phi and K*.
// The stores of a lane are `es` doubles apart (the API's layouts have the path index outside the output's): element (t, s)
// of output d is out[(t S + s) es + d ds] -- es = n_out, ds = 1 for F; out = J + j, es = n_out D, ds = D for column j of J.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sr_paths_eval_kernel(const double* __restrict__ Phi, const double* __restrict__ Wk,
                                                               const double* __restrict__ Ks, const double* __restrict__ C,
                                                               double* __restrict__ F, int Np, int Mp, int k_lo, long T, long Tp,
                                                               int S, int Sp, int es, int ds) {
    __shared__ double smem[srt::SMEM_DOUBLES];
    const int d = blockIdx.z;
    const long t0 = (long)blockIdx.y * srt::BM;
    const int s0 = blockIdx.x * srt::BN;
    srt::Acc acc;
    acc.zero();
    // mainloop_tn_glds for both ranges (the same order of accumulation as the pipelined loop, bit for bit): with the pipelined
    // loop in either place hipcc keeps a second copy of the 128 accumulator registers across the second loop -- 232 bytes of
    // scratch per lane at two workgroups per CU, or 256 AGPRs at one; this form takes 158 VGPRs and no scratch
    srt::mainloop_tn_glds<srt::BK>(Phi + (long)d * Mp * Tp + t0, Tp, Wk + (long)d * Mp * Sp + s0, Sp, 0, Mp, smem, acc);
    srt::mainloop_tn_glds<srt::BK>(Ks + (long)d * Np * Tp + t0, Tp, C + (long)d * Np * Sp + s0, Sp, k_lo, Np, smem, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // element (mi, ni, r) of the lane is (16 mi + 4 r) queries and 16 ni paths further: one address per lane, uniform offsets
    // (per-element addresses, computed ahead of the stores, spilled the accumulators)
    const long tl = t0 + wm * 64 + (lane >> 4);
    const int sl = s0 + wn * 64 + (lane & 15);
    double* f0 = F + (tl * S + sl) * es + d * ds;
    const long st = (long)S * es;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __builtin_amdgcn_sched_barrier(0);
            if (tl + mi * 16 + 4 * r >= T) continue;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                if (sl + ni * 16 < S) f0[(mi * 16 + 4 * r) * st + ni * 16 * es] = acc.v[mi][ni][r];
        }
}

int sr_launch_paths_eval(const double* Phi, const double* Wk, const double* Ks, const double* C, double* F, int N, int Np,
                         int Mp, long T, long Tp, int S, int Sp, int n_out, hipStream_t s, int es, int ds) {
    SR_CHECK(Np % srt::BK == 0 && Mp % srt::BK == 0 && Mp > 0 && Tp % srt::BM == 0 && Sp % srt::BN == 0 && T <= Tp && S <= Sp,
             SR_EINVAL, "paths_eval: Np=%d Mp=%d Tp=%ld Sp=%d", Np, Mp, Tp, Sp);
    SR_CHECK(Tp / srt::BM <= 65535, SR_EINVAL, "paths_eval: %ld queries in one chunk (sr_gp_set_chunk)", T);
    const int k_lo = ((Np - N) / srt::BK) * srt::BK;     // rows k < Np - N are padding: K* and c are zero there
    if (es <= 0) { es = n_out; ds = 1; }
    return sr_launch(sr_paths_eval_kernel, dim3(Sp / srt::BN, (unsigned)(Tp / srt::BM), n_out), dim3(256), 0, s, Phi, Wk, Ks, C, F,
                     Np, Mp, k_lo, T, Tp, S, Sp, es, ds);
}

// ------------------------------------------------------------------------------------------------
// KPT: the N + M terms of f_{d,s}(x_s) as one index range [0, N + M): training rows first, features behind; split
// blockIdx.z takes the terms [sp per, (sp + 1) per).  256 rows of Z (scaled by 1 / l_d, as the K* pass scales them) resp. of
// omega at a time through LDS.
// GRAD: next to each range's sum, D sums of its terms' derivatives in the scaled coordinates the loop holds --
// kappa c_i (z_ij - x_j) / l_j resp. sin(arg) w_i omega_ij -- with the prefactors sf2 / l_j and -sqrt(2 sf2 / M) / l_j at the
// end; a split's partial sums are then 1 + D rows of Sp (the value first).  The plain form keeps its own statements where the
// two differ: written through shared temporaries it compiled to 102 instead of 94 VGPRs at DT = 3 (five waves per SIMD -> four).
// ------------------------------------------------------------------------------------------------
#define SR_PATHS_ZT 256
template <int DT, bool GRAD>
__global__ __launch_bounds__(256) void sr_paths_step_kernel(sr_paths_step_args a) {
    __shared__ double rows[SR_PATHS_ZT * DT];
    __shared__ double ta[SR_PATHS_ZT];
    const int d = blockIdx.y, sp = blockIdx.z;
    const int sq = blockIdx.x * 256 + threadIdx.x;
    const bool live = sq < a.S;
    const int D = a.m.D, off = a.Np - a.N;
    double x[DT], inv_l[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        inv_l[j] = (j < D) ? 1.0 / a.m.ls[d * D + j] : 0.0;
        x[j] = (live && j < D) ? a.Xs[(long)sq * D + j] : 0.0;
    }
    const int total = a.N + a.m.M;
    const int per = (total + a.nsplit - 1) / a.nsplit;
    const int e_beg = sp * per, e_end = min(total, e_beg + per);
    // training rows [e_beg, min(e_end, N)): sum_i exp(-r2 / 2) c_i, times sf2 at the end
    double acck = 0.0;
    double gk[GRAD ? DT : 1], gf[GRAD ? DT : 1];
    if (GRAD) {
#pragma unroll
        for (int j = 0; j < DT; ++j) gk[j] = gf[j] = 0.0;
    }
    {
        double xs[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) xs[j] = x[j] * inv_l[j];
        const int i_end = min(e_end, a.N);
        const double* cc = a.C + ((long)d * a.Np + off) * a.Sp + (live ? sq : 0);
        for (int i0 = e_beg; i0 < i_end; i0 += SR_PATHS_ZT) {
            const int nrow = min(SR_PATHS_ZT, i_end - i0);
            __syncthreads();
            if (threadIdx.x < nrow) {
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
                if (!GRAD) {
                    acck = fma(sr_kappa(0, r2), cc[(long)(i0 + r) * a.Sp], acck);
                } else {
                    const double kap = sr_kappa(0, r2), ci = cc[(long)(i0 + r) * a.Sp];
                    acck = fma(kap, ci, acck);
                    const double kc = kap * ci;
#pragma unroll
                    for (int j = 0; j < DT; ++j) gk[j] = fma(kc, rows[r * DT + j] - xs[j], gk[j]);
                }
            }
        }
    }
    // features [max(e_beg, N) - N, e_end - N): sum_i cos(omega_i . (x / l) + tau_i) w_i, times sqrt(2 sf2 / M) at the end
    double accf = 0.0;
    {
        double xs[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) xs[j] = (j < D) ? x[j] / a.m.ls[d * D + j] : 0.0;
        const int f_beg = max(e_beg, a.N) - a.N, f_end = e_end - a.N;
        const double* ww = a.Wk + (long)d * a.m.Mp * a.Sp + (live ? sq : 0);
        for (int i0 = f_beg; i0 < f_end; i0 += SR_PATHS_ZT) {
            const int nrow = min(SR_PATHS_ZT, f_end - i0);
            __syncthreads();
            if (threadIdx.x < nrow) {
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
                if (!GRAD) {
                    accf = fma(cos(arg + ta[r]), ww[(long)(i0 + r) * a.Sp], accf);
                } else {                                 // (cos stays the value's cos: sin is taken on its own)
                    const double wi = ww[(long)(i0 + r) * a.Sp];
                    accf = fma(cos(arg + ta[r]), wi, accf);
                    const double sw = sin(arg + ta[r]) * wi;
#pragma unroll
                    for (int j = 0; j < DT; ++j) gf[j] = fma(sw, rows[r * DT + j], gf[j]);
                }
            }
        }
    }
    if (!GRAD) {
        if (live)
            a.part[((long)sp * a.m.n_out + d) * a.Sp + sq] =
                fma(a.m.sf2[d], acck, sqrt(2.0 * a.m.sf2[d] / (double)a.m.M) * accf);
    } else if (live) {
        const double sf2 = a.m.sf2[d], amp = sqrt(2.0 * sf2 / (double)a.m.M);
        double* p = a.part + ((long)sp * a.m.n_out + d) * (1 + D) * a.Sp + sq;
        p[0] = fma(sf2, acck, amp * accf);
#pragma unroll
        for (int j = 0; j < DT; ++j)
            if (j < D) p[(long)(1 + j) * a.Sp] = fma(sf2 * inv_l[j], gk[j], -(amp * inv_l[j]) * gf[j]);
    }
}

// KPR: one thread per path: per output the splits in ascending order, then the inputs of the next step as sr_sample_kernel
// forms them.  GRAD: the partial sums in the layout of KPT<GRAD>; blockIdx.y == 0 does the above, blockIdx.y = 1 + d D + j
// one element of J (S x n_out x D) per thread the same way -- the pass is bound by the latency of its nsplit dependent
// additions per sum, so the rows of J go beside the value's instead of behind them
template <bool GRAD>
__global__ __launch_bounds__(256) void sr_paths_step_sum_kernel(sr_paths_step_args a) {
    const int sq = blockIdx.x * 256 + threadIdx.x;
    if (sq >= a.S) return;
    const int n_out = a.m.n_out;
    if (GRAD && blockIdx.y > 0) {
        const int row = blockIdx.y - 1, d = row / a.m.D, j = row % a.m.D;
        const long rows = 1 + a.m.D;
        const double* p = a.part + ((long)d * rows + 1 + j) * a.Sp + sq;
        double g = 0.0;
#pragma unroll 8
        for (int sp = 0; sp < a.nsplit; ++sp) g += p[(long)sp * n_out * rows * a.Sp];
        a.J[((long)sq * n_out + d) * a.m.D + j] = g;
        return;
    }
    double u[SR_PATHS_MAX_D];
    if (a.z_next)
        for (int q = 0; q < a.n_u; ++q) u[q] = a.k_ff[q];
    for (int d = 0; d < n_out; ++d) {
        const long rows = GRAD ? 1 + a.m.D : 1;          // rows of Sp per (split, output)
        const double* p = a.part + (long)d * rows * a.Sp + sq;
        double f = 0.0;
        for (int sp = 0; sp < a.nsplit; ++sp) f += p[(long)sp * n_out * rows * a.Sp];
        a.F[(long)sq * n_out + d] = f;
        if (a.z_next) {
            a.z_next[(long)sq * a.m.D + d] = f;
            for (int q = 0; q < a.n_u; ++q) u[q] = fma(a.k_fb[q * n_out + d], f, u[q]);
        }
    }
    if (a.z_next)
        for (int q = 0; q < a.n_u; ++q) a.z_next[(long)sq * a.m.D + n_out + q] = u[q];
}

int sr_launch_paths_step(const sr_paths_step_args& a, hipStream_t s) {
    SR_CHECK(a.S >= 1 && a.S <= a.Sp && a.nsplit >= 1 && a.n_u >= 0 && a.n_u <= SR_PATHS_MAX_D, SR_EINVAL,
             "paths_step: S=%d Sp=%d nsplit=%d n_u=%d", a.S, a.Sp, a.nsplit, a.n_u);
    const dim3 grid((a.S + 255) / 256, a.m.n_out, a.nsplit);
    SR_TRY((sr_pick_le<3, 5, 8>("paths_step", a.m.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (a.J) return sr_launch(sr_paths_step_kernel<DT, true>, grid, dim3(256), 0, s, a);
        return sr_launch(sr_paths_step_kernel<DT, false>, grid, dim3(256), 0, s, a); })));
    if (a.J)
        return sr_launch(sr_paths_step_sum_kernel<true>, dim3((a.S + 255) / 256, 1 + a.m.n_out * a.m.D), dim3(256), 0, s, a);
    return sr_launch(sr_paths_step_sum_kernel<false>, dim3((a.S + 255) / 256), dim3(256), 0, s, a);
}
