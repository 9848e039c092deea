// sr_paths_gen.hip -- posterior FUNCTION samples of a general-family model with the RBF radial part (sr_kernel_dev.h:
// k = (c0 + sum_j a_j x_j y_j) v kappa(r) + sum_j b_j x_j y_j), the kernels sr_paths.hip cannot share because they hold the
// ARD-RBF feature map and the ARD-RBF derivative of K*.  The kernel is a sum of products of PSD kernels, so a prior sample is
// a sum over products of their features (the algebra and the C-ABI: include/safereach.h, the launch plan: sr_capi_paths.hip):
//   base_i(x) = sqrt(2 v / M) cos(sum_j omega_ij s_j x_j + tau_i)     i < M
//   A_0(x) = sqrt(c0),  A_l(x) = sqrt(a_l) x_l                          the groups; the G active ones ascending (sr_paths_gen)
//   phi(x)    = [A_g(x) base_i(x) at row g M + i | sqrt(b_j) x_j at row G M + j],  n_w = G M + D weights per path and output
//
//   KGF sr_paths_gen_feature_kernel : the slab of phi (or of its derivative in one input dimension) as a k-major operand of
//                                     n_out x Mp x ncols; ONE cos (GRAD: one sin as well) per (i, column), written into the
//                                     G group rows; the strip behind the last base strip writes the D linear rows and the
//                                     zero padding up to Mp                                             [cos / HBM bound]
//   KGD sr_paths_gen_dkstar_kernel  : d k(x_c, z_k) / d x_jg from Z, X and kp (sr_dk: no longer K* times a factor), the shape
//                                     of sr_paths_dkstar_kernel's output, padding exactly zero                  [exp bound]
//   KGT sr_paths_gen_step_kernel    : path s at its own input: one lane per path, rows of Z and omega through LDS, the N + M
//                                     terms split as sr_paths_step_kernel splits them, ONE cos per (i, path) shared by the G
//                                     group weights, the D linear features in split 0                      [exp / cos bound]
// KGT writes the splits' partial sums in the layout of KPT, and KPR (sr_paths_step_sum_kernel of sr_paths.hip) adds them up
// as it is.  The pack, the solve, the TN products and the two-range tile (KPP, KPS, KPE) take the slab with Mp as their
// feature count.  Only __syncthreads(), no atomics, every sum in a fixed order.
#include "sr_mfma_tile.h"
#include "sr_kernel_dev.h"

// A_grp[g](x) of a lane for g < G, zero behind; GRAD: dA[g] = d A_grp[g] / d x_jg.  Static indices only: x stays in registers.
template <int DT, bool GRAD>
__device__ __forceinline__ void sr_paths_gen_amps(const sr_paths_gen& g, const sr_kpar<DT>& p, const double* x, int jg,
                                                  double* A, double* dA) {
#pragma unroll
    for (int q = 0; q < DT + 1; ++q) {
        const int l = q < g.G ? g.grp[q] : -1;
        A[q] = (l == 0) ? sqrt(p.c0) : 0.0;
        if (GRAD) dA[q] = 0.0;
#pragma unroll
        for (int j = 0; j < DT; ++j)
            if (l == j + 1) {
                const double sa = sqrt(p.a[j]);
                A[q] = sa * x[j];
                if (GRAD && j == jg) dA[q] = sa;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// KGF: strip blockIdx.y < ceil(M / 16) takes SR_PATHS_FROWS base features x 256 columns (the omega rows of the strip in LDS,
// the lane's row of X in registers) and writes each into its G group rows; the strip behind them the linear rows and the
// padding rows [n_w, Mp).  Together they write every element of the slab.
// ------------------------------------------------------------------------------------------------
template <int DT, bool GRAD>
__global__ __launch_bounds__(256) void sr_paths_gen_feature_kernel(sr_paths_feat m, sr_paths_gen g, const double* __restrict__ X,
                                                                   long ldx, long T, long col0, long ncols,
                                                                   double* __restrict__ Phi, int jg) {
    constexpr int GT = DT + 1;
    __shared__ double om[SR_PATHS_FROWS * DT];
    __shared__ double ta[SR_PATHS_FROWS];
    const int d = blockIdx.z, nstrip = (m.M + SR_PATHS_FROWS - 1) / SR_PATHS_FROWS, i0 = blockIdx.y * SR_PATHS_FROWS;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const long t = c - col0;
    const bool live = c < ncols && t >= 0 && t < T;
    const double* kp = g.kp + (long)d * SR_KP(m.D);
    double x[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) x[j] = (live && j < m.D) ? X[t * ldx + j] : 0.0;
    if ((int)blockIdx.y == nstrip) {                     // (the whole workgroup: nobody waits at the barrier below)
        if (c >= ncols) return;
        double* out = Phi + ((long)d * m.Mp + (long)g.G * m.M) * ncols + c;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            if (j >= m.D) continue;
            const double sb = sqrt(sr_kp_b(kp, m.D, j));
            const double val = GRAD ? (j == jg ? sb : 0.0) : sb * x[j];
            out[(long)j * ncols] = live ? val : 0.0;
        }
        for (int r = g.n_w; r < m.Mp; ++r) Phi[((long)d * m.Mp + r) * ncols + c] = 0.0;
        return;
    }
    if (threadIdx.x < SR_PATHS_FROWS) {
        const int i = i0 + threadIdx.x;
#pragma unroll
        for (int j = 0; j < DT; ++j) om[threadIdx.x * DT + j] = (i < m.M && j < m.D) ? m.omega[(long)i * m.D + j] : 0.0;
        ta[threadIdx.x] = i < m.M ? m.tau[i] : 0.0;
    }
    __syncthreads();
    if (c >= ncols) return;
    sr_kpar<DT> p;
    p.load(kp, m.D);
    double xs[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) xs[j] = (j < m.D) ? x[j] * sr_kp_s(kp, j) : 0.0;
    const double amp = sqrt(2.0 * p.v / (double)m.M);
    double A[GT], dA[GRAD ? GT : 1];
    sr_paths_gen_amps<DT, GRAD>(g, p, x, jg, A, dA);
#pragma unroll
    for (int q = 0; q < GT; ++q) {
        A[q] *= amp;
        if (GRAD) dA[q] *= amp;
    }
    const double sjg = GRAD ? sr_kp_s(kp, jg) : 0.0;
    double* out = Phi + (long)d * m.Mp * ncols + c;
#pragma unroll 2
    for (int r = 0; r < SR_PATHS_FROWS; ++r) {
        const int i = i0 + r;
        if (i >= m.M) break;
        double arg = 0.0;
#pragma unroll
        for (int j = 0; j < DT; ++j) arg = fma(om[r * DT + j], xs[j], arg);
        const double cs = cos(arg + ta[r]);
        const double sn = GRAD ? sin(arg + ta[r]) * (om[r * DT + jg] * sjg) : 0.0;
#pragma unroll
        for (int q = 0; q < GT; ++q) {
            if (q >= g.G) continue;
            double val;
            if (GRAD) val = fma(dA[q], cs, -(A[q] * sn));
            else val = A[q] * cs;
            out[((long)q * m.M + i) * ncols] = live ? val : 0.0;
        }
    }
}

int sr_launch_paths_gen_features(const sr_paths_feat& m, const sr_paths_gen& g, const double* X, long ldx, long T, long col0,
                                 long ncols, double* Phi, hipStream_t s, int jg) {
    const int nstrip = (m.M + SR_PATHS_FROWS - 1) / SR_PATHS_FROWS;
    SR_CHECK(m.M >= 1 && g.G >= 0 && g.G <= m.D + 1 && g.n_w == g.G * m.M + m.D && m.Mp % SR_PATHS_FROWS == 0 && m.Mp >= g.n_w &&
                 nstrip < 65535 && ncols > 0 && jg < m.D,
             SR_EINVAL, "paths_gen_features: M=%d G=%d n_w=%d Mp=%d ncols=%ld jg=%d", m.M, g.G, g.n_w, m.Mp, ncols, jg);
    const dim3 grid((unsigned)((ncols + 255) / 256), nstrip + 1, m.n_out);
    return sr_pick_le<3, 5, 8>("paths_gen_features", m.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (jg >= 0)
            return sr_launch(sr_paths_gen_feature_kernel<DT, true>, grid, dim3(256), 0, s, m, g, X, ldx, T, col0, ncols, Phi, jg);
        return sr_launch(sr_paths_gen_feature_kernel<DT, false>, grid, dim3(256), 0, s, m, g, X, ldx, T, col0, ncols, Phi, 0); });
}

// ------------------------------------------------------------------------------------------------
// KGD: one element per lane and row, 256 columns x 16 rows per workgroup, the rows' z through LDS, the column's x in registers.
// ------------------------------------------------------------------------------------------------
#define SR_PATHS_GDROWS 16
template <int DT>
__global__ __launch_bounds__(256) void sr_paths_gen_dkstar_kernel(double* __restrict__ dKs, const double* __restrict__ Z,
                                                                  const double* __restrict__ X, const double* __restrict__ kp_all,
                                                                  int N, int Np, int D, long T, long Tp, int jg) {
    __shared__ double zr[SR_PATHS_GDROWS * DT];
    const int d = blockIdx.z, k0 = blockIdx.y * SR_PATHS_GDROWS, off = Np - N;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (threadIdx.x < SR_PATHS_GDROWS * DT) {
        const int r = threadIdx.x / DT, j = threadIdx.x % DT, i = k0 + r - off;
        zr[threadIdx.x] = (i >= 0 && i < N && j < D) ? Z[(long)i * D + j] : 0.0;
    }
    __syncthreads();
    if (c >= Tp) return;
    const bool live = c < T;
    const double* kp = kp_all + (long)d * SR_KP(D);
    sr_kpar<DT> p;
    p.load(kp, D);
    double x[DT], ax[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        x[j] = (live && j < D) ? X[c * D + j] : 0.0;
        ax[j] = p.a[j] * x[j];
    }
    const double sg = sr_kp_s(kp, jg), s2g = sg * sg, ag = sr_kp_a(kp, D, jg), bg = sr_kp_b(kp, D, jg);
    const double xg = live ? X[c * D + jg] : 0.0;
    const long e = ((long)d * Np + k0) * Tp + c;
#pragma unroll 2
    for (int r = 0; r < SR_PATHS_GDROWS; ++r) {
        double r2 = 0.0, la = 0.0;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            const double z = zr[r * DT + j], df = x[j] - z;
            r2 = fma(p.s2[j] * df, df, r2);
            la = fma(ax[j], z, la);
        }
        double kap, gg, hh;
        sr_radial<1>(p.kind, r2, kap, gg, hh);
        const double zg = zr[r * DT + jg], ug = s2g * (xg - zg);
        const double val = sr_dk(0, &ug, &zg, &ag, &bg, p.v * kap, (p.c0 + la) * (p.v * gg));
        dKs[e + (long)r * Tp] = (live && k0 + r >= off) ? val : 0.0;
    }
}

int sr_launch_paths_gen_dkstar(double* dKs, const double* Z, const double* X, const double* kp, int N, int Np, int D, int n_out,
                               long T, long Tp, int jg, hipStream_t s) {
    SR_CHECK(Np % SR_PATHS_GDROWS == 0 && N >= 1 && N <= Np && T <= Tp && jg >= 0 && jg < D, SR_EINVAL,
             "paths_gen_dkstar: N=%d Np=%d T=%ld Tp=%ld jg=%d", N, Np, T, Tp, jg);
    const dim3 grid((unsigned)((Tp + 255) / 256), Np / SR_PATHS_GDROWS, n_out);
    return sr_pick_le<3, 5, 8>("paths_gen_dkstar", D, [&](auto dt) {
        return sr_launch(sr_paths_gen_dkstar_kernel<decltype(dt)::value>, grid, dim3(256), 0, s, dKs, Z, X, kp, N, Np, D, T, Tp,
                         jg); });
}

// ------------------------------------------------------------------------------------------------
// KGT: the index range [0, N + M) of KPT -- training rows first, base features behind -- split the same way; 256 rows of Z
// resp. of omega at a time through LDS, unscaled (the linear parts read z itself).  The parameters of the output are uniform
// over the workgroup and every vector of the lane is indexed by unrolled loops only: registers, no scratch.
//   training rows: sum_i k(x, z_i) c_i, k as sr_kpair forms it
//   features:      C_g = sum_i cos(arg_i) w[g M + i] per group, then sqrt(2 v / M) sum_g A_g(x) C_g
//   split 0:       + sum_j sqrt(b_j) x_j w[G M + j]
// GRAD: next to them sum_i c_i dk(x, z_i)/dx_j (sr_dk) and sum_i sin(arg_i) omega_ij (sum_g A_g w[g M + i]); the derivative of
// A_g in its own x_l comes from C_g.  The value's statements are the same in both forms.
// ------------------------------------------------------------------------------------------------
#define SR_PATHS_GZT 256
template <int DT, bool GRAD>
__global__ __launch_bounds__(256) void sr_paths_gen_step_kernel(sr_paths_step_args a, sr_paths_gen g) {
    constexpr int GT = DT + 1;
    __shared__ double rows[SR_PATHS_GZT * DT];
    __shared__ double ta[SR_PATHS_GZT];
    const int d = blockIdx.y, sp = blockIdx.z;
    const int sq = blockIdx.x * 256 + threadIdx.x;
    const bool live = sq < a.S;
    const int D = a.m.D, M = a.m.M, off = a.Np - a.N;
    const double* kp = g.kp + (long)d * SR_KP(D);
    sr_kpar<DT> p;
    p.load(kp, D);
    double x[DT], ax[DT], bx[DT], xs[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        x[j] = (live && j < D) ? a.Xs[(long)sq * D + j] : 0.0;
        ax[j] = p.a[j] * x[j];
        bx[j] = p.b[j] * x[j];
        xs[j] = (j < D) ? x[j] * sr_kp_s(kp, j) : 0.0;
    }
    const int total = a.N + M;
    const int per = (total + a.nsplit - 1) / a.nsplit;
    const int e_beg = sp * per, e_end = min(total, e_beg + per);
    double acck = 0.0;
    double gk[GRAD ? DT : 1], gf[GRAD ? DT : 1];
    if (GRAD) {
#pragma unroll
        for (int j = 0; j < DT; ++j) gk[j] = gf[j] = 0.0;
    }
    {
        const int i_end = min(e_end, a.N);
        const double* cc = a.C + ((long)d * a.Np + off) * a.Sp + (live ? sq : 0);
        for (int i0 = e_beg; i0 < i_end; i0 += SR_PATHS_GZT) {
            const int nrow = min(SR_PATHS_GZT, i_end - i0);
            __syncthreads();
            if ((int)threadIdx.x < nrow) {
#pragma unroll
                for (int j = 0; j < DT; ++j) rows[threadIdx.x * DT + j] = (j < D) ? a.Z[(long)(i0 + threadIdx.x) * D + j] : 0.0;
            }
            __syncthreads();
            if (!live) continue;
#pragma unroll 2
            for (int r = 0; r < nrow; ++r) {
                double z[DT], u[DT];
                double r2 = 0.0, la = 0.0, lb = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    z[j] = rows[r * DT + j];
                    const double df = x[j] - z[j];
                    u[j] = p.s2[j] * df;
                    r2 = fma(u[j], df, r2);
                    la = fma(ax[j], z[j], la);
                    lb = fma(bx[j], z[j], lb);
                }
                double kap, gg, hh;
                sr_radial<GRAD ? 1 : 0>(p.kind, r2, kap, gg, hh);
                const double ci = cc[(long)(i0 + r) * a.Sp];
                const double vk = p.v * kap, cl = p.c0 + la;
                acck = fma(fma(cl, vk, lb), ci, acck);
                if (GRAD) {
                    const double pg = cl * (p.v * gg);
#pragma unroll
                    for (int j = 0; j < DT; ++j) gk[j] = fma(ci, sr_dk(j, u, z, p.a, p.b, vk, pg), gk[j]);
                }
            }
        }
    }
    double A[GT], dA[1], Cg[GT];
    sr_paths_gen_amps<DT, false>(g, p, x, 0, A, dA);
#pragma unroll
    for (int q = 0; q < GT; ++q) Cg[q] = 0.0;
    const double* ww = a.Wk + (long)d * a.m.Mp * a.Sp + (live ? sq : 0);
    {
        const int f_beg = max(e_beg, a.N) - a.N, f_end = e_end - a.N;
        for (int i0 = f_beg; i0 < f_end; i0 += SR_PATHS_GZT) {
            const int nrow = min(SR_PATHS_GZT, f_end - i0);
            __syncthreads();
            if ((int)threadIdx.x < nrow) {
#pragma unroll
                for (int j = 0; j < DT; ++j)
                    rows[threadIdx.x * DT + j] = (j < D) ? a.m.omega[(long)(i0 + threadIdx.x) * D + j] : 0.0;
                ta[threadIdx.x] = a.m.tau[i0 + threadIdx.x];
            }
            __syncthreads();
            if (!live) continue;
#pragma unroll 2
            for (int r = 0; r < nrow; ++r) {
                double arg = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) arg = fma(rows[r * DT + j], xs[j], arg);
                const double cs = cos(arg + ta[r]);
                double wsum = 0.0;
#pragma unroll
                for (int q = 0; q < GT; ++q) {
                    if (q >= g.G) continue;
                    const double wv = ww[((long)q * M + i0 + r) * a.Sp];
                    Cg[q] = fma(cs, wv, Cg[q]);
                    if (GRAD) wsum = fma(A[q], wv, wsum);
                }
                if (GRAD) {                              // (cos stays the value's cos: sin is taken on its own)
                    const double sw = sin(arg + ta[r]) * wsum;
#pragma unroll
                    for (int j = 0; j < DT; ++j) gf[j] = fma(sw, rows[r * DT + j], gf[j]);
                }
            }
        }
    }
    if (!live) return;
    const double amp = sqrt(2.0 * p.v / (double)M);
    double featv = 0.0;
#pragma unroll
    for (int q = 0; q < GT; ++q) featv = fma(A[q], Cg[q], featv);          // (A is zero behind the active groups)
    const double* wl = ww + (long)g.G * M * a.Sp;
    double lin = 0.0;
    if (sp == 0) {
#pragma unroll
        for (int j = 0; j < DT; ++j)
            if (j < D) lin = fma(sqrt(p.b[j]) * x[j], wl[(long)j * a.Sp], lin);
    }
    const long prow = GRAD ? 1 + D : 1;
    double* pp = a.part + ((long)sp * a.m.n_out + d) * prow * a.Sp + sq;
    pp[0] = fma(amp, featv, acck) + lin;
    if (GRAD) {
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            if (j >= D) continue;
            double da = 0.0;                             // d A_g / d x_j . C_g of the group l = j + 1, if it is active
#pragma unroll
            for (int q = 0; q < GT; ++q)
                if (q < g.G && g.grp[q] == j + 1) da = sqrt(p.a[j]) * Cg[q];
            double v = fma(amp, fma(-sr_kp_s(kp, j), gf[j], da), gk[j]);
            if (sp == 0) v = fma(sqrt(p.b[j]), wl[(long)j * a.Sp], v);
            pp[(long)(1 + j) * a.Sp] = v;
        }
    }
}

// KPR of sr_paths.hip, which instantiates both forms (sr_launch_paths_step): launched here on the same arguments
template <bool GRAD>
__global__ void sr_paths_step_sum_kernel(sr_paths_step_args a);

int sr_launch_paths_gen_step(const sr_paths_step_args& a, const sr_paths_gen& g, hipStream_t s) {
    SR_CHECK(a.S >= 1 && a.S <= a.Sp && a.nsplit >= 1 && a.n_u >= 0 && a.n_u <= SR_PATHS_MAX_D && g.G >= 0 && g.G <= a.m.D + 1 &&
                 g.n_w == g.G * a.m.M + a.m.D && a.m.Mp >= g.n_w,
             SR_EINVAL, "paths_gen_step: S=%d Sp=%d nsplit=%d n_u=%d G=%d n_w=%d Mp=%d", a.S, a.Sp, a.nsplit, a.n_u, g.G, g.n_w,
             a.m.Mp);
    const dim3 grid((a.S + 255) / 256, a.m.n_out, a.nsplit);
    SR_TRY((sr_pick_le<3, 5, 8>("paths_gen_step", a.m.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if (a.J) return sr_launch(sr_paths_gen_step_kernel<DT, true>, grid, dim3(256), 0, s, a, g);
        return sr_launch(sr_paths_gen_step_kernel<DT, false>, grid, dim3(256), 0, s, a, g); })));
    if (a.J)
        return sr_launch(sr_paths_step_sum_kernel<true>, dim3((a.S + 255) / 256, 1 + a.m.n_out * a.m.D), dim3(256), 0, s, a);
    return sr_launch(sr_paths_step_sum_kernel<false>, dim3((a.S + 255) / 256), dim3(256), 0, s, a);
}
