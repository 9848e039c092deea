// sr_kernel_dev.h -- the general kernel family (the reference's mat52 / lin_rbf / lin_mat52,
// ssm_gpy/gp_models_utils_casadi.py:17-157), once, for every kernel that evaluates it:
//   k(x,y) = (c0 + sum_j a_j x_j y_j) * v * kappa(r) + sum_j b_j x_j y_j ,  r^2 = sum_j ((x_j-y_j) s_j)^2
//   kappa = exp(-r^2/2) (RBF, id 0) or (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r) (Matern-5/2, id 1)
// packed per output as SR_KP(D) doubles [kappa id, v, c0, s[D], a[D], b[D]] (sr_common.h).  A further radial function is
// one more branch of sr_radial.  The per-pair sums r^2, la = sum a x y, lb = sum b x y of the query-side kernels stay in
// those kernels: each is fused with its own loads and rounds in its own order.
#pragma once
#include "sr_common.h"

#define SR_SQRT5 2.23606797749978969641

// entry j of the packed s / a / b
__device__ __forceinline__ double sr_kp_s(const double* kp, int j) { return kp[3 + j]; }
__device__ __forceinline__ double sr_kp_a(const double* kp, int D, int j) { return kp[3 + D + j]; }
__device__ __forceinline__ double sr_kp_b(const double* kp, int D, int j) { return kp[3 + 2 * D + j]; }

// packed parameters of one output -> what a DT-wide evaluation uses (s_j^2; zeros beyond D)
template <int DT>
struct sr_kpar {
    int kind; double v, c0, s2[DT], a[DT], b[DT];
    __device__ __forceinline__ void load(const double* kp, int D) {
        kind = (int)kp[0]; v = kp[1]; c0 = kp[2];
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            const double sj = (j < D) ? kp[3 + j] : 0.0;
            s2[j] = sj * sj;
            a[j] = (j < D) ? kp[3 + D + j] : 0.0;
            b[j] = (j < D) ? kp[3 + 2 * D + j] : 0.0;
        }
    }
};

// the same for any D: the packed entries where they lie (sv: a copy of s[D] the caller holds, if any)
struct sr_kview {
    const double *const kp, *const sv, *const av, *const bv;
    __device__ __forceinline__ sr_kview(const double* kp, int D, const double* sv = nullptr)
        : kp(kp), sv(sv ? sv : kp + 3), av(kp + 3 + D), bv(kp + 3 + 2 * D) {}
    __device__ __forceinline__ int kind() const { return (int)kp[0]; }
    __device__ __forceinline__ double v() const { return kp[1]; }
    __device__ __forceinline__ double c0() const { return kp[2]; }
};

// kappa(r) and, from ORDER 1 / 2 on, g = kappa'(r)/r and h = g'(r)/r (RBF: g = -kappa, h = kappa; Matern-5/2:
// g = -5/3 (1 + sqrt5 r) e, h = 25/3 e, e = exp(-sqrt5 r)).  Outputs beyond ORDER are left alone; one nobody reads costs
// nothing.
template <int ORDER>
__device__ __forceinline__ void sr_radial(int kind, double r2, double& kap, double& g, double& h) {
    if (kind == 0) {
        kap = exp(-0.5 * r2);
        if (ORDER >= 1) g = -kap;
        if (ORDER >= 2) h = kap;
    } else {
        const double rr = sqrt(r2);
        const double e = exp(-SR_SQRT5 * rr);
        kap = (1.0 + SR_SQRT5 * rr + (5.0 / 3.0) * r2) * e;
        if (ORDER >= 1) g = -(5.0 / 3.0) * (1.0 + SR_SQRT5 * rr) * e;
        if (ORDER >= 2) h = (25.0 / 3.0) * e;
    }
}
__device__ __forceinline__ double sr_kappa(int kind, double r2) {
    double kap, g, h;
    sr_radial<0>(kind, r2, kap, g, h);
    return kap;
}

// k(x, y) as the Gram matrix holds it: the model update, the row append, max-variance selection and the sparse panel must
// agree to the bit (an appended row equals the refit's, a data row that is an inducing row reproduces K_uu's entry).
// The form with `diag` is for the sites that have a diagonal case (diag: the entry's form there, kappa(0)); the others call
// the four-argument form, whose arithmetic carries no select.
template <bool DIAG>
__device__ __forceinline__ double sr_kpair_(const sr_kview& k, int D, const double* x, const double* y, bool diag) {
    double r2 = 0.0, la = 0.0, lb = 0.0;
    for (int c = 0; c < D; ++c) {
        const double t = (x[c] - y[c]) * k.sv[c];
        r2 = fma(t, t, r2);
        la = fma(k.av[c] * x[c], y[c], la);
        lb = fma(k.bv[c] * x[c], y[c], lb);
    }
    return (k.c0() + la) * k.v() * sr_kappa(k.kind(), (DIAG && diag) ? 0.0 : r2) + lb;
}
__device__ __forceinline__ double sr_kpair(const sr_kview& k, int D, const double* x, const double* y) {
    return sr_kpair_<false>(k, D, x, y, false);
}
__device__ __forceinline__ double sr_kpair(const sr_kview& k, int D, const double* x, const double* y, bool diag) {
    return sr_kpair_<true>(k, D, x, y, diag);
}
// k(x, x) in that form with kappa(0) = 1 written out (the pivot of an appended row)
__device__ __forceinline__ double sr_kdiag(const double* kp, int D, const double* x) {
    double la = 0.0, lb = 0.0;
    for (int c = 0; c < D; ++c) {
        la = fma(sr_kp_a(kp, D, c) * x[c], x[c], la);
        lb = fma(sr_kp_b(kp, D, c) * x[c], x[c], lb);
    }
    return (kp[2] + la) * kp[1] + lb;
}

// prior variance of a query, k(x,x) = c0 v + sum_j (a_j v + b_j) x_j^2: term j added to kxx (the sites start their sum
// from 0 or from c0 v), and d k(x,x)/dx_j
__device__ __forceinline__ double sr_kxx_term(const double* kp, int D, int j, double xj, double kxx) {
    return fma((sr_kp_a(kp, D, j) * kp[1] + sr_kp_b(kp, D, j)) * xj, xj, kxx);
}
__device__ __forceinline__ double sr_dkxx(const double* kp, int D, int j, double xj) {
    return 2.0 * (sr_kp_a(kp, D, j) * kp[1] + sr_kp_b(kp, D, j)) * xj;
}

// Derivatives with respect to x, differentiated by hand (the reference leaves them to CasADi's AD).  With
// u_j = s_j^2 (x_j - z_j), c = c0 + sum a_j x_j z_j and the row's scalars vk = v kappa, vg = v g, pg = c v g, ph = c v h:
//   d k/dx_j       = a_j z_j v kappa + c v g u_j + b_j z_j
//   d2 k/dx_j dx_c = v g (a_j z_j u_c + a_c z_c u_j) + c v (h u_j u_c + g s_j^2 delta_jc)          (j <= c)
// (so d var/dx_j = 2 (a_j v + b_j) x_j - 2 sum_i G_i d k_i/dx_j , G = K_y^-1 k*)
__device__ __forceinline__ double sr_dk(int j, const double* u, const double* z, const double* av, const double* bv,
                                        double vk, double pg) {
    return fma(vk, av[j] * z[j], fma(pg, u[j], bv[j] * z[j]));
}
__device__ __forceinline__ double sr_d2k(int j, int c, const double* u, const double* z, const double* av, const double* s2,
                                         double vg, double pg, double ph) {
    double hv = fma(vg, fma(av[j] * z[j], u[c], av[c] * z[c] * u[j]), ph * u[j] * u[c]);
    if (c == j) hv = fma(pg, s2[j], hv);
    return hv;
}
