// sr_moments_vjp_dev.h -- the reverse pass (vector-Jacobian product) of the per-query Gaussian moment step of
// sr_ellipsoid_dev.h (mode 1: first-order Taylor, mode 2: mean-equivalent), both starts, as a device function.  The GP link
// that carries the seeds on (mu_g, var_g, jac_g) back to the GP input is the one of sr_ellipsoid_vjp_dev.h
// (sr_reach_gp_jac_one, sr_reach_gp_vjp_one); sr_moments_vjp.hip launches both in one kernel.
//
// the forward it differentiates replaces the algebra of the reference's
//   safe_exploration/uncertainty_propagation_casadi.py:11-87    (one_step_taylor)
//   safe_exploration/uncertainty_propagation_casadi.py:210-283  (one_step_mean_equivalent)
// (the reference has no reverse pass of its own: its CautiousMPC differentiates the CasADi graph of the same lines)
//
// Seeds mu1_bar (n_s), S = sym(sigma1_bar), gpvar_bar (n_s, on the GP variances the roll-out returns beside its moments); a NULL
// seed is a zero seed, same bits.
//
//   linear part      mu1 = a mu_x + b k_ff + mu_g
//                    mug_bar = mu1_bar,  mux_bar = a^T mu1_bar,  kff_bar = b^T mu1_bar
//   both starts      Sigma1 = ... + diag(var_g):   var_bar_i = S_ii + gpvar_bar_i
//   point start      Sigma1 = diag(var_g):         jac_bar (and sigma_bar, kfb_bar where given) = 0
//   Gaussian start   Sigma1 = H Sigma H^T + diag(var_g):   sigma_bar = H^T S H,   H_bar = 2 S H Sigma     (Sigma symmetric, below)
//     mode 1   H = a + J_x + (J_u + b) K:   jac_bar = [H_bar, H_bar K^T],   kfb_bar = (J_u + b)^T H_bar
//     mode 2   H = a + b K:                 jac_bar = 0,                    kfb_bar = b^T H_bar
//
// CONVENTIONS, those of sr_ellipsoid_vjp_dev.h.  sigma_x is read as (Sigma + Sigma^T) / 2 and sigma_bar is exactly symmetric (both
// halves are written from one value).  a and b get no gradient.  Nothing is saved by the forward: H is recomputed.  There is no
// square root here, so no query is "bad" and nothing is NaN that was not NaN in the inputs.
//
// LAYOUT, that of sr_ellipsoid_vjp_one.  One thread per query; every matrix index is a compile-time constant or addresses LDS.
// S H and H_bar exist one row at a time.  n_s <= 4: everything in registers, 256 threads per workgroup.  n_s >= 5: H lives in LDS
// (sr_tmat, element-major with the thread innermost), 64 threads per workgroup, the loop over its rows stays a loop and K is read
// again inside it.  No instance uses scratch memory: profiles/r16_moments_vjp_resources.txt.
#pragma once
#include "sr_ellipsoid_vjp_dev.h"

// (sr_momvjp_args: sr_common.h)

// the reverse of sr_ellipsoid_one in mode MODE (1 or 2) for query t; writes every output of the query that is not NULL.
// ts (default: t), as in sr_ellipsoid_vjp_one: the index of the query in the arrays the stages hand to each other and to the next
// step -- the two seeds, every output, jac where it is jac_s --, which the roll-out sweep (sr_moments_rollout_vjp.hip) keeps one
// slot per thread; t indexes the query's inputs (q, k_fb, jac where it is not jac_s, gpvar_bar).
template <int NS, int NU, int MODE>
__device__ __forceinline__ void sr_moments_vjp_one(const sr_momvjp_args& m, long t, double* lds, int lds_stride, long ts_ = -1) {
    static_assert(MODE == 1 || MODE == 2, "the moment modes");
    const long ts = ts_ < 0 ? t : ts_;
    const sr_ellvjp_args& a = m.e;
    constexpr int D = NS + NU;
    const double* G = a.q1_bar ? a.q1_bar + ts * NS * NS : nullptr;
    auto g = [&](int i, int j) { return G ? 0.5 * (G[i * NS + j] + G[j * NS + i]) : 0.0; };
    {
        double pb[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) pb[i] = a.p1_bar ? a.p1_bar[ts * NS + i] : 0.0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            a.mu_bar[ts * NS + i] = pb[i];
            a.var_bar[ts * NS + i] = g(i, i) + (m.gpvar_bar ? m.gpvar_bar[t * NS + i] : 0.0);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(a.a[k * NS + i], pb[k], s);
            a.p_bar[ts * NS + i] = s;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(a.b[k * NU + u], pb[k], s);
            a.kff_bar[ts * NU + u] = s;
        }
    }
    if (a.q == nullptr) {
        if (a.jac_bar)
#pragma unroll
            for (int e = 0; e < NS * D; ++e) a.jac_bar[ts * NS * D + e] = 0.0;
        if (a.q_bar)
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) a.q_bar[ts * NS * NS + e] = 0.0;
        if (a.kfb_bar)
#pragma unroll
            for (int e = 0; e < NU * NS; ++e) a.kfb_bar[ts * NU * NS + e] = 0.0;
        return;
    }

    // ---- forward quantities: K, (Sigma + Sigma^T) / 2 (upper triangle; the lower entries of qs are never read), H ----------------
    double K[NU][NS];
    const double* kg = a.k_fb + t * NU * NS;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) K[u][j] = kg[u * NS + j];
    double qs[NS][NS];
    const double* qg = a.q + t * NS * NS;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j >= i) qs[i][j] = 0.5 * (qg[i * NS + j] + qg[j * NS + i]);
#define SR_QS(i, j) qs[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]
    const double* jac = (MODE == 1) ? a.jac + (a.jac == a.jac_s ? ts : t) * NS * D : nullptr;
    sr_tmat<NS, sr_vjp_in_lds<NS>()> H(lds, lds_stride);
    constexpr int ROW_UNROLL = sr_vjp_in_lds<NS>() ? 1 : NS;
#pragma unroll ROW_UNROLL
    for (int i = 0; i < NS; ++i) {
        double bm[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) bm[u] = (MODE == 1 ? jac[i * D + NS + u] : 0.0) + a.b[i * NU + u];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double s = a.a[i * NS + j] + (MODE == 1 ? jac[i * D + j] : 0.0);
#pragma unroll
            for (int u = 0; u < NU; ++u) s = fma(bm[u], K[u][j], s);
            H.set(i, j, s);
        }
    }

    // ---- reverse: rows of T2 = S H;  H_bar = 2 T2 Sigma;  sigma_bar = H^T T2 (upper triangle accumulated) -------------------------
    double qacc[NS][NS], kacc[NU][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j >= i) qacc[i][j] = 0.0;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) kacc[u][j] = 0.0;
    // (the LDS instances read K again here rather than hold it through the loop, as sr_ellipsoid_vjp_one does)
    const double* kq = sr_opaque(a.k_fb) + t * NU * NS;
#pragma unroll ROW_UNROLL
    for (int i = 0; i < NS; ++i) {
        double t2[NS], hb[NS], gr[NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) gr[l] = g(i, l);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double gh = 0.0;
#pragma unroll
            for (int l = 0; l < NS; ++l) gh = fma(gr[l], H.get(l, k), gh);
            t2[k] = gh;
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(t2[k], SR_QS(k, j), s);
            hb[j] = 2.0 * s;
            if (a.jac_bar) a.jac_bar[(ts * NS + i) * D + j] = (MODE == 1) ? hb[j] : 0.0;
#pragma unroll
            for (int l = 0; l < NS; ++l)
                if (l >= j) qacc[j][l] = fma(H.get(i, j), t2[l], qacc[j][l]);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (MODE == 1) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < NS; ++j) s = fma(hb[j], sr_vjp_in_lds<NS>() ? kq[u * NS + j] : K[u][j], s);
                if (a.jac_bar) a.jac_bar[(ts * NS + i) * D + NS + u] = s;
            } else if (a.jac_bar) {
                a.jac_bar[(ts * NS + i) * D + NS + u] = 0.0;
            }
            const double bm = (MODE == 1 ? jac[i * D + NS + u] : 0.0) + a.b[i * NU + u];
#pragma unroll
            for (int j = 0; j < NS; ++j) kacc[u][j] = fma(bm, hb[j], kacc[u][j]);
        }
    }
#undef SR_QS
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j >= i) {
                a.q_bar[(ts * NS + i) * NS + j] = qacc[i][j];
                a.q_bar[(ts * NS + j) * NS + i] = qacc[i][j];
            }
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) a.kfb_bar[(ts * NU + u) * NS + j] = kacc[u][j];
}
