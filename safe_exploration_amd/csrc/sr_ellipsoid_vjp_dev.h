// sr_ellipsoid_vjp_dev.h -- the reverse pass (vector-Jacobian product) of the per-query ellipsoid step of sr_ellipsoid_dev.h
// in mode 0, both branches, as a device function; and the GP link that carries the seeds on (mu, var, jac) back to the GP
// input (sr_reach_vjp.hip launches both in one kernel; sr_moments_vjp.hip launches the same link behind the moment algebra of
// sr_moments_vjp_dev.h), and the workgroup size of both kernels (sr_vjp_threads).
//
// the forward it differentiates replaces the algebra of the reference's
//   safe_exploration/gp_reachability.py:65-88   (point branch)
//   safe_exploration/gp_reachability.py:89-156  (ellipsoid branch)
//   safe_exploration/utils.py:108-144           (compute_remainder_overapproximations)
//   safe_exploration/utils_ellipsoid.py:63-94, 197-233
// (the reference has no reverse pass of its own: its MPC differentiates the CasADi graph of the same lines)
//
// Seeds p1_bar (n_s), G = sym(q1_bar) (only the symmetric part of q1_bar counts; a NULL seed is a zero seed, same bits).
//
//   linear part      p1 = a p + b u + mu                        (gp_reachability.py:82-83 / :115)
//                    mu_bar = p1_bar,  p_bar = a^T p1_bar,  kff_bar = b^T p1_bar
//   point branch     q1 = diag(n_s c^2 var)                     (:78-80)
//                    var_bar_i = n_s c^2 G_ii;  jac_bar (and q_bar, kfb_bar where given) = 0
//   ellipsoid branch q1 = (1 + c2) Q0 + (1 + 1/c2) diag(dL)     (:148, utils_ellipsoid.py:88-92)
//     Q0_bar  = (1 + c2) G,   dL_bar_i = (1 + 1/c2) G_ii,   c2_bar = <G, Q0> - sum_i G_ii dL_i / c2^2
//     c2 = sqrt(tr dL / tr Q0):       dL_bar_i += c2_bar / (2 c2 tr Q0),   Q0_bar_ii -= c2_bar c2 / (2 tr Q0)
//     dL = (1 + 1/c1) dS + (1 + c1) dM  (:143):
//                                     dS_bar = (1 + 1/c1) dL_bar,  dM_bar = (1 + c1) dL_bar,  c1_bar = sum_i dL_bar_i (dM_i - dS_i / c1^2)
//     c1 = sqrt(tr dS / tr dM):       dS_bar_i += c1_bar / (2 c1 tr dM),   dM_bar_i -= c1_bar c1 / (2 tr dM)
//     dS_i = n_s (c (sqrt(var_i) + l_sigma_i r))^2  (:127, utils_ellipsoid.py:197-233), ub_i = c (sqrt(var_i) + l_sigma_i r):
//                                     ub_bar_i = 2 n_s ub_i dS_bar_i,  var_bar_i = c ub_bar_i / (2 sqrt(var_i)),  r_bar = sum_i c l_sigma_i ub_bar_i
//     dM_i = n_s (l_mu_i r^2)^2  (utils.py:129-142):   r2_bar = sum_i 2 n_s l_mu_i^2 r^2 dM_bar_i + r_bar / (2 r)
//     Q0 = H q H^T  (:117):           q_bar = H^T Q0_bar H,   H_bar = 2 Q0_bar H q      (q symmetric, see below)
//     H = a + J_x + (J_u + b) K  (:110-114):   jac_bar = [H_bar, H_bar K^T],   kfb_bar = (J_u + b)^T H_bar
//     r^2 = lambda_max(Q (I + K^T K))  (utils.py:133-134).  In the forward's own symmetric form M = L^T Q L, B = I + K^T K = L L^T:
//       with y the unit top eigenvector of M,  w = L y (left eigenvector of Q B),  v = L^-T y (right eigenvector, w . v = 1):
//                                     q_bar += r2_bar w w^T,   kfb_bar += r2_bar 2 r^2 (K v) v^T
//
// THE EIGENVECTOR.  sr_lambda_max_qb iterates eigenvalues only.  Here the same cyclic Jacobi iteration also accumulates its
// rotations (V <- V J, n_s^2 more values) and y is the column of V under the largest diagonal entry.  The other candidate,
// inverse iteration at the computed lambda, solves with the nearly singular M - lambda I: that needs pivoting, a row choice at
// run time indexes the thread's register arrays dynamically and puts them in scratch memory, and it holds n_s^2 values of its
// own anyway.  The iteration runs further than the forward's (squared off-diagonal norm below 1e-34 of the diagonal's instead
// of 1e-26): an eigenVALUE is accurate to the square of what is left off the diagonal, an eigenVECTOR only to its first power
// over the gap.
// TIES.  Where the top eigenvalue is repeated r^2 is not differentiable.  The kernel returns the formulas at the column of V
// it found, a unit vector of the top eigenspace: an element of the generalised gradient, finite.  Near a tie (relative gap
// g = (lambda_1 - lambda_2) / lambda_1) the rounding error of y, and with it that of the outputs that pass through r^2,
// grows as 1 / g.
//
// CONVENTIONS.  q is read as (q + q^T) / 2 and q_bar is exactly symmetric (both halves are written from one value): the
// gradient of the function extended to unsymmetric arguments by q -> (q + q^T) / 2.  A query whose box half-widths are not all
// > 0 (the queries the forward counts in n_bad) gets NaN in every output of that query; no other query is affected.
// A query with var_i = 0 in the ELLIPSOID branch is no violation (c l_sigma_i r > 0), but d sqrt(var) / d var is infinite there:
// var_bar_i is +-inf (NaN under a zero seed), every other output of the query is finite.
// a, b, l_mu, l_sigma, c_safety get no gradient.  Nothing is saved by the forward: H, tr Q0, r^2, c1, c2, dL are recomputed.
//
// LAYOUT.  One thread per query; every matrix index is a compile-time constant or addresses LDS.  Q0, H q and Q0_bar H exist one
// row at a time (tr Q0 and <G, Q0> are sums over those rows, and the rows of G H are formed twice rather than kept); L is factored
// a second time behind the eigenvalue iteration and K and q are read a second time rather than held across it.
//   n_s <= 4: everything in registers, 256 threads per workgroup.
//   n_s >= 5: the thread's one n_s x n_s block -- V during the iteration, then H during the reverse -- lives in LDS, element-major
//             with the thread innermost (sr_tmat), 64 threads per workgroup (12.5 .. 32 KB); the loops over the rows of H stay
//             loops there (a run-time row index is an LDS address, and eight unrolled rows' loads in flight filled the registers),
//             and K is read a third time inside the reverse loop.
// No instance uses scratch memory (everything in registers spills 12 .. 2924 bytes per lane from n_s = 5 on).  The compiler's figures for all 32 instances: profiles/r15_reach_vjp_resources.txt.
#pragma once
#include "sr_common.h"

// (sr_ellvjp_args: sr_common.h)

// an n_s x n_s matrix of one thread: in registers, or in LDS element-major with the thread innermost (entry (i, j) of thread x
// at base[(i n_s + j) stride + x]: a wavefront's 64 lanes read 64 consecutive doubles, no bank conflicts, every index still a
// compile-time constant).  The LDS form needs no barrier: a thread only ever touches its own column.
template <int NS, bool IN_LDS>
struct sr_tmat;
template <int NS>
struct sr_tmat<NS, false> {
    double m[NS][NS];
    __device__ __forceinline__ sr_tmat(double*, int) {}
    __device__ __forceinline__ double get(int i, int j) const { return m[i][j]; }
    __device__ __forceinline__ void set(int i, int j, double x) { m[i][j] = x; }
};
template <int NS>
struct sr_tmat<NS, true> {
    double* base; int stride;
    __device__ __forceinline__ sr_tmat(double* b, int s) : base(b), stride(s) {}
    __device__ __forceinline__ double get(int i, int j) const { return base[(i * NS + j) * stride]; }
    __device__ __forceinline__ void set(int i, int j, double x) { base[(i * NS + j) * stride] = x; }
};
// from n_s = 5 on V (during the eigenvalue iteration) and then H (during the reverse) live in LDS
template <int NS>
constexpr bool sr_vjp_in_lds() { return NS >= 5; }
// threads per workgroup of both reverse kernels (sr_reach_vjp.hip, sr_moments_vjp.hip): 256, or one wavefront where the thread's
// n_s x n_s block lives in LDS (n_s >= 5: 12.5 .. 32 KB per workgroup; the kernels run at one wavefront per SIMD either way, so
// the smaller workgroup costs no occupancy)
template <int NS>
constexpr int sr_vjp_threads() { return sr_vjp_in_lds<NS>() ? 64 : 256; }

// a uniform pointer the optimiser cannot see through: what is loaded through it again is loaded, not kept in registers
template <class T>
__device__ __forceinline__ const T* sr_opaque(const T* p) {
    asm volatile("" : "+s"(p));
    return p;
}

// lower Cholesky factor of B = I + K^T K, K read from global memory (n_u x n_s)
template <int NS, int NU>
__device__ __forceinline__ void sr_chol_b(const double* kg, double (&L)[NS][NS]) {
    double kfb[NU][NS];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) kfb[u][j] = kg[u * NS + j];
    auto Bij = [&](int i, int j) {
        double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
        for (int u = 0; u < NU; ++u) s = fma(kfb[u][i], kfb[u][j], s);
        return s;
    };
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double s = Bij(j, j);
#pragma unroll
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        const double ljj = sqrt(s);
        L[j][j] = ljj;
        const double inv = 1.0 / ljj;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (i > j) {
                double x = Bij(i, j);
#pragma unroll
                for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
                L[i][j] = x * inv;
            } else if (i < j) {
                L[i][j] = 0.0;
            }
        }
    }
}

// r^2 = lambda_max(Q (I + K^T K)) with its eigenvectors: w = L y, v = L^-T y, kv = K v (see the header comment).
// Q is read as (q + q^T) / 2.  Only M and V live through the iteration: L is factored again behind it and K and q are read again
// by the caller (through sr_opaque pointers, or the compiler keeps all of them in registers across the sweeps).
template <int NS, int NU>
__device__ __forceinline__ void sr_top_eigenpair_qb(const double* q_base, const double* k_base, long t, double& lam,
                                                    double (&w)[NS], double (&v)[NS], double (&kv)[NU],
                                                    sr_tmat<NS, sr_vjp_in_lds<NS>()>& V) {
    double y[NS];
    if (NS == 1) {
        double L[NS][NS];
        sr_chol_b<NS, NU>(k_base + t * NU * NS, L);
        lam = q_base[t] * L[0][0] * L[0][0];
        y[0] = 1.0;
    } else {
        // M = L^T Q L, upper triangle; V = I
        double M[NS][NS];
        {
            double L[NS][NS], qs[NS][NS], QL[NS][NS];
            sr_chol_b<NS, NU>(k_base + t * NU * NS, L);
            const double* qg = q_base + t * NS * NS;
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j >= i) qs[i][j] = 0.5 * (qg[i * NS + j] + qg[j * NS + i]);
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < NS; ++k)
                        if (k >= j) s = fma(qs[i < k ? i : k][i < k ? k : i], L[k][j], s);
                    QL[i][j] = s;
                }
#pragma unroll
            for (int i = 0; i < NS; ++i)
#pragma unroll
                for (int j = 0; j < NS; ++j) {
                    V.set(i, j, (i == j) ? 1.0 : 0.0);
                    if (j >= i) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < NS; ++k)
                            if (k >= i) s = fma(L[k][i], QL[k][j], s);
                        M[i][j] = s;
                    }
                }
        }
#define SR_SYM(i, j) M[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]
        // the rotations of sr_lambda_max_qb, applied to the columns of V as well
        for (int sweep = 0; sweep < 30; ++sweep) {
            double off = 0.0, dia = 0.0;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                dia = fma(M[i][i], M[i][i], dia);
#pragma unroll
                for (int j = 0; j < NS; ++j)
                    if (j > i) off = fma(M[i][j], M[i][j], off);
            }
            if (off <= 1e-34 * dia || off == 0.0) break;
#pragma unroll
            for (int p = 0; p < NS; ++p)
#pragma unroll
                for (int r = 0; r < NS; ++r) {
                    if (r > p) {
                        const double apr = M[p][r];
                        if (apr != 0.0) {
                            const double dd = M[r][r] - M[p][p];
                            const double two_a = 2.0 * apr;
                            const double den = fabs(dd) + sqrt(fma(dd, dd, two_a * two_a));
                            const double tt = ((dd >= 0.0) ? two_a : -two_a) / den;
                            const double c = rsqrt(fma(tt, tt, 1.0));
                            const double s = tt * c;
                            M[p][p] = fma(-tt, apr, M[p][p]);
                            M[r][r] = fma(tt, apr, M[r][r]);
                            M[p][r] = 0.0;
#pragma unroll
                            for (int k = 0; k < NS; ++k) {
                                if (k != p && k != r) {
                                    const double mkp = SR_SYM(k, p), mkr = SR_SYM(k, r);
                                    SR_SYM(k, p) = c * mkp - s * mkr;
                                    SR_SYM(k, r) = s * mkp + c * mkr;
                                }
                                const double vkp = V.get(k, p), vkr = V.get(k, r);
                                V.set(k, p, c * vkp - s * vkr);
                                V.set(k, r, s * vkp + c * vkr);
                            }
                        }
                    }
                }
        }
#undef SR_SYM
        // the column under the largest diagonal entry (the first one of equals), picked by selects: no run-time index
        lam = M[0][0];
#pragma unroll
        for (int k = 0; k < NS; ++k) y[k] = V.get(k, 0);
#pragma unroll
        for (int i = 1; i < NS; ++i) {
            const bool up = M[i][i] > lam;
            lam = up ? M[i][i] : lam;
#pragma unroll
            for (int k = 0; k < NS; ++k) y[k] = up ? V.get(k, i) : y[k];
        }
    }
    // w = L y;  L^T v = y from the last row up
    const double* kg = sr_opaque(k_base) + t * NU * NS;
    double L[NS][NS];
    sr_chol_b<NS, NU>(kg, L);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NS; ++k)
            if (k <= i) s = fma(L[i][k], y[k], s);
        w[i] = s;
    }
#pragma unroll
    for (int ii = 0; ii < NS; ++ii) {
        const int i = NS - 1 - ii;
        double s = y[i];
#pragma unroll
        for (int k = 0; k < NS; ++k)
            if (k > i) s -= L[k][i] * v[k];
        v[i] = s / L[i][i];
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) s = fma(kg[u * NS + j], v[j], s);
        kv[u] = s;
    }
}

// doubles per query of a stored eigenpair (sr_reach_rollout_vjp.hip): r^2 | w | v | K v
constexpr int sr_vjp_eig_doubles(int ns, int nu) { return 1 + 2 * ns + nu; }

// the reverse of sr_ellipsoid_one (mode 0) for query t; writes every output of the query that is not NULL.
// PRE_EIG: r^2 and its eigenvectors are not found here but read from eig[t] (sr_vjp_eig_doubles per query), where
// sr_top_eigenpair_qb of the same (q, k_fb) was stored: the part of the step that depends on no seed and stands apart.
// ts (default: t) is the index of the query in the arrays the stages hand to each other and to the next step -- p1_bar, q1_bar,
// p_bar, q_bar, kff_bar, kfb_bar, mu_bar, var_bar, jac_bar, jac_s, jz --, which a kernel with one thread per trajectory keeps in LDS, one slot
// per thread; t indexes the query's inputs (q, k_fb, var, jac where it is not jac_s, the GP derivatives, eig).
template <int NS, int NU, bool PRE_EIG = false>
__device__ __forceinline__ void sr_ellipsoid_vjp_one(const sr_ellvjp_args& a, long t, double* lds, int lds_stride,
                                                     const double* eig = nullptr, long ts_ = -1) {
    const long ts = ts_ < 0 ? t : ts_;
    constexpr int D = NS + NU;
    const double c = a.c_safety;
    const double* G = a.q1_bar ? a.q1_bar + ts * NS * NS : nullptr;
    auto g = [&](int i, int j) { return G ? 0.5 * (G[i * NS + j] + G[j * NS + i]) : 0.0; };
    double pb[NS], vb[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) pb[i] = a.p1_bar ? a.p1_bar[ts * NS + i] : 0.0;
    bool bad = false;
    const double qnan = __builtin_nan("");
    // linear part and var_bar, once `bad` is known
    auto store_linear = [&]() {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            a.mu_bar[ts * NS + i] = bad ? qnan : pb[i];
            a.var_bar[ts * NS + i] = bad ? qnan : vb[i];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(a.a[k * NS + i], pb[k], s);
            a.p_bar[ts * NS + i] = bad ? qnan : s;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(a.b[k * NU + u], pb[k], s);
            a.kff_bar[ts * NU + u] = bad ? qnan : s;
        }
    };

    if (a.q == nullptr) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const double ub = c * sqrt(a.var[t * NS + i]);
            bad |= !(ub > 0.0);
            vb[i] = (NS * c * c) * g(i, i);
        }
        store_linear();
        const double z = bad ? qnan : 0.0;
        if (a.jac_bar)
#pragma unroll
            for (int e = 0; e < NS * D; ++e) a.jac_bar[ts * NS * D + e] = z;
        if (a.q_bar)
#pragma unroll
            for (int e = 0; e < NS * NS; ++e) a.q_bar[ts * NS * NS + e] = z;
        if (a.kfb_bar)
#pragma unroll
            for (int e = 0; e < NU * NS; ++e) a.kfb_bar[ts * NU * NS + e] = z;
        return;
    }

    // ---- forward quantities -------------------------------------------------------------------------------------------
    double r2, w[NS], v[NS], kv[NU];
    sr_tmat<NS, sr_vjp_in_lds<NS>()> H(lds, lds_stride);        // V first, then H: the one n_s x n_s block of this thread
    if constexpr (PRE_EIG) {
        const double* e = eig + t * sr_vjp_eig_doubles(NS, NU);
        r2 = e[0];
#pragma unroll
        for (int i = 0; i < NS; ++i) { w[i] = e[1 + i]; v[i] = e[1 + NS + i]; }
#pragma unroll
        for (int u = 0; u < NU; ++u) kv[u] = e[1 + 2 * NS + u];
    } else {
        sr_top_eigenpair_qb<NS, NU>(a.q, a.k_fb, t, r2, w, v, kv, H);
    }
    double K[NU][NS];
    const double* kg = sr_opaque(a.k_fb) + t * NU * NS;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) K[u][j] = kg[u * NS + j];
    // (q + q^T) / 2, upper triangle (the lower entries of qs are never read)
    double qs[NS][NS];
    const double* qg = sr_opaque(a.q) + t * NS * NS;
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j >= i) qs[i][j] = 0.5 * (qg[i * NS + j] + qg[j * NS + i]);
#define SR_QS(i, j) qs[(i) < (j) ? (i) : (j)][(i) < (j) ? (j) : (i)]
    const double r1 = sqrt(r2);

    const double* jac = a.jac + (a.jac == a.jac_s ? ts : t) * NS * D;
    constexpr int ROW_UNROLL = sr_vjp_in_lds<NS>() ? 1 : NS;
#pragma unroll ROW_UNROLL
    for (int i = 0; i < NS; ++i) {
        double bm[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) bm[u] = jac[i * D + NS + u] + a.b[i * NU + u];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double s = a.a[i * NS + j] + jac[i * D + j];
#pragma unroll
            for (int u = 0; u < NU; ++u) s = fma(bm[u], K[u][j], s);
            H.set(i, j, s);
        }
    }
    // tr Q0 and <G, Q0> = sum_i (G H)_i . (H q)_i, one row of H q and of G H at a time
    // (with H in LDS the loops over its rows stay loops: a row index at run time costs an address there, and eight rows' loads
    //  in flight at once were what filled the registers)
    double trQ0 = 0.0, GQ0 = 0.0;
#pragma unroll ROW_UNROLL
    for (int i = 0; i < NS; ++i) {
        double gr[NS];
#pragma unroll
        for (int l = 0; l < NS; ++l) gr[l] = g(i, l);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            double t1 = 0.0, gh = 0.0;
#pragma unroll
            for (int l = 0; l < NS; ++l) {
                t1 = fma(H.get(i, l), SR_QS(l, k), t1);
                gh = fma(gr[l], H.get(l, k), gh);
            }
            trQ0 = fma(t1, H.get(i, k), trQ0);
            GQ0 = fma(gh, t1, GQ0);
        }
    }
    double dS[NS], dM[NS], ubs[NS], sv[NS];
    double trS = 0.0, trM = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        sv[i] = sqrt(a.var[t * NS + i]);
        const double ub_mu = a.l_mu[i] * r2;
        ubs[i] = c * (sv[i] + a.l_sigma[i] * r1);
        bad |= !(ub_mu > 0.0) || !(ubs[i] > 0.0);
        dS[i] = NS * ubs[i] * ubs[i];
        dM[i] = NS * ub_mu * ub_mu;
        trS += dS[i];
        trM += dM[i];
    }
    const double c1 = sqrt(trS / trM);
    double trL = 0.0, gdl = 0.0;
    double dLb[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double dl = (1.0 + 1.0 / c1) * dS[i] + (1.0 + c1) * dM[i];
        trL += dl;
        gdl = fma(g(i, i), dl, gdl);
    }
    const double c2 = sqrt(trL / trQ0);
    // ---- reverse -------------------------------------------------------------------------------------------------------
    const double c2b = GQ0 - gdl / (c2 * c2);
    const double trLb = c2b / (2.0 * c2 * trQ0);
    const double trQ0b = -c2b * c2 / (2.0 * trQ0);
    double c1b = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        dLb[i] = (1.0 + 1.0 / c2) * g(i, i) + trLb;
        c1b = fma(dLb[i], dM[i] - dS[i] / (c1 * c1), c1b);
    }
    const double trSb = c1b / (2.0 * c1 * trM);
    const double trMb = -c1b * c1 / (2.0 * trM);
    double r1b = 0.0, r2b = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const double dSb = (1.0 + 1.0 / c1) * dLb[i] + trSb;
        const double dMb = (1.0 + c1) * dLb[i] + trMb;
        const double ubb = 2.0 * NS * ubs[i] * dSb;
        vb[i] = c * ubb / (2.0 * sv[i]);
        r1b = fma(c * a.l_sigma[i], ubb, r1b);
        r2b = fma(2.0 * NS * a.l_mu[i] * a.l_mu[i] * r2, dMb, r2b);
    }
    r2b += r1b / (2.0 * r1);
    store_linear();

    // rows of T2 = Q0_bar H = (1 + c2) G H + trQ0_bar H;  H_bar = 2 T2 q;  q_bar = H^T T2 (upper triangle accumulated)
    double qacc[NS][NS], kacc[NU][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (j >= i) qacc[i][j] = r2b * w[i] * w[j];
    const double kscale = 2.0 * r2b * r2;
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) kacc[u][j] = kscale * kv[u] * v[j];
    // (the LDS instances read K a third time here rather than hold it through the loop: n_s = 8, n_u = 4 spilled 12 bytes)
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
            t2[k] = fma(1.0 + c2, gh, trQ0b * H.get(i, k));
        }
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) s = fma(t2[k], SR_QS(k, j), s);
            hb[j] = 2.0 * s;
            a.jac_bar[(ts * NS + i) * D + j] = bad ? qnan : hb[j];
#pragma unroll
            for (int l = 0; l < NS; ++l)
                if (l >= j) qacc[j][l] = fma(H.get(i, j), t2[l], qacc[j][l]);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NS; ++j) s = fma(hb[j], sr_vjp_in_lds<NS>() ? kq[u * NS + j] : K[u][j], s);
            a.jac_bar[(ts * NS + i) * D + NS + u] = bad ? qnan : s;
            const double bm = jac[i * D + NS + u] + a.b[i * NU + u];
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
                const double x = bad ? qnan : qacc[i][j];
                a.q_bar[(ts * NS + i) * NS + j] = x;
                a.q_bar[(ts * NS + j) * NS + i] = x;
            }
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int j = 0; j < NS; ++j) a.kfb_bar[(ts * NU + u) * NS + j] = bad ? qnan : kacc[u][j];
}

// The GP link of query t (run-time sizes, no thread-local arrays): the state-space Jacobian the step reads, from the GP's.
//   jac_s[a][:n_s] = jac_mu[a][:n_xin] Tz,   jac_s[a][n_s:] = jac_mu[a][n_xin:]
__device__ __forceinline__ void sr_reach_gp_jac_one(const sr_ellvjp_args& a, long t, int n_s, int n_u, long ts_ = -1) {
    const long ts = ts_ < 0 ? t : ts_;
    const int D = a.D, nx = a.n_xin, Ds = n_s + n_u;
    for (int o = 0; o < n_s; ++o) {
        const double* gm = a.jac_mu + (t * n_s + o) * D;
        double* js = a.jac_s + (ts * n_s + o) * Ds;
        for (int cc = 0; cc < n_s; ++cc) {
            double s = 0.0;
            for (int i = 0; i < nx; ++i) s = fma(gm[i], a.Tz[i * n_s + cc], s);
            js[cc] = s;
        }
        for (int u = 0; u < n_u; ++u) js[n_s + u] = gm[nx + u];
    }
}

// ... and the seeds on (mu, var, jac) carried to z = [Tz p; k_ff], added to p_bar and kff_bar of the same query:
//   z_bar = sum_a jac_mu[a] mu_bar[a] + jac_var[a] var_bar[a] + sum_{a,d} jz[a][d] hess_mu[a][d],
//   jz[a][:n_xin] = jac_bar[a][:n_s] Tz^T,  jz[a][n_xin:] = jac_bar[a][n_s:];   p_bar += Tz^T z_bar[:n_xin],  kff_bar += z_bar[n_xin:]
// The sums run in ascending order of a and d by one thread: deterministic, no atomics.  hess_mu == NULL (the host leaves it so
// where jac_bar is zero: a point start, the mean-equivalent mode): no second-order term, neither jac_bar nor the Hessian is read.
__device__ __forceinline__ void sr_reach_gp_vjp_one(const sr_ellvjp_args& a, long t, int n_s, int n_u, long ts_ = -1) {
    const long ts = ts_ < 0 ? t : ts_;
    const int D = a.D, Ds = n_s + n_u;
    const int nx = a.Tz ? a.n_xin : n_s;
    const double* mb = a.mu_bar + ts * n_s;
    const double* vb = a.var_bar + ts * n_s;
    const double* jb = a.jac_bar + ts * n_s * Ds;
    const bool second = a.hess_mu != nullptr;
    const double* jz = jb;                      // identity transform: the same layout
    if (second && a.Tz) {
        double* w = a.jz + ts * n_s * D;
        for (int o = 0; o < n_s; ++o) {
            for (int d = 0; d < nx; ++d) {
                double s = 0.0;
                for (int j = 0; j < n_s; ++j) s = fma(jb[o * Ds + j], a.Tz[d * n_s + j], s);
                w[o * D + d] = s;
            }
            for (int u = 0; u < n_u; ++u) w[o * D + nx + u] = jb[o * Ds + n_s + u];
        }
        jz = w;
    }
    for (int e = 0; e < D; ++e) {
        double zb = 0.0;
        for (int o = 0; o < n_s; ++o) {
            zb = fma(a.jac_mu[(t * n_s + o) * D + e], mb[o], zb);
            zb = fma(a.jac_var[(t * n_s + o) * D + e], vb[o], zb);
        }
        if (second)
            for (int o = 0; o < n_s; ++o) {
                const double* hm = a.hess_mu + (t * n_s + o) * (long)D * D;
                for (int d = 0; d < D; ++d) zb = fma(jz[o * D + d], hm[d * D + e], zb);
            }
        if (e >= nx) {
            a.kff_bar[ts * n_u + (e - nx)] += zb;
        } else if (a.Tz) {
            for (int j = 0; j < n_s; ++j) a.p_bar[ts * n_s + j] = fma(a.Tz[e * n_s + j], zb, a.p_bar[ts * n_s + j]);
        } else {
            a.p_bar[ts * n_s + e] += zb;
        }
    }
}
