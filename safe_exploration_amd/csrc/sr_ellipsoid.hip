// sr_ellipsoid.hip -- per-query Jacobian-linearised ellipsoid propagate / sum.
//
// One thread per query; everything lives in registers (n_s <= 8, n_u <= 4 are template parameters
// so every small-matrix index is a compile-time constant).
//
// replaces the algebra of
//   /root/reference/safe_exploration/gp_reachability.py:65-88   (point branch)
//   /root/reference/safe_exploration/gp_reachability.py:89-156  (ellipsoid branch)
//   /root/reference/safe_exploration/utils.py:108-144           (compute_remainder_overapproximations)
//   /root/reference/safe_exploration/utils_ellipsoid.py:63-94, 197-233
//   /root/reference/safe_exploration/gp_reachability.py:215-250 (lin_ellipsoid_safety_distance)
#include "sr_common.h"
#include "sr_ellipsoid_dev.h"

template <int NS, int NU>
__global__ __launch_bounds__(256) void sr_ellipsoid_kernel(sr_ell_args a) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    sr_ellipsoid_one<NS, NU>(a, t);
}

template <int NS, int NU>
__global__ __launch_bounds__(256) void sr_remainder_kernel(long T, const double* __restrict__ qg,
                                                           const double* __restrict__ kg,
                                                           const double* __restrict__ l_mu,
                                                           const double* __restrict__ l_sigma,
                                                           double* __restrict__ u_mu,
                                                           double* __restrict__ u_sigma) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double q[NS][NS], kfb[NU][NS];
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int j = 0; j < NS; ++j) q[i][j] = qg[(t * NS + i) * NS + j];
#pragma unroll
    for (int k = 0; k < NU; ++k)
#pragma unroll
        for (int j = 0; j < NS; ++j) kfb[k][j] = kg[(t * NU + k) * NS + j];
    const double r2 = sr_lambda_max_qb<NS, NU>(q, kfb);
    const double r1 = sqrt(r2);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        u_mu[t * NS + i] = l_mu[i] * r2;
        u_sigma[t * NS + i] = l_sigma[i] * r1;
    }
}

// d[t][m] = h_m . p + c sqrt(h_m Q h_m^T) - h_vec[m]           (gp_reachability.py:245-248)
__global__ __launch_bounds__(256) void sr_safety_kernel(long T, int n_s, int m,
                                                        const double* __restrict__ p,
                                                        const double* __restrict__ q,
                                                        const double* __restrict__ h_mat,
                                                        const double* __restrict__ h_vec, double c,
                                                        double* __restrict__ d) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const double* pt = p + t * n_s;
    const double* qt = q + t * n_s * n_s;
    for (int r = 0; r < m; ++r) {
        double quad;
        d[t * m + r] = sr_safety_row(h_mat + r * n_s, pt, [&](int i, int j) { return qt[i * n_s + j]; }, n_s, c, h_vec[r], quad);
    }
}

// d[t][k] = (s_k - p_t)^T Q_t^-1 (s_k - p_t): T ellipsoids x K samples (samples shared, or one set per
// ellipsoid when per_t != 0).  Cholesky of Q_t per thread, then a triangular solve: |L^-1 (s-p)|^2.
// replaces utils_ellipsoid.distance_to_center / sample_inside_ellipsoid  utils_ellipsoid.py:16-60
template <int NS>
__global__ __launch_bounds__(256) void sr_distance_kernel(long T, int K, const double* __restrict__ samples,
                                                          int per_t, const double* __restrict__ p,
                                                          const double* __restrict__ q, double* __restrict__ d) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * K) return;
    const long t = idx / K;
    const int k = (int)(idx % K);
    double L[NS][NS], y[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        double sjj = q[(t * NS + j) * NS + j];
#pragma unroll
        for (int c = 0; c < j; ++c) sjj -= L[j][c] * L[j][c];
        const double ljj = sqrt(sjj);
        L[j][j] = ljj;
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i > j) {
                double v = q[(t * NS + i) * NS + j];
#pragma unroll
                for (int c = 0; c < j; ++c) v -= L[i][c] * L[j][c];
                L[i][j] = v / ljj;
            }
    }
    const double* sm = samples + (per_t ? (t * K + k) : (long)k) * NS;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        double v = sm[i] - p[t * NS + i];
#pragma unroll
        for (int c = 0; c < i; ++c) v -= L[i][c] * y[c];
        y[i] = v / L[i][i];
        acc = fma(y[i], y[i], acc);
    }
    d[idx] = acc;
}

int sr_launch_distance(long T, int K, int n_s, const double* samples, int per_t, const double* p,
                       const double* q, double* d, hipStream_t s) {
    if (T <= 0 || K <= 0) return SR_OK;
    dim3 grid((unsigned)((T * K + 255) / 256));
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>("distance: n_s=%d outside 1..8", n_s, [&](auto ns) {
        return sr_launch(sr_distance_kernel<decltype(ns)::value>, grid, dim3(256), 0, s, T, K, samples, per_t, p, q, d); });
}

// ---------------------------------------------------------------------------------------------
// Monte-Carlo propagation step (sampling_models.py:66-80 + ssm_gpy/gaussian_process.py:598-619):
//   S[t][j][:]  = mu[t][:] + sqrt(var[t][:]) * eps[t][j][:]          (marginal posterior samples)
//   z[t][j][:]  = [ S[t][j][:],  k_fb S[t][j][:] + k_ff ]            (next GP inputs, optional)
// One thread per sample; pure streaming (eps in, S/z out).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_sample_kernel(long T, int size, int n_out, int n_u,
                                                        const double* __restrict__ mu,
                                                        const double* __restrict__ var,
                                                        const double* __restrict__ eps,
                                                        double* __restrict__ S,
                                                        const double* __restrict__ k_fb,
                                                        const double* __restrict__ k_ff,
                                                        double* __restrict__ z) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * size) return;
    const long t = idx / size;
    double sv[SR_MAX_NS];
    for (int d = 0; d < n_out; ++d) {
        const double v = mu[t * n_out + d] + sqrt(var[t * n_out + d]) * eps[idx * n_out + d];
        sv[d] = v;
        S[idx * n_out + d] = v;
    }
    if (z) {
        double* zr = z + idx * (n_out + n_u);
        for (int d = 0; d < n_out; ++d) zr[d] = sv[d];
        for (int u = 0; u < n_u; ++u) {
            double a = k_ff[u];
            for (int d = 0; d < n_out; ++d) a = fma(k_fb[u * n_out + d], sv[d], a);
            zr[n_out + u] = a;
        }
    }
}

int sr_launch_sample(long T, int size, int n_out, int n_u, const double* mu, const double* var,
                     const double* eps, double* S, const double* k_fb, const double* k_ff, double* z,
                     hipStream_t s) {
    if (T <= 0 || size <= 0) return SR_OK;
    dim3 grid((unsigned)((T * size + 255) / 256));
    hipLaunchKernelGGL(sr_sample_kernel, grid, dim3(256), 0, s, T, size, n_out, n_u, mu, var, eps, S, k_fb,
                       k_ff, z);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

// ---------------------------------------------------------------------------------------------
// dispatch on (n_s, n_u)
// ---------------------------------------------------------------------------------------------
// f(ns, nu) with the two sizes as integral constants; the refusals are the caller's texts
template <class F>
static int pick_ns_nu(const char* fmt_ns, int n_s, const char* fmt_nu, int n_u, F&& f) {
    static_assert(SR_MAX_NS == 8 && SR_MAX_NU == 4, "the two lists below");
    return sr_pick_eq<1, 2, 3, 4, 5, 6, 7, 8>(fmt_ns, n_s, [&](auto ns) {
        return sr_pick_eq<1, 2, 3, 4>(fmt_nu, n_u, [&](auto nu) { return f(ns, nu); }); });
}

int sr_launch_ellipsoid(const sr_ell_args& a, hipStream_t s) {
    if (a.T <= 0) return SR_OK;
    return pick_ns_nu("ellipsoid: n_s=%d outside 1..8", a.n_s, "ellipsoid: n_u=%d outside 1..4", a.n_u, [&](auto ns, auto nu) {
        return sr_launch(sr_ellipsoid_kernel<decltype(ns)::value, decltype(nu)::value>, dim3((unsigned)((a.T + 255) / 256)), dim3(256), 0,
                         s, a); });
}

int sr_launch_remainder(long T, int n_s, int n_u, const double* q, const double* k_fb,
                        const double* l_mu, const double* l_sigma, double* u_mu, double* u_sigma,
                        hipStream_t s) {
    if (T <= 0) return SR_OK;
    return pick_ns_nu("remainder: n_s=%d outside 1..8", n_s, "remainder: n_u=%d outside 1..4", n_u, [&](auto ns, auto nu) {
        return sr_launch(sr_remainder_kernel<decltype(ns)::value, decltype(nu)::value>, dim3((unsigned)((T + 255) / 256)), dim3(256), 0,
                         s, T, q, k_fb, l_mu, l_sigma, u_mu, u_sigma); });
}

int sr_launch_safety(long T, int n_s, int m, const double* p, const double* q, const double* h_mat,
                     const double* h_vec, double c, double* d, hipStream_t s) {
    if (T <= 0) return SR_OK;
    hipLaunchKernelGGL(sr_safety_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, T, n_s,
                       m, p, q, h_mat, h_vec, c, d);
    SR_HIP(hipGetLastError());
    return SR_OK;
}
