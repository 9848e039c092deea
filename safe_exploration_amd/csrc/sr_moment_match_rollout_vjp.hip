// sr_moment_match_rollout_vjp.hip -- reverse pass of the closed-loop roll-out of exact moment matching
// (sr_gp_moment_match_rollout_vjp): the gradient of
//   L = sum mu_all_bar . mu_all + sum sigma_all_bar . sigma_all + sum cov_all_bar . cov_all        (cov the unclipped closed form)
// in mu0, sigma0, k_ff and k_fb, per trajectory, at the (mu, Sigma) a forward stored.
//
// One step, with G = [tz; K] (D x n_s), A = a + b K, W = V G, Hm = A + W:
//   mu+ = A mu + b k + mu_g,     Sigma+ = Hm Sigma Hm^T + C - W Sigma W^T,     cov = C
// and its reverse, with Ss = sym(Sigma+_bar) and Sigma read as its symmetric part:
//   SEED   mu_g_bar = mu+_bar,  C_bar = Ss + sym(c_bar),  W_bar = 2 Ss A Sigma,  V_bar = W_bar G^T
//          A_bar = 2 Ss Hm Sigma + mu+_bar mu^T,  mu_bar = A^T mu+_bar,  Sigma_bar = Hm^T Ss Hm - W^T Ss W
//          k_bar = b^T mu+_bar,  K_bar = b^T A_bar + (V^T W_bar)[n_x_in:]
//   GP     (m_z_bar, S_z_bar) = the reverse pass of sr_moment_match.hip at the seeds (mu_g_bar, C_bar, V_bar)
//   LINK   mu_bar += G^T m_z_bar,  k_bar += m_z_bar[n_x_in:],  Sigma_bar += G^T S_z_bar G
//          K_bar += (m_z_bar mu^T + 2 S_z_bar G Sigma)[n_x_in:]
// Step 0 has K = 0 and no K_bar; from a point Sigma = 0 there: V_bar = 0 and Sigma_bar is not returned.  The seed of step i is
// the caller's seed at i plus the (mu_bar, Sigma_bar) of step i + 1.
//
// The GP inputs of all H steps are fixed by the stored states, and nothing that is quadratic in N reads the seeds.  So per
// group of Tg trajectories (Q = H Tg queries, step-major: a step's queries are contiguous):
//   KR0 sr_mmrv_inputs_kernel   one thread per (query, element): m_z = G mu + [0; k], S_z = G Sigma G^T (zero at a point start)
//   the one-off pass            KM0, KM1, KG2 of sr_moment_match.hip ONCE over all Q queries: records, mu_g, V and the tiles' sums
//   the sweep, i = H-1 .. 0     KG1, KG3, KG4 on step i's slice of the records, and
//   KR1 sr_mmrv_sweep_kernel    one workgroup of 64 threads per trajectory: the LINK of step i, then the SEED of step i - 1 (the
//                               first launch seeds step H - 1 only, the last links step 0 only): four launches per step
// KR1 keeps its matrices (n_s x n_s, D x n_s, D x D; n_s, D <= 12) in LDS, one thread per element, every sum in index order.
// No atomics, no waiting between workgroups: a trajectory's results do not depend on its group or on the chunk size.
#include "sr_common.h"

#define SR_MMRV_BT 64
#define MX SR_MMRV_MAX_NS
static_assert(SR_MMRV_MAX_NS >= SR_MAX_D, "KR1: one LDS size for the n_s and the D side");

long sr_mmrv_ws_per_traj(int N, int D, int n_s, int H) {
    const long DD = (long)D * D, nn = (long)n_s * n_s;
    return H * (sr_mmg_ws_per_query(N, D, n_s) + D + DD) + (n_s + nn + (long)n_s * D) + (D + DD) + (n_s + nn);
}

// what step i of trajectory tl reads: the state in front of it, its gains
struct mmrv_step {
    const double *mu, *sig, *K, *kff;       // n_s; n_s x n_s | NULL (a point); n_u x n_s | NULL (step 0); n_u
};
__device__ static inline mmrv_step mmrv_step_of(const sr_mmrv_args& r, long tl, int i) {
    const long n = r.n_s, n_u = r.D - r.n_x_in, g = r.gains_per_traj ? tl : 0;
    mmrv_step st;
    st.mu = i == 0 ? r.mu0 + tl * n : r.mu_all + (tl * r.H + i - 1) * n;
    st.sig = i == 0 ? (r.sigma0 ? r.sigma0 + tl * n * n : nullptr) : r.sigma_all + (tl * r.H + i - 1) * n * n;
    st.K = i == 0 ? nullptr : r.k_fb + (g * (r.H - 1) + i - 1) * n_u * n;
    st.kff = r.k_ff + (g * r.H + i) * n_u;
    return st;
}
// G = [tz; K]
__device__ static inline double mmrv_G(const sr_mmrv_args& r, const mmrv_step& st, int row, int j) {
    if (row < r.n_x_in) return r.tz ? r.tz[row * r.n_s + j] : (row == j ? 1.0 : 0.0);
    return st.K ? st.K[(row - r.n_x_in) * r.n_s + j] : 0.0;
}
__device__ static inline double mmrv_sym(const double* S, int n, int j, int k) { return S ? 0.5 * (S[j * n + k] + S[k * n + j]) : 0.0; }

// KR0
__global__ __launch_bounds__(256) void sr_mmrv_inputs_kernel(sr_mmrv_args r) {
    const int D = r.D, n = r.n_s, per = D + D * D;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= r.Tg * r.H * per) return;
    const long q = e / per, tl = q % r.Tg;
    const int k = (int)(e % per), i = (int)(q / r.Tg);
    const mmrv_step st = mmrv_step_of(r, tl, i);
    if (k < D) {
        double s = k >= r.n_x_in ? st.kff[k - r.n_x_in] : 0.0;
        for (int j = 0; j < n; ++j) s = fma(mmrv_G(r, st, k, j), st.mu[j], s);
        r.m_z[q * D + k] = s;
        return;
    }
    int row = (k - D) / D, col = (k - D) % D;
    if (row < col) { const int x = row; row = col; col = x; }          // (both halves from the same sum: exactly symmetric)
    double s = 0.0;
    if (st.sig)
        for (int j = 0; j < n; ++j) {
            double y = 0.0;
            for (int p = 0; p < n; ++p) y = fma(mmrv_sym(st.sig, n, j, p), mmrv_G(r, st, col, p), y);
            s = fma(mmrv_G(r, st, row, j), y, s);
        }
    r.S_z[q * D * D + (k - D)] = s;
}

// C (rows x cols, dense) = scale * A B over `inner`; A(i, p) = A[i * a0 + p * a1], B(p, j) = B[p * b0 + j * b1]
__device__ static inline void mmrv_mul(double* C, int rows, int cols, int inner, const double* A, int a0, int a1, const double* B,
                                       int b0, int b1, double scale) {
    for (int e = threadIdx.x; e < rows * cols; e += SR_MMRV_BT) {
        const int i = e / cols, j = e % cols;
        double s = 0.0;
        for (int p = 0; p < inner; ++p) s = fma(A[i * a0 + p * a1], B[p * b0 + j * b1], s);
        C[e] = scale * s;
    }
}

// KR1
__global__ __launch_bounds__(SR_MMRV_BT) void sr_mmrv_sweep_kernel(sr_mmrv_args r, int link, int seed) {
    __shared__ double mu[MX], mub[MX], mzb[MX], cm[MX];
    __shared__ double Sg[MX * MX], G[MX * MX], cs[MX * MX], X[MX * MX], Y[MX * MX];
    __shared__ double Ss[MX * MX], A[MX * MX], W[MX * MX], Hm[MX * MX], Wb[MX * MX], V[MX * MX];
    const int tid = threadIdx.x, D = r.D, n = r.n_s, nx = r.n_x_in, n_u = D - nx, H = r.H;
    const long tl = blockIdx.x;
    double* kffb = r.kff_bar + tl * H * n_u;
    double* kfbb = r.kfb_bar ? r.kfb_bar + tl * (H - 1) * n_u * n : nullptr;
    if (link < 0) {
        for (int e = tid; e < n * n; e += SR_MMRV_BT) cs[e] = 0.0;
        if (tid < n) cm[tid] = 0.0;
    } else {
        // ---- LINK of step `link`: X = S_z_bar here
        const mmrv_step st = mmrv_step_of(r, tl, link);
        for (int e = tid; e < n * n; e += SR_MMRV_BT) {
            Sg[e] = mmrv_sym(st.sig, n, e / n, e % n);
            cs[e] = r.carry_sig[tl * n * n + e];
        }
        for (int e = tid; e < D * n; e += SR_MMRV_BT) G[e] = mmrv_G(r, st, e / n, e % n);
        for (int e = tid; e < D * D; e += SR_MMRV_BT) X[e] = r.Sz_bar[tl * D * D + e];
        if (tid < n) { mu[tid] = st.mu[tid]; cm[tid] = r.carry_mu[tl * n + tid]; }
        if (tid < D) mzb[tid] = r.mz_bar[tl * D + tid];
        __syncthreads();
        mmrv_mul(Y, D, n, D, X, D, 1, G, n, 1, 1.0);                    // Y = S_z_bar G
        if (tid < n) {
            double s = cm[tid];
            for (int row = 0; row < D; ++row) s = fma(G[row * n + tid], mzb[row], s);
            cm[tid] = s;
        }
        if (tid < n_u) kffb[link * n_u + tid] += mzb[nx + tid];
        __syncthreads();
        if (st.sig) {
            for (int e = tid; e < n * n; e += SR_MMRV_BT) {               // Sigma_bar += G^T Y
                const int j = e / n, k = e % n;
                double s = cs[e];
                for (int row = 0; row < D; ++row) s = fma(G[row * n + j], Y[row * n + k], s);
                cs[e] = s;
            }
        }
        if (link > 0) {
            for (int e = tid; e < n_u * n; e += SR_MMRV_BT) {             // K_bar += (m_z_bar mu^T + 2 Y Sigma)[n_x_in:]
                const int u = e / n, j = e % n;
                double s = 0.0;
                for (int k = 0; k < n; ++k) s = fma(Y[(nx + u) * n + k], Sg[k * n + j], s);
                kfbb[(link - 1) * n_u * n + e] += fma(mzb[nx + u], mu[j], 2.0 * s);
            }
        }
        __syncthreads();
        if (link == 0) {
            if (tid < n) r.mu0_bar[tl * n + tid] = cm[tid];
            if (r.sigma0)
                for (int e = tid; e < n * n; e += SR_MMRV_BT) {
                    const int j = e / n, k = e % n;
                    r.sigma0_bar[tl * n * n + e] = 0.5 * (cs[j * n + k] + cs[k * n + j]);
                }
        }
    }
    if (seed < 0) return;
    __syncthreads();
    // ---- SEED of step `seed`, from the caller's seeds and the carry (cm, cs)
    const mmrv_step st = mmrv_step_of(r, tl, seed);
    const long q = (long)seed * r.Tg + tl, row0 = tl * H + seed;
    for (int e = tid; e < n * n; e += SR_MMRV_BT) {
        const int j = e / n, k = e % n;
        Sg[e] = mmrv_sym(st.sig, n, j, k);
        // (the caller's seed through its symmetric part alone: an unsymmetric seed and its symmetric part give the same bits)
        Ss[e] = mmrv_sym(r.sigma_all_bar ? r.sigma_all_bar + row0 * n * n : nullptr, n, j, k) + mmrv_sym(cs, n, j, k);
        double s = r.a[e];
        if (st.K)
            for (int u = 0; u < n_u; ++u) s = fma(r.b[j * n_u + u], st.K[u * n + k], s);
        A[e] = s;
    }
    for (int e = tid; e < D * n; e += SR_MMRV_BT) {
        G[e] = mmrv_G(r, st, e / n, e % n);
        V[e] = r.V[q * n * D + e];                                        // (n x D)
    }
    if (tid < n) {
        mu[tid] = st.mu[tid];
        mub[tid] = (r.mu_all_bar ? r.mu_all_bar[row0 * n + tid] : 0.0) + cm[tid];
    }
    __syncthreads();
    mmrv_mul(W, n, n, D, V, D, 1, G, n, 1, 1.0);                         // W = V G
    mmrv_mul(X, n, n, n, A, n, 1, Sg, n, 1, 1.0);                        // X = A Sigma
    if (tid < n) r.mu_bar[tl * n + tid] = mub[tid];
    for (int e = tid; e < n * n; e += SR_MMRV_BT)
        r.cov_bar[tl * n * n + e] = Ss[e] + mmrv_sym(r.cov_all_bar ? r.cov_all_bar + row0 * n * n : nullptr, n, e / n, e % n);
    __syncthreads();
    for (int e = tid; e < n * n; e += SR_MMRV_BT) Hm[e] = A[e] + W[e];
    mmrv_mul(Wb, n, n, n, Ss, n, 1, X, n, 1, 2.0);                       // W_bar = 2 Ss A Sigma
    __syncthreads();
    mmrv_mul(Y, n, n, n, Hm, n, 1, Sg, n, 1, 1.0);                       // Y = Hm Sigma
    for (int e = tid; e < n * D; e += SR_MMRV_BT) {                       // V_bar = W_bar G^T
        const int j = e / D, row = e % D;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s = fma(Wb[j * n + k], G[row * n + k], s);
        r.V_bar[tl * n * D + e] = s;
    }
    if (tid < n_u) {                                                      // k_bar = b^T mu+_bar
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = fma(r.b[j * n_u + tid], mub[j], s);
        kffb[seed * n_u + tid] = s;
    }
    if (tid < n) {                                                        // mu_bar = A^T mu+_bar
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = fma(A[j * n + tid], mub[j], s);
        r.carry_mu[tl * n + tid] = s;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += SR_MMRV_BT) {                       // X = A_bar = 2 Ss Y + mu+_bar mu^T
        const int j = e / n, k = e % n;
        double s = 0.0;
        for (int p = 0; p < n; ++p) s = fma(Ss[j * n + p], Y[p * n + k], s);
        X[e] = fma(mub[j], mu[k], 2.0 * s);
    }
    __syncthreads();
    if (seed > 0) {
        for (int e = tid; e < n_u * n; e += SR_MMRV_BT) {                 // K_bar = b^T A_bar + (V^T W_bar)[n_x_in:]
            const int u = e / n, k = e % n;
            double s = 0.0;
            for (int j = 0; j < n; ++j) s = fma(r.b[j * n_u + u], X[j * n + k], s);
            for (int j = 0; j < n; ++j) s = fma(V[j * D + nx + u], Wb[j * n + k], s);
            kfbb[(seed - 1) * n_u * n + e] = s;
        }
    }
    __syncthreads();
    mmrv_mul(X, n, n, n, Ss, n, 1, Hm, n, 1, 1.0);                       // X = Ss Hm, Y = Ss W
    mmrv_mul(Y, n, n, n, Ss, n, 1, W, n, 1, 1.0);
    __syncthreads();
    for (int e = tid; e < n * n; e += SR_MMRV_BT) {                       // Sigma_bar = Hm^T Ss Hm - W^T Ss W
        const int j = e / n, k = e % n;
        double s1 = 0.0, s2 = 0.0;
        for (int p = 0; p < n; ++p) {
            s1 = fma(Hm[p * n + j], X[p * n + k], s1);
            s2 = fma(W[p * n + j], Y[p * n + k], s2);
        }
        r.carry_sig[tl * n * n + e] = s1 - s2;
    }
}
#undef MX

// one group: r holds the group's rows; ws: r.Tg x sr_mmrv_ws_per_traj doubles
int sr_launch_moment_match_rollout_vjp(sr_mmrv_args r, double* ws, hipStream_t s) {
    const long Tg = r.Tg, Q = Tg * r.H, D = r.D, n = r.n_s, DD = D * D, nn = n * n;
    double* gws = ws;                                  // the one-step reverse pass's scratch for Q queries
    double* w = ws + Q * sr_mmg_ws_per_query(r.N, r.D, r.n_s);
    r.m_z = w; w += Q * D;
    r.S_z = w; w += Q * DD;
    r.mu_bar = w; w += Tg * n;
    r.cov_bar = w; w += Tg * nn;
    r.V_bar = w; w += Tg * n * D;
    r.mz_bar = w; w += Tg * D;
    r.Sz_bar = w; w += Tg * DD;
    r.carry_mu = w; w += Tg * n;
    r.carry_sig = w;
    r.V = sr_mmg_ws_v(gws, Q, r.D, r.n_s);
    const long nin = Q * (D + DD);
    hipLaunchKernelGGL(sr_mmrv_inputs_kernel, dim3((unsigned)((nin + 255) / 256)), dim3(256), 0, s, r);
    SR_HIP(hipGetLastError());
    SR_TRY(sr_launch_moment_match_vjp_records(r.Z, r.alpha, r.ls, r.sf2, r.N, r.Np, r.D, r.n_s, r.m_z, r.S_z, Q, r.inv_k, gws, s));
    hipLaunchKernelGGL(sr_mmrv_sweep_kernel, dim3((unsigned)Tg), dim3(SR_MMRV_BT), 0, s, r, -1, r.H - 1);
    for (int i = r.H - 1; i >= 0; --i) {
        SR_TRY(sr_launch_moment_match_vjp_seeded(r.Z, r.alpha, r.ls, r.sf2, r.N, r.Np, r.D, r.n_s, r.m_z, i * Tg, Tg, Q,
                                                 r.mu_bar, r.cov_bar, r.V_bar, r.mz_bar, r.Sz_bar, gws, s));
        hipLaunchKernelGGL(sr_mmrv_sweep_kernel, dim3((unsigned)Tg), dim3(SR_MMRV_BT), 0, s, r, i, i - 1);
    }
    SR_HIP(hipGetLastError());
    return SR_OK;
}
