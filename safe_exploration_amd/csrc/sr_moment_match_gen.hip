// sr_moment_match_gen.hip -- exact moment matching for the general kernel family with the RBF radial part (kappa id 0 on every
// output; the reference's lin_rbf, and rbf outputs beside it), z ~ N(m, S):
//   k_a(x, z) = v_a (c0_a + sum_j a_aj x_j z_j) e_a(x, z) + sum_j b_aj x_j z_j ,   e_a = exp(-1/2 sum_j s_aj^2 (x_j - z_j)^2)
// a polynomial of degree <= 1 times a Gaussian plus a bilinear term: its expectations are Gaussian moments of order <= 2.
// With Li_a = diag(s_a^2) (entries may be ZERO: lin_rbf has its RBF on one input dimension), nu_i = z_i - m, az_i = a_a o z_i:
//   single tilt  E[e_ai] = q_ai = |I + S Li_a|^-1/2 exp(-1/2 nu_i^T Ab_a nu_i),  Ab_a = Li_a (I + S Li_a)^-1 = W^T W ;
//                under it x ~ N(mt_ai, St_a),  mt_ai = m + S Ab_a nu_i,  St_a = S - S Ab_a S,  c_ai = c0_a + mt_ai . az_i
//   E[k_ai] = v_a q_ai c_ai + m . (b_a o z_i)
//   V_a = sum_i alpha_ai { v_a q_ai [c_ai Ab_a nu_i + (I - Ab_a S) az_i] + b_a o z_i }                  (cov(x, g_a) = S V_a)
//   double tilt  E[e_ai e_bj] = Q_ij = |I + S Ld|^-1/2 exp(-1/2 nu_i^T Li_a nu_i - 1/2 nu_j^T Li_b nu_j + 1/2 zeta^T M zeta),
//                Ld = Li_a + Li_b,  M = (I + S Ld)^-1 S,  zeta = Li_a nu_i + Li_b nu_j ;  under it x ~ N(m + M zeta, M)
//   E[k_ai k_bj] = (1) v_a v_b Q_ij [(c0_a + mh . az_i)(c0_b + mh . bz_j) + az_i^T M bz_j]     mh = m + M zeta, bz_j = a_b o z_j
//                + (2) f_ai . (b_b o z_j) + (3) f_bj . (b_a o z_i) + (4) (b_a o z_i)^T (S + m m^T) (b_b o z_j)
//                f_ai = v_a q_ai [c_ai mt_ai + St_a az_i]
//   Cov[a, b] = sum_ij (alpha_ai alpha_bj - [a == b] Kinv_a,ij) E[k_ai k_bj] - mu_a mu_b + [a == b] E[k_a(x, x)]
// Only (1) is a double sum.  (2) - (4) separate in (i, j): against alpha_a alpha_b^T they are products of O(N D) sums (every term
// that carries m cancels against - mu_a mu_b and is never formed), against Kinv_a they need Kinv_a Z (N x D) and Z^T Kinv_a Z
// (D x D), which do not depend on the query: once per call and output.
// Nothing inverts S or Li: every D x D factorisation is of C = I + r S r with r = diag(s) or sqrt(Ld), SPD for any PSD S;
// Ab = r C^-1 r, and M comes from Y = C^-1 r S as Y^T r^-1 on the columns with r_j != 0 (no cancellation) and as S - S r Y
// on the others.
//
// Launches, all deterministic (two-stage sums, no floating-point atomics):
//   KX0a sr_mmx_kz_kernel     per call: one thread per (output, row i): (Kinv_a Z)_i, Kinv_a read as [j][i]
//   KX0b sr_mmx_zkz_kernel    per call: one workgroup per (output, d): row d of Z^T Kinv_a Z and (Z^T alpha_a)_d
//   KX0  sr_mmx_prep_kernel   one thread per (query, output | pair): the D x D algebra (in LDS) into the scratch
//   KX1  sr_mmx_mean_kernel   one workgroup per (query, output): mu, V and the O(N D) sums of (2) - (3), O(N D^2)
//   KX2  sr_mmx_pair_kernel   one workgroup per (query, tile of SR_MMX_IT rows i, pair): the double sum of (1) -- a lane keeps
//                             the four D-vectors of ITS row in registers (Li_b M Li_a nu_i for the exponent, Li_b M az_i,
//                             M Li_a nu_i and M az_i for the bracket), the four wavefronts share the j of a staged tile of
//                             SR_MMX_JT rows (nu_j, bz_j and three scalars in LDS, read as broadcasts); 4 D FMAs and one exp per
//                             (i, j); a == b: weight and bracket are symmetric in (i, j), so j tiles before the one that holds
//                             the i tile are skipped and those behind it count twice; Kinv_a is read as [j][i]
//   KX3  sr_mmx_final_kernel  one thread per (query, pair): the i tiles' partial sums in order, the separable terms, clip, mirror
// The reverse pass exists for the ARD-RBF route only (sr_moment_match.hip).
#include "sr_common.h"

#define SR_MMX_IT 64         // rows i per workgroup of KX2 (one per lane)
#define SR_MMX_JT 256        // rows j per staged tile of KX2 (one per thread while staging)
static_assert(SR_MMX_JT % SR_MMX_IT == 0 && SR_MMX_JT == 256, "KX2: j tiles hold whole i tiles, one j per thread");

struct sr_mmx_args {
    const double *Z, *alpha, *kp;            // the model as the handle holds it (alpha n_out x Np, front padding)
    const double *m, *S, *inv_k;             // T x D, T x D x D | NULL, n_out x N x N
    double *mu, *cov, *V;                    // T x n_out, T x n_out x n_out, T x n_out x D | NULL
    double* call;                            // per output [Kinv Z (N x D) | Z^T Kinv Z (D x D) | Z^T alpha (D)]
    double* ws;                              // [mean records | pair records | mean sums | partial sums] of this chunk
    int N, Np, D, n_out, npairs, nit;
    long T;
};

__host__ __device__ static inline long mmx_call_rec(int N, int D) { return (long)N * D + (long)D * D + D; }
__host__ __device__ static inline long mmx_mean_rec(int D) { return 1 + 2 * (long)D * D; }     // [-1/2 log|C|, W, T1 = W S]
__host__ __device__ static inline long mmx_pair_rec(int D) { return 2 + (long)D * D; }         // [-1/2 log|C|, point, M]
__host__ __device__ static inline long mmx_stat_rec(int D) { return 2 + D; }                   // [g0, h2, F' (D)]
static inline int mmx_nit(int N) { return (N + SR_MMX_IT - 1) / SR_MMX_IT; }
__device__ static inline long mmx_off_pair(const sr_mmx_args& a) { return a.T * a.n_out * mmx_mean_rec(a.D); }
__device__ static inline long mmx_off_stat(const sr_mmx_args& a) { return mmx_off_pair(a) + a.T * a.npairs * mmx_pair_rec(a.D); }
__device__ static inline long mmx_off_part(const sr_mmx_args& a) { return mmx_off_stat(a) + a.T * a.n_out * mmx_stat_rec(a.D); }

long sr_mmx_call_ws(int N, int D, int n_out) { return n_out * mmx_call_rec(N, D); }
long sr_mmx_ws_per_query(int N, int D, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2;
    return n_out * (mmx_mean_rec(D) + mmx_stat_rec(D)) + npairs * (mmx_pair_rec(D) + mmx_nit(N));
}
// queries one launch sequence may take: the grid of KX2 stays below 2^23 workgroups
long sr_mmx_max_queries(int N, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2, per = npairs * mmx_nit(N);
    const long q = ((long)1 << 23) / per;
    return q < 1 ? 1 : q;
}

// p-th pair (a <= b) in row-major order of the upper triangle
__device__ static inline void mmx_pair_of(int p, int n, int& a, int& b) {
    a = 0;
    while (p >= n - a) { p -= n - a; ++a; }
    b = a + p;
}

// sum of red[k * 256 + tid] over tid, k < nk, in a fixed tree order; the sums end in red[k * 256]
__device__ static inline void mmx_block_sum(double* red, int nk) {
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s)
            for (int k = 0; k < nk; ++k) red[k * 256 + threadIdx.x] += red[k * 256 + threadIdx.x + s];
    }
    __syncthreads();
}

// KX0a
template <int DT>
__global__ __launch_bounds__(256) void sr_mmx_kz_kernel(sr_mmx_args a) {
    const int D = a.D, N = a.N, o = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double* kinv = a.inv_k + (size_t)o * N * N;
    double acc[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) acc[d] = 0.0;
    for (int j = 0; j < N; ++j) {
        const double kv = kinv[(size_t)j * N + i];
#pragma unroll
        for (int d = 0; d < DT; ++d)
            if (d < D) acc[d] = fma(kv, a.Z[(long)j * D + d], acc[d]);
    }
    double* kz = a.call + o * mmx_call_rec(N, D);
#pragma unroll
    for (int d = 0; d < DT; ++d)
        if (d < D) kz[(long)i * D + d] = acc[d];
}

// KX0b
template <int DT>
__global__ __launch_bounds__(256) void sr_mmx_zkz_kernel(sr_mmx_args a) {
    __shared__ double red[(DT + 1) * 256];
    const int D = a.D, N = a.N, tid = threadIdx.x, d = blockIdx.x, o = blockIdx.y;
    double* rec = a.call + o * mmx_call_rec(N, D);
    const double* kz = rec;
    const double* al = a.alpha + (long)o * a.Np + (a.Np - N);
    double acc[DT + 1];
#pragma unroll
    for (int k = 0; k <= DT; ++k) acc[k] = 0.0;
    for (int i = tid; i < N; i += 256) {
        const double zd = a.Z[(long)i * D + d];
#pragma unroll
        for (int e = 0; e < DT; ++e)
            if (e < D) acc[e] = fma(zd, kz[(long)i * D + e], acc[e]);
        acc[DT] = fma(al[i], zd, acc[DT]);
    }
#pragma unroll
    for (int k = 0; k <= DT; ++k) red[k * 256 + tid] = acc[k];
    mmx_block_sum(red, DT + 1);
    if (tid < D) rec[(long)N * D + d * D + tid] = red[tid * 256];
    if (tid == 0) rec[(long)N * D + D * D + d] = red[DT * 256];
}

// KX0 keeps its D x D matrices in LDS, element-major with the threads of the block innermost (a thread's own column: no
// bank conflicts, and no dynamically indexed private array -- those live in scratch memory)
#define MMX_AT(M, i, j) M[((i) * DT + (j)) * BT + threadIdx.x]
#define MMX_V(v, d) v[(d) * BT + threadIdx.x]
template <int DT> struct mmx_prep_bt { static constexpr int value = DT <= 4 ? 64 : (DT <= 8 ? 32 : 16); };

// lower Cholesky factor in place (lower triangle read and written); returns log det
template <int DT, int BT>
__device__ static inline double mmx_chol(double* C, int D) {
    double logdet = 0.0;
    for (int k = 0; k < D; ++k) {
        double s = MMX_AT(C, k, k);
        for (int p = 0; p < k; ++p) s -= MMX_AT(C, k, p) * MMX_AT(C, k, p);
        logdet += log(s);
        const double l = sqrt(s), inv = 1.0 / l;
        MMX_AT(C, k, k) = l;
        for (int i = k + 1; i < D; ++i) {
            double v = MMX_AT(C, i, k);
            for (int p = 0; p < k; ++p) v -= MMX_AT(C, i, p) * MMX_AT(C, k, p);
            MMX_AT(C, i, k) = v * inv;
        }
    }
    return logdet;
}

template <int DT>
__global__ __launch_bounds__(mmx_prep_bt<DT>::value) void sr_mmx_prep_kernel(sr_mmx_args a) {
    constexpr int BT = mmx_prep_bt<DT>::value;
    __shared__ double C[DT * DT * BT], X[DT * DT * BT], r[DT * BT];
    const int D = a.D, nslot = a.n_out + a.npairs;
    const long e = (long)blockIdx.x * BT + threadIdx.x;
    if (e >= a.T * nslot) return;
    const long t = e / nslot;
    const int slot = (int)(e % nslot);
    const double* S = a.S ? a.S + t * D * D : nullptr;
    if (slot < a.n_out) {
        // mean of output o: C = I + s S s = Lc Lc^T;  Ab = W^T W with W = Lc^-1 s;  |I + S Li| = |C|;  T1 = W S
        const double* kp = a.kp + (long)slot * SR_KP(D);
        for (int d = 0; d < D; ++d) MMX_V(r, d) = fabs(kp[3 + d]);
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j)
                MMX_AT(C, i, j) = (i == j ? 1.0 : 0.0) + (S ? MMX_V(r, i) * MMX_V(r, j) * S[i * D + j] : 0.0);
        const double logdet = mmx_chol<DT, BT>(C, D);
        for (int j = 0; j < D; ++j) {              // X = Lc^-1 (lower), column by column
            MMX_AT(X, j, j) = 1.0 / MMX_AT(C, j, j);
            for (int i = j + 1; i < D; ++i) {
                double v = 0.0;
                for (int p = j; p < i; ++p) v -= MMX_AT(C, i, p) * MMX_AT(X, p, j);
                MMX_AT(X, i, j) = v / MMX_AT(C, i, i);
            }
        }
        double* rec = a.ws + (t * a.n_out + slot) * mmx_mean_rec(D);
        rec[0] = -0.5 * logdet;
        double *W = rec + 1, *T1 = W + D * D;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) {
                W[i * D + j] = j <= i ? MMX_AT(X, i, j) * MMX_V(r, j) : 0.0;
                double v = 0.0;
                if (S)
                    for (int k = 0; k <= i; ++k) v = fma(MMX_AT(X, i, k) * MMX_V(r, k), S[k * D + j], v);
                T1[i * D + j] = v;
            }
        return;
    }
    // pair (oa, ob): r = sqrt(Li_a + Li_b), C = I + r S r = Lc Lc^T, |I + S Ld| = |C|, Y = C^-1 r S, M = (I + S Ld)^-1 S
    int oa, ob;
    mmx_pair_of(slot - a.n_out, a.n_out, oa, ob);
    const double *ka = a.kp + (long)oa * SR_KP(D), *kb = a.kp + (long)ob * SR_KP(D);
    bool point = true;
    for (int d = 0; d < D; ++d) MMX_V(r, d) = sqrt(ka[3 + d] * ka[3 + d] + kb[3 + d] * kb[3 + d]);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            const double sij = S ? S[i * D + j] : 0.0;
            if (sij != 0.0) point = false;
            if (j <= i) MMX_AT(C, i, j) = (i == j ? 1.0 : 0.0) + MMX_V(r, i) * MMX_V(r, j) * sij;
            MMX_AT(X, i, j) = MMX_V(r, i) * sij;
        }
    const double logdet = mmx_chol<DT, BT>(C, D);
    for (int j = 0; j < D; ++j) {              // X[:, j] <- C^-1 X[:, j]
        for (int i = 0; i < D; ++i) {
            double v = MMX_AT(X, i, j);
            for (int p = 0; p < i; ++p) v -= MMX_AT(C, i, p) * MMX_AT(X, p, j);
            MMX_AT(X, i, j) = v / MMX_AT(C, i, i);
        }
        for (int i = D - 1; i >= 0; --i) {
            double v = MMX_AT(X, i, j);
            for (int p = i + 1; p < D; ++p) v -= MMX_AT(C, p, i) * MMX_AT(X, p, j);
            MMX_AT(X, i, j) = v / MMX_AT(C, i, i);
        }
    }
    double* rec = a.ws + mmx_off_pair(a) + (t * a.npairs + (slot - a.n_out)) * mmx_pair_rec(D);
    rec[0] = -0.5 * logdet;
    rec[1] = point ? 1.0 : 0.0;
    double* M = rec + 2;
    // M_ij r_j = Y_ji (no cancellation); a column with r_j = 0 takes the row's form, and S - S r Y where both are zero
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) {
            double mv[2];
            for (int h = 0; h < 2; ++h) {
                const int p = h ? j : i, q = h ? i : j;              // M_pq
                if (MMX_V(r, q) != 0.0) mv[h] = MMX_AT(X, q, p) / MMX_V(r, q);
                else if (MMX_V(r, p) != 0.0) mv[h] = MMX_AT(X, p, q) / MMX_V(r, p);
                else {
                    double v = S ? S[p * D + q] : 0.0;
                    if (S)
                        for (int k = 0; k < D; ++k) v -= S[p * D + k] * MMX_V(r, k) * MMX_AT(X, k, q);
                    mv[h] = v;
                }
            }
            const double mij = 0.5 * (mv[0] + mv[1]);
            M[i * D + j] = mij;
            M[j * D + i] = mij;
        }
}
#undef MMX_AT
#undef MMX_V

// D x D record -> DT x DT in LDS (zero padding; src NULL: zero), all 256 threads
template <int DT>
__device__ static inline void mmx_load_mat(double* dst, const double* src, int D) {
    for (int e = threadIdx.x; e < DT * DT; e += 256) {
        const int i = e / DT, j = e % DT;
        dst[e] = (src && i < D && j < D) ? src[i * D + j] : 0.0;
    }
}

// KX1
template <int DT>
__global__ __launch_bounds__(256) void sr_mmx_mean_kernel(sr_mmx_args a) {
    __shared__ double W[DT * DT], T1[DT * DT], Sm[DT * DT], mq[DT], av[DT], bv[DT], bzal[DT], xs[DT], red[(DT + 1) * 256];
    __shared__ double sA[DT + 1], sB[DT + 1];
    const int D = a.D, N = a.N, tid = threadIdx.x, o = blockIdx.y, off = a.Np - N;
    const long t = blockIdx.x;
    const double* rec = a.ws + (t * a.n_out + o) * mmx_mean_rec(D);
    const double* kp = a.kp + (long)o * SR_KP(D);
    const double* crec = a.call + o * mmx_call_rec(N, D);
    const double clog = rec[0], v = kp[1], c0 = kp[2];
    mmx_load_mat<DT>(W, rec + 1, D);
    mmx_load_mat<DT>(T1, rec + 1 + D * D, D);
    mmx_load_mat<DT>(Sm, a.S ? a.S + t * D * D : nullptr, D);
    if (tid < DT) {
        const bool in = tid < D;
        mq[tid] = in ? a.m[t * D + tid] : 0.0;
        av[tid] = in ? kp[3 + D + tid] : 0.0;
        bv[tid] = in ? kp[3 + 2 * D + tid] : 0.0;
        bzal[tid] = in ? kp[3 + 2 * D + tid] * crec[(long)N * D + D * D + tid] : 0.0;
    }
    __syncthreads();
    double g0 = 0.0, h2 = 0.0, g1[DT], g2[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) { g1[d] = 0.0; g2[d] = 0.0; }
    const double* al = a.alpha + (long)o * a.Np + off;
    for (int i = tid; i < N; i += 256) {
        double nu[DT], az[DT], kap[DT];
        double amq = 0.0, kmq = 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            const double z = d < D ? a.Z[(long)i * D + d] : 0.0;
            nu[d] = d < D ? z - mq[d] : 0.0;
            az[d] = av[d] * z;
            kap[d] = d < D ? bv[d] * crec[(long)i * D + d] : 0.0;
            amq = fma(az[d], mq[d], amq);
            kmq = fma(kap[d], mq[d], kmq);
        }
        double e = 0.0, yt = 0.0, ytk = 0.0, ttk = 0.0, azsk = 0.0;
#pragma unroll 1                                  // (unrolled, the matrices are kept in registers)
        for (int r = 0; r < D; ++r) {
            double y = 0.0, tt = 0.0, tk = 0.0, sk = 0.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) {
                y = fma(W[r * DT + c], nu[c], y);                   // (zero above the diagonal)
                tt = fma(T1[r * DT + c], az[c], tt);
                tk = fma(T1[r * DT + c], kap[c], tk);
                sk = fma(Sm[r * DT + c], kap[c], sk);
            }
            e = fma(y, y, e);
            yt = fma(y, tt, yt);
            ytk = fma(y, tk, ytk);
            ttk = fma(tt, tk, ttk);
            azsk = fma(av[r] * a.Z[(long)i * D + r], sk, azsk);
        }
        const double c = c0 + amq + yt;                            // c_ai
        const double q = v * exp(clog - 0.5 * e);                  // v_a q_ai
        const double fk = c * (kmq + ytk) - ttk + azsk;            // f_ai . (b o (Kinv Z)_i) / (v_a q_ai)
        const double wq = al[i] * q, wqc = wq * c;
        g0 += wqc;
        h2 = fma(q, fk, h2);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            g1[d] = fma(wqc, nu[d], g1[d]);
            g2[d] = fma(wq, az[d], g2[d]);
        }
    }
    red[tid] = g0;
#pragma unroll
    for (int d = 0; d < DT; ++d) red[(1 + d) * 256 + tid] = g1[d];
    mmx_block_sum(red, DT + 1);
    if (tid <= DT) sA[tid] = red[tid * 256];
    __syncthreads();
    red[tid] = h2;
#pragma unroll
    for (int d = 0; d < DT; ++d) red[(1 + d) * 256 + tid] = g2[d];
    mmx_block_sum(red, DT + 1);
    if (tid <= DT) sB[tid] = red[tid * 256];
    __syncthreads();
    // x = W g1 - T1 g2;  V = W^T x + g2 + b o Z^T alpha;  F' = S g2 + T1^T x  (F = F' + m g0: the part that cancels)
    if (tid < DT) {
        double x = 0.0;
        for (int c = 0; c < DT; ++c) x += W[tid * DT + c] * sA[1 + c] - T1[tid * DT + c] * sB[1 + c];
        xs[tid] = x;
    }
    __syncthreads();
    double* st = a.ws + mmx_off_stat(a) + (t * a.n_out + o) * mmx_stat_rec(D);
    if (tid == 0) {
        double lin = 0.0;
        for (int d = 0; d < D; ++d) lin = fma(mq[d], bzal[d], lin);
        a.mu[t * a.n_out + o] = sA[0] + lin;
        st[0] = sA[0];
        st[1] = sB[0];
    }
    if (tid < D) {
        double wx = 0.0, f = 0.0;
        for (int r = 0; r < D; ++r) {
            wx = fma(W[r * DT + tid], xs[r], wx);
            f = fma(T1[r * DT + tid], xs[r], f);
            f = fma(Sm[tid * DT + r], sB[1 + r], f);
        }
        if (a.V) a.V[(t * a.n_out + o) * D + tid] = wx + sB[1 + tid] + bzal[tid];
        st[2 + tid] = f;
    }
}

// KX2
template <int DT>
__global__ __launch_bounds__(256) void sr_mmx_pair_kernel(sr_mmx_args a) {
    __shared__ double M[DT * DT], mq[DT], la[DT], lb[DT], aa[DT], ab[DT];
    __shared__ double nus[SR_MMX_JT * DT], azs[SR_MMX_JT * DT], sjs[SR_MMX_JT], ajs[SR_MMX_JT], pbs[SR_MMX_JT], red[256];
    const int D = a.D, N = a.N, tid = threadIdx.x, it = blockIdx.y, p = blockIdx.z, off = a.Np - N;
    const long t = blockIdx.x;
    int oa, ob;
    mmx_pair_of(p, a.n_out, oa, ob);
    const bool diag = oa == ob;
    const double* rec = a.ws + mmx_off_pair(a) + (t * a.npairs + p) * mmx_pair_rec(D);
    const double clog = rec[0];
    if (!diag && rec[1] != 0.0) return;         // a point input: the outputs are independent, KX3 writes the zero
    const double *ka = a.kp + (long)oa * SR_KP(D), *kb = a.kp + (long)ob * SR_KP(D);
    const double c0a = ka[2], c0b = kb[2];
    mmx_load_mat<DT>(M, rec + 2, D);
    if (tid < DT) {
        const bool in = tid < D;
        mq[tid] = in ? a.m[t * D + tid] : 0.0;
        la[tid] = in ? ka[3 + tid] * ka[3 + tid] : 0.0;
        lb[tid] = in ? kb[3 + tid] * kb[3 + tid] : 0.0;
        aa[tid] = in ? ka[3 + D + tid] : 0.0;
        ab[tid] = in ? kb[3 + D + tid] : 0.0;
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, i = it * SR_MMX_IT + lane;
    const bool iv = i < N;
    // the row's registers: u = Li_b M Li_a nu_i, ha = Li_b M az_i, mi = M Li_a nu_i, ka = M az_i
    double u[DT], ha[DT], mi[DT], kv[DT], si, ai, pa;
    {
        double nu[DT], az[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            const double z = (iv && d < D) ? a.Z[(long)i * D + d] : 0.0;
            nu[d] = (iv && d < D) ? z - mq[d] : 0.0;
            az[d] = aa[d] * z;
            nus[tid * DT + d] = la[d] * nu[d];                     // (the thread's own slots: no barrier)
            azs[tid * DT + d] = az[d];
            mi[d] = 0.0;
            kv[d] = 0.0;
        }
#pragma unroll 1                                  // (unrolled, M passes through the registers at once)
        for (int e = 0; e < D; ++e) {
            const double xe = nus[tid * DT + e], ze = azs[tid * DT + e];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                mi[d] = fma(M[d * DT + e], xe, mi[d]);
                kv[d] = fma(M[d * DT + e], ze, kv[d]);
            }
        }
        double qf = 0.0;
        pa = c0a;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            u[d] = lb[d] * mi[d];
            ha[d] = lb[d] * kv[d];
            qf = fma(la[d] * nu[d], nu[d] - mi[d], qf);
            pa = fma(az[d], mq[d] + mi[d], pa);
        }
        si = clog - 0.5 * qf;
        ai = iv ? a.alpha[(long)oa * a.Np + off + i] : 0.0;
    }
    const double* kinv = a.inv_k + (size_t)oa * N * N;
    const double* alb = a.alpha + (long)ob * a.Np + off;
    const int njt = (N + SR_MMX_JT - 1) / SR_MMX_JT, jt0 = diag ? it / (SR_MMX_JT / SR_MMX_IT) : 0;
    double acc = 0.0;
    for (int jt = jt0; jt < njt; ++jt) {
        __syncthreads();                        // (the row set-up above, or the last tile's readers, are done with the slots)
        {
            const int j = jt * SR_MMX_JT + tid;
            const bool jv = j < N;
            double x[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const double z = (jv && d < D) ? a.Z[(long)j * D + d] : 0.0;
                const double nu = (jv && d < D) ? z - mq[d] : 0.0;
                nus[tid * DT + d] = nu;
                azs[tid * DT + d] = ab[d] * z;
                x[d] = lb[d] * nu;
            }
            double qf = 0.0, pb = c0b;
#pragma unroll 1                                  // (unrolled, M is hoisted out of the tile loop into registers)
            for (int d = 0; d < D; ++d) {
                double mj = 0.0;
#pragma unroll
                for (int e = 0; e < DT; ++e) mj = fma(M[d * DT + e], x[e], mj);
                const double nd = nus[tid * DT + d];
                qf = fma(lb[d] * nd, nd - mj, qf);
                pb = fma(azs[tid * DT + d], mq[d] + mj, pb);
            }
            sjs[tid] = -0.5 * qf;
            pbs[tid] = pb;
            ajs[tid] = jv ? alb[j] : 0.0;
        }
        __syncthreads();
        const int cnt = min(SR_MMX_JT, N - jt * SR_MMX_JT);
        double tacc = 0.0;
        for (int jj = w; jj < cnt; jj += 4) {
            double e = si + sjs[jj], f1 = pa, f2 = pbs[jj], f3 = 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                const double nj = nus[jj * DT + d], zj = azs[jj * DT + d];
                e = fma(u[d], nj, e);
                f1 = fma(ha[d], nj, f1);
                f2 = fma(mi[d], zj, f2);
                f3 = fma(kv[d], zj, f3);
            }
            double wv = ai * ajs[jj];
            if (diag && iv) wv -= kinv[(size_t)(jt * SR_MMX_JT + jj) * N + i];
            tacc = fma(wv * fma(f1, f2, f3), exp(e), tacc);
        }
        acc += (diag && jt > jt0) ? 2.0 * tacc : tacc;
    }
    red[tid] = iv ? acc : 0.0;
    mmx_block_sum(red, 1);
    if (tid == 0) a.ws[mmx_off_part(a) + (t * a.npairs + p) * a.nit + it] = red[0];
}

// KX3
__global__ __launch_bounds__(256) void sr_mmx_final_kernel(sr_mmx_args a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.T * a.npairs) return;
    const long t = e / a.npairs;
    const int p = (int)(e % a.npairs), D = a.D, n = a.n_out, N = a.N;
    int oa, ob;
    mmx_pair_of(p, n, oa, ob);
    const double* rec = a.ws + mmx_off_pair(a) + e * mmx_pair_rec(D);
    double* cv = a.cov + t * n * n;
    if (oa != ob && rec[1] != 0.0) {
        cv[oa * n + ob] = 0.0;
        cv[ob * n + oa] = 0.0;
        return;
    }
    const double* part = a.ws + mmx_off_part(a) + e * a.nit;
    double s = 0.0;
    for (int it = 0; it < a.nit; ++it) s += part[it];
    const double *ka = a.kp + (long)oa * SR_KP(D), *kb = a.kp + (long)ob * SR_KP(D);
    const double *ca = a.call + oa * mmx_call_rec(N, D) + (long)N * D, *cb = a.call + ob * mmx_call_rec(N, D) + (long)N * D;
    const double *za = ca + D * D, *zb = cb + D * D;                 // Z^T alpha of the two outputs
    const double *sta = a.ws + mmx_off_stat(a) + (t * n + oa) * mmx_stat_rec(D);
    const double *stb = a.ws + mmx_off_stat(a) + (t * n + ob) * mmx_stat_rec(D);
    const double* S = a.S ? a.S + t * D * D : nullptr;
    const double* m = a.m + t * D;
    // the alpha alpha^T part of (2) - (4) less mu_a mu_b, with everything that carries m cancelled
    double v = ka[1] * kb[1] * s - sta[0] * stb[0];
    for (int d = 0; d < D; ++d) {
        const double ba = ka[3 + 2 * D + d] * za[d], bb = kb[3 + 2 * D + d] * zb[d];
        v = fma(sta[2 + d], bb, v);
        v = fma(stb[2 + d], ba, v);
        if (S) {
            double sb = 0.0;
            for (int c = 0; c < D; ++c) sb = fma(S[d * D + c], kb[3 + 2 * D + c] * zb[c], sb);
            v = fma(ba, sb, v);
        }
    }
    if (oa == ob) {
        // - sum_ij Kinv_ij of (2) - (4), + E[k(x, x)] = c0 v + sum_j (a_j v + b_j) (S_jj + m_j^2)
        double w = ka[2] * ka[1] - 2.0 * sta[1];
        for (int d = 0; d < D; ++d) {
            const double bd = ka[3 + 2 * D + d];
            w = fma(ka[3 + D + d] * ka[1] + bd, (S ? S[d * D + d] : 0.0) + m[d] * m[d], w);
            double r = 0.0;
            for (int c = 0; c < D; ++c)
                r = fma(ka[3 + 2 * D + c] * ((S ? S[d * D + c] : 0.0) + m[d] * m[c]), ca[d * D + c], r);
            w = fma(-bd, r, w);
        }
        v += w;
        cv[oa * n + oa] = v > SR_VAR_CLIP ? v : SR_VAR_CLIP;
    } else {
        cv[oa * n + ob] = v;
        cv[ob * n + oa] = v;
    }
}

// the per-call pass: Kinv_a Z, Z^T Kinv_a Z and Z^T alpha_a of every output into `call` (sr_mmx_call_ws doubles)
template <int DT>
static int mmx_launch_call(const sr_mmx_args& a, hipStream_t s) {
    hipLaunchKernelGGL((sr_mmx_kz_kernel<DT>), dim3((a.N + 255) / 256, a.n_out), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sr_mmx_zkz_kernel<DT>), dim3(a.D, a.n_out), dim3(256), 0, s, a);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

template <int DT>
static int mmx_launch(const sr_mmx_args& a, hipStream_t s) {
    const long nprep = a.T * (a.n_out + a.npairs);
    constexpr int BT = mmx_prep_bt<DT>::value;
    hipLaunchKernelGGL((sr_mmx_prep_kernel<DT>), dim3((unsigned)((nprep + BT - 1) / BT)), dim3(BT), 0, s, a);
    hipLaunchKernelGGL((sr_mmx_mean_kernel<DT>), dim3((unsigned)a.T, a.n_out), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sr_mmx_pair_kernel<DT>), dim3((unsigned)a.T, a.nit, a.npairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sr_mmx_final_kernel, dim3((unsigned)((a.T * a.npairs + 255) / 256)), dim3(256), 0, s, a);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

static sr_mmx_args mmx_args(const double* Z, const double* alpha, const double* kp, int N, int Np, int D, int n_out,
                            const double* inv_k, double* call) {
    sr_mmx_args a{};
    a.Z = Z; a.alpha = alpha; a.kp = kp; a.inv_k = inv_k; a.call = call;
    a.N = N; a.Np = Np; a.D = D; a.n_out = n_out; a.npairs = n_out * (n_out + 1) / 2; a.nit = mmx_nit(N);
    return a;
}

int sr_launch_moment_match_gen_call(const double* Z, const double* alpha, const double* kp, int N, int Np, int D, int n_out,
                                    const double* inv_k, double* call, hipStream_t s) {
    const sr_mmx_args a = mmx_args(Z, alpha, kp, N, Np, D, n_out, inv_k, call);
    SR_CHECK(n_out < 65536, SR_EUNSUPPORTED, "moment_match: n_out=%d outside the launch grid", n_out);
    return sr_pick_le<4, 8, 12>("moment_match", D, [&](auto dt) { return mmx_launch_call<decltype(dt)::value>(a, s); });
}

// one chunk of T queries behind the per-call pass; ws: T x sr_mmx_ws_per_query doubles
int sr_launch_moment_match_gen(const double* Z, const double* alpha, const double* kp, int N, int Np, int D, int n_out,
                               const double* m, const double* S, long T, const double* inv_k, double* mu, double* cov,
                               double* V, const double* call, double* ws, hipStream_t s) {
    sr_mmx_args a = mmx_args(Z, alpha, kp, N, Np, D, n_out, inv_k, const_cast<double*>(call));
    a.m = m; a.S = S; a.mu = mu; a.cov = cov; a.V = V; a.ws = ws; a.T = T;
    SR_CHECK(a.npairs < 65536 && a.nit < 65536 && T <= sr_mmx_max_queries(N, n_out), SR_EUNSUPPORTED,
             "moment_match: n_out=%d N=%d T=%ld outside the launch grid", n_out, N, T);
    return sr_pick_le<4, 8, 12>("moment_match", D, [&](auto dt) { return mmx_launch<decltype(dt)::value>(a, s); });
}
