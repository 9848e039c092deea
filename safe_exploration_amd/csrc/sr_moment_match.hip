// sr_moment_match.hip -- exact moment matching: an ARD-RBF GP evaluated at Gaussian inputs z ~ N(m, S)
// (Deisenroth's closed forms; sr_gp_moment_match).  Per query and output a
//   q_ai = sf2_a |S L_a^-1 + I|^-1/2 exp(-1/2 nu_i^T (S + L_a)^-1 nu_i),   nu_i = z_i - m,  L_a = diag(ls_a^2)
//   mu_a = sum_i alpha_ai q_ai,        V_a = (S + L_a)^-1 sum_i alpha_ai q_ai nu_i      (cov(z, g_a) = S V_a)
// and per pair of outputs a <= b, with R = S (L_a^-1 + L_b^-1) + I and M = R^-1 S,
//   log Q_ij = log(sf2_a sf2_b) - 1/2 log|R| + s^a_i + s^b_j + u_i . nu_j
//   s^a_i = -1/2 nu_i^T G_a nu_i,  G_a = L_a^-1 - L_a^-1 M L_a^-1,   u_i = P nu_i,  P = L_b^-1 M L_a^-1
//   Cov[a, b] = sum_ij (alpha_ai alpha_bj - [a == b] Kinv_a,ij) Q_ij - mu_a mu_b + [a == b] sf2_a
// Nothing inverts S (it is singular whenever it comes from a state of lower dimension): every D x D factorisation is of
// I + D^1/2 S D^1/2 with a positive diagonal D, which is SPD for any PSD S and the identity for S = 0.
//
// Four launches per chunk of queries, all deterministic (no floating-point atomics):
//   KM0 sr_mm_prep_kernel   one thread per (query, output | pair): the D x D algebra (in LDS), once, into the handle's scratch
//   KM1 sr_mm_mean_kernel   one workgroup per (query, output): mu and V, O(N D^2)
//   KM2 sr_mm_pair_kernel   one workgroup per (query, tile of SR_MM_IT rows i, pair): the double sum -- a lane keeps u_i, s_i and
//                           alpha_ai of ITS row in registers, the four wavefronts share the j of a staged tile of SR_MM_JT rows
//                           (nu_j, s_j, alpha_bj in LDS, read as broadcasts); D FMAs, one exp and one weighted add per (i, j);
//                           a == b: Q and the weight are symmetric in (i, j), so j tiles before the one that holds the i tile
//                           are skipped and those behind it count twice; Kinv_a is read as [j][i] (coalesced along the lanes)
//   KM3 sr_mm_final_kernel  one thread per (query, pair): the i tiles' partial sums in order, - mu_a mu_b, clip, mirror
// Queries are the fastest grid index of KM2: the workgroups in flight at one time read the same tile of Kinv_a.
// The reverse pass (sr_gp_moment_match_vjp: KG1 - KG4, behind KM0 and KM1) is the second half of this file.
#include "sr_common.h"

#define SR_MM_IT 64          // rows i per workgroup of KM2 (one per lane)
#define SR_MM_JT 256         // rows j per staged tile of KM2 (one per thread while staging; 64 per wavefront in the loop)
static_assert(SR_MM_JT % SR_MM_IT == 0 && SR_MM_JT == 256, "KM2: j tiles hold whole i tiles, one j per thread");

struct sr_mm_args {
    const double *Z, *alpha, *ls, *sf2;      // the model as the handle holds it (alpha n_out x Np, front padding)
    const double *m, *S, *inv_k;             // T x D, T x D x D | NULL, n_out x N x N
    double *mu, *cov, *V;                    // T x n_out, T x n_out x n_out, T x n_out x D | NULL
    double* ws;                              // [mean records | pair records | partial sums] of this chunk
    int N, Np, D, n_out, npairs, nit;
    long T;
    // the seed-dependent kernels of the reverse pass (KG1, KG3) may run on a slice of a larger record block: queries
    // q0 .. q0 + T of the Tq whose records ws holds (every other pointer is then the slice's own).  Elsewhere q0 = 0, Tq = T.
    long q0, Tq;
};

__host__ __device__ static inline long mm_mean_rec(int D) { return 1 + (long)D * D; }       // [c0, W (D x D)]
__host__ __device__ static inline long mm_pair_rec(int D) { return 2 + 3 * (long)D * D; }   // [c, point, P, G_a, G_b]
static inline int mm_nit(int N) { return (N + SR_MM_IT - 1) / SR_MM_IT; }

long sr_mm_ws_per_query(int N, int D, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2;
    return n_out * mm_mean_rec(D) + npairs * mm_pair_rec(D) + npairs * mm_nit(N);
}

// p-th pair (a <= b) in row-major order of the upper triangle
__device__ static inline void mm_pair_of(int p, int n, int& a, int& b) {
    a = 0;
    while (p >= n - a) { p -= n - a; ++a; }
    b = a + p;
}

// KM0 keeps its D x D matrices in LDS, element-major with the threads of the block innermost (a thread's own column: no
// bank conflicts, and no dynamically indexed private array -- those live in scratch memory)
#define MM_AT(M, i, j) M[((i) * DT + (j)) * BT + threadIdx.x]
#define MM_V(v, d) v[(d) * BT + threadIdx.x]
template <int DT> struct mm_prep_bt { static constexpr int value = DT <= 4 ? 64 : (DT <= 8 ? 32 : 16); };

// lower Cholesky factor in place (lower triangle read and written); returns log det
template <int DT, int BT>
__device__ static inline double mm_chol(double* C, int D) {
    double logdet = 0.0;
    for (int k = 0; k < D; ++k) {
        double s = MM_AT(C, k, k);
        for (int p = 0; p < k; ++p) s -= MM_AT(C, k, p) * MM_AT(C, k, p);
        logdet += log(s);
        const double l = sqrt(s), inv = 1.0 / l;
        MM_AT(C, k, k) = l;
        for (int i = k + 1; i < D; ++i) {
            double v = MM_AT(C, i, k);
            for (int p = 0; p < k; ++p) v -= MM_AT(C, i, p) * MM_AT(C, k, p);
            MM_AT(C, i, k) = v * inv;
        }
    }
    return logdet;
}

// KM0
template <int DT>
__global__ __launch_bounds__(mm_prep_bt<DT>::value) void sr_mm_prep_kernel(sr_mm_args a) {
    constexpr int BT = mm_prep_bt<DT>::value;
    __shared__ double C[DT * DT * BT], X[DT * DT * BT], r[DT * BT], la[DT * BT], lb[DT * BT];
    const int D = a.D, nslot = a.n_out + a.npairs;
    const long e = (long)blockIdx.x * BT + threadIdx.x;
    if (e >= a.T * nslot) return;
    const long t = e / nslot;
    const int slot = (int)(e % nslot);
    const double* S = a.S ? a.S + t * D * D : nullptr;
    if (slot < a.n_out) {
        // mean of output o: C = I + L^-1/2 S L^-1/2 = Lc Lc^T;  (S + L)^-1 = W^T W with W = Lc^-1 L^-1/2;  |S L^-1 + I| = |C|
        const int o = slot;
        for (int d = 0; d < D; ++d) MM_V(r, d) = 1.0 / a.ls[o * D + d];
        for (int i = 0; i < D; ++i)
            for (int j = 0; j <= i; ++j)
                MM_AT(C, i, j) = (i == j ? 1.0 : 0.0) + (S ? MM_V(r, i) * MM_V(r, j) * S[i * D + j] : 0.0);
        const double logdet = mm_chol<DT, BT>(C, D);
        // X = Lc^-1 (lower), column by column
        for (int j = 0; j < D; ++j) {
            MM_AT(X, j, j) = 1.0 / MM_AT(C, j, j);
            for (int i = j + 1; i < D; ++i) {
                double v = 0.0;
                for (int p = j; p < i; ++p) v -= MM_AT(C, i, p) * MM_AT(X, p, j);
                MM_AT(X, i, j) = v / MM_AT(C, i, i);
            }
        }
        double* rec = a.ws + (t * a.n_out + o) * mm_mean_rec(D);
        rec[0] = log(a.sf2[o]) - 0.5 * logdet;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < D; ++j) rec[1 + i * D + j] = j <= i ? MM_AT(X, i, j) * MM_V(r, j) : 0.0;
        return;
    }
    // pair (oa, ob): Ld = L_a^-1 + L_b^-1, C = I + Ld^1/2 S Ld^1/2 = Lc Lc^T, |R| = |C|, M = Ld^-1/2 (C^-1 (C - I)) Ld^-1/2
    int oa, ob;
    mm_pair_of(slot - a.n_out, a.n_out, oa, ob);
    bool point = true;
    for (int d = 0; d < D; ++d) {
        const double x = a.ls[oa * D + d], y = a.ls[ob * D + d];
        MM_V(la, d) = 1.0 / (x * x);
        MM_V(lb, d) = 1.0 / (y * y);
        MM_V(r, d) = sqrt(MM_V(la, d) + MM_V(lb, d));
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            const double sij = S ? S[i * D + j] : 0.0;
            if (sij != 0.0) point = false;
            const double bij = MM_V(r, i) * MM_V(r, j) * sij;
            MM_AT(C, i, j) = (i == j ? 1.0 : 0.0) + bij;
            MM_AT(X, i, j) = bij;
            MM_AT(X, j, i) = bij;
        }
    const double logdet = mm_chol<DT, BT>(C, D);
    for (int j = 0; j < D; ++j) {              // X[:, j] <- C^-1 X[:, j]
        for (int i = 0; i < D; ++i) {
            double v = MM_AT(X, i, j);
            for (int p = 0; p < i; ++p) v -= MM_AT(C, i, p) * MM_AT(X, p, j);
            MM_AT(X, i, j) = v / MM_AT(C, i, i);
        }
        for (int i = D - 1; i >= 0; --i) {
            double v = MM_AT(X, i, j);
            for (int p = i + 1; p < D; ++p) v -= MM_AT(C, p, i) * MM_AT(X, p, j);
            MM_AT(X, i, j) = v / MM_AT(C, i, i);
        }
    }
    double* rec = a.ws + a.T * a.n_out * mm_mean_rec(D) + (t * a.npairs + (slot - a.n_out)) * mm_pair_rec(D);
    rec[0] = log(a.sf2[oa] * a.sf2[ob]) - 0.5 * logdet;
    rec[1] = point ? 1.0 : 0.0;
    double *P = rec + 2, *Ga = P + D * D, *Gb = Ga + D * D;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            const double mij = 0.5 * (MM_AT(X, i, j) + MM_AT(X, j, i)) / (MM_V(r, i) * MM_V(r, j));
            P[i * D + j] = MM_V(lb, i) * mij * MM_V(la, j);
            Ga[i * D + j] = (i == j ? MM_V(la, i) : 0.0) - MM_V(la, i) * mij * MM_V(la, j);
            Gb[i * D + j] = (i == j ? MM_V(lb, i) : 0.0) - MM_V(lb, i) * mij * MM_V(lb, j);
        }
}
#undef MM_AT
#undef MM_V

// D x D record -> DT x DT in LDS (zero padding), all 256 threads
template <int DT>
__device__ static inline void mm_load_mat(double* dst, const double* src, int D) {
    for (int e = threadIdx.x; e < DT * DT; e += 256) {
        const int i = e / DT, j = e % DT;
        dst[e] = (i < D && j < D) ? src[i * D + j] : 0.0;
    }
}

// sum of red[k * 256 + tid] over tid, k < nk, in a fixed tree order; the sums end in red[k * 256]
__device__ static inline void mm_block_sum(double* red, int nk) {
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s)
            for (int k = 0; k < nk; ++k) red[k * 256 + threadIdx.x] += red[k * 256 + threadIdx.x + s];
    }
    __syncthreads();
}

// KM1
template <int DT>
__global__ __launch_bounds__(256) void sr_mm_mean_kernel(sr_mm_args a) {
    __shared__ double W[DT * DT], mq[DT], red[(DT + 1) * 256];
    const int D = a.D, tid = threadIdx.x, o = blockIdx.y, off = a.Np - a.N;
    const long t = blockIdx.x;
    const double* rec = a.ws + (t * a.n_out + o) * mm_mean_rec(D);
    const double c0 = rec[0];
    mm_load_mat<DT>(W, rec + 1, D);
    if (tid < DT) mq[tid] = tid < D ? a.m[t * D + tid] : 0.0;
    __syncthreads();
    double acc[DT + 1];
#pragma unroll
    for (int k = 0; k <= DT; ++k) acc[k] = 0.0;
    const double* al = a.alpha + (long)o * a.Np + off;
    for (int i = tid; i < a.N; i += 256) {
        double nu[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) nu[d] = d < D ? a.Z[(long)i * D + d] - mq[d] : 0.0;
        double e = 0.0;
#pragma unroll 1                                  // (unrolled, the whole of W is kept in registers: 256 VGPRs at DT = 12)
        for (int r = 0; r < D; ++r) {
            double y = 0.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) y = fma(W[r * DT + c], nu[c], y);      // (zero above the diagonal)
            e = fma(y, y, e);
        }
        const double q = al[i] * exp(c0 - 0.5 * e);
        acc[0] += q;
#pragma unroll
        for (int d = 0; d < DT; ++d) acc[1 + d] = fma(q, nu[d], acc[1 + d]);
    }
#pragma unroll
    for (int k = 0; k <= DT; ++k) red[k * 256 + tid] = acc[k];
    mm_block_sum(red, DT + 1);
    if (tid == 0) a.mu[t * a.n_out + o] = red[0];
    if (a.V && tid < D) {
        // V = W^T (W g), g = sum_i alpha_i q_i nu_i
        double v = 0.0;
        for (int r = 0; r < D; ++r) {
            double y = 0.0;
            for (int c = 0; c <= r; ++c) y = fma(W[r * DT + c], red[(1 + c) * 256], y);
            v = fma(W[r * DT + tid], y, v);
        }
        a.V[(t * a.n_out + o) * D + tid] = v;
    }
}

// KM2
template <int DT>
__global__ __launch_bounds__(256) void sr_mm_pair_kernel(sr_mm_args a) {
    __shared__ double P[DT * DT], Ga[DT * DT], Gb[DT * DT], mq[DT];
    __shared__ double nus[SR_MM_JT * DT], sjs[SR_MM_JT], ajs[SR_MM_JT], red[256];
    const int D = a.D, N = a.N, tid = threadIdx.x, it = blockIdx.y, p = blockIdx.z, off = a.Np - N;
    const long t = blockIdx.x;
    int oa, ob;
    mm_pair_of(p, a.n_out, oa, ob);
    const bool diag = oa == ob;
    const double* rec = a.ws + a.T * a.n_out * mm_mean_rec(D) + (t * a.npairs + p) * mm_pair_rec(D);
    const double c = rec[0];
    if (!diag && rec[1] != 0.0) return;         // a point input: the outputs are independent, KM3 writes the zero
    mm_load_mat<DT>(P, rec + 2, D);
    mm_load_mat<DT>(Ga, rec + 2 + D * D, D);
    mm_load_mat<DT>(Gb, rec + 2 + 2 * D * D, D);
    if (tid < DT) mq[tid] = tid < D ? a.m[t * D + tid] : 0.0;
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, i = it * SR_MM_IT + lane;
    const bool iv = i < N;
    double u[DT], si, ai;
    {
        double nu[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) nu[d] = (iv && d < D) ? a.Z[(long)i * D + d] - mq[d] : 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) { nus[tid * DT + d] = nu[d]; u[d] = 0.0; }      // (the thread's own slot: no barrier)
        double qf = 0.0;
#pragma unroll 1                                  // (unrolled, P and G_a pass through 256 VGPRs at once)
        for (int e = 0; e < D; ++e) {
            const double ne = nus[tid * DT + e];
            double g = 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                u[d] = fma(P[d * DT + e], ne, u[d]);
                g = fma(Ga[e * DT + d], nu[d], g);
            }
            qf = fma(ne, g, qf);
        }
        si = c - 0.5 * qf;
        ai = iv ? a.alpha[(long)oa * a.Np + off + i] : 0.0;
    }
    const double* kinv = a.inv_k + (size_t)oa * N * N;
    const double* alb = a.alpha + (long)ob * a.Np + off;
    const int njt = (N + SR_MM_JT - 1) / SR_MM_JT, jt0 = diag ? it / (SR_MM_JT / SR_MM_IT) : 0;
    double acc = 0.0;
    for (int jt = jt0; jt < njt; ++jt) {
        {
            const int j = jt * SR_MM_JT + tid;
            const bool jv = j < N;
            double nu[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) nu[d] = (jv && d < D) ? a.Z[(long)j * D + d] - mq[d] : 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) nus[tid * DT + d] = nu[d];
            double qf = 0.0;
#pragma unroll 1                                  // (unrolled, G_b is hoisted out of the tile loop into registers)
            for (int d = 0; d < D; ++d) {
                double g = 0.0;
#pragma unroll
                for (int e = 0; e < DT; ++e) g = fma(Gb[d * DT + e], nu[e], g);
                qf = fma(nus[tid * DT + d], g, qf);
            }
            sjs[tid] = -0.5 * qf;
            ajs[tid] = jv ? alb[j] : 0.0;
        }
        __syncthreads();
        const int cnt = min(SR_MM_JT, N - jt * SR_MM_JT);
        double tacc = 0.0;
        for (int jj = w; jj < cnt; jj += 4) {
            double e = si + sjs[jj];
#pragma unroll
            for (int d = 0; d < DT; ++d) e = fma(u[d], nus[jj * DT + d], e);
            double wv = ai * ajs[jj];
            if (diag && iv) wv -= kinv[(size_t)(jt * SR_MM_JT + jj) * N + i];
            tacc = fma(wv, exp(e), tacc);      // (a compensated sum changes nothing: the error left is the rounding of e)
        }
        acc += (diag && jt > jt0) ? 2.0 * tacc : tacc;
        __syncthreads();
    }
    red[tid] = iv ? acc : 0.0;
    mm_block_sum(red, 1);
    if (tid == 0) a.ws[a.T * (a.n_out * mm_mean_rec(D) + a.npairs * mm_pair_rec(D)) + (t * a.npairs + p) * a.nit + it] = red[0];
}

// KM3
__global__ __launch_bounds__(256) void sr_mm_final_kernel(sr_mm_args a) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.T * a.npairs) return;
    const long t = e / a.npairs;
    const int p = (int)(e % a.npairs), D = a.D, n = a.n_out;
    int oa, ob;
    mm_pair_of(p, n, oa, ob);
    const double* rec = a.ws + a.T * n * mm_mean_rec(D) + e * mm_pair_rec(D);
    double* cv = a.cov + t * n * n;
    if (oa != ob && rec[1] != 0.0) {
        cv[oa * n + ob] = 0.0;
        cv[ob * n + oa] = 0.0;
        return;
    }
    const double* part = a.ws + a.T * (n * mm_mean_rec(D) + a.npairs * mm_pair_rec(D)) + e * a.nit;
    double s = 0.0;
    for (int it = 0; it < a.nit; ++it) s += part[it];
    double v = s - a.mu[t * n + oa] * a.mu[t * n + ob];
    if (oa == ob) {
        v += a.sf2[oa];
        cv[oa * n + oa] = v > SR_VAR_CLIP ? v : SR_VAR_CLIP;
    } else {
        cv[oa * n + ob] = v;
        cv[ob * n + oa] = v;
    }
}

template <int DT>
static int mm_launch(const sr_mm_args& a, hipStream_t s) {
    const long nprep = a.T * (a.n_out + a.npairs);
    constexpr int BT = mm_prep_bt<DT>::value;
    hipLaunchKernelGGL((sr_mm_prep_kernel<DT>), dim3((unsigned)((nprep + BT - 1) / BT)), dim3(BT), 0, s, a);
    hipLaunchKernelGGL((sr_mm_mean_kernel<DT>), dim3((unsigned)a.T, a.n_out), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sr_mm_pair_kernel<DT>), dim3((unsigned)a.T, a.nit, a.npairs), dim3(256), 0, s, a);
    hipLaunchKernelGGL(sr_mm_final_kernel, dim3((unsigned)((a.T * a.npairs + 255) / 256)), dim3(256), 0, s, a);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

// queries one launch sequence may take: grid.y / grid.z stay below 65536, the grid of KM2 below 2^23 workgroups
long sr_mm_max_queries(int N, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2, per = npairs * mm_nit(N);
    const long q = ((long)1 << 23) / per;
    return q < 1 ? 1 : q;
}

// one chunk of T queries; ws: T x sr_mm_ws_per_query doubles
int sr_launch_moment_match(const double* Z, const double* alpha, const double* ls, const double* sf2, int N, int Np, int D,
                           int n_out, const double* m, const double* S, long T, const double* inv_k, double* mu,
                           double* cov, double* V, double* ws, hipStream_t s) {
    sr_mm_args a;
    a.Z = Z; a.alpha = alpha; a.ls = ls; a.sf2 = sf2; a.m = m; a.S = S; a.inv_k = inv_k; a.mu = mu; a.cov = cov; a.V = V;
    a.ws = ws; a.N = N; a.Np = Np; a.D = D; a.n_out = n_out; a.npairs = n_out * (n_out + 1) / 2; a.nit = mm_nit(N);
    a.T = T; a.q0 = 0; a.Tq = T;
    SR_CHECK(a.npairs < 65536 && a.nit < 65536 && T <= sr_mm_max_queries(N, n_out), SR_EUNSUPPORTED,
             "moment_match: n_out=%d N=%d T=%ld outside the launch grid", n_out, N, T);
    return sr_pick_le<4, 8, 12>("moment_match", D, [&](auto dt) { return mm_launch<decltype(dt)::value>(a, s); });
}

// ================================================================================================================
// Reverse pass (sr_gp_moment_match_vjp): m_bar = dL/dm and S_bar = dL/dS of
//   L = mu_bar . mu + sum_ab cov_bar_ab Cov_ab + sum_a V_bar_a . V_a        (Cov the unclipped closed form)
// Only Cs = (cov_bar + cov_bar^T) / 2 counts.  With A_a = (S + L_a)^-1, h_a = A_a V_bar_a, me_a = mu_bar_a - 2 sum_b Cs_ab mu_b
// (the - mu_a mu_b of Cov) and c_i = alpha_ai q_ai (me_a + h_a . nu_i), per output
//   m_bar += A_a sum_i c_i nu_i - mu_a h_a
//   S_bar += 1/2 A_a (sum_i c_i nu_i nu_i^T) A_a - 1/2 (sum_i c_i) A_a - 1/2 (h_a V_a^T + V_a h_a^T)
// and per pair a <= b with weight om = Cs_aa or 2 Cs_ab (the ordered pairs (a, b) and (b, a) give the same term), t_ij = w_ij Q_ij,
// y_ij = R^-T zeta_ij = Ya nu_i + Yb nu_j, Ya = R^-T L_a^-1, Yb = R^-T L_b^-1, R^-T = I - Ld M, Ld R^-1 = Ld - Ld M Ld:
//   m_bar += om sum_ij t_ij y_ij,      S_bar += om (1/2 sum_ij t_ij y_ij y_ij^T - 1/2 (sum_ij t_ij) Ld R^-1)
// y is linear in nu_i and nu_j, so nothing of size D^2 is kept per (i, j): a lane keeps r_i = sum_j t_ij and
// g_i = sum_j t_ij nu_j of ITS row, and
//   sum_ij t_ij y y^T = Ya [sum_i r_i nu_i nu_i^T] Ya^T + Ya [sum_i nu_i g_i^T] Yb^T + transpose + Yb [sum_j c_j nu_j nu_j^T] Yb^T
// with the column sums c_j = sum_i t_ij from a second pass with the outputs exchanged (a == b: c = r).  The symmetric-half
// trick of KM2 gives the total only, so every pass runs over full rows; there is no point-input shortcut either (dCov_ab/dS
// is not zero at S = 0).  M comes back from the forward's record as M_ij = P_ij ls_b,i^2 ls_a,j^2: no new factorisation.
//
// Launches per chunk, behind KM0 and KM1 of the forward (mu and V go to the scratch), all deterministic:
//   KG1 sr_mmg_mean_kernel     one workgroup per (query, output): the 1 + D + D (D + 1) / 2 moments of c_i in registers, block
//                              sums in groups of DT + 1, then the D x D algebra -> one contribution record [m (D) | S (D x D)]
//   KG2 sr_mmg_pair_kernel     one workgroup per (query, tile of SR_MM_IT rows i, ORDERED pair): KM2's loop over all j tiles with
//                              1 + D accumulators per lane (1 for a > b: only the column sums are wanted), then per tile the
//                              sums over its rows of r [1, nu, nu nu^T] and nu g^T, one thread per sum, rows in order
//   KG3 sr_mmg_pairfin_kernel  one workgroup per (query, pair a <= b): the tiles' sums in order, Ya, Yb, Ld R^-1, the seed
//                              -> one contribution record
//   KG4 sr_mmg_final_kernel    one thread per (query, element): the records in order; S_bar = (C + C^T) / 2, exactly symmetric
struct sr_mmg_args {
    sr_mm_args f;                                  // the forward's arguments: mu, V and ws (records) point into the scratch
    const double *mu_bar, *cov_bar, *V_bar;        // T x n_out, T x n_out x n_out, T x n_out x D; NULL = zero
    double *m_bar, *S_bar;                         // T x D, T x D x D; either may be NULL
    double *contrib, *part;                        // T x (n_out + npairs) x (D + D D); T x n_out^2 x nit x mmg_nstat(D)
};

__host__ __device__ static inline int mmg_nrstat(int D) { return 1 + D + D * (D + 1) / 2; }     // sums of r [1, nu, nu nu^T]
__host__ __device__ static inline int mmg_nstat(int D) { return mmg_nrstat(D) + D * D; }        // ... and of nu g^T
__host__ __device__ static inline int mmg_crec(int D) { return D + D * D; }
// (d, e), e <= d, of the k-th element of a packed lower triangle; and back
__device__ static inline void mmg_tri_of(int k, int& d, int& e) {
    d = 0;
    while (k > d) { k -= d + 1; ++d; }
    e = k;
}
__device__ static inline int mmg_tri(int d, int e) { return d >= e ? d * (d + 1) / 2 + e : e * (e + 1) / 2 + d; }

static long mmg_fwd_recs(int D, int n_out) {
    return n_out * mm_mean_rec(D) + ((long)n_out * (n_out + 1) / 2) * mm_pair_rec(D);
}
long sr_mmg_ws_per_query(int N, int D, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2;
    return mmg_fwd_recs(D, n_out) + n_out + (long)n_out * D + (n_out + npairs) * mmg_crec(D) +
           (long)n_out * n_out * mm_nit(N) * mmg_nstat(D);
}
// queries one launch sequence may take: the grid of KG2 (n_out^2 ordered pairs) stays below 2^23 workgroups
long sr_mmg_max_queries(int N, int n_out) {
    const long q = ((long)1 << 23) / ((long)n_out * n_out * mm_nit(N));
    return q < 1 ? 1 : q;
}

// KG1
template <int DT>
__global__ __launch_bounds__(256) void sr_mmg_mean_kernel(sr_mmg_args g) {
    constexpr int G = DT + 1, NG = 1 + DT / 2, NM = G * NG;
    static_assert(NM == 1 + DT + DT * (DT + 1) / 2, "KG1: the moments go in whole groups of DT + 1");
    __shared__ double W[DT * DT], A[DT * DT], U[DT * DT], mq[DT], h[DT], red[G * 256], mom[NM];
    const sr_mm_args& a = g.f;
    const int D = a.D, n = a.n_out, tid = threadIdx.x, o = blockIdx.y, off = a.Np - a.N;
    const long t = blockIdx.x;
    const double* rec = a.ws + ((a.q0 + t) * n + o) * mm_mean_rec(D);
    const double c0 = rec[0];
    mm_load_mat<DT>(W, rec + 1, D);
    if (tid < DT) mq[tid] = tid < D ? a.m[t * D + tid] : 0.0;
    __syncthreads();
    for (int e = tid; e < DT * DT; e += 256) {              // A = W^T W = (S + L)^-1, zero padding
        const int i = e / DT, j = e % DT;
        double s = 0.0;
        for (int r = 0; r < DT; ++r) s = fma(W[r * DT + i], W[r * DT + j], s);
        A[e] = s;
    }
    __syncthreads();
    if (tid < DT) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = fma(A[tid * DT + j], g.V_bar ? g.V_bar[(t * n + o) * D + j] : 0.0, s);
        h[tid] = s;
    }
    double me = g.mu_bar ? g.mu_bar[t * n + o] : 0.0;
    for (int b = 0; b < n; ++b) {
        const double cs = g.cov_bar ? 0.5 * (g.cov_bar[(t * n + o) * n + b] + g.cov_bar[(t * n + b) * n + o]) : 0.0;
        me = fma(-2.0 * cs, a.mu[t * n + b], me);
    }
    __syncthreads();
    double hr[DT], acc[NM];
#pragma unroll
    for (int d = 0; d < DT; ++d) hr[d] = h[d];
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0.0;
    const double* al = a.alpha + (long)o * a.Np + off;
    for (int i = tid; i < a.N; i += 256) {
        double nu[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) nu[d] = d < D ? a.Z[(long)i * D + d] - mq[d] : 0.0;
        double e = 0.0;
#pragma unroll 1
        for (int r = 0; r < D; ++r) {
            double y = 0.0;
#pragma unroll
            for (int c = 0; c < DT; ++c) y = fma(W[r * DT + c], nu[c], y);
            e = fma(y, y, e);
        }
        double hn = me;
#pragma unroll
        for (int d = 0; d < DT; ++d) hn = fma(hr[d], nu[d], hn);
        const double c = al[i] * exp(c0 - 0.5 * e) * hn;
        acc[0] += c;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            const double cn = c * nu[d];
            acc[1 + d] += cn;
#pragma unroll
            for (int e2 = 0; e2 <= d; ++e2) acc[1 + DT + d * (d + 1) / 2 + e2] = fma(cn, nu[e2], acc[1 + DT + d * (d + 1) / 2 + e2]);
        }
    }
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
#pragma unroll
        for (int k = 0; k < G; ++k) red[k * 256 + tid] = acc[gi * G + k];
        mm_block_sum(red, G);
        if (tid < G) mom[gi * G + tid] = red[tid * 256];
        __syncthreads();
    }
    // mom = [s0 | s1 (DT) | s2 packed (DT)]:  U = A s2
    for (int e = tid; e < DT * DT; e += 256) {
        const int i = e / DT, j = e % DT;
        double s = 0.0;
        for (int k = 0; k < DT; ++k) s = fma(A[i * DT + k], mom[1 + DT + mmg_tri(k, j)], s);
        U[e] = s;
    }
    __syncthreads();
    double* cr = g.contrib + (t * (n + a.npairs) + o) * mmg_crec(D);
    const double mu_o = a.mu[t * n + o];
    const double* Vo = a.V + (t * n + o) * D;
    for (int e = tid; e < DT * DT; e += 256) {
        const int i = e / DT, j = e % DT;
        if (i >= D || j >= D) continue;
        double s = 0.0;
        for (int k = 0; k < DT; ++k) s = fma(U[i * DT + k], A[k * DT + j], s);
        cr[D + i * D + j] = 0.5 * s - 0.5 * mom[0] * A[e] - 0.5 * (h[i] * Vo[j] + Vo[i] * h[j]);
    }
    if (tid < D) {
        double s = 0.0;
        for (int k = 0; k < DT; ++k) s = fma(A[tid * DT + k], mom[1 + k], s);
        cr[tid] = s - mu_o * h[tid];
    }
}

// D x D record -> DT x DT in LDS, transposed (zero padding), all 256 threads
template <int DT>
__device__ static inline void mm_load_mat_t(double* dst, const double* src, int D) {
    for (int e = threadIdx.x; e < DT * DT; e += 256) {
        const int i = e / DT, j = e % DT;
        dst[e] = (i < D && j < D) ? src[j * D + i] : 0.0;
    }
}

// KG2
template <int DT>
__global__ __launch_bounds__(256) void sr_mmg_pair_kernel(sr_mmg_args g) {
    constexpr int NF = 1 + 2 * DT, NC = 1 + DT;          // fields of a staged row [r | g | nu]; accumulators of a lane
    static_assert(3 * NC * 64 <= SR_MM_JT * DT, "KG2: the wavefronts' partial sums are exchanged through the j tile's LDS");
    __shared__ double P[DT * DT], Ga[DT * DT], Gb[DT * DT], mq[DT];
    __shared__ double nus[SR_MM_JT * DT], sjs[SR_MM_JT], ajs[SR_MM_JT], stage[SR_MM_IT * NF];
    const sr_mm_args& a = g.f;
    const int D = a.D, N = a.N, n = a.n_out, tid = threadIdx.x, it = blockIdx.y, z = blockIdx.z, off = a.Np - N;
    const int oa = z / n, ob = z % n;
    const long t = blockIdx.x;
    const bool diag = oa == ob, swap = oa > ob;          // swap: rows i of the record's second output, only r is wanted
    const int lo = swap ? ob : oa, hi = swap ? oa : ob, p = lo * n - lo * (lo - 1) / 2 + (hi - lo);
    const double* rec = a.ws + a.T * n * mm_mean_rec(D) + (t * a.npairs + p) * mm_pair_rec(D);
    const double c = rec[0];
    if (swap) {
        mm_load_mat_t<DT>(P, rec + 2, D);
        mm_load_mat<DT>(Ga, rec + 2 + 2 * D * D, D);
        mm_load_mat<DT>(Gb, rec + 2 + D * D, D);
    } else {
        mm_load_mat<DT>(P, rec + 2, D);
        mm_load_mat<DT>(Ga, rec + 2 + D * D, D);
        mm_load_mat<DT>(Gb, rec + 2 + 2 * D * D, D);
    }
    if (tid < DT) mq[tid] = tid < D ? a.m[t * D + tid] : 0.0;
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6, i = it * SR_MM_IT + lane;
    const bool iv = i < N;
    double u[DT], si, ai;
    {
        double nu[DT];
#pragma unroll
        for (int d = 0; d < DT; ++d) nu[d] = (iv && d < D) ? a.Z[(long)i * D + d] - mq[d] : 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) { nus[tid * DT + d] = nu[d]; u[d] = 0.0; }      // (the thread's own slot: no barrier)
        double qf = 0.0;
#pragma unroll 1
        for (int e = 0; e < D; ++e) {
            const double ne = nus[tid * DT + e];
            double q = 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
                u[d] = fma(P[d * DT + e], ne, u[d]);
                q = fma(Ga[e * DT + d], nu[d], q);
            }
            qf = fma(ne, q, qf);
        }
        si = c - 0.5 * qf;
        ai = iv ? a.alpha[(long)oa * a.Np + off + i] : 0.0;
    }
    const double* kinv = a.inv_k + (size_t)oa * N * N;
    const double* alb = a.alpha + (long)ob * a.Np + off;
    const int njt = (N + SR_MM_JT - 1) / SR_MM_JT;
    double r = 0.0, gs[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) gs[d] = 0.0;
    for (int jt = 0; jt < njt; ++jt) {
        {
            const int j = jt * SR_MM_JT + tid;
            const bool jv = j < N;
            double nu[DT];
#pragma unroll
            for (int d = 0; d < DT; ++d) nu[d] = (jv && d < D) ? a.Z[(long)j * D + d] - mq[d] : 0.0;
#pragma unroll
            for (int d = 0; d < DT; ++d) nus[tid * DT + d] = nu[d];
            double qf = 0.0;
#pragma unroll 1
            for (int d = 0; d < D; ++d) {
                double q = 0.0;
#pragma unroll
                for (int e = 0; e < DT; ++e) q = fma(Gb[d * DT + e], nu[e], q);
                qf = fma(nus[tid * DT + d], q, qf);
            }
            sjs[tid] = -0.5 * qf;
            ajs[tid] = jv ? alb[j] : 0.0;
        }
        __syncthreads();
        const int cnt = min(SR_MM_JT, N - jt * SR_MM_JT);
        for (int jj = w; jj < cnt; jj += 4) {
            double e = si + sjs[jj];
#pragma unroll
            for (int d = 0; d < DT; ++d) e = fma(u[d], nus[jj * DT + d], e);
            double wv = ai * ajs[jj];
            if (diag && iv) wv -= kinv[(size_t)(jt * SR_MM_JT + jj) * N + i];
            const double tv = wv * exp(e);
            r += tv;
            if (!swap) {
#pragma unroll
                for (int d = 0; d < DT; ++d) gs[d] = fma(tv, nus[jj * DT + d], gs[d]);
            }
        }
        __syncthreads();
    }
    // the four wavefronts' sums of a row, added in order by the first; then the row [r | g | nu] staged for the tile's sums
    if (w > 0) {
        nus[((w - 1) * NC) * 64 + lane] = r;
#pragma unroll
        for (int d = 0; d < DT; ++d) nus[((w - 1) * NC + 1 + d) * 64 + lane] = gs[d];
    }
    __syncthreads();
    if (w == 0) {
        for (int ww = 0; ww < 3; ++ww) {
            r += nus[(ww * NC) * 64 + lane];
#pragma unroll
            for (int d = 0; d < DT; ++d) gs[d] += nus[(ww * NC + 1 + d) * 64 + lane];
        }
        stage[lane * NF] = iv ? r : 0.0;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
            stage[lane * NF + 1 + d] = iv ? gs[d] : 0.0;
            stage[lane * NF + 1 + DT + d] = (iv && d < D) ? a.Z[(long)i * D + d] - mq[d] : 0.0;
        }
    }
    __syncthreads();
    const int NR = mmg_nrstat(D), NS = mmg_nstat(D);
    if (tid < (swap ? NR : NS)) {
        double s = 0.0;
        if (tid == 0) {
            for (int l = 0; l < SR_MM_IT; ++l) s += stage[l * NF];
        } else if (tid < 1 + D) {
            const int d = tid - 1;
            for (int l = 0; l < SR_MM_IT; ++l) s = fma(stage[l * NF], stage[l * NF + 1 + DT + d], s);
        } else if (tid < NR) {
            int d, e;
            mmg_tri_of(tid - 1 - D, d, e);
            for (int l = 0; l < SR_MM_IT; ++l)
                s = fma(stage[l * NF] * stage[l * NF + 1 + DT + d], stage[l * NF + 1 + DT + e], s);
        } else {
            const int d = (tid - NR) / D, e = (tid - NR) % D;
            for (int l = 0; l < SR_MM_IT; ++l) s = fma(stage[l * NF + 1 + DT + d], stage[l * NF + 1 + e], s);
        }
        g.part[(((t * n * n + z) * a.nit) + it) * NS + tid] = s;
    }
}

// KG3
__global__ __launch_bounds__(256) void sr_mmg_pairfin_kernel(sr_mmg_args g) {
    constexpr int DM = SR_MAX_D, NRM = 1 + DM + DM * (DM + 1) / 2;
    static_assert(NRM + DM * DM <= 256, "KG2 / KG3: one thread per sum");
    __shared__ double st[NRM + DM * DM], stc[NRM], Ya[DM * DM], Yb[DM * DM], Bm[DM * DM], UA[DM * DM], UB[DM * DM];
    const sr_mm_args& a = g.f;
    const int D = a.D, n = a.n_out, tid = threadIdx.x, p = blockIdx.y, NR = mmg_nrstat(D), NS = mmg_nstat(D);
    const long t = blockIdx.x;
    int oa, ob;
    mm_pair_of(p, n, oa, ob);
    if (tid < NS) {
        const double* pp = g.part + ((t * n * n + oa * n + ob) * a.nit) * NS + tid;
        double s = 0.0;
        for (int it = 0; it < a.nit; ++it) s += pp[(long)it * NS];
        st[tid] = s;
    }
    if (tid < NR) {                                  // the column sums' moments: the pass with the outputs exchanged
        const double* pp = g.part + ((t * n * n + ob * n + oa) * a.nit) * NS + tid;
        double s = 0.0;
        for (int it = 0; it < a.nit; ++it) s += pp[(long)it * NS];
        stc[tid] = s;
    }
    const double* P = a.ws + a.Tq * n * mm_mean_rec(D) + ((a.q0 + t) * a.npairs + p) * mm_pair_rec(D) + 2;
    if (tid < D * D) {
        const int i = tid / D, j = tid % D;
        const double xi = a.ls[oa * D + i], yi = a.ls[ob * D + i], xj = a.ls[oa * D + j], yj = a.ls[ob * D + j];
        const double lai = 1.0 / (xi * xi), lbi = 1.0 / (yi * yi), laj = 1.0 / (xj * xj), lbj = 1.0 / (yj * yj);
        const double ldm = (lai + lbi) * (P[i * D + j] / (lbi * laj));          // (Ld M)_ij,  P = L_b^-1 M L_a^-1
        const double rt = (i == j ? 1.0 : 0.0) - ldm;                           // R^-T = I - Ld M
        Ya[tid] = rt * laj;
        Yb[tid] = rt * lbj;
        Bm[tid] = (i == j ? lai + lbi : 0.0) - ldm * (laj + lbj);               // Ld R^-1 = Ld - Ld M Ld
    }
    __syncthreads();
    if (tid < D * D) {
        const int i = tid / D, j = tid % D;
        double ua = 0.0, ub = 0.0;
        for (int k = 0; k < D; ++k) {
            ua = fma(Ya[i * D + k], st[1 + D + mmg_tri(k, j)], ua);
            ub = fma(2.0 * Ya[i * D + k], st[NR + k * D + j], ub);
            ub = fma(Yb[i * D + k], stc[1 + D + mmg_tri(k, j)], ub);
        }
        UA[tid] = ua;
        UB[tid] = ub;
    }
    __syncthreads();
    const double* cb = g.cov_bar ? g.cov_bar + t * n * n : nullptr;
    const double om = (cb ? 0.5 * (cb[oa * n + ob] + cb[ob * n + oa]) : 0.0) * (oa == ob ? 1.0 : 2.0);
    double* cr = g.contrib + (t * (n + a.npairs) + n + p) * mmg_crec(D);
    if (tid < D * D) {
        const int i = tid / D, j = tid % D;
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            s = fma(UA[i * D + k], Ya[j * D + k], s);
            s = fma(UB[i * D + k], Yb[j * D + k], s);
        }
        cr[D + tid] = om * (0.5 * s - 0.5 * st[0] * Bm[tid]);
    }
    if (tid < D) {
        double s = 0.0;
        for (int k = 0; k < D; ++k) {
            s = fma(Ya[tid * D + k], st[1 + k], s);
            s = fma(Yb[tid * D + k], stc[1 + k], s);
        }
        cr[tid] = om * s;
    }
}

// KG4
__global__ __launch_bounds__(256) void sr_mmg_final_kernel(sr_mmg_args g) {
    const sr_mm_args& a = g.f;
    const int D = a.D, CR = mmg_crec(D), nslot = a.n_out + a.npairs;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= a.T * CR) return;
    const long t = e / CR;
    const int k = (int)(e % CR);
    const double* cr = g.contrib + t * nslot * CR;
    if (k < D) {
        if (!g.m_bar) return;
        double s = 0.0;
        for (int sl = 0; sl < nslot; ++sl) s += cr[sl * CR + k];
        g.m_bar[t * D + k] = s;
    } else {
        if (!g.S_bar) return;
        const int i = (k - D) / D, j = (k - D) % D;
        double s1 = 0.0, s2 = 0.0;
        for (int sl = 0; sl < nslot; ++sl) {
            s1 += cr[sl * CR + D + i * D + j];
            s2 += cr[sl * CR + D + j * D + i];
        }
        g.S_bar[t * D * D + i * D + j] = 0.5 * (s1 + s2);
    }
}

// the seed-independent half: KM0, KM1 (mu and V into the scratch) and KG2 (the tiles' sums into part) over all a.T queries
template <int DT>
static int mmg_launch_records(const sr_mmg_args& g, hipStream_t s) {
    const sr_mm_args& a = g.f;
    const long nprep = a.T * (a.n_out + a.npairs);
    constexpr int BT = mm_prep_bt<DT>::value;
    hipLaunchKernelGGL((sr_mm_prep_kernel<DT>), dim3((unsigned)((nprep + BT - 1) / BT)), dim3(BT), 0, s, a);
    hipLaunchKernelGGL((sr_mm_mean_kernel<DT>), dim3((unsigned)a.T, a.n_out), dim3(256), 0, s, a);
    hipLaunchKernelGGL((sr_mmg_pair_kernel<DT>), dim3((unsigned)a.T, a.nit, a.n_out * a.n_out), dim3(256), 0, s, g);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

// the seed-dependent half: KG1, KG3, KG4 on the a.T queries from a.q0 on (nothing of size N^2)
template <int DT>
static int mmg_launch_seeded(const sr_mmg_args& g, hipStream_t s) {
    const sr_mm_args& a = g.f;
    hipLaunchKernelGGL((sr_mmg_mean_kernel<DT>), dim3((unsigned)a.T, a.n_out), dim3(256), 0, s, g);
    hipLaunchKernelGGL(sr_mmg_pairfin_kernel, dim3((unsigned)a.T, a.npairs), dim3(256), 0, s, g);
    hipLaunchKernelGGL(sr_mmg_final_kernel, dim3((unsigned)((a.T * mmg_crec(a.D) + 255) / 256)), dim3(256), 0, s, g);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

// the arguments of both halves for a block of Tq queries whose scratch is ws (Tq x sr_mmg_ws_per_query doubles:
// [records | mu | V | contribution records | part]); then the slice q0 .. q0 + T of it for the seed-dependent half
static sr_mmg_args mmg_block(const double* Z, const double* alpha, const double* ls, const double* sf2, int N, int Np, int D,
                             int n_out, const double* m, const double* S, long Tq, const double* inv_k, double* ws) {
    sr_mmg_args g;
    sr_mm_args& a = g.f;
    a.Z = Z; a.alpha = alpha; a.ls = ls; a.sf2 = sf2; a.m = m; a.S = S; a.inv_k = inv_k; a.cov = nullptr;
    a.N = N; a.Np = Np; a.D = D; a.n_out = n_out; a.npairs = n_out * (n_out + 1) / 2; a.nit = mm_nit(N);
    a.T = Tq; a.q0 = 0; a.Tq = Tq;
    a.ws = ws;
    a.mu = ws + Tq * mmg_fwd_recs(D, n_out);
    a.V = a.mu + Tq * n_out;
    g.contrib = a.V + Tq * n_out * D;
    g.part = g.contrib + Tq * (n_out + a.npairs) * mmg_crec(D);
    g.mu_bar = g.cov_bar = g.V_bar = nullptr; g.m_bar = g.S_bar = nullptr;
    return g;
}
static void mmg_slice(sr_mmg_args& g, long q0, long T) {
    sr_mm_args& a = g.f;
    const long n = a.n_out, D = a.D;
    a.q0 = q0; a.T = T;
    a.m += q0 * D;
    if (a.S) a.S += q0 * D * D;
    a.mu += q0 * n;
    a.V += q0 * n * D;
    g.contrib += q0 * (n + a.npairs) * mmg_crec(a.D);
    g.part += q0 * n * n * a.nit * mmg_nstat(a.D);
}
static int mmg_check_grid(const char* who, int N, int n_out, long T) {
    SR_CHECK(n_out * n_out < 65536 && mm_nit(N) < 65536 && T <= sr_mmg_max_queries(N, n_out), SR_EUNSUPPORTED,
             "%s: n_out=%d N=%d T=%ld outside the launch grid", who, n_out, N, T);
    return SR_OK;
}

// one chunk of T queries; ws: T x sr_mmg_ws_per_query doubles
int sr_launch_moment_match_vjp(const double* Z, const double* alpha, const double* ls, const double* sf2, int N, int Np,
                               int D, int n_out, const double* m, const double* S, long T, const double* inv_k,
                               const double* mu_bar, const double* cov_bar, const double* V_bar, double* m_bar,
                               double* S_bar, double* ws, hipStream_t s) {
    sr_mmg_args g = mmg_block(Z, alpha, ls, sf2, N, Np, D, n_out, m, S, T, inv_k, ws);
    g.mu_bar = mu_bar; g.cov_bar = cov_bar; g.V_bar = V_bar; g.m_bar = m_bar; g.S_bar = S_bar;
    SR_TRY(mmg_check_grid("moment_match_vjp", N, n_out, T));
    const int rc = sr_pick_le<4, 8, 12>("moment_match_vjp", D, [&](auto dt) { return mmg_launch_records<decltype(dt)::value>(g, s); });
    if (rc != SR_OK) return rc;
    return sr_pick_le<4, 8, 12>("moment_match_vjp", D, [&](auto dt) { return mmg_launch_seeded<decltype(dt)::value>(g, s); });
}

// The two halves on their own (sr_moment_match_rollout_vjp.hip): the records, mu, V and part of Tq queries once, ...
int sr_launch_moment_match_vjp_records(const double* Z, const double* alpha, const double* ls, const double* sf2, int N,
                                       int Np, int D, int n_out, const double* m, const double* S, long Tq,
                                       const double* inv_k, double* ws, hipStream_t s) {
    sr_mmg_args g = mmg_block(Z, alpha, ls, sf2, N, Np, D, n_out, m, S, Tq, inv_k, ws);
    SR_TRY(mmg_check_grid("moment_match_vjp", N, n_out, Tq));
    return sr_pick_le<4, 8, 12>("moment_match_vjp", D, [&](auto dt) { return mmg_launch_records<decltype(dt)::value>(g, s); });
}
// ... then, as often as wanted, the seeds of the queries q0 .. q0 + T (seeds and results are the slice's own arrays, T rows)
int sr_launch_moment_match_vjp_seeded(const double* Z, const double* alpha, const double* ls, const double* sf2, int N,
                                      int Np, int D, int n_out, const double* m, long q0, long T, long Tq,
                                      const double* mu_bar, const double* cov_bar, const double* V_bar, double* m_bar,
                                      double* S_bar, double* ws, hipStream_t s) {
    sr_mmg_args g = mmg_block(Z, alpha, ls, sf2, N, Np, D, n_out, m, nullptr, Tq, nullptr, ws);
    mmg_slice(g, q0, T);
    g.mu_bar = mu_bar; g.cov_bar = cov_bar; g.V_bar = V_bar; g.m_bar = m_bar; g.S_bar = S_bar;
    return sr_pick_le<4, 8, 12>("moment_match_vjp", D, [&](auto dt) { return mmg_launch_seeded<decltype(dt)::value>(g, s); });
}
// where mu (Tq x n_out) and V (Tq x n_out x D) of the records half lie in ws
double* sr_mmg_ws_mu(double* ws, long Tq, int D, int n_out) { return ws + Tq * mmg_fwd_recs(D, n_out); }
double* sr_mmg_ws_v(double* ws, long Tq, int D, int n_out) { return sr_mmg_ws_mu(ws, Tq, D, n_out) + Tq * n_out; }
