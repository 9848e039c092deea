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
    a.T = T;
    SR_CHECK(a.npairs < 65536 && a.nit < 65536 && T <= sr_mm_max_queries(N, n_out), SR_EUNSUPPORTED,
             "moment_match: n_out=%d N=%d T=%ld outside the launch grid", n_out, N, T);
    return sr_pick_le<4, 8, 12>("moment_match", D, [&](auto dt) { return mm_launch<decltype(dt)::value>(a, s); });
}
