// sr_moment_match_rollout.hip -- exact moment matching over a whole horizon in ONE launch (sr_gp_moment_match_rollout; the
// C-ABI: include/safereach.h, the checks: sr_capi_reach.hip, the per-step kernels it stands beside: sr_moment_match.hip KM0 - KM3
// with the torch algebra of uncertainty_propagation_casadi._mm_step between them).
//
//   KMR sr_mm_rollout_kernel<DT, NT> : one workgroup owns one trajectory for all H steps.  Step i + 1 of a trajectory depends on
//                                      its own step i alone, so nothing crosses a workgroup: the only synchronisation is
//                                      __syncthreads(), every loop is bounded by H, N, D, n_out, there are no atomics and no
//                                      result depends on which other trajectories are in flight.
// Per step, with the state N(mu, Sigma) and u = K x + k_ff (K = 0 at step 0), G = [tz; K]:
//   1 the GP input  m_z = G mu + [0; k_ff],  S_z = G Sigma G^T (none from a point), A = a + b K            [state block in LDS]
//   2 KM0's D x D algebra, one thread per output resp. pair of outputs (wave 0: outputs, waves 1 - 3: pairs), its matrices in
//     LDS columns as KM0 keeps them; nothing inverts S_z: every factorisation is of I + D^1/2 S_z D^1/2.  The records
//     [c0, W] and [c, point, P, G_a, G_b] stay in LDS where they fit, else they go to the workgroup's slice of the handle's
//     scratch (sr_mmr_ws_per_traj doubles)
//   3 per output the mean pass of KM1: all threads over the rows i, 1 + D sums per thread -> mu_g, V
//   4 per pair a <= b the double sum of KM2: tiles of SR_MMR_IT = 64 rows i (one per lane, u_i, s_i, alpha_ai in registers)
//     against staged tiles of SR_MMR_JT = 256 rows j (nu_j, s_j, alpha_bj in LDS, read as broadcasts), the NT / 64 wavefronts
//     share the j of a tile, four exp chains in flight per thread; a == b: the j before the i tile are skipped, those behind
//     it count twice (KM2's half-sum trick at the grain of the i tile); Kinv_a is read from global memory as [j][i]
//     (coalesced along the lanes).  A thread adds its i tiles in ascending order, then ONE ordered sum per pair; - mu_a mu_b,
//     + sf2 and the clip on the diagonal; exact zeros off it from a point
//   5 mu+ = A mu + b k_ff + mu_g,  Sigma+ = Hm Sigma Hm^T + Cov - (VG) Sigma (VG)^T with Hm = A + VG (Cov from a point); the
//     upper triangle is computed and mirrored: Sigma+ is stored exactly symmetric
// Ordered sums: a wavefront's 64 values by __shfl_down in a fixed tree, the wavefronts' sums in ascending order by one thread.
// The same inputs give the same bits; the first h steps of a longer roll-out are the h-step roll-out; cov_all is only a store.
// The double sum is added in another order than KM2 / KM3 add it: the results equal those of the per-step route to rounding,
// not bit for bit.
//
// Sizes (profiles/r20_moment_match_rollout.txt: what was tried): NT = 512 threads at DT <= 8 (two wavefronts per SIMD: a
// workgroup is alone on its CU up to T = 256, nothing else hides the latency of its exp chains), 256 at DT = 12 (LDS); tiles
// 64 x 256, those of KM2.  Z and alpha are copied into LDS once per launch where they fit beside the tiles (N (D + n_out)
// doubles; 10.5 KB in the cart-pole regime), else they are re-read through the caches every step; the trajectory's state
// never leaves LDS.  No private array is indexed dynamically, no instance uses scratch memory
// (profiles/r20_moment_match_rollout_resources.txt).
#include "sr_common.h"

#define SR_MMR_IT 64          // rows i per tile (one per lane)
#define SR_MMR_JT 256         // rows j per staged tile
template <int DT> struct mmr_nt { static constexpr int value = DT <= 8 ? 512 : 256; };     // threads per workgroup

__host__ __device__ static inline long mmr_mean_rec(int D) { return 1 + (long)D * D; }       // [c0, W (D x D)]
__host__ __device__ static inline long mmr_pair_rec(int D) { return 2 + 3 * (long)D * D; }   // [c, point, P, G_a, G_b]

long sr_mmr_ws_per_traj(int D, int n_out) {
    const long npairs = (long)n_out * (n_out + 1) / 2;
    return n_out * mmr_mean_rec(D) + npairs * mmr_pair_rec(D);
}

// the state block of a trajectory (dynamic LDS), in doubles: mu, mu_g, the new mean (n each); Sigma, A, VG, Hm, Cov, two
// temporaries, the new Sigma (n x n each); G, G Sigma, V (D x n each); S_z (D x D); k_ff (n_u < D)
__host__ __device__ static inline int mmr_state_doubles(int n, int D) {
    return 3 * n + 8 * n * n + 3 * D * n + D * D + D;
}

// p-th pair (a <= b) in row-major order of the upper triangle
__device__ static inline void mmr_pair_of(int p, int n, int& a, int& b) {
    a = 0;
    while (p >= n - a) { p -= n - a; ++a; }
    b = a + p;
}

// columns of the D x D algebra held in LDS at one time (a quarter of them per wavefront)
template <int DT> struct mmr_bt { static constexpr int value = DT <= 8 ? 16 : 8; };

// the algebra's matrices in LDS, element-major with the column of the thread innermost (no bank conflicts, and no dynamically
// indexed private array)
#define RM(M, i, j) M[((i) * DT + (j)) * BT + col]
#define RV(v, d) v[(d) * BT + col]

// lower Cholesky factor in place (lower triangle read and written); returns log det
template <int DT, int BT>
__device__ static inline double mmr_chol(double* C, int D, int col) {
    double logdet = 0.0;
    for (int k = 0; k < D; ++k) {
        double s = RM(C, k, k);
        for (int p = 0; p < k; ++p) s -= RM(C, k, p) * RM(C, k, p);
        logdet += log(s);
        const double l = sqrt(s), inv = 1.0 / l;
        RM(C, k, k) = l;
        for (int i = k + 1; i < D; ++i) {
            double v = RM(C, i, k);
            for (int p = 0; p < k; ++p) v -= RM(C, i, p) * RM(C, k, p);
            RM(C, i, k) = v * inv;
        }
    }
    return logdet;
}

// the record of output o (KM0's first half): C = I + L^-1/2 S L^-1/2 = Lc Lc^T, (S + L)^-1 = W^T W with W = Lc^-1 L^-1/2
template <int DT, int BT>
__device__ static inline void mmr_prep_mean(double* C, double* X, double* r, const double* ls, double sf2, const double* S,
                                            int D, int col, double* rec) {
    for (int d = 0; d < D; ++d) RV(r, d) = 1.0 / ls[d];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) RM(C, i, j) = (i == j ? 1.0 : 0.0) + (S ? RV(r, i) * RV(r, j) * S[i * D + j] : 0.0);
    const double logdet = mmr_chol<DT, BT>(C, D, col);
    for (int j = 0; j < D; ++j) {              // X = Lc^-1 (lower), column by column
        RM(X, j, j) = 1.0 / RM(C, j, j);
        for (int i = j + 1; i < D; ++i) {
            double v = 0.0;
            for (int p = j; p < i; ++p) v -= RM(C, i, p) * RM(X, p, j);
            RM(X, i, j) = v / RM(C, i, i);
        }
    }
    rec[0] = log(sf2) - 0.5 * logdet;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) rec[1 + i * D + j] = j <= i ? RM(X, i, j) * RV(r, j) : 0.0;
}

// the record of the pair (oa, ob) (KM0's second half): Ld = L_a^-1 + L_b^-1, C = I + Ld^1/2 S Ld^1/2 = Lc Lc^T, |R| = |C|,
// M = Ld^-1/2 (C^-1 (C - I)) Ld^-1/2
template <int DT, int BT>
__device__ static inline void mmr_prep_pair(double* C, double* X, double* r, double* la, double* lb, const double* lsa,
                                            const double* lsb, double sf2ab, const double* S, int D, int col, double* rec) {
    bool point = true;
    for (int d = 0; d < D; ++d) {
        const double x = lsa[d], y = lsb[d];
        RV(la, d) = 1.0 / (x * x);
        RV(lb, d) = 1.0 / (y * y);
        RV(r, d) = sqrt(RV(la, d) + RV(lb, d));
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j <= i; ++j) {
            const double sij = S ? S[i * D + j] : 0.0;
            if (sij != 0.0) point = false;
            const double bij = RV(r, i) * RV(r, j) * sij;
            RM(C, i, j) = (i == j ? 1.0 : 0.0) + bij;
            RM(X, i, j) = bij;
            RM(X, j, i) = bij;
        }
    const double logdet = mmr_chol<DT, BT>(C, D, col);
    for (int j = 0; j < D; ++j) {              // X[:, j] <- C^-1 X[:, j]
        for (int i = 0; i < D; ++i) {
            double v = RM(X, i, j);
            for (int p = 0; p < i; ++p) v -= RM(C, i, p) * RM(X, p, j);
            RM(X, i, j) = v / RM(C, i, i);
        }
        for (int i = D - 1; i >= 0; --i) {
            double v = RM(X, i, j);
            for (int p = i + 1; p < D; ++p) v -= RM(C, p, i) * RM(X, p, j);
            RM(X, i, j) = v / RM(C, i, i);
        }
    }
    rec[0] = log(sf2ab) - 0.5 * logdet;
    rec[1] = point ? 1.0 : 0.0;
    double *P = rec + 2, *Ga = P + D * D, *Gb = Ga + D * D;
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            const double mij = 0.5 * (RM(X, i, j) + RM(X, j, i)) / (RV(r, i) * RV(r, j));
            P[i * D + j] = RV(lb, i) * mij * RV(la, j);
            Ga[i * D + j] = (i == j ? RV(la, i) : 0.0) - RV(la, i) * mij * RV(la, j);
            Gb[i * D + j] = (i == j ? RV(lb, i) : 0.0) - RV(lb, i) * mij * RV(lb, j);
        }
}
#undef RM
#undef RV

// D x D record -> DT x DT in LDS (zero padding), all threads
template <int DT, int NT>
__device__ static inline void mmr_load_mat(double* dst, const double* src, int D) {
    for (int e = threadIdx.x; e < DT * DT; e += NT) {
        const int i = e / DT, j = e % DT;
        dst[e] = (i < D && j < D) ? src[i * D + j] : 0.0;
    }
}

// the 64 values of a wavefront in a fixed tree; lane 0 holds the sum
__device__ static inline double mmr_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}

// KMR
template <int DT, int NT>
__global__ __launch_bounds__(NT) void sr_mm_rollout_kernel(sr_mmr_args a) {
    constexpr int IT = SR_MMR_IT, JT = SR_MMR_JT, NW = NT / 64, BT = mmr_bt<DT>::value, CW = BT / 4;
    constexpr int NROW = NT > JT ? NT : JT;                    // a slot of DT doubles per thread and per staged row
    constexpr int NPREP = (2 * DT * DT + 3 * DT) * BT;
    constexpr int NBUF = NROW * DT > NPREP ? NROW * DT : NPREP;
    static_assert(NT % 64 == 0 && NT >= JT && JT % IT == 0 && BT % 4 == 0, "KMR: whole wavefronts, one staged row per thread");
    __shared__ double buf[NBUF];                               // step 2: the algebra's columns; steps 3 - 4: the staged j tile
    __shared__ double sjs[JT], ajs[JT];
    __shared__ double P[DT * DT], Ga[DT * DT], Gb[DT * DT], mq[DT];      // (P is W in the mean pass)
    __shared__ double part[NW * (DT + 1)], gsum[DT + 1];
    extern __shared__ double st[];
    const int D = a.D, N = a.N, n = a.n_out, nx = a.n_x_in, n_u = D - nx, H = a.H, off = a.Np - N;
    const int npairs = n * (n + 1) / 2, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long t = blockIdx.x;
    double* mu = st;                    // n
    double* Sig = mu + n;               // n x n
    double* Gm = Sig + n * n;           // D x n
    double* Sz = Gm + D * n;            // D x D
    double* GS = Sz + D * D;            // D x n
    double* Am = GS + D * n;            // n x n
    double* mug = Am + n * n;           // n
    double* Vm = mug + n;               // n x D
    double* VG = Vm + n * D;            // n x n
    double* Hm = VG + n * n;            // n x n
    double* Cov = Hm + n * n;           // n x n
    double* T1 = Cov + n * n;           // n x n
    double* T2 = T1 + n * n;            // n x n
    double* Sn = T2 + n * n;            // n x n
    double* mun = Sn + n * n;           // n
    double* kf = mun + n;               // n_u < D  (mmr_state_doubles in all)
    // behind the state block, where the host found room (sr_launch_moment_match_rollout): the step's records, else they go
    // to the workgroup's slice of the scratch; then Z and alpha, else they are re-read through the caches
    const long per = n * mmr_mean_rec(D) + npairs * mmr_pair_rec(D);
    double* extra = st + mmr_state_doubles(n, D);
    double* rec_m = a.stage_rec ? extra : a.ws + t * per;
    double* rec_p = rec_m + n * mmr_mean_rec(D);
    const double* Zs = a.Z;
    const double* al0 = a.alpha + off;
    long als = a.Np;
    if (a.stage_model) {
        double* zl = extra + (a.stage_rec ? per : 0);
        double* all = zl + N * D;
        for (int e = tid; e < N * D; e += NT) zl[e] = a.Z[e];
        for (int e = tid; e < n * N; e += NT) all[e] = a.alpha[(long)(e / N) * a.Np + off + e % N];
        Zs = zl;
        al0 = all;
        als = N;
    }
    const double* kff_t = a.k_ff + (a.gains_per_traj ? t * H * n_u : 0);
    const double* kfb_t = a.k_fb ? a.k_fb + (a.gains_per_traj ? t * (long)(H - 1) * n_u * n : 0) : nullptr;
    const int nit = (N + IT - 1) / IT, njt = (N + JT - 1) / JT;

    for (int e = tid; e < n; e += NT) mu[e] = a.mu0[t * n + e];
    if (a.sigma0)
        for (int e = tid; e < n * n; e += NT) Sig[e] = a.sigma0[t * n * n + e];
    bool has_sig = a.sigma0 != nullptr;
    __syncthreads();

    for (int step = 0; step < H; ++step) {
        // ---- 1: G, A, k_ff; then m_z and G Sigma; then S_z
        const double* K = step > 0 ? kfb_t + (long)(step - 1) * n_u * n : nullptr;
        for (int e = tid; e < D * n; e += NT) {
            const int r = e / n, c = e % n;
            Gm[e] = r < nx ? (a.tz ? a.tz[r * n + c] : (r == c ? 1.0 : 0.0)) : (K ? K[(r - nx) * n + c] : 0.0);
        }
        for (int e = tid; e < n * n; e += NT) {
            const int r = e / n, c = e % n;
            double s = a.a[e];
            if (K)
                for (int q = 0; q < n_u; ++q) s = fma(a.b[r * n_u + q], K[q * n + c], s);
            Am[e] = s;
        }
        for (int e = tid; e < n_u; e += NT) kf[e] = kff_t[(long)step * n_u + e];
        __syncthreads();
        if (tid < DT) {
            double s = 0.0;
            if (tid < D) {
                for (int c = 0; c < n; ++c) s = fma(Gm[tid * n + c], mu[c], s);
                if (tid >= nx) s += kf[tid - nx];
            }
            mq[tid] = s;
        }
        if (has_sig)
            for (int e = tid; e < D * n; e += NT) {
                const int r = e / n, c = e % n;
                double s = 0.0;
                for (int k = 0; k < n; ++k) s = fma(Gm[r * n + k], Sig[k * n + c], s);
                GS[e] = s;
            }
        __syncthreads();
        if (has_sig)
            for (int e = tid; e < D * D; e += NT) {
                const int r = e / D, c = e % D;
                if (c > r) continue;
                double s = 0.0;
                for (int k = 0; k < n; ++k) s = fma(GS[r * n + k], Gm[c * n + k], s);
                Sz[r * D + c] = s;
                Sz[c * D + r] = s;
            }
        __syncthreads();

        // ---- 2: the D x D algebra of every output (wavefront 0) and pair (wavefronts 1 - 3), CW columns each
        if (w < 4 && lane < CW) {
            const int col = w * CW + lane;
            double *C = buf, *X = C + DT * DT * BT, *r = X + DT * DT * BT, *la = r + DT * BT, *lb = la + DT * BT;
            const double* S = has_sig ? Sz : nullptr;
            if (w == 0) {
                for (int o = lane; o < n; o += CW)
                    mmr_prep_mean<DT, BT>(C, X, r, a.ls + o * D, a.sf2[o], S, D, col, rec_m + o * mmr_mean_rec(D));
            } else {
                for (int p = (w - 1) * CW + lane; p < npairs; p += 3 * CW) {
                    int oa, ob;
                    mmr_pair_of(p, n, oa, ob);
                    mmr_prep_pair<DT, BT>(C, X, r, la, lb, a.ls + oa * D, a.ls + ob * D, a.sf2[oa] * a.sf2[ob], S, D, col,
                                          rec_p + p * mmr_pair_rec(D));
                }
            }
        }
        __syncthreads();

        // ---- 3: mu_g and V of every output (KM1)
        for (int o = 0; o < n; ++o) {
            const double* rec = rec_m + o * mmr_mean_rec(D);
            const double c0 = rec[0];
            mmr_load_mat<DT, NT>(P, rec + 1, D);
            __syncthreads();
            double acc[DT + 1];
#pragma unroll
            for (int k = 0; k <= DT; ++k) acc[k] = 0.0;
            const double* al = al0 + (long)o * als;
            for (int i = tid; i < N; i += NT) {
                double nu[DT];
#pragma unroll
                for (int d = 0; d < DT; ++d) nu[d] = d < D ? Zs[(long)i * D + d] - mq[d] : 0.0;
                double e = 0.0;
#pragma unroll 1                                  // (unrolled, the whole of W is kept in registers)
                for (int r = 0; r < D; ++r) {
                    double y = 0.0;
#pragma unroll
                    for (int c = 0; c < DT; ++c) y = fma(P[r * DT + c], nu[c], y);      // (zero above the diagonal)
                    e = fma(y, y, e);
                }
                const double q = al[i] * exp(c0 - 0.5 * e);
                acc[0] += q;
#pragma unroll
                for (int d = 0; d < DT; ++d) acc[1 + d] = fma(q, nu[d], acc[1 + d]);
            }
#pragma unroll
            for (int k = 0; k <= DT; ++k) {
                const double v = mmr_wave_sum(acc[k]);
                if (lane == 0) part[w * (DT + 1) + k] = v;
            }
            __syncthreads();
            if (tid <= DT) {
                double s = 0.0;
                for (int ww = 0; ww < NW; ++ww) s += part[ww * (DT + 1) + tid];
                gsum[tid] = s;
            }
            __syncthreads();
            if (tid == 0) mug[o] = gsum[0];
            if (tid < D) {
                // V = W^T (W g), g = sum_i alpha_i q_i nu_i
                double v = 0.0;
                for (int r = 0; r < D; ++r) {
                    double y = 0.0;
                    for (int c = 0; c <= r; ++c) y = fma(P[r * DT + c], gsum[1 + c], y);
                    v = fma(P[r * DT + tid], y, v);
                }
                Vm[o * D + tid] = v;
            }
            __syncthreads();
        }

        // ---- 4: Cov, pair by pair (KM2 with the i tiles in a loop, KM3)
        for (int p = 0; p < npairs; ++p) {
            int oa, ob;
            mmr_pair_of(p, n, oa, ob);
            const bool diag = oa == ob;
            const double* rec = rec_p + p * mmr_pair_rec(D);
            const double c = rec[0];
            if (!diag && rec[1] != 0.0) {             // a point input: the outputs are independent (uniform in the workgroup)
                if (tid == 0) Cov[oa * n + ob] = Cov[ob * n + oa] = 0.0;
                continue;
            }
            mmr_load_mat<DT, NT>(P, rec + 2, D);
            mmr_load_mat<DT, NT>(Ga, rec + 2 + D * D, D);
            mmr_load_mat<DT, NT>(Gb, rec + 2 + 2 * D * D, D);
            __syncthreads();
            const double* kinv = a.inv_k + (size_t)oa * N * N;
            const double* ala = al0 + (long)oa * als;
            const double* alb = al0 + (long)ob * als;
            double* nus = buf;
            double accp = 0.0;
            for (int it = 0; it < nit; ++it) {
                const int i = it * IT + lane;
                const bool iv = i < N;
                double u[DT], si, ai;
                {
                    double nu[DT];
#pragma unroll
                    for (int d = 0; d < DT; ++d) nu[d] = (iv && d < D) ? Zs[(long)i * D + d] - mq[d] : 0.0;
#pragma unroll
                    for (int d = 0; d < DT; ++d) { nus[tid * DT + d] = nu[d]; u[d] = 0.0; }      // (the thread's own slot: no barrier)
                    double qf = 0.0;
#pragma unroll 1                                  // (unrolled, P and G_a pass through the registers at once)
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
                    ai = iv ? ala[i] : 0.0;
                }
                // a == b: Q and the weight are symmetric in (i, j), so the j before the i tile are skipped and those behind
                // it count twice
                const int jt0 = diag ? it / (JT / IT) : 0, ic = iv ? i : 0;
                double acc = 0.0;
                for (int jt = jt0; jt < njt; ++jt) {
                    const int jbase = jt * JT;
                    if (tid < JT) {
                        const int j = jbase + tid;
                        const bool jv = j < N;
                        double nu[DT];
#pragma unroll
                        for (int d = 0; d < DT; ++d) nu[d] = (jv && d < D) ? Zs[(long)j * D + d] - mq[d] : 0.0;
#pragma unroll
                        for (int d = 0; d < DT; ++d) nus[tid * DT + d] = nu[d];
                        double qf = 0.0;
#pragma unroll 1
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
                    const int cnt = min(JT, N - jbase);
                    const int jlo = diag ? max(it * IT - jbase, 0) : 0, j2 = (it + 1) * IT - jbase;
                    double tacc = 0.0;
#pragma unroll 4                                  // (four exp chains in flight: a workgroup is one wavefront per SIMD or two)
                    for (int jj = jlo + w; jj < cnt; jj += NW) {
                        double e = si + sjs[jj];
#pragma unroll
                        for (int d = 0; d < DT; ++d) e = fma(u[d], nus[jj * DT + d], e);
                        double wv = ai * ajs[jj];
                        if (diag) {                    // (rows past N read row 0 and are dropped below)
                            wv -= kinv[(size_t)(jbase + jj) * N + ic];
                            if (jj >= j2) wv += wv;
                        }
                        tacc = fma(wv, exp(e), tacc);
                    }
                    acc += tacc;
                    __syncthreads();
                }
                accp += iv ? acc : 0.0;
            }
            const double ws_ = mmr_wave_sum(accp);
            if (lane == 0) part[w] = ws_;
            __syncthreads();
            if (tid == 0) {
                double s = 0.0;
                for (int ww = 0; ww < NW; ++ww) s += part[ww];
                double v = s - mug[oa] * mug[ob];
                if (diag) {
                    v += a.sf2[oa];
                    Cov[oa * n + oa] = v > SR_VAR_CLIP ? v : SR_VAR_CLIP;
                } else {
                    Cov[oa * n + ob] = v;
                    Cov[ob * n + oa] = v;
                }
            }
        }
        __syncthreads();

        // ---- 5: the state's step
        for (int e = tid; e < n * n; e += NT) {
            const int r = e / n, c = e % n;
            double s = 0.0;
            for (int d = 0; d < D; ++d) s = fma(Vm[r * D + d], Gm[d * n + c], s);
            VG[e] = s;
            Hm[e] = Am[e] + s;
        }
        for (int e = tid; e < n; e += NT) {
            double s = 0.0, bk = 0.0;
            for (int c = 0; c < n; ++c) s = fma(Am[e * n + c], mu[c], s);
            for (int q = 0; q < n_u; ++q) bk = fma(a.b[e * n_u + q], kf[q], bk);
            mun[e] = s + bk + mug[e];
        }
        __syncthreads();
        if (has_sig)
            for (int e = tid; e < n * n; e += NT) {
                const int r = e / n, c = e % n;
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < n; ++k) {
                    s1 = fma(Hm[r * n + k], Sig[k * n + c], s1);
                    s2 = fma(VG[r * n + k], Sig[k * n + c], s2);
                }
                T1[e] = s1;
                T2[e] = s2;
            }
        __syncthreads();
        for (int e = tid; e < n * n; e += NT) {
            const int r = e / n, c = e % n;
            if (c < r) continue;
            double v = Cov[e];
            if (has_sig) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < n; ++k) {
                    s1 = fma(T1[r * n + k], Hm[c * n + k], s1);
                    s2 = fma(T2[r * n + k], VG[c * n + k], s2);
                }
                v = s1 + v - s2;
            }
            Sn[r * n + c] = v;
            Sn[c * n + r] = v;
        }
        __syncthreads();
        const long orow = t * H + step;
        for (int e = tid; e < n; e += NT) {
            mu[e] = mun[e];
            a.mu_all[orow * n + e] = mun[e];
        }
        for (int e = tid; e < n * n; e += NT) {
            Sig[e] = Sn[e];
            a.sigma_all[orow * n * n + e] = Sn[e];
            if (a.cov_all) a.cov_all[orow * n * n + e] = Cov[e];
        }
        has_sig = true;
        __syncthreads();
    }
}

// one launch of T <= 2^31 - 1 trajectories; ws: T x sr_mmr_ws_per_traj doubles.  The dynamic LDS of a workgroup, up to what the
// instance's static LDS leaves of 64 KB: the state block (a must), then the step's records, then Z and alpha.
int sr_launch_moment_match_rollout(const sr_mmr_args& a0, hipStream_t s) {
    sr_mmr_args a = a0;
    SR_CHECK(a.T >= 1 && a.T <= 0x7fffffffL, SR_EINVAL, "moment_match_rollout: T=%ld", a.T);
    const long nt_lab = sr_lab_env("SR_MMR_NT", 0);      // (lab build: 256 at every width)
    return sr_pick_le<4, 8, 12>("moment_match_rollout (use the per-step route)", a.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value, NT = mmr_nt<DT>::value;
        auto go = [&](auto kernel, int nt) {
            hipFuncAttributes fa;
            SR_HIP(hipFuncGetAttributes(&fa, (const void*)kernel));
            const long room = (65536 - (long)fa.sharedSizeBytes) / (long)sizeof(double);
            long dyn = mmr_state_doubles(a.n_out, a.D);
            SR_CHECK(dyn <= room, SR_EUNSUPPORTED,
                     "moment_match_rollout: the state block of n_out=%d, D=%d does not fit the workgroup's LDS: use the "
                     "per-step route", a.n_out, a.D);
            const long rec = sr_mmr_ws_per_traj(a.D, a.n_out), mdl = (long)a.N * a.D + (long)a.n_out * a.N;
            a.stage_rec = dyn + rec <= room;
            if (a.stage_rec) dyn += rec;
            a.stage_model = dyn + mdl <= room;
            if (a.stage_model) dyn += mdl;
            return sr_launch(kernel, dim3((unsigned)a.T), dim3(nt), sizeof(double) * (size_t)dyn, s, a);
        };
#ifdef SR_LAB
        if (nt_lab == 256) return go(sr_mm_rollout_kernel<DT, 256>, 256);
#endif
        (void)nt_lab;
        return go(sr_mm_rollout_kernel<DT, NT>, NT);
    });
}
