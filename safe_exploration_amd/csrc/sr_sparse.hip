// sr_sparse.hip -- sparse GP regression (DTC / VarDTC predictive; GPy's SparseGPRegression posterior as the reference keeps
// it: woodbury_vector and woodbury_inv, ssm_gpy/gaussian_process.py:204, 224-243, 397-400): sr_gp_fit_sparse.
//
// The handle holds the m inducing inputs Z_u (its "training rows"), the kernel and s2 = the likelihood variance (its noise).
//   streamed over the N data rows, in chunks:   G_d = K_uf K_fu (upper block triangle),  b_d = K_uf y_d
//   on m x m:   Sigma = K_uu + G / s2 ;  beta = Sigma^-1 b / s2 ;  M = K_uu^-1 - Sigma^-1 = P P^T, P upper triangular
//   -> alpha = beta, Wt = P: every posterior consumer evaluates mu = k_u^T beta, var = k** - |P^T k_u|^2 as for an exact model.
// The streamed product is the fp64 MFMA tile (sr_launch_gemm_tn_upper, accumulating); its operand is the chunk's
// cross-covariance panel K_fu, k-major with the inducing index contiguous: the TRANSPOSE of what sr_kstar_kernel writes,
// hence a kernel of its own below (both kernel families), which also leaves the chunk's share of b.
// The three factorisations (K_uu, Sigma, J M J) are the chain of launches of sr_gp_factorize on given matrices
// (srh::factorize_matrix).  P = J L J with J M J = L L^T: the factor is taken from the last row upwards.
// Order of every sum: chunks in ascending order, inside a chunk the GEMM's k order and the strips of SR_SP_ROWS rows in
// ascending order -- two fits of the same data with the same chunk are bit-identical.
#include "sr_handle.h"
#include "sr_kernel_dev.h"
using namespace srh;

#define SR_SP_ROWS 32            // data rows per workgroup of the panel kernel (one partial sum of b per strip and column)
#define SR_SP_MAX_ROWS 16384     // data rows per chunk at most (the panel: n_out x rows x Np doubles)

// ------------------------------------------------------------------------------------------------
// P_d[r][j] = k_d(x_{row0 + r}, z_{j - off}) for the rows of one chunk (r < rows; the rows behind them up to the padded
// count and the off front columns are zero), bpart[strip][d][j] = sum over the strip's rows of P_d[r][j] y_d[row0 + r].
// Thread = one column, SR_SP_ROWS rows; the strip's inputs (ARD-RBF: scaled) in LDS.  The entries take the form the Gram
// kernels give them (sr_gram_kernel / sr_gram_general_kernel): a data row that IS an inducing row reproduces K_uu's entry.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_sp_panel_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                          long row0, int rows, const double* __restrict__ Z,
                                                          const double* __restrict__ ls, const double* __restrict__ sf2,
                                                          const double* __restrict__ kp, double* __restrict__ P,
                                                          long sP, double* __restrict__ bpart, int N, int Np, int D,
                                                          int n_out) {
    __shared__ double xs[SR_SP_ROWS][SR_MAX_D];
    __shared__ double ys[SR_SP_ROWS];
    const int d = blockIdx.z;
    const int r0 = blockIdx.y * SR_SP_ROWS;
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int off = Np - N;
    const bool real = j < Np && j >= off;
    double sc[SR_MAX_D], zj[SR_MAX_D];
    if (kp) {
        const sr_kview k(kp + (long)d * SR_KP(D), D);
        for (int c = 0; c < D; ++c) { sc[c] = k.sv[c]; zj[c] = real ? Z[(long)(j - off) * D + c] : 0.0; }
    } else {
        for (int c = 0; c < D; ++c) {
            sc[c] = 1.0 / ls[(long)d * D + c];
            zj[c] = real ? Z[(long)(j - off) * D + c] * sc[c] : 0.0;
        }
    }
    for (int e = threadIdx.x; e < SR_SP_ROWS * D; e += 256) {
        const int r = e / D, c = e % D;
        double v = (r0 + r < rows) ? X[(row0 + r0 + r) * D + c] : 0.0;
        if (!kp) v *= 1.0 / ls[(long)d * D + c];
        xs[r][c] = v;
    }
    if (threadIdx.x < SR_SP_ROWS)
        ys[threadIdx.x] = (r0 + threadIdx.x < rows) ? Y[(row0 + r0 + threadIdx.x) * n_out + d] : 0.0;
    __syncthreads();
    if (j >= Np) return;
    double* Pd = P + (long)d * sP + (long)r0 * Np + j;
    double acc = 0.0;
    if (kp) {
        const sr_kview k(kp + (long)d * SR_KP(D), D, sc);    // (s[D]: the thread's copy)
        for (int u = 0; u < SR_SP_ROWS; ++u) {
            double v = 0.0;
            if (real && r0 + u < rows) v = sr_kpair(k, D, xs[u], zj);
            Pd[(long)u * Np] = v;
            acc = fma(v, ys[u], acc);
        }
    } else {
        const double f = sf2[d];
        for (int u = 0; u < SR_SP_ROWS; ++u) {
            double v = 0.0;
            if (real && r0 + u < rows) {
                double r2 = 0.0;
                for (int c = 0; c < D; ++c) {
                    const double t = xs[u][c] - zj[c];
                    r2 = fma(t, t, r2);
                }
                v = f * exp(-0.5 * r2);
            }
            Pd[(long)u * Np] = v;
            acc = fma(v, ys[u], acc);
        }
    }
    bpart[((long)blockIdx.y * n_out + d) * Np + j] = acc;
}

// b[d][j] += the strips' partial sums of one chunk, in ascending order
__global__ __launch_bounds__(256) void sr_sp_bsum_kernel(const double* __restrict__ bpart, int strips, double* __restrict__ b,
                                                         long n) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double t = 0.0;
    for (int s = 0; s < strips; ++s) t += bpart[(long)s * n + e];
    b[e] += t;
}

// Sigma = K_uu + G / s2 on the upper block triangle (what the factorisation reads), in place of G; identity on the padding
// (K_uu carries it, G is zero there).  rhs = b / s2.
__global__ __launch_bounds__(256) void sr_sp_sigma_kernel(double* __restrict__ G, const double* __restrict__ Kuu,
                                                          const double* __restrict__ s2, double* __restrict__ b, int Np) {
    const int d = blockIdx.z, i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Np) return;
    const double inv = 1.0 / s2[d];
    if (i == 0) b[(long)d * Np + j] *= inv;
    if ((j | (SR_NB - 1)) < i) return;
    const long e = ((long)d * Np + i) * Np + j;
    G[e] = Kuu[e] + G[e] * inv;
}

// dst[i][j] = src[Np-1-j][Np-1-i] (the transpose about the anti-diagonal: J A^T J) in 32 x 32 tiles through LDS.
//   mode 0: src = srcO, the tiles of dst's upper block triangle; where the source index lies on the padding (< off) dst gets
//           the identity -- R = J M J of a symmetric M given by its upper block triangle.
//   mode 1: src = srcD inside the diagonal 128-blocks and srcO elsewhere (the Cholesky factor as the update leaves it: diagonal
//           blocks in U, block rows in W); only i <= j is written -- Wt = J U^T J, its strict lower triangle stays zero.
__global__ __launch_bounds__(256) void sr_sp_antitranspose_kernel(const double* __restrict__ srcD,
                                                                  const double* __restrict__ srcO, double* __restrict__ dst,
                                                                  int Np, int off, int mode, long sS, long sD) {
    __shared__ double t[32][33];
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    if ((j0 | (SR_NB - 1)) < i0) return;
    if (mode == 1 && j0 + 31 < i0) return;
    srcD += (long)blockIdx.z * sS; srcO += (long)blockIdx.z * sS; dst += (long)blockIdx.z * sD;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    // source tile: rows Np-1-j0-b (b = 0 .. 31), columns Np-1-i0-a (a = 0 .. 31)
    for (int bq = ty; bq < 32; bq += 8) {
        const int r = Np - 1 - j0 - bq, c = Np - 1 - i0 - tx;
        double v;
        if (mode == 0) v = (r < off || c < off) ? ((r == c) ? 1.0 : 0.0) : srcO[(long)r * Np + c];
        else v = (r / SR_NB == c / SR_NB) ? srcD[(long)r * Np + c] : srcO[(long)r * Np + c];
        t[bq][tx] = v;                                        // t[b][a]
    }
    __syncthreads();
    for (int a = ty; a < 32; a += 8) {
        const int i = i0 + a, j = j0 + tx;
        if (mode == 1 && i > j) continue;
        dst[(long)i * Np + j] = t[tx][a];
    }
}

int sr_launch_reversed_factor(const double* U, const double* W, double* Wt, int Np, hipStream_t s, int nbatch, long sS,
                              long sD) {
    hipLaunchKernelGGL(sr_sp_antitranspose_kernel, dim3(Np / 32, Np / 32, nbatch), dim3(256), 0, s, U, W, Wt, Np, 0, 1, sS, sD);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

// A pivot that is positive only by rounding is a breakdown too (two identical inducing rows leave +-1e-16 k(z, z)): the first
// real row i whose pivot 1 / Wt[i][i]^2 is not above Np eps max_i A[i][i] goes to info[d] (1-based padded index), unless the
// factorisation has already named one.  One workgroup per output.
__global__ __launch_bounds__(256) void sr_sp_pivot_check_kernel(const double* __restrict__ Wt, const double* __restrict__ A,
                                                                int Np, int off, int* __restrict__ info) {
    __shared__ unsigned long long amax;
    __shared__ int first;
    const int d = blockIdx.x;
    Wt += (long)d * Np * Np; A += (long)d * Np * Np;
    if (threadIdx.x == 0) { amax = 0ull; first = Np + 1; }
    __syncthreads();
    double mx = 0.0;
    for (int i = off + threadIdx.x; i < Np; i += 256) mx = fmax(mx, fabs(A[(long)i * Np + i]));
    atomicMax(&amax, (unsigned long long)__double_as_longlong(mx));       // (non-negative doubles order as their bits)
    __syncthreads();
    const double tol = (double)Np * 2.220446049250313e-16 * __longlong_as_double((long long)amax);
    for (int i = off + threadIdx.x; i < Np; i += 256) {
        const double w = Wt[(long)i * Np + i];
        if (!(1.0 / (w * w) > tol)) atomicMin(&first, i + 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && first <= Np && info[d] == 0) info[d] = first;
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
extern "C" int sr_gp_is_sparse(sr_gp_t h) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_is_sparse: NULL handle");
    return (h->factorized && h->sparse) ? 1 : 0;
}

namespace {
struct sp_ws {
    double *G = nullptr, *Km = nullptr, *T = nullptr, *panel = nullptr, *bpart = nullptr, *b = nullptr;
    int* info = nullptr;
    ~sp_ws() { dev_free(G); dev_free(Km); dev_free(T); dev_free(panel); dev_free(bpart); dev_free(b); dev_free(info); }
};
}  // namespace

static int fit_sparse(sr_gp* h, const double* X, const double* Y, long N, double jitter, void* stream, int* info);

extern "C" int sr_gp_fit_sparse(sr_gp_t h, const double* X, const double* Y, long N, double jitter, void* stream,
                                int* info) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_fit_sparse: NULL handle");
    SR_CHECK(X && Y, SR_EINVAL, "sr_gp_fit_sparse: NULL data");
    SR_CHECK(jitter >= 0.0, SR_EINVAL, "sr_gp_fit_sparse: jitter %g < 0", jitter);
    SR_CHECK(h->have_data, SR_ESTATE, "sr_gp_fit_sparse: call sr_gp_set_data first (inducing inputs, kernel, likelihood variance)");
    SR_CHECK(N >= h->N, SR_EINVAL, "sr_gp_fit_sparse: %ld data rows for %d inducing inputs", N, h->N);
    SR_DEVICE(h->device);
    h->sparse = 0;
    const int rc = fit_sparse(h, X, Y, N, jitter, stream, info);
    if (rc != SR_OK) h->factorized = 0;                  // (the passes of the factorisation mark the handle one by one)
    else h->sparse = 1;
    return rc;
}

static int fit_sparse(sr_gp* h, const double* X, const double* Y, long N, double jitter, void* stream, int* info) {
    hipStream_t s = (hipStream_t)stream;
    const int m = h->N, Np = h->Np, D = h->D, n_out = h->n_out, off = Np - m;
    const size_t NN = (size_t)Np * Np;
    if (info) for (int d = 0; d < n_out; ++d) info[d] = 0;

    // workspace: bounded by the chunk, nothing of size N x m
    long rows_max = std::min<long>(std::min<long>(h->chunk, SR_SP_MAX_ROWS), round_up(N, SR_SP_ROWS));
    rows_max = std::max<long>(SR_SP_ROWS, rows_max / SR_SP_ROWS * SR_SP_ROWS);
    const int strips_max = (int)(rows_max / SR_SP_ROWS);
    sp_ws w;
    SR_TRY(dev_alloc(&w.G, (size_t)n_out * NN));
    SR_TRY(dev_alloc(&w.Km, (size_t)n_out * NN));
    SR_TRY(dev_alloc(&w.T, NN));
    SR_TRY(dev_alloc(&w.panel, (size_t)n_out * rows_max * Np));
    SR_TRY(dev_alloc(&w.bpart, (size_t)strips_max * n_out * Np));
    SR_TRY(dev_alloc(&w.b, (size_t)n_out * Np));
    SR_TRY(dev_alloc(&w.info, (size_t)n_out));
    SR_HIP(hipMemsetAsync(w.G, 0, sizeof(double) * n_out * NN, s));
    SR_HIP(hipMemsetAsync(w.b, 0, sizeof(double) * n_out * Np, s));

    // ---- streamed part: G += K_fu^T K_fu, b += K_uf y, chunk by chunk
    const sr_batch bt{n_out, (long)rows_max * Np, (long)rows_max * Np, (long)NN, 0};
    for (long row0 = 0; row0 < N; row0 += rows_max) {
        const int rows = (int)std::min<long>(rows_max, N - row0);
        const int rows_p = (int)round_up(rows, SR_SP_ROWS);       // (a multiple of the tile's k step, 16)
        const int strips = rows_p / SR_SP_ROWS;
        {
            sr_prof_scope ps(&h->prof, SR_K_SPARSE_PANEL, s);
            hipLaunchKernelGGL(sr_sp_panel_kernel, dim3((Np + 255) / 256, strips, n_out), dim3(256), 0, s, X, Y, row0, rows,
                               h->Z, h->ls, h->sf2, h->general ? h->kp : nullptr, w.panel, (long)rows_max * Np, w.bpart, m, Np, D,
                               n_out);
            SR_HIP(hipGetLastError());
            const long nb_ = (long)n_out * Np;
            hipLaunchKernelGGL(sr_sp_bsum_kernel, dim3((unsigned)((nb_ + 255) / 256)), dim3(256), 0, s, w.bpart, strips, w.b, nb_);
            SR_HIP(hipGetLastError());
        }
        {
            sr_prof_scope ps(&h->prof, SR_K_SPARSE_GEMM, s);
            SR_TRY(sr_launch_gemm_tn_upper(w.panel, Np, w.panel, Np, w.G, Np, Np, Np, rows_p, 1.0, 1.0, s, 0, -1, &bt));
        }
    }

    // ---- m x m part.  K_uu + jitter I (the Gram kernels, the jitter in the place of the noise), Sigma in place of G
    if (h->general) SR_TRY(sr_launch_gram_general(h->Z, h->kp, jitter, nullptr, w.Km, m, Np, D, s, n_out, (long)NN));
    else SR_TRY(sr_launch_gram(h->Z, h->ls, 0.0, jitter, h->sf2, nullptr, w.Km, m, Np, D, s, n_out, (long)NN));
    hipLaunchKernelGGL(sr_sp_sigma_kernel, dim3((Np + 255) / 256, Np, n_out), dim3(256), 0, s, w.G, w.Km, h->noise, w.b, Np);
    SR_HIP(hipGetLastError());

    std::vector<int> raw(n_out, 0);
    auto fail = [&](const char* what, bool reversed) {
        int bad = -1;
        for (int d = 0; d < n_out; ++d) {
            int p = raw[d];
            if (p > 0) p = reversed ? std::min(m, std::max(1, m - p + 1)) : std::max(1, p - off);     // padded -> inducing row
            if (info) info[d] = p;
            if (p != 0 && bad < 0) bad = d;
        }
        h->factorized = 0;
        sr_set_error("sr_gp_fit_sparse: Cholesky breakdown of %s: output %d, pivot %d not positive", what, bad, info ? info[bad] : 0);
        return SR_ENOTPD;
    };
    // a pass of the factorisation; check (K_uu only: Sigma's and M's pivots are bounded below by its): then the pivots that
    // are positive by rounding only
    auto pass = [&](const sr_fact_src& src, const char* what, bool check) -> int {
        const int rc = factorize_matrix(h, stream, raw.data(), &src);
        if (rc == SR_ENOTPD) return fail(what, src.reversed != 0);
        SR_TRY(rc);
        if (!check) return SR_OK;
        SR_HIP(hipMemsetAsync(w.info, 0, sizeof(int) * n_out, s));
        hipLaunchKernelGGL(sr_sp_pivot_check_kernel, dim3(n_out), dim3(256), 0, s, h->Wt, src.mat, Np, off, w.info);
        SR_HIP(hipGetLastError());
        SR_HIP(hipMemcpyAsync(raw.data(), w.info, sizeof(int) * n_out, hipMemcpyDeviceToHost, s));
        SR_HIP(hipStreamSynchronize(s));
        for (int d = 0; d < n_out; ++d) if (raw[d] != 0) return fail(what, false);
        return SR_OK;
    };
    // A^-1 = Wt Wt^T on the upper block triangle: C (op)= sign T^T T with T = Wt^T (k-major)
    auto add_inverse = [&](double sign, double beta) -> int {
        for (int d = 0; d < n_out; ++d) {
            SR_TRY(sr_launch_transpose(h->Wt + (size_t)d * NN, w.T, Np, s));
            sr_prof_scope ps(&h->prof, SR_K_GEMM, s);
            SR_TRY(sr_launch_gemm_tn_upper(w.T, Np, w.T, Np, w.Km + (size_t)d * NN, Np, Np, Np, Np, sign, beta, s));
        }
        return SR_OK;
    };
    SR_TRY(pass(sr_fact_src{w.Km, nullptr, 0}, "K_uu", true));
    SR_TRY(add_inverse(1.0, 0.0));                       // Km = K_uu^-1
    SR_TRY(pass(sr_fact_src{w.G, w.b, 0}, "Sigma", false));   // alpha = Sigma^-1 b / s2 = beta
    SR_TRY(add_inverse(-1.0, 1.0));                      // Km = M
    // R = J M J (identity on the padding, now at the back) in place of Sigma; its factor, reversed again, is P
    hipLaunchKernelGGL(sr_sp_antitranspose_kernel, dim3(Np / 32, Np / 32, n_out), dim3(256), 0, s, w.Km, w.Km, w.G, Np, off, 0,
                       (long)NN, (long)NN);
    SR_HIP(hipGetLastError());
    return pass(sr_fact_src{w.G, nullptr, 1}, "K_uu^-1 - Sigma^-1", false);
}
