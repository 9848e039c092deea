// sr_predict_grad.hip -- batched gradient of the predictive variance, d var / dx, for every query of a batch
// (sr_gp_predict_grad).  With K_y = U^T U, Wt = U^-1 (k-major, upper triangular) and K* the cross-covariance slab:
//
//   KV  sr_var_v_kernel   : the variance contraction of sr_var_kernel (V = Wt^T K*, part[rb][t] = sum_{i in rb} V[i][t]^2)
//                           that also STORES V (n_out x Np x Tp, the shape of K*)                       [MFMA bound]
//   KG  sr_grad_g_kernel  : G = Wt V = K_y^-1 K* on the fp64 matrix cores (row block kb contracts over i in [kb 128, Np)),
//                           never stored: the epilogue forms  sum_{i in kb} G[i][t] dk_i/dx_j  per query column
//                           -> gpart[kb][j][t]                                                          [MFMA bound]
//   KF  sr_grad_finish    : jac_var[t][d][j] = dk(x,x)/dx_j - 2 sum_kb gpart (row blocks in ascending order)
//
// RBF: dk_i/dx_j = k_i (z_ij - x_j) / l_j^2 (the 1 / l_j^2 goes into the finish), dk(x,x)/dx = 0.
// General family (sr_kernel_dev.h): dk_i/dx_j = a_j z_ij v kappa + c v g u_j + b_j z_ij, u_j = s_j^2 (x_j - z_ij),
// c = c0 + sum a_j x_j z_ij, g = kappa'(r)/r; dk(x,x)/dx_j = 2 (a_j v + b_j) x_j  (the closed forms of
// sr_linearize_general_kernel, there for one query).
// mu, var and d mu/dx come from the K* pass and sr_finalize exactly as in sr_gp_predict.
// sr_gp_linearize_batch (below) adds the Hessian of the mean behind that pass: KH / KHF.
#include "sr_handle.h"
#include "sr_kernel_dev.h"
using namespace srh;

// ------------------------------------------------------------------------------------------------
// KV: sr_var_kernel<4> (one 128 x 128 tile per workgroup, row blocks heavy first inside groups of `group` query tiles,
// the pipelined loop without the structural zeros of the diagonal block) plus non-temporal stores of the V tile.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sr_var_v_kernel(const double* __restrict__ Wt, const double* __restrict__ Ks,
                                                          double* __restrict__ part, double* __restrict__ V, int Np,
                                                          long Tp, int nrb, int ntq, int group, int k_beg) {
    __shared__ double smem[srt::SMEM_DOUBLES];
    const int ngrp = (ntq + group - 1) / group;
    const long per_d_padded = (long)ngrp * nrb * group;
    const long b = blockIdx.x;
    const int d = (int)(b / per_d_padded);
    long rem = b % per_d_padded;
    const int xg = (int)(rem / ((long)nrb * group));
    rem = rem % ((long)nrb * group);
    const int item = (int)(rem / group);
    const int x = xg * group + (int)(rem % group);
    if (x >= ntq) return;
    const int rb = nrb - 1 - item;
    const double* B = Ks + (long)d * Np * Tp + (long)x * srt::BN;
    const double* A = Wt + (long)d * Np * Np + (long)rb * srt::BM;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    srt::Acc acc;
    acc.zero();
    srt::mainloop_tn_pipe<true>(A, Np, B, Tp, k_beg, (rb + 1) * srt::BM, smem, acc);

    double* Vt = V + ((long)d * Np + (long)rb * srt::BM) * Tp + (long)x * srt::BN;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double* row = Vt + (long)srt::acc_row_ilv(wm, mi, lane, r) * Tp;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) __builtin_nontemporal_store(acc.v[mi][ni][r], row + srt::acc_col(wn, ni, lane));
        }
    double s[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        double v = 0.0;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) v = fma(acc.v[mi][ni][r], acc.v[mi][ni][r], v);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        s[ni] = v;
    }
    double* red = smem;                        // the main loop ended with a barrier
    if (lane < 16) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) red[wm * 128 + wn * 64 + ni * 16 + lane] = s[ni];
    }
    __syncthreads();
    if (threadIdx.x < 128)
        part[((long)d * nrb + rb) * Tp + (long)x * srt::BN + threadIdx.x] = red[threadIdx.x] + red[128 + threadIdx.x];
}

// ------------------------------------------------------------------------------------------------
// KG: row block kb (128 rows of G), query tile x.  The workgroups of one query tile contract over (nrb - kb) 128-blocks;
// they are dealt in PAIRS (kb, nrb - 1 - kb) as in sr_var_kernel<5>: every pair costs nrb + 1 blocks, so the resident
// workgroups start and finish together.  Rows below the first real training row (front padding, off = Np - N) have no Z
// row and K* = 0 there: they contribute nothing (the k range starts at the padding's last whole 16-row step).
// ------------------------------------------------------------------------------------------------
#define SR_GRAD_MAX_D 8
struct sr_grad_args {
    const double* Wt; const double* V; const double* Ks; const double* Z; const double* Xq; const double* kp;
    double* gpart;                             // n_out x nrb x D x Tp
    int N, Np, D, nrb, ntq, group;
    long T, Tp;
};

// one row block kb of query tile x (the body of sr_grad_g_kernel; a function rather than a loop over the pair so that
// nothing of the epilogue is hoisted in front of the main loop, where it would hold registers the MFMA tiles need)
template <int DT, bool GEN>
__device__ __forceinline__ void grad_tile(const sr_grad_args& a, int d, int x, int kb, double* smem) {
    const int Np = a.Np, D = a.D;
    const long Tp = a.Tp;
    const int off = Np - a.N;
    const int k_lo = (off / srt::BK) * srt::BK;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const double* kp = GEN ? a.kp + (long)d * SR_KP(D) : nullptr;
    const double* Bv = a.V + (long)d * Np * Tp + (long)x * srt::BN;
    const int m0 = kb * srt::BM;
    double* gp = a.gpart + ((long)d * a.nrb + kb) * D * Tp + (long)x * srt::BN;
    if (m0 + srt::BM <= off) {                           // padding only
        for (int e = threadIdx.x; e < D * srt::BN; e += 256) gp[(long)(e / srt::BN) * Tp + e % srt::BN] = 0.0;
        return;
    }
    srt::Acc acc;
    acc.zero();
    srt::mainloop_nt_glds(a.Wt + (long)d * Np * Np + (long)m0 * Np, Np, Bv, Tp, max(m0, k_lo), Np, smem, acc);

    // epilogue: Z rows of the block into LDS (zeros on padding rows), then per query column the D weighted sums
    double* zs = smem;                                   // 128 x DT
    double* red = smem + srt::BM * DT;                   // 2 (wm) x DT x 128 columns
    if (threadIdx.x < srt::BM) {
        const int i = m0 + threadIdx.x - off;
#pragma unroll
        for (int j = 0; j < DT; ++j) zs[threadIdx.x * DT + j] = (i >= 0 && j < D) ? a.Z[(long)i * D + j] : 0.0;
    }
    __syncthreads();
    sr_kpar<DT> P;                                       // (read by the general form only)
    if (GEN) P.load(kp, D);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int col = srt::acc_col(wn, ni, lane);
        const long t = (long)x * srt::BN + col;
        // K* of this column in the rows of the lane: element (mi, r) is 16 mi + 4 r rows further (uniform offsets)
        const double* kcol = a.Ks + ((long)d * Np + m0 + wm * 64 + (lane >> 4)) * Tp + t;
        double xq[DT], sum[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            xq[j] = (t < a.T && j < D) ? a.Xq[t * D + j] : 0.0;
            sum[j] = 0.0;
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // one element at a time: hoisting the loads of all 64 would spill the accumulators
                __builtin_amdgcn_sched_barrier(0);
                const int row = srt::acc_row(wm, mi, lane, r);
                const double g = acc.v[mi][ni][r];
                if (!GEN) {
                    // G_i k_i (z_ij - x_j): K* is zero on padding rows and on padded query columns
                    const double w = g * kcol[(long)(mi * 16 + 4 * r) * Tp];
#pragma unroll
                    for (int j = 0; j < DT; ++j) sum[j] = fma(w, zs[row * DT + j] - xq[j], sum[j]);
                } else if (m0 + row >= off && t < a.T) {
                    double r2 = 0.0, la = 0.0;
#pragma unroll
                    for (int j = 0; j < DT; ++j) {
                        const double df = xq[j] - zs[row * DT + j];
                        r2 = fma(df * P.s2[j], df, r2);
                        la = fma(P.a[j] * xq[j], zs[row * DT + j], la);
                    }
                    double kap, gk, hk;                  // kappa and kappa'(r)/r
                    sr_radial<1>(P.kind, r2, kap, gk, hk);
                    const double gvk = g * P.v * kap, gcg = g * (P.c0 + la) * P.v * gk;
#pragma unroll
                    for (int j = 0; j < DT; ++j) {
                        const double z = zs[row * DT + j];
                        sum[j] = fma(gvk * P.a[j] + g * P.b[j], z, fma(gcg * P.s2[j], xq[j] - z, sum[j]));
                    }
                }
            }
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            double v = sum[j];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16 && j < D) red[(wm * DT + j) * srt::BN + col] = v;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < D * srt::BN; e += 256) {
        const int j = e / srt::BN, c = e % srt::BN;
        gp[(long)j * Tp + c] = red[j * srt::BN + c] + red[(DT + j) * srt::BN + c];
    }
    __syncthreads();                                     // zs / red are read: the next block's DMA may land
}

// (D <= 3 -- the pendulum-shaped systems of the headline -- fits two workgroups per CU without scratch; the wider inputs
//  hold 2 x DT query coordinates and sums per column beside the 64 accumulator doubles and take one workgroup per CU.
//  D = 9 .. 12 spilled even there and is not compiled: SR_GRAD_MAX_D)
template <int DT, bool GEN>
__global__ __launch_bounds__(256, DT <= 3 ? 2 : 1) void sr_grad_g_kernel(sr_grad_args a) {
    __shared__ double smem[srt::SMEM_DOUBLES];
    const int npair = (a.nrb + 1) / 2;
    const int ngrp = (a.ntq + a.group - 1) / a.group;
    const long per_d_padded = (long)ngrp * npair * a.group;
    const long b = blockIdx.x;
    const int d = (int)(b / per_d_padded);
    long rem = b % per_d_padded;
    const int xg = (int)(rem / ((long)npair * a.group));
    rem = rem % ((long)npair * a.group);
    const int item = (int)(rem / a.group);
    const int x = xg * a.group + (int)(rem % a.group);
    if (x >= a.ntq) return;
    grad_tile<DT, GEN>(a, d, x, item, smem);
    if (a.nrb - 1 - item != item) grad_tile<DT, GEN>(a, d, x, a.nrb - 1 - item, smem);   // (odd count: the middle one alone)
}

// KF: one thread per (query, output): the row blocks' partial sums in ascending order (deterministic), the prior term
__global__ __launch_bounds__(256) void sr_grad_finish_kernel(const double* __restrict__ gpart, const double* __restrict__ ls,
                                                             const double* __restrict__ kp, const double* __restrict__ Xq,
                                                             double* __restrict__ jac_var, int n_out, int D, int nrb,
                                                             long T, long Tp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= T * n_out) return;
    const long t = e / n_out;
    const int d = (int)(e % n_out);
    for (int j = 0; j < D; ++j) {
        const double* p = gpart + ((long)d * nrb * D + j) * Tp + t;
        double s = 0.0;
        for (int kb = 0; kb < nrb; ++kb) s += p[(long)kb * D * Tp];
        double out;
        if (kp) {
            out = sr_dkxx(kp + (long)d * SR_KP(D), D, j, Xq[t * D + j]) - 2.0 * s;
        } else {
            const double l = ls[d * D + j];
            out = -2.0 * s / (l * l);
        }
        jac_var[e * D + j] = out;
    }
}

static int launch_grad_g(const sr_grad_args& a, bool gen, int n_out, hipStream_t s) {
    const int npair = (a.nrb + 1) / 2;
    const int ngrp = (a.ntq + a.group - 1) / a.group;
    const long blocks = (long)n_out * ngrp * npair * a.group;
    SR_CHECK(blocks < 2147483647L, SR_EINVAL, "predict_grad: grid too large (%ld blocks)", blocks);
    const dim3 grid((unsigned)blocks);
    return sr_pick_le<3, 5, 8>("predict_grad", a.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return gen ? sr_launch(sr_grad_g_kernel<DT, true>, grid, dim3(256), 0, s, a)
                   : sr_launch(sr_grad_g_kernel<DT, false>, grid, dim3(256), 0, s, a); });
}

// workspace of the gradient route: V (the shape of K*) and the row blocks' partial sums
static int grad_buffers(sr_gp* h, long Tp, hipStream_t s) {
    const long nv = (long)h->n_out * h->Np * Tp;
    const long np = (long)h->n_out * (h->Np / SR_NB) * h->D * Tp;
    SR_TRY(h->grad_v.grow((size_t)nv, wait::stream(s)));
    return h->grad_part.grow((size_t)np, wait::stream(s));
}

// one chunk: K* pass -> V-storing contraction -> G + epilogue -> finalize (mu, var, jac_mu) + jac_var
static int grad_pass(sr_gp* h, long Tc, const double* Xq, double* mu, double* var, double* jac_mu, double* jac_var,
                     hipStream_t s) {
    const long Tp = round_up(Tc, srt::BN);
    const int nsplit = pick_nsplit(h, Tp);
    SR_TRY(ensure_ws(h, Tp, nsplit));
    SR_TRY(grad_buffers(h, Tp, s));
    sr_kstar_args ka = kstar_ws(h, nsplit, Tc, Tp);
    ka.xa = Xq; ka.lda = h->D; ka.na = h->D;
    {
        sr_prof_scope ps(&h->prof, SR_K_KSTAR, s);
        SR_TRY(sr_launch_kstar(ka, s));
    }
    const int nrb = h->Np / SR_NB;
    const int ntq = (int)(Tp / srt::BN);
    const int group = std::max(1, std::min(h->var_group, ntq));
    {
        sr_prof_scope ps(&h->prof, SR_K_VAR, s);
        SR_TRY(tile_route_alignment(h));
        const int k_beg = ((h->Np - h->N) / srt::BK) * srt::BK;
        const int ngrp = (ntq + group - 1) / group;
        const long blocks = (long)h->n_out * ngrp * nrb * group;
        SR_CHECK(blocks < 2147483647L, SR_EINVAL, "predict_grad: grid too large (%ld blocks)", blocks);
        hipLaunchKernelGGL(sr_var_v_kernel, dim3((unsigned)blocks), dim3(256), 0, s, h->Wt, h->Ks, h->var_part, h->grad_v.get(),
                           h->Np, Tp, nrb, ntq, group, k_beg);
        SR_HIP(hipGetLastError());
        sr_grad_args ga;
        ga.Wt = h->Wt; ga.V = h->grad_v.get(); ga.Ks = h->Ks; ga.Z = h->Z; ga.Xq = Xq; ga.kp = h->general ? h->kp : nullptr;
        ga.gpart = h->grad_part.get();
        ga.N = h->N; ga.Np = h->Np; ga.D = h->D; ga.nrb = nrb; ga.ntq = ntq; ga.group = group; ga.T = Tc; ga.Tp = Tp;
        SR_TRY(launch_grad_g(ga, h->general != 0, h->n_out, s));
    }
    const sr_final_args fa = final_args(h, nsplit, nrb, Tc, Tp, h->var_part, mu, var, jac_mu);
    sr_prof_scope ps(&h->prof, SR_K_FINAL, s);
    SR_TRY(sr_launch_finalize(fa, s));
    const long n = Tc * h->n_out;
    hipLaunchKernelGGL(sr_grad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->grad_part.get(), h->ls,
                       h->general ? h->kp : nullptr, Xq, jac_var, h->n_out, h->D, nrb, Tc, Tp);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

extern "C" int sr_gp_predict_grad(sr_gp_t h, const double* Xq, long T, double* mu, double* var, double* jac_mu,
                                  double* jac_var, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_predict_grad: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_predict_grad: model not factorized");
    SR_CHECK(T >= 0, SR_EINVAL, "sr_gp_predict_grad: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(Xq && mu && var && jac_var, SR_EINVAL, "sr_gp_predict_grad: NULL argument");
    if (h->D > SR_GRAD_MAX_D) {
        sr_set_error("sr_gp_predict_grad: D=%d > %d (sr_gp_linearize serves one query of any D)", h->D, SR_GRAD_MAX_D);
        return SR_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    for (long t0 = 0; t0 < T; t0 += h->chunk) {
        const long Tc = std::min(h->chunk, T - t0);
        SR_TRY(grad_pass(h, Tc, Xq + t0 * h->D, mu + t0 * h->n_out, var + t0 * h->n_out,
                         jac_mu ? jac_mu + t0 * h->n_out * h->D : nullptr, jac_var + t0 * h->n_out * h->D, s));
    }
    return SR_OK;
}

// ------------------------------------------------------------------------------------------------
// sr_gp_linearize_batch: the pass of sr_gp_predict_grad, then the Hessian of the mean for every query of the chunk.
//   KH  sr_hess_kernel        : per output d and query t, over the training rows i of one split (blockIdx.z)
//         RBF      H_jc = sum_i alpha_i k_ti (z_ij - x_j)(z_ic - x_c) / (l_j^2 l_c^2)  [- delta_jc / l_j^2 sum_i alpha_i k_ti]
//                  k_ti read from the chunk's K* slab (the K* pass of grad_pass left it there);
//         general  H_jl = sum_i alpha_i [v g (a_j z_j u_l + a_l z_l u_j) + c v (h u_j u_l + g s_j^2 delta_jl)]
//                  (sr_d2k of sr_kernel_dev.h; g and h recomputed per pair).
//       Summed in centred coordinates z_i - x_t: the expanded form W^T [1 | Z | Z Z^T] would be one matrix product, but it
//       cancels terms of size |x|^2 sum |alpha k| down to the result and loses the digits the fp64 bars need.
//       One thread per (query, output); Z rows and alpha staged through LDS (broadcast reads); the upper triangle of the
//       D x D block (plus sum_i alpha_i k_ti for RBF) -> hpart[split][d][q][t]                           [HBM / VALU bound]
//   KHF sr_hess_finish_kernel : the splits in ascending order (deterministic), the diagonal term, both halves of the triangle
//       written from the one value (exactly symmetric)
// ------------------------------------------------------------------------------------------------
#define SR_HZT 256
struct sr_hess_args {
    const double* Ks; const double* Z; const double* alpha; const double* ls; const double* kp; const double* Xq;
    double* hpart;                             // nsplit x n_out x nhp x Tp
    int N, Np, D, n_out, nsplit, nhp;          // nhp: D (D + 1) / 2 triangle entries (+ 1 for sum alpha k, RBF)
    long T, Tp;
};

// entry q of the D-wide upper triangle, row by row: (0,0) (0,1) .. (0,D-1) (1,1) ..
__host__ __device__ static inline int sr_tri_index(int j, int c, int D) { return j * D - j * (j - 1) / 2 + (c - j); }

template <int DT, bool GEN>
__global__ __launch_bounds__(256) void sr_hess_kernel(sr_hess_args a) {
    constexpr int NH = DT * (DT + 1) / 2;
    __shared__ double zs[SR_HZT * DT];
    __shared__ double al[SR_HZT];
    const int d = blockIdx.y, sp = blockIdx.z;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < a.T;
    const int D = a.D, off = a.Np - a.N;
    double x[DT], il2[DT], acc[NH], sw = 0.0;            // il2: 1 / l_j^2 (RBF)
    sr_kpar<DT> P;
    if (GEN) P.load(a.kp + (long)d * SR_KP(D), D);
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        x[j] = (live && j < D) ? a.Xq[t * D + j] : 0.0;
        if (!GEN) {
            const double l = (j < D) ? a.ls[d * D + j] : 1.0;
            il2[j] = (j < D) ? 1.0 / (l * l) : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < NH; ++q) acc[q] = 0.0;
    // real training rows only: row i of Z is row i + off of K* and alpha (front padding)
    const int rows_per = (a.N + a.nsplit - 1) / a.nsplit;
    const int i_beg = sp * rows_per;
    const int i_end = min(a.N, i_beg + rows_per);
    const double* ks = GEN ? nullptr : a.Ks + ((long)d * a.Np + off) * a.Tp + (live ? t : 0);
    for (int i0 = i_beg; i0 < i_end; i0 += SR_HZT) {
        const int nrow = min(SR_HZT, i_end - i0);
        __syncthreads();
        if (threadIdx.x < nrow) {
            const int r = threadIdx.x;
#pragma unroll
            for (int j = 0; j < DT; ++j) zs[r * DT + j] = (j < D) ? a.Z[(long)(i0 + r) * D + j] : 0.0;
            al[r] = a.alpha[(long)d * a.Np + off + i0 + r];
        }
        __syncthreads();
        if (!live) continue;
        if (!GEN) {
#pragma unroll 4
            for (int r = 0; r < nrow; ++r) {
                const double w = al[r] * ks[(long)(i0 + r) * a.Tp];
                double df[DT];
#pragma unroll
                for (int j = 0; j < DT; ++j) df[j] = (zs[r * DT + j] - x[j]) * il2[j];
                sw += w;
                int q = 0;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    const double wd = w * df[j];
#pragma unroll
                    for (int c = j; c < DT; ++c) { acc[q] = fma(wd, df[c], acc[q]); ++q; }
                }
            }
        } else {
            for (int r = 0; r < nrow; ++r) {
                double z[DT], u[DT], r2 = 0.0, la = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    z[j] = zs[r * DT + j];
                    const double df = x[j] - z[j];
                    u[j] = P.s2[j] * df;
                    r2 = fma(u[j], df, r2);
                    la = fma(P.a[j] * x[j], z[j], la);
                }
                double kap, g, h;                 // kappa'(r)/r and g'(r)/r (kappa itself is not needed: nobody reads it)
                sr_radial<2>(P.kind, r2, kap, g, h);
                const double pre = (P.c0 + la) * P.v;
                const double w = al[r];
                const double vg = P.v * g, pg = pre * g, ph = pre * h;
                int q = 0;
#pragma unroll
                for (int j = 0; j < DT; ++j)
#pragma unroll
                    for (int c = j; c < DT; ++c) {
                        acc[q] = fma(w, sr_d2k(j, c, u, z, P.a, P.s2, vg, pg, ph), acc[q]);
                        ++q;
                    }
            }
        }
    }
    if (!live) return;
    double* hp = a.hpart + ((long)sp * a.n_out + d) * a.nhp * a.Tp + t;
    int q = 0;
#pragma unroll
    for (int j = 0; j < DT; ++j)
#pragma unroll
        for (int c = j; c < DT; ++c) {
            if (c < D) hp[(long)sr_tri_index(j, c, D) * a.Tp] = acc[q];
            ++q;
        }
    if (!GEN) hp[(long)(a.nhp - 1) * a.Tp] = sw;
}

// KHF: one thread per (query, output, triangle entry), queries fastest (the partials are read along t)
__global__ __launch_bounds__(256) void sr_hess_finish_kernel(const double* __restrict__ hpart, const double* __restrict__ ls,
                                                             double* __restrict__ hess, int gen, int n_out, int D,
                                                             int nsplit, int nhp, long T, long Tp) {
    const int nhd = D * (D + 1) / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= T * n_out * nhd) return;
    const long t = e % T;
    const int q = (int)((e / T) % nhd), d = (int)(e / (T * nhd));
    int j = 0, c = q;
    while (c >= D - j) { c -= D - j; ++j; }
    c += j;
    const long stride = (long)n_out * nhp * Tp;
    const double* p = hpart + (long)d * nhp * Tp + t;
    const bool diag = !gen && c == j;                   // RBF diagonal: sum_i alpha_i k_ti as well
    double s = 0.0, sw = 0.0;
    // (unrolled: the loads of several splits in flight -- a small batch has up to N / SR_HESS_MIN_ROWS splits)
#pragma unroll 8
    for (int sp = 0; sp < nsplit; ++sp) {
        s += p[sp * stride + (long)q * Tp];
        if (diag) sw += p[sp * stride + (long)(nhp - 1) * Tp];
    }
    if (diag) {
        const double l = ls[d * D + j];
        s -= sw * (1.0 / (l * l));
    }
    double* hm = hess + (t * n_out + d) * (long)D * D;
    hm[j * D + c] = s;
    hm[c * D + j] = s;
}

// one chunk after grad_pass: reads the chunk's K* slab (RBF) before the next chunk's K* pass overwrites it
static int hess_pass(sr_gp* h, long Tc, const double* Xq, double* hess_mu, hipStream_t s) {
    const long Tp = round_up(Tc, srt::BN);              // the K* slab's row stride, as in grad_pass
    const int nsplit = sr_hess_nsplit(h->N, h->n_out, Tp);
    const int nhd = h->D * (h->D + 1) / 2;
    const int nhp = nhd + (h->general ? 0 : 1);
    SR_TRY(h->hess_part.grow((size_t)nsplit * h->n_out * nhp * Tp, wait::stream(s)));       // the splits' partial sums
    sr_hess_args a;
    a.Ks = h->Ks; a.Z = h->Z; a.alpha = h->alpha; a.ls = h->ls; a.kp = h->general ? h->kp : nullptr; a.Xq = Xq;
    a.hpart = h->hess_part.get();
    a.N = h->N; a.Np = h->Np; a.D = h->D; a.n_out = h->n_out; a.nsplit = nsplit; a.nhp = nhp; a.T = Tc; a.Tp = Tp;
    const dim3 grid((unsigned)((Tp + 255) / 256), h->n_out, nsplit);
    SR_TRY((sr_pick_le<3, 5, 8>("linearize_batch", h->D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        return h->general ? sr_launch(sr_hess_kernel<DT, true>, grid, dim3(256), 0, s, a)
                          : sr_launch(sr_hess_kernel<DT, false>, grid, dim3(256), 0, s, a); })));
    const long n = Tc * h->n_out * nhd;
    hipLaunchKernelGGL(sr_hess_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->hess_part.get(), h->ls,
                       hess_mu, h->general, h->n_out, h->D, nsplit, nhp, Tc, Tp);
    SR_HIP(hipGetLastError());
    return SR_OK;
}

extern "C" int sr_gp_linearize_batch(sr_gp_t h, const double* Xq, long T, double* mu, double* var, double* jac_mu,
                                     double* jac_var, double* hess_mu, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_linearize_batch: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_linearize_batch: model not factorized");
    SR_CHECK(T >= 0, SR_EINVAL, "sr_gp_linearize_batch: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(Xq && mu && var && jac_mu && jac_var && hess_mu, SR_EINVAL, "sr_gp_linearize_batch: NULL argument");
    if (h->D > SR_GRAD_MAX_D) {
        sr_set_error("sr_gp_linearize_batch: D=%d > %d (sr_gp_linearize serves one query of any D)", h->D, SR_GRAD_MAX_D);
        return SR_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const long nd = (long)h->n_out * h->D;
    for (long t0 = 0; t0 < T; t0 += h->chunk) {
        const long Tc = std::min(h->chunk, T - t0);
        SR_TRY(grad_pass(h, Tc, Xq + t0 * h->D, mu + t0 * h->n_out, var + t0 * h->n_out, jac_mu + t0 * nd,
                         jac_var + t0 * nd, s));
        SR_TRY(hess_pass(h, Tc, Xq + t0 * h->D, hess_mu + t0 * nd * h->D, s));
    }
    return SR_OK;
}

#ifdef SR_LAB
// ------------------------------------------------------------------------------------------------
// Lab build only: C = A B through srt::mainloop_nt_glds (A M x K row-major, B K x N k-major, C M x N row-major; M, N
// multiples of 128, K of 16; device pointers, A and B 16-byte aligned).  Checked with an identity A and an asymmetric B.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void sr_test_nt_kernel(const double* A, long lda, const double* B, long ldb, double* C,
                                                            long ldc, int K) {
    __shared__ double smem[srt::SMEM_DOUBLES];
    const int m0 = blockIdx.x * srt::BM, n0 = blockIdx.y * srt::BN;
    srt::Acc acc;
    acc.zero();
    srt::mainloop_nt_glds(A + (long)m0 * lda, lda, B + n0, ldb, 0, K, smem, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                C[(long)(m0 + srt::acc_row(wm, mi, lane, r)) * ldc + n0 + srt::acc_col(wn, ni, lane)] = acc.v[mi][ni][r];
}

extern "C" int sr_test_gemm_nt(int device, const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                               int M, int N, int K, void* stream) {
    SR_CHECK(M > 0 && N > 0 && K > 0 && M % srt::BM == 0 && N % srt::BN == 0 && K % srt::BK == 0, SR_EINVAL,
             "sr_test_gemm_nt: M=%d N=%d K=%d", M, N, K);
    SR_CHECK(lda >= K && ldb >= N && ldc >= N && lda % 2 == 0 && ldb % 2 == 0, SR_EINVAL, "sr_test_gemm_nt: strides");
    SR_DEVICE(device);
    hipLaunchKernelGGL(sr_test_nt_kernel, dim3(M / srt::BM, N / srt::BN), dim3(256), 0, (hipStream_t)stream, A, lda, B,
                       ldb, C, ldc, K);
    SR_HIP(hipGetLastError());
    return SR_OK;
}
#endif
