// sr_remove.hip -- retire ONE training point from the exact model without refactorising (sr_gp_remove), and the
// leave-one-out posterior of the training rows (sr_gp_loo).  fp64, gfx950; bandwidth-bound passes over U^-1, no matrix cores.
//
// The handle keeps Wt = U^-1 per output: upper triangular, row-major with stride Np, K_y^-1 = Wt Wt^T, the Np - N padding
// rows at the FRONT (identity block).  Removing training point j = padded index q = j + off deletes column q of the factor of
// K_y^-1 and makes row q a multiple of e_q: the product of the Givens rotations of the column pairs (q, k), k = q+1 .. Np-1,
// that turn row q, w = Wt[q, q:], into rho e_q.  Written without the chain, for every other row x = Wt[i, :]
//     p_k^2 = sum_{q <= l < k} w_l^2   (p_{q+1} = w_q = 1 / U_qq > 0,  rho^2 = p_Np^2 = (K_y^-1)_jj)
//     d_k   = sum_{q <= l < k} w_l x_l                        (a prefix sum along the row)
//     x'_k  = (p_k / p_{k+1}) x_k - (w_k / (p_k p_{k+1})) d_k     for k > q;   x'_k = x_k for k < q;   column q disappears
//     alpha'_i = alpha_i - (d_Np(i) / rho^2) alpha_q,          log det K'_y = log det K_y + log rho^2.
// The rows are independent of each other; along a row it is ONE scan.
//
// Launches of one removal (each finishes on its own: no device-wide barrier, no resident workgroup, no spin-wait):
//   sr_remove_rownorm_kernel   row q of every output -> coefficient tables w_k, a_k = p_k / p_{k+1}, b_k = w_k / (p_k p_{k+1})
//                              (w = 0, a = 1, b = 0 left of q: the rows kernel needs no case for those columns) and rho^2;
//                              3 Np + 4 doubles per output in scratch of the handle (the issue of the divisions out of the hot
//                              loop costs one table more than w and p alone).  Further workgroups of the same launch copy the
//                              input rows behind j aside (Z is compacted in place: the copy back must not overtake its source).
//   sr_remove_compact_kernel   Z rows back one place up; yT compacted into the destination vector; the destination's alpha
//                              padding zeroed
//   sr_remove_rows_kernel      the hot path: every row of the factor, transformed and shifted, into the destination factor;
//                              alpha' from the row's final d
//   sr_remove_clean_kernel     only after a removal from the slid state of the in-place appends (below)
// Routes (sr_capi_remove.hip): ONE route is built, the general one.  The new factor is written into the spare buffer Wt_alt
// (yT_alt / alpha_alt), which ping-pongs with Wt as on the small appends, so nothing big is allocated while the padded size
// stays; when N - 1 becomes a multiple of 128 it is written with the new stride into a fresh allocation.  The source may be
// the VIEW the in-place one-point appends leave (sr_gp::slide): it is read where it lies (8-byte aligned loads when the
// slide is odd) -- no unslide(), which would copy the whole factor first -- and the result is a plain model again.  The
// allocation the view lived in becomes the spare buffer: sr_remove_clean_kernel puts back what makes it a well-formed factor
// in its own coordinates (the view's last `slide` columns wrap into its first ones; the slack behind it is zeroed), one
// pass over n_out Np slide doubles.  The loop "append one point in place, retire one" therefore moves the triangle once per
// step and allocates, copies and clears nothing of its size.
// The in-place route for j = 0 (the sliding window: no row moves) is NOT built: retiring the oldest point costs the same
// read and write of the triangle as any other.
#include "sr_common.h"

#define SR_RM_ROWS 2          // rows a wave carries through the columns together (the coefficient loads are shared)
#define SR_RM_WAVES 4         // waves per workgroup
#define SR_RM_CHUNK 256       // columns per step of a wave: 4 consecutive doubles per lane (two 16-byte loads, 2 KiB per wave and row)
#define SR_RM_NORM_T 1024     // threads of the row-norm workgroup, 4 consecutive columns each per step

// inclusive scan over the 64 lanes of a wave, in a fixed order (the same inputs give the same bits)
static __device__ __forceinline__ double rm_wave_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// Workgroups 0 .. n_out-1: the coefficient tables of output blockIdx.x.  Workgroups n_out ..: Z rows j+1 .. N-1 -> zstash.
__global__ __launch_bounds__(SR_RM_NORM_T) void sr_remove_rownorm_kernel(const double* __restrict__ Wt, int Np, int q, int n_out,
                                                                         double* __restrict__ coef, const double* __restrict__ Z,
                                                                         double* __restrict__ zstash, long zcount, long zfrom) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= n_out) {
        const long e = (long)(blockIdx.x - n_out) * SR_RM_NORM_T + tid;
        if (e < zcount) zstash[e] = Z[zfrom + e];
        return;
    }
    const int d = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* row = Wt + ((size_t)d * Np + q) * Np;
    double* cw = coef + (size_t)d * sr_remove_coef_stride(Np);
    double *ca = cw + Np, *cb = ca + Np;
    for (int k = tid; k < q; k += SR_RM_NORM_T) { cw[k] = 0.0; ca[k] = 1.0; cb[k] = 0.0; }
    __shared__ double wtot[SR_RM_NORM_T / 64];
    double carry = 0.0;                                           // p_k^2 at the first column of the step
    for (int base = q; base < Np; base += 4 * SR_RM_NORM_T) {
        const int k0 = base + 4 * tid;
        double w[4], s[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[e] = (k0 + e < Np) ? row[k0 + e] : 0.0;
            s[e] = w[e] * w[e];
        }
        const double l1 = s[0], l2 = l1 + s[1], l3 = l2 + s[2], tot = l3 + s[3];
        const double inc = rm_wave_scan(tot, lane);
        double exc = __shfl_up(inc, 1);
        if (lane == 0) exc = 0.0;
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        double before = 0.0, all = 0.0;
#pragma unroll
        for (int v = 0; v < SR_RM_NORM_T / 64; ++v) {
            if (v < wave) before += wtot[v];
            all += wtot[v];
        }
        const double p0 = carry + (before + exc);
        const double pk2[5] = {p0, p0 + l1, p0 + l2, p0 + l3, p0 + tot};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k0 + e;
            if (k >= Np) continue;
            double a = 0.0, b = 0.0;
            if (k > q) {                                          // (p_k >= w_q > 0: nothing divides by zero)
                const double pk = sqrt(pk2[e]), pk1 = sqrt(pk2[e + 1]);
                a = pk / pk1;
                b = w[e] / (pk * pk1);
            }
            cw[k] = w[e]; ca[k] = a; cb[k] = b;
        }
        carry += all;
        __syncthreads();                                          // (wtot is written again in the next step)
    }
    if (tid == 0) cw[3 * (size_t)Np] = carry;                     // rho^2
}

// source padded index s (!= q) -> destination padded index: everything behind q keeps its place, everything in front of it
// moves one place down; sh = Np0 - Np1 (0, or 128 when the padded size shrinks: then the destination drops the 128 front rows)
static __device__ __forceinline__ int rm_dst(int s, int q, int sh) { return s - sh + (s < q ? 1 : 0); }

__global__ __launch_bounds__(256) void sr_remove_compact_kernel(const double* __restrict__ yT0, int Np0, int N0, int q, double* __restrict__ yT1,
                                                                double* __restrict__ alpha1, int Np1, int n_out,
                                                                const double* __restrict__ zstash, double* __restrict__ Z, long zcount,
                                                                long zto) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < zcount) Z[zto + i] = zstash[i];
    if (i >= (long)n_out * Np1) return;
    const int d = (int)(i / Np1), r = (int)(i % Np1);
    const int sh = Np0 - Np1, off1 = Np1 - (N0 - 1);
    double y = 0.0;
    if (r >= off1) {
        const int s = (r + sh > q) ? r + sh : r + sh - 1;         // (inverse of rm_dst; s >= Np0 - N0)
        y = yT0[(size_t)d * Np0 + s];
    } else {
        alpha1[(size_t)d * Np1 + r] = 0.0;
    }
    yT1[(size_t)d * Np1 + r] = y;
}

// One wave carries SR_RM_ROWS consecutive rows of U^-1 through the columns, SR_RM_CHUNK at a time (the next step's loads in
// flight under this step's scan): a lane holds 4 consecutive
// columns of every row (its own prefix in registers), the wave scans the lanes' sums (rm_wave_scan) and carries the running
// dot product d to the next step.  Reads: the upper triangle (the step a row starts in is read from the column group its
// diagonal lies in); writes: the upper triangle of the destination, in 32-byte pieces behind column q (where source and
// destination columns coincide), single doubles in front of it (the copy that moves one place down the diagonal).  The wave
// that meets row q writes the identity row the removal leaves at padded index off0 instead (sh == 0), so the destination may
// hold any earlier well-formed factor of this padded size with at least off0 padding rows.
typedef double d4u_t __attribute__((ext_vector_type(4), aligned(8)));     // four doubles of a slid view: 8-byte aligned

template <bool ALIGNED>
__global__ __launch_bounds__(64 * SR_RM_WAVES) void sr_remove_rows_kernel(const double* __restrict__ Wt0, int Np0, int off0, int q,
                                                                          const double* __restrict__ alpha0, const double* __restrict__ coef,
                                                                          double* __restrict__ Wt1, int Np1, double* __restrict__ alpha1) {
    const int d = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = off0 + ((int)blockIdx.x * SR_RM_WAVES + wave) * SR_RM_ROWS;
    if (i0 >= Np0) return;
    const int sh = Np0 - Np1;
    const double* W0 = Wt0 + (size_t)d * Np0 * Np0;
    double* W1 = Wt1 + (size_t)d * Np1 * Np1;
    const double* cw = coef + (size_t)d * sr_remove_coef_stride(Np0);
    const double *ca = cw + Np0, *cb = ca + Np0;
    bool live[SR_RM_ROWS];
    double carry[SR_RM_ROWS];
#pragma unroll
    for (int r = 0; r < SR_RM_ROWS; ++r) {
        live[r] = i0 + r < Np0 && i0 + r != q;
        carry[r] = 0.0;
    }
    // one step's registers: the tables and the rows' columns of this lane.  The NEXT step's are loaded before this step's
    // scan (its load -> scan -> store chain would otherwise be paid once per step: at N = 5000 every wave is resident at
    // once and the longest one walks 20 steps)
    struct step_regs { d4_t w, a, b, x[SR_RM_ROWS]; };
    auto load = [&](int cbase, step_regs& t) {
        const int c = cbase + 4 * lane;
        const bool in = c < Np0;                                  // (Np0 is a multiple of 128: a group of 4 is inside or outside)
        t.w = d4_t{0.0, 0.0, 0.0, 0.0}; t.a = t.w; t.b = t.w;
        if (in) {
            t.w = *reinterpret_cast<const d4_t*>(cw + c);
            t.a = *reinterpret_cast<const d4_t*>(ca + c);
            t.b = *reinterpret_cast<const d4_t*>(cb + c);
        }
#pragma unroll
        for (int r = 0; r < SR_RM_ROWS; ++r) {
            const int i = i0 + r;
            t.x[r] = d4_t{0.0, 0.0, 0.0, 0.0};
            if (live[r] && in && c + 3 >= i) {
                if (ALIGNED) t.x[r] = *reinterpret_cast<const d4_t*>(W0 + (size_t)i * Np0 + c);
                else t.x[r] = *reinterpret_cast<const d4u_t*>(W0 + (size_t)i * Np0 + c);
            }
        }
    };
    step_regs cur, nxt;
    load(i0 & ~(SR_RM_CHUNK - 1), cur);
    for (int cbase = i0 & ~(SR_RM_CHUNK - 1); cbase < Np0; cbase += SR_RM_CHUNK) {
        const int c = cbase + 4 * lane;
        const bool in = c < Np0;
        if (cbase + SR_RM_CHUNK < Np0) load(cbase + SR_RM_CHUNK, nxt);
        const d4_t w = cur.w, a = cur.a, b = cur.b;
        d4_t x[SR_RM_ROWS];
#pragma unroll
        for (int r = 0; r < SR_RM_ROWS; ++r) {
            x[r] = cur.x[r];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < i0 + r) x[r][e] = 0.0;                // (below the diagonal: zero whatever the buffer holds)
        }
#pragma unroll
        for (int r = 0; r < SR_RM_ROWS; ++r) {
            const int i = i0 + r;
            const double t0 = w[0] * x[r][0], t1 = w[1] * x[r][1], t2 = w[2] * x[r][2], t3 = w[3] * x[r][3];
            const double l1 = t0, l2 = l1 + t1, l3 = l2 + t2, tot = l3 + t3;
            const double inc = rm_wave_scan(tot, lane);           // (every lane takes part, live row or not)
            double exc = __shfl_up(inc, 1);
            if (lane == 0) exc = 0.0;
            const double all = __shfl(inc, 63);
            const double d0 = carry[r] + exc;
            carry[r] += all;
            if (!live[r] || !in || c + 3 < i) continue;
            d4_t o;
            o[0] = a[0] * x[r][0] - b[0] * d0;
            o[1] = a[1] * x[r][1] - b[1] * (d0 + l1);
            o[2] = a[2] * x[r][2] - b[2] * (d0 + l2);
            o[3] = a[3] * x[r][3] - b[3] * (d0 + l3);
            double* orow = W1 + (size_t)rm_dst(i, q, sh) * Np1;
            if (c > q && c >= i) {
                *reinterpret_cast<d4_t*>(orow + (c - sh)) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = c + e;
                    if (k >= i && k != q) orow[rm_dst(k, q, sh)] = o[e];
                }
            }
        }
        cur = nxt;
    }
    const double rho2 = cw[3 * (size_t)Np0], aq = alpha0[(size_t)d * Np0 + q];
#pragma unroll
    for (int r = 0; r < SR_RM_ROWS; ++r) {
        const int i = i0 + r;
        if (live[r] && lane == 0)
            alpha1[(size_t)d * Np1 + rm_dst(i, q, sh)] = alpha0[(size_t)d * Np0 + i] - (carry[r] / rho2) * aq;
        if (i == q && sh == 0)                                    // the identity row of the padding the removal leaves
            for (int k = off0 + lane; k < Np1; k += 64) W1[(size_t)off0 * Np1 + k] = (k == off0) ? 1.0 : 0.0;
    }
}

// The allocation a slid view lived in (Wt: n_out Np^2 doubles + wt_slack behind them; alpha, yT: n_out Np + vec_slack), back
// to a well-formed factor in its OWN coordinates.  The view sat `slide` places down the diagonal, so in the allocation's
// coordinates it is upper triangular where it was, except that its last `slide` columns lie wrapped in columns 0 .. slide-1
// (one row further down; those of the last output in the slack): these columns get the identity pattern back, the slack
// zeros.  The vectors are overwritten whole by the next removal or append; their slack is zeroed.
__global__ __launch_bounds__(256) void sr_remove_clean_kernel(double* __restrict__ Wt, double* __restrict__ alpha, double* __restrict__ yT,
                                                              int Np, int n_out, int slide, long wt_slack, long vec_slack) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)n_out * Np * slide) {
        const int c = (int)(i % slide);
        const long dr = i / slide;                                 // output * Np + row
        Wt[dr * Np + c] = (int)(dr % Np) == c ? 1.0 : 0.0;
    }
    if (i < wt_slack) Wt[(size_t)n_out * Np * Np + i] = 0.0;
    if (i < vec_slack) { alpha[(size_t)n_out * Np + i] = 0.0; yT[(size_t)n_out * Np + i] = 0.0; }
}

// Leave-one-out posterior (Rasmussen & Williams 5.12): one wave per training row and output, rho^2 = |row j + off of U^-1|^2.
// Single doubles are loaded: a view of the in-place appends keeps no more than 8-byte alignment.
__global__ __launch_bounds__(256) void sr_loo_kernel(const double* __restrict__ Wt, const double* __restrict__ alpha,
                                                     const double* __restrict__ yT, int N, int Np, double* __restrict__ mu_loo,
                                                     double* __restrict__ var_loo) {
    const int d = blockIdx.y, lane = threadIdx.x & 63, j = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    const int i = j + (Np - N);
    const double* row = Wt + ((size_t)d * Np + i) * Np;
    double s = 0.0;
    for (int k = i + lane; k < Np; k += 64) s += row[k] * row[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if (var_loo) var_loo[(size_t)d * N + j] = 1.0 / s;
        if (mu_loo) mu_loo[(size_t)d * N + j] = yT[(size_t)d * Np + i] - alpha[(size_t)d * Np + i] / s;
    }
}

int sr_launch_remove_rownorm(const double* Wt, int Np, int q, int n_out, double* coef, const double* Z, double* zstash, long zcount,
                             long zfrom, hipStream_t s) {
    const int nz = (int)((zcount + SR_RM_NORM_T - 1) / SR_RM_NORM_T);
    return sr_launch(sr_remove_rownorm_kernel, dim3(n_out + nz), dim3(SR_RM_NORM_T), 0, s, Wt, Np, q, n_out, coef, Z, zstash, zcount,
                     zfrom);
}

int sr_launch_remove_compact(const double* yT0, int Np0, int N0, int q, double* yT1, double* alpha1, int Np1, int n_out,
                             const double* zstash, double* Z, long zcount, long zto, hipStream_t s) {
    const long n = std::max((long)n_out * Np1, zcount);
    return sr_launch(sr_remove_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, yT0, Np0, N0, q, yT1, alpha1, Np1, n_out,
                     zstash, Z, zcount, zto);
}

int sr_launch_remove_rows(const double* Wt0, int Np0, int N0, int q, const double* alpha0, const double* coef, double* Wt1, int Np1,
                          double* alpha1, int n_out, hipStream_t s) {
    const int per_wg = SR_RM_WAVES * SR_RM_ROWS;
    const dim3 grid((N0 + per_wg - 1) / per_wg, n_out), block(64 * SR_RM_WAVES);
    if (reinterpret_cast<uintptr_t>(Wt0) % 32 == 0)
        return sr_launch(sr_remove_rows_kernel<true>, grid, block, 0, s, Wt0, Np0, Np0 - N0, q, alpha0, coef, Wt1, Np1, alpha1);
    return sr_launch(sr_remove_rows_kernel<false>, grid, block, 0, s, Wt0, Np0, Np0 - N0, q, alpha0, coef, Wt1, Np1, alpha1);
}

int sr_launch_remove_clean(double* Wt, double* alpha, double* yT, int Np, int n_out, int slide, long wt_slack, long vec_slack,
                           hipStream_t s) {
    const long n = std::max((long)n_out * Np * slide, wt_slack);
    return sr_launch(sr_remove_clean_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wt, alpha, yT, Np, n_out, slide, wt_slack,
                     vec_slack);
}

int sr_launch_loo(const double* Wt, const double* alpha, const double* yT, int N, int Np, int n_out, double* mu_loo, double* var_loo,
                  hipStream_t s) {
    return sr_launch(sr_loo_kernel, dim3((N + 3) / 4, n_out), dim3(256), 0, s, Wt, alpha, yT, N, Np, mu_loo, var_loo);
}
