// sr_paths_rollout.hip -- the closed-loop roll-out of the posterior function samples in ONE launch (sr_gp_paths_rollout; the
// C-ABI: include/safereach.h, the checks: sr_capi_paths.hip, the per-step kernels it stands beside: sr_paths.hip KPT / KPR).
//
//   KPO sr_paths_rollout_kernel : a workgroup owns P consecutive paths for all H steps.  Path s at step i + 1 depends on path
//                                 s at step i alone, so nothing crosses a workgroup: the only synchronisation is
//                                 __syncthreads(), every loop is bounded by H, N, M, and no result depends on how many
//                                 workgroups are resident.                                                  [exp / cos bound]
// Threads are (slot, path) with the path index fastest -- c and w are k-major with the path index fastest, so the P lanes of a
// slot read one P x 8 byte segment per term -- and a slot is (output d, split g) with G = (threads / P) / n_out splits per output.
// A tile of Z rows (one copy per output, divided by that output's lengthscales as KPT stages them) resp. of omega / tau rows
// goes through LDS; split g takes the rows g, g + G, .. of every tile, in that order.  Per step: the partial sums of every
// thread into LDS, the splits added in ascending order (no atomics: the same inputs give the same bits, and the first h steps
// of a longer roll-out are the h-step roll-out), X_all[i], the row of A_all[i] = J_x + J_u k_fb[i], the next controls.
// The formulas per term, their scalings and the prefactors at the end are those of KPT<GRAD>; the value's operations are the
// same in both forms (X_all with A_all is X_all without, bit for bit).
#include "sr_common.h"
#include "sr_kernel_dev.h"

#define SR_ROLL_ZT 64                /* Z rows per tile (n_out copies of each in LDS) */

template <int DT, bool GRAD, int P, int NT>
__global__ __launch_bounds__(NT) void sr_paths_rollout_kernel(sr_paths_rollout_args a) {
    constexpr int ZT = SR_ROLL_ZT, SLOTS = NT / P;
    constexpr int RS = DT | 1;                           // row stride in LDS: odd, so that the rows of a wave's slots miss each other's banks
    constexpr int NR = GRAD ? 1 + DT : 1;                // sums per (output, split): the value, then D derivatives
    constexpr int NROWS = (DT - 1) * ZT > NT ? (DT - 1) * ZT : NT;
    static_assert(SLOTS >= 16 && NT % ZT == 0, "a slot per output and per input column");
    __shared__ double rows[NROWS * RS];
    __shared__ double ta[NT];
    __shared__ double red[SLOTS * NR * P];               // [slot][row][path]
    __shared__ double sum[(DT - 1) * NR * P];            // [output][row][path]
    __shared__ double xst[DT * P];                       // [input column][path]: the inputs of the step
    __shared__ double lsv[(DT - 1) * DT], invl[(DT - 1) * DT];
    const int tid = threadIdx.x, p = tid % P, slot = tid / P;
    const int n_out = a.m.n_out, D = a.m.D, n_u = D - n_out, M = a.m.M, N = a.N;
    const int G = SLOTS / n_out;                         // n_out <= 7 < SLOTS
    const bool work = slot < n_out * G;
    const int d = work ? slot / G : 0, g = slot - (slot / G) * G;
    const int s = blockIdx.x * P + p;                    // (< Sp: P divides the padding of the coefficients' path index)
    const bool live = s < a.S;
    const int off = a.Np - N;

    for (int e = tid; e < n_out * D; e += NT) {
        lsv[e] = a.m.ls[e];
        invl[e] = 1.0 / a.m.ls[e];
    }
    if (slot < n_out) xst[slot * P + p] = live ? a.x0[(a.x0_per_path ? (long)s * n_out : 0) + slot] : 0.0;
    __syncthreads();
    // the controls of step i as KPR forms them: u_q = k_ff[i][q] + sum_c k_fb[i][q][c] x_c, one thread per (path, q)
    auto controls = [&](int i) {
        if (slot >= n_out && slot < D) {
            const int q = slot - n_out;
            const double* kb = a.k_fb + ((long)i * n_u + q) * n_out;
            double u = a.k_ff[(long)i * n_u + q];
            for (int c = 0; c < n_out; ++c) u = fma(kb[c], xst[c * P + p], u);
            xst[slot * P + p] = u;
        }
    };
    controls(0);
    __syncthreads();

    const double sf2 = a.m.sf2[d], amp = sqrt(2.0 * sf2 / (double)M);
    const double* cc = a.C + ((long)d * a.Np + off) * a.Sp + s;
    const double* ww = a.Wk + (long)d * a.m.Mp * a.Sp + s;
    for (int i = 0; i < a.H; ++i) {
        double xs[DT], xf[DT];                           // x / l as the kernel range resp. the feature range of KPT forms it
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            const double xv = (j < D) ? xst[j * P + p] : 0.0;
            xs[j] = (j < D) ? xv * invl[d * D + j] : 0.0;
            xf[j] = (j < D) ? xv / lsv[d * D + j] : 0.0;
        }
        // training rows: sum_i exp(-r2 / 2) c_i, times sf2 at the end
        double acck = 0.0, accf = 0.0;
        double gk[GRAD ? DT : 1], gf[GRAD ? DT : 1];
        if (GRAD) {
#pragma unroll
            for (int j = 0; j < DT; ++j) gk[j] = gf[j] = 0.0;
        }
        for (int i0 = 0; i0 < N; i0 += ZT) {
            const int nrow = min(ZT, N - i0);
            __syncthreads();
            {
                const int r = tid / (NT / ZT);
                if (r < nrow)
                    for (int j = tid % (NT / ZT); j < DT; j += NT / ZT) {
                        const double z = (j < D) ? a.Z[(long)(i0 + r) * D + j] : 0.0;
                        for (int dd = 0; dd < n_out; ++dd) rows[(dd * ZT + r) * RS + j] = (j < D) ? z * invl[dd * D + j] : 0.0;
                    }
            }
            __syncthreads();
            if (!work) continue;
            const double* rw = rows + d * ZT * RS;
#pragma unroll 4
            for (int r = g; r < nrow; r += G) {
                double r2 = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    const double df = xs[j] - rw[r * RS + j];
                    r2 = fma(df, df, r2);
                }
                const double kap = sr_kappa(0, r2), ci = cc[(long)(i0 + r) * a.Sp];
                acck = fma(kap, ci, acck);
                if (GRAD) {
                    const double kc = kap * ci;
#pragma unroll
                    for (int j = 0; j < DT; ++j) gk[j] = fma(kc, rw[r * RS + j] - xs[j], gk[j]);
                }
            }
        }
        // features: sum_i cos(omega_i . (x / l) + tau_i) w_i, times sqrt(2 sf2 / M) at the end
        for (int i0 = 0; i0 < M; i0 += NT) {
            const int nrow = min(NT, M - i0);
            __syncthreads();
            if (tid < nrow) {
#pragma unroll
                for (int j = 0; j < DT; ++j) rows[tid * RS + j] = (j < D) ? a.m.omega[(long)(i0 + tid) * D + j] : 0.0;
                ta[tid] = a.m.tau[i0 + tid];
            }
            __syncthreads();
            if (!work) continue;
#pragma unroll 4
            for (int r = g; r < nrow; r += G) {
                double arg = 0.0;
#pragma unroll
                for (int j = 0; j < DT; ++j) arg = fma(rows[r * RS + j], xf[j], arg);
                const double wi = ww[(long)(i0 + r) * a.Sp];
                accf = fma(cos(arg + ta[r]), wi, accf);
                if (GRAD) {                              // (cos stays the value's cos: sin is taken on its own)
                    const double sw = sin(arg + ta[r]) * wi;
#pragma unroll
                    for (int j = 0; j < DT; ++j) gf[j] = fma(sw, rows[r * RS + j], gf[j]);
                }
            }
        }
        if (work) {
            red[(slot * NR) * P + p] = fma(sf2, acck, amp * accf);
            if (GRAD) {
#pragma unroll
                for (int j = 0; j < DT; ++j)
                    if (j < D) {
                        const double il = invl[d * D + j];
                        red[(slot * NR + 1 + j) * P + p] = fma(sf2 * il, gk[j], -(amp * il) * gf[j]);
                    }
            }
        }
        __syncthreads();
        // per (output, row, path) the splits in ascending order
        const int nk = GRAD ? 1 + D : 1;
        for (int rr = slot; rr < n_out * nk; rr += SLOTS) {
            const int dd = rr / nk, k = rr - dd * nk;
            double v = 0.0;
            for (int gg = 0; gg < G; ++gg) v += red[((dd * G + gg) * NR + k) * P + p];
            sum[(dd * NR + k) * P + p] = v;
        }
        __syncthreads();
        if (slot < n_out) {
            const double f = sum[(slot * NR) * P + p];
            xst[slot * P + p] = f;
            if (live) a.X_all[((long)i * a.S + s) * n_out + slot] = f;
            if (GRAD && live) {                          // row `slot` of A_all[i][s] = J_x + J_u k_fb[i]
                const double* kb = a.k_fb + (long)i * n_u * n_out;
                double* A = a.A_all + (((long)i * a.S + s) * n_out + slot) * n_out;
                for (int c = 0; c < n_out; ++c) {
                    double v = sum[(slot * NR + 1 + c) * P + p];
                    for (int q = 0; q < n_u; ++q) v = fma(sum[(slot * NR + 1 + n_out + q) * P + p], kb[q * n_out + c], v);
                    A[c] = v;
                }
            }
        }
        __syncthreads();
        if (i + 1 < a.H) controls(i + 1);
        __syncthreads();
    }
}

// paths per workgroup: 256 workgroups of 4 paths at S = 1024 (what was measured).  The threads of a
// workgroup are also the omega rows of a tile.
#define SR_ROLL_P 4

int sr_launch_paths_rollout(const sr_paths_rollout_args& a, hipStream_t s) {
    const int n_u = a.m.D - a.m.n_out;
    SR_CHECK(a.S >= 1 && a.S <= a.Sp && a.H >= 1 && n_u >= 1 && a.m.D <= SR_PATHS_MAX_D && a.N >= 1 && a.m.M >= 1, SR_EINVAL,
             "paths_rollout: S=%d Sp=%d H=%d D=%d n_out=%d", a.S, a.Sp, a.H, a.m.D, a.m.n_out);
    const int P = (int)sr_lab_env("SR_ROLLOUT_PATHS", SR_ROLL_P);
    return sr_pick_le<3, 5, 8>("paths_rollout", a.m.D, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        auto go = [&](auto pp, auto nt) {
            constexpr int P_ = decltype(pp)::value, NT_ = decltype(nt)::value;
            const dim3 grid((a.S + P_ - 1) / P_);
            if (a.A_all) return sr_launch(sr_paths_rollout_kernel<DT, true, P_, NT_>, grid, dim3(NT_), 0, s, a);
            return sr_launch(sr_paths_rollout_kernel<DT, false, P_, NT_>, grid, dim3(NT_), 0, s, a);
        };
        // 512 threads (two waves per SIMD) where the LDS of the widest form allows it; a bucket's two forms share the count,
        // so that they split the terms alike
        using nt = std::integral_constant<int, DT <= 5 ? 512 : 256>;
#ifdef SR_LAB                                            // SR_ROLLOUT_PATHS: P at 256 threads; 4256 / 8512: P and the threads
        using nt256 = std::integral_constant<int, 256>;
        if (P == 2) return go(std::integral_constant<int, 2>{}, nt256{});
        if (P == 8) return go(std::integral_constant<int, 8>{}, nt256{});
        if (P == 16) return go(std::integral_constant<int, 16>{}, nt256{});
        if (P == 4256) return go(std::integral_constant<int, 4>{}, nt256{});
        if (P == 8512) return go(std::integral_constant<int, 8>{}, nt{});
#endif
        (void)P;
        return go(std::integral_constant<int, SR_ROLL_P>{}, nt{}); });
}
