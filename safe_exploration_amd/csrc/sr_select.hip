// sr_select.hip -- greedy max-variance subset (choose_datapoints_maxvar) by pivoted Cholesky downdates: sr_gp_select_maxvar.
//
// With the hyper-parameters fixed, "add the pool row of largest sum_d var_d(x | rows chosen so far)" is pivoted Cholesky on
// K_pool + sigma_d^2 I (sigma_d^2 = the handle's noise[d]).  Round r with pivot j = j_r:
//   c_d(x)    = k_d(x, x_j) - sum_{p<r} L_d(x, p) L_d(j, p)
//   s_d       = sqrt(var_d(j) + sigma_d^2)
//   L_d(x, r) = c_d(x) / s_d,   var_d(x) -= L_d(x, r)^2            (var_d starts at k_d(x, x))
//   score(x)  = sum_d max(var_d(x), 1e-15), d ascending, rows taken so far masked  ->  next pivot = first argmax
// A round streams n r n_out doubles of L instead of the O(n r^2) triangular contraction of a posterior pass, and nothing
// goes back to the host between rounds: each workgroup leaves its (score, row) partial, and the next round's launch begins
// by reducing all of them -- redundantly in every workgroup, in a fixed order, ties to the smaller row -- to its pivot.
//
// Launches: one per round 0 .. m-2 (the seeds first, in their order; round 0 also writes var = k(x, x) and the taken
// marks), then one single-workgroup launch that settles the last pick.  Nothing is read or written across workgroups
// inside one launch: the pivot row's L and var are read by everyone and written by no one (a taken row is never updated),
// a row's var / L / taken mark belong to the workgroup of that row.
#include "sr_handle.h"
#include "sr_kernel_dev.h"
#include <climits>
using namespace srh;

#define SR_SEL_ROWS 64        // pool rows per workgroup: one per lane
#define SR_SEL_WAVES 4        // wavefronts per workgroup: wave w sums entries [64 w, 64 w + 64) of every pivot-row tile
#define SR_SEL_PT 256         // pivot-row entries staged in LDS at a time (one per thread)
#define SR_SEL_MAX_OUT 64     // outputs of a handle (sr_gp_create)

struct sr_sel_args {
    const double* X;                  // pool, n x D
    int n, npad, D, n_out, general;
    const double* ls; const double* sf2;    // ARD-RBF (general == 0)
    const double* kp;                       // general family: n_out x SR_KP(D)
    const double* noise;                    // n_out: sigma_n^2 + noise_diag + jitter, as on the Gram diagonal
    const int* seeds; int k;
    double* L; long sL;               // L_d(x, p) at L[d sL + p npad + x]
    double* var;                      // n_out x npad
    int* taken;                       // npad
    double* pscore; int* pidx; int nwg;     // 2 x nwg partials (round parity)
    int* idx; double* score;          // the caller's outputs (score may be NULL)
};

// k_d(xi, xj) in the form the model update's Gram kernels give it (sr_gram_kernel: scaled coordinates, then the
// difference; sr_gram_general_kernel: the packed family); diag = the diagonal entry's form
__device__ __forceinline__ double sel_kernel(const sr_sel_args& a, int d, const double* xi, const double* xj, bool diag) {
    const int D = a.D;
    if (!a.general) {
        if (diag) return a.sf2[d];
        const double* ls = a.ls + (long)d * D;
        double r2 = 0.0;
        for (int c = 0; c < D; ++c) {
            const double il = 1.0 / ls[c];
            const double t = xi[c] * il - xj[c] * il;
            r2 = fma(t, t, r2);
        }
        return a.sf2[d] * exp(-0.5 * r2);
    }
    return sr_kpair(sr_kview(a.kp + (long)d * SR_KP(D), D), D, xi, xj, diag);
}

__device__ __forceinline__ double sel_clip(double v) { return (v > SR_VAR_CLIP) ? v : SR_VAR_CLIP; }   // as sr_finalize

// (s1, i1) before (s2, i2): larger score, then smaller row (np.argmax / torch.argmax).  A total order on distinct rows: the
// maximum does not depend on the order of the comparisons.
__device__ __forceinline__ bool sel_better(double s1, int i1, double s2, int i2) {
    return s1 > s2 || (s1 == s2 && i1 < i2);
}

__device__ __forceinline__ void sel_wave_argmax(double& s, int& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double s2 = __shfl_xor(s, o);
        const int i2 = __shfl_xor(i, o);
        if (sel_better(s2, i2, s, i)) { s = s2; i = i2; }
    }
}

// pivot of round r: seed r, or the first argmax over the partials round r - 1 left.  Every thread of the workgroup calls
// it (block-uniform branch) and gets the same row.
__device__ __forceinline__ int sel_pivot(const sr_sel_args& a, int r, double* red_s, int* red_i) {
    if (r < a.k) return a.seeds[r];
    const int tid = threadIdx.x;
    const double* ps = a.pscore + (long)((r - 1) & 1) * a.nwg;
    const int* pi = a.pidx + (long)((r - 1) & 1) * a.nwg;
    double s = -__builtin_huge_val();
    int i = INT_MAX;
    for (int w = tid; w < a.nwg; w += 256)
        if (sel_better(ps[w], pi[w], s, i)) { s = ps[w]; i = pi[w]; }
    sel_wave_argmax(s, i);
    if ((tid & 63) == 0) { red_s[tid >> 6] = s; red_i[tid >> 6] = i; }
    __syncthreads();
    s = red_s[0];
    i = red_i[0];
    for (int w = 1; w < SR_SEL_WAVES; ++w)
        if (sel_better(red_s[w], red_i[w], s, i)) { s = red_s[w]; i = red_i[w]; }
    return (i >= 0 && i < a.n) ? i : 0;      // (an untaken real row always exists while k <= m <= n: never the fallback)
}

// one round: downdate every untaken row by pivot j_r, write column r of L, score, leave this workgroup's partial
__global__ __launch_bounds__(256) void sr_select_round_kernel(sr_sel_args a, int r) {
    __shared__ double prow[SR_SEL_PT];
    __shared__ double dots[SR_SEL_WAVES - 1][SR_SEL_ROWS];
    __shared__ double xj[SR_MAX_D];
    __shared__ double sj[SR_SEL_MAX_OUT], vj[SR_SEL_MAX_OUT];
    __shared__ double red_s[SR_SEL_WAVES];
    __shared__ int red_i[SR_SEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int D = a.D, n_out = a.n_out;
    const long npad = a.npad;
    const int j = sel_pivot(a, r, red_s, red_i);
    if (tid < D) xj[tid] = a.X[(long)j * D + tid];
    __syncthreads();
    if (tid < n_out) {
        const double v = (r == 0) ? sel_kernel(a, tid, a.X + (long)j * D, xj, true) : a.var[(long)tid * npad + j];
        vj[tid] = v;
        sj[tid] = sqrt(v + a.noise[tid]);
    }
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) {
        double sc = 0.0;
        for (int d = 0; d < n_out; ++d) sc += sel_clip(vj[d]);
        a.idx[r] = j;
        if (a.score) a.score[r] = sc;
    }
    const int x = blockIdx.x * SR_SEL_ROWS + lane;               // < npad: L, var and taken have room for every x
    const double* xi = a.X + (long)(x < a.n ? x : a.n - 1) * D;  // (a padding row computes on a real row's coordinates; discarded)
    const bool live = x < a.n && x != j && (r == 0 || a.taken[x] == 0);
    double score = 0.0;
    for (int d = 0; d < n_out; ++d) {
        double* Ld = a.L + (long)d * a.sL;
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        for (int p0 = 0; p0 < r; p0 += SR_SEL_PT) {
            __syncthreads();                                     // the previous tile has been read
            if (p0 + tid < r) prow[tid] = Ld[(long)(p0 + tid) * npad + j];
            __syncthreads();
            const int q1 = min(64 * w + 64, r - p0);
            int q = 64 * w;
            const double* col = Ld + (long)(p0 + q) * npad + x;
            for (; q + 8 <= q1; q += 8, col += 8 * npad) {       // eight loads in flight per lane
                const double v0 = col[0], v1 = col[npad], v2 = col[2 * npad], v3 = col[3 * npad];
                const double v4 = col[4 * npad], v5 = col[5 * npad], v6 = col[6 * npad], v7 = col[7 * npad];
                acc0 = fma(v0, prow[q], acc0);
                acc1 = fma(v1, prow[q + 1], acc1);
                acc2 = fma(v2, prow[q + 2], acc2);
                acc3 = fma(v3, prow[q + 3], acc3);
                acc0 = fma(v4, prow[q + 4], acc0);
                acc1 = fma(v5, prow[q + 5], acc1);
                acc2 = fma(v6, prow[q + 6], acc2);
                acc3 = fma(v7, prow[q + 7], acc3);
            }
            for (; q < q1; ++q, col += npad) acc0 = fma(col[0], prow[q], acc0);
        }
        const double dot = (acc0 + acc1) + (acc2 + acc3);
        if (w > 0) dots[w - 1][lane] = dot;
        __syncthreads();
        if (w == 0) {
            const double sum = ((dot + dots[0][lane]) + dots[1][lane]) + dots[2][lane];
            const double c = sel_kernel(a, d, xi, xj, false) - sum;
            const double l = c / sj[d];
            const long o = (long)d * npad + x;
            const double v = ((r == 0) ? sel_kernel(a, d, xi, xi, true) : a.var[o]) - l * l;
            if (live) {
                Ld[(long)r * npad + x] = l;
                a.var[o] = v;
            }
            score += sel_clip(v);
        }
        __syncthreads();                                         // dots[] is free again
    }
    if (w == 0) {
        if (r == 0) a.taken[x] = (x == j);
        else if (x == j) a.taken[x] = 1;
        double s = live ? score : -__builtin_huge_val();
        int i = x;
        sel_wave_argmax(s, i);
        if (lane == 0) {
            a.pscore[(long)(r & 1) * a.nwg + blockIdx.x] = s;
            a.pidx[(long)(r & 1) * a.nwg + blockIdx.x] = i;
        }
    }
}

// the last pick (round m - 1): no downdate behind it, only its row and score
__global__ __launch_bounds__(256) void sr_select_last_kernel(sr_sel_args a, int r) {
    __shared__ double red_s[SR_SEL_WAVES];
    __shared__ int red_i[SR_SEL_WAVES];
    const int j = sel_pivot(a, r, red_s, red_i);
    if (threadIdx.x == 0) {
        const double* xj = a.X + (long)j * a.D;
        double sc = 0.0;
        for (int d = 0; d < a.n_out; ++d)
            sc += sel_clip((r == 0) ? sel_kernel(a, d, xj, xj, true) : a.var[(long)d * a.npad + j]);
        a.idx[r] = j;
        if (a.score) a.score[r] = sc;
    }
}

extern "C" int sr_gp_select_maxvar(sr_gp_t h, const double* X, long n, int m, const int* init_idx, int k, int* idx,
                                   double* score, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_select_maxvar: NULL handle");
    SR_CHECK(X && init_idx && idx, SR_EINVAL, "sr_gp_select_maxvar: NULL argument");
    SR_CHECK(k >= 1 && k <= m && (long)m <= n, SR_EINVAL, "sr_gp_select_maxvar: need 1 <= k <= m <= n (k=%d, m=%d, n=%ld)",
             k, m, n);
    SR_CHECK(n <= (long)INT_MAX - SR_SEL_ROWS, SR_EINVAL, "sr_gp_select_maxvar: n=%ld rows", n);
    SR_CHECK(h->have_data, SR_ESTATE, "sr_gp_select_maxvar: call sr_gp_set_data first (kernel and noise)");
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    // the seeds are checked on the host: one small read-back before the first launch
    std::vector<int> seeds(k);
    SR_HIP(hipMemcpyAsync(seeds.data(), init_idx, sizeof(int) * k, hipMemcpyDeviceToHost, s));
    SR_HIP(hipStreamSynchronize(s));
    std::sort(seeds.begin(), seeds.end());
    for (int i = 0; i < k; ++i)
        SR_CHECK(seeds[i] >= 0 && seeds[i] < n && (i == 0 || seeds[i] != seeds[i - 1]), SR_EINVAL,
                 "sr_gp_select_maxvar: init_idx must hold %d distinct rows in [0, %ld)", k, n);
    const int npad = (int)round_up(n, SR_SEL_ROWS), nwg = npad / SR_SEL_ROWS;
    const long mcap = std::max(m - 1, 1);
    const long nvar = (long)h->n_out * npad;
    // L (n_out x (m - 1) x npad doubles) and [var | partial scores | partial rows | taken]; earlier selections on this
    // stream may still read the old blocks
    SR_TRY(h->sel_L.grow((size_t)h->n_out * mcap * npad, wait::stream(s)));
    SR_TRY(h->sel_ws.grow((size_t)(nvar + 2L * nwg + (2L * nwg + npad + 1) / 2), wait::stream(s)));
    sr_sel_args a;
    a.X = X; a.n = (int)n; a.npad = npad; a.D = h->D; a.n_out = h->n_out; a.general = h->general;
    a.ls = h->ls; a.sf2 = h->sf2; a.kp = h->general ? h->kp : nullptr; a.noise = h->noise;
    a.seeds = init_idx; a.k = k;
    a.L = h->sel_L.get(); a.sL = mcap * npad;
    a.var = h->sel_ws.get();
    a.pscore = a.var + nvar;
    a.pidx = (int*)(a.var + nvar + 2L * nwg);
    a.taken = a.pidx + 2L * nwg;
    a.nwg = nwg;
    a.idx = idx; a.score = score;
    for (int r = 0; r + 1 < m; ++r)
        hipLaunchKernelGGL(sr_select_round_kernel, dim3(nwg), dim3(256), 0, s, a, r);
    hipLaunchKernelGGL(sr_select_last_kernel, dim3(1), dim3(256), 0, s, a, m - 1);
    SR_HIP(hipGetLastError());
    return SR_OK;
}
