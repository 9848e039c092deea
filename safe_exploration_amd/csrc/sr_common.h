// sr_common.h -- shared declarations for libsafereach (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <cstring>
#include <vector>
#include "../../include/safereach.h"

#define SR_NB 128          // factor block size == GEMM tile edge; Np is a multiple of it
#define SR_PANEL 4         // factor blocks per Cholesky panel (deferred trailing update with K = 512)
#define SR_MAX_NS 8
#define SR_MAX_DEVICES 64    // per-device tables of the host side (locks)
#define SR_FACT_SLOTS 8      // outputs factorised concurrently (own streams + scratch each)
#define SR_MAX_NU 4
#define SR_MAX_D 12
#define SR_VAR_CLIP 1e-15  // GPy GP._raw_predict clips the predictive variance here

void sr_set_error(const char* fmt, ...);

// Measurement switches exist in the LAB build only (make lab: scripts/_bin/libsafereach_lab.so, -DSR_LAB; the scripts that
// sweep them load it through SAFEREACH_LIB).  In the product every one of them is its default, at compile time: the
// library reads no environment variable except the three allocator diagnostics of sr_capi_handle.hip.
#include <cstdlib>
#ifdef SR_LAB
static inline const char* sr_lab_str(const char* name) { return getenv(name); }
#else
static inline constexpr const char* sr_lab_str(const char*) { return nullptr; }
#endif
static inline long sr_lab_env(const char* name, long dflt) { const char* v = sr_lab_str(name); return v ? atol(v) : dflt; }
static inline double sr_lab_envf(const char* name, double dflt) { const char* v = sr_lab_str(name); return v ? atof(v) : dflt; }
static inline bool sr_lab_on(const char* name) { return sr_lab_str(name) != nullptr; }

#define SR_HIP(call)                                                                  \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            sr_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            return SR_EHIP;                                                           \
        }                                                                             \
    } while (0)

#define SR_CHECK(cond, code, ...)                                                     \
    do {                                                                              \
        if (!(cond)) { sr_set_error(__VA_ARGS__); return (code); }                    \
    } while (0)

#define SR_TRY(expr)                                                                  \
    do { int rc_ = (expr); if (rc_ != SR_OK) return rc_; } while (0)

#include "sr_dispatch.h"   // sr_width_bucket, sr_pick_le / _eq / _np, sr_launch (uses SR_HIP)

typedef double d4_t __attribute__((ext_vector_type(4)));

struct sr_prof_rec { int id; hipEvent_t e0, e1; };
struct sr_prof {
    int enabled = 0;
    double ms[SR_K_COUNT] = {0};
    long launches[SR_K_COUNT] = {0};
    std::vector<hipEvent_t> pool;        // recycled events
    std::vector<sr_prof_rec> pending;    // recorded, not yet resolved
    hipEvent_t take() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    // wait for every recorded pair and fold the elapsed times into ms[] / launches[]
    void resolve() {
        for (auto& r : pending) {
            float t = 0.f;
            if (r.e0 && r.e1 && hipEventSynchronize(r.e1) == hipSuccess &&
                hipEventElapsedTime(&t, r.e0, r.e1) == hipSuccess) {
                ms[r.id] += t;
                launches[r.id] += 1;
            }
            if (r.e0) pool.push_back(r.e0);
            if (r.e1) pool.push_back(r.e1);
        }
        pending.clear();
    }
    void destroy() {
        resolve();
        for (auto e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
};

// Optional per-launch timing: a hipEvent pair recorded on the launch stream around one kernel.
// Nothing synchronises at launch time; pairs are resolved lazily by sr_prof_get / sr_prof_reset.
struct sr_prof_scope {
    sr_prof* p; sr_prof_rec r;
    sr_prof_scope(sr_prof* p_, int id_, hipStream_t s_) : p(p_), s(s_) {
        r.id = id_; r.e0 = r.e1 = nullptr;
        if (p && p->enabled) {
            if (p->pending.size() >= 8192) p->resolve();
            r.e0 = p->take();
            if (r.e0) (void)hipEventRecord(r.e0, s);
        }
    }
    ~sr_prof_scope() {
        if (p && p->enabled) {
            r.e1 = p->take();
            if (r.e1) (void)hipEventRecord(r.e1, s);
            p->pending.push_back(r);
        }
    }
    hipStream_t s;
};

// ---- launchers implemented in the .hip files ---------------------------------------------------
// C[m][n] (op)= alpha * sum_k A[k][m] * B[k][n]; A: K x M (lda), B: K x N (ldb), C: M x N (ldc).
// M, N multiples of 128; K multiple of 16.
//   mode 0: all tiles.  mode 1: only tiles with n0 >= m0 (upper block triangle).
//   mode 2: B block-lower-triangular (B[k][n] == 0 for k < n0): per tile k starts at n0.
//   mode 4: A block-lower-triangular (A[k][m] == 0 for k < m0): per tile k starts at m0.
//   mode 3: A block-upper-triangular (A[k][m] == 0 for k >= m0 + 128): per tile k ends at m0 + 128.
// prio != 0: the workgroups raise their wavefront priority (critical-path products that share CUs with bulk work)
// Batch of independent, equally shaped problems in ONE launch (the outputs of a model: the same product on n operand
// sets `stride` doubles apart): every launcher below takes an optional sr_batch; n = 1 / NULL = the plain call.
struct sr_batch { int n = 1; long sA = 0, sB = 0, sC = 0, sCT = 0; };
int sr_launch_gemm_tn(const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                      int M, int N, int K, double alpha, double beta, int mode, hipStream_t s, int prio = 0,
                      const sr_batch* bt = nullptr);

// upper block triangle only (tiles n0 >= m0; M <= N) on a linear grid -- the trailing updates of the Cholesky
int sr_launch_gemm_tn_upper(const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                            int M, int N, int K, double alpha, double beta, hipStream_t s, int prio = 0,
                            int order = -1,    // order: 0 row-major tiles, 1 XCD-aware super-tiles, -1 by size
                            const sr_batch* bt = nullptr);
// thin products (N a few tiles, K long): K-slices of ks rows as grid.z into `part` (ceil(K / ks) x M x N doubles), then
// summed in order into C (M x N contiguous).  modes as sr_launch_gemm_tn.
int sr_launch_gemm_tn_splitk(const double* A, long lda, const double* B, long ldb, double* C, int M, int N, int K,
                             int ks, double alpha, int mode, double* part, hipStream_t s);
// a list of independent TN products in one launch (one level of the recursive triangular inversion):
// C_j = alpha A_j^T B_j, optionally also CT_j = C_j^T; operands at offsets (doubles) of common base pointers,
// common leading dimension.  mode 2 / 3 as above.
// struct sr_gemm_job { long a, b, c, ct; int M, N, K, pad; }: include/safereach.h (the test entry of the list takes it)
// tiles128: 128 x 128 tiles of the whole list (picks the workgroup tile)
int sr_launch_gemm_tn_jobs(const double* Ab, const double* Bb, double* Cb, double* CTb, long ld,
                           const sr_gemm_job* jobs_dev, int njobs, int maxM, int maxN, long tiles128, double alpha,
                           int mode, hipStream_t s, const sr_batch* bt = nullptr);

// padded index space: the Np - N padding rows/cols sit at the FRONT (identity), training point i lives
// at padded index i + (Np - N); the contraction kernels simply start at k = 16*floor((Np-N)/16).
// sf2_dev / noise_dev: device scalars that take precedence over the by-value arguments when not NULL
// nbatch > 1: outputs b = 0 .. nbatch-1 in one launch (ls + b D, sf2_dev + b, noise_dev + b, K + b strideK)
int sr_launch_gram(const double* Z, const double* ls, double sf2, double noise, const double* sf2_dev,
                   const double* noise_dev, double* K, int N, int Np, int D, hipStream_t s, int nbatch = 1,
                   long strideK = 0);
// factor the diagonal block kb of the Np x Np matrix A (upper), write U_kk in place, U_kk^-1 to
// wt_diag (into Wt's diagonal block) and U_kk^-T to w_diag (into W's diagonal block).
int sr_launch_append_move(const double* Wt0, int Np0, int off0, int N0, const double* U12t, const double* invS, int m,
                          double* Xt, double* Y2, double* Wt1, int Np1, int off1, hipStream_t s, int nbatch = 1,
                          long sXt = 0, long sY2 = 0);
int sr_launch_eye_front(double* W, int ld, int n, hipStream_t s, int nbatch = 1);
// G != NULL: factor A - G (rows / columns >= pf); nbatch blocks with strides sA (A) and sW (wt_diag), info_dev + b
int sr_launch_potrf_corner16(double* A, long lda, double* wt_diag, long ldw, int* info_dev, hipStream_t s,
                             const double* G = nullptr, int pf = 0, int nbatch = 1, long sA = 0, long sW = 0);
// bt: batch of blocks (sA: stride of A, sB: of wt_diag, sC: of w_diag; info_dev + b)
int sr_launch_potrf_diag(double* A, long lda, double* wt_diag, double* w_diag, long ldw,
                         int kb, int* info_dev, hipStream_t s, int skip = 0, const sr_batch* bt = nullptr);
// one-thread hand-over between streams: publish set_flag = set_v (NULL: nothing), then wait for *w0 >= v0 and *w1 >= v1
// (NULL: no wait); a wait longer than timeout_s sets *status = 1 and passes (sr_factor.hip)
int sr_launch_fact_handover(unsigned* set_flag, unsigned set_v, const unsigned* w0, unsigned v0, const unsigned* w1,
                            unsigned v1, unsigned* status, double timeout_s, hipStream_t s);
int sr_launch_transpose(const double* src, double* dst, int n, hipStream_t s);
int sr_launch_transpose_rect(const double* src, long lds_, double* dst, long ldd, int rows, int cols,
                             hipStream_t s);
// y[r] = sum_c M[r][c] x[c], c in [0..r] (lower=1) or [r..n) (lower=0)
// nbatch members, matrix / x / y sM / sx / sy doubles apart
int sr_launch_trmv(const double* M, long ld, const double* x, double* y, int n, int lower,
                   hipStream_t s, int nbatch = 1, long sM = 0, long sx = 0, long sy = 0);
long sr_mll_ws(int N);
int sr_launch_mll(const double* Kinv, int Np, int N, const double* alpha, const double* yT, const double* Z,
                  const double* kp, int D, const double* logdet, double* partial, double* nll, double* grad,
                  hipStream_t s);
int sr_launch_logdet(const double* Wt, int Np, int n_out, double* out, hipStream_t s);
// exact moment matching (sr_moment_match.hip): one chunk of T <= sr_mm_max_queries queries of an ARD-RBF model at Gaussian
// inputs N(m, S) (S NULL: points); ws: T x sr_mm_ws_per_query doubles (the D x D algebra per query and the partial sums)
long sr_mm_ws_per_query(int N, int D, int n_out);
long sr_mm_max_queries(int N, int n_out);
int sr_launch_moment_match(const double* Z, const double* alpha, const double* ls, const double* sf2, int N, int Np, int D,
                           int n_out, const double* m, const double* S, long T, const double* inv_k, double* mu,
                           double* cov, double* V, double* ws, hipStream_t s);
// its reverse pass: m_bar (T x D) and S_bar (T x D x D, exactly symmetric; either may be NULL) from the seeds mu_bar, cov_bar,
// V_bar (NULL = zero); one chunk of T <= sr_mmg_max_queries queries, ws: T x sr_mmg_ws_per_query doubles
long sr_mmg_ws_per_query(int N, int D, int n_out);
long sr_mmg_max_queries(int N, int n_out);
int sr_launch_moment_match_vjp(const double* Z, const double* alpha, const double* ls, const double* sf2, int N, int Np,
                               int D, int n_out, const double* m, const double* S, long T, const double* inv_k,
                               const double* mu_bar, const double* cov_bar, const double* V_bar, double* m_bar,
                               double* S_bar, double* ws, hipStream_t s);
// its two halves on their own (the same kernels, the same sums): everything that does not read the seeds -- the D x D records,
// mu, V and the O(N^2) sums of the pair kernel -- once for Tq <= sr_mmg_max_queries queries into ws (Tq x sr_mmg_ws_per_query
// doubles); then the seeds of the queries q0 .. q0 + T of that block (m: all Tq rows; seeds and results: the T rows of the slice)
int sr_launch_moment_match_vjp_records(const double* Z, const double* alpha, const double* ls, const double* sf2, int N,
                                       int Np, int D, int n_out, const double* m, const double* S, long Tq,
                                       const double* inv_k, double* ws, hipStream_t s);
int sr_launch_moment_match_vjp_seeded(const double* Z, const double* alpha, const double* ls, const double* sf2, int N,
                                      int Np, int D, int n_out, const double* m, long q0, long T, long Tq,
                                      const double* mu_bar, const double* cov_bar, const double* V_bar, double* m_bar,
                                      double* S_bar, double* ws, hipStream_t s);
double* sr_mmg_ws_mu(double* ws, long Tq, int D, int n_out);     // mu (Tq x n_out) and V (Tq x n_out x D) of the records half
double* sr_mmg_ws_v(double* ws, long Tq, int D, int n_out);
// the reverse pass of the closed-loop roll-out (sr_moment_match_rollout_vjp.hip): one group of Tg trajectories through H steps,
// Tg H <= sr_mmg_max_queries; ws: Tg x sr_mmrv_ws_per_traj doubles.  The pointers of the group's own rows; the scratch
// pointers (V .. carry_sig) are set by the launch.
struct sr_mmrv_args {
    const double *Z, *alpha, *ls, *sf2, *inv_k;      // the model as the handle holds it; n_s x N x N
    const double *mu0, *sigma0;                      // Tg x n_s; Tg x n_s x n_s | NULL (points)
    const double *k_ff, *k_fb;                       // [Tg x] H x n_u; [Tg x] (H - 1) x n_u x n_s | NULL (H == 1)
    const double *a, *b, *tz;                        // n_s x n_s, n_s x n_u, n_x_in x n_s | NULL (identity)
    const double *mu_all, *sigma_all;                // Tg x H x n_s, Tg x H x n_s x n_s: what the forward stored
    const double *mu_all_bar, *sigma_all_bar, *cov_all_bar;      // the seeds, shaped like the forward's outputs; NULL = zero
    double *mu0_bar, *sigma0_bar, *kff_bar, *kfb_bar;            // Tg x n_s, Tg x n_s x n_s | NULL, Tg x H x n_u, Tg x (H-1) x n_u x n_s | NULL
    const double* V;                                 // Q x n_s x D of the one-off pass, Q = H Tg queries, step-major
    double *m_z, *S_z;                               // Q x D, Q x D x D: the GP's inputs
    double *mu_bar, *cov_bar, *V_bar;                // Tg x n_s, Tg x n_s x n_s, Tg x n_s x D: the GP's seeds of one step
    double *mz_bar, *Sz_bar;                         // Tg x D, Tg x D x D: what the GP's reverse pass returns for them
    double *carry_mu, *carry_sig;                    // Tg x n_s, Tg x n_s x n_s: (mu_bar, Sigma_bar) handed to the step before
    int N, Np, D, n_s, n_x_in, H, gains_per_traj;
    long Tg;
};
#define SR_MMRV_MAX_NS 12                            // the sweep kernel keeps its n_s x n_s matrices in LDS at this size
long sr_mmrv_ws_per_traj(int N, int D, int n_s, int H);
int sr_launch_moment_match_rollout_vjp(sr_mmrv_args r, double* ws, hipStream_t s);
// the same for the general family with the RBF radial part on every output (sr_moment_match_gen.hip; kp n_out x SR_KP(D)):
// once per call the query-independent block `call` (sr_mmx_call_ws doubles), then chunks of T <= sr_mmx_max_queries queries
// with ws: T x sr_mmx_ws_per_query doubles
long sr_mmx_call_ws(int N, int D, int n_out);
long sr_mmx_ws_per_query(int N, int D, int n_out);
long sr_mmx_max_queries(int N, int n_out);
int sr_launch_moment_match_gen_call(const double* Z, const double* alpha, const double* kp, int N, int Np, int D, int n_out,
                                    const double* inv_k, double* call, hipStream_t s);
int sr_launch_moment_match_gen(const double* Z, const double* alpha, const double* kp, int N, int Np, int D, int n_out,
                               const double* m, const double* S, long T, const double* inv_k, double* mu, double* cov,
                               double* V, const double* call, double* ws, hipStream_t s);
// the closed-loop roll-out of T trajectories through H steps of exact moment matching in one launch
// (sr_moment_match_rollout.hip): one workgroup per trajectory; ws: T x sr_mmr_ws_per_traj doubles (the records of one step)
struct sr_mmr_args {
    const double *Z, *alpha, *ls, *sf2, *inv_k;      // the model as the handle holds it; n_out x N x N
    const double *mu0, *sigma0;                      // T x n_out; T x n_out x n_out | NULL (points)
    const double *k_ff, *k_fb;                       // [T x] H x n_u; [T x] (H - 1) x n_u x n_out | NULL (H == 1)
    const double *a, *b, *tz;                        // n_out x n_out, n_out x n_u, n_x_in x n_out | NULL (identity)
    double *mu_all, *sigma_all, *cov_all;            // T x H x n_out, T x H x n_out x n_out, the same | NULL
    double* ws;
    int N, Np, D, n_out, n_x_in, H, gains_per_traj;
    int stage_rec, stage_model;                      // set by the launch: the records resp. Z and alpha live in LDS
    long T;
};
long sr_mmr_ws_per_traj(int D, int n_out);
int sr_launch_moment_match_rollout(const sr_mmr_args& a, hipStream_t s);
int sr_launch_fill(double* p, size_t n, double v, hipStream_t s);
// Wt = J U^T J from the factor as the model update leaves it (diagonal 128-blocks in U, block rows in W; sr_sparse.hip);
// nbatch members, U / W sS and Wt sD doubles apart
int sr_launch_reversed_factor(const double* U, const double* W, double* Wt, int Np, hipStream_t s, int nbatch, long sS,
                              long sD);
int sr_launch_sub_block(double* S, const double* G, int pf, hipStream_t s);
int sr_launch_append_assemble(const double* Wt0, int Np0, int off0, int N0, const double* Y2,
                              const double* invS, int m, double* Wt1, int Np1, int off1, hipStream_t s);

// General kernel family (sr_kernel_dev.h), packed per output as SR_KP(D) doubles: [kappa id, v, c0, s[D], a[D], b[D]]
#define SR_KP(D) (3 + 3 * (D))
int sr_launch_gram_general(const double* Z, const double* kp, double noise, const double* noise_dev, double* K, int N,
                           int Np, int D, hipStream_t s, int nbatch = 1, long strideK = 0);

struct sr_kstar_args {
    const double* Z;        // N x D
    const double* alpha;    // n_out x Np
    const double* ls;       // n_out x D
    const double* sf2;      // n_out
    const double* xa; long lda; int na;   // query part a: T x na (row stride lda)
    const double* xb; long ldb; int nb;   // query part b: T x nb (row stride ldb), na+nb == D
    const double* kp;       // general kernels: n_out x SR_KP(D) packed parameters, else NULL (ARD-RBF fast path)
    double* kxx;            // general kernels: prior variance k(x_t, x_t), n_out x Tp
    double* Ks;             // n_out x Np x Tp
    double* mu_part;        // nsplit x n_out x Tp
    double* jac_part;       // nsplit x n_out x D x Tp
    int N, Np, D, n_out, nsplit;
    long T, Tp;
    // one-launch blocking single query (sr_gp_call1; K0 only): the query travels in the kernel arguments, the results
    // go straight to pinned host memory and the last workgroup writes the sequence number the host spins on
    long Tw = 0;            // width (padded queries) of THIS launch when it covers a column range of the buffers only;
                            // 0: all Tp columns.  Pointers (xa, xb, Ks, mu_part, jac_part, kxx) are then pre-offset.
    int xv_on = 0; double xv[SR_MAX_D] = {};
    unsigned* done_ticket = nullptr; unsigned long long* host_flag = nullptr; unsigned long long host_seq = 0;
};
int sr_launch_kstar(const sr_kstar_args& a, hipStream_t s);

// K0 (sr_small.hip): whole posterior of a small ARD-RBF model in one launch, outputs in the API layout
int sr_launch_gp_small(const sr_kstar_args& a, const double* Wt, double* mu, double* var, double* jac,
                       hipStream_t s);
int sr_launch_gp_small_lin(const sr_kstar_args& a, const double* Wt, double* mu, double* var, double* jac_mu,
                           double* jac_var, double* hess_mu, hipStream_t s);

// K0s (sr_server.hip): resident single-query server of a small ARD-RBF model: one workgroup per output polls a mailbox in
// pinned host memory.  All pointers are the DEVICE-visible addresses of pinned host memory.
struct sr_server_args {
    unsigned long long* mb;          // mailbox, ONE 64-byte line: [0 .. 4] x (D <= 5 doubles), [5] (launch epoch << 8) | command (any
                                     // other epoch: leave), [6] sequence number, [7] check word = [0] ^ .. ^ [6] ^ SR_SERVER_CHK
    double* out;                     // reply block: per (output d, part) one record of SR_SERVER_REC doubles
                                     // [mu, var or its share, d mu/dx (D), d var/dx or its shares (D), d2 mu/dx2 (D x D), .., sf2]
    unsigned long long* reply;       // [d]: sequence number last answered by output d; [SR_SERVER_ALIVE + d]: 1 while it runs;
                                     // [2 SR_SERVER_ALIVE + d]: device ticks (100 MHz) of the last evaluation
    unsigned long long first_seq;    // the first sequence number this launch answers
    unsigned long long epoch;        // of this launch (mb[5] holds it while the launch is wanted)
    unsigned long long idle_ticks;   // leave after this long without a request (100 MHz wall clock)
};
#define SR_SERVER_ALIVE 64           /* reply words: one per (output, part) */
#define SR_SERVER_REC 40          /* doubles per output record in the reply block (2 + 2 D + D^2 <= 37 for D <= 5) */
#define SR_SERVER_CHK 0x5afe5eedc0ffee11ull   /* the eight words of a consistent mailbox line xor to this */
#define SR_SERVER_CMD_FIRST 0ull     /* mu, var, d mu/dx */
#define SR_SERVER_CMD_SECOND 1ull    /* + d var/dx, d2 mu/dx2 */
#define SR_SERVER_CMD_STOP 2ull
#define SR_SERVER_CMD_IDLE 3ull      /* (device-internal: the idle time-out) */
#define SR_SERVER_CMD_PING 4ull      /* diagnostics: answer at once, evaluate nothing */
int sr_launch_gp_server(const sr_kstar_args& a, const double* Wt, const sr_server_args& sv, hipStream_t s);

// Persistent multi-step kernel (sr_chain.hip): the whole H-step chain of up to SR_CHAIN_GROUPS / (n_out Np / 128) * 16
// rollouts in ONE launch (the posterior of sr_gp_small_kernel and the step of sr_ellipsoid_kernel inside a loop over the steps).
struct sr_xel { double v; unsigned long long chk; };      // 16 bytes, written and read by single instructions; chk = bits(v) ^ mix(tag)
struct sr_chain_args {
    sr_kstar_args k;                  // model (Z, alpha, ls, sf2, N, Np, D, n_out, na = n_s, nb = n_u); queries unused
    const double* Wt;
    long T; int H; int mode;          // mode as in sr_ell_args
    const double* p0; const double* q0; const double* k_fb0;      // T x n_s, T x n_s^2 | NULL, T x n_u x n_s | NULL
    const double* k_ff; const double* k_fb;                       // T x H x n_u, T x (H-1) x n_u x n_s
    const double* a; const double* b; const double* l_mu; const double* l_sigma; double c_safety;
    double* p_all; double* q_all; double* gp_var_all;             // T x H x n_s, T x H x n_s^2, T x H x n_s | NULL
    int* n_bad;
    sr_xel* xch;                      // groups x H x n_out x (16 (D + 1) + 16 parts) tagged values: every step's results
                                      // of the n_out x Np / 128 posterior workgroups of a group of 16 rollouts (zeroed once)
    // per group: the last tag used so far (the tags of a launch are epoch + 1 .. epoch + H; written by the launch's last
    // workgroup to leave: nothing of the protocol lives on the host, so a captured launch can be replayed), workgroups
    // done, and the tag with which the group's tail workgroup (the shape matrices) reported for this launch
    unsigned long long* epoch; unsigned* done; unsigned long long* alive;
    // status word in PINNED HOST memory (device-visible address): a group whose hand-off did not complete within
    // SR_CHAIN_TIMEOUT_TICKS ORs 1 into it with a system-scope atomic (and poisons its outputs with NaN).  The host
    // reads it without a copy: after the stream has been synchronised it says whether this launch failed.
    int* status;
    int test_drop = 0;                // tests only: launch this many workgroups fewer than the chain needs
};
#define SR_CHAIN_GROUPS 240          /* workgroups of one launch: all must be resident (they wait for each other) */
#define SR_CHAIN_XELS (240ul * 112 * 96)      /* exchange elements (16 B): 240 posterior workgroups x 96 steps at most */
int sr_chain_wgs_per_group(int Np, int n_s);                    // posterior workgroups + the tail workgroup
long sr_chain_xels_per_group(int Np, int n_s, int n_u, int H);  // exchange elements one group of 16 rollouts needs
#define SR_CHAIN_TIMEOUT_TICKS 10000000ull   /* 100 ms of the 100 MHz wall clock (a step takes ~10 us) */
bool sr_chain_supported(int Np, int D, int n_s, int n_u, int H);
// workgroups of the chain kernel for this model that one CU can hold (hipOccupancyMaxActiveBlocksPerMultiprocessor of
// the instantiation the dispatcher would pick; 0 = it cannot run at all); H sizes the dynamic LDS
int sr_chain_blocks_per_cu(int Np, int n_s, int n_u, int H, int* blocks);
int sr_launch_chain(const sr_chain_args& a, hipStream_t s);

// part[d][rb][t] = sum_{i in row block rb} ( sum_k Wt[d][k][i] Ks[d][k][t] )^2
int sr_launch_var(const double* Wt, const double* Ks, double* part, int N, int Np, long Tp, int n_out,
                  int group, int variant, hipStream_t s, long Tw = 0);

// 64 x 64 tile variant for small models (sr_predict.hip, K2m): part layout [d][Np/64][Tp]
int sr_launch_var64(const double* Wt, const double* Ks, double* part, int N, int Np, long Tp, int n_out,
                    hipStream_t s);

// few query tiles: balanced shares of the k-blocks + a reduce pass (sr_predict.hip, K2b); workspace doubles; part layout
// [d][4 nrb][Tp]
long sr_var_bal_ws(int Np, long Tp, int n_out);
int sr_launch_var_bal(const double* Wt, const double* Ks, double* Vt, double* part, int N, int Np, long Tp, int n_out,
                      hipStream_t s);

// small-batch (T <= 16) variance path: U^-1 streamed once at HBM rate (sr_predict.hip, K2s)
#define SR_SMALL_T 16
#define SR_FUSED_T 1024        /* up to here a model with Np <= SR_FUSED_NP takes the one-launch pass of sr_small.hip */
#define SR_FUSED_NP 512
#ifndef SR_STREAM_MIN_NP
#define SR_STREAM_MIN_NP 384    /* T <= 16 streams U^-1 (K2s) above this padded size unless the one-launch pass K0 takes it */
#endif
#define SR_STREAM_MAX_T 64     /* up to here a batch beyond the one-launch sizes streams U^-1 once (sr_stream.hip) */
#define SR_FINAL_WAVE_T 4096   /* up to here sr_finalize runs one wavefront per (query, output) */

// ================================================================================================================
// DISPATCH TABLE -- every size threshold by which the host side picks a kernel, in one place, with the measurement that
// set it (profiles/<round>_<file>; "r1d" .. "r04" = the round that measured it, MI355X).  Np = padded training points
// (multiple of 128), T = queries of one call, Tp = T padded to 128, D = GP input dimension, nb = Np / 128.
//
//  posterior of ONE call (sr_capi_posterior.hip: gp_pass)
//   K0  one launch (sr_small.hip)            Np <= SR_FUSED_NP (512), T <= SR_FUSED_T (1024), D <= 8; not Np = 512 with
//                                            T <= 128 (streamed: 22-23 against 28 us, r02_latency_grid), not Np = 384 with T = 1
//                                            (SR_ONE_STREAMED_NP: 12.4 against 18.8 us, r02_latency_grid)
//   K2f streamed, fused (sr_stream.hip)      Np > SR_STREAM_MIN_NP (384), T <= SR_STREAM_MAX_T (64): N = 5000 T = 1 54 -> 37 us, T = 64
//                                            143 -> 111 us (r02 / r03_latency_grid); one launch for T <= 4 with D <= 5 unless
//                                            2 <= T <= 4 and Np <= SR_MFMA_SMALL_MAX_NP (2048): N = 700 27 against 21 us, N = 3000 34 / 40
//                                            no K* pass either for 16 columns per workgroup on one-chunk work items, nor for 32 up to
//                                            SR_STREAM_FUSED32_MAX_NCB (8) column blocks: T = 16 N = 2000 / 3000 28 / 39 -> 25 / 34 us (r04_latency_grid)
//   K2s streamed, groups of 16               T <= 16 x sr_var_small_groups_max (300 MB of re-read U^-1): N = 700 T = 128 41 -> 25 us,
//                                            N = 2000 71 -> 40 us, from N = 3000 on the tiles win (r01d_latency_grid)
//   K2b balanced shares (sr_predict.hip)     sr_var_splitk_wanted (nb > 2, <= 1024 plain workgroups): one workgroup per cell below
//                                            256 cells, 256 workgroups up to 8192 cells, 512 beyond (r05_bal_ab); the chunked
//                                            split-K route K2k of rounds 1 - 4 and the XCD slabs K2x of round 4 are gone
//   K2m 64 x 64 tiles                        sr_var64_wanted: Np <= 1024 and < 256 plain workgroups (N = 200: 60 -> 31-37 us, r01d)
//   K2  plain 128 x 128 tiles                everything else (the benchmark regime: 0.89-0.90 of the fp64 MFMA peak, r03_kernel_stats)
//   K3  final stage                          one wavefront per (query, output) up to SR_FINAL_WAVE_T (4096) queries (44 -> 9.8 us at
//                                            N = 5000, T = 1, r01d); K1 splits N down to 16 rows per workgroup there (26.6 -> 8.7 us)
//   K1  splits of the training rows          sr_kstar_nsplit: until the grid holds SR_KSTAR_WGS (768) workgroups, at least SR_KSTAR_MIN_ROWS
//                                            (16) padded rows per split; beyond SR_FINAL_WAVE_T queries at most max(SR_KSTAR_SERIAL_SPLITS
//                                            (16), Np / 128) splits
//  single blocking query (host entry points)
//   K0s resident server (sr_capi_server.hip) sr_gp_server_supported: Np <= 512, D <= 5; one 16-wavefront workgroup per output at Np = 128,
//                                            Np / 64 parts of 8 wavefronts from 256 on (U^-1 fragments in registers): __call__ 21.6 -> 9.6 us
//                                            at N <= 128, 27 -> 11.9 at N = 150 (cart-pole), 33 -> 12.8 at N = 350 (r04_call_latency)
//   one command (sr_gp_call1)                where K0 applies (Np <= 384; 512 with second order): 26.4 us at N = 200 (r03_call_latency)
//                                            and on the streamed route from 512 padded rows on (query read from the pinned block,
//                                            results + flag by the final stage's workgroup): N = 1000 32 -> 26 us (r04_call_latency)
//  second order of one query (sr_gp_linearize)  K0 LIN up to Np = 384 (18 us at N = 200), streamed above: one launch for D <= 3
//                                            (SR_LIN_FUSED_MAX_D): N = 5000 61 -> 51 us (r02_latency_grid)
//  Hessian of the mean of a batch            KH sr_hess_kernel (sr_predict_grad.hip, behind the gradient pass): one thread per
//   (sr_gp_linearize_batch)                  (query, output), the training rows split until the grid holds SR_HESS_WGS workgroups,
//                                            at least SR_HESS_MIN_ROWS rows per split (T = 2 at N = 5000: 157 splits; T = 65536: 2);
//                                            sizes set from the K* pass's 768-workgroup target, not swept (profiles/r08_linearize_batch.txt)
//  reverse pass of one step                  passes of at most sr_stable_pass_max(N, Np, n_out) queries: the widest batch at which
//   (sr_capi_reach.hip: onestep_vjp_impl)    sr_kstar_nsplit and sr_hess_nsplit still give the counts of one 256-query block, SR_FINAL_WAVE_T
//                                            at most (the same bits for any chunk size; N = 2000, two outputs: 768)
//  multi-step chains (sr_capi_chain.hip)     persistent kernel K0c up to SR_CHAIN_GROUPS workgroups (device CUs - 16 at most),
//                                            1 launch for H <= 2, <= 2 launches for T <= 1024, <= 6 beyond (N = 200 H = 15: 1024
//                                            rollouts 203 against 253 us, 4096 in six launches 608 / 722, r03_chain_bench); one-step
//                                            through it for n_s <= 2 (24.5 -> 21.5 us; n_s >= 3: 25 -> 35 us)
//  model update (sr_capi_update.hip)         panels of sr_fact_panel(nb) blocks (r03_factor_bench and the comment there); streams:
//                                            up to SR_FACT_ONE_STREAM_MAX_NB (15) blocks the caller's stream only (r06_small_update_streams),
//                                            regime 1 up to SR_FACT_CHAIN_MAX_NB (128) blocks -- bulk stream without 32 CUs (64 for
//                                            36 < nb <= 52: N = 5000 5.14 -> 4.99 ms) --, regime 2 beyond (8 CUs for the diagonal
//                                            blocks; a trailing update SR_FACT_FREE_RATIO (2) times longer than the next chain takes
//                                            the whole chip: N = 50000 66.8 -> 67.2 TF, r04_timeline50000); early inversion from
//                                            nb >= 8; GEMM tile: sr_use_tile64* (sr_gemm.hip)
//  posterior function samples               draw: the prior at the training rows and V = U^-T R through sr_launch_gemm_tn (its own tile
//   (sr_capi_paths.hip, sr_paths.hip)        choice: sr_use_tile64), C = U^-1 V on the NT loop of the gradient pass, all outputs per launch;
//                                            eval: 128 x 128 tiles, grid Sp / 128 x Tp / 128 x n_out, feature slab in strips of
//                                            SR_PATHS_FROWS (16) features x 256 columns; step: one lane per path, the N + M terms
//                                            split by sr_hess_nsplit(N + M, n_out, S) (SR_HESS_WGS workgroups, SR_HESS_MIN_ROWS terms
//                                            at least), partial sums added in ascending order.  Sizes taken from the Hessian pass and
//                                            the variance tile, not swept (profiles/r12_paths.txt holds the times they give);
//                                            Jacobians: the same tile, strips and split count (F keeps its bits), derivative slabs
//                                            in strips of 16 rows x 256 columns, the ordered sum one thread per (path, element of
//                                            J) (profiles/r13_paths_grad.txt); reverse pass of the roll-out: the Jacobians of all
//                                            H S (step, path) pairs in one launch split by sr_hess_nsplit(N + M, n_out, H S), the
//                                            adjoint sweep one lane per path in blocks of SR_RVJP_BLOCK (256) paths; neither swept
//                                            (profiles/r19_paths_rollout_vjp.txt)
//  row append (sr_capi_append.hip)           one launch for +1 point with Np <= 512 (SR_APPEND1_MAX_NP0, r03_exploration_step), <= 16
//                                            points matrix-vector shaped, 17 .. 128 on the MFMA tile (r03_append_bench); the Python layer
//                                            appends up to N / 5 points and refactorises beyond (break-even r03_growing_model)
// ================================================================================================================
#define SR_ONE_STREAMED_NP 384       /* ONE query at this padded size takes the streamed kernel, not K0 */
#define SR_MFMA_SMALL_MAX_NP 2048    /* 2 .. 4 queries up to here: K1 + MFMA streaming kernel instead of the one-launch VALU kernel */
#define SR_STREAM_FUSED_MAX_D 5      /* one-launch streamed predict (T <= 4) evaluates its own K* columns up to this D */
#define SR_LIN_FUSED_MAX_D 3         /* one-launch streamed linearize up to this D */
#define SR_FACT_CHAIN_MAX_NB 128     /* model update: up to here the chain of diagonal blocks bounds it (stream regime 1) */
#define SR_FLOW_MIN_NB 1000           /* model update: tile-flow Cholesky (sr_flow.hip) from this many blocks ... */
#define SR_FLOW_MAX_NB 0              /* ... up to this many (empty range: opt-in through sr_gp_set_fact_pipeline(h, 3)) */
#define SR_FLOW_BAND 2                /* blocks right of the diagonal block that go in 64 x 64 tiles */
static inline int sr_flow_panel(int nb) { return nb <= 12 ? 2 : (nb <= 28 ? 3 : (nb <= 36 ? 4 : (nb <= 44 ? 6 : 8))); }   /* block rows per panel of the tile flow */
#define SR_FLOW_KEEP_WGS 128          /* tile flow: workgroups that stay to the end ... */
#define SR_FLOW_EXIT_PCT 50           /* ... the others leave after a row task past this percentage of the block rows */
#define SR_FLOW_EXIT_PCT_BIG 65       /* ... beyond 64 block rows (GEMM-bound for longer; N = 14000: 61.0 -> 59.4 ms, profiles/r06_flow.txt) */
#define SR_FLOW_TIMEOUT_S 0.25        /* a wait of the tile flow that lasts longer (+ 1 ps per output and Np^3: sr_capi_update.hip) gives up (the host repeats the update by launches) */
#define SR_FACT_ONE_STREAM_MAX_NB 15 /* model update: up to here every launch stays on the caller's stream (no side streams, no events) */
#define SR_APPEND1_MAX_NP0 512       /* +1 point in ONE launch of one workgroup per output up to this padded size (the grown model: <= 640) */
#define SR_APPEND1G_MAX_NP0 8192     /* +1 point in ONE launch of a grid of workgroups up to this padded size (K* row in LDS) */
#define SR_APPEND1G_MAX_W 128        /* workgroups per output of that grid */
#define SR_SLIDE_STEPS SR_NB         /* in-place one-point appends a set of model buffers can take: zeroed slack behind U^-1 (SR_SLIDE_STEPS (Np + 1) doubles), alpha and yT (SR_SLIDE_STEPS each) */
#define SR_STREAM_FUSED32_MAX_NCB 8   // 32 columns per workgroup are evaluated inside the MFMA kernel up to this many 256-column blocks (Np <= 2048)
#define SR_HESS_WGS 1024             /* Hessian-of-the-mean pass: workgroups the row splits aim at ... */
#define SR_HESS_MIN_ROWS 32          /* ... with at least this many training rows per split */
static inline int sr_hess_nsplit(int N, int n_out, long Tp) {
    const long blocks = ((Tp + 255) / 256) * n_out;
    long ns = (SR_HESS_WGS + blocks - 1) / blocks;
    const long cap = ((long)N + SR_HESS_MIN_ROWS - 1) / SR_HESS_MIN_ROWS;
    if (ns > cap) ns = cap;
    return ns < 1 ? 1 : (int)ns;
}
#define SR_KSTAR_WGS 768             /* K* pass (K1, and the gradient pass on its loop): workgroups the row splits aim at ... */
#define SR_KSTAR_MIN_ROWS 16         /* ... with at least this many padded training rows per split (a 16-long exp chain) */
#define SR_KSTAR_SERIAL_SPLITS 16    /* ... and, where the final stage sums them serially, at most max(this, Np / SR_NB) splits */
// splits of the training rows in the mean / Jacobian partial sums (srh::pick_nsplit(h, Tp) is this rule on a handle)
static inline int sr_kstar_nsplit(int Np, int n_out, long Tp) {
    const long blocks = ((Tp + 255) / 256) * n_out;
    long ns = (SR_KSTAR_WGS + blocks - 1) / blocks;
    // down to SR_KSTAR_MIN_ROWS training rows per workgroup; beyond SR_FINAL_WAVE_T queries
    // sr_finalize_kernel adds the partial sums serially per thread: never more than max(SR_KSTAR_SERIAL_SPLITS, Np/128) there
    // (32 / 64 / 128 rows per workgroup for 128 queries at N = 5000: K* pass 10.9 -> 13.1 / 17.7 / 29.8 us, final stage 10.2 ->
    //  7.4 / 5.9 / 5.5 us: no gain in the sum)
    long maxs = (long)Np / SR_KSTAR_MIN_ROWS;
    if (Tp > SR_FINAL_WAVE_T) {
        const long serial = (long)Np / SR_NB > SR_KSTAR_SERIAL_SPLITS ? (long)Np / SR_NB : SR_KSTAR_SERIAL_SPLITS;
        if (maxs > serial) maxs = serial;
    }
    if (ns > maxs) ns = maxs;
    return ns < 1 ? 1 : (int)ns;
}
// The widest pass whose split counts are those of a one-block batch.  Both rules above split the sums over the training rows
// by the width b = n_out ceil(Tp / 256) of the batch they are given -- sr_kstar_nsplit: min(Np / SR_KSTAR_MIN_ROWS,
// ceil(SR_KSTAR_WGS / b)), sr_hess_nsplit: min(ceil(N / SR_HESS_MIN_ROWS), ceil(SR_HESS_WGS / b)) -- and sr_finalize sums in
// another order beyond SR_FINAL_WAVE_T queries.  Passes of at most 256 k queries, k the largest count of 256-query blocks at
// which both minima are still the first term (at least one block: b = n_out for every width up to 256), take the split counts
// the model size sets, whatever chunk the caller chose: the same bits for any chunk size (the reverse passes of
// sr_capi_reach.hip cut their batches here).
static inline long sr_stable_pass_max(int N, int Np, int n_out) {
    long kstar_cap = Np / SR_KSTAR_MIN_ROWS, hess_cap = ((long)N + SR_HESS_MIN_ROWS - 1) / SR_HESS_MIN_ROWS;    // the first terms
    if (kstar_cap < 1) kstar_cap = 1;
    if (hess_cap < 1) hess_cap = 1;
    long k = SR_KSTAR_WGS / kstar_cap;
    if (k > SR_HESS_WGS / hess_cap) k = SR_HESS_WGS / hess_cap;
    k /= n_out;
    if (k > SR_FINAL_WAVE_T / 256) k = SR_FINAL_WAVE_T / 256;
    return 256 * (k < 1 ? 1 : k);
}

static inline bool sr_gp_small_wanted(int Np, long T, int D, bool general) {
    (void)general;   // ARD-RBF and the general family both have a one-launch kernel
    if (Np == 512 && T <= 128) return false;  // measured: streaming U^-1 (K2s, groups of 16 queries) 22-23 us against 28 us here
    return Np % 128 == 0 && Np <= SR_FUSED_NP && T <= SR_FUSED_T && D <= 8;   // (D > 8: the hoisted training rows do not fit 128 VGPRs)
}
// ONE query with second-order outputs in one launch (K0 LIN): the ARD-RBF form up to D = 8, the general family (its own phase A:
// two MFMA products, rows 9 + j of the first) up to D = 5
static inline bool sr_gp_small_lin_wanted(int Np, int D, bool general) {
    return sr_gp_small_wanted(Np, SR_SMALL_T, D, general) && (!general || D <= 5);
}
// workgroups per output of the resident server: from Np = 256 on an output is served in Np / 64 parts of eight wavefronts
// (the U^-1 fragments of a part fit its registers), Np = 128 by one workgroup of sixteen
// (a general-family model -- mat52 / lin_* -- is served in parts at every size: two at Np = 128)
constexpr int sr_gp_server_parts(int Np, bool general) { return (Np >= 256 || general) ? Np / 64 : 1; }
// D <= 5 (pendulum: 3, cart-pole: 4 or 5): the D = 6 .. 8 instantiations of the sixteen-wavefront kernel spill and are not built
static inline bool sr_gp_server_supported(int Np, int D) { return Np % 128 == 0 && Np <= SR_FUSED_NP && D <= 5; }
// 64 x 64 tiles: profitable when the model is small and the 128-tile grid would leave most of the chip idle
static inline bool sr_var64_wanted(int Np, long Tp, int n_out) {
    const long wgs128 = (long)(Np / SR_NB) * (Tp / SR_NB) * n_out;
    return Np <= 1024 && wgs128 < 256;
}
// split-K / balanced shares: profitable when the plain kernel cannot fill the chip and there is a K range to split
static inline bool sr_var_splitk_wanted(int Np, long Tp, int n_out) {
    const int nrb = Np / SR_NB;
    const long wgs = (long)nrb * (Tp / SR_NB) * n_out;
    return nrb > 2 && wgs <= 1024;
}
// workgroups of the balanced launch: one per CU, two from 8192 cells on.  Round 5, with the pipelined main loop (G = 256
// against 512, n_out = 2, profiles/archive/r05_bal_ab.txt): N = 5000 T = 128 (U = 1640) 142 / 148 us, T = 256 (3280) 235 / 250, T = 512
// (6560) 426 / 425, T = 1024 (13120) 801 / 795; N = 4000 T = 512 (4224) 291 / 306, T = 1024 (8448) 525 / 535; N = 3000 T = 1024
// 321 / 329 -- the threshold of round 3 (2304 cells, old loop) sent T = 256 at N = 5000 to 512 workgroups; 384, 768 or
// 1024 workgroups -- shares that do not line up with the residency of the chip -- lose 15 - 30 %.  Half of a 512-way launch's
// time goes to twice the partial products (128 KB each, written and read again by the reduce pass).
static inline long sr_var_bal_wgs(long U) {
    static const long forced = sr_lab_env("SR_BAL_WGS", 0);     // (lab build: scripts/bal_ab.py)
    static const long thr = sr_lab_env("SR_BAL_THR", 8192);
    if (forced > 0) return U < forced ? U : forced;
    return U >= thr ? 512 : (U >= 256 ? 256 : U);
}
// The MFMA streaming kernel also serves 17 .. 1024 queries as groups of 16 (every group re-reads U^-1 from
// L2 / Infinity Cache) as long as that stays cheap: n_out Np^2/2 8 B x groups <= 300 MB.  Measured at N = 700,
// T = 128: 41 -> 25 us against the split-K tiles; N = 2000: 71 -> 40 us; from N = 3000 on the tiles win.
static inline int sr_var_small_groups_max(int Np, int n_out) {
    const double bytes = (double)n_out * Np * (double)Np * 4.0;
    int g = (int)(300e6 / bytes);
    if (g > 64) g = 64;
    return g < 1 ? 1 : g;
}
// blocks per Cholesky panel by the number of 128-blocks (measurements: sr_capi_update.hip, pick_fact_panel)
// (round 5, with the pipelined GEMM loops: at N = 50000 panels of 12 .. 24 blocks 69.0 - 69.2 TF, 32: 68.5, 48 -- round 4's choice --
//  67.8, 64: 66.5 on one box, profiles/archive/r05_c4_panels.txt; N = 10000 / 20000 / 30000 keep 8 / 8 / 24)
static inline int sr_fact_panel(int nb) { return nb <= 28 ? 2 : (nb <= 44 ? 3 : (nb <= 64 ? 4 : (nb <= 200 ? 8 : 24))); }
// CUs the bulk streams of the model update leave to the critical chain (regime 1: one per shader engine, two for 36 < nb
// <= 52; regime 2: one per XCD for the diagonal blocks)
// regime 2 of the model update (nb > SR_FACT_CHAIN_MAX_NB): a trailing update this many times longer than the next panel's
// chain runs on the unmasked bulk stream (whole chip; the chain's diagonal blocks then wait for their CUs, hidden)
#define SR_FACT_FREE_RATIO 2.0
static inline int sr_fact_reserved_cus(int regime, int nb) { return regime == 2 ? 8 : ((nb > 36 && nb <= 52) ? 64 : 32); }
// launches of the persistent chain kernel a batch of T rollouts over H steps may take before the per-step route is better
static inline long sr_chain_max_launches(long T, int H) { return H <= 2 ? 1 : (T > SR_FUSED_T ? 6 : 2); }
long sr_var_small_ws(int Np, int n_out);
int sr_launch_var_small(const double* Wt, const double* Ks, double* Vp, double* part, int N, int Np,
                        long Tp, int n_out, int T, hipStream_t s, int dot0 = 0, bool reduce = true);

int sr_launch_var_small_gather(const double* Vp, double* v, int Np, int n_out, int t, int T, hipStream_t s);
int sr_launch_var_small_gather_all(const double* Vp, double* v, int Np, int n_out, int T, hipStream_t s);
int sr_launch_append_alpha(const double* alpha0, int Np0, int N0, const double* Y2, const double* invS,
                           const double* mu_part, int nsplit, int n_out, int d, long Tp, const double* Ynew, int m,
                           double* alpha1, int Np1, hipStream_t s, int qoff = 0, int nbatch = 1, long sY2 = 0);
// one new point on a small model (Np0 <= 512, Np1 <= 640; kp != NULL: general kernels), all outputs, ONE launch (sr_append.hip);
// logdet: n_out x SR_APPEND1_WGS partial sums
#define SR_APPEND1_WGS 8
#define SR_APPEND1_MAX_OUT 16   // outputs whose new targets fit the kernel arguments (sr_gp_append1_host)
long sr_append1_grid_ws(int Np0, int n_out);
int sr_launch_append1_grid(const double* Wt0, const double* alpha0, const double* yT0, const double* Z, const double* ls,
                           const double* sf2, const double* noise, const double* kp, const double* znew, const double* ynew, double* Wt1,
                           double* alpha1, double* yT1, double* Zdst, double* logdet, int* info, int N0, int Np0, int Np1,
                           int D, int n_out, int W, double* ws, unsigned* cnt, unsigned base, unsigned q0, hipStream_t s,
                           const double* x_host = nullptr, const double* y_host = nullptr, int inplace = 0);
#define SR_APPG_ABORTED (-2)         /* status word of every output when the grid of sr_append1_grid_kernel did not assemble */
int sr_launch_append1_small(const double* Wt0, const double* alpha0, const double* yT0, const double* Z, const double* ls,
                            const double* sf2, const double* noise, const double* kp, const double* znew, const double* ynew, double* Wt1,
                            double* alpha1, double* yT1, double* Zdst, double* logdet, int* info, int N0, int Np0, int Np1,
                            int D, int n_out, hipStream_t s, const double* x_host = nullptr, const double* y_host = nullptr);
int sr_launch_append_small(const double* U12t, const double* Wt0, int Np0, int m, int stage, double* G,
                           const double* invS, double* Xt, double* Y2, hipStream_t s, int nbatch = 1);

// retire one training point / leave-one-out posterior (sr_remove.hip).  coef: n_out x sr_remove_coef_stride(Np) doubles
// [w | a | b | rho^2 ..]; zstash: room for the (N - 1 - j) D input values behind the retired row
static inline SR_HOST_DEVICE long sr_remove_coef_stride(int Np) { return 3L * Np + 4; }
int sr_launch_remove_rownorm(const double* Wt, int Np, int q, int n_out, double* coef, const double* Z, double* zstash, long zcount,
                             long zfrom, hipStream_t s);
int sr_launch_remove_compact(const double* yT0, int Np0, int N0, int q, double* yT1, double* alpha1, int Np1, int n_out,
                             const double* zstash, double* Z, long zcount, long zto, hipStream_t s);
int sr_launch_remove_rows(const double* Wt0, int Np0, int N0, int q, const double* alpha0, const double* coef, double* Wt1, int Np1,
                          double* alpha1, int n_out, hipStream_t s);
int sr_launch_remove_clean(double* Wt, double* alpha, double* yT, int Np, int n_out, int slide, long wt_slack, long vec_slack,
                           hipStream_t s);
int sr_launch_loo(const double* Wt, const double* alpha, const double* yT, int N, int Np, int n_out, double* mu_loo, double* var_loo,
                  hipStream_t s);

// ---- posterior function samples by pathwise conditioning (sr_paths.hip; the algebra: include/safereach.h) -------------------
#define SR_PATHS_MAX_D 8             /* input widths the feature and step kernels are compiled for (3 / 5 / 8), as the gradient pass */
#define SR_PATHS_FROWS 16            /* features per workgroup of the feature slab (one k-tile of the MFMA loop); not swept */
struct sr_paths_feat {
    const double* ls; const double* sf2; const double* omega; const double* tau;   // n_out x D, n_out, M x D, M
    int D, n_out, M, Mp;
};
// Phi[d][i][c] = sqrt(2 sf2_d / M) cos(omega_i . (x_t / l_d) + tau_i), t = c - col0, for i < M and 0 <= t < T; zero elsewhere
// (i < Mp, c < ncols): a k-major operand of the MFMA tile, n_out x Mp x ncols
// jg >= 0: the derivative in input dimension jg in its place, -sqrt(2 sf2_d / M) sin(..) omega[i][jg] / l_d[jg]
int sr_launch_paths_features(const sr_paths_feat& m, const double* X, long ldx, long T, long col0, long ncols, double* Phi,
                             hipStream_t s, int jg = -1);
// dKs[d][k][c] = Ks[d][k][c] (z_{k - (Np - N), jg} - x_{c, jg}) / l_d[jg]^2 on the real rows and the columns c < T, zero
// elsewhere (n_out x Np x Tp, as Ks; X is T x D)
int sr_launch_paths_dkstar(const double* Ks, double* dKs, const double* Z, const double* X, const double* ls, int N, int Np,
                           int D, int n_out, long T, long Tp, int jg, hipStream_t s);
// path-major draws src (n_out x S x n) -> k-major dst (n_out x Rp x Sp) rows off .. off + n, the rest zero.  yT == NULL:
// dst = src^T; else dst = yT - dst - sqrt(noise_d) src^T on the real rows and columns (dst holds the prior on entry; Rp = Np)
int sr_launch_paths_pack(const double* src, double* dst, const double* yT, const double* noise, int n, int off, int Rp, int S,
                         int Sp, int n_out, hipStream_t s);
// C = U^-1 V (n_out x Np x Sp, rows of the front padding exactly zero) on srt::mainloop_nt_glds
int sr_launch_paths_solve(const double* Wt, const double* V, double* C, int N, int Np, int Sp, int n_out, hipStream_t s);
// F[t][s][d] = sum_{k < Mp} Phi[d][k][t] Wk[d][k][s] + sum_{k >= front padding} Ks[d][k][t] C[d][k][s], t < T, s < S
// es > 0: the element goes to F[(t S + s) es + d ds] instead (a column of J: F = J + j, es = n_out D, ds = D)
int sr_launch_paths_eval(const double* Phi, const double* Wk, const double* Ks, const double* C, double* F, int N, int Np,
                         int Mp, long T, long Tp, int S, int Sp, int n_out, hipStream_t s, int es = 0, int ds = 1);
struct sr_paths_step_args {
    sr_paths_feat m; const double* Z; const double* Wk; const double* C; const double* Xs;
    double* part;                     // nsplit x n_out x Sp; with J: nsplit x n_out x (1 + D) x Sp
    double* F; const double* k_fb; const double* k_ff; double* z_next; int n_u;
    double* J;                        // S x n_out x D, or NULL: the value alone
    int N, Np, S, Sp, nsplit;
};
int sr_launch_paths_step(const sr_paths_step_args& a, hipStream_t s);
// the closed-loop roll-out of every path in one launch (sr_paths_rollout.hip): H steps from x0 (n_out, or S x n_out with
// x0_per_path) under the gains k_fb (H x n_u x n_out), k_ff (H x n_u)
struct sr_paths_rollout_args {
    sr_paths_feat m; const double* Z; const double* Wk; const double* C;
    const double* x0; int x0_per_path, H; const double* k_fb; const double* k_ff;
    double* X_all;                    // H x S x n_out
    double* A_all;                    // H x S x n_out x n_out, or NULL: the states alone
    int N, Np, S, Sp;
};
int sr_launch_paths_rollout(const sr_paths_rollout_args& a, hipStream_t s);
// its reverse pass (sr_paths_rollout_vjp.hip): the Jacobians of all H S (step, path) pairs at the stored states, the adjoint
// sweep one lane per path, the sums over the paths in a fixed order
#define SR_RVJP_BLOCK 256            /* paths per workgroup of the sweep = per partial record; not swept */
static inline int sr_paths_rollout_vjp_blocks(int S) { return (S + SR_RVJP_BLOCK - 1) / SR_RVJP_BLOCK; }
struct sr_paths_rollout_vjp_args {
    sr_paths_feat m; const double* Z; const double* Wk; const double* C;
    const double* x0; int x0_per_path, H; const double* k_fb; const double* k_ff;
    const double* X_all; const double* X_bar;            // H x S x n_out each (X_all[H - 1] is not read)
    double* x0_bar; double* k_fb_bar; double* k_ff_bar;  // n_out (S x n_out with x0_per_path), H x n_u x n_out, H x n_u
    double* J; long j_si, j_ss, j_se;                    // J_i[s][d][j] at J[i j_si + s j_ss + (d D + j) j_se]
    double* part;                     // nsplit x n_out x D x H x Sp
    double* rec;                      // blocks x H x n_u (1 + n_out), then blocks x n_out (shared start), blocks = .._vjp_blocks(S)
    int N, Np, S, Sp, nsplit;
};
int sr_launch_paths_rollout_vjp(const sr_paths_rollout_vjp_args& a, hipStream_t s);
// ---- the same for the general family with the RBF radial part (sr_paths_gen.hip; the algebra: include/safereach.h) -----------
// A path of one output takes n_w = G M + D weights: group g < G is the base feature map times A_grp[g](x) (A_0 = sqrt(c0),
// A_l = sqrt(a_l) x_l; grp: the l active on at least one output, ascending), rows [g M, (g + 1) M) of the slab; the linear
// features sqrt(b_j) x_j are rows G M + j.  m.M is the base count M, m.Mp is n_w rounded up to SR_PATHS_FROWS, m.ls and
// m.sf2 are not read (the parameters are kp: n_out x SR_KP(D), kappa id 0 on every output, nothing negative).
struct sr_paths_gen {
    const double* kp; int G, n_w; int grp[SR_PATHS_MAX_D + 1];
};
// Phi[d][g M + i][c] = A_grp[g](x_t) sqrt(2 v_d / M) cos(sum_j omega[i][j] s_dj x_tj + tau[i]) and Phi[d][G M + j][c] =
// sqrt(b_dj) x_tj, t = c - col0, for 0 <= t < T; zero elsewhere (rows < m.Mp, c < ncols).  jg >= 0: the derivative in x_jg
int sr_launch_paths_gen_features(const sr_paths_feat& m, const sr_paths_gen& g, const double* X, long ldx, long T, long col0,
                                 long ncols, double* Phi, hipStream_t s, int jg = -1);
// dKs[d][k][c] = d k_d(x_c, z_{k - (Np - N)}) / d x_jg (sr_dk) on the real rows and the columns c < T, zero elsewhere
int sr_launch_paths_gen_dkstar(double* dKs, const double* Z, const double* X, const double* kp, int N, int Np, int D, int n_out,
                               long T, long Tp, int jg, hipStream_t s);
// the step: a.part in the layout of sr_launch_paths_step (whose ordered sum runs behind it), a.Wk n_out x m.Mp x Sp
int sr_launch_paths_gen_step(const sr_paths_step_args& a, const sr_paths_gen& g, hipStream_t s);

struct sr_final_args {
    const double* mu_part; const double* jac_part; const double* var_part; const double* sf2;
    const double* ls; const double* kxx;    // kxx != NULL: per-query prior variance instead of sf2
    double* mu; double* var; double* jac;   // T x n_out, T x n_out, T x n_out x D (jac may be NULL)
    int n_out, D, nsplit, nrb; long T, Tp;
};
int sr_launch_finalize(const sr_final_args& a, hipStream_t s);

struct sr_ell_args {
    long T; int n_s, n_u;
    const double* p; long ldp;        // T x n_s, row stride ldp
    const double* q; long ldq;        // T x n_s*n_s or NULL
    const double* k_ff; long ldkff;   // T x n_u
    const double* k_fb; long ldkfb;   // T x n_u*n_s or NULL
    const double* mu; const double* var; const double* jac;   // dense T x n_s, T x n_s, T x n_s x D
    const double* a; const double* b; const double* l_mu; const double* l_sigma;
    double c_safety;
    double* p_out; long ldpo;         // T x n_s
    double* q_out; long ldqo;         // T x n_s*n_s
    int* n_bad;                       // device counter (nullable): queries whose box bounds were not > 0
    int mode;                         // 0 robust ellipsoid (gp_reachability.py), 1 Taylor / 2 mean-equivalent
                                      // Gaussian moment propagation (uncertainty_propagation_casadi.py)
};
int sr_launch_ellipsoid(const sr_ell_args& a, hipStream_t s);
// reverse pass of one step in mode 0 (sr_ellipsoid_vjp_dev.h, sr_reach_vjp.hip); every array dense
struct sr_ellvjp_args {
    long T;
    // forward inputs (dense): q T x n_s^2 or NULL (point branch), k_fb T x n_u n_s, jac T x n_s (n_s + n_u)
    const double* q; const double* k_fb; const double* var; const double* jac;
    const double* a; const double* b; const double* l_mu; const double* l_sigma; double c_safety;
    const double* p1_bar; const double* q1_bar;            // seeds, either may be NULL
    double* p_bar; double* q_bar; double* kff_bar; double* kfb_bar; double* mu_bar; double* var_bar; double* jac_bar;
    // GP link (jac_mu == NULL: none; hess_mu == NULL: no second-order term -- jac_bar is zero and is not read).  jac_mu / jac_var
    // T x n_s x D, hess_mu T x n_s x D x D at z = [Tz p; k_ff]; Tz n_xin x n_s or NULL (identity, n_xin = n_s); jac_s
    // T x n_s (n_s + n_u) and jz T x n_s x D: per-query scratch, touched only with hess_mu and Tz both set
    const double* jac_mu; const double* jac_var; const double* hess_mu; const double* Tz; int D, n_xin;
    double* jac_s; double* jz;
};
int sr_launch_reach_vjp(const sr_ellvjp_args& a, int n_s, int n_u, hipStream_t s);
// z[t] = [Tz p[t]; k_ff[t]] (T x (n_xin + n_u); Tz NULL: the identity, n_xin = n_s)
int sr_launch_reach_z(long T, int n_s, int n_u, int n_xin, const double* p, const double* k_ff, const double* Tz, double* z,
                      hipStream_t s);
// reverse pass of one step in mode 1 / 2 (sr_moments_vjp_dev.h, sr_moments_vjp.hip): the fields of sr_ellvjp_args under the names of
// the moment step -- q = sigma_x (NULL: point start), var / l_mu / l_sigma / c_safety unread, jac unread in mode 2, p1_bar = mu1_bar,
// q1_bar = sigma1_bar, p_bar = mux_bar, q_bar = sigma_bar, mu_bar = mug_bar; jac_bar may be NULL where it is zero (point start,
// mode 2); GP link: as above -- the host sets hess_mu in mode 1 with sigma_x only
struct sr_momvjp_args {
    sr_ellvjp_args e;
    const double* gpvar_bar;          // seed on the GP variances (T x n_s) or NULL
    int mode;                         // 1 Taylor, 2 mean-equivalent
};
int sr_launch_moments_vjp(const sr_momvjp_args& m, int n_s, int n_u, hipStream_t s);
// reverse pass of a roll-out of H steps in mode 0 (sr_reach_rollout_vjp.hip) for a group of e.T trajectories.  Query n = t H + i is
// step i of trajectory t; every array of `e` is dense in n (e.q = q_in, e.k_fb = kfb_in, e.p1_bar = p_seed, e.q1_bar = q_seed),
// the GP link fields as in sr_ellvjp_args with hess_mu always set.
struct sr_rrv_args {
    sr_ellvjp_args e;
    int H, n_s, n_u;
    // the caller's arrays, from the group's first trajectory on: q0 NULL = point start; k_fb NULL where H == 1; either seed may be NULL
    const double* p0; const double* q0; const double* k_fb0; const double* k_ff; const double* k_fb;
    const double* p_all; const double* q_all; const double* p_all_bar; const double* q_all_bar;
    double* p0_bar; double* q0_bar; double* kfb0_bar; double* kff_bar; double* kfb_bar;   // q0_bar, kfb0_bar may be NULL in a point start
    // seed on the GP variances the roll-out returns beside its outputs (T x H x n_s) or NULL: added to the step's var_bar in mode 0
    // (sr_multistep_reach_var_vjp), read by sr_moments_vjp_one in modes 1 / 2
    const double* gpvar_all_bar;
    // per-query scratch: z (n_xin + n_u), q_in / q_seed (n_s^2), kfb_in (n_u n_s), p_seed (n_s), eig (1 + 2 n_s + n_u: r^2, w, v, K v)
    double* z; double* q_in; double* kfb_in; double* p_seed; double* q_seed; double* eig;
};
int sr_launch_reach_rollout_prep(const sr_rrv_args& r, hipStream_t s);
int sr_launch_reach_rollout_eig(const sr_rrv_args& r, hipStream_t s);
int sr_launch_reach_rollout_vjp(const sr_rrv_args& r, hipStream_t s);
// reverse pass of a roll-out of H steps in mode 1 / 2 (sr_moments_rollout_vjp.hip): the fields of sr_rrv_args under the names of the
// moment roll-out -- p0 = mu0, q0 = sigma0 (NULL: point start), k_fb0 NULL (step 0 has a zero gain), p_all / q_all = mu_all / sigma_all
// and their seeds, p0_bar / q0_bar = mu0_bar / sigma0_bar, kfb0_bar and eig unread; r.e as sr_momvjp_args names it: jac_bar NULL in
// mode 2, hess_mu set in mode 1 only (the sweep drops it at step 0 of a point start).  sr_launch_reach_rollout_prep(m.r) fills z, q_in
// and kfb_in.
struct sr_mrv_args {
    sr_rrv_args r;                    // (r.gpvar_all_bar: the seed on the GP variances)
    int mode;                         // 1 Taylor, 2 mean-equivalent
};
int sr_launch_moments_rollout_vjp(const sr_mrv_args& m, hipStream_t s);
int sr_launch_remainder(long T, int n_s, int n_u, const double* q, const double* k_fb,
                        const double* l_mu, const double* l_sigma, double* u_mu, double* u_sigma,
                        hipStream_t s);
int sr_launch_sample(long T, int size, int n_out, int n_u, const double* mu, const double* var,
                     const double* eps, double* S, const double* k_fb, const double* k_ff, double* z,
                     hipStream_t s);
int sr_launch_distance(long T, int K, int n_s, const double* samples, int per_t, const double* p,
                       const double* q, double* d, hipStream_t s);
int sr_launch_safety(long T, int n_s, int m, const double* p, const double* q, const double* h_mat,
                     const double* h_vec, double c, double* d, hipStream_t s);
// the MPC objective over a stored moment trajectory and its reverse pass (sr_rollout_cost.hip): the arguments of sr_rollout_cost /
// sr_rollout_cost_vjp; n_c the width of the augmented state (n_s, n_s + 1 or n_s + 2), G the trajectories per workgroup (set by the
// launch)
struct sr_cost_args {
    long T; int H, n_s, n_u, idx, keep, loss, n_c, G;
    double a_trig, w_stage, w_term;
    const double *z, *F, *R, *mu, *sigma, *u, *cost_bar;
    double *cost, *cost_steps, *mu_bar, *sigma_bar, *u_bar;
};
int sr_launch_rollout_cost(sr_cost_args a, bool reverse, hipStream_t s);
// the SafeMPC constraint rows over a stored roll-out and their reverse pass (sr_rollout_constraints.hip): the arguments of
// sr_rollout_constraints / sr_rollout_constraints_vjp; bounds: control rows present, n_g the rows per trajectory, G the
// trajectories per workgroup of the forward (set by the launch)
struct sr_rcn_args {
    long T; int H, n_s, n_u, m_obs, m_safe, n_g, bounds, G;
    double c;
    const double *p_all, *q_all, *k_ff, *k_fb, *q0, *kfb0, *u_min, *u_max, *h_obs_mat, *h_obs, *h_safe_mat, *h_safe, *g_bar;
    double *g, *g_max, *p_all_bar, *q_all_bar, *kff_bar, *kfb_bar, *q0_bar, *kfb0_bar;
};
int sr_launch_rollout_constraints(sr_rcn_args a, bool reverse, hipStream_t s);
// the exploration objective over stored GP variances and its reverse pass (sr_rollout_explore.hip): the arguments of
// sr_rollout_explore / sr_rollout_explore_vjp; G the trajectories per workgroup of the forward (set by the launch)
struct sr_xpl_args {
    long T; int kind, n_s, H_v, n_dev, H_p, H_m, G;
    double eps;
    const double *gp_var, *p, *mu, *W, *cost_bar;
    double *cost, *cost_steps, *gpvar_bar, *p_bar, *mu_bar;
};
int sr_launch_rollout_explore(sr_xpl_args a, bool reverse, hipStream_t s);

// ---- fused small-batch posterior (sr_stream.hip) ------------------------------------------------------
struct sr_lin_args;
// ---- single-query second-order outputs (sr_linearize.hip) --------------------------------------
struct sr_lin_args {
    const double* Z; const double* alpha; const double* ls; const double* Ks; const double* g;
    const double* sf2;               // ARD-RBF signal variances (n_out)
    const double* x;                 // D query coordinates (or the first na of them when xb is set)
    const double* xb = nullptr; int na = 0;   // streamed route: coordinates na .. D-1 come from xb
    const double* kp;                // general kernels: n_out x SR_KP(D) packed parameters, else NULL (ARD-RBF)
    double* jac_var; double* hess_mu;   // n_out x D, n_out x D x D
    int N, Np, D, n_out; long Tp;
};
int sr_launch_trmv_t(const double* M, long ld, const double* x, long xs, double* y, int n, hipStream_t s);

// fused small-batch posterior (sr_stream.hip): up to 128 columns through U^-1 in one pass, reduction and final stage
// behind tickets.  mode 0: columns = queries (predict), fa describes the final stage; mode 1: columns = [k*, dk*/dx]
// of one query (linearize), la / lin_part / nblk / lin_dt / lmu.. describe it.
struct sr_stream_args {
    const double* Wt; const double* Ks; double* Vp; double* part; unsigned* tickets;
    int N, Np, D, n_out, ncb, npairs, k_lo, ncols, ncols_pad, dot0, mode;
    int width_min;                   // take at least this kernel width (16: the MFMA kernel also for <= 4 columns)
    long Tp;
    // columns evaluated in the kernel (ARD-RBF): model and queries
    const double* Z; const double* alpha; const double* ls; const double* sf2;
    const double* xa; long lda; int na; const double* xb; long ldb;
    double* mu_part_w; double* jac_part_w; double* lin_part_w;
    sr_final_args fa;
    sr_lin_args la; const double* lin_part; int nblk, lin_dt; double* lmu; double* lvar; double* ljac_mu;
    // one-command single query (sr_gp_call1 on a streamed model): the workgroup that runs the final stage publishes this
    // sequence number into pinned host memory after its outputs (which then live in pinned host memory too)
    unsigned long long* host_flag; unsigned long long host_seq;
    int probe = 0;                   // measurements only (SR_ST1_PROBE): 1 = sr_stream1_kernel stops after its streaming part
    // polling finaliser of the one-column kernel (round 6): dedicated, self-validating slots (SR_ST1_EMPTY until written):
    // [d][cb] column-block norms, then [j][d][1 + D] the N-split partial sums of mean and mean-Jacobian; NULL = tickets
    double* slots = nullptr;
    // work items of the run kernel (sr_stream_items): device table [column block, run, slot] x nitems, rows per run
    // followed by the workgroups' first entries (nwg + 1): a workgroup runs entries [first[w], first[w + 1])
    const int* item_tab = nullptr; int kr = 0, nitems = 0, nwg = 0;
    int epi = 1;                     // partial products of the MFMA kernels: 1 one 32-byte run per lane; lab build: 0 8-byte pieces (round 5), 2 non-temporal
};
#define SR_ST1_SLOTS_MAX 1536        /* doubles of LDS the finaliser gathers the slots in */
__host__ __device__ static inline long sr_st1_slots(int ncb, int n_out, int D) { return (long)n_out * ncb * (1 + 2 * (1 + D)); }
// bit pattern no arithmetic produces (a signalling NaN with a payload): "not written yet"
#define SR_ST1_EMPTY 0x7FF4C0FFEE5AFE01ull
long sr_stream_vp_doubles(int Np, int n_out, int ncols);
int sr_stream_tickets(int Np, int n_out);
int sr_stream_width(int ncols);
// can_fuse: the caller can have the kernel evaluate its own K* rows (ARD-RBF, D <= 5): one-chunk items then reach further
void sr_stream_plan(int Np, int n_out, int nc, int* g, int* kc, bool can_fuse = false);
#ifdef __cplusplus
#include <vector>
int sr_stream_items(int Np, int n_out, int nc, int n_cu, bool can_fuse, std::vector<int>& tab, int* nitems, int* nwg);   // rows per run (0: no run kernel)
#endif
// route != NULL: the launcher notes the kernel form it picked there (SR_ROUTE_* words of include/safereach.h; host side only)
int sr_launch_stream(sr_stream_args a, int src, hipStream_t s, int* route = nullptr);
int sr_launch_linearize(const sr_lin_args& a, hipStream_t s);
int sr_lin_nacc(int D);
int sr_launch_lin_columns(const sr_lin_args& a, int tq, double* Ks, double* lin_part, hipStream_t s);
int sr_launch_lin_final(const sr_lin_args& a, const double* lin_part, const double* dots, int ncb, double* mu,
                        double* var, double* jac_mu, hipStream_t s);
