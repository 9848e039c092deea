// sr_handle.h -- the model handle behind sr_gp_t and the host-side helpers the entry-point files share.
// Private to the library (include/safereach.h is the public face).  The entry points live in
//   sr_capi_handle.hip     handle life cycle, device-memory block cache, data, export / import / packed replication,
//                          switches, per-kernel timing
//   sr_capi_update.hip     model update: Gram -> blocked Cholesky -> U^-1 -> alpha (sr_gp_factorize) and its diagnostics
//   sr_capi_append.hip     block row append (sr_gp_append)
//   sr_capi_remove.hip     retiring training points (sr_gp_remove), leave-one-out posterior (sr_gp_loo)
//   sr_capi_posterior.hip  workspace, dispatch of the posterior pass (sr_gp_predict, sr_gp_linearize, sr_gp_call1),
//                          input transform, completion mailbox
//   sr_capi_reach.hip      reachability / moment propagation with the GP inside, forward and reverse (scratch: sr_reach_ws.h);
//                          the stateless steps, roll-out cost, distances, sampling
//   sr_capi_chain.hip      dispatch of the persistent chain kernel (try_chain), its launch gate and switches
//   sr_capi_moment_match.hip  exact moment matching: per query, whole roll-outs, and their reverse passes
//   sr_capi_server.hip     resident single-query server: start / stop / blocking call
//   sr_capi_paths.hip      posterior function samples by pathwise conditioning (sr_gp_paths_draw / _count / _weight_count /
//                          _eval / _step ...)
#pragma once
#include "sr_mfma_tile.h"
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>
#include <algorithm>

// resident single-query server (sr_capi_server.hip, kernel K0s of sr_server.hip)
struct sr_server {
    int armed = 0;                           // sr_gp_server_start was called: sr_gp_server_call (re)launches as needed
    int running = 0;                         // a launch of this handle may be resident
    void* pinned = nullptr; size_t pinned_bytes = 0;      // one pinned block: mailbox | reply words | reply block
    unsigned long long *mb = nullptr, *reply = nullptr; double* out = nullptr;              // host addresses
    unsigned long long *mb_dev = nullptr, *reply_dev = nullptr; double* out_dev = nullptr;  // the device's addresses of the same
    hipStream_t stream = nullptr;            // non-blocking stream of its own: nothing else is ever ordered behind the kernel
    unsigned long long next_seq = 1, idle_ticks = 500000, epoch = 0;
    unsigned long long cmd = 0;              // command of the request in the mailbox (the line's word 5 also carries the epoch and is
                                             // overwritten when a launch is called off: the host keeps the command)
    long launches = 0, calls = 0;
    int stale = 0;                           // a request was given up (time-out): the next call starts from a fresh launch
    std::mutex mu;                           // one caller at a time: a call, and a quiesce from another thread's entry point
};

struct sr_gp;
namespace srh {

// device memory through the block cache (sr_capi_handle.hip)
int dev_alloc_bytes(void** p, size_t bytes);
template <typename T>
static inline int dev_alloc(T** p, size_t count) { return dev_alloc_bytes((void**)p, count * sizeof(T)); }
void dev_free(void* p);
int dev_zero(void* p, size_t bytes);

// resident server (sr_capi_server.hip): off the device before the model is written / before a device-wide wait
int server_quiesce(sr_gp* h);
void servers_quiesce_device(int device);
void server_release(sr_gp* h);
// hipDeviceSynchronize for the library: resident servers of the current device leave first (they would keep the wait
// until their idle time-out otherwise)
static inline hipError_t device_sync() {
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess) servers_quiesce_device(dev);
    return hipDeviceSynchronize();
}

// what must have finished before a scratch block that is being replaced goes back to the block cache: nothing (no launch
// has seen the block), the work of one stream, or the device (device_sync: several streams may still read the block)
struct wait {
    enum { NONE, STREAM, DEVICE } what; hipStream_t s;
    static wait none() { return {NONE, nullptr}; }
    static wait stream(hipStream_t s) { return {STREAM, s}; }
    static wait device() { return {DEVICE, nullptr}; }
};

// grow-only device scratch of the handle: a block and its capacity in elements.  The contents do not survive a growth.
template <typename T>
struct scratch {
    T* p = nullptr; size_t cap = 0;
    T* get() const { return p; }
    void drop() { dev_free(p); p = nullptr; cap = 0; }
    // room for `need` elements; *grew: the block is a new one (its contents are unspecified)
    int grow(size_t need, wait w, bool* grew = nullptr) {
        if (grew) *grew = false;
        if (need <= cap) return SR_OK;
        if (w.what == wait::STREAM) SR_HIP(hipStreamSynchronize(w.s));
        if (w.what == wait::DEVICE) SR_HIP(device_sync());
        drop();
        SR_TRY(dev_alloc(&p, need));
        cap = need;
        if (grew) *grew = true;
        return SR_OK;
    }
};

}  // namespace srh

struct sr_gp {
    int device = 0, N = 0, Np = 0, D = 0, n_out = 0;
    sr_server srv;
    // persistent device state
    double *Z = nullptr, *yT = nullptr, *ls = nullptr, *sf2 = nullptr, *noise = nullptr,
           *alpha = nullptr, *Wt = nullptr;
    double* kp = nullptr;     // general kernel family: n_out x SR_KP(D) packed parameters (else NULL)
    // GP input transform of the reachability / moment entry points: x_gp = Tz x (Tz n_xin x n_s), NULL = identity
    double* Tz = nullptr; int n_xin = 0;
    srh::scratch<double> tz_x, tz_jac;       // transformed inputs / chain-ruled Jacobians (per chunk; both sized by its queries)
    // persistent multi-step kernel (sr_chain.hip K0c): exchange buffer, per group ticket + epoch + done counter (all of
    // the hand-off state lives on the device), switch
    sr_xel* chain_xch = nullptr; unsigned long long* chain_tickets = nullptr;       // the groups' epochs
    unsigned* chain_done = nullptr; int chain = 1; int last_chain = 0; int chain_cap = -1;
    int* chain_status_host = nullptr; int* chain_status_dev = nullptr;   // pinned: set by a chain launch that timed out
    int chain_occ_key = -1, chain_occ_blocks = 0;                         // occupancy of the kernel last asked about
    int chain_test_drop = 0;                                              // sr_test_chain_drop
    unsigned* call_ticket = nullptr;        // sr_gp_call1: workgroups done (reset by the last one)
    int general = 0;
    // general: what srh::general_info read back from the packed parameters of this data set (gen_rbf == -1: not read yet) --
    // every output has the RBF radial part (kappa id 0); the groups of the paths' feature map, bit l set where c0 (l = 0) or
    // a_l is non-zero on at least one output (l <= D, D <= SR_PATHS_MAX_D); the first negative v, c0, a_j or b_j by name
    int gen_rbf = -1; unsigned gen_groups = 0; char gen_negative[48] = "";
    int have_data = 0, factorized = 0;
    int sparse = 0;          // the posterior is that of sr_gp_fit_sparse: Wt Wt^T = K_uu^-1 - Sigma^-1, not K_y^-1
    int import_open = 0;     // between sr_gp_import_begin and sr_gp_import_end
    // Model generation: bumped (srh::model_rewritten) by every entry point that rewrites Z, the hyper-parameters, yT, alpha or
    // U^-1.  State derived from the model remembers the generation it was made from (the paths below).
    unsigned long long model_gen = 1;
    // per-chunk workspace (ensure_ws / free_ws: one group, two capacities)
    long chunk = 65536, ws_Tp = 0, ws_part = 0;     // ws_part: capacity of mu_part in units of n_out doubles
    int ws_locked = 0;       // internal buffers (mu / var / jac) are referenced by an entry point: growing now is a bug
    double *Ks = nullptr, *mu_part = nullptr, *jac_part = nullptr, *var_part = nullptr,
           *mu = nullptr, *var = nullptr, *jac = nullptr, *kxx = nullptr;
    srh::scratch<double> lin_v;                      // sr_gp_linearize: v = U^-T k* (n_out x Np) / the streamed route's partial sums
    double *lin_g = nullptr, *small_vp = nullptr;    // g = U^-1 v (n_out x Np); partial sums of the streaming variance pass
    srh::scratch<double> stream_vp;                  // fused small-batch path: partial sums
    unsigned* stream_tickets = nullptr;
    srh::scratch<int> stream_tab; long stream_tab_key = -1; int stream_tab_kr = 0, stream_tab_n = 0, stream_tab_nwg = 0;   // work items of the run kernel (+ workgroups they are dealt to)
    srh::scratch<double> stream_slots;               // self-validating hand-over slots of the T = 1 kernel's polling finaliser
    srh::scratch<double> splitk_vt;                  // partial products of the balanced few-query-tile route
    // sr_gp_predict_grad: V = U^-T K* of a chunk (n_out x Np x Tp) and the row blocks' partial sums of
    // d var/dx (n_out x Np/128 x D x Tp)
    srh::scratch<double> grad_v, grad_part;
    // sr_gp_linearize_batch: the training-row splits' partial sums of the Hessian of the mean
    // (n_split x n_out x (D (D + 1) / 2 + 1) x Tp)
    srh::scratch<double> hess_part;
    // sr_gp_select_maxvar: the pivoted factor L (n_out x (m - 1) x padded pool) and [var | partial scores |
    // partial rows | taken marks]
    srh::scratch<double> sel_L, sel_ws;
    // sr_gp_moment_match: per query of a chunk the D x D algebra of every output and pair of outputs, and the row tiles'
    // partial sums of the double sum (sr_mm_ws_per_query doubles each); sr_gp_moment_match_vjp: the same records, mu, V, the
    // contribution records and the row tiles' sums (sr_mmg_ws_per_query doubles each); a general-family handle: the per-call
    // block (sr_mmx_call_ws doubles) in front of the chunk's records (sr_mmx_ws_per_query doubles per query)
    // sr_gp_moment_match_rollout: one step's records per trajectory of a chunk (sr_mmr_ws_per_traj doubles each)
    // sr_gp_moment_match_rollout_vjp: per trajectory of a group the reverse pass's scratch of its H queries, their inputs, one
    // step's seeds and results, and the carried adjoint (sr_mmrv_ws_per_traj doubles each)
    srh::scratch<double> mm_ws;
    // the reverse passes with the GP inside, of one step and of a whole roll-out (sr_capi_reach.hip): per query of a pass, or per
    // (trajectory, step) pair of a group, the blocks that sr_reach_ws.h lays out
    srh::scratch<double> reach_ws;
    // sr_gp_remove: per output the coefficient tables of the retired row (3 Np + 4), then the input rows behind it
    srh::scratch<double> rm_ws;
    // sr_gp_paths_*: the drawn paths [omega M x D | tau M | w n_out x Mp x Sp | c n_out x Np x Sp] (k-major operands of the MFMA
    // tile), valid while paths_gen == model_gen; and the workspace of the three calls (draw: Phi(Z), R, V; eval: Phi of a chunk;
    // step: the splits' partial sums), which sr_gp_release_scratch gives back
    srh::scratch<double> paths, paths_ws;
    int paths_S = 0, paths_M = 0, paths_Np = 0; unsigned long long paths_gen = 0;
    // log det(K + noise) per output as of the last <= 16-row append (read back with its status words): the blocking read of
    // sr_gp_logdet costs the exploration loop 30 us per step
    std::vector<double> logdet_host; int logdet_valid = 0;
    double* splitk_part = nullptr;                      // n_out x 4 nrb x Tp partial norms (<= 4 MB)
    int var_group = 64;      // query tiles per scheduling group of the variance kernel.  With the diagonal blocks cut short
                             // (variant 2) 64 beats 32: 70.7 against 70.0 TF at C2', fabric-side fetches 61.3 -> 42.9 M KiB per launch
                             // (scripts/pmc_groups.sh); 256 and more lose the sharing of the K* tiles (68.7 TF)
    int small_path = 1;      // latency paths (streaming T <= 16, 64-tiles, split-K) instead of the plain MFMA tiles
    int last_streamed = 0;   // the last gp_pass went through the streaming kernels (their partials hold U^-T k*)
    int force_stream = 0;    // sr_gp_linearize wants those partials whatever the model size
    int last_route[SR_ROUTE_WORDS] = {0};   // what the last gp_pass launched (sr_gp_last_route; diagnostics / tests)
    int var_variant = 4;     // 1: the loop of rounds 1 - 4 (LDS-DMA, barrier on top of a k-tile: 70 TF; the A/B reference), 3: the
                             // pipelined loop of round 5 (barrier under the MFMA stream: 73.1 TF), 4: 3 + diagonal blocks without
                             // their structural zeros (default: 74.5 TF)
    // factorisation: the outputs are independent problems -- below SR_FACT_PAR_BYTES of scratch each gets its own
    // HIP stream (the small-grid kernels of a modest model then overlap) and the scratch stays with the handle
    srh::scratch<double> fact_ws;                        // n_par x (U, W: Np^2 each, v: Np)
    // row append of few points (m <= 16): scratch and a second U^-1 buffer the new factor is assembled into
    // (kept while the padded size does not change: appends then allocate nothing big)
    srh::scratch<double> app_ws;
    unsigned long long* call_flag = nullptr; unsigned long long call_seq = 0;   // set by sr_gp_call1 around a streamed pass
    // In-place one-point appends (sr_capi_append.hip): Wt, alpha and yT may be VIEWS `slide` steps into their allocations
    // (Wt: slide * (Np + 1) doubles, alpha / yT: slide doubles); every entry point that rewrites the model, and every kernel
    // that wants U^-1 aligned to 16 bytes, calls unslide() first.  slack_ok: the three allocations carry the zeroed slack.
    int slide = 0; int slack_ok = 0;
    // A tile route of the posterior pass (16-byte reads of U^-1) that meets an odd slide has to unslide: a full copy of the
    // factor and a device-wide wait.  A loop that alternates one append with one big batch would pay that every step, so such
    // an unslide keeps the next `slide_hold` one-point appends off the in-place route (64, doubling with every forced
    // unslide since the last refit: slide_forced).
    int slide_hold = 0, slide_forced = 0;
    // Grid route of the one-point append: a grid that cannot become resident gives up after ~5 ms.  After such an abort the
    // route is left alone for `grid_hold` one-point appends (16, doubling with every further abort in a row, at most 16384).
    int grid_hold = 0, grid_aborts_row = 0; long grid_aborts = 0;
    double* appg_cnt = nullptr; unsigned appg_base = 0, appg_q = 0;   // (arrivals and barriers of all launches so far)      // barrier counters of the grid append (zero at allocation), their value after the last launch
    void* app_pin = nullptr; double* app_pin_dev = nullptr;   // pinned, mapped: results of sr_gp_append1_host (log det partials, status words)
    double* Wt_alt = nullptr; size_t wt_alt_cap = 0;
    int wt_alt_off = -1;     // front padding of the (complete, well-formed) factor Wt_alt last held; -1 unknown
    // small appends allocate nothing while the padded size stays: Z has room for z_cap points, yT / alpha ping-pong
    long z_cap = 0; double *yT_alt = nullptr, *alpha_alt = nullptr; int vec_alt_np = 0;
    std::vector<double> sf2_host, noise_host;    // host copies of sf2 / noise (filled on first use after set_data)
    // up to SR_FACT_SLOTS outputs are factorised at once as a BATCH (every launch covers all of them).  Streams:
    // CRITICAL (diagonal blocks, panel rows, look-ahead rows, late inversion), BULK (the trailing update behind the
    // look-ahead rows) and INVERSION (the early part of the triangular inversion); the caller's stream waits for them
    hipStream_t fact_stream = nullptr, bulk_stream = nullptr, inv_stream = nullptr;
    // pipelined chain (round 6, chain-bound sizes): the diagonal blocks on a stream of their own BESIDE the rest of the
    // previous block row (row stream); the three streams hand over through counters in device memory (sr_fact_handover_kernel)
    hipStream_t diag_stream = nullptr, row_stream = nullptr;
    unsigned* fact_flags = nullptr; int fact_flags_nb = 0;   // [status | c[nb] | d[nb] | r[nb]]; zero at allocation, values = epochs
    unsigned fact_epoch = 0;
    // tile-flow Cholesky (round 6; sr_flow.h): its counters, their capacity in words, the epoch of the last run
    unsigned* flow_flags = nullptr; long flow_words = 0; unsigned flow_epoch = 0;
    void* flow_segs = nullptr; int flow_segs_key[3] = {0, 0, 0}; long flow_total = 0, flow_total_far = 0, flow_total_upd = 0, flow_total_m = 0;   // task plan on the device for (nb, band, panel)
    int fact_pipe = 0;                                    // sr_gp_set_fact_pipeline: 0 = one chain of launches (default: the pipelined
                                                          // forms measured slower, profiles/r06_fact_pipeline.txt), 1 = three streams, 2 = two,
                                                          // 3 = tile-flow Cholesky (one resident kernel), -1 = never the tile flow
    int last_fact_pipe = 0;                               // the last update ran pipelined (diagnostics / tests)
    int last_update[SR_UPDATE_WORDS] = {0};               // how the last fit / append ran (sr_gp_last_update; diagnostics / tests)
    int last_remove[SR_REMOVE_WORDS] = {0}; int rm_count = 0;   // how the last point was retired, points retired since the last fit (sr_gp_last_remove)
    hipEvent_t fact_fork = nullptr, fact_join = nullptr;
    hipEvent_t ev_panel[2] = {nullptr, nullptr}, ev_bulk[2] = {nullptr, nullptr};
    hipEvent_t ev_inv[2] = {nullptr, nullptr};            // critical -> inversion stream, back
    int fact_panel = 0;                                  // blocks per Cholesky panel; 0 = by size
    int fact_regime = 0;                                 // how the streams below were made: 0 none, else 1000 x (1 chain-bound, 2 GEMM-bound) + reserved CUs
    int ncu = 0;                                         // compute units of the device (cached)
    // job lists of the level-batched triangular inversion (depend on Np only)
    int* fact_info = nullptr;                            // status words of the factorisation (64 ints)
    size_t mem_total = 0;                                // device memory (cached)
    sr_gemm_job* inv_jobs = nullptr; int inv_jobs_np = 0;
    // jobs of a level in ascending order of their block range [lo, hi); per job: where it ends, where its left child ends
    // (blocks), its 128-tiles -- the inversion is launched in stages as the Cholesky passes those points (sr_capi_update.hip)
    struct inv_level { int off1, off2, count, maxM, maxN; long tiles; int depth; std::vector<int> hi, mid; std::vector<long> tl; };
    std::vector<inv_level> inv_levels;
    sr_prof prof;
};
#define SR_FACT_PAR_BYTES ((size_t)8 << 30)

// every entry point runs on the handle's device and leaves the caller's current device as it found it
// (PyTorch reads its current device from the HIP runtime)
struct sr_dev_guard {
    int prev = -1; hipError_t err = hipSuccess;
    explicit sr_dev_guard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~sr_dev_guard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define SR_DEVICE(dev) sr_dev_guard dev_guard_(dev); SR_HIP(dev_guard_.err)

namespace srh {

static inline long round_up(long v, long m) { return (v + m - 1) / m * m; }

// one turn of a host spin loop (the pause hint where the host has one)
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}

// the handle's drop lists (sr_capi_handle.hip): the per-chunk workspace; everything whose size or content depends on the
// padded size (a block append that crosses a 128-row boundary; re-created lazily)
void free_ws(sr_gp* h);
void drop_np_sized(sr_gp* h);
// the spare factor buffer of the appends goes back (Wt_alt is a model buffer, not scratch: it ping-pongs with Wt)
static inline void drop_wt_alt(sr_gp* h) { dev_free(h->Wt_alt); h->Wt_alt = nullptr; h->wt_alt_cap = 0; h->wt_alt_off = -1; }
int ensure_wt(sr_gp* h);
// doubles of the three model buffers with their slack (see sr_gp::slide)
static inline size_t wt_doubles(int n_out, int Np) { return (size_t)n_out * Np * Np + (size_t)SR_SLIDE_STEPS * (Np + 1); }
static inline size_t vec_doubles(int n_out, int Np) { return (size_t)n_out * Np + SR_SLIDE_STEPS; }
static inline double* wt_alloc_of(const sr_gp* h) { return h->Wt ? h->Wt - (size_t)h->slide * (h->Np + 1) : nullptr; }
static inline double* alpha_alloc_of(const sr_gp* h) { return h->alpha ? h->alpha - h->slide : nullptr; }
static inline double* yT_alloc_of(const sr_gp* h) { return h->yT ? h->yT - h->slide : nullptr; }
static inline void model_rewritten(sr_gp* h) { ++h->model_gen; }     // (see sr_gp::model_gen)
// sr_gp_set_data_general leaves the packed parameters on the device: read them once per data set (one blocking copy behind
// `s`) -> h->gen_rbf, gen_groups, gen_negative.  Users: sr_gp_moment_match, sr_gp_paths_*.
int general_info(sr_gp* h, hipStream_t s);
int unslide(sr_gp* h);               // back to plain buffers (fresh allocations, two contiguous copies); no-op when slide == 0

// The chain of launches of sr_gp_factorize on the caller's matrices (sr_capi_update.hip; the sparse fit, sr_sparse.hip):
// mat n_out x Np x Np symmetric in the padded layout (identity on the padding; the upper block triangle is read), copied
// into the scratch in place of the Gram matrix; rhs n_out x Np in place of yT (NULL: alpha is not written).
// -> Wt = U^-1 with U^T U = mat, or, reversed != 0, Wt = J U^T J (J the reversal of the padded index: upper triangular,
// Wt Wt^T = J mat J).  info [host, n_out]: the 1-based PADDED index of the first non-positive pivot.
struct sr_fact_src { const double* mat; const double* rhs; int reversed; };
int factorize_matrix(sr_gp* h, void* stream, int* info, const sr_fact_src* src);

// posterior pass and its workspace (sr_capi_posterior.hip)
static inline int pick_nsplit(const sr_gp* h, long Tp) { return sr_kstar_nsplit(h->Np, h->n_out, Tp); }   // (the rule: sr_common.h)
int ensure_ws(sr_gp* h, long Tp, int nsplit);
int prepare_ws(sr_gp* h, long Tc);
struct sr_ws_lock {
    sr_gp* h;
    explicit sr_ws_lock(sr_gp* h_) : h(h_) { h->ws_locked = 1; }
    ~sr_ws_lock() { h->ws_locked = 0; }
};
int gp_pass(sr_gp* h, long Tc, const double* xa, long lda, int na, const double* xb, long ldb,
            int nb, double* mu, double* var, double* jac, hipStream_t s);
// a tile route meets an odd slide of U^-1: back to plain buffers first (see sr_capi_posterior.hip)
int tile_route_alignment(sr_gp* h);
int gp_pass_states(sr_gp* h, long Tc, const double* p, long ldp, int n_s, const double* kff, long ldkff, int n_u,
                   double* mu, double* var, const double** jac_out, hipStream_t s);
// the persistent chain kernel for a chain of H >= 1 steps, where it applies; *taken says whether it ran (sr_capi_chain.hip;
// hidden: the library's dynamic symbols stay those it had while this was a static function)
__attribute__((visibility("hidden")))
int try_chain(sr_gp* h, long T, int H, int mode, const double* p0, const double* q0, const double* k_fb0,
              const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
              const double* l_sigma, double c_safety, double* p_all, double* q_all, double* gp_var_all,
              int* n_bad, int n_s, int n_u, hipStream_t s, bool* taken);

// what every entry point that reads the fitted model checks first, under its own name
static inline int handle_ready(const sr_gp* h, const char* who) {
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(h->factorized, SR_ESTATE, "%s: model not factorized", who);
    return SR_OK;
}

// ---- the model as a launch reads it --------------------------------------------------------------------------------
// the fields every argument struct of the posterior kernels shares (sr_kstar_args, sr_lin_args)
template <typename A>
static inline void model_args(A& a, const sr_gp* h) {
    a.Z = h->Z; a.alpha = h->alpha; a.ls = h->ls; a.sf2 = h->sf2; a.kp = h->general ? h->kp : nullptr;
    a.N = h->N; a.Np = h->Np; a.D = h->D; a.n_out = h->n_out;
}
// one-launch passes (sr_small.hip, the resident server): the model, no workspace; the caller adds its queries
static inline sr_kstar_args kstar_model(const sr_gp* h) {
    sr_kstar_args a{};
    model_args(a, h);
    a.nsplit = 1;
    return a;
}
// passes through the per-chunk workspace (ensure_ws first)
static inline sr_kstar_args kstar_ws(const sr_gp* h, int nsplit, long T, long Tp) {
    sr_kstar_args a = kstar_model(h);
    a.Ks = h->Ks; a.mu_part = h->mu_part; a.jac_part = h->jac_part; a.kxx = h->kxx;
    a.nsplit = nsplit; a.T = T; a.Tp = Tp;
    return a;
}
static inline sr_final_args final_args(const sr_gp* h, int nsplit, int nrb, long T, long Tp, const double* var_part,
                                       double* mu, double* var, double* jac) {
    sr_final_args a{};
    a.mu_part = h->mu_part; a.jac_part = h->jac_part; a.var_part = var_part; a.sf2 = h->sf2;
    a.ls = h->ls; a.kxx = h->general ? h->kxx : nullptr; a.mu = mu; a.var = var; a.jac = jac;
    a.n_out = h->n_out; a.D = h->D; a.nsplit = nsplit; a.nrb = nrb; a.T = T; a.Tp = Tp;
    return a;
}

}  // namespace srh
