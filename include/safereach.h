/* safereach.h -- C-ABI of libsafereach.so (MI355X / gfx950).
 *
 * Drop-in boundary for the GP-dynamics inference + ellipsoid reachability hot path of
 * befelix/safe-exploration.  The reference has NO native interface (pure Python); the Python
 * surface it exposes is mirrored by safe_exploration_amd/ and every entry point below names the
 * reference function(s) it replaces (paths relative to /root/reference/safe_exploration/).
 *
 * Conventions
 *   - plain C, fp64, row-major; every array argument is a DEVICE pointer owned by the caller
 *     unless marked [host]; the library owns only what hangs off its opaque handle.
 *   - every function returns 0 on success, <0 on error (SR_E*); sr_last_error() returns a
 *     thread-local message.  Nothing throws across the boundary.
 *   - work is enqueued asynchronously on the hipStream_t passed as `void* stream` (NULL = default
 *     stream).  A handle is bound to one device and is not thread-safe.
 *   - n_out (GP outputs) == n_s for the reachability entry points; D = n_s + n_u (D = n_x_in + n_u with an input
 *     transform, sr_gp_set_input_transform).
 */
#ifndef SAFEREACH_H
#define SAFEREACH_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sr_gp* sr_gp_t;

#define SR_OK          0
#define SR_EINVAL     -1   /* bad argument / shape                        */
#define SR_EHIP       -2   /* HIP runtime error (no device, OOM, launch)  */
#define SR_ENOTPD     -3   /* Cholesky breakdown: matrix not positive definite */
#define SR_ESTATE     -4   /* call order violated (e.g. predict before factorize) */
#define SR_EBUSY      -6   /* transient: the device could not take the request now (a grid of co-resident workgroups did
                            * not assemble).  Nothing was changed; retry, or take the entry point the comment names. */
#define SR_EUNSUPPORTED -5 /* dimension outside compiled range (n_s<=8, n_u<=4, D<=12).  The reference's systems (n_s <= 4,
                            * D <= 5) run in registers, and so does everything up to n_s = 8 with n_u <= 2; the ellipsoid
                            * step with n_s = 8 and n_u = 3, 4 is compiled but spills 164 / 452 B per lane to scratch
                            * (profiles/archive/r03_kernel_resources.txt): correct, tested, and several times slower per query
                            * than the small instantiations */

/* kernel ids for sr_prof_get() */
#define SR_K_GRAM      0
#define SR_K_POTRF     1
#define SR_K_GEMM      2
#define SR_K_KSTAR     3   /* RBF cross-covariance + mean + mean-Jacobian              */
#define SR_K_VAR       4   /* triangular fp64-MFMA contraction |W k*|^2 (dominant)     */
#define SR_K_FINAL     5
#define SR_K_ELL       6   /* ellipsoid propagate/sum                                  */
#define SR_K_TRINV     7   /* GEMMs of the blocked triangular inversion W = U^-T            */
#define SR_K_SMALL     8   /* one-launch posterior of a small model (Np <= 512, T <= 1024)  */
#define SR_K_SPARSE_PANEL 9  /* sr_gp_fit_sparse: cross-covariance panel K_fu of a chunk (+ its share of K_uf y) */
#define SR_K_SPARSE_GEMM  10 /* sr_gp_fit_sparse: streamed G += K_fu^T K_fu on the fp64 MFMA tile                 */
#define SR_K_PATHS_DRAW   11 /* sr_gp_paths_draw: feature slab, residual, the two triangular products              */
#define SR_K_PATHS_EVAL   12 /* sr_gp_paths_eval[_grad]: feature (and derivative) slabs of the chunk + the two-range MFMA tile (K* pass: SR_K_KSTAR) */
#define SR_K_PATHS_STEP   13 /* sr_gp_paths_step[_grad]: split pass + ordered sum; sr_gp_paths_rollout: its one launch */
#define SR_K_REACH_VJP    14 /* sr_ellipsoid_step_vjp / sr_onestep_reach_vjp, sr_onestep_moments_vjp: the reverse of the step's algebra + the GP link (its linearisation: SR_K_KSTAR, SR_K_VAR, SR_K_FINAL) */
#define SR_K_COUNT     15

int         sr_version(void);
const char* sr_last_error(void);
/* number of visible HIP devices; SR_EHIP (and *n = 0) if the runtime reports none. */
int         sr_device_count(int* n);

/* ---- model life cycle --------------------------------------------------------------------
 * replaces: SimpleGPModel.__init__/train(opt_hyp=False)/update_model  ssm_gpy/gaussian_process.py:32-70,189-278,347-419
 * One handle = n_out independent ARD-RBF GPs over the same N training inputs Z (N x D). */
int sr_gp_create (sr_gp_t* h, int device, int N, int D, int n_out);
int sr_gp_destroy(sr_gp_t h);

/* Z N x D, Y N x n_out, lengthscale n_out x D, signal_var n_out, noise_var n_out (noise_var must
 * already include every diagonal term: sigma_n^2 + noise_diag(1e-5) + GPy's 1e-8 jitter). */
int sr_gp_set_data(sr_gp_t h, const double* Z, const double* Y, const double* lengthscale,
                   const double* signal_var, const double* noise_var, void* stream);

/* Same, for the general kernel family of the reference's non-RBF kernel types
 * (ssm_gpy/gp_models_utils_casadi.py:43-157: mat52, lin_rbf, lin_mat52):
 *   k(x,y) = (c0 + sum_j a_j x_j y_j) * v * kappa(r) + sum_j b_j x_j y_j,  r^2 = sum_j ((x_j - y_j) s_j)^2
 *   kappa(r) = exp(-r^2/2) (0) | (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r) (1)
 * kparams [device]: n_out x (3 + 3 D) doubles, per output [kappa, v, c0, s_1..s_D, a_1..a_D, b_1..b_D]
 * (s_j = 1/lengthscale_j on the dimensions the stationary factor acts on, 0 elsewhere). */
int sr_gp_set_data_general(sr_gp_t h, const double* Z, const double* Y, const double* kparams,
                           const double* noise_var, void* stream);

/* K_d = rbf(Z,Z) + noise I ; K_d = U^T U (blocked fp64-MFMA Cholesky) ; W = U^-T ; alpha = K^-1 y.
 * replaces the GPy posterior the reference caches as inv_K/beta (ssm_gpy/gaussian_process.py:255-275).
 * info [host, n_out ints]: 0, or 1-based index of the first non-positive pivot (then returns SR_ENOTPD).
 * Synchronises the stream before returning. */
int sr_gp_factorize(sr_gp_t h, void* stream, int* info);

/* ---- sparse GP regression (inducing points): the fit that takes the place of sr_gp_factorize ----------------
 * replaces: SparseGPRegression(X, y, Z=Z) behind do_sparse_gp  ssm_gpy/gaussian_process.py:204, 224-243, 397-400.
 * h: created with N = m and given the inducing inputs, the kernel and noise_var = s2 (likelihood variance) by
 * sr_gp_set_data[_general] (its Y is not read).  X N x D, Y N x n_out: ALL data, streamed in chunks of sr_gp_set_chunk rows
 * (<= 16384; workspace n_out x chunk x Np + 2 n_out x Np^2 doubles beside that of sr_gp_factorize, freed on return).
 * Sigma = K_uu + jitter I + K_uf K_fu / s2; alpha = Sigma^-1 K_uf y / s2; Wt = P upper, P P^T = (K_uu + jitter I)^-1 - Sigma^-1.
 * The handle is then factorized AND sparse; repeated fits with one chunk size are bit-identical (another chunk size: equal to
 * rounding).  SR_EINVAL N < m, NULL, jitter < 0; SR_ESTATE no data; SR_ENOTPD + info[d] (as sr_gp_factorize; a pivot of K_uu
 * not above Np eps k_max counts as non-positive); SR_EHIP no workspace.  Synchronises the stream. */
int sr_gp_fit_sparse(sr_gp_t h, const double* X, const double* Y, long N, double jitter, void* stream, int* info);
/* 1 after sr_gp_fit_sparse, 0 otherwise (sr_gp_factorize clears the mark), < 0 on error.  On a sparse handle sr_gp_append,
 * sr_gp_append1_host, sr_gp_remove, sr_gp_loo, sr_gp_mll, sr_gp_logdet and sr_gp_logdet_cached return SR_ESTATE (Wt is not the
 * factor of K_y); sr_gp_inv_k gives P P^T; export / import, predictions, reachability and the server work unchanged.  The
 * exported state does not carry the mark (the packed format is unchanged): the receiver of a sparse model must not append
 * or remove. */
int sr_gp_is_sparse(sr_gp_t h);

/* Condition on m <= 128 ADDITIONAL training points (same hyper-parameters) without refactorising: block row append of
 * the triangular factor, O(N^2 m).  Znew m x D, Ynew m x n_out; info [host, n_out] like sr_gp_factorize.
 * replaces: update_model(x, y, opt_hyp=False, replace_old=False)  ssm_gpy/gaussian_process.py:347-419
 * (the reference refactorises; its own row-append sketch is ssm_pytorch/utilities.py:74-117).
 * On success N grows by m and Np may grow; no buffer of the factor's size is allocated while Np stays.  m <= 16 also leaves
 * log det of the grown model on the host (sr_gp_logdet_cached).  Blocks the host.  Routes by m: docs/HISTORY.md. */
int sr_gp_append(sr_gp_t h, const double* Znew, const double* Ynew, int m, void* stream, int* info);
/* ONE new point given in HOST memory (x_host: D doubles, y_host: n_out doubles; any host memory): the reference's
 * exploration loop after every step (exploration_runner.py:186-188 -> update_model(x, y, replace_old=False)).
 * The point travels in the kernel arguments, status and log det come back through a pinned block: no copy command.
 * Only where a one-launch append applies (<= 8192 padded rows, n_out <= 16, small path on).
 * SR_EUNSUPPORTED otherwise and SR_EBUSY when the grid of co-resident workgroups could not assemble this time -- either
 * way nothing was touched: copy the point to the device and call sr_gp_append.
 * Beyond 512 padded rows, while Np stays, the point is appended IN PLACE (the model's buffers become views one step further
 * into their allocations; calls that rewrite the model, and big batches after an odd number of steps, copy it back first). */
int sr_gp_append1_host(sr_gp_t h, const double* x_host, const double* y_host, void* stream, int* info);

/* Retire m training points (idx_host: m distinct indices into the CURRENT rows, any order, host memory) without
 * refactorising: O(N^2) per point.  The mirror image of the row append: per point ONE bandwidth-bound pass over U^-1 (the
 * product of the Givens rotations that delete a column of the factor of K_y^-1, in closed form), no matrix cores.
 * replaces: update_model(x, y, replace_old=True) on the remaining rows  ssm_gpy/gaussian_process.py:347-419 (the reference
 * can only refit).
 * The points go one at a time, in descending index order.  Afterwards N is m smaller (Np shrinks when N passes a multiple
 * of 128 downward) and sr_gp_padded_n, sr_gp_dims, export, export_packed, inv_k and logdet are those of a handle fitted on
 * the remaining rows in their old order; the same call on the same state gives the same bits.  The new factor is written
 * into the spare buffers of the small appends, so nothing big is allocated while Np stays; scratch (3 Np + 4 doubles per
 * output + N D) is owned by the handle and freed by sr_gp_release_scratch.
 * SR_EINVAL NULL, m < 1, m >= N (at least one point stays), an index outside [0, N) or given twice -- all checked on the
 * host before anything is launched; SR_ESTATE not factorized, a sparse handle, between sr_gp_import_begin and
 * sr_gp_import_end; SR_EHIP no scratch.  On these errors the model is unchanged; a device error in the middle of several
 * removals leaves the points retired so far retired (sr_gp_dims tells).
 * The resident server is taken off the device first and stays armed.  The host copy of log det is invalidated
 * (sr_gp_logdet_cached: SR_ESTATE until the next small append; sr_gp_logdet computes it).  Synchronises the stream. */
int sr_gp_remove(sr_gp_t h, const int* idx_host, int m, void* stream);

/* Leave-one-out posterior of the training rows (Rasmussen & Williams 5.12) from the rows of U^-1, without the explicit
 * inverse: mu_loo, var_loo n_out x N (device; either may be NULL).  var_loo[d][j] = 1 / (K_y^-1)_jj includes the noise term
 * (the predictive variance of the OBSERVATION y_j given the other rows), mu_loo[d][j] = y_j - alpha_j / (K_y^-1)_jj.
 * Factorized, non-sparse handles (SR_ESTATE otherwise).  Asynchronous on `stream`. */
int sr_gp_loo(sr_gp_t h, double* mu_loo, double* var_loo, void* stream);

/* padded leading dimension Np (multiple of 128) of the factor matrices.  The Np - N padding rows and
 * columns are at the FRONT (identity block): training point i has padded index i + (Np - N). */
int sr_gp_padded_n(sr_gp_t h, long* Np);

/* current shape of the model: training points, input dimension, outputs, padded size (any pointer may be NULL) */
int sr_gp_dims(sr_gp_t h, int* N, int* D, int* n_out, long* Np);

/* Export / import the cached posterior state (what a broadcast receiver needs):
 * alpha n_out x N ; Wt n_out x Np x Np = U^-1 (upper triangular, row-major, zero below the diagonal).
 * Either pointer may be NULL.  import marks the handle as factorized. */
int sr_gp_export(sr_gp_t h, double* alpha, double* Wt, void* stream);
int sr_gp_import(sr_gp_t h, const double* alpha, const double* Wt, void* stream);

/* The same state PACKED for the one-time replication to the other GPUs (the reference has no multi-GPU
 * path, so nothing of it is replaced): of U^-1 only the N (N + 1) / 2 entries on and above the diagonal of the real
 * rows travel -- 100 MB instead of 210 MB per output at N = 5000.  Training row i (0 <= i < N) contributes
 * U^-1[i][i .. N-1]; the rows [row0, row1) of output d are packed back to back into buf (sr_gp_packed_count doubles;
 * -1 for a bad range), so a sender can move the factor in bounded pieces through a staging buffer of any size.
 * Receiver: sr_gp_import_begin(alpha n_out x N) after sr_gp_set_data, sr_gp_import_packed for every piece of every
 * output (any order), sr_gp_import_end -> factorized.  Predictions are bit-identical to the sender's. */
long sr_gp_packed_count(sr_gp_t h, long row0, long row1);
int sr_gp_export_packed(sr_gp_t h, int d, long row0, long row1, double* buf, void* stream);
int sr_gp_import_begin(sr_gp_t h, const double* alpha, void* stream);
int sr_gp_import_packed(sr_gp_t h, int d, long row0, long row1, const double* buf, void* stream);
int sr_gp_import_end(sr_gp_t h);

/* explicit (K + noise I)^-1 of output d, N x N -- the reference's `inv_K[d]` attribute
 * (ssm_gpy/gaussian_process.py:258-262).  Cold path; needs factorize() on this handle. */
int sr_gp_inv_k(sr_gp_t h, int d, double* inv_k, void* stream);

/* ---- batched GP posterior ------------------------------------------------------------------
 * replaces: SimpleGPModel.predict / predictive_gradients  ssm_gpy/gaussian_process.py:546-596
 * (formulas: ssm_gpy/gp_models_utils_casadi.py:17-40,160-197).
 * Xq T x D -> mu T x n_out, var T x n_out (clipped at 1e-15), jac T x n_out x D (may be NULL). */
int sr_gp_predict(sr_gp_t h, const double* Xq, long T, double* mu, double* var, double* jac,
                  void* stream);

/* ---- batched posterior with the gradient of the variance -----------------------------------------
 * replaces: predict(states, actions, jacobians=True) for N > 1  state_space_models.py:74-104 (the reference's
 *           backends loop or autograd per batch, ssm_pytorch/gaussian_process.py:280-292), and GPy's
 *           predictive_gradients(x, grad_sigma=True)  (ssm_gpy/gaussian_process.py:570-596 raises there).
 * Xq T x D -> mu T x n_out, var T x n_out (as sr_gp_predict), jac_mu T x n_out x D (may be NULL),
 * jac_var T x n_out x D (d var/dx).  One tiled pass per chunk of sr_gp_set_chunk queries: the variance contraction
 * also stores V = U^-T K*, a second triangular product G = U^-1 V = K_y^-1 K* is reduced on the fly against dk(Z, x)/dx.
 * About twice the matrix-core work of sr_gp_predict.  All kernel identifiers, any n_out, D <= 8 (SR_EUNSUPPORTED beyond).
 * Memory: a grow-only workspace of n_out x Np x chunk doubles (V, the size of the K* slab) and
 * n_out x Np/128 x D x chunk doubles, owned by the handle and freed by sr_gp_release_scratch. */
int sr_gp_predict_grad(sr_gp_t h, const double* Xq, long T, double* mu, double* var, double* jac_mu,
                       double* jac_var, void* stream);

/* ---- batched second-order linearisation: the Hessian of the mean for a batch of queries ----------------
 * replaces: a loop of linearize_predict(states 1xn, actions 1xm, jacobians=True) over the rows of a batch
 *           (state_space_models.py:106-138; ssm_pytorch/gaussian_process.py:333-385 builds the Hessian per output by autograd).
 * Xq T x D -> mu, var (T x n_out), jac_mu, jac_var (T x n_out x D): bit-identical to sr_gp_predict_grad on the same
 * inputs; hess_mu (T x n_out x D x D), exactly symmetric.  Per chunk of sr_gp_set_chunk queries the pass of
 * sr_gp_predict_grad, then one pass over the chunk's K* slab (ARD-RBF) or over Z (the general family) that sums
 * alpha_i d2 k(x_t, z_i)/dx2 in centred coordinates z_i - x_t.  All kernel identifiers, any n_out, D <= 8
 * (SR_EUNSUPPORTED beyond: sr_gp_linearize serves one query of any D).  No pointer may be NULL (T = 0 excepted).
 * Memory: the workspace of sr_gp_predict_grad and a grow-only n_split x n_out x (D (D + 1) / 2 + 1) x chunk doubles of
 * partial sums, owned by the handle and freed by sr_gp_release_scratch. */
int sr_gp_linearize_batch(sr_gp_t h, const double* Xq, long T, double* mu, double* var,
                          double* jac_mu, double* jac_var, double* hess_mu, void* stream);

/* ---- greedy max-variance subset (choose_datapoints_maxvar) by pivoted Cholesky downdates ----
 * X n x D (device): the pool.  init_idx k (device, distinct, 0 <= i < n, k >= 1): forced first pivots, in order.
 * idx m (device): the k seeds then m - k greedy picks; score m (device, may be NULL): Sigma_d var_d(pick) just
 * before it was picked (seeds: the same quantity).  Kernel and noise are the handle's (sr_gp_set_data*), its
 * training rows are not read.  k <= m <= n.  One launch per round, no host synchronisation.
 * replaces: the greedy loop of ssm_gpy/gaussian_process.py:323-343 with fixed hyper-parameters.  Pivot = first argmax of
 * Sigma_d max(var_d, 1e-15) over the rows not taken (ties: the smaller row); repeated calls are bit-identical.  The k seeds
 * are read back once and checked before anything is launched (SR_EINVAL: k < 1, k > m, m > n, a seed outside [0, n) or
 * twice).  Memory: grow-only n_out x (m - 1) x n (padded to 64) doubles of the factor and n_out x n more, owned by the
 * handle and freed by sr_gp_release_scratch; SR_EHIP when they cannot be allocated. */
int sr_gp_select_maxvar(sr_gp_t h, const double* X, long n, int m, const int* init_idx, int k,
                        int* idx, double* score, void* stream);

/* ---- single query with second-order outputs (the CasADi Jacobian callback) ------------------------
 * replaces: linearize_predict(states 1xn, actions 1xm, jacobians=True)  state_space_models.py:106-138,
 *           consumed at :402-415; reference implementation ssm_pytorch/gaussian_process.py:333-385.
 * x D -> mu n_out, var n_out, jac_mu n_out x D, jac_var n_out x D (d var/dx), hess_mu n_out x D x D.
 * All kernel identifiers (rbf, mat52, lin_rbf, lin_mat52) in closed form. */
int sr_gp_linearize(sr_gp_t h, const double* x, double* mu, double* var, double* jac_mu,
                    double* jac_var, double* hess_mu, void* stream);

/* ---- GP input transform ---------------------------------------------------------------------------
 * replaces: the t_z_gp / a_gp_inp_x arguments of gp_reachability_casadi.onestep_reachability (:60-61,85,94-97) and
 * uncertainty_propagation_casadi.one_step_taylor (:40-47,60): the GP is evaluated at x_gp = Tz x (the journal's cart-pole
 * model drops the cart position: D = 4), its state Jacobian is jac[:, :n_x_in] Tz.  Tz [device] n_x_in x n_out (copied);
 * NULL restores the identity.  While set, the reachability / moment entry points below use n_s = n_out,
 * n_u = D - n_x_in.  Plain predictions are not affected. */
int sr_gp_set_input_transform(sr_gp_t h, const double* Tz, int n_x_in, void* stream);

/* ---- one-step reachability, batched over T queries ------------------------------------------
 * replaces: gp_reachability.onestep_reachability  gp_reachability.py:19-156  (+ utils.py:108-144,
 *   utils_ellipsoid.py:63-94,197-233)
 * p T x n_s ; q T x n_s x n_s or NULL (point branch) ; k_ff T x n_u ; k_fb T x n_u x n_s (required iff q != NULL) ;
 * a n_s x n_s ; b n_s x n_u ; l_mu, l_sigma n_s.  -> p_out T x n_s ; q_out T x n_s x n_s ; var_out T x n_s or NULL.
 * n_bad: device int or NULL, atomically incremented once per query whose box half-widths were not all > 0 -- where the
 * reference raises AssertionError (utils_ellipsoid.py:226-228).  The caller zeroes it. */
int sr_onestep_reach(sr_gp_t h, long T, const double* p, const double* q, const double* k_ff,
                     const double* k_fb, const double* a, const double* b, const double* l_mu,
                     const double* l_sigma, double c_safety, double* p_out, double* q_out,
                     double* var_out, int* n_bad, void* stream);

/* ---- multi-step reachability, batched over T trajectories ------------------------------------
 * replaces: gp_reachability.multistep_reachability  gp_reachability.py:159-212
 * p0 T x n_s ; q0 T x n_s x n_s or NULL ; k_fb0 T x n_u x n_s or NULL (required iff q0 != NULL) ;
 * k_ff T x H x n_u ; k_fb T x (H-1) x n_u x n_s (may be NULL when H == 1).
 * -> p_all T x H x n_s ; q_all T x H x n_s x n_s. */
int sr_multistep_reach(sr_gp_t h, long T, int H, const double* p0, const double* q0,
                       const double* k_fb0, const double* k_ff, const double* k_fb, const double* a,
                       const double* b, const double* l_mu, const double* l_sigma, double c_safety,
                       double* p_all, double* q_all, int* n_bad, void* stream);

/* ---- ellipsoid step alone (GP outputs supplied by the caller: any StateSpaceModel) -----------
 * replaces: the algebra of gp_reachability.py:65-156 after `ssm(x, u)` returned.
 * mu T x n_s ; var T x n_s ; jac T x n_s x (n_s+n_u) (ignored in the point branch, may be NULL). */
int sr_ellipsoid_step(int device, long T, int n_s, int n_u, const double* p, const double* q,
                      const double* k_ff, const double* k_fb, const double* mu, const double* var,
                      const double* jac, const double* a, const double* b, const double* l_mu,
                      const double* l_sigma, double c_safety, double* p_out, double* q_out,
                      int* n_bad, void* stream);

/* ---- reverse pass of ONE reachability step (beyond the reference, whose MPC differentiates a CasADi graph of the same lines,
 * one problem at a time) -------------------------------------------------------------------------------------------------
 * sr_ellipsoid_step_vjp: the vector-Jacobian product of sr_ellipsoid_step, both branches.  Forward inputs as there (q NULL =
 * point branch; k_fb and jac required iff q != NULL).  For seeds p1_bar T x n_s and q1_bar T x n_s x n_s (either NULL = zero,
 * with the same bits as a zero array; not both) the derivatives of
 *   L = sum_t p1_bar[t] . p_out[t] + sum_ij q1_bar[t]_ij q_out[t]_ij
 * in the inputs:  p_bar T x n_s ; q_bar T x n_s x n_s ; kff_bar T x n_u ; kfb_bar T x n_u x n_s ; mu_bar, var_bar T x n_s ;
 * jac_bar T x n_s x (n_s+n_u).  q_bar and kfb_bar are meaningless in the point branch and may be NULL there (zero-filled when
 * given, and so is jac_bar, which may be NULL there too).  a, b, l_mu, l_sigma, c_safety get no derivative.
 * Only the symmetric part of q1_bar counts.  q_bar is exactly symmetric: the gradient of the function extended to unsymmetric
 * arguments by q -> (q + q^T) / 2.  Nothing is saved by the forward; H, Q0, r^2, c1, c2 are recomputed.
 * r^2 = lambda_max(Q (I + K^T K)) is differentiated through its top eigenvector (accumulated Jacobi rotations):
 *   d r^2 / dQ = w w^T,  d r^2 / dK = 2 r^2 (K v) v^T   (w, v the left / right eigenvector of Q (I + K^T K), w . v = 1).
 * Where the top eigenvalue is repeated r^2 is not differentiable: the formulas are evaluated at the unit vector of the top
 * eigenspace the iteration found -- an element of the generalised gradient, finite; near a tie the rounding error of what
 * passes through r^2 grows as lambda_1 / (lambda_1 - lambda_2).
 * A query whose box half-widths are not all > 0 (the queries sr_ellipsoid_step counts in n_bad) gets NaN in every output of
 * that query; no other query is affected.  (var_i = 0 in the ellipsoid branch is no such query, but d sqrt(var)/d var is infinite
 * there: var_bar_i is +-inf, or NaN under a zero seed, and the rest of the query is finite.)  n_s <= 8, n_u <= 4 (SR_EUNSUPPORTED beyond); SR_EINVAL: NULL where required, q
 * without k_fb / jac, both seeds NULL, T < 0; T == 0 is a no-op.  Asynchronous on `stream`; one thread per query, no atomics. */
int sr_ellipsoid_step_vjp(int device, long T, int n_s, int n_u, const double* p, const double* q, const double* k_ff,
                          const double* k_fb, const double* mu, const double* var, const double* jac, const double* a,
                          const double* b, const double* l_mu, const double* l_sigma, double c_safety,
                          const double* p1_bar, const double* q1_bar, double* p_bar, double* q_bar, double* kff_bar,
                          double* kfb_bar, double* mu_bar, double* var_bar, double* jac_bar, void* stream);
/* sr_onestep_reach_vjp: the reverse pass of sr_onestep_reach, GP included: seeds on (p_out, q_out) as above -> p_bar, q_bar,
 * kff_bar, kfb_bar (q_bar, kfb_bar may be NULL in the point branch).  Per chunk of sr_gp_set_chunk queries: z = [Tz p; k_ff]
 * (Tz: sr_gp_set_input_transform, else the identity), sr_gp_linearize_batch at z into a grow-only scratch owned by the handle
 * (freed by sr_gp_release_scratch), then ONE launch with the reverse of the ellipsoid algebra and the GP link
 *   z_bar = sum_a jac_mu[a] mu_bar[a] + jac_var[a] var_bar[a] + sum_{a,d} jac_z_bar[a][d] hess_mu[a][d],
 *   p_bar += Tz^T z_bar[:n_x_in],  kff_bar += z_bar[n_x_in:].
 * The model rules are those of sr_gp_linearize_batch: every kernel identifier, exact and sparse handles, D <= 8
 * (SR_EUNSUPPORTED beyond).  The GP outputs the step is differentiated at are those of the linearisation pass (equal to the
 * forward's up to the rounding of another route).  The derivative ignores the clip of the predictive variance at 1e-15.
 * The same inputs give the same bits for ANY chunk size.  The new kernels work one query per thread.  The linearisation pass splits
 * its sums over the training rows by the width of the batch it is given (K* pass: min(Np / 16, ceil(768 / b)) splits, Hessian pass:
 * min(ceil(N / 32), ceil(1024 / b)), b = n_out ceil(width / 256)) and its final stage sums in another order beyond 4096 queries, so
 * this entry point gives it at most min(chunk, 256 k) queries at a time, k = clamp(min(768 / (Np / 16), 1024 / ceil(N / 32)) / n_out,
 * 1, 16): up to there both split counts are the ones set by the model size alone (k = 1: a width of 256 is one block whatever
 * the chunk).  Small models go through whole (N = 150, n_out = 4: 3072 queries per pass), big ones in passes of 256 (N = 5000).
 * In the point branch the Hessian is not read and the pass is sr_gp_predict_grad's.
 * SR_ESTATE not factorized; SR_EINVAL NULL where required, q != NULL without k_fb,
 * both seeds NULL, T < 0; T == 0 is a no-op.  Asynchronous on `stream`. */
int sr_onestep_reach_vjp(sr_gp_t h, long T, const double* p, const double* q, const double* k_ff, const double* k_fb,
                         const double* a, const double* b, const double* l_mu, const double* l_sigma, double c_safety,
                         const double* p1_bar, const double* q1_bar, double* p_bar, double* q_bar, double* kff_bar,
                         double* kfb_bar, void* stream);
/* sr_multistep_reach_vjp: the reverse pass of sr_multistep_reach, GP included.  The forward arguments are exactly those of
 * sr_multistep_reach (q0 == NULL: step 0 is the point branch; k_fb0 required iff q0 is given; k_fb may be NULL when H == 1);
 * p_all T x H x n_s and q_all T x H x n_s x n_s are what it returned.  Seeds p_all_bar, q_all_bar of those shapes (either NULL =
 * zero, the same bits; not both).  With L = sum p_all_bar . p_all + sum q_all_bar . q_all the outputs are dL/dp0 (T x n_s), dL/dq0
 * (T x n_s x n_s), dL/dk_fb0 (T x n_u x n_s), dL/dk_ff (T x H x n_u) and dL/dk_fb (T x (H-1) x n_u x n_s; may be NULL when H == 1).
 * q0_bar and kfb0_bar may be NULL in a point start (zero-filled where given), and are required with q0.
 * Per trajectory, for i = H-1 .. 0: the seed of step i is (p_all_bar, q_all_bar)[i] plus the (p_bar, q_bar) step i+1 produced; the
 * step is differentiated by the formulas of sr_onestep_reach_vjp -- the same device functions -- at its inputs (p_{i-1}, q_{i-1},
 * k_ff_i, k_fb_{i-1}), step 0 at (p0, q0, k_fb0) or in the point branch; the GP link adds Tz^T z_bar[:n_x_in] to p_bar and
 * z_bar[n_x_in:] to kff_bar[i].  The conventions are those of sr_onestep_reach_vjp: only the symmetric part of a q seed counts (the
 * seed is symmetrised before the carried q_bar is added: a seed and its symmetric part give the same bits), q0_bar is exactly
 * symmetric, the variance clip is ignored, r^2 is differentiated through its top eigenvector.
 * Structure: trajectories in groups of max(1, chunk / H) (sr_gp_set_chunk).  Per group ONE launch forms z_i = [Tz p_{i-1}; k_ff_i]
 * of every (trajectory, step) pair -- the centres do not depend on the sweep --, sr_gp_linearize_batch runs over all of them into
 * the grow-only scratch of sr_onestep_reach_vjp, in passes of at most min(chunk, 256 k) queries exactly as there (the split counts
 * depend on the model alone), the Hessian of the mean included (not read at step 0 of a point start); ONE launch finds r^2 and its eigenvectors of every
 * (trajectory, step) pair, which depend on no seed; then ONE launch sweeps, one thread per trajectory.  No atomics, no waiting
 * between workgroups, sums in a fixed order: the same bits on every call and for ANY chunk size.
 * A (trajectory, step) pair whose box half-widths are not all > 0 (the ones sr_multistep_reach counts in n_bad) gets NaN as in
 * sr_onestep_reach_vjp, and the NaN reaches every gradient of that trajectory that flows through that step -- kff_bar[t][:i+1],
 * kfb_bar[t][:i], p0_bar[t], q0_bar[t], kfb0_bar[t]; the gradients of later steps and of other trajectories are untouched.
 * Every kernel identifier, exact and sparse handles and the input transform are accepted.  Before any launch: SR_EINVAL NULL where
 * required, q0 without k_fb0 / q0_bar / kfb0_bar, both seeds NULL, H < 1, T < 0; SR_ESTATE not factorized; SR_EUNSUPPORTED D > 8,
 * n_s > 8, n_u > 4; T == 0 is a no-op.  Asynchronous on `stream`. */
int sr_multistep_reach_vjp(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                           const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
                           const double* l_sigma, double c_safety, const double* p_all, const double* q_all,
                           const double* p_all_bar, const double* q_all_bar, double* p0_bar, double* q0_bar, double* kfb0_bar,
                           double* kff_bar, double* kfb_bar, void* stream);
/* ---- the GP variances of a reachability roll-out (the reference's third output, gp_pred_sigma_all) and their seed ----------------
 * sr_multistep_reach_var: sr_multistep_reach with one more output, gp_var_all T x H x n_s (or NULL): gp_var_all[t][i] is the
 * predictive variance step i used, at z_i = [Tz p_{i-1}; k_ff_i], clipped at 1e-15 as everywhere.  The same driver and the same
 * routes (the persistent chain where it applies, else per-step launches): p_all, q_all and n_bad are the bits of sr_multistep_reach
 * on whichever route the call takes, with and without gp_var_all.  Refusals as sr_multistep_reach. */
int sr_multistep_reach_var(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0, const double* k_ff,
                           const double* k_fb, const double* a, const double* b, const double* l_mu, const double* l_sigma,
                           double c_safety, double* p_all, double* q_all, double* gp_var_all, int* n_bad, void* stream);
/* sr_multistep_reach_var_vjp: sr_multistep_reach_vjp with a third seed, gpvar_all_bar T x H x n_s on the variances above:
 *   L = sum p_all_bar . p_all + sum q_all_bar . q_all + sum gpvar_all_bar . gp_var_all.
 * Any seed NULL = zero; all three NULL is SR_EINVAL.  In the sweep gpvar_all_bar[t][i] is added to the var_bar of step i after the
 * step's reverse algebra has written it and before the GP link reads it (z_bar += jac_var^T gpvar_all_bar[t][i]); the clip of the
 * variance is ignored, as in every reverse pass here.  A step that is a bound violation has a NaN var_bar, which stays NaN: under a
 * seed on the variances alone the NaN reaches exactly what it reaches under any seed -- kff_bar[t][:i+1], kfb_bar[t][:i], p0_bar[t],
 * q0_bar[t], kfb0_bar[t] -- and nothing else.  Everything else is the contract of sr_multistep_reach_vjp: outputs, symmetry
 * conventions, grouping, pass width, the same bits on every call and for any chunk size, D <= 8, n_s <= 8, n_u <= 4.  With
 * gpvar_all_bar == NULL the add is not executed at all and the outputs are the bits of sr_multistep_reach_vjp, which itself keeps
 * returning the bits it returned before this entry point existed. */
int sr_multistep_reach_var_vjp(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                               const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
                               const double* l_sigma, double c_safety, const double* p_all, const double* q_all,
                               const double* p_all_bar, const double* q_all_bar, const double* gpvar_all_bar, double* p0_bar,
                               double* q0_bar, double* kfb0_bar, double* kff_bar, double* kfb_bar, void* stream);

/* ---- Gaussian moment propagation (the CautiousMPC baseline), batched -----------------------------
 * replaces: uncertainty_propagation_casadi.one_step_taylor / multi_step_taylor_symbolic (mode 1)
 *           uncertainty_propagation_casadi.one_step_mean_equivalent / mean_equivalent_multistep (mode 2)
 *           uncertainty_propagation_casadi.py:11-283 (numeric evaluation of the symbolic graphs)
 * Step 0 starts from a point (sigma_0 = None is the only case the reference implements, :124,:170);
 * step i >= 1 uses k_fb[i-1].  mu0 T x n_s ; k_ff T x H x n_u ; k_fb T x (H-1) x n_u x n_s
 * -> mu_all T x H x n_s ; sigma_all T x H x n_s x n_s ; gp_var_all T x H x n_s (GP variances, or NULL). */
int sr_multistep_moments(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* k_ff,
                         const double* k_fb, const double* a, const double* b, double* mu_all,
                         double* sigma_all, double* gp_var_all, void* stream);
/* one step with the GP outputs supplied by the caller (sigma_x NULL = point input). */
int sr_moment_step(int device, long T, int n_s, int n_u, int mode, const double* mu_x,
                   const double* sigma_x, const double* k_ff, const double* k_fb, const double* mu_g,
                   const double* var_g, const double* jac_g, const double* a, const double* b,
                   double* mu_out, double* sigma_out, void* stream);
/* sr_onestep_moments: one step with the GP inside, from a point (sigma_x NULL) or from N(mu_x, sigma_x) -- what
 * sr_multistep_moments cannot start from.  mu_x T x n_s ; sigma_x T x n_s x n_s ; k_ff T x n_u ; k_fb T x n_u x n_s (required iff
 * sigma_x != NULL) -> mu_out T x n_s ; sigma_out T x n_s x n_s ; var_out T x n_s (GP variances, or NULL).  u = k_ff, the GP is
 * evaluated at z = [Tz mu_x; k_ff] (Tz: sr_gp_set_input_transform, else the identity).  No new kernel: per chunk of
 * sr_gp_set_chunk the launches of one step of sr_multistep_moments on its per-step route (the posterior with its Jacobian into
 * the handle's workspace, then the moment step), so H calls in a row give the bits of that route.
 * SR_ESTATE not factorized; SR_EINVAL NULL where required, sigma_x without k_fb, T < 0, mode outside {1, 2}; T == 0 is a no-op;
 * n_s <= 8, n_u <= 4 (SR_EUNSUPPORTED beyond).  Asynchronous on `stream`. */
int sr_onestep_moments(sr_gp_t h, long T, int mode, const double* mu_x, const double* sigma_x, const double* k_ff,
                       const double* k_fb, const double* a, const double* b, double* mu_out, double* sigma_out,
                       double* var_out, void* stream);

/* ---- reverse pass of ONE moment step, modes 1 and 2 (beyond the reference, whose CautiousMPC differentiates a CasADi graph of the
 * same lines, one problem at a time) ---------------------------------------------------------------------------------------
 * sr_moment_step_vjp: the vector-Jacobian product of sr_moment_step, both starts.  Forward inputs as there (sigma_x NULL = point
 * start; k_fb required iff sigma_x != NULL, jac_g iff sigma_x != NULL in mode 1 -- it is never read in mode 2).  With
 *   mu1 = a mu_x + b k_ff + mu_g ,  Sigma1 = H Sigma H^T + diag(var_g) ,  H = a + J_x + (b + J_u) K (mode 1) or a + b K (mode 2)
 * and seeds mu1_bar T x n_s, sigma1_bar T x n_s x n_s (either NULL = zero, with the same bits as a zero array; not both), S its
 * symmetric part, the derivatives of  L = sum_t mu1_bar[t] . mu_out[t] + sum_ij sigma1_bar[t]_ij sigma_out[t]_ij  in the inputs:
 *   mux_bar = a^T mu1_bar ; kff_bar = b^T mu1_bar ; mug_bar = mu1_bar ; var_bar_i = S_ii ;
 *   sigma_bar = H^T S H ; with H_bar = 2 S H sym(Sigma):  jac_bar = [H_bar, H_bar K^T], kfb_bar = (J_u + b)^T H_bar (mode 1),
 *   jac_bar = 0, kfb_bar = b^T H_bar (mode 2).
 * At a point start jac_bar, sigma_bar and kfb_bar are zero: they may be NULL there and are zero-filled where given.  sigma_x is
 * read as (Sigma + Sigma^T) / 2 and sigma_bar is exactly symmetric: the gradient of the function extended to unsymmetric
 * arguments that way.  Only the symmetric part of sigma1_bar counts.  a and b get no derivative.  Nothing is saved by the
 * forward; H is recomputed.  There is no square root in these modes: no query is refused and nothing is NaN that was not.
 * n_s <= 8, n_u <= 4 (SR_EUNSUPPORTED beyond); SR_EINVAL: NULL where required, sigma_x without k_fb / jac_g (mode 1) / sigma_bar /
 * kfb_bar / jac_bar, both seeds NULL, T < 0, mode outside {1, 2}; T == 0 is a no-op.  Asynchronous on `stream`; one thread per
 * query, no atomics, sums in a fixed order. */
int sr_moment_step_vjp(int device, long T, int n_s, int n_u, int mode, const double* mu_x, const double* sigma_x,
                       const double* k_ff, const double* k_fb, const double* mu_g, const double* var_g, const double* jac_g,
                       const double* a, const double* b, const double* mu1_bar, const double* sigma1_bar, double* mux_bar,
                       double* sigma_bar, double* kff_bar, double* kfb_bar, double* mug_bar, double* var_bar, double* jac_bar,
                       void* stream);
/* sr_onestep_moments_vjp: the reverse pass of sr_onestep_moments, GP included: seeds on (mu_out, sigma_out) as above and
 * gpvar_bar T x n_s on var_out (var_bar_i = S_ii + gpvar_bar_i; any seed NULL = zero, not all three) -> mux_bar, sigma_bar,
 * kff_bar, kfb_bar (sigma_bar, kfb_bar may be NULL at a point start).  Per pass: z = [Tz mu_x; k_ff], the GP derivatives at z
 * into the grow-only scratch of sr_onestep_reach_vjp (freed by sr_gp_release_scratch), then ONE launch with the reverse of the
 * moment algebra and the GP link of sr_onestep_reach_vjp
 *   z_bar = sum_a jac_mu[a] mug_bar[a] + jac_var[a] var_bar[a] + sum_{a,d} jac_z_bar[a][d] hess_mu[a][d],
 *   mux_bar += Tz^T z_bar[:n_x_in],  kff_bar += z_bar[n_x_in:].
 * The Hessian term is there only where jac_bar is not zero, mode 1 from a Gaussian start: that case runs sr_gp_linearize_batch,
 * every other one (mode 2, point starts) sr_gp_predict_grad.  The width of a pass is bounded exactly as in sr_onestep_reach_vjp
 * (see there), so the same inputs give the same bits for ANY chunk size.  Model rules of sr_gp_linearize_batch in every case:
 * every kernel identifier, exact and sparse handles, D <= 8 (SR_EUNSUPPORTED beyond).  The GP outputs the step is differentiated
 * at are those of this pass (equal to the forward's up to the rounding of another route); the clip of the predictive variance
 * at 1e-15 is ignored.  SR_ESTATE not factorized; SR_EINVAL NULL where required, sigma_x without k_fb / sigma_bar / kfb_bar,
 * every seed NULL, T < 0, mode outside {1, 2}; T == 0 is a no-op.  Asynchronous on `stream`. */
int sr_onestep_moments_vjp(sr_gp_t h, long T, int mode, const double* mu_x, const double* sigma_x, const double* k_ff,
                           const double* k_fb, const double* a, const double* b, const double* mu1_bar,
                           const double* sigma1_bar, const double* gpvar_bar, double* mux_bar, double* sigma_bar,
                           double* kff_bar, double* kfb_bar, void* stream);
/* sr_multistep_moments_vjp: the reverse pass of a whole Taylor (mode 1) / mean-equivalent (mode 2) roll-out, GP included.  The
 * forward arguments are those of sr_multistep_moments with an optional sigma0 T x n_s x n_s: sigma0 == NULL, step 0 starts from a
 * point (what sr_multistep_moments computes); sigma0 given, the roll-out starts from N(mu0, sigma0) and step 0 has a zero gain (H
 * rounds of sr_onestep_moments, the first with k_fb = 0).  Step i >= 1 uses k_fb[i-1]; k_fb and kfb_bar may be NULL when H == 1.
 * mu_all T x H x n_s and sigma_all T x H x n_s x n_s are what either forward returned (the two agree to rounding): step i is
 * differentiated at the stored (mu_{i-1}, Sigma_{i-1}), step 0 at (mu0, sigma0) or in the point branch.
 * Seeds mu_all_bar, sigma_all_bar, gpvar_all_bar (T x H x n_s) shaped like the three forward outputs (any NULL = zero, the same
 * bits; not all three).  With L = sum mu_all_bar . mu_all + sum sigma_all_bar . sigma_all + sum gpvar_all_bar . gp_var_all the
 * outputs are dL/dmu0 (T x n_s), dL/dsigma0 (T x n_s x n_s, exactly symmetric; required iff sigma0 is given, not read otherwise),
 * dL/dk_ff (T x H x n_u) and dL/dk_fb (T x (H-1) x n_u x n_s).  a, b and the model get no derivative.
 * Per trajectory, for i = H-1 .. 0: the seed of step i is the caller's seed on step i plus the (mu_bar, sigma_bar) step i+1
 * produced; the step is differentiated by the formulas of sr_onestep_moments_vjp -- the same device functions --; the GP link adds
 * Tz^T z_bar[:n_x_in] to mu_bar and z_bar[n_x_in:] to kff_bar[i].  The conventions are those of sr_onestep_moments_vjp: only the
 * symmetric part of a sigma seed counts (the seed is symmetrised before the carried sigma_bar is added: a seed and its symmetric
 * part give the same bits), the clip of the GP variance at 1e-15 is ignored, there is no square root: nothing is NaN that was not.
 * Structure: trajectories in groups of max(1, chunk / H) (sr_gp_set_chunk), at most 2^28 doubles of scratch.  Per group ONE launch
 * forms z_n = [Tz mu_in; k_ff[t][i]], n = t H + i, of every (trajectory, step) pair with the step's (Sigma_in, K_in) dense in n
 * (the launch of sr_multistep_reach_vjp); the GP derivatives of all pairs go into the grow-only scratch of sr_onestep_reach_vjp, in
 * passes of at most min(chunk, 256 k) queries exactly as there (the split counts depend on the model alone): sr_gp_linearize_batch
 * in mode 1 (the Hessian of the mean is read at steps with a Gaussian input only), sr_gp_predict_grad in mode 2 and for H == 1 from
 * a point; then ONE launch sweeps, one thread per trajectory in workgroups of one wavefront.  No atomics, no waiting between
 * workgroups, sums in a fixed order: the same bits on every call, for ANY chunk size and whatever other trajectories are in the batch.
 * Every kernel identifier, exact and sparse handles and the input transform are accepted.  Before any launch: SR_EINVAL NULL where
 * required, sigma0 without sigma0_bar, every seed NULL, mode outside {1, 2}, H < 1, T < 0; SR_ESTATE not factorized;
 * SR_EUNSUPPORTED D > 8, n_s > 8, n_u > 4; T == 0 is a no-op.  Asynchronous on `stream`. */
int sr_multistep_moments_vjp(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* sigma0, const double* k_ff,
                             const double* k_fb, const double* a, const double* b, const double* mu_all, const double* sigma_all,
                             const double* mu_all_bar, const double* sigma_all_bar, const double* gpvar_all_bar, double* mu0_bar,
                             double* sigma0_bar, double* kff_bar, double* kfb_bar, void* stream);

/* ---- exact moment matching: the GP at Gaussian inputs (beyond the reference, which has the two approximations above) ----
 * For T inputs z ~ N(m[t], S[t]) (m T x D; S T x D x D symmetric PSD, may be singular; NULL = all zero) the exact mean,
 * the FULL covariance across outputs and the expected Jacobian of an ARD-RBF model (Deisenroth's closed forms), or of a
 * general-family model (sr_gp_set_data_general) whose radial part is the RBF (kappa id 0) on EVERY output -- the reference's
 * lin_rbf, and rbf outputs beside it: a polynomial of degree <= 1 times a Gaussian plus a bilinear term, whose expectations are
 * Gaussian moments of order <= 2 (entries of s may be zero; nothing inverts S or diag(s^2)):
 *   mu T x n_out ; cov T x n_out x n_out (exactly symmetric, diagonal clipped at 1e-15; exactly zero off the diagonal where
 *   S[t] == 0) ; V T x n_out x D (may be NULL): cov(z, g_a) = S V_a, and V_a -> d mu_a/dx as S -> 0.
 * inv_k n_out x N x N: the matrices sr_gp_inv_k writes, back to back (on a sparse handle: P P^T, the matrix of its variance).
 * Cost: T n_out (n_out + 1) / 2 N^2 evaluations of exp (general family: about twice the time per evaluation, and once per call
 * the products inv_k Z, O(n_out N^2 D)); queries go through in chunks of sr_gp_set_chunk with a grow-only scratch owned by the
 * handle (freed by sr_gp_release_scratch).  Asynchronous on `stream` (the first call after sr_gp_set_data_general reads the
 * radial identifiers back: one blocking copy); the same inputs give the same bits, for any chunk size.
 * SR_ESTATE not factorized; SR_EUNSUPPORTED a general-family model with a Matern output (no closed form; the error text names
 * ARD-RBF); SR_EINVAL NULL argument or T < 0; T == 0 is a no-op. */
int sr_gp_moment_match(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k,
                       double* mu, double* cov, double* V, void* stream);
/* Its reverse pass (vector-Jacobian product): for seeds mu_bar T x n_out, cov_bar T x n_out x n_out, V_bar T x n_out x D (any of
 * them NULL = zero, with the same bits as a zero array) the derivatives of
 *   L = sum_t mu_bar[t] . mu[t] + sum_ab cov_bar[t]_ab cov[t]_ab + sum_a V_bar[t]_a . V[t]_a
 * in the inputs:  m_bar T x D = dL/dm ; S_bar T x D x D = dL/dS (either may be NULL, not both).  m, S (NULL = zero) and inv_k as
 * above.  Only the symmetric part of cov_bar counts.  S_bar is exactly symmetric: the gradient of the function extended to
 * unsymmetric arguments by S -> (S + S^T) / 2 (what autograd gives when the forward symmetrises).  The clip of the covariance
 * diagonal at 1e-15 is ignored by the derivative, and so is the exact zero the forward writes off the diagonal at S == 0:
 * d cov_ab / dS is not zero there, so the pair sums run for every pair.  Nothing inverts S: singular and zero S are fine.
 * Cost: T n_out^2 N^2 evaluations of exp (about four forward calls); chunks, scratch, determinism (the same bits for any
 * chunk size) and refusals as sr_gp_moment_match, except that EVERY general-family handle is SR_EUNSUPPORTED: the reverse pass
 * of the family is not provided.  SR_EINVAL also when both outputs are NULL.  Asynchronous on `stream`. */
int sr_gp_moment_match_vjp(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k,
                           const double* mu_bar, const double* cov_bar, const double* V_bar,
                           double* m_bar, double* S_bar, void* stream);
/* sr_gp_moment_match_rollout: T trajectories through H closed-loop steps of exact moment matching in ONE launch (a workgroup
 * owns a trajectory for the whole horizon; what H rounds of sr_gp_moment_match with the algebra between them compute, to
 * rounding, not bit for bit).  n_s = n_out, n_u = D - n_x_in >= 1.  State N(mu, Sigma), control u = K x + k_ff, G = [tz; K]:
 *   GP input m_z = [tz mu; K mu + k_ff], S_z = G Sigma G^T (step 0: K = 0; a point start: no S_z); mu_g, Cov, V as above;
 *   mu+ = (a + b K) mu + b k_ff + mu_g ; Sigma+ = Hm Sigma Hm^T + Cov - (V G) Sigma (V G)^T, Hm = a + b K + V G (Cov from a point).
 * mu0 T x n_s; sigma0 NULL (points) or T x n_s x n_s; k_ff [T x] H x n_u; k_fb [T x] (H - 1) x n_u x n_s (may be NULL when H == 1;
 * step i >= 1 uses k_fb[i - 1]); gains_per_traj 0: one policy for all trajectories, 1: one per trajectory; a n_s x n_s; b n_s x n_u;
 * tz NULL (identity: n_x_in == n_s) or n_x_in x n_s; inv_k as above.  Outputs: mu_all T x H x n_s; sigma_all T x H x n_s x n_s
 * (exactly symmetric); cov_all NULL or T x H x n_s x n_s, the GP's output covariance per step (diagonal clipped at 1e-15, exact
 * zeros off it at step 0 from a point).  The same bits on every call, with and without cov_all; the first h steps equal the
 * h-step call; a trajectory's result does not depend on the other trajectories of the batch nor on sr_gp_set_chunk (which only
 * sizes the scratch: one step's records per trajectory, freed by sr_gp_release_scratch).  Asynchronous on `stream`.
 * Errors, before any launch: SR_EINVAL NULL where required, T < 0, H < 1, gains_per_traj outside {0, 1}, n_x_in outside
 * 1 .. D - 1, tz NULL with n_x_in != n_s; SR_ESTATE not factorized; SR_EUNSUPPORTED any general-family handle, N > 1024 (a
 * step is milliseconds of double sum there), D > 12, a state block beyond the workgroup's LDS (n_s of about 20): the error text
 * names the per-step route.  T == 0 is a no-op. */
int sr_gp_moment_match_rollout(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj,
        const double* mu0, const double* sigma0, const double* k_ff, const double* k_fb,
        const double* a, const double* b, const double* tz, const double* inv_k,
        double* mu_all, double* sigma_all, double* cov_all, void* stream);
/* sr_gp_moment_match_rollout_vjp: the reverse pass of that roll-out, the gradient of
 *   L = sum mu_all_bar . mu_all + sum sigma_all_bar . sigma_all + sum cov_all_bar . cov_all      (cov the unclipped closed form)
 * in mu0, sigma0, k_ff and k_fb; a, b and the model get no derivative.  The forward inputs are those of
 * sr_gp_moment_match_rollout (the same shapes, the same gains_per_traj reading of k_ff / k_fb, tz NULL = identity).  mu_all
 * T x H x n_s and sigma_all T x H x n_s x n_s are what a forward returned -- the fused call or H rounds of sr_gp_moment_match,
 * which agree to rounding --: step i is differentiated at the stored (mu_{i-1}, Sigma_{i-1}), step 0 at (mu0, sigma0) or in the
 * point branch when sigma0 is NULL.  Seeds mu_all_bar, sigma_all_bar, cov_all_bar shaped like the three forward outputs; any of
 * them may be NULL (= zero, the same bits as a zero array), not all three; only the symmetric parts of the two matrix seeds
 * count.  Outputs: mu0_bar T x n_s; sigma0_bar T x n_s x n_s, exactly symmetric (required iff sigma0 is given, else unread);
 * kff_bar T x H x n_u; kfb_bar T x (H - 1) x n_u x n_s (may be NULL when H == 1).  The two gain gradients are ALWAYS per
 * trajectory, also with gains_per_traj == 0: a shared policy's gradient is their sum over T.
 * Trajectories go in groups of max(1, min(chunk, what the launch grid takes) / H), chunk from sr_gp_set_chunk.  Per group the
 * records of sr_gp_moment_match_vjp, the GP's mean and V and the O(N^2) sums of its pair kernel are computed ONCE for all
 * (trajectory, step) pairs -- nothing of that reads the seeds --; then, for i = H-1 .. 0, four small launches carry the adjoint
 * through step i.  No atomics: the same bits on every call, for any chunk size and whatever other trajectories are in the
 * batch.  Scratch: grow-only, the handle's, freed by sr_gp_release_scratch.  Cost: about H calls of sr_gp_moment_match_vjp on T
 * queries in exp evaluations, in 5 + 4 H launches per group.  Asynchronous on `stream`.
 * Domain: that of sr_gp_moment_match_vjp (ARD-RBF handles, exact or sparse, any N, D <= 12), not that of the fused forward.
 * Errors, before any launch: SR_EINVAL NULL where required, sigma0 without sigma0_bar, all seeds NULL, T < 0, H < 1,
 * gains_per_traj outside {0, 1}, n_x_in outside 1 .. D - 1, tz NULL with n_x_in != n_s; SR_ESTATE not factorized;
 * SR_EUNSUPPORTED any general-family handle (the reverse pass is for ARD-RBF models only), D > 12, n_s > 12 (the sweep kernel
 * keeps its n_s x n_s matrices in LDS at that size), H beyond the launch grid.  T == 0 is a no-op. */
int sr_gp_moment_match_rollout_vjp(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj,
        const double* mu0, const double* sigma0, const double* k_ff, const double* k_fb,
        const double* a, const double* b, const double* tz, const double* inv_k,
        const double* mu_all, const double* sigma_all,
        const double* mu_all_bar, const double* sigma_all_bar, const double* cov_all_bar,
        double* mu0_bar, double* sigma0_bar, double* kff_bar, double* kfb_bar, void* stream);

/* replaces: utils.compute_remainder_overapproximations  utils.py:108-144 (batched)
 * q T x n_s x n_s, k_fb T x n_u x n_s -> u_mu T x n_s, u_sigma T x n_s */
int sr_remainder_overapprox(int device, long T, int n_s, int n_u, const double* q, const double* k_fb,
                            const double* l_mu, const double* l_sigma, double* u_mu, double* u_sigma,
                            void* stream);

/* replaces: gp_reachability.lin_ellipsoid_safety_distance  gp_reachability.py:215-250 (batched)
 * p T x n_s, q T x n_s x n_s, h_mat m x n_s, h_vec m -> d T x m */
int sr_safety_distance(int device, long T, int n_s, int m, const double* p, const double* q,
                       const double* h_mat, const double* h_vec, double c_safety, double* d,
                       void* stream);

/* replaces: utils_casadi.generic_cost with trig_aug as state transformation and loss_sat / loss_quadratic as stage and terminal
 * cost  utils_casadi.py:178-395 (batched; the objective of the reference's journal experiments)
 * sr_rollout_cost: the MPC objective over T stored moment trajectories of H states in ONE launch.  mu T x H x n_s, sigma
 * T x H x n_s x n_s (read as (sigma + sigma^T) / 2; NULL = zero, the same bits as a zero array), u T x H x n_u (row H - 1 unread):
 * the layouts of mu_all / sigma_all of sr_multistep_moments and sr_gp_moment_match_rollout, and of p_all / q_all of
 * sr_multistep_reach.  Per state: the augmentation trig_aug(m, v, idx_angle, a_trig, keep_radian) -- [m; a E sin; a E cos] with the
 * exact covariance, the angle's own row and column deleted unless keep_radian; idx_angle == -1: none -- to width n_c = n_s,
 * n_s + 1 or n_s + 2, then the loss against the target z (n_c) under W = F F^T (F n_c x n_c, row-major; W symmetric PSD, may be
 * singular; the caller factors it once):  loss 0, saturating: 1 - exp(-d^T W (I + S W)^-1 d / 2) / sqrt|I + S W|, d = m - z,
 * computed from the Cholesky factor of I + F^T S F (SPD for any PSD S: nothing inverts S, W or I + S W) and with expm1 / log1p, so
 * that a cost of 1e-9 at the target keeps its digits;  loss 1, quadratic: d^T W d + tr(W S).
 *   cost_steps[t][i] = w_stage loss_i + u_i^T R u_i  (i < H - 1) ;  w_term loss_{H-1}  (i = H - 1)       (T x H, may be NULL)
 *   cost[t] = the sum of cost_steps[t][:] in the order i = 0 .. H - 1                                     (T)
 * R n_u x n_u (need not be symmetric) or NULL: no control term; u NULL iff R NULL.  The same bits on every call, with and without
 * cost_steps, and whatever other trajectories are in the batch.  No model handle, no scratch.  Asynchronous on `stream`.
 * Errors, before any launch: SR_EINVAL NULL where required, T < 0, H < 1, n_s < 1, idx_angle outside -1 .. n_s - 1, loss outside
 * {0, 1}, R without u or u without R, keep_radian with idx_angle == -1; SR_EUNSUPPORTED n_s > 12 or n_u > 12; T == 0 is a no-op. */
int sr_rollout_cost(int device, long T, int H, int n_s, int n_u, int idx_angle /* -1: none */, double a_trig,
                    int keep_radian, int loss /* 0 sat, 1 quadratic */, const double* z, const double* F,
                    double w_stage, double w_term, const double* R /* n_u x n_u | NULL */,
                    const double* mu, const double* sigma /* | NULL */, const double* u /* | NULL iff R NULL */,
                    double* cost, double* cost_steps /* | NULL */, void* stream);
/* Its reverse pass in ONE launch: for the seed cost_bar (T; NULL = ones, the same bits as an array of ones) the gradient of
 * sum_t cost_bar[t] cost[t] in the inputs:  mu_bar T x H x n_s ; sigma_bar T x H x n_s x n_s, exactly symmetric, also when sigma
 * is NULL (the gradient of the function extended to unsymmetric arguments by sigma -> (sigma + sigma^T) / 2) ; u_bar T x H x n_u
 * (row H - 1 exactly zero; all zero without R).  Each of the three may be NULL, not all three.  They are shaped like, and are, the
 * seeds mu_all_bar / sigma_all_bar of sr_multistep_moments_vjp and sr_gp_moment_match_rollout_vjp and p_all_bar / q_all_bar of
 * sr_multistep_reach_vjp: the gradient of the objective in k_ff, k_fb is a roll-out, this call and the roll-out's reverse pass.
 * Closed form, no differences: with A = F B^-1 F^T, B = I + F^T S F, g = A d, q = 1 - loss the saturating loss has
 * d loss / d m = q g and d loss / d S = q (A - g g^T) / 2; the quadratic 2 W d and W; then back through the augmentation.
 * Inputs, determinism and refusals as sr_rollout_cost; SR_EINVAL also when every output is NULL.  Asynchronous on `stream`. */
int sr_rollout_cost_vjp(int device, long T, int H, int n_s, int n_u, int idx_angle, double a_trig, int keep_radian, int loss,
                        const double* z, const double* F, double w_stage, double w_term, const double* R,
                        const double* mu, const double* sigma, const double* u, const double* cost_bar,
                        double* mu_bar, double* sigma_bar, double* u_bar, void* stream);

/* replaces: SimpleSafeMPC.generate_safety_constraints / _generate_control_constraint  safempc_simple.py:317-392, 488-532 (batched;
 * the constraint vector of the SafeMPC problem, every row a lin_ellipsoid_safety_distance)
 * sr_rollout_constraints: the constraint rows of T stored roll-outs of H ellipsoids in ONE launch.  p_all T x H x n_s, q_all
 * T x H x n_s x n_s are what sr_multistep_reach returned, k_ff T x H x n_u, k_fb T x (H - 1) x n_u x n_s (may be NULL when H == 1
 * or without bounds) what it was given, q0 T x n_s x n_s with k_fb0 T x n_u x n_s its ellipsoid start (both NULL: point start).
 * q_all and q0 are read as their symmetric parts (q + q^T) / 2.  Every row is satisfied iff g <= 0; per trajectory
 * n_g = (bounds ? 2 n_u H : 0) + m_obs (H - 1) + m_safe rows in this order:
 *   control    (u_min, u_max given, n_u each; both NULL: no such rows) for the steps i = 0 .. H - 1, 2 n_u rows each:
 *              [k_ff[i] + r_i - u_max ; u_min - k_ff[i] + r_i],  r_i[j] = c_safety sqrt(K_i[j, :] Q_i K_i[j, :]^T) with
 *              (Q_0, K_0) = (q0, k_fb0) -- a point start has r_0 = 0: the two-sided bound on u_0 -- and (Q_i, K_i) =
 *              (q_all[i - 1], k_fb[i - 1]) for i >= 1, the indices of sr_multistep_reach (step i applies k_fb[i - 1] at
 *              p_all[i - 1]); the reference's h_mat = [I; -I], h_vec = [u_max; -u_min] on the ellipsoid (k_ff, K Q K^T)
 *   obstacle   (h_obs_mat m_obs x n_s, h_obs m_obs; m_obs == 0: both NULL) for the states i = 0 .. H - 2, m_obs rows each:
 *              h . p_all[i] + c_safety sqrt(h q_all[i] h^T) - h_obs
 *   terminal   (h_safe_mat m_safe x n_s, h_safe m_safe; m_safe == 0: both NULL) m_safe rows of that form on the last state
 * c_safety scales every square root, the control rows' included (the control set is the image of the same ellipsoid; the
 * reference passes its default 1 everywhere).  The obstacle and terminal rows are the bits of sr_safety_distance on the same
 * ellipsoids at a symmetric q.  A negative radicand gives NaN in its row, as there.  g T x n_g; g_max (T, may be NULL) the
 * largest row of each trajectory, NaN if any of its rows is NaN: g_max[t] <= 0 iff candidate t is feasible.  The rows work on
 * mu_all / sigma_all of the moment roll-outs as they are (the chance constraints of CautiousMPC).  The same bits on every call, with
 * and without g_max, and whatever other trajectories are in the batch.  No model handle, no scratch.  Asynchronous on `stream`.
 * Errors, before any launch: SR_EINVAL NULL where required (p_all, q_all, g; k_ff with bounds; k_fb with bounds and H > 1), q0
 * without k_fb0 or the reverse, u_min without u_max or the reverse, m_obs < 0 or m_safe < 0, m > 0 with a NULL matrix or vector,
 * n_g == 0, T < 0, H < 1, n_s < 1, n_u < 1 with bounds; SR_EUNSUPPORTED n_s > 12 or n_u > 12; T == 0 is a no-op. */
int sr_rollout_constraints(int device, long T, int H, int n_s, int n_u,
                           const double* p_all, const double* q_all, const double* k_ff, const double* k_fb,
                           const double* q0, const double* k_fb0 /* both NULL: point start */,
                           const double* u_min, const double* u_max /* both NULL: no control rows */,
                           int m_obs, const double* h_obs_mat, const double* h_obs,
                           int m_safe, const double* h_safe_mat, const double* h_safe,
                           double c_safety, double* g /* T x n_g */, double* g_max /* T | NULL */, void* stream);
/* Its reverse pass in ONE launch: for the seed g_bar (T x n_g) the gradient of sum(g_bar * g) in the inputs:  p_all_bar
 * T x H x n_s ; q_all_bar T x H x n_s x n_s, exactly symmetric ; kff_bar T x H x n_u ; kfb_bar T x (H - 1) x n_u x n_s ; with
 * q0 also q0_bar T x n_s x n_s, exactly symmetric, and kfb0_bar T x n_u x n_s (both required iff q0 is given, else unread).
 * Overwritten, not accumulated (zero where no row reads the input); each of the four main outputs may be NULL, not all four.
 * p_all_bar / q_all_bar are shaped like, and are, the seeds of sr_multistep_reach_vjp: the gradient of a Lagrangian or penalty of
 * the SafeMPC problem in k_ff, k_fb is a roll-out, this call and the roll-out's reverse pass, plus kff_bar / kfb_bar of this call
 * (the rows read the gains directly as well).
 * Closed form, with s = sqrt(h Q_s h^T), Q_s the symmetric part:  state rows  d / d p = g_bar h,  d / d Q = c g_bar h^T h / (2 s);
 * control output j with g+ = g_bar_upper + g_bar_lower, k = K[j, :]:  d / d k_ff[j] = g_bar_upper - g_bar_lower,
 * d / d k = c g+ Q_s k^T / s_j,  d / d Q = c g+ k^T k / (2 s_j).
 * A radicand that is exactly zero -- a k_fb row of zeros, the usual initial guess, or q = 0 -- contributes ZERO through its
 * square root: in k this is an element of the subdifferential of the norm k -> sqrt(k Q k^T) at its kink, in Q it truncates an
 * infinite one-sided slope.  This deliberately differs from var_bar = +-inf of sr_ellipsoid_step_vjp: a zero gain must not poison
 * a whole gradient with 0 * inf.  A negative radicand gives NaN in exactly the outputs of its (trajectory, state) that the row
 * touches (q_all_bar[t, i], kfb_bar[t, i]; p_all_bar stays finite) and nothing else.
 * One writer per output element, no atomics, sums in a fixed order: the same bits on every call and whatever other trajectories
 * are in the batch.  Inputs and refusals as sr_rollout_constraints; SR_EINVAL also for g_bar NULL, every main output NULL, q0
 * without q0_bar or kfb0_bar.  Asynchronous on `stream`. */
int sr_rollout_constraints_vjp(int device, long T, int H, int n_s, int n_u,
                               const double* p_all, const double* q_all, const double* k_ff, const double* k_fb,
                               const double* q0, const double* k_fb0, const double* u_min, const double* u_max,
                               int m_obs, const double* h_obs_mat, const double* h_obs,
                               int m_safe, const double* h_safe_mat, const double* h_safe,
                               double c_safety, const double* g_bar /* T x n_g */,
                               double* p_all_bar, double* q_all_bar, double* kff_bar, double* kfb_bar,
                               double* q0_bar, double* kfb0_bar /* required iff q0 is given */, void* stream);

/* ---- the exploration objective over the stored GP variances of roll-outs ------------------------------------------------------
 * replaces: the default cost of SimpleSafeMPC.generate_cost_function  safempc_simple.py:286-315  (kind 1; with the deviation term
 *           its n_perf > 1 branch) and of StaticSafeMPCExploration.init_solver  safempc_exploration.py:104  (kind 0)
 * sr_rollout_explore: the objective of T roll-outs in ONE launch; no model handle, no scratch.  gp_var T x H_v x n_s are GP variances
 * of a roll-out (gp_var_all of sr_multistep_reach_var or of sr_multistep_moments).  Per trajectory t, with v = gp_var[t]:
 *   kind 0   info_i = -r_i,        r_i = (v[i][0] + v[i][1]) + ... + v[i][n_s-1]
 *   kind 1   info_i = -sqrt(r_i),  r_i = ((v[i][0] + v[i][1]) + ... + v[i][n_s-1]) + eps
 *            (the reference adds eps_noise to every element: eps = n_s eps_noise)
 *   n_dev >= 2:  dev_i = d^T W d for 1 <= i < n_dev, d = mu[t][i] - p[t][i]; row 0 is skipped as in the reference.  p T x H_p x n_s
 *            is the safe trajectory, mu T x H_m x n_s the performance trajectory, W n_s x n_s need not be symmetric (the caller
 *            passes 0.1 wx_cost).  s_a = fma(W[a][n_s-1], d_{n_s-1}, ... fma(W[a][0], d_0, 0)), dev_i = fma(d_{n_s-1}, s_{n_s-1}, ...
 *            fma(d_0, s_0, 0)).
 *   cost[t] = ((info_0 + info_1) + ... + info_{H_v-1}) + ((dev_1 + dev_2) + ... + dev_{n_dev-1})   (the second bracket only with n_dev >= 2)
 * cost_steps T x H_v (or NULL) receives the information terms info_i.  Every sum runs in the order written here, one writer per
 * output element, no atomics: the same bits on every call and whatever else is in the batch, with and without cost_steps.
 * r_i < 0 (kind 1) gives NaN in cost[t] and cost_steps[t][i] only.
 * Before any launch: SR_EINVAL for NULL where required (gp_var, cost), kind outside {0, 1}, T < 0, H_v < 1, n_s < 1, n_dev < 0 or
 * n_dev == 1, n_dev > min(H_p, H_m), n_dev >= 2 without p, mu or W, eps < 0; SR_EUNSUPPORTED for n_s > 12; T == 0 is a no-op.
 * p and mu may be NULL with n_dev == 0 (H_p, H_m are then ignored).  Asynchronous on `stream`. */
int sr_rollout_explore(int device, long T, int kind /* 0 sum, 1 sqrt */, int n_s, int H_v, const double* gp_var /* T x H_v x n_s */,
                       double eps, int n_dev /* 0: no deviation term */, int H_p, const double* p /* T x H_p x n_s | NULL */,
                       int H_m, const double* mu /* T x H_m x n_s | NULL */, const double* W /* n_s x n_s | NULL */,
                       double* cost /* T */, double* cost_steps /* T x H_v | NULL */, void* stream);
/* Its reverse pass in ONE launch, in closed form: for the seed cost_bar (T; NULL = ones, the same bits) the gradient of
 * sum(cost_bar * cost):  gpvar_bar[t][i][:] = -cost_bar[t] (kind 0) or -cost_bar[t] / (2 sqrt(r_i)) (kind 1);
 * mu_bar[t][i][a] = cost_bar[t] fma-sum_{b = 0 ..} (W[a][b] + W[b][a]) d_b and p_bar[t][i] = -mu_bar[t][i] for 1 <= i < n_dev; every
 * other row of p_bar (T x H_p x n_s) and mu_bar (T x H_m x n_s) is exactly zero.  Overwritten, not accumulated.  gpvar_bar is shaped
 * like, and is, the seed gpvar_all_bar of sr_multistep_reach_var_vjp (or of sr_multistep_moments_vjp); p_bar is added to the seed on
 * p_all, mu_bar is the seed on the means of the performance roll-out: the gradient of the exploration problem is a roll-out, this
 * call and the roll-out's reverse pass.
 * r_i == 0 contributes exactly ZERO (the convention of sr_rollout_constraints_vjp for a zero radicand: the infinite one-sided
 * slope is truncated, not +-inf); r_i < 0 gives NaN in gpvar_bar[t][i][:] only.
 * Each output may be NULL, not all three; p_bar needs p and mu_bar needs mu (SR_EINVAL).  Inputs, determinism and the other refusals
 * as sr_rollout_explore.  Asynchronous on `stream`. */
int sr_rollout_explore_vjp(int device, long T, int kind, int n_s, int H_v, const double* gp_var, double eps, int n_dev, int H_p,
                           const double* p, int H_m, const double* mu, const double* W, const double* cost_bar /* T | NULL = ones */,
                           double* gpvar_bar /* T x H_v x n_s */, double* p_bar /* T x H_p x n_s */, double* mu_bar /* T x H_m x n_s */,
                           void* stream);

/* replaces: utils_ellipsoid.distance_to_center / sample_inside_ellipsoid  utils_ellipsoid.py:16-60 (batched;
 * the Monte-Carlo verification of sampling_models.py / gp_reachability.py:323-356 evaluates it per step)
 * T ellipsoids (p T x n_s, q T x n_s x n_s) against K samples: samples K x n_s shared by all ellipsoids
 * (per_t = 0) or T x K x n_s (per_t = 1) -> d T x K with d = (s-p)^T Q^-1 (s-p). */
int sr_distance_to_center(int device, long T, int K, int n_s, const double* samples, int per_t,
                          const double* p, const double* q, double* d, void* stream);

/* replaces: the objective that GPy's model.optimize() minimises inside SimpleGPModel.train(opt_hyp=True)
 * ssm_gpy/gaussian_process.py:249-250 (the optimiser itself stays on the host: L-BFGS-B over these values).
 * For the factorised model (data set with sr_gp_set_data_general):
 *   nll[d]  = 1/2 y^T alpha + 1/2 log det K_y + N/2 log 2pi
 *   grad[d] = d nll / d [v, c0, s[D], a[D], b[D], noise]   (SR_KP(D) = 3+3D entries per output, the packed
 *             kernel parameters in their order, then the diagonal noise term). */
int sr_gp_mll(sr_gp_t h, double* nll /* n_out, device */, double* grad /* n_out x (3+3D), device */,
              void* stream);

/* replaces: the determinant inside SimpleGPModel.information_gain  ssm_gpy/gaussian_process.py:621-634
 * (log det(I + K/sigma_n^2) = log det(K + sigma_n^2 I) - N log sigma_n^2).
 * logdet[d] = log det(K_d + noise_d I) of the factorised (or imported) model, from the diagonal of U^-1. */
int sr_gp_logdet(sr_gp_t h, double* logdet /* n_out, device */, void* stream);
/* The same numbers from the HOST copy that sr_gp_append (<= 16 rows) reads back together with its status words -- no
 * launch, no synchronisation: the reference's exploration loop asks for the information gain after every appended
 * transition (exploration_runner.py:186-189).  SR_ESTATE when the last model update left no copy (a factorisation, an
 * imported model, an append of more than 16 rows): call sr_gp_logdet then. */
int sr_gp_logdet_cached(sr_gp_t h, double* logdet_host /* n_out, host */);

/* replaces: SimpleGPModel.sample_from_gp  ssm_gpy/gaussian_process.py:598-619 (marginal posterior samples,
 * GPy posterior_samples_f(full_cov=False)) and the propagation step of
 * MonteCarloSafetyVerification.sample_n_step  sampling_models.py:66-80.
 * mu, var T x n_out (from sr_gp_predict), eps T x size x n_out standard-normal draws supplied by the
 * caller -> S T x size x n_out = mu + sqrt(var) * eps.  If z_next != NULL it also receives the next GP
 * inputs T x size x (n_out + n_u): [S, k_fb S + k_ff] with k_fb n_u x n_out, k_ff n_u. */
int sr_gp_sample(int device, long T, int size, int n_out, int n_u, const double* mu, const double* var,
                 const double* eps, double* S, const double* k_fb, const double* k_ff, double* z_next,
                 void* stream);

/* ---- posterior FUNCTION samples: pathwise conditioning (Matheron's rule on a random-Fourier-feature prior) ----------
 * S whole posterior functions of an ARD-RBF model (or of a general-family model with the RBF radial part: further down)
 * that can be evaluated anywhere, consistently, in O(N + M) per value:
 * per output d and path s, with l_d, sf2_d the kernel's parameters and n_d the diagonal term as sr_gp_set_data received it,
 *   phi_d(x)_i = sqrt(2 sf2_d / M) cos(sum_j omega[i][j] x_j / l_d[j] + tau[i])                         i < M
 *   c_{d,s}    = K_y,d^-1 (y_d - Phi_d(Z) w_{d,s} - sqrt(n_d) eps_{d,s}) = U^-1 (U^-T r_{d,s})            (N)
 *   f_{d,s}(x) = phi_d(x) . w_{d,s} + k_d(x, Z) c_{d,s}
 * The reference has no counterpart: it draws marginal samples only (sample_from_gp  ssm_gpy/gaussian_process.py:598-619,
 * used by sampling_models.py:66-80), so a particle of its Monte-Carlo rollout meets an unrelated function at every step.
 * The caller supplies all randomness (device memory), as sr_gp_sample takes eps; the device code is deterministic and the
 * same inputs give the same bits: omega M x D standard normal, tau M uniform in [0, 2 pi) (both shared by all outputs and
 * paths), w n_out x S x M and eps n_out x S x N standard normal.  With w = 0, eps = 0 every path is the posterior mean.
 *
 * sr_gp_paths_draw builds w and c in the k-major layout of the MFMA tile (n_out x Mp x Sp and n_out x Np x Sp, Mp = M to 16,
 * Sp = S to 128; padding exactly zero) and keeps them, omega and tau with the handle (a grow-only block; SR_EHIP if it cannot
 * be had).  S == 0 drops the paths (the pointers may be NULL).  Asynchronous on `stream`.
 * sr_gp_paths_count: S and M of the valid paths, 0, 0 when the handle holds none.
 * sr_gp_paths_eval: every path at every query, Xq T x D -> F T x S x n_out (the layout of sr_gp_sample's output), in chunks
 * of sr_gp_set_chunk queries.  T == 0 is a no-op.  Asynchronous on `stream`.
 * sr_gp_paths_step: path s at its OWN input Xs[s] (S x D) -> F S x n_out; with k_fb (n_u x n_out) and k_ff (n_u) non-NULL
 * z_next (S x D) receives the closed-loop next inputs [F[s], k_fb F[s] + k_ff] as sr_gp_sample's z_next does; that form needs
 * D = n_out + n_u with n_u >= 1, otherwise SR_EINVAL.  Asynchronous on `stream`.
 * The paths belong to the model they were drawn from: everything that rewrites the model (sr_gp_set_data*, sr_gp_factorize,
 * sr_gp_fit_sparse, sr_gp_append, sr_gp_append1_host, sr_gp_remove, sr_gp_import*) invalidates them -- _eval and _step then
 * return SR_ESTATE and _count gives 0, 0 until the next _draw.  sr_gp_release_scratch frees the workspaces of the three
 * calls, not the paths.
 * All errors are found on the host before any launch, and invalid arguments leave paths drawn earlier intact: SR_EINVAL NULL
 * where not allowed, S < 0, M < 1 or M > 1048560 with S > 0, T < 0; SR_ESTATE not factorized, a sparse handle (Wt is not the factor of K_y),
 * between sr_gp_import_begin and sr_gp_import_end, no valid paths; SR_EUNSUPPORTED a general-family model with a Matern
 * output (the feature map is the Gaussian spectral density: mat52 / lin_mat52 are out of scope; nothing is read from the
 * caller's arrays) or D > 8, as the other batched entry points.
 * sr_gp_paths_eval_grad / _step_grad: the same calls with the Jacobian of every value in the input,
 *   d f_{d,s}(x) / d x_j = -sqrt(2 sf2_d / M) / l_d[j] sum_i sin(omega_i . x / l_d + tau_i) omega[i][j] w_{d,s,i}
 *                          + sf2_d / l_d[j]^2 sum_i exp(-r_i^2 / 2) (z_ij - x_j) c_{d,s,i}
 * over the w and c the draw keeps (nothing is drawn or solved): J T x S x n_out x D resp. S x n_out x D.  F is bit for bit F
 * of _eval / _step on the same inputs (_eval_grad: F may be NULL); k_fb, k_ff, z_next, the chunks, T == 0, the errors (J NULL:
 * SR_EINVAL), the states and the invalidation are theirs.  Deterministic, no atomics.  Workspace (grow-only, freed by
 * sr_gp_release_scratch): _eval_grad one more feature slab and one K*-sized slab per chunk, n_out (2 Mp + Np) Tp doubles in
 * all; _step_grad 1 + D times the partial sums of _step.
 * The general family (sr_gp_set_data_general) with the RBF radial part on every output, k = (c0 + sum_j a_j x_j y_j) v kappa(r)
 * + sum_j b_j x_j y_j, r^2 = sum_j (s_j (x_j - y_j))^2: a sum of products of PSD kernels, so a prior sample is a sum over
 * products of their features.  With base_i(x) = sqrt(2 v / M) cos(sum_j omega[i][j] s_j x_j + tau[i]) (omega, tau as above),
 * A_0(x) = sqrt(c0), A_l(x) = sqrt(a_l) x_l (l = 1 .. D) and the G active groups -- the l, ascending, whose c0 resp. a_l is
 * non-zero on at least one output of the handle --
 *   f_prior(x) = sum_{g < G} A_{l_g}(x) sum_{i < M} w[g M + i] base_i(x) + sum_j sqrt(b_j) x_j w[G M + j]
 * takes n_w = G M + D weights per path and output: w is n_out x S x n_w (sr_gp_paths_weight_count; M for an ARD-RBF handle),
 * c and f(x) = phi(x) . w + k(x, Z) c are as above and sr_gp_paths_count keeps returning the base M.  The Jacobian: the
 * features' d/dx_j [A_l base_i] = [l == j + 1] sqrt(a_j) base_i - A_l sqrt(2 v / M) sin(..) omega[i][j] s_j and sqrt(b_j)
 * w[G M + j], plus sum_i c_i dk(x, z_i)/dx_j with dk/dx_j = a_j z_j v kappa - (c0 + sum a x z) v kappa s_j^2 (x_j - z_j)
 * + b_j z_j.  Layouts, chunks, invalidation, errors, determinism and F of the _grad forms are those above; v, c0, a_j and b_j
 * sit under square roots: a negative one is SR_EINVAL at the draw (named in the error text; paths drawn earlier stay).
 * sr_gp_paths_weight_count: n_w for M features, with the refusals of sr_gp_paths_draw in its order (M, the model, the signs).
 * Out of scope: Hessians of the paths, replication of paths to other ranks, Matern radial parts (their spectral draw is a
 * Student-t, a rule for the caller's omega), the roll-out in one launch for the general family (below). */
int sr_gp_paths_draw(sr_gp_t h, int S, int M, const double* omega, const double* tau, const double* w, const double* eps,
                     void* stream);
int sr_gp_paths_count(sr_gp_t h, int* S, int* M);
int sr_gp_paths_weight_count(sr_gp_t h, int M, int* n_w);
int sr_gp_paths_eval(sr_gp_t h, const double* Xq, long T, double* F, void* stream);
int sr_gp_paths_step(sr_gp_t h, const double* Xs, double* F, const double* k_fb, const double* k_ff, double* z_next,
                     void* stream);
int sr_gp_paths_eval_grad(sr_gp_t h, const double* Xq, long T, double* F, double* J, void* stream);
int sr_gp_paths_step_grad(sr_gp_t h, const double* Xs, double* F, double* J, const double* k_fb, const double* k_ff,
                          double* z_next, void* stream);
/* sr_gp_paths_rollout: every valid path through H closed-loop steps in ONE launch (what H chained _step / _step_grad calls
 * compute, not bit for bit: the terms are summed in another order).  n_s = n_out, n_u = D - n_out >= 1.  x0: n_s doubles
 * (x0_per_path == 0: one start for all paths) or S x n_s (x0_per_path == 1); k_fb H x n_u x n_s, k_ff H x n_u.  Step i
 * evaluates path s at [x_i[s], k_fb[i] x_i[s] + k_ff[i]] and x_{i+1}[s] is the result: X_all H x S x n_s holds x_1 .. x_H;
 * A_all, NULL or H x S x n_s x n_s, A_all[i][s] = J_x + J_u k_fb[i] with J = d f_s / d(input) at step i's input.  X_all is
 * the same bits with and without A_all, on every call, and its first h steps are the h-step call.  Device pointers, no
 * workspace, asynchronous on `stream`.  Errors in the order of _step, before any launch: SR_EINVAL NULL h, x0, k_fb, k_ff or
 * X_all, H < 1, x0_per_path not 0 / 1, D == n_out; then the model's SR_ESTATE / SR_EUNSUPPORTED; SR_ESTATE no valid paths. */
int sr_gp_paths_rollout(sr_gp_t h, const double* x0, int x0_per_path, int H, const double* k_fb, const double* k_ff,
                        double* X_all, double* A_all, void* stream);
/* sr_gp_paths_rollout_vjp: the reverse pass of sr_gp_paths_rollout in the gains and the start.  x0, x0_per_path, H, k_fb, k_ff
 * as the forward took them, X_all (H x S x n_s) the states it returned (X_all[H-1] is not read), X_bar (H x S x n_s) the seeds:
 * with L = sum_{i,s} X_bar[i][s] . x_{i+1}[s], z_i[s] = [x_i[s], k_fb[i] x_i[s] + k_ff[i]] and J_i[s] = d f_s / d z at z_i[s]
 * (n_s x D = [J_x | J_u], the closed form of sr_gp_paths_step_grad over the w and c the draw keeps: nothing is drawn or solved),
 * per path, lambda = X_bar[H-1][s], for i = H-1 .. 0:
 *   g = J_i[s]^T lambda = [g_x, g_u];  k_ff_bar[i] += g_u;  k_fb_bar[i] += g_u x_i[s]^T;
 *   lambda = (i >= 1 ? X_bar[i-1][s] : 0) + g_x + k_fb[i]^T g_u;                      x0_bar[s] = lambda at the end.
 * k_fb_bar H x n_u x n_s and k_ff_bar H x n_u are summed over the paths; x0_bar is S x n_s with x0_per_path == 1 and n_s doubles,
 * the sum over the paths, with x0_per_path == 0.  J_all, NULL or H x S x n_s x D, receives every J_i[s] (the J_u that A_all
 * folds away); the three gradients are the same bits with and without it.  Gradients in the model or the draws: out of scope.
 * Device pointers, asynchronous on `stream`, deterministic: no floating-point atomics, every sum in a fixed order (the splits
 * of the N + M terms ascending, the paths in a fixed tree per block of 256 and the blocks ascending), the same bits on every
 * call.  Workspace: the handle's grow-only block of the path calls (freed by sr_gp_release_scratch) -- J when J_all is NULL,
 * the splits' partial sums (the split rule of _step for H S evaluations; n_s D H Sp doubles each), one record per block; SR_EHIP
 * if it cannot be had.  Errors in the forward's order, before any launch, the paths and the other calls' results untouched:
 * SR_EINVAL NULL h, x0, k_fb, k_ff, X_all, X_bar, x0_bar, k_fb_bar or k_ff_bar, H < 1, x0_per_path not 0 / 1, D == n_out; then
 * the model's SR_ESTATE / SR_EUNSUPPORTED; SR_ESTATE no valid paths. */
int sr_gp_paths_rollout_vjp(sr_gp_t h, const double* x0, int x0_per_path, int H, const double* k_fb, const double* k_ff,
                            const double* X_all, const double* X_bar, double* x0_bar, double* k_fb_bar, double* k_ff_bar,
                            double* J_all, void* stream);

/* ---- tuning / measurement -------------------------------------------------------------------- */
/* max queries processed per internal pass (workspace = n_out * Np * chunk * 8 B); default 65536. */
int sr_gp_set_chunk(sr_gp_t h, long chunk);
/* query tiles per scheduling group of the variance kernel (L2/XCD locality knob); default 64. */
int sr_gp_set_var_group(sr_gp_t h, int group);
/* main loop of the variance kernel: 1 = the loop of rounds 1 - 4 (LDS-DMA tiles, workgroup barrier on top of every
 * k-tile), 3 = the pipelined loop of round 5 (barrier under the MFMA stream; same results as 1 bit for bit), 4 = 3 with
 * the structural zeros of the diagonal blocks of U^-1 left out (same numbers summed in another order: equal to 1e-13),
 * 5 = 4 with the row blocks (nrb - 1 - p, p) of a query tile in ONE workgroup (equal work per workgroup; bit for bit 4).
 * A measurement knob; other values are SR_EINVAL. */
int sr_gp_set_var_variant(sr_gp_t h, int variant);
/* blocks of 128 rows per Cholesky panel of sr_gp_factorize (the trailing matrix is read-modify-written once per
 * panel); 0 = chosen by size (default).  Results agree to rounding; a measurement knob. */
int sr_gp_set_fact_panel(sr_gp_t h, int panel);
/* How sr_gp_factorize runs between 3 and 128 blocks of 128 rows.  0 (default) = one chain of launches.  1 / 2 = the pipelined
 * prototypes of round 6 (diagonal blocks on a stream of their own / only the rest of the rows moved; identical numbers,
 * 1.2 - 2.8 times slower: profiles/r06_fact_pipeline.txt).  3 = the tile-flow Cholesky (csrc/sr_flow.hip: ONE resident
 * kernel of tile tasks plus a resident diagonal-block workgroup per output, device counters for dependencies; results to
 * rounding, time within 2 % of the launched form from N = 6000 on, behind below: profiles/r06_flow.txt).  -1 = never the tile flow.
 * sr_gp_fact_pipelined: how the last update of h ran -- 0 chain of launches, 1 pipelined prototype, 4 tile flow. */
int sr_gp_set_fact_pipeline(sr_gp_t h, int on);
int sr_gp_fact_pipelined(sr_gp_t h);
/* diagnostics of the last tile-flow update (SR_ESTATE if it was none): out[0..23] = per kind of task (look-ahead update,
 * bulk update, diagonal tiles, near updates, near solves, far blocks) [count, ticks inside, ticks of those waiting, 0] at
 * 100 MHz; then per output the ticks from the start to each diagonal block.  Returns the words written (cap too small:
 * SR_EINVAL). */
int sr_gp_flow_stats(sr_gp_t h, unsigned* out, int cap);
/* latency paths instead of the plain MFMA tiles: one-launch pass for small models (Np <= 512, T <= 1024),
 * HBM-bound streaming of U^-1 for batches of <= 64 queries, 64 x 64 tiles, balanced shares of the k-blocks under few
 * query tiles.  on = 1 (default) all of them, 2 all but the one-launch pass, 0 none; an A/B measurement knob.  Results
 * agree to rounding. */
int sr_gp_set_small_path(sr_gp_t h, int on);
/* multi-step chains (sr_multistep_reach / sr_multistep_moments) of small ARD-RBF models (Np <= 512, <= 4096 rollouts,
 * the reference's systems n_s <= 4) run all H steps inside ONE persistent launch; on = 0 forces the per-step launches.
 * Default on; results agree to rounding.  sr_gp_last_chain: 1 if the last chain took the persistent kernel. */
int sr_gp_set_chain(sr_gp_t h, int on);
/* The workgroups of the persistent kernel wait for each other; they are launched only when the kernel's occupancy
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) and the device's CU count say they can all be resident.  Should the
 * hand-off of a group still not complete within 100 ms (the CUs were held by other work for that long), the group fills
 * its outputs with NaN AND raises a status word in pinned host memory.  sr_gp_chain_status: call after synchronising the
 * stream; *timed_out = 1 if a launch since the last query failed that way (the word is cleared, and the handle takes the
 * per-step launches from then on).  A caller that does not ask is told by the next reachability entry point, which
 * returns SR_ESTATE once. */
int sr_gp_chain_status(sr_gp_t h, int* timed_out);
/* The model update keeps its scratch (two Np x Np matrices per output in flight) with the handle while that is at most a
 * third of the device's memory, so that refits allocate nothing (40 GB at N = 50000); the row append keeps a strip and
 * the previous U^-1 buffer.  A host that will only evaluate the model from here on hands them back with this call. */
int sr_gp_release_scratch(sr_gp_t h);
/* Device buffers of >= 1 MB that a handle releases (a model that grew, a handle that was destroyed) stay with the library
 * for the next request of their size class -- the first touch of a fresh allocation, not hipMalloc, is what a refit after
 * a change of N used to pay for (48 against 6 ms at N = 5000); at most an eighth of the device's memory is held, an
 * allocation that fails returns them all before it is reported.  This call hands
 * everything cached back to the driver (all devices). */
int sr_release_cached_memory(void);

/* ---- completion mailbox for a host that blocks on ONE small result --------------------------------
 * (the CasADi / IPOPT callback: CasadiSSMEvaluator.eval, state_space_models.py:271-303, calls the model, waits, and
 * hands NumPy arrays back).  sr_publish enqueues, behind the work already on `stream`, a copy of n doubles from device
 * memory into PINNED host memory followed by a store of `seq` to *flag_host (pinned as well); sr_wait_flag spins on the
 * host until *flag_host == seq (SR_ESTATE after timeout_s).  The result is visible a PCIe write after the producing
 * kernel ends; a D2H copy + hipStreamSynchronize takes ~4 us longer (N = 200: 33.7 -> 29.4 us per blocking call). */
int sr_publish(int device, const double* src_dev, int n, double* dst_host, unsigned long long* flag_host,
               unsigned long long seq, void* stream);
int sr_wait_flag(const unsigned long long* flag_host, unsigned long long seq, double timeout_s);
/* 1 where kernels of `device` may be handed the HOST address of this pinned block as it is (device-visible at the same
 * address, and the device's atomic adds -- the n_bad counters -- reach pinned host memory: probed once per device and
 * process with one tiny launch on a word of the library's own), 0 otherwise: asked once by a host layer that lets the kernels read / write its pinned staging
 * blocks directly (tiny batches: no copy command in either direction; safe_exploration_amd/_buffers.py). */
int sr_host_block_is_device_visible(int device, const void* host_block);
/* hipStreamSynchronize(stream) with `device` current, for a host layer that holds the raw stream handle (the handle 0 --
 * the null stream, PyTorch's default -- names the stream of whichever device is current: hence the device). */
int sr_stream_synchronize(int device, void* stream);
/* One blocking single query as ONE command.  replaces SimpleGPModel.__call__ (ssm_gpy/gaussian_process.py:135-144) and
 * linearize_predict(jacobians=True) as CasadiSSMEvaluator drives them (state_space_models.py:271-303, 384-417).
 * x_host (D doubles, read at call time) travels in the kernel arguments; the results go to the pinned block
 *   out_host = [mu n | var n | jac_mu n x D]   (+ [jac_var n x D | hess_mu n x D x D] with second_order != 0)
 * and the last workgroup stores seq to *flag_host (pinned; wait with sr_wait_flag).
 * From 512 padded rows on the streamed kernels read the query from x_host: it must then be pinned, device-visible too.
 * SR_EUNSUPPORTED with an input transform, with the size dispatch switched off, or where a block is not device-visible:
 * use sr_gp_predict / sr_gp_linearize. */
int sr_gp_call1(sr_gp_t h, const double* x_host, int second_order, double* out_host,
                unsigned long long* flag_host, unsigned long long seq, void* stream);
/* Resident single-query server (the MPC loop's latency path).  replaces the blocking model evaluation inside
 * CasadiSSMEvaluator.eval / JacFun.eval / BackFun.eval (state_space_models.py:278-303, 384-417, 534-562).
 * _start launches workgroups that STAY on the device and poll a mailbox line in pinned host memory; _call posts x_host
 * (D doubles, any host memory; GP input space), waits and copies the answer to out_host (layout of sr_gp_call1).
 * Every kernel identifier, Np <= 512, D <= 5; SR_EUNSUPPORTED otherwise and from _call when no server is armed.
 * The kernel leaves after idle_timeout_s without a request and _call launches it again; model updates take it off the
 * device first (it stays armed).  No answer within timeout_s: SR_ESTATE, the next call starts a fresh launch.
 * Threads, device-wide synchronisation, mailbox protocol: INTEGRATION.md 2.3 and csrc/sr_capi_server.hip. */
int sr_gp_server_start(sr_gp_t h, double idle_timeout_s);
int sr_gp_server_stop(sr_gp_t h);
int sr_gp_server_call(sr_gp_t h, const double* x_host, int second_order, double* out_host, double timeout_s);
int sr_gp_server_state(sr_gp_t h, int* armed, int* resident, long* launches, long* calls);
int sr_gp_last_chain(sr_gp_t h);
/* diagnostic: C(M x N) = alpha * A^T B + beta * C with A (K x M), B (K x N) k-major; M, N multiples
 * of 128, K multiple of 16; mode 0 all tiles, 1 upper block triangle, 2 B block-lower-triangular.
 * Exposed so the fp64-MFMA tile can be tested in isolation. */
int sr_test_gemm_tn(int device, const double* A, long lda, const double* B, long ldb, double* C,
                    long ldc, int M, int N, int K, double alpha, double beta, int mode, void* stream);
/* diagnostic: the trailing-update product of the factorisation alone: C (M x N, only the 128-tiles n0 >= m0) =
 * alpha A^T B + beta C, A (K x M), B (K x N) k-major, M <= N multiples of 128; order 0 row-major tiles, 1 XCD-aware
 * super-tiles, -1 chosen by size. */
int sr_test_gemm_tn_upper(int device, const double* A, long lda, const double* B, long ldb, double* C, long ldc,
                          int M, int N, int K, double alpha, double beta, int order, void* stream);
/* diagnostics: the TN products of csrc/sr_gemm.hip one at a time, for tests that compare a single product with a reference.
 * Every entry checks its arguments BEFORE it touches a device and answers SR_EINVAL (sr_last_error says why) instead of
 * launching: NULL pointers, M / N no multiples of 128, K no multiple of 16, a leading dimension below the width or -- for the
 * operands A and B, whose tiles travel in 16-byte pieces -- odd, operands not 16-byte aligned, odd operand strides of a batch.
 * mode as sr_test_gemm_tn plus 3 (A block-upper-triangular: k ends at m0 + 128) and 4 (A block-lower-triangular: k starts at
 * m0).  Batch: n equally shaped products, member z at A + z sA, B + z sB, C + z sC (doubles); n = 1 is the plain call.
 * prio != 0: the workgroups raise their wavefront priority (same results).
 * _ex: sr_test_gemm_tn / sr_test_gemm_tn_upper with prio and a batch. */
int sr_test_gemm_tn_ex(int device, const double* A, long lda, const double* B, long ldb, double* C, long ldc, int M, int N,
                       int K, double alpha, double beta, int mode, int prio, int n, long sA, long sB, long sC, void* stream);
int sr_test_gemm_tn_upper_ex(int device, const double* A, long lda, const double* B, long ldb, double* C, long ldc, int M,
                             int N, int K, double alpha, double beta, int order, int prio, int n, long sA, long sB, long sC,
                             void* stream);
/* split-K form: C (M x N, contiguous) = alpha A^T B restricted by mode, summed in order from K-slices of ks rows (a
 * multiple of 128) that are written to part first; part_len (doubles) must be at least ceil(K / ks) M N. */
int sr_test_gemm_tn_splitk(int device, const double* A, long lda, const double* B, long ldb, double* C, int M, int N, int K,
                           int ks, double alpha, int mode, double* part, long part_len, void* stream);
/* a list of products in one launch: C_j (M_j x N_j) = alpha A_j^T B_j and, with CTb != NULL, CT_j = C_j^T, at the offsets
 * a, b, c, ct (doubles) of the base pointers, common leading dimension ld.  mode 2: B lower-triangular (k starts at the
 * tile's first column), mode 3: A upper-triangular (k ends behind the tile's last row) -- at the granularity of the
 * workgroup tile, 64 if tiles128 < 1024 and 128 otherwise.  jobs_host is a HOST array (copied to the device for the call);
 * lenA .. lenCT are the lengths of the base buffers in doubles, and every job's rectangles -- of every batch member, sCT
 * being the stride of CTb -- must lie inside them; maxM, maxN: at least every job's M, N (they size the grid). */
typedef struct sr_gemm_job { long a, b, c, ct; int M, N, K, pad; } sr_gemm_job;
int sr_test_gemm_tn_jobs(int device, const double* Ab, long lenA, const double* Bb, long lenB, double* Cb, long lenC,
                         double* CTb, long lenCT, long ld, const sr_gemm_job* jobs_host, int njobs, int maxM, int maxN,
                         long tiles128, double alpha, int mode, int n, long sA, long sB, long sC, long sCT, void* stream);
/* diagnostic: the diagonal-block kernel of the factorisation alone: A (128 x 128 SPD, upper triangle read, leading
 * dimension lda) -> upper Cholesky factor in place, wt = its inverse, w = the inverse transposed (leading dimension
 * ldw); info: device int, 0 or the 1-based first non-positive pivot.  skip: 0 in production; 64 leaves A untouched
 * (back-to-back timing on one input). */
int sr_test_potrf_diag(int device, double* A, long lda, double* wt, double* w, long ldw, int* info, int skip,
                       void* stream);
/* diagnostic: the following persistent multi-step launches of the handle are `drop` workgroups short, so that the last
 * group of rollouts waits for partners that never come: the deterministic way into the time-out path (the tests check
 * that it is reported -- sr_gp_chain_status -- and not silent).  0 restores normal launches. */
int sr_test_chain_drop(sr_gp_t h, int drop);
/* host only: the task plan of the tile-flow Cholesky (csrc/sr_flow.h) for nb block rows -- segs[4 i + 0..3] = first critical
 * task, far task, panel update, position in the one order of block row i (i = 0 .. nb: one behind the last); totals[0..3] =
 * critical tasks, far tasks, panel updates, positions per output. */
int sr_test_flow_plan(int nb, int band, int panel, int* segs, long* totals);
/* n > 0: the next n tile-flow model updates of this process fail ON THE DEVICE (their diagonal-block workgroups never get
 * their go: every wait runs into its time-out, the status word is raised) -- sr_gp_factorize must then repeat the update by
 * launches, and the process' next 16 (then 32, .. 4096) would-be tile flows run by launches too; n = 0: forget that (the tile
 * flow runs again at once). */
int sr_test_flow_fail(int n);
/* diagnostic: the next n launches of the one-launch append of a grid of workgroups (sr_gp_append / sr_gp_append1_host with
 * one point beyond 512 padded rows) wait at their first device-wide barrier for a workgroup that does not exist and give
 * it up after ~5 ms: the deterministic way into the path a grid takes that cannot become resident as a whole (nothing of
 * the model written, the append done by separate launches instead; sr_gp_append1_host answers SR_EBUSY).
 * sr_gp_grid_append_aborts: how often that has happened to h so far. */
int sr_test_grid_append_abort(int n);
int sr_gp_grid_append_aborts(sr_gp_t h, long* n);
/* diagnostic: in-place one-point appends the model's buffers have taken since they were last plain (0: U^-1, alpha and the
 * targets start at their allocations; k: they are views k steps in).  Read-only; tests use it to know which state they met. */
int sr_gp_slide_steps(sr_gp_t h, int* steps);
/* diagnostic: which kernels the last posterior pass of h launched (the last chunk of an sr_gp_predict; the pass inside a
 * reachability step or an append counts too).  Fills out[0 .. min(cap, SR_ROUTE_WORDS)) and returns the words written:
 *   [SR_ROUTE_ID]      SR_ROUTE_K0 one launch, _STREAM1 the VALU streaming kernel (<= 4 columns), _MFMA1 one-chunk MFMA work
 *                      items, _RUNS the MFMA run kernel on the planned work-item table, _K2S streamed groups of 16, _K2B balanced
 *                      shares, _K2M 64 x 64 tiles, _K2 plain tiles; 0 = no pass yet
 *   [SR_ROUTE_SRC]     streamed kernels: 0 columns read from the K* pass, 1 evaluated inside the kernel
 *   [SR_ROUTE_WIDTH]   _STREAM1: columns per thread (1 / 4); _MFMA1 / _RUNS: groups of 16 columns per workgroup (1 / 2 / 4 / 8)
 *   [SR_ROUTE_NC]      columns the streamed kernels work on (1, 4, 16, 32, 64)
 *   [SR_ROUTE_KC]      k-chunks per work item of the plan (1: one-chunk items)
 *   [SR_ROUTE_KR .. _NWG]  _RUNS: rows per run, work items and workgroups per (output, column group)
 *   [SR_ROUTE_MULTI]   _RUNS: 1 = workgroups that run several items one after the other
 *   [SR_ROUTE_REDUCE]  _RUNS: items of the last column block (the reduce kernel's register form holds up to 12)
 *   [SR_ROUTE_POLLED]  _STREAM1: 1 = the polling finaliser on its self-validating slots
 *   [SR_ROUTE_NSPLIT]  splits of the training rows in the mean / Jacobian partial sums
 *   [SR_ROUTE_BAL_WGS] _K2B: workgroups of the balanced launch
 *   [SR_ROUTE_FINAL]   0 final stage inside the posterior kernels, 1 one wavefront per (query, output), 2 one thread per query
 *   [SR_ROUTE_UNSLID]  1 = the pass met an odd slide and put the model back into plain buffers first
 *   [SR_ROUTE_T]       queries of the pass */
#define SR_ROUTE_WORDS 16
enum { SR_ROUTE_ID = 0, SR_ROUTE_SRC, SR_ROUTE_WIDTH, SR_ROUTE_NC, SR_ROUTE_KC, SR_ROUTE_KR, SR_ROUTE_NITEMS, SR_ROUTE_NWG,
       SR_ROUTE_MULTI, SR_ROUTE_REDUCE, SR_ROUTE_POLLED, SR_ROUTE_NSPLIT, SR_ROUTE_BAL_WGS, SR_ROUTE_FINAL, SR_ROUTE_UNSLID,
       SR_ROUTE_T };
enum { SR_ROUTE_K0 = 1, SR_ROUTE_STREAM1, SR_ROUTE_MFMA1, SR_ROUTE_RUNS, SR_ROUTE_K2S, SR_ROUTE_K2B, SR_ROUTE_K2M, SR_ROUTE_K2 };
int sr_gp_last_route(sr_gp_t h, int* out, int cap);
/* diagnostic: how the last model update of h ran -- the last sr_gp_factorize (a sparse fit's factorisation counts too) or the
 * last sr_gp_append / sr_gp_append1_host that succeeded.  Host state only: plain ints the two drivers fill; no kernel, launch or
 * stream depends on them.  Fills out[0 .. min(cap, SR_UPDATE_WORDS)) and returns the words written (SR_EINVAL for a NULL
 * argument or cap < 1):
 *   [SR_UPD_KIND]        0 no update yet, SR_UPD_FIT, SR_UPD_APPEND
 *  after a fit:
 *   [SR_UPD_NB]          blocks of 128 padded rows
 *   [SR_UPD_PANEL]       blocks per Cholesky panel
 *   [SR_UPD_REGIME]      stream regime: 1 chain-bound, 2 two bulk streams
 *   [SR_UPD_OWN_STREAMS] 1 = the update's own streams beside the caller's, 0 = every launch on the caller's stream
 *   [SR_UPD_NPAR]        outputs factorised at once
 *   [SR_UPD_ROUNDS]      rounds of SR_UPD_NPAR outputs
 *   [SR_UPD_INV_STAGES]  stages of the triangular inversion launched beside the chain (per round)
 *   [SR_UPD_FORM]        SR_UPD_PLAIN one chain of launches, SR_UPD_PIPELINED, SR_UPD_FLOW
 *  after an append (the same word positions, other meanings):
 *   [SR_UPD_ROUTE]       SR_UPD_SMALL the matrix-vector route (<= 16 points), SR_UPD_ONE_WG one launch of one workgroup per
 *                        output, SR_UPD_GRID one launch of a grid of workgroups, SR_UPD_TILE the MFMA-tile route (17 .. 128)
 *   [SR_UPD_IN_PLACE]    1 = written into the model's own buffers (the views slide one step)
 *   [SR_UPD_NP0], [SR_UPD_NP1]  padded size before and after
 *   [SR_UPD_SPARE]       1 = the new U^-1 went into the spare buffer kept from an earlier append */
#define SR_UPDATE_WORDS 9
enum { SR_UPD_KIND = 0, SR_UPD_NB, SR_UPD_PANEL, SR_UPD_REGIME, SR_UPD_OWN_STREAMS, SR_UPD_NPAR, SR_UPD_ROUNDS,
       SR_UPD_INV_STAGES, SR_UPD_FORM };
enum { SR_UPD_ROUTE = 1, SR_UPD_IN_PLACE, SR_UPD_NP0, SR_UPD_NP1, SR_UPD_SPARE };
enum { SR_UPD_FIT = 1, SR_UPD_APPEND };
enum { SR_UPD_PLAIN = 0, SR_UPD_PIPELINED, SR_UPD_FLOW };
enum { SR_UPD_SMALL = 0, SR_UPD_ONE_WG, SR_UPD_GRID, SR_UPD_TILE };
int sr_gp_last_update(sr_gp_t h, int* out, int cap);
/* diagnostic: how sr_gp_remove retired its LAST point (host state only: no kernel or launch depends on it).  Fills
 * out[0 .. min(cap, SR_REMOVE_WORDS)), returns the words written (SR_EINVAL: NULL argument, cap < 1):
 *   [SR_RM_COUNT] points retired since the last fit (0: the other words are stale)   [SR_RM_NP0], [SR_RM_NP1] padded size before / after
 *   [SR_RM_OFF0] front padding before   [SR_RM_Q] padded index retired   [SR_RM_SLIDE] slide of the source view (sr_gp_slide_steps)
 *   [SR_RM_ALIGNED] rows kernel: 1 32-byte loads, 0 the 8-byte instance   [SR_RM_SPARE] the factor went into SR_RM_SPARE_NONE a fresh
 *   allocation, _AS_IS the spare buffer as it lay, _CLEARED the spare buffer zeroed first   [SR_RM_VEC_SPARE] 1 = spare alpha / target vectors
 *   reused   [SR_RM_CLEAN] 1 = sr_remove_clean_kernel ran on the slid source's allocation   [SR_RM_KEPT_OLD] 1 = the old buffers became the spares */
#define SR_REMOVE_WORDS 11
enum { SR_RM_COUNT = 0, SR_RM_NP0, SR_RM_NP1, SR_RM_OFF0, SR_RM_Q, SR_RM_SLIDE, SR_RM_ALIGNED, SR_RM_SPARE, SR_RM_VEC_SPARE, SR_RM_CLEAN,
       SR_RM_KEPT_OLD };
enum { SR_RM_SPARE_NONE = 0, SR_RM_SPARE_AS_IS, SR_RM_SPARE_CLEARED };
int sr_gp_last_remove(sr_gp_t h, int* out, int cap);
/* host only: the plan of the streamed MFMA route (csrc/sr_stream.hip) for a model of Np padded rows and n_out outputs, ncols
 * queries (5 .. 128, or 1 .. 4 widened to 16 as the 2 .. 4-query route does: pass 16) on a device of n_cu compute units;
 * can_fuse != 0: the kernel may evaluate its own K* rows (ARD-RBF, D <= 5).  out[0..5] = groups of 16 columns per workgroup,
 * k-chunks per item of the plan, rows per run (0: one-chunk items, no table), work items, workgroups, items of the last column
 * block. */
int sr_test_stream_plan(int Np, int n_out, int ncols, int n_cu, int can_fuse, int* out);
/* host only: how a batch padded to Tp queries splits its sums over the training rows of a model of N points (Np padded rows,
 * a multiple of 128) and n_out outputs, and the widest pass the reverse passes of one step cut their batches into.  out[0] =
 * splits of the mean / Jacobian partial sums (the K* pass), out[1] = splits of the Hessian pass of sr_gp_linearize_batch, out[2] =
 * the pass bound (both counts are those of one query at every width up to it; it does not depend on Tp), out[3] = the batch size
 * beyond which the final stage sums in another order (the bound never exceeds it). */
int sr_test_split_plan(int N, int Np, int n_out, long Tp, int* out);
/* per-kernel hipEvent timing inside the library (adds an event pair per launch while enabled). */
int sr_prof_enable(sr_gp_t h, int on);
int sr_prof_reset (sr_gp_t h);
int sr_prof_get   (sr_gp_t h, int kernel_id, double* ms_total, long* launches);

/* model replication over RCCL for hosts without PyTorch: include/safereach_comm.h (libsafereach_comm.so) */

#ifdef __cplusplus
}
#endif
#endif /* SAFEREACH_H */
