// sr_capi_reach.hip -- the reachability and moment-propagation entry points.
// Forward, with the GP inside: one step and H steps of ellipsoid propagation (mode 0) and of Gaussian moment propagation
// (modes 1 / 2).  Both go through one step function (ell_args, reach_step) and one driver each (onestep_impl, multistep_impl);
// a multi-step call tries the persistent chain kernel first (try_chain, sr_capi_chain.hip).
// Reverse, with the GP inside: one step through onestep_vjp_impl, a whole roll-out through rollout_vjp_impl, in all three
// modes.  Their scratch is the handle's reach_ws, laid out by sr_reach_ws.h.
// Stateless, per query: the ellipsoid and moment steps and their reverse passes, the remainder, the safety distance, the
// roll-out cost, the roll-out constraints and the exploration objective with their reverse passes, the distance to the centre, and
// sampling.
#include "sr_handle.h"
#include "sr_reach_ws.h"
using namespace srh;

static int check_reach_dims(const sr_gp* h, int* n_s, int* n_u) {
    *n_s = h->n_out;
    *n_u = h->D - (h->n_xin ? h->n_xin : h->n_out);
    SR_CHECK(*n_u >= 1, SR_EINVAL, "reachability needs D = n_s + n_u with n_u >= 1 (D=%d, n_out=%d)",
             h->D, h->n_out);
    SR_CHECK(*n_s <= SR_MAX_NS && *n_u <= SR_MAX_NU, SR_EUNSUPPORTED,
             "reachability supports n_s <= %d, n_u <= %d (got %d, %d)", SR_MAX_NS, SR_MAX_NU, *n_s, *n_u);
    return SR_OK;
}

// the reverse passes go through sr_gp_linearize_batch: the widths it is compiled for
static int check_linearize_width(const sr_gp* h, const char* who) {
    SR_CHECK(h->D <= 8, SR_EUNSUPPORTED, "%s: D=%d > 8 (the batched linearisation behind it)", who, h->D);
    return SR_OK;
}

// The one place that fills sr_ell_args: T rows of the step's inputs and outputs with their row strides, the constants and the mode.
// The moment modes read neither l_mu, l_sigma nor c_safety and pass NULL: any valid device pointer will do.  mu, var and jac
// (dense) are the caller's, or reach_step's.
static sr_ell_args ell_args(long T, int n_s, int n_u, int mode, const double* p, long ldp, const double* q, long ldq,
                            const double* k_ff, long ldkff, const double* k_fb, long ldkfb, const double* a, const double* b,
                            const double* l_mu, const double* l_sigma, double c_safety, double* p_out, long ldpo,
                            double* q_out, long ldqo, int* n_bad) {
    sr_ell_args ea;
    ea.T = T; ea.n_s = n_s; ea.n_u = n_u;
    ea.p = p; ea.ldp = ldp; ea.q = q; ea.ldq = ldq;
    ea.k_ff = k_ff; ea.ldkff = ldkff; ea.k_fb = k_fb; ea.ldkfb = ldkfb;
    ea.mu = nullptr; ea.var = nullptr; ea.jac = nullptr;
    ea.a = a; ea.b = b; ea.l_mu = mode ? a : l_mu; ea.l_sigma = mode ? a : l_sigma; ea.c_safety = mode ? 1.0 : c_safety;
    ea.p_out = p_out; ea.ldpo = ldpo; ea.q_out = q_out; ea.ldqo = ldqo;
    ea.n_bad = n_bad; ea.mode = mode;
    return ea;
}

// ... for the T rows from row t0 on of dense arrays (q, k_fb and n_bad may be NULL)
static sr_ell_args ell_args_dense(long T, long t0, int n_s, int n_u, int mode, const double* p, const double* q,
                                  const double* k_ff, const double* k_fb, const double* a, const double* b,
                                  const double* l_mu, const double* l_sigma, double c_safety, double* p_out, double* q_out,
                                  int* n_bad) {
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s;
    return ell_args(T, n_s, n_u, mode, p + t0 * n_s, n_s, q ? q + t0 * nss : nullptr, nss, k_ff + t0 * n_u, n_u,
                    k_fb ? k_fb + t0 * nus : nullptr, nus, a, b, l_mu, l_sigma, c_safety, p_out + t0 * n_s, n_s,
                    q_out + t0 * nss, nss, n_bad);
}

// One step with the GP inside, on the per-step route: the posterior at the rows of ea (mean and Jacobian into the workspace, the
// variances into var, dense), then the step kernel.  var_rows != NULL: the variances are copied there too, row stride ldvar,
// between the two.  The caller has sized the workspace (prepare_ws) and holds its lock.
static int reach_step(sr_gp* h, sr_ell_args ea, double* var, double* var_rows, long ldvar, hipStream_t s) {
    const double* jac_su = nullptr;
    SR_TRY(gp_pass_states(h, ea.T, ea.p, ea.ldp, ea.n_s, ea.k_ff, ea.ldkff, ea.n_u, h->mu, var, &jac_su, s));
    if (var_rows)
        SR_HIP(hipMemcpy2DAsync(var_rows, sizeof(double) * ldvar, var, sizeof(double) * ea.n_s, sizeof(double) * ea.n_s, ea.T,
                                hipMemcpyDeviceToDevice, s));
    ea.mu = h->mu; ea.var = var; ea.jac = jac_su;
    sr_prof_scope ps(&h->prof, SR_K_ELL, s);
    return sr_launch_ellipsoid(ea, s);
}

// sr_onestep_reach (mode 0) and sr_onestep_moments (mode 1 / 2) behind their argument checks
static int onestep_impl(sr_gp* h, long T, int mode, const double* p, const double* q, const double* k_ff, const double* k_fb,
                        const double* a, const double* b, const double* l_mu, const double* l_sigma, double c_safety,
                        double* p_out, double* q_out, double* var_out, int* n_bad, hipStream_t s) {
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    SR_DEVICE(h->device);
    h->last_chain = 0;
    if (mode == 0 && n_s <= 2) {
        // small model, few states: posterior and ellipsoid step in one launch (the chain kernel with H = 1): 24.5 ->
        // 21.5 us per call at N = 200 (host-bound from there).  Not for n_s >= 3: the Jacobi rotations of the
        // eigenvalue bound run on one lane per state inside a 512-thread workgroup there (cart-pole: 25 -> 35 us).
        // Not for the moment modes either: their bits are documented as those of the per-step launches.
        bool chained = false;
        SR_TRY(try_chain(h, T, 1, 0, p, q, k_fb, k_ff, nullptr, a, b, l_mu, l_sigma, c_safety, p_out, q_out, var_out,
                         n_bad, n_s, n_u, s, &chained));
        if (chained) return SR_OK;
    }
    for (long t0 = 0; t0 < T; t0 += h->chunk) {
        const long Tc = std::min(h->chunk, T - t0);
        // gp_pass must not (re)allocate the workspace once internal pointers are resolved
        SR_TRY(prepare_ws(h, Tc));
        sr_ws_lock lock(h);
        SR_TRY(reach_step(h, ell_args_dense(Tc, t0, n_s, n_u, mode, p, q, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_out,
                                            q_out, n_bad),
                          var_out ? var_out + t0 * n_s : h->var, nullptr, 0, s));
    }
    return SR_OK;
}

extern "C" int sr_onestep_reach(sr_gp_t h, long T, const double* p, const double* q,
                                const double* k_ff, const double* k_fb, const double* a,
                                const double* b, const double* l_mu, const double* l_sigma,
                                double c_safety, double* p_out, double* q_out, double* var_out,
                                int* n_bad, void* stream) {
    SR_TRY(handle_ready(h, "sr_onestep_reach"));
    SR_CHECK(T >= 0, SR_EINVAL, "sr_onestep_reach: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(p && k_ff && a && b && l_mu && l_sigma && p_out && q_out, SR_EINVAL,
             "sr_onestep_reach: NULL argument");
    SR_CHECK(q == nullptr || k_fb != nullptr, SR_EINVAL, "sr_onestep_reach: k_fb required with q");
    return onestep_impl(h, T, 0, p, q, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_out, q_out, var_out, n_bad,
                        (hipStream_t)stream);
}

// Moment propagation from a point or from N(mu_x, sigma_x) with the GP inside: the launches of one step of sr_multistep_moments
// on its per-step route (transformed states, posterior with the Jacobian, the moment step of sr_ellipsoid.hip).
extern "C" int sr_onestep_moments(sr_gp_t h, long T, int mode, const double* mu_x, const double* sigma_x, const double* k_ff,
                                  const double* k_fb, const double* a, const double* b, double* mu_out, double* sigma_out,
                                  double* var_out, void* stream) {
    SR_TRY(handle_ready(h, "sr_onestep_moments"));
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_onestep_moments: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && a && b && mu_out && sigma_out, SR_EINVAL, "sr_onestep_moments: NULL argument");
    SR_CHECK(sigma_x == nullptr || k_fb != nullptr, SR_EINVAL, "sr_onestep_moments: k_fb required with sigma_x");
    return onestep_impl(h, T, mode, mu_x, sigma_x, k_ff, k_fb, a, b, nullptr, nullptr, 1.0, mu_out, sigma_out, var_out,
                        nullptr, (hipStream_t)stream);
}

// shared H-step chain: mode 0 = robust ellipsoids (gp_reachability.py:159-212),
// mode 1/2 = Taylor / mean-equivalent Gaussian moments (uncertainty_propagation_casadi.py:88-190)
static int multistep_impl(sr_gp* h, long T, int H, int mode, const double* p0, const double* q0,
                          const double* k_fb0, const double* k_ff, const double* k_fb, const double* a,
                          const double* b, const double* l_mu, const double* l_sigma, double c_safety,
                          double* p_all, double* q_all, double* gp_var_all, int* n_bad, hipStream_t s) {
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    SR_DEVICE(h->device);
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s;
    h->last_chain = 0;
    bool chained = false;
    SR_TRY(try_chain(h, T, H, mode, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_all, q_all, gp_var_all,
                     n_bad, n_s, n_u, s, &chained));
    if (chained) return SR_OK;
    for (long t0 = 0; t0 < T; t0 += h->chunk) {
        const long Tc = std::min(h->chunk, T - t0);
        SR_TRY(prepare_ws(h, Tc));
        sr_ws_lock lock(h);
        for (int i = 0; i < H; ++i) {
            // inputs of step i (gp_reachability.py:195-210): the caller's start, then the outputs of step i - 1
            const long r = t0 * H + i;                                       // the first of the rows of step i, stride H
            const bool first = i == 0;
            const double* kfb_in = first ? (k_fb0 ? k_fb0 + t0 * nus : nullptr) : k_fb + (t0 * (H - 1) + (i - 1)) * nus;
            SR_TRY(reach_step(h, ell_args(Tc, n_s, n_u, mode,
                                          first ? p0 + t0 * n_s : p_all + (r - 1) * n_s, first ? n_s : (long)H * n_s,
                                          first ? (q0 ? q0 + t0 * nss : nullptr) : q_all + (r - 1) * nss, first ? nss : H * nss,
                                          k_ff + r * n_u, (long)H * n_u, kfb_in, first ? nus : (H - 1) * nus,
                                          a, b, l_mu, l_sigma, c_safety, p_all + r * n_s, (long)H * n_s, q_all + r * nss, H * nss,
                                          n_bad),
                              h->var, gp_var_all ? gp_var_all + r * n_s : nullptr, (long)H * n_s, s));
        }
    }
    return SR_OK;
}

extern "C" int sr_multistep_reach(sr_gp_t h, long T, int H, const double* p0, const double* q0,
                                  const double* k_fb0, const double* k_ff, const double* k_fb,
                                  const double* a, const double* b, const double* l_mu,
                                  const double* l_sigma, double c_safety, double* p_all,
                                  double* q_all, int* n_bad, void* stream) {
    SR_TRY(handle_ready(h, "sr_multistep_reach"));
    SR_CHECK(T >= 0 && H >= 1, SR_EINVAL, "sr_multistep_reach: T=%ld H=%d", T, H);
    if (T == 0) return SR_OK;
    SR_CHECK(p0 && k_ff && a && b && l_mu && l_sigma && p_all && q_all, SR_EINVAL,
             "sr_multistep_reach: NULL argument");
    SR_CHECK(H == 1 || k_fb != nullptr, SR_EINVAL, "sr_multistep_reach: k_fb required for H > 1");
    SR_CHECK(q0 == nullptr || k_fb0 != nullptr, SR_EINVAL, "sr_multistep_reach: k_fb0 required with q0");
    return multistep_impl(h, T, H, 0, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_all, q_all,
                          nullptr, n_bad, (hipStream_t)stream);
}

// sr_multistep_reach with the GP variances of every step beside its outputs: the same driver, the same routes, the same bits
extern "C" int sr_multistep_reach_var(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                                      const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
                                      const double* l_sigma, double c_safety, double* p_all, double* q_all, double* gp_var_all,
                                      int* n_bad, void* stream) {
    SR_TRY(handle_ready(h, "sr_multistep_reach_var"));
    SR_CHECK(T >= 0 && H >= 1, SR_EINVAL, "sr_multistep_reach_var: T=%ld H=%d", T, H);
    if (T == 0) return SR_OK;
    SR_CHECK(p0 && k_ff && a && b && l_mu && l_sigma && p_all && q_all, SR_EINVAL, "sr_multistep_reach_var: NULL argument");
    SR_CHECK(H == 1 || k_fb != nullptr, SR_EINVAL, "sr_multistep_reach_var: k_fb required for H > 1");
    SR_CHECK(q0 == nullptr || k_fb0 != nullptr, SR_EINVAL, "sr_multistep_reach_var: k_fb0 required with q0");
    return multistep_impl(h, T, H, 0, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_all, q_all, gp_var_all, n_bad,
                          (hipStream_t)stream);
}

extern "C" int sr_multistep_moments(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* k_ff,
                                    const double* k_fb, const double* a, const double* b, double* mu_all,
                                    double* sigma_all, double* gp_var_all, void* stream) {
    SR_TRY(handle_ready(h, "sr_multistep_moments"));
    SR_CHECK(T >= 0 && H >= 1 && (mode == 1 || mode == 2), SR_EINVAL, "sr_multistep_moments: T=%ld H=%d mode=%d",
             T, H, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && mu_all && sigma_all, SR_EINVAL, "sr_multistep_moments: NULL argument");
    SR_CHECK(H == 1 || k_fb != nullptr, SR_EINVAL, "sr_multistep_moments: k_fb required for H > 1");
    return multistep_impl(h, T, H, mode, mu0, nullptr, nullptr, k_ff, k_fb, a, b, nullptr, nullptr, 1.0, mu_all, sigma_all,
                          gp_var_all, nullptr, (hipStream_t)stream);
}

extern "C" int sr_moment_step(int device, long T, int n_s, int n_u, int mode, const double* mu_x,
                              const double* sigma_x, const double* k_ff, const double* k_fb, const double* mu_g,
                              const double* var_g, const double* jac_g, const double* a, const double* b,
                              double* mu_out, double* sigma_out, void* stream) {
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_moment_step: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && mu_g && var_g && a && b && mu_out && sigma_out, SR_EINVAL, "sr_moment_step: NULL argument");
    SR_CHECK(sigma_x == nullptr || (k_fb != nullptr && (mode == 2 || jac_g != nullptr)), SR_EINVAL,
             "sr_moment_step: k_fb (and jac for the Taylor mode) required with sigma_x");
    SR_DEVICE(device);
    sr_ell_args ea = ell_args_dense(T, 0, n_s, n_u, mode, mu_x, sigma_x, k_ff, k_fb, a, b, nullptr, nullptr, 1.0, mu_out,
                                    sigma_out, nullptr);
    ea.mu = mu_g; ea.var = var_g; ea.jac = jac_g ? jac_g : mu_g;     // never dereferenced in mode 2
    return sr_launch_ellipsoid(ea, (hipStream_t)stream);
}

extern "C" int sr_ellipsoid_step(int device, long T, int n_s, int n_u, const double* p,
                                 const double* q, const double* k_ff, const double* k_fb,
                                 const double* mu, const double* var, const double* jac,
                                 const double* a, const double* b, const double* l_mu,
                                 const double* l_sigma, double c_safety, double* p_out,
                                 double* q_out, int* n_bad, void* stream) {
    SR_CHECK(T >= 0, SR_EINVAL, "sr_ellipsoid_step: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(p && k_ff && mu && var && a && b && l_mu && l_sigma && p_out && q_out, SR_EINVAL,
             "sr_ellipsoid_step: NULL argument");
    SR_CHECK(q == nullptr || (k_fb != nullptr && jac != nullptr), SR_EINVAL,
             "sr_ellipsoid_step: k_fb and jac required with q");
    SR_DEVICE(device);
    sr_ell_args ea = ell_args_dense(T, 0, n_s, n_u, 0, p, q, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_out, q_out, n_bad);
    ea.mu = mu; ea.var = var; ea.jac = jac;
    return sr_launch_ellipsoid(ea, (hipStream_t)stream);
}

// ---- reverse pass of one step (sr_reach_vjp.hip, sr_moments_vjp.hip): stateless, then with the GP inside ------------------------
extern "C" int sr_ellipsoid_step_vjp(int device, long T, int n_s, int n_u, const double* p, const double* q,
                                     const double* k_ff, const double* k_fb, const double* mu, const double* var,
                                     const double* jac, const double* a, const double* b, const double* l_mu,
                                     const double* l_sigma, double c_safety, const double* p1_bar, const double* q1_bar,
                                     double* p_bar, double* q_bar, double* kff_bar, double* kfb_bar, double* mu_bar,
                                     double* var_bar, double* jac_bar, void* stream) {
    SR_CHECK(T >= 0, SR_EINVAL, "sr_ellipsoid_step_vjp: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(p && k_ff && mu && var && a && b && l_mu && l_sigma && p_bar && kff_bar && mu_bar && var_bar, SR_EINVAL,
             "sr_ellipsoid_step_vjp: NULL argument");
    SR_CHECK(q == nullptr || (k_fb && jac && q_bar && kfb_bar && jac_bar), SR_EINVAL,
             "sr_ellipsoid_step_vjp: k_fb, jac, q_bar, kfb_bar and jac_bar required with q");
    SR_CHECK(p1_bar || q1_bar, SR_EINVAL, "sr_ellipsoid_step_vjp: both seeds NULL");
    SR_DEVICE(device);
    sr_ellvjp_args ea{};
    ea.T = T; ea.q = q; ea.k_fb = k_fb; ea.var = var; ea.jac = jac;
    ea.a = a; ea.b = b; ea.l_mu = l_mu; ea.l_sigma = l_sigma; ea.c_safety = c_safety;
    ea.p1_bar = p1_bar; ea.q1_bar = q1_bar;
    ea.p_bar = p_bar; ea.q_bar = q_bar; ea.kff_bar = kff_bar; ea.kfb_bar = kfb_bar;
    ea.mu_bar = mu_bar; ea.var_bar = var_bar; ea.jac_bar = jac_bar;
    return sr_launch_reach_vjp(ea, n_s, n_u, (hipStream_t)stream);
}

// The reverse pass of one step with the GP inside, behind the argument checks of sr_onestep_reach_vjp (mode 0; gpvar_bar NULL)
// and sr_onestep_moments_vjp (mode 1 / 2; l_mu, l_sigma unread).  Per pass: z = [Tz p; k_ff], the GP at z with its first
// derivatives -- and the Hessian of the mean (sr_gp_linearize_batch) only where jac_bar is not zero: modes 0 and 1 from an
// ellipsoid / a Gaussian start --, then one launch of the step's reverse algebra with the GP link behind it.
static int onestep_vjp_impl(sr_gp* h, const char* who, long T, int mode, const double* p, const double* q, const double* k_ff,
                            const double* k_fb, const double* a, const double* b, const double* l_mu, const double* l_sigma,
                            double c_safety, const double* p1_bar, const double* q1_bar, const double* gpvar_bar,
                            double* p_bar, double* q_bar, double* kff_bar, double* kfb_bar, void* stream) {
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    SR_TRY(check_linearize_width(h, who));
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const int D = h->D, n_xin = h->n_xin ? h->n_xin : n_s;
    const double* Tz = h->n_xin ? h->Tz : nullptr;
    const bool second = mode != 2 && q != nullptr;
    const sr_reach_ws_use use{n_s, n_u, D, false, mode, second};
    const long per = sr_reach_ws_carve(use, 0, nullptr).per;
    // a pass: the handle's chunk, at most 2^28 doubles (2 GB) of scratch, and never wider than the batch at which both GP calls
    // still split their sums as the model size alone sets it (sr_common.h): the same bits for any chunk size
    const long chunk = std::max(1L, std::min({h->chunk, sr_stable_pass_max(h->N, h->Np, h->n_out), SR_REACH_WS_MAX_DOUBLES / per}));
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s;
    const long Tw = std::min(chunk, T);
    SR_TRY(h->reach_ws.grow((size_t)(Tw * per), wait::stream(s)));
    const sr_reach_ws w = sr_reach_ws_carve(use, Tw, h->reach_ws.get());
    for (long t0 = 0; t0 < T; t0 += chunk) {
        const long Tc = std::min(chunk, T - t0);
        SR_TRY(sr_launch_reach_z(Tc, n_s, n_u, n_xin, p + t0 * n_s, k_ff + t0 * n_u, Tz, w.z, s));
        if (second) SR_TRY(sr_gp_linearize_batch(h, w.z, Tc, w.mu, w.var, w.jac_mu, w.jac_var, w.hess_mu, stream));
        else SR_TRY(sr_gp_predict_grad(h, w.z, Tc, w.mu, w.var, w.jac_mu, w.jac_var, stream));
        sr_momvjp_args ma{};
        sr_ellvjp_args& ea = ma.e;
        ea.T = Tc; ea.q = q ? q + t0 * nss : nullptr; ea.k_fb = k_fb ? k_fb + t0 * nus : nullptr;
        ea.var = w.var; ea.jac = w.jac_mu;            // (identity transform: the GP's Jacobian is the state-space one)
        ea.a = a; ea.b = b; ea.l_mu = l_mu; ea.l_sigma = l_sigma; ea.c_safety = c_safety;
        ea.p1_bar = p1_bar ? p1_bar + t0 * n_s : nullptr; ea.q1_bar = q1_bar ? q1_bar + t0 * nss : nullptr;
        ea.p_bar = p_bar + t0 * n_s; ea.q_bar = q_bar ? q_bar + t0 * nss : nullptr;
        ea.kff_bar = kff_bar + t0 * n_u; ea.kfb_bar = kfb_bar ? kfb_bar + t0 * nus : nullptr;
        ea.mu_bar = w.mu_bar; ea.var_bar = w.var_bar;
        ea.jac_bar = (second || mode == 0) ? w.jac_bar : nullptr;    // (the ellipsoid kernel writes its zeros from a point too)
        ea.jac_mu = w.jac_mu; ea.jac_var = w.jac_var; ea.hess_mu = second ? w.hess_mu : nullptr; ea.Tz = Tz; ea.D = D; ea.n_xin = n_xin;
        ea.jac_s = w.jac_s; ea.jz = w.jz;
        ma.gpvar_bar = gpvar_bar ? gpvar_bar + t0 * n_s : nullptr; ma.mode = mode;
        sr_prof_scope ps(&h->prof, SR_K_REACH_VJP, s);
        SR_TRY(mode == 0 ? sr_launch_reach_vjp(ea, n_s, n_u, s) : sr_launch_moments_vjp(ma, n_s, n_u, s));
    }
    return SR_OK;
}

extern "C" int sr_onestep_reach_vjp(sr_gp_t h, long T, const double* p, const double* q, const double* k_ff,
                                    const double* k_fb, const double* a, const double* b, const double* l_mu,
                                    const double* l_sigma, double c_safety, const double* p1_bar, const double* q1_bar,
                                    double* p_bar, double* q_bar, double* kff_bar, double* kfb_bar, void* stream) {
    SR_TRY(handle_ready(h, "sr_onestep_reach_vjp"));
    SR_CHECK(T >= 0, SR_EINVAL, "sr_onestep_reach_vjp: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(p && k_ff && a && b && l_mu && l_sigma && p_bar && kff_bar, SR_EINVAL, "sr_onestep_reach_vjp: NULL argument");
    SR_CHECK(q == nullptr || (k_fb && q_bar && kfb_bar), SR_EINVAL, "sr_onestep_reach_vjp: k_fb, q_bar and kfb_bar required with q");
    SR_CHECK(p1_bar || q1_bar, SR_EINVAL, "sr_onestep_reach_vjp: both seeds NULL");
    return onestep_vjp_impl(h, "sr_onestep_reach_vjp", T, 0, p, q, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p1_bar, q1_bar,
                            nullptr, p_bar, q_bar, kff_bar, kfb_bar, stream);
}

extern "C" int sr_onestep_moments_vjp(sr_gp_t h, long T, int mode, const double* mu_x, const double* sigma_x, const double* k_ff,
                                      const double* k_fb, const double* a, const double* b, const double* mu1_bar,
                                      const double* sigma1_bar, const double* gpvar_bar, double* mux_bar, double* sigma_bar,
                                      double* kff_bar, double* kfb_bar, void* stream) {
    SR_TRY(handle_ready(h, "sr_onestep_moments_vjp"));
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_onestep_moments_vjp: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && a && b && mux_bar && kff_bar, SR_EINVAL, "sr_onestep_moments_vjp: NULL argument");
    SR_CHECK(sigma_x == nullptr || (k_fb && sigma_bar && kfb_bar), SR_EINVAL,
             "sr_onestep_moments_vjp: k_fb, sigma_bar and kfb_bar required with sigma_x");
    SR_CHECK(mu1_bar || sigma1_bar || gpvar_bar, SR_EINVAL, "sr_onestep_moments_vjp: every seed NULL");
    return onestep_vjp_impl(h, "sr_onestep_moments_vjp", T, mode, mu_x, sigma_x, k_ff, k_fb, a, b, nullptr, nullptr, 1.0,
                            mu1_bar, sigma1_bar, gpvar_bar, mux_bar, sigma_bar, kff_bar, kfb_bar, stream);
}

// The reverse pass of a whole roll-out, behind the argument checks of sr_multistep_reach_vjp (mode 0: sr_reach_rollout_vjp.hip;
// gpvar_all_bar NULL), sr_multistep_reach_var_vjp (mode 0 with the seed on the GP variances) and sr_multistep_moments_vjp (mode 1 / 2: sr_moments_rollout_vjp.hip; k_fb0, kfb0_bar, l_mu, l_sigma NULL;
// also H rounds of sr_onestep_moments from N(mu0, sigma0)).  Per group of max(1, chunk / H) trajectories: the inputs of all their
// steps (one launch), in mode 0 the eigenpairs of their ellipsoids, the GP derivatives at them in passes bounded as
// onestep_vjp_impl bounds them -- sr_gp_linearize_batch where a step reads the Hessian of the mean (mode 0; mode 1 but for one step
// from a point), else sr_gp_predict_grad --, then the sweep, one thread per trajectory.  A thread owns its trajectory: the grouping
// decides nothing but the size of the scratch.
static int rollout_vjp_impl(sr_gp* h, int n_s, int n_u, long T, int H, int mode, const double* p0, const double* q0,
                            const double* k_fb0, const double* k_ff, const double* k_fb, const double* a, const double* b,
                            const double* l_mu, const double* l_sigma, double c_safety, const double* p_all, const double* q_all,
                            const double* p_all_bar, const double* q_all_bar, const double* gpvar_all_bar, double* p0_bar,
                            double* q0_bar, double* kfb0_bar, double* kff_bar, double* kfb_bar, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const int D = h->D, n_xin = h->n_xin ? h->n_xin : n_s;
    const bool second = mode == 0 || (mode == 1 && (H > 1 || q0 != nullptr));
    const sr_reach_ws_use use{n_s, n_u, D, true, mode, second};
    const long per = sr_reach_ws_carve(use, 0, nullptr).per;
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s, nd = (long)n_s * D;
    // a group: chunk / H trajectories and at most 2^28 doubles (2 GB) of scratch; a pass of GP derivatives: as in onestep_vjp_impl
    const long group = std::max(1L, std::min(h->chunk / H, SR_REACH_WS_MAX_DOUBLES / (per * H)));
    const long pass = std::max(1L, std::min(h->chunk, sr_stable_pass_max(h->N, h->Np, h->n_out)));
    const long Qw = std::min(group, T) * H;
    SR_TRY(h->reach_ws.grow((size_t)(Qw * per), wait::stream(s)));
    const sr_reach_ws w = sr_reach_ws_carve(use, Qw, h->reach_ws.get());
    sr_mrv_args m{};
    sr_rrv_args& r = m.r;
    sr_ellvjp_args& ea = r.e;
    r.z = w.z; r.q_in = w.q_in; r.kfb_in = w.kfb_in; r.p_seed = w.p_seed; r.q_seed = w.q_seed; r.eig = w.eig;
    ea.q = w.q_in; ea.k_fb = w.kfb_in; ea.var = w.var; ea.jac = w.jac_mu;
    ea.a = a; ea.b = b; ea.l_mu = l_mu; ea.l_sigma = l_sigma; ea.c_safety = c_safety;
    ea.p1_bar = w.p_seed; ea.q1_bar = w.q_seed;
    ea.p_bar = w.p_bar; ea.q_bar = w.q_bar; ea.kff_bar = w.kff_bar; ea.kfb_bar = w.kfb_bar;
    ea.mu_bar = w.mu_bar; ea.var_bar = w.var_bar; ea.jac_bar = w.jac_bar;
    ea.jac_mu = w.jac_mu; ea.jac_var = w.jac_var; ea.hess_mu = w.hess_mu; ea.Tz = h->n_xin ? h->Tz : nullptr; ea.D = D; ea.n_xin = n_xin;
    ea.jac_s = w.jac_s; ea.jz = w.jz;
    r.H = H; r.n_s = n_s; r.n_u = n_u;
    m.mode = mode;
    for (long t0 = 0; t0 < T; t0 += group) {
        const long Tg = std::min(group, T - t0), Q = Tg * H;
        ea.T = Tg;
        r.p0 = p0 + t0 * n_s; r.q0 = q0 ? q0 + t0 * nss : nullptr; r.k_fb0 = q0 && k_fb0 ? k_fb0 + t0 * nus : nullptr;
        r.k_ff = k_ff + t0 * H * n_u; r.k_fb = k_fb ? k_fb + t0 * (H - 1) * nus : nullptr;
        r.p_all = p_all + t0 * H * n_s; r.q_all = q_all + t0 * H * nss;
        r.p_all_bar = p_all_bar ? p_all_bar + t0 * H * n_s : nullptr; r.q_all_bar = q_all_bar ? q_all_bar + t0 * H * nss : nullptr;
        r.gpvar_all_bar = gpvar_all_bar ? gpvar_all_bar + t0 * H * n_s : nullptr;
        r.p0_bar = p0_bar + t0 * n_s; r.q0_bar = q0_bar ? q0_bar + t0 * nss : nullptr;
        r.kfb0_bar = kfb0_bar ? kfb0_bar + t0 * nus : nullptr; r.kfb_bar = kfb_bar ? kfb_bar + t0 * (H - 1) * nus : nullptr;
        r.kff_bar = kff_bar + t0 * H * n_u;
        SR_TRY(sr_launch_reach_rollout_prep(r, s));
        if (mode == 0) SR_TRY(sr_launch_reach_rollout_eig(r, s));
        for (long q1 = 0; q1 < Q; q1 += pass) {
            const long Qc = std::min(pass, Q - q1);
            if (second)
                SR_TRY(sr_gp_linearize_batch(h, w.z + q1 * D, Qc, w.mu + q1 * n_s, w.var + q1 * n_s, w.jac_mu + q1 * nd,
                                             w.jac_var + q1 * nd, w.hess_mu + q1 * nd * D, stream));
            else
                SR_TRY(sr_gp_predict_grad(h, w.z + q1 * D, Qc, w.mu + q1 * n_s, w.var + q1 * n_s, w.jac_mu + q1 * nd,
                                          w.jac_var + q1 * nd, stream));
        }
        sr_prof_scope ps(&h->prof, SR_K_REACH_VJP, s);
        SR_TRY(mode == 0 ? sr_launch_reach_rollout_vjp(r, s) : sr_launch_moments_rollout_vjp(m, s));
    }
    return SR_OK;
}

// sr_multistep_reach_vjp (gpvar_all_bar NULL) and sr_multistep_reach_var_vjp behind their shared argument checks
static int multistep_reach_vjp_checked(const char* who, sr_gp_t h, long T, int H, const double* p0, const double* q0,
                                       const double* k_fb0, const double* k_ff, const double* k_fb, const double* a, const double* b,
                                       const double* l_mu, const double* l_sigma, double c_safety, const double* p_all,
                                       const double* q_all, const double* p_all_bar, const double* q_all_bar,
                                       const double* gpvar_all_bar, double* p0_bar, double* q0_bar, double* kfb0_bar, double* kff_bar,
                                       double* kfb_bar, void* stream) {
    SR_TRY(handle_ready(h, who));
    SR_CHECK(T >= 0 && H >= 1, SR_EINVAL, "%s: T=%ld H=%d", who, T, H);
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    SR_TRY(check_linearize_width(h, who));
    if (T == 0) return SR_OK;
    SR_CHECK(p0 && k_ff && a && b && l_mu && l_sigma && p_all && q_all && p0_bar && kff_bar, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H == 1 || (k_fb && kfb_bar), SR_EINVAL, "%s: k_fb and kfb_bar required for H > 1", who);
    SR_CHECK(q0 == nullptr || (k_fb0 && q0_bar && kfb0_bar), SR_EINVAL, "%s: k_fb0, q0_bar and kfb0_bar required with q0", who);
    SR_CHECK(p_all_bar || q_all_bar || gpvar_all_bar, SR_EINVAL, "%s: every seed NULL", who);
    return rollout_vjp_impl(h, n_s, n_u, T, H, 0, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_all, q_all, p_all_bar,
                            q_all_bar, gpvar_all_bar, p0_bar, q0_bar, kfb0_bar, kff_bar, kfb_bar, stream);
}

extern "C" int sr_multistep_reach_vjp(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                                      const double* k_ff, const double* k_fb, const double* a, const double* b,
                                      const double* l_mu, const double* l_sigma, double c_safety, const double* p_all,
                                      const double* q_all, const double* p_all_bar, const double* q_all_bar, double* p0_bar,
                                      double* q0_bar, double* kfb0_bar, double* kff_bar, double* kfb_bar, void* stream) {
    return multistep_reach_vjp_checked("sr_multistep_reach_vjp", h, T, H, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety,
                                       p_all, q_all, p_all_bar, q_all_bar, nullptr, p0_bar, q0_bar, kfb0_bar, kff_bar, kfb_bar, stream);
}

extern "C" int sr_multistep_reach_var_vjp(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                                          const double* k_ff, const double* k_fb, const double* a, const double* b,
                                          const double* l_mu, const double* l_sigma, double c_safety, const double* p_all,
                                          const double* q_all, const double* p_all_bar, const double* q_all_bar,
                                          const double* gpvar_all_bar, double* p0_bar, double* q0_bar, double* kfb0_bar,
                                          double* kff_bar, double* kfb_bar, void* stream) {
    return multistep_reach_vjp_checked("sr_multistep_reach_var_vjp", h, T, H, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma,
                                       c_safety, p_all, q_all, p_all_bar, q_all_bar, gpvar_all_bar, p0_bar, q0_bar, kfb0_bar, kff_bar,
                                       kfb_bar, stream);
}

extern "C" int sr_multistep_moments_vjp(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* sigma0,
                                        const double* k_ff, const double* k_fb, const double* a, const double* b,
                                        const double* mu_all, const double* sigma_all, const double* mu_all_bar,
                                        const double* sigma_all_bar, const double* gpvar_all_bar, double* mu0_bar,
                                        double* sigma0_bar, double* kff_bar, double* kfb_bar, void* stream) {
    const char* who = "sr_multistep_moments_vjp";
    SR_TRY(handle_ready(h, who));
    SR_CHECK(T >= 0 && H >= 1 && (mode == 1 || mode == 2), SR_EINVAL, "%s: T=%ld H=%d mode=%d", who, T, H, mode);
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    SR_TRY(check_linearize_width(h, who));
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && mu_all && sigma_all && mu0_bar && kff_bar, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H == 1 || (k_fb && kfb_bar), SR_EINVAL, "%s: k_fb and kfb_bar required for H > 1", who);
    SR_CHECK(sigma0 == nullptr || sigma0_bar != nullptr, SR_EINVAL, "%s: sigma0 without sigma0_bar", who);
    SR_CHECK(mu_all_bar || sigma_all_bar || gpvar_all_bar, SR_EINVAL, "%s: every seed NULL", who);
    // (sigma0_bar of a point start is not written)
    return rollout_vjp_impl(h, n_s, n_u, T, H, mode, mu0, sigma0, nullptr, k_ff, k_fb, a, b, nullptr, nullptr, 1.0, mu_all, sigma_all,
                            mu_all_bar, sigma_all_bar, gpvar_all_bar, mu0_bar, sigma0 ? sigma0_bar : nullptr, nullptr, kff_bar,
                            kfb_bar, stream);
}

extern "C" int sr_moment_step_vjp(int device, long T, int n_s, int n_u, int mode, const double* mu_x, const double* sigma_x,
                                  const double* k_ff, const double* k_fb, const double* mu_g, const double* var_g,
                                  const double* jac_g, const double* a, const double* b, const double* mu1_bar,
                                  const double* sigma1_bar, double* mux_bar, double* sigma_bar, double* kff_bar, double* kfb_bar,
                                  double* mug_bar, double* var_bar, double* jac_bar, void* stream) {
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_moment_step_vjp: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && mu_g && var_g && a && b && mux_bar && kff_bar && mug_bar && var_bar, SR_EINVAL,
             "sr_moment_step_vjp: NULL argument");
    SR_CHECK(sigma_x == nullptr || (k_fb && (mode == 2 || jac_g) && sigma_bar && kfb_bar && jac_bar), SR_EINVAL,
             "sr_moment_step_vjp: k_fb (and jac_g for the Taylor mode), sigma_bar, kfb_bar and jac_bar required with sigma_x");
    SR_CHECK(mu1_bar || sigma1_bar, SR_EINVAL, "sr_moment_step_vjp: both seeds NULL");
    SR_DEVICE(device);
    sr_momvjp_args ma{};
    ma.e.T = T; ma.e.q = sigma_x; ma.e.k_fb = k_fb; ma.e.var = var_g; ma.e.jac = jac_g;
    ma.e.a = a; ma.e.b = b; ma.e.c_safety = 1.0;
    ma.e.p1_bar = mu1_bar; ma.e.q1_bar = sigma1_bar;
    ma.e.p_bar = mux_bar; ma.e.q_bar = sigma_bar; ma.e.kff_bar = kff_bar; ma.e.kfb_bar = kfb_bar;
    ma.e.mu_bar = mug_bar; ma.e.var_bar = var_bar; ma.e.jac_bar = jac_bar;
    ma.gpvar_bar = nullptr; ma.mode = mode;
    return sr_launch_moments_vjp(ma, n_s, n_u, (hipStream_t)stream);
}

extern "C" int sr_remainder_overapprox(int device, long T, int n_s, int n_u, const double* q,
                                       const double* k_fb, const double* l_mu, const double* l_sigma,
                                       double* u_mu, double* u_sigma, void* stream) {
    SR_CHECK(T >= 0, SR_EINVAL, "sr_remainder_overapprox: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(q && k_fb && l_mu && l_sigma && u_mu && u_sigma, SR_EINVAL,
             "sr_remainder_overapprox: NULL argument");
    SR_DEVICE(device);
    return sr_launch_remainder(T, n_s, n_u, q, k_fb, l_mu, l_sigma, u_mu, u_sigma, (hipStream_t)stream);
}

extern "C" int sr_safety_distance(int device, long T, int n_s, int m, const double* p,
                                  const double* q, const double* h_mat, const double* h_vec,
                                  double c_safety, double* d, void* stream) {
    SR_CHECK(T >= 0 && n_s >= 1 && m >= 1, SR_EINVAL, "sr_safety_distance: T=%ld n_s=%d m=%d", T, n_s, m);
    if (T == 0) return SR_OK;
    SR_CHECK(p && q && h_mat && h_vec && d, SR_EINVAL, "sr_safety_distance: NULL argument");
    SR_DEVICE(device);
    return sr_launch_safety(T, n_s, m, p, q, h_mat, h_vec, c_safety, d, (hipStream_t)stream);
}

// the arguments sr_rollout_cost and sr_rollout_cost_vjp share: checked, then packed; before any launch
static int rollout_cost_args(const char* who, long T, int H, int n_s, int n_u, int idx_angle, double a_trig, int keep_radian, int loss,
                             const double* z, const double* F, double w_stage, double w_term, const double* R, const double* mu,
                             const double* sigma, const double* u, sr_cost_args& c) {
    SR_CHECK(T >= 0 && H >= 1 && n_s >= 1 && n_u >= 0, SR_EINVAL, "%s: T=%ld H=%d n_s=%d n_u=%d", who, T, H, n_s, n_u);
    SR_CHECK(idx_angle >= -1 && idx_angle < n_s, SR_EINVAL, "%s: idx_angle=%d outside -1 .. %d", who, idx_angle, n_s - 1);
    SR_CHECK(loss == 0 || loss == 1, SR_EINVAL, "%s: loss=%d (0 saturating, 1 quadratic)", who, loss);
    SR_CHECK(!(keep_radian && idx_angle < 0), SR_EINVAL, "%s: keep_radian without an angle", who);
    SR_CHECK(z && F && mu, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(!R || (u && n_u >= 1), SR_EINVAL, "%s: R without u", who);
    SR_CHECK(R || !u, SR_EINVAL, "%s: u without R", who);
    SR_CHECK(n_s <= 12 && n_u <= 12, SR_EUNSUPPORTED, "%s: n_s=%d n_u=%d beyond 12", who, n_s, n_u);
    c = sr_cost_args{};
    c.T = T; c.H = H; c.n_s = n_s; c.n_u = n_u; c.idx = idx_angle; c.keep = keep_radian != 0; c.loss = loss;
    c.n_c = idx_angle < 0 ? n_s : (keep_radian ? n_s + 2 : n_s + 1);
    c.a_trig = a_trig; c.w_stage = w_stage; c.w_term = w_term;
    c.z = z; c.F = F; c.R = R; c.mu = mu; c.sigma = sigma; c.u = u;
    return SR_OK;
}

extern "C" int sr_rollout_cost(int device, long T, int H, int n_s, int n_u, int idx_angle, double a_trig, int keep_radian, int loss,
                               const double* z, const double* F, double w_stage, double w_term, const double* R, const double* mu,
                               const double* sigma, const double* u, double* cost, double* cost_steps, void* stream) {
    sr_cost_args c;
    SR_TRY(rollout_cost_args("sr_rollout_cost", T, H, n_s, n_u, idx_angle, a_trig, keep_radian, loss, z, F, w_stage, w_term, R, mu,
                             sigma, u, c));
    SR_CHECK(cost != nullptr, SR_EINVAL, "sr_rollout_cost: NULL argument");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.cost = cost; c.cost_steps = cost_steps;
    return sr_launch_rollout_cost(c, false, (hipStream_t)stream);
}

extern "C" int sr_rollout_cost_vjp(int device, long T, int H, int n_s, int n_u, int idx_angle, double a_trig, int keep_radian, int loss,
                                   const double* z, const double* F, double w_stage, double w_term, const double* R, const double* mu,
                                   const double* sigma, const double* u, const double* cost_bar, double* mu_bar, double* sigma_bar,
                                   double* u_bar, void* stream) {
    sr_cost_args c;
    SR_TRY(rollout_cost_args("sr_rollout_cost_vjp", T, H, n_s, n_u, idx_angle, a_trig, keep_radian, loss, z, F, w_stage, w_term, R,
                             mu, sigma, u, c));
    SR_CHECK(mu_bar || sigma_bar || u_bar, SR_EINVAL, "sr_rollout_cost_vjp: every output NULL");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.cost_bar = cost_bar; c.mu_bar = mu_bar; c.sigma_bar = sigma_bar; c.u_bar = u_bar;
    return sr_launch_rollout_cost(c, true, (hipStream_t)stream);
}

// the arguments sr_rollout_constraints and sr_rollout_constraints_vjp share: checked, then packed; before any launch
static int rollout_constraints_args(const char* who, long T, int H, int n_s, int n_u, const double* p_all, const double* q_all,
                                    const double* k_ff, const double* k_fb, const double* q0, const double* k_fb0, const double* u_min,
                                    const double* u_max, int m_obs, const double* h_obs_mat, const double* h_obs, int m_safe,
                                    const double* h_safe_mat, const double* h_safe, double c_safety, sr_rcn_args& c) {
    SR_CHECK(T >= 0 && H >= 1 && n_s >= 1 && n_u >= 0, SR_EINVAL, "%s: T=%ld H=%d n_s=%d n_u=%d", who, T, H, n_s, n_u);
    SR_CHECK(m_obs >= 0 && m_safe >= 0, SR_EINVAL, "%s: m_obs=%d m_safe=%d", who, m_obs, m_safe);
    SR_CHECK(p_all && q_all, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(!q0 == !k_fb0, SR_EINVAL, "%s: q0 and k_fb0 go together", who);
    SR_CHECK(!u_min == !u_max, SR_EINVAL, "%s: u_min and u_max go together", who);
    const bool bounds = u_min != nullptr;
    SR_CHECK(!bounds || n_u >= 1, SR_EINVAL, "%s: control bounds with n_u=%d", who, n_u);
    SR_CHECK(!bounds || k_ff, SR_EINVAL, "%s: control bounds without k_ff", who);
    SR_CHECK(!bounds || H == 1 || k_fb, SR_EINVAL, "%s: control bounds without k_fb (H=%d)", who, H);
    SR_CHECK(m_obs == 0 || (h_obs_mat && h_obs), SR_EINVAL, "%s: m_obs=%d without h_obs_mat, h_obs", who, m_obs);
    SR_CHECK(m_safe == 0 || (h_safe_mat && h_safe), SR_EINVAL, "%s: m_safe=%d without h_safe_mat, h_safe", who, m_safe);
    const long n_g = (bounds ? 2L * n_u * H : 0L) + (long)m_obs * (H - 1) + m_safe;
    SR_CHECK(n_g > 0, SR_EINVAL, "%s: no constraint rows (no bounds, m_obs (H - 1) = 0, m_safe = 0)", who);
    SR_CHECK(n_s <= 12 && n_u <= 12, SR_EUNSUPPORTED, "%s: n_s=%d n_u=%d beyond 12", who, n_s, n_u);
    SR_CHECK(n_g <= 2147483647L, SR_EUNSUPPORTED, "%s: %ld rows per trajectory", who, n_g);
    c = sr_rcn_args{};
    c.T = T; c.H = H; c.n_s = n_s; c.n_u = n_u; c.m_obs = m_obs; c.m_safe = m_safe; c.n_g = (int)n_g; c.bounds = bounds; c.c = c_safety;
    c.p_all = p_all; c.q_all = q_all; c.k_ff = k_ff; c.k_fb = k_fb; c.q0 = q0; c.kfb0 = k_fb0; c.u_min = u_min; c.u_max = u_max;
    c.h_obs_mat = h_obs_mat; c.h_obs = h_obs; c.h_safe_mat = h_safe_mat; c.h_safe = h_safe;
    return SR_OK;
}

extern "C" int sr_rollout_constraints(int device, long T, int H, int n_s, int n_u, const double* p_all, const double* q_all,
                                      const double* k_ff, const double* k_fb, const double* q0, const double* k_fb0,
                                      const double* u_min, const double* u_max, int m_obs, const double* h_obs_mat,
                                      const double* h_obs, int m_safe, const double* h_safe_mat, const double* h_safe,
                                      double c_safety, double* g, double* g_max, void* stream) {
    sr_rcn_args c;
    SR_TRY(rollout_constraints_args("sr_rollout_constraints", T, H, n_s, n_u, p_all, q_all, k_ff, k_fb, q0, k_fb0, u_min, u_max, m_obs,
                                    h_obs_mat, h_obs, m_safe, h_safe_mat, h_safe, c_safety, c));
    SR_CHECK(g != nullptr, SR_EINVAL, "sr_rollout_constraints: NULL argument");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.g = g; c.g_max = g_max;
    return sr_launch_rollout_constraints(c, false, (hipStream_t)stream);
}

extern "C" int sr_rollout_constraints_vjp(int device, long T, int H, int n_s, int n_u, const double* p_all, const double* q_all,
                                          const double* k_ff, const double* k_fb, const double* q0, const double* k_fb0,
                                          const double* u_min, const double* u_max, int m_obs, const double* h_obs_mat,
                                          const double* h_obs, int m_safe, const double* h_safe_mat, const double* h_safe,
                                          double c_safety, const double* g_bar, double* p_all_bar, double* q_all_bar, double* kff_bar,
                                          double* kfb_bar, double* q0_bar, double* kfb0_bar, void* stream) {
    sr_rcn_args c;
    SR_TRY(rollout_constraints_args("sr_rollout_constraints_vjp", T, H, n_s, n_u, p_all, q_all, k_ff, k_fb, q0, k_fb0, u_min, u_max,
                                    m_obs, h_obs_mat, h_obs, m_safe, h_safe_mat, h_safe, c_safety, c));
    SR_CHECK(g_bar != nullptr, SR_EINVAL, "sr_rollout_constraints_vjp: NULL argument");
    SR_CHECK(p_all_bar || q_all_bar || kff_bar || kfb_bar, SR_EINVAL, "sr_rollout_constraints_vjp: every output NULL");
    SR_CHECK(!q0 || (q0_bar && kfb0_bar), SR_EINVAL, "sr_rollout_constraints_vjp: q0 without q0_bar, kfb0_bar");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.g_bar = g_bar; c.p_all_bar = p_all_bar; c.q_all_bar = q_all_bar; c.kff_bar = kff_bar; c.kfb_bar = kfb_bar;
    c.q0_bar = q0_bar; c.kfb0_bar = kfb0_bar;
    return sr_launch_rollout_constraints(c, true, (hipStream_t)stream);
}

// the arguments sr_rollout_explore and sr_rollout_explore_vjp share: checked, then packed; before any launch
static int rollout_explore_args(const char* who, long T, int kind, int n_s, int H_v, const double* gp_var, double eps, int n_dev,
                                int H_p, const double* p, int H_m, const double* mu, const double* W, sr_xpl_args& c) {
    SR_CHECK(T >= 0 && H_v >= 1 && n_s >= 1, SR_EINVAL, "%s: T=%ld H_v=%d n_s=%d", who, T, H_v, n_s);
    SR_CHECK(kind == 0 || kind == 1, SR_EINVAL, "%s: kind=%d (0 sum, 1 sqrt)", who, kind);
    SR_CHECK(gp_var != nullptr, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(eps >= 0.0, SR_EINVAL, "%s: eps=%g", who, eps);                 // (a NaN eps fails it too)
    SR_CHECK(n_dev >= 0 && n_dev != 1, SR_EINVAL, "%s: n_dev=%d (0: no deviation term, else >= 2)", who, n_dev);
    SR_CHECK(n_dev == 0 || (p && mu && W), SR_EINVAL, "%s: n_dev=%d without p, mu or W", who, n_dev);
    SR_CHECK(n_dev == 0 || (n_dev <= H_p && n_dev <= H_m), SR_EINVAL, "%s: n_dev=%d beyond H_p=%d or H_m=%d", who, n_dev, H_p, H_m);
    SR_CHECK((!p || H_p >= 1) && (!mu || H_m >= 1), SR_EINVAL, "%s: H_p=%d H_m=%d", who, H_p, H_m);
    SR_CHECK(n_s <= 12, SR_EUNSUPPORTED, "%s: n_s=%d beyond 12", who, n_s);
    c = sr_xpl_args{};
    c.T = T; c.kind = kind; c.n_s = n_s; c.H_v = H_v; c.n_dev = n_dev; c.H_p = p ? H_p : 0; c.H_m = mu ? H_m : 0; c.eps = eps;
    c.gp_var = gp_var; c.p = p; c.mu = mu; c.W = W;
    return SR_OK;
}

extern "C" int sr_rollout_explore(int device, long T, int kind, int n_s, int H_v, const double* gp_var, double eps, int n_dev, int H_p,
                                  const double* p, int H_m, const double* mu, const double* W, double* cost, double* cost_steps,
                                  void* stream) {
    sr_xpl_args c;
    SR_TRY(rollout_explore_args("sr_rollout_explore", T, kind, n_s, H_v, gp_var, eps, n_dev, H_p, p, H_m, mu, W, c));
    SR_CHECK(cost != nullptr, SR_EINVAL, "sr_rollout_explore: NULL argument");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.cost = cost; c.cost_steps = cost_steps;
    return sr_launch_rollout_explore(c, false, (hipStream_t)stream);
}

extern "C" int sr_rollout_explore_vjp(int device, long T, int kind, int n_s, int H_v, const double* gp_var, double eps, int n_dev,
                                      int H_p, const double* p, int H_m, const double* mu, const double* W, const double* cost_bar,
                                      double* gpvar_bar, double* p_bar, double* mu_bar, void* stream) {
    sr_xpl_args c;
    SR_TRY(rollout_explore_args("sr_rollout_explore_vjp", T, kind, n_s, H_v, gp_var, eps, n_dev, H_p, p, H_m, mu, W, c));
    SR_CHECK(gpvar_bar || p_bar || mu_bar, SR_EINVAL, "sr_rollout_explore_vjp: every output NULL");
    SR_CHECK((!p_bar || p) && (!mu_bar || mu), SR_EINVAL, "sr_rollout_explore_vjp: p_bar without p, or mu_bar without mu");
    if (T == 0) return SR_OK;
    SR_DEVICE(device);
    c.cost_bar = cost_bar; c.gpvar_bar = gpvar_bar; c.p_bar = p_bar; c.mu_bar = mu_bar;
    return sr_launch_rollout_explore(c, true, (hipStream_t)stream);
}

extern "C" int sr_distance_to_center(int device, long T, int K, int n_s, const double* samples, int per_t,
                                     const double* p, const double* q, double* d, void* stream) {
    SR_CHECK(T >= 0 && K >= 0 && n_s >= 1, SR_EINVAL, "sr_distance_to_center: T=%ld K=%d n_s=%d", T, K, n_s);
    if (T == 0 || K == 0) return SR_OK;
    SR_CHECK(samples && p && q && d, SR_EINVAL, "sr_distance_to_center: NULL argument");
    SR_DEVICE(device);
    return sr_launch_distance(T, K, n_s, samples, per_t, p, q, d, (hipStream_t)stream);
}

extern "C" int sr_gp_sample(int device, long T, int size, int n_out, int n_u, const double* mu,
                            const double* var, const double* eps, double* S, const double* k_fb,
                            const double* k_ff, double* z_next, void* stream) {
    SR_CHECK(T >= 0 && size >= 0 && n_out >= 1 && n_out <= SR_MAX_NS && n_u >= 0, SR_EINVAL,
             "sr_gp_sample: T=%ld size=%d n_out=%d n_u=%d", T, size, n_out, n_u);
    if (T == 0 || size == 0) return SR_OK;
    SR_CHECK(mu && var && eps && S, SR_EINVAL, "sr_gp_sample: NULL argument");
    SR_CHECK(!z_next || n_u == 0 || (k_fb && k_ff), SR_EINVAL, "sr_gp_sample: z_next needs k_fb and k_ff");
    SR_DEVICE(device);
    return sr_launch_sample(T, size, n_out, n_u, mu, var, eps, S, k_fb, k_ff, z_next, (hipStream_t)stream);
}

// tests (host only): the two split rules of sr_common.h and the pass bound the reverse drivers take from them
extern "C" int sr_test_split_plan(int N, int Np, int n_out, long Tp, int* out) {
    SR_CHECK(N >= 1 && Np >= N && Np % SR_NB == 0 && n_out >= 1 && Tp >= 1 && out, SR_EINVAL, "sr_test_split_plan: bad argument");
    out[0] = sr_kstar_nsplit(Np, n_out, Tp);
    out[1] = sr_hess_nsplit(N, n_out, Tp);
    out[2] = (int)sr_stable_pass_max(N, Np, n_out);
    out[3] = SR_FINAL_WAVE_T;
    return SR_OK;
}
