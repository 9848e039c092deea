// sr_capi_moment_match.hip -- the entry points of exact moment matching: the GP's prediction at Gaussian inputs.
// sr_gp_moment_match (ARD-RBF models, and the general family with the RBF radial part) and its reverse pass
// sr_gp_moment_match_vjp work on queries.  sr_gp_moment_match_rollout and sr_gp_moment_match_rollout_vjp take whole closed-loop
// trajectories.  All of them keep their scratch in the handle's mm_ws and cut their batches by mm_chunk below.
// Unlike the reachability entry points they split the GP's input as n_x_in + n_u themselves and have refusals of their own.
#include "sr_handle.h"
using namespace srh;

// at most 2^28 doubles (2 GB) of mm_ws
static constexpr long MM_WS_MAX_DOUBLES = (long)1 << 28;

// A chunk of queries (or trajectories): the handle's, what the launch grid takes, and what the scratch bound leaves at `per`
// doubles each.  Grows mm_ws to `head` doubles in front of the records of the widest chunk of a batch of T.
static int mm_chunk(sr_gp* h, long T, long per, long grid_max, long head, hipStream_t s, long* chunk) {
    *chunk = std::max(1L, std::min({h->chunk, grid_max, MM_WS_MAX_DOUBLES / per}));
    return h->mm_ws.grow((size_t)(head + std::min(*chunk, T) * per), wait::stream(s));
}

// the general family with the RBF radial part (sr_moment_match_gen.hip): the scratch holds the per-call block (Kinv Z,
// Z^T Kinv Z, Z^T alpha of every output) in front of the chunk's records
static int moment_match_general(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k, double* mu,
                                double* cov, double* V, hipStream_t s) {
    const long head = sr_mmx_call_ws(h->N, h->D, h->n_out);
    long chunk;
    SR_TRY(mm_chunk(h, T, sr_mmx_ws_per_query(h->N, h->D, h->n_out), sr_mmx_max_queries(h->N, h->n_out), head, s, &chunk));
    const long DD = (long)h->D * h->D, nn = (long)h->n_out * h->n_out;
    double* call = h->mm_ws.get();
    SR_TRY(sr_launch_moment_match_gen_call(h->Z, h->alpha, h->kp, h->N, h->Np, h->D, h->n_out, inv_k, call, s));
    for (long t0 = 0; t0 < T; t0 += chunk) {
        const long Tc = std::min(chunk, T - t0);
        SR_TRY(sr_launch_moment_match_gen(h->Z, h->alpha, h->kp, h->N, h->Np, h->D, h->n_out, m + t0 * h->D,
                                          S ? S + t0 * DD : nullptr, Tc, inv_k, mu + t0 * h->n_out, cov + t0 * nn,
                                          V ? V + t0 * h->n_out * h->D : nullptr, call, call + head, s));
    }
    return SR_OK;
}

// exact moment matching (sr_moment_match.hip; sr_moment_match_gen.hip for a general-family handle whose outputs all have the
// RBF radial part).  Reads the model where the handle holds it (alpha may be a slid view: single
// doubles are loaded, no unslide()); writes nothing into the handle but the grow-only scratch.
extern "C" int sr_gp_moment_match(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k, double* mu,
                                  double* cov, double* V, void* stream) {
    SR_TRY(handle_ready(h, "sr_gp_moment_match"));
    hipStream_t s = (hipStream_t)stream;
    if (h->general) {
        SR_DEVICE(h->device);
        SR_TRY(general_info(h, s));
        if (!h->gen_rbf) {
            sr_set_error("sr_gp_moment_match: the closed form is for ARD-RBF models and the general family with the RBF "
                         "radial part only (a Matern output has none)");
            return SR_EUNSUPPORTED;
        }
    }
    SR_CHECK(T >= 0, SR_EINVAL, "sr_gp_moment_match: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(m && inv_k && mu && cov, SR_EINVAL, "sr_gp_moment_match: NULL argument");
    SR_DEVICE(h->device);
    if (h->general) return moment_match_general(h, m, S, T, inv_k, mu, cov, V, s);
    long chunk;
    SR_TRY(mm_chunk(h, T, sr_mm_ws_per_query(h->N, h->D, h->n_out), sr_mm_max_queries(h->N, h->n_out), 0, s, &chunk));
    const long DD = (long)h->D * h->D, nn = (long)h->n_out * h->n_out;
    for (long t0 = 0; t0 < T; t0 += chunk) {
        const long Tc = std::min(chunk, T - t0);
        SR_TRY(sr_launch_moment_match(h->Z, h->alpha, h->ls, h->sf2, h->N, h->Np, h->D, h->n_out, m + t0 * h->D,
                                      S ? S + t0 * DD : nullptr, Tc, inv_k, mu + t0 * h->n_out, cov + t0 * nn,
                                      V ? V + t0 * h->n_out * h->D : nullptr, h->mm_ws.get(), s));
    }
    return SR_OK;
}

// the reverse pass of sr_gp_moment_match: the same refusals in the same order, the same scratch (its own per-query size)
extern "C" int sr_gp_moment_match_vjp(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k,
                                      const double* mu_bar, const double* cov_bar, const double* V_bar, double* m_bar,
                                      double* S_bar, void* stream) {
    SR_TRY(handle_ready(h, "sr_gp_moment_match_vjp"));
    if (h->general) {
        sr_set_error("sr_gp_moment_match_vjp: the reverse pass is for ARD-RBF models only (data set with sr_gp_set_data)");
        return SR_EUNSUPPORTED;
    }
    SR_CHECK(T >= 0, SR_EINVAL, "sr_gp_moment_match_vjp: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(m && inv_k && (m_bar || S_bar), SR_EINVAL, "sr_gp_moment_match_vjp: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    long chunk;
    SR_TRY(mm_chunk(h, T, sr_mmg_ws_per_query(h->N, h->D, h->n_out), sr_mmg_max_queries(h->N, h->n_out), 0, s, &chunk));
    const long Dl = h->D, DD = Dl * Dl, n = h->n_out;
    for (long t0 = 0; t0 < T; t0 += chunk) {
        const long Tc = std::min(chunk, T - t0);
        SR_TRY(sr_launch_moment_match_vjp(h->Z, h->alpha, h->ls, h->sf2, h->N, h->Np, h->D, h->n_out, m + t0 * Dl,
                                          S ? S + t0 * DD : nullptr, Tc, inv_k, mu_bar ? mu_bar + t0 * n : nullptr,
                                          cov_bar ? cov_bar + t0 * n * n : nullptr, V_bar ? V_bar + t0 * n * Dl : nullptr,
                                          m_bar ? m_bar + t0 * Dl : nullptr, S_bar ? S_bar + t0 * DD : nullptr,
                                          h->mm_ws.get(), s));
    }
    return SR_OK;
}

// T trajectories through H closed-loop steps of exact moment matching in one launch per chunk (sr_moment_match_rollout.hip).
// Every refusal comes before the first launch; the scratch holds one step's records per trajectory of a chunk.  A workgroup
// owns a trajectory, so the chunk decides nothing but the size of the scratch.
extern "C" int sr_gp_moment_match_rollout(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj, const double* mu0,
                                          const double* sigma0, const double* k_ff, const double* k_fb, const double* a,
                                          const double* b, const double* tz, const double* inv_k, double* mu_all,
                                          double* sigma_all, double* cov_all, void* stream) {
    const char* who = "sr_gp_moment_match_rollout";
    SR_TRY(handle_ready(h, who));
    SR_CHECK(!h->general, SR_EUNSUPPORTED, "%s: ARD-RBF models only (data set with sr_gp_set_data): use the per-step route", who);
    SR_CHECK(h->N <= 1024, SR_EUNSUPPORTED, "%s: N=%d > 1024: use the per-step route", who, h->N);
    SR_CHECK(h->D <= 12, SR_EUNSUPPORTED, "%s: D=%d > 12: use the per-step route", who, h->D);
    SR_CHECK(T >= 0 && H >= 1 && (gains_per_traj == 0 || gains_per_traj == 1), SR_EINVAL, "%s: T=%ld H=%d gains_per_traj=%d",
             who, T, H, gains_per_traj);
    SR_CHECK(n_x_in >= 1 && n_x_in <= h->D - 1, SR_EINVAL, "%s: n_x_in=%d outside 1 .. D - 1 (D=%d)", who, n_x_in, h->D);
    SR_CHECK(tz != nullptr || n_x_in == h->n_out, SR_EINVAL, "%s: tz NULL needs n_x_in == n_out (%d, %d)", who, n_x_in,
             h->n_out);
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && inv_k && mu_all && sigma_all && (k_fb || H == 1), SR_EINVAL, "%s: NULL argument", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    long chunk;
    SR_TRY(mm_chunk(h, T, sr_mmr_ws_per_traj(h->D, h->n_out), 0x7fffffffL, 0, s, &chunk));
    const long n = h->n_out, n_u = h->D - n_x_in;
    sr_mmr_args r;
    r.Z = h->Z; r.alpha = h->alpha; r.ls = h->ls; r.sf2 = h->sf2; r.inv_k = inv_k; r.a = a; r.b = b; r.tz = tz;
    r.ws = h->mm_ws.get();
    r.N = h->N; r.Np = h->Np; r.D = h->D; r.n_out = h->n_out; r.n_x_in = n_x_in; r.H = H; r.gains_per_traj = gains_per_traj;
    for (long t0 = 0; t0 < T; t0 += chunk) {
        r.T = std::min(chunk, T - t0);
        r.mu0 = mu0 + t0 * n;
        r.sigma0 = sigma0 ? sigma0 + t0 * n * n : nullptr;
        r.k_ff = k_ff + (gains_per_traj ? t0 * H * n_u : 0);
        r.k_fb = k_fb ? k_fb + (gains_per_traj ? t0 * (H - 1) * n_u * n : 0) : nullptr;
        r.mu_all = mu_all + t0 * H * n;
        r.sigma_all = sigma_all + t0 * H * n * n;
        r.cov_all = cov_all ? cov_all + t0 * H * n * n : nullptr;
        SR_TRY(sr_launch_moment_match_rollout(r, s));
    }
    return SR_OK;
}

// The reverse pass of that roll-out (sr_moment_match_rollout_vjp.hip) at the states a forward stored.  Its domain is that of
// sr_gp_moment_match_vjp (any N), not of the fused forward.  Every refusal comes before the first launch.  Trajectories go in
// groups of max(1, min(chunk, sr_mmg_max_queries) / H): a trajectory's results depend on nothing but its own rows, so the
// group size decides the size of the scratch and how full the one-off pass runs, not a bit of the results.  (Not mm_chunk: the
// handle's chunk and the launch grid bound the group's queries, the scratch bound its trajectories.)
extern "C" int sr_gp_moment_match_rollout_vjp(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj, const double* mu0,
                                              const double* sigma0, const double* k_ff, const double* k_fb, const double* a,
                                              const double* b, const double* tz, const double* inv_k, const double* mu_all,
                                              const double* sigma_all, const double* mu_all_bar, const double* sigma_all_bar,
                                              const double* cov_all_bar, double* mu0_bar, double* sigma0_bar, double* kff_bar,
                                              double* kfb_bar, void* stream) {
    const char* who = "sr_gp_moment_match_rollout_vjp";
    SR_TRY(handle_ready(h, who));
    SR_CHECK(!h->general, SR_EUNSUPPORTED, "%s: the reverse pass is for ARD-RBF models only (data set with sr_gp_set_data)", who);
    SR_CHECK(h->D <= SR_MAX_D, SR_EUNSUPPORTED, "%s: D=%d > %d", who, h->D, SR_MAX_D);
    SR_CHECK(h->n_out <= SR_MMRV_MAX_NS, SR_EUNSUPPORTED, "%s: n_s=%d > %d (the sweep kernel's matrices in LDS)", who, h->n_out,
             SR_MMRV_MAX_NS);
    SR_CHECK(T >= 0 && H >= 1 && (gains_per_traj == 0 || gains_per_traj == 1), SR_EINVAL, "%s: T=%ld H=%d gains_per_traj=%d",
             who, T, H, gains_per_traj);
    SR_CHECK(n_x_in >= 1 && n_x_in <= h->D - 1, SR_EINVAL, "%s: n_x_in=%d outside 1 .. D - 1 (D=%d)", who, n_x_in, h->D);
    SR_CHECK(tz != nullptr || n_x_in == h->n_out, SR_EINVAL, "%s: tz NULL needs n_x_in == n_out (%d, %d)", who, n_x_in,
             h->n_out);
    SR_CHECK(H <= sr_mmg_max_queries(h->N, h->n_out), SR_EUNSUPPORTED, "%s: H=%d steps of N=%d, n_out=%d outside the launch grid",
             who, H, h->N, h->n_out);
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && inv_k && mu_all && sigma_all && mu0_bar && kff_bar && (H == 1 || (k_fb && kfb_bar)),
             SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(sigma0 == nullptr || sigma0_bar != nullptr, SR_EINVAL, "%s: sigma0 without sigma0_bar", who);
    SR_CHECK(mu_all_bar || sigma_all_bar || cov_all_bar, SR_EINVAL, "%s: all seeds NULL", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const long per = sr_mmrv_ws_per_traj(h->N, h->D, h->n_out, H);
    const long queries = std::max(1L, std::min(h->chunk, sr_mmg_max_queries(h->N, h->n_out)));
    const long group = std::max(1L, std::min(queries / H, MM_WS_MAX_DOUBLES / per));
    SR_TRY(h->mm_ws.grow((size_t)(std::min(group, T) * per), wait::stream(s)));
    const long n = h->n_out, n_u = h->D - n_x_in;
    sr_mmrv_args r{};
    r.Z = h->Z; r.alpha = h->alpha; r.ls = h->ls; r.sf2 = h->sf2; r.inv_k = inv_k; r.a = a; r.b = b; r.tz = tz;
    r.N = h->N; r.Np = h->Np; r.D = h->D; r.n_s = h->n_out; r.n_x_in = n_x_in; r.H = H; r.gains_per_traj = gains_per_traj;
    for (long t0 = 0; t0 < T; t0 += group) {
        r.Tg = std::min(group, T - t0);
        r.mu0 = mu0 + t0 * n;
        r.sigma0 = sigma0 ? sigma0 + t0 * n * n : nullptr;
        r.k_ff = k_ff + (gains_per_traj ? t0 * H * n_u : 0);
        r.k_fb = k_fb ? k_fb + (gains_per_traj ? t0 * (H - 1) * n_u * n : 0) : nullptr;
        r.mu_all = mu_all + t0 * H * n;
        r.sigma_all = sigma_all + t0 * H * n * n;
        r.mu_all_bar = mu_all_bar ? mu_all_bar + t0 * H * n : nullptr;
        r.sigma_all_bar = sigma_all_bar ? sigma_all_bar + t0 * H * n * n : nullptr;
        r.cov_all_bar = cov_all_bar ? cov_all_bar + t0 * H * n * n : nullptr;
        r.mu0_bar = mu0_bar + t0 * n;
        r.sigma0_bar = sigma0 ? sigma0_bar + t0 * n * n : nullptr;
        r.kff_bar = kff_bar + t0 * H * n_u;
        r.kfb_bar = H > 1 ? kfb_bar + t0 * (H - 1) * n_u * n : nullptr;
        SR_TRY(sr_launch_moment_match_rollout_vjp(r, h->mm_ws.get(), s));
    }
    return SR_OK;
}
