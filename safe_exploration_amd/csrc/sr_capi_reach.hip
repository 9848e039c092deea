// sr_capi_reach.hip -- reachability entry points: one-step and multi-step ellipsoid propagation (mode 0) and Gaussian moment
// propagation (modes 1 / 2) through one forward step (ell_args, reach_step) and one driver each (onestep_impl, multistep_impl);
// the reverse pass of one step of either through one driver (onestep_vjp_impl) and of a whole roll-out (sr_multistep_reach_vjp, mode 0; sr_multistep_moments_vjp, modes 1 / 2); exact moment matching, its reverse pass and
// its roll-out in one launch; the stateless per-query steps (ellipsoid, moments, their reverse passes, remainder, safety distance, the roll-out cost and its reverse pass, distance to centre, sampling);
// and the dispatch of the persistent chain kernel (sr_chain.hip K0c) with its process-wide launch gate.
#include "sr_handle.h"
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

static int try_chain(sr_gp* h, long T, int H, int mode, const double* p0, const double* q0, const double* k_fb0,
                     const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
                     const double* l_sigma, double c_safety, double* p_all, double* q_all, double* gp_var_all,
                     int* n_bad, int n_s, int n_u, hipStream_t s, bool* taken);

// The one place that fills sr_ell_args: T rows of the step's inputs and outputs with their row strides, the constants and the mode.
// The moment modes read neither l_mu, l_sigma nor c_safety: any valid device pointer will do.  mu, var and jac (dense) are the
// caller's, or reach_step's.
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_onestep_reach: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_onestep_reach: model not factorized");
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_onestep_moments: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_onestep_moments: model not factorized");
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_onestep_moments: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && a && b && mu_out && sigma_out, SR_EINVAL, "sr_onestep_moments: NULL argument");
    SR_CHECK(sigma_x == nullptr || k_fb != nullptr, SR_EINVAL, "sr_onestep_moments: k_fb required with sigma_x");
    return onestep_impl(h, T, mode, mu_x, sigma_x, k_ff, k_fb, a, b, nullptr, nullptr, 1.0, mu_out, sigma_out, var_out,
                        nullptr, (hipStream_t)stream);
}

// Persistent chain launches of one device never overlap, whichever handle or stream they come from: each needs (almost)
// every CU resident at once, two of them side by side would wait for each other's workgroups until the time-out.  Every
// launch waits for the event the previous one recorded (per device, process-wide) and records its own.  Not while the
// caller's stream is being captured into a graph (a cross-stream wait on an uncaptured event is not capturable): a
// captured chain is ordered by its graph.
struct sr_chain_gate { std::mutex m; hipEvent_t ev[32] = {}; hipStream_t last[32] = {}; bool any[32] = {}; };
static sr_chain_gate g_chain_gate;
struct sr_chain_turn {                 // holds the gate from the wait to the record: host threads take turns too
    int device; hipStream_t s; bool active = false;
    sr_chain_turn(int device_, hipStream_t s_) : device(device_), s(s_) {}
    int enter() {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        const hipError_t ce = hipStreamIsCapturing(s, &st);
        const bool capturing = (ce == hipSuccess && st != hipStreamCaptureStatusNone);
        if (capturing || device < 0 || device >= 32) return SR_OK;
        g_chain_gate.m.lock();
        active = true;
        // (the previous launch on the SAME stream is ordered by the stream itself)
        if (g_chain_gate.ev[device] && !(g_chain_gate.any[device] && g_chain_gate.last[device] == s))
            SR_HIP(hipStreamWaitEvent(s, g_chain_gate.ev[device], 0));
        return SR_OK;
    }
    int leave() {
        if (!active) return SR_OK;
        if (!g_chain_gate.ev[device]) SR_HIP(hipEventCreateWithFlags(&g_chain_gate.ev[device], hipEventDisableTiming));
        SR_HIP(hipEventRecord(g_chain_gate.ev[device], s));
        g_chain_gate.last[device] = s; g_chain_gate.any[device] = true;
        return SR_OK;
    }
    ~sr_chain_turn() { if (active) g_chain_gate.m.unlock(); }
};

// The persistent kernel of sr_chain.hip (K0c) for a chain of H >= 1 steps, where it applies; *taken says whether it ran.
static int try_chain(sr_gp* h, long T, int H, int mode, const double* p0, const double* q0, const double* k_fb0,
                     const double* k_ff, const double* k_fb, const double* a, const double* b, const double* l_mu,
                     const double* l_sigma, double c_safety, double* p_all, double* q_all, double* gp_var_all,
                     int* n_bad, int n_s, int n_u, hipStream_t s, bool* taken) {
    *taken = false;
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s;
    // small model, few rollouts: the whole chain in one launch (sr_chain.hip K0c).  One launch holds SR_CHAIN_GROUPS
    // workgroups = gmax groups of 16 rollouts (n_s Np / 128 posterior workgroups + the tail workgroup each): 768 rollouts
    // of a pendulum model with N <= 256, 416 of a cart-pole model.  Measured at N = 200, H = 15: 256 rollouts 246
    // (per-step launches) -> 102 us.
    // every workgroup of a launch must be resident (one per CU): leave 16 CUs of whatever this device (or partition of
    // a device) has to other work
    if (h->chain_cap < 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 0;
        h->chain_cap = std::max(0, std::min(SR_CHAIN_GROUPS, cus - 16));
    }
    const int wpg = sr_chain_wgs_per_group(h->Np, n_s);                 // posterior workgroups + the tail workgroup
    if (h->chain_cap < wpg) return SR_OK;                               // not even one group fits: per-step launches
    // A chain launch whose hand-off timed out (SR_CHAIN_TIMEOUT_TICKS: its workgroups were not co-resident in time) has
    // poisoned its outputs with NaN and raised the pinned status word.  The first entry after that reports it -- a
    // caller that never looked at the outputs must not go on with them -- and the handle takes the per-step launches
    // from here on (sr_gp_set_chain(h, 1) re-arms the persistent kernel).
    if (h->chain_status_host && *(volatile int*)h->chain_status_host != 0) {
        *(volatile int*)h->chain_status_host = 0;
        h->chain = 0;
        sr_set_error("a previous persistent multi-step launch timed out (its workgroups did not become co-resident within "
                     "100 ms); its outputs were filled with NaN.  The handle now uses per-step launches; repeat the call.");
        return SR_ESTATE;
    }
    const long xpg = std::max(1l, sr_chain_xels_per_group(h->Np, n_s, n_u, H));
    const int gmax = (int)std::max(1l, std::min((long)(h->chain_cap / wpg), (long)SR_CHAIN_XELS / xpg));   // groups of 16 rollouts per launch
    const long chain_launches = ((T + SR_SMALL_T - 1) / SR_SMALL_T + gmax - 1) / gmax;
    // Several launches in a row still beat the per-step route (N = 200, H = 15: 1024 rollouts 203 against 253 us, 4096
    // rollouts in six launches 608 against 722 us; cart-pole N = 150: 832 rollouts 304 against 411 us) -- except where
    // the per-step route still has its one-launch posterior (T <= SR_FUSED_T) and three launches are needed (cart-pole,
    // 960 rollouts: 454 against 413 us).
    // (one or two steps: a second launch costs what the per-step route's two launches per step cost -- N = 200, H = 1,
    //  960 rollouts: 29 against 24 us)
    const long chain_max_launches = sr_chain_max_launches(T, H);
    if (h->chain && h->small_path == 1 && !h->force_stream && !h->general && h->n_xin == 0 &&
        chain_launches <= chain_max_launches &&
        sr_chain_supported(h->Np, h->D, n_s, n_u, H)) {
        // the kernel must be able to run at all: at least one workgroup per CU (registers, static + dynamic LDS)
        const int occ_key = ((h->Np * 8 + n_s) * 8 + n_u) * 128 + std::min(H, 127);      // (H sizes the dynamic LDS; sr_chain_supported bounds it at 96)
        if (h->chain_occ_key != occ_key) {
            h->chain_occ_blocks = 0;
            SR_TRY(sr_chain_blocks_per_cu(h->Np, n_s, n_u, H, &h->chain_occ_blocks));
            h->chain_occ_key = occ_key;
        }
        if (h->chain_occ_blocks < 1) return SR_OK;                       // per-step launches
        if (!h->chain_xch) {
            // all or nothing: the pointers are committed to the handle only once every allocation and memset is in place
            // (a launch with one of them missing would run on NULL epoch / alive / done words)
            int* st_host = h->chain_status_host; int* st_dev = h->chain_status_dev;
            sr_xel* xch = nullptr; unsigned long long* tickets = nullptr; unsigned* done = nullptr;
            int rc = SR_OK;
            hipError_t he = hipSuccess;
            if (!st_host) {
                he = hipHostMalloc((void**)&st_host, sizeof(int), hipHostMallocMapped);
                if (he == hipSuccess) { *st_host = 0; he = hipHostGetDevicePointer((void**)&st_dev, st_host, 0); }
            }
            if (he == hipSuccess) rc = dev_alloc(&xch, (size_t)SR_CHAIN_XELS);
            if (he == hipSuccess && rc == SR_OK) rc = dev_alloc(&tickets, (size_t)2 * SR_CHAIN_GROUPS);
            if (he == hipSuccess && rc == SR_OK) rc = dev_alloc(&done, (size_t)SR_CHAIN_GROUPS);
            // ON THE CALLER'S STREAM: a memset on the null stream is not ordered with a launch on a non-blocking stream --
            // it wiped tags the first launch had already written (41 MB take 20 us) and that launch timed out
            if (he == hipSuccess && rc == SR_OK) he = hipMemsetAsync(xch, 0, sizeof(sr_xel) * (size_t)SR_CHAIN_XELS, s);     // tag 0 = never written
            if (he == hipSuccess && rc == SR_OK) he = hipMemsetAsync(tickets, 0, sizeof(unsigned long long) * 2 * SR_CHAIN_GROUPS, s);
            if (he == hipSuccess && rc == SR_OK) he = hipMemsetAsync(done, 0, sizeof(unsigned) * SR_CHAIN_GROUPS, s);
            if (he != hipSuccess || rc != SR_OK) {
                if (he != hipSuccess) {
                    (void)hipStreamSynchronize(s);
                    sr_set_error("persistent chain: setting up the exchange buffers -> %s", hipGetErrorString(he));
                    (void)hipGetLastError();
                    rc = SR_EHIP;
                }
                dev_free(xch); dev_free(tickets); dev_free(done);
                if (st_host && !h->chain_status_host) (void)hipHostFree(st_host);
                return rc;
            }
            h->chain_status_host = st_host; h->chain_status_dev = st_dev;
            h->chain_xch = xch; h->chain_tickets = tickets; h->chain_done = done;
        }
        // every workgroup of a chain launch must be resident at once: resident single-query servers (up to n_out Np / 64 CUs
        // each) leave the device first; they come back with their next query
        servers_quiesce_device(h->device);
        sr_prof_scope ps(&h->prof, SR_K_SMALL, s);
        for (long t0 = 0; t0 < T; t0 += (long)gmax * SR_SMALL_T) {
            const long Tc = std::min((long)gmax * SR_SMALL_T, T - t0);
            const int groups = (int)((Tc + SR_SMALL_T - 1) / SR_SMALL_T);
            sr_chain_args ca{};
            model_args(ca.k, h);
            ca.k.na = n_s; ca.k.nb = n_u;
            ca.Wt = h->Wt; ca.T = Tc; ca.H = H; ca.mode = mode;
            ca.p0 = p0 + t0 * n_s; ca.q0 = q0 ? q0 + t0 * nss : nullptr; ca.k_fb0 = k_fb0 ? k_fb0 + t0 * nus : nullptr;
            ca.k_ff = k_ff + t0 * H * n_u; ca.k_fb = k_fb ? k_fb + t0 * (H - 1) * nus : nullptr;
            ca.a = a; ca.b = b; ca.l_mu = l_mu; ca.l_sigma = l_sigma; ca.c_safety = c_safety;
            ca.p_all = p_all + t0 * H * n_s; ca.q_all = q_all + t0 * H * nss;
            ca.gp_var_all = gp_var_all ? gp_var_all + t0 * H * n_s : nullptr;
            ca.n_bad = n_bad; ca.xch = h->chain_xch;
            ca.epoch = h->chain_tickets; ca.alive = h->chain_tickets + SR_CHAIN_GROUPS; ca.done = h->chain_done;
            ca.status = h->chain_status_dev;
            ca.test_drop = h->chain_test_drop;
            sr_chain_turn turn(h->device, s);
            SR_TRY(turn.enter());
            SR_TRY(sr_launch_chain(ca, s));
            SR_TRY(turn.leave());
            (void)groups;
        }
        h->last_chain = 1;
        *taken = true;
        return SR_OK;
    }
    return SR_OK;
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_multistep_reach: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_multistep_reach: model not factorized");
    SR_CHECK(T >= 0 && H >= 1, SR_EINVAL, "sr_multistep_reach: T=%ld H=%d", T, H);
    if (T == 0) return SR_OK;
    SR_CHECK(p0 && k_ff && a && b && l_mu && l_sigma && p_all && q_all, SR_EINVAL,
             "sr_multistep_reach: NULL argument");
    SR_CHECK(H == 1 || k_fb != nullptr, SR_EINVAL, "sr_multistep_reach: k_fb required for H > 1");
    SR_CHECK(q0 == nullptr || k_fb0 != nullptr, SR_EINVAL, "sr_multistep_reach: k_fb0 required with q0");
    return multistep_impl(h, T, H, 0, p0, q0, k_fb0, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p_all, q_all,
                          nullptr, n_bad, (hipStream_t)stream);
}

extern "C" int sr_multistep_moments(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* k_ff,
                                    const double* k_fb, const double* a, const double* b, double* mu_all,
                                    double* sigma_all, double* gp_var_all, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_multistep_moments: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_multistep_moments: model not factorized");
    SR_CHECK(T >= 0 && H >= 1 && (mode == 1 || mode == 2), SR_EINVAL, "sr_multistep_moments: T=%ld H=%d mode=%d",
             T, H, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && mu_all && sigma_all, SR_EINVAL, "sr_multistep_moments: NULL argument");
    SR_CHECK(H == 1 || k_fb != nullptr, SR_EINVAL, "sr_multistep_moments: k_fb required for H > 1");
    // l_mu / l_sigma are unused by the moment modes: any valid device pointer will do
    return multistep_impl(h, T, H, mode, mu0, nullptr, nullptr, k_ff, k_fb, a, b, a, a, 1.0, mu_all, sigma_all,
                          gp_var_all, nullptr, (hipStream_t)stream);
}

// the general family with the RBF radial part (sr_moment_match_gen.hip): the scratch holds the per-call block (Kinv Z,
// Z^T Kinv Z, Z^T alpha of every output) in front of the chunk's records
static int moment_match_general(sr_gp_t h, const double* m, const double* S, long T, const double* inv_k, double* mu,
                                double* cov, double* V, hipStream_t s) {
    const long per = sr_mmx_ws_per_query(h->N, h->D, h->n_out), head = sr_mmx_call_ws(h->N, h->D, h->n_out);
    const long chunk = std::max(1L, std::min({h->chunk, sr_mmx_max_queries(h->N, h->n_out), ((long)1 << 28) / per}));
    const long DD = (long)h->D * h->D, nn = (long)h->n_out * h->n_out;
    SR_TRY(h->mm_ws.grow((size_t)(head + std::min(chunk, T) * per), wait::stream(s)));
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_moment_match: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_moment_match: model not factorized");
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
    const long per = sr_mm_ws_per_query(h->N, h->D, h->n_out);
    // a chunk: the handle's, what the launch grid takes, and at most 2^28 doubles (2 GB) of scratch
    const long chunk = std::max(1L, std::min({h->chunk, sr_mm_max_queries(h->N, h->n_out), ((long)1 << 28) / per}));
    const long DD = (long)h->D * h->D, nn = (long)h->n_out * h->n_out;
    SR_TRY(h->mm_ws.grow((size_t)(std::min(chunk, T) * per), wait::stream(s)));
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_moment_match_vjp: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_moment_match_vjp: model not factorized");
    if (h->general) {
        sr_set_error("sr_gp_moment_match_vjp: the reverse pass is for ARD-RBF models only (data set with sr_gp_set_data)");
        return SR_EUNSUPPORTED;
    }
    SR_CHECK(T >= 0, SR_EINVAL, "sr_gp_moment_match_vjp: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(m && inv_k && (m_bar || S_bar), SR_EINVAL, "sr_gp_moment_match_vjp: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const long per = sr_mmg_ws_per_query(h->N, h->D, h->n_out);
    const long chunk = std::max(1L, std::min({h->chunk, sr_mmg_max_queries(h->N, h->n_out), ((long)1 << 28) / per}));
    const long Dl = h->D, DD = Dl * Dl, n = h->n_out;
    SR_TRY(h->mm_ws.grow((size_t)(std::min(chunk, T) * per), wait::stream(s)));
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
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(h->factorized, SR_ESTATE, "%s: model not factorized", who);
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
    const long per = sr_mmr_ws_per_traj(h->D, h->n_out);
    const long chunk = std::max(1L, std::min({h->chunk, 0x7fffffffL, ((long)1 << 28) / per}));
    SR_TRY(h->mm_ws.grow((size_t)(std::min(chunk, T) * per), wait::stream(s)));
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
// group size decides the size of the scratch and how full the one-off pass runs, not a bit of the results.
extern "C" int sr_gp_moment_match_rollout_vjp(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj, const double* mu0,
                                              const double* sigma0, const double* k_ff, const double* k_fb, const double* a,
                                              const double* b, const double* tz, const double* inv_k, const double* mu_all,
                                              const double* sigma_all, const double* mu_all_bar, const double* sigma_all_bar,
                                              const double* cov_all_bar, double* mu0_bar, double* sigma0_bar, double* kff_bar,
                                              double* kfb_bar, void* stream) {
    const char* who = "sr_gp_moment_match_rollout_vjp";
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(h->factorized, SR_ESTATE, "%s: model not factorized", who);
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
    const long group = std::max(1L, std::min(queries / H, ((long)1 << 28) / per));
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

// doubles of reach_ws per query: z | mu, var | jac_mu, jac_var | hess_mu | mu_bar, var_bar | jac_bar, jac_s | jz
static long sr_reach_vjp_ws_per_query(int n_s, int n_u, int D) {
    return D + 4L * n_s + 3L * n_s * D + (long)n_s * D * D + 2L * n_s * (n_s + n_u);
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
    if (h->D > 8) {                                   // the widths sr_gp_linearize_batch is compiled for
        sr_set_error("%s: D=%d > 8 (the batched linearisation behind it)", who, h->D);
        return SR_EUNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const int D = h->D, n_xin = h->n_xin ? h->n_xin : n_s;
    const double* Tz = h->n_xin ? h->Tz : nullptr;
    const bool second = mode != 2 && q != nullptr;
    const long per = sr_reach_vjp_ws_per_query(n_s, n_u, D);
    // a pass: the handle's chunk, at most 2^28 doubles (2 GB) of scratch, and never wider than the batch at which both GP calls
    // still split their sums as the model size alone sets it (sr_common.h): the same bits for any chunk size
    const long chunk = std::max(1L, std::min({h->chunk, sr_stable_pass_max(h->N, h->Np, h->n_out), ((long)1 << 28) / per}));
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s, nd = (long)n_s * D, nds = (long)n_s * (n_s + n_u);
    const long Tw = std::min(chunk, T);
    SR_TRY(h->reach_ws.grow((size_t)(Tw * per), wait::stream(s)));
    double* w = h->reach_ws.get();                   // (the order of sr_reach_vjp_ws_per_query)
    double* z = w; w += Tw * D;
    double* mu = w; w += Tw * n_s;
    double* var = w; w += Tw * n_s;
    double* jm = w; w += Tw * nd;
    double* jv = w; w += Tw * nd;
    double* hm = w; w += Tw * nd * D;
    double* mu_bar = w; w += Tw * n_s;
    double* var_bar = w; w += Tw * n_s;
    double* jac_bar = w; w += Tw * nds;
    double* jac_s = w; w += Tw * nds;
    double* jz = w;
    for (long t0 = 0; t0 < T; t0 += chunk) {
        const long Tc = std::min(chunk, T - t0);
        SR_TRY(sr_launch_reach_z(Tc, n_s, n_u, n_xin, p + t0 * n_s, k_ff + t0 * n_u, Tz, z, s));
        if (second) SR_TRY(sr_gp_linearize_batch(h, z, Tc, mu, var, jm, jv, hm, stream));
        else SR_TRY(sr_gp_predict_grad(h, z, Tc, mu, var, jm, jv, stream));
        sr_momvjp_args ma{};
        sr_ellvjp_args& ea = ma.e;
        ea.T = Tc; ea.q = q ? q + t0 * nss : nullptr; ea.k_fb = k_fb ? k_fb + t0 * nus : nullptr;
        ea.var = var; ea.jac = jm;                    // (identity transform: the GP's Jacobian is the state-space one)
        ea.a = a; ea.b = b; ea.l_mu = l_mu; ea.l_sigma = l_sigma; ea.c_safety = c_safety;
        ea.p1_bar = p1_bar ? p1_bar + t0 * n_s : nullptr; ea.q1_bar = q1_bar ? q1_bar + t0 * nss : nullptr;
        ea.p_bar = p_bar + t0 * n_s; ea.q_bar = q_bar ? q_bar + t0 * nss : nullptr;
        ea.kff_bar = kff_bar + t0 * n_u; ea.kfb_bar = kfb_bar ? kfb_bar + t0 * nus : nullptr;
        ea.mu_bar = mu_bar; ea.var_bar = var_bar;
        ea.jac_bar = (second || mode == 0) ? jac_bar : nullptr;      // (the ellipsoid kernel writes its zeros from a point too)
        ea.jac_mu = jm; ea.jac_var = jv; ea.hess_mu = second ? hm : nullptr; ea.Tz = Tz; ea.D = D; ea.n_xin = n_xin;
        ea.jac_s = jac_s; ea.jz = jz;
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
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_onestep_reach_vjp: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_onestep_reach_vjp: model not factorized");
    SR_CHECK(T >= 0, SR_EINVAL, "sr_onestep_reach_vjp: T=%ld", T);
    if (T == 0) return SR_OK;
    SR_CHECK(p && k_ff && a && b && l_mu && l_sigma && p_bar && kff_bar, SR_EINVAL, "sr_onestep_reach_vjp: NULL argument");
    SR_CHECK(q == nullptr || (k_fb && q_bar && kfb_bar), SR_EINVAL, "sr_onestep_reach_vjp: k_fb, q_bar and kfb_bar required with q");
    SR_CHECK(p1_bar || q1_bar, SR_EINVAL, "sr_onestep_reach_vjp: both seeds NULL");
    return onestep_vjp_impl(h, "sr_onestep_reach_vjp", T, 0, p, q, k_ff, k_fb, a, b, l_mu, l_sigma, c_safety, p1_bar, q1_bar,
                            nullptr, p_bar, q_bar, kff_bar, kfb_bar, stream);
}

// doubles of reach_ws per (trajectory, step) pair of sr_multistep_reach_vjp: those of one step's reverse pass, and
// q_in, kfb_in | p_seed, q_seed | p_bar, q_bar, kff_bar, kfb_bar | eig
static long sr_reach_rollout_vjp_ws_per_query(int n_s, int n_u, int D) {
    return sr_reach_vjp_ws_per_query(n_s, n_u, D) + 2L * n_s + 3L * n_s * n_s + 2L * n_u * n_s + n_u + (1L + 2L * n_s + n_u);
}

// The reverse pass of sr_multistep_reach (sr_reach_rollout_vjp.hip).  Per group of max(1, chunk / H) trajectories: the inputs of all
// their steps (one launch), sr_gp_linearize_batch over them in passes bounded as onestep_vjp_impl bounds them, then the sweep, one
// thread per trajectory.  A thread owns its trajectory: the grouping decides nothing but the size of the scratch.
extern "C" int sr_multistep_reach_vjp(sr_gp_t h, long T, int H, const double* p0, const double* q0, const double* k_fb0,
                                      const double* k_ff, const double* k_fb, const double* a, const double* b,
                                      const double* l_mu, const double* l_sigma, double c_safety, const double* p_all,
                                      const double* q_all, const double* p_all_bar, const double* q_all_bar, double* p0_bar,
                                      double* q0_bar, double* kfb0_bar, double* kff_bar, double* kfb_bar, void* stream) {
    const char* who = "sr_multistep_reach_vjp";
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(h->factorized, SR_ESTATE, "%s: model not factorized", who);
    SR_CHECK(T >= 0 && H >= 1, SR_EINVAL, "%s: T=%ld H=%d", who, T, H);
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    if (h->D > 8) {                                   // the widths sr_gp_linearize_batch is compiled for
        sr_set_error("%s: D=%d > 8 (the batched linearisation behind it)", who, h->D);
        return SR_EUNSUPPORTED;
    }
    if (T == 0) return SR_OK;
    SR_CHECK(p0 && k_ff && a && b && l_mu && l_sigma && p_all && q_all && p0_bar && kff_bar, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H == 1 || (k_fb && kfb_bar), SR_EINVAL, "%s: k_fb and kfb_bar required for H > 1", who);
    SR_CHECK(q0 == nullptr || (k_fb0 && q0_bar && kfb0_bar), SR_EINVAL, "%s: k_fb0, q0_bar and kfb0_bar required with q0", who);
    SR_CHECK(p_all_bar || q_all_bar, SR_EINVAL, "%s: both seeds NULL", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const int D = h->D, n_xin = h->n_xin ? h->n_xin : n_s;
    const long per = sr_reach_rollout_vjp_ws_per_query(n_s, n_u, D);
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s, nd = (long)n_s * D, nds = (long)n_s * (n_s + n_u);
    // a group: chunk / H trajectories and at most 2^28 doubles (2 GB) of scratch; a linearisation pass: as in onestep_vjp_impl
    const long group = std::max(1L, std::min(h->chunk / H, ((long)1 << 28) / (per * H)));
    const long pass = std::max(1L, std::min(h->chunk, sr_stable_pass_max(h->N, h->Np, h->n_out)));
    const long Qw = std::min(group, T) * H;
    SR_TRY(h->reach_ws.grow((size_t)(Qw * per), wait::stream(s)));
    double* w = h->reach_ws.get();
    auto take = [&](long each) { double* x = w; w += Qw * each; return x; };
    sr_rrv_args r{};
    sr_ellvjp_args& ea = r.e;
    r.z = take(D);
    double* mu = take(n_s);
    double* var = take(n_s);
    double* jm = take(nd);
    double* jv = take(nd);
    double* hm = take(nd * D);
    ea.mu_bar = take(n_s); ea.var_bar = take(n_s); ea.jac_bar = take(nds); ea.jac_s = take(nds); ea.jz = take(nd);
    r.q_in = take(nss); r.kfb_in = take(nus); r.p_seed = take(n_s); r.q_seed = take(nss);
    ea.p_bar = take(n_s); ea.q_bar = take(nss); ea.kff_bar = take(n_u); ea.kfb_bar = take(nus);
    r.eig = take(1 + 2 * n_s + n_u);
    ea.q = r.q_in; ea.k_fb = r.kfb_in; ea.var = var; ea.jac = jm;
    ea.a = a; ea.b = b; ea.l_mu = l_mu; ea.l_sigma = l_sigma; ea.c_safety = c_safety;
    ea.p1_bar = r.p_seed; ea.q1_bar = r.q_seed;
    ea.jac_mu = jm; ea.jac_var = jv; ea.hess_mu = hm; ea.Tz = h->n_xin ? h->Tz : nullptr; ea.D = D; ea.n_xin = n_xin;
    r.H = H; r.n_s = n_s; r.n_u = n_u;
    for (long t0 = 0; t0 < T; t0 += group) {
        const long Tg = std::min(group, T - t0), Q = Tg * H;
        ea.T = Tg;
        r.p0 = p0 + t0 * n_s; r.q0 = q0 ? q0 + t0 * nss : nullptr; r.k_fb0 = q0 ? k_fb0 + t0 * nus : nullptr;
        r.k_ff = k_ff + t0 * H * n_u; r.k_fb = k_fb ? k_fb + t0 * (H - 1) * nus : nullptr;
        r.p_all = p_all + t0 * H * n_s; r.q_all = q_all + t0 * H * nss;
        r.p_all_bar = p_all_bar ? p_all_bar + t0 * H * n_s : nullptr; r.q_all_bar = q_all_bar ? q_all_bar + t0 * H * nss : nullptr;
        r.p0_bar = p0_bar + t0 * n_s; r.q0_bar = q0_bar ? q0_bar + t0 * nss : nullptr;
        r.kfb0_bar = kfb0_bar ? kfb0_bar + t0 * nus : nullptr; r.kfb_bar = kfb_bar ? kfb_bar + t0 * (H - 1) * nus : nullptr;
        r.kff_bar = kff_bar + t0 * H * n_u;
        SR_TRY(sr_launch_reach_rollout_prep(r, s));
        SR_TRY(sr_launch_reach_rollout_eig(r, s));
        for (long q1 = 0; q1 < Q; q1 += pass) {
            const long Qc = std::min(pass, Q - q1);
            SR_TRY(sr_gp_linearize_batch(h, r.z + q1 * D, Qc, mu + q1 * n_s, var + q1 * n_s, jm + q1 * nd, jv + q1 * nd,
                                         hm + q1 * nd * D, stream));
        }
        sr_prof_scope ps(&h->prof, SR_K_REACH_VJP, s);
        SR_TRY(sr_launch_reach_rollout_vjp(r, s));
    }
    return SR_OK;
}

// doubles of reach_ws per (trajectory, step) pair of sr_multistep_moments_vjp: z | mu, var | jac_mu, jac_var | hess_mu (where it is
// read) | mu_bar, var_bar | jac_bar, jac_s, jz (mode 1) | q_in, kfb_in | p_seed, q_seed | p_bar, q_bar, kff_bar, kfb_bar
static long sr_moments_rollout_vjp_ws_per_query(int n_s, int n_u, int D, int mode, bool second) {
    return D + 4L * n_s + 2L * n_s * D + (second ? (long)n_s * D * D : 0) + (mode == 1 ? 2L * n_s * (n_s + n_u) + (long)n_s * D : 0) +
           2L * n_s + 3L * n_s * n_s + 2L * n_u * n_s + n_u;
}

// The reverse pass of sr_multistep_moments, and of H rounds of sr_onestep_moments from N(mu0, sigma0) (sr_moments_rollout_vjp.hip).
// Per group of max(1, chunk / H) trajectories: the inputs of all their steps (the launch of sr_multistep_reach_vjp), the GP derivatives
// at them in passes bounded as onestep_vjp_impl bounds them -- sr_gp_linearize_batch in mode 1, where a step from a Gaussian reads
// the Hessian of the mean, sr_gp_predict_grad in mode 2 and for one step from a point --, then the sweep, one thread per trajectory.
// A thread owns its trajectory: the grouping decides nothing but the size of the scratch.
extern "C" int sr_multistep_moments_vjp(sr_gp_t h, long T, int H, int mode, const double* mu0, const double* sigma0,
                                        const double* k_ff, const double* k_fb, const double* a, const double* b,
                                        const double* mu_all, const double* sigma_all, const double* mu_all_bar,
                                        const double* sigma_all_bar, const double* gpvar_all_bar, double* mu0_bar,
                                        double* sigma0_bar, double* kff_bar, double* kfb_bar, void* stream) {
    const char* who = "sr_multistep_moments_vjp";
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(h->factorized, SR_ESTATE, "%s: model not factorized", who);
    SR_CHECK(T >= 0 && H >= 1 && (mode == 1 || mode == 2), SR_EINVAL, "%s: T=%ld H=%d mode=%d", who, T, H, mode);
    int n_s, n_u;
    SR_TRY(check_reach_dims(h, &n_s, &n_u));
    if (h->D > 8) {                                   // the widths sr_gp_linearize_batch is compiled for
        sr_set_error("%s: D=%d > 8 (the batched linearisation behind it)", who, h->D);
        return SR_EUNSUPPORTED;
    }
    if (T == 0) return SR_OK;
    SR_CHECK(mu0 && k_ff && a && b && mu_all && sigma_all && mu0_bar && kff_bar, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H == 1 || (k_fb && kfb_bar), SR_EINVAL, "%s: k_fb and kfb_bar required for H > 1", who);
    SR_CHECK(sigma0 == nullptr || sigma0_bar != nullptr, SR_EINVAL, "%s: sigma0 without sigma0_bar", who);
    SR_CHECK(mu_all_bar || sigma_all_bar || gpvar_all_bar, SR_EINVAL, "%s: every seed NULL", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const int D = h->D, n_xin = h->n_xin ? h->n_xin : n_s;
    const bool second = mode == 1 && (H > 1 || sigma0 != nullptr);
    const long per = sr_moments_rollout_vjp_ws_per_query(n_s, n_u, D, mode, second);
    const long nss = (long)n_s * n_s, nus = (long)n_u * n_s, nd = (long)n_s * D, nds = (long)n_s * (n_s + n_u);
    // a group: chunk / H trajectories and at most 2^28 doubles (2 GB) of scratch; a pass of GP derivatives: as in onestep_vjp_impl
    const long group = std::max(1L, std::min(h->chunk / H, ((long)1 << 28) / (per * H)));
    const long pass = std::max(1L, std::min(h->chunk, sr_stable_pass_max(h->N, h->Np, h->n_out)));
    const long Qw = std::min(group, T) * H;
    SR_TRY(h->reach_ws.grow((size_t)(Qw * per), wait::stream(s)));
    double* w = h->reach_ws.get();
    auto take = [&](long each) { double* x = w; w += Qw * each; return x; };
    sr_mrv_args m{};
    sr_rrv_args& r = m.r;
    sr_ellvjp_args& ea = r.e;
    r.z = take(D);
    double* mu = take(n_s);
    double* var = take(n_s);
    double* jm = take(nd);
    double* jv = take(nd);
    double* hm = second ? take(nd * D) : nullptr;
    ea.mu_bar = take(n_s); ea.var_bar = take(n_s);
    if (mode == 1) { ea.jac_bar = take(nds); ea.jac_s = take(nds); ea.jz = take(nd); }
    r.q_in = take(nss); r.kfb_in = take(nus); r.p_seed = take(n_s); r.q_seed = take(nss);
    ea.p_bar = take(n_s); ea.q_bar = take(nss); ea.kff_bar = take(n_u); ea.kfb_bar = take(nus);
    ea.q = r.q_in; ea.k_fb = r.kfb_in; ea.var = var; ea.jac = jm;
    ea.a = a; ea.b = b; ea.c_safety = 1.0;
    ea.p1_bar = r.p_seed; ea.q1_bar = r.q_seed;
    ea.jac_mu = jm; ea.jac_var = jv; ea.hess_mu = hm; ea.Tz = h->n_xin ? h->Tz : nullptr; ea.D = D; ea.n_xin = n_xin;
    r.H = H; r.n_s = n_s; r.n_u = n_u;
    m.mode = mode;
    for (long t0 = 0; t0 < T; t0 += group) {
        const long Tg = std::min(group, T - t0), Q = Tg * H;
        ea.T = Tg;
        r.p0 = mu0 + t0 * n_s; r.q0 = sigma0 ? sigma0 + t0 * nss : nullptr;
        r.k_ff = k_ff + t0 * H * n_u; r.k_fb = k_fb ? k_fb + t0 * (H - 1) * nus : nullptr;
        r.p_all = mu_all + t0 * H * n_s; r.q_all = sigma_all + t0 * H * nss;
        r.p_all_bar = mu_all_bar ? mu_all_bar + t0 * H * n_s : nullptr;
        r.q_all_bar = sigma_all_bar ? sigma_all_bar + t0 * H * nss : nullptr;
        m.gpvar_all_bar = gpvar_all_bar ? gpvar_all_bar + t0 * H * n_s : nullptr;
        r.p0_bar = mu0_bar + t0 * n_s; r.q0_bar = sigma0 ? sigma0_bar + t0 * nss : nullptr;
        r.kff_bar = kff_bar + t0 * H * n_u; r.kfb_bar = H > 1 ? kfb_bar + t0 * (H - 1) * nus : nullptr;
        SR_TRY(sr_launch_reach_rollout_prep(r, s));
        for (long q1 = 0; q1 < Q; q1 += pass) {
            const long Qc = std::min(pass, Q - q1);
            if (second)
                SR_TRY(sr_gp_linearize_batch(h, r.z + q1 * D, Qc, mu + q1 * n_s, var + q1 * n_s, jm + q1 * nd, jv + q1 * nd,
                                             hm + q1 * nd * D, stream));
            else
                SR_TRY(sr_gp_predict_grad(h, r.z + q1 * D, Qc, mu + q1 * n_s, var + q1 * n_s, jm + q1 * nd, jv + q1 * nd, stream));
        }
        sr_prof_scope ps(&h->prof, SR_K_REACH_VJP, s);
        SR_TRY(sr_launch_moments_rollout_vjp(m, s));
    }
    return SR_OK;
}

extern "C" int sr_onestep_moments_vjp(sr_gp_t h, long T, int mode, const double* mu_x, const double* sigma_x, const double* k_ff,
                                      const double* k_fb, const double* a, const double* b, const double* mu1_bar,
                                      const double* sigma1_bar, const double* gpvar_bar, double* mux_bar, double* sigma_bar,
                                      double* kff_bar, double* kfb_bar, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_onestep_moments_vjp: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_onestep_moments_vjp: model not factorized");
    SR_CHECK(T >= 0 && (mode == 1 || mode == 2), SR_EINVAL, "sr_onestep_moments_vjp: T=%ld mode=%d", T, mode);
    if (T == 0) return SR_OK;
    SR_CHECK(mu_x && k_ff && a && b && mux_bar && kff_bar, SR_EINVAL, "sr_onestep_moments_vjp: NULL argument");
    SR_CHECK(sigma_x == nullptr || (k_fb && sigma_bar && kfb_bar), SR_EINVAL,
             "sr_onestep_moments_vjp: k_fb, sigma_bar and kfb_bar required with sigma_x");
    SR_CHECK(mu1_bar || sigma1_bar || gpvar_bar, SR_EINVAL, "sr_onestep_moments_vjp: every seed NULL");
    return onestep_vjp_impl(h, "sr_onestep_moments_vjp", T, mode, mu_x, sigma_x, k_ff, k_fb, a, b, nullptr, nullptr, 1.0,
                            mu1_bar, sigma1_bar, gpvar_bar, mux_bar, sigma_bar, kff_bar, kfb_bar, stream);
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

extern "C" int sr_gp_set_chain(sr_gp_t h, int on) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_set_chain: NULL handle");
    h->chain = on != 0;
    return SR_OK;
}

extern "C" int sr_gp_last_chain(sr_gp_t h) { return h ? h->last_chain : 0; }

extern "C" int sr_gp_chain_status(sr_gp_t h, int* timed_out) {
    SR_CHECK(h != nullptr && timed_out != nullptr, SR_EINVAL, "sr_gp_chain_status: NULL argument");
    *timed_out = 0;
    if (h->chain_status_host && *(volatile int*)h->chain_status_host != 0) {
        *timed_out = 1;
        *(volatile int*)h->chain_status_host = 0;
        h->chain = 0;                        // per-step launches from here on (sr_gp_set_chain re-arms)
    }
    return SR_OK;
}

// tests (host only): the two split rules of sr_common.h and the pass bound the reverse driver takes from them
extern "C" int sr_test_split_plan(int N, int Np, int n_out, long Tp, int* out) {
    SR_CHECK(N >= 1 && Np >= N && Np % SR_NB == 0 && n_out >= 1 && Tp >= 1 && out, SR_EINVAL, "sr_test_split_plan: bad argument");
    out[0] = sr_kstar_nsplit(Np, n_out, Tp);
    out[1] = sr_hess_nsplit(N, n_out, Tp);
    out[2] = (int)sr_stable_pass_max(N, Np, n_out);
    out[3] = SR_FINAL_WAVE_T;
    return SR_OK;
}

// tests: the next persistent multi-step launches are short of `drop` workgroups, i.e. the last group waits for partners
// that never come -- the deterministic way to reach the time-out path (a CU mask of one or two bits does not do it: the
// driver widens such masks, the chain completed on "1 CU")
extern "C" int sr_test_chain_drop(sr_gp_t h, int drop) {
    SR_CHECK(h != nullptr && drop >= 0, SR_EINVAL, "sr_test_chain_drop: bad argument");
    h->chain_test_drop = drop;
    if (drop == 0 && h->chain_tickets) {
        // a launch that was short of a workgroup leaves its group's counters in a state no real launch can produce
        // (in the field every workgroup runs, however late, and the last one to leave resynchronises the group)
        SR_DEVICE(h->device);
        SR_HIP(device_sync());
        SR_TRY(dev_zero(h->chain_xch, sizeof(sr_xel) * (size_t)SR_CHAIN_XELS));
        SR_TRY(dev_zero(h->chain_tickets, sizeof(unsigned long long) * 2 * SR_CHAIN_GROUPS));
        SR_TRY(dev_zero(h->chain_done, sizeof(unsigned) * SR_CHAIN_GROUPS));
    }
    return SR_OK;
}

