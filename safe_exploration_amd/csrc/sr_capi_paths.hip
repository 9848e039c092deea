// sr_capi_paths.hip -- posterior function samples by pathwise conditioning: sr_gp_paths_draw / _count / _eval / _step and
// their Jacobians sr_gp_paths_eval_grad / _step_grad (the same plans with J: one body each), and the closed-loop roll-out in one
// launch, sr_gp_paths_rollout, with its reverse pass sr_gp_paths_rollout_vjp.  The algebra: include/safereach.h; the kernels:
// sr_paths.hip, sr_paths_rollout.hip, sr_paths_rollout_vjp.hip; for a general-family handle with the RBF radial part the
// feature slab, dK* and the step of sr_paths_gen.hip in their places (draw, _eval, _step and their Jacobians; the roll-out in
// one launch is refused), with G M + D weights per path instead of M (sr_gp_paths_weight_count).
// Host-side orchestration only.
#include "sr_handle.h"
using namespace srh;

namespace {

// the feature map of a general-family handle (after model_checks: the groups are read, D <= SR_PATHS_MAX_D)
sr_paths_gen gen_args(const sr_gp* h, int M) {
    sr_paths_gen g;
    g.kp = h->kp; g.G = 0;
    for (int l = 0; l <= h->D; ++l)
        if (h->gen_groups >> l & 1u) g.grp[g.G++] = l;
    for (int q = g.G; q <= SR_PATHS_MAX_D; ++q) g.grp[q] = -1;
    g.n_w = g.G * M + h->D;
    return g;
}
// weights per path and output: the M features of the ARD-RBF kernel, G M + D for the general family
int weight_count(const sr_gp* h, int M) { return h->general ? gen_args(h, M).n_w : M; }

// the handle's block of drawn paths: [omega M x D | tau M | w n_out x Mp x Sp | c n_out x Np x Sp], every part 16-byte aligned
// (Mp: the weights per path, to 16)
struct paths_layout {
    int S, M, Sp, Mp; size_t o_tau, o_w, o_c, total;
    paths_layout(const sr_gp* h, int S_, int M_) : S(S_), M(M_) {
        Sp = (int)round_up(S, srt::BN); Mp = (int)round_up(weight_count(h, M), srt::BK);
        o_tau = (size_t)round_up((long)M * h->D, 2);
        o_w = o_tau + (size_t)round_up(M, 2);
        o_c = o_w + (size_t)h->n_out * Mp * Sp;
        total = o_c + (size_t)h->n_out * h->Np * Sp;
    }
};

bool paths_valid(const sr_gp* h) { return h->paths_S > 0 && h->paths_gen == h->model_gen && h->paths_Np == h->Np && h->paths.get(); }

sr_paths_feat feat_args(const sr_gp* h, const paths_layout& L) {
    sr_paths_feat m;
    m.ls = h->ls; m.sf2 = h->sf2; m.omega = h->paths.get(); m.tau = h->paths.get() + L.o_tau;
    m.D = h->D; m.n_out = h->n_out; m.M = L.M; m.Mp = L.Mp;
    return m;
}

// the feature slab (jg >= 0: its derivative in input dimension jg) by the handle's kernel
int launch_features(const sr_gp* h, const paths_layout& L, const double* X, long T, long col0, long ncols, double* Phi,
                    hipStream_t s, int jg = -1) {
    const sr_paths_feat fm = feat_args(h, L);
    if (h->general) return sr_launch_paths_gen_features(fm, gen_args(h, L.M), X, h->D, T, col0, ncols, Phi, s, jg);
    return sr_launch_paths_features(fm, X, h->D, T, col0, ncols, Phi, s, jg);
}

// what all calls ask of the model (after their own arguments, before the question whether paths exist).  A general-family
// handle: its packed parameters are read back once per data set (behind `s`); fused: the roll-out in one launch, which the
// family does not have.
int model_checks(sr_gp* h, const char* who, hipStream_t s, bool fused = false) {
    SR_CHECK(h->factorized && !h->import_open, SR_ESTATE, "%s: model not factorized%s", who,
             h->import_open ? " (between sr_gp_import_begin and sr_gp_import_end)" : "");
    SR_CHECK(!h->sparse, SR_ESTATE, "%s: sparse model (U^-1 is not the factor of K_y)", who);
    SR_CHECK(!(h->general && fused), SR_EUNSUPPORTED,
             "%s: general kernel family (the roll-out in one launch is that of the ARD-RBF kernel: chain sr_gp_paths_step)", who);
    SR_CHECK(h->D <= SR_PATHS_MAX_D, SR_EUNSUPPORTED, "%s: D=%d > %d", who, h->D, SR_PATHS_MAX_D);
    if (!h->general) return SR_OK;
    SR_DEVICE(h->device);
    SR_TRY(general_info(h, s));
    SR_CHECK(h->gen_rbf, SR_EUNSUPPORTED,
             "%s: general kernel family with a Matern output (the feature map is the Gaussian spectral density)", who);
    return SR_OK;
}
// ... and the draw of its parameters: each sits under a square root (and its slab has one more strip along grid.y)
int sign_check(const sr_gp* h, const char* who, int M) {
    if (!h->general) return SR_OK;
    SR_CHECK(!h->gen_negative[0], SR_EINVAL, "%s: negative kernel parameter (%s)", who, h->gen_negative);
    SR_CHECK(M <= 65534 * SR_PATHS_FROWS, SR_EINVAL, "%s: M=%d outside 1..%d (general family)", who, M, 65534 * SR_PATHS_FROWS);
    return SR_OK;
}

}  // namespace

extern "C" int sr_gp_paths_count(sr_gp_t h, int* S, int* M) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_paths_count: NULL handle");
    const bool ok = paths_valid(h);
    if (S) *S = ok ? h->paths_S : 0;
    if (M) *M = ok ? h->paths_M : 0;
    return SR_OK;
}

// the refusals of the draw in its order (M, the model, the signs); the one-off readback of a general handle's parameters waits
// for the device, as this call has no stream
extern "C" int sr_gp_paths_weight_count(sr_gp_t h, int M, int* n_w) {
    const char* who = "sr_gp_paths_weight_count";
    SR_CHECK(h != nullptr && n_w != nullptr, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(M >= 1 && M <= 65535 * SR_PATHS_FROWS, SR_EINVAL, "%s: M=%d outside 1..%d", who, M, 65535 * SR_PATHS_FROWS);
    if (h->general && h->gen_rbf < 0 && h->factorized && !h->import_open && !h->sparse && h->D <= SR_PATHS_MAX_D) {
        SR_DEVICE(h->device);
        SR_HIP(device_sync());
    }
    SR_TRY(model_checks(h, who, nullptr));
    SR_TRY(sign_check(h, who, M));
    *n_w = weight_count(h, M);
    return SR_OK;
}

extern "C" int sr_gp_paths_draw(sr_gp_t h, int S, int M, const double* omega, const double* tau, const double* w,
                                const double* eps, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_paths_draw: NULL handle");
    SR_CHECK(S >= 0, SR_EINVAL, "sr_gp_paths_draw: S=%d", S);
    if (S == 0) {                                        // drop the paths
        SR_DEVICE(h->device);
        h->paths_S = h->paths_M = 0;
        // the block goes back to the block cache: an _eval or _step still in flight on any stream must have finished with it
        if (h->paths.get()) SR_HIP(device_sync());
        h->paths.drop();
        return SR_OK;
    }
    // (the feature slab takes 16 features per workgroup along grid.y)
    SR_CHECK(M >= 1 && M <= 65535 * SR_PATHS_FROWS, SR_EINVAL, "sr_gp_paths_draw: M=%d outside 1..%d", M, 65535 * SR_PATHS_FROWS);
    SR_CHECK(omega && tau && w && eps, SR_EINVAL, "sr_gp_paths_draw: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    SR_TRY(model_checks(h, "sr_gp_paths_draw", s));
    SR_TRY(sign_check(h, "sr_gp_paths_draw", M));
    SR_DEVICE(h->device);
    SR_TRY(tile_route_alignment(h));                     // (the two triangular products read U^-1 in 16-byte pieces)
    const int N = h->N, Np = h->Np, off = Np - N, n_out = h->n_out;
    const paths_layout L(h, S, M);
    // workspace first: if it cannot be had, the paths drawn earlier stay
    const size_t n_phi = (size_t)n_out * L.Mp * Np, n_rs = (size_t)n_out * Np * L.Sp;
    SR_TRY(h->paths_ws.grow(n_phi + 2 * n_rs, wait::device()));
    h->paths_S = h->paths_M = 0;                         // from here on the old paths are gone
    SR_TRY(h->paths.grow(L.total, wait::device()));
    double *P = h->paths.get(), *Wk = P + L.o_w, *C = P + L.o_c;
    double *Phi = h->paths_ws.get(), *R = Phi + n_phi, *V = R + n_rs;
    sr_prof_scope ps(&h->prof, SR_K_PATHS_DRAW, s);
    SR_HIP(hipMemcpyAsync(P, omega, sizeof(double) * M * h->D, hipMemcpyDeviceToDevice, s));
    SR_HIP(hipMemcpyAsync(P + L.o_tau, tau, sizeof(double) * M, hipMemcpyDeviceToDevice, s));
    SR_TRY(sr_launch_paths_pack(w, Wk, nullptr, nullptr, weight_count(h, M), 0, L.Mp, S, L.Sp, n_out, s));
    SR_TRY(launch_features(h, L, h->Z, N, off, Np, Phi, s));
    // the prior at the training rows, P = Phi(Z)^T w (Np x Sp per output), then R = y - P - sqrt(n_d) eps^T in its place
    sr_batch bp; bp.n = n_out; bp.sA = (long)L.Mp * Np; bp.sB = (long)L.Mp * L.Sp; bp.sC = (long)Np * L.Sp;
    SR_TRY(sr_launch_gemm_tn(Phi, Np, Wk, L.Sp, R, L.Sp, Np, L.Sp, L.Mp, 1.0, 0.0, 0, s, 0, &bp));
    SR_TRY(sr_launch_paths_pack(eps, R, h->yT, h->noise, N, off, Np, S, L.Sp, n_out, s));
    // V = U^-T R: U^-1 is upper triangular, the k range of a row block of V ends with the block (mode 3); C = U^-1 V
    sr_batch bv; bv.n = n_out; bv.sA = (long)Np * Np; bv.sB = (long)Np * L.Sp; bv.sC = (long)Np * L.Sp;
    SR_TRY(sr_launch_gemm_tn(h->Wt, Np, R, L.Sp, V, L.Sp, Np, L.Sp, Np, 1.0, 0.0, 3, s, 0, &bv));
    SR_TRY(sr_launch_paths_solve(h->Wt, V, C, N, Np, L.Sp, n_out, s));
    h->paths_S = S; h->paths_M = M; h->paths_Np = Np; h->paths_gen = h->model_gen;
    return SR_OK;
}

namespace {

// _eval (grad == false: F required, J unused) and _eval_grad (J required, F optional).  Per chunk: K*, the feature slab and the
// two-range tile for F; then per input dimension j the derivative slabs of both ranges (behind the feature slab in paths_ws:
// one more feature-sized and one K*-sized slab, reused by every j) and the same tile into column j of J.
int paths_eval(sr_gp_t h, const double* Xq, long T, double* F, double* J, bool grad, void* stream, const char* who) {
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(T >= 0, SR_EINVAL, "%s: T=%ld", who, T);
    SR_CHECK(grad ? J != nullptr : true, SR_EINVAL, "%s: NULL J", who);
    SR_CHECK(T == 0 || (Xq && (F || grad)), SR_EINVAL, "%s: NULL argument", who);
    hipStream_t s = (hipStream_t)stream;
    SR_TRY(model_checks(h, who, s));
    SR_CHECK(paths_valid(h), SR_ESTATE, "%s: no valid paths (sr_gp_paths_draw after the last model update)", who);
    if (T == 0) return SR_OK;
    SR_DEVICE(h->device);
    const paths_layout L(h, h->paths_S, h->paths_M);
    const double *P = h->paths.get(), *Wk = P + L.o_w, *C = P + L.o_c;
    for (long t0 = 0; t0 < T; t0 += h->chunk) {
        const long Tc = std::min(h->chunk, T - t0);
        const long Tp = round_up(Tc, srt::BN);
        const int nsplit = pick_nsplit(h, Tp);
        SR_TRY(ensure_ws(h, Tp, nsplit));
        const size_t n_phi = (size_t)h->n_out * L.Mp * Tp, n_ks = (size_t)h->n_out * h->Np * Tp;
        SR_TRY(h->paths_ws.grow(grad ? 2 * n_phi + n_ks : n_phi, wait::device()));
        const double* Xc = Xq + t0 * h->D;
        sr_kstar_args ka = kstar_ws(h, nsplit, Tc, Tp);
        ka.xa = Xc; ka.lda = h->D; ka.na = h->D;
        {
            sr_prof_scope ps(&h->prof, SR_K_KSTAR, s);
            SR_TRY(sr_launch_kstar(ka, s));
        }
        sr_prof_scope ps(&h->prof, SR_K_PATHS_EVAL, s);
        if (F) {
            SR_TRY(launch_features(h, L, Xc, Tc, 0, Tp, h->paths_ws.get(), s));
            SR_TRY(sr_launch_paths_eval(h->paths_ws.get(), Wk, h->Ks, C, F + t0 * L.S * h->n_out, h->N, h->Np, L.Mp, Tc, Tp, L.S,
                                        L.Sp, h->n_out, s));
        }
        if (!grad) continue;
        double *dPhi = h->paths_ws.get() + n_phi, *dKs = dPhi + n_phi;
        for (int j = 0; j < h->D; ++j) {
            SR_TRY(launch_features(h, L, Xc, Tc, 0, Tp, dPhi, s, j));
            if (h->general)                              // (from Z, X and kp: not K* times a factor)
                SR_TRY(sr_launch_paths_gen_dkstar(dKs, h->Z, Xc, h->kp, h->N, h->Np, h->D, h->n_out, Tc, Tp, j, s));
            else
                SR_TRY(sr_launch_paths_dkstar(h->Ks, dKs, h->Z, Xc, h->ls, h->N, h->Np, h->D, h->n_out, Tc, Tp, j, s));
            SR_TRY(sr_launch_paths_eval(dPhi, Wk, dKs, C, J + t0 * L.S * h->n_out * h->D + j, h->N, h->Np, L.Mp, Tc, Tp, L.S, L.Sp,
                                        h->n_out, s, h->n_out * h->D, h->D));
        }
    }
    return SR_OK;
}

}  // namespace

extern "C" int sr_gp_paths_eval(sr_gp_t h, const double* Xq, long T, double* F, void* stream) {
    return paths_eval(h, Xq, T, F, nullptr, false, stream, "sr_gp_paths_eval");
}

extern "C" int sr_gp_paths_eval_grad(sr_gp_t h, const double* Xq, long T, double* F, double* J, void* stream) {
    return paths_eval(h, Xq, T, F, J, true, stream, "sr_gp_paths_eval_grad");
}

namespace {

// _step (grad == false) and _step_grad (J required): the same split count, 1 + D rows of partial sums per split with J
int paths_step(sr_gp_t h, const double* Xs, double* F, double* J, bool grad, const double* k_fb, const double* k_ff,
               double* z_next, void* stream, const char* who) {
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(Xs && F && (J || !grad), SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK((k_fb != nullptr) == (k_ff != nullptr) && (z_next != nullptr) == (k_fb != nullptr), SR_EINVAL,
             "%s: k_fb, k_ff and z_next come together", who);
    SR_CHECK(!k_fb || h->D > h->n_out, SR_EINVAL, "%s: the closed loop needs D = n_out + n_u (D=%d, n_out=%d)", who, h->D,
             h->n_out);
    hipStream_t s = (hipStream_t)stream;
    SR_TRY(model_checks(h, who, s));
    SR_CHECK(paths_valid(h), SR_ESTATE, "%s: no valid paths (sr_gp_paths_draw after the last model update)", who);
    SR_DEVICE(h->device);
    const paths_layout L(h, h->paths_S, h->paths_M);
    sr_paths_step_args a;
    a.m = feat_args(h, L);
    a.Z = h->Z; a.Wk = h->paths.get() + L.o_w; a.C = h->paths.get() + L.o_c; a.Xs = Xs;
    a.F = F; a.J = grad ? J : nullptr; a.k_fb = k_fb; a.k_ff = k_ff; a.z_next = z_next; a.n_u = k_fb ? h->D - h->n_out : 0;
    a.N = h->N; a.Np = h->Np; a.S = L.S; a.Sp = L.Sp;
    a.nsplit = sr_hess_nsplit(h->N + L.M, h->n_out, L.S);     // (the split rule of the Hessian pass over the N + M terms)
    SR_TRY(h->paths_ws.grow((size_t)a.nsplit * h->n_out * (grad ? 1 + h->D : 1) * L.Sp, wait::device()));
    a.part = h->paths_ws.get();
    sr_prof_scope ps(&h->prof, SR_K_PATHS_STEP, s);
    return h->general ? sr_launch_paths_gen_step(a, gen_args(h, L.M), s) : sr_launch_paths_step(a, s);
}

}  // namespace

extern "C" int sr_gp_paths_step(sr_gp_t h, const double* Xs, double* F, const double* k_fb, const double* k_ff,
                                double* z_next, void* stream) {
    return paths_step(h, Xs, F, nullptr, false, k_fb, k_ff, z_next, stream, "sr_gp_paths_step");
}

extern "C" int sr_gp_paths_step_grad(sr_gp_t h, const double* Xs, double* F, double* J, const double* k_fb, const double* k_ff,
                                     double* z_next, void* stream) {
    return paths_step(h, Xs, F, J, true, k_fb, k_ff, z_next, stream, "sr_gp_paths_step_grad");
}

// the checks in the order of paths_step; no workspace: the launch reads the handle's paths and writes the caller's buffers
extern "C" int sr_gp_paths_rollout(sr_gp_t h, const double* x0, int x0_per_path, int H, const double* k_fb, const double* k_ff,
                                   double* X_all, double* A_all, void* stream) {
    const char* who = "sr_gp_paths_rollout";
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(x0 && k_fb && k_ff && X_all, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H >= 1 && (x0_per_path == 0 || x0_per_path == 1), SR_EINVAL, "%s: H=%d x0_per_path=%d", who, H, x0_per_path);
    SR_CHECK(h->D > h->n_out, SR_EINVAL, "%s: the closed loop needs D = n_out + n_u (D=%d, n_out=%d)", who, h->D, h->n_out);
    SR_TRY(model_checks(h, who, (hipStream_t)stream, true));
    SR_CHECK(paths_valid(h), SR_ESTATE, "%s: no valid paths (sr_gp_paths_draw after the last model update)", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const paths_layout L(h, h->paths_S, h->paths_M);
    sr_paths_rollout_args a;
    a.m = feat_args(h, L);
    a.Z = h->Z; a.Wk = h->paths.get() + L.o_w; a.C = h->paths.get() + L.o_c;
    a.x0 = x0; a.x0_per_path = x0_per_path; a.H = H; a.k_fb = k_fb; a.k_ff = k_ff; a.X_all = X_all; a.A_all = A_all;
    a.N = h->N; a.Np = h->Np; a.S = L.S; a.Sp = L.Sp;
    sr_prof_scope ps(&h->prof, SR_K_PATHS_STEP, s);
    return sr_launch_paths_rollout(a, s);
}

// the forward's checks in the forward's order; then the workspace (before it is there nothing of the handle has changed)
extern "C" int sr_gp_paths_rollout_vjp(sr_gp_t h, const double* x0, int x0_per_path, int H, const double* k_fb, const double* k_ff,
                                       const double* X_all, const double* X_bar, double* x0_bar, double* k_fb_bar, double* k_ff_bar,
                                       double* J_all, void* stream) {
    const char* who = "sr_gp_paths_rollout_vjp";
    SR_CHECK(h != nullptr, SR_EINVAL, "%s: NULL handle", who);
    SR_CHECK(x0 && k_fb && k_ff && X_all && X_bar && x0_bar && k_fb_bar && k_ff_bar, SR_EINVAL, "%s: NULL argument", who);
    SR_CHECK(H >= 1 && (x0_per_path == 0 || x0_per_path == 1), SR_EINVAL, "%s: H=%d x0_per_path=%d", who, H, x0_per_path);
    SR_CHECK(h->D > h->n_out, SR_EINVAL, "%s: the closed loop needs D = n_out + n_u (D=%d, n_out=%d)", who, h->D, h->n_out);
    SR_TRY(model_checks(h, who, (hipStream_t)stream, true));
    SR_CHECK(paths_valid(h), SR_ESTATE, "%s: no valid paths (sr_gp_paths_draw after the last model update)", who);
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    const paths_layout L(h, h->paths_S, h->paths_M);
    const int n_s = h->n_out, D = h->D, n_u = D - n_s;
    sr_paths_rollout_vjp_args a;
    a.m = feat_args(h, L);
    a.Z = h->Z; a.Wk = h->paths.get() + L.o_w; a.C = h->paths.get() + L.o_c;
    a.x0 = x0; a.x0_per_path = x0_per_path; a.H = H; a.k_fb = k_fb; a.k_ff = k_ff; a.X_all = X_all; a.X_bar = X_bar;
    a.x0_bar = x0_bar; a.k_fb_bar = k_fb_bar; a.k_ff_bar = k_ff_bar;
    a.N = h->N; a.Np = h->Np; a.S = L.S; a.Sp = L.Sp;
    a.nsplit = sr_hess_nsplit(h->N + L.M, n_s, (long)H * L.S);     // (the rule of _step, for all H S evaluations at once)
    // [J, path index fastest, unless the caller takes it | the splits' partial sums | the sweep's records]
    const size_t n_j = J_all ? 0 : (size_t)H * n_s * D * L.Sp, n_part = (size_t)a.nsplit * n_s * D * H * L.Sp;
    const size_t n_rec = (size_t)sr_paths_rollout_vjp_blocks(L.S) * ((size_t)H * n_u * (1 + n_s) + n_s);
    SR_TRY(h->paths_ws.grow(n_j + n_part + n_rec, wait::device()));
    if (J_all) { a.J = J_all; a.j_si = (long)L.S * n_s * D; a.j_ss = (long)n_s * D; a.j_se = 1; }
    else { a.J = h->paths_ws.get(); a.j_si = (long)n_s * D * L.Sp; a.j_ss = 1; a.j_se = L.Sp; }
    a.part = h->paths_ws.get() + n_j; a.rec = a.part + n_part;
    sr_prof_scope ps(&h->prof, SR_K_PATHS_STEP, s);
    return sr_launch_paths_rollout_vjp(a, s);
}
