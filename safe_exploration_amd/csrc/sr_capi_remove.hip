// sr_capi_remove.hip -- sr_gp_remove: retire training points without refactorising; sr_gp_loo: leave-one-out posterior.
// The algebra and the kernels: sr_remove.hip.
#include "sr_handle.h"
using namespace srh;

// ONE point, index j of the current rows (the caller has grown rm_ws).  The new factor, yT and alpha are written into the
// spare buffers of the small appends where the padded size stays (they ping-pong with the model's: nothing big is
// allocated), into fresh allocations with the new stride where it shrinks.  The model may be the slid view of the in-place
// appends: it is read as it lies, the result is a plain model, and the allocations the views lived in become the spare
// buffers (sr_remove_clean_kernel).  Nothing of the model is written before the last launch has been accepted; the commit
// follows the stream synchronisation.
static int remove_one(sr_gp* h, int j, hipStream_t s) {
    const int N0 = h->N, Np0 = h->Np, off0 = Np0 - N0, D = h->D, n_out = h->n_out, q = j + off0;
    const int N1 = N0 - 1, Np1 = (int)round_up(N1, SR_NB), off1 = Np1 - N1;
    const size_t NN0 = (size_t)Np0 * Np0, NN1 = (size_t)Np1 * Np1;
    const size_t o_z = (size_t)n_out * sr_remove_coef_stride(Np0);
    SR_TRY(h->rm_ws.grow(o_z + (size_t)N0 * D, wait::device()));
    double *coef = h->rm_ws.get(), *zstash = coef + o_z;
    const bool same = Np1 == Np0;
    const bool reuse_alt = same && h->Wt_alt && h->wt_alt_cap >= (size_t)n_out * NN1;
    const bool vec_alt = same && h->yT_alt && h->alpha_alt && h->vec_alt_np == Np1;
    double *yT1 = nullptr, *alpha1 = nullptr, *Wt1 = nullptr;
    int rc = SR_OK;
    auto drop_new = [&]() {
        if (!vec_alt) { dev_free(yT1); dev_free(alpha1); }
        if (!reuse_alt) dev_free(Wt1);
        else h->wt_alt_off = -1;       // the spare factor buffer may hold a half-written state now
    };
#define SR_A(expr) do { rc = (expr); if (rc != SR_OK) { drop_new(); return rc; } } while (0)
#define SR_AH(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        sr_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); drop_new(); return SR_EHIP; } } while (0)
    if (vec_alt) { yT1 = h->yT_alt; alpha1 = h->alpha_alt; }
    else {
        SR_A(dev_alloc(&yT1, vec_doubles(n_out, Np1)));
        SR_A(dev_alloc(&alpha1, vec_doubles(n_out, Np1)));
        SR_AH(hipMemsetAsync(yT1 + (size_t)n_out * Np1, 0, sizeof(double) * SR_SLIDE_STEPS, s));         // (the slack: sr_gp::slide)
        SR_AH(hipMemsetAsync(alpha1 + (size_t)n_out * Np1, 0, sizeof(double) * SR_SLIDE_STEPS, s));
    }
    if (reuse_alt) {
        // the rows kernel writes the whole upper triangle from padded row off0 on (row off0: the identity row the removal
        // leaves); a spare buffer that held a factor of this model with at least off0 padding rows has the rest in place
        if (h->wt_alt_off < off0) {
            SR_AH(hipMemsetAsync(h->Wt_alt, 0, (size_t)n_out * NN1 * sizeof(double), s));
            SR_A(sr_launch_eye_front(h->Wt_alt, Np1, off1, s, n_out));
        }
        Wt1 = h->Wt_alt;
    } else {
        SR_A(dev_alloc(&Wt1, wt_doubles(n_out, Np1)));
        SR_AH(hipMemsetAsync(Wt1, 0, sizeof(double) * wt_doubles(n_out, Np1), s));                       // (lower triangle, slack)
        SR_A(sr_launch_eye_front(Wt1, Np1, off1, s, n_out));
    }
    const long zcount = (long)(N1 - j) * D, zfrom = (long)(j + 1) * D;
    SR_A(sr_launch_remove_rownorm(h->Wt, Np0, q, n_out, coef, h->Z, zstash, zcount, zfrom, s));
    SR_A(sr_launch_remove_rows(h->Wt, Np0, N0, q, h->alpha, coef, Wt1, Np1, alpha1, n_out, s));
    SR_A(sr_launch_remove_compact(h->yT, Np0, N0, q, yT1, alpha1, Np1, n_out, zstash, h->Z, zcount, (long)j * D, s));
    const int slide0 = h->slide;
    double *old_wt = wt_alloc_of(h), *old_yT = yT_alloc_of(h), *old_alpha = alpha_alloc_of(h);
    // (behind the launches that read the views; a failure here costs the spare buffers only: they are dropped below)
    const bool keep_old = same && (size_t)n_out * NN0 * sizeof(double) <= SR_FACT_PAR_BYTES * 2;
    bool cleaned = slide0 == 0;
    const bool clean_run = slide0 > 0 && keep_old && h->slack_ok;
    if (clean_run)
        cleaned = sr_launch_remove_clean(old_wt, old_alpha, old_yT, Np0, n_out, slide0, (long)(wt_doubles(n_out, Np0) - (size_t)n_out * NN0),
                                         SR_SLIDE_STEPS, s) == SR_OK;
    SR_AH(hipStreamSynchronize(s));
#undef SR_A
#undef SR_AH
    {   // sr_gp_last_remove: how this removal ran (host state only; the predicates above, and sr_launch_remove_rows' for the instance)
        int* lr = h->last_remove;
        lr[SR_RM_COUNT] = ++h->rm_count; lr[SR_RM_NP0] = Np0; lr[SR_RM_NP1] = Np1; lr[SR_RM_OFF0] = off0; lr[SR_RM_Q] = q;
        lr[SR_RM_SLIDE] = slide0; lr[SR_RM_ALIGNED] = reinterpret_cast<uintptr_t>(h->Wt) % 32 == 0 ? 1 : 0;
        lr[SR_RM_SPARE] = !reuse_alt ? SR_RM_SPARE_NONE : (h->wt_alt_off < off0 ? SR_RM_SPARE_CLEARED : SR_RM_SPARE_AS_IS);
        lr[SR_RM_VEC_SPARE] = vec_alt ? 1 : 0; lr[SR_RM_CLEAN] = clean_run && cleaned ? 1 : 0;
        lr[SR_RM_KEPT_OLD] = same && keep_old && cleaned ? 1 : 0;
    }
    h->yT = yT1; h->alpha = alpha1; h->Wt = Wt1;
    h->slide = 0;                                 // (a plain model; its buffers carry the zeroed slack: slack_ok stays)
    h->N = N1;
    h->logdet_valid = 0;
    if (same && !(keep_old && cleaned)) {
        // the old buffers cannot serve as spare ones (too big to keep, or slid and not put back in order)
        if (!vec_alt) { dev_free(h->yT_alt); dev_free(h->alpha_alt); }
        h->yT_alt = h->alpha_alt = nullptr; h->vec_alt_np = 0;
        if (reuse_alt) h->Wt_alt = nullptr;
        drop_wt_alt(h);
        dev_free(old_wt); dev_free(old_yT); dev_free(old_alpha);
        return SR_OK;
    }
    if (same) {
        if (!vec_alt) { dev_free(h->yT_alt); dev_free(h->alpha_alt); }
        h->yT_alt = old_yT; h->alpha_alt = old_alpha; h->vec_alt_np = Np0;
        // keep the previous buffer for the next removal or append (bounded: not for huge factors)
        if (reuse_alt) h->Wt_alt = nullptr;      // (that buffer holds the model now)
        drop_wt_alt(h);
        // (in the coordinates of its allocation a view `slide0` places down the diagonal has that many padding rows more)
        h->Wt_alt = old_wt; h->wt_alt_cap = (size_t)n_out * NN0; h->wt_alt_off = off0 + slide0;
    } else {
        // the padded size shrank: everything sized by Np is dropped and re-created lazily, as when an append grows it
        dev_free(old_wt);
        dev_free(old_yT); dev_free(old_alpha);
        dev_free(h->yT_alt); dev_free(h->alpha_alt); h->yT_alt = h->alpha_alt = nullptr; h->vec_alt_np = 0;
        drop_wt_alt(h);
        h->Np = Np1;
        drop_np_sized(h);
    }
    return SR_OK;
}

extern "C" int sr_gp_remove(sr_gp_t h, const int* idx_host, int m, void* stream) {
    SR_CHECK(h != nullptr && idx_host, SR_EINVAL, "sr_gp_remove: NULL argument");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_remove: model not factorized");
    SR_CHECK(!h->sparse, SR_ESTATE, "sr_gp_remove: sparse model (U^-1 is not the factor of K_y): refit with sr_gp_fit_sparse");
    SR_CHECK(!h->import_open, SR_ESTATE, "sr_gp_remove: between sr_gp_import_begin and sr_gp_import_end");
    SR_CHECK(m >= 1 && m < h->N, SR_EINVAL, "sr_gp_remove: m=%d outside 1..N-1 (N=%d: at least one point stays)", m, h->N);
    std::vector<int> idx(idx_host, idx_host + m);
    std::sort(idx.begin(), idx.end(), [](int a, int b) { return a > b; });       // descending: the indices behind stay valid
    for (int k = 0; k < m; ++k) {
        SR_CHECK(idx[k] >= 0 && idx[k] < h->N, SR_EINVAL, "sr_gp_remove: index %d outside [0, %d)", idx[k], h->N);
        SR_CHECK(k == 0 || idx[k] != idx[k - 1], SR_EINVAL, "sr_gp_remove: index %d given twice", idx[k]);
    }
    hipStream_t s = (hipStream_t)stream;
    SR_DEVICE(h->device);
    SR_TRY(server_quiesce(h));            // (it stays armed: the next single query launches it on the shrunken model)
    model_rewritten(h);
    // the scratch of every removal of this call up front (the first one is the biggest): none of them can run out of it
    SR_TRY(h->rm_ws.grow((size_t)h->n_out * sr_remove_coef_stride(h->Np) + (size_t)h->N * h->D, wait::device()));
    for (int k = 0; k < m; ++k) SR_TRY(remove_one(h, idx[k], s));
    return SR_OK;
}

extern "C" int sr_gp_last_remove(sr_gp_t h, int* out, int cap) {
    SR_CHECK(h && out && cap >= 1, SR_EINVAL, "sr_gp_last_remove: bad argument");
    const int n = std::min(cap, (int)SR_REMOVE_WORDS);
    std::copy(h->last_remove, h->last_remove + n, out);
    out[SR_RM_COUNT] = h->rm_count;               // (a fit in between has set it back; the other words stay those of the last removal)
    return n;
}

extern "C" int sr_gp_loo(sr_gp_t h, double* mu_loo, double* var_loo, void* stream) {
    SR_CHECK(h != nullptr, SR_EINVAL, "sr_gp_loo: NULL handle");
    SR_CHECK(h->factorized, SR_ESTATE, "sr_gp_loo: model not factorized");
    SR_CHECK(!h->sparse, SR_ESTATE, "sr_gp_loo: sparse model (U^-1 is not the factor of K_y)");
    SR_CHECK(!h->import_open, SR_ESTATE, "sr_gp_loo: between sr_gp_import_begin and sr_gp_import_end");
    if (!mu_loo && !var_loo) return SR_OK;
    SR_DEVICE(h->device);
    // (no unslide: the kernel loads single doubles, a view of the in-place appends is read as it is)
    return sr_launch_loo(h->Wt, h->alpha, h->yT, h->N, h->Np, h->n_out, mu_loo, var_loo, (hipStream_t)stream);
}
