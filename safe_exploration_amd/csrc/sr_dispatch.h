// sr_dispatch.h -- from a run-time value to a kernel template instantiation, and the launch (host side only).
//
//   sr_pick_le<3, 5, 8, 12>("kstar", a.D, [&](auto dt) {
//       return sr_launch(sr_kstar_general_kernel<decltype(dt)::value>, grid, dim3(256), 0, s, a); });
//
// Every site names its own list, so the set of instantiated kernels is what the site spells out.  A value outside the list is
// SR_EUNSUPPORTED, also where a predicate in front keeps such values away (sr_gp_small_wanted, SR_STREAM_FUSED_MAX_D,
// sr_gp_server_supported, sr_chain_supported): the predicates decide the route, the refusal here is what is left if one of
// them and a list ever disagree.
// The pickers need no HIP: a host compiler takes this header alone (tests/test_dispatch_host.py).
#pragma once
#include <algorithm>
#include <type_traits>
#include "../../include/safereach.h"

void sr_set_error(const char* fmt, ...);

#ifdef __HIPCC__
#define SR_HOST_DEVICE __host__ __device__
#else
#define SR_HOST_DEVICE
#endif

// the compiled input widths: the only definition of the 3 / 5 / 8 / 12 bucket (kernels templated on DT hold D <= DT columns)
constexpr SR_HOST_DEVICE int sr_width_bucket(int D) { return D <= 3 ? 3 : (D <= 5 ? 5 : (D <= 8 ? 8 : 12)); }

// f(std::integral_constant<int, W>{}) for the first W of the list that takes v (LE: v <= W, otherwise v == W), its return code
// in rc; false, and f not called, when none does
template <bool LE, int... Ws, class F>
bool sr_pick_first(int v, int& rc, F&& f) {
    return (((LE ? v <= Ws : v == Ws) && ((rc = f(std::integral_constant<int, Ws>{})), true)) || ...);
}

// first width that takes the value; no width: "<what>: D=<v> > <largest W>"
template <int... Ws, class F>
int sr_pick_le(const char* what, int v, F&& f) {
    int rc = SR_EUNSUPPORTED;
    if (!sr_pick_first<true, Ws...>(v, rc, f)) sr_set_error("%s: D=%d > %d", what, v, std::max({Ws...}));
    return rc;
}

// the exact value; not in the list: the site's own text `fmt` with v for its one %d
template <int... Vs, class F>
int sr_pick_eq(const char* fmt, int v, F&& f) {
    int rc = SR_EUNSUPPORTED;
    if (!sr_pick_first<false, Vs...>(v, rc, f)) sr_set_error(fmt, v);
    return rc;
}

// the padded sizes of the one-workgroup-per-output family (small, server, chain): SR_FUSED_NP in steps of SR_NB
template <class F>
int sr_pick_np(const char* fmt, int Np, F&& f) { return sr_pick_eq<128, 256, 384, 512>(fmt, Np, f); }

#ifdef __HIPCC__
// launch and check: the arguments are converted to the kernel's parameter types here, as a <<< >>> launch would
template <class... KA, class... A>
int sr_launch(void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, static_cast<KA>(args)...);
    SR_HIP(hipGetLastError());
    return SR_OK;
}
#endif
