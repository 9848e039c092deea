// sr_capi_chain.hip -- the dispatch of the persistent chain kernel (sr_chain.hip K0c).
// try_chain decides whether a chain of H steps runs in that kernel and launches it; sr_capi_reach.hip calls it ahead of its
// per-step launches.  The process-wide gate keeps two chain launches of one device from overlapping.  The switches of the
// route are here too: sr_gp_set_chain, sr_gp_last_chain, sr_gp_chain_status, and the test hook sr_test_chain_drop.
#include "sr_handle.h"
using namespace srh;

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
int srh::try_chain(sr_gp* h, long T, int H, int mode, const double* p0, const double* q0, const double* k_fb0,
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
            sr_chain_args ca{};
            model_args(ca.k, h);
            ca.k.na = n_s; ca.k.nb = n_u;
            ca.Wt = h->Wt; ca.T = Tc; ca.H = H; ca.mode = mode;
            ca.p0 = p0 + t0 * n_s; ca.q0 = q0 ? q0 + t0 * nss : nullptr; ca.k_fb0 = k_fb0 ? k_fb0 + t0 * nus : nullptr;
            ca.k_ff = k_ff + t0 * H * n_u; ca.k_fb = k_fb ? k_fb + t0 * (H - 1) * nus : nullptr;
            // the kernel stages l_mu and l_sigma into LDS in every mode; the moment modes use neither (nor c_safety) and pass
            // NULL: `a` stands in, as in ell_args for the per-step launches
            ca.a = a; ca.b = b; ca.l_mu = mode ? a : l_mu; ca.l_sigma = mode ? a : l_sigma; ca.c_safety = mode ? 1.0 : c_safety;
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
        }
        h->last_chain = 1;
        *taken = true;
        return SR_OK;
    }
    return SR_OK;
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
