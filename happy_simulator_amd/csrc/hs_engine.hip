// hs_engine.hip -- libhs_hip.so: HIP kernels (gfx950) and the C ABI declared in include/hs_engine.h.
//
// Replaces `Simulation._execute_until` / `_build_summary` (happysimulator/core/simulation.py:449-505,
// :543-591) and the replica fan-out of happysimulator/parallel for station LPs.  Data layout, kernels and
// their rooflines are described in DESIGN.md.  There is no CPU fallback in this file by design.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <vector>
#include <map>
#include <mutex>
#include <utility>

#define HS_KERNELS_MAIN
#include "hs_kernels.hpp"
#include "hs_tables_api.hpp"
#include "hs_host.hpp"
#include "hs_plan.hpp"

// =============================================================================================
// host side
// =============================================================================================
struct hs_engine {
    bool pending_async = false;   // hs_engine_run_until_async enqueued a run whose results hs_engine_synchronize has not finalised yet

    hs_config cfg{};
    int C = 1;                 // departure slots compiled for (>= max concurrency)
    bool have_stations = false;
    bool initialised = false;  // reset done
    hipStream_t stream = nullptr;
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    std::vector<void *> allocs;
    std::vector<std::pair<void *, size_t>> uncached;   // buffers of the process-wide uncached pool this engine holds (uncached_alloc)
    StationParams P{};
    StationState X{};
    RecordLogs L{};
    Totals *tot = nullptr;
    Candidate *cands = nullptr;
    bool is_net = false;
    bool any_xsrc = false;     // some LP has more than one Source (general path + prologue)
    int n_pass = 0;            // tandem queues (Server -> Server): passes of the station kernel, 0 = none
    // ... whose nanosecond ties the passes' lineage key does not decide (Totals::undecided), or which stand next to Probes / scheduled
    // Requests / several Sources per Server, run on the single-heap loop (hs_exact.hpp) from start to end instead
    bool exact_only = false;
    bool net_on_heap = false;     // ... a network that moved there behind an undecided election (tandem_fallback); hs_engine_reset moves it back
    std::vector<int32_t> h_src_lp;     // the Sources in `sources=[...]` order (hs_engine_set_stations), kept for setup_exact_plain
    std::vector<uint8_t> h_src_slot;
    std::vector<uint64_t> h_stream_base;   // the stations' effective stream_base (hs_engine_set_network: the default of routers and links)
    bool tandem_fan_in = false;   // some Server is the downstream of several Servers: no passes, the single heap from the start
    bool exact_prologue = false;   // the prologue takes part in ordinary runs (pre-run events whose indices run-time events can pass)
    // ... but only where a pre-run event shares its nanosecond with another event of its LP, or while the run has created fewer
    // events than there are pre-run events, can the second counter change an order -- and the prologue is one lane for the whole
    // engine (65 536 chains with a Probe each: 2.2 s before a 3 ms run).  A station engine therefore runs WITHOUT it first; the
    // kernels report the coincidences (Totals::undecided bit 2), and only then is the run repeated, window by window, behind the
    // prologue (prologue_fallback).  Debug flag 1 << 16 keeps the prologue in every run.  Round 4: network engines driven with
    // hs_engine_run_until do the same (NetStation::run_group reports the coincidences, messages included) -- a 16 384-station ring with
    // a Probe per station spent 0.5 s on the single lane before a run of milliseconds; shards of a partitioned network keep it.
    bool lazy_prologue = false, lazy_failed = false;
    int64_t n_init = 0;            // pre-run events of the engine
    std::vector<int64_t> window_ends;   // tandem queues: the end times of the run_until calls since the last reset (replayed on the single heap)
    bool uni_stations = false; // every LP: Poisson Source, exponential single-worker Server, unbounded queue, no stop_after
    bool uni_grid = false;     // ... and a Sink behind every Server: hs_station_run<1, false, true, true>
    bool f64_times = false;    // every time of a run is a whole number of ns in [0, 2^52): the UNI kernels' exact binary64 time algebra
    bool net_uni = false;      // ... and every router has exactly one NetworkLink (exponential jitter, no loss): hs_net_async<1, false, true>
    bool any_timevarying = false, any_sched = false;   // (subsets of any_profile: what a network does not lower)
    bool any_profile = false;  // some source has a time-varying rate profile (or a probe: same kernel instantiation)
    bool any_probe = false;
    int n_probe_slots = 1;     // probe slots in use (max probes on one LP): sizes the probe logs
    NetParams NP{};
    NetState NX{};
    ShardCtl SC{};             // wend_slots == nullptr: the engine holds the whole network
    bool net_global = false;   // link endpoints are network-wide station indices (set_network with n_global_lp > 0)
    int32_t n_global_lp = 0;
    int32_t *gid2local = nullptr;
    int64_t n_gid = 0;
    const int64_t *inbox = nullptr;
    int64_t *shard_gvt = nullptr;
    int64_t final_win = 0;
    bool external_stream = false;
    hipStream_t own_stream = nullptr;
    std::vector<int32_t> h_link_dst, h_link_src, h_gid2local;
    int64_t window_ns = 0;
    bool net_ran = false;
    int64_t net_last_end = INT64_MIN;   // end_ns of the run since the last reset (windows: see hs_engine_run_until_async)
    bool net_resume = false;            // ... and this run_until continues from the state that run left (hs_net_resume first)
    int64_t net_resume_from = 0;        // ... whose end_ns this was
    int net_window_path = 0;            // hs_engine_window_path
    int run_path = 0;                   // hs_engine_run_path: HS_RUN_* bits of what the last run launched
    int xs_phase_seen = 0;              // ... and the prologue's phase (XState::phase)
    Totals tot_seen{};                  // the totals hs_engine_run_until read behind the last run (valid until the next launch):
    bool tot_seen_valid = false;        //   the next window's decision without another round trip to the device
    std::vector<int64_t> drop_off_host;  // table-decided link losses (hs_network.link_drop_capacity): bit offsets per link
    uint32_t *drop_bits_dev = nullptr;
    LossTables loss_host{};              // (host copy of the device object: the send log's pointers)
    bool async_ok = false;     // the network can run on hs_net_async (whole network on this engine, queues allocated)
    int round_iters = 0;       // > 0: hs_net_async runs one exchange round of a shard (that many iterations), not a whole run
    // asynchronous shard rounds (hs_engine_shard_async_*): the network's cross-shard links
    int n_cross = 0;
    const int32_t *cross_local = nullptr;   // [n_cross] local link index (-1: this shard does not touch the link)
    const uint8_t *cross_role = nullptr;    // [n_cross] bit 0: the source station is here, bit 1: the destination is
    int64_t *cross_bounds = nullptr;        // device int64[n_cross + 1], owned by the caller (all-reduced with MAX)
    bool shard_async = false;
    // device-side exchange (hs_engine_shard_ipc_*): this rank's exchange buffers, written by the peers, and the peers' buffers
    int64_t *ipc_inbox = nullptr, *ipc_bounds = nullptr;      // [2][world][row] / [2][world][n_cross + 1], uncached device memory
    int64_t **peer_inbox_dev = nullptr, **peer_bounds_dev = nullptr;   // device arrays [world] of the ranks' buffers as mapped here
    std::vector<void *> ipc_opened;                           // peer mappings to close
    // LIVE exchange (ShardCtl::live): the ranks' link-queue arrays as mapped here, the links' indices at their destination ranks
    bool live_ready = false;
    int64_t **live_rec_dev = nullptr, **live_ea_dev = nullptr;
    unsigned long long **live_head_dev = nullptr;
    int32_t *live_link_dev = nullptr;
    hipStream_t live_stream = nullptr;   // the live launch's own stream: it waits for the peers' launches, nothing may queue behind it
    hipEvent_t live_ev = nullptr;
    bool ipc_ready = false;
    int ipc_parity = 0;
    bool net_pf = false;       // the network has probes / profiles / scheduled Requests: the PF instantiation of hs_net_async
    int round_iters_cfg = 0;
    int async_fit = -1;        // -1 unknown, 0 the grid is not co-resident (segments take turns: run_net_segments), 1 it is
    long long async_resident_blocks = 0;   // workgroups of hs_net_async one cooperative launch holds
    int async_lanes = 64;      // LPs per wavefront in hs_net_async
    int n_blocks = 0;
    int flags = 0;
    // prologue (hs_exact.hpp): SINGLE mode with probes / scheduled Requests
    bool exact = false;
    XState *xs = nullptr;
    XState xs_host{};          // the device pointers / capacities of *xs (phase etc. are reset from it)
    XInit XI{};
    // K lanes per LP (hs_kernels_wide.hpp): the uniform grid with fewer LPs than the device has lanes
    WideCtl *wide_ctl = nullptr; int32_t *wide_bail = nullptr;
    WavePart *wave_parts = nullptr;   // one wavefront per LP (hs_kernels_wave.hpp): the workgroups' partial totals
    int wide_K = 0;            // 0: one lane per LP (hs_station_run)
    bool fresh = false;        // nothing has run since the last reset (the wide kernel starts from empty queues)
    // hs_engine_reset on an engine whose next run is one wavefront per LP: the bootstrap is DEFERRED into that run's kernel
    // (hs_station_wave<NW, true>); anything else that touches the state first launches the reset kernel after all (ensure_reset)
    bool reset_pending = false;
    mutable long long device_lanes = 0;   // CUs x 4 SIMDs x 64 lanes of the engine's device (wide_lanes)
    // tick tables (hs_tables.hpp): Sources with a time-varying profile and Probes
    TickRow *tab_rows = nullptr; int n_tab_rows = 0; int64_t tab_cap = 0;
    int64_t *tab_times = nullptr, *tab_count = nullptr;
    unsigned long long *tab_status = nullptr;
    bool tables_built = false;
    long long lane_budget = kDefaultLaneBudget;
    double last_run_ms = 0.0, last_kernel_ms = 0.0;
    int64_t launches = 0;
    std::string error;
};

namespace {

// Uncached device memory (hipExtMallocWithFlags(hipDeviceMallocUncached): the buffers other ranks' kernels write into while this
// rank's kernel runs) comes from a process-wide pool and is never handed back to the runtime while the process lives.  Measured
// (round 6, tests/test_gpu_sharded.py in one process): after ~50 engines that each freed five such buffers, ordinary hipMalloc'ed
// arrays of a LATER engine read back as zeros although its kernels had written them -- an address range that changes its memory
// type between allocations is not safe here; with the pool (or without uncached memory) the same sequence is clean.
struct UncachedPool {
    std::mutex m;
    std::multimap<size_t, void *> idle;      // capacity in bytes -> buffer
};
UncachedPool &uncached_pool() { static UncachedPool *p = new UncachedPool; return *p; }
int uncached_alloc(hs_engine *h, void **out, size_t bytes) {
    const size_t want = ((bytes ? bytes : 1) + 65535) & ~(size_t)65535;
    {
        UncachedPool &P = uncached_pool();
        std::lock_guard<std::mutex> g(P.m);
        auto it = P.idle.lower_bound(want);
        if (it != P.idle.end() && it->first <= 2 * want) {
            *out = it->second;
            h->uncached.emplace_back(it->second, it->first);
            P.idle.erase(it);
            return HS_OK;
        }
    }
    void *q = nullptr;
    const hipError_t e = hipExtMallocWithFlags(&q, want, hipDeviceMallocUncached);
    if (e != hipSuccess) return fail(h, HS_E_HIP, "hipExtMallocWithFlags(%zu B, uncached): %s", want, hipGetErrorString(e));
    h->uncached.emplace_back(q, want);
    *out = q;
    return HS_OK;
}
void uncached_release(hs_engine *h) {
    UncachedPool &P = uncached_pool();
    std::lock_guard<std::mutex> g(P.m);
    for (auto &b : h->uncached) P.idle.emplace(b.second, b.first);
    h->uncached.clear();
}

template <int C>
void launch_run(hs_engine *h, int64_t end_ns, int mode, int flags) {
    if (h->n_pass > 0) {      // tandem queues: the general-path instantiation, one pass (hs_station.hpp `trk`)
        h->run_path |= HS_RUN_TANDEM;
        hipLaunchKernelGGL((hs_station_run<C, true>), dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->X, h->L, h->tot,
                           h->cands, h->cfg.n_lp, end_ns, mode, flags);
        return;
    }
    if constexpr (C == 1) {
        if (!h->any_profile && !(flags & 512)) {     // producer / consumer wavefronts (debug flag 512: the one-role kernel)
            h->run_path |= (h->uni_grid && (flags & (1 << 20)) == 0) ? HS_RUN_ONE_LANE_UNI : HS_RUN_ONE_LANE;
            if (h->uni_grid && (flags & (1 << 20)) == 0)   // uniform entity kinds: compile-time predicates (hs_station.hpp HSG)
                hipLaunchKernelGGL((hs_station_run<1, false, true, true>), dim3(h->n_blocks), dim3(2 * kBlock), 0, h->stream, h->P,
                                   h->X, h->L, h->tot, h->cands, h->cfg.n_lp, end_ns, mode, flags);
            else
                hipLaunchKernelGGL((hs_station_run<1, false, true>), dim3(h->n_blocks), dim3(2 * kBlock), 0, h->stream, h->P, h->X,
                                   h->L, h->tot, h->cands, h->cfg.n_lp, end_ns, mode, flags);
            return;
        }
    }
    h->run_path |= HS_RUN_ONE_LANE;
    if (h->any_profile)
        hipLaunchKernelGGL((hs_station_run<C, true>), dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->X, h->L, h->tot,
                           h->cands, h->cfg.n_lp, end_ns, mode, flags);
    else
        hipLaunchKernelGGL((hs_station_run<C, false>), dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->X, h->L, h->tot,
                           h->cands, h->cfg.n_lp, end_ns, mode, flags);
}

// K lanes per LP when the grid is uniform and leaves lanes idle (hs_kernels_wide.hpp); debug flag 1 << 22 keeps the one-lane kernel,
// bits 24..27 force K = 1 << (value - 1)
int wide_lanes(const hs_engine *h) {
    if (h->is_net) return 0;      // (a network's stations run on the network engines, whatever their egress arrays said before hs_engine_set_network)
    if (h->C != 1 || !h->uni_grid || h->any_profile || h->cfg.mode != HS_MODE_SINGLE || !h->fresh || h->wide_ctl == nullptr) return 0;
    if (h->flags & ((1 << 22) | 1 | 512 | (1 << 20))) return 0;
    const int forced = (h->flags >> 24) & 0xf;
    if (forced) return forced == 7 ? 64 : forced == 8 ? 65 : (1 << (forced - 1)) <= 16 ? 1 << (forced - 1) : 16;   // 7 / 8: a wavefront per LP, 16 / 8 LPs per workgroup
    const bool wave_ok = h->cfg.horizon_ns < (1ll << 39);      // (the speculated whole-ns arrival steps: hs_kernels_wave.hpp)
    // Measured on MI355X (tools/wide_timing.py, profiles/r03_wide_timing.log; 60 s of the headline grid, kernel ms):
    //   n_lp      one lane   K = 4    K = 8    K = 16
    //    1 024     0.372     0.118    0.087    0.093
    //    4 096     0.378     0.138    0.129    0.177
    //    8 192     0.385     0.166    0.187    0.315
    //   16 384     0.388     0.231    0.344    0.579
    //   32 768     0.403     0.422    0.610    1.059
    // Fewer lanes per LP = less redundant work in the serial arrival chain, more = shorter steps: K = 8 while the device has SIMDs
    // to spare, K = 4 up to a quarter of the size at which a lane per LP fills the machine.
    if (h->device_lanes == 0) {                                                  // (asked once: it is a ~10 us host call, twice per step)
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->cfg.device) != hipSuccess) return 0;
        h->device_lanes = (long long)prop.multiProcessorCount * 4 * 64;          // one wavefront per SIMD
    }
    const long long lanes = h->device_lanes;
    const long long n = h->cfg.n_lp;
    // Round 5: one wavefront per LP (hs_kernels_wave.hpp).  Measured (tools/wide_timing.py, profiles/r05_wide_timing.log; kernel ms incl.
    // hs_station_wide_finish): 1 024 LPs 0.056 (8 LPs per workgroup) / 0.068 (16) against K = 8: 0.087; 8 192: 0.106 against K = 4: 0.168;
    // 16 384: 0.17 against K = 4: 0.23; 32 768: 0.31 against one lane per LP: 0.40; 65 536: ~0.6 against 0.42 -- one lane per LP from there.
    // Later in round 5 (T without selects, bootstrap and fold once per LP on wavefront 0): 8 192: 0.089; 32 768: 0.27; 40 960: 0.34 against
    // 0.40; 45 056: 0.37 against 0.41; 49 152: 0.405 against 0.410 (the crossover); 65 536: 0.53 against 0.43.
    if (wave_ok && n * 16 <= lanes) return 65;  // <= 4 096 LPs: 8 LPs per workgroup (more workgroups than CUs)
    if (wave_ok && n * 3 <= lanes * 2) return 64;   // <= 43 690 LPs: 16 LPs per workgroup (a whole line of every record row)
    if (n * 16 <= lanes) return 8;              // <= 4 096 LPs on 256 CUs
    if (n * 4 <= lanes) return 4;               // <= 16 384 LPs
    return 0;
}
template <int K>
void launch_wide(hs_engine *h, int64_t end_ns) {
    const int n = h->cfg.n_lp, G = 64 / K, nb = (n + G - 1) / G;
    h->run_path |= HS_RUN_WIDE | (K << 16);
    hipLaunchKernelGGL(hs_station_wide<K>, dim3(nb), dim3(kWideBlock), 0, h->stream, h->P, h->X, h->L, h->tot, h->cands, h->wide_ctl,
                       h->wide_bail, n, end_ns, h->flags);
    hipLaunchKernelGGL(hs_station_wide_finish, dim3(1), dim3(kBlock), 0, h->stream, h->P, h->X, h->L, h->tot, h->cands, nb, h->wide_ctl,
                       h->wide_bail, n, end_ns, (const WavePart *)nullptr, (long long)INT64_MIN);
}
template <int NW>
void launch_wave(hs_engine *h, int64_t end_ns) {
    const int n = h->cfg.n_lp, nb = (n + NW - 1) / NW;
    h->run_path |= HS_RUN_WAVE | (NW << 16);
    const bool fresh = h->reset_pending;                      // the bootstrap inside the kernel, no hs_station_reset launch
    h->reset_pending = false;
    if (fresh)
        hipLaunchKernelGGL((hs_station_wave<NW, true>), dim3(nb), dim3(NW * 64), 0, h->stream, h->P, h->X, h->L, h->tot, h->cands, h->wide_ctl,
                           h->wide_bail, h->wave_parts, n, end_ns, h->flags, h->cfg.start_ns);
    else    // (wide_lanes() needs `fresh`: also this one only ever starts at ak0 = 1, sk0 = 0 -- its `ds` and `!da` branches are unreachable from here)
        hipLaunchKernelGGL((hs_station_wave<NW, false>), dim3(nb), dim3(NW * 64), 0, h->stream, h->P, h->X, h->L, h->tot, h->cands, h->wide_ctl,
                           h->wide_bail, h->wave_parts, n, end_ns, h->flags, h->cfg.start_ns);
    hipLaunchKernelGGL(hs_station_wide_finish, dim3(1), dim3(kBlock), 0, h->stream, h->P, h->X, h->L, h->tot, h->cands, nb, h->wide_ctl,
                       h->wide_bail, n, end_ns, (const WavePart *)h->wave_parts, fresh ? (long long)h->cfg.start_ns : (long long)INT64_MIN);
}

int ensure_reset(hs_engine *h);
int launch_run_dispatch(hs_engine *h, int64_t end_ns) {
    if (h->exact_only) return HS_OK;     // (the single-heap loop has run the whole window: launch_prologue)
    const int K = wide_lanes(h);
    // (only hs_station_wave performs a deferred bootstrap itself; ADVICE r5: a reset launch that fails is the run's failure)
    if (K != 64 && K != 65) { const int rcr = ensure_reset(h); if (rcr) return rcr; }
    h->fresh = false;
    switch (K) {
        case 4: launch_wide<4>(h, end_ns); return HS_OK;
        case 8: launch_wide<8>(h, end_ns); return HS_OK;
        case 16: launch_wide<16>(h, end_ns); return HS_OK;
        case 64: launch_wave<16>(h, end_ns); return HS_OK;
        case 65: launch_wave<8>(h, end_ns); return HS_OK;
        default: break;
    }
    // Tandem queues: one launch per pass, upstream Servers first; the last one elects the event beyond end_ns among ALL LPs
    // (an internal mode 2 = "no election" for the others).  Everything else: one launch.
    const int passes = h->n_pass > 0 ? h->n_pass : 1;
    for (int p = 0; p < passes; ++p) {
        const int mode = (p == passes - 1) ? h->cfg.mode : 2;
        const int flags = h->n_pass > 0 ? (h->flags | ((p + 1) << 28)) : h->flags;
        switch (h->C) {
            case 1: launch_run<1>(h, end_ns, mode, flags); break;
            case 2: launch_run<2>(h, end_ns, mode, flags); break;
            case 4: launch_run<4>(h, end_ns, mode, flags); break;
            case 8: launch_run<8>(h, end_ns, mode, flags); break;
            case 16: launch_run<16>(h, end_ns, mode, flags); break;
            default: launch_run<32>(h, end_ns, mode, flags); break;     // (departure slots beyond 16 live in scratch: correct, not fast)
        }
    }
    return HS_OK;
}

template <int C>
void launch_net(hs_engine *h, int64_t wend, int win, int flags) {
    hipLaunchKernelGGL(hs_net_window<C>, dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->NP, h->X, h->NX, h->L,
                       h->tot, h->cands, h->cfg.n_lp, wend, win, flags, h->SC);
}
void launch_net_dispatch(hs_engine *h, int64_t wend, int win, int flags) {
    switch (h->C) {
        case 1: launch_net<1>(h, wend, win, flags); break;
        case 2: launch_net<2>(h, wend, win, flags); break;
        default: launch_net<4>(h, wend, win, flags); break;
    }
}

// windows: finish the timestamp group the last run_until's election stopped inside (hs_kernels.hpp hs_net_resume)
void launch_net_resume(hs_engine *h, const NetState &NX, int send_idx) {
    switch (h->C) {
        case 1: hipLaunchKernelGGL(hs_net_resume<1>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, NX, h->L, h->tot, h->cfg.n_lp, send_idx, h->SC); break;
        case 2: hipLaunchKernelGGL(hs_net_resume<2>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, NX, h->L, h->tot, h->cfg.n_lp, send_idx, h->SC); break;
        default: hipLaunchKernelGGL(hs_net_resume<4>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, NX, h->L, h->tot, h->cfg.n_lp, send_idx, h->SC); break;
    }
    h->launches++;
}

// the uniform-kind instantiation of hs_net_async (debug flag 1 << 20 keeps the generic one)
bool async_uni(const hs_engine *h, int lanes) {
    return h->C == 1 && h->net_uni && !h->net_pf && !h->net_global && (h->flags & ((1 << 20) | 1 | 32)) == 0 && h->round_iters == 0 && lanes == 64;
}
template <int C>
hipError_t launch_async(hs_engine *h, int64_t end_ns, NetState NX) {
    int n = h->cfg.n_lp, flags = h->flags & (1 | 64 | 128 | 1024 | 0xff00 | (1 << 21)), lanes = h->async_lanes;
    const int per_block = (kBlock / 64) * lanes;
    int max_iters = h->round_iters;
    void *args[] = {&h->P, &h->NP, &h->X, &NX, &h->L, &h->tot, &n, &end_ns, &flags, &h->SC, &lanes, &max_iters};
    const void *fn = h->net_pf ? (const void *)hs_net_async<C, true> : (const void *)hs_net_async<C, false>;
    if constexpr (C == 1) {    // uniform entity kinds: the specialised instantiation (debug flag 1 << 20 keeps the generic one)
        if (async_uni(h, lanes)) fn = (const void *)hs_net_async<1, false, true>;
    }
    // LIVE exchange: the ranks' kernels wait for one another, and several of them may share this device (shards of one process, or
    // of several processes) -- a plain launch each: what makes them co-resident is that together they have no more workgroups than
    // the device has CUs (hs_engine_shard_live_run checks its own share)
    if (h->SC.live) return hipLaunchKernel(fn, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBlock), args, 0, h->stream);
    return hipLaunchCooperativeKernel(fn, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(kBlock), args, 0, h->stream);
}
// one SEGMENT of a network that does not fit one cooperative launch: stations [lp0, lp0 + blocks x 256) for `iters` iterations of
// the generic asynchronous kernel (the segment's first station travels in bits 8.. of `lanes`)
template <int C>
hipError_t launch_async_segment(hs_engine *h, int64_t end_ns, NetState NX, int lp0, int blocks, int iters) {
    int n = h->cfg.n_lp, flags = h->flags & (1 | 64 | 128 | 1024 | 0xff00 | (1 << 21)), lanes = 64 | ((lp0 / kBlock) << 8), max_iters = iters;
    void *args[] = {&h->P, &h->NP, &h->X, &NX, &h->L, &h->tot, &n, &end_ns, &flags, &h->SC, &lanes, &max_iters};
    const void *fn = h->net_pf ? (const void *)hs_net_async<C, true> : (const void *)hs_net_async<C, false>;
    return hipLaunchCooperativeKernel(fn, dim3((unsigned)blocks), dim3(kBlock), args, 0, h->stream);
}
template <int C, bool PF>
int async_blocks_per_cu() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, hs_net_async<C, PF>, kBlock, 0) != hipSuccess) return 0;
    return nb;
}

// The whole run in one launch of hs_net_async + the final launch of hs_net_window (election of the one event beyond
// end_ns).  Returns 1 if it ran, 0 if the network has to use the windowed engine, < 0 on error.
int try_run_net_whole(hs_engine *h, int64_t end_ns);
int ensure_async_fit(hs_engine *h) {
    if (h->async_fit < 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, h->cfg.device) != hipSuccess) return 0;
        const int per_cu = h->net_pf ? (h->C == 1 ? async_blocks_per_cu<1, true>() : h->C == 2 ? async_blocks_per_cu<2, true>() : async_blocks_per_cu<4, true>())
                                     : (h->C == 1 ? async_blocks_per_cu<1, false>() : h->C == 2 ? async_blocks_per_cu<2, false>() : async_blocks_per_cu<4, false>());
        const long long resident = prop.cooperativeLaunch ? (long long)per_cu * prop.multiProcessorCount : 0;   // workgroups
        h->async_resident_blocks = resident;
        h->async_fit = 0;
        for (int lanes = (h->flags & 32) ? 16 : 64; lanes <= 64; lanes *= 2) {
            const int per_block = (kBlock / 64) * lanes;
            if (((long long)h->cfg.n_lp + per_block - 1) / per_block <= resident) { h->async_lanes = lanes; h->async_fit = 1; break; }
        }
    }
    return h->async_fit;
}
// A network with MORE stations than one cooperative launch holds (round 5, VERDICT r4 missing 5: at 65 537 stations hs_engine_run_until
// used to fall to one launch per smallest link latency, 60 000 launches per 60 s).  The asynchronous protocol does not care who runs
// when: a station only ever advances below the bounds its incoming links carry, and a neighbour that is not running simply does
// not raise its bound.  So contiguous SEGMENTS of stations take turns on the device -- every launch advances one segment by
// `kSegmentIters` iterations against the bounds and queues the others left in global memory -- until no station has work at or
// before end_ns (Totals::not_done, read once per sweep).  The same bits as one launch (tests/test_gpu_ring.py); what the
// partitioned run does across GPUs (sharded.py), without outboxes: all segments share this engine's link queues.
constexpr int kSegmentIters = 64;
int run_net_segments(hs_engine *h, int64_t end_ns, NetState NX, long long resident_blocks) {
    const int n = h->cfg.n_lp;
    const long long total_blocks = ((long long)n + kBlock - 1) / kBlock;
    const int nseg = (int)((total_blocks + resident_blocks - 1) / resident_blocks);
    const long long per_seg = (total_blocks + nseg - 1) / nseg;              // balanced: no short last segment
    for (int sweep = 0; sweep < (1 << 20); ++sweep) {
        HS_HIP(h, hipMemsetAsync(&h->tot->not_done, 0, sizeof(unsigned long long), h->stream));
        for (int sgm = 0; sgm < nseg; ++sgm) {
            const long long b0 = (long long)sgm * per_seg, b1 = std::min<long long>(total_blocks, b0 + per_seg);
            if (b1 <= b0) continue;
            const hipError_t e = h->C == 1 ? launch_async_segment<1>(h, end_ns, NX, (int)(b0 * kBlock), (int)(b1 - b0), kSegmentIters)
                               : h->C == 2 ? launch_async_segment<2>(h, end_ns, NX, (int)(b0 * kBlock), (int)(b1 - b0), kSegmentIters)
                                           : launch_async_segment<4>(h, end_ns, NX, (int)(b0 * kBlock), (int)(b1 - b0), kSegmentIters);
            if (e != hipSuccess) return fail(h, HS_E_HIP, "cooperative launch of a network segment failed: %s", hipGetErrorString(e));
            h->launches++;
        }
        unsigned long long left[2] = {0, 0};
        int ov = 0;
        HS_HIP(h, hipMemcpyAsync(&left[0], &h->tot->not_done, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipMemcpyAsync(&ov, &h->tot->overflow, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (left[0] == 0ull || ov != 0) return HS_OK;
    }
    return fail(h, HS_E_HIP, "the segmented asynchronous run did not finish");
}

int try_run_net_whole(hs_engine *h, int64_t end_ns) {
    if (!h->async_ok || (h->flags & 16)) return 0;
    if (!ensure_async_fit(h)) {
        // more stations than one cooperative launch holds: segments take turns (debug flag 1 << 23: the window protocol instead)
        if ((h->flags & (1 << 23)) || h->async_resident_blocks < 1) return 0;
        NetState NXs = h->NX;
        NXs.aq_on = 1;
        if (h->net_resume) launch_net_resume(h, NXs, 0);
        h->run_path |= HS_RUN_NET_SEGMENTED;
        const int rc = run_net_segments(h, end_ns, NXs, h->async_resident_blocks);
        if (rc) return rc;
        const NetState keep = h->NX;
        h->NX = NXs;
        launch_net_dispatch(h, end_ns, 1, (h->flags & 1) | 2 | 8);       // FINAL: leftover queue entries, overshoot
        h->NX = keep;
        HS_HIP(h, hipGetLastError());
        h->launches += 1;
        h->net_ran = true;
        return 1;
    }
    NetState NX = h->NX;
    NX.aq_on = 1;
    if (h->net_resume) launch_net_resume(h, NX, 0);
    hipError_t e = h->C == 1 ? launch_async<1>(h, end_ns, NX) : h->C == 2 ? launch_async<2>(h, end_ns, NX) : launch_async<4>(h, end_ns, NX);
    if (e != hipSuccess) {      // not co-resident after all
        (void)hipGetLastError();
        h->async_fit = 0;
        if (h->net_resume) return fail(h, HS_E_HIP, "the cooperative launch of a resumed window failed: %s", hipGetErrorString(e));
        return 0;               // ... windows
    }
    h->run_path |= HS_RUN_NET_ASYNC | (async_uni(h, h->async_lanes) ? HS_RUN_NET_ASYNC_UNI : 0);
    const NetState keep = h->NX;
    h->NX = NX;
    launch_net_dispatch(h, end_ns, 1, (h->flags & 1) | 2 | 8);       // FINAL: leftover queue entries, overshoot
    h->NX = keep;
    HS_HIP(h, hipGetLastError());
    h->launches += 2;
    h->net_ran = true;
    return 1;
}

// EXECUTE / EXCHANGE / ADVANCE (parallel/coordinator.py:87-124) as a stream of window launches
int run_net_async(hs_engine *h, int64_t end_ns) {
    { const int rcr = ensure_reset(h); if (rcr) return rcr; }     // (never a network run on a deferred bootstrap)
    {
        const int whole = try_run_net_whole(h, end_ns);
        if (whole != 0) return whole < 0 ? whole : HS_OK;
    }
    const int64_t W = h->window_ns;
    int64_t t0 = h->cfg.start_ns;
    int win = 0;
    h->run_path |= HS_RUN_NET_WINDOWED;
    if (h->net_resume) {
        // windows: the conservative windows continue behind the last end (everything at or before it has happened); what the
        // finished group sends waits in the incoming bags the first window merges (parity 1)
        launch_net_resume(h, h->NX, 1);
        t0 = h->net_resume_from + 1;
    }
    for (;;) {
        int64_t wend = t0 + W - 1;
        if (wend >= end_ns || wend < t0) wend = end_ns;
        launch_net_dispatch(h, wend, win, h->flags & 1);
        ++win;
        if (wend >= end_ns) break;
        t0 = wend + 1;
    }
    launch_net_dispatch(h, end_ns, win, (h->flags & 1) | 2);   // FINAL: merge the last window's messages, overshoot
    HS_HIP(h, hipGetLastError());
    h->launches += win + 1;
    h->net_ran = true;
    return HS_OK;
}

// the reset kernel itself (the Simulation.__init__ bootstrap on the device)
int launch_reset(hs_engine *h);
int ensure_reset(hs_engine *h) {
    if (!h->reset_pending) return HS_OK;
    h->reset_pending = false;
    return launch_reset(h);
}
int do_reset_async(hs_engine *h) {
    // An engine whose next run is hs_station_wave (wide_lanes() == 64 / 65 once `fresh`): that kernel performs the bootstrap itself
    // (FRESH instantiation) and hs_station_wide_finish starts the totals -- no reset launch, no state round trip through HBM.
    // Debug flag 1 << 29 keeps the reset kernel.
    {
        const bool was_fresh = h->fresh;
        h->fresh = true;
        const int K = (h->flags & (1 << 29)) ? 0 : wide_lanes(h);
        h->fresh = was_fresh;
        if ((K == 64 || K == 65) && !h->exact) {
            h->reset_pending = true;
            h->initialised = true;
            h->net_ran = false;
            h->net_last_end = INT64_MIN;
            h->tot_seen_valid = false;
            h->fresh = true;
            h->window_ends.clear();
            h->pending_async = false;
            return HS_OK;
        }
    }
    h->reset_pending = false;
    return launch_reset(h);
}
int launch_reset(hs_engine *h) {
    if (h->n_tab_rows > 0 && !h->tables_built) {      // the tick tables (hs_tables.hpp): once, BEFORE the bootstrap reads tick 0
        HS_HIP(h, tick_tables_launch(h->stream, h->tab_rows, h->n_tab_rows, h->cfg.start_ns, h->cfg.horizon_ns, h->tab_cap,
                                     h->tab_times, h->tab_count, h->tab_status, h->lane_budget, false));
        h->tables_built = true;
    }
    if (h->any_profile)
        hipLaunchKernelGGL(hs_station_reset<true>, dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->X, h->tot,
                           h->cfg.n_lp, h->C, h->cfg.start_ns, h->NX, h->is_net ? h->NP.n_links : 0);
    else
        hipLaunchKernelGGL(hs_station_reset<false>, dim3(h->n_blocks), dim3(kBlock), 0, h->stream, h->P, h->X, h->tot,
                           h->cfg.n_lp, h->C, h->cfg.start_ns, h->NX, h->is_net ? h->NP.n_links : 0);
    HS_HIP(h, hipGetLastError());
    if (h->exact) {            // the prologue starts over: empty heap, both counters at 0
        if (h->XI.per_lp) HS_HIP(h, hipMemsetAsync(h->xs, 0, ((size_t)h->cfg.n_lp + 1) * sizeof(XState), h->stream));
        HS_HIP(h, hipMemcpyAsync(h->xs, &h->xs_host, sizeof(XState), hipMemcpyHostToDevice, h->stream));
        HS_HIP(h, hipMemsetAsync(h->xs_host.qhead, 0xff, (size_t)h->cfg.n_lp * sizeof(int32_t), h->stream));
        HS_HIP(h, hipMemsetAsync(h->xs_host.qtail, 0xff, (size_t)h->cfg.n_lp * sizeof(int32_t), h->stream));
    }
    if (h->is_net && h->loss_host.send_log_n) HS_HIP(h, hipMemsetAsync(h->loss_host.send_log_n, 0, sizeof(unsigned long long), h->stream));
    h->initialised = true;
    h->net_ran = false;
    h->net_last_end = INT64_MIN;
    h->tot_seen_valid = false;
    h->fresh = true;
    h->window_ends.clear();
    h->pending_async = false;      // (a run enqueued before this reset has nothing left to finalise)
    return HS_OK;
}

bool lazy_active(const hs_engine *h) {
    // (a shard of a partitioned network is driven window by window / round by round from outside: it keeps the eager prologue)
    return h->lazy_prologue && !h->lazy_failed && !(h->is_net && h->net_global) && !h->exact_only && (h->flags & (1 << 16)) == 0;
}

// the prologue of a run (hs_exact.hpp); a no-op launch once it has handed over
int launch_prologue(hs_engine *h, int64_t end_ns) {
    if (!h->exact || (h->flags & 256)) return HS_OK;
    if (!h->exact_prologue && !h->exact_only) return HS_OK;
    if (h->lazy_prologue) h->P.sched_idx = lazy_active(h) ? nullptr : h->XI.sched_idx;   // (the prologue writes them)
    if (lazy_active(h)) return HS_OK;
    h->XI.no_handover = h->exact_only ? 1 : 0;
    if (h->exact_only) h->run_path |= HS_RUN_SINGLE_HEAP;
    hipLaunchKernelGGL(hs_exact_run, dim3(h->XI.per_lp ? (unsigned)((h->cfg.n_lp + 63) / 64) : 1u), dim3(64), 0, h->stream, h->P, h->NP, h->X, h->NX, h->L, h->tot, h->xs, h->XI,
                       h->cfg.n_lp, h->C, h->is_net ? 1 : 0, h->is_net ? h->NP.n_links : 0, h->cfg.start_ns, end_ns);
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

// the ranks' exchange buffers as this process addresses them -> device arrays for hs_shard_push
int ipc_set_peers(hs_engine *h, const std::vector<int64_t *> &pin, const std::vector<int64_t *> &pbd) {
    const int world = h->SC.world;
    int rc;
    if ((rc = dev_alloc(h, &h->peer_inbox_dev, (size_t)world))) return rc;
    if ((rc = dev_alloc(h, &h->peer_bounds_dev, (size_t)world))) return rc;
    HS_HIP(h, hipMemcpy(h->peer_inbox_dev, pin.data(), (size_t)world * sizeof(int64_t *), hipMemcpyHostToDevice));
    HS_HIP(h, hipMemcpy(h->peer_bounds_dev, pbd.data(), (size_t)world * sizeof(int64_t *), hipMemcpyHostToDevice));
    h->ipc_ready = true;
    h->ipc_parity = 0;
    return HS_OK;
}

}  // namespace

// =============================================================================================
// set-up: plan_stations / plan_network (hs_plan.hpp) decide, these two allocate and upload what was decided
// =============================================================================================
namespace {

template <typename T>
int upload_vec(hs_engine *h, const T **dst, const std::vector<T> &v) { return upload<T>(h, dst, v.data(), v.size(), T{}); }
template <typename T>
int upload_col(hs_engine *h, const T **dst, const Col<T> &c) { return upload<T>(h, dst, c.p, (size_t)h->cfg.n_lp, c.dflt); }
// (inside the apply functions: `h`, the plan `p` and `int rc` are in scope)
#define DA(ptr, count) if ((rc = dev_alloc(h, &(ptr), count))) return rc
#define UPV(dst, vec) if ((rc = upload_vec(h, &(dst), p.vec))) return rc
#define UPC(dst, col) if ((rc = upload_col(h, &(dst), p.col))) return rc
template <typename T>
int alloc_zeroed(hs_engine *h, T **p, size_t count) {
    const int rc = dev_alloc(h, p, count);
    if (rc) return rc;
    HS_HIP(h, hipMemset(*p, 0, (count ? count : 1) * sizeof(T)));     // (dev_alloc hands out at least one element)
    return HS_OK;
}

// the buffers of the prologue / the single heap (hs_exact.hpp XState), sized by the plan
int alloc_xstate(hs_engine *h, const StationPlan &p) {
    const size_t n = (size_t)h->cfg.n_lp;
    int rc;
    h->xs_host = p.xs;
    DA(h->xs_host.heap, p.xs_heap); DA(h->xs_host.qhead, n); DA(h->xs_host.qtail, n);
    DA(h->xs_host.pnext, p.xs_pool); DA(h->xs_host.pidx, p.xs_pool); DA(h->xs_host.init_t, p.xs_init);
    return dev_alloc(h, &h->xs, p.xs_count);
}

// the tick tables and the arrays that travel with them (hs_tables.hpp TickTables)
int apply_tick_tables(hs_engine *h, const StationPlan &p) {
    const size_t n = (size_t)h->cfg.n_lp, cap = (size_t)p.log_cap;
    int rc;
    if (!p.rows.empty()) {
        DA(h->tab_rows, p.rows.size());
        HS_HIP(h, hipMemcpy(h->tab_rows, p.rows.data(), p.rows.size() * sizeof(TickRow), hipMemcpyHostToDevice));
        DA(h->tab_times, p.rows.size() * (size_t)p.tab_cap); DA(h->tab_count, p.rows.size());
        if ((rc = alloc_zeroed(h, &h->tab_status, 2))) return rc;
    }
    TickTables tt{};
    tt.times = h->tab_times; tt.cap = p.tab_cap; tt.t_start = h->cfg.start_ns;
    if (!p.tandem.empty()) {                                      // tandem queues: hs_tables.hpp TickTables::tandem
        UPV(tt.tandem, tandem);
        if ((rc = alloc_zeroed(h, &tt.inj_i, (size_t)kMaxUp * n))) return rc;
        for (int64_t **col : {&tt.fw_rc, &tt.fw_rrc, &tt.fw_rdr, &tt.fw_dep}) DA(*col, n * cap);
        for (int64_t **col : {&tt.q_rrc, &tt.q_rdr, &tt.q_pay}) DA(*col, n * (size_t)kQCap);
    }
    if (p.cand_key && (rc = alloc_zeroed(h, &tt.cand_key, n * 4))) return rc;
    tt.standin_sched = p.standin_sched ? 1 : 0;
    if (p.lineage_src) {
        DA(tt.rs_dep, n * (size_t)p.C); DA(tt.rs_q, n * (size_t)kQCap);
        HS_HIP(h, hipMemset(tt.rs_dep, 0xff, n * (size_t)p.C));
        HS_HIP(h, hipMemset(tt.rs_q, 0xff, n * (size_t)kQCap));
    }
    UPV(tt.src_row, src_row); UPV(tt.probe_row, probe_row);
    return upload<TickTables>(h, &h->P.tabs, &tt, 1, TickTables{});
}

// the pre-run events in construction order and the prologue's state (hs_exact.hpp XInit / XState)
int apply_prologue(hs_engine *h, const StationPlan &p) {
    int rc;
    if (p.XI.per_lp) {
        UPV(h->XI.lp_src_slots, lp_src_slots); UPV(h->XI.sched_rank, sched_rank); UPV(h->XI.sched_entry, sched_entry);
    } else {
        UPV(h->XI.sched_rank, sched_rank); UPV(h->XI.src_lp, src_lp); UPV(h->XI.src_slot, src_slot); UPV(h->XI.probe_lp, probe_lp);
        UPV(h->XI.probe_slot, probe_slot); UPV(h->XI.sched_lp, sched_lp); UPV(h->XI.sched_entry, sched_entry);
    }
    if ((rc = alloc_zeroed(h, &h->XI.sched_idx, (size_t)p.n_sched))) return rc;
    h->P.sched_idx = h->XI.sched_idx;
    return alloc_xstate(h, p);
}

int apply_stations(hs_engine *h, const StationPlan &p) {
    const int n = h->cfg.n_lp;
    // ---- the plan's facts
    h->any_xsrc = p.any_xsrc; h->uni_stations = p.uni_stations; h->uni_grid = p.uni_grid; h->f64_times = p.f64_times;
    h->any_profile = p.any_profile; h->any_timevarying = p.any_timevarying; h->any_sched = p.any_sched; h->any_probe = p.any_probe;
    h->n_pass = p.n_pass; h->tandem_fan_in = p.tandem_fan_in; h->n_probe_slots = p.n_probe_slots; h->C = p.C;
    h->exact = p.exact; h->exact_prologue = p.exact_prologue; h->exact_only = p.exact_only; h->lazy_prologue = p.lazy_prologue;
    h->n_init = p.n_init; h->XI = p.XI;
    h->L.cap = p.log_cap; h->L.pcap = p.probe_cap; h->tab_cap = p.tab_cap; h->n_tab_rows = (int)p.rows.size();
    h->h_src_lp = p.src_lp; h->h_src_slot = p.src_slot;      // (setup_exact_plain: the single-heap machinery built on demand)
    h->h_stream_base = p.stream_base;                        // (hs_engine_set_network: the routers' and links' default streams)
    // ---- the stations' columns
    int rc;
    UPC(h->P.src_kind, cols.src_kind); UPC(h->P.src_rate, cols.src_rate); UPC(h->P.src_stop, cols.src_stop); UPC(h->P.conc, cols.conc);
    UPC(h->P.svc_kind, cols.svc_kind); UPC(h->P.svc_mean, cols.svc_mean); UPC(h->P.qcap, cols.qcap); UPC(h->P.egress, cols.egress);
    UPC(h->P.seed, cols.seed); UPV(h->P.stream_base, stream_base);
    UPV(h->P.prof_kind, prof_kind); UPV(h->P.prof_p, prof_p); UPV(h->P.probe_metric, probe_metric); UPV(h->P.probe_rate, probe_rate);
    h->P.tabs = nullptr;
    if (p.want_tabs && (rc = apply_tick_tables(h, p))) return rc;
    h->P.xsrc_kind = nullptr; h->P.xsrc_rate = nullptr; h->P.xsrc_stop = nullptr;
    if (p.any_xsrc) { UPV(h->P.xsrc_kind, xsrc_kind); UPV(h->P.xsrc_rate, xsrc_rate); UPV(h->P.xsrc_stop, xsrc_stop); }
    h->P.sched_off = nullptr; h->P.sched_t = nullptr;
    if (p.n_sched > 0) {
        if ((rc = upload<int64_t>(h, &h->P.sched_off, p.sched_off, (size_t)n + 1, 0))) return rc;
        if ((rc = upload<int64_t>(h, &h->P.sched_t, p.sched_time_ns, (size_t)p.n_sched, 0))) return rc;
    }
    h->P.tie_rank = nullptr;
    if (!p.tie_rank.empty()) UPV(h->P.tie_rank, tie_rank);
    h->P.sched_idx = nullptr;
    if (p.exact && (rc = apply_prologue(h, p))) return rc;
    // ---- the stations' state, the logs, the totals
    const size_t N = (size_t)n, NC = (size_t)n * (size_t)h->C, cap = (size_t)p.log_cap;
#define AL(field, count) DA(h->X.field, count)
    AL(A, N); AL(seqA, N); AL(crtA, N); AL(arr_k, N); AL(arr_time, N); AL(svc_k, N);
    AL(D, NC); AL(seqD, NC); AL(crtD, NC); AL(svc_s, NC); AL(crt, NC);
    AL(seq, N); AL(buf, N); AL(active, N);
    AL(generated, N); AL(accepted, N); AL(dropped, N); AL(completed, N); AL(rejected, N); AL(started, N);
    AL(received, N); AL(sink_w, N); AL(total_service, N); AL(q, N); AL(grp_time, N); AL(last_time, N);
    AL(events, N); AL(ev_kind, N * 11);
    AL(dpA, N); AL(rcA, N); AL(dpD, NC); AL(rcD, NC); AL(wkD, NC); AL(qdep, N * kQCap); AL(qrc, N * kQCap);   // lineage (hs_station.hpp)
    if (h->any_profile) {      // the general-path instantiation of the run kernel loads / stores the probe state of every LP
        AL(PA, N * kMaxProbes); AL(seqP, N * kMaxProbes); AL(crtP, N * kMaxProbes); AL(p_arr, N * kMaxProbes);
        AL(p_n, N * kMaxProbes); AL(ev_probe, N * 2); AL(sched_i, N); AL(rcP, N * kMaxProbes);
    }
    if (h->any_xsrc) {
        AL(XA, N * kMaxXSrc); AL(crtX, N * kMaxXSrc); AL(x_arr, N * kMaxXSrc); AL(x_n, N * kMaxXSrc); AL(seqX, N * kMaxXSrc);
        AL(x_k, N * kMaxXSrc); AL(dpX, N * kMaxXSrc); AL(rcX, N * kMaxXSrc);
    }
#undef AL
    if (h->any_probe) {
        DA(h->L.probe_t, N * (size_t)h->L.pcap * (size_t)h->n_probe_slots); DA(h->L.probe_v, N * (size_t)h->L.pcap * (size_t)h->n_probe_slots);
    }
    DA(h->L.adm, N * cap); DA(h->L.sink_t, N * cap);
    if (h->C > 1) DA(h->L.sink_created_own, N * cap);   // explicit created_at column: completions leave in a different order than admissions
    h->L.sink_created = (h->C > 1) ? h->L.sink_created_own : h->L.adm;
    if ((rc = alloc_zeroed(h, &h->tot, 1))) return rc;
    DA(h->cands, std::max<size_t>((size_t)h->n_blocks, (size_t)(n + 1) / 2));   // (the wide kernel: one per >= 2 LPs)
    if (p.wide) {
        if ((rc = alloc_zeroed(h, &h->wide_ctl, 1))) return rc;
        DA(h->wide_bail, (size_t)n); DA(h->wave_parts, ((size_t)n + 7) / 8);
    }
    // (the uploads and fills above went through the NULL stream; the engine's launches use a non-blocking stream, which does not
    //  wait for it: everything is in place before the caller can enqueue a run)
    HS_HIP(h, hipDeviceSynchronize());
    h->have_stations = true;
    return HS_OK;
}

// the link queues of hs_net_async and what goes with them
int apply_link_queues(hs_engine *h, const NetworkPlan &p) {
    const size_t n = (size_t)h->cfg.n_lp, NL = p.NL, NQ = NL * (size_t)p.aq_cap;
    int rc;
#define ALN(field, count) DA(h->NX.field, count)
    if (p.global) {
        // a shard: the link queues other ranks may write into while this rank's kernel runs (LIVE exchange) -- uncached device
        // memory, exportable with hipIpcGetMemHandle: a peer's stores arrive in HBM past this device's L2
        void *a = nullptr, *b = nullptr, *c = nullptr;
        if ((rc = uncached_alloc(h, &a, NQ * 4 * sizeof(int64_t)))) return rc;
        if ((rc = uncached_alloc(h, &b, NL * sizeof(unsigned long long)))) return rc;
        if ((rc = uncached_alloc(h, &c, NL * sizeof(int64_t)))) return rc;
        h->NX.aq_rec = (int64_t *)a; h->NX.aq_head = (unsigned long long *)b; h->NX.aq_ea = (int64_t *)c;
        HS_HIP(h, hipMemset(a, 0, NQ * 4 * sizeof(int64_t)));
        HS_HIP(h, hipMemset(b, 0, NL * sizeof(unsigned long long)));
        HS_HIP(h, hipMemset(c, 0, NL * sizeof(int64_t)));
        ALN(aq_tail, NL);
    } else {
        ALN(aq_rec, NQ * 4); ALN(aq_tail, NL); ALN(aq_head, NL); ALN(aq_ea, NL);
    }
    ALN(early_upto, n); ALN(d_pre, n);
#undef ALN
    return HS_OK;
}

#ifndef HS_NO_LOSS_TABLES
// table-decided losses (hs_network.link_drop_capacity): the bit tables, all clear, and the send log
int apply_loss_tables(hs_engine *h, const NetworkPlan &p) {
    int rc;
    LossTables lt{};
    uint32_t *bits = nullptr;
    UPV(lt.drop_off, drop_off);
    if ((rc = alloc_zeroed(h, &bits, (size_t)(p.drop_total / 32)))) return rc;
    lt.drop_bits = bits;
    h->drop_bits_dev = bits;
    DA(lt.send_log, (size_t)p.drop_total * 3);
    if ((rc = alloc_zeroed(h, &lt.send_log_n, 1))) return rc;
    lt.send_log_cap = p.drop_total;
    lt.overflow_word = &h->tot->overflow;
    h->loss_host = lt;
    return upload<LossTables>(h, &h->NP.loss_tables, &lt, 1, lt);
}
#endif

int apply_network(hs_engine *h, const NetworkPlan &p) {
    const int n = h->cfg.n_lp;
    // ---- the plan's facts
    h->window_ns = p.window_ns;
    h->drop_off_host = p.drop_off;
    h->net_global = p.global; h->n_global_lp = (int32_t)p.n_all; h->n_gid = p.n_gid;
    h->SC = ShardCtl{};
    h->SC.lp_base = p.lo;
    h->h_link_dst = p.link_dst; h->h_link_src = p.link_src; h->h_gid2local = p.gid2local;
    h->async_ok = p.async_ok; h->net_pf = p.net_pf; h->net_uni = p.net_uni;
    h->NP.n_links = p.nl;
    h->NX.bag_cap = p.bag_cap; h->NX.aq_cap = p.aq_cap; h->NX.aq_on = 0; h->NX.pk_base = h->cfg.start_ns;
    // ---- routers and links
    int rc;
    UPC(h->NP.egress, egress); UPV(h->NP.rt0, rt0); UPV(h->NP.rt1, rt1); UPV(h->NP.rt2, rt2); UPV(h->NP.rt3, rt3); UPV(h->NP.rt_cnt, rt_cnt);
    UPV(h->NP.link_of, link_of); UPV(h->NP.route_base, route_base);
    UPV(h->NP.link_dst, link_dst); UPV(h->NP.link_lat_min, lat_min); UPV(h->NP.link_jit_kind, jit_kind); UPV(h->NP.link_jit_mean, jit_mean);
    UPV(h->NP.link_base, link_base);
#ifndef HS_NO_LOSS_TABLES    // (scratch build: plan_network has refused a network that needs them)
    h->NP.loss_tables = nullptr;
    if (p.drop_total > 0 && (rc = apply_loss_tables(h, p))) return rc;
#endif
    UPV(h->NP.link_loss, loss); UPV(h->NP.in_off, in_off); UPV(h->NP.in_links, in_links); UPV(h->NP.link_lat_ns, lat_ns);
    h->NP.link_gid = nullptr;
    if (p.have_gid) {
        const int32_t *g2l_dev = nullptr;
        UPV(h->NP.link_gid, gid); UPV(g2l_dev, gid2local);
        h->gid2local = const_cast<int32_t *>(g2l_dev);
    }
    // ---- the network's state
    const size_t N = (size_t)n, NL = p.NL, NB = (size_t)n * (size_t)p.bag_cap;
#define ALN(field, count) DA(h->NX.field, count)
    ALN(route_k, N); ALN(routed, N); ALN(link_k, NL); ALN(link_in, NL); ALN(link_sent, NL); ALN(link_packets, NL); ALN(next_time, N);
    ALN(pend_pay, N);
    ALN(bag_cnt, N); ALN(bag_t, NB); ALN(bag_ts, NB); ALN(bag_cr, NB); ALN(bag_link, NB); ALN(bag_lin, NB);
    ALN(in_cnt, 2 * N); ALN(in_t, 2 * NB); ALN(in_ts, 2 * NB); ALN(in_cr, 2 * NB); ALN(in_link, 2 * NB); ALN(in_lin, 2 * NB);
#undef ALN
    DA(h->X.enqpay, N * (size_t)kEnqPay);    // hs_net_async's ENQ payloads (general path)
    if (p.nl > 0 && (rc = apply_link_queues(h, p))) return rc;
    if (!h->L.sink_created_own) DA(h->L.sink_created_own, N * (size_t)h->L.cap);   // not every completion reaches the Sink any more: explicit created_at column
    h->L.sink_created = h->L.sink_created_own;
#ifndef HS_LOGS_ROW_MAJOR   // (scratch build: the [cap][n_lp] logs the network engines had until round 5)
    h->L.lp_major = 1;          // an LP's records contiguous (hs_station.hpp RecordLogs::lp_major); nothing has been logged yet
#endif
    if (p.pool_want > 0) {      // (the single heap's list cells for a whole run: plan_net_paths)
        DA(h->xs_host.pnext, (size_t)p.pool_want); DA(h->xs_host.pidx, (size_t)p.pool_want);
        h->xs_host.pool_cap = p.pool_want;
    }
    HS_HIP(h, hipDeviceSynchronize());      // (null-stream uploads and fills, as in apply_stations)
    h->is_net = true;
    return HS_OK;
}
#undef DA
#undef UPV
#undef UPC

}  // namespace

extern "C" {

int hs_abi_version(void) { return HS_ABI_VERSION; }

int hs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *hs_last_error(const hs_engine *h) { return h ? h->error.c_str() : g_last_error.c_str(); }
const char *hs_last_global_error(void) { return g_last_error.c_str(); }

int hs_engine_create(const hs_config *cfg, hs_engine **out) {
    if (!cfg || !out) return fail(nullptr, HS_E_INVALID, "hs_engine_create: null argument");
    if (cfg->struct_size != sizeof(hs_config))
        return fail(nullptr, HS_E_INVALID, "hs_engine_create: hs_config size mismatch (ABI %d)", HS_ABI_VERSION);
    if (cfg->n_lp <= 0) return fail(nullptr, HS_E_INVALID, "hs_engine_create: n_lp must be > 0");
    if (cfg->mode != HS_MODE_SINGLE && cfg->mode != HS_MODE_REPLICAS)
        return fail(nullptr, HS_E_INVALID, "hs_engine_create: unknown mode %d", cfg->mode);
    if (cfg->horizon_ns < cfg->start_ns)
        return fail(nullptr, HS_E_INVALID, "hs_engine_create: horizon_ns precedes start_ns");
    if (cfg->start_ns < 0)      // (the Sinks' merged records and the packed link bounds hold non-negative times)
        return fail(nullptr, HS_E_UNSUPPORTED, "start_time %lld ns is negative: not lowered", (long long)cfg->start_ns);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, HS_E_INVALID, "device ordinal %d out of range (%d devices)", cfg->device, ndev);
    hs_engine *h = new (std::nothrow) hs_engine();
    if (!h) return fail(nullptr, HS_E_INVALID, "out of host memory");
    h->cfg = *cfg;
    hipError_t e = hipSetDevice(cfg->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_a);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_b);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_k0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_k1);
    if (e != hipSuccess) {
        int rc = fail(nullptr, HS_E_HIP, "device setup: %s", hipGetErrorString(e));
        delete h;
        return rc;
    }
    h->n_blocks = (cfg->n_lp + kBlock - 1) / kBlock;
    h->own_stream = h->stream;
    *out = h;
    return HS_OK;
}

int hs_engine_set_stations(hs_engine *h, const hs_stations *st) {
    if (!h || !st) return fail(h, HS_E_INVALID, "hs_engine_set_stations: null argument");
    if (h->have_stations) return fail(h, HS_E_STATE, "stations already set");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    StationPlan plan;
    std::string err;
    const int rc = plan_stations(h->cfg, *st, plan, err);
    if (rc) return fail(h, rc, "%s", err.c_str());       // (refused: the engine is as it was before the call)
    return apply_stations(h, plan);
}

int hs_engine_set_network(hs_engine *h, const hs_network *net) {
    if (!h || !net) return fail(h, HS_E_INVALID, "hs_engine_set_network: null argument");
    if (!h->have_stations) return fail(h, HS_E_STATE, "set stations before the network");
    if (h->is_net) return fail(h, HS_E_STATE, "network already set");
    if (h->initialised) return fail(h, HS_E_STATE, "set the network before the first run");
    if (h->cfg.mode != HS_MODE_SINGLE) return fail(h, HS_E_INVALID, "a network of stations is one Simulation: HS_MODE_SINGLE");
    if (h->C > 4) return fail(h, HS_E_UNSUPPORTED, "networked stations support concurrency <= 4 for now");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    { const int rcr = ensure_reset(h); if (rcr) return rcr; }     // (a bootstrap deferred for a station engine this no longer is)
    NetStationFacts sf;
    sf.C = h->C; sf.uni_stations = h->uni_stations; sf.f64_times = h->f64_times;
    sf.net_pf = h->any_probe || h->any_timevarying || h->any_sched || h->any_xsrc;
    sf.exact = h->exact; sf.pool_cap = h->xs_host.pool_cap; sf.log_cap = h->L.cap;
    sf.stream_base = h->h_stream_base.data();
    NetworkPlan plan;
    std::string err;
    const int rc = plan_network(h->cfg, sf, *net, plan, err);
    if (rc) return fail(h, rc, "%s", err.c_str());       // (refused: the engine is as it was before the call)
    return apply_network(h, plan);
}

int hs_engine_set_stream(hs_engine *h, void *hip_stream, int external) {
    if (!h) return fail(h, HS_E_INVALID, "null handle");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    // external != 0: run on the caller's stream; a NULL handle then means the device's default (null) stream,
    // which is what torch.cuda.current_stream().cuda_stream is unless the caller switched streams
    h->stream = external ? (hipStream_t)hip_stream : h->own_stream;
    h->external_stream = external != 0;
    return HS_OK;
}

int hs_engine_shard_attach(hs_engine *h, const hs_shard *sh) {
    if (!h || !sh) return fail(h, HS_E_INVALID, "hs_engine_shard_attach: null argument");
    if (!h->is_net || !h->net_global) return fail(h, HS_E_STATE, "set a network with n_global_lp > 0 before attaching the shard");
    if (h->initialised) return fail(h, HS_E_STATE, "attach the shard before the first run");
    if (sh->world < 1 || sh->rank < 0 || sh->rank >= sh->world || !sh->shard_lo)
        return fail(h, HS_E_INVALID, "bad rank / world / shard_lo");
    if (sh->shard_lo[sh->rank] != (int64_t)h->cfg.lp_base || sh->shard_lo[sh->rank + 1] != (int64_t)h->cfg.lp_base + h->cfg.n_lp)
        return fail(h, HS_E_INVALID, "shard_lo[rank] does not match this engine's [lp_base, lp_base + n_lp)");
    if (sh->shard_lo[0] != 0 || sh->shard_lo[sh->world] != h->n_global_lp)
        return fail(h, HS_E_INVALID, "shard_lo must cover [0, n_global_lp)");
    if (!sh->outbox_dev || !sh->inbox_dev || !sh->gvt_dev || !sh->cand_dev || sh->msg_capacity < 1)
        return fail(h, HS_E_INVALID, "exchange buffers are required");
    if (sh->window_ns < 1 || sh->window_ns > h->window_ns)
        return fail(h, HS_E_INVALID, "window_ns must be the minimum lookahead over ALL shards (got %lld, this shard's links allow %lld)",
                    (long long)sh->window_ns, (long long)h->window_ns);
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int nl = h->NP.n_links;
    std::vector<int32_t> lrank((size_t)(nl > 0 ? nl : 1), sh->rank);
    for (int l = 0; l < nl; ++l) {
        const int64_t d = h->h_link_dst[(size_t)l];
        int r = 0;
        while (r + 1 < sh->world && d >= sh->shard_lo[r + 1]) ++r;
        lrank[(size_t)l] = r;
    }
    int rc;
    if ((rc = upload<int32_t>(h, &h->SC.link_rank, lrank.data(), lrank.size(), 0))) return rc;
    if ((rc = dev_alloc(h, &h->SC.wend_slots, 2))) return rc;
    h->SC.gvt_in = sh->gvt_dev; h->SC.gvt_out = sh->gvt_dev;     // re-pointed per launch (parity)
    h->SC.outbox = sh->outbox_dev; h->SC.cand_out = sh->cand_dev;
    h->SC.msg_cap = sh->msg_capacity; h->SC.row = 1 + kMsgWords * sh->msg_capacity;
    h->SC.rank = sh->rank; h->SC.world = sh->world;
    h->SC.W = sh->window_ns;
    h->SC.lp_base = (int64_t)h->cfg.lp_base;
    h->inbox = sh->inbox_dev;
    h->window_ns = sh->window_ns;
    h->shard_gvt = sh->gvt_dev;
    return HS_OK;
}

// Sharded run, driven by the host one window at a time (all calls only enqueue work on the engine's stream):
//   begin;  for k = 0, 1, ...: window(k); <all-to-all outbox -> inbox>; inject(k); <all-reduce(min) gvt[k & 1]>;
//   every so often progress() (synchronises) until the returned window end reaches end_ns;
//   final(k); <all-gather cand>; overshoot(lp) on the winner.
int hs_engine_shard_begin(hs_engine *h, int64_t end_ns) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_begin: no shard attached");
    if (end_ns > h->cfg.horizon_ns) return fail(h, HS_E_INVALID, "end_ns beyond the configured horizon");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    int rc = do_reset_async(h);
    if (rc) return rc;
    rc = ensure_reset(h);
    if (rc) return rc;
    h->SC.end_ns = end_ns;
    const int64_t init_slots[2] = {h->cfg.start_ns - 1, h->cfg.start_ns - 1};
    const int64_t init_gvt[2] = {kInfNs, h->cfg.start_ns};       // window 0 reads gvt[1], accumulates into gvt[0]
    HS_HIP(h, hipMemcpyAsync(h->SC.wend_slots, init_slots, sizeof init_slots, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipMemcpyAsync(h->shard_gvt, init_gvt, sizeof init_gvt, hipMemcpyHostToDevice, h->stream));
    HS_HIP(h, hipMemsetAsync(h->SC.outbox, 0, (size_t)h->SC.world * h->SC.row * 8, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));                   // the host arrays above are stack memory
    h->launches = 1;
    h->net_ran = true;
    h->ipc_parity = 0;            // (every rank starts a run on the same half of the double-buffered exchange buffers)
    return HS_OK;
}

int hs_engine_shard_window(hs_engine *h, int64_t k) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_window: no shard attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    h->SC.gvt_in = h->shard_gvt + ((k + 1) & 1);
    h->SC.gvt_out = h->shard_gvt + (k & 1);
    launch_net_dispatch(h, 0, (int)(k & 0x3fffffff), h->flags & 1);
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

int hs_engine_shard_inject(hs_engine *h, int64_t k) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_inject: no shard attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int64_t items = (int64_t)h->SC.world * h->SC.msg_cap;
    const unsigned blocks = (unsigned)((items + 255) / 256);
    hipLaunchKernelGGL(hs_shard_inject, dim3(blocks ? blocks : 1), dim3(256), 0, h->stream, h->NX, h->inbox, h->SC.outbox,
                       h->SC.world, h->SC.msg_cap, h->SC.row, h->cfg.n_lp, h->SC.lp_base, (int)(k & 1), h->gid2local,
                       h->n_gid, h->shard_gvt + ((k + 1) & 1), h->tot);
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

int hs_engine_shard_progress(hs_engine *h, int64_t k_last, int64_t *wend_out) {
    if (!h || !h->SC.wend_slots || !wend_out) return fail(h, HS_E_STATE, "hs_engine_shard_progress: no shard attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipMemcpyAsync(wend_out, h->SC.wend_slots + (k_last & 1), 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    Totals t;
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    if (t.qoverflow) return fail(h, HS_E_UNSUPPORTED, "a same-timestamp event cascade exceeded the in-group queue");
    if (t.overflow & 4) return fail(h, HS_E_INVALID, "a message arrived for a station or link this shard does not own");
    if (t.overflow & 32) return fail(h, HS_E_OVERFLOW, "a link's loss table (hs_network.link_drop_capacity) is shorter than the packets that entered the link");
    if (t.overflow & 2) return fail(h, HS_E_OVERFLOW, "a message bag or an exchange row overflowed; raise bag_capacity / msg_capacity");
    if (t.overflow) return fail(h, HS_E_OVERFLOW, "a per-LP record log overflowed (capacity %lld records)", (long long)h->L.cap);
    return HS_OK;
}

// Asynchronous rounds instead of windows (same attach / begin / final / overshoot):
//   begin;  loop: round; <all-to-all outbox -> inbox>; <all-reduce(MAX) bounds>; inject_async;
//   every so often async_done() (synchronises) until no rank has work left;  final(0); <all-gather cand>; overshoot.
int hs_engine_shard_async_setup(hs_engine *h, int32_t n_cross, const int64_t *cross_gid, int64_t *bounds_dev,
                                int32_t max_iters) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_async_setup: no shard attached");
    if (n_cross < 0 || (n_cross > 0 && !cross_gid) || !bounds_dev || max_iters < 1)
        return fail(h, HS_E_INVALID, "hs_engine_shard_async_setup: bad argument");
    if (!h->NX.aq_tail) return fail(h, HS_E_STATE, "the network has no links");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    if (!ensure_async_fit(h)) return fail(h, HS_E_UNSUPPORTED, "the shard's stations are not co-resident on this device (asynchronous rounds need a cooperative launch)");
    if (h->cfg.horizon_ns - h->cfg.start_ns >= (int64_t)kPkNever - 2)
        return fail(h, HS_E_UNSUPPORTED, "asynchronous rounds hold 44 bits of nanoseconds per link bound (4.9 h of simulated time); use rounds = False");
    const int64_t lo = (int64_t)h->cfg.lp_base, hi = lo + h->cfg.n_lp;
    std::vector<int32_t> loc((size_t)(n_cross > 0 ? n_cross : 1), -1);
    std::vector<uint8_t> role((size_t)(n_cross > 0 ? n_cross : 1), 0);
    int out_here = 0;
    for (int i = 0; i < n_cross; ++i) {
        const int64_t g = cross_gid[i];
        if (g < 0 || g >= h->n_gid) return fail(h, HS_E_INVALID, "cross link id %lld out of range", (long long)g);
        const int l = h->h_gid2local[(size_t)g];
        if (l < 0) continue;
        loc[(size_t)i] = l;
        const bool s_here = h->h_link_src[(size_t)l] >= lo && h->h_link_src[(size_t)l] < hi;
        const bool d_here = h->h_link_dst[(size_t)l] >= lo && h->h_link_dst[(size_t)l] < hi;
        if (s_here && d_here) return fail(h, HS_E_INVALID, "link %lld does not cross a shard boundary", (long long)g);
        role[(size_t)i] = (uint8_t)((s_here ? 1 : 0) | (d_here ? 2 : 0));
        out_here += s_here ? 1 : 0;
    }
    // a round may append 2 x group_cap x iterations x C messages per outgoing cross link: to one outbox row on this side, to
    // one link queue on the other.  The iterations per round are clamped to what those hold.
    // (a group of a pre-sending station may append two: a departure that was not pre-sent + the next request's pre-send)
    const long long per_iter = 2ll * kAsyncGroupCap * h->C;
    long long fit = (h->NX.aq_cap / 2) / per_iter;
    if (out_here > 0) { const long long f2 = h->SC.msg_cap / (per_iter * out_here); if (f2 < fit) fit = f2; }
    if (fit < 1)
        return fail(h, HS_E_INVALID, "msg_capacity %d is too small for %d outgoing cross links x %lld messages per iteration; "
                    "raise msg_capacity", h->SC.msg_cap, out_here, per_iter);
    if (max_iters > fit) max_iters = (int32_t)fit;
    int rc;
    if ((rc = upload<int32_t>(h, &h->cross_local, loc.data(), loc.size(), -1))) return rc;
    if ((rc = upload<uint8_t>(h, &h->cross_role, role.data(), role.size(), 0))) return rc;
    h->n_cross = n_cross;
    h->cross_bounds = bounds_dev;
    h->round_iters_cfg = max_iters;
    h->shard_async = true;
    return HS_OK;
}

// ---- device-side exchange between asynchronous rounds (csrc/hs_kernels.hpp hs_shard_push) -----------------------------------
int hs_engine_shard_ipc_export(hs_engine *h, void *handles_out) {
    if (!h || !h->shard_async || !handles_out) return fail(h, HS_E_STATE, "hs_engine_shard_ipc_export: call hs_engine_shard_async_setup first");
    static_assert(sizeof(hipIpcMemHandle_t) == HS_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    if (!h->ipc_inbox) {
        const size_t nin = (size_t)2 * h->SC.world * h->SC.row, nb = (size_t)2 * h->SC.world * ((size_t)h->n_cross + 1);
        void *a = nullptr, *b = nullptr;
        // uncached: a peer's stores arrive in HBM past this device's L2, the readers use system-scope loads
        { const int rca = uncached_alloc(h, &a, nin * 8); if (rca) return rca; }
        { const int rcb = uncached_alloc(h, &b, nb * 8); if (rcb) return rcb; }
        HS_HIP(h, hipMemset(a, 0, nin * 8));
        {   // bounds start at "nothing known" (INT64_MIN), like the vector they replace
            std::vector<int64_t> init(nb, INT64_MIN);
            HS_HIP(h, hipMemcpy(b, init.data(), nb * 8, hipMemcpyHostToDevice));
        }
        HS_HIP(h, hipDeviceSynchronize());  // (the peers write into these from their own streams)
        h->ipc_inbox = (int64_t *)a; h->ipc_bounds = (int64_t *)b;
    }
    hipIpcMemHandle_t hh[2];
    HS_HIP(h, hipIpcGetMemHandle(&hh[0], h->ipc_inbox));
    HS_HIP(h, hipIpcGetMemHandle(&hh[1], h->ipc_bounds));
    memcpy(handles_out, hh, sizeof hh);
    return HS_OK;
}

int hs_engine_shard_ipc_attach(hs_engine *h, const void *all_handles) {
    if (!h || !h->ipc_inbox || !all_handles) return fail(h, HS_E_STATE, "hs_engine_shard_ipc_attach: call hs_engine_shard_ipc_export first");
    if (h->ipc_ready) return fail(h, HS_E_STATE, "hs_engine_shard_ipc_attach: already attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int world = h->SC.world;
    const hipIpcMemHandle_t *hh = (const hipIpcMemHandle_t *)all_handles;
    std::vector<int64_t *> pin((size_t)world), pbd((size_t)world);
    for (int r = 0; r < world; ++r) {
        if (r == h->SC.rank) { pin[(size_t)r] = h->ipc_inbox; pbd[(size_t)r] = h->ipc_bounds; continue; }
        void *a = nullptr, *b = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&a, hh[2 * r], hipIpcMemLazyEnablePeerAccess);
        if (e == hipSuccess) { h->ipc_opened.push_back(a); e = hipIpcOpenMemHandle(&b, hh[2 * r + 1], hipIpcMemLazyEnablePeerAccess); }
        if (e != hipSuccess) return fail(h, HS_E_HIP, "hipIpcOpenMemHandle (rank %d's exchange buffers): %s", r, hipGetErrorString(e));
        h->ipc_opened.push_back(b);
        pin[(size_t)r] = (int64_t *)a; pbd[(size_t)r] = (int64_t *)b;
    }
    return ipc_set_peers(h, pin, pbd);
}

int hs_engine_shard_peers_local(hs_engine *h, int64_t *const *inbox_ptrs, int64_t *const *bounds_ptrs) {
    if (!h || !h->ipc_inbox || !inbox_ptrs || !bounds_ptrs) return fail(h, HS_E_STATE, "hs_engine_shard_peers_local: call hs_engine_shard_ipc_export first");
    if (h->ipc_ready) return fail(h, HS_E_STATE, "hs_engine_shard_peers_local: already attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int world = h->SC.world;
    std::vector<int64_t *> pin(inbox_ptrs, inbox_ptrs + world), pbd(bounds_ptrs, bounds_ptrs + world);
    if (pin[(size_t)h->SC.rank] != h->ipc_inbox || pbd[(size_t)h->SC.rank] != h->ipc_bounds)
        return fail(h, HS_E_INVALID, "hs_engine_shard_peers_local: entry [rank] must be this engine's own buffers (hs_engine_shard_ipc_buffers)");
    return ipc_set_peers(h, pin, pbd);
}

int hs_engine_shard_ipc_buffers(hs_engine *h, int64_t **inbox_out, int64_t **bounds_out) {
    if (!h || !h->ipc_inbox || !inbox_out || !bounds_out) return fail(h, HS_E_STATE, "hs_engine_shard_ipc_buffers: call hs_engine_shard_ipc_export first");
    *inbox_out = h->ipc_inbox; *bounds_out = h->ipc_bounds;
    return HS_OK;
}

int hs_engine_shard_push(hs_engine *h) {
    if (!h || !h->ipc_ready) return fail(h, HS_E_STATE, "hs_engine_shard_push: call hs_engine_shard_ipc_attach first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(hs_shard_push, dim3((unsigned)h->SC.world), dim3(256), 0, h->stream, h->SC.outbox, h->SC.row, h->SC.msg_cap,
                       h->SC.world, h->SC.rank, h->ipc_parity, h->peer_inbox_dev, h->peer_bounds_dev, h->cross_bounds, h->n_cross, h->tot);
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

int hs_engine_shard_inject_ipc(hs_engine *h) {
    if (!h || !h->ipc_ready) return fail(h, HS_E_STATE, "hs_engine_shard_inject_ipc: call hs_engine_shard_ipc_attach first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(hs_shard_combine_bounds, dim3((unsigned)((h->n_cross + 1 + 255) / 256)), dim3(256), 0, h->stream, h->ipc_bounds,
                       h->SC.world, h->ipc_parity, h->n_cross, h->cross_bounds);
    hipLaunchKernelGGL(hs_shard_fetch_inbox, dim3((unsigned)h->SC.world), dim3(256), 0, h->stream, h->ipc_inbox, h->SC.world, h->ipc_parity,
                       h->SC.row, h->SC.msg_cap, const_cast<int64_t *>(h->inbox));
    HS_HIP(h, hipGetLastError());
    h->ipc_parity ^= 1;
    h->launches += 2;
    return hs_engine_shard_inject_async(h);
}

// ---- LIVE exchange (ShardCtl::live): no launch boundary per round ----------------------------------------------------------------
static int live_set_peers(hs_engine *h, const std::vector<int64_t *> &rec, const std::vector<int64_t *> &ea,
                          const std::vector<unsigned long long *> &head, const int32_t *peer_link) {
    const int world = h->SC.world;
    int rc;
    if ((rc = dev_alloc(h, &h->live_rec_dev, (size_t)world))) return rc;
    if ((rc = dev_alloc(h, &h->live_ea_dev, (size_t)world))) return rc;
    if ((rc = dev_alloc(h, &h->live_head_dev, (size_t)world))) return rc;
    HS_HIP(h, hipMemcpy(h->live_rec_dev, rec.data(), (size_t)world * sizeof(void *), hipMemcpyHostToDevice));
    HS_HIP(h, hipMemcpy(h->live_ea_dev, ea.data(), (size_t)world * sizeof(void *), hipMemcpyHostToDevice));
    HS_HIP(h, hipMemcpy(h->live_head_dev, head.data(), (size_t)world * sizeof(void *), hipMemcpyHostToDevice));
    const size_t NL = (size_t)(h->NP.n_links > 0 ? h->NP.n_links : 1);
    {
        const int32_t *pl = nullptr;
        if ((rc = upload<int32_t>(h, &pl, peer_link, NL, -1))) return rc;
        h->live_link_dev = const_cast<int32_t *>(pl);
    }
    // every link that leaves the shard needs a place in its destination's table
    const int64_t lo = (int64_t)h->cfg.lp_base, hi = lo + h->cfg.n_lp;
    for (int l = 0; l < h->NP.n_links; ++l) {
        const bool s_here = h->h_link_src[(size_t)l] >= lo && h->h_link_src[(size_t)l] < hi;
        const bool d_here = h->h_link_dst[(size_t)l] >= lo && h->h_link_dst[(size_t)l] < hi;
        if (s_here && !d_here && peer_link[l] < 0) return fail(h, HS_E_INVALID, "link %d leaves the shard but has no index at its destination rank", l);
    }
    if (!ensure_async_fit(h)) return fail(h, HS_E_UNSUPPORTED, "the shard's stations are not co-resident on this device");
    h->SC.peer_rec = h->live_rec_dev; h->SC.peer_ea = h->live_ea_dev; h->SC.peer_head = h->live_head_dev; h->SC.peer_link = h->live_link_dev;
    h->SC.live = 0;                       // (set for the duration of a live launch only: rounds and windows keep their outbox rows)
    h->live_ready = true;
    return HS_OK;
}

int hs_engine_shard_live_export(hs_engine *h, void *handles_out) {
    if (!h || !h->SC.wend_slots || !h->NX.aq_rec || !handles_out) return fail(h, HS_E_STATE, "hs_engine_shard_live_export: attach the shard first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    hipIpcMemHandle_t hh[3];
    HS_HIP(h, hipIpcGetMemHandle(&hh[0], h->NX.aq_rec));
    HS_HIP(h, hipIpcGetMemHandle(&hh[1], h->NX.aq_ea));
    HS_HIP(h, hipIpcGetMemHandle(&hh[2], h->NX.aq_head));
    memcpy(handles_out, hh, sizeof hh);
    return HS_OK;
}

int hs_engine_shard_live_attach(hs_engine *h, const void *all_handles, const int32_t *peer_link) {
    if (!h || !h->SC.wend_slots || !h->NX.aq_rec || !all_handles || !peer_link) return fail(h, HS_E_STATE, "hs_engine_shard_live_attach: attach the shard first");
    if (h->live_ready) return fail(h, HS_E_STATE, "hs_engine_shard_live_attach: already attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int world = h->SC.world;
    const hipIpcMemHandle_t *hh = (const hipIpcMemHandle_t *)all_handles;
    std::vector<int64_t *> rec((size_t)world), ea((size_t)world);
    std::vector<unsigned long long *> head((size_t)world);
    for (int r = 0; r < world; ++r) {
        if (r == h->SC.rank) { rec[(size_t)r] = h->NX.aq_rec; ea[(size_t)r] = h->NX.aq_ea; head[(size_t)r] = h->NX.aq_head; continue; }
        void *p[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < 3; ++k) {
            const hipError_t e = hipIpcOpenMemHandle(&p[k], hh[3 * r + k], hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) return fail(h, HS_E_HIP, "hipIpcOpenMemHandle (rank %d's link queues): %s", r, hipGetErrorString(e));
            h->ipc_opened.push_back(p[k]);
        }
        rec[(size_t)r] = (int64_t *)p[0]; ea[(size_t)r] = (int64_t *)p[1]; head[(size_t)r] = (unsigned long long *)p[2];
    }
    return live_set_peers(h, rec, ea, head, peer_link);
}

// enqueue the whole run of this rank (hs_engine_shard_begin set its end): ONE launch of the asynchronous engine, which exchanges
// messages and bounds with the other ranks' launches while it runs.  Every rank must have passed hs_engine_shard_begin (a barrier
// of the caller's) before any rank gets here.
int hs_engine_shard_live_run(hs_engine *h) {
    if (!h || !h->live_ready) return fail(h, HS_E_STATE, "hs_engine_shard_live_run: call hs_engine_shard_live_attach first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    if (!h->live_stream) {
        HS_HIP(h, hipStreamCreateWithFlags(&h->live_stream, hipStreamNonBlocking));
        HS_HIP(h, hipEventCreateWithFlags(&h->live_ev, hipEventDisableTiming));
    }
    // behind everything enqueued on the engine's stream so far (the reset), on a stream of its own: the launch waits for the peers'
    // launches, which -- shards of one process -- may sit on the very stream this engine shares with them
    HS_HIP(h, hipEventRecord(h->live_ev, h->stream));
    HS_HIP(h, hipStreamWaitEvent(h->live_stream, h->live_ev, 0));
    NetState NX = h->NX;
    NX.aq_on = 1;
    h->round_iters = 0;
    h->SC.live = 1;
    const int64_t end_ns = h->SC.end_ns;
    const hipStream_t keep = h->stream;
    h->stream = h->live_stream;
    const hipError_t e = h->C == 1 ? launch_async<1>(h, end_ns, NX) : h->C == 2 ? launch_async<2>(h, end_ns, NX) : launch_async<4>(h, end_ns, NX);
    h->stream = keep;
    h->SC.live = 0;
    if (e != hipSuccess) return fail(h, HS_E_HIP, "launch of the live asynchronous engine failed: %s", hipGetErrorString(e));
    h->launches += 1;
    return HS_OK;
}

int hs_engine_shard_live_wait(hs_engine *h) {
    if (!h || !h->live_ready) return fail(h, HS_E_STATE, "hs_engine_shard_live_wait: not attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    if (h->live_stream) HS_HIP(h, hipStreamSynchronize(h->live_stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    Totals t;
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    if (t.qoverflow) return fail(h, HS_E_UNSUPPORTED, "a same-timestamp event cascade exceeded the in-group queue");
    if (t.overflow & 8) return fail(h, HS_E_HIP, "the asynchronous engine gave up waiting for a neighbour (bounded spin exhausted): did every rank launch?");
    if (t.overflow & 32) return fail(h, HS_E_OVERFLOW, "a link's loss table (hs_network.link_drop_capacity) is shorter than the packets that entered the link");
    if (t.overflow & 2) return fail(h, HS_E_OVERFLOW, "a message bag or a link queue overflowed; raise bag_capacity");
    if (t.overflow) return fail(h, HS_E_OVERFLOW, "a per-LP record log overflowed (capacity %lld records)", (long long)h->L.cap);
    return HS_OK;
}

int hs_engine_shard_round(hs_engine *h) {
    if (!h || !h->shard_async) return fail(h, HS_E_STATE, "hs_engine_shard_round: call hs_engine_shard_async_setup first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    NetState NX = h->NX;
    NX.aq_on = 1;
    h->round_iters = h->round_iters_cfg;
    const int64_t end_ns = h->SC.end_ns;
    hipError_t e = h->C == 1 ? launch_async<1>(h, end_ns, NX) : h->C == 2 ? launch_async<2>(h, end_ns, NX) : launch_async<4>(h, end_ns, NX);
    h->round_iters = 0;
    if (e != hipSuccess) return fail(h, HS_E_HIP, "cooperative launch failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(hs_shard_bounds_out, dim3((unsigned)((h->n_cross + 1 + 255) / 256)), dim3(256), 0, h->stream, h->NX.aq_ea,
                       h->NX.pk_base, h->cross_local, h->cross_role, h->n_cross, h->cross_bounds, h->tot);
    HS_HIP(h, hipGetLastError());
    h->launches += 2;
    return HS_OK;
}

int hs_engine_shard_inject_async(hs_engine *h) {
    if (!h || !h->shard_async) return fail(h, HS_E_STATE, "hs_engine_shard_inject_async: call hs_engine_shard_async_setup first");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(hs_shard_inject_async, dim3(1), dim3(256), 0, h->stream, h->NX, h->inbox, h->SC.outbox, h->SC.world,
                       h->SC.msg_cap, h->SC.row, h->cfg.n_lp, h->SC.lp_base, h->gid2local, h->n_gid, h->cross_local,
                       h->cross_role, h->n_cross, h->cross_bounds, h->tot);
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

// synchronises; *any_not_done = the all-reduced "some rank still has work" flag of the last exchanged round
int hs_engine_shard_async_done(hs_engine *h, int32_t *any_not_done) {
    if (!h || !h->shard_async || !any_not_done) return fail(h, HS_E_STATE, "hs_engine_shard_async_done: not set up");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    int64_t v = 0;
    HS_HIP(h, hipMemcpyAsync(&v, h->cross_bounds + h->n_cross, 8, hipMemcpyDeviceToHost, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    *any_not_done = v != 0;
    Totals t;
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    if (t.qoverflow) return fail(h, HS_E_UNSUPPORTED, "a same-timestamp event cascade exceeded the in-group queue");
    if (t.overflow & 4) return fail(h, HS_E_INVALID, "a message arrived for a station or link this shard does not own");
    if (t.overflow & 8) return fail(h, HS_E_HIP, "the asynchronous engine gave up waiting for a neighbour (bounded spin exhausted)");
    if (t.overflow & 32) return fail(h, HS_E_OVERFLOW, "a link's loss table (hs_network.link_drop_capacity) is shorter than the packets that entered the link");
    if (t.overflow & 2) return fail(h, HS_E_OVERFLOW, "a message bag, a link queue or an exchange row overflowed; raise bag_capacity / msg_capacity");
    if (t.overflow) return fail(h, HS_E_OVERFLOW, "a per-LP record log overflowed (capacity %lld records)", (long long)h->L.cap);
    return HS_OK;
}

int hs_engine_shard_final(hs_engine *h, int64_t k) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_final: no shard attached");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    h->SC.gvt_in = h->shard_gvt + ((k + 1) & 1);
    h->SC.gvt_out = h->shard_gvt + (k & 1);
    launch_net_dispatch(h, h->SC.end_ns, (int)(k & 0x3fffffff), (h->flags & 1) | 2 | 4 | ((h->shard_async || h->live_ready) ? 8 : 0));
    HS_HIP(h, hipGetLastError());
    h->launches++;
    h->final_win = k;
    return HS_OK;
}

int hs_engine_shard_overshoot(hs_engine *h, int32_t lp) {
    if (!h || !h->SC.wend_slots) return fail(h, HS_E_STATE, "hs_engine_shard_overshoot: no shard attached");
    if (lp < 0 || lp >= h->cfg.n_lp) return fail(h, HS_E_INVALID, "LP index %d out of range", lp);
    HS_HIP(h, hipSetDevice(h->cfg.device));
    const int win = (int)(h->final_win & 0x3fffffff);
    switch (h->C) {
        case 1: hipLaunchKernelGGL(hs_shard_overshoot<1>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, h->NX, h->L, h->tot, h->cfg.n_lp, lp, win, h->SC); break;
        case 2: hipLaunchKernelGGL(hs_shard_overshoot<2>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, h->NX, h->L, h->tot, h->cfg.n_lp, lp, win, h->SC); break;
        default: hipLaunchKernelGGL(hs_shard_overshoot<4>, dim3(1), dim3(64), 0, h->stream, h->P, h->NP, h->X, h->NX, h->L, h->tot, h->cfg.n_lp, lp, win, h->SC); break;
    }
    HS_HIP(h, hipGetLastError());
    h->launches++;
    return HS_OK;
}

static int results_final(hs_engine *h);
int hs_engine_get_net_stats(hs_engine *h, const hs_net_stats *o) {
    if (!h || !o) return fail(h, HS_E_INVALID, "hs_engine_get_net_stats: null argument");
    if (!h->is_net) return fail(h, HS_E_STATE, "no network set");
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->cfg.n_lp, nl = (size_t)h->NP.n_links;
    if (o->routed) HS_HIP(h, hipMemcpy(o->routed, h->NX.routed, n * 8, hipMemcpyDeviceToHost));
    if (o->link_entered && nl) HS_HIP(h, hipMemcpy(o->link_entered, h->NX.link_in, nl * 8, hipMemcpyDeviceToHost));
    if (o->link_packets_sent && nl) HS_HIP(h, hipMemcpy(o->link_packets_sent, h->NX.link_packets, nl * 8, hipMemcpyDeviceToHost));
    if (o->link_packets_dropped && nl) {                     // entered - not lost
        std::vector<int64_t> in(nl), sent(nl);
        HS_HIP(h, hipMemcpy(in.data(), h->NX.link_in, nl * 8, hipMemcpyDeviceToHost));
        HS_HIP(h, hipMemcpy(sent.data(), h->NX.link_sent, nl * 8, hipMemcpyDeviceToHost));
        for (size_t l = 0; l < nl; ++l) o->link_packets_dropped[l] = in[l] - sent[l];
    }
    return HS_OK;
}

int hs_engine_set_link_drops(hs_engine *h, int32_t link, const uint32_t *bits, int64_t n_bits) {
    if (!h || !h->is_net) return fail(h, HS_E_STATE, "hs_engine_set_link_drops: no network set");
    if (link < 0 || link >= h->NP.n_links || !h->drop_bits_dev) return fail(h, HS_E_INVALID, "link %d has no loss table", (int)link);
    const int64_t b0 = h->drop_off_host[(size_t)link], cap = h->drop_off_host[(size_t)link + 1] - b0;
    if (cap <= 0) return fail(h, HS_E_INVALID, "link %d has no loss table", (int)link);
    if (n_bits < 0 || n_bits > cap || (n_bits > 0 && !bits)) return fail(h, HS_E_INVALID, "link %d: %lld bits for a table of %lld", (int)link, (long long)n_bits, (long long)cap);
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    HS_HIP(h, hipMemset(h->drop_bits_dev + b0 / 32, 0, (size_t)(cap / 32) * sizeof(uint32_t)));
    if (n_bits > 0) HS_HIP(h, hipMemcpy(h->drop_bits_dev + b0 / 32, bits, (size_t)((n_bits + 31) / 32) * sizeof(uint32_t), hipMemcpyHostToDevice));
    HS_HIP(h, hipDeviceSynchronize());
    return HS_OK;
}

int64_t hs_engine_read_send_log(hs_engine *h, int64_t *out_triples, int64_t capacity) {
    if (!h || !h->is_net) return fail(h, HS_E_STATE, "hs_engine_read_send_log: no network set");
    if (!h->loss_host.send_log_n) return 0;
    { const int rcf = results_final(h); if (rcf) return rcf; }
    unsigned long long n = 0;
    HS_HIP(h, hipMemcpy(&n, h->loss_host.send_log_n, sizeof n, hipMemcpyDeviceToHost));
    const int64_t have = (int64_t)(n < (unsigned long long)h->loss_host.send_log_cap ? n : (unsigned long long)h->loss_host.send_log_cap);
    const int64_t take = have < capacity ? have : capacity;
    if (take > 0 && out_triples) HS_HIP(h, hipMemcpy(out_triples, h->loss_host.send_log, (size_t)take * 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return (int64_t)n;
}

int hs_engine_reset(hs_engine *h) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "hs_engine_reset: stations not set");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    if (h->net_on_heap) { h->exact_only = false; h->net_on_heap = false; }      // (the next run starts on the parallel engines again)
    int rc = do_reset_async(h);
    if (rc) return rc;
    HS_HIP(h, hipStreamSynchronize(h->stream));
    return HS_OK;
}

// Windows over a network: what a run_until with a later end does.  0: repeat the run from the start; 1: continue from the state the
// last run left; 2: nothing moves.
static int net_window_state(hs_engine *h, int64_t end_ns, int &state, const Totals *seen) {
    state = 0;
    if (h->net_global || (h->flags & (1 << 24)) || h->NX.pend_pay == nullptr) return HS_OK;
    Totals t;
    int phase = h->xs_phase_seen;
    if (seen) t = *seen;
    else {
        HS_HIP(h, hipStreamSynchronize(h->stream));
        HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
        if (h->exact && h->xs && !h->XI.per_lp) HS_HIP(h, hipMemcpy(&phase, &h->xs->phase, sizeof phase, hipMemcpyDeviceToHost));
    }
    // An engine with a prologue (hs_exact.hpp) continues while the prologue is skipped (lazy_prologue: a hazard repeats ALL windows
    // behind it, prologue_fallback) or once it has handed over to the parallel engines (phase 2: its launches are no-ops from then on);
    // in between -- the single lane still holds the heap at a window end -- the run is repeated
    if (h->exact && !lazy_active(h) && phase != 2) return HS_OK;
    // (undecided bit 2 -- a pre-run root beside another root of its nanosecond -- only matters while the prologue is skipped)
    const int und = lazy_active(h) ? t.undecided : (t.undecided & ~4);
    if (t.overflow != 0 || t.qoverflow != 0 || und != 0 || t.no_resume != 0) return HS_OK;
    state = t.cur_time > end_ns ? 2 : 1;
    return HS_OK;
}

int hs_engine_run_until_async(hs_engine *h, int64_t end_ns) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "hs_engine_run_until: stations not set");
    if (end_ns > h->cfg.horizon_ns)
        return fail(h, HS_E_INVALID, "end_ns %lld beyond the configured horizon %lld", (long long)end_ns,
                    (long long)h->cfg.horizon_ns);
    HS_HIP(h, hipSetDevice(h->cfg.device));
    h->launches = 0;
    h->run_path = 0;
    const bool seen_valid = h->tot_seen_valid && !h->pending_async;
    h->tot_seen_valid = false;
    h->net_resume = false;
    HS_HIP(h, hipEventRecord(h->ev_a, h->stream));
    if (!h->initialised) { int rc = do_reset_async(h); if (rc) return rc; h->launches++; }
    HS_HIP(h, hipEventRecord(h->ev_k0, h->stream));
    if (h->is_net) {
        if (h->net_global) return fail(h, HS_E_STATE, "a shard of a partitioned network is driven with hs_engine_shard_*");
        h->net_window_path = 0;
        if (h->exact_only) {
            // the single-heap loop (hs_exact.hpp, no hand-over) holds the whole network since an election its lineage key did not
            // decide (tandem_fallback): `_execute_until` again is that loop again -- the heap keeps every pending event
            h->window_ends.push_back(end_ns);
            if (end_ns > h->net_last_end) h->net_last_end = end_ns;
            h->net_window_path = 1;
            int rc = launch_prologue(h, end_ns);
            if (rc) return rc;
            h->net_ran = true;
            HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
            HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
            h->pending_async = true;
            return HS_OK;
        }
        if (h->net_ran) {
            // Windows over a network (core/simulation.py:527-541 `_run_window` = `_execute_until` again).  The reference pops events in
            // one global order whatever the window ends are, and every call stops behind the first event beyond its end -- so after
            // windows e_1 <= ... <= e_k the state is that of ONE run to e_k.  An end at or before the last one moves nothing: the
            // reference's loop condition `current_time <= end` is already false (the event beyond the earlier end was processed).
            if (end_ns <= h->net_last_end) {
                h->net_window_path = 2;
                HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
                HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
                h->pending_async = true;
                return HS_OK;
            }
            // Round 6: a later end CONTINUES from the state the last run left -- every station's rows, the bags (the final launch took
            // the link queues' leftovers into them), the links' bounds (lower bounds whatever the end was: NetStation::pre_send) and
            // the group the election stopped inside (hs_net_resume) -- O(window) as the reference's `_run_window`, not O(prefix).
            // Not for shards; a prologue that still holds the single-lane heap (net_window_state), a state the asynchronous kernel
            // cannot take back (a bag larger than its LDS column, an overflow) and debug flag 1 << 24 repeat the run from the start
            // as rounds 4-5 did.
            int state = 0;
            { const int rc = net_window_state(h, end_ns, state, seen_valid ? &h->tot_seen : nullptr); if (rc) return rc; }
            h->net_window_path = state == 0 ? 3 : state;
            if (state == 2) {            // the event beyond the last end lies beyond this one too: `current_time <= end` is false
                h->net_last_end = end_ns;
                HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
                HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
                h->pending_async = true;
                return HS_OK;
            }
            if (state == 1) { h->net_resume = true; h->net_resume_from = h->net_last_end; }
            else {
                int rc = do_reset_async(h);
                if (rc) return rc;
                h->launches++;
            }
        }
        h->net_last_end = end_ns;
        if (h->exact) h->window_ends.push_back(end_ns);       // (a skipped prologue's hazards and an undecided election repeat the run)
        int rc = launch_prologue(h, end_ns);
        if (rc) return rc;
        rc = run_net_async(h, end_ns);
        h->net_resume = false;
        if (rc) return rc;
    } else {
        if (h->n_pass > 0 && ((h->flags & (1 << 17)) || ((h->flags & (1 << 16)) && h->exact_prologue)) && h->exact && h->window_ends.empty())
            h->exact_only = true;   // debug: single heap from the start (1 << 16: wherever a prologue exists -- with tandem queues that is this loop)
        if (h->n_pass > 0 || lazy_active(h) || ((h->any_xsrc || h->any_sched) && h->exact)) h->window_ends.push_back(end_ns);
        int rc = launch_prologue(h, end_ns);
        if (rc) return rc;
        rc = launch_run_dispatch(h, end_ns);
        if (rc) return rc;
        HS_HIP(h, hipGetLastError());
        h->launches++;
    }
    HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
    HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
    h->pending_async = true;
    return HS_OK;
}

// A station engine that skipped the prologue (lazy_prologue): did the run meet what only the prologue orders exactly?
static bool lazy_hazard(hs_engine *h, bool &hazard) {
    Totals t;
    if (hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost) != hipSuccess) return false;
    unsigned long long total = 0;
    for (int k = 0; k < HS_EV_KINDS; ++k) total += t.ev[k];
    // (the election of the event beyond end_ns ranks a pre-run event first: true once the run has created n_init events)
    hazard = (t.undecided & 4) != 0 || total < 2ull * (unsigned long long)h->n_init;
    return true;
}
// The single-heap machinery (hs_exact.hpp) for an engine whose model has no pre-run events beyond its Sources' first ticks -- built
// on demand, the first time an election needs the reference's sort-index ledger (tandem_fallback).  Mirrors the HS_MODE_SINGLE block
// of hs_engine_set_stations with no Probes and no scheduled Requests.
int setup_exact_plain(hs_engine *h) {
    const int n = h->cfg.n_lp;
    int rc;
    const int32_t zero32 = 0; const uint8_t zero8 = 0; const int64_t zero64 = 0;
    if ((rc = upload<int32_t>(h, &h->XI.src_lp, h->h_src_lp.data(), h->h_src_lp.size(), 0))) return rc;
    if ((rc = upload<uint8_t>(h, &h->XI.src_slot, h->h_src_slot.data(), h->h_src_slot.size(), 0))) return rc;
    if ((rc = upload<int32_t>(h, &h->XI.probe_lp, &zero32, 0, 0))) return rc;
    if ((rc = upload<uint8_t>(h, &h->XI.probe_slot, &zero8, 0, 0))) return rc;
    if ((rc = upload<int32_t>(h, &h->XI.sched_lp, &zero32, 0, 0))) return rc;
    if ((rc = upload<int64_t>(h, &h->XI.sched_entry, &zero64, 0, 0))) return rc;
    if ((rc = upload<int64_t>(h, &h->XI.sched_rank, &zero64, 0, 0))) return rc;
    h->XI.n_src = (int32_t)h->h_src_lp.size(); h->XI.n_probe = 0; h->XI.n_sched = 0; h->XI.per_lp = 0;
    if ((rc = dev_alloc(h, &h->XI.sched_idx, (size_t)1))) return rc;
    HS_HIP(h, hipMemset(h->XI.sched_idx, 0, sizeof(uint32_t)));
    const int64_t n_init = (int64_t)h->h_src_lp.size();
    h->n_init = n_init;
    h->xs_host = XState{};
    h->xs_host.heap_cap = n_init + (int64_t)n * (h->C + 16) + 1024;
    h->xs_host.pool_cap = std::min<int64_t>(2 * n_init + 16 * (int64_t)n + 1024 + (int64_t)n * h->L.cap, (int64_t)1 << 28);
    if ((rc = dev_alloc(h, &h->xs_host.heap, (size_t)h->xs_host.heap_cap))) return rc;
    if ((rc = dev_alloc(h, &h->xs_host.qhead, (size_t)n))) return rc;
    if ((rc = dev_alloc(h, &h->xs_host.qtail, (size_t)n))) return rc;
    if ((rc = dev_alloc(h, &h->xs_host.pnext, (size_t)h->xs_host.pool_cap))) return rc;
    if ((rc = dev_alloc(h, &h->xs_host.pidx, (size_t)h->xs_host.pool_cap))) return rc;
    if ((rc = dev_alloc(h, &h->xs_host.init_t, (size_t)std::max<int64_t>(n_init, 1)))) return rc;
    if ((rc = dev_alloc(h, &h->xs, 1))) return rc;
    HS_HIP(h, hipDeviceSynchronize());
    h->exact = true;
    return HS_OK;
}

constexpr unsigned long long kSingleHeapReplayMax = 4000000ull;   // events a network's undecided election may cost on the single lane (~2 us each)
// Tandem queues: the passes met an order between two LPs' events that their lineage key does not decide (Totals::undecided).
// The run since the last reset is repeated, window by window, on the single-heap loop -- the reference's own algorithm.
int tandem_fallback(hs_engine *h) {
    // (also engines with several Sources per Server whose election rested on a departure's construction rank: set_stations)
    // (round 6: and station NETWORKS held by one engine whose election of the one event beyond end_time rested on a stand-in rank --
    //  hs_net_window's tie check: until now refused by name; the single heap IS the reference's sort-index ledger)
    const bool net_election = h->is_net && !h->net_global && h->cfg.mode == HS_MODE_SINGLE;
    const bool station_election = (h->any_xsrc || h->any_sched) && !h->is_net && h->cfg.mode == HS_MODE_SINGLE;
    if ((h->n_pass == 0 && !station_election && !net_election) || h->exact_only) return HS_OK;
    if (!h->exact && !net_election) return HS_OK;
    int und = 0;
    HS_HIP(h, hipMemcpy(&und, &h->tot->undecided, sizeof und, hipMemcpyDeviceToHost));
    if (h->n_pass == 0) {                     // several Sources per Server, no tandem queues: only the election's tie (value 2) moves the
        und &= 2;                             // run to the single heap; a skipped prologue's hazards (value 4) are prologue_fallback's
        if (!und) return HS_OK;
    }
    if (net_election && und) {
        // one lane replays the whole run: only while that is seconds (lock-step constants live in small models); beyond it the run
        // stays refused by name (hs_engine_run_until)
        Totals t;
        HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
        unsigned long long total = 0;
        for (int k = 0; k < HS_EV_KINDS; ++k) total += t.ev[k];
        if (total > kSingleHeapReplayMax) return HS_OK;
        if (!h->exact) {                       // a model without Probes / scheduled Requests / further Sources: no machinery yet
            if (h->net_last_end == INT64_MIN) return HS_OK;
            h->window_ends.assign(1, h->net_last_end);      // (plain networks keep no list of ends: the state is that of ONE run to the last one)
            const int rcx = setup_exact_plain(h);
            if (rcx) return rcx;
        }
    }
    if (!und && lazy_active(h)) {             // (pre-run events next to tandem queues: lazy_prologue's short-run rule)
        bool hazard = false;
        if (!lazy_hazard(h, hazard)) return fail(h, HS_E_HIP, "reading the totals failed");
        und = hazard ? 4 : 0;
    }
    if (!und) return HS_OK;
    if (h->window_ends.empty()) return HS_OK;     // (nothing ran since the last reset: no run to repeat -- ADVICE r4)
    const std::vector<int64_t> ends = h->window_ends;
    h->exact_only = true;
    h->net_on_heap = net_election;
    int rc = do_reset_async(h);
    if (rc) return rc;
    h->window_ends = ends;
    for (int64_t e : ends) {
        rc = launch_prologue(h, e);
        if (rc) return rc;
    }
    HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
    HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    return HS_OK;
}

int prologue_fallback(hs_engine *h) {
    if (!lazy_active(h) || h->window_ends.empty()) return HS_OK;
    bool hazard = false;
    if (!lazy_hazard(h, hazard)) return fail(h, HS_E_HIP, "reading the totals failed");
    if (!hazard) return HS_OK;
    const std::vector<int64_t> ends = h->window_ends;
    h->lazy_failed = true;
    int rc = do_reset_async(h);
    if (rc) return rc;
    int64_t prev = INT64_MIN;
    for (int64_t e : ends) {
        rc = launch_prologue(h, e);
        if (rc) return rc;
        if (h->is_net) {
            // (round 6: the windows of a network continue from one another -- hs_engine_run_until_async -- so does their repetition)
            if (prev != INT64_MIN) { h->net_resume = true; h->net_resume_from = prev; }
            rc = run_net_async(h, e);
            h->net_resume = false;
            if (rc) return rc;
        }
        else { rc = launch_run_dispatch(h, e); if (rc) return rc; h->launches++; }
        HS_HIP(h, hipGetLastError());
        prev = e;
    }
    // the reset above forgot the network's last window end; an earlier or equal end after this moves nothing
    if (h->is_net) h->net_last_end = ends.back();
    HS_HIP(h, hipEventRecord(h->ev_k1, h->stream));
    HS_HIP(h, hipEventRecord(h->ev_b, h->stream));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    return HS_OK;
}

int hs_engine_prologue_path(const hs_engine *h) {
    if (!h || !h->exact || (!h->exact_prologue && !h->exact_only)) return 0;
    return lazy_active(h) ? 1 : 2;
}
int hs_engine_window_path(const hs_engine *h) { return h ? h->net_window_path : 0; }
int hs_engine_tandem_path(const hs_engine *h) { return !h || h->n_pass == 0 ? 0 : h->exact_only ? 2 : 1; }
int hs_engine_run_path(const hs_engine *h) { return !h ? 0 : h->run_path | (h->f64_times ? HS_RUN_F64_TIMES : 0); }

int hs_engine_synchronize(hs_engine *h) {
    if (!h) return fail(h, HS_E_INVALID, "null handle");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    { int rc = tandem_fallback(h); if (rc) return rc; }
    { int rc = prologue_fallback(h); if (rc) return rc; }
    h->pending_async = false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev_a, h->ev_b) == hipSuccess) h->last_run_ms = ms;
    if (hipEventElapsedTime(&ms, h->ev_k0, h->ev_k1) == hipSuccess) h->last_kernel_ms = ms;
    return HS_OK;
}

// Every getter goes through here: a run enqueued with hs_engine_run_until_async is FINAL only behind hs_engine_synchronize -- that is
// where a run that skipped the prologue, or tandem passes that met an undecided tie, are repeated on the single heap (ADVICE r3:
// a getter that merely waited for the stream returned the results of the skipped path).
static int results_final(hs_engine *h) {
    { const int rcr = ensure_reset(h); if (rcr) return rcr; }      // (a reset whose bootstrap was deferred into a run that never came)
    if (h->pending_async) return hs_engine_synchronize(h);
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, HS_E_HIP, "device synchronisation failed");
    return HS_OK;
}

int hs_engine_run_until(hs_engine *h, int64_t end_ns) {
    int rc = hs_engine_run_until_async(h, end_ns);
    if (rc) return rc;
    rc = hs_engine_synchronize(h);
    if (rc) return rc;
    Totals t;
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    h->tot_seen = t; h->tot_seen_valid = h->is_net;
    if (h->is_net && h->exact && h->xs && !h->XI.per_lp) HS_HIP(h, hipMemcpy(&h->xs_phase_seen, &h->xs->phase, sizeof(int), hipMemcpyDeviceToHost));
    if (h->n_tab_rows > 0) {
        unsigned long long st[2] = {0ull, 0ull};
        HS_HIP(h, hipMemcpy(st, h->tab_status, sizeof st, hipMemcpyDeviceToHost));
        if (st[0] != 0ull)
            return fail(h, HS_E_UNSUPPORTED, "LP %lld: one arrival of its time-varying Source needs more than 64 x %lld adaptive-Simpson "
                        "intervals (the reference's own integrator needs minutes for such an arrival; hs_engine_set_profile_budget "
                        "raises the limit, tools/profile_cost.py shows the cost) -- refused instead of stalling the device",
                        (long long)st[0] - 2, (long long)h->lane_budget);
        if (st[1] != 0ull)
            return fail(h, HS_E_OVERFLOW, "LP %lld: the tick table of its Source / Probe overflowed (capacity %lld ticks); raise log_capacity",
                        (long long)st[1] - 2, (long long)h->tab_cap);
    }
    if (t.qoverflow) return fail(h, HS_E_UNSUPPORTED, "a same-timestamp event cascade exceeded the in-group queue");
    if (h->is_net && (t.undecided & 2))
        return fail(h, HS_E_UNSUPPORTED, "the one event beyond end_time is a lock-step tie between two stations (same time, creation time and "
                    "lineage) that only the reference's sort-index ledger decides, and one of the two is a departure, a message or an injected "
                    "Request, whose construction rank the network engines do not carry: refused instead of guessing (constant arrivals, "
                    "services and link latencies in lock step; a different end_time or seed-free jitter avoids it; runs of up to "
                    "4 000 000 events are repeated on the single-heap loop and answered instead)");
    if (t.overflow & 16)
        return fail(h, HS_E_OVERFLOW, "the prologue (csrc/hs_exact.hpp) ran out of heap / payload-pool space");
    if (t.overflow & 8)
        return fail(h, HS_E_HIP, "the asynchronous network engine gave up waiting for a neighbour (bounded spin); "
                                 "set debug flag 16 to use the windowed engine");
    if (t.overflow & 32) return fail(h, HS_E_OVERFLOW, "a link's loss table (hs_network.link_drop_capacity) is shorter than the packets that entered the link");
    if (t.overflow & 2)
        return fail(h, HS_E_OVERFLOW, "a station's in-flight message bag overflowed (capacity %d); raise bag_capacity",
                    (int)h->NX.bag_cap);
    if (t.overflow)
        return fail(h, HS_E_OVERFLOW, "a per-LP record log overflowed (capacity %lld records)", (long long)h->L.cap);
    return HS_OK;
}

int hs_engine_bench_runs(hs_engine *h, int64_t end_ns, int32_t repeats, float *kernel_ms_out, float *total_ms_out) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "hs_engine_bench_runs: stations not set");
    if (repeats <= 0) return fail(h, HS_E_INVALID, "repeats must be > 0");
    HS_HIP(h, hipSetDevice(h->cfg.device));
    h->run_path = 0;
    std::vector<hipEvent_t> ev((size_t)repeats * 2 + 2);
    for (auto &e : ev) HS_HIP(h, hipEventCreate(&e));
    // Round 6: the kernel duration is SAMPLED on every eighth repeat instead of bracketed on every one.  An event pair is two barrier
    // packets on the stream; around a 90 us step (the strong shard) they were 13.7 us of every step the caller's clock saw (measured:
    // 0.1078 against 0.0941 ms per step).  A repeat without a pair reports the latest sample.  HS_BENCH_STEP_EVENTS=1 brackets every
    // repeat as before, =0 none (every repeat then reports the batch average).
    static const int step_events_mode = []() { const char *e = getenv("HS_BENCH_STEP_EVENTS"); return e ? (e[0] == '0' ? 0 : 1) : 2; }();
    auto step_events_at = [&](int r) { return step_events_mode == 1 || (step_events_mode == 2 && (r & 7) == 0); };
    for (int attempt = 0; attempt < 2; ++attempt) {
        HS_HIP(h, hipEventRecord(ev[(size_t)repeats * 2], h->stream));
        for (int r = 0; r < repeats; ++r) {
            int rc = do_reset_async(h);
            if (rc) return rc;
            if (step_events_at(r)) HS_HIP(h, hipEventRecord(ev[(size_t)2 * r], h->stream));
            { int rc1 = launch_prologue(h, end_ns); if (rc1) return rc1; }
            if (h->is_net) { h->launches = 0; int rc2 = run_net_async(h, end_ns); if (rc2) return rc2; }
            else { const int rc2 = launch_run_dispatch(h, end_ns); if (rc2) return rc2; }
            HS_HIP(h, hipGetLastError());
            if (step_events_at(r)) HS_HIP(h, hipEventRecord(ev[(size_t)2 * r + 1], h->stream));
        }
        HS_HIP(h, hipEventRecord(ev[(size_t)repeats * 2 + 1], h->stream));
        HS_HIP(h, hipStreamSynchronize(h->stream));
        if (!lazy_active(h)) break;          // (lazy_prologue: a run that needs the prologue is timed with it)
        bool hazard = false;
        if (!lazy_hazard(h, hazard)) return fail(h, HS_E_HIP, "reading the totals failed");
        if (!hazard) break;
        h->lazy_failed = true;
    }
    float tot_ms = 0.f;
    HS_HIP(h, hipEventElapsedTime(&tot_ms, ev[(size_t)repeats * 2], ev[(size_t)repeats * 2 + 1]));
    float sample_ms = tot_ms / (float)repeats;
    for (int r = 0; r < repeats; ++r) {
        if (step_events_at(r)) HS_HIP(h, hipEventElapsedTime(&sample_ms, ev[(size_t)2 * r], ev[(size_t)2 * r + 1]));
        if (kernel_ms_out) kernel_ms_out[r] = sample_ms;
        h->last_kernel_ms = sample_ms;
    }
    if (total_ms_out) *total_ms_out = tot_ms;
    h->last_run_ms = tot_ms / (float)repeats;
    if (!h->is_net) h->launches = 2;
    for (auto &e : ev) hipEventDestroy(e);
    Totals t;                                                       // a timed run that overflowed is not a result
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    if ((h->n_pass > 0 || h->any_xsrc || h->any_sched) && !h->is_net && !h->exact_only && (t.undecided & 3))
        return fail(h, HS_E_UNSUPPORTED, "tandem queues / several Sources per Server: this configuration needs the single-heap path (lock-step ties); hs_engine_run_until "
                                         "switches to it, hs_engine_bench_runs does not");
    if (t.qoverflow) return fail(h, HS_E_UNSUPPORTED, "a same-timestamp event cascade exceeded the in-group queue");
    if (t.overflow & 8) return fail(h, HS_E_HIP, "the asynchronous network engine gave up waiting for a neighbour (bounded spin)");
    if (t.overflow & 32) return fail(h, HS_E_OVERFLOW, "a link's loss table (hs_network.link_drop_capacity) is shorter than the packets that entered the link");
    if (t.overflow & 2) return fail(h, HS_E_OVERFLOW, "a station's in-flight message bag overflowed (capacity %d); raise bag_capacity", (int)h->NX.bag_cap);
    if (t.overflow) return fail(h, HS_E_OVERFLOW, "a per-LP record log overflowed (capacity %lld records)", (long long)h->L.cap);
    return HS_OK;
}

int hs_engine_set_profile_budget(hs_engine *h, int64_t intervals_per_lane) {
    if (!h) return fail(h, HS_E_INVALID, "hs_engine_set_profile_budget: null handle");
    if (intervals_per_lane < 1) return fail(h, HS_E_INVALID, "hs_engine_set_profile_budget: the budget must be >= 1");
    h->lane_budget = (long long)intervals_per_lane;
    h->tables_built = false;       // the next reset produces the tables again
    return HS_OK;
}

int hs_engine_get_summary(hs_engine *h, hs_summary *out) {
    if (!h || !out) return fail(h, HS_E_INVALID, "hs_engine_get_summary: null argument");
    if (!h->have_stations) return fail(h, HS_E_STATE, "stations not set");
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    Totals t;
    HS_HIP(h, hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    int64_t total = 0;
    for (int k = 0; k < HS_EV_KINDS; ++k) { out->events_by_kind[k] = (int64_t)t.ev[k]; total += (int64_t)t.ev[k]; }
    out->events_processed = total;
    out->events_cancelled = 0;
    out->final_time_ns = (h->cfg.mode == HS_MODE_SINGLE) ? t.cur_time : t.final_time;
    out->requests_completed = (int64_t)t.completed;
    out->sink_records = (int64_t)t.received;
    out->last_run_ms = h->last_run_ms;
    out->kernel_ms = h->last_kernel_ms;
    out->launches = h->launches;
    out->window_ns = h->window_ns;
    out->overflow = t.overflow;
    return HS_OK;
}

int hs_engine_get_lp_stats(hs_engine *h, const hs_lp_stats *o) {
    if (!h || !o) return fail(h, HS_E_INVALID, "hs_engine_get_lp_stats: null argument");
    if (!h->have_stations) return fail(h, HS_E_STATE, "stations not set");
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    const size_t n = (size_t)h->cfg.n_lp;
#define DL(dst, src, T) if (o->dst) HS_HIP(h, hipMemcpy(o->dst, h->X.src, n * sizeof(T), hipMemcpyDeviceToHost))
    DL(generated, generated, int64_t); DL(accepted, accepted, int64_t); DL(dropped, dropped, int64_t);
    DL(completed, completed, int64_t); DL(rejected, rejected, int64_t); DL(total_service_s, total_service, double);
    DL(sink_received, received, int64_t); DL(queue_depth, buf, int64_t); DL(active, active, int32_t);
    DL(events, events, int64_t); DL(final_time_ns, last_time, int64_t);
#undef DL
    return HS_OK;
}

// C == 1 reads created_at from the admission log, where the entries of Requests the worker rejected stay in place, marked
// (hs_station.hpp log_time): the m-th Sink record's created_at is the m-th UNMARKED entry.  `created` holds the first `cnt` entries
// of LP `lp`'s log; with `rej` rejected Requests the records lie within the first cnt + rej.
static int skip_rejected_admissions(hs_engine *h, int32_t lp, int64_t cnt, int64_t rej, int64_t *created) {
    int64_t want = cnt + rej;
    if (want > h->L.cap) want = h->L.cap;
    int64_t *tmp = nullptr;
    if (hipMalloc(&tmp, (size_t)want * 8) != hipSuccess) return fail(h, HS_E_HIP, "hipMalloc of the read-back staging buffer failed");
    std::vector<int64_t> all((size_t)want);
    hipLaunchKernelGGL(hs_gather_one, dim3((unsigned)((want + 255) / 256)), dim3(256), 0, h->stream, h->L.adm, tmp, h->cfg.n_lp, lp, want,
                       h->L.lp_major ? h->L.cap : (int64_t)0);
    const bool ok = hipStreamSynchronize(h->stream) == hipSuccess &&
                    hipMemcpy(all.data(), tmp, (size_t)want * 8, hipMemcpyDeviceToHost) == hipSuccess;
    hipFree(tmp);
    if (!ok) return fail(h, HS_E_HIP, "sink read-back failed");
    int64_t m = 0;
    for (int64_t k = 0; k < want && m < cnt; ++k) if (all[(size_t)k] >= 0) created[m++] = all[(size_t)k];
    return HS_OK;
}
static bool created_is_the_admission_log(const hs_engine *h) { return h->L.sink_created == h->L.adm; }

int64_t hs_engine_read_sink(hs_engine *h, int32_t lp, int64_t *t_ns, int64_t *created_ns, int64_t cap) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "stations not set");
    if (lp < 0 || lp >= h->cfg.n_lp) return fail(h, HS_E_INVALID, "LP index %d out of range", lp);
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(h, HS_E_HIP, "device synchronisation failed");
    int64_t cnt = 0;
    if (hipMemcpy(&cnt, h->X.received + lp, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HS_E_HIP, "memcpy");
    if (cnt > h->L.cap) cnt = h->L.cap;
    if (cnt > cap) cnt = cap;
    if (cnt > 0) {
        int64_t *tmp = nullptr;
        if (hipMalloc(&tmp, (size_t)cnt * 8) != hipSuccess) return fail(h, HS_E_HIP, "hipMalloc of the read-back staging buffer failed");
        const int64_t *cols[2] = {h->L.sink_t, h->L.sink_created};
        int64_t *dsts[2] = {t_ns, created_ns};
        for (int c = 0; c < 2; ++c) {
            if (!dsts[c]) continue;
            hipLaunchKernelGGL(hs_gather_one, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, cols[c], tmp,
                               h->cfg.n_lp, lp, cnt, h->L.lp_major ? h->L.cap : (int64_t)0);
            if (hipStreamSynchronize(h->stream) != hipSuccess ||
                hipMemcpy(dsts[c], tmp, (size_t)cnt * 8, hipMemcpyDeviceToHost) != hipSuccess) {
                hipFree(tmp);
                return fail(h, HS_E_HIP, "sink read-back failed");
            }
        }
        hipFree(tmp);
        if (created_ns && created_is_the_admission_log(h)) {
            int64_t rej = 0;
            if (hipMemcpy(&rej, h->X.rejected + lp, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HS_E_HIP, "memcpy");
            if (rej > 0) { const int rc = skip_rejected_admissions(h, lp, cnt, rej, created_ns); if (rc) return rc; }
        }
    }
    return cnt;
}

int64_t hs_engine_read_sinks(hs_engine *h, int64_t *counts, int64_t *t_ns, int64_t *created_ns, int64_t cap_total) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "stations not set");
    if (!counts) return fail(h, HS_E_INVALID, "counts is required");
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(h, HS_E_HIP, "device synchronisation failed");
    const size_t n = (size_t)h->cfg.n_lp;
    if (hipMemcpy(counts, h->X.received, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HS_E_HIP, "memcpy");
    // exclusive offsets of each LP's run in the concatenated output; the transposition [cap][n_lp] -> per-LP runs
    // happens on the device (hs_gather_logs), then one bulk D2H per column
    const int64_t cap = h->L.cap;
    std::vector<int64_t> off(n);
    int64_t total = 0, maxc = 0;
    for (size_t i = 0; i < n; ++i) {
        const int64_t c = counts[i] > cap ? cap : counts[i];
        off[i] = total;
        total += c;
        maxc = c > maxc ? c : maxc;
    }
    if (total > cap_total) return fail(h, HS_E_INVALID, "output buffers too small for the sink records");
    if (total == 0 || (!t_ns && !created_ns)) return total;
    int64_t *d_off = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_off, n * 8) != hipSuccess || hipMalloc(&d_out, (size_t)total * 8) != hipSuccess) {
        if (d_off) hipFree(d_off);
        return fail(h, HS_E_HIP, "hipMalloc of the read-back staging buffers failed");
    }
    bool ok = hipMemcpy(d_off, off.data(), n * 8, hipMemcpyHostToDevice) == hipSuccess;
    const int64_t *cols[2] = {h->L.sink_t, h->L.sink_created};
    int64_t *dsts[2] = {t_ns, created_ns};
    for (int c = 0; c < 2 && ok; ++c) {
        if (!dsts[c]) continue;
        const dim3 grid((unsigned)((n + 63) / 64), (unsigned)((maxc + 63) / 64));
        hipLaunchKernelGGL(hs_gather_logs, grid, dim3(256), 0, h->stream, cols[c], h->X.received, d_off, d_out, (int)n, cap, (int)h->L.lp_major);
        ok = hipStreamSynchronize(h->stream) == hipSuccess &&
             hipMemcpy(dsts[c], d_out, (size_t)total * 8, hipMemcpyDeviceToHost) == hipSuccess;
    }
    hipFree(d_off);
    hipFree(d_out);
    if (!ok) return fail(h, HS_E_HIP, "sink read-back failed");
    if (created_ns && created_is_the_admission_log(h)) {     // (rare: LPs whose worker rejected a Request are read again, one by one)
        std::vector<int64_t> rej(n);
        if (hipMemcpy(rej.data(), h->X.rejected, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HS_E_HIP, "memcpy");
        for (size_t i = 0; i < n; ++i) {
            const int64_t c = counts[i] > cap ? cap : counts[i];
            if (rej[i] <= 0 || c <= 0) continue;
            const int rc = skip_rejected_admissions(h, (int32_t)i, c, rej[i], created_ns + off[i]);
            if (rc) return rc;
        }
    }
    return total;
}

int64_t hs_engine_read_probe(hs_engine *h, int32_t lp, int64_t *t_ns, int64_t *values, int64_t cap) {
    return hs_engine_read_probe_slot(h, lp, 0, t_ns, values, cap);
}

int hs_engine_read_source_generated(hs_engine *h, int32_t slot, int64_t *out) {
    if (!h || !h->have_stations || !out) return fail(h, HS_E_STATE, "stations not set");
    if (slot < 0 || slot > kMaxXSrc) return fail(h, HS_E_INVALID, "source slot %d out of range", slot);
    const size_t n = (size_t)h->cfg.n_lp;
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    HS_HIP(h, hipSetDevice(h->cfg.device));
    HS_HIP(h, hipStreamSynchronize(h->stream));
    if (slot == 0) { HS_HIP(h, hipMemcpy(out, h->X.generated, n * 8, hipMemcpyDeviceToHost)); return HS_OK; }
    if (!h->any_xsrc) { for (size_t i = 0; i < n; ++i) out[i] = 0; return HS_OK; }
    HS_HIP(h, hipMemcpy(out, h->X.x_n + (size_t)(slot - 1) * n, n * 8, hipMemcpyDeviceToHost));
    return HS_OK;
}

int64_t hs_engine_read_probe_slot(hs_engine *h, int32_t lp, int32_t slot, int64_t *t_ns, int64_t *values, int64_t cap) {
    if (!h || !h->have_stations) return fail(h, HS_E_STATE, "stations not set");
    if (lp < 0 || lp >= h->cfg.n_lp) return fail(h, HS_E_INVALID, "LP index %d out of range", lp);
    if (slot < 0 || slot >= kMaxProbes) return fail(h, HS_E_INVALID, "probe slot %d out of range", slot);
    if (!h->any_probe || slot >= h->n_probe_slots) return 0;
    if (h) { const int rcf = results_final(h); if (rcf) return rcf; }
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(h, HS_E_HIP, "device synchronisation failed");
    int64_t cnt = 0;
    if (hipMemcpy(&cnt, h->X.p_n + (size_t)slot * h->cfg.n_lp + lp, 8, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, HS_E_HIP, "memcpy");
    if (cnt > h->L.pcap) cnt = h->L.pcap;
    if (cnt > cap) cnt = cap;
    if (cnt > 0) {
        int64_t *tmp = nullptr;
        if (hipMalloc(&tmp, (size_t)cnt * 8) != hipSuccess) return fail(h, HS_E_HIP, "hipMalloc of the read-back staging buffer failed");
        const size_t so = (size_t)slot * (size_t)h->L.pcap * (size_t)h->cfg.n_lp;
        const int64_t *cols[2] = {h->L.probe_t + so, h->L.probe_v + so};
        int64_t *dsts[2] = {t_ns, values};
        for (int c = 0; c < 2; ++c) {
            if (!dsts[c]) continue;
            hipLaunchKernelGGL(hs_gather_one, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->stream, cols[c], tmp,
                               h->cfg.n_lp, lp, cnt, (int64_t)0);
            if (hipStreamSynchronize(h->stream) != hipSuccess ||
                hipMemcpy(dsts[c], tmp, (size_t)cnt * 8, hipMemcpyDeviceToHost) != hipSuccess) {
                hipFree(tmp);
                return fail(h, HS_E_HIP, "probe read-back failed");
            }
        }
        hipFree(tmp);
    }
    return cnt;
}

void hs_engine_destroy(hs_engine *h) {
    if (!h) return;
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (void *p : h->ipc_opened) hipIpcCloseMemHandle(p);      // the peers' exchange buffers as mapped here
    if (h->live_stream) { hipStreamDestroy(h->live_stream); hipEventDestroy(h->live_ev); }
    for (void *p : h->allocs) hipFree(p);
    uncached_release(h);                       // (back to the process-wide pool, never to the runtime)
    if (h->ev_a) hipEventDestroy(h->ev_a);
    if (h->ev_b) hipEventDestroy(h->ev_b);
    if (h->ev_k0) hipEventDestroy(h->ev_k0);
    if (h->ev_k1) hipEventDestroy(h->ev_k1);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;
}

int hs_debug_async_counters(hs_engine *h, unsigned long long out[4]) {
    if (!h || !out) return HS_E_INVALID;
    Totals t;
    if (hipSetDevice(h->cfg.device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess ||
        hipMemcpy(&t, h->tot, sizeof t, hipMemcpyDeviceToHost) != hipSuccess) return HS_E_HIP;
    for (int i = 0; i < 4; ++i) out[i] = t.dbg[i];
    return HS_OK;
}

int hs_debug_set_flags(hs_engine *h, int flags) {
    if (!h) return HS_E_INVALID;
    h->flags = flags;
    return HS_OK;
}

int hs_debug_draws(int32_t device, uint64_t seed, uint64_t sid, uint64_t k0, int64_t n, double rate, double *u,
                   double *e, int64_t *ns) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (n <= 0 || !u || !e || !ns) return fail(nullptr, HS_E_INVALID, "hs_debug_draws: bad arguments");
    HS_HIP(nullptr, hipSetDevice(device));
    double *du = nullptr, *de = nullptr;
    int64_t *dn = nullptr;
    HS_HIP(nullptr, hipMalloc((void **)&du, (size_t)n * 8));
    HS_HIP(nullptr, hipMalloc((void **)&de, (size_t)n * 8));
    HS_HIP(nullptr, hipMalloc((void **)&dn, (size_t)n * 8));
    hipLaunchKernelGGL(hs_debug_draws_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, seed, sid, k0, n, rate,
                       du, de, dn);
    HS_HIP(nullptr, hipGetLastError());
    HS_HIP(nullptr, hipMemcpy(u, du, (size_t)n * 8, hipMemcpyDeviceToHost));
    HS_HIP(nullptr, hipMemcpy(e, de, (size_t)n * 8, hipMemcpyDeviceToHost));
    HS_HIP(nullptr, hipMemcpy(ns, dn, (size_t)n * 8, hipMemcpyDeviceToHost));
    hipFree(du); hipFree(de); hipFree(dn);
    return HS_OK;
}

// The three hooks below share one shape: host arrays up, one launch, the results down, every device buffer freed on every path.
namespace {
struct DebugBuffers {
    void *d[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~DebugBuffers() { for (void *p : d) if (p) (void)hipFree(p); }
    hipError_t alloc(const size_t *bytes, int n) {
        for (int k = 0; k < n; ++k) {
            const hipError_t e = hipMalloc(&d[k], bytes[k]);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};
int debug_device(const char *who, int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, HS_E_INVALID, "%s: device ordinal %d out of range (%d devices)", who, device, ndev);
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, HS_E_HIP, "%s: hipSetDevice failed", who);
    return HS_OK;
}
}  // namespace

int hs_debug_log(int32_t device, int64_t n, const double *x, const double *u, double *out_log, double *out_exp1) {
    if (n <= 0 || !x || !u || !out_log || !out_exp1) return fail(nullptr, HS_E_INVALID, "hs_debug_log: bad arguments");
    if (const int rc = debug_device("hs_debug_log", device)) return rc;
    const size_t b = (size_t)n * 8, bytes[4] = {b, b, b, b};
    DebugBuffers m;
    hipError_t e = m.alloc(bytes, 4);
    if (e == hipSuccess) e = hipMemcpy(m.d[0], x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.d[1], u, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_log_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, (const double *)m.d[0],
                           (const double *)m.d[1], (double *)m.d[2], (double *)m.d[3]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out_log, m.d[2], b, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_exp1, m.d[3], b, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_log: %s", hipGetErrorString(e));
    return HS_OK;
}

int hs_debug_philox(int32_t device, int64_t n, const uint32_t *ctr_key, uint32_t *out) {
    if (n <= 0 || !ctr_key || !out) return fail(nullptr, HS_E_INVALID, "hs_debug_philox: bad arguments");
    if (const int rc = debug_device("hs_debug_philox", device)) return rc;
    const size_t bytes[2] = {(size_t)n * 24, (size_t)n * 16};
    DebugBuffers m;
    hipError_t e = m.alloc(bytes, 2);
    if (e == hipSuccess) e = hipMemcpy(m.d[0], ctr_key, bytes[0], hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, (const uint32_t *)m.d[0],
                           (uint32_t *)m.d[1]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, m.d[1], bytes[1], hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_philox: %s", hipGetErrorString(e));
    return HS_OK;
}

int hs_debug_stream_walk(int32_t device, int64_t n_walks, const uint64_t *seed, const uint64_t *sid, const uint64_t *k0,
                         int32_t n_steps, const uint8_t *steps, double *out, uint64_t *k_end) {
    if (n_walks <= 0 || n_steps <= 0 || !seed || !sid || !k0 || !steps || !out || !k_end)
        return fail(nullptr, HS_E_INVALID, "hs_debug_stream_walk: bad arguments");
    int64_t row = 0;
    for (int32_t j = 0; j < n_steps; ++j) {
        if (steps[j] != 1 && steps[j] != 2 && steps[j] != 4)
            return fail(nullptr, HS_E_INVALID, "hs_debug_stream_walk: steps[%d] = %d (each step draws 1, 2 or 4)", j, (int)steps[j]);
        row += steps[j];
    }
    if (const int rc = debug_device("hs_debug_stream_walk", device)) return rc;
    const size_t w = (size_t)n_walks * 8, bytes[6] = {w, w, w, (size_t)n_steps, w * (size_t)row, w};
    DebugBuffers m;
    hipError_t e = m.alloc(bytes, 6);
    if (e == hipSuccess) e = hipMemcpy(m.d[0], seed, w, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.d[1], sid, w, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.d[2], k0, w, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.d[3], steps, (size_t)n_steps, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_stream_walk_kernel, dim3((unsigned)((n_walks + 63) / 64)), dim3(64), 0, 0, n_walks,
                           (const uint64_t *)m.d[0], (const uint64_t *)m.d[1], (const uint64_t *)m.d[2], n_steps,
                           (const uint8_t *)m.d[3], row, (double *)m.d[4], (uint64_t *)m.d[5]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, m.d[4], bytes[4], hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(k_end, m.d[5], w, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_stream_walk: %s", hipGetErrorString(e));
    return HS_OK;
}

// The tick table of ONE stream (csrc/hs_tables.hpp) -- `lone` = 0: the cooperative kernel the engine uses; 1: the same chain on
// one lane with the sequential integrator (the device-side reference: tests/test_gpu_tables.py compares the two bit for bit).
// profile: {kind, p0, p1, p2, p3}; returns the number of entries written to out_times (<= cap), or < 0.
int64_t hs_debug_tick_table(int32_t device, const double *profile, int32_t poisson, uint64_t seed, uint64_t sid, int64_t start_ns,
                            int64_t horizon_ns, int64_t cap, int64_t lane_budget, int32_t lone, int64_t *out_times,
                            uint64_t *out_status) {
    if (!profile || !out_times || cap <= 0) return fail(nullptr, HS_E_INVALID, "hs_debug_tick_table: bad argument");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, HS_E_NO_DEVICE, "no HIP device");
    TickRow r{};
    r.kind = (uint32_t)profile[0]; r.p0 = profile[1]; r.p1 = profile[2]; r.p2 = profile[3]; r.p3 = profile[4];
    r.poisson = poisson ? 1u : 0u; r.seed = seed; r.sid = sid; r.owner = 0;
    TickRow *drow = nullptr; int64_t *dt = nullptr, *dc = nullptr; unsigned long long *ds = nullptr;
    hipError_t e = hipMalloc((void **)&drow, sizeof r);
    if (e == hipSuccess) e = hipMalloc((void **)&dt, (size_t)cap * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&dc, 8);
    if (e == hipSuccess) e = hipMalloc((void **)&ds, 16);
    if (e == hipSuccess) e = hipMemcpy(drow, &r, sizeof r, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = tick_tables_launch(nullptr, drow, 1, start_ns, horizon_ns, cap, dt, dc, ds, lane_budget > 0 ? lane_budget : kDefaultLaneBudget, lone != 0);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    int64_t cnt = 0;
    unsigned long long st[2] = {0ull, 0ull};
    if (e == hipSuccess) e = hipMemcpy(&cnt, dc, 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(st, ds, 16, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_times, dt, (size_t)cap * 8, hipMemcpyDeviceToHost);
    (void)hipFree(drow); (void)hipFree(dt); (void)hipFree(dc); (void)hipFree(ds);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_tick_table: %s", hipGetErrorString(e));
    if (out_status) { out_status[0] = st[0]; out_status[1] = st[1]; }
    return cnt;
}

int hs_debug_const_div(int32_t device, double b, int64_t n, const double *a, double *q_fast, double *q_ieee,
                       double *q_ns) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (n <= 0 || !a || !q_fast || !q_ieee || !q_ns) return fail(nullptr, HS_E_INVALID, "hs_debug_const_div: bad arguments");
    HS_HIP(nullptr, hipSetDevice(device));
    double *d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto &p : d) HS_HIP(nullptr, hipMalloc((void **)&p, (size_t)n * 8));
    HS_HIP(nullptr, hipMemcpy(d[0], a, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(hs_debug_const_div_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, b, n, d[0], d[1],
                       d[2], d[3]);
    HS_HIP(nullptr, hipGetLastError());
    HS_HIP(nullptr, hipMemcpy(q_fast, d[1], (size_t)n * 8, hipMemcpyDeviceToHost));
    HS_HIP(nullptr, hipMemcpy(q_ieee, d[2], (size_t)n * 8, hipMemcpyDeviceToHost));
    HS_HIP(nullptr, hipMemcpy(q_ns, d[3], (size_t)n * 8, hipMemcpyDeviceToHost));
    for (auto &p : d) hipFree(p);
    return HS_OK;
}

int hs_debug_time_ops(int32_t device, int64_t n, const int64_t *ns, const double *secs, double *out_f64, int64_t *out_i64) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (n <= 0 || !ns || !secs || !out_f64 || !out_i64) return fail(nullptr, HS_E_INVALID, "hs_debug_time_ops: bad arguments");
    if (device < 0 || device >= ndev) return fail(nullptr, HS_E_INVALID, "device ordinal %d out of range (%d devices)", device, ndev);
    HS_HIP(nullptr, hipSetDevice(device));
    void *d[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[4] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 24, (size_t)n * 16};
    for (int k = 0; k < 4; ++k) {
        const hipError_t e = hipMalloc(&d[k], bytes[k]);
        if (e != hipSuccess) { for (auto &p : d) if (p) hipFree(p); return fail(nullptr, HS_E_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    }
    hipError_t e = hipMemcpy(d[0], ns, bytes[0], hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[1], secs, bytes[1], hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_time_ops_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, (const int64_t *)d[0],
                           (const double *)d[1], (double *)d[2], (int64_t *)d[3]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out_f64, d[2], bytes[2], hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_i64, d[3], bytes[3], hipMemcpyDeviceToHost);
    for (auto &p : d) hipFree(p);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_time_ops: %s", hipGetErrorString(e));
    return HS_OK;
}

}  // extern "C"
