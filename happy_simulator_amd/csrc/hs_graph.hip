// hs_graph.hip -- general entity graphs on ONE heap (include/hs_engine.h "General entity graphs", ABI 15, LoadBalancer nodes ABI 16).
//
// The station engines (hs_station.hpp / hs_netstation.hpp) get their speed from a fixed LP shape; what the same entity classes
// can be wired into beyond that shape -- links with several senders, routers with any fan-out that also target Servers and
// routers, Servers behind Servers next to links, any number of Sources per Server -- has no LP decomposition that the lineage
// key orders, and the reference's own definition of the order is the heap: (time, _sort_index) with the index taken from two
// global creation counters (core/event.py:53-77, core/event_heap.py:48).  So this file IS that loop, on the device:
//   * one lane of one wavefront pops and invokes events exactly like `Simulation._execute_until` (core/simulation.py:449-505);
//   * the binary heap follows CPython's heapq sift procedures step for step, so equal (time, index) keys -- possible between
//     the pre-run counter and the run-time counter -- pop in heapq's layout order;
//   * the first kLdsHeap entries of the heap (every level a sift touches first) live in LDS, the rest in HBM; node parameters
//     and state are two 64-byte rows per node (L2-resident for the models this path is for);
//   * heap, Request pool and the Sink record log grow on demand: the kernel stops in front of the event that would not fit,
//     the host enlarges the buffer and launches again (a launch also ends after kBudget events, so no launch runs for minutes).
// Handlers restate the reference handler by handler (citations at each); arithmetic through hs_device.hpp (the same fixed IEEE
// operation sequences as every other engine), streams through the Philox streams of DESIGN.md section 3.
//
// Cost: ~2.4 us per event (~1 000 vector instructions of ONE lane; measured: not memory).  An exactness path for the graphs the parallel
// engines refuse; its throughput comes from heaps side by side: replicas (hs_graph_run_many) and a Simulation's disconnected parts
// (hs_graph_run_parts).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <type_traits>
#include <utility>

#include "../../include/hs_engine.h"
#include "hs_device.hpp"
#include "hs_tables_api.hpp"
#include "hs_ring.hpp"
#include "hs_wrr.hpp"

namespace hs {
namespace graph {

constexpr int kBatchStat = 4;                  // int64 per heap a batch launch reports: status, processed, pending events, the earliest's time
constexpr int kLdsNodes = 192, kLdsNodesBatch = 48;   // nodes whose parameters and state stay in LDS for a launch (24 KB / 6 KB)
constexpr int kLdsHeapBatch = 1024;            // ... of each of the heaps hs_graph_run_many runs side by side
constexpr int kLdsHeap = 4096;                 // heap entries in LDS: 4 096 x 32 B = 128 KB of the CU's 160 (+ 24 KB of nodes)
constexpr long long kBudget = 1ll << 21;       // events per launch (~2 s)
// LeastConnections / WeightedLeastConnections: from this many backends on, all 64 lanes take the selection (graph_loop's outer loop);
// below it the lone lane scans them itself.  NOT MEASURED YET -- an estimate: the hand-over costs two workgroup barriers, an LDS
// round trip and six cross-lane steps on a (binary64, int32) pair, a few hundred cycles of the lone wavefront, i.e. a few dozen of
// the lane-serial scan's dependent load pairs.  tools/lb_strategies_profile.py measures both sides at 8 .. 32 768 backends
// (hs_debug_graph_flags); the crossover it finds belongs here.  Either side leaves the same bits, so the value is a matter of time only.
constexpr int kCoopMinBackends = 32;

struct GEvent {                                // 32 bytes
    int64_t t;                                 // Event.time
    uint64_t idx;                              // Event._sort_index
    int32_t node;                              // target entity
    int32_t req;                               // the Request it carries (-1: none)
    uint32_t kind;                             // HS_EV_*
    uint32_t pad;
};

struct GParam {                                // 64 bytes, read-only
    uint64_t stream_base;
    double mean;                               // Source: rate; Server: mean service; link: mean jitter
    double lat_min;                            // link: ConstantLatency base
    double loss;                               // link: packet_loss_rate
    int64_t lim;                               // Source: stop_after ns (< 0 never); Server: queue capacity (< 0 unbounded)
    int32_t target;
    int32_t conc;                              // Server: max_concurrent; Source: n_clients of its ClientKeyEventProvider (0: none);
                                               // LoadBalancer: entries of its client -> backend-slot table (lim = its offset);
                                               // WeightedRoundRobin: the total weight W = entries of its selection table (lim = its offset)
                                               // HealthChecker: mean = interval, lat_min = timeout (seconds), conc = healthy_threshold,
                                               // lim = unhealthy_threshold, sub = _is_running, target = its LoadBalancer
                                               // Bulkhead: conc = max_concurrent, lim = max_wait_queue, lat_min = max_wait_time (sub = 1: it has one),
                                               // rt_off / rt_cnt = its table in GCtl::rs_tab;  TimeoutWrapper: lat_min = timeout, rt_off / rt_cnt likewise
                                               // Client: lat_min = timeout (sub = 1: it has one), conc = max_attempts - 1 = entries of its delay
                                               // table at GCtl::cl_delays + lim, rt_off / rt_cnt = its table in GCtl::rs_tab (two words per place)
    int32_t rt_off, rt_cnt;                    // router / LoadBalancer: its targets; Source / Probe: rt_off = row of its tick table (-1: none)
    uint8_t kind, sub;                         // sub: Source arrival kind (hs_source_kind); Server / link latency kind; Probe metric; LB strategy
    uint8_t crashed;                           // entity._crashed (faults/node_faults.py:46-62): the one byte of a row a run writes -- kFaultOn / kFaultOff
    uint8_t pad[5];
};

struct GState {                                // 64 bytes
    // Source: a = ArrivalTimeProvider.current_time, b = arrival draws, c = generated_count, d = payload Requests built
    // Server: a = stats_accepted, b = stats_dropped, c = completed, d = rejected
    // link:   a = entered, b = packets_sent, c = packets_dropped, d = jitter draws; a graph with link faults (GVars::n_link_faults):
    //         svc_draws = loss draws, qlen / active = the latency / loss fault in force (1 + its place in GVars::faults; 0: none)
    // router: a = stats_routed (= route draws);  Sink: a = events_received
    // Probe:  a = ticks taken from its table, c = samples
    // limiter: a = received (= Requests handled), b = dropped, c = queued, d = polls handled; forwarded = a - b - qlen;
    //          active = kLimPollScheduled | kLimHasTime; svc_draws = _last_refill_time / _last_leak_time / _current_window_start ns
    //          (SlidingWindow: the ring's head); total_service = tokens (the windows: their count, as int64 bits)
    // LoadBalancer: a = requests_received, b = requests_forwarded, c = requests_failed (= no_backend_available), d = in flight,
    //               svc_draws = RoundRobin._index (ConsistentHash / IPHash: their fallback's, the key-less Requests; WeightedRoundRobin:
    //               its selections);  Source: svc_draws = KEY draws
    //               a graph with health state (GCtl::health): qlen = healthy_count, qhead / qtail = backends_marked_unhealthy / _healthy
    // HealthChecker: a = checks_performed, b = checks_passed, c = checks_failed (= checks_timed_out), d = _next_check_id,
    //                qlen = backends_marked_healthy, active = backends_marked_unhealthy
    // Bulkhead: a = total, b = accepted, c = rejected, d = timed_out, svc_draws = _next_request_id (queued = svc_draws - b: every forward
    //           and every enqueue takes one id), total_service = peak_concurrent | peak_queue_depth (two int32), active = _active_count
    //           (= len(_in_flight)), qhead / qtail / qlen = _wait_queue through Request::next (Request::idx = enqueue time, service_s = id)
    // TimeoutWrapper: a = total, b = successful, c = timed_out, svc_draws = _next_request_id, qlen = len(_in_flight)
    // Client: a = requests_sent, b = responses_received, c = timeouts, d = retries, svc_draws = failures, qlen = len(_in_flight)
    int64_t a, b, c, d;
    double total_service;                      // Server._total_service_time
    uint64_t svc_draws;
    int32_t qhead, qtail;                      // FIFOQueue (components/queue_policy.py:75-114) as a list through Request::next
    int32_t qlen, active;
};

struct GRequest {                              // 32 bytes: the payload Event's identity + its context
    int64_t created;                           // context["created_at"] (load/source.py:76-79; forwarded unchanged, core/entity.py:100-105)
    uint64_t idx;                              // sort index of the queued payload Event (kept on retarget, queue_driver.py:86-90)
    double service_s;                          // service_time_s of the generator frame (server/server.py:246-247); dead until WORK: while a
                                               // wrapper's hook rides on the Event (and in a Bulkhead's queue) the wrapper's request id, as bits
                                               // (a Client's hook: its key, request_id | attempt << 30)
    int64_t client;                            // context["metadata"]["client_id"] (-1: none; <= -2: no client_id, but the metadata of the
                                               // Client the Request passed last: -2 - its key)
    int32_t next;                              // FIFO / free list
    int32_t hook : 31;                         // LoadBalancer / checker / wrapper whose completion hook rides on the Event (-1: none)
    uint32_t pre : 1;                          // `idx` came from the process-wide counter (GEvent::pad), set where the payload is queued
};

// RateLimitedEntity's two handlers: heap-entry kinds of this loop only, beyond the public fifteen (hs_summary.events_by_kind keeps its
// meaning; they are counted per node: GState::a Requests, GState::d polls)
constexpr uint32_t kEvLimRequest = HS_EV_KINDS, kEvLimPoll = HS_EV_KINDS + 1;
// CrashNode / PauseNode (faults/node_faults.py): the two daemon Events of a node fault, two more internal kinds.  GEvent::node is the
// entity whose flag they set / clear; GEvent::pad bit 1: the Event was cancelled before the run (popped and skipped,
// core/simulation.py:475-477).  They count in events_processed and per graph (GVars::faults_processed), not in events_by_kind.
constexpr uint32_t kEvFaultOn = HS_EV_KINDS + 2, kEvFaultOff = HS_EV_KINDS + 3;
// HealthChecker (components/load_balancer/health_check.py:253-444): its three handlers, three more internal kinds, aimed at the checker
// itself.  GEvent::node is the checker; a response / timeout carries the backend's slot in its LoadBalancer as req = -2 - slot (negative:
// no Request) and the check id in GEvent::pad above the two flag bits.  They count in events_processed and per graph
// (GVars::health_by_kind), not in events_by_kind.
constexpr uint32_t kEvHcCycle = HS_EV_KINDS + 4, kEvHcResp = HS_EV_KINDS + 5, kEvHcTimeout = HS_EV_KINDS + 6, kEvAllKinds = HS_EV_KINDS + 7;
// Bulkhead / TimeoutWrapper (components/resilience/bulkhead.py, timeout.py): a Request at the wrapper, the `_bh_response` /
// `_tw_response` Event its completion hook constructs, and the `_bh_timeout` / `_tw_timeout` Event -- six more internal kinds, aimed at
// the wrapper itself.  A response / timeout carries no Request: its per-wrapper request id rides in GEvent::pad above the two flag bits
// (the low 30 bits) and in GEvent::req (-2 - the bits above them).  They count in events_processed and per graph
// (GVars::resil_by_kind), not in events_by_kind.
constexpr uint32_t kEvBhReq = kEvAllKinds, kEvBhResp = kEvAllKinds + 1, kEvBhTimeout = kEvAllKinds + 2, kEvTwReq = kEvAllKinds + 3,
                   kEvTwResp = kEvAllKinds + 4, kEvTwTimeout = kEvAllKinds + 5, kEvResKinds = kEvAllKinds + 6;
// Client (components/client/client.py): a request at the Client (a Source's or Server's Request, a schedule()d one, a retry), the
// `_client_response` Event its completion hook constructs and the `_client_timeout` Event -- three more internal kinds, aimed at the
// Client itself.  The key (request_id, attempt) is ONE word, request_id (30 bits, 0: None) | attempt << 30 (at most 2^16): a response, a
// timeout, a retry and a schedule()d request carry no Request but the key like the wrappers' ids -- its low 30 bits (the request_id) in
// GEvent::pad above the two flag bits, the attempt in GEvent::req (-2 - attempt); a request that carries a Request (req >= 0) has no
// request_id and is attempt 1.  They count in events_processed and per graph (GVars::client_by_kind), not in events_by_kind.
constexpr uint32_t kEvClReq = kEvResKinds, kEvClResp = kEvResKinds + 1, kEvClTimeout = kEvResKinds + 2, kEvCliKinds = kEvResKinds + 3;
constexpr int kKeyAttemptShift = 30;
// BatchProcessor / ConveyorBelt / GateController (components/industrial/): eight more internal kinds.  An item carries its Request; a
// `_BatchTimeout` carries the processor's timeout id in GEvent::pad above the two flag bits (GState::d holds the id of the ONE pending
// timeout, 0: none -- an entry with another id was cancelled when its batch started, core/simulation.py:326-329); the continuation of
// a batch carries the head of its list through Request::next in GEvent::req and its length in GEvent::pad above the flag bits, so
// several batches of one processor are in process at once.  They count in events_processed and per graph (GVars::flow_by_kind).
constexpr uint32_t kEvBpItem = kEvCliKinds, kEvBpTimeout = kEvCliKinds + 1, kEvBpCont = kEvCliKinds + 2, kEvCvItem = kEvCliKinds + 3,
                   kEvCvCont = kEvCliKinds + 4, kEvGtItem = kEvCliKinds + 5, kEvGtOpen = kEvCliKinds + 6, kEvGtClose = kEvCliKinds + 7,
                   kEvFlowKinds = kEvCliKinds + HS_FLOW_KINDS;
// AutoScaler (components/deployment/auto_scaler.py:321-357): its `_autoscaler_evaluate` Event, one more internal kind, a daemon aimed at
// the scaler itself, no Request.  It counts in events_processed and per graph (GVars::as_evals).
constexpr uint32_t kEvAsEval = kEvFlowKinds, kEvAsKinds = kEvFlowKinds + 1;
constexpr int kMaxScalerSteps = HS_AUTOSCALER_MAX_STEPS;
// RollingDeployer (components/deployment/rolling_deployer.py:158-175): its seven handlers, seven more internal kinds, aimed at the
// deployer itself, no daemons.  A `_rolling_health_pass` / `_rolling_health_timeout` carries the instance's slot in the LoadBalancer as
// req = -2 - slot (its `server_name`).  They count in events_processed and per graph (GVars::rd_by_kind).
constexpr uint32_t kEvRdStart = kEvAsKinds, kEvRdBatch = kEvAsKinds + 1, kEvRdCheck = kEvAsKinds + 2, kEvRdPass = kEvAsKinds + 3,
                   kEvRdTimeout = kEvAsKinds + 4, kEvRdRollback = kEvAsKinds + 5, kEvRdComplete = kEvAsKinds + 6,
                   kEvDpKinds = kEvAsKinds + HS_DEPLOYER_KINDS;
// CanaryDeployer (components/deployment/canary_deployer.py:265-280): its six handlers, six more internal kinds, aimed at the deployer
// itself, no daemons, no Request.  They count in events_processed and per graph (GVars::cn_by_kind).
constexpr uint32_t kEvCnStart = kEvDpKinds, kEvCnStage = kEvDpKinds + 1, kEvCnEval = kEvDpKinds + 2, kEvCnPromote = kEvDpKinds + 3,
                   kEvCnRollback = kEvDpKinds + 4, kEvCnComplete = kEvDpKinds + 5, kEvCnKinds = kEvDpKinds + HS_CANARY_KINDS;
// Hedge / Fallback (components/resilience/hedge.py, fallback.py): a Request at a Hedge, its `_hg_response`, its `_hg_send_hedge`; a
// Request at a Fallback, its `_fb_primary_response`, its `_fb_timeout`, its `_fb_fallback_response` -- seven more internal kinds, aimed
// at the wrapper itself.  A response / send-hedge / timeout carries no Request but its key like the wrappers' ids (mk_id): the request
// id in the low kHgIdBits bits, above them `hedge_number` (a send-hedge) and the flag bit -- `is_hedge` of a Hedge's response, "the
// fallback entity's response" of a Fallback's.  They count in events_processed and per graph (GVars::hg_by_kind).
constexpr uint32_t kEvHgReq = kEvCnKinds, kEvHgResp = kEvCnKinds + 1, kEvHgSend = kEvCnKinds + 2, kEvFbReq = kEvCnKinds + 3,
                   kEvFbPrimResp = kEvCnKinds + 4, kEvFbTimeout = kEvCnKinds + 5, kEvFbFbResp = kEvCnKinds + 6,
                   kEvHgKinds = kEvCnKinds + HS_HEDGE_KINDS;
constexpr int kHgIdBits = 34, kHgFlagBit = 50;               // (a key's bits above the low 30 ride in GEvent::req: at most 31 of them)
constexpr int64_t kHgIdMask = (1ll << kHgIdBits) - 1, kHgFlag = 1ll << kHgFlagBit;
static_assert(HS_HEDGE_MAX_HEDGES < (1 << (kHgFlagBit - kHgIdBits)), "hedge_number fits between the id and the flag");
// PooledCycleResource / InventoryBuffer (components/industrial/pooled_cycle.py, inventory.py): a Request at a pool, the continuation of
// its cycle (it carries the Request); a consume Request at a buffer, its `_InventoryReplenish` (no Request) -- the last four kinds the
// kind word holds (60 .. 63 of 64: the next family widens kDrop and s_by_kind first).  They count in events_processed and per graph
// (GVars::st_by_kind).
constexpr uint32_t kEvPcItem = kEvHgKinds, kEvPcCont = kEvHgKinds + 1, kEvIbItem = kEvHgKinds + 2, kEvIbReplenish = kEvHgKinds + 3,
                   kEvStKinds = kEvHgKinds + HS_STOCK_KINDS;
constexpr int kMaxFlowItems = HS_FLOW_MAX_ITEMS;            // batch_size / a bounded gate queue: a batch's length rides in 30 bits of GEvent::pad
constexpr uint32_t kPadPre = 1u, kPadCancelled = 2u;
constexpr int kPadIdShift = 2;                 // a check id in GEvent::pad (its low 30 bits: only the one pending id of a backend and ids
                                               // at most one timeout older are ever compared)
// Event.invoke drops an Event whose TARGET has `_crashed` set (core/event.py:261); ProcessContinuation.invoke (:465) does not look.
// These kinds are aimed at the entity itself; NOTIFY / POLL / DELIVER / WORK / PROBE go to its driver, queue, worker adapter or the
// probe's callback, the two continuations resume a generator: never dropped.
constexpr uint32_t kDropKinds = (1u << HS_EV_SOURCE) | (1u << HS_EV_PROBE_TICK) | (1u << HS_EV_ENQUEUE) | (1u << HS_EV_SINK) | (1u << HS_EV_LINK) |
                                (1u << HS_EV_ROUTE) | (1u << HS_EV_LB) | (1u << HS_EV_LB_RESP) | (1u << kEvLimRequest) | (1u << kEvLimPoll) |
                                (1u << kEvHcCycle) | (1u << kEvHcResp) | (1u << kEvHcTimeout);
// ... and all six kinds of the two wrappers (the instantiation that dispatches them tests this word; the others keep theirs)
constexpr uint32_t kDropKindsRes = kDropKinds | (1u << kEvBhReq) | (1u << kEvBhResp) | (1u << kEvBhTimeout) | (1u << kEvTwReq) |
                                   (1u << kEvTwResp) | (1u << kEvTwTimeout);
// ... and the three of a Client
constexpr uint32_t kDropKindsCli = kDropKindsRes | (1u << kEvClReq) | (1u << kEvClResp) | (1u << kEvClTimeout);
static_assert(kEvCliKinds <= 32, "kDropKinds is one word");
// ... and, beyond the 32 kinds one word holds, the six of the three flow entities that are aimed at the entity itself (the two
// continuations resume a generator): a second constant of 64 bits, tested by the one instantiation that dispatches them
constexpr uint64_t kDropKindsFlow = (uint64_t)kDropKindsCli | (1ull << kEvBpItem) | (1ull << kEvBpTimeout) | (1ull << kEvCvItem) |
                                    (1ull << kEvGtItem) | (1ull << kEvGtOpen) | (1ull << kEvGtClose);
static_assert(kEvFlowKinds <= 64, "kDropKindsFlow is two words; s_by_kind is zeroed by one lane per kind");
// ... and a scaler's evaluation, tested by the one instantiation that dispatches it
constexpr uint64_t kDropKindsAs = kDropKindsFlow | (1ull << kEvAsEval);
static_assert(kEvAsKinds <= 64, "kDropKindsAs is two words; s_by_kind is zeroed by one lane per kind");
// ... and a deployer's seven
constexpr uint64_t kDropKindsDp = kDropKindsAs | (((1ull << (HS_DEPLOYER_KINDS + HS_CANARY_KINDS)) - 1ull) << kEvRdStart);
static_assert(kEvCnKinds <= 64, "kDropKindsDp is two words; s_by_kind is zeroed by one lane per kind");
// ... and all seven of a Hedge and a Fallback
constexpr uint64_t kDropKindsHg = kDropKindsDp | (((1ull << HS_HEDGE_KINDS) - 1ull) << kEvHgReq);
static_assert(kEvHgKinds <= 64, "kDropKindsHg is two words; s_by_kind is zeroed by one lane per kind");
// ... and the three of a pool and a buffer that are aimed at the entity itself (the end of a cycle resumes a generator)
constexpr uint64_t kDropKindsSt = kDropKindsHg | (1ull << kEvPcItem) | (1ull << kEvIbItem) | (1ull << kEvIbReplenish);
static_assert(kEvStKinds <= 64, "kDropKindsSt is two words; s_by_kind is zeroed by one lane per kind");
// The levels of graph_loop.  A level carries all the code of the levels below it, and a graph (or a batch of graphs) runs at the lowest
// level that dispatches all its kinds: the lone lane's loop is bound by its own instruction count and register allocation, so a graph
// does not carry the code of a family it does not hold (the two fault tests per event were measurable).
enum {
    kLvPlain,          // Source, Server, Sink, Link, Router, LoadBalancer, Probe, RateLimitedEntity
    kLvFaults,         // + fault Events (CrashNode / PauseNode)
    kLvHealth,         // + a HealthChecker or an unhealthy backend
    kLvResilience,     // + a Bulkhead or a TimeoutWrapper
    kLvClient,         // + a Client
    kLvFlow,           // + a BatchProcessor, a ConveyorBelt or a GateController
    kLvQueues,         // + a Server with a LIFOQueue, an AdaptiveLIFO or a CoDelQueue (no kinds of its own)
    kLvLinkFaults,     // + a link fault, InjectLatency / InjectPacketLoss (no kinds of its own)
    kLvScaler,         // + an AutoScaler
    kLvDeploy,         // + a RollingDeployer or a CanaryDeployer
    kLvHedge,          // + a Hedge or a Fallback
    kLvStock,          // + a PooledCycleResource or an InventoryBuffer
    kLevels
};
// ... the kinds a level dispatches (any other: kBadKind) ...
constexpr uint32_t kLevelKinds[kLevels] = {kEvFaultOn, kEvHcCycle, kEvAllKinds, kEvResKinds, kEvCliKinds, kEvFlowKinds, kEvFlowKinds, kEvFlowKinds,
                                           kEvAsKinds, kEvCnKinds, kEvHgKinds, kEvStKinds};
// ... and those of them a crashed target drops (one word is tested below kLvFlow, two from there on)
constexpr uint64_t kLevelDrop[kLevels] = {kDropKinds, kDropKinds, kDropKinds, kDropKindsRes, kDropKindsCli, kDropKindsFlow, kDropKindsFlow, kDropKindsFlow,
                                          kDropKindsAs, kDropKindsDp, kDropKindsHg, kDropKindsSt};
// GParam of a PooledCycleResource: conc = pool_size, lim = cycle_time in ns, rt_cnt = queue_capacity (0: unbounded), target = its
// downstream (-1: none).  GState: a = completed, b = rejected, active = _active (_available = pool_size - _active: the two move
// together), qhead / qtail / qlen = _queue through Request::next.
// GParam of an InventoryBuffer: lim = reorder_point, stream_base = order_quantity, mean = lead_time in seconds, target = its downstream,
// conc = its stockout_target (-1: none).  GState: a = _stock, b = stockouts, c = reorders, d = items_consumed,
// svc_draws = items_replenished, active = _order_pending.
constexpr int kDefaultHedgeTable = 256;                 // entries a Hedge's / Fallback's table holds before it first grows
// One entry of a Hedge's or a Fallback's `_in_flight`: the id, start_time, the state and what a later duplicate of the Request is built
// from -- the original Event's context as GRequest carries it (the first copy may long have been freed at a Sink).
struct GHgEnt {                                // 40 bytes
    int64_t id;                                // 0: the place is empty (ids count from 1)
    int64_t start;                             // start_time ns
    int64_t created, client;                   // GRequest::created / GRequest::client of the original Request
    int64_t st;                                // Hedge: bit 0 completed, bits 8-31 hedges_sent, bits 32-63 responses_received; Fallback: 0 "primary", 1 "fallback"
};
constexpr int kHgSentShift = 8, kHgRecvShift = 32;
// A Hedge's / Fallback's table, one row per wrapper in HBM (GVars::hg; GParam::rt_off = its row): open addressing on the id -- ids
// ascend and are never reused, so `id & (cap - 1)` spreads the live ones evenly --, linear probing, removal by shifting the cluster's
// tail back (no tombstones).  At most half full, so a probe for an id that has left ends after a few places however many leaked
// entries the table holds.
struct GHg { GHgEnt *tab; long long cap; };    // cap: a power of two
// GParam of a Hedge: lim = hedge_delay ns, conc = max_hedges; of a Fallback: lim = timeout ns (< 0: None), conc = the fallback entity.
// GState of a Hedge: a = total_requests, b = primary_wins, c = hedge_wins, d = hedges_sent, total_service = hedges_cancelled (as int64
// bits), svc_draws = _next_request_id, qlen = len(_in_flight); of a Fallback: a = total_requests, b = primary_successes,
// c = primary_failures, d = fallback_invocations, total_service = fallback_successes (as int64 bits), svc_draws, qlen likewise.
constexpr int kMaxBulkheadConcurrent = HS_BULKHEAD_MAX_CONCURRENT;         // Bulkhead.max_concurrent the in-flight table is sized for (include/hs_engine.h)
constexpr int kDefaultTimeoutTable = 256;                // ids a TimeoutWrapper's (keys a Client's) table holds before it first grows
constexpr int kMaxClientAttempts = HS_CLIENT_MAX_ATTEMPTS;   // the attempt of a key is 16 bits and one
// hs_graph_add_fault: flags bit 0 = on, bit 1 = cancelled.  hs_graph_add_link_fault: bits 2-3 = 1 latency / 2 loss (0: a node fault),
// value = what an activation puts in force -- the extra latency in seconds as the Duration the reference adds, or the loss rate.  A link
// fault's heap entry carries 1 + its place in this array in GEvent::pad above the two flag bits (0: a node fault); the link's state
// names the entry in force, so a link's handler reads the value here: the array stays on the device for the graph's life.
struct GFault { int64_t t; int32_t node; uint32_t flags; double value; };
constexpr uint32_t kFaultWhatShift = 2, kFaultLatency = 1, kFaultLoss = 2;
// HealthChecker._backend_states / _pending_checks of one backend, at its slot of the LoadBalancer's targets (one checker per LoadBalancer)
struct GHc {                                   // 32 bytes
    int64_t succ, fail;                        // consecutive_successes / consecutive_failures
    int64_t last_time;                         // last_check_time (has_time)
    int32_t pending;                           // _pending_checks[backend.name] (0: none; ids count from 1)
    int8_t is_checking, last_passed, has_time;        // last_check_passed: -1 = None
    int8_t wrr_seen;                           // WeightedRoundRobin._current_weights has an entry for the backend: it was in a list select() saw
};
// A Server's queue policy other than FIFOQueue (components/queue_policy.py LIFOQueue, components/queue_policies/adaptive_lifo.py,
// codel.py): its parameters and state, one row per such Server in HBM (GVars::qp; GParam::pad[0] = hs_queue_policy, GParam::rt_cnt = its
// row; GParam::lim = the policy's capacity).  While a Request waits in such a queue GRequest::hook is the link to its predecessor (what a
// pop-newest needs; ENQUEUE fired and cleared the hook, a pop restores -1) and, under CoDel, GRequest::service_s its enqueue time in ns,
// as bits (dead until WORK; the hook's id is read before it is overwritten).
struct GQueue {                                // 112 bytes
    double target, interval;                   // CoDelQueue: target_delay, interval (seconds)
    int64_t threshold;                         // AdaptiveLIFO: congestion_threshold
    int64_t first_above, drop_next;            // CoDel: _first_above_time / _drop_next in ns (kQueueNone: None)
    int64_t count, last_count;                 // CoDel: _count, _last_count
    int64_t enqueued, deq_a, deq_b;            // enqueued; dequeued (CoDel) / dequeued_fifo; dequeued_lifo
    int64_t dropped, cap_rejected;             // CoDel: dropped; capacity_rejected
    int64_t switches;                          // AdaptiveLIFO: mode_switches; CoDel: drop_intervals
    int32_t flag, kind;                        // AdaptiveLIFO: _was_congested; CoDel: _dropping
};
constexpr int64_t kQueueNone = INT64_MIN;
// An AutoScaler's policy and what its GState row has no room for, one row per scaler in HBM (GVars::as; GParam::stream_base = its row).
// GParam of a scaler: mean = evaluation_interval, lat_min = scale_out_cooldown, loss = scale_in_cooldown (seconds), conc = min_instances,
// lim = max_instances, target = its LoadBalancer, sub = _is_running, rt_off = the slot of instance 1 among the LoadBalancer's targets
// (= its initial backends), rt_cnt = the pool's size P.  GState: a = evaluations, b = scale_out_count, c = scale_in_count,
// d = cooldown_blocks.
struct GAs {
    double target;                             // TargetUtilization._target
    double thr_out, thr_in;                    // QueueDepthScaling's two thresholds
    double step_thr[kMaxScalerSteps];          // StepScaling._steps as the host sorted them
    int32_t step_adj[kMaxScalerSteps];
    int32_t n_steps, policy;                   // hs_autoscaler_policy
    int64_t *hist; long long hist_cap, hist_len;   // scaling_history: (time ns, action + 4 x the instances it counted, from_count, to_count) per record
    int64_t last_time;                         // _last_scale_time (last_action != 0)
    int32_t last_action;                       // _last_scale_action: 0 None, 1 "scale_out", 2 "scale_in"
    int32_t next_id;                           // _next_instance_id
    int64_t added, removed;                    // instances_added / instances_removed
    int32_t wanted;                            // the instance id beyond the pool a scale-out asked for (kPoolOut; 0: none)
    int32_t pad;
};
constexpr int kAsOut = 1, kAsIn = 2;
// A RollingDeployer's state, one row per deployer in HBM (GVars::rd; GParam::stream_base = its row).  GParam of a deployer:
// mean = health_check_interval (seconds), conc = healthy_threshold, lim = max_failures, target = its LoadBalancer, rt_off = the slot of
// instance 1 among the LoadBalancer's targets (= its initial backends), rt_cnt = the pool's size P.  The four lists hold slots of
// the LoadBalancer, `cap` (= its targets) places each.
// A CanaryDeployer's parameters and state, one row per deployer in HBM (GVars::cn; GParam::stream_base = its row).  GParam of a canary
// deployer: mean = evaluation_interval (seconds), target = its LoadBalancer, rt_off = the canary's slot among the LoadBalancer's
// targets (= its initial backends), rt_cnt = 1.
struct GCn {
    double pct[HS_CANARY_MAX_STAGES], period[HS_CANARY_MAX_STAGES];   // CanaryStage.traffic_percentage / evaluation_period
    double ev_max, ev_mult;                    // max_error_rate / max_latency, threshold_multiplier
    double cur_pct;                            // state.canary_traffic_pct
    int64_t stage_start;                       // _stage_start_time ns (has_start)
    int32_t *base;                             // [cap] _baseline_backends as slots
    int32_t *wr;                               // [cap] 1: the strategy's set_weight was called for the slot during the run (-1: never)
    int32_t lb;                                // its LoadBalancer's node
    int32_t pad2;
    int32_t cap, n_base, n_stages, evaluator;  // hs_canary_evaluator
    int32_t status, cur_stage, total_stages;   // state.status (hs_canary_status), current_stage, total_stages
    int32_t has_start, has_canary, pad;
    int64_t started, completed, rolled_back, stages_completed, ev_performed, ev_passed, ev_failed;   // CanaryDeployerStats
};
struct GRd {
    int32_t *old_b, *new_b, *cur_old, *cur_new;    // _old_backends (from old_head on), _new_backends, _current_batch_old, _current_batch_new
    int32_t *pass;                             // [cap] _health_pass_count by slot (-1: the name has no entry)
    int32_t *readd;                            // [cap] 1: a rollback brought the backend back (a new BackendInfo, weight 1); -1: never
    int32_t cap, batch_size;
    int32_t old_head, old_n, new_n, cur_old_n, cur_new_n;
    int32_t status;                            // state.status: hs_deployment_status
    int32_t total, replaced, failed, cur_batch;    // state.total_instances / replaced / failed / current_batch
    int32_t next_id, fail_count;               // _next_instance_id, _health_fail_count
    int32_t wanted;                            // the instance id beyond the pool a batch asked for (kPoolOut; 0: none)
    int32_t lb;                                // its LoadBalancer's node
    int64_t started, completed, rolled_back, inst_replaced, hc_performed, hc_passed, hc_failed;   // RollingDeployerStats
};
constexpr int kLimPollScheduled = 1, kLimHasTime = 2;   // GState::active of a limiter: _poll_scheduled; _last_*_time / _current_window_start is set
constexpr long long kMaxSlidingLog = 1ll << 20;          // SlidingWindowPolicy.max_requests the ring is sized for

enum : int { kRunning = 0, kDone = 1, kGrowHeap = 2, kGrowReq = 4, kGrowRec = 8, kBadKind = 16, kGrowTicks = 32, kUndecided = 64, kGrowTab = 128,
             kGrowHist = 256, kPoolOut = 512 };

struct GVars {                                 // device scalars
    long long heap_len;
    unsigned long long counter;                // the heap's own counter (run-time sort indices, core/event_heap.py:48)
    unsigned long long global_counter;         // the process-wide counter (pre-run events and schedule()d Events)
    long long cur;                             // Simulation._current_time
    long long processed;
    long long by_kind[HS_EV_KINDS];
    long long completed, received;
    long long rec_n;
    int req_len, req_free;
    int booted;
    int status;
    long long sched_done;                      // scheduled entries already pushed
    long long heap_peak;
    long long coop_selects;                    // least-loaded selections all 64 lanes took (hs_graph_coop_selects)
    long long polls_pending;                   // daemon Events in the heap: the limiters' polls and the fault Events
    long long internal_by_kind[4];             // the four internal kinds as events_by_kind counts the public ones (hs_graph_get_faults)
    long long faults_cancelled;                // cancelled fault Events popped
    const GFault *faults; long long n_faults;  // the fault Events in the order FaultSchedule.start constructed them: read once, at boot
    long long health_by_kind[3];               // the checkers' cycle / response / timeout Events (hs_graph_get_health)
    long long resil_by_kind[6];                // the wrappers' request / response / timeout Events, Bulkhead then TimeoutWrapper (hs_graph_get_wrapper)
    long long client_by_kind[3];               // the Clients' request / response / timeout Events (hs_graph_get_client)
    long long flow_by_kind[HS_FLOW_KINDS];     // the flow entities' Events, kEvBpItem .. kEvGtClose (hs_graph_get_flow)
    long long flow_cancelled;                  // cancelled `_BatchTimeout` Events popped
    GQueue *qp;                                // the rows of the Servers with a queue policy (hs_graph_set_queue_policy; null: none)
    long long n_link_faults;                   // entries of `faults` that are link faults (hs_graph_add_link_fault)
    GAs *as;                                   // the rows of the AutoScalers (hs_graph_set_auto_scaler; null: none)
    uint8_t *as_mem;                           // [n_rt] the membership word of every backend slot: the backend is in LoadBalancer._backends
    long long as_evals;                        // the scalers' `_autoscaler_evaluate` Events (hs_graph_get_auto_scaler)
    GRd *rd;                                   // the rows of the RollingDeployers (hs_graph_set_rolling_deployer; null: none)
    long long rd_by_kind[HS_DEPLOYER_KINDS];   // the deployers' Events by kind (hs_graph_get_rolling_deployer)
    GCn *cn;                                   // the rows of the CanaryDeployers (hs_graph_set_canary_deployer; null: none)
    long long cn_by_kind[HS_CANARY_KINDS];     // the canary deployers' Events by kind (hs_graph_get_canary_deployer)
    double *svc_sum; long long *svc_cnt;       // [n] per node: Server._service_times as a running left-to-right sum and a count, taken at the
                                               // draw (graphs with a CanaryDeployer; null: none)
    int n_rd, n_cn;                            // rows of `rd` / `cn`
    long long rd_compactions[2];               // member lists compacted behind a removal: by the lone lane, by all 64 lanes
    int rd_coop_min;                           // a removal from a list of >= this many members is compacted by all 64 lanes (0: never)
    GHg *hg;                                   // the rows of the Hedges and Fallbacks (hs_graph_set_hedge / hs_graph_set_fallback; null: none)
    long long hg_by_kind[HS_HEDGE_KINDS];      // their Events by kind, kEvHgReq .. kEvFbFbResp (hs_graph_get_hedge)
    long long st_by_kind[HS_STOCK_KINDS];      // the pools' and buffers' Events by kind, kEvPcItem .. kEvIbReplenish (hs_graph_get_pool)
};

struct GCtl {                                  // kernel argument
    GEvent *heap; long long heap_cap;
    GRequest *reqs; int req_cap;
    int32_t *rec_node; int64_t *rec_t, *rec_cr; long long rec_cap;
    const GParam *P; GState *S; int n;
    const int32_t *rt_targets; long long *rt_taken;
    const int32_t *sched_node; const int64_t *sched_t; long long n_sched;
    // tick tables (hs_tables.hpp) of the time-varying Sources and the Probes: tick k of row r at ticks[r * tick_cap + k]; a row
    // holds tick_count[r] ticks -- up to two beyond the horizon it was computed for, or up to the stream's end (kInfNs)
    const int64_t *ticks; long long tick_cap; const int64_t *tick_count;
    const int32_t *key_table;                  // ConsistentHash / IPHash .select(str(client id)) as a backend slot, per LoadBalancer (GParam::lim);
                                               // WeightedRoundRobin: one period of its selection sequence
    int32_t *lb_w;                             // [n_rt] the weighted strategies' weight of every backend slot (strategy._weights; default 1);
                                               // written during a run by the deployer instantiation alone (add_backend's set_weight)
    int coop_reset;                            // 1: the first launch of a run -- the lone lane zeroes GVars::coop_selects (the host clears it after the launch)
    int64_t *lim_ring;                         // SlidingWindowPolicy._request_log of every such limiter: a ring at GParam::rt_off of GParam::rt_cnt entries
    int auto_term;                             // 1: end_ns = 2^61 (end_time = Infinity) -- the run ends when only daemon Events (polls, faults) are pending
    int coop_min;                              // least-loaded selections over >= this many backends go to all 64 lanes; 0: never (no such
                                               // LoadBalancer in the graph, or the lane-serial scan is forced)
    GVars *V;
    uint64_t seed;
    int64_t start_ns, end_ns;
    long long budget;
    int part;                                  // 1: this heap holds PART of a Simulation (hs_graph_run_parts); 2: ... and runs its one Event beyond the end
    // Backend health (LoadBalancer.mark_unhealthy / mark_healthy, load_balancer.py:244-297): only a graph with a HealthChecker or a
    // backend marked unhealthy before the run has these (health = 1); every array is indexed like rt_targets
    int health;
    uint8_t *hl_flag;                          // BackendInfo.is_healthy of every backend slot
    int32_t *hl_list;                          // per LoadBalancer at its rt_off: its healthy slots, ascending (= `healthy_backends`); GState::qlen of them
    long long *wrr_cur;                        // WeightedRoundRobin._current_weights of every backend slot (they persist while a backend is out)
    GHc *hc;                                   // the checker's state of every backend slot
    // Bulkhead / TimeoutWrapper `_in_flight`: the live request ids of every wrapper, unordered, GParam::rt_cnt places at GParam::rt_off
    // (a Bulkhead holds GState::active of them, a TimeoutWrapper GState::qlen)
    int64_t *rs_tab;
    // Client: `_in_flight` lives in rs_tab as well, two words per place -- the key, then start_time in ns -- GState::qlen places in use;
    const int64_t *cl_delays;                  // Duration.from_seconds(policy.get_delay(a)) in ns for a = 1 .. max_attempts - 1 of every Client (GParam::lim)
    const int32_t *sched_id;                   // request_id of every scheduled entry (0: none; read for Client nodes only; null without any)
};

__device__ __forceinline__ bool ev_lt(const GEvent &a, const GEvent &b) {   // Event.__lt__, core/event.py:337-344
    if (a.t != b.t) return a.t < b.t;
    return a.idx < b.idx;
}

// The window's entries are addressed as LDS (address space 3), two 16-byte words each: a pointer that may be LDS or HBM compiles to FLAT
// loads and stores, which wait on both memory counters (113 + 118 of them in the loop before: every level of a sift).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
template <int W>
struct Heap {
    lds_u32x4 *lds; GEvent *glob; long long len;
    __device__ __forceinline__ GEvent get(long long i) const {
        if (i < W) {
            const u32x4 a = lds[2 * i], b = lds[2 * i + 1];
            GEvent e;
            e.t = (int64_t)(((uint64_t)a.y << 32) | (uint64_t)a.x); e.idx = ((uint64_t)a.w << 32) | (uint64_t)a.z;
            e.node = (int32_t)b.x; e.req = (int32_t)b.y; e.kind = b.z; e.pad = b.w;
            return e;
        }
        return glob[i];
    }
    __device__ __forceinline__ void set(long long i, const GEvent &e) {
        if (i < W) {
            u32x4 a, b;
            a.x = (uint32_t)(uint64_t)e.t; a.y = (uint32_t)((uint64_t)e.t >> 32); a.z = (uint32_t)e.idx; a.w = (uint32_t)(e.idx >> 32);
            b.x = (uint32_t)e.node; b.y = (uint32_t)e.req; b.z = e.kind; b.w = e.pad;
            lds[2 * i] = a; lds[2 * i + 1] = b;
        } else glob[i] = e;
    }
    // heapq.heappush: append, then _siftdown(heap, 0, len - 1)
    __device__ inline void push(const GEvent &e) {
        long long pos = len++;
        while (pos > 0) {
            const long long parent = (pos - 1) >> 1;
            const GEvent p = get(parent);
            if (!ev_lt(e, p)) break;
            set(pos, p);
            pos = parent;
        }
        set(pos, e);
    }
    // heapq.heappop: the last leaf replaces the root; _siftup walks the hole down to a leaf along the smaller child (the right
    // one unless left < right), then _siftdown bubbles the moved item back up
    __device__ inline GEvent pop() {
        const GEvent top = get(0);
        const GEvent last = get(--len);
        const long long n = len;
        if (n == 0) return top;
        long long pos = 0, child = 1;
        while (child < n) {
            GEvent c = get(child);
            const long long right = child + 1;
            if (right < n) {
                const GEvent r = get(right);
                if (!ev_lt(c, r)) { child = right; c = r; }
            }
            set(pos, c);
            pos = child;
            child = 2 * pos + 1;
        }
        while (pos > 0) {
            const long long parent = (pos - 1) >> 1;
            const GEvent p = get(parent);
            if (!ev_lt(last, p)) break;
            set(pos, p);
            pos = parent;
        }
        set(pos, last);
        return top;
    }
};

__device__ __forceinline__ double uniform_at(uint64_t seed, uint64_t sid, uint64_t k) {
    Stream s;
    s.init(seed, sid, k);
    return s.next_uniform();
}

// a Request-carrying Event aimed at `node`: which handler it lands in (Entity.handle_event of that class)
template <int L>
__device__ __forceinline__ uint32_t arrival_kind(const GParam *P, int node) {
    constexpr bool R = L >= kLvResilience, CL = L >= kLvClient, FL = L >= kLvFlow, HG = L >= kLvHedge, ST = L >= kLvStock;
    if constexpr (ST) {
        if (P[node].kind == HS_NODE_POOLED_CYCLE) return kEvPcItem;
        if (P[node].kind == HS_NODE_INVENTORY) return kEvIbItem;
    }
    if constexpr (HG) {
        if (P[node].kind == HS_NODE_HEDGE) return kEvHgReq;
        if (P[node].kind == HS_NODE_FALLBACK) return kEvFbReq;
    }
    if constexpr (FL) {
        if (P[node].kind == HS_NODE_BATCH_PROCESSOR) return kEvBpItem;
        if (P[node].kind == HS_NODE_CONVEYOR) return kEvCvItem;
        if (P[node].kind == HS_NODE_GATE) return kEvGtItem;
    }
    if constexpr (CL) {
        if (P[node].kind == HS_NODE_CLIENT) return kEvClReq;
    }
    if constexpr (R) {                         // (the wrappers exist in the one instantiation that dispatches their kinds)
        if (P[node].kind == HS_NODE_BULKHEAD) return kEvBhReq;
        if (P[node].kind == HS_NODE_TIMEOUT_WRAPPER) return kEvTwReq;
    }
    switch (P[node].kind) {
        case HS_NODE_SERVER: return HS_EV_ENQUEUE;
        case HS_NODE_SINK: return HS_EV_SINK;
        case HS_NODE_LINK: return HS_EV_LINK;
        case HS_NODE_ROUTER: return HS_EV_ROUTE;
        case HS_NODE_LB: return HS_EV_LB;
        case HS_NODE_RATE_LIMITER: return kEvLimRequest;
        default: return 0xffffffffu;
    }
}

__device__ __forceinline__ GEvent mk(int64_t t, uint64_t idx, uint32_t kind, int node, int req) {
    GEvent e;
    e.t = t; e.idx = idx; e.node = node; e.req = req; e.kind = kind; e.pad = 0;
    return e;
}
// ... one constructed BEFORE the run: its index comes from the process-wide counter (core/event.py:53-67), the run's own events count
// from zero again -- GEvent::pad tells the two apart (part runs: a timestamp group that mixes them is order-sensitive to ALL of a
// Simulation's events, hs_graph_run_parts)
__device__ __forceinline__ GEvent mk_pre(int64_t t, uint64_t idx, uint32_t kind, int node, int req) {
    GEvent e = mk(t, idx, kind, node, req);
    e.pad = 1;
    return e;
}

// ArrivalTimeProvider.next_arrival_time, constant-rate fast path (load/arrival_time_provider.py:72-82) with the target area of
// poisson_arrival.py:31 / constant_arrival.py:23
__device__ inline int64_t next_arrival(const GCtl &c, int n) {
    const GParam &p = c.P[n];
    GState &s = c.S[n];
    if (p.rt_off >= 0) {                       // a time-varying profile: tick number `generated` of the Source's table
        const int64_t a2 = c.ticks[(size_t)p.rt_off * (size_t)c.tick_cap + (size_t)s.c];
        s.a = a2;
        return a2;
    }
    double area = 1.0;
    if (p.sub == HS_SRC_POISSON) {
        area = exp1_from_uniform(uniform_at(c.seed, stream_id(p.stream_base, kStreamArrival), (uint64_t)s.b));
        s.b += 1;
    }
    const int64_t a2 = ns_from_seconds(__dadd_rn(seconds_from_ns(s.a), __ddiv_rn(area, p.mean)));
    s.a = a2;
    return a2;
}

// LeastConnections._get_connections (strategies.py:163-177: Server.active_requests) / WeightedLeastConnections._get_score (:227-231:
// connections / weight, a true division of two ints = the correctly rounded binary64 quotient)
__device__ __forceinline__ double lb_score(const GCtl &c, const GParam &p, int slot) {
    const int be = c.rt_targets[p.rt_off + slot];
    const double act = (double)c.S[be].active;
    return p.sub == HS_LB_WEIGHTED_LEAST_CONNECTIONS ? __ddiv_rn(act, (double)c.lb_w[p.rt_off + slot]) : act;
}

// ---- rate limiter policies (components/rate_limiter/policy.py), the reference's binary64 operations one by one --------------------
// GParam of a limiter: sub = hs_limiter_policy, lim = FIFO capacity, conc = max_requests / requests_per_window,
//   TokenBucket: lat_min = capacity, mean = refill_rate;  LeakyBucket: mean = leak_rate, lat_min = _leak_interval;
//   SlidingWindow / FixedWindow: mean = the window in seconds; SlidingWindow: rt_off / rt_cnt = its ring in GCtl::lim_ring.

// fmod(x, y) for finite x >= 0 and normal y > 0, exactly (the remainder of the two significands as integers, one binary digit of the
// quotient per step): the C library's result, which CPython's float floor division starts from (Objects/floatobject.c float_divmod)
__device__ inline double exact_fmod_pos(double x, double y) {
    if (x < y) return x;
    const uint64_t bx = (uint64_t)__double_as_longlong(x), by = (uint64_t)__double_as_longlong(y);
    const int ex = (int)(bx >> 52), ey = (int)(by >> 52);                      // (x >= y > 0 normal: both biased exponents >= 1)
    const uint64_t mx = (bx & 0xfffffffffffffull) | (1ull << 52), my = (by & 0xfffffffffffffull) | (1ull << 52);
    uint64_t r = mx % my;
    for (int i = ex - ey; i > 0; --i) { r <<= 1; if (r >= my) r -= my; }      // (r < my < 2^53: no overflow)
    return ldexp((double)r, ey - 1075);                                       // r < my: at most y's own digits, exact
}
// Python's `v // w` on floats for v >= 0, w > 0 (float_floor_div: fmod, the exact quotient of the rest, floor with its half-way fix-up)
__device__ inline double py_floordiv_pos(double v, double w) {
    const double mod = exact_fmod_pos(v, w);
    const double div = __ddiv_rn(__dsub_rn(v, mod), w);
    if (div == 0.0) return 0.0;
    double fl = floor(div);
    if (__dsub_rn(div, fl) > 0.5) fl = __dadd_rn(fl, 1.0);
    return fl;
}
__device__ __forceinline__ int64_t &lim_count(GState &s) { return *reinterpret_cast<int64_t *>(&s.total_service); }
__device__ inline void lim_token_refill(const GParam &p, GState &s, int64_t now) {           // TokenBucketPolicy._refill
    if (!(s.active & kLimHasTime)) { s.active |= kLimHasTime; s.svc_draws = (uint64_t)now; return; }
    const double elapsed = seconds_from_ns(now - (int64_t)s.svc_draws);
    if (elapsed <= 0.0) return;
    const double x = __dadd_rn(s.total_service, __dmul_rn(elapsed, p.mean));
    s.total_service = x < p.lat_min ? x : p.lat_min;                                          // min(capacity, x)
    s.svc_draws = (uint64_t)now;
}
__device__ inline void lim_sliding_prune(const GCtl &c, const GParam &p, GState &s, int64_t now) {   // SlidingWindowPolicy._prune
    const int64_t cutoff = now - ns_from_seconds(p.mean);
    int64_t &cnt = lim_count(s);
    while (cnt > 0 && c.lim_ring[p.rt_off + (int64_t)s.svc_draws] < cutoff) {
        s.svc_draws = s.svc_draws + 1 == (uint64_t)p.rt_cnt ? 0 : s.svc_draws + 1;
        cnt -= 1;
    }
}
__device__ inline void lim_fixed_reset(const GParam &p, GState &s, int64_t now) {             // FixedWindowPolicy._maybe_reset
    const int64_t ws = ns_from_seconds(__dmul_rn(py_floordiv_pos(seconds_from_ns(now), p.mean), p.mean));
    if (!(s.active & kLimHasTime) || ws > (int64_t)s.svc_draws) { s.active |= kLimHasTime; s.svc_draws = (uint64_t)ws; lim_count(s) = 0; }
}
// CoDelQueue._control_law (codel.py:246-250): Duration.from_seconds(interval / math.sqrt(count)) in ns -- the correctly rounded root
// and quotient, the product with 1e9 truncated
__device__ __forceinline__ int64_t codel_next_ns(int64_t count, double interval) {
    return ns_from_seconds(__ddiv_rn(interval, __dsqrt_rn(__ll2double_rn(count))));
}
// ... one (count, interval) pair per thread (hs_debug_codel_next)
__global__ void hs_debug_codel_next_kernel(int64_t n, const int64_t *count, const double *interval, int64_t *out_ns) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out_ns[i] = codel_next_ns(count[i], interval[i]);
}
// FixedWindowPolicy._get_window_start, one input per thread (hs_debug_window_start)
__global__ void hs_debug_window_start_kernel(int64_t n, const int64_t *now_ns, const double *w, double *out_div, int64_t *out_start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double div = py_floordiv_pos(seconds_from_ns(now_ns[i]), w[i]);
    out_div[i] = div;
    out_start[i] = ns_from_seconds(__dmul_rn(div, w[i]));
}
__device__ inline bool lim_try_acquire(const GCtl &c, const GParam &p, GState &s, int64_t now) {
    switch (p.sub) {
    case HS_LIMITER_TOKEN_BUCKET:
        lim_token_refill(p, s, now);
        if (s.total_service >= 1.0) { s.total_service = __dsub_rn(s.total_service, 1.0); return true; }
        return false;
    case HS_LIMITER_LEAKY_BUCKET:
        if (!(s.active & kLimHasTime)) { s.active |= kLimHasTime; s.svc_draws = (uint64_t)now; return true; }
        if (seconds_from_ns(now - (int64_t)s.svc_draws) >= p.lat_min) { s.svc_draws = (uint64_t)now; return true; }
        return false;
    case HS_LIMITER_SLIDING_WINDOW: {
        lim_sliding_prune(c, p, s, now);
        int64_t &cnt = lim_count(s);
        if (cnt < (int64_t)p.conc) {
            int64_t at = (int64_t)s.svc_draws + cnt;
            if (at >= p.rt_cnt) at -= p.rt_cnt;
            c.lim_ring[p.rt_off + at] = now;
            cnt += 1;
            return true;
        }
        return false;
    }
    default: {
        lim_fixed_reset(p, s, now);
        int64_t &cnt = lim_count(s);
        if (cnt < (int64_t)p.conc) { cnt += 1; return true; }
        return false;
    }
    }
}
// policy.time_until_available(now) in nanoseconds, with the three `wait == Duration.ZERO -> Duration(1)` guards (and LeakyBucket's)
__device__ inline int64_t lim_wait_ns(const GCtl &c, const GParam &p, GState &s, int64_t now) {
    int64_t wait;
    switch (p.sub) {
    case HS_LIMITER_TOKEN_BUCKET:
        lim_token_refill(p, s, now);
        if (s.total_service >= 1.0) return 0;
        wait = ns_from_seconds(__ddiv_rn(__dsub_rn(1.0, s.total_service), p.mean));
        break;
    case HS_LIMITER_LEAKY_BUCKET: {
        if (!(s.active & kLimHasTime)) return 0;
        const double remaining = __dsub_rn(p.lat_min, seconds_from_ns(now - (int64_t)s.svc_draws));
        if (remaining <= 0.0) return 0;
        wait = ns_from_seconds(remaining);
    } break;
    case HS_LIMITER_SLIDING_WINDOW: {
        lim_sliding_prune(c, p, s, now);
        if (lim_count(s) < (int64_t)p.conc) return 0;
        const int64_t expires = c.lim_ring[p.rt_off + (int64_t)s.svc_draws] + ns_from_seconds(p.mean);
        wait = ns_from_seconds(seconds_from_ns(expires - now));
    } break;
    default: {
        lim_fixed_reset(p, s, now);
        if (lim_count(s) < (int64_t)p.conc) return 0;
        const double remaining = seconds_from_ns((int64_t)s.svc_draws + ns_from_seconds(p.mean) - now);
        if (remaining <= 0.0) return 0;
        wait = ns_from_seconds(remaining);
    } break;
    }
    return wait == 0 ? 1 : wait;
}

// LoadBalancer.mark_healthy / mark_unhealthy (load_balancer.py:244-297) of backend `slot`: the flag, the mark counter and the list of
// healthy slots, kept ascending (marks are rare, selections are not).  A plain method call in the reference: it takes effect whatever
// the LoadBalancer's own `_crashed` flag says.  Returns false when the backend was in that state already.
__device__ inline bool lb_mark(const GCtl &c, int lb, int slot, bool healthy) {
    const GParam &lp = c.P[lb];
    GState &ls = c.S[lb];
    uint8_t &flag = c.hl_flag[lp.rt_off + slot];
    if ((flag != 0) == healthy) return false;
    flag = healthy ? 1 : 0;
    int32_t *hl = c.hl_list + lp.rt_off;
    int nh = ls.qlen;
    if (healthy) {
        int i = nh;
        while (i > 0 && hl[i - 1] > slot) { hl[i] = hl[i - 1]; --i; }
        hl[i] = slot;
        ls.qlen = nh + 1; ls.qtail += 1;
    } else {
        int i = 0;
        while (i < nh && hl[i] != slot) ++i;
        for (; i + 1 < nh; ++i) hl[i] = hl[i + 1];
        ls.qlen = nh - 1; ls.qhead += 1;
    }
    return true;
}

// A wrapper's response / timeout Event with its request id (GEvent::pad above the flag bits, GEvent::req beyond 30 bits)
__device__ __forceinline__ GEvent mk_id(int64_t t, uint64_t idx, uint32_t kind, int node, int64_t id) {
    GEvent e = mk(t, idx, kind, node, -2 - (int)(id >> 30));
    e.pad = (uint32_t)(id & 0x3fffffffll) << kPadIdShift;
    return e;
}
__device__ __forceinline__ int64_t ev_id(const GEvent &e) { return ((int64_t)(-2 - e.req) << 30) | (int64_t)(e.pad >> kPadIdShift); }
__device__ __forceinline__ int64_t req_id(const GRequest &q) { return __double_as_longlong(q.service_s); }
// the `_bh_response` / `_tw_response` / `_client_response` kind of a hook's owner
// (a Fallback's two hooks differ by the flag bit of the key that rode on the Request)
template <int L>
__device__ __forceinline__ uint32_t hook_resp_kind(uint8_t hk, [[maybe_unused]] int64_t key = 0) {
    constexpr bool CL = L >= kLvClient, HG = L >= kLvHedge;
    if constexpr (HG) {
        if (hk == HS_NODE_HEDGE) return kEvHgResp;
        if (hk == HS_NODE_FALLBACK) return (key & kHgFlag) ? kEvFbFbResp : kEvFbPrimResp;
    }
    if constexpr (CL) {
        if (hk == HS_NODE_CLIENT) return kEvClResp;
    }
    return hk == HS_NODE_BULKHEAD ? kEvBhResp : kEvTwResp;
}
template <int L>
__device__ __forceinline__ bool hook_has_id(uint8_t hk) {
    constexpr bool CL = L >= kLvClient, HG = L >= kLvHedge;
    if constexpr (HG) {
        if (hk == HS_NODE_HEDGE || hk == HS_NODE_FALLBACK) return true;
    }
    if constexpr (CL) {
        if (hk == HS_NODE_CLIENT) return true;
    }
    return hk == HS_NODE_BULKHEAD || hk == HS_NODE_TIMEOUT_WRAPPER;
}
// `request_id in self._in_flight` and its removal: the live ids are unordered, the last one takes the place of the one that leaves
__device__ inline bool tab_remove(int64_t *tab, int live, int64_t id) {
    for (int i = 0; i < live; ++i)
        if (tab[i] == id) { tab[i] = tab[live - 1]; return true; }
    return false;
}

// A Hedge's / Fallback's table (GHg): the place of `id`, -1 when it is not there.  The table is at most half full, so every probe
// meets an empty place.
__device__ inline long long hg_find(const GHg &row, int64_t id) {
    const long long mask = row.cap - 1;
    for (long long i = id & mask;; i = (i + 1) & mask) {
        const int64_t at = row.tab[i].id;
        if (at == id) return i;
        if (at == 0) return -1;
    }
}
// ... a new entry (room: tested in front of the pop)
__device__ inline void hg_insert(const GHg &row, const GHgEnt &ent) {
    const long long mask = row.cap - 1;
    long long i = ent.id & mask;
    while (row.tab[i].id != 0) i = (i + 1) & mask;
    row.tab[i] = ent;
}
// ... and `del self._in_flight[id]` of the entry at place `i`: every later entry of the cluster whose home place does not lie
// cyclically in (hole, its place] moves back into the hole, so no probe sequence is ever cut
__device__ inline void hg_remove(const GHg &row, long long i) {
    const long long mask = row.cap - 1;
    for (long long j = (i + 1) & mask; row.tab[j].id != 0; j = (j + 1) & mask) {
        const long long k = row.tab[j].id & mask;
        if (i <= j ? (i < k && k <= j) : (i < k || k <= j)) continue;
        row.tab[i] = row.tab[j];
        i = j;
    }
    row.tab[i].id = 0;
}

// NL: graphs of up to NL nodes keep their nodes' parameters and state in LDS for the launch (the loop's dependent chain goes
// through them several times per event: 64-cycle LDS round trips instead of L2's) -- `lnodes`: NL x (GParam + GState).
// L: the level (kLvPlain ... kLvStock, above), which decides what code the instantiation carries.
// A LoadBalancer's member list `hl` (`len` slots in insertion order) compacted by the membership words `mem` (by slot), order kept;
// the new length.  On the lone lane ...
__device__ inline int compact_members_lone(int32_t *hl, const uint8_t *mem, int len) {
    int w = 0;
    for (int q = 0; q < len; ++q) { const int sl = hl[q]; if (mem[sl]) hl[w++] = sl; }
    return w;
}
// ... and by all 64 lanes of the one wavefront: per chunk of 64 entries a ballot of the entries that stay and a prefix count of the
// lanes below.  Every lane has read its entry of a chunk before any lane writes one (one wavefront, in program order), and an entry
// only ever moves towards the front.  Every lane returns the new length.
__device__ inline int compact_members_wave(int32_t *hl, const uint8_t *mem, int len, int lane) {
    int w = 0;
    for (int base = 0; base < len; base += 64) {
        const int q = base + lane;
        const int sl = q < len ? hl[q] : 0;
        const bool keep = q < len && mem[sl] != 0;
        const unsigned long long stay = __ballot(keep);
        const int pos = w + __popcll(stay & ((1ull << lane) - 1ull));
        if (keep) hl[pos] = sl;
        w += __popcll(stay);
    }
    return w;
}

template <int W, int NL, int L = kLvPlain>
__device__ __forceinline__ void graph_loop(const GCtl &c0, GEvent *lheap, char *lnodes) {
    constexpr bool F = L >= kLvFaults, HC = L >= kLvHealth, R = L >= kLvResilience, CL = L >= kLvClient, FL = L >= kLvFlow,
                   Q = L >= kLvQueues, LF = L >= kLvLinkFaults, AS = L >= kLvScaler, DP = L >= kLvDeploy, HG = L >= kLvHedge,
                   ST = L >= kLvStock;
    constexpr uint32_t kKinds = kLevelKinds[L];            // the kinds this instantiation dispatches (any other: kBadKind)
    // (one word for the instantiations whose kinds fit in it, two from the flow instantiation's 39 on)
    constexpr std::conditional_t<FL, uint64_t, uint32_t> kDrop = (std::conditional_t<FL, uint64_t, uint32_t>)kLevelDrop[L];
    constexpr int kPushes = R ? 3 : 2;         // heap entries one event constructs at most (R: a limiter's forward or poll + the hook's response)
    __shared__ unsigned long long s_by_kind[kKinds];
    __shared__ int s_want;                     // the LoadBalancer whose least-loaded selection the lone lane hands to the wavefront (-1: none)
    GCtl c = c0;
    GVars &V = *c.V;
    const int lane = threadIdx.x;
    const bool nodes_in_lds = c.n <= NL;
    if (nodes_in_lds) {
        const long long n8 = (long long)c.n * (long long)(sizeof(GParam) / 8);
        static_assert(sizeof(GParam) == sizeof(GState), "one copy loop for both");
        const uint64_t *sp = reinterpret_cast<const uint64_t *>(c0.P), *ss = reinterpret_cast<const uint64_t *>(c0.S);
        uint64_t *dp = reinterpret_cast<uint64_t *>(lnodes), *ds = reinterpret_cast<uint64_t *>(lnodes + (size_t)NL * sizeof(GParam));
        for (long long i = lane; i < n8; i += 64) { dp[i] = sp[i]; ds[i] = ss[i]; }
        c.P = reinterpret_cast<const GParam *>(lnodes);
        c.S = reinterpret_cast<GState *>(lnodes + (size_t)NL * sizeof(GParam));
    }
    if (lane < (int)kKinds) s_by_kind[lane] = 0ull;
    {   // the heap's head comes into LDS (all 64 lanes copy; 8 bytes per lane and step)
        const long long n8 = (V.heap_len < W ? V.heap_len : (long long)W) * (long long)(sizeof(GEvent) / 8);
        const uint64_t *src = reinterpret_cast<const uint64_t *>(c.heap);
        uint64_t *dst = reinterpret_cast<uint64_t *>(lheap);
        for (long long i = lane; i < n8; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    // The lone lane's registers live across the outer loop below (the other 63 lanes carry copies they never use).
    int req_free = V.req_free, req_len = V.req_len;                         // (registers for the launch)
    Heap<W> H{(lds_u32x4 *)lheap, c.heap, V.heap_len};
    unsigned long long G = V.counter;
    int status = kRunning;
    int sel = -1, sel_node = -1;               // a selection the wavefront made for the LoadBalancer event on top of the heap
    long long cur = V.cur, processed = 0, n_completed = 0, n_received = 0, rec_n = V.rec_n, n_coop = 0;
    long long peak = V.heap_peak;
    long long polls_pending = V.polls_pending;   // daemon Events in the heap: they do not keep an auto-terminating run alive
    long long n_cancelled = 0;
    [[maybe_unused]] long long n_flow_cancelled = 0;
    [[maybe_unused]] const bool lf_graph = LF && V.n_link_faults > 0;   // (a handle without link faults in a batch with one: the plain link)
    if (lane == 0) {
        if (!V.booted) {
            // Simulation.__init__ (core/simulation.py:145-154) + Source.start (load/source.py:120-140): the Sources in list order,
            // their first SourceEvents numbered by the process-wide counter
            unsigned long long g = 0;
            for (int i = 0; i < c.n; ++i) {
                if (c.P[i].kind != HS_NODE_SOURCE) continue;
                c.S[i].a = c.start_ns;                          // provider.current_time = start_time
                const int64_t t = next_arrival(c, i);
                if (t == kInfNs) continue;                      // "Rate is zero indefinitely. Source will not start." (source.py:137-139)
                H.push(mk_pre(t, g++, HS_EV_SOURCE, i, -1));    // (heap_cap >= 4 n: hs_graph_create)
            }
            for (int i = 0; i < c.n; ++i) {                     // then the probes, in list order (core/simulation.py:156-160)
                if (c.P[i].kind != HS_NODE_PROBE) continue;
                const int64_t t = c.ticks[(size_t)c.P[i].rt_off * (size_t)c.tick_cap];
                if (t == kInfNs) continue;
                H.push(mk_pre(t, g++, HS_EV_PROBE_TICK, i, -1));
            }
            // then the fault Events (FaultSchedule.start, core/simulation.py:162-169): daemons, in add() order
            if constexpr (F) {
                const GFault *faults = V.faults;
                const long long n_faults = V.n_faults;
                for (long long i = 0; i < n_faults; ++i) {      // (heap_cap >= n + n_faults: prepare_run)
                    const GFault f = faults[i];
                    GEvent fe = mk_pre(f.t, g++, (f.flags & 1u) ? kEvFaultOn : kEvFaultOff, f.node, -1);
                    if (f.flags & 2u) fe.pad |= kPadCancelled;
                    if constexpr (LF) {
                        if (f.flags >> kFaultWhatShift) fe.pad |= (uint32_t)(i + 1) << kPadIdShift;   // (at most 2^24 entries)
                    }
                    H.push(fe);
                    polls_pending += 1;
                }
            }
            V.global_counter = g; V.booted = 1; G = 0; V.cur = c.start_ns;
        }
        // Simulation.schedule (core/simulation.py:195-206): Events constructed outside the run
        while (status == kRunning && V.sched_done < c.n_sched) {
            if (H.len + 1 > c.heap_cap) { status |= kGrowHeap; break; }
            if constexpr (HC) {
                // HealthChecker.start() (health_check.py:201-216): the first _health_check_cycle Event, no Request
                const int hn = c.sched_node[V.sched_done];
                if (c.P[hn].kind == HS_NODE_HEALTH_CHECKER) {
                    H.push(mk_pre(c.sched_t[V.sched_done], V.global_counter++, kEvHcCycle, hn, -1));
                    V.sched_done++;
                    continue;
                }
            }
            if constexpr (CL) {
                // an Event aimed at a Client (Client.send_request's, or a plain one: request_id None): its key, attempt 1, no Request
                const int cn = c.sched_node[V.sched_done];
                if (c.P[cn].kind == HS_NODE_CLIENT) {
                    const int64_t id = c.sched_id ? (int64_t)c.sched_id[V.sched_done] : 0;
                    GEvent ce = mk_id(c.sched_t[V.sched_done], V.global_counter++, kEvClReq, cn, id | (1ll << kKeyAttemptShift));
                    ce.pad |= kPadPre;
                    H.push(ce);
                    V.sched_done++;
                    continue;
                }
            }
            if constexpr (FL) {
                // one Event of GateController.start_events() (gate_controller.py:89-111): `_GateOpen` / `_GateClose`, a daemon, no Request
                const int gn = c.sched_node[V.sched_done];
                const int32_t what = c.sched_id ? c.sched_id[V.sched_done] : 0;
                if (c.P[gn].kind == HS_NODE_GATE && what < 0) {
                    H.push(mk_pre(c.sched_t[V.sched_done], V.global_counter++, what == -1 ? kEvGtOpen : kEvGtClose, gn, -1));
                    polls_pending += 1;
                    V.sched_done++;
                    continue;
                }
            }
            if constexpr (AS) {
                // AutoScaler.start() (auto_scaler.py:302-315): the first `_autoscaler_evaluate` Event, a daemon, no Request
                const int an = c.sched_node[V.sched_done];
                if (c.P[an].kind == HS_NODE_AUTO_SCALER) {
                    H.push(mk_pre(c.sched_t[V.sched_done], V.global_counter++, kEvAsEval, an, -1));
                    polls_pending += 1;
                    V.sched_done++;
                    continue;
                }
            }
            if constexpr (DP) {
                // RollingDeployer.deploy() (rolling_deployer.py:145-156): a `_rolling_deploy_start` Event, no daemon, no Request
                const int dn = c.sched_node[V.sched_done];
                if (c.P[dn].kind == HS_NODE_ROLLING_DEPLOYER || c.P[dn].kind == HS_NODE_CANARY_DEPLOYER) {   // (`_canary_deploy_start` likewise)
                    H.push(mk_pre(c.sched_t[V.sched_done], V.global_counter++, c.P[dn].kind == HS_NODE_ROLLING_DEPLOYER ? kEvRdStart : kEvCnStart, dn, -1));
                    V.sched_done++;
                    continue;
                }
            }
            int r = req_free;
            if (r >= 0) req_free = c.reqs[r].next;
            else if (req_len < c.req_cap) r = req_len++;
            else { status |= kGrowReq; break; }
            const int node = c.sched_node[V.sched_done];
            const int64_t t = c.sched_t[V.sched_done];
            GRequest q; q.created = t; q.idx = V.global_counter; q.service_s = 0.0; q.client = -1; q.next = -1; q.hook = -1; q.pre = 1;
            c.reqs[r] = q;
            H.push(mk_pre(t, V.global_counter++, arrival_kind<L>(c.P, node), node, r));
            V.sched_done++;
        }
        cur = V.cur;
    }
    // Wave-uniform outer loop: the lone lane walks the event loop until it ends or until the event on top of the heap is a least-loaded
    // selection over many backends; that one all 64 lanes take (an O(B) scan is no work for one lane), then the lone lane goes on.
    for (;;) {
      int want = -1;
      if (lane == 0) {
        while (status == kRunning) {
            // core/simulation.py:472 tests the PREVIOUS event's time; a PART of a Simulation stops in front of the first event beyond
            // the end (which of the parts' first events the reference still processes is decided across all of them)
            if (!(H.len > (c.auto_term ? polls_pending : 0) && (c.part ? H.get(0).t <= c.end_ns : cur <= c.end_ns))) { status = kDone; break; }
            if (processed >= c.budget) break;
            // room for whatever this event constructs (at most two pushes, one Request, one record)
            if (H.len + kPushes > c.heap_cap) { status |= kGrowHeap; break; }
            if (req_free < 0 && req_len >= c.req_cap) { status |= kGrowReq; break; }
            if (rec_n >= c.rec_cap) { status |= kGrowRec; break; }
            if (c.ticks != nullptr) {                                              // the next tick of a table-driven stream must be in its table
                const GEvent top = H.get(0);
                if (top.kind == HS_EV_SOURCE || top.kind == HS_EV_PROBE_TICK) {
                    const GParam &tp = c.P[top.node];
                    if (tp.rt_off >= 0) {
                        const int64_t need = (top.kind == HS_EV_SOURCE ? c.S[top.node].c : c.S[top.node].a) + 1;
                        const int64_t cnt = c.tick_count[tp.rt_off];
                        if (need >= cnt && c.ticks[(size_t)tp.rt_off * (size_t)c.tick_cap + (size_t)(cnt - 1)] != kInfNs && top.t >= cur) {
                            status |= kGrowTicks; break;
                        }
                    }
                }
            }
            if constexpr (HC) {
                const GEvent top = H.get(0);
                if (top.kind == kEvHcCycle && top.t >= cur) {                      // a cycle constructs two Events and one Request per backend
                    const long long nb = c.P[c.P[top.node].target].rt_cnt;
                    if (H.len + 2 * nb + 1 > c.heap_cap) { status |= kGrowHeap; break; }
                    long long room = (long long)c.req_cap - (long long)req_len;    // never-used entries, then as much of the free list as it takes
                    for (int r = req_free; r >= 0 && room < nb; r = c.reqs[r].next) room += 1;
                    if (room < nb) { status |= kGrowReq; break; }
                }
            }
            if constexpr (R) {
                const GEvent top = H.get(0);                                       // a TimeoutWrapper's table has a place for the id it is about to take
                if (top.kind == kEvTwReq && c.S[top.node].qlen >= c.P[top.node].rt_cnt) { status |= kGrowTab; break; }
                if constexpr (CL) {                                                // ... and a Client's for the key
                    if (top.kind == kEvClReq && c.S[top.node].qlen >= c.P[top.node].rt_cnt) { status |= kGrowTab; break; }
                }
            }
            if constexpr (HG) {
                const GEvent top = H.get(0);                                       // a Hedge's / Fallback's table stays at most half full
                if ((top.kind == kEvHgReq || top.kind == kEvFbReq) && 2ll * ((long long)c.S[top.node].qlen + 1) > V.hg[c.P[top.node].rt_off].cap) {
                    status |= kGrowTab; break;
                }
            }
            if constexpr (FL) {
                // a batch that leaves its processor and a gate that opens construct one Event per item in ONE handler: the heap has
                // room for all of them before anything changes, or the run stops in front of the Event (the items keep their Requests)
                const GEvent top = H.get(0);
                long long items = 0;
                if (top.kind == kEvBpCont) items = (long long)(top.pad >> kPadIdShift);
                else if (top.kind == kEvGtOpen) items = c.S[top.node].qlen;
                if (H.len + items + kPushes > c.heap_cap) { status |= kGrowHeap; break; }
            }
            if constexpr (AS) {
                const GEvent top = H.get(0);                                       // an evaluation may append one record to its scaling history
                if (top.kind == kEvAsEval && top.t >= cur) {
                    const GAs &row = V.as[c.P[top.node].stream_base];
                    if (row.hist_len >= row.hist_cap) { status |= kGrowHist; break; }
                }
            }
            if constexpr (DP) {
                const GEvent top = H.get(0);                                       // a health check constructs two Events and one Request per instance
                if (top.kind == kEvRdCheck && top.t >= cur) {                      // of the batch
                    const long long nb = V.rd[c.P[top.node].stream_base].cur_new_n;
                    if (H.len + 2 * nb + 1 > c.heap_cap) { status |= kGrowHeap; break; }
                    long long room = (long long)c.req_cap - (long long)req_len;
                    for (int r = req_free; r >= 0 && room < nb; r = c.reqs[r].next) room += 1;
                    if (room < nb) { status |= kGrowReq; break; }
                }
            }
            if (c.coop_min > 0 && sel < 0) {                                       // (a graph without such a LoadBalancer: one uniform test)
                const GEvent top = H.get(0);
                if (top.kind == HS_EV_LB && top.t >= cur) {
                    const GParam &tp = c.P[top.node];
                    // (a crashed LoadBalancer makes no selection: its Event is dropped below)
                    bool coop = tp.sub >= HS_LB_LEAST_CONNECTIONS && tp.rt_cnt >= c.coop_min;
                    if constexpr (HC) {
                        // ... over the healthy list; the live WeightedRoundRobin adds, takes the first maximum and subtracts the same way.
                        // Every test that could stop the loop in front of this Event has passed above and passes again unchanged
                        // behind the hand-over, so the selection the wavefront makes (and, for WeightedRoundRobin, applies) is consumed.
                        if (c.health) coop = (tp.sub >= HS_LB_LEAST_CONNECTIONS || tp.sub == HS_LB_WEIGHTED_ROUND_ROBIN) && c.S[top.node].qlen >= c.coop_min;
                    }
                    if constexpr (DP) {
                        // (a deployed LoadBalancer's list is in insertion order; the cooperative selection's tie rule needs ascending
                        //  slots, so that one selects on the lone lane -- every other LoadBalancer of the graph keeps the wavefront)
                        for (int r = 0; r < V.n_rd; ++r) coop = coop && V.rd[r].lb != top.node;
                        for (int r = 0; r < V.n_cn; ++r) coop = coop && V.cn[r].lb != top.node;
                    }
                    if (coop && !(F && tp.crashed)) { want = top.node; break; }
                }
            }
            if (H.len > peak) peak = H.len;
            const GEvent e = H.pop();
            if (c.part && H.len > 0) {
                // two PENDING events of one nanosecond, one numbered before the run and one by the run: which comes first depends on how
                // many events the WHOLE Simulation had created by then, not only this part -- undecided here.  (Every such pair meets as
                // (popped, next) at some pop: a timestamp group is popped back to back.)
                const GEvent nx = H.get(0);
                if (nx.t == e.t && ((nx.pad ^ e.pad) & 1u)) { status |= kUndecided; break; }
            }
            if constexpr (F) {
                if (e.kind >= kEvFaultOn && e.kind < kEvHcCycle) {                 // a daemon leaves the heap; a cancelled one is skipped
                    polls_pending -= 1;                                            // before anything else (core/simulation.py:475-477)
                    if (e.pad & kPadCancelled) { n_cancelled++; continue; }
                }
            }
            if constexpr (FL) {
                if (e.kind == kEvGtOpen || e.kind == kEvGtClose) polls_pending -= 1;   // a daemon leaves the heap
                // a `_BatchTimeout` whose batch has started since: Event.cancel() (batch_processor.py:135-138), skipped like a cancelled fault
                // (the one Event beyond the end of a PART run, GCtl::part = 2: a cancelled entry in front of it ends the launch -- whether the
                //  next entry of this part or one of another part comes next is decided across all of them, hs_graph_run_parts)
                if (e.kind == kEvBpTimeout && ((uint32_t)c.S[e.node].d << kPadIdShift) != (e.pad & ~3u)) {
                    n_flow_cancelled++;
                    if (c.part == 2) break;
                    continue;
                }
            }
            if constexpr (AS) {
                if (e.kind == kEvAsEval) polls_pending -= 1;                       // a daemon leaves the heap
            }
            if (e.t < cur) continue;                                              // time-travel drop, core/simulation.py:480-489
            cur = e.t;
            processed++;
            const int n = e.node;
            const int64_t t = e.t;
            if (e.kind >= kKinds) { status |= kBadKind; break; }
            s_by_kind[e.kind] += 1ull;
            const GParam p = c.P[n];
            GState &s = c.S[n];
            if constexpr (F) {
                if (p.crashed && ((kDrop >> e.kind) & 1u)) {
                    // Event.invoke returns [] (core/event.py:261-262): no handler, no completion hooks, nothing constructed.  A
                    // Source's or Probe's one pending tick ends there for good, a limiter keeps _poll_scheduled without a poll.
                    if (e.kind == kEvLimPoll) polls_pending -= 1;
                    if (e.req >= 0) { c.reqs[e.req].next = req_free; req_free = e.req; }
                    continue;
                }
                if (e.kind >= kEvFaultOn && (!HC || e.kind < kEvHcCycle)) {
                    if constexpr (LF) {
                        // a link fault's activate / deactivate (faults/network_faults.py:83-100,159-176): the entry that is in force
                        // from now on.  Every fault read the link's original when it was constructed, so a deactivation restores
                        // the original whichever activation came last.  (The callback is no Event at the link: a crashed link's
                        // faults fire all the same -- these two kinds are not among kDrop.)
                        const uint32_t fi = e.pad >> kPadIdShift;
                        if (fi) {
                            const int32_t now_on = e.kind == kEvFaultOn ? (int32_t)fi : 0;
                            if (((V.faults[fi - 1].flags >> kFaultWhatShift) & 3u) == kFaultLatency) s.qlen = now_on; else s.active = now_on;
                            continue;
                        }
                    }
                    // crash / restart, pause / resume (faults/node_faults.py:46-62,103-109): a flag, not a count.  The row may be the
                    // launch's LDS copy: the byte goes to its place in HBM as well, nothing else of a row is ever written.
                    const uint8_t v = e.kind == kEvFaultOn ? 1 : 0;
                    const_cast<GParam *>(c.P)[n].crashed = v;
                    if (nodes_in_lds) const_cast<GParam *>(c0.P)[n].crashed = v;
                    continue;
                }
            }
            if constexpr (HC) {
                if (e.kind == kEvHcCycle) {
                    // HealthChecker._run_check_cycle / _check_backend (health_check.py:253-349): per backend of `all_backends` that is not
                    // being checked the probe -- a Request of the backend in every respect -- and its timeout, then the next cycle
                    if (!p.sub) continue;                                           // `if not self._is_running: return []`
                    const GParam &lp = c.P[p.target];
                    for (int q = 0; q < lp.rt_cnt; ++q) {
                        GHc &h = c.hc[lp.rt_off + q];
                        if (h.is_checking) continue;
                        h.is_checking = 1; h.last_time = t; h.has_time = 1;
                        s.d += 1;                                                   // _next_check_id
                        const int64_t id = s.d;
                        h.pending = (int32_t)id;
                        s.a += 1;
                        int r = req_free;
                        if (r >= 0) req_free = c.reqs[r].next; else r = req_len++;  // (room: tested in front of the pop)
                        const unsigned long long idx_p = G++;
                        GRequest rq; rq.created = t; rq.idx = idx_p; rq.service_s = 0.0; rq.client = (id << 32) | (int64_t)q; rq.next = -1; rq.hook = n; rq.pre = 0;
                        c.reqs[r] = rq;
                        const int be = c.rt_targets[lp.rt_off + q];
                        H.push(mk(t, idx_p, arrival_kind<L>(c.P, be), be, r));
                        GEvent te = mk(t + ns_from_seconds(p.lat_min), G++, kEvHcTimeout, n, -2 - q);
                        te.pad = (uint32_t)id << kPadIdShift;
                        H.push(te);
                    }
                    H.push(mk(t + ns_from_seconds(p.mean), G++, kEvHcCycle, n, -1));  // self.now + Duration.from_seconds(interval)
                    continue;
                }
                if (e.kind > kEvHcCycle && (!R || e.kind < kEvAllKinds)) {
                    // _handle_response / _handle_timeout (health_check.py:351-444)
                    const int q = -2 - e.req;
                    const GParam &lp = c.P[p.target];
                    GHc &h = c.hc[lp.rt_off + q];
                    if (h.pending == 0 || ((uint32_t)h.pending << kPadIdShift) != (e.pad & ~3u)) continue;   // stale: a processed no-op
                    h.pending = 0;
                    h.is_checking = 0;
                    const bool healthy = c.hl_flag[lp.rt_off + q] != 0;
                    if (e.kind == kEvHcResp) {
                        h.last_passed = 1; h.succ += 1; h.fail = 0;
                        s.b += 1;
                        if (!healthy && h.succ >= (int64_t)p.conc) { lb_mark(c, p.target, q, true); s.qlen += 1; }
                    } else {
                        h.last_passed = 0; h.fail += 1; h.succ = 0;
                        s.c += 1;
                        if (healthy && h.fail >= p.lim) { lb_mark(c, p.target, q, false); s.active += 1; }
                    }
                    continue;
                }
            }
            if constexpr (AS) {
                if (e.kind == kEvAsEval) {
                    // AutoScaler._evaluate (auto_scaler.py:326-357).  `all_backends` is the LoadBalancer's member list (its initial
                    // backends, then the live managed instances in id order: hl_list, GState::qlen of them -- under a scaler every
                    // member is healthy).
                    if (!p.sub) continue;                                           // `if not self._is_running: return []`
                    s.a += 1;
                    GAs &row = V.as[p.stream_base];
                    const GParam &lp = c.P[p.target];
                    GState &ls = c.S[p.target];
                    int32_t *hl = c.hl_list + lp.rt_off;
                    const int current = ls.qlen;
                    const long long lo = p.conc, hi = p.lim;
                    long long desired = current;
                    if (row.policy == HS_AUTOSCALER_QUEUE_DEPTH) {
                        // QueueDepthScaling.evaluate (:149-168): an integer sum
                        long long total = 0;
                        for (int q = 0; q < current; ++q) total += c.S[c.rt_targets[lp.rt_off + hl[q]]].qlen;
                        if ((double)total >= row.thr_out) desired = current + 1;
                        else if ((double)total <= row.thr_in && current > lo) desired = current - 1;
                        desired = desired < hi ? desired : hi;
                        desired = desired > lo ? desired : lo;
                    } else if (current == 0) {
                        if (row.policy == HS_AUTOSCALER_TARGET_UTILIZATION) desired = lo;   // `if not backends: return min_instances` (:81-82)
                    } else {
                        // sum(utilizations) / len(utilizations) (:90,132): the interpreter's plain left-to-right sum in list order, every
                        // utilization active / limit (a true division of two ints)
                        double sum = 0.0;
                        for (int q = 0; q < current; ++q) {
                            const int be = c.rt_targets[lp.rt_off + hl[q]];
                            sum = __dadd_rn(sum, __ddiv_rn((double)c.S[be].active, (double)c.P[be].conc));
                        }
                        const double avg = __ddiv_rn(sum, (double)current);
                        bool decided = true;
                        if (row.policy == HS_AUTOSCALER_TARGET_UTILIZATION) {
                            // int(current_count * avg_util / target + 0.5) (:94): three roundings, none fused
                            desired = (long long)__dadd_rn(__ddiv_rn(__dmul_rn((double)current, avg), row.target), 0.5);
                        } else {
                            decided = false;                                        // StepScaling.evaluate (:134-139)
                            for (int k = 0; k < row.n_steps; ++k)
                                if (avg >= row.step_thr[k]) { desired = (long long)current + row.step_adj[k]; decided = true; break; }
                        }
                        if (decided) {
                            desired = desired < hi ? desired : hi;
                            desired = desired > lo ? desired : lo;
                        }
                    }
                    // _in_cooldown (:359-367): (now - _last_scale_time).to_seconds() against the action's cooldown
                    const double elapsed = row.last_action ? seconds_from_ns(t - row.last_time) : 0.0;
                    if (desired > current) {
                        // _try_scale_out (:369-414)
                        if (row.last_action && elapsed < p.lat_min) s.d += 1;
                        else {
                            long long to_add = desired - current;
                            if (hi - current < to_add) to_add = hi - current;
                            if (to_add > 0) {
                                if ((long long)row.next_id + to_add > (long long)p.rt_cnt) {    // the host's bound on the pool did not hold
                                    row.wanted = row.next_id + 1;
                                    status |= kPoolOut;
                                    break;
                                }
                                for (long long k = 0; k < to_add; ++k) {
                                    // `add_backend(new_server)` at weight 1 (set_weight: the slot's weight is 1 already), behind every
                                    // member: pool slots ascend with the ids
                                    row.next_id += 1;
                                    const int slot = p.rt_off + row.next_id - 1;
                                    V.as_mem[lp.rt_off + slot] = 1;
                                    hl[ls.qlen] = slot;
                                    ls.qlen += 1;
                                }
                                row.last_time = t; row.last_action = kAsOut;
                                s.b += 1;
                                row.added += to_add;
                                int64_t *h = row.hist + 4 * row.hist_len;
                                h[0] = t; h[1] = kAsOut + 4 * to_add; h[2] = current; h[3] = ls.qlen;
                                row.hist_len += 1;
                            }
                        }
                    } else if (desired < current) {
                        // _try_scale_in (:416-455): the newest managed instances leave; with none managed the action still counts
                        if (row.last_action && elapsed < p.loss) s.d += 1;
                        else {
                            long long to_remove = current - desired;
                            if (current - lo < to_remove) to_remove = current - lo;
                            if (to_remove > 0) {
                                for (long long k = 0; k < to_remove; ++k) {
                                    if (ls.qlen > 0 && hl[ls.qlen - 1] >= p.rt_off) {   // `if self._managed_servers:` -- the list's last member
                                        V.as_mem[lp.rt_off + hl[ls.qlen - 1]] = 0;
                                        ls.qlen -= 1;
                                    }
                                }
                                row.last_time = t; row.last_action = kAsIn;
                                s.c += 1;
                                row.removed += to_remove;
                                int64_t *h = row.hist + 4 * row.hist_len;
                                h[0] = t; h[1] = kAsIn + 4 * to_remove; h[2] = current; h[3] = ls.qlen;
                                row.hist_len += 1;
                            }
                        }
                    }
                    H.push(mk(t + ns_from_seconds(p.mean), G++, kEvAsEval, n, -1));   // self.now + Duration.from_seconds(evaluation_interval)
                    polls_pending += 1;
                    continue;
                }
            }
            if constexpr (ST) {
                if (e.kind >= kEvPcItem) {
                    // PooledCycleResource.handle_event (pooled_cycle.py:120-141) / InventoryBuffer.handle_event (inventory.py:118-121).
                    // No completion hook ever rides on an Event that reaches one of them (a wrapper's or Client's target is refused,
                    // a LoadBalancer's backends are Servers), so a handler ends with the Events it constructs.
                    // A NEW Event for `to` at `now` with the Request's context (created_at and a client key survive), no hook;
                    // without a receiver the Request ends here:
                    auto forward = [&](int to, int r) {
                        if (to >= 0) H.push(mk(t, G++, arrival_kind<L>(c.P, to), to, r));
                        else { c.reqs[r].next = req_free; req_free = r; }
                    };
                    switch (e.kind) {
                    case kEvPcItem:
                        if (s.active < p.conc) {                                    // _start_cycle up to its yield (:143-148) via
                            s.active += 1;                                          // Event._start_process: one continuation is built and
                            (void)G++;                                              // invoked at once, the pushed one is the second
                            H.push(mk(t + p.lim, G++, kEvPcCont, n, e.req));
                        } else if (p.rt_cnt > 0 && s.qlen >= p.rt_cnt) {            // the line is full (:125-133)
                            s.b += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                        } else {                                                    // _queue.append (:135)
                            c.reqs[e.req].next = -1;
                            if (s.qtail >= 0) c.reqs[s.qtail].next = e.req; else s.qhead = e.req;
                            s.qtail = e.req;
                            s.qlen += 1;
                        }
                        break;
                    case kEvPcCont:                                                 // behind the yield (:149-179): the unit returns, the
                        s.active -= 1;                                              // Request travels on, then the head of the line is sent
                        s.a += 1;                                                   // to the pool ITSELF as a new Event: it takes a fresh
                        forward(p.target, e.req);                                   // sort index and goes through the heap
                        if (s.qlen > 0 && s.active < p.conc) {
                            const int r = s.qhead;
                            s.qhead = c.reqs[r].next;
                            if (s.qhead < 0) s.qtail = -1;
                            s.qlen -= 1;
                            c.reqs[r].next = -1;
                            H.push(mk(t, G++, kEvPcItem, n, r));
                        }
                        break;
                    case kEvIbItem:                                                 // _handle_consume (inventory.py:123-181), amount = 1
                        if (s.a >= 1) {
                            s.a -= 1;
                            s.d += 1;
                            forward(p.target, e.req);
                        } else {
                            s.b += 1;
                            forward(p.conc, e.req);
                        }
                        if (s.a <= p.lim && !s.active) {                            // the reorder (:161-172), behind the forward:
                            s.active = 1;                                           // Instant.from_seconds(now.to_seconds() + lead_time)
                            s.c += 1;
                            H.push(mk(ns_from_seconds(__dadd_rn(seconds_from_ns(t), p.mean)), G++, kEvIbReplenish, n, -1));
                        }
                        break;
                    default:                                                        // _handle_replenish (:183-194)
                        s.a += (int64_t)p.stream_base;
                        s.svc_draws += p.stream_base;
                        s.active = 0;
                        break;
                    }
                    continue;
                }
            }
            if constexpr (HG) {
                if (e.kind >= kEvHgReq) {
                    // Hedge.handle_event (hedge.py:152-174) / Fallback.handle_event (fallback.py:152-177).  No completion hook ever rides
                    // on an Event that reaches one of them (a wrapper's or Client's target is refused, a LoadBalancer's backends are
                    // Servers), so a handler ends with the Events it constructs.
                    const GHg &row = V.hg[p.rt_off];
                    int64_t &extra = *reinterpret_cast<int64_t *>(&s.total_service);   // hedges_cancelled / fallback_successes
                    // a NEW Event for `to` at `now` with the entry's context and this wrapper's hook, its key on the Request
                    auto send_copy = [&](const GHgEnt &en, int to, int64_t key) {
                        int r = req_free;
                        if (r >= 0) req_free = c.reqs[r].next; else r = req_len++;  // (room: tested in front of the pop)
                        const unsigned long long idx_p = G++;
                        GRequest q; q.created = en.created; q.idx = idx_p; q.service_s = __longlong_as_double(key); q.client = en.client;
                        q.next = -1; q.hook = n; q.pre = 0;
                        c.reqs[r] = q;
                        H.push(mk(t, idx_p, arrival_kind<L>(c.P, to), to, r));
                    };
                    // _forward_primary (hedge.py:176-217) / _forward_to_primary (fallback.py:179-248) up to the trigger / timeout: a new
                    // id, the entry with the original's context, the Request itself travels on as the NEW Event's
                    auto take_request = [&]() {
                        s.a += 1;
                        s.svc_draws += 1;
                        const int64_t id = (int64_t)s.svc_draws;
                        GRequest &q = c.reqs[e.req];
                        GHgEnt en; en.id = id; en.start = t; en.created = q.created; en.client = q.client; en.st = 0;
                        hg_insert(row, en);                                        // (room: tested in front of the pop)
                        s.qlen += 1;
                        q.hook = n; q.service_s = __longlong_as_double(id);
                        H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, e.req));
                        return id;
                    };
                    const int64_t key = e.req >= 0 ? 0 : ev_id(e);
                    const int64_t id = key & kHgIdMask;
                    switch (e.kind) {
                    case kEvHgReq: {
                        const int64_t nid = take_request();                        // (max_hedges >= 1: the first trigger always)
                        H.push(mk_id(t + p.lim, G++, kEvHgSend, n, nid | (1ll << kHgIdBits)));
                    } break;
                    case kEvHgSend: {                                              // _send_hedge (hedge.py:261-315)
                        const long long at = hg_find(row, id);
                        if (at < 0) break;                                         // the entry has left: a processed no-op
                        GHgEnt &en = row.tab[at];
                        if (en.st & 1) { extra += 1; break; }                      // completed: hedges_cancelled
                        if (((en.st >> kHgSentShift) & 0xffffffll) >= (int64_t)p.conc) break;
                        en.st += 1ll << kHgSentShift;
                        s.d += 1;
                        send_copy(en, p.target, id | kHgFlag);                     // is_hedge = True
                        const int64_t number = (key >> kHgIdBits) & 0xffffll;
                        if (number < (int64_t)p.conc) H.push(mk_id(t + p.lim, G++, kEvHgSend, n, id | ((number + 1) << kHgIdBits)));
                    } break;
                    case kEvHgResp: {                                              // _handle_response (hedge.py:317-362)
                        const long long at = hg_find(row, id);
                        if (at < 0) break;
                        GHgEnt &en = row.tab[at];
                        en.st += 1ll << kHgRecvShift;
                        if (!(en.st & 1)) {
                            en.st |= 1;
                            if (key & kHgFlag) s.c += 1; else s.b += 1;            // hedge_wins / primary_wins
                        }
                        if ((int64_t)((uint64_t)en.st >> kHgRecvShift) >= 1 + ((en.st >> kHgSentShift) & 0xffffffll)) {
                            hg_remove(row, at);
                            s.qlen -= 1;
                        }
                    } break;
                    case kEvFbReq: {
                        const int64_t nid = take_request();
                        if (p.lim >= 0) H.push(mk_id(t + p.lim, G++, kEvFbTimeout, n, nid));
                    } break;
                    case kEvFbPrimResp: {                                          // _handle_primary_response (fallback.py:314-355), no predicate
                        const long long at = hg_find(row, id);
                        if (at < 0 || row.tab[at].st != 0) break;                  // unknown, or timed out already: a processed no-op
                        hg_remove(row, at);
                        s.qlen -= 1;
                        s.b += 1;
                    } break;
                    case kEvFbTimeout: {                                           // _handle_timeout (:357-380) + _forward_to_fallback (:250-312)
                        const long long at = hg_find(row, id);
                        if (at < 0 || row.tab[at].st != 0) break;
                        s.c += 1;
                        row.tab[at].st = 1;
                        s.d += 1;
                        send_copy(row.tab[at], p.conc, id | kHgFlag);              // the `_fb_fallback_response` hook
                    } break;
                    default: {                                                     // _handle_fallback_response (:382-410)
                        const long long at = hg_find(row, id);
                        if (at < 0 || row.tab[at].st != 1) break;
                        hg_remove(row, at);
                        s.qlen -= 1;
                        extra += 1;
                    } break;
                    }
                    continue;
                }
            }
            if constexpr (DP) {
                if (e.kind >= kEvCnStart) {
                    // CanaryDeployer.handle_event (canary_deployer.py:265-280) over the ordered member list, like the rolling deployer's.
                    GCn &row = V.cn[p.stream_base];
                    const GParam &lp = c.P[p.target];
                    GState &ls = c.S[p.target];
                    int32_t *hl = c.hl_list + lp.rt_off;
                    uint8_t *mem = V.as_mem + lp.rt_off;
                    const int canary = p.rt_off;
                    const bool weighted = lp.sub == HS_LB_WEIGHTED_ROUND_ROBIN || lp.sub == HS_LB_WEIGHTED_LEAST_CONNECTIONS;   // hasattr(strategy, "set_weight")
                    auto set_weight = [&](int slot, int32_t w) { c.lb_w[lp.rt_off + slot] = w; row.wr[slot] = 1; };
                    // _reset_weights (:487-494): every backend that is a member NOW (an entry whose word has fallen is about to leave)
                    auto reset_weights = [&]() {
                        if (!weighted) return;
                        for (int q = 0; q < ls.qlen; ++q) if (mem[hl[q]]) set_weight(hl[q], 1);
                    };
                    int compact_lb = -1;
                    auto compact = [&]() {
                        if (V.rd_coop_min > 0 && ls.qlen >= V.rd_coop_min) { compact_lb = p.target; return; }
                        ls.qlen = compact_members_lone(hl, mem, ls.qlen);
                        V.rd_compactions[0] += 1;
                    };
                    // the evaluators' figure of one backend (:102-109, :140-143; server.py:176-180)
                    auto metric = [&](int slot) -> double {
                        const int be = c.rt_targets[lp.rt_off + slot];
                        if (row.evaluator == HS_CANARY_LATENCY) {
                            const long long cnt = V.svc_cnt[be];
                            return cnt > 0 ? __ddiv_rn(V.svc_sum[be], (double)cnt) : 0.0;
                        }
                        const int64_t total = c.S[be].c + c.S[be].d;                // requests_completed + requests_rejected
                        return total > 0 ? __ddiv_rn((double)c.S[be].d, (double)total) : 0.0;   // (total_failures: no attribute of ServerStats)
                    };
                    const int64_t iv_ns = ns_from_seconds(p.mean);
                    switch (e.kind) {
                    case kEvCnStart:                                                // _start_deployment (:282-310)
                        row.n_base = ls.qlen;
                        for (int q = 0; q < ls.qlen; ++q) row.base[q] = hl[q];
                        row.has_canary = 1;
                        if (!mem[canary]) {                                         // add_backend (load_balancer.py:176-216)
                            mem[canary] = 1;
                            hl[ls.qlen] = canary;
                            ls.qlen += 1;
                            c.rt_taken[lp.rt_off + canary] = 0;
                            if (weighted) set_weight(canary, 1);
                        }
                        row.status = HS_CANARY_IN_PROGRESS; row.cur_stage = 0; row.total_stages = row.n_stages; row.cur_pct = 0.0;
                        row.started += 1;
                        H.push(mk(t, G++, kEvCnStage, n, -1));
                        break;
                    case kEvCnStage: {                                              // _start_stage (:312-347)
                        if (row.cur_stage >= row.n_stages) { H.push(mk(t, G++, kEvCnPromote, n, -1)); break; }
                        const double pct = row.pct[row.cur_stage];
                        row.cur_pct = pct;
                        row.stage_start = t; row.has_start = 1;
                        // _set_traffic_weight (:453-485): two products, a difference and a quotient, each rounded on its own
                        if (weighted && row.n_base > 0) {
                            long long cw = 1, bw = 1;
                            if (!(pct >= 1.0)) {
                                const double a = __dmul_rn(pct, 100.0);
                                const double b = __ddiv_rn(__dmul_rn(__dsub_rn(1.0, pct), 100.0), (double)row.n_base);
                                cw = a >= 2147483647.0 ? 2147483647ll : a <= 1.0 ? 1ll : (long long)a;      // max(1, int(...))
                                bw = b >= 2147483647.0 ? 2147483647ll : b <= 1.0 ? 1ll : (long long)b;
                            }
                            for (int q = 0; q < row.n_base; ++q) set_weight(row.base[q], (int32_t)bw);
                            set_weight(canary, (int32_t)cw);
                        }
                        H.push(mk(t + iv_ns, G++, kEvCnEval, n, -1));
                    } break;
                    case kEvCnEval: {                                               // _evaluate (:349-411)
                        if (row.status != HS_CANARY_IN_PROGRESS) break;
                        row.ev_performed += 1;
                        // ErrorRateEvaluator / LatencyEvaluator.is_healthy (:87-100, :123-138): the baseline's plain left-to-right sum
                        const double x = metric(canary);
                        bool healthy;
                        if (x > row.ev_max) healthy = false;
                        else if (row.n_base == 0) healthy = x <= row.ev_max;
                        else {
                            double sum = 0.0;
                            for (int q = 0; q < row.n_base; ++q) sum = __dadd_rn(sum, metric(row.base[q]));
                            const double avg = __ddiv_rn(sum, (double)row.n_base);
                            healthy = avg > 0.0 ? x <= __dmul_rn(avg, row.ev_mult) : x <= row.ev_max;
                        }
                        if (!healthy) { row.ev_failed += 1; H.push(mk(t, G++, kEvCnRollback, n, -1)); break; }
                        row.ev_passed += 1;
                        if (seconds_from_ns(t - row.stage_start) >= row.period[row.cur_stage]) {
                            row.stages_completed += 1;
                            row.cur_stage += 1;
                            H.push(mk(t, G++, row.cur_stage >= row.n_stages ? kEvCnPromote : kEvCnStage, n, -1));
                        } else H.push(mk(t + iv_ns, G++, kEvCnEval, n, -1));
                    } break;
                    case kEvCnPromote: {                                            // _promote (:413-430): the whole baseline leaves in one pass
                        row.status = HS_CANARY_PROMOTING;
                        int gone = 0;
                        for (int q = 0; q < row.n_base; ++q) if (mem[row.base[q]]) { mem[row.base[q]] = 0; gone += 1; }
                        reset_weights();
                        if (gone) compact();
                        H.push(mk(t, G++, kEvCnComplete, n, -1));
                    } break;
                    case kEvCnRollback:                                             // _do_rollback (:432-444)
                        row.status = HS_CANARY_ROLLED_BACK;
                        row.rolled_back += 1;
                        if (row.has_canary && mem[canary]) {
                            mem[canary] = 0;
                            reset_weights();
                            compact();
                        } else reset_weights();
                        break;
                    default:                                                        // _complete (:446-451)
                        row.status = HS_CANARY_COMPLETED;
                        row.completed += 1;
                        break;
                    }
                    if (compact_lb >= 0) { want = -2 - compact_lb; break; }
                    continue;
                }
            }
            if constexpr (DP) {
                if (e.kind >= kEvRdStart) {
                    // RollingDeployer.handle_event (rolling_deployer.py:158-175).  The LoadBalancer's `_backends` is its member list in
                    // INSERTION order (hl_list, GState::qlen of them; under a deployer every member is healthy): add_backend appends,
                    // remove_backend keeps the order of the rest.
                    GRd &row = V.rd[p.stream_base];
                    const GParam &lp = c.P[p.target];
                    GState &ls = c.S[p.target];
                    int32_t *hl = c.hl_list + lp.rt_off;
                    uint8_t *mem = V.as_mem + lp.rt_off;
                    // add_backend (load_balancer.py:176-216): a name already registered only has its weight updated; a new BackendInfo
                    // counts from 0 and the strategy's weight becomes 1
                    auto add = [&](int slot) {
                        if (mem[slot]) return;
                        mem[slot] = 1;
                        hl[ls.qlen] = slot;
                        ls.qlen += 1;
                        c.rt_taken[lp.rt_off + slot] = 0;
                        if (slot < p.rt_off) row.readd[slot] = 1;
                        c.lb_w[lp.rt_off + slot] = 1;
                    };
                    // remove_backend over a whole list (load_balancer.py:218-236): the membership words fall, then ONE pass compacts the
                    // member list, order kept
                    // From GVars::rd_coop_min members on the pass belongs to all 64 lanes (below, behind the hand-over): the handler
                    // ends first -- whatever it appends in the meantime stands behind every entry the pass drops.
                    int compact_lb = -1;
                    auto remove_all = [&](const int32_t *list, int cnt, bool may_defer) {
                        int gone = 0;
                        for (int k = 0; k < cnt; ++k) if (mem[list[k]]) { mem[list[k]] = 0; gone += 1; }
                        if (!gone) return;
                        if (may_defer && V.rd_coop_min > 0 && ls.qlen >= V.rd_coop_min) { compact_lb = p.target; return; }
                        ls.qlen = compact_members_lone(hl, mem, ls.qlen);
                        V.rd_compactions[0] += 1;
                    };
                    const int64_t iv_ns = ns_from_seconds(p.mean);                  // Duration.from_seconds(health_check_interval)
                    switch (e.kind) {
                    case kEvRdStart:                                                // _start_deployment (:177-203)
                        row.old_head = 0; row.old_n = ls.qlen;
                        for (int q = 0; q < ls.qlen; ++q) row.old_b[q] = hl[q];
                        row.new_n = 0;
                        row.fail_count = 0;
                        for (int q = 0; q < row.cap; ++q) row.pass[q] = -1;
                        row.status = HS_DEPLOYMENT_IN_PROGRESS; row.total = ls.qlen; row.replaced = 0; row.failed = 0; row.cur_batch = 0;
                        row.started += 1;
                        H.push(mk(t, G++, kEvRdBatch, n, -1));
                        break;
                    case kEvRdBatch: {                                              // _replace_batch (:205-257)
                        const int remaining = row.old_n - row.old_head;
                        if (remaining == 0) { H.push(mk(t, G++, kEvRdComplete, n, -1)); break; }
                        const int cnt = row.batch_size < remaining ? row.batch_size : remaining;
                        if ((long long)row.next_id + cnt > (long long)p.rt_cnt) {   // the host's bound on the pool did not hold:
                            row.wanted = p.rt_cnt + 1;                              // the first instance of the batch the pool lacks
                            status |= kPoolOut;
                            break;
                        }
                        row.cur_batch += 1;
                        for (int k = 0; k < cnt; ++k) row.cur_old[k] = row.old_b[row.old_head + k];
                        row.cur_old_n = cnt;
                        row.old_head += cnt;
                        row.cur_new_n = 0;
                        for (int k = 0; k < cnt; ++k) {
                            row.next_id += 1;
                            const int slot = p.rt_off + row.next_id - 1;
                            add(slot);
                            row.cur_new[row.cur_new_n++] = slot;
                            row.new_b[row.new_n++] = slot;
                            row.pass[slot] = 0;
                        }
                        H.push(mk(t + iv_ns, G++, kEvRdCheck, n, -1));
                    } break;
                    case kEvRdCheck:                                                // _run_health_check (:259-304): the only status guard
                        if (row.status != HS_DEPLOYMENT_IN_PROGRESS) break;
                        for (int k = 0; k < row.cur_new_n; ++k) {
                            // the probe -- a `health_check` Event at the new Server, a Request of it in every respect -- and its timeout
                            const int slot = row.cur_new[k];
                            row.hc_performed += 1;
                            int r = req_free;
                            if (r >= 0) req_free = c.reqs[r].next; else r = req_len++;  // (room: tested in front of the pop)
                            const unsigned long long idx_p = G++;
                            GRequest rq; rq.created = t; rq.idx = idx_p; rq.service_s = 0.0; rq.client = (int64_t)slot; rq.next = -1; rq.hook = n; rq.pre = 0;
                            c.reqs[r] = rq;
                            const int be = c.rt_targets[lp.rt_off + slot];
                            H.push(mk(t, idx_p, arrival_kind<L>(c.P, be), be, r));
                            H.push(mk(t + iv_ns, G++, kEvRdTimeout, n, -2 - slot));
                        }
                        break;
                    case kEvRdPass: {                                               // _handle_health_pass (:306-361)
                        const int slot = -2 - e.req;
                        if (row.pass[slot] < 0) break;                              // `server_name not in self._health_pass_count`
                        row.pass[slot] += 1;
                        row.hc_passed += 1;
                        bool all_healthy = true;                                    // all() over an empty batch is true
                        for (int k = 0; k < row.cur_new_n; ++k) {
                            const int pc = row.pass[row.cur_new[k]];
                            if ((pc < 0 ? 0 : pc) < p.conc) { all_healthy = false; break; }
                        }
                        if (all_healthy) {
                            remove_all(row.cur_old, row.cur_old_n, true);
                            row.replaced += row.cur_old_n;
                            row.inst_replaced += row.cur_old_n;
                            H.push(mk(t, G++, kEvRdBatch, n, -1));
                        } else H.push(mk(t + iv_ns, G++, kEvRdCheck, n, -1));
                    } break;
                    case kEvRdTimeout: {                                            // _handle_health_timeout (:363-396)
                        const int pc = row.pass[-2 - e.req];
                        if ((pc < 0 ? 0 : pc) >= p.conc) break;
                        row.fail_count += 1;
                        row.hc_failed += 1;
                        row.failed += 1;
                        if ((int64_t)row.fail_count > p.lim) H.push(mk(t, G++, kEvRdRollback, n, -1));
                    } break;
                    case kEvRdRollback: {                                           // _rollback (:398-413)
                        row.status = HS_DEPLOYMENT_ROLLED_BACK;
                        row.rolled_back += 1;
                        // (a backend that comes back is appended at once: the lone lane compacts first -- also where the batch's old
                        //  backends are instances, which could be among the new ones that leave here)
                        bool readds = false;
                        for (int k = 0; k < row.cur_old_n; ++k) readds |= !mem[row.cur_old[k]] || row.cur_old[k] >= p.rt_off;
                        remove_all(row.new_b, row.new_n, !readds);
                        for (int k = 0; k < row.cur_old_n; ++k) add(row.cur_old[k]);
                    } break;
                    default:                                                        // _complete (:415-424)
                        row.status = HS_DEPLOYMENT_COMPLETED;
                        row.completed += 1;
                        break;
                    }
                    if (status != kRunning) break;
                    if (compact_lb >= 0) { want = -2 - compact_lb; break; }         // (<= -2: the member list of that LoadBalancer, to all lanes)
                    continue;
                }
            }
            // Event.invoke (core/event.py:277-283) with a wrapper's hook on the Event: the handler returned, `_bh_response` / `_tw_response`
            // is constructed behind the handler's own Events.  `keep`: NetworkLink copied the still-full hook list onto the Event for its
            // egress before the hooks ran (link.py:181), so the egress' handler fires it once more.
            [[maybe_unused]] auto fire_hook = [&](int r, bool keep) {
                const int hook = c.reqs[r].hook;
                if (hook < 0) return;
                if (!keep) c.reqs[r].hook = -1;
                const uint8_t hk = c.P[hook].kind;
                if (hook_has_id<L>(hk))
                    H.push(mk_id(t, G++, hook_resp_kind<L>(hk, req_id(c.reqs[r])), hook, req_id(c.reqs[r])));
                else if (hk == HS_NODE_LB) H.push(mk(t, G++, HS_EV_LB_RESP, hook, -1));
            };
            if constexpr (FL) {
                if (e.kind >= kEvBpItem) {
                    // BatchProcessor / ConveyorBelt / GateController (components/industrial/).  GParam: conc = batch_size / capacity /
                    // queue_capacity, lim = process_time / transit_time in ns, stream_base = the timeout in ns (sub = 1: it has one).
                    // GState: see hs_graph_get_flow.  No completion hook ever reaches one of them (a LoadBalancer's backends are Servers,
                    // a wrapper's or Client's target is refused), so a handler ends with the Events it constructs.
                    // A NEW Event for the downstream at `now` with the item's context (created_at survives), no hook:
                    auto forward = [&](int r) { H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, r)); };
                    // BatchProcessor._process_batch up to its yield (batch_processor.py:131-141) via Event._start_process: the buffer
                    // becomes the batch, the pending timeout is cancelled; one continuation is built and invoked at once, the pushed
                    // one is the second.  The batch's list and length travel in the entry: any number of batches is in process.
                    auto start_batch = [&]() {
                        (void)G++;
                        GEvent ce = mk(t + p.lim, G++, kEvBpCont, n, s.qhead);
                        ce.pad = (uint32_t)s.qlen << kPadIdShift;
                        s.qhead = -1; s.qtail = -1; s.qlen = 0;
                        s.d = 0;
                        H.push(ce);
                    };
                    auto append = [&](int r) {
                        c.reqs[r].next = -1;
                        if (s.qtail >= 0) c.reqs[s.qtail].next = r; else s.qhead = r;
                        s.qtail = r;
                        s.qlen += 1;
                    };
                    switch (e.kind) {
                    case kEvBpItem:                                                 // BatchProcessor.handle_event (:104-122)
                        append(e.req);
                        if (s.qlen == 1 && p.sub) {                                 // the first item of an empty buffer: the timeout and nothing else
                            s.svc_draws += 1;
                            if ((s.svc_draws & 0x3fffffffull) == 0) s.svc_draws += 1;
                            s.d = (int64_t)(s.svc_draws & 0x3fffffffull);
                            GEvent te = mk(t + (int64_t)p.stream_base, G++, kEvBpTimeout, n, -1);
                            te.pad = (uint32_t)s.d << kPadIdShift;
                            H.push(te);
                        } else if (s.qlen >= p.conc) start_batch();
                        break;
                    case kEvBpTimeout:                                              // _handle_timeout (:124-129): on an empty buffer a no-op
                        s.d = 0;
                        if (s.qlen == 0) break;
                        s.c += 1;
                        start_batch();
                        break;
                    case kEvBpCont:                                                 // the generator resumes (:142-157): every item, in buffer order
                        s.a += 1;                                                   // (room in the heap: tested in front of the pop)
                        s.b += (int64_t)(e.pad >> kPadIdShift);
                        for (int r = e.req; r >= 0;) { const int nx = c.reqs[r].next; forward(r); r = nx; }
                        break;
                    case kEvCvItem:                                                 // ConveyorBelt.handle_event (conveyor.py:91-98)
                        if (p.conc > 0 && s.active >= p.conc) {
                            s.b += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                            break;
                        }
                        s.active += 1;
                        (void)G++;                                                  // the continuation built by _start_process
                        H.push(mk(t + p.lim, G++, kEvCvCont, n, e.req));
                        break;
                    case kEvCvCont:                                                 // _transport behind its yield (:100-113)
                        s.active -= 1;
                        s.a += 1;
                        forward(e.req);
                        break;
                    case kEvGtItem:                                                 // GateController.handle_event (gate_controller.py:121-152)
                        if (s.active) { s.a += 1; forward(e.req); break; }
                        if (p.conc > 0 && s.qlen >= p.conc) {
                            s.c += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                            break;
                        }
                        append(e.req);
                        s.b += 1;
                        break;
                    case kEvGtOpen:                                                 // _do_open (:154-179): the whole queue, in FIFO order
                        if (s.active) break;
                        s.active = 1;
                        s.d += 1;
                        for (int r = s.qhead; r >= 0;) { const int nx = c.reqs[r].next; s.a += 1; forward(r); r = nx; }
                        s.qhead = -1; s.qtail = -1; s.qlen = 0;                     // (room in the heap: tested in front of the pop)
                        break;
                    default:                                                        // kEvGtClose: _do_close (:181-186)
                        s.active = 0;
                        break;
                    }
                    continue;
                }
            }
            if constexpr (CL) {
                if (e.kind >= kEvClReq) {
                    int64_t *tab = c.rs_tab + p.rt_off;                            // _in_flight: (key, start_time ns) per place, unordered
                    if (e.kind == kEvClReq) {
                        // Client._send_request (client.py:233-317): _in_flight[(request_id, attempt)] is set (an equal key is overwritten),
                        // a NEW Event for the target with the hook -- its context holds the metadata alone: created_at is this
                        // attempt's send time, no client id survives -- then the timeout Event
                        int r = e.req;
                        int64_t key = 1ll << kKeyAttemptShift;                     // a Request that came along: no request_id, attempt 1
                        if (r < 0) {
                            key = ev_id(e);
                            r = req_free;
                            if (r >= 0) req_free = c.reqs[r].next; else r = req_len++;   // (room: tested in front of the pop)
                        } else if (c.reqs[r].client <= -2) {
                            // the Request passed a Client before: every handler on the way forwards the context, so this Client reads
                            // THAT Client's metadata (core/entity.py:100-105, client.py:235-237) -- its request_id and its attempt
                            key = -2 - c.reqs[r].client;
                        }
                        int i = 0;
                        while (i < s.qlen && tab[2 * i] != key) ++i;
                        tab[2 * i] = key; tab[2 * i + 1] = t;                      // (room for a new key: tested in front of the pop)
                        if (i == s.qlen) s.qlen += 1;
                        s.a += 1;
                        if ((key >> kKeyAttemptShift) > 1) s.d += 1;
                        GRequest q; q.created = t; q.idx = 0; q.service_s = __longlong_as_double(key); q.client = -2 - key; q.next = -1; q.hook = n; q.pre = 0;
                        c.reqs[r] = q;
                        H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, r));
                        if (p.sub) H.push(mk_id(t + ns_from_seconds(p.lat_min), G++, kEvClTimeout, n, key));
                        continue;
                    }
                    // _handle_response / _handle_timeout (:319-443): an unknown key is a processed no-op
                    const int64_t key = ev_id(e);
                    int i = 0;
                    while (i < s.qlen && tab[2 * i] != key) ++i;
                    if (i == s.qlen) continue;
                    const int64_t start = tab[2 * i + 1];
                    s.qlen -= 1;
                    tab[2 * i] = tab[2 * s.qlen]; tab[2 * i + 1] = tab[2 * s.qlen + 1];    // the last entry takes the place of the one that leaves
                    if (e.kind == kEvClResp) {
                        s.b += 1;
                        c.rec_node[rec_n] = n; c.rec_t[rec_n] = t - start; c.rec_cr[rec_n] = start;   // _response_times: (now - start_time)
                        rec_n++;
                    } else {
                        s.c += 1;
                        const int64_t attempt = key >> kKeyAttemptShift;
                        if (attempt - 1 < (int64_t)p.conc)                         // policy.should_retry(attempt): attempt < max_attempts
                            H.push(mk_id(t + c.cl_delays[p.lim + attempt - 1], G++, kEvClReq, n, key + (1ll << kKeyAttemptShift)));
                        else s.svc_draws += 1;                                     // failures
                    }
                    continue;
                }
            }
            if constexpr (R) {
                if (e.kind >= kEvBhReq) {
                    int64_t *tab = c.rs_tab + p.rt_off;
                    // Bulkhead._forward_request (bulkhead.py:231-291): a new id, the permit, a NEW Event for the target with the hook
                    auto bh_forward = [&](int r) {
                        s.svc_draws += 1;
                        const int64_t id = (int64_t)s.svc_draws;
                        s.active += 1; s.b += 1;
                        int32_t *peaks = reinterpret_cast<int32_t *>(&s.total_service);
                        if (s.active > peaks[0]) peaks[0] = s.active;
                        tab[s.active - 1] = id;                                    // (active <= max_concurrent = rt_cnt)
                        c.reqs[r].hook = n; c.reqs[r].service_s = __longlong_as_double(id);
                        H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, r));
                    };
                    switch (e.kind) {
                    case kEvBhReq: {                                               // Bulkhead.handle_event (bulkhead.py:191-229)
                        s.a += 1;
                        if (s.active < p.conc) bh_forward(e.req);
                        else if ((int64_t)s.qlen < p.lim) {                        // _enqueue_request (:293-335)
                            s.svc_draws += 1;
                            const int64_t id = (int64_t)s.svc_draws;
                            GRequest &q = c.reqs[e.req];
                            q.idx = (uint64_t)t; q.service_s = __longlong_as_double(id); q.next = -1;
                            if (s.qtail >= 0) c.reqs[s.qtail].next = e.req; else s.qhead = e.req;
                            s.qtail = e.req;
                            s.qlen += 1;
                            int32_t *peaks = reinterpret_cast<int32_t *>(&s.total_service);
                            if (s.qlen > peaks[1]) peaks[1] = s.qlen;
                            if (p.sub) H.push(mk_id(t + ns_from_seconds(p.lat_min), G++, kEvBhTimeout, n, id));
                        } else {
                            s.c += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                        }
                    } break;
                    case kEvBhResp: {                                              // _handle_response (:337-362) + _try_process_queued (:384-409)
                        if (!tab_remove(tab, s.active, ev_id(e))) break;           // an unknown id: a processed no-op
                        s.active = s.active > 0 ? s.active - 1 : 0;
                        while (s.qlen > 0 && s.active < p.conc) {
                            const int r = s.qhead;
                            s.qhead = c.reqs[r].next;
                            if (s.qhead < 0) s.qtail = -1;
                            s.qlen -= 1;
                            if (p.sub && seconds_from_ns(t - (int64_t)c.reqs[r].idx) > p.lat_min) {   // expired: skipped, the next one is tried
                                s.d += 1;
                                c.reqs[r].next = req_free; req_free = r;
                                continue;
                            }
                            bh_forward(r);
                            break;
                        }
                    } break;
                    case kEvBhTimeout: {                                           // _handle_timeout (:364-382): the entry of that id, if it still waits
                        const int64_t id = ev_id(e);
                        int prev = -1;
                        for (int r = s.qhead; r >= 0; prev = r, r = c.reqs[r].next) {
                            const int64_t rid = req_id(c.reqs[r]);
                            if (rid > id) break;                                   // (ids ascend along the queue)
                            if (rid != id) continue;
                            const int nx = c.reqs[r].next;
                            if (prev >= 0) c.reqs[prev].next = nx; else s.qhead = nx;
                            if (nx < 0) s.qtail = prev;
                            s.qlen -= 1;
                            s.d += 1;
                            c.reqs[r].next = req_free; req_free = r;
                            break;
                        }
                    } break;
                    case kEvTwReq: {                                               // TimeoutWrapper._forward_request (timeout.py:155-220)
                        s.a += 1;
                        s.svc_draws += 1;
                        const int64_t id = (int64_t)s.svc_draws;
                        tab[s.qlen] = id;                                          // (room: tested in front of the pop)
                        s.qlen += 1;
                        c.reqs[e.req].hook = n; c.reqs[e.req].service_s = __longlong_as_double(id);
                        H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, e.req));
                        H.push(mk_id(t + ns_from_seconds(p.lat_min), G++, kEvTwTimeout, n, id));
                    } break;
                    default: {                                                     // _handle_response / _handle_timeout (:222-295): whichever comes second finds nothing
                        if (!tab_remove(tab, s.qlen, ev_id(e))) break;
                        s.qlen -= 1;
                        if (e.kind == kEvTwResp) s.b += 1; else s.c += 1;
                    } break;
                    }
                    continue;
                }
            }
            if constexpr (Q) {
                if (p.pad[0] != HS_QUEUE_FIFO && (e.kind == HS_EV_ENQUEUE || e.kind == HS_EV_POLL)) {
                    // a Server whose Queue has a LIFOQueue, an AdaptiveLIFO or a CoDelQueue: Queue._handle_enqueue / _handle_poll
                    // (components/queue.py:122-166) with that policy's push / pop.  The list runs through Request::next as the FIFO's
                    // does and, backwards, through Request::hook.
                    GQueue &qs = V.qp[p.rt_cnt];
                    if (e.kind == HS_EV_ENQUEUE) {
                        const int hook = c.reqs[e.req].hook;                       // (as the FIFO handler below: one-shot)
                        c.reqs[e.req].hook = -1;
                        int64_t probe_tag = -1;
                        if (hook >= 0 && c.P[hook].kind == HS_NODE_HEALTH_CHECKER) { probe_tag = c.reqs[e.req].client; c.reqs[e.req].client = -1; }
                        [[maybe_unused]] int rd_slot = -1;
                        if constexpr (DP) {
                            if (hook >= 0 && c.P[hook].kind == HS_NODE_ROLLING_DEPLOYER) { rd_slot = (int)c.reqs[e.req].client; c.reqs[e.req].client = -1; }
                        }
                        const int64_t hook_id = req_id(c.reqs[e.req]);             // a wrapper's id / a Client's key: read before the stamp
                        if (p.lim >= 0 && s.qlen >= p.lim) {                       // push refuses at capacity
                            s.b += 1;
                            qs.cap_rejected += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                        } else {
                            GRequest &q = c.reqs[e.req];
                            q.idx = e.idx;
                            q.pre = e.pad & 1u;
                            q.next = -1;
                            q.hook = s.qtail;                                      // the predecessor (-1: none)
                            if (p.pad[0] == HS_QUEUE_CODEL) q.service_s = __longlong_as_double(t);   // _QueuedItem.enqueue_time
                            if (s.qtail >= 0) c.reqs[s.qtail].next = e.req; else s.qhead = e.req;
                            s.qtail = e.req;
                            s.a += 1;
                            qs.enqueued += 1;
                            const bool was_empty = s.qlen == 0;
                            s.qlen += 1;
                            if (was_empty) H.push(mk(t, G++, HS_EV_NOTIFY, n, -1));
                        }
                        if (DP && rd_slot >= 0) H.push(mk(t, G++, kEvRdPass, hook, -2 - rd_slot));
                        else if (probe_tag >= 0) {
                            GEvent re = mk(t, G++, kEvHcResp, hook, -2 - (int)(probe_tag & 0xffffffffll));
                            re.pad = (uint32_t)(probe_tag >> 32) << kPadIdShift;
                            H.push(re);
                        } else if (hook >= 0) {
                            const uint8_t hk = c.P[hook].kind;
                            if (hook_has_id<L>(hk)) H.push(mk_id(t, G++, hook_resp_kind<L>(hk, hook_id), hook, hook_id));
                            else H.push(mk(t, G++, HS_EV_LB_RESP, hook, -1));
                        }
                        continue;
                    }
                    if (s.qlen == 0) continue;                                      // pop() returns None: no Event
                    auto pop_oldest = [&]() {
                        const int r = s.qhead;
                        s.qlen -= 1;
                        if (s.qlen == 0) { s.qhead = -1; s.qtail = -1; } else s.qhead = c.reqs[r].next;
                        return r;
                    };
                    auto pop_newest = [&]() {
                        const int r = s.qtail;
                        s.qlen -= 1;
                        if (s.qlen == 0) { s.qhead = -1; s.qtail = -1; } else { s.qtail = c.reqs[r].hook; c.reqs[s.qtail].next = -1; }
                        return r;
                    };
                    int r;
                    if (p.pad[0] == HS_QUEUE_LIFO) r = pop_newest();
                    else if (p.pad[0] == HS_QUEUE_ADAPTIVE_LIFO) {                 // AdaptiveLIFO.pop (adaptive_lifo.py:135-162)
                        const int congested = (int64_t)s.qlen >= qs.threshold ? 1 : 0;   // before anything is removed
                        if (congested != qs.flag) { qs.switches += 1; qs.flag = congested; }
                        if (congested) { r = pop_newest(); qs.deq_b += 1; }
                        else { r = pop_oldest(); qs.deq_a += 1; }
                    } else {
                        // CoDelQueue.pop / _codel_dequeue (codel.py:177-256), operation for operation
                        r = pop_oldest();
                        const double sojourn = seconds_from_ns(t - __double_as_longlong(c.reqs[r].service_s));
                        bool ok_to_drop;                                            // _should_mark_or_drop: the head is gone already
                        if (sojourn < qs.target || s.qlen == 0) { qs.first_above = kQueueNone; ok_to_drop = false; }
                        else if (qs.first_above == kQueueNone) { qs.first_above = t + ns_from_seconds(qs.interval); ok_to_drop = false; }
                        else ok_to_drop = t >= qs.first_above;
                        auto drop = [&]() {                                         // _drop: the head goes, no handler sees it
                            if (s.qlen == 0) return;
                            const int d = pop_oldest();
                            c.reqs[d].next = req_free; req_free = d;
                            qs.dropped += 1;
                        };
                        auto control_law = [&]() { return t + codel_next_ns(qs.count, qs.interval); };
                        if (qs.flag) {
                            if (!ok_to_drop) qs.flag = 0;
                            else while (qs.drop_next != kQueueNone && t >= qs.drop_next && s.qlen > 0) {
                                drop();
                                qs.count += 1;
                                qs.drop_next = control_law();
                            }
                        } else if (ok_to_drop) {
                            drop();
                            qs.flag = 1;
                            qs.switches += 1;                                       // drop_intervals
                            const int64_t delta = qs.count - qs.last_count;
                            // (delta >= 1 only behind a drop of the loop above, which set _drop_next; the difference is signed)
                            qs.count = (delta < 1 || qs.drop_next == kQueueNone || seconds_from_ns(t - qs.drop_next) < qs.interval) ? 1 : delta;
                            qs.last_count = qs.count;
                            qs.drop_next = control_law();
                        }
                        qs.deq_a += 1;
                    }
                    c.reqs[r].hook = -1;                                            // every later handler reads it
                    H.push(mk(t, G++, HS_EV_DELIVER, n, r));
                    continue;
                }
            }
            switch (e.kind) {
            case HS_EV_SOURCE: {
                // Source.handle_event (load/source.py:142-180): the payload is constructed first, then the next SourceEvent;
                // `return [*payload_events, next_tick]`
                const bool payload = !(p.lim >= 0 && t > p.lim);                    // SimpleEventProvider.get_events :68
                int r = -1;
                unsigned long long idx_p = 0;
                if (payload) {
                    r = req_free;
                    if (r >= 0) req_free = c.reqs[r].next; else r = req_len++;
                    idx_p = G++;
                    GRequest q; q.created = t; q.idx = idx_p; q.service_s = 0.0; q.client = -1; q.next = -1; q.hook = -1; q.pre = 0;
                    if (p.conc > 0) {                                               // chash_example.py:83: one client id per Request
                        const double u = uniform_at(c.seed, stream_id(p.stream_base, kStreamKey), s.svc_draws);
                        s.svc_draws += 1;
                        q.client = (int64_t)__dmul_rn(u, (double)p.conc);
                    }
                    c.reqs[r] = q;
                    s.d += 1;
                }
                s.c += 1;                                                           // _generated_count (:159)
                const int64_t a2 = next_arrival(c, n);
                if (payload) H.push(mk(t, idx_p, arrival_kind<L>(c.P, p.target), p.target, r));
                if (a2 != kInfNs) H.push(mk(a2, G++, HS_EV_SOURCE, n, -1));       // RuntimeError: the source is exhausted (:176-180)
            } break;
            case HS_EV_ENQUEUE: {
                // QueuedResource.handle_event -> Queue._handle_enqueue (components/queue.py:122-147)
                const int hook = c.reqs[e.req].hook;                               // Event.on_complete of THIS Event: one-shot (core/event.py:290-311)
                c.reqs[e.req].hook = -1;
                int64_t probe_tag = -1;                                            // a health probe: (check id << 32) | backend slot rode in `client`
                if constexpr (HC) {
                    if (hook >= 0 && c.P[hook].kind == HS_NODE_HEALTH_CHECKER) { probe_tag = c.reqs[e.req].client; c.reqs[e.req].client = -1; }
                }
                [[maybe_unused]] int rd_slot = -1;                                 // a deployer's probe: the instance's slot rode in `client`
                if constexpr (DP) {
                    if (hook >= 0 && c.P[hook].kind == HS_NODE_ROLLING_DEPLOYER) { rd_slot = (int)c.reqs[e.req].client; c.reqs[e.req].client = -1; }
                }
                if (p.lim >= 0 && s.qlen >= p.lim) {                               // FIFOQueue.push refuses (queue_policy.py:94-98)
                    s.b += 1;
                    c.reqs[e.req].next = req_free; req_free = e.req;
                } else {
                    c.reqs[e.req].idx = e.idx;              // the queued payload IS this Event object
                    c.reqs[e.req].pre = e.pad & 1u;         // ... and its index keeps its origin (WORK re-uses it)
                    c.reqs[e.req].next = -1;
                    if (s.qtail >= 0) c.reqs[s.qtail].next = e.req; else s.qhead = e.req;
                    s.qtail = e.req;
                    s.a += 1;
                    const bool was_empty = s.qlen == 0;
                    s.qlen += 1;
                    if (was_empty) H.push(mk(t, G++, HS_EV_NOTIFY, n, -1));        // queue.py:144-146
                }
                // Event.invoke (core/event.py:277-283): the handler returned a plain list, so the completion hooks run now, behind
                // the handler's own events: the LoadBalancer's `_lb_response`
                if (DP && rd_slot >= 0) {
                    // ... or the deployer's `_rolling_health_pass` (rolling_deployer.py:283-291): a probe the queue refused passes as well
                    H.push(mk(t, G++, kEvRdPass, hook, -2 - rd_slot));
                } else if (HC && probe_tag >= 0) {
                    // ... or the checker's _health_check_response (health_check.py:321-334): a probe the queue refused passes as well
                    GEvent re = mk(t, G++, kEvHcResp, hook, -2 - (int)(probe_tag & 0xffffffffll));
                    re.pad = (uint32_t)(probe_tag >> 32) << kPadIdShift;
                    H.push(re);
                } else if (hook >= 0) {
                    if constexpr (R) {                                             // (a wrapper's hook: its id stayed on the Request)
                        const uint8_t hk = c.P[hook].kind;
                        if (hook_has_id<L>(hk)) {
                            H.push(mk_id(t, G++, hook_resp_kind<L>(hk, req_id(c.reqs[e.req])), hook, req_id(c.reqs[e.req])));
                            break;
                        }
                    }
                    H.push(mk(t, G++, HS_EV_LB_RESP, hook, -1));
                }
            } break;
            case HS_EV_NOTIFY:                                                      // QueueDriver._handle_notify (queue_driver.py:92-99)
                if (s.active < p.conc) H.push(mk(t, G++, HS_EV_POLL, n, -1));
                break;
            case HS_EV_POLL: {                                                      // Queue._handle_poll (queue.py:149-166)
                if (s.qlen == 0) break;
                const int r = s.qhead;
                s.qhead = c.reqs[r].next;
                if (s.qhead < 0) s.qtail = -1;
                s.qlen -= 1;
                H.push(mk(t, G++, HS_EV_DELIVER, n, r));
            } break;
            case HS_EV_DELIVER: {                                                   // queue_driver.py:66-90: same payload, ORIGINAL index
                const GRequest &q = c.reqs[e.req];                                  // (a schedule()d Request's: a pre-run index)
                H.push(q.pre ? mk_pre(t, q.idx, HS_EV_WORK, n, e.req) : mk(t, q.idx, HS_EV_WORK, n, e.req));
            } break;
            case HS_EV_WORK: {
                // Server.handle_queued_event up to its yield (server/server.py:202-250) via Event._start_process
                // (core/event.py:313-325): one continuation is built and invoked at once, the pushed one is the second
                (void)G++;
                if (!(s.active < p.conc)) {                                         // acquire() failed (server.py:223-234)
                    s.d += 1;
                    c.reqs[e.req].next = req_free; req_free = e.req;
                    break;
                }
                s.active += 1;
                double sv;
                if (p.sub == HS_LAT_EXPONENTIAL) {
                    const double u = uniform_at(c.seed, stream_id(p.stream_base, kStreamService), s.svc_draws);
                    s.svc_draws += 1;
                    const double sample = __ddiv_rn(exp1_from_uniform(u), __ddiv_rn(1.0, p.mean));   // expovariate(1 / mean)
                    sv = seconds_from_ns(ns_from_seconds(sample));
                } else sv = seconds_from_ns(ns_from_seconds(p.mean));
                c.reqs[e.req].service_s = sv;
                if constexpr (DP) {
                    // `_service_times.append(service_time_s)` (server.py:250): what LatencyEvaluator's average reads, in draw order
                    if (V.svc_sum) { V.svc_sum[n] = __dadd_rn(V.svc_sum[n], sv); V.svc_cnt[n] += 1; }
                }
                H.push(mk(t + ns_from_seconds(sv), G++, HS_EV_CONTINUATION, n, e.req));   // Instant + float seconds (temporal.py:222)
            } break;
            case HS_EV_CONTINUATION: {
                // the generator resumes (server/server.py:252-273): statistics, forward(event, downstream), then the
                // schedule_poll completion hook (queue_driver.py:79-84)
                s.active = s.active > 0 ? s.active - 1 : 0;
                s.c += 1; n_completed++;
                s.total_service = __dadd_rn(s.total_service, c.reqs[e.req].service_s);
                if (p.target >= 0) H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, e.req));
                else { c.reqs[e.req].next = req_free; req_free = e.req; }
                if (s.active < p.conc) H.push(mk(t, G++, HS_EV_POLL, n, -1));
            } break;
            case HS_EV_SINK: {                                                      // Sink.handle_event (components/common.py:36-44)
                c.rec_node[rec_n] = n; c.rec_t[rec_n] = t; c.rec_cr[rec_n] = c.reqs[e.req].created;
                rec_n++;
                s.a += 1; n_received++;
                if constexpr (R) fire_hook(e.req, false);
                c.reqs[e.req].next = req_free; req_free = e.req;
            } break;
            case HS_EV_ROUTE: {                                                     // RandomRouter.handle_event (random_router.py:32-45)
                const double u = uniform_at(c.seed, stream_id(p.stream_base, kStreamRoute), (uint64_t)s.a);
                s.a += 1;
                const int ri = (int)__dmul_rn(u, (double)p.rt_cnt);                 // targets[int(u * len(targets))]
                const int tg = c.rt_targets[p.rt_off + ri];
                c.rt_taken[p.rt_off + ri] += 1;
                if constexpr (R) {                                                  // (the router's new Event carries no hook: fired and cleared first,
                    const int hook = c.reqs[e.req].hook;                            //  its Event constructed behind the forward's)
                    const int64_t id = req_id(c.reqs[e.req]);
                    c.reqs[e.req].hook = -1;
                    H.push(mk(t, G++, arrival_kind<L>(c.P, tg), tg, e.req));
                    if (hook >= 0) H.push(mk_id(t, G++, hook_resp_kind<L>(c.P[hook].kind, id), hook, id));
                    break;
                }
                H.push(mk(t, G++, arrival_kind<L>(c.P, tg), tg, e.req));
            } break;
            case HS_EV_LINK: {
                // NetworkLink.handle_event up to its yield (components/network/link.py:114-154, _calculate_delay :190-216)
                (void)G++;                                                          // the continuation built by _start_process
                const int64_t entered = s.a;
                s.a = entered + 1;
                double loss = p.loss;
                uint64_t loss_k = (uint64_t)entered;                                // (the rate never changes: every Request draws, or none does)
                [[maybe_unused]] bool extra_on = false;
                [[maybe_unused]] double extra_s = 0.0;
                if constexpr (LF) {
                    if (lf_graph) {
                        // the rate and the latency in force (an InjectPacketLoss / InjectLatency between its two Events); the LOSS stream
                        // is read one value per draw, and a Request that meets a rate of 0 draws nothing (link.py:130)
                        if (s.active) loss = V.faults[s.active - 1].value;
                        if (s.qlen) { extra_on = true; extra_s = V.faults[s.qlen - 1].value; }
                        loss_k = s.svc_draws;
                        if (loss > 0.0) s.svc_draws = loss_k + 1;
                    }
                }
                if (loss > 0.0 && uniform_at(c.seed, stream_id(p.stream_base, kStreamLoss), loss_k) < loss) {   // link.py:131-138
                    s.c += 1;
                    if constexpr (R) fire_hook(e.req, false);                       // the generator ended before its first yield: the hooks run at once
                    c.reqs[e.req].next = req_free; req_free = e.req;
                    break;
                }
                double delay = seconds_from_ns(ns_from_seconds(p.lat_min));
                if constexpr (LF) {
                    // _CompoundLatency.get_latency (network_faults.py:41-44): Duration.from_seconds over the sum of the two Durations'
                    // seconds, taken back to seconds -- also for an extra of 0, which may move the base by a nanosecond
                    if (extra_on) delay = seconds_from_ns(ns_from_seconds(__dadd_rn(delay, extra_s)));
                }
                if (p.sub == HS_LAT_EXPONENTIAL) {
                    const double u = uniform_at(c.seed, stream_id(p.stream_base, kStreamLink), (uint64_t)s.d);
                    s.d += 1;
                    const double sample = __ddiv_rn(exp1_from_uniform(u), __ddiv_rn(1.0, p.mean));
                    delay = __dadd_rn(delay, seconds_from_ns(ns_from_seconds(sample)));
                } else if (p.mean > 0.0) delay = __dadd_rn(delay, seconds_from_ns(ns_from_seconds(p.mean)));   // ConstantLatency jitter: no draw
                if (!(delay > 0.0)) delay = 0.0;                                    // max(0.0, delay)
                H.push(mk(t + ns_from_seconds(delay), G++, HS_EV_LINK_CONT, n, e.req));
            } break;
            case HS_EV_LINK_CONT:                                                   // transit over (link.py:156-189): a NEW Event for the egress
                s.b += 1;
                if (p.target >= 0) {
                    H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, e.req));
                    if constexpr (R) fire_hook(e.req, true);                        // ... and stays on the Event for the egress (link.py:181)
                } else {
                    if constexpr (R) fire_hook(e.req, false);
                    c.reqs[e.req].next = req_free; req_free = e.req;
                }
                break;
            case HS_EV_LB: {
                // LoadBalancer._forward_request (load_balancer.py:347-433); without health state every backend is healthy
                s.a += 1;                                                           // :349
                int slot = 0;
                bool picked = false;
                if constexpr (HC) {
                    // `backends = self.healthy_backends`: the registration order, filtered (the three hashed / random strategies are
                    // refused over a changing list: with health state their backends all stay healthy, the tables below hold)
                    if (c.health && (p.sub == HS_LB_ROUND_ROBIN || p.sub == HS_LB_WEIGHTED_ROUND_ROBIN || p.sub >= HS_LB_LEAST_CONNECTIONS)) {
                        const int nh = s.qlen;
                        if (nh == 0) {                                              // :352-366
                            s.c += 1;
                            c.reqs[e.req].next = req_free; req_free = e.req;
                            break;
                        }
                        const int32_t *hl = c.hl_list + p.rt_off;
                        if (p.sub == HS_LB_ROUND_ROBIN) {
                            slot = hl[(int)(s.svc_draws % (uint64_t)nh)];          // healthy[_index % len(healthy)]
                            s.svc_draws += 1;
                        } else if (sel >= 0 && sel_node == n) {                    // (the wavefront took it, below)
                            slot = sel; n_coop++;
                            if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN) s.svc_draws += 1;
                        } else if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN) {
                            // the live smooth weighted round robin (strategies.py:111-134): every healthy backend's current weight grows
                            // by its weight, the first maximum in list order is taken and loses the healthy total
                            long long total = 0, best = 0;
                            for (int q = 0; q < nh; ++q) {
                                const int sl = hl[q];
                                const long long w = c.lb_w[p.rt_off + sl];
                                const long long cw = c.wrr_cur[p.rt_off + sl] + w;
                                c.wrr_cur[p.rt_off + sl] = cw;
                                c.hc[p.rt_off + sl].wrr_seen = 1;
                                total += w;
                                if (q == 0 || cw > best) { best = cw; slot = sl; }
                            }
                            c.wrr_cur[p.rt_off + slot] = best - total;
                            s.svc_draws += 1;
                        } else {
                            slot = hl[0];
                            double best = lb_score(c, p, slot);
                            for (int q = 1; q < nh; ++q) {
                                const double sc = lb_score(c, p, hl[q]);
                                if (sc < best) { best = sc; slot = hl[q]; }
                            }
                        }
                        sel = -1;
                        picked = true;
                    }
                }
                if (!picked && p.rt_cnt == 0) {                                     // no healthy backends, :352-366
                    s.c += 1;
                    c.reqs[e.req].next = req_free; req_free = e.req;
                    break;
                }
                const int64_t client = c.reqs[e.req].client;
                if (picked) {
                } else if (p.sub == HS_LB_CONSISTENT_HASH || p.sub == HS_LB_IP_HASH) {
                    if (client >= 0 && client < (int64_t)p.conc) slot = c.key_table[p.lim + client];   // .select(str(client_id)): a table
                    else {                                                          // no key: `self._fallback.select(...)`, a RoundRobin of
                        slot = (int)(s.svc_draws % (uint64_t)p.rt_cnt);             // the strategy's own (strategies.py:309,326-328,362,420-421)
                        s.svc_draws += 1;
                    }
                } else if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN) {                   // strategies.py:111-134: periodic in the total weight
                    slot = c.key_table[p.lim + (int64_t)(s.svc_draws % (uint64_t)p.conc)];
                    s.svc_draws += 1;
                } else if (p.sub >= HS_LB_LEAST_CONNECTIONS) {
                    // min(backends, key=...) (strategies.py:179-186,233-237): the FIRST backend with the smallest score
                    if (sel >= 0 && sel_node == n) { slot = sel; n_coop++; }        // (the wavefront took it, below)
                    else {
                        double best = lb_score(c, p, 0);
                        for (int q = 1; q < p.rt_cnt; ++q) {
                            const double sc = lb_score(c, p, q);
                            if (sc < best) { best = sc; slot = q; }
                        }
                    }
                    sel = -1;
                } else if (p.sub == HS_LB_ROUND_ROBIN) {
                    slot = (int)(s.svc_draws % (uint64_t)p.rt_cnt);                 // backends[_index % len], _index += 1 (strategies.py:66-67)
                    s.svc_draws += 1;
                } else if (client >= 0 && client < (int64_t)p.rt_cnt) slot = (int)client;            // Random: the plugged random.choice
                s.d += 1;                                                           // _in_flight, :378-382
                c.rt_taken[p.rt_off + slot] += 1;                                   // BackendInfo.total_requests, :385-386
                s.b += 1;                                                           // :388
                // a NEW Event for the backend with the same context (created_at survives) + the response hook (:398-431)
                const int be = c.rt_targets[p.rt_off + slot];
                c.reqs[e.req].hook = n;
                H.push(mk(t, G++, arrival_kind<L>(c.P, be), be, e.req));
            } break;
            case HS_EV_LB_RESP:                                                     // LoadBalancer._handle_response (load_balancer.py:435-473)
                if (s.d > 0) s.d -= 1;
                break;
            case HS_EV_PROBE_TICK: {
                // Source.handle_event with _ProbeEventProvider (instrumentation/probe.py:69-78): the daemon probe_event, then the next tick
                const unsigned long long idx_pe = G++;
                const int64_t k2 = s.a + 1;
                const int64_t a2 = c.ticks[(size_t)p.rt_off * (size_t)c.tick_cap + (size_t)k2];
                s.a = k2;
                H.push(mk(t, idx_pe, HS_EV_PROBE, n, -1));
                if (a2 != kInfNs) H.push(mk(a2, G++, HS_EV_PROBE_TICK, n, -1));
            } break;
            case HS_EV_PROBE: {                                                     // measure_callback (probe.py:51-66)
                const GState &tg = c.S[p.target];
                int64_t v = 0;
                switch (p.sub) {
                    case HS_PROBE_DEPTH: v = tg.qlen; break;
                    case HS_PROBE_ACTIVE: v = tg.active; break;
                    case HS_PROBE_ACCEPTED: v = tg.a; break;
                    case HS_PROBE_DROPPED: v = tg.b; break;
                    case HS_PROBE_COMPLETED: v = tg.c; break;
                    case HS_PROBE_RECEIVED: v = tg.a; break;                        // Sink.events_received
                    case HS_PROBE_GENERATED: v = tg.c; break;                       // Source.generated_count
                    case HS_PROBE_LIMITER_DEPTH: v = tg.qlen; break;                // RateLimitedEntity.queue_depth
                    default: break;
                }
                if constexpr (R) {                                                  // (the wrappers' metrics: this instantiation only)
                    switch (p.sub) {
                    case HS_PROBE_BH_ACTIVE: v = tg.active; break;                  // Bulkhead.active_count
                    case HS_PROBE_BH_QUEUE_DEPTH: v = tg.qlen; break;               // Bulkhead.queue_depth
                    case HS_PROBE_BH_PERMITS: {                                     // Bulkhead.available_permits: max(0, max_concurrent - active)
                        const int left = c.P[p.target].conc - tg.active;
                        v = left > 0 ? left : 0;
                    } break;
                    case HS_PROBE_TW_IN_FLIGHT: v = tg.qlen; break;                 // TimeoutWrapper.in_flight_count
                    case HS_PROBE_CL_IN_FLIGHT: if constexpr (CL) v = tg.qlen; break;   // Client.in_flight_count
                    default: break;
                    }
                }
                if constexpr (AS) {                                                 // AutoScaler.current_count: len(load_balancer.all_backends)
                    if (p.sub == HS_PROBE_AS_CURRENT_COUNT) v = c.S[c.P[p.target].target].qlen;
                }
                if constexpr (HG) {                                                 // Hedge.in_flight_count
                    if (p.sub == HS_PROBE_HG_IN_FLIGHT) v = tg.qlen;
                }
                if constexpr (ST) {                                                 // PooledCycleResource.available / active / queued,
                    if (p.sub == HS_PROBE_PC_AVAILABLE) v = (int64_t)c.P[p.target].conc - tg.active;     // InventoryBuffer.stock
                    else if (p.sub == HS_PROBE_PC_ACTIVE) v = tg.active;
                    else if (p.sub == HS_PROBE_PC_QUEUED) v = tg.qlen;
                    else if (p.sub == HS_PROBE_IB_STOCK) v = tg.a;
                }
                if constexpr (FL) {                                                 // (the flow entities' metrics likewise)
                    if (p.sub == HS_PROBE_BP_BUFFER_DEPTH || p.sub == HS_PROBE_GT_QUEUE_DEPTH) v = tg.qlen;   // buffer_depth / queue_depth
                    else if (p.sub == HS_PROBE_CV_IN_TRANSIT) v = tg.active;        // ConveyorBelt.items_in_transit
                }
                c.rec_node[rec_n] = n; c.rec_t[rec_n] = t; c.rec_cr[rec_n] = v;
                rec_n++;
                s.c += 1;
            } break;
            case kEvLimRequest: {
                // RateLimitedEntity._handle_request (rate_limited_entity.py:114-142): count, try_acquire, forward or queue or drop
                s.a += 1;
                int64_t outcome;
                [[maybe_unused]] int hook = -1;                                     // a wrapper's hook on THIS Event: the limiter's own Events carry none
                [[maybe_unused]] int64_t hook_id = 0;
                if constexpr (R) { hook = c.reqs[e.req].hook; hook_id = req_id(c.reqs[e.req]); c.reqs[e.req].hook = -1; }
                if (lim_try_acquire(c, p, s, t)) {
                    // _forward (:164-178): a NEW Event for the downstream at `now` with a copy of the context, no completion hook
                    outcome = HS_LIMITER_FORWARDED;
                    H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, e.req));
                } else if (!(p.lim >= 0 && s.qlen >= p.lim)) {                     // FIFOQueue.push (queue_policy.py:94-98)
                    outcome = HS_LIMITER_QUEUED;
                    c.reqs[e.req].next = -1;
                    if (s.qtail >= 0) c.reqs[s.qtail].next = e.req; else s.qhead = e.req;
                    s.qtail = e.req;
                    s.qlen += 1;
                    s.c += 1;
                    if (!(s.active & kLimPollScheduled)) {                          // _ensure_poll_scheduled (:180-193): ONE daemon Event
                        s.active |= kLimPollScheduled;
                        H.push(mk(t + lim_wait_ns(c, p, s, t), G++, kEvLimPoll, n, -1));
                        polls_pending += 1;
                    }
                } else {
                    outcome = HS_LIMITER_DROPPED;
                    s.b += 1;
                    c.reqs[e.req].next = req_free; req_free = e.req;
                }
                c.rec_node[rec_n] = n; c.rec_t[rec_n] = t; c.rec_cr[rec_n] = outcome;
                rec_n++;
                if constexpr (R) {
                    if (hook >= 0) H.push(mk_id(t, G++, hook_resp_kind<L>(c.P[hook].kind, hook_id), hook, hook_id));
                }
            } break;
            case kEvLimPoll: {
                // RateLimitedEntity._handle_poll (:144-162)
                s.d += 1;
                s.active &= ~kLimPollScheduled;
                polls_pending -= 1;
                if (s.qlen == 0) break;
                bool again = true;
                if (lim_try_acquire(c, p, s, t)) {
                    const int r = s.qhead;
                    s.qhead = c.reqs[r].next;
                    if (s.qhead < 0) s.qtail = -1;
                    s.qlen -= 1;
                    c.rec_node[rec_n] = n; c.rec_t[rec_n] = t; c.rec_cr[rec_n] = HS_LIMITER_DRAINED;
                    rec_n++;
                    H.push(mk(t, G++, arrival_kind<L>(c.P, p.target), p.target, r));
                    again = s.qlen > 0;
                }
                if (again) {
                    s.active |= kLimPollScheduled;
                    H.push(mk(t + lim_wait_ns(c, p, s, t), G++, kEvLimPoll, n, -1));
                    polls_pending += 1;
                }
            } break;
            default: status |= kBadKind; break;
            }
        }
        s_want = want;
      }
      __syncthreads();
      const int wn = s_want;
      if constexpr (DP) {
        if (wn <= -2) {
            // The member list of LoadBalancer -2 - wn, compacted by membership by all 64 lanes (the lone lane's state is visible behind
            // the barrier, as for a selection).
            const int lbn = -2 - wn;
            const GParam wp = c.P[lbn];
            const int w = compact_members_wave(c.hl_list + wp.rt_off, V.as_mem + wp.rt_off, c.S[lbn].qlen, lane);
            if (lane == 0) { c.S[lbn].qlen = w; V.rd_compactions[1] += 1; }
            __syncthreads();
            continue;
        }
        if (wn == -1) break;
      } else {
      if (wn < 0) break;
      }
      {
        // The selection of LoadBalancer `wn` by all 64 lanes: lane l scores slots l, l + 64, ... (ascending, so a lane keeps its first
        // minimum), then a butterfly over the lanes keeps the smaller (score, slot) pair -- the first minimum in add_backend order.  The
        // nodes' state is the lone lane's, visible behind the barrier (LDS, or HBM written by this very wavefront).
        const GParam wp = c.P[wn];
        bool taken = false;
        if constexpr (HC) {
            if (c.health) {
                // ... over the LoadBalancer's healthy list (ascending slots: a lane's first extremum is its smallest slot, and the smaller
                // slot wins a tie across lanes -- the first one in list order)
                const int nh = c.S[wn].qlen;
                const int32_t *hl = c.hl_list + wp.rt_off;
                int bslot = 0x7fffffff;
                if (wp.sub == HS_LB_WEIGHTED_ROUND_ROBIN) {
                    long long best = INT64_MIN, total = 0;
                    for (int q = lane; q < nh; q += 64) {
                        const int sl = hl[q];
                        const long long w = c.lb_w[wp.rt_off + sl];
                        const long long cw = c.wrr_cur[wp.rt_off + sl] + w;
                        c.wrr_cur[wp.rt_off + sl] = cw;
                        c.hc[wp.rt_off + sl].wrr_seen = 1;
                        total += w;
                        if (cw > best) { best = cw; bslot = sl; }
                    }
                    for (int m = 32; m >= 1; m >>= 1) {
                        const long long ob = __shfl_xor(best, m, 64), ot = __shfl_xor(total, m, 64);
                        const int os = __shfl_xor(bslot, m, 64);
                        total += ot;
                        if (ob > best || (ob == best && os < bslot)) { best = ob; bslot = os; }
                    }
                    __syncthreads();                                               // (every lane's store before the winner's)
                    if (lane == 0) c.wrr_cur[wp.rt_off + bslot] = best - total;
                } else {
                    double best = __longlong_as_double(0x7ff0000000000000ll);
                    for (int q = lane; q < nh; q += 64) {
                        const int sl = hl[q];
                        const double sc = lb_score(c, wp, sl);
                        if (sc < best) { best = sc; bslot = sl; }
                    }
                    for (int m = 32; m >= 1; m >>= 1) {
                        const double ob = __shfl_xor(best, m, 64);
                        const int os = __shfl_xor(bslot, m, 64);
                        if (ob < best || (ob == best && os < bslot)) { best = ob; bslot = os; }
                    }
                }
                sel = bslot; sel_node = wn;
                taken = true;
            }
        }
        if (!taken) {
        double best = __longlong_as_double(0x7ff0000000000000ll);
        int bslot = 0x7fffffff;
        for (int q = lane; q < wp.rt_cnt; q += 64) {
            const double sc = lb_score(c, wp, q);
            if (sc < best) { best = sc; bslot = q; }
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m, 64);
            const int os = __shfl_xor(bslot, m, 64);
            if (ob < best || (ob == best && os < bslot)) { best = ob; bslot = os; }
        }
        sel = bslot; sel_node = wn;
        }
      }
      __syncthreads();
    }
    if (lane == 0) {
        V.heap_len = H.len; V.counter = G; V.cur = cur; V.processed += processed; V.rec_n = rec_n;
        for (int k = 0; k < HS_EV_KINDS; ++k) V.by_kind[k] += (long long)s_by_kind[k];
        V.req_free = req_free; V.req_len = req_len;
        V.completed += n_completed; V.received += n_received;
        V.heap_peak = peak; V.polls_pending = polls_pending;
        if constexpr (F) {
            for (int k = 0; k < 4; ++k) V.internal_by_kind[k] += (long long)s_by_kind[HS_EV_KINDS + k];
            V.faults_cancelled += n_cancelled;
        }
        if constexpr (HC) {
            for (int k = 0; k < 3; ++k) V.health_by_kind[k] += (long long)s_by_kind[kEvHcCycle + k];
        }
        if constexpr (R) {
            for (int k = 0; k < 6; ++k) V.resil_by_kind[k] += (long long)s_by_kind[kEvBhReq + k];
        }
        if constexpr (CL) {
            for (int k = 0; k < 3; ++k) V.client_by_kind[k] += (long long)s_by_kind[kEvClReq + k];
        }
        if constexpr (FL) {
            for (int k = 0; k < HS_FLOW_KINDS; ++k) V.flow_by_kind[k] += (long long)s_by_kind[kEvBpItem + k];
            V.flow_cancelled += n_flow_cancelled;
        }
        if constexpr (AS) V.as_evals += (long long)s_by_kind[kEvAsEval];
        if constexpr (DP) {
            for (int k = 0; k < HS_DEPLOYER_KINDS; ++k) V.rd_by_kind[k] += (long long)s_by_kind[kEvRdStart + k];
            for (int k = 0; k < HS_CANARY_KINDS; ++k) V.cn_by_kind[k] += (long long)s_by_kind[kEvCnStart + k];
        }
        if constexpr (HG) {
            for (int k = 0; k < HS_HEDGE_KINDS; ++k) V.hg_by_kind[k] += (long long)s_by_kind[kEvHgReq + k];
        }
        if constexpr (ST) {
            for (int k = 0; k < HS_STOCK_KINDS; ++k) V.st_by_kind[k] += (long long)s_by_kind[kEvPcItem + k];
        }
        V.coop_selects = (c.coop_reset ? 0 : V.coop_selects) + n_coop;
        V.status = status;
    }
    __syncthreads();
    {   // ... and back
        const long long n8 = (V.heap_len < W ? V.heap_len : (long long)W) * (long long)(sizeof(GEvent) / 8);
        uint64_t *dst = reinterpret_cast<uint64_t *>(c.heap);
        const uint64_t *src = reinterpret_cast<const uint64_t *>(lheap);
        for (long long i = lane; i < n8; i += 64) dst[i] = src[i];
    }
    if (nodes_in_lds) {   // the nodes' state returns to its place
        const long long n8 = (long long)c.n * (long long)(sizeof(GState) / 8);
        const uint64_t *ss = reinterpret_cast<const uint64_t *>(lnodes + (size_t)NL * sizeof(GParam));
        uint64_t *ds = reinterpret_cast<uint64_t *>(c0.S);
        for (long long i = lane; i < n8; i += 64) ds[i] = ss[i];
    }
}

template <int L>
__global__ void __launch_bounds__(64) hs_graph_run_level(GCtl c) {
    __shared__ GEvent lheap[kLdsHeap];
    __shared__ __attribute__((aligned(16))) char lnodes[kLdsNodes * (sizeof(GParam) + sizeof(GState))];
    graph_loop<kLdsHeap, kLdsNodes, L>(c, lheap, lnodes);
}

// hs_debug_compact_members: one list, one wavefront
__global__ void __launch_bounds__(64) hs_graph_compact_members(int32_t *hl, const uint8_t *mem, int len, int wave, int32_t *out_len) {
    const int lane = threadIdx.x;
    int w = 0;
    if (wave) w = compact_members_wave(hl, mem, len, lane);
    else if (lane == 0) w = compact_members_lone(hl, mem, len);
    if (lane == 0) *out_len = w;
}

// Independent graphs -- the replicas / sweep points of parallel/runner.py:82-142 -- side by side: one workgroup (one heap) each, one
// with a quarter of the lone run's LDS window (32 KB + 6 KB of nodes: four workgroups per CU, 1 024 heaps on the device at once; a heap that outgrows
// the window continues in HBM as it does behind the large one -- the window's size changes nothing the loop computes).
__device__ __forceinline__ void batch_report(const GCtl &c, long long *stat) {
    __syncthreads();
    if (threadIdx.x == 0) {                    // what the host decides on, in ONE array for the whole batch
        long long *o = stat + kBatchStat * blockIdx.x;
        o[0] = c.V->status; o[1] = c.V->processed; o[2] = c.V->heap_len;
        o[3] = c.V->heap_len > 0 ? c.heap[0].t : 0;                // (the earliest pending event: hs_graph_run_parts elects across parts)
    }
}
// (the batch runs at the highest level any of its handles needs: a handle of a lower level computes the same either way)
template <int L>
__global__ void __launch_bounds__(64) hs_graph_run_batch_level(const GCtl *cs, long long *stat) {
    __shared__ GEvent lheap[kLdsHeapBatch];
    __shared__ __attribute__((aligned(16))) char lnodes[kLdsNodesBatch * (sizeof(GParam) + sizeof(GState))];
    const GCtl c = cs[blockIdx.x];
    graph_loop<kLdsHeapBatch, kLdsNodesBatch, L>(c, lheap, lnodes);
    batch_report(c, stat);
}

// One kernel of each form per level: these two tables are the only place that instantiates them.
using LoneKernel = void (*)(GCtl);
using BatchKernel = void (*)(const GCtl *, long long *);
template <int... Ls>
constexpr std::array<LoneKernel, sizeof...(Ls)> lone_kernels(std::integer_sequence<int, Ls...>) { return {{hs_graph_run_level<Ls>...}}; }
template <int... Ls>
constexpr std::array<BatchKernel, sizeof...(Ls)> batch_kernels(std::integer_sequence<int, Ls...>) { return {{hs_graph_run_batch_level<Ls>...}}; }
constexpr auto kLoneKernels = lone_kernels(std::make_integer_sequence<int, kLevels>{});
constexpr auto kBatchKernels = batch_kernels(std::make_integer_sequence<int, kLevels>{});

}  // namespace graph
}  // namespace hs

using namespace hs::graph;

struct hs_graph {
    hs_graph_config cfg{};
    int n = 0, n_rt = 0;
    double reach_s = 0.0;          // the longest single step of any node, in seconds: end + this must stay inside int64 (reach_fits_int64)
    GCtl ctl{};
    std::vector<GParam> params;
    std::vector<int32_t> sched_node; std::vector<int64_t> sched_t;
    int32_t *d_sched_node = nullptr; int64_t *d_sched_t = nullptr; long long d_sched_cap = 0;
    std::vector<GFault> faults; GFault *d_faults = nullptr;   // hs_graph_add_fault, in call order; on the device with the first run
    int32_t *d_rt_targets = nullptr;
    int32_t *d_key_table = nullptr;
    std::vector<int32_t> key_table;            // host image of d_key_table (hs_graph_set_lb_weights appends a WeightedRoundRobin's new table)
    std::vector<int32_t> lb_w;                 // [n_rt] host image of ctl.lb_w
    std::vector<hs_limiter_policy_params> lim_policy;   // per node (policy = HS_LIMITER_NONE until hs_graph_set_limiter_policy)
    int n_limiters = 0;
    long long lim_ring_len = 0;                // entries of ctl.lim_ring handed out so far
    std::vector<GState> state_cache; bool state_cache_valid = false;   // hs_graph_get_limiter: one copy of the nodes' state per run
    std::vector<int64_t> ring_cache;           // ... and of ctl.lim_ring
    bool has_least_loaded = false;             // a LeastConnections / WeightedLeastConnections LoadBalancer among the nodes
    // backend health: hs_graph_set_health_checker / hs_graph_set_lb_health make the graph one with health state (the third instantiation
    // of the loop); the device arrays come with the first run, in one allocation
    bool health = false, has_wrr = false;
    int n_checkers = 0;                        // HS_NODE_HEALTH_CHECKER nodes: every one is configured before a run
    std::vector<uint8_t> hl_flag;              // [n_rt] the initial BackendInfo.is_healthy of every backend slot
    std::vector<int32_t> checker_of;           // [n] the configured checker of a LoadBalancer node (-1: none)
    std::vector<uint8_t> checker_set;          // [n] hs_graph_set_health_checker has been called for the node
    char *d_health = nullptr;
    // Bulkhead / TimeoutWrapper: a graph that holds one runs the fourth instantiation of the loop; their in-flight tables (ctl.rs_tab)
    // come with the first run, laid out in node order
    int n_wrappers = 0;
    std::vector<uint8_t> wrapper_set;          // [n] hs_graph_set_wrapper has been called for the node
    std::vector<int32_t> tab_cap;              // [n] the table capacity the node starts with
    long long rs_tab_len = 0;
    // Client: a graph that holds one runs the fifth instantiation; its in-flight table is one of rs_tab (two words per place)
    int n_clients = 0;
    std::vector<GQueue> qpol;                  // hs_graph_set_queue_policy: the rows of the Servers with a queue policy, in call order; a graph
    GQueue *d_qp = nullptr;                    // that holds one runs the seventh instantiation (the rows go to the device with the first run)
    long long n_link_faults = 0;               // entries of `faults` from hs_graph_add_link_fault: a graph that holds one runs the eighth instantiation
    int n_flows = 0;                           // BatchProcessor / ConveyorBelt / GateController nodes: a graph that holds one runs the sixth instantiation
    std::vector<int64_t> cl_delays;            // every configured Client's delay table, back to back (GParam::lim = its offset)
    int64_t *d_cl_delays = nullptr;
    std::vector<int32_t> sched_id;             // request_id per scheduled entry (0: none)
    int32_t *d_sched_id = nullptr;
    bool any_sched_id = false;
    // AutoScaler: a graph that holds one runs the ninth instantiation; the rows, the membership words and the history buffers go to
    // the device with the first run
    int n_scalers = 0;
    std::vector<GAs> as_rows;                  // hs_graph_set_auto_scaler, in call order (GParam::stream_base = the row)
    std::vector<int32_t> as_node;              // the scaler node of every row
    std::vector<int32_t> scaler_of;            // [n] the configured scaler of a LoadBalancer node (-1: none)
    std::vector<uint8_t> as_member;            // [n_rt] the initial membership word of every backend slot (0: a dormant pool instance)
    GAs *d_as = nullptr; uint8_t *d_as_mem = nullptr;
    std::vector<int64_t *> d_as_hist;          // every row's history buffer
    // RollingDeployer: a graph that holds one runs the tenth instantiation; the rows and their lists go to the device with the first
    // run (the membership words are the scalers': as_member / d_as_mem)
    int n_deployers = 0;
    std::vector<GRd> rd_rows;                  // hs_graph_set_rolling_deployer, in call order (GParam::stream_base = the row)
    std::vector<int32_t> rd_node;              // the deployer node of every row
    std::vector<int32_t> deployer_of;          // [n] the configured deployer of a LoadBalancer node (-1: none)
    GRd *d_rd = nullptr;
    std::vector<int32_t *> d_rd_lists;         // every row's six lists, one allocation
    // CanaryDeployer: the same instantiation; its rows, the baseline lists and the Servers' service-time sums go to the device with the
    // first run
    int n_canaries = 0;
    std::vector<GCn> cn_rows;                  // hs_graph_set_canary_deployer, in call order (GParam::stream_base = the row)
    std::vector<int32_t> cn_node;
    GCn *d_cn = nullptr;
    std::vector<int32_t *> d_cn_lists;         // every row's two lists, one allocation
    double *d_svc_sum = nullptr; long long *d_svc_cnt = nullptr;
    // Hedge / Fallback: a graph that holds one runs the eleventh instantiation; the rows and every wrapper's table (an allocation of
    // its own, so that one table grows without the others) go to the device with the first run
    int n_hedges = 0;
    std::vector<GHg> hg_rows;                  // in node order (GParam::rt_off = the row)
    std::vector<int32_t> hg_node;              // the wrapper node of every row
    GHg *d_hg = nullptr;
    int n_stock = 0;                           // PooledCycleResource / InventoryBuffer nodes: a graph that holds one runs at kLvStock
    int debug_flags = 0;                       // hs_debug_graph_flags
    // tick tables: one row per time-varying Source and per distinct Probe interval, computed up to `tick_horizon`
    std::vector<hs::TickRow> rows;
    std::vector<double> row_rate;              // ticks per second a row may reach (sizes the table)
    hs::TickRow *d_rows = nullptr; int64_t *d_ticks = nullptr, *d_tick_count = nullptr; unsigned long long *d_tick_status = nullptr;
    int64_t tick_horizon = INT64_MIN, tick_cap = 0;
    hipStream_t stream = nullptr;              // created with the first launch that needs one (a replica run in a batch never does)
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    char *slab = nullptr; size_t slab_bytes = 0, slab_alloc = 0;   // every buffer of hs_graph_create in ONE allocation (a replica costs one hipMalloc / hipFree)
    double last_run_ms = 0.0;
    long long launches = 0;
    int last_level = -1;                       // the level of the most recent launch the handle ran in (hs_graph_level)
    bool ran = false;
    long long pending_events = 0; int64_t earliest_ns = 0;   // after a batch launch: the heap's length and its top's time
    bool undecided = false;                    // a part run met a timestamp group only the whole Simulation orders (hs_graph_run_parts)
    std::string error;
};

#include "hs_host.hpp"

// Slabs of destroyed handles wait here for the next handle of about their size: a Simulation spread over thousands of parts, or a sweep of
// thousands of replicas, creates and frees as many handles back to back, and hipFree synchronises the device every time (0.2 ms).
// Bounded: 4 096 slabs / 4 GB; the rest goes back to the runtime.
struct SlabPool {
    std::mutex mu;
    std::vector<std::pair<size_t, char *>> free;          // (bytes, pointer) of ONE device (the pool serves the device of its first slab)
    size_t bytes = 0; int device = -1;
    char *take(int dev, size_t want, size_t *have) {
        std::lock_guard<std::mutex> lk(mu);
        if (dev != device) return nullptr;
        for (size_t i = free.size(); i-- > 0;) {
            if (free[i].first >= want && free[i].first <= want + want / 2 + 4096) {
                char *p = free[i].second; *have = free[i].first; bytes -= free[i].first;
                free[i] = free.back(); free.pop_back();
                return p;
            }
            if (free.size() - i > 64) break;              // (the newest 64: a sweep's handles are all of one size)
        }
        return nullptr;
    }
    bool give(int dev, size_t have, char *p) {
        std::lock_guard<std::mutex> lk(mu);
        if (device < 0) device = dev;
        if (dev != device || free.size() >= 4096 || bytes + have > (4ull << 30)) return false;
        free.emplace_back(have, p); bytes += have;
        return true;
    }
};
static SlabPool g_slabs;

static bool in_slab(const hs_graph *g, const void *p) {
    return g->slab && (const char *)p >= g->slab && (const char *)p < g->slab + g->slab_bytes;
}

template <typename T>
static int grow(hs_graph *g, T **buf, long long old_n, long long new_n) {
    T *nb = nullptr;
    HS_HIP(g, hipMalloc(&nb, (size_t)new_n * sizeof(T)));
    if (*buf && old_n > 0) HS_HIP(g, hipMemcpy(nb, *buf, (size_t)old_n * sizeof(T), hipMemcpyDeviceToDevice));
    if (*buf && !in_slab(g, *buf)) HS_HIP(g, hipFree(*buf));
    *buf = nb;
    return HS_OK;
}

static int ensure_stream(hs_graph *g) {
    if (g->stream) return HS_OK;
    HS_HIP(g, hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    HS_HIP(g, hipEventCreate(&g->ev_a));
    HS_HIP(g, hipEventCreate(&g->ev_b));
    return HS_OK;
}

// The lowest level of graph_loop that dispatches every kind the graph holds.
static int level_of(const hs_graph *g) {
    if (g->n_stock > 0) return kLvStock;
    if (g->n_hedges > 0) return kLvHedge;
    if (g->n_deployers + g->n_canaries > 0) return kLvDeploy;
    if (g->n_scalers > 0) return kLvScaler;
    if (g->n_link_faults > 0) return kLvLinkFaults;
    if (!g->qpol.empty()) return kLvQueues;
    if (g->n_flows > 0) return kLvFlow;
    if (g->n_clients > 0) return kLvClient;
    if (g->n_wrappers > 0) return kLvResilience;
    if (g->health) return kLvHealth;
    if (!g->faults.empty()) return kLvFaults;
    return kLvPlain;
}
static void launch_lone(int level, hipStream_t stream, const GCtl &ctl) {
    hipLaunchKernelGGL(kLoneKernels[(size_t)level], dim3(1), dim3(64), 0, stream, ctl);
}
static void launch_batch(int level, unsigned blocks, hipStream_t stream, const GCtl *d_ctl, long long *d_stat) {
    hipLaunchKernelGGL(kBatchKernels[(size_t)level], dim3(blocks), dim3(64), 0, stream, d_ctl, d_stat);
}

extern "C" {

const char *hs_graph_last_error(const hs_graph *g) { return g ? g->error.c_str() : g_last_error.c_str(); }

void hs_graph_destroy(hs_graph *g) {
    if (!g) return;
    (void)hipSetDevice(g->cfg.device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    void *bufs[] = {g->ctl.heap, g->ctl.reqs, g->ctl.rec_node, g->ctl.rec_t, g->ctl.rec_cr, (void *)g->ctl.P, g->ctl.S,
                    g->d_rt_targets, g->d_key_table, g->ctl.lb_w, g->ctl.rt_taken, g->d_sched_node, g->d_sched_t, g->ctl.V, g->d_rows, g->d_ticks, g->d_tick_count,
                    g->d_tick_status, g->ctl.lim_ring, g->d_faults, g->d_health, g->d_as, g->d_as_mem, g->ctl.rs_tab, g->d_cl_delays, g->d_sched_id, g->d_qp};
    for (void *b : bufs) if (b && !in_slab(g, b)) (void)hipFree(b);
    for (int64_t *h : g->d_as_hist) if (h) (void)hipFree(h);
    for (int32_t *l : g->d_rd_lists) if (l) (void)hipFree(l);
    if (g->d_rd) (void)hipFree(g->d_rd);
    for (int32_t *l : g->d_cn_lists) if (l) (void)hipFree(l);
    if (g->d_cn) (void)hipFree(g->d_cn);
    if (g->d_svc_sum) (void)hipFree(g->d_svc_sum);
    if (g->d_svc_cnt) (void)hipFree(g->d_svc_cnt);
    if (g->d_hg) { for (GHg &r : g->hg_rows) if (r.tab) (void)hipFree(r.tab); (void)hipFree(g->d_hg); }
    if (g->slab && !g_slabs.give(g->cfg.device, g->slab_alloc, g->slab)) (void)hipFree(g->slab);
    if (g->ev_a) (void)hipEventDestroy(g->ev_a);
    if (g->ev_b) (void)hipEventDestroy(g->ev_b);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
}

// Why a Hedge's target / a Fallback's primary or fallback entity of this kind is refused (nullptr: it is lowered)
static const char *hook_refused(int kind) {
    switch (kind) {
    case HS_NODE_LB: case HS_NODE_BULKHEAD: case HS_NODE_TIMEOUT_WRAPPER: case HS_NODE_CLIENT: case HS_NODE_HEDGE: case HS_NODE_FALLBACK:
        return "a LoadBalancer, Bulkhead, TimeoutWrapper, Client, Hedge or Fallback: two completion hooks on one Event are not lowered";
    case HS_NODE_BATCH_PROCESSOR: case HS_NODE_CONVEYOR: case HS_NODE_GATE:
        return "a BatchProcessor, ConveyorBelt or GateController: a completion hook on an item they hold is not lowered";
    case HS_NODE_POOLED_CYCLE: case HS_NODE_INVENTORY:
        return "a PooledCycleResource or an InventoryBuffer: a completion hook on an item they hold or forward is not lowered";
    default: return nullptr;
    }
}

int hs_graph_create(const hs_graph_config *cfg, const hs_graph_nodes *nd, hs_graph **out) {
    if (!cfg || !nd || !out) return fail(nullptr, HS_E_INVALID, "hs_graph_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != sizeof(hs_graph_config)) return fail(nullptr, HS_E_INVALID, "hs_graph_config.struct_size mismatch (ABI)");
    const int n = nd->n_nodes;
    if (n < 1) return fail(nullptr, HS_E_INVALID, "n_nodes must be >= 1");
    if (!nd->kind || !nd->target) return fail(nullptr, HS_E_INVALID, "kind and target are required");
    if (nd->n_rt < 0 || (nd->n_rt > 0 && !nd->rt_targets)) return fail(nullptr, HS_E_INVALID, "rt_targets is required with n_rt > 0");
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count < 1)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device is visible (the engine has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= dev_count) return fail(nullptr, HS_E_INVALID, "device %d out of range", cfg->device);
    if (cfg->start_ns < 0)        // (the Sinks' merged records hold non-negative times)
        return fail(nullptr, HS_E_UNSUPPORTED, "start_time %lld ns is negative: not lowered", (long long)cfg->start_ns);
    bool has_wrr = false;
    auto takes_requests = [&](int t) { const int k = nd->kind[t]; return k == HS_NODE_SERVER || k == HS_NODE_SINK || k == HS_NODE_LINK || k == HS_NODE_ROUTER || k == HS_NODE_LB || k == HS_NODE_RATE_LIMITER || k == HS_NODE_BULKHEAD || k == HS_NODE_TIMEOUT_WRAPPER || k == HS_NODE_CLIENT || k == HS_NODE_BATCH_PROCESSOR || k == HS_NODE_CONVEYOR || k == HS_NODE_GATE || k == HS_NODE_HEDGE || k == HS_NODE_FALLBACK || k == HS_NODE_POOLED_CYCLE || k == HS_NODE_INVENTORY; };
    int64_t kmax = 0;                                  // client ids any Source hands out: [0, kmax)
    for (int i = 0; i < n; ++i)
        if (nd->kind[i] == HS_NODE_SOURCE && nd->src_n_clients && nd->src_n_clients[i] > kmax) kmax = nd->src_n_clients[i];
    if (kmax > (1ll << 26)) return fail(nullptr, HS_E_UNSUPPORTED, "n_clients above 2^26 is not supported (client -> backend table)");
    std::vector<int32_t> key_table;
    std::vector<GParam> P((size_t)n);
    std::vector<hs::TickRow> rows;
    std::vector<double> row_rate;
    double rate_sum = 0.0;
    int n_src = 0;
    bool has_ll = false;
    bool seen_other = false, seen_probe = false;      // node order: Sources, then Probes (the pre-run sort indices), then the rest
    for (int i = 0; i < n; ++i) {
        GParam p{};
        p.kind = nd->kind[i];
        p.target = nd->target[i];
        p.stream_base = nd->stream_base ? nd->stream_base[i] : (uint64_t)i;
        p.conc = 1; p.lim = -1; p.rt_off = 0; p.rt_cnt = 0; p.mean = 0.0; p.lat_min = 0.0; p.loss = 0.0;
        p.rt_off = -1;
        if (p.target < -1 || p.target >= n) return fail(nullptr, HS_E_INVALID, "node %d: target %d out of range", i, p.target);
        if (p.kind != HS_NODE_PROBE && p.target >= 0 && !takes_requests(p.target))
            return fail(nullptr, HS_E_INVALID, "node %d: its target %d takes no Requests (a Source or a Probe)", i, p.target);
        if (p.kind == HS_NODE_SOURCE && (seen_other || seen_probe))
            return fail(nullptr, HS_E_INVALID, "node %d: SOURCE nodes come first, in sources=[...] order", i);
        if (p.kind == HS_NODE_PROBE && seen_other)
            return fail(nullptr, HS_E_INVALID, "node %d: PROBE nodes come behind the SOURCE nodes, in probes=[...] order", i);
        if (p.kind == HS_NODE_PROBE) seen_probe = true;
        else if (p.kind != HS_NODE_SOURCE) seen_other = true;
        switch (p.kind) {
        case HS_NODE_SOURCE: {
            if (!nd->src_rate) return fail(nullptr, HS_E_INVALID, "src_rate is required");
            p.sub = nd->src_kind ? nd->src_kind[i] : (uint8_t)HS_SRC_POISSON;
            if (p.sub != HS_SRC_POISSON && p.sub != HS_SRC_CONSTANT) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: source kind %d is not lowered", i, (int)p.sub);
            p.mean = nd->src_rate[i];
            if (!(p.mean > 0.0) || !std::isfinite(p.mean)) return fail(nullptr, HS_E_INVALID, "node %d: source rate must be > 0, got %g", i, p.mean);
            p.lim = nd->src_stop_after_ns ? nd->src_stop_after_ns[i] : -1;
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a Source needs a target", i);
            {
                const int64_t nc = nd->src_n_clients ? nd->src_n_clients[i] : 0;
                if (nc < 0) return fail(nullptr, HS_E_INVALID, "node %d: src_n_clients < 0", i);
                p.conc = (int32_t)nc;
            }
            rate_sum += p.mean;
            ++n_src;
            const int pk = nd->src_profile_kind ? nd->src_profile_kind[i] : 0;
            if (pk != HS_PROF_CONSTANT) {
                if (pk != HS_PROF_LINEAR_RAMP && pk != HS_PROF_SPIKE) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: profile kind %d is not lowered", i, pk);
                if (!nd->src_profile_params) return fail(nullptr, HS_E_INVALID, "src_profile_params is required with src_profile_kind");
                const double *q = nd->src_profile_params + 4 * (size_t)i;
                for (int j = 0; j < 4; ++j) if (!std::isfinite(q[j]) || q[j] < 0.0) return fail(nullptr, HS_E_INVALID, "node %d: bad profile parameter %g", i, q[j]);
                hs::TickRow r{};
                r.kind = (uint32_t)pk; r.poisson = p.sub == HS_SRC_POISSON ? 1u : 0u;
                r.p0 = q[0]; r.p1 = q[1]; r.p2 = q[2]; r.p3 = q[3];
                r.seed = cfg->seed; r.sid = hs::stream_id(p.stream_base, hs::kStreamArrival); r.owner = i;
                p.rt_off = (int32_t)rows.size();
                rows.push_back(r);
                row_rate.push_back(p.mean);
            }
        } break;
        case HS_NODE_PROBE: {
            if (!nd->probe_metric || !nd->probe_interval_s) return fail(nullptr, HS_E_INVALID, "probe_metric and probe_interval_s are required for probes");
            p.sub = nd->probe_metric[i];
            const double iv = nd->probe_interval_s[i];
            if (!(iv > 0.0) || !std::isfinite(iv)) return fail(nullptr, HS_E_INVALID, "node %d: Probe interval must be positive", i);   // probe.py:29-30
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a Probe needs a target", i);
            const int tk = nd->kind[p.target];
            const bool ok = p.sub == HS_PROBE_GENERATED ? tk == HS_NODE_SOURCE : p.sub == HS_PROBE_RECEIVED ? tk == HS_NODE_SINK
                            : p.sub == HS_PROBE_LIMITER_DEPTH ? tk == HS_NODE_RATE_LIMITER
                            : (p.sub >= HS_PROBE_BH_ACTIVE && p.sub <= HS_PROBE_BH_PERMITS) ? tk == HS_NODE_BULKHEAD
                            : p.sub == HS_PROBE_TW_IN_FLIGHT ? tk == HS_NODE_TIMEOUT_WRAPPER
                            : p.sub == HS_PROBE_CL_IN_FLIGHT ? tk == HS_NODE_CLIENT
                            : p.sub == HS_PROBE_HG_IN_FLIGHT ? tk == HS_NODE_HEDGE
                            : (p.sub >= HS_PROBE_PC_AVAILABLE && p.sub <= HS_PROBE_PC_QUEUED) ? tk == HS_NODE_POOLED_CYCLE
                            : p.sub == HS_PROBE_IB_STOCK ? tk == HS_NODE_INVENTORY
                            : p.sub == HS_PROBE_BP_BUFFER_DEPTH ? tk == HS_NODE_BATCH_PROCESSOR
                            : p.sub == HS_PROBE_CV_IN_TRANSIT ? tk == HS_NODE_CONVEYOR
                            : p.sub == HS_PROBE_GT_QUEUE_DEPTH ? tk == HS_NODE_GATE
                            : p.sub == HS_PROBE_AS_CURRENT_COUNT ? tk == HS_NODE_AUTO_SCALER : (p.sub <= HS_PROBE_COMPLETED && tk == HS_NODE_SERVER);
            if (!ok) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: metric %d is not an attribute of its target (node kind %d)", i, (int)p.sub, tk);
            const double rate = 1.0 / iv;                           // _ProbeProfile.rate (probe.py:31)
            int found = -1;
            for (size_t q = 0; q < rows.size() && found < 0; ++q)
                if (rows[q].kind == hs::kProfGeneralConstant && rows[q].p0 == rate) found = (int)q;
            if (found < 0) {
                hs::TickRow r{};
                r.kind = hs::kProfGeneralConstant; r.poisson = 0; r.p0 = rate; r.owner = i;
                found = (int)rows.size();
                rows.push_back(r);
                row_rate.push_back(rate);
            }
            p.rt_off = found;
        } break;
        case HS_NODE_SERVER: {
            p.conc = nd->concurrency ? nd->concurrency[i] : 1;
            if (p.conc < 1) return fail(nullptr, HS_E_INVALID, "node %d: max_concurrent must be >= 1, got %d", i, p.conc);
            p.sub = nd->lat_kind ? nd->lat_kind[i] : (uint8_t)HS_LAT_CONSTANT;
            if (p.sub != HS_LAT_EXPONENTIAL && p.sub != HS_LAT_CONSTANT) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: service distribution kind %d is not lowered", i, (int)p.sub);
            p.mean = nd->lat_mean_s ? nd->lat_mean_s[i] : 0.0;
            if (!(p.mean >= 0.0) || !std::isfinite(p.mean)) return fail(nullptr, HS_E_INVALID, "node %d: bad service mean %g", i, p.mean);
            if (p.sub == HS_LAT_EXPONENTIAL && !(p.mean > 0.0)) return fail(nullptr, HS_E_INVALID, "node %d: exponential service needs mean > 0", i);
            p.lim = nd->queue_cap ? nd->queue_cap[i] : -1;
        } break;
        case HS_NODE_SINK: break;
        case HS_NODE_LINK: {
            p.sub = nd->lat_kind ? nd->lat_kind[i] : (uint8_t)HS_LAT_CONSTANT;
            if (p.sub != HS_LAT_EXPONENTIAL && p.sub != HS_LAT_CONSTANT) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: jitter kind %d is not lowered", i, (int)p.sub);
            p.mean = nd->lat_mean_s ? nd->lat_mean_s[i] : 0.0;
            if (p.sub == HS_LAT_EXPONENTIAL && !(p.mean > 0.0)) return fail(nullptr, HS_E_INVALID, "node %d: exponential jitter needs mean > 0", i);
            if (!(p.mean >= 0.0) || !std::isfinite(p.mean)) return fail(nullptr, HS_E_INVALID, "node %d: bad jitter mean %g", i, p.mean);
            p.lat_min = nd->link_lat_min_s ? nd->link_lat_min_s[i] : 0.0;
            if (!(p.lat_min >= 0.0) || !std::isfinite(p.lat_min)) return fail(nullptr, HS_E_INVALID, "node %d: bad link latency %g", i, p.lat_min);
            p.loss = nd->link_loss_rate ? nd->link_loss_rate[i] : 0.0;
            if (!(p.loss >= 0.0 && p.loss <= 1.0)) return fail(nullptr, HS_E_INVALID, "node %d: packet_loss_rate must be in [0, 1], got %g", i, p.loss);   // link.py:71-72
        } break;
        case HS_NODE_ROUTER: {
            if (!nd->rt_off || !nd->rt_cnt) return fail(nullptr, HS_E_INVALID, "rt_off and rt_cnt are required for routers");
            p.rt_off = nd->rt_off[i]; p.rt_cnt = nd->rt_cnt[i];
            if (p.rt_cnt < 1) return fail(nullptr, HS_E_INVALID, "node %d: a RandomRouter needs at least one target", i);
            if (p.rt_off < 0 || (long long)p.rt_off + p.rt_cnt > nd->n_rt) return fail(nullptr, HS_E_INVALID, "node %d: router targets out of range", i);
            for (int q = 0; q < p.rt_cnt; ++q) {
                const int t = nd->rt_targets[p.rt_off + q];
                if (t < 0 || t >= n || !takes_requests(t)) return fail(nullptr, HS_E_INVALID, "node %d: router target %d takes no Requests", i, t);
            }
        } break;
        case HS_NODE_LB: {
            if (!nd->rt_off || !nd->rt_cnt) return fail(nullptr, HS_E_INVALID, "rt_off and rt_cnt are required for LoadBalancers");
            p.rt_off = nd->rt_off[i]; p.rt_cnt = nd->rt_cnt[i];
            if (p.rt_cnt < 0 || p.rt_off < 0 || (long long)p.rt_off + p.rt_cnt > nd->n_rt) return fail(nullptr, HS_E_INVALID, "node %d: backends out of range", i);
            p.sub = nd->lb_strategy ? nd->lb_strategy[i] : (uint8_t)HS_LB_ROUND_ROBIN;                  // load_balancer.py:112: the default
            if (p.sub > HS_LB_WEIGHTED_LEAST_CONNECTIONS) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: load-balancing strategy %d is not lowered", i, (int)p.sub);
            for (int q = 0; q < p.rt_cnt; ++q) {
                const int t = nd->rt_targets[p.rt_off + q];
                if (t < 0 || t >= n || nd->kind[t] != HS_NODE_SERVER) return fail(nullptr, HS_E_UNSUPPORTED, "node %d: backend %d is not a Server (only Server backends are lowered)", i, t);
            }
            p.lim = -1; p.conc = 0;
            if (p.sub == HS_LB_CONSISTENT_HASH && p.rt_cnt > 0) {
                const int V = nd->lb_vnodes ? nd->lb_vnodes[i] : 100;
                if (V < 1) return fail(nullptr, HS_E_INVALID, "node %d: virtual_nodes must be >= 1, got %d", i, V);   // strategies.py:355-356
                if (!nd->names || !nd->name_off) return fail(nullptr, HS_E_INVALID, "names / name_off are required for a ConsistentHash LoadBalancer");
                std::string names;
                std::vector<int32_t> off(1, 0);
                for (int q = 0; q < p.rt_cnt; ++q) {
                    const int t = nd->rt_targets[p.rt_off + q];
                    const int nl = nd->name_off[t + 1] - nd->name_off[t];
                    if (nl < 1 || nl > 200) return fail(nullptr, HS_E_INVALID, "node %d: backend %d needs a name (1 .. 200 bytes)", i, t);
                    names.append(nd->names + nd->name_off[t], (size_t)nl);
                    off.push_back((int32_t)names.size());
                }
                const std::vector<hs::ring::RingPoint> ring = hs::ring::build_ring(names.data(), off.data(), p.rt_cnt, V);
                p.lim = (int64_t)key_table.size(); p.conc = (int32_t)kmax;
                char key[32];
                for (int64_t cid = 0; cid < kmax; ++cid) {                          // ConsistentHash.select for key str(id): a pure function of the id
                    const int len = snprintf(key, sizeof key, "%lld", (long long)cid);
                    key_table.push_back(hs::ring::ring_select(ring, key, (size_t)len));
                }
            }
            if (p.sub == HS_LB_IP_HASH && p.rt_cnt > 0) {                           // IPHash.select for key str(id) (strategies.py:330-333)
                p.lim = (int64_t)key_table.size(); p.conc = (int32_t)kmax;
                char key[32];
                for (int64_t cid = 0; cid < kmax; ++cid) {
                    const int len = snprintf(key, sizeof key, "%lld", (long long)cid);
                    key_table.push_back(hs::wrr::ip_hash_select(key, (size_t)len, p.rt_cnt));
                }
            }
            if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN && p.rt_cnt > 0) {              // every weight 1 (the default): RoundRobin's sequence
                p.lim = (int64_t)key_table.size(); p.conc = p.rt_cnt;
                for (int q = 0; q < p.rt_cnt; ++q) key_table.push_back(q);
            }
            if (p.sub >= HS_LB_LEAST_CONNECTIONS) has_ll = true;
            if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN) has_wrr = true;
        } break;
        case HS_NODE_HEALTH_CHECKER: {
            // HealthChecker (health_check.py:83-154); its LoadBalancer and parameters: hs_graph_set_health_checker
            if (p.target >= 0 && nd->kind[p.target] != HS_NODE_LB) return fail(nullptr, HS_E_INVALID, "node %d: a HealthChecker's target %d is not a LoadBalancer", i, p.target);
            p.sub = 0; p.conc = 2; p.lim = 3; p.mean = 10.0; p.lat_min = 5.0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_RATE_LIMITER: {
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a RateLimitedEntity needs a downstream", i);
            p.lim = nd->queue_cap ? nd->queue_cap[i] : 1000;                        // rate_limited_entity.py:60
            p.sub = (uint8_t)HS_LIMITER_NONE; p.conc = 0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_CLIENT:
        case HS_NODE_BULKHEAD:
        case HS_NODE_TIMEOUT_WRAPPER: {
            // Bulkhead / TimeoutWrapper (components/resilience/) and Client (components/client/): the parameters come with
            // hs_graph_set_wrapper / hs_graph_set_client
            const char *nm = p.kind == HS_NODE_BULKHEAD ? "Bulkhead" : p.kind == HS_NODE_CLIENT ? "Client" : "TimeoutWrapper";
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a %s needs a target", i, nm);
            // the target's handler must fire ONE hook: through any chain of links it is a Server, Sink, router or limiter
            int t = p.target;
            for (int hops = 0; hops <= n && t >= 0 && nd->kind[t] == HS_NODE_LINK; ++hops) t = nd->target[t];
            if (t >= 0 && (nd->kind[t] == HS_NODE_BATCH_PROCESSOR || nd->kind[t] == HS_NODE_CONVEYOR || nd->kind[t] == HS_NODE_GATE))
                return fail(nullptr, HS_E_UNSUPPORTED, "node %d: the target of a %s is (through %s) node %d, a BatchProcessor, ConveyorBelt or GateController: "
                            "a completion hook on an item they hold is not lowered", i, nm, t == p.target ? "no link" : "its links", t);
            if (t >= 0 && (nd->kind[t] == HS_NODE_LB || nd->kind[t] == HS_NODE_BULKHEAD || nd->kind[t] == HS_NODE_TIMEOUT_WRAPPER || nd->kind[t] == HS_NODE_CLIENT))
                return fail(nullptr, HS_E_UNSUPPORTED, "node %d: the target of a %s is (through %s) node %d, a LoadBalancer, Bulkhead, TimeoutWrapper or Client: "
                            "two completion hooks on one Event are not lowered", i, nm, t == p.target ? "no link" : "its links", t);
            if (t >= 0 && (nd->kind[t] == HS_NODE_HEDGE || nd->kind[t] == HS_NODE_FALLBACK))
                return fail(nullptr, HS_E_UNSUPPORTED, "node %d: the target of a %s is (through %s) node %d, a Hedge or a Fallback: "
                            "two completion hooks on one Event are not lowered", i, nm, t == p.target ? "no link" : "its links", t);
            if (t >= 0 && (nd->kind[t] == HS_NODE_POOLED_CYCLE || nd->kind[t] == HS_NODE_INVENTORY))
                return fail(nullptr, HS_E_UNSUPPORTED, "node %d: the target of a %s is (through %s) node %d, %s", i, nm,
                            t == p.target ? "no link" : "its links", t, hook_refused(nd->kind[t]));
            p.conc = 1; p.lim = 0; p.sub = 0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_HEDGE:
        case HS_NODE_FALLBACK: {
            // Hedge / Fallback (components/resilience/hedge.py, fallback.py): the parameters come with hs_graph_set_hedge /
            // hs_graph_set_fallback (which checks the fallback entity the same way)
            const char *nm = p.kind == HS_NODE_HEDGE ? "Hedge" : "Fallback";
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a %s needs a target", i, nm);
            int t = p.target;
            for (int hops = 0; hops <= n && t >= 0 && nd->kind[t] == HS_NODE_LINK; ++hops) t = nd->target[t];
            if (t >= 0 && hook_refused(nd->kind[t]))
                return fail(nullptr, HS_E_UNSUPPORTED, "node %d: the %s of a %s is (through %s) node %d, %s", i, p.kind == HS_NODE_HEDGE ? "target" : "primary",
                            nm, t == p.target ? "no link" : "its links", t, hook_refused(nd->kind[t]));
            p.conc = 1; p.lim = -1; p.sub = 0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_BATCH_PROCESSOR:
        case HS_NODE_CONVEYOR:
        case HS_NODE_GATE: {
            // BatchProcessor / ConveyorBelt / GateController (components/industrial/): the parameters come with hs_graph_set_flow
            if (p.target < 0) return fail(nullptr, HS_E_INVALID, "node %d: a BatchProcessor, ConveyorBelt or GateController needs a downstream", i);
            p.conc = 0; p.lim = 0; p.sub = 0; p.stream_base = 0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_POOLED_CYCLE:
        case HS_NODE_INVENTORY: {
            // PooledCycleResource / InventoryBuffer (components/industrial/pooled_cycle.py, inventory.py): a downstream is optional;
            // the parameters come with hs_graph_set_pool / hs_graph_set_inventory
            if (p.target >= 0 && !takes_requests(p.target)) return fail(nullptr, HS_E_INVALID, "node %d: its downstream %d takes no Requests", i, p.target);
            p.conc = p.kind == HS_NODE_POOLED_CYCLE ? 1 : -1; p.lim = 0; p.sub = 0; p.mean = 0.0; p.stream_base = 0; p.rt_off = 0; p.rt_cnt = 0;
        } break;
        case HS_NODE_AUTO_SCALER: {
            // AutoScaler (auto_scaler.py:207-263); its LoadBalancer, policy and parameters: hs_graph_set_auto_scaler
            if (p.target >= 0 && nd->kind[p.target] != HS_NODE_LB) return fail(nullptr, HS_E_INVALID, "node %d: an AutoScaler's target %d is not a LoadBalancer", i, p.target);
            p.sub = 0; p.conc = 1; p.lim = 10; p.mean = 10.0; p.lat_min = 30.0; p.loss = 60.0; p.rt_off = 0; p.rt_cnt = 0; p.stream_base = 0;
        } break;
        case HS_NODE_ROLLING_DEPLOYER: {
            // RollingDeployer (rolling_deployer.py:69-124); its LoadBalancer and parameters: hs_graph_set_rolling_deployer
            if (p.target >= 0 && nd->kind[p.target] != HS_NODE_LB) return fail(nullptr, HS_E_INVALID, "node %d: a RollingDeployer's target %d is not a LoadBalancer", i, p.target);
            p.sub = 0; p.conc = 2; p.lim = 1; p.mean = 2.0; p.lat_min = 0.0; p.loss = 0.0; p.rt_off = 0; p.rt_cnt = 0; p.stream_base = 0;
        } break;
        case HS_NODE_CANARY_DEPLOYER: {
            // CanaryDeployer (canary_deployer.py:180-225); its LoadBalancer, stages and evaluator: hs_graph_set_canary_deployer
            if (p.target >= 0 && nd->kind[p.target] != HS_NODE_LB) return fail(nullptr, HS_E_INVALID, "node %d: a CanaryDeployer's target %d is not a LoadBalancer", i, p.target);
            p.sub = 0; p.conc = 0; p.lim = 0; p.mean = 5.0; p.lat_min = 0.0; p.loss = 0.0; p.rt_off = 0; p.rt_cnt = 0; p.stream_base = 0;
        } break;
        default: return fail(nullptr, HS_E_UNSUPPORTED, "node %d: kind %d is not lowered", i, (int)p.kind);
        }
        P[(size_t)i] = p;
    }
    hs_graph *g = new hs_graph();
    g->cfg = *cfg; g->n = n; g->n_rt = nd->n_rt; g->params = P; g->rows = rows; g->row_rate = row_rate;
    g->key_table = key_table; g->has_least_loaded = has_ll; g->has_wrr = has_wrr;
    g->hl_flag.assign((size_t)(nd->n_rt > 0 ? nd->n_rt : 1), 1);
    g->checker_of.assign((size_t)n, -1); g->checker_set.assign((size_t)n, 0);
    g->scaler_of.assign((size_t)n, -1);
    g->deployer_of.assign((size_t)n, -1);
    for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_ROLLING_DEPLOYER) g->n_deployers++;
    for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_CANARY_DEPLOYER) g->n_canaries++;
    g->as_member.assign((size_t)(nd->n_rt > 0 ? nd->n_rt : 1), 1);
    for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_AUTO_SCALER) g->n_scalers++;
    g->lb_w.assign((size_t)(nd->n_rt > 0 ? nd->n_rt : 1), 1);
    {
        hs_limiter_policy_params none{};
        none.struct_size = sizeof none; none.policy = HS_LIMITER_NONE;
        g->lim_policy.assign((size_t)n, none);
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_RATE_LIMITER) g->n_limiters++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_HEALTH_CHECKER) g->n_checkers++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_BULKHEAD || P[(size_t)i].kind == HS_NODE_TIMEOUT_WRAPPER) g->n_wrappers++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_CLIENT) g->n_clients++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_HEDGE || P[(size_t)i].kind == HS_NODE_FALLBACK) g->n_hedges++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind == HS_NODE_POOLED_CYCLE || P[(size_t)i].kind == HS_NODE_INVENTORY) g->n_stock++;
        for (int i = 0; i < n; ++i) if (P[(size_t)i].kind >= HS_NODE_BATCH_PROCESSOR && P[(size_t)i].kind <= HS_NODE_GATE) g->n_flows++;
        g->wrapper_set.assign((size_t)n, 0); g->tab_cap.assign((size_t)n, 0);
    }
    for (int i = 0; i < n; ++i) {
        const GParam &p = P[(size_t)i];
        const double draw = p.sub == HS_LAT_EXPONENTIAL ? hs::kLongestExpDraw * p.mean : p.mean;       // (-log(2^-53) = 36.7 means at most)
        if (p.kind == HS_NODE_SOURCE) g->reach_s = std::max(g->reach_s, hs::kLongestExpDraw / p.mean);
        else if (p.kind == HS_NODE_SERVER) g->reach_s = std::max(g->reach_s, draw);
        else if (p.kind == HS_NODE_LINK) g->reach_s = std::max(g->reach_s, p.lat_min + draw);
        else if (p.kind == HS_NODE_PROBE) g->reach_s = std::max(g->reach_s, 1.0 / row_rate[(size_t)p.rt_off]);
    }
#define HSG_TRY(expr) do { int rc_ = (expr); if (rc_) { g_last_error = g->error; hs_graph_destroy(g); return rc_; } } while (0)
#define HSG_HIPD(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(g, HS_E_HIP, "%s: %s", #expr, hipGetErrorString(e_)); g_last_error = g->error; hs_graph_destroy(g); return HS_E_HIP; } } while (0)
    HSG_HIPD(hipSetDevice(cfg->device));
    GCtl &c = g->ctl;
    c.n = n; c.seed = cfg->seed; c.start_ns = cfg->start_ns; c.budget = kBudget;
    c.heap_cap = std::max<long long>(cfg->heap_capacity > 0 ? cfg->heap_capacity : 0, (long long)n * 4 + 1024);
    c.req_cap = (int)std::min<long long>(std::max<long long>(cfg->request_capacity > 0 ? cfg->request_capacity : 0, (long long)n * 4 + 1024), 1ll << 30);
    c.rec_cap = cfg->record_capacity > 0 ? cfg->record_capacity : 65536;
    (void)rate_sum;
    // one allocation: the initialised arrays first (one copy from a host image), behind them the ones the run fills (a buffer that
    // has to grow later moves into an allocation of its own, grow())
    const size_t nrt = (size_t)(nd->n_rt > 0 ? nd->n_rt : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_P = take((size_t)n * sizeof(GParam)), o_S = take((size_t)n * sizeof(GState)), o_rt = take(nrt * sizeof(int32_t)),
                 o_key = take(key_table.size() * sizeof(int32_t)), o_w = take(nrt * sizeof(int32_t)), o_taken = take(nrt * sizeof(long long)),
                 o_rows = take(rows.size() * sizeof(hs::TickRow)), o_V = take(sizeof(GVars));
    const size_t image_bytes = off;
    const size_t o_tcount = take(rows.size() * sizeof(int64_t)), o_tstatus = take(rows.empty() ? 0 : 2 * sizeof(unsigned long long)),
                 o_heap = take((size_t)c.heap_cap * sizeof(GEvent)), o_reqs = take((size_t)c.req_cap * sizeof(GRequest)),
                 o_rnode = take((size_t)c.rec_cap * sizeof(int32_t)), o_rt_ns = take((size_t)c.rec_cap * sizeof(int64_t)),
                 o_rcr = take((size_t)c.rec_cap * sizeof(int64_t));
    g->slab_bytes = off;
    g->slab = g_slabs.take(cfg->device, off, &g->slab_alloc);   // (a destroyed handle's slab of about this size, else a new one)
    if (!g->slab) { HSG_HIPD(hipMalloc((void **)&g->slab, g->slab_bytes)); g->slab_alloc = g->slab_bytes; }
    {
        std::vector<char> image(image_bytes, 0);
        std::memcpy(image.data() + o_P, P.data(), (size_t)n * sizeof(GParam));
        GState *S0 = reinterpret_cast<GState *>(image.data() + o_S);
        for (int i = 0; i < n; ++i) { S0[i].qhead = -1; S0[i].qtail = -1; }
        if (nd->n_rt > 0) std::memcpy(image.data() + o_rt, nd->rt_targets, (size_t)nd->n_rt * sizeof(int32_t));
        if (!key_table.empty()) std::memcpy(image.data() + o_key, key_table.data(), key_table.size() * sizeof(int32_t));
        std::memcpy(image.data() + o_w, g->lb_w.data(), nrt * sizeof(int32_t));
        if (!rows.empty()) std::memcpy(image.data() + o_rows, rows.data(), rows.size() * sizeof(hs::TickRow));
        GVars v{};
        v.req_free = -1; v.cur = cfg->start_ns;
        std::memcpy(image.data() + o_V, &v, sizeof v);
        HSG_HIPD(hipMemcpy(g->slab, image.data(), image_bytes, hipMemcpyHostToDevice));
    }
    c.P = reinterpret_cast<const GParam *>(g->slab + o_P);
    c.S = reinterpret_cast<GState *>(g->slab + o_S);
    g->d_rt_targets = reinterpret_cast<int32_t *>(g->slab + o_rt);
    c.rt_targets = g->d_rt_targets;
    g->d_key_table = key_table.empty() ? nullptr : reinterpret_cast<int32_t *>(g->slab + o_key);
    c.key_table = g->d_key_table;
    c.lb_w = reinterpret_cast<int32_t *>(g->slab + o_w);
    c.rt_taken = reinterpret_cast<long long *>(g->slab + o_taken);
    c.V = reinterpret_cast<GVars *>(g->slab + o_V);
    if (!rows.empty()) {
        g->d_rows = reinterpret_cast<hs::TickRow *>(g->slab + o_rows);
        g->d_tick_count = reinterpret_cast<int64_t *>(g->slab + o_tcount);
        g->d_tick_status = reinterpret_cast<unsigned long long *>(g->slab + o_tstatus);
    }
    c.heap = reinterpret_cast<GEvent *>(g->slab + o_heap);
    c.reqs = reinterpret_cast<GRequest *>(g->slab + o_reqs);
    c.rec_node = reinterpret_cast<int32_t *>(g->slab + o_rnode);
    c.rec_t = reinterpret_cast<int64_t *>(g->slab + o_rt_ns);
    c.rec_cr = reinterpret_cast<int64_t *>(g->slab + o_rcr);
    HSG_HIPD(hipDeviceSynchronize());
#undef HSG_TRY
#undef HSG_HIPD
    *out = g;
    return HS_OK;
}

int hs_graph_set_lb_weights(hs_graph *g, int32_t node, const int32_t *weights, int32_t n) {
    if (!g || !weights) return fail(g, HS_E_INVALID, "null argument");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_lb_weights: node %d is not a LoadBalancer", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_lb_weights: the weights are set before the first run");
    GParam &p = g->params[(size_t)node];
    if (n != p.rt_cnt) return fail(g, HS_E_INVALID, "set_lb_weights: node %d has %d backends, got %d weights", node, p.rt_cnt, n);
    for (int q = 0; q < n; ++q)
        if (weights[q] < 1) return fail(g, HS_E_INVALID, "weight must be >= 1, got %d", weights[q]);     // strategies.py:103-104,205-206
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (p.sub == HS_LB_WEIGHTED_ROUND_ROBIN && n > 0) {
        long long W = 0;
        for (int q = 0; q < n; ++q) W += weights[q];
        if (W > hs::wrr::kMaxTotalWeight)
            return fail(g, HS_E_UNSUPPORTED, "WeightedRoundRobin: a total weight of %lld needs a selection table beyond 2^24 entries", W);
        std::vector<int32_t> table;
        hs::wrr::build_table(weights, n, table);
        // the new table goes behind everything the other LoadBalancers keep; the device copy moves into an allocation of its own
        const size_t at = g->key_table.size();
        g->key_table.insert(g->key_table.end(), table.begin(), table.end());
        int32_t *nk = nullptr;
        HS_HIP(g, hipMalloc(&nk, g->key_table.size() * sizeof(int32_t)));
        hipError_t e = hipMemcpy(nk, g->key_table.data(), g->key_table.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(nk); return fail(g, HS_E_HIP, "copying the selection table: %s", hipGetErrorString(e)); }
        if (g->d_key_table && !in_slab(g, g->d_key_table)) (void)hipFree(g->d_key_table);
        g->d_key_table = nk; g->ctl.key_table = nk;
        p.lim = (int64_t)at; p.conc = (int32_t)W;
        HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    }
    if (n > 0) {
        std::copy(weights, weights + n, g->lb_w.begin() + p.rt_off);
        HS_HIP(g, hipMemcpy(g->ctl.lb_w + p.rt_off, weights, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return HS_OK;
}

int hs_graph_set_limiter_policy(hs_graph *g, int32_t node, const hs_limiter_policy_params *q) {
    if (!g || !q) return fail(g, HS_E_INVALID, "null argument");
    if (q->struct_size != sizeof(hs_limiter_policy_params)) return fail(g, HS_E_INVALID, "hs_limiter_policy_params.struct_size mismatch (ABI)");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_RATE_LIMITER)
        return fail(g, HS_E_INVALID, "set_limiter_policy: node %d is not a RateLimitedEntity", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_limiter_policy: the policy is set before the first run");
    if (g->lim_policy[(size_t)node].policy != HS_LIMITER_NONE) return fail(g, HS_E_STATE, "set_limiter_policy: node %d has its policy already", node);
    GParam p = g->params[(size_t)node];                    // (a copy: a refused policy leaves the node as it was)
    GState s0{};
    s0.qhead = -1; s0.qtail = -1;
    auto finite = [](double v) { return std::isfinite(v); };
    double reach = 0.0;
    switch (q->policy) {
    case HS_LIMITER_TOKEN_BUCKET:
        if (!finite(q->p0) || !finite(q->p1) || !finite(q->p2)) return fail(g, HS_E_INVALID, "TokenBucketPolicy: parameters must be finite");
        if (!(q->p1 > 0.0)) return fail(g, HS_E_INVALID, "TokenBucketPolicy: refill_rate must be > 0, got %g (the reference divides by it)", q->p1);
        p.lat_min = q->p0; p.mean = q->p1; s0.total_service = q->p2;
        reach = (1.0 + (q->p2 < 0.0 ? -q->p2 : 0.0)) / q->p1;
        break;
    case HS_LIMITER_LEAKY_BUCKET:
        if (!finite(q->p0) || !(q->p0 > 0.0)) return fail(g, HS_E_INVALID, "LeakyBucketPolicy: leak_rate must be > 0, got %g", q->p0);
        if (!finite(q->p1) || !(q->p1 > 0.0)) return fail(g, HS_E_INVALID, "LeakyBucketPolicy: bad leak interval %g", q->p1);
        p.mean = q->p0; p.lat_min = q->p1;
        reach = q->p1;
        break;
    case HS_LIMITER_SLIDING_WINDOW:
    case HS_LIMITER_FIXED_WINDOW: {
        const char *nm = q->policy == HS_LIMITER_SLIDING_WINDOW ? "SlidingWindowPolicy" : "FixedWindowPolicy";
        if (!finite(q->p0) || !(q->p0 >= 1e-9)) return fail(g, HS_E_INVALID, "%s: a window of %g s is below one nanosecond", nm, q->p0);
        if (q->count < 1) return fail(g, HS_E_INVALID, "%s: at least one request per window, got %lld", nm, (long long)q->count);
        if (q->policy == HS_LIMITER_SLIDING_WINDOW && q->count > kMaxSlidingLog)
            return fail(g, HS_E_UNSUPPORTED, "SlidingWindowPolicy: max_requests = %lld needs a log beyond 2^20 entries", (long long)q->count);
        if (q->count > INT32_MAX) return fail(g, HS_E_UNSUPPORTED, "%s: %lld requests per window is beyond 2^31", nm, (long long)q->count);
        p.mean = q->p0; p.conc = (int32_t)q->count;
        reach = q->p0;
        if (q->policy == HS_LIMITER_SLIDING_WINDOW) {
            if (g->lim_ring_len + q->count > (1ll << 30)) return fail(g, HS_E_UNSUPPORTED, "the SlidingWindowPolicy logs of this graph exceed 2^30 entries");
            p.rt_off = (int32_t)g->lim_ring_len; p.rt_cnt = (int32_t)q->count;                // (the ring itself: prepare_run, once)
        }
    } break;
    default: return fail(g, HS_E_UNSUPPORTED, "rate limiter policy %d is not lowered", (int)q->policy);
    }
    p.sub = (uint8_t)q->policy;
    g->reach_s = std::max(g->reach_s, reach);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    HS_HIP(g, hipMemcpy(g->ctl.S + node, &s0, sizeof s0, hipMemcpyHostToDevice));
    g->params[(size_t)node] = p;
    if (q->policy == HS_LIMITER_SLIDING_WINDOW) g->lim_ring_len += q->count;
    g->lim_policy[(size_t)node] = *q;
    return HS_OK;
}

int hs_debug_window_start(int32_t device, int64_t n, const int64_t *now_ns, const double *window_s, double *out_div, int64_t *out_start_ns) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (n <= 0 || !now_ns || !window_s || !out_div || !out_start_ns) return fail(nullptr, HS_E_INVALID, "hs_debug_window_start: bad arguments");
    if (device < 0 || device >= ndev) return fail(nullptr, HS_E_INVALID, "device ordinal %d out of range (%d devices)", device, ndev);
    for (int64_t i = 0; i < n; ++i)
        if (now_ns[i] < 0 || !(window_s[i] >= 2.2250738585072014e-308) || !std::isfinite(window_s[i]))
            return fail(nullptr, HS_E_INVALID, "hs_debug_window_start: entry %lld is outside now >= 0, window normal and > 0", (long long)i);
    HS_HIP(nullptr, hipSetDevice(device));
    void *d[4] = {nullptr, nullptr, nullptr, nullptr};
    const size_t bytes = (size_t)n * 8;
    for (int k = 0; k < 4; ++k) {
        const hipError_t e = hipMalloc(&d[k], bytes);
        if (e != hipSuccess) { for (auto &p : d) if (p) hipFree(p); return fail(nullptr, HS_E_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    }
    hipError_t e = hipMemcpy(d[0], now_ns, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[1], window_s, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_window_start_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, (const int64_t *)d[0],
                           (const double *)d[1], (double *)d[2], (int64_t *)d[3]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out_div, d[2], bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out_start_ns, d[3], bytes, hipMemcpyDeviceToHost);
    for (auto &p : d) hipFree(p);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_window_start: %s", hipGetErrorString(e));
    return HS_OK;
}

int hs_graph_get_limiter(hs_graph *g, int32_t node, hs_limiter_state *out, int64_t *log, int64_t log_cap) {
    if (!g || !out) return fail(g, HS_E_INVALID, "null argument");
    if (out->struct_size != sizeof(hs_limiter_state)) return fail(g, HS_E_INVALID, "hs_limiter_state.struct_size mismatch (ABI)");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_RATE_LIMITER)
        return fail(g, HS_E_INVALID, "get_limiter: node %d is not a RateLimitedEntity", node);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (!g->state_cache_valid) {
        g->state_cache.resize((size_t)g->n);
        HS_HIP(g, hipMemcpy(g->state_cache.data(), g->ctl.S, (size_t)g->n * sizeof(GState), hipMemcpyDeviceToHost));
        g->ring_cache.resize((size_t)g->lim_ring_len);    // ... and every sliding-window log with it: one copy per run, not one per limiter
        if (g->lim_ring_len > 0 && g->ctl.lim_ring)
            HS_HIP(g, hipMemcpy(g->ring_cache.data(), g->ctl.lim_ring, (size_t)g->lim_ring_len * sizeof(int64_t), hipMemcpyDeviceToHost));
        g->state_cache_valid = true;
    }
    const GState &s = g->state_cache[(size_t)node];
    const GParam &p = g->params[(size_t)node];
    int64_t bits;
    std::memcpy(&bits, &s.total_service, sizeof bits);
    const bool window = p.sub == HS_LIMITER_SLIDING_WINDOW || p.sub == HS_LIMITER_FIXED_WINDOW;
    out->policy = p.sub;
    out->received = s.a; out->dropped = s.b; out->queued = s.c; out->forwarded = s.a - s.b - s.qlen;
    out->queue_depth = s.qlen;
    out->poll_scheduled = (s.active & kLimPollScheduled) ? 1 : 0;
    out->requests_handled = s.a; out->polls_handled = s.d;
    out->has_time = p.sub != HS_LIMITER_SLIDING_WINDOW && (s.active & kLimHasTime) ? 1 : 0;
    out->time_ns = out->has_time ? (int64_t)s.svc_draws : 0;
    out->tokens = p.sub == HS_LIMITER_TOKEN_BUCKET ? s.total_service : 0.0;
    out->count = window ? bits : 0;
    if (p.sub == HS_LIMITER_SLIDING_WINDOW && log && log_cap > 0 && bits > 0) {
        const int64_t m = std::min<int64_t>(bits, log_cap), head = (int64_t)s.svc_draws, first = std::min<int64_t>(m, p.rt_cnt - head);
        const int64_t *ring = g->ring_cache.data() + p.rt_off;
        std::copy(ring + head, ring + head + first, log);
        if (m > first) std::copy(ring, ring + (m - first), log + first);
    }
    return HS_OK;
}

int hs_debug_graph_flags(hs_graph *g, int flags) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    g->debug_flags = flags;
    return HS_OK;
}

int64_t hs_graph_coop_selects(const hs_graph *g) {
    if (!g) return HS_E_INVALID;
    if (hipSetDevice(g->cfg.device) != hipSuccess) return HS_E_HIP;
    GVars v;
    if (hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return HS_E_HIP;
    return v.coop_selects;
}

int64_t hs_lb_wrr_table(const int32_t *weights, int32_t n, int32_t *out, int64_t cap) {
    if (!weights || n < 1) return fail(nullptr, HS_E_INVALID, "hs_lb_wrr_table: weights of at least one backend are required");
    long long W = 0;
    for (int q = 0; q < n; ++q) {
        if (weights[q] < 1) return fail(nullptr, HS_E_INVALID, "weight must be >= 1, got %d", weights[q]);
        W += weights[q];
    }
    if (W > hs::wrr::kMaxTotalWeight)
        return fail(nullptr, HS_E_UNSUPPORTED, "WeightedRoundRobin: a total weight of %lld needs a selection table beyond 2^24 entries", W);
    std::vector<int32_t> table;
    hs::wrr::build_table(weights, n, table);
    if (out) std::copy(table.begin(), table.begin() + std::min<long long>(W, cap > 0 ? cap : 0), out);
    return W;
}

int32_t hs_lb_ip_hash_select(const char *key, int32_t n_backends) {
    if (!key || n_backends < 1) return fail(nullptr, HS_E_INVALID, "hs_lb_ip_hash_select: a key and at least one backend are required");
    return hs::wrr::ip_hash_select(key, strlen(key), n_backends);
}

int hs_graph_set_health_checker(hs_graph *g, int32_t node, int32_t lb_node, double interval_s, double timeout_s, int32_t healthy_threshold,
                                int32_t unhealthy_threshold, int32_t running) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_HEALTH_CHECKER)
        return fail(g, HS_E_INVALID, "set_health_checker: node %d is not a HealthChecker", node);
    if (lb_node < 0 || lb_node >= g->n || g->params[(size_t)lb_node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_health_checker: node %d is not a LoadBalancer", lb_node);
    if (g->ran || g->launches > 0 || g->d_health) return fail(g, HS_E_STATE, "set_health_checker: a checker is configured before the first run");
    if (g->checker_set[(size_t)node]) return fail(g, HS_E_STATE, "set_health_checker: node %d is configured already", node);
    if (g->checker_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has HealthChecker node %d already: one checker per LoadBalancer is lowered", lb_node,
                    g->checker_of[(size_t)lb_node]);
    if (g->scaler_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has AutoScaler node %d: a HealthChecker and an AutoScaler on one LoadBalancer are not lowered", lb_node,
                    g->scaler_of[(size_t)lb_node]);
    if (g->deployer_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has RollingDeployer node %d: a HealthChecker and a deployer on one LoadBalancer are not lowered", lb_node,
                    g->deployer_of[(size_t)lb_node]);
    const uint8_t strat = g->params[(size_t)lb_node].sub;
    if (strat == HS_LB_CONSISTENT_HASH || strat == HS_LB_IP_HASH || strat == HS_LB_RANDOM)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: strategy %d is not lowered over a changing backend list (under a HealthChecker)", lb_node, (int)strat);
    // the reference's own checks (health_check.py:109-118)
    if (!std::isfinite(interval_s) || !(interval_s > 0.0)) return fail(g, HS_E_INVALID, "interval must be > 0, got %g", interval_s);
    if (!std::isfinite(timeout_s) || !(timeout_s > 0.0)) return fail(g, HS_E_INVALID, "timeout must be > 0, got %g", timeout_s);
    if (timeout_s >= interval_s) return fail(g, HS_E_INVALID, "timeout (%g) must be < interval (%g)", timeout_s, interval_s);
    if (healthy_threshold < 1) return fail(g, HS_E_INVALID, "healthy_threshold must be >= 1, got %d", healthy_threshold);
    if (unhealthy_threshold < 1) return fail(g, HS_E_INVALID, "unhealthy_threshold must be >= 1, got %d", unhealthy_threshold);
    if (!(interval_s * 1e9 >= 1.0)) return fail(g, HS_E_UNSUPPORTED, "an interval of %g s is below one nanosecond (the cycle would never advance)", interval_s);
    GParam &p = g->params[(size_t)node];
    p.target = lb_node; p.mean = interval_s; p.lat_min = timeout_s; p.conc = healthy_threshold; p.lim = unhealthy_threshold; p.sub = running ? 1 : 0;
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->checker_of[(size_t)lb_node] = node; g->checker_set[(size_t)node] = 1;
    g->reach_s = std::max(g->reach_s, interval_s);
    g->health = true;
    return HS_OK;
}

int hs_graph_set_lb_health(hs_graph *g, int32_t node, const uint8_t *healthy, int32_t n) {
    if (!g || !healthy) return fail(g, HS_E_INVALID, "null argument");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_lb_health: node %d is not a LoadBalancer", node);
    if (g->ran || g->launches > 0 || g->d_health) return fail(g, HS_E_STATE, "set_lb_health: the initial health flags are set before the first run");
    const GParam &p = g->params[(size_t)node];
    if (n != p.rt_cnt) return fail(g, HS_E_INVALID, "set_lb_health: node %d has %d backends, got %d flags", node, p.rt_cnt, n);
    bool all = true;
    for (int q = 0; q < n; ++q) all &= healthy[q] != 0;
    if (!all && (p.sub == HS_LB_CONSISTENT_HASH || p.sub == HS_LB_IP_HASH || p.sub == HS_LB_RANDOM))
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: strategy %d is not lowered with an unhealthy backend", node, (int)p.sub);
    for (int q = 0; q < n; ++q) g->hl_flag[(size_t)p.rt_off + (size_t)q] = healthy[q] ? 1 : 0;
    g->health = true;
    return HS_OK;
}

int hs_graph_get_health(hs_graph *g, int32_t node, int64_t *checker_stats, int64_t *backend_states, uint8_t *healthy, int64_t *marks, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node == -1 && !checker_stats && !backend_states && !healthy && !marks) {          // the graph's event counts alone
        if (events) {
            HS_HIP(g, hipSetDevice(g->cfg.device));
            GVars v;
            HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
            for (int k = 0; k < 3; ++k) events[k] = v.health_by_kind[k];
        }
        return HS_OK;
    }
    if (node < 0 || node >= g->n) return fail(g, HS_E_INVALID, "get_health: node %d out of range", node);
    const GParam &np = g->params[(size_t)node];
    if (np.kind != HS_NODE_LB && np.kind != HS_NODE_HEALTH_CHECKER) return fail(g, HS_E_INVALID, "get_health: node %d is neither a LoadBalancer nor a HealthChecker", node);
    if (np.kind == HS_NODE_HEALTH_CHECKER && !g->checker_set[(size_t)node]) return fail(g, HS_E_STATE, "get_health: HealthChecker node %d was never configured", node);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    const int lb = np.kind == HS_NODE_LB ? node : np.target;
    const GParam &lp = g->params[(size_t)lb];
    GState cs{}, ls{};
    HS_HIP(g, hipMemcpy(&ls, g->ctl.S + lb, sizeof ls, hipMemcpyDeviceToHost));
    if (np.kind == HS_NODE_HEALTH_CHECKER) HS_HIP(g, hipMemcpy(&cs, g->ctl.S + node, sizeof cs, hipMemcpyDeviceToHost));
    if (checker_stats) {                       // HealthCheckStats (health_check.py:44-53) in field order
        checker_stats[0] = cs.a; checker_stats[1] = cs.b; checker_stats[2] = cs.c; checker_stats[3] = cs.c;
        checker_stats[4] = cs.qlen; checker_stats[5] = cs.active;
    }
    if (backend_states && lp.rt_cnt > 0) {
        std::vector<GHc> h((size_t)lp.rt_cnt);
        for (auto &x : h) { x = GHc{}; x.last_passed = -1; }
        if (g->ctl.hc) HS_HIP(g, hipMemcpy(h.data(), g->ctl.hc + lp.rt_off, h.size() * sizeof(GHc), hipMemcpyDeviceToHost));
        for (int q = 0; q < lp.rt_cnt; ++q) {
            int64_t *o = backend_states + 6 * (size_t)q;
            o[0] = h[(size_t)q].succ; o[1] = h[(size_t)q].fail; o[2] = h[(size_t)q].has_time ? h[(size_t)q].last_time : -1;
            o[3] = h[(size_t)q].last_passed; o[4] = h[(size_t)q].is_checking; o[5] = h[(size_t)q].pending;
        }
    }
    if (healthy && lp.rt_cnt > 0) {
        if (g->ctl.hl_flag) HS_HIP(g, hipMemcpy(healthy, g->ctl.hl_flag + lp.rt_off, (size_t)lp.rt_cnt, hipMemcpyDeviceToHost));
        else std::copy(g->hl_flag.begin() + lp.rt_off, g->hl_flag.begin() + lp.rt_off + lp.rt_cnt, healthy);
    }
    if (marks) { marks[0] = g->d_health ? ls.qhead : 0; marks[1] = g->d_health ? ls.qtail : 0; }
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k) events[k] = v.health_by_kind[k];
    }
    return HS_OK;
}

int64_t hs_graph_get_lb_current_weights(hs_graph *g, int32_t node, int64_t *out, uint8_t *present, int32_t n) {
    if (!g || !out) return fail(g, HS_E_INVALID, "null argument");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "get_lb_current_weights: node %d is not a LoadBalancer", node);
    const GParam &p = g->params[(size_t)node];
    if (n != p.rt_cnt) return fail(g, HS_E_INVALID, "get_lb_current_weights: node %d has %d backends, got room for %d", node, p.rt_cnt, n);
    if (!g->ctl.wrr_cur) return 0;             // (no health state: the periodic table ran, the weights follow from the counts)
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (n > 0) {
        HS_HIP(g, hipMemcpy(out, g->ctl.wrr_cur + p.rt_off, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (present) {
            std::vector<GHc> h((size_t)n);
            HS_HIP(g, hipMemcpy(h.data(), g->ctl.hc + p.rt_off, h.size() * sizeof(GHc), hipMemcpyDeviceToHost));
            for (int q = 0; q < n; ++q) present[q] = h[(size_t)q].wrr_seen ? 1 : 0;
        }
    }
    return 1;
}

int hs_graph_set_wrapper(hs_graph *g, int32_t node, int32_t max_concurrent, int32_t max_wait_queue, double max_wait_time_s, double timeout_s,
                         int32_t table_capacity) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || (g->params[(size_t)node].kind != HS_NODE_BULKHEAD && g->params[(size_t)node].kind != HS_NODE_TIMEOUT_WRAPPER))
        return fail(g, HS_E_INVALID, "set_wrapper: node %d is neither a Bulkhead nor a TimeoutWrapper", node);
    if (g->ran || g->launches > 0 || g->ctl.rs_tab) return fail(g, HS_E_STATE, "set_wrapper: a wrapper is configured before the first run");
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "set_wrapper: node %d is configured already", node);
    GParam &p = g->params[(size_t)node];
    if (p.kind == HS_NODE_BULKHEAD) {
        // the reference's own checks (bulkhead.py:98-103)
        if (max_concurrent < 1) return fail(g, HS_E_INVALID, "max_concurrent must be >= 1, got %d", max_concurrent);
        if (max_wait_queue < 0) return fail(g, HS_E_INVALID, "max_wait_queue must be >= 0, got %d", max_wait_queue);
        if (std::isnan(max_wait_time_s) || max_wait_time_s == 0.0 || std::isinf(max_wait_time_s))
            return fail(g, HS_E_INVALID, "max_wait_time must be > 0 or None, got %g", max_wait_time_s);
        if (max_concurrent > kMaxBulkheadConcurrent)
            return fail(g, HS_E_UNSUPPORTED, "Bulkhead: max_concurrent = %d is beyond the %d ids its in-flight table holds", max_concurrent, kMaxBulkheadConcurrent);
        p.conc = max_concurrent; p.lim = max_wait_queue;
        p.sub = max_wait_time_s > 0.0 ? 1 : 0;                 // (negative: None)
        p.lat_min = p.sub ? max_wait_time_s : 0.0;
        g->tab_cap[(size_t)node] = max_concurrent;
        if (p.sub) g->reach_s = std::max(g->reach_s, max_wait_time_s);
    } else {
        if (!std::isfinite(timeout_s) || !(timeout_s > 0.0)) return fail(g, HS_E_INVALID, "timeout must be > 0, got %g", timeout_s);   // timeout.py:76-77
        if (table_capacity < 0 || table_capacity > (1 << 28)) return fail(g, HS_E_INVALID, "set_wrapper: table_capacity %d out of range", table_capacity);
        p.lat_min = timeout_s;
        g->tab_cap[(size_t)node] = table_capacity > 0 ? table_capacity : kDefaultTimeoutTable;
        g->reach_s = std::max(g->reach_s, timeout_s);
    }
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

int hs_graph_get_wrapper(hs_graph *g, int32_t node, int64_t *counters, int64_t *queue_ids, int64_t queue_cap, int64_t *in_flight_ids,
                         int64_t in_flight_cap, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < 6; ++k) events[k] = v.resil_by_kind[k];
    }
    if (node == -1 && !counters && !queue_ids && !in_flight_ids) return HS_OK;          // the graph's event counts alone
    if (node < 0 || node >= g->n || (g->params[(size_t)node].kind != HS_NODE_BULKHEAD && g->params[(size_t)node].kind != HS_NODE_TIMEOUT_WRAPPER))
        return fail(g, HS_E_INVALID, "get_wrapper: node %d is neither a Bulkhead nor a TimeoutWrapper", node);
    if (!g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "get_wrapper: node %d was never configured", node);
    const GParam &p = g->params[(size_t)node];
    const bool bh = p.kind == HS_NODE_BULKHEAD;
    GState s{};
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    const int64_t live = bh ? s.active : s.qlen;
    if (counters) {
        int32_t peaks[2];
        std::memcpy(peaks, &s.total_service, sizeof peaks);
        for (int k = 0; k < HS_WRAPPER_COUNTERS; ++k) counters[k] = 0;
        counters[0] = s.a; counters[1] = s.b; counters[2] = s.c;
        if (bh) { counters[3] = s.d; counters[4] = (int64_t)s.svc_draws - s.b; counters[5] = peaks[0]; counters[6] = peaks[1]; counters[7] = s.active; counters[8] = s.qlen; }
        counters[9] = (int64_t)s.svc_draws; counters[10] = live; counters[11] = g->ctl.rs_tab ? p.rt_cnt : g->tab_cap[(size_t)node];
    }
    if (in_flight_ids && in_flight_cap > 0 && live > 0 && g->ctl.rs_tab)
        HS_HIP(g, hipMemcpy(in_flight_ids, g->ctl.rs_tab + p.rt_off, (size_t)std::min<int64_t>(live, in_flight_cap) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (bh && queue_ids && queue_cap > 0 && s.qlen > 0) {
        // the wait queue is a list through the Request pool: walked on a copy of the pool
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        std::vector<GRequest> pool((size_t)std::max(v.req_len, 1));
        HS_HIP(g, hipMemcpy(pool.data(), g->ctl.reqs, (size_t)v.req_len * sizeof(GRequest), hipMemcpyDeviceToHost));
        int64_t k = 0;
        for (int r = s.qhead; r >= 0 && r < v.req_len && k < queue_cap && k < s.qlen; r = pool[(size_t)r].next) {
            int64_t id;
            std::memcpy(&id, &pool[(size_t)r].service_s, sizeof id);
            queue_ids[k++] = id;
        }
        if (k != std::min<int64_t>(s.qlen, queue_cap)) return fail(g, HS_E_INVALID, "get_wrapper: the wait queue of node %d is broken (internal error)", node);
    }
    return HS_OK;
}

static int set_hedge_common(hs_graph *g, int32_t node, int kind, const char *what, int32_t table_capacity) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != kind) return fail(g, HS_E_INVALID, "%s: node %d is not a %s", what, node, kind == HS_NODE_HEDGE ? "Hedge" : "Fallback");
    if (g->ran || g->launches > 0 || g->d_hg) return fail(g, HS_E_STATE, "%s: a wrapper is configured before the first run", what);
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "%s: node %d is configured already", what, node);
    if (table_capacity < 0 || table_capacity > 2 * HS_HEDGE_MAX_IN_FLIGHT) return fail(g, HS_E_INVALID, "%s: table_capacity %d out of range", what, table_capacity);
    int cap = 1;                               // the table's places: a power of two
    while (cap < (table_capacity > 0 ? table_capacity : kDefaultHedgeTable)) cap *= 2;
    g->tab_cap[(size_t)node] = cap;
    return HS_OK;
}

int hs_graph_set_hedge(hs_graph *g, int32_t node, int64_t hedge_delay_ns, int32_t max_hedges, int32_t table_capacity) {
    { const int rc = set_hedge_common(g, node, HS_NODE_HEDGE, "set_hedge", table_capacity); if (rc) return rc; }
    if (hedge_delay_ns < 0 || hedge_delay_ns > (1ll << 61)) return fail(g, HS_E_INVALID, "set_hedge: hedge_delay of %lld ns out of range", (long long)hedge_delay_ns);
    if (max_hedges < 1) return fail(g, HS_E_INVALID, "max_hedges must be >= 1, got %d", max_hedges);                     // hedge.py:86-87
    if (max_hedges > HS_HEDGE_MAX_HEDGES)
        return fail(g, HS_E_UNSUPPORTED, "Hedge: max_hedges = %d is beyond the %d a request's entry counts", max_hedges, HS_HEDGE_MAX_HEDGES);
    GParam &p = g->params[(size_t)node];
    p.lim = hedge_delay_ns; p.conc = max_hedges;
    g->reach_s = std::max(g->reach_s, (double)hedge_delay_ns * 1e-9);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

int hs_graph_set_fallback(hs_graph *g, int32_t node, int32_t fallback_node, int64_t timeout_ns, int32_t table_capacity) {
    { const int rc = set_hedge_common(g, node, HS_NODE_FALLBACK, "set_fallback", table_capacity); if (rc) return rc; }
    if (timeout_ns > (1ll << 61)) return fail(g, HS_E_INVALID, "set_fallback: timeout of %lld ns out of range", (long long)timeout_ns);
    if (fallback_node < 0 || fallback_node >= g->n) return fail(g, HS_E_INVALID, "set_fallback: fallback node %d out of range", fallback_node);
    {
        const int k = g->params[(size_t)fallback_node].kind;
        if (k == HS_NODE_SOURCE || k == HS_NODE_PROBE || k == HS_NODE_HEALTH_CHECKER || k == HS_NODE_AUTO_SCALER || k == HS_NODE_ROLLING_DEPLOYER || k == HS_NODE_CANARY_DEPLOYER)
            return fail(g, HS_E_INVALID, "node %d: its fallback entity %d takes no Requests", node, fallback_node);
        int t = fallback_node;
        for (int hops = 0; hops <= g->n && t >= 0 && g->params[(size_t)t].kind == HS_NODE_LINK; ++hops) t = g->params[(size_t)t].target;
        if (t >= 0 && hook_refused(g->params[(size_t)t].kind))
            return fail(g, HS_E_UNSUPPORTED, "node %d: the fallback entity of a Fallback is (through %s) node %d, %s", node,
                        t == fallback_node ? "no link" : "its links", t, hook_refused(g->params[(size_t)t].kind));
    }
    GParam &p = g->params[(size_t)node];
    p.lim = timeout_ns < 0 ? -1 : timeout_ns; p.conc = fallback_node;
    if (timeout_ns > 0) g->reach_s = std::max(g->reach_s, (double)timeout_ns * 1e-9);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

// hs_graph_get_hedge / hs_graph_get_fallback: the counters, then the live entries of the node's table
static int get_hedge_common(hs_graph *g, int32_t node, int kind, const char *what, int64_t *counters, int64_t *entries, int64_t cap, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < HS_HEDGE_KINDS; ++k) events[k] = v.hg_by_kind[k];
    }
    if (node == -1 && !counters && !entries) return HS_OK;
    const bool hedge = kind == HS_NODE_HEDGE;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != kind) return fail(g, HS_E_INVALID, "%s: node %d is not a %s", what, node, hedge ? "Hedge" : "Fallback");
    if (!g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "%s: node %d was never configured", what, node);
    const GParam &p = g->params[(size_t)node];
    GState s{};
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    int64_t extra;
    std::memcpy(&extra, &s.total_service, sizeof extra);
    const long long tab_cap = g->d_hg ? g->hg_rows[(size_t)p.rt_off].cap : g->tab_cap[(size_t)node];
    if (counters) {
        int k = 0;
        counters[k++] = s.a; counters[k++] = s.b; counters[k++] = s.c; counters[k++] = s.d; counters[k++] = extra;
        if (!hedge) counters[k++] = 0;                     // fallback_failures: the reference never counts one
        counters[k++] = (int64_t)s.svc_draws; counters[k++] = s.qlen; counters[k++] = tab_cap;
    }
    if (entries && cap > 0 && s.qlen > 0 && g->d_hg) {
        const GHg &row = g->hg_rows[(size_t)p.rt_off];
        std::vector<GHgEnt> tab((size_t)row.cap);
        HS_HIP(g, hipMemcpy(tab.data(), row.tab, tab.size() * sizeof(GHgEnt), hipMemcpyDeviceToHost));
        int64_t k = 0;
        for (const GHgEnt &en : tab) {
            if (en.id == 0 || k >= cap) continue;
            if (hedge) {
                int64_t *o = entries + 5 * k;
                o[0] = en.id; o[1] = en.start; o[2] = en.st & 1; o[3] = (en.st >> kHgSentShift) & 0xffffffll; o[4] = (int64_t)((uint64_t)en.st >> kHgRecvShift);
            } else {
                int64_t *o = entries + 3 * k;
                o[0] = en.id; o[1] = en.start; o[2] = en.st;
            }
            ++k;
        }
        if (k != std::min<int64_t>(s.qlen, cap)) return fail(g, HS_E_INVALID, "%s: the table of node %d is broken (internal error)", what, node);
    }
    return HS_OK;
}
int hs_graph_get_hedge(hs_graph *g, int32_t node, int64_t *counters, int64_t *entries, int64_t cap, int64_t *events) {
    return get_hedge_common(g, node, HS_NODE_HEDGE, "get_hedge", counters, entries, cap, events);
}
int hs_graph_get_fallback(hs_graph *g, int32_t node, int64_t *counters, int64_t *entries, int64_t cap, int64_t *events) {
    return get_hedge_common(g, node, HS_NODE_FALLBACK, "get_fallback", counters, entries, cap, events);
}

int hs_graph_set_client(hs_graph *g, int32_t node, double timeout_s, const int64_t *delays_ns, int32_t n_delays, int32_t table_capacity) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_CLIENT) return fail(g, HS_E_INVALID, "set_client: node %d is not a Client", node);
    if (g->ran || g->launches > 0 || g->ctl.rs_tab) return fail(g, HS_E_STATE, "set_client: a Client is configured before the first run");
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "set_client: node %d is configured already", node);
    if (std::isnan(timeout_s) || std::isinf(timeout_s)) return fail(g, HS_E_INVALID, "set_client: timeout must be finite or negative (None)");
    if (n_delays < 0) return fail(g, HS_E_INVALID, "max_attempts must be >= 1, got %d", n_delays + 1);                  // retry.py:115-116
    if (n_delays + 1 > kMaxClientAttempts)
        return fail(g, HS_E_UNSUPPORTED, "Client: max_attempts = %d is beyond the %d attempts a key holds", n_delays + 1, kMaxClientAttempts);
    if (n_delays > 0 && !delays_ns) return fail(g, HS_E_INVALID, "set_client: %d delays without a table", n_delays);
    for (int k = 0; k < n_delays; ++k)
        if (delays_ns[k] < 0) return fail(g, HS_E_INVALID, "delay must be >= 0, got %g", (double)delays_ns[k] / 1e9);   // retry.py:117-118
    if (table_capacity < 0 || table_capacity > (1 << 27)) return fail(g, HS_E_INVALID, "set_client: table_capacity %d out of range", table_capacity);
    GParam &p = g->params[(size_t)node];
    p.sub = timeout_s >= 0.0 ? 1 : 0;                      // (negative: None; 0 is legal, client.py:89-90)
    p.lat_min = p.sub ? timeout_s : 0.0;
    p.conc = n_delays; p.lim = (int64_t)g->cl_delays.size();
    g->cl_delays.insert(g->cl_delays.end(), delays_ns, delays_ns + n_delays);
    g->tab_cap[(size_t)node] = table_capacity > 0 ? table_capacity : kDefaultTimeoutTable;
    double reach = p.lat_min;
    for (int k = 0; k < n_delays; ++k) reach = std::max(reach, (double)delays_ns[k] / 1e9);
    g->reach_s = std::max(g->reach_s, reach);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

int hs_graph_get_client(hs_graph *g, int32_t node, int64_t *counters, int64_t *in_flight_keys, int64_t cap, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < 3; ++k) events[k] = v.client_by_kind[k];
    }
    if (node == -1 && !counters && !in_flight_keys) return HS_OK;                       // the graph's event counts alone
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_CLIENT) return fail(g, HS_E_INVALID, "get_client: node %d is not a Client", node);
    if (!g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "get_client: node %d was never configured", node);
    const GParam &p = g->params[(size_t)node];
    GState s{};
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    if (counters) {
        counters[0] = s.a; counters[1] = s.b; counters[2] = s.c; counters[3] = s.d; counters[4] = (int64_t)s.svc_draws; counters[5] = s.qlen;
        counters[6] = g->ctl.rs_tab ? p.rt_cnt : g->tab_cap[(size_t)node];
    }
    const int64_t take = std::min<int64_t>(s.qlen, cap);
    if (in_flight_keys && take > 0 && g->ctl.rs_tab) {
        std::vector<int64_t> rows((size_t)take * 2);
        HS_HIP(g, hipMemcpy(rows.data(), g->ctl.rs_tab + p.rt_off, rows.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < take; ++k) {                                            // (request_id or 0, attempt) pairs
            in_flight_keys[2 * k] = rows[(size_t)(2 * k)] & ((1ll << kKeyAttemptShift) - 1);
            in_flight_keys[2 * k + 1] = rows[(size_t)(2 * k)] >> kKeyAttemptShift;
        }
    }
    return HS_OK;
}

int hs_graph_set_flow(hs_graph *g, int32_t node, int64_t count, int64_t delay_ns, int64_t aux_ns, int32_t flag) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind < HS_NODE_BATCH_PROCESSOR || g->params[(size_t)node].kind > HS_NODE_GATE)
        return fail(g, HS_E_INVALID, "set_flow: node %d is not a BatchProcessor, ConveyorBelt or GateController", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_flow: a node is configured before the first run");
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "set_flow: node %d is configured already", node);
    GParam &p = g->params[(size_t)node];
    GState s0{};
    s0.qhead = -1; s0.qtail = -1;
    if (delay_ns > (1ll << 61) || aux_ns > (1ll << 61)) return fail(g, HS_E_INVALID, "set_flow: a delay beyond 2^61 ns");
    if (p.kind == HS_NODE_BATCH_PROCESSOR) {
        if (count <= 0) return fail(g, HS_E_INVALID, "batch_size must be > 0, got %lld", (long long)count);                      // batch_processor.py:59-60
        if (delay_ns < 0) return fail(g, HS_E_INVALID, "process_time must be >= 0, got %g", (double)delay_ns / 1e9);             // :61-62
        if (count > kMaxFlowItems) return fail(g, HS_E_UNSUPPORTED, "BatchProcessor: batch_size = %lld is beyond the %d items of one batch", (long long)count, kMaxFlowItems);
        p.conc = (int32_t)count; p.lim = delay_ns; p.sub = aux_ns > 0 ? 1 : 0; p.stream_base = (uint64_t)(aux_ns > 0 ? aux_ns : 0);
    } else if (p.kind == HS_NODE_CONVEYOR) {
        if (delay_ns < 0) return fail(g, HS_E_INVALID, "transit_time must be >= 0, got %g", (double)delay_ns / 1e9);             // conveyor.py:53-54
        p.conc = (int32_t)std::min<int64_t>(std::max<int64_t>(count, 0), INT32_MAX); p.lim = delay_ns; p.sub = 0; p.stream_base = 0;
    } else {
        if (count > kMaxFlowItems) return fail(g, HS_E_UNSUPPORTED, "GateController: queue_capacity = %lld is beyond %d items (0: unbounded)", (long long)count, kMaxFlowItems);
        p.conc = (int32_t)std::max<int64_t>(count, 0); p.lim = 0; p.sub = flag ? 1 : 0; p.stream_base = 0;
        s0.active = flag ? 1 : 0;                           // _is_open
        s0.d = aux_ns > 0 ? aux_ns : 0;                     // _open_cycles so far: open() on the host before the run
        delay_ns = 0; aux_ns = 0;
    }
    g->reach_s = std::max(g->reach_s, (double)std::max(delay_ns, aux_ns) / 1e9);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    HS_HIP(g, hipMemcpy(g->ctl.S + node, &s0, sizeof s0, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

int hs_graph_schedule_gate(hs_graph *g, int32_t node, int64_t time_ns, int32_t open) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_GATE) return fail(g, HS_E_INVALID, "schedule_gate: node %d is not a GateController", node);
    g->sched_node.push_back(node);
    g->sched_t.push_back(time_ns);
    g->sched_id.push_back(open ? -1 : -2);                 // (negative: no request id but a gate Event)
    g->any_sched_id = true;
    return HS_OK;
}

int hs_graph_get_flow(hs_graph *g, int32_t node, int64_t *counters, int64_t *events, int64_t *cancelled) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events || cancelled) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        if (events) for (int k = 0; k < HS_FLOW_KINDS; ++k) events[k] = v.flow_by_kind[k];
        if (cancelled) *cancelled = v.flow_cancelled;
    }
    if (node == -1 && !counters) return HS_OK;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind < HS_NODE_BATCH_PROCESSOR || g->params[(size_t)node].kind > HS_NODE_GATE)
        return fail(g, HS_E_INVALID, "get_flow: node %d is not a BatchProcessor, ConveyorBelt or GateController", node);
    if (!g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "get_flow: node %d was never configured", node);
    if (!counters) return HS_OK;
    GState s{};
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    for (int k = 0; k < HS_FLOW_COUNTERS; ++k) counters[k] = 0;
    switch (g->params[(size_t)node].kind) {
    case HS_NODE_BATCH_PROCESSOR: counters[0] = s.a; counters[1] = s.b; counters[2] = s.c; counters[3] = s.qlen; break;
    case HS_NODE_CONVEYOR: counters[0] = s.a; counters[1] = s.b; counters[2] = s.active; break;
    default: counters[0] = s.a; counters[1] = s.b; counters[2] = s.c; counters[3] = s.d; counters[4] = s.qlen; counters[5] = s.active; break;
    }
    return HS_OK;
}

int hs_graph_set_pool(hs_graph *g, int32_t node, int32_t pool_size, int64_t cycle_ns, int32_t queue_capacity) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_POOLED_CYCLE) return fail(g, HS_E_INVALID, "set_pool: node %d is not a PooledCycleResource", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_pool: a node is configured before the first run");
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "set_pool: node %d is configured already", node);
    if (pool_size <= 0) return fail(g, HS_E_INVALID, "pool_size must be > 0, got %d", pool_size);                                // pooled_cycle.py:61-62
    if (cycle_ns < 0) return fail(g, HS_E_INVALID, "cycle_time must be >= 0, got %g", (double)cycle_ns / 1e9);                   // :63-64
    if (cycle_ns > (1ll << 61)) return fail(g, HS_E_INVALID, "set_pool: a cycle_time beyond 2^61 ns");
    if (pool_size > HS_POOL_MAX_UNITS) return fail(g, HS_E_UNSUPPORTED, "PooledCycleResource: pool_size = %d is beyond %d units", pool_size, HS_POOL_MAX_UNITS);
    if (queue_capacity > HS_POOL_MAX_UNITS)
        return fail(g, HS_E_UNSUPPORTED, "PooledCycleResource: queue_capacity = %d is beyond %d items (0: unbounded)", queue_capacity, HS_POOL_MAX_UNITS);
    GParam &p = g->params[(size_t)node];
    p.conc = pool_size; p.lim = cycle_ns; p.rt_cnt = queue_capacity > 0 ? queue_capacity : 0; p.rt_off = 0; p.sub = 0;
    GState s0{};
    s0.qhead = -1; s0.qtail = -1;
    g->reach_s = std::max(g->reach_s, (double)cycle_ns / 1e9);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    HS_HIP(g, hipMemcpy(g->ctl.S + node, &s0, sizeof s0, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

int hs_graph_set_inventory(hs_graph *g, int32_t node, int64_t initial_stock, int64_t reorder_point, int64_t order_quantity, double lead_time_s,
                           int32_t stockout_node) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_INVENTORY) return fail(g, HS_E_INVALID, "set_inventory: node %d is not an InventoryBuffer", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_inventory: a node is configured before the first run");
    if (g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "set_inventory: node %d is configured already", node);
    if (initial_stock < 0) return fail(g, HS_E_INVALID, "initial_stock must be >= 0, got %lld", (long long)initial_stock);       // inventory.py:73-78
    if (reorder_point < 0) return fail(g, HS_E_INVALID, "reorder_point must be >= 0, got %lld", (long long)reorder_point);
    if (order_quantity <= 0) return fail(g, HS_E_INVALID, "order_quantity must be > 0, got %lld", (long long)order_quantity);
    if (initial_stock > HS_INVENTORY_MAX || reorder_point > HS_INVENTORY_MAX || order_quantity > HS_INVENTORY_MAX)
        return fail(g, HS_E_UNSUPPORTED, "InventoryBuffer: a stock parameter beyond 2^62 is not lowered");
    if (reorder_point + order_quantity > HS_INVENTORY_MAX_LEVEL)       // (each <= 2^62: the sum itself cannot wrap)
        return fail(g, HS_E_UNSUPPORTED, "InventoryBuffer: reorder_point + order_quantity = %llu is beyond 2^63 - 2^48, the level a 64-bit stock holds",
                    (unsigned long long)reorder_point + (unsigned long long)order_quantity);
    if (!(lead_time_s >= 0.0) || !std::isfinite(lead_time_s) || lead_time_s > 2.0e9)
        return fail(g, HS_E_UNSUPPORTED, "InventoryBuffer: lead_time = %g is not a finite number in [0, 2e9] s", lead_time_s);
    if (stockout_node < -1 || stockout_node >= g->n) return fail(g, HS_E_INVALID, "set_inventory: stock-out node %d out of range", stockout_node);
    if (stockout_node >= 0) {
        const int k = g->params[(size_t)stockout_node].kind;
        if (k == HS_NODE_SOURCE || k == HS_NODE_PROBE || k == HS_NODE_HEALTH_CHECKER || k == HS_NODE_AUTO_SCALER || k == HS_NODE_ROLLING_DEPLOYER || k == HS_NODE_CANARY_DEPLOYER)
            return fail(g, HS_E_INVALID, "node %d: its stockout_target %d takes no Requests", node, stockout_node);
    }
    GParam &p = g->params[(size_t)node];
    p.lim = reorder_point; p.stream_base = (uint64_t)order_quantity; p.mean = lead_time_s; p.conc = stockout_node; p.sub = 0; p.rt_off = 0; p.rt_cnt = 0;
    GState s0{};
    s0.qhead = -1; s0.qtail = -1;
    s0.a = initial_stock;
    g->reach_s = std::max(g->reach_s, lead_time_s);
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    HS_HIP(g, hipMemcpy(g->ctl.S + node, &s0, sizeof s0, hipMemcpyHostToDevice));
    g->wrapper_set[(size_t)node] = 1;
    return HS_OK;
}

// hs_graph_get_pool / hs_graph_get_inventory
static int get_stock_common(hs_graph *g, int32_t node, int kind, const char *what, int64_t *counters, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < HS_STOCK_KINDS; ++k) events[k] = v.st_by_kind[k];
    }
    if (node == -1 && !counters) return HS_OK;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != kind)
        return fail(g, HS_E_INVALID, "%s: node %d is not %s", what, node, kind == HS_NODE_POOLED_CYCLE ? "a PooledCycleResource" : "an InventoryBuffer");
    if (!g->wrapper_set[(size_t)node]) return fail(g, HS_E_STATE, "%s: node %d was never configured", what, node);
    if (!counters) return HS_OK;
    GState s{};
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    if (kind == HS_NODE_POOLED_CYCLE) {
        counters[0] = (int64_t)g->params[(size_t)node].conc - s.active; counters[1] = s.active; counters[2] = s.qlen; counters[3] = s.a; counters[4] = s.b;
    } else {
        counters[0] = s.a; counters[1] = s.b; counters[2] = s.c; counters[3] = s.d; counters[4] = (int64_t)s.svc_draws; counters[5] = s.active;
    }
    return HS_OK;
}

int hs_graph_get_pool(hs_graph *g, int32_t node, int64_t *counters, int64_t *events) {
    return get_stock_common(g, node, HS_NODE_POOLED_CYCLE, "get_pool", counters, events);
}

int hs_graph_get_inventory(hs_graph *g, int32_t node, int64_t *counters, int64_t *events) {
    return get_stock_common(g, node, HS_NODE_INVENTORY, "get_inventory", counters, events);
}

int hs_graph_set_queue_policy(hs_graph *g, int32_t node, int32_t policy, int64_t capacity, int64_t threshold, double target_s, double interval_s) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_SERVER) return fail(g, HS_E_INVALID, "set_queue_policy: node %d is not a Server", node);
    if (g->ran || g->launches > 0) return fail(g, HS_E_STATE, "set_queue_policy: a Server is configured before the first run");
    GParam &p = g->params[(size_t)node];
    if (p.pad[0] != HS_QUEUE_FIFO) return fail(g, HS_E_STATE, "set_queue_policy: node %d is configured already", node);
    if (policy != HS_QUEUE_LIFO && policy != HS_QUEUE_ADAPTIVE_LIFO && policy != HS_QUEUE_CODEL)
        return fail(g, HS_E_UNSUPPORTED, "set_queue_policy: policy %d is not lowered", (int)policy);
    GQueue q{};
    q.kind = policy; q.first_above = kQueueNone; q.drop_next = kQueueNone;
    if (policy != HS_QUEUE_LIFO && capacity == 0) return fail(g, HS_E_INVALID, "capacity must be >= 1 or None, got %lld", (long long)capacity);   // adaptive_lifo.py:68-69, codel.py:93-94
    if (policy == HS_QUEUE_ADAPTIVE_LIFO) {
        if (threshold < 1) return fail(g, HS_E_INVALID, "congestion_threshold must be >= 1, got %lld", (long long)threshold);     // adaptive_lifo.py:66-67
        q.threshold = threshold;
    } else if (policy == HS_QUEUE_CODEL) {
        if (!(target_s > 0.0)) return fail(g, HS_E_INVALID, "target_delay must be > 0, got %g", target_s);                         // codel.py:89-92
        if (!(interval_s > 0.0)) return fail(g, HS_E_INVALID, "interval must be > 0, got %g", interval_s);
        if (!std::isfinite(target_s) || !(interval_s <= 4.0e9)) return fail(g, HS_E_UNSUPPORTED, "set_queue_policy: target_delay = %g, interval = %g: beyond 4e9 s or not finite", target_s, interval_s);
        q.target = target_s; q.interval = interval_s;
        g->reach_s = std::max(g->reach_s, interval_s);
    }
    if ((long long)g->qpol.size() >= (1ll << 30)) return fail(g, HS_E_UNSUPPORTED, "set_queue_policy: too many Servers with a policy");
    p.lim = capacity < 0 ? -1 : capacity;                  // the policy's own capacity: the Server's queue_capacity is ignored (server.py)
    p.pad[0] = (uint8_t)policy; p.rt_cnt = (int32_t)g->qpol.size();
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->qpol.push_back(q);
    return HS_OK;
}

int hs_graph_get_queue_policy(hs_graph *g, int32_t node, int64_t *out) {
    if (!g || !out) return fail(g, HS_E_INVALID, "null argument");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_SERVER || g->params[(size_t)node].pad[0] == HS_QUEUE_FIFO)
        return fail(g, HS_E_INVALID, "get_queue_policy: node %d is not a Server with a queue policy", node);
    const GParam &p = g->params[(size_t)node];
    GQueue q = g->qpol[(size_t)p.rt_cnt];
    GState s{};
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (g->d_qp) HS_HIP(g, hipMemcpy(&q, g->d_qp + p.rt_cnt, sizeof q, hipMemcpyDeviceToHost));
    HS_HIP(g, hipMemcpy(&s, g->ctl.S + node, sizeof s, hipMemcpyDeviceToHost));
    out[0] = q.kind; out[1] = s.qlen; out[2] = q.enqueued; out[3] = q.deq_a; out[4] = q.deq_b; out[5] = q.dropped; out[6] = q.cap_rejected;
    out[7] = q.switches; out[8] = q.flag; out[9] = q.count; out[10] = q.last_count;
    out[11] = q.first_above != kQueueNone; out[12] = q.first_above != kQueueNone ? q.first_above : 0;
    out[13] = q.drop_next != kQueueNone; out[14] = q.drop_next != kQueueNone ? q.drop_next : 0;
    out[15] = 0;
    return HS_OK;
}

int hs_debug_codel_next(int32_t device, int64_t n, const int64_t *count, const double *interval_s, int64_t *out_ns) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, HS_E_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (n <= 0 || !count || !interval_s || !out_ns) return fail(nullptr, HS_E_INVALID, "hs_debug_codel_next: bad arguments");
    if (device < 0 || device >= ndev) return fail(nullptr, HS_E_INVALID, "device ordinal %d out of range (%d devices)", device, ndev);
    for (int64_t i = 0; i < n; ++i)
        if (count[i] < 1 || !(interval_s[i] > 0.0) || !(interval_s[i] <= 4.0e9))
            return fail(nullptr, HS_E_INVALID, "hs_debug_codel_next: entry %lld is outside count >= 1, 0 < interval <= 4e9", (long long)i);
    HS_HIP(nullptr, hipSetDevice(device));
    void *d[3] = {nullptr, nullptr, nullptr};
    const size_t bytes = (size_t)n * 8;
    for (int k = 0; k < 3; ++k) {
        const hipError_t e = hipMalloc(&d[k], bytes);
        if (e != hipSuccess) { for (auto &p : d) if (p) hipFree(p); return fail(nullptr, HS_E_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    }
    hipError_t e = hipMemcpy(d[0], count, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d[1], interval_s, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(hs_debug_codel_next_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, (const int64_t *)d[0],
                           (const double *)d[1], (int64_t *)d[2]);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out_ns, d[2], bytes, hipMemcpyDeviceToHost);
    for (auto &p : d) hipFree(p);
    if (e != hipSuccess) return fail(nullptr, HS_E_HIP, "hs_debug_codel_next: %s", hipGetErrorString(e));
    return HS_OK;
}

int hs_graph_set_auto_scaler(hs_graph *g, int32_t node, int32_t lb_node, int32_t policy, double p0, double p1, int32_t n_steps,
                             const double *step_threshold, const int32_t *step_adjustment, int32_t min_instances, int32_t max_instances,
                             double interval_s, double scale_out_cooldown_s, double scale_in_cooldown_s, int32_t n_pool, int32_t running) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_AUTO_SCALER)
        return fail(g, HS_E_INVALID, "set_auto_scaler: node %d is not an AutoScaler", node);
    if (lb_node < 0 || lb_node >= g->n || g->params[(size_t)lb_node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_auto_scaler: node %d is not a LoadBalancer", lb_node);
    if (g->ran || g->launches > 0 || g->d_health || g->d_as) return fail(g, HS_E_STATE, "set_auto_scaler: a scaler is configured before the first run");
    for (int32_t a : g->as_node) if (a == node) return fail(g, HS_E_STATE, "set_auto_scaler: node %d is configured already", node);
    if (g->scaler_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has AutoScaler node %d already: one scaler per LoadBalancer is lowered", lb_node,
                    g->scaler_of[(size_t)lb_node]);
    if (g->checker_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has HealthChecker node %d: a HealthChecker and an AutoScaler on one LoadBalancer are not lowered",
                    lb_node, g->checker_of[(size_t)lb_node]);
    if (g->deployer_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has RollingDeployer node %d: an AutoScaler and a deployer on one LoadBalancer are not lowered", lb_node,
                    g->deployer_of[(size_t)lb_node]);
    const GParam &lp = g->params[(size_t)lb_node];
    if (lp.sub == HS_LB_CONSISTENT_HASH || lp.sub == HS_LB_IP_HASH || lp.sub == HS_LB_RANDOM)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: strategy %d is not lowered over a changing backend list (under an AutoScaler)", lb_node, (int)lp.sub);
    if (policy < HS_AUTOSCALER_TARGET_UTILIZATION || policy > HS_AUTOSCALER_QUEUE_DEPTH) return fail(g, HS_E_UNSUPPORTED, "scaling policy %d is not lowered", policy);
    if (policy == HS_AUTOSCALER_TARGET_UTILIZATION && !(p0 > 0.0 && p0 <= 1.0)) return fail(g, HS_E_INVALID, "target must be in (0, 1], got %g", p0);
    if (policy == HS_AUTOSCALER_STEP) {
        if (n_steps < 0 || n_steps > kMaxScalerSteps) return fail(g, HS_E_UNSUPPORTED, "StepScaling with %d steps: at most %d are lowered", n_steps, kMaxScalerSteps);
        if (n_steps > 0 && (!step_threshold || !step_adjustment)) return fail(g, HS_E_INVALID, "set_auto_scaler: null steps");
        for (int k = 0; k < n_steps; ++k) if (std::isnan(step_threshold[k])) return fail(g, HS_E_INVALID, "set_auto_scaler: step %d has no threshold", k);
    }
    if (n_pool < 0 || n_pool > HS_AUTOSCALER_MAX_POOL) return fail(g, HS_E_UNSUPPORTED, "a pool of %d instances is beyond the %d of one AutoScaler", n_pool, HS_AUTOSCALER_MAX_POOL);
    if (n_pool > lp.rt_cnt) return fail(g, HS_E_INVALID, "set_auto_scaler: LoadBalancer node %d has %d targets, fewer than the pool's %d", lb_node, lp.rt_cnt, n_pool);
    if (!std::isfinite(interval_s) || !(interval_s * 1e9 >= 1.0))
        return fail(g, HS_E_UNSUPPORTED, "an evaluation_interval of %g s is below one nanosecond or not finite (the evaluation would never advance)", interval_s);
    if (std::isnan(scale_out_cooldown_s) || std::isnan(scale_in_cooldown_s)) return fail(g, HS_E_INVALID, "set_auto_scaler: a cooldown is not a number");
    for (int q = 0; q < lp.rt_cnt - n_pool; ++q)
        if (!g->hl_flag[(size_t)lp.rt_off + (size_t)q])
            return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: backend %d is marked unhealthy under an AutoScaler (not lowered)", lb_node, q);
    GAs row{};
    row.policy = policy;
    row.target = policy == HS_AUTOSCALER_TARGET_UTILIZATION ? p0 : 0.7;
    row.thr_out = p0; row.thr_in = p1;
    row.n_steps = policy == HS_AUTOSCALER_STEP ? n_steps : 0;
    for (int k = 0; k < row.n_steps; ++k) { row.step_thr[k] = step_threshold[k]; row.step_adj[k] = step_adjustment[k]; }
    GParam &p = g->params[(size_t)node];
    p.target = lb_node; p.mean = interval_s; p.lat_min = scale_out_cooldown_s; p.loss = scale_in_cooldown_s; p.conc = min_instances;
    p.lim = max_instances; p.sub = running ? 1 : 0; p.rt_off = lp.rt_cnt - n_pool; p.rt_cnt = n_pool; p.stream_base = (uint64_t)g->as_rows.size();
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    for (int q = lp.rt_cnt - n_pool; q < lp.rt_cnt; ++q) g->as_member[(size_t)lp.rt_off + (size_t)q] = 0;
    g->as_rows.push_back(row); g->as_node.push_back(node);
    g->scaler_of[(size_t)lb_node] = node;
    g->reach_s = std::max(g->reach_s, interval_s);
    g->health = true;                          // (the member list is the healthy list of the health lowering)
    return HS_OK;
}

int hs_graph_get_auto_scaler(hs_graph *g, int32_t node, int64_t *state, int64_t *history, int64_t history_cap, uint8_t *member, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        *events = v.as_evals;
    }
    if (node == -1 && !state && !history && !member) return HS_OK;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_AUTO_SCALER)
        return fail(g, HS_E_INVALID, "get_auto_scaler: node %d is not an AutoScaler", node);
    const GParam &np = g->params[(size_t)node];
    size_t r = 0;
    while (r < g->as_node.size() && g->as_node[r] != node) ++r;
    if (r == g->as_node.size()) return fail(g, HS_E_STATE, "get_auto_scaler: AutoScaler node %d was never configured", node);
    const GParam &lp = g->params[(size_t)np.target];
    GAs row = g->as_rows[r];
    GState cs{}, ls{};
    if (g->d_as) {
        HS_HIP(g, hipMemcpy(&row, g->d_as + r, sizeof row, hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(&cs, g->ctl.S + node, sizeof cs, hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(&ls, g->ctl.S + np.target, sizeof ls, hipMemcpyDeviceToHost));
    } else ls.qlen = lp.rt_cnt - np.rt_cnt;
    if (state) {
        state[0] = cs.a; state[1] = cs.b; state[2] = cs.c; state[3] = row.added; state[4] = row.removed; state[5] = cs.d;
        state[6] = row.next_id; state[7] = row.last_action; state[8] = row.last_action ? row.last_time : -1; state[9] = row.hist_len;
        state[10] = ls.qlen; state[11] = 0;
    }
    if (history && history_cap > 0 && row.hist_len > 0 && g->d_as)
        HS_HIP(g, hipMemcpy(history, row.hist, 4 * (size_t)std::min<long long>(row.hist_len, history_cap) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (member && lp.rt_cnt > 0) {
        if (g->d_as_mem) HS_HIP(g, hipMemcpy(member, g->d_as_mem + lp.rt_off, (size_t)lp.rt_cnt, hipMemcpyDeviceToHost));
        else std::copy(g->as_member.begin() + lp.rt_off, g->as_member.begin() + lp.rt_off + lp.rt_cnt, member);
    }
    return HS_OK;
}

int hs_graph_set_rolling_deployer(hs_graph *g, int32_t node, int32_t lb_node, int32_t batch_size, double interval_s, int32_t healthy_threshold,
                                  int64_t max_failures, int32_t n_pool) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_ROLLING_DEPLOYER)
        return fail(g, HS_E_INVALID, "set_rolling_deployer: node %d is not a RollingDeployer", node);
    if (lb_node < 0 || lb_node >= g->n || g->params[(size_t)lb_node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_rolling_deployer: node %d is not a LoadBalancer", lb_node);
    if (g->ran || g->launches > 0 || g->d_health || g->d_rd) return fail(g, HS_E_STATE, "set_rolling_deployer: a deployer is configured before the first run");
    for (int32_t a : g->rd_node) if (a == node) return fail(g, HS_E_STATE, "set_rolling_deployer: node %d is configured already", node);
    if (g->deployer_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has RollingDeployer node %d already: one deployer per LoadBalancer is lowered", lb_node,
                    g->deployer_of[(size_t)lb_node]);
    if (g->scaler_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has AutoScaler node %d: an AutoScaler and a deployer on one LoadBalancer are not lowered", lb_node,
                    g->scaler_of[(size_t)lb_node]);
    if (g->checker_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has HealthChecker node %d: a HealthChecker and a deployer on one LoadBalancer are not lowered",
                    lb_node, g->checker_of[(size_t)lb_node]);
    const GParam &lp = g->params[(size_t)lb_node];
    if (lp.sub != HS_LB_ROUND_ROBIN && lp.sub != HS_LB_WEIGHTED_ROUND_ROBIN && lp.sub != HS_LB_LEAST_CONNECTIONS && lp.sub != HS_LB_WEIGHTED_LEAST_CONNECTIONS)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: strategy %d is not lowered over a changing backend list (under a deployer)", lb_node, (int)lp.sub);
    if (batch_size < 1) return fail(g, HS_E_INVALID, "batch_size must be at least 1, got %d", batch_size);
    if (healthy_threshold < 1) return fail(g, HS_E_INVALID, "healthy_threshold must be at least 1, got %d", healthy_threshold);
    if (!std::isfinite(interval_s) || !(interval_s * 1e9 >= 1.0))
        return fail(g, HS_E_UNSUPPORTED, "a health_check_interval of %g s is below one nanosecond or not finite", interval_s);
    if (n_pool < 0 || n_pool > HS_DEPLOYER_MAX_POOL) return fail(g, HS_E_UNSUPPORTED, "a pool of %d instances is beyond the %d of one deployer", n_pool, HS_DEPLOYER_MAX_POOL);
    if (n_pool > lp.rt_cnt) return fail(g, HS_E_INVALID, "set_rolling_deployer: LoadBalancer node %d has %d targets, fewer than the pool's %d", lb_node, lp.rt_cnt, n_pool);
    for (int q = 0; q < lp.rt_cnt - n_pool; ++q)
        if (!g->hl_flag[(size_t)lp.rt_off + (size_t)q])
            return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: backend %d is marked unhealthy under a deployer (not lowered)", lb_node, q);
    GRd row{};
    row.cap = lp.rt_cnt; row.batch_size = batch_size; row.lb = lb_node;
    GParam &p = g->params[(size_t)node];
    p.target = lb_node; p.mean = interval_s; p.conc = healthy_threshold; p.lim = max_failures; p.rt_off = lp.rt_cnt - n_pool; p.rt_cnt = n_pool;
    p.stream_base = (uint64_t)g->rd_rows.size();
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    for (int q = lp.rt_cnt - n_pool; q < lp.rt_cnt; ++q) g->as_member[(size_t)lp.rt_off + (size_t)q] = 0;
    g->rd_rows.push_back(row); g->rd_node.push_back(node);
    g->deployer_of[(size_t)lb_node] = node;
    g->reach_s = std::max(g->reach_s, interval_s);
    g->health = true;                          // (the member list is the healthy list of the health lowering)
    return HS_OK;
}

int hs_graph_get_rolling_deployer(hs_graph *g, int32_t node, int64_t *state, int32_t *lists, int32_t *members, int32_t *pass, int32_t *readded,
                                  int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < HS_DEPLOYER_KINDS; ++k) events[k] = v.rd_by_kind[k];
        events[HS_DEPLOYER_KINDS] = v.rd_compactions[0]; events[HS_DEPLOYER_KINDS + 1] = v.rd_compactions[1];
    }
    if (node == -1 && !state && !lists && !members && !pass && !readded) return HS_OK;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_ROLLING_DEPLOYER)
        return fail(g, HS_E_INVALID, "get_rolling_deployer: node %d is not a RollingDeployer", node);
    const GParam &np = g->params[(size_t)node];
    size_t r = 0;
    while (r < g->rd_node.size() && g->rd_node[r] != node) ++r;
    if (r == g->rd_node.size()) return fail(g, HS_E_STATE, "get_rolling_deployer: RollingDeployer node %d was never configured", node);
    const GParam &lp = g->params[(size_t)np.target];
    const size_t cap = (size_t)lp.rt_cnt;
    GRd row = g->rd_rows[r];
    GState ls{};
    std::vector<int32_t> all(6 * std::max<size_t>(cap, 1), -1), hl(std::max<size_t>(cap, 1), 0);
    if (g->d_rd) {
        HS_HIP(g, hipMemcpy(&row, g->d_rd + r, sizeof row, hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(&ls, g->ctl.S + np.target, sizeof ls, hipMemcpyDeviceToHost));
        if (cap) HS_HIP(g, hipMemcpy(all.data(), g->d_rd_lists[r], 6 * cap * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (cap) HS_HIP(g, hipMemcpy(hl.data(), g->ctl.hl_list + lp.rt_off, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
    } else {
        ls.qlen = lp.rt_cnt - np.rt_cnt;
        for (int q = 0; q < ls.qlen; ++q) hl[(size_t)q] = q;
    }
    if (state) {
        const int64_t out[HS_DEPLOYER_FIELDS] = {row.started, row.completed, row.rolled_back, row.inst_replaced, row.hc_performed, row.hc_passed, row.hc_failed,
                                                 row.status, row.total, row.replaced, row.failed, row.cur_batch, row.next_id, row.fail_count,
                                                 row.old_n - row.old_head, row.new_n, row.cur_old_n, row.cur_new_n, ls.qlen, 0};
        std::copy(out, out + HS_DEPLOYER_FIELDS, state);
    }
    if (lists && cap) {
        std::fill(lists, lists + 4 * cap, -1);
        std::copy(all.begin() + row.old_head, all.begin() + row.old_n, lists);
        std::copy(all.begin() + cap, all.begin() + cap + row.new_n, lists + cap);
        std::copy(all.begin() + 2 * cap, all.begin() + 2 * cap + row.cur_old_n, lists + 2 * cap);
        std::copy(all.begin() + 3 * cap, all.begin() + 3 * cap + row.cur_new_n, lists + 3 * cap);
    }
    if (members && cap) { std::fill(members, members + cap, -1); std::copy(hl.begin(), hl.begin() + ls.qlen, members); }
    if (pass && cap) std::copy(all.begin() + 4 * cap, all.begin() + 5 * cap, pass);
    if (readded && cap) for (size_t q = 0; q < cap; ++q) readded[q] = all[5 * cap + q] > 0 ? 1 : 0;
    return HS_OK;
}

int hs_graph_set_canary_deployer(hs_graph *g, int32_t node, int32_t lb_node, int32_t n_stages, const double *traffic_percentage,
                                 const double *evaluation_period, int32_t evaluator, double ev_max, double ev_multiplier, double interval_s) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_CANARY_DEPLOYER)
        return fail(g, HS_E_INVALID, "set_canary_deployer: node %d is not a CanaryDeployer", node);
    if (lb_node < 0 || lb_node >= g->n || g->params[(size_t)lb_node].kind != HS_NODE_LB)
        return fail(g, HS_E_INVALID, "set_canary_deployer: node %d is not a LoadBalancer", lb_node);
    if (g->ran || g->launches > 0 || g->d_health || g->d_cn) return fail(g, HS_E_STATE, "set_canary_deployer: a deployer is configured before the first run");
    for (int32_t a : g->cn_node) if (a == node) return fail(g, HS_E_STATE, "set_canary_deployer: node %d is configured already", node);
    if (g->deployer_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has deployer node %d already: one deployer per LoadBalancer is lowered", lb_node,
                    g->deployer_of[(size_t)lb_node]);
    if (g->scaler_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has AutoScaler node %d: an AutoScaler and a deployer on one LoadBalancer are not lowered", lb_node,
                    g->scaler_of[(size_t)lb_node]);
    if (g->checker_of[(size_t)lb_node] >= 0)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d has HealthChecker node %d: a HealthChecker and a deployer on one LoadBalancer are not lowered",
                    lb_node, g->checker_of[(size_t)lb_node]);
    const GParam &lp = g->params[(size_t)lb_node];
    if (lp.sub != HS_LB_ROUND_ROBIN && lp.sub != HS_LB_WEIGHTED_ROUND_ROBIN && lp.sub != HS_LB_LEAST_CONNECTIONS && lp.sub != HS_LB_WEIGHTED_LEAST_CONNECTIONS)
        return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: strategy %d is not lowered over a changing backend list (under a deployer)", lb_node, (int)lp.sub);
    if (n_stages < 1 || n_stages > HS_CANARY_MAX_STAGES || !traffic_percentage || !evaluation_period)
        return fail(g, HS_E_UNSUPPORTED, "a CanaryDeployer with %d stages: 1 .. %d are lowered", n_stages, HS_CANARY_MAX_STAGES);
    for (int k = 0; k < n_stages; ++k)
        if (!std::isfinite(traffic_percentage[k]) || !std::isfinite(evaluation_period[k]))
            return fail(g, HS_E_INVALID, "set_canary_deployer: stage %d has a traffic_percentage or evaluation_period that is no finite number", k);
    if (evaluator != HS_CANARY_ERROR_RATE && evaluator != HS_CANARY_LATENCY) return fail(g, HS_E_UNSUPPORTED, "metric evaluator %d is not lowered", evaluator);
    if (std::isnan(ev_max) || std::isnan(ev_multiplier)) return fail(g, HS_E_INVALID, "set_canary_deployer: an evaluator parameter is no number");
    if (!std::isfinite(interval_s) || !(interval_s * 1e9 >= 1.0))
        return fail(g, HS_E_UNSUPPORTED, "an evaluation_interval of %g s is below one nanosecond or not finite", interval_s);
    if (lp.rt_cnt < 1) return fail(g, HS_E_INVALID, "set_canary_deployer: LoadBalancer node %d has no target for the canary", lb_node);
    for (int q = 0; q < lp.rt_cnt - 1; ++q)
        if (!g->hl_flag[(size_t)lp.rt_off + (size_t)q])
            return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: backend %d is marked unhealthy under a deployer (not lowered)", lb_node, q);
    GCn row{};
    row.cap = lp.rt_cnt; row.lb = lb_node; row.n_stages = n_stages; row.evaluator = evaluator; row.ev_max = ev_max; row.ev_mult = ev_multiplier;
    for (int k = 0; k < n_stages; ++k) { row.pct[k] = traffic_percentage[k]; row.period[k] = evaluation_period[k]; }
    GParam &p = g->params[(size_t)node];
    p.target = lb_node; p.mean = interval_s; p.rt_off = lp.rt_cnt - 1; p.rt_cnt = 1; p.stream_base = (uint64_t)g->cn_rows.size();
    HS_HIP(g, hipSetDevice(g->cfg.device));
    HS_HIP(g, hipMemcpy(const_cast<GParam *>(g->ctl.P) + node, &p, sizeof p, hipMemcpyHostToDevice));
    g->as_member[(size_t)lp.rt_off + (size_t)lp.rt_cnt - 1] = 0;
    g->cn_rows.push_back(row); g->cn_node.push_back(node);
    g->deployer_of[(size_t)lb_node] = node;
    g->reach_s = std::max(g->reach_s, interval_s);
    g->health = true;                          // (the member list is the healthy list of the health lowering)
    return HS_OK;
}

int hs_graph_get_canary_deployer(hs_graph *g, int32_t node, int64_t *state, double *traffic_pct, int32_t *baseline, int32_t *members,
                                 int32_t *weights, int32_t *weight_set, double *service_sum, int64_t *service_count, int64_t *events) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (events) {
        GVars v;
        HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < HS_CANARY_KINDS; ++k) events[k] = v.cn_by_kind[k];
    }
    if (node == -1) return HS_OK;
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_CANARY_DEPLOYER)
        return fail(g, HS_E_INVALID, "get_canary_deployer: node %d is not a CanaryDeployer", node);
    const GParam &np = g->params[(size_t)node];
    size_t r = 0;
    while (r < g->cn_node.size() && g->cn_node[r] != node) ++r;
    if (r == g->cn_node.size()) return fail(g, HS_E_STATE, "get_canary_deployer: CanaryDeployer node %d was never configured", node);
    const GParam &lp = g->params[(size_t)np.target];
    const size_t cap = (size_t)lp.rt_cnt;
    GCn row = g->cn_rows[r];
    GState ls{};
    std::vector<int32_t> all(2 * cap, -1), hl(cap, 0);
    if (g->d_cn) {
        HS_HIP(g, hipMemcpy(&row, g->d_cn + r, sizeof row, hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(&ls, g->ctl.S + np.target, sizeof ls, hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(all.data(), g->d_cn_lists[r], 2 * cap * sizeof(int32_t), hipMemcpyDeviceToHost));
        HS_HIP(g, hipMemcpy(hl.data(), g->ctl.hl_list + lp.rt_off, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
    } else {
        ls.qlen = lp.rt_cnt - 1;
        for (int q = 0; q < ls.qlen; ++q) hl[(size_t)q] = q;
    }
    if (state) {
        const int64_t out[HS_CANARY_FIELDS] = {row.started, row.completed, row.rolled_back, row.stages_completed, row.ev_performed, row.ev_passed, row.ev_failed,
                                               row.status, row.cur_stage, row.total_stages, row.has_canary, row.has_start ? row.stage_start : -1,
                                               row.n_base, ls.qlen, row.has_start, 0};
        std::copy(out, out + HS_CANARY_FIELDS, state);
    }
    if (traffic_pct) *traffic_pct = row.cur_pct;
    if (baseline) { std::fill(baseline, baseline + cap, -1); std::copy(all.begin(), all.begin() + row.n_base, baseline); }
    if (members) { std::fill(members, members + cap, -1); std::copy(hl.begin(), hl.begin() + ls.qlen, members); }
    if (weight_set) for (size_t q = 0; q < cap; ++q) weight_set[q] = all[cap + q] > 0 ? 1 : 0;
    if (weights) {
        if (g->d_cn) HS_HIP(g, hipMemcpy(weights, g->ctl.lb_w + lp.rt_off, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
        else std::copy(g->lb_w.begin() + lp.rt_off, g->lb_w.begin() + lp.rt_off + lp.rt_cnt, weights);
    }
    std::vector<int32_t> tg(cap, 0);
    if ((service_sum || service_count) && cap) HS_HIP(g, hipMemcpy(tg.data(), g->d_rt_targets + lp.rt_off, cap * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < cap && (service_sum || service_count); ++q) {
        const int be = tg[q];
        double sum = 0.0; long long cnt = 0;
        if (g->d_svc_sum) {
            HS_HIP(g, hipMemcpy(&sum, g->d_svc_sum + be, sizeof sum, hipMemcpyDeviceToHost));
            HS_HIP(g, hipMemcpy(&cnt, g->d_svc_cnt + be, sizeof cnt, hipMemcpyDeviceToHost));
        }
        if (service_sum) service_sum[q] = sum;
        if (service_count) service_count[q] = cnt;
    }
    return HS_OK;
}

int hs_debug_compact_members(int32_t device, int32_t n_slots, int32_t len, int32_t *list, const uint8_t *member, int32_t wave, int32_t *out_len) {
    if (n_slots < 0 || len < 0 || len > n_slots || !out_len || (len > 0 && (!list || !member))) return HS_E_INVALID;
    for (int q = 0; q < len; ++q) if (list[q] < 0 || list[q] >= n_slots) return HS_E_INVALID;
    *out_len = 0;
    if (len == 0) return HS_OK;
    if (hipSetDevice(device) != hipSuccess) return HS_E_HIP;
    int32_t *d_list = nullptr, *d_len = nullptr;
    uint8_t *d_mem = nullptr;
    int rc = HS_OK;
    if (hipMalloc(&d_list, (size_t)len * sizeof(int32_t)) != hipSuccess || hipMalloc(&d_mem, (size_t)n_slots) != hipSuccess ||
        hipMalloc(&d_len, sizeof(int32_t)) != hipSuccess) rc = HS_E_HIP;
    if (rc == HS_OK && (hipMemcpy(d_list, list, (size_t)len * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
                        hipMemcpy(d_mem, member, (size_t)n_slots, hipMemcpyHostToDevice) != hipSuccess)) rc = HS_E_HIP;
    if (rc == HS_OK) {
        hipLaunchKernelGGL(hs::graph::hs_graph_compact_members, dim3(1), dim3(64), 0, nullptr, d_list, d_mem, len, wave ? 1 : 0, d_len);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out_len, d_len, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(list, d_list, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) rc = HS_E_HIP;
    }
    if (d_list) (void)hipFree(d_list);
    if (d_mem) (void)hipFree(d_mem);
    if (d_len) (void)hipFree(d_len);
    return rc;
}

int hs_graph_add_fault(hs_graph *g, int32_t node, int64_t time_ns, int32_t on, int32_t cancelled) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n) return fail(g, HS_E_INVALID, "add_fault: node %d out of range", node);
    if (g->ran || g->launches > 0 || g->d_faults) return fail(g, HS_E_STATE, "add_fault: fault Events are constructed before the first run");
    if (g->faults.size() >= (size_t)1 << 24) return fail(g, HS_E_OVERFLOW, "more than 2^24 fault Events");
    g->faults.push_back(GFault{time_ns, node, (on ? 1u : 0u) | (cancelled ? 2u : 0u), 0.0});
    return HS_OK;
}

int hs_graph_add_link_fault(hs_graph *g, int32_t link_node, int64_t time_ns, int32_t what, int32_t on, double value, int32_t cancelled) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (link_node < 0 || link_node >= g->n || g->params[(size_t)link_node].kind != HS_NODE_LINK)
        return fail(g, HS_E_INVALID, "add_link_fault: node %d is not a NetworkLink", link_node);
    if (g->ran || g->launches > 0 || g->d_faults) return fail(g, HS_E_STATE, "add_link_fault: fault Events are constructed before the first run");
    if (g->faults.size() >= (size_t)1 << 24) return fail(g, HS_E_OVERFLOW, "more than 2^24 fault Events");
    if (what != HS_LINK_FAULT_LATENCY && what != HS_LINK_FAULT_LOSS) return fail(g, HS_E_INVALID, "add_link_fault: what = %d is neither latency nor loss", what);
    if (what == HS_LINK_FAULT_LATENCY && on && !(value >= 0.0 && value < 4.0e9))
        return fail(g, HS_E_UNSUPPORTED, "add_link_fault: an extra latency of %.6g s is not in [0, 4e9)", value);
    if (what == HS_LINK_FAULT_LOSS && !(value >= 0.0 && value <= 1.0))
        return fail(g, HS_E_UNSUPPORTED, "add_link_fault: a packet loss rate of %.6g is not in [0, 1]", value);
    if (what == HS_LINK_FAULT_LATENCY && on) {                 // one step of the link may now be this much longer
        const GParam &p = g->params[(size_t)link_node];
        const double draw = p.sub == HS_LAT_EXPONENTIAL ? hs::kLongestExpDraw * p.mean : p.mean;
        g->reach_s = std::max(g->reach_s, p.lat_min + value + draw);
    }
    g->faults.push_back(GFault{time_ns, link_node, (on ? 1u : 0u) | (cancelled ? 2u : 0u) | ((uint32_t)what << kFaultWhatShift), on || what == HS_LINK_FAULT_LOSS ? value : 0.0});
    g->n_link_faults += 1;
    return HS_OK;
}

int hs_graph_get_link_faults(hs_graph *g, int32_t *active_latency, int32_t *active_loss, int64_t *loss_draws) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    std::vector<GState> S((size_t)g->n);
    HS_HIP(g, hipMemcpy(S.data(), g->ctl.S, (size_t)g->n * sizeof(GState), hipMemcpyDeviceToHost));
    for (int i = 0; i < g->n; ++i) {
        const GState &s = S[(size_t)i];
        const GParam &p = g->params[(size_t)i];
        const bool lnk = p.kind == HS_NODE_LINK, lf = lnk && g->n_link_faults > 0;
        if (active_latency) active_latency[i] = lf ? s.qlen - 1 : -1;
        if (active_loss) active_loss[i] = lf ? s.active - 1 : -1;
        // (without link faults the rate never changes: every Request that entered drew, or none did)
        if (loss_draws) loss_draws[i] = lf ? (int64_t)s.svc_draws : lnk && p.loss > 0.0 ? s.a : 0;
    }
    return HS_OK;
}

int hs_graph_get_faults(hs_graph *g, uint8_t *crashed, int64_t *internal_by_kind, int64_t *cancelled) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    if (crashed) {
        std::vector<GParam> P((size_t)g->n);
        HS_HIP(g, hipMemcpy(P.data(), g->ctl.P, (size_t)g->n * sizeof(GParam), hipMemcpyDeviceToHost));
        for (int i = 0; i < g->n; ++i) crashed[i] = P[(size_t)i].crashed;
    }
    GVars v;
    HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
    if (internal_by_kind) {
        for (int k = 0; k < 4; ++k) internal_by_kind[k] = v.internal_by_kind[k];
        if (g->faults.empty()) {
            // A graph without fault Events: its own loop does not count the internal kinds, the batch loop of a launch it shares with
            // a graph that has some does -- so the device's counts are not taken.  Nothing is ever dropped there: a limiter's Events
            // are exactly the ones its two handlers counted.
            for (int k = 0; k < 4; ++k) internal_by_kind[k] = 0;
            std::vector<GState> S((size_t)g->n);
            HS_HIP(g, hipMemcpy(S.data(), g->ctl.S, (size_t)g->n * sizeof(GState), hipMemcpyDeviceToHost));
            for (int i = 0; i < g->n; ++i)
                if (g->params[(size_t)i].kind == HS_NODE_RATE_LIMITER) { internal_by_kind[0] += S[(size_t)i].a; internal_by_kind[1] += S[(size_t)i].d; }
        }
    }
    if (cancelled) *cancelled = v.faults_cancelled;
    return HS_OK;
}

int hs_graph_schedule(hs_graph *g, int32_t node, int64_t time_ns) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n) return fail(g, HS_E_INVALID, "schedule: node %d out of range", node);
    if (g->params[(size_t)node].kind == HS_NODE_SOURCE)
        return fail(g, HS_E_UNSUPPORTED, "schedule: node %d is a Source (only Requests for a Server, Sink, link or router are lowered)", node);
    g->sched_node.push_back(node);
    g->sched_t.push_back(time_ns);
    g->sched_id.push_back(0);
    return HS_OK;
}

int hs_graph_schedule_client(hs_graph *g, int32_t node, int64_t time_ns, int32_t request_id) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (node < 0 || node >= g->n || g->params[(size_t)node].kind != HS_NODE_CLIENT) return fail(g, HS_E_INVALID, "schedule_client: node %d is not a Client", node);
    if (request_id < 0 || request_id >= (1 << kKeyAttemptShift))
        return fail(g, HS_E_UNSUPPORTED, "schedule_client: request_id %d is not in [0, 2^30) (0: none)", request_id);
    g->sched_node.push_back(node);
    g->sched_t.push_back(time_ns);
    g->sched_id.push_back(request_id);
    g->any_sched_id |= request_id != 0;
    return HS_OK;
}

}  // extern "C"

// Tick tables up to `horizon` (two ticks beyond it, hs_tables.hip); the same prefix whatever the horizon, so a later, longer table
// continues the run that used the shorter one.
static int build_tables(hs_graph *g, int64_t horizon) {
    if (g->rows.empty() || horizon <= g->tick_horizon) return HS_OK;
    const double span_s = (double)(horizon - g->cfg.start_ns) / 1e9;
    int64_t cap = g->tick_cap > 0 ? g->tick_cap : 0;
    for (double r : g->row_rate) {
        const double mean = r * (span_s > 0 ? span_s : 0.0);
        const double want = mean + 10.0 * std::sqrt(mean + 1.0) + 72.0;
        if (want > 4e9) return fail(g, HS_E_INVALID, "a tick table up to %lld ns would need %.3g ticks", (long long)horizon, want);
        if ((int64_t)want > cap) cap = (int64_t)want;
    }
    const long long budget = g->cfg.profile_budget > 0 ? g->cfg.profile_budget : hs::kDefaultLaneBudget;
    for (int attempt = 0; attempt < 8; ++attempt) {
        if ((double)g->rows.size() * (double)cap * 8.0 > 64e9) return fail(g, HS_E_INVALID, "tick tables would need %.1f GB", (double)g->rows.size() * (double)cap * 8.0 / 1e9);
        if (cap != g->tick_cap || !g->d_ticks) {
            if (g->d_ticks) HS_HIP(g, hipFree(g->d_ticks));
            g->d_ticks = nullptr;
            HS_HIP(g, hipMalloc(&g->d_ticks, g->rows.size() * (size_t)cap * sizeof(int64_t)));
            g->tick_cap = cap;
        }
        { const int rc = ensure_stream(g); if (rc) return rc; }
        HS_HIP(g, hs::tick_tables_launch(g->stream, g->d_rows, (int)g->rows.size(), g->cfg.start_ns, horizon, cap, g->d_ticks, g->d_tick_count,
                                          g->d_tick_status, budget, false));
        HS_HIP(g, hipStreamSynchronize(g->stream));
        unsigned long long st[2] = {0ull, 0ull};
        HS_HIP(g, hipMemcpy(st, g->d_tick_status, sizeof st, hipMemcpyDeviceToHost));
        if (st[0] != 0ull)
            return fail(g, HS_E_UNSUPPORTED, "node %lld: one tick of its time-varying Source / Probe needs more than 64 x %lld adaptive-Simpson "
                         "intervals (hs_graph_config.profile_budget raises the limit) -- refused instead of stalling the device",
                         (long long)st[0] - 2, budget);
        if (st[1] == 0ull) {
            g->tick_horizon = horizon;
            g->ctl.ticks = g->d_ticks; g->ctl.tick_cap = cap; g->ctl.tick_count = g->d_tick_count;
            return HS_OK;
        }
        cap *= 2;                                           // (a Poisson stream that ran ahead of its mean: a longer table)
    }
    return fail(g, HS_E_OVERFLOW, "a tick table overflowed after eight doublings");
}

// What a run needs before its first launch: tick tables up to the end, the schedule()d entries on the device.
static int prepare_run(hs_graph *g, int64_t end_ns) {
    GCtl &c = g->ctl;
    g->state_cache_valid = false;
    if (g->n_limiters > 0)
        for (int i = 0; i < g->n; ++i)
            if (g->params[(size_t)i].kind == HS_NODE_RATE_LIMITER && g->lim_policy[(size_t)i].policy == HS_LIMITER_NONE)
                return fail(g, HS_E_STATE, "node %d: a RateLimitedEntity without a policy (hs_graph_set_limiter_policy comes before the run)", i);
    if (g->lim_ring_len > 0 && !c.lim_ring) {              // the SlidingWindowPolicy logs of all such limiters, sized once (every policy is set)
        HS_HIP(g, hipSetDevice(g->cfg.device));
        HS_HIP(g, hipMalloc(&c.lim_ring, (size_t)g->lim_ring_len * sizeof(int64_t)));
    }
    if (!hs::reach_fits_int64(end_ns, g->reach_s))
        return fail(g, HS_E_UNSUPPORTED, "the end (%lld ns) plus one longest step (%.6g s: 36.8 / the smallest rate, 36.8 x the largest "
                     "exponential mean, a constant service, a link's delay, a probe interval or a rate limiter's longest wait) leaves int64 nanoseconds -- refused, "
                     "never wrapped", (long long)end_ns, g->reach_s);
    // table-driven streams: up to this end when it is a real horizon, else (an auto-terminating run) a minute at a time
    int64_t table_h = end_ns;
    if (!g->rows.empty()) {
        const int64_t minute = 60ll * 1000000000ll;
        if (end_ns - g->cfg.start_ns > 64 * minute) table_h = std::max<int64_t>(g->tick_horizon, g->cfg.start_ns + minute);
        const int rc = build_tables(g, table_h);
        if (rc) return rc;
    }
    if (!g->faults.empty() && !g->d_faults) {              // the fault Events: read once, by the launch that boots the heap
        const long long need = (long long)g->n + (long long)g->faults.size() + 16;
        if (c.heap_cap < need) {
            const int rc = grow(g, &c.heap, 0, need);
            if (rc) return rc;
            c.heap_cap = need;
        }
        HS_HIP(g, hipMalloc(&g->d_faults, g->faults.size() * sizeof(GFault)));
        HS_HIP(g, hipMemcpy(g->d_faults, g->faults.data(), g->faults.size() * sizeof(GFault), hipMemcpyHostToDevice));
        const GFault *df = g->d_faults;
        const long long nf = (long long)g->faults.size();
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, faults), &df, sizeof df, hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, n_faults), &nf, sizeof nf, hipMemcpyHostToDevice));
        const long long nlf = g->n_link_faults;
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, n_link_faults), &nlf, sizeof nlf, hipMemcpyHostToDevice));
    }
    if (g->n_checkers > 0 && !g->d_health)
        for (int i = 0; i < g->n; ++i)
            if (g->params[(size_t)i].kind == HS_NODE_HEALTH_CHECKER && !g->checker_set[(size_t)i])
                return fail(g, HS_E_STATE, "node %d: a HealthChecker without its LoadBalancer (hs_graph_set_health_checker comes before the run)", i);
    if (g->n_scalers > 0 && !g->d_as) {
        // the scalers' rows, their history buffers and the membership words, once; the device finds them through GVars
        if ((int)g->as_rows.size() != g->n_scalers)
            return fail(g, HS_E_STATE, "an AutoScaler without its LoadBalancer (hs_graph_set_auto_scaler comes before the run)");
        for (int i = 0; i < g->n; ++i) {
            const GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_LB || g->scaler_of[(size_t)i] < 0) continue;
            for (int q = 0; q < p.rt_cnt; ++q)
                if (!g->hl_flag[(size_t)p.rt_off + (size_t)q])
                    return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: backend %d is marked unhealthy under an AutoScaler (not lowered)", i, q);
        }
        HS_HIP(g, hipSetDevice(g->cfg.device));
        const long long cap0 = g->cfg.record_capacity > 0 && g->cfg.record_capacity < 64 ? g->cfg.record_capacity : 64;
        for (GAs &row : g->as_rows) {
            int64_t *h = nullptr;
            HS_HIP(g, hipMalloc(&h, 4 * (size_t)cap0 * sizeof(int64_t)));
            g->d_as_hist.push_back(h);
            row.hist = h; row.hist_cap = cap0; row.hist_len = 0;
        }
        const size_t nrt = (size_t)(g->n_rt > 0 ? g->n_rt : 1);
        HS_HIP(g, hipMalloc(&g->d_as, g->as_rows.size() * sizeof(GAs)));
        HS_HIP(g, hipMemcpy(g->d_as, g->as_rows.data(), g->as_rows.size() * sizeof(GAs), hipMemcpyHostToDevice));
        HS_HIP(g, hipMalloc(&g->d_as_mem, nrt));
        HS_HIP(g, hipMemcpy(g->d_as_mem, g->as_member.data(), nrt, hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, as), &g->d_as, sizeof g->d_as, hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, as_mem), &g->d_as_mem, sizeof g->d_as_mem, hipMemcpyHostToDevice));
    }
    if (g->n_deployers > 0 && !g->d_rd) {
        // the deployers' rows, their lists and the membership words, once; the device finds them through GVars
        if ((int)g->rd_rows.size() != g->n_deployers)
            return fail(g, HS_E_STATE, "a RollingDeployer without its LoadBalancer (hs_graph_set_rolling_deployer comes before the run)");
        for (int i = 0; i < g->n; ++i) {
            const GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_LB || g->deployer_of[(size_t)i] < 0) continue;
            for (int q = 0; q < p.rt_cnt; ++q)
                if (!g->hl_flag[(size_t)p.rt_off + (size_t)q])
                    return fail(g, HS_E_UNSUPPORTED, "LoadBalancer node %d: backend %d is marked unhealthy under a deployer (not lowered)", i, q);
        }
        HS_HIP(g, hipSetDevice(g->cfg.device));
        for (GRd &row : g->rd_rows) {
            const size_t cap = (size_t)std::max(row.cap, 1);
            int32_t *l = nullptr;
            HS_HIP(g, hipMalloc(&l, 6 * cap * sizeof(int32_t)));
            HS_HIP(g, hipMemset(l, 0xff, 6 * cap * sizeof(int32_t)));
            g->d_rd_lists.push_back(l);
            row.old_b = l; row.new_b = l + cap; row.cur_old = l + 2 * cap; row.cur_new = l + 3 * cap; row.pass = l + 4 * cap; row.readd = l + 5 * cap;
        }
        HS_HIP(g, hipMalloc(&g->d_rd, g->rd_rows.size() * sizeof(GRd)));
        HS_HIP(g, hipMemcpy(g->d_rd, g->rd_rows.data(), g->rd_rows.size() * sizeof(GRd), hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, rd), &g->d_rd, sizeof g->d_rd, hipMemcpyHostToDevice));
        const int n_rd = (int)g->rd_rows.size();
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, n_rd), &n_rd, sizeof n_rd, hipMemcpyHostToDevice));
        if (!g->d_as_mem) {
            const size_t nrt = (size_t)(g->n_rt > 0 ? g->n_rt : 1);
            HS_HIP(g, hipMalloc(&g->d_as_mem, nrt));
            HS_HIP(g, hipMemcpy(g->d_as_mem, g->as_member.data(), nrt, hipMemcpyHostToDevice));
            HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, as_mem), &g->d_as_mem, sizeof g->d_as_mem, hipMemcpyHostToDevice));
        }
    }
    if (g->n_canaries > 0 && !g->d_cn) {
        // the canary deployers' rows, their lists, the Servers' service-time sums and the membership words, once
        if ((int)g->cn_rows.size() != g->n_canaries)
            return fail(g, HS_E_STATE, "a CanaryDeployer without its LoadBalancer (hs_graph_set_canary_deployer comes before the run)");
        HS_HIP(g, hipSetDevice(g->cfg.device));
        for (GCn &row : g->cn_rows) {
            const size_t cap = (size_t)std::max(row.cap, 1);
            int32_t *l = nullptr;
            HS_HIP(g, hipMalloc(&l, 2 * cap * sizeof(int32_t)));
            HS_HIP(g, hipMemset(l, 0xff, 2 * cap * sizeof(int32_t)));
            g->d_cn_lists.push_back(l);
            row.base = l; row.wr = l + cap;
        }
        HS_HIP(g, hipMalloc(&g->d_cn, g->cn_rows.size() * sizeof(GCn)));
        HS_HIP(g, hipMemcpy(g->d_cn, g->cn_rows.data(), g->cn_rows.size() * sizeof(GCn), hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, cn), &g->d_cn, sizeof g->d_cn, hipMemcpyHostToDevice));
        const int n_cn = (int)g->cn_rows.size();
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, n_cn), &n_cn, sizeof n_cn, hipMemcpyHostToDevice));
        HS_HIP(g, hipMalloc(&g->d_svc_sum, (size_t)g->n * sizeof(double)));
        HS_HIP(g, hipMemset(g->d_svc_sum, 0, (size_t)g->n * sizeof(double)));
        HS_HIP(g, hipMalloc(&g->d_svc_cnt, (size_t)g->n * sizeof(long long)));
        HS_HIP(g, hipMemset(g->d_svc_cnt, 0, (size_t)g->n * sizeof(long long)));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, svc_sum), &g->d_svc_sum, sizeof g->d_svc_sum, hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, svc_cnt), &g->d_svc_cnt, sizeof g->d_svc_cnt, hipMemcpyHostToDevice));
        if (!g->d_as_mem) {
            const size_t nrt = (size_t)(g->n_rt > 0 ? g->n_rt : 1);
            HS_HIP(g, hipMalloc(&g->d_as_mem, nrt));
            HS_HIP(g, hipMemcpy(g->d_as_mem, g->as_member.data(), nrt, hipMemcpyHostToDevice));
            HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, as_mem), &g->d_as_mem, sizeof g->d_as_mem, hipMemcpyHostToDevice));
        }
    }
    if (g->health && !g->d_health) {
        // health state, once: flags, healthy lists, current weights and the checkers' per-backend state in one allocation; the
        // LoadBalancers' rows get their healthy count and their two mark counters
        const size_t nrt = (size_t)(g->n_rt > 0 ? g->n_rt : 1);
        const size_t o_cur = 0, o_hc = o_cur + nrt * sizeof(long long), o_list = o_hc + nrt * sizeof(GHc), o_flag = o_list + nrt * sizeof(int32_t);
        std::vector<char> image(o_flag + nrt, 0);
        GHc *hc0 = reinterpret_cast<GHc *>(image.data() + o_hc);
        int32_t *list0 = reinterpret_cast<int32_t *>(image.data() + o_list);
        for (size_t q = 0; q < nrt; ++q) hc0[q].last_passed = -1;
        std::memcpy(image.data() + o_flag, g->hl_flag.data(), nrt);
        HS_HIP(g, hipSetDevice(g->cfg.device));
        HS_HIP(g, hipMalloc((void **)&g->d_health, image.size()));
        for (int i = 0; i < g->n; ++i) {
            const GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_LB) continue;
            int nh = 0;
            for (int q = 0; q < p.rt_cnt; ++q) if (g->hl_flag[(size_t)p.rt_off + (size_t)q] && g->as_member[(size_t)p.rt_off + (size_t)q]) list0[p.rt_off + nh++] = q;
            GState s0{};
            s0.qhead = 0; s0.qtail = 0; s0.qlen = nh;
            HS_HIP(g, hipMemcpy(c.S + i, &s0, sizeof s0, hipMemcpyHostToDevice));
        }
        HS_HIP(g, hipMemcpy(g->d_health, image.data(), image.size(), hipMemcpyHostToDevice));
        c.wrr_cur = reinterpret_cast<long long *>(g->d_health + o_cur);
        c.hc = reinterpret_cast<GHc *>(g->d_health + o_hc);
        c.hl_list = reinterpret_cast<int32_t *>(g->d_health + o_list);
        c.hl_flag = reinterpret_cast<uint8_t *>(g->d_health + o_flag);
        c.health = 1;
    }
    if (g->n_wrappers + g->n_clients > 0 && !c.rs_tab) {
        // the wrappers' in-flight tables, once: one allocation, every wrapper's places in node order
        long long len = 0;
        HS_HIP(g, hipSetDevice(g->cfg.device));
        for (int i = 0; i < g->n; ++i) {
            GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_BULKHEAD && p.kind != HS_NODE_TIMEOUT_WRAPPER && p.kind != HS_NODE_CLIENT) continue;
            if (!g->wrapper_set[(size_t)i])
                return fail(g, HS_E_STATE, p.kind == HS_NODE_CLIENT ? "node %d: a Client without its parameters (hs_graph_set_client comes before the run)"
                            : "node %d: a Bulkhead / TimeoutWrapper without its parameters (hs_graph_set_wrapper comes before the run)", i);
            const long long words = p.kind == HS_NODE_CLIENT ? 2 : 1;                  // a Client's place: key + start time
            if (len + words * g->tab_cap[(size_t)i] > (1ll << 30)) return fail(g, HS_E_UNSUPPORTED, "the wrappers' in-flight tables of this graph exceed 2^30 ids");
            p.rt_off = (int32_t)len; p.rt_cnt = g->tab_cap[(size_t)i];
            len += words * p.rt_cnt;
            HS_HIP(g, hipMemcpy(const_cast<GParam *>(c.P) + i, &p, sizeof p, hipMemcpyHostToDevice));
        }
        HS_HIP(g, hipMalloc(&c.rs_tab, (size_t)len * sizeof(int64_t)));
        HS_HIP(g, hipMemset(c.rs_tab, 0, (size_t)len * sizeof(int64_t)));
        g->rs_tab_len = len;
        if (!g->cl_delays.empty()) {
            HS_HIP(g, hipMalloc(&g->d_cl_delays, g->cl_delays.size() * sizeof(int64_t)));
            HS_HIP(g, hipMemcpy(g->d_cl_delays, g->cl_delays.data(), g->cl_delays.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        c.cl_delays = g->d_cl_delays;
    }
    if (g->n_hedges > 0 && !g->d_hg) {
        // the Hedges' and Fallbacks' rows and tables, once; the device finds them through GVars
        HS_HIP(g, hipSetDevice(g->cfg.device));
        for (int i = 0; i < g->n; ++i) {
            GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_HEDGE && p.kind != HS_NODE_FALLBACK) continue;
            if (!g->wrapper_set[(size_t)i])
                return fail(g, HS_E_STATE, "node %d: a Hedge / Fallback without its parameters (hs_graph_set_hedge / hs_graph_set_fallback comes before the run)", i);
        }
        for (int i = 0; i < g->n; ++i) {
            GParam &p = g->params[(size_t)i];
            if (p.kind != HS_NODE_HEDGE && p.kind != HS_NODE_FALLBACK) continue;
            GHg row{};
            row.cap = g->tab_cap[(size_t)i];
            HS_HIP(g, hipMalloc(&row.tab, (size_t)row.cap * sizeof(GHgEnt)));
            g->hg_rows.push_back(row); g->hg_node.push_back(i);               // (owned from here on: hs_graph_destroy frees it)
            HS_HIP(g, hipMemset(row.tab, 0, (size_t)row.cap * sizeof(GHgEnt)));
            p.rt_off = (int32_t)g->hg_rows.size() - 1; p.rt_cnt = 0;
            HS_HIP(g, hipMemcpy(const_cast<GParam *>(c.P) + i, &p, sizeof p, hipMemcpyHostToDevice));
        }
        HS_HIP(g, hipMalloc(&g->d_hg, g->hg_rows.size() * sizeof(GHg)));
        HS_HIP(g, hipMemcpy(g->d_hg, g->hg_rows.data(), g->hg_rows.size() * sizeof(GHg), hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, hg), &g->d_hg, sizeof g->d_hg, hipMemcpyHostToDevice));
    }
    if (!g->qpol.empty() && !g->d_qp) {
        // the queue policies' rows, once (hs_graph_set_queue_policy comes before the first run): the device finds them through GVars
        HS_HIP(g, hipSetDevice(g->cfg.device));
        HS_HIP(g, hipMalloc(&g->d_qp, g->qpol.size() * sizeof(GQueue)));
        HS_HIP(g, hipMemcpy(g->d_qp, g->qpol.data(), g->qpol.size() * sizeof(GQueue), hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, qp), &g->d_qp, sizeof g->d_qp, hipMemcpyHostToDevice));
    }
    if (g->n_stock > 0)
        for (int i = 0; i < g->n; ++i) {
            const uint8_t k = g->params[(size_t)i].kind;
            if ((k == HS_NODE_POOLED_CYCLE || k == HS_NODE_INVENTORY) && !g->wrapper_set[(size_t)i])
                return fail(g, HS_E_STATE, "node %d: a PooledCycleResource / InventoryBuffer without its parameters (hs_graph_set_pool / hs_graph_set_inventory comes before the run)", i);
        }
    if (g->n_flows > 0)
        for (int i = 0; i < g->n; ++i) {
            const uint8_t k = g->params[(size_t)i].kind;
            if (k >= HS_NODE_BATCH_PROCESSOR && k <= HS_NODE_GATE && !g->wrapper_set[(size_t)i])
                return fail(g, HS_E_STATE, "node %d: a BatchProcessor, ConveyorBelt or GateController without its parameters (hs_graph_set_flow comes before the run)", i);
        }
    const long long ns = (long long)g->sched_node.size();
    if (ns > g->d_sched_cap) {
        if (g->d_sched_node) HS_HIP(g, hipFree(g->d_sched_node));
        if (g->d_sched_t) HS_HIP(g, hipFree(g->d_sched_t));
        g->d_sched_node = nullptr; g->d_sched_t = nullptr;
        g->d_sched_cap = ns + ns / 2 + 16;
        HS_HIP(g, hipMalloc(&g->d_sched_node, (size_t)g->d_sched_cap * sizeof(int32_t)));
        HS_HIP(g, hipMalloc(&g->d_sched_t, (size_t)g->d_sched_cap * sizeof(int64_t)));
    }
    if (ns > 0) {
        HS_HIP(g, hipMemcpy(g->d_sched_node, g->sched_node.data(), (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice));
        HS_HIP(g, hipMemcpy(g->d_sched_t, g->sched_t.data(), (size_t)ns * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    c.sched_id = nullptr;
    if (g->any_sched_id) {                                  // (request ids: only a graph whose Client was handed one has the array)
        if (g->d_sched_id) HS_HIP(g, hipFree(g->d_sched_id));
        g->d_sched_id = nullptr;
        HS_HIP(g, hipMalloc(&g->d_sched_id, (size_t)ns * sizeof(int32_t)));
        HS_HIP(g, hipMemcpy(g->d_sched_id, g->sched_id.data(), (size_t)ns * sizeof(int32_t), hipMemcpyHostToDevice));
        c.sched_id = g->d_sched_id;
    }
    c.sched_node = g->d_sched_node; c.sched_t = g->d_sched_t; c.n_sched = ns;
    c.end_ns = end_ns;
    c.auto_term = end_ns == (1ll << 61);                   // end_time = Infinity: the limiters' polls are daemons (core/simulation.py:306-322)
    c.coop_min = !(g->has_least_loaded || (g->health && g->has_wrr)) || (g->debug_flags & 1) ? 0 : (g->debug_flags & 2) ? 1 : kCoopMinBackends;
    c.coop_reset = 1;                                      // (hs_graph_coop_selects counts the LAST run: zeroed by its first launch)
    if (g->n_deployers + g->n_canaries > 0) {              // where a member list is compacted behind a removal (hs_debug_graph_flags)
        const int rd_min = (g->debug_flags & 1) ? 0 : (g->debug_flags & 2) ? 1 : kCoopMinBackends;
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(c.V) + offsetof(GVars, rd_coop_min), &rd_min, sizeof rd_min, hipMemcpyHostToDevice));
    }
    g->launches = 0;
    return HS_OK;
}

// A TimeoutWrapper's or a Client's table was full: every one of them gets twice the places (a Bulkhead never holds more than
// max_concurrent ids).
// The rows' rt_off / rt_cnt alone are rewritten: the `crashed` byte of a row is the run's.
static int grow_tables(hs_graph *g) {
    GCtl &c = g->ctl;
    std::vector<int64_t> old((size_t)std::max<long long>(g->rs_tab_len, 1)), now;
    HS_HIP(g, hipMemcpy(old.data(), c.rs_tab, (size_t)g->rs_tab_len * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < g->n; ++i) {
        GParam &p = g->params[(size_t)i];
        if (p.kind != HS_NODE_BULKHEAD && p.kind != HS_NODE_TIMEOUT_WRAPPER && p.kind != HS_NODE_CLIENT) continue;
        const long long cnt = p.kind == HS_NODE_BULKHEAD ? p.rt_cnt : 2ll * p.rt_cnt;
        const long long words = p.kind == HS_NODE_CLIENT ? 2 : 1;
        if ((long long)now.size() + words * cnt > (1ll << 30)) return fail(g, HS_E_OVERFLOW, "more than 2^30 request ids in flight at the wrappers");
        const size_t at = now.size();
        now.insert(now.end(), old.begin() + p.rt_off, old.begin() + p.rt_off + words * p.rt_cnt);
        now.resize(at + (size_t)(words * cnt), 0);
        p.rt_off = (int32_t)at; p.rt_cnt = (int32_t)cnt;
        static_assert(offsetof(GParam, rt_cnt) == offsetof(GParam, rt_off) + sizeof(int32_t), "rt_off and rt_cnt are copied together");
        const int32_t pair[2] = {p.rt_off, p.rt_cnt};
        HS_HIP(g, hipMemcpy(reinterpret_cast<char *>(const_cast<GParam *>(c.P) + i) + offsetof(GParam, rt_off), pair, sizeof pair, hipMemcpyHostToDevice));
    }
    int64_t *nt = nullptr;
    HS_HIP(g, hipMalloc(&nt, now.size() * sizeof(int64_t)));
    HS_HIP(g, hipMemcpy(nt, now.data(), now.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    HS_HIP(g, hipFree(c.rs_tab));
    c.rs_tab = nt; g->rs_tab_len = (long long)now.size();
    return HS_OK;
}

// A Hedge's or a Fallback's table would be more than half full with one more entry: every such table gets twice the places, its
// entries at their new homes (ascending ids keep the probe order of the old table, which no lookup depends on).
static int grow_hedge_tables(hs_graph *g) {
    std::vector<GState> S((size_t)g->n);
    HS_HIP(g, hipMemcpy(S.data(), g->ctl.S, (size_t)g->n * sizeof(GState), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < g->hg_rows.size(); ++r) {
        GHg &row = g->hg_rows[r];
        const int node = g->hg_node[r];
        const long long live = S[(size_t)node].qlen;
        if (2 * (live + 1) <= row.cap) continue;
        if (live >= HS_HEDGE_MAX_IN_FLIGHT)
            return fail(g, HS_E_OVERFLOW, "%s node %d: more than %d requests in flight (entries leak behind a crashed or paused target)",
                        g->params[(size_t)node].kind == HS_NODE_HEDGE ? "Hedge" : "Fallback", node, HS_HEDGE_MAX_IN_FLIGHT);
        std::vector<GHgEnt> old((size_t)row.cap);
        HS_HIP(g, hipMemcpy(old.data(), row.tab, old.size() * sizeof(GHgEnt), hipMemcpyDeviceToHost));
        long long nc = row.cap;
        while (2 * (live + 1) > nc) nc *= 2;
        std::vector<GHgEnt> now((size_t)nc, GHgEnt{});
        for (const GHgEnt &en : old) {
            if (en.id == 0) continue;
            long long i = en.id & (nc - 1);
            while (now[(size_t)i].id != 0) i = (i + 1) & (nc - 1);
            now[(size_t)i] = en;
        }
        GHgEnt *nt = nullptr;
        HS_HIP(g, hipMalloc(&nt, now.size() * sizeof(GHgEnt)));
        HS_HIP(g, hipMemcpy(nt, now.data(), now.size() * sizeof(GHgEnt), hipMemcpyHostToDevice));
        HS_HIP(g, hipFree(row.tab));
        row.tab = nt; row.cap = nc;
        HS_HIP(g, hipMemcpy(g->d_hg + r, &row, sizeof row, hipMemcpyHostToDevice));
    }
    return HS_OK;
}

// What a launch left (the device is idle): enlarge what it ran out of; *done = the run reached its end.
static int after_launch_with(hs_graph *g, int status, long long processed, bool *done);
static int after_launch(hs_graph *g, bool *done) {
    GVars v;
    HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
    return after_launch_with(g, v.status, v.processed, done);
}
static int after_launch_with(hs_graph *g, int status, long long processed, bool *done) {
    GCtl &c = g->ctl;
    g->launches++;
    c.coop_reset = 0;
    struct { int status; long long processed; } v{status, processed};
    if (v.status & kBadKind) return fail(g, HS_E_INVALID, "an event of unknown kind reached the loop (internal error)");
    if (g->cfg.max_events > 0 && v.processed > g->cfg.max_events)
    {
        bool fixed_window = false;                         // (the reference's own livelock, README "Admission control": name it)
        for (const auto &q : g->lim_policy) fixed_window |= q.policy == HS_LIMITER_FIXED_WINDOW;
        return fail(g, HS_E_UNSUPPORTED, "the run exceeds max_events = %lld events on the single-heap path (one lane, ~2.4 us per event); "
                     "raise max_events, or bring the graph into the shape the station engines take%s", (long long)g->cfg.max_events,
                     fixed_window ? "; likely cause in this graph: a FixedWindowPolicy whose window_size is no exact binary fraction of a "
                                    "second (0.1, 0.3, 1/3 ...) can reschedule its poll for the same nanosecond for ever, as the "
                                    "reference does -- use a window such as 0.125, 0.25 or 0.5" : "");
    }
    if (v.status & kGrowHeap) {
        const long long nc = c.heap_cap * 2;
        int rc = grow(g, &c.heap, c.heap_cap, nc); if (rc) return rc;
        c.heap_cap = nc;
    }
    if (v.status & kGrowReq) {
        if (c.req_cap >= (1 << 30)) return fail(g, HS_E_OVERFLOW, "more than 2^30 Requests alive at once");
        const int nc = c.req_cap * 2;
        int rc = grow(g, &c.reqs, c.req_cap, nc); if (rc) return rc;
        c.req_cap = nc;
    }
    if (v.status & kGrowTicks) {
        // a table-driven stream reached the end of its table: twice the span (never beyond the end the caller asked for + the two
        // ticks every table holds beyond its horizon)
        const int64_t span = g->tick_horizon - g->cfg.start_ns;
        int64_t nh = g->cfg.start_ns + (span > 0 ? 2 * span : 1000000000ll);
        if (nh <= g->tick_horizon) return fail(g, HS_E_OVERFLOW, "the tick tables cannot grow any further");
        const int rc = build_tables(g, nh);
        if (rc) return rc;
    }
    if (v.status & kGrowRec) {
        const long long nc = c.rec_cap * 2;
        int rc;
        if ((rc = grow(g, &c.rec_node, c.rec_cap, nc))) return rc;
        if ((rc = grow(g, &c.rec_t, c.rec_cap, nc))) return rc;
        if ((rc = grow(g, &c.rec_cr, c.rec_cap, nc))) return rc;
        c.rec_cap = nc;
    }
    if ((v.status & kGrowTab) && g->ctl.rs_tab) {
        const int rc = grow_tables(g);
        if (rc) return rc;
    }
    if ((v.status & kGrowTab) && g->d_hg) {
        const int rc = grow_hedge_tables(g);
        if (rc) return rc;
    }
    if ((v.status & kPoolOut) && g->d_rd) {
        std::vector<GRd> rows(g->rd_rows.size());
        HS_HIP(g, hipMemcpy(rows.data(), g->d_rd, rows.size() * sizeof(GRd), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < rows.size(); ++r)
            if (rows[r].wanted)
                return fail(g, HS_E_OVERFLOW, "RollingDeployer node %d needs instance %d, beyond its pool of %d instances (the pool's bound did not hold)",
                            g->rd_node[r], rows[r].wanted, g->params[(size_t)g->rd_node[r]].rt_cnt);
    }
    if (v.status & kPoolOut) {
        std::vector<GAs> rows(g->as_rows.size());
        HS_HIP(g, hipMemcpy(rows.data(), g->d_as, rows.size() * sizeof(GAs), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < rows.size(); ++r)
            if (rows[r].wanted)
                return fail(g, HS_E_OVERFLOW, "AutoScaler node %d needs instance %d, beyond its pool of %d instances (the pool's bound did not hold)",
                            g->as_node[r], rows[r].wanted, g->params[(size_t)g->as_node[r]].rt_cnt);
        return fail(g, HS_E_OVERFLOW, "an AutoScaler needs an instance beyond its pool");
    }
    if (v.status & kGrowHist) {
        // a scaling history was full: every full one gets twice the records
        std::vector<GAs> rows(g->as_rows.size());
        HS_HIP(g, hipMemcpy(rows.data(), g->d_as, rows.size() * sizeof(GAs), hipMemcpyDeviceToHost));
        for (size_t r = 0; r < rows.size(); ++r) {
            if (rows[r].hist_len < rows[r].hist_cap) continue;
            const long long nc = rows[r].hist_cap * 2;
            int64_t *h = nullptr;
            HS_HIP(g, hipMalloc(&h, 4 * (size_t)nc * sizeof(int64_t)));
            HS_HIP(g, hipMemcpy(h, rows[r].hist, 4 * (size_t)rows[r].hist_len * sizeof(int64_t), hipMemcpyDeviceToDevice));
            HS_HIP(g, hipFree(rows[r].hist));
            g->d_as_hist[r] = h;
            rows[r].hist = h; rows[r].hist_cap = nc;
            HS_HIP(g, hipMemcpy(g->d_as + r, &rows[r], sizeof(GAs), hipMemcpyHostToDevice));
        }
    }
    if (v.status & kUndecided) { g->undecided = true; *done = true; return HS_OK; }
    *done = v.status == kDone;
    return HS_OK;
}

extern "C" {

int hs_graph_run_until(hs_graph *g, int64_t end_ns) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    {
        const int rc = prepare_run(g, end_ns);
        if (rc) return rc;
    }
    { const int rc = ensure_stream(g); if (rc) return rc; }
    HS_HIP(g, hipEventRecord(g->ev_a, g->stream));
    for (bool done = false; !done;) {
        launch_lone(g->last_level = level_of(g), g->stream, g->ctl);
        HS_HIP(g, hipGetLastError());
        HS_HIP(g, hipStreamSynchronize(g->stream));
        const int rc = after_launch(g, &done);
        if (rc) return rc;
    }
    HS_HIP(g, hipEventRecord(g->ev_b, g->stream));
    HS_HIP(g, hipStreamSynchronize(g->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g->ev_a, g->ev_b) == hipSuccess) g->last_run_ms = ms;
    g->ran = true;
    return HS_OK;
}

static int run_batch(hs_graph *const *gs, int32_t n, int64_t end_ns, int part) {
    if (!gs || n < 1) return fail(nullptr, HS_E_INVALID, "no handles");
    for (int i = 0; i < n; ++i) {
        if (!gs[i]) return fail(nullptr, HS_E_INVALID, "handle %d is null", i);
        if (gs[i]->cfg.device != gs[0]->cfg.device) return fail(gs[i], HS_E_INVALID, "handle %d lives on another device", i);
    }
    {   // (a handle listed twice would run on one heap from two workgroups)
        std::vector<hs_graph *> sorted(gs, gs + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(gs[0], HS_E_INVALID, "a handle is listed twice");
    }
    hs_graph *g0 = gs[0];
    HS_HIP(g0, hipSetDevice(g0->cfg.device));
    { const int rc = ensure_stream(g0); if (rc) return rc; }
    for (int i = 0; i < n; ++i) {
        const int rc = prepare_run(gs[i], end_ns);
        if (rc) { if (gs[i] != g0) fail(g0, rc, "graph %d: %s", i, gs[i]->error.c_str()); return rc; }
    }
    GCtl *d_ctl = nullptr;
    HS_HIP(g0, hipMalloc(&d_ctl, (size_t)n * (sizeof(GCtl) + kBatchStat * sizeof(long long))));
    long long *d_stat = reinterpret_cast<long long *>(d_ctl + n);
    std::vector<long long> h_stat;
    std::vector<int> pending((size_t)n);
    for (int i = 0; i < n; ++i) pending[(size_t)i] = i;
    std::vector<GCtl> h_ctl;
    int rc = HS_OK;
    hipError_t he = hipEventRecord(g0->ev_a, g0->stream);
    while (he == hipSuccess && rc == HS_OK && !pending.empty()) {
        h_ctl.clear();
        for (int i : pending) {
            h_ctl.push_back(gs[i]->ctl);
            h_ctl.back().part = part;              // (the handles themselves never keep part semantics: no early return can leave it set)
        }
        if ((he = hipMemcpy(d_ctl, h_ctl.data(), h_ctl.size() * sizeof(GCtl), hipMemcpyHostToDevice)) != hipSuccess) break;
        int level = kLvPlain;                      // (the highest any pending handle needs: the others compute the same either way)
        for (int i : pending) level = std::max(level, level_of(gs[i]));
        for (int i : pending) gs[i]->last_level = level;
        launch_batch(level, (unsigned)pending.size(), g0->stream, d_ctl, d_stat);
        if ((he = hipGetLastError()) != hipSuccess) break;
        if ((he = hipStreamSynchronize(g0->stream)) != hipSuccess) break;
        h_stat.resize((size_t)kBatchStat * pending.size());
        if ((he = hipMemcpy(h_stat.data(), d_stat, h_stat.size() * sizeof(long long), hipMemcpyDeviceToHost)) != hipSuccess) break;
        std::vector<int> left;
        size_t slot = 0;
        for (int i : pending) {
            bool done = false;
            const long long *st = &h_stat[(size_t)kBatchStat * slot++];
            rc = after_launch_with(gs[i], (int)st[0], st[1], &done);
            gs[i]->pending_events = st[2]; gs[i]->earliest_ns = st[3];
            if (rc) { if (gs[i] != g0) fail(g0, rc, "graph %d: %s", i, gs[i]->error.c_str()); break; }
            if (done) gs[i]->ran = true; else left.push_back(i);
        }
        pending.swap(left);
    }
    if (he == hipSuccess && rc == HS_OK) {
        he = hipEventRecord(g0->ev_b, g0->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(g0->stream);
        float ms = 0.f;
        if (he == hipSuccess && hipEventElapsedTime(&ms, g0->ev_a, g0->ev_b) == hipSuccess)
            for (int i = 0; i < n; ++i) gs[i]->last_run_ms = ms;          // (the batch's wall time: the heaps ran side by side)
    }
    (void)hipFree(d_ctl);
    if (rc) return rc;
    if (he != hipSuccess) return fail(g0, HS_E_HIP, "batch launch: %s", hipGetErrorString(he));
    return HS_OK;
}

int hs_graph_run_many(hs_graph *const *gs, int32_t n, int64_t end_ns) { return run_batch(gs, n, end_ns, 0); }

int hs_graph_level(const hs_graph *g, int which) {
    if (!g || (which != 0 && which != 1)) return -1;
    return which == 0 ? level_of(g) : g->last_level;
}

int hs_graph_run_parts(hs_graph *const *gs, int32_t n, int64_t end_ns) {
    {
        const int rc = run_batch(gs, n, end_ns, 1);
        if (rc) return rc;
    }
    hs_graph *g0 = gs[0];
    for (int i = 0; i < n; ++i) if (gs[i]->undecided) return 1;
    // every part stands in front of its first event beyond end_ns: the reference processes the earliest of them (its loop tests the
    // PREVIOUS event's time, core/simulation.py:472) and nothing else
    // A cancelled `_BatchTimeout` in front of that event is popped and counted like any cancelled Event (core/simulation.py:326-329):
    // the part that holds the earliest entry pops it, and the election is repeated with that part's next entry.
    for (int round = 0; round < (1 << 16); ++round) {
    int best = -1; int64_t best_t = 0; bool tie = false;
    for (int i = 0; i < n; ++i) {
        if (gs[i]->pending_events <= 0) continue;
        const int64_t t = gs[i]->earliest_ns;
        if (best < 0 || t < best_t) { best = i; best_t = t; tie = false; }
        else if (t == best_t) tie = true;              // (two parts' events on one nanosecond: their order is the whole Simulation's)
    }
    if (tie) return 1;
    if (best < 0) return HS_OK;
    hs_graph *g = gs[best];
    {
        const int rc = ensure_stream(g);
        if (rc) { fail(g0, rc, "%s", g->error.c_str()); return rc; }
    }
    GCtl one = g->ctl;
    one.part = 2; one.budget = 1; one.end_ns = INT64_MAX;
    GVars before;
    HS_HIP(g0, hipMemcpy(&before, g->ctl.V, sizeof before, hipMemcpyDeviceToHost));
    bool again = false;
    for (int attempt = 0; attempt < 64 && !again; ++attempt) {
        one.heap = g->ctl.heap; one.heap_cap = g->ctl.heap_cap; one.reqs = g->ctl.reqs; one.req_cap = g->ctl.req_cap;
        one.rec_node = g->ctl.rec_node; one.rec_t = g->ctl.rec_t; one.rec_cr = g->ctl.rec_cr; one.rec_cap = g->ctl.rec_cap;
        one.ticks = g->ctl.ticks; one.tick_cap = g->ctl.tick_cap; one.tick_count = g->ctl.tick_count; one.rs_tab = g->ctl.rs_tab;
        launch_lone(g->last_level = level_of(g), g->stream, one);
        HS_HIP(g0, hipGetLastError());
        HS_HIP(g0, hipStreamSynchronize(g->stream));
        bool done = false;
        const int rc = after_launch(g, &done);       // (enlarges what the one event needed)
        if (rc) { if (g != g0) fail(g0, rc, "%s", g->error.c_str()); return rc; }
        if (g->undecided) return 1;                  // (the popped event was dropped: the handle's state is no answer any more)
        GVars now;
        HS_HIP(g0, hipMemcpy(&now, g->ctl.V, sizeof now, hipMemcpyDeviceToHost));
        if (now.processed > before.processed) return HS_OK;
        if (now.flow_cancelled > before.flow_cancelled) {
            // a cancelled entry stood in front: this part's next entry (the launch wrote the heap's head back) joins the election
            g->pending_events = now.heap_len;
            if (now.heap_len > 0) {
                GEvent top;
                HS_HIP(g0, hipMemcpy(&top, g->ctl.heap, sizeof top, hipMemcpyDeviceToHost));
                g->earliest_ns = top.t;
            }
            again = true;
        } else if (now.heap_len <= 0) return HS_OK;
    }
    if (!again) return fail(g0, HS_E_OVERFLOW, "the event beyond the end could not be processed");
    }
    return 1;                                        // (tens of thousands of cancelled entries in front of the end: the one heap decides)
}

int hs_graph_get_summary(hs_graph *g, hs_summary *out) {
    if (!g || !out) return fail(g, HS_E_INVALID, "null argument");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    GVars v;
    HS_HIP(g, hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost));
    std::memset(out, 0, sizeof *out);
    out->events_processed = v.processed;
    for (int k = 0; k < HS_EV_KINDS; ++k) out->events_by_kind[k] = v.by_kind[k];
    out->final_time_ns = v.cur;
    out->requests_completed = v.completed;
    out->sink_records = v.received;
    out->last_run_ms = g->last_run_ms;
    out->kernel_ms = g->last_run_ms;
    out->launches = g->launches;
    return HS_OK;
}

int hs_graph_get_stats(hs_graph *g, hs_graph_stats *o) {
    if (!g || !o) return fail(g, HS_E_INVALID, "null argument");
    HS_HIP(g, hipSetDevice(g->cfg.device));
    std::vector<GState> S((size_t)g->n);
    HS_HIP(g, hipMemcpy(S.data(), g->ctl.S, (size_t)g->n * sizeof(GState), hipMemcpyDeviceToHost));
    for (int i = 0; i < g->n; ++i) {
        const GState &s = S[(size_t)i];
        const int k = g->params[(size_t)i].kind;
        const bool src = k == HS_NODE_SOURCE, srv = k == HS_NODE_SERVER, lnk = k == HS_NODE_LINK;
        if (o->generated) o->generated[i] = src ? s.c : 0;
        if (o->payloads) o->payloads[i] = src ? s.d : 0;
        if (o->accepted) o->accepted[i] = srv ? s.a : 0;
        if (o->dropped) o->dropped[i] = srv ? s.b : 0;
        if (o->completed) o->completed[i] = srv ? s.c : 0;
        if (o->rejected) o->rejected[i] = srv ? s.d : 0;
        if (o->total_service_s) o->total_service_s[i] = srv ? s.total_service : 0.0;
        if (o->queue_depth) o->queue_depth[i] = srv ? s.qlen : 0;
        if (o->active) o->active[i] = srv ? s.active : 0;
        if (o->received) o->received[i] = k == HS_NODE_SINK ? s.a : 0;
        if (o->entered) o->entered[i] = lnk ? s.a : 0;
        if (o->packets_sent) o->packets_sent[i] = lnk ? s.b : 0;
        if (o->packets_dropped) o->packets_dropped[i] = lnk ? s.c : 0;
        if (o->routed) o->routed[i] = k == HS_NODE_ROUTER ? s.a : 0;
        if (o->lb) {
            const bool lb = k == HS_NODE_LB;
            int64_t *r = o->lb + 6 * (size_t)i;
            r[0] = lb ? s.a : 0; r[1] = lb ? s.b : 0; r[2] = lb ? s.c : 0; r[3] = lb ? s.c : 0; r[4] = lb ? s.d : 0;
            r[5] = lb ? (int64_t)s.svc_draws : 0;
        }
    }
    if (o->rt_taken && g->n_rt > 0)
        HS_HIP(g, hipMemcpy(o->rt_taken, g->ctl.rt_taken, (size_t)g->n_rt * sizeof(int64_t), hipMemcpyDeviceToHost));
    return HS_OK;
}

int64_t hs_graph_read_records(hs_graph *g, int32_t *node, int64_t *t_ns, int64_t *created_ns, int64_t cap) {
    if (!g) return fail(g, HS_E_INVALID, "null handle");
    if (hipSetDevice(g->cfg.device) != hipSuccess) return fail(g, HS_E_HIP, "hipSetDevice failed");
    GVars v;
    if (hipMemcpy(&v, g->ctl.V, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return fail(g, HS_E_HIP, "reading the run's scalars failed");
    const long long m = std::min<long long>(v.rec_n, cap > 0 ? cap : 0);
    if (m > 0) {
        if (node && hipMemcpy(node, g->ctl.rec_node, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return fail(g, HS_E_HIP, "record copy failed");
        if (t_ns && hipMemcpy(t_ns, g->ctl.rec_t, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return fail(g, HS_E_HIP, "record copy failed");
        if (created_ns && hipMemcpy(created_ns, g->ctl.rec_cr, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return fail(g, HS_E_HIP, "record copy failed");
    }
    return v.rec_n;
}

}  // extern "C"
