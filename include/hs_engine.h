/* hs_engine.h -- C ABI of the MI355X discrete-event engine (libhs_hip.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (adamfilli/happy-simulator, pure Python) has no FFI; the seam these entry
 * points replace is `Simulation._execute_until(end_time_ns)` plus
 * `_build_summary()` (happysimulator/core/simulation.py:449-505, :543-591)
 * for the lowered entity set {Source, Server(QueuedResource), Sink}, and the
 * replica / partition fan-out of happysimulator/parallel (runner.py:82-142,
 * simulation.py:164-223).  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions: plain pointers and sizes, caller-owned host buffers (the engine
 * copies; it never frees or retains caller memory), no exceptions or aborts
 * across the ABI.  Every function returns HS_OK (0) or a negative hs_status;
 * hs_last_error() gives the message.  A handle is not thread-safe.  There is
 * NO CPU fallback: if no gfx950 device is present hs_engine_create() fails.
 */
#ifndef HS_ENGINE_H
#define HS_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HS_ABI_VERSION 16

typedef enum hs_status {
    HS_OK = 0,
    HS_E_INVALID = -1,      /* bad argument / configuration (the reference raises ValueError) */
    HS_E_NO_DEVICE = -2,    /* no HIP device: the product path has no CPU fallback */
    HS_E_HIP = -3,          /* HIP runtime error */
    HS_E_UNSUPPORTED = -4,  /* entity / topology not lowered by this engine (never silent) */
    HS_E_OVERFLOW = -5,     /* a per-LP record log overflowed its capacity; re-create with a larger one */
    HS_E_STATE = -6         /* call order violation */
} hs_status;

/* How `Simulation`s map onto logical processes (LPs).
 * SINGLE:   all LPs belong to ONE Simulation (one heap): exactly one event beyond
 *           end_time is processed in total (core/simulation.py:472), the globally first.
 * REPLICAS: every LP is its own Simulation (ParallelRunner, parallel/runner.py:73-79, or
 *           ParallelSimulation without links, parallel/simulation.py:170-195): each LP
 *           processes its own first event beyond end_time. */
typedef enum hs_mode { HS_MODE_SINGLE = 0, HS_MODE_REPLICAS = 1 } hs_mode;

/* load/source.py:182-268 factories */
typedef enum hs_source_kind { HS_SRC_NONE = 0, HS_SRC_POISSON = 1, HS_SRC_CONSTANT = 2 } hs_source_kind;
/* distributions/{exponential,constant}.py */
typedef enum hs_latency_kind {
    HS_LAT_EXPONENTIAL = 0,
    HS_LAT_CONSTANT = 1,
    HS_LAT_NO_SERVER = 2   /* svc_kind only: the LP has no Server, its Source feeds the Sink/Counter directly */
} hs_latency_kind;
/* Server(downstream=...): nothing, a Sink-like collector, a NetworkLink to another station's Server
 * (components/network/link.py:114), or a RandomRouter over {the station's Sink, NetworkLinks}
 * (components/random_router.py:9).  LINK and ROUTER need hs_engine_set_network. */
typedef enum hs_egress_kind {
    HS_EGRESS_NONE = 0,
    HS_EGRESS_SINK = 1,
    HS_EGRESS_LINK = 2,
    HS_EGRESS_ROUTER = 3,
    HS_EGRESS_SERVER = 4   /* hs_stations.egress only: another Server (hs_stations.downstream_lp), tandem queues */
} hs_egress_kind;

/* reference-equivalent event kinds counted by the engine */
enum {
    HS_EV_SOURCE = 0,       /* SourceEvent @ Source                         */
    HS_EV_ENQUEUE = 1,      /* Request @ Server (QueuedResource.handle_event) */
    HS_EV_NOTIFY = 2,       /* QUEUE_NOTIFY @ driver                        */
    HS_EV_POLL = 3,         /* QUEUE_POLL @ queue                           */
    HS_EV_DELIVER = 4,      /* QUEUE_DELIVER @ driver                       */
    HS_EV_WORK = 5,         /* Request @ worker (handle_queued_event start) */
    HS_EV_CONTINUATION = 6, /* ProcessContinuation @ worker                 */
    HS_EV_SINK = 7,         /* Request @ Sink                               */
    HS_EV_LINK = 8,         /* Request @ NetworkLink (transit starts)       */
    HS_EV_LINK_CONT = 9,    /* ProcessContinuation @ NetworkLink (transit over) */
    HS_EV_ROUTE = 10,       /* Request @ RandomRouter                       */
    HS_EV_LB = 11,          /* Request @ LoadBalancer (forwarded to the selected backend)        */
    HS_EV_LB_RESP = 12,     /* _lb_response @ LoadBalancer (completion hook of the forwarded Request) */
    HS_EV_PROBE_TICK = 13,  /* SourceEvent @ Probe (instrumentation/probe.py:81-164)                         */
    HS_EV_PROBE = 14,       /* probe_event (daemon) @ the measurement callback                                */
    HS_EV_KINDS = 15
};

typedef struct hs_config {
    uint32_t struct_size;   /* sizeof(hs_config), for ABI evolution */
    int32_t device;         /* HIP device ordinal */
    int32_t n_lp;           /* station LPs resident on this engine (this GPU's shard) */
    int32_t mode;           /* hs_mode */
    int64_t start_ns;       /* Simulation start_time (Instant.Epoch = 0) */
    int64_t horizon_ns;     /* latest end_time that will be passed to hs_engine_run_until: sizes the record logs */
    uint64_t seed;          /* Philox key of the run (per-LP override: hs_stations.seed) */
    uint64_t lp_base;       /* global index of LP 0: default stream_base of LP i is lp_base + i */
    int64_t log_capacity;   /* records per LP in the admission / sink logs; 0 = derive from rate * horizon */
} hs_config;

/* One station LP = [optional Source] -> Server(c, FIFO, capacity) -> [Sink].
 * Struct-of-arrays; every pointer is [n_lp] or NULL for the documented default.
 * Field meanings and defaults follow the reference constructors:
 *   Source.poisson/constant(rate, stop_after)            load/source.py:182-268
 *   Server(concurrency=1, service_time=ConstantLatency(0.01), queue_capacity=None, downstream=None)
 *                                                        components/server/server.py:64-122 */
typedef struct hs_stations {
    const uint8_t *src_kind;           /* hs_source_kind; NULL = HS_SRC_POISSON */
    const double *src_rate;            /* events/s; required when any source exists */
    const int64_t *src_stop_after_ns;  /* < 0 = never; NULL = never */
    const int32_t *concurrency;        /* 1..32; NULL = 1 */
    const uint8_t *svc_kind;           /* hs_latency_kind; NULL = HS_LAT_CONSTANT */
    const double *svc_mean_s;          /* NULL = 0.01 */
    const int64_t *queue_cap;          /* < 0 = unbounded; NULL = unbounded */
    const uint8_t *egress;             /* hs_egress_kind; NULL = HS_EGRESS_SINK */
    const uint64_t *seed;              /* per-LP Philox key (replica i: base_seed + i); NULL = cfg.seed */
    const uint64_t *stream_base;       /* per-LP stream id base; NULL = cfg.lp_base + i */
    /* Time-varying arrival rate (Source.with_profile, load/source.py:271-320; load/profile.py:52-113): the next arrival
     * is found by the reference's own numerical procedure -- adaptive Simpson + bracket search + Brent
     * (load/arrival_time_provider.py:84-144) -- restated on the device (csrc/hs_profile.hpp).  src_rate of such a source
     * is its PEAK rate (used to size the record logs).  NULL = every source has a ConstantRateProfile(src_rate). */
    const uint8_t *src_profile_kind;   /* hs_profile_kind */
    const double *src_profile_params;  /* [n_lp][4]: LINEAR_RAMP {duration_s, start_rate, end_rate, -};
                                          SPIKE {baseline_rate, spike_rate, warmup_s, spike_duration_s} */
    /* Probe(target, metric, interval) attached to the LP's Source / Server / Sink (instrumentation/probe.py:81-164):
     * a daemon Source of its own that samples getattr(target, metric) every `interval` seconds (tick times follow
     * ConstantArrivalTimeProvider over _ProbeProfile: the general numerical path, like the reference).  Each tick is two
     * reference events (SourceEvent@Probe, probe_event).  Up to four probes per LP (probe_metric_more).  NULL = no probes. */
    const uint8_t *probe_metric;       /* hs_probe_metric; 255 = none */
    const double *probe_interval_s;    /* > 0 */
    /* Simulation.schedule(Event(time, "Request", target=<the LP's Server>)) before run() (core/simulation.py:195-206):
     * LP i receives the Requests sched_time_ns[sched_off[i] .. sched_off[i + 1]), ascending per LP and, among equal
     * times, in the order the caller built the Events; context["created_at"] = the Event's own time (core/event.py:176).
     * An Event built before run() precedes every run-time event of the same nanosecond on its LP.  NULL = none. */
    const int64_t *sched_off;          /* [n_lp + 1] */
    const int64_t *sched_time_ns;      /* [sched_off[n_lp]], each >= start_ns */
    /* The order in which the reference CONSTRUCTS its pre-run events -- the first SourceEvent of every Source in
     * `sources=[...]` order, the first tick of every Probe in `probes=[...]` order (Simulation.__init__,
     * core/simulation.py:145-160), then the Events handed to schedule() in the order the caller built them -- fixes their
     * `_sort_index` values 0 .. N_init-1 from the process-wide counter (core/event.py:53-77), while run() numbers its own
     * events from 0 again (core/event_heap.py:48).  In HS_MODE_SINGLE, when probes or scheduled Requests exist, the engine
     * runs the first N_init constructions of the run in the reference's exact heap order (csrc/hs_exact.hpp) so that every
     * same-nanosecond meeting of the two counters is decided as the reference decides it.  All three NULL = LP order /
     * array order. */
    const int32_t *source_order;       /* [number of Sources] LP indices in `sources=` order (also the last key of the election of
                                        * the one event beyond end_time: a pending tick ranks by its own Source's position here) */
    const int32_t *probe_order;        /* [number of LPs with a Probe] LP indices in `probes=` order */
    /* More than one Probe on an LP (Probe.on_many, instrumentation/probe.py:119-164): slots 1 .. 3 (slot 0 = probe_metric /
     * probe_interval_s above); slots are filled from 0.  probe_slot_order[k] = slot of the k-th entry of probe_order (an LP
     * with several probes appears several times there); NULL = every entry is slot 0. */
    const uint8_t *probe_metric_more;  /* [3][n_lp] hs_probe_metric; 255 = none */
    const double *probe_interval_more; /* [3][n_lp] */
    const uint8_t *probe_slot_order;   /* [number of probes] */
    const int64_t *sched_rank;         /* [sched_off[n_lp]], indexed like sched_time_ns: the Event's position among ALL the
                                          Events the caller constructed for schedule(), distinct and >= 0 (an Event that was
                                          cancelled before run() keeps its position -- it consumed a sort index -- but is not
                                          passed to the engine); NULL = array order */
    /* Several Sources feeding one Server (`Source.poisson(rate, target=server)` more than once; load/source.py:142-180 runs per
     * Source): slots 1 .. 3 of the LP (slot 0 = src_kind / src_rate / src_stop_after_ns above); slots are filled from 0.  Each
     * is an entity of its own with its own arrival stream -- stream base (1 << 40) | (stream_base[lp] << 2) | (slot - 1), kind
     * ARRIVAL -- constant or Poisson rate (no profile).  An LP with more than one Source runs on the engines' general path, and
     * the run starts with the prologue (csrc/hs_exact.hpp): the first ticks of an LP's Sources carry consecutive pre-run sort
     * indices, which run-time events of the same nanosecond can overtake.  source_slot_order[k] = slot of the k-th entry of
     * source_order (an LP with several Sources appears several times there); NULL = every entry is slot 0.  Also on networked
     * stations (both network engines and shards).  NULL = one Source per LP at most.
     * The election of the one event beyond end_ns: a pending DEPARTURE of a Server with several Sources ranks by its LP's
     * first-listed Source -- a stand-in for the Source its lineage goes back to.  A station engine (HS_MODE_SINGLE) notices when the
     * election comes down to that key and repeats the run on the single-heap loop (exact, one lane: hs_engine_prologue_path() == 2
     * afterwards).  So does a station NETWORK held by one engine (since the round of ABI 14: runs of up to 4 000 000 events; the
     * single-heap machinery is built on demand for models without pre-run events, and hs_engine_reset returns to the parallel
     * engines); longer runs and shards of a partitioned network detect such an election and refuse it by name (HS_E_UNSUPPORTED). */
    const uint8_t *src_more_kind;      /* [3][n_lp] hs_source_kind; HS_SRC_NONE = none */
    const double *src_more_rate;       /* [3][n_lp] */
    const int64_t *src_more_stop_after_ns; /* [3][n_lp] < 0 = never; NULL = never */
    const uint8_t *source_slot_order;  /* [number of Sources] */
    /* Tandem queues: `Server(..., downstream=<another Server>)` (components/server/server.py:64-122,271-272; the forwarded Event
     * keeps its context, core/entity.py:83-105).  egress[i] == HS_EGRESS_SERVER: every completion of LP i arrives at the Server of
     * LP downstream_lp[i] at the same instant, created_at unchanged.  At most 7 Servers in a row, no cycles, HS_MODE_SINGLE, no
     * hs_engine_set_network.  A Server may have several upstream Servers: up to four merge on the passes, more run on the single-heap
     * loop from the start (hs_engine_tandem_path() == 2).  Tandem queues next to Probes / scheduled Requests / several Sources per
     * Server start on the passes and move to the single heap when a pre-run event shares its nanosecond with another event of its LP
     * (hs_engine_prologue_path).  The engine runs the chain in passes, upstream first (csrc/hs_station.hpp "tandem queues"); results
     * equal the reference's single heap event for event, ties inside a nanosecond included.  NULL = no such Server. */
    const int32_t *downstream_lp;      /* [n_lp] read where egress == HS_EGRESS_SERVER */
} hs_stations;
typedef enum hs_probe_metric {
    HS_PROBE_DEPTH = 0,        /* QueuedResource.depth */
    HS_PROBE_ACTIVE = 1,       /* Server.active_requests */
    HS_PROBE_ACCEPTED = 2,     /* stats_accepted */
    HS_PROBE_DROPPED = 3,      /* stats_dropped */
    HS_PROBE_COMPLETED = 4,    /* Server._requests_completed */
    HS_PROBE_RECEIVED = 5,     /* Sink.events_received */
    HS_PROBE_GENERATED = 6,    /* Source.generated_count */
    HS_PROBE_LIMITER_DEPTH = 7,/* RateLimitedEntity.queue_depth (general graphs only) */
    HS_PROBE_BH_ACTIVE = 8,    /* Bulkhead.active_count (general graphs only, like the three below) */
    HS_PROBE_BH_QUEUE_DEPTH = 9,   /* Bulkhead.queue_depth */
    HS_PROBE_BH_PERMITS = 10,  /* Bulkhead.available_permits */
    HS_PROBE_TW_IN_FLIGHT = 11,/* TimeoutWrapper.in_flight_count */
    HS_PROBE_CL_IN_FLIGHT = 12,/* Client.in_flight_count (general graphs only) */
    HS_PROBE_BP_BUFFER_DEPTH = 13, /* BatchProcessor.buffer_depth (general graphs only) */
    HS_PROBE_CV_IN_TRANSIT = 14,   /* ConveyorBelt.items_in_transit */
    HS_PROBE_GT_QUEUE_DEPTH = 15,  /* GateController.queue_depth */
    HS_PROBE_AS_CURRENT_COUNT = 16,/* AutoScaler.current_count (general graphs only) */
    HS_PROBE_HG_IN_FLIGHT = 17,/* Hedge.in_flight_count (general graphs only) */
    HS_PROBE_PC_AVAILABLE = 18,/* PooledCycleResource.available (general graphs only, like the three below) */
    HS_PROBE_PC_ACTIVE = 19,   /* PooledCycleResource.active */
    HS_PROBE_PC_QUEUED = 20,   /* PooledCycleResource.queued */
    HS_PROBE_IB_STOCK = 21,    /* InventoryBuffer.stock */
    HS_PROBE_NONE = 255
} hs_probe_metric;
typedef enum hs_profile_kind { HS_PROF_CONSTANT = 0, HS_PROF_LINEAR_RAMP = 1, HS_PROF_SPIKE = 2 } hs_profile_kind;

/* Links between stations (the engine-side form of the reference's partition links, parallel/link.py:18-79,
 * and of `NetworkLink(latency=ConstantLatency(lat_min), jitter=ExponentialLatency(jitter_mean) | None,
 * egress=<Server of station dst>)`).  The smallest constant latency over all links is the lookahead W of the
 * conservative time windows; it must be > 0 (the reference enforces min_latency > 0 the same way). */
typedef struct hs_network {
    const uint8_t *egress_kind;      /* [n_lp] hs_egress_kind; replaces hs_stations.egress */
    const int32_t *router_target0;   /* [n_lp] RandomRouter targets in constructor order: -1 = the station's Sink, */
    const int32_t *router_target1;   /* [n_lp]   >= 0 = link index; used when egress_kind == HS_EGRESS_ROUTER */
    const int32_t *link_of;          /* [n_lp] link index when egress_kind == HS_EGRESS_LINK */
    const uint64_t *router_stream_base; /* [n_lp] NULL = the station's stream base */
    int32_t n_links;
    const int32_t *link_dst;         /* [n_links] destination station (its Server) */
    const double *link_lat_min_s;    /* [n_links] ConstantLatency seconds, > 0 */
    const uint8_t *link_jitter_kind; /* [n_links] HS_LAT_EXPONENTIAL: jitter = ExponentialLatency(mean), one draw of the link's stream per
                                      * packet; HS_LAT_CONSTANT: jitter = ConstantLatency(mean), no draw (link.py:195-200); mean 0 = jitter=None */
    const double *link_jitter_mean_s;/* [n_links] */
    const uint64_t *link_stream_base;/* [n_links] NULL = stream base of the source station */
    const int32_t *link_src;         /* [n_links] source station (for the default stream base and validation) */
    int32_t bag_capacity;            /* in-flight messages per destination station; 0 = 16 */
    /* --- one shard of a network partitioned over several engines (one per GPU); 0 / NULL = the whole network ---
     * The engine owns stations [cfg.lp_base, cfg.lp_base + cfg.n_lp) of n_global_lp; link_src / link_dst are then
     * NETWORK-WIDE station indices, the link table holds every link that starts or ends in the shard, and
     * link_gid gives each link its network-wide id.  This is the engine-side form of the reference's
     * SimulationPartition / PartitionLink split (parallel/partition.py:21-38, parallel/link.py:18-79). */
    int32_t n_global_lp;
    const int64_t *link_gid;         /* [n_links] */
    int64_t n_global_links;
    /* NetworkLink(packet_loss_rate) (components/network/link.py:131-138): every request entering the link is lost
     * with this probability (u of the link's LOSS stream < rate, where the reference asks the process-wide
     * `random.random()`); in [0, 1].  NULL = lossless.  NetworkLink(bandwidth_bps) needs no field: the lowered event
     * providers put no payload_size into the metadata, so the transmission time (link.py:209-214) is 0 for any
     * bandwidth and bytes_transmitted stays 0, exactly as in the reference. */
    const double *link_loss_rate;    /* [n_links] */
    /* RandomRouter(targets=[...]) with other than two targets (components/random_router.py:32-45): the route draw picks
     * targets[int(u * len(targets))].  1..4 targets, at most two of them NetworkLinks (-1 = the station's Sink, which may
     * appear several times).  NULL = every router has exactly two targets (router_target0 / router_target1). */
    const uint8_t *router_n_targets; /* [n_lp] */
    const int32_t *router_target2;   /* [n_lp] */
    const int32_t *router_target3;   /* [n_lp] */
    /* Links whose losses are decided by a TABLE instead of a stream (ABI 14): `PartitionLink(packet_loss=p)`
     * (parallel/link.py:31-39) is applied by the reference's coordinator at the exchange with ONE `random.Random(seed)`
     * for the whole run, drawn in exchange order (parallel/coordinator.py:68,203-205) -- a sequence the caller replays
     * over the cross-partition sends of a run (hs_engine_read_send_log) and hands back as one bit per packet
     * (hs_engine_set_link_drops).  link_drop_capacity[l] > 0: link l has a table of that many packets (all zero = nothing
     * is lost until the caller says so); a packet beyond it is HS_E_OVERFLOW.  Such a link must have link_loss_rate 0.
     * NULL = no link has one. */
    const int64_t *link_drop_capacity; /* [n_links] */
} hs_network;

/* Exchange buffers of a shard: device memory owned by the caller (torch tensors on the host side, so that
 * torch.distributed / RCCL can move them).  A row is {count, then 5 x int64 per message}: arrival ns, send ns,
 * created_at ns, (destination station << 32 | link gid), lineage (csrc/hs_netstation.hpp lin_pack).  Replaces the reference's per-partition Python outbox lists
 * (parallel/simulation.py:107,142-151) and `_exchange_events` (parallel/coordinator.py:182-227). */
typedef struct hs_shard {
    int32_t rank, world;
    const int64_t *shard_lo;         /* host, [world + 1]: rank r owns stations [shard_lo[r], shard_lo[r+1]) */
    int64_t *outbox_dev;             /* device int64 [world][1 + 5 * msg_capacity]: row r = messages for rank r */
    int64_t *inbox_dev;              /* device, same shape: row r = messages from rank r (after the all-to-all) */
    int32_t msg_capacity;
    int32_t reserved;
    int64_t window_ns;               /* lookahead W = min over ALL shards of hs_summary.window_ns (caller all-reduces) */
    int64_t *gvt_dev;                /* device int64[2]: window k accumulates this rank's earliest pending work into
                                        [k & 1]; the caller all-reduces (min) it before window k + 1 reads it */
    int64_t *cand_dev;               /* device int64[8]: {valid, t, t_created, station, steps from its group's root, that root's
                                        creation time, construction rank among this shard's entities, kind}: this rank's first
                                        event beyond end_ns; the ranks' candidates compare by (t, t_created, steps, root time,
                                        construction rank) = (time, _sort_index), core/event.py:337-344.  The rank in [6] only
                                        orders entities of ONE shard; across shards the caller derives the network-wide rank from
                                        (station, kind): kind 0 = a departure / message / injected Request (ranks like the
                                        station's first-listed Source), 2 + s = the tick of the station's Source in slot s,
                                        8 + s = the tick of its Probe in slot s (happy_simulator_amd/sharded.py election_rank) */
} hs_shard;

typedef struct hs_net_stats {
    int64_t *routed;                 /* [n_lp]    RandomRouter.stats_routed            components/random_router.py:36 */
    int64_t *link_entered;           /* [n_links] requests that entered the link (Request@Link events) */
    int64_t *link_packets_sent;      /* [n_links] NetworkLink.packets_sent             components/network/link.py:162 */
    int64_t *link_packets_dropped;   /* [n_links] NetworkLink.packets_dropped          components/network/link.py:132 */
} hs_net_stats;

typedef struct hs_summary {
    /* SimulationSummary fields (instrumentation/summary.py:47-87), engine-wide */
    int64_t events_processed;              /* total_events_processed */
    int64_t events_by_kind[HS_EV_KINDS];
    int64_t events_cancelled;              /* always 0 on this path */
    int64_t final_time_ns;                 /* SINGLE: time of the last processed event; REPLICAS: max over LPs */
    int64_t requests_completed;            /* sum of Server._requests_completed */
    int64_t sink_records;                  /* sum of Sink.events_received */
    /* engine telemetry */
    double last_run_ms;                    /* device time of the last hs_engine_run_until (HIP events) */
    double kernel_ms;                      /* device time of the dominant kernel(s) in that call */
    int64_t launches;                      /* kernel launches in the last run (network engine: windows + 1) */
    int64_t window_ns;                     /* network engine: lookahead W; 0 otherwise */
    int32_t overflow;                      /* 1 if a record log overflowed */
    int32_t reserved;
} hs_summary;

/* Per-LP results, SoA out-buffers [n_lp]; any pointer may be NULL. */
typedef struct hs_lp_stats {
    int64_t *generated;        /* Source._generated_count            load/source.py:159 */
    int64_t *accepted;         /* Queue.stats_accepted               components/queue.py:138 */
    int64_t *dropped;          /* Queue.stats_dropped                components/queue.py:128 */
    int64_t *completed;        /* Server._requests_completed         server/server.py:256 */
    int64_t *rejected;         /* Server._requests_rejected          server/server.py:233 */
    double *total_service_s;   /* Server._total_service_time         server/server.py:257 */
    int64_t *sink_received;    /* Sink.events_received               components/common.py:37 */
    int64_t *queue_depth;      /* QueuedResource.depth */
    int32_t *active;           /* Server.active_requests */
    int64_t *events;           /* events processed by this LP (REPLICAS: that replica's total_events_processed) */
    int64_t *final_time_ns;    /* time of the LP's last processed event */
} hs_lp_stats;

typedef struct hs_engine hs_engine;

int hs_abi_version(void);
/* Build identity: the hash of the sources (csrc/, this header, the compiler flags) the library was built from, compiled into the
 * library itself; the host side rebuilds when it differs from the sources next to it (happy_simulator_amd/_native.py). */
const char *hs_build_sources_hash(void);
/* Number of visible HIP devices (0 when there is no GPU). */
int hs_device_count(void);

/* Tandem queues (hs_stations.downstream_lp): which path the engine is on -- 0 no tandem queues, 1 passes of the station kernel
 * (upstream Servers first), 2 the single-heap loop (csrc/hs_exact.hpp): hs_engine_run_until repeats a run there when the passes
 * met a same-nanosecond order between two Servers' events that their lineage key does not decide (lock-step constant arrivals
 * and services, comparisons around the Sources' first ticks), and a Server with more than four upstream Servers starts there. */
int hs_engine_tandem_path(const hs_engine *h);

/* The prologue (csrc/hs_exact.hpp): the reference numbers the events constructed before run() -- the Sources' and Probes' first
 * ticks, Requests injected with Simulation.schedule() -- first and restarts the count for the run's own events
 * (core/simulation.py:77,145-160), so a run-time event can sort BEFORE a pre-run event of its nanosecond.  Engines with Probes,
 * scheduled Requests or several Sources per Server replay that on a single-heap loop -- one lane for the whole engine.  A station
 * engine and (since ABI 12's round) a network engine driven with hs_engine_run_until skip it at first and repeat the run behind it
 * only if a pre-run event shared its nanosecond with another event of its LP (an arriving message counts), or the run was shorter
 * than the pre-run events are many; shards of a partitioned network (hs_engine_shard_*) keep it.  0: the engine has no prologue,
 * 1: skipped so far, 2: it runs (debug flag 1 << 16 makes it run always). */
int hs_engine_prologue_path(const hs_engine *h);

/* Windows over a station NETWORK (ABI 14): `Simulation.control.run_until / _run_window` (core/simulation.py:527-541) call
 * `_execute_until` again with a later end, and the reference continues from its heap -- O(window).  What the last hs_engine_run_until on a
 * network engine did: 0 the first run since the reset, 1 it CONTINUED from the state the run before it left (every station's rows, the
 * messages in flight, the links' lower bounds, and the timestamp group the election of the one event beyond the earlier end stopped
 * inside -- finished first, csrc/hs_kernels.hpp hs_net_resume), 2 nothing moved (the end is not beyond the event the earlier run
 * already processed: the reference's loop condition `current_time <= end` is false), 3 the run was REPEATED from the start to the
 * new end (an engine whose prologue -- Probes, scheduled Requests, several Sources per Server -- still holds the single-lane heap at
 * the window end, a state the asynchronous kernel cannot take back, debug flag 1 << 24): exact as well, at the cost of the prefix.
 * Diagnostics only; results are identical. */
int hs_engine_window_path(const hs_engine *h);

/* Which kernels the last hs_engine_run_until ran (everything since it started, the repetitions hs_engine_synchronize makes
 * included), as HS_RUN_* bits; bits 16..23 hold the lanes per LP of the wide kernel or the LPs per workgroup of the wavefront-per-LP
 * kernel.  HS_RUN_F64_TIMES: the engine keeps whole nanoseconds as binary64 on its uniform paths (start >= 0, horizon < 2^51,
 * rates > 1e-3, means < 1e4).  Read-only, for tests that must know which side of a host-side gate a configuration landed on. */
#define HS_RUN_ONE_LANE        (1 << 0)    /* hs_station_run, one lane per LP, general entity kinds */
#define HS_RUN_ONE_LANE_UNI    (1 << 1)    /* hs_station_run, uniform entity kinds (binary64 times) */
#define HS_RUN_WIDE            (1 << 2)    /* hs_station_wide<K>, K lanes per LP */
#define HS_RUN_WAVE            (1 << 3)    /* hs_station_wave<NW>, one wavefront per LP */
#define HS_RUN_TANDEM          (1 << 4)    /* passes of the station kernel, upstream Servers first */
#define HS_RUN_SINGLE_HEAP     (1 << 5)    /* the single-heap loop held the whole run (csrc/hs_exact.hpp) */
#define HS_RUN_F64_TIMES       (1 << 6)
#define HS_RUN_NET_ASYNC       (1 << 7)    /* hs_net_async, one cooperative launch */
#define HS_RUN_NET_ASYNC_UNI   (1 << 8)    /* ... its uniform-kind instantiation */
#define HS_RUN_NET_WINDOWED    (1 << 9)    /* conservative windows of hs_net_window */
#define HS_RUN_NET_SEGMENTED   (1 << 10)   /* segments of hs_net_async taking turns */
int hs_engine_run_path(const hs_engine *h);

int hs_engine_create(const hs_config *cfg, hs_engine **out);
int hs_engine_set_stations(hs_engine *h, const hs_stations *st);
/* Optional, after hs_engine_set_stations and before the first run: connect stations with links / routers.
 * Requires HS_MODE_SINGLE.  The engine then advances in conservative windows of W = min link latency; one
 * hs_engine_run_until per hs_engine_reset (windows are internal, the call is not re-entrant). */
int hs_engine_set_network(hs_engine *h, const hs_network *net);
int hs_engine_get_net_stats(hs_engine *h, const hs_net_stats *out);
/* Table-decided link losses (hs_network.link_drop_capacity; replaces the `self._rng.random() < link.packet_loss` of
 * parallel/coordinator.py:203-205).  hs_engine_set_link_drops: packet number e of `link` (a local link index) is lost iff
 * bit e of `bits` is set (n_bits <= the link's capacity; the rest stays 0); takes effect at the next reset / run.
 * hs_engine_read_send_log: every packet that entered a table-decided link since the last reset, as int64 triples
 * {send time ns, network-wide link id, packet number}, in no particular order; returns their number (the first
 * `capacity` are written) or a negative hs_status. */
int hs_engine_set_link_drops(hs_engine *h, int32_t link, const uint32_t *bits, int64_t n_bits);
int64_t hs_engine_read_send_log(hs_engine *h, int64_t *out_triples, int64_t capacity);
/* external != 0: run on the caller's HIP stream (e.g. torch's current stream, so that collectives and engine
 * launches are ordered by the stream; a NULL handle is the device's default stream).  external == 0: back to the
 * engine's own stream. */
int hs_engine_set_stream(hs_engine *h, void *hip_stream, int external);
/* Sharded network = WindowedCoordinator.run (parallel/coordinator.py:75-172) with one partition per GPU and
 * GVT-driven windows.  After create / set_stations / set_network(n_global_lp > 0) / shard_attach, per run:
 *   shard_begin(end);
 *   for k = 0, 1, 2, ...:  shard_window(k)            EXECUTE: window end = min(end, max(prev+1, GVT) + W - 1)
 *                          all-to-all outbox -> inbox   EXCHANGE (caller: RCCL)
 *                          shard_inject(k)
 *                          all-reduce(min) gvt_dev[k&1] GVT     (caller: RCCL)
 *      until shard_progress(k) reports a window end == end;
 *   shard_final(k+1); all-gather cand_dev; shard_overshoot(station - lp_base) on the rank that owns the minimum.
 * All calls except shard_progress only enqueue work on the engine's stream. */
int hs_engine_shard_attach(hs_engine *h, const hs_shard *sh);
/* LIVE exchange (ABI 14): the EXCHANGE step of parallel/coordinator.py:182-227 without a launch boundary.  Every rank runs ONE
 * launch of the asynchronous engine for the whole run; a station whose link leaves the shard appends to the link's queue in the
 * DESTINATION rank's memory and publishes the link's lower bound there (system-scope stores over hipIpcOpenMemHandle mappings:
 * peer-to-peer over xGMI between GPUs, plain device memory when ranks share a device), the receiver polls its own memory.  A shard
 * engine's link queues are uncached, exportable device memory for this.  Per process:
 *   live_export -> all-gather the 3 handles per rank -> live_attach(all handles, peer_link)        (once)
 *   per run: shard_begin(end); <barrier of the caller's: every rank has reset>; live_run(); live_wait();
 *            shard_final(0); all-gather cand_dev; shard_overshoot on the winner           (as for the other exchange paths)
 * peer_link[l] (local link index l): the link's index in the link table of the rank that owns its destination station (-1 when
 * that is this rank).  The launches wait for one another: together they must be resident on the device(s) -- no more workgroups
 * of 256 stations than CUs per device; every wait is bounded (HS_E_HIP instead of a hang).  One shard per PROCESS: launches of one
 * process on several streams may share a hardware queue and then run one after the other. */
int hs_engine_shard_live_export(hs_engine *h, void *handles_out);               /* 3 x HS_IPC_HANDLE_BYTES: records, words, positions */
int hs_engine_shard_live_attach(hs_engine *h, const void *all_handles, const int32_t *peer_link);
int hs_engine_shard_live_run(hs_engine *h);
int hs_engine_shard_live_wait(hs_engine *h);
int hs_engine_shard_begin(hs_engine *h, int64_t end_ns);
int hs_engine_shard_window(hs_engine *h, int64_t k);
int hs_engine_shard_inject(hs_engine *h, int64_t k);
int hs_engine_shard_progress(hs_engine *h, int64_t k_last, int64_t *window_end_out);
int hs_engine_shard_final(hs_engine *h, int64_t k);
int hs_engine_shard_overshoot(hs_engine *h, int32_t lp);
/* Asynchronous exchange ROUNDS instead of windows (same attach / begin / final / overshoot): every shard runs the
 * asynchronous engine (per-link lower bounds, hs_net_async) for `max_iters` iterations, then the caller moves the outbox
 * rows (all-to-all) and all-reduces (MAX) `bounds_dev` -- device int64[n_cross + 1]: the lower bound of every cross-shard
 * link (network-wide ids in cross_gid, the same list on every rank) and, last, an "I still have work" flag -- and calls
 * inject_async.  Rounds follow the boundary stations' lookahead (tens of ms of simulated time) instead of the smallest
 * link latency.  async_done synchronises and reports the all-reduced flag of the last round.
 *   begin; do { round; <all-to-all>; <all-reduce MAX bounds_dev>; inject_async; } while (any_not_done); final(0); ... */
int hs_engine_shard_async_setup(hs_engine *h, int32_t n_cross, const int64_t *cross_gid, int64_t *bounds_dev, int32_t max_iters);
int hs_engine_shard_round(hs_engine *h);
int hs_engine_shard_inject_async(hs_engine *h);
int hs_engine_shard_async_done(hs_engine *h, int32_t *any_not_done);
/* DEVICE-SIDE exchange between the rounds, replacing the all-to-all and the all-reduce of the bounds (the reference's exchange
 * step: parallel/coordinator.py:182-227 drains Python outboxes on the main thread).  Every rank exports the handles of its two
 * exchange buffers (hipIpcGetMemHandle; HS_IPC_HANDLE_BYTES each: inbox, bounds), the ranks all-gather them (2 x world handles in
 * rank order) and attach (hipIpcOpenMemHandle: the peers' buffers mapped into this process -- xGMI peer-to-peer across GPUs, plain
 * device memory when ranks share a GPU).  After a round, `push` writes this rank's outbox rows and link bounds straight into the
 * peers' buffers (system-scope stores, only the messages that exist); then ONE barrier -- the stream-ordered all-reduce of the
 * "still working" word, the only collective left on the path -- and `inject_ipc` takes what the peers pushed (system-scope loads,
 * element-wise max of the bounds) and injects it as inject_async does.  The buffers are double-buffered by round parity, which is
 * what makes one barrier per round enough.
 *   export; <all-gather handles>; attach; begin; do { round; push; <all-reduce MAX of 1 word>; inject_ipc; } while (any_not_done); final(0) */
#define HS_IPC_HANDLE_BYTES 64
int hs_engine_shard_ipc_export(hs_engine *h, void *handles_out /* 2 x HS_IPC_HANDLE_BYTES */);
int hs_engine_shard_ipc_attach(hs_engine *h, const void *all_handles /* world x 2 x HS_IPC_HANDLE_BYTES, rank order */);
/* ... ranks that live in ONE process (virtual shards on one device: tests, tools) hand each other the buffers' addresses instead:
 * ipc_buffers returns this engine's two buffers (after ipc_export), peers_local takes the [world] addresses of every rank's. */
int hs_engine_shard_ipc_buffers(hs_engine *h, int64_t **inbox_out, int64_t **bounds_out);
int hs_engine_shard_peers_local(hs_engine *h, int64_t *const *inbox_ptrs, int64_t *const *bounds_ptrs);
int hs_engine_shard_push(hs_engine *h);
int hs_engine_shard_inject_ipc(hs_engine *h);
/* Simulation.__init__ bootstrap (core/simulation.py:145-154): clock to start_ns, every Source draws its
 * first arrival.  Called implicitly by the first run; call again to rewind the engine for another run.
 * (On a uniform grid small enough for one wavefront per LP -- csrc/hs_kernels_wave.hpp -- the bootstrap is performed by the next
 * run's kernel itself instead of a launch of its own; any getter or other run path in between performs it first: no observable
 * difference, one launch and one round trip of the state through HBM less.) */
int hs_engine_reset(hs_engine *h);
/* == Simulation._execute_until(end_ns): process events until the last processed event's time exceeds
 * end_ns (one-event overshoot included).  Re-entrant (windows, core/simulation.py:527-541 `_run_window`): station engines continue
 * from the state the call before left; NETWORK engines (hs_engine_set_network) hold no mid-run state between launches and REPEAT
 * the run from start_ns to the new end_ns -- the reference processes events in one global order whatever the window ends are, so
 * the state after windows e_1 <= ... <= e_k is the state of one run to e_k (tests/test_gpu_ring.py) -- at the cost of the whole
 * prefix per window.  An end_ns at or before the previous one moves nothing (the reference's loop condition is already false).
 * Blocks until the device work is complete. */
int hs_engine_run_until(hs_engine *h, int64_t end_ns);
/* Same, but only enqueues the work on the engine's stream.  The results are FINAL behind hs_engine_synchronize: that is where a run
 * that skipped the prologue (hs_engine_prologue_path) or tandem passes that met an undecided tie (hs_engine_tandem_path) are
 * repeated on the single heap.  Every getter below (get_summary, get_lp_stats, get_net_stats, read_sink(s), read_probe(_slot),
 * read_source_generated) finalises a pending asynchronous run first, so results read without an explicit synchronize are final too. */
int hs_engine_run_until_async(hs_engine *h, int64_t end_ns);
int hs_engine_synchronize(hs_engine *h);
/* hs_engine_reset + hs_engine_run_until_async, `repeats` times back to back on the engine stream, timing
 * each run kernel with HIP events recorded on that stream; ms_out[repeats] receives per-run kernel times.
 * Used by bench.py (the whole call is also wall-clocked by the caller). */
int hs_engine_bench_runs(hs_engine *h, int64_t end_ns, int32_t repeats, float *kernel_ms_out, float *total_ms_out);

int hs_engine_get_summary(hs_engine *h, hs_summary *out);
int hs_engine_get_lp_stats(hs_engine *h, const hs_lp_stats *out);
/* Sink records of one LP in processing order: completion time and context["created_at"]
 * (components/common.py:36-44).  Returns the number of records copied (<= cap) or a negative hs_status. */
int64_t hs_engine_read_sink(hs_engine *h, int32_t lp, int64_t *t_ns, int64_t *created_ns, int64_t cap);
/* All LPs at once: counts[n_lp] receives per-LP record counts; t_ns/created_ns receive the records
 * concatenated in LP order (caller sizes them from a previous get_lp_stats / sink_records). */
int64_t hs_engine_read_sinks(hs_engine *h, int64_t *counts, int64_t *t_ns, int64_t *created_ns, int64_t cap_total);

/* =====================================================================================================
 * Load-balancer topologies (BASELINE configs[4]; reference: components/load_balancer/load_balancer.py:347-433,
 * strategies.py:336-433, wiring of examples/visual/chash_example.py:118-140):
 *
 *     S x Source  ->  LoadBalancer(strategy=ConsistentHash(virtual_nodes))  ->  B x Server  ->  Sink(s)
 *
 * All hops between a Source's tick and the backend's queue take zero simulated time, so there is no lookahead for
 * conservative windows; but the graph is feed-forward, so one `_execute_until(end)` is a PIPELINE of device passes:
 *   1. every Source LP (one lane each) generates its ticks up to end_ns, draws the client id of each Request
 *      (metadata["client_id"] = str(int(u * n_clients)), u from the source's KEY stream -- the Philox-plugged form of
 *      chash_example.py:69-88) and looks up the backend ConsistentHash.select picks for it;
 *   2. the Requests are radix-sorted by (backend, arrival ns) -- this is the part of the reference's global heap
 *      order (core/event_heap.py:54-108) that matters to a backend;
 *   3. every backend LP (one lane each) runs the Queue/Driver/Worker protocol over its arrival list;
 *   4. completions of a Sink shared by all backends are radix-sorted by completion ns (the Sink's processing order);
 *   5. the first event beyond end_ns is elected among all LPs (one-event overshoot, core/simulation.py:472).
 * The md5 ring is built on the host once, at creation (ConsistentHash.add_backend runs in LoadBalancer.__init__).
 * One run per hs_lb_run call (the call is not re-entrant: it restarts from start_ns). */
typedef struct hs_lb_config {
    uint32_t struct_size;
    int32_t device;
    int32_t n_sources;
    int32_t n_backends;
    int64_t start_ns;
    int64_t horizon_ns;        /* latest end_ns that will be passed to hs_lb_run: sizes every buffer */
    uint64_t seed;             /* Philox key of the run */
    int32_t virtual_nodes;     /* ConsistentHash(virtual_nodes=...), >= 1 */
    int32_t shared_sink;       /* 1: every backend's downstream is ONE Sink; 0: one Sink per backend (or none, see egress) */
    int64_t tick_capacity;     /* ticks per source in the arrival log; 0 = derive from rate * horizon */
    int32_t strategy;          /* hs_lb_strategy: how LoadBalancer._forward_request picks the backend (load_balancer.py:368) */
    int32_t reserved;
} hs_lb_config;
/* LoadBalancingStrategy.select (components/load_balancer/strategies.py), all backends healthy:
 *   CONSISTENT_HASH  strategies.py:336-433: the md5 ring over `virtual_nodes` points per backend, key = metadata["client_id"];
 *   ROUND_ROBIN      strategies.py:50-73, the LoadBalancer's DEFAULT: backends[_index % len(backends)], _index += 1 per select --
 *                    i.e. the k-th Request the LoadBalancer processes (global (time, _sort_index) order over all Sources) goes
 *                    to backend k mod B.  The engine ranks all Requests by arrival first (one more device sort), then proceeds
 *                    as for any other assignment;  hs_lb_sources.n_clients and virtual_nodes are ignored;
 *   RANDOM           strategies.py:137-150: random.choice(backends) with the choice plugged like every draw of the seed-matched
 *                    definition: backends[int(u * len(backends))], u = the Request's draw from its Source's
 *                    KEY stream (the stream the client ids come from otherwise);  n_clients and virtual_nodes are ignored.
 *   WEIGHTED_ROUND_ROBIN  strategies.py:75-134, the smooth (nginx) algorithm: every current weight grows by its backend's weight,
 *                    the first maximum is taken and loses the total weight W.  The sequence is periodic in W, so the engine keeps
 *                    ONE period as a table (csrc/hs_wrr.hpp: built per weight class in exact int64 arithmetic) and the k-th
 *                    selection is table[k % W]; W <= 2^24 entries of int32 (a longer table is refused by name, HS_E_UNSUPPORTED).
 *                    Weights: strategy._weights (set_weight), default 1 -- hs_lb_set_weights / hs_graph_set_lb_weights.  Here the
 *                    Requests are ranked like ROUND_ROBIN's and the rank indexes the table (hs_lb_rr_assign);
 *   IP_HASH          strategies.py:294-333: backends[int(md5(key).hexdigest(), 16) % len(backends)], key = str(client_id) -- the
 *                    CONSISTENT_HASH path with another client -> backend table (a Request without a key takes the strategy's own
 *                    RoundRobin, which only such Requests advance: general entity graphs run those);
 *   The two strategies below select by live backend state; hs_lb_create refuses them by name, general entity graphs
 *   (HS_NODE_LB of hs_graph_nodes) run them:
 *   LEAST_CONNECTIONS  strategies.py:152-186: min(backends, key=active_requests), the first minimum in add_backend order;
 *                    Server.active_requests is the requests IN SERVICE (FixedConcurrency._active), not the queue depth;
 *   WEIGHTED_LEAST_CONNECTIONS  strategies.py:189-237: min(backends, key=active_requests / weight), a binary64 quotient; first minimum. */
typedef enum hs_lb_strategy { HS_LB_CONSISTENT_HASH = 0, HS_LB_ROUND_ROBIN = 1, HS_LB_RANDOM = 2, HS_LB_WEIGHTED_ROUND_ROBIN = 3,
                              HS_LB_IP_HASH = 4, HS_LB_LEAST_CONNECTIONS = 5, HS_LB_WEIGHTED_LEAST_CONNECTIONS = 6 } hs_lb_strategy;

typedef struct hs_lb_sources {     /* [n_sources] each; NULL = documented default */
    const uint8_t *src_kind;           /* hs_source_kind (POISSON / CONSTANT); NULL = POISSON */
    const double *src_rate;            /* required */
    const int64_t *src_stop_after_ns;  /* < 0 = never; the provider returns no Request when time > stop_after */
    const int64_t *n_clients;          /* client ids are drawn uniformly from [0, n_clients); required, >= 1 */
    const uint64_t *stream_base;       /* NULL = i */
    /* Source.with_profile(LinearRampProfile | SpikeProfile) in front of the LoadBalancer: as hs_stations.src_profile_kind /
     * src_profile_params (src_rate = the PEAK rate: it sizes the tick log).  NULL = constant rates. */
    const uint8_t *src_profile_kind;   /* hs_profile_kind */
    const double *src_profile_params;  /* [n_sources][4] */
} hs_lb_sources;

typedef struct hs_lb_backends {    /* [n_backends] each */
    const int32_t *concurrency;        /* 1..32; NULL = 1 */
    const uint8_t *svc_kind;           /* hs_latency_kind; NULL = HS_LAT_CONSTANT */
    const double *svc_mean_s;          /* NULL = 0.01 */
    const int64_t *queue_cap;          /* < 0 = unbounded */
    const uint8_t *egress;             /* HS_EGRESS_NONE / HS_EGRESS_SINK; NULL = SINK */
    const uint64_t *stream_base;       /* NULL = n_sources + j */
    const char *names;                 /* concatenated backend names (the ring hashes "<name>:<i>"); required */
    const int32_t *name_off;           /* [n_backends + 1] offsets into names */
} hs_lb_backends;

typedef struct hs_lb_stats {       /* any pointer may be NULL */
    int64_t *generated;        /* [n_sources]  Source._generated_count */
    int64_t *lb;               /* [5] LoadBalancer.stats: requests_received, requests_forwarded, requests_failed,
                                      no_backend_available, len(_in_flight) */
    int64_t *total_requests;   /* [n_backends] BackendInfo.total_requests (load_balancer.py:385-386) */
    int64_t *accepted, *dropped, *completed, *rejected;   /* [n_backends] as hs_lp_stats */
    double *total_service_s;   /* [n_backends] */
    int64_t *queue_depth;      /* [n_backends] */
    int32_t *active;           /* [n_backends] */
    int64_t *sink_received;    /* [n_backends] Request@Sink events caused by this backend's completions */
} hs_lb_stats;

typedef struct hs_lb hs_lb;

int hs_lb_create(const hs_lb_config *cfg, const hs_lb_sources *src, const hs_lb_backends *be, hs_lb **out);
/* Simulation.__init__ + run() to end_ns.  Blocks until the device work is complete.  Every call runs from start_ns: windows
 * e_1 <= ... <= e_k over a load-balancer graph (`_run_window`, core/simulation.py:527-541) are k calls, and the state after the
 * last one is the state of one run to e_k -- which is what the reference's windows leave (one global event order, every call stops
 * behind the first event beyond its end): tests/test_gpu_lb.py::test_lb_windows_equal_one_run. */
int hs_lb_run(hs_lb *h, int64_t end_ns);
/* WeightedRoundRobin.set_weight (strategies.py:93-105) for every backend at once: weights[n_backends], before the first run; the
 * default is all ones (RoundRobin's sequence).  HS_E_INVALID for a weight below 1, HS_E_UNSUPPORTED for a total weight above 2^24,
 * HS_E_STATE after a run.  A strategy that reads no weights ignores them (as the reference ignores BackendInfo.weight). */
int hs_lb_set_weights(hs_lb *h, const int32_t *weights);
/* Which paths the last hs_lb_run took, as HS_LB_RUN_* bits (read-only, for tests). */
#define HS_LB_RUN_F64_TIMES    (1 << 0)    /* Sources and the scan keep whole nanoseconds as binary64 */
#define HS_LB_RUN_MARGIN       (1 << 1)    /* speculated whole-ns arrival steps (lb_step_encode; horizon < 2^40) */
#define HS_LB_RUN_LEAN         (1 << 2)    /* hs_lbk_sources_lean */
#define HS_LB_RUN_SCAN         (1 << 3)    /* the backends as (max, +) scans (hs_lbk_scan) */
#define HS_LB_RUN_SINK_PACKED  (1 << 4)    /* shared Sink merge: created_at << slot_bits | slot in one word */
#define HS_LB_RUN_SINK_GATHER  (1 << 5)    /* shared Sink merge: created_at gathered by slot */
#define HS_LB_RUN_DENSE        (1 << 6)    /* backends outside the scan read the dense segments, not [k][backend]: debug flag 4, no
                                            * rows allocated, or the busiest backend had more Requests than the rows allocated */
int hs_lb_run_path(const hs_lb *h);
/* The sorts' plan, fixed at hs_lb_create (read-only, for tests that must cross these sizes):
 * out = { tb, bb, g_arr, g_sink, kSegTile, kSegHalo } -- time and backend bits of the sort key, the low key bits the arrival sort
 * and the Sink merge skip, and the LDS tile and halo of the kernels that finish the runs those bits leave.  HS_OK, or HS_E_INVALID
 * on null. */
int hs_lb_sort_plan(const hs_lb *h, int32_t out[6]);
/* `repeats` complete runs back to back on the engine's stream; per-run device time of the whole pipeline and of the
 * sort passes alone (HIP events on that stream). */
int hs_lb_bench_runs(hs_lb *h, int64_t end_ns, int32_t repeats, float *run_ms_out, float *sort_ms_out);
int hs_lb_get_summary(hs_lb *h, hs_summary *out);
int hs_lb_get_stats(hs_lb *h, const hs_lb_stats *out);
/* Sink records in the Sink's processing order.  shared_sink: sink must be 0 (all completions, global order);
 * otherwise sink = backend index.  Returns the number of records copied or a negative hs_status. */
int64_t hs_lb_read_sink(hs_lb *h, int32_t sink, int64_t *t_ns, int64_t *created_ns, int64_t cap);
/* Probe.on(<backend Server> | <Sink>, metric, interval) on a load-balancer graph (instrumentation/probe.py:81-164), set once
 * after hs_lb_create and before the first run: target_kind 0 = backend Server `target_index` (depth, active_requests,
 * stats_accepted, stats_dropped, requests_completed), 1 = Sink `target_index` (events_received; the shared Sink is index 0),
 * 2 = Source `target_index` (generated_count; not for a Source with stop_after).
 * Tick times follow the reference's ConstantArrivalTimeProvider over _ProbeProfile; each tick at or before end_ns is two
 * reference events (kinds 13, 14) and the pending tick takes part in the election of the one event beyond end_ns.  The samples
 * are read off the run's logs; a sample on the very nanosecond of an event of its target makes hs_lb_run fail with
 * HS_E_UNSUPPORTED (that order is the reference's sort-index ledger, not lowered for this graph) -- never a guess. */
int hs_lb_set_probes(hs_lb *h, int32_t n_probes, const int32_t *target_kind, const int32_t *target_index,
                     const uint8_t *metric, const double *interval_s);
/* samples of probe `probe` in the last run: times and values -> returns their number (<= cap) */
int64_t hs_lb_read_probe(hs_lb *h, int32_t probe, int64_t *t_ns, int64_t *values, int64_t cap);
/* Sink.latency_stats() of the shared Sink, computed on the device (components/common.py:59-76 with
 * instrumentation/data.py:197-210): out = {count, avg, min, max, p50, p99} in seconds.  avg = sum(sorted latencies) / n with
 * the sum taken in index order in binary64 the way hs_set_float_sum_mode says. */
int hs_lb_latency_stats(hs_lb *h, double out[6]);
/* What `sum(list_of_floats)` means on the interpreter that runs the reference (CPython Python/bltinmodule.c builtin_sum):
 * 0 = plain left-to-right additions (CPython < 3.12; the library's default), 1 = Neumaier's compensated sum (CPython >= 3.12 --
 * the reference requires >= 3.13, pyproject.toml:11).  The host side sets it from sys.version_info, so that the device
 * statistics (hs_lb_latency_stats, hs_sink_latency_stats) equal what the same interpreter computes from the list
 * (components/common.py:59-76 `sum(sorted_vals) / n`).  Process-wide. */
int hs_set_float_sum_mode(int compensated);
/* The sorted ring's backend index per point, [n_backends * virtual_nodes] (strategies.py:381-391). */
int hs_lb_ring(hs_lb *h, int32_t *ring_backend);
/* ConsistentHash.select for a key string (strategies.py:412-433): backend index. */
int32_t hs_lb_select(hs_lb *h, const char *key);
const char *hs_lb_last_error(const hs_lb *h);
void hs_lb_destroy(hs_lb *h);
/* md5 digest of a byte string (the ring's hash function), exported so tests can check it against RFC 1321. */
void hs_md5(const char *msg, int64_t len, uint8_t out[16]);
/* WeightedRoundRobin.select (strategies.py:111-134) over backends 0 .. n-1 as ONE period of its selection sequence: out[k] = the
 * backend of selection k for k < min(W, cap); returns the total weight W = the period.  Host only (no device).  HS_E_INVALID for a
 * weight below 1 (`set_weight` raises ValueError, :103-104), HS_E_UNSUPPORTED for W > 2^24. */
int64_t hs_lb_wrr_table(const int32_t *weights, int32_t n, int32_t *out, int64_t cap);
/* IPHash.select for a key string (strategies.py:330-333): int(md5(key).hexdigest(), 16) % n_backends.  Host only. */
int32_t hs_lb_ip_hash_select(const char *key, int32_t n_backends);

/* Debug: bit 0 routes every timestamp group of every backend through the general in-group FIFO path; bit 1 disables the
 * request-order loop of single-worker unbounded backends (event-order loop with its single-event fast path instead);
 * bit 2 keeps the backend streams in dense per-backend segments instead of the wave-coalesced [k][backend] layout;
 * 8: the Sources draw their own stream values; 16: look-back radix passes; 32: 32 LPs per wavefront; 64: round 3's backend pipeline
 * instead of the segmented scan; 128: the int64 instantiation of the scan; 256: no speculated whole-ns arrival steps;
 * 512: hs_lbk_sources instead of hs_lbk_sources_lean; 1024: the lean Source kernel gives up, so that the run repeats with
 * hs_lbk_sources.  Every combination gives bit-identical results (tests/test_gpu_lb.py). */
int hs_debug_lb_flags(hs_lb *h, int flags);

/* Debug / tests: stable LSD radix sort of n (key, value) pairs on `device` over key bits [0, key_bits) --
 * the sort the load-balancer engine uses (csrc/hs_radix.hpp).  Host arrays in, host arrays out. */
int hs_debug_radix_sort(int32_t device, int64_t n, int32_t key_bits, const uint64_t *keys_in, const uint64_t *vals_in,
                        uint64_t *keys_out, uint64_t *vals_out, float *device_ms);
/* Merge of per-station Sink logs into ONE Sink shared by several stations (components/common.py:36-44 appends in global
 * processing order): stable device sort of n (completion ns, created_at ns) records by completion time, in place on host
 * arrays.  Feed it the stations' records concatenated in station order. */
int hs_merge_sink_records(int32_t device, int64_t n, int64_t *t_ns, int64_t *created_ns);

/* Sink.latency_stats() (components/common.py:59-76; percentiles as instrumentation/data.py:197-210) of a Sink's records on
 * the device: latency = t - created_at in ns -> seconds, radix sort, binary64 sum of the SORTED values in index order (what
 * `sum(sorted_vals)` does: hs_set_float_sum_mode), interpolated percentiles.  out = {count, avg, min, max, p50, p99}.  Host buffers. */
int hs_sink_latency_stats(int32_t device, int64_t n, const int64_t *t_ns, const int64_t *created_ns, double out[6]);

/* Samples of the LP's Probe in sampling order: (sample time ns, value) -- what the reference appends to the probe's
 * Data container (instrumentation/probe.py:63).  Returns the number copied or a negative hs_status. */
int64_t hs_engine_read_probe(hs_engine *h, int32_t lp, int64_t *t_ns, int64_t *values, int64_t cap);
/* ... of the probe in `slot` (0 .. 3) of the LP */
int64_t hs_engine_read_probe_slot(hs_engine *h, int32_t lp, int32_t slot, int64_t *t_ns, int64_t *values, int64_t cap);
/* Source.generated_count of the Sources in `slot` (1 .. 3: hs_stations.src_more_*; slot 0 = hs_lp_stats.generated) of
 * every LP -> out[n_lp]. */
int hs_engine_read_source_generated(hs_engine *h, int32_t slot, int64_t *out);

const char *hs_last_error(const hs_engine *h);
const char *hs_last_global_error(void);
void hs_engine_destroy(hs_engine *h);

/* Device-side scalar semantics, exported so tests can compare them bit-for-bit with the oracle:
 * fills u[i] = uniform(seed, sid, k0+i), e[i] = -hs_log(1-u[i]), ns[i] = trunc((e[i]/rate)*1e9). */
/* Debug: bit 0 routes every timestamp group through the general in-group FIFO path (tests compare it with
 * the fast path); bit 4 (16) runs a station network on the windowed engine (one launch per window) even when the
 * asynchronous whole-run engine is available; bit 6 (64) disables the asynchronous engine's in-wavefront scan of the
 * per-link bounds; bit 7 (128) makes its idle wavefronts back off (s_sleep) between polls. */
int hs_debug_set_flags(hs_engine *h, int flags);
/* Debug: telemetry of the last asynchronous network run: {sum over wavefronts of loop iterations, max over wavefronts,
 * timestamp groups run (sum over LPs), wavefronts}. */
int hs_debug_async_counters(hs_engine *h, unsigned long long out[4]);

int hs_debug_draws(int32_t device, uint64_t seed, uint64_t sid, uint64_t k0, int64_t n, double rate,
                   double *u, double *e, int64_t *ns);
/* Debug: the stream functions of csrc/hs_device.hpp at CHOSEN inputs, host arrays in and out, one element per thread
 * (tests/test_gpu_streams.py compares every bit with the oracle).
 *   hs_debug_log          out_log[i] = hs_log(x[i]) (x normal and positive), out_exp1[i] = exp1_from_uniform(u[i])
 *   hs_debug_philox       ctr_key[6 i ..] = {c0, c1, c2, c3, k0, k1} -> out[4 i ..] = the raw Philox4x32-10 block, all 128 bits
 *   hs_debug_stream_walk  one thread per walk: Stream::init(seed[w], sid[w], k0[w]), then for each of the n_steps entries of
 *                         `steps` (shared by all walks; each 1, 2 or 4) next_uniform / next2 / next4; out[w][..] = the
 *                         sum(steps) values in draw order, k_end[w] = the stream's final draw index. */
int hs_debug_log(int32_t device, int64_t n, const double *x, const double *u, double *out_log, double *out_exp1);
int hs_debug_philox(int32_t device, int64_t n, const uint32_t *ctr_key, uint32_t *out);
int hs_debug_stream_walk(int32_t device, int64_t n_walks, const uint64_t *seed, const uint64_t *sid, const uint64_t *k0,
                         int32_t n_steps, const uint8_t *steps, double *out, uint64_t *k_end);

/* Evaluation budget of the tick-table kernel (csrc/hs_tables.hpp): adaptive-Simpson intervals ONE lane may visit for ONE
 * arrival of a time-varying Source (64 lanes share an integral).  Replaces nothing in the reference -- its integrator
 * (numerics/integration.py:11-90) has no limit and needs minutes for such arrivals; this is the device's time guard, a
 * RUN-TIME argument (round 2: a build-time constant).  Default 2^24; takes effect at the next reset / run. */
int hs_engine_set_profile_budget(hs_engine *h, int64_t intervals_per_lane);
int hs_lb_set_profile_budget(hs_lb *h, int64_t intervals_per_lane);

/* Debug / test hook: the tick table of one stream -- next_arrival_time's general path (load/arrival_time_provider.py:84-144)
 * iterated from start_ns until two ticks lie beyond horizon_ns.  profile = {kind (1 ramp, 2 spike, 3 constant rate through the
 * general path), p0..p3}; lone = 0: the cooperative kernel, 1: one lane with the sequential integrator.  Returns the number of
 * entries (<= cap) or a negative error; out_status[0] != 0: over the evaluation budget, out_status[1] != 0: cap too small. */
int64_t hs_debug_tick_table(int32_t device, const double *profile, int32_t poisson, uint64_t seed, uint64_t sid,
                            int64_t start_ns, int64_t horizon_ns, int64_t cap, int64_t lane_budget, int32_t lone,
                            int64_t *out_times, uint64_t *out_status);

/* Debug: the engine divides by per-LP constants (1e9, rate, lambda) with a multiply + FMA sequence that must be
 * bit-identical to the IEEE quotient.  q_fast[i] = that sequence for a[i] / b, q_ieee[i] = the hardware
 * division, q_ns[i] = seconds_from_ns((int64)a[i]) (compare with a[i] / 1e9). */
int hs_debug_const_div(int32_t device, double b, int64_t n, const double *a, double *q_fast, double *q_ieee,
                       double *q_ns);
/* Debug: the device time algebra (csrc/hs_device.hpp) on n inputs: out_f64[3 i] = seconds_from_ns(ns[i]),
 * out_f64[3 i + 1] = seconds_from_ns_d((double)ns[i]), out_f64[3 i + 2] = ns_from_seconds_d(secs[i]),
 * out_i64[2 i] = ns_from_seconds(secs[i]), out_i64[2 i + 1] = i64_from_whole_d((double)ns[i]). */
int hs_debug_time_ops(int32_t device, int64_t n, const int64_t *ns, const double *secs, double *out_f64, int64_t *out_i64);

/* ------------------------------------------------------------------------------------------------------------------
 * General entity graphs (ABI 15; LoadBalancer nodes: ABI 16).
 *
 * The station engines take graphs of the shape [Sources] -> Server -> {Sink | NetworkLink | RandomRouter} with one sender
 * per link, <= 4 Sources per Server, <= 4 router targets ... (hs_engine_set_stations / hs_engine_set_network).  Everything
 * else the same entity classes can be wired into -- a NetworkLink with several senders (components/network/link.py:114-189),
 * a RandomRouter with any number of targets, among them Servers and other routers, and with several upstreams
 * (components/random_router.py:32-45), Server(downstream=<Server>) next to links (components/server/server.py:64-122,271-272),
 * any number of Sources per Server (load/source.py:93-180), any concurrency (server/concurrency.py:67-141) -- runs here:
 * ONE heap ordered by (time, _sort_index), popped event by event like `Simulation._execute_until`
 * (core/simulation.py:449-505), every reference Event materialised with the sort index the reference gives it (the two
 * counters of core/event.py:53-77 and core/event_heap.py:48), push / pop in CPython's heapq sift order.  One lane of one
 * wavefront walks the loop; the first 4 096 heap entries live in LDS (128 KB of the CU's 160), the rest and all node state
 * in HBM.  An exactness path for small models (~2.4 us per event and heap; heaps side by side: hs_graph_run_many / _parts), not a throughput path: the station engines stay the
 * product's hot path, and the host (happy_simulator_amd/graph_engine.py) only comes here with a graph they refuse.
 * Replaces: Simulation.__init__'s bootstrap (core/simulation.py:145-160), Simulation.schedule (:195-206), _execute_until
 * (:449-505) and the handlers of load/source.py:142-180, components/queue.py:122-166, components/queue_driver.py:66-99,
 * components/server/server.py:202-273, components/common.py:36-44, components/random_router.py:32-45,
 * components/network/link.py:114-216 for such a graph.
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct hs_graph hs_graph;

typedef enum hs_node_kind { HS_NODE_SOURCE = 0, HS_NODE_SERVER = 1, HS_NODE_SINK = 2, HS_NODE_LINK = 3, HS_NODE_ROUTER = 4, HS_NODE_PROBE = 5, HS_NODE_LB = 6,
                             HS_NODE_RATE_LIMITER = 7, /* RateLimitedEntity: `target` = its downstream, `queue_cap` = its FIFO capacity; policy: hs_graph_set_limiter_policy */
                             HS_NODE_HEALTH_CHECKER = 8, /* HealthChecker: `target` = -1 or its LoadBalancer; everything else: hs_graph_set_health_checker */
                             HS_NODE_BULKHEAD = 9,        /* Bulkhead: `target` = the entity it protects; everything else: hs_graph_set_wrapper */
                             HS_NODE_TIMEOUT_WRAPPER = 10, /* TimeoutWrapper: `target` = the entity it wraps; everything else: hs_graph_set_wrapper */
                             HS_NODE_CLIENT = 11,         /* Client: `target` = the entity it sends to; everything else: hs_graph_set_client */
                             HS_NODE_BATCH_PROCESSOR = 12, /* BatchProcessor, ConveyorBelt, GateController: `target` = their downstream; */
                             HS_NODE_CONVEYOR = 13,        /* everything else: hs_graph_set_flow */
                             HS_NODE_GATE = 14,
                             HS_NODE_AUTO_SCALER = 15,     /* AutoScaler: `target` = -1 or its LoadBalancer; everything else: hs_graph_set_auto_scaler */
                             HS_NODE_ROLLING_DEPLOYER = 16,/* RollingDeployer: `target` = -1 or its LoadBalancer; everything else: hs_graph_set_rolling_deployer */
                             HS_NODE_CANARY_DEPLOYER = 17, /* CanaryDeployer: `target` = -1 or its LoadBalancer; everything else: hs_graph_set_canary_deployer */
                             HS_NODE_HEDGE = 18,           /* Hedge: `target` = the entity it sends to; everything else: hs_graph_set_hedge */
                             HS_NODE_FALLBACK = 19,        /* Fallback: `target` = its primary; the fallback entity and the rest: hs_graph_set_fallback */
                             HS_NODE_POOLED_CYCLE = 20,    /* PooledCycleResource: `target` = its downstream or -1; everything else: hs_graph_set_pool */
                             HS_NODE_INVENTORY = 21        /* InventoryBuffer: `target` = its downstream or -1; its stock-out target and the rest: hs_graph_set_inventory */
} hs_node_kind;

typedef struct hs_graph_config {
    uint32_t struct_size;            /* sizeof(hs_graph_config) */
    int32_t device;
    int64_t start_ns;                /* Simulation(start_time=) */
    uint64_t seed;                   /* Philox key of every entity stream */
    int64_t heap_capacity;           /* pending events; 0 = sized from the graph.  All three capacities GROW on demand: */
    int64_t request_capacity;        /* Requests alive (queued, in service, in transit); 0 = sized from the graph */
    int64_t record_capacity;         /* Sink records of the whole run; 0 = 65 536 */
    int64_t max_events;              /* a run that would process more is refused (HS_E_UNSUPPORTED); 0 = no limit */
    int64_t profile_budget;          /* adaptive-Simpson intervals one lane may visit for one tick of a time-varying Source or a
                                      * Probe (hs_engine_set_profile_budget); 0 = the default 2^24 */
} hs_graph_config;

/* Nodes in the caller's order.  SOURCE nodes must come in `sources=[...]` order (their first SourceEvents take the pre-run
 * sort indices 0, 1, ... in that order, core/simulation.py:145-154).  Entity streams: sid = stream_base << 3 | kind
 * (DESIGN.md section 3): a Source draws ARRIVAL, a Server SERVICE, a link LINK (jitter) and LOSS, a router ROUTE. */
typedef struct hs_graph_nodes {
    int32_t n_nodes;
    const uint8_t *kind;             /* [n] hs_node_kind */
    const int32_t *target;           /* [n] Source: the node its Requests are aimed at; Server: downstream; link: egress; -1 = none */
    const uint64_t *stream_base;     /* [n] */
    const uint8_t *src_kind;         /* [n] Sources: HS_SRC_POISSON / HS_SRC_CONSTANT (constant-rate profile) */
    const double *src_rate;          /* [n] Sources: events / s, > 0 */
    const int64_t *src_stop_after_ns;/* [n] Sources: SimpleEventProvider(stop_after); < 0 = never */
    const int32_t *concurrency;      /* [n] Servers: FixedConcurrency(max_concurrent) >= 1 */
    const uint8_t *lat_kind;         /* [n] Servers: service distribution; links: jitter (HS_LAT_EXPONENTIAL / HS_LAT_CONSTANT) */
    const double *lat_mean_s;        /* [n] ... its mean (a link with HS_LAT_CONSTANT and mean 0: jitter=None) */
    const double *link_lat_min_s;    /* [n] links: ConstantLatency base latency, >= 0 */
    const double *link_loss_rate;    /* [n] links: packet_loss_rate in [0, 1]; NULL = lossless */
    const int64_t *queue_cap;        /* [n] Servers: FIFOQueue capacity; < 0 = unbounded */
    const int32_t *rt_off;           /* [n] routers: targets rt_targets[rt_off .. rt_off + rt_cnt) in constructor order */
    const int32_t *rt_cnt;           /* [n] */
    const int32_t *rt_targets;       /* [n_rt] node ids (Sink / link / Server / router) */
    int32_t n_rt;
    /* Sources with a time-varying profile (load/profile.py:52-113; Source.with_profile): hs_profile_kind and its four parameters as
     * in hs_stations.src_profile_*; src_rate is then the peak rate.  Their ticks -- next_arrival_time's general path,
     * load/arrival_time_provider.py:84-144 -- come from the tick-table kernel (csrc/hs_tables.hpp), like the station engines'.  NULL = none. */
    const uint8_t *src_profile_kind; /* [n] */
    const double *src_profile_params;/* [n][4] */
    /* HS_NODE_PROBE: Probe(target, metric, interval) (instrumentation/probe.py:81-164) -- a Source whose provider is a constant
     * tick chain over _ProbeProfile(interval) (the general path too) and whose payload is the daemon probe_event that samples
     * getattr(target, metric).  `target` = the sampled node; PROBE nodes come behind the SOURCE nodes in `probes=[...]` order (their
     * first ticks take the pre-run indices behind the Sources', core/simulation.py:156-160).  Samples: hs_graph_read_records
     * (node = the probe, t = sample time, created = the value). */
    const uint8_t *probe_metric;     /* [n] hs_probe_metric */
    const double *probe_interval_s;  /* [n] > 0 */
    /* HS_NODE_LB: LoadBalancer(backends=[...], strategy) (components/load_balancer/load_balancer.py:347-473) -- any number of them,
     * anywhere a Request can go.  Backends = rt_targets[rt_off .. rt_off + rt_cnt) in add_backend order, SERVER nodes, all healthy.
     * ConsistentHash (strategies.py:336-433): lb_vnodes ring points md5("<backend name>:<i>") per backend (names / name_off), the key
     * of a Request is str(client_id); RoundRobin (strategies.py:50-73); Random (strategies.py:137-150) with random.choice plugged by
     * the Request's key draw: backends[client_id].  A Source with src_n_clients > 0 builds its Requests like a
     * ClientKeyEventProvider (examples/visual/chash_example.py:69-88): client_id = int(u * n_clients), u from its KEY stream.
     * WeightedRoundRobin / IPHash / LeastConnections / WeightedLeastConnections: see hs_lb_strategy; weights: hs_graph_set_lb_weights.
     * A Request WITHOUT a client_id (a scheduled one, one of a plain Source) at a ConsistentHash or IPHash LoadBalancer takes the strategy's own
     * fallback RoundRobin, which only such Requests advance (strategies.py:362,420-421); it must not reach a Random LoadBalancer
     * (the reference draws from the process-wide generator): the caller refuses such graphs; the device sends it to backend 0.  Every forwarded Request carries the `_lb_response` completion hook
     * (load_balancer.py:413-431): one more event behind the backend's enqueue.  NULL = no LoadBalancer. */
    const uint8_t *lb_strategy;      /* [n] hs_lb_strategy */
    const int32_t *lb_vnodes;        /* [n] ConsistentHash(virtual_nodes) */
    const char *names;               /* concatenated entity names (only an LB's backends need one) */
    const int32_t *name_off;         /* [n + 1] */
    const int64_t *src_n_clients;    /* [n] Sources; 0 = a plain SimpleEventProvider */
} hs_graph_nodes;

typedef struct hs_graph_stats {      /* host arrays [n_nodes] (rt_taken: [n_rt]); any pointer may be NULL */
    int64_t *generated;              /* Source._generated_count                         load/source.py:159 */
    int64_t *payloads;               /* Requests the Source's event provider built      load/source.py:67-86 */
    int64_t *accepted, *dropped;     /* Queue.stats_accepted / stats_dropped            components/queue.py:127-139 */
    int64_t *completed, *rejected;   /* Server._requests_completed / _rejected          server/server.py:112-114 */
    double *total_service_s;         /* Server._total_service_time */
    int64_t *queue_depth, *active;   /* QueuedResource.depth, Server.active_requests */
    int64_t *received;               /* Sink.events_received */
    int64_t *entered;                /* Requests that entered the link */
    int64_t *packets_sent;           /* NetworkLink.packets_sent                        components/network/link.py:162 */
    int64_t *packets_dropped;        /* NetworkLink.packets_dropped                     components/network/link.py:132 */
    int64_t *routed;                 /* RandomRouter.stats_routed                       components/random_router.py:36 */
    int64_t *rt_taken;               /* [n_rt] how often each target slot was drawn     (target_counts, random_router.py:37);
                                      * a LoadBalancer's slots: BackendInfo.total_requests       load_balancer.py:385-386 */
    int64_t *lb;                     /* [n][6] LoadBalancer: requests_received, requests_forwarded, requests_failed,
                                      * no_backend_available, len(_in_flight)                    load_balancer.py:349-388
                                      * and the selections of the strategy's RoundRobin: RoundRobin._index, the index of
                                      * ConsistentHash's / IPHash's key-less fallback, or WeightedRoundRobin's selections
                                      *                                                            strategies.py:66-67,309,362 */
} hs_graph_stats;

int hs_graph_create(const hs_graph_config *cfg, const hs_graph_nodes *nodes, hs_graph **out);
/* Simulation.schedule(Event(time, "Request", target=<node>)) (core/simulation.py:195-206): the Event was constructed outside
 * the run, so it takes the next index of the process-wide counter behind the Sources' first ticks; context["created_at"] =
 * its own time.  Calls in the order the caller constructed the Events.  `node`: a Server, Sink, link, router or
 * LoadBalancer. */
int hs_graph_schedule(hs_graph *g, int32_t node, int64_t time_ns);
/* WeightedRoundRobin.set_weight / WeightedLeastConnections.set_weight (strategies.py:93-105,203-207) for every backend of the
 * LoadBalancer `node` at once: weights[n] in slot (add_backend) order, n = its backend count.  Before the first run; the default is
 * all ones.  HS_E_INVALID for a weight below 1 or a node that is no LoadBalancer (a strategy that reads no weights ignores them, as
 * the reference ignores BackendInfo.weight), HS_E_UNSUPPORTED for a WeightedRoundRobin total weight above 2^24, HS_E_STATE after a run. */
int hs_graph_set_lb_weights(hs_graph *g, int32_t node, const int32_t *weights, int32_t n);

/* HS_NODE_RATE_LIMITER: RateLimitedEntity(name, downstream, policy, queue_capacity) (components/rate_limiter/rate_limited_entity.py)
 * -- admission control in front of any node that takes Requests.  A Request is forwarded at once when policy.try_acquire(now)
 * grants it (a NEW Event for the downstream at `now`, run-time sort index, same context, no completion hook), else queued in a FIFO
 * of `queue_cap` places and drained by ONE self-scheduled daemon poll Event at now + policy.time_until_available(now), else dropped.
 * The two handlers are internal heap-entry kinds beyond HS_EV_KINDS: they count in hs_summary.events_processed but not in
 * events_by_kind; hs_graph_get_limiter reports them per node (events_processed == sum(events_by_kind) + sum(requests + polls)).
 * The policies (components/rate_limiter/policy.py), binary64 operation for operation: */
typedef enum hs_limiter_policy {
    HS_LIMITER_TOKEN_BUCKET = 0,   /* TokenBucketPolicy(capacity, refill_rate, initial_tokens): p0 = capacity, p1 = refill_rate > 0,
                                    * p2 = the tokens the bucket starts with */
    HS_LIMITER_LEAKY_BUCKET = 1,   /* LeakyBucketPolicy(leak_rate): p0 = leak_rate > 0, p1 = its _leak_interval = 1.0 / leak_rate */
    HS_LIMITER_SLIDING_WINDOW = 2, /* SlidingWindowPolicy(window_size_seconds, max_requests): p0 = the window, count = max_requests in
                                    * [1, 2^20]: the log is a ring of that many timestamps */
    HS_LIMITER_FIXED_WINDOW = 3,   /* FixedWindowPolicy(requests_per_window, window_size): p0 = window_size, count = requests_per_window
                                    * >= 1; the window's start is Python's float floor division (now_s // window_size) * window_size */
    HS_LIMITER_NONE = 255
} hs_limiter_policy;
typedef struct hs_limiter_policy_params {
    uint32_t struct_size;            /* sizeof(hs_limiter_policy_params) */
    int32_t policy;                  /* hs_limiter_policy */
    double p0, p1, p2;
    int64_t count;
} hs_limiter_policy_params;
/* The policy of limiter `node`, between hs_graph_create and the first run (HS_E_STATE afterwards).  A run of a graph that holds a
 * limiter without a policy returns HS_E_STATE.  HS_E_INVALID: no limiter, a rate <= 0, a count < 1, a window below one nanosecond;
 * HS_E_UNSUPPORTED: a sliding-window log beyond 2^20 entries. */
int hs_graph_set_limiter_policy(hs_graph *g, int32_t node, const hs_limiter_policy_params *params);
typedef struct hs_limiter_state {
    uint32_t struct_size;            /* sizeof(hs_limiter_state), set by the caller */
    int32_t policy;
    int64_t received, forwarded, queued, dropped;   /* RateLimitedEntity.stats */
    int64_t queue_depth;
    int64_t poll_scheduled;          /* _poll_scheduled */
    int64_t requests_handled, polls_handled;        /* events of the two internal kinds this node processed */
    int64_t has_time;                /* 0: _last_refill_time / _last_leak_time / _current_window_start is None */
    int64_t time_ns;                 /* ... else its nanoseconds */
    double tokens;                   /* TokenBucketPolicy.tokens */
    int64_t count;                   /* _current_window_count; SlidingWindowPolicy: len(_request_log) */
} hs_limiter_state;
/* One limiter's state after a run; `log` (capacity `log_cap`, may be NULL) receives min(count, log_cap) timestamps of a
 * SlidingWindowPolicy's _request_log, oldest first.  Outcome of every Request and every drained one, in processing order:
 * hs_graph_read_records with node = the limiter, t = the time, created = hs_limiter_outcome. */
int hs_graph_get_limiter(hs_graph *g, int32_t node, hs_limiter_state *out, int64_t *log, int64_t log_cap);
typedef enum hs_limiter_outcome { HS_LIMITER_FORWARDED = 0, HS_LIMITER_QUEUED = 1, HS_LIMITER_DROPPED = 2, HS_LIMITER_DRAINED = 3 } hs_limiter_outcome;
/* Node faults: CrashNode / PauseNode of a FaultSchedule (faults/node_faults.py, faults/schedule.py:68-100).  One call per fault
 * Event, in the order FaultSchedule.start constructs them (add() order, crash before restart): at `time_ns` (absolute) the
 * `_crashed` flag of `node` is set (`on` != 0) or cleared.  The Events are daemon pre-run Events: they take the next values of the
 * process-wide counter behind the Sources' and Probes' first ticks and before every hs_graph_schedule entry, count in
 * hs_summary.events_processed (not in events_by_kind: two more internal kinds) and do not keep a run to end_ns = 2^61 alive.
 * While a node's flag is set, every Event aimed at the entity itself is popped, counted and dropped (core/event.py:261): SOURCE,
 * PROBE_TICK, ENQUEUE, SINK, LINK, ROUTE, LB, LB_RESP and a limiter's two kinds -- its Request returns to the pool, no completion
 * hook runs; NOTIFY / POLL / DELIVER / WORK / PROBE and the two continuations are not (other targets; ProcessContinuation.invoke
 * does not look).  `cancelled` != 0: the Event was cancelled after its construction; it keeps its counter value, is popped, skipped
 * and not processed.  Before the first run (HS_E_STATE afterwards). */
int hs_graph_add_fault(hs_graph *g, int32_t node, int64_t time_ns, int32_t on, int32_t cancelled);
/* After a run: crashed[n_nodes] = every node's flag as the run left it; internal_by_kind[4] = the graph's Events of the four
 * internal kinds, counted like events_by_kind counts the public ones (an Event dropped at a crashed target included): a limiter's
 * Requests, its polls, fault Events that set a flag, fault Events that clear one -- events_processed == sum(events_by_kind) +
 * sum(internal_by_kind); *cancelled = cancelled fault Events popped.  Any of the three may be NULL. */
int hs_graph_get_faults(hs_graph *g, uint8_t *crashed, int64_t *internal_by_kind, int64_t *cancelled);
/* Link faults: InjectLatency and InjectPacketLoss (faults/network_faults.py:27-198).  Each of a fault's two Events is one call, in the
 * one FaultSchedule.add() order with hs_graph_add_fault's (they share the numbering, the daemon rule, `cancelled` and the two internal
 * kinds: an activation counts as a fault Event that sets, a deactivation as one that clears).  The Events are aimed at a callback, not
 * at the link: a crashed or paused link does not drop them.  `what`: HS_LINK_FAULT_LATENCY -- from an activation on, the base term of
 * the link's delay is Duration.from_seconds(base.to_seconds() + value) taken back to seconds, value = the extra as the seconds of the
 * Duration the reference's ConstantLatency(extra_ms / 1000) returns; HS_LINK_FAULT_LOSS -- from an activation on, the loss rate is
 * `value` (min(1.0, original + loss_rate)).  A deactivation restores the node's own lat_min / loss_rate whichever activation came last
 * (every fault read the original when it was constructed).  A Request in transit keeps its delay.  A graph with a link fault reads the
 * link's LOSS stream one value per draw (a Request that meets a rate of 0 draws nothing) and runs an eighth instantiation of the loop
 * (it carries the code of all the others).  Before the first run (HS_E_STATE afterwards).
 * hs_graph_get_link_faults, per node (any may be NULL): the place -- among all hs_graph_add_fault / hs_graph_add_link_fault calls, from
 * 0 -- of the latency / loss activation in force on a link (-1: none, or no link), and the values the link has read from its LOSS
 * stream. */
typedef enum hs_link_fault { HS_LINK_FAULT_LATENCY = 1, HS_LINK_FAULT_LOSS = 2 } hs_link_fault;
int hs_graph_add_link_fault(hs_graph *g, int32_t link_node, int64_t time_ns, int32_t what, int32_t on, double value, int32_t cancelled);
int hs_graph_get_link_faults(hs_graph *g, int32_t *active_latency, int32_t *active_loss, int64_t *loss_draws);
/* Backend health: HealthChecker (components/load_balancer/health_check.py) and LoadBalancer.mark_unhealthy / mark_healthy
 * (load_balancer.py:244-297).  A graph with a configured checker, or with initial health flags, runs an instantiation of the loop of
 * its own; `_forward_request` then selects over the healthy backends in registration order (RoundRobin, LeastConnections,
 * WeightedLeastConnections; WeightedRoundRobin as the live smooth-weighted algorithm with per-backend current weights that persist
 * while a backend is out, strategies.py:111-134).  ConsistentHash, IPHash and Random are refused (HS_E_UNSUPPORTED) under a checker or
 * with an unhealthy backend.
 *
 * hs_graph_set_health_checker: node `node` (HS_NODE_HEALTH_CHECKER) checks the backends of LoadBalancer `lb_node` every `interval_s`
 * with `timeout_s` per check; the reference's own ValueErrors as HS_E_INVALID with its texts; a second checker on one LoadBalancer:
 * HS_E_UNSUPPORTED.  `running`: `_is_running` when the run begins (start() sets it, stop() clears it).  hs_graph_schedule on the
 * checker node is the `_health_check_cycle` Event start() returns, numbered in call order with the other scheduled entries.  Three
 * more internal kinds -- the cycle, a check's response, its timeout -- are aimed at the checker itself (dropped while it is crashed,
 * after which its cycle chain has ended and the backends stay `is_checking`); a probe is a Request of the backend in every respect
 * (queue capacity, stats_accepted, service draw, downstream, Sink record with created_at = its own time), its response is pushed when
 * the backend's enqueue handler returns, a probe at a crashed backend is dropped and only its timeout comes.
 * hs_graph_set_lb_health: healthy[n] = BackendInfo.is_healthy of the LoadBalancer's `n` backends when the run begins.
 * Both before the first run (HS_E_STATE afterwards). */
int hs_graph_set_health_checker(hs_graph *g, int32_t node, int32_t lb_node, double interval_s, double timeout_s, int32_t healthy_threshold,
                                int32_t unhealthy_threshold, int32_t running);
int hs_graph_set_lb_health(hs_graph *g, int32_t node, const uint8_t *healthy, int32_t n);
/* After a run, for `node` a HealthChecker or a LoadBalancer (any output may be NULL):
 *   checker_stats[6]  HealthCheckStats in field order: performed, passed, failed, timed out, marked healthy, marked unhealthy (zeros for a LoadBalancer node);
 *   backend_states[6 * n_backends]  per backend of the LoadBalancer: consecutive_successes, consecutive_failures, last_check_time ns (-1: None),
 *                     last_check_passed (-1: None), is_checking, the pending check id (0: none);
 *   healthy[n_backends]  BackendInfo.is_healthy;  marks[2]  the LoadBalancer's backends_marked_unhealthy / _healthy of the run;
 *   events[3]         the graph's cycle / response / timeout Events, counted like events_by_kind counts the public kinds:
 *                     events_processed == sum(events_by_kind) + sum(internal_by_kind of hs_graph_get_faults) + sum(events).
 * node = -1 with every other output NULL: the event counts alone. */
int hs_graph_get_health(hs_graph *g, int32_t node, int64_t *checker_stats, int64_t *backend_states, uint8_t *healthy, int64_t *marks, int64_t *events);
/* WeightedRoundRobin._current_weights of the LoadBalancer's `n` backends after a run with health state: returns 1 and fills `out`
 * and, if not NULL, present[n] = the dict has an entry for the backend (it was healthy at one selection at least, strategies.py:117-119);
 * 0 when the graph has none (the periodic table ran: the weights follow from the selection counts); negative: an hs_status. */
int64_t hs_graph_get_lb_current_weights(hs_graph *g, int32_t node, int64_t *out, uint8_t *present, int32_t n);
/* Client-side guards: Bulkhead and TimeoutWrapper (components/resilience/bulkhead.py, timeout.py).  A graph that holds one runs a
 * fourth instantiation of the loop (it carries the fault and health code too).  A Request at a wrapper is forwarded as a NEW Event
 * for `target` with the wrapper's completion hook; the hook's `_bh_response` / `_tw_response` Event is constructed when the handler
 * that receives the forwarded Event returns -- a Server's enqueue (accepted or refused), a Sink, a RandomRouter, a RateLimitedEntity's
 * request handler, a NetworkLink at the end of transit (at once on a lost packet) -- behind that handler's own Events.  A NetworkLink
 * leaves the hook on the Event it constructs for its egress, so the egress' handler fires it a second time (link.py:181): the second
 * response finds no id and is a processed no-op, as in the reference.  An Event aimed at a crashed entity is dropped before any handler
 * runs: no hook fires, a Bulkhead's permit leaks, a TimeoutWrapper's id waits for its timeout.  Six more internal kinds -- request,
 * response, timeout of a Bulkhead, then of a TimeoutWrapper -- are aimed at the wrapper itself (dropped while it is crashed); they count
 * in hs_summary.events_processed, not in events_by_kind.
 * Refused (HS_E_UNSUPPORTED): a wrapper whose target is, directly or through a chain of NetworkLinks, a LoadBalancer, a Bulkhead or a
 * TimeoutWrapper (two hooks on one Event); Bulkhead.max_concurrent above HS_BULKHEAD_MAX_CONCURRENT.
 *
 * hs_graph_set_wrapper: the parameters of node `node`.  A Bulkhead takes max_concurrent, max_wait_queue and max_wait_time_s (negative:
 * None); a TimeoutWrapper takes timeout_s and table_capacity, the request ids its in-flight table holds at first (0: 256) -- a full
 * table stops the launch in front of the Request, the host doubles it and the run goes on, nothing is ever dropped.  The reference's own
 * ValueErrors as HS_E_INVALID with its texts.  Before the first run (HS_E_STATE afterwards); every wrapper node is configured before a
 * run (HS_E_STATE otherwise). */
#define HS_BULKHEAD_MAX_CONCURRENT 65536
#define HS_WRAPPER_COUNTERS 12
int hs_graph_set_wrapper(hs_graph *g, int32_t node, int32_t max_concurrent, int32_t max_wait_queue, double max_wait_time_s, double timeout_s,
                         int32_t table_capacity);
/* After a run, for `node` a Bulkhead or a TimeoutWrapper (any output may be NULL):
 *   counters[HS_WRAPPER_COUNTERS]  Bulkhead: total, accepted, rejected, timed_out, queued requests, peak_concurrent, peak_queue_depth,
 *                     active_count, queue_depth, _next_request_id, len(_in_flight), the table's capacity;
 *                     TimeoutWrapper: total, successful, timed_out, five zeros, 0, _next_request_id, len(_in_flight), the table's capacity;
 *   queue_ids[min(queue_depth, queue_cap)]  the request ids of a Bulkhead's wait queue, head first;
 *   in_flight_ids[min(len(_in_flight), in_flight_cap)]  the ids in flight, in no particular order;
 *   events[6]         the graph's Bulkhead request / response / timeout and TimeoutWrapper request / response / timeout Events, counted
 *                     like events_by_kind counts the public kinds: events_processed == sum(events_by_kind) + sum(internal_by_kind of
 *                     hs_graph_get_faults) + sum(events of hs_graph_get_health) + sum(events).
 * node = -1 with the three node outputs NULL: the event counts alone. */
int hs_graph_get_wrapper(hs_graph *g, int32_t node, int64_t *counters, int64_t *queue_ids, int64_t queue_cap, int64_t *in_flight_ids,
                         int64_t in_flight_cap, int64_t *events);
/* Client with timeouts and retry policies (components/client/client.py, retry.py).  A graph that holds one runs a fifth
 * instantiation of the loop (it carries the fault, health and wrapper code too).  Every Event that reaches a Client and is neither its
 * `_client_response` nor its `_client_timeout` is an outgoing request: `_in_flight[(request_id, attempt)]` is set (an equal key is
 * overwritten), a NEW Event for `target` is constructed -- its context is the metadata alone, so `created_at` downstream is the send
 * time of THIS attempt and no client id survives -- with the Client's completion hook, then the timeout Event at now + timeout.  The
 * hook fires where a wrapper's fires (see above; twice behind a NetworkLink, never at a crashed target).  A response of a key in
 * flight removes it and appends now - start_time to the response times; a timeout of a key in flight removes it and, while
 * attempt < max_attempts, constructs the retry -- a request at the Client with attempt + 1 -- at now + delays_ns[attempt - 1];
 * otherwise it counts a failure.  A Request from a Source, a Server, a link, a router, a limiter or hs_graph_schedule has no request_id:
 * all of them share the keys (None, attempt), as in the reference.  Three more internal kinds -- request, response, timeout -- are
 * aimed at the Client itself (dropped while it is crashed); they count in hs_summary.events_processed, not in events_by_kind.
 * Refused (HS_E_UNSUPPORTED): a Client whose target is, directly or through a chain of NetworkLinks, a LoadBalancer, a Bulkhead, a
 * TimeoutWrapper or a Client, and a wrapper whose target is a Client (two hooks on one Event); more than HS_CLIENT_MAX_ATTEMPTS
 * attempts.
 *
 * hs_graph_set_client: timeout_s (negative: None; 0 is legal), the policy's delays in whole nanoseconds for attempt 1 ..
 * max_attempts - 1 (n_delays = max_attempts - 1; NoRetry: 0) -- the host evaluates Duration.from_seconds(policy.get_delay(a)), the
 * device never does -- and table_capacity, the keys the in-flight table holds at first (0: 256; it doubles on demand like a
 * TimeoutWrapper's, nothing is ever dropped).  The reference's own ValueErrors as HS_E_INVALID with its texts.  Before the first run
 * (HS_E_STATE afterwards); every Client node is configured before a run (HS_E_STATE otherwise). */
#define HS_CLIENT_MAX_ATTEMPTS 65536
#define HS_CLIENT_COUNTERS 7
int hs_graph_set_client(hs_graph *g, int32_t node, double timeout_s, const int64_t *delays_ns, int32_t n_delays, int32_t table_capacity);
/* An Event aimed at Client `node` with metadata request_id = `request_id` (1 .. 2^30 - 1; 0: none, which is what hs_graph_schedule on a
 * Client node schedules) and attempt 1 -- Client.send_request's Event.  Numbered in call order with the other scheduled entries. */
int hs_graph_schedule_client(hs_graph *g, int32_t node, int64_t time_ns, int32_t request_id);
/* After a run, for `node` a Client (any output may be NULL):
 *   counters[HS_CLIENT_COUNTERS]  requests_sent, responses_received, timeouts, retries, failures, len(_in_flight), the table's capacity;
 *   in_flight_keys[2 * min(len(_in_flight), cap)]  (request_id or 0, attempt) of every key in flight, in no particular order;
 *   events[3]         the graph's Client request / response / timeout Events: events_processed == sum(events_by_kind) + the internal
 *                     kinds of hs_graph_get_faults, hs_graph_get_health, hs_graph_get_wrapper + sum(events).
 * node = -1 with the two node outputs NULL: the event counts alone.  The response times are rows of the record log
 * (hs_graph_read_records): node = the Client, t = the response time in ns, value = start_time in ns, in the order they were appended. */
int hs_graph_get_client(hs_graph *g, int32_t node, int64_t *counters, int64_t *in_flight_keys, int64_t cap, int64_t *events);
/* BatchProcessor, ConveyorBelt and GateController (components/industrial/batch_processor.py, conveyor.py, gate_controller.py): the
 * stations that hold Requests back and release them together.  A graph that holds one runs a sixth instantiation of the loop (it
 * carries the fault, health, wrapper and Client code too).  Eight more internal kinds, in this order: a Request at a BatchProcessor,
 * its `_BatchTimeout`, the continuation of a batch in process; a Request at a ConveyorBelt, the continuation of its transit; a Request
 * at a GateController, its `_GateOpen`, its `_GateClose`.  They count in hs_summary.events_processed, not in events_by_kind.  The
 * two continuations resume a generator and are never dropped; the other six are aimed at the entity and are dropped while it is
 * crashed or paused.  Every forwarded Event is a NEW Event with the item's context (created_at survives) and no completion hook.
 *   BatchProcessor: an item joins the buffer; the first item of an empty buffer with a timeout constructs the `_BatchTimeout` Event at
 *     now + timeout_ns and nothing else; otherwise len(buffer) >= batch_size starts a batch: the buffer becomes the batch, the pending
 *     timeout is cancelled (its entry stays in the heap, is popped without being processed and counts as cancelled), and after
 *     process_ns every item goes downstream in buffer order, in ONE handler.  Several batches may be in process at once.
 *   ConveyorBelt: at capacity (> 0) the item is rejected; otherwise it is in transit for transit_ns, then goes downstream.
 *   GateController: open, an item passes at once; closed, it joins the queue, or is rejected when queue_capacity (> 0) items wait.
 *     `_GateOpen` on a closed gate forwards the whole queue in FIFO order in ONE handler.  Gate Events are daemons.
 * A handler that releases N items is only entered once the heap has room for all N (the run stops in front of the Event and the heap
 * grows, as for any other Event): a release is never partial.  The delays are whole nanoseconds the host computed
 * (int(seconds * 1e9), core/temporal.py:222): they do not depend on `now`.
 *
 * hs_graph_set_flow, before the first run (HS_E_STATE afterwards; every such node is configured before a run):
 *   BatchProcessor  count = batch_size (1 .. HS_FLOW_MAX_ITEMS), delay_ns = process_time, aux_ns = timeout (<= 0: none), flag unused
 *   ConveyorBelt    count = capacity (<= 0: unlimited), delay_ns = transit_time
 *   GateController  count = queue_capacity (<= 0: unbounded; at most HS_FLOW_MAX_ITEMS), flag = is_open when the run begins,
 *                   aux_ns = open_cycles counted so far (GateController.open() on the host before the run), no time
 * The reference's own ValueErrors as HS_E_INVALID with its texts. */
#define HS_FLOW_MAX_ITEMS (1 << 20)
#define HS_FLOW_COUNTERS 8
#define HS_FLOW_KINDS 8
int hs_graph_set_flow(hs_graph *g, int32_t node, int64_t count, int64_t delay_ns, int64_t aux_ns, int32_t flag);
/* A `_GateOpen` (open != 0) or `_GateClose` Event for GateController `node` -- one Event of GateController.start_events(), a daemon --
 * numbered in call order with the other scheduled entries. */
int hs_graph_schedule_gate(hs_graph *g, int32_t node, int64_t time_ns, int32_t open);
/* After a run, for `node` one of the three (any output may be NULL):
 *   counters[HS_FLOW_COUNTERS]  BatchProcessor: batches_processed, items_processed, timeouts, buffer_depth, 0, 0, 0, 0
 *                               ConveyorBelt:   items_transported, items_rejected, items_in_transit, 0 ...
 *                               GateController: passed_through, queued_while_closed, rejected, open_cycles, queue_depth, is_open, 0, 0
 *   events[HS_FLOW_KINDS]       the graph's Events of the eight kinds above; events_processed == sum(events_by_kind) + the internal kinds
 *                               of hs_graph_get_faults, _health, _wrapper, _client + sum(events)
 *   cancelled                   `_BatchTimeout` Events popped after their batch had started (events_cancelled counts them).
 * node = -1 with counters NULL: the graph's counts alone. */
int hs_graph_get_flow(hs_graph *g, int32_t node, int64_t *counters, int64_t *events, int64_t *cancelled);
/* A Server's queue policy other than the FIFO (components/queue_policy.py LIFOQueue, components/queue_policies/adaptive_lifo.py
 * AdaptiveLIFO, codel.py CoDelQueue).  A graph that holds such a Server runs a seventh instantiation of the loop (it carries the
 * fault, health, wrapper, Client and flow code too); its other Servers keep the FIFO path.  No new Event kinds: the policy changes what
 * HS_EV_ENQUEUE pushes and what HS_EV_POLL pops, events_by_kind and events_processed keep their meaning.
 *   LIFO          push appends and refuses at capacity; pop takes the newest item.
 *   AdaptiveLIFO  push likewise (capacity_rejected / enqueued); pop evaluates len >= congestion_threshold BEFORE it removes anything,
 *                 counts a mode switch when that differs from the last pop's, then takes the newest (dequeued_lifo) or the oldest
 *                 (dequeued_fifo) item.
 *   CoDel         push stamps the item with `now`; pop removes the head, computes its sojourn time and runs the reference's
 *                 `_codel_dequeue` operation for operation in binary64 (correctly rounded division and square root, from_seconds
 *                 truncates): the popped item is always delivered, the items it drops behind it go back to the free list and reach no
 *                 handler (their completion hook fired when they were enqueued).
 * hs_graph_set_queue_policy, before the first run (HS_E_STATE afterwards), once per Server: capacity < 0 is unbounded and replaces the
 * node's queue_cap; threshold is read for HS_QUEUE_ADAPTIVE_LIFO, target_s / interval_s for HS_QUEUE_CODEL.  The reference's own
 * ValueErrors as HS_E_INVALID with its texts.
 * hs_graph_get_queue_policy, out[HS_QUEUE_FIELDS]: policy, len, enqueued, dequeued (CoDel) / dequeued_fifo, dequeued_lifo, dropped,
 *   capacity_rejected, mode_switches (AdaptiveLIFO) / drop_intervals (CoDel), _was_congested / _dropping, _count, _last_count,
 *   _first_above_time is set, its ns, _drop_next is set, its ns, 0. */
typedef enum hs_queue_policy { HS_QUEUE_FIFO = 0, HS_QUEUE_LIFO = 1, HS_QUEUE_ADAPTIVE_LIFO = 2, HS_QUEUE_CODEL = 3 } hs_queue_policy;
#define HS_QUEUE_FIELDS 16
int hs_graph_set_queue_policy(hs_graph *g, int32_t node, int32_t policy, int64_t capacity, int64_t threshold, double target_s, double interval_s);
int hs_graph_get_queue_policy(hs_graph *g, int32_t node, int64_t *out);
/* AutoScaler (components/deployment/auto_scaler.py): a periodic controller that adds Servers to a LoadBalancer's backends and removes
 * them again during the run.  The instances it may add are a POOL of dormant Server nodes: the last `n_pool` targets of the
 * LoadBalancer (its initial backends stand in front of them), instance k = pool target k - 1.  A LoadBalancer with a scaler keeps a
 * membership word per target next to the health flag; `_forward_request` selects over the members in list order (the path of the
 * health lowering: RoundRobin, the live WeightedRoundRobin, LeastConnections, WeightedLeastConnections; the other strategies:
 * HS_E_UNSUPPORTED).  A graph with a scaler runs an instantiation of the loop of its own.
 *
 * hs_graph_set_auto_scaler, before the first run (HS_E_STATE afterwards), once per scaler node: `policy` with its parameters --
 * HS_AUTOSCALER_TARGET_UTILIZATION: p0 = target; HS_AUTOSCALER_QUEUE_DEPTH: p0 / p1 = scale_out / scale_in threshold;
 * HS_AUTOSCALER_STEP: n_steps (at most HS_AUTOSCALER_MAX_STEPS) pairs step_threshold[k] / step_adjustment[k] in the order the
 * reference evaluates them --, the limits, the interval and the two cooldowns in seconds, the LoadBalancer node, the pool's size and
 * `running` (`_is_running` when the run begins).  A second scaler on one LoadBalancer, a scaler next to a HealthChecker on it and an
 * initially unhealthy backend under a scaler: HS_E_UNSUPPORTED.  hs_graph_schedule on the scaler node is the daemon
 * `_autoscaler_evaluate` Event start() returns.  The handler restates _evaluate / _in_cooldown / _try_scale_out / _try_scale_in; a
 * scale-out that needs an instance beyond the pool ends the run with HS_E_OVERFLOW and a message that names the scaler.
 *
 * hs_graph_get_auto_scaler, after a run (any output may be NULL): state[HS_AUTOSCALER_FIELDS] = evaluations, scale_out_count,
 * scale_in_count, instances_added, instances_removed, cooldown_blocks, _next_instance_id, _last_scale_action (0 None, 1 scale_out,
 * 2 scale_in), _last_scale_time ns, records in the scaling history, members of the LoadBalancer, 0; history[4 * min(records,
 * history_cap)] = (time ns, action + 4 x the instances it counted, from_count, to_count) per ScalingEvent; member[n targets of the LoadBalancer] = the membership
 * word of every target; *events = the graph's `_autoscaler_evaluate` Events: events_processed == sum(events_by_kind) + the other
 * internal kinds + *events.  node = -1 with every other output NULL: the event count alone. */
typedef enum hs_autoscaler_policy { HS_AUTOSCALER_TARGET_UTILIZATION = 0, HS_AUTOSCALER_STEP = 1, HS_AUTOSCALER_QUEUE_DEPTH = 2 } hs_autoscaler_policy;
#define HS_AUTOSCALER_MAX_STEPS 16
#define HS_AUTOSCALER_MAX_POOL 4096
#define HS_AUTOSCALER_FIELDS 12
int hs_graph_set_auto_scaler(hs_graph *g, int32_t node, int32_t lb_node, int32_t policy, double p0, double p1, int32_t n_steps,
                             const double *step_threshold, const int32_t *step_adjustment, int32_t min_instances, int32_t max_instances,
                             double interval_s, double scale_out_cooldown_s, double scale_in_cooldown_s, int32_t n_pool, int32_t running);
int hs_graph_get_auto_scaler(hs_graph *g, int32_t node, int64_t *state, int64_t *history, int64_t history_cap, uint8_t *member, int64_t *events);
/* RollingDeployer (components/deployment/rolling_deployer.py): replaces the backends of a LoadBalancer batch by batch with new
 * instances, probing every new instance until it has passed `healthy_threshold` health checks, and rolls back after more than
 * `max_failures` failed ones.  The instances are a POOL of dormant Server nodes as an AutoScaler's are: the last `n_pool` targets of the
 * LoadBalancer, instance k = pool target k - 1.  Unlike a scaler a deployer removes INITIAL backends, can re-add one behind newer
 * instances and can empty the list, so the LoadBalancer's members are an ordered list of slots in insertion order (`all_backends` is a
 * dict's order): adding appends, removing keeps the order of the rest.  A re-added backend starts with total_requests 0 and weight 1
 * (add_backend's BackendInfo and set_weight).  RoundRobin, the live WeightedRoundRobin, LeastConnections and WeightedLeastConnections
 * select over that list on the lone lane; the other strategies: HS_E_UNSUPPORTED.  A graph with a deployer runs an instantiation of
 * the loop of its own.
 *
 * hs_graph_set_rolling_deployer, before the first run (HS_E_STATE afterwards), once per deployer node: the LoadBalancer node, batch_size
 * (>= 1), health_check_interval in seconds (>= 1 ns, finite), healthy_threshold (>= 1), max_failures and the pool's size (at most
 * HS_DEPLOYER_MAX_POOL).  A second deployer on one LoadBalancer, a deployer next to an AutoScaler or a HealthChecker on it and an
 * initially unhealthy backend under a deployer: HS_E_UNSUPPORTED.  hs_graph_schedule on the deployer node is the
 * `_rolling_deploy_start` Event deploy() returns (no daemon).  The handlers restate _start_deployment, _replace_batch,
 * _run_health_check, _handle_health_pass, _handle_health_timeout, _rollback and _complete; a probe is a Request of the new Server whose
 * completion hook names the deployer.  A batch that needs an instance beyond the pool ends the run with HS_E_OVERFLOW and a message
 * that names the deployer.
 *
 * hs_graph_get_rolling_deployer, after a run (any output may be NULL), B = the LoadBalancer's targets: state[HS_DEPLOYER_FIELDS] =
 * deployments_started, deployments_completed, deployments_rolled_back, instances_replaced, health_checks_performed,
 * health_checks_passed, health_checks_failed, state.status (hs_deployment_status), total_instances, replaced, failed, current_batch,
 * _next_instance_id, _health_fail_count, len(_old_backends), len(_new_backends), len(_current_batch_old), len(_current_batch_new),
 * members of the LoadBalancer, 0; lists[4 * B] = _old_backends, _new_backends, _current_batch_old, _current_batch_new as slots of the
 * LoadBalancer, B places each, -1 behind a list's end; members[B] = the LoadBalancer's members IN ORDER, -1 behind the end; pass[B] =
 * _health_pass_count by slot (-1: the name has no entry); readded[B] = 1 for a backend a rollback added again (its BackendInfo is a
 * new one: weight 1, total_requests from 0); events[HS_DEPLOYER_KINDS + 2] = the graph's deployer Events by kind (start,
 * replace_batch, health_check, health_pass, health_timeout, rollback, complete): events_processed == sum(events_by_kind) + the other
 * internal kinds + sum(events[0 .. 6]); behind them events[7] / events[8] = the member lists the graph compacted behind a removal on
 * the lone lane / with all 64 lanes (from 32 members on the 64 lanes compact the list by membership, a ballot and a prefix count per
 * chunk of 64 entries, order kept; hs_debug_graph_flags bit 0 keeps every compaction on the lone lane, bit 1 hands every one to the
 * wavefront; both leave the same list).  node = -1 with every other output NULL: the event counts alone. */
typedef enum hs_deployment_status { HS_DEPLOYMENT_IDLE = 0, HS_DEPLOYMENT_IN_PROGRESS = 1, HS_DEPLOYMENT_COMPLETED = 2, HS_DEPLOYMENT_ROLLED_BACK = 3 } hs_deployment_status;
#define HS_DEPLOYER_KINDS 7
#define HS_DEPLOYER_MAX_POOL 4096
#define HS_DEPLOYER_FIELDS 20
int hs_graph_set_rolling_deployer(hs_graph *g, int32_t node, int32_t lb_node, int32_t batch_size, double interval_s, int32_t healthy_threshold,
                                  int64_t max_failures, int32_t n_pool);
int hs_graph_get_rolling_deployer(hs_graph *g, int32_t node, int64_t *state, int32_t *lists, int32_t *members, int32_t *pass, int32_t *readded,
                                  int64_t *events);
/* CanaryDeployer (components/deployment/canary_deployer.py): ONE new instance `{name}_canary` joins a LoadBalancer -- its last target,
 * a dormant Server like a rolling deployer's pool of one --, the strategy's weights are rewritten stage by stage
 * (`_set_traffic_weight`: max(1, int(pct * 100)) for the canary, max(1, int((1.0 - pct) * 100 / num_baseline)) for every baseline
 * backend, in binary64 with separate roundings; all 1 from pct >= 1.0 on; nothing without a baseline; a no-op unless the strategy is
 * WeightedRoundRobin or WeightedLeastConnections), every `evaluation_interval` the evaluator compares the canary with the baseline's
 * plain left-to-right average, and the deployment ends with a promotion -- the whole baseline leaves in one compaction pass, every
 * remaining member's weight becomes 1 -- or a rollback (the canary leaves, the weights likewise).  The member list is the ordered one
 * of a deployed LoadBalancer (see above); a graph with a canary deployer runs the deployers' instantiation and keeps, per node, the
 * Servers' `_service_times` as a running binary64 sum and a count taken at the draw.
 *
 * hs_graph_set_canary_deployer, before the first run (HS_E_STATE afterwards), once per deployer node: the LoadBalancer node, n_stages
 * (1 .. HS_CANARY_MAX_STAGES) pairs traffic_percentage[k] / evaluation_period[k] (finite), the evaluator -- HS_CANARY_ERROR_RATE:
 * requests_rejected / (requests_completed + requests_rejected), ev_max = max_error_rate; HS_CANARY_LATENCY: the mean of the service
 * times drawn so far, ev_max = max_latency --, its threshold_multiplier and the interval in seconds.  A second deployer on one
 * LoadBalancer, a deployer next to an AutoScaler or a HealthChecker on it, an initially unhealthy backend: HS_E_UNSUPPORTED.
 * hs_graph_schedule on the deployer node is the `_canary_deploy_start` Event deploy() returns (no daemon); one per deployer.
 *
 * hs_graph_get_canary_deployer, after a run (any output may be NULL), B = the LoadBalancer's targets: state[HS_CANARY_FIELDS] =
 * deployments_started, deployments_completed, deployments_rolled_back, stages_completed, evaluations_performed, evaluations_passed,
 * evaluations_failed, state.status (hs_canary_status), current_stage, total_stages, 1 if `canary` is set, _stage_start_time ns (-1:
 * None), len(_baseline_backends), members of the LoadBalancer, 0, 0; *traffic_pct = state.canary_traffic_pct; baseline[B] =
 * _baseline_backends as slots, -1 behind the end; members[B] = the LoadBalancer's members IN ORDER; weights[B] = the strategy's weight
 * of every slot now; weight_set[B] = 1 where set_weight was called for the slot during the run; service_sum[B] / service_count[B] = the
 * sum and count of every target's service times; events[HS_CANARY_KINDS] = the graph's canary Events by kind (start, stage_start,
 * evaluate, promote, rollback, complete).  node = -1: the event counts alone. */
typedef enum hs_canary_status { HS_CANARY_IDLE = 0, HS_CANARY_IN_PROGRESS = 1, HS_CANARY_PROMOTING = 2, HS_CANARY_ROLLED_BACK = 3, HS_CANARY_COMPLETED = 4 } hs_canary_status;
typedef enum hs_canary_evaluator { HS_CANARY_ERROR_RATE = 0, HS_CANARY_LATENCY = 1 } hs_canary_evaluator;
#define HS_CANARY_KINDS 6
#define HS_CANARY_MAX_STAGES 16
#define HS_CANARY_FIELDS 16
int hs_graph_set_canary_deployer(hs_graph *g, int32_t node, int32_t lb_node, int32_t n_stages, const double *traffic_percentage,
                                 const double *evaluation_period, int32_t evaluator, double ev_max, double ev_multiplier, double interval_s);
int hs_graph_get_canary_deployer(hs_graph *g, int32_t node, int64_t *state, double *traffic_pct, int32_t *baseline, int32_t *members,
                                 int32_t *weights, int32_t *weight_set, double *service_sum, int64_t *service_count, int64_t *events);
/* Hedge and Fallback (components/resilience/hedge.py, fallback.py): the two wrappers that send a Request a SECOND time.  A graph that
 * holds one runs an eleventh instantiation of the loop (it carries the code of all the others).  Seven more internal kinds, in this
 * order -- a Request at a Hedge, its `_hg_response`, its `_hg_send_hedge`; a Request at a Fallback, its `_fb_primary_response`, its
 * `_fb_timeout`, its `_fb_fallback_response` -- are aimed at the wrapper itself (dropped while it is crashed or paused); they count in
 * hs_summary.events_processed, not in events_by_kind.
 *   Hedge: a Request takes id ++_next_request_id, its entry is stored with a copy of the Request's context (created_at, the client
 *     key), a NEW Event for `target` at `now` is constructed with the Hedge's hook, then `_hg_send_hedge` number 1 at now +
 *     hedge_delay_ns.  `_hg_send_hedge`: an unknown id is a processed no-op; a completed entry counts hedges_cancelled; an entry with
 *     hedges_sent >= max_hedges does nothing; otherwise a duplicate Request is built FROM THE ENTRY (a fresh Request of the pool) and,
 *     while its number < max_hedges, the next `_hg_send_hedge`.  `_hg_response` carries is_hedge: responses_received += 1, the first
 *     one decides primary_wins / hedge_wins, and the entry leaves once responses_received >= 1 + hedges_sent at that moment.
 *   Fallback: a Request takes an id, its entry is stored in state "primary", a NEW Event for the primary is constructed with the hook,
 *     then, with a timeout, `_fb_timeout` at now + timeout_ns.  `_fb_primary_response` in state "primary" deletes the entry
 *     (primary_successes); `_fb_timeout` in state "primary" counts primary_failures and fallback_invocations, the state becomes
 *     "fallback" and a NEW Event for the fallback entity is built from the entry with the `_fb_fallback_response` hook;
 *     `_fb_fallback_response` in state "fallback" deletes the entry (fallback_successes).  Everything else is a processed no-op;
 *     fallback_failures is never incremented by the reference.
 * The hooks fire where a TimeoutWrapper's fire (above; twice behind a NetworkLink, never at a crashed or paused target: such an entry
 * stays for ever).  The in-flight table of a wrapper lives in device memory of its own: open addressing on the id (ids ascend and are
 * never reused), kept at most half full.
 * Refused (HS_E_UNSUPPORTED): a target, primary or fallback entity that is, directly or through a chain of NetworkLinks, a LoadBalancer,
 * Bulkhead, TimeoutWrapper, Client, Hedge or Fallback (two hooks on one Event) or a BatchProcessor, ConveyorBelt or GateController; a
 * Bulkhead, TimeoutWrapper or Client whose target is a Hedge or a Fallback; max_hedges above HS_HEDGE_MAX_HEDGES.
 *
 * hs_graph_set_hedge / hs_graph_set_fallback: the delays in whole nanoseconds (the host evaluates Duration.from_seconds; timeout_ns < 0:
 * None, the fallback entity is never invoked) and table_capacity, the entries the table holds at first (0: 256) -- a full table stops
 * the launch in front of the Request, the host doubles it and the run goes on, nothing is ever dropped; beyond HS_HEDGE_MAX_IN_FLIGHT
 * entries the run ends with HS_E_OVERFLOW naming the wrapper.  Before the first run (HS_E_STATE afterwards); every such node is
 * configured before a run (HS_E_STATE otherwise). */
#define HS_HEDGE_MAX_HEDGES 65535
#define HS_HEDGE_MAX_IN_FLIGHT (1 << 20)
#define HS_HEDGE_KINDS 7
#define HS_HEDGE_COUNTERS 8
#define HS_FALLBACK_COUNTERS 9
int hs_graph_set_hedge(hs_graph *g, int32_t node, int64_t hedge_delay_ns, int32_t max_hedges, int32_t table_capacity);
int hs_graph_set_fallback(hs_graph *g, int32_t node, int32_t fallback_node, int64_t timeout_ns, int32_t table_capacity);
/* After a run, for `node` a Hedge (any output may be NULL):
 *   counters[HS_HEDGE_COUNTERS]  total_requests, primary_wins, hedge_wins, hedges_sent, hedges_cancelled, _next_request_id,
 *                     len(_in_flight), the table's capacity;
 *   entries[5 * min(len(_in_flight), cap)]  per entry in flight, in no particular order: id, start_time ns, completed, hedges_sent,
 *                     responses_received;
 *   events[HS_HEDGE_KINDS]  the graph's Hedge request / response / send-hedge and Fallback request / primary-response / timeout /
 *                     fallback-response Events: events_processed == sum(events_by_kind) + every other family's internal counts + sum(events).
 * node = -1 with the two node outputs NULL: the event counts alone. */
int hs_graph_get_hedge(hs_graph *g, int32_t node, int64_t *counters, int64_t *entries, int64_t cap, int64_t *events);
/* ... for `node` a Fallback:
 *   counters[HS_FALLBACK_COUNTERS]  total_requests, primary_successes, primary_failures, fallback_invocations, fallback_successes,
 *                     fallback_failures, _next_request_id, len(_in_flight), the table's capacity;
 *   entries[3 * min(len(_in_flight), cap)]  id, start_time ns, state (0 "primary", 1 "fallback");
 *   events[HS_HEDGE_KINDS]  as above. */
int hs_graph_get_fallback(hs_graph *g, int32_t node, int64_t *counters, int64_t *entries, int64_t cap, int64_t *events);
/* PooledCycleResource and InventoryBuffer (components/industrial/pooled_cycle.py, inventory.py) on HS_NODE_POOLED_CYCLE /
 * HS_NODE_INVENTORY nodes: the twelfth level of the single-heap loop, four more internal Event kinds (60 .. 63 of the 64 the kind word
 * holds): a Request at a pool, the end of a cycle (a generator's continuation: never dropped), a consume Request at a buffer, its
 * `_InventoryReplenish`.  Neither draws a random number.
 *   PooledCycleResource: a Request that finds a unit free takes it (available -= 1, active += 1) and its continuation is constructed
 *     at now + cycle_ns; otherwise it is rejected when queue_capacity > 0 and the line is that long, or appended to the line
 *     (queue_capacity = 0: unbounded).  The continuation releases the unit, counts `completed`, forwards the Request to `target` with
 *     its context (no target: the Request ends there) and, when the line is not empty, re-sends its head to the pool ITSELF as a NEW
 *     Event at `now`: it goes through the heap with a fresh sort index, so an arrival of the same nanosecond that sorts ahead of it
 *     takes the unit and the re-sent Request queues again at the back; a crashed pool drops it like any arrival.
 *   InventoryBuffer: a consume takes one item (stock -= 1, items_consumed += 1, a NEW Event for `target`) or counts a stock-out (a NEW
 *     Event for the stock-out target); then, when stock <= reorder_point and no order is pending, `reorders` += 1 and
 *     `_InventoryReplenish` is constructed at from_seconds(to_seconds(now) + lead_time_s) -- a binary64 sum of seconds, truncated to
 *     nanoseconds --, behind the forward.  The replenish adds order_quantity and clears the pending flag; one that a crashed buffer
 *     drops leaves the flag set for ever.
 * No completion hook reaches either of them: refused (HS_E_UNSUPPORTED) as a LoadBalancer's backend and as the target, primary or
 * fallback entity -- directly or through NetworkLinks -- of a Bulkhead, TimeoutWrapper, Client, Hedge or Fallback.
 *
 * hs_graph_set_pool: pool_size in [1, HS_POOL_MAX_UNITS], cycle_ns = int(cycle_time * 1e9) >= 0 (what `Instant + seconds` adds),
 * queue_capacity in [0, HS_POOL_MAX_UNITS] (0: unbounded).  hs_graph_set_inventory: initial_stock, reorder_point >= 0 and
 * order_quantity > 0, each at most HS_INVENTORY_MAX (2^62) and reorder_point + order_quantity at most HS_INVENTORY_MAX_LEVEL -- the stock
 * never passes max(initial_stock, reorder_point + order_quantity), an order being placed only at or below the reorder point and one at a
 * time, and items_replenished never passes that plus the items consumed, so both stay inside int64 for any run of fewer than 2^48
 * Events (HS_E_UNSUPPORTED beyond: the reference's integers are unbounded) --, lead_time_s finite and >= 0, stockout_node = -1 or a node
 * that takes Requests.  Before the first run (HS_E_STATE afterwards); every such node is configured before a run (HS_E_STATE otherwise). */
#define HS_POOL_MAX_UNITS (1 << 20)
#define HS_INVENTORY_MAX (1ll << 62)
#define HS_INVENTORY_MAX_LEVEL 0x7fff000000000000ll   /* 2^63 - 2^48 */
#define HS_STOCK_KINDS 4
#define HS_POOL_COUNTERS 5
#define HS_INVENTORY_COUNTERS 6
int hs_graph_set_pool(hs_graph *g, int32_t node, int32_t pool_size, int64_t cycle_ns, int32_t queue_capacity);
int hs_graph_set_inventory(hs_graph *g, int32_t node, int64_t initial_stock, int64_t reorder_point, int64_t order_quantity, double lead_time_s,
                           int32_t stockout_node);
/* After a run (any output may be NULL; node = -1 with `counters` NULL: the event counts alone):
 *   hs_graph_get_pool       counters[HS_POOL_COUNTERS]  _available, _active, len(_queue), _completed, _rejected;
 *   hs_graph_get_inventory  counters[HS_INVENTORY_COUNTERS]  _stock, _stockouts, _reorders, _items_consumed, _items_replenished,
 *                           _order_pending;
 *   events[HS_STOCK_KINDS]  the graph's pool Request / cycle end / consume Request / replenish Events: events_processed ==
 *                           sum(events_by_kind) + every other family's internal counts + sum(events). */
int hs_graph_get_pool(hs_graph *g, int32_t node, int64_t *counters, int64_t *events);
int hs_graph_get_inventory(hs_graph *g, int32_t node, int64_t *counters, int64_t *events);
/* Debug / tests only (the null stream, its own allocations): the compaction of a deployed LoadBalancer's member list on the device.
 * list[len] = slots in [0, n_slots) in insertion order, member[n_slots] = the membership word of every slot; the entries whose word is
 * 0 leave, the others keep their order: list[0 .. *out_len) afterwards.  wave = 0: the lone lane; 1: all 64 lanes (a ballot and a
 * prefix count per chunk of 64 entries).  Tests require both to leave the same list. */
int hs_debug_compact_members(int32_t device, int32_t n_slots, int32_t len, int32_t *list, const uint8_t *member, int32_t wave, int32_t *out_len);
/* Debug / tests only (the null stream, its own allocations): CoDelQueue._control_law's step on the device, one (count, interval_s) pair
 * per thread: out_ns[i] = Duration.from_seconds(interval_s[i] / sqrt(count[i])) in ns (count >= 1, 0 < interval <= 4e9).  Tests compare
 * it with CPython. */
int hs_debug_codel_next(int32_t device, int64_t n, const int64_t *count, const double *interval_s, int64_t *out_ns);
/* Auto-termination (core/simulation.py:306-322, end_time = Infinity): a run to end_ns = 2^61 ends in front of a pop when only daemon
 * events -- the limiters' polls -- are pending.  A run with any other end processes polls like any event. */
/* Debug / tests only (no engine path calls it; the null stream, its own allocations): FixedWindowPolicy._get_window_start on the device, one (now_ns, window_s) pair per thread: out_div[i] = Python's float
 * `to_seconds(now_ns[i]) // window_s[i]` (now_ns >= 0, window_s normal and > 0), out_start_ns[i] = from_seconds(out_div[i] * window_s[i]).
 * Tests compare both with CPython. */
int hs_debug_window_start(int32_t device, int64_t n, const int64_t *now_ns, const double *window_s, double *out_div, int64_t *out_start_ns);
/* How many LeastConnections / WeightedLeastConnections selections of the last run all 64 lanes of the wavefront took (min() over the
 * backends, strategies.py:186,237, as a strided scan + cross-lane reduction) instead of the lone lane (read-only, for tests).
 * Negative: an hs_status. */
int64_t hs_graph_coop_selects(const hs_graph *g);
/* Debug: bit 0 keeps every least-loaded selection on the lone lane, bit 1 hands every one to the wavefront (default: from
 * 32 backends on -- csrc/hs_graph.hip kCoopMinBackends, an estimate until tools/lb_strategies_profile.py has been run).  Takes effect at the next run; both give bit-identical results (tests/test_gpu_lb_strategies.py). */
int hs_debug_graph_flags(hs_graph *g, int flags);
/* `_execute_until(end)`: pops while the PREVIOUS event's time <= end_ns (so exactly one event beyond the end is processed,
 * core/simulation.py:472); may be called again with a later end (windows, :527-541). */
int hs_graph_run_until(hs_graph *g, int64_t end_ns);
/* ParallelRunner.run_sweep / run_replicas (parallel/runner.py:82-142: one worker process per independent Simulation) for graphs of
 * this path: `n` handles on one device run to `end_ns` SIDE BY SIDE -- one workgroup and one heap each, one launch for all of them
 * (up to 1 024 resident at once: four per CU with a 32 KB window of the heap in LDS), relaunched for the ones that have to grow a buffer.  Every handle ends in
 * exactly the state hs_graph_run_until(handle, end_ns) would leave; the device time a handle reports (hs_summary.last_run_ms) is the batch's.  On
 * an error the first handle's hs_graph_last_error names the graph. */
int hs_graph_run_many(hs_graph *const *graphs, int32_t n, int64_t end_ns);
/* ONE Simulation whose entity graph falls into parts that no Request can cross (connected components, or unions of them), every
 * handle one part with its nodes in the Simulation's order: the parts run side by side like hs_graph_run_many's replicas and
 * together leave what ONE heap over all of them leaves (core/simulation.py:449-505).  Why that is exact: an event's place among
 * its part's events never depends on the other parts -- except (i) inside a timestamp group that holds both an event numbered
 * BEFORE the run (a Source's / Probe's first tick, a schedule()d Request: the process-wide counter, core/event.py:53-67) and one
 * numbered BY the run (the heap's own counter, which counts every part's events), and (ii) for the single event beyond `end_ns`,
 * which is the earliest over all parts (the loop tests the previous event's time, core/simulation.py:472).  The parts stop in front
 * of their first event beyond `end_ns`; the one part that holds the earliest then processes it.  Returns HS_OK; or 1 = UNDECIDED
 * -- case (i) occurred, or two parts hold the earliest time: the caller repeats the run on one heap (the handles' state is then
 * meaningless); or a negative hs_status.  Call once per handle set (no later end). */
int hs_graph_run_parts(hs_graph *const *parts, int32_t n, int64_t end_ns);
/* Read-only: the level of the loop (csrc/hs_graph.hip kLvPlain ... kLvStock: 0 plain, 1 faults, 2 health, 3 resilience, 4 client,
 * 5 flow, 6 queue policies, 7 link faults, 8 scaler, 9 deployers, 10 hedge, 11 pools and stock; a level carries the code of all below it).  which = 0: the
 * lowest level that dispatches all the graph's kinds, the one a lone run takes; which = 1: the level of the most recent launch the
 * handle ran in (a batch runs at the highest level of its handles), -1 before the first launch.  -1 for any other `which`. */
int hs_graph_level(const hs_graph *g, int which);
int hs_graph_get_summary(hs_graph *g, hs_summary *out);
int hs_graph_get_stats(hs_graph *g, hs_graph_stats *out);
/* Every Sink record of the run in processing order: (Sink node, completion ns, created_at ns).  Returns the number of
 * records (copies min(that, cap)) or a negative hs_status. */
int64_t hs_graph_read_records(hs_graph *g, int32_t *node, int64_t *t_ns, int64_t *created_ns, int64_t cap);
const char *hs_graph_last_error(const hs_graph *g);
void hs_graph_destroy(hs_graph *g);

#ifdef __cplusplus
}
#endif
#endif /* HS_ENGINE_H */
