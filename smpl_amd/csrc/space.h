// smpl_amd/csrc/space.h -- the records behind the handles of the C-ABI (include/smpl_amd.h).  smplx_space is the handle's
// own fields (stream, model, grid, scratch, counters) plus one member per concern: the goal (goals.h), the lattice
// (lattice.h), the device copy of the state table, the BFS buffers, the plain-GetSuccs speculation, the small-batch
// governor, the step-launch switches, the attached bodies, the device-resident search and the lazy pair.  The components
// are plain structs with public fields; the functions that work on them take the space and live in the header of their
// concern (goals.h, bfs_host.h, heuristic_host.h, device_table.h, step.h, expand_entry.h, attached_host.h, search_host.h,
// lazy.h, plan_entry.h).  Every device allocation, stream and event is held by an owner of device_mem.h: deleting the
// space frees them; only the device image `hs`, which the kernels read, names them by plain pointers.  At the end: the two operations that touch several components
// at once, a state joining the lattice (new_state) and a query starting over (reset_lattice).
#pragma once

#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "device_mem.h"
#include "device_types.h"
#include "grid_handle.h"
#include "host_core.h"
#include "lattice.h"
#include "model_compile.h"
#include "specialize.h"

namespace {

// Dense outputs of a planner frontier batch in ONE allocation -- successor joint values | coordinates | heuristic |
// flags -- so that they come back in one DMA copy; the device block and its pinned host twin share the layout.
struct OutView {
    double* sq = nullptr;
    int32_t* coord = nullptr;
    int32_t* h = nullptr;
    int32_t* id = nullptr;      // K5: state id of the successor's coordinate in the device table, -1 = not there
    unsigned char* flags = nullptr;
    size_t bytes = 0;
};

inline OutView carve_out(unsigned char* base, size_t BM, int N)
{
    OutView v;
    size_t o = 0;
    v.sq = (double*)(base + o); o += BM * N * sizeof(double);
    v.coord = (int32_t*)(base + o); o += BM * N * sizeof(int32_t);
    v.h = (int32_t*)(base + o); o += BM * sizeof(int32_t);
    v.id = (int32_t*)(base + o); o += BM * sizeof(int32_t);
    v.flags = base + o; o += BM;
    v.bytes = (o + 15) / 16 * 16;
    return v;
}

// The buffers of one frontier batch (issue_frontier).  A space owns one for its own batches -- its b_q, b_work, b_cost,
// b_lookups and b_out are also the scratch of the C-ABI expansion entry points -- and the asynchronous multi-query
// driver keeps a ring of them.
struct FrontierBatch {
    DevBuf<double> b_q;                  // parents, then the staged K5 inserts (one upload)
    DevBuf<unsigned short> b_stateq;     // cross-query batch: per-row query index
    DevBuf<unsigned char> b_work, b_out;
    DevBuf<int32_t> b_cost, b_lookups;
    PinBuf<double> p_q;
    PinBuf<unsigned short> p_stateq;
    PinBuf<unsigned char> p_out;
    std::vector<int32_t> ins_items;      // K5 inserts of the requesting spaces, tagged with their query slots
    OutView dv, pv;                      // packed outputs: device block, pinned host twin
    DevEvent done;                       // recorded behind the batch on its stream
    bool zero_copy = false;              // the batch wrote its results straight into pv (single launch, no copies)
    std::chrono::steady_clock::time_point t_issue;
};

// device copy of the state table (K5; SmplxTableDev in hs.table): the states created since the last synchronisation
// wait in pending_ins as (query slot, id, coord[N]) triples and go up with the next frontier batch (device_table.h)
struct DeviceTable {
    DevPtr<int32_t> d_table;
    size_t cap = 0, count = 0;
    size_t test_slots = 0;        // test hook: slots of the first table table_ensure allocates (0: the default)
    int64_t regrows = 0;          // times the table was outgrown (load factor above 1/2) and allocated again, every state re-inserted
    std::vector<int32_t> pending_ins;
    DevBuf<int32_t> b_ins;
    PinBuf<int32_t> p_ins;
};

// buffers and bookkeeping of the BFS heuristic's distance field (bfs_host.h)
struct BfsHost {
    DevPtr<int32_t> d_dist;                     // brick-major distance records (hs.bfs.dist)
    DevPtr<int32_t> d_queue;                    // brick lists of the two passes in flight
    DevPtr<int32_t> d_counts;
    DevPtr<int32_t> d_brick_queued;             // wave-per-brick mode: 2 x nbricks "queued for the next pass" words
    int bricks[3] = {0, 0, 0};
    int64_t total = 0;                          // cells of the padded grid the API hands out (smplx_bfs_copy)
    int64_t ints = 0;                           // ints of the brick-major records on the device
    bool reset_due = false;
    int tag = 0;                                // tag of the last BFS run (device_types.h SmplxBfsDev), 0 before the first
    std::vector<int32_t> queue_sizes;           // bricks queued in every pass of the last BFS: sizes the next goal's launches
    int levels = 0;
    int wall_thr = -1;
    // of the leading space of a multi-goal run (run_bfs_multi): the goals' records and the per-pass queue totals
    DevBuf<SmplxBfsGoalDev> b_goals;
    DevBuf<int32_t> b_pass_stats;
};

// Speculation for callers that only know GetSuccs (an unchanged SBPL planner never calls smplx_hint_frontier): the
// space mirrors the g-values the caller's expansions imply (Lattice::g_est; g[succ] = min(g[succ], g[id] + cost), exactly
// what ARAStar::expand does, arastar.cpp:546-551) and, on a miss, lets the created-but-unevaluated states with the
// smallest g + w*h ride along.  Only a guess at the caller's OPEN order: a wrong guess costs GPU work, never results.
struct PlainSpeculation {
    bool plain_mode = false;            // set by the first smplx_get_succs from outside the engine's own search
    int auto_spec = 96;                 // states that ride along per miss (SMPLX_AUTO_SPECULATE, 0 = off)
    double auto_w = 5.0;                // weight of h in the ranking (SMPLX_AUTO_SPECULATE_W)
    std::vector<std::pair<uint64_t, int32_t>> pool;   // binary min-heap of (rank key, id) of unevaluated states
    std::vector<int32_t> hint;          // the frontier states that ride with the next miss (smplx_hint_frontier, auto_hint)
};

// Small batches: the single-launch kernel costs the host one launch (27 us issue-to-landing for the handful of states
// a lone query misses on), the pipeline several launches and copies (~34 us).  Both give the same bytes.  The engine
// watches the issue-to-landing time of the single-launch path and sits out 2000 batches on the pipeline path whenever
// its moving average exceeds 70 us: a safety net from the time the kernel checked the snap-to-goal edge of every
// state ungated (105 us per launch; fixed, see k_small_batch) -- it costs nothing when the kernel behaves.
struct SmallBatchGovernor {
    int batch_max = 512;          // batches up to this many states take the single-launch kernel (SMPLX_SPACE_NO_SMALL_KERNEL disables)
    double latency_limit = 70e-6; // SMPLX_SMALL_KERNEL=always lifts it, =never disables the single-launch kernel
    bool adaptive = false;        // only a lone query measures: with several queries per thread the landing time includes their turns
    double latency = 0.0;         // moving average, seconds
    int seen = 0, pipeline_left = 0;
    int64_t small_launches = 0, pipe_launches = 0;
};

// how an expansion step is launched: mode switches, test hooks (test_hooks.h), per-stream counters, profiling events
struct StepLaunch {
    bool fused_mode = false;   // SMPLX_SPACE_FUSED: one thread per edge (reference lookup tallies)
    int work_list_items = 0;   // > 0: test hook -- a work list this small, so that the deferred pass is exercised
    bool pipe_prep = false;    // test hook: k_pipe_prep in a launch of its own in front of k_pipe_setup
    int three_launch_blocks = 0;   // largest k_pipe_setup grid (edge blocks) that runs the three-launch step; 0: not asked yet
    int one_launch = -1;       // test hook: -1 the rule (expand_path), 0 never k_step_block, 1 whenever it can run at all
    size_t one_launch_lds = 0; // dynamic LDS of a k_step_block block
    int one_launch_per_cu = 0; // blocks of k_step_block that share a CU (occupancy query)
    int one_launch_blocks = 0; // blocks of k_step_block resident in one round (occupancy query x CUs); 0: it cannot run
    int64_t one_launch_steps = 0;   // steps that took k_step_block
    // Counters of a step, SMPLX_WORK_COUNTER_BYTES: the pipeline's work-list counters (8 shard counters + deferred count, one
    // 128-byte line each) and, behind them, what k_step_block keeps (kernels.h SMPLX_STEP_CTR_*: one packed claim word per
    // shard of the compact stream -- records of both regions and the blocks that have claimed -- and the count of finished
    // shards).  One set per stream the space has launched a step
    // on.  A set is all-zero whenever no step is in flight on its stream: k_pipe_finish clears its part behind its last
    // reader, the last block of k_step_block its own.  dirty: a launch sequence on it failed part-way, it is cleared before
    // its next use.
    struct WorkCounters { hipStream_t stream; DevPtr<int32_t> p; bool dirty; };
    std::vector<WorkCounters> work_counters;
    // optional per-kernel timing of expand launches (bench.py roofline): 3 events per launch
    std::vector<DevEvent> prof_events;
    size_t prof_used = 0;
};

// collision bodies attached to robot links (CollisionSpace::attachObject, collision_space.cpp:297-345), in attach order;
// their device image (hs.bodies, null while there are none) is rebuilt at every attach and detach
struct AttachedBodies {
    struct Body {
        std::string id, link;
        int joint = -1;                    // depth-first joint whose child link carries it, -1 = the root link
        std::vector<double> xyzr;          // spheres in the link's frame
        std::vector<std::string> allowed;  // link names and body ids it may touch
        int first = 0, count = 0;          // its nodes in the device image
    };
    std::vector<Body> bodies;
    DevPtr<SmplxBodiesDev> d_bodies;
    WorkSpace vox;                     // of the voxeliser for objects attached by shape (object_sphere_rows.h), like the grid's
    uint64_t epoch = 0;                // attaches + detaches so far
    uint64_t epoch_goal = 0;           // ... when the goal was set: the successor caches belong to that set of bodies
};

const char* const kBodiesChanged = "bodies were attached or detached after the goal was set: cached successors are stale, set the goal again";

// scratch and tallies of the lazy successor pair (lazy.h): its own buffers, like the clearance queries'
struct LazyHost {
    DevBuf<double> b_q, b_sq;
    DevBuf<int32_t> b_coord, b_h, b_id, b_out;   // b_out: n costs, n primitives, n match counts
    DevBuf<unsigned char> b_flags, b_goal;
    int riders = 64;                 // most states that ride along with a GetLazySuccs miss (SMPLX_LAZY_RIDERS, 0 = none)
    // binary min-heap of (heuristic, id) of the states GetLazySuccs created and has not evaluated: a caller that never hints
    // (a lazy SBPL planner) gets the ones nearest the goal as riders -- a guess at its OPEN order that costs GPU work when
    // wrong, never results
    std::vector<std::pair<int32_t, int32_t>> pool;
    // GetTrueCost misses: the unevaluated edges of the parent's lazy list ride along, and those of the `ride_parents` states
    // whose lists were committed last (SMPLX_TRUE_COST_PARENTS, 0 = the parent alone) -- the edges a lazy search is likeliest
    // to ask about next
    int ride_parents = 8;
    std::vector<int32_t> recent;     // ids in the order their lazy lists were committed
    // [0] k_lazy_succs launches of GetLazySuccs, [1] GetLazySuccs calls served without one, [2] k_true_cost launches of
    // GetTrueCost / the batch call, [3] edges they evaluated, [4] pairs answered from the cache, [5] pairs that were not
    int64_t counters[6] = {0, 0, 0, 0, 0, 0};
};

// scratch of smplx_post_process_paths (path_multi.h), held by the call's leading space: its own buffers, like the
// clearance queries', so that the call touches nothing a search or a frontier batch may hold between calls
struct PathMultiHost {
    DevBuf<const SmplxSpaceDev*> b_stab;   // per path: its space's device image
    DevBuf<double> b_rows;                 // the rows of a pass; the points and accumulated costs of the shortcut stage
    DevBuf<unsigned char> b_valid;
    DevBuf<int32_t> b_ints;                // the block table of a pass; offsets, keep lists, counts and error words of the shortcut stage
    DevBuf<long long> b_checked;
};

// the goal as the host holds it (goals.h; the device's record is hs.goal), and the start's position
struct GoalHost {
    bool set = false;
    uint64_t grid_epoch = 0;     // the grid's edit count when the goal was set: the successor caches belong to that field
    double xyz[3] = {0, 0, 0};
    double rpy[3] = {0, 0, 0};   // of a pose goal (SMPLX_GOAL_XYZ_RPY), as the caller gave them
    double rpy_tol = 0;
    double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // the goal rotation the Euclidean heuristic measures against (SmplxHeurDev::rot)
    double start_xyz[3] = {0, 0, 0};   // planning-link position of the start state (getMetricStartDistance)
};

struct Search;   // the host-driven ARA* (ara_search.h)

// the device-resident ARA* of a query (search_host.h)
struct DevSearch {
    DevPtr<unsigned char> arena;         // one allocation carved into the buffers of SmplxSearchDev
    DevPtr<SmplxSearchDev> d_hdr;
    SmplxSearchDev h;                    // host copy of the header: pointers, capacities, and the last state read back
    struct Caps { int states = 0, heap = 0, incons = 0, log = 0, succ = 0, path = 0; } caps;
    int dev_states = 0;                  // ids [0, dev_states) exist on the device
    bool table_fresh = false;            // the device table was just (re)allocated: empty
    bool host_behind = false;            // the device created states / committed lists the host arrays do not hold yet
    bool log_on_device = false;          // the expansion log of the last search has not been read back
    int call_number = 0, n_succ_kept = 0;
    int64_t grows = 0, searches = 0, ticks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t table_allocs = 0;            // state tables the search allocated: each starts empty and is filled by k_search_table_fill
    int dup_pushes = 0;
    int64_t evals_base[3] = {0, 0, 0};   // the header's committed / GPU evaluations and grid lookups when the call began
    int test_capacity = 0;               // test hook: first capacity in states
    bool test_no_helper = false;         // test hook: launch k_search without its helper wave
};

}  // namespace

struct smplx_model {
    smplx::HostModel hm;
};

struct smplx_space {
    smplx::HostModel model;
    const smplx_grid* grid = nullptr;
    smplx::HostActions actions;
    smplx_params params;
    SmplxSpaceDev hs;
    // before every member that owns device memory, so that it dies after them: members go in reverse order, and every
    // buffer and event below is freed while the stream still exists.  smplx_space_destroy waits for it first.
    DevStream stream;
    DevPtr<SmplxSpaceDev> d_space;
    int device = 0;   // HIP device the handle lives on (worker threads select it explicitly)
    int N = 0, M = 0;
    size_t lds_bytes = 0, blob_bytes = 0;
    size_t lds_bytes_valid = 0;      // k_state_valid, k_edge_valid, k_pipe_configs: in the per-robot build they keep the saved link transforms in registers
    size_t lds_bytes_clearance = 0;  // k_state_clearance, k_edge_clearance (kernels.h smplx_clearance_lds_bytes)
    int lds_nroot = 0;   // root-position slots per thread in LDS: none in the per-robot build (they live in registers there)
    smplx::KernelSet ks;       // per-robot kernels (specialize.h), generic ones with SMPLX_SPACE_GENERIC_KERNELS or SMPLX_SPECIALIZE=0
    std::string specialize_note;   // why the per-robot build is absent, if it is
    GoalHost goal;
    int status = SMPLX_OK;            // sticky: first error of a call that has no way to report one (smplx_space_status)
    std::string status_msg;
    // scratch of the C-ABI entry points
    DevBuf<double> b_q2, b_sq, b_xyz;
    DevBuf<unsigned char> b_flags;
    DevBuf<int32_t> b_coord, b_h, b_way;
    DevBuf<unsigned long long> b_counters;
    // the clearance queries' own scratch: they never touch a buffer a search or a frontier batch may hold between calls
    DevBuf<double> b_clr_q, b_clr_q2, b_clr_out;   // b_clr_out: n clearances, then n x 2 parts
    DevBuf<int32_t> b_clr_wit;
    DevBuf<const SmplxSpaceDev*> b_stab;   // cross-query batches (smplx_plan_multi): the query table, owned by the leading space
    FrontierBatch batch;           // the space's own frontier batches (issued on `stream`)
    // the states of the frontier batch in flight
    std::vector<int32_t> inflight;
    std::vector<double> inflight_q;     // smplx_plan_multi: the joint values of `inflight`, staged by the query's worker
    // stats
    int64_t gpu_batches = 0, cache_hits = 0, cache_misses = 0, committed_evals = 0, gpu_evals = 0;
    std::vector<int32_t> expansion_log;
    // the search of the last smplx_plan / smplx_replan call, which a later smplx_replan may continue
    int search_side = 0;                 // 0: none (or not resumable), 1: device-resident, 2: host-driven loop
    int search_start = -1;               // its start id
    std::shared_ptr<Search> host_search; // the host loop's search (OPEN, INCONS, search states) between calls
    // one member per concern
    Lattice lat;
    DeviceTable dt;
    BfsHost bfs;
    PlainSpeculation spec;
    SmallBatchGovernor small;
    StepLaunch step;
    AttachedBodies att;
    DevSearch ds;
    LazyHost lazy;
    PathMultiHost pm;
};
static_assert(!std::is_copy_constructible<smplx_space>::value && !std::is_copy_assignable<smplx_space>::value,
              "a space owns its stream and its device memory");

namespace {

int upload_space(smplx_space* s)
{
    HIP_TRY(hipMemcpyAsync(s->d_space, &s->hs, sizeof(SmplxSpaceDev), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// a state joins the lattice (getOrCreateState's create branch) and waits for the next upload to the device table
int new_state(smplx_space* s, const int32_t* coord, const double* q, int32_t h)
{
    const int id = s->lat.append(coord, q, h);
    if (s->dt.d_table) {
        s->dt.pending_ins.push_back(0);
        s->dt.pending_ins.push_back(id);
        s->dt.pending_ins.insert(s->dt.pending_ins.end(), coord, coord + s->N);
        ++s->dt.count;
    }
    return id;
}

// a new goal starts a new query: state ids are renumbered, so every component that names one starts over
void reset_lattice(smplx_space* s)
{
    s->lat.clear(s->N);
    s->ds.dev_states = 0; s->ds.host_behind = false; s->ds.log_on_device = false; s->ds.n_succ_kept = 0;
    s->search_side = 0;                             // no search continues across this
    s->ds.table_fresh = s->dt.d_table != nullptr;   // (emptied below)
    s->spec.hint.clear();
    s->spec.pool.clear();
    s->spec.plain_mode = false;
    s->dt.pending_ins.clear();
    s->dt.count = 0;
    for (int64_t& c : s->lazy.counters) c = 0;
    s->lazy.pool.clear();
    s->lazy.recent.clear();
    if (s->dt.d_table) (void)hipMemsetAsync(s->dt.d_table, 0, s->dt.cap * (size_t)s->hs.table.stride * sizeof(int32_t), s->stream);
}

}  // namespace
