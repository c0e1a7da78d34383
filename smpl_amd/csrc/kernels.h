// smpl_amd/csrc/kernels.h -- launch geometry and prototypes of the gfx950 kernels (kernels.hip and the headers it includes)
#pragma once

#ifndef __HIPCC_RTC__   // hiprtc (per-robot specialisation, specialize.cpp) brings its own runtime declarations
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

#include "device_types.h"

#define SMPLX_BLOCK 128          // 2 waves; per-thread LDS scratch keeps ~4 blocks per CU resident
#define SMPLX_SETUP_BLOCK (SMPLX_BLOCK + 64)   // threads of a k_pipe_setup block: the edge threads and the goal-distance wave
#define SMPLX_STEP_BLOCK SMPLX_SETUP_BLOCK      // threads of a k_step_block block: 128 edge lanes and the goal-distance wave
#define SMPLX_STEP_STATES 16                    // most states whose edges one k_step_block block may hold (smplx_step_states)
// k_step_block's part of a stream's counter set (ints; StepLaunch::WorkCounters): behind the pipeline's 2 KB, one 64-bit claim
// word per shard of the compact stream on a 128-byte line of its own -- records claimed in region A in bits 0-23, in region
// B in bits 24-47, blocks of the shard that have claimed in bits 48-63 -- then, on a line of its own, the count of shards
// whose blocks have all claimed
#define SMPLX_STEP_CTR_BASE 512
#define SMPLX_STEP_CTR_DONE (SMPLX_STEP_CTR_BASE + 32 * SMPLX_CMP_SHARDS)
#define SMPLX_STEP_CLAIM_BITS 24    // bits of a claim word's record fields
#define SMPLX_STEP_COUNT_BITS 16    // ... and of its block count
#define SMPLX_WORK_COUNTER_BYTES 16384
#define SMPLX_SEARCH_STATIC_LDS (44 * 1024)   // static LDS of k_search (2 x ExpandLds + SearchLds + header and primitives copies), an upper bound
#define SMPLX_GLOBAL_AS __attribute__((address_space(1)))   // device code: a pointer known to be device memory (model_lds.h as_global)
#define SMPLX_LAZY_COST 1000      // every cost of the lazy pair: the three-argument cost() (manip_lattice.cpp:1388-1412), int(1000 * 1) (:1156)
#define SMPLX_TRUE_COST_LANES 8    // lanes that share an item of k_true_cost: the waypoints of its edge are dealt out to them
#define SMPLX_TALLIES 6           // per-block tallies (tally_block)     // per-thread DFS stack (node indices, one byte each)

// dynamic LDS bytes: the packed model, plus (collision kernels) per-thread scratch
// small-batch kernel: 7 waypoint lanes per primitive + the state's own lane in whole "config" waves, then one more wave
// whose lanes are the primitives' bookkeeping lanes + the goal-distance lane (nprims + 1 <= 64)
static inline int smplx_small_block(int nprims) { return ((nprims * 7 + 1) + 63) / 64 * 64 + 64; }
// k_search: the same, plus a wave that works out the successors' heuristics beside the search wave where 512 threads allow it
static inline int smplx_search_block(int nprims) { const int b = smplx_small_block(nprims); return b + 64 <= 512 ? b + 64 : b; }
static inline size_t smplx_lds_bytes_n(size_t blob_bytes, int nroot, int nslots, int nvars, int stack_bytes, int nthreads)
{
    return blob_bytes + (size_t)(3 * nroot + 12 * nslots + nvars) * 8 * nthreads + (size_t)stack_bytes * nthreads;
}
static inline size_t smplx_lds_bytes(size_t blob_bytes, int nroot, int nslots, int nvars, int stack_bytes)
{
    return smplx_lds_bytes_n(blob_bytes, nroot, nslots, nvars, stack_bytes, SMPLX_BLOCK);
}
// the clearance kernels (clearance.h clearance_lds): a root position for every tree, the saved transforms in LDS in both builds
static inline size_t smplx_clearance_lds_bytes(size_t blob_bytes, int ntrees, int nslots, int nvars, int stack_bytes)
{
    return smplx_lds_bytes_n(blob_bytes, ntrees, nslots, nvars, stack_bytes, SMPLX_BLOCK);
}

// most states that 128 consecutive edges of the (state, primitive) grid belong to
static inline int smplx_step_states(int nprims) { return (SMPLX_BLOCK - 2 + nprims) / nprims + 1; }
// can a k_step_block grid of `blocks` blocks claim in the packed words: a shard's blocks fit the count field and the records
// they can hold (SMPLX_BLOCK each) a record field
static inline bool smplx_step_claim_fits(long long blocks)
{
    const long long in_shard = (blocks + SMPLX_CMP_SHARDS - 1) / SMPLX_CMP_SHARDS;
    return in_shard < (1ll << SMPLX_STEP_COUNT_BITS) && in_shard * SMPLX_BLOCK < (1ll << SMPLX_STEP_CLAIM_BITS);
}

// The kernels that have a per-robot build, stated once as X(id, kernel): enum KernelId (K_<id>, specialize.h), the names
// asked of the per-robot code object and the generic kernels beside them (specialize.cpp) all come from this list.
#define SMPLX_PER_ROBOT_KERNELS(X) \
    X(STATE_PREP, k_state_prep) X(EXPAND, k_expand) X(PIPE_PREP, k_pipe_prep) X(PIPE_SETUP, k_pipe_setup) \
    X(PIPE_CONFIGS, k_pipe_configs) X(PIPE_FINISH, k_pipe_finish) X(SMALL_BATCH, k_small_batch) X(EDGE_VALID, k_edge_valid) \
    X(STATE_VALID, k_state_valid) X(HEURISTIC, k_heuristic) X(SPHERE_POSITIONS, k_sphere_positions) X(SEARCH, k_search) \
    X(ATTACHED_POSITIONS, k_attached_positions) X(PLANNING_POSE, k_planning_pose) X(STEP_BLOCK, k_step_block) \
    X(STATE_CLEARANCE, k_state_clearance) X(EDGE_CLEARANCE, k_edge_clearance) X(LAZY_SUCCS, k_lazy_succs) \
    X(TRUE_COST, k_true_cost) X(HEURISTIC_CLOSED, k_heuristic_closed) X(SHORTCUT, k_shortcut) X(PATHS_VALID, k_paths_valid) \
    X(PATH_WAYPOINTS, k_path_waypoints)

extern "C" {
__global__ void k_state_prep(const SmplxSpaceDev* S, const double* Q, int B, double* goal_dist,
                             unsigned char* parent_valid, int* parent_lookups,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q);
__global__ void k_expand(const SmplxSpaceDev* S, const double* Q, int B, const double* goal_dist,
                         const unsigned char* parent_valid, const int* parent_lookups, unsigned char* out_flags,
                         int* out_coord, double* out_q, int* out_h, int* out_cost, int* out_lookups,
                         unsigned long long* counters, const int* deferred_count,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q);
__global__ void k_pipe_prep(const SmplxSpaceDev* S, const double* Q, int B, double* goal_dist,
                            int* work_count,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q, int* cmp_totals,
                            const int* ins_items, int n_ins, double* trig);
__global__ void k_pipe_setup(const SmplxSpaceDev* S, const double* Q, int B, double* goal_dist,
                             unsigned char* out_flags, double* out_q, int* edge_w, int* edge_lookups,
                             unsigned char* edge_bad, int* state_lookups, unsigned char* state_bad, unsigned long long* work,
                             int* work_count, int capacity,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q, int have_goal_dist,
                             int* cmp_totals, const int* ins_items, int n_ins, int nprims, int nvars, double* trig);
__global__ void k_pipe_configs(const SmplxSpaceDev* S, const double* Q, int B, const double* out_q,
                               const int* edge_w, int* edge_lookups, unsigned char* edge_bad, int* state_lookups,
                               unsigned char* state_bad, const unsigned long long* work, const int* work_count, int capacity,
                               int cfg_blocks, const unsigned char* out_flags, int* succ_coord,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q, int want_id,
                               unsigned long long* succ_eval, unsigned char* succ_goal, int nprims, int nvars,
                               const unsigned char* blob, int blob_bytes, const double* trig);
__global__ void k_pipe_finish(const SmplxSpaceDev* S, const double* Q, int B, const int* edge_w,
                              const int* edge_lookups, const unsigned char* edge_bad, const int* state_lookups,
                              const unsigned char* state_bad, unsigned char* out_flags, int* out_coord, double* out_q,
                              int* out_h, int* out_cost, int* out_lookups, unsigned long long* counters,
                              const double* goal_dist,
                         const SmplxSpaceDev* const* stab, const unsigned short* state_q, int* out_id, SmplxCompactDev cmp,
                              const unsigned long long* succ_eval, const unsigned char* succ_goal, const int* succ_coord,
                              int* work_count, int nprims, int nvars);
__global__ void k_step_block(const SmplxSpaceDev* S, const double* Q, int B, unsigned char* out_flags, int* out_coord,
                             double* out_q, int* out_h, int* out_cost, int* out_lookups, unsigned long long* counters,
                             const SmplxSpaceDev* const* stab, const unsigned short* state_q, int* out_id, SmplxCompactDev cmp,
                             int* step_ctr, int nprims, int nvars, const unsigned char* blob, int blob_bytes);
__global__ void k_small_batch(const SmplxSpaceDev* S, const double* Q, int B, double* goal_dist_out,
                              unsigned char* state_bad_out, int* state_lookups_out, unsigned char* out_flags, int* out_coord,
                              double* out_q, int* out_h, int* out_cost, int* out_lookups,
                              const SmplxSpaceDev* const* stab, const unsigned short* state_q, unsigned char* host_flags,
                              int* host_coord, double* host_q, int* host_h, int* out_id, int* host_id, const int* ins_items,
                              int n_ins);
__global__ void k_search(const SmplxSpaceDev* const* stab, int max_steps, int lh, int* status_out, long long pre_ticks);
__global__ void k_search_table_fill(const SmplxSpaceDev* Sq, const int* coord, int first, int n, int nvars);
__global__ void k_table_probe_ops(SmplxTableDev T, const int* coords, int n, int nv, int one_home, int insert, int* out);
__global__ void k_heap_ops(const int* ops, int nops, int lh, unsigned long long* heap_hbm, SmplxSState* st, int* top_after);
__global__ void k_edge_valid(const SmplxSpaceDev* S, const double* Aq, const double* Bq, int n, unsigned char* out,
                             int* out_lookups, int* out_waypoints);
__global__ void k_state_valid(const SmplxSpaceDev* S, const double* Q, int n, unsigned char* out, int* out_lookups);
__global__ void k_heuristic(const SmplxSpaceDev* S, const double* Q, int n, int* out_h, double* out_xyz);
__global__ void k_heuristic_closed(const SmplxSpaceDev* S, const double* Q, int n, int* out_h, double* out_xyz);
__global__ void k_planning_pose(const SmplxSpaceDev* S, const double* Q, int n, double* out_T);
__global__ void k_sphere_positions(const SmplxSpaceDev* S, const double* Q, int n, double* out);
__global__ void k_attached_positions(const SmplxSpaceDev* S, const double* Q, int n, double* out);
__global__ void k_state_clearance(const SmplxSpaceDev* S, const double* Q, int n, double padding, double* out, double* out_parts,
                                  int* out_witness);
__global__ void k_edge_clearance(const SmplxSpaceDev* S, const double* Aq, const double* Bq, int n, double padding, double* out,
                                 double* out_parts, int* out_witness);
__global__ void k_lazy_succs(const SmplxSpaceDev* S, const double* Q, int B, unsigned char* out_flags, int* out_coord, double* out_q,
                             int* out_h, int* out_id);
__global__ void k_true_cost(const SmplxSpaceDev* S, const double* Pq, const int* child_coord, const unsigned char* goal_edge, int n,
                            double* work_q, int* out_cost, int* out_prim, int* out_nmatch);
__global__ void k_shortcut(const SmplxSpaceDev* const* stab, const double* pts, const int* first, const double* accum, int* keep_all,
                           int* nkeep, int* err, long long* checked);
__global__ void k_paths_valid(const SmplxSpaceDev* const* stab, const int* blocks, const double* Q, unsigned char* out);
__global__ void k_path_waypoints(const SmplxSpaceDev* S, const double* A, const double* B, const int* first, double* out,
                                 int* out_count);
__global__ void k_table_insert(const SmplxSpaceDev* S, const SmplxSpaceDev* const* stab, const int* items, int n, int nvars);
__global__ void k_bfs_metric(SmplxGridDev grid, SmplxBfsDev bfs, const double* xyz, int n, double* out);
__global__ void k_bfs_init(SmplxGridDev g, int wall_thr, int nbx, int nby, int nbz, int* dist);
__global__ void k_bfs_reset(int* dist, size_t total);
__global__ void k_bfs_export(SmplxBfsDev b, int* out);
__global__ void k_bfs_brick_seed(int* dist, int cx, int cy, int cz, int nbx, int nby, int nbz, int* list0, int* counts, int tag_word);
__global__ void k_bfs_brick_wave(int* dist, int nbx, int nby, int nbz, const int* list_in, const int* counts_in, int* list_next,
                                 int* counts_next, int* counts_after, int shard_cap, int* queued_mine, int* queued_next, int* queue_size_out, int tag_word, int tag_mask);
__global__ void k_bfs_brick_seed_multi(const SmplxBfsGoalDev* goals, int nq, int nbx, int nby, int nbz, int* pass_stats, int n_stats);
__global__ void k_bfs_brick_wave_multi(const SmplxBfsGoalDev* goals, int nbx, int nby, int nbz, int pass, int history_slot, int* stats);
}
