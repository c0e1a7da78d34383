/* smpl_amd/csrc/test_hooks.h -- entry points that exist for the parity tests only.  They are exported by the shared
 * library but are NOT part of the drop-in boundary (include/smpl_amd.h): nothing a planner needs is declared here. */
#pragma once

#include "../../include/smpl_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Shrinks the (edge, waypoint) work list of the expansion pipeline to `items` entries, so that nearly every edge
 * overflows it and is walked whole by its finish thread (the deferred pass, which an ordinary batch never needs);
 * 0 restores the default size. */
int smplx_test_set_work_list_items(smplx_space* s, int items);

/* on = 1: the expansion pipeline runs as four launches -- k_pipe_prep (goal distance per state, counters, K5 inserts) in a
 * launch of its own in front of k_pipe_setup, which then takes its gate from what k_pipe_prep left; 0 restores the
 * default: three launches, where k_pipe_setup computes the goal distance itself, for every batch whose setup blocks fit
 * the chip in one round (four beyond that).  Same results, bit for bit. */
int smplx_test_set_pipe_prep(smplx_space* s, int on);

/* Which pipeline steps run as the one launch k_step_block (step_block.h): -1 the rule (per-robot kernels, no pipeline test
 * hook, no profile-event triple armed, every block resident in one round), 0 never, 1 whenever the kernel can run at all --
 * a step that then cannot take it fails with an error instead of running the pipeline.  Same results, bit for bit. */
int smplx_test_set_one_launch(smplx_space* s, int mode);

/* Steps of this space that took k_step_block so far. */
long long smplx_test_one_launch_steps(const smplx_space* s);

/* Waits for `stream` and returns 1 if the space's step counters of that stream are all-zero, as they must be whenever no step
 * is in flight on it, 0 if not; an error (negative) if no step has run on the stream. */
int smplx_test_step_counters_zero(smplx_space* s, void* stream);

/* The heap primitives of the device-resident search (search_heap.h; pop is the search's own heap_pop_wave) driven by an op
 * sequence in the language of oracle/heap_ref_driver.cpp (pairs code, key; see k_heap_ops): top_after[i] = element at the top
 * after op i, -1 when empty.
 * lds_entries = how many leading heap entries live in LDS (the rest in HBM), 1 .. 4096. */
int smplx_test_heap_ops(const int32_t* ops, int nops, int lds_entries, int32_t* top_after);

/* The state-table probe of the device-resident search (search_table.h table_probe_start / table_probe_finish /
 * table_store_own, see k_table_probe_ops) on an empty table of `slots` slots (a power of two, more than n_inserted) for
 * coordinates of nvars ints: `inserted` go in one after the other, coordinate i under id i (found_at_insert[i] = what the
 * probe found before the store: -1 unless the coordinate was there already), then every row of `queries` is looked up
 * (ids[i] = id or -1).  one_home = 1: every probe starts at slot 0 instead of the coordinate's hash. */
int smplx_test_table_probe(int nvars, int slots, int one_home, const int32_t* inserted, int n_inserted, const int32_t* queries, int n_queries,
                           int32_t* found_at_insert, int32_t* ids);

/* While `slots` is set (a power of two, at least 64; 0 restores the default of 2^18), the first device copy of the state table
 * that a space without one allocates (smplx_table_sync, the K5 entry points) starts at that many slots; it still grows by the
 * ordinary rule (a table four times the size at load factor 1/2), so a small lattice gets a table that is between one eighth
 * and one half full instead of nearly empty, with probe chains that go beyond the home slot. */
int smplx_test_set_table_slots(smplx_space* s, int slots);

/* Slots of the space's device copy of the state table now; 0 while it has none. */
long long smplx_test_table_slots(const smplx_space* s);

/* First capacity (states) of the device-resident search's buffers, so that a test can make a search outgrow them
 * (SMPLX_SS_GROW: the host enlarges and launches again); 0 restores the default sizing.  A state table that the search
 * allocates while the hook is set starts at the smallest size that holds this capacity half full (instead of 2^16 slots),
 * so it is outgrown and filled again along with the buffers.  The path buffer of a search that starts while the hook is set
 * holds 64 ids at first (instead of 2^16): a longer solution does not fit, and the host doubles the buffer and launches
 * again for the path alone (grow_what = 3). */
int smplx_test_set_search_capacity(smplx_space* s, int states);

/* on = 0: the device-resident search runs WITHOUT its helper wave (the search wave does the successors' bookkeeping inline,
 * as it does for robots whose block would exceed 512 threads with one); 1 restores the default. */
int smplx_test_set_search_helper(smplx_space* s, int on);

/* The host build of smplx_acos (det_math.h) at n arguments: what the accuracy statement in its comment is measured on.
 * Needs no GPU. */
int smplx_test_acos(const double* x, int n, double* out);

/* The goal rotation a SMPLX_H_EUCLID space measures against (row-major 3x3), as the engine holds it: the identity under an
 * xyz goal, the rotation it built from a pose goal's rpy, its own FK of a joint goal's angles.  SMPLX_E_STATE without a goal. */
int smplx_test_goal_rotation(const smplx_space* s, double R[9]);

/* smplx_model_const_header for either flavour of the per-robot build: closed_form = 1 gives the header a closed-form space's
 * build is compiled against (specialize.h kClosedFormDefine appended).  Returns the size needed, including the NUL. */
int smplx_test_const_header(const smplx_model* m, int closed_form, char* out, int cap);

/* The joint values the lanes of k_shortcut (path_kernels.h) check on the edges a[i] -> b[i], i < n: one block an edge, the
 * waypoints dealt to its lanes as in the kernel, each written as stage_config staged it.  first: n + 1 row offsets into
 * out (the caller's waypoint counts, smplx_cc_interpolate's); counts[i] = the device's count.  An edge writes no more rows
 * than the caller gave it; rows it does not write stay 0. */
int smplx_test_path_waypoints(smplx_space* s, const double* a, const double* b, int n, const int32_t* first, double* out, int32_t* counts);

#ifdef __cplusplus
}
#endif
