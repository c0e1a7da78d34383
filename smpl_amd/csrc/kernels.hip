// smpl_amd/csrc/kernels.hip -- the one device translation unit: gfx950 (CDNA4, wave64) kernels of the ARA*
// state-expansion path.  The code is in the headers below, one concern each, included in dependency order; the per-robot
// build (specialize.cpp) compiles this same file with SMPLX_CONST_MODEL set, against the sources embedded in the library.
//
//   bfs_record.h        one cell of the BFS distance field out of its brick-major records
//   model_lds.h         joint mathematics, the MV_* macros, the model image staged into LDS (ModelLds, ThreadLds)
//   sphere_checks.h     voxel lookup, sphere tree vs grid, link pairs; the per-robot (SMPLX_CONST_MODEL) chain
//   attached_bodies.h   bodies attached to links, checked behind the robot's own trees and pairs
//   config_checks.h     config_valid (isStateValid), edge_waypoint_count, edge_valid (isStateToStateValid)
//   heuristics.h        the two closed-form heuristics' arithmetic, host and device (det_math.h)
//   lattice_steps.h     planning-link FK, goal distance, heuristic, limits, discretisation, the state table with
//                       k_table_insert, successor_values, successor_goal_h: one definition each for every kernel below
//   step_kernels.h      a frontier step.  Default: the waypoint-parallel pipeline k_pipe_setup -> k_pipe_configs ->
//                       k_pipe_finish (three launches; k_pipe_prep in front of them in the four-launch mode of large
//                       batches).  Also the fused pair k_state_prep + k_expand, one thread per (state, primitive)
//                       (manip_lattice.cpp:254-305 loop body), which the pipeline is checked against
//   step_block.h        k_step_block: the same step in ONE launch for a batch whose blocks are resident in one round;
//                       each block owns 128 edges and keeps everything between its phases in LDS
//   small_batch.h       k_small_batch: one block per state, and the lane functions k_search is built from
//   query_kernels.h     k_edge_valid, k_state_valid, k_heuristic, k_heuristic_closed, k_planning_pose, k_sphere_positions,
//                       k_attached_positions, k_bfs_metric: batch queries of the C-ABI
//   clearance.h         distance to collision of a configuration and of an edge: leaf spheres against the grid, branch
//                       and bound over the checked pairs and the attached bodies
//   clearance_kernels.h k_state_clearance, k_edge_clearance: the clearance queries of the C-ABI
//   lazy_kernels.h      k_lazy_succs, k_true_cost: GetLazySuccs and GetTrueCost, an expansion without its checks and the
//                       checks of one (parent, child) pair
//   path_kernels.h      k_shortcut, k_paths_valid, k_path_waypoints: post-processing of a batch of paths, the shortcut loop
//                       one workgroup per path, run to the end on the device
//   bfs_kernels.h       k_bfs_*: label-correcting 26-connected BFS over 8x8x8 bricks (bfs3d.cpp:507-547)
//   search_kernel.h     k_search: device-resident ARA*, one persistent workgroup per query, and the pieces of its step; it
//                       includes search_heap.h (OPEN: the wave-parallel binary heap, k_heap_ops) and search_table.h (the
//                       state table as the search's workgroup probes and fills it, k_search_table_fill, k_table_probe_ops)
//
// No MFMA: the path is integer/byte gathers from the voxel grid plus a short serial FK chain in fp64.
// The sphere trees are staged in LDS; per-thread scratch (tree-root positions, saved link transforms,
// DFS stack) lives in LDS in structure-of-arrays form (conflict-free: lane i touches word i).
// Compile with -ffp-contract=off (arithmetic contract, det_math.h).
#ifndef __HIPCC_RTC__   // hiprtc (per-robot specialisation, specialize.cpp) brings its own runtime declarations
#include <hip/hip_runtime.h>
#endif

#include "kernels.h"

#define BLOCK SMPLX_BLOCK

#include "bfs_record.h"
#include "model_lds.h"
#include "sphere_checks.h"
#include "attached_bodies.h"
#include "config_checks.h"
#include "lattice_steps.h"
#include "step_kernels.h"
#include "step_block.h"
#include "small_batch.h"
#include "query_kernels.h"
#include "clearance.h"
#include "clearance_kernels.h"
#include "lazy_kernels.h"
#include "path_kernels.h"
#include "bfs_kernels.h"
#include "search_kernel.h"
