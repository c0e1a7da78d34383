// smpl_amd/csrc/lattice_steps.h -- the steps of ManipLattice::GetSuccs that are not collision checks, one definition
// each for every expansion kernel.
// Owns: planning_fk, world_to_cell, metric_goal_distance, bfs_cost_to_goal, check_joint_limits, var_to_coord; the dispatch
// on the space's heuristic kind (closed_form_of, closed_form_goal_distance, closed_form_h; the arithmetic is heuristics.h);
// the device copy of the state table (table_probe_issue / table_probe_resolve, table_lookup, the insert functions and
// k_table_insert); mprim_gate / mprim_active, prim_has_action, successor_values, successor_goal_h.
// Restates: kdl_robot_model.cpp:173-235, 400-423; bfs_heuristic.cpp:129-138, 355-366;
// manip_lattice.cpp:1263-1354, 1596-1684; manip_lattice_action_space.cpp:551-621, 662-691.
#pragma once

#include "bfs_record.h"
#include "heuristics.h"
#include "model_lds.h"
#include "sphere_checks.h"   // const_planning_chain

// planning-link position and rotation (row-major 3x3) ("KDL" FK restated as the same serial chain;
// kdl_robot_model.cpp:400-423, continuous joints normalised first :191-198): what a pose goal tests and
// smplx_planning_pose_batch reports.  The chain and its T stay in this one function, the rotation an optional output:
// with T handed in by a caller, k_pipe_setup, k_pipe_prep and k_heuristic of the generic build lose an occupancy step
__device__ __forceinline__ void planning_fk(const ModelLds* __restrict__ M, const double* __restrict__ q, double p[3], double* R)
{
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
#ifdef SMPLX_CONST_MODEL
    const_planning_chain<0, true>(M, q, T);
#else
    bool first = true;
    const int nj = M->njoints;
    for (int j = 0; j < nj; ++j) {
        JointPtr jt = &M->joints[j];
        if (!jt->on_chain) continue;
        double qv = 0.0;
        if (jt->var >= 0) {
            qv = q[jt->var];
            if (MV_TYPE(M, jt->var) == SMPLX_JT_CONTINUOUS) qv = smplx_normalize_angle(qv);
        }
        apply_joint(jt, qv, T, first);
        first = false;
    }
#endif
    p[0] = T[3]; p[1] = T[7]; p[2] = T[11];
    if (R) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { R[3 * i] = T[4 * i]; R[3 * i + 1] = T[4 * i + 1]; R[3 * i + 2] = T[4 * i + 2]; }
    }
}

// ... its position alone: the same chain (the last joint's rotation is dead code)
__device__ __forceinline__ void planning_fk(const ModelLds* __restrict__ M, const double* __restrict__ q, double p[3])
{
    planning_fk(M, q, p, nullptr);
}

#ifdef SMPLX_CONST_MODEL
// ... with the sines and cosines of the (normalised) joint values handed in (sphere_checks.h const_planning_chain_sc)
__device__ __forceinline__ void planning_fk_sc(const ModelLds* __restrict__ M, const double* __restrict__ q, const double* __restrict__ sn,
                                               const double* __restrict__ cs, double p[3], double* R)
{
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
    const_planning_chain_sc<0, true>(M, q, sn, cs, T);
    p[0] = T[3]; p[1] = T[7]; p[2] = T[11];
    if (R) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { R[3 * i] = T[4 * i]; R[3 * i + 1] = T[4 * i + 1]; R[3 * i + 2] = T[4 * i + 2]; }
    }
}
#endif

__device__ __forceinline__ void world_to_cell(const SmplxGridDev& g, const double p[3], int c[3])
{
    c[0] = (int)(g.inv_res * (p[0] - g.origin_minus_res[0]) + 0.5) - 1;
    c[1] = (int)(g.inv_res * (p[1] - g.origin_minus_res[1]) + 0.5) - 1;
    c[2] = (int)(g.inv_res * (p[2] - g.origin_minus_res[2]) + 0.5) - 1;
}

// The heuristic kind of a space (device_types.h SmplxBfsDev, SmplxHeurDev).  closed_form_of is null for a space that plans
// with the BFS: the kernels test that one value, the same for every state of a space, and take the BFS code below
// unchanged.  Otherwise it is the space's heuristic record, which says which closed form (heuristics.h) stands in for the
// BFS's two functions:
//   getMetricGoalDistance, the gate of the primitives -- Euclidean: the distance of the planning link to the goal position;
//     joint distance: 0.0, so every state counts as "at the goal" (joint_dist_heuristic.cpp:52-55; kept, not repaired)
//   GetGoalHeuristic -- (int)(1000 * distance) of the state's pose, or of its joint values, to the goal's
// The generic kernels test at run time, per space.  A per-robot build knows when it compiles (specialize.cpp: a space of a
// closed-form kind gets a build of its own, CM_CLOSED_FORM): the build of the BFS spaces holds no dispatch at all and is,
// instruction for instruction, what it was without the closed forms (any test in front of or behind the chain cost the
// per-robot k_pipe_setup its fifth wave: profiles/heuristic_kinds_ab.txt); the other build holds no BFS arm.  Hence
// spaces that share a launch (smplx_plan_multi, multi_query.h same_scene_and_robot) are all BFS or all closed-form;
// the two closed forms may mix, their kind is read from the record.
__device__ __forceinline__ const SMPLX_GLOBAL_AS SmplxHeurDev* closed_form_of(const SmplxBfsDev& bfs)
{
#if defined(SMPLX_CONST_MODEL) && defined(CM_CLOSED_FORM)
    return as_global(bfs.heur);
#elif defined(SMPLX_CONST_MODEL)
    return nullptr;
#else
    return bfs.dim_x == 0 ? as_global(bfs.heur) : nullptr;
#endif
}
__device__ __forceinline__ bool closed_form_needs_fk(const SMPLX_GLOBAL_AS SmplxHeurDev* H) { return H->kind == SMPLX_HEUR_EUCLID; }
__device__ __forceinline__ double closed_form_goal_distance(const SMPLX_GLOBAL_AS SmplxHeurDev* H, const double p[3])
{
    return smplx_point_dist(p, (const double*)H->xyz);
}
__device__ __forceinline__ int closed_form_h(const ModelLds* __restrict__ M, const SMPLX_GLOBAL_AS SmplxHeurDev* H, const double p[3],
                                             const double R[9], const double* __restrict__ q)
{
    if (H->kind == SMPLX_HEUR_EUCLID)
        return smplx_fixed_h(smplx_pose_dist(p, R, (const double*)H->xyz, (const double*)H->rot, (const double*)H->w));
    if (!H->joint_goal) return 0;
    return smplx_fixed_h(smplx_joint_dist(q, (const double*)H->angles, MV_NVARS(M)));
}

// BfsHeuristic::getMetricGoalDistance (bfs_heuristic.cpp:129-138) of the state with joint values q: the gate of its
// primitives.  The one definition for every path; goal_distance_of_h (search_kernel.h, for round_prepare) recovers the same
// value from a state's heuristic and must keep the same distance for an unreachable cell.
__device__ __forceinline__ double metric_goal_distance(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                       const double* __restrict__ q)
{
    const SMPLX_GLOBAL_AS SmplxHeurDev* H = closed_form_of(bfs);
    if (H && !closed_form_needs_fk(H)) return 0.0;
    double p[3];
    planning_fk(M, q, p);
    if (H) return closed_form_goal_distance(H, p);
    int c[3];
    world_to_cell(grid, p, c);
    return !bfs_in_bounds(bfs, c) ? (double)0x7FFFFFFF * grid.res : (double)bfs_dist(bfs, c) * grid.res;
}

#ifdef SMPLX_CONST_MODEL
// ... from the state's sines and cosines (planning_fk_sc)
__device__ __forceinline__ double metric_goal_distance_sc(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                          const double* __restrict__ q, const double* __restrict__ sn,
                                                          const double* __restrict__ cs)
{
    const SMPLX_GLOBAL_AS SmplxHeurDev* H = closed_form_of(bfs);
    if (H && !closed_form_needs_fk(H)) return 0.0;
    double p[3];
    planning_fk_sc(M, q, sn, cs, p, nullptr);
    if (H) return closed_form_goal_distance(H, p);
    int c[3];
    world_to_cell(grid, p, c);
    return !bfs_in_bounds(bfs, c) ? (double)0x7FFFFFFF * grid.res : (double)bfs_dist(bfs, c) * grid.res;
}
#endif

#ifdef SMPLX_CONST_MODEL
// metric_goal_distance of the state with joint values q, and -- store -- the state's row of sines and cosines
// (sphere_checks.h parent_trig): the normalised ones are what the distance's chain evaluates anyway, the raw ones are
// evaluated where they can differ (a continuous variable outside [-pi, pi])
__device__ __forceinline__ double trig_row_and_goal_distance(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                             const double* __restrict__ q, double* __restrict__ trig_row, bool store)
{
    double sn[CM_NV], cs[CM_NV];
    trig_pair_t* row = reinterpret_cast<trig_pair_t*>(trig_row);
#pragma unroll
    for (int v = 0; v < CM_NV; ++v) {
        const double x = q[v];
        double xn = x;
        if (CM_VAR_TYPE[v] == SMPLX_JT_CONTINUOUS) xn = smplx_normalize_angle(x);
        sn[v] = 0.0; cs[v] = 0.0;   // a variable no SMPLX_TK_REV_*_T joint turns on: nobody reads its pairs, zeros are stored
        if ((CM_TRIG_ANY >> v) & 1u) smplx_sincos(xn, &sn[v], &cs[v]);
        double rs = sn[v], rc = cs[v];
        if (((CM_TRIG_ANY >> v) & 1u) && CM_VAR_TYPE[v] == SMPLX_JT_CONTINUOUS)
            if (__double_as_longlong(xn) != __double_as_longlong(x)) smplx_sincos(x, &rs, &rc);
        if (store) {
            trig_pair_t raw, nrm;
            raw.x = rs; raw.y = rc; nrm.x = sn[v]; nrm.y = cs[v];
            row[v] = raw; row[CM_NV + v] = nrm;
        }
    }
    return metric_goal_distance_sc(M, grid, bfs, q, sn, cs);
}
#endif

// BfsHeuristic::getBfsCostToGoal (bfs_heuristic.cpp:355-366)
__device__ __forceinline__ int bfs_cost_to_goal(const SmplxBfsDev& b, const int c[3])
{
    if (!bfs_in_bounds(b, c)) return 32767;
    const int d = bfs_dist(b, c);
    if (d == 0x7FFFFFFF) return 32767;
    return b.cost_per_cell * d;
}

// KDLRobotModel::checkJointLimits (kdl_robot_model.cpp:173-189, 210-235)
__device__ __forceinline__ bool check_joint_limits(const ModelLds* __restrict__ M, const double* __restrict__ q)
{
    const int nv = MV_NVARS(M);
    MV_UNROLL
    for (int v = 0; v < nv; ++v) {
        const double a_min = MV_MIN(M, v), a_max = MV_MIN_NORM(M, v);
        double a = q[v];
        if (fabs(a) > SMPLX_2PI) a = fmod(a, SMPLX_2PI);
        while (a > a_max) a -= SMPLX_2PI;
        while (a < a_min) a += SMPLX_2PI;
        if (a < MV_MIN(M, v) || a > MV_MAX(M, v)) return false;
    }
    return true;
}

// ManipLattice::stateToCoord for one variable (manip_lattice.cpp:1263-1289)
__device__ __forceinline__ int var_to_coord(const ModelLds* __restrict__ M, int v, double x)
{
    const double delta = MV_COORD_DELTA(M, v);
    const int ty = MV_TYPE(M, v);
    if (ty == SMPLX_JT_CONTINUOUS) {
        const double pos = smplx_normalize_angle_positive(x);
        int c = (int)((pos + delta * 0.5) / delta);
        if (c == MV_COORD_VALS(M, v)) c = 0;
        return c;
    }
    // bounded variables (every non-continuous variable of the plain-text model has limits)
    return (int)(((x - MV_MIN(M, v)) / delta) + 0.5);
}

// ManipLattice::getHashEntry (manip_lattice.cpp:1302-1316) against the device copy of the state table: state id of a
// discretised coordinate, -1 if the host has not committed it (yet)
// Inserts of the same launch may still be running (they ride at the head of the batch's first kernel): a slot whose tag
// is negative is being filled.  No slot between a coordinate's home and its own slot can have been empty since it was
// inserted, so meeting an empty or a busy slot first means the coordinate was not in the table before this launch.
// ConcurrentInserts: inserts may run in other workgroups of the SAME launch (k_small_batch: the extra blocks of
// table_insert_block).  In the pipeline the inserts ride with the first kernel and the lookups run in a later one, a
// kernel boundary behind them, where plain loads do (acquires there cost k_pipe_finish 15 -> 33 us, measured): that form
// is table_probe_issue + table_probe_resolve below, the whole slot in one round of 16-byte loads.
// A slot's tag and coordinate take (nv + 1 + 3) / 4 words of 16 bytes: SMPLX_TABLE_WORDS for the widest robot.  Loops over
// the words run to that bound and stop at the robot's own count, which a per-robot build knows when it compiles, so that
// the words a robot does not have cost it nothing.  smplx_table_stride pads a slot to a multiple of 32 bytes and the table
// comes from hipMalloc: every word is 16-byte aligned.
#define SMPLX_TABLE_WORDS ((SMPLX_MAX_VARS + 1 + 3) / 4)
static_assert(4 * SMPLX_TABLE_WORDS >= SMPLX_MAX_VARS + 1, "the words of a probe hold the tag and every coordinate of the widest robot");
static_assert(4 * SMPLX_TABLE_WORDS <= (SMPLX_MAX_VARS + 1 + 7) / 8 * 8, "... and lie inside its slot (smplx_table_stride)");
typedef int __attribute__((ext_vector_type(4))) table_int4;
struct TableSlotWords { table_int4 w[SMPLX_TABLE_WORDS]; unsigned int slot; };

// the whole slot in one round of plain 16-byte loads
__device__ __forceinline__ void table_slot_load(const SmplxTableDev& T, unsigned int slot, int nv, table_int4 w[SMPLX_TABLE_WORDS])
{
    const SMPLX_GLOBAL_AS table_int4* sl = (const SMPLX_GLOBAL_AS table_int4*)(as_global(T.slots) + (size_t)slot * T.stride);
    const int nw = (nv + 1 + 3) / 4;
#pragma unroll
    for (int k = 0; k < SMPLX_TABLE_WORDS; ++k) if (k < nw) w[k] = sl[k];
}
// every coordinate compared, no short circuit: nothing here waits for anything (c: global memory, registers or LDS)
template <class CoordPtr>
__device__ __forceinline__ bool table_slot_match(const table_int4 w[SMPLX_TABLE_WORDS], CoordPtr c, int nv)
{
    const int nw = (nv + 1 + 3) / 4;
    int differ = 0;
#pragma unroll
    for (int k = 0; k < SMPLX_TABLE_WORDS; ++k) {
        if (k >= nw) continue;
        const int base = 4 * k - 1;        // coordinate index of .x
        if (k > 0 && base < nv) differ |= w[k].x ^ c[base];
        if (base + 1 < nv) differ |= w[k].y ^ c[base + 1];
        if (base + 2 < nv) differ |= w[k].z ^ c[base + 2];
        if (base + 3 < nv) differ |= w[k].w ^ c[base + 3];
    }
    return differ == 0;
}

// The probe of a table that no workgroup of this launch writes (the inserts ran in an earlier launch: k_table_insert in
// front of k_step_block, a kernel boundary in the pipeline), cut in two after the pattern of issue_root / resolve_root
// (sphere_checks.h).  table_probe_issue hashes the coordinate and issues the loads of its home slot; it waits for
// nothing, so a caller can put other work behind it.  table_probe_resolve looks at those words and walks on, one slot a
// round, only where the home slot held another coordinate.  A slot whose tag is not positive is free (or, in a table that
// IS being written, being filled): a miss.
// (what resolves to a miss without a load: a free slot)
__device__ __forceinline__ TableSlotWords table_probe_none()
{
    TableSlotWords r;
#pragma unroll
    for (int k = 0; k < SMPLX_TABLE_WORDS; ++k) r.w[k] = table_int4{0, 0, 0, 0};
    r.slot = 0;
    return r;
}
__device__ __forceinline__ TableSlotWords table_probe_issue(const SmplxTableDev& T, const int* __restrict__ c, int nv)
{
    TableSlotWords r = table_probe_none();
    if (!T.slots) return r;               // no table: a miss
    r.slot = smplx_coord_hash(c, nv) & T.mask;
    table_slot_load(T, r.slot, nv, r.w);
    return r;
}
__device__ __forceinline__ int table_probe_resolve(const SmplxTableDev& T, const int* __restrict__ c, int nv, TableSlotWords ld)
{
    while (true) {
        const int tag = ld.w[0].x;
        if (tag <= 0) return -1;          // free, or being filled: a miss (the host resolves misses)
        if (table_slot_match(ld.w, c, nv)) return tag - 1;
        ld.slot = (ld.slot + 1) & T.mask;
        table_slot_load(T, ld.slot, nv, ld.w);
    }
}

template <bool ConcurrentInserts>
__device__ __forceinline__ int table_lookup(const SmplxTableDev& T, const int* __restrict__ c, int nv)
{
    if constexpr (!ConcurrentInserts) return table_probe_resolve(T, c, nv, table_probe_issue(T, c, nv));
    if (!T.slots) return -1;
    unsigned int i = smplx_coord_hash(c, nv) & T.mask;
    while (true) {
        const SMPLX_GLOBAL_AS int* sl = as_global(T.slots) + (size_t)i * T.stride;
        // k_small_batch: table_insert_item publishes the tag with a release after the coordinates, from another workgroup;
        // the tag is read with an acquire and the coordinates with loads that bypass this CU's L1, which is never refreshed
        // by another CU's stores -- a plain load could compare against a stale line (zeros, or half a coordinate) and
        // return another state's id
        const int tag = __atomic_load_n(&sl[0], __ATOMIC_ACQUIRE);
        if (tag <= 0) return -1;          // free, or being filled: a miss (the host resolves misses)
        bool same = true;
        for (int v = 0; v < nv; ++v) same = same && __atomic_load_n(&sl[1 + v], __ATOMIC_RELAXED) == c[v];
        if (same) return tag - 1;
        i = (i + 1) & T.mask;
    }
}

// ManipLattice::createHashEntry (manip_lattice.cpp:1318-1354), device side: the host assigns ids in commit order and
// sends the (query, id, coordinate) triples of the states created since the last batch; a slot is claimed with one CAS
// on its tag and filled afterwards (lookups run in later launches of the same stream).  items: n x (nvars + 2) int32.
__device__ __forceinline__ void table_insert_item(const SmplxSpaceDev* __restrict__ S, const SmplxSpaceDev* const* __restrict__ stab,
                                                  const int* __restrict__ it, int nvars)
{
    const SmplxTableDev T = (stab ? stab[it[0]] : S)->table;
    if (!T.slots) return;
    const int id = it[1];
    int c[SMPLX_MAX_VARS];
    for (int v = 0; v < nvars; ++v) c[v] = it[2 + v];   // the items may live in pinned host memory: read them once
    unsigned int k = smplx_coord_hash(c, nvars) & T.mask;
    while (true) {
        SMPLX_GLOBAL_AS int* sl = as_global(T.slots) + (size_t)k * T.stride;
        // claim with a negative ("busy") tag, fill, publish: a concurrent lookup never sees a half-written slot as a hit
        if (atomicCAS((int*)&sl[0], 0, -(id + 1)) == 0) {
            for (int v = 0; v < nvars; ++v) __atomic_store_n(&sl[1 + v], c[v], __ATOMIC_RELAXED);
            __atomic_store_n(&sl[0], id + 1, __ATOMIC_RELEASE);
            return;
        }
        k = (k + 1) & T.mask;
    }
}

// bulk inserts (k_table_insert): every thread of the launch takes its share
__device__ __forceinline__ void table_insert_items(const SmplxSpaceDev* __restrict__ S, const SmplxSpaceDev* const* __restrict__ stab,
                                                   const int* __restrict__ items, int n, int nvars)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) table_insert_item(S, stab, items + (size_t)i * (nvars + 2), nvars);
}

// The inserts that ride with a batch's first kernel take EXTRA blocks behind the `first_block` working ones, so they run
// beside the batch instead of in front of it (a lookup that misses one of them just reports "unknown").  Returns true
// for such a block: the caller returns at once.
__device__ __forceinline__ bool table_insert_block(const SmplxSpaceDev* __restrict__ S, const SmplxSpaceDev* const* __restrict__ stab,
                                                   const int* __restrict__ items, int n, int first_block)
{
    if ((int)blockIdx.x < first_block) return false;
    const int i = ((int)blockIdx.x - first_block) * (int)blockDim.x + (int)threadIdx.x;
    const int nvars = S->model.nvars;
    if (i < n) table_insert_item(S, stab, items + (size_t)i * (nvars + 2), nvars);
    return true;
}

extern "C" __global__ void __launch_bounds__(BLOCK)
k_table_insert(const SmplxSpaceDev* __restrict__ S, const SmplxSpaceDev* const* __restrict__ stab, const int* __restrict__ items,
               int n, int nvars)
{
    table_insert_items(S, stab, items, n, nvars);
}

// manip_lattice_action_space.cpp:662-691 in two steps.  mprim_gate loads what the gate of a primitive of kind `type` needs
// from the action record -- constants of the launch, so a kernel loads them at its head, beside its other first loads --
// and mprim_active decides from them and the state's goal distance.  A long primitive is gated by the SHORT kind's
// switch and threshold, every other kind by its own.
struct MprimGate { int type, use_long_and_short, enabled; double thresh; };
__device__ __forceinline__ MprimGate mprim_gate(const SmplxActionsDev& A, int type)
{
    const int kind = type == SMPLX_MP_LONG ? SMPLX_MP_SHORT : type;
    MprimGate g;
    g.type = type;
    g.use_long_and_short = A.use_long_and_short;
    g.enabled = A.enabled[kind];
    g.thresh = A.thresh[kind];
    return g;
}
__device__ __forceinline__ bool mprim_active(const MprimGate& g, double goal_dist)
{
    const bool near_goal = goal_dist <= g.thresh;
    if (g.type == SMPLX_MP_LONG) return g.use_long_and_short || !(g.enabled && near_goal);
    if (g.type == SMPLX_MP_SHORT && g.use_long_and_short) return g.enabled != 0;
    return g.enabled && near_goal;
}
__device__ __forceinline__ bool mprim_active(const SmplxActionsDev& A, double goal_dist, int type)
{
    return mprim_active(mprim_gate(A, type), goal_dist);
}

// can the primitive produce an action at all (a snap needs a joint-space goal: manip_lattice_action_space.cpp:551-559)
__device__ __forceinline__ bool prim_has_action(const SmplxActionsDev& A, const SmplxGoalDev& G, int p)
{
    const int ty = A.type[p];
    return ty == SMPLX_MP_LONG || ty == SMPLX_MP_SHORT || (ty == SMPLX_MP_SNAP_XYZ_RPY && G.type == SMPLX_GOAL_JOINT);
}

// Joint values of the successor of `parent` under primitive pi -> sq (global memory, registers or LDS).  Returns
// prim_has_action: false, with sq untouched, where the primitive has no action for this goal type.  The one definition
// for every path; host_apply_prim (engine.hip) mirrors its first branch.
__device__ __forceinline__ bool successor_values(const ModelLds* __restrict__ M, const SmplxActionsDev& A, const SmplxGoalDev& G,
                                                 int pi, const double* __restrict__ parent, double* __restrict__ sq)
{
    const int nv = MV_NVARS(M);
    const int type = A.type[pi];
    if (type == SMPLX_MP_LONG || type == SMPLX_MP_SHORT) {
        // applyMotionPrimitive (manip_lattice_action_space.cpp:575-621)
        double d0 = A.delta[pi][0], d1 = nv > 1 ? A.delta[pi][1] : 0.0;
        if (A.xy_rotate_by_var3 && nv > 3) {
            double s, c;
            smplx_sincos(parent[3], &s, &c);
            const double a0 = d0, a1 = d1;
            d0 = c * a0 + (-s) * a1;
            d1 = s * a0 + c * a1;
        }
        MV_UNROLL
        for (int v = 0; v < nv; ++v) {
            const double d = v == 0 ? d0 : (v == 1 ? d1 : A.delta[pi][v]);
            sq[v] = d + parent[v];
        }
        return true;
    }
    if (type == SMPLX_MP_SNAP_XYZ_RPY && G.type == SMPLX_GOAL_JOINT) {
        MV_UNROLL
        for (int v = 0; v < nv; ++v) sq[v] = G.angles[v];   // :551-559
        return true;
    }
    return false;
}

// Goal test and heuristic of the successor with joint values sq and coordinates sc: planning-link FK, isGoal, BFS cost of
// its cell -- or, in a space of a closed-form kind, closed_form_h of the same pose.  Returns h.  The one definition for every path; discretisation and the table probe stay
// with the callers.
// SC (per-robot build): sn, cs = the sines and cosines the planning-link chain would evaluate (planning_fk_sc).
template <bool SC = false>
__device__ __forceinline__ int successor_goal_h(const ModelLds* __restrict__ M, const SmplxGoalDev& G, const SmplxBfsDev& bfs,
                                                const SmplxGridDev& grid, const double* __restrict__ sq, const int* sc,
                                                bool& is_goal, const double* sn = nullptr, const double* cs = nullptr)
{
    const int nv = MV_NVARS(M);
    double p[3], R[9];
#ifdef SMPLX_CONST_MODEL
    if constexpr (SC) planning_fk_sc(M, sq, sn, cs, p, R);
    else
#endif
    planning_fk(M, sq, p, R);
    if (G.type == SMPLX_GOAL_JOINT) {      // manip_lattice.cpp:1596-1606
        is_goal = true;
        MV_UNROLL
        for (int v = 0; v < nv; ++v)
            if (fabs((double)(sc[v] - G.coord[v])) > G.angle_tol[v]) is_goal = false;
    } else {                               // the position box of both pose goals :1632-1637, :1682-1684
        is_goal = fabs(p[0] - G.xyz[0]) <= G.xyz_tol[0] && fabs(p[1] - G.xyz[1]) <= G.xyz_tol[1] &&
                  fabs(p[2] - G.xyz[2]) <= G.xyz_tol[2];
        // XYZ_RPY :1652-1667: the angle theta between the link's rotation and the goal's is below the tolerance iff
        // 4 cos^2(theta / 2) = 1 + trace(Rg^T R) is above the goal's rpy_c4 (device_types.h SmplxGoalDev)
        if (G.type == SMPLX_GOAL_XYZ_RPY && is_goal) {
            double t = 1.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) t += G.rot[i] * R[i];
            is_goal = t > G.rpy_c4;
        }
    }
    if (const SMPLX_GLOBAL_AS SmplxHeurDev* H = closed_form_of(bfs)) return closed_form_h(M, H, p, R, sq);
    int c[3];
    world_to_cell(grid, p, c);
    return bfs_cost_to_goal(bfs, c);
}
