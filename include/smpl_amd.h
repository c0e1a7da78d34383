/* include/smpl_amd.h -- C-ABI of the MI355X-native ARA* state-expansion engine for smpl.
 *
 * This is the drop-in boundary: plain pointers and sizes, opaque handles, int status codes,
 * nothing thrown across it.  Each entry point names the reference interface it stands behind
 * (paths relative to the dyouakim/smpl tree).  INTEGRATION.md shows the C++ shims a maintainer
 * adds on the smpl side (include/smpl_amd/plugin.hpp holds them ready-made).
 *
 * Conventions
 *   - every function returns SMPLX_OK (0) or a negative SMPLX_E_* code; smplx_last_error() gives text
 *   - q / state arrays hold the planning variables in planning-joint order (RobotState,
 *     smpl/include/smpl/types.h:66)
 *   - host pointers are copied during the call; "_device" variants take pointers into HBM and a
 *     hipStream_t (passed as void*) and do not synchronise
 *   - joint values handed in through host pointers must be finite with |q| < 1e6 (SMPLX_E_ARG otherwise: the limit
 *     folding of KDLRobotModel::checkJointLimits would not terminate on them); "_device" variants cannot check
 *   - calls on one handle are serialised by the caller, like the reference's single-threaded
 *     plugins (sbpl_collision_checking/src/collision_space.cpp:741-774 mutates state per query)
 */
#ifndef SMPL_AMD_H
#define SMPL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    SMPLX_OK = 0,
    SMPLX_E_ARG = -1,        /* bad argument */
    SMPLX_E_PARSE = -2,      /* robot / primitive text malformed */
    SMPLX_E_LIMIT = -3,      /* exceeds a compile-time capacity */
    SMPLX_E_HIP = -4,        /* HIP runtime error (no GPU, out of memory, ...) */
    SMPLX_E_STATE = -5,      /* call sequence error (goal/start not set, unknown id) */
    SMPLX_E_INVALID = -6     /* start state violates limits or is in collision */
};

typedef struct smplx_grid smplx_grid;     /* OccupancyGrid, lookup side */
typedef struct smplx_model smplx_model;   /* RobotCollisionModel + RobotModel as flat arrays */
typedef struct smplx_space smplx_space;   /* ManipLattice + BfsHeuristic + CollisionSpace, one query */

const char* smplx_last_error(void);
int smplx_device_count(void);

/* ---- voxel grid ---------------------------------------------------------------------------
 * sbpl::OccupancyGrid / DistanceMap, lookup side
 * (smpl/include/smpl/occupancy_grid.h:56-304; smpl/include/smpl/distance_map/detail/distance_map.hpp:281-300,520-536).
 * d2[nx*ny*nz]: squared cell distance to the nearest occupied or border cell, capped at
 * ceil(max_dist/res)^2 -- the `dist` field of the reference's cells (distance_map.h:115), x-major,
 * z fastest.  Stored in HBM as 16-bit values in 4x4x4 bricks. */
int smplx_grid_create(const double origin[3], int nx, int ny, int nz, double res, double max_dist,
                      const int32_t* d2, smplx_grid** out);
void smplx_grid_destroy(smplx_grid* g);

/* ---- voxel grid, construction side -----------------------------------------------------------------
 * OccupancyGrid::addPointsToField / removePointsFromField (smpl/src/occupancy_grid.cpp:357-422) over
 * DistanceMap::addPointsToMap / removePointsFromMap (distance_map.hpp:306-435): the field is built and kept on the
 * GPU.  Specified as the EXACT Euclidean transform with the reference's cap (ceil(max_dist/res) cells) and border rule
 * (the one-cell layer around the grid is occupied): d2 = min(dmax^2, min over occupied/border cells of |c - o|^2).
 * The reference's own bucketed propagation (distance_map.hpp:627-839) depends on its pop order where distances tie and
 * cannot be compiled here (Eigen): parity with it is unpinned; exactness is tested against brute force.
 * A new field takes three separable passes over the grid; an edit re-runs them on the window its cells can reach. */
int smplx_grid_create_empty(const double origin[3], int nx, int ny, int nz, double res, double max_dist, smplx_grid** out);
/* OccupancyGrid's ref_counted mode (smpl/include/smpl/occupancy_grid.h:66-74, initRefCounts occupancy_grid.cpp:424-441):
 * every cell keeps the number of times it was added; a cell becomes an obstacle when its count leaves 0 and free again
 * when it returns to 0 (a point listed twice counts twice; removing from a cell with count 0 does nothing).  Turning it
 * on gives every occupied cell the count 1. */
int smplx_grid_set_ref_counted(smplx_grid* g, int on);
/* boxes: n x {cx, cy, cz, sx, sy, sz} (world metres), the objects of a scene file (smpl_test/src/call_planner.cpp:158-207):
 * a box occupies the cells from the cell of its low corner to the cell of its high corner */
int smplx_grid_add_boxes(smplx_grid* g, const double* boxes, int n);
/* xyz: n world points (voxel centres); points outside the grid are skipped (distance_map.hpp:312-316) */
int smplx_grid_add_points(smplx_grid* g, const double* xyz, int n);
int smplx_grid_remove_points(smplx_grid* g, const double* xyz, int n);
/* OccupancyGrid::updatePointsInField -> DistanceMap::updatePointsInMap (occupancy_grid.cpp:408-415, distance_map.hpp:367-435):
 * as sets of cells, the obstacles in old \ new are removed and those in new \ old added; like the reference's it does not
 * touch the reference counts */
int smplx_grid_update_points(smplx_grid* g, const double* old_xyz, int n_old, const double* new_xyz, int n_new);
/* the reference counts, x-major / z fastest like d2 (SMPLX_E_STATE when the grid keeps none) */
int smplx_grid_copy_counts(const smplx_grid* g, int32_t* counts);
/* cells the last edit recomputed: the bounding box of the changed cells grown by ceil(max_dist / res) along every axis (an
 * edit is incremental, like the reference's propagation), or the whole grid when that box covers more than half of it */
long long smplx_grid_last_edit_cells(const smplx_grid* g);
/* EDITS AND SPACES.  CollisionChecker queries (smplx_cc_*, smplx_expand_batch) read the field as it is.  A planning space,
 * however, caches successor lists (the reference's ManipLattice re-evaluates every GetSuccs), and its BFS walls are those of
 * the field it was created on (BfsHeuristic::syncGridAndBfs runs once, at init: bfs_heuristic.cpp:52-71, 331-353 -- the
 * reference's heuristic has the same staleness).  After an edit, smplx_get_succs / smplx_plan* on a space of that grid
 * return SMPLX_E_STATE until the goal is set again (which restarts the lattice); re-create the space to get new walls.
 * Coordinates must be finite with |x| < 1e6 (SMPLX_E_ARG). */
/* the field as smplx_grid_create takes it: d2[nx*ny*nz], x-major, z fastest */
int smplx_grid_copy_d2(const smplx_grid* g, int32_t* d2);

/* ---- world objects --------------------------------------------------------------------------------------------------
 * CollisionSpace::insertObject / removeObject / moveShapes / insertShapes / removeShapes
 * (sbpl_collision_checking/src/collision_space.cpp:228-275) over WorldCollisionModel
 * (src/world_collision_model.cpp:193-280): named objects made of shapes at poses, voxelised on the GPU and kept in a
 * registry on the grid.
 * Every shape becomes a triangle mesh on the host exactly as the reference builds it (smpl/src/geometry/mesh_utils.cpp:
 * box :39-112, sphere with 7 x 8 lines :116-204, cylinder with 16 rim points :208-264, cone :268-299; a MESH is the
 * caller's vertices and index triples), its vertices go through the pose (R v + t, voxelize.cpp:608-615), and the
 * SURFACE of the mesh is voxelised (fill = false, voxel_operations.cpp:319-402) by VoxelizeTriangle
 * (smpl/include/smpl/geometry/detail/voxelize.hpp:46-180) on the PivotVoxelGrid whose pivot is the grid's origin
 * (voxelize.cpp:1008-1035): voxel index i along an axis is cell i of the grid.  The arithmetic is the reference's, in
 * binary64 without fused multiply-add, quirks included (edge p1-p2 of a triangle is never tested on its own).
 * A shape's cell list holds each filled cell once, in ExtractVoxels order (x-major, z fastest, voxelize.cpp:207-222).
 * Deliberate difference: only cells inside the grid are kept -- every triangle's candidate range is clipped to the grid
 * -- where the reference keeps the outside points and addPointsToMap skips them (distance_map.hpp:312-316); the field is
 * the same and a huge off-grid mesh cannot ask for an unbounded mask.
 *
 * An OCTREE (the planning scene's octomap: collision_space.cpp:154-156, 285-288, world_collision_model.cpp:303-330,
 * 434-470) is no mesh.  It holds the occupied leaves of an octree as rows {cx, cy, cz, size} -- centre and edge length in
 * the octree's own frame, in the order the caller's octomap library yields them (begin_leafs()); the engine links no
 * octomap code and reads no .bt / .ot files -- and is voxelised as VoxelizeOcTree does it (voxel_operations.cpp:405-436),
 * in binary64 without fused multiply-add, leaf by leaf: a leaf with size <= res gives one point, its centre; any other
 * gives c = ceil(size / res) * res and three nested loops, x outermost and z innermost, each
 * `for (v = centre - c; v < centre + c; v += res)`, so the value at step k is the k-fold running sum and the trips are
 * what that sum yields against `<` (2 c / res, or one more).  The reference samples twice the leaf's width; so does
 * this.  Every point goes through the pose like a mesh vertex (R v + t) and through the point rule of
 * smplx_grid_add_points (OccupancyGrid::worldToGrid) to a cell; points whose cell lies outside the grid are dropped (the
 * deliberate difference above).  The cell list of an OCTREE is the remaining cells in that generation order, DUPLICATES
 * KEPT -- the reference stores and adds every point -- so on a reference-counted grid a cell hit k times counts k, and
 * remove takes the same k out again.  Only the leaf rows cross to the device: trips, prefix sums, points and the
 * order-preserving compaction are kernels (smpl_amd/csrc/octree_points.h, world_objects.h).
 *
 * pose: 3x4 row major (rotation | translation), world frame, like smplx_planning_pose_batch.  Planes are not supported
 * (SMPLX_E_ARG, like any unknown type; the reference's VoxelizeShape does not voxelise them either).
 * Refused with SMPLX_E_ARG: a null pointer, an empty id or one with a line break, n < 1, an unknown shape type,
 * non-finite numbers (|x| >= 1e6), a dimension <= 0, a MESH without vertices or triangles or with an index outside
 * [0, nvertices), an OCTREE without leaves (null vertices or nvertices < 1), with triangles (non-null, or ntriangles
 * != 0) or with a leaf of size <= 0, an id already in the world (checkObjectInsert, world_collision_model.cpp:394-407)
 * and, for remove and move, an id that is not (checkObjectRemove :414-417).  SMPLX_E_STATE: a grid created from a
 * finished field (smplx_grid_create), which refuses objects as it refuses points.  SMPLX_E_LIMIT, before anything is
 * allocated or launched: an OCTREE leaf with size / res > 1024, more than 2^28 leaves in one call, or a bound on the
 * call's sample points -- (2 ceil(size / res) + 1)^3 summed over its leaves, 1 for a leaf of size <= res -- above the
 * voxeliser's cap of 2^31 / 3 cells in one call.  A refused call changes nothing.
 *
 * insert adds each shape's list in order (:227-231): on a reference-counted grid a cell covered by two shapes counts
 * twice.  remove takes the stored lists out again (:241-262): WITHOUT reference counts this frees cells another object
 * also covers, exactly like the reference.  move is the reference's moveShapes / insertShapes / removeShapes (:264-280,
 * all three are remove-then-insert with the new shape list) done as ONE field edit: both occupancy changes are applied,
 * then the field is updated once over the union of the two windows; field and counts equal remove followed by insert.
 * Every edit follows EDITS AND SPACES above; an object whose shapes lie wholly outside the grid is a valid edit that
 * changes no cell.  Cell lists stay on the device; smplx_world_object_cells copies one on request. */
enum { SMPLX_SHAPE_BOX = 1, SMPLX_SHAPE_SPHERE = 2, SMPLX_SHAPE_CYLINDER = 3, SMPLX_SHAPE_CONE = 4, SMPLX_SHAPE_MESH = 5,
       SMPLX_SHAPE_OCTREE = 6 };
typedef struct {
    int32_t type;            /* SMPLX_SHAPE_BOX / SPHERE / CYLINDER / CONE / MESH / OCTREE */
    double dims[3];          /* box: x y z;  sphere: r;  cylinder, cone: r, height;  mesh, octree: ignored */
    double pose[12];         /* 3x4 row major, world frame, like smplx_planning_pose_batch; OCTREE: the octomap's origin */
    const double* vertices;  int32_t nvertices;    /* MESH: nvertices x 3;  OCTREE: nvertices leaf rows of cx, cy, cz, size */
    const int32_t* triangles; int32_t ntriangles;  /* MESH only: ntriangles x 3 indices;  OCTREE: NULL and 0 */
} smplx_shape;
int smplx_world_insert_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n);
int smplx_world_remove_object(smplx_grid* g, const char* id);
int smplx_world_move_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n);
int smplx_world_remove_all(smplx_grid* g);
/* the ids in insertion order, one per line; *n = their number; names (cap bytes, NUL-terminated, truncated when too
 * small) may be NULL with cap 0 */
int smplx_world_objects(const smplx_grid* g, char* names, int cap, int* n);  /* '\n'-separated, insertion order */
/* the cell list of one shape of an object: *n = its length, the first min(cap, *n) cells are copied (cells may be NULL
 * with cap 0); SMPLX_E_ARG for an unknown id or shape index.  The analytic shapes and meshes list each cell once, in
 * ExtractVoxels order; an OCTREE lists one cell per sample point inside the grid, in generation order, so a cell appears
 * as often as points fell into it */
int smplx_world_object_cells(const smplx_grid* g, const char* id, int shape, int32_t* cells /* n x 3 */, int cap, int* n);
/* runs the voxeliser and changes nothing (any grid, also one from a finished field): first[s] .. first[s + 1] is the
 * range of shape s in the lists laid back to back; the first min(cap, first[n]) cells are copied.  Like the edits it
 * uses the grid's voxeliser work space (kept on the device, grown on demand): one world call at a time per grid */
int smplx_world_voxelize(const smplx_grid* g, const smplx_shape* shapes, int n, int32_t* cells, int cap, int32_t* first /* n+1 */);

/* ---- robot body: the links outside the planning group as obstacles ---------------------------------------------------
 * SelfCollisionModelImpl::updateGroup / updateVoxelsStates (sbpl_collision_checking/src/self_collision_model.cpp:616-760,
 * 770-837): every link that has a voxel model (CollisionVoxelsModel, robot_collision_model.cpp:566-573) and is not in
 * the planning group is voxelised into the occupancy grid and kept there as the robot's other joints move.
 *
 * The body is a host record beside the model, described by a text in the style of the robot text (DESIGN.md sections 4
 * and 20): the robot text's `link` and `joint` rows, plus
 *     geom LINK box SX SY SZ | sphere R | cylinder R LENGTH | mesh NV NT     x y z  r p y
 *         one <collision> element: the shape, then its origin in the link frame; a mesh is followed by NV rows
 *         "v x y z" and NT rows "t a b c"
 *     voxels LINK RES       the link has a voxel model at this resolution
 *     group NAME LINK ...   the planning group's links: their voxel models are never placed
 *     value JOINT Q         the joint's position at creation (default 0)
 * Limits (SMPLX_E_LIMIT beyond them): SMPLX_BODY_MAX_LINKS links, SMPLX_BODY_MAX_MODEL_POINTS voxels in one model (and
 * vertices or triangles in one mesh), SMPLX_BODY_MAX_POINTS voxels in all models, SMPLX_BODY_MAX_LATTICE lattice cells
 * in the bounding box of one geom.  There is no limit of 40 joints: the body is not part of the device model.
 *
 * Link transforms are computed on the host in binary64 with the arithmetic of the group's links (the root link's frame
 * is the world's; T_child = T_parent * fn(origin, axis, q), transform_functions.h:95-258; prismatic joints move along
 * the joint frame's Z).
 * Voxel models are built once, at smplx_body_create, on the GPU: RobotCollisionModel::voxelizeLink /
 * voxelizeCollisionElement / voxelizeGeometry (robot_collision_model.cpp:959-1073).  Each geom row of the link, in file
 * order, becomes the mesh the world objects use (box, sphere 7 x 8, cylinder with 16 rim points), goes through its
 * origin (R v + t) and its SURFACE is voxelised by the gridless VoxelizeMesh (smpl/src/geometry/voxelize.cpp:962-986):
 * VoxelizeTriangle on the HalfResVoxelGrid over the mesh's bounding box (discretize.h:94-113, voxel_grid.h:187-193), the
 * filled voxels as continuous link-frame points in ExtractVoxels order; the elements' points are appended one after
 * another, duplicates kept.  A link without geom rows has an empty model (the reference warns, :996-998).
 * Deliberate clip: the grid's high index is discretize(min + (max - min)), which can round below discretize(max); the
 * reference then indexes its grid past the end, here every triangle's candidates are clipped to the voxel grid's range.
 *
 * A voxels state is its model's points under the link's current transform (RobotCollisionState::updateVoxelsState,
 * robot_collision_state.h:473-497); every point then takes the point rule of smplx_grid_add_points, and one outside the
 * grid is skipped.  Every state starts dirty; smplx_body_set_joint with a value different from the current one dirties
 * the states of the joint's child link and all its descendants (robot_collision_state.cpp:62-96); the same value
 * dirties nothing.  smplx_grid_put_body places every dirty state of a link outside the group, in model order: the
 * state's stored cell list is taken out, the new one is computed, stored on the grid and added; then the field is
 * updated ONCE over the union of all windows (as smplx_world_move_object does).  With reference counts every point
 * counts (several points in one cell count several times); without them a removal frees cells a world object also
 * covers, like the reference and smplx_world_remove_object.  A put with nothing to place is not an edit; one that
 * changes cells follows EDITS AND SPACES above.  smplx_grid_take_body removes all stored lists and forgets the body.
 * Deliberate difference: the reference's updateGroup first inserts the states' initial voxels, still in the LINK frame
 * (robot_collision_state.cpp:264-266), and the first updateVoxelsStates removes them again, which frees world cells near
 * the origin on a grid without counts.  Here a state enters the grid transformed, and only so.
 *
 * The placement belongs to the grid: a grid holds at most one body (SMPLX_E_STATE for another one), the body handle may
 * be destroyed while placed, smplx_grid_destroy frees the lists, and a grid from a finished field refuses
 * (SMPLX_E_STATE).  SMPLX_E_ARG: null pointers, unknown names, non-finite numbers (|x| >= 1e6), res <= 0, dimensions
 * <= 0, a mesh index outside its vertices, a voxels or geom row on an unknown link, malformed rows -- the text's errors
 * name their line ("line N: ...") and are found before any GPU is touched.  A refused call changes nothing.
 * Out of scope: setWorldToModelTransform (it would move the group's spheres too), voxel models of attached bodies,
 * folding non-zero held joints into the group's model, loading mesh files, planar and floating joints. */
#define SMPLX_BODY_MAX_LINKS 4096
#define SMPLX_BODY_MAX_MODEL_POINTS 4000000
#define SMPLX_BODY_MAX_POINTS 16000000
#define SMPLX_BODY_MAX_LATTICE 268435456
typedef struct smplx_body smplx_body;
int smplx_body_create(const char* body_text, smplx_body** out);
void smplx_body_destroy(smplx_body* b);
/* models: links with a voxels row, in the order of those rows; outside: those that are placed; points: in all models */
int smplx_body_counts(const smplx_body* b, int* links, int* joints, int* models, int* outside_models, int* points);
int smplx_body_set_joint(smplx_body* b, const char* joint, double q);
int smplx_body_joint(const smplx_body* b, const char* joint, double* q);
/* world frames of all links in the order of the text's link rows, 3x4 row major each */
int smplx_body_link_transforms(const smplx_body* b, double* T /* nlinks x 12 */);
/* the link of a model: its index among the link rows */
int smplx_body_model_link(const smplx_body* b, int model, int* link);
/* the link-frame points of one model, in order: *n = their number, the first min(cap, *n) are copied */
int smplx_body_model_points(const smplx_body* b, int model, double* xyz /* n x 3 */, int cap, int* n);
int smplx_body_dirty(const smplx_body* b, uint8_t* per_model);
int smplx_grid_put_body(smplx_grid* g, smplx_body* b);
int smplx_grid_take_body(smplx_grid* g);
/* the stored list of one model: one cell per point in point order, a point outside the grid as (-1, -1, -1); *n = 0 for
 * a model that has no list (a group link's, or nothing placed yet) */
int smplx_grid_body_cells(const smplx_grid* g, int model, int32_t* cells /* n x 3 */, int cap, int* n);

/* ---- robot model --------------------------------------------------------------------------
 * RobotCollisionModel (sbpl_collision_checking/src/robot_collision_model.cpp:117-623),
 * sphere trees (base_collision_models.cpp:337-444), RobotMotionCollisionModel
 * (robot_motion_collision_model.cpp:41-275) and the planning RobotModel limits/FK
 * (sbpl_kdl_robot_model/src/kdl_robot_model.cpp:210-235,400-423) from a plain-text description
 * (format: DESIGN.md section 4). */
int smplx_model_create(const char* robot_text, smplx_model** out);
void smplx_model_destroy(smplx_model* m);
int smplx_model_counts(const smplx_model* m, int* njoints, int* nvars, int* ntrees, int* nnodes, int* npairs, int* nslots);
/* compiled arrays, for inspection: per joint (depth-first order) origin[12], k, file index;
 * per node xyz+r, left, right (global indices); tree_first[ntrees+1]; pairs[2*npairs] */
int smplx_model_joints(const smplx_model* m, double* origins, double* k, int* file_index);
int smplx_model_nodes(const smplx_model* m, double* xyzr, int* left, int* right, int* tree_first);
int smplx_model_pairs(const smplx_model* m, int* pairs);

/* ---- planning space ------------------------------------------------------------------------ */
typedef struct smplx_params {
    double resolutions[16];       /* PlanningParams "discretization" (smpl_ros/src/ros/planner_interface.cpp:149-181) */
    double bfs_inflation_radius;  /* planning_link_sphere_radius (smpl/include/smpl/planning_params.h:71) */
    int32_t cost_per_cell;        /* planning_params.h:68 */
    int32_t use_short_dist_mprims;
    double short_dist_mprims_thresh;
    int32_t use_xyzrpy_snap_mprim;    /* joint-space goals only: the action is the goal itself
                                         (manip_lattice_action_space.cpp:551-559) */
    double xyzrpy_snap_dist_thresh;
    int32_t xy_rotate_by_var3;        /* [FORK] manip_lattice_action_space.cpp:590-599 rotates delta[0], delta[1] by
                                         state[3] in every applyMotionPrimitive: 1 = the reference's behaviour (what
                                         every caller of this repo passes unless it asks for upstream smpl), 0 = upstream */
    int32_t use_long_and_short;
    double padding;                   /* SelfCollisionModel m_padding, default 0 */
    int32_t batch_states;             /* frontier batch B (0 = default 4096) */
    int32_t flags;                    /* SMPLX_SPACE_* bits below; 0 = defaults */
    int32_t heuristic;                /* SMPLX_H_* below: the heuristic the space plans with; 0 (a zero-initialised
                                         struct) = the BFS.  Any other value: SMPLX_E_ARG */
} smplx_params;

/* smplx_params.heuristic: PlannerInterface's search.heuristic.space for arastar + manip
 * (smpl_ros/src/ros/planner_interface.cpp:855-882).
 *   SMPLX_H_BFS         BfsHeuristic ("bfs").
 *   SMPLX_H_EUCLID      EuclidDistHeuristic ("euclid", its pose branch, euclid_dist_heuristic.cpp:124-141, 244-272):
 *                       h = (int)(1000 sqrt(wx dx^2 + wy dy^2 + wz dz^2 + wr theta^2)) between the planning link's pose
 *                       and the goal's, theta the angle between the two rotations in [0, pi]; weights 1 until
 *                       smplx_set_euclid_weights.  The goal rotation: a pose goal's rpy; for a joint goal the planning
 *                       link's rotation at the goal angles; the identity for smplx_set_goal_xyz.  The metric goal
 *                       distance, which gates the short and snap primitives, is the plain distance to the goal position.
 *                       theta comes from the rotation matrices (1 + trace = 4 cos^2(theta / 2)), not from the
 *                       reference's Euler angles and quaternions: parity of its last bits is unpinned, as for pose goals.
 *   SMPLX_H_JOINT_DIST  JointDistHeuristic ("joint_distance", joint_dist_heuristic.cpp): h = (int)(1000 |q - goal angles|),
 *                       raw joint values in variable order, no angle wrapping; 0 for every state unless the goal is a
 *                       joint goal.  Its metric goal distance is 0.0 everywhere, so the gate sees every state "at the
 *                       goal": short primitives and the snap are active on every expansion, long ones only with
 *                       use_long_and_short.  That is the reference's behaviour and is kept.
 * The goal id has h = 0 under every kind.  A space of a closed-form kind (the last two) has no BFS: it allocates no BFS
 * buffers, setting its goal runs none, smplx_bfs_size and smplx_bfs_levels return 0, and smplx_bfs_copy,
 * smplx_bfs_metric_goal_distance and smplx_bfs_metric_start_distance fail with SMPLX_E_STATE.  Everything else -- the
 * goals, smplx_get_succs, the lazy pair, smplx_plan*, smplx_replan*, both searches -- is the same call for every kind. */
enum { SMPLX_H_BFS = 0, SMPLX_H_EUCLID = 1, SMPLX_H_JOINT_DIST = 2 };

/* smplx_params.flags: which kernels serve the space.  Results are identical whatever the bits (the parity suite runs
 * every combination); they exist for A/B measurements and for callers that want the reference's own lookup tallies. */
enum {
    SMPLX_SPACE_FUSED = 1,            /* one GPU thread walks a whole edge in the reference's waypoint order (exact
                                         reference lookup tallies also on colliding edges); default: waypoint-parallel */
    SMPLX_SPACE_NO_SMALL_KERNEL = 4,  /* small batches (<= 512 states) go through the four-kernel pipeline too */
    SMPLX_SPACE_GENERIC_KERNELS = 8   /* no per-robot kernel build (see smplx_space_specialized) */
};

/* RobotPlanningSpace::init + insertHeuristic (smpl/include/smpl/graph/robot_planning_space.h:68,89;
 * smpl/src/graph/manip_lattice.cpp:72-149; smpl/src/heuristic/bfs_heuristic.cpp:52-71,331-353;
 * sbpl_collision_checking/src/collision_space.cpp:689-739).  mprim_text: .mprim file contents
 * (manip_lattice_action_space.cpp:103-195, upstream or fork rows). */
int smplx_space_create(const smplx_model* model, const smplx_grid* grid, const char* mprim_text,
                       const smplx_params* params, smplx_space** out);
/* the SMPLX_H_* kind the space was created with (SMPLX_E_ARG for a null space) */
int smplx_space_heuristic(const smplx_space* s);
void smplx_space_destroy(smplx_space* s);
/* 1 if the space runs kernels compiled for this robot: at creation the model's kinematic structure is turned into
 * compile-time constants and the kernels are built against them with hiprtc (cached per process and on disk under
 * $SMPLX_CACHE_DIR / $XDG_CACHE_HOME/smpl_amd / $HOME/.cache/smpl_amd); results are bit-identical to the generic
 * kernels'.  0: generic kernels (note says why).  Env SMPLX_SPECIALIZE=0 disables, =2 makes a failed build an error. */
int smplx_space_specialized(const smplx_space* s, char* note, int cap);
/* the constants header the per-robot build is compiled against (returns the size needed, including the NUL) */
int smplx_model_const_header(const smplx_model* m, char* out, int cap);
int smplx_space_num_vars(const smplx_space* s);
int smplx_space_num_prims(const smplx_space* s);
int smplx_space_discretization(const smplx_space* s, int32_t* coord_vals, double* coord_deltas);

/* RobotModel::checkJointLimits as KDLRobotModel implements it (sbpl_kdl_robot_model/src/kdl_robot_model.cpp:173-189,
 * 210-235: fold by 2*pi into [min, min + 2*pi), then compare with the limits); host arithmetic, n states */
int smplx_check_joint_limits(const smplx_space* s, const double* q, int n, uint8_t* ok);

/* ---- CollisionChecker (smpl/include/smpl/collision_checker.h:48-130) ---- */
/* isStateValid (collision_space.cpp:532-536) */
int smplx_cc_state_valid_batch(smplx_space* s, const double* q, int n, uint8_t* valid, int32_t* lookups);
/* same with everything resident in HBM: launches on `stream` (a hipStream_t) and returns without synchronising;
 * d_lookups may be NULL.  One launch = n configurations through FK + sphere trees vs grid + checked link pairs: the
 * "K2" collision micro-benchmark of sbpl_collision_checking_test/src/benchmark_cc.cpp:234-256 is a loop over this. */
int smplx_cc_state_valid_batch_device(smplx_space* s, const double* d_q, int n, uint8_t* d_valid, int32_t* d_lookups,
                                      void* stream);
/* isStateToStateValid (collision_space.cpp:538-581); lookups/waypoints may be NULL */
int smplx_cc_edge_valid_batch(smplx_space* s, const double* a, const double* b, int n, uint8_t* valid,
                              int32_t* lookups, int32_t* waypoints);
/* interpolatePath (collision_space.cpp:583-640): waypoints of the edge a->b, out holds cap*nvars doubles */
int smplx_cc_interpolate(smplx_space* s, const double* a, const double* b, double* out, int cap, int* n);
/* world positions of all sphere-tree nodes for n states: out[n][nnodes][3] (RobotCollisionState::updateSphereState) */
int smplx_cc_sphere_positions(smplx_space* s, const double* q, int n, double* out);

/* ---- CollisionDistanceExtension (smpl/include/smpl/collision_checker.h:132-144): distance to collision ----
 * How far a configuration, or an edge, is from collision and what is closest, in metres, fp64, bit-reproducible (the
 * arithmetic contract of DESIGN.md section 3; DESIGN.md section 16 has the whole specification).  The reference's own
 * CollisionSpace::collisionDistance is unfinished (self_collision_model.cpp:1386-1511, 1641), so there is no reference
 * value to equal; the terms are the reference's, the minimum over them is defined here.  For one configuration, with the
 * grid, the padding, the checked pairs and the attached bodies as smplx_cc_state_valid_batch uses them:
 *   world term of a LEAF sphere (of a robot tree or of an attached body) at world position p with radius r:
 *       res * sqrt((double)d2) - (r + padding),   d2 = the squared cell distance of p's cell, 0 outside the grid
 *     (SphereCollisionDistance, collision_operations.h:81-89, over distance_map.hpp:143-146).  The grid stores d2 only up
 *     to dmax_sqrd, so the term saturates at res * sqrt(dmax_sqrd) - (r + padding): a result at that cap means "at
 *     least".  A sphere outside the grid has the term -(r + padding).
 *   pair term of two leaf spheres at pa, pb with radii ra, rb (d = pb - pa):
 *       sqrt((dx*dx + dy*dy) + dz*dz) - (ra + rb)      (sphereDistance, self_collision_model.cpp:1644-1649; no padding)
 *     over exactly the pairs the validity check tests: leaf x leaf of every checked tree pair (smplx_model_pairs), every
 *     body against every robot tree not in its allowed list, every body against every later body unless either allows
 *     the other.
 *   world = min of the world terms, self = min of the pair terms (+infinity where there is none),
 *   clearance = min(world, self).  Inner nodes of the sphere trees contribute no term: only leaves are looked up.
 * parts (may be NULL): n x 2 {world, self}.  witness (may be NULL): n x 4 int32 {kind, a, b, waypoint}, a term that attains
 * the clearance (any of them where several tie):
 *   kind 0  robot leaf vs world      a = robot node (smplx_model_nodes order), b = -1
 *   kind 1  robot leaf vs robot leaf a = node of the group-earlier tree, b = node of the later one
 *   kind 2  body leaf vs world       a = body node (smplx_attached_nodes order), b = -1
 *   kind 3  body leaf vs robot leaf  a = body node, b = robot node
 *   kind 4  body leaf vs body leaf   a = node of the earlier body, b = node of the later one
 *   kind -1 no term at all (a = b = -1)
 * waypoint is 0 for a state.  For an edge a -> b everything is the minimum over the configurations isStateToStateValid
 * interpolates -- W waypoints, waypoint j at alpha = j * (1 / (W - 1)), the rows smplx_cc_interpolate returns -- each part
 * over all of them, and waypoint is the index of the one the witness belongs to.  An edge without motion (W == 0) answers
 * with its start configuration alone as waypoint 0; note that the edge CHECK visits nothing there and calls such an
 * edge valid whatever the configuration is.
 * Relation to validity, in one direction only: clearance > 1e-9 implies smplx_cc_state_valid_batch (for an edge:
 * smplx_cc_edge_valid_batch) says valid.  The converse does not hold: the reference's traversal looks at a leaf only when
 * all its ancestors fail, so a leaf may be in collision while an ancestor's lookup clears it.
 * Conventions of smplx_cc_state_valid_batch*: SMPLX_E_ARG for a null s / q / clearance, n < 0 and non-finite joint
 * values; n == 0 is SMPLX_OK and touches nothing; the _device form takes device pointers, launches on `stream` and does
 * not synchronise.  The calls read the field and the bodies as they are, need no goal, are not refused after a grid edit
 * or an attach, and leave a search that smplx_replan may resume untouched. */
int smplx_cc_state_clearance_batch(smplx_space* s, const double* q, int n, double* clearance,
                                   double* parts /* n x 2 {world, self}, may be NULL */,
                                   int32_t* witness /* n x 4, may be NULL */);
int smplx_cc_state_clearance_batch_device(smplx_space* s, const double* d_q, int n, double* d_clearance,
                                          double* d_parts, int32_t* d_witness, void* stream);
int smplx_cc_edge_clearance_batch(smplx_space* s, const double* a, const double* b, int n, double* clearance,
                                  double* parts, int32_t* witness);

/* ---- attached collision bodies (CollisionSpace::processAttachedCollisionObject -> attachObject / detachObject,
 * sbpl_collision_checking/src/collision_space.cpp:119-124, 297-345) ----
 * A body is a set of spheres (n x {x, y, z, r}, metres, in the frame of `link`) rigidly attached to a link of the
 * collision group.  The caller passes the spheres themselves (smplx_attach_body) or, as the reference's attachObject
 * does, shapes at poses that the engine voxelises into spheres on the GPU (smplx_attach_object, below).  The engine
 * builds the body's bounding sphere tree as it builds a link's (base_collision_models.cpp:337-444) and from then on every
 * state and edge check -- smplx_cc_*, the
 * start check of smplx_set_start, successor evaluation and both searches -- also checks the body:
 *   - against the grid, with the space's padding (collision_operations.h:67-77);
 *   - against every tree of the robot whose link is not in `allowed`, and against every other body unless either
 *     body lists the other's id in `allowed` (self_collision_model.cpp:1270-1345; leaf x leaf overlap = collision).
 *     The link the body hangs on is NOT implicitly allowed: list it (MoveIt's touch links).  Names in `allowed` that are
 *     neither a link nor an attached body are kept: they take effect when a body with that id is attached.
 * Motion-sphere factors and waypoint counts are those of the robot alone (the reference's RobotMotionCollisionModel).
 * Refused with SMPLX_E_ARG: an id already attached (or empty, or with white space), an unknown link, a link outside the
 * collision group (the reference would accept it and never check it); SMPLX_E_LIMIT above SMPLX_MAX_BODIES (8) bodies or
 * SMPLX_MAX_BODY_NODES (1024) tree nodes (n spheres make 2n - 1 nodes) per space.
 * An attach or detach acts like a grid edit (see EDITS AND SPACES above): smplx_get_succs / smplx_plan* return
 * SMPLX_E_STATE and smplx_replan* does not resume until the goal is set again.  It waits for the device to finish its
 * work (launches on the caller's streams included) before it changes the bodies' image. */
int smplx_attach_body(smplx_space* s, const char* id, const char* link, const double* spheres, int n, const char* const* allowed,
                      int nallowed);
/* CollisionSpace::attachObject(id, shapes, transforms, link_name) (collision_space.cpp:297-304): the object arrives as
 * shapes at poses in the frame of `link` (smplx_shape as for world objects, its pose relative to the link instead of the
 * world) and its sphere model is made on the GPU as AttachedBodiesCollisionModel::generateSpheresModel makes it
 * (attached_bodies_collision_model.cpp:264-313).  For shapes 0 .. n-1 in order: the mesh of the shape as for a world
 * object, its vertices through the pose; the SURFACE voxelised (fill = false) at res = radius / sqrt(2) on a
 * PivotVoxelGrid with pivot (0, 0, 0) that covers the mesh's own bounding box (voxelize.cpp:1008-1035; index range
 * [discretize(min), discretize(min + (max - min))], voxel_grid.h:174-196), indices negative where the mesh is, no cell
 * dropped; every filled voxel (i, j, k) in ExtractVoxels order gives the sphere {i * res, j * res, k * res, radius}.  The
 * shapes' lists lie back to back: a voxel two shapes fill gives two spheres.  The reference's radius is the constant
 * SMPLX_ATTACHED_SPHERE_RADIUS.
 * smplx_attach_object then leaves the space exactly as smplx_attach_body with those rows would: same nodes, same
 * `allowed`, same EDITS AND SPACES rule, same wait for the device; detach and the three queries below serve both kinds.
 * SMPLX_E_ARG: whatever smplx_attach_body refuses of id and link; whatever the world-object calls refuse of shapes (n < 1,
 * an unknown type, non-finite numbers, a dimension <= 0, bad mesh arrays); an OCTREE shape (nobody holds an octomap in a
 * gripper: octrees are world objects only, and the text names them); a radius that is not finite or <= 0; and
 * shapes that give no sphere at all (only degenerate triangles) -- the reference would attach an empty model that is never
 * checked, this refuses it.  SMPLX_E_LIMIT as for smplx_attach_body, the text giving the number of spheres the shapes
 * made, and for shapes whose index ranges hold more than 2^28 voxels.  A refused call changes nothing: bodies, device
 * image and query state stay, smplx_get_succs keeps working.
 * What fits: a surface makes about one sphere per 2 cm^2 at radius 0.025, and one body may have 512 spheres (1023 nodes),
 * so about 1000 cm^2 of surface: a 6 x 4 x 10 cm box makes 122 spheres, a 20 cm cube 1172 and is refused. */
#define SMPLX_ATTACHED_SPHERE_RADIUS 0.025
int smplx_attach_object(smplx_space* s, const char* id, const char* link, const smplx_shape* shapes, int n, double radius,
                        const char* const* allowed, int nallowed);
/* what smplx_attach_object would attach; changes nothing: first[k] .. first[k + 1] is shape k's range, the first
 * min(cap, first[n]) rows {x, y, z, r} are copied (xyzr may be NULL with cap 0).  Shapes that give no sphere are
 * SMPLX_OK here, with first[n] == 0.  Uses the space's voxeliser work space: one such call at a time per space */
int smplx_object_spheres(smplx_space* s, const smplx_shape* shapes, int n, double radius, double* xyzr, int cap,
                         int32_t* first /* n+1 */);
int smplx_detach_body(smplx_space* s, const char* id);            /* SMPLX_E_ARG for an id not attached */
/* the attached bodies in attach order: returns their number; names gets one "id link\n" line per body (cap bytes,
 * NUL-terminated, may be NULL with cap 0); first_node / nnodes (SMPLX_MAX_BODIES entries each, may be NULL): each body's
 * range of nodes in the order of smplx_attached_nodes and smplx_cc_attached_positions */
int smplx_attached_bodies(const smplx_space* s, char* names, int cap, int32_t* first_node, int32_t* nnodes);
/* returns the number of body tree nodes; xyzr[4 * count] (centre in the link frame, radius), left[count] and right[count]
 * (children, -1 for a leaf; a body's tree is stored in pre-order, root first) may be NULL */
int smplx_attached_nodes(const smplx_space* s, double* xyzr, int32_t* left, int32_t* right);
/* world positions of all body tree nodes for n states: out[n][count][3], the counterpart of smplx_cc_sphere_positions */
int smplx_cc_attached_positions(smplx_space* s, const double* q, int n, double* out);

/* ---- RobotHeuristic / BfsHeuristic (smpl/include/smpl/heuristic/robot_heuristic.h:53-101) ---- */
/* RobotPlanningSpace::setGoal with a JOINT_STATE_GOAL (manip_lattice.cpp:2248-2287; goal pose = FK of the
 * angles, planner_interface.cpp:1232-1235) -> BfsHeuristic::updateGoal -> BFS_3D::run to completion */
int smplx_set_goal_joint(smplx_space* s, const double* angles, const double* tolerances);
/* XYZ_GOAL (manip_lattice.cpp:1672-1687) */
int smplx_set_goal_xyz(smplx_space* s, const double xyz[3], const double tol[3]);
/* The goals of nq spaces in ONE call: smplx_set_goal_joint / smplx_set_goal_xyz for spaces[q] with row q of the arrays
 * (angles, tolerances: nq rows of the spaces' number of variables; xyz, tol: nq rows of 3).  The BFS runs of all goals
 * share one sequence of launches on the leading space's stream -- in every pass each goal's queued bricks are visited
 * side by side, each goal in its own space's grid -- where the single calls run about 45 narrow launches per goal one
 * goal after the other; the goal poses of joint goals come from one FK launch when the spaces run the same kernels
 * on the same model image.
 * Contract: afterwards every space is in exactly the state the single-goal call would have left it in -- goal record,
 * goal pose (bit-equal), BFS grid, metric distances, smplx_get_goal_heuristic(0), the lattice reset, the grid and
 * attached-body epochs -- so smplx_set_start, smplx_plan*, smplx_replan* and smplx_get_succs follow as usual, and a later
 * smplx_set_goal_* on any of the spaces is right as well.  The brick sweep is label-correcting: its fixed point, the exact
 * 26-connected hop counts, does not depend on the order or the launch in which bricks are visited.  The one visible
 * difference: smplx_bfs_levels returns the number of passes of the SHARED sequence, the same for every space of the call
 * (the longest goal's passes plus the empty pass that ends the sequence).
 * The spaces must live on one device and have the same number of 8x8x8 bricks per axis (and, for joint goals, of
 * variables); they need not share a grid handle, walls (a space keeps the walls of the grid as it was when the space
 * was created), robot or primitives.  nq = 1 is allowed and equals the single call.  The call allocates nothing that
 * grows with nq x grid size: every goal uses the buffers its space already holds.
 * All arguments are checked before any space is touched.  SMPLX_E_ARG: a null pointer, nq < 1, the same space twice
 * (checked on the handles alone), a non-finite value (|v| >= 1e6 for angles), spaces on different devices or with
 * different bricks per axis.  After a HIP error no space of the call has a goal: set the goals again. */
int smplx_set_goals_joint_multi(smplx_space** spaces, int nq, const double* angles /* nq x nvars */, const double* tolerances /* nq x nvars */);
int smplx_set_goals_xyz_multi(smplx_space** spaces, int nq, const double* xyz /* nq x 3 */, const double* tol /* nq x 3 */);
/* XYZ_RPY_GOAL (ManipLattice::isGoal, manip_lattice.cpp:1614-1671): the XYZ goal's position box, and inside it the angle
 * theta between the planning link's rotation and Rz(yaw) Ry(pitch) Rx(roll) of rpy must be below rpy_tol (the reference
 * reads rpy_tolerance[0] alone).  theta lies in [0, pi]: rpy_tol > pi admits every orientation (the goal then equals
 * the XYZ goal), rpy_tol <= 0 none.  The kernels test 1 + trace(Rg^T R) > 4 cos^2(rpy_tol / 2), the same predicate
 * without inverse trigonometry; smplx_rpy_angle is the reference's formula for callers.  Everything else is the XYZ
 * goal's: the BFS is seeded at xyz, snap primitives stay inactive, smplx_goal_pose returns xyz.  xyz is the pose the
 * reference calls tgt_off_pose: a GoalConstraint::xyz_offset is the caller's to apply.
 * SMPLX_E_ARG: a null pointer, a non-finite pose value (|xyz| >= 1e6, |rpy| >= 1e6), a NaN tolerance. */
int smplx_set_goal_pose(smplx_space* s, const double xyz[3], const double rpy[3], const double xyz_tol[3], double rpy_tol);
/* smplx_set_goal_pose for nq spaces in one call: contract and checks of smplx_set_goals_xyz_multi */
int smplx_set_goals_pose_multi(smplx_space** spaces, int nq, const double* xyz /* nq x 3 */, const double* rpy /* nq x 3 */,
                               const double* xyz_tol /* nq x 3 */, const double* rpy_tol /* nq */);
int smplx_goal_pose(const smplx_space* s, double xyz[3]);
/* roll, pitch, yaw and tolerance of a pose goal as they were given; SMPLX_E_STATE unless the goal is one */
int smplx_goal_orientation(const smplx_space* s, double rpy[3], double* rpy_tol);
/* the reference's orientation distance between two roll/pitch/yaw triples (manip_lattice.cpp:1652-1665: ZYX quaternions,
 * sign flip, 2 acos of the dot product), in [0, pi]; host arithmetic, needs no space */
int smplx_rpy_angle(const double a[3], const double b[3], double* theta);
/* computePlanningLinkFK for n states: the planning link's transform, row-major 3x4 each, by the FK the goal test and
 * the heuristic run (column 3 is bit-equal to smplx_heuristic_batch's xyz) */
int smplx_planning_pose_batch(smplx_space* s, const double* q, int n, double* T /* n x 12 */);
/* GetGoalHeuristic of the space's heuristic kind for arbitrary states (bfs_heuristic.cpp:148-163,
 * euclid_dist_heuristic.cpp:118-141, joint_dist_heuristic.cpp:70-88); xyz (n*3) may be NULL */
int smplx_heuristic_batch(smplx_space* s, const double* q, int n, int32_t* h, double* xyz);
/* setWeightX / Y / Z / Rot of a SMPLX_H_EUCLID space (euclid_dist_heuristic.cpp:78-96), w = {x, y, z, rot}.  The
 * reference's factory passes its x coefficient to all four setters (planner_interface.cpp:472-475): that is the caller's
 * to copy.  SMPLX_E_ARG: a negative or non-finite weight; SMPLX_E_STATE: the space's kind is not SMPLX_H_EUCLID.
 * Afterwards the space has no goal, as after a field edit: every h recorded so far used the old weights, so set the goal
 * again before any query. */
int smplx_set_euclid_weights(smplx_space* s, const double w[4]);
/* getMetricGoalDistance of the space's heuristic kind for n workspace points xyz[n*3]: the value the action space gates the
 * short and snap primitives on.  SMPLX_H_BFS: smplx_bfs_metric_goal_distance; SMPLX_H_EUCLID: the distance to the goal
 * position; SMPLX_H_JOINT_DIST: 0.0.  SMPLX_E_STATE without a goal. */
int smplx_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out);
/* The arithmetic of the two closed-form heuristics on the host, the very functions the kernels compile
 * (smpl_amd/csrc/heuristics.h); they need no space and no GPU.  (int)(1000 * dist) is the h of a state at pose Ta
 * (row-major 3x4, as smplx_planning_pose_batch gives it) under a goal at pose Tb with weights w = {x, y, z, rot}, and of a
 * state with joint values a under goal angles b.  SMPLX_E_ARG: a null pointer, a non-finite value, a negative weight,
 * n < 0 or n > 16. */
int smplx_pose_distance(const double Ta[12], const double Tb[12], const double w[4], double* dist);
int smplx_joint_distance(const double* a, const double* b, int n, double* dist);
/* BfsHeuristic::getMetricGoalDistance (bfs_heuristic.cpp:129-138) for n workspace points xyz[n*3]:
 * BFS cell distance * resolution, WALL * resolution outside the grid.  This is the value the action space gates the
 * short / snap primitives on (manip_lattice_action_space.cpp:393-397). */
int smplx_bfs_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out);
/* BfsHeuristic::getMetricStartDistance (bfs_heuristic.cpp:103-127): Manhattan cell distance to the cell of the start
 * state's planning link, times the resolution (needs smplx_set_start) */
int smplx_bfs_metric_start_distance(smplx_space* s, const double* xyz, int n, double* out);
/* the padded (nx+2)(ny+2)(nz+2) BFS_3D distance grid, node order of bfs3d.h:213-220.  A space of a closed-form heuristic
 * kind has none: smplx_bfs_size is 0 and smplx_bfs_copy, like the two calls above, fails with SMPLX_E_STATE. */
int64_t smplx_bfs_size(const smplx_space* s);
int smplx_bfs_copy(smplx_space* s, int32_t* out);
/* passes the last BFS took: sweeps over the queued 8x8x8 bricks (the device keeps the grid in brick-major records); after
 * smplx_set_goals_*_multi the passes of the shared sequence, the same for every space of the call */
int smplx_bfs_levels(const smplx_space* s);

/* ---- ManipLattice (smpl/include/smpl/graph/manip_lattice.h:63-307) ---- */
/* successor evaluation for B arbitrary parent states: the loop body of GetSuccs
 * (manip_lattice.cpp:254-305) for every (state, primitive), dense outputs indexed [state][prim]:
 * flags (SMPLX_F_* of device_types.h: 1 valid, 2 goal, 4 unchecked (smplx_lazy_expand_batch only), 0x10 inactive, 0x20 limits, 0x40 collision),
 * coord[nvars], q[nvars], h, cost, lookups.  Any output may be NULL.
 * Defined entries: flags everywhere; coord, h and cost where flags has the valid bit (h and cost are 0 elsewhere); q on every
 * edge that is not inactive; lookups on every edge not in collision (a colliding edge's tally stops at its first colliding
 * waypoint lane).  Other entries hold whatever the kernel that served the batch left there. */
int smplx_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q,
                       int32_t* h, int32_t* cost, int32_t* lookups);
/* same, everything resident in HBM; launches on `stream` and returns without synchronising.
 * work: device scratch of smplx_expand_work_bytes(s, B) bytes, 16-byte aligned.  d_counters: see smplx_counters_bytes (may be NULL). */
size_t smplx_expand_work_bytes(const smplx_space* s, int B);
/* d_counters: device scratch of smplx_counters_bytes(s, B) bytes, zeroed by the caller; tallies accumulate per
 * thread block without atomics.  smplx_counters_read sums them (synchronous copy): out[0] successor evaluations,
 * out[1] valid successors, out[2] grid lookups the reference algorithm makes for those edges, out[3] grid lookups
 * the edge kernels themselves issued (waypoint 0 is checked once per state), out[4] configurations checked by
 * k_pipe_configs (states + waypoints; 0 in fused mode), out[5] lookups of the per-state checks among them. */
size_t smplx_counters_bytes(const smplx_space* s, int B);
int smplx_counters_read(const smplx_space* s, const uint64_t* d_counters, int B, uint64_t out[6]);
int smplx_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord,
                              double* d_succ_q, int32_t* d_h, int32_t* d_cost, int32_t* d_lookups,
                              void* d_work, uint64_t* d_counters, void* stream);

/* ---- K5: state table on the device + compacted successor stream --------------------------------------------------
 * ManipLattice::getHashEntry / createHashEntry (manip_lattice.cpp:1302-1354).  Every space keeps a device copy of its
 * coordinate -> id table (open addressing over 32-byte slots).  Ids are still ASSIGNED by the host in the caller's
 * sequential commit order (that order is what makes them the reference's ids); the states committed since the last
 * batch are inserted on the device at the head of the next one.  The successor kernels look every valid successor's
 * coordinate up: a hit hands the id back with the batch and the host skips its own lookup when it commits the
 * successor; a miss (-1) means "not committed when the batch ran" and the host does getOrCreateState as before.
 * With the compact arguments the same launch also leaves the VALID successors as a stream built with wavefront
 * ballots (one atomic per region and thread block):
 *   region A, 8 bytes per valid successor: {id or -1, primitive | goal << 8 | state index in the batch << 9}
 *   region B, smplx_compact_rec_b_bytes() per successor the host needs in full (unknown coordinate, or goal successor):
 *             int32 h, int32 coord[nvars], padding to 8 bytes, double q[nvars]
 *   block_tab[4 b .. 4 b + 3] = {first A, count A, first B, count B} of thread block b (smplx_compact_blocks(B) blocks);
 *             walking the blocks in order gives the records in (state, primitive) order
 *   Each region is cut into 16 sub-regions with their own counters (same-address atomics serialise on this chip): on
 *   the device d_totals has smplx_compact_totals_len() int32 -- [32 k], [32 k + 1] = records of sub-region k in A, B
 *   (sub-region k starts at k * cap / 16), the last one = 1 if a sub-region was too small (the dense outputs are still
 *   complete); the host-pointer form returns totals[0], totals[1] = records in A, B and totals[2] = that flag
 * smplx_table_sync creates the device table if the space has none yet and pushes pending inserts without a batch; so do
 * the two entry points below.  The searches driven by smplx_plan / smplx_plan_multi / smplx_get_succs use the device
 * table only with env SMPLX_DEVICE_TABLE=1 (same results either way): at the batch sizes a search produces the ids it
 * hands back save the host less time than the lookups add to every batch (A/B figures in DESIGN.md section 6). */
int smplx_table_sync(smplx_space* s);
size_t smplx_compact_rec_b_bytes(const smplx_space* s);
int smplx_compact_blocks(const smplx_space* s, int B);
int smplx_compact_totals_len(void);
int smplx_compact_capacity(const smplx_space* s, int B);   /* records per region with which no sub-region can overflow */
/* everything resident in HBM (d_succ_id, and the four compact arguments together, may be NULL); launches on `stream` */
int smplx_expand_batch_k5_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                 int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, int32_t* d_succ_id, int32_t* d_rec_a, int cap_a,
                                 void* d_rec_b, int cap_b, int32_t* d_block_tab, int32_t* d_totals, void* d_work,
                                 uint64_t* d_counters, void* stream);
/* host-pointer form (synchronous): dense flags / coord / succ_q / h / succ_id may be NULL */
int smplx_expand_batch_k5(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                          int32_t* succ_id, int32_t* rec_a, int cap_a, void* rec_b, int cap_b, int32_t* block_tab, int32_t totals[3]);

/* per-kernel timing of the next max_launches expand launches with HIP events recorded on the launch
 * stream (no synchronisation until _end): summed milliseconds of k_state_prep and k_expand.
 * Mirrors the ARAStar/ManipLattice stopwatch hooks (smpl/src/profiling.h:56-117). */
int smplx_profile_begin(smplx_space* s, int max_launches);
int smplx_profile_end(smplx_space* s, double* prep_ms, double* expand_ms, int* launches);

/* ManipLattice::setStart (manip_lattice.cpp:1944-1981): limits + collision check, id assigned */
int smplx_set_start(smplx_space* s, const double* q, int* id);
int smplx_start_id(const smplx_space* s);
int smplx_goal_id(const smplx_space* s);   /* always 0 (manip_lattice.cpp:122) */
/* GetSuccs (manip_lattice.cpp:219-313): valid successors of a state id in primitive order */
int smplx_get_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n);
/* ---- lazy successors (RobotPlanningSpace::GetLazySuccs / GetTrueCost, smpl/include/smpl/graph/robot_planning_space.h:124-130) ----
 * What a lazy planner (the reference's larastar, lmhastar) calls instead of GetSuccs: successors first, without the edge
 * check that dominates an expansion, and the check later, only for the edges the search comes to rely on.
 *
 * smplx_get_lazy_succs: ManipLattice::GetLazySuccs (manip_lattice.cpp:1012-1090).  The goal id has no successors.  For any
 * other state every action of the primitives that are active there (GetSuccs' gating, manip_lattice_action_space.cpp:339-449)
 * gets its state -- getOrCreateState, with NO joint-limit and NO collision test in front -- in primitive order: the goal id
 * where isGoal holds for the action, else the state's id.  Every cost is 1000 (the three-argument cost(), :1388-1412) and
 * every true_cost flag of the reference is false, so there is no array for it.  A lazy caller therefore sees ids an eager
 * caller never would (states out of limits or in collision are created too); ids follow the caller's own call sequence,
 * and smplx_get_succs, smplx_get_lazy_succs and smplx_set_start of one space draw from one counter.  The first call on an id
 * runs one kernel launch (the states of smplx_hint_frontier ride along; env SMPLX_LAZY_RIDERS = most of them, default 64);
 * later calls return the stored list and create nothing.  n gets the count, succs / costs (may be NULL) the first cap entries.
 *
 * smplx_get_true_cost: ManipLattice::GetTrueCost (manip_lattice.cpp:1094-1167).  The parent's actions are applied again;
 * those whose coordinate equals the child's in every variable -- for child == goal id: those for which isGoal holds -- go
 * through checkAction (:1511-1580: joint limits, then the edge parent -> successor, attached bodies included) until one
 * passes.  *cost = 1000 (int(1000 * 1), :1156) if one does, else -1.  Answers are cached per (parent, child); a miss also
 * evaluates, in the same launch, the other unevaluated edges of the parent's lazy list and of the lists of the states
 * expanded last (env SMPLX_TRUE_COST_PARENTS = how many, default 8, 0 = the parent alone).
 * smplx_true_cost_batch: the same for n pairs in one launch.  prims (may be NULL): the lowest-indexed matching primitive
 * that passed, -1 if none; nmatch (may be NULL): the number of matching actions.  n == 0 is SMPLX_OK.
 *
 * Refused like smplx_get_succs (SMPLX_E_STATE): no goal, a grid edited or bodies attached / detached after the goal was
 * set.  The reference reads a state without a coordinate when the parent is the goal id or an id is unknown: here the
 * parent being the goal id is SMPLX_E_ARG, an unknown id SMPLX_E_STATE.  On failure the list is empty and *cost is -1; the
 * first error of smplx_get_lazy_succs / smplx_get_true_cost stays on the space (smplx_space_status).  Setting the goal again
 * drops the lists and the cache with the rest of the lattice. */
int smplx_get_lazy_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n);
int smplx_get_true_cost(smplx_space* s, int parent_id, int child_id, int32_t* cost);
int smplx_true_cost_batch(smplx_space* s, const int32_t* parent_ids, const int32_t* child_ids, int n, int32_t* costs, int32_t* prims,
                          int32_t* nmatch);
/* The loop body of GetLazySuccs (manip_lattice.cpp:1040-1087) for B arbitrary parent states, dense outputs indexed
 * [state][prim]; it creates no state.  flags: 0x10 (inactive) where the primitive has no action at the state, else 4
 * ("generated, unchecked"), plus 2 where isGoal holds.  coord[nvars], q[nvars], h (BFS cost of the planning link's cell)
 * and succ_id (the state's id in the device table, -1 if the coordinate has not been committed) are defined where the
 * primitive is active; elsewhere coord and q are 0 in the host form and untouched in the device form, h is 0, succ_id -1.
 * Any output may be NULL (the device form needs d_flags).  The device form launches on `stream` and does not synchronise. */
int smplx_lazy_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                            int32_t* succ_id);
int smplx_lazy_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                   int32_t* d_h, int32_t* d_succ_id, void* stream);
/* GetTrueCost (manip_lattice.cpp:1094-1167) without ids: item i is the parent's joint values parent_q[i], and the child's
 * coordinate child_coord[i] or, where goal_edge[i] != 0, "the child is the goal" (the coordinate is then ignored; goal_edge
 * NULL = no such item).  costs / prims / nmatch as smplx_true_cost_batch.  The device form also takes
 * smplx_true_cost_work_doubles(s, n) doubles of scratch (d_work_q), needs every pointer but d_prims and d_nmatch, launches on `stream` and does not synchronise. */
int smplx_true_cost_q_batch(smplx_space* s, const double* parent_q, const int32_t* child_coord, const uint8_t* goal_edge, int n,
                            int32_t* costs, int32_t* prims, int32_t* nmatch);
size_t smplx_true_cost_work_doubles(const smplx_space* s, int n);
int smplx_true_cost_q_batch_device(smplx_space* s, const double* d_parent_q, const int32_t* d_child_coord, const uint8_t* d_goal_edge,
                                   int n, double* d_work_q, int32_t* d_costs, int32_t* d_prims, int32_t* d_nmatch, void* stream);
/* running totals since the goal was last set: out[0] kernel launches of smplx_get_lazy_succs, [1] its calls served without
 * one, [2] launches of smplx_get_true_cost / smplx_true_cost_batch, [3] edges they evaluated, [4] pairs answered from the
 * cache, [5] pairs that were not */
int smplx_lazy_counters(const smplx_space* s, int64_t out[6]);
/* optional: ids the caller expects to expand soon (top of OPEN); they ride along in the next batch.  A caller that
 * never hints (an unchanged SBPL planner) still gets frontier batches: the space mirrors the g-values the caller's
 * GetSuccs sequence implies (arastar.cpp:546-551) and lets the unevaluated states with the smallest g + w*h ride
 * along on every miss (env SMPLX_AUTO_SPECULATE = states per miss, default 96, 0 = off; w = 5).  Speculation never
 * changes results: ids are assigned when the caller's own sequence commits a state. */
int smplx_hint_frontier(smplx_space* s, const int32_t* ids, int n);
/* GetSuccs has no way to report a failure to an SBPL caller (the successor list just stays empty, which reads as a
 * dead end): the first such error is kept on the space.  Returns SMPLX_OK or that error code; msg gets its text. */
int smplx_space_status(const smplx_space* s, char* msg, int cap);
void smplx_space_clear_status(smplx_space* s);
/* RobotHeuristic::GetGoalHeuristic(state_id) */
int smplx_get_goal_heuristic(smplx_space* s, int id, int32_t* h);
int smplx_num_states(const smplx_space* s);
/* running totals of the space since its goal was last set: out[0] GPU frontier batches, [1] GetSuccs calls served from
 * the cache, [2] GetSuccs calls that had to wait for a batch, [3] committed successor evaluations, [4] successor
 * evaluations the GPU performed (incl. speculative), [5] states ("expands"/"stats" of planner_interface.cpp:1438-1446) */
int smplx_space_counters(const smplx_space* s, int64_t out[6]);
int smplx_get_state(const smplx_space* s, int id, double* q, int32_t* coord);

/* ---- the caller: ARA* (smpl/src/search/arastar.cpp:107-215,486-582) ---- */
typedef struct smplx_search_params {
    double initial_eps, final_eps, delta_eps;
    int32_t improve;              /* ARAStar::setImproveSolution */
    int32_t bounded;              /* expansion bound (TimeParameters::EXPANSIONS) */
    int32_t max_expansions_init, max_expansions;
} smplx_search_params;

typedef struct smplx_search_stats {
    int32_t solved;               /* 1 = success, as ARAStar::replan's return */
    int32_t path_len, cost, expansions, expansions_init;
    double satisfied_eps;
    double seconds;               /* wall time inside replan */
    int64_t gpu_succ_evals;       /* successor evaluations the GPU performed (incl. speculative) */
    int64_t committed_succ_evals; /* evaluations of the committed expansions, counted as the reference performs them:
                                     once per GetSuccs call, so a state re-expanded in a later ARA* iteration counts
                                     again although the engine serves the repeat from its committed list */
    int64_t gpu_batches;
    int64_t cache_hits, cache_misses;
    int64_t grid_lookups;
} smplx_search_stats;

/* ARAStar::replan from scratch (arastar.cpp:107-215) on the query of `s`.
 * Where the search runs.  Two or more queries (smplx_plan_multi), or env SMPLX_SEARCH=device: ON THE DEVICE (SURVEY row
 * N2): one persistent workgroup owns a query -- OPEN (the
 * reference's binary heap with its sift rules, intrusive_heap.hpp:346-395), INCONS, the state table and the search
 * states live in HBM, the workgroup pops a state, evaluates its successors on its lanes, creates states with ids in its
 * own commit order (= the reference's ids) and pushes them; the host only launches, enlarges buffers when asked, and
 * reads results (stats: gpu_batches = kernel launches, cache_misses = 0).  The lattice stays in HBM until an entry point
 * needs it on the host (smplx_get_state, smplx_expansion_log, smplx_get_succs ...), which then see every state the
 * device created.  A single query (it is a chain of dependent expansions: the host loop's speculative batches are the
 * faster way to run one), robots whose expansion does not fit one workgroup's LDS, spaces created with SMPLX_SPACE_FUSED /
 * SMPLX_SPACE_NO_SMALL_KERNEL, and env SMPLX_SEARCH=host take the host-driven loop instead: the same sequential ARA*
 * on the host with frontier batches on the GPU (what an external SBPL planner gets through smplx_get_succs).  Results
 * are identical either way. */
int smplx_plan(smplx_space* s, const smplx_search_params* p, int32_t* path_ids, int cap, smplx_search_stats* stats);
/* diagnostics of the device-resident search of this space: out[0] searches run on the device, [1] buffer enlargements,
 * [2] pushes of a state already in OPEN in the last search (the reference's INCONS holds a state once per improvement),
 * [3..9] 10-ns ticks the search wave of the workgroup spent, last search: (idle), select + pop, until the waypoint lanes'
 * round has closed (ancestor prefetch, preparing the next round, waiting), getOrCreateState, relaxation + pushes, epsilon
 * steps (reorder), load / store of the launch state; [10] states on the device, [11] heap entries cached in LDS;
 * [12] evaluation rounds opened on a guess of the next pop, [13] guesses the pop confirmed; [14] empty state
 * tables the search allocated and filled from its states' coordinates (the first one, and one each time the states outgrew
 * it), [15] times the host loop's device table was outgrown and built again */
int smplx_search_counters(const smplx_space* s, int64_t out[16]);
/* nq independent queries (each its own smplx_space: goal, BFS grid, state table) on one GPU.  Device-resident search
 * (default): one workgroup per query, all in ONE launch when the queries share grid, robot and primitives.  Host-driven
 * loop (SMPLX_SEARCH=host): a query runs until it misses, its frontier batch is issued, and the thread moves on to
 * the next query.  No data is exchanged between queries; every query's result equals what smplx_plan gives alone.
 * path_ids holds nq rows of cap ids (may be NULL); stats holds nq entries (seconds = completion time since the
 * start of the call); wall_seconds = duration of the whole call.  Queries created on the same smplx_grid and
 * smplx_model with the same primitives share launches (one cross-query frontier batch per sweep); host_threads > 1
 * splits them into that many slices, each driven by its own host thread.  (BASELINE config 4: 128 queries per GPU.) */
int smplx_plan_multi(smplx_space** spaces, int nq, const smplx_search_params* p, int32_t* path_ids, int cap,
                     smplx_search_stats* stats, double* wall_seconds, int host_threads);

/* ---- anytime ARA*: time budgets, resumable replans, partial solutions (ARAStar::replan(const TimeParameters&, ...),
 * arastar.cpp:107-215 and 486-527; TimeParameters / timedOut: arastar.h:80-90, arastar.cpp:454-484) ----
 * A call CONTINUES the previous search of the space (resumed = 1) when from_scratch == 0, the space has a search from an
 * earlier smplx_plan / smplx_replan call that ran on the same side (device or host loop), the start id is the same, no
 * smplx_set_goal_* (it renumbers the lattice) and no failed call on the space came since; otherwise it plans from scratch
 * (the reference's "start changed -> reinitialise", arastar.cpp:128-162).  A resumed call keeps OPEN, INCONS, the search
 * states, the iteration, curr_eps and satisfied_eps; its expansion count and budget clock start at 0; final_eps,
 * delta_eps, improve and the budgets are this call's (the setters of arastar.h:96-123 between calls), initial_eps is
 * used only from scratch.  The budget is checked where timedOut sits (after the goal test, before the pop): max_*_init
 * while there is no solution, max_* once there is one; wall mode counts seconds since the call entered smplx_replan*,
 * and a budget of 0 expands nothing.  With no solution, allow_partial and OPEN not empty, the call returns the bp chain
 * from OPEN's minimum, its g as the cost, result SMPLX_ARA_PARTIAL and solved = 1 (arastar.cpp:204-209).  A call that
 * times out while improving returns the goal's current chain (arastar.cpp:213).  smplx_expansion_log holds the pops of
 * the whole search since it last started from scratch, across resumed calls. */
enum { SMPLX_TIME_EXPANSIONS = 0, SMPLX_TIME_WALL = 1 };                /* ARAStar::TimeParameters::TimingType */
enum { SMPLX_ARA_SUCCESS = 0, SMPLX_ARA_PARTIAL = 1,                     /* ReplanResultCode, arastar.cpp:97-105 */
       SMPLX_ARA_TIMED_OUT = 4, SMPLX_ARA_EXHAUSTED = 5 };
typedef struct smplx_time_params {
    double initial_eps, final_eps, delta_eps;
    int32_t improve, bounded, type;               /* type: SMPLX_TIME_* */
    int32_t max_expansions_init, max_expansions;
    double max_seconds_init, max_seconds;         /* max_allowed_time_init / max_allowed_time */
    int32_t allow_partial;                        /* ARAStar::allowPartialSolutions */
    int32_t from_scratch;                         /* force_planning_from_scratch before this call */
} smplx_time_params;
typedef struct smplx_replan_stats {
    smplx_search_stats s;         /* expansions / expansions_init / satisfied_eps: since the search began (get_n_expands ...);
                                     seconds, evaluations, lookups, batches: this call's */
    int32_t result;               /* SMPLX_ARA_* of this call */
    int32_t call_expansions;      /* expansions of this call */
    int32_t resumed;              /* 1 = continued the previous search of this space */
    int32_t pad;
} smplx_replan_stats;
/* smplx_plan / smplx_plan_multi are these with from_scratch = 1, SMPLX_TIME_EXPANSIONS and allow_partial = 0. */
int smplx_replan(smplx_space* s, const smplx_time_params* p, int32_t* path_ids, int cap, smplx_replan_stats* st);
int smplx_replan_multi(smplx_space** spaces, int nq, const smplx_time_params* p, int32_t* path_ids, int cap,
                       smplx_replan_stats* st, double* wall_seconds, int host_threads);

/* Query sharding over ranks, one process per GPU (independent queries partition over GPUs with no data-path
 * collective; the demo's outer loop over requests, smpl_test/src/call_planner.cpp): rank r of `world` owns queries
 * [*first, *first + *count) of a list of `total`, `per_rank` each (BASELINE config 4: 128), the last ranks possibly fewer or
 * none.  A C or C++ caller plans its range with smplx_plan_multi on its own GPU and gathers the per-query results with
 * whatever its job uses (MPI, RCCL: a few integers per query). */
int smplx_shard_range(int rank, int world, int total, int per_rank, int* first, int* count);

int smplx_expansion_log_size(const smplx_space* s);
int smplx_expansion_log(const smplx_space* s, int32_t* out);
/* ManipLattice::extractPath for a plain id path (manip_lattice.cpp:2018-2155): q[len][nvars] */
int smplx_extract_path(smplx_space* s, const int32_t* ids, int len, double* q);

/* --- path post-processing: PlannerInterface::postProcessPath (smpl_ros/src/ros/planner_interface.cpp:2651-2697) over
 * ShortcutPath(JOINT_SPACE) (smpl/src/post_processing.cpp:281-309, smpl/include/smpl/geometry/detail/shortcut.hpp:110-286)
 * and InterpolatePath (post_processing.cpp:464-523).  path: n points of nvars doubles.  The collision questions of the
 * greedy loops are answered from waypoint-parallel GPU batches.  stats (may be NULL): [0] edge batches, [1] configurations
 * checked.  out may be NULL to query the size. */
enum {
    SMPLX_PP_SHORTCUT = 1,          /* shortcut_path */
    SMPLX_PP_INTERPOLATE = 2,       /* interpolate_path */
    SMPLX_PP_UPSTREAM_LIMITS = 4    /* use upstream's limit test in CollisionSpace::interpolatePath; the default is the
                                       fork's (collision_space.cpp:592-597), under which interpolation of an in-limits
                                       path reports failure and leaves the path as it was */
};
int smplx_post_process_path(smplx_space* s, const double* path, int n, int flags, double* out, int cap, int* nout,
                            int64_t* stats);

/* The same for nq paths in one call, in a bounded number of launches: for every k the points of output path k are
 * byte-identical to what smplx_post_process_path(spaces[k], path k, flags) returns, in every flag combination.
 * paths: first[nq] points of nvars doubles, back to back; first: nq + 1 offsets in points, first[0] == 0, non-decreasing.
 * out: room for cap points, may be NULL to ask the sizes; out_first: nq + 1 offsets into out, filled on SMPLX_OK and on
 * SMPLX_E_LIMIT (out given and out_first[nq] > cap: out is untouched).
 * A space may appear several times.  The spaces may differ in their attached bodies -- each path is checked with its own
 * space's -- but share one grid handle, one model image (robot, padding) and one kernel build (SMPLX_SPACE_GENERIC_KERNELS
 * alike); primitives and heuristic kind do not matter.  Anything else, a null pointer, nq < 0, bad offsets or a value
 * that is not finite with |q| < 1e6 is SMPLX_E_ARG, and nothing is written.  nq == 0 is SMPLX_OK.
 * The call needs no goal, is not refused after a grid edit or an attach, and leaves the lattices, the caches and a search
 * that smplx_replan may resume untouched; it uses the stream of spaces[0] and scratch of its own there.
 * The shortcut loop of every path runs to its end in one kernel, one workgroup a path (csrc/path_kernels.h k_shortcut); each
 * interpolation pass checks all waypoints of all paths in one launch.  A workgroup that exceeds the loop's trip bound
 * (2P + 2 for a path of P points) stops and the call returns SMPLX_E_HIP.
 * stats (may be NULL): [0] kernel launches, [1] host waits (stream synchronisations), [2] configurations checked on the
 * device, [3] paths.  [0] and [1] never exceed SMPLX_PP_MULTI_MAX_LAUNCHES, whatever nq and the path lengths are. */
#define SMPLX_PP_MULTI_MAX_LAUNCHES 3
int smplx_post_process_paths(smplx_space* const* spaces, int nq, const double* paths, const int32_t* first, int flags, double* out,
                             int cap, int32_t* out_first, int64_t* stats);

#ifdef __cplusplus
}
#endif

#endif /* SMPL_AMD_H */
