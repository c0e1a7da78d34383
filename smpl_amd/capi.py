"""ctypes binding of smpl_amd/libsmpl_amd.so -- the C-ABI declared in include/smpl_amd.h.

Thin by design: numpy arrays in, numpy arrays out, one Python method per C entry point.  The
library is the product; this file only marshals pointers.  There is no CPU fallback: if the
shared object is missing or no GPU is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)

# every symbol include/smpl_amd.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "smplx_last_error", "smplx_device_count", "smplx_shard_range", "smplx_grid_create", "smplx_grid_destroy", "smplx_model_create",
    "smplx_model_destroy", "smplx_model_counts", "smplx_model_joints", "smplx_model_nodes", "smplx_model_pairs",
    "smplx_space_create", "smplx_space_destroy", "smplx_space_num_vars", "smplx_space_num_prims",
    "smplx_space_discretization", "smplx_cc_state_valid_batch", "smplx_cc_edge_valid_batch", "smplx_cc_interpolate",
    "smplx_cc_sphere_positions", "smplx_set_goal_joint", "smplx_set_goal_xyz", "smplx_goal_pose",
    "smplx_heuristic_batch", "smplx_bfs_size", "smplx_bfs_copy", "smplx_bfs_levels", "smplx_expand_batch",
    "smplx_expand_work_bytes", "smplx_expand_batch_device", "smplx_set_start", "smplx_start_id", "smplx_goal_id",
    "smplx_get_succs", "smplx_hint_frontier", "smplx_get_goal_heuristic", "smplx_num_states", "smplx_get_state",
    "smplx_plan", "smplx_expansion_log_size", "smplx_expansion_log", "smplx_extract_path", "smplx_post_process_path", "smplx_space_specialized", "smplx_model_const_header", "smplx_profile_begin",
    "smplx_profile_end", "smplx_counters_bytes", "smplx_counters_read", "smplx_plan_multi",
    "smplx_bfs_metric_goal_distance", "smplx_bfs_metric_start_distance", "smplx_space_status", "smplx_space_clear_status",
    "smplx_check_joint_limits", "smplx_cc_state_valid_batch_device", "smplx_space_counters",
    "smplx_table_sync", "smplx_compact_rec_b_bytes", "smplx_compact_blocks", "smplx_expand_batch_k5_device", "smplx_expand_batch_k5",
    "smplx_compact_totals_len", "smplx_compact_capacity",
    "smplx_grid_create_empty", "smplx_grid_add_boxes", "smplx_grid_add_points", "smplx_grid_remove_points", "smplx_grid_copy_d2",
    "smplx_search_counters", "smplx_grid_set_ref_counted", "smplx_grid_update_points", "smplx_grid_copy_counts", "smplx_grid_last_edit_cells",
    "smplx_replan", "smplx_replan_multi", "smplx_set_goals_joint_multi", "smplx_set_goals_xyz_multi",
    "smplx_attach_body", "smplx_detach_body", "smplx_attached_bodies", "smplx_attached_nodes", "smplx_cc_attached_positions",
    "smplx_set_goal_pose", "smplx_set_goals_pose_multi", "smplx_goal_orientation", "smplx_planning_pose_batch", "smplx_rpy_angle",
    "smplx_cc_state_clearance_batch", "smplx_cc_state_clearance_batch_device", "smplx_cc_edge_clearance_batch",
    "smplx_get_lazy_succs", "smplx_get_true_cost", "smplx_true_cost_batch", "smplx_lazy_expand_batch", "smplx_lazy_expand_batch_device",
    "smplx_true_cost_q_batch", "smplx_true_cost_work_doubles", "smplx_true_cost_q_batch_device", "smplx_lazy_counters",
    "smplx_world_insert_object", "smplx_world_remove_object", "smplx_world_move_object", "smplx_world_remove_all",
    "smplx_world_objects", "smplx_world_object_cells", "smplx_world_voxelize",
    "smplx_body_create", "smplx_body_destroy", "smplx_body_counts", "smplx_body_set_joint", "smplx_body_joint",
    "smplx_body_link_transforms", "smplx_body_model_link", "smplx_body_model_points", "smplx_body_dirty",
    "smplx_grid_put_body", "smplx_grid_take_body", "smplx_grid_body_cells",
    "smplx_set_euclid_weights", "smplx_metric_goal_distance", "smplx_pose_distance", "smplx_joint_distance",
    "smplx_space_heuristic",
    "smplx_attach_object", "smplx_object_spheres",
    "smplx_post_process_paths",
]

# SMPLX_ATTACHED_SPHERE_RADIUS (include/smpl_amd.h): the reference's radius of an attached object's spheres
ATTACHED_SPHERE_RADIUS = 0.025

# smplx_params.heuristic (include/smpl_amd.h)
H_BFS, H_EUCLID, H_JOINT_DIST = 0, 1, 2
E_STATE = -5

# smplx_time_params.type and smplx_replan_stats.result (include/smpl_amd.h)
TIME_EXPANSIONS, TIME_WALL = 0, 1
ARA_SUCCESS, ARA_PARTIAL, ARA_TIMED_OUT, ARA_EXHAUSTED = 0, 1, 4, 5


class Params(C.Structure):
    _fields_ = [("resolutions", C.c_double * 16), ("bfs_inflation_radius", C.c_double), ("cost_per_cell", C.c_int32),
                ("use_short_dist_mprims", C.c_int32), ("short_dist_mprims_thresh", C.c_double),
                ("use_xyzrpy_snap_mprim", C.c_int32), ("xyzrpy_snap_dist_thresh", C.c_double),
                ("xy_rotate_by_var3", C.c_int32), ("use_long_and_short", C.c_int32), ("padding", C.c_double),
                ("batch_states", C.c_int32), ("flags", C.c_int32), ("heuristic", C.c_int32)]


class SearchParams(C.Structure):
    _fields_ = [("initial_eps", C.c_double), ("final_eps", C.c_double), ("delta_eps", C.c_double),
                ("improve", C.c_int32), ("bounded", C.c_int32), ("max_expansions_init", C.c_int32),
                ("max_expansions", C.c_int32)]


class SearchStats(C.Structure):
    _fields_ = [("solved", C.c_int32), ("path_len", C.c_int32), ("cost", C.c_int32), ("expansions", C.c_int32),
                ("expansions_init", C.c_int32), ("satisfied_eps", C.c_double), ("seconds", C.c_double),
                ("gpu_succ_evals", C.c_int64), ("committed_succ_evals", C.c_int64), ("gpu_batches", C.c_int64),
                ("cache_hits", C.c_int64), ("cache_misses", C.c_int64), ("grid_lookups", C.c_int64)]


class TimeParams(C.Structure):
    _fields_ = [("initial_eps", C.c_double), ("final_eps", C.c_double), ("delta_eps", C.c_double),
                ("improve", C.c_int32), ("bounded", C.c_int32), ("type", C.c_int32),
                ("max_expansions_init", C.c_int32), ("max_expansions", C.c_int32),
                ("max_seconds_init", C.c_double), ("max_seconds", C.c_double),
                ("allow_partial", C.c_int32), ("from_scratch", C.c_int32)]


class ReplanStats(C.Structure):
    _fields_ = [("s", SearchStats), ("result", C.c_int32), ("call_expansions", C.c_int32), ("resumed", C.c_int32),
                ("pad", C.c_int32)]


def time_params(eps0, eps_final, eps_delta, improve=True, bounded=False, max_init=0, max_rep=0, wall=False,
                seconds_init=0.0, seconds=0.0, allow_partial=False, from_scratch=False):
    """smplx_time_params: expansion bounds (wall=False) or wall-clock budgets in seconds (wall=True)."""
    return TimeParams(eps0, eps_final, eps_delta, int(improve), int(bounded), TIME_WALL if wall else TIME_EXPANSIONS,
                      int(max_init), int(max_rep), float(seconds_init), float(seconds), int(allow_partial), int(from_scratch))


_lib = None


def lib():
    """Load (building in-tree if needed) the shared library."""
    global _lib
    if _lib is None:
        path = os.environ.get("SMPL_AMD_LIB", _build.LIB)   # override: kernel experiments (tools/)
        if not os.path.exists(path):
            _build.build()
        L = C.CDLL(path)
        L.smplx_last_error.restype = C.c_char_p
        L.smplx_bfs_size.restype = C.c_int64
        L.smplx_expand_work_bytes.restype = C.c_size_t
        L.smplx_grid_create.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _ip, C.POINTER(C.c_void_p)]
        L.smplx_model_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.smplx_space_create.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(Params), C.POINTER(C.c_void_p)]
        for name in ["smplx_grid_destroy", "smplx_model_destroy", "smplx_space_destroy"]:
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.smplx_expand_batch_device.argtypes = [C.c_void_p] + [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        L.smplx_expand_work_bytes.argtypes = [C.c_void_p, C.c_int]
        L.smplx_counters_bytes.restype = C.c_size_t
        L.smplx_counters_bytes.argtypes = [C.c_void_p, C.c_int]
        L.smplx_counters_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _u64p]
        L.smplx_bfs_metric_goal_distance.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.smplx_bfs_metric_start_distance.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.smplx_space_clear_status.argtypes = [C.c_void_p]
        L.smplx_space_clear_status.restype = None
        L.smplx_set_goal_pose.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_double]
        L.smplx_set_goals_pose_multi.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
        L.smplx_goal_orientation.argtypes = [C.c_void_p, _dp, _dp]
        L.smplx_planning_pose_batch.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.smplx_rpy_angle.argtypes = [_dp, _dp, _dp]
        L.smplx_set_euclid_weights.argtypes = [C.c_void_p, _dp]
        L.smplx_metric_goal_distance.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        L.smplx_pose_distance.argtypes = [_dp, _dp, _dp, _dp]
        L.smplx_joint_distance.argtypes = [_dp, _dp, C.c_int, _dp]
        L.smplx_test_acos.argtypes = [_dp, C.c_int, _dp]
        L.smplx_test_goal_rotation.argtypes = [C.c_void_p, _dp]
        L.smplx_space_heuristic.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class SmplxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"smplx error {code}: {msg}")
        self.code = code


def _chk(code):
    if code != 0:
        raise SmplxError(code, lib().smplx_last_error().decode())


def _p(a, t):
    return a.ctypes.data_as(t)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def rpy_angle(a, b):
    """The pose goal's orientation distance between two roll/pitch/yaw triples, in [0, pi] (smplx_rpy_angle): what
    set_goal_pose compares with rpy_tol.  Host arithmetic, needs no GPU."""
    x = _f64(a); y = _f64(b); t = C.c_double(0.0)
    _chk(lib().smplx_rpy_angle(_p(x, _dp), _p(y, _dp), C.byref(t)))
    return t.value


def pose_distance(Ta, Tb, w=(1.0, 1.0, 1.0, 1.0)):
    """EuclidDistHeuristic's distance between two 3x4 (or 4x4) transforms with weights {x, y, z, rot} (smplx_pose_distance):
    int(1000 * it) is the h of a SMPLX_H_EUCLID space.  Host arithmetic, needs no GPU."""
    a = _f64(np.asarray(Ta, float).reshape(-1)[:12]); b = _f64(np.asarray(Tb, float).reshape(-1)[:12]); ww = _f64(w)
    d = C.c_double(0.0)
    _chk(lib().smplx_pose_distance(_p(a, _dp), _p(b, _dp), _p(ww, _dp), C.byref(d)))
    return d.value


def joint_distance(a, b):
    """JointDistHeuristic's distance between two joint vectors (smplx_joint_distance).  Host arithmetic, needs no GPU."""
    x = _f64(a).reshape(-1); y = _f64(b).reshape(-1)
    assert x.shape == y.shape
    d = C.c_double(0.0)
    _chk(lib().smplx_joint_distance(_p(x, _dp), _p(y, _dp), x.shape[0], C.byref(d)))
    return d.value


def host_acos(x):
    """Test hook (csrc/test_hooks.h smplx_test_acos): the host build of smplx_acos at every element of x."""
    a = _f64(x).reshape(-1); out = np.zeros(a.shape[0])
    _chk(lib().smplx_test_acos(_p(a, _dp), a.shape[0], _p(out, _dp)))
    return out


def table_probe(nvars, slots, one_home, inserted, queries):
    """Test hook (csrc/test_hooks.h smplx_test_table_probe): the device search's state-table probe on an empty table of
    `slots` slots.  Returns (what the probe found for each inserted coordinate before it was stored, id of each query)."""
    a = np.ascontiguousarray(inserted, dtype=np.int32).reshape(-1, nvars)
    q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1, nvars)
    found = np.zeros(a.shape[0], np.int32); ids = np.zeros(q.shape[0], np.int32)
    lib().smplx_test_table_probe.argtypes = [C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, C.c_int, _ip, _ip]
    _chk(lib().smplx_test_table_probe(nvars, slots, int(bool(one_home)), _p(a, _ip), a.shape[0], _p(q, _ip), q.shape[0],
                                      _p(found, _ip), _p(ids, _ip)))
    return found, ids


# SMPLX_PP_MULTI_MAX_LAUNCHES (include/smpl_amd.h): the most launches, and the most host waits, of one post_process_paths call
PP_MULTI_MAX_LAUNCHES = 3


def _post_process_paths_fn():
    f = lib().smplx_post_process_paths
    f.argtypes = [C.POINTER(C.c_void_p), C.c_int, _dp, _ip, C.c_int, _dp, C.c_int, _ip, C.POINTER(C.c_int64)]
    return f


def post_process_paths(spaces, paths, shortcut=True, interpolate=True, upstream_limits=False):
    """smplx_post_process_paths: PlannerInterface::postProcessPath of paths[k] in spaces[k], all in one call.
    Returns (list of arrays, stats)."""
    nq = len(spaces)
    assert len(paths) == nq
    N = spaces[0].N if nq else 1
    P = [np.ascontiguousarray(p, np.float64).reshape(-1, N) for p in paths]
    first = np.zeros(nq + 1, np.int32)
    for k, p in enumerate(P):
        first[k + 1] = first[k] + p.shape[0]
    flat = np.ascontiguousarray(np.vstack(P + [np.zeros((1, N))]))     # (never empty: a pointer to pass)
    flags = (1 if shortcut else 0) | (2 if interpolate else 0) | (4 if upstream_limits else 0)
    H = (C.c_void_p * max(nq, 1))(*[sp.h for sp in spaces])
    of = np.zeros(nq + 1, np.int32); st = (C.c_int64 * 4)()
    f = _post_process_paths_fn()
    _chk(f(H, nq, _p(flat, _dp), _p(first, _ip), flags, None, 0, _p(of, _ip), st))
    out = np.zeros((max(int(of[nq]), 1), N))
    _chk(f(H, nq, _p(flat, _dp), _p(first, _ip), flags, _p(out, _dp), out.shape[0], _p(of, _ip), st))
    return ([out[of[k]:of[k + 1]].copy() for k in range(nq)],
            dict(launches=st[0], waits=st[1], configs=st[2], paths=st[3]))


def path_waypoints(space, a, b):
    """Test hook (csrc/test_hooks.h smplx_test_path_waypoints): for the edges a[i] -> b[i], the joint values the lanes of
    k_shortcut check, in rows sized by smplx_cc_interpolate's counts.  Returns (list of arrays, the device's counts)."""
    a = _f64(a).reshape(-1, space.N); b = _f64(b).reshape(-1, space.N)
    n = a.shape[0]
    first = np.zeros(n + 1, np.int32)
    for i in range(n):
        first[i + 1] = first[i] + space.interpolate(a[i], b[i], cap=1)[1]
    out = np.zeros((max(int(first[n]), 1), space.N)); counts = np.zeros(n, np.int32)
    lib().smplx_test_path_waypoints.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _ip, _dp, _ip]
    _chk(lib().smplx_test_path_waypoints(space.h, _p(a, _dp), _p(b, _dp), n, _p(first, _ip), _p(out, _dp), _p(counts, _ip)))
    return [out[first[i]:first[i + 1]].copy() for i in range(n)], counts


# smplx_shape.type (include/smpl_amd.h)
SHAPE_BOX, SHAPE_SPHERE, SHAPE_CYLINDER, SHAPE_CONE, SHAPE_MESH, SHAPE_OCTREE = 1, 2, 3, 4, 5, 6
E_ARG = -1


class ShapeStruct(C.Structure):
    _fields_ = [("type", C.c_int32), ("dims", C.c_double * 3), ("pose", C.c_double * 12), ("vertices", _dp),
                ("nvertices", C.c_int32), ("triangles", _ip), ("ntriangles", C.c_int32)]


def pose_at(xyz=(0.0, 0.0, 0.0), R=None):
    """3x4 [R | t] of a shape, row major; identity rotation unless R (3x3) is given."""
    P = np.zeros((3, 4))
    P[:, :3] = np.eye(3) if R is None else np.asarray(R, float).reshape(3, 3)
    P[:, 3] = xyz
    return P


def _shape(ty, dims, pose, **more):
    d = list(dims) + [0.0] * (3 - len(dims))
    return dict(type=ty, dims=tuple(float(x) for x in d), pose=pose_at() if pose is None else _f64(pose).reshape(3, 4), **more)


def box(size, pose=None):
    """shapes::Box: size = (x, y, z) edge lengths, centred on the pose."""
    return _shape(SHAPE_BOX, size, pose)


def sphere(radius, pose=None):
    return _shape(SHAPE_SPHERE, [radius], pose)


def cylinder(radius, height, pose=None):
    """z-aligned, centred on the pose."""
    return _shape(SHAPE_CYLINDER, [radius, height], pose)


def cone(radius, height, pose=None):
    """z-aligned, apex up, centred on the pose."""
    return _shape(SHAPE_CONE, [radius, height], pose)


def mesh(vertices, triangles, pose=None):
    """vertices: n x 3, triangles: index triples.  A triangle list whose length is no multiple of 3 is refused
    (VoxelizeMesh, smpl/src/geometry/voxelize.cpp:1016-1019)."""
    t = np.ascontiguousarray(triangles, dtype=np.int32).ravel()
    v = _f64(vertices).ravel()
    if t.size % 3 != 0 or v.size % 3 != 0:
        raise SmplxError(E_ARG, "mesh triangles and vertices come in triples")
    return _shape(SHAPE_MESH, [], pose, vertices=v.reshape(-1, 3), triangles=t.reshape(-1, 3))


def octree(leaves, pose=None):
    """shapes::OcTree: leaves is n x 4, one row {cx, cy, cz, size} per occupied leaf (centre and edge length in the
    octree's frame, in the order the octomap's begin_leafs() yields them); pose is the octomap's origin.  Anything that
    is not n x 4 with n >= 1 is refused here; scenes.octree_leaves makes such rows from a point cloud."""
    v = _f64(leaves)
    if v.ndim != 2 or v.shape[1] != 4 or v.shape[0] < 1:
        raise SmplxError(E_ARG, "octree leaves come as n x 4 rows of cx, cy, cz, size")
    return _shape(SHAPE_OCTREE, [], pose, leaves=v)


def _shape_array(shapes):
    """-> (smplx_shape array, the numpy arrays it points into: keep them alive over the call)"""
    shapes = list(shapes)
    arr, keep = (ShapeStruct * max(1, len(shapes)))(), []
    for a, s in zip(arr, shapes):
        a.type = int(s["type"])
        a.dims[:] = [float(x) for x in s["dims"]]
        a.pose[:] = [float(x) for x in _f64(s["pose"]).ravel()]
        if "vertices" in s:
            v = _f64(s["vertices"]).reshape(-1, 3); t = np.ascontiguousarray(s["triangles"], dtype=np.int32).reshape(-1, 3)
            keep += [v, t]
            a.vertices, a.nvertices, a.triangles, a.ntriangles = _p(v, _dp), v.shape[0], _p(t, _ip), t.shape[0]
        elif "leaves" in s:      # an octree's rows travel through `vertices`, four doubles each
            v = _f64(s["leaves"]).reshape(-1, 4)
            keep.append(v)
            a.vertices, a.nvertices = _p(v, _dp), v.shape[0]
    return arr, len(shapes), keep


class Grid:
    """OccupancyGrid, lookup side, resident in HBM (16-bit squared distances in 4x4x4 bricks)."""

    def __init__(self, origin, dims, res, max_dist, d2):
        self.h = C.c_void_p()
        o = _f64(origin)
        d2 = np.ascontiguousarray(d2, dtype=np.int32)
        assert d2.shape == tuple(dims)
        _chk(lib().smplx_grid_create(_p(o, _dp), dims[0], dims[1], dims[2], res, max_dist, _p(d2, _ip), C.byref(self.h)))
        self.dims = tuple(dims)

    @classmethod
    def empty(cls, origin, dims, res, max_dist):
        """A grid built and kept on the GPU (row N1): starts empty (only the border cells count as obstacles)."""
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        o = _f64(origin)
        lib().smplx_grid_create_empty.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_void_p)]
        _chk(lib().smplx_grid_create_empty(_p(o, _dp), dims[0], dims[1], dims[2], res, max_dist, C.byref(self.h)))
        self.dims = tuple(dims)
        return self

    @classmethod
    def from_boxes(cls, origin, dims, res, max_dist, boxes):
        self = cls.empty(origin, dims, res, max_dist)
        self.add_boxes(boxes)
        return self

    def add_boxes(self, boxes):
        b = _f64([list(c) + list(s) for (c, s) in boxes]).reshape(-1, 6)
        lib().smplx_grid_add_boxes.argtypes = [C.c_void_p, _dp, C.c_int]
        _chk(lib().smplx_grid_add_boxes(self.h, _p(b, _dp), b.shape[0]))

    def add_points(self, xyz):
        p = _f64(xyz).reshape(-1, 3)
        lib().smplx_grid_add_points.argtypes = [C.c_void_p, _dp, C.c_int]
        _chk(lib().smplx_grid_add_points(self.h, _p(p, _dp), p.shape[0]))

    def remove_points(self, xyz):
        p = _f64(xyz).reshape(-1, 3)
        lib().smplx_grid_remove_points.argtypes = [C.c_void_p, _dp, C.c_int]
        _chk(lib().smplx_grid_remove_points(self.h, _p(p, _dp), p.shape[0]))

    def set_ref_counted(self, on=True):
        lib().smplx_grid_set_ref_counted.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_grid_set_ref_counted(self.h, int(on)))

    def update_points(self, old_xyz, new_xyz):
        a = _f64(old_xyz).reshape(-1, 3); b = _f64(new_xyz).reshape(-1, 3)
        lib().smplx_grid_update_points.argtypes = [C.c_void_p, _dp, C.c_int, _dp, C.c_int]
        _chk(lib().smplx_grid_update_points(self.h, _p(a, _dp), a.shape[0], _p(b, _dp), b.shape[0]))

    def counts(self):
        out = np.zeros(self.dims, np.int32)
        lib().smplx_grid_copy_counts.argtypes = [C.c_void_p, _ip]
        _chk(lib().smplx_grid_copy_counts(self.h, _p(out, _ip)))
        return out

    def last_edit_cells(self):
        lib().smplx_grid_last_edit_cells.restype = C.c_longlong
        lib().smplx_grid_last_edit_cells.argtypes = [C.c_void_p]
        return int(lib().smplx_grid_last_edit_cells(self.h))

    def d2(self):
        out = np.zeros(self.dims, np.int32)
        lib().smplx_grid_copy_d2.argtypes = [C.c_void_p, _ip]
        _chk(lib().smplx_grid_copy_d2(self.h, _p(out, _ip)))
        return out

    # ---- world objects (include/smpl_amd.h "world objects"): shapes are what box() / sphere() / cylinder() / cone() /
    # mesh() / octree() above return
    def insert_object(self, object_id, shapes):
        arr, n, keep = _shape_array(shapes)
        lib().smplx_world_insert_object.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(ShapeStruct), C.c_int]
        _chk(lib().smplx_world_insert_object(self.h, object_id.encode(), arr, n))

    def move_object(self, object_id, shapes):
        """moveShapes / insertShapes / removeShapes: the object's shapes become `shapes`, as one field edit."""
        arr, n, keep = _shape_array(shapes)
        lib().smplx_world_move_object.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(ShapeStruct), C.c_int]
        _chk(lib().smplx_world_move_object(self.h, object_id.encode(), arr, n))

    def remove_object(self, object_id):
        lib().smplx_world_remove_object.argtypes = [C.c_void_p, C.c_char_p]
        _chk(lib().smplx_world_remove_object(self.h, object_id.encode()))

    def remove_all_objects(self):
        lib().smplx_world_remove_all.argtypes = [C.c_void_p]
        _chk(lib().smplx_world_remove_all(self.h))

    def objects(self):
        """ids in insertion order"""
        L = lib()
        L.smplx_world_objects.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_int)]
        n = C.c_int(0)
        cap = 256
        while True:
            buf = C.create_string_buffer(cap)
            _chk(L.smplx_world_objects(self.h, buf, cap, C.byref(n)))
            names = buf.value.decode().split("\n")[:-1]
            if len(names) == n.value and (n.value == 0 or buf.value.endswith(b"\n")):
                return names
            cap *= 4

    def object_cells(self, object_id, shape=0):
        """the cells (n x 3) shape `shape` of the object was voxelised into, in ExtractVoxels order; for an octree one
        cell per sample point inside the grid, in generation order, duplicates kept"""
        L = lib()
        L.smplx_world_object_cells.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _ip, C.c_int, C.POINTER(C.c_int)]
        n = C.c_int(0)
        _chk(L.smplx_world_object_cells(self.h, object_id.encode(), shape, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), np.int32)
        _chk(L.smplx_world_object_cells(self.h, object_id.encode(), shape, _p(out, _ip), n.value, C.byref(n)))
        return out

    def voxelize(self, shapes):
        """runs the voxeliser and changes nothing: one cell array (n x 3) per shape"""
        arr, n, keep = _shape_array(shapes)
        L = lib()
        L.smplx_world_voxelize.argtypes = [C.c_void_p, C.POINTER(ShapeStruct), C.c_int, _ip, C.c_int, _ip]
        first = np.zeros(n + 1, np.int32)
        cap = 4096
        while True:
            cells = np.zeros((cap, 3), np.int32)
            _chk(L.smplx_world_voxelize(self.h, arr, n, _p(cells, _ip), cap, _p(first, _ip)))
            if first[n] <= cap:
                return [cells[first[i]:first[i + 1]].copy() for i in range(n)]
            cap = int(first[n])

    # ---- robot body (include/smpl_amd.h "robot body")
    def put_body(self, body):
        """places every dirty voxels state of a link outside the group: one field edit, or none when nothing is dirty"""
        lib().smplx_grid_put_body.argtypes = [C.c_void_p, C.c_void_p]
        _chk(lib().smplx_grid_put_body(self.h, body.h))

    def take_body(self):
        lib().smplx_grid_take_body.argtypes = [C.c_void_p]
        _chk(lib().smplx_grid_take_body(self.h))

    def body_cells(self, model):
        """the stored list of one model (n x 3): one cell per point in point order, (-1, -1, -1) outside the grid"""
        L = lib()
        L.smplx_grid_body_cells.argtypes = [C.c_void_p, C.c_int, _ip, C.c_int, C.POINTER(C.c_int)]
        n = C.c_int(0)
        _chk(L.smplx_grid_body_cells(self.h, model, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), np.int32)
        if n.value:
            _chk(L.smplx_grid_body_cells(self.h, model, _p(out, _ip), n.value, C.byref(n)))
        return out

    def close(self):
        if self.h:
            lib().smplx_grid_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Body:
    """The robot body (include/smpl_amd.h "robot body"): links outside the planning group with their voxel models, built
    on the GPU at creation.  The text's errors are found before any GPU is touched."""

    def __init__(self, body_text: str):
        self.h = C.c_void_p()
        L = lib()
        L.smplx_body_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.smplx_body_destroy.argtypes = [C.c_void_p]
        L.smplx_body_destroy.restype = None
        _chk(L.smplx_body_create(body_text.encode(), C.byref(self.h)))
        c = [C.c_int() for _ in range(5)]
        L.smplx_body_counts.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 5
        _chk(L.smplx_body_counts(self.h, *[C.byref(x) for x in c]))
        self.nlinks, self.njoints, self.nmodels, self.noutside, self.npoints = [x.value for x in c]

    def set_joint(self, joint, q):
        lib().smplx_body_set_joint.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        _chk(lib().smplx_body_set_joint(self.h, joint.encode(), float(q)))

    def joint(self, joint):
        q = C.c_double(0.0)
        lib().smplx_body_joint.argtypes = [C.c_void_p, C.c_char_p, _dp]
        _chk(lib().smplx_body_joint(self.h, joint.encode(), C.byref(q)))
        return q.value

    def link_transforms(self):
        """[nlinks][3][4] world frames in the order of the text's link rows"""
        T = np.zeros((self.nlinks, 3, 4))
        lib().smplx_body_link_transforms.argtypes = [C.c_void_p, _dp]
        _chk(lib().smplx_body_link_transforms(self.h, _p(T, _dp)))
        return T

    def model_link(self, model):
        l = C.c_int(-1)
        lib().smplx_body_model_link.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        _chk(lib().smplx_body_model_link(self.h, model, C.byref(l)))
        return l.value

    def model_points(self, model):
        """the link-frame points of one model (n x 3), in order"""
        L = lib()
        L.smplx_body_model_points.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int, C.POINTER(C.c_int)]
        n = C.c_int(0)
        _chk(L.smplx_body_model_points(self.h, model, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3))
        if n.value:
            _chk(L.smplx_body_model_points(self.h, model, _p(out, _dp), n.value, C.byref(n)))
        return out

    def dirty(self):
        out = np.zeros(max(1, self.nmodels), np.uint8)
        lib().smplx_body_dirty.argtypes = [C.c_void_p, _up]
        _chk(lib().smplx_body_dirty(self.h, _p(out, _up)))
        return out[:self.nmodels].astype(bool)

    def close(self):
        if self.h:
            lib().smplx_body_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """Compiled robot model (host-side compile; no GPU needed)."""

    def __init__(self, robot_text: str):
        self.h = C.c_void_p()
        _chk(lib().smplx_model_create(robot_text.encode(), C.byref(self.h)))
        c = [C.c_int() for _ in range(6)]
        _chk(lib().smplx_model_counts(self.h, *[C.byref(x) for x in c]))
        self.njoints, self.nvars, self.ntrees, self.nnodes, self.npairs, self.nslots = [x.value for x in c]

    def arrays(self):
        L = lib()
        origins = np.zeros((self.njoints, 12)); k = np.zeros(self.njoints); fi = np.zeros(self.njoints, np.int32)
        _chk(L.smplx_model_joints(self.h, _p(origins, _dp), _p(k, _dp), _p(fi, _ip)))
        xyzr = np.zeros((self.nnodes, 4)); left = np.zeros(self.nnodes, np.int32); right = np.zeros(self.nnodes, np.int32)
        first = np.zeros(self.ntrees + 1, np.int32)
        _chk(L.smplx_model_nodes(self.h, _p(xyzr, _dp), _p(left, _ip), _p(right, _ip), _p(first, _ip)))
        pairs = np.zeros((self.npairs, 2), np.int32)
        if self.npairs:
            _chk(L.smplx_model_pairs(self.h, _p(pairs, _ip)))
        return dict(origins=origins, k=k, file_index=fi, xyzr=xyzr, left=left, right=right, tree_first=first, pairs=pairs)

    def close(self):
        if self.h:
            lib().smplx_model_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Space:
    """ManipLattice + BfsHeuristic + CollisionSpace for one query, on one GPU."""

    def __init__(self, model: Model, grid: Grid, mprim_text: str, params, batch_states: int = 0, fused: bool = False,
                 tiny_work_list: bool = False, no_small_kernel: bool = False, generic_kernels: bool = False,
                 padding: float = 0.0, heuristic: int = H_BFS):
        self.model, self.grid = model, grid
        P = Params()
        for i, r in enumerate(params.resolutions):
            P.resolutions[i] = r
        P.bfs_inflation_radius = params.bfs_radius
        P.cost_per_cell = params.cost_per_cell
        P.use_short_dist_mprims = int(params.use_short)
        P.short_dist_mprims_thresh = params.short_thresh
        P.use_xyzrpy_snap_mprim = int(params.use_xyzrpy_snap)
        P.xyzrpy_snap_dist_thresh = params.xyzrpy_thresh
        P.xy_rotate_by_var3 = int(params.xy_rotate_by_var3)
        P.use_long_and_short = int(params.use_long_and_short)
        P.padding = padding
        P.batch_states = batch_states
        P.flags = (1 if fused else 0) | (4 if no_small_kernel else 0) | (8 if generic_kernels else 0)
        P.heuristic = int(heuristic)
        self.heuristic = int(heuristic)
        self.h = C.c_void_p()
        _chk(lib().smplx_space_create(model.h, grid.h, mprim_text.encode(), C.byref(P), C.byref(self.h)))
        if tiny_work_list:   # test hook (smpl_amd/csrc/test_hooks.h; not part of include/smpl_amd.h)
            lib().smplx_test_set_work_list_items.argtypes = [C.c_void_p, C.c_int]
            _chk(lib().smplx_test_set_work_list_items(self.h, 8 * 16))
        self.N = lib().smplx_space_num_vars(self.h)
        self.M = lib().smplx_space_num_prims(self.h)

    @classmethod
    def from_config(cls, cfg, batch_states: int = 0, xy_rotate=None, fused: bool = False, tiny_work_list: bool = False,
                    no_small_kernel: bool = False, generic_kernels: bool = False, padding: float = 0.0, heuristic: int = H_BFS,
                    grid=None):
        g = grid if grid is not None else Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
        m = Model(cfg.robot_text)
        p = cfg.params
        if xy_rotate is not None:
            import copy
            p = copy.copy(p)
            p.xy_rotate_by_var3 = xy_rotate
        return cls(m, g, cfg.mprim, p, batch_states, fused, tiny_work_list, no_small_kernel, generic_kernels, padding, heuristic)

    def specialized(self):
        """(True/False, note): whether the space runs the per-robot kernel build (smplx_space_specialized)."""
        buf = C.create_string_buffer(4096)
        lib().smplx_space_specialized.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        r = lib().smplx_space_specialized(self.h, buf, 4096)
        return bool(r), buf.value.decode(errors="replace")

    def close(self):
        if self.h:
            lib().smplx_space_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def discretization(self):
        v = np.zeros(self.N, np.int32); d = np.zeros(self.N)
        _chk(lib().smplx_space_discretization(self.h, _p(v, _ip), _p(d, _dp)))
        return v, d

    def check_joint_limits(self, q):
        q = _f64(q).reshape(-1, self.N); out = np.zeros(q.shape[0], np.uint8)
        lib().smplx_check_joint_limits.argtypes = [C.c_void_p, _dp, C.c_int, _up]
        _chk(lib().smplx_check_joint_limits(self.h, _p(q, _dp), q.shape[0], _p(out, _up)))
        return out

    # ---- CollisionChecker ----
    def state_valid_batch(self, q):
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        out = np.zeros(n, np.uint8); lk = np.zeros(n, np.int32)
        _chk(lib().smplx_cc_state_valid_batch(self.h, _p(q, _dp), n, _p(out, _up), _p(lk, _ip)))
        return out, lk

    def state_valid_batch_device(self, d_q, n, d_valid, d_lookups, stream):
        """Raw device pointers (ints); launches on `stream`, does not synchronise."""
        lib().smplx_cc_state_valid_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(lib().smplx_cc_state_valid_batch_device(self.h, d_q, n, d_valid, d_lookups, stream))

    def edge_valid_batch(self, a, b):
        a = _f64(a).reshape(-1, self.N); b = _f64(b).reshape(-1, self.N); n = a.shape[0]
        out = np.zeros(n, np.uint8); lk = np.zeros(n, np.int32); w = np.zeros(n, np.int32)
        _chk(lib().smplx_cc_edge_valid_batch(self.h, _p(a, _dp), _p(b, _dp), n, _p(out, _up), _p(lk, _ip), _p(w, _ip)))
        return out, lk, w

    def interpolate(self, a, b, cap=4096):
        a = _f64(a); b = _f64(b); out = np.zeros((cap, self.N)); n = C.c_int()
        _chk(lib().smplx_cc_interpolate(self.h, _p(a, _dp), _p(b, _dp), _p(out, _dp), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy(), n.value

    def sphere_positions(self, q):
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        out = np.zeros((n, self.model.nnodes, 3))
        _chk(lib().smplx_cc_sphere_positions(self.h, _p(q, _dp), n, _p(out, _dp)))
        return out

    # ---- CollisionDistanceExtension: distance to collision (include/smpl_amd.h has the specification) ----
    def state_clearance_batch(self, q):
        """(clearance[n], parts[n, 2] = {world, self}, witness[n, 4] = {kind, a, b, waypoint}) of n states, in metres"""
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        clr = np.zeros(n); parts = np.zeros((n, 2)); wit = np.zeros((n, 4), np.int32)
        lib().smplx_cc_state_clearance_batch.argtypes = [C.c_void_p, _dp, C.c_int, _dp, _dp, _ip]
        _chk(lib().smplx_cc_state_clearance_batch(self.h, _p(q, _dp), n, _p(clr, _dp), _p(parts, _dp), _p(wit, _ip)))
        return clr, parts, wit

    def state_clearance_batch_device(self, d_q, n, d_clearance, d_parts, d_witness, stream):
        """Raw device pointers (ints; d_parts and d_witness may be None); launches on `stream`, does not synchronise."""
        lib().smplx_cc_state_clearance_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                                C.c_void_p, C.c_void_p]
        _chk(lib().smplx_cc_state_clearance_batch_device(self.h, d_q, n, d_clearance, d_parts, d_witness, stream))

    def edge_clearance_batch(self, a, b):
        """state_clearance_batch's triple for n edges a[i] -> b[i]: the minimum over each edge's waypoints"""
        a = _f64(a).reshape(-1, self.N); b = _f64(b).reshape(-1, self.N); n = a.shape[0]
        assert b.shape == a.shape
        clr = np.zeros(n); parts = np.zeros((n, 2)); wit = np.zeros((n, 4), np.int32)
        lib().smplx_cc_edge_clearance_batch.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _dp, _dp, _ip]
        _chk(lib().smplx_cc_edge_clearance_batch(self.h, _p(a, _dp), _p(b, _dp), n, _p(clr, _dp), _p(parts, _dp), _p(wit, _ip)))
        return clr, parts, wit

    # ---- attached collision bodies (CollisionSpace::attachObject / detachObject) ----
    def attach_body(self, body_id, link, spheres, allowed=()):
        """spheres: n x (x, y, z, r) in the frame of `link`; allowed: link names and body ids the body may touch"""
        sp = _f64(spheres).reshape(-1, 4)
        names = [str(a).encode() for a in allowed]
        arr = (C.c_char_p * max(1, len(names)))(*names)
        L = lib()
        L.smplx_attach_body.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, _dp, C.c_int, C.POINTER(C.c_char_p), C.c_int]
        _chk(L.smplx_attach_body(self.h, str(body_id).encode(), str(link).encode(), _p(sp, _dp), sp.shape[0], arr, len(names)))

    def attach_object(self, body_id, link, shapes, allowed=(), radius=ATTACHED_SPHERE_RADIUS):
        """CollisionSpace::attachObject: shapes (box() / sphere() / cylinder() / cone() / mesh(), poses in the frame of
        `link`) voxelised on the GPU into spheres of `radius`, then attached like attach_body's"""
        arr, n, keep = _shape_array(shapes)
        names = [str(a).encode() for a in allowed]
        al = (C.c_char_p * max(1, len(names)))(*names)
        L = lib()
        L.smplx_attach_object.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(ShapeStruct), C.c_int, C.c_double,
                                          C.POINTER(C.c_char_p), C.c_int]
        _chk(L.smplx_attach_object(self.h, str(body_id).encode(), str(link).encode(), arr, n, float(radius), al, len(names)))

    def object_spheres(self, shapes, radius=ATTACHED_SPHERE_RADIUS):
        """what attach_object would attach, changing nothing: (xyzr (m x 4), first (n + 1): shape k owns rows
        first[k]:first[k + 1])"""
        arr, n, keep = _shape_array(shapes)
        L = lib()
        L.smplx_object_spheres.argtypes = [C.c_void_p, C.POINTER(ShapeStruct), C.c_int, C.c_double, _dp, C.c_int, _ip]
        first = np.zeros(n + 1, np.int32)
        cap = 1024
        while True:
            xyzr = np.zeros((cap, 4))
            _chk(L.smplx_object_spheres(self.h, arr, n, float(radius), _p(xyzr, _dp), cap, _p(first, _ip)))
            if first[n] <= cap:
                return xyzr[:first[n]].copy(), first
            cap = int(first[n])

    def detach_body(self, body_id):
        lib().smplx_detach_body.argtypes = [C.c_void_p, C.c_char_p]
        _chk(lib().smplx_detach_body(self.h, str(body_id).encode()))

    def attached_bodies(self):
        """[{id, link, first, count}] in attach order: each body's range of nodes in attached_nodes / attached_positions"""
        L = lib()
        L.smplx_attached_bodies.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _ip, _ip]
        first = np.zeros(8, np.int32); cnt = np.zeros(8, np.int32)
        buf = C.create_string_buffer(8 * 600)
        n = L.smplx_attached_bodies(self.h, buf, len(buf), _p(first, _ip), _p(cnt, _ip))
        _chk(min(n, 0))
        lines = buf.value.decode().splitlines()
        return [dict(id=lines[b].split(" ")[0], link=lines[b].split(" ")[1], first=int(first[b]), count=int(cnt[b]))
                for b in range(n)]

    def attached_nodes(self):
        """(xyzr in the link frame, left child, right child; -1 for a leaf) of every body tree node"""
        L = lib()
        L.smplx_attached_nodes.argtypes = [C.c_void_p, _dp, _ip, _ip]
        n = L.smplx_attached_nodes(self.h, None, None, None)
        _chk(min(n, 0))
        xyzr = np.zeros((n, 4)); left = np.zeros(n, np.int32); right = np.zeros(n, np.int32)
        if n:
            _chk(min(L.smplx_attached_nodes(self.h, _p(xyzr, _dp), _p(left, _ip), _p(right, _ip)), 0))
        return xyzr, left, right

    def attached_positions(self, q):
        """world positions of every body tree node: [n states][nodes][3]"""
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        nn = sum(b["count"] for b in self.attached_bodies())
        out = np.zeros((n, nn, 3))
        lib().smplx_cc_attached_positions.argtypes = [C.c_void_p, _dp, C.c_int, _dp]
        _chk(lib().smplx_cc_attached_positions(self.h, _p(q, _dp), n, _p(out, _dp)))
        return out

    # ---- heuristic ----
    def set_goal_joint(self, angles, tol):
        a = _f64(angles); t = _f64(tol)
        _chk(lib().smplx_set_goal_joint(self.h, _p(a, _dp), _p(t, _dp)))

    def set_goal_xyz(self, xyz, tol):
        a = _f64(xyz); t = _f64(tol)
        _chk(lib().smplx_set_goal_xyz(self.h, _p(a, _dp), _p(t, _dp)))

    @staticmethod
    def set_goals_joint_multi(spaces, angles, tols):
        """set_goal_joint for spaces[q] with row q of angles / tols, the BFS runs of all goals in one shared
        sequence of launches (smplx_set_goals_joint_multi)."""
        nq = len(spaces)
        a = _f64(angles).reshape(nq, -1); t = _f64(tols).reshape(nq, -1)
        H = (C.c_void_p * max(nq, 1))(*[sp.h for sp in spaces])
        lib().smplx_set_goals_joint_multi.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        _chk(lib().smplx_set_goals_joint_multi(H, nq, _p(a, _dp), _p(t, _dp)))

    @staticmethod
    def set_goals_xyz_multi(spaces, xyz, tols):
        """set_goal_xyz for spaces[q] with row q of xyz / tols in one call (smplx_set_goals_xyz_multi)."""
        nq = len(spaces)
        a = _f64(xyz).reshape(nq, 3); t = _f64(tols).reshape(nq, 3)
        H = (C.c_void_p * max(nq, 1))(*[sp.h for sp in spaces])
        lib().smplx_set_goals_xyz_multi.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        _chk(lib().smplx_set_goals_xyz_multi(H, nq, _p(a, _dp), _p(t, _dp)))

    def set_goal_pose(self, xyz, rpy, xyz_tol, rpy_tol):
        """XYZ_RPY goal: the XYZ goal's position box and, inside it, rpy_angle(link, rpy) < rpy_tol (smplx_set_goal_pose)."""
        a = _f64(xyz); r = _f64(rpy); t = _f64(xyz_tol)
        _chk(lib().smplx_set_goal_pose(self.h, _p(a, _dp), _p(r, _dp), _p(t, _dp), float(rpy_tol)))

    @staticmethod
    def set_goals_pose_multi(spaces, xyz, rpy, xyz_tols, rpy_tols):
        """set_goal_pose for spaces[q] with row q of the arrays in one call (smplx_set_goals_pose_multi)."""
        nq = len(spaces)
        a = _f64(xyz).reshape(nq, 3); r = _f64(rpy).reshape(nq, 3); t = _f64(xyz_tols).reshape(nq, 3); rt = _f64(rpy_tols).reshape(nq)
        H = (C.c_void_p * max(nq, 1))(*[sp.h for sp in spaces])
        _chk(lib().smplx_set_goals_pose_multi(H, nq, _p(a, _dp), _p(r, _dp), _p(t, _dp), _p(rt, _dp)))

    def goal_pose(self):
        x = np.zeros(3)
        _chk(lib().smplx_goal_pose(self.h, _p(x, _dp)))
        return x

    rpy_angle = staticmethod(rpy_angle)

    def goal_orientation(self):
        """(rpy, rpy_tol) of a pose goal; raises (SMPLX_E_STATE) for any other goal"""
        r = np.zeros(3); t = C.c_double(0.0)
        _chk(lib().smplx_goal_orientation(self.h, _p(r, _dp), C.byref(t)))
        return r, t.value

    def planning_pose_batch(self, q):
        """planning-link transforms of n states, [n][3][4] (computePlanningLinkFK)"""
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        T = np.zeros((n, 3, 4))
        _chk(lib().smplx_planning_pose_batch(self.h, _p(q, _dp), n, _p(T, _dp)))
        return T

    def heuristic_batch(self, q):
        q = _f64(q).reshape(-1, self.N); n = q.shape[0]
        h = np.zeros(n, np.int32); xyz = np.zeros((n, 3))
        _chk(lib().smplx_heuristic_batch(self.h, _p(q, _dp), n, _p(h, _ip), _p(xyz, _dp)))
        return h, xyz

    def metric_goal_distance(self, xyz):
        xyz = _f64(xyz).reshape(-1, 3); out = np.zeros(xyz.shape[0])
        _chk(lib().smplx_bfs_metric_goal_distance(self.h, _p(xyz, _dp), xyz.shape[0], _p(out, _dp)))
        return out

    def heuristic_metric_goal_distance(self, xyz):
        """getMetricGoalDistance of the space's heuristic kind (smplx_metric_goal_distance): the BFS's for H_BFS"""
        xyz = _f64(xyz).reshape(-1, 3); out = np.zeros(xyz.shape[0])
        _chk(lib().smplx_metric_goal_distance(self.h, _p(xyz, _dp), xyz.shape[0], _p(out, _dp)))
        return out

    def goal_rotation(self):
        """Test hook (csrc/test_hooks.h smplx_test_goal_rotation): the goal rotation an H_EUCLID space measures against"""
        R = np.zeros((3, 3))
        _chk(lib().smplx_test_goal_rotation(self.h, _p(R, _dp)))
        return R

    def set_euclid_weights(self, w):
        """setWeightX / Y / Z / Rot of an H_EUCLID space; the goal must be set again afterwards"""
        ww = _f64(w).reshape(4)
        _chk(lib().smplx_set_euclid_weights(self.h, _p(ww, _dp)))

    def metric_start_distance(self, xyz):
        xyz = _f64(xyz).reshape(-1, 3); out = np.zeros(xyz.shape[0])
        _chk(lib().smplx_bfs_metric_start_distance(self.h, _p(xyz, _dp), xyz.shape[0], _p(out, _dp)))
        return out

    def status(self):
        buf = C.create_string_buffer(1024)
        lib().smplx_space_status.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        return lib().smplx_space_status(self.h, buf, 1024), buf.value.decode(errors="replace")

    def bfs_grid(self):
        n = lib().smplx_bfs_size(self.h)
        out = np.zeros(n, np.int32)
        _chk(lib().smplx_bfs_copy(self.h, _p(out, _ip)))
        g = self.grid.dims
        return out.reshape(g[2] + 2, g[1] + 2, g[0] + 2)

    def bfs_size(self):
        """cells of the padded BFS grid; 0 for a space of a closed-form heuristic kind, which has none"""
        return lib().smplx_bfs_size(self.h)

    def bfs_levels(self):
        return lib().smplx_bfs_levels(self.h)

    # ---- lattice ----
    def expand_batch(self, q):
        q = _f64(q).reshape(-1, self.N); B = q.shape[0]; M, N = self.M, self.N
        flags = np.zeros((B, M), np.uint8); coord = np.zeros((B, M, N), np.int32); sq = np.zeros((B, M, N))
        h = np.zeros((B, M), np.int32); cost = np.zeros((B, M), np.int32); lk = np.zeros((B, M), np.int32)
        _chk(lib().smplx_expand_batch(self.h, _p(q, _dp), B, _p(flags, _up), _p(coord, _ip), _p(sq, _dp), _p(h, _ip),
                                      _p(cost, _ip), _p(lk, _ip)))
        return dict(flags=flags, coord=coord, q=sq, h=h, cost=cost, lookups=lk)

    def table_sync(self):
        _chk(lib().smplx_table_sync(self.h))

    def compact_rec_b_bytes(self):
        lib().smplx_compact_rec_b_bytes.restype = C.c_size_t
        return lib().smplx_compact_rec_b_bytes(self.h)

    def compact_blocks(self, B):
        return lib().smplx_compact_blocks(self.h, B)

    def expand_batch_k5(self, q, cap_a=None, cap_b=None):
        """Dense outputs + device-table ids + the compacted successor stream (decoded into per-state lists)."""
        q = _f64(q).reshape(-1, self.N); B = q.shape[0]; M, N = self.M, self.N
        cap_a = lib().smplx_compact_capacity(self.h, B) if cap_a is None else cap_a
        cap_b = lib().smplx_compact_capacity(self.h, B) if cap_b is None else cap_b
        flags = np.zeros((B, M), np.uint8); coord = np.zeros((B, M, N), np.int32); sq = np.zeros((B, M, N))
        h = np.zeros((B, M), np.int32); sid = np.zeros((B, M), np.int32)
        rb = self.compact_rec_b_bytes(); nb = self.compact_blocks(B)
        rec_a = np.zeros((cap_a, 2), np.int32); rec_b = np.zeros((cap_b, rb), np.uint8)
        bt = np.zeros((nb, 4), np.int32); tot = np.zeros(3, np.int32)
        lib().smplx_expand_batch_k5.argtypes = [C.c_void_p, _dp, C.c_int, _up, _ip, _dp, _ip, _ip, _ip, C.c_int, C.c_void_p, C.c_int,
                                                _ip, _ip]
        _chk(lib().smplx_expand_batch_k5(self.h, _p(q, _dp), B, _p(flags, _up), _p(coord, _ip), _p(sq, _dp), _p(h, _ip), _p(sid, _ip),
                                         _p(rec_a, _ip), cap_a, rec_b.ctypes.data_as(C.c_void_p), cap_b, _p(bt, _ip), _p(tot, _ip)))
        return dict(flags=flags, coord=coord, q=sq, h=h, succ_id=sid, rec_a=rec_a, rec_b=rec_b, block_tab=bt, totals=tot)

    def expand_batch_k5_device(self, d_q, B, d_flags, d_coord, d_sq, d_h, d_cost, d_lookups, d_id, d_rec_a, cap_a, d_rec_b, cap_b,
                               d_block_tab, d_totals, d_work, d_counters, stream):
        lib().smplx_expand_batch_k5_device.argtypes = ([C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_int] +
                                                       [C.c_void_p] * 5)
        _chk(lib().smplx_expand_batch_k5_device(self.h, d_q, B, d_flags, d_coord, d_sq, d_h, d_cost, d_lookups, d_id, d_rec_a, cap_a,
                                                d_rec_b, cap_b, d_block_tab, d_totals, d_work, d_counters, stream))

    def expand_work_bytes(self, B):
        return lib().smplx_expand_work_bytes(self.h, B)

    def counters_bytes(self, B):
        return lib().smplx_counters_bytes(self.h, B)

    def counters_read(self, d_counters, B):
        out = np.zeros(6, np.uint64)
        _chk(lib().smplx_counters_read(self.h, d_counters, B, _p(out, _u64p)))
        return [int(x) for x in out]

    def expand_batch_device(self, d_q, B, d_flags, d_coord, d_sq, d_h, d_cost, d_lookups, d_work, d_counters, stream):
        """All arguments are raw device pointers (ints); launches on `stream`, does not synchronise."""
        _chk(lib().smplx_expand_batch_device(self.h, d_q, B, d_flags, d_coord, d_sq, d_h, d_cost, d_lookups, d_work,
                                             d_counters, stream))

    def profile_begin(self, max_launches):
        _chk(lib().smplx_profile_begin(self.h, max_launches))

    def profile_end(self):
        a, b, n = C.c_double(), C.c_double(), C.c_int()
        _chk(lib().smplx_profile_end(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def set_start(self, q):
        q = _f64(q); i = C.c_int()
        _chk(lib().smplx_set_start(self.h, _p(q, _dp), C.byref(i)))
        return i.value

    def get_succs(self, i):
        s = np.zeros(self.M, np.int32); k = np.zeros(self.M, np.int32); n = C.c_int()
        _chk(lib().smplx_get_succs(self.h, i, _p(s, _ip), _p(k, _ip), self.M, C.byref(n)))
        return s[:n.value].copy(), k[:n.value].copy()

    # ---- lazy successors: GetLazySuccs / GetTrueCost (include/smpl_amd.h has the specification) ----
    def get_lazy_succs(self, i):
        """(ids, costs) of GetLazySuccs(i): every active action's state, unchecked; the goal id for a goal successor"""
        s = np.zeros(self.M, np.int32); k = np.zeros(self.M, np.int32); n = C.c_int()
        lib().smplx_get_lazy_succs.argtypes = [C.c_void_p, C.c_int, _ip, _ip, C.c_int, C.POINTER(C.c_int)]
        _chk(lib().smplx_get_lazy_succs(self.h, i, _p(s, _ip), _p(k, _ip), self.M, C.byref(n)))
        return s[:n.value].copy(), k[:n.value].copy()

    def get_true_cost(self, parent, child):
        """GetTrueCost(parent, child): 1000, or -1 when no matching action passes limits and the edge check"""
        c = C.c_int32()
        lib().smplx_get_true_cost.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        _chk(lib().smplx_get_true_cost(self.h, parent, child, C.byref(c)))
        return c.value

    def true_cost_batch(self, parents, children):
        """(costs, prims, nmatch) of n (parent id, child id) pairs in one launch"""
        a = np.ascontiguousarray(parents, np.int32).reshape(-1); b = np.ascontiguousarray(children, np.int32).reshape(-1)
        assert a.shape == b.shape
        n = a.shape[0]
        cost = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); nm = np.zeros(n, np.int32)
        lib().smplx_true_cost_batch.argtypes = [C.c_void_p, _ip, _ip, C.c_int, _ip, _ip, _ip]
        _chk(lib().smplx_true_cost_batch(self.h, _p(a, _ip), _p(b, _ip), n, _p(cost, _ip), _p(prim, _ip), _p(nm, _ip)))
        return cost, prim, nm

    def lazy_expand_batch(self, q):
        """Dense rows of k_lazy_succs for arbitrary parent states: flags (0x10 inactive; else 4, plus 2 for a goal), coord, q,
        h and succ_id (device-table id, -1 = unknown), indexed [state][prim].  Creates no state."""
        q = _f64(q).reshape(-1, self.N); B = q.shape[0]; M, N = self.M, self.N
        flags = np.zeros((B, M), np.uint8); coord = np.zeros((B, M, N), np.int32); sq = np.zeros((B, M, N))
        h = np.zeros((B, M), np.int32); sid = np.zeros((B, M), np.int32)
        lib().smplx_lazy_expand_batch.argtypes = [C.c_void_p, _dp, C.c_int, _up, _ip, _dp, _ip, _ip]
        _chk(lib().smplx_lazy_expand_batch(self.h, _p(q, _dp), B, _p(flags, _up), _p(coord, _ip), _p(sq, _dp), _p(h, _ip), _p(sid, _ip)))
        return dict(flags=flags, coord=coord, q=sq, h=h, succ_id=sid)

    def lazy_expand_batch_device(self, d_q, B, d_flags, d_coord, d_sq, d_h, d_id, stream):
        """Raw device pointers (ints; all but d_flags may be None); launches on `stream`, does not synchronise."""
        lib().smplx_lazy_expand_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _chk(lib().smplx_lazy_expand_batch_device(self.h, d_q, B, d_flags, d_coord, d_sq, d_h, d_id, stream))

    def true_cost_q_batch(self, parent_q, child_coord, goal_edge=None):
        """(costs, prims, nmatch) of n items of k_true_cost: a parent's joint values and either the child's coordinate or,
        where goal_edge is set, "the child is the goal" """
        q = _f64(parent_q).reshape(-1, self.N); n = q.shape[0]
        c = np.ascontiguousarray(child_coord, np.int32).reshape(n, self.N)
        g = np.zeros(n, np.uint8) if goal_edge is None else np.ascontiguousarray(goal_edge, np.uint8).reshape(n)
        cost = np.zeros(n, np.int32); prim = np.zeros(n, np.int32); nm = np.zeros(n, np.int32)
        lib().smplx_true_cost_q_batch.argtypes = [C.c_void_p, _dp, _ip, _up, C.c_int, _ip, _ip, _ip]
        _chk(lib().smplx_true_cost_q_batch(self.h, _p(q, _dp), _p(c, _ip), _p(g, _up), n, _p(cost, _ip), _p(prim, _ip), _p(nm, _ip)))
        return cost, prim, nm

    def true_cost_work_doubles(self, n):
        """doubles of scratch true_cost_q_batch_device needs for n items"""
        lib().smplx_true_cost_work_doubles.restype = C.c_size_t
        lib().smplx_true_cost_work_doubles.argtypes = [C.c_void_p, C.c_int]
        return lib().smplx_true_cost_work_doubles(self.h, n)

    def true_cost_q_batch_device(self, d_parent_q, d_child_coord, d_goal_edge, n, d_work_q, d_costs, d_prims, d_nmatch, stream):
        """Raw device pointers (ints; d_prims and d_nmatch may be None); launches on `stream`, does not synchronise."""
        lib().smplx_true_cost_q_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        _chk(lib().smplx_true_cost_q_batch_device(self.h, d_parent_q, d_child_coord, d_goal_edge, n, d_work_q, d_costs, d_prims,
                                                  d_nmatch, stream))

    def lazy_counters(self):
        """smplx_lazy_counters as a dict"""
        out = (C.c_int64 * 6)()
        lib().smplx_lazy_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _chk(lib().smplx_lazy_counters(self.h, out))
        names = ("lazy_launches", "lazy_served", "true_cost_launches", "edges_evaluated", "cache_hits", "cache_misses")
        return dict(zip(names, (int(x) for x in out)))

    def hint_frontier(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        _chk(lib().smplx_hint_frontier(self.h, _p(ids, _ip), ids.shape[0]))

    def goal_heuristic(self, i):
        h = C.c_int32()
        _chk(lib().smplx_get_goal_heuristic(self.h, i, C.byref(h)))
        return h.value

    def num_states(self):
        return lib().smplx_num_states(self.h)

    def get_state(self, i):
        q = np.zeros(self.N); c = np.zeros(self.N, np.int32)
        _chk(lib().smplx_get_state(self.h, i, _p(q, _dp), _p(c, _ip)))
        return q, c

    def search_counters(self):
        """Diagnostics of the device-resident search (smplx_search_counters)."""
        out = (C.c_int64 * 16)()
        lib().smplx_search_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _chk(lib().smplx_search_counters(self.h, out))
        names = ["searches", "grows", "dup_pushes", "t_idle", "t_select_pop", "t_evaluate", "t_commit", "t_relax", "t_reorder", "t_launch_io",
                 "device_states", "heap_cache_entries", "spec_rounds", "spec_hits", "table_allocs", "table_regrows"]
        return {n: int(out[i]) for i, n in enumerate(names)}

    def set_search_helper(self, on):
        """Test hook (csrc/test_hooks.h): run the device search with (default) or without its helper wave."""
        lib().smplx_test_set_search_helper.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_test_set_search_helper(self.h, 1 if on else 0))

    def set_pipe_prep(self, on):
        """Test hook (csrc/test_hooks.h): the pipeline with k_pipe_prep in a launch of its own (four launches) or, the
        default, with the goal distance computed inside k_pipe_setup (three)."""
        lib().smplx_test_set_pipe_prep.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_test_set_pipe_prep(self.h, 1 if on else 0))

    def set_one_launch(self, mode):
        """Test hook (csrc/test_hooks.h): which pipeline steps run as the one launch k_step_block: -1 the rule, 0 never,
        1 whenever the kernel can run at all (a step that then cannot take it raises)."""
        lib().smplx_test_set_one_launch.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_test_set_one_launch(self.h, int(mode)))

    def one_launch_steps(self):
        """Test hook: steps of this space that took k_step_block so far."""
        lib().smplx_test_one_launch_steps.argtypes = [C.c_void_p]
        lib().smplx_test_one_launch_steps.restype = C.c_longlong
        return int(lib().smplx_test_one_launch_steps(self.h))

    def step_counters_zero(self, stream=None):
        """Test hook: waits for `stream` and tells whether the space's step counters of that stream are all-zero."""
        lib().smplx_test_step_counters_zero.argtypes = [C.c_void_p, C.c_void_p]
        r = lib().smplx_test_step_counters_zero(self.h, C.c_void_p(stream))
        if r < 0:
            _chk(r)
        return r == 1

    def set_table_slots(self, slots):
        """Test hook (csrc/test_hooks.h): slots of the first device state table this space allocates (0: the default)."""
        lib().smplx_test_set_table_slots.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_test_set_table_slots(self.h, int(slots)))

    def table_slots(self):
        """Test hook: slots of the space's device state table now (0 while it has none)."""
        lib().smplx_test_table_slots.argtypes = [C.c_void_p]
        lib().smplx_test_table_slots.restype = C.c_longlong
        return int(lib().smplx_test_table_slots(self.h))

    def set_search_capacity(self, states):
        """Test hook (csrc/test_hooks.h): first capacity of the device search's buffers; its path buffer then starts at 64 ids."""
        lib().smplx_test_set_search_capacity.argtypes = [C.c_void_p, C.c_int]
        _chk(lib().smplx_test_set_search_capacity(self.h, int(states)))

    # ---- search ----
    def plan(self, eps0, eps_final, eps_delta, improve=True, bounded=False, max_init=0, max_rep=0, cap=100000):
        P = SearchParams(eps0, eps_final, eps_delta, int(improve), int(bounded), max_init, max_rep)
        S = SearchStats()
        ids = np.zeros(cap, np.int32)
        _chk(lib().smplx_plan(self.h, C.byref(P), _p(ids, _ip), cap, C.byref(S)))
        n = lib().smplx_expansion_log_size(self.h)
        log = np.zeros(n, np.int32)
        if n:
            _chk(lib().smplx_expansion_log(self.h, _p(log, _ip)))
        out = {f: getattr(S, f) for f, _ in SearchStats._fields_}
        out["path"] = ids[:S.path_len].copy()
        out["expansion_log"] = log
        return out

    @staticmethod
    def plan_multi(spaces, eps0, eps_final, eps_delta, improve=True, bounded=False, max_init=0, max_rep=0, cap=4096,
                   host_threads=1):
        """Interleaved ARA* over independent queries on one GPU (smplx_plan_multi)."""
        nq = len(spaces)
        P = SearchParams(eps0, eps_final, eps_delta, int(improve), int(bounded), max_init, max_rep)
        St = (SearchStats * nq)()
        H = (C.c_void_p * nq)(*[sp.h for sp in spaces])
        ids = np.zeros((nq, cap), np.int32)
        wall = C.c_double()
        _chk(lib().smplx_plan_multi(H, nq, C.byref(P), _p(ids, _ip), cap, St, C.byref(wall), int(host_threads)))
        out = []
        for q, sp in enumerate(spaces):
            d = {f: getattr(St[q], f) for f, _ in SearchStats._fields_}
            d["path"] = ids[q, :St[q].path_len].copy()
            n = lib().smplx_expansion_log_size(sp.h)
            log = np.zeros(n, np.int32)
            if n:
                _chk(lib().smplx_expansion_log(sp.h, _p(log, _ip)))
            d["expansion_log"] = log
            out.append(d)
        return out, wall.value

    def _log(self):
        n = lib().smplx_expansion_log_size(self.h)
        log = np.zeros(n, np.int32)
        if n:
            _chk(lib().smplx_expansion_log(self.h, _p(log, _ip)))
        return log

    @staticmethod
    def _replan_dict(S, ids):
        d = {f: getattr(S.s, f) for f, _ in SearchStats._fields_}
        d["path"] = ids[:S.s.path_len].copy()
        d["result"], d["call_expansions"], d["resumed"] = S.result, S.call_expansions, S.resumed
        return d

    def replan(self, eps0, eps_final, eps_delta, improve=True, bounded=False, max_init=0, max_rep=0, wall=False,
               seconds_init=0.0, seconds=0.0, allow_partial=False, from_scratch=False, cap=100000):
        """Anytime ARA* (smplx_replan): continues the space's previous search where include/smpl_amd.h allows it.  The dict of
        plan() plus result (ARA_*), call_expansions and resumed; expansion_log is the whole search's since it started."""
        P = time_params(eps0, eps_final, eps_delta, improve, bounded, max_init, max_rep, wall, seconds_init, seconds,
                        allow_partial, from_scratch)
        S = ReplanStats()
        ids = np.zeros(cap, np.int32)
        _chk(lib().smplx_replan(self.h, C.byref(P), _p(ids, _ip), cap, C.byref(S)))
        out = self._replan_dict(S, ids)
        out["expansion_log"] = self._log()
        return out

    @staticmethod
    def replan_multi(spaces, eps0, eps_final, eps_delta, improve=True, bounded=False, max_init=0, max_rep=0, wall=False,
                     seconds_init=0.0, seconds=0.0, allow_partial=False, from_scratch=False, cap=4096, host_threads=1):
        """smplx_replan_multi: replan() for independent queries on one GPU.  Returns (list of dicts, wall seconds)."""
        nq = len(spaces)
        P = time_params(eps0, eps_final, eps_delta, improve, bounded, max_init, max_rep, wall, seconds_init, seconds,
                        allow_partial, from_scratch)
        St = (ReplanStats * nq)()
        H = (C.c_void_p * nq)(*[sp.h for sp in spaces])
        ids = np.zeros((nq, cap), np.int32)
        wall_s = C.c_double()
        _chk(lib().smplx_replan_multi(H, nq, C.byref(P), _p(ids, _ip), cap, St, C.byref(wall_s), int(host_threads)))
        out = []
        for q, sp in enumerate(spaces):
            d = Space._replan_dict(St[q], ids[q])
            d["expansion_log"] = sp._log()
            out.append(d)
        return out, wall_s.value

    def post_process_path(self, path, shortcut=True, interpolate=True, upstream_limits=False):
        """PlannerInterface::postProcessPath (planner_interface.cpp:2651-2697).  Returns (path, stats)."""
        path = np.ascontiguousarray(path, np.float64).reshape(-1, self.N)
        flags = (1 if shortcut else 0) | (2 if interpolate else 0) | (4 if upstream_limits else 0)
        n = C.c_int(); st = (C.c_int64 * 2)()
        lib().smplx_post_process_path.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip, C.POINTER(C.c_int64)]
        _chk(lib().smplx_post_process_path(self.h, _p(path, _dp), path.shape[0], flags, None, 0, C.byref(n), st))
        out = np.zeros((max(n.value, 1), self.N))
        _chk(lib().smplx_post_process_path(self.h, _p(path, _dp), path.shape[0], flags, _p(out, _dp), out.shape[0], C.byref(n), st))
        return out[:n.value], dict(edge_batches=st[0], configs=st[1])

    def extract_path(self, ids):
        ids = np.ascontiguousarray(ids, np.int32); q = np.zeros((ids.shape[0], self.N))
        _chk(lib().smplx_extract_path(self.h, _p(ids, _ip), ids.shape[0], _p(q, _dp)))
        return q
