"""A plain model of the robot body (include/smpl_amd.h "robot body"): the judge of the body tests.  Nothing here calls the
engine.

Restated (binary64, the reference's operation order):
  - the body text: link / joint rows as in the robot text, geom, voxels, group and value rows;
  - link frames: tests/kinematics_ref.py, fed the link / joint rows (every moving joint as a planning variable);
  - the gridless VoxelizeMesh (smpl/src/geometry/voxelize.cpp:962-986): the HalfResVoxelGrid over the mesh's bounding box
    (HalfResDiscretizer, smpl/include/smpl/geometry/discretize.h:94-113; the grid's range, voxel_grid.h:187-193), every
    triangle's candidates from the discretised minimum to maximum of its vertices (detail/voxelize.hpp:115-122) clipped
    to the grid's range (the engine's deliberate clip), the decision per (triangle, voxel) by tests/voxelize_ref.py with
    the lattice's continuize expressed as the pivot 0.5 * res, ExtractVoxels order, elements appended with duplicates;
  - voxelizeLink (sbpl_collision_checking/src/robot_collision_model.cpp:959-1073): the geom rows of a link in file order;
  - the dirtiness rule (robot_collision_state.cpp:62-96), the group exclusion (:297-314) and the point rule
    (distance_map.hpp:520-527) of a placed point.
Like voxelize_ref it reports, per voxel, whether a comparison it reached came within eps of equality, and per placed
point the distance of inv_res * (w - (origin - res)) + 0.5 from an integer."""
import math

import numpy as np

import kinematics_ref as K
import voxelize_ref as V


# ---- the HalfRes lattice --------------------------------------------------------------------------------------------
def discretize(d, res):
    return int(d / res) if d >= 0 else int(d / res) - 1


def continuize(i, res):
    return float(i) * res + 0.5 * res


def grid_range(vmin, vmax, res):
    """(lo[3], hi[3]) of the HalfResVoxelGrid(origin = min, size = max - min)"""
    lo = [discretize(vmin[a], res) for a in range(3)]
    hi = [discretize(vmin[a] + (vmax[a] - vmin[a]), res) for a in range(3)]
    return lo, hi


def _triangle(p1, p2, p3, res, lo, hi):
    """voxelize_ref's decision over the HalfRes candidates of one triangle, clipped to [lo, hi]"""
    def half_range(a, b, c, origin, r):
        tl = [max(lo[k], discretize(min(a[k], b[k], c[k]), r)) for k in range(3)]
        th = [min(hi[k], discretize(max(a[k], b[k], c[k]), r)) for k in range(3)]
        return tl, th
    saved = V.candidate_range
    V.candidate_range = half_range
    try:
        return V.voxelize_triangle(p1, p2, p3, (0.5 * res,) * 3, res)
    finally:
        V.candidate_range = saved


def voxelize_mesh(vertices, triangles, res, eps=1e-9):
    """-> (cells[n, 3] in ExtractVoxels order, each once; undecided cells[m, 3])"""
    v = np.asarray(vertices, float).reshape(-1, 3)
    lo, hi = grid_range(v.min(axis=0), v.max(axis=0), res)
    filled, near = set(), set()
    for t in np.asarray(triangles, int).reshape(-1, 3):
        cells, f, m = _triangle(v[t[0]], v[t[1]], v[t[2]], res, lo, hi)
        filled.update(map(tuple, cells[f]))
        near.update(map(tuple, cells[m < eps]))
    return np.array(sorted(filled), int).reshape(-1, 3), np.array(sorted(near), int).reshape(-1, 3)


def points_of(cells, res):
    c = np.asarray(cells, int).reshape(-1, 3)
    return c.astype(float) * res + 0.5 * res


# ---- the body text --------------------------------------------------------------------------------------------------
def origin_pose(xyz, rpy):
    """Translation(xyz) * Rz(yaw) * Ry(pitch) * Rx(roll) as 3x4"""
    r, p, y = rpy
    sr, cr, sp, cp, sy, cy = math.sin(r), math.cos(r), math.sin(p), math.cos(p), math.sin(y), math.cos(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, xyz[0]],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, xyz[1]],
                     [-sp, cp * sr, cp * cr, xyz[2]]])


class Body:
    def __init__(self, text):
        self.links, self.joints, self.geoms, self.models, self.group, self.values = [], [], [], [], [], {}
        rows = [l.split("#")[0].split() for l in text.splitlines()]
        rows = [w for w in rows if w]
        i = 0
        while i < len(rows):
            w = rows[i]
            i += 1
            if w[0] == "link":
                self.links.append(w[1])
            elif w[0] == "joint":
                self.joints.append(dict(name=w[1], type=w[2], parent=w[3], child=w[4], row=" ".join(w)))
            elif w[0] == "geom":
                g = dict(link=w[1], shape=w[2])
                if w[2] == "mesh":
                    nv, nt = int(w[3]), int(w[4])
                    o = [float(x) for x in w[5:11]]
                    g["v"] = np.array([[float(x) for x in r[1:4]] for r in rows[i:i + nv]])
                    g["t"] = np.array([[int(x) for x in r[1:4]] for r in rows[i + nv:i + nv + nt]])
                    i += nv + nt
                else:
                    nd = dict(box=3, sphere=1, cylinder=2)[w[2]]
                    g["dims"] = [float(x) for x in w[3:3 + nd]]
                    o = [float(x) for x in w[3 + nd:9 + nd]]
                g["pose"] = origin_pose(o[0:3], o[3:6])
                self.geoms.append(g)
            elif w[0] == "voxels":
                self.models.append(dict(link=w[1], res=float(w[2])))
            elif w[0] == "group":
                self.group = w[2:]
            elif w[0] == "value":
                self.values[w[1]] = float(w[2])
        self.moving = [j["name"] for j in self.joints if j["type"] != "fixed"]
        self.q = {n: self.values.get(n, 0.0) for n in self.moving}
        text = "\n".join(["link " + l for l in self.links] + [j["row"] for j in self.joints] + ["planning_joints " + " ".join(self.moving)])
        self.robot = K.Robot(text)
        self.outside = [m["link"] not in self.group for m in self.models]
        self.dirty = [True] * len(self.models)           # every state starts dirty
        self._points = {}

    # ---- kinematics
    def frames(self):
        """{link: (hi, lo)} of the 3x4 world frame of every link, as kinematics_ref splits them"""
        F = self.robot.frames([self.q[n] for n in self.moving], self.links)
        out = {}
        for l, (R, t) in F.items():
            hi, lo = np.zeros((3, 4)), np.zeros((3, 4))
            for i in range(3):
                for j in range(3):
                    hi[i, j], lo[i, j] = K.split(R[i][j])
                hi[i, 3], lo[i, 3] = K.split(t[i])
            out[l] = (hi, lo)
        return out

    # ---- dirtiness
    def descendants(self, joint):
        child = {j["name"]: j["child"] for j in self.joints}[joint]
        out, grew = {child}, True
        while grew:
            grew = False
            for j in self.joints:
                if j["parent"] in out and j["child"] not in out:
                    out.add(j["child"]); grew = True
        return out

    def set_joint(self, joint, q):
        if self.q[joint] == q:
            return
        self.q[joint] = q
        moved = self.descendants(joint)
        for m, model in enumerate(self.models):
            if model["link"] in moved:
                self.dirty[m] = True

    def put(self):
        """the models a put places, in order; clears their flags"""
        todo = [m for m in range(len(self.models)) if self.outside[m] and self.dirty[m]]
        for m in todo:
            self.dirty[m] = False
        return todo

    # ---- voxel models
    def element_mesh(self, g):
        if g["shape"] == "box":
            v, t = V.box_mesh(*g["dims"])
        elif g["shape"] == "sphere":
            v, t = V.sphere_mesh(g["dims"][0], 7, 8)
        elif g["shape"] == "cylinder":
            v, t = V.cylinder_mesh(*g["dims"])
        else:
            v, t = g["v"], g["t"]
        return V.transform(g["pose"], np.asarray(v, float)), t

    def model_points(self, m, eps=1e-9):
        """-> (points[n, 3] link frame in order, near[n] bool: the voxel is undecided at eps, count of undecided voxels
        that are NOT filled): the elements of the link in file order, duplicates kept"""
        if (m, eps) not in self._points:
            model = self.models[m]
            pts, near, missing = [np.zeros((0, 3))], [np.zeros(0, bool)], []
            for g in self.geoms:
                if g["link"] != model["link"]:
                    continue
                v, t = self.element_mesh(g)
                cells, und = voxelize_mesh(v, t, model["res"], eps)
                und = set(map(tuple, und))
                pts.append(points_of(cells, model["res"]))
                near.append(np.array([tuple(c) in und for c in cells], bool))
                missing += [points_of([c], model["res"])[0] for c in sorted(und - set(map(tuple, cells)))]
            self._points[(m, eps)] = (np.concatenate(pts), np.concatenate(near), np.array(missing).reshape(-1, 3))
        return self._points[(m, eps)]


# ---- placing --------------------------------------------------------------------------------------------------------
def place(T, points, origin, res, dims):
    """-> (cells[n, 3] with (-1, -1, -1) for a point outside the grid, margin[n]: the smallest distance over the three axes
    of inv_res * (w - (origin - res)) + 0.5 from an integer).  T: 3x4 as given."""
    T = np.asarray(T, float).reshape(3, 4)
    p = np.asarray(points, float).reshape(-1, 3)
    inv_res = 1.0 / res
    cells = np.zeros((len(p), 3), np.int64)
    margin = np.full(len(p), np.inf)
    for a in range(3):
        w = (T[a, 0] * p[:, 0] + (T[a, 1] * p[:, 1] + T[a, 2] * p[:, 2])) + T[a, 3]
        f = inv_res * (w - (origin[a] - res)) + 0.5
        cells[:, a] = np.trunc(f).astype(np.int64) - 1
        margin = np.minimum(margin, np.abs(f - np.rint(f)))
    out = np.any((cells < 0) | (cells >= np.asarray(dims)), axis=1)
    cells[out] = -1
    return cells.astype(np.int32), margin


def occupancy_after(steps, dims, counted):
    """replays (remove list, add list) pairs -- cell arrays, (-1, -1, -1) rows skipped -- on an empty grid with the rules
    of k_occ_points: -> (occupied bool[dims], counts int[dims] or None)"""
    counts = np.zeros(dims, np.int64)
    occ = np.zeros(dims, bool)
    for rem, add in steps:
        for cells, sign in ((rem, -1), (add, 1)):
            c = np.asarray(cells, int).reshape(-1, 3)
            c = c[c[:, 0] >= 0]
            if not len(c):
                continue
            if counted:
                if sign > 0:
                    np.add.at(counts, (c[:, 0], c[:, 1], c[:, 2]), 1)
                else:
                    for x, y, z in c:
                        if counts[x, y, z] > 0:
                            counts[x, y, z] -= 1
                occ = counts > 0
            else:
                occ[c[:, 0], c[:, 1], c[:, 2]] = sign > 0
    return occ, (counts.astype(np.int32) if counted else None)
