// smpl_amd/csrc/voxelize.h -- surface voxelisation of triangle meshes (world objects), included by field.hip.
// What it stands behind: sbpl::geometry::VoxelizeTriangle (smpl/include/smpl/geometry/detail/voxelize.hpp:46-180) over the
// PivotVoxelGrid of VoxelizeMesh(..., res, voxel_origin, ...) (smpl/src/geometry/voxelize.cpp:1008-1035), with fill = false
// (sbpl_collision_checking/src/voxel_operations.cpp:319-402): the pivot is the occupancy grid's origin, so voxel index i
// along an axis is cell i of the grid (tests/test_voxelize_model.py shows it through the point rule).
//
// The arithmetic is restated line by line in binary64 under the contract of det_math.h (no fused multiply-add; host and
// device compile this one source): the per-triangle constants (vox_tri_setup) and the per-voxel decision (vox_filled) run
// on the device; the host compiler builds the same source for tests/cpp/voxelize_host_driver.cpp.  Three-term sums follow
// Eigen's unrolled reduction, a0*b0 + (a1*b1 + a2*b2), which is what Vector3d::dot / squaredNorm and the rows of
// Affine3d * Vector3d evaluate.
// Quirks kept on purpose: the edge test runs on the pairs (p1,p3), (p2,p3), (p3,p1) as written, so
// edge p1-p2 is never tested on its own; the corner constant is 0.5774; the candidates of a triangle are exactly the voxels
// between the discretised minimum and maximum of its vertices.
#pragma once

#include "det_math.h"

struct VoxTri {
    double p1[3], p2[3], p3[3];
    double n[3], d, t;
    double e1[3], e2[3], e3[3];
    double d1, d2, d3;
    double rc2;
    int lo[3];        // low corner of the candidate range, clipped to the occupancy grid
    int ny, nz;       // extent of the clipped range along y and z (x follows from the pair count)
    int shape;        // which mask it writes
    int skip;         // the reference skips the triangle (voxelize.hpp:57-60)
};

// what the host lists per triangle: its vertices in the call's vertex array and its clipped candidate range
struct VoxItem {
    int v[3];
    int lo[3];
    int ny, nz;
    int shape;
};

// the mask of one shape: one byte per cell of the shape's clipped bounding range, x-major / z fastest
struct VoxShape {
    long long mask_first;   // first byte of its mask in the call's mask buffer
    long long list_first;   // first cell of its list in the call's cell buffer
    int lo[3], dim[3];
    int first_chunk;        // first entry of the call's chunk counts that belongs to it
    int pad;
};

SMPLX_HD double vox_dot(const double* a, const double* b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
SMPLX_HD void vox_sub(const double* a, const double* b, double* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
// Affine3d * Vector3d (TransformVertices, voxelize.cpp:608-615; `pose * pt`, voxel_operations.cpp:417, 426): R v + t for a
// 3x4 row-major pose
SMPLX_HD void vox_transform(const double* pose, const double* v, double* o)
{
    for (int r = 0; r < 3; ++r) o[r] = vox_dot(pose + 4 * r, v) + pose[4 * r + 3];
}
SMPLX_HD void vox_cross(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// Eigen's normalize(): divide by the norm unless the squared norm is 0
SMPLX_HD void vox_normalize(double* v)
{
    const double z = vox_dot(v, v);
    if (z > 0.0) { const double s = sqrt(z); v[0] /= s; v[1] /= s; v[2] /= s; }
}
// inward normal of an edge: -(edge x n), normalised (voxelize.hpp:98-108)
SMPLX_HD void vox_edge_normal(const double* edge, const double* n, double* e)
{
    vox_cross(edge, n, e);
    e[0] = -e[0]; e[1] = -e[1]; e[2] = -e[2];
    vox_normalize(e);
}

// PivotDiscretizer (smpl/include/smpl/geometry/discretize.h:40-61).  The index is clamped to [-1, n] in double before
// the cast: beyond the grid only "outside" matters, and a far vertex must not overflow an int.
SMPLX_HD int vox_discretize(double w, double pivot, double res, int n)
{
    double f = floor((w - pivot) / res + 0.5);
    if (f < -1.0) f = -1.0;
    if (f > (double)n) f = (double)n;
    return (int)f;
}
// the same index for a lattice whose kept range is [lo, hi] (indices may be negative): clamped to [lo - 1, hi + 1], which
// for the occupancy grid's range [0, n - 1] is vox_discretize
SMPLX_HD int vox_discretize_in(double w, double pivot, double res, int lo, int hi)
{
    double f = floor((w - pivot) / res + 0.5);
    if (f < (double)lo - 1.0) f = (double)lo - 1.0;
    if (f > (double)hi + 1.0) f = (double)hi + 1.0;
    return (int)f;
}
SMPLX_HD double vox_continuize(int i, double pivot, double res) { return pivot + i * res; }

// HalfResDiscretizer (discretize.h:94-113), the lattice of the gridless VoxelizeMesh (voxelize.cpp:962-986) that makes a
// link's voxel model: discretize(d) = d >= 0 ? (int)(d / res) : (int)(d / res) - 1.  Its continuize(i) = i * res + 0.5 * res
// is vox_continuize with the pivot 0.5 * res (the sum commutes, so the bits are the same).  The quotient is clamped to
// +-2^30 in double before the cast: a tiny resolution must not overflow an int (the caller refuses such a model).
SMPLX_HD int vox_half_discretize(double d, double res)
{
    double f = d / res;
    if (f < -1073741824.0) f = -1073741824.0;
    if (f > 1073741824.0) f = 1073741824.0;
    return d >= 0.0 ? (int)f : (int)f - 1;
}

// the constants of one triangle (voxelize.hpp:52-113); false when the triangle is skipped (:57-60)
SMPLX_HD bool vox_tri_setup(const double* p1, const double* p2, const double* p3, double res, VoxTri* T)
{
    double a[3], b[3], c[3];
    vox_sub(p2, p1, a);
    vox_sub(p3, p1, b);
    vox_cross(a, b, c);
    const double det = sqrt(vox_dot(c, c));
    if (det == 0.0) return false;
    for (int k = 0; k < 3; ++k) { T->p1[k] = p1[k]; T->p2[k] = p2[k]; T->p3[k] = p3[k]; }
    const double rc = sqrt(3.0) * 0.5 * res;
    T->rc2 = rc * rc;
    double u[3], v[3], w[3];
    vox_sub(p2, p1, u);
    vox_sub(p3, p2, v);
    vox_sub(p1, p3, w);
    vox_cross(u, v, T->n);
    vox_normalize(T->n);
    double ca = 0.0;
    for (int i = 0; i < 8; ++i) {
        const double corner[3] = {(i & 4) ? 0.5774 : -0.5774, (i & 2) ? 0.5774 : -0.5774, (i & 1) ? 0.5774 : -0.5774};
        const double x = vox_dot(corner, T->n);
        if (i == 0 || x > ca) ca = x;
    }
    T->t = rc * ca;
    T->d = -vox_dot(T->n, p1);
    vox_edge_normal(u, T->n, T->e1);
    vox_edge_normal(v, T->n, T->e2);
    vox_edge_normal(w, T->n, T->e3);
    T->d1 = -vox_dot(T->e1, p1);
    T->d2 = -vox_dot(T->e2, p2);
    T->d3 = -vox_dot(T->e3, p3);
    return true;
}

// Distance(p, q, radius_sqrd, x) != -1.0 (voxelize.cpp:626-649): x projects onto the segment and lies within the radius
SMPLX_HD bool vox_near_edge(const double* p, const double* q, double r2, const double* x)
{
    double pq[3], px[3];
    vox_sub(q, p, pq);
    vox_sub(x, p, px);
    const double d = vox_dot(px, pq);
    const double len2 = vox_dot(pq, pq);
    if (d < 0.0 || d > len2) return false;
    const double dsq = vox_dot(px, px) - (d * d) / len2;
    if (dsq > r2) return false;
    return dsq != -1.0;
}

SMPLX_HD int vox_sign(double v) { return v == 0.0 ? 0 : (v > 0.0 ? 1 : -1); }

// does the triangle fill the voxel centred on x (voxelize.hpp:139-176)
SMPLX_HD bool vox_filled(const VoxTri& T, const double* x)
{
    double dx[3];
    vox_sub(x, T.p1, dx);
    if (vox_dot(dx, dx) <= T.rc2) return true;
    vox_sub(x, T.p2, dx);
    if (vox_dot(dx, dx) <= T.rc2) return true;
    vox_sub(x, T.p3, dx);
    if (vox_dot(dx, dx) <= T.rc2) return true;
    if (vox_near_edge(T.p1, T.p3, T.rc2, x) || vox_near_edge(T.p2, T.p3, T.rc2, x) || vox_near_edge(T.p3, T.p1, T.rc2, x)) return true;
    const double nx = vox_dot(T.n, x);
    if (vox_sign(nx + (T.d + T.t)) == vox_sign(nx + (T.d - T.t))) return false;
    return vox_dot(T.e1, x) + T.d1 > 0.0 && vox_dot(T.e2, x) + T.d2 > 0.0 && vox_dot(T.e3, x) + T.d3 > 0.0;
}
