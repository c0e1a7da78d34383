// smpl_amd/csrc/shape_meshes.h -- shapes to triangle meshes, for every voxeliser of field.hip (world objects, attached
// objects, the robot body's voxel models).  Host only: no HIP call.  Reference: smpl/src/geometry/mesh_utils.cpp:39-299
// (the indexed primitive meshes), smpl/src/geometry/voxelize.cpp:608-615 (TransformVertices), :741-756 (the sphere's 7 x 8).
// libm sin / cos as the reference: at most 112 triangles a primitive, not the hot path.
#pragma once

#include "grid_handle.h"
#include "voxelize.h"

namespace {

struct Mesh { std::vector<double> v; std::vector<int> t; };

// CreateIndexedBoxMesh (mesh_utils.cpp:39-112)
void box_mesh(double length, double width, double height, Mesh& m)
{
    const double x = 0.5 * length, y = 0.5 * width, z = 0.5 * height;
    m.v = {-x, -y, -z, x, -y, -z, -x, y, -z, x, y, -z, -x, -y, z, x, -y, z, -x, y, z, x, y, z};
    m.t = {0, 2, 1, 1, 2, 3, 5, 1, 7, 1, 3, 7, 5, 7, 4, 4, 7, 6, 4, 6, 0, 0, 6, 2, 6, 7, 2, 7, 3, 2, 5, 0, 1, 4, 5, 0};
}

// CreateIndexedSphereMesh (mesh_utils.cpp:116-204)
void sphere_mesh(double radius, int lon, int lat, Mesh& m)
{
    m.v = {0.0, 0.0, radius};
    const double theta_inc = SMPLX_PI / (lat + 1), phi_inc = (2.0 * SMPLX_PI) / lon;
    for (int ti = 0; ti < lat; ++ti)
        for (int pi = 0; pi < lon; ++pi) {
            const double theta = (ti + 1) * theta_inc, phi = pi * phi_inc;
            m.v.push_back(radius * std::sin(theta) * std::cos(phi));
            m.v.push_back(radius * std::sin(theta) * std::sin(phi));
            m.v.push_back(radius * std::cos(theta));
        }
    m.v.insert(m.v.end(), {0.0, 0.0, -radius});
    const int nv = (int)(m.v.size() / 3);
    for (int i = 0; i < lon; ++i) m.t.insert(m.t.end(), {0, i + 1, i == lon - 1 ? 1 : i + 2});
    for (int i = 0; i < lat - 1; ++i)
        for (int j = 0; j < lon; ++j) {
            const int base = i * lon + j + 1, b = base + lon;
            int br = b + 1, r = base + 1;
            if ((br - 1) / lon != (b - 1) / lon) br -= lon;
            if ((r - 1) / lon != (base - 1) / lon) r -= lon;
            m.t.insert(m.t.end(), {base, b, br, base, br, r});
        }
    for (int i = 0; i < lon; ++i) m.t.insert(m.t.end(), {nv - 1, i == 0 ? nv - 1 - lon : nv - 1 - i, nv - 1 - (i + 1)});
}

// CreateIndexedCylinderMesh (mesh_utils.cpp:208-264)
void cylinder_mesh(double radius, double length, Mesh& m)
{
    const int rim = 16;
    for (int cap = 0; cap < 2; ++cap)
        for (int i = 0; i < rim; ++i) {
            const double theta = 2.0 * SMPLX_PI * (double)i / double(rim);
            m.v.insert(m.v.end(), {radius * std::cos(theta), radius * std::sin(theta), cap == 0 ? 0.5 * length : -0.5 * length});
        }
    m.v.insert(m.v.end(), {0.0, 0.0, 0.5 * length, 0.0, 0.0, -0.5 * length});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, i + rim, (i + 1) % rim, (i + 1) % rim + rim, i + rim});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {2 * rim, (i + 1) % rim, i});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {2 * rim + 1, (i + 1) % rim + rim, i + rim});
}

// CreateIndexedConeMesh (mesh_utils.cpp:268-299)
void cone_mesh(double radius, double height, Mesh& m)
{
    const int rim = 16;
    for (int i = 0; i < rim; ++i) {
        const double theta = 2.0 * SMPLX_PI * (double)i / (double)rim;
        m.v.insert(m.v.end(), {radius * std::cos(theta), radius * std::sin(theta), -0.5 * height});
    }
    m.v.insert(m.v.end(), {0.0, 0.0, 0.5 * height, 0.0, 0.0, -0.5 * height});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, rim});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, rim + 1});
}

// the mesh of a primitive in its own frame; false (and m as it was) for a type that brings its own triangles
bool primitive_mesh(int type, const double* dims, Mesh& m)
{
    m.v.clear(); m.t.clear();
    switch (type) {
    case SMPLX_SHAPE_BOX: box_mesh(dims[0], dims[1], dims[2], m); return true;
    case SMPLX_SHAPE_SPHERE: sphere_mesh(dims[0], 7, 8, m); return true;            // voxelize.cpp:741-756
    case SMPLX_SHAPE_CYLINDER: cylinder_mesh(dims[0], dims[1], m); return true;
    case SMPLX_SHAPE_CONE: cone_mesh(dims[0], dims[1], m); return true;
    default: return false;
    }
}

// TransformVertices (voxelize.cpp:608-615): R v + t for a 3x4 row-major pose
void transform_vertices(const double* pose, Mesh& m)
{
    for (size_t i = 0; i + 2 < m.v.size(); i += 3) {
        const double v[3] = {m.v[i], m.v[i + 1], m.v[i + 2]};
        vox_transform(pose, v, &m.v[i]);
    }
}

void shape_mesh(const WorldShape& s, Mesh& m)
{
    if (!primitive_mesh(s.type, s.dims, m)) { m.v = s.vertices; m.t.assign(s.triangles.begin(), s.triangles.end()); }
    transform_vertices(s.pose, m);
}

// checks the caller's shapes and copies them (mesh arrays included)
int take_shapes(const smplx_shape* shapes, int n, std::vector<WorldShape>& out)
{
    if (!shapes || n < 1) return smplx_internal_set_error(SMPLX_E_ARG, "an object needs at least one shape");
    out.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const smplx_shape& s = shapes[i];
        WorldShape& w = out[(size_t)i];
        w.type = s.type;
        int nd = 0;
        switch (s.type) {
        case SMPLX_SHAPE_BOX: nd = 3; break;
        case SMPLX_SHAPE_SPHERE: nd = 1; break;
        case SMPLX_SHAPE_CYLINDER: case SMPLX_SHAPE_CONE: nd = 2; break;
        case SMPLX_SHAPE_MESH: case SMPLX_SHAPE_OCTREE: nd = 0; break;
        default: return smplx_internal_set_error(SMPLX_E_ARG, "unknown shape type (planes are not supported)");
        }
        for (int k = 0; k < 3; ++k) w.dims[k] = k < nd ? s.dims[k] : 0.0;
        if (!finite_coords(w.dims, 3) || !finite_coords(s.pose, 12)) return smplx_internal_set_error(SMPLX_E_ARG, "shape dimensions and pose must be finite (|x| < 1e6)");
        for (int k = 0; k < nd; ++k)
            if (!(w.dims[k] > 0.0)) return smplx_internal_set_error(SMPLX_E_ARG, "shape dimensions must be positive");
        std::memcpy(w.pose, s.pose, sizeof(w.pose));
        if (s.type == SMPLX_SHAPE_OCTREE) {
            if (!s.vertices || s.nvertices < 1 || s.triangles || s.ntriangles != 0)
                return smplx_internal_set_error(SMPLX_E_ARG, "an octree needs leaves (vertices: rows of cx cy cz size) and takes no triangles");
            if (!finite_coords(s.vertices, (size_t)s.nvertices * 4)) return smplx_internal_set_error(SMPLX_E_ARG, "octree leaves must be finite (|x| < 1e6)");
            for (size_t k = 0; k < (size_t)s.nvertices; ++k)
                if (!(s.vertices[4 * k + 3] > 0.0)) return smplx_internal_set_error(SMPLX_E_ARG, "the size of an octree leaf must be positive");
            w.vertices.assign(s.vertices, s.vertices + (size_t)s.nvertices * 4);
            continue;
        }
        if (s.type != SMPLX_SHAPE_MESH) continue;
        if (!s.vertices || !s.triangles || s.nvertices < 1 || s.ntriangles < 1) return smplx_internal_set_error(SMPLX_E_ARG, "a mesh needs vertices and triangles");
        if (!finite_coords(s.vertices, (size_t)s.nvertices * 3)) return smplx_internal_set_error(SMPLX_E_ARG, "mesh vertices must be finite (|x| < 1e6)");
        for (size_t k = 0; k < (size_t)s.ntriangles * 3; ++k)
            if (s.triangles[k] < 0 || s.triangles[k] >= s.nvertices) return smplx_internal_set_error(SMPLX_E_ARG, "triangle index outside the vertices");
        w.vertices.assign(s.vertices, s.vertices + (size_t)s.nvertices * 3);
        w.triangles.assign(s.triangles, s.triangles + (size_t)s.ntriangles * 3);
    }
    return SMPLX_OK;
}

}  // namespace
