// smpl_amd/csrc/world_objects.h -- world objects on a grid (include/smpl_amd.h "world objects"), the tail of field.hip:
// the run that voxelises an object's shapes on the grid's lattice, the registry of named objects, and the entry points.
// Reference: sbpl_collision_checking/src/world_collision_model.cpp:193-280, src/voxel_operations.cpp:319-402.
// The kernels are elsewhere: meshes and the shapes that become meshes (shape_meshes.h) go through mesh_voxelizer.h,
// octrees through octree_voxelizer.h, the sphere rows of attached objects through object_sphere_rows.h; all of them
// share vox_common.h and the work space of device_mem.h.
#pragma once

#include "mesh_voxelizer.h"
#include "object_sphere_rows.h"
#include "octree_voxelizer.h"

namespace {

bool good_id(const char* id) { return id && *id && !std::strchr(id, '\n'); }

int find_object(const smplx_grid* g, const char* id)
{
    for (size_t i = 0; i < g->objects.size(); ++i)
        if (g->objects[i].id == id) return (int)i;
    return -1;
}

// voxelises the shapes on the grid's lattice: the pivot is the grid's origin and the candidates are clipped to the grid.
// Meshes and the shapes that become meshes go through voxelize_meshes together, every octree through octree_run; with
// both kinds in one call the lists are then laid back to back in shape order.  With edit the cells also become obstacles
// (the caller updates the field).  Waits for the device.
int voxelize_run(const smplx_grid* g, const std::vector<WorldShape>& shapes, bool edit, VoxLists& out)
{
    const size_t ns = shapes.size();
    std::vector<Mesh> meshes;
    std::vector<int> clip;
    for (size_t s = 0; s < ns; ++s) {
        if (shapes[s].type == SMPLX_SHAPE_OCTREE) continue;
        meshes.emplace_back();
        shape_mesh(shapes[s], meshes.back());
        clip.insert(clip.end(), {0, 0, 0, g->n[0] - 1, g->n[1] - 1, g->n[2] - 1});
    }
    const VoxLattice L{{g->origin[0], g->origin[1], g->origin[2]}, g->res, false};
    unsigned char* const occ = edit ? g->d_occ.p : nullptr;
    int* const counts = edit && g->ref_counted ? g->d_counts.p : nullptr;
    g_vox_kernel_ms = 0.0;
    if (meshes.size() == ns) return voxelize_meshes(g->vox, L, meshes, clip, occ, counts, g->n[1], g->n[2], out);
    if (int e = octree_limits(shapes, g->res)) return e;
    if (ns == 1) return octree_run(g, shapes[0], edit, out);      // one octree: its list is the call's
    VoxLists part;                                     // the meshes' lists, and one VoxLists per octree
    if (!meshes.empty())
        if (int e = voxelize_meshes(g->vox, L, meshes, clip, occ, counts, g->n[1], g->n[2], part)) return e;
    std::vector<VoxLists> octs(ns);
    out.first.assign(ns + 1, 0);
    out.box.assign(ns * 6, 0);
    long long total = 0;
    for (size_t s = 0, m = 0; s < ns; ++s) {
        const bool oct = shapes[s].type == SMPLX_SHAPE_OCTREE;
        if (oct)
            if (int e = octree_run(g, shapes[s], edit, octs[s])) return e;
        const VoxLists& from = oct ? octs[s] : part;
        const size_t k = oct ? 0 : m++;
        total += from.first[k + 1] - from.first[k];
        std::copy(&from.box[6 * k], &from.box[6 * k] + 6, &out.box[6 * s]);
        if (total > INT_MAX / 3) return smplx_internal_set_error(SMPLX_E_LIMIT, "too many cells in one call");
        out.first[s + 1] = (int)total;
    }
    if (total == 0) return SMPLX_OK;
    FIELD_TRY(out.d_cells.alloc(3 * (size_t)total));
    for (size_t s = 0, m = 0; s < ns; ++s) {
        const bool oct = shapes[s].type == SMPLX_SHAPE_OCTREE;
        const int32_t* from = oct ? octs[s].d_cells.p : part.d_cells + 3 * (size_t)part.first[m];
        const int n = out.first[s + 1] - out.first[s];
        if (!oct) ++m;
        if (n > 0) FIELD_TRY(hipMemcpy(out.d_cells + 3 * (size_t)out.first[s], from, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyDeviceToDevice));
    }
    return SMPLX_OK;
}

// takes the stored lists of an object out of the occupancy (removePointsFromField per shape, world_collision_model.cpp:
// 254-257) and grows `box` by the ranges they lie in; the caller updates the field
void remove_lists(smplx_grid* g, const WorldObject& o, Window& box)
{
    for (size_t s = 0; s + 1 < o.first.size(); ++s) {
        const int n = o.first[s + 1] - o.first[s];
        if (n <= 0) continue;
        occ_points(g, o.d_cells + 3 * (size_t)o.first[s], (size_t)n, 0, true);
        grow_box(box, &o.box[6 * s]);
    }
}

// insert (old < 0) or move: remove the old lists, voxelise and add the new ones, update the field once
int put_object(smplx_grid* g, const char* id, int old, std::vector<WorldShape>& shapes)
{
    if (int e = octree_limits(shapes, g->res)) return e;      // before the old lists go: a refused call changes nothing
    Window box = empty_box();
    if (old >= 0) remove_lists(g, g->objects[(size_t)old], box);
    VoxLists lists;
    const int rc = voxelize_run(g, shapes, true, lists);
    if (rc != SMPLX_OK) return rc;
    for (size_t s = 0; s + 1 < lists.first.size(); ++s)
        if (lists.first[s + 1] != lists.first[s]) grow_box(box, &lists.box[6 * s]);
    if (old < 0) { g->objects.emplace_back(); old = (int)g->objects.size() - 1; g->objects[(size_t)old].id = id; }
    WorldObject& o = g->objects[(size_t)old];
    o.d_cells = std::move(lists.d_cells);
    o.first.swap(lists.first);
    o.box.swap(lists.box);
    o.shapes.swap(shapes);
    if (box.x1 < 0) return SMPLX_OK;       // no cell inside the grid, before or after
    return field_update(g, edit_window(g, box));
}

// insert (the id is new) or move (the id is known): the checks, then put_object
int insert_or_move(smplx_grid* g, const char* id, const smplx_shape* shapes, int n, bool move)
{
    if (!g || !good_id(id)) return smplx_internal_set_error(SMPLX_E_ARG, "null grid, or an id that is empty or holds a line break");
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    const int old = find_object(g, id);
    if (!move && old >= 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("already have a world object with id ") + id).c_str());
    if (move && old < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    return put_object(g, id, old, ws);
}

}  // namespace

extern "C" {

// test hooks, not part of the ABI: time of the voxelisation launches of the last call (an octree's k_occ_points
// included), in milliseconds
void smplx_test_voxelize_timing(int on) { g_vox_timing = on != 0; }
double smplx_test_voxelize_kernel_ms(void) { return g_vox_kernel_ms; }

int smplx_world_insert_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n) { return insert_or_move(g, id, shapes, n, false); }
int smplx_world_move_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n) { return insert_or_move(g, id, shapes, n, true); }

int smplx_world_remove_object(smplx_grid* g, const char* id)
{
    if (!g || !good_id(id)) return smplx_internal_set_error(SMPLX_E_ARG, "null grid, or an id that is empty or holds a line break");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    const int at = find_object(g, id);
    if (at < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    Window box = empty_box();
    remove_lists(g, g->objects[(size_t)at], box);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipDeviceSynchronize());
    g->objects.erase(g->objects.begin() + at);
    if (box.x1 < 0) return SMPLX_OK;
    return field_update(g, edit_window(g, box));
}

int smplx_world_remove_all(smplx_grid* g)
{
    if (!g) return smplx_internal_set_error(SMPLX_E_ARG, "null grid");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    Window box = empty_box();
    for (const WorldObject& o : g->objects) remove_lists(g, o, box);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipDeviceSynchronize());
    g->objects.clear();
    if (box.x1 < 0) return SMPLX_OK;
    return field_update(g, edit_window(g, box));
}

int smplx_world_objects(const smplx_grid* g, char* names, int cap, int* n)
{
    if (n) *n = 0;
    if (!g || !n || cap < 0 || (cap > 0 && !names)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    std::string text;
    for (const WorldObject& o : g->objects) text += o.id + "\n";
    if (cap > 0) { std::strncpy(names, text.c_str(), (size_t)cap - 1); names[cap - 1] = 0; }
    *n = (int)g->objects.size();
    return SMPLX_OK;
}

int smplx_world_object_cells(const smplx_grid* g, const char* id, int shape, int32_t* cells, int cap, int* n)
{
    if (n) *n = 0;
    if (!g || !good_id(id) || !n || cap < 0 || (cap > 0 && !cells)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    const int at = find_object(g, id);
    if (at < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    const WorldObject& o = g->objects[(size_t)at];
    if (shape < 0 || shape + 1 >= (int)o.first.size()) return smplx_internal_set_error(SMPLX_E_ARG, "shape index outside the object");
    const int count = o.first[(size_t)shape + 1] - o.first[(size_t)shape];
    const int take = std::min(cap, count);
    if (take > 0) FIELD_TRY(hipMemcpy(cells, o.d_cells + 3 * (size_t)o.first[(size_t)shape], sizeof(int32_t) * 3 * (size_t)take, hipMemcpyDeviceToHost));
    *n = count;
    return SMPLX_OK;
}

int smplx_world_voxelize(const smplx_grid* g, const smplx_shape* shapes, int n, int32_t* cells, int cap, int32_t* first)
{
    if (!g || !first || cap < 0 || (cap > 0 && !cells)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    VoxLists lists;
    if (int e = voxelize_run(g, ws, false, lists)) return e;
    for (int s = 0; s <= n; ++s) first[s] = lists.first[(size_t)s];
    const int take = std::min(cap, lists.first[(size_t)n]);
    if (take > 0) FIELD_TRY(hipMemcpy(cells, lists.d_cells, sizeof(int32_t) * 3 * (size_t)take, hipMemcpyDeviceToHost));
    return SMPLX_OK;
}

// for engine.hip (smplx_attach_object / smplx_object_spheres), not part of the ABI: checks the shapes and the radius and
// makes the sphere rows of the object; work is the voxeliser work space of the calling space
int smplx_internal_object_spheres(WorkSpace* work, const smplx_shape* shapes, int n, double radius, std::vector<double>* rows, std::vector<int32_t>* first)
{
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    for (const WorldShape& w : ws)
        if (w.type == SMPLX_SHAPE_OCTREE) return smplx_internal_set_error(SMPLX_E_ARG, "octrees cannot be attached: an attached object has no octree shapes");
    if (!(radius > 0.0 && radius < 1.0e6)) return smplx_internal_set_error(SMPLX_E_ARG, "the sphere radius must be positive and finite (< 1e6)");
    return object_spheres_run(*work, ws, radius, *rows, *first);
}

}  // extern "C"
