// smpl_amd/csrc/body_place.h -- the robot body on a grid (include/smpl_amd.h "robot body"), the tail of field.hip behind
// world_objects.h: the voxel models of a body's links (built once, by mesh_voxelizer.h on the HalfRes lattice), the
// kernel that places them under the current link transforms, and the bookkeeping of updateVoxelsStates.  Reference:
// sbpl_collision_checking/src/robot_collision_model.cpp:959-1073 (voxelizeLink), smpl/src/geometry/voxelize.cpp:962-986
// (the gridless VoxelizeMesh), include/sbpl_collision_checking/robot_collision_state.h:473-497 (updateVoxelsState),
// src/self_collision_model.cpp:770-837 (updateVoxelsStates).  The parser, the kinematics and the dirtiness are host code
// without HIP calls: robot_body.h.
//
// k_body_place: one thread per point of all states placed by one put.  The thread finds its state by a search over the
// prefix (as k_vox_fill finds its triangle), reads the state's 12 doubles from memory (a wavefront inside one state reads
// one address), evaluates p = T v as Affine3d * Vector3d is evaluated elsewhere (row dot product a0 b0 + (a1 b1 + a2 b2),
// then the translation), applies the point rule (world_to_cell) and writes the cell, or (-1, -1, -1) -- which occ_points
// skips -- for a point outside the grid.  Each state's bounding cell range is reduced per wavefront by shuffles and
// finished with atomicMin / atomicMax on six ints; a wavefront that straddles two states lets its lanes do their own.
#pragma once

#include <cstdint>

#include "mesh_voxelizer.h"
#include "robot_body.h"

struct smplx_body {
    smplx_body_host::Body rec;
    uint64_t serial = 0;
    std::vector<int> point_first;     // models + 1: model m's points are [point_first[m], point_first[m + 1])
    std::vector<double> points;       // link-frame points of all models, back to back
    DevPtr<double> d_points;          // the same on the device
};

namespace {

struct PlaceState {
    double T[12];
    long long src;     // first point of the state's model in the points array
    long long dst;     // first cell of the list it writes
};

__global__ void __launch_bounds__(FIELD_BLOCK)
k_body_place(const PlaceState* __restrict__ states, const int* __restrict__ first, int nstates, const double* __restrict__ points,
             int* __restrict__ cells, int* __restrict__ boxes, double inv_res, double ox, double oy, double oz, int nx, int ny, int nz)
{
    const int total = first[nstates];
    const int lane = threadIdx.x & 63;
    for (int k0 = blockIdx.x * FIELD_BLOCK; k0 < total; k0 += gridDim.x * FIELD_BLOCK) {
        const int k = k0 + threadIdx.x;
        const bool live = k < total;
        int s = 0;
        int c[3] = {-1, -1, -1};
        bool in = false;
        if (live) {
            int lo = 0, hi = nstates;                  // first[lo] <= k < first[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (first[mid] <= k) lo = mid; else hi = mid;
            }
            s = lo;
            const PlaceState& S = states[s];
            const long long i = k - first[s];
            const double* v = points + 3 * (S.src + i);
            const double p[3] = {vox_dot(S.T, v) + S.T[3], vox_dot(S.T + 4, v) + S.T[7], vox_dot(S.T + 8, v) + S.T[11]};
            const double o[3] = {ox, oy, oz};
            const int n[3] = {nx, ny, nz};
            in = true;
            for (int a = 0; a < 3; ++a) {
                const double f = inv_res * (p[a] - o[a]) + 0.5;    // OccupancyGrid::worldToGrid (distance_map.hpp:520-527)
                if (!(f > -1.0e9 && f < 1.0e9)) { in = false; continue; }   // far outside: no cast of a value an int cannot hold
                c[a] = (int)f - 1;
                in = in && c[a] >= 0 && c[a] < n[a];
            }
            int* out = cells + 3 * (S.dst + i);
            out[0] = in ? c[0] : -1; out[1] = in ? c[1] : -1; out[2] = in ? c[2] : -1;
        }
        if (__ballot(live) == 0ull) continue;
        const int s0 = __shfl(s, 0);                   // lane 0 is live whenever a lane of the wavefront is
        int mn[3], mx[3];
        for (int a = 0; a < 3; ++a) { mn[a] = in ? c[a] : INT_MAX; mx[a] = in ? c[a] : INT_MIN; }
        if (__all(!live || s == s0)) {
            for (int off = 32; off > 0; off >>= 1)
                for (int a = 0; a < 3; ++a) {
                    const int lo = __shfl_xor(mn[a], off), hi = __shfl_xor(mx[a], off);
                    mn[a] = lo < mn[a] ? lo : mn[a];
                    mx[a] = hi > mx[a] ? hi : mx[a];
                }
            if (lane == 0 && mn[0] != INT_MAX)
                for (int a = 0; a < 3; ++a) { atomicMin(&boxes[6 * s0 + a], mn[a]); atomicMax(&boxes[6 * s0 + 3 + a], mx[a]); }
        } else if (in) {
            for (int a = 0; a < 3; ++a) { atomicMin(&boxes[6 * s + a], mn[a]); atomicMax(&boxes[6 * s + 3 + a], mx[a]); }
        }
    }
}

uint64_t g_body_serial = 0;

// the link's geom rows as meshes in the link frame (voxelizeCollisionElement / voxelizeGeometry,
// robot_collision_model.cpp:1005-1073), and the HalfResVoxelGrid's index range over each one's bounding box
int body_model_meshes(const smplx_body_host::Body& rec, int link, double res, std::vector<Mesh>& meshes, std::vector<int>& clip)
{
    for (const smplx_body_host::BodyGeom& g : rec.geoms) {
        if (g.link != link) continue;
        meshes.emplace_back();
        Mesh& m = meshes.back();
        if (!primitive_mesh(g.type, g.dims, m)) { m.v = g.v; m.t = g.t; }
        transform_vertices(g.origin, m);
        double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
        for (size_t i = 0; i < m.v.size(); ++i) { mn[i % 3] = std::min(mn[i % 3], m.v[i]); mx[i % 3] = std::max(mx[i % 3], m.v[i]); }
        // VoxelGrid(origin = min, size = max - min) (voxel_grid.h:187-193): discretize(min) .. discretize(min + size)
        long long cells = 1;
        for (int a = 0; a < 3; ++a) {
            const double top = mn[a] + (mx[a] - mn[a]);
            if (!(std::fabs(mn[a] / res) < 1.0e9 && std::fabs(top / res) < 1.0e9))
                return smplx_internal_set_error(SMPLX_E_LIMIT, "a voxel model's resolution is too fine for its geometry");
            const int lo = vox_half_discretize(mn[a], res), hi = vox_half_discretize(top, res);
            clip.push_back(lo);
            cells *= (long long)(hi - lo + 1);
            if (cells > SMPLX_BODY_MAX_LATTICE) return smplx_internal_set_error(SMPLX_E_LIMIT, "a geom's bounding box holds more lattice cells than SMPLX_BODY_MAX_LATTICE");
        }
        for (int a = 0; a < 3; ++a) clip.push_back(vox_half_discretize(mn[a] + (mx[a] - mn[a]), res));
    }
    return SMPLX_OK;
}

// voxelizeLink for every model: models of one resolution share a run of the voxeliser
int body_build_models(smplx_body* b)
{
    const smplx_body_host::Body& rec = b->rec;
    const int nm = (int)rec.models.size();
    std::vector<std::vector<double>> pts((size_t)nm);
    std::vector<unsigned char> done((size_t)nm, 0);
    WorkSpace work;
    for (int m0 = 0; m0 < nm; ++m0) {
        if (done[(size_t)m0]) continue;
        const double res = rec.models[(size_t)m0].res;
        std::vector<Mesh> meshes;
        std::vector<int> clip, owner;                  // owner: the model of every mesh
        for (int m = m0; m < nm; ++m) {
            if (done[(size_t)m] || rec.models[(size_t)m].res != res) continue;
            done[(size_t)m] = 1;
            const size_t before = meshes.size();
            if (int e = body_model_meshes(rec, rec.models[(size_t)m].link, res, meshes, clip)) return e;
            owner.insert(owner.end(), meshes.size() - before, m);
        }
        if (meshes.empty()) continue;
        VoxLists lists;
        const VoxLattice L{{0.5 * res, 0.5 * res, 0.5 * res}, res, true};
        if (int e = voxelize_meshes(work, L, meshes, clip, nullptr, nullptr, 0, 0, lists)) return e;
        const int total = lists.first.back();
        std::vector<int32_t> cells(3 * (size_t)total);
        if (total > 0) FIELD_TRY(hipMemcpy(cells.data(), lists.d_cells, sizeof(int32_t) * cells.size(), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < meshes.size(); ++e) {
            std::vector<double>& out = pts[(size_t)owner[e]];
            for (int i = lists.first[e]; i < lists.first[e + 1]; ++i)
                for (int a = 0; a < 3; ++a) out.push_back((double)cells[3 * (size_t)i + a] * res + 0.5 * res);   // HalfRes continuize
            if (out.size() / 3 > (size_t)SMPLX_BODY_MAX_MODEL_POINTS) return smplx_internal_set_error(SMPLX_E_LIMIT, "a voxel model has more points than SMPLX_BODY_MAX_MODEL_POINTS");
        }
    }
    b->point_first.assign((size_t)nm + 1, 0);
    for (int m = 0; m < nm; ++m) {
        b->points.insert(b->points.end(), pts[(size_t)m].begin(), pts[(size_t)m].end());
        if (b->points.size() / 3 > (size_t)SMPLX_BODY_MAX_POINTS) return smplx_internal_set_error(SMPLX_E_LIMIT, "the voxel models have more points than SMPLX_BODY_MAX_POINTS");
        b->point_first[(size_t)m + 1] = (int)(b->points.size() / 3);
    }
    if (!b->points.empty()) {
        FIELD_TRY(b->d_points.alloc(b->points.size()));
        FIELD_TRY(hipMemcpy(b->d_points, b->points.data(), sizeof(double) * b->points.size(), hipMemcpyHostToDevice));
    }
    return SMPLX_OK;
}

// the grid's record of a body: lists for the outside models, its own copy of the points
int make_grid_body(smplx_grid* g, const smplx_body* b)
{
    const int nm = (int)b->rec.models.size();
    std::unique_ptr<GridBody> gb(new GridBody);
    gb->serial = b->serial;
    gb->first.assign((size_t)nm + 1, 0);
    for (int m = 0; m < nm; ++m)
        gb->first[(size_t)m + 1] = gb->first[(size_t)m] + (b->rec.models[(size_t)m].outside ? b->point_first[(size_t)m + 1] - b->point_first[(size_t)m] : 0);
    gb->placed.assign((size_t)nm, 0);
    gb->half.assign((size_t)nm, 0);
    gb->box.assign((size_t)nm * 6, 0);
    for (int m = 0; m < nm; ++m) gb->box[6 * (size_t)m + 3] = -1;
    gb->point_first = b->point_first;
    if (gb->first.back() > 0) FIELD_TRY(gb->d_cells.alloc(3 * 2 * (size_t)gb->first.back()));
    if (!b->points.empty()) {
        FIELD_TRY(gb->d_points.alloc(b->points.size()));
        FIELD_TRY(hipMemcpy(gb->d_points, b->d_points, sizeof(double) * b->points.size(), hipMemcpyDeviceToDevice));
    }
    g->body = std::move(gb);
    return SMPLX_OK;
}

}  // namespace

extern "C" {

int smplx_body_create(const char* body_text, smplx_body** out)
{
    if (out) *out = nullptr;
    if (!body_text || !out) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    smplx_body* b = new smplx_body;
    std::string err;
    if (int e = smplx_body_host::parse_body_text(body_text, b->rec, err)) { delete b; return smplx_internal_set_error(e, err.c_str()); }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { delete b; return smplx_internal_set_error(SMPLX_E_HIP, "no HIP device: the engine has no CPU path"); }
    if (int e = body_build_models(b)) { smplx_body_destroy(b); return e; }
    b->serial = ++g_body_serial;
    *out = b;
    return SMPLX_OK;
}

void smplx_body_destroy(smplx_body* b)
{
    delete b;
}

int smplx_body_counts(const smplx_body* b, int* links, int* joints, int* models, int* outside_models, int* points)
{
    if (!b) return smplx_internal_set_error(SMPLX_E_ARG, "null body");
    int outside = 0;
    for (const smplx_body_host::BodyModel& m : b->rec.models) outside += m.outside ? 1 : 0;
    if (links) *links = (int)b->rec.links.size();
    if (joints) *joints = (int)b->rec.joints.size();
    if (models) *models = (int)b->rec.models.size();
    if (outside_models) *outside_models = outside;
    if (points) *points = (int)(b->points.size() / 3);
    return SMPLX_OK;
}

int smplx_body_set_joint(smplx_body* b, const char* joint, double q)
{
    if (!b || !joint) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    std::string err;
    if (int e = smplx_body_host::set_joint(b->rec, joint, q, err)) return smplx_internal_set_error(e, err.c_str());
    return SMPLX_OK;
}

int smplx_body_joint(const smplx_body* b, const char* joint, double* q)
{
    if (!b || !joint || !q) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    const int j = smplx_body_host::find_joint(b->rec, joint);
    if (j < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no joint named ") + joint).c_str());
    *q = b->rec.joints[(size_t)j].q;
    return SMPLX_OK;
}

int smplx_body_link_transforms(const smplx_body* b, double* T)
{
    if (!b || !T) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    smplx_body_host::link_transforms(b->rec, T);
    return SMPLX_OK;
}

int smplx_body_model_link(const smplx_body* b, int model, int* link)
{
    if (!b || !link) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    if (model < 0 || model >= (int)b->rec.models.size()) return smplx_internal_set_error(SMPLX_E_ARG, "model index outside the body");
    *link = b->rec.models[(size_t)model].link;
    return SMPLX_OK;
}

int smplx_body_model_points(const smplx_body* b, int model, double* xyz, int cap, int* n)
{
    if (n) *n = 0;
    if (!b || !n || cap < 0 || (cap > 0 && !xyz)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    if (model < 0 || model >= (int)b->rec.models.size()) return smplx_internal_set_error(SMPLX_E_ARG, "model index outside the body");
    const int at = b->point_first[(size_t)model], count = b->point_first[(size_t)model + 1] - at;
    const int take = std::min(cap, count);
    if (take > 0) std::memcpy(xyz, &b->points[3 * (size_t)at], sizeof(double) * 3 * (size_t)take);
    *n = count;
    return SMPLX_OK;
}

int smplx_body_dirty(const smplx_body* b, uint8_t* per_model)
{
    if (!b || !per_model) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    for (size_t m = 0; m < b->rec.dirty.size(); ++m) per_model[m] = b->rec.dirty[m];
    return SMPLX_OK;
}

int smplx_grid_put_body(smplx_grid* g, smplx_body* b)
{
    if (!g || !b) return smplx_internal_set_error(SMPLX_E_ARG, "null argument");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    if (g->body && g->body->serial != b->serial) return smplx_internal_set_error(SMPLX_E_STATE, "the grid already holds another body: take it first");
    const smplx_body_host::Body& rec = b->rec;
    const int nm = (int)rec.models.size();
    std::vector<int> todo;             // the dirty outside states, and those this grid has not seen yet
    for (int m = 0; m < nm; ++m)
        if (rec.models[(size_t)m].outside && (rec.dirty[(size_t)m] || !g->body || !g->body->placed[(size_t)m])) todo.push_back(m);
    if (todo.empty()) return SMPLX_OK;
    if (!g->body)
        if (int e = make_grid_body(g, b)) return e;
    GridBody* gb = g->body.get();
    const long long half_cells = gb->first.back();

    std::vector<double> T(12 * rec.links.size());
    smplx_body_host::link_transforms(rec, T.data());
    std::vector<PlaceState> states;
    std::vector<int> first(1, 0), owner;
    for (int m : todo) {
        const int count = gb->first[(size_t)m + 1] - gb->first[(size_t)m];
        if (count == 0) continue;
        PlaceState S;
        std::memcpy(S.T, &T[12 * (size_t)rec.models[(size_t)m].link], sizeof(S.T));
        S.src = gb->point_first[(size_t)m];
        S.dst = gb->first[(size_t)m] + (gb->half[(size_t)m] ? 0 : half_cells);
        states.push_back(S);
        owner.push_back(m);
        first.push_back(first.back() + count);
    }
    const int ns = (int)states.size();
    std::vector<int> boxes((size_t)ns * 6);
    for (int s = 0; s < ns; ++s)
        for (int a = 0; a < 3; ++a) { boxes[6 * (size_t)s + a] = INT_MAX; boxes[6 * (size_t)s + 3 + a] = INT_MIN; }
    Window box = empty_box();
    if (ns > 0) {
        const size_t bytes[3] = {sizeof(PlaceState) * (size_t)ns, sizeof(int) * first.size(), sizeof(int) * boxes.size()};
        size_t at[3];
        FIELD_TRY(gb->states.carve(bytes, at));
        char* const base = gb->states.base;
        FIELD_TRY(hipMemcpy(base + at[0], states.data(), bytes[0], hipMemcpyHostToDevice));
        FIELD_TRY(hipMemcpy(base + at[1], first.data(), bytes[1], hipMemcpyHostToDevice));
        FIELD_TRY(hipMemcpy(base + at[2], boxes.data(), bytes[2], hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_body_place, dim3(blocks_of((size_t)first.back())), dim3(FIELD_BLOCK), 0, 0, (const PlaceState*)(base + at[0]),
                           (const int*)(base + at[1]), ns, (const double*)gb->d_points, gb->d_cells.p, (int*)(base + at[2]), g->dev.inv_res,
                           g->dev.origin_minus_res[0], g->dev.origin_minus_res[1], g->dev.origin_minus_res[2], g->n[0], g->n[1], g->n[2]);
        // updateVoxelsStates (self_collision_model.cpp:770-837), state by state: the old list out, the new one in
        for (int s = 0; s < ns; ++s) {
            const int m = owner[(size_t)s], count = first[(size_t)s + 1] - first[(size_t)s];
            const int32_t* old_list = gb->d_cells + 3 * (gb->first[(size_t)m] + (gb->half[(size_t)m] ? half_cells : 0));
            const int32_t* new_list = gb->d_cells + 3 * states[(size_t)s].dst;
            if (gb->placed[(size_t)m]) occ_points(g, old_list, (size_t)count, 0, true);
            occ_points(g, new_list, (size_t)count, 1, true);
        }
        FIELD_TRY(hipGetLastError());
        FIELD_TRY(hipMemcpy(boxes.data(), base + at[2], bytes[2], hipMemcpyDeviceToHost));
        for (int s = 0; s < ns; ++s) {
            const int m = owner[(size_t)s];
            if (gb->placed[(size_t)m]) grow_box(box, &gb->box[6 * (size_t)m]);
            const int* nb = &boxes[6 * (size_t)s];
            const bool any = nb[0] != INT_MAX;
            for (int a = 0; a < 3; ++a) { gb->box[6 * (size_t)m + a] = any ? nb[a] : 0; gb->box[6 * (size_t)m + 3 + a] = any ? nb[3 + a] : -1; }
            grow_box(box, &gb->box[6 * (size_t)m]);
            gb->half[(size_t)m] = gb->half[(size_t)m] ? 0 : 1;
        }
    }
    for (int m : todo) { gb->placed[(size_t)m] = 1; b->rec.dirty[(size_t)m] = 0; }
    if (box.x1 < 0) return SMPLX_OK;       // no cell inside the grid, before or after
    return field_update(g, edit_window(g, box));
}

int smplx_grid_take_body(smplx_grid* g)
{
    if (!g) return smplx_internal_set_error(SMPLX_E_ARG, "null grid");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    GridBody* gb = g->body.get();
    if (!gb) return smplx_internal_set_error(SMPLX_E_STATE, "the grid holds no body");
    const long long half_cells = gb->first.back();
    Window box = empty_box();
    for (size_t m = 0; m + 1 < gb->first.size(); ++m) {
        const int count = gb->first[m + 1] - gb->first[m];
        if (!gb->placed[m] || count == 0) continue;
        occ_points(g, gb->d_cells + 3 * (gb->first[m] + (gb->half[m] ? half_cells : 0)), (size_t)count, 0, true);
        grow_box(box, &gb->box[6 * m]);
    }
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipDeviceSynchronize());
    g->body.reset();
    if (box.x1 < 0) return SMPLX_OK;
    return field_update(g, edit_window(g, box));
}

int smplx_grid_body_cells(const smplx_grid* g, int model, int32_t* cells, int cap, int* n)
{
    if (n) *n = 0;
    if (!g || !n || cap < 0 || (cap > 0 && !cells) || model < 0) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    const GridBody* gb = g->body.get();
    if (!gb) return SMPLX_OK;
    if (model + 1 >= (int)gb->first.size()) return smplx_internal_set_error(SMPLX_E_ARG, "model index outside the body");
    if (!gb->placed[(size_t)model]) return SMPLX_OK;
    const int count = gb->first[(size_t)model + 1] - gb->first[(size_t)model];
    const int take = std::min(cap, count);
    if (take > 0)
        FIELD_TRY(hipMemcpy(cells, gb->d_cells + 3 * (gb->first[(size_t)model] + (gb->half[(size_t)model] ? (long long)gb->first.back() : 0)),
                            sizeof(int32_t) * 3 * (size_t)take, hipMemcpyDeviceToHost));
    *n = count;
    return SMPLX_OK;
}

}  // extern "C"
