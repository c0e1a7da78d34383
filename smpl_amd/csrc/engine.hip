// smpl_amd/csrc/engine.hip -- host side of the C-ABI (include/smpl_amd.h): the one translation unit of the host engine.
// It holds lifetime -- grids, models and spaces are created and destroyed here -- with the model accessors, the space's
// plain getters and its status; every other entry point is in the header of its concern, included below in dependency
// order.  The records behind the handles are in space.h, the owners of what they hold on the device in device_mem.h.
// There is no CPU fallback: every query runs the gfx950 kernels and fails with SMPLX_E_HIP when no GPU is present.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/smpl_amd.h"
#include "det_math.h"
#include "heuristics.h"
#include "device_types.h"
#include "kernels.h"
#include "model_compile.h"
#include "specialize.h"
#include "test_hooks.h"
// the host engine, in dependency order
#include "host_core.h"
#include "grid_handle.h"
#include "lattice.h"
#include "space.h"
#include "bfs_host.h"
#include "device_table.h"
#include "step.h"
#include "search_host.h"
#include "lazy.h"
#include "ara_search.h"
#include "multi_query.h"
#include "path_tools.h"
#include "path_multi.h"
// the entry points, by concern
#include "queries.h"
#include "attached_host.h"
#include "heuristic_host.h"
#include "goals.h"
#include "expand_entry.h"
#include "plan_entry.h"

namespace {

// host mirror of the applyMotionPrimitive branch (manip_lattice_action_space.cpp:575-621) of successor_values in lattice_steps.h,
// the one device definition: change the two together.  Same expressions, same order, -ffp-contract=off like the kernels.
void host_apply_prim(const SmplxActionsDev& A, const double* parent, int pi, int nv, double* out)
{
    double d0 = A.delta[pi][0], d1 = nv > 1 ? A.delta[pi][1] : 0.0;
    if (A.xy_rotate_by_var3 && nv > 3) {
        double sn, cs;
        smplx_sincos(parent[3], &sn, &cs);
        const double a0 = d0, a1 = d1;
        d0 = cs * a0 + (-sn) * a1;
        d1 = sn * a0 + cs * a1;
    }
    for (int v = 0; v < nv; ++v) {
        const double d = v == 0 ? d0 : (v == 1 ? d1 : A.delta[pi][v]);
        out[v] = d + parent[v];
    }
}

}  // namespace

extern "C" {

const char* smplx_last_error(void) { return g_error.c_str(); }

int smplx_shard_range(int rank, int world, int total, int per_rank, int* first, int* count)
{
    if (!first || !count || world <= 0 || rank < 0 || rank >= world || total < 0 || per_rank <= 0) return set_error(SMPLX_E_ARG, "bad shard arguments");
    const long long f = (long long)rank * per_rank;
    *first = (int)std::min<long long>(f, total);
    *count = (int)std::max<long long>(0, std::min<long long>(f + per_rank, total) - *first);
    return SMPLX_OK;
}

int smplx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int smplx_grid_create(const double origin[3], int nx, int ny, int nz, double res, double max_dist, const int32_t* d2,
                      smplx_grid** out)
{
    if (!origin || !d2 || !out || nx <= 0 || ny <= 0 || nz <= 0 || !(res > 0.0)) return set_error(SMPLX_E_ARG, "bad grid arguments");
    smplx_grid* g = new smplx_grid;
    const double inv_res = 1.0 / res;
    g->dmax_int = (int)std::ceil(max_dist * inv_res);   // distance_map.hpp:126
    g->dmax_sqrd = g->dmax_int * g->dmax_int;
    if (g->dmax_sqrd > 65535) { delete g; return set_error(SMPLX_E_LIMIT, "max_dist/res exceeds 255 cells (16-bit squared distances)"); }
    g->res = res; g->max_dist = max_dist;
    g->n[0] = nx; g->n[1] = ny; g->n[2] = nz;
    const int bx = (nx + 3) / 4, by = (ny + 3) / 4, bz = (nz + 3) / 4;
    std::vector<uint16_t> tiled((size_t)bx * by * bz * 64, 0);
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z) {
                const int v = d2[((size_t)x * ny + y) * nz + z];
                if (v < 0 || v > g->dmax_sqrd) { delete g; return set_error(SMPLX_E_ARG, "squared distance outside [0, dmax^2]"); }
                const size_t brick = ((size_t)(x >> 2) * by + (y >> 2)) * bz + (z >> 2);
                tiled[brick * 64 + ((x & 3) << 4) + ((y & 3) << 2) + (z & 3)] = (uint16_t)v;
            }
    hipError_t e = g->d_d2.alloc(tiled.size());
    if (e == hipSuccess) e = hipMemcpy(g->d_d2, tiled.data(), tiled.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { delete g; return set_error(SMPLX_E_HIP, std::string("grid upload: ") + hipGetErrorString(e)); }
    for (int a = 0; a < 3; ++a) { g->origin[a] = origin[a]; g->dev.origin_minus_res[a] = origin[a] - res; g->dev.n[a] = g->n[a]; }
    g->dev.res = res; g->dev.inv_res = inv_res;
    g->dev.bricks[0] = bx; g->dev.bricks[1] = by; g->dev.bricks[2] = bz;
    g->dev.dmax_sqrd = g->dmax_sqrd; g->dev.pad = 0;
    g->dev.d2 = g->d_d2;
    *out = g;
    return SMPLX_OK;
}

void smplx_grid_destroy(smplx_grid* g)
{
    if (!g) return;
    delete g;      // every device array is owned by a member (grid_handle.h)
}

// error text for the other translation units of the library (field.hip)
int smplx_internal_set_error(int code, const char* msg) { return set_error(code, msg ? msg : ""); }

int smplx_model_create(const char* robot_text, smplx_model** out)
{
    if (!robot_text || !out) return set_error(SMPLX_E_ARG, "null argument");
    smplx_model* m = new smplx_model;
    if (!smplx::compile_robot_text(robot_text, m->hm)) {
        const std::string err = m->hm.error;
        delete m;
        return set_error(err.find("too many") != std::string::npos ? SMPLX_E_LIMIT : SMPLX_E_PARSE, err);
    }
    *out = m;
    return SMPLX_OK;
}

void smplx_model_destroy(smplx_model* m) { delete m; }

int smplx_model_counts(const smplx_model* m, int* njoints, int* nvars, int* ntrees, int* nnodes, int* npairs, int* nslots)
{
    if (!m) return set_error(SMPLX_E_ARG, "null model");
    const SmplxModelDev& d = m->hm.dev;
    if (njoints) *njoints = d.njoints;
    if (nvars) *nvars = d.nvars;
    if (ntrees) *ntrees = d.ntrees;
    if (nnodes) *nnodes = d.nnodes;
    if (npairs) *npairs = d.npairs;
    if (nslots) *nslots = d.nslots;
    return SMPLX_OK;
}

int smplx_model_joints(const smplx_model* m, double* origins, double* k, int* file_index)
{
    if (!m) return set_error(SMPLX_E_ARG, "null model");
    const SmplxModelDev& d = m->hm.dev;
    for (int j = 0; j < d.njoints; ++j) {
        if (origins) std::memcpy(origins + 12 * (size_t)j, d.joints[j].origin, sizeof(double) * 12);
        if (k) k[j] = m->hm.joint_k[j];
        if (file_index) file_index[j] = m->hm.file_joint_index[j];
    }
    return SMPLX_OK;
}

int smplx_model_nodes(const smplx_model* m, double* xyzr, int* left, int* right, int* tree_first)
{
    if (!m) return set_error(SMPLX_E_ARG, "null model");
    const SmplxModelDev& d = m->hm.dev;
    for (int i = 0; i < d.nnodes; ++i) {
        if (xyzr) { xyzr[4 * i] = d.nodes[i].c[0]; xyzr[4 * i + 1] = d.nodes[i].c[1]; xyzr[4 * i + 2] = d.nodes[i].c[2]; xyzr[4 * i + 3] = d.nodes[i].r; }
        if (left) left[i] = d.nodes[i].left;
        if (right) right[i] = d.nodes[i].right;
    }
    if (tree_first) for (int t = 0; t <= d.ntrees; ++t) tree_first[t] = d.tree_first[t];
    return SMPLX_OK;
}

int smplx_model_pairs(const smplx_model* m, int* pairs)
{
    if (!m || !pairs) return set_error(SMPLX_E_ARG, "null argument");
    const SmplxModelDev& d = m->hm.dev;
    for (int i = 0; i < d.npairs; ++i) { pairs[2 * i] = d.pair_a[i]; pairs[2 * i + 1] = d.pair_b[i]; }
    return SMPLX_OK;
}

int smplx_model_const_header(const smplx_model* m, char* out, int cap)
{
    if (!m) return set_error(SMPLX_E_ARG, "null argument");
    const std::string h = smplx::model_const_header(m->hm.dev);
    if (out && cap > 0) { std::strncpy(out, h.c_str(), cap - 1); out[cap - 1] = 0; }
    return (int)h.size() + 1;
}

int smplx_space_create(const smplx_model* model, const smplx_grid* grid, const char* mprim_text, const smplx_params* params,
                       smplx_space** out)
{
    if (!model || !grid || !mprim_text || !params || !out) return set_error(SMPLX_E_ARG, "null argument");
    if (params->heuristic != SMPLX_H_BFS && params->heuristic != SMPLX_H_EUCLID && params->heuristic != SMPLX_H_JOINT_DIST)
        return set_error(SMPLX_E_ARG, "smplx_params.heuristic: SMPLX_H_BFS, SMPLX_H_EUCLID or SMPLX_H_JOINT_DIST");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_error(SMPLX_E_HIP, "no HIP device: the engine has no CPU path");
    // one way out on failure: the space is destroyed (stream waited for, then every member frees what it owns)
    std::unique_ptr<smplx_space, void (*)(smplx_space*)> owner(new smplx_space, smplx_space_destroy);
    smplx_space* s = owner.get();
    s->model = model->hm;
    s->grid = grid;
    s->params = *params;
    s->step.fused_mode = (params->flags & SMPLX_SPACE_FUSED) != 0;
    if (params->flags & SMPLX_SPACE_NO_SMALL_KERNEL) s->small.batch_max = 0;
    if (const char* e = getenv("SMPLX_AUTO_SPECULATE")) s->spec.auto_spec = std::max(0, atoi(e));
    if (const char* e = getenv("SMPLX_LAZY_RIDERS")) s->lazy.riders = std::max(0, atoi(e));
    if (const char* e = getenv("SMPLX_TRUE_COST_PARENTS")) s->lazy.ride_parents = std::max(0, atoi(e));
    s->N = s->model.dev.nvars;
    if (!smplx::load_mprim_text(mprim_text, params->resolutions, s->N, s->actions)) return set_error(SMPLX_E_PARSE, "mprim: " + s->actions.error);
    s->M = s->actions.dev.nprims;
    SmplxActionsDev& A = s->actions.dev;
    A.use_long_and_short = params->use_long_and_short;
    A.xy_rotate_by_var3 = params->xy_rotate_by_var3;
    // defaults of ManipLatticeActionSpace::init (manip_lattice_action_space.cpp:75-84), then the caller's overrides
    for (int i = 0; i < 4; ++i) { A.enabled[i] = 0; A.thresh[i] = 0.4; }
    A.enabled[SMPLX_MP_SHORT] = params->use_short_dist_mprims;
    A.thresh[SMPLX_MP_SHORT] = params->short_dist_mprims_thresh;
    A.enabled[SMPLX_MP_SNAP_XYZ_RPY] = params->use_xyzrpy_snap_mprim;
    A.thresh[SMPLX_MP_SNAP_XYZ_RPY] = params->xyzrpy_snap_dist_thresh;
    smplx::fill_discretization(s->model.dev, params->resolutions);
    for (int i = 0; i < s->model.dev.nnodes; ++i)
        s->model.dev.nodes[i].thr = smplx::sphere_threshold(s->model.dev.nodes[i].r, params->padding, grid->res, grid->dmax_sqrd);
    s->bfs.wall_thr = smplx::wall_threshold(params->bfs_inflation_radius, grid->res, grid->dmax_sqrd);
    std::memset(&s->hs, 0, sizeof(s->hs));
    s->hs.model = s->model.dev;
    s->blob_bytes = smplx::pack_model_blob(s->model.dev, s->hs.model_blob, sizeof(s->hs.model_blob));
    if (s->blob_bytes == 0) return set_error(SMPLX_E_LIMIT, "model does not fit the packed LDS image");
    s->hs.grid = grid->dev;
    s->hs.actions = A;
    s->hs.goal.type = SMPLX_GOAL_JOINT;

    if (int e = hip_status(hipGetDevice(&s->device), "hipGetDevice")) return e;
    if (int e = hip_status(s->stream.create(), "hipStreamCreate")) return e;
    {
        const char* env = getenv("SMPLX_SPECIALIZE");
        smplx::generic_kernels(s->ks);
        if (params->flags & SMPLX_SPACE_GENERIC_KERNELS) s->specialize_note = "disabled by SMPLX_SPACE_GENERIC_KERNELS";
        else if (env && env[0] == '0') s->specialize_note = "disabled by SMPLX_SPECIALIZE=0";
        else if (!smplx::specialized_kernels(s->model.dev, closed_form(s), s->ks, s->specialize_note) && env && env[0] == '2') {
            // SMPLX_SPECIALIZE=2: the per-robot build is required
            return set_error(SMPLX_E_HIP, "kernel specialisation failed: " + s->specialize_note);
        }
    }
    s->lds_nroot = s->ks.specialized ? 0 : s->model.dev.nroot;
    s->lds_bytes = smplx_lds_bytes(s->blob_bytes, s->lds_nroot, s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->lds_bytes_valid = smplx_lds_bytes(s->blob_bytes, s->lds_nroot, s->ks.specialized ? 0 : s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->lds_bytes_clearance = smplx_clearance_lds_bytes(s->blob_bytes, s->model.dev.ntrees, s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->step.one_launch_lds = smplx_lds_bytes_n(s->blob_bytes, s->lds_nroot, s->ks.specialized ? 0 : s->model.dev.nslots, s->model.dev.nvars,
                                               s->model.dev.stack_bytes, SMPLX_STEP_BLOCK);
    s->step.one_launch_blocks = step_block_resident(s, s->step.one_launch_lds, &s->step.one_launch_per_cu);
    if (s->lds_bytes > 160 * 1024) return set_error(SMPLX_E_LIMIT, "model needs more LDS per block than a CU has (160 KB)");
    if (int e = hip_status(s->batch.done.create(hipEventDisableTiming), "hipEventCreate")) return e;
    if (int e = hip_status(s->d_space.alloc(1), "hipMalloc space")) return e;
    const int dx = grid->n[0] + 2, dy = grid->n[1] + 2, dz = grid->n[2] + 2;
    for (int a = 0; a < 3; ++a) s->bfs.bricks[a] = (grid->n[a] + 7) / 8;
    const size_t nbricks = (size_t)s->bfs.bricks[0] * s->bfs.bricks[1] * s->bfs.bricks[2];
    s->hs.heur.kind = params->heuristic;
    for (int k = 0; k < 4; ++k) s->hs.heur.w[k] = 1.0;          // euclid_dist_heuristic.h:77-80
    for (int k = 0; k < 9; ++k) s->hs.heur.rot[k] = s->goal.rot[k];
    if (closed_form(s)) {
        // no BFS: no distance records, no brick lists, no wall sync (bfs.total stays 0, hs.bfs all zero); the kernels find
        // the heuristic record of this space's device image through hs.bfs.heur (device_types.h SmplxBfsDev)
        s->hs.bfs.heur = reinterpret_cast<const SmplxHeurDev*>(reinterpret_cast<const unsigned char*>(s->d_space.p) + offsetof(SmplxSpaceDev, heur));
    } else {
        s->bfs.total = (int64_t)dx * dy * dz;
        s->bfs.ints = (int64_t)nbricks * SMPLX_BFS_REC;
        if (int e = hip_status(s->bfs.d_dist.alloc(s->bfs.ints), "hipMalloc bfs")) return e;
        if (int e = hip_status(s->bfs.d_brick_queued.alloc(2 * nbricks + 16), "hipMalloc bfs queued")) return e;
        if (int e = hip_status(hipMemset(s->bfs.d_brick_queued, 0, sizeof(int32_t) * 2 * nbricks + 64), "hipMemset bfs queued")) return e;
        if (int e = hip_status(s->bfs.d_queue.alloc(2 * 16 * nbricks + 64), "hipMalloc bfs queue")) return e;
        if (int e = hip_status(s->bfs.d_counts.alloc(3 * 16 * 32 + kBfsHistory), "hipMalloc bfs counts")) return e;
        s->hs.bfs.dim_x = dx; s->hs.bfs.dim_y = dy; s->hs.bfs.dim_z = dz; s->hs.bfs.dim_xy = dx * dy;
        s->hs.bfs.cost_per_cell = params->cost_per_cell;
        s->hs.bfs.nbx = s->bfs.bricks[0]; s->hs.bfs.nby = s->bfs.bricks[1]; s->hs.bfs.nbz = s->bfs.bricks[2];
        s->hs.bfs.dist = s->bfs.d_dist;
        s->hs.bfs.tag_mask = (int64_t)grid->n[0] * grid->n[1] * grid->n[2] < ((int64_t)1 << 28) ? (int32_t)0xF0000000u : 0;
        s->hs.bfs.tag_word = 0;
        // BfsHeuristic::syncGridAndBfs (bfs_heuristic.cpp:331-353), once, at init
        hipLaunchKernelGGL(k_bfs_init, dim3(2048), dim3(256), 0, s->stream, grid->dev, s->bfs.wall_thr, s->bfs.bricks[0], s->bfs.bricks[1], s->bfs.bricks[2], s->bfs.d_dist);
        if (int e = hip_status(hipGetLastError(), "k_bfs_init")) return e;
    }
    {
        // Device copy of the state table (K5).  The K5 entry points and smplx_table_sync create it on first use.  The
        // planner's own batches use it only with SMPLX_DEVICE_TABLE=1: measured on MI355X (cfg 2 / cfg 4, bench.py) the
        // ids it hands back save the host ~0.5 us per expansion, but the lookups and the rides of the inserts add more
        // than that to the latency of every batch (single query 79k -> 70k states/s, 128-query shard 1.26M -> 1.03M).
        const char* env = getenv("SMPLX_DEVICE_TABLE");
        if (env && env[0] == '1' && table_alloc(s, (size_t)1 << 18) != SMPLX_OK) return SMPLX_E_HIP;
    }
    if (upload_space(s) != SMPLX_OK) return SMPLX_E_HIP;
    reset_lattice(s);
    *out = owner.release();
    return SMPLX_OK;
}

void smplx_space_destroy(smplx_space* s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);   // nothing is freed before the stream has drained
    delete s;   // every buffer, event and the stream is owned by a member (space.h)
}

int smplx_space_specialized(const smplx_space* s, char* note, int cap)
{
    if (!s) return 0;
    if (note && cap > 0) { std::strncpy(note, s->specialize_note.c_str(), cap - 1); note[cap - 1] = 0; }
    return s->ks.specialized ? 1 : 0;
}

int smplx_test_const_header(const smplx_model* m, int closed_form, char* out, int cap)
{
    if (!m) return set_error(SMPLX_E_ARG, "null argument");
    const std::string h = smplx::model_const_header(m->hm.dev) + (closed_form ? smplx::kClosedFormDefine : "");
    if (out && cap > 0) { std::strncpy(out, h.c_str(), cap - 1); out[cap - 1] = 0; }
    return (int)h.size() + 1;
}

int smplx_space_num_vars(const smplx_space* s) { return s ? s->N : 0; }
int smplx_space_heuristic(const smplx_space* s) { return s ? s->params.heuristic : SMPLX_E_ARG; }
int smplx_space_num_prims(const smplx_space* s) { return s ? s->M : 0; }

int smplx_space_discretization(const smplx_space* s, int32_t* coord_vals, double* coord_deltas)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    for (int v = 0; v < s->N; ++v) {
        if (coord_vals) coord_vals[v] = s->model.dev.coord_vals[v];
        if (coord_deltas) coord_deltas[v] = s->model.dev.coord_delta[v];
    }
    return SMPLX_OK;
}

int smplx_space_status(const smplx_space* s, char* msg, int cap)
{
    if (!s) return SMPLX_E_ARG;
    if (msg && cap > 0) { std::strncpy(msg, s->status_msg.c_str(), cap - 1); msg[cap - 1] = 0; }
    return s->status;
}

void smplx_space_clear_status(smplx_space* s)
{
    if (!s) return;
    s->status = SMPLX_OK;
    s->status_msg.clear();
}

int smplx_extract_path(smplx_space* s, const int32_t* ids, int len, double* q)
{
    if (!s || !ids || !q) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = pull_lattice(s)) return e;
    // manip_lattice.cpp:2018-2155: every id maps to its stored state; a trailing goal id (0) maps to the
    // cheapest goal-satisfying successor of its predecessor
    for (int i = 0; i < len; ++i) {
        int id = ids[i];
        if (id == 0) {
            if (i == 0) return set_error(SMPLX_E_STATE, "path cannot start at the goal id");
            const int prev = ids[i - 1];
            if (prev > 0 && prev < (int)s->lat.cache_off.size() && s->lat.cache_off[prev] < 0 && s->lat.done_off[prev] >= 0 &&
                s->lat.done_prim.size() == s->lat.done_succ.size()) {
                // expanded by the device-resident search: the committed list names the primitive of every successor; the
                // first goal successor in primitive order is the cheapest (every edge costs 1000 here, manip_lattice.cpp:
                // 1388-1412) and its joint values are recomputed with the device's arithmetic
                int prim = -1;
                for (int k = 0; k < s->lat.done_cnt[prev] && prim < 0; ++k)
                    if (s->lat.done_succ[s->lat.done_off[prev] + k] == 0) prim = s->lat.done_prim[s->lat.done_off[prev] + k];
                if (prim < 0) return set_error(SMPLX_E_STATE, "no goal successor found during path extraction");
                const SmplxActionsDev& A = s->actions.dev;
                if (A.type[prim] == SMPLX_MP_LONG || A.type[prim] == SMPLX_MP_SHORT)
                    host_apply_prim(A, &s->lat.qs[(size_t)prev * s->N], prim, s->N, q + (size_t)i * s->N);
                else
                    std::memcpy(q + (size_t)i * s->N, s->hs.goal.angles, sizeof(double) * s->N);   // snap to a joint goal (:551-559)
                continue;
            }
            if (prev <= 0 || prev >= (int)s->lat.cache_off.size() || s->lat.cache_off[prev] < 0)
                return set_error(SMPLX_E_STATE, "goal predecessor was never expanded");
            int best = -1, best_cost = std::numeric_limits<int>::max();
            for (int k = 0; k < s->lat.cache_cnt[prev]; ++k) {
                const Lattice::Rec& r = s->lat.recs[s->lat.cache_off[prev] + k];
                if (!r.goal) continue;
                const int edge_cost = 1000;   // 3-argument cost() (manip_lattice.cpp:1388-1412)
                if (edge_cost < best_cost) { best_cost = edge_cost; best = k; }
            }
            if (best < 0) return set_error(SMPLX_E_STATE, "no goal successor found during path extraction");
            std::memcpy(q + (size_t)i * s->N, &s->lat.rec_q[(size_t)(s->lat.cache_off[prev] + best) * s->N], sizeof(double) * s->N);
            continue;
        }
        if (id < 0 || id >= (int)s->lat.h_of_id.size()) return set_error(SMPLX_E_STATE, "unknown state id in path");
        std::memcpy(q + (size_t)i * s->N, &s->lat.qs[(size_t)id * s->N], sizeof(double) * s->N);
    }
    return SMPLX_OK;
}

}  // extern "C"
