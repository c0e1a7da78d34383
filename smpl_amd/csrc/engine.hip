// smpl_amd/csrc/engine.hip -- host side of the C-ABI (include/smpl_amd.h): the entry points, which check their
// arguments and call into the headers below.  The records behind the handles are in space.h, the ManipLattice state
// table in lattice.h, the kernel launches and frontier batches in step.h, the lazy successor pair in lazy.h, the two
// ARA* callers in ara_search.h and search_host.h.  There is no CPU fallback: every query below runs the gfx950 kernels and fails with SMPLX_E_HIP when
// no GPU is present.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
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

namespace {

// host mirror of ManipLattice::stateToCoord (manip_lattice.cpp:1263-1289) on det_math
void state_to_coord(const SmplxModelDev& m, const double* q, int32_t* c)
{
    for (int v = 0; v < m.nvars; ++v) {
        const double delta = m.coord_delta[v];
        if (m.var_type[v] == SMPLX_JT_CONTINUOUS) {
            const double pos = smplx_normalize_angle_positive(q[v]);
            int k = (int)((pos + delta * 0.5) / delta);
            if (k == m.coord_vals[v]) k = 0;
            c[v] = k;
        } else {
            c[v] = (int)(((q[v] - m.var_min[v]) / delta) + 0.5);
        }
    }
}

// KDLRobotModel::checkJointLimits (kdl_robot_model.cpp:173-189, 210-235)
bool host_check_limits(const SmplxModelDev& m, const double* q)
{
    for (int v = 0; v < m.nvars; ++v) {
        double a = q[v];
        if (std::fabs(a) > SMPLX_2PI) a = std::fmod(a, SMPLX_2PI);
        while (a > m.var_min_norm[v]) a -= SMPLX_2PI;
        while (a < m.var_min[v]) a += SMPLX_2PI;
        if (a < m.var_min[v] || a > m.var_max[v]) return false;
    }
    return true;
}

static_assert(SMPLX_HEUR_BFS == SMPLX_H_BFS && SMPLX_HEUR_EUCLID == SMPLX_H_EUCLID && SMPLX_HEUR_JOINT_DIST == SMPLX_H_JOINT_DIST,
              "the device's heuristic kinds are the public ones");

// does the space plan with one of the closed forms of heuristics.h (no BFS: bfs_host.h is never entered for it)
bool closed_form(const smplx_space* s) { return s->params.heuristic != SMPLX_H_BFS; }

int run_heuristic(smplx_space* s, const double* q, int n, int32_t* h, double* xyz)
{
    const int N = s->N;
    if (int e = s->batch.b_q.reserve((size_t)n * N)) return e;
    if (int e = s->b_h.reserve(n)) return e;
    if (int e = s->b_xyz.reserve((size_t)n * 3)) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * N, hipMemcpyHostToDevice, s->stream));
    if (closed_form(s))
        KLAUNCH(s, K_HEURISTIC_CLOSED, k_heuristic_closed, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->blob_bytes, s->stream, s->d_space,
                s->batch.b_q.p, n, s->b_h.p, s->b_xyz.p);
    else
        KLAUNCH(s, K_HEURISTIC, k_heuristic, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->blob_bytes, s->stream, s->d_space, s->batch.b_q.p, n,
                       s->b_h.p, s->b_xyz.p);
    HIP_TRY(hipGetLastError());
    if (h) HIP_TRY(hipMemcpyAsync(h, s->b_h.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    if (xyz) HIP_TRY(hipMemcpyAsync(xyz, s->b_xyz.p, sizeof(double) * n * 3, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

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

// =================================================================================================
// C-ABI
// =================================================================================================

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
// ... and field.hip owns the voxeliser: the sphere rows of an object attached by shape (object_sphere_rows.h)
int smplx_internal_object_spheres(WorkSpace* work, const smplx_shape* shapes, int n, double radius, std::vector<double>* rows,
                                  std::vector<int32_t>* first);

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
    smplx_space* s = new smplx_space;
    s->model = model->hm;
    s->grid = grid;
    s->params = *params;
    s->step.fused_mode = (params->flags & SMPLX_SPACE_FUSED) != 0;
    if (params->flags & SMPLX_SPACE_NO_SMALL_KERNEL) s->small.batch_max = 0;
    if (const char* e = getenv("SMPLX_AUTO_SPECULATE")) s->spec.auto_spec = std::max(0, atoi(e));
    if (const char* e = getenv("SMPLX_LAZY_RIDERS")) s->lazy.riders = std::max(0, atoi(e));
    if (const char* e = getenv("SMPLX_TRUE_COST_PARENTS")) s->lazy.ride_parents = std::max(0, atoi(e));
    s->N = s->model.dev.nvars;
    if (!smplx::load_mprim_text(mprim_text, params->resolutions, s->N, s->actions)) {
        const std::string err = s->actions.error;
        delete s;
        return set_error(SMPLX_E_PARSE, "mprim: " + err);
    }
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
    if (s->blob_bytes == 0) { delete s; return set_error(SMPLX_E_LIMIT, "model does not fit the packed LDS image"); }
    s->hs.grid = grid->dev;
    s->hs.actions = A;
    s->hs.goal.type = SMPLX_GOAL_JOINT;

    auto bail = [&](hipError_t e, const char* what) {
        const std::string msg = std::string(what) + ": " + hipGetErrorString(e);
        smplx_space_destroy(s);
        return set_error(SMPLX_E_HIP, msg);
    };
    hipError_t e;
    if ((e = hipGetDevice(&s->device)) != hipSuccess) return bail(e, "hipGetDevice");
    if ((e = hipStreamCreate(&s->stream)) != hipSuccess) return bail(e, "hipStreamCreate");
    {
        const char* env = getenv("SMPLX_SPECIALIZE");
        smplx::generic_kernels(s->ks);
        if (params->flags & SMPLX_SPACE_GENERIC_KERNELS) s->specialize_note = "disabled by SMPLX_SPACE_GENERIC_KERNELS";
        else if (env && env[0] == '0') s->specialize_note = "disabled by SMPLX_SPECIALIZE=0";
        else if (!smplx::specialized_kernels(s->model.dev, closed_form(s), s->ks, s->specialize_note) && env && env[0] == '2') {
            // SMPLX_SPECIALIZE=2: the per-robot build is required
            const std::string msg = "kernel specialisation failed: " + s->specialize_note;
            smplx_space_destroy(s);
            return set_error(SMPLX_E_HIP, msg);
        }
    }
    s->lds_nroot = s->ks.specialized ? 0 : s->model.dev.nroot;
    s->lds_bytes = smplx_lds_bytes(s->blob_bytes, s->lds_nroot, s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->lds_bytes_valid = smplx_lds_bytes(s->blob_bytes, s->lds_nroot, s->ks.specialized ? 0 : s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->lds_bytes_clearance = smplx_clearance_lds_bytes(s->blob_bytes, s->model.dev.ntrees, s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes);
    s->step.one_launch_lds = smplx_lds_bytes_n(s->blob_bytes, s->lds_nroot, s->ks.specialized ? 0 : s->model.dev.nslots, s->model.dev.nvars,
                                               s->model.dev.stack_bytes, SMPLX_STEP_BLOCK);
    s->step.one_launch_blocks = step_block_resident(s, s->step.one_launch_lds, &s->step.one_launch_per_cu);
    if (s->lds_bytes > 160 * 1024) { smplx_space_destroy(s); return set_error(SMPLX_E_LIMIT, "model needs more LDS per block than a CU has (160 KB)"); }
    if ((e = hipEventCreateWithFlags(&s->batch.done, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipMalloc((void**)&s->d_space, sizeof(SmplxSpaceDev))) != hipSuccess) return bail(e, "hipMalloc space");
    const int dx = grid->n[0] + 2, dy = grid->n[1] + 2, dz = grid->n[2] + 2;
    for (int a = 0; a < 3; ++a) s->bfs.bricks[a] = (grid->n[a] + 7) / 8;
    const size_t nbricks = (size_t)s->bfs.bricks[0] * s->bfs.bricks[1] * s->bfs.bricks[2];
    s->hs.heur.kind = params->heuristic;
    for (int k = 0; k < 4; ++k) s->hs.heur.w[k] = 1.0;          // euclid_dist_heuristic.h:77-80
    for (int k = 0; k < 9; ++k) s->hs.heur.rot[k] = s->goal_rot[k];
    if (closed_form(s)) {
        // no BFS: no distance records, no brick lists, no wall sync (bfs.total stays 0, hs.bfs all zero); the kernels find
        // the heuristic record of this space's device image through hs.bfs.heur (device_types.h SmplxBfsDev)
        s->hs.bfs.heur = reinterpret_cast<const SmplxHeurDev*>(reinterpret_cast<const unsigned char*>(s->d_space) + offsetof(SmplxSpaceDev, heur));
    } else {
        s->bfs.total = (int64_t)dx * dy * dz;
        s->bfs.ints = (int64_t)nbricks * SMPLX_BFS_REC;
        if ((e = hipMalloc((void**)&s->bfs.d_dist, sizeof(int32_t) * s->bfs.ints)) != hipSuccess) return bail(e, "hipMalloc bfs");
        if ((e = hipMalloc((void**)&s->bfs.d_brick_queued, sizeof(int32_t) * 2 * nbricks + 64)) != hipSuccess) return bail(e, "hipMalloc bfs queued");
        if ((e = hipMemset(s->bfs.d_brick_queued, 0, sizeof(int32_t) * 2 * nbricks + 64)) != hipSuccess) return bail(e, "hipMemset bfs queued");
        if ((e = hipMalloc((void**)&s->bfs.d_queue, sizeof(int32_t) * (2 * 16 * nbricks + 64))) != hipSuccess) return bail(e, "hipMalloc bfs queue");
        if ((e = hipMalloc((void**)&s->bfs.d_counts, sizeof(int32_t) * (3 * 16 * 32 + kBfsHistory))) != hipSuccess) return bail(e, "hipMalloc bfs counts");
        s->hs.bfs.dim_x = dx; s->hs.bfs.dim_y = dy; s->hs.bfs.dim_z = dz; s->hs.bfs.dim_xy = dx * dy;
        s->hs.bfs.cost_per_cell = params->cost_per_cell;
        s->hs.bfs.nbx = s->bfs.bricks[0]; s->hs.bfs.nby = s->bfs.bricks[1]; s->hs.bfs.nbz = s->bfs.bricks[2];
        s->hs.bfs.dist = s->bfs.d_dist;
        s->hs.bfs.tag_mask = (int64_t)grid->n[0] * grid->n[1] * grid->n[2] < ((int64_t)1 << 28) ? (int32_t)0xF0000000u : 0;
        s->hs.bfs.tag_word = 0;
        // BfsHeuristic::syncGridAndBfs (bfs_heuristic.cpp:331-353), once, at init
        hipLaunchKernelGGL(k_bfs_init, dim3(2048), dim3(256), 0, s->stream, grid->dev, s->bfs.wall_thr, s->bfs.bricks[0], s->bfs.bricks[1], s->bfs.bricks[2], s->bfs.d_dist);
        if ((e = hipGetLastError()) != hipSuccess) return bail(e, "k_bfs_init");
    }
    {
        // Device copy of the state table (K5).  The K5 entry points and smplx_table_sync create it on first use.  The
        // planner's own batches use it only with SMPLX_DEVICE_TABLE=1: measured on MI355X (cfg 2 / cfg 4, bench.py) the
        // ids it hands back save the host ~0.5 us per expansion, but the lookups and the rides of the inserts add more
        // than that to the latency of every batch (single query 79k -> 70k states/s, 128-query shard 1.26M -> 1.03M).
        const char* env = getenv("SMPLX_DEVICE_TABLE");
        if (env && env[0] == '1' && table_alloc(s, (size_t)1 << 18) != SMPLX_OK) {
            const std::string m = g_error; smplx_space_destroy(s); return set_error(SMPLX_E_HIP, m);
        }
    }
    if (upload_space(s) != SMPLX_OK) { const std::string m = g_error; smplx_space_destroy(s); return set_error(SMPLX_E_HIP, m); }
    reset_lattice(s);
    *out = s;
    return SMPLX_OK;
}

void smplx_space_destroy(smplx_space* s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (hipEvent_t e : s->step.prof_events) (void)hipEventDestroy(e);
    if (s->batch.done) (void)hipEventDestroy(s->batch.done);
    if (s->d_space) (void)hipFree(s->d_space);
    if (s->bfs.d_dist) (void)hipFree(s->bfs.d_dist);
    if (s->bfs.d_queue) (void)hipFree(s->bfs.d_queue);
    if (s->bfs.d_counts) (void)hipFree(s->bfs.d_counts);
    if (s->bfs.d_brick_queued) (void)hipFree(s->bfs.d_brick_queued);
    if (s->dt.d_table) (void)hipFree(s->dt.d_table);
    if (s->att.d_bodies) (void)hipFree(s->att.d_bodies);
    for (StepLaunch::WorkCounters& w : s->step.work_counters) (void)hipFree(w.p);
    (void)search_free(s);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int smplx_space_specialized(const smplx_space* s, char* note, int cap)
{
    if (!s) return 0;
    if (note && cap > 0) { std::strncpy(note, s->specialize_note.c_str(), cap - 1); note[cap - 1] = 0; }
    return s->ks.specialized ? 1 : 0;
}

int smplx_test_set_work_list_items(smplx_space* s, int items)
{
    if (!s || items < 0) return set_error(SMPLX_E_ARG, "bad argument");
    s->step.work_list_items = items / 8 * 8;
    return SMPLX_OK;
}

int smplx_test_set_pipe_prep(smplx_space* s, int on)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    s->step.pipe_prep = on != 0;
    return SMPLX_OK;
}

int smplx_test_set_one_launch(smplx_space* s, int mode)
{
    if (!s || mode < -1 || mode > 1) return set_error(SMPLX_E_ARG, "bad argument");
    s->step.one_launch = mode;
    return SMPLX_OK;
}

long long smplx_test_one_launch_steps(const smplx_space* s) { return s ? (long long)s->step.one_launch_steps : -1; }

int smplx_test_step_counters_zero(smplx_space* s, void* stream)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    for (StepLaunch::WorkCounters& w : s->step.work_counters) {
        if (w.stream != (hipStream_t)stream) continue;
        std::vector<int32_t> h(SMPLX_WORK_COUNTER_BYTES / sizeof(int32_t));
        HIP_TRY(hipStreamSynchronize(w.stream));
        HIP_TRY(hipMemcpy(h.data(), w.p, SMPLX_WORK_COUNTER_BYTES, hipMemcpyDeviceToHost));
        for (int32_t v : h) if (v != 0) return 0;
        return 1;
    }
    return set_error(SMPLX_E_ARG, "no step has run on this stream");
}

int smplx_test_set_table_slots(smplx_space* s, int slots)
{
    if (!s || slots < 0 || (slots != 0 && (slots < 64 || (slots & (slots - 1)) != 0)))
        return set_error(SMPLX_E_ARG, "slots must be 0 or a power of two of at least 64");
    s->dt.test_slots = (size_t)slots;
    return SMPLX_OK;
}

long long smplx_test_table_slots(const smplx_space* s) { return s ? (long long)(s->dt.d_table ? s->dt.cap : 0) : -1; }

int smplx_test_set_search_helper(smplx_space* s, int on)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    s->ds.test_no_helper = on == 0;
    return SMPLX_OK;
}

int smplx_test_set_search_capacity(smplx_space* s, int states)
{
    if (!s || states < 0) return set_error(SMPLX_E_ARG, "bad argument");
    s->ds.test_capacity = states;
    return SMPLX_OK;
}

int smplx_test_acos(const double* x, int n, double* out)
{
    if (!x || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    for (int i = 0; i < n; ++i) out[i] = smplx_acos(x[i]);
    return SMPLX_OK;
}

int smplx_test_goal_rotation(const smplx_space* s, double R[9])
{
    if (!s || !R) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "goal not set");
    for (int k = 0; k < 9; ++k) R[k] = s->goal_rot[k];
    return SMPLX_OK;
}

int smplx_test_const_header(const smplx_model* m, int closed_form, char* out, int cap)
{
    if (!m) return set_error(SMPLX_E_ARG, "null argument");
    const std::string h = smplx::model_const_header(m->hm.dev) + (closed_form ? smplx::kClosedFormDefine : "");
    if (out && cap > 0) { std::strncpy(out, h.c_str(), cap - 1); out[cap - 1] = 0; }
    return (int)h.size() + 1;
}

int smplx_search_counters(const smplx_space* s, int64_t out[16])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 16; ++k) out[k] = 0;
    const DevSearch& D = s->ds;
    out[0] = D.searches; out[1] = D.grows; out[2] = D.dup_pushes;
    for (int k = 0; k < 7; ++k) out[3 + k] = D.ticks[k];
    out[10] = D.h.nstates;
    out[11] = search_heap_cache_entries(s, nullptr);
    out[12] = D.ticks[7] >> 32;            // evaluation rounds opened on a guess of the next pop
    out[13] = D.ticks[7] & 0xFFFFFFFFll;   // ... that the pop confirmed
    out[14] = D.table_allocs;              // empty state tables the search allocated and filled from the states' coordinates
    out[15] = s->dt.regrows;               // times the host loop's device table was outgrown and built again
    return SMPLX_OK;
}

int smplx_test_heap_ops(const int32_t* ops, int nops, int lds_entries, int32_t* top_after)
{
    if (!ops || !top_after || nops <= 0 || lds_entries < 1 || lds_entries > 4096) return set_error(SMPLX_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_error(SMPLX_E_HIP, "no HIP device");
    DevBuf<int32_t> d_ops, d_top;
    DevBuf<unsigned long long> d_heap;
    DevBuf<SmplxSState> d_st;
    int e;
    if ((e = d_ops.reserve(2 * (size_t)nops))) return e;
    if ((e = d_top.reserve((size_t)nops))) return e;
    if ((e = d_heap.reserve((size_t)nops + 2))) return e;
    if ((e = d_st.reserve((size_t)nops + 1))) return e;
    HIP_TRY(hipMemcpy(d_ops.p, ops, sizeof(int32_t) * 2 * (size_t)nops, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_st.p, 0, sizeof(SmplxSState) * ((size_t)nops + 1)));
    hipLaunchKernelGGL(k_heap_ops, dim3(1), dim3(64), (size_t)lds_entries * 8, 0, d_ops.p, nops, lds_entries, d_heap.p, d_st.p, d_top.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(top_after, d_top.p, sizeof(int32_t) * (size_t)nops, hipMemcpyDeviceToHost));
    return SMPLX_OK;
}

int smplx_test_table_probe(int nvars, int slots, int one_home, const int32_t* inserted, int n_inserted, const int32_t* queries, int n_queries,
                           int32_t* found_at_insert, int32_t* ids)
{
    if (!inserted || !queries || !found_at_insert || !ids || nvars < 1 || nvars > SMPLX_MAX_VARS || slots < 2 || slots > 4096 ||
        (slots & (slots - 1)) != 0 || n_inserted < 1 || n_inserted >= slots || n_queries < 1 || n_queries > 65536)
        return set_error(SMPLX_E_ARG, "bad argument (slots: a power of two up to 4096 with room for an empty slot)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_error(SMPLX_E_HIP, "no HIP device");
    const int stride = smplx_table_stride(nvars);
    DevBuf<int32_t> d_table, d_in, d_out;
    int e;
    const size_t n_max = (size_t)std::max(n_inserted, n_queries);
    if ((e = d_table.reserve((size_t)slots * stride))) return e;
    if ((e = d_in.reserve(n_max * nvars))) return e;
    if ((e = d_out.reserve(n_max))) return e;
    HIP_TRY(hipMemset(d_table.p, 0, sizeof(int32_t) * (size_t)slots * stride));
    SmplxTableDev T;
    T.slots = d_table.p; T.mask = (uint32_t)(slots - 1); T.stride = stride; T.pad = 0;
    for (int pass = 0; pass < 2; ++pass) {     // the inserts, then the lookups in a launch of their own
        const int32_t* src = pass == 0 ? inserted : queries;
        const int n = pass == 0 ? n_inserted : n_queries;
        HIP_TRY(hipMemcpy(d_in.p, src, sizeof(int32_t) * (size_t)n * nvars, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_table_probe_ops, dim3(1), dim3(64), 0, 0, T, (const int*)d_in.p, n, nvars, one_home ? 1 : 0, pass == 0 ? 1 : 0, d_out.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(pass == 0 ? found_at_insert : ids, d_out.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return SMPLX_OK;
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

int smplx_check_joint_limits(const smplx_space* s, const double* q, int n, uint8_t* ok)
{
    if (!s || !q || !ok || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    for (int i = 0; i < n; ++i) ok[i] = host_check_limits(s->model.dev, q + (size_t)i * s->N) ? 1 : 0;
    return SMPLX_OK;
}

int smplx_cc_state_valid_batch(smplx_space* s, const double* q, int n, uint8_t* valid, int32_t* lookups)
{
    if (!s || !q || !valid || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    int e;
    if ((e = s->batch.b_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_flags.reserve(n))) return e;
    if ((e = s->batch.b_lookups.reserve(n))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_STATE_VALID, k_state_valid, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_valid, s->stream, s->d_space,
                       s->batch.b_q.p, n, s->b_flags.p, s->batch.b_lookups.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(valid, s->b_flags.p, n, hipMemcpyDeviceToHost, s->stream));
    if (lookups) HIP_TRY(hipMemcpyAsync(lookups, s->batch.b_lookups.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int smplx_cc_state_valid_batch_device(smplx_space* s, const double* d_q, int n, uint8_t* d_valid, int32_t* d_lookups, void* stream)
{
    if (!s || !d_q || !d_valid || n <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    KLAUNCH(s, K_STATE_VALID, k_state_valid, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_valid, (hipStream_t)stream,
            s->d_space, d_q, n, d_valid, d_lookups);
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

int smplx_cc_edge_valid_batch(smplx_space* s, const double* a, const double* b, int n, uint8_t* valid, int32_t* lookups,
                              int32_t* waypoints)
{
    if (!s || !a || !b || !valid || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(a, (size_t)n * s->N) || !sane_values(b, (size_t)n * s->N))
        return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    int e;
    if ((e = s->batch.b_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_q2.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_flags.reserve(n))) return e;
    if ((e = s->batch.b_lookups.reserve(n))) return e;
    if ((e = s->b_way.reserve(n))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, a, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->b_q2.p, b, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_EDGE_VALID, k_edge_valid, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_valid, s->stream, s->d_space,
                       s->batch.b_q.p, s->b_q2.p, n, s->b_flags.p, s->batch.b_lookups.p, s->b_way.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(valid, s->b_flags.p, n, hipMemcpyDeviceToHost, s->stream));
    if (lookups) HIP_TRY(hipMemcpyAsync(lookups, s->batch.b_lookups.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    if (waypoints) HIP_TRY(hipMemcpyAsync(waypoints, s->b_way.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int smplx_cc_interpolate(smplx_space* s, const double* a, const double* b, double* out, int cap, int* n)
{
    if (!s || !a || !b || !n) return set_error(SMPLX_E_ARG, "bad argument");
    if (!sane_values(a, s->N) || !sane_values(b, s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    // waypoint count and interpolation are host arithmetic on det_math (collision_space.cpp:583-640,
    // robot_motion_collision_model.h:297-320); no grid or sphere data is involved
    const SmplxModelDev& M = s->model.dev;
    double motion = 0.0;
    for (int v = 0; v < M.nvars; ++v) {
        if (M.var_type[v] == SMPLX_JT_CONTINUOUS) motion += M.var_k[v] * std::fabs(smplx_shortest_angle_diff(b[v], a[v]));
        else if (M.var_type[v] == SMPLX_JT_REVOLUTE) motion += M.var_k[v] * std::fabs(b[v] - a[v]);
        else if (M.var_type[v] == SMPLX_JT_PRISMATIC) motion += std::fabs(b[v] - a[v]);
    }
    int W = 0;
    if (motion != 0.0) W = std::max(2, (int)std::ceil(motion / 0.05) + 1);
    *n = W;
    if (!out) return SMPLX_OK;
    const double inv = W > 0 ? 1.0 / (double)(W - 1) : 0.0;
    for (int w = 0; w < W && w < cap; ++w) {
        const double alpha = (double)w * inv;
        for (int v = 0; v < M.nvars; ++v) {
            const double d = M.var_type[v] == SMPLX_JT_CONTINUOUS ? smplx_shortest_angle_diff(b[v], a[v]) : b[v] - a[v];
            out[(size_t)w * M.nvars + v] = a[v] + alpha * d;
        }
    }
    return SMPLX_OK;
}

int smplx_cc_sphere_positions(smplx_space* s, const double* q, int n, double* out)
{
    if (!s || !q || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    int e;
    const size_t cnt = (size_t)n * s->model.dev.nnodes * 3;
    if ((e = s->batch.b_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_sq.reserve(cnt))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_SPHERE_POSITIONS, k_sphere_positions, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes, s->stream,
                       s->d_space, s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->b_sq.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// ---- clearance: distance to collision (include/smpl_amd.h; kernels: clearance_kernels.h) -------------------------------

namespace {

const char* const kClearanceLds = "the clearance kernels need more LDS per block than a CU has (160 KB) for this model";

// n rows of results from the space's clearance scratch to the caller's arrays, on the space's stream
int clearance_results(smplx_space* s, int n, double* clearance, double* parts, int32_t* witness)
{
    HIP_TRY(hipMemcpyAsync(clearance, s->b_clr_out.p, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    if (parts) HIP_TRY(hipMemcpyAsync(parts, s->b_clr_out.p + n, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, s->stream));
    if (witness) HIP_TRY(hipMemcpyAsync(witness, s->b_clr_wit.p, sizeof(int32_t) * 4 * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

}  // namespace

int smplx_cc_state_clearance_batch(smplx_space* s, const double* q, int n, double* clearance, double* parts, int32_t* witness)
{
    if (!s || !q || !clearance || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (s->lds_bytes_clearance > 160 * 1024) return set_error(SMPLX_E_LIMIT, kClearanceLds);
    int e;
    if ((e = s->b_clr_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_clr_out.reserve((size_t)n * 3))) return e;
    if ((e = s->b_clr_wit.reserve((size_t)n * 4))) return e;
    HIP_TRY(hipMemcpyAsync(s->b_clr_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_STATE_CLEARANCE, k_state_clearance, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_clearance, s->stream,
            s->d_space, s->b_clr_q.p, n, s->params.padding, s->b_clr_out.p, s->b_clr_out.p + n, s->b_clr_wit.p);
    HIP_TRY(hipGetLastError());
    return clearance_results(s, n, clearance, parts, witness);
}

int smplx_cc_state_clearance_batch_device(smplx_space* s, const double* d_q, int n, double* d_clearance, double* d_parts,
                                          int32_t* d_witness, void* stream)
{
    if (!s || !d_q || !d_clearance || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (s->lds_bytes_clearance > 160 * 1024) return set_error(SMPLX_E_LIMIT, kClearanceLds);
    KLAUNCH(s, K_STATE_CLEARANCE, k_state_clearance, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_clearance,
            (hipStream_t)stream, s->d_space, d_q, n, s->params.padding, d_clearance, d_parts, d_witness);
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

int smplx_cc_edge_clearance_batch(smplx_space* s, const double* a, const double* b, int n, double* clearance, double* parts,
                                  int32_t* witness)
{
    if (!s || !a || !b || !clearance || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(a, (size_t)n * s->N) || !sane_values(b, (size_t)n * s->N))
        return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (s->lds_bytes_clearance > 160 * 1024) return set_error(SMPLX_E_LIMIT, kClearanceLds);
    int e;
    if ((e = s->b_clr_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_clr_q2.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_clr_out.reserve((size_t)n * 3))) return e;
    if ((e = s->b_clr_wit.reserve((size_t)n * 4))) return e;
    HIP_TRY(hipMemcpyAsync(s->b_clr_q.p, a, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->b_clr_q2.p, b, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_EDGE_CLEARANCE, k_edge_clearance, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_clearance, s->stream,
            s->d_space, s->b_clr_q.p, s->b_clr_q2.p, n, s->params.padding, s->b_clr_out.p, s->b_clr_out.p + n, s->b_clr_wit.p);
    HIP_TRY(hipGetLastError());
    return clearance_results(s, n, clearance, parts, witness);
}

// ---- attached bodies -------------------------------------------------------------------------------------------------


namespace {

// the device image of the space's bodies (device_types.h SmplxBodiesDev): trees in pre-order, thresholds bound to the
// space's grid and padding, allowed masks resolved by name.  Rebuilt whole at every attach and detach (the reference
// rebuilds its pair lists only when the group or the ACM changes, self_collision_model.cpp:1311).
int upload_bodies(smplx_space* s)
{
    std::unique_ptr<SmplxBodiesDev> img(new SmplxBodiesDev);
    std::memset(img.get(), 0, sizeof(SmplxBodiesDev));
    const SmplxModelDev& D = s->model.dev;
    // ancestors: the transform flow of the chain pass (running / root / saved slot), joint by joint
    uint64_t slot_anc[SMPLX_MAX_SLOTS] = {};
    for (int j = 0; j < D.njoints; ++j) {
        const SmplxJoint& J = D.joints[j];
        const uint64_t base = J.src == SMPLX_SRC_ROOT ? 0ull : (J.src == SMPLX_SRC_RUNNING ? img->ancestors[j - 1] : slot_anc[J.src]);
        img->ancestors[j] = base | (1ull << j);
        if (J.save_slot >= 0) slot_anc[J.save_slot] = img->ancestors[j];
    }
    int nn = 0;
    for (size_t b = 0; b < s->att.bodies.size(); ++b) {
        AttachedBodies::Body& B = s->att.bodies[b];
        std::vector<SmplxNode> post;
        smplx::build_sphere_tree(B.xyzr.data(), (int)(B.xyzr.size() / 4), post);
        B.first = nn;
        // post-order (root last, local indices) -> pre-order with the end of each subtree in `pad`
        std::function<void(int)> emit = [&](int k) {
            const int at = nn++;
            SmplxNode n = post[k];
            n.thr = smplx::sphere_threshold(n.r, s->params.padding, s->grid->res, s->grid->dmax_sqrd);
            const int l = n.left, r = n.right;
            img->nodes[at] = n;
            if (l >= 0) {
                img->nodes[at].left = at + 1;
                emit(l);
                img->nodes[at].right = nn;
                emit(r);
            }
            img->nodes[at].pad = nn;
        };
        emit((int)post.size() - 1);
        B.count = nn - B.first;
        SmplxBodyDev& o = img->body[b];
        o.joint = B.joint;
        o.root = B.first;
        o.end = nn;
        for (const std::string& a : B.allowed) {
            for (int t = 0; t < D.ntrees; ++t)
                if (s->model.child_links[D.tree_joint[t]] == a) o.allow_trees |= 1u << t;
            for (size_t c = 0; c < s->att.bodies.size(); ++c)
                if (c != b && s->att.bodies[c].id == a) { o.allow_bodies |= 1u << c; img->body[c].allow_bodies |= 1u << b; }
        }
    }
    img->n = (int)s->att.bodies.size();
    img->nnodes = nn;
    if (!s->att.d_bodies) HIP_TRY(hipMalloc((void**)&s->att.d_bodies, sizeof(SmplxBodiesDev)));
    // kernels in flight may still read the old image, on the space's stream or on a caller's (the _device entry points)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyAsync(s->att.d_bodies, img.get(), sizeof(SmplxBodiesDev), hipMemcpyHostToDevice, s->stream));
    s->hs.bodies = s->att.bodies.empty() ? nullptr : s->att.d_bodies;
    HIP_TRY(hipMemcpyAsync((unsigned char*)s->d_space + offsetof(SmplxSpaceDev, bodies), &s->hs.bodies, sizeof(s->hs.bodies),
                           hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

}  // namespace

namespace {

// the checks every attach starts with, in the order of the reference's attachBody: the id, then the link.  Fills B.id,
// B.link and B.joint.
int attach_target(smplx_space* s, const char* id, const char* link, AttachedBodies::Body& B)
{
    const std::string sid(id);
    if (sid.empty() || sid.size() > 255 || sid.find_first_of(" \t\r\n") != std::string::npos)
        return set_error(SMPLX_E_ARG, "a body id is 1 to 255 characters without white space");
    for (const AttachedBodies::Body& b : s->att.bodies)
        if (b.id == sid) return set_error(SMPLX_E_ARG, "a body with id " + sid + " is attached already");
    B.id = sid;
    B.link = link;
    const smplx::HostModel& hm = s->model;
    if (B.link == hm.root_link) B.joint = -1;
    else {
        B.joint = -2;
        for (size_t j = 0; j < hm.child_links.size(); ++j) if (hm.child_links[j] == B.link) B.joint = (int)j;
        if (B.joint == -2) return set_error(SMPLX_E_ARG, "unknown link " + B.link);
    }
    // the reference never checks a body on a link outside the group (attached_bodies_collision_model.cpp:124-135): refused
    if (std::find(hm.group_links.begin(), hm.group_links.end(), B.link) == hm.group_links.end())
        return set_error(SMPLX_E_ARG, "link " + B.link + " is outside the collision group: a body there would never be checked");
    return SMPLX_OK;
}

int attach_allowed(const char* const* allowed, int nallowed, AttachedBodies::Body& B)
{
    for (int i = 0; i < nallowed; ++i) {
        if (!allowed[i]) return set_error(SMPLX_E_ARG, "null name in the allowed list");
        B.allowed.emplace_back(allowed[i]);
    }
    return SMPLX_OK;
}

// the limits, then the body joins the space: n rows {x, y, z, r} in the link's frame.  `made` ends the text of a refusal
// (what made the rows, for an object attached by shape).
int attach_rows(smplx_space* s, AttachedBodies::Body& B, const double* rows, int n, const std::string& made)
{
    if ((int)s->att.bodies.size() >= SMPLX_MAX_BODIES) return set_error(SMPLX_E_LIMIT, "more than SMPLX_MAX_BODIES (8) attached bodies" + made);
    int used = 0;
    for (const AttachedBodies::Body& b : s->att.bodies) used += b.count;
    if ((long long)used + 2ll * n - 1 > SMPLX_MAX_BODY_NODES)
        return set_error(SMPLX_E_LIMIT, "the attached bodies need more than SMPLX_MAX_BODY_NODES (1024) tree nodes" + made);
    B.xyzr.assign(rows, rows + 4 * (size_t)n);
    s->att.bodies.push_back(std::move(B));
    if (int e = upload_bodies(s)) { const std::string m = g_error; s->att.bodies.pop_back(); (void)upload_bodies(s); return set_error(e, m); }
    ++s->att.epoch;
    return SMPLX_OK;
}

}  // namespace

int smplx_attach_body(smplx_space* s, const char* id, const char* link, const double* spheres, int n, const char* const* allowed,
                      int nallowed)
{
    if (!s || !id || !link || !spheres || n <= 0 || nallowed < 0 || (nallowed > 0 && !allowed))
        return set_error(SMPLX_E_ARG, "bad argument");
    AttachedBodies::Body B;
    if (int e = attach_target(s, id, link, B)) return e;
    for (int i = 0; i < 4 * n; ++i)
        if (!std::isfinite(spheres[i]) || std::fabs(spheres[i]) >= 1e6 || (i % 4 == 3 && spheres[i] < 0.0))
            return set_error(SMPLX_E_ARG, "spheres: finite x y z r with |value| < 1e6 and r >= 0");
    if (int e = attach_allowed(allowed, nallowed, B)) return e;
    return attach_rows(s, B, spheres, n, "");
}

int smplx_attach_object(smplx_space* s, const char* id, const char* link, const smplx_shape* shapes, int n, double radius,
                        const char* const* allowed, int nallowed)
{
    if (!s || !id || !link || !shapes || n <= 0 || nallowed < 0 || (nallowed > 0 && !allowed))
        return set_error(SMPLX_E_ARG, "bad argument");
    AttachedBodies::Body B;
    if (int e = attach_target(s, id, link, B)) return e;
    if (int e = attach_allowed(allowed, nallowed, B)) return e;
    std::vector<double> rows;
    std::vector<int32_t> first;
    if (int e = smplx_internal_object_spheres(&s->att.vox, shapes, n, radius, &rows, &first)) return e;
    const int made = (int)(rows.size() / 4);
    // the reference would attach an empty model that is never checked
    if (made == 0) return set_error(SMPLX_E_ARG, "the shapes make no sphere: every triangle is degenerate");
    return attach_rows(s, B, rows.data(), made, ": the shapes made " + std::to_string(made) + " spheres of radius " + std::to_string(radius));
}

int smplx_object_spheres(smplx_space* s, const smplx_shape* shapes, int n, double radius, double* xyzr, int cap, int32_t* first)
{
    if (!s || !shapes || n <= 0 || !first || cap < 0 || (cap > 0 && !xyzr)) return set_error(SMPLX_E_ARG, "bad argument");
    std::vector<double> rows;
    std::vector<int32_t> f;
    if (int e = smplx_internal_object_spheres(&s->att.vox, shapes, n, radius, &rows, &f)) return e;
    for (int k = 0; k <= n; ++k) first[k] = f[(size_t)k];
    const int take = std::min(cap, f[(size_t)n]);
    if (take > 0) std::memcpy(xyzr, rows.data(), sizeof(double) * 4 * (size_t)take);
    return SMPLX_OK;
}

int smplx_detach_body(smplx_space* s, const char* id)
{
    if (!s || !id) return set_error(SMPLX_E_ARG, "bad argument");
    for (size_t b = 0; b < s->att.bodies.size(); ++b) {
        if (s->att.bodies[b].id != id) continue;
        AttachedBodies::Body keep = s->att.bodies[b];
        s->att.bodies.erase(s->att.bodies.begin() + b);
        if (int e = upload_bodies(s)) {
            const std::string m = g_error;
            s->att.bodies.insert(s->att.bodies.begin() + b, std::move(keep));
            (void)upload_bodies(s);
            return set_error(e, m);
        }
        ++s->att.epoch;
        return SMPLX_OK;
    }
    return set_error(SMPLX_E_ARG, std::string("no attached body with id ") + id);
}

int smplx_attached_bodies(const smplx_space* s, char* names, int cap, int32_t* first_node, int32_t* nnodes)
{
    if (!s || cap < 0 || (cap > 0 && !names)) return set_error(SMPLX_E_ARG, "bad argument");
    std::string text;
    for (size_t b = 0; b < s->att.bodies.size(); ++b) {
        text += s->att.bodies[b].id + " " + s->att.bodies[b].link + "\n";
        if (first_node) first_node[b] = s->att.bodies[b].first;
        if (nnodes) nnodes[b] = s->att.bodies[b].count;
    }
    if (cap > 0) { std::strncpy(names, text.c_str(), cap - 1); names[cap - 1] = 0; }
    return (int)s->att.bodies.size();
}

int smplx_attached_nodes(const smplx_space* s, double* xyzr, int32_t* left, int32_t* right)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    int nn = 0;
    for (const AttachedBodies::Body& b : s->att.bodies) nn += b.count;
    if ((xyzr || left || right) && nn > 0) {
        std::vector<SmplxNode> nodes((size_t)nn);
        HIP_TRY(hipMemcpy(nodes.data(), s->att.d_bodies->nodes, sizeof(SmplxNode) * nn, hipMemcpyDeviceToHost));
        for (int i = 0; i < nn; ++i) {
            if (xyzr) for (int k = 0; k < 3; ++k) xyzr[4 * i + k] = nodes[i].c[k];
            if (xyzr) xyzr[4 * i + 3] = nodes[i].r;
            if (left) left[i] = nodes[i].left;
            if (right) right[i] = nodes[i].right;
        }
    }
    return nn;
}

int smplx_cc_attached_positions(smplx_space* s, const double* q, int n, double* out)
{
    if (!s || !q || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    int nn = 0;
    for (const AttachedBodies::Body& b : s->att.bodies) nn += b.count;
    if (n == 0 || nn == 0) return SMPLX_OK;
    int e;
    const size_t cnt = (size_t)n * nn * 3;
    if ((e = s->batch.b_q.reserve((size_t)n * s->N))) return e;
    if ((e = s->b_sq.reserve(cnt))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_ATTACHED_POSITIONS, k_attached_positions, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes, s->stream,
            s->d_space, s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->b_sq.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// A goal is set in three steps, shared by the single-goal entry points (finish_goal) and the multi-goal ones
// (finish_goals_multi): begin_goal -- the goal position into the device record, the tag of this goal's BFS run, the
// upload; the BFS (run_bfs / run_bfs_multi); end_goal -- the goal stands, the query starts over.
static int begin_goal(smplx_space* s)
{
    for (int a = 0; a < 3; ++a) s->hs.goal.xyz[a] = s->goal_xyz[a];
    if (closed_form(s)) {
        // what the closed form needs of the goal (device_types.h SmplxHeurDev); there is no BFS run to tag
        SmplxHeurDev& H = s->hs.heur;
        H.joint_goal = s->hs.goal.type == SMPLX_GOAL_JOINT ? 1 : 0;
        for (int a = 0; a < 3; ++a) H.xyz[a] = s->goal_xyz[a];
        for (int k = 0; k < 9; ++k) H.rot[k] = s->goal_rot[k];
        for (int v = 0; v < SMPLX_MAX_VARS; ++v) H.angles[v] = H.joint_goal && v < s->N ? s->hs.goal.angles[v] : 0.0;
        return upload_space(s);
    }
    // the tag of this goal's BFS run (device_types.h SmplxBfsDev): 1..7, a reset of the records when they wrap
    if (s->hs.bfs.tag_mask != 0) {
        s->bfs.reset_due = s->bfs.tag == 7;
        s->bfs.tag = s->bfs.tag % 7 + 1;
        s->hs.bfs.tag_word = s->bfs.tag << 28;
    } else {
        s->bfs.reset_due = s->bfs.tag != 0;
        s->bfs.tag = 1;
        s->hs.bfs.tag_word = 0;
    }
    return upload_space(s);
}

static void end_goal(smplx_space* s)
{
    s->goal_set = true;
    s->grid_epoch = s->grid->epoch;
    s->att.epoch_goal = s->att.epoch;
    // a new goal starts a new query: the state table restarts (ids are per query)
    reset_lattice(s);
    // heuristic of the goal id = BFS cost at the goal pose's cell (manip_lattice.cpp:1176-1190); the closed forms give the
    // goal id 0 outright (euclid_dist_heuristic.cpp:120-122, joint_dist_heuristic.cpp:72-74)
    int c[3];
    s->lat.h_of_id[0] = closed_form(s) || bfs_goal_cell(s, s->goal_xyz, c) ? 0 : 32767;   // the seeded cell has distance 0 (bfs3d.cpp:178)
}

static int finish_goal(smplx_space* s)
{
    if (int e = begin_goal(s)) return e;
    if (!closed_form(s))
        if (int e = run_bfs(s, s->goal_xyz)) return e;
    end_goal(s);
    return SMPLX_OK;
}

// the goal record of a joint goal, all but the goal pose (planner_interface.cpp:1232-1235 takes it from the FK)
static void joint_goal_record(smplx_space* s, const double* angles, const double* tolerances)
{
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_JOINT;
    for (int v = 0; v < s->N; ++v) { G.angles[v] = angles[v]; G.angle_tol[v] = tolerances[v]; }
    state_to_coord(s->model.dev, angles, G.coord);
}

static void xyz_goal_record(smplx_space* s, const double xyz[3], const double tol[3])
{
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_XYZ;
    for (int a = 0; a < 3; ++a) { s->goal_xyz[a] = xyz[a]; G.xyz_tol[a] = tol[a]; }
    // the Euclidean heuristic's goal rotation: the identity, what the reference makes of the pose {x, y, z, 0, 0, 0}
    for (int k = 0; k < 9; ++k) s->goal_rot[k] = k % 4 == 0 ? 1.0 : 0.0;
}

// the bound of the device's orientation test (device_types.h SmplxGoalDev::rpy_c4): theta < tol, theta in [0, pi], is
// 4 cos^2(theta / 2) > 4 cos^2(tol / 2) for 0 < tol <= pi; a wider tolerance admits every orientation, tol <= 0 none
static double rpy_bound(double tol)
{
    if (!(tol > 0.0)) return std::numeric_limits<double>::infinity();
    if (tol > SMPLX_PI) return -1.0;
    const double c = std::cos(0.5 * tol);
    return 4.0 * c * c;
}

// Rz(yaw) Ry(pitch) Rx(roll), row-major 3x3: origin_matrix (model_compile.cpp) without the translation
static void rpy_matrix(const double rpy[3], double r[9])
{
    double sr, cr, sp, cp, sy, cy;
    smplx_sincos(rpy[0], &sr, &cr);
    smplx_sincos(rpy[1], &sp, &cp);
    smplx_sincos(rpy[2], &sy, &cy);
    r[0] = cy * cp; r[1] = (cy * sp) * sr - sy * cr; r[2] = (cy * sp) * cr + sy * sr;
    r[3] = sy * cp; r[4] = (sy * sp) * sr + cy * cr; r[5] = (sy * sp) * cr - cy * sr;
    r[6] = -sp;     r[7] = cp * sr;                  r[8] = cp * cr;
}

// XYZ_RPY_GOAL (manip_lattice.cpp:1614-1671): the XYZ goal's record plus the goal rotation and the bound of its test
static void pose_goal_record(smplx_space* s, const double xyz[3], const double rpy[3], const double xyz_tol[3], double rpy_tol)
{
    xyz_goal_record(s, xyz, xyz_tol);
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_XYZ_RPY;
    rpy_matrix(rpy, G.rot);
    for (int k = 0; k < 9; ++k) s->goal_rot[k] = G.rot[k];
    G.rpy_c4 = rpy_bound(rpy_tol);
    for (int a = 0; a < 3; ++a) s->goal_rpy[a] = rpy[a];
    s->goal_rpy_tol = rpy_tol;
}

// what the pose-goal entry points refuse in n goals: a non-finite pose, |xyz| >= 1e6 or |rpy| >= 1e6 (smplx_sincos reduces
// its argument through an int: the bound of the joint values), a NaN tolerance
static bool sane_pose_goals(const double* xyz, const double* rpy, const double* xyz_tol, const double* rpy_tol, size_t n)
{
    if (!sane_values(xyz, 3 * n) || !sane_values(rpy, 3 * n)) return false;
    for (size_t i = 0; i < 3 * n; ++i) if (std::isnan(xyz_tol[i])) return false;
    for (size_t i = 0; i < n; ++i) if (std::isnan(rpy_tol[i])) return false;
    return true;
}

// the Euclidean heuristic's goal rotation under a joint goal: the planning link's at the goal angles
// (planner_interface.cpp:1236-1238), by the FK that gave the goal position
static int joint_goal_rotation(smplx_space* s, const double* angles)
{
    if (s->params.heuristic != SMPLX_H_EUCLID) return SMPLX_OK;
    double T[12];
    if (int e = smplx_planning_pose_batch(s, angles, 1, T)) return e;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) s->goal_rot[3 * r + c] = T[4 * r + c];
    return SMPLX_OK;
}

int smplx_set_goal_joint(smplx_space* s, const double* angles, const double* tolerances)
{
    if (!s || !angles || !tolerances) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_values(angles, s->N)) return set_error(SMPLX_E_ARG, "goal angles must be finite (|q| < 1e6)");
    joint_goal_record(s, angles, tolerances);
    // goal pose = planning-link FK of the goal angles (planner_interface.cpp:1232-1235)
    int32_t h;
    if (int e = run_heuristic(s, angles, 1, &h, s->goal_xyz)) return e;
    if (int e = joint_goal_rotation(s, angles)) return e;
    return finish_goal(s);
}

int smplx_set_goal_xyz(smplx_space* s, const double xyz[3], const double tol[3])
{
    if (!s || !xyz || !tol) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_values(xyz, 3)) return set_error(SMPLX_E_ARG, "goal position must be finite");
    xyz_goal_record(s, xyz, tol);
    return finish_goal(s);
}

int smplx_set_goal_pose(smplx_space* s, const double xyz[3], const double rpy[3], const double xyz_tol[3], double rpy_tol)
{
    if (!xyz || !rpy || !xyz_tol) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_pose_goals(xyz, rpy, xyz_tol, &rpy_tol, 1)) return set_error(SMPLX_E_ARG, "goal pose must be finite (|xyz|, |rpy| < 1e6), tolerances not NaN");
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    pose_goal_record(s, xyz, rpy, xyz_tol, rpy_tol);
    return finish_goal(s);
}

// what the multi-goal entry points check before they touch a space: the array, no space twice (on the handles alone)
static int check_goal_spaces(smplx_space* const* spaces, int nq)
{
    if (!spaces || nq < 1) return set_error(SMPLX_E_ARG, "bad argument");
    for (int q = 0; q < nq; ++q) if (!spaces[q]) return set_error(SMPLX_E_ARG, "null space");
    for (int q = 0; q < nq; ++q)
        for (int r = 0; r < q; ++r)
            if (spaces[q] == spaces[r]) return set_error(SMPLX_E_ARG, "a space appears twice");
    return SMPLX_OK;
}

// ... and on the spaces: one device, the same bricks per axis (the goals share the launches of run_bfs_multi)
static int check_goal_spaces_match(smplx_space* const* spaces, int nq)
{
    const smplx_space* lead = nullptr;       // the first space that takes part in the shared BFS: a closed-form space does not
    for (int q = 0; q < nq; ++q) {
        if (spaces[q]->device != spaces[0]->device) return set_error(SMPLX_E_ARG, "the spaces live on different devices");
        if (closed_form(spaces[q])) continue;
        if (!lead) lead = spaces[q];
        for (int a = 0; a < 3; ++a)
            if (spaces[q]->bfs.bricks[a] != lead->bfs.bricks[a]) return set_error(SMPLX_E_ARG, "the spaces' grids differ in bricks per axis");
    }
    return SMPLX_OK;
}

// finish_goal for nq spaces whose goal records and goal poses are in place: one shared BFS
static int finish_goals_multi(smplx_space* const* spaces, int nq)
{
    int e = SMPLX_OK;
    for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = begin_goal(spaces[q]);
    // the shared sweep is of the spaces that plan with the BFS; a closed-form space has its goal from begin_goal alone
    std::vector<smplx_space*> with_bfs;
    for (int q = 0; q < nq; ++q) if (!closed_form(spaces[q])) with_bfs.push_back(spaces[q]);
    if (e == SMPLX_OK && !with_bfs.empty()) e = run_bfs_multi(with_bfs.data(), (int)with_bfs.size());
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) spaces[q]->goal_set = false;   // some grids are half written: no space keeps a goal
        return e;
    }
    for (int q = 0; q < nq; ++q) end_goal(spaces[q]);
    return SMPLX_OK;
}

int smplx_set_goals_joint_multi(smplx_space** spaces, int nq, const double* angles, const double* tolerances)
{
    if (int e = check_goal_spaces(spaces, nq)) return e;
    if (!angles || !tolerances) return set_error(SMPLX_E_ARG, "null argument");
    const int N = spaces[0]->N;
    for (int q = 1; q < nq; ++q) if (spaces[q]->N != N) return set_error(SMPLX_E_ARG, "the spaces differ in their number of variables");
    if (!sane_values(angles, (size_t)nq * N)) return set_error(SMPLX_E_ARG, "goal angles must be finite (|q| < 1e6)");
    if (int e = check_goal_spaces_match(spaces, nq)) return e;
    HIP_TRY(hipSetDevice(spaces[0]->device));
    for (int q = 0; q < nq; ++q) joint_goal_record(spaces[q], angles + (size_t)q * N, tolerances + (size_t)q * N);
    // goal poses = planning-link FK of the goal angles: one launch of the leading space's kernel when all run the same
    // kernel on the same model image (the same code on the same values: bit-equal to each space's own), else one each
    bool shared = true;
    for (int q = 1; q < nq && shared; ++q) shared = same_scene_and_robot(spaces[0], spaces[q]) && spaces[q]->ks.specialized == spaces[0]->ks.specialized;
    int e = SMPLX_OK;
    if (shared) {
        std::vector<double> xyz((size_t)nq * 3);
        e = run_heuristic(spaces[0], angles, nq, nullptr, xyz.data());
        for (int q = 0; q < nq && e == SMPLX_OK; ++q) for (int a = 0; a < 3; ++a) spaces[q]->goal_xyz[a] = xyz[(size_t)q * 3 + a];
    } else {
        for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = run_heuristic(spaces[q], angles + (size_t)q * N, 1, nullptr, spaces[q]->goal_xyz);
    }
    for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = joint_goal_rotation(spaces[q], angles + (size_t)q * N);
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) spaces[q]->goal_set = false;
        return e;
    }
    return finish_goals_multi(spaces, nq);
}

int smplx_set_goals_xyz_multi(smplx_space** spaces, int nq, const double* xyz, const double* tol)
{
    if (int e = check_goal_spaces(spaces, nq)) return e;
    if (!xyz || !tol) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_values(xyz, (size_t)nq * 3)) return set_error(SMPLX_E_ARG, "goal position must be finite");
    if (int e = check_goal_spaces_match(spaces, nq)) return e;
    HIP_TRY(hipSetDevice(spaces[0]->device));
    for (int q = 0; q < nq; ++q) xyz_goal_record(spaces[q], xyz + (size_t)q * 3, tol + (size_t)q * 3);
    return finish_goals_multi(spaces, nq);
}

int smplx_set_goals_pose_multi(smplx_space** spaces, int nq, const double* xyz, const double* rpy, const double* xyz_tol, const double* rpy_tol)
{
    if (int e = check_goal_spaces(spaces, nq)) return e;
    if (!xyz || !rpy || !xyz_tol || !rpy_tol) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_pose_goals(xyz, rpy, xyz_tol, rpy_tol, (size_t)nq)) return set_error(SMPLX_E_ARG, "goal poses must be finite (|xyz|, |rpy| < 1e6), tolerances not NaN");
    if (int e = check_goal_spaces_match(spaces, nq)) return e;
    HIP_TRY(hipSetDevice(spaces[0]->device));
    for (int q = 0; q < nq; ++q) pose_goal_record(spaces[q], xyz + (size_t)q * 3, rpy + (size_t)q * 3, xyz_tol + (size_t)q * 3, rpy_tol[q]);
    return finish_goals_multi(spaces, nq);
}

int smplx_goal_orientation(const smplx_space* s, double rpy[3], double* rpy_tol)
{
    if (!s || !rpy || !rpy_tol) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal_set || s->hs.goal.type != SMPLX_GOAL_XYZ_RPY) return set_error(SMPLX_E_STATE, "the goal is not a pose goal");
    for (int a = 0; a < 3; ++a) rpy[a] = s->goal_rpy[a];
    *rpy_tol = s->goal_rpy_tol;
    return SMPLX_OK;
}

// The reference's orientation distance (manip_lattice.cpp:1652-1665) literally: the ZYX-Euler quaternions of the two
// orientations, the sign flip, 2 acos of their dot product.  Rounding can put the dot product of two unit quaternions a
// few ulp above 1, where acos has no value: it counts as 1.
int smplx_rpy_angle(const double a[3], const double b[3], double* theta)
{
    if (!a || !b || !theta) return set_error(SMPLX_E_ARG, "null argument");
    for (int i = 0; i < 3; ++i) if (!std::isfinite(a[i]) || !std::isfinite(b[i])) return set_error(SMPLX_E_ARG, "angles must be finite");
    auto quat = [](const double rpy[3], double q[4]) {
        const double sr = std::sin(0.5 * rpy[0]), cr = std::cos(0.5 * rpy[0]), sp = std::sin(0.5 * rpy[1]), cp = std::cos(0.5 * rpy[1]);
        const double sy = std::sin(0.5 * rpy[2]), cy = std::cos(0.5 * rpy[2]);
        q[0] = cr * cp * cy + sr * sp * sy;   // w of AngleAxis(yaw, Z) * AngleAxis(pitch, Y) * AngleAxis(roll, X)
        q[1] = sr * cp * cy - cr * sp * sy;
        q[2] = cr * sp * cy + sr * cp * sy;
        q[3] = cr * cp * sy - sr * sp * cy;
    };
    double qa[4], qb[4];
    quat(a, qa);
    quat(b, qb);
    double d = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3];
    if (d < 0.0) d = -d;                      // qg negated (:1660-1662)
    if (d > 1.0) d = 1.0;
    *theta = smplx_normalize_angle(2.0 * std::acos(d));
    return SMPLX_OK;
}

int smplx_planning_pose_batch(smplx_space* s, const double* q, int n, double* T)
{
    if (!s || !q || !T || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = s->batch.b_q.reserve((size_t)n * s->N)) return e;
    if (int e = s->b_sq.reserve((size_t)n * 12)) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_PLANNING_POSE, k_planning_pose, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->blob_bytes, s->stream, s->d_space,
            s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(T, s->b_sq.p, sizeof(double) * n * 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int smplx_goal_pose(const smplx_space* s, double xyz[3])
{
    if (!s || !xyz) return set_error(SMPLX_E_ARG, "null argument");
    for (int a = 0; a < 3; ++a) xyz[a] = s->goal_xyz[a];
    return SMPLX_OK;
}

int smplx_heuristic_batch(smplx_space* s, const double* q, int n, int32_t* h, double* xyz)
{
    if (!s || !q || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    return run_heuristic(s, q, n, h, xyz);
}

static const char* const kNoBfs = "the space plans with a closed-form heuristic (smplx_params.heuristic): it has no BFS grid";

int64_t smplx_bfs_size(const smplx_space* s) { return s ? s->bfs.total : 0; }
int smplx_bfs_levels(const smplx_space* s) { return s ? s->bfs.levels : 0; }

int smplx_bfs_copy(smplx_space* s, int32_t* out)
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    if (closed_form(s)) return set_error(SMPLX_E_STATE, kNoBfs);
    // the device keeps brick-major records (device_types.h SmplxBfsDev); what goes out is the reference's padded array
    int32_t* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, sizeof(int32_t) * s->bfs.total));
    hipLaunchKernelGGL(k_bfs_export, dim3(2048), dim3(256), 0, s->stream, s->hs.bfs, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, sizeof(int32_t) * s->bfs.total, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return set_error(SMPLX_E_HIP, std::string("smplx_bfs_copy: ") + hipGetErrorString(e));
    return SMPLX_OK;
}

int smplx_bfs_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out)
{
    if (!s || !xyz || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (closed_form(s)) return set_error(SMPLX_E_STATE, kNoBfs);
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "goal not set");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(xyz, (size_t)n * 3)) return set_error(SMPLX_E_ARG, "positions must be finite");
    int e;
    if ((e = s->b_xyz.reserve((size_t)n * 3))) return e;
    if ((e = s->b_q2.reserve(n))) return e;
    HIP_TRY(hipMemcpyAsync(s->b_xyz.p, xyz, sizeof(double) * n * 3, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_bfs_metric, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), 0, s->stream, s->hs.grid, s->hs.bfs, s->b_xyz.p, n,
                       s->b_q2.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->b_q2.p, sizeof(double) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int smplx_bfs_metric_start_distance(smplx_space* s, const double* xyz, int n, double* out)
{
    if (!s || !xyz || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (closed_form(s)) return set_error(SMPLX_E_STATE, kNoBfs);
    if (s->lat.start_id < 0) return set_error(SMPLX_E_STATE, "start not set");
    // bfs_heuristic.cpp:103-127: Manhattan distance in cells between the start's planning-link cell and the point's
    const smplx_grid* g = s->grid;
    auto cell = [&](const double* p, int c[3]) {
        for (int a = 0; a < 3; ++a) c[a] = (int)(g->dev.inv_res * (p[a] - g->dev.origin_minus_res[a]) + 0.5) - 1;
    };
    int sc[3];
    cell(s->start_xyz, sc);
    for (int i = 0; i < n; ++i) {
        int c[3];
        cell(xyz + 3 * (size_t)i, c);
        out[i] = g->res * (double)(std::abs(sc[0] - c[0]) + std::abs(sc[1] - c[1]) + std::abs(sc[2] - c[2]));
    }
    return SMPLX_OK;
}

int smplx_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out)
{
    if (!s || !xyz || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!closed_form(s)) return smplx_bfs_metric_goal_distance(s, xyz, n, out);
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "goal not set");
    if (!sane_values(xyz, (size_t)n * 3)) return set_error(SMPLX_E_ARG, "positions must be finite");
    // euclid_dist_heuristic.cpp:98-102 / joint_dist_heuristic.cpp:52-55: host arithmetic, the kernels' own functions
    for (int i = 0; i < n; ++i)
        out[i] = s->params.heuristic == SMPLX_H_EUCLID ? smplx_point_dist(xyz + 3 * (size_t)i, s->goal_xyz) : 0.0;
    return SMPLX_OK;
}

int smplx_set_euclid_weights(smplx_space* s, const double w[4])
{
    if (!s || !w) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 4; ++k) if (!std::isfinite(w[k]) || w[k] < 0.0) return set_error(SMPLX_E_ARG, "weights must be finite and not negative");
    if (s->params.heuristic != SMPLX_H_EUCLID) return set_error(SMPLX_E_STATE, "the space's heuristic is not SMPLX_H_EUCLID");
    for (int k = 0; k < 4; ++k) s->hs.heur.w[k] = w[k];
    // every h recorded so far used the old weights: the space has no goal until it is set again (which uploads the record
    // and restarts the lattice)
    s->goal_set = false;
    return SMPLX_OK;
}

int smplx_pose_distance(const double Ta[12], const double Tb[12], const double w[4], double* dist)
{
    if (!Ta || !Tb || !w || !dist) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 12; ++k) if (!std::isfinite(Ta[k]) || !std::isfinite(Tb[k])) return set_error(SMPLX_E_ARG, "transforms must be finite");
    for (int k = 0; k < 4; ++k) if (!std::isfinite(w[k]) || w[k] < 0.0) return set_error(SMPLX_E_ARG, "weights must be finite and not negative");
    double pa[3], pb[3], Ra[9], Rb[9];
    for (int r = 0; r < 3; ++r) {
        pa[r] = Ta[4 * r + 3]; pb[r] = Tb[4 * r + 3];
        for (int c = 0; c < 3; ++c) { Ra[3 * r + c] = Ta[4 * r + c]; Rb[3 * r + c] = Tb[4 * r + c]; }
    }
    *dist = smplx_pose_dist(pa, Ra, pb, Rb, w);
    return SMPLX_OK;
}

int smplx_joint_distance(const double* a, const double* b, int n, double* dist)
{
    if (!a || !b || !dist || n < 0 || n > SMPLX_MAX_VARS) return set_error(SMPLX_E_ARG, "bad argument (n: 0 to 16)");
    for (int k = 0; k < n; ++k) if (!std::isfinite(a[k]) || !std::isfinite(b[k])) return set_error(SMPLX_E_ARG, "joint values must be finite");
    *dist = smplx_joint_dist(a, b, n);
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

int smplx_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                       int32_t* cost, int32_t* lookups)
{
    if (!s || !q || B < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (B == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = reserve_expand(s, B)) return e;
    const size_t BM = (size_t)B * s->M;
    HIP_TRY(hipMemsetAsync(s->b_coord.p, 0, sizeof(int32_t) * BM * s->N, s->stream));
    HIP_TRY(hipMemsetAsync(s->b_sq.p, 0, sizeof(double) * BM * s->N, s->stream));
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * B * s->N, hipMemcpyHostToDevice, s->stream));
    if (int e = smplx_expand_batch_device(s, s->batch.b_q.p, B, s->b_flags.p, s->b_coord.p, s->b_sq.p, s->b_h.p, s->batch.b_cost.p,
                                          s->batch.b_lookups.p, s->batch.b_work.p, nullptr, s->stream)) return e;
    if (flags) HIP_TRY(hipMemcpyAsync(flags, s->b_flags.p, BM, hipMemcpyDeviceToHost, s->stream));
    if (coord) HIP_TRY(hipMemcpyAsync(coord, s->b_coord.p, sizeof(int32_t) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (succ_q) HIP_TRY(hipMemcpyAsync(succ_q, s->b_sq.p, sizeof(double) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (h) HIP_TRY(hipMemcpyAsync(h, s->b_h.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, s->batch.b_cost.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    if (lookups) HIP_TRY(hipMemcpyAsync(lookups, s->batch.b_lookups.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

size_t smplx_expand_work_bytes(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    return expand_work_bytes(B, s->M, s->N);
}

int smplx_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                              int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, void* d_work, uint64_t* d_counters, void* stream)
{
    if (!s || !d_q || !d_flags || !d_coord || !d_succ_q || !d_h || !d_cost || !d_lookups || !d_work || B <= 0)
        return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first");
    // the K5 launch without its outputs
    return smplx_expand_batch_k5_device(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_cost, d_lookups, nullptr, nullptr, 0, nullptr, 0,
                                        nullptr, nullptr, d_work, d_counters, stream);
}

int smplx_table_sync(smplx_space* s)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = table_ensure(s)) return e;
    if (int e = table_flush(s, s->stream)) return e;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

size_t smplx_compact_rec_b_bytes(const smplx_space* s) { return s ? (size_t)smplx_rec_b_bytes(s->N) : 0; }
int smplx_compact_blocks(const smplx_space* s, int B) { return s && B > 0 ? blocks_for((long long)B * s->M, SMPLX_BLOCK) : 0; }
int smplx_compact_totals_len(void) { return SMPLX_CMP_TOTALS; }
int smplx_compact_capacity(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    const int nblocks = blocks_for((long long)B * s->M, SMPLX_BLOCK);
    return SMPLX_CMP_SHARDS * ((nblocks + SMPLX_CMP_SHARDS - 1) / SMPLX_CMP_SHARDS) * SMPLX_BLOCK;   // no sub-region can overflow
}

namespace {
// smplx_expand_batch_k5_device, plus the states to insert at the head of the step's first kernel (device memory)
int expand_k5_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                     int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, int32_t* d_succ_id, int32_t* d_rec_a, int cap_a,
                     void* d_rec_b, int cap_b, int32_t* d_block_tab, int32_t* d_totals, void* d_work,
                     uint64_t* d_counters, void* stream, const int32_t* d_items, int n_items)
{
    if (!s || !d_q || !d_flags || !d_coord || !d_succ_q || !d_h || !d_cost || !d_lookups || !d_work || B <= 0)
        return set_error(SMPLX_E_ARG, "bad argument");
    if (d_rec_a && (!d_rec_b || !d_block_tab || !d_totals || cap_a < SMPLX_CMP_SHARDS || cap_b < SMPLX_CMP_SHARDS))
        return set_error(SMPLX_E_ARG, "incomplete compact-stream arguments");
    cap_a = cap_a / SMPLX_CMP_SHARDS * SMPLX_CMP_SHARDS;
    cap_b = cap_b / SMPLX_CMP_SHARDS * SMPLX_CMP_SHARDS;
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (s->step.fused_mode && d_rec_a) return set_error(SMPLX_E_STATE, "the compact stream needs the pipeline kernels (not fused mode)");
    SmplxCompactDev cmp;
    std::memset(&cmp, 0, sizeof(cmp));
    cmp.rec_a = d_rec_a; cmp.rec_b = (unsigned char*)d_rec_b; cmp.block_tab = d_block_tab; cmp.totals = d_totals;
    cmp.cap_a = cap_a; cmp.cap_b = cap_b; cmp.rec_b_bytes = smplx_rec_b_bytes(s->N);
    K5Out k5;
    k5.d_id = d_succ_id;
    k5.cmp = d_rec_a ? &cmp : nullptr;
    k5.items = d_items;
    k5.n_items = n_items;
    ExpandArgs a;
    a.q = d_q; a.B = B;
    a.flags = d_flags; a.coord = d_coord; a.sq = d_succ_q; a.h = d_h; a.cost = d_cost; a.lookups = d_lookups;
    a.work = d_work;
    a.counters = (unsigned long long*)d_counters;
    a.stream = (hipStream_t)stream;
    a.k5 = &k5;
    return launch_expand(s, a);
}
}  // namespace

int smplx_expand_batch_k5_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                 int32_t* d_h, int32_t* d_cost, int32_t* d_lookups, int32_t* d_succ_id, int32_t* d_rec_a, int cap_a,
                                 void* d_rec_b, int cap_b, int32_t* d_block_tab, int32_t* d_totals, void* d_work,
                                 uint64_t* d_counters, void* stream)
{
    return expand_k5_device(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_cost, d_lookups, d_succ_id, d_rec_a, cap_a, d_rec_b, cap_b,
                            d_block_tab, d_totals, d_work, d_counters, stream, nullptr, 0);
}

int smplx_expand_batch_k5(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                          int32_t* succ_id, int32_t* rec_a, int cap_a, void* rec_b, int cap_b, int32_t* block_tab, int32_t totals[3])
{
    if (!s || !q || B <= 0 || !rec_a || !rec_b || !block_tab || !totals || cap_a <= 0 || cap_b <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = reserve_expand(s, B)) return e;
    const size_t BM = (size_t)B * s->M;
    const size_t rb = (size_t)smplx_rec_b_bytes(s->N);
    const int nblocks = blocks_for((long long)BM, SMPLX_BLOCK);
    int e;
    if ((e = s->b_way.reserve(BM))) return e;                                       // dense ids
    if ((e = s->dt.b_ins.reserve(2 * (size_t)cap_a + 4 * (size_t)nblocks + SMPLX_CMP_TOTALS))) return e;   // A records | block table | totals
    if ((e = s->batch.b_out.reserve(rb * (size_t)cap_b))) return e;                       // B records
    if ((e = table_ensure(s))) return e;
    // the states committed since the last batch ride with the step's first kernel, behind the parents in the same
    // buffer, as they do in a search's own batches (issue_frontier)
    if ((e = table_grow_if_needed(s))) return e;
    std::vector<int32_t>& items = s->batch.ins_items;   // stays put until the synchronise below
    items.clear();
    table_take_pending(s, 0, items);
    const size_t parent_doubles = (size_t)B * s->N;
    if ((e = s->batch.b_q.reserve(parent_doubles + (items.size() + 1) / 2))) return e;
    int32_t* d_a = s->dt.b_ins.p;
    int32_t* d_bt = d_a + 2 * (size_t)cap_a;
    int32_t* d_tot = d_bt + 4 * (size_t)nblocks;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * parent_doubles, hipMemcpyHostToDevice, s->stream));
    if (!items.empty())
        HIP_TRY(hipMemcpyAsync(s->batch.b_q.p + parent_doubles, items.data(), sizeof(int32_t) * items.size(), hipMemcpyHostToDevice, s->stream));
    if ((e = expand_k5_device(s, s->batch.b_q.p, B, s->b_flags.p, s->b_coord.p, s->b_sq.p, s->b_h.p, s->batch.b_cost.p, s->batch.b_lookups.p,
                              s->b_way.p, d_a, cap_a, s->batch.b_out.p, cap_b, d_bt, d_tot, s->batch.b_work.p, nullptr, s->stream,
                              (const int32_t*)(s->batch.b_q.p + parent_doubles), (int)(items.size() / ((size_t)s->N + 2))))) return e;
    if (flags) HIP_TRY(hipMemcpyAsync(flags, s->b_flags.p, BM, hipMemcpyDeviceToHost, s->stream));
    if (coord) HIP_TRY(hipMemcpyAsync(coord, s->b_coord.p, sizeof(int32_t) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (succ_q) HIP_TRY(hipMemcpyAsync(succ_q, s->b_sq.p, sizeof(double) * BM * s->N, hipMemcpyDeviceToHost, s->stream));
    if (h) HIP_TRY(hipMemcpyAsync(h, s->b_h.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    if (succ_id) HIP_TRY(hipMemcpyAsync(succ_id, s->b_way.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(rec_a, d_a, sizeof(int32_t) * 2 * (size_t)cap_a, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(rec_b, s->batch.b_out.p, rb * (size_t)cap_b, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(block_tab, d_bt, sizeof(int32_t) * 4 * (size_t)nblocks, hipMemcpyDeviceToHost, s->stream));
    int32_t raw[SMPLX_CMP_TOTALS];
    HIP_TRY(hipMemcpyAsync(raw, d_tot, sizeof(raw), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    totals[0] = totals[1] = 0;
    for (int k = 0; k < SMPLX_CMP_SHARDS; ++k) { totals[0] += raw[32 * k]; totals[1] += raw[32 * k + 1]; }
    totals[2] = raw[32 * SMPLX_CMP_SHARDS];
    return SMPLX_OK;
}

size_t smplx_counters_bytes(const smplx_space* s, int B)
{
    if (!s || B <= 0) return 0;
    return counter_words(B, s->M) * sizeof(unsigned long long);
}

int smplx_counters_read(const smplx_space* s, const uint64_t* d_counters, int B, uint64_t out[6])
{
    if (!s || !d_counters || !out || B <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    const size_t cw = counter_words(B, s->M);
    std::vector<unsigned long long> part(cw);
    HIP_TRY(hipMemcpy(part.data(), d_counters, sizeof(unsigned long long) * cw, hipMemcpyDeviceToHost));
    for (int k = 0; k < SMPLX_TALLIES; ++k) out[k] = 0;
    for (size_t i = 0; i < cw; ++i) out[i % SMPLX_TALLIES] += part[i];
    return SMPLX_OK;
}

int smplx_profile_begin(smplx_space* s, int max_launches)
{
    if (!s || max_launches < 0) return set_error(SMPLX_E_ARG, "bad argument");
    for (hipEvent_t e : s->step.prof_events) (void)hipEventDestroy(e);
    s->step.prof_events.clear();
    s->step.prof_used = 0;
    for (int i = 0; i < 3 * max_launches; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        s->step.prof_events.push_back(e);
    }
    return SMPLX_OK;
}

int smplx_profile_end(smplx_space* s, double* prep_ms, double* expand_ms, int* launches)
{
    if (!s || !prep_ms || !expand_ms || !launches) return set_error(SMPLX_E_ARG, "null argument");
    double a = 0.0, b = 0.0;
    const int n = (int)(s->step.prof_used / 3);
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        HIP_TRY(hipEventSynchronize(s->step.prof_events[3 * i + 2]));
        HIP_TRY(hipEventElapsedTime(&t, s->step.prof_events[3 * i], s->step.prof_events[3 * i + 1]));
        a += t;
        HIP_TRY(hipEventElapsedTime(&t, s->step.prof_events[3 * i + 1], s->step.prof_events[3 * i + 2]));
        b += t;
    }
    *prep_ms = a; *expand_ms = b; *launches = n;
    for (hipEvent_t e : s->step.prof_events) (void)hipEventDestroy(e);
    s->step.prof_events.clear();
    s->step.prof_used = 0;
    return SMPLX_OK;
}

int smplx_set_start(smplx_space* s, const double* q, int* id)
{
    if (!s || !q) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set the goal before the start (planner_interface.cpp:1469-1500 order)");
    if (!sane_values(q, s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (!host_check_limits(s->model.dev, q)) return set_error(SMPLX_E_INVALID, "start state violates joint limits");
    if (int e = pull_lattice(s)) return e;
    uint8_t ok = 0;
    if (int e = smplx_cc_state_valid_batch(s, q, 1, &ok, nullptr)) return e;
    if (!ok) return set_error(SMPLX_E_INVALID, "start state is in collision");
    std::vector<int32_t> c(s->N);
    state_to_coord(s->model.dev, q, c.data());
    int sid = s->lat.table.find(c.data(), s->lat.coords);
    int32_t h = 0;
    if (int e = run_heuristic(s, q, 1, &h, s->start_xyz)) return e;   // also the start's planning-link position
    if (sid < 0) sid = new_state(s, c.data(), q, h);
    s->lat.start_id = sid;
    if (s->spec.plain_mode) { std::fill(s->lat.g_est.begin(), s->lat.g_est.end(), 1000000000u); s->lat.g_est[sid] = 0; s->spec.pool.clear(); }
    if (id) *id = sid;
    return SMPLX_OK;
}

int smplx_start_id(const smplx_space* s) { return s ? s->lat.start_id : -1; }
int smplx_goal_id(const smplx_space* s) { (void)s; return 0; }

int smplx_get_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n)
{
    if (!s || !n) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "goal not set");
    if (s->grid->epoch != s->grid_epoch) return set_error(SMPLX_E_STATE, "the grid was edited after the goal was set: cached successors are stale, set the goal again");
    if (s->att.epoch != s->att.epoch_goal) return set_error(SMPLX_E_STATE, kBodiesChanged);
    if (int e = pull_lattice(s)) return e;
    if (!s->spec.plain_mode) {
        // first GetSuccs from outside: start mirroring the caller's g-values (the start has g = 0, arastar.cpp:172-176)
        s->spec.plain_mode = true;
        std::fill(s->lat.g_est.begin(), s->lat.g_est.end(), 1000000000u);
        if (s->lat.start_id > 0) s->lat.g_est[s->lat.start_id] = 0;
        s->spec.pool.clear();
    }
    const int32_t *ps, *pc;
    int cnt = 0;
    if (int e = get_succs(s, id, &ps, &pc, &cnt)) {
        // the SBPL-side caller (GetSuccs has no return value) sees an empty list; the error stays readable here
        if (s->status == SMPLX_OK) { s->status = e; s->status_msg = g_error; }
        return e;
    }
    *n = cnt;
    for (int i = 0; i < cnt && i < cap; ++i) {
        if (succs) succs[i] = ps[i];
        if (costs) costs[i] = pc[i];
    }
    return SMPLX_OK;
}

// ---- lazy successors: GetLazySuccs / GetTrueCost (include/smpl_amd.h; kernels: lazy_kernels.h, host: lazy.h) ----------

int smplx_get_lazy_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n)
{
    if (n) *n = 0;
    if (!s || !n) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = lazy_guard(s)) return lazy_keep_status(s, e);
    const int32_t* ps = nullptr;
    int cnt = 0;
    if (int e = get_lazy_succs(s, id, &ps, &cnt)) return lazy_keep_status(s, e);
    *n = cnt;
    for (int i = 0; i < cnt && i < cap; ++i) {
        if (succs) succs[i] = ps[i];
        if (costs) costs[i] = SMPLX_LAZY_COST;
    }
    return SMPLX_OK;
}

int smplx_true_cost_batch(smplx_space* s, const int32_t* parent_ids, const int32_t* child_ids, int n, int32_t* costs, int32_t* prims,
                          int32_t* nmatch)
{
    if (!s || n < 0 || (n > 0 && (!parent_ids || !child_ids || !costs))) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (int e = lazy_guard(s)) return e;
    return true_cost_pairs(s, parent_ids, child_ids, n, costs, prims, nmatch, false);
}

int smplx_get_true_cost(smplx_space* s, int parent_id, int child_id, int32_t* cost)
{
    if (cost) *cost = -1;
    if (!s || !cost) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = lazy_guard(s)) return lazy_keep_status(s, e);
    const int32_t p = parent_id, c = child_id;
    return lazy_keep_status(s, true_cost_pairs(s, &p, &c, 1, cost, nullptr, nullptr, true));
}

int smplx_lazy_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                            int32_t* succ_id)
{
    if (!s || !q || B < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (B == 0) return SMPLX_OK;
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = pull_lattice(s)) return e;
    return lazy_rows(s, q, B, flags, coord, succ_q, h, succ_id, true);
}

int smplx_lazy_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                   int32_t* d_h, int32_t* d_succ_id, void* stream)
{
    if (!s || !d_q || !d_flags || B <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (int e = pull_lattice(s)) return e;
    return launch_lazy_succs(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_succ_id, (hipStream_t)stream, true);
}

int smplx_true_cost_q_batch(smplx_space* s, const double* parent_q, const int32_t* child_coord, const uint8_t* goal_edge, int n,
                            int32_t* costs, int32_t* prims, int32_t* nmatch)
{
    if (!s || n < 0 || (n > 0 && (!parent_q || !child_coord || !costs))) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (!sane_values(parent_q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    return true_cost_items(s, parent_q, child_coord, goal_edge, n, costs, prims, nmatch);
}

size_t smplx_true_cost_work_doubles(const smplx_space* s, int n)
{
    return s && n > 0 ? (size_t)n * s->N * SMPLX_TRUE_COST_LANES : 0;
}

int smplx_true_cost_q_batch_device(smplx_space* s, const double* d_parent_q, const int32_t* d_child_coord, const uint8_t* d_goal_edge,
                                   int n, double* d_work_q, int32_t* d_costs, int32_t* d_prims, int32_t* d_nmatch, void* stream)
{
    if (!s || !d_parent_q || !d_child_coord || !d_goal_edge || !d_work_q || !d_costs || n <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal_set) return set_error(SMPLX_E_STATE, "set a goal first");
    return launch_true_cost(s, d_parent_q, d_child_coord, d_goal_edge, n, d_work_q, d_costs, d_prims, d_nmatch, (hipStream_t)stream);
}

int smplx_lazy_counters(const smplx_space* s, int64_t out[6])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = s->lazy.counters[k];
    return SMPLX_OK;
}

int smplx_hint_frontier(smplx_space* s, const int32_t* ids, int n)
{
    if (!s || (!ids && n > 0)) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = pull_lattice(s)) return e;
    s->spec.hint.assign(ids, ids + n);
    return SMPLX_OK;
}

int smplx_get_goal_heuristic(smplx_space* s, int id, int32_t* h)
{
    if (!s || !h) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = pull_lattice(s)) return e;
    if (id < 0 || id >= (int)s->lat.h_of_id.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    *h = s->lat.h_of_id[id];
    return SMPLX_OK;
}

int smplx_num_states(const smplx_space* s)
{
    if (!s) return 0;
    if (s->ds.host_behind) return s->ds.h.nstates;     // the device-resident search created states the host has not fetched yet
    return (int)s->lat.h_of_id.size();
}

int smplx_space_counters(const smplx_space* s, int64_t out[6])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    out[0] = s->gpu_batches; out[1] = s->cache_hits; out[2] = s->cache_misses; out[3] = s->committed_evals;
    out[4] = s->gpu_evals; out[5] = (int64_t)smplx_num_states(s);
    return SMPLX_OK;
}

int smplx_get_state(const smplx_space* cs, int id, double* q, int32_t* coord)
{
    if (!cs) return set_error(SMPLX_E_ARG, "null argument");
    smplx_space* s = const_cast<smplx_space*>(cs);      // (fetching what the device created does not change the lattice)
    if (int e = pull_lattice(s)) return e;
    if (id < 0 || id >= (int)s->lat.h_of_id.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    if (q) std::memcpy(q, &s->lat.qs[(size_t)id * s->N], sizeof(double) * s->N);
    if (coord) std::memcpy(coord, &s->lat.coords[(size_t)id * s->N], sizeof(int32_t) * s->N);
    return SMPLX_OK;
}

int smplx_replan_multi(smplx_space** spaces, int nq, const smplx_time_params* p, int32_t* path_ids, int cap,
                       smplx_replan_stats* stats, double* wall_seconds, int host_threads)
{
    const auto t_call = std::chrono::steady_clock::now();
    if (!spaces || nq <= 0 || !p || !stats) return set_error(SMPLX_E_ARG, "bad argument");
    if (path_ids && cap <= 0) return set_error(SMPLX_E_ARG, "path_ids needs cap > 0");
    if (p->type != SMPLX_TIME_EXPANSIONS && p->type != SMPLX_TIME_WALL) return set_error(SMPLX_E_ARG, "unknown timing type");
    if (!(p->max_seconds_init >= 0.0) || !(p->max_seconds >= 0.0)) return set_error(SMPLX_E_ARG, "time budgets must be >= 0");
    if (!(p->initial_eps >= 1.0) || !(p->final_eps >= 0.0) || !(p->delta_eps > 0.0) || !std::isfinite(p->initial_eps))
        return set_error(SMPLX_E_ARG, "epsilons: initial_eps >= 1 (finite), final_eps >= 0, delta_eps > 0");
    for (int q = 0; q < nq; ++q)
        for (int r = 0; r < q; ++r)
            if (spaces[q] && spaces[q] == spaces[r]) return set_error(SMPLX_E_ARG, "a space appears twice");
    const int e = replan_multi(spaces, nq, p, path_ids, cap, stats, wall_seconds, host_threads, t_call);
    if (e != SMPLX_OK)
        for (int q = 0; q < nq; ++q) if (spaces[q]) spaces[q]->search_side = 0;   // a failed call: the next one starts from scratch
    return e;
}

int smplx_replan(smplx_space* s, const smplx_time_params* p, int32_t* path_ids, int cap, smplx_replan_stats* st)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    return smplx_replan_multi(&s, 1, p, path_ids, cap, st, nullptr, 1);
}

// ARAStar::replan from scratch under an expansion bound: smplx_replan_multi with from_scratch = 1
int smplx_plan_multi(smplx_space** spaces, int nq, const smplx_search_params* p, int32_t* path_ids, int cap,
                     smplx_search_stats* stats, double* wall_seconds, int host_threads)
{
    const auto t_call = std::chrono::steady_clock::now();
    if (!spaces || nq <= 0 || !p || !stats) return set_error(SMPLX_E_ARG, "bad argument");
    smplx_time_params tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.initial_eps = p->initial_eps; tp.final_eps = p->final_eps; tp.delta_eps = p->delta_eps;
    tp.improve = p->improve; tp.bounded = p->bounded; tp.type = SMPLX_TIME_EXPANSIONS;
    tp.max_expansions_init = p->max_expansions_init; tp.max_expansions = p->max_expansions;
    tp.from_scratch = 1;
    std::vector<smplx_replan_stats> rs(nq);
    const int e = replan_multi(spaces, nq, &tp, path_ids, cap, rs.data(), wall_seconds, host_threads, t_call);
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) if (spaces[q]) spaces[q]->search_side = 0;
        return e;
    }
    for (int q = 0; q < nq; ++q) stats[q] = rs[q].s;
    return SMPLX_OK;
}

int smplx_plan(smplx_space* s, const smplx_search_params* p, int32_t* path_ids, int cap, smplx_search_stats* stats)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    return smplx_plan_multi(&s, 1, p, path_ids, cap, stats, nullptr, 1);
}

int smplx_expansion_log_size(const smplx_space* s)
{
    if (!s) return 0;
    return s->ds.log_on_device ? s->ds.h.n_log : (int)s->expansion_log.size();
}

int smplx_expansion_log(const smplx_space* cs, int32_t* out)
{
    if (!cs || !out) return set_error(SMPLX_E_ARG, "null argument");
    smplx_space* s = const_cast<smplx_space*>(cs);
    if (int e = pull_log(s)) return e;
    std::copy(s->expansion_log.begin(), s->expansion_log.end(), out);
    return SMPLX_OK;
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

int smplx_post_process_path(smplx_space* s, const double* path, int n, int flags, double* out, int cap, int* nout,
                            int64_t* stats)
{
    if (!s || (!path && n > 0) || n < 0 || !nout) return set_error(SMPLX_E_ARG, "bad argument");
    if (n > 0 && !sane_values(path, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    PathTools T(s);
    std::vector<double> p(path, path + (size_t)n * s->N);
    const bool fork_test = !(flags & SMPLX_PP_UPSTREAM_LIMITS);
    bool done = false;
    // PlannerInterface::postProcessPath (planner_interface.cpp:2651-2697)
    if (flags & SMPLX_PP_SHORTCUT) {
        if (int e = interpolate_path(T, p, fork_test, &done)) return e;   // failure leaves the path as it was
        std::vector<double> in = p;
        if (int e = shortcut_path(T, in, p)) return e;
    }
    if (flags & SMPLX_PP_INTERPOLATE) {
        if (int e = interpolate_path(T, p, fork_test, &done)) return e;
    }
    const int np = (int)(p.size() / s->N);
    *nout = np;
    if (stats) { stats[0] = T.edge_batches; stats[1] = T.configs; }
    if (out) {
        if (np > cap) return set_error(SMPLX_E_LIMIT, "output path does not fit");
        std::memcpy(out, p.data(), sizeof(double) * p.size());
    }
    return SMPLX_OK;
}

}  // extern "C"
