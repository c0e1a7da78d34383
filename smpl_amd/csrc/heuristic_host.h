// smpl_amd/csrc/heuristic_host.h -- the heuristic as the C-ABI shows it: the kernel launch behind every h value and
// planning-link position the host asks for (run_heuristic), the planning link's pose, read access to the BFS distance
// field (bfs_host.h runs it), the metric distances, and the closed forms of heuristics.h on host values.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "bfs_host.h"
#include "det_math.h"
#include "heuristics.h"

namespace {

static_assert(SMPLX_HEUR_BFS == SMPLX_H_BFS && SMPLX_HEUR_EUCLID == SMPLX_H_EUCLID && SMPLX_HEUR_JOINT_DIST == SMPLX_H_JOINT_DIST,
              "the device's heuristic kinds are the public ones");

// does the space plan with one of the closed forms of heuristics.h (no BFS: bfs_host.h is never entered for it)
bool closed_form(const smplx_space* s) { return s->params.heuristic != SMPLX_H_BFS; }

int run_heuristic(smplx_space* s, const double* q, int n, int32_t* h, double* xyz)
{
    const int N = s->N;
    if (int e = reserve(s->batch.b_q, (size_t)n * N)) return e;
    if (int e = reserve(s->b_h, n)) return e;
    if (int e = reserve(s->b_xyz, (size_t)n * 3)) return e;
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

const char* const kNoBfs = "the space plans with a closed-form heuristic (smplx_params.heuristic): it has no BFS grid";

}  // namespace

extern "C" {

int smplx_heuristic_batch(smplx_space* s, const double* q, int n, int32_t* h, double* xyz)
{
    if (!s || !q || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    return run_heuristic(s, q, n, h, xyz);
}

int smplx_planning_pose_batch(smplx_space* s, const double* q, int n, double* T)
{
    if (!s || !q || !T || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = reserve(s->batch.b_q, (size_t)n * s->N)) return e;
    if (int e = reserve(s->b_sq, (size_t)n * 12)) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_PLANNING_POSE, k_planning_pose, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->blob_bytes, s->stream, s->d_space,
            s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(T, s->b_sq.p, sizeof(double) * n * 12, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int64_t smplx_bfs_size(const smplx_space* s) { return s ? s->bfs.total : 0; }
int smplx_bfs_levels(const smplx_space* s) { return s ? s->bfs.levels : 0; }

int smplx_bfs_copy(smplx_space* s, int32_t* out)
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    if (closed_form(s)) return set_error(SMPLX_E_STATE, kNoBfs);
    // the device keeps brick-major records (device_types.h SmplxBfsDev); what goes out is the reference's padded array
    DevPtr<int32_t> tmp;
    HIP_TRY(tmp.alloc(s->bfs.total));
    hipLaunchKernelGGL(k_bfs_export, dim3(2048), dim3(256), 0, s->stream, s->hs.bfs, tmp.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, sizeof(int32_t) * s->bfs.total, hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    return hip_status(e, "smplx_bfs_copy");
}

int smplx_bfs_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out)
{
    if (!s || !xyz || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (closed_form(s)) return set_error(SMPLX_E_STATE, kNoBfs);
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(xyz, (size_t)n * 3)) return set_error(SMPLX_E_ARG, "positions must be finite");
    int e;
    if ((e = reserve(s->b_xyz, (size_t)n * 3))) return e;
    if ((e = reserve(s->b_q2, n))) return e;
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
    int sc[3];
    (void)bfs_goal_cell(s, s->goal.start_xyz, sc);
    for (int i = 0; i < n; ++i) {
        int c[3];
        (void)bfs_goal_cell(s, xyz + 3 * (size_t)i, c);
        out[i] = s->grid->res * (double)(std::abs(sc[0] - c[0]) + std::abs(sc[1] - c[1]) + std::abs(sc[2] - c[2]));
    }
    return SMPLX_OK;
}

int smplx_metric_goal_distance(smplx_space* s, const double* xyz, int n, double* out)
{
    if (!s || !xyz || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!closed_form(s)) return smplx_bfs_metric_goal_distance(s, xyz, n, out);
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
    if (!sane_values(xyz, (size_t)n * 3)) return set_error(SMPLX_E_ARG, "positions must be finite");
    // euclid_dist_heuristic.cpp:98-102 / joint_dist_heuristic.cpp:52-55: host arithmetic, the kernels' own functions
    for (int i = 0; i < n; ++i)
        out[i] = s->params.heuristic == SMPLX_H_EUCLID ? smplx_point_dist(xyz + 3 * (size_t)i, s->goal.xyz) : 0.0;
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
    s->goal.set = false;
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

int smplx_test_acos(const double* x, int n, double* out)
{
    if (!x || !out || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    for (int i = 0; i < n; ++i) out[i] = smplx_acos(x[i]);
    return SMPLX_OK;
}

}  // extern "C"
