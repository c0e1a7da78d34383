// smpl_amd/csrc/queries.h -- the collision queries of the C-ABI on joint values the caller hands over: joint limits, state
// and edge validity, the interpolation between two states, the world-frame sphere positions of the robot and of its
// attached bodies, and the clearance of states and edges (kernels: query_kernels.h, clearance_kernels.h).  A host variant
// stages its rows in the space's scratch and, where the ABI has a _device twin, calls that twin on the space's own
// buffers and stream: the launch is written once.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "det_math.h"
#include "kernels.h"
#include "space.h"

namespace {

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

extern "C" {

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
    if ((e = reserve(s->batch.b_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_flags, n))) return e;
    if ((e = reserve(s->batch.b_lookups, n))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    if ((e = smplx_cc_state_valid_batch_device(s, s->batch.b_q.p, n, s->b_flags.p, s->batch.b_lookups.p, s->stream))) return e;
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
    if ((e = reserve(s->batch.b_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_q2, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_flags, n))) return e;
    if ((e = reserve(s->batch.b_lookups, n))) return e;
    if ((e = reserve(s->b_way, n))) return e;
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
    if ((e = reserve(s->batch.b_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_sq, cnt))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_SPHERE_POSITIONS, k_sphere_positions, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes, s->stream,
                       s->d_space, s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->b_sq.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
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
    if ((e = reserve(s->batch.b_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_sq, cnt))) return e;
    HIP_TRY(hipMemcpyAsync(s->batch.b_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_ATTACHED_POSITIONS, k_attached_positions, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes, s->stream,
            s->d_space, s->batch.b_q.p, n, s->b_sq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, s->b_sq.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// ---- clearance: distance to collision (include/smpl_amd.h; kernels: clearance_kernels.h)

int smplx_cc_state_clearance_batch(smplx_space* s, const double* q, int n, double* clearance, double* parts, int32_t* witness)
{
    if (!s || !q || !clearance || n < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!sane_values(q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (s->lds_bytes_clearance > 160 * 1024) return set_error(SMPLX_E_LIMIT, kClearanceLds);
    int e;
    if ((e = reserve(s->b_clr_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_clr_out, (size_t)n * 3))) return e;
    if ((e = reserve(s->b_clr_wit, (size_t)n * 4))) return e;
    HIP_TRY(hipMemcpyAsync(s->b_clr_q.p, q, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    if ((e = smplx_cc_state_clearance_batch_device(s, s->b_clr_q.p, n, s->b_clr_out.p, s->b_clr_out.p + n, s->b_clr_wit.p, s->stream))) return e;
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
    if ((e = reserve(s->b_clr_q, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_clr_q2, (size_t)n * s->N))) return e;
    if ((e = reserve(s->b_clr_out, (size_t)n * 3))) return e;
    if ((e = reserve(s->b_clr_wit, (size_t)n * 4))) return e;
    HIP_TRY(hipMemcpyAsync(s->b_clr_q.p, a, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->b_clr_q2.p, b, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    KLAUNCH(s, K_EDGE_CLEARANCE, k_edge_clearance, dim3(blocks_for(n, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->lds_bytes_clearance, s->stream,
            s->d_space, s->b_clr_q.p, s->b_clr_q2.p, n, s->params.padding, s->b_clr_out.p, s->b_clr_out.p + n, s->b_clr_wit.p);
    HIP_TRY(hipGetLastError());
    return clearance_results(s, n, clearance, parts, witness);
}

}  // extern "C"
