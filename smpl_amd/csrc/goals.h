// smpl_amd/csrc/goals.h -- setting the goal of a space (GoalHost in space.h, the device's record in hs.goal): the records of
// a joint, a position and a pose goal, the three steps every goal is set in, for one space or for many at once, and the
// entry points that set a goal or read it back.
#pragma once

#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "bfs_host.h"
#include "det_math.h"
#include "heuristic_host.h"
#include "multi_query.h"
#include "space.h"

namespace {

// A goal is set in three steps, shared by the single-goal entry points (finish_goal) and the multi-goal ones
// (finish_goals_multi): begin_goal -- the goal position into the device record, the tag of this goal's BFS run, the
// upload; the BFS (run_bfs / run_bfs_multi); end_goal -- the goal stands, the query starts over.
int begin_goal(smplx_space* s)
{
    for (int a = 0; a < 3; ++a) s->hs.goal.xyz[a] = s->goal.xyz[a];
    if (closed_form(s)) {
        // what the closed form needs of the goal (device_types.h SmplxHeurDev); there is no BFS run to tag
        SmplxHeurDev& H = s->hs.heur;
        H.joint_goal = s->hs.goal.type == SMPLX_GOAL_JOINT ? 1 : 0;
        for (int a = 0; a < 3; ++a) H.xyz[a] = s->goal.xyz[a];
        for (int k = 0; k < 9; ++k) H.rot[k] = s->goal.rot[k];
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

void end_goal(smplx_space* s)
{
    s->goal.set = true;
    s->goal.grid_epoch = s->grid->epoch;
    s->att.epoch_goal = s->att.epoch;
    // a new goal starts a new query: the state table restarts (ids are per query)
    reset_lattice(s);
    // heuristic of the goal id = BFS cost at the goal pose's cell (manip_lattice.cpp:1176-1190); the closed forms give the
    // goal id 0 outright (euclid_dist_heuristic.cpp:120-122, joint_dist_heuristic.cpp:72-74)
    int c[3];
    s->lat.h_of_id[0] = closed_form(s) || bfs_goal_cell(s, s->goal.xyz, c) ? 0 : 32767;   // the seeded cell has distance 0 (bfs3d.cpp:178)
}

int finish_goal(smplx_space* s)
{
    if (int e = begin_goal(s)) return e;
    if (!closed_form(s))
        if (int e = run_bfs(s, s->goal.xyz)) return e;
    end_goal(s);
    return SMPLX_OK;
}

// the goal record of a joint goal, all but the goal pose (planner_interface.cpp:1232-1235 takes it from the FK)
void joint_goal_record(smplx_space* s, const double* angles, const double* tolerances)
{
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_JOINT;
    for (int v = 0; v < s->N; ++v) { G.angles[v] = angles[v]; G.angle_tol[v] = tolerances[v]; }
    state_to_coord(s->model.dev, angles, G.coord);
}

void xyz_goal_record(smplx_space* s, const double xyz[3], const double tol[3])
{
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_XYZ;
    for (int a = 0; a < 3; ++a) { s->goal.xyz[a] = xyz[a]; G.xyz_tol[a] = tol[a]; }
    // the Euclidean heuristic's goal rotation: the identity, what the reference makes of the pose {x, y, z, 0, 0, 0}
    for (int k = 0; k < 9; ++k) s->goal.rot[k] = k % 4 == 0 ? 1.0 : 0.0;
}

// the bound of the device's orientation test (device_types.h SmplxGoalDev::rpy_c4): theta < tol, theta in [0, pi], is
// 4 cos^2(theta / 2) > 4 cos^2(tol / 2) for 0 < tol <= pi; a wider tolerance admits every orientation, tol <= 0 none
double rpy_bound(double tol)
{
    if (!(tol > 0.0)) return std::numeric_limits<double>::infinity();
    if (tol > SMPLX_PI) return -1.0;
    const double c = std::cos(0.5 * tol);
    return 4.0 * c * c;
}

// Rz(yaw) Ry(pitch) Rx(roll), row-major 3x3: origin_matrix (model_compile.cpp) without the translation
void rpy_matrix(const double rpy[3], double r[9])
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
void pose_goal_record(smplx_space* s, const double xyz[3], const double rpy[3], const double xyz_tol[3], double rpy_tol)
{
    xyz_goal_record(s, xyz, xyz_tol);
    SmplxGoalDev& G = s->hs.goal;
    G.type = SMPLX_GOAL_XYZ_RPY;
    rpy_matrix(rpy, G.rot);
    for (int k = 0; k < 9; ++k) s->goal.rot[k] = G.rot[k];
    G.rpy_c4 = rpy_bound(rpy_tol);
    for (int a = 0; a < 3; ++a) s->goal.rpy[a] = rpy[a];
    s->goal.rpy_tol = rpy_tol;
}

// what the pose-goal entry points refuse in n goals: a non-finite pose, |xyz| >= 1e6 or |rpy| >= 1e6 (smplx_sincos reduces
// its argument through an int: the bound of the joint values), a NaN tolerance
bool sane_pose_goals(const double* xyz, const double* rpy, const double* xyz_tol, const double* rpy_tol, size_t n)
{
    if (!sane_values(xyz, 3 * n) || !sane_values(rpy, 3 * n)) return false;
    for (size_t i = 0; i < 3 * n; ++i) if (std::isnan(xyz_tol[i])) return false;
    for (size_t i = 0; i < n; ++i) if (std::isnan(rpy_tol[i])) return false;
    return true;
}

// the Euclidean heuristic's goal rotation under a joint goal: the planning link's at the goal angles
// (planner_interface.cpp:1236-1238), by the FK that gave the goal position
int joint_goal_rotation(smplx_space* s, const double* angles)
{
    if (s->params.heuristic != SMPLX_H_EUCLID) return SMPLX_OK;
    double T[12];
    if (int e = smplx_planning_pose_batch(s, angles, 1, T)) return e;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) s->goal.rot[3 * r + c] = T[4 * r + c];
    return SMPLX_OK;
}

// what the multi-goal entry points check before they touch a space: the array, no space twice (on the handles alone)
int check_goal_spaces(smplx_space* const* spaces, int nq)
{
    if (!spaces || nq < 1) return set_error(SMPLX_E_ARG, "bad argument");
    for (int q = 0; q < nq; ++q) if (!spaces[q]) return set_error(SMPLX_E_ARG, "null space");
    for (int q = 0; q < nq; ++q)
        for (int r = 0; r < q; ++r)
            if (spaces[q] == spaces[r]) return set_error(SMPLX_E_ARG, "a space appears twice");
    return SMPLX_OK;
}

// ... and on the spaces: one device, the same bricks per axis (the goals share the launches of run_bfs_multi)
int check_goal_spaces_match(smplx_space* const* spaces, int nq)
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
int finish_goals_multi(smplx_space* const* spaces, int nq)
{
    int e = SMPLX_OK;
    for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = begin_goal(spaces[q]);
    // the shared sweep is of the spaces that plan with the BFS; a closed-form space has its goal from begin_goal alone
    std::vector<smplx_space*> with_bfs;
    for (int q = 0; q < nq; ++q) if (!closed_form(spaces[q])) with_bfs.push_back(spaces[q]);
    if (e == SMPLX_OK && !with_bfs.empty()) e = run_bfs_multi(with_bfs.data(), (int)with_bfs.size());
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) spaces[q]->goal.set = false;   // some grids are half written: no space keeps a goal
        return e;
    }
    for (int q = 0; q < nq; ++q) end_goal(spaces[q]);
    return SMPLX_OK;
}

}  // namespace

extern "C" {

int smplx_set_goal_joint(smplx_space* s, const double* angles, const double* tolerances)
{
    if (!s || !angles || !tolerances) return set_error(SMPLX_E_ARG, "null argument");
    if (!sane_values(angles, s->N)) return set_error(SMPLX_E_ARG, "goal angles must be finite (|q| < 1e6)");
    joint_goal_record(s, angles, tolerances);
    // goal pose = planning-link FK of the goal angles (planner_interface.cpp:1232-1235)
    int32_t h;
    if (int e = run_heuristic(s, angles, 1, &h, s->goal.xyz)) return e;
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
        for (int q = 0; q < nq && e == SMPLX_OK; ++q) for (int a = 0; a < 3; ++a) spaces[q]->goal.xyz[a] = xyz[(size_t)q * 3 + a];
    } else {
        for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = run_heuristic(spaces[q], angles + (size_t)q * N, 1, nullptr, spaces[q]->goal.xyz);
    }
    for (int q = 0; q < nq && e == SMPLX_OK; ++q) e = joint_goal_rotation(spaces[q], angles + (size_t)q * N);
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) spaces[q]->goal.set = false;
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
    if (!s->goal.set || s->hs.goal.type != SMPLX_GOAL_XYZ_RPY) return set_error(SMPLX_E_STATE, "the goal is not a pose goal");
    for (int a = 0; a < 3; ++a) rpy[a] = s->goal.rpy[a];
    *rpy_tol = s->goal.rpy_tol;
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

int smplx_goal_pose(const smplx_space* s, double xyz[3])
{
    if (!s || !xyz) return set_error(SMPLX_E_ARG, "null argument");
    for (int a = 0; a < 3; ++a) xyz[a] = s->goal.xyz[a];
    return SMPLX_OK;
}

int smplx_test_goal_rotation(const smplx_space* s, double R[9])
{
    if (!s || !R) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
    for (int k = 0; k < 9; ++k) R[k] = s->goal.rot[k];
    return SMPLX_OK;
}

}  // extern "C"
