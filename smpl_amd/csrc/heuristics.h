// smpl_amd/csrc/heuristics.h -- the closed-form heuristics, EuclidDistHeuristic and JointDistHeuristic, as host and device
// inline functions: the C-ABI's host calls (smplx_pose_distance, smplx_joint_distance; engine.hip) and every kernel
// (lattice_steps.h) compile this same text, so a state's h is the same integer on both sides (det_math.h, DESIGN.md
// section 3: the same IEEE operations in the same order, no contraction, no libm or ocml).
// Owns: smplx_rotation_angle, smplx_pose_dist, smplx_point_dist, smplx_joint_dist, smplx_fixed_h.
// Restates: euclid_dist_heuristic.cpp:46-55, 98-102, 244-272; joint_dist_heuristic.cpp:126-136.
//
// The orientation term.  The reference turns both rotations into quaternions -- the state's from its rotation matrix, the
// goal's from the goal's roll, pitch and yaw, which for a joint goal went through KDL's GetRPY first -- and takes
// theta = 2 acos |qa . qb|.  The engine holds rotation matrices, so it takes the same angle from the identity
// 4 cos^2(theta / 2) = 1 + trace(Rb^T Ra): cos(theta / 2) = sqrt(max(0, 1 + trace)) / 2, clamped to 1, theta in [0, pi]
// (the relation the pose goal's orientation test uses, lattice_steps.h successor_goal_h).  Parity with the reference's
// Euler round trip (KDL GetRPY, Eigen's matrix-to-quaternion) is unpinned: the two agree as real numbers, their last
// bits are not compared anywhere -- as for pose goals.
#pragma once

#include "det_math.h"

// angle between two rotations (row-major 3x3), in [0, pi]
SMPLX_HD double smplx_rotation_angle(const double* Ra, const double* Rb)
{
    double t = 1.0;
    for (int i = 0; i < 9; ++i) t += Rb[i] * Ra[i];
    double c = 0.5 * sqrt(t > 0.0 ? t : 0.0);
    if (c > 1.0) c = 1.0;
    return 2.0 * smplx_acos(c);
}

// EuclidDistHeuristic::computeDistance (euclid_dist_heuristic.cpp:244-272) from the pose (pa, Ra) to the pose (pb, Rb):
// sqrt(wx dx^2 + wy dy^2 + wz dz^2 + wr theta^2), summed in the reference's order
SMPLX_HD double smplx_pose_dist(const double* pa, const double* Ra, const double* pb, const double* Rb, const double* w)
{
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2];
    const double dp2 = (w[0] * (dx * dx) + w[1] * (dy * dy)) + w[2] * (dz * dz);
    double dr2 = smplx_rotation_angle(Ra, Rb);
    dr2 *= (w[3] * dr2);
    return sqrt(dp2 + dr2);
}

// EuclidDistHeuristic::getMetricGoalDistance (:46-55, 98-102): the plain distance from p to the goal position g
SMPLX_HD double smplx_point_dist(const double* p, const double* g)
{
    const double dx = g[0] - p[0], dy = g[1] - p[1], dz = g[2] - p[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// JointDistHeuristic::computeJointDistance (joint_dist_heuristic.cpp:126-136): raw joint values, variable order, no
// angle wrapping
SMPLX_HD double smplx_joint_dist(const double* a, const double* b, int n)
{
    double dsum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double dj = a[i] - b[i];
        dsum += dj * dj;
    }
    return sqrt(dsum);
}

// (int)(FIXED_POINT_RATIO * dist) (euclid_dist_heuristic.h:72, joint_dist_heuristic.h:67: 1000.0).  The reference's
// conversion has no defined value beyond the int range; here such a distance (over two thousand kilometres or radians)
// gives INT_MAX on both sides.
SMPLX_HD int smplx_fixed_h(double dist)
{
    const double v = 1000.0 * dist;
    return v >= 2147483647.0 ? 2147483647 : (int)v;
}
