"""Plain numpy references of the pose-goal tests: the planning link's transform from the robot description's joint
lines (a serial chain of origin * motion products, transform_functions.h:95-258), and the reference's orientation
distance (manip_lattice.cpp:1652-1665).  Nothing here calls the engine or the oracle."""
import numpy as np


def rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def rpy_matrix(rpy):
    """Rz(yaw) Ry(pitch) Rx(roll): URDF origins and the goal orientation alike"""
    return rot_z(rpy[2]) @ rot_y(rpy[1]) @ rot_x(rpy[0])


def axis_angle(axis, a):
    """Rodrigues' formula"""
    u = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


class Chain:
    """The joints between the root link and the planning link of a robot description (smpl_amd/scenes.py text form:
    `joint name type parent child  x y z  r p y  ax ay az  lo hi`, `planning_joints ...`, `planning_link L`)."""

    def __init__(self, robot_text):
        joints, planning, link = {}, [], None
        for line in robot_text.splitlines():
            w = line.split()
            if not w:
                continue
            if w[0] == "joint":
                v = [float(x) for x in w[5:16]]
                joints[w[4]] = dict(name=w[1], type=w[2], parent=w[3], xyz=v[0:3], rpy=v[3:6], axis=v[6:9])
            elif w[0] == "planning_joints":
                planning = w[1:]
            elif w[0] == "planning_link":
                link = w[1]
        self.nvars = len(planning)
        self.chain = []
        while link in joints:                   # child link -> its joint, up to the root
            j = joints[link]
            j["var"] = planning.index(j["name"]) if j["name"] in planning else -1
            self.chain.append(j)
            link = j["parent"]
        self.chain.reverse()

    def transform(self, q):
        """4x4 transform of the planning link at joint values q"""
        T = np.eye(4)
        for j in self.chain:
            O = np.eye(4)
            O[:3, :3] = rpy_matrix(j["rpy"])
            O[:3, 3] = j["xyz"]
            M = np.eye(4)
            a = q[j["var"]] if j["var"] >= 0 else 0.0
            if j["type"] in ("revolute", "continuous"):
                M[:3, :3] = axis_angle(j["axis"], a)
            elif j["type"] == "prismatic":      # along the joint frame's Z whatever the axis (transform_functions.h:218-226)
                M[2, 3] = a
            T = T @ O @ M
        return T

    def transforms(self, Q):
        return np.stack([self.transform(q) for q in np.asarray(Q, float).reshape(-1, self.nvars)])


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def rpy_quat(rpy):
    """AngleAxis(yaw, Z) * AngleAxis(pitch, Y) * AngleAxis(roll, X) as a quaternion (w, x, y, z)"""
    r, p, y = (0.5 * float(v) for v in rpy)
    qx = np.array([np.cos(r), np.sin(r), 0, 0])
    qy = np.array([np.cos(p), 0, np.sin(p), 0])
    qz = np.array([np.cos(y), 0, 0, np.sin(y)])
    return _quat_mul(_quat_mul(qz, qy), qx)


def rpy_angle(a, b):
    """2 acos(q . qg) with qg negated when the dot product is negative (manip_lattice.cpp:1660-1665)"""
    d = abs(float(np.dot(rpy_quat(a), rpy_quat(b))))
    return 2.0 * np.arccos(min(d, 1.0))


def rotation_angle(Ra, Rb):
    """the angle of Ra^T Rb in [0, pi]: what rpy_angle is for the rotations the two triples recompose to.  atan2 of
    the sine (norm of the skew part) and the cosine (trace): well conditioned at both ends of the range"""
    D = Ra.T @ Rb
    s = 0.5 * np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    c = 0.5 * (np.trace(D) - 1.0)
    return float(np.arctan2(s, c))


def matrix_rpy(R):
    """roll, pitch, yaw with R = Rz(yaw) Ry(pitch) Rx(roll) (away from pitch = +-pi/2)"""
    return np.array([np.arctan2(R[2, 1], R[2, 2]), -np.arcsin(np.clip(R[2, 0], -1.0, 1.0)), np.arctan2(R[1, 0], R[0, 0])])
