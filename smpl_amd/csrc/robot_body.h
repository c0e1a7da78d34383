// smpl_amd/csrc/robot_body.h -- the robot body record (include/smpl_amd.h "robot body"): the body text's parser, the
// kinematics of every link and the dirtiness of the voxels states.  Host only: nothing here makes a HIP call, so the host
// compiler builds it for tests/cpp/robot_body_host_driver.cpp as it builds voxelize.h for voxelize_host_driver.cpp.
// What it stands behind: RobotCollisionModel's link / joint tree and CollisionVoxelsModels
// (sbpl_collision_checking/src/robot_collision_model.cpp:117-623, 566-573), RobotCollisionState::setJointVarPosition and
// its dirtying of descendant voxels states (src/robot_collision_state.cpp:62-96), the joint transforms of
// src/transform_functions.h:95-258 and the group's outside voxels states (robot_collision_state.cpp:297-314).
//
// Arithmetic: binary64, no fused multiply-add, smplx_sincos for every sine and cosine.  The origin
// matrix, the joint forms and the product T_parent * J are the expressions of model_compile.cpp (origin_matrix) and
// model_lds.h (joint_matrix, mul_affine), so a body link and a group link under the same ancestors get the same bits.
#pragma once

#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/smpl_amd.h"
#include "det_math.h"

namespace smplx_body_host {

enum { JT_FIXED = 0, JT_REVOLUTE = 1, JT_CONTINUOUS = 2, JT_PRISMATIC = 3 };
enum { TK_FIXED = 0, TK_REV_X = 1, TK_REV_Y = 2, TK_REV_Z = 3, TK_REV_GENERIC = 4, TK_PRISMATIC = 5 };

struct BodyJoint {
    std::string name;
    int type = JT_FIXED, kind = TK_FIXED;
    int parent = -1, child = -1;      // link indices
    double axis[3] = {0, 0, 1};
    double origin[12];
    double lo = 0, hi = 0;
    double q = 0;
};

struct BodyGeom {
    int link = -1;
    int type = 0;                     // SMPLX_SHAPE_BOX / SPHERE / CYLINDER / MESH
    double dims[3] = {0, 0, 0};
    double origin[12];                // the <collision> element's origin in the link frame, 3x4
    std::vector<double> v;            // MESH only
    std::vector<int> t;
};

struct BodyModel {
    int link = -1;
    double res = 0;
    bool outside = true;              // the link is not in the group row: the model is placed
};

struct Body {
    std::string name;
    std::vector<std::string> links;
    std::vector<int> parent_joint;    // per link, -1 for a root
    std::vector<int> order;           // links, parents before children
    std::vector<BodyJoint> joints;
    std::vector<BodyGeom> geoms;      // file order
    std::vector<BodyModel> models;    // file order of the voxels rows
    std::vector<int> link_model;      // per link, -1 without a voxels row
    std::vector<unsigned char> dirty; // per model
};

// urdf origin: Translation(xyz) * Rz(yaw) * Ry(pitch) * Rx(roll)  (model_compile.cpp origin_matrix)
inline void origin_matrix(const double xyz[3], const double rpy[3], double o[12])
{
    double sr, cr, sp, cp, sy, cy;
    smplx_sincos(rpy[0], &sr, &cr);
    smplx_sincos(rpy[1], &sp, &cp);
    smplx_sincos(rpy[2], &sy, &cy);
    o[0] = cy * cp; o[1] = (cy * sp) * sr - sy * cr; o[2] = (cy * sp) * cr + sy * sr; o[3] = xyz[0];
    o[4] = sy * cp; o[5] = (sy * sp) * sr + cy * cr; o[6] = (sy * sp) * cr - cy * sr; o[7] = xyz[1];
    o[8] = -sp;     o[9] = cp * sr;                  o[10] = cp * cr;                 o[11] = xyz[2];
}

// local transform of a joint: origin * R(q)  (transform_functions.h:95-258; model_lds.h joint_matrix)
inline void joint_matrix(const BodyJoint& j, double q, double J[12])
{
    const double* o = j.origin;
    if (j.kind == TK_FIXED) { std::memcpy(J, o, sizeof(double) * 12); return; }
    if (j.kind == TK_PRISMATIC) {     // translates along local Z whatever the axis (:218-226)
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0]; J[4 * i + 1] = o[4 * i + 1]; J[4 * i + 2] = o[4 * i + 2];
            J[4 * i + 3] = ((o[4 * i + 0] * 0.0 + o[4 * i + 1] * 0.0) + o[4 * i + 2] * q) + o[4 * i + 3];
        }
        return;
    }
    double s, c;
    smplx_sincos(q, &s, &c);
    if (j.kind == TK_REV_X) {
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0];
            J[4 * i + 1] = c * o[4 * i + 1] + s * o[4 * i + 2];
            J[4 * i + 2] = c * o[4 * i + 2] - s * o[4 * i + 1];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else if (j.kind == TK_REV_Y) {
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = c * o[4 * i + 0] - s * o[4 * i + 2];
            J[4 * i + 1] = o[4 * i + 1];
            J[4 * i + 2] = s * o[4 * i + 0] + c * o[4 * i + 2];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else if (j.kind == TK_REV_Z) {
        for (int i = 0; i < 3; ++i) {
            J[4 * i + 0] = o[4 * i + 0] * c + o[4 * i + 1] * s;
            J[4 * i + 1] = o[4 * i + 1] * c - o[4 * i + 0] * s;
            J[4 * i + 2] = o[4 * i + 2];
            J[4 * i + 3] = o[4 * i + 3];
        }
    } else {                          // generic axis: o * AngleAxis(q, axis)  (Eigen toRotationMatrix restated)
        const double ax = j.axis[0], ay = j.axis[1], az = j.axis[2];
        const double sx = s * ax, sy = s * ay, sz = s * az;
        const double c1 = 1.0 - c;
        const double cx = c1 * ax, cy = c1 * ay, cz = c1 * az;
        double R[9];
        double tmp;
        tmp = cx * ay; R[1] = tmp - sz; R[3] = tmp + sz;
        tmp = cx * az; R[2] = tmp + sy; R[6] = tmp - sy;
        tmp = cy * az; R[5] = tmp - sx; R[7] = tmp + sx;
        R[0] = cx * ax + c; R[4] = cy * ay + c; R[8] = cz * az + c;
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) J[4 * i + k] = (o[4 * i + 0] * R[k] + o[4 * i + 1] * R[3 + k]) + o[4 * i + 2] * R[6 + k];
            J[4 * i + 3] = o[4 * i + 3];
        }
    }
}

// out = T * J  (robot_collision_state.h:419-421; model_lds.h mul_affine)
inline void mul_affine(const double T[12], const double J[12], double out[12])
{
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) out[4 * i + k] = (T[4 * i + 0] * J[k] + T[4 * i + 1] * J[4 + k]) + T[4 * i + 2] * J[8 + k];
        out[4 * i + 3] = ((T[4 * i + 0] * J[3] + T[4 * i + 1] * J[7]) + T[4 * i + 2] * J[11]) + T[4 * i + 3];
    }
}

// world frames of all links, nlinks x 12: a root link's frame is the world's; a joint on a root link gives T = J
inline void link_transforms(const Body& b, double* T)
{
    for (int l : b.order) {
        double* out = T + 12 * (size_t)l;
        const int pj = b.parent_joint[(size_t)l];
        if (pj < 0) {
            for (int i = 0; i < 12; ++i) out[i] = (i % 5 == 0) ? 1.0 : 0.0;
            continue;
        }
        const BodyJoint& j = b.joints[(size_t)pj];
        double J[12];
        joint_matrix(j, j.q, J);
        if (b.parent_joint[(size_t)j.parent] < 0) std::memcpy(out, J, sizeof(J));
        else mul_affine(T + 12 * (size_t)j.parent, J, out);
    }
}

inline bool finite_number(double v) { return v > -1.0e6 && v < 1.0e6; }   // also refuses NaN

inline int find_joint(const Body& b, const char* name)
{
    for (size_t i = 0; i < b.joints.size(); ++i)
        if (b.joints[i].name == name) return (int)i;
    return -1;
}

// setJointVarPosition (robot_collision_state.cpp:62-96): a value different from the current one dirties the voxels states
// of the joint's child link and of all its descendants; the same value dirties nothing.  Returns SMPLX_OK or SMPLX_E_ARG.
inline int set_joint(Body& b, const char* name, double q, std::string& err)
{
    const int j = name ? find_joint(b, name) : -1;
    if (j < 0) { err = std::string("no joint named ") + (name ? name : "(null)"); return SMPLX_E_ARG; }
    if (b.joints[(size_t)j].type == JT_FIXED) { err = std::string("joint ") + name + " is fixed: it has no value"; return SMPLX_E_ARG; }
    if (!finite_number(q)) { err = "joint values must be finite (|x| < 1e6)"; return SMPLX_E_ARG; }
    if (b.joints[(size_t)j].q == q) return SMPLX_OK;
    b.joints[(size_t)j].q = q;
    std::vector<unsigned char> moved(b.links.size(), 0);
    for (int l : b.order) {
        const int pj = b.parent_joint[(size_t)l];
        if (pj < 0) continue;
        if (pj == j || moved[(size_t)b.joints[(size_t)pj].parent]) {
            moved[(size_t)l] = 1;
            if (b.link_model[(size_t)l] >= 0) b.dirty[(size_t)b.link_model[(size_t)l]] = 1;
        }
    }
    return SMPLX_OK;
}

// Parses a body text.  SMPLX_OK, or SMPLX_E_ARG / SMPLX_E_LIMIT with err = "line N: ..." where a row is at fault.
inline int parse_body_text(const char* text, Body& b, std::string& err)
{
    b = Body();
    struct Pending { std::string a, b2; double v; int line; };
    std::vector<Pending> joint_links, geom_links, voxel_rows, values;
    std::vector<std::string> group;
    std::istringstream in(text);
    std::string line;
    int lineno = 0;
    int want_v = 0, want_t = 0;        // rows of the mesh being read
    auto fail = [&](int ln, const std::string& s, int code = SMPLX_E_ARG) { err = "line " + std::to_string(ln) + ": " + s; return code; };
    auto numbers = [&](std::istringstream& ls, double* out, int n) {
        for (int i = 0; i < n; ++i)
            if (!(ls >> out[i]) || !finite_number(out[i])) return false;
        return true;
    };
    auto ended = [&](std::istringstream& ls) { std::string extra; return !(ls >> extra); };
    while (std::getline(in, line)) {
        ++lineno;
        const size_t h = line.find('#');
        if (h != std::string::npos) line.resize(h);
        std::istringstream ls(line);
        std::string kw;
        if (!(ls >> kw)) continue;
        if (want_v > 0 || want_t > 0) {
            BodyGeom& g = b.geoms.back();
            if (want_v > 0) {
                double p[3];
                if (kw != "v" || !numbers(ls, p, 3) || !ended(ls)) return fail(lineno, "expected a mesh vertex row \"v x y z\" with finite numbers (|x| < 1e6)");
                g.v.insert(g.v.end(), p, p + 3);
                --want_v;
            } else {
                long long a[3];
                if (kw != "t" || !(ls >> a[0] >> a[1] >> a[2]) || !ended(ls)) return fail(lineno, "expected a mesh triangle row \"t a b c\"");
                for (long long x : a) {
                    if (x < 0 || x >= (long long)(g.v.size() / 3)) return fail(lineno, "triangle index outside the mesh's vertices");
                    g.t.push_back((int)x);
                }
                --want_t;
            }
            continue;
        }
        if (kw == "robot") {
            if (!(ls >> b.name) || !ended(ls)) return fail(lineno, "robot needs one name");
        } else if (kw == "link") {
            std::string n;
            if (!(ls >> n) || !ended(ls)) return fail(lineno, "link needs one name");
            for (const std::string& l : b.links)
                if (l == n) return fail(lineno, "link " + n + " is listed twice");
            if (b.links.size() >= (size_t)SMPLX_BODY_MAX_LINKS) return fail(lineno, "more links than SMPLX_BODY_MAX_LINKS", SMPLX_E_LIMIT);
            b.links.push_back(n);
        } else if (kw == "joint") {
            BodyJoint j;
            std::string type, parent, child;
            if (!(ls >> j.name >> type >> parent >> child)) return fail(lineno, "malformed joint row");
            if (type == "fixed") j.type = JT_FIXED;
            else if (type == "revolute") j.type = JT_REVOLUTE;
            else if (type == "continuous") j.type = JT_CONTINUOUS;
            else if (type == "prismatic") j.type = JT_PRISMATIC;
            else return fail(lineno, "unknown joint type " + type + " (planar and floating joints are not supported)");
            double n[11];
            if (!numbers(ls, n, 11) || !ended(ls)) return fail(lineno, "a joint row needs 11 finite numbers (|x| < 1e6): x y z  r p y  ax ay az  lo hi");
            for (const BodyJoint& o : b.joints)
                if (o.name == j.name) return fail(lineno, "joint " + j.name + " is listed twice");
            origin_matrix(n, n + 3, j.origin);
            for (int a = 0; a < 3; ++a) j.axis[a] = n[6 + a];
            j.lo = n[9]; j.hi = n[10];
            const double* a = j.axis;
            if (j.type == JT_FIXED) j.kind = TK_FIXED;
            else if (j.type == JT_PRISMATIC) j.kind = TK_PRISMATIC;
            else if (a[0] == 1.0 && a[1] == 0.0 && a[2] == 0.0) j.kind = TK_REV_X;   // robot_collision_model.cpp:331-407
            else if (a[0] == 0.0 && a[1] == 1.0 && a[2] == 0.0) j.kind = TK_REV_Y;
            else if (a[0] == 0.0 && a[1] == 0.0 && a[2] == 1.0) j.kind = TK_REV_Z;
            else j.kind = TK_REV_GENERIC;
            b.joints.push_back(j);
            joint_links.push_back({parent, child, 0.0, lineno});
        } else if (kw == "geom") {
            BodyGeom g;
            std::string link, shape;
            if (!(ls >> link >> shape)) return fail(lineno, "malformed geom row");
            int nd = 0;
            long long nv = 0, nt = 0;
            if (shape == "box") { g.type = SMPLX_SHAPE_BOX; nd = 3; }
            else if (shape == "sphere") { g.type = SMPLX_SHAPE_SPHERE; nd = 1; }
            else if (shape == "cylinder") { g.type = SMPLX_SHAPE_CYLINDER; nd = 2; }
            else if (shape == "mesh") { g.type = SMPLX_SHAPE_MESH; nd = 0; }
            else return fail(lineno, "unknown geom shape " + shape + " (box, sphere, cylinder, mesh)");
            if (g.type == SMPLX_SHAPE_MESH) {
                if (!(ls >> nv >> nt)) return fail(lineno, "a mesh geom needs its vertex and triangle counts");
                if (nv < 1 || nt < 1) return fail(lineno, "a mesh needs vertices and triangles");
                if (nv > SMPLX_BODY_MAX_MODEL_POINTS || nt > SMPLX_BODY_MAX_MODEL_POINTS) return fail(lineno, "mesh too large", SMPLX_E_LIMIT);
            } else if (!numbers(ls, g.dims, nd)) {
                return fail(lineno, "geom dimensions must be finite numbers (|x| < 1e6)");
            }
            for (int k = 0; k < nd; ++k)
                if (!(g.dims[k] > 0.0)) return fail(lineno, "geom dimensions must be positive");
            double o[6];
            if (!numbers(ls, o, 6) || !ended(ls)) return fail(lineno, "a geom row ends with its origin: x y z  r p y, finite (|x| < 1e6)");
            origin_matrix(o, o + 3, g.origin);
            b.geoms.push_back(g);
            geom_links.push_back({link, "", 0.0, lineno});
            want_v = (int)nv; want_t = (int)nt;
        } else if (kw == "voxels") {
            std::string link;
            double res;
            if (!(ls >> link) || !numbers(ls, &res, 1) || !ended(ls)) return fail(lineno, "a voxels row is \"voxels LINK RES\" with a finite RES");
            if (!(res > 0.0)) return fail(lineno, "the resolution of a voxels model must be positive");
            voxel_rows.push_back({link, "", res, lineno});
        } else if (kw == "group") {
            std::string n, l;
            if (!(ls >> n)) return fail(lineno, "group needs a name");
            while (ls >> l) group.push_back(l);
        } else if (kw == "value") {
            std::string jn;
            double q;
            if (!(ls >> jn) || !numbers(ls, &q, 1) || !ended(ls)) return fail(lineno, "a value row is \"value JOINT Q\" with a finite Q (|x| < 1e6)");
            values.push_back({jn, "", q, lineno});
        } else {
            return fail(lineno, "unknown keyword " + kw);
        }
    }
    if (want_v > 0 || want_t > 0) return fail(lineno, "the text ends inside a mesh");
    if (b.links.empty()) { err = "no links"; return SMPLX_E_ARG; }
    auto link_index = [&](const std::string& n) {
        for (size_t i = 0; i < b.links.size(); ++i)
            if (b.links[i] == n) return (int)i;
        return -1;
    };
    const int nl = (int)b.links.size();
    b.parent_joint.assign((size_t)nl, -1);
    for (size_t j = 0; j < b.joints.size(); ++j) {
        BodyJoint& J = b.joints[j];
        J.parent = link_index(joint_links[j].a);
        J.child = link_index(joint_links[j].b2);
        if (J.parent < 0 || J.child < 0) return fail(joint_links[j].line, "joint " + J.name + " names an unknown link");
        if (b.parent_joint[(size_t)J.child] >= 0) return fail(joint_links[j].line, "link " + b.links[(size_t)J.child] + " has two parent joints");
        b.parent_joint[(size_t)J.child] = (int)j;
    }
    // parents before children; a link that is never reached hangs on a cycle
    std::vector<std::vector<int>> children((size_t)nl);
    for (const BodyJoint& J : b.joints) children[(size_t)J.parent].push_back(J.child);
    for (int l = 0; l < nl; ++l)
        if (b.parent_joint[(size_t)l] < 0) b.order.push_back(l);
    for (size_t head = 0; head < b.order.size(); ++head)
        for (int c : children[(size_t)b.order[head]]) b.order.push_back(c);
    if ((int)b.order.size() != nl) { err = "the joints form a cycle"; return SMPLX_E_ARG; }
    for (size_t i = 0; i < b.geoms.size(); ++i) {
        b.geoms[i].link = link_index(geom_links[i].a);
        if (b.geoms[i].link < 0) return fail(geom_links[i].line, "geom on unknown link " + geom_links[i].a);
    }
    b.link_model.assign((size_t)nl, -1);
    for (const Pending& v : voxel_rows) {
        const int l = link_index(v.a);
        if (l < 0) return fail(v.line, "voxels on unknown link " + v.a);
        if (b.link_model[(size_t)l] >= 0) return fail(v.line, "link " + v.a + " has two voxels rows");
        BodyModel m;
        m.link = l; m.res = v.v;
        b.link_model[(size_t)l] = (int)b.models.size();
        b.models.push_back(m);
    }
    for (const std::string& gname : group) {
        const int l = link_index(gname);
        if (l < 0) { err = "group names an unknown link " + gname; return SMPLX_E_ARG; }
        if (b.link_model[(size_t)l] >= 0) b.models[(size_t)b.link_model[(size_t)l]].outside = false;
    }
    for (const Pending& v : values) {
        const int j = find_joint(b, v.a.c_str());
        if (j < 0) return fail(v.line, "value for unknown joint " + v.a);
        if (b.joints[(size_t)j].type == JT_FIXED) return fail(v.line, "joint " + v.a + " is fixed: it has no value");
        b.joints[(size_t)j].q = v.v;
    }
    b.dirty.assign(b.models.size(), 1);   // every state starts dirty
    return SMPLX_OK;
}

}  // namespace smplx_body_host
