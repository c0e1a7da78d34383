// smpl_amd/csrc/attached_host.h -- collision bodies attached to robot links (AttachedBodies in space.h; the kernels'
// side is attached_bodies.h): the builder of their device image, the checks every attach starts with, and the entry
// points that attach by spheres or by shape, detach, and list what is attached.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "model_compile.h"
#include "space.h"

// field.hip owns the voxeliser: the sphere rows of an object attached by shape (object_sphere_rows.h)
extern "C" int smplx_internal_object_spheres(WorkSpace* work, const smplx_shape* shapes, int n, double radius, std::vector<double>* rows,
                                             std::vector<int32_t>* first);

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
    if (!s->att.d_bodies) HIP_TRY(s->att.d_bodies.alloc(1));
    // kernels in flight may still read the old image, on the space's stream or on a caller's (the _device entry points)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyAsync(s->att.d_bodies, img.get(), sizeof(SmplxBodiesDev), hipMemcpyHostToDevice, s->stream));
    s->hs.bodies = s->att.bodies.empty() ? nullptr : s->att.d_bodies.p;
    HIP_TRY(hipMemcpyAsync((unsigned char*)s->d_space.p + offsetof(SmplxSpaceDev, bodies), &s->hs.bodies, sizeof(s->hs.bodies),
                           hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

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

extern "C" {

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
        HIP_TRY(hipMemcpy(nodes.data(), s->att.d_bodies.p->nodes, sizeof(SmplxNode) * nn, hipMemcpyDeviceToHost));
        for (int i = 0; i < nn; ++i) {
            if (xyzr) for (int k = 0; k < 3; ++k) xyzr[4 * i + k] = nodes[i].c[k];
            if (xyzr) xyzr[4 * i + 3] = nodes[i].r;
            if (left) left[i] = nodes[i].left;
            if (right) right[i] = nodes[i].right;
        }
    }
    return nn;
}

}  // extern "C"
