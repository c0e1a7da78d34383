// tests/cpp/attach_object_driver.cpp -- attaches an object by shape through smpl_amd::GpuCollisionChecker
// (include/smpl_amd/plugin.hpp): attachObject(id, shapes, transforms, link), processAttachedCollisionObject and
// detachObject.  object.txt: the link, the touch links, the edges of a box, its pose in the link's frame (12 numbers)
// and a state that is free without the object and in collision with it.  Prints one line per step (the bool returns and
// isStateValid of that state); tests/test_gpu_attach_object_cpp.py compares them.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <smpl_amd/plugin.hpp>

using namespace smpl_amd;

static std::string slurp(const std::string& p)
{
    std::ifstream f(p);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::string robot = slurp(dir + "/robot.txt"), mprim = slurp(dir + "/mprim.txt");
    std::ifstream q(dir + "/query.txt");
    double origin[3], res, max_dist;
    int n[3], nv;
    smplx_params P = {};
    q >> origin[0] >> origin[1] >> origin[2] >> n[0] >> n[1] >> n[2] >> res >> max_dist >> nv;
    for (int i = 0; i < nv; ++i) q >> P.resolutions[i];
    q >> P.bfs_inflation_radius >> P.cost_per_cell >> P.use_short_dist_mprims >> P.short_dist_mprims_thresh >>
        P.use_xyzrpy_snap_mprim >> P.xyzrpy_snap_dist_thresh >> P.xy_rotate_by_var3 >> P.use_long_and_short;
    std::ifstream of(dir + "/object.txt");
    std::string link;
    int ntouch = 0;
    of >> link >> ntouch;
    std::vector<std::string> touch(ntouch);
    for (std::string& t : touch) of >> t;
    double edge[3];
    Pose pose;
    of >> edge[0] >> edge[1] >> edge[2];
    for (double& v : pose) of >> v;
    RobotState state(nv);
    for (double& v : state) of >> v;
    if (!of) return 3;
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuCollisionChecker cc(&ctx);
    const std::vector<Shape> shapes{Shape::Box(edge[0], edge[1], edge[2])};
    const std::vector<Pose> poses{pose};
    AttachedCollisionObject ao;
    ao.object.id = "crate";
    ao.object.shapes = shapes;
    ao.object.shape_poses = poses;
    ao.link_name = link;
    ao.touch_links = touch;

    bool ok = false;      // each call is made before the state is checked
    printf("free %d\n", (int)cc.isStateValid(state));
    ok = cc.attachObject("crate", shapes, poses, link, touch);
    printf("attach %d %d\n", (int)ok, (int)cc.isStateValid(state));
    printf("attach_mismatched %d\n", (int)cc.attachObject("other", shapes, std::vector<Pose>(), link, touch));
    printf("attach_again %d\n", (int)cc.attachObject("crate", shapes, poses, link, touch));
    printf("attach_unknown_link %d\n", (int)cc.attachObject("other", shapes, poses, "no_such_link"));
    ok = cc.detachObject("crate");
    printf("detach %d %d\n", (int)ok, (int)cc.isStateValid(state));
    printf("detach_again %d\n", (int)cc.detachObject("crate"));
    ao.operation = AttachedCollisionObject::ADD;
    ok = cc.processAttachedCollisionObject(ao);
    printf("process_add %d %d\n", (int)ok, (int)cc.isStateValid(state));
    printf("process_add_again %d\n", (int)cc.processAttachedCollisionObject(ao));
    ao.operation = AttachedCollisionObject::MOVE;
    printf("process_move %d\n", (int)cc.processAttachedCollisionObject(ao));
    ao.operation = AttachedCollisionObject::APPEND;
    printf("process_append %d\n", (int)cc.processAttachedCollisionObject(ao));
    ao.operation = AttachedCollisionObject::REMOVE;
    ok = cc.processAttachedCollisionObject(ao);
    printf("process_remove %d %d\n", (int)ok, (int)cc.isStateValid(state));
    printf("process_remove_again %d\n", (int)cc.processAttachedCollisionObject(ao));
    printf("done\n");
    return 0;
}
