// tests/cpp/world_objects_driver.cpp -- world objects through smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp):
// insertObject, moveShapes, insertShapes, removeShapes and both removeObject overloads on a context with an editable
// grid.  object.txt: x y z of a point inside the robot at the start state, and the edge of the box to put there.  Prints
// one line per step (the bool returns and isStateValid of the start); tests/test_gpu_world_plugin.py compares them.
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
    RobotState start(nv);
    for (double& v : start) q >> v;
    std::ifstream of(dir + "/object.txt");
    double at[3], edge;
    of >> at[0] >> at[1] >> at[2] >> edge;

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, P);     // an empty, editable grid
    GpuCollisionChecker cc(&ctx);
    CollisionObject box;
    box.id = "crate";
    box.shapes.push_back(Shape::Box(edge, edge, edge));
    box.shape_poses.push_back(PoseAt(at[0], at[1], at[2]));
    CollisionObject away = box;
    away.shape_poses[0] = PoseAt(origin[0] + 3 * res, origin[1] + 3 * res, origin[2] + 3 * res);
    CollisionObject two = away;
    two.shapes.push_back(Shape::Box(edge, edge, edge));
    two.shape_poses.push_back(PoseAt(at[0], at[1], at[2]));
    CollisionObject bad = box;
    bad.id = "bad";
    bad.shape_poses.clear();
    CollisionObject ghost = box;
    ghost.id = "ghost";

    bool ok = false;      // each edit is made before the state is checked
    printf("empty %d\n", (int)cc.isStateValid(start));
    ok = cc.insertObject(box);
    printf("insert %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("insert_again %d\n", (int)cc.insertObject(box));
    printf("insert_mismatched %d\n", (int)cc.insertObject(bad));
    ok = cc.moveShapes(away);
    printf("move %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.insertShapes(two);
    printf("insert_shapes %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.removeShapes(away);
    printf("remove_shapes %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("move_unknown %d\n", (int)cc.moveShapes(ghost));
    ok = cc.removeObject(std::string("crate"));
    printf("remove %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("remove_again %d\n", (int)cc.removeObject(box));
    ok = cc.insertObject(box);
    printf("reinsert %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.removeObject(box);
    printf("remove_by_object %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("done\n");
    return 0;
}
