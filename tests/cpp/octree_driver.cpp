// tests/cpp/octree_driver.cpp -- octomaps through smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp):
// processOctomapMsg, a duplicate id, moveShapes with an octree shape, an object mixing a box and an octree, and
// removeObject, on a context with an editable grid.  object.txt: x y z of a point inside the robot at the start state, and
// the grid's resolution (the edge of the leaf to put there).  Prints one line per step (the bool returns and isStateValid
// of the start); tests/test_gpu_octree_plugin.py compares them.
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
    // the octomap's frame sits at `at`: a leaf at its origin, and one three cells inside the grid's low corner
    const Pose frame = PoseAt(at[0], at[1], at[2]);
    const std::vector<double> here = {0.0, 0.0, 0.0, edge};
    const std::vector<double> corner = {origin[0] + 3 * res - at[0], origin[1] + 3 * res - at[1], origin[2] + 3 * res - at[2], edge};
    std::vector<double> both = corner;
    both.insert(both.end(), here.begin(), here.end());

    bool ok = false;      // each edit is made before the state is checked
    printf("empty %d\n", (int)cc.isStateValid(start));
    ok = cc.processOctomapMsg("map", here, frame);
    printf("octomap %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("octomap_again %d\n", (int)cc.processOctomapMsg("map", corner, frame));       // checkInsertOctomap: the id is taken
    printf("octomap_no_leaves %d\n", (int)cc.processOctomapMsg("none", std::vector<double>(), frame));
    printf("octomap_ragged %d\n", (int)cc.processOctomapMsg("ragged", std::vector<double>(7, 0.01), frame));
    CollisionObject moved;
    moved.id = "map";
    moved.shapes.push_back(Shape::OcTree(corner));
    moved.shape_poses.push_back(frame);
    ok = cc.moveShapes(moved);
    printf("move %d %d\n", (int)ok, (int)cc.isStateValid(start));
    moved.shapes[0] = Shape::OcTree(both);
    ok = cc.moveShapes(moved);
    printf("move_back %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.removeObject(std::string("map"));
    printf("remove %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("remove_again %d\n", (int)cc.removeObject(std::string("map")));
    CollisionObject mixed;
    mixed.id = "mixed";
    mixed.shapes.push_back(Shape::Box(edge, edge, edge));
    mixed.shape_poses.push_back(PoseAt(origin[0] + 3 * res, origin[1] + 3 * res, origin[2] + 3 * res));
    mixed.shapes.push_back(Shape::OcTree(here));
    mixed.shape_poses.push_back(frame);
    ok = cc.insertObject(mixed);
    printf("insert_mixed %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.processOctomapMsg("map", corner, frame);                                     // the id is free again
    printf("octomap_beside %d %d\n", (int)ok, (int)cc.isStateValid(start));
    ok = cc.removeObject(mixed);
    printf("remove_mixed %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("done\n");
    return 0;
}
