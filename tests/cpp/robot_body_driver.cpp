// tests/cpp/robot_body_driver.cpp -- the robot body through smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp) only:
// attachRobotBody, setJointPosition, isStateValid and detachRobotBody on a context with an editable grid.  body.txt: a body
// text with a joint named "swing"; values.txt: the positions to give it.  Prints one line per step (the bool returns and
// isStateValid of the start); tests/test_gpu_robot_body_cpp.py compares them with the same sequence through the C ABI.
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
    const std::string robot = slurp(dir + "/robot.txt"), mprim = slurp(dir + "/mprim.txt"), body = slurp(dir + "/body.txt");
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
    std::vector<double> values;
    std::ifstream vf(dir + "/values.txt");
    for (double v; vf >> v;) values.push_back(v);

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, P);     // an empty, editable grid
    GpuCollisionChecker cc(&ctx);
    bool ok = false;      // each edit is made before the state is checked
    printf("empty %d\n", (int)cc.isStateValid(start));
    printf("set_without_body %d\n", (int)cc.setJointPosition("swing", 0.5));
    printf("detach_without_body %d\n", (int)cc.detachRobotBody());
    printf("attach_malformed %d\n", (int)cc.attachRobotBody("link a\nvoxels nosuch 0.01\n"));
    ok = cc.attachRobotBody(body);
    printf("attach %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("attach_again %d\n", (int)cc.attachRobotBody(body));
    for (double v : values) {
        ok = cc.setJointPosition("swing", v);
        printf("set %d %d\n", (int)ok, (int)cc.isStateValid(start));
    }
    printf("set_unknown %d\n", (int)cc.setJointPosition("nosuch", 0.5));
    ok = cc.detachRobotBody();
    printf("detach %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("detach_again %d\n", (int)cc.detachRobotBody());
    ok = cc.attachRobotBody(body);
    printf("reattach %d %d\n", (int)ok, (int)cc.isStateValid(start));
    printf("done\n");
    return 0;
}
