// tests/cpp/clearance_driver.cpp -- distance to collision through include/smpl_amd/plugin.hpp: the checker is asked for its
// CollisionDistanceExtension the way a reference caller asks (getExtension<T>() on the CollisionChecker it holds), then
// for the distance of the start state, of the edge start -> goal, and of a few states and edges at once.  Prints one line
// per answer with %.17g; tests/test_gpu_clearance_cpp.py compares them bit for bit with the C-ABI's.
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
    RobotState start(nv), goal(nv), tol(nv);
    for (double& v : start) q >> v;
    for (double& v : goal) q >> v;
    for (double& v : tol) q >> v;
    // the tail: a count, then that many states (the batched forms take state k -> state k + 1 as their edges)
    int nb = 0;
    q >> nb;
    std::vector<double> states((size_t)nb * nv);
    for (double& v : states) q >> v;
    if (!q) return 3;
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuCollisionChecker gpu_checker(&ctx);
    CollisionChecker* checker = &gpu_checker;   // used through the abstract interfaces from here on
    CollisionDistanceExtension* dist = checker->getExtension<CollisionDistanceExtension>();
    printf("extension %d %d\n", dist != nullptr, checker->getExtension<CollisionChecker>() == checker);
    if (!dist) return 4;
    printf("state %.17g\n", dist->distanceToCollision(start));
    printf("edge %.17g\n", dist->distanceToCollision(start, goal));
    printf("still %.17g\n", dist->distanceToCollision(start, start));
    // isStateValid(state, dist) is what it was: the validity, and the largest double
    double d = 0.0;
    const bool ok = checker->isStateValid(start, d);
    printf("valid %d %d\n", (int)ok, d == std::numeric_limits<double>::max());

    std::vector<double> out;
    if (!gpu_checker.distancesToCollision(states, out) || (int)out.size() != nb) return 5;
    printf("states");
    for (double v : out) printf(" %.17g", v);
    printf("\n");
    const std::vector<double> from(states.begin(), states.end() - nv), to(states.begin() + nv, states.end());
    if (!gpu_checker.distancesToCollision(from, to, out) || (int)out.size() != nb - 1) return 6;
    printf("edges");
    for (double v : out) printf(" %.17g", v);
    printf("\n");
    // a state of the wrong length is refused, not read
    printf("short %d\n", dist->distanceToCollision(RobotState(nv - 1, 0.0)) != dist->distanceToCollision(RobotState(nv - 1, 0.0)));
    printf("done\n");
    return 0;
}
