// tests/cpp/attached_body_driver.cpp -- attaches an object through smpl_amd::GpuCollisionChecker::attachObject
// (include/smpl_amd/plugin.hpp), plans with GpuARAStar, detaches it, sets the goal again and plans once more.  body.txt:
// id, link, the touch links, then x y z r rows.  Prints one line per step; tests/test_gpu_attached_bodies.py compares them.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
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
    std::ifstream bf(dir + "/body.txt");
    std::string id, link;
    int nallowed = 0;
    bf >> id >> link >> nallowed;
    std::vector<std::string> allowed(nallowed);
    for (std::string& a : allowed) bf >> a;
    std::vector<std::array<double, 4>> spheres;
    std::array<double, 4> sp;
    while (bf >> sp[0] >> sp[1] >> sp[2] >> sp[3]) spheres.push_back(sp);
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuManipLattice lattice(&ctx);
    GpuCollisionChecker cc(&ctx);
    CollisionChecker* checker = &cc;
    auto plan = [&](const char* tag) {
        if (!lattice.setGoalConfiguration(goal, tol)) { printf("%s goal_failed\n", tag); return; }
        if (!lattice.setStart(start)) { printf("%s start_invalid\n", tag); return; }
        GpuARAStar a(&ctx);
        a.set_initialsolution_eps(5.0);
        a.set_search_mode(false);          // bounded by the expansion budget below
        a.setImproveSolution(false);
        GpuARAStar::TimeParameters tp = a.timeParameters();
        tp.type = GpuARAStar::TimeParameters::EXPANSIONS;
        tp.max_expansions_init = tp.max_expansions = 6000;
        std::vector<int> path;
        int cost = 0;
        const int ret = a.replan(tp, &path, &cost);
        printf("%s %d %d %d", tag, ret, cost, a.get_n_expands());
        for (int p : path) printf(" %d", p);
        printf("\n");
    };
    const bool start_free = checker->isStateValid(start);
    if (!cc.attachObject(id, spheres, link, allowed)) return 6;
    if (cc.attachObject(id, spheres, link, allowed)) return 7;             // the same id twice
    if (cc.attachObject("other", spheres, "no_such_link", allowed)) return 8;
    printf("valid %d %d\n", (int)start_free, (int)checker->isStateValid(start));
    plan("with");
    if (!cc.detachObject(id)) return 9;
    if (cc.detachObject(id)) return 10;
    plan("without");
    printf("done\n");
    return 0;
}
