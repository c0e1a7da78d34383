// tests/cpp/post_process_multi_driver.cpp -- smpl_amd::PostProcessPaths through include/smpl_amd/plugin.hpp: the states in
// the query's tail are cut into three paths (a long one, a two-point one, the rest), processed in one call and, one after
// the other, by PostProcessPath.  Prints "equal k 1" where path k came out of both with the same doubles, the sizes, the
// call's counters and the launch bound; tests/test_gpu_post_process_multi_cpp.py reads them.
#include <cstdio>
#include <cstring>
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
    int nb = 0;
    q >> nb;
    std::vector<RobotState> states(nb, RobotState(nv));
    for (RobotState& s : states) for (double& v : s) q >> v;
    if (!q || nb < 8) return 3;
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    const int cut = nb - 5;
    std::vector<std::vector<RobotState>> paths(3);
    paths[0].assign(states.begin(), states.begin() + cut);
    paths[1].assign(states.begin() + cut, states.begin() + cut + 2);
    paths[2].assign(states.begin() + cut + 2, states.end());
    std::vector<std::vector<RobotState>> single = paths;
    for (std::vector<RobotState>& p : single)
        if (!PostProcessPath(&ctx, p, true, true, true)) return 4;
    int64_t stats[4] = {-1, -1, -1, -1};
    if (!PostProcessPaths({&ctx, &ctx, &ctx}, paths, true, true, true, stats)) return 5;
    for (int k = 0; k < 3; ++k) {
        bool same = paths[k].size() == single[k].size();
        for (size_t i = 0; same && i < paths[k].size(); ++i)
            same = paths[k][i].size() == single[k][i].size() &&
                   std::memcmp(paths[k][i].data(), single[k][i].data(), sizeof(double) * paths[k][i].size()) == 0;
        printf("equal %d %d\n", k, (int)same);
        printf("size %d %zu\n", k, paths[k].size());
    }
    printf("stats %lld %lld %lld %lld\n", (long long)stats[0], (long long)stats[1], (long long)stats[2], (long long)stats[3]);
    printf("bound %d\n", SMPLX_PP_MULTI_MAX_LAUNCHES);
    // mismatched sizes are refused, an empty batch is fine
    std::vector<std::vector<RobotState>> two(2);
    printf("mismatch %d\n", (int)PostProcessPaths({&ctx}, two, true, true, true));
    std::vector<std::vector<RobotState>> none;
    printf("empty %d\n", (int)PostProcessPaths({}, none, true, true, true));
    printf("done\n");
    return 0;
}
