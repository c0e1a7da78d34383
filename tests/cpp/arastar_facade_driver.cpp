// tests/cpp/arastar_facade_driver.cpp -- drives smpl_amd::GpuARAStar (include/smpl_amd/plugin.hpp), the mirror of smpl's
// ARAStar over the engine's own search, the way an anytime caller does: expansion-bounded chunks that continue one search,
// replan(0.0) with and without partial solutions, and force_planning_from_scratch + replan(allowed_time) to completion.
// A query file with a second goal selects another run instead: an unbounded replan for a goal that no state satisfies, then
// one for the second goal.  Prints one line per call; tests/test_gpu_arastar_facade.py compares them with the C-ABI and the oracle.
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
    int chunk = 0;
    q >> chunk;
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuManipLattice lattice(&ctx);
    if (!lattice.setGoalConfiguration(goal, tol)) return 4;
    if (!lattice.setStart(start)) return 5;
    auto print_path = [](const std::vector<int>& p) { for (int id : p) printf(" %d", id); printf("\n"); };
    std::vector<int> path;
    int cost = 0;

    // A query file that goes on behind `chunk` with a 1 and a second goal: the first goal is one that no state satisfies.
    // An unbounded replan for it ends with an empty OPEN: it returns 0 and touches neither the solution nor the cost; the
    // same planner then plans to the second goal on the same space.
    int unreachable = 0;
    if (q >> unreachable && unreachable == 1) {
        RobotState second(nv);
        for (double& v : second) q >> v;
        if (!q) return 3;
        GpuARAStar e(&ctx);
        e.set_initialsolution_eps(5.0);
        e.setTargetEpsilon(1.0);
        e.setDeltaEpsilon(1.0);
        GpuARAStar::TimeParameters tp = e.timeParameters();
        tp.bounded = false;
        tp.type = GpuARAStar::TimeParameters::EXPANSIONS;
        path.assign(2, -7);
        cost = -3;
        int ret = e.replan(tp, &path, &cost);
        const smplx_replan_stats st = e.lastCallStats();
        printf("exhausted %d %d %d %d %d %d %d %.17g", ret, st.result, st.call_expansions, e.get_n_expands(), st.s.solved, st.s.path_len, cost,
               e.get_solution_eps());
        print_path(path);
        if (!lattice.setGoalConfiguration(second, tol)) return 4;
        if (!lattice.setStart(start)) return 5;
        path.clear();
        ret = e.replan(tp, &path, &cost);
        printf("second %d %d %d %d %d %.17g", ret, e.lastCallStats().result, e.lastCallStats().resumed, cost, e.get_n_expands(),
               e.get_solution_eps());
        print_path(path);
        printf("done\n");
        return 0;
    }

    // 1. set_search_mode(false): every call bounded by `chunk` expansions; the search continues between calls
    GpuARAStar a(&ctx);
    a.set_initialsolution_eps(5.0);
    a.setTargetEpsilon(3.0);
    a.setDeltaEpsilon(1.0);
    a.set_search_mode(false);
    GpuARAStar::TimeParameters tp = a.timeParameters();
    tp.type = GpuARAStar::TimeParameters::EXPANSIONS;
    tp.max_expansions_init = tp.max_expansions = chunk;
    int ret = 0;
    for (int k = 0; k < 100000; ++k) {
        path.clear();
        ret = a.replan(tp, &path, &cost);
        const smplx_replan_stats& st = a.lastCallStats();
        printf("call %d %d %d %d %d\n", k, ret, st.result, st.call_expansions, st.resumed);
        if (st.result != SMPLX_ARA_TIMED_OUT) break;
    }
    printf("final %d %d %d %d %.17g %.17g %.17g", ret, cost, a.get_n_expands(), a.get_n_expands_init_solution(), a.get_solution_eps(),
           a.get_initial_eps(), a.get_final_epsilon());
    print_path(path);

    // 2. a new planner on the same space: replan(0.0) expands nothing; with partial solutions it returns the start
    GpuARAStar b(&ctx);
    b.set_initialsolution_eps(5.0);
    b.setTargetEpsilon(3.0);
    path.clear();
    ret = b.replan(0.0, &path, &cost);
    printf("zero %d %d %d %d\n", ret, b.lastCallStats().result, b.lastCallStats().call_expansions, (int)path.size());
    b.allowPartialSolutions(true);
    path.clear();
    ret = b.replan(0.0, &path, &cost);
    printf("zero_partial %d %d %d %d", ret, b.lastCallStats().result, b.lastCallStats().call_expansions, cost);
    print_path(path);

    // 3. force_planning_from_scratch, then replan(allowed_time) to completion
    b.allowPartialSolutions(false);
    b.force_planning_from_scratch();
    path.clear();
    ret = b.replan(120.0, &path, &cost);
    printf("timed %d %d %d %d %.17g", ret, b.lastCallStats().result, cost, b.get_n_expands(), b.get_solution_eps());
    print_path(path);
    printf("done\n");
    return 0;
}
