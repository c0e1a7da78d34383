// tests/cpp/pose_goal_driver.cpp -- an XYZ_RPY_GOAL through include/smpl_amd/plugin.hpp, set the way
// PlannerInterface::setGoalPosition sets it (planner_interface.cpp:1267-1344): GoalConstraint -> setGoal -> setStart,
// then a weighted A* that knows only GetSuccs / GetGoalHeuristic until a successor is the goal id.  Prints one line per
// step; tests/test_gpu_pose_goal_cpp.py reads them.
#include <cstdio>
#include <fstream>
#include <functional>
#include <queue>
#include <sstream>
#include <string>
#include <unordered_map>
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
    RobotState start(nv), goal_angles(nv), tol(nv);
    for (double& v : start) q >> v;
    for (double& v : goal_angles) q >> v;
    for (double& v : tol) q >> v;
    // the tail: pose (x, y, z, R, P, Y), position tolerance, orientation tolerance, weight, expansion bound
    GoalConstraint goal;
    goal.type = XYZ_RPY_GOAL;
    goal.pose.resize(6);
    for (double& v : goal.pose) q >> v;
    double xyz_tol = 0, rpy_tol = 0, eps = 1;
    int max_expansions = 0;
    q >> xyz_tol >> rpy_tol >> eps >> max_expansions;
    for (int a = 0; a < 3; ++a) { goal.xyz_tolerance[a] = xyz_tol; goal.rpy_tolerance[a] = rpy_tol; }
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuManipLattice lattice(&ctx);
    GpuBfsHeuristic heur(&ctx);
    RobotPlanningSpace* space = &lattice;   // used through the abstract interfaces from here on
    RobotHeuristic* h = &heur;

    // a target offset would move the pose (getTargetOffsetPose): refused, not ignored
    GoalConstraint off = goal;
    off.xyz_offset[1] = 0.05;
    printf("offset %d\n", (int)space->setGoal(off));
    GoalConstraint shortpose = goal;
    shortpose.pose.resize(3);
    printf("short %d\n", (int)space->setGoal(shortpose));
    printf("pose %d\n", (int)space->setGoal(goal));
    if (!space->setStart(start)) return 5;
    double T[12];
    if (!lattice.planningLinkTransform(start, T)) return 6;
    printf("fk");
    for (double v : T) printf(" %.17g", v);
    printf("\n");

    // weighted A* over GetSuccs: f = g + eps * h, no re-expansions
    typedef std::pair<long long, int> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> open;
    std::unordered_map<int, int> gval, parent;
    std::unordered_map<int, bool> closed;
    const int sid = space->getStartStateID(), gid = space->getGoalStateID();
    gval[sid] = 0;
    open.push({(long long)(eps * h->GetGoalHeuristic(sid)), sid});
    int expansions = 0, reached = 0, cost = 0;
    while (!open.empty() && expansions < max_expansions && !reached) {
        const int s = open.top().second;
        open.pop();
        if (closed[s]) continue;
        closed[s] = true;
        ++expansions;
        std::vector<int> succs, costs;
        space->GetSuccs(s, &succs, &costs);
        for (size_t k = 0; k < succs.size() && !reached; ++k) {
            const int gs = gval[s] + costs[k];
            if (succs[k] == gid) { reached = 1; cost = gs; parent[gid] = s; break; }
            auto it = gval.find(succs[k]);
            if (it != gval.end() && it->second <= gs) continue;
            gval[succs[k]] = gs;
            parent[succs[k]] = s;
            open.push({gs + (long long)(eps * h->GetGoalHeuristic(succs[k])), succs[k]});
        }
    }
    printf("reached %d expansions %d cost %d\n", reached, expansions, cost);
    if (reached) {
        std::vector<int> ids;
        for (int s = gid;; s = parent[s]) { ids.insert(ids.begin(), s); if (s == sid) break; }
        std::vector<RobotState> path;
        if (!space->extractPath(ids, path)) return 7;
        printf("last");
        for (double v : path.back()) printf(" %.17g", v);
        printf("\n");
    }
    std::string msg;
    if (lattice.engineStatus(&msg) != SMPLX_OK) { fprintf(stderr, "engine: %s\n", msg.c_str()); return 8; }
    printf("done\n");
    return 0;
}
