// tests/cpp/lazy_loop_driver.cpp -- a small lazy weighted A* over include/smpl_amd/plugin.hpp.
//
// The caller here knows ONLY what a lazy SBPL planner knows of its environment: RobotPlanningSpace::GetLazySuccs,
// GetTrueCost and GetGoalHeuristic through the abstract base class.  The loop was written for this test (it is not the
// reference's larastar): OPEN holds candidates (f, insertion number, state, parent, g, evaluated?) ordered by
// (f, insertion number).  A popped candidate whose parent edge is unevaluated gets GetTrueCost and goes back with the true
// cost, or is dropped; a popped candidate with an evaluated edge closes its state and expands it lazily.  At most
// max_expansions expansions.  tests/lazy_ref.py lazy_search is the same loop in Python, line for line, and
// tests/test_gpu_lazy_cpp.py requires identical output.
//
// usage: lazy_loop_driver <dir>      dir holds robot.txt mprim.txt grid.bin query.txt (query tail: eps max_expansions)
// prints: "expanded id ...", "evaluated parent>child:cost ...", "path id ..." (empty if none), "cost c", "stats ...", "done"
#include <chrono>
#include <cstdio>
#include <fstream>
#include <map>
#include <queue>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include <smpl_amd/plugin.hpp>

using namespace smpl_amd;

namespace {

struct Candidate {
    int f;
    long counter;
    int id, parent, g;
    bool evaluated;
};
struct Later {
    bool operator()(const Candidate& a, const Candidate& b) const { return std::tie(a.f, a.counter) > std::tie(b.f, b.counter); }
};

std::string slurp(const std::string& p)
{
    std::ifstream f(p);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::string robot = slurp(dir + "/robot.txt"), mprim = slurp(dir + "/mprim.txt");
    std::ifstream q(dir + "/query.txt");
    double origin[3], res, max_dist;
    int n[3], nv;
    PlanningParams params;
    smplx_params& P = params.engine;
    P = smplx_params();
    q >> origin[0] >> origin[1] >> origin[2] >> n[0] >> n[1] >> n[2] >> res >> max_dist >> nv;
    for (int i = 0; i < nv; ++i) q >> P.resolutions[i];
    q >> P.bfs_inflation_radius >> P.cost_per_cell >> P.use_short_dist_mprims >> P.short_dist_mprims_thresh >>
        P.use_xyzrpy_snap_mprim >> P.xyzrpy_snap_dist_thresh >> P.xy_rotate_by_var3 >> P.use_long_and_short;
    GoalConstraint goal;
    goal.type = JOINT_STATE_GOAL;
    RobotState start(nv);
    goal.angles.resize(nv); goal.angle_tolerances.resize(nv);
    for (double& v : start) q >> v;
    for (double& v : goal.angles) q >> v;
    for (double& v : goal.angle_tolerances) q >> v;
    double eps;
    int max_expansions;
    q >> eps >> max_expansions;
    if (!q) { fprintf(stderr, "bad query.txt\n"); return 2; }
    std::vector<int32_t> d2((size_t)n[0] * n[1] * n[2]);
    std::ifstream g(dir + "/grid.bin", std::ios::binary);
    g.read((char*)d2.data(), (std::streamsize)(d2.size() * sizeof(int32_t)));
    params.mprim_text = mprim;

    GpuPlanningContext ctx(robot, mprim, origin, n[0], n[1], n[2], res, max_dist, d2.data(), P);
    GpuRobotModel model(&ctx);
    GpuCollisionChecker cc(&ctx);
    GpuManipLattice lattice(&ctx);
    GpuBfsHeuristic heur(&ctx);
    RobotPlanningSpace* space = &lattice;
    if (!space->init(&model, &cc, &params)) return 3;
    if (!heur.init(space)) return 3;
    space->insertObserver(&heur);
    if (!space->insertHeuristic(&heur)) return 3;
    if (!space->setGoal(goal)) return 4;
    if (!space->setStart(start)) return 5;
    const int start_id = space->getStartStateID(), goal_id = space->getGoalStateID();

    const auto t0 = std::chrono::steady_clock::now();
    std::priority_queue<Candidate, std::vector<Candidate>, Later> open;
    std::map<int, int> gval, bp, hval;
    std::set<int> closed;
    auto heuristic = [&](int id) {
        auto it = hval.find(id);
        if (it == hval.end()) it = hval.emplace(id, space->GetGoalHeuristic(id)).first;
        return it->second;
    };
    long counter = 0;
    gval[start_id] = 0; bp[start_id] = -1;
    open.push(Candidate{(int)(eps * heuristic(start_id)), counter, start_id, -1, 0, true});
    std::vector<int> expanded;
    std::vector<std::tuple<int, int, int>> evaluated;
    bool found = false;
    std::vector<int> succs, costs;
    std::vector<bool> true_costs;
    while (!open.empty() && (int)expanded.size() < max_expansions) {
        const Candidate c = open.top();
        open.pop();
        if (closed.count(c.id)) continue;
        if (!c.evaluated) {
            const int cost = space->GetTrueCost(c.parent, c.id);
            evaluated.emplace_back(c.parent, c.id, cost);
            if (cost < 0) continue;
            ++counter;
            const int gnew = gval[c.parent] + cost;       // (the parent was closed when it generated this candidate)
            open.push(Candidate{gnew + (int)(eps * heuristic(c.id)), counter, c.id, c.parent, gnew, true});
            continue;
        }
        closed.insert(c.id); gval[c.id] = c.g; bp[c.id] = c.parent;
        if (c.id == goal_id) { found = true; break; }
        expanded.push_back(c.id);
        succs.clear(); costs.clear(); true_costs.clear();
        space->GetLazySuccs(c.id, &succs, &costs, &true_costs);
        for (size_t i = 0; i < succs.size(); ++i) {
            if (closed.count(succs[i])) continue;
            ++counter;
            open.push(Candidate{c.g + costs[i] + (int)(eps * heuristic(succs[i])), counter, succs[i], c.id, c.g + costs[i], (bool)true_costs[i]});
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::string msg;
    if (lattice.engineStatus(&msg) != SMPLX_OK) { fprintf(stderr, "engine error: %s\n", msg.c_str()); return 6; }
    printf("expanded");
    for (int id : expanded) printf(" %d", id);
    printf("\nevaluated");
    for (const auto& e : evaluated) printf(" %d>%d:%d", std::get<0>(e), std::get<1>(e), std::get<2>(e));
    printf("\npath");
    if (found) {   // the bp chain runs from the goal: printed from the start
        std::vector<int> path;
        for (int s = goal_id; s >= 0; s = bp[s]) path.push_back(s);
        for (size_t i = path.size(); i-- > 0;) printf(" %d", path[i]);
    }
    printf("\ncost %d\n", found ? gval[goal_id] : -1);
    int64_t lz[6] = {0, 0, 0, 0, 0, 0};
    smplx_lazy_counters(ctx.space(), lz);
    printf("stats seconds=%.6f expansions=%zu evaluated=%zu states=%d lazy_launches=%lld lazy_served=%lld true_cost_launches=%lld "
           "edges_evaluated=%lld cache_hits=%lld cache_misses=%lld\n",
           secs, expanded.size(), evaluated.size(), smplx_num_states(ctx.space()), (long long)lz[0], (long long)lz[1], (long long)lz[2],
           (long long)lz[3], (long long)lz[4], (long long)lz[5]);
    printf("done\n");
    return 0;
}
