// include/smpl_amd/plugin.hpp -- C++ mirror of smpl's plugin interfaces for the expansion path,
// implemented over the C-ABI (include/smpl_amd.h).  Header-only; link with libsmpl_amd.so.
//
// Same class and method names, argument meaning and error behaviour (bool success, empty successor list
// = dead end) as the reference, minus Eigen/ROS/SBPL types:
//   CollisionChecker     smpl/include/smpl/collision_checker.h:48-130
//   RobotHeuristic       smpl/include/smpl/heuristic/robot_heuristic.h:53-101
//   RobotPlanningSpace   smpl/include/smpl/graph/robot_planning_space.h:60-218
//                        (+ SBPL DiscreteSpaceInformation::GetSuccs, Heuristic::GetGoalHeuristic)
//   Extension            smpl/include/smpl/extension.h:40-60
//   ARAStar              smpl/include/smpl/search/arastar.h:80-165 (GpuARAStar: the engine's own search)
// In a real integration these classes derive from the reference's own bases; the bodies
// stay as they are here.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <typeinfo>
#include <vector>

#include "../smpl_amd.h"

namespace smpl_amd {

typedef std::vector<double> RobotState;   // smpl/include/smpl/types.h:66

// smpl/include/smpl/extension.h:40-60
class Extension {
public:
    virtual ~Extension() {}
    template <class T> T* getExtension() { return dynamic_cast<T*>(getExtension(typeid(T).hash_code())); }
    virtual Extension* getExtension(size_t class_code) = 0;
};
template <class T> inline size_t GetClassCode() { return typeid(T).hash_code(); }

// smpl/include/smpl/types.h:148-195
enum GoalType { INVALID_GOAL_TYPE = -1, XYZ_GOAL, XYZ_RPY_GOAL, JOINT_STATE_GOAL, NUMBER_OF_GOAL_TYPES };
enum GroupType { FAILURE = -2, ANY = -1, BASE = 0, ARM = 1, BASE_ISO = 2 };
struct GoalConstraint {
    RobotState angles;                       // joint-state goals
    std::vector<double> angle_tolerances;
    std::vector<double> pose;                // workspace goals: planning-link pose (x, y, z, R, P, Y)
    double xyz_offset[3] = {0, 0, 0};
    double xyz_tolerance[3] = {0, 0, 0};
    double rpy_tolerance[3] = {0, 0, 0};
    std::vector<double> tgt_off_pose;        // goal pose offset from the planning link
    int xyz[3] = {0, 0, 0};
    GoalType type = INVALID_GOAL_TYPE;
};

// smpl/include/smpl/collision_checker.h:48-130, every virtual of the fork
class CollisionChecker : public virtual Extension {
public:
    virtual bool isStateValid(const RobotState& state, bool verbose = false) = 0;                       // :62
    virtual bool isStateValid(const RobotState& state, double& distToObst, bool verbose = false) = 0;  // :64
    virtual bool isStateToStateValid(const RobotState& start, const RobotState& finish, bool verbose = false) = 0;   // :77-80
    // [FORK] :82-88 -- non-pure, and the reference's default body is empty (falls off the end); here it answers with
    // the three-argument form and leaves the two distances untouched
    virtual bool isStateToStateValid(const RobotState& angles0, const RobotState& angles1, double& distToObst, int& distToObstCells,
                                     bool verbose = false)
    {
        (void)distToObst; (void)distToObstCells;
        return isStateToStateValid(angles0, angles1, verbose);
    }
    virtual bool interpolatePath(const RobotState& start, const RobotState& finish, std::vector<RobotState>& path) = 0;   // :99-102
    // [FORK] no-op hooks (:110-128)
    virtual void setLastExpansionStep(int) {}
    virtual void markGridForExpandedState(const RobotState&, const RobotState&, int) {}
    virtual void resetCellsMarking(int) {}
    virtual void setClearanceThreshold(double) {}
};

// smpl/include/smpl/collision_checker.h:132-144
class CollisionDistanceExtension : public virtual Extension {
public:
    virtual double distanceToCollision(const RobotState& state) = 0;                                 // :137
    virtual double distanceToCollision(const RobotState& start, const RobotState& finish) = 0;      // :141-143
};

class RobotPlanningSpace;

// smpl/include/smpl/graph/robot_planning_space_observer.h:42-50
class RobotPlanningSpaceObserver {
public:
    virtual ~RobotPlanningSpaceObserver() {}
    virtual void updateStart(const RobotState&) {}
    virtual void updateGoal(const GoalConstraint&) {}
};

// SBPL Heuristic + smpl/include/smpl/heuristic/robot_heuristic.h:53-101
class RobotHeuristic : public RobotPlanningSpaceObserver, public virtual Extension {
public:
    static const int Infinity = 32767;                       // :62 (INT16_MAX)
    bool init(RobotPlanningSpace* space) { m_space = space; return space != nullptr; }   // robot_heuristic.cpp:39-50
    RobotPlanningSpace* planningSpace() { return m_space; }
    virtual double getMetricStartDistance(double x, double y, double z) = 0;
    virtual double getMetricGoalDistance(double x, double y, double z) = 0;
    virtual bool setGoal(const GoalConstraint&) { return true; }
    virtual int GetGoalHeuristic(int state_id) = 0;
    virtual int GetGoalHeuristic(int state_id, int /*planning_group*/, int /*base_heuristic_idx*/) { return GetGoalHeuristic(state_id); }   // :88-91
    virtual int GetStartHeuristic(int state_id) = 0;
    virtual int GetFromToHeuristic(int from_id, int to_id) = 0;

private:
    RobotPlanningSpace* m_space = nullptr;
};

// smpl/include/smpl/robot_model.h:50-151, the part the lattice touches; the kinematics themselves live in the
// compiled model behind the C-ABI (smplx_model_create), so this carries names and limits only
class RobotModel : public virtual Extension {
public:
    virtual int jointVariableCount() const = 0;
    virtual bool checkJointLimits(const RobotState& state, bool verbose = false) = 0;
};

// smpl/include/smpl/planning_params.h:63-155: the fields this path reads; the rest of the reference's struct
// (log names, shortcutting options) stays with the caller
struct PlanningParams {
    smplx_params engine;        // discretization, cost_per_cell, planning_link_sphere_radius, primitive gating
    std::string mprim_text;     // contents of the file named by "mprim_filename"
};

// SBPL DiscreteSpaceInformation + smpl/include/smpl/graph/robot_planning_space.h:60-218
class RobotPlanningSpace : public virtual Extension {
public:
    virtual bool init(RobotModel* robot, CollisionChecker* checker, const PlanningParams* params)   // :68-71
    {
        m_robot = robot; m_checker = checker; m_params = params;
        return robot && checker && params;
    }
    virtual bool setStart(const RobotState& state) = 0;                                            // :73
    virtual bool setMultipleStart(const std::vector<RobotState>&) { return false; }               // [FORK] :74
    virtual bool setGoal(const GoalConstraint& goal) = 0;                                          // :76
    virtual int getStartStateID() const = 0;
    virtual int getGoalStateID() const = 0;
    virtual std::vector<int> getStartStatesID() const { return std::vector<int>(1, getStartStateID()); }   // [FORK] :80-83
    virtual bool extractPath(const std::vector<int>& ids, std::vector<RobotState>& path) = 0;      // :85-87
    virtual bool insertHeuristic(RobotHeuristic* h)                                                // :89, robot_planning_space.cpp:96-108
    {
        if (!h || hasHeuristic(h)) return false;
        m_heuristics.push_back(h);
        return true;
    }
    virtual bool eraseHeuristic(const RobotHeuristic* h)
    {
        for (size_t i = 0; i < m_heuristics.size(); ++i)
            if (m_heuristics[i] == h) { m_heuristics.erase(m_heuristics.begin() + i); return true; }
        return false;
    }
    virtual bool hasHeuristic(const RobotHeuristic* h)
    {
        for (RobotHeuristic* x : m_heuristics) if (x == h) return true;
        return false;
    }
    RobotModel* robot() { return m_robot; }
    CollisionChecker* collisionChecker() { return m_checker; }
    const PlanningParams* params() const { return m_params; }
    size_t numHeuristics() const { return m_heuristics.size(); }
    RobotHeuristic* heuristic(size_t i) { return i < m_heuristics.size() ? m_heuristics[i] : nullptr; }
    void insertObserver(RobotPlanningSpaceObserver* obs) { if (obs && !hasObserver(obs)) m_obs.push_back(obs); }
    void eraseObserver(RobotPlanningSpaceObserver* obs)
    {
        for (size_t i = 0; i < m_obs.size(); ++i) if (m_obs[i] == obs) { m_obs.erase(m_obs.begin() + i); return; }
    }
    bool hasObserver(RobotPlanningSpaceObserver* obs) const
    {
        for (RobotPlanningSpaceObserver* x : m_obs) if (x == obs) return true;
        return false;
    }
    void notifyStartChanged(const RobotState& state) { for (RobotPlanningSpaceObserver* o : m_obs) o->updateStart(state); }   // robot_planning_space.cpp:117-123
    void notifyGoalChanged(const GoalConstraint& goal) { for (RobotPlanningSpaceObserver* o : m_obs) o->updateGoal(goal); }

    // DiscreteSpaceInformation side
    virtual void GetSuccs(int state_id, std::vector<int>* succs, std::vector<int>* costs) = 0;     // :135-138
    virtual void GetPreds(int state_id, std::vector<int>* preds, std::vector<int>* costs) = 0;     // :172-175
    // lazy variants (:124-130); the defaults are GetSuccs with every cost true and its cost (robot_planning_space.cpp:182-200)
    virtual void GetLazySuccs(int state_id, std::vector<int>* succs, std::vector<int>* costs, std::vector<bool>* true_costs)
    {
        GetSuccs(state_id, succs, costs);
        true_costs->assign(succs->size(), true);
    }
    virtual int GetTrueCost(int parent_id, int child_id)
    {
        std::vector<int> succs, costs;
        GetSuccs(parent_id, &succs, &costs);
        for (size_t i = 0; i < succs.size(); ++i)
            if (succs[i] == child_id) return costs[i];
        return -1;
    }
    virtual void PrintState(int state_id, bool verbose, FILE* f = nullptr) = 0;                    // :177-180
    virtual int GetGoalHeuristic(int state_id)                                                    // robot_planning_space.cpp:133-140
    {
        return numHeuristics() == 0 ? 0 : heuristic(0)->GetGoalHeuristic(state_id);
    }
    virtual int GetStartHeuristic(int state_id) { return numHeuristics() == 0 ? 0 : heuristic(0)->GetStartHeuristic(state_id); }
    virtual int GetFromToHeuristic(int from_id, int to_id)
    {
        return numHeuristics() == 0 ? 0 : heuristic(0)->GetFromToHeuristic(from_id, to_id);
    }
    // [FORK] group / expansion-step entry points (:140-158), driven only by the fork's other planners.  With
    // group ANY they are GetSuccs (manip_lattice.cpp:315-411 differs from :219-313 only in the no-op
    // setLastExpansionStep hook); other groups are outside this path and yield no successors.
    virtual void GetSuccsByGroup(int state_id, std::vector<int>* succs, std::vector<int>* costs, std::vector<int>* /*clearance_cells*/, int group)
    {
        if (group == ANY) GetSuccs(state_id, succs, costs);
    }
    virtual void GetSuccsByGroupAndExpansion(int state_id, std::vector<int>* succs, std::vector<int>* costs, int group, int /*expansion_step*/)
    {
        if (group == ANY) GetSuccs(state_id, succs, costs);
    }
    virtual void GetSuccsWithExpansion(int state_id, std::vector<int>* succs, std::vector<int>* costs, int expansion_step)
    {
        if (m_checker) m_checker->setLastExpansionStep(expansion_step);
        GetSuccs(state_id, succs, costs);
    }
    virtual void GetPredsByGroupAndExpansion(int, std::vector<int>*, std::vector<int>*, std::vector<int>*, int, int, int) {}
    virtual bool updateMultipleStartStates(std::vector<int>*, std::vector<double>*, int) { return false; }
    virtual void setMotionPlanRequestType(int) {}
    virtual void setSelectedStartId(int) {}

private:
    RobotModel* m_robot = nullptr;
    CollisionChecker* m_checker = nullptr;
    const PlanningParams* m_params = nullptr;
    std::vector<RobotHeuristic*> m_heuristics;
    std::vector<RobotPlanningSpaceObserver*> m_obs;
};

// sbpl::collision::Object (sbpl_collision_checking/include/sbpl_collision_checking/shapes.h, world_collision_model.h): an
// id, shapes and one pose per shape.  A Shape is the flat form of the reference's shapes::Shape hierarchy: box size, sphere
// radius, cylinder / cone radius and length, a mesh's vertices and index triples, or an octree's occupied leaves (shapes::
// OcTree: rows {cx, cy, cz, size} in the order the octomap's begin_leafs() yields them; world objects only).  Planes are
// not supported.
struct Shape {
    enum Type { BOX = SMPLX_SHAPE_BOX, SPHERE = SMPLX_SHAPE_SPHERE, CYLINDER = SMPLX_SHAPE_CYLINDER, CONE = SMPLX_SHAPE_CONE, MESH = SMPLX_SHAPE_MESH,
                OCTREE = SMPLX_SHAPE_OCTREE };
    Type type = BOX;
    double dims[3] = {0.0, 0.0, 0.0};      // box: x y z;  sphere: r;  cylinder, cone: r, length
    std::vector<double> vertices;          // MESH: 3 per vertex;  OCTREE: 4 per leaf
    std::vector<int32_t> triangles;        // MESH: 3 per triangle
    static Shape OcTree(std::vector<double> leaves) { Shape s; s.type = OCTREE; s.vertices = std::move(leaves); return s; }
    static Shape Box(double x, double y, double z) { Shape s; s.type = BOX; s.dims[0] = x; s.dims[1] = y; s.dims[2] = z; return s; }
    static Shape Sphere(double r) { Shape s; s.type = SPHERE; s.dims[0] = r; return s; }
    static Shape Cylinder(double r, double length) { Shape s; s.type = CYLINDER; s.dims[0] = r; s.dims[1] = length; return s; }
    static Shape Cone(double r, double length) { Shape s; s.type = CONE; s.dims[0] = r; s.dims[1] = length; return s; }
    static Shape Mesh(std::vector<double> v, std::vector<int32_t> t) { Shape s; s.type = MESH; s.vertices = std::move(v); s.triangles = std::move(t); return s; }
};
using Pose = std::array<double, 12>;       // 3x4 row major [R | t], world frame (the reference's Eigen::Affine3d)
inline Pose PoseAt(double x, double y, double z) { return Pose{{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z}}; }
struct CollisionObject {
    std::string id;
    std::vector<Shape> shapes;
    std::vector<Pose> shape_poses;
};
// moveit_msgs::AttachedCollisionObject as CollisionSpace::processAttachedCollisionObject reads it (collision_space.cpp:
// 318-348): the object (its shape poses in the frame of link_name), the link, the touch links and the operation, which
// the message keeps in object.operation
struct AttachedCollisionObject {
    CollisionObject object;
    std::string link_name;
    std::vector<std::string> touch_links;
    enum Operation { ADD, REMOVE, APPEND, MOVE } operation = ADD;
};

// One query context on one GPU.  Owns the C-ABI handles; the three plugin facades below share it, the
// way the reference's lattice, heuristic and checker share one OccupancyGrid and one RobotModel.
class GpuPlanningContext {
public:
    GpuPlanningContext(const std::string& robot_text, const std::string& mprim_text, const double origin[3], int nx, int ny,
                       int nz, double res, double max_dist, const int32_t* d2, const smplx_params& params)
    {
        check(smplx_grid_create(origin, nx, ny, nz, res, max_dist, d2, &grid_));
        check(smplx_model_create(robot_text.c_str(), &model_));
        check(smplx_space_create(model_, grid_, mprim_text.c_str(), &params, &space_));
        nvars_ = smplx_space_num_vars(space_);
        nprims_ = smplx_space_num_prims(space_);
        res_ = res;
    }
    // the same on an EDITABLE grid, built and kept on the GPU (smplx_grid_create_empty): starts empty and takes world objects
    // through GpuCollisionChecker::insertObject, as CollisionSpace does on its OccupancyGrid
    GpuPlanningContext(const std::string& robot_text, const std::string& mprim_text, const double origin[3], int nx, int ny,
                       int nz, double res, double max_dist, const smplx_params& params)
    {
        check(smplx_grid_create_empty(origin, nx, ny, nz, res, max_dist, &grid_));
        check(smplx_model_create(robot_text.c_str(), &model_));
        check(smplx_space_create(model_, grid_, mprim_text.c_str(), &params, &space_));
        nvars_ = smplx_space_num_vars(space_);
        nprims_ = smplx_space_num_prims(space_);
        res_ = res;
    }
    ~GpuPlanningContext()
    {
        smplx_space_destroy(space_);
        smplx_model_destroy(model_);
        smplx_grid_destroy(grid_);
    }
    GpuPlanningContext(const GpuPlanningContext&) = delete;
    GpuPlanningContext& operator=(const GpuPlanningContext&) = delete;
    smplx_space* space() const { return space_; }
    smplx_grid* grid() const { return grid_; }
    int nvars() const { return nvars_; }
    int nprims() const { return nprims_; }
    double resolution() const { return res_; }
    static void check(int code)
    {
        if (code != SMPLX_OK) throw std::runtime_error(std::string("smpl_amd: ") + smplx_last_error());
    }

private:
    smplx_grid* grid_ = nullptr;
    smplx_model* model_ = nullptr;
    smplx_space* space_ = nullptr;
    int nvars_ = 0, nprims_ = 0;
    double res_ = 0.0;
};

// RobotModel facade over the compiled model: variable count and KDLRobotModel::checkJointLimits
// (sbpl_kdl_robot_model/src/kdl_robot_model.cpp:210-235)
class GpuRobotModel : public RobotModel {
public:
    using Extension::getExtension;
    explicit GpuRobotModel(GpuPlanningContext* ctx) : ctx_(ctx) {}
    int jointVariableCount() const override { return ctx_->nvars(); }
    bool checkJointLimits(const RobotState& state, bool = false) override
    {
        uint8_t ok = 0;
        return (int)state.size() == ctx_->nvars() && smplx_check_joint_limits(ctx_->space(), state.data(), 1, &ok) == SMPLX_OK && ok;
    }
    Extension* getExtension(size_t class_code) override { return class_code == GetClassCode<RobotModel>() ? this : nullptr; }

private:
    GpuPlanningContext* ctx_;
};

// sbpl::collision::CollisionSpace (sbpl_collision_checking/include/sbpl_collision_checking/collision_space.h:66-266)
class GpuCollisionChecker : public CollisionChecker, public CollisionDistanceExtension {
public:
    using Extension::getExtension;   // keep the typed lookup visible next to the override
    explicit GpuCollisionChecker(GpuPlanningContext* ctx) : ctx_(ctx) {}
    GpuCollisionChecker(const GpuCollisionChecker&) = delete;
    GpuCollisionChecker& operator=(const GpuCollisionChecker&) = delete;
    ~GpuCollisionChecker() { smplx_body_destroy(body_); }   // a placed body stays on the grid, which owns the placement
    bool isStateValid(const RobotState& state, bool = false) override
    {
        uint8_t ok = 0;
        return smplx_cc_state_valid_batch(ctx_->space(), state.data(), 1, &ok, nullptr) == SMPLX_OK && ok;
    }
    // collision_space.h:202-205: the reference's override has an empty body; this one answers with the validity and
    // the value CollisionSpace::isStateValid starts its own `dist` at (collision_space.cpp:532-536).  The distance itself
    // is what the CollisionDistanceExtension below answers: getExtension<CollisionDistanceExtension>()->distanceToCollision(state)
    bool isStateValid(const RobotState& state, double& distToObst, bool verbose = false) override
    {
        distToObst = std::numeric_limits<double>::max();
        return isStateValid(state, verbose);
    }
    using CollisionChecker::isStateToStateValid;   // keep the fork's 5-argument overload visible
    bool isStateToStateValid(const RobotState& start, const RobotState& finish, bool = false) override
    {
        uint8_t ok = 0;
        return smplx_cc_edge_valid_batch(ctx_->space(), start.data(), finish.data(), 1, &ok, nullptr, nullptr) == SMPLX_OK && ok;
    }
    // batched forms: what a frontier-batched caller uses instead of one call per edge
    bool areStatesToStatesValid(const std::vector<double>& starts, const std::vector<double>& finishes, std::vector<uint8_t>& ok)
    {
        const int n = (int)(starts.size() / ctx_->nvars());
        ok.assign(n, 0);
        return smplx_cc_edge_valid_batch(ctx_->space(), starts.data(), finishes.data(), n, ok.data(), nullptr, nullptr) == SMPLX_OK;
    }
    bool interpolatePath(const RobotState& start, const RobotState& finish, std::vector<RobotState>& path) override
    {
        int n = 0;
        if (smplx_cc_interpolate(ctx_->space(), start.data(), finish.data(), nullptr, 0, &n) != SMPLX_OK) return false;
        std::vector<double> buf((size_t)n * ctx_->nvars());
        if (smplx_cc_interpolate(ctx_->space(), start.data(), finish.data(), buf.data(), n, &n) != SMPLX_OK) return false;
        path.clear();
        for (int i = 0; i < n; ++i) path.emplace_back(buf.begin() + (size_t)i * ctx_->nvars(), buf.begin() + (size_t)(i + 1) * ctx_->nvars());
        return true;
    }
    // collision_space.cpp:297-312.  The object arrives as spheres (x, y, z, r in the link's frame) instead of shapes and
    // transforms; `allowed` holds the links and attached objects it may touch (MoveIt's touch links).  False with the
    // reason in smplx_last_error() where the reference returns false, and also for a link outside the collision group.
    bool attachObject(const std::string& id, const std::vector<std::array<double, 4>>& spheres, const std::string& link_name,
                      const std::vector<std::string>& allowed = {})
    {
        std::vector<double> xyzr;
        for (const auto& s : spheres) xyzr.insert(xyzr.end(), s.begin(), s.end());
        std::vector<const char*> names;
        for (const std::string& a : allowed) names.push_back(a.c_str());
        return smplx_attach_body(ctx_->space(), id.c_str(), link_name.c_str(), xyzr.data(), (int)spheres.size(), names.data(),
                                 (int)names.size()) == SMPLX_OK;
    }
    // collision_space.cpp:297-304, the reference's own signature plus the allowed list: shapes at poses in the frame of
    // link_name, voxelised on the GPU into spheres of SMPLX_ATTACHED_SPHERE_RADIUS exactly as generateSpheresModel makes them
    // (smplx_attach_object in include/smpl_amd.h).  False for shapes and transforms of different lengths and wherever the
    // C call fails: an id already attached, a link unknown or outside the group, a bad shape, shapes that make no sphere,
    // an object of more than 512 spheres.
    bool attachObject(const std::string& id, const std::vector<Shape>& shapes, const std::vector<Pose>& transforms,
                      const std::string& link_name, const std::vector<std::string>& allowed = {})
    {
        std::vector<smplx_shape> flat;
        if (!flatten(shapes, transforms, flat)) return false;
        std::vector<const char*> names;
        for (const std::string& a : allowed) names.push_back(a.c_str());
        return smplx_attach_object(ctx_->space(), id.c_str(), link_name.c_str(), flat.data(), (int)flat.size(), SMPLX_ATTACHED_SPHERE_RADIUS,
                                   names.data(), (int)names.size()) == SMPLX_OK;
    }
    bool detachObject(const std::string& id) { return smplx_detach_body(ctx_->space(), id.c_str()) == SMPLX_OK; }
    // collision_space.cpp:318-348: ADD attaches the object's shapes to link_name, REMOVE detaches the id; APPEND and MOVE
    // return false where the reference throws "unimplemented".  Difference: the reference ignores the touch links
    // ("TODO: handle touch links", :331) and so checks the object against the link that holds it; here they are passed
    // as the allowed list.
    bool processAttachedCollisionObject(const AttachedCollisionObject& ao)
    {
        switch (ao.operation) {
        case AttachedCollisionObject::ADD:
            return attachObject(ao.object.id, ao.object.shapes, ao.object.shape_poses, ao.link_name, ao.touch_links);
        case AttachedCollisionObject::REMOVE:
            return detachObject(ao.object.id);
        default:
            return false;
        }
    }
    // collision_space.cpp:228-275 over world_collision_model.cpp:193-280: world objects, voxelised on the GPU as the
    // reference voxelises them (smplx_world_* in include/smpl_amd.h).  False with the reason in smplx_last_error() where the
    // reference returns false (an id already in the world, an unknown id, shapes and poses of different lengths) and for
    // a context whose grid came from a finished field.  Each is a grid edit: set the lattice's goal again before planning.
    virtual bool insertObject(const CollisionObject& object)
    {
        std::vector<smplx_shape> shapes;
        return flatten(object, shapes) && smplx_world_insert_object(ctx_->grid(), object.id.c_str(), shapes.data(), (int)shapes.size()) == SMPLX_OK;
    }
    virtual bool removeObject(const CollisionObject& object) { return removeObject(object.id); }
    virtual bool removeObject(const std::string& object_name) { return smplx_world_remove_object(ctx_->grid(), object_name.c_str()) == SMPLX_OK; }
    // moveShapes, insertShapes and removeShapes are one operation in the reference (remove, then insert the object as
    // given: world_collision_model.cpp:264-280); here one field edit
    virtual bool moveShapes(const CollisionObject& object)
    {
        std::vector<smplx_shape> shapes;
        return flatten(object, shapes) && smplx_world_move_object(ctx_->grid(), object.id.c_str(), shapes.data(), (int)shapes.size()) == SMPLX_OK;
    }
    virtual bool insertShapes(const CollisionObject& object) { return moveShapes(object); }
    virtual bool removeShapes(const CollisionObject& object) { return moveShapes(object); }
    // CollisionSpace::processOctomapMsg (collision_space.cpp:285-288) -> WorldCollisionModel::insertOctomap
    // (world_collision_model.cpp:303-318): the octomap becomes a world object of one octree shape at its origin pose.  The
    // caller walks their octomap's begin_leafs() and passes the occupied leaves, 4 doubles each {cx, cy, cz, size}.  False
    // where checkInsertOctomap (:553-572) refuses -- an id already in the world (the frame and the binary flag of the
    // message have no counterpart here) -- and for leaves the engine refuses.  The object is removed and moved like any
    // other (removeObject, moveShapes with Shape::OcTree).
    virtual bool processOctomapMsg(const std::string& id, const std::vector<double>& leaves, const Pose& origin)
    {
        CollisionObject object;
        object.id = id;
        object.shapes.push_back(Shape::OcTree(leaves));
        object.shape_poses.push_back(origin);
        return insertObject(object);
    }
    // The robot's links outside the planning group as obstacles (smplx_body_* in include/smpl_amd.h; the reference keeps
    // them in the grid through SelfCollisionModelImpl::updateVoxelsStates, self_collision_model.cpp:770-837).
    // attachRobotBody builds the voxel models of a body text and places them; setJointPosition
    // (CollisionSpace::setJointPosition, collision_space.cpp) sets the value of a joint of the attached body record and
    // puts the body again, and returns false for a joint it does not know, as the reference does.  Every call that changes
    // cells is a grid edit: set the lattice's goal again before planning.  Needs a context on an editable grid.
    bool attachRobotBody(const std::string& body_text)
    {
        if (body_) return false;
        smplx_body* b = nullptr;
        if (smplx_body_create(body_text.c_str(), &b) != SMPLX_OK) return false;
        if (smplx_grid_put_body(ctx_->grid(), b) != SMPLX_OK) { smplx_body_destroy(b); return false; }
        body_ = b;
        return true;
    }
    bool detachRobotBody()
    {
        if (!body_) return false;
        const bool ok = smplx_grid_take_body(ctx_->grid()) == SMPLX_OK;
        smplx_body_destroy(body_);
        body_ = nullptr;
        return ok;
    }
    bool setJointPosition(const std::string& name, double position)
    {
        if (!body_ || smplx_body_set_joint(body_, name.c_str(), position) != SMPLX_OK) return false;
        return smplx_grid_put_body(ctx_->grid(), body_) == SMPLX_OK;
    }
    // CollisionDistanceExtension: metres to the nearest collision of a state, or of the waypoints of an edge
    // (smplx_cc_state_clearance_batch / smplx_cc_edge_clearance_batch, include/smpl_amd.h: leaf spheres against the
    // distance field and against each other over the checked pairs; saturates at the field's maximum distance).  NaN, with
    // the reason in smplx_last_error(), where the engine refuses the call.
    double distanceToCollision(const RobotState& state) override
    {
        double d = std::numeric_limits<double>::quiet_NaN();
        if ((int)state.size() != ctx_->nvars()) return d;
        (void)smplx_cc_state_clearance_batch(ctx_->space(), state.data(), 1, &d, nullptr, nullptr);
        return d;
    }
    double distanceToCollision(const RobotState& start, const RobotState& finish) override
    {
        double d = std::numeric_limits<double>::quiet_NaN();
        if ((int)start.size() != ctx_->nvars() || (int)finish.size() != ctx_->nvars()) return d;
        (void)smplx_cc_edge_clearance_batch(ctx_->space(), start.data(), finish.data(), 1, &d, nullptr, nullptr);
        return d;
    }
    // batched forms: states (and finishes) hold n * nvars values, out gets n distances
    bool distancesToCollision(const std::vector<double>& states, std::vector<double>& out)
    {
        if (states.size() % ctx_->nvars() != 0) return false;
        const int n = (int)(states.size() / ctx_->nvars());
        out.assign(n, 0.0);
        return smplx_cc_state_clearance_batch(ctx_->space(), states.data(), n, out.data(), nullptr, nullptr) == SMPLX_OK;
    }
    bool distancesToCollision(const std::vector<double>& starts, const std::vector<double>& finishes, std::vector<double>& out)
    {
        if (starts.size() % ctx_->nvars() != 0 || finishes.size() != starts.size()) return false;
        const int n = (int)(starts.size() / ctx_->nvars());
        out.assign(n, 0.0);
        return smplx_cc_edge_clearance_batch(ctx_->space(), starts.data(), finishes.data(), n, out.data(), nullptr, nullptr) == SMPLX_OK;
    }
    Extension* getExtension(size_t class_code) override
    {
        if (class_code == GetClassCode<CollisionChecker>()) return static_cast<CollisionChecker*>(this);   // collision_space.cpp:523-529
        if (class_code == GetClassCode<CollisionDistanceExtension>()) return static_cast<CollisionDistanceExtension*>(this);
        return nullptr;
    }

private:
    // checkObjectInsert (world_collision_model.cpp:401-404): one pose per shape
    static bool flatten(const CollisionObject& object, std::vector<smplx_shape>& out) { return flatten(object.shapes, object.shape_poses, out); }
    static bool flatten(const std::vector<Shape>& shapes, const std::vector<Pose>& poses, std::vector<smplx_shape>& out)
    {
        if (shapes.size() != poses.size()) return false;
        for (size_t i = 0; i < shapes.size(); ++i) {
            const Shape& s = shapes[i];
            smplx_shape c = {};
            c.type = (int32_t)s.type;
            for (int k = 0; k < 3; ++k) c.dims[k] = s.dims[k];
            for (int k = 0; k < 12; ++k) c.pose[k] = poses[i][k];
            c.vertices = s.vertices.data(); c.nvertices = (int32_t)(s.vertices.size() / 3);
            c.triangles = s.triangles.data(); c.ntriangles = (int32_t)(s.triangles.size() / 3);
            if (s.type == Shape::MESH && (s.vertices.size() % 3 != 0 || s.triangles.size() % 3 != 0)) return false;   // voxelize.cpp:1016-1019
            if (s.type == Shape::OCTREE) {         // leaf rows of four doubles, no triangles
                if (s.vertices.empty() || s.vertices.size() % 4 != 0 || !s.triangles.empty()) return false;
                c.nvertices = (int32_t)(s.vertices.size() / 4);
                c.triangles = nullptr;
            }
            out.push_back(c);
        }
        return true;
    }
    GpuPlanningContext* ctx_;
    smplx_body* body_ = nullptr;
};

// sbpl::motion::ManipLattice (smpl/include/smpl/graph/manip_lattice.h:63-307)
class GpuManipLattice : public RobotPlanningSpace {
public:
    using Extension::getExtension;   // keep the typed lookup visible next to the override
    explicit GpuManipLattice(GpuPlanningContext* ctx) : ctx_(ctx) {}
    // GoalConstraint with JOINT_STATE_GOAL / XYZ_GOAL / XYZ_RPY_GOAL (manip_lattice.cpp:1982-1997); observers (the BFS
    // heuristic) are notified inside the engine: BFS_3D::run completes before this returns
    bool setGoalConfiguration(const RobotState& angles, const RobotState& tolerances)
    {
        return smplx_set_goal_joint(ctx_->space(), angles.data(), tolerances.data()) == SMPLX_OK;
    }
    bool setGoalPosition(const double xyz[3], const double tol[3]) { return smplx_set_goal_xyz(ctx_->space(), xyz, tol) == SMPLX_OK; }
    // XYZ_RPY_GOAL: isGoal (manip_lattice.cpp:1614-1671) reads rpy_tolerance[0] alone; smplx_rpy_angle is its distance
    bool setGoalPose(const double xyz[3], const double rpy[3], const double xyz_tol[3], double rpy_tol)
    {
        return smplx_set_goal_pose(ctx_->space(), xyz, rpy, xyz_tol, rpy_tol) == SMPLX_OK;
    }
    // ManipLattice::setGoal (manip_lattice.cpp:1982-1997): dispatch on the goal type, then notify the observers
    // (the heuristic; its BFS has already been run to completion inside the engine)
    bool setGoal(const GoalConstraint& goal) override
    {
        bool ok = false;
        switch (goal.type) {
        case XYZ_GOAL: {
            const std::vector<double>& p = goal.tgt_off_pose.size() >= 3 ? goal.tgt_off_pose : goal.pose;
            if (p.size() < 3) return false;
            // EuclidDistHeuristic measures against the rotation of the pose's rpy even under an XYZ goal; smplx_set_goal_xyz
            // has no way to pass one and measures against the identity (rpy 0 0 0): a wrong h is worse than a refusal
            if (smplx_space_heuristic(ctx_->space()) == SMPLX_H_EUCLID && p.size() >= 6 && (p[3] != 0.0 || p[4] != 0.0 || p[5] != 0.0)) return false;
            const double xyz[3] = {p[0], p[1], p[2]};
            ok = setGoalPosition(xyz, goal.xyz_tolerance);
        } break;
        case JOINT_STATE_GOAL:
            if ((int)goal.angles.size() != ctx_->nvars() || goal.angle_tolerances.size() != goal.angles.size()) return false;
            ok = setGoalConfiguration(goal.angles, goal.angle_tolerances);
            break;
        case XYZ_RPY_GOAL: {
            // the pose is the reference's tgt_off_pose; getTargetOffsetPose (manip_lattice.cpp:2297-2312) is not applied
            // here, so a goal that asks for an offset is refused rather than planned to the wrong pose
            if (goal.xyz_offset[0] != 0.0 || goal.xyz_offset[1] != 0.0 || goal.xyz_offset[2] != 0.0) return false;
            const std::vector<double>& p = goal.tgt_off_pose.size() >= 6 ? goal.tgt_off_pose : goal.pose;
            if (p.size() < 6) return false;
            ok = setGoalPose(&p[0], &p[3], goal.xyz_tolerance, goal.rpy_tolerance[0]);
        } break;
        default:
            return false;
        }
        if (ok) notifyGoalChanged(goal);
        return ok;
    }
    // the planning link's transform at a state, row-major 3x4 (what computePlanningLinkFK gives the reference's callers)
    bool planningLinkTransform(const RobotState& state, double T[12])
    {
        return (int)state.size() == ctx_->nvars() && smplx_planning_pose_batch(ctx_->space(), state.data(), 1, T) == SMPLX_OK;
    }
    bool setStart(const RobotState& state) override
    {
        if (smplx_set_start(ctx_->space(), state.data(), nullptr) != SMPLX_OK) return false;
        notifyStartChanged(state);
        return true;
    }
    int getStartStateID() const override { return smplx_start_id(ctx_->space()); }
    int getGoalStateID() const override { return smplx_goal_id(ctx_->space()); }
    void GetSuccs(int state_id, std::vector<int>* succs, std::vector<int>* costs) override
    {
        const int cap = ctx_->nprims();
        std::vector<int32_t> s(cap), c(cap);
        int n = 0;
        if (smplx_get_succs(ctx_->space(), state_id, s.data(), c.data(), cap, &n) != SMPLX_OK) {
            // GetSuccs cannot report: the list stays empty (a dead end to the search), the error stays on the space
            // (smplx_space_status / engineStatus()) and is logged once
            if (!logged_) { fprintf(stderr, "smpl_amd: GetSuccs(%d) failed: %s\n", state_id, smplx_last_error()); logged_ = true; }
            return;
        }
        succs->insert(succs->end(), s.begin(), s.begin() + n);
        costs->insert(costs->end(), c.begin(), c.begin() + n);
    }
    // manip_lattice.cpp:1012-1090: every active action's state, created without a limits or collision test; cost 1000,
    // true_cost false.  On an engine error the list stays empty, as in GetSuccs.
    void GetLazySuccs(int state_id, std::vector<int>* succs, std::vector<int>* costs, std::vector<bool>* true_costs) override
    {
        const int cap = ctx_->nprims();
        std::vector<int32_t> s(cap), c(cap);
        int n = 0;
        if (smplx_get_lazy_succs(ctx_->space(), state_id, s.data(), c.data(), cap, &n) != SMPLX_OK) {
            if (!logged_) { fprintf(stderr, "smpl_amd: GetLazySuccs(%d) failed: %s\n", state_id, smplx_last_error()); logged_ = true; }
            return;
        }
        succs->insert(succs->end(), s.begin(), s.begin() + n);
        costs->insert(costs->end(), c.begin(), c.begin() + n);
        true_costs->insert(true_costs->end(), (size_t)n, false);
    }
    // manip_lattice.cpp:1094-1167: 1000 if an action of the parent that lands in the child's cell (child == goal id: that
    // satisfies the goal) passes limits and the edge check, else -1; -1 on an engine error too (engineStatus())
    int GetTrueCost(int parent_id, int child_id) override
    {
        int32_t cost = -1;
        if (smplx_get_true_cost(ctx_->space(), parent_id, child_id, &cost) != SMPLX_OK) {
            if (!logged_) { fprintf(stderr, "smpl_amd: GetTrueCost(%d, %d) failed: %s\n", parent_id, child_id, smplx_last_error()); logged_ = true; }
            return -1;
        }
        return cost;
    }
    // not in the reference: many (parent, child) pairs in one launch; false on an engine error
    bool GetTrueCosts(const std::vector<int>& parent_ids, const std::vector<int>& child_ids, std::vector<int>* costs)
    {
        if (parent_ids.size() != child_ids.size()) return false;
        costs->assign(parent_ids.size(), -1);
        return smplx_true_cost_batch(ctx_->space(), parent_ids.data(), child_ids.data(), (int)parent_ids.size(), costs->data(), nullptr,
                                     nullptr) == SMPLX_OK;
    }
    void GetPreds(int, std::vector<int>*, std::vector<int>*) override {}   // "GetPreds unimplemented" (manip_lattice.cpp:1238-1241)
    // manip_lattice.cpp:152-197
    void PrintState(int state_id, bool /*verbose*/, FILE* f = nullptr) override
    {
        if (!f) f = stdout;
        if (state_id == getGoalStateID()) { fprintf(f, "<goal state>\n"); return; }
        RobotState q(ctx_->nvars());
        if (smplx_get_state(ctx_->space(), state_id, q.data(), nullptr) != SMPLX_OK) { fprintf(f, "<unknown state %d>\n", state_id); return; }
        fprintf(f, "{ ");
        for (size_t i = 0; i < q.size(); ++i) fprintf(f, "%.3g%s", q[i], i + 1 < q.size() ? ", " : "");
        fprintf(f, " }\n");
    }
    // the first engine error a GetSuccs call swallowed (SMPLX_OK if none)
    int engineStatus(std::string* msg = nullptr) const
    {
        char buf[512];
        const int st = smplx_space_status(ctx_->space(), buf, (int)sizeof(buf));
        if (msg) *msg = buf;
        return st;
    }
    // optional, not in the reference: ids the search will expand soon ride along in the next frontier batch
    void hintFrontier(const std::vector<int>& ids) { smplx_hint_frontier(ctx_->space(), ids.data(), (int)ids.size()); }
    bool extractPath(const std::vector<int>& ids, std::vector<RobotState>& path) override
    {
        std::vector<double> q(ids.size() * (size_t)ctx_->nvars());
        if (smplx_extract_path(ctx_->space(), ids.data(), (int)ids.size(), q.data()) != SMPLX_OK) return false;
        path.clear();
        for (size_t i = 0; i < ids.size(); ++i) path.emplace_back(q.begin() + i * ctx_->nvars(), q.begin() + (i + 1) * ctx_->nvars());
        return true;
    }
    Extension* getExtension(size_t class_code) override
    {
        return class_code == GetClassCode<RobotPlanningSpace>() ? this : nullptr;   // manip_lattice.cpp:2157-2170
    }

private:
    GpuPlanningContext* ctx_;
    bool logged_ = false;
};

// sbpl::motion::BfsHeuristic (smpl/include/smpl/heuristic/bfs_heuristic.h:49-105)
class GpuBfsHeuristic : public RobotHeuristic {
public:
    using Extension::getExtension;   // keep the typed lookup visible next to the override
    explicit GpuBfsHeuristic(GpuPlanningContext* ctx) : ctx_(ctx) {}
    // fails if the context's space was created with another kind (smplx_params.heuristic): its h would not be the BFS's
    bool init(RobotPlanningSpace* space)
    {
        return smplx_space_heuristic(ctx_->space()) == SMPLX_H_BFS && RobotHeuristic::init(space);
    }
    int GetGoalHeuristic(int state_id) override
    {
        int32_t h = 0;
        return smplx_get_goal_heuristic(ctx_->space(), state_id, &h) == SMPLX_OK ? h : 0;
    }
    int GetStartHeuristic(int) override { return 0; }         // "unimplemented" in the reference (bfs_heuristic.cpp:165-169)
    int GetFromToHeuristic(int from_id, int to_id) override                             // bfs_heuristic.cpp:171-180
    {
        return to_id == smplx_goal_id(ctx_->space()) ? GetGoalHeuristic(from_id) : 0;
    }
    // bfs_heuristic.cpp:129-138 / 103-127, served by the engine (the same values its primitive gating uses)
    double getMetricGoalDistance(double x, double y, double z) override
    {
        const double p[3] = {x, y, z};
        double d = 0.0;
        return smplx_bfs_metric_goal_distance(ctx_->space(), p, 1, &d) == SMPLX_OK ? d : 0.0;
    }
    double getMetricStartDistance(double x, double y, double z) override
    {
        const double p[3] = {x, y, z};
        double d = 0.0;
        return smplx_bfs_metric_start_distance(ctx_->space(), p, 1, &d) == SMPLX_OK ? d : 0.0;
    }
    Extension* getExtension(size_t class_code) override
    {
        return class_code == GetClassCode<RobotHeuristic>() ? this : nullptr;       // bfs_heuristic.cpp:140-146
    }

private:
    GpuPlanningContext* ctx_;
};

// sbpl::motion::EuclidDistHeuristic (smpl/include/smpl/heuristic/euclid_dist_heuristic.h:44-105) over a space created with
// smplx_params.heuristic = SMPLX_H_EUCLID.  h to the goal is the engine's (every kernel's); between two states it is the
// same arithmetic on the host (smplx_pose_distance over smplx_planning_pose_batch).  The distance is symmetric bit for bit
// (squares of the differences, the trace of the same nine products), so "from the goal" is "to the goal".
// The weight setters mirror setWeightX / Y / Z / Rot; after any of them the goal must be set again (smplx_set_euclid_weights).
// The reference's factory passes its x coefficient to all four setters (planner_interface.cpp:472-475): a quirk that is the
// caller's to copy, not this class's.
class GpuEuclidDistHeuristic : public RobotHeuristic {
public:
    using Extension::getExtension;
    explicit GpuEuclidDistHeuristic(GpuPlanningContext* ctx) : ctx_(ctx) {}
    bool init(RobotPlanningSpace* space)
    {
        return smplx_space_heuristic(ctx_->space()) == SMPLX_H_EUCLID && RobotHeuristic::init(space);
    }
    bool setWeightX(double wx) { w_[0] = wx; return push(); }
    bool setWeightY(double wy) { w_[1] = wy; return push(); }
    bool setWeightZ(double wz) { w_[2] = wz; return push(); }
    bool setWeightRot(double wr) { w_[3] = wr; return push(); }
    int GetGoalHeuristic(int state_id) override                                          // euclid_dist_heuristic.cpp:118-141
    {
        int32_t h = 0;
        return smplx_get_goal_heuristic(ctx_->space(), state_id, &h) == SMPLX_OK ? h : 0;
    }
    int GetStartHeuristic(int) override { return 0; }                                    // :161-164
    int GetFromToHeuristic(int from_id, int to_id) override                              // :166-191
    {
        const int goal = smplx_goal_id(ctx_->space());
        if (from_id == goal) return GetGoalHeuristic(to_id);
        if (to_id == goal) return GetGoalHeuristic(from_id);
        double Ta[12], Tb[12], d = 0.0;
        if (!pose(from_id, Ta) || !pose(to_id, Tb) || smplx_pose_distance(Ta, Tb, w_, &d) != SMPLX_OK) return 0;
        return (int)(1000.0 * d);
    }
    double getMetricGoalDistance(double x, double y, double z) override                  // :98-102
    {
        const double p[3] = {x, y, z};
        double d = 0.0;
        return smplx_metric_goal_distance(ctx_->space(), p, 1, &d) == SMPLX_OK ? d : 0.0;
    }
    double getMetricStartDistance(double, double, double) override { return 0.0; }       // :104-108
    Extension* getExtension(size_t class_code) override
    {
        return class_code == GetClassCode<RobotHeuristic>() ? this : nullptr;            // :110-116
    }

private:
    bool push() { return smplx_set_euclid_weights(ctx_->space(), w_) == SMPLX_OK; }
    bool pose(int id, double T[12])
    {
        std::vector<double> q((size_t)ctx_->nvars());
        return smplx_get_state(ctx_->space(), id, q.data(), nullptr) == SMPLX_OK &&
               smplx_planning_pose_batch(ctx_->space(), q.data(), 1, T) == SMPLX_OK;
    }
    GpuPlanningContext* ctx_;
    double w_[4] = {1.0, 1.0, 1.0, 1.0};                                                 // euclid_dist_heuristic.h:77-80
};

// sbpl::motion::JointDistHeuristic (smpl/include/smpl/heuristic/joint_dist_heuristic.h:44-73) over a space created with
// smplx_params.heuristic = SMPLX_H_JOINT_DIST.  Both metric distances are 0.0, as the reference's are.
class GpuJointDistHeuristic : public RobotHeuristic {
public:
    using Extension::getExtension;
    explicit GpuJointDistHeuristic(GpuPlanningContext* ctx) : ctx_(ctx) {}
    bool init(RobotPlanningSpace* space)
    {
        return smplx_space_heuristic(ctx_->space()) == SMPLX_H_JOINT_DIST && RobotHeuristic::init(space);
    }
    int GetGoalHeuristic(int state_id) override                                          // joint_dist_heuristic.cpp:70-88
    {
        int32_t h = 0;
        return smplx_get_goal_heuristic(ctx_->space(), state_id, &h) == SMPLX_OK ? h : 0;
    }
    int GetStartHeuristic(int state_id) override                                         // :90-103
    {
        const int start = smplx_start_id(ctx_->space());
        return state_id == start ? 0 : between(start, state_id);
    }
    int GetFromToHeuristic(int from_id, int to_id) override                              // :105-124
    {
        const int goal = smplx_goal_id(ctx_->space());
        if (from_id == goal) return GetGoalHeuristic(to_id);
        if (to_id == goal) return GetGoalHeuristic(from_id);
        return between(from_id, to_id);
    }
    double getMetricGoalDistance(double, double, double) override { return 0.0; }        // :52-55
    double getMetricStartDistance(double, double, double) override { return 0.0; }       // :57-60
    Extension* getExtension(size_t class_code) override
    {
        return class_code == GetClassCode<RobotHeuristic>() ? this : nullptr;            // :62-68
    }

private:
    int between(int a, int b)
    {
        const int n = ctx_->nvars();
        std::vector<double> qa((size_t)n), qb((size_t)n);
        double d = 0.0;
        if (smplx_get_state(ctx_->space(), a, qa.data(), nullptr) != SMPLX_OK || smplx_get_state(ctx_->space(), b, qb.data(), nullptr) != SMPLX_OK ||
            smplx_joint_distance(qa.data(), qb.data(), n, &d) != SMPLX_OK)
            return 0;
        return (int)(1000.0 * d);
    }
    GpuPlanningContext* ctx_;
};

// sbpl::ARAStar (smpl/include/smpl/search/arastar.h:80-165, smpl/src/search/arastar.cpp) over the engine's own search
// (smplx_replan): the same public interface, for a caller that wants the device-resident or host-driven ARA* instead of
// an ARAStar that calls GetSuccs.  The search lives in the context's space; it continues between replan calls while the
// start is unchanged (the reference's contract, arastar.h:55-78).  Return values follow the reference: replan returns 1
// on success or partial success, 0 otherwise.  (The ReplanParams overloads are not mirrored.)
class GpuARAStar {
public:
    typedef std::chrono::steady_clock clock;
    struct TimeParameters {                        // arastar.h:84-92
        bool bounded = true;
        bool improve = true;
        enum TimingType { EXPANSIONS, TIME } type = TIME;
        int max_expansions_init = 0;
        int max_expansions = 0;
        clock::duration max_allowed_time_init = clock::duration::zero();
        clock::duration max_allowed_time = clock::duration::zero();
    };

    explicit GpuARAStar(GpuPlanningContext* ctx) : ctx_(ctx) {}

    void allowPartialSolutions(bool enabled) { allow_partial_ = enabled; }
    bool allowPartialSolutions() const { return allow_partial_; }
    void setAllowedRepairTime(double allowed_time_secs) { time_params_.max_allowed_time = to_duration(allowed_time_secs); }
    double allowedRepairTime() const { return to_seconds(time_params_.max_allowed_time); }
    void setTargetEpsilon(double target_eps) { final_eps_ = std::max(target_eps, 1.0); }
    double targetEpsilon() const { return final_eps_; }
    void setDeltaEpsilon(double delta_eps) { delta_eps_ = delta_eps; }
    double deltaEpsilon() const { return delta_eps_; }
    void setImproveSolution(bool improve) { time_params_.improve = improve; }
    bool improveSolution() const { return time_params_.improve; }
    void setBoundExpansions(bool bound) { time_params_.bounded = bound; }
    bool boundExpansions() const { return time_params_.bounded; }

    int replan(const TimeParameters& params, std::vector<int>* solution, int* cost)   // arastar.cpp:107-215
    {
        time_params_ = params;
        smplx_time_params p;
        p.initial_eps = initial_eps_; p.final_eps = final_eps_; p.delta_eps = delta_eps_;
        p.improve = params.improve; p.bounded = params.bounded;
        p.type = params.type == TimeParameters::TIME ? SMPLX_TIME_WALL : SMPLX_TIME_EXPANSIONS;
        p.max_expansions_init = params.max_expansions_init; p.max_expansions = params.max_expansions;
        p.max_seconds_init = std::max(0.0, to_seconds(params.max_allowed_time_init));
        p.max_seconds = std::max(0.0, to_seconds(params.max_allowed_time));
        p.allow_partial = allow_partial_;
        p.from_scratch = from_scratch_;
        ids_.resize(1 << 16);
        smplx_replan_stats st;
        if (smplx_replan(ctx_->space(), &p, ids_.data(), (int)ids_.size(), &st) != SMPLX_OK || st.s.path_len > (int)ids_.size()) {
            from_scratch_ = 1;
            return 0;
        }
        from_scratch_ = 0;
        stats_ = st;
        if (!st.s.solved) return 0;
        if (solution) solution->assign(ids_.begin(), ids_.begin() + st.s.path_len);
        if (cost) *cost = st.s.cost;
        return 1;
    }
    int replan(double allowed_time_secs, std::vector<int>* solution)
    {
        int cost;
        return replan(allowed_time_secs, solution, &cost);
    }
    int replan(double allowed_time_secs, std::vector<int>* solution, int* cost)      // arastar.cpp:245-265
    {
        TimeParameters tparams = time_params_;
        if (tparams.max_allowed_time_init == tparams.max_allowed_time) {
            tparams.max_allowed_time_init = to_duration(allowed_time_secs);
            tparams.max_allowed_time = to_duration(allowed_time_secs);
        } else {
            tparams.max_allowed_time_init = to_duration(allowed_time_secs);   // the repair time stays
        }
        return replan(tparams, solution, cost);
    }
    int force_planning_from_scratch() { from_scratch_ = 1; return 0; }                 // arastar.cpp:380-385
    int force_planning_from_scratch_and_free_memory() { return force_planning_from_scratch(); }
    int set_search_mode(bool first_solution_unbounded) { time_params_.bounded = !first_solution_unbounded; return 0; }
    void set_initialsolution_eps(double eps) { initial_eps_ = eps; }
    double get_solution_eps() const { return stats_.s.satisfied_eps; }
    int get_n_expands() const { return stats_.s.expansions; }
    int get_n_expands_init_solution() const { return stats_.s.expansions_init; }
    double get_initial_eps() const { return initial_eps_; }
    double get_final_epsilon() const { return final_eps_; }
    const TimeParameters& timeParameters() const { return time_params_; }
    // what the last call did (SMPLX_ARA_* result, its own expansions, whether it continued the previous search)
    const smplx_replan_stats& lastCallStats() const { return stats_; }

private:
    static clock::duration to_duration(double secs)
    {
        return std::chrono::duration_cast<clock::duration>(std::chrono::duration<double>(secs));
    }
    static double to_seconds(const clock::duration& d) { return std::chrono::duration<double>(d).count(); }

    GpuPlanningContext* ctx_;
    TimeParameters time_params_;
    double initial_eps_ = 1.0, final_eps_ = 1.0, delta_eps_ = 1.0;   // arastar.cpp:58-73
    bool allow_partial_ = false;
    int from_scratch_ = 1;
    smplx_replan_stats stats_ = smplx_replan_stats();
    std::vector<int32_t> ids_;
};

// sbpl::motion::PlannerInterface::postProcessPath (smpl_ros/src/ros/planner_interface.cpp:2651-2697): ShortcutPath with
// ShortcutType::JOINT_SPACE (smpl/include/smpl/post_processing.h:49-71) between two InterpolatePath passes.  The greedy
// loops are the reference's; their collision questions are answered from waypoint-parallel GPU batches.
// upstream_limit_test = false keeps the fork's CollisionSpace::interpolatePath limit test (collision_space.cpp:592-597).
inline bool PostProcessPath(GpuPlanningContext* ctx, std::vector<RobotState>& path, bool shortcut_path, bool interpolate_path,
                            bool upstream_limit_test = false)
{
    const int N = ctx->nvars();
    std::vector<double> in(path.size() * (size_t)N);
    for (size_t i = 0; i < path.size(); ++i) std::copy(path[i].begin(), path[i].end(), in.begin() + i * N);
    const int flags = (shortcut_path ? SMPLX_PP_SHORTCUT : 0) | (interpolate_path ? SMPLX_PP_INTERPOLATE : 0) |
                      (upstream_limit_test ? SMPLX_PP_UPSTREAM_LIMITS : 0);
    int n = 0;
    if (smplx_post_process_path(ctx->space(), in.data(), (int)path.size(), flags, nullptr, 0, &n, nullptr) != SMPLX_OK) return false;
    std::vector<double> out((size_t)std::max(n, 1) * N);
    if (smplx_post_process_path(ctx->space(), in.data(), (int)path.size(), flags, out.data(), n, &n, nullptr) != SMPLX_OK) return false;
    path.clear();
    for (int i = 0; i < n; ++i) path.emplace_back(out.begin() + (size_t)i * N, out.begin() + (size_t)(i + 1) * N);
    return true;
}

// PostProcessPath for many paths in one call (smplx_post_process_paths): paths[k] is processed in ctxs[k], whose spaces
// share a grid and a robot model (a context may appear several times); every path comes out as PostProcessPath gives it.
// The shortcut loops run on the device, one workgroup a path, in a number of launches that does not depend on the batch.
// stats (may be null): the four counters of smplx_post_process_paths.
inline bool PostProcessPaths(const std::vector<GpuPlanningContext*>& ctxs, std::vector<std::vector<RobotState>>& paths,
                             bool shortcut_path, bool interpolate_path, bool upstream_limit_test = false, int64_t* stats = nullptr)
{
    if (ctxs.size() != paths.size()) return false;
    const int nq = (int)paths.size();
    if (nq == 0) return true;
    const int N = ctxs[0]->nvars();
    std::vector<smplx_space*> spaces(nq);
    std::vector<int32_t> first(nq + 1, 0), out_first(nq + 1, 0);
    for (int k = 0; k < nq; ++k) {
        if (!ctxs[k]) return false;
        spaces[k] = ctxs[k]->space();
        first[k + 1] = first[k] + (int32_t)paths[k].size();
    }
    std::vector<double> in((size_t)first[nq] * N + 1);
    for (int k = 0; k < nq; ++k)
        for (size_t i = 0; i < paths[k].size(); ++i) {
            if ((int)paths[k][i].size() != N) return false;
            std::copy(paths[k][i].begin(), paths[k][i].end(), in.begin() + ((size_t)first[k] + i) * N);
        }
    const int flags = (shortcut_path ? SMPLX_PP_SHORTCUT : 0) | (interpolate_path ? SMPLX_PP_INTERPOLATE : 0) |
                      (upstream_limit_test ? SMPLX_PP_UPSTREAM_LIMITS : 0);
    if (smplx_post_process_paths(spaces.data(), nq, in.data(), first.data(), flags, nullptr, 0, out_first.data(), nullptr) != SMPLX_OK)
        return false;
    std::vector<double> out((size_t)std::max(out_first[nq], 1) * N);
    if (smplx_post_process_paths(spaces.data(), nq, in.data(), first.data(), flags, out.data(), out_first[nq], out_first.data(), stats) !=
        SMPLX_OK)
        return false;
    for (int k = 0; k < nq; ++k) {
        paths[k].clear();
        for (int i = out_first[k]; i < out_first[k + 1]; ++i)
            paths[k].emplace_back(out.begin() + (size_t)i * N, out.begin() + (size_t)(i + 1) * N);
    }
    return true;
}

}  // namespace smpl_amd
