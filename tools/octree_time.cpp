// tools/octree_time.cpp -- the measurement of octree world objects (profiles/octree_ab.txt records it), driven by
// tools/octree_time.py.  argv: a file of leaf rows (binary doubles, 4 a leaf), the 12 pose entries, the repetitions.
// Grid 256^3 at 0.02 m, max_dist 0.2 m, as tools/voxelize_time.py.  Per repetition, alternating:
//   insert_ms       smplx_world_insert_object of the octree (leaf rows up, everything else on the device, field update)
//   remove_ms       smplx_world_remove_object
//   expand_ms       the only route the engine offered before: the reference's loops (voxel_operations.cpp:405-436) and the
//                   pose run on the host, here in C++ ...
//   add_points_ms   ... and the points handed to smplx_grid_add_points on the same grid (cells on the host, the cell list up,
//                   field update)
//   kernels_ms      HIP events inside the library around the launches of one insert's voxelisation, in a call of its own
// Host clock around synchronous calls.  Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <smpl_amd.h>

extern "C" void smplx_test_voxelize_timing(int on);
extern "C" double smplx_test_voxelize_kernel_ms(void);

static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static void expand(const std::vector<double>& leaves, const double* P, double res, std::vector<double>& out)
{
    out.clear();
    auto put = [&](double x, double y, double z) {
        for (int r = 0; r < 3; ++r) out.push_back(P[4 * r] * x + (P[4 * r + 1] * y + P[4 * r + 2] * z) + P[4 * r + 3]);
    };
    for (size_t l = 0; l + 3 < leaves.size(); l += 4) {
        const double cx = leaves[l], cy = leaves[l + 1], cz = leaves[l + 2], size = leaves[l + 3];
        if (size <= res) { put(cx, cy, cz); continue; }
        const double c = std::ceil(size / res) * res;
        for (double x = cx - c; x < cx + c; x += res)
            for (double y = cy - c; y < cy + c; y += res)
                for (double z = cz - c; z < cz + c; z += res) put(x, y, z);
    }
}

static void line(const char* name, std::vector<double> v, bool last = false)
{
    std::sort(v.begin(), v.end());
    std::printf("\"%s\": {\"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, \"calls\": %zu}%s", name, v[v.size() / 2], v.front(), v.back(), v.size(),
                last ? "" : ", ");
}

int main(int argc, char** argv)
{
    if (argc < 15) return 2;
    std::vector<double> leaves;
    if (FILE* f = std::fopen(argv[1], "rb")) {
        double row[4];
        while (std::fread(row, sizeof(double), 4, f) == 4) leaves.insert(leaves.end(), row, row + 4);
        std::fclose(f);
    }
    if (leaves.empty()) return 2;
    smplx_shape s = {};
    s.type = SMPLX_SHAPE_OCTREE;
    for (int k = 0; k < 12; ++k) s.pose[k] = std::atof(argv[2 + k]);
    s.vertices = leaves.data();
    s.nvertices = (int32_t)(leaves.size() / 4);
    const int reps = std::atoi(argv[14]), warm = 3;
    const double origin[3] = {-1.0, -2.5, 0.0}, res = 0.02;
    smplx_grid* g = nullptr;
    if (smplx_grid_create_empty(origin, 256, 256, 256, res, 0.2, &g) != SMPLX_OK) { std::fprintf(stderr, "%s\n", smplx_last_error()); return 1; }
    std::vector<double> ins, rem, exp_ms, add, route, ker, pts;
    int ncells = 0;
    long long window = 0;
    for (int r = 0; r < reps + warm; ++r) {
        double t0 = now_ms();
        if (smplx_world_insert_object(g, "map", &s, 1) != SMPLX_OK) { std::fprintf(stderr, "%s\n", smplx_last_error()); return 1; }
        const double t_ins = now_ms() - t0;
        window = smplx_grid_last_edit_cells(g);
        (void)smplx_world_object_cells(g, "map", 0, nullptr, 0, &ncells);
        t0 = now_ms();
        if (smplx_world_remove_object(g, "map") != SMPLX_OK) return 1;
        const double t_rem = now_ms() - t0;
        t0 = now_ms();
        expand(leaves, s.pose, res, pts);
        const double t_exp = now_ms() - t0;
        t0 = now_ms();
        if (smplx_grid_add_points(g, pts.data(), (int)(pts.size() / 3)) != SMPLX_OK) return 1;
        const double t_add = now_ms() - t0;
        if (smplx_grid_remove_points(g, pts.data(), (int)(pts.size() / 3)) != SMPLX_OK) return 1;
        smplx_test_voxelize_timing(1);
        if (smplx_world_insert_object(g, "map", &s, 1) != SMPLX_OK) return 1;
        const double t_ker = smplx_test_voxelize_kernel_ms();
        smplx_test_voxelize_timing(0);
        if (smplx_world_remove_object(g, "map") != SMPLX_OK) return 1;
        if (r < warm) continue;
        ins.push_back(t_ins); rem.push_back(t_rem); exp_ms.push_back(t_exp); add.push_back(t_add); route.push_back(t_exp + t_add); ker.push_back(t_ker);
    }
    std::printf("{\"measure\": \"octree\", \"grid\": [256, 256, 256], \"res\": %g, \"leaves\": %d, \"points\": %zu, \"cells_in_grid\": %d, "
                "\"insert_window_cells\": %lld, \"leaf_bytes\": %zu, \"point_bytes\": %zu, ",
                res, (int)s.nvertices, pts.size() / 3, ncells, window, leaves.size() * sizeof(double), pts.size() * sizeof(double));
    line("insert_ms", ins); line("kernels_ms", ker); line("remove_ms", rem); line("expand_ms", exp_ms); line("add_points_ms", add);
    line("expand_plus_add_points_ms", route, true);
    std::printf("}\n");
    smplx_grid_destroy(g);
    return 0;
}
