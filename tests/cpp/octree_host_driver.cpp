// tests/cpp/octree_host_driver.cpp -- the octree voxeliser's arithmetic (smpl_amd/csrc/octree_points.h, and the pose of
// voxelize.h) compiled by the host compiler: the source the kernels compile, run on the CPU the way the kernels use it --
// the trips of every (leaf, axis) first, then every point from its (i, j, k) alone.  Reads "ox oy oz res", 12 pose entries
// (3x4 row major), "nleaves" and nleaves x {cx cy cz size} (hexadecimal floats) from stdin.  Prints per leaf a line
// "leaf NPOINTS" and per point, in generation order, "x y z" (world frame, hexadecimal floats) and its cell "cx cy cz".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../smpl_amd/csrc/octree_points.h"
#include "../../smpl_amd/csrc/voxelize.h"

static double read_double()
{
    char tok[128];
    if (std::scanf("%127s", tok) != 1) std::exit(2);
    return std::strtod(tok, nullptr);
}

int main()
{
    double o[3], pose[12];
    for (double& x : o) x = read_double();
    const double res = read_double();
    for (double& x : pose) x = read_double();
    const int nleaves = (int)read_double();
    std::vector<double> leaves((size_t)nleaves * 4);
    for (double& x : leaves) x = read_double();
    const double inv_res = 1.0 / res;
    double omr[3];
    for (int a = 0; a < 3; ++a) omr[a] = o[a] - res;
    for (int l = 0; l < nleaves; ++l) {
        const double* L = &leaves[4 * (size_t)l];
        int t[3];
        for (int a = 0; a < 3; ++a) t[a] = oct_single(L[3], res) ? 1 : oct_axis_trips(L[a], L[3], res);
        if (t[0] > oct_axis_bound(L[3], res) || t[1] > oct_axis_bound(L[3], res) || t[2] > oct_axis_bound(L[3], res)) return 3;
        const long long n = (long long)t[0] * t[1] * t[2];
        std::printf("leaf %lld\n", n);
        for (long long p = 0; p < n; ++p) {
            const int k[3] = {(int)(p / ((long long)t[2] * t[1])), (int)(p / t[2] % t[1]), (int)(p % t[2])};
            const double v[3] = {oct_axis_value(L[0], L[3], res, k[0]), oct_axis_value(L[1], L[3], res, k[1]), oct_axis_value(L[2], L[3], res, k[2])};
            double w[3];
            vox_transform(pose, v, w);
            std::printf("%a %a %a %d %d %d\n", w[0], w[1], w[2], oct_world_to_cell(w[0], omr[0], inv_res), oct_world_to_cell(w[1], omr[1], inv_res),
                        oct_world_to_cell(w[2], omr[2], inv_res));
        }
    }
    return 0;
}
