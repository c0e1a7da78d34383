// tests/cpp/object_spheres_host_driver.cpp -- the host side of an attached object's sphere model
// (smpl_amd/csrc/object_spheres.h over smpl_amd/csrc/voxelize.h) compiled by the host compiler: the bounding box and index
// range of every mesh, the voxeliser's arithmetic over every candidate voxel inside the range, and the sphere rows.
// Reads "radius nshapes", then per shape "nvertices ntriangles", the vertices (already at the shape's pose, hexadecimal
// floats) and the index triples from stdin.  Prints per shape "shape k count lo0 lo1 lo2 hi0 hi1 hi2" (the index range),
// then one "x y z r" row per filled voxel as hexadecimal floats, each voxel once, x-major / z fastest.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <set>
#include <tuple>
#include <vector>

#include "../../smpl_amd/csrc/object_spheres.h"

static double read_double()
{
    char tok[128];
    if (std::scanf("%127s", tok) != 1) std::exit(2);
    return std::strtod(tok, nullptr);
}

int main()
{
    using namespace smplx_object_host;
    const double radius = read_double();
    const int nshapes = (int)read_double();
    const double res = resolution(radius);
    for (int s = 0; s < nshapes; ++s) {
        const int nv = (int)read_double(), nt = (int)read_double();
        if (nv < 1 || nt < 0) return 2;
        std::vector<double> v((size_t)nv * 3);
        for (double& x : v) x = read_double();
        std::vector<int> t((size_t)nt * 3);
        for (int& i : t) { i = (int)read_double(); if (i < 0 || i >= nv) return 2; }
        int clip[6];
        clip_range(v.data(), (size_t)nv, res, clip);
        if (range_cells(clip) > kMaxRangeCells) return 3;
        std::set<std::tuple<int, int, int>> cells;
        for (int k = 0; k < nt; ++k) {
            const double* p[3] = {&v[3 * (size_t)t[3 * k]], &v[3 * (size_t)t[3 * k + 1]], &v[3 * (size_t)t[3 * k + 2]]};
            VoxTri T;
            if (!vox_tri_setup(p[0], p[1], p[2], res, &T)) continue;
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                const double mn = std::min(p[0][a], std::min(p[1][a], p[2][a])), mx = std::max(p[0][a], std::max(p[1][a], p[2][a]));
                lo[a] = std::max(clip[a], vox_discretize_in(mn, 0.0, res, clip[a], clip[3 + a]));
                hi[a] = std::min(clip[3 + a], vox_discretize_in(mx, 0.0, res, clip[a], clip[3 + a]));
            }
            for (int x = lo[0]; x <= hi[0]; ++x)
                for (int y = lo[1]; y <= hi[1]; ++y)
                    for (int z = lo[2]; z <= hi[2]; ++z) {
                        const double w[3] = {vox_continuize(x, 0.0, res), vox_continuize(y, 0.0, res), vox_continuize(z, 0.0, res)};
                        if (vox_filled(T, w)) cells.insert(std::make_tuple(x, y, z));
                    }
        }
        std::printf("shape %d %d %d %d %d %d %d %d\n", s, (int)cells.size(), clip[0], clip[1], clip[2], clip[3], clip[4], clip[5]);
        for (const auto& c : cells) {
            const int cell[3] = {std::get<0>(c), std::get<1>(c), std::get<2>(c)};
            double row[4];
            sphere_row(cell, res, radius, row);
            std::printf("%a %a %a %a\n", row[0], row[1], row[2], row[3]);
        }
    }
    return 0;
}
