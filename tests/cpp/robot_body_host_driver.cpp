// tests/cpp/robot_body_host_driver.cpp -- the robot body's parser, kinematics and dirtiness (smpl_amd/csrc/robot_body.h) and
// the HalfRes lattice (smpl_amd/csrc/voxelize.h) compiled by the host compiler: the source the library compiles, run on
// the CPU.  argv[1] is a file holding a body text.  A text that is refused prints "error CODE TEXT" and the program ends
// with status 0 (so a sanitizer's report is the only way it fails).  Otherwise it prints "ok LINKS JOINTS MODELS" and
// then answers the commands on stdin:
//     set JOINT Q      smplx_body_host::set_joint (Q a hexadecimal float); prints "set CODE"
//     transforms       one line of nlinks x 12 hexadecimal floats
//     dirty            one line of per-model flags
//     put              clears the flags of the outside models, as a put does; prints their indices
//     disc D RES       vox_half_discretize
//     cont I RES       vox_continuize(I, 0.5 * RES, RES) as a hexadecimal float
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>

#include "../../smpl_amd/csrc/robot_body.h"
#include "../../smpl_amd/csrc/voxelize.h"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) return 2;
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    smplx_body_host::Body b;
    std::string err;
    const int rc = smplx_body_host::parse_body_text(text.c_str(), b, err);
    if (rc != SMPLX_OK) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
    std::printf("ok %zu %zu %zu\n", b.links.size(), b.joints.size(), b.models.size());
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "set") {
            std::string j, q;
            std::cin >> j >> q;
            std::printf("set %d\n", smplx_body_host::set_joint(b, j.c_str(), std::strtod(q.c_str(), nullptr), err));
        } else if (cmd == "transforms") {
            std::vector<double> T(12 * b.links.size());
            smplx_body_host::link_transforms(b, T.data());
            for (double x : T) std::printf("%a ", x);
            std::printf("\n");
        } else if (cmd == "dirty") {
            for (unsigned char d : b.dirty) std::printf("%d ", (int)d);
            std::printf("\n");
        } else if (cmd == "put") {
            for (size_t m = 0; m < b.models.size(); ++m)
                if (b.models[m].outside && b.dirty[m]) { b.dirty[m] = 0; std::printf("%zu ", m); }
            std::printf("\n");
        } else if (cmd == "disc") {
            std::string d, r;
            std::cin >> d >> r;
            std::printf("%d\n", vox_half_discretize(std::strtod(d.c_str(), nullptr), std::strtod(r.c_str(), nullptr)));
        } else if (cmd == "cont") {
            int i;
            std::string r;
            std::cin >> i >> r;
            const double res = std::strtod(r.c_str(), nullptr);
            std::printf("%a\n", vox_continuize(i, 0.5 * res, res));
        } else {
            return 3;
        }
    }
    return 0;
}
