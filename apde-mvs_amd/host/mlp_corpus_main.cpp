// mlp_corpus_main.cpp — runs read_mlp, mlp_to_world and write_ply_xyz_rgb (io.cpp) over a list of
// (possibly corrupt) MeshLab project files. Built with AddressSanitizer + UndefinedBehaviorSanitizer
// by `make sanitize-mlp` (tests/test_eval_protocol_host.py): every file must be either read or
// rejected with a message, never read out of bounds. For every mesh of an accepted project whose
// PLY can be read, the world points are written as a coloured cloud next to the project
// (<project>.<mesh>.rgb.ply) and read back. Links no device library.
//   mlp_corpus_main <file>...
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "io.h"

int main(int argc, char **argv) {
    int ok = 0, rejected = 0, clouds = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<apdhost::MlpMesh> meshes;
        std::string err;
        if (!apdhost::read_mlp(argv[i], meshes, err)) {
            if (err.empty() || !meshes.empty()) { std::printf("BAD rejection %s\n", argv[i]); return 2; }
            ++rejected;
            continue;
        }
        if (meshes.empty()) { std::printf("BAD empty %s\n", argv[i]); return 2; }
        ++ok;
        for (size_t m = 0; m < meshes.size(); ++m) {
            if (meshes[m].M[15] != 1.0 || meshes[m].ply_path.empty()) { std::printf("BAD mesh %s\n", argv[i]); return 2; }
            std::vector<float> xyz, back;
            if (!apdhost::read_ply_xyz(meshes[m].ply_path, xyz, err)) continue;
            float origin[3];
            apdhost::mlp_to_world(meshes[m], xyz, origin);
            std::vector<uint8_t> rgb(xyz.size());
            for (size_t k = 0; k < rgb.size(); ++k) rgb[k] = (uint8_t)(k * 7);
            const std::string out = std::string(argv[i]) + "." + std::to_string(m) + ".rgb.ply";
            if (!apdhost::write_ply_xyz_rgb(out, xyz, rgb) || !apdhost::read_ply_xyz(out, back, err) ||
                back.size() != xyz.size() || (!xyz.empty() && memcmp(back.data(), xyz.data(), xyz.size() * 4) != 0)) {
                std::printf("BAD round trip %s\n", out.c_str());
                return 2;
            }
            ++clouds;
        }
    }
    std::printf("mlp corpus: %d read, %d rejected, %d clouds written\n", ok, rejected, clouds);
    return 0;
}
