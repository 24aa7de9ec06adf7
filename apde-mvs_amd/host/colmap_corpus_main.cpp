// colmap_corpus_main.cpp — runs read_colmap_model and colmap_prep_arrays (io.cpp) over a list of
// (possibly corrupt) COLMAP model directories. Built with AddressSanitizer + UndefinedBehaviorSanitizer
// by `make sanitize-colmap` (tests/test_prep_host.py): every model must be either read or rejected
// with a message, never read out of bounds. An accepted model is written back (cameras.txt,
// images.txt into <dir>/back) and read again. Links no device library.
//   colmap_corpus_main (<dir> <.txt|.bin>)...
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "io.h"

int main(int argc, char **argv) {
    int ok = 0, rejected = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        apdhost::ColmapModel m, back;
        apdhost::PrepArrays a;
        std::string err;
        if (!apdhost::read_colmap_model(argv[i], argv[i + 1], m, err) || !apdhost::colmap_prep_arrays(m, a, err)) {
            if (err.empty()) { std::printf("BAD rejection %s\n", argv[i]); return 2; }
            ++rejected;
            continue;
        }
        if (m.images.empty() || a.obs_offset.size() != m.images.size() + 1 || a.rot.size() != 9 * m.images.size() ||
            (size_t)a.obs_offset.back() != a.obs_point.size()) {
            std::printf("BAD arrays %s\n", argv[i]);
            return 2;
        }
        for (int32_t p : a.obs_point)
            if (p < 0 || (size_t)p >= m.point_ids.size()) { std::printf("BAD index %s\n", argv[i]); return 2; }
        const std::string out = std::string(argv[i]) + "/back";
        if (!apdhost::make_dir(out) || !apdhost::write_colmap_cameras_txt(out + "/cameras.txt", m.cameras) ||
            !apdhost::write_colmap_images_txt(out + "/images.txt", m.images) ||
            !apdhost::copy_file(std::string(argv[i]) + "/points3D" + argv[i + 1], out + "/points3D" + argv[i + 1])) {
            std::printf("BAD write %s\n", out.c_str());
            return 2;
        }
        if (std::string(argv[i + 1]) == ".txt") {
            if (!apdhost::read_colmap_model(out, ".txt", back, err) || back.images.size() != m.images.size() ||
                back.cameras.size() != m.cameras.size()) {
                std::printf("BAD round trip %s: %s\n", out.c_str(), err.c_str());
                return 2;
            }
            for (size_t k = 0; k < m.images.size(); ++k)
                if (memcmp(back.images[k].q, m.images[k].q, sizeof m.images[k].q) != 0 ||
                    memcmp(back.images[k].t, m.images[k].t, sizeof m.images[k].t) != 0 ||
                    back.images[k].point_ids != m.images[k].point_ids || back.images[k].xy != m.images[k].xy) {
                    std::printf("BAD round trip values %s\n", out.c_str());
                    return 2;
                }
        }
        ++ok;
    }
    std::printf("colmap corpus: %d read, %d rejected\n", ok, rejected);
    return 0;
}
