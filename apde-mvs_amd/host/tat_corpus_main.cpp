// tat_corpus_main.cpp — runs read_tat_crop (files named *.json) and read_matrix4 (everything else) of
// io.cpp over a list of (possibly corrupt) files. Built with AddressSanitizer +
// UndefinedBehaviorSanitizer by `make sanitize-tat` (tests/test_eval_register_host.py): every file must
// be either read or rejected with a message, never read out of bounds. Links no device library.
//   tat_corpus_main <file>...
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "io.h"

int main(int argc, char **argv) {
    int ok = 0, rejected = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string path = argv[i];
        std::string err;
        const bool json = path.size() >= 5 && path.compare(path.size() - 5, 5, ".json") == 0;
        bool good;
        if (json) {
            apdhost::TatCrop crop;
            good = apdhost::read_tat_crop(path, crop, err);
            if (good) {
                // touch every value so a short buffer shows up under ASan
                const std::vector<double> uv = crop.polygon();
                double sum = crop.axis_min + crop.axis_max;
                for (double v : uv) sum += v;
                if (uv.size() < 6 || uv.size() * 3 != crop.vertices.size() * 2 || crop.axis < 0 || crop.axis > 2 ||
                    !std::isfinite(sum)) {
                    std::printf("BAD crop %s\n", argv[i]);
                    return 2;
                }
            } else if (!crop.vertices.empty()) {
                std::printf("BAD rejection %s\n", argv[i]);
                return 2;
            }
        } else {
            double M[16];
            good = apdhost::read_matrix4(path, M, err);
            if (good) {
                double sum = 0.0;
                for (double v : M) sum += v;
                if (!std::isfinite(sum)) { std::printf("BAD matrix %s\n", argv[i]); return 2; }
            }
        }
        if (good) ++ok;
        else if (err.empty()) { std::printf("BAD rejection %s\n", argv[i]); return 2; }
        else ++rejected;
    }
    std::printf("tat corpus: %d read, %d rejected\n", ok, rejected);
    return 0;
}
