// ply_corpus_main.cpp — runs read_ply_xyz (io.cpp) over a list of (possibly corrupt) files. Built
// with AddressSanitizer + UndefinedBehaviorSanitizer by `make sanitize-ply`
// (tests/test_eval_host.py): every file must be either read or rejected with a message, never read
// out of bounds. Links no device library.
//   ply_corpus_main <file>...
#include <cstdio>
#include <string>
#include <vector>

#include "io.h"

int main(int argc, char **argv) {
    int ok = 0, rejected = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<float> xyz;
        std::string err;
        if (apdhost::read_ply_xyz(argv[i], xyz, err)) {
            // touch every value so a short buffer shows up under ASan
            unsigned sum = 0;
            for (float v : xyz) sum += v > 0.0f;
            if (xyz.size() % 3 != 0) { std::printf("BAD size %s\n", argv[i]); return 2; }
            if (sum == 0xFFFFFFFFu) std::printf(".");
            ++ok;
        } else {
            if (err.empty() || !xyz.empty()) { std::printf("BAD rejection %s\n", argv[i]); return 2; }
            ++rejected;
        }
    }
    std::printf("ply corpus: %d read, %d rejected\n", ok, rejected);
    return 0;
}
