// mat_corpus_main.cpp — runs read_mat5 of io.cpp over a list of (possibly corrupt) Level-5 MAT-files.
// Built with AddressSanitizer + UndefinedBehaviorSanitizer by `make sanitize-mat`
// (tests/test_eval_dtu_host.py): every file must be either read or rejected with a message, never
// read out of bounds. Links no device library.
//   mat_corpus_main [--dump] [--want NAME | --mask NAME]... <file>...
// The names asked of every file (default: ObsMask as a mask, BB, Res, P as values). --dump prints one
// JSON line per file that was read: the arrays as the reader understood them (a file name is printed
// as it is, so it must need no escaping). A non-finite value is printed as printf prints it.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "io.h"

int main(int argc, char **argv) {
    std::vector<apdhost::MatWanted> wanted;
    std::vector<std::string> files;
    bool dump = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if ((a == "--want" || a == "--mask") && i + 1 < argc) wanted.push_back({argv[++i], a == "--mask"});
        else if (a == "--dump") dump = true;
        else files.push_back(a);
    }
    if (wanted.empty()) wanted = {{"ObsMask", true}, {"BB", false}, {"Res", false}, {"P", false}};
    int ok = 0, rejected = 0;
    for (const std::string &path : files) {
        std::string err;
        std::vector<apdhost::MatArray> arrays;
        // every wanted name singly as well, so that a file holding only some of them is still read
        for (size_t k = 0; k <= wanted.size(); ++k) {
            const std::vector<apdhost::MatWanted> ask =
                k == wanted.size() ? wanted : std::vector<apdhost::MatWanted>{wanted[k]};
            err.clear();
            const bool good = apdhost::read_mat5(path, ask, arrays, err);
            if (good) {
                // touch every value so a short buffer shows up under ASan
                double sum = 0.0;
                if (arrays.size() != ask.size()) { std::printf("BAD count %s\n", path.c_str()); return 2; }
                for (size_t j = 0; j < arrays.size(); ++j) {
                    const apdhost::MatArray &a = arrays[j];
                    uint64_t count = 1;
                    for (int64_t d : a.dims) count *= (uint64_t)d;
                    const size_t have = ask[j].as_mask ? a.bytes.size() : a.values.size();
                    if (a.dims.empty() || a.dims.size() > 3 || have != count || a.name != ask[j].name) {
                        std::printf("BAD array %s\n", path.c_str());
                        return 2;
                    }
                    for (double v : a.values) sum += std::isfinite(v) ? v : 0.0;
                    for (uint8_t v : a.bytes) sum += v;
                }
                if (!std::isfinite(sum)) { std::printf("BAD sum %s\n", path.c_str()); return 2; }
                if (k == wanted.size()) ++ok;
                if (k == wanted.size() && dump) {  // one JSON line per file: what the reader understood
                    std::printf("{\"file\": \"%s\", \"arrays\": [", path.c_str());
                    for (size_t j = 0; j < arrays.size(); ++j) {
                        const apdhost::MatArray &a = arrays[j];
                        std::printf("%s{\"name\": \"%s\", \"logical\": %s, \"dims\": [", j ? ", " : "", a.name.c_str(),
                                    a.logical ? "true" : "false");
                        for (size_t d = 0; d < a.dims.size(); ++d) std::printf("%s%lld", d ? ", " : "", (long long)a.dims[d]);
                        std::printf("], \"values\": [");
                        for (size_t i = 0; i < a.values.size(); ++i) std::printf("%s%.17g", i ? ", " : "", a.values[i]);
                        for (size_t i = 0; i < a.bytes.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)a.bytes[i]);
                        std::printf("]}");
                    }
                    std::printf("]}\n");
                }
            } else if (err.empty() || !arrays.empty()) {
                std::printf("BAD rejection %s\n", path.c_str());
                return 2;
            } else if (k == wanted.size()) {
                ++rejected;
            }
        }
    }
    std::printf("mat corpus: %d read, %d rejected\n", ok, rejected);
    return 0;
}
