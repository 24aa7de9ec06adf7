// segment_main.cpp — `apd_segment`: SCAN/images/* -> SCAN/sa_masks/<stem>.bin (+ <stem>.png), the files
// the depth binary reads with --use_sa true. Where the reference runs tools/run_SAM.py (a learned
// model), this labels flat zones (include/apd_seg.h): it is not SAM and claims nothing about quality.
// Every argument and every image is checked before a device context exists (exit 2); device or write
// failures exit 1. --host runs the host twin and creates no context.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/apd_seg.h"
#include "image.h"
#include "io.h"

using namespace apdhost;

namespace {

const char *kUsage =
    "usage: apd_segment --dense_folder SCAN [options]\n"
    "  For every image of SCAN/images: flat-zone labels (include/apd_seg.h; not SAM) -> SCAN/sa_masks/<stem>.bin,\n"
    "  the uint8 bin-mat `apd --use_sa true` reads, at the working size; <stem> = the name up to its first dot.\n"
    "  --max_size N      shrink by an integer factor until the longer side is at most N; 0: never (default 2560)\n"
    "  --threshold T     grey levels two neighbours of a flat pixel may differ by after smoothing (default 1.0)\n"
    "  --min_area A      smallest region that gets a label, in working pixels (default 256)\n"
    "  --views a,b,...   only these stems\n"
    "  --host            the host twin on one thread; no device is touched\n"
    "  --no_png          without it <stem>.png shows label 0 white and label k in the header's fixed colour\n"
    "  --overwrite       without it an existing SCAN/sa_masks is refused\n"
    "  --device G        HIP device (default 0)\n"
    "  The defaults are reasoned, not tuned on photographs. Prints one JSON line.\n";

int usage_error(const std::string &msg) {
    std::cerr << "apd_segment: " << msg << "\n" << kUsage;
    return 2;
}

bool parse_int(const std::string &s, long lo, long hi, int &v) {
    char *end = nullptr;
    const long l = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || !end || *end != '\0' || l < lo || l > hi) return false;
    v = (int)l;
    return true;
}

bool is_dir(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

std::string fmt_ms(double v) {
    char b[64];
    std::snprintf(b, sizeof b, "%.6g", v);
    return b;
}

std::string json_str(const std::string &s) {
    std::string o = "\"";
    for (unsigned char c : s) {
        char b[8];
        if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
        else if (c < 0x20) { std::snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o += (char)c;
    }
    return o + "\"";
}

struct View {
    std::string file, stem;
    int W = 0, H = 0, survivors = 0, labels = 0;
};

}  // namespace

int main(int argc, char **argv) {
    std::string dense, views_arg;
    int max_size = 2560, min_area = 256, device = 0, threshold_q8 = 256;
    bool host = false, png = true, overwrite = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
        if (a == "--host") { host = true; continue; }
        if (a == "--no_png") { png = false; continue; }
        if (a == "--overwrite") { overwrite = true; continue; }
        if (i + 1 >= argc) return usage_error("missing value for " + a);
        const std::string v = argv[++i];
        bool ok = true;
        if (a == "--dense_folder") dense = v;
        else if (a == "--views") views_arg = v;
        else if (a == "--max_size") ok = parse_int(v, 0, 1 << 30, max_size);
        else if (a == "--min_area") ok = parse_int(v, 1, INT32_MAX, min_area);
        else if (a == "--device") ok = parse_int(v, 0, 1023, device);
        else if (a == "--threshold") {
            char *end = nullptr;
            const double t = std::strtod(v.c_str(), &end);
            ok = !v.empty() && end && *end == '\0' && std::isfinite(t) && t >= 0.0 && 256.0 * t <= APD_SEG_MAX_THRESHOLD_Q8;
            if (ok) threshold_q8 = (int)std::nearbyint(256.0 * t);  // to even at .5, like Python's round
        } else return usage_error("unknown option " + a);
        if (!ok) return usage_error("bad value '" + v + "' for " + a);
    }
    if (dense.empty()) return usage_error("--dense_folder is required");
    const std::string image_dir = dense + "/images", out_dir = dense + "/sa_masks";
    if (!is_dir(image_dir)) {
        std::cerr << "apd_segment: no directory " << image_dir << "\n";
        return 2;
    }
    if (file_exists(out_dir) && !overwrite) {
        std::cerr << "apd_segment: " << out_dir << " exists (pass --overwrite to replace its files)\n";
        return 2;
    }

    // ---- every input, before a device context exists ----
    std::vector<std::string> wanted;
    for (size_t p = 0; p < views_arg.size();) {
        const size_t q = std::min(views_arg.find(',', p), views_arg.size());
        if (q > p) wanted.push_back(views_arg.substr(p, q - p));
        p = q + 1;
    }
    std::vector<View> views;
    if (DIR *d = opendir(image_dir.c_str())) {
        while (const dirent *e = readdir(d)) {
            const std::string name = e->d_name;
            if (name[0] == '.' || is_dir(image_dir + "/" + name)) continue;
            View v;
            v.file = name;
            v.stem = name.substr(0, name.find('.'));
            if (!wanted.empty() && std::find(wanted.begin(), wanted.end(), v.stem) == wanted.end()) continue;
            views.push_back(v);
        }
        closedir(d);
    }
    std::sort(views.begin(), views.end(), [](const View &a, const View &b) { return a.file < b.file; });
    for (const std::string &s : wanted)
        if (std::none_of(views.begin(), views.end(), [&](const View &v) { return v.stem == s; })) {
            std::cerr << "apd_segment: no image of view " << s << " in " << image_dir << "\n";
            return 2;
        }
    for (size_t i = 1; i < views.size(); ++i)
        if (views[i].stem == views[i - 1].stem) {
            std::cerr << "apd_segment: " << views[i - 1].file << " and " << views[i].file << " would share one mask\n";
            return 2;
        }
    if (views.empty()) {
        std::cerr << "apd_segment: no images in " << image_dir << "\n";
        return 2;
    }
    for (View &v : views) {
        Bgr8 img;
        std::string err;
        if (!read_bgr8(image_dir + "/" + v.file, img, err)) {
            std::cerr << "apd_segment: " << image_dir << "/" << v.file << ": " << err << "\n";
            return 2;
        }
        if (apd_seg_working_size(img.width, img.height, max_size, nullptr, &v.W, &v.H) != APD_OK) {
            std::cerr << "apd_segment: " << v.file << ": a size the library does not take\n";
            return 2;
        }
    }

    apd_seg_ctx *ctx = nullptr;
    if (!host) {
        ctx = apd_seg_create(device);
        if (!ctx) {
            std::cerr << "apd_segment: " << apd_seg_last_error(nullptr) << "\n";
            return 1;
        }
    }
    auto fail = [&](const std::string &what) {
        std::cerr << "apd_segment: " << what << "\n";
        if (ctx) apd_seg_destroy(ctx);
        return 1;
    };
    if (!make_dir(out_dir)) return fail("cannot create " + out_dir);
    double total[APD_SEG_NUM_TIMES] = {};
    for (View &v : views) {
        Bgr8 img;
        std::string err;
        if (!read_bgr8(image_dir + "/" + v.file, img, err)) return fail(v.file + ": " + err);
        Mat labels(v.H, v.W, CV_8UC1);
        int W = 0, H = 0;
        const int st = host ? apd_seg_flat_zones_bgr8_host(img.width, img.height, img.px.data(), max_size, threshold_q8,
                                                           min_area, labels.ptr<uint8_t>(), &W, &H, &v.survivors,
                                                           &v.labels, nullptr, nullptr, nullptr, nullptr, nullptr)
                            : apd_seg_flat_zones_bgr8(ctx, img.width, img.height, img.px.data(), max_size, threshold_q8,
                                                      min_area, labels.ptr<uint8_t>(), &W, &H, &v.survivors, &v.labels);
        if (st != APD_OK || W != v.W || H != v.H)
            return fail(v.file + ": status " + std::to_string(st) + (ctx ? std::string(": ") + apd_seg_last_error(ctx) : ""));
        if (ctx) {
            double ms[APD_SEG_NUM_TIMES];
            apd_seg_get_timing(ctx, ms);
            for (int k = 0; k < APD_SEG_NUM_TIMES; ++k) total[k] += ms[k];
        }
        if (!write_binmat_file(out_dir + "/" + v.stem + ".bin", labels)) return fail("cannot write " + v.stem + ".bin");
        if (png) {
            std::vector<uint8_t> pic(3 * (size_t)W * (size_t)H);
            uint8_t lut[256][3];
            for (int k = 0; k < 256; ++k) apd_seg_label_colour(k, lut[k]);
            const uint8_t *l = labels.ptr<uint8_t>();
            for (size_t i = 0; i < (size_t)W * (size_t)H; ++i) std::memcpy(&pic[3 * i], lut[l[i]], 3);
            if (!write_png_bgr8(out_dir + "/" + v.stem + ".png", pic.data(), W, H)) return fail("cannot write " + v.stem + ".png");
        }
    }
    if (ctx) apd_seg_destroy(ctx);

    static const char *kTimes[APD_SEG_NUM_TIMES] = {"upload_ms", "downscale_ms", "smooth_flat_ms", "ccl_tile_ms", "ccl_merge_ms",
                                                    "flatten_area_ms", "rank_ms", "relabel_ms", "download_ms"};
    std::string json = "{\"views\": " + std::to_string(views.size()) + ", \"host\": " + (host ? "true" : "false") +
                       ", \"max_size\": " + std::to_string(max_size) + ", \"threshold_q8\": " + std::to_string(threshold_q8) +
                       ", \"min_area\": " + std::to_string(min_area) + ", \"per_view\": [";
    for (size_t i = 0; i < views.size(); ++i) {
        const View &v = views[i];
        json += std::string(i ? ", " : "") + "{\"view\": " + json_str(v.stem) + ", \"width\": " + std::to_string(v.W) +
                ", \"height\": " + std::to_string(v.H) + ", \"survivors\": " + std::to_string(v.survivors) +
                ", \"labels\": " + std::to_string(v.labels) + "}";
    }
    json += "], \"times_ms\": {";
    for (int k = 0; k < APD_SEG_NUM_TIMES; ++k)
        json += std::string(k ? ", " : "") + "\"" + kTimes[k] + "\": " + (host ? "null" : fmt_ms(total[k]));
    json += "}}";
    std::cout << json << std::endl;
    return 0;
}
