// eval_main.cpp — `apd_eval`: accuracy / completeness / F1 of a fused cloud against a ground-truth
// cloud (cloud mode, on the GPU through include/apd_eval.h) and agreement of two sets of depth maps
// (depth mode, host only). It stands where the reference calls an external evaluator
// (tools/eval_eth_train.py), with the plain nearest-neighbour definition: the ETH3D tool's
// free-space and visibility handling is not modelled.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/apd_eval.h"
#include "io.h"

using namespace apdhost;

namespace {

const char *kHelp =
    "apd_eval - evaluate apd's results\n"
    "\n"
    "cloud mode (uses the GPU):\n"
    "  apd_eval --cloud REC.ply --gt GT.ply [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--max_dist D]\n"
    "           [--voxel V] [--gpu_index G] [--json OUT.json]\n"
    "  R and G are the two clouds after dropping non-finite points and, for V > 0, keeping the\n"
    "  lowest-index point of every V-sized voxel of each cloud. Per tolerance t:\n"
    "    accuracy = #{dist(R_i, G) <= t} / |R|, completeness = #{dist(G_j, R) <= t} / |G|,\n"
    "    F1 = 2ac / (a + c); each ratio is 0 when its denominator is 0.\n"
    "  Distances are plain nearest-neighbour distances truncated at D (default: the largest\n"
    "  tolerance). This is the DTU-style definition: the ETH3D evaluation's free-space and\n"
    "  visibility handling is NOT modelled, so the numbers compare runs of this project with each\n"
    "  other, not with published ETH3D tables.\n"
    "\n"
    "depth mode (host only):\n"
    "  apd_eval --dense_folder A (--against B | --gt_depth DIR) [--json OUT.json]\n"
    "  For every reference view of A/pair.txt compares A/APD/<id>/depths.bin + weak.bin with\n"
    "  B/APD/<id>/depths.bin + weak.bin, or with DIR/<id>.bin (CV_32FC1, valid where depth > 0).\n"
    "  valid = depth > 0 and weak != UNKNOWN. Reports valid pixels per side and in both, pixels\n"
    "  whose validity agrees, and among pixels valid in both the counts with |da - db| <= 1e-3 db\n"
    "  and <= 1e-2 db and the lower median of |da - db| / db.\n"
    "\n"
    "Both modes may be combined in one invocation; --json then holds both.\n"
    "Exit status: 0 ok, 1 run-time failure, 2 bad arguments or unreadable input.\n";

struct Options {
    std::string cloud, gt, json, dense, against, gt_depth;
    std::vector<float> tol = {0.01f, 0.02f, 0.05f, 0.1f, 0.2f, 0.5f};
    float max_dist = -1.0f;  // < 0: the largest tolerance
    float voxel = 0.0f;
    int gpu = 0;
};

bool parse_float(const std::string &s, float &v) {
    char *end = nullptr;
    v = std::strtof(s.c_str(), &end);
    return !s.empty() && end && *end == '\0';
}

std::string fmt_g(double v) {
    char b[64];
    if (std::isfinite(v)) std::snprintf(b, sizeof b, "%.17g", v);
    else std::snprintf(b, sizeof b, "null");
    return b;
}

// the shortest decimal that reads back as the same float (0.01f prints as 0.01)
std::string fmt_f32(float v) {
    char b[64];
    for (int p = 1; p <= 9; ++p) {
        std::snprintf(b, sizeof b, "%.*g", p, (double)v);
        if (std::strtof(b, nullptr) == v) break;
    }
    return b;
}

template <class T, class F> std::string join(const std::vector<T> &v, F f, const char *sep = ", ") {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? sep : "") + f(v[i]);
    return s;
}

// ---- cloud mode ---------------------------------------------------------------------------------

struct Direction {
    std::vector<int64_t> within;
    int64_t n = 0, inf = 0;
    double mean = 0.0, build_ms = 0.0, query_ms = 0.0;
};

struct CloudInfo {
    std::vector<float> xyz;
    int64_t points_in = 0, points_finite = 0, points = 0;
};

void drop_non_finite(CloudInfo &c) {
    c.points_in = (int64_t)(c.xyz.size() / 3);
    size_t o = 0;
    for (size_t i = 0; i + 2 < c.xyz.size(); i += 3)
        if (std::isfinite(c.xyz[i]) && std::isfinite(c.xyz[i + 1]) && std::isfinite(c.xyz[i + 2])) {
            for (int a = 0; a < 3; ++a) c.xyz[o + a] = c.xyz[i + a];
            o += 3;
        }
    c.xyz.resize(o);
    c.points_finite = c.points = (int64_t)(o / 3);
}

bool fail_ctx(apd_eval_ctx *ctx, const char *what, int st) {
    std::fprintf(stderr, "apd_eval: %s failed (%d): %s\n", what, st, apd_eval_last_error(ctx));
    return false;
}

bool downsample(apd_eval_ctx *ctx, CloudInfo &c, float voxel) {
    const int64_t n = c.points;
    std::vector<int32_t> keep((size_t)std::max<int64_t>(n, 1));
    int64_t nk = 0;
    const int st = apd_eval_voxel_downsample(ctx, n, c.xyz.data(), voxel, keep.data(), &nk);
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_voxel_downsample", st);
    std::vector<float> out((size_t)nk * 3);
    for (int64_t i = 0; i < nk; ++i)
        for (int a = 0; a < 3; ++a) out[3 * (size_t)i + a] = c.xyz[3 * (size_t)keep[(size_t)i] + a];
    c.xyz.swap(out);
    c.points = nk;
    return true;
}

bool direction(apd_eval_ctx *ctx, const CloudInfo &q, const CloudInfo &t, const Options &opt, float max_dist,
               Direction &d) {
    int st = apd_eval_set_target(ctx, t.points, t.xyz.data());
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_set_target", st);
    std::vector<float> dist((size_t)q.points);
    d.within.assign(opt.tol.size(), 0);
    st = apd_eval_distances(ctx, q.points, q.xyz.data(), max_dist, dist.data(), (int32_t)opt.tol.size(), opt.tol.data(),
                            d.within.data());
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_distances", st);
    double voxel_ms = 0.0;
    apd_eval_get_timing(ctx, &d.build_ms, &d.query_ms, &voxel_ms);
    d.n = q.points;
    double sum = 0.0;
    int64_t fin = 0;
    for (float v : dist)  // in index order, in double
        if (std::isfinite(v)) {
            sum += (double)v;
            ++fin;
        }
    d.inf = d.n - fin;
    d.mean = fin ? sum / (double)fin : 0.0;
    return true;
}

std::string json_cloud(const CloudInfo &c) {
    return "{\"points_in\": " + std::to_string(c.points_in) + ", \"points_finite\": " + std::to_string(c.points_finite) +
           ", \"points\": " + std::to_string(c.points) + "}";
}

std::string json_direction(const Direction &d) {
    auto ratio = [&](int64_t w) { return fmt_g(d.n ? (double)w / (double)d.n : 0.0); };
    return "{\"points\": " + std::to_string(d.n) + ", \"within\": [" +
           join(d.within, [](int64_t w) { return std::to_string(w); }) + "], \"ratio\": [" + join(d.within, ratio) +
           "], \"inf\": " + std::to_string(d.inf) + ", \"mean\": " + fmt_g(d.mean) + ", \"build_ms\": " +
           fmt_g(d.build_ms) + ", \"query_ms\": " + fmt_g(d.query_ms) + "}";
}

// returns the exit status; appends "cloud": {...} to json
int run_cloud(const Options &opt, std::string &json) {
    CloudInfo rec, gt;
    std::string err;
    // both files are parsed before any device context exists: a malformed file fails without a GPU
    if (!read_ply_xyz(opt.cloud, rec.xyz, err) || !read_ply_xyz(opt.gt, gt.xyz, err)) {
        std::fprintf(stderr, "apd_eval: %s\n", err.c_str());
        return 2;
    }
    drop_non_finite(rec);
    drop_non_finite(gt);
    const float max_dist = opt.max_dist >= 0.0f ? opt.max_dist : *std::max_element(opt.tol.begin(), opt.tol.end());
    apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
    if (!ctx) {
        std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
        return 1;
    }
    Direction acc, comp;
    bool ok = true;
    if (opt.voxel > 0.0f) ok = downsample(ctx, rec, opt.voxel) && downsample(ctx, gt, opt.voxel);
    ok = ok && direction(ctx, rec, gt, opt, max_dist, acc) && direction(ctx, gt, rec, opt, max_dist, comp);
    apd_eval_destroy(ctx);
    if (!ok) return 1;

    const size_t k = opt.tol.size();
    std::vector<double> a(k), c(k), f(k);
    for (size_t i = 0; i < k; ++i) {
        a[i] = acc.n ? (double)acc.within[i] / (double)acc.n : 0.0;
        c[i] = comp.n ? (double)comp.within[i] / (double)comp.n : 0.0;
        f[i] = a[i] + c[i] > 0.0 ? 2.0 * a[i] * c[i] / (a[i] + c[i]) : 0.0;
    }
    auto six = [](double v) {
        char b[64];
        std::snprintf(b, sizeof b, "%.6f", v);
        return std::string(b);
    };
    std::printf("Tolerances: %s\n", join(opt.tol, fmt_f32, " ").c_str());
    std::printf("Completenesses: %s\n", join(c, six, " ").c_str());
    std::printf("Accuracies: %s\n", join(a, six, " ").c_str());
    std::printf("F1-scores: %s\n", join(f, six, " ").c_str());
    json += "\"cloud\": {\"definition\": \"plain nearest neighbour (no free-space / visibility model)\", "
            "\"tolerances\": [" + join(opt.tol, fmt_f32) + "], \"max_dist\": " +
            fmt_g((double)max_dist) + ", \"voxel\": " + fmt_g((double)opt.voxel) + ", \"rec\": " + json_cloud(rec) +
            ", \"gt\": " + json_cloud(gt) + ", \"accuracy\": " + json_direction(acc) + ", \"completeness\": " +
            json_direction(comp) + ", \"f1\": [" + join(f, fmt_g) + "]}";
    return 0;
}

// ---- depth mode ---------------------------------------------------------------------------------

struct DepthStats {
    int id = 0;
    std::string error;
    int64_t pixels = 0, valid_a = 0, valid_b = 0, valid_both = 0, mask_agree = 0, within_1e3 = 0, within_1e2 = 0;
    double median_rel = 0.0;  // lower median of |da - db| / db over the pixels valid in both
    std::vector<double> rel;
};

double lower_median(std::vector<double> &v) {
    if (v.empty()) return 0.0;
    const size_t k = (v.size() - 1) / 2;
    std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)k, v.end());
    return v[k];
}

// the reference ids of pair.txt (main.cpp:44-102 reads the same lines; the images are not needed here)
bool read_pair_ids(const std::string &dense, std::vector<int> &ids, std::string &err) {
    std::ifstream file(dense + "/pair.txt");
    if (!file) { err = "cannot open " + dense + "/pair.txt"; return false; }
    std::string line;
    std::getline(file, line);
    long n = 0;
    std::istringstream(line) >> n;
    for (long i = 0; i < n; ++i) {
        int id = -1;
        if (!std::getline(file, line) || !(std::istringstream(line) >> id) || id < 0) {
            err = dense + "/pair.txt: truncated or malformed";
            return false;
        }
        ids.push_back(id);
        std::getline(file, line);
    }
    return true;
}

void depth_view(const Options &opt, DepthStats &s) {
    const std::string name = format_index(s.id);
    Mat da, wa, db, wb;
    const std::string fa = opt.dense + "/APD/" + name;
    if (!read_binmat_file(fa + "/depths.bin", da) || !read_binmat_file(fa + "/weak.bin", wa)) {
        s.error = "cannot read " + fa + "/depths.bin or weak.bin";
        return;
    }
    const bool has_wb = opt.gt_depth.empty();
    if (has_wb) {
        const std::string fb = opt.against + "/APD/" + name;
        if (!read_binmat_file(fb + "/depths.bin", db) || !read_binmat_file(fb + "/weak.bin", wb)) {
            s.error = "cannot read " + fb + "/depths.bin or weak.bin";
            return;
        }
    } else if (!read_binmat_file(opt.gt_depth + "/" + name + ".bin", db)) {
        s.error = "cannot read " + opt.gt_depth + "/" + name + ".bin";
        return;
    }
    if (da.type != CV_32FC1 || db.type != CV_32FC1 || wa.type != CV_8UC1 || (has_wb && wb.type != CV_8UC1)) {
        s.error = "unexpected matrix type";
        return;
    }
    if (da.rows != db.rows || da.cols != db.cols || wa.rows != da.rows || wa.cols != da.cols ||
        (has_wb && (wb.rows != db.rows || wb.cols != db.cols))) {
        s.error = "size mismatch: " + std::to_string(da.cols) + "x" + std::to_string(da.rows) + " vs " +
                  std::to_string(db.cols) + "x" + std::to_string(db.rows);
        return;
    }
    const size_t n = (size_t)da.rows * da.cols;
    s.pixels = (int64_t)n;
    const float *pa = da.ptr<float>(), *pb = db.ptr<float>();
    const uint8_t *qa = wa.ptr<uint8_t>(), *qb = has_wb ? wb.ptr<uint8_t>() : nullptr;
    for (size_t i = 0; i < n; ++i) {
        const bool va = pa[i] > 0.0f && qa[i] != APD_UNKNOWN;
        const bool vb = pb[i] > 0.0f && (!qb || qb[i] != APD_UNKNOWN);
        s.valid_a += va;
        s.valid_b += vb;
        s.mask_agree += va == vb;
        if (va && vb) {
            ++s.valid_both;
            const double a = (double)pa[i], b = (double)pb[i], diff = std::fabs(a - b);
            s.within_1e3 += diff <= 1e-3 * b;
            s.within_1e2 += diff <= 1e-2 * b;
            s.rel.push_back(diff / b);
        }
    }
    std::vector<double> tmp = s.rel;
    s.median_rel = lower_median(tmp);
}

std::string json_depth(const DepthStats &s, bool with_id) {
    std::string o = "{";
    if (with_id) o += "\"id\": " + std::to_string(s.id) + ", ";
    if (!s.error.empty()) {
        std::string e = s.error;
        for (char &ch : e)
            if (ch == '"' || ch == '\\' || (unsigned char)ch < 32) ch = '\'';
        return o + "\"error\": \"" + e + "\"}";
    }
    return o + "\"pixels\": " + std::to_string(s.pixels) + ", \"valid_a\": " + std::to_string(s.valid_a) +
           ", \"valid_b\": " + std::to_string(s.valid_b) + ", \"valid_both\": " + std::to_string(s.valid_both) +
           ", \"mask_agree\": " + std::to_string(s.mask_agree) + ", \"within_1e-3\": " + std::to_string(s.within_1e3) +
           ", \"within_1e-2\": " + std::to_string(s.within_1e2) + ", \"median_rel\": " + fmt_g(s.median_rel) + "}";
}

int run_depth(const Options &opt, std::string &json) {
    std::vector<int> ids;
    std::string err;
    if (!read_pair_ids(opt.dense, ids, err)) {
        std::fprintf(stderr, "apd_eval: %s\n", err.c_str());
        return 2;
    }
    std::vector<DepthStats> views(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) views[i].id = ids[i];
    std::atomic<size_t> next{0};
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t workers = std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)(hw ? hw : 1), ids.size()}));
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([&] {
            for (size_t i; (i = next.fetch_add(1)) < views.size();) depth_view(opt, views[i]);
        });
    for (auto &t : pool) t.join();

    DepthStats total;
    int failed = 0;
    for (DepthStats &v : views) {
        if (!v.error.empty()) {
            ++failed;
            std::printf("view %d: error: %s\n", v.id, v.error.c_str());
            continue;
        }
        total.pixels += v.pixels;
        total.valid_a += v.valid_a;
        total.valid_b += v.valid_b;
        total.valid_both += v.valid_both;
        total.mask_agree += v.mask_agree;
        total.within_1e3 += v.within_1e3;
        total.within_1e2 += v.within_1e2;
        total.rel.insert(total.rel.end(), v.rel.begin(), v.rel.end());
        std::vector<double>().swap(v.rel);
        std::printf("view %d: pixels %lld valid_a %lld valid_b %lld both %lld mask_agree %lld within_1e-3 %lld "
                    "within_1e-2 %lld median_rel %.9g\n",
                    v.id, (long long)v.pixels, (long long)v.valid_a, (long long)v.valid_b, (long long)v.valid_both,
                    (long long)v.mask_agree, (long long)v.within_1e3, (long long)v.within_1e2, v.median_rel);
    }
    total.median_rel = lower_median(total.rel);
    std::printf("total: pixels %lld valid_a %lld valid_b %lld both %lld mask_agree %lld within_1e-3 %lld "
                "within_1e-2 %lld median_rel %.9g (%d views failed)\n",
                (long long)total.pixels, (long long)total.valid_a, (long long)total.valid_b, (long long)total.valid_both,
                (long long)total.mask_agree, (long long)total.within_1e3, (long long)total.within_1e2, total.median_rel,
                failed);
    auto esc = [](std::string s) {
        for (char &ch : s)
            if (ch == '"' || ch == '\\' || (unsigned char)ch < 32) ch = '\'';
        return s;
    };
    json += "\"depth\": {\"a\": \"" + esc(opt.dense) + "\", \"b\": \"" +
            esc(opt.gt_depth.empty() ? opt.against : opt.gt_depth) + "\", \"b_is_gt_depth\": " +
            (opt.gt_depth.empty() ? "false" : "true") + ", \"views\": [" +
            join(views, [](const DepthStats &s) { return json_depth(s, true); }) + "], \"failed_views\": " +
            std::to_string(failed) + ", \"total\": " + json_depth(total, false) + "}";
    return failed ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
    Options opt;
    auto bad = [](const std::string &m) {
        std::fprintf(stderr, "apd_eval: %s (see --help)\n", m.c_str());
        return 2;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--help" || a == "-h") {
            std::fputs(kHelp, stdout);
            return 0;
        }
        if (i + 1 >= argc) return bad("missing value for " + a);
        const std::string v = argv[++i];
        if (a == "--cloud") opt.cloud = v;
        else if (a == "--gt") opt.gt = v;
        else if (a == "--json") opt.json = v;
        else if (a == "--dense_folder") opt.dense = v;
        else if (a == "--against") opt.against = v;
        else if (a == "--gt_depth") opt.gt_depth = v;
        else if (a == "--gpu_index") opt.gpu = std::atoi(v.c_str());
        else if (a == "--max_dist") {
            if (!parse_float(v, opt.max_dist) || !(opt.max_dist >= 0.0f)) return bad("bad --max_dist " + v);
        } else if (a == "--voxel") {
            if (!parse_float(v, opt.voxel) || !(opt.voxel >= 0.0f) || !std::isfinite(opt.voxel))
                return bad("bad --voxel " + v);
        } else if (a == "--tolerances") {
            opt.tol.clear();
            std::istringstream ss(v);
            std::string tok;
            while (std::getline(ss, tok, ',')) {
                float t;
                if (!parse_float(tok, t) || !(t >= 0.0f)) return bad("bad tolerance '" + tok + "'");
                opt.tol.push_back(t);
            }
            if (opt.tol.empty()) return bad("empty --tolerances");
        } else {
            return bad("unknown option " + a);
        }
    }
    const bool cloud_mode = !opt.cloud.empty() || !opt.gt.empty();
    const bool depth_mode = !opt.dense.empty() || !opt.against.empty() || !opt.gt_depth.empty();
    if (!cloud_mode && !depth_mode) return bad("nothing to do");
    if (cloud_mode && (opt.cloud.empty() || opt.gt.empty())) return bad("cloud mode needs --cloud and --gt");
    if (depth_mode && (opt.dense.empty() || opt.against.empty() == opt.gt_depth.empty()))
        return bad("depth mode needs --dense_folder and exactly one of --against / --gt_depth");
    if (cloud_mode && opt.max_dist >= 0.0f)
        for (float t : opt.tol)
            if (t > opt.max_dist) return bad("a tolerance exceeds --max_dist");

    std::string json = "{";
    int status = 0;
    if (depth_mode) {
        status = run_depth(opt, json);
        if (status == 2) return 2;
    }
    if (cloud_mode) {
        if (depth_mode) json += ", ";
        const int st = run_cloud(opt, json);
        if (st == 2) return 2;
        status = std::max(status, st);
        if (st != 0) json += "\"cloud\": null";
    }
    json += "}\n";
    if (!opt.json.empty()) {
        std::ofstream out(opt.json);
        out << json;
        if (!out) {
            std::fprintf(stderr, "apd_eval: cannot write %s\n", opt.json.c_str());
            return 1;
        }
    }
    return status;
}
