// eval_main.cpp — `apd_eval`: accuracy / completeness / F1 of a fused cloud against a ground-truth
// cloud (cloud mode, on the GPU through include/apd_eval.h) and agreement of two sets of depth maps
// (depth mode, host only). It stands where the reference calls an external evaluator
// (tools/eval_eth_train.py), with the plain nearest-neighbour definition: the ETH3D tool's
// free-space and visibility handling is not modelled. A ground-truth cloud can be rendered into the
// scan's cameras with a z-buffer (render mode, and --gt_cloud in depth mode), and cloud mode can
// restrict completeness to the ground-truth points such a z-buffer test sees (--visible_views).
// Scanner mode (--gt_mlp) reads the MeshLab project of the laser scans and scores with a scanner
// free-space test and voxel averages, modelled on the ETH3D protocol (not the ETH3D tool itself).
// Tanks and Temples mode (--tat_gt) moves the reconstruction into the scan's frame, refines that by ICP
// on the GPU, cuts both clouds to the scene's crop volume, thins both by voxel and reports precision,
// recall and F-score at tau (modelled on the Tanks and Temples toolbox, not that toolbox).
// DTU mode (--dtu_gt) thins the reconstruction to a minimum point spacing on the GPU, restricts accuracy
// to the scan's observability mask and completeness to the points above the table plane, and reports
// the mean and median distances (modelled on the DTU MATLAB evaluation, not that code).
#include <algorithm>
#include <atomic>
#include <cerrno>
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
#include "image.h"
#include "io.h"

using namespace apdhost;

namespace {

const char *kHelp =
    "apd_eval - evaluate apd's results\n"
    "\n"
    "cloud mode (uses the GPU):\n"
    "  apd_eval --cloud REC.ply --gt GT.ply [--tolerances 0.01,0.02,0.05,0.1,0.2,0.5] [--max_dist D]\n"
    "           [--voxel V] [--gpu_index G] [--json OUT.json]\n"
    "           [--scan S --visible_views K [--splat s] [--occlusion_tol r]]\n"
    "  R and G are the two clouds after dropping non-finite points and, for V > 0, keeping the\n"
    "  lowest-index point of every V-sized voxel of each cloud. Per tolerance t:\n"
    "    accuracy = #{dist(R_i, G) <= t} / |R|, completeness = #{dist(G_j, R) <= t} / |G|,\n"
    "    F1 = 2ac / (a + c); each ratio is 0 when its denominator is 0.\n"
    "  Distances are plain nearest-neighbour distances truncated at D (default: the largest\n"
    "  tolerance). This is the DTU-style definition: the ETH3D evaluation's free-space and\n"
    "  visibility handling is NOT modelled, so the numbers compare runs of this project with each\n"
    "  other, not with published ETH3D tables.\n"
    "  With --scan S --visible_views K (K >= 1) completeness is taken over G', the points of G seen\n"
    "  in at least K of the reference views of S/pair.txt: G is rendered into every view with a\n"
    "  z-buffer (footprint 2s+1 pixels, --splat s, default 0) and a point is seen in a view when it\n"
    "  projects into the image no deeper than (1 + r) times the rendered depth at that pixel\n"
    "  (--occlusion_tol r, default 0.01). Accuracy is still taken against all of G. This visibility\n"
    "  filter is a z-buffer test, NOT ETH3D's free-space model.\n"
    "\n"
    "depth mode (host only, except --gt_cloud, which renders on the GPU):\n"
    "  apd_eval --dense_folder A (--against B | --gt_depth DIR | --gt_cloud GT.ply [--splat s])\n"
    "           [--json OUT.json]\n"
    "  For every reference view of A/pair.txt compares A/APD/<id>/depths.bin + weak.bin with\n"
    "  B/APD/<id>/depths.bin + weak.bin, or with DIR/<id>.bin (CV_32FC1, valid where depth > 0), or\n"
    "  with GT.ply rendered into A's views in memory (the maps --render_gt would write).\n"
    "  valid = depth > 0 and weak != UNKNOWN. Reports valid pixels per side and in both, pixels\n"
    "  whose validity agrees, and among pixels valid in both the counts with |da - db| <= 1e-3 db\n"
    "  and <= 1e-2 db and the lower median of |da - db| / db.\n"
    "\n"
    "render mode (uses the GPU):\n"
    "  apd_eval --render_gt GT.ply --scan S --out DIR [--splat s] [--gpu_index G] [--json OUT.json]\n"
    "  For every reference view of S/pair.txt writes DIR/<id>.bin (CV_32FC1, 0 = no surface, the\n"
    "  layout --gt_depth reads): the z-buffer of GT.ply in the camera S/cams/<id>_cam.txt, at the\n"
    "  size of S/APD/<id>/depths.bin when that exists, else of the image, the intrinsics rescaled\n"
    "  from the image's size as fusion does. Nearest point per pixel, ties to the lowest index.\n"
    "\n"
    "scanner mode (uses the GPU):\n"
    "  apd_eval --cloud REC.ply --gt_mlp SCAN.mlp [--tolerances ...] [--voxel V] [--cube_size N] [--splat s]\n"
    "           [--max_dist D] [--accuracy_cloud_out DIR] [--completeness_cloud_out DIR] [--gpu_index G]\n"
    "           [--json OUT.json]\n"
    "  SCAN.mlp is a MeshLab project: one PLY per laser-scanner position with its pose (<MLMesh\n"
    "  filename> + <MLMatrix44>), the ground-truth layout of ETH3D. G is the union of the scans in\n"
    "  world coordinates, R the reconstruction; no cloud is down-sampled. Per tolerance t a point of\n"
    "  R is good when dist(R_i, G) <= t, bad when it is not good and lies more than t in front of\n"
    "  the surface a scanner saw along its ray, and unobserved otherwise (behind the scanned\n"
    "  surface or where no beam went): unobserved points do not count. A scanner sees through the\n"
    "  six faces of a cube map of N^2 pixels (--cube_size, default 2048), the z-buffer of ITS OWN\n"
    "  points with footprint 2s+1 (--splat s, default 1). A point of G is good when dist(G_j, R) <= t,\n"
    "  else bad. Accuracy and completeness are the means over the V-sized voxels (--voxel, default\n"
    "  0.01: a scoring voxel) of good / (good + bad), as integers (good << 32) / (good + bad).\n"
    "  Prints the lines Tolerances: / Completenesses: / Accuracies: / F1-scores: that\n"
    "  tools/eval_eth_train.py parses. --accuracy_cloud_out / --completeness_cloud_out DIR write\n"
    "  DIR/tolerance_<t>.ply, the points of R / G coloured green (good), red (bad), blue (unobserved).\n"
    "  Modelled on the ETH3D protocol, NOT the ETH3D tool: a z-buffer per cube-map pixel instead of\n"
    "  per-beam cones, a free-space margin equal to the tolerance, integer-rounded voxel ratios.\n"
    "  Parity with that tool is unpinned; the numbers are not for published tables.\n"
    "  --gt_mlp excludes --gt, --dense_folder, --render_gt, --visible_views and --scan.\n"
    "\n"
    "Tanks and Temples mode (uses the GPU):\n"
    "  apd_eval --cloud REC.ply --tat_gt SCENE.ply --tat_crop SCENE.json --tau T [--tat_trans SCENE_trans.txt]\n"
    "           [--init_trans FILE] [--no_refine] [--refine_stages v:c,v:c,...] [--no_scale]\n"
    "           [--aligned_cloud_out OUT.ply] [--gpu_index G] [--json OUT.json]\n"
    "  SCENE.ply is the laser scan, SCENE.json its crop volume (Open3D SelectionPolygonVolume: axis_min,\n"
    "  axis_max, orthogonal_axis, bounding_polygon), the matrices are 4x4 text files mapping the\n"
    "  reconstruction's frame to the scan's (default identity; --init_trans is applied after --tat_trans).\n"
    "  1. T = init * trans. 2. Unless --no_refine, T is refined by point-to-point ICP with scaling\n"
    "  (--no_scale: rigid) in stages (voxel:max_corr, default T:80T, T/2:20T, T/2:2T): per stage both\n"
    "  clouds are cut to the crop volume (the reconstruction under T) and voxel-downsampled (the\n"
    "  reconstruction in the scan's frame; the lowest-index point of a voxel represents it), then 20\n"
    "  iterations at the most. 3. Both clouds are cropped with the final T and downsampled at T/2.\n"
    "  4. precision = share of reconstruction points closer than T to the scan, recall the same share the\n"
    "  other way, fscore = 2PR / (P + R). --aligned_cloud_out writes all of REC.ply under the final T.\n"
    "  Modelled on the Tanks and Temples toolbox, NOT that toolbox: a voxel is represented by its\n"
    "  lowest-index point, not its mean; the third stage downsamples by voxel, not uniformly; there is no\n"
    "  alignment from camera trajectories (.log). Parity is unpinned. --tat_dump prints what the readers\n"
    "  understood of --tat_crop / --tat_trans / --init_trans and exits.\n"
    "  --tat_gt excludes every other mode.\n"
    "\n"
    "DTU mode (uses the GPU):\n"
    "  apd_eval --cloud REC.ply --dtu_gt stlNNN_total.ply --dtu_mask ObsMaskN_10.mat --dtu_plane PlaneN.mat\n"
    "           [--dtu_density 0.2] [--dtu_max_dist 20] [--dtu_seed 0] [--dtu_no_thin]\n"
    "           [--thinned_cloud_out FILE.ply] [--gpu_index G] [--json OUT.json]\n"
    "  The mask file (Level-5 MAT, not -v7.3) supplies ObsMask, BB (2x3: min row, max row) and Res, the\n"
    "  plane file P (4 values). 1. Unless --dtu_no_thin, REC is thinned to a minimum point spacing of the\n"
    "  density: the points are visited in the order of a Philox rank drawn from --dtu_seed (ties by index)\n"
    "  and a point is kept iff no point kept before it lies within the density (exact, on the GPU).\n"
    "  2. Distances thinned REC -> GT and GT -> thinned REC, truncated at max_dist. 3. Accuracy takes the\n"
    "  points of REC whose cell round((p - BB(1,:)) / Res + 1) lies inside ObsMask and is set, completeness\n"
    "  the points of GT with [p 1] * P > 0; both take the distances < max_dist and report their mean and\n"
    "  median; overall = (accuracy mean + completeness mean) / 2. --thinned_cloud_out writes the thinned REC.\n"
    "  Modelled on the DTU MATLAB evaluation, NOT that code: a seeded order instead of randperm (the\n"
    "  numbers are reproducible, but not MATLAB's for any seed), doubles for the mask index, no chunks.\n"
    "  Parity is unpinned. --dtu_gt excludes every other mode.\n"
    "\n"
    "The modes may be combined in one invocation; --json then holds all of them.\n"
    "Exit status: 0 ok, 1 run-time failure, 2 bad arguments or unreadable input.\n";

struct Options {
    std::string cloud, gt, json, dense, against, gt_depth, gt_cloud, render_gt, scan, out;
    std::string gt_mlp, accuracy_out, completeness_out;  // scanner mode
    int cube_size = 2048;
    int splat = 0;
    bool splat_given = false, occlusion_given = false, voxel_given = false, cube_given = false;
    int visible_views = 0;  // 0: no visibility filter
    float occlusion_tol = 0.01f;
    std::vector<float> tol = {0.01f, 0.02f, 0.05f, 0.1f, 0.2f, 0.5f};
    float max_dist = -1.0f;  // < 0: the largest tolerance
    float voxel = 0.0f;
    int gpu = 0;
    // Tanks and Temples mode
    std::string tat_gt, tat_crop, tat_trans, init_trans, aligned_out;
    float tau = 0.0f;
    bool tau_given = false, no_refine = false, no_scale = false, tat_dump = false, stages_given = false;
    std::vector<std::pair<float, float>> stages;  // (voxel, max_corr)
    // DTU mode
    std::string dtu_gt, dtu_mask, dtu_plane, thinned_out;
    float dtu_density = 0.2f, dtu_max_dist = 20.0f;
    uint32_t dtu_seed = 0;
    bool dtu_no_thin = false, dtu_option_given = false;
};

bool parse_float(const std::string &s, float &v) {
    char *end = nullptr;
    v = std::strtof(s.c_str(), &end);
    return !s.empty() && end && *end == '\0';
}

bool parse_int(const std::string &s, int &v) {
    char *end = nullptr;
    const long l = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || !end || *end != '\0' || l < -1000000 || l > 1000000) return false;
    v = (int)l;
    return true;
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

// ---- scan views and rendering --------------------------------------------------------------------

bool read_pair_ids(const std::string &dense, std::vector<int> &ids, std::string &err);

struct ScanView {
    int id = 0;
    apd_camera cam{};  // width / height: the view's size; K rescaled to it
};

// rows and cols of a bin-mat file from its 16-byte header
bool probe_binmat_size(const std::string &path, int &rows, int &cols) {
    std::ifstream in(path, std::ios::binary);
    int32_t h[4];
    if (!in || !in.read(reinterpret_cast<char *>(h), sizeof h) || h[0] != 1) return false;
    rows = h[1];
    cols = h[2];
    return true;
}

// The reference views of scan/pair.txt with their cameras. The view size is that of
// scan/APD/<id>/depths.bin when it exists, else the image's; the intrinsics are rescaled from the
// image's size as fusion.cpp::load_view does (RescaleImageAndCamera).
bool load_scan_views(const std::string &scan, std::vector<ScanView> &views, std::string &err) {
    std::vector<int> ids;
    if (!read_pair_ids(scan, ids, err)) return false;
    static const char *exts[] = {".jpg", ".png", ".jpeg", ".JPG", ".PNG", ".JPEG"};  // as read_pair_file
    for (int id : ids) {
        ScanView v;
        v.id = id;
        const std::string name = format_index(id), cam = scan + "/cams/" + name + "_cam.txt";
        if (!read_camera(cam, v.cam)) { err = "cannot read " + cam; return false; }
        std::string img;
        for (const char *e : exts)
            if (file_exists(scan + "/images/" + name + e)) { img = scan + "/images/" + name + e; break; }
        Gray8 src;
        if (img.empty()) { err = "can not find image: " + scan + "/images/" + name; return false; }
        if (!read_gray8(img, src, err)) { err = img + ": " + err; return false; }
        int W = src.width, H = src.height;
        const std::string dep = scan + "/APD/" + name + "/depths.bin";
        if (file_exists(dep) && !probe_binmat_size(dep, H, W)) { err = "cannot read " + dep; return false; }
        if (W < 1 || H < 1 || src.width < 1 || src.height < 1 || (int64_t)W * H > ((int64_t)1 << 28)) {
            err = "view " + name + ": unusable size " + std::to_string(W) + "x" + std::to_string(H);
            return false;
        }
        if (src.width != W || src.height != H) {
            const float scale_x = W / static_cast<float>(src.width);
            const float scale_y = H / static_cast<float>(src.height);
            v.cam.K[0] *= scale_x;
            v.cam.K[2] *= scale_x;
            v.cam.K[4] *= scale_y;
            v.cam.K[5] *= scale_y;
        }
        v.cam.width = W;
        v.cam.height = H;
        views.push_back(v);
    }
    return true;
}

constexpr size_t kViewBatch = 8;  // views rendered per library call (the cloud is uploaded once per call)

// z-buffers of views [lo, hi) as CV_32FC1 Mats
bool render_batch(apd_eval_ctx *ctx, const std::vector<float> &xyz, const std::vector<ScanView> &views, size_t lo,
                  size_t hi, int splat, std::vector<Mat> &maps, double &render_ms) {
    std::vector<apd_camera> cams;
    std::vector<float *> ptrs;
    maps.clear();
    for (size_t i = lo; i < hi; ++i) {
        cams.push_back(views[i].cam);
        maps.emplace_back(views[i].cam.height, views[i].cam.width, (int)CV_32FC1);
        ptrs.push_back(maps.back().ptr<float>());
    }
    const int st = apd_eval_render_depth(ctx, (int64_t)(xyz.size() / 3), xyz.data(), (int32_t)cams.size(), cams.data(),
                                         splat, ptrs.data(), nullptr);
    if (st != APD_OK) {
        std::fprintf(stderr, "apd_eval: apd_eval_render_depth failed (%d): %s\n", st, apd_eval_last_error(ctx));
        return false;
    }
    double ms = 0.0;
    apd_eval_get_render_timing(ctx, &ms, nullptr);
    render_ms += ms;
    return true;
}

std::string esc(std::string s) {
    for (char &ch : s)
        if (ch == '"' || ch == '\\' || (unsigned char)ch < 32) ch = '\'';
    return s;
}

struct RenderInputs {
    std::vector<float> xyz;
    std::vector<ScanView> views;
};

// returns the exit status; appends "render": {...} to json
int run_render(const Options &opt, const RenderInputs &in, std::string &json) {
    if (!make_dir(opt.out)) {
        std::fprintf(stderr, "apd_eval: cannot create %s\n", opt.out.c_str());
        return 1;
    }
    apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
    if (!ctx) {
        std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
        return 1;
    }
    double render_ms = 0.0;
    std::vector<std::string> rows;
    bool ok = true;
    for (size_t lo = 0; ok && lo < in.views.size(); lo += kViewBatch) {
        const size_t hi = std::min(in.views.size(), lo + kViewBatch);
        std::vector<Mat> maps;
        ok = render_batch(ctx, in.xyz, in.views, lo, hi, opt.splat, maps, render_ms);
        for (size_t i = lo; ok && i < hi; ++i) {
            const Mat &m = maps[i - lo];
            const std::string path = opt.out + "/" + format_index(in.views[i].id) + ".bin";
            if (!write_binmat_file(path, m)) {
                std::fprintf(stderr, "apd_eval: cannot write %s\n", path.c_str());
                ok = false;
                break;
            }
            int64_t covered = 0;
            const float *p = m.ptr<float>();
            for (size_t k = 0, n = (size_t)m.rows * m.cols; k < n; ++k) covered += p[k] > 0.0f;
            std::printf("rendered view %d: %dx%d covered %lld\n", in.views[i].id, m.cols, m.rows, (long long)covered);
            rows.push_back("{\"id\": " + std::to_string(in.views[i].id) + ", \"width\": " + std::to_string(m.cols) +
                           ", \"height\": " + std::to_string(m.rows) + ", \"covered\": " + std::to_string(covered) + "}");
        }
    }
    apd_eval_destroy(ctx);
    if (!ok) return 1;
    json += "\"render\": {\"gt\": \"" + esc(opt.render_gt) + "\", \"scan\": \"" + esc(opt.scan) + "\", \"out\": \"" +
            esc(opt.out) + "\", \"splat\": " + std::to_string(opt.splat) + ", \"points\": " +
            std::to_string(in.xyz.size() / 3) + ", \"views\": [" +
            join(rows, [](const std::string &r) { return r; }) + "], \"render_ms\": " + fmt_g(render_ms) + "}";
    return 0;
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
    int64_t points_visible = -1;  // |G'| with --visible_views, else unused
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
           ", \"points\": " + std::to_string(c.points) +
           (c.points_visible >= 0 ? ", \"points_visible\": " + std::to_string(c.points_visible) : std::string()) + "}";
}

// G' = the points of g seen in at least opt.visible_views of the views: g is rendered into every
// view and tested against its own z-buffers (a z-buffer test, not a free-space model)
bool visible_subset(apd_eval_ctx *ctx, const CloudInfo &g, const std::vector<ScanView> &views, const Options &opt,
                    CloudInfo &vis, double &render_ms, double &visibility_ms) {
    std::vector<int32_t> seen((size_t)g.points, 0), part((size_t)g.points);
    for (size_t lo = 0; lo < views.size(); lo += kViewBatch) {
        const size_t hi = std::min(views.size(), lo + kViewBatch);
        std::vector<Mat> maps;
        if (!render_batch(ctx, g.xyz, views, lo, hi, opt.splat, maps, render_ms)) return false;
        std::vector<apd_camera> cams;
        std::vector<const float *> ptrs;
        for (size_t i = lo; i < hi; ++i) {
            cams.push_back(views[i].cam);
            ptrs.push_back(maps[i - lo].ptr<float>());
        }
        const int st = apd_eval_visibility(ctx, g.points, g.xyz.data(), (int32_t)cams.size(), cams.data(), ptrs.data(),
                                           opt.occlusion_tol, part.data(), nullptr);
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_visibility", st);
        double ms = 0.0;
        apd_eval_get_render_timing(ctx, nullptr, &ms);
        visibility_ms += ms;
        for (size_t i = 0; i < seen.size(); ++i) seen[i] += part[i];
    }
    vis = CloudInfo{};
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] >= opt.visible_views)
            for (int a = 0; a < 3; ++a) vis.xyz.push_back(g.xyz[3 * i + a]);
    vis.points = (int64_t)(vis.xyz.size() / 3);
    return true;
}

std::string json_direction(const Direction &d) {
    auto ratio = [&](int64_t w) { return fmt_g(d.n ? (double)w / (double)d.n : 0.0); };
    return "{\"points\": " + std::to_string(d.n) + ", \"within\": [" +
           join(d.within, [](int64_t w) { return std::to_string(w); }) + "], \"ratio\": [" + join(d.within, ratio) +
           "], \"inf\": " + std::to_string(d.inf) + ", \"mean\": " + fmt_g(d.mean) + ", \"build_ms\": " +
           fmt_g(d.build_ms) + ", \"query_ms\": " + fmt_g(d.query_ms) + "}";
}

struct CloudInputs {
    CloudInfo rec, gt;
    std::vector<ScanView> views;  // with --visible_views
};

// returns the exit status; appends "cloud": {...} to json. The files were parsed by main() before
// any device context existed: a malformed file fails without a GPU
int run_cloud(const Options &opt, CloudInputs &in, std::string &json) {
    CloudInfo &rec = in.rec, &gt = in.gt;
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
    const bool filter = opt.visible_views > 0;
    CloudInfo gt_vis;
    double render_ms = 0.0, visibility_ms = 0.0;
    if (ok && filter) {
        ok = visible_subset(ctx, gt, in.views, opt, gt_vis, render_ms, visibility_ms);
        gt.points_visible = gt_vis.points;
    }
    ok = ok && direction(ctx, rec, gt, opt, max_dist, acc) &&
         direction(ctx, filter ? gt_vis : gt, rec, opt, max_dist, comp);
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
    if (filter)
        std::printf("Visible ground truth: %lld of %lld points (seen in >= %d of %zu views)\n",
                    (long long)gt.points_visible, (long long)gt.points, opt.visible_views, in.views.size());
    std::printf("Tolerances: %s\n", join(opt.tol, fmt_f32, " ").c_str());
    std::printf("Completenesses: %s\n", join(c, six, " ").c_str());
    std::printf("Accuracies: %s\n", join(a, six, " ").c_str());
    std::printf("F1-scores: %s\n", join(f, six, " ").c_str());
    json += std::string("\"cloud\": {\"definition\": \"") +
            (filter ? "plain nearest neighbour; completeness over the ground-truth points that pass a z-buffer "
                      "visibility test (not the ETH3D free-space model)"
                    : "plain nearest neighbour (no free-space / visibility model)") +
            "\", " +
            (filter ? "\"visibility\": {\"scan\": \"" + esc(opt.scan) + "\", \"views\": " + std::to_string(in.views.size()) +
                          ", \"min_views\": " + std::to_string(opt.visible_views) + ", \"splat\": " +
                          std::to_string(opt.splat) + ", \"occlusion_tol\": " + fmt_f32(opt.occlusion_tol) +
                          ", \"render_ms\": " + fmt_g(render_ms) + ", \"visibility_ms\": " + fmt_g(visibility_ms) + "}, "
                    : std::string()) +
            "\"tolerances\": [" + join(opt.tol, fmt_f32) + "], \"max_dist\": " +
            fmt_g((double)max_dist) + ", \"voxel\": " + fmt_g((double)opt.voxel) + ", \"rec\": " + json_cloud(rec) +
            ", \"gt\": " + json_cloud(gt) + ", \"accuracy\": " + json_direction(acc) + ", \"completeness\": " +
            json_direction(comp) + ", \"f1\": [" + join(f, fmt_g) + "]}";
    return 0;
}

// ---- scanner mode -------------------------------------------------------------------------------

struct Scanner {
    std::string ply;
    std::vector<float> xyz;  // world coordinates, finite points only after run_scanners' first step
    float origin[3] = {0, 0, 0};
    int64_t points_in = 0;
};

struct ScannerInputs {
    CloudInfo rec;
    std::vector<Scanner> scanners;
};

struct SideScores {
    int64_t n = 0;
    std::vector<int64_t> good, bad, voxels;
    std::vector<uint64_t> ratio_sum;
    std::vector<double> score;
    std::vector<float> dist;
    double build_ms = 0.0, query_ms = 0.0, scores_ms = 0.0;
};

// set_target(t), distances(q), voxel_scores(q, dist, gap)
bool score_side(apd_eval_ctx *ctx, const std::vector<float> &q, const std::vector<float> &t, const float *gap,
                const Options &opt, float max_dist, SideScores &s) {
    s.n = (int64_t)(q.size() / 3);
    int st = apd_eval_set_target(ctx, (int64_t)(t.size() / 3), t.data());
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_set_target", st);
    s.dist.resize((size_t)s.n);
    st = apd_eval_distances(ctx, s.n, q.data(), max_dist, s.dist.data(), 0, nullptr, nullptr);
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_distances", st);
    apd_eval_get_timing(ctx, &s.build_ms, &s.query_ms, nullptr);
    const size_t k = opt.tol.size();
    s.good.assign(k, 0);
    s.bad.assign(k, 0);
    s.voxels.assign(k, 0);
    s.ratio_sum.assign(k, 0);
    st = apd_eval_voxel_scores(ctx, s.n, q.data(), opt.voxel, s.dist.data(), gap, (int32_t)k, opt.tol.data(),
                               s.good.data(), s.bad.data(), s.ratio_sum.data(), s.voxels.data());
    if (st != APD_OK) return fail_ctx(ctx, "apd_eval_voxel_scores", st);
    apd_eval_get_protocol_timing(ctx, nullptr, &s.scores_ms);
    s.score.assign(k, 0.0);
    for (size_t i = 0; i < k; ++i)
        if (s.voxels[i] > 0) s.score[i] = (double)s.ratio_sum[i] / ((double)s.voxels[i] * 4294967296.0);
    return true;
}

std::string json_side(const SideScores &s) {
    auto i64 = [](int64_t v) { return std::to_string(v); };
    std::vector<int64_t> unobs(s.good.size());
    std::vector<double> of_all(s.good.size()), plain(s.good.size());
    for (size_t i = 0; i < s.good.size(); ++i) {
        unobs[i] = s.n - s.good[i] - s.bad[i];
        of_all[i] = s.n ? (double)s.good[i] / (double)s.n : 0.0;
        plain[i] = s.good[i] + s.bad[i] ? (double)s.good[i] / (double)(s.good[i] + s.bad[i]) : 0.0;
    }
    return "{\"points\": " + std::to_string(s.n) + ", \"good\": [" + join(s.good, i64) + "], \"bad\": [" +
           join(s.bad, i64) + "], \"unobserved\": [" + join(unobs, i64) + "], \"ratio_sum\": [" +
           join(s.ratio_sum, [](uint64_t v) { return std::to_string(v); }) + "], \"voxels\": [" + join(s.voxels, i64) +
           "], \"score\": [" + join(s.score, fmt_g) + "], \"plain_of_all\": [" + join(of_all, fmt_g) +
           "], \"plain\": [" + join(plain, fmt_g) + "], \"build_ms\": " + fmt_g(s.build_ms) + ", \"query_ms\": " +
           fmt_g(s.query_ms) + ", \"scores_ms\": " + fmt_g(s.scores_ms) + "}";
}

// DIR/tolerance_<t>.ply per tolerance: green good, red bad, blue unobserved (gap == nullptr: none)
bool write_class_clouds(const std::string &dir, const std::vector<float> &xyz, const std::vector<float> &dist,
                        const float *gap, const std::vector<float> &tol) {
    if (!make_dir(dir)) {
        std::fprintf(stderr, "apd_eval: cannot create %s\n", dir.c_str());
        return false;
    }
    std::vector<uint8_t> rgb(xyz.size());
    for (float t : tol) {
        for (size_t i = 0; i < dist.size(); ++i) {
            const bool good = dist[i] <= t, bad = !good && (!gap || gap[i] > t);
            rgb[3 * i] = bad ? 255 : 0;
            rgb[3 * i + 1] = good ? 255 : 0;
            rgb[3 * i + 2] = !good && !bad ? 255 : 0;
        }
        const std::string path = dir + "/tolerance_" + fmt_f32(t) + ".ply";
        if (!write_ply_xyz_rgb(path, xyz, rgb)) {
            std::fprintf(stderr, "apd_eval: cannot write %s\n", path.c_str());
            return false;
        }
    }
    return true;
}

// returns the exit status; appends "scanners": {...} to json
int run_scanners(const Options &opt, ScannerInputs &in, std::string &json) {
    CloudInfo &rec = in.rec;
    drop_non_finite(rec);
    std::vector<float> G;
    for (Scanner &s : in.scanners) {
        CloudInfo c;
        c.xyz.swap(s.xyz);
        drop_non_finite(c);
        s.points_in = c.points_in;
        s.xyz.swap(c.xyz);
        G.insert(G.end(), s.xyz.begin(), s.xyz.end());
    }
    const float max_dist = opt.max_dist >= 0.0f ? opt.max_dist : *std::max_element(opt.tol.begin(), opt.tol.end());
    apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
    if (!ctx) {
        std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
        return 1;
    }
    // the free gap of R: one scanner's six cube faces at a time, rendered from that scanner's own
    // points, the maximum over the scanners taken here (a maximum has no order)
    const int64_t nr = rec.points;
    std::vector<float> gap((size_t)nr, -INFINITY), part((size_t)nr);
    double render_ms = 0.0, gap_ms = 0.0;
    bool ok = true;
    for (size_t si = 0; ok && si < in.scanners.size(); ++si) {
        const Scanner &s = in.scanners[si];
        std::vector<ScanView> faces(6);
        apd_camera cams[6];
        if (apd_eval_cube_cameras(s.origin, opt.cube_size, cams) != APD_OK) {
            std::fprintf(stderr, "apd_eval: scanner %zu has no usable origin\n", si);
            ok = false;
            break;
        }
        for (int f = 0; f < 6; ++f) faces[(size_t)f].cam = cams[f];
        std::vector<Mat> maps;
        if (!(ok = render_batch(ctx, s.xyz, faces, 0, 6, opt.splat, maps, render_ms))) break;
        const float *ptrs[6];
        for (int f = 0; f < 6; ++f) ptrs[f] = maps[(size_t)f].ptr<float>();
        const int st = apd_eval_free_gap(ctx, nr, rec.xyz.data(), 6, cams, ptrs, part.data());
        if (st != APD_OK) {
            ok = fail_ctx(ctx, "apd_eval_free_gap", st);
            break;
        }
        double ms = 0.0;
        apd_eval_get_protocol_timing(ctx, &ms, nullptr);
        gap_ms += ms;
        for (size_t i = 0; i < gap.size(); ++i) gap[i] = std::max(gap[i], part[i]);
    }
    SideScores acc, comp;
    ok = ok && score_side(ctx, rec.xyz, G, gap.data(), opt, max_dist, acc) &&
         score_side(ctx, G, rec.xyz, nullptr, opt, max_dist, comp);
    apd_eval_destroy(ctx);
    if (!ok) return 1;
    if (!opt.accuracy_out.empty() && !write_class_clouds(opt.accuracy_out, rec.xyz, acc.dist, gap.data(), opt.tol))
        return 1;
    if (!opt.completeness_out.empty() && !write_class_clouds(opt.completeness_out, G, comp.dist, nullptr, opt.tol))
        return 1;

    const size_t k = opt.tol.size();
    std::vector<double> f(k);
    for (size_t i = 0; i < k; ++i) {
        const double a = acc.score[i], c = comp.score[i];
        f[i] = a + c > 0.0 ? 2.0 * a * c / (a + c) : 0.0;
    }
    auto six = [](double v) {
        char b[64];
        std::snprintf(b, sizeof b, "%.6f", v);
        return std::string(b);
    };
    std::printf("Scanner free-space model: %zu scanner positions, cube maps of %d^2, voxel %s\n", in.scanners.size(),
                opt.cube_size, fmt_f32(opt.voxel).c_str());
    std::printf("%-10s %10s %10s %10s %9s   %10s %10s %9s\n", "tolerance", "acc good", "acc bad", "unobserved", "accuracy",
                "comp good", "comp bad", "complete");
    for (size_t i = 0; i < k; ++i)
        std::printf("%-10s %10lld %10lld %10lld %9.6f   %10lld %10lld %9.6f\n", fmt_f32(opt.tol[i]).c_str(),
                    (long long)acc.good[i], (long long)acc.bad[i], (long long)(acc.n - acc.good[i] - acc.bad[i]),
                    acc.score[i], (long long)comp.good[i], (long long)comp.bad[i], comp.score[i]);
    std::printf("Tolerances: %s\n", join(opt.tol, fmt_f32, " ").c_str());
    std::printf("Completenesses: %s\n", join(comp.score, six, " ").c_str());
    std::printf("Accuracies: %s\n", join(acc.score, six, " ").c_str());
    std::printf("F1-scores: %s\n", join(f, six, " ").c_str());
    json += "\"scanners\": {\"definition\": \"scanner free-space model and voxel-averaged scores, modelled on the ETH3D "
            "protocol (a z-buffer per cube-map pixel, a free-space margin equal to the tolerance, integer voxel "
            "ratios); parity with the ETH3D tool is not pinned\", \"tolerances\": [" +
            join(opt.tol, fmt_f32) + "], \"max_dist\": " + fmt_g((double)max_dist) + ", \"voxel\": " +
            fmt_g((double)opt.voxel) + ", \"cube_size\": " + std::to_string(opt.cube_size) + ", \"splat\": " +
            std::to_string(opt.splat) + ", \"rec\": " + json_cloud(rec) + ", \"gt\": {\"points\": " +
            std::to_string(G.size() / 3) + "}, \"positions\": [" +
            join(in.scanners,
                 [](const Scanner &s) {
                     return "{\"ply\": \"" + esc(s.ply) + "\", \"points_in\": " + std::to_string(s.points_in) +
                            ", \"points\": " + std::to_string(s.xyz.size() / 3) + ", \"origin\": [" +
                            fmt_g((double)s.origin[0]) + ", " + fmt_g((double)s.origin[1]) + ", " +
                            fmt_g((double)s.origin[2]) + "]}";
                 }) +
            "], \"accuracy\": " + json_side(acc) + ", \"completeness\": " + json_side(comp) + ", \"f1\": [" +
            join(f, fmt_g) + "], \"render_ms\": " + fmt_g(render_ms) + ", \"free_gap_ms\": " + fmt_g(gap_ms) + "}";
    return 0;
}

// ---- Tanks and Temples mode ------------------------------------------------------------------------

struct TatInputs {
    std::vector<float> rec, gt;
    TatCrop crop;
    double trans[16], init[16];
};

void identity16(double *M) {
    for (int i = 0; i < 16; ++i) M[i] = i % 5 == 0 ? 1.0 : 0.0;
}

void mul16(const double *A, const double *B, double *C) {
    double r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
            r[4 * i + j] = s;
        }
    std::copy(r, r + 16, C);
}

std::string json_mat(const double *M) {
    std::string s = "[";
    for (int i = 0; i < 16; ++i) s += (i ? ", " : "") + fmt_g(M[i]);
    return s + "]";
}

std::vector<float> gather(const std::vector<float> &xyz, const std::vector<int32_t> &keep, int64_t nk) {
    std::vector<float> out((size_t)nk * 3);
    for (int64_t i = 0; i < nk; ++i)
        for (int a = 0; a < 3; ++a) out[3 * (size_t)i + a] = xyz[3 * (size_t)keep[(size_t)i] + a];
    return out;
}

struct TatStage {
    float voxel = 0.0f, max_corr = 0.0f;
    int64_t source_points = 0, target_points = 0;
    apd_eval_reg_info info{};
    bool ok = false;
    double eval_ms = 0.0, fold_ms = 0.0, solve_ms = 0.0;
    int32_t evaluations = 0;
};

// returns the exit status; appends "tat": {...} to json
int run_tat(const Options &opt, const TatInputs &in, std::string &json) {
    apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
    if (!ctx) {
        std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
        return 1;
    }
    const std::vector<double> poly = in.crop.polygon();
    const int32_t m = (int32_t)(poly.size() / 2);
    double crop_ms = 0.0, voxel_ms = 0.0, transform_ms = 0.0;
    bool ok = true;
    auto crop = [&](const std::vector<float> &xyz, const double *T, std::vector<float> &out) {
        const int64_t n = (int64_t)(xyz.size() / 3);
        std::vector<int32_t> keep((size_t)std::max<int64_t>(n, 1));
        int64_t nk = 0;
        const int st = apd_eval_crop_volume(ctx, n, xyz.data(), T, in.crop.axis, in.crop.axis_min, in.crop.axis_max, m,
                                            poly.data(), keep.data(), &nk);
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_crop_volume", st);
        double ms = 0.0;
        apd_eval_get_register_timing(ctx, nullptr, nullptr, nullptr, nullptr, &ms, nullptr);
        crop_ms += ms;
        out = gather(xyz, keep, nk);
        return true;
    };
    auto transform = [&](const std::vector<float> &xyz, const double *T, std::vector<float> &out) {
        out.resize(xyz.size());
        const int st = apd_eval_transform(ctx, (int64_t)(xyz.size() / 3), xyz.data(), T, out.data());
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_transform", st);
        double ms = 0.0;
        apd_eval_get_register_timing(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, &ms);
        transform_ms += ms;
        return true;
    };
    // indices of the lowest-index point of every voxel of `at` (the cloud in the scan's frame)
    auto voxel_keep = [&](const std::vector<float> &at, float voxel, std::vector<int32_t> &keep, int64_t &nk) {
        const int64_t n = (int64_t)(at.size() / 3);
        keep.assign((size_t)std::max<int64_t>(n, 1), 0);
        const int st = apd_eval_voxel_downsample(ctx, n, at.data(), voxel, keep.data(), &nk);
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_voxel_downsample", st);
        double ms = 0.0;
        apd_eval_get_timing(ctx, nullptr, nullptr, &ms);
        voxel_ms += ms;
        return true;
    };
    // the reconstruction cut to the volume under T and thinned in the scan's frame: `orig` in its own
    // coordinates (what the registration takes), `moved` under T
    int64_t rec_cropped = 0;
    auto source = [&](const double *T, float voxel, std::vector<float> &orig, std::vector<float> &moved) {
        std::vector<float> cut, cut_moved;
        std::vector<int32_t> keep;
        int64_t nk = 0;
        if (!crop(in.rec, T, cut) || !transform(cut, T, cut_moved) || !voxel_keep(cut_moved, voxel, keep, nk))
            return false;
        rec_cropped = (int64_t)(cut.size() / 3);
        orig = gather(cut, keep, nk);
        moved = gather(cut_moved, keep, nk);
        return true;
    };
    std::vector<float> gt_cut;
    ok = crop(in.gt, nullptr, gt_cut);
    std::vector<std::pair<float, std::vector<float>>> targets;  // by voxel
    auto target = [&](float voxel) -> const std::vector<float> * {
        for (auto &t : targets)
            if (t.first == voxel) return &t.second;
        std::vector<int32_t> keep;
        int64_t nk = 0;
        if (!voxel_keep(gt_cut, voxel, keep, nk)) return nullptr;
        targets.emplace_back(voxel, gather(gt_cut, keep, nk));
        return &targets.back().second;
    };

    double T[16];
    mul16(in.init, in.trans, T);
    std::vector<TatStage> stages;
    if (!opt.no_refine)
        for (size_t k = 0; ok && k < opt.stages.size(); ++k) {
            TatStage s;
            s.voxel = opt.stages[k].first;
            s.max_corr = opt.stages[k].second;
            std::vector<float> src, moved;
            const std::vector<float> *tgt = nullptr;
            if (!(ok = source(T, s.voxel, src, moved) && (tgt = target(s.voxel)) != nullptr)) break;
            s.source_points = (int64_t)(src.size() / 3);
            s.target_points = (int64_t)(tgt->size() / 3);
            int st = apd_eval_set_target(ctx, s.target_points, tgt->data());
            if (st != APD_OK) { ok = fail_ctx(ctx, "apd_eval_set_target", st); break; }
            double Tn[16];
            st = apd_eval_register(ctx, s.source_points, src.data(), T, s.max_corr, opt.no_scale ? 0 : 1, 20, 1e-6, 1e-6,
                                   Tn, &s.info);
            if (st != APD_OK && st != APD_ESTATE) { ok = fail_ctx(ctx, "apd_eval_register", st); break; }
            s.ok = st == APD_OK;
            apd_eval_get_register_timing(ctx, &s.eval_ms, &s.fold_ms, &s.solve_ms, &s.evaluations, nullptr, nullptr);
            std::copy(Tn, Tn + 16, T);  // on APD_ESTATE: the last transform with 3 correspondences, T itself if none
            std::printf("stage %zu: voxel %s max_corr %s source %lld target %lld iterations %d n_corr %lld fitness %.6f "
                        "rmse %.6g%s\n",
                        k + 1, fmt_f32(s.voxel).c_str(), fmt_f32(s.max_corr).c_str(), (long long)s.source_points,
                        (long long)s.target_points, s.info.iterations, (long long)s.info.n_corr, s.info.fitness,
                        s.info.rmse, s.ok ? "" : " (too few correspondences: transform kept)");
            stages.push_back(s);
        }

    const float half = opt.tau / 2.0f, strict = std::nextafterf(opt.tau, 0.0f);
    std::vector<float> src, moved;
    const std::vector<float> *tgt = nullptr;
    int64_t within_p = 0, within_r = 0;
    double build_ms = 0.0, query_ms = 0.0;
    ok = ok && source(T, half, src, moved) && (tgt = target(half)) != nullptr;
    if (ok) {
        auto side = [&](const std::vector<float> &q, const std::vector<float> &t, int64_t &within) {
            int st = apd_eval_set_target(ctx, (int64_t)(t.size() / 3), t.data());
            if (st != APD_OK) return fail_ctx(ctx, "apd_eval_set_target", st);
            st = apd_eval_distances(ctx, (int64_t)(q.size() / 3), q.data(), opt.tau, nullptr, 1, &strict, &within);
            if (st != APD_OK) return fail_ctx(ctx, "apd_eval_distances", st);
            double b = 0.0, qm = 0.0;
            apd_eval_get_timing(ctx, &b, &qm, nullptr);
            build_ms += b;
            query_ms += qm;
            return true;
        };
        ok = side(moved, *tgt, within_p) && side(*tgt, moved, within_r);
    }
    if (ok && !opt.aligned_out.empty()) {
        std::vector<float> all;
        if ((ok = transform(in.rec, T, all))) {
            const std::vector<uint8_t> rgb(all.size(), 200);
            if (!write_ply_xyz_rgb(opt.aligned_out, all, rgb)) {
                std::fprintf(stderr, "apd_eval: cannot write %s\n", opt.aligned_out.c_str());
                ok = false;
            }
        }
    }
    apd_eval_destroy(ctx);
    if (!ok) return 1;

    const int64_t ns = (int64_t)(moved.size() / 3), ng = (int64_t)(tgt->size() / 3);
    const double P = ns ? (double)within_p / (double)ns : 0.0, R = ng ? (double)within_r / (double)ng : 0.0;
    const double F = P + R > 0.0 ? 2.0 * P * R / (P + R) : 0.0;
    std::printf("Tanks and Temples protocol: tau %s, %s, %zu refinement stages\n", fmt_f32(opt.tau).c_str(),
                opt.no_scale ? "rigid" : "with scale", stages.size());
    std::printf("source points: %zu in, %lld in the crop volume, %lld after downsampling\n", in.rec.size() / 3,
                (long long)rec_cropped, (long long)ns);
    std::printf("target points: %zu in, %zu in the crop volume, %lld after downsampling\n", in.gt.size() / 3,
                gt_cut.size() / 3, (long long)ng);
    std::printf("precision: %.6f\nrecall: %.6f\nf-score: %.6f\n", P, R, F);
    json += std::string("\"tat\": {\"definition\": \"modelled on the Tanks and Temples protocol (crop volume, ICP "
                        "refinement, voxel downsampling, precision / recall / F-score at tau) with this project's own "
                        "contract: lowest-index voxel representative, third stage by voxel, no trajectory alignment; "
                        "parity with the toolbox is not pinned\", \"tau\": ") +
            fmt_g((double)opt.tau) + ", \"with_scale\": " + (opt.no_scale ? "false" : "true") + ", \"refine\": " +
            (opt.no_refine ? "false" : "true") + ", \"stages\": [" +
            join(stages,
                 [](const TatStage &s) {
                     return "{\"voxel\": " + fmt_g((double)s.voxel) + ", \"max_corr\": " + fmt_g((double)s.max_corr) +
                            ", \"source_points\": " + std::to_string(s.source_points) + ", \"target_points\": " +
                            std::to_string(s.target_points) + ", \"ok\": " + (s.ok ? "true" : "false") +
                            ", \"iterations\": " + std::to_string(s.info.iterations) + ", \"n_corr\": " +
                            std::to_string(s.info.n_corr) + ", \"n_finite\": " + std::to_string(s.info.n_finite) +
                            ", \"fitness\": " + fmt_g(s.info.fitness) + ", \"rmse\": " + fmt_g(s.info.rmse) +
                            ", \"evaluations\": " + std::to_string(s.evaluations) + ", \"eval_ms\": " + fmt_g(s.eval_ms) +
                            ", \"fold_ms\": " + fmt_g(s.fold_ms) + ", \"solve_ms\": " + fmt_g(s.solve_ms) + "}";
                 }) +
            "], \"transform\": " + json_mat(T) + ", \"source\": {\"points_in\": " + std::to_string(in.rec.size() / 3) +
            ", \"points_cropped\": " + std::to_string(rec_cropped) + ", \"points\": " + std::to_string(ns) +
            "}, \"target\": {\"points_in\": " + std::to_string(in.gt.size() / 3) + ", \"points_cropped\": " +
            std::to_string(gt_cut.size() / 3) + ", \"points\": " + std::to_string(ng) + "}, \"within_precision\": " +
            std::to_string(within_p) + ", \"within_recall\": " + std::to_string(within_r) + ", \"precision\": " +
            fmt_g(P) + ", \"recall\": " + fmt_g(R) + ", \"fscore\": " + fmt_g(F) + ", \"crop_ms\": " + fmt_g(crop_ms) +
            ", \"voxel_ms\": " + fmt_g(voxel_ms) + ", \"transform_ms\": " + fmt_g(transform_ms) + ", \"build_ms\": " +
            fmt_g(build_ms) + ", \"query_ms\": " + fmt_g(query_ms) + "}";
    return 0;
}

// what the readers understood, for tests and for checking a scene's files by eye
int run_tat_dump(const TatInputs &in, bool have_crop) {
    double T[16];
    mul16(in.init, in.trans, T);
    std::string o = "{\"trans\": " + json_mat(in.trans) + ", \"init\": " + json_mat(in.init) + ", \"transform\": " +
                    json_mat(T);
    if (have_crop) {
        o += std::string(", \"crop\": {\"orthogonal_axis\": \"") + "XYZ"[in.crop.axis] + "\", \"axis_min\": " +
             fmt_g(in.crop.axis_min) + ", \"axis_max\": " + fmt_g(in.crop.axis_max) + ", \"bounding_polygon\": [";
        for (size_t i = 0; i + 2 < in.crop.vertices.size(); i += 3)
            o += std::string(i ? ", " : "") + "[" + fmt_g(in.crop.vertices[i]) + ", " + fmt_g(in.crop.vertices[i + 1]) +
                 ", " + fmt_g(in.crop.vertices[i + 2]) + "]";
        o += "]}";
    }
    std::printf("%s}\n", o.c_str());
    return 0;
}

// ---- DTU mode ----------------------------------------------------------------------------------------

struct DtuInputs {
    std::vector<float> rec, gt;
    std::vector<uint8_t> mask;  // column-major
    int32_t dims[3] = {1, 1, 1};
    double origin[3] = {0, 0, 0}, res = 0.0, plane[4] = {0, 0, 0, 0};
};

// ObsMask, BB and Res of the mask file, P of the plane file
bool read_dtu_side_files(const Options &opt, DtuInputs &in, std::string &err) {
    std::vector<MatArray> a;
    if (!read_mat5(opt.dtu_mask, {{"ObsMask", true}, {"BB", false}, {"Res", false}}, a, err)) return false;
    const MatArray &m = a[0], &bb = a[1], &res = a[2];
    if (m.dims.size() < 2 || m.bytes.empty()) {
        err = opt.dtu_mask + ": ObsMask is not a non-empty 2-D or 3-D array";
        return false;
    }
    for (size_t k = 0; k < m.dims.size(); ++k) in.dims[k] = (int32_t)m.dims[k];  // each below 2^31 (read_mat5)
    if (bb.dims.size() != 2 || bb.dims[0] != 2 || bb.dims[1] != 3 || res.values.size() != 1) {
        err = opt.dtu_mask + ": BB is not 2x3 or Res is not a scalar";
        return false;
    }
    for (int k = 0; k < 3; ++k) in.origin[k] = bb.values[(size_t)(2 * k)];  // row 0 of a column-major 2x3
    in.res = res.values[0];
    if (!std::isfinite(in.origin[0]) || !std::isfinite(in.origin[1]) || !std::isfinite(in.origin[2]) ||
        !(in.res > 0.0) || !std::isfinite(in.res)) {
        err = opt.dtu_mask + ": BB is not finite or Res is not positive and finite";
        return false;
    }
    in.mask = std::move(a[0].bytes);
    if (!read_mat5(opt.dtu_plane, {{"P", false}}, a, err)) return false;
    if (a[0].values.size() != 4) {
        err = opt.dtu_plane + ": P does not hold 4 values";
        return false;
    }
    for (int k = 0; k < 4; ++k) {
        in.plane[k] = a[0].values[(size_t)k];
        if (!std::isfinite(in.plane[k])) {
            err = opt.dtu_plane + ": P is not finite";
            return false;
        }
    }
    return true;
}

// returns the exit status; appends "dtu": {...} to json
int run_dtu(const Options &opt, const DtuInputs &in, std::string &json) {
    apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
    if (!ctx) {
        std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
        return 1;
    }
    const int64_t n_in = (int64_t)(in.rec.size() / 3), n_gt = (int64_t)(in.gt.size() / 3);
    std::vector<float> data;
    double sort_ms = 0.0, rounds_ms = 0.0, build_ms = 0.0, query_ms = 0.0, mask_ms = 0.0, plane_ms = 0.0, stats_ms = 0.0;
    int32_t rounds = 0;
    bool ok = true;
    if (opt.dtu_no_thin) {
        data = in.rec;
    } else {
        std::vector<uint32_t> rank((size_t)std::max<int64_t>(n_in, 1));
        std::vector<int32_t> keep((size_t)std::max<int64_t>(n_in, 1));
        int64_t nk = 0;
        apd_eval_dtu_ranks(n_in, opt.dtu_seed, rank.data());
        const int st = apd_eval_radius_thin(ctx, n_in, in.rec.data(), opt.dtu_density, rank.data(), keep.data(), &nk);
        if (st != APD_OK) ok = fail_ctx(ctx, "apd_eval_radius_thin", st);
        else {
            apd_eval_get_thin_timing(ctx, &sort_ms, &rounds_ms, &rounds);
            data = gather(in.rec, keep, nk);
        }
    }
    const int64_t n_data = (int64_t)(data.size() / 3);
    std::vector<float> d_acc((size_t)std::max<int64_t>(n_data, 1)), d_comp((size_t)std::max<int64_t>(n_gt, 1));
    std::vector<uint8_t> inside((size_t)std::max<int64_t>(n_data, 1)), above((size_t)std::max<int64_t>(n_gt, 1));
    auto side = [&](const std::vector<float> &q, const std::vector<float> &t, std::vector<float> &dist) {
        int st = apd_eval_set_target(ctx, (int64_t)(t.size() / 3), t.data());
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_set_target", st);
        st = apd_eval_distances(ctx, (int64_t)(q.size() / 3), q.data(), opt.dtu_max_dist, dist.data(), 0, nullptr, nullptr);
        if (st != APD_OK) return fail_ctx(ctx, "apd_eval_distances", st);
        double b = 0.0, qm = 0.0;
        apd_eval_get_timing(ctx, &b, &qm, nullptr);
        build_ms += b;
        query_ms += qm;
        return true;
    };
    ok = ok && side(data, in.gt, d_acc) && side(in.gt, data, d_comp);
    if (ok) {
        int st = apd_eval_obs_mask(ctx, n_data, data.data(), in.dims, in.origin, in.res, in.mask.data(), inside.data());
        if (st != APD_OK) ok = fail_ctx(ctx, "apd_eval_obs_mask", st);
        else if ((st = apd_eval_half_space(ctx, n_gt, in.gt.data(), in.plane, above.data())) != APD_OK)
            ok = fail_ctx(ctx, "apd_eval_half_space", st);
        apd_eval_get_dtu_timing(ctx, &mask_ms, &plane_ms, nullptr);
    }
    // MATLAB's strict `< MaxDist`, as `<=` against the float below it
    const float limit = std::nextafterf(opt.dtu_max_dist, 0.0f);
    int64_t acc_n = 0, comp_n = 0;
    double acc_sum = 0.0, acc_med = 0.0, comp_sum = 0.0, comp_med = 0.0;
    if (ok) {
        double ms = 0.0;
        int st = apd_eval_masked_stats(ctx, n_data, d_acc.data(), inside.data(), limit, &acc_n, &acc_sum, &acc_med);
        if (st != APD_OK) ok = fail_ctx(ctx, "apd_eval_masked_stats", st);
        apd_eval_get_dtu_timing(ctx, nullptr, nullptr, &ms);
        stats_ms += ms;
        if (ok && (st = apd_eval_masked_stats(ctx, n_gt, d_comp.data(), above.data(), limit, &comp_n, &comp_sum,
                                              &comp_med)) != APD_OK)
            ok = fail_ctx(ctx, "apd_eval_masked_stats", st);
        apd_eval_get_dtu_timing(ctx, nullptr, nullptr, &ms);
        stats_ms += ms;
    }
    apd_eval_destroy(ctx);
    if (ok && !opt.thinned_out.empty()) {
        const std::vector<uint8_t> rgb(data.size(), 200);
        if (!write_ply_xyz_rgb(opt.thinned_out, data, rgb)) {
            std::fprintf(stderr, "apd_eval: cannot write %s\n", opt.thinned_out.c_str());
            ok = false;
        }
    }
    if (!ok) return 1;
    int64_t n_inside = 0, n_above = 0;
    for (int64_t i = 0; i < n_data; ++i) n_inside += inside[(size_t)i];
    for (int64_t i = 0; i < n_gt; ++i) n_above += above[(size_t)i];
    const double acc_mean = acc_n ? acc_sum / (double)acc_n : 0.0, comp_mean = comp_n ? comp_sum / (double)comp_n : 0.0;
    const double overall = (acc_mean + comp_mean) / 2.0;
    std::printf("DTU protocol: density %s, max_dist %s, %s\n", fmt_f32(opt.dtu_density).c_str(),
                fmt_f32(opt.dtu_max_dist).c_str(),
                opt.dtu_no_thin ? "not thinned" : ("seed " + std::to_string(opt.dtu_seed)).c_str());
    std::printf("input points: %lld\nthinned points: %lld\nin mask points: %lld\n", (long long)n_in, (long long)n_data,
                (long long)n_inside);
    std::printf("gt points: %lld\ngt above plane points: %lld\n", (long long)n_gt, (long long)n_above);
    std::printf("accuracy selected: %lld\ncompleteness selected: %lld\n", (long long)acc_n, (long long)comp_n);
    std::printf("accuracy mean: %s\naccuracy median: %s\ncompleteness mean: %s\ncompleteness median: %s\noverall: %s\n",
                fmt_g(acc_mean).c_str(), fmt_g(acc_med).c_str(), fmt_g(comp_mean).c_str(), fmt_g(comp_med).c_str(),
                fmt_g(overall).c_str());
    json += std::string("\"dtu\": {\"definition\": \"modelled on the DTU evaluation (radius thinning, observability "
                        "mask, table plane, mean and median of the distances below max_dist) with this project's own "
                        "contract: a seeded Philox order instead of randperm, doubles for the mask index, <= the float "
                        "below max_dist, no chunks; parity with the MATLAB code is not pinned\", \"density\": ") +
            fmt_g((double)opt.dtu_density) + ", \"max_dist\": " + fmt_g((double)opt.dtu_max_dist) + ", \"seed\": " +
            std::to_string(opt.dtu_seed) + ", \"thinned\": " + (opt.dtu_no_thin ? "false" : "true") +
            ", \"input_points\": " + std::to_string(n_in) + ", \"thinned_points\": " + std::to_string(n_data) +
            ", \"in_mask_points\": " + std::to_string(n_inside) + ", \"gt_points\": " + std::to_string(n_gt) +
            ", \"gt_above_plane_points\": " + std::to_string(n_above) + ", \"accuracy_selected\": " +
            std::to_string(acc_n) + ", \"completeness_selected\": " + std::to_string(comp_n) + ", \"accuracy_mean\": " +
            fmt_g(acc_mean) + ", \"accuracy_median\": " + fmt_g(acc_med) + ", \"completeness_mean\": " +
            fmt_g(comp_mean) + ", \"completeness_median\": " + fmt_g(comp_med) + ", \"overall\": " + fmt_g(overall) +
            ", \"thin_rounds\": " + std::to_string(rounds) + ", \"thin_sort_ms\": " + fmt_g(sort_ms) +
            ", \"thin_rounds_ms\": " + fmt_g(rounds_ms) + ", \"build_ms\": " + fmt_g(build_ms) + ", \"query_ms\": " +
            fmt_g(query_ms) + ", \"mask_ms\": " + fmt_g(mask_ms) + ", \"half_space_ms\": " + fmt_g(plane_ms) +
            ", \"stats_ms\": " + fmt_g(stats_ms) + "}";
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

// rendered: the ground-truth map of this view from --gt_cloud, else nullptr
void depth_view(const Options &opt, DepthStats &s, const Mat *rendered) {
    const std::string name = format_index(s.id);
    Mat da, wa, db, wb;
    const std::string fa = opt.dense + "/APD/" + name;
    if (!read_binmat_file(fa + "/depths.bin", da) || !read_binmat_file(fa + "/weak.bin", wa)) {
        s.error = "cannot read " + fa + "/depths.bin or weak.bin";
        return;
    }
    const bool has_wb = !opt.against.empty();
    if (rendered) {
        db = *rendered;
    } else if (has_wb) {
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

struct DepthInputs {
    std::vector<int> ids;
    RenderInputs gt;  // with --gt_cloud: the cloud and A's views (ids in the same order)
};

// compares views [lo, hi); maps (may be empty) holds the rendered ground truth of those views
void compare_views(const Options &opt, std::vector<DepthStats> &views, size_t lo, size_t hi,
                   const std::vector<Mat> &maps) {
    std::atomic<size_t> next{lo};
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t workers = std::max<size_t>(1, std::min<size_t>({(size_t)16, (size_t)(hw ? hw : 1), hi - lo}));
    std::vector<std::thread> pool;
    for (size_t w = 0; w < workers; ++w)
        pool.emplace_back([&] {
            for (size_t i; (i = next.fetch_add(1)) < hi;) depth_view(opt, views[i], maps.empty() ? nullptr : &maps[i - lo]);
        });
    for (auto &t : pool) t.join();
}

int run_depth(const Options &opt, const DepthInputs &in, std::string &json) {
    const std::vector<int> &ids = in.ids;
    std::vector<DepthStats> views(ids.size());
    for (size_t i = 0; i < ids.size(); ++i) views[i].id = ids[i];
    if (opt.gt_cloud.empty()) {
        compare_views(opt, views, 0, views.size(), {});
    } else {
        apd_eval_ctx *ctx = apd_eval_create(opt.gpu);
        if (!ctx) {
            std::fprintf(stderr, "apd_eval: %s (device %d)\n", apd_eval_last_error(nullptr), opt.gpu);
            return 1;
        }
        double render_ms = 0.0;
        for (size_t lo = 0; lo < views.size(); lo += kViewBatch) {
            const size_t hi = std::min(views.size(), lo + kViewBatch);
            std::vector<Mat> maps;
            if (!render_batch(ctx, in.gt.xyz, in.gt.views, lo, hi, opt.splat, maps, render_ms)) {
                apd_eval_destroy(ctx);
                return 1;
            }
            compare_views(opt, views, lo, hi, maps);
        }
        apd_eval_destroy(ctx);
    }

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
    json += "\"depth\": {\"a\": \"" + esc(opt.dense) + "\", \"b\": \"" +
            esc(!opt.against.empty() ? opt.against : !opt.gt_depth.empty() ? opt.gt_depth : opt.gt_cloud) +
            "\", \"b_is_gt_depth\": " + (opt.against.empty() ? "true" : "false") + ", \"views\": [" +
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
        if (a == "--no_refine") { opt.no_refine = true; continue; }
        if (a == "--no_scale") { opt.no_scale = true; continue; }
        if (a == "--tat_dump") { opt.tat_dump = true; continue; }
        if (a == "--dtu_no_thin") { opt.dtu_no_thin = opt.dtu_option_given = true; continue; }
        if (i + 1 >= argc) return bad("missing value for " + a);
        const std::string v = argv[++i];
        if (a == "--cloud") opt.cloud = v;
        else if (a == "--gt") opt.gt = v;
        else if (a == "--json") opt.json = v;
        else if (a == "--dense_folder") opt.dense = v;
        else if (a == "--against") opt.against = v;
        else if (a == "--gt_depth") opt.gt_depth = v;
        else if (a == "--gt_cloud") opt.gt_cloud = v;
        else if (a == "--render_gt") opt.render_gt = v;
        else if (a == "--scan") opt.scan = v;
        else if (a == "--out") opt.out = v;
        else if (a == "--gpu_index") opt.gpu = std::atoi(v.c_str());
        else if (a == "--gt_mlp") opt.gt_mlp = v;
        else if (a == "--accuracy_cloud_out") opt.accuracy_out = v;
        else if (a == "--completeness_cloud_out") opt.completeness_out = v;
        else if (a == "--tat_gt") opt.tat_gt = v;
        else if (a == "--tat_crop") opt.tat_crop = v;
        else if (a == "--tat_trans") opt.tat_trans = v;
        else if (a == "--init_trans") opt.init_trans = v;
        else if (a == "--aligned_cloud_out") opt.aligned_out = v;
        else if (a == "--dtu_gt") opt.dtu_gt = v;
        else if (a == "--dtu_mask") { opt.dtu_mask = v; opt.dtu_option_given = true; }
        else if (a == "--dtu_plane") { opt.dtu_plane = v; opt.dtu_option_given = true; }
        else if (a == "--thinned_cloud_out") { opt.thinned_out = v; opt.dtu_option_given = true; }
        else if (a == "--dtu_density") {
            // the bounds of include/apd_eval.h's radius: its fp32 square must be a normal number
            if (!parse_float(v, opt.dtu_density) || !(opt.dtu_density >= 1.1e-19f) || !(opt.dtu_density <= 1.8e19f))
                return bad("bad --dtu_density " + v);
            opt.dtu_option_given = true;
        } else if (a == "--dtu_max_dist") {
            if (!parse_float(v, opt.dtu_max_dist) || !(opt.dtu_max_dist > 0.0f) || !std::isfinite(opt.dtu_max_dist))
                return bad("bad --dtu_max_dist " + v);
            opt.dtu_option_given = true;
        } else if (a == "--dtu_seed") {
            char *end = nullptr;
            errno = 0;
            const unsigned long long s = std::strtoull(v.c_str(), &end, 10);
            if (v.empty() || v[0] == '-' || !end || *end != '\0' || errno != 0 || s > 0xFFFFFFFFull)
                return bad("bad --dtu_seed " + v + " (0..4294967295)");
            opt.dtu_seed = (uint32_t)s;
            opt.dtu_option_given = true;
        }
        else if (a == "--tau") {
            if (!parse_float(v, opt.tau) || !(opt.tau > 0.0f) || !std::isfinite(opt.tau)) return bad("bad --tau " + v);
            opt.tau_given = true;
        } else if (a == "--refine_stages") {
            std::istringstream ss(v);
            std::string tok;
            while (std::getline(ss, tok, ',')) {
                const size_t c = tok.find(':');
                float vox, mc;
                if (c == std::string::npos || !parse_float(tok.substr(0, c), vox) || !parse_float(tok.substr(c + 1), mc) ||
                    !(vox > 0.0f) || !std::isfinite(vox) || !(mc > 0.0f) || !std::isfinite(mc))
                    return bad("bad refinement stage '" + tok + "' (voxel:max_corr, both positive)");
                opt.stages.emplace_back(vox, mc);
            }
            if (opt.stages.empty() || opt.stages.size() > 16) return bad("--refine_stages takes 1 to 16 stages");
            opt.stages_given = true;
        }
        else if (a == "--cube_size") {
            if (!parse_int(v, opt.cube_size) || opt.cube_size < 2 || opt.cube_size > 16384)
                return bad("bad --cube_size " + v + " (2..16384)");
            opt.cube_given = true;
        }
        else if (a == "--splat") {
            if (!parse_int(v, opt.splat) || opt.splat < 0 || opt.splat > 16) return bad("bad --splat " + v + " (0..16)");
            opt.splat_given = true;
        } else if (a == "--visible_views") {
            if (!parse_int(v, opt.visible_views) || opt.visible_views < 1) return bad("bad --visible_views " + v);
        } else if (a == "--occlusion_tol") {
            if (!parse_float(v, opt.occlusion_tol) || !(opt.occlusion_tol >= 0.0f) || !std::isfinite(opt.occlusion_tol))
                return bad("bad --occlusion_tol " + v);
            opt.occlusion_given = true;
        } else if (a == "--max_dist") {
            if (!parse_float(v, opt.max_dist) || !(opt.max_dist >= 0.0f)) return bad("bad --max_dist " + v);
        } else if (a == "--voxel") {
            if (!parse_float(v, opt.voxel) || !(opt.voxel >= 0.0f) || !std::isfinite(opt.voxel))
                return bad("bad --voxel " + v);
            opt.voxel_given = true;
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
    const bool tat_mode = !opt.tat_gt.empty() || opt.tat_dump;
    const bool scanner_mode = !opt.gt_mlp.empty();
    const bool dtu_mode = !opt.dtu_gt.empty();
    const bool cloud_mode = !scanner_mode && !tat_mode && !dtu_mode && (!opt.cloud.empty() || !opt.gt.empty());
    const bool depth_mode = !opt.dense.empty() || !opt.against.empty() || !opt.gt_depth.empty() || !opt.gt_cloud.empty();
    const bool render_mode = !opt.render_gt.empty();
    if (scanner_mode) {
        if (opt.cloud.empty()) return bad("scanner mode needs --cloud and --gt_mlp");
        if (!opt.gt.empty() || depth_mode || render_mode)
            return bad("--gt_mlp excludes --gt, --dense_folder and --render_gt");
        if (opt.visible_views > 0 || !opt.scan.empty()) return bad("--gt_mlp does not take --visible_views / --scan");
        if (!opt.voxel_given) opt.voxel = 0.01f;  // the scoring voxel
        if (!(opt.voxel > 0.0f)) return bad("--gt_mlp needs a positive --voxel");
        if (!opt.splat_given) opt.splat = 1;
        if (opt.max_dist >= 0.0f)
            for (float t : opt.tol)
                if (t > opt.max_dist) return bad("a tolerance exceeds --max_dist");
    } else if (opt.cube_given || !opt.accuracy_out.empty() || !opt.completeness_out.empty()) {
        return bad("--cube_size / --accuracy_cloud_out / --completeness_cloud_out without --gt_mlp");
    }
    if (tat_mode) {
        if (scanner_mode || depth_mode || render_mode || !opt.gt.empty() || opt.visible_views > 0 || !opt.scan.empty() ||
            opt.voxel_given)
            return bad("--tat_gt excludes the other modes and their options");
        if (opt.no_refine && opt.stages_given) return bad("--no_refine with --refine_stages");
        if (!opt.tat_dump) {
            if (opt.cloud.empty() || opt.tat_gt.empty() || opt.tat_crop.empty() || !opt.tau_given)
                return bad("Tanks and Temples mode needs --cloud, --tat_gt, --tat_crop and --tau");
            if (!opt.stages_given)
                opt.stages = {{opt.tau, 80.0f * opt.tau}, {opt.tau / 2.0f, 20.0f * opt.tau}, {opt.tau / 2.0f, 2.0f * opt.tau}};
        }
    } else if (!opt.tat_crop.empty() || !opt.tat_trans.empty() || !opt.init_trans.empty() || !opt.aligned_out.empty() ||
               opt.tau_given || opt.no_refine || opt.no_scale || opt.stages_given) {
        return bad("--tat_crop / --tat_trans / --init_trans / --tau / --no_refine / --refine_stages / --no_scale / "
                   "--aligned_cloud_out without --tat_gt");
    }
    if (dtu_mode) {
        if (scanner_mode || tat_mode || depth_mode || render_mode || !opt.gt.empty() || opt.visible_views > 0 ||
            !opt.scan.empty() || opt.voxel_given || opt.max_dist >= 0.0f)
            return bad("--dtu_gt excludes the other modes and their options");
        if (opt.cloud.empty() || opt.dtu_mask.empty() || opt.dtu_plane.empty())
            return bad("DTU mode needs --cloud, --dtu_gt, --dtu_mask and --dtu_plane");
    } else if (opt.dtu_option_given) {
        return bad("--dtu_mask / --dtu_plane / --dtu_density / --dtu_max_dist / --dtu_seed / --dtu_no_thin / "
                   "--thinned_cloud_out without --dtu_gt");
    }
    if (!cloud_mode && !depth_mode && !render_mode && !scanner_mode && !tat_mode && !dtu_mode) return bad("nothing to do");
    if (cloud_mode && (opt.cloud.empty() || opt.gt.empty())) return bad("cloud mode needs --cloud and --gt");
    if (depth_mode && (opt.dense.empty() ||
                       (int)!opt.against.empty() + (int)!opt.gt_depth.empty() + (int)!opt.gt_cloud.empty() != 1))
        return bad("depth mode needs --dense_folder and exactly one of --against / --gt_depth / --gt_cloud");
    if (render_mode && (opt.scan.empty() || opt.out.empty())) return bad("render mode needs --render_gt, --scan and --out");
    if (!render_mode && !opt.out.empty()) return bad("--out without --render_gt");
    if (opt.visible_views > 0 && (!cloud_mode || opt.scan.empty()))
        return bad("--visible_views needs cloud mode and --scan");
    if (!opt.scan.empty() && !render_mode && opt.visible_views == 0)
        return bad("--scan with nothing that uses it (--render_gt or --visible_views)");
    if (opt.splat_given && !render_mode && opt.visible_views == 0 && opt.gt_cloud.empty() && !scanner_mode)
        return bad("--splat with nothing that renders");
    if (opt.occlusion_given && opt.visible_views == 0) return bad("--occlusion_tol without --visible_views");
    if (cloud_mode && opt.max_dist >= 0.0f)
        for (float t : opt.tol)
            if (t > opt.max_dist) return bad("a tolerance exceeds --max_dist");

    // every input is read here, before any device context exists: an unreadable one exits 2 without a GPU
    DepthInputs din;
    CloudInputs cin;
    RenderInputs rin;
    ScannerInputs sin;
    TatInputs tin;
    std::string err;
    auto unreadable = [&] {
        std::fprintf(stderr, "apd_eval: %s\n", err.c_str());
        return 2;
    };
    if (depth_mode) {
        if (!read_pair_ids(opt.dense, din.ids, err)) return unreadable();
        if (!opt.gt_cloud.empty() &&
            (!read_ply_xyz(opt.gt_cloud, din.gt.xyz, err) || !load_scan_views(opt.dense, din.gt.views, err)))
            return unreadable();
    }
    if (cloud_mode) {
        if (!read_ply_xyz(opt.cloud, cin.rec.xyz, err) || !read_ply_xyz(opt.gt, cin.gt.xyz, err)) return unreadable();
        if (opt.visible_views > 0 && !load_scan_views(opt.scan, cin.views, err)) return unreadable();
    }
    if (render_mode && (!read_ply_xyz(opt.render_gt, rin.xyz, err) || !load_scan_views(opt.scan, rin.views, err)))
        return unreadable();
    if (tat_mode) {
        identity16(tin.trans);
        identity16(tin.init);
        if ((!opt.tat_crop.empty() && !read_tat_crop(opt.tat_crop, tin.crop, err)) ||
            (!opt.tat_trans.empty() && !read_matrix4(opt.tat_trans, tin.trans, err)) ||
            (!opt.init_trans.empty() && !read_matrix4(opt.init_trans, tin.init, err)))
            return unreadable();
        if (opt.tat_dump) return run_tat_dump(tin, !opt.tat_crop.empty());
        if (!read_ply_xyz(opt.cloud, tin.rec, err) || !read_ply_xyz(opt.tat_gt, tin.gt, err)) return unreadable();
    }
    DtuInputs uin;
    if (dtu_mode && (!read_dtu_side_files(opt, uin, err) || !read_ply_xyz(opt.cloud, uin.rec, err) ||
                     !read_ply_xyz(opt.dtu_gt, uin.gt, err)))
        return unreadable();
    if (scanner_mode) {
        std::vector<MlpMesh> meshes;
        if (!read_ply_xyz(opt.cloud, sin.rec.xyz, err) || !read_mlp(opt.gt_mlp, meshes, err)) return unreadable();
        for (const MlpMesh &m : meshes) {
            Scanner s;
            s.ply = m.ply_path;
            if (!read_ply_xyz(m.ply_path, s.xyz, err)) return unreadable();
            mlp_to_world(m, s.xyz, s.origin);
            if (!std::isfinite(s.origin[0]) || !std::isfinite(s.origin[1]) || !std::isfinite(s.origin[2])) {
                err = opt.gt_mlp + ": the scanner position of " + m.ply_path + " is not finite";
                return unreadable();
            }
            sin.scanners.push_back(std::move(s));
        }
    }

    std::string json = "{";
    int status = 0;
    bool first = true;
    auto sep = [&] {
        if (!first) json += ", ";
        first = false;
    };
    if (depth_mode) {
        sep();
        status = run_depth(opt, din, json);
        if (status != 0 && json.size() == 1) json += "\"depth\": null";
    }
    if (cloud_mode) {
        sep();
        const int st = run_cloud(opt, cin, json);
        status = std::max(status, st);
        if (st != 0) json += "\"cloud\": null";
    }
    if (scanner_mode) {
        sep();
        const int st = run_scanners(opt, sin, json);
        status = std::max(status, st);
        if (st != 0) json += "\"scanners\": null";
    }
    if (tat_mode) {
        sep();
        const int st = run_tat(opt, tin, json);
        status = std::max(status, st);
        if (st != 0) json += "\"tat\": null";
    }
    if (dtu_mode) {
        sep();
        const int st = run_dtu(opt, uin, json);
        status = std::max(status, st);
        if (st != 0) json += "\"dtu\": null";
    }
    if (render_mode) {
        sep();
        const int st = run_render(opt, rin, json);
        status = std::max(status, st);
        if (st != 0) json += "\"render\": null";
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
