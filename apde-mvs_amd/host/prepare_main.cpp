// prepare_main.cpp — `apd_prepare`: a COLMAP sparse model (cameras, images, points3D; PINHOLE images)
// -> the scan layout the depth binary reads: cams/%08d_cam.txt, images/, pair.txt, sparse/0/.
// The reference's tools/colmap2mvsnet.py without cv2/tqdm; covisibility pair counts and per-image depth
// ranks on the device (include/apd_prep.h). Every input is read and validated before a device context
// exists (exit 2); device or write failures exit 1.
// With --undistort the images of cameras with a distorted model are warped on the device into pinhole
// images of the same size and fx fy cx cy (include/apd_prep.h, "Undistortion"), their cameras are
// written as PINHOLE and their keypoints are carried along; pinhole cameras go the usual way.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/apd_prep.h"
#include "image.h"
#include "io.h"

using namespace apdhost;

namespace {

const char *kUsage =
    "usage: apd_prepare --dense_folder IN --save_folder OUT [options]\n"
    "  A COLMAP sparse model and its undistorted (PINHOLE) images -> OUT/cams, OUT/images, OUT/pair.txt,\n"
    "  OUT/sparse/0: the scan layout `apd` reads. Distorted images: see --undistort.\n"
    "  --dense_folder IN        holds sparse/ and images/ unless the next two say otherwise\n"
    "  --model_dir DIR          cameras/images/points3D (default IN/sparse)\n"
    "  --image_dir DIR          the images; names may carry a sub-directory (default IN/images)\n"
    "  --model_ext .txt|.bin    (default .txt)\n"
    "  --max_d N                depth hypotheses; 0: from the inverse-depth rule (default 192)\n"
    "  --interval_scale S       (default 1)\n"
    "  --scale_factor F         divide image size and intrinsics by F (default 1)\n"
    "  --sequential | --no-sequential   +-k window (default) or covisibility score on the device\n"
    "  --sequential_k K         (default 5)\n"
    "  --max_views N            sources per view with --no-sequential (default 20)\n"
    "  --theta0 --sigma1 --sigma2      accepted and unused, as in the reference\n"
    "  --device G               HIP device (default 0)\n"
    "  --json OUT.json          counts and device times\n"
    "  --undistort              also accept SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, FULL_OPENCV,\n"
    "                           SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE and THIN_PRISM_FISHEYE cameras (not FOV):\n"
    "                           their images are warped on the device to pinhole images of the same size and\n"
    "                           fx fy cx cy (bilinear, black where there is no source) and written as PNG, their\n"
    "                           cameras become PINHOLE and their keypoints in sparse/0/images.txt are undistorted\n"
    "                           ((-1, -1) where that fails). Without it such models are rejected.\n"
    "  Images are copied byte for byte when they are JPEG/PNG, need no padding and F = 1; otherwise they are\n"
    "  padded bottom/right to the largest size, resized (nearest) and written as 8-bit colour PNG.\n";

struct Options {
    std::string dense, save, model_dir, image_dir, ext = ".txt", json;
    int max_d = 192, seq_k = 5, max_views = 20, device = 0;
    double interval_scale = 1.0, scale = 1.0;
    bool sequential = true, undistort = false;
};

bool parse_double(const std::string &s, double &v) {
    char *end = nullptr;
    v = std::strtod(s.c_str(), &end);
    return !s.empty() && end && *end == '\0' && std::isfinite(v);
}
bool parse_int(const std::string &s, int lo, int hi, int &v) {
    char *end = nullptr;
    const long l = std::strtol(s.c_str(), &end, 10);
    if (s.empty() || !end || *end != '\0' || l < lo || l > hi) return false;
    v = (int)l;
    return true;
}

int usage_error(const std::string &msg) {
    std::cerr << "apd_prepare: " << msg << "\n" << kUsage;
    return 2;
}

std::string fmt_g(double v) {
    char b[64];
    if (std::isfinite(v)) std::snprintf(b, sizeof b, "%.17g", v);
    else std::snprintf(b, sizeof b, "null");
    return b;
}

}  // namespace

int main(int argc, char **argv) {
    Options opt;
    bool seq_set = false, noseq_set = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "--help" || a == "-h") { std::cout << kUsage; return 0; }
        if (a == "--sequential") { seq_set = true; continue; }
        if (a == "--no-sequential") { noseq_set = true; continue; }
        if (a == "--undistort") { opt.undistort = true; continue; }
        if (i + 1 >= argc) return usage_error("missing value for " + a);
        const std::string v = argv[++i];
        double unused;
        bool ok = true;
        if (a == "--dense_folder") opt.dense = v;
        else if (a == "--save_folder") opt.save = v;
        else if (a == "--model_dir") opt.model_dir = v;
        else if (a == "--image_dir") opt.image_dir = v;
        else if (a == "--model_ext") opt.ext = v;
        else if (a == "--json") opt.json = v;
        else if (a == "--max_d") ok = parse_int(v, 0, 1000000, opt.max_d);
        else if (a == "--sequential_k") ok = parse_int(v, 0, 1000000, opt.seq_k);
        else if (a == "--max_views") ok = parse_int(v, 0, 1000000, opt.max_views);
        else if (a == "--device") ok = parse_int(v, 0, 1023, opt.device);
        else if (a == "--interval_scale") ok = parse_double(v, opt.interval_scale) && opt.interval_scale > 0;
        else if (a == "--scale_factor") ok = parse_double(v, opt.scale) && opt.scale > 0;
        else if (a == "--theta0" || a == "--sigma1" || a == "--sigma2") ok = parse_double(v, unused);
        else return usage_error("unknown option " + a);
        if (!ok) return usage_error("bad value '" + v + "' for " + a);
    }
    if (seq_set && noseq_set) return usage_error("--sequential and --no-sequential exclude each other");
    opt.sequential = !noseq_set;
    if (opt.save.empty()) return usage_error("--save_folder is required");
    if (opt.dense.empty() && (opt.model_dir.empty() || opt.image_dir.empty()))
        return usage_error("--dense_folder is required (or both --model_dir and --image_dir)");
    if (opt.ext != ".txt" && opt.ext != ".bin") return usage_error("--model_ext is .txt or .bin");
    if (opt.max_d == 1) return usage_error("--max_d 1 leaves no depth interval");
    if (opt.model_dir.empty()) opt.model_dir = opt.dense + "/sparse";
    if (opt.image_dir.empty()) opt.image_dir = opt.dense + "/images";

    // ---- every input, before a device context exists ----
    ColmapModel model;
    PrepArrays arr;
    std::string err;
    if (!read_colmap_model(opt.model_dir, opt.ext, model, err, opt.undistort) || !colmap_prep_arrays(model, arr, err)) {
        std::cerr << "apd_prepare: " << err << "\n";
        if (!opt.undistort && err.find("unsupported camera model") != std::string::npos &&
            err.find("unsupported camera model FOV") == std::string::npos)
            std::cerr << "apd_prepare: (or pass --undistort, if it is one of the models --help lists)\n";
        return 2;
    }
    const int n = (int)model.images.size();
    if (n > APD_PREP_MAX_IMAGES) {
        std::cerr << "apd_prepare: " << n << " images, more than " << APD_PREP_MAX_IMAGES << "\n";
        return 2;
    }
    std::vector<std::string> names;
    for (const ColmapImage &im : model.images) names.push_back(im.name);
    std::vector<int> widths, heights;
    if (!scan_image_sizes(opt.image_dir, names, widths, heights, err)) {
        std::cerr << "apd_prepare: " << err << "\n";
        return 2;
    }
    {
        const int max_w = *std::max_element(widths.begin(), widths.end());
        const int max_h = *std::max_element(heights.begin(), heights.end());
        if ((int)((double)max_w / opt.scale) < 1 || (int)((double)max_h / opt.scale) < 1) {
            std::cerr << "apd_prepare: --scale_factor leaves no pixels\n";
            return 2;
        }
    }

    // distorted cameras (only with --undistort): the library's own argument rules, and an image of
    // the size its camera states, since that is the size its parameters are for
    auto source_camera = [&](uint32_t id) -> const ColmapCamera & {
        for (const ColmapCamera &c : model.cameras)
            if (c.id == id) return c;
        return model.cameras[0];  // read_colmap_model has checked that every image's camera exists
    };
    std::vector<char> distorted((size_t)n, 0);
    int n_distorted = 0;
    for (int i = 0; i < n; ++i) {
        const ColmapCamera &c = source_camera(model.images[(size_t)i].camera_id);
        const int id = colmap_model_id(c.model);
        if (id <= 1) continue;
        const bool one_f = c.params.size() == 4 || c.params.size() == 5;
        if (!(c.params[0] > 0) || (!one_f && !(c.params[1] > 0))) {
            std::cerr << "apd_prepare: camera " << c.id << ": a focal length that is not positive\n";
            return 2;
        }
        if ((uint64_t)widths[(size_t)i] != c.width || (uint64_t)heights[(size_t)i] != c.height) {
            std::cerr << "apd_prepare: " << names[(size_t)i] << " is " << widths[(size_t)i] << "x" << heights[(size_t)i]
                      << ", its " << c.model << " camera " << c.id << " says " << c.width << "x" << c.height << "\n";
            return 2;
        }
        distorted[(size_t)i] = 1;
        ++n_distorted;
    }

    // ---- device: depth ranks, and pair counts unless sequential ----
    apd_prep_ctx *ctx = apd_prep_create(opt.device);
    if (!ctx) {
        std::cerr << "apd_prepare: " << apd_prep_last_error(nullptr) << "\n";
        return 1;
    }
    auto dev_fail = [&](const char *what) {
        std::cerr << "apd_prepare: " << what << ": " << apd_prep_last_error(ctx) << "\n";
        apd_prep_destroy(ctx);
        return 1;
    };
    if (apd_prep_set_model(ctx, n, arr.rot.data(), arr.trans.data(), arr.centres.data(), (int64_t)model.point_ids.size(),
                           model.xyz.data(), (int64_t)arr.obs_point.size(), arr.obs_offset.data(),
                           arr.obs_point.data()) != APD_OK)
        return dev_fail("apd_prep_set_model");
    const double fractions[2] = {0.01, 0.99};
    std::vector<double> z_at(2 * (size_t)n);
    std::vector<int64_t> n_obs((size_t)n);
    if (apd_prep_depth_ranks(ctx, 2, fractions, z_at.data(), n_obs.data()) != APD_OK)
        return dev_fail("apd_prep_depth_ranks");
    ViewSelection sel;
    uint64_t records = 0;
    if (opt.sequential) {
        sel = select_sequential(n, opt.seq_k);
    } else {
        std::vector<uint32_t> shared((size_t)n * n), narrow((size_t)n * n);
        if (apd_prep_pair_counts(ctx, apd_prep_cos_gate(1.0), APD_PREP_ATOMICS_DEFAULT, shared.data(), narrow.data(),
                                 &records) != APD_OK)
            return dev_fail("apd_prep_pair_counts");
        sel = select_scored(n, shared.data(), narrow.data(), opt.max_views);
    }
    double tracks_ms = 0, pairs_ms = 0, records_ms = 0, ranks_ms = 0;
    apd_prep_get_timing(ctx, &tracks_ms, &pairs_ms, &records_ms, &ranks_ms);
    if (n_distorted == 0) {  // else the context lives until the images are warped
        apd_prep_destroy(ctx);
        ctx = nullptr;
    }

    // ---- write ----
    auto write_fail = [&](const std::string &what) {
        std::cerr << "apd_prepare: cannot write " << what << "\n";
        if (ctx) apd_prep_destroy(ctx);
        return 1;
    };
    if (!make_dir(opt.save) || !make_dir(opt.save + "/cams") || !make_dir(opt.save + "/images") ||
        !make_dir(opt.save + "/sparse") || !make_dir(opt.save + "/sparse/0"))
        return write_fail(opt.save);
    std::vector<ColmapCamera> cams = model.cameras;
    for (ColmapCamera &c : cams) {
        if (colmap_model_id(c.model) > 1) {  // the warped images' camera: PINHOLE fx fy cx cy
            const bool one_f = c.params.size() == 4 || c.params.size() == 5;
            const std::vector<double> p = c.params;
            c.params = one_f ? std::vector<double>{p[0], p[0], p[1], p[2]} : std::vector<double>{p[0], p[1], p[2], p[3]};
            c.model = "PINHOLE";
        }
        for (double &p : c.params) p = p / opt.scale;
    }
    auto camera_of = [&](uint32_t id) -> ColmapCamera & {
        for (ColmapCamera &c : cams)
            if (c.id == id) return c;
        return cams[0];  // read_colmap_model has checked that every image's camera exists
    };
    for (int i = 0; i < n; ++i) {
        const ColmapCamera &c = camera_of(model.images[(size_t)i].camera_id);
        const bool simple = c.model == "SIMPLE_PINHOLE";
        const double fx = c.params[0], fy = simple ? c.params[0] : c.params[1];
        const double cx = c.params[simple ? 1 : 2], cy = c.params[simple ? 2 : 3];
        const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
        double dmin = 0.0, dmax = 0.0;
        if (n_obs[(size_t)i] > 0) {
            dmin = z_at[2 * (size_t)i] * 0.75;
            dmax = z_at[2 * (size_t)i + 1] * 1.25;
        }
        double num = (double)opt.max_d;
        if (opt.max_d == 0) num = (1 / dmin - 1 / dmax) / (1 / dmin - 1 / (dmin + dmin / fx));
        const double interval = (dmax - dmin) / (num - 1) / opt.interval_scale;
        if (!write_cam_txt(opt.save + "/cams/" + format_index(i) + "_cam.txt", &arr.rot[9 * (size_t)i],
                           &arr.trans[3 * (size_t)i], K, dmin, interval, num, dmax))
            return write_fail("cams/" + format_index(i) + "_cam.txt");
    }
    if (!write_pair_txt(opt.save + "/pair.txt", sel)) return write_fail("pair.txt");

    int copied = 0, out_w = 0, out_h = 0;
    std::vector<std::string> out_names;
    double ud_upload_ms = 0, ud_kernel_ms = 0, ud_download_ms = 0;
    ScanImageWarp warp;
    warp.mask = distorted;
    warp.apply = [&](size_t i, Bgr8 &img, std::string &e) {
        const ColmapCamera &c = source_camera(model.images[i].camera_id);
        const bool one_f = c.params.size() == 4 || c.params.size() == 5;
        const double K[4] = {c.params[0], one_f ? c.params[0] : c.params[1], c.params[one_f ? 1 : 2],
                             c.params[one_f ? 2 : 3]};
        std::vector<uint8_t> out(img.px.size());
        if (apd_prep_undistort_bgr8(ctx, colmap_model_id(c.model), c.params.data(), (int32_t)c.params.size(), img.width,
                                    img.height, img.px.data(), K, img.width, img.height, out.data()) != APD_OK) {
            e = std::string("apd_prep_undistort_bgr8: ") + apd_prep_last_error(ctx);
            return false;
        }
        double up = 0, ke = 0, down = 0;
        apd_prep_get_undistort_timing(ctx, &up, &ke, &down);
        ud_upload_ms += up;
        ud_kernel_ms += ke;
        ud_download_ms += down;
        img.px.swap(out);
        return true;
    };
    const bool converted_ok = convert_scan_images(opt.image_dir, names, widths, heights, opt.scale, opt.save + "/images",
                                                  out_names, out_w, out_h, copied, err, n_distorted ? &warp : nullptr);
    if (ctx) {
        apd_prep_destroy(ctx);
        ctx = nullptr;
    }
    if (!converted_ok) {
        std::cerr << "apd_prepare: " << err << "\n";
        return 1;
    }
    const int converted = n - copied;
    std::vector<ColmapImage> out_images = model.images;
    int64_t unresolved = 0;
    for (int i = 0; i < n; ++i) {
        if (distorted[(size_t)i]) {  // the list keeps its length and order: points3D refers to it by index
            const ColmapCamera &c = source_camera(model.images[(size_t)i].camera_id);
            std::vector<double> &xy = out_images[(size_t)i].xy;
            int64_t bad = 0;
            if (apd_prep_undistort_xy(colmap_model_id(c.model), c.params.data(), (int32_t)c.params.size(),
                                      (int64_t)(xy.size() / 2), xy.data(), xy.data(), &bad) != APD_OK) {
                std::cerr << "apd_prepare: apd_prep_undistort_xy failed for image " << model.images[(size_t)i].id << "\n";
                return 1;
            }
            unresolved += bad;
        }
        out_images[(size_t)i].name = out_names[(size_t)i];
        ColmapCamera &c = camera_of(model.images[(size_t)i].camera_id);
        c.width = (uint64_t)out_w;
        c.height = (uint64_t)out_h;
    }
    if (!write_colmap_cameras_txt(opt.save + "/sparse/0/cameras.txt", cams)) return write_fail("sparse/0/cameras.txt");
    if (!write_colmap_images_txt(opt.save + "/sparse/0/images.txt", out_images)) return write_fail("sparse/0/images.txt");
    if (!copy_file(opt.model_dir + "/points3D" + opt.ext, opt.save + "/sparse/0/points3D" + opt.ext))
        return write_fail("sparse/0/points3D" + opt.ext);

    std::string json = "{\"images\": " + std::to_string(n) + ", \"points\": " + std::to_string(model.point_ids.size()) +
                       ", \"observations\": " + std::to_string(arr.obs_point.size()) + ", \"sequential\": " +
                       (opt.sequential ? "true" : "false") + ", \"pair_records\": " + std::to_string(records) +
                       ", \"width\": " + std::to_string(out_w) + ", \"height\": " + std::to_string(out_h) +
                       ", \"images_copied\": " + std::to_string(copied) + ", \"images_converted\": " +
                       std::to_string(converted) + ", \"tracks_ms\": " + fmt_g(tracks_ms) + ", \"pairs_ms\": " +
                       fmt_g(pairs_ms) + ", \"records_ms\": " + fmt_g(records_ms) + ", \"ranks_ms\": " + fmt_g(ranks_ms);
    if (opt.undistort)
        json += ", \"images_undistorted\": " + std::to_string(n_distorted) + ", \"keypoints_unresolved\": " +
                std::to_string(unresolved) + ", \"undistort_upload_ms\": " + fmt_g(ud_upload_ms) +
                ", \"undistort_kernel_ms\": " + fmt_g(ud_kernel_ms) + ", \"undistort_download_ms\": " +
                fmt_g(ud_download_ms);
    json += "}";
    std::cout << json << std::endl;
    if (!opt.json.empty()) {
        std::ofstream o(opt.json);
        o << json << "\n";
        o.flush();
        if (!o) return write_fail(opt.json);
    }
    return 0;
}
