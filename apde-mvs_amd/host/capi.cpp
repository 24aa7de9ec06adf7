// capi.cpp -- C entry points over the host helpers (image decode, OpenCV-rule resize, cam.txt / pair.txt
// parsing, the PLY / MeshLab project readers and the coloured-cloud writer) as libapdhost.so: used by the
// multi-process scan runner (apde-mvs_amd/scan_runner.py) and by the CPU tests (tests/test_host.py,
// tests/test_eval_protocol_host.py).
#include <cstring>
#include <string>

#include "image.h"
#include "io.h"

using namespace apdhost;

extern "C" {
// decode an image file to gray; returns width*height (copied into out if out_cap suffices) or < 0
long apdhost_read_gray8(const char *path, unsigned char *out, long out_cap, int *w, int *h) {
    Gray8 g;
    std::string err;
    if (!read_gray8(path, g, err)) return -1;
    *w = g.width;
    *h = g.height;
    const long n = (long)g.px.size();
    if (out && out_cap >= n) memcpy(out, g.px.data(), n);
    return n;
}
void apdhost_resize_linear_f32(const float *src, int sw, int sh, float *dst, int dw, int dh) {
    resize_linear_f32(src, sw, sh, dst, dw, dh);
}
void apdhost_resize_nearest(const void *src, int sw, int sh, void *dst, int dw, int dh, int elem) {
    resize_nearest(src, sw, sh, dst, dw, dh, elem);
}
int apdhost_read_camera(const char *path, apd_camera *cam) { return read_camera(path, *cam) ? 0 : -1; }
// ReadBinMat (APD.cpp:18-56): payload bytes (copied into out if out_cap suffices) or -1 when the file
// is missing, malformed or truncated (then no Mat at all, not a partly filled one)
long apdhost_read_binmat(const char *path, void *out, long out_cap, int *rows, int *cols, int *type) {
    Mat m;
    if (!read_binmat_file(path, m)) return m.empty() ? -1 : -2;
    *rows = m.rows;
    *cols = m.cols;
    *type = m.type;
    const long n = (long)m.size_bytes();
    if (out && out_cap >= n) memcpy(out, m.bytes(), n);
    return n;
}
}

#include "fusion.h"
extern "C" {
// cv::imread(IMREAD_COLOR): BGR bytes; same return convention as apdhost_read_gray8
long apdhost_read_bgr8(const char *path, unsigned char *out, long out_cap, int *w, int *h) {
    Bgr8 g;
    std::string err;
    if (!read_bgr8(path, g, err)) return -1;
    *w = g.width;
    *h = g.height;
    const long n = (long)g.px.size();
    if (out && out_cap >= n) memcpy(out, g.px.data(), n);
    return n;
}
void apdhost_resize_linear_u8c3(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh) {
    resize_linear_u8c3(src, sw, sh, dst, dw, dh);
}
int apdhost_write_png_gray8(const char *path, const unsigned char *px, int w, int h) {
    return write_png_gray8(path, px, w, h) ? 0 : -1;
}
static void put_err(const std::string &e, char *err, long err_cap) {
    if (err && err_cap > 0) {
        strncpy(err, e.c_str(), (size_t)err_cap - 1);
        err[err_cap - 1] = '\0';
    }
}
// read_ply_xyz: the vertex count (3 floats each copied into out if out_cap floats suffice) or -1 with
// the message in err
long apdhost_read_ply_xyz(const char *path, float *out, long out_cap, char *err, long err_cap) {
    std::vector<float> xyz;
    std::string e;
    if (!read_ply_xyz(path, xyz, e)) { put_err(e, err, err_cap); return -1; }
    if (out && out_cap >= (long)xyz.size() && !xyz.empty()) memcpy(out, xyz.data(), xyz.size() * 4);
    return (long)(xyz.size() / 3);
}
int apdhost_write_ply_xyz_rgb(const char *path, const float *xyz, const unsigned char *rgb, long n) {
    if (n < 0 || (n > 0 && (!xyz || !rgb))) return -1;
    return write_ply_xyz_rgb(path, std::vector<float>(xyz, xyz + 3 * n), std::vector<uint8_t>(rgb, rgb + 3 * n)) ? 0 : -1;
}
// read_mlp: the number of meshes or -1 with the message in err. mats: 16 doubles per mesh (filled for
// the first mesh_cap meshes); paths: the PLY paths joined by '\n' (if paths_cap suffices)
long apdhost_read_mlp(const char *path, double *mats, long mesh_cap, char *paths, long paths_cap, char *err,
                      long err_cap) {
    std::vector<MlpMesh> meshes;
    std::string e;
    if (!read_mlp(path, meshes, e)) { put_err(e, err, err_cap); return -1; }
    std::string joined;
    for (size_t i = 0; i < meshes.size(); ++i) {
        if (mats && (long)i < mesh_cap) memcpy(mats + 16 * i, meshes[i].M, sizeof meshes[i].M);
        joined += (i ? "\n" : "") + meshes[i].ply_path;
    }
    if (paths && paths_cap > (long)joined.size()) memcpy(paths, joined.c_str(), joined.size() + 1);
    return (long)meshes.size();
}
// world points and scanner origin of mesh `index` of a project: the point count (copied into out if
// out_cap floats suffice) or -1 with the message in err
long apdhost_read_mlp_scan(const char *path, long index, float *out, long out_cap, float *origin, char *err,
                           long err_cap) {
    std::vector<MlpMesh> meshes;
    std::vector<float> xyz;
    std::string e;
    if (!read_mlp(path, meshes, e)) { put_err(e, err, err_cap); return -1; }
    if (index < 0 || index >= (long)meshes.size()) { put_err("no such mesh", err, err_cap); return -1; }
    if (!read_ply_xyz(meshes[(size_t)index].ply_path, xyz, e)) { put_err(e, err, err_cap); return -1; }
    float o[3];
    mlp_to_world(meshes[(size_t)index], xyz, o);
    if (origin) memcpy(origin, o, sizeof o);
    if (out && out_cap >= (long)xyz.size() && !xyz.empty()) memcpy(out, xyz.data(), xyz.size() * 4);
    return (long)(xyz.size() / 3);
}
float apdhost_angle_cut_lt(float t) { return angle_cut_lt(t); }
float apdhost_view_cut_deg(float d) { return view_cut_deg(d); }

// ---- apd_prepare's host side (tests/test_prep_host.py) ----
// read_colmap_model + colmap_prep_arrays; a canonical dump (hex floats, one record per line, images in
// ascending id) goes to dump_path if it is not NULL. Returns the number of observations or -1 with the
// message in err.
static long colmap_dump(const char *dir, const char *ext, const char *dump_path, char *err, long err_cap,
                        bool distorted_ok) {
    ColmapModel m;
    PrepArrays a;
    std::string e;
    if (!read_colmap_model(dir, ext, m, e, distorted_ok) || !colmap_prep_arrays(m, a, e)) {
        put_err(e, err, err_cap);
        return -1;
    }
    if (dump_path) {
        FILE *f = fopen(dump_path, "w");
        if (!f) { put_err("cannot write the dump", err, err_cap); return -1; }
        for (const ColmapCamera &c : m.cameras) {
            fprintf(f, "camera %u %s %llu %llu", c.id, c.model.c_str(), (unsigned long long)c.width,
                    (unsigned long long)c.height);
            for (double p : c.params) fprintf(f, " %a", p);
            fprintf(f, "\n");
        }
        for (size_t i = 0; i < m.images.size(); ++i) {
            const ColmapImage &im = m.images[i];
            fprintf(f, "image %u %a %a %a %a %a %a %a %u %s", im.id, im.q[0], im.q[1], im.q[2], im.q[3], im.t[0], im.t[1],
                    im.t[2], im.camera_id, im.name.c_str());
            for (size_t k = 0; k < im.point_ids.size(); ++k)
                fprintf(f, " %a %a %lld", im.xy[2 * k], im.xy[2 * k + 1], (long long)im.point_ids[k]);
            fprintf(f, "\nprep");
            for (int k = 0; k < 9; ++k) fprintf(f, " %a", a.rot[9 * i + (size_t)k]);
            for (int k = 0; k < 3; ++k) fprintf(f, " %a", a.centres[3 * i + (size_t)k]);
            for (int64_t j = a.obs_offset[i]; j < a.obs_offset[i + 1]; ++j) fprintf(f, " %d", a.obs_point[(size_t)j]);
            fprintf(f, "\n");
        }
        for (size_t k = 0; k < m.point_ids.size(); ++k)
            fprintf(f, "point %lld %a %a %a\n", (long long)m.point_ids[k], m.xyz[3 * k], m.xyz[3 * k + 1], m.xyz[3 * k + 2]);
        if (fclose(f) != 0) { put_err("cannot write the dump", err, err_cap); return -1; }
    }
    return (long)a.obs_point.size();
}
long apdhost_colmap_dump(const char *dir, const char *ext, const char *dump_path, char *err, long err_cap) {
    return colmap_dump(dir, ext, dump_path, err, err_cap, false);
}
// the same with the distorted camera models read too (apd_prepare --undistort; tests/test_undistort_host.py)
long apdhost_colmap_dump_distorted(const char *dir, const char *ext, const char *dump_path, char *err, long err_cap) {
    return colmap_dump(dir, ext, dump_path, err, err_cap, true);
}
int apdhost_write_cam_txt(const char *path, const double *R, const double *t, const double *K, double depth_min,
                          double interval, double depth_num, double depth_max) {
    return write_cam_txt(path, R, t, K, depth_min, interval, depth_num, depth_max) ? 0 : -1;
}
// pair.txt of the sequential window (n images, +-k)
int apdhost_write_pair_sequential(const char *path, int n, int k) {
    if (n < 0 || k < 0) return -1;
    return write_pair_txt(path, select_sequential(n, k)) ? 0 : -1;
}
// pair.txt of the scored selection from n x n shared / narrow counts
int apdhost_write_pair_scored(const char *path, int n, const unsigned *shared, const unsigned *narrow, int max_views) {
    if (n < 0 || !shared || !narrow) return -1;
    return write_pair_txt(path, select_scored(n, shared, narrow, max_views)) ? 0 : -1;
}
// read_pair_file: the number of problems, or -1 with the message in err. flat (if cap ints suffice):
// per problem ref, number of sources, the sources.
long apdhost_read_pair_file(const char *dense, int *flat, long cap, char *err, long err_cap) {
    std::vector<Problem> problems;
    std::string e;
    if (!read_pair_file(dense, problems, e)) { put_err(e, err, err_cap); return -1; }
    std::vector<int> out;
    for (const Problem &p : problems) {
        out.push_back(p.ref_image_id);
        out.push_back((int)p.src_image_ids.size());
        out.insert(out.end(), p.src_image_ids.begin(), p.src_image_ids.end());
    }
    if (flat && cap >= (long)out.size() && !out.empty()) memcpy(flat, out.data(), out.size() * sizeof(int));
    return (long)problems.size();
}
int apdhost_write_png_bgr8(const char *path, const unsigned char *bgr, int w, int h) {
    return write_png_bgr8(path, bgr, w, h) ? 0 : -1;
}
// names: image names joined by '\n'. out_names likewise (if the capacity suffices). Returns the number
// of images copied byte for byte, or -1 with the message in err.
long apdhost_convert_scan_images(const char *image_dir, const char *names, double scale, const char *out_dir,
                                 char *out_names, long out_cap, int *out_w, int *out_h, char *err, long err_cap) {
    std::vector<std::string> in, out;
    std::string cur, e;
    for (const char *p = names; *p; ++p) {
        if (*p == '\n') { in.push_back(cur); cur.clear(); } else cur += *p;
    }
    if (!cur.empty()) in.push_back(cur);
    std::vector<int> w, h;
    int copied = 0;
    if (!scan_image_sizes(image_dir, in, w, h, e) ||
        !convert_scan_images(image_dir, in, w, h, scale, out_dir, out, *out_w, *out_h, copied, e)) {
        put_err(e, err, err_cap);
        return -1;
    }
    std::string joined;
    for (size_t i = 0; i < out.size(); ++i) joined += (i ? "\n" : "") + out[i];
    if (out_names && out_cap > (long)joined.size()) memcpy(out_names, joined.c_str(), joined.size() + 1);
    return copied;
}
}
