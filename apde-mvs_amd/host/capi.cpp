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
}
