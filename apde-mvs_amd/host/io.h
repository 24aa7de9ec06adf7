// io.h — on-disk contract of the reference's depth binary, restated without OpenCV/Boost:
// bin-mat files (APD.cpp:18-83), MVSNet cam.txt (APD.cpp:85-135), pair.txt (main.cpp:44-102),
// and the MemoryCache write-back semantics (APD.cpp:3-16, main.cpp:381-393).
#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include <condition_variable>
#include <deque>
#include <thread>
#include <atomic>

#include "../../include/apd_hip.h"

namespace apdhost {

// OpenCV type codes used by the reference's bin-mat files
enum { CV_8UC1 = 0, CV_32SC1 = 4, CV_32FC1 = 5, CV_32FC3 = 21 };
int cv_elem_size(int type);

// Pixels are reference-counted like a cv::Mat's: copying a Mat (MemoryCache reads and writes,
// priors) shares the buffer instead of copying hundreds of MB per problem. Every writer fills a
// freshly constructed Mat, so sharing never exposes a partial write. Like cv::Mat::create, the
// buffer is not zero-filled (every writer fills all of it; a 3024x2016 problem's four result Mats
// would otherwise cost ~100 MB of memset).
// Large host buffers come from a process-wide pool: a released buffer is kept (up to a byte cap)
// and handed to the next request of the same size, so the per-problem result Mats and staging
// buffers of a scan reuse resident pages instead of faulting in (and zeroing) fresh ones.
std::shared_ptr<uint8_t[]> pool_buffer(size_t bytes);
struct Mat {
    int rows = 0, cols = 0, type = CV_8UC1;
    size_t nbytes = 0;
    std::shared_ptr<uint8_t[]> buf;  // row-major, rows * cols * elem bytes
    Mat() = default;
    Mat(int r, int c, int t)
        : rows(r), cols(c), type(t), nbytes((size_t)r * c * cv_elem_size(t)), buf(pool_buffer(nbytes)) {}
    uint8_t *bytes() { return buf.get(); }
    const uint8_t *bytes() const { return buf.get(); }
    size_t size_bytes() const { return buf ? nbytes : 0; }
    template <class T> T *ptr() { return reinterpret_cast<T *>(bytes()); }
    template <class T> const T *ptr() const { return reinterpret_cast<const T *>(bytes()); }
    bool empty() const { return rows == 0 || cols == 0; }
};
Mat resize_nearest(const Mat &m, int w, int h);

// MemoryCache (APD.cpp:3-16): when enabled, bin-mat writes land in memory and reach the disk only
// when flushed; reads check the cache first. Thread-safe.
// With the cache on, a flushed write (--flush / --no_fuse) only persists a Mat that every read is
// served from memory anyway, so the file is written by a background thread (in submission order;
// drained by flush_all and the destructor) instead of on the problem's critical path. Without the
// cache, reads come from the files and writes stay synchronous.
class MatStore {
public:
    explicit MatStore(bool cache) : cache_(cache) {}
    ~MatStore();
    bool read(const std::string &path, Mat &m);                    // ReadBinMat   APD.cpp:18-56
    bool write(const std::string &path, const Mat &m, bool flush);  // WriteBinMat  APD.cpp:58-83
    void flush_all();                                              // main.cpp:381-393
    void drain();                                                  // wait for queued file writes
    bool cached() const { return cache_; }
    // result files that could not be written so far (synchronous, queued and flushed writes alike);
    // the caller waits with drain() before reading it, and main() exits non-zero when it is not 0
    size_t failed_writes() const { return failed_.load(); }

private:
    void writer_loop();
    bool cache_;
    std::mutex mu_;
    std::map<std::string, Mat> mats_;
    std::mutex qmu_;
    std::condition_variable qcv_, qdone_;
    std::deque<std::pair<std::string, Mat>> queue_;
    size_t inflight_ = 0;
    bool stop_ = false;
    std::atomic<size_t> failed_{0};
    std::thread writer_;
};

bool read_binmat_file(const std::string &path, Mat &m);
bool write_binmat_file(const std::string &path, const Mat &m);

// ReadCamera (APD.cpp:85-135): extrinsic 4x4 (last row ignored), intrinsic 3x3, depth_min interval
// [depth_num depth_max] with the depth_num = 192 fallback; centre c = -R^T t in double.
bool read_camera(const std::string &path, apd_camera &cam);

struct Problem {  // main.h:102-115
    int ref_image_id = 0;
    std::vector<int> src_image_ids;
    std::string img_ext;
};
// GenerateSampleList (main.cpp:44-102): sources with score <= 0 are dropped; the image extension
// is the first of .jpg .png .jpeg .JPG .PNG .JPEG present for the reference image.
bool read_pair_file(const std::string &dense_folder, std::vector<Problem> &problems, std::string &err);

// Vertex positions of a binary_little_endian 1.0 PLY (APD.ply's 12- and 15-byte records among
// others): one `vertex` element with scalar properties of any standard type in any order, of which
// x, y and z must be `float`; the other properties are skipped by size, `comment` and `obj_info`
// lines are accepted and elements after `vertex` are ignored. Rejected with a message in `err`,
// before anything is allocated from the header's count: ascii and big-endian files, a list
// property on `vertex`, an element in front of `vertex`, a missing coordinate, and a vertex count
// the file does not hold.
bool read_ply_xyz(const std::string &path, std::vector<float> &xyz, std::string &err);

// binary_little_endian PLY of 15-byte records float x, y, z + uchar red, green, blue (rgb: three
// bytes per point); read_ply_xyz reads it back
bool write_ply_xyz_rgb(const std::string &path, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb);

// One scanner position of a MeshLab project (.mlp): the PLY of its points and its pose.
struct MlpMesh {
    std::string ply_path;  // as given if absolute, else relative to the project file's directory
    double M[16];          // <MLMatrix44>, row-major: mesh coordinates -> world
};
// Every <MLMesh ... filename="F" ...> with its <MLMatrix44> of 16 numbers separated by white space
// (line breaks included). No XML library: the tags are scanned for. Rejected with a message in
// `err`: an unreadable file, no mesh, a mesh without filename or matrix, fewer or more than 16
// numbers, a token that is not a finite number, a last row other than 0 0 0 1.
bool read_mlp(const std::string &path, std::vector<MlpMesh> &meshes, std::string &err);
// xyz (mesh coordinates, from read_ply_xyz) -> world: M (x, y, z, 1) evaluated in double left to
// right and rounded once to float. origin = the translation column rounded to float: the scanner.
void mlp_to_world(const MlpMesh &m, std::vector<float> &xyz, float origin[3]);

// ---- Tanks and Temples ground-truth side files (apd_eval --tat_gt) ------------------------------------
// The crop volume <Scene>.json (Open3D's SelectionPolygonVolume): a JSON object of which only the keys
// axis_max, axis_min (numbers), orthogonal_axis ("X", "Y" or "Z") and bounding_polygon (an array of
// 3 to 2^20 arrays of exactly three numbers) are taken; every other key is parsed and ignored.
struct TatCrop {
    int axis = 0;  // 0, 1, 2 for X, Y, Z
    double axis_min = 0.0, axis_max = 0.0;
    std::vector<double> vertices;  // 3 per vertex, as in the file
    // the (u, v) pairs of include/apd_eval.h's crop rule: coordinates (1, 2), (0, 2), (0, 1) for X, Y, Z
    std::vector<double> polygon() const;
};
// A minimal strict JSON parser (RFC 8259 syntax, no extensions): files over 64 MiB, nesting deeper than
// 64, a missing or repeated wanted key, a wrong type, a number outside the double range, a vertex count
// outside 3..2^20 and anything after the closing brace are rejected with a message in `err`.
bool read_tat_crop(const std::string &path, TatCrop &crop, std::string &err);
// A 4x4 matrix as 16 numbers separated by white space (<Scene>_trans.txt), row-major. A number has the
// JSON grammar (-?digits[.digits][e[+-]digits], as in the crop file; read without regard to the locale).
// Rejected: files over 1 MiB, fewer or more than 16 tokens, a token that is no such number (hex floats,
// inf, nan, a leading '+' or '.') or lies outside the double range, a last row other than 0 0 0 1.
bool read_matrix4(const std::string &path, double M[16], std::string &err);

// ---- DTU ground-truth side files (apd_eval --dtu_gt): Level-5 MAT-files ------------------------------
struct MatWanted {
    std::string name;
    bool as_mask = false;  // a logical or uint8 array, delivered as bytes (1 where non-zero)
};
struct MatArray {
    std::string name;
    std::vector<int64_t> dims;  // 1 to 3, each >= 0, as in the file
    bool logical = false;
    std::vector<double> values;  // column-major, every stored type converted to double (not as_mask)
    std::vector<uint8_t> bytes;  // as_mask
};
constexpr uint64_t kMatMaxFile = (uint64_t)1 << 31;                    // bytes of a file
constexpr uint64_t kMatMaxInflated = ((uint64_t)1 << 31) + (1 << 16);  // bytes of one inflated element
constexpr uint64_t kMatMaxElems = (uint64_t)1 << 31;                   // elements of one array
// The wanted variables of a little-endian Level-5 MAT-file (128-byte header, version 0x0100, endian
// indicator "IM"), in the order of `wanted`. Top-level elements are miMATRIX, or miCOMPRESSED (zlib)
// holding one miMATRIX; per matrix: array flags, 1 to 3 dimensions, name, real part, with the small
// tag form and the 8-byte padding. Classes double, single and int8..uint64 (with the logical flag);
// stored data type any of miINT8..miUINT64, miSINGLE, miDOUBLE (MATLAB narrows integral doubles).
// Variables not asked for are skipped whatever their class, a compressed one after its first 64 KiB.
// Rejected with a message naming the file (and the variable): a wanted name that is missing, occurs
// twice, is complex, sparse, a cell, struct, object or char array or has more than 3 dimensions; a
// "MATLAB 7.3" (HDF5) file, with the advice to re-save with -v7; a big-endian file ("MI"); any tag or
// byte count that overruns its parent or the file; more than kMatMaxElems elements; a file above
// kMatMaxFile; a compressed element that declares or inflates to more than kMatMaxInflated or past its
// own declared size. Nothing is allocated before the bytes that justify it are known to be in the
// file: inflation is incremental and its output at most doubles per step.
bool read_mat5(const std::string &path, const std::vector<MatWanted> &wanted, std::vector<MatArray> &out,
               std::string &err);

// ---- COLMAP sparse models (apd_prepare; the reference's tools/colmap2mvsnet.py) ---------------------
struct ColmapCamera {
    uint32_t id = 0;
    std::string model;  // SIMPLE_PINHOLE or PINHOLE; with distorted_ok any of include/apd_prep.h's models
    uint64_t width = 0, height = 0;
    std::vector<double> params;  // the model's own count and order: f cx cy | fx fy cx cy | f cx cy k | ...
};
struct ColmapImage {
    uint32_t id = 0, camera_id = 0;
    double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
    std::string name;
    std::vector<double> xy;          // 2 per 2D point
    std::vector<int64_t> point_ids;  // -1: no 3D point
};
struct ColmapModel {
    std::vector<ColmapCamera> cameras;
    std::vector<ColmapImage> images;  // ascending id: index = the new image number
    std::vector<int64_t> point_ids;   // in file order
    std::vector<double> xyz;          // 3 per point
};
// cameras, images and points3D of `dir` with extension ".txt" or ".bin". Only SIMPLE_PINHOLE and
// PINHOLE cameras are accepted, as in the reference. Every count is bounded by the file's size before
// anything is allocated; truncated or garbled files, non-numeric tokens, non-finite numbers, duplicate
// ids and an image whose camera is missing are rejected with a message in `err`.
// With distorted_ok (apd_prepare --undistort) the eight distorted models of include/apd_prep.h are
// read too, each with its own parameter count; FOV and unknown models are rejected either way.
bool read_colmap_model(const std::string &dir, const std::string &ext, ColmapModel &m, std::string &err,
                       bool distorted_ok = false);
// COLMAP's id of a model name that include/apd_prep.h supports (0..6, 8..10), else -1
int colmap_model_id(const std::string &model);

// The arrays of apd_prep_set_model (include/apd_prep.h): R by the contract's qvec formula, centres,
// and the observations as indices into the point array, grouped by image. A point id an image names
// that points3D lacks is an error.
struct PrepArrays {
    std::vector<double> rot, trans, centres;
    std::vector<int64_t> obs_offset;
    std::vector<int32_t> obs_point;
};
bool colmap_prep_arrays(const ColmapModel &m, PrepArrays &a, std::string &err);

typedef std::vector<std::vector<std::pair<int, int>>> ViewSelection;  // per view: (source, score)
// tools/colmap2mvsnet.py:453-468
ViewSelection select_sequential(int n, int k);
// score = shared, 0 where narrow >= floor(3*shared/4) + 1; per view the first min(max_views, n-1) of
// j != i by (score descending, j ascending), zero scores included
ViewSelection select_scored(int n, const uint32_t *shared, const uint32_t *narrow, int max_views);

// shortest decimal that parses back to the same double
std::string shortest_double(double v);
// cam.txt in the reference's layout (:495-507): extrinsic 4x4, intrinsic 3x3 (shortest round-trip
// decimals), then "%f %f %f %f" of depth_min, interval, depth_num, depth_max
bool write_cam_txt(const std::string &path, const double R[9], const double t[3], const double K[9],
                   double depth_min, double interval, double depth_num, double depth_max);
bool write_pair_txt(const std::string &path, const ViewSelection &sel);  // :508-514
bool write_colmap_cameras_txt(const std::string &path, const std::vector<ColmapCamera> &cams);
bool write_colmap_images_txt(const std::string &path, const std::vector<ColmapImage> &images);
bool copy_file(const std::string &from, const std::string &to);
// The images of a scan (:516-536). scan_image_sizes decodes every image_dir/name for its size.
// convert_scan_images writes out_dir/%08d<ext>: with scale == 1 and an image of the largest size, a
// source named .jpg/.jpeg/.png (any case) is copied byte for byte under its lower-cased extension;
// otherwise it is decoded, padded bottom and right with zeros to the largest size, resized to
// (int(W/scale), int(H/scale)) by resize_nearest and written as 8-bit colour PNG (there is no JPEG
// encoder here: lossless, where the reference recompresses). Files %08d.{jpg,jpeg,png} of another
// extension left by an earlier run are removed, so every index has one image.
// With `warp`, an image i with warp->mask[i] is never copied: it is decoded, handed to warp->apply
// (which replaces its pixels and keeps its size; false with a message in `err` fails the call) and
// then padded, resized and written as PNG like any other decoded image.
struct Bgr8;  // image.h
struct ScanImageWarp {
    std::vector<char> mask;  // one entry per image
    std::function<bool(size_t, Bgr8 &, std::string &)> apply;
};
bool scan_image_sizes(const std::string &image_dir, const std::vector<std::string> &names, std::vector<int> &widths,
                      std::vector<int> &heights, std::string &err);
bool convert_scan_images(const std::string &image_dir, const std::vector<std::string> &names,
                         const std::vector<int> &widths, const std::vector<int> &heights, double scale,
                         const std::string &out_dir, std::vector<std::string> &out_names, int &out_w, int &out_h,
                         int &copied, std::string &err, const ScanImageWarp *warp = nullptr);

std::string format_index(int id);  // ToFormatIndex: %08d
bool file_exists(const std::string &p);
bool make_dir(const std::string &p);

}  // namespace apdhost
