// io.cpp — bin-mat / cam.txt / pair.txt I/O of the `apd` driver (see io.h for the reference lines).
#include "io.h"

#include <map>
#include <mutex>

#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>

#include "image.h"

namespace apdhost {

int cv_elem_size(int type) {
    switch (type) {
        case CV_8UC1: return 1;
        case CV_32SC1: return 4;
        case CV_32FC1: return 4;
        case CV_32FC3: return 12;
        default: return 0;
    }
}

namespace {
struct BufferPool {
    std::mutex mu;
    std::multimap<size_t, uint8_t *> free_;
    size_t pooled = 0;
    static constexpr size_t kCap = (size_t)8 << 30;   // bytes kept for reuse
    static constexpr size_t kMin = (size_t)1 << 20;   // smaller buffers use plain new/delete
    uint8_t *take(size_t n) {
        std::lock_guard<std::mutex> g(mu);
        auto it = free_.find(n);
        if (it == free_.end()) return nullptr;
        uint8_t *p = it->second;
        free_.erase(it);
        pooled -= n;
        return p;
    }
    void give(uint8_t *p, size_t n) {
        {
            std::lock_guard<std::mutex> g(mu);
            if (pooled + n <= kCap) {
                free_.emplace(n, p);
                pooled += n;
                return;
            }
        }
        delete[] p;
    }
};
BufferPool &pool() {
    static BufferPool *p = new BufferPool();  // never destroyed: buffers may be released at exit
    return *p;
}
}  // namespace

std::shared_ptr<uint8_t[]> pool_buffer(size_t bytes) {
    if (bytes < BufferPool::kMin) return std::shared_ptr<uint8_t[]>(new uint8_t[bytes]);
    uint8_t *p = pool().take(bytes);
    if (!p) p = new uint8_t[bytes];
    return std::shared_ptr<uint8_t[]>(p, [bytes](uint8_t *q) { pool().give(q, bytes); });
}

Mat resize_nearest(const Mat &m, int w, int h) {
    Mat o(h, w, m.type);
    resize_nearest(m.bytes(), m.cols, m.rows, o.bytes(), w, h, cv_elem_size(m.type));
    return o;
}

bool read_binmat_file(const std::string &path, Mat &m) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    int32_t hdr[4];
    in.read(reinterpret_cast<char *>(hdr), sizeof(hdr));
    if (!in || hdr[0] != 1) return false;
    const int es = cv_elem_size(hdr[3]);
    if (es == 0 || hdr[1] < 0 || hdr[2] < 0) return false;
    // the payload must be in the file before a buffer of its size is allocated (a corrupt header
    // could otherwise ask for terabytes)
    const std::streampos here = in.tellg();
    in.seekg(0, std::ios::end);
    const std::streamoff avail = in.tellg() - here;
    in.seekg(here);
    if (avail < 0 || (uint64_t)avail < (uint64_t)hdr[1] * (uint64_t)hdr[2] * (uint64_t)es) return false;
    Mat r(hdr[1], hdr[2], hdr[3]);
    in.read(reinterpret_cast<char *>(r.bytes()), (std::streamsize)r.size_bytes());
    if (!in) {  // truncated file: no Mat (a pooled buffer would expose another problem's bytes)
        m = Mat();
        return false;
    }
    m = r;
    return true;
}

bool write_binmat_file(const std::string &path, const Mat &m) {
    std::ofstream out(path, std::ios::binary);
    if (!out) return false;
    const int32_t hdr[4] = {1, m.rows, m.cols, m.type};
    out.write(reinterpret_cast<const char *>(hdr), sizeof(hdr));
    out.write(reinterpret_cast<const char *>(m.bytes()), (std::streamsize)m.size_bytes());
    return (bool)out;
}

bool MatStore::read(const std::string &path, Mat &m) {
    if (cache_) {
        std::lock_guard<std::mutex> g(mu_);
        auto it = mats_.find(path);
        if (it != mats_.end()) {
            m = it->second;
            return true;
        }
    }
    if (!read_binmat_file(path, m)) {
        std::cout << "Error opening file: \"" << path << "\"" << std::endl;
        return false;
    }
    if (cache_) {
        std::lock_guard<std::mutex> g(mu_);
        mats_.emplace(path, m);
    }
    return true;
}

bool MatStore::write(const std::string &path, const Mat &m, bool flush) {
    if (cache_) {
        std::lock_guard<std::mutex> g(mu_);
        mats_[path] = m;
    }
    if (cache_ && flush) {
        std::lock_guard<std::mutex> g(qmu_);
        if (!writer_.joinable()) writer_ = std::thread(&MatStore::writer_loop, this);
        queue_.emplace_back(path, m);
        ++inflight_;
        qcv_.notify_one();
        return true;
    }
    if (!cache_) {
        if (!write_binmat_file(path, m)) {
            std::cout << "Error opening file: \"" << path << "\"" << std::endl;
            ++failed_;
            return false;
        }
    }
    return true;
}

void MatStore::writer_loop() {
    std::unique_lock<std::mutex> l(qmu_);
    for (;;) {
        qcv_.wait(l, [&] { return stop_ || !queue_.empty(); });
        if (queue_.empty()) return;  // stop_ and drained
        auto job = std::move(queue_.front());
        queue_.pop_front();
        l.unlock();
        if (!write_binmat_file(job.first, job.second)) {
            std::cout << "Error opening file: \"" << job.first << "\"" << std::endl;
            ++failed_;
        }
        job.second = Mat();
        l.lock();
        if (--inflight_ == 0) qdone_.notify_all();
    }
}

void MatStore::drain() {
    std::unique_lock<std::mutex> l(qmu_);
    qdone_.wait(l, [&] { return inflight_ == 0; });
}

MatStore::~MatStore() {
    {
        std::lock_guard<std::mutex> g(qmu_);
        stop_ = true;
        qcv_.notify_all();
    }
    if (writer_.joinable()) writer_.join();
}

void MatStore::flush_all() {
    drain();
    std::lock_guard<std::mutex> g(mu_);
    for (auto &kv : mats_)
        if (!write_binmat_file(kv.first, kv.second)) {
            std::cout << "Error opening file: \"" << kv.first << "\"" << std::endl;
            ++failed_;
        }
    mats_.clear();
}

bool read_camera(const std::string &path, apd_camera &cam) {
    std::ifstream in(path);
    if (!in) return false;
    memset(&cam, 0, sizeof(cam));
    std::string tok;
    in >> tok;  // "extrinsic"
    for (int i = 0; i < 3; ++i) in >> cam.R[3 * i + 0] >> cam.R[3 * i + 1] >> cam.R[3 * i + 2] >> cam.t[i];
    float tmp[4];
    in >> tmp[0] >> tmp[1] >> tmp[2] >> tmp[3];
    in >> tok;  // "intrinsic"
    for (int i = 0; i < 3; ++i) in >> cam.K[3 * i + 0] >> cam.K[3 * i + 1] >> cam.K[3 * i + 2];
    for (int j = 0; j < 3; ++j)
        cam.c[j] = -(float)((double)cam.R[0 + j] * (double)cam.t[0] + (double)cam.R[3 + j] * (double)cam.t[1] +
                            (double)cam.R[6 + j] * (double)cam.t[2]);
    in >> cam.depth_min >> cam.interval;
    if (!(in >> cam.depth_num >> cam.depth_max)) {
        cam.depth_num = 192;
        cam.depth_max = cam.interval * cam.depth_num + cam.depth_min;
    }
    return true;
}

namespace {
int ply_type_size(const std::string &t) {
    static const std::map<std::string, int> sizes = {
        {"char", 1},  {"uchar", 1},  {"int8", 1},  {"uint8", 1},   {"short", 2},  {"ushort", 2},
        {"int16", 2}, {"uint16", 2}, {"int", 4},   {"uint", 4},    {"int32", 4},  {"uint32", 4},
        {"float", 4}, {"float32", 4}, {"double", 8}, {"float64", 8}};
    auto it = sizes.find(t);
    return it == sizes.end() ? 0 : it->second;
}
}  // namespace

bool read_ply_xyz(const std::string &path, std::vector<float> &xyz, std::string &err) {
    xyz.clear();
    std::ifstream in(path, std::ios::binary);
    if (!in) { err = "cannot open " + path; return false; }
    auto fail = [&](const std::string &what) { err = path + ": " + what; return false; };
    std::string line;
    auto next_line = [&]() {
        if (!std::getline(in, line) || line.size() > 4096) return false;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        return true;
    };
    if (!next_line() || line != "ply") return fail("not a PLY file");
    bool have_format = false, in_vertex = false, seen_vertex = false, ended = false;
    uint64_t count = 0;
    size_t stride = 0;
    long off[3] = {-1, -1, -1};
    for (int lines = 0; lines < 100000 && next_line(); ++lines) {
        std::istringstream ls(line);
        std::string kw;
        ls >> kw;
        if (kw == "end_header") { ended = true; break; }
        if (kw.empty() || kw == "comment" || kw == "obj_info") continue;
        if (kw == "format") {
            std::string fmt, ver;
            ls >> fmt >> ver;
            if (fmt != "binary_little_endian" || ver != "1.0")
                return fail("unsupported format '" + fmt + " " + ver + "' (binary_little_endian 1.0 only)");
            have_format = true;
        } else if (kw == "element") {
            std::string name;
            std::string num;
            ls >> name >> num;
            in_vertex = false;
            if (name == "vertex") {
                if (seen_vertex) return fail("more than one vertex element");
                if (num.empty() || num.size() > 18 || num.find_first_not_of("0123456789") != std::string::npos)
                    return fail("bad vertex count");
                count = std::stoull(num);
                seen_vertex = in_vertex = true;
            } else if (!seen_vertex) {
                return fail("element '" + name + "' in front of vertex");
            }
        } else if (kw == "property") {
            if (!in_vertex) {
                if (!seen_vertex) return fail("property outside an element");
                continue;  // a later element's: ignored
            }
            std::string type, name;
            ls >> type >> name;
            if (type == "list") return fail("list property on vertex");
            const int sz = ply_type_size(type);
            if (sz == 0 || name.empty()) return fail("unknown property type '" + type + "'");
            for (int a = 0; a < 3; ++a)
                if (name == std::string(1, "xyz"[a])) {
                    if (sz != 4 || (type != "float" && type != "float32")) return fail(name + " is not float");
                    if (off[a] >= 0) return fail("duplicate property " + name);
                    off[a] = (long)stride;
                }
            stride += (size_t)sz;
            if (stride > 65536) return fail("vertex record too large");
        } else {
            return fail("unexpected header line '" + kw + "'");
        }
    }
    if (!ended) return fail("header has no end_header");
    if (!have_format) return fail("header has no format line");
    if (!seen_vertex) return fail("no vertex element");
    for (int a = 0; a < 3; ++a)
        if (off[a] < 0) return fail(std::string("vertex has no property ") + "xyz"[a]);
    // the body must be in the file before anything of its size is allocated
    const std::streampos here = in.tellg();
    in.seekg(0, std::ios::end);
    const std::streamoff avail = in.tellg() - here;
    in.seekg(here);
    if (here < 0 || avail < 0 || count > (uint64_t)avail / stride) return fail("vertex count exceeds the file's size");
    if (count > (uint64_t)INT32_MAX) return fail("more than 2^31-1 vertices");
    xyz.resize((size_t)count * 3);
    const size_t chunk = std::max<size_t>(1, ((size_t)4 << 20) / stride);
    std::vector<char> buf(chunk * stride);
    for (size_t done = 0; done < count;) {
        const size_t m = std::min<size_t>(chunk, (size_t)count - done);
        in.read(buf.data(), (std::streamsize)(m * stride));
        if (!in) { xyz.clear(); return fail("truncated body"); }
        for (size_t i = 0; i < m; ++i)
            for (int a = 0; a < 3; ++a) memcpy(&xyz[3 * (done + i) + a], &buf[i * stride + (size_t)off[a]], 4);
        done += m;
    }
    return true;
}

bool write_ply_xyz_rgb(const std::string &path, const std::vector<float> &xyz, const std::vector<uint8_t> &rgb) {
    if (xyz.size() % 3 != 0 || rgb.size() != xyz.size()) return false;
    std::ofstream out(path, std::ios::binary);
    if (!out) return false;
    const size_t n = xyz.size() / 3;
    out << "ply\nformat binary_little_endian 1.0\nelement vertex " << n
        << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
           "property uchar blue\nend_header\n";
    const size_t chunk = 1 << 16;
    std::vector<char> buf(chunk * 15);
    for (size_t done = 0; done < n;) {
        const size_t m = std::min(chunk, n - done);
        for (size_t i = 0; i < m; ++i) {
            memcpy(&buf[i * 15], &xyz[3 * (done + i)], 12);
            memcpy(&buf[i * 15 + 12], &rgb[3 * (done + i)], 3);
        }
        out.write(buf.data(), (std::streamsize)(m * 15));
        done += m;
    }
    out.flush();
    return (bool)out;
}

bool read_mlp(const std::string &path, std::vector<MlpMesh> &meshes, std::string &err) {
    meshes.clear();
    std::ifstream in(path, std::ios::binary);
    if (!in) { err = "cannot open " + path; return false; }
    auto fail = [&](const std::string &what) { err = path + ": " + what; meshes.clear(); return false; };
    std::string text;
    for (char buf[1 << 16]; in.read(buf, sizeof buf) || in.gcount() > 0;) {  // a directory opens but does not read
        text.append(buf, (size_t)in.gcount());
        if (text.size() > ((size_t)64 << 20)) return fail("project file larger than 64 MiB");
    }
    if (in.bad()) return fail("read error");
    const size_t slash = path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string(".") : path.substr(0, slash);
    // the next "<MLMesh" that is a whole tag name, from `from` on
    auto next_mesh = [&](size_t from) {
        for (size_t p; (p = text.find("<MLMesh", from)) != std::string::npos; from = p + 1) {
            const size_t e = p + 7;
            if (e >= text.size() || text[e] == '>' || text[e] == '/' || std::isspace((unsigned char)text[e])) return p;
        }
        return std::string::npos;
    };
    for (size_t p = next_mesh(0); p != std::string::npos;) {
        const std::string which = "mesh " + std::to_string(meshes.size() + 1);
        const size_t tag_end = text.find('>', p);
        if (tag_end == std::string::npos) return fail(which + ": unterminated <MLMesh tag");
        const size_t next = next_mesh(tag_end);
        const size_t body_end = next == std::string::npos ? text.size() : next;
        MlpMesh m;
        {  // the attribute filename="F" of the tag
            const std::string tag = text.substr(p, tag_end - p);
            size_t a = std::string::npos;
            for (size_t q = 0; (q = tag.find("filename=\"", q)) != std::string::npos; ++q)
                if (q > 0 && std::isspace((unsigned char)tag[q - 1])) { a = q + 10; break; }
            const size_t b = a == std::string::npos ? a : tag.find('"', a);
            if (b == std::string::npos || b == a) return fail(which + ": no filename attribute");
            const std::string f = tag.substr(a, b - a);
            m.ply_path = f[0] == '/' ? f : dir + "/" + f;
        }
        const size_t ms = text.find("<MLMatrix44>", tag_end);
        if (ms == std::string::npos || ms >= body_end) return fail(which + " (" + m.ply_path + ") has no <MLMatrix44>");
        const size_t me = text.find("</MLMatrix44>", ms);
        if (me == std::string::npos || me > body_end) return fail(which + ": unterminated <MLMatrix44>");
        std::istringstream nums(text.substr(ms + 12, me - ms - 12));
        std::string tok;
        int k = 0;
        while (nums >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (!end || *end != '\0' || end == tok.c_str() || !std::isfinite(v))
                return fail(which + ": '" + tok.substr(0, 32) + "' in the matrix is not a number");
            if (k >= 16) return fail(which + ": more than 16 numbers in the matrix");
            m.M[k++] = v;
        }
        if (k < 16) return fail(which + ": " + std::to_string(k) + " numbers in the matrix, 16 expected");
        if (m.M[12] != 0.0 || m.M[13] != 0.0 || m.M[14] != 0.0 || m.M[15] != 1.0)
            return fail(which + ": the last row of the matrix is not 0 0 0 1");
        meshes.push_back(m);
        p = next;
    }
    if (meshes.empty()) return fail("no <MLMesh> in the project");
    return true;
}

void mlp_to_world(const MlpMesh &m, std::vector<float> &xyz, float origin[3]) {
    const double *M = m.M;
    for (size_t i = 0; i + 2 < xyz.size(); i += 3) {
        const double x = xyz[i], y = xyz[i + 1], z = xyz[i + 2];
        for (int r = 0; r < 3; ++r)  // in double, rounded once
            xyz[i + r] = (float)(M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3]);
    }
    for (int r = 0; r < 3; ++r) origin[r] = (float)M[4 * r + 3];
}

std::string format_index(int id) {
    std::ostringstream ss;
    ss << std::setw(8) << std::setfill('0') << id;
    return ss.str();
}

bool file_exists(const std::string &p) {
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}

bool make_dir(const std::string &p) { return mkdir(p.c_str(), 0755) == 0 || file_exists(p); }

bool read_pair_file(const std::string &dense, std::vector<Problem> &problems, std::string &err) {
    std::ifstream file(dense + "/pair.txt");
    if (!file) { err = "cannot open " + dense + "/pair.txt"; return false; }
    static const char *exts[] = {".jpg", ".png", ".jpeg", ".JPG", ".PNG", ".JPEG"};
    std::string line;
    std::getline(file, line);
    int num_images = 0;
    std::istringstream(line) >> num_images;
    problems.clear();
    for (int i = 0; i < num_images; ++i) {
        Problem p;
        std::getline(file, line);
        std::istringstream(line) >> p.ref_image_id;
        std::getline(file, line);
        std::istringstream iss(line);
        int n = 0;
        iss >> n;
        for (int j = 0; j < n; ++j) {
            int id;
            float score;
            iss >> id >> score;
            if (score <= 0.0f) continue;
            p.src_image_ids.push_back(id);
        }
        for (const char *e : exts) {
            if (file_exists(dense + "/images/" + format_index(p.ref_image_id) + e)) {
                p.img_ext = e;
                break;
            }
        }
        if (p.img_ext.empty()) {
            err = "can not find image: " + format_index(p.ref_image_id);
            return false;
        }
        problems.push_back(p);
    }
    return true;
}

}  // namespace apdhost
