// io.cpp — bin-mat / cam.txt / pair.txt I/O of the `apd` driver (see io.h for the reference lines).
#include "io.h"

#include <map>
#include <mutex>

#include <sys/stat.h>
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <charconv>
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

// ----------------------------------------------------------------------------------------------
// Tanks and Temples side files
// ----------------------------------------------------------------------------------------------
namespace {

bool read_text_bounded(const std::string &path, size_t cap, const char *cap_name, std::string &text, std::string &err) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { err = "cannot open " + path; return false; }
    text.clear();
    for (char buf[1 << 16]; in.read(buf, sizeof buf) || in.gcount() > 0;) {  // a directory opens but does not read
        text.append(buf, (size_t)in.gcount());
        if (text.size() > cap) { err = path + ": larger than " + cap_name; return false; }
    }
    if (in.bad()) { err = path + ": read error"; return false; }
    return true;
}

// Recursive-descent JSON over a string; values outside the wanted keys are validated and dropped.
struct JsonCursor {
    const std::string &s;
    size_t p = 0;
    std::string err;
    explicit JsonCursor(const std::string &text) : s(text) {}
    static constexpr int kMaxDepth = 64;

    bool fail(const std::string &what) {
        if (err.empty()) err = what + " at byte " + std::to_string(p);
        return false;
    }
    void ws() {
        while (p < s.size() && (s[p] == ' ' || s[p] == '\t' || s[p] == '\n' || s[p] == '\r')) ++p;
    }
    bool lit(const char *word) {
        const size_t n = std::strlen(word);
        if (s.compare(p, n, word) != 0) return fail("unexpected token");
        p += n;
        return true;
    }
    bool string(std::string &out) {
        if (p >= s.size() || s[p] != '"') return fail("expected a string");
        ++p;
        out.clear();
        while (p < s.size()) {
            const unsigned char c = (unsigned char)s[p];
            if (c == '"') { ++p; return true; }
            if (c < 0x20) return fail("control character in a string");
            if (c == '\\') {
                if (p + 1 >= s.size()) break;
                const char e = s[p + 1];
                if (e == 'u') {
                    if (p + 6 > s.size()) break;
                    for (size_t k = p + 2; k < p + 6; ++k)
                        if (!std::isxdigit((unsigned char)s[k])) return fail("bad \\u escape");
                    out.push_back('?');  // no wanted string holds an escape: the code point is not needed
                    p += 6;
                    continue;
                }
                if (!std::strchr("\"\\/bfnrt", e) || e == '\0') return fail("bad escape");
                out.push_back(e);
                p += 2;
                continue;
            }
            if (out.size() < 4096) out.push_back((char)c);
            ++p;
        }
        return fail("unterminated string");
    }
    bool number(double &v) {
        const size_t b = p;
        if (p < s.size() && s[p] == '-') ++p;
        if (p >= s.size() || !std::isdigit((unsigned char)s[p])) return fail("expected a number");
        if (s[p] == '0') ++p;
        else while (p < s.size() && std::isdigit((unsigned char)s[p])) ++p;
        if (p < s.size() && s[p] == '.') {
            ++p;
            if (p >= s.size() || !std::isdigit((unsigned char)s[p])) return fail("digits expected after '.'");
            while (p < s.size() && std::isdigit((unsigned char)s[p])) ++p;
        }
        if (p < s.size() && (s[p] == 'e' || s[p] == 'E')) {
            ++p;
            if (p < s.size() && (s[p] == '+' || s[p] == '-')) ++p;
            if (p >= s.size() || !std::isdigit((unsigned char)s[p])) return fail("digits expected in the exponent");
            while (p < s.size() && std::isdigit((unsigned char)s[p])) ++p;
        }
        if (p - b > 400) return fail("number token longer than 400 characters");
        // std::from_chars: no locale, and a token of this grammar is all it accepts here
        const std::from_chars_result r = std::from_chars(s.data() + b, s.data() + p, v);
        if (r.ec != std::errc() || r.ptr != s.data() + p || !std::isfinite(v)) {
            p = b;
            return fail("number outside the double range");
        }
        return true;
    }
    // any value, validated and dropped
    bool skip(int depth) {
        if (depth > kMaxDepth) return fail("nesting deeper than 64");
        ws();
        if (p >= s.size()) return fail("unexpected end of file");
        const char c = s[p];
        std::string str;
        double v;
        if (c == '"') return string(str);
        if (c == 't') return lit("true");
        if (c == 'f') return lit("false");
        if (c == 'n') return lit("null");
        if (c == '[') {
            ++p;
            ws();
            if (p < s.size() && s[p] == ']') { ++p; return true; }
            for (;;) {
                if (!skip(depth + 1)) return false;
                ws();
                if (p < s.size() && s[p] == ',') { ++p; continue; }
                if (p < s.size() && s[p] == ']') { ++p; return true; }
                return fail("expected ',' or ']'");
            }
        }
        if (c == '{') {
            ++p;
            ws();
            if (p < s.size() && s[p] == '}') { ++p; return true; }
            for (;;) {
                ws();
                if (!string(str)) return false;
                ws();
                if (p >= s.size() || s[p] != ':') return fail("expected ':'");
                ++p;
                if (!skip(depth + 1)) return false;
                ws();
                if (p < s.size() && s[p] == ',') { ++p; continue; }
                if (p < s.size() && s[p] == '}') { ++p; return true; }
                return fail("expected ',' or '}'");
            }
        }
        return number(v);
    }
};

}  // namespace

std::vector<double> TatCrop::polygon() const {
    const int ui = axis == 0 ? 1 : 0, vi = axis == 2 ? 1 : 2;
    std::vector<double> uv;
    for (size_t i = 0; i + 2 < vertices.size(); i += 3) {
        uv.push_back(vertices[i + (size_t)ui]);
        uv.push_back(vertices[i + (size_t)vi]);
    }
    return uv;
}

bool read_tat_crop(const std::string &path, TatCrop &crop, std::string &err) {
    crop = TatCrop{};
    std::string text;
    if (!read_text_bounded(path, (size_t)64 << 20, "64 MiB", text, err)) return false;
    JsonCursor js(text);
    auto fail = [&](const std::string &what) {
        err = path + ": " + (js.err.empty() ? what : js.err);
        crop = TatCrop{};
        return false;
    };
    js.ws();
    if (js.p >= text.size() || text[js.p] != '{') return fail("not a JSON object");
    ++js.p;
    bool have_min = false, have_max = false, have_axis = false, have_poly = false;
    js.ws();
    if (js.p < text.size() && text[js.p] == '}') {
        ++js.p;
    } else {
        for (;;) {
            std::string key, sval;
            js.ws();
            if (!js.string(key)) return fail("");
            js.ws();
            if (js.p >= text.size() || text[js.p] != ':') return fail("expected ':' after a key");
            ++js.p;
            js.ws();
            if (key == "axis_min" || key == "axis_max") {
                bool &have = key == "axis_min" ? have_min : have_max;
                if (have) return fail("key " + key + " is repeated");
                if (!js.number(key == "axis_min" ? crop.axis_min : crop.axis_max)) return fail("");
                have = true;
            } else if (key == "orthogonal_axis") {
                if (have_axis) return fail("key orthogonal_axis is repeated");
                if (!js.string(sval)) return fail("");
                if (sval != "X" && sval != "Y" && sval != "Z") return fail("orthogonal_axis is not \"X\", \"Y\" or \"Z\"");
                crop.axis = sval[0] - 'X';
                have_axis = true;
            } else if (key == "bounding_polygon") {
                if (have_poly) return fail("key bounding_polygon is repeated");
                if (js.p >= text.size() || text[js.p] != '[') return fail("bounding_polygon is not an array");
                ++js.p;
                js.ws();
                if (js.p < text.size() && text[js.p] == ']') {
                    ++js.p;
                } else {
                    for (;;) {
                        js.ws();
                        if (js.p >= text.size() || text[js.p] != '[') return fail("a polygon vertex is not an array");
                        ++js.p;
                        if (crop.vertices.size() / 3 >= ((size_t)1 << 20)) return fail("more than 2^20 polygon vertices");
                        for (int k = 0; k < 3; ++k) {
                            double v;
                            js.ws();
                            if (!js.number(v)) return fail("");
                            crop.vertices.push_back(v);
                            js.ws();
                            if (js.p >= text.size() || text[js.p] != (k < 2 ? ',' : ']'))
                                return fail("a polygon vertex does not have exactly three numbers");
                            ++js.p;
                        }
                        js.ws();
                        if (js.p < text.size() && text[js.p] == ',') { ++js.p; continue; }
                        if (js.p < text.size() && text[js.p] == ']') { ++js.p; break; }
                        return fail("expected ',' or ']' in bounding_polygon");
                    }
                }
                have_poly = true;
            } else if (!js.skip(1)) {
                return fail("");
            }
            js.ws();
            if (js.p < text.size() && text[js.p] == ',') { ++js.p; continue; }
            if (js.p < text.size() && text[js.p] == '}') { ++js.p; break; }
            return fail("expected ',' or '}'");
        }
    }
    js.ws();
    if (js.p != text.size()) return fail("data after the closing brace");
    if (!have_min || !have_max || !have_axis || !have_poly)
        return fail("axis_min, axis_max, orthogonal_axis or bounding_polygon is missing");
    if (crop.vertices.size() / 3 < 3) return fail("bounding_polygon has fewer than 3 vertices");
    return true;
}

bool read_matrix4(const std::string &path, double M[16], std::string &err) {
    std::string text;
    if (!read_text_bounded(path, (size_t)1 << 20, "1 MiB", text, err)) return false;
    auto fail = [&](const std::string &what) { err = path + ": " + what; return false; };
    int k = 0;
    for (size_t p = 0; p < text.size();) {
        if (std::isspace((unsigned char)text[p])) { ++p; continue; }
        size_t e = p;
        while (e < text.size() && !std::isspace((unsigned char)text[e])) ++e;
        if (e - p > 400) return fail("a token longer than 400 characters");
        const std::string tok = text.substr(p, e - p);
        JsonCursor num(tok);  // the JSON number grammar: no hex floats, no inf / nan, no locale
        double v;
        if (!num.number(v) || num.p != tok.size()) return fail("'" + tok.substr(0, 32) + "' is not a finite number");
        if (k >= 16) return fail("more than 16 numbers, a 4x4 matrix expected");
        M[k++] = v;
        p = e;
    }
    if (k < 16) return fail(std::to_string(k) + " numbers, 16 (a 4x4 matrix) expected");
    if (M[12] != 0.0 || M[13] != 0.0 || M[14] != 0.0 || M[15] != 1.0) return fail("the last row is not 0 0 0 1");
    return true;
}

// ----------------------------------------------------------------------------------------------
// Level-5 MAT-files
// ----------------------------------------------------------------------------------------------
namespace {

enum : uint32_t { kMiInt8 = 1, kMiUint8 = 2, kMiInt16 = 3, kMiUint16 = 4, kMiInt32 = 5, kMiUint32 = 6, kMiSingle = 7,
                  kMiDouble = 9, kMiInt64 = 12, kMiUint64 = 13, kMiMatrix = 14, kMiCompressed = 15, kMiUtf8 = 16 };

uint32_t mat_u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// bytes per value of a numeric storage type, 0 for any other
size_t mat_type_size(uint32_t mi) {
    switch (mi) {
    case kMiInt8: case kMiUint8: return 1;
    case kMiInt16: case kMiUint16: return 2;
    case kMiInt32: case kMiUint32: case kMiSingle: return 4;
    case kMiDouble: case kMiInt64: case kMiUint64: return 8;
    default: return 0;
    }
}

double mat_value(uint32_t mi, const uint8_t *p) {
    switch (mi) {
    case kMiInt8: return (double)(int8_t)p[0];
    case kMiUint8: return (double)p[0];
    case kMiInt16: { int16_t v; std::memcpy(&v, p, 2); return (double)v; }
    case kMiUint16: { uint16_t v; std::memcpy(&v, p, 2); return (double)v; }
    case kMiInt32: { int32_t v; std::memcpy(&v, p, 4); return (double)v; }
    case kMiUint32: { uint32_t v; std::memcpy(&v, p, 4); return (double)v; }
    case kMiSingle: { float v; std::memcpy(&v, p, 4); return (double)v; }
    case kMiDouble: { double v; std::memcpy(&v, p, 8); return v; }
    case kMiInt64: { int64_t v; std::memcpy(&v, p, 8); return (double)v; }
    default: { uint64_t v; std::memcpy(&v, p, 8); return (double)v; }
    }
}

// One sub-element at offset `off` of a parent whose tag declares `declared` bytes, of which `avail`
// are at hand. data / nbytes: its payload; next: the offset behind its padding.
struct MatSub {
    uint32_t type = 0, nbytes = 0;
    size_t data = 0, next = 0;
};
bool mat_sub(const uint8_t *b, size_t avail, size_t declared, size_t off, MatSub &s, std::string &what) {
    if (off + 8 > declared) { what = "a sub-element tag overruns its matrix"; return false; }
    if (off + 8 > avail) { what = "truncated inside a matrix"; return false; }
    const uint32_t w0 = mat_u32(b + off);
    if (w0 >> 16) {  // the small form: type in the low half, 1 to 4 bytes of payload inside the tag
        s.type = w0 & 0xFFFFu;
        s.nbytes = w0 >> 16;
        if (s.nbytes > 4) { what = "a small element of more than 4 bytes"; return false; }
        s.data = off + 4;
        s.next = off + 8;
        return true;
    }
    s.type = w0;
    s.nbytes = mat_u32(b + off + 4);
    s.data = off + 8;
    if ((uint64_t)s.nbytes > (uint64_t)(declared - s.data)) { what = "a byte count overruns its matrix"; return false; }
    if (s.data + s.nbytes > avail) { what = "truncated inside a matrix"; return false; }
    s.next = s.data + (((size_t)s.nbytes + 7) & ~(size_t)7);
    return true;
}

struct MatHead {
    std::string name;
    uint32_t cls = 0;
    bool complex = false, logical = false;
    std::vector<int64_t> dims;
    size_t data_off = 0;  // offset of the real part's tag
};
// flags, dimensions and name of a matrix body; false with `what` set if malformed
bool mat_head(const uint8_t *b, size_t avail, size_t declared, MatHead &h, std::string &what) {
    MatSub s;
    if (!mat_sub(b, avail, declared, 0, s, what)) return false;
    if (s.type != kMiUint32 || s.nbytes != 8) { what = "no array flags at the start of a matrix"; return false; }
    const uint32_t flags = mat_u32(b + s.data);
    h.cls = flags & 0xFFu;
    h.complex = (flags & 0x0800u) != 0;
    h.logical = (flags & 0x0200u) != 0;
    if (!mat_sub(b, avail, declared, s.next, s, what)) return false;
    if (s.type != kMiInt32 || s.nbytes % 4 != 0 || s.nbytes == 0 || s.nbytes > 4 * 32) {
        what = "a matrix without a dimensions array of 1 to 32 int32";
        return false;
    }
    h.dims.clear();
    for (uint32_t k = 0; k < s.nbytes / 4; ++k) {
        const int32_t d = (int32_t)mat_u32(b + s.data + 4 * k);
        if (d < 0) { what = "a negative dimension"; return false; }
        h.dims.push_back(d);
    }
    if (!mat_sub(b, avail, declared, s.next, s, what)) return false;
    if ((s.type != kMiInt8 && s.type != kMiUint8 && s.type != kMiUtf8) || s.nbytes > 255) {
        what = "a matrix name that is not 0 to 255 bytes of text";
        return false;
    }
    h.name.assign((const char *)b + s.data, s.nbytes);
    h.data_off = s.next;
    return true;
}

const char *mat_class_name(uint32_t cls) {
    switch (cls) {
    case 1: return "a cell array";
    case 2: return "a struct";
    case 3: return "an object";
    case 4: return "a char array";
    case 5: return "sparse";
    default: return "of an unsupported class";
    }
}

// the values of a wanted matrix whose whole body is at hand
bool mat_take(const uint8_t *b, size_t len, const MatHead &h, bool as_mask, MatArray &a, std::string &what) {
    if (h.cls < 6 || h.cls > 15) { what = std::string("is ") + mat_class_name(h.cls); return false; }
    if (h.complex) { what = "is complex"; return false; }
    if (h.dims.size() > 3) { what = "has more than 3 dimensions"; return false; }
    if (as_mask && !h.logical && h.cls != 9) { what = "is neither logical nor uint8"; return false; }
    uint64_t count = 1;
    for (int64_t d : h.dims) {
        count *= (uint64_t)d;  // each factor is below 2^31 and the product is checked every step: no overflow
        if (count > kMatMaxElems) { what = "has more than 2^31 elements"; return false; }
    }
    MatSub s;
    if (!mat_sub(b, len, len, h.data_off, s, what)) return false;
    const size_t size = mat_type_size(s.type);
    if (size == 0) { what = "stores its values in an unsupported type"; return false; }
    if ((uint64_t)s.nbytes != count * size) { what = "holds a byte count that does not match its dimensions"; return false; }
    a.name = h.name;
    a.dims = h.dims;
    a.logical = h.logical;
    const uint8_t *p = b + s.data;
    if (as_mask) {
        a.bytes.resize((size_t)count);
        for (size_t i = 0; i < (size_t)count; ++i) a.bytes[i] = mat_value(s.type, p + i * size) != 0.0 ? 1 : 0;
    } else {
        a.values.resize((size_t)count);
        for (size_t i = 0; i < (size_t)count; ++i) a.values[i] = mat_value(s.type, p + i * size);
    }
    return true;
}

// zlib inflation in steps; the output at most doubles per step (never less than 64 KiB at a time)
struct MatInflater {
    z_stream zs{};
    bool init = false, done = false;
    std::vector<uint8_t> out;
    ~MatInflater() {
        if (init) inflateEnd(&zs);
    }
    bool begin(const uint8_t *p, size_t n) {
        zs.next_in = const_cast<Bytef *>(p);
        zs.avail_in = (uInt)n;  // n <= kMatMaxFile
        init = inflateInit(&zs) == Z_OK;
        return init;
    }
    // inflate until the output holds `upto` bytes or the stream ends; false: corrupt or cut short
    bool fill(size_t upto) {
        while (!done && out.size() < upto) {
            const size_t have = out.size();
            const size_t chunk = std::min(upto - have, std::max<size_t>((size_t)1 << 16, have));
            out.resize(have + chunk);
            zs.next_out = out.data() + have;
            zs.avail_out = (uInt)chunk;
            const int r = inflate(&zs, Z_NO_FLUSH);
            const size_t got = chunk - zs.avail_out;
            out.resize(have + got);
            if (r == Z_STREAM_END) done = true;
            else if (r != Z_OK || got == 0) return false;
        }
        return true;
    }
};

}  // namespace

bool read_mat5(const std::string &path, const std::vector<MatWanted> &wanted, std::vector<MatArray> &out,
               std::string &err) {
    std::string file;
    out.clear();
    if (!read_text_bounded(path, (size_t)kMatMaxFile, "2 GiB", file, err)) return false;
    auto fail = [&](const std::string &what) { err = path + ": " + what; out.clear(); return false; };
    const uint8_t *f = (const uint8_t *)file.data();
    const size_t size = file.size();
    if (size >= 10 && file.compare(0, 10, "MATLAB 7.3") == 0)
        return fail("a MATLAB 7.3 (HDF5) file; re-save it with -v7");
    if (size < 128) return fail("shorter than the 128-byte header of a Level-5 MAT-file");
    if (f[126] == 'M' && f[127] == 'I') return fail("a big-endian MAT-file");
    if (f[126] != 'I' || f[127] != 'M') return fail("no MAT-file endian indicator");
    if (f[124] != 0x00 || f[125] != 0x01) return fail("not version 0x0100 of the MAT-file format");
    std::vector<bool> found(wanted.size(), false);
    out.resize(wanted.size());
    auto want = [&](const std::string &name) {
        for (size_t k = 0; k < wanted.size(); ++k)
            if (wanted[k].name == name) return (int)k;
        return -1;
    };
    // a matrix body with `avail` of its `declared` bytes at hand: <0 malformed, 0 not wanted, 1 wanted
    auto head = [&](const uint8_t *b, size_t avail, size_t declared, MatHead &h, int &slot) {
        std::string what;
        slot = -1;
        if (declared == 0) return 0;  // an empty matrix has no name
        if (!mat_head(b, avail, declared, h, what)) { fail(what); return -1; }
        slot = want(h.name);
        if (slot < 0) return 0;
        if (found[(size_t)slot]) { fail("variable '" + h.name + "' occurs twice"); return -1; }
        return 1;
    };
    auto take = [&](const uint8_t *b, size_t len, const MatHead &h, int slot) {
        std::string what;
        if (!mat_take(b, len, h, wanted[(size_t)slot].as_mask, out[(size_t)slot], what))
            return fail("variable '" + h.name + "' " + what);
        found[(size_t)slot] = true;
        return true;
    };
    size_t pos = 128;
    while (pos < size) {
        if (size - pos < 8) return fail("truncated inside an element tag");
        const uint32_t type = mat_u32(f + pos), nbytes = mat_u32(f + pos + 4);
        if ((type >> 16) != 0) return fail("a small element at the top level");
        if ((uint64_t)nbytes > (uint64_t)(size - pos - 8)) return fail("an element's byte count overruns the file");
        const uint8_t *body = f + pos + 8;
        MatHead h;
        int slot;
        if (type == kMiMatrix) {
            const int r = head(body, nbytes, nbytes, h, slot);
            if (r < 0 || (r > 0 && !take(body, nbytes, h, slot))) return false;
        } else if (type == kMiCompressed) {
            MatInflater z;
            if (!z.begin(body, nbytes)) return fail("zlib could not start");
            if (!z.fill(8) || z.out.size() < 8) return fail("a compressed element that does not inflate to a tag");
            const uint32_t itype = mat_u32(z.out.data()), ibytes = mat_u32(z.out.data() + 4);
            if (itype == kMiMatrix) {
                const uint64_t total = 8 + (uint64_t)ibytes;
                if (total > kMatMaxInflated) return fail("a compressed element declares more than the 2 GiB inflation cap");
                if (!z.fill((size_t)std::min<uint64_t>(total, (uint64_t)1 << 16)))
                    return fail("a compressed element is corrupt or cut short");
                const int r = head(z.out.data() + 8, z.out.size() - 8, ibytes, h, slot);
                if (r < 0) return false;
                if (r > 0) {
                    // one byte beyond the declared size shows a stream that goes on
                    if (!z.fill((size_t)total + 1)) return fail("a compressed element is corrupt or cut short");
                    if (z.out.size() > total) return fail("a compressed element inflates past its declared size");
                    if (z.out.size() < total) return fail("a compressed element inflates to less than its declared size");
                    if (!take(z.out.data() + 8, ibytes, h, slot)) return false;
                }
            }
        }
        pos += 8 + (size_t)nbytes;
    }
    for (size_t k = 0; k < wanted.size(); ++k)
        if (!found[k]) return fail("variable '" + wanted[k].name + "' is missing");
    return true;
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

// ----------------------------------------------------------------------------------------------
// COLMAP sparse models
// ----------------------------------------------------------------------------------------------
namespace {
bool slurp(const std::string &path, std::vector<uint8_t> &data, std::string &err) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { err = "cannot open " + path; return false; }
    in.seekg(0, std::ios::end);
    const std::streamoff n = in.tellg();
    if (n < 0) { err = "cannot size " + path; return false; }
    in.seekg(0);
    data.resize((size_t)n);
    if (n > 0 && !in.read(reinterpret_cast<char *>(data.data()), n)) { err = "cannot read " + path; return false; }
    return true;
}

// the data lines of a COLMAP text file: '#' lines are comments; `keep_empty` keeps blank lines
// (the 2D-point line of an image may be empty)
std::vector<std::string> text_lines(const std::vector<uint8_t> &data, bool keep_empty) {
    std::vector<std::string> lines;
    size_t i = 0;
    while (i < data.size()) {
        size_t j = i;
        while (j < data.size() && data[j] != '\n') ++j;
        std::string line(data.begin() + (long)i, data.begin() + (long)j);
        if (!line.empty() && line.back() == '\r') line.pop_back();
        size_t k = 0;
        while (k < line.size() && isspace((unsigned char)line[k])) ++k;
        const bool blank = k == line.size();
        if (!(k < line.size() && line[k] == '#') && (keep_empty || !blank)) lines.push_back(line);
        i = j + 1;
    }
    return lines;
}

std::vector<std::string> split_ws(const std::string &line) {
    std::vector<std::string> t;
    size_t i = 0;
    while (i < line.size()) {
        while (i < line.size() && isspace((unsigned char)line[i])) ++i;
        size_t j = i;
        while (j < line.size() && !isspace((unsigned char)line[j])) ++j;
        if (j > i) t.push_back(line.substr(i, j - i));
        i = j;
    }
    return t;
}

bool tok_double(const std::string &s, double &v) {
    if (s.empty() || s.size() > 64) return false;
    char *end = nullptr;
    v = std::strtod(s.c_str(), &end);
    return end == s.c_str() + s.size() && std::isfinite(v);
}
bool tok_int(const std::string &s, long long lo, long long hi, long long &v) {
    if (s.empty() || s.size() > 24) return false;
    char *end = nullptr;
    errno = 0;
    v = std::strtoll(s.c_str(), &end, 10);
    return errno == 0 && end == s.c_str() + s.size() && v >= lo && v <= hi;
}

// little-endian cursor over a binary file
struct Cursor {
    const std::vector<uint8_t> &d;
    size_t pos = 0;
    size_t left() const { return d.size() - pos; }
    template <class T> bool get(T &v) {
        if (left() < sizeof(T)) return false;
        memcpy(&v, d.data() + pos, sizeof(T));
        pos += sizeof(T);
        return true;
    }
};

const char *const kColmapModels[] = {"SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE",
                                     "FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE",
                                     "THIN_PRISM_FISHEYE"};
const int kColmapModelParams[] = {3, 4, 4, 5, 8, 8, 12, 0, 4, 5, 12};  // 0: FOV, never read

// the parameter count of a model that may be read, else 0
int model_params(const std::string &model, bool distorted_ok) {
    const int id = colmap_model_id(model);
    return id < 0 || (id > 1 && !distorted_ok) ? 0 : kColmapModelParams[id];
}

bool read_cameras(const std::string &path, bool bin, bool distorted_ok, std::vector<ColmapCamera> &cams,
                  std::string &err) {
    std::vector<uint8_t> data;
    if (!slurp(path, data, err)) return false;
    auto fail = [&](const std::string &w) { err = path + ": " + w; return false; };
    if (bin) {
        Cursor c{data};
        uint64_t n = 0;
        if (!c.get(n)) return fail("truncated header");
        if (n > c.left() / 48) return fail("camera count " + std::to_string(n) + " exceeds the file");
        for (uint64_t i = 0; i < n; ++i) {
            ColmapCamera cam;
            int32_t model = 0;
            if (!c.get(cam.id) || !c.get(model) || !c.get(cam.width) || !c.get(cam.height)) return fail("truncated camera");
            if (model < 0 || model > 10 || !model_params(kColmapModels[model], distorted_ok))
                return fail("unsupported camera model " +
                            (model >= 2 && model <= 10 ? std::string(kColmapModels[model]) : "id " + std::to_string(model)) +
                            " (only SIMPLE_PINHOLE and PINHOLE; undistort the images first)");
            cam.model = kColmapModels[model];
            cam.params.resize((size_t)model_params(cam.model, distorted_ok));
            for (double &p : cam.params)
                if (!c.get(p) || !std::isfinite(p)) return fail("truncated or non-finite camera parameters");
            cams.push_back(cam);
        }
        if (c.left()) return fail("bytes after the last camera");
    } else {
        for (const std::string &line : text_lines(data, false)) {
            const std::vector<std::string> t = split_ws(line);
            ColmapCamera cam;
            long long id, w, h;
            if (t.size() < 4 || !tok_int(t[0], 0, UINT32_MAX, id) || !tok_int(t[2], 0, INT32_MAX, w) ||
                !tok_int(t[3], 0, INT32_MAX, h))
                return fail("bad camera line '" + line.substr(0, 80) + "'");
            cam.id = (uint32_t)id;
            cam.model = t[1];
            cam.width = (uint64_t)w;
            cam.height = (uint64_t)h;
            const int np = model_params(cam.model, distorted_ok);
            if (!np)
                return fail("unsupported camera model " + cam.model.substr(0, 40) +
                            " (only SIMPLE_PINHOLE and PINHOLE; undistort the images first)");
            if ((int)t.size() != 4 + np) return fail("camera " + t[0] + ": wrong number of parameters");
            cam.params.resize((size_t)np);
            for (int k = 0; k < np; ++k)
                if (!tok_double(t[4 + (size_t)k], cam.params[(size_t)k])) return fail("camera " + t[0] + ": bad parameter");
            cams.push_back(cam);
        }
    }
    for (const ColmapCamera &cam : cams)
        if (cam.width < 1 || cam.height < 1 || cam.width > 65536 || cam.height > 65536)
            return fail("camera " + std::to_string(cam.id) + ": size out of range");
    if (cams.empty()) return fail("no camera");
    return true;
}

bool read_images(const std::string &path, bool bin, std::vector<ColmapImage> &images, std::string &err) {
    std::vector<uint8_t> data;
    if (!slurp(path, data, err)) return false;
    auto fail = [&](const std::string &w) { err = path + ": " + w; return false; };
    if (bin) {
        Cursor c{data};
        uint64_t n = 0;
        if (!c.get(n)) return fail("truncated header");
        if (n > c.left() / 73) return fail("image count " + std::to_string(n) + " exceeds the file");
        images.reserve((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            ColmapImage im;
            if (!c.get(im.id)) return fail("truncated image");
            for (double &v : im.q) if (!c.get(v) || !std::isfinite(v)) return fail("truncated or non-finite pose");
            for (double &v : im.t) if (!c.get(v) || !std::isfinite(v)) return fail("truncated or non-finite pose");
            if (!c.get(im.camera_id)) return fail("truncated image");
            size_t e = c.pos;
            while (e < data.size() && data[e] != 0) ++e;
            if (e == data.size() || e - c.pos > 4096) return fail("unterminated image name");
            im.name.assign(data.begin() + (long)c.pos, data.begin() + (long)e);
            c.pos = e + 1;
            uint64_t np = 0;
            if (!c.get(np)) return fail("truncated image");
            if (np > c.left() / 24) return fail("2D point count " + std::to_string(np) + " exceeds the file");
            im.xy.resize(2 * (size_t)np);
            im.point_ids.resize((size_t)np);
            for (size_t k = 0; k < (size_t)np; ++k) {
                c.get(im.xy[2 * k]);
                c.get(im.xy[2 * k + 1]);
                c.get(im.point_ids[k]);
                if (im.point_ids[k] < -1) return fail("image " + std::to_string(im.id) + ": bad point id");
            }
            images.push_back(std::move(im));
        }
        if (c.left()) return fail("bytes after the last image");
    } else {
        const std::vector<std::string> lines = text_lines(data, true);
        size_t li = 0;
        while (li < lines.size()) {
            const std::vector<std::string> t = split_ws(lines[li]);
            if (t.empty()) { ++li; continue; }  // blank lines between images
            ColmapImage im;
            long long id, cam;
            if (t.size() != 10 || !tok_int(t[0], 0, UINT32_MAX, id) || !tok_int(t[8], 0, UINT32_MAX, cam))
                return fail("bad image line '" + lines[li].substr(0, 80) + "'");
            for (int k = 0; k < 4; ++k) if (!tok_double(t[1 + (size_t)k], im.q[k])) return fail("image " + t[0] + ": bad pose");
            for (int k = 0; k < 3; ++k) if (!tok_double(t[5 + (size_t)k], im.t[k])) return fail("image " + t[0] + ": bad pose");
            im.id = (uint32_t)id;
            im.camera_id = (uint32_t)cam;
            im.name = t[9];
            if (li + 1 >= lines.size()) return fail("image " + t[0] + ": missing 2D-point line");
            const std::vector<std::string> p = split_ws(lines[li + 1]);
            if (p.size() % 3) return fail("image " + t[0] + ": the 2D-point line is not made of triples");
            im.xy.resize(p.size() / 3 * 2);
            im.point_ids.resize(p.size() / 3);
            for (size_t k = 0; k < p.size() / 3; ++k) {
                long long pid;
                if (!tok_double(p[3 * k], im.xy[2 * k]) || !tok_double(p[3 * k + 1], im.xy[2 * k + 1]) ||
                    !tok_int(p[3 * k + 2], -1, LLONG_MAX, pid))
                    return fail("image " + t[0] + ": bad 2D point '" + p[3 * k + 2].substr(0, 40) + "'");
                im.point_ids[k] = pid;
            }
            images.push_back(std::move(im));
            li += 2;
        }
    }
    if (images.empty()) return fail("no image");
    std::sort(images.begin(), images.end(), [](const ColmapImage &a, const ColmapImage &b) { return a.id < b.id; });
    for (size_t i = 1; i < images.size(); ++i)
        if (images[i].id == images[i - 1].id) return fail("duplicate image id " + std::to_string(images[i].id));
    for (const ColmapImage &im : images)
        if (im.name.empty() || im.name[0] == '/' || im.name.find("..") != std::string::npos)
            return fail("image " + std::to_string(im.id) + ": unusable name");
    return true;
}

bool read_points(const std::string &path, bool bin, std::vector<int64_t> &ids, std::vector<double> &xyz, std::string &err) {
    std::vector<uint8_t> data;
    if (!slurp(path, data, err)) return false;
    auto fail = [&](const std::string &w) { err = path + ": " + w; return false; };
    if (bin) {
        Cursor c{data};
        uint64_t n = 0;
        if (!c.get(n)) return fail("truncated header");
        if (n > c.left() / 51) return fail("point count " + std::to_string(n) + " exceeds the file");
        ids.reserve((size_t)n);
        xyz.reserve(3 * (size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t id = 0, track = 0;
            double p[3], e;
            uint8_t rgb[3];
            if (!c.get(id) || !c.get(p[0]) || !c.get(p[1]) || !c.get(p[2]) || !c.get(rgb[0]) || !c.get(rgb[1]) ||
                !c.get(rgb[2]) || !c.get(e) || !c.get(track))
                return fail("truncated point");
            if (id > (uint64_t)INT64_MAX) return fail("point id out of range");
            if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return fail("non-finite point");
            if (track > c.left() / 8) return fail("track length " + std::to_string(track) + " exceeds the file");
            c.pos += 8 * (size_t)track;
            ids.push_back((int64_t)id);
            xyz.insert(xyz.end(), p, p + 3);
        }
        if (c.left()) return fail("bytes after the last point");
    } else {
        for (const std::string &line : text_lines(data, false)) {
            const std::vector<std::string> t = split_ws(line);
            long long id;
            double p[3];
            if (t.size() < 8 || t.size() % 2 || !tok_int(t[0], 0, LLONG_MAX, id) || !tok_double(t[1], p[0]) ||
                !tok_double(t[2], p[1]) || !tok_double(t[3], p[2]))
                return fail("bad point line '" + line.substr(0, 80) + "'");
            ids.push_back(id);
            xyz.insert(xyz.end(), p, p + 3);
        }
    }
    return true;
}
}  // namespace

int colmap_model_id(const std::string &model) {
    for (int id = 0; id <= 10; ++id)
        if (id != 7 && model == kColmapModels[id]) return id;
    return -1;
}

bool read_colmap_model(const std::string &dir, const std::string &ext, ColmapModel &m, std::string &err,
                       bool distorted_ok) {
    m = ColmapModel();
    if (ext != ".txt" && ext != ".bin") { err = "model extension must be .txt or .bin, not '" + ext + "'"; return false; }
    const bool bin = ext == ".bin";
    if (!read_cameras(dir + "/cameras" + ext, bin, distorted_ok, m.cameras, err) ||
        !read_images(dir + "/images" + ext, bin, m.images, err) ||
        !read_points(dir + "/points3D" + ext, bin, m.point_ids, m.xyz, err))
        return false;
    std::map<uint32_t, int> cams;
    for (const ColmapCamera &c : m.cameras)
        if (!cams.emplace(c.id, 0).second) { err = dir + ": duplicate camera id " + std::to_string(c.id); return false; }
    for (const ColmapImage &im : m.images)
        if (!cams.count(im.camera_id)) {
            err = dir + ": image " + std::to_string(im.id) + " names camera " + std::to_string(im.camera_id) + ", which is missing";
            return false;
        }
    return true;
}

bool colmap_prep_arrays(const ColmapModel &m, PrepArrays &a, std::string &err) {
    a = PrepArrays();
    std::vector<std::pair<int64_t, int32_t>> index(m.point_ids.size());
    if (m.point_ids.size() > (size_t)INT32_MAX) { err = "more than INT32_MAX points"; return false; }
    for (size_t k = 0; k < m.point_ids.size(); ++k) index[k] = {m.point_ids[k], (int32_t)k};
    std::sort(index.begin(), index.end());
    for (size_t k = 1; k < index.size(); ++k)
        if (index[k].first == index[k - 1].first) { err = "duplicate point id " + std::to_string(index[k].first); return false; }
    a.obs_offset.push_back(0);
    for (const ColmapImage &im : m.images) {
        const double w = im.q[0], x = im.q[1], y = im.q[2], z = im.q[3];
        const double R[9] = {(1 - 2 * (y * y)) - 2 * (z * z), (2 * x) * y - (2 * w) * z, (2 * z) * x + (2 * w) * y,
                             (2 * x) * y + (2 * w) * z, (1 - 2 * (x * x)) - 2 * (z * z), (2 * y) * z - (2 * w) * x,
                             (2 * z) * x - (2 * w) * y, (2 * y) * z + (2 * w) * x, (1 - 2 * (x * x)) - 2 * (y * y)};
        a.rot.insert(a.rot.end(), R, R + 9);
        a.trans.insert(a.trans.end(), im.t, im.t + 3);
        for (int k = 0; k < 3; ++k) a.centres.push_back(-((R[k] * im.t[0] + R[3 + k] * im.t[1]) + R[6 + k] * im.t[2]));
        for (int64_t pid : im.point_ids) {
            if (pid == -1) continue;
            auto it = std::lower_bound(index.begin(), index.end(), std::make_pair(pid, (int32_t)INT32_MIN));
            if (it == index.end() || it->first != pid) {
                err = "image " + std::to_string(im.id) + " names point " + std::to_string(pid) + ", which points3D lacks";
                return false;
            }
            a.obs_point.push_back(it->second);
        }
        if (a.obs_point.size() > (size_t)INT32_MAX) { err = "more than INT32_MAX observations"; return false; }
        a.obs_offset.push_back((int64_t)a.obs_point.size());
    }
    return true;
}

ViewSelection select_sequential(int n, int k) {
    ViewSelection sel((size_t)std::max(n, 0));
    const long lim = std::min<long>((long)n - 1, 2L * k);
    for (int i = 0; i < n; ++i) {
        std::vector<std::pair<int, int>> nb;
        for (int off = 1; off <= k; ++off)
            for (int dir = -1; dir <= 1; dir += 2) {
                const long j = (long)i + (long)dir * off;
                if (j >= 0 && j < n) nb.push_back({(int)j, k + 1 - off});
            }
        std::stable_sort(nb.begin(), nb.end(), [i](const std::pair<int, int> &a, const std::pair<int, int> &b) {
            if (a.second != b.second) return a.second > b.second;
            return std::abs(a.first - i) < std::abs(b.first - i);
        });
        if ((long)nb.size() > lim) nb.resize((size_t)std::max(lim, 0L));
        sel[(size_t)i] = nb;
    }
    return sel;
}

ViewSelection select_scored(int n, const uint32_t *shared, const uint32_t *narrow, int max_views) {
    ViewSelection sel((size_t)std::max(n, 0));
    const int take = std::max(0, std::min(max_views, n - 1));
    std::vector<std::pair<int64_t, int>> cand;
    for (int i = 0; i < n; ++i) {
        cand.clear();
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const uint64_t s = shared[(size_t)i * n + j], nar = narrow[(size_t)i * n + j];
            const int64_t score = nar >= 3 * s / 4 + 1 ? 0 : (int64_t)s;
            cand.push_back({-score, j});
        }
        std::partial_sort(cand.begin(), cand.begin() + take, cand.end());
        for (int k = 0; k < take; ++k) sel[(size_t)i].push_back({cand[(size_t)k].second, (int)-cand[(size_t)k].first});
    }
    return sel;
}

std::string shortest_double(double v) {
    char buf[40];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof buf, v);  // shortest round-trip form
    return std::string(buf, r.ptr);
}

bool write_cam_txt(const std::string &path, const double R[9], const double t[3], const double K[9], double depth_min,
                   double interval, double depth_num, double depth_max) {
    std::ofstream o(path);
    if (!o) return false;
    o << "extrinsic\n";
    for (int r = 0; r < 3; ++r)
        o << shortest_double(R[3 * r]) << ' ' << shortest_double(R[3 * r + 1]) << ' ' << shortest_double(R[3 * r + 2])
          << ' ' << shortest_double(t[r]) << " \n";
    o << "0.0 0.0 0.0 1.0 \n\nintrinsic\n";
    for (int r = 0; r < 3; ++r)
        o << shortest_double(K[3 * r]) << ' ' << shortest_double(K[3 * r + 1]) << ' ' << shortest_double(K[3 * r + 2])
          << " \n";
    char buf[256];
    snprintf(buf, sizeof buf, "\n%f %f %f %f\n", depth_min, interval, depth_num, depth_max);
    o << buf;
    o.flush();
    return (bool)o;
}

bool write_pair_txt(const std::string &path, const ViewSelection &sel) {
    std::ofstream o(path);
    if (!o) return false;
    o << sel.size() << '\n';
    for (size_t i = 0; i < sel.size(); ++i) {
        o << i << '\n' << sel[i].size() << ' ';
        for (const auto &js : sel[i]) o << js.first << ' ' << js.second << ' ';
        o << '\n';
    }
    o.flush();
    return (bool)o;
}

bool write_colmap_cameras_txt(const std::string &path, const std::vector<ColmapCamera> &cams) {
    std::ofstream o(path);
    if (!o) return false;
    o << "# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n"
      << "# Number of cameras: " << cams.size() << '\n';
    for (const ColmapCamera &c : cams) {
        o << c.id << ' ' << c.model << ' ' << c.width << ' ' << c.height;
        for (double p : c.params) o << ' ' << shortest_double(p);
        o << '\n';
    }
    o.flush();
    return (bool)o;
}

bool write_colmap_images_txt(const std::string &path, const std::vector<ColmapImage> &images) {
    std::ofstream o(path);
    if (!o) return false;
    o << "# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
      << "#   POINTS2D[] as (X, Y, POINT3D_ID)\n# Number of images: " << images.size() << '\n';
    for (const ColmapImage &im : images) {
        o << im.id;
        for (double v : im.q) o << ' ' << shortest_double(v);
        for (double v : im.t) o << ' ' << shortest_double(v);
        o << ' ' << im.camera_id << ' ' << im.name << '\n';
        for (size_t k = 0; k < im.point_ids.size(); ++k)
            o << (k ? " " : "") << shortest_double(im.xy[2 * k]) << ' ' << shortest_double(im.xy[2 * k + 1]) << ' '
              << im.point_ids[k];
        o << '\n';
    }
    o.flush();
    return (bool)o;
}

bool copy_file(const std::string &from, const std::string &to) {
    std::ifstream in(from, std::ios::binary);
    if (!in) return false;
    std::ofstream o(to, std::ios::binary);
    if (!o) return false;
    o << in.rdbuf();
    o.flush();
    return (bool)o && !in.bad();
}

bool scan_image_sizes(const std::string &image_dir, const std::vector<std::string> &names, std::vector<int> &widths,
                      std::vector<int> &heights, std::string &err) {
    widths.assign(names.size(), 0);
    heights.assign(names.size(), 0);
    for (size_t i = 0; i < names.size(); ++i) {
        Bgr8 img;
        if (!read_bgr8(image_dir + "/" + names[i], img, err)) return false;
        if (img.width < 1 || img.height < 1) { err = "empty image " + names[i]; return false; }
        widths[i] = img.width;
        heights[i] = img.height;
    }
    return true;
}

bool convert_scan_images(const std::string &image_dir, const std::vector<std::string> &names,
                         const std::vector<int> &widths, const std::vector<int> &heights, double scale,
                         const std::string &out_dir, std::vector<std::string> &out_names, int &out_w, int &out_h,
                         int &copied, std::string &err, const ScanImageWarp *warp) {
    out_names.clear();
    copied = 0;
    if (names.empty() || widths.size() != names.size() || heights.size() != names.size() || !(scale > 0) ||
        (warp && warp->mask.size() != names.size())) {
        err = "convert_scan_images: bad arguments";
        return false;
    }
    const int max_w = *std::max_element(widths.begin(), widths.end());
    const int max_h = *std::max_element(heights.begin(), heights.end());
    out_w = (int)((double)max_w / scale);
    out_h = (int)((double)max_h / scale);
    if (out_w < 1 || out_h < 1) { err = "the scale factor leaves no pixels"; return false; }
    for (size_t i = 0; i < names.size(); ++i) {
        const std::string src = image_dir + "/" + names[i];
        std::string e;
        const size_t dot = names[i].rfind('.'), slash = names[i].rfind('/');
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) e = names[i].substr(dot);
        for (char &c : e) c = (char)tolower((unsigned char)c);
        const bool warped = warp && warp->mask[i];
        const bool as_is = !warped && scale == 1.0 && widths[i] == max_w && heights[i] == max_h &&
                           (e == ".jpg" || e == ".jpeg" || e == ".png");
        const std::string name = format_index((int)i) + (as_is ? e : ".png");
        for (const char *stale : {".jpg", ".jpeg", ".png"})
            if (name != format_index((int)i) + stale) std::remove((out_dir + "/" + format_index((int)i) + stale).c_str());
        if (as_is) {
            if (!copy_file(src, out_dir + "/" + name)) { err = "cannot copy " + src + " to " + out_dir + "/" + name; return false; }
            ++copied;
        } else {
            Bgr8 img;
            if (!read_bgr8(src, img, err)) return false;
            if (img.width != widths[i] || img.height != heights[i]) { err = src + " changed size"; return false; }
            if (warped) {
                if (!warp->apply(i, img, err)) return false;
                if (img.width != widths[i] || img.height != heights[i] ||
                    img.px.size() != 3 * (size_t)img.width * (size_t)img.height) {
                    err = "the warp of " + src + " changed its size";
                    return false;
                }
            }
            std::vector<uint8_t> pad(3 * (size_t)max_w * max_h, 0);
            for (int r = 0; r < img.height; ++r)
                memcpy(&pad[3 * (size_t)r * max_w], &img.px[3 * (size_t)r * img.width], 3 * (size_t)img.width);
            std::vector<uint8_t> out(3 * (size_t)out_w * out_h);
            resize_nearest(pad.data(), max_w, max_h, out.data(), out_w, out_h, 3);
            if (!write_png_bgr8(out_dir + "/" + name, out.data(), out_w, out_h)) {
                err = "cannot write " + out_dir + "/" + name;
                return false;
            }
        }
        out_names.push_back(name);
    }
    return true;
}

}  // namespace apdhost
