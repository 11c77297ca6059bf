// Argument plumbing shared by the harness programs of this directory (ref_main.cc, ref_bow_main.cc).  Written for this project.
// <in> / <out>: int32 count, then per array { int32 dtype (0 u8, 1 i32, 2 f32, 3 f64), int64 elements, data }.
#ifndef RFE_REF_IO_H
#define RFE_REF_IO_H
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace {
struct Arr {
    int32_t dtype;
    std::vector<unsigned char> bytes;
    static size_t esz(int t) { return t == 0 ? 1 : t == 3 ? 8 : 4; }
    size_t n() const { return bytes.size() / esz(dtype); }
    const uint8_t* u8() const { need(0); return bytes.data(); }
    const int32_t* i32() const { need(1); return (const int32_t*)bytes.data(); }
    const float* f32() const { need(2); return (const float*)bytes.data(); }
    const double* f64() const { need(3); return (const double*)bytes.data(); }
    void need(int t) const { if (dtype != t) throw std::runtime_error("array dtype mismatch"); }
};

std::vector<Arr> read_all(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    int32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1 || count < 0 || count > 64) throw std::runtime_error("bad header");
    std::vector<Arr> out((size_t)count);
    for (auto& a : out) {
        int64_t n = 0;
        if (std::fread(&a.dtype, 4, 1, f) != 1 || std::fread(&n, 8, 1, f) != 1 || a.dtype < 0 || a.dtype > 3 || n < 0)
            throw std::runtime_error("bad array header");
        a.bytes.resize((size_t)n * Arr::esz(a.dtype));
        if (!a.bytes.empty() && std::fread(a.bytes.data(), 1, a.bytes.size(), f) != a.bytes.size()) throw std::runtime_error("short read");
    }
    std::fclose(f);
    return out;
}

struct Writer {
    std::vector<Arr> arrs;
    template <typename T> void add(int dtype, const T* p, size_t n) {
        if (sizeof(T) != Arr::esz(dtype)) throw std::runtime_error("Writer::add: element size");
        Arr a; a.dtype = dtype;
        a.bytes.assign((const unsigned char*)p, (const unsigned char*)p + n * sizeof(T));
        arrs.push_back(a);
    }
    template <typename T> void add(int dtype, const std::vector<T>& v) { add(dtype, v.data(), v.size()); }
    void write(const char* path) {
        FILE* f = std::fopen(path, "wb");
        if (!f) throw std::runtime_error(std::string("cannot write ") + path);
        int32_t count = (int32_t)arrs.size();
        std::fwrite(&count, 4, 1, f);
        for (auto& a : arrs) {
            int64_t n = (int64_t)a.n();
            std::fwrite(&a.dtype, 4, 1, f); std::fwrite(&n, 8, 1, f);
            if (!a.bytes.empty()) std::fwrite(a.bytes.data(), 1, a.bytes.size(), f);
        }
        if (std::fclose(f) != 0) throw std::runtime_error("write failed");
    }
};

void want(bool ok, const char* what) { if (!ok) throw std::runtime_error(what); }
}  // namespace
#endif
