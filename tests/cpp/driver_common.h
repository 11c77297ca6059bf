// driver_common.h -- what the drop-in drivers of this directory share: Eigen / Sophus-shaped stand-ins with the reference's member names, the
// case-file and context prologue, and the exit codes the Python tests see.  A stand-in that differs on purpose stays in its driver.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rover_fe.h"

enum { EXIT_BAD_CASE = 2, EXIT_LIBRARY = 3, EXIT_OUTPUT = 5 };

struct Vec3 {
    float v[3];
    Vec3() : v{0, 0, 0} {}
    Vec3(float x, float y, float z) : v{x, y, z} {}
    float operator()(int i) const { return v[i]; }
};
struct Mat3 {
    float m[9];
    float operator()(int r, int c) const { return m[3 * r + c]; }
};
struct MiniSE3 {                        // rotation + translation, as Sophus::SE3f hands them out
    Mat3 R; Vec3 t;
    Mat3 rotationMatrix() const { return R; }
    Vec3 translation() const { return t; }
};
struct MockCamera {                     // GeometricCamera::GetType is unsigned and not const (include/CameraModels/GeometricCamera.h)
    unsigned int type = 0;
    unsigned int GetType() { return type; }
};

template <class T>
inline bool get(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == n; }
template <class T>
inline void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

// the case file; NULL after "cannot open" (exit EXIT_BAD_CASE)
inline FILE* open_case(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) fprintf(stderr, "cannot open %s\n", path);
    return f;
}
inline int short_case() { fprintf(stderr, "short case file\n"); return EXIT_BAD_CASE; }
// the context; NULL after rfe_init's error (exit EXIT_LIBRARY)
inline rfe_ctx* make_context() {
    rfe_ctx* ctx = nullptr;
    if (rfe_init(0, &ctx) != RFE_OK) { fprintf(stderr, "rfe_init: %s\n", rfe_last_error(nullptr)); return nullptr; }
    return ctx;
}
