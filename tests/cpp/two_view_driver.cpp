// two_view_driver.cpp -- TwoViewReconstruction (reference src/TwoViewReconstruction.cc) through the drop-in of
// include/rfe/two_view_reconstruction.h on a case read from a file, over mock KeyPoint / Point3f types; dumps what came back and where the
// random stream stands.
// usage: two_view_driver <case.bin> <out.bin>    (with fewer arguments it exits 0 at once: tests/test_two_view_ref.py compiles it)
// case.bin: i32 n1, n2, iterations, number of random numbers | f32 fx fy cx cy sigma rh_threshold | n1 x (f32 x, y) | n2 x (f32 x, y) |
//           n1 x i32 vMatches12 | the random numbers x i32
// out.bin:  i32 ret, status, model, random numbers taken, size of vP3D, size of vbTriangulated | i32 stats[16] | f32 R21[9], t21[3] |
//           vP3D x (f32 x, y, z) | vbTriangulated x u8
#include "driver_common.h"
#include "rfe/two_view_reconstruction.h"

struct MockPoint2 { float x = 0, y = 0; };
struct MockKeyPoint { MockPoint2 pt; int octave = 0; };
struct MockPoint3 {
    float x, y, z;
    MockPoint3() : x(-1.f), y(-1.f), z(-1.f) {}
    MockPoint3(float a, float b, float c) : x(a), y(b), z(c) {}
};

int main(int argc, char** argv) {
    if (argc < 3) return 0;
    FILE* fi = open_case(argv[1]);
    if (!fi) return EXIT_BAD_CASE;
    int32_t hd[4]; float cam[6];
    if (fread(hd, 4, 4, fi) != 4 || fread(cam, 4, 6, fi) != 6 || hd[0] < 0 || hd[1] < 0 || hd[3] < 0) return EXIT_BAD_CASE;
    std::vector<float> k1, k2;
    std::vector<int32_t> m12, numbers;
    if (!get(fi, k1, (size_t)hd[0] * 2) || !get(fi, k2, (size_t)hd[1] * 2) || !get(fi, m12, (size_t)hd[0]) || !get(fi, numbers, (size_t)hd[3]))
        return short_case();
    fclose(fi);
    std::vector<MockKeyPoint> keys1(hd[0]), keys2(hd[1]);
    for (int i = 0; i < hd[0]; ++i) { keys1[i].pt.x = k1[2 * i]; keys1[i].pt.y = k1[2 * i + 1]; }
    for (int i = 0; i < hd[1]; ++i) { keys2[i].pt.x = k2[2 * i]; keys2[i].pt.y = k2[2 * i + 1]; }
    std::vector<int> matches(m12.begin(), m12.end());
    rfe_ctx* ctx = make_context();
    if (!ctx) return EXIT_LIBRARY;
    size_t taken = 0;
    auto rand31 = [&]() { return taken < numbers.size() ? numbers[taken++] : (++taken, 0); };
    ORB_SLAM3::TwoViewReconstruction_rfe tvr(ctx, rand31, cam[0], cam[1], cam[2], cam[3], cam[4], hd[2]);
    tvr.SetHomographyRatio(cam[5]);
    ORB_SLAM3::TwoViewReconstruction_rfe::Mat3 R21; R21.fill(-2.f);
    ORB_SLAM3::TwoViewReconstruction_rfe::Vec3 t21; t21.fill(-2.f);
    std::vector<MockPoint3> vP3D(3);                                     // a caller's stale vectors
    std::vector<bool> vbTriangulated(5, true);
    const bool ret = tvr.Reconstruct(keys1, keys2, matches, R21, t21, vP3D, vbTriangulated);
    if (tvr.status() < -1) fprintf(stderr, "drop-in: %d %s\n", tvr.status(), rfe_last_error(ctx));
    const int32_t head[6] = {ret, tvr.status(), tvr.model(), (int32_t)taken, (int32_t)vP3D.size(), (int32_t)vbTriangulated.size()};
    int32_t stats[16];
    for (int k = 0; k < 16; ++k) stats[k] = tvr.stats()[k];
    rfe_destroy(ctx);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return EXIT_OUTPUT;
    fwrite(head, 4, 6, fo); fwrite(stats, 4, 16, fo); fwrite(R21.data(), 4, 9, fo); fwrite(t21.data(), 4, 3, fo);
    for (const MockPoint3& p : vP3D) { const float v[3] = {p.x, p.y, p.z}; fwrite(v, 4, 3, fo); }
    std::vector<uint8_t> o(vbTriangulated.size());
    for (size_t i = 0; i < o.size(); ++i) o[i] = vbTriangulated[i] ? 1 : 0;
    put(fo, o);
    fclose(fo);
    return 0;
}
