// Minimal stand-in for the few OpenCV names the classic Rover-SLAM function bodies use (oracle/ref_classic/build_ref.py).
// Written for this project; no OpenCV text.  Only what those bodies touch is here: a reference-counted 2-D Mat of u8 / f32 with
// views, KeyPoint / Point2f / Size, norm (L1 / L2), threshold (THRESH_BINARY) and cvRound; for DBoW3 (ref_bow_main.cc) also
// Mat::create / ptr<T> / isContinuous and the NAMES FileStorage / FileNode, declared only (Vocabulary.h mentions them).
#ifndef RFE_REF_CV_STANDIN_H
#define RFE_REF_CV_STANDIN_H
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

typedef unsigned char uchar;
#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 CV_8U
#define CV_32FC1 CV_32F

namespace cv {

class Exception : public std::exception {
public:
    explicit Exception(const std::string& m) : msg(m) {}
    const char* what() const noexcept override { return msg.c_str(); }
    std::string msg;
};

struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};

struct Point2f {
    float x, y;
    Point2f() : x(0), y(0) {}
    Point2f(float x_, float y_) : x(x_), y(y_) {}
};
// OpenCV's Point_<float> operators: component-wise, every result saturate_cast<float> of a float expression (= the float itself)
inline Point2f operator-(const Point2f& a, const Point2f& b) { return Point2f(a.x - b.x, a.y - b.y); }
inline Point2f operator+(const Point2f& a, const Point2f& b) { return Point2f(a.x + b.x, a.y + b.y); }
inline Point2f operator/(const Point2f& a, float b) { return Point2f(a.x / b, a.y / b); }
inline Point2f operator*(const Point2f& a, float b) { return Point2f(a.x * b, a.y * b); }

struct KeyPoint {
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

// 2-D single-channel matrix of u8 or f32.  Copies share the buffer (as cv::Mat does); row / rowRange / colRange are views.
// `tag` is the stand-in's own: row(i) stamps i on the view and clone() keeps it, so that a caller can tell WHICH row a cloned
// descriptor came from (MapPoint::ComputeDistinctiveDescriptors keeps only the clone).
class Mat {
public:
    int rows, cols;
    size_t step;      // bytes per row
    uchar* data;
    int tag;
    Mat() : rows(0), cols(0), step(0), data(nullptr), tag(-1), type_(CV_8U) {}
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(Size s, int type) { create(s.height, s.width, type); }
    Mat(int r, int c, int type, void* ext, size_t step_bytes = 0)    // external data, not owned
        : rows(r), cols(c), step(step_bytes ? step_bytes : (size_t)c * esz(type)), data((uchar*)ext), tag(-1), type_(type) {}
    int type() const { return type_; }
    int channels() const { return 1; }
    bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
    Size size() const { return Size(cols, rows); }
    size_t elemSize() const { return esz(type_); }
    Mat row(int y) const {
        if (y < 0 || y >= rows) throw Exception("Mat::row out of range");
        Mat m = rowRange(y, y + 1);
        m.tag = y;
        return m;
    }
    Mat rowRange(int a, int b) const {
        if (!(0 <= a && a <= b && b <= rows)) throw Exception("Mat::rowRange out of range");
        Mat m(*this);
        m.rows = b - a;
        m.data = data + (size_t)a * step;
        return m;
    }
    Mat colRange(int a, int b) const {
        if (!(0 <= a && a <= b && b <= cols)) throw Exception("Mat::colRange out of range");
        Mat m(*this);
        m.cols = b - a;
        m.data = data + (size_t)a * elemSize();
        return m;
    }
    template <typename T> T& at(int y, int x) { chk<T>(y, x); return *(T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
    template <typename T> const T& at(int y, int x) const { chk<T>(y, x); return *(const T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
    // one index: element i of a single-row (or single-column) matrix
    template <typename T> T& at(int i) { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    template <typename T> const T& at(int i) const { return rows == 1 ? at<T>(0, i) : at<T>(i, 0); }
    Mat clone() const {
        Mat m(rows, cols, type_);
        for (int y = 0; y < rows; ++y) std::memcpy(m.data + (size_t)y * m.step, data + (size_t)y * step, (size_t)cols * elemSize());
        m.tag = tag;
        return m;
    }
    const uchar* ptr(int y) const { return data + (size_t)y * step; }
    // typed row pointer; as in OpenCV the type is the caller's claim (DescManip::distance reads CV_8U rows as uint64_t)
    template <typename T> T* ptr(int y = 0) { rowchk(y); return (T*)(data + (size_t)y * step); }
    template <typename T> const T* ptr(int y = 0) const { rowchk(y); return (const T*)(data + (size_t)y * step); }
    bool isContinuous() const { return rows <= 1 || step == (size_t)cols * elemSize(); }
    // a fresh zeroed buffer of the given shape (OpenCV keeps the old one when the shape is unchanged and does not zero)
    void create(int r, int c, int type) {
        if (type != CV_8U && type != CV_32F) throw Exception("Mat: unsupported type");
        rows = r; cols = c; type_ = type; tag = -1;
        step = (size_t)c * esz(type);
        own_ = std::make_shared<std::vector<uchar> >((size_t)r * step + 1, (uchar)0);
        data = own_->data();
    }

private:
    int type_;
    std::shared_ptr<std::vector<uchar> > own_;
    static size_t esz(int type) { return type == CV_32F ? 4 : 1; }
    void rowchk(int y) const { if (y < 0 || (y >= rows && !(y == 0 && rows == 0))) throw Exception("Mat::ptr out of range"); }
    template <typename T> void chk(int y, int x) const {
        if (sizeof(T) != elemSize() || y < 0 || y >= rows || x < 0 || x >= cols) throw Exception("Mat::at out of range");
    }
};

class FileStorage;   // named by Vocabulary.h's YAML save / load declarations; nothing here defines or calls them
class FileNode;

enum { NORM_L1 = 2, NORM_L2 = 4 };
enum { THRESH_BINARY = 0 };

// norm of the difference, accumulated in double in element order (rows, then columns).  u8: integer |a - b|; f32: the float
// difference widened to double (L2: squared there), as OpenCV's normDiff kernels do before their own unrolling.
inline double norm(const Mat& a, const Mat& b, int normType) {
    if (a.rows != b.rows || a.cols != b.cols || a.type() != b.type() || a.empty()) throw Exception("norm: size / type mismatch");
    if (normType != NORM_L1 && normType != NORM_L2) throw Exception("norm: unsupported norm");
    double s = 0.0;
    for (int y = 0; y < a.rows; ++y) {
        if (a.type() == CV_8U) {
            const uchar *p = a.ptr(y), *q = b.ptr(y);
            for (int x = 0; x < a.cols; ++x) {
                const int d = (int)p[x] - (int)q[x];
                s += normType == NORM_L1 ? (double)(d < 0 ? -d : d) : (double)d * (double)d;
            }
        } else {
            const float *p = (const float*)a.ptr(y), *q = (const float*)b.ptr(y);
            for (int x = 0; x < a.cols; ++x) {
                const double d = (double)(p[x] - q[x]);
                s += normType == NORM_L1 ? std::fabs(d) : d * d;
            }
        }
    }
    return normType == NORM_L2 ? std::sqrt(s) : s;
}

// THRESH_BINARY on f32: dst = src > thresh ? maxval : 0 (a NaN compares false)
inline double threshold(const Mat& src, Mat& dst, double thresh, double maxval, int type) {
    if (type != THRESH_BINARY || src.type() != CV_32F) throw Exception("threshold: unsupported");
    dst = Mat(src.rows, src.cols, CV_32F);
    const float t = (float)thresh, mv = (float)maxval;
    for (int y = 0; y < src.rows; ++y)
        for (int x = 0; x < src.cols; ++x) dst.at<float>(y, x) = src.at<float>(y, x) > t ? mv : 0.0f;
    return thresh;
}

}  // namespace cv

// round to nearest, ties to even (the default rounding mode), as OpenCV's cvRound
inline int cvRound(double v) { return (int)lrint(v); }

#endif
