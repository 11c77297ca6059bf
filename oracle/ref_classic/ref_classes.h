// Just enough of Frame, SPmatcher, MapPoint, KeyFrame and SPextractor for the extracted Rover-SLAM function bodies to compile
// (oracle/ref_classic/build_ref.py).  Written for this project.  Member names and TYPES follow the reference's headers
// (include/Frame.h, include/MapPoint.h, include/Matchers/SPmatcher.h, include/Extractors/SPextractor.h): the arithmetic of the
// bodies depends on them, e.g. `double scaleFactor` makes mvScaleFactor[i-1]*scaleFactor a double product.
#ifndef RFE_REF_CLASSES_H
#define RFE_REF_CLASSES_H
#include <algorithm>
#include <climits>
#include <cmath>
#include <iostream>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>
#include "cv_standin.h"

namespace ORB_SLAM3 {
using namespace std;   // the reference's sources see std through their headers

class SPmatcher {
public:
    static const float TH_LOW;
    static const float TH_HIGH;
    static float DescriptorDistance_sp(const cv::Mat& a, const cv::Mat& b);
};

class Frame {
public:
    void ComputeStereoMatches();
    void binarize_descriptors();
    float mbf;
    float mb;
    int N;
    std::vector<cv::KeyPoint> mvKeys, mvKeysRight;
    std::vector<float> mvuRight;
    std::vector<float> mvDepth;
    cv::Mat mDescriptors, mDescriptorsRight;
    cv::Mat mDescriptors_bin;
    vector<float> mvScaleFactors;
    vector<float> mvInvScaleFactors;
    cv::Mat imgLeft, imgRight;
};

class KeyFrame {
public:
    KeyFrame() : bad(false) {}
    bool isBad() { return bad; }
    cv::Mat mDescriptors;
    bool bad;
};

class MapPoint {
public:
    MapPoint() : mbBad(false) {}
    void ComputeDistinctiveDescriptors();
    std::map<KeyFrame*, std::tuple<int, int> > mObservations;
    cv::Mat mDescriptor;
    bool mbBad;
    std::mutex mMutexFeatures;
};

class SPextractor {
public:
    // the constructor's signature types: (int nfeatures, float scaleFactor, int nlevels, ...) stored in int / double / int members
    SPextractor(int _nfeatures, float _scaleFactor, int _nlevels) : nfeatures(_nfeatures), scaleFactor(_scaleFactor), nlevels(_nlevels) {
        InitScales();
        InitFeaturesPerLevel();
    }
    void InitScales();             // body = the constructor fragment mvScaleFactor.resize .. (before) mvImagePyramid.resize
    void InitFeaturesPerLevel();   // body = the constructor fragment mnFeaturesPerLevel.resize .. end of the constructor
    cv::Size LevelSize(cv::Mat image, int level);   // body = the two level-size lines of ComputePyramid
    int nfeatures;
    double scaleFactor;
    int nlevels;
    std::vector<int> mnFeaturesPerLevel;
    std::vector<float> mvScaleFactor;
    std::vector<float> mvInvScaleFactor;
    std::vector<float> mvLevelSigma2;
    std::vector<float> mvInvLevelSigma2;
};

}  // namespace ORB_SLAM3
#endif
