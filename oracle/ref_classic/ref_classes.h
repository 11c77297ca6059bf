// Just enough of Frame, SPmatcher, MapPoint, KeyFrame and SPextractor for the extracted Rover-SLAM function bodies to compile
// (oracle/ref_classic/build_ref.py).  Written for this project.  Member names and TYPES follow the reference's headers
// (include/Frame.h, include/MapPoint.h, include/Matchers/SPmatcher.h, include/Extractors/SPextractor.h): the arithmetic of the
// bodies depends on them, e.g. `double scaleFactor` makes mvScaleFactor[i-1]*scaleFactor a double product.
// With RFE_REF_BOW (ref_bow_main.cc) also the members KeyFrameDatabase's BoW bodies touch (include/KeyFrame.h, include/Frame.h,
// include/KeyFrameDatabase.h), over DBoW3's OWN headers, which build_ref.py puts on the include path from the checkout.
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
#ifdef RFE_REF_BOW
#include <list>
#include <set>
#include "BowVector.h"
#include "Vocabulary.h"
#endif

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
#ifdef RFE_REF_BOW
    DBoW3::BowVector mBow3Vec;
    long unsigned int mnId;
#endif
};

class KeyFrame {
public:
    KeyFrame() : bad(false) {}
    bool isBad() { return bad; }
    cv::Mat mDescriptors;
    bool bad;
#ifdef RFE_REF_BOW
    std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
    std::set<KeyFrame*> connected;     // the stand-in's own: what GetConnectedKeyFrames returns
    long unsigned int mnId;
    long unsigned int mnRelocQuery;
    int mnRelocWords;
    float mRelocScore;
    long unsigned int mnPlaceRecognitionQuery;
    int mnPlaceRecognitionWords;
    float mPlaceRecognitionScore;
    DBoW3::BowVector mBow3Vec;
#endif
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

#ifdef RFE_REF_BOW
typedef DBoW3::Vocabulary SPVocabulary;
class Map;

class KeyFrameDatabase {
public:
    // the reference sizes the inverted file by voc.size(); the scripts bring their own word range
    KeyFrameDatabase(const SPVocabulary& voc, size_t n_words) : mpVoc(&voc) { mvInvertedFile.resize(n_words); }
    void add(KeyFrame* pKF);
    void erase(KeyFrame* pKF);
    // what the two fronts leave behind when the cut range has run to its end (early == true: it returned inside the range)
    struct Front {
        bool early;
        int maxCommonWords, minCommonWords;
        std::list<KeyFrame*> sharing;
        std::list<std::pair<float, KeyFrame*> > scored;
        Front() : early(true), maxCommonWords(0), minCommonWords(0) {}
    };
    // body = DetectNBestCandidates_sp from its first declaration to the end of the scoring loop
    void FrontNBest_sp(KeyFrame* pKF, Front& front);
    // body = DetectRelocalizationCandidates from its first declaration to the end of the scoring loop
    std::vector<KeyFrame*> FrontReloc(Frame* F, Front& front);
    const SPVocabulary* mpVoc;
    std::vector<list<KeyFrame*> > mvInvertedFile;
    std::mutex mMutex;
};
#endif

}  // namespace ORB_SLAM3
#endif
