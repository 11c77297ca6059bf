// <opencv2/core/core.hpp> as DBoW3's headers ask for it: the project's own stand-in (oracle/ref_classic/cv_standin.h), no OpenCV text.
#include "../../cv_standin.h"
