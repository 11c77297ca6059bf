// <boost/serialization/map.hpp> as DBoW3's headers ask for it: nothing of it is used by what the harness compiles.
#include "serialization.hpp"
