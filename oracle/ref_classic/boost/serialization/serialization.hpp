// <boost/serialization/serialization.hpp> as DBoW3's BowVector.h / FeatureVector.h ask for it.  Written for this project: only the two
// names their never-instantiated serialize() templates mention.
#ifndef RFE_REF_BOOST_SERIALIZATION_STANDIN_H
#define RFE_REF_BOOST_SERIALIZATION_STANDIN_H
// the standard headers DBoW3's headers lean on Boost to bring in
#include <cstddef>
#include <cstdint>
#include <istream>
#include <ostream>
#include <string>
namespace boost {
namespace serialization {
class access;
template <class Base, class Derived> Base& base_object(Derived& d) { return static_cast<Base&>(d); }
}  // namespace serialization
}  // namespace boost
#endif
