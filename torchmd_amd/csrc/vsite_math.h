// Linear virtual sites (tmdhip_vsite_construct / _spread, the constrained MD step): the two expressions every kernel that
// places a site or hands its force on shares, so that a site placed inside md_step_cons_kernel and one placed by the
// stateless kernel from the same stored parents have the same bits.  Double in both precisions, one rounding on the store.
#pragma once

#include "common.h"

namespace tmd {

// one coordinate of a site: w0 p0 + w1 p1 (+ w2 p2), parents in table order
template <typename R>
__device__ __forceinline__ R vsite_coord(double w0, double w1, double w2, R p0, R p1, R p2, bool three) {
#pragma clang fp contract(off)
  double s = w0 * (double)p0;
  s = s + w1 * (double)p1;
  if (three) s = s + w2 * (double)p2;
  return (R)s;
}

// one force component of a parent after the site's share has been added
template <typename R>
__device__ __forceinline__ R vsite_share(R f_parent, double w, R f_site) {
#pragma clang fp contract(off)
  return (R)((double)f_parent + w * (double)f_site);
}

}  // namespace tmd
