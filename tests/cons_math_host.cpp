// Host build of torchmd_amd/csrc/cons_math.h for tests/test_cons_math_host.py: the arithmetic of the constrained MD step
// (settle_water, shake_cluster<2..5>, cons_velocities) behind a plain C interface, compiled with the system C++ compiler
// and -ffp-contract=off (the kernel's `#pragma clang fp contract(off)`).  Arrays are row-major doubles, [atoms][3].
#include "cons_math.h"

namespace {

template <int NA>
void load(const double *src, double (&dst)[NA][3]) {
  for (int j = 0; j < NA; ++j)
    for (int k = 0; k < 3; ++k) dst[j][k] = src[3 * j + k];
}

template <int NA>
void store(const double (&src)[NA][3], double *dst) {
  for (int j = 0; j < NA; ++j)
    for (int k = 0; k < 3; ++k) dst[3 * j + k] = src[j][k];
}

template <int NA>
int shake(const double *ref, double *x, const double *im, const double *d, double tol, int max_iter) {
  double r[NA][3], y[NA][3], w[NA], len[NA];
  load<NA>(ref, r);
  load<NA>(x, y);
  for (int j = 0; j < NA; ++j) {
    w[j] = im[j];
    len[j] = d[j];
  }
  const bool ok = tmd::shake_cluster<NA>(r, y, w, len, tol, max_iter);
  store<NA>(y, x);
  return ok ? 1 : 0;
}

template <int NA, int NC, bool WATER>
void velocities(const double *p, double *v, const double *im) {
  double q[NA][3], u[NA][3], w[NA];
  load<NA>(p, q);
  load<NA>(v, u);
  for (int j = 0; j < NA; ++j) w[j] = im[j];
  tmd::cons_velocities<NA, NC, WATER>(q, u, w);
  store<NA>(u, v);
}

}  // namespace

extern "C" {

// xp [3][3] in place; 1 = settle_water returned true
int cm_settle(const double *b4, double *xp, double mO, double mH, double dOH, double dHH) {
  double r[3][3], y[3][3];
  load<3>(b4, r);
  load<3>(xp, y);
  const bool ok = tmd::settle_water(r, y, mO, mH, dOH, dHH);
  store<3>(y, xp);
  return ok ? 1 : 0;
}

// x [na][3] in place (na = 2 .. 5; d[0] unused); 1 = converged, 0 = not, -1 = na out of range
int cm_shake(int na, const double *ref, double *x, const double *im, const double *d, double tol, int max_iter) {
  switch (na) {
    case 2: return shake<2>(ref, x, im, d, tol, max_iter);
    case 3: return shake<3>(ref, x, im, d, tol, max_iter);
    case 4: return shake<4>(ref, x, im, d, tol, max_iter);
    case 5: return shake<5>(ref, x, im, d, tol, max_iter);
  }
  return -1;
}

// v [na][3] in place: the cluster form with na - 1 constraints (na = 2 .. 5), or the water form (water != 0, na = 3)
int cm_velocities(int na, int water, const double *p, double *v, const double *im) {
  if (water) {
    if (na != 3) return -1;
    velocities<3, 3, true>(p, v, im);
    return 0;
  }
  switch (na) {
    case 2: velocities<2, 1, false>(p, v, im); return 0;
    case 3: velocities<3, 2, false>(p, v, im); return 0;
    case 4: velocities<4, 3, false>(p, v, im); return 0;
    case 5: velocities<5, 4, false>(p, v, im); return 0;
  }
  return -1;
}
}
