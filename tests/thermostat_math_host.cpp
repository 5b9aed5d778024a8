// Host build of torchmd_amd/csrc/thermostat_math.h for tests/test_thermostat_host.py: the scale factor of the velocity-rescaling
// thermostat behind a plain C interface, compiled with the system C++ compiler and -ffp-contract=off (the kernel's
// `#pragma clang fp contract(off)`).
#include "thermostat_math.h"

extern "C" {

double tm_alpha(double K, double kbar, double nf, double c, double r1, double s) { return tmd::csvr_alpha(K, kbar, nf, c, r1, s); }

// sums = {sum m, sum m vx, sum m vy, sum m vz, sum m v^2}; vcm [3] out; returns K
double tm_kinetic(const double *sums, int remove_com, double *vcm) {
  double v[3];
  const double K = tmd::csvr_kinetic(sums[0], sums[1], sums[2], sums[3], sums[4], remove_com, v);
  for (int k = 0; k < 3; ++k) vcm[k] = v[k];
  return K;
}
}
