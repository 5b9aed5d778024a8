// The scale factor of the stochastic velocity-rescaling thermostat (Bussi, Donadio & Parrinello, J. Chem. Phys. 126, 014101,
// 2007, eq. A7), shared by the update kernel of thermostat.hip and a host program (tests/thermostat_math_host.cpp), in double.
// Compile with floating-point contraction off: the order of the operations below is the contract.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace tmd {

// K: kinetic energy now; kbar = N_f k_B T / 2: its target; nf = N_f; c = exp(-dt / tau) in [0, 1]; r1: a standard normal;
// s: a chi-squared variate with N_f - 1 degrees of freedom.  Returns alpha >= 0 with K_new = alpha^2 K:
//   alpha^2 = c + (1 - c) kbar (r1^2 + s) / (nf K) + 2 r1 sqrt(c (1 - c) kbar / (nf K))
// K = 0 (or not a positive number): 1, nothing to scale.  c = 1: exactly 1.  c = 0: K_new = (kbar / nf) (r1^2 + s) whatever K was.
// alpha^2 is a perfect square, (sqrt(c) + r1 sqrt((1 - c) kbar / (nf K)))^2, plus a non-negative term, so it can be negative
// by rounding only: clamped at 0.
__host__ __device__ inline double csvr_alpha(double K, double kbar, double nf, double c, double r1, double s) {
  if (!(K > 0.0)) return 1.0;
  const double nk = nf * K;
  const double a2 = c + ((1.0 - c) * kbar * (r1 * r1 + s)) / nk + 2.0 * r1 * sqrt((c * (1.0 - c) * kbar) / nk);
  return sqrt(a2 > 0.0 ? a2 : 0.0);
}

// Kinetic energy of the velocities with the centre-of-mass velocity taken out, from the sums over the massive atoms:
// K = (1/2) sum m v^2 - (1/2) (sum m) V_cm^2 with V_cm = sum m v / sum m (vcm[] on return; zero when `remove_com` is off or
// there is no mass).  Never negative.
__host__ __device__ inline double csvr_kinetic(double sm, double px, double py, double pz, double mv2, int remove_com, double (&vcm)[3]) {
  vcm[0] = vcm[1] = vcm[2] = 0.0;
  double K = 0.5 * mv2;
  if (remove_com && sm > 0.0) {
    vcm[0] = px / sm, vcm[1] = py / sm, vcm[2] = pz / sm;
    K = K - 0.5 * sm * (vcm[0] * vcm[0] + vcm[1] * vcm[1] + vcm[2] * vcm[2]);
  }
  return K > 0.0 ? K : 0.0;
}

}  // namespace tmd
