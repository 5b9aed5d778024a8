// Stochastic cell rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107, 2020; GROMACS' pcoupl = C-rescale): the step of
// eps = ln V and the rigid shift of one molecule, shared by the kernels of crescale.hip and a host program
// (tests/crescale_math_host.cpp).  Compile with floating-point contraction off: the order of the operations below is the
// contract.
//
//   d eps = -(beta dt_p / tau_p) (P0 - P_int) + sqrt(2 kT beta dt_p / (V tau_p)) xi        mu = exp(d eps / 3)
// with beta the isothermal compressibility, dt_p the time between two applications, tau_p the relaxation time, P_int the
// instantaneous molecular pressure (virial.hip), xi a standard normal.  Without the noise term it is the Berendsen barostat.
// Energies in kcal/mol, volumes in A^3, pressures in kcal/mol/A^3, beta in A^3 mol/kcal; dt_over_tau = dt_p / tau_p.
// The kernels use the shift, the store and m v^2; the factor itself is formed on the host once per replica (Python:
// crescale.delta_epsilon, the same operations in the same order) — crescale_delta_eps / crescale_mu state it for C callers of
// tmdhip_rescale_molecules and are held to the same model by the host test.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace tmd {

__host__ __device__ inline double crescale_delta_eps(double beta, double dt_over_tau, double p0, double pint, double kT, double vol,
                                                     double xi, int stochastic) {
#pragma clang fp contract(off)
  const double drift = -(beta * dt_over_tau) * (p0 - pint);
  if (!stochastic) return drift;
  return drift + sqrt(((2.0 * kT) * (beta * dt_over_tau)) / vol) * xi;
}

// the factor of every box edge
__host__ __device__ inline double crescale_mu(double delta_eps) { return exp(delta_eps / 3.0); }

// A molecule follows a box edge that is multiplied by s: every atom is translated by (s - 1) R_a and every velocity by
// (1 / s - 1) V_a, with R = sum m x / sum m and V = sum m v / sum m the mass-weighted centre and its velocity.  sum_m > 0.
__host__ __device__ inline double crescale_shift_pos(double s, double sum_mx, double sum_m) {
#pragma clang fp contract(off)
  return (s - 1.0) * (sum_mx / sum_m);
}

__host__ __device__ inline double crescale_shift_vel(double s, double sum_mv, double sum_m) {
#pragma clang fp contract(off)
  return (1.0 / s - 1.0) * (sum_mv / sum_m);
}

// x + shift, rounded once to the storage precision
template <typename R>
__host__ __device__ inline R crescale_apply(R x, double shift) {
#pragma clang fp contract(off)
  return (R)((double)x + shift);
}

// m v^2 of one atom (twice its kinetic energy; the fold halves the sum)
__host__ __device__ inline double crescale_mv2(double m, double vx, double vy, double vz) {
#pragma clang fp contract(off)
  return m * ((vx * vx + vy * vy) + vz * vz);
}

}  // namespace tmd
