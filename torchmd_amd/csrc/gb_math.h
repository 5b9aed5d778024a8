// Generalized-Born implicit solvent (OBC2, Onufriev-Bashford-Case 2004) with the ACE-type surface-area term: the per-pair
// functions of the three pair passes and the per-atom closes, shared by the kernels of gb.hip and a host program
// (tests/gb_math_host.cpp).  Plain C++ templated on the real type R of the pair arithmetic; the per-atom closes are double.
//
//   rho_i = r_i - 0.09, sigma_j = s_j rho_j.  No minimum image, no cutoff, no exclusions: every ordered pair i != j.
//   pass 1  I_i = (1/2) sum_j t(r_ij, rho_i, sigma_j);  psi = rho I;  T = tanh(psi - 0.8 psi^2 + 4.85 psi^3);
//           B = 1 / (1/rho - T/r);  c = rho (1 - 1.6 psi + 14.55 psi^2)(1 - T^2) / r  (= (dB/dI) / B^2)
//   pass 2  G_ij = p q_i q_j / f, f^2 = r^2 + B_i B_j e^-D, D = r^2 / (4 B_i B_j);  E_GB = (1/2) sum_ij G_ij (i = j included)
//           F_i += g_ij (x_j - x_i), g = -G (1 - e^-D / 4) / f^2;  b_i = sum_j h_ij B_j, h = -(1/2) G e^-D (1 + D) / f^2
//           E_SA,i = sa_i (r_i / B_i)^6;  b_i <- (b_i - 6 E_SA,i / B_i) B_i^2 c_i  (= dE/dI_i)
//   pass 3  F_i += [b_i t3(r, rho_i, sigma_j) + b_j t3(r, rho_j, sigma_i)] (x_i - x_j) / r,  t3 = -(dt/dr) / 2
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace tmd {

constexpr double kGbOffset = 0.09;  // rho = r - 0.09 A

__host__ __device__ inline float gb_log(float x) { return logf(x); }
__host__ __device__ inline double gb_log(double x) { return log(x); }
__host__ __device__ inline float gb_exp(float x) { return expf(x); }
__host__ __device__ inline double gb_exp(double x) { return exp(x); }
__host__ __device__ inline float gb_sqrt(float x) { return sqrtf(x); }
__host__ __device__ inline double gb_sqrt(double x) { return sqrt(x); }
__host__ __device__ inline float gb_abs(float x) { return fabsf(x); }
__host__ __device__ inline double gb_abs(double x) { return fabs(x); }

// The descreening integral of atom j over atom i (r > 0).  Three regimes: separate (rho_i <= r - sigma_j: l = 1/(r - sigma_j)),
// overlapping (l = 1/rho_i) and engulfed (rho_i < sigma_j - r: l = 1/(sigma_j - r) and the extra 2 (1/rho_i - l)); atom j out of
// reach of i's sphere from inside (rho_i >= r + sigma_j) gives 0.
template <typename R>
__host__ __device__ inline R gb_pair_t(R r, R rho_i, R sig_j) {
  if (!(rho_i < r + sig_j)) return R(0);
  const R a = gb_abs(r - sig_j);
  const R l = R(1) / (rho_i > a ? rho_i : a), u = R(1) / (r + sig_j);
  const R l2 = l * l, u2 = u * u, rinv = R(1) / r;
  R t = l - u + R(0.25) * r * (u2 - l2) + R(0.5) * rinv * gb_log(u / l) + R(0.25) * sig_j * sig_j * rinv * (l2 - u2);
  if (rho_i < sig_j - r) t += R(2) * (R(1) / rho_i - l);
  return t;
}

// -(dt/dr) / 2 of gb_pair_t, in every regime
template <typename R>
__host__ __device__ inline R gb_pair_t3(R r, R rho_i, R sig_j) {
  if (!(rho_i < r + sig_j)) return R(0);
  const R a = gb_abs(r - sig_j);
  const R l = R(1) / (rho_i > a ? rho_i : a), u = R(1) / (r + sig_j);
  const R l2 = l * l, u2 = u * u, rinv = R(1) / r, r2inv = rinv * rinv;
  return R(0.125) * (R(1) + sig_j * sig_j * r2inv) * (l2 - u2) + R(0.25) * gb_log(u / l) * r2inv;
}

// G_ij and its two derivatives from r^2 (0: the self term, G = pqq / B_i), pqq = p q_i q_j, B_i, B_j
template <typename R>
struct GbPair {
  R G;  // the pair energy (counted with weight 1/2 per ordered pair)
  R g;  // F_i += g (x_j - x_i)
  R h;  // b_i += h B_j
};
template <typename R>
__host__ __device__ inline GbPair<R> gb_pair_energy(R r2, R pqq, R Bi, R Bj) {
  const R BB = Bi * Bj, D = r2 / (R(4) * BB), e = gb_exp(-D);
  const R f2 = r2 + BB * e, finv = R(1) / gb_sqrt(f2), if2 = finv * finv;
  GbPair<R> o;
  o.G = pqq * finv;
  o.g = -o.G * (R(1) - R(0.25) * e) * if2;
  o.h = R(-0.5) * o.G * e * (R(1) + D) * if2;
  return o;
}

// close of pass 1: I = (1/2) sum t  ->  B and c
__host__ __device__ inline void gb_close_born(double I, double radius, double &B, double &c) {
  const double rho = radius - kGbOffset, psi = rho * I;
  const double T = tanh(psi - 0.8 * psi * psi + 4.85 * psi * psi * psi);
  B = 1.0 / (1.0 / rho - T / radius);
  c = rho * (1.0 - 1.6 * psi + 14.55 * psi * psi) * (1.0 - T * T) / radius;
}

// close of pass 2: the surface-area energy E_SA,i (returned) and b_i <- (b_i - 6 E_SA,i / B_i) B_i^2 c_i; sa = 4 pi gamma (r + r_probe)^2
__host__ __device__ inline double gb_close_chain(double bsum, double radius, double sa, double B, double c, double &b) {
  const double q = radius / B, q2 = q * q, esa = sa * (q2 * q2 * q2);
  b = (bsum - 6.0 * esa / B) * (B * B) * c;
  return esa;
}

}  // namespace tmd
