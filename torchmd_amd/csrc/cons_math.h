// Constraint arithmetic of the constrained MD step (md_cons.hip: md_step_cons_kernel), in double in both precisions:
// analytic SETTLE for rigid waters (Miyamoto & Kollman 1992, in the form of GROMACS' settle), iterated SHAKE for X-H
// clusters, and the exact velocity constraint of a unit (its k x k linear system, k <= 4).  Host-callable, so that the
// formulas can be checked on a CPU.  A unit's atoms are local indices 0 .. NA-1; the constraints of a water are (0,1), (0,2),
// (1,2) (O-H1, O-H2, H1-H2), those of a cluster (0,c+1) (central atom, hydrogen c).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace tmd {

template <bool WATER>
struct ConsTopo {
  __host__ __device__ static constexpr int a(int c) { return WATER ? (c < 2 ? 0 : 1) : 0; }
  __host__ __device__ static constexpr int b(int c) { return WATER ? (c == 0 ? 1 : 2) : c + 1; }
};

__host__ __device__ inline double cdot(const double (&x)[3], const double (&y)[3]) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// Velocity constraint (RATTLE's second half): v += sum_c mu_c sigma r_c / m such that r_c . (v_a - v_b) = 0 for every
// constraint c of the unit at positions p.  The conditions are linear in mu: A mu = -b with the symmetric positive definite
// A_cd = (r_c . r_d) ([a_c = a_d] - [a_c = b_d]) / m_{a_c} - ([b_c = a_d] - [b_c = b_d]) / m_{b_c}), solved exactly.
template <int NA, int NC, bool WATER>
__host__ __device__ inline void cons_velocities(const double (&p)[NA][3], double (&v)[NA][3], const double (&im)[NA]) {
  using T = ConsTopo<WATER>;
  double r[NC][3], A[NC][NC], mu[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double dv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r[c][k] = p[T::a(c)][k] - p[T::b(c)][k];
      dv[k] = v[T::a(c)][k] - v[T::b(c)][k];
    }
    mu[c] = -cdot(r[c], dv);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int d = 0; d < NC; ++d) {
      const double sa = (T::a(c) == T::a(d) ? 1.0 : 0.0) - (T::a(c) == T::b(d) ? 1.0 : 0.0);
      const double sb = (T::b(c) == T::a(d) ? 1.0 : 0.0) - (T::b(c) == T::b(d) ? 1.0 : 0.0);
      A[c][d] = cdot(r[c], r[d]) * (sa * im[T::a(c)] - sb * im[T::b(c)]);
    }
  // Gaussian elimination without pivoting (A is symmetric positive definite)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double inv = 1.0 / A[c][c];
#pragma unroll
    for (int d = c + 1; d < NC; ++d) {
      const double f = A[d][c] * inv;
#pragma unroll
      for (int e = c; e < NC; ++e) A[d][e] -= f * A[c][e];
      mu[d] -= f * mu[c];
    }
  }
#pragma unroll
  for (int c = NC - 1; c >= 0; --c) {
#pragma unroll
    for (int e = c + 1; e < NC; ++e) mu[c] -= A[c][e] * mu[e];
    mu[c] /= A[c][c];
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v[T::a(c)][k] += mu[c] * r[c][k] * im[T::a(c)];
      v[T::b(c)][k] -= mu[c] * r[c][k] * im[T::b(c)];
    }
}

// Iterated SHAKE of a cluster (central atom 0, hydrogens 1 .. NA-1) along the bond vectors of `ref`; true once every
// |d^2 - s^2| <= 2 tol d^2 (relative bond-length error tol).  false: not converged within max_iter sweeps.
template <int NA>
__host__ __device__ inline bool shake_cluster(const double (&ref)[NA][3], double (&x)[NA][3], const double (&im)[NA],
                                              const double (&d)[NA], double tol, int max_iter) {
  for (int it = 0; it < max_iter; ++it) {
    bool done = true;
#pragma unroll
    for (int h = 1; h < NA; ++h) {
      double s[3], r[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        s[k] = x[0][k] - x[h][k];
        r[k] = ref[0][k] - ref[h][k];
      }
      const double d2 = d[h] * d[h], diff = d2 - cdot(s, s);
      if (fabs(diff) <= 2.0 * tol * d2) continue;
      done = false;
      const double g = diff / (2.0 * cdot(r, s) * (im[0] + im[h]));
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        x[0][k] += g * r[k] * im[0];
        x[h][k] -= g * r[k] * im[h];
      }
    }
    if (done) return true;
  }
  return false;
}

// Analytic SETTLE: moves the unconstrained new positions xp (O, H1, H2) onto the rigid geometry (d_OH, d_HH) so that the
// displacement is along the constraint forces of the old positions b4, keeping the centre of mass.  false: the molecule
// was too distorted for the closed form (the result is then unreliable).
__host__ __device__ inline bool settle_water(const double (&b4)[3][3], double (&xp)[3][3], double mO, double mH, double dOH,
                                             double dHH) {
  const double wohh = mO + 2.0 * mH, wh = mH / wohh;
  const double rc = 0.5 * dHH, h = sqrt(dOH * dOH - rc * rc);
  const double ra = 2.0 * mH * h / wohh, rb = h - ra, irc2 = 1.0 / dHH;
  double dist21[3], dist31[3], doh2[3], doh3[3], a1[3], b1[3], c1[3], com[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    dist21[k] = b4[1][k] - b4[0][k];
    dist31[k] = b4[2][k] - b4[0][k];
    doh2[k] = xp[1][k] - xp[0][k];
    doh3[k] = xp[2][k] - xp[0][k];
    // (the centre of mass from the O-H vectors, not from the absolute positions: GROMACS found the latter the largest
    // source of energy drift in water, the oxygen coordinate scaled by 0.89 every step)
    a1[k] = -(doh2[k] + doh3[k]) * wh;
    com[k] = xp[0][k] - a1[k];
    b1[k] = xp[0][k] + doh2[k] - com[k];
    c1[k] = xp[0][k] + doh3[k] - com[k];
  }
  const double xakszd = dist21[1] * dist31[2] - dist21[2] * dist31[1];
  const double yakszd = dist21[2] * dist31[0] - dist21[0] * dist31[2];
  const double zakszd = dist21[0] * dist31[1] - dist21[1] * dist31[0];
  const double xaksxd = a1[1] * zakszd - a1[2] * yakszd;
  const double yaksxd = a1[2] * xakszd - a1[0] * zakszd;
  const double zaksxd = a1[0] * yakszd - a1[1] * xakszd;
  const double xaksyd = yakszd * zaksxd - zakszd * yaksxd;
  const double yaksyd = zakszd * xaksxd - xakszd * zaksxd;
  const double zaksyd = xakszd * yaksxd - yakszd * xaksxd;
  const double axlng = 1.0 / sqrt(xaksxd * xaksxd + yaksxd * yaksxd + zaksxd * zaksxd);
  const double aylng = 1.0 / sqrt(xaksyd * xaksyd + yaksyd * yaksyd + zaksyd * zaksyd);
  const double azlng = 1.0 / sqrt(xakszd * xakszd + yakszd * yakszd + zakszd * zakszd);
  // rows of the rotation into the molecule's frame: trns[d] = axis d (x, y, z)
  const double t1[3] = {xaksxd * axlng, xaksyd * aylng, xakszd * azlng};
  const double t2[3] = {yaksxd * axlng, yaksyd * aylng, yakszd * azlng};
  const double t3[3] = {zaksxd * axlng, zaksyd * aylng, zakszd * azlng};
  double b0d[2], c0d[2], b1d[3], c1d[3];
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    b0d[d] = t1[d] * dist21[0] + t2[d] * dist21[1] + t3[d] * dist21[2];
    c0d[d] = t1[d] * dist31[0] + t2[d] * dist31[1] + t3[d] * dist31[2];
  }
  const double a1d_z = t1[2] * a1[0] + t2[2] * a1[1] + t3[2] * a1[2];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    b1d[d] = t1[d] * b1[0] + t2[d] * b1[1] + t3[d] * b1[2];
    c1d[d] = t1[d] * c1[0] + t2[d] * c1[1] + t3[d] * c1[2];
  }
  const double sinphi = a1d_z / ra;
  double tmp2 = 1.0 - sinphi * sinphi;
  const bool ok = tmp2 > 1e-12;
  if (!ok) tmp2 = 1e-12;
  const double cosphi = sqrt(tmp2);
  const double sinpsi = (b1d[2] - c1d[2]) * irc2 / cosphi;
  const double cospsi = sqrt(1.0 - sinpsi * sinpsi);
  const double a2d_y = ra * cosphi, b2d_x = -rc * cospsi;
  const double tt1 = -rb * cosphi, tt2 = rc * sinpsi * sinphi;
  const double b2d_y = tt1 - tt2, c2d_y = tt1 + tt2;
  const double alpha = b2d_x * (b0d[0] - c0d[0]) + b0d[1] * b2d_y + c0d[1] * c2d_y;
  const double beta = b2d_x * (c0d[1] - b0d[1]) + b0d[0] * b2d_y + c0d[0] * c2d_y;
  const double gamma = b0d[0] * b1d[1] - b1d[0] * b0d[1] + c0d[0] * c1d[1] - c1d[0] * c0d[1];
  const double al2be2 = alpha * alpha + beta * beta;
  const double sinthe = (alpha * gamma - beta * sqrt(al2be2 - gamma * gamma)) / al2be2;
  const double costhe = sqrt(1.0 - sinthe * sinthe);
  const double a3d[3] = {-a2d_y * sinthe, a2d_y * costhe, a1d_z};
  const double b3d[3] = {b2d_x * costhe - b2d_y * sinthe, b2d_x * sinthe + b2d_y * costhe, b1d[2]};
  const double c3d[3] = {-b2d_x * costhe - c2d_y * sinthe, -b2d_x * sinthe + c2d_y * costhe, c1d[2]};
  const double *tr[3] = {t1, t2, t3};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    xp[0][k] = com[k] + (tr[k][0] * a3d[0] + tr[k][1] * a3d[1] + tr[k][2] * a3d[2]);
    xp[1][k] = com[k] + (tr[k][0] * b3d[0] + tr[k][1] * b3d[1] + tr[k][2] * b3d[2]);
    xp[2][k] = com[k] + (tr[k][0] * c3d[0] + tr[k][1] * c3d[1] + tr[k][2] * c3d[2]);
  }
  return ok && al2be2 - gamma * gamma >= 0.0;
}

}  // namespace tmd
