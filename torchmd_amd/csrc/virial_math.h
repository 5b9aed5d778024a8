// Molecular virial: the contribution of one pair seen from one of its atoms, and the validation of the molecule table, shared by
// the kernels of virial.hip and a host program (tests/virial_math_host.cpp).  Compile with floating-point contraction off: the
// order of the operations below is the contract.
//
//   W_aa = 1/2 sum_i sum_{j in list(i)} d_ij,a f_ij,a  -  sum_i delta_i,a F_i,a        (a = x, y, z)
// with d_ij the engine's minimum-image vector, f_ij = -d_ij fs the force on i (fs = pair_terms' return value) and
// delta_i = r_i - R_I(i) the atom's offset from the mass-weighted centre of its molecule.  Both sums are linear in the pair
// force, so every (i, j) visit adds f_a (d_a / 2 - delta_i,a): no force array, no sum of forces across lanes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tmd {

// w[a] += f_a (d_a / 2 - delta_a), f_a = -(d_a fs) rounded in the engine's precision R as the pair kernels form it, everything
// after that in double
template <typename R>
__host__ __device__ inline void virial_pair(R dx, R dy, R dz, R fs, const double *delta, double *w) {
#pragma clang fp contract(off)
  const R fx = -(dx * fs), fy = -(dy * fs), fz = -(dz * fs);
  w[0] += (double)fx * (0.5 * (double)dx - delta[0]);
  w[1] += (double)fy * (0.5 * (double)dy - delta[1]);
  w[2] += (double)fz * (0.5 * (double)dz - delta[2]);
}

// Reciprocal-space PME (Essmann et al. 1995, eq. 2.20) with the grid and beta fixed: a mode of energy e(m) = w_z G(m) |S(m)|^2 / 2
// contributes e(m) [1 - 2 (1 + pi^2 m^2 / beta^2) m_a^2 / m^2] to W_aa under an affine scaling of the box edge a (G ~ exp(-pi^2
// m^2 / beta^2) / (V m^2) with m_a ~ 1 / L_a).  m2 = |m|^2 > 0 and ma2 = m_a^2 in 1 / A^2.
__host__ __device__ inline double virial_mode_factor(double m2, double ma2, double beta) {
#pragma clang fp contract(off)
  const double pi2 = 9.869604401089358;
  return 1.0 - 2.0 * (1.0 + pi2 * m2 / (beta * beta)) * ma2 / m2;
}

// P_aa V and the scalar pressure from the two halves: out[8] = (sum M V_a^2 [3], W_aa [3], V, P)
__host__ __device__ inline void virial_finish(const double *kin, const double *w, const double *box, double *out) {
#pragma clang fp contract(off)
  const double vol = (box[0] * box[1]) * box[2];
  for (int a = 0; a < 3; ++a) out[a] = kin[a], out[3 + a] = w[a];
  out[6] = vol;
  out[7] = (((kin[0] + w[0]) + (kin[1] + w[1])) + (kin[2] + w[2])) / (3.0 * vol);
}

}  // namespace tmd

// ---- host side: the molecule table ----
#include <string>
#include <vector>

namespace tmd {

// "" when offsets / members are a CSR of nmol non-empty molecules that covers each of the natoms atoms exactly once;
// mol_of[natoms] receives the molecule of every atom
inline std::string virial_validate_molecules(int64_t natoms, int64_t nmol, const int32_t *offsets, const int32_t *members,
                                             std::vector<int32_t> &mol_of) {
  if (nmol <= 0 || nmol > natoms) return "the number of molecules must lie in 1 .. natoms";
  if (!offsets || !members) return "null molecule table";
  if (offsets[0] != 0 || offsets[nmol] != natoms) return "the molecule offsets must run from 0 to natoms";
  mol_of.assign((size_t)natoms, -1);
  for (int64_t m = 0; m < nmol; ++m) {
    if (offsets[m + 1] <= offsets[m]) return "molecule " + std::to_string(m) + " is empty (or the offsets decrease)";
    if (offsets[m + 1] > natoms) return "molecule offsets out of range";
    for (int32_t k = offsets[m]; k < offsets[m + 1]; ++k) {
      const int32_t a = members[k];
      if (a < 0 || a >= natoms) return "molecule " + std::to_string(m) + ": atom index " + std::to_string(a) + " out of range";
      if (mol_of[a] >= 0) return "atom " + std::to_string(a) + " is in two molecules";
      mol_of[a] = (int32_t)m;
    }
  }
  return "";
}

}  // namespace tmd
