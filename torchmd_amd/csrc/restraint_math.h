// Harmonic position and distance restraints: energy and force of one entry, shared by the kernel of restraint.hip and a host
// program (tests/restraint_math_host.cpp), in double.  Compile with floating-point contraction off: the order of the operations
// below is the contract.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace tmd {

// d <- minimum image of d in the orthorhombic box (edge lengths); an edge of zero: no image along that axis
__host__ __device__ inline void restraint_min_image(double (&d)[3], const double *box) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k)
    if (box[k] != 0.0) d[k] = d[k] - box[k] * rint(d[k] / box[k]);
}

// Position restraint: d = minimum image of x - ref, E = (1/2) k |d|^2, F = -k d.  Returns E.
__host__ __device__ inline double restraint_position(const double *x, const double *ref, const double *box, double k, double (&f)[3]) {
#pragma clang fp contract(off)
  double d[3] = {x[0] - ref[0], x[1] - ref[1], x[2] - ref[2]};
  restraint_min_image(d, box);
  for (int c = 0; c < 3; ++c) f[c] = -k * d[c];
  return 0.5 * k * ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// Distance restraint: d = minimum image of xi - xj, r = |d|, E = (1/2) k (r - r0)^2 (the bond term with k0 = k / 2),
// F_i = -k (r - r0) d / r = -F_j (fi on return).  r = 0: no direction, F = 0 and E = (1/2) k r0^2.  Returns E.
__host__ __device__ inline double restraint_distance(const double *xi, const double *xj, const double *box, double k, double r0,
                                                     double (&fi)[3]) {
#pragma clang fp contract(off)
  double d[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  restraint_min_image(d, box);
  const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  const double x = r - r0;
  if (r > 0.0) {
    const double s = (-k * x) / r;
    for (int c = 0; c < 3; ++c) fi[c] = s * d[c];
  } else {
    fi[0] = fi[1] = fi[2] = 0.0;
  }
  return 0.5 * k * (x * x);
}

// One entry of a restrained atom's row: a position restraint (kind 0: `index` into the position tables, partner = -1,
// sign = 0) or one end of a distance restraint (kind 1: `index` into the distance tables, `partner` the other atom, sign = +1
// for the first atom of the pair, whose force is F_i, and -1 for the second).
struct RestraintEntry {
  int32_t kind, index, partner, sign;
};

}  // namespace tmd

// ---- host side: validation and the per-atom rows ----
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace tmd {

// What tmdhip_set_restraints refuses in the tables themselves ("" = nothing).  Real arrays as in tmdhip_restraint_desc.
inline std::string restraint_validate(int64_t natoms, int64_t nrep, int64_t npos, int64_t ndist, const int32_t *pos_atom,
                                      const double *pos_ref, const double *pos_k, const int32_t *dist_pair, const double *dist_r0,
                                      const double *dist_k) {
  if (natoms <= 0 || nrep <= 0 || npos < 0 || ndist < 0) return "bad size";
  if (npos > 0 && (!pos_atom || !pos_ref || !pos_k)) return "null position table";
  if (ndist > 0 && (!dist_pair || !dist_r0 || !dist_k)) return "null distance table";
  std::vector<char> seen((size_t)natoms, 0);
  for (int64_t p = 0; p < npos; ++p) {
    const int32_t a = pos_atom[p];
    if (a < 0 || a >= natoms) return "position restraint " + std::to_string(p) + ": atom index out of range";
    if (seen[a]) return "position restraint " + std::to_string(p) + ": a second position entry for atom " + std::to_string(a);
    seen[a] = 1;
  }
  for (int64_t d = 0; d < ndist; ++d) {
    const int32_t i = dist_pair[2 * d], j = dist_pair[2 * d + 1];
    if (i < 0 || i >= natoms || j < 0 || j >= natoms) return "distance restraint " + std::to_string(d) + ": atom index out of range";
    if (i == j) return "distance restraint " + std::to_string(d) + ": the two atoms of a pair must differ";
  }
  for (int64_t e = 0; e < nrep * npos; ++e) {
    if (!(pos_k[e] >= 0.0) || !std::isfinite(pos_k[e])) return "position restraints need a finite k >= 0";
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(pos_ref[3 * e + c])) return "position restraints need a finite reference";
  }
  for (int64_t e = 0; e < nrep * ndist; ++e) {
    if (!(dist_k[e] >= 0.0) || !std::isfinite(dist_k[e])) return "distance restraints need a finite k >= 0";
    if (!(dist_r0[e] >= 0.0) || !std::isfinite(dist_r0[e])) return "distance restraints need a finite r0 >= 0";
  }
  return "";
}

// The rows of the restrained atoms (ascending atom index): atoms[t] is written by thread t, which walks
// ent[off[t] .. off[t + 1]): the atom's position entry first, then its distance entries by restraint index.
inline void restraint_build_csr(int64_t npos, int64_t ndist, const int32_t *pos_atom, const int32_t *dist_pair,
                                std::vector<int32_t> &atoms, std::vector<int32_t> &off, std::vector<RestraintEntry> &ent) {
  atoms.clear();
  for (int64_t p = 0; p < npos; ++p) atoms.push_back(pos_atom[p]);
  for (int64_t d = 0; d < 2 * ndist; ++d) atoms.push_back(dist_pair[d]);
  std::sort(atoms.begin(), atoms.end());
  atoms.erase(std::unique(atoms.begin(), atoms.end()), atoms.end());
  auto row = [&](int32_t a) { return (size_t)(std::lower_bound(atoms.begin(), atoms.end(), a) - atoms.begin()); };
  std::vector<int32_t> count(atoms.size(), 0);
  for (int64_t p = 0; p < npos; ++p) count[row(pos_atom[p])]++;
  for (int64_t d = 0; d < 2 * ndist; ++d) count[row(dist_pair[d])]++;
  off.assign(atoms.size() + 1, 0);
  for (size_t t = 0; t < atoms.size(); ++t) off[t + 1] = off[t] + count[t];
  ent.assign((size_t)off[atoms.size()], RestraintEntry{0, 0, -1, 0});
  std::vector<int32_t> fill(off.begin(), off.end() - 1);
  for (int64_t p = 0; p < npos; ++p) ent[(size_t)fill[row(pos_atom[p])]++] = RestraintEntry{0, (int32_t)p, -1, 0};
  for (int64_t d = 0; d < ndist; ++d) {
    const int32_t i = dist_pair[2 * d], j = dist_pair[2 * d + 1];
    ent[(size_t)fill[row(i)]++] = RestraintEntry{1, (int32_t)d, j, +1};
    ent[(size_t)fill[row(j)]++] = RestraintEntry{1, (int32_t)d, i, -1};
  }
}

}  // namespace tmd
