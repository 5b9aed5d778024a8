// Restraints on the distance, angle and dihedral between centres of groups of atoms: the centre's member term, energy and
// force of one restraint on its centres, shared by the kernels of group_restraint.hip and a host program
// (tests/group_math_host.cpp), in double.  Compile with floating-point contraction off: the order of the operations below is
// the contract.
//
//   centre      X_g = x_a0 + sum_a w_a mi(x_a - x_a0), a0 the group's first atom, w_a = W_a / sum W, mi the minimum image of
//               restraint_math.h.  Every atom of a group must lie within half a box edge of a0 along every periodic axis.
//   distance    s = |mi(X_a - X_b)|
//   angle       s = acos(clamp(u.v / (|u| |v|), -1, 1)), u = mi(X_a - X_b), v = mi(X_c - X_b)
//   dihedral    s = metad_dihedral of the four centres (metad_math.h), delta wrapped into [-pi, pi]
//   energy      delta = s - s0, u = sign(delta) max(|delta| - flat, 0), E = k u^2 / 2, dE/ds = k u
// Singular geometries (r = 0, sin theta = 0, a zero arm, what metad_dihedral reports as degenerate) give no force and the
// energy of the formula.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "metad_math.h"
#include "restraint_math.h"

namespace tmd {

constexpr int kGroupDistance = 0, kGroupAngle = 1, kGroupDihedral = 2;
__host__ __device__ inline int group_arity(int kind) { return kind + 2; }

// one member's term of its group's centre: w mi(x - x0), added to acc
__host__ __device__ inline void group_centre_add(const double *x, const double *x0, const double *box, double w, double (&acc)[3]) {
#pragma clang fp contract(off)
  double d[3] = {x[0] - x0[0], x[1] - x0[1], x[2] - x0[2]};
  restraint_min_image(d, box);
  for (int c = 0; c < 3; ++c) acc[c] += w * d[c];
}

// u of the flat-bottomed harmonic well
__host__ __device__ inline double group_flat(double delta, double flat) {
#pragma clang fp contract(off)
  const double m = fabs(delta) - flat;
  const double um = m > 0.0 ? m : 0.0;
  return delta < 0.0 ? -um : um;
}

// One restraint of `kind` on the centres X[0 .. arity): returns E, and F[a] = -dE/dX_a (rows beyond the arity are zeroed).
__host__ __device__ inline double group_restraint(int kind, const double (&X)[4][3], const double *box, double s0, double k, double flat,
                                                  double (&F)[4][3]) {
#pragma clang fp contract(off)
  for (int a = 0; a < 4; ++a) F[a][0] = F[a][1] = F[a][2] = 0.0;
  if (kind == kGroupDistance) {
    double d[3] = {X[0][0] - X[1][0], X[0][1] - X[1][1], X[0][2] - X[1][2]};
    restraint_min_image(d, box);
    const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const double u = group_flat(r - s0, flat);
    if (r > 0.0) {
      const double s = (-k * u) / r;
      for (int c = 0; c < 3; ++c) {
        F[0][c] = s * d[c];
        F[1][c] = -F[0][c];
      }
    }
    return 0.5 * k * (u * u);
  }
  if (kind == kGroupAngle) {
    double u[3], v[3];
    for (int c = 0; c < 3; ++c) {
      u[c] = X[0][c] - X[1][c];
      v[c] = X[2][c] - X[1][c];
    }
    restraint_min_image(u, box);
    restraint_min_image(v, box);
    const double nu = sqrt(metad_dot(u, u)), nv = sqrt(metad_dot(v, v));
    double co = 1.0;  // (a zero arm: no direction; theta = 0 by convention)
    if (nu > 0.0 && nv > 0.0) co = metad_dot(u, v) / (nu * nv);
    co = co > 1.0 ? 1.0 : (co < -1.0 ? -1.0 : co);
    const double theta = acos(co);
    const double w = group_flat(theta - s0, flat);
    const double si = sqrt(1.0 - co * co);
    if (nu > 0.0 && nv > 0.0 && si > 0.0) {
      // d theta / d X_a = -(v^ - cos u^) / (|u| sin), d theta / d X_c = -(u^ - cos v^) / (|v| sin); F = -k w d theta / d X
      const double fa = (k * w) / (nu * si), fc = (k * w) / (nv * si);
      for (int c = 0; c < 3; ++c) {
        const double uh = u[c] / nu, vh = v[c] / nv;
        F[0][c] = fa * (vh - co * uh);
        F[2][c] = fc * (uh - co * vh);
        F[1][c] = -F[0][c] - F[2][c];
      }
    }
    return 0.5 * k * (w * w);
  }
  double g[4][3];
  const double phi = metad_dihedral(X, box, g);
  double delta = phi - s0;
  delta = delta - (2.0 * kMetadPi) * rint(delta / (2.0 * kMetadPi));
  const double u = group_flat(delta, flat);
  const double s = -k * u;
  for (int a = 0; a < 4; ++a)
    for (int c = 0; c < 3; ++c) F[a][c] = s * g[a][c];
  return 0.5 * k * (u * u);
}

}  // namespace tmd

// ---- host side: validation, normalised weights and the per-atom rows ----
#include <algorithm>
#include <string>
#include <vector>

namespace tmd {

// What tmdhip_set_group_restraints refuses in the tables themselves ("" = nothing).  Arrays as in tmdhip_group_restraint_desc.
inline std::string group_validate(int64_t natoms, int64_t nrep, int64_t ngroups, const int32_t *group_off, const int32_t *member_atom,
                                  const double *member_weight, int64_t nrest, const int32_t *kind, const int32_t *groups,
                                  const double *target, const double *k, const double *flat) {
  if (natoms <= 0 || nrep <= 0 || ngroups <= 0 || nrest <= 0) return "bad size";
  if (!group_off || !member_atom || !member_weight) return "null group table";
  if (!kind || !groups || !target || !k || !flat) return "null restraint table";
  if (group_off[0] != 0) return "group offsets must start at 0";
  std::vector<int64_t> seen((size_t)natoms, -1);
  for (int64_t g = 0; g < ngroups; ++g) {
    if (group_off[g + 1] < group_off[g]) return "group offsets must not decrease";
    if (group_off[g + 1] == group_off[g]) return "group " + std::to_string(g) + " is empty";
    for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) {
      const int32_t a = member_atom[m];
      if (a < 0 || a >= natoms) return "group " + std::to_string(g) + ": atom index out of range";
      if (seen[a] == g) return "group " + std::to_string(g) + ": atom " + std::to_string(a) + " is named twice";
      seen[a] = g;
      if (!std::isfinite(member_weight[m]) || !(member_weight[m] > 0.0))
        return "group " + std::to_string(g) + ": weights must be finite and > 0";
    }
  }
  for (int64_t m = 0; m < nrest; ++m) {
    if (kind[m] < kGroupDistance || kind[m] > kGroupDihedral) return "restraint " + std::to_string(m) + ": unknown kind";
    const int n = group_arity(kind[m]);
    for (int a = 0; a < 4; ++a) {
      const int32_t g = groups[4 * m + a];
      if (a >= n) {
        if (g != -1) return "restraint " + std::to_string(m) + ": wrong number of groups for its kind";
        continue;
      }
      if (g == -1) return "restraint " + std::to_string(m) + ": wrong number of groups for its kind";
      if (g < 0 || g >= ngroups) return "restraint " + std::to_string(m) + ": group index out of range";
      for (int b = 0; b < a; ++b)
        if (groups[4 * m + b] == g) return "restraint " + std::to_string(m) + ": a group is named twice";
    }
  }
  for (int64_t r = 0; r < nrep; ++r)
    for (int64_t m = 0; m < nrest; ++m) {
      const int64_t e = r * nrest + m;
      if (!(k[e] >= 0.0) || !std::isfinite(k[e])) return "group restraints need a finite k >= 0";
      if (!(flat[e] >= 0.0) || !std::isfinite(flat[e])) return "group restraints need a finite flat >= 0";
      if (!std::isfinite(target[e])) return "group restraints need a finite target";
      if (kind[m] == kGroupAngle && !(target[e] >= 0.0 && target[e] <= kMetadPi)) return "an angle target must lie in [0, pi]";
    }
  return "";
}

// w_a = W_a / sum W, the sum taken in member order
inline void group_normalise(int64_t ngroups, const int32_t *group_off, const double *member_weight, std::vector<double> &w) {
  w.assign((size_t)group_off[ngroups], 0.0);
  for (int64_t g = 0; g < ngroups; ++g) {
    double sum = 0.0;
    for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) sum += member_weight[m];
    for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) w[(size_t)m] = member_weight[m] / sum;
  }
}

// place `role` of restraint `index` in a group's row
struct GroupUse {
  int32_t index, role;
};
// one membership of an atom: the group and the member's place in member_atom / the normalised weights
struct GroupMember {
  int32_t group, member;
};

// The rows the force kernel walks.  use_off / use: per group, the restraints that name it, by ascending restraint index.
// atoms (ascending, distinct, members of groups that some restraint names): atoms[t] is written by thread t, which walks
// mem[mem_off[t] .. mem_off[t + 1]) by ascending group index.
inline void group_build_csr(int64_t ngroups, const int32_t *group_off, const int32_t *member_atom, int64_t nrest, const int32_t *kind,
                            const int32_t *groups, std::vector<int32_t> &use_off, std::vector<GroupUse> &use, std::vector<int32_t> &atoms,
                            std::vector<int32_t> &mem_off, std::vector<GroupMember> &mem) {
  std::vector<std::vector<GroupUse>> per((size_t)ngroups);
  for (int64_t m = 0; m < nrest; ++m)
    for (int a = 0; a < group_arity(kind[m]); ++a) per[(size_t)groups[4 * m + a]].push_back(GroupUse{(int32_t)m, (int32_t)a});
  use_off.assign((size_t)ngroups + 1, 0);
  use.clear();
  for (int64_t g = 0; g < ngroups; ++g) {
    use.insert(use.end(), per[(size_t)g].begin(), per[(size_t)g].end());
    use_off[(size_t)g + 1] = (int32_t)use.size();
  }
  atoms.clear();
  for (int64_t g = 0; g < ngroups; ++g)
    if (!per[(size_t)g].empty())
      for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) atoms.push_back(member_atom[m]);
  std::sort(atoms.begin(), atoms.end());
  atoms.erase(std::unique(atoms.begin(), atoms.end()), atoms.end());
  auto row = [&](int32_t a) { return (size_t)(std::lower_bound(atoms.begin(), atoms.end(), a) - atoms.begin()); };
  std::vector<int32_t> count(atoms.size(), 0);
  for (int64_t g = 0; g < ngroups; ++g)
    if (!per[(size_t)g].empty())
      for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) count[row(member_atom[m])]++;
  mem_off.assign(atoms.size() + 1, 0);
  for (size_t t = 0; t < atoms.size(); ++t) mem_off[t + 1] = mem_off[t] + count[t];
  mem.assign((size_t)mem_off[atoms.size()], GroupMember{0, 0});
  std::vector<int32_t> fill(mem_off.begin(), mem_off.end() - 1);
  for (int64_t g = 0; g < ngroups; ++g)
    if (!per[(size_t)g].empty())
      for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) mem[(size_t)fill[row(member_atom[m])]++] = GroupMember{(int32_t)g, m};
}

}  // namespace tmd
