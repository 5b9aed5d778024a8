// Collective variables of groups of atoms for metadynamics: the distance, angle and dihedral of group centres and the
// coordination number of two sets, with their gradients, shared by the kernels of metad_group.hip and a host program
// (tests/metad_group_math_host.cpp), in double.  Compile with floating-point contraction off: the order of the operations below
// is the contract.  The centre of a group is group_math.h's (group_centre_add), the dihedral metad_math.h's.
//
//   distance      s = |mi(X_A - X_B)|                                        ds/dX_A = d / r, ds/dX_B = -d / r; r = 0: no gradient
//   angle         s = acos(clamp(u.v / (|u| |v|), -1, 1)), u = mi(X_A - X_B), v = mi(X_C - X_B); a zero arm or sin = 0: no gradient
//   dihedral      metad_dihedral of the four centres
//   coordination  s = sum_{i in A} sum_{j in B, j != i} f(r_ij), r = |mi(x_i - x_j)|, x = (r - d0) / r0,
//                 phi(x) = 1 for x <= 0, 1 / (1 + x^n) otherwise: the rational switch (1 - x^n) / (1 - x^2n) without its removable
//                 singularity at x = 1; x^n by repeated multiplication, p = x, then n - 1 times p = p * x.
//                 With dmax: f = (phi - phi_max) / (1 - phi_max) for r < dmax and 0 from dmax on, phi_max = phi((dmax - d0) / r0),
//                 continuous and 0 at dmax.  Without: f = phi.  df/dr = 0 where x <= 0 (so also at r = 0: d0 >= 0).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "group_math.h"
#include "metad_math.h"

namespace tmd {

constexpr int kCvDistance = 2, kCvAngle = 3, kCvDihedral = 4, kCvCoordination = 5;  // TMDHIP_METAD_GROUP_* / _COORDINATION
__host__ __device__ inline int cv_arity(int kind) { return kind == kCvCoordination ? 2 : kind; }
__host__ __device__ inline bool cv_periodic(int kind) { return kind == kCvDihedral; }

// the switch of one coordination CV; phimax and scale = 1 / (1 - phimax) are made once on the host (coord_params)
struct CoordParams {
  double r0, d0, dmax, phimax, scale;
  int32_t n, has_dmax;
};

// phi(x) and d phi / dx: 1 and 0 for x <= 0; otherwise q = x^(n-1), 1 / (1 + q x) and -(n q) / (1 + q x)^2
__host__ __device__ inline double coord_phi(double x, int n, double &dphi) {
#pragma clang fp contract(off)
  if (!(x > 0.0)) {
    dphi = 0.0;
    return 1.0;
  }
  double q = 1.0;
  for (int k = 1; k < n; ++k) q = q * x;
  const double den = 1.0 + q * x;
  dphi = -((double)n * q) / (den * den);
  return 1.0 / den;
}

inline CoordParams coord_params(double r0, int n, double d0, double dmax) {
#pragma clang fp contract(off)
  CoordParams P{r0, d0, dmax > 0.0 ? dmax : 0.0, 0.0, 1.0, n, dmax > 0.0 ? 1 : 0};
  if (P.has_dmax) {
    double unused;
    P.phimax = coord_phi((dmax - d0) / r0, n, unused);
    P.scale = 1.0 / (1.0 - P.phimax);
  }
  return P;
}

// f(r) and df/dr
__host__ __device__ inline double coord_switch(const CoordParams &P, double r, double &df) {
#pragma clang fp contract(off)
  df = 0.0;
  if (P.has_dmax && !(r < P.dmax)) return 0.0;
  double dphi;
  const double phi = coord_phi((r - P.d0) / P.r0, P.n, dphi);
  if (!P.has_dmax) {
    df = dphi / P.r0;
    return phi;
  }
  df = (dphi / P.r0) * P.scale;
  return (phi - P.phimax) * P.scale;
}

// One pair seen from atom i: val += f(r), grad += df/dr d / r with d = mi(x_i - x_j).  (mi is odd, so what atom j adds for
// itself from mi(x_j - x_i) is the exact negative.)
__host__ __device__ inline void coord_pair_add(const CoordParams &P, const double *xi, const double *xj, const double *box, double &val,
                                               double (&grad)[3]) {
#pragma clang fp contract(off)
  double d[3] = {xi[0] - xj[0], xi[1] - xj[1], xi[2] - xj[2]};
  metad_min_image(d, box);
  const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  double df;
  val += coord_switch(P, r, df);
  if (df != 0.0) {
    const double g = df / r;
    for (int c = 0; c < 3; ++c) grad[c] += g * d[c];
  }
}

// A CV of centres X[0 .. arity): s and g[a] = ds/dX_a (rows beyond the arity are zeroed)
__host__ __device__ inline double cv_of_centres(int kind, const double (&X)[4][3], const double *box, double (&g)[4][3]) {
#pragma clang fp contract(off)
  for (int a = 0; a < 4; ++a) g[a][0] = g[a][1] = g[a][2] = 0.0;
  if (kind == kCvDistance) {
    double d[3] = {X[0][0] - X[1][0], X[0][1] - X[1][1], X[0][2] - X[1][2]};
    metad_min_image(d, box);
    const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (r > 0.0)
      for (int c = 0; c < 3; ++c) {
        g[0][c] = d[c] / r;
        g[1][c] = -g[0][c];
      }
    return r;
  }
  if (kind == kCvAngle) {
    double u[3], v[3];
    for (int c = 0; c < 3; ++c) {
      u[c] = X[0][c] - X[1][c];
      v[c] = X[2][c] - X[1][c];
    }
    metad_min_image(u, box);
    metad_min_image(v, box);
    const double nu = sqrt(metad_dot(u, u)), nv = sqrt(metad_dot(v, v));
    double co = 1.0;  // (a zero arm: no direction; theta = 0 by convention, as group_math.h)
    if (nu > 0.0 && nv > 0.0) co = metad_dot(u, v) / (nu * nv);
    co = co > 1.0 ? 1.0 : (co < -1.0 ? -1.0 : co);
    const double theta = acos(co);
    const double si = sqrt(1.0 - co * co);
    if (nu > 0.0 && nv > 0.0 && si > 0.0) {
      const double fa = 1.0 / (nu * si), fc = 1.0 / (nv * si);
      for (int c = 0; c < 3; ++c) {
        const double uh = u[c] / nu, vh = v[c] / nv;
        g[0][c] = -(fa * (vh - co * uh));
        g[2][c] = -(fc * (uh - co * vh));
        g[1][c] = -g[0][c] - g[2][c];
      }
    }
    return theta;
  }
  return metad_dihedral(X, box, g);
}

}  // namespace tmd

// ---- host side: validation and the tables the kernels walk ----
#include <algorithm>
#include <string>
#include <vector>

namespace tmd {

constexpr int kCvThreads = 256;       // the block of every kernel of metad_group.hip
// A lane's partners are a chain of dependent double divisions and square roots, about 0.35 us a pair on an MI355X whatever
// the number of live lanes: an ion against 32 768 partners took 356 us in splits of 1 024.  Hence short
// splits, and as many blocks as keep every compute unit busy a few times over.
constexpr int kCvSplitPairs = 64;     // partners one lane takes per split of the streamed set
constexpr int kCvSplitBlocks = 1024;  // no more splits than bring a pass to this many blocks

// What tmdhip_set_metadynamics_groups refuses in the definition itself ("" = nothing); fields as in tmdhip_metad_group_desc.
inline std::string cv_validate(int64_t natoms, int64_t ncv, const int32_t *kind, const int32_t *groups /* [ncv][4] */, int64_t ngroups,
                               const int32_t *group_off, const int32_t *member_atom, const double *member_weight, const int32_t *bins,
                               const double *grid_min, const double *grid_max, const double *sigma, const int32_t *coord_n,
                               const double *coord_r0, const double *coord_d0, const double *coord_dmax) {
  if (natoms <= 0) return "bad size";
  if (ncv < 1) return "at least one CV is needed";
  if (ncv > kMetadMaxCv) return "more than 2 CVs";
  for (int64_t c = 0; c < ncv; ++c)
    if (kind[c] < kCvDistance || kind[c] > kCvCoordination) return "CV " + std::to_string(c) + ": unknown kind";
  if (ngroups <= 0) return "at least one group is needed";
  if (!group_off || !member_atom || !member_weight) return "null group table";
  if (group_off[0] != 0) return "group offsets must start at 0";
  std::vector<int64_t> seen((size_t)natoms, -1);
  for (int64_t g = 0; g < ngroups; ++g) {
    if (group_off[g + 1] < group_off[g]) return "group offsets must not decrease";
    if (group_off[g + 1] == group_off[g]) return "group " + std::to_string(g) + " is empty";
    for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) {
      const int32_t a = member_atom[m];
      if (a < 0 || a >= natoms) return "group " + std::to_string(g) + ": atom index out of range";
      if (seen[a] == g) return "group " + std::to_string(g) + ": atom " + std::to_string(a) + " is repeated";
      seen[a] = g;
      if (!std::isfinite(member_weight[m]) || !(member_weight[m] > 0.0))
        return "group " + std::to_string(g) + ": weights must be finite and > 0";
    }
  }
  for (int64_t c = 0; c < ncv; ++c) {
    const std::string cv = "CV " + std::to_string(c) + ": ";
    const int n = cv_arity(kind[c]);
    for (int a = 0; a < 4; ++a) {
      const int32_t g = groups[4 * c + a];
      if (a >= n) {
        if (g != -1) return cv + "wrong number of groups for its kind";
        continue;
      }
      if (g == -1) return cv + "wrong number of groups for its kind";
      if (g < 0 || g >= ngroups) return cv + "group index out of range";
      if (kind[c] != kCvCoordination)
        for (int b = 0; b < a; ++b)
          if (groups[4 * c + b] == g) return cv + "a group is named twice";
    }
    if (kind[c] == kCvCoordination) {
      if (!(coord_r0[c] > 0.0) || !std::isfinite(coord_r0[c])) return cv + "r0 must be finite and positive";
      if (coord_n[c] < 2 || coord_n[c] > 24) return cv + "n must be a whole number in [2, 24]";
      if (!(coord_d0[c] >= 0.0) || !std::isfinite(coord_d0[c])) return cv + "d0 must be finite and >= 0";
      if (!std::isfinite(coord_dmax[c]) || (coord_dmax[c] > 0.0 && !(coord_d0[c] < coord_dmax[c]))) return cv + "d_max must lie above d0";
      const int64_t na = group_off[groups[4 * c] + 1] - group_off[groups[4 * c]];
      const int64_t nb = group_off[groups[4 * c + 1] + 1] - group_off[groups[4 * c + 1]];
      if (na * nb >= ((int64_t)1 << 31)) return cv + "|A| |B| must stay below 2^31";
    }
    if (!(sigma[c] > 0.0) || !std::isfinite(sigma[c])) return cv + "sigma must be finite and positive";
    if (bins[c] < 1) return cv + "bins must be positive";
    double lo = -kMetadPi, hi = kMetadPi;
    if (!cv_periodic(kind[c])) {
      lo = grid_min[c];
      hi = grid_max[c];
      if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return cv + "grid_min must lie below grid_max";
    }
    const double h = (hi - lo) / (double)bins[c];
    if (h > 0.5 * sigma[c] * (1.0 + 1e-12)) return cv + "the grid spacing must not exceed sigma / 2";
  }
  return "";
}

// What a coordination CV refuses in a box: without dmax, or with dmax beyond half the shortest non-zero edge, the minimum image
// puts a kink into f
inline std::string cv_check_box(const CoordParams &P, const double *box) {
  double shortest = 0.0;
  for (int k = 0; k < 3; ++k)
    if (box[k] != 0.0 && (shortest == 0.0 || box[k] < shortest)) shortest = box[k];
  if (shortest == 0.0) return "";
  if (!P.has_dmax) return "a coordination CV in a periodic box needs d_max";
  if (P.dmax > 0.5 * shortest) return "d_max of a coordination CV must not exceed half the shortest non-zero box edge";
  return "";
}

// the grid side of a definition: ncv, axes and sigma (what metad_interp / metad_gauss read)
inline MetadDef cv_grid_define(int64_t ncv, const int32_t *kind, const int32_t *bins, const double *grid_min, const double *grid_max,
                               const double *sigma) {
  MetadDef D{};
  D.ncv = (int32_t)ncv;
  D.nrows = 0;
  for (int c = 0; c < kMetadMaxCv; ++c) {
    for (int a = 0; a < 4; ++a) D.atom[c][a] = -1;
    if (c >= ncv) continue;
    D.kind[c] = kind[c];
    D.sigma[c] = sigma[c];
    const bool per = cv_periodic(kind[c]);
    const double lo = per ? -kMetadPi : grid_min[c], hi = per ? kMetadPi : grid_max[c];
    D.axis[c] = MetadAxis{lo, (hi - lo) / (double)bins[c], per ? bins[c] : bins[c] + 1, per ? 1 : 0};
  }
  for (int t = 0; t < kMetadMaxRows; ++t) {
    D.row_atom[t] = -1;
    D.row_role[t][0] = D.row_role[t][1] = -1;
  }
  return D;
}

// One pass of a coordination CV: the lanes stand for `nlane` members from `lane0` of member_atom, the `nstream` members from
// `stream0` stream through LDS in `nsplit` splits of `chunk`.  Lane i of split q writes its gradient to grad_off + (q nlane + i) 3
// of the replica's gradient scratch; the pass that reports the value (value = 1) also writes row part_off + block nsplit + q of
// the replica's partials.
struct CvPass {
  int32_t cv, value, lane0, nlane, stream0, nstream, nsplit, chunk, nblocks, grad_off, part_off, pad;
};
// one block of the first launch beyond the centres' blocks
struct CvTask {
  int32_t pass, block, split, pad;
};
// one addend of an atom's ds_c/dx: a centre (type 0: weight w times ds/dX of place `at`) or a pass of a coordination CV (type 1:
// the sum over `nsplit` partials from `at`, `stride` doubles apart)
struct CvEntry {
  int32_t cv, type, at, nsplit, stride, pad;
  double w;
};

struct CvTables {
  std::vector<CvPass> pass;
  std::vector<CvTask> task;
  std::vector<int32_t> atom, ent_off;  // the distinct atoms of the CVs, ascending; their entries: CV order, then group / pass order
  std::vector<CvEntry> ent;
  int64_t grad_doubles = 0, part_rows = 0;  // per replica
  int32_t part_off[kMetadMaxCv] = {0, 0}, part_n[kMetadMaxCv] = {0, 0};
};

inline int cv_nsplit(int64_t nlane, int64_t nstream) {
  const int64_t nblocks = (nlane + kCvThreads - 1) / kCvThreads;
  const int64_t want = (nstream + kCvSplitPairs - 1) / kCvSplitPairs, cap = std::max<int64_t>(1, kCvSplitBlocks / nblocks);
  return (int)std::max<int64_t>(1, std::min(want, cap));
}

inline CvTables cv_build(int64_t ncv, const int32_t *kind, const int32_t *groups, int64_t ngroups, const int32_t *group_off,
                         const int32_t *member_atom, const std::vector<double> &w /* normalised */) {
  CvTables T;
  struct Add {
    int32_t atom;
    CvEntry e;
  };
  std::vector<Add> adds;
  for (int c = 0; c < ncv; ++c) {
    if (kind[c] != kCvCoordination) {
      // (ascending group index: the order in which an atom in two groups of the CV adds)
      std::vector<std::pair<int32_t, int32_t>> gs;
      for (int a = 0; a < cv_arity(kind[c]); ++a) gs.push_back({groups[4 * c + a], a});
      std::sort(gs.begin(), gs.end());
      for (auto &ga : gs)
        for (int32_t m = group_off[ga.first]; m < group_off[ga.first + 1]; ++m)
          adds.push_back({member_atom[m], CvEntry{c, 0, ga.second, 0, 0, 0, w[(size_t)m]}});
      continue;
    }
    const int32_t gA = groups[4 * c], gB = groups[4 * c + 1];
    const int32_t nA = group_off[gA + 1] - group_off[gA], nB = group_off[gB + 1] - group_off[gB];
    T.part_off[c] = (int32_t)T.part_rows;
    for (int p = 0; p < 2; ++p) {
      CvPass P{};
      P.cv = c;
      P.value = (p == 0) == (nA >= nB) ? 1 : 0;  // (the larger set's pass reports the value: more lanes share the sum)
      P.lane0 = group_off[p == 0 ? gA : gB];
      P.nlane = p == 0 ? nA : nB;
      P.stream0 = group_off[p == 0 ? gB : gA];
      P.nstream = p == 0 ? nB : nA;
      P.nsplit = cv_nsplit(P.nlane, P.nstream);
      P.chunk = (P.nstream + P.nsplit - 1) / P.nsplit;
      P.nblocks = (P.nlane + kCvThreads - 1) / kCvThreads;
      P.grad_off = (int32_t)T.grad_doubles;
      P.part_off = (int32_t)T.part_rows;
      T.grad_doubles += (int64_t)P.nsplit * P.nlane * 3;
      if (P.value) {
        T.part_n[c] = P.nblocks * P.nsplit;
        T.part_rows += T.part_n[c];
      }
      const int32_t ip = (int32_t)T.pass.size();
      T.pass.push_back(P);
      for (int32_t b = 0; b < P.nblocks; ++b)
        for (int32_t q = 0; q < P.nsplit; ++q) T.task.push_back(CvTask{ip, b, q, 0});
      for (int32_t i = 0; i < P.nlane; ++i)
        adds.push_back({member_atom[P.lane0 + i], CvEntry{c, 1, P.grad_off + 3 * i, P.nsplit, 3 * P.nlane, 0, 1.0}});
    }
  }
  // rows by ascending atom; a stable sort keeps every atom's entries in the order made above
  std::stable_sort(adds.begin(), adds.end(), [](const Add &a, const Add &b) { return a.atom < b.atom; });
  for (size_t k = 0; k < adds.size(); ++k) {
    if (k == 0 || adds[k].atom != adds[k - 1].atom) {
      T.atom.push_back(adds[k].atom);
      T.ent_off.push_back((int32_t)k);
    }
    T.ent.push_back(adds[k].e);
  }
  T.ent_off.push_back((int32_t)adds.size());
  return T;
}

}  // namespace tmd
