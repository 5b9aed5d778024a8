// Well-tempered metadynamics on one or two collective variables (CVs): the CVs and their gradients, the Hermite interpolant of
// the tabulated bias and the Gaussian node terms of a deposition, shared by the kernels of metad.hip and a host program
// (tests/metad_math_host.cpp), in double.  Compile with floating-point contraction off: the order of the operations below is
// the contract.
//
// A grid node holds the ANALYTIC sum of the deposited Gaussians and of its derivatives: (V, V') in one dimension, (V, d1 V,
// d2 V, d1 d2 V) in two, the second CV's node index running fastest.  The bias is DEFINED as the cubic / bicubic Hermite
// interpolant of those node values: C1, exact on the nodes, and its force is the exact derivative of what the energy reports.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace tmd {

constexpr int kMetadMaxCv = 2;
constexpr int kMetadMaxRows = 8;  // distinct atoms of two CVs of four atoms each
constexpr double kMetadPi = 3.14159265358979323846;
constexpr int kMetadDistance = 0, kMetadDihedral = 1;

// one CV's axis of the grid: node k lies at lo + k h.  Periodic (a dihedral): `nodes` = bins nodes on [-pi, pi), wrapped;
// otherwise `nodes` = bins + 1 and the CV is clamped to [lo, lo + bins h] for the lookup
struct MetadAxis {
  double lo, h;
  int32_t nodes, periodic;
};

// What the kernels need to know of a bias: the CVs, the rows (one per DISTINCT atom, ascending; row_role[t][c] = the place of
// row t's atom in CV c, or -1), the grid's axes and the Gaussian widths.
struct MetadDef {
  int32_t ncv, nrows;
  int32_t kind[kMetadMaxCv];
  int32_t atom[kMetadMaxCv][4];
  int32_t row_atom[kMetadMaxRows];
  int32_t row_role[kMetadMaxRows][kMetadMaxCv];
  MetadAxis axis[kMetadMaxCv];
  double sigma[kMetadMaxCv];
};

// doubles per node and nodes per grid
__host__ __device__ inline int metad_width(const MetadDef &D) { return D.ncv == 1 ? 2 : 4; }
__host__ __device__ inline int64_t metad_nodes(const MetadDef &D) {
  return D.ncv == 1 ? (int64_t)D.axis[0].nodes : (int64_t)D.axis[0].nodes * D.axis[1].nodes;
}

// d <- minimum image of d in the orthorhombic box (edge lengths); an edge of zero: no image along that axis
__host__ __device__ inline void metad_min_image(double (&d)[3], const double *box) {
#pragma clang fp contract(off)
  for (int k = 0; k < 3; ++k)
    if (box[k] != 0.0) d[k] = d[k] - box[k] * rint(d[k] / box[k]);
}

// r = |minimum image of x_i - x_j| and its gradients (rows 0, 1 of g; r = 0: no direction, zero gradient)
__host__ __device__ inline double metad_distance(const double (&x)[4][3], const double *box, double (&g)[4][3]) {
#pragma clang fp contract(off)
  double d[3] = {x[0][0] - x[1][0], x[0][1] - x[1][1], x[0][2] - x[1][2]};
  metad_min_image(d, box);
  const double r = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  for (int c = 0; c < 3; ++c) {
    g[0][c] = r > 0.0 ? d[c] / r : 0.0;
    g[1][c] = -g[0][c];
    g[2][c] = g[3][c] = 0.0;
  }
  return r;
}

__host__ __device__ inline double metad_dot(const double (&a)[3], const double (&b)[3]) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__host__ __device__ inline void metad_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// atan on [0, 1] and atan2 by the four operations alone: the kernel, the host build and the numpy model give the SAME BITS,
// whatever libm each of them has.  That matters because a hill centre that differs by one ulp moves the term of a node at
// distance Delta by |Delta| / sigma^2 ulps: with a shared atan2 the grids of device and model agree to the rounding of a sum.
// x = c + (x - c), c = k / 8 the nearest eighth: atan x = atan c + atan z, z = (x - c) / (1 + x c), |z| <= 1/16, and the odd
// series of atan z to z^17 (the next term is below 2e-22).  About one ulp from the true value.
__host__ __device__ inline double metad_atan_unit(double x) {
#pragma clang fp contract(off)
  constexpr double kAtanEighths[9] = {0.0,
                                      0.12435499454676144,
                                      0.24497866312686414,
                                      0.35877067027057225,
                                      0.4636476090008061,
                                      0.5585993153435624,
                                      0.6435011087932844,
                                      0.7188299996216245,
                                      0.7853981633974483};
  const int k = (int)(8.0 * x + 0.5);
  const double c = 0.125 * (double)k;
  const double z = (x - c) / (1.0 + x * c);
  const double q = z * z;
  double p = 1.0 / 17.0;
  p = 1.0 / 15.0 - q * p;
  p = 1.0 / 13.0 - q * p;
  p = 1.0 / 11.0 - q * p;
  p = 1.0 / 9.0 - q * p;
  p = 1.0 / 7.0 - q * p;
  p = 1.0 / 5.0 - q * p;
  p = 1.0 / 3.0 - q * p;
  p = 1.0 - q * p;
  return kAtanEighths[k] + z * p;
}

// atan2(y, x) in [-pi, pi]; (0, 0) gives 0, a NaN gives NaN
__host__ __device__ inline double metad_atan2(double y, double x) {
#pragma clang fp contract(off)
  const double ax = fabs(x), ay = fabs(y);
  if (!(ax == ax) || !(ay == ay)) return ax + ay;
  if (!(ax <= 1.7976931348623157e308) || !(ay <= 1.7976931348623157e308)) return (ax + ay) - (ax + ay);  // (an infinity: NaN)
  double a = 0.0;
  if (ay <= ax) {
    if (ax > 0.0) a = metad_atan_unit(ay / ax);
  } else {
    a = 0.5 * kMetadPi - metad_atan_unit(ax / ay);
  }
  if (x < 0.0) a = kMetadPi - a;
  return y < 0.0 ? -a : a;
}

// The torsion of atoms i, j, k, l from the minimum-imaged bond vectors b1 = x_j - x_i, b2 = x_k - x_j, b3 = x_l - x_k:
// phi = atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3)), the sign of the bonded term (bonded_math.h: -atan2(sin, cos) of
// r12 = -b1, r23 = -b2, r34 = -b3 is the same angle).  Gradients without 1 / sin phi (with A = b1 x b2, B = b2 x b3):
//   d phi / d x_i = -|b2| A / |A|^2              d phi / d x_l = |b2| B / |B|^2
//   d phi / d x_j = -(1 + p) g_i + q g_l         d phi / d x_k = -(1 + q) g_l + p g_i      p = b1 . b2 / |b2|^2, q = b3 . b2 / |b2|^2
// singular only where three atoms are collinear (A = 0 or B = 0): zero gradient there.
__host__ __device__ inline double metad_dihedral(const double (&x)[4][3], const double *box, double (&g)[4][3]) {
#pragma clang fp contract(off)
  double b1[3], b2[3], b3[3], A[3], B[3];
  for (int c = 0; c < 3; ++c) {
    b1[c] = x[1][c] - x[0][c];
    b2[c] = x[2][c] - x[1][c];
    b3[c] = x[3][c] - x[2][c];
  }
  metad_min_image(b1, box);
  metad_min_image(b2, box);
  metad_min_image(b3, box);
  metad_cross(b1, b2, A);
  metad_cross(b2, b3, B);
  const double n2 = metad_dot(b2, b2), nb = sqrt(n2);
  const double A2 = metad_dot(A, A), B2 = metad_dot(B, B);
  const double phi = metad_atan2(nb * metad_dot(b1, B), metad_dot(A, B));
  if (!(A2 > 0.0) || !(B2 > 0.0)) {
    for (int a = 0; a < 4; ++a) g[a][0] = g[a][1] = g[a][2] = 0.0;
    return phi;
  }
  const double si = -nb / A2, sl = nb / B2;
  const double p = metad_dot(b1, b2) / n2, q = metad_dot(b3, b2) / n2;
  for (int c = 0; c < 3; ++c) {
    const double gi = si * A[c], gl = sl * B[c];
    g[0][c] = gi;
    g[3][c] = gl;
    g[1][c] = (-gi - p * gi) + q * gl;
    g[2][c] = (-gl - q * gl) + p * gi;
  }
  return phi;
}

// The cubic Hermite basis on a cell of width h at t in [0, 1], for the cell's two nodes a = 0, 1:
//   val[a][0] weighs the node's value, val[a][1] its slope (h included); der[a][.] are their derivatives by the CV.
__host__ __device__ inline void metad_basis(double t, double h, double (&val)[2][2], double (&der)[2][2]) {
#pragma clang fp contract(off)
  const double u = 1.0 - t;
  val[0][0] = (1.0 + 2.0 * t) * (u * u);
  val[1][0] = (t * t) * (3.0 - 2.0 * t);
  val[0][1] = h * (t * (u * u));
  val[1][1] = h * ((t * t) * (t - 1.0));
  der[0][0] = (6.0 * t * (t - 1.0)) / h;
  der[1][0] = (6.0 * t * u) / h;
  der[0][1] = u * (1.0 - 3.0 * t);
  der[1][1] = t * (3.0 * t - 2.0);
}

// The cell of CV value s on an axis: nodes k[0], k[1], the place t in the cell; returns 1 where the bias depends on s (0
// outside a non-periodic grid: s is clamped, V constant, no force).  A periodic axis wraps (atan2 may return +pi itself).
__host__ __device__ inline double metad_locate(const MetadAxis &a, double s, int (&k)[2], double &t) {
#pragma clang fp contract(off)
  double x = (s - a.lo) / a.h;
  if (a.periodic) {
    if (!(x == x)) x = 0.0;
    const double fl = floor(x);
    t = x - fl;
    int64_t c = (int64_t)fl % a.nodes;
    if (c < 0) c += a.nodes;
    k[0] = (int)c;
    k[1] = k[0] + 1 == a.nodes ? 0 : k[0] + 1;
    return 1.0;
  }
  const int bins = a.nodes - 1;
  double live = 1.0;
  if (!(x >= 0.0)) {  // (a NaN too)
    x = 0.0;
    live = 0.0;
  } else if (x > (double)bins) {
    x = (double)bins;
    live = 0.0;
  }
  double fl = floor(x);
  if (fl > (double)(bins - 1)) fl = (double)(bins - 1);
  t = x - fl;
  k[0] = (int)fl;
  k[1] = k[0] + 1;
  return live;
}

// V(s) of the interpolant on `grid` (one grid: [nodes0][2] or [nodes0][nodes1][4] doubles) and dV[c] = dV / ds_c.
__host__ __device__ inline double metad_interp(const MetadDef &D, const double *grid, const double *s, double (&dV)[kMetadMaxCv]) {
#pragma clang fp contract(off)
  int k0[2];
  double t0, v0[2][2], d0[2][2];
  const double live0 = metad_locate(D.axis[0], s[0], k0, t0);
  metad_basis(t0, D.axis[0].h, v0, d0);
  dV[0] = dV[1] = 0.0;
  if (D.ncv == 1) {
    double V = 0.0, dv = 0.0;
    for (int a = 0; a < 2; ++a) {
      const double *nd = grid + 2 * (size_t)k0[a];
      V += v0[a][0] * nd[0] + v0[a][1] * nd[1];
      dv += d0[a][0] * nd[0] + d0[a][1] * nd[1];
    }
    dV[0] = live0 * dv;
    return V;
  }
  int k1[2];
  double t1, v1[2][2], d1[2][2];
  const double live1 = metad_locate(D.axis[1], s[1], k1, t1);
  metad_basis(t1, D.axis[1].h, v1, d1);
  double V = 0.0, da = 0.0, db = 0.0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const double *nd = grid + 4 * ((size_t)k0[a] * D.axis[1].nodes + k1[b]);
      V += (v0[a][0] * v1[b][0] * nd[0] + v0[a][1] * v1[b][0] * nd[1]) + (v0[a][0] * v1[b][1] * nd[2] + v0[a][1] * v1[b][1] * nd[3]);
      da += (d0[a][0] * v1[b][0] * nd[0] + d0[a][1] * v1[b][0] * nd[1]) + (d0[a][0] * v1[b][1] * nd[2] + d0[a][1] * v1[b][1] * nd[3]);
      db += (v0[a][0] * d1[b][0] * nd[0] + v0[a][1] * d1[b][0] * nd[1]) + (v0[a][0] * d1[b][1] * nd[2] + v0[a][1] * d1[b][1] * nd[3]);
    }
  dV[0] = live0 * da;
  dV[1] = live1 * db;
  return V;
}

// The CVs at the positions x[c] of their atoms (in the CV's order): s[c] and the gradients g[c][place][3]
__host__ __device__ inline void metad_cvs(const MetadDef &D, const double (&x)[kMetadMaxCv][4][3], const double *box, double *s,
                                          double (&g)[kMetadMaxCv][4][3]) {
  for (int c = 0; c < D.ncv; ++c) s[c] = D.kind[c] == kMetadDistance ? metad_distance(x[c], box, g[c]) : metad_dihedral(x[c], box, g[c]);
}

// The bias force on the atom of row t: -sum over the CVs, in CV order, of dV / ds_c times the CV's gradient at the atom
__host__ __device__ inline void metad_row_force(const MetadDef &D, int t, const double (&dV)[kMetadMaxCv],
                                                const double (&g)[kMetadMaxCv][4][3], double (&f)[3]) {
#pragma clang fp contract(off)
  f[0] = f[1] = f[2] = 0.0;
  for (int c = 0; c < D.ncv; ++c) {
    const int role = D.row_role[t][c];
    if (role < 0) continue;
    for (int k = 0; k < 3; ++k) f[k] += -dV[c] * g[c][role][k];
  }
}

// What a hill of height w centred at s0 adds to the node of indices k (Delta = node - s0, the minimum image on a periodic
// axis): the Gaussian w exp(-sum Delta_c^2 / 2 sigma_c^2) and its derivatives by the node's coordinates, `width` doubles.
__host__ __device__ inline void metad_gauss(const MetadDef &D, const int *k, const double *s0, double w, double *out) {
#pragma clang fp contract(off)
  double dl[kMetadMaxCv], arg = 0.0;
  for (int c = 0; c < D.ncv; ++c) {
    double d = (D.axis[c].lo + (double)k[c] * D.axis[c].h) - s0[c];
    if (D.axis[c].periodic) d = d - (2.0 * kMetadPi) * rint(d / (2.0 * kMetadPi));
    dl[c] = d;
    arg += (d * d) / (2.0 * (D.sigma[c] * D.sigma[c]));
  }
  const double e = w * exp(-arg);
  out[0] = e;
  out[1] = (-dl[0] / (D.sigma[0] * D.sigma[0])) * e;
  if (D.ncv == 2) {
    out[2] = (-dl[1] / (D.sigma[1] * D.sigma[1])) * e;
    out[3] = ((dl[0] / (D.sigma[0] * D.sigma[0])) * (dl[1] / (D.sigma[1] * D.sigma[1]))) * e;
  }
}

// The height of the next hill: `height` (plain), or height exp(-V(s0) / k_B dT) with V read from the grid as it is
__host__ __device__ inline double metad_height(double height, double V, double kdt, int plain) {
#pragma clang fp contract(off)
  return plain ? height : height * exp(-V / kdt);
}

}  // namespace tmd

// ---- host side: validation, the axes and the rows ----
#include <algorithm>
#include <string>
#include <vector>

namespace tmd {

// What tmdhip_set_metadynamics refuses in the definition itself ("" = nothing); fields as in tmdhip_metad_desc.
inline std::string metad_validate(int64_t natoms, int64_t ncv, const int32_t *kind, const int32_t *atoms /* [ncv][4] */,
                                  const int32_t *bins, const double *grid_min, const double *grid_max, const double *sigma) {
  if (natoms <= 0) return "bad size";
  if (ncv < 1) return "at least one CV is needed";
  if (ncv > kMetadMaxCv) return "more than 2 CVs";
  for (int64_t c = 0; c < ncv; ++c) {
    const std::string cv = "CV " + std::to_string(c) + ": ";
    if (kind[c] != kMetadDistance && kind[c] != kMetadDihedral) return cv + "unknown kind";
    const int na = kind[c] == kMetadDistance ? 2 : 4;
    for (int a = 0; a < na; ++a) {
      const int32_t i = atoms[4 * c + a];
      if (i < 0 || i >= natoms) return cv + "atom index out of range";
      for (int b = 0; b < a; ++b)
        if (atoms[4 * c + b] == i) return cv + "atom " + std::to_string(i) + " is repeated";
    }
    if (!(sigma[c] > 0.0) || !std::isfinite(sigma[c])) return cv + "sigma must be finite and positive";
    if (bins[c] < 1) return cv + "bins must be positive";
    double lo = -kMetadPi, hi = kMetadPi;
    if (kind[c] == kMetadDistance) {
      lo = grid_min[c];
      hi = grid_max[c];
      if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return cv + "grid_min must lie below grid_max";
    }
    const double h = (hi - lo) / (double)bins[c];
    if (h > 0.5 * sigma[c] * (1.0 + 1e-12)) return cv + "the grid spacing must not exceed sigma / 2";
  }
  return "";
}

// The axes, the rows of the distinct atoms (ascending) and each row's place in every CV
inline MetadDef metad_define(int64_t ncv, const int32_t *kind, const int32_t *atoms, const int32_t *bins, const double *grid_min,
                             const double *grid_max, const double *sigma) {
  MetadDef D{};
  D.ncv = (int32_t)ncv;
  std::vector<int32_t> all;
  for (int c = 0; c < ncv; ++c) {
    D.kind[c] = kind[c];
    D.sigma[c] = sigma[c];
    const bool per = kind[c] == kMetadDihedral;
    const double lo = per ? -kMetadPi : grid_min[c], hi = per ? kMetadPi : grid_max[c];
    D.axis[c] = MetadAxis{lo, (hi - lo) / (double)bins[c], per ? bins[c] : bins[c] + 1, per ? 1 : 0};
    for (int a = 0; a < 4; ++a) {
      D.atom[c][a] = a < (per ? 4 : 2) ? atoms[4 * c + a] : -1;
      if (D.atom[c][a] >= 0) all.push_back(D.atom[c][a]);
    }
  }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  D.nrows = (int32_t)all.size();
  for (int t = 0; t < kMetadMaxRows; ++t) {
    D.row_atom[t] = t < D.nrows ? all[t] : -1;
    for (int c = 0; c < kMetadMaxCv; ++c) {
      D.row_role[t][c] = -1;
      if (t < D.nrows && c < ncv)
        for (int a = 0; a < 4; ++a)
          if (D.atom[c][a] == all[t]) D.row_role[t][c] = a;
    }
  }
  return D;
}

}  // namespace tmd
