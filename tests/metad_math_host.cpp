// Host build of torchmd_amd/csrc/metad_math.h for tests/test_metad_host.py: the CVs, the Hermite interpolant, the Gaussian node
// terms and the validation of a definition behind a plain C interface, compiled with the system C++ compiler and
// -ffp-contract=off (the kernels' `#pragma clang fp contract(off)`).
#include "metad_math.h"

#include <cstring>

namespace {

tmd::MetadDef define(int64_t ncv, const int32_t *kind, const int32_t *atoms, const int32_t *bins, const double *gmin, const double *gmax,
                     const double *sigma) {
  return tmd::metad_define(ncv, kind, atoms, bins, gmin, gmax, sigma);
}

}  // namespace

extern "C" {

// returns the length of the message ("" = accepted), copied to `why` (at most cap - 1 characters)
int mm_validate(int64_t natoms, int64_t ncv, const int32_t *kind, const int32_t *atoms, const int32_t *bins, const double *gmin,
                const double *gmax, const double *sigma, char *why, int cap) {
  const std::string s = tmd::metad_validate(natoms, ncv, kind, atoms, bins, gmin, gmax, sigma);
  std::strncpy(why, s.c_str(), (size_t)cap - 1);
  why[cap - 1] = 0;
  return (int)s.size();
}

// What one lane of the bias kernel computes, for every row: pos [N][3], one grid.  out = (V, s_0, s_1, dV_0, dV_1);
// row_atom [8], row_force [8][3]; returns the number of rows.
int mm_bias(int64_t ncv, const int32_t *kind, const int32_t *atoms, const int32_t *bins, const double *gmin, const double *gmax,
            const double *sigma, const double *grid, const double *pos, const double *box, double *out, int32_t *row_atom,
            double *row_force) {
  const tmd::MetadDef D = define(ncv, kind, atoms, bins, gmin, gmax, sigma);
  double x[tmd::kMetadMaxCv][4][3], g[tmd::kMetadMaxCv][4][3], s[tmd::kMetadMaxCv] = {0.0, 0.0}, dV[tmd::kMetadMaxCv];
  for (int c = 0; c < tmd::kMetadMaxCv; ++c)
    for (int a = 0; a < 4; ++a)
      for (int k = 0; k < 3; ++k) x[c][a][k] = (c < D.ncv && D.atom[c][a] >= 0) ? pos[3 * (size_t)D.atom[c][a] + k] : 0.0;
  tmd::metad_cvs(D, x, box, s, g);
  out[0] = tmd::metad_interp(D, grid, s, dV);
  out[1] = s[0];
  out[2] = s[1];
  out[3] = dV[0];
  out[4] = dV[1];
  for (int t = 0; t < D.nrows; ++t) {
    double f[3];
    tmd::metad_row_force(D, t, dV, g, f);
    row_atom[t] = D.row_atom[t];
    for (int k = 0; k < 3; ++k) row_force[3 * t + k] = f[k];
  }
  return D.nrows;
}

// What the node kernel does with one hill (s0, w), for every node of one grid in place; returns the doubles per node
int mm_deposit(int64_t ncv, const int32_t *kind, const int32_t *atoms, const int32_t *bins, const double *gmin, const double *gmax,
               const double *sigma, double *grid, const double *s0, double w) {
  const tmd::MetadDef D = define(ncv, kind, atoms, bins, gmin, gmax, sigma);
  const int W = tmd::metad_width(D);
  const int64_t nodes = tmd::metad_nodes(D);
  for (int64_t n = 0; n < nodes; ++n) {
    int k[tmd::kMetadMaxCv] = {(int)n, 0};
    if (D.ncv == 2) {
      k[0] = (int)(n / D.axis[1].nodes);
      k[1] = (int)(n % D.axis[1].nodes);
    }
    double add[4];
    tmd::metad_gauss(D, k, s0, w, add);
    for (int c = 0; c < W; ++c) grid[W * n + c] = grid[W * n + c] + add[c];
  }
  return W;
}

double mm_height(double height, double V, double kdt, int plain) { return tmd::metad_height(height, V, kdt, plain); }
}
