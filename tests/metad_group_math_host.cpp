// Host build of torchmd_amd/csrc/cv_math.h for tests/test_metad_groups_host.py: the validator, the switch, and one application
// of a grouped bias walked as the kernels of metad_group.hip walk it (the tables of cv_build, the lanes, splits, butterflies,
// meets and folds of reduce.h spelled out), behind a plain C interface.  Compiled with the system C++ compiler and
// -ffp-contract=off (the kernels' `#pragma clang fp contract(off)`).
#include "cv_math.h"

#include <cstring>

namespace {

int put(const std::string &s, char *why, int cap) {
  std::strncpy(why, s.c_str(), (size_t)cap - 1);
  why[cap - 1] = 0;
  return (int)s.size();
}

// the 64-lane xor butterfly of reduce.h: every lane ends with the same bits
void butterfly(double *v) {
  for (int o = 32; o > 0; o >>= 1) {
    double t[64];
    for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ o];
    std::memcpy(v, t, sizeof(t));
  }
}

// block_sums<4, Pairwise> of one column: lanes [256]
double block_sum(const double *lanes) {
  double p[4];
  for (int w = 0; w < 4; ++w) {
    double v[64];
    std::memcpy(v, lanes + 64 * w, sizeof(v));
    butterfly(v);
    p[w] = v[0];
  }
  return (p[0] + p[1]) + (p[2] + p[3]);
}

// fold_rows of one column
double fold(const double *rows, int n) {
  double acc[64];
  for (int l = 0; l < 64; ++l) acc[l] = 0.0;
  for (int l = 0; l < 64; ++l)
    for (int b = l; b < n; b += 64) acc[l] = acc[l] + rows[b];
  butterfly(acc);
  return acc[0];
}

}  // namespace

extern "C" {

int mg_validate(int64_t natoms, int64_t ncv, const int32_t *kind, const int32_t *groups, int64_t ngroups, const int32_t *group_off,
                const int32_t *member_atom, const double *member_weight, const int32_t *bins, const double *gmin, const double *gmax,
                const double *sigma, const int32_t *coord_n, const double *r0, const double *d0, const double *dmax, char *why, int cap) {
  return put(tmd::cv_validate(natoms, ncv, kind, groups, ngroups, group_off, member_atom, member_weight, bins, gmin, gmax, sigma, coord_n,
                              r0, d0, dmax),
             why, cap);
}

int mg_check_box(double r0, int n, double d0, double dmax, const double *box, char *why, int cap) {
  return put(tmd::cv_check_box(tmd::coord_params(r0, n, d0, dmax), box), why, cap);
}

// out = (f, df/dr)
void mg_switch(double r0, int n, double d0, double dmax, double r, double *out) {
  const tmd::CoordParams P = tmd::coord_params(r0, n, d0, dmax);
  out[0] = tmd::coord_switch(P, r, out[1]);
}

int mg_nsplit(int64_t nlane, int64_t nstream) { return tmd::cv_nsplit(nlane, nstream); }

// One application for one replica: pos [N][3], one grid.  out = (V, s_0, s_1, dV_0, dV_1); row_atom [nrows] and row_force
// [nrows][3] (capacity `cap_rows`); returns the number of rows, or -1 when the definition is refused.
int mg_bias(int64_t natoms, int64_t ncv, const int32_t *kind, const int32_t *groups, int64_t ngroups, const int32_t *group_off,
            const int32_t *member_atom, const double *member_weight, const int32_t *bins, const double *gmin, const double *gmax,
            const double *sigma, const int32_t *coord_n, const double *r0, const double *d0, const double *dmax, const double *grid,
            const double *pos, const double *box, double *out, int32_t *row_atom, double *row_force, int cap_rows) {
  using namespace tmd;
  if (!cv_validate(natoms, ncv, kind, groups, ngroups, group_off, member_atom, member_weight, bins, gmin, gmax, sigma, coord_n, r0, d0,
                   dmax)
           .empty())
    return -1;
  const MetadDef D = cv_grid_define(ncv, kind, bins, gmin, gmax, sigma);
  std::vector<double> w;
  group_normalise(ngroups, group_off, member_weight, w);
  const CvTables T = cv_build(ncv, kind, groups, ngroups, group_off, member_atom, w);
  if ((int)T.atom.size() > cap_rows) return -1;
  // ---- the gather: centres, then every task of the coordination CVs
  std::vector<double> centres(3 * (size_t)ngroups);
  for (int g = 0; g < ngroups; ++g) {
    const int m0 = group_off[g], m1 = group_off[g + 1];
    const double *x0 = pos + 3 * (size_t)member_atom[m0];
    std::vector<double> lanes(3 * (size_t)kCvThreads, 0.0);
    for (int t = 0; t < kCvThreads; ++t) {
      double acc[3] = {0.0, 0.0, 0.0};
      for (int m = m0 + t; m < m1; m += kCvThreads) group_centre_add(pos + 3 * (size_t)member_atom[m], x0, box, w[(size_t)m], acc);
      for (int c = 0; c < 3; ++c) lanes[(size_t)c * kCvThreads + t] = acc[c];
    }
    for (int c = 0; c < 3; ++c) centres[3 * (size_t)g + c] = x0[c] + block_sum(lanes.data() + (size_t)c * kCvThreads);
  }
  CoordParams P[kMetadMaxCv];
  for (int c = 0; c < ncv; ++c)
    if (kind[c] == kCvCoordination) P[c] = coord_params(r0[c], coord_n[c], d0[c], dmax[c]);
  std::vector<double> grad((size_t)T.grad_doubles, 0.0), partials((size_t)T.part_rows, 0.0);
  for (const CvTask &task : T.task) {
    const CvPass &Q = T.pass[(size_t)task.pass];
    double lanes[kCvThreads];
    for (int t = 0; t < kCvThreads; ++t) {
      lanes[t] = 0.0;
      const int i = task.block * kCvThreads + t;
      if (i >= Q.nlane) continue;
      const int ai = member_atom[Q.lane0 + i];
      double val = 0.0, g[3] = {0.0, 0.0, 0.0};
      const int j0 = task.split * Q.chunk, j1 = std::min(Q.nstream, j0 + Q.chunk);
      for (int j = j0; j < j1; ++j) {
        const int aj = member_atom[Q.stream0 + j];
        if (aj == ai) continue;
        coord_pair_add(P[Q.cv], pos + 3 * (size_t)ai, pos + 3 * (size_t)aj, box, val, g);
      }
      lanes[t] = val;
      for (int c = 0; c < 3; ++c) grad[(size_t)Q.grad_off + ((size_t)task.split * Q.nlane + i) * 3 + c] = g[c];
    }
    if (Q.value) partials[(size_t)Q.part_off + (size_t)task.block * Q.nsplit + task.split] = block_sum(lanes);
  }
  // ---- the scatter: the CVs, the bias, the rows
  double s[kMetadMaxCv] = {0.0, 0.0}, gC[kMetadMaxCv][4][3], dV[kMetadMaxCv];
  for (int c = 0; c < kMetadMaxCv; ++c) {
    for (int a = 0; a < 4; ++a) gC[c][a][0] = gC[c][a][1] = gC[c][a][2] = 0.0;
    if (c >= ncv) continue;
    if (kind[c] == kCvCoordination) {
      s[c] = fold(partials.data() + T.part_off[c], T.part_n[c]);
      continue;
    }
    double X[4][3];
    for (int a = 0; a < 4; ++a)
      for (int k = 0; k < 3; ++k) X[a][k] = a < cv_arity(kind[c]) ? centres[3 * (size_t)groups[4 * c + a] + k] : 0.0;
    s[c] = cv_of_centres(kind[c], X, box, gC[c]);
  }
  out[0] = metad_interp(D, grid, s, dV);
  out[1] = s[0];
  out[2] = s[1];
  out[3] = dV[0];
  out[4] = dV[1];
  for (size_t t = 0; t < T.atom.size(); ++t) {
    double f[3] = {0.0, 0.0, 0.0};
    int e = T.ent_off[t];
    const int e1 = T.ent_off[t + 1];
    for (int c = 0; c < ncv; ++c) {
      double ds[3] = {0.0, 0.0, 0.0};
      bool any = false;
      for (; e < e1; ++e) {
        const CvEntry &E = T.ent[(size_t)e];
        if (E.cv != c) break;
        any = true;
        if (E.type == 0) {
          for (int k = 0; k < 3; ++k) ds[k] += E.w * gC[c][E.at][k];
        } else {
          double part[3] = {0.0, 0.0, 0.0};
          for (int q = 0; q < E.nsplit; ++q)
            for (int k = 0; k < 3; ++k) part[k] += grad[(size_t)E.at + (size_t)q * E.stride + k];
          for (int k = 0; k < 3; ++k) ds[k] += part[k];
        }
      }
      if (any)
        for (int k = 0; k < 3; ++k) f[k] += -dV[c] * ds[k];
    }
    row_atom[t] = T.atom[t];
    for (int k = 0; k < 3; ++k) row_force[3 * t + k] = f[k];
  }
  return (int)T.atom.size();
}
}
