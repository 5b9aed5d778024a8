// Host build of torchmd_amd/csrc/restraint_math.h for tests/test_restraints_host.py: the per-entry arithmetic of the restraint
// kernel, the validation of the tables and the per-atom rows behind a plain C interface, compiled with the system C++
// compiler and -ffp-contract=off (the kernel's `#pragma clang fp contract(off)`).
#include "restraint_math.h"

#include <cstring>

extern "C" {

double rm_position(const double *x, const double *ref, const double *box, double k, double *f) {
  double g[3];
  const double e = tmd::restraint_position(x, ref, box, k, g);
  for (int c = 0; c < 3; ++c) f[c] = g[c];
  return e;
}

double rm_distance(const double *xi, const double *xj, const double *box, double k, double r0, double *fi) {
  double g[3];
  const double e = tmd::restraint_distance(xi, xj, box, k, r0, g);
  for (int c = 0; c < 3; ++c) fi[c] = g[c];
  return e;
}

// returns the length of the message ("" = accepted), copied to `why` (at most cap - 1 characters)
int rm_validate(int64_t natoms, int64_t nrep, int64_t npos, int64_t ndist, const int32_t *pos_atom, const double *pos_ref,
                const double *pos_k, const int32_t *dist_pair, const double *dist_r0, const double *dist_k, char *why, int cap) {
  const std::string s = tmd::restraint_validate(natoms, nrep, npos, ndist, pos_atom, pos_ref, pos_k, dist_pair, dist_r0, dist_k);
  std::strncpy(why, s.c_str(), (size_t)cap - 1);
  why[cap - 1] = 0;
  return (int)s.size();
}

// atoms [<= npos + 2 ndist], off [that + 1], ent [npos + 2 ndist][4]; returns the number of rows
int rm_rows(int64_t npos, int64_t ndist, const int32_t *pos_atom, const int32_t *dist_pair, int32_t *atoms, int32_t *off, int32_t *ent) {
  std::vector<int32_t> a, o;
  std::vector<tmd::RestraintEntry> e;
  tmd::restraint_build_csr(npos, ndist, pos_atom, dist_pair, a, o, e);
  std::memcpy(atoms, a.data(), sizeof(int32_t) * a.size());
  std::memcpy(off, o.data(), sizeof(int32_t) * o.size());
  std::memcpy(ent, e.data(), sizeof(tmd::RestraintEntry) * e.size());
  return (int)a.size();
}
}
