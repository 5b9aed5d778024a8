// Host build of torchmd_amd/csrc/virial_math.h for tests/test_pressure_host.py: the per-pair contribution to the molecular virial,
// the per-mode factor of the PME reciprocal part, the last arithmetic of the fold and the validation of the molecule table behind
// a plain C interface, compiled with the system C++ compiler and -ffp-contract=off (the header's `#pragma clang fp contract(off)`).
#include "virial_math.h"

#include <cstring>

extern "C" {

void vm_pair_f64(const double *d, double fs, const double *delta, double *w) { tmd::virial_pair<double>(d[0], d[1], d[2], fs, delta, w); }

void vm_pair_f32(const float *d, float fs, const double *delta, double *w) { tmd::virial_pair<float>(d[0], d[1], d[2], fs, delta, w); }

double vm_mode_factor(double m2, double ma2, double beta) { return tmd::virial_mode_factor(m2, ma2, beta); }

void vm_finish(const double *kin, const double *w, const double *box, double *out) { tmd::virial_finish(kin, w, box, out); }

// returns the length of the message ("" = accepted), copied to `why` (at most cap - 1 characters); mol_of [natoms] is written
int vm_validate(int64_t natoms, int64_t nmol, const int32_t *offsets, const int32_t *members, int32_t *mol_of, char *why, int cap) {
  std::vector<int32_t> m;
  const std::string s = tmd::virial_validate_molecules(natoms, nmol, offsets, members, m);
  if (s.empty()) std::memcpy(mol_of, m.data(), sizeof(int32_t) * m.size());
  std::strncpy(why, s.c_str(), (size_t)cap - 1);
  why[cap - 1] = 0;
  return (int)s.size();
}
}
