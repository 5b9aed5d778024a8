// Host build of torchmd_amd/csrc/group_math.h for tests/test_group_restraints_host.py: one restraint on its centres, the
// validation of the tables, the rows of the force kernel and the kernel's whole walk (centres summed in member order) behind a
// plain C interface, compiled with the system C++ compiler and -ffp-contract=off (the kernel's `#pragma clang fp contract(off)`).
#include "group_math.h"

#include <cstring>

extern "C" {

// X [4][3] (rows beyond the arity ignored), F [4][3]
double gm_restraint(int kind, const double *X, const double *box, double s0, double k, double flat, double *F) {
  double C[4][3], G[4][3];
  for (int a = 0; a < 4; ++a)
    for (int c = 0; c < 3; ++c) C[a][c] = a < tmd::group_arity(kind) ? X[3 * a + c] : 0.0;
  const double e = tmd::group_restraint(kind, C, box, s0, k, flat, G);
  for (int a = 0; a < 4; ++a)
    for (int c = 0; c < 3; ++c) F[3 * a + c] = G[a][c];
  return e;
}

// returns the length of the message ("" = accepted), copied to `why` (at most cap - 1 characters)
int gm_validate(int64_t natoms, int64_t nrep, int64_t ngroups, const int32_t *group_off, const int32_t *member_atom,
                const double *member_weight, int64_t nrest, const int32_t *kind, const int32_t *groups, const double *target,
                const double *k, const double *flat, char *why, int cap) {
  const std::string s = tmd::group_validate(natoms, nrep, ngroups, group_off, member_atom, member_weight, nrest, kind, groups, target, k, flat);
  std::strncpy(why, s.c_str(), (size_t)cap - 1);
  why[cap - 1] = 0;
  return (int)s.size();
}

// use_off [G + 1], use [<= 4 M][2], atoms [<= members], mem_off [that + 1], mem [<= members][2]; returns the number of rows
int gm_rows(int64_t ngroups, const int32_t *group_off, const int32_t *member_atom, int64_t nrest, const int32_t *kind,
            const int32_t *groups, int32_t *use_off, int32_t *use, int32_t *atoms, int32_t *mem_off, int32_t *mem) {
  std::vector<int32_t> uo, a, mo;
  std::vector<tmd::GroupUse> u;
  std::vector<tmd::GroupMember> m;
  tmd::group_build_csr(ngroups, group_off, member_atom, nrest, kind, groups, uo, u, a, mo, m);
  std::memcpy(use_off, uo.data(), sizeof(int32_t) * uo.size());
  std::memcpy(use, u.data(), sizeof(tmd::GroupUse) * u.size());
  std::memcpy(atoms, a.data(), sizeof(int32_t) * a.size());
  std::memcpy(mem_off, mo.data(), sizeof(int32_t) * mo.size());
  std::memcpy(mem, m.data(), sizeof(tmd::GroupMember) * m.size());
  return (int)a.size();
}

void gm_normalise(int64_t ngroups, const int32_t *group_off, const double *member_weight, double *w) {
  std::vector<double> v;
  tmd::group_normalise(ngroups, group_off, member_weight, v);
  std::memcpy(w, v.data(), sizeof(double) * v.size());
}

// One replica: the centres (members summed in their order), then the force kernel's walk over the rows.  pos [N][3], the tables of
// one replica [M]; centres [G][3], energy [3], forces [N][3] (added to).
void gm_energy_forces(int64_t natoms, const double *pos, const double *box, int64_t ngroups, const int32_t *group_off,
                      const int32_t *member_atom, const double *member_weight, int64_t nrest, const int32_t *kind, const int32_t *groups,
                      const double *target, const double *k, const double *flat, double *centres, double *energy, double *forces) {
  (void)natoms;
  std::vector<double> w;
  tmd::group_normalise(ngroups, group_off, member_weight, w);
  for (int64_t g = 0; g < ngroups; ++g) {
    const double *x0 = pos + 3 * (size_t)member_atom[group_off[g]];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int32_t m = group_off[g]; m < group_off[g + 1]; ++m) tmd::group_centre_add(pos + 3 * (size_t)member_atom[m], x0, box, w[(size_t)m], acc);
    for (int c = 0; c < 3; ++c) centres[3 * g + c] = x0[c] + acc[c];
  }
  auto eval = [&](int m, double(&F)[4][3]) {
    double C[4][3];
    for (int a = 0; a < 4; ++a)
      for (int c = 0; c < 3; ++c) C[a][c] = a < tmd::group_arity(kind[m]) ? centres[3 * (size_t)groups[4 * m + a] + c] : 0.0;
    return tmd::group_restraint(kind[m], C, box, target[m], k[m], flat[m], F);
  };
  energy[0] = energy[1] = energy[2] = 0.0;
  for (int m = 0; m < nrest; ++m) {
    double F[4][3];
    if (k[m] > 0.0) energy[kind[m]] += eval(m, F);
  }
  std::vector<int32_t> uo, atoms, mo;
  std::vector<tmd::GroupUse> use;
  std::vector<tmd::GroupMember> mem;
  tmd::group_build_csr(ngroups, group_off, member_atom, nrest, kind, groups, uo, use, atoms, mo, mem);
  for (size_t t = 0; t < atoms.size(); ++t) {
    double f[3] = {0.0, 0.0, 0.0};
    for (int32_t e = mo[t]; e < mo[t + 1]; ++e) {
      double G[3] = {0.0, 0.0, 0.0};
      for (int32_t u = uo[(size_t)mem[(size_t)e].group]; u < uo[(size_t)mem[(size_t)e].group + 1]; ++u) {
        const int m = use[(size_t)u].index;
        if (!(k[m] > 0.0)) continue;
        double F[4][3];
        eval(m, F);
        for (int c = 0; c < 3; ++c) G[c] += F[use[(size_t)u].role][c];
      }
      for (int c = 0; c < 3; ++c) f[c] += w[(size_t)mem[(size_t)e].member] * G[c];
    }
    for (int c = 0; c < 3; ++c) forces[3 * (size_t)atoms[t] + c] += f[c];
  }
}
}
