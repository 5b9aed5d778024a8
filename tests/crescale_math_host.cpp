// Host build of torchmd_amd/csrc/crescale_math.h for tests/test_crescale_host.py: the step of eps = ln V, the box factor and the
// rigid move of one molecule (the loops of one thread of rescale_molecules_kernel, written with the header's functions) behind a
// plain C interface, compiled with the system C++ compiler and -ffp-contract=off (the header's `#pragma clang fp contract(off)`).
// With -DCRESCALE_HOST_MAIN it is a stand-alone program that moves a few molecules of its own and prints the result as hex
// floats: the form that runs under -fsanitize=address,undefined.
#include "crescale_math.h"

#include <cstdio>
#include <vector>

namespace {

// pos, vel [n][3] in place, mass [n]; k[2] = (sum m v^2 / 2 before, after)
template <typename R>
void move_molecule(int n, R *pos, R *vel, const R *mass, const double *s, double *k) {
  double sm = 0, sx[3] = {0, 0, 0}, sv[3] = {0, 0, 0}, kb = 0, ka = 0;
  for (int a = 0; a < n; ++a) {
    const double m = (double)mass[a];
    if (!(m > 0.0)) continue;
    sm += m;
    for (int c = 0; c < 3; ++c) sx[c] += m * (double)pos[3 * a + c], sv[c] += m * (double)vel[3 * a + c];
    kb += tmd::crescale_mv2(m, (double)vel[3 * a], (double)vel[3 * a + 1], (double)vel[3 * a + 2]);
  }
  double dx[3] = {0, 0, 0}, dv[3] = {0, 0, 0};
  if (sm > 0.0)
    for (int c = 0; c < 3; ++c) dx[c] = tmd::crescale_shift_pos(s[c], sx[c], sm), dv[c] = tmd::crescale_shift_vel(s[c], sv[c], sm);
  for (int a = 0; a < n; ++a) {
    for (int c = 0; c < 3; ++c) pos[3 * a + c] = tmd::crescale_apply<R>(pos[3 * a + c], dx[c]);
    if (!((double)mass[a] > 0.0)) continue;
    for (int c = 0; c < 3; ++c) vel[3 * a + c] = tmd::crescale_apply<R>(vel[3 * a + c], dv[c]);
    ka += tmd::crescale_mv2((double)mass[a], (double)vel[3 * a], (double)vel[3 * a + 1], (double)vel[3 * a + 2]);
  }
  k[0] = 0.5 * kb, k[1] = 0.5 * ka;
}

}  // namespace

extern "C" {

double cm_delta_eps(double beta, double dt_over_tau, double p0, double pint, double kT, double vol, double xi, int stochastic) {
  return tmd::crescale_delta_eps(beta, dt_over_tau, p0, pint, kT, vol, xi, stochastic);
}

double cm_mu(double delta_eps) { return tmd::crescale_mu(delta_eps); }

double cm_shift_pos(double s, double sum_mx, double sum_m) { return tmd::crescale_shift_pos(s, sum_mx, sum_m); }

double cm_shift_vel(double s, double sum_mv, double sum_m) { return tmd::crescale_shift_vel(s, sum_mv, sum_m); }

void cm_move_f64(int n, double *pos, double *vel, const double *mass, const double *s, double *k) { move_molecule<double>(n, pos, vel, mass, s, k); }

void cm_move_f32(int n, float *pos, float *vel, const float *mass, const double *s, double *k) { move_molecule<float>(n, pos, vel, mass, s, k); }
}

#ifdef CRESCALE_HOST_MAIN
// Molecules of 1, 3, 4 (the fourth atom massless) and 65 atoms from a fixed linear congruential stream; one line per molecule:
// n, then pos, vel [n][3] after the move and k[2], all as hex floats.  The test rebuilds the inputs and compares with its model.
int main() {
  unsigned long long state = 12345;
  auto next = [&state]() {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(state >> 11) / 9007199254740992.0;  // [0, 1)
  };
  const int sizes[4] = {1, 3, 4, 65};
  const double s[3] = {1.001, 0.9985, 1.0};
  const double de = tmd::crescale_delta_eps(3000.0, 0.02, 1.4e-5, -3.0e-3, 0.596, 27000.0, 0.7, 1);
  std::printf("%a %a\n", de, tmd::crescale_mu(de));
  for (int n : sizes) {
    std::vector<double> pos(3 * n), vel(3 * n), mass(n);
    for (int a = 0; a < n; ++a) {
      mass[a] = (n == 4 && a == 3) ? 0.0 : 1.0 + 15.0 * next();
      for (int c = 0; c < 3; ++c) pos[3 * a + c] = 40.0 * next(), vel[3 * a + c] = 0.02 * (next() - 0.5);
    }
    double k[2];
    move_molecule<double>(n, pos.data(), vel.data(), mass.data(), s, k);
    std::printf("%d", n);
    for (double x : pos) std::printf(" %a", x);
    for (double x : vel) std::printf(" %a", x);
    std::printf(" %a %a\n", k[0], k[1]);
  }
  return 0;
}
#endif
