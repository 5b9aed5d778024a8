// Host build of torchmd_amd/csrc/gb_math.h for tests/test_gb_host.py: the per-pair functions and the per-atom closes of the
// generalized-Born kernels behind a plain C interface, in double and in float, compiled with the system C++ compiler.
// With -DGB_MATH_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined by the test): it walks a
// small cluster through all three passes on heap arrays and prints the energies.
#include "gb_math.h"

#include <cstdio>
#include <vector>

extern "C" {

double gb_t_f64(double r, double rho_i, double sig_j) { return tmd::gb_pair_t<double>(r, rho_i, sig_j); }
double gb_t3_f64(double r, double rho_i, double sig_j) { return tmd::gb_pair_t3<double>(r, rho_i, sig_j); }
float gb_t_f32(float r, float rho_i, float sig_j) { return tmd::gb_pair_t<float>(r, rho_i, sig_j); }
float gb_t3_f32(float r, float rho_i, float sig_j) { return tmd::gb_pair_t3<float>(r, rho_i, sig_j); }

// out = (G, g, h)
void gb_pair_f64(double r2, double pqq, double Bi, double Bj, double *out) {
  const tmd::GbPair<double> o = tmd::gb_pair_energy<double>(r2, pqq, Bi, Bj);
  out[0] = o.G, out[1] = o.g, out[2] = o.h;
}
void gb_pair_f32(float r2, float pqq, float Bi, float Bj, float *out) {
  const tmd::GbPair<float> o = tmd::gb_pair_energy<float>(r2, pqq, Bi, Bj);
  out[0] = o.G, out[1] = o.g, out[2] = o.h;
}

// out = (B, c)
void gb_born(double I, double radius, double *out) { tmd::gb_close_born(I, radius, out[0], out[1]); }
// out = (E_SA, b)
void gb_chain(double bsum, double radius, double sa, double B, double c, double *out) {
  out[0] = tmd::gb_close_chain(bsum, radius, sa, B, c, out[1]);
}

// The three passes on one structure, in the kernels' order of operations (d = x_j - x_i, sums over j in index order):
// pos [n][3], q (with sqrt(k_e) folded in), radii, scale, sa [n]; B, F [n][3] and E[2] = (GB, SA) out.
void gb_all_f64(int n, const double *pos, const double *q, const double *radii, const double *scale, const double *sa, double p,
                double *B, double *F, double *E) {
  std::vector<double> rho(n), sig(n), c(n), b(n);
  for (int i = 0; i < n; ++i) rho[i] = radii[i] - tmd::kGbOffset, sig[i] = scale[i] * rho[i];
  for (int i = 0; i < n; ++i) {
    double acc = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double dx = pos[3 * j] - pos[3 * i], dy = pos[3 * j + 1] - pos[3 * i + 1], dz = pos[3 * j + 2] - pos[3 * i + 2];
      acc += tmd::gb_pair_t<double>(std::sqrt((dx * dx + dy * dy) + dz * dz), rho[i], sig[j]);
    }
    tmd::gb_close_born(0.5 * acc, radii[i], B[i], c[i]);
  }
  E[0] = E[1] = 0.0;
  for (int i = 0; i < n; ++i) {
    double bacc = 0.0, f[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) {
      const double d[3] = {pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]};
      const tmd::GbPair<double> o = tmd::gb_pair_energy<double>((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], p * q[i] * q[j], B[i], B[j]);
      E[0] += 0.5 * o.G;
      bacc += o.h * B[j];
      for (int k = 0; k < 3; ++k) f[k] += o.g * d[k];
    }
    E[1] += tmd::gb_close_chain(bacc, radii[i], sa[i], B[i], c[i], b[i]);
    for (int k = 0; k < 3; ++k) F[3 * i + k] = f[k];
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      if (j == i) continue;
      const double d[3] = {pos[3 * j] - pos[3 * i], pos[3 * j + 1] - pos[3 * i + 1], pos[3 * j + 2] - pos[3 * i + 2]};
      const double r = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      const double s = -(b[i] * tmd::gb_pair_t3<double>(r, rho[i], sig[j]) + b[j] * tmd::gb_pair_t3<double>(r, rho[j], sig[i])) / r;
      for (int k = 0; k < 3; ++k) F[3 * i + k] += s * d[k];
    }
}
}

#ifdef GB_MATH_MAIN
int main() {
  // a dense cluster on a jittered lattice (spacing 1.1 A: overlapping pairs, and engulfed ones between the large and small atoms)
  const int n = 48;
  std::vector<double> pos(3 * n), q(n), radii(n), scale(n), sa(n), B(n), F(3 * n);
  unsigned s = 12345u;
  auto rnd = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0;
  };
  for (int i = 0; i < n; ++i) {
    pos[3 * i] = 1.1 * (i % 4) + 0.6 * rnd();
    pos[3 * i + 1] = 1.1 * ((i / 4) % 4) + 0.6 * rnd();
    pos[3 * i + 2] = 1.1 * (i / 16) + 0.6 * rnd();
    q[i] = 18.2 * (1.6 * rnd() - 0.8);
    radii[i] = i % 3 == 0 ? 1.2 : i % 3 == 1 ? 1.7 : 1.8;
    scale[i] = i % 3 == 0 ? 0.85 : i % 3 == 1 ? 0.72 : 0.96;
    sa[i] = 4.0 * 3.14159265358979323846 * 0.0054 * (radii[i] + 1.4) * (radii[i] + 1.4);
  }
  double E[2];
  gb_all_f64(n, pos.data(), q.data(), radii.data(), scale.data(), sa.data(), -(1.0 - 1.0 / 78.5), B.data(), F.data(), E);
  double fsum[3] = {0.0, 0.0, 0.0}, fabs_sum = 0.0;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) fsum[k] += F[3 * i + k], fabs_sum += std::fabs(F[3 * i + k]);
  float o32[3];
  gb_pair_f32(2.25f, -1.0f, 1.5f, 2.0f, o32);
  std::printf("E_GB %.17g E_SA %.17g sumF %.3e %.3e %.3e of %.3e t32 %.9g G32 %.9g\n", E[0], E[1], fsum[0], fsum[1], fsum[2], fabs_sum,
              (double)gb_t_f32(2.0f, 1.11f, 1.2f), (double)o32[0]);
  const bool ok = std::isfinite(E[0]) && std::isfinite(E[1]) && E[0] < 0.0 && E[1] > 0.0 &&
                  std::fabs(fsum[0]) + std::fabs(fsum[1]) + std::fabs(fsum[2]) < 1e-10 * fabs_sum;
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
#endif
