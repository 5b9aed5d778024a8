// Host build of torchmd_amd/csrc/alchemy_math.h for tests/test_alchemy_host.py: the pair functions behind a plain C interface,
// in double and in float, and the validation and CSR builder of tmdhip_set_alchemical, compiled with the system C++ compiler.
// With -DALCHEMY_MATH_MAIN the same source is a stand-alone program (built with -fsanitize=address,undefined by the test): it
// evaluates a small solute in a cloud of environment atoms on heap arrays, builds the rows and prints the energies.
#include "alchemy_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {
template <typename R>
tmd::AlchConsts<R> consts(double r2max, double switch_dist, double cutoff, double krf, double crf, double alpha, int reference, int rfa,
                          unsigned parts) {
  tmd::AlchConsts<R> c;
  c.r2max = (R)r2max;
  c.switch_on = switch_dist > 0 && cutoff > 0;
  c.switch_dist = (R)switch_dist;
  c.inv_switch_range = c.switch_on ? (R)(1.0 / (cutoff - switch_dist)) : R(0);
  c.krf = (R)krf, c.crf = (R)crf, c.alpha = (R)alpha;
  c.switch_reference_mode = reference, c.rfa = rfa, c.parts = parts;
  return c;
}
}  // namespace

extern "C" {

// cfg = (switch_dist, cutoff, krf, crf, alpha, reference, rfa, parts); out = (ulj, gel, dv, fs)
void alch_pair_f64(const double *cfg, double r2, double qq, double A, double B, double lv, double le, double *out) {
  const auto c = consts<double>(1e300, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], (int)cfg[5], (int)cfg[6], (unsigned)cfg[7]);
  const tmd::AlchPair<double> o = tmd::alch_pair<double>(c, r2, qq, A, B, lv, le);
  out[0] = o.ulj, out[1] = o.gel, out[2] = o.dv, out[3] = o.fs;
}
void alch_pair_f32(const double *cfg, float r2, float qq, float A, float B, float lv, float le, float *out) {
  const auto c = consts<float>(1e30, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], (int)cfg[5], (int)cfg[6], (unsigned)cfg[7]);
  const tmd::AlchPair<float> o = tmd::alch_pair<float>(c, r2, qq, A, B, lv, le);
  out[0] = o.ulj, out[1] = o.gel, out[2] = o.dv, out[3] = o.fs;
}
double alch_lj_at_f64(const double *cfg, double r2, double A, double B, double lv) {
  const auto c = consts<double>(1e300, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], (int)cfg[5], (int)cfg[6], (unsigned)cfg[7]);
  double sw, dsw;
  tmd::alch_switch(c, std::sqrt(r2), sw, dsw);
  return tmd::alch_lj_at<double>(r2, A, B, c.alpha * (A / B), sw, lv);
}
// out = (E, fs)
void alch_pair14_f64(double r2, double qq, double scee, double *out) { out[0] = tmd::alch_pair14<double>(r2, qq, scee, out[1]); }
void alch_pair14_f32(float r2, float qq, float scee, float *out) { out[0] = tmd::alch_pair14<float>(r2, qq, scee, out[1]); }

// the refusal ("" = none) copied into msg[cap]
void alch_validate_c(long natoms, long nrep, long ns, const int32_t *atoms, const double *lv, const double *le, double alpha, char *msg,
                     int cap) {
  const std::string s = tmd::alch_validate(natoms, nrep, ns, atoms, lv, le, alpha);
  std::snprintf(msg, (size_t)cap, "%s", s.c_str());
}
void alch_closed_c(long natoms, long ns, const int32_t *atoms, const int32_t *idx, long count, int width, char *msg, int cap) {
  std::vector<int32_t> slot((size_t)natoms, -1);
  for (long k = 0; k < ns; ++k) slot[atoms[k]] = (int32_t)k;
  const std::string s = tmd::alch_closed(slot, idx, count, width, "tuple");
  std::snprintf(msg, (size_t)cap, "%s", s.c_str());
}
// The rows of the solute `atoms` (ascending): returns the number of entries; off[ns + 1]; partner, kind [cap]; prm [cap][4] =
// (qq, A, B, scee).  f32 != 0: charge products rounded as an fp32 context rounds them.
long alch_csr_c(long ns, const int32_t *atoms, const int32_t *excl_off, const int32_t *excl_idx, const double *qs, const int32_t *cls,
                int ntypes, const double *tabA, const double *tabB, long n14, const int32_t *pair14, const double *scee, int f32,
                int32_t *off, int32_t *partner, int32_t *kind, double *prm, long cap) {
  std::vector<int32_t> a(atoms, atoms + ns), o;
  std::vector<tmd::AlchEntry> ent;
  if (f32)
    tmd::alch_build_csr(a, excl_off, excl_idx, qs, cls, ntypes, tabA, tabB, n14, pair14, scee,
                        [](double x, double y) { return (double)((float)x * (float)y); }, o, ent);
  else
    tmd::alch_build_csr(a, excl_off, excl_idx, qs, cls, ntypes, tabA, tabB, n14, pair14, scee, [](double x, double y) { return x * y; }, o,
                        ent);
  for (long t = 0; t <= ns; ++t) off[t] = o[(size_t)t];
  for (size_t e = 0; e < ent.size() && (long)e < cap; ++e) {
    partner[e] = ent[e].partner, kind[e] = ent[e].kind;
    prm[4 * e] = ent[e].qq, prm[4 * e + 1] = ent[e].A, prm[4 * e + 2] = ent[e].B, prm[4 * e + 3] = ent[e].scee;
  }
  return (long)ent.size();
}
}

#ifdef ALCHEMY_MATH_MAIN
int main() {
  // a five-atom chain (1-2, 1-3 excluded, one 1-4 pair) among 40 environment atoms, at three couplings and at r = 0
  const int ns = 5, ne = 40, n = ns + ne, T = 3;
  std::vector<double> pos(3 * n), q(n);
  std::vector<int32_t> cls(n), atoms(ns);
  unsigned s = 2024u;
  auto rnd = [&s]() {
    s = s * 1664525u + 1013904223u;
    return (double)(s >> 8) / 16777216.0;
  };
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = i < ns ? 6.0 + 1.4 * i * (k == 0) : 12.0 * rnd();
    q[i] = 18.2 * (i % 2 ? 0.4 : -0.4);
    cls[i] = i < ns ? i % 2 : 2;
    if (i < ns) atoms[i] = i;
  }
  for (int k = 0; k < 3; ++k) pos[3 * ns + k] = pos[k];  // the first environment atom sits on the first solute atom
  std::vector<double> tabA(T * T), tabB(T * T);
  for (int a = 0; a < T; ++a)
    for (int b = 0; b < T; ++b) tabA[a * T + b] = 5.0e5 + 1.0e5 * (a + b), tabB[a * T + b] = 600.0 + 50.0 * (a + b);
  std::vector<int32_t> eoff(n + 1, 0), eidx;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < ns; ++j)
      if (i < ns && j != i && std::abs(i - j) <= 3) eidx.push_back(j);
    eoff[i + 1] = (int32_t)eidx.size();
  }
  const int32_t pair14[4] = {0, 3, 1, 4};
  const double scee[2] = {1.2, 1.2};
  std::vector<int32_t> off;
  std::vector<tmd::AlchEntry> ent;
  tmd::alch_build_csr(atoms, eoff.data(), eidx.data(), q.data(), cls.data(), T, tabA.data(), tabB.data(), 2, pair14, scee,
                      [](double a, double b) { return a * b; }, off, ent);
  const auto c = consts<double>(81.0, 7.5, 9.0, 1e-3, 0.16, 0.5, 0, 1, tmd::kAlchLj | tmd::kAlchEl);
  const auto c32 = consts<float>(81.0, 7.5, 9.0, 1e-3, 0.16, 0.5, 1, 1, tmd::kAlchLj | tmd::kAlchEl);
  bool ok = true;
  const double lams[3][2] = {{1.0, 1.0}, {0.5, 0.0}, {0.0, 0.0}};
  for (const auto &lam : lams) {
    double e = 0.0, dv = 0.0, f32sum = 0.0;
    for (int i = 0; i < ns; ++i)
      for (int j = ns; j < n; ++j) {
        const double d[3] = {pos[3 * i] - pos[3 * j], pos[3 * i + 1] - pos[3 * j + 1], pos[3 * i + 2] - pos[3 * j + 2]};
        const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        if (!(r2 <= c.r2max) || (r2 == 0.0 && lam[0] == 1.0)) continue;
        const size_t k = (size_t)cls[j] * T + cls[i];
        const tmd::AlchPair<double> o = tmd::alch_pair<double>(c, r2, q[i] * q[j], tabA[k], tabB[k], lam[0], lam[1]);
        const tmd::AlchPair<float> o32 = tmd::alch_pair<float>(c32, (float)r2, (float)(q[i] * q[j]), (float)tabA[k], (float)tabB[k],
                                                               (float)lam[0], (float)lam[1]);
        e += o.ulj + lam[1] * o.gel, dv += o.dv, f32sum += (double)o32.fs;
        if (r2 == 0.0) ok = ok && o.fs == 0.0 && std::isfinite(o.ulj) && std::isfinite(o.dv);
      }
    double intra = 0.0;
    for (int t = 0; t < ns; ++t)
      for (int en = off[t]; en < off[t + 1]; ++en) {
        const tmd::AlchEntry &E = ent[en];
        if (E.partner < atoms[t]) continue;
        const double d[3] = {pos[3 * t] - pos[3 * E.partner], pos[3 * t + 1] - pos[3 * E.partner + 1], pos[3 * t + 2] - pos[3 * E.partner + 2]};
        const double r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        double fs;
        if (E.kind == 0) {
          const tmd::AlchPair<double> o = tmd::alch_pair<double>(c, r2, E.qq, E.A, E.B, 1.0, 1.0);
          intra += o.ulj + o.gel;
        } else {
          intra += tmd::alch_pair14<double>(r2, E.qq, E.scee, fs);
        }
      }
    std::printf("lv %.1f le %.1f: cross %.17g dU/dlv %.17g intra %.17g sum fs32 %.9g entries %zu\n", lam[0], lam[1], e, dv, intra, f32sum,
                ent.size());
    ok = ok && std::isfinite(e) && std::isfinite(dv) && std::isfinite(intra) && std::isfinite(f32sum);
    if (lam[0] == 0.0) ok = ok && e == 0.0;
  }
  char msg[256];
  const double lv[2] = {1.0, 0.5}, le[2] = {1.0, 0.5};
  alch_validate_c(n, 2, ns, atoms.data(), lv, le, 0.5, msg, sizeof msg);
  ok = ok && std::strlen(msg) > 0;  // (replica 1 breaks the staging rule)
  std::printf(ok ? "ok\n" : "FAILED\n");
  return ok ? 0 : 1;
}
#endif
