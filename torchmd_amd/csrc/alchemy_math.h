// Alchemical decoupling: the soft-core pair function of a solute-environment pair, the full-strength pair and
// the 1-4 Coulomb term of the solute's own rows, shared by the kernels of alchemy.hip and a host program
// (tests/alchemy_math_host.cpp).  Plain C++ templated on the real type R of the pair arithmetic.  The host program is compiled
// with floating-point contraction off; the kernels contract as the engine's own value arithmetic does (pair_math.h).
//
//   sigma^6 = A / B,  s = r^6 + alpha sigma^6 (1 - lv)
//   U_lj = lv (A / s^2 - B / s) sw(r)          sw: the context's switching function at the true r
//   U_el = le qq g(r)                          g = 1/r, or 1/r + k_rf r^2 - c_rf; no soft core on the charges
//   dU/dlv = (A / s^2 - B / s) sw - lv (-2 A / s^3 + B / s^2) alpha sigma^6 sw,   dU/dle = qq g(r)
// The force on atom i of the pair is -d fs with d = x_i - x_j (pair_terms' convention).  lv = 1: s = r^6 exactly and the
// Lennard-Jones part is pair_terms' own sequence of operations on 1/r.  A = 0: no Lennard-Jones part.  r = 0 at lv < 1: the
// Lennard-Jones energy is finite, the force is zero and the charge part is left out (it has no soft core: the staging rule
// le = 0 or lv = 1 keeps such pairs from carrying charge).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace tmd {

constexpr uint32_t kAlchLj = 1u, kAlchEl = 2u;  // AlchConsts::parts

template <typename R>
struct AlchConsts {
  R r2max;  // the engine's decision threshold on |d|^2 (+inf: no cutoff)
  R switch_dist, inv_switch_range;
  R krf, crf;
  R alpha;
  int32_t switch_on, switch_reference_mode, rfa;
  uint32_t parts;
};

template <typename R>
struct AlchPair {
  R ulj;  // lv (A/s^2 - B/s) sw
  R gel;  // qq g(r): the charge energy at le = 1, and dU/dle
  R dv;   // dU/dlv
  R fs;   // force on i = -d fs, at (lv, le)
};

__host__ __device__ inline float alch_sqrt(float x) { return sqrtf(x); }
__host__ __device__ inline double alch_sqrt(double x) { return sqrt(x); }

// 1 / sqrt(x): on the device the engine's own (pair_math.h: fast_rsqrt), on the host the correctly rounded pair of operations
__host__ __device__ inline float alch_rsqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __frsqrt_rn(x);
#else
  return 1.0f / sqrtf(x);
#endif
}
__host__ __device__ inline double alch_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double y = __builtin_amdgcn_rsq(x);
  const double h = __builtin_fma(-(x * y), y, 1.0);
  return __builtin_fma(y, h * __builtin_fma(h, 0.375, 0.5), y);
#else
  return 1.0 / sqrt(x);
#endif
}

// sw(r) and dsw/dr (pair_terms' polynomial); false, 1 and 0 below the switching distance
template <typename R>
__host__ __device__ inline bool alch_switch(const AlchConsts<R> &c, R r, R &sw, R &dsw) {
  sw = R(1), dsw = R(0);
  if (!(c.switch_on && r > c.switch_dist)) return false;
  const R t = (r - c.switch_dist) * c.inv_switch_range;
  sw = R(1) + t * t * t * (R(-10) + t * (R(15) - t * R(6)));
  dsw = t * t * (R(-30) + t * (R(60) - t * R(30))) * c.inv_switch_range;
  return true;
}

// One pair at squared distance r2 (inside the cutoff: the caller decides) at the coupling (lv, le).
template <typename R>
__host__ __device__ inline AlchPair<R> alch_pair(const AlchConsts<R> &c, R r2, R qq, R A, R B, R lv, R le) {
  AlchPair<R> o{R(0), R(0), R(0), R(0)};
  R dEdr = R(0);
  if (lv == R(1)) {  // the plain 12-6 form: pair_terms' operations
    const R rinv = alch_rsqrt(r2), rinv2 = rinv * rinv, r = r2 * rinv;
    const R rinv6 = rinv2 * rinv2 * rinv2;
    if ((c.parts & kAlchLj) && A != R(0)) {
      R elj = (A * rinv6 - B) * rinv6;
      R f = (R(-12) * A * rinv6 + R(6) * B) * rinv6 * rinv;
      R sw, dsw;
      if (alch_switch(c, r, sw, dsw)) {
        // the reference's explicit force divides the switching term by r once more (pair_terms)
        f = sw * f + elj * dsw * (c.switch_reference_mode ? rinv : R(1));
        elj *= sw;
      }
      dEdr += f;
      o.ulj = elj;
      o.dv = elj - ((R(-2) * A * rinv6 + B) * (rinv6 * rinv6)) * (c.alpha * (A / B)) * sw;
    }
    if (c.parts & kAlchEl) {
      if (c.rfa) {
        dEdr += le * (qq * (R(2) * c.krf * r - rinv2));
        o.gel = qq * (rinv + c.krf * r2 - c.crf);
      } else {
        const R eel = qq * rinv;
        dEdr -= le * (eel * rinv);
        o.gel = eel;
      }
    }
    o.fs = dEdr * rinv;
    return o;
  }
  // soft core: everything in powers of r^2, so that r = 0 is an ordinary argument
  R fs = R(0);
  const R r = alch_sqrt(r2), rinv = r > R(0) ? R(1) / r : R(0);
  if ((c.parts & kAlchLj) && A != R(0)) {
    const R r6 = r2 * r2 * r2, sig6 = A / B, a6 = c.alpha * sig6;
    const R s = r6 + a6 * (R(1) - lv), sinv = R(1) / s;
    const R u = (A * sinv - B) * sinv;                    // A/s^2 - B/s
    const R du = (R(-2) * A * sinv + B) * (sinv * sinv);  // d/ds
    R sw, dsw;
    if (alch_switch(c, r, sw, dsw) && c.switch_reference_mode) dsw *= rinv;
    o.ulj = lv * u * sw;
    o.dv = u * sw - lv * du * a6 * sw;
    // (1/r) dU/dr = lv [du 6 r^4 sw + u dsw / r]
    fs = lv * (du * (R(6) * (r2 * r2)) * sw + u * dsw * rinv);
  }
  if ((c.parts & kAlchEl) && r > R(0)) {
    const R rinv2 = rinv * rinv;
    if (c.rfa) {
      fs += le * (qq * (R(2) * c.krf * r - rinv2)) * rinv;
      o.gel = qq * (rinv + c.krf * r2 - c.crf);
    } else {
      const R eel = qq * rinv;
      fs -= le * (eel * rinv) * rinv;
      o.gel = eel;
    }
  }
  o.fs = fs;
  return o;
}

// The Lennard-Jones energy of the pair at another coupling lv (the foreign-energy pass: no force, no derivative); sw from
// alch_switch.  lv = 0 gives exactly 0.
template <typename R>
__host__ __device__ inline R alch_lj_at(R r2, R A, R B, R a6, R sw, R lv) {
  const R r6 = r2 * r2 * r2;
  const R s = r6 + a6 * (R(1) - lv), sinv = R(1) / s;
  return lv * ((A * sinv - B) * sinv) * sw;
}

// The solute's 1-4 Coulomb term (bonded_math.h: pair14_term's charge part): E = qq / r / scee, no cutoff.  Returns E; fs as above.
template <typename R>
__host__ __device__ inline R alch_pair14(R r2, R qq, R scee, R &fs) {
  const R rinv = R(1) / alch_sqrt(r2);
  const R ee = qq * rinv / scee;
  fs = (-(ee * rinv)) * rinv;
  return ee;
}

// One entry of a solute atom's intra row: kind 0, a non-excluded solute-solute pair at full strength (qq, A, B; the context's
// cutoff, switch and electrostatics); kind 1, the charge part of a 1-4 pair (qq, scee).  `partner` is an atom index; the pair's
// vector is always formed as x_low - x_high, so that its two ends see each other's negatives bit for bit.
struct AlchEntry {
  int32_t partner, kind;
  double qq, A, B, scee;
};

}  // namespace tmd

// ---- host side: validation and the solute's rows ----
#include <algorithm>
#include <string>
#include <vector>

namespace tmd {

// What tmdhip_set_alchemical refuses in the numbers themselves ("" = nothing).
inline std::string alch_validate(int64_t natoms, int64_t nrep, int64_t ns, const int32_t *atoms, const double *lam_v, const double *lam_e,
                                 double alpha) {
  if (natoms <= 0 || nrep <= 0 || ns <= 0) return "bad size";
  if (!atoms || !lam_v || !lam_e) return "null table";
  if (!(alpha >= 0.0) || !std::isfinite(alpha)) return "alpha must be finite and not negative";
  std::vector<char> seen((size_t)natoms, 0);
  for (int64_t k = 0; k < ns; ++k) {
    const int32_t a = atoms[k];
    if (a < 0 || a >= natoms) return "solute atom " + std::to_string(k) + ": index out of range";
    if (seen[a]) return "atom " + std::to_string(a) + " is given twice";
    seen[a] = 1;
  }
  for (int64_t r = 0; r < nrep; ++r) {
    if (!(lam_v[r] >= 0.0 && lam_v[r] <= 1.0) || !(lam_e[r] >= 0.0 && lam_e[r] <= 1.0))
      return "replica " + std::to_string(r) + ": every lambda must lie in [0, 1]";
    if (lam_e[r] != 0.0 && lam_v[r] != 1.0)
      return "replica " + std::to_string(r) + ": the charges have no soft core, so lambda_elec must be 0 or lambda_vdw must be 1";
  }
  return "";
}

// Closure of the solute under a list of index tuples (`width` atoms each): a tuple that names a solute atom names only solute
// atoms.  slot[a] >= 0 marks the solute.  "" = closed.
inline std::string alch_closed(const std::vector<int32_t> &slot, const int32_t *idx, int64_t count, int width, const char *what) {
  for (int64_t t = 0; t < count; ++t) {
    int in = 0;
    for (int k = 0; k < width; ++k) {
      const int32_t a = idx[t * width + k];
      if (a < 0 || a >= (int32_t)slot.size()) return std::string(what) + " " + std::to_string(t) + ": atom index out of range";
      in += slot[a] >= 0;
    }
    if (in != 0 && in != width)
      return std::string(what) + " " + std::to_string(t) + " joins the solute to the environment: the solute must be closed under the topology";
  }
  return "";
}

// The intra rows of the solute atoms (atoms ascending; row t belongs to atoms[t]): first the non-excluded solute-solute pairs by
// partner index, then the atom's 1-4 entries by their index in the 1-4 table.  Every pair appears in both rows.
// excl_off / excl_idx: the context's exclusion CSR (both directions stored).  qs[t]: the scaled charge of atoms[t];
// cls[t]: its Lennard-Jones class; tabA / tabB [ntypes x ntypes].  mul(a, b): the product in the context's precision.
template <typename Mul>
inline void alch_build_csr(const std::vector<int32_t> &atoms, const int32_t *excl_off, const int32_t *excl_idx, const double *qs,
                           const int32_t *cls, int ntypes, const double *tabA, const double *tabB, int64_t n14,
                           const int32_t *pair14, const double *scee, Mul mul, std::vector<int32_t> &off,
                           std::vector<AlchEntry> &ent) {
  const size_t ns = atoms.size();
  auto row = [&](int32_t a) { return (size_t)(std::lower_bound(atoms.begin(), atoms.end(), a) - atoms.begin()); };
  off.assign(ns + 1, 0);
  ent.clear();
  std::vector<std::vector<AlchEntry>> rows(ns);
  for (size_t t = 0; t < ns; ++t) {
    const int32_t a = atoms[t];
    for (size_t u = 0; u < ns; ++u) {
      const int32_t b = atoms[u];
      if (b == a) continue;
      if (excl_off && std::binary_search(excl_idx + excl_off[a], excl_idx + excl_off[a + 1], b)) continue;
      const size_t k = (size_t)cls[t] * ntypes + cls[u];
      rows[t].push_back(AlchEntry{b, 0, mul(qs[t], qs[u]), tabA ? tabA[k] : 0.0, tabB ? tabB[k] : 0.0, 1.0});
    }
  }
  for (int64_t p = 0; p < n14; ++p) {
    const int32_t i = pair14[2 * p], j = pair14[2 * p + 1];
    const size_t ti = row(i), tj = row(j);
    const double qq = mul(qs[ti], qs[tj]);
    rows[ti].push_back(AlchEntry{j, 1, qq, 0.0, 0.0, scee[p]});
    rows[tj].push_back(AlchEntry{i, 1, qq, 0.0, 0.0, scee[p]});
  }
  for (size_t t = 0; t < ns; ++t) {
    off[t + 1] = off[t] + (int32_t)rows[t].size();
    ent.insert(ent.end(), rows[t].begin(), rows[t].end());
  }
}

}  // namespace tmd
