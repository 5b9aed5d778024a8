// Are the charges of a system a function of the LJ class?  Plain C++ (no HIP): context.hip decides with it, once per atom
// set, whether the lean fp32 pair kernel may take the charge products of a pair from its LDS class table instead of the
// gathered records (pair_fast_kernel.h: QTAB); tests/charge_class_host.cpp calls it on the host.
//
// The kernel's results must not change by a bit, so "the same charge" means the same fp32 BIT PATTERN: -0.0 and +0.0 differ,
// two NaNs are equal exactly when their payloads are.
#pragma once

#include <cstdint>
#include <cstring>

namespace tmd {

// qs: the scaled charges q * sqrt(k_e) as they go into the .w of the cell-sorted records (null: all zero); types[i] in
// 0 .. ntypes - 1 (an atom outside that range makes the answer "no").  qclass[t] receives the charge of the first atom of
// class t, +0.0 for a class without atoms.  True when every atom carries the bits of its class's charge; qclass is filled
// in either case.
inline bool charges_by_class(int natoms, const int32_t *types, const float *qs, int ntypes, float *qclass) {
  if (ntypes <= 0 || (natoms > 0 && !types)) return false;
  constexpr int kSeenMax = 256;  // (classes per context: tmdhip_create)
  if (ntypes > kSeenMax) return false;
  bool seen[kSeenMax] = {};
  uint32_t bits[kSeenMax] = {};
  bool ok = true;
  for (int i = 0; i < natoms; ++i) {
    const int t = types[i];
    if (t < 0 || t >= ntypes) {
      ok = false;
      continue;
    }
    uint32_t b = 0;
    if (qs) std::memcpy(&b, &qs[i], sizeof(b));
    if (!seen[t]) {
      seen[t] = true;
      bits[t] = b;
    } else if (bits[t] != b) {
      ok = false;
    }
  }
  for (int t = 0; t < ntypes; ++t) std::memcpy(&qclass[t], &bits[t], sizeof(float));
  return ok;
}

}  // namespace tmd
