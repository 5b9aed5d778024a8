// Host program around torchmd_amd/csrc/charge_class.h for tests/test_charge_class_host.py: the test that decides whether a
// context's charges are a function of the LJ class (charges_by_class), compiled with the system C++ compiler — the header
// needs no HIP.  A stand-alone program, so that it can also be built with -fsanitize=address,undefined and run as it is.
//
// stdin:   ntypes natoms has_charges
//          natoms lines "type bits" (bits: the fp32 charge as 8 hex digits)
// stdout:  "1" or "0" (the answer), then ntypes words of 8 hex digits: the class charges
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "charge_class.h"

int main() {
  int ntypes = 0, natoms = 0, has_q = 0;
  if (std::scanf("%d %d %d", &ntypes, &natoms, &has_q) != 3 || natoms < 0 || ntypes > 4096) return 2;
  // (exactly natoms elements: a read or write past either array is what the sanitizer build is for)
  std::vector<int32_t> types((size_t)natoms);
  std::vector<float> qs((size_t)natoms);
  for (int i = 0; i < natoms; ++i) {
    int t = 0;
    uint32_t b = 0;
    if (std::scanf("%d %" SCNx32, &t, &b) != 2) return 2;
    types[i] = t;
    std::memcpy(&qs[i], &b, sizeof(b));
  }
  std::vector<float> qclass((size_t)(ntypes > 0 ? ntypes : 0));
  const bool ok = tmd::charges_by_class(natoms, types.data(), has_q ? qs.data() : nullptr, ntypes, qclass.data());
  std::printf("%d", ok ? 1 : 0);
  for (int t = 0; t < ntypes && ntypes <= 256; ++t) {
    uint32_t b = 0;
    std::memcpy(&b, &qclass[t], sizeof(b));
    std::printf(" %08" PRIx32, b);
  }
  std::printf("\n");
  return 0;
}
