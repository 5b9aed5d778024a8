// The j split of the tiled all-pairs launches (pair_generic.hip: launch_allpairs, virial.hip: pressure) — free of HIP so that it
// also compiles for the host alone (tests/allpairs_split_host.cpp).
#pragma once

#include <algorithm>
#include <cstdlib>

namespace tmd {

// TMDHIP_ALLPAIRS_WAVES: the wave target of the split; 0 (or less) = not set
inline int read_allpairs_waves() {
  const char *e = std::getenv("TMDHIP_ALLPAIRS_WAVES");
  return e ? std::atoi(e) : 0;
}
inline int allpairs_waves_knob() {  // (read once per process)
  static const int v = read_allpairs_waves();
  return v;
}

// grid = (nb, nsplit, nrep) one-wave blocks: block (x, y) walks the atoms 64 x .. of i against the j range [y jchunk, (y + 1) jchunk).
// The j range is split so that ~1024 waves are in flight even for a few hundred atoms (each block then walks a short j range; the
// partial sums of the blocks of one i are combined by the caller).
// (round 5: the wave target grows with the work — n^2 x replicas pairs / 512, 1 024 .. 4 096 waves: a batch of 16
// alanine-dipeptide replicas ran 880 waves of 144 iterations each, one per SIMD, nothing to hide a wave's latency
// behind.  Measured, us per MD step at 1 024 / 2 048 / 4 096 / 8 192 waves (profiles/r05_allpairs_waves.txt): ala2 x 16
// 71.1 / 43.3 / 37.8 / 44.2, tests/water x 64 46.0 / 29.5 / 23.0 / 25.7, x 16 18.5 / 15.3 / 15.2 / 15.6.)
inline void allpairs_split(int n, int nrep, int &nb, int &nsplit, int &jchunk, int waves_knob = allpairs_waves_knob()) {
  nb = (n + 63) / 64;
  const double pairs = (double)n * (double)n * (double)nrep;
  const int want_waves = waves_knob > 0 ? waves_knob : (int)std::min(4096.0, std::max(1024.0, pairs / 512.0));
  nsplit = std::max(1, std::min((n + 15) / 16, want_waves / std::max(nb * nrep, 1)));
  jchunk = ((n + nsplit - 1) / nsplit + 15) / 16 * 16;
  nsplit = (n + jchunk - 1) / jchunk;
}

}  // namespace tmd
