// Host build of torchmd_amd/csrc/allpairs_split.h for tests/test_allpairs_split_host.py: the j split of the all-pairs
// launches behind a plain C interface, compiled with the system C++ compiler.
#include "allpairs_split.h"

using namespace tmd;

extern "C" {

int aps_read_waves() { return read_allpairs_waves(); }  // (from the environment)

// out [nmax][3] = (nb, nsplit, jchunk) for n = 1 .. nmax
void aps_split_range(int nmax, int nrep, int waves_knob, int *out) {
  for (int n = 1; n <= nmax; ++n) allpairs_split(n, nrep, out[3 * (n - 1)], out[3 * (n - 1) + 1], out[3 * (n - 1) + 2], waves_knob);
}

}  // extern "C"
