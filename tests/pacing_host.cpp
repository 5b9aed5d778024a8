// Host build of torchmd_amd/csrc/pacing.h for tests/test_pacing_host.py: the chain-skip decision of the pacing host
// (pace_decide, next_seq) behind a plain C interface, compiled with the system C++ compiler.
#include "pacing.h"

extern "C" {

// hp: the eight host-mapped words of a replica.  out[0] = skip_chain (0 / 1), out[1] = this step's sequence number.
void pc_decide(const unsigned *hp, unsigned seq, int seq_valid, int follows, int timed_out, int prev_skipped, unsigned *out) {
  const tmd::PaceStep p = tmd::pace_decide(hp, seq, seq_valid != 0, follows != 0, timed_out != 0, prev_skipped != 0);
  out[0] = p.skip_chain ? 1u : 0u;
  out[1] = p.seq;
}

unsigned pc_next_seq(unsigned seq) { return tmd::next_seq(seq); }

}  // extern "C"
