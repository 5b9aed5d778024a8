// Host build of torchmd_amd/csrc/pacing.h for tests/test_pacing_host.py: the chain-skip decision of the pacing host
// (pace_decide, next_seq) and the grid geometry of a fused pair + step launch (fused_grid) behind a plain C interface, compiled
// with the system C++ compiler.
#include "pacing.h"

extern "C" {

// hp: the eight host-mapped words of a replica.  out[0] = skip_chain (0 / 1), out[1] = this step's sequence number.
void pc_decide(const unsigned *hp, unsigned seq, int seq_valid, int follows, int timed_out, int prev_skipped, unsigned *out) {
  const tmd::PaceStep p = tmd::pace_decide(hp, seq, seq_valid != 0, follows != 0, timed_out != 0, prev_skipped != 0);
  out[0] = p.skip_chain ? 1u : 0u;
  out[1] = p.seq;
}

unsigned pc_next_seq(unsigned seq) { return tmd::next_seq(seq); }

int pc_fast_threads() { return tmd::kFastThreads; }

// out = {pair_blocks, units, step_blocks} of a replica's share of a fused pair + step launch
void pc_fused_grid(int natoms, int apw, int lpa, int bonded, int *out) {
  const tmd::FusedGrid g = tmd::fused_grid(natoms, apw, lpa, bonded);
  out[0] = g.pair_blocks;
  out[1] = g.units;
  out[2] = g.step_blocks;
}

}  // extern "C"
