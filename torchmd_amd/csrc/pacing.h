// Chain skipping (ListCheck, engine.h): the decision the pacing host makes per step, free of HIP so that it also compiles for
// the host alone (tests/pacing_host.cpp).  The device side and the waiting are pace_behind_device's (md_loop.hip).
#pragma once

namespace tmd {

constexpr double kChainSkipNear = 0.75;  // "near": beyond this fraction of the displacement limit (0.15 A of room at
                                         // skin 1.2: 2.2 x the largest per-step move seen in the water box, 9.5
                                         // standard deviations of a hydrogen's thermal velocity at 300 K)

// the sequence number after `seq`: never 0, which means "nothing published yet"
inline unsigned next_seq(unsigned seq) { return seq + 1u == 0u ? 1u : seq + 1u; }

struct PaceStep {
  bool skip_chain;  // leave the rebuild chain out of this step
  unsigned seq;     // this step's sequence number
};

// hp: the replica's host-mapped words — [0] progress, [1 + parity] the last sequence number in which an atom was near its
// limit, [3 + parity] the last one that rebuilt the list (parity = seq & 1).  `seq`: the previous step's number, whose report has
// arrived unless `timed_out`; `follows`: nothing has moved since that step.  No chain when nobody was near its limit in the
// previous step — or when that step rebuilt the list (with its chain in place: every displacement is one step old now).
inline PaceStep pace_decide(const volatile unsigned *hp, unsigned seq, bool seq_valid, bool follows, bool timed_out, bool prev_skipped) {
  bool skip_chain = false;
  if (seq_valid && follows && !timed_out) {
    const bool near = hp[1 + (seq & 1u)] == seq, rebuilt = hp[3 + (seq & 1u)] == seq;
    skip_chain = !near || (rebuilt && !prev_skipped);
  }
  return {skip_chain, next_seq(seq)};
}

}  // namespace tmd
