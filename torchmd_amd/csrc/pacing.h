// Chain skipping (ListCheck, engine.h): the decision the pacing host makes per step, free of HIP so that it also compiles for
// the host alone (tests/pacing_host.cpp).  The device side and the waiting are pace_behind_device's (md_loop.hip).  Also the
// other pure host arithmetic of a fused pair + step launch: its launch numbers (next_seq) and its grid geometry (fused_grid).
#pragma once

namespace tmd {

constexpr double kChainSkipNear = 0.75;  // "near": beyond this fraction of the displacement limit (0.15 A of room at
                                         // skin 1.2: 2.2 x the largest per-step move seen in the water box, 9.5
                                         // standard deviations of a hydrogen's thermal velocity at 300 K)

// the sequence number after `seq`: never 0, which means "nothing published yet"
inline unsigned next_seq(unsigned seq) { return seq + 1u == 0u ? 1u : seq + 1u; }

constexpr int kFastThreads = 256;  // threads of a block of the lean fp32 pair kernel (step blocks are four waves)

// Grid geometry of ONE replica's share of a fused pair + step launch (FusedStepT, engine.h), for the lone launch and the batched
// one alike: the pair blocks (four waves of `apw` = 64 / lpa atoms) rounded up to a whole round of the 8 XCDs, and behind them the
// step blocks — per XCD's eighth one 64-atom unit for every lpa / 4 pair blocks; a unit is a block where the step blocks evaluate
// inline bonded records (bonded == 1), a wave otherwise.  The step blocks find their atoms from these numbers alone.
struct FusedGrid {
  int pair_blocks, units, step_blocks;  // (units: 64-atom units per XCD's eighth; both block counts are multiples of 8)
};
inline FusedGrid fused_grid(int natoms, int apw, int lpa, int bonded) {
  constexpr int wpb = kFastThreads / 64;
  const int waves = (natoms + apw - 1) / apw;
  const int pair_blocks = ((waves + wpb - 1) / wpb + 7) / 8 * 8;
  const int k = lpa * 64 / kFastThreads;  // pair blocks per unit (0 below 4 lanes per atom: such a launch has no step blocks)
  const int units = k > 0 ? (pair_blocks / 8 + k - 1) / k : 0;
  return {pair_blocks, units, 8 * (bonded == 1 ? units : (units + 3) / 4)};
}

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
