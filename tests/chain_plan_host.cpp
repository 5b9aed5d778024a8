// Host build of torchmd_amd/csrc/chain_plan.h for tests/test_chain_plan_host.py: the rebuild chain's binning and build-cut
// rules and its knobs behind a plain C interface, compiled with the system C++ compiler.
#include "chain_plan.h"

using namespace tmd;

namespace {
// knobs as five ints: prep_small, batch_prep_small, build_split, batch_build_split, together
ChainKnobs knobs_of(const int *k) { return {k[0] != 0, k[1] != 0, k[2], k[3], k[4] != 0}; }
struct Row {
  Binning mode;
  int wskin, lpas3;
};
}  // namespace

extern "C" {

void cp_read_knobs(int *out) {  // (from the environment)
  const ChainKnobs k = read_chain_knobs();
  out[0] = k.prep_small, out[1] = k.batch_prep_small, out[2] = k.build_split, out[3] = k.batch_build_split, out[4] = k.together;
}

int cp_binning(int natoms, int ncell, int cell_cap_fallback, int members_allocated, const int *knobs, int batched) {
  return (int)choose_binning(natoms, ncell, cell_cap_fallback != 0, members_allocated != 0, knobs_of(knobs), batched != 0);
}

int cp_clears_counts(int binning) { return clears_counts((Binning)binning) ? 1 : 0; }

void cp_build(int ncell, const int *knobs, int batched, int *out) {  // out: split, blocks, looped
  const BuildCut c = choose_build(ncell, knobs_of(knobs), batched != 0);
  out[0] = c.split, out[1] = c.blocks, out[2] = c.looped ? 1 : 0;
}

int cp_batch_single_block_per_cell(long total_cells, const int *knobs) {
  return batch_single_block_per_cell(total_cells, knobs_of(knobs)) ? 1 : 0;
}

int cp_batch_covers(int nsel, const int *mode, const int *wskin, const int *lpas3) {
  Row rows[64];
  for (int k = 0; k < nsel && k < 64; ++k) rows[k] = {(Binning)mode[k], wskin[k], lpas3[k]};
  return batch_covers(rows, nsel) ? 1 : 0;
}

}  // extern "C"
