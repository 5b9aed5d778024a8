// The rebuild chain's host decisions (list_build.hip: plan_chain): which binning a replica uses, how the build is cut into
// blocks, and the environment knobs that steer both — free of HIP so that they also compile for the host alone
// (tests/chain_plan_host.cpp).  One rule each for a lone chain and for a row of the batched chain (ChainRepT).
#pragma once

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace tmd {

constexpr int kPrepSmallMaxCells = 4096;   // the one-block binning (prep_small_kernel) holds the cells' counts and starts in LDS
constexpr int kPrepSmallMaxAtoms = 8192;   // ... and one CU bins more atoms slower than four parallel launches (list_build.hip)
constexpr int kScanPlaceMaxCells = 12288;  // cells whose prefix a block of scan_place_kernel can hold in LDS (48 KB)
constexpr int kMaxBuildBlocks = 16384;     // blocks of one build launch; grids with more cells loop over them
constexpr int kSplitCells = 1100;          // grids up to here: two blocks per cell, so that ~2 000 waves are in flight
constexpr int kBatchFullCells = 3000;      // cells of a whole batched launch from which the chip is full at one block per cell

// Read by every enqueue (tests switch them within a process).  The splits: 0 = not set, else 1..8.
struct ChainKnobs {
  bool prep_small;        // TMDHIP_PREP_SMALL=0: no one-launch binning
  bool batch_prep_small;  // TMDHIP_BATCH_PREP_SMALL=1: the batched chain bins small systems in one launch too
  int build_split;        // TMDHIP_BUILD_SPLIT: blocks per cell, lone and batched
  int batch_build_split;  // TMDHIP_BATCH_BUILD_SPLIT: blocks per cell of the batched chain (TMDHIP_BUILD_SPLIT goes first)
  bool together;          // TMDHIP_REPLICA_REBUILDS=together: all replicas rebuild when one has to (chain_any)
};
inline ChainKnobs read_chain_knobs() {
  const auto split = [](const char *e) { return e ? std::max(1, std::min(std::atoi(e), 8)) : 0; };
  const char *ps = std::getenv("TMDHIP_PREP_SMALL"), *bps = std::getenv("TMDHIP_BATCH_PREP_SMALL"),
             *tog = std::getenv("TMDHIP_REPLICA_REBUILDS");
  return {!(ps && std::atoi(ps) == 0), bps && std::atoi(bps) != 0, split(std::getenv("TMDHIP_BUILD_SPLIT")),
          split(std::getenv("TMDHIP_BATCH_BUILD_SPLIT")), tog && std::strcmp(tog, "together") == 0};
}

// The values are those of ChainRepT::mode in the batched chain's device table.
enum class Binning : int {
  OwnChain = -1,   // (batched only) the batched kernels do not cover this replica: it keeps a chain of its own
  OneLaunch = 0,   // prep_small
  TwoLaunch = 1,   // bin_members + scan_place; the build clears the cell counts for the next one (clears_counts)
  FourLaunch = 2,  // bin_count + scan_cells + fill_cells + place_sorted
};
// members_allocated: the replica holds the two-launch binning's member arrays for this grid.  A lone replica saves launches with
// the one-block binning (44 us on its one CU at 5 184 atoms); a batch shares its launches and bins in parallel: two launches
// wherever they apply (profiles/r06_replica_batch.txt).
inline Binning choose_binning(int natoms, int ncell, bool cell_cap_fallback, bool members_allocated, const ChainKnobs &k, bool batched) {
  const bool two = !cell_cap_fallback && ncell <= kScanPlaceMaxCells && members_allocated;
  const bool one = k.prep_small && natoms <= kPrepSmallMaxAtoms && ncell <= kPrepSmallMaxCells;
  if (!batched) return one ? Binning::OneLaunch : two ? Binning::TwoLaunch : Binning::FourLaunch;
  if (ncell > kMaxBuildBlocks) return Binning::OwnChain;  // (more cells than one block per cell covers)
  if (two && !(one && k.batch_prep_small)) return Binning::TwoLaunch;
  return one ? Binning::OneLaunch : Binning::OwnChain;
}
// bin_members counts into cells it expects to be zero; the build of the same chain zeroes them again behind it
inline bool clears_counts(Binning b) { return b == Binning::TwoLaunch; }

// split: blocks per cell; blocks: of the build launch (batched: of this replica's row); looped: more cells than blocks
struct BuildCut { int split, blocks; bool looped; };
// Blocks per cell, measured (water boxes of 5 184 / 12 288 / 41 472 atoms = 343 / 729 / 2 197 cells, us per MD step at split 1,
// 2, 4): 29.7 27.7 (28-37) / 37.8 35.5 35.0 / 43.0 44.6 48.3.  Cutting small grids finer because the chip idles behind a batched
// chain is slower (12 288 atoms x 8 / 5 184 atoms x 16 at 2 / 4 / 8 blocks per cell: 92.7 / 97.7 / 105.8 and 98.5 / 99.9 / 110.2).
inline BuildCut choose_build(int ncell, const ChainKnobs &k, bool batched) {
  int split = k.build_split ? k.build_split : (batched && k.batch_build_split) ? k.batch_build_split : ncell <= kSplitCells ? 2 : 1;
  // THE TWO RULES DIFFER: a batched row falls back to one block per cell when its BLOCKS exceed kMaxBuildBlocks, a lone chain only
  // when its CELLS do (the looped kernel): TMDHIP_BUILD_SPLIT=8 at 3 000 cells is 24 000 blocks alone, 3 000 in a batch.  Kept as found.
  if (batched ? ncell * split > kMaxBuildBlocks : ncell > kMaxBuildBlocks) split = 1;
  const bool looped = !batched && ncell > kMaxBuildBlocks;
  return {split, looped ? kMaxBuildBlocks : ncell * split, looped};
}
// Many replicas in one launch (always so with TMDHIP_REPLICA_REBUILDS=together): the chip is as full as under one big box, where
// ONE block per cell is the fastest cut (T = 54 us x blocks per cell + 111 us at C3's 6 859 cells, profiles/r06_build_experiments.txt);
// two per cell are for a replica that rebuilds alone.  (Which block builds an atom's row does not change the row.)
inline bool batch_single_block_per_cell(long total_cells, const ChainKnobs &k) {
  return total_cells >= kBatchFullCells && !k.build_split && !k.batch_build_split;
}

// One launch per kernel serves rows[0 .. nsel) when there are several, all covered, and all of one binning and kernel variant.
template <typename Row>
inline bool batch_covers(const Row *rows, int nsel) {
  for (int k = 0; k < nsel; ++k)
    if ((rows[k].mode != Binning::OneLaunch && rows[k].mode != Binning::TwoLaunch) || rows[k].mode != rows[0].mode ||
        rows[k].wskin != rows[0].wskin || rows[k].lpas3 != rows[0].lpas3) return false;
  return nsel > 1;
}

}  // namespace tmd
