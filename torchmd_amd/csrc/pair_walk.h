// The two generic walks over the nonbonded pair set, each written once: the Verlet-list rows and the all-pairs tiles.  The force
// kernels (pair_generic.hip: list_pair_kernel, allpairs_kernel) and the virial kernels (virial.hip: virial_list_kernel,
// virial_allpairs_kernel) call them with what they accumulate per pair, so both walk the same pairs in the same order by
// construction.  The lean kernels (pair_fast_kernel.h, pair_lean_f64.hip) have a loop shape of their own.
#pragma once

#include "engine.h"

namespace tmd {

template <typename R>
struct ListLane {
  int a, sub, lane;  // the lane's atom (cell-sorted slot), its place among the atom's LPA lanes, its place in the wave
  bool active;       // a < n
  typename Vec<R>::T4 pi;
};

// ---- the Verlet-list rows --------------------------------------------------------------------------
// Blocks of 256 threads, dynamic LDS = ntypes^2 table entries.  LPA lanes cooperate on one atom (strided over its list),
// APW = 64 / LPA atoms per wave.  The neighbour stream is read with one coalesced 256-B load per wave and iteration; UNROLL
// iterations are issued together so that their index loads and the dependent position gathers overlap (memory-level
// parallelism), and the pair maths is predicated instead of branched.
//   own(a, pi)                           once for an active lane, after its own atom is loaded
//   entry(dx, dy, dz, r2s, hit, qq, ab)  per visited entry, padding included: r2s = 1 and hit = false where nothing is to add
template <typename R, int LPA, typename Own, typename Entry>
__device__ __forceinline__ ListLane<R> walk_list_rows(int n, const typename Vec<R>::T4 *__restrict__ sorted, const int *__restrict__ stype,
                                                      int ntypes, const typename Vec<R>::T2 *__restrict__ tab,
                                                      const unsigned *__restrict__ nlist, const int *__restrict__ nneigh, int maxn,
                                                      const PairConsts<R> &c, Own &&own, Entry &&entry) {
  using R4 = typename Vec<R>::T4;
  using R2 = typename Vec<R>::T2;
  constexpr int APW = 64 / LPA;
  constexpr int UNROLL = 4;
  extern __shared__ __align__(16) unsigned char smem[];
  R2 *stab = reinterpret_cast<R2 *>(smem);
  for (int t = threadIdx.x; t < ntypes * ntypes; t += blockDim.x) stab[t] = tab[t];
  __syncthreads();

  ListLane<R> L;
  L.lane = threadIdx.x & 63;
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  L.a = wave * APW + L.lane / LPA;
  L.sub = L.lane % LPA;
  L.active = L.a < n;
  const int aself = L.active ? L.a : 0;
  L.pi.x = L.pi.y = L.pi.z = L.pi.w = 0;
  int nn = 0, trow = 0;
  if (L.active) {
    L.pi = sorted[L.a];
    nn = nneigh[L.a];
    trow = stype[L.a] * ntypes;
    own(L.a, L.pi);
  }
  const R4 pi = L.pi;
  const int sub = L.sub;
  int nmax = nn;
#pragma unroll
  for (int o = 32; o >= LPA; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o, 64));
  const int nkk = (nmax + LPA - 1) / LPA;
  const unsigned *row = nlist + (size_t)wave * maxn * APW + L.lane * 4;  // + (kk / 4) * 256 + kk % 4

  for (int kk0 = 0; kk0 < nkk; kk0 += UNROLL) {
    unsigned ent[UNROLL];
    R4 pj[UNROLL];
    bool valid[UNROLL];
    int jdx[UNROLL], tj[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) ent[u] = (kk0 + u < nkk) ? row[(size_t)(kk0 >> 2) * 256 + u] : 0u;
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      valid[u] = (kk0 + u) * LPA + sub < nn;
      jdx[u] = valid[u] ? (int)((ent[u] & kEntryOffMask) >> 4) : aself;
      pj[u] = sorted[jdx[u]];
      tj[u] = !valid[u] ? 0 : (ntypes <= kEntryTypes ? (int)(ent[u] >> kEntryTypeShift) : stype[jdx[u]]);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const R dx = min_image(pi.x - pj[u].x, c.box[0], c.invbox[0]);
      const R dy = min_image(pi.y - pj[u].y, c.box[1], c.invbox[1]);
      const R dz = min_image(pi.z - pj[u].z, c.box[2], c.invbox[2]);
      const R r2 = norm2(dx, dy, dz);
      const bool hit = valid[u] && (r2 <= c.r2max);
      const R2 ab = stab[trow + tj[u]];
      const R r2s = hit ? r2 : R(1);
      entry(dx, dy, dz, r2s, hit, pi.w * pj[u].w, ab);
    }
  }
  return L;
}

// ---- the all-pairs tiles ---------------------------------------------------------------------------
// One wave per block, grid = (ceil(N / 64), nsplit[, replicas]): lane = atom i = 64 blockIdx.x + lane, the j range
// [blockIdx.y jchunk, + jchunk) streamed through LDS in tiles of 64 (broadcast reads).  Every (i, j) with i != j is visited from
// i's side only.  pos / c: this replica's (the caller offsets them).
//   hit(dx, dy, dz, r2, qq, ab, j)  per pair inside the cutoff that is not excluded, in ascending j
//
// Round 5: small systems run ~1 000 of these waves for a few hundred atoms — 64 x 16 pairs each — so a wave's life is
// its chain of memory round trips, not its arithmetic (688-atom alanine dipeptide: 12 us per launch).  The chain was:
// own atom + exclusion offsets -> the exclusion row scanned entry by entry up to the wave's j range (one dependent load
// each: ~20 for a solute atom) -> barrier -> the j tile -> per hit a load of the LJ table from global memory.  Now:
// ONE batch holds the own atom, the exclusion offsets and the first j tile; a second one the first eight entries of
// the exclusion row (tested against every tile from registers; longer rows read the rest per tile); the LJ table is
// staged in LDS (up to kAllpairsLdsTypes classes).  Same arithmetic on the same values: results are unchanged.
constexpr int kAllpairsLdsTypes = 16;  // LJ classes whose table the all-pairs walk stages in LDS (2 / 4 KB)
template <typename R, typename Hit>
__device__ __forceinline__ void walk_allpairs_tiles(int n, const R *__restrict__ pos, const R *__restrict__ qs, const int *__restrict__ types,
                                                    int ntypes, const typename Vec<R>::T2 *__restrict__ tab,
                                                    const int *__restrict__ excl_off, const int *__restrict__ excl_idx,
                                                    const PairConsts<R> &c, int jchunk, Hit &&on_hit) {
  using R4 = typename Vec<R>::T4;
  constexpr int kExReg = 8;
  __shared__ R4 sj[64];
  __shared__ int st[64];
  __shared__ typename Vec<R>::T2 s_tab[kAllpairsLdsTypes * kAllpairsLdsTypes];
  const int lane = threadIdx.x;
  const int i = blockIdx.x * 64 + lane;
  const bool active = i < n;
  const int jbeg = blockIdx.y * jchunk;
  const int jend = min(n, jbeg + jchunk);
  const bool tab_in_lds = ntypes <= kAllpairsLdsTypes;
  R xi = 0, yi = 0, zi = 0, qi = 0;
  int trow = 0;
  int ebeg = 0, eend = 0;
  R4 v0;  // this lane's record of the first tile
  v0.x = v0.y = v0.z = v0.w = R(0);
  int t0 = 0;
  {
    const int jl = jbeg + lane;
    if (jl < jend) {
      v0.x = pos[3 * jl + 0];
      v0.y = pos[3 * jl + 1];
      v0.z = pos[3 * jl + 2];
      v0.w = qs[jl];
      t0 = types[jl];
    }
  }
  if (active) {
    xi = pos[3 * i + 0];
    yi = pos[3 * i + 1];
    zi = pos[3 * i + 2];
    qi = qs[i];
    trow = types[i] * ntypes;
    ebeg = excl_off[i];
    eend = excl_off[i + 1];
  }
  if (tab_in_lds)
    for (int t = lane; t < ntypes * ntypes; t += 64) s_tab[t] = tab[t];
  int ex[kExReg];
#pragma unroll
  for (int k = 0; k < kExReg; ++k) ex[k] = (ebeg + k < eend) ? excl_idx[ebeg + k] : -1;

  for (int j0 = jbeg; j0 < jend; j0 += 64) {
    __syncthreads();
    const int jl = j0 + lane;
    if (j0 == jbeg) {
      sj[lane] = v0;
      st[lane] = t0;
    } else if (jl < jend) {
      R4 v;
      v.x = pos[3 * jl + 0];
      v.y = pos[3 * jl + 1];
      v.z = pos[3 * jl + 2];
      v.w = qs[jl];
      sj[lane] = v;
      st[lane] = types[jl];
    }
    __syncthreads();
    // exclusion mask of this tile for atom i: the row's first entries from registers, the rest (long rows: proteins) read here
    unsigned long long skip = 0;
#pragma unroll
    for (int k = 0; k < kExReg; ++k) {
      const unsigned d = (unsigned)(ex[k] - j0);
      if (d < 64u) skip |= 1ull << d;
    }
    for (int e = ebeg + kExReg; e < eend; ++e) {
      const int x = excl_idx[e];
      if (x >= j0 + 64) break;  // (rows are sorted)
      if (x >= j0) skip |= 1ull << (x - j0);
    }
    if (i >= j0 && i < j0 + 64) skip |= 1ull << (i - j0);
    const int tile = min(64, jend - j0);
    for (int k = 0; k < tile; ++k) {
      const R4 pj = sj[k];
      const R dx = min_image(xi - pj.x, c.box[0], c.invbox[0]);
      const R dy = min_image(yi - pj.y, c.box[1], c.invbox[1]);
      const R dz = min_image(zi - pj.z, c.box[2], c.invbox[2]);
      const R r2 = norm2(dx, dy, dz);
      const bool hit = active && !((skip >> k) & 1ull) && (r2 <= c.r2max);
      if (hit) {
        const typename Vec<R>::T2 ab = tab_in_lds ? s_tab[trow + st[k]] : tab[trow + st[k]];
        on_hit(dx, dy, dz, r2, qi * pj.w, ab, j0 + k);
      }
    }
  }
}

}  // namespace tmd
