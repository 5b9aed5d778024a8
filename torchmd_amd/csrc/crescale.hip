// The move of a virial-driven barostat (stochastic cell rescaling / Berendsen) for gfx950: every molecule follows the box
// rigidly, positions and velocities (tmdhip_rescale_molecules; the arithmetic: crescale_math.h).
//
// The box edges of replica r are multiplied by s_r,a.  Every atom of molecule I is translated by (s_a - 1) R_I,a and its
// velocity by (1 / s_a - 1) V_I,a, with R_I / V_I the MASS-WEIGHTED centre of the molecule and its velocity: the quantities
// the molecular virial (virial.hip) is defined on, not the unweighted mean tmdhip_scale_groups uses.  Distances and relative
// velocities inside a molecule do not change, so SETTLE / SHAKE / RATTLE states survive to storage rounding.  Molecules must be
// whole (no minimum image inside a molecule).
//
// Work decomposition as in mol_centre_kernel and scale_groups_kernel: one thread per molecule of up to 64 atoms, one wave per
// larger molecule (second launch, only when the caller says that such molecules exist: `has_big`), blockIdx.y = replica; the
// factors of 16 replicas travel as kernel arguments.  The table is the caller's and lives on the device, so the list of the
// larger molecules (mol_centre_kernel's `big`) is made there by big_list_kernel at every call, and 64 one-wave blocks per replica
// share it: no wave is launched for a molecule that is not on it.
//   rescale_molecules_kernel  pass 1: sum m, sum m x, sum m v in double, members in index order, and sum m v^2 over the ATOMS
//                             as they are; pass 2: x and v written back in the context's precision (one rounding), and
//                             sum m v^2 of the velocities as stored.  Per-block partials [2] of both sums.
//   rescale_fold_kernel       one wave per replica folds the partials; writes double [R][2] = (K_before, K_after).
// Fixed-order sum (reduce.h), the wave sums meet pairwise: two calls on the same state give the same bits.
//
// Edge cases:
//   a replica whose three factors are exactly 1   neither positions nor velocities are written; its two K entries are
//                                                 computed all the same (and are equal)
//   a member of mass 0 (a virtual site)           shifted in position with its molecule; its velocity is never read or
//                                                 written (it may hold anything) and it enters no sum
//   a molecule without mass                       has no centre: left where it is (tmdhip_pressure refuses such a table)
//   a member index outside [0, natoms)            skipped
// Streaming: two reads of x, v, m per atom and one write of x and v; a few microseconds at 10^5 atoms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "crescale_math.h"
#include "pair_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kBigMol = 64;  // more atoms than this: one wave per molecule

struct ScaleArgs {
  double s[kSideChunk][3];
};

constexpr int kBigBlocks = 64;  // one-wave blocks per replica that share the molecules of more than kBigMol atoms

__host__ __device__ inline int small_blocks_of(int nmol) { return (nmol + kThreads - 1) / kThreads; }

// One molecule, by one thread (BIG = false: members first .. e, stride 1) or by one wave (BIG = true: lane l takes the members
// first + l, first + l + 64, ...; all 64 lanes arrive together).  Adds sum m v^2 before and after to kb / ka of the lane.
template <typename R, bool BIG>
__device__ __forceinline__ void move_molecule(int natoms, const int *__restrict__ mem, R *__restrict__ p, R *__restrict__ v,
                                              const R *__restrict__ mass, const double (&s)[3], bool write, int first, int e, double &kb,
                                              double &ka) {
#pragma clang fp contract(off)
  constexpr int stride = BIG ? kWave : 1;
  first = max(first, 0), e = min(e, natoms);  // (a table that is not a CSR over the atoms must not reach past `mem`)
  double sm = 0, sx[3] = {0, 0, 0}, sv[3] = {0, 0, 0};
  for (int k = first; k < e; k += stride) {
    const int a = mem[k];
    if ((unsigned)a >= (unsigned)natoms) continue;
    const double m = (double)mass[a];
    if (!(m > 0.0)) continue;
    const double vx = (double)v[3 * a], vy = (double)v[3 * a + 1], vz = (double)v[3 * a + 2];
    sm += m;
    sx[0] += m * (double)p[3 * a], sx[1] += m * (double)p[3 * a + 1], sx[2] += m * (double)p[3 * a + 2];
    sv[0] += m * vx, sv[1] += m * vy, sv[2] += m * vz;
    kb += crescale_mv2(m, vx, vy, vz);
  }
  if (BIG) {
    sm = wave_sum(sm);
#pragma unroll
    for (int c = 0; c < 3; ++c) sx[c] = wave_sum(sx[c]), sv[c] = wave_sum(sv[c]);
  }
  double dx[3] = {0, 0, 0}, dv[3] = {0, 0, 0};
  if (sm > 0.0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) dx[c] = crescale_shift_pos(s[c], sx[c], sm), dv[c] = crescale_shift_vel(s[c], sv[c], sm);
  }
  for (int k = first; k < e; k += stride) {
    const int a = mem[k];
    if ((unsigned)a >= (unsigned)natoms) continue;
    const double m = (double)mass[a];
    if (write) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p[3 * a + c] = crescale_apply<R>(p[3 * a + c], dx[c]);
    }
    if (!(m > 0.0)) continue;
    const R nx = crescale_apply<R>(v[3 * a], dv[0]), ny = crescale_apply<R>(v[3 * a + 1], dv[1]), nz = crescale_apply<R>(v[3 * a + 2], dv[2]);
    ka += crescale_mv2(m, (double)nx, (double)ny, (double)nz);
    if (write) v[3 * a] = nx, v[3 * a + 1] = ny, v[3 * a + 2] = nz;
  }
}

// One wave: big[0 .. count) = the molecules of more than kBigMol atoms in index order, big[nmol] = count (ballot and prefix
// count per 64 molecules: the list does not depend on timing).  Made on the device because the table lives there.
__global__ __launch_bounds__(64) void big_list_kernel(int nmol, const int *__restrict__ off, int *__restrict__ big) {
  int count = 0;
  for (int base = 0; base < nmol; base += 64) {
    const int g = base + (int)threadIdx.x;
    const bool is_big = g < nmol && off[g + 1] - off[g] > kBigMol;
    const unsigned long long mask = __ballot(is_big);
    if (is_big) big[count + __popcll(mask & ((1ull << threadIdx.x) - 1ull))] = g;
    count += __popcll(mask);
  }
  if (threadIdx.x == 0) big[nmol] = count;
}

// big_pass = 0: thread = molecule (those of more than kBigMol atoms are left out), grid.x = ceil(nmol / 256), partial row
// blockIdx.x; big_pass = 1: kBigBlocks blocks of one wave, block b takes big[b], big[b + kBigBlocks], ..., partial row
// small_blocks + b.  blockIdx.y = replica.  partials: double [R][prows][2].
template <typename R>
__global__ __launch_bounds__(kThreads) void rescale_molecules_kernel(int natoms, int nmol, const int *__restrict__ off,
                                                                     const int *__restrict__ mem, const int *__restrict__ big,
                                                                     R *__restrict__ pos, R *__restrict__ vel, const R *__restrict__ mass,
                                                                     ScaleArgs S, int replica0, double *__restrict__ partials, int prows,
                                                                     int big_pass) {
#pragma clang fp contract(off)
  const int rl = blockIdx.y, r = replica0 + rl;
  const size_t base = (size_t)r * (size_t)natoms * 3;
  R *p = pos + base;
  R *v = vel + base;
  const double s[3] = {S.s[rl][0], S.s[rl][1], S.s[rl][2]};
  const bool write = s[0] != 1.0 || s[1] != 1.0 || s[2] != 1.0;
  double kb = 0, ka = 0;
  if (!big_pass) {
    const int g = blockIdx.x * kThreads + threadIdx.x;
    int first = 0, e = 0;
    if (g < nmol) {
      first = off[g], e = off[g + 1];
      if (e - first > kBigMol) e = first;
    }
    move_molecule<R, false>(natoms, mem, p, v, mass, s, write, first, e, kb, ka);
  } else {  // (count and the list are the same in every lane: the wave stays together)
    const int count = min(big[nmol], nmol);
    for (int i = blockIdx.x; i < count; i += gridDim.x) {
      const int g = big[i];
      if ((unsigned)g >= (unsigned)nmol) continue;
      move_molecule<R, true>(natoms, mem, p, v, mass, s, write, off[g] + (int)threadIdx.x, off[g + 1], kb, ka);
    }
  }
  const double k[2] = {kb, ka};
  double *dst = partials + ((size_t)r * prows + (big_pass ? small_blocks_of(nmol) + blockIdx.x : blockIdx.x)) * 2;
  if (big_pass) {
    block_sums<1, Meet::Pairwise>(k, dst);
  } else {
    block_sums<kThreads / 64, Meet::Pairwise>(k, dst);
  }
}

// one wave per replica folds the `nrows` partial rows that were written
__global__ __launch_bounds__(64) void rescale_fold_kernel(const double *__restrict__ partials, int prows, int nrows, double *__restrict__ record) {
#pragma clang fp contract(off)
  const int r = blockIdx.x;
  double k[2];
  fold_rows(partials + (size_t)r * prows * 2, nrows, k);
  if (threadIdx.x == 0) record[2 * (size_t)r] = 0.5 * k[0], record[2 * (size_t)r + 1] = 0.5 * k[1];
}

// the workspace: double [R][prows][2] of partials, then int [nmol + 1]: the list of big molecules and its length
inline int64_t partial_rows(int64_t nmol) { return small_blocks_of((int)nmol) + kBigBlocks; }

template <typename R>
int rescale(int64_t nreplicas, int n, void *pos, void *vel, const void *mass, const double *scale_host, int nmol, const int32_t *off,
            const int32_t *mem, int has_big, double *record, double *partials, hipStream_t st) {
  const int small = small_blocks_of(nmol), prows = (int)partial_rows(nmol);
  int *big = (int *)(partials + (size_t)nreplicas * prows * 2);
  if (has_big) hipLaunchKernelGGL(big_list_kernel, dim3(1), dim3(64), 0, st, nmol, off, big);
  for (int64_t r0 = 0; r0 < nreplicas; r0 += kSideChunk) {
    const int nr = (int)std::min<int64_t>(kSideChunk, nreplicas - r0);
    ScaleArgs S;
    for (int r = 0; r < kSideChunk; ++r)
      for (int k = 0; k < 3; ++k) S.s[r][k] = r < nr ? scale_host[3 * (r0 + r) + k] : 1.0;
    hipLaunchKernelGGL((rescale_molecules_kernel<R>), dim3((unsigned)small, (unsigned)nr), dim3(kThreads), 0, st, n, nmol, off, mem,
                       (const int *)big, (R *)pos, (R *)vel, (const R *)mass, S, (int)r0, partials, prows, 0);
    if (has_big)
      hipLaunchKernelGGL((rescale_molecules_kernel<R>), dim3((unsigned)kBigBlocks, (unsigned)nr), dim3(kWave), 0, st, n, nmol, off, mem,
                         (const int *)big, (R *)pos, (R *)vel, (const R *)mass, S, (int)r0, partials, prows, 1);
  }
  hipLaunchKernelGGL(rescale_fold_kernel, dim3((unsigned)nreplicas), dim3(64), 0, st, (const double *)partials, prows,
                     has_big ? prows : small, record);
  TMD_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_rescale_molecules_workspace(int64_t nreplicas, int64_t nmol, int64_t *record_doubles, int64_t *partials_doubles) {
  if (nreplicas <= 0 || nreplicas > 65535) return fail("tmdhip_rescale_molecules_workspace: nreplicas must lie in 1 .. 65535");
  if (nmol <= 0 || nmol > INT32_MAX / 4) return fail("tmdhip_rescale_molecules_workspace: nmol must be positive (and fit 32-bit indices)");
  if (record_doubles) *record_doubles = nreplicas * 2;
  if (partials_doubles) *partials_doubles = nreplicas * partial_rows(nmol) * 2 + (nmol + 1 + 1) / 2;
  return 0;
}

int tmdhip_rescale_molecules(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *vel_dev, const void *mass_dev,
                             const double *scale_host, int32_t nmol, const int32_t *offsets_dev, const int32_t *members_dev,
                             int32_t has_big, double *record_dev, double *partials_dev, void *stream) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail("tmdhip_rescale_molecules: bad dtype");
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > 65535 || natoms > INT32_MAX / 4)
    return fail("tmdhip_rescale_molecules: nreplicas must lie in 1 .. 65535 and natoms must be positive (and fit 32-bit indices)");
  if (nmol <= 0 || nmol > natoms) return fail("tmdhip_rescale_molecules: the number of molecules must lie in 1 .. natoms");
  if (!pos_dev || !vel_dev || !mass_dev || !scale_host || !offsets_dev || !members_dev || !record_dev || !partials_dev)
    return fail("tmdhip_rescale_molecules: null pointer");
  if (pos_dev == vel_dev) return fail("tmdhip_rescale_molecules: vel_dev must not alias pos_dev");
  for (int64_t k = 0; k < 3 * nreplicas; ++k)
    if (!(scale_host[k] > 0.0) || !std::isfinite(scale_host[k])) return fail("tmdhip_rescale_molecules: scale factors must be positive and finite");
  hipStream_t st = (hipStream_t)stream;
  return dtype == TMDHIP_F32 ? rescale<float>(nreplicas, (int)natoms, pos_dev, vel_dev, mass_dev, scale_host, nmol, offsets_dev, members_dev,
                                              has_big != 0, record_dev, partials_dev, st)
                             : rescale<double>(nreplicas, (int)natoms, pos_dev, vel_dev, mass_dev, scale_host, nmol, offsets_dev,
                                               members_dev, has_big != 0, record_dev, partials_dev, st);
}

}  // extern "C"
