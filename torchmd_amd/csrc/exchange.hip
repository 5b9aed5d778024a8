// Velocity rescaling by one given factor per replica, with the kinetic-energy book-keeping of the rescaling, for gfx950: the
// device half of temperature replica exchange (Sugita & Okamoto, Chem. Phys. Lett. 314, 141, 1999), where two replica slots that
// trade rungs of a temperature ladder have their velocities scaled by sqrt(T_new / T_old).  The Metropolis decision is the
// host's (exchange.py); this file knows nothing of temperatures.  Stateless (no tmdhip_ctx): applied between two tmdhip_md_run
// calls to velocities that are in memory; the factors come from the host, so nothing is read back.
//
// Two launches per application, blockIdx.y = replica (the shape of thermostat.hip):
//   exchange_reduce_kernel  per block: sum m v^2 over its atoms with mass > 0 -> partials[r][block]
//   exchange_update_kernel  every thread writes v <- factor v for its atom; wave 0 of block 0 folds the partials of its replica
//                           and its thread 0 writes the replica's record.  (The factor is given, not derived from the sum as
//                           the thermostat's alpha is, so no other block needs the sum.)
// Fixed-order sum (reduce.h), the wave sums meet in sequence.  The sum and the record arithmetic in double in both precisions,
// contraction off; the new velocity is one IEEE product in double and one rounding on the store.
//
// Edge cases:
//   factor == 1.0 exactly                 reduced and recorded (K_after = K_before), the velocities are not written at all
//   rows with mass == 0 (virtual sites)   never read into a sum, never written: they keep their bits, NaNs included
// The factors travel as kernel arguments, kSideChunk replicas per pair of launches (as tmdhip_thermostat_apply passes its
// parameters): no device parameter array, no host-to-device copy.
// Streaming and HBM-bound: in fp32 the two passes read v and m twice (16 B/atom each) and write v (12 B/atom).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "pair_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = TMDHIP_EXCHANGE_MAX_BLOCKS;  // reduction blocks per replica = partials per replica
constexpr int kRec = TMDHIP_EXCHANGE_RECORD_DOUBLES;
enum { R_KBEFORE = 0, R_FACTOR, R_KAFTER, R_WORK, R_COUNT };

struct ChunkArgs {
  double factor[kSideChunk];
};

template <typename R>
__global__ __launch_bounds__(kThreads) void exchange_reduce_kernel(int natoms, const R *__restrict__ vel, const R *__restrict__ mass,
                                                                   double *__restrict__ partials, int replica0) {
#pragma clang fp contract(off)
  const int r = replica0 + blockIdx.y;
  const R *v = vel + (size_t)r * natoms * 3;
  double sum = 0.0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < natoms; i += gridDim.x * kThreads) {
    const double m = mass[i];
    if (!(m > 0.0)) continue;
    const double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    sum += m * (vx * vx + vy * vy + vz * vz);
  }
  const double lane[1] = {sum};
  block_sums<kThreads / 64, Meet::Sequential>(lane, partials + (size_t)r * kMaxBlocks + blockIdx.x);
}

template <typename R>
__global__ __launch_bounds__(kThreads) void exchange_update_kernel(int natoms, R *__restrict__ vel, const R *__restrict__ mass,
                                                                   const double *__restrict__ partials, int nblocks,
                                                                   double *__restrict__ record, ChunkArgs A, int replica0) {
#pragma clang fp contract(off)
  const int r = replica0 + blockIdx.y;
  const double factor = A.factor[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x < 64) {  // wave 0 of block 0: the record (no other block needs the sum)
    double sum[1];
    fold_rows(partials + (size_t)r * kMaxBlocks, nblocks, sum);
    if (threadIdx.x == 0) {
      double *rec = record + (size_t)r * kRec;
      const double K = 0.5 * sum[0];
      const double after = (factor * factor) * K;
      rec[R_KBEFORE] = K;
      rec[R_FACTOR] = factor;
      rec[R_KAFTER] = after;
      rec[R_WORK] = rec[R_WORK] + (after - K);
      rec[R_COUNT] = rec[R_COUNT] + 1.0;
    }
  }
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (factor == 1.0 || i >= natoms) return;
  if (!(mass[i] > R(0))) return;
  const size_t o = ((size_t)r * natoms + i) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) vel[o + k] = (R)(factor * (double)vel[o + k]);
}

template <typename R>
int rescale(int64_t nreplicas, int n, void *vel, const void *mass, const double *factor, double *record, double *partials,
            hipStream_t st) {
  const int nupdate = (n + kThreads - 1) / kThreads, nreduce = std::min(nupdate, kMaxBlocks);
  for (int64_t r0 = 0; r0 < nreplicas; r0 += kSideChunk) {
    const int nr = (int)std::min<int64_t>(kSideChunk, nreplicas - r0);
    ChunkArgs A;
    for (int r = 0; r < kSideChunk; ++r) A.factor[r] = r < nr ? factor[r0 + r] : 1.0;
    hipLaunchKernelGGL(exchange_reduce_kernel<R>, dim3((unsigned)nreduce, (unsigned)nr), dim3(kThreads), 0, st, n, (const R *)vel,
                       (const R *)mass, partials, (int)r0);
    hipLaunchKernelGGL(exchange_update_kernel<R>, dim3((unsigned)nupdate, (unsigned)nr), dim3(kThreads), 0, st, n, (R *)vel,
                       (const R *)mass, (const double *)partials, nreduce, record, A, (int)r0);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_velocity_rescale_workspace(int64_t nreplicas, int64_t *record_doubles, int64_t *partials_doubles) {
  if (nreplicas <= 0 || nreplicas > 65535) return fail("tmdhip_velocity_rescale_workspace: nreplicas must lie in 1 .. 65535");
  if (record_doubles) *record_doubles = nreplicas * kRec;
  if (partials_doubles) *partials_doubles = nreplicas * kMaxBlocks;
  return 0;
}

int tmdhip_velocity_rescale(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev, const void *mass_dev,
                            const double *factor_host, double *record_dev, double *partials_dev, void *stream) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail("tmdhip_velocity_rescale: bad dtype");
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > 65535 || natoms > INT32_MAX / 4)
    return fail("tmdhip_velocity_rescale: nreplicas must lie in 1 .. 65535 and natoms must be positive (and fit 32-bit indices)");
  if (!vel_dev || !mass_dev || !factor_host || !record_dev || !partials_dev) return fail("tmdhip_velocity_rescale: null pointer");
  for (int64_t r = 0; r < nreplicas; ++r)
    if (!(factor_host[r] > 0.0) || !std::isfinite(factor_host[r]))
      return fail("tmdhip_velocity_rescale: need a finite factor > 0 for every replica");
  hipStream_t st = (hipStream_t)stream;
  return dtype == TMDHIP_F32 ? rescale<float>(nreplicas, (int)natoms, vel_dev, mass_dev, factor_host, record_dev, partials_dev, st)
                             : rescale<double>(nreplicas, (int)natoms, vel_dev, mass_dev, factor_host, record_dev, partials_dev, st);
}

}  // extern "C"
