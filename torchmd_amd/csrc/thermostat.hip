// Stochastic velocity rescaling (Bussi, Donadio & Parrinello, J. Chem. Phys. 126, 014101, 2007; GROMACS' v-rescale) with one
// target temperature per replica, and centre-of-mass motion removal, for gfx950.  Stateless (no tmdhip_ctx): applied between two
// tmdhip_md_run calls to velocities that are in memory.  The random numbers of an application (R1, S) come from the host, so it
// depends on no device state and needs no host synchronisation.
//
// Two launches per application, blockIdx.y = replica:
//   thermostat_reduce_kernel  per block: sum m, sum m vx, sum m vy, sum m vz, sum m v^2 over its atoms with mass > 0
//                             -> partials[r][block][5]
//   thermostat_update_kernel  wave 0 of every block folds the partials of its replica (all blocks see the same bits), derives
//                             V_cm, K and alpha (thermostat_math.h) and hands them to the block through LDS; every thread
//                             writes v <- alpha (v - V_cm) for its atom; thread 0 of block 0 writes the replica's record.
// Fixed-order sum (reduce.h), the wave sums meet in sequence.  All sums and all state arithmetic in double in both precisions,
// contraction off, one rounding on the store of v.
//
// Edge cases:
//   K = 0 (all velocities equal V_cm, or zero)   alpha = 1: nothing is scaled (V_cm is still taken out when asked for)
//   c = 1 and remove_com off                     alpha = 1 and V_cm = 0: the replica's velocities are not written at all
//                                                (its record is)
//   rows with mass == 0 (virtual sites)          never read into a sum, never written: they keep their bits, NaNs included
//   active[r] == 0                               replica r is skipped: neither its velocities nor its record are touched
// The per-replica parameters travel as kernel arguments, kSideChunk replicas per pair of launches (as tmdhip_scale_groups passes its
// scale factors): no device parameter array, no host-to-device copy.
// Streaming and HBM-bound: in fp32 the two passes read v and m twice (16 B/atom each) and write v (12 B/atom).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "common.h"
#include "pair_math.h"
#include "thermostat_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = TMDHIP_THERMOSTAT_MAX_BLOCKS;  // reduction blocks per replica = rows of partials per replica
constexpr int kRec = TMDHIP_THERMOSTAT_RECORD_DOUBLES;
constexpr int kSums = 5;
enum { R_KBEFORE = 0, R_ALPHA, R_KAFTER, R_VCM, R_HEAT, R_COUNT };

struct ChunkArgs {
  double kbar[kSideChunk], nf[kSideChunk], c[kSideChunk], r1[kSideChunk], s[kSideChunk];
  int active[kSideChunk];
};

template <typename R>
__global__ __launch_bounds__(kThreads) void thermostat_reduce_kernel(int natoms, const R *__restrict__ vel, const R *__restrict__ mass,
                                                                     double *__restrict__ partials, ChunkArgs A, int replica0) {
#pragma clang fp contract(off)
  if (!A.active[blockIdx.y]) return;  // (the update pass does not read the partials then)
  const int r = replica0 + blockIdx.y;
  const R *v = vel + (size_t)r * natoms * 3;
  double sum[kSums] = {0, 0, 0, 0, 0};
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < natoms; i += gridDim.x * kThreads) {
    const double m = mass[i];
    if (!(m > 0.0)) continue;
    const double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    sum[0] += m;
    sum[1] += m * vx;
    sum[2] += m * vy;
    sum[3] += m * vz;
    sum[4] += m * (vx * vx + vy * vy + vz * vz);
  }
  block_sums<kThreads / 64, Meet::Sequential>(sum, partials + ((size_t)r * kMaxBlocks + blockIdx.x) * kSums);
}

// what every thread of a block needs
struct Scale {
  double alpha, vcm[3];
  int write;
};

template <typename R>
__global__ __launch_bounds__(kThreads) void thermostat_update_kernel(int natoms, R *__restrict__ vel, const R *__restrict__ mass,
                                                                     const double *__restrict__ partials, int nblocks,
                                                                     double *__restrict__ record, ChunkArgs A, int replica0,
                                                                     int remove_com) {
#pragma clang fp contract(off)
  const int rl = blockIdx.y;
  if (!A.active[rl]) return;
  const int r = replica0 + rl;
  __shared__ Scale sc;
  if (threadIdx.x < 64) {  // wave 0: the same order of additions in every block
    double sum[kSums];
    fold_rows(partials + (size_t)r * kMaxBlocks * kSums, nblocks, sum);
    if (threadIdx.x == 0) {
      Scale s;
      const double K = csvr_kinetic(sum[0], sum[1], sum[2], sum[3], sum[4], remove_com, s.vcm);
      s.alpha = csvr_alpha(K, A.kbar[rl], A.nf[rl], A.c[rl], A.r1[rl], A.s[rl]);
      s.write = remove_com || A.c[rl] != 1.0;
      sc = s;
      if (blockIdx.x == 0) {
        double *rec = record + (size_t)r * kRec;
        const double after = (s.alpha * s.alpha) * K;
        rec[R_KBEFORE] = K;
        rec[R_ALPHA] = s.alpha;
        rec[R_KAFTER] = after;
        rec[R_VCM] = sqrt(s.vcm[0] * s.vcm[0] + s.vcm[1] * s.vcm[1] + s.vcm[2] * s.vcm[2]);
        rec[R_HEAT] = rec[R_HEAT] + (after - K);
        rec[R_COUNT] = rec[R_COUNT] + 1.0;
      }
    }
  }
  __syncthreads();
  const Scale s = sc;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (!s.write || i >= natoms) return;
  if (!(mass[i] > R(0))) return;
  const size_t o = ((size_t)r * natoms + i) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) vel[o + k] = (R)(s.alpha * ((double)vel[o + k] - s.vcm[k]));
}

template <typename R>
int apply(int64_t nreplicas, int n, void *vel, const void *mass, const double *kbar, const double *nf, const double *c,
          const double *r1, const double *s, const int32_t *active, int remove_com, double *record, double *partials, hipStream_t st) {
  const int nupdate = (n + kThreads - 1) / kThreads, nreduce = std::min(nupdate, kMaxBlocks);
  for (int64_t r0 = 0; r0 < nreplicas; r0 += kSideChunk) {
    const int nr = (int)std::min<int64_t>(kSideChunk, nreplicas - r0);
    ChunkArgs A;
    bool any = false;
    for (int r = 0; r < kSideChunk; ++r) {
      const bool in = r < nr;
      A.kbar[r] = in ? kbar[r0 + r] : 0.0, A.nf[r] = in ? nf[r0 + r] : 1.0, A.c[r] = in ? c[r0 + r] : 1.0;
      A.r1[r] = in ? r1[r0 + r] : 0.0, A.s[r] = in ? s[r0 + r] : 0.0;
      A.active[r] = in && (!active || active[r0 + r] != 0);
      any = any || A.active[r];
    }
    if (!any) continue;
    hipLaunchKernelGGL(thermostat_reduce_kernel<R>, dim3((unsigned)nreduce, (unsigned)nr), dim3(kThreads), 0, st, n, (const R *)vel,
                       (const R *)mass, partials, A, (int)r0);
    hipLaunchKernelGGL(thermostat_update_kernel<R>, dim3((unsigned)nupdate, (unsigned)nr), dim3(kThreads), 0, st, n, (R *)vel,
                       (const R *)mass, (const double *)partials, nreduce, record, A, (int)r0, remove_com);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_thermostat_workspace(int64_t nreplicas, int64_t *record_doubles, int64_t *partials_doubles) {
  if (nreplicas <= 0 || nreplicas > 65535) return fail("tmdhip_thermostat_workspace: nreplicas must lie in 1 .. 65535");
  if (record_doubles) *record_doubles = nreplicas * kRec;
  if (partials_doubles) *partials_doubles = nreplicas * kMaxBlocks * kSums;
  return 0;
}

int tmdhip_thermostat_apply(int dtype, int64_t nreplicas, int64_t natoms, void *vel_dev, const void *mass_dev,
                            const double *kbar_host, const double *ndof_host, const double *c_host, const double *r1_host,
                            const double *s_host, const int32_t *active_host, int32_t remove_com, double *record_dev,
                            double *partials_dev, void *stream) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail("tmdhip_thermostat_apply: bad dtype");
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > 65535 || natoms > INT32_MAX / 4)
    return fail("tmdhip_thermostat_apply: nreplicas must lie in 1 .. 65535 and natoms must be positive (and fit 32-bit indices)");
  if (!vel_dev || !mass_dev || !kbar_host || !ndof_host || !c_host || !r1_host || !s_host || !record_dev || !partials_dev)
    return fail("tmdhip_thermostat_apply: null pointer");
  for (int64_t r = 0; r < nreplicas; ++r) {
    if (active_host && !active_host[r]) continue;
    if (!(kbar_host[r] >= 0.0) || !std::isfinite(kbar_host[r]) || !(ndof_host[r] > 0.0) || !std::isfinite(ndof_host[r]) ||
        !(c_host[r] >= 0.0 && c_host[r] <= 1.0) || !std::isfinite(r1_host[r]) || !(s_host[r] >= 0.0) || !std::isfinite(s_host[r]))
      return fail("tmdhip_thermostat_apply: need finite kbar >= 0, ndof > 0, 0 <= c <= 1, finite r1 and s >= 0 for every active replica");
  }
  hipStream_t st = (hipStream_t)stream;
  return dtype == TMDHIP_F32 ? apply<float>(nreplicas, (int)natoms, vel_dev, mass_dev, kbar_host, ndof_host, c_host, r1_host, s_host,
                                            active_host, remove_com != 0, record_dev, partials_dev, st)
                             : apply<double>(nreplicas, (int)natoms, vel_dev, mass_dev, kbar_host, ndof_host, c_host, r1_host, s_host,
                                             active_host, remove_com != 0, record_dev, partials_dev, st);
}

}  // extern "C"
