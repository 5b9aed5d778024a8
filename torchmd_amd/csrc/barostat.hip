// Monte Carlo barostat move for gfx950: scale the centre of every molecule, move the molecule rigidly.
//
// A trial volume change of the Monte Carlo barostat (Chow & Ferguson 1995; Aqvist et al. 2004) multiplies the box
// edges of replica r by s_r and moves every bonded group so that its centre c (unweighted mean of its atoms, the
// centre tmdhip_wrap uses) goes to s_r * c: every atom of the group is translated by (s_r - 1) * c.  Distances inside
// a group do not change, so constrained bond lengths survive the move.  Molecules must be whole (not split across
// the periodic boundary): the mean of a split group is not its centre.  That holds for what Wrapper.wrap leaves
// and for unwrapped trajectories.
//
// Work decomposition as in wrap_groups_kernel (integrator.hip): one thread per group of up to 64 atoms, one wave
// per larger group (second launch, only when such groups exist), blockIdx.y = replica.  The centre is accumulated
// in double in both precisions (an fp32 mean of 3 000 coordinates of magnitude 50 A is good to ~1e-4 A only, which
// the energy difference of the move would see), members in index order, no atomics: two calls give the same bits.
// The kernel that moves a group also writes its atoms' previous positions to `saved` (the copy a rejected move is
// restored from), so no separate copy launch is needed.  A replica whose three scale factors are exactly 1 is only
// copied to `saved`, never rewritten.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "pair_math.h"

using namespace tmd;

namespace {

constexpr int kScaleReplicas = 16;  // replicas served by one launch (their scale factors travel as kernel arguments)
constexpr int kBigGroup = 64;

struct ScaleArgs {
  double s[kScaleReplicas][3];
};

template <typename R>
__global__ void scale_groups_kernel(int64_t natoms, int ngroups, const int *__restrict__ goff, const int *__restrict__ gmem,
                                    R *__restrict__ pos, R *__restrict__ saved, ScaleArgs S, int replica0, int big_pass) {
  const int rl = blockIdx.y;
  const size_t base = (size_t)(replica0 + rl) * (size_t)natoms * 3;
  R *p = pos + base;
  R *q = saved ? saved + base : nullptr;
  const double ax = S.s[rl][0] - 1.0, ay = S.s[rl][1] - 1.0, az = S.s[rl][2] - 1.0;
  const bool move = ax != 0.0 || ay != 0.0 || az != 0.0;
  if (!move && !q) return;
  int s, e, first, stride;
  if (!big_pass) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    s = goff[g], e = goff[g + 1];
    if (e - s > kBigGroup) return;
    first = s, stride = 1;
  } else {  // one wave per group: every exit up to the wave sum is taken by all 64 lanes together
    s = goff[blockIdx.x], e = goff[blockIdx.x + 1];
    if (e - s <= kBigGroup) return;
    first = s + (int)threadIdx.x, stride = kWave;
  }
  if (e <= s) return;
  double sx = 0, sy = 0, sz = 0;
  if (move) {
    for (int k = first; k < e; k += stride) {
      const int a = gmem[k];
      if ((unsigned)a >= (unsigned)natoms) continue;
      sx += (double)p[3 * a], sy += (double)p[3 * a + 1], sz += (double)p[3 * a + 2];
    }
    if (big_pass) sx = wave_sum(sx), sy = wave_sum(sy), sz = wave_sum(sz);
  }
  const double n = (double)(e - s);
  const double dx = ax * (sx / n), dy = ay * (sy / n), dz = az * (sz / n);
  for (int k = first; k < e; k += stride) {
    const int a = gmem[k];
    if ((unsigned)a >= (unsigned)natoms) continue;
    const R x = p[3 * a], y = p[3 * a + 1], z = p[3 * a + 2];
    if (q) q[3 * a] = x, q[3 * a + 1] = y, q[3 * a + 2] = z;
    if (move) {
      p[3 * a] = (R)((double)x + dx);
      p[3 * a + 1] = (R)((double)y + dy);
      p[3 * a + 2] = (R)((double)z + dz);
    }
  }
}

template <typename R>
int scale_groups(int64_t nreplicas, int64_t natoms, void *pos, void *saved, const double *scale_host, int32_t ngroups,
                 const int32_t *goff, const int32_t *gmem, int32_t has_big, hipStream_t st) {
  for (int64_t r0 = 0; r0 < nreplicas; r0 += kScaleReplicas) {
    const int nr = (int)std::min<int64_t>(kScaleReplicas, nreplicas - r0);
    ScaleArgs S;
    for (int r = 0; r < kScaleReplicas; ++r)
      for (int k = 0; k < 3; ++k) S.s[r][k] = r < nr ? scale_host[3 * (r0 + r) + k] : 1.0;
    hipLaunchKernelGGL((scale_groups_kernel<R>), dim3((unsigned)((ngroups + 255) / 256), (unsigned)nr), dim3(256), 0, st, natoms,
                       ngroups, goff, gmem, (R *)pos, (R *)saved, S, (int)r0, 0);
    if (has_big)
      hipLaunchKernelGGL((scale_groups_kernel<R>), dim3((unsigned)ngroups, (unsigned)nr), dim3(kWave), 0, st, natoms, ngroups,
                         goff, gmem, (R *)pos, (R *)saved, S, (int)r0, 1);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int tmdhip_scale_groups(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *saved_pos_dev,
                                   const double *scale_host, int32_t ngroups, const int32_t *group_offsets_dev,
                                   const int32_t *group_members_dev, int32_t has_big_groups, void *stream) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail("tmdhip_scale_groups: bad dtype");
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > INT32_MAX / 2 || natoms > INT32_MAX / 4)
    return fail("tmdhip_scale_groups: nreplicas and natoms must be positive (and fit 32-bit indices)");
  if (!pos_dev || !scale_host || !group_offsets_dev || !group_members_dev || ngroups <= 0 || ngroups > natoms)
    return fail("tmdhip_scale_groups: null pointer or bad group count");
  if (pos_dev == saved_pos_dev) return fail("tmdhip_scale_groups: saved_pos_dev must not alias pos_dev");
  for (int64_t k = 0; k < 3 * nreplicas; ++k)
    if (!(scale_host[k] > 0.0) || !(scale_host[k] < 1e6)) return fail("tmdhip_scale_groups: scale factors must be positive and finite");
  hipStream_t st = (hipStream_t)stream;
  return dtype == TMDHIP_F32 ? scale_groups<float>(nreplicas, natoms, pos_dev, saved_pos_dev, scale_host, ngroups, group_offsets_dev,
                                                   group_members_dev, has_big_groups, st)
                             : scale_groups<double>(nreplicas, natoms, pos_dev, saved_pos_dev, scale_host, ngroups,
                                                    group_offsets_dev, group_members_dev, has_big_groups, st);
}
