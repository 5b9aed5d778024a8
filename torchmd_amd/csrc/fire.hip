// FIRE energy minimisation (Bitzek et al., PRL 97, 170201, 2006) for gfx950: one iteration of every replica from forces
// that are already in memory.  Stateless (no tmdhip_ctx); the per-replica state lives in device memory, so a caller can
// enqueue force evaluation + tmdhip_fire_step hundreds of times without a host synchronisation.
//
// Two launches per iteration, blockIdx.y = replica:
//   fire_reduce_kernel  per block: max |F_i|^2, sum F.v, sum v.v, sum F.F over its atoms with mass > 0 -> partials[r][block][4]
//   fire_update_kernel  wave 0 of every block folds the partials of its replica (so all blocks see the same bits), derives the
//                       new state from the state slot `iteration & 1`, moves its atoms; thread 0 of block 0 stores the new
//                       state into the other slot.  No block can read a half-written state.
// Fixed-order sum (reduce.h), the wave sums meet in sequence (the maxima pairwise: any order gives the same bits).
// All sums and all state arithmetic in double in both precisions, contraction off, one rounding on the store of vel and pos.
// Rows with mass == 0 (virtual sites) are neither read into a sum nor written.  A replica whose state says `done` is not
// written at all (its state is copied to the other slot), so its positions stay bit for bit those at convergence.
// Streaming and HBM-bound: in fp32 the two passes read F, v and m twice and x once (68 B/atom) and write v and x (24 B/atom).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "pair_math.h"

using namespace tmd;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = TMDHIP_FIRE_MAX_BLOCKS;  // reduction blocks per replica = rows of partials per replica
constexpr int kSlot = TMDHIP_FIRE_STATE_DOUBLES;
enum { S_DT = 0, S_ALPHA, S_NPOS, S_DONE, S_ITER, S_FMAX, S_NUPHILL, S_RESERVED };

__global__ void fire_init_kernel(int nreplicas, double *__restrict__ state, double dt, double alpha) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nreplicas) return;
  for (int slot = 0; slot < 2; ++slot) {
    double *s = state + ((size_t)r * 2 + slot) * kSlot;
    for (int k = 0; k < kSlot; ++k) s[k] = 0.0;
    s[S_DT] = dt;
    s[S_ALPHA] = alpha;
  }
}

template <typename R>
__global__ __launch_bounds__(kThreads) void fire_reduce_kernel(int natoms, const R *__restrict__ vel, const R *__restrict__ frc,
                                                               const R *__restrict__ mass, const double *__restrict__ state,
                                                               double *__restrict__ partials, int slot) {
#pragma clang fp contract(off)
  const int r = blockIdx.y;
  if (state[((size_t)r * 2 + slot) * kSlot + S_DONE] != 0.0) return;  // (the update pass does not read the partials then)
  const R *v = vel + (size_t)r * natoms * 3, *f = frc + (size_t)r * natoms * 3;
  double f2max[1] = {0}, s[3] = {0, 0, 0};  // F.v, v.v, F.F
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < natoms; i += gridDim.x * kThreads) {
    if (!(mass[i] > R(0))) continue;
    const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
    const double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    const double f2 = fx * fx + fy * fy + fz * fz;
    f2max[0] = fmax(f2max[0], f2);
    s[0] += fx * vx + fy * vy + fz * vz;
    s[1] += vx * vx + vy * vy + vz * vz;
    s[2] += f2;
  }
  double *out = partials + ((size_t)r * kMaxBlocks + blockIdx.x) * 4;
  block_sums<kThreads / 64, Meet::Pairwise, 1, Max>(f2max, out);
  block_sums<kThreads / 64, Meet::Sequential>(s, out + 1);
}

// what every thread of a block needs from the new state
struct Move {
  double dt, keep, mix;  // v <- keep * v + mix * F  (P <= 0: keep = mix = 0), then the Euler step with dt
  int frozen;            // done before, or converged now: nothing moves
};

template <typename R>
__global__ __launch_bounds__(kThreads) void fire_update_kernel(int natoms, R *__restrict__ pos, R *__restrict__ vel,
                                                               const R *__restrict__ frc, const R *__restrict__ mass,
                                                               double *__restrict__ state, const double *__restrict__ partials,
                                                               int nblocks, tmdhip_fire_params prm, int slot) {
#pragma clang fp contract(off)
  const int r = blockIdx.y;
  const double *in = state + ((size_t)r * 2 + slot) * kSlot;
  double *out = state + ((size_t)r * 2 + (slot ^ 1)) * kSlot;
  __shared__ Move mv;
  if (threadIdx.x < 64) {  // wave 0: the same order of additions in every block
    double s[kSlot];
#pragma unroll
    for (int k = 0; k < kSlot; ++k) s[k] = in[k];
    Move m;
    m.dt = s[S_DT], m.keep = 0, m.mix = 0, m.frozen = 1;
    if (s[S_DONE] == 0.0) {
      const double *rows = partials + (size_t)r * kMaxBlocks * 4;
      double f2max[1] = {0}, sum[3] = {0, 0, 0};
      fold_into<4, Max, Sum>(f2max, rows, sum, rows + 1, nblocks);
      const double p = wave_sum(sum[0]), vv = wave_sum(sum[1]), ff = wave_sum(sum[2]);
      s[S_FMAX] = sqrt(wave_max(f2max[0]));
      if (s[S_FMAX] < prm.f_tol) {
        s[S_DONE] = 1.0;
      } else {
        m.frozen = 0;
        if (p > 0.0) {
          m.keep = 1.0 - s[S_ALPHA];
          m.mix = s[S_ALPHA] * sqrt(vv / ff);
          s[S_NPOS] += 1.0;
          if (s[S_NPOS] > (double)prm.n_min) {
            s[S_DT] = fmin(s[S_DT] * prm.f_inc, prm.dt_max);
            s[S_ALPHA] = s[S_ALPHA] * prm.f_alpha;
          }
        } else {
          s[S_DT] = s[S_DT] * prm.f_dec;
          s[S_ALPHA] = prm.alpha_start;
          s[S_NPOS] = 0.0;
          s[S_NUPHILL] += 1.0;
        }
        s[S_ITER] += 1.0;
        m.dt = s[S_DT];
      }
    }
    if (threadIdx.x == 0) {
      mv = m;
      if (blockIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kSlot; ++k) out[k] = s[k];
      }
    }
  }
  __syncthreads();
  const Move m = mv;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (m.frozen || i >= natoms) return;
  const double ms = mass[i];
  if (!(ms > 0.0)) return;
  const size_t o = ((size_t)r * natoms + i) * 3;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = frc[o + k];
    v[k] = m.keep * (double)vel[o + k] + m.mix * f;
    v[k] = v[k] + (m.dt * f) / ms;
  }
  const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (vn * m.dt > prm.max_step) {
    const double c = (prm.max_step / m.dt) / vn;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = v[k] * c;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pos[o + k] = (R)((double)pos[o + k] + m.dt * v[k]);
    vel[o + k] = (R)v[k];
  }
}

int check_params(const char *who, const tmdhip_fire_params *p) {
  if (!p) return fail(std::string(who) + ": null parameters");
  if (p->struct_size != (int32_t)sizeof(tmdhip_fire_params)) return fail(std::string(who) + ": tmdhip_fire_params size mismatch (ABI)");
  if (!(p->f_tol > 0) || !(p->dt_start > 0) || !(p->dt_max >= p->dt_start) || !(p->max_step > 0) || p->n_min < 0 || !(p->f_inc >= 1) ||
      !(p->f_dec > 0 && p->f_dec < 1) || !(p->alpha_start > 0 && p->alpha_start <= 1) || !(p->f_alpha > 0 && p->f_alpha <= 1))
    return fail(std::string(who) + ": need f_tol > 0, 0 < dt_start <= dt_max, max_step > 0, n_min >= 0, f_inc >= 1, 0 < f_dec < 1, "
                                   "0 < alpha_start <= 1, 0 < f_alpha <= 1");
  return 0;
}

}  // namespace

extern "C" {

int tmdhip_fire_init(int64_t nreplicas, double *state_dev, const tmdhip_fire_params *params, void *stream) {
  TMD_TRY(check_params("tmdhip_fire_init", params));
  if (nreplicas <= 0 || nreplicas > 65535) return fail("tmdhip_fire_init: nreplicas must lie in 1 .. 65535");
  if (!state_dev) return fail("tmdhip_fire_init: null pointer");
  hipLaunchKernelGGL(fire_init_kernel, dim3((unsigned)((nreplicas + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (int)nreplicas,
                     state_dev, params->dt_start, params->alpha_start);
  TMD_HIP(hipGetLastError());
  return 0;
}

int tmdhip_fire_step(int dtype, int64_t nreplicas, int64_t natoms, void *pos_dev, void *vel_dev, const void *forces_dev,
                     const void *mass_dev, double *state_dev, double *partials_dev, const tmdhip_fire_params *params,
                     int64_t iteration, void *stream) {
  if (dtype != TMDHIP_F32 && dtype != TMDHIP_F64) return fail("tmdhip_fire_step: bad dtype");
  TMD_TRY(check_params("tmdhip_fire_step", params));
  if (nreplicas <= 0 || natoms <= 0 || nreplicas > 65535 || natoms > INT32_MAX / 4)
    return fail("tmdhip_fire_step: nreplicas must lie in 1 .. 65535 and natoms must be positive (and fit 32-bit indices)");
  if (iteration < 0) return fail("tmdhip_fire_step: negative iteration");
  if (!pos_dev || !vel_dev || !forces_dev || !mass_dev || !state_dev || !partials_dev) return fail("tmdhip_fire_step: null pointer");
  const int n = (int)natoms, slot = (int)(iteration & 1);
  const int nupdate = (n + kThreads - 1) / kThreads, nreduce = std::min(nupdate, kMaxBlocks);
  const dim3 gr((unsigned)nreduce, (unsigned)nreplicas), gu((unsigned)nupdate, (unsigned)nreplicas), block(kThreads);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TMDHIP_F32) {
    hipLaunchKernelGGL(fire_reduce_kernel<float>, gr, block, 0, st, n, (const float *)vel_dev, (const float *)forces_dev,
                       (const float *)mass_dev, state_dev, partials_dev, slot);
    hipLaunchKernelGGL(fire_update_kernel<float>, gu, block, 0, st, n, (float *)pos_dev, (float *)vel_dev, (const float *)forces_dev,
                       (const float *)mass_dev, state_dev, partials_dev, nreduce, *params, slot);
  } else {
    hipLaunchKernelGGL(fire_reduce_kernel<double>, gr, block, 0, st, n, (const double *)vel_dev, (const double *)forces_dev,
                       (const double *)mass_dev, state_dev, partials_dev, slot);
    hipLaunchKernelGGL(fire_update_kernel<double>, gu, block, 0, st, n, (double *)pos_dev, (double *)vel_dev, (const double *)forces_dev,
                       (const double *)mass_dev, state_dev, partials_dev, nreduce, *params, slot);
  }
  TMD_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
